// Random voices: RandomLatentConverter (five EqualLinear layers and one nn.Linear over a Gaussian row) as a chain of 1..16-row f32 GEMVs.
//   k_linear_rows<R> : out[r][n] = gain * act(sum_k x[r][k] * W[n][k] + bias[n]) for R rows at once.  A wave owns one output channel: lane l
//                      takes the 16-byte chunks l, l + 64, l + 128, .. of W's row n straight into registers (the weight is streamed once and shared
//                      by no other wave, so LDS would be a round trip for nothing; the loads are asynchronous until the first fmaf needs them), and
//                      every row accumulates against those registers; x is small (R * K floats) and comes through the caches.
//                      Order of one sum, whatever R is: per lane fmaf over its chunks in rising k, the four elements of a chunk in order, from 0.f;
//                      then the xor butterfly 32, 16, .. 1 over the wave; then + bias, the activation, * gain.  No atomics, no split K.
//                      A workgroup is four waves = four channels: N = 1024 gives 256 workgroups.
// Reference: tortoise_tts/models/random_latent_generator.py:10-52 (fused_leaky_relu, EqualLinear, RandomLatentConverter).
#include "ttk_common.h"
#include "ttk_host.h"

using namespace ttk;

namespace {

constexpr int LT = 256;            // threads of a workgroup
constexpr int LW = LT / 64;        // its waves = the output channels it owns
constexpr int kMaxRows = 16, kMaxK = 8192;

template <int R>
__global__ __launch_bounds__(LT) void k_linear_rows(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W, const float* __restrict__ bias, int K, int N,
													 int act, float slope, float gain, float* __restrict__ out, int64_t ldo) {
	const int lane = threadIdx.x & 63;
	const int n = blockIdx.x * LW + (threadIdx.x >> 6);
	if (n >= N) return;      // per wave; the kernel has no barrier
	const float4* w4 = (const float4*)(W + (int64_t)n * K);
	const int nv = K >> 2;
	float acc[R];
#pragma unroll
	for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 4
	for (int v = lane; v < nv; v += 64) {
		const float4 w = w4[v];
#pragma unroll
		for (int r = 0; r < R; ++r) {
			const float4 a = *(const float4*)(x + (int64_t)r * ldx + 4 * v);
			acc[r] = fmaf(a.x, w.x, acc[r]);
			acc[r] = fmaf(a.y, w.y, acc[r]);
			acc[r] = fmaf(a.z, w.z, acc[r]);
			acc[r] = fmaf(a.w, w.w, acc[r]);
		}
	}
#pragma unroll
	for (int r = 0; r < R; ++r)
		for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);      // a + b on both partners: every lane ends with the same bits
	float y = 0.f;
#pragma unroll
	for (int r = 0; r < R; ++r)
		if (lane == r) y = acc[r];
	if (lane < R) {
		y += bias ? bias[n] : 0.f;
		if (act == 1) y = y > 0.f ? y : y * slope;
		out[(int64_t)lane * ldo + n] = y * gain;
	}
}

int launch_linear_rows(const float* x, int64_t ldx, const float* W, const float* bias, int rows, int K, int N, int act, float slope, float gain, float* out, int64_t ldo,
					   hipStream_t s) {
	const dim3 grid((unsigned)((N + LW - 1) / LW));
	switch (rows) {
#define TTK_LINEAR_ROWS(RR) case RR: hipLaunchKernelGGL(k_linear_rows<RR>, grid, dim3(LT), 0, s, x, ldx, W, bias, K, N, act, slope, gain, out, ldo); break;
		TTK_LINEAR_ROWS(1) TTK_LINEAR_ROWS(2) TTK_LINEAR_ROWS(3) TTK_LINEAR_ROWS(4) TTK_LINEAR_ROWS(5) TTK_LINEAR_ROWS(6) TTK_LINEAR_ROWS(7) TTK_LINEAR_ROWS(8)
		TTK_LINEAR_ROWS(9) TTK_LINEAR_ROWS(10) TTK_LINEAR_ROWS(11) TTK_LINEAR_ROWS(12) TTK_LINEAR_ROWS(13) TTK_LINEAR_ROWS(14) TTK_LINEAR_ROWS(15) TTK_LINEAR_ROWS(16)
#undef TTK_LINEAR_ROWS
		default: TTK_REQUIRE(false, TTK_E_ARG, "ttk_linear_rows: rows = %d has no instantiation (1..%d)", rows, kMaxRows);
	}
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// the argument checks of ttk_linear_rows; `who` names the entry point in the message
int check_linear_rows(const char* who, const float* x, int64_t ldx, const float* W, const float* bias, int rows, int K, int N, int act, const float* out, int64_t ldo) {
	TTK_REQUIRE(x && W && out, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(x != out, TTK_E_ARG, "%s: x and out must be different buffers", who);
	TTK_REQUIRE(rows >= 1 && rows <= kMaxRows, TTK_E_ARG, "%s: rows = %d out of range (1..%d)", who, rows, kMaxRows);
	TTK_REQUIRE(K >= 4 && K <= kMaxK && K % 4 == 0, TTK_E_ARG, "%s: K = %d unsupported (a multiple of 4 in 4..%d)", who, K, kMaxK);
	TTK_REQUIRE(N >= 1, TTK_E_ARG, "%s: N = %d out of range (>= 1)", who, N);
	TTK_REQUIRE(act == 0 || act == 1, TTK_E_ARG, "%s: act = %d unknown (0 identity, 1 leaky-ReLU)", who, act);
	TTK_REQUIRE(ldx >= K && ldx % 4 == 0, TTK_E_ARG, "%s: ldx = %lld must be a multiple of 4 and >= K = %d (rows are read in 16-byte chunks)", who, (long long)ldx, K);
	TTK_REQUIRE(ldo >= N, TTK_E_ARG, "%s: ldo = %lld is below N = %d", who, (long long)ldo, N);
	TTK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)W & 15) == 0, TTK_E_ARG, "%s: x and W must be 16-byte aligned", who);
	TTK_REQUIRE(((uintptr_t)out & 3) == 0 && (!bias || ((uintptr_t)bias & 3) == 0), TTK_E_ARG, "%s: out and bias must be 4-byte aligned", who);
	return TTK_OK;
}

}  // namespace

struct ttk_rlg {
	ttk_rlg_config cfg;
	Arena arena;
	std::vector<float*> W, b;      // per layer: the effective [channels][channels] matrix and [channels] bias, as given
	float* act[2] = {nullptr, nullptr};      // ping-pong activations [max_rows][channels]
};

extern "C" {

int ttk_linear_rows(const float* x, int64_t ldx, const float* W, const float* bias, int rows, int K, int N, int act, float slope, float gain, float* out, int64_t ldo,
					void* stream) {
	TTK_TRY(check_linear_rows("ttk_linear_rows", x, ldx, W, bias, rows, K, N, act, out, ldo));
	return launch_linear_rows(x, ldx, W, bias, rows, K, N, act, slope, gain, out, ldo, (hipStream_t)stream);
}

int ttk_rlg_create(ttk_rlg** out, const ttk_rlg_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_rlg_create: null argument");
	const int C = cfg->channels;
	TTK_REQUIRE(C >= 4 && C <= kMaxK && C % 4 == 0, TTK_E_ARG, "ttk_rlg_create: channels %d unsupported (a multiple of 4 in 4..%d)", C, kMaxK);
	TTK_REQUIRE(cfg->n_layers >= 1 && cfg->n_layers <= 64, TTK_E_ARG, "ttk_rlg_create: n_layers %d out of range (1..64)", cfg->n_layers);
	TTK_REQUIRE(cfg->max_rows >= 1 && cfg->max_rows <= kMaxRows, TTK_E_ARG, "ttk_rlg_create: max_rows %d out of range (1..%d)", cfg->max_rows, kMaxRows);
	std::unique_ptr<ttk_rlg> h(new ttk_rlg());
	h->cfg = *cfg;
	WeightMap wm(w, n_w);
	h->W.resize(cfg->n_layers);
	h->b.resize(cfg->n_layers);
	for (int i = 0; i < cfg->n_layers; ++i) {
		const std::string p = "layers." + std::to_string(i) + ".";
		TTK_TRY(upload_f32(h->arena, wm, p + "weight", (int64_t)C * C, &h->W[i]));
		TTK_TRY(upload_f32(h->arena, wm, p + "bias", C, &h->b[i]));
	}
	for (int i = 0; i < 2; ++i) TTK_TRY(h->arena.alloc((void**)&h->act[i], (size_t)cfg->max_rows * C * sizeof(float)));
	*out = h.release();
	return TTK_OK;
}

int ttk_rlg_destroy(ttk_rlg* h) {
	if (!h) return TTK_OK;
	delete h;
	return TTK_OK;
}

int ttk_rlg_forward(ttk_rlg* h, const float* noise, int rows, float* out, void* stream) {
	TTK_REQUIRE(h && noise && out, TTK_E_ARG, "ttk_rlg_forward: null argument");
	TTK_REQUIRE(rows >= 1 && rows <= h->cfg.max_rows, TTK_E_ARG, "ttk_rlg_forward: rows = %d out of range (1..max_rows = %d)", rows, h->cfg.max_rows);
	TTK_REQUIRE(noise != out, TTK_E_ARG, "ttk_rlg_forward: noise and out must be different buffers");
	const int C = h->cfg.channels, L = h->cfg.n_layers;
	const float* x = noise;
	for (int i = 0; i < L; ++i) {
		const bool last = i == L - 1;
		float* y = last ? out : h->act[i & 1];
		TTK_TRY(check_linear_rows("ttk_rlg_forward", x, C, h->W[i], h->b[i], rows, C, C, last ? 0 : 1, y, C));
		TTK_TRY(launch_linear_rows(x, C, h->W[i], h->b[i], rows, C, C, last ? 0 : 1, h->cfg.slope, last ? 1.f : h->cfg.gain, y, C, (hipStream_t)stream));
		x = y;
	}
	return TTK_OK;
}

}  // extern "C"
