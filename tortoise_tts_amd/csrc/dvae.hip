// DiscreteVAE (models/dvae.py): mel -> mel codes (get_codebook_indices :239-246) and mel codes -> mel (decode :248-270).
//
// Reference: tortoise_tts/models/dvae.py -- Quantize :12-72, ResBlock :89-101, UpsampledConv :104-114, DiscreteVAE :116-219 in its default
// configuration (1-D, two stride-2 k = 3 layers, ReLU, no encoder norm, no transposed convs, no normalisation).
//
// Layout: channels-last rows.  Every convolution runs on the segment GEMM of gemm.hip through ttk_conv.h, in the handle's dtype, with f32
// output; the residual stream of the ResBlocks is f32.  No GEMM epilogue form was added:
//  - k_dvae_pack turns a GEMM's f32 rows [B * L][C] into the next layer's T-typed operand rows [B][Lp][ld] (columns >= C and rows >= L zero),
//    applying ReLU on the way where the layer has one, and writing the activated f32 rows back where they are needed as a residual.
//  - the stride-2 convolutions view the operand rows [Lp][ld] (Lp = L rounded up to even: the zero row above) as [Lp / 2][2 ld]: tap 0 is the
//    second half of view row m - 1, taps 1 and 2 the two halves of view row m -- three ordinary segments with lda = 2 ld.
//  - nearest x2 + conv3 is two output phases with weights folded in f32 at upload, written through the GEMM's output row stride like a transposed
//    convolution:  y[2m] = W0 x[m-1] + (W1 + W2) x[m],  y[2m+1] = (W0 + W1) x[m] + W2 x[m+1].  Half the products of the materialised form.
//  - k_dvae_gather: codes -> T-typed rows of the codebook, the operand of the decoder's first 1x1 convolution.
//
// Quantizer (k_dvae_quant + k_dvae_qcombine), f32 in EVERY handle dtype: the codes are ids, and a 16-bit distance GEMM over 8192 candidates whose
// best two are often closer than a 16-bit rounding step moves them; the convolutions before it may run in 16 bits, the argmin may not.
//   score[m][j] = |e_j|^2 - 2 z_m . e_j  (the reference's distance :31-35 less the row constant |z_m|^2), on v_mfma_f32_16x16x4_f32.
//   A workgroup of four waves owns 64 consecutive codes (kQuantCodes), a wave 16 of them: its B operand, 16 codes x D floats, is read from the
//   codebook ONCE into D / 4 registers per lane and stays there, so the 16 MB codebook streams through the chip once per row chunk.  The rows come
//   through LDS, 16 at a time (row stride D + 4 floats: the 16 lanes of a ds_read_b128 pass hit 16 distinct bank quads); step (s, i) of the k-loop
//   contracts k = 16 s + 4 g + i over the lane groups g -- A and B use the same map, so a lane's operands are contiguous float4s.  Two accumulators
//   take alternate steps (40-cycle dependent latency against a 32-cycle issue).  Per 16-row tile the lanes fold (score, index) over the tile's 16
//   codes, the waves over the workgroup's 64, and the workgroup writes one (score, index) pair per row; no [M][num_tokens] matrix exists.
//   k_dvae_qcombine folds the pairs of the num_tokens / 64 workgroups per row in index order.  Every fold takes the smaller score and, on equal
//   scores, the smaller index: the result does not depend on arrival order, there are no atomics.  A row of NaNs gets code 0.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ttk_common.h"
#include "ttk_conv.h"
#include "ttk_kernels.h"

using namespace ttk;

namespace {

constexpr int kQuantCodes = 64;        // codes of one k_dvae_quant workgroup (4 waves x one 16-code MFMA tile)
constexpr int kQuantRows = 128;        // rows of one workgroup along grid.y, at most (8 tiles of 16)

// mel f32 [B][C][T] -> T [B][Tp][ld], rows >= T and columns >= C zero
template <typename T>
__global__ void k_dvae_in(const float* mel, int C, int Tn, int Tp, T* out, int ld, int64_t total) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= total) return;
	const int c = (int)(idx % ld);
	const int64_t r = idx / ld;
	const int t = (int)(r % Tp);
	const int64_t b = r / Tp;
	out[idx] = cvt<T>(c < C && t < Tn ? mel[(b * C + c) * Tn + t] : 0.f);
}

// src f32 [B * L][C] -> dst T [B][Lp][ld] = relu?(src), rows >= L and columns >= C zero; keep (optional, may alias src): the activated f32 rows [B * L][C]
template <typename T>
__global__ void k_dvae_pack(const float* src, int C, int L, int Lp, int relu, float* keep, T* dst, int ld, int64_t total) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= total) return;
	const int c = (int)(idx % ld);
	const int64_t r = idx / ld;
	const int t = (int)(r % Lp);
	const int64_t b = r / Lp;
	float v = 0.f;
	if (c < C && t < L) {
		const int64_t i = (b * L + t) * C + c;
		v = src[i];
		if (relu) v = v < 0.f ? 0.f : v;        // NaN stays NaN, as in torch
		if (keep) keep[i] = v;
	}
	dst[idx] = cvt<T>(v);
}

// codes int64 [M] -> dst T [M][ld] = codebook rows (f32 [V][D]), columns >= D zero.  The host has checked the codes; the clamp keeps a read in range whatever arrives.
template <typename T>
__global__ void k_dvae_gather(const int64_t* codes, const float* cb, int V, int D, T* dst, int ld, int64_t total) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= total) return;
	const int c = (int)(idx % ld);
	const int64_t r = idx / ld;
	int64_t code = codes[r];
	code = code < 0 ? 0 : (code >= V ? V - 1 : code);
	dst[idx] = cvt<T>(c < D ? cb[code * D + c] : 0.f);
}

// embed f32 [D][V] -> cb f32 [V][D], e2[j] = sum_k cb[j][k]^2 (one thread per code, ascending k)
__global__ void k_dvae_codebook(const float* embed, int D, int V, float* cb, float* e2) {
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= V) return;
	float s = 0.f;
	for (int k = 0; k < D; ++k) {
		const float v = embed[(int64_t)k * V + j];
		cb[(int64_t)j * D + k] = v;
		s = fmaf(v, v, s);
	}
	e2[j] = s;
}

__device__ __forceinline__ void take_min(float& v, int& i, float v2, int i2) {
	if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// See the file header.  z f32 [M][D], cb f32 [V][D], e2 f32 [V].  Grid (ceil(V / 64), row chunks), 256 threads; workgroup (x, y) handles the 16-row tiles
// [y * tiles_per_chunk, (y + 1) * tiles_per_chunk) and writes pmin / pidx [x][M] for their rows.
template <int D>
__global__ __launch_bounds__(256) void k_dvae_quant(const float* __restrict__ z, int M, const float* __restrict__ cb, const float* __restrict__ e2, int V,
													int tiles_per_chunk, float* __restrict__ pmin, int* __restrict__ pidx) {
	constexpr int LDZ = D + 4, S = D / 16, D4 = D / 4;
	__shared__ __attribute__((aligned(16))) float zs[16 * LDZ];
	__shared__ float redv[4][16];
	__shared__ int redi[4][16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
	const int j = blockIdx.x * kQuantCodes + 16 * wave + l15;      // this lane's code
	const int jr = j < V ? j : V - 1;                              // the row it reads (in range; a code >= V is masked below)
	f32x4 bw[S];
#pragma unroll
	for (int s = 0; s < S; ++s) bw[s] = *(const f32x4*)(cb + (int64_t)jr * D + 16 * s + 4 * g);
	const float ej = e2[jr];
	const int mt_end = (M + 15) / 16;
	const int t0 = blockIdx.y * tiles_per_chunk, t1 = min(t0 + tiles_per_chunk, mt_end);
	for (int mt = t0; mt < t1; ++mt) {
		const int m0 = 16 * mt;
		__syncthreads();                                           // the previous tile's zs reads and red reads are done
		for (int e = threadIdx.x; e < 16 * D4; e += 256) {
			const int row = e / D4, c4 = e - row * D4;
			f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
			if (m0 + row < M) v = *(const f32x4*)(z + (int64_t)(m0 + row) * D + 4 * c4);
			*(f32x4*)(zs + row * LDZ + 4 * c4) = v;
		}
		__syncthreads();
		f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
		const float* zr = zs + l15 * LDZ + 4 * g;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const f32x4 a = *(const f32x4*)(zr + 16 * s);
			acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bw[s][0], acc0, 0, 0, 0);
			acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bw[s][1], acc1, 0, 0, 0);
			acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bw[s][2], acc0, 0, 0, 0);
			acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bw[s][3], acc1, 0, 0, 0);
		}
		// D[row 4 g + r][col l15]: row m0 + 4 g + r against code j
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			float v = j < V ? fmaf(-2.f, acc0[r] + acc1[r], ej) : INFINITY;
			int i = jr;
#pragma unroll
			for (int o = 1; o < 16; o <<= 1) {
				const float v2 = __shfl_xor(v, o);
				const int i2 = __shfl_xor(i, o);
				take_min(v, i, v2, i2);
			}
			if (l15 == 0) { redv[wave][4 * g + r] = v; redi[wave][4 * g + r] = i; }
		}
		__syncthreads();
		if (threadIdx.x < 16 && m0 + (int)threadIdx.x < M) {
			float v = redv[0][threadIdx.x];
			int i = redi[0][threadIdx.x];
#pragma unroll
			for (int w = 1; w < 4; ++w) take_min(v, i, redv[w][threadIdx.x], redi[w][threadIdx.x]);
			pmin[(int64_t)blockIdx.x * M + m0 + threadIdx.x] = v;
			pidx[(int64_t)blockIdx.x * M + m0 + threadIdx.x] = i;
		}
	}
}

// codes[m] = the index of the smallest pmin[w][m] over the nw workgroups, the smaller index on equal scores
__global__ void k_dvae_qcombine(const float* pmin, const int* pidx, int nw, int M, int64_t* codes) {
	const int m = blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= M) return;
	float v = pmin[m];
	int i = pidx[m];
	for (int w = 1; w < nw; ++w) take_min(v, i, pmin[(int64_t)w * M + m], pidx[(int64_t)w * M + m]);
	codes[m] = i;
}

struct Res { Mat c0, c2, c4; };     // ResBlock.net.0 (k 3), .2 (k 3), .4 (k 1)

}  // namespace

struct ttk_dvae {
	ttk_dvae_config cfg;
	int dt;
	size_t es;
	Arena arena;
	Mat enc0, enc1, enc_out;           // encoder.0.0 (s2), encoder.1.0 (s2), encoder.<2 + R> (1x1 -> codebook_dim)
	std::vector<Res> enc_res, dec_res;
	Mat dec_in, up0, up1, dec_out;     // decoder.0 (1x1), the two folded upsampled convs (4 matrices each), the last 1x1
	float *cb = nullptr, *e2 = nullptr;   // codebook f32 [V][D], |e_j|^2 [V]
	WsBuf ws, qws;
};

namespace {

void launch_pack(int dt, const float* src, int C, int B, int L, int Lp, int relu, float* keep, void* dst, int ld, hipStream_t s) {
	const int64_t total = (int64_t)B * Lp * ld;
	by_dtype(dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k_dvae_pack<T>), dim3(grid_for(total)), dim3(256), 0, s, src, C, L, Lp, relu, keep, (T*)dst, ld, total); });
}

// k = 3, stride 2, padding 1 over operand rows x T [B][Lp][ld] (Lp even, rows >= L zero): f32 y [B * Lp / 2][N]
void conv_stride2(int dt, const void* x, int ld, size_t es, const Mat& w, int B, int Lp, float* y, hipStream_t s) {
	const int Lo = Lp / 2;
	GemmParams g = conv_gemm(w, w.bias, B * Lo, Lo, y, w.N, 1);
	const char* base = (const char*)x;
	const int64_t tap = (int64_t)w.Npad * w.Kpad;
	g.nseg = 3;
	g.seg[0] = {base + (size_t)ld * es, 2 * (int64_t)ld, -1, 0};
	g.seg[1] = {base, 2 * (int64_t)ld, 0, tap};
	g.seg[2] = {base + (size_t)ld * es, 2 * (int64_t)ld, 0, 2 * tap};
	launch_gemm(dt, g, s);
}

// nearest x2 + conv3 (padding 1) over operand rows x T [B * L][ld]: f32 y [B * 2 L][N]; w holds W0, W1 + W2, W0 + W1, W2
void conv_up2(int dt, const void* x, int ld, const Mat& w, int B, int L, float* y, hipStream_t s) {
	const int64_t tap = (int64_t)w.Npad * w.Kpad;
	for (int r = 0; r < 2; ++r) {
		GemmParams g = conv_gemm(w, w.bias, B * L, L, y + (size_t)r * w.N, 2 * (int64_t)w.N, 1);
		g.nseg = 2;
		g.seg[0] = {x, ld, r - 1, (2 * r) * tap};
		g.seg[1] = {x, ld, r, (2 * r + 1) * tap};
		launch_gemm(dt, g, s);
	}
}

// x (f32 residual stream [M][C], updated in place) through one ResBlock; a / a2 T [M][ld], hb f32 [M][C]
void resblock(int dt, const Res& rb, float* x, int C, int ld, int B, int L, void* a, void* a2, float* hb, hipStream_t s) {
	const int M = B * L;
	launch_pack(dt, x, C, B, L, L, 0, nullptr, a, ld, s);
	conv_same(dt, a, ld, rb.c0, 3, 1, M, L, nullptr, hb, 1, s);
	launch_pack(dt, hb, C, B, L, L, 1, nullptr, a2, ld, s);
	conv_same(dt, a2, ld, rb.c2, 3, 1, M, L, nullptr, hb, 1, s);
	launch_pack(dt, hb, C, B, L, L, 1, nullptr, a, ld, s);
	conv_same(dt, a, ld, rb.c4, 1, 1, M, L, x, x, 1, s);
}

int upload_res(Arena& ar, const WeightMap& wm, int dt, const std::string& p, int C, Res* r) {
	TTK_TRY(upload_mat(ar, wm, dt, p + "net.0.weight", p + "net.0.bias", PK_CONVK, C, C, false, &r->c0, 3));
	TTK_TRY(upload_mat(ar, wm, dt, p + "net.2.weight", p + "net.2.bias", PK_CONVK, C, C, false, &r->c2, 3));
	TTK_TRY(upload_mat(ar, wm, dt, p + "net.4.weight", p + "net.4.bias", PK_CONVK, C, C, false, &r->c4, 1));
	return TTK_OK;
}

// Conv1d weight [N][K][3] -> [N][K][4] = (W0, W1 + W2, W0 + W1, W2), folded in f32 on the host, then packed like any k-tap convolution
int upload_folded(Arena& ar, const WeightMap& wm, int dt, const std::string& wname, const std::string& bname, int N, int K, Mat* out) {
	const ttk_weight_view* v = wm.find(wname);
	const ttk_weight_view* b = wm.find(bname);
	TTK_REQUIRE(v != nullptr, TTK_E_WEIGHT, "missing weight '%s'", wname.c_str());
	TTK_REQUIRE(b != nullptr, TTK_E_WEIGHT, "missing weight '%s'", bname.c_str());
	TTK_REQUIRE(numel(v) == (int64_t)N * K * 3, TTK_E_WEIGHT, "weight '%s' has %lld elements, expected %lld", wname.c_str(), (long long)numel(v), (long long)N * K * 3);
	std::vector<float> w((size_t)N * K * 3), f((size_t)N * K * 4);
	TTK_HIP(hipMemcpy(w.data(), v->data, w.size() * sizeof(float), hipMemcpyDefault));
	for (size_t i = 0; i < (size_t)N * K; ++i) {
		const float w0 = w[3 * i], w1 = w[3 * i + 1], w2 = w[3 * i + 2];
		f[4 * i] = w0; f[4 * i + 1] = w1 + w2; f[4 * i + 2] = w0 + w1; f[4 * i + 3] = w2;
	}
	ttk_weight_view views[2];
	views[0].name = "__folded"; views[0].data = f.data(); views[0].ndim = 3;
	views[0].shape[0] = N; views[0].shape[1] = K; views[0].shape[2] = 4; views[0].shape[3] = 1;
	views[1] = *b;
	WeightMap local(views, 2);
	return upload_mat(ar, local, dt, "__folded", bname, PK_CONVK, N, K, false, out, 4);
}

int launch_quant(ttk_dvae* h, const float* z, int M, float* pmin, int* pidx, int64_t* codes, hipStream_t s) {
	const int V = h->cfg.num_tokens, D = h->cfg.codebook_dim;
	const int nw = (V + kQuantCodes - 1) / kQuantCodes;
	const int tiles = (M + 15) / 16, chunks = (M + kQuantRows - 1) / kQuantRows, tpc = (tiles + chunks - 1) / chunks;
	const dim3 grid((unsigned)nw, (unsigned)chunks);
	switch (D) {
#define TTK_DVAE_QUANT(DD) case DD: hipLaunchKernelGGL(k_dvae_quant<DD>, grid, dim3(256), 0, s, z, M, h->cb, h->e2, V, tpc, pmin, pidx); break;
		TTK_DVAE_QUANT(32) TTK_DVAE_QUANT(64) TTK_DVAE_QUANT(128) TTK_DVAE_QUANT(256) TTK_DVAE_QUANT(512)
#undef TTK_DVAE_QUANT
		default: TTK_REQUIRE(false, TTK_E_ARG, "ttk_dvae: codebook_dim %d has no quantizer instantiation", D);
	}
	hipLaunchKernelGGL(k_dvae_qcombine, dim3(grid_for(M)), dim3(256), 0, s, pmin, pidx, nw, M, codes);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}
size_t quant_partial_bytes(const ttk_dvae_config& c, int M) { return (size_t)((c.num_tokens + kQuantCodes - 1) / kQuantCodes) * M * 4; }

constexpr int64_t kMaxRows = 1 << 20;      // rows of one call: keeps every buffer of the widest layer below the GEMM's 2 GiB operand range (checked per call)

}  // namespace

extern "C" {

int ttk_dvae_create(ttk_dvae** out, const ttk_dvae_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_dvae_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16 || cfg->dtype == TTK_F16, TTK_E_ARG, "ttk_dvae_create: bad dtype %d (f32, bf16 or f16)", cfg->dtype);
	TTK_REQUIRE(cfg->channels >= 1 && cfg->channels <= 4096, TTK_E_ARG, "ttk_dvae_create: channels %d out of range", cfg->channels);
	TTK_REQUIRE(cfg->hidden_dim >= 8 && cfg->hidden_dim <= 4096 && cfg->hidden_dim % 8 == 0, TTK_E_ARG, "ttk_dvae_create: hidden_dim %d unsupported (a multiple of 8, <= 4096)", cfg->hidden_dim);
	const int D = cfg->codebook_dim;
	TTK_REQUIRE(D == 32 || D == 64 || D == 128 || D == 256 || D == 512, TTK_E_ARG, "ttk_dvae_create: codebook_dim %d unsupported (32, 64, 128, 256 or 512)", D);
	TTK_REQUIRE(cfg->num_tokens >= 1 && cfg->num_tokens <= (1 << 20), TTK_E_ARG, "ttk_dvae_create: num_tokens %d out of range", cfg->num_tokens);
	TTK_REQUIRE(cfg->num_resnet_blocks >= 1 && cfg->num_resnet_blocks <= 8, TTK_E_ARG,
				"ttk_dvae_create: num_resnet_blocks %d unsupported (1..8; without ResBlocks the reference builds a different decoder)", cfg->num_resnet_blocks);
	std::unique_ptr<ttk_dvae> h(new ttk_dvae());
	h->cfg = *cfg;
	h->dt = cfg->dtype;
	h->es = dtype_size(h->dt);
	const int dt = h->dt, ch = cfg->channels, H = cfg->hidden_dim, C2 = 2 * H, R = cfg->num_resnet_blocks, V = cfg->num_tokens;
	WeightMap wm(w, n_w);
	TTK_TRY(upload_mat(h->arena, wm, dt, "encoder.0.0.weight", "encoder.0.0.bias", PK_CONVK, H, ch, false, &h->enc0, 3));
	TTK_TRY(upload_mat(h->arena, wm, dt, "encoder.1.0.weight", "encoder.1.0.bias", PK_CONVK, C2, H, false, &h->enc1, 3));
	h->enc_res.resize(R);
	h->dec_res.resize(R);
	for (int i = 0; i < R; ++i) {
		TTK_TRY(upload_res(h->arena, wm, dt, "encoder." + std::to_string(2 + i) + ".", C2, &h->enc_res[i]));
		TTK_TRY(upload_res(h->arena, wm, dt, "decoder." + std::to_string(1 + i) + ".", C2, &h->dec_res[i]));
	}
	const std::string eo = "encoder." + std::to_string(2 + R) + ".", u0 = "decoder." + std::to_string(1 + R) + ".0.conv.", u1 = "decoder." + std::to_string(2 + R) + ".0.conv.",
					  dout = "decoder." + std::to_string(3 + R) + ".";
	TTK_TRY(upload_mat(h->arena, wm, dt, eo + "weight", eo + "bias", PK_CONVK, D, C2, false, &h->enc_out, 1));
	TTK_TRY(upload_mat(h->arena, wm, dt, "decoder.0.weight", "decoder.0.bias", PK_CONVK, C2, D, false, &h->dec_in, 1));
	TTK_TRY(upload_folded(h->arena, wm, dt, u0 + "weight", u0 + "bias", C2, C2, &h->up0));
	TTK_TRY(upload_folded(h->arena, wm, dt, u1 + "weight", u1 + "bias", H, C2, &h->up1));
	TTK_TRY(upload_mat(h->arena, wm, dt, dout + "weight", dout + "bias", PK_CONVK, ch, H, false, &h->dec_out, 1));
	{
		float* embed = nullptr;
		Arena tmp;
		TTK_TRY(upload_f32(tmp, wm, "codebook.embed", (int64_t)D * V, &embed));
		TTK_TRY(h->arena.alloc((void**)&h->cb, (size_t)V * D * 4));
		TTK_TRY(h->arena.alloc((void**)&h->e2, (size_t)V * 4));
		hipLaunchKernelGGL(k_dvae_codebook, dim3(grid_for(V)), dim3(256), 0, 0, embed, D, V, h->cb, h->e2);
		TTK_HIP(hipDeviceSynchronize());
	}
	*out = h.release();
	return TTK_OK;
}

int ttk_dvae_destroy(ttk_dvae* h) {
	if (!h) return TTK_OK;
	delete h;
	return TTK_OK;
}

int ttk_dvae_quantize(ttk_dvae* h, const float* z, int M, int64_t* codes_out, void* stream) {
	TTK_REQUIRE(h && z && codes_out, TTK_E_ARG, "ttk_dvae_quantize: null argument");
	TTK_REQUIRE(M >= 1 && M <= kMaxRows, TTK_E_ARG, "ttk_dvae_quantize: M = %d out of range (1..%lld)", M, (long long)kMaxRows);
	TTK_REQUIRE(((uintptr_t)z & 15) == 0, TTK_E_ARG, "ttk_dvae_quantize: z must be 16-byte aligned");
	const size_t pb = quant_partial_bytes(h->cfg, M);
	WsPlan ws;
	const size_t o_min = ws.take(pb), o_idx = ws.take(pb);
	TTK_TRY(h->qws.reserve(ws.total));
	char* base = (char*)h->qws.p;
	return launch_quant(h, z, M, (float*)(base + o_min), (int*)(base + o_idx), codes_out, (hipStream_t)stream);
}

int ttk_dvae_encode(ttk_dvae* h, const float* mel, int B, int T, int64_t* codes_out, float* z_out, void* stream) {
	TTK_REQUIRE(h && mel && codes_out, TTK_E_ARG, "ttk_dvae_encode: null argument");
	TTK_REQUIRE(B >= 1 && T >= 1, TTK_E_ARG, "ttk_dvae_encode: empty input (B=%d, T=%d)", B, T);
	TTK_REQUIRE(!z_out || ((uintptr_t)z_out & 15) == 0, TTK_E_ARG, "ttk_dvae_encode: z_out must be 16-byte aligned");
	const ttk_dvae_config& c = h->cfg;
	hipStream_t s = (hipStream_t)stream;
	const int dt = h->dt;
	const size_t es = h->es;
	const int H = c.hidden_dim, C2 = 2 * H, D = c.codebook_dim;
	const int L0 = T, L0p = round_up(L0, 2), L1 = L0p / 2, L1p = round_up(L1, 2), L2 = L1p / 2;
	const int ld0 = h->enc0.Kpad, ld1 = h->enc1.Kpad, ld2 = h->enc_out.Kpad;      // operand row widths: round_up(channels | H | 2 H, 64)
	const int64_t widest = std::max<int64_t>(std::max(2 * ld0, 2 * ld1), ld2);
	TTK_REQUIRE((int64_t)B * L0p <= kMaxRows && (int64_t)B * L0p * widest * 4 < ((int64_t)1 << 31), TTK_E_ARG,
				"ttk_dvae_encode: B = %d clips of T = %d frames exceed the 2 GiB buffer range of one call", B, T);
	const int M = B * L2;
	WsPlan ws;
	const size_t o_x0 = ws.take((size_t)B * L0p * ld0 * es), o_x1 = ws.take((size_t)B * L1p * ld1 * es);
	const size_t o_y = ws.take(std::max((size_t)B * L1 * H, (size_t)M * C2) * 4), o_hb = ws.take((size_t)M * C2 * 4);
	const size_t o_a = ws.take((size_t)M * ld2 * es), o_a2 = ws.take((size_t)M * ld2 * es), o_z = ws.take((size_t)M * D * 4);
	const size_t pb = quant_partial_bytes(c, M);
	const size_t o_min = ws.take(pb), o_idx = ws.take(pb);
	TTK_TRY(h->ws.reserve(ws.total));
	char* base = (char*)h->ws.p;
	void *x0 = base + o_x0, *x1 = base + o_x1, *a = base + o_a, *a2 = base + o_a2;
	float *y = (float*)(base + o_y), *hb = (float*)(base + o_hb), *z = z_out ? z_out : (float*)(base + o_z);

	{
		const int64_t total = (int64_t)B * L0p * ld0;
		by_dtype(dt, [&](auto t) { using TT = decltype(t); hipLaunchKernelGGL((k_dvae_in<TT>), dim3(grid_for(total)), dim3(256), 0, s, mel, c.channels, L0, L0p, (TT*)x0, ld0, total); });
	}
	conv_stride2(dt, x0, ld0, es, h->enc0, B, L0p, y, s);                  // f32 [B * L1][H]
	launch_pack(dt, y, H, B, L1, L1p, 1, nullptr, x1, ld1, s);
	conv_stride2(dt, x1, ld1, es, h->enc1, B, L1p, y, s);                  // f32 [B * L2][2 H]; its ReLU is applied in place by the first ResBlock's pack below
	launch_pack(dt, y, C2, B, L2, L2, 1, y, a, ld2, s);                    // (a is rewritten by resblock(); this launch is the in-place ReLU of the residual stream)
	for (int i = 0; i < c.num_resnet_blocks; ++i) resblock(dt, h->enc_res[i], y, C2, ld2, B, L2, a, a2, hb, s);
	launch_pack(dt, y, C2, B, L2, L2, 0, nullptr, a, ld2, s);
	conv_same(dt, a, ld2, h->enc_out, 1, 1, M, L2, nullptr, z, 1, s);      // f32 [M][D]
	TTK_HIP(hipGetLastError());
	return launch_quant(h, z, M, (float*)(base + o_min), (int*)(base + o_idx), codes_out, s);
}

int ttk_dvae_decode(ttk_dvae* h, const int64_t* codes, int B, int n, float* mel_out, float* hidden_out, void* stream) {
	TTK_REQUIRE(h && codes && mel_out, TTK_E_ARG, "ttk_dvae_decode: null argument");
	TTK_REQUIRE(B >= 1 && n >= 1, TTK_E_ARG, "ttk_dvae_decode: empty input (B=%d, n=%d)", B, n);
	const ttk_dvae_config& c = h->cfg;
	hipStream_t s = (hipStream_t)stream;
	const int dt = h->dt;
	const size_t es = h->es;
	const int H = c.hidden_dim, C2 = 2 * H, D = c.codebook_dim, ch = c.channels;
	const int ldD = h->dec_in.Kpad, ld2 = h->up0.Kpad, ldH = h->dec_out.Kpad;
	const int64_t widest = std::max<int64_t>(std::max(ldD, ld2), ldH);
	TTK_REQUIRE((int64_t)B * n * 4 <= kMaxRows && (int64_t)B * n * 4 * widest * 4 < ((int64_t)1 << 31), TTK_E_ARG,
				"ttk_dvae_decode: B = %d sequences of n = %d codes exceed the 2 GiB buffer range of one call", B, n);
	const int M = B * n;
	{
		std::vector<int64_t> host((size_t)M);
		TTK_HIP(hipMemcpyAsync(host.data(), codes, (size_t)M * sizeof(int64_t), hipMemcpyDefault, s));
		TTK_HIP(hipStreamSynchronize(s));
		for (int i = 0; i < M; ++i)
			TTK_REQUIRE(host[i] >= 0 && host[i] < c.num_tokens, TTK_E_ARG, "ttk_dvae_decode: code %lld at position %d is outside [0, %d)", (long long)host[i], i, c.num_tokens);
	}
	WsPlan ws;
	const size_t o_g = ws.take((size_t)M * ldD * es), o_x = ws.take((size_t)M * C2 * 4), o_hb = ws.take((size_t)M * C2 * 4);
	const size_t o_a = ws.take((size_t)M * ld2 * es), o_a2 = ws.take((size_t)M * ld2 * es);
	const size_t o_y1 = ws.take((size_t)2 * M * C2 * 4), o_a3 = ws.take((size_t)2 * M * ld2 * es);
	const size_t o_y2 = ws.take((size_t)4 * M * H * 4), o_a4 = ws.take((size_t)4 * M * ldH * es), o_o = ws.take((size_t)4 * M * ch * 4);
	TTK_TRY(h->ws.reserve(ws.total));
	char* base = (char*)h->ws.p;
	void *gt = base + o_g, *a = base + o_a, *a2 = base + o_a2, *a3 = base + o_a3, *a4 = base + o_a4;
	float *x = (float*)(base + o_x), *hb = (float*)(base + o_hb), *y1 = (float*)(base + o_y1), *y2 = (float*)(base + o_y2), *o = (float*)(base + o_o);

	{
		const int64_t total = (int64_t)M * ldD;
		by_dtype(dt, [&](auto t) { using TT = decltype(t); hipLaunchKernelGGL((k_dvae_gather<TT>), dim3(grid_for(total)), dim3(256), 0, s, codes, h->cb, c.num_tokens, D, (TT*)gt, ldD, total); });
	}
	conv_same(dt, gt, ldD, h->dec_in, 1, 1, M, n, nullptr, x, 1, s);                 // f32 [M][2 H]
	for (int i = 0; i < c.num_resnet_blocks; ++i) resblock(dt, h->dec_res[i], x, C2, ld2, B, n, a, a2, hb, s);
	launch_pack(dt, x, C2, B, n, n, 0, nullptr, a, ld2, s);
	conv_up2(dt, a, ld2, h->up0, B, n, y1, s);                                      // f32 [2 M][2 H]
	launch_pack(dt, y1, C2, B, 2 * n, 2 * n, 1, nullptr, a3, ld2, s);
	conv_up2(dt, a3, ld2, h->up1, B, 2 * n, y2, s);                                 // f32 [4 M][H]
	launch_pack(dt, y2, H, B, 4 * n, 4 * n, 1, y2, a4, ldH, s);                     // ReLU kept in f32 too: the `hidden` output
	conv_same(dt, a4, ldH, h->dec_out, 1, 1, 4 * M, 4 * n, nullptr, o, 1, s);       // f32 [4 M][channels]
	launch_cl_to_cf(o, B, ch, 4 * n, mel_out, s);
	if (hidden_out) launch_cl_to_cf(y2, B, H, 4 * n, hidden_out, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
