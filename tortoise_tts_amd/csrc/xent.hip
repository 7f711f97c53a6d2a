// Row cross-entropy of teacher-forced logits (F.cross_entropy(reduction="none") and its mean) and the reference's [B][C][T] logits layout.
//   k_xent_rows       : one workgroup per row, ONE pass over the row: every thread keeps a running (max, sum of exp(x - max)) over the 16-byte chunks it
//                       loads, the pairs are merged over the wave (xor butterfly) and over the four waves through LDS: nll = max + log(sum) - x[target]
//   k_xent_transpose  : logits [rows][ld] -> [rows / T][C][T] through a 64 x 64 LDS tile: both the loads (along C) and the stores (along T) are contiguous
//                       per wave -- the naive form stores 4 bytes per lane at stride T
//   k_xent_mean       : ONE workgroup, fixed order (include/ttk.h: ttk_xent_rows), no float atomics: two runs give the same bits
// Reference: F.cross_entropy at /root/reference/tortoise_tts/models/unified_voice.py:604-605, the permute of get_logits :526-530.
#include "ttk_common.h"
#include "ttk_host.h"

using namespace ttk;

namespace {

constexpr int XT = 256;       // threads of every launch in this file
constexpr int XTILE = 64;     // transpose tile edge

// (m, s) <- merge of two running pairs: s counts exp(x - m).  A pair that has seen nothing is (-inf, 0); -inf never meets -inf inside expf.
__device__ __forceinline__ void xent_merge(float& m, float& s, float m2, float s2) {
	const float mn = fmaxf(m, m2);
	if (mn == -INFINITY) { m = mn; s = 0.f; return; }
	s = s * expf(m - mn) + s2 * expf(m2 - mn);
	m = mn;
}

__device__ __forceinline__ void xent_take(float& m, float& s, float x) {
	if (x > m) { s = s * expf(m - x) + 1.f; m = x; }      // (m == -inf: s is 0 and expf(-inf) is 0)
	else if (x != -INFINITY) s += expf(x - m);
}

__device__ __forceinline__ void xent_take4(float& m, float& s, const float4 v) {
	const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
	if (mx == -INFINITY) return;
	const float mn = fmaxf(m, mx);
	s = s * expf(m - mn) + ((expf(v.x - mn) + expf(v.y - mn)) + (expf(v.z - mn) + expf(v.w - mn)));
	m = mn;
}

__global__ __launch_bounds__(XT) void k_xent_rows(const float* __restrict__ logits, int64_t ld, int C, const int64_t* __restrict__ target, float* __restrict__ nll) {
	const int row = blockIdx.x, tid = threadIdx.x;
	const float* x = logits + (int64_t)row * ld;
	// columns [0, head) up to the first 16-byte boundary and [body_end, C) behind the last whole chunk are read one by one; nothing at or past C is read
	int head = (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3);
	head = head < C ? head : C;
	const int nvec = (C - head) / 4, body_end = head + 4 * nvec;
	float m = -INFINITY, s = 0.f;
	if (tid < head) xent_take(m, s, x[tid]);
	const float4* xv = (const float4*)(x + head);
	for (int i = tid; i < nvec; i += XT) xent_take4(m, s, xv[i]);
	if (tid < C - body_end) xent_take(m, s, x[body_end + tid]);
	for (int o = 32; o > 0; o >>= 1) {
		const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
		xent_merge(m, s, m2, s2);
	}
	__shared__ float sm[XT / 64], ss[XT / 64];
	if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
	__syncthreads();
	if (tid == 0) {
		for (int w = 1; w < XT / 64; ++w) xent_merge(m, s, sm[w], ss[w]);
		const int64_t t = target[row];
		nll[row] = (t >= 0 && t < C) ? (m + logf(s)) - x[t] : NAN;      // (the callers validate the targets; an id outside the row is not read)
	}
}

__global__ __launch_bounds__(XT) void k_xent_transpose(const float* __restrict__ logits, int64_t ld, int C, int T, float* __restrict__ out) {
	__shared__ float tile[XTILE][XTILE + 1];
	const int c0 = blockIdx.x * XTILE, t0 = blockIdx.y * XTILE, b = blockIdx.z;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	for (int i = w; i < XTILE; i += XT / 64) {      // row t0 + i, 64 consecutive classes per wave
		const int t = t0 + i, c = c0 + lane;
		if (t < T && c < C) tile[i][lane] = logits[((int64_t)b * T + t) * ld + c];
	}
	__syncthreads();
	for (int i = w; i < XTILE; i += XT / 64) {      // class c0 + i, 64 consecutive frames per wave
		const int c = c0 + i, t = t0 + lane;
		if (c < C && t < T) out[((int64_t)b * C + c) * T + t] = tile[lane][i];
	}
}

__global__ __launch_bounds__(XT) void k_xent_mean(const float* __restrict__ nll, int rows, float* __restrict__ mean) {
	__shared__ float part[XT];
	float a = 0.f;
	for (int i = threadIdx.x; i < rows; i += XT) a += nll[i];
	part[threadIdx.x] = a;
	__syncthreads();
	for (int o = XT / 2; o > 0; o >>= 1) {
		if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
		__syncthreads();
	}
	if (threadIdx.x == 0) mean[0] = part[0] / (float)rows;
}

}  // namespace

namespace ttk {

void launch_xent_rows(const float* logits, int64_t ld, int rows, int C, const int64_t* target, float* nll, float* mean, float* logits_t, int T, hipStream_t s) {
	hipLaunchKernelGGL(k_xent_rows, dim3((unsigned)rows), dim3(XT), 0, s, logits, ld, C, target, nll);
	if (mean) hipLaunchKernelGGL(k_xent_mean, dim3(1), dim3(XT), 0, s, nll, rows, mean);
	if (logits_t) {
		const int nb = rows / T;
		for (int b0 = 0; b0 < nb; b0 += 65535) {      // grid z is a 16-bit count
			const int nz = nb - b0 < 65535 ? nb - b0 : 65535;
			hipLaunchKernelGGL(k_xent_transpose, dim3((unsigned)((C + XTILE - 1) / XTILE), (unsigned)((T + XTILE - 1) / XTILE), (unsigned)nz), dim3(XT), 0, s,
							   logits + (int64_t)b0 * T * ld, ld, C, T, logits_t + (int64_t)b0 * C * T);
		}
	}
}

}  // namespace ttk

extern "C" int ttk_xent_rows(const float* logits, int64_t ld, int rows, int C, const int64_t* target, float* nll_out, float* mean_out, float* logits_t_out, int T, void* stream) {
	TTK_REQUIRE(logits && target && nll_out, TTK_E_ARG, "ttk_xent_rows: null argument");
	TTK_REQUIRE(rows >= 1 && C >= 1 && ld >= C, TTK_E_ARG, "ttk_xent_rows: need rows >= 1, C >= 1 and ld >= C (got rows=%d C=%d ld=%lld)", rows, C, (long long)ld);
	TTK_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)nll_out & 3) == 0, TTK_E_ARG, "ttk_xent_rows: logits and nll_out must be 4-byte aligned");
	TTK_REQUIRE(!logits_t_out || (T >= 1 && rows % T == 0), TTK_E_ARG, "ttk_xent_rows: the transposed output is [rows / T][C][T]: rows=%d is no multiple of T=%d", rows, T);
	launch_xent_rows(logits, ld, rows, C, target, nll_out, mean_out, logits_t_out, T, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}
