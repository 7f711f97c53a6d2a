// AttentionBlock of models/arch_utils.py:136-190 (+ QKVAttentionLegacy :59-94) over channels-last rows with an f32 residual stream, shared by
// the conditioning encoders (cond.hip) and the audio classifier (classifier.hip): GroupNorm for any channels-per-group, the qkv GEMM, attention
// (the MFMA kernel for head width 64, one wave per query row for head width 128) and the proj GEMM with the residual.
#pragma once
#include <float.h>

#include <vector>

#include "ttk_common.h"
#include "ttk_conv.h"

namespace ttk {
namespace {

constexpr int kRowWaveMaxT = 3584;      // positions whose scores fit k_attn_rowwave's LDS strip (4 waves x T floats + 4 query rows)

__device__ __forceinline__ float block_sum256(float v, float* red) {
	v = wave_sum(v);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	return (red[0] + red[1]) + (red[2] + red[3]);
}

// GroupNorm of one (batch element, group) per workgroup: two-pass mean / biased variance in f32 (F.group_norm, eps 1e-5), any C / groups
template <typename OT>
__global__ __launch_bounds__(256) void k_cond_gn(const float* __restrict__ x, int T, int C, int groups, const float* __restrict__ gamma,
												 const float* __restrict__ beta, OT* __restrict__ out) {
	__shared__ float red[4];
	const int g = blockIdx.x, cpg = C / groups, n = T * cpg;
	const int64_t off = (int64_t)blockIdx.y * T * C + g * cpg;
	float s = 0.f;
	for (int e = threadIdx.x; e < n; e += 256) { const int t = e / cpg, c = e - t * cpg; s += x[off + (int64_t)t * C + c]; }
	const float mean = block_sum256(s, red) / (float)n;
	float q = 0.f;
	for (int e = threadIdx.x; e < n; e += 256) { const int t = e / cpg, c = e - t * cpg; const float d = x[off + (int64_t)t * C + c] - mean; q += d * d; }
	const float rstd = rsqrtf(block_sum256(q, red) / (float)n + 1e-5f);
	for (int e = threadIdx.x; e < n; e += 256) {
		const int t = e / cpg, c = e - t * cpg;
		const int64_t i = off + (int64_t)t * C + c;
		out[i] = cvt<OT>((x[i] - mean) * rstd * gamma[g * cpg + c] + beta[g * cpg + c]);
	}
}

// Attention for head widths the MFMA kernel does not cover.  One wave per query row: lanes split the keys for q.k (+ bias) and the
// softmax statistics, scores live in the wave's LDS strip, then lanes split the head dims for P.V.  f32 throughout.
template <typename T, int HD>
__global__ __launch_bounds__(256) void k_attn_rowwave(AttnParams p) {
	typedef typename Frag<T>::type FragT;
	extern __shared__ float smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
	if (q >= p.T) return;                               // no workgroup barrier below: a wave may leave alone
	float* sc = smem + (int64_t)wave * p.T;
	float* qs = smem + (int64_t)4 * p.T + wave * HD;
	const T* base = (const T*)p.qkv + (int64_t)b * p.T * p.ld + h * p.head_stride;
	for (int d = lane; d < HD; d += 64) qs[d] = (float)base[(int64_t)q * p.ld + p.q_off + d] * p.scale;
	__builtin_amdgcn_wave_barrier();
	float m = -FLT_MAX;
	for (int j = lane; j < p.T; j += 64) {
		const T* kp = base + (int64_t)j * p.ld + p.k_off;
		float s = 0.f;
#pragma unroll 4
		for (int d = 0; d < HD; d += 8) {
			const FragT kf = *(const FragT*)(kp + d);
#pragma unroll
			for (int e = 0; e < 8; ++e) s += qs[d + e] * (float)kf[e];
		}
		if (p.bias) { int rel = j - q; rel = rel < -64 ? -64 : (rel > 64 ? 64 : rel); s += p.bias[h * 129 + rel + 64]; }
		sc[j] = s;
		m = fmaxf(m, s);
	}
	m = wave_max(m);
	float l = 0.f;
	for (int j = lane; j < p.T; j += 64) { const float e = __expf(sc[j] - m); sc[j] = e; l += e; }
	l = wave_sum(l);
	__builtin_amdgcn_wave_barrier();
	constexpr int DPL = HD / 64;
	float o[DPL];
#pragma unroll
	for (int e = 0; e < DPL; ++e) o[e] = 0.f;
	const T* vp = base + p.v_off + lane * DPL;
	for (int j = 0; j < p.T; ++j) {
		const float pj = sc[j];
#pragma unroll
		for (int e = 0; e < DPL; ++e) o[e] += pj * (float)vp[(int64_t)j * p.ld + e];
	}
	T* op = (T*)p.out + ((int64_t)b * p.T + q) * p.ldo + h * HD + lane * DPL;
	const float inv = 1.f / l;
#pragma unroll
	for (int e = 0; e < DPL; ++e) op[e] = cvt<T>(o[e] * inv);
}

// The launches of the two kernels above, each described once: attn_blocks and the entry points on caller-provided operands (cond.hip: ttk_block_gn_rows,
// ttk_attn_rowwave) both go through them.
template <typename OT>
inline void launch_cond_gn(const float* x, int nb, int Tn, int C, int groups, const float* gamma, const float* beta, OT* out, hipStream_t s) {
	hipLaunchKernelGGL((k_cond_gn<OT>), dim3(groups, nb), dim3(256), 0, s, x, Tn, C, groups, gamma, beta, out);
}
template <typename T>
inline void launch_attn_rowwave(const AttnParams& ap, hipStream_t s) {   // head width 128, ap.T <= kRowWaveMaxT
	hipLaunchKernelGGL((k_attn_rowwave<T, 128>), dim3((ap.T + 3) / 4, ap.H, ap.nb), dim3(256), (size_t)(4 * ap.T + 4 * 128) * 4, s, ap);
}

struct Block { float *gn_g = nullptr, *gn_b = nullptr, *relbias = nullptr; Mat qkv, proj; };

inline int gn_groups(int channels) {    // arch_utils.py:27-44
	int g = 32;
	if (channels <= 16) g = 8;
	else if (channels <= 64) g = 16;
	while (channels % g != 0) g /= 2;
	return g;
}

// blocks "<prefix><i>.{norm,qkv,proj_out}.*" (+ "__relbias" [heads][129] when relpos) of C channels
inline int upload_attn_blocks(Arena& ar, const WeightMap& wm, int dt, const std::string& prefix, int n, int C, int heads, bool relpos, std::vector<Block>* out) {
	out->resize(n);
	for (int i = 0; i < n; ++i) {
		Block& B = (*out)[i];
		const std::string p = prefix + std::to_string(i) + ".";
		TTK_TRY(upload_f32(ar, wm, p + "norm.weight", C, &B.gn_g));
		TTK_TRY(upload_f32(ar, wm, p + "norm.bias", C, &B.gn_b));
		TTK_TRY(upload_mat(ar, wm, dt, p + "qkv.weight", p + "qkv.bias", PK_NK, 3 * C, C, false, &B.qkv));
		TTK_TRY(upload_mat(ar, wm, dt, p + "proj_out.weight", p + "proj_out.bias", PK_NK, C, C, false, &B.proj));
		if (relpos) TTK_TRY(upload_f32(ar, wm, p + "__relbias", (int64_t)heads * 129, &B.relbias));
	}
	return TTK_OK;
}

// x f32 [b * T][C] through the blocks, in place.  a T [rows][C], qkv T [rows][3C], ao T [rows][C]: scratch.  hd = C / heads is 64 or 128; for 128 the caller
// has checked T <= kRowWaveMaxT.
template <typename T>
inline void attn_blocks(int dt, const std::vector<Block>& blocks, float* x, int b, int Tn, int C, int groups, int heads, T* a, T* qkv, T* ao, hipStream_t s) {
	const int hd = C / heads;
	const int64_t rows = (int64_t)b * Tn;
	for (const Block& B : blocks) {
		launch_cond_gn<T>(x, b, Tn, C, groups, B.gn_g, B.gn_b, a, s);
		gemm_plain(dt, a, C, B.qkv, (int)rows, nullptr, qkv, 0, s);
		AttnParams ap = {};
		ap.qkv = qkv; ap.ld = 3 * C; ap.q_off = 0; ap.k_off = hd; ap.v_off = 2 * hd; ap.head_stride = 3 * hd;   // head-major [H][3][hd], arch_utils.py:79
		ap.out = ao; ap.ldo = C; ap.nb = b; ap.T = Tn; ap.H = heads; ap.causal = 0; ap.bias = B.relbias;
		ap.scale = 1.f / sqrtf((float)hd);                                      // (q * hd^-1/4) . (k * hd^-1/4)
		if (hd == 64) launch_attn_fwd(dt, ap, s);
		else launch_attn_rowwave<T>(ap, s);
		gemm_plain(dt, ao, C, B.proj, (int)rows, x, x, 1, s);
	}
}

}  // namespace
}  // namespace ttk
