// Host layer over the segment GEMM (gemm.hip), shared by every handle that launches it on a Mat: the dense layer, Conv1d and ConvTranspose1d over
// channels-last rows, the workspace planner, and for the vocoders the ResBlock weight upload and the tanh + clamp + trim output kernel.
#pragma once
#include "ttk_host.h"

namespace ttk {

// what every convolution launch has in common: operand matrix, bias, M rows in batch elements of L rows, f32 or T-typed output at row stride ldc
inline GemmParams conv_gemm(const Mat& w, const float* bias, int M, int L, void* C, int64_t ldc, int out_f32) {
	GemmParams g = {};
	g.W = w.w; g.ldw = w.Kpad; g.M = M; g.N = w.N; g.K = w.Kpad; g.rows_per_batch = L; g.bias = bias;
	g.C = C; g.ldc = ldc; g.out_f32 = out_f32;
	return g;
}

// the plain-matrix sibling, a dense layer: C = A W^T + bias over the M rows of A (T-typed [M][lda]), one segment, rows without batch structure (rows_per_batch
// stays 0), f32 or T-typed output at row stride N.  The caller adds what its layer has besides: act, residual / ldr, out_scale, another ldc.
inline GemmParams dense_gemm(const void* A, int64_t lda, const Mat& w, int M, void* C, int out_f32) {
	GemmParams g = {};
	g.nseg = 1; g.seg[0] = {A, lda, 0, 0};
	g.W = w.w; g.ldw = w.Kpad; g.M = M; g.N = w.N; g.K = w.Kpad; g.bias = w.bias;
	g.C = C; g.ldc = w.N; g.out_f32 = out_f32;
	return g;
}
// ... launched, with an optional f32 residual [M][N] (may alias an f32 C)
inline void gemm_plain(int dt, const void* A, int64_t lda, const Mat& w, int M, const float* residual, void* C, int out_f32, hipStream_t s) {
	GemmParams g = dense_gemm(A, lda, w, M, C, out_f32);
	g.residual = residual; g.ldr = w.N;
	launch_gemm(dt, g, s);
}

// Conv1d of k taps, one GEMM segment per tap: out[m] = bias + sum_j A[m + shift0 + j * step] * W_j^T (+ residual), rows outside m's batch
// element zero.  `bias` is explicit (HiFiGAN's conv_pre takes a folded one).  ldr is set with or without a residual: the GEMM reads it only with one.
inline void conv_taps(int dt, const void* A, int lda, const Mat& w, const float* bias, int k, int shift0, int step, int M, int L, const float* residual,
					  void* C, int out_f32, hipStream_t s) {
	GemmParams g = conv_gemm(w, bias, M, L, C, w.N, out_f32);
	g.nseg = k;
	for (int j = 0; j < k; ++j) g.seg[j] = {A, lda, shift0 + j * step, (int64_t)j * w.Npad * w.Kpad};
	g.residual = residual; g.ldr = w.N;
	launch_gemm(dt, g, s);
}
// 'same' convolution: tap j multiplies row m + (j - (k-1)/2) * dil
inline void conv_same(int dt, const void* A, int lda, const Mat& w, int k, int dil, int M, int L, const float* residual, void* C, int out_f32, hipStream_t s) {
	conv_taps(dt, A, lda, w, w.bias, k, -((k - 1) / 2) * dil, dil, M, L, residual, C, out_f32, s);
}
// 'valid' convolution over rows that already carry (k-1)/2 padding rows on each side: f32 out row b * Lp + t (t < Lp - k + 1)
inline void conv_valid(int dt, const void* A, int lda, const Mat& w, int k, int M, int Lp, float* C, hipStream_t s) {
	conv_taps(dt, A, lda, w, w.bias, k, 0, 1, M, Lp, nullptr, C, 1, s);
}

// ConvTranspose1d(kernel k, stride u, padding pd) as one GEMM per output phase r < u, each seeing k / u taps and writing its phase through the
// output row stride:  y[u m + r] = bias + sum_t A[m + (r + pd - j_t) / u] * W_{j_t}^T,  j_t = the taps congruent to r + pd modulo u.   y f32 [M * u][N].
inline void convt_phases(int dt, const void* A, int lda, const Mat& W, int k, int u, int pd, int M, int L, float* y, hipStream_t s) {
	for (int r = 0; r < u; ++r) {
		GemmParams g = conv_gemm(W, W.bias, M, L, y + (size_t)r * W.N, (int64_t)u * W.N, 1);
		g.nseg = k / u;
		for (int t = 0; t < g.nseg; ++t) {
			const int j = (r + pd) % u + u * t;
			g.seg[t] = {A, lda, (r + pd - j) / u, (int64_t)j * W.Npad * W.Kpad};
		}
		launch_gemm(dt, g, s);
	}
}

// carves one WsBuf into 256-byte aligned pieces: take() every piece, reserve `total`, add the offsets to the base
struct WsPlan {
	size_t total = 0;
	size_t take(size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; }
};

// convs1.m / convs2.m (m = 0..2) of ResBlock `prefix` (BigVGAN AMPBlock1, HiFiGAN ResBlock1): k taps, ch -> ch
inline int upload_resblock(Arena& ar, const WeightMap& wm, int dt, const std::string& prefix, int ch, int k, Mat* c1, Mat* c2) {
	for (int m = 0; m < 3; ++m) {
		const std::string a = prefix + "convs1." + std::to_string(m) + ".", b = prefix + "convs2." + std::to_string(m) + ".";
		TTK_TRY(upload_mat(ar, wm, dt, a + "weight", a + "bias", PK_CONVK, ch, ch, false, &c1[m], k));
		TTK_TRY(upload_mat(ar, wm, dt, b + "weight", b + "bias", PK_CONVK, ch, ch, false, &c2[m], k));
	}
	return TTK_OK;
}

namespace {

// audio[b][t] = clamp(tanh(y[b * L + t]), -1, 1) for t < keep: the generator's final Tanh, the padding frames' samples trimmed.
// Grid ceil(B * keep / 256), 256 threads: tanh_out_grid.  (A template only because a plain kernel is emitted by every file that
// includes this header; this one exists where it is launched.)
template <int = 0>
__global__ void k_tanh_out(const float* y, int B, int L, int keep, float* audio) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (int64_t)B * keep) return;
	const int b = (int)(i / keep), t = (int)(i - (int64_t)b * keep);
	float v = tanhf(y[(int64_t)b * L + t]);
	audio[i] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
}

}  // namespace

inline dim3 tanh_out_grid(int B, int keep) { return dim3(grid_for((int64_t)B * keep)); }

}  // namespace ttk
