// ttk_cls: AudioMiniEncoderWithClassifierHead (models/classifier.py:79-149), the network behind TorToiSe's `classify_audio_clip`: raw audio at 24 kHz ->
// embedding -> logits.  Building blocks: models/arch_utils.py:24-44 (normalization), :59-94 / :136-190 (AttentionBlock), :220-245 (Downsample).
//
// Layout: channels-last rows.  The residual stream and every GroupNorm are f32; the handle's dtype (f32 or bf16) rounds only GEMM / MFMA operands.
//
// ~94 % of the rows sit in the 32- and 64-channel stages (hundreds of thousands of rows for a few seconds of audio), where the 128-column tiles of the
// segment GEMM would spend most of their MFMA work on padding and a materialised operand tensor would double the traffic.  Those stages run on kernels of
// their own:
//  - k_cls_stem: Conv1d(1, 32, k = 3) straight from the samples.
//  - k_cls_stats + k_cls_stats_fold: GroupNorm statistics split over row chunks.  One workgroup per (batch element, chunk) computes a two-pass
//    (count, mean, M2) per group over its chunk; the fold merges the chunks in ascending order with Chan's formula into (mean, rstd).  No atomics.
//  - k_cls_conv5<T, C>, C = 32 | 64: GroupNorm + SiLU + Conv1d(C, C, k = 5) + bias (+ residual) in one launch.  A workgroup stages a 64-row tile plus a
//    2-row halo into LDS, normalised, activated and rounded to T once (rows outside the batch element's [0, L) are zero); every wave keeps the
//    [5][16][C] weights of its 16 output channels in registers and runs taps ascending, then k ascending in 32-wide steps, on
//    v_mfma_f32_16x16x32_bf16 / 8 x v_mfma_f32_16x16x4_f32.  The weights are the MFMA's first operand, so a lane ends with 4 consecutive channels of one
//    row: one float4 store (and one float4 residual load) per 16 x 16 tile.
// Everything wider runs on the segment GEMM through ttk_conv.h: k_cls_pack writes T-typed operand rows (GroupNorm + SiLU applied with the SAME
// arithmetic as the fused kernel's staging: gn_fold_coef / gn_fold_apply / silu_f), ResBlock convs are conv_same(k = 5), and every Downsample
// (k = 5, stride 4, padding 2) is five segments over the operand rows [Lp][ld] viewed as [Lp / 4][4 ld]: taps 0, 1 are quarters 2, 3 of view row
// m - 1, taps 2, 3, 4 quarters 0, 1, 2 of view row m.  The AttentionBlocks are those of cond.hip (ttk_attn_block.h).
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ttk_attn_block.h"
#include "ttk_common.h"
#include "ttk_conv.h"
#include "ttk_kernels.h"

using namespace ttk;

namespace {

constexpr int kTile = 64;              // output rows of one k_cls_conv5 tile
constexpr int kMaxConvGrid = 2048;     // workgroups along x of one k_cls_conv5 launch; a workgroup takes consecutive tiles
constexpr int kMaxGroups = 32;

// rows of one statistics chunk: 2048 at 32 channels .. 64 at 1024 and above (64 Ki elements per workgroup)
inline int stats_rows(int C) { return std::min(2048, std::max(64, 65536 / C)); }
inline int stats_chunks(int L, int C) { const int R = stats_rows(C); return (L + R - 1) / R; }

// audio f32 [B][T] -> rows f32 [B][T][32]: out[t][c] = bias[c] + sum_j w[c][j] * x[t + j - 1], taps ascending, zero outside the clip
__global__ __launch_bounds__(256) void k_cls_stem(const float* __restrict__ x, int Tn, const float* __restrict__ w, const float* __restrict__ bias,
												   float* __restrict__ out, int64_t total) {
	const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= total) return;
	const int c = (int)(idx & 31);
	const int64_t r = idx >> 5;
	const int t = (int)(r % Tn);
	const float* xb = x + (r - t);
	float v = bias[c];
#pragma unroll
	for (int j = 0; j < 3; ++j) {
		const int ts = t + j - 1;
		const float xv = ts >= 0 && ts < Tn ? xb[ts] : 0.f;
		v = fmaf(w[c * 3 + j], xv, v);
	}
	out[idx] = v;
}

// x f32 [B][L][C] -> part[b][chunk][g] = (count, mean, M2) of group g over rows [chunk * R, min(L, (chunk + 1) * R)).  Grid (chunks, B), 256 threads.
// Channels are taken 256 at a time (C itself when smaller): thread t owns channel t % cw and every (256 / cw)-th row, so a wave reads whole rows.  Per
// pass the threads' sums are folded per group by one thread in a fixed order (row lane ascending, then channel ascending).  C and C / G are powers of two.
__global__ __launch_bounds__(256) void k_cls_stats(const float* __restrict__ x, int L, int C, int G, int R, float* __restrict__ part) {
	__shared__ float acc[256];
	__shared__ float gm[256];
	const int t = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, nch = gridDim.x;
	const int r0 = chunk * R, r1 = min(L, r0 + R), cpg = C / G;
	const int cw = C < 256 ? C : 256, rpar = 256 / cw, gw = cw / cpg;      // channels, row lanes and groups of one channel block
	const int cl = t % cw, rl = t / cw;
	const float n = (float)(r1 - r0) * (float)cpg;
	for (int c0 = 0; c0 < C; c0 += cw) {
		const float* col = x + (int64_t)b * L * C + c0 + cl;
		float s = 0.f;
		for (int r = r0 + rl; r < r1; r += rpar) s += col[(int64_t)r * C];
		acc[t] = s;
		__syncthreads();
		if (t < gw) {
			float tot = 0.f;
			for (int i = 0; i < rpar; ++i)
				for (int cc = 0; cc < cpg; ++cc) tot += acc[i * cw + t * cpg + cc];
			gm[t] = tot / n;
		}
		__syncthreads();
		const float mean = gm[cl / cpg];
		float q = 0.f;
		for (int r = r0 + rl; r < r1; r += rpar) { const float d = col[(int64_t)r * C] - mean; q = fmaf(d, d, q); }
		acc[t] = q;
		__syncthreads();
		if (t < gw) {
			float tot = 0.f;
			for (int i = 0; i < rpar; ++i)
				for (int cc = 0; cc < cpg; ++cc) tot += acc[i * cw + t * cpg + cc];
			float* o = part + (((int64_t)b * nch + chunk) * G + c0 / cpg + t) * 3;
			o[0] = n; o[1] = gm[t]; o[2] = tot;
		}
		__syncthreads();
	}
}

// part [B][nch][G][3] -> ms [B][G][2] = (mean, rstd): the chunks merged in ascending order (Chan et al.), biased variance, eps 1e-5.  One thread per (b, g).
__global__ void k_cls_stats_fold(const float* __restrict__ part, int nch, int G, int total, float* __restrict__ ms) {
#pragma clang fp contract(off)
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= total) return;
	const int b = i / G, g = i - b * G;
	const float* p = part + ((int64_t)b * nch * G + g) * 3;
	float n = p[0], mean = p[1], m2 = p[2];
	for (int k = 1; k < nch; ++k) {
		const float* q = p + (int64_t)k * G * 3;
		const float nb = q[0], d = q[1] - mean, nt = n + nb;
		mean = mean + d * (nb / nt);
		m2 = m2 + q[2] + d * d * (n * nb / nt);
		n = nt;
	}
	ms[2 * i] = mean;
	ms[2 * i + 1] = 1.f / sqrtf(m2 / n + 1e-5f);
}

// the one definition of "GroupNorm, then SiLU" of this file: y = silu(x * a + d), (a, d) = gn_fold_coef(mean, rstd, gamma, beta)
__device__ __forceinline__ void cls_coef(const float* ms, const float* gamma, const float* beta, int b, int G, int cpg, int c, float& a, float& d) {
	const float* m = ms + ((int64_t)b * G + c / cpg) * 2;
	gn_fold_coef(m[0], m[1], gamma[c], beta[c], 0.f, 0.f, a, d);
}
__device__ __forceinline__ float cls_norm_act(float x, float a, float d) { return silu_f(gn_fold_apply(x, a, d)); }

// src f32 [B][L][C] -> dst T [B][Lp][ld]: rows >= L and columns >= C zero; with ms != null the value is silu(gn(src)) (statistics ms [B][G][2])
template <typename T>
__global__ __launch_bounds__(256) void k_cls_pack(const float* __restrict__ src, int C, int L, int Lp, const float* __restrict__ ms, const float* __restrict__ gamma,
												   const float* __restrict__ beta, int G, T* __restrict__ dst, int ld, int64_t total) {
	const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= total) return;
	const int c = (int)(idx % ld);
	const int64_t r = idx / ld;
	const int t = (int)(r % Lp);
	const int64_t b = r / Lp;
	float v = 0.f;
	if (c < C && t < L) {
		v = src[(b * L + t) * C + c];
		if (ms) {
			float a, d;
			cls_coef(ms, gamma, beta, (int)b, G, C / G, c, a, d);
			v = cls_norm_act(v, a, d);
		}
	}
	dst[idx] = cvt<T>(v);
}

template <typename T> struct StageRow;      // LDS row of the staged tile: C elements of T plus 16 bytes (spreads the rows of a 16-lane read over the banks)
template <> struct StageRow<float> { static constexpr int pad = 4; };
template <> struct StageRow<bf16> { static constexpr int pad = 8; };

template <typename T> __device__ __forceinline__ void stage4(T* p, float4 v);
template <> __device__ __forceinline__ void stage4<float>(float* p, float4 v) { *(float4*)p = v; }
template <> __device__ __forceinline__ void stage4<bf16>(bf16* p, float4 v) { *(uint2*)p = pack4_16<bf16>(v.x, v.y, v.z, v.w); }

template <typename T> __device__ __forceinline__ typename Frag<T>::type read_frag(const T* p);
template <> __device__ __forceinline__ f32x8 read_frag<float>(const float* p) {      // two 16-byte reads: the padded row stride is no multiple of 32 bytes
	const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
	return f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <> __device__ __forceinline__ bf16x8 read_frag<bf16>(const bf16* p) { return *(const bf16x8*)p; }

// See the file header.  x f32 [B][L][C]; ms [B][G][2] or null (null: plain convolution, no GroupNorm, no SiLU); w f32 [C][C][5] (Conv1d's own layout,
// rounded to T on its way into the registers); residual f32 [B][L][C] or null (may be `out`); out f32 [B][L][C], not x.
// Grid (workgroups, B), 256 threads; workgroup x takes tiles [x * tiles_per_wg, (x + 1) * tiles_per_wg) of kTile rows.
template <typename T, int C>
__global__ __launch_bounds__(256) void k_cls_conv5(const float* __restrict__ x, int L, const float* __restrict__ ms, const float* __restrict__ gamma,
													const float* __restrict__ beta, int G, const float* __restrict__ w, const float* __restrict__ bias,
													const float* residual, float* out, int tiles_per_wg) {
	typedef typename Frag<T>::type FragT;
	constexpr int LDR = C + StageRow<T>::pad, KS = C / 32, NT = C / 16, C4 = C / 4, SUBS = kTile / 16;
	constexpr int RSTEP = 4 / NT;                               // waves that share one 16-channel tile split the tile's 16-row subtiles between them
	static_assert(NT == 2 || NT == 4, "k_cls_conv5 is instantiated for 32 and 64 channels");
	__shared__ __attribute__((aligned(16))) T rows[(kTile + 4) * LDR];
	__shared__ float ca[C], cd[C];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4, b = blockIdx.y;
	const int n0 = 16 * (wave % NT), sub0 = wave / NT;
	if (ms && threadIdx.x < C) {
		float a, d;
		cls_coef(ms, gamma, beta, b, G, C / G, threadIdx.x, a, d);
		ca[threadIdx.x] = a; cd[threadIdx.x] = d;
	}
	FragT wr[5][KS];
#pragma unroll
	for (int tap = 0; tap < 5; ++tap)
#pragma unroll
		for (int ks = 0; ks < KS; ++ks)
#pragma unroll
			for (int j = 0; j < 8; ++j) wr[tap][ks][j] = cvt<T>(w[((int64_t)(n0 + l15) * C + 32 * ks + 8 * g + j) * 5 + tap]);
	const float4 bv = *(const float4*)(bias + n0 + 4 * g);
	const int ntiles = (L + kTile - 1) / kTile;
	const int tile0 = blockIdx.x * tiles_per_wg, tile1 = min(tile0 + tiles_per_wg, ntiles);
	const float* xb = x + (int64_t)b * L * C;
	for (int tile = tile0; tile < tile1; ++tile) {
		const int t0 = tile * kTile;
		__syncthreads();                                        // the coefficients are written; the previous tile's reads are done
		for (int e = threadIdx.x; e < (kTile + 4) * C4; e += 256) {
			const int i = e / C4, q = e - i * C4, row = t0 - 2 + i;
			float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
			if (row >= 0 && row < L) {
				v = *(const float4*)(xb + (int64_t)row * C + 4 * q);
				if (ms) {
					v.x = cls_norm_act(v.x, ca[4 * q], cd[4 * q]);
					v.y = cls_norm_act(v.y, ca[4 * q + 1], cd[4 * q + 1]);
					v.z = cls_norm_act(v.z, ca[4 * q + 2], cd[4 * q + 2]);
					v.w = cls_norm_act(v.w, ca[4 * q + 3], cd[4 * q + 3]);
				}
			}
			stage4<T>(rows + i * LDR + 4 * q, v);
		}
		__syncthreads();
		for (int sub = sub0; sub < SUBS; sub += RSTEP) {
			if (t0 + 16 * sub >= L) break;
			f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
			const T* rp = rows + (16 * sub + l15) * LDR + 8 * g;      // output row o reads staged rows o + tap: the tile starts two rows early
#pragma unroll
			for (int tap = 0; tap < 5; ++tap)
#pragma unroll
				for (int ks = 0; ks < KS; ++ks) acc = mma16<T>(wr[tap][ks], read_frag<T>(rp + tap * LDR + 32 * ks), acc);
			// acc[r] = D[channel n0 + 4 g + r][row t0 + 16 sub + l15]
			const int row = t0 + 16 * sub + l15;
			if (row < L) {
				const int64_t o = ((int64_t)b * L + row) * C + n0 + 4 * g;
				float4 y = make_float4(acc[0] + bv.x, acc[1] + bv.y, acc[2] + bv.z, acc[3] + bv.w);
				if (residual) { const float4 rv = *(const float4*)(residual + o); y.x += rv.x; y.y += rv.y; y.z += rv.z; y.w += rv.w; }
				*(float4*)(out + o) = y;
			}
		}
	}
}

// x f32 [B][L][E]: emb[b] = row 0, logits[b][c] = bias[c] + sum_k W[c][k] * x[b][0][k] (f32, k ascending).  Grid B, 256 threads.
__global__ __launch_bounds__(256) void k_cls_head(const float* __restrict__ x, int L, int E, const float* __restrict__ W, const float* __restrict__ bias, int classes,
												   float* __restrict__ emb, float* __restrict__ logits) {
	const int b = blockIdx.x;
	const float* row = x + (int64_t)b * L * E;
	if (emb)
		for (int k = threadIdx.x; k < E; k += 256) emb[(int64_t)b * E + k] = row[k];
	if (logits && (int)threadIdx.x < classes) {
		const int c = threadIdx.x;
		float v = bias[c];
		for (int k = 0; k < E; ++k) v = fmaf(W[(int64_t)c * E + k], row[k], v);
		logits[(int64_t)b * classes + c] = v;
	}
}

int launch_stats(const float* x, int B, int L, int C, int G, float* part, float* ms, hipStream_t s) {
	const int nch = stats_chunks(L, C);
	hipLaunchKernelGGL(k_cls_stats, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, s, x, L, C, G, stats_rows(C), part);
	hipLaunchKernelGGL(k_cls_stats_fold, dim3((unsigned)((B * G + 63) / 64)), dim3(64), 0, s, part, nch, G, B * G, ms);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int launch_conv5(int dt, const float* x, int B, int L, int C, const float* ms, const float* gamma, const float* beta, int G, const float* w, const float* bias,
				 const float* residual, float* out, hipStream_t s) {
	const int ntiles = (L + kTile - 1) / kTile, gx = std::min(ntiles, kMaxConvGrid), tpw = (ntiles + gx - 1) / gx;
	const dim3 grid((unsigned)((ntiles + tpw - 1) / tpw), (unsigned)B);
	by_f32_bf16(dt, [&](auto t) {
		using T = decltype(t);
		if (C == 32) hipLaunchKernelGGL((k_cls_conv5<T, 32>), grid, dim3(256), 0, s, x, L, ms, gamma, beta, G, w, bias, residual, out, tpw);
		else hipLaunchKernelGGL((k_cls_conv5<T, 64>), grid, dim3(256), 0, s, x, L, ms, gamma, beta, G, w, bias, residual, out, tpw);
	});
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

void launch_pack(int dt, const float* src, int C, int B, int L, int Lp, const float* ms, const float* gamma, const float* beta, int G, void* dst, int ld, hipStream_t s) {
	const int64_t total = (int64_t)B * Lp * ld;
	by_f32_bf16(dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k_cls_pack<T>), dim3(grid_for(total)), dim3(256), 0, s, src, C, L, Lp, ms, gamma, beta, G, (T*)dst, ld, total); });
}

// Conv1d(k = 5, stride 4, padding 2) over operand rows x T [B][Lp][ld] (Lp % 4 == 0, rows >= L zero): f32 y [B * Lp / 4][N]
void conv_down4(int dt, const void* x, int ld, size_t es, const Mat& w, int B, int Lp, float* y, hipStream_t s) {
	const int Lo = Lp / 4;
	GemmParams g = conv_gemm(w, w.bias, B * Lo, Lo, y, w.N, 1);
	const char* base = (const char*)x;
	const int64_t tap = (int64_t)w.Npad * w.Kpad, lda = 4 * (int64_t)ld;
	const size_t q = (size_t)ld * es;
	g.nseg = 5;
	g.seg[0] = {base + 2 * q, lda, -1, 0};
	g.seg[1] = {base + 3 * q, lda, -1, tap};
	g.seg[2] = {base, lda, 0, 2 * tap};
	g.seg[3] = {base + q, lda, 0, 3 * tap};
	g.seg[4] = {base + 2 * q, lda, 0, 4 * tap};
	launch_gemm(dt, g, s);
}

struct ResBlock {
	float *gn0_g = nullptr, *gn0_b = nullptr, *gn1_g = nullptr, *gn1_b = nullptr;
	float *w0 = nullptr, *b0 = nullptr, *w1 = nullptr, *b1 = nullptr;      // fused stages (32 / 64 channels): Conv1d weights as they are
	Mat c0, c1;                                                             // GEMM stages
};
struct Stage { int ch = 0; bool fused = false; std::vector<ResBlock> res; Mat down; };

int check_dtype(const char* who, int dtype) {
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16, TTK_E_ARG, "%s: bad dtype %d (f32 or bf16)", who, dtype);
	return TTK_OK;
}

}  // namespace

struct ttk_cls {
	ttk_cls_config cfg;
	int dt, ch_final, groups_emb;
	size_t es;
	Arena arena;
	float *stem_w = nullptr, *stem_b = nullptr, *fin_g = nullptr, *fin_b = nullptr, *head_w = nullptr, *head_b = nullptr;
	std::vector<Stage> stages;
	Mat fin;
	std::vector<Block> blocks;
	WsBuf ws;
};

extern "C" {

int ttk_cls_stats_rows(int C) { return C >= 1 ? stats_rows(C) : 0; }

int ttk_cls_gn_stats(const float* x, int B, int L, int C, int groups, float* part, int64_t part_floats, float* stats_out, void* stream) {
	TTK_REQUIRE(x && part && stats_out, TTK_E_ARG, "ttk_cls_gn_stats: null argument");
	TTK_REQUIRE(B >= 1 && L >= 1, TTK_E_ARG, "ttk_cls_gn_stats: empty input (B=%d, L=%d)", B, L);
	TTK_REQUIRE(C >= 2 && C <= 4096 && (C & (C - 1)) == 0, TTK_E_ARG, "ttk_cls_gn_stats: C = %d unsupported (a power of two in 2..4096)", C);
	TTK_REQUIRE(groups >= 1 && groups <= kMaxGroups && (groups & (groups - 1)) == 0 && C / groups >= 1 && C / groups <= 256 && C >= groups, TTK_E_ARG,
				"ttk_cls_gn_stats: groups = %d unsupported for C = %d (a power of two, at most %d, at most 256 channels each)", groups, C, kMaxGroups);
	const int64_t need = (int64_t)B * stats_chunks(L, C) * groups * 3;
	TTK_REQUIRE(part_floats >= need, TTK_E_ARG, "ttk_cls_gn_stats: part holds %lld floats, %lld are needed", (long long)part_floats, (long long)need);
	return launch_stats(x, B, L, C, groups, part, stats_out, (hipStream_t)stream);
}

int ttk_cls_conv5_rows(int dtype, const float* x, int B, int L, int C, const float* stats, int groups, const float* gamma, const float* beta, const float* w,
					   const float* bias, const float* residual, float* out, void* stream) {
	TTK_TRY(check_dtype("ttk_cls_conv5_rows", dtype));
	TTK_REQUIRE(x && w && bias && out, TTK_E_ARG, "ttk_cls_conv5_rows: null argument");
	TTK_REQUIRE(x != out, TTK_E_ARG, "ttk_cls_conv5_rows: x and out must be different buffers (a tile reads its neighbours' rows)");
	TTK_REQUIRE(C == 32 || C == 64, TTK_E_ARG, "ttk_cls_conv5_rows: C = %d has no instantiation (32 or 64)", C);
	TTK_REQUIRE(B >= 1 && B <= 65535 && L >= 1, TTK_E_ARG, "ttk_cls_conv5_rows: B = %d, L = %d out of range (B 1..65535, L >= 1)", B, L);
	if (stats) {
		TTK_REQUIRE(gamma && beta, TTK_E_ARG, "ttk_cls_conv5_rows: statistics without gamma / beta");
		TTK_REQUIRE(groups >= 1 && groups <= kMaxGroups && C % groups == 0, TTK_E_ARG, "ttk_cls_conv5_rows: groups = %d does not divide C = %d (1..%d)", groups, C, kMaxGroups);
	}
	TTK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)bias & 15) == 0 && (!residual || ((uintptr_t)residual & 15) == 0), TTK_E_ARG,
				"ttk_cls_conv5_rows: x, out, bias and residual must be 16-byte aligned");
	return launch_conv5(dtype == TTK_BF16 ? DT_BF16 : DT_F32, x, B, L, C, stats, gamma, beta, stats ? groups : 1, w, bias, residual, out, (hipStream_t)stream);
}

int ttk_cls_create(ttk_cls** out, const ttk_cls_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_cls_create: null argument");
	TTK_TRY(check_dtype("ttk_cls_create", cfg->dtype));
	TTK_REQUIRE(cfg->spec_dim == 1, TTK_E_ARG, "ttk_cls_create: spec_dim %d unsupported (1: the stem reads raw audio)", cfg->spec_dim);
	TTK_REQUIRE(cfg->kernel_size == 5, TTK_E_ARG, "ttk_cls_create: kernel_size %d unsupported (5)", cfg->kernel_size);
	TTK_REQUIRE(cfg->downsample_factor == 4, TTK_E_ARG, "ttk_cls_create: downsample_factor %d unsupported (4)", cfg->downsample_factor);
	TTK_REQUIRE(cfg->base_channels == 32, TTK_E_ARG, "ttk_cls_create: base_channels %d unsupported (32)", cfg->base_channels);
	TTK_REQUIRE(cfg->depth >= 1 && cfg->depth <= 6, TTK_E_ARG, "ttk_cls_create: depth %d unsupported (1..6)", cfg->depth);
	TTK_REQUIRE(cfg->resnet_blocks >= 0 && cfg->resnet_blocks <= 16 && cfg->attn_blocks >= 0 && cfg->attn_blocks <= 64, TTK_E_ARG,
				"ttk_cls_create: resnet_blocks %d / attn_blocks %d out of range (0..16 / 0..64)", cfg->resnet_blocks, cfg->attn_blocks);
	TTK_REQUIRE(cfg->num_attn_heads >= 1 && cfg->embedding_dim >= 128 && cfg->embedding_dim <= 4096 && cfg->embedding_dim % 128 == 0 &&
				cfg->embedding_dim % cfg->num_attn_heads == 0, TTK_E_ARG, "ttk_cls_create: embedding_dim %d / num_attn_heads %d unsupported (a multiple of 128, divisible by the heads)",
				cfg->embedding_dim, cfg->num_attn_heads);
	const int E = cfg->embedding_dim, hd = E / cfg->num_attn_heads;
	TTK_REQUIRE(hd == 64 || hd == 128, TTK_E_ARG, "ttk_cls_create: head width %d unsupported (64 or 128)", hd);
	TTK_REQUIRE(cfg->classes >= 1 && cfg->classes <= 16, TTK_E_ARG, "ttk_cls_create: classes %d unsupported (1..16)", cfg->classes);
	std::unique_ptr<ttk_cls> h(new ttk_cls());
	h->cfg = *cfg;
	h->dt = cfg->dtype == TTK_BF16 ? DT_BF16 : DT_F32;
	h->es = dtype_size(h->dt);
	h->groups_emb = gn_groups(E);
	const int dt = h->dt;
	WeightMap wm(w, n_w);
	TTK_TRY(upload_f32(h->arena, wm, "enc.init.0.weight", 32 * 3, &h->stem_w));
	TTK_TRY(upload_f32(h->arena, wm, "enc.init.0.bias", 32, &h->stem_b));
	h->stages.resize(cfg->depth);
	int ch = 32, idx = 0;
	for (int l = 0; l < cfg->depth; ++l) {
		Stage& st = h->stages[l];
		st.ch = ch;
		st.fused = ch <= 64;
		st.res.resize(cfg->resnet_blocks);
		for (ResBlock& rb : st.res) {
			const std::string p = "enc.res." + std::to_string(idx++) + ".";
			TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.0.weight", ch, &rb.gn0_g));
			TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.0.bias", ch, &rb.gn0_b));
			TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.0.weight", ch, &rb.gn1_g));
			TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.0.bias", ch, &rb.gn1_b));
			if (st.fused) {
				TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.2.weight", (int64_t)ch * ch * 5, &rb.w0));
				TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.2.bias", ch, &rb.b0));
				TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.3.weight", (int64_t)ch * ch * 5, &rb.w1));
				TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.3.bias", ch, &rb.b1));
			} else {
				TTK_TRY(upload_mat(h->arena, wm, dt, p + "in_layers.2.weight", p + "in_layers.2.bias", PK_CONVK, ch, ch, false, &rb.c0, 5));
				TTK_TRY(upload_mat(h->arena, wm, dt, p + "out_layers.3.weight", p + "out_layers.3.bias", PK_CONVK, ch, ch, false, &rb.c1, 5));
			}
		}
		const std::string p = "enc.res." + std::to_string(idx++) + ".op.";
		TTK_TRY(upload_mat(h->arena, wm, dt, p + "weight", p + "bias", PK_CONVK, 2 * ch, ch, false, &st.down, 5));
		ch *= 2;
	}
	h->ch_final = ch;
	TTK_TRY(upload_f32(h->arena, wm, "enc.final.0.weight", ch, &h->fin_g));
	TTK_TRY(upload_f32(h->arena, wm, "enc.final.0.bias", ch, &h->fin_b));
	TTK_TRY(upload_mat(h->arena, wm, dt, "enc.final.2.weight", "enc.final.2.bias", PK_CONVK, E, ch, false, &h->fin, 1));
	TTK_TRY(upload_attn_blocks(h->arena, wm, dt, "enc.attn.", cfg->attn_blocks, E, cfg->num_attn_heads, false, &h->blocks));
	TTK_TRY(upload_f32(h->arena, wm, "head.weight", (int64_t)cfg->classes * E, &h->head_w));
	TTK_TRY(upload_f32(h->arena, wm, "head.bias", cfg->classes, &h->head_b));
	TTK_HIP(hipDeviceSynchronize());
	*out = h.release();
	return TTK_OK;
}

int ttk_cls_destroy(ttk_cls* h) {
	if (!h) return TTK_OK;
	(void)hipDeviceSynchronize();
	delete h;
	return TTK_OK;
}

int ttk_cls_forward_taps(ttk_cls* h, const float* audio, int B, int T, float* emb_out, float* logits_out, float* const* taps, int n_taps, void* stream) {
	TTK_REQUIRE(h && audio && (emb_out || logits_out), TTK_E_ARG, "ttk_cls_forward: null argument");
	TTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1, TTK_E_ARG, "ttk_cls_forward: B = %d, T = %d out of range (B 1..65535, T >= 1)", B, T);
	const ttk_cls_config& c = h->cfg;
	const int depth = c.depth, E = c.embedding_dim, dt = h->dt, hd = E / c.num_attn_heads;
	const size_t es = h->es;
	TTK_REQUIRE(!taps || n_taps == depth + 2, TTK_E_ARG, "ttk_cls_forward_taps: n_taps = %d, expected depth + 2 = %d", n_taps, depth + 2);
	hipStream_t s = (hipStream_t)stream;
	std::vector<int> L(depth + 1);
	L[0] = T;
	for (int l = 0; l < depth; ++l) L[l + 1] = (L[l] + 3) / 4;
	const int Lf = L[depth];
	TTK_REQUIRE(hd == 64 || Lf <= kRowWaveMaxT, TTK_E_ARG,
				"ttk_cls_forward: a clip of %d samples leaves %d positions after the %d stride-4 stages, above the row-wave attention's limit of %d positions", T, Lf, depth,
				kRowWaveMaxT);
	// sizes: the two f32 streams, the T-typed operand / attention scratch, the statistics
	int64_t fmax = std::max<int64_t>((int64_t)Lf * E, (int64_t)Lf * h->ch_final), amax = std::max<int64_t>((int64_t)Lf * E * 5, (int64_t)Lf * h->ch_final), pmax = 0;
	for (int l = 0; l < depth; ++l) {
		const int ch = h->stages[l].ch;
		fmax = std::max(fmax, (int64_t)L[l] * ch);
		amax = std::max(amax, (int64_t)round_up(L[l], 4) * h->stages[l].down.Kpad);
		pmax = std::max(pmax, (int64_t)stats_chunks(L[l], ch) * gn_groups(ch) * 3);
	}
	pmax = std::max(pmax, (int64_t)stats_chunks(Lf, h->ch_final) * gn_groups(h->ch_final) * 3);
	TTK_REQUIRE((int64_t)B * amax * (int64_t)es < ((int64_t)1 << 31) && (int64_t)B * fmax < ((int64_t)1 << 31), TTK_E_ARG,
				"ttk_cls_forward: B = %d clips of T = %d samples exceed the 2 GiB buffer range of one call", B, T);
	WsPlan ws;
	const size_t o_x = ws.take((size_t)B * fmax * 4), o_h = ws.take((size_t)B * fmax * 4), o_a = ws.take((size_t)B * amax * es);
	const size_t o_p = ws.take((size_t)B * pmax * 4), o_ms = ws.take((size_t)B * kMaxGroups * 2 * 4);
	TTK_TRY(h->ws.reserve(ws.total));
	char* base = (char*)h->ws.p;
	float *x = (float*)(base + o_x), *hb = (float*)(base + o_h), *part = (float*)(base + o_p), *ms = (float*)(base + o_ms);
	void* a = base + o_a;
	auto tap_out = [&](int i, const float* src, int64_t n) -> int {
		if (taps && taps[i]) TTK_HIP(hipMemcpyAsync(taps[i], src, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
		return TTK_OK;
	};

	{
		const int64_t total = (int64_t)B * T * 32;
		hipLaunchKernelGGL(k_cls_stem, dim3(grid_for(total)), dim3(256), 0, s, audio, T, h->stem_w, h->stem_b, x, total);
		TTK_TRY(tap_out(0, x, total));
	}
	for (int l = 0; l < depth; ++l) {
		const Stage& st = h->stages[l];
		const int ch = st.ch, G = gn_groups(ch), Ll = L[l], M = B * Ll;
		for (const ResBlock& rb : st.res) {
			TTK_TRY(launch_stats(x, B, Ll, ch, G, part, ms, s));
			if (st.fused) {
				TTK_TRY(launch_conv5(dt, x, B, Ll, ch, ms, rb.gn0_g, rb.gn0_b, G, rb.w0, rb.b0, nullptr, hb, s));
				TTK_TRY(launch_stats(hb, B, Ll, ch, G, part, ms, s));
				TTK_TRY(launch_conv5(dt, hb, B, Ll, ch, ms, rb.gn1_g, rb.gn1_b, G, rb.w1, rb.b1, x, x, s));
			} else {
				launch_pack(dt, x, ch, B, Ll, Ll, ms, rb.gn0_g, rb.gn0_b, G, a, ch, s);
				conv_same(dt, a, ch, rb.c0, 5, 1, M, Ll, nullptr, hb, 1, s);
				TTK_TRY(launch_stats(hb, B, Ll, ch, G, part, ms, s));
				launch_pack(dt, hb, ch, B, Ll, Ll, ms, rb.gn1_g, rb.gn1_b, G, a, ch, s);
				conv_same(dt, a, ch, rb.c1, 5, 1, M, Ll, x, x, 1, s);
			}
		}
		const int Lp = round_up(Ll, 4), ld = st.down.Kpad;
		launch_pack(dt, x, ch, B, Ll, Lp, nullptr, nullptr, nullptr, 1, a, ld, s);
		conv_down4(dt, a, ld, es, st.down, B, Lp, hb, s);      // f32 [B * L[l + 1]][2 ch]
		std::swap(x, hb);
		TTK_TRY(tap_out(l + 1, x, (int64_t)B * L[l + 1] * 2 * ch));
	}
	{
		const int ch = h->ch_final, G = gn_groups(ch);
		TTK_TRY(launch_stats(x, B, Lf, ch, G, part, ms, s));
		launch_pack(dt, x, ch, B, Lf, Lf, ms, h->fin_g, h->fin_b, G, a, ch, s);
		conv_same(dt, a, ch, h->fin, 1, 1, B * Lf, Lf, nullptr, hb, 1, s);
		std::swap(x, hb);
		TTK_TRY(tap_out(depth + 1, x, (int64_t)B * Lf * E));
	}
	const int64_t rows = (int64_t)B * Lf;
	by_f32_bf16(dt, [&](auto t) {
		decltype(t)* at = (decltype(t)*)a;
		attn_blocks(dt, h->blocks, x, B, Lf, E, h->groups_emb, c.num_attn_heads, at, at + rows * E, at + rows * E * 4, s);
	});
	hipLaunchKernelGGL(k_cls_head, dim3((unsigned)B), dim3(256), 0, s, x, Lf, E, h->head_w, h->head_b, c.classes, emb_out, logits_out);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_cls_forward(ttk_cls* h, const float* audio, int B, int T, float* emb_out, float* logits_out, void* stream) {
	return ttk_cls_forward_taps(h, audio, B, T, emb_out, logits_out, nullptr, 0, stream);
}

}  // extern "C"
