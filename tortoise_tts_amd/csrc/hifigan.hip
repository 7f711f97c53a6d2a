// HiFiGAN generator (vocoder_type="hifigan"): the AR model's final_norm latents, one per mel token, straight to audio -- no diffusion.
//
// Reference: tortoise_tts/models/hifigan.py -- ResBlock1 :17-98, HifiganGenerator.forward :239-268, inference :270-296 (the two linear
// interpolations), built at models/__init__.py:126-138.
//
// Layout: channels-last rows, one utterance per call.  The residual stream is f32 [L][C]; every GEMM operand is a T-typed copy whose
// row holds round_up(C, 64) elements (the tail zero, it meets zero weight columns).  LeakyReLU is applied where such a copy is written,
// never inside a GEMM.  conv_pre, the transposed convolutions (u phase GEMMs of k / u taps each) and, in f32 mode or at
// C > 64, the ResBlock convolutions run on the segment GEMM of gemm.hip (ttk_conv.h: one segment per tap).  New kernels:
//  - k_hifi_interp: both interpolations of inference :285-294 in one pass, [n][C] f32 -> [F][C] T-typed, F = floor(4 n * 24000 / 22050).
//    align_corners=False with the scale factor itself as the coordinate scale: src = max((i + 0.5) / scale - 0.5, 0), right neighbour
//    clamped to the last frame; when a stage keeps the length (the second one for n = 1, 2) torch copies, and so does this kernel.
//  - k_hifi_conv_mfma (bf16, C = 32 or 64): a 'same' dilated Conv1d C -> C with TIME as the MFMA M dimension.  A workgroup owns 256
//    consecutive output rows: it stages their window plus (k - 1) / 2 * dilation halo rows on each side in LDS (zeros outside the
//    sequence) and the whole [k * C][C] weight matrix, pre-packed in B-fragment order (k = 11, C = 64: 88 KiB + 43 KiB of the 160 KiB).
//    Each wave owns 64 rows = four 16-row tiles x C / 16 column tiles; k-step = (tap, block of 32 input channels); one 16-byte LDS read
//    per fragment, every B fragment feeds four v_mfma_f32_16x16x32_bf16.  The epilogue adds the bias and, by mode,
//      0: writes lrelu(y) T-typed                                     (the first conv of a ResBlock pair)
//      1: x = y + residual, writes x f32 and lrelu(x) T-typed         (the second)
//      2 / 3: x = y + residual, sets / adds x into the stage's MRF sum (the last pair of a ResBlock: no separate gather of the three)
//  - k_hifi_post: LeakyReLU(0.01) -> conv_post (C -> 1, 7 taps) -> tanh as plain f32 FMA.
//  - k_hifi_cond: cond_layer(g), a 1x1 conv on a length-1 sequence, folded into conv_pre's bias once per utterance.
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

constexpr float kSlope = 0.1f;          // LRELU_SLOPE (hifigan.py:10)
constexpr float kSlopePost = 0.01f;     // F.leaky_relu's default, forward :265
constexpr int kTile = 256;              // output rows of a k_hifi_conv_mfma workgroup
constexpr int kLdsMax = 160 * 1024;

__device__ __forceinline__ float lrelu(float v, float s) { return v > 0.f ? v : v * s; }

// F.interpolate(mode="linear", scale_factor=s) source of output frame i in f32, as ATen computes it (rs = float(1 / s))
__device__ __forceinline__ void interp_src(int i, float rs, int size, int& i0, int& i1, float& l0, float& l1) {
	float r = rs * ((float)i + 0.5f) - 0.5f;
	if (r < 0.f) r = 0.f;
	i0 = min((int)r, size - 1);
	i1 = i0 + (i0 < size - 1 ? 1 : 0);
	l1 = r - (float)i0;
	l0 = 1.f - l1;
}
__device__ __forceinline__ float interp_up1(const float* lat, int C, int n, int j, int c) {
	int i0, i1; float l0, l1;
	interp_src(j, 0.25f, n, i0, i1, l0, l1);
	return l0 * lat[(int64_t)i0 * C + c] + l1 * lat[(int64_t)i1 * C + c];
}
// latents f32 [n][C] -> T [F][ldo] (columns >= C zero).  F == 4 n: the second interpolation is a copy.
template <typename T>
__global__ void k_hifi_interp(const float* lat, int n, int C, int F, float rs2, T* out, int ldo) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (int64_t)F * ldo) return;
	const int c = (int)(idx % ldo), f = (int)(idx / ldo);
	float v = 0.f;
	if (c < C) {
		const int F1 = 4 * n;
		if (F == F1) v = interp_up1(lat, C, n, f, c);
		else {
			int i0, i1; float l0, l1;
			interp_src(f, rs2, F1, i0, i1, l0, l1);
			v = l0 * interp_up1(lat, C, n, i0, c) + l1 * interp_up1(lat, C, n, i1, c);
		}
	}
	out[idx] = cvt<T>(v);
}

// out[c] = pre_bias[c] + cond_bias[c] + sum_k w[c][k] g[k]   (one wave per channel)
__global__ __launch_bounds__(64) void k_hifi_cond(const float* w, const float* cond_bias, const float* pre_bias, const float* g, int K, float* out) {
	const int c = blockIdx.x;
	float s = 0.f;
	for (int k = threadIdx.x; k < K; k += 64) s += w[(int64_t)c * K + k] * g[k];
	s = wave_sum(s);
	if (threadIdx.x == 0) out[c] = pre_bias[c] + (cond_bias[c] + s);
}

// T [rows][ldo] = lrelu(x f32 [rows][C]) (columns >= C zero)
template <typename T>
__global__ void k_hifi_act(const float* x, int C, float slope, T* out, int ldo, int64_t rows) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= rows * ldo) return;
	const int c = (int)(idx % ldo);
	const int64_t row = idx / ldo;
	out[idx] = cvt<T>(c < C ? lrelu(x[row * C + c], slope) : 0.f);
}

// o = (y0 [+ y1 + y2 + y3]) / div  (forward :258-264), f32 out [rows][C] + T copy lrelu(o) [rows][ldo] for the next transposed conv
template <typename T>
__global__ void k_hifi_mean(const float* y0, const float* y1, const float* y2, const float* y3, int n, float div, int C, float* out, T* out_t, int ldo,
							float slope, int64_t rows) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= rows * ldo) return;
	const int c = (int)(idx % ldo);
	const int64_t row = idx / ldo;
	float s = 0.f;
	if (c < C) {
		const int64_t i = row * C + c;
		s = y0[i];
		if (n > 1) s += y1[i];
		if (n > 2) s += y2[i];
		if (n > 3) s += y3[i];
		s = s / div;
		out[i] = s;
	}
	if (out_t) out_t[idx] = cvt<T>(lrelu(s, slope));
}

// audio[t] = tanh(b + sum_j sum_c lrelu(x[t + j - 3][c], 0.01) w[c][j])     (forward :265-267)
__global__ __launch_bounds__(256) void k_hifi_post(const float* __restrict__ x, int L, int C, const float* __restrict__ w, const float* __restrict__ b, float* audio) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	float* ws = (float*)smem;                           // [7][C]
	for (int e = threadIdx.x; e < 7 * C; e += 256) { const int j = e / C, c = e - j * C; ws[e] = w[c * 7 + j]; }
	__syncthreads();
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= L) return;
	float acc = b[0];
	for (int j = 0; j < 7; ++j) {
		const int tt = t + j - 3;
		if (tt < 0 || tt >= L) continue;
		const float4* xr = (const float4*)(x + (int64_t)tt * C);
		const float* wj = ws + j * C;
		for (int c4 = 0; c4 < C / 4; ++c4) {
			const float4 v = xr[c4];
			acc += lrelu(v.x, kSlopePost) * wj[4 * c4] + lrelu(v.y, kSlopePost) * wj[4 * c4 + 1] + lrelu(v.z, kSlopePost) * wj[4 * c4 + 2] +
				   lrelu(v.w, kSlopePost) * wj[4 * c4 + 3];
		}
	}
	audio[t] = tanhf(acc);
}

// bf16 [ntap][Npad][Kpad] (W_tap[n][k]) -> B-fragment order [tap][C / 32][C / 16][lane][8]: lane (l15, g) of (tap, kb, nt) holds
// W_tap[16 nt + l15][32 kb + 8 g + j], j = 0..7
__global__ void k_hifi_pack_frag(const bf16* w, int Npad, int Kpad, int C, int k, bf16* dst) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= k * C * C) return;
	const int NT = C / 16, KB = C / 32;
	const int j = idx & 7, lane = (idx >> 3) & 63;
	int rest = idx >> 9;
	const int nt = rest % NT; rest /= NT;
	const int kb = rest % KB, tap = rest / KB;
	const int l15 = lane & 15, g = lane >> 4;
	dst[idx] = w[((int64_t)tap * Npad + 16 * nt + l15) * Kpad + 32 * kb + 8 * g + j];
}

enum { HM_ACT = 0, HM_RES = 1, HM_MRF_SET = 2, HM_MRF_ADD = 3 };

// See the file header.  a bf16 [L][lda] (the operand copy), wfrag from k_hifi_pack_frag, grid ceil(L / 256), 256 threads,
// dynamic LDS = k C C * 2 + (256 + (k - 1) dil) * (C + 8) * 2 bytes.  xres may alias xout; at_out must not alias a.
// Packing, both widths and every mode run in isolation against a float64 convolution with a per-element bound in tests/test_gpu_voc_forms.py (through
// ttk_hifi_conv_rows below; the bound and a replica of the fragment order and the tiling: tests/voc_ref.py).
template <int C>
__global__ __launch_bounds__(256) void k_hifi_conv_mfma(const bf16* __restrict__ a, int lda, const bf16* __restrict__ wfrag, const float* __restrict__ bias,
														int L, int k, int dil, int mode, const float* xres, float* xout, bf16* at_out, int ldo, float* mrf) {
	constexpr int NT = C / 16, KB = C / 32, LDY = C + 8, C8 = C / 8;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	bf16* wl = (bf16*)smem;                               // k * C * C
	bf16* ys = wl + k * C * C;                            // R rows of LDY
	const int halo = (k - 1) / 2 * dil, R = kTile + 2 * halo;
	const int t0 = blockIdx.x * kTile;
	{
		const uint4* src = (const uint4*)wfrag;
		uint4* dst = (uint4*)wl;
		const int nw = k * C * C / 8;
		for (int e = threadIdx.x; e < nw; e += 256) dst[e] = src[e];
		for (int e = threadIdx.x; e < R * C8; e += 256) {
			const int r = e / C8, c8 = e - r * C8, t = t0 - halo + r;
			uint4 v = make_uint4(0u, 0u, 0u, 0u);
			if (t >= 0 && t < L) v = *(const uint4*)(a + (int64_t)t * lda + 8 * c8);
			*(uint4*)(ys + r * LDY + 8 * c8) = v;
		}
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
	const int r0 = t0 + 64 * w;                           // first row of this wave (wave-uniform)
	if (r0 >= L) return;
	f32x4 acc[4][NT];
#pragma unroll
	for (int mt = 0; mt < 4; ++mt)
#pragma unroll
		for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
	for (int tap = 0; tap < k; ++tap) {
		const bf16* yrow = ys + (64 * w + l15 + tap * dil) * LDY + 8 * g;
#pragma unroll
		for (int kb = 0; kb < KB; ++kb) {
			bf16x8 bw[NT];
#pragma unroll
			for (int nt = 0; nt < NT; ++nt) bw[nt] = *(const bf16x8*)(wl + ((((tap * KB + kb) * NT + nt) * 64 + lane) << 3));
#pragma unroll
			for (int mt = 0; mt < 4; ++mt) {
				const bf16x8 av = *(const bf16x8*)(yrow + 16 * mt * LDY + 32 * kb);
#pragma unroll
				for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bw[nt], acc[mt][nt], 0, 0, 0);
			}
		}
	}
	// D[row 4 g + i][col l15] of tile (mt, nt): time r0 + 16 mt + 4 g + i, channel 16 nt + l15
	float bn[NT];
#pragma unroll
	for (int nt = 0; nt < NT; ++nt) bn[nt] = bias[16 * nt + l15];
#pragma unroll
	for (int mt = 0; mt < 4; ++mt)
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int t = r0 + 16 * mt + 4 * g + i;
			if (t >= L) continue;
#pragma unroll
			for (int nt = 0; nt < NT; ++nt) {
				const int n = 16 * nt + l15;
				float v = acc[mt][nt][i] + bn[nt];
				const int64_t xi = (int64_t)t * C + n;
				if (mode != HM_ACT) v += xres[xi];
				if (mode == HM_MRF_SET) mrf[xi] = v;
				else if (mode == HM_MRF_ADD) mrf[xi] += v;
				else {
					if (mode == HM_RES) xout[xi] = v;
					at_out[(int64_t)t * ldo + n] = cvt<bf16>(lrelu(v, kSlope));
				}
			}
		}
}

struct ResBlock { Mat c1[3], c2[3]; bf16 *f1[3] = {nullptr, nullptr, nullptr}, *f2[3] = {nullptr, nullptr, nullptr}; int k = 3; int dil[3] = {1, 3, 5}; };

size_t narrow_lds(int C, int k, int dil) { return (size_t)k * C * C * 2 + (size_t)(kTile + (k - 1) * dil) * (C + 8) * 2; }

}  // namespace

struct ttk_hifigan {
	ttk_hifigan_config cfg;
	int dt;
	size_t es;
	Arena arena;
	Mat conv_pre;
	std::vector<Mat> ups;
	std::vector<ResBlock> blocks;
	std::vector<int> narrow;              // per stage: the ResBlocks run on k_hifi_conv_mfma
	float *cond_w = nullptr, *cond_b = nullptr, *pre_bias = nullptr;   // cond_layer [ch0][cond_channels], [ch0]; conv_pre.bias + cond_layer(g)
	float *post_w = nullptr, *post_b = nullptr;                        // conv_post [C][7], [1]
	bool cond_set = false;
	int hop = 1;
	WsBuf ws;
};

namespace {

void launch_act(int dt, const float* x, int C, void* out, int ldo, int64_t rows, hipStream_t s) {
	by_f32_bf16(dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k_hifi_act<T>), dim3(grid_for(rows * ldo)), dim3(256), 0, s, x, C, kSlope, (T*)out, ldo, rows); });
}
template <typename T>
void launch_mean_t(float* const* y, int n, float div, int C, float* out, void* out_t, int ldo, int64_t rows, hipStream_t s) {
	hipLaunchKernelGGL((k_hifi_mean<T>), dim3(grid_for(rows * ldo)), dim3(256), 0, s, y[0], y[1], y[2], y[3], n, div, C, out, (T*)out_t, ldo, kSlope, rows);
}

void launch_narrow(int C, const void* a, int lda, const bf16* wfrag, const float* bias, int L, int k, int dil, int mode, const float* xres, float* xout,
				   void* at_out, int ldo, float* mrf, hipStream_t s) {
	const size_t lds = narrow_lds(C, k, dil);
	const dim3 grid((unsigned)((L + kTile - 1) / kTile));
	if (C == 64) {
		(void)hipFuncSetAttribute((const void*)k_hifi_conv_mfma<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		hipLaunchKernelGGL(k_hifi_conv_mfma<64>, grid, dim3(256), lds, s, (const bf16*)a, lda, wfrag, bias, L, k, dil, mode, xres, xout, (bf16*)at_out, ldo, mrf);
	} else {
		(void)hipFuncSetAttribute((const void*)k_hifi_conv_mfma<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		hipLaunchKernelGGL(k_hifi_conv_mfma<32>, grid, dim3(256), lds, s, (const bf16*)a, lda, wfrag, bias, L, k, dil, mode, xres, xout, (bf16*)at_out, ldo, mrf);
	}
}

int pack_frag(Arena& ar, const Mat& m, int C, int k, bf16** out) {
	TTK_TRY(ar.alloc((void**)out, (size_t)k * C * C * 2));
	const int total = k * C * C;
	hipLaunchKernelGGL(k_hifi_pack_frag, dim3(grid_for(total)), dim3(256), 0, 0, (const bf16*)m.w, m.Npad, m.Kpad, C, k, *out);
	TTK_HIP(hipDeviceSynchronize());
	return TTK_OK;
}

// F.interpolate's output length floor(len * scale) in double arithmetic, twice (inference :285-294)
int hifi_frames(int n) { return (int)floor((double)(4 * (int64_t)n) * (24000.0 / 22050.0)); }

}  // namespace

extern "C" {

int ttk_hifigan_create(ttk_hifigan** out, const ttk_hifigan_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_hifigan_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16, TTK_E_ARG, "ttk_hifigan_create: bad dtype %d (f32 or bf16)", cfg->dtype);
	TTK_REQUIRE(cfg->resblock_type == 1, TTK_E_ARG, "ttk_hifigan_create: resblock_type \"%d\" unsupported (\"1\")", cfg->resblock_type);
	TTK_REQUIRE(cfg->cond_channels >= 1 && cfg->cond_channels <= 8192, TTK_E_ARG,
				"ttk_hifigan_create: cond_channels %d unsupported (the generator without a cond_layer is not built)", cfg->cond_channels);
	TTK_REQUIRE(cfg->in_channels >= 1 && cfg->in_channels <= 8192, TTK_E_ARG, "ttk_hifigan_create: in_channels %d out of range", cfg->in_channels);
	TTK_REQUIRE(cfg->n_ups >= 1 && cfg->n_ups <= 8 && cfg->n_kernels >= 1 && cfg->n_kernels <= 4, TTK_E_ARG,
				"ttk_hifigan_create: %d upsamplers / %d resblock kernels unsupported (1..8 / 1..4)", cfg->n_ups, cfg->n_kernels);
	int ch = cfg->upsample_initial_channel, hop = 1;
	TTK_REQUIRE(ch >= 16 && ch <= 4096, TTK_E_ARG, "ttk_hifigan_create: upsample_initial_channel %d out of range", ch);
	for (int i = 0; i < cfg->n_ups; ++i) {
		const int u = cfg->up_rate[i], k = cfg->up_kernel[i];
		TTK_REQUIRE(u >= 1 && k >= u && k % u == 0 && (k - u) % 2 == 0 && k / u <= 12, TTK_E_ARG,
					"ttk_hifigan_create: upsampler %d (kernel %d, stride %d) unsupported (the stride must divide the kernel, kernel - stride even)", i, k, u);
		TTK_REQUIRE(ch % 2 == 0, TTK_E_ARG, "ttk_hifigan_create: channel count %d does not halve", ch);
		ch /= 2;
		TTK_REQUIRE(ch % 8 == 0, TTK_E_ARG, "ttk_hifigan_create: stage %d has %d channels (must be a multiple of 8)", i, ch);
		hop *= u;
	}
	TTK_REQUIRE(ch <= 512, TTK_E_ARG, "ttk_hifigan_create: %d channels into conv_post unsupported (<= 512)", ch);
	for (int j = 0; j < cfg->n_kernels; ++j) {
		TTK_REQUIRE(cfg->rb_kernel[j] % 2 == 1 && cfg->rb_kernel[j] >= 1 && cfg->rb_kernel[j] <= 11, TTK_E_ARG,
					"ttk_hifigan_create: resblock kernel %d unsupported (odd, <= 11)", cfg->rb_kernel[j]);
		for (int m = 0; m < 3; ++m)
			TTK_REQUIRE(cfg->rb_dil[j][m] >= 1 && cfg->rb_dil[j][m] <= 4096, TTK_E_ARG, "ttk_hifigan_create: dilation %d unsupported", cfg->rb_dil[j][m]);
	}
	std::unique_ptr<ttk_hifigan> h(new ttk_hifigan());
	h->cfg = *cfg;
	h->dt = cfg->dtype;
	h->es = dtype_size(h->dt);
	h->hop = hop;
	const char* env = getenv("TTK_HIFI_NARROW");               // 0: the ResBlocks of every stage on the segment GEMM
	const bool want_narrow = h->dt == DT_BF16 && !(env && atoi(env) == 0);
	WeightMap wm(w, n_w);
	const int ch0 = cfg->upsample_initial_channel;
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "conv_pre.weight", "conv_pre.bias", PK_CONVK, ch0, cfg->in_channels, false, &h->conv_pre, 7));
	TTK_TRY(upload_f32(h->arena, wm, "cond_layer.weight", (int64_t)ch0 * cfg->cond_channels, &h->cond_w));
	TTK_TRY(upload_f32(h->arena, wm, "cond_layer.bias", ch0, &h->cond_b));
	TTK_TRY(h->arena.alloc((void**)&h->pre_bias, (size_t)ch0 * 4));
	h->ups.resize(cfg->n_ups);
	h->blocks.resize((size_t)cfg->n_ups * cfg->n_kernels);
	h->narrow.assign(cfg->n_ups, 0);
	ch = ch0;
	for (int i = 0; i < cfg->n_ups; ++i) {
		const std::string u = "ups." + std::to_string(i) + ".";
		TTK_TRY(upload_mat(h->arena, wm, h->dt, u + "weight", u + "bias", PK_CONVT, ch / 2, ch, false, &h->ups[i], cfg->up_kernel[i]));
		ch /= 2;
		bool nar = want_narrow && (ch == 32 || ch == 64);
		for (int j = 0; j < cfg->n_kernels && nar; ++j)
			for (int m = 0; m < 3; ++m) nar = nar && narrow_lds(ch, cfg->rb_kernel[j], cfg->rb_dil[j][m]) <= (size_t)kLdsMax;
		h->narrow[i] = nar ? 1 : 0;
		for (int j = 0; j < cfg->n_kernels; ++j) {
			ResBlock& b = h->blocks[(size_t)i * cfg->n_kernels + j];
			b.k = cfg->rb_kernel[j];
			const std::string p = "resblocks." + std::to_string(i * cfg->n_kernels + j) + ".";
			TTK_TRY(upload_resblock(h->arena, wm, h->dt, p, ch, b.k, b.c1, b.c2));
			for (int m = 0; m < 3; ++m) {
				b.dil[m] = cfg->rb_dil[j][m];
				if (nar) {
					TTK_TRY(pack_frag(h->arena, b.c1[m], ch, b.k, &b.f1[m]));
					TTK_TRY(pack_frag(h->arena, b.c2[m], ch, b.k, &b.f2[m]));
				}
			}
		}
	}
	TTK_TRY(upload_f32(h->arena, wm, "conv_post.weight", (int64_t)ch * 7, &h->post_w));
	TTK_TRY(upload_f32(h->arena, wm, "conv_post.bias", 1, &h->post_b));
	*out = h.release();
	return TTK_OK;
}

int ttk_hifigan_destroy(ttk_hifigan* h) {
	if (!h) return TTK_OK;
	delete h;
	return TTK_OK;
}

int ttk_hifigan_set_cond(ttk_hifigan* h, const float* g, void* stream) {
	TTK_REQUIRE(h && g, TTK_E_ARG, "ttk_hifigan_set_cond: null argument");
	hipLaunchKernelGGL(k_hifi_cond, dim3((unsigned)h->cfg.upsample_initial_channel), dim3(64), 0, (hipStream_t)stream, h->cond_w, h->cond_b, h->conv_pre.bias, g,
					   h->cfg.cond_channels, h->pre_bias);
	TTK_HIP(hipGetLastError());
	h->cond_set = true;
	return TTK_OK;
}

int ttk_hifigan_inference(ttk_hifigan* h, const float* latents, int n, float* audio, void* stream) {
	TTK_REQUIRE(h && latents && audio, TTK_E_ARG, "ttk_hifigan_inference: null argument");
	TTK_REQUIRE(n >= 1, TTK_E_ARG, "ttk_hifigan_inference: empty input (n=%d)", n);
	TTK_REQUIRE(n <= (1 << 16), TTK_E_ARG, "ttk_hifigan_inference: %d latents is too long for one call", n);
	TTK_REQUIRE(h->cond_set, TTK_E_ARG, "ttk_hifigan_inference: no conditioning latent set (ttk_hifigan_set_cond comes first)");
	const ttk_hifigan_config& c = h->cfg;
	hipStream_t s = (hipStream_t)stream;
	const int dt = h->dt;
	const size_t es = h->es;
	const int F = hifi_frames(n);
	const int ch0 = c.upsample_initial_channel, in_ld = h->conv_pre.Kpad;
	// workspace: the largest stage decides
	int64_t max_el = (int64_t)F * round_up(ch0, 64);
	{
		int64_t L = F; int ch = ch0;
		for (int i = 0; i < c.n_ups; ++i) { L *= c.up_rate[i]; ch /= 2; max_el = std::max(max_el, L * round_up(ch, 64)); }
	}
	TTK_REQUIRE(max_el * 4 < ((int64_t)1 << 31), TTK_E_ARG, "ttk_hifigan_inference: %d latents exceed the 2 GiB buffer range of one call", n);
	const int nxb = std::max(c.n_kernels, 2);
	WsPlan ws;
	const size_t f32b = (size_t)max_el * 4, tb = (size_t)max_el * es;
	const size_t o_in = ws.take((size_t)F * in_ld * es), o_xt = ws.take(tb), o_at = ws.take(tb), o_at2 = ws.take(tb), o_y = ws.take(f32b), o_h = ws.take(f32b);
	size_t o_xb[4];
	for (int j = 0; j < 4; ++j) o_xb[j] = j < nxb ? ws.take(f32b) : o_xb[0];
	TTK_TRY(h->ws.reserve(ws.total));
	char* base = (char*)h->ws.p;
	void* in_t = base + o_in;          // T [F][in_ld]: the interpolated latents
	void* xt = base + o_xt;            // T lrelu(stage input): the transposed conv's operand; then lrelu(y), the first operand of the stage's ResBlocks
	void* at = base + o_at;            // T operand of the ResBlock convs
	void* at2 = base + o_at2;          // T, between the two convs of a pair (k_hifi_conv_mfma route)
	float* y = (float*)(base + o_y);   // f32 transposed-conv output = input of the stage's ResBlocks; later the stage's MRF mean
	float* hb = (float*)(base + o_h);  // f32 output of conv_pre / convs1 (GEMM route)
	float* xb[4];
	for (int j = 0; j < 4; ++j) xb[j] = (float*)(base + o_xb[j]);

	{
		const int64_t total = (int64_t)F * in_ld;
		const float rs2 = (float)(1.0 / (24000.0 / 22050.0));
		by_f32_bf16(dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k_hifi_interp<T>), dim3(grid_for(total)), dim3(256), 0, s, latents, n, c.in_channels, F, rs2, (T*)in_t, in_ld); });
	}
	conv_taps(dt, in_t, in_ld, h->conv_pre, h->pre_bias, 7, -3, 1, F, F, nullptr, hb, 1, s);         // conv_pre + cond_layer(g), f32 [F][ch0]
	int L = F, ch = ch0;
	launch_act(dt, hb, ch, xt, round_up(ch, 64), L, s);
	for (int i = 0; i < c.n_ups; ++i) {
		const int u = c.up_rate[i], k = c.up_kernel[i];
		convt_phases(dt, xt, round_up(ch, 64), h->ups[i], k, u, (k - u) / 2, L, L, y, s);
		L *= u; ch /= 2;
		const int ld = round_up(ch, 64);
		const bool last = i == c.n_ups - 1;
		if (h->narrow[i]) {
			launch_act(dt, y, ch, xt, ld, L, s);                                             // lrelu(y): the first operand of all ResBlocks
			for (int j = 0; j < c.n_kernels; ++j) {
				const ResBlock& b = h->blocks[(size_t)i * c.n_kernels + j];
				for (int m = 0; m < 3; ++m) {
					launch_narrow(ch, m == 0 ? xt : at, ld, b.f1[m], b.c1[m].bias, L, b.k, b.dil[m], HM_ACT, nullptr, nullptr, at2, ld, nullptr, s);
					const int mode = m < 2 ? HM_RES : (j == 0 ? HM_MRF_SET : HM_MRF_ADD);
					launch_narrow(ch, at2, ld, b.f2[m], b.c2[m].bias, L, b.k, 1, mode, m == 0 ? y : xb[0], xb[0], at, ld, xb[1], s);
				}
			}
			float* const sum[4] = {xb[1], xb[1], xb[1], xb[1]};
			launch_mean_t<bf16>(sum, 1, (float)c.n_kernels, ch, y, last ? nullptr : xt, ld, L, s);
		} else {
			for (int j = 0; j < c.n_kernels; ++j) {
				const ResBlock& b = h->blocks[(size_t)i * c.n_kernels + j];
				const float* cur = y;
				for (int m = 0; m < 3; ++m) {
					launch_act(dt, cur, ch, at, ld, L, s);
					conv_same(dt, at, ld, b.c1[m], b.k, b.dil[m], L, L, nullptr, hb, 1, s);
					launch_act(dt, hb, ch, at, ld, L, s);
					conv_same(dt, at, ld, b.c2[m], b.k, 1, L, L, cur, xb[j], 1, s);   // + bias + residual (aliases the output from m = 1 on)
					cur = xb[j];
				}
			}
			by_f32_bf16(dt, [&](auto t) { launch_mean_t<decltype(t)>(xb, c.n_kernels, (float)c.n_kernels, ch, y, last ? nullptr : xt, ld, L, s); });
		}
	}
	hipLaunchKernelGGL(k_hifi_post, dim3(grid_for(L)), dim3(256), (size_t)7 * ch * 4, s, y, L, ch, h->post_w, h->post_b, audio);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// One k_hifi_conv_mfma launch on caller-provided operands (include/ttk.h).  The weights take the handle's route -- upload_mat with PK_CONVK, then pack_frag --
// into an arena of this call's own, freed after the stream has been synchronised; what the kernel takes for granted is refused before anything is allocated.
int ttk_hifi_conv_rows(const ttk_hifi_conv_desc* d, void* stream) {
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_hifi_conv_rows: null descriptor");
	TTK_REQUIRE(d->a && d->w && d->bias, TTK_E_ARG, "ttk_hifi_conv_rows: null argument (a, w and bias are required)");
	TTK_REQUIRE(d->C == 32 || d->C == 64, TTK_E_ARG, "ttk_hifi_conv_rows: C = %d has no instantiation (32 or 64)", d->C);
	TTK_REQUIRE(d->k >= 1 && d->k <= 11 && d->k % 2 == 1, TTK_E_ARG, "ttk_hifi_conv_rows: kernel size %d unsupported (odd, 1..11)", d->k);
	TTK_REQUIRE(d->dil >= 1 && d->dil <= 4096, TTK_E_ARG, "ttk_hifi_conv_rows: dilation %d unsupported (1..4096)", d->dil);
	TTK_REQUIRE(narrow_lds(d->C, d->k, d->dil) <= (size_t)kLdsMax, TTK_E_ARG, "ttk_hifi_conv_rows: C = %d, k = %d, dilation %d need %zu bytes of LDS (at most %d)", d->C,
				d->k, d->dil, narrow_lds(d->C, d->k, d->dil), kLdsMax);
	TTK_REQUIRE(d->L >= 1 && d->L <= (1 << 24), TTK_E_ARG, "ttk_hifi_conv_rows: L = %d out of range (1..2^24)", d->L);
	TTK_REQUIRE(d->lda >= d->C && d->lda % 8 == 0, TTK_E_ARG, "ttk_hifi_conv_rows: lda must be >= C and a multiple of 8 (lda %d, C %d)", d->lda, d->C);
	TTK_REQUIRE(((uintptr_t)d->a & 15) == 0, TTK_E_ARG, "ttk_hifi_conv_rows: a must be 16-byte aligned");
	TTK_REQUIRE(d->mode >= HM_ACT && d->mode <= HM_MRF_ADD, TTK_E_ARG, "ttk_hifi_conv_rows: mode %d unknown (0..3)", d->mode);
	const bool mrf_mode = d->mode == HM_MRF_SET || d->mode == HM_MRF_ADD;
	TTK_REQUIRE(d->mode == HM_ACT || d->xres, TTK_E_ARG, "ttk_hifi_conv_rows: mode %d needs xres", d->mode);
	TTK_REQUIRE(d->mode != HM_RES || d->xout, TTK_E_ARG, "ttk_hifi_conv_rows: mode 1 needs xout");
	TTK_REQUIRE(mrf_mode || d->at_out, TTK_E_ARG, "ttk_hifi_conv_rows: mode %d needs at_out", d->mode);
	TTK_REQUIRE(!mrf_mode || d->mrf, TTK_E_ARG, "ttk_hifi_conv_rows: mode %d needs mrf", d->mode);
	TTK_REQUIRE(mrf_mode || d->ldo >= d->C, TTK_E_ARG, "ttk_hifi_conv_rows: ldo < C (%d < %d)", d->ldo, d->C);
	TTK_REQUIRE(((uintptr_t)d->w & 3) == 0 && ((uintptr_t)d->bias & 3) == 0 && ((uintptr_t)d->xres & 3) == 0 && ((uintptr_t)d->xout & 3) == 0 &&
				((uintptr_t)d->mrf & 3) == 0 && ((uintptr_t)d->at_out & 1) == 0, TTK_E_ARG, "ttk_hifi_conv_rows: a buffer is misaligned for its element type");
	const size_t ab = (size_t)d->L * d->lda * 2, xb = (size_t)d->L * d->C * 4, ob = (size_t)d->L * (mrf_mode ? 0 : d->ldo) * 2;
	auto overlap = [](const void* p, size_t n, const void* q, size_t m) { return (const char*)p < (const char*)q + m && (const char*)q < (const char*)p + n; };
	TTK_REQUIRE(mrf_mode || !overlap(d->at_out, ob, d->a, ab), TTK_E_ARG, "ttk_hifi_conv_rows: at_out overlaps a (a workgroup reads its neighbours' rows of a)");
	TTK_REQUIRE(d->mode != HM_RES || !overlap(d->xout, xb, d->a, ab), TTK_E_ARG, "ttk_hifi_conv_rows: xout overlaps a");
	TTK_REQUIRE(!mrf_mode || !overlap(d->mrf, xb, d->a, ab), TTK_E_ARG, "ttk_hifi_conv_rows: mrf overlaps a");
	TTK_REQUIRE(d->mode != HM_RES || d->xout == d->xres || !overlap(d->xout, xb, d->xres, xb), TTK_E_ARG,
				"ttk_hifi_conv_rows: xout overlaps xres without being xres (only the element-for-element update is allowed)");
	TTK_REQUIRE(!mrf_mode || !overlap(d->mrf, xb, d->xres, xb), TTK_E_ARG, "ttk_hifi_conv_rows: mrf overlaps xres");
	TTK_REQUIRE(d->mode != HM_RES || (!overlap(d->at_out, ob, d->xout, xb) && !overlap(d->at_out, ob, d->xres, xb)), TTK_E_ARG,
				"ttk_hifi_conv_rows: at_out overlaps xres or xout");
	hipStream_t s = (hipStream_t)stream;
	Arena arena;
	ttk_weight_view view = {};
	view.name = "weight"; view.data = d->w; view.ndim = 3; view.shape[0] = d->C; view.shape[1] = d->C; view.shape[2] = d->k;
	WeightMap wm(&view, 1);
	Mat m;
	bf16* frag = nullptr;
	TTK_TRY(upload_mat(arena, wm, DT_BF16, "weight", "", PK_CONVK, d->C, d->C, false, &m, d->k));
	TTK_TRY(pack_frag(arena, m, d->C, d->k, &frag));
	launch_narrow(d->C, d->a, d->lda, frag, d->bias, d->L, d->k, d->dil, d->mode, d->xres, d->xout, d->at_out, d->ldo, d->mrf, s);
	const hipError_t e = hipGetLastError();
	TTK_HIP(hipStreamSynchronize(s));       // the launch reads `frag`: the arena goes only after it
	TTK_HIP(e);
	return TTK_OK;
}

}  // extern "C"
