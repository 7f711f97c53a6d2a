// UnivNet generator (the TorToiSe "vocoder" of vocoder_type="vocoder") on the hot path's GEMM plus one new kernel, the
// location-variable convolution (LVC) with the gated update fused into its epilogue.
//
// Reference: tortoise_tts/models/vocoder.py -- KernelPredictor.forward :68-95, LVCBlock.forward :157-182,
// location_variable_convolution :184-218, UnivNetGenerator.forward :269-284, inference :302-314.
//
// Layout: channels-last everywhere.  The residual stream x is f32 [B * L][c_g]; GEMM A operands are T-typed with their channel count
// zero-padded to the weight matrix's Kpad (64), so no GEMM reads past a row.  Every Conv1d is the segment GEMM of ttk_conv.h (one
// segment per tap); the two reflect-padded convs (conv_pre, conv_post) run as 'valid' convolutions (shifts 0..6) over a copy of their
// input with the 3 reflected rows written on each side, and read their outputs back at the padded row stride.  convt_pre
// (ConvTranspose1d, kernel 2s, stride s) is s phase GEMMs of two taps each (convt_phases).  LeakyReLU(0.2) never runs inside a GEMM
// (gemm.hip has no such epilogue and stays as it is): it is applied where the next operand is written -- k_act_rows, or the LVC
// epilogue, which writes lrelu(x) for whatever reads x next (the next layer's dilated conv, the next block's convt_pre).
//
// LVC: per segment l (hop h rows) a small GEMM  O[t][n] = bias[l][n] + sum_kk Y[t][kk] W_l[kk][n],  Y = the (h + 2)-row window of
// lrelu(y) (the segment halo comes from the neighbouring rows, zero at the sequence ends), kk = (tap, input channel), 2 c_g output
// channels.  A workgroup owns 64 consecutive output rows of one batch element (8 segments at hop 8, one at hop 64, a quarter at hop
// 256) and stages their 66-row window in LDS; the predicted kernels are read from the kernel predictor's output, where one frame's
// [layer][in][out][tap] block is contiguous.
//  - bf16 mode, c_g = 32 (k_lvc_mfma): v_mfma_f32_16x16x32_bf16 with TIME as the M dimension: each wave owns a 16-row tile, A = the
//    bf16 window rows (one 16-byte LDS read per fragment, k-step = tap, k = input channel), B = W_l columns (n = output channel, 4
//    n-tiles of 16), 12 MFMAs per segment.  A tile that spans several segments (hop 8: two; hop 4: four) runs the 12 MFMAs once per
//    segment with the A rows of the other segments zeroed -- "h = 8 padded to 16 rows".  The sigmoid half (n-tiles 0, 1) and the tanh
//    half (n-tiles 2, 3) of an output land in the same lane, so the gate is computed in registers.
//  - f32 mode, and bf16 with c_g = 16 (k_lvc): exact f32 FMA, lane = row, wave w = channel slice [w c_g/4, (w+1) c_g/4) plus its tanh
//    partners; in bf16 mode the predicted kernels are bf16.
// Both write x (f32) and lrelu(x) (T-typed) in the epilogue.
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

constexpr float kSlope = 0.2f;          // lReLU_slope, every LeakyReLU of the generator
constexpr int kMelPad = 10;             // inference :305-306
constexpr float kMelPadValue = -11.5129f;

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * kSlope; }

// One activation / relayout pass into a T-typed GEMM operand [B * (L + 2 pad)][ldo] (channels >= C zero).  Source element (b, t, c)
// sits at src[b * sb + t * st + c * sc] for t < tvalid, frames [tvalid, L) read `fill` (the mel padding).  pad > 0: `pad` reflected
// rows on each side (F.pad(mode='reflect')).  act: LeakyReLU.  out32 (pad == 0 only): f32 [B * L][C] receives the value as well, or
// -- accumulate -- out32 += value and the T copy is written from the sum (the kernel predictor's `c = c + residual_conv(c)`).
struct ActRows {
	const float* src; int64_t sb, st, sc;
	int B, L, C, tvalid; float fill; int pad, act, accumulate;
	float* out32; void* outT; int ldo;
};

template <typename T>
__global__ void k_act_rows(ActRows p) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int Lp = p.L + 2 * p.pad;
	if (idx >= (int64_t)p.B * Lp * p.ldo) return;
	const int c = (int)(idx % p.ldo);
	const int64_t row = idx / p.ldo;
	const int b = (int)(row / Lp);
	int t = (int)(row - (int64_t)b * Lp) - p.pad;
	if (t < 0) t = -t;
	if (t > p.L - 1) t = 2 * (p.L - 1) - t;
	float v = 0.f;
	if (c < p.C) {
		v = t < p.tvalid ? p.src[(int64_t)b * p.sb + (int64_t)t * p.st + (int64_t)c * p.sc] : p.fill;
		if (p.act) v = lrelu(v);
		if (p.out32) {
			float* o = p.out32 + ((int64_t)b * p.L + t) * p.C + c;
			if (p.accumulate) v = *o + v;
			*o = v;
		}
	}
	((T*)p.outT)[idx] = cvt<T>(v);
}

// Location-variable convolution of layer `layer` + gated update (LVCBlock.forward :172-180, location_variable_convolution :184-218,
// always dilation 1):
//   o[t][n]  = bias[l][n] + sum_i sum_k lrelu(y)[t + k - 1][i] * kern[l][layer][i][n][k],   l = t / hop,  rows outside [0, L) zero
//   x[t][c] += sigmoid(o[t][c]) * tanh(o[t][c + CG]);   at[t][c] = T(lrelu(x[t][c]))
// y f32 [B * L][CG] (the dilated conv's output before its LeakyReLU), kern T [B * Tc][kstride], kbias f32 [B * Tc][bstride].
// Grid (ceil(L / 64), B), 256 threads.  See the file header for the tiling.  Both kernels run in isolation, against a float64 reference of this definition with a
// per-element bound, in tests/test_gpu_voc_forms.py (through ttk_lvc_rows below; the bound and a replica of the indexing: tests/voc_ref.py).
template <typename T, int CG>
__global__ __launch_bounds__(256) void k_lvc(const float* __restrict__ y, const T* __restrict__ kern, const float* __restrict__ kbias, float* x, T* at,
											 int L, int hop, int Tc, int layer, int kstride, int bstride, int lda) {
	constexpr int CPW = CG / 4;                 // output channels per wave (plus their tanh partners)
	constexpr int LAYER = CG * 2 * CG * 3;      // predicted values per layer and frame
	__shared__ float ys[66][CG + 1];
	const int b = blockIdx.y, t0 = blockIdx.x * 64;
	const float* yb = y + (int64_t)b * L * CG;
	for (int e = threadIdx.x; e < 66 * CG; e += 256) {
		const int r = e / CG, c = e - r * CG, t = t0 - 1 + r;
		ys[r][c] = (t >= 0 && t < L) ? lrelu(yb[(int64_t)t * CG + c]) : 0.f;
	}
	__syncthreads();
	const int r = threadIdx.x & 63, w = threadIdx.x >> 6, t = t0 + r;
	if (t >= L) return;
	const int64_t frame = (int64_t)b * Tc + t / hop;
	const T* wl = kern + frame * kstride + (int64_t)layer * LAYER + w * CPW * 3;
	float lo[CPW], hi[CPW];
#pragma unroll
	for (int j = 0; j < CPW; ++j) { lo[j] = 0.f; hi[j] = 0.f; }
#pragma unroll 4
	for (int i = 0; i < CG; ++i) {
		const float y0 = ys[r][i], y1 = ys[r + 1][i], y2 = ys[r + 2][i];
		const T* wi = wl + i * (2 * CG * 3);
#pragma unroll
		for (int j = 0; j < CPW; ++j) {
			lo[j] += y0 * (float)wi[3 * j] + y1 * (float)wi[3 * j + 1] + y2 * (float)wi[3 * j + 2];
			hi[j] += y0 * (float)wi[3 * (CG + j)] + y1 * (float)wi[3 * (CG + j) + 1] + y2 * (float)wi[3 * (CG + j) + 2];
		}
	}
	const float* bl = kbias + frame * bstride + layer * 2 * CG + w * CPW;
	const int64_t row = (int64_t)b * L + t;
	float* xr = x + row * CG + w * CPW;
	T* ar = at + row * lda + w * CPW;
#pragma unroll
	for (int j = 0; j < CPW; ++j) {
		const float a = lo[j] + bl[j], g = hi[j] + bl[CG + j];
		const float v = xr[j] + (1.f / (1.f + expf(-a))) * tanhf(g);
		xr[j] = v;
		ar[j] = cvt<T>(lrelu(v));
	}
}

// bf16, c_g = 32: the LVC of k_lvc on the MFMA (see the file header).  Same arguments, same grid (ceil(L / 64), B), 256 threads.
__global__ __launch_bounds__(256) void k_lvc_mfma(const float* __restrict__ y, const bf16* __restrict__ kern, const float* __restrict__ kbias,
												  float* x, bf16* at, int L, int hop, int Tc, int layer, int kstride, int bstride, int lda) {
	constexpr int CG = 32, LAYER = CG * 2 * CG * 3, LDY = 40;     // LDS row: 32 channels + 8 pad (80 bytes, 16-byte aligned rows)
	__shared__ __attribute__((aligned(16))) bf16 ys[66 * LDY];
	const int b = blockIdx.y, t0 = blockIdx.x * 64;
	const float* yb = y + (int64_t)b * L * CG;
	for (int e = threadIdx.x; e < 66 * CG; e += 256) {
		const int r = e / CG, c = e - r * CG, t = t0 - 1 + r;
		ys[r * LDY + c] = cvt<bf16>((t >= 0 && t < L) ? lrelu(yb[(int64_t)t * CG + c]) : 0.f);
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
	const int r0 = t0 + 16 * w;                                   // first row of this wave's tile (wave-uniform)
	if (r0 >= L) return;
	const int rlast = min(r0 + 15, L - 1);
	// A fragments: row r0 + l15 of the tile, k-step = tap, k = 8 g + j = input channel -> window row (16 w + l15 + tap)
	bf16x8 a[3];
#pragma unroll
	for (int tap = 0; tap < 3; ++tap) a[tap] = *(const bf16x8*)&ys[(16 * w + l15 + tap) * LDY + 8 * g];
	const int ta = r0 + l15;
	const bf16x8 zero = {};
	f32x4 acc[4];
#pragma unroll
	for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
	for (int seg = r0 / hop; seg <= rlast / hop; ++seg) {
		const bool own = ta < L && ta / hop == seg;               // this lane's A row belongs to segment seg
		const bf16* wl = kern + ((int64_t)b * Tc + seg) * kstride + (int64_t)layer * LAYER;
#pragma unroll
		for (int nt = 0; nt < 4; ++nt) {
			const int n = 16 * nt + l15;
#pragma unroll
			for (int tap = 0; tap < 3; ++tap) {
				bf16x8 bw;                                        // B[k = 8 g + j][n] = kern[i = 8 g + j][n][tap]
#pragma unroll
				for (int j = 0; j < 8; ++j) bw[j] = wl[(8 * g + j) * (2 * CG * 3) + n * 3 + tap];
				acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(own ? a[tap] : zero, bw, acc[nt], 0, 0, 0);
			}
		}
	}
	// D[row 4 g + i][col l15] of n-tile nt: time r0 + 4 g + i, channel 16 nt + l15; tanh partner in n-tile nt + 2
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int t = r0 + 4 * g + i;
		if (t >= L) continue;
		const float* bl = kbias + ((int64_t)b * Tc + t / hop) * bstride + layer * 2 * CG;
		const int64_t row = (int64_t)b * L + t;
#pragma unroll
		for (int nt = 0; nt < 2; ++nt) {
			const int n = 16 * nt + l15;
			const float av = acc[nt][i] + bl[n], gv = acc[nt + 2][i] + bl[n + CG];
			const float v = x[row * CG + n] + (1.f / (1.f + expf(-av))) * tanhf(gv);
			x[row * CG + n] = v;
			at[row * lda + n] = cvt<bf16>(lrelu(v));
		}
	}
}

struct KPred { Mat in, res[3][2], kernel, bias; };
struct LvcBlock { Mat convt; KPred kp; Mat conv[4]; };

}  // namespace

struct ttk_univnet {
	ttk_univnet_config cfg;
	int dt;
	size_t es;
	Arena arena;
	Mat conv_pre, conv_post;
	std::vector<LvcBlock> blocks;
	WsBuf ws;
};

namespace {

void launch_act(int dt, const ActRows& p, hipStream_t s) {
	const dim3 grid(grid_for((int64_t)p.B * (p.L + 2 * p.pad) * p.ldo));
	by_f32_bf16(dt, [&](auto t) { hipLaunchKernelGGL((k_act_rows<decltype(t)>), grid, dim3(256), 0, s, p); });
}
// channels-last f32 [B * L][C] rows (row stride st, batch stride sb) -> T operand
ActRows act_cl(const float* src, int64_t sb, int64_t st, int B, int L, int C, int act, int pad, void* outT, int ldo) {
	ActRows p = {};
	p.src = src; p.sb = sb; p.st = st; p.sc = 1; p.B = B; p.L = L; p.C = C; p.tvalid = L; p.pad = pad; p.act = act; p.outT = outT; p.ldo = ldo;
	return p;
}

template <typename T>
void launch_lvc_t(int cg, const float* y, const void* kern, const float* kbias, float* x, void* at, int B, int L, int hop, int Tc, int layer,
				  int kstride, int bstride, int lda, hipStream_t s) {
	const dim3 grid((unsigned)((L + 63) / 64), (unsigned)B);
	if (cg == 32 && sizeof(T) == 2)
		hipLaunchKernelGGL(k_lvc_mfma, grid, dim3(256), 0, s, y, (const bf16*)kern, kbias, x, (bf16*)at, L, hop, Tc, layer, kstride, bstride, lda);
	else if (cg == 32) hipLaunchKernelGGL((k_lvc<T, 32>), grid, dim3(256), 0, s, y, (const T*)kern, kbias, x, (T*)at, L, hop, Tc, layer, kstride, bstride, lda);
	else hipLaunchKernelGGL((k_lvc<T, 16>), grid, dim3(256), 0, s, y, (const T*)kern, kbias, x, (T*)at, L, hop, Tc, layer, kstride, bstride, lda);
}

std::string pfx(int i) { return "res_stack." + std::to_string(i) + "."; }

}  // namespace

extern "C" {

int ttk_univnet_create(ttk_univnet** out, const ttk_univnet_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_univnet_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16, TTK_E_ARG, "ttk_univnet_create: bad dtype %d (f32 or bf16)", cfg->dtype);
	TTK_REQUIRE(cfg->channels == 16 || cfg->channels == 32, TTK_E_ARG, "ttk_univnet_create: channel_size %d unsupported (16 or 32)", cfg->channels);
	TTK_REQUIRE(cfg->conv_kernel_size == 3, TTK_E_ARG, "ttk_univnet_create: LVC kernel size %d unsupported (3)", cfg->conv_kernel_size);
	TTK_REQUIRE(cfg->kpnet_conv_size >= 1 && cfg->kpnet_conv_size <= 11 && cfg->kpnet_conv_size % 2 == 1, TTK_E_ARG,
				"ttk_univnet_create: kpnet_conv_size %d unsupported (odd, <= 11)", cfg->kpnet_conv_size);
	TTK_REQUIRE(cfg->kpnet_hidden >= 1 && cfg->kpnet_hidden <= 512, TTK_E_ARG, "ttk_univnet_create: kpnet hidden width %d out of range", cfg->kpnet_hidden);
	TTK_REQUIRE(cfg->num_mels >= 1 && cfg->num_mels <= 256, TTK_E_ARG, "ttk_univnet_create: num_mels %d out of range", cfg->num_mels);
	TTK_REQUIRE(cfg->noise_dim >= 1 && cfg->noise_dim <= 256, TTK_E_ARG, "ttk_univnet_create: noise_dim %d out of range", cfg->noise_dim);
	TTK_REQUIRE(cfg->n_blocks >= 1 && cfg->n_blocks <= 4, TTK_E_ARG, "ttk_univnet_create: %d LVC blocks unsupported (1..4)", cfg->n_blocks);
	TTK_REQUIRE(cfg->n_layers >= 1 && cfg->n_layers <= 4, TTK_E_ARG, "ttk_univnet_create: %d dilations per block unsupported (1..4)", cfg->n_layers);
	int hop = 1;
	for (int i = 0; i < cfg->n_blocks; ++i) {
		TTK_REQUIRE(cfg->strides[i] >= 1 && cfg->strides[i] <= 16, TTK_E_ARG, "ttk_univnet_create: stride %d of block %d unsupported (1..16)", cfg->strides[i], i);
		hop *= cfg->strides[i];
	}
	TTK_REQUIRE(hop == cfg->hop_length, TTK_E_ARG, "ttk_univnet_create: the strides multiply to %d, not the hop length %d", hop, cfg->hop_length);
	for (int n = 0; n < cfg->n_layers; ++n)
		TTK_REQUIRE(cfg->dilations[n] >= 1 && cfg->dilations[n] <= 4096, TTK_E_ARG, "ttk_univnet_create: dilation %d unsupported", cfg->dilations[n]);
	std::unique_ptr<ttk_univnet> h(new ttk_univnet());
	h->cfg = *cfg;
	h->dt = cfg->dtype;
	h->es = dtype_size(h->dt);
	WeightMap wm(w, n_w);
	const int C = cfg->channels, H = cfg->kpnet_hidden, kc = cfg->kpnet_conv_size;
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "conv_pre.weight", "conv_pre.bias", PK_CONVK, C, cfg->noise_dim, false, &h->conv_pre, 7));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "conv_post.1.weight", "conv_post.1.bias", PK_CONVK, 1, C, false, &h->conv_post, 7));
	h->blocks.resize(cfg->n_blocks);
	for (int i = 0; i < cfg->n_blocks; ++i) {
		LvcBlock& B = h->blocks[i];
		const std::string p = pfx(i), kp = p + "kernel_predictor.";
		TTK_TRY(upload_mat(h->arena, wm, h->dt, p + "convt_pre.1.weight", p + "convt_pre.1.bias", PK_CONVT, C, C, false, &B.convt, 2 * cfg->strides[i]));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, kp + "input_conv.0.weight", kp + "input_conv.0.bias", PK_CONVK, H, cfg->num_mels, false, &B.kp.in, 5));
		for (int j = 0; j < 3; ++j)
			for (int m = 0; m < 2; ++m) {
				const std::string r = kp + "residual_convs." + std::to_string(j) + "." + std::to_string(1 + 2 * m) + ".";
				TTK_TRY(upload_mat(h->arena, wm, h->dt, r + "weight", r + "bias", PK_CONVK, H, H, false, &B.kp.res[j][m], kc));
			}
		TTK_TRY(upload_mat(h->arena, wm, h->dt, kp + "kernel_conv.weight", kp + "kernel_conv.bias", PK_CONVK, cfg->n_layers * C * 2 * C * 3, H, false, &B.kp.kernel, kc));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, kp + "bias_conv.weight", kp + "bias_conv.bias", PK_CONVK, cfg->n_layers * 2 * C, H, false, &B.kp.bias, kc));
		for (int n = 0; n < cfg->n_layers; ++n) {
			const std::string c = p + "conv_blocks." + std::to_string(n) + ".1.";
			TTK_TRY(upload_mat(h->arena, wm, h->dt, c + "weight", c + "bias", PK_CONVK, C, C, false, &B.conv[n], 3));
		}
	}
	*out = h.release();
	return TTK_OK;
}

int ttk_univnet_destroy(ttk_univnet* h) {
	if (!h) return TTK_OK;
	delete h;
	return TTK_OK;
}

int ttk_univnet_inference(ttk_univnet* h, const float* mel, const float* z, int B, int Tm, float* audio, void* stream) {
	TTK_REQUIRE(h && mel && z && audio, TTK_E_ARG, "ttk_univnet_inference: null argument");
	TTK_REQUIRE(B >= 1 && Tm >= 1, TTK_E_ARG, "ttk_univnet_inference: empty input (B=%d T=%d)", B, Tm);
	const ttk_univnet_config& c = h->cfg;
	hipStream_t s = (hipStream_t)stream;
	const int dt = h->dt;
	const size_t es = h->es;
	const int C = c.channels, H = c.kpnet_hidden, kc = c.kpnet_conv_size, hop = c.hop_length;
	const int T1 = Tm + kMelPad;                               // T' frames (mel with its padding, z)
	const int64_t Lmax = (int64_t)T1 * hop;
	TTK_REQUIRE((int64_t)B * (Lmax + 6) < ((int64_t)1 << 30), TTK_E_ARG, "ttk_univnet_inference: %d x %d frames is too long for one call", B, Tm);
	const int kst = c.n_layers * C * 2 * C * 3, bst = c.n_layers * 2 * C;
	const int lda = h->blocks[0].conv[0].Kpad;                  // operand width of every c_g-channel GEMM (64)
	const int mel_ld = h->blocks[0].kp.in.Kpad, hid_ld = h->blocks[0].kp.res[0][0].Kpad, z_ld = h->conv_pre.Kpad;
	const int64_t kern_el = (int64_t)B * T1 * kst;
	const int64_t x_el = (int64_t)B * Lmax * C, at_el = (int64_t)B * (Lmax + 6) * lda;
	TTK_REQUIRE(kern_el * (int64_t)es < ((int64_t)1 << 31) && at_el * 4 < ((int64_t)1 << 31), TTK_E_ARG,
				"ttk_univnet_inference: %d x %d frames exceed the 2 GiB buffer range of one call", B, Tm);
	WsPlan ws;
	const size_t o_kern = ws.take((size_t)kern_el * es), o_kb = ws.take((size_t)B * T1 * bst * 4);
	const size_t o_x = ws.take((size_t)x_el * 4), o_y = ws.take((size_t)std::max(std::max<int64_t>(x_el, (int64_t)B * (Lmax + 6)), (int64_t)B * (T1 + 6) * C) * 4);
	const size_t o_at = ws.take((size_t)at_el * es), o_mel = ws.take((size_t)B * T1 * mel_ld * es), o_z = ws.take((size_t)B * (T1 + 6) * z_ld * es);
	const size_t o_c = ws.take((size_t)B * T1 * H * 4), o_tmp = ws.take((size_t)B * T1 * H * 4), o_ct = ws.take((size_t)B * T1 * hid_ld * es),
				 o_ht = ws.take((size_t)B * T1 * hid_ld * es);
	TTK_TRY(h->ws.reserve(ws.total));
	char* base = (char*)h->ws.p;
	void* kern = base + o_kern;        // T [B*T'][kst]: predicted kernels of the current block
	float* kb = (float*)(base + o_kb); // f32 [B*T'][bst]: predicted biases
	float* x = (float*)(base + o_x);   // f32 [B*L][C]: residual stream
	float* y = (float*)(base + o_y);   // f32 GEMM outputs (conv_pre, dilated convs, conv_post)
	void* at = base + o_at;            // T [B*L][lda] (or reflect-padded [B*(L+6)][lda]): lrelu(x), the next GEMM's operand
	void* melt = base + o_mel;         // T [B*T'][mel_ld]
	void* zt = base + o_z;             // T [B*(T'+6)][z_ld]: z, reflect-padded
	float* kc32 = (float*)(base + o_c);   // kernel predictor stream f32 [B*T'][H]
	float* ktmp = (float*)(base + o_tmp); // f32 [B*T'][H]
	void* kct = base + o_ct;              // T copy of the stream [B*T'][hid_ld]
	void* kht = base + o_ht;              // T, inside a residual unit

	// mel [B][num_mels][T] -> T [B*T'][mel_ld] with the 10 padding frames; z [B][noise][T'] -> reflect-padded rows
	{
		ActRows p = {};
		p.src = mel; p.sb = (int64_t)c.num_mels * Tm; p.st = 1; p.sc = Tm; p.B = B; p.L = T1; p.C = c.num_mels; p.tvalid = Tm; p.fill = kMelPadValue;
		p.outT = melt; p.ldo = mel_ld;
		launch_act(dt, p, s);
		ActRows q = {};
		q.src = z; q.sb = (int64_t)c.noise_dim * T1; q.st = 1; q.sc = T1; q.B = B; q.L = T1; q.C = c.noise_dim; q.tvalid = T1; q.pad = 3;
		q.outT = zt; q.ldo = z_ld;
		launch_act(dt, q, s);
	}
	conv_valid(dt, zt, z_ld, h->conv_pre, 7, B * (T1 + 6), T1 + 6, y, s);                          // conv_pre -> y rows b*(T'+6) + t
	launch_act(dt, act_cl(y, (int64_t)(T1 + 6) * C, C, B, T1, C, 1, 0, at, lda), s);                // convt_pre's LeakyReLU
	int L = T1, cond_hop = 1;
	for (int i = 0; i < c.n_blocks; ++i) {
		const LvcBlock& blk = h->blocks[i];
		const int u = c.strides[i];
		cond_hop *= u;
		convt_phases(dt, at, lda, blk.convt, 2 * u, u, u / 2 + u % 2, B * L, L, x, s);       // convt_pre: kernel 2u, two taps per phase
		L *= u;
		const int M = B * L;
		// kernel predictor at mel rate
		{
			const int M1 = B * T1;
			conv_same(dt, melt, mel_ld, blk.kp.in, 5, 1, M1, T1, nullptr, ktmp, 1, s);
			ActRows p = act_cl(ktmp, (int64_t)T1 * H, H, B, T1, H, 1, 0, kct, hid_ld);
			p.out32 = kc32;
			launch_act(dt, p, s);                                                                     // c = lrelu(input_conv(mel))
			for (int j = 0; j < 3; ++j) {
				conv_same(dt, kct, hid_ld, blk.kp.res[j][0], kc, 1, M1, T1, nullptr, ktmp, 1, s);
				launch_act(dt, act_cl(ktmp, (int64_t)T1 * H, H, B, T1, H, 1, 0, kht, hid_ld), s);
				conv_same(dt, kht, hid_ld, blk.kp.res[j][1], kc, 1, M1, T1, nullptr, ktmp, 1, s);
				ActRows q = act_cl(ktmp, (int64_t)T1 * H, H, B, T1, H, 1, 0, kct, hid_ld);
				q.out32 = kc32; q.accumulate = 1;
				launch_act(dt, q, s);                                                                 // c = c + lrelu(conv(...))
			}
			conv_same(dt, kct, hid_ld, blk.kp.kernel, kc, 1, M1, T1, nullptr, kern, 0, s);                     // T [B*T'][kst]
			conv_same(dt, kct, hid_ld, blk.kp.bias, kc, 1, M1, T1, nullptr, kb, 1, s);                         // f32 [B*T'][bst]
		}
		launch_act(dt, act_cl(x, (int64_t)L * C, C, B, L, C, 1, 0, at, lda), s);                     // lrelu(x), first layer's operand
		for (int n = 0; n < c.n_layers; ++n) {
			conv_same(dt, at, lda, blk.conv[n], 3, c.dilations[n], M, L, nullptr, y, 1, s);                    // y = conv_d(lrelu(x)), f32
			by_f32_bf16(dt, [&](auto t) { launch_lvc_t<decltype(t)>(C, y, kern, kb, x, at, B, L, cond_hop, T1, n, kst, bst, lda, s); });
		}
		// `at` now holds lrelu(x): the next block's convt_pre operand
	}
	// conv_post: LeakyReLU, reflect pad 3, Conv1d(C -> 1, 7), Tanh; trim the padding frames' hops, clamp
	launch_act(dt, act_cl(x, (int64_t)L * C, C, B, L, C, 1, 3, at, lda), s);
	conv_valid(dt, at, lda, h->conv_post, 7, B * (L + 6), L + 6, y, s);
	hipLaunchKernelGGL(k_tanh_out<>, tanh_out_grid(B, Tm * hop), dim3(256), 0, s, y, B, L + 6, Tm * hop, audio);   // conv_post's Tanh, inference :312-313
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// One LVC launch on caller-provided operands (include/ttk.h), through launch_lvc_t: what k_lvc / k_lvc_mfma take for granted is refused here.
int ttk_lvc_rows(int dtype, const ttk_lvc_desc* d, void* stream) {
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_lvc_rows: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16, TTK_E_ARG, "ttk_lvc_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(d->y && d->kern && d->kbias && d->x && d->at, TTK_E_ARG, "ttk_lvc_rows: null argument (y, kern, kbias, x and at are all required)");
	TTK_REQUIRE(d->CG == 16 || d->CG == 32, TTK_E_ARG, "ttk_lvc_rows: CG = %d has no instantiation (16 or 32)", d->CG);
	TTK_REQUIRE(d->B >= 1 && d->B <= 65535 && d->L >= 1 && d->L <= (1 << 30), TTK_E_ARG, "ttk_lvc_rows: B = %d, L = %d out of range (B 1..65535, L 1..2^30)", d->B, d->L);
	TTK_REQUIRE(d->hop >= 1, TTK_E_ARG, "ttk_lvc_rows: hop = %d (must be >= 1)", d->hop);
	TTK_REQUIRE(d->Tc >= 1 && (d->L + d->hop - 1) / d->hop <= d->Tc, TTK_E_ARG, "ttk_lvc_rows: L = %d rows at hop %d need %d frames, Tc = %d", d->L, d->hop,
				(d->L + d->hop - 1) / d->hop, d->Tc);
	TTK_REQUIRE(d->n_layers >= 1 && d->n_layers <= 4 && d->layer >= 0 && d->layer < d->n_layers, TTK_E_ARG,
				"ttk_lvc_rows: layer %d of n_layers %d out of range (0 <= layer < n_layers <= 4)", d->layer, d->n_layers);
	TTK_REQUIRE(d->lda >= d->CG, TTK_E_ARG, "ttk_lvc_rows: lda < CG (%d < %d)", d->lda, d->CG);
	const size_t es = dtype == TTK_BF16 ? 2 : 4;
	TTK_REQUIRE(((uintptr_t)d->y & 3) == 0 && ((uintptr_t)d->kbias & 3) == 0 && ((uintptr_t)d->x & 3) == 0 && ((uintptr_t)d->kern & (es - 1)) == 0 &&
				((uintptr_t)d->at & (es - 1)) == 0, TTK_E_ARG, "ttk_lvc_rows: a buffer is misaligned for its element type");
	const int kstride = d->n_layers * d->CG * 2 * d->CG * 3, bstride = d->n_layers * 2 * d->CG;
	const size_t rows = (size_t)d->B * d->L, frames = (size_t)d->B * d->Tc;
	const size_t xb = rows * d->CG * 4, atb = rows * d->lda * es;
	auto overlap = [](const void* p, size_t n, const void* q, size_t m) { return (const char*)p < (const char*)q + m && (const char*)q < (const char*)p + n; };
	TTK_REQUIRE(!overlap(d->x, xb, d->y, xb) && !overlap(d->x, xb, d->kern, frames * kstride * es) && !overlap(d->x, xb, d->kbias, frames * bstride * 4), TTK_E_ARG,
				"ttk_lvc_rows: x overlaps an input (a workgroup reads its neighbours' rows of y while x is updated)");
	TTK_REQUIRE(!overlap(d->at, atb, d->y, xb) && !overlap(d->at, atb, d->x, xb) && !overlap(d->at, atb, d->kern, frames * kstride * es) &&
				!overlap(d->at, atb, d->kbias, frames * bstride * 4), TTK_E_ARG, "ttk_lvc_rows: at overlaps another operand");
	by_f32_bf16(dtype == TTK_BF16 ? DT_BF16 : DT_F32, [&](auto t) {
		launch_lvc_t<decltype(t)>(d->CG, d->y, d->kern, d->kbias, d->x, d->at, d->B, d->L, d->hop, d->Tc, d->layer, kstride, bstride, d->lda, (hipStream_t)stream);
	});
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
