// ttk_cond: the two conditioning-latent encoders behind the C ABI of include/ttk.h.
//   AR:        ConditioningEncoder       /root/reference/tortoise_tts/models/unified_voice.py:269-293 (1x1 conv + 6 AttentionBlocks, position 0)
//   diffusion: contextual_embedder       /root/reference/tortoise_tts/models/diffusion.py:1441-1447 (two stride-2 k=3 convs + 5 AttentionBlocks
//              of 2048 channels / 16 heads = head width 128, relative position bias), mean over positions :1477-1485
//   block:     AttentionBlock._forward   /root/reference/tortoise_tts/models/arch_utils.py:136-190 (+ QKVAttentionLegacy :59-94)
// One-off per voice (a few hundred mel frames), so this file reuses the dense GEMM and, for head width 64, the MFMA attention of
// the hot path, and adds plain kernels for what those do not cover: the strided stem (im2col), GroupNorm for any channels-per-group,
// attention for head width 128 (one wave per query row), and the pooling.  Layout: channels-last [b*T rows][C], f32 residual stream.
// The AttentionBlock (its GroupNorm, the row-wave attention, the block loop) lives in ttk_attn_block.h, shared with classifier.hip.
#include <stdlib.h>

#include "ttk_attn_block.h"
#include "ttk_common.h"
#include "ttk_host.h"

using namespace ttk;

namespace {

// rows of a strided 'same'-style convolution as GEMM operand: out[(b, t)][c * taps + j] = src[b][c][t * stride + j - pad] (0 outside),
// the k order of `weight.reshape(N, Cin * taps)`.  src is f32 with element strides (sb, sc, st): channels-first mel or channels-last rows.
template <typename T>
__global__ __launch_bounds__(256) void k_cond_im2col(const float* __restrict__ src, int64_t sb, int64_t sc, int64_t st, int Cin, int Tin, int Tout,
													 int taps, int stride, int pad, int Kpad, int64_t total, T* __restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= total) return;
	const int k = (int)(i % Kpad);
	const int64_t row = i / Kpad;
	const int t = (int)(row % Tout);
	const int64_t b = row / Tout;
	float v = 0.f;
	if (k < Cin * taps) {
		const int c = k / taps, j = k - c * taps, ts = t * stride + j - pad;
		if (ts >= 0 && ts < Tin) v = src[b * sb + c * sc + ts * st];
	}
	out[i] = cvt<T>(v);
}

// out[b][c] = mean over the T rows (mode 1) or row 0 (mode 0) of x f32 [b][T][C]
__global__ __launch_bounds__(256) void k_cond_pool(const float* __restrict__ x, int T, int C, int mode, float* __restrict__ out) {
	const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
	if (c >= C) return;
	const float* base = x + (int64_t)b * T * C + c;
	float s = base[0];
	if (mode) {
		for (int t = 1; t < T; ++t) s += base[(int64_t)t * C];
		s /= (float)T;
	}
	out[(int64_t)b * C + c] = s;
}

// The launches of the two kernels above, each described once: encode_t and the entry points on caller-provided operands both go through them.
template <typename T>
void launch_cond_im2col(const float* src, int64_t sb, int64_t sc, int64_t st, int nb, int Cin, int Tin, int Tout, int taps, int stride, int pad, int Kpad, T* out,
						hipStream_t s) {
	const int64_t total = (int64_t)nb * Tout * Kpad;
	hipLaunchKernelGGL((k_cond_im2col<T>), dim3(grid_for(total)), dim3(256), 0, s, src, sb, sc, st, Cin, Tin, Tout, taps, stride, pad, Kpad, total, out);
}
void launch_cond_pool(const float* x, int nb, int T, int C, int mode, float* out, hipStream_t s) {
	hipLaunchKernelGGL(k_cond_pool, dim3(grid_for(C), nb), dim3(256), 0, s, x, T, C, mode, out);
}

}  // namespace

struct ttk_cond {
	ttk_cond_config cfg;
	int dt, groups, hd;
	size_t es;
	Arena arena;
	Mat stem0, stem1;
	std::vector<Block> blocks;
	WsBuf ws;
};

namespace {

template <typename T>
int encode_t(ttk_cond* h, const float* mel, int b, int Tf, float* out, hipStream_t s) {
	const ttk_cond_config& c = h->cfg;
	const int C = c.channels, dt = h->dt;
	const int T1 = c.stem == TTK_COND_STEM_DOWN4 ? (Tf - 1) / 2 + 1 : Tf;
	const int T2 = c.stem == TTK_COND_STEM_DOWN4 ? (T1 - 1) / 2 + 1 : Tf;
	const int64_t rows = (int64_t)b * T2;
	TTK_REQUIRE(h->hd == 64 || T2 <= kRowWaveMaxT, TTK_E_ARG, "ttk_cond_encode: %d positions exceed the row-wave attention's LDS strip (%d)", T2, kRowWaveMaxT);
	// workspace: x f32 [rows][C] | a T [rows][C] | qkv T [rows][3C] | ao T [rows][C]; the stem's operands alias a/qkv/ao (free until block 0)
	const bool down4 = c.stem == TTK_COND_STEM_DOWN4;
	WsPlan stem, blk, ws;
	const size_t o_a0 = stem.take((size_t)b * T1 * h->stem0.Kpad * h->es), o_y = stem.take(down4 ? (size_t)b * T1 * (C / 2) * 4 : 0),
				 o_a1 = stem.take(down4 ? (size_t)rows * h->stem1.Kpad * h->es : 0);
	const size_t o_a = blk.take((size_t)rows * C * h->es), o_qkv = blk.take((size_t)rows * 3 * C * h->es), o_ao = blk.take((size_t)rows * C * h->es);
	const size_t o_x = ws.take((size_t)rows * C * 4), o_sp = ws.take(std::max(blk.total, stem.total));
	TTK_TRY(h->ws.reserve(ws.total));
	float* x = (float*)((char*)h->ws.p + o_x);
	char* sp = (char*)h->ws.p + o_sp;
	{
		T* a0 = (T*)(sp + o_a0);
		if (down4) {
			float* y = (float*)(sp + o_y);
			T* a1 = (T*)(sp + o_a1);
			launch_cond_im2col<T>(mel, (int64_t)c.in_channels * Tf, (int64_t)Tf, (int64_t)1, b, c.in_channels, Tf, T1, 3, 2, 1, h->stem0.Kpad, a0, s);
			gemm_plain(dt, a0, h->stem0.Kpad, h->stem0, b * T1, nullptr, y, 1, s);
			launch_cond_im2col<T>(y, (int64_t)T1 * (C / 2), (int64_t)1, (int64_t)(C / 2), b, C / 2, T1, T2, 3, 2, 1, h->stem1.Kpad, a1, s);
			gemm_plain(dt, a1, h->stem1.Kpad, h->stem1, (int)rows, nullptr, x, 1, s);
		} else {
			launch_cond_im2col<T>(mel, (int64_t)c.in_channels * Tf, (int64_t)Tf, (int64_t)1, b, c.in_channels, Tf, Tf, 1, 1, 0, h->stem0.Kpad, a0, s);
			gemm_plain(dt, a0, h->stem0.Kpad, h->stem0, (int)rows, nullptr, x, 1, s);
		}
	}
	attn_blocks<T>(dt, h->blocks, x, b, T2, C, h->groups, c.num_heads, (T*)(sp + o_a), (T*)(sp + o_qkv), (T*)(sp + o_ao), s);
	launch_cond_pool(x, b, T2, C, c.pool, out, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // namespace

extern "C" {

int ttk_cond_create(ttk_cond** out, const ttk_cond_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_cond_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16, TTK_E_ARG, "ttk_cond_create: bad dtype %d", cfg->dtype);
	TTK_REQUIRE(cfg->stem == TTK_COND_STEM_CONV1 || cfg->stem == TTK_COND_STEM_DOWN4, TTK_E_ARG, "ttk_cond_create: bad stem %d", cfg->stem);
	TTK_REQUIRE(cfg->num_heads >= 1 && cfg->channels % cfg->num_heads == 0 && cfg->channels % 128 == 0 && cfg->in_channels >= 1 && cfg->num_blocks >= 0,
				TTK_E_ARG, "ttk_cond_create: bad widths (channels %d, heads %d, in %d)", cfg->channels, cfg->num_heads, cfg->in_channels);
	const int hd = cfg->channels / cfg->num_heads;
	TTK_REQUIRE(hd == 64 || hd == 128, TTK_E_ARG, "ttk_cond_create: head width %d unsupported (64 or 128)", hd);
	std::unique_ptr<ttk_cond> h(new ttk_cond());
	h->cfg = *cfg;
	h->dt = cfg->dtype;
	h->es = dtype_size(h->dt);
	h->hd = hd;
	h->groups = gn_groups(cfg->channels);
	const int C = cfg->channels;
	WeightMap wm(w, n_w);
	if (cfg->stem == TTK_COND_STEM_DOWN4) {
		TTK_TRY(upload_mat(h->arena, wm, h->dt, "stem.0.weight", "stem.0.bias", PK_NK, C / 2, cfg->in_channels * 3, false, &h->stem0));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, "stem.1.weight", "stem.1.bias", PK_NK, C, (C / 2) * 3, false, &h->stem1));
	} else {
		TTK_TRY(upload_mat(h->arena, wm, h->dt, "stem.0.weight", "stem.0.bias", PK_NK, C, cfg->in_channels, false, &h->stem0));
	}
	TTK_TRY(upload_attn_blocks(h->arena, wm, h->dt, "blocks.", cfg->num_blocks, C, cfg->num_heads, cfg->relpos != 0, &h->blocks));
	hipError_t e = hipDeviceSynchronize();
	if (e != hipSuccess) { set_error("ttk_cond_create: %s", hipGetErrorString(e)); return TTK_E_HIP; }
	*out = h.release();
	return TTK_OK;
}

int ttk_cond_destroy(ttk_cond* h) {
	if (!h) return TTK_OK;
	(void)hipDeviceSynchronize();
	delete h;
	return TTK_OK;
}

int ttk_cond_encode(ttk_cond* h, const float* mel, int b, int T, float* out, void* stream) {
	TTK_REQUIRE(h && mel && out, TTK_E_ARG, "ttk_cond_encode: null argument");
	TTK_REQUIRE(b >= 1 && T >= 1, TTK_E_ARG, "ttk_cond_encode: empty input (b=%d T=%d)", b, T);
	TTK_REQUIRE(T <= 8192, TTK_E_ARG, "ttk_cond_encode: %d frames exceed the 8192-frame limit of a conditioning clip", T);
	return by_f32_bf16(h->dt, [&](auto t) { return encode_t<decltype(t)>(h, mel, b, T, out, (hipStream_t)stream); });
}

// ---- the AttentionBlock's and the stem's own kernels on caller-provided operands (tests/test_gpu_side_forms.py), through the launches encode_t and attn_blocks use
static bool side_dtype(int dtype) { return dtype == TTK_F32 || dtype == TTK_BF16; }
static bool aligned_to(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

int ttk_block_gn_rows(int dtype, const float* x, int nb, int T, int C, int groups, const float* gamma, const float* beta, void* out, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_block_gn_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(x && gamma && beta && out, TTK_E_ARG, "ttk_block_gn_rows: null argument");
	TTK_REQUIRE(nb >= 1 && nb <= 65535 && T >= 1 && C >= 1 && groups >= 1, TTK_E_ARG, "ttk_block_gn_rows: nb = %d, T = %d, C = %d, groups = %d out of range (each >= 1, nb <= 65535)", nb, T, C, groups);
	TTK_REQUIRE(C % groups == 0, TTK_E_ARG, "ttk_block_gn_rows: C = %d is not a multiple of groups = %d", C, groups);
	TTK_REQUIRE((int64_t)T * (C / groups) <= INT32_MAX, TTK_E_ARG, "ttk_block_gn_rows: %d rows x %d channels per group exceed one workgroup's int index", T, C / groups);
	TTK_REQUIRE(aligned_to(x, 4) && aligned_to(gamma, 4) && aligned_to(beta, 4) && aligned_to(out, dtype == TTK_BF16 ? 2 : 4), TTK_E_ARG,
				"ttk_block_gn_rows: an operand is misaligned for its element type");
	by_f32_bf16(dtype, [&](auto t) { using OT = decltype(t); launch_cond_gn<OT>(x, nb, T, C, groups, gamma, beta, (OT*)out, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_attn_rowwave(int dtype, const ttk_attn_desc* d, void* stream) {
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_attn_rowwave: null descriptor");
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_attn_rowwave: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(d->qkv && d->out, TTK_E_ARG, "ttk_attn_rowwave: null qkv or out");
	TTK_REQUIRE(!d->causal && !d->tlen && !d->out_f8 && d->form == 0, TTK_E_ARG, "ttk_attn_rowwave: causal, tlen, out_f8 and form are not served by the row-wave kernel");
	TTK_REQUIRE(d->nb >= 1 && d->nb <= 65535 && d->H >= 1 && d->H <= 65535, TTK_E_ARG, "ttk_attn_rowwave: nb = %d, H = %d out of range (1..65535)", d->nb, d->H);
	TTK_REQUIRE(d->T >= 1 && d->T <= kRowWaveMaxT, TTK_E_ARG, "ttk_attn_rowwave: T = %d outside 1..%d (the scores of 4 query rows live in LDS)", d->T, kRowWaveMaxT);
	TTK_REQUIRE(d->q_off >= 0 && d->k_off >= 0 && d->v_off >= 0 && d->head_stride >= 128, TTK_E_ARG, "ttk_attn_rowwave: negative offset or head_stride < 128 (the head width is 128)");
	const int64_t span = (int64_t)(d->H - 1) * d->head_stride + 128;
	TTK_REQUIRE(d->ld <= ((int64_t)1 << 30) && d->ldo <= ((int64_t)1 << 30) && d->q_off + span <= d->ld && d->k_off + span <= d->ld && d->v_off + span <= d->ld, TTK_E_ARG, "ttk_attn_rowwave: ld = %lld does not hold %d heads of width 128 at the given offsets",
				(long long)d->ld, d->H);
	TTK_REQUIRE(d->ldo >= (int64_t)d->H * 128, TTK_E_ARG, "ttk_attn_rowwave: ldo = %lld < H * 128", (long long)d->ldo);
	const size_t es = dtype == TTK_BF16 ? 2 : 4;
	TTK_REQUIRE(aligned_to(d->qkv, 8 * es) && d->ld % 8 == 0 && d->k_off % 8 == 0 && d->head_stride % 8 == 0, TTK_E_ARG,
				"ttk_attn_rowwave: k is read 8 elements at a time: qkv must be aligned to 8 elements (16-byte aligned at least) and ld, k_off, head_stride multiples of 8");
	TTK_REQUIRE(aligned_to(d->out, es) && (!d->bias || aligned_to(d->bias, 4)), TTK_E_ARG, "ttk_attn_rowwave: out or bias is misaligned for its element type");
	{
		const char *a = (const char*)d->qkv, *o = (const char*)d->out;
		const int64_t rows = (int64_t)d->nb * d->T;
		TTK_REQUIRE(!(a < o + rows * d->ldo * (int64_t)es && o < a + rows * d->ld * (int64_t)es), TTK_E_ARG, "ttk_attn_rowwave: qkv and out overlap");
	}
	AttnParams ap = {};
	ap.qkv = d->qkv; ap.ld = d->ld; ap.q_off = d->q_off; ap.k_off = d->k_off; ap.v_off = d->v_off; ap.head_stride = d->head_stride;
	ap.out = d->out; ap.ldo = d->ldo; ap.nb = d->nb; ap.T = d->T; ap.H = d->H; ap.causal = 0; ap.bias = d->bias; ap.scale = d->scale;
	by_f32_bf16(dtype, [&](auto t) { launch_attn_rowwave<decltype(t)>(ap, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_cond_im2col_rows(int dtype, const float* src, int64_t sb, int64_t sc, int64_t st, int nb, int Cin, int Tin, int Tout, int taps, int stride, int pad, int Kpad,
						 void* out, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_cond_im2col_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(src && out, TTK_E_ARG, "ttk_cond_im2col_rows: null argument");
	TTK_REQUIRE(nb >= 1 && Cin >= 1 && Tin >= 1 && Tout >= 1 && taps >= 1 && stride >= 1 && pad >= 0, TTK_E_ARG,
				"ttk_cond_im2col_rows: nb = %d, Cin = %d, Tin = %d, Tout = %d, taps = %d, stride = %d, pad = %d out of range", nb, Cin, Tin, Tout, taps, stride, pad);
	TTK_REQUIRE((int64_t)Cin * taps <= Kpad, TTK_E_ARG, "ttk_cond_im2col_rows: Kpad = %d < Cin * taps = %lld", Kpad, (long long)Cin * taps);
	TTK_REQUIRE((int64_t)(Tout - 1) * stride + taps <= INT32_MAX, TTK_E_ARG, "ttk_cond_im2col_rows: source positions exceed an int");
	TTK_REQUIRE((int64_t)nb * Tout * Kpad <= ((int64_t)1 << 38), TTK_E_ARG, "ttk_cond_im2col_rows: %d x %d x %d elements are too many for one launch", nb, Tout, Kpad);
	TTK_REQUIRE(sb >= 0 && sc >= 1 && st >= 1, TTK_E_ARG, "ttk_cond_im2col_rows: strides must be positive (sb = %lld, sc = %lld, st = %lld)", (long long)sb, (long long)sc, (long long)st);
	TTK_REQUIRE(aligned_to(src, 4) && aligned_to(out, dtype == TTK_BF16 ? 2 : 4), TTK_E_ARG, "ttk_cond_im2col_rows: src or out is misaligned for its element type");
	by_f32_bf16(dtype, [&](auto t) {
		using T = decltype(t);
		launch_cond_im2col<T>(src, sb, sc, st, nb, Cin, Tin, Tout, taps, stride, pad, Kpad, (T*)out, (hipStream_t)stream);
	});
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_cond_pool_rows(const float* x, int nb, int T, int C, int mode, float* out, void* stream) {
	TTK_REQUIRE(x && out, TTK_E_ARG, "ttk_cond_pool_rows: null argument");
	TTK_REQUIRE(nb >= 1 && nb <= 65535 && T >= 1 && C >= 1, TTK_E_ARG, "ttk_cond_pool_rows: nb = %d, T = %d, C = %d out of range (each >= 1, nb <= 65535)", nb, T, C);
	TTK_REQUIRE(mode == 0 || mode == 1, TTK_E_ARG, "ttk_cond_pool_rows: bad mode %d (0: position 0, 1: mean)", mode);
	TTK_REQUIRE(aligned_to(x, 4) && aligned_to(out, 4), TTK_E_ARG, "ttk_cond_pool_rows: x or out is misaligned");
	launch_cond_pool(x, nb, T, C, mode, out, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
