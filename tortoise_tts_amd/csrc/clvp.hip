// CLVP candidate scoring on the kernels of the hot path.
//
// Reference: /root/reference/tortoise_tts/models/clvp.py:100-131 (CLVP.forward, return_loss=False) over two x-transformers encoders
// (models/xtransformers.py: ContinuousTransformerWrapper :1189-1248, AttentionLayers.forward :841-1015, Attention.forward :578-731,
// RMSNorm :337-346, FeedForward / GLU :431-478, rotary :266-290).  Per encoder layer:
//     x += to_out( softmax(rot(q) rot(k)^T / 8) rot(v) ),  q|k|v = rmsnorm(x) W_qkv   (bias-free; rotary on the first 32 features of q, k AND v)
//     x += W2 ( val * gelu(gate) ) + b2,                   val|gate = rmsnorm(x) W1 + b1
// then LayerNorm, mean over the sequence, a bias-free Linear, L2 normalisation; score = <text, speech> * exp(temperature).
// Dense GEMMs, attention and LayerNorm are the hot path's kernels; RMSNorm, rotary, GEGLU and the tail are the small kernels below.
#include <math.h>

#include <string>
#include <vector>

#include "ttk_common.h"
#include "ttk_conv.h"
#include "ttk_kernels.h"

using namespace ttk;

namespace {

__global__ void k_embed_rows(const float* emb, const int64_t* ids, int64_t n_ids_per_batch, int batch_stride_ids, float* out, int64_t rows, int d, int vocab) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int d4 = d / 4;
	if (idx >= rows * d4) return;
	const int64_t r = idx / d4;
	const int c = (int)(idx - r * d4) * 4;
	const int64_t b = r / n_ids_per_batch, t = r - b * n_ids_per_batch;
	int64_t id = ids[b * batch_stride_ids + t];
	id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);                 // the host validates ids; never index outside the table
	*(float4*)(out + r * d + c) = *(const float4*)(emb + id * d + c);
}

// RMSNorm (xtransformers.py:337-346): y = x / max(||x|| * d^-0.5, 1e-8) * g.  One wave per row.
template <typename T>
__global__ __launch_bounds__(256) void k_rmsnorm(const float* x, int64_t rows, int d, const float* g, T* y) {
	const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (row >= rows) return;
	const float* xr = x + row * d;
	float ss = 0.f;
	for (int c = lane * 4; c < d; c += 256) { const float4 v = *(const float4*)(xr + c); ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
	ss = wave_sum(ss);
	const float norm = fmaxf(sqrtf(ss) * rsqrtf((float)d), 1e-8f);
	T* yr = y + row * d;
	for (int c = lane * 4; c < d; c += 256) {
		const float4 v = *(const float4*)(xr + c), gg = *(const float4*)(g + c);
		yr[c] = cvt<T>(v.x / norm * gg.x); yr[c + 1] = cvt<T>(v.y / norm * gg.y); yr[c + 2] = cvt<T>(v.z / norm * gg.z); yr[c + 3] = cvt<T>(v.w / norm * gg.w);
	}
}

// rotary position embedding on the first 32 features of every head of q, k and v, in place on the fused projection [rows][3 * H * 64]:
// (x1, x2) halves of 16 -> (x1 cos - x2 sin, x2 cos + x1 sin), angle = position * inv_freq[i]   (xtransformers.py:266-290, 622-626)
template <typename T>
__global__ void k_rotary(T* qkv, int64_t rows, int S, int H, const float* inv_freq) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // (row, which * H + head, i < 16)
	const int per_row = 3 * H * 16;
	if (idx >= rows * per_row) return;
	const int64_t row = idx / per_row;
	const int rem = (int)(idx - row * per_row);
	const int hh = rem >> 4, i = rem & 15;
	const float ang = (float)(row % S) * inv_freq[i];
	float sn, cs;
	sincosf(ang, &sn, &cs);
	T* p = qkv + row * (int64_t)(3 * H * 64) + hh * 64 + i;
	const float x1 = (float)p[0], x2 = (float)p[16];
	p[0] = cvt<T>(x1 * cs - x2 * sn);
	p[16] = cvt<T>(x2 * cs + x1 * sn);
}

// GLU with exact GELU (xtransformers.py:431-440, nn.GELU()): out[r][c] = h[r][c] * gelu(h[r][inner + c])
template <typename T>
__global__ void k_geglu(const T* h, int64_t rows, int inner, T* out) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= rows * inner) return;
	const int64_t r = idx / inner;
	const int c = (int)(idx - r * inner);
	const float v = (float)h[r * 2 * inner + c], gt = (float)h[r * 2 * inner + inner + c];
	out[idx] = cvt<T>(v * (0.5f * gt * (1.0f + erff(gt * 0.70710678118654752f))));
}

// mean over the S positions of each batch element (masked_mean with an all-true mask, clvp.py:17-19,123-124) -> T [B][d]
template <typename T>
__global__ void k_mean_rows(const float* x, int B, int S, int d, T* out) {
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= B * d) return;
	const int b = idx / d, c = idx - b * d;
	float s = 0.f;
	for (int t = 0; t < S; ++t) s += x[((int64_t)b * S + t) * d + c];
	out[idx] = cvt<T>(s / (float)S);
}

// score[b] = <normalize(text[b or 0]), normalize(speech[b])> * exp(temperature)     (F.normalize eps 1e-12)
__global__ __launch_bounds__(64) void k_clvp_score(const float* tl, int Bt, const float* sl, int d, const float* temperature, float* scores) {
	const int b = blockIdx.x, lane = threadIdx.x;
	const float* t = tl + (int64_t)(Bt == 1 ? 0 : b) * d;
	const float* s = sl + (int64_t)b * d;
	float tt = 0.f, ss = 0.f, ts = 0.f;
	for (int c = lane; c < d; c += 64) { tt += t[c] * t[c]; ss += s[c] * s[c]; ts += t[c] * s[c]; }
	tt = wave_sum(tt); ss = wave_sum(ss); ts = wave_sum(ts);
	if (lane == 0) scores[b] = ts / (fmaxf(sqrtf(tt), 1e-12f) * fmaxf(sqrtf(ss), 1e-12f)) * expf(*temperature);
}

// The launches of the kernels above, each described once: encode_t / ttk_clvp_score and the entry points on caller-provided operands both go through them.
void launch_embed_rows(const float* emb, int vocab, int d, const int64_t* ids, int B, int S, int ids_stride, float* out, hipStream_t s) {
	const int64_t rows = (int64_t)B * S, total = rows * (d / 4);
	hipLaunchKernelGGL(k_embed_rows, dim3(grid_for(total)), dim3(256), 0, s, emb, ids, (int64_t)S, ids_stride, out, rows, d, vocab);
}
template <typename T>
void launch_rmsnorm(const float* x, int64_t rows, int d, const float* g, T* y, hipStream_t s) {
	hipLaunchKernelGGL((k_rmsnorm<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, d, g, y);
}
template <typename T>
void launch_rotary(T* qkv, int64_t rows, int S, int H, const float* inv_freq, hipStream_t s) {
	const int64_t total = rows * 3 * H * 16;
	hipLaunchKernelGGL((k_rotary<T>), dim3(grid_for(total)), dim3(256), 0, s, qkv, rows, S, H, inv_freq);
}
template <typename T>
void launch_geglu(const T* h, int64_t rows, int inner, T* out, hipStream_t s) {
	const int64_t total = rows * inner;
	hipLaunchKernelGGL((k_geglu<T>), dim3(grid_for(total)), dim3(256), 0, s, h, rows, inner, out);
}
template <typename T>
void launch_mean_rows(const float* x, int B, int S, int d, T* out, hipStream_t s) {
	hipLaunchKernelGGL((k_mean_rows<T>), dim3(grid_for(B * d)), dim3(256), 0, s, x, B, S, d, out);
}
void launch_clvp_score(const float* tl, int Bt, const float* sl, int B, int d, const float* temperature, float* scores, hipStream_t s) {
	hipLaunchKernelGGL(k_clvp_score, dim3(B), dim3(64), 0, s, tl, Bt, sl, d, temperature, scores);
}

struct EncLayer { float *g_attn = nullptr, *g_ff = nullptr; Mat qkv, out, ff1, ff2; };
struct Encoder { float* emb = nullptr; int vocab = 0; std::vector<EncLayer> L; float *norm_g = nullptr, *norm_b = nullptr; Mat to_latent; };

}  // namespace

struct ttk_clvp {
	ttk_clvp_config cfg;
	int dt;
	size_t es;
	Arena arena;
	Encoder text, speech;
	float *inv_freq = nullptr, *temperature = nullptr;
	WsBuf ws;
};

namespace {

// h->ws of a score call: the buffers of one encoder pass over at most `rows` rows (the two passes run one after the other), then both latents f32 [B][d]
struct Ws {
	size_t x, xn, qkv, ao, tl, sl, total;
	Ws(const ttk_clvp* h, size_t rows, size_t B) {
		const size_t d = h->cfg.dim, inner = h->cfg.inner;
		WsPlan p;
		x = p.take(rows * d * 4);                                     // [rows][d] f32 residual stream
		xn = p.take(rows * d * h->es);                                // [rows][d]
		qkv = p.take(rows * std::max(3 * d, 2 * inner) * h->es);      // [rows][3d]  (also the GLU projection [rows][2 * inner])
		ao = p.take(rows * std::max(d, inner) * h->es);               // [rows][max(d, inner)]
		tl = p.take(B * d * 4); sl = p.take(B * d * 4);
		total = p.total;
	}
};

template <typename T>
void encode_t(ttk_clvp* h, const Ws& w, const Encoder& e, const int64_t* ids, int B, int S, int ids_stride, float* latent /* [B][d] f32 */, hipStream_t s) {
	const ttk_clvp_config& c = h->cfg;
	const int d = c.dim, H = c.heads, inner = c.inner, dt = h->dt;
	const int64_t rows = (int64_t)B * S;
	char* base = (char*)h->ws.p;
	float* x = (float*)(base + w.x);
	T *xn = (T*)(base + w.xn), *qkv = (T*)(base + w.qkv), *ao = (T*)(base + w.ao);
	launch_embed_rows(e.emb, e.vocab, d, ids, B, S, ids_stride, x, s);
	for (const EncLayer& L : e.L) {
		launch_rmsnorm<T>(x, rows, d, L.g_attn, xn, s);
		gemm_plain(dt, xn, d, L.qkv, (int)rows, nullptr, qkv, 0, s);
		launch_rotary<T>(qkv, rows, S, H, h->inv_freq, s);
		AttnParams a = {};
		a.qkv = qkv; a.ld = 3 * d; a.q_off = 0; a.k_off = d; a.v_off = 2 * d; a.head_stride = 64; a.out = ao; a.ldo = d;
		a.nb = B; a.T = S; a.H = H; a.causal = 0; a.bias = nullptr; a.scale = 0.125f;
		launch_attn_fwd(dt, a, s);
		gemm_plain(dt, ao, d, L.out, (int)rows, x, x, 1, s);
		launch_rmsnorm<T>(x, rows, d, L.g_ff, xn, s);
		gemm_plain(dt, xn, d, L.ff1, (int)rows, nullptr, qkv, 0, s);
		launch_geglu<T>(qkv, rows, inner, ao, s);
		gemm_plain(dt, ao, inner, L.ff2, (int)rows, x, x, 1, s);
	}
	float* xf = (float*)qkv;                                         // final LayerNorm output, f32 [rows][d] (the qkv buffer is free now)
	launch_layernorm(dt, x, d, (int)rows, d, e.norm_g, e.norm_b, nullptr, nullptr, xf, d, 1, s);
	launch_mean_rows<T>(xf, B, S, d, xn, s);
	gemm_plain(dt, xn, d, e.to_latent, B, nullptr, latent, 1, s);
}

int upload_encoder(ttk_clvp* h, const WeightMap& wm, const std::string& which, int vocab, Encoder* e) {
	const ttk_clvp_config& c = h->cfg;
	const int d = c.dim;
	e->vocab = vocab;
	TTK_TRY(upload_f32(h->arena, wm, which + "_emb.weight", (int64_t)vocab * d, &e->emb));
	const std::string p = which + "_transformer.transformer.";
	e->L.resize(c.depth);
	for (int i = 0; i < c.depth; ++i) {
		EncLayer& L = e->L[i];
		const std::string a = p + "attn_layers.layers." + std::to_string(2 * i) + ".", f = p + "attn_layers.layers." + std::to_string(2 * i + 1) + ".";
		TTK_TRY(upload_f32(h->arena, wm, a + "0.0.g", d, &L.g_attn));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, a + "1.wrap.__qkv.weight", "", PK_NK, 3 * d, d, false, &L.qkv));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, a + "1.wrap.to_out.weight", a + "1.wrap.to_out.bias", PK_NK, d, d, false, &L.out));
		TTK_TRY(upload_f32(h->arena, wm, f + "0.0.g", d, &L.g_ff));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, f + "1.wrap.net.0.proj.weight", f + "1.wrap.net.0.proj.bias", PK_NK, 2 * c.inner, d, false, &L.ff1));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, f + "1.wrap.net.3.weight", f + "1.wrap.net.3.bias", PK_NK, d, c.inner, false, &L.ff2));
	}
	TTK_TRY(upload_f32(h->arena, wm, p + "norm.weight", d, &e->norm_g));
	TTK_TRY(upload_f32(h->arena, wm, p + "norm.bias", d, &e->norm_b));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "to_" + which + "_latent.weight", "", PK_NK, d, d, false, &e->to_latent));
	return TTK_OK;
}

}  // namespace

extern "C" {

int ttk_clvp_create(ttk_clvp** out, const ttk_clvp_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_clvp_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16, TTK_E_ARG, "ttk_clvp_create: bad dtype %d", cfg->dtype);
	TTK_REQUIRE(cfg->dim % 64 == 0 && cfg->heads * 64 == cfg->dim, TTK_E_ARG, "ttk_clvp_create: head width must be 64 with heads * 64 == dim (dim %d, heads %d)", cfg->dim, cfg->heads);
	TTK_REQUIRE(cfg->inner % 64 == 0 && cfg->depth >= 1, TTK_E_ARG, "ttk_clvp_create: inner width %d / depth %d unsupported", cfg->inner, cfg->depth);
	std::unique_ptr<ttk_clvp> h(new ttk_clvp());
	h->cfg = *cfg;
	h->dt = cfg->dtype;
	h->es = dtype_size(h->dt);
	WeightMap wm(w, n_w);
	TTK_TRY(upload_f32(h->arena, wm, "__rotary_inv_freq", 16, &h->inv_freq));
	TTK_TRY(upload_f32(h->arena, wm, "temperature", 1, &h->temperature));
	TTK_TRY(upload_encoder(h.get(), wm, "text", cfg->num_text_tokens, &h->text));
	TTK_TRY(upload_encoder(h.get(), wm, "speech", cfg->num_speech_tokens, &h->speech));
	*out = h.release();
	return TTK_OK;
}

int ttk_clvp_destroy(ttk_clvp* h) {
	if (!h) return TTK_OK;
	delete h;
	return TTK_OK;
}

int ttk_clvp_score(ttk_clvp* h, const int64_t* text, int Bt, int Tt, const int64_t* codes, int B, int M, float* scores, void* stream) {
	TTK_REQUIRE(h && text && codes && scores, TTK_E_ARG, "ttk_clvp_score: null argument");
	TTK_REQUIRE(B >= 1 && Tt >= 1 && M >= 1 && (Bt == 1 || Bt == B), TTK_E_ARG, "ttk_clvp_score: bad shape (Bt=%d Tt=%d B=%d M=%d)", Bt, Tt, B, M);
	const ttk_clvp_config& c = h->cfg;
	hipStream_t s = (hipStream_t)stream;
	const int d = c.dim;
	const Ws w(h, std::max((size_t)Bt * Tt, (size_t)B * M), B);
	TTK_TRY(h->ws.reserve(w.total));
	float *tl = (float*)((char*)h->ws.p + w.tl), *sl = (float*)((char*)h->ws.p + w.sl);
	by_f32_bf16(h->dt, [&](auto t) {
		using T = decltype(t);
		encode_t<T>(h, w, h->text, text, Bt, Tt, Tt, tl, s);
		encode_t<T>(h, w, h->speech, codes, B, M, M, sl, s);
	});
	launch_clvp_score(tl, Bt, sl, B, d, h->temperature, scores, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// ---- the encoders' small kernels on caller-provided operands (tests/test_gpu_side_forms.py), through the launches encode_t and ttk_clvp_score use
static bool side_dtype(int dtype) { return dtype == TTK_F32 || dtype == TTK_BF16; }
static bool aligned_to(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }
static const int64_t kMaxElems = (int64_t)1 << 38;      // elements of one launch: 2^30 workgroups of 256 threads

int ttk_clvp_embed_rows(const float* emb, int vocab, int d, const int64_t* ids, int B, int S, int batch_stride_ids, float* out, void* stream) {
	TTK_REQUIRE(emb && ids && out, TTK_E_ARG, "ttk_clvp_embed_rows: null argument");
	TTK_REQUIRE(vocab >= 1 && B >= 1 && S >= 1, TTK_E_ARG, "ttk_clvp_embed_rows: vocab = %d, B = %d, S = %d out of range (each >= 1)", vocab, B, S);
	TTK_REQUIRE(d >= 64 && d % 64 == 0, TTK_E_ARG, "ttk_clvp_embed_rows: d = %d is not a positive multiple of 64", d);
	TTK_REQUIRE(batch_stride_ids >= S, TTK_E_ARG, "ttk_clvp_embed_rows: batch_stride_ids = %d < S = %d", batch_stride_ids, S);
	TTK_REQUIRE((int64_t)B * S * d <= kMaxElems, TTK_E_ARG, "ttk_clvp_embed_rows: %d x %d x %d elements are too many for one launch", B, S, d);
	TTK_REQUIRE(aligned_to(emb, 16) && aligned_to(out, 16) && aligned_to(ids, 8), TTK_E_ARG, "ttk_clvp_embed_rows: emb and out must be 16-byte aligned (float4 copies), ids 8-byte aligned");
	launch_embed_rows(emb, vocab, d, ids, B, S, batch_stride_ids, out, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_clvp_rmsnorm_rows(int dtype, const float* x, int64_t rows, int d, const float* g, void* y, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_clvp_rmsnorm_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(x && g && y, TTK_E_ARG, "ttk_clvp_rmsnorm_rows: null argument");
	TTK_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 31), TTK_E_ARG, "ttk_clvp_rmsnorm_rows: rows = %lld out of range (1..2^31)", (long long)rows);
	TTK_REQUIRE(d >= 64 && d % 64 == 0, TTK_E_ARG, "ttk_clvp_rmsnorm_rows: d = %d is not a positive multiple of 64", d);
	TTK_REQUIRE(aligned_to(x, 16) && aligned_to(g, 16) && aligned_to(y, dtype == TTK_BF16 ? 2 : 4), TTK_E_ARG, "ttk_clvp_rmsnorm_rows: x and g must be 16-byte aligned (float4 loads), y for its element type");
	by_f32_bf16(dtype, [&](auto t) { using T = decltype(t); launch_rmsnorm<T>(x, rows, d, g, (T*)y, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_clvp_rotary_rows(int dtype, void* qkv, int B, int S, int H, const float* inv_freq, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_clvp_rotary_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(qkv && inv_freq, TTK_E_ARG, "ttk_clvp_rotary_rows: null argument");
	TTK_REQUIRE(B >= 1 && S >= 1 && H >= 1 && H <= 1024, TTK_E_ARG, "ttk_clvp_rotary_rows: B = %d, S = %d, H = %d out of range (each >= 1, H <= 1024)", B, S, H);
	TTK_REQUIRE((int64_t)B * S * 3 * H * 16 <= kMaxElems, TTK_E_ARG, "ttk_clvp_rotary_rows: %d x %d rows of %d heads are too many for one launch", B, S, H);
	TTK_REQUIRE(aligned_to(qkv, dtype == TTK_BF16 ? 2 : 4) && aligned_to(inv_freq, 4), TTK_E_ARG, "ttk_clvp_rotary_rows: qkv or inv_freq is misaligned for its element type");
	by_f32_bf16(dtype, [&](auto t) { using T = decltype(t); launch_rotary<T>((T*)qkv, (int64_t)B * S, S, H, inv_freq, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_clvp_geglu_rows(int dtype, const void* h, int64_t rows, int inner, void* out, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_clvp_geglu_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(h && out, TTK_E_ARG, "ttk_clvp_geglu_rows: null argument");
	TTK_REQUIRE(rows >= 1 && inner >= 1 && rows <= kMaxElems / inner, TTK_E_ARG, "ttk_clvp_geglu_rows: rows = %lld, inner = %d out of range", (long long)rows, inner);
	const int64_t es = dtype == TTK_BF16 ? 2 : 4;
	TTK_REQUIRE(aligned_to(h, es) && aligned_to(out, es), TTK_E_ARG, "ttk_clvp_geglu_rows: h or out is misaligned for its element type");
	TTK_REQUIRE(!((const char*)h < (const char*)out + rows * inner * es && (const char*)out < (const char*)h + rows * 2 * inner * es), TTK_E_ARG,
				"ttk_clvp_geglu_rows: h and out overlap");
	by_f32_bf16(dtype, [&](auto t) { using T = decltype(t); launch_geglu<T>((const T*)h, rows, inner, (T*)out, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_clvp_mean_rows(int dtype, const float* x, int B, int S, int d, void* out, void* stream) {
	TTK_REQUIRE(side_dtype(dtype), TTK_E_ARG, "ttk_clvp_mean_rows: bad dtype %d (f32 or bf16)", dtype);
	TTK_REQUIRE(x && out, TTK_E_ARG, "ttk_clvp_mean_rows: null argument");
	TTK_REQUIRE(B >= 1 && S >= 1 && d >= 64 && d % 64 == 0 && (int64_t)B * d <= ((int64_t)1 << 30), TTK_E_ARG,
				"ttk_clvp_mean_rows: B = %d, S = %d, d = %d out of range (B, S >= 1, d a positive multiple of 64, B * d <= 2^30)", B, S, d);
	TTK_REQUIRE(aligned_to(x, 4) && aligned_to(out, dtype == TTK_BF16 ? 2 : 4), TTK_E_ARG, "ttk_clvp_mean_rows: x or out is misaligned for its element type");
	by_f32_bf16(dtype, [&](auto t) { using T = decltype(t); launch_mean_rows<T>(x, B, S, d, (T*)out, (hipStream_t)stream); });
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_clvp_latent_score(const float* text_latents, int Bt, const float* speech_latents, int B, int d, const float* temperature, float* scores, void* stream) {
	TTK_REQUIRE(text_latents && speech_latents && temperature && scores, TTK_E_ARG, "ttk_clvp_latent_score: null argument");
	TTK_REQUIRE(B >= 1 && (Bt == 1 || Bt == B), TTK_E_ARG, "ttk_clvp_latent_score: bad shape (Bt = %d, B = %d: Bt == 1 or Bt == B)", Bt, B);
	TTK_REQUIRE(d >= 64 && d % 64 == 0, TTK_E_ARG, "ttk_clvp_latent_score: d = %d is not a positive multiple of 64", d);
	TTK_REQUIRE(aligned_to(text_latents, 4) && aligned_to(speech_latents, 4) && aligned_to(temperature, 4) && aligned_to(scores, 4), TTK_E_ARG,
				"ttk_clvp_latent_score: an operand is misaligned");
	launch_clvp_score(text_latents, Bt, speech_latents, B, d, temperature, scores, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
