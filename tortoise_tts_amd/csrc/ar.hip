// ttk_ar: the autoregressive half of the hot path -- UnifiedVoice's GPT-2 stack behind the C ABI of include/ttk.h.
//   prefill / latent pass : token-major dense pipeline (LayerNorm -> MFMA GEMM -> causal flash attention ...)
//   decode step           : 5 fused weight-streaming launches per layer + head, all position-dependent state read
//                           from a device scalar so the step is HIP-graph capturable
// Reference: /root/reference/tortoise_tts/models/unified_voice.py:98-254 (GPT2InferenceModel), :334-668 (UnifiedVoice),
//            HF:models/gpt2/modeling_gpt2.py:144-310,514-634 (GPT-2 block math).
#include "ttk_common.h"
#include "ttk_conv.h"

#include <algorithm>
#include <array>

using namespace ttk;

namespace {

struct ARLayer {
	float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
	Mat attn, proj, fc, proj2;
};

// rows of the prefill input: [cond | start_text, text.., stop_text | start_mel]      (unified_voice.py:639-649, :203-211)
// rows of the prefill: [cond | start_text, text.., stop_text | start_mel | prompt tokens (optional: prompted continuation, unified_voice.py:651-656)];
// the mel rows sit at mel positions 0, 1, ..., n_in   (GPT2InferenceModel.forward's first branch, unified_voice.py:203-211)
__global__ void k_build_prefill_emb(const float* cond, int Bc, const int64_t* text, int Tt, int B, int d,
									const float* text_emb, const float* text_pos, const float* mel_emb, const float* mel_pos,
									int start_text, int stop_text, int start_mel, float* out, const int64_t* prompt = nullptr, int prompt_rows = 0, int n_in = 0) {
	const int S = Tt + 4 + n_in;
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int d4 = d / 4;
	if (idx >= (int64_t)B * S * d4) return;
	const int c = (int)(idx % d4) * 4;
	const int64_t row = idx / d4;
	const int b = (int)(row / S), s = (int)(row - (int64_t)b * S);
	float4 v;
	if (s == 0) {
		v = *(const float4*)(cond + (int64_t)(Bc == 1 ? 0 : b) * d + c);
	} else if (s >= Tt + 3) {
		const int j = s - (Tt + 3);   // mel position: 0 = start_mel, j >= 1 = prompt token j - 1
		const int64_t tok = j == 0 ? start_mel : prompt[(int64_t)(prompt_rows == 1 ? 0 : b) * n_in + j - 1];
		const float4 e = *(const float4*)(mel_emb + tok * d + c), w = *(const float4*)(mel_pos + (int64_t)j * d + c);
		v = make_float4(e.x + w.x, e.y + w.y, e.z + w.z, e.w + w.w);
	} else {
		const int j = s - 1;   // position in [start, text.., stop]
		const int64_t tok = j == 0 ? start_text : (j == Tt + 1 ? stop_text : text[j - 1]);
		const float4 e = *(const float4*)(text_emb + tok * d + c), w = *(const float4*)(text_pos + (int64_t)j * d + c);
		v = make_float4(e.x + w.x, e.y + w.y, e.z + w.z, e.w + w.w);
	}
	*(float4*)(out + row * d + c) = v;
}

// rows of the latent pass: [cond | start_text, text.., stop_text | start_mel, codes.., stop_mel]   (unified_voice.py:576-593)
__global__ void k_build_latent_emb(const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, int d,
								   const float* text_emb, const float* text_pos, const float* mel_emb, const float* mel_pos,
								   int start_text, int stop_text, int start_mel, int stop_mel, float* out) {
	const int S = Tt + M + 5;
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int d4 = d / 4;
	if (idx >= (int64_t)B * S * d4) return;
	const int c = (int)(idx % d4) * 4;
	const int64_t row = idx / d4;
	const int b = (int)(row / S), s = (int)(row - (int64_t)b * S);
	float4 v;
	if (s == 0) {
		v = *(const float4*)(cond + (int64_t)b * d + c);
	} else if (s < Tt + 3) {
		const int j = s - 1;
		const int64_t tok = j == 0 ? start_text : (j == Tt + 1 ? stop_text : text[(int64_t)b * Tt + j - 1]);
		const float4 e = *(const float4*)(text_emb + tok * d + c), w = *(const float4*)(text_pos + (int64_t)j * d + c);
		v = make_float4(e.x + w.x, e.y + w.y, e.z + w.z, e.w + w.w);
	} else {
		const int j = s - (Tt + 3);   // position in [start, codes.., stop]
		const int64_t tok = j == 0 ? start_mel : (j == M + 1 ? stop_mel : codes[(int64_t)b * M + j - 1]);
		const float4 e = *(const float4*)(mel_emb + tok * d + c), w = *(const float4*)(mel_pos + (int64_t)j * d + c);
		v = make_float4(e.x + w.x, e.y + w.y, e.z + w.z, e.w + w.w);
	}
	*(float4*)(out + row * d + c) = v;
}

// targets of the scoring pass: build_aligned_inputs_and_targets (unified_voice.py:489-492) on the padded inputs of :577-578 -- [ids.., stop, stop] per sequence
__global__ void k_build_score_targets(const int64_t* text, int Tt, int stop_text, const int64_t* codes, int M, int stop_mel, int B, int64_t* tgt_text, int64_t* tgt_mel) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t nt = (int64_t)B * (Tt + 2), nm = (int64_t)B * (M + 2);
	if (idx < nt) {
		const int b = (int)(idx / (Tt + 2)), j = (int)(idx - (int64_t)b * (Tt + 2));
		tgt_text[idx] = j < Tt ? text[(int64_t)b * Tt + j] : stop_text;
	} else if (idx < nt + nm) {
		const int64_t i = idx - nt;
		const int b = (int)(i / (M + 2)), j = (int)(i - (int64_t)b * (M + 2));
		tgt_mel[i] = j < M ? codes[(int64_t)b * M + j] : stop_mel;
	}
}

}  // namespace

struct ttk_ar {
	ttk_ar_config cfg;
	int dt;                 // arithmetic type the kernels run in (DT_F32 / DT_BF16 / DT_F16)
	int wdt;                // storage type of the GPT-2 block matrices (== dt, or DT_FP8W)
	size_t es;
	Arena arena;
	std::vector<ARLayer> L;
	float *lnf_g, *lnf_b, *fn_g, *fn_b;
	Mat head;
	Mat text_head;          // ttk_ar_score only: uploaded when `text_head.weight` is among the weights (scoring); the mel head's dense copy is head.w
	bool scoring = false;
	float *text_emb, *mel_emb, *mel_pos, *text_pos;
	void *kc, *vc;          // [layers][max_batch][H][max_ctx][64]
	size_t kv_layer_stride; // elements
	int* d_pos;             // device: [0] valid cache rows, [1] rows of the shared prefix -- in the attention's position line when pos_slot >= 0, else at the start of the block that holds row_info
	int pos_slot = -1;
	int2* d_rowinfo;        // per candidate {first cache row, first candidate of its line}: line batches (ttk_ar_prefill_lines), prefixes right-aligned
	int lines_mode = 0;     // the current generation was started by ttk_ar_prefill_lines: the attention launches read d_rowinfo
	int rows_per_line = 0;  // ... with this many candidates per line (ttk_ar_reorder_cache_lines gathers inside a line only)
	float *x, *qbuf;        // decode residual stream / scaled queries [max_batch][d]
	void *attn_out, *hbuf;  // T, A-fragment order: [frag_rows][d] (attention output; the head's normalised rows), [frag_rows][4d] (MLP activations)
	void* x_frag = nullptr; // T copy of x in A-fragment order [m_tile][d/32][64][8]: operand of the folded-LayerNorm launches
	int poison = 0;         // TTK_DEBUG_POISON=1: the dense passes' scratch (ws_*) is filled with 0xFF when a prefill / latent pass ends -- nothing may read it afterwards
	int frag_rows = 0;      // rows attn_out / hbuf / x_frag were allocated (and zeroed) for: 16 * decode_row_tiles(max_batch)
	int shared_rows = 0;    // leading cache rows that are identical for all candidates of the current generation (AttnDecodeParams.shared_rows)
	// multinomial noise drawn by the mel-head launch (ttk_ar_set_noise): device RngArgs, per-row draw counters, q rows of this handle's candidates
	const int64_t* rng_args = nullptr; const int64_t* rng_draws = nullptr; float* rng_q = nullptr;
	int* d_health = nullptr;  // GemvParams.health of the folded launches (ttk_ar_health reads and clears it)
	float* ring_base = nullptr; const int64_t* ring_idx = nullptr; int64_t ring_stride = 0;      // ttk_ar_set_hidden_ring
	int64_t* d_ring = nullptr;                                                                 // device word holding ring_base: what the (possibly captured) launch reads
	int lnfold = 1;         // ln_1 + c_attn and ln_2 + c_fc of the decode step with the LayerNorm folded into the matrix (TTK_AR_LNFOLD=0: LN prologue, normalises in f32 first)
	int lean = 1;           // decode launches on the compile-time-specialised kernels of gemv.hip where one exists (TTK_AR_LEAN=0: k_skinny everywhere)
	WsBuf ws_x, ws_a, ws_qkv, ws_ao, ws_h;
	WsBuf ws_score;         // ttk_ar_score: row-major logits of both heads, targets, nll rows
	WsBuf ws_tap;           // ttk_ar_attentions / ttk_ar_text_attention: the device lists {head}, {output slot} of the selection
	std::vector<int> tap_host;      // ... and their host copy (alive until the upload has run)
	int B = 0, P = 0, k = 0, ready = 0;
	int Pmax = 0;           // longest prefix of the batch (capacity checks); == P for one line
	// run-time adapters (ttk_ar_lora_init / ttk_ar_lora_set): f32 masters of the 4 x layers block matrices, index 4 l + {0 c_attn, 1 attn.c_proj, 2 c_fc, 3 mlp.c_proj},
	// one f32 scratch of 4d x d, one T-typed scratch for the folded matrix, and which matrices currently hold an adapted copy
	bool lora_ready = false;
	std::vector<float*> lora_master;
	std::vector<char> lora_adapted;
	float* lora_scratch = nullptr;
	void* lora_wt = nullptr;
	~ttk_ar() { attn_pos_slot_release(pos_slot); }      // also the failure path of ttk_ar_create; the workspaces and the arena free themselves after this
};

// Debug aid: per-call scratch must not outlive its call.  A captured token step that kept reading one of these buffers would see
// NaN patterns from here on (tests/test_gpu_reuse.py runs the reuse scenarios under the flag).
static int poison_scratch(ttk_ar* h, hipStream_t s) {
	if (!h->poison) return TTK_OK;
	for (WsBuf* w : {&h->ws_x, &h->ws_a, &h->ws_qkv, &h->ws_ao, &h->ws_h, &h->ws_score})
		if (w->p) TTK_HIP(hipMemsetAsync(w->p, 0xFF, w->cap, s));
	return TTK_OK;
}

// A tap into the dense pass (ttk_ar_attentions, ttk_ar_text_attention): behind the c_attn GEMM of a layer with selected heads, k_attn_probs (align.hip) reads
// that layer's q and k columns from ws_qkv and writes the window [r0, r0 + R) x [c0, c0 + C) of each selected head's map; the pass ends behind layer `last`.
struct AttnTap {
	struct Layer { int first = 0, count = 0; float* out = nullptr; };      // entries [first, first + count) of the device lists; where this layer's maps go
	std::vector<Layer> layer;
	const int* heads = nullptr; const int* slots = nullptr;
	int n_out = 0, r0 = 0, R = 0, c0 = 0, C = 0, last = -1;
};

static int dense_forward(ttk_ar* h, float* x, int B, int S, bool write_kv, hipStream_t s, int kv_row0 = 0, int kv_t0 = 0, const AttnTap* tap = nullptr) {
	const int d = h->cfg.model_dim, H = h->cfg.heads, dt = h->dt;
	const int rows = B * S;
	TTK_TRY(h->ws_a.reserve((size_t)rows * d * h->es));
	TTK_TRY(h->ws_qkv.reserve((size_t)rows * 3 * d * h->es));
	TTK_TRY(h->ws_ao.reserve((size_t)rows * d * h->es));
	TTK_TRY(h->ws_h.reserve((size_t)rows * 4 * d * h->es));
	for (int l = 0; l < h->cfg.layers; ++l) {
		const ARLayer& L = h->L[l];
		launch_layernorm(dt, x, d, rows, d, L.ln1_g, L.ln1_b, nullptr, nullptr, h->ws_a.p, d, 0, s);
		launch_gemm(dt, dense_gemm(h->ws_a.p, d, L.attn, rows, h->ws_qkv.p, 0), s);
		if (write_kv) {
			const size_t row0 = (size_t)kv_row0 * H * h->cfg.max_ctx * 64;      // first candidate slice written
			char* kc = (char*)h->kc + ((size_t)l * h->kv_layer_stride + row0) * h->es;
			char* vc = (char*)h->vc + ((size_t)l * h->kv_layer_stride + row0) * h->es;
			launch_kv_scatter(dt, h->ws_qkv.p, B, S, H, kc, vc, h->cfg.max_ctx, s, kv_t0);
		}
		if (tap) {
			const AttnTap::Layer& t = tap->layer[l];
			if (t.count) {
				AttnProbsParams q = {};
				q.qkv = h->ws_qkv.p; q.ld = 3 * d; q.q_off = 0; q.k_off = d; q.head_stride = 64; q.scale = 0.125f; q.nb = B; q.T = S; q.H = H;
				q.heads = tap->heads + t.first; q.slots = tap->slots ? tap->slots + t.first : nullptr; q.n_sel = t.count; q.n_out = tap->n_out;
				q.r0 = tap->r0; q.R = tap->R; q.c0 = tap->c0; q.C = tap->C; q.out = t.out;
				launch_attn_probs(dt, q, s);
			}
			if (l == tap->last) return TTK_OK;
		}
		AttnParams a = {};
		a.qkv = h->ws_qkv.p; a.ld = 3 * d; a.q_off = 0; a.k_off = d; a.v_off = 2 * d; a.head_stride = 64;
		a.out = h->ws_ao.p; a.ldo = d; a.nb = B; a.T = S; a.H = H; a.causal = 1; a.bias = nullptr; a.scale = 0.125f;
		launch_attn_fwd(dt, a, s);
		gemm_plain(dt, h->ws_ao.p, d, L.proj, rows, x, x, 1, s);
		launch_layernorm(dt, x, d, rows, d, L.ln2_g, L.ln2_b, nullptr, nullptr, h->ws_a.p, d, 0, s);
		GemmParams fc = dense_gemm(h->ws_a.p, d, L.fc, rows, h->ws_h.p, 0);
		fc.act = ACT_GELU_NEW;
		launch_gemm(dt, fc, s);
		gemm_plain(dt, h->ws_h.p, 4 * d, L.proj2, rows, x, x, 1, s);
	}
	return TTK_OK;
}

namespace ttk {

// Waves per workgroup of the k_skinny launches (k_gemv's are template parameters that repeat them).  A wave requests its operands in batches of 8 k-steps
// (4 in f32), so K / 32 / waves should be a multiple of that: with 8 waves on K = 1024 every bf16 wave owned 4 k-steps and half of its 16 load
// instructions re-read the last fragment -- on a path bound by what a CU can take in.  More than 8 lose again (16 partial tiles to merge through LDS):
// 4 (K = 1024) / 8 (K = 4096) measured best in the 250-token loop (bf16, B = 16).  f32: batches of 4 k-steps, 32 / 4 = 8 waves; K = 4096: 4 batches each.
// LN prologue: 8 waves x 2 rows normalise 16 candidates in one pass.  The head has 513 n-tiles: two 8-wave workgroups fit a CU (512 slots), so tile 513
// ran as a second round on an empty chip; five 4-wave ones fit and the tiles run as one round.  Small models: 4 everywhere.
int skinny_waves(int role, bool ln_prologue, int dt, int d) {
	if (d < 1024 || role == DR_HEAD) return 4;
	if (ln_prologue || dt == DT_F32) return 8;
	return role == DR_PROJ2 ? 8 : 4;
}

int decode_launch(const DecodeCtx& c, const DecodeLaunch& L, int M, hipStream_t s) {
	const Mat& W = *L.W;
	const bool fold = c.lnfold && (L.role == DR_QKV || L.role == DR_FC);      // x_frag times gamma o W, the norm finished in the epilogue
	const bool prologue = L.ln_g && !fold;                                     // f32 rows of L.x normalised inside the launch
	const bool residual = L.role == DR_PROJ || L.role == DR_PROJ2;
	GemvParams g = {};
	g.Wp = fold ? W.wfrag_fold : W.wfrag; g.bias = fold ? W.bias_fold : W.bias; g.csum = fold ? W.csum : nullptr;
	g.w8 = fold ? 0 : W.w8; g.wscale = W.wscale;       // (fp8 weights: the fold is kept in bf16)
	g.a = L.a; g.out_f32 = L.out_f32; g.out_T = L.out_T; g.M = M; g.N = L.N; g.K = L.K; g.row0 = 0;
	if (fold) g.health = c.health;
	if (L.role == DR_QKV) { g.qbuf = L.qbuf; g.kcache = L.kc; g.vcache = L.vc; g.d_pos = L.d_pos; g.max_ctx = L.max_ctx; g.H = L.H; g.q_scale = 0.125f; }
	if (L.role == DR_HEAD) { g.d_pos = L.bump ? L.d_pos : nullptr; g.noise = c.rng_q; g.rng = c.rng_args; g.draws = c.rng_draws; }
	const int gv = L.role == DR_QKV ? GV_QKV : (L.role == DR_FC ? GV_FC : (L.role == DR_HEAD ? GV_HEAD : GV_PROJ));
	// the ONE place that decides between the kernel families: launch_gemv declines (gemv_supported) what it has no instantiation for
	if (c.family == 2 || (c.family == 0 && c.lean && c.lnfold && !prologue)) {
		if (!prologue && launch_gemv(c.dt, gv, g, s)) { if (c.launched) *c.launched = 2; return TTK_OK; }
		TTK_REQUIRE(c.family != 2, TTK_E_ARG, "decode_launch: k_gemv has no instantiation for this launch");
	}
	SkinnyParams p = {};
	p.Wp = g.Wp; p.w8 = g.w8; p.wscale = g.wscale; p.N = L.N; p.K = L.K; p.M = M; p.bias = g.bias;
	if (prologue) { p.ln_count = L.ln2_g ? 2 : 1; p.x = L.x; p.ldx = L.ldx; p.g1 = L.ln_g; p.b1 = L.ln_b; p.g2 = L.ln2_g; p.b2 = L.ln2_b; }
	else { p.a = L.a; p.g1 = g.csum; p.health = g.health; }
	p.mode = L.role == DR_QKV ? SK_QKV : (L.role == DR_FC ? SK_ACT_T : (residual ? SK_RESIDUAL : SK_STORE_F32));
	p.act = L.role == DR_FC ? ACT_GELU_NEW : ACT_NONE;
	p.out_f32 = L.out_f32; p.ldc = L.N; p.out_T = L.out_T;
	p.qbuf = g.qbuf; p.kcache = g.kcache; p.vcache = g.vcache; p.max_ctx = g.max_ctx; p.H = g.H; p.q_scale = g.q_scale; p.d_pos = g.d_pos;
	p.noise = g.noise; p.rng = g.rng; p.draws = g.draws;
	const int waves = c.waves ? c.waves : skinny_waves(L.role, prologue, c.dt, c.model_dim);
	const hipError_t e = launch_skinny(c.dt, p, waves, s);
	if (e != hipSuccess) {
		const size_t lds = skinny_lds_bytes(c.dt, decode_row_tiles(M), L.K, skinny_launch_waves(waves, prologue), prologue ? SKF_PROLOGUE : (fold ? SKF_FOLD : SKF_PLAIN));
		set_error("decode launch over M=%d rows, K=%d (%zu bytes of LDS; a compute unit has %zu) was not launched: %s", M, L.K, lds, CU_LDS_BYTES, hipGetErrorString(e));
		return lds > CU_LDS_BYTES ? TTK_E_ARG : TTK_E_HIP;
	}
	if (c.launched) *c.launched = 1;
	return TTK_OK;
}

}  // namespace ttk

static DecodeCtx decode_ctx(const ttk_ar* h) {
	return DecodeCtx{h->dt, h->lnfold, h->lean, h->cfg.model_dim, h->d_health, h->rng_args, h->rng_draws, h->rng_q, 0, 0, nullptr};
}

// the prefill's head: ln_f + final_norm + mel_head on the f32 rows h->x [B][d], the norms inside the launch (once per utterance; the decode step splits them off)
static int head_launch(ttk_ar* h, int B, float* logits, hipStream_t s) {
	DecodeLaunch L = {DR_HEAD, &h->head, h->cfg.number_mel_codes, h->cfg.model_dim};
	L.ln_g = h->lnf_g; L.ln_b = h->lnf_b; L.ln2_g = h->fn_g; L.ln2_b = h->fn_b; L.out_f32 = logits;
	L.x = h->x; L.ldx = h->cfg.model_dim;
	return decode_launch(decode_ctx(h), L, B, s);
}

// one decode step of the whole batch on stream s: layers x {ln_1+c_attn+KV append, attention, c_proj+res, ln_2+c_fc+gelu, mlp.c_proj+res} + ln_f/final_norm + mel_head
static int decode_rows(ttk_ar* h, float* logits_out, float* hidden_out, hipStream_t s) {
	const ttk_ar_config& c = h->cfg;
	const int d = c.model_dim, B = h->B, dt = h->dt;
	const DecodeCtx ctx = decode_ctx(h);
	void* xf = h->lnfold ? h->x_frag : nullptr;      // T copy of the residual rows: written by the projections, operand of the folded launches
	for (int l = 0; l < c.layers; ++l) {
		const ARLayer& L = h->L[l];
		char* kc = (char*)h->kc + (size_t)l * h->kv_layer_stride * h->es;
		char* vc = (char*)h->vc + (size_t)l * h->kv_layer_stride * h->es;
		DecodeLaunch qkv = {DR_QKV, &L.attn, 3 * d, d, h->x_frag, L.ln1_g, L.ln1_b};
		qkv.kc = kc; qkv.vc = vc; qkv.x = h->x; qkv.ldx = d; qkv.qbuf = h->qbuf; qkv.d_pos = h->d_pos; qkv.max_ctx = c.max_ctx; qkv.H = c.heads;
		TTK_TRY(decode_launch(ctx, qkv, B, s));
		AttnDecodeParams a = {};
		a.qbuf = h->qbuf; a.kcache = kc; a.vcache = vc; a.d_pos = h->d_pos; a.pos_slot_p1 = h->pos_slot + 1; a.B = B; a.H = c.heads; a.max_ctx = c.max_ctx; a.ctx_hint = h->P + 2 + h->k;
		a.out = h->attn_out; a.out_frag = 1; a.shared_rows = 1; a.row_info = h->lines_mode ? h->d_rowinfo : nullptr;
		launch_attn_decode(dt, a, s);
		DecodeLaunch proj = {DR_PROJ, &L.proj, d, d, h->attn_out};
		proj.out_f32 = h->x; proj.out_T = xf;
		TTK_TRY(decode_launch(ctx, proj, B, s));
		DecodeLaunch fc = {DR_FC, &L.fc, 4 * d, d, h->x_frag, L.ln2_g, L.ln2_b};
		fc.out_T = h->hbuf; fc.x = h->x; fc.ldx = d;
		TTK_TRY(decode_launch(ctx, fc, B, s));
		DecodeLaunch proj2 = {DR_PROJ2, &L.proj2, d, 4 * d, h->hbuf};
		proj2.out_f32 = h->x; proj2.out_T = xf;
		TTK_TRY(decode_launch(ctx, proj2, B, s));
	}
	// ln_f + final_norm ONCE (4 workgroups), the mel head as a plain 513-tile GEMV over the normalised rows in fragment order: with the norms inside the
	// GEMV every one of the 513 workgroups normalised all 16 rows, two passes each -- 17 us for 16.8 MB of weights
	if (h->ring_base && !hidden_out) launch_layernorm(dt, h->x, d, B, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b, h->attn_out, d, 0, s, 1, nullptr, h->ring_idx, h->ring_stride, h->d_ring);
	else launch_layernorm(dt, h->x, d, B, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b, h->attn_out, d, 0, s, 1, hidden_out);
	DecodeLaunch head = {DR_HEAD, &h->head, c.number_mel_codes, d, h->attn_out};
	head.out_f32 = logits_out; head.bump = true; head.d_pos = h->d_pos;      // the last launch of the step advances the cache length
	return decode_launch(ctx, head, B, s);
}

extern "C" {

int ttk_ar_create(ttk_ar** out, const ttk_ar_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_ar_create: null argument");
	TTK_REQUIRE(cfg->model_dim % 64 == 0 && cfg->heads * 64 == cfg->model_dim, TTK_E_ARG,
				"ttk_ar_create: head_dim must be 64 (model_dim %d, heads %d)", cfg->model_dim, cfg->heads);
	TTK_REQUIRE(cfg->model_dim <= 2048, TTK_E_ARG, "ttk_ar_create: model_dim %d > 2048 unsupported", cfg->model_dim);
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16 || cfg->dtype == TTK_F16 || cfg->dtype == TTK_FP8W, TTK_E_ARG, "ttk_ar_create: bad dtype %d", cfg->dtype);
	TTK_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= (cfg->dtype == TTK_F32 ? 32 : 64), TTK_E_ARG,
				"ttk_ar_create: max_batch %d out of range", cfg->max_batch);
	TTK_REQUIRE(cfg->max_ctx >= 8, TTK_E_ARG, "ttk_ar_create: max_ctx %d too small", cfg->max_ctx);
	{   // The launches that hold every candidate's normalised row in LDS must fit a compute unit for every batch this handle accepts: the prefill's head
		// (two norms inside the launch, all B rows) and the step launches of TTK_AR_LNFOLD=0 (at most 32 rows: decode_impl).  Checked here, not at the first prefill.
		const int kdt = kernel_dtype(cfg->dtype), d = cfg->model_dim;
		for (int B = 1; B <= cfg->max_batch; ++B) {
			const int mt = decode_row_tiles(B);
			const size_t head = skinny_lds_bytes(kdt, mt, d, skinny_launch_waves(skinny_waves(DR_HEAD, true, kdt, d), true), SKF_PROLOGUE);
			TTK_REQUIRE(head <= CU_LDS_BYTES, TTK_E_ARG, "ttk_ar_create: model_dim %d with max_batch %d: the prefill's head over %d rows needs %zu bytes of LDS, a compute unit has %zu", d,
						cfg->max_batch, B, head, CU_LDS_BYTES);
			const size_t step = skinny_lds_bytes(kdt, mt, d, skinny_launch_waves(skinny_waves(DR_QKV, true, kdt, d), true), SKF_PROLOGUE);
			TTK_REQUIRE(B > 32 || step <= CU_LDS_BYTES, TTK_E_ARG, "ttk_ar_create: model_dim %d with max_batch %d: the TTK_AR_LNFOLD=0 step over %d rows needs %zu bytes of LDS, a compute unit has %zu", d,
						cfg->max_batch, B, step, CU_LDS_BYTES);
		}
	}
	std::unique_ptr<ttk_ar> h(new ttk_ar());
	h->cfg = *cfg;
	h->wdt = cfg->dtype;
	h->dt = kernel_dtype(cfg->dtype);
	h->es = dtype_size(h->dt);
	WeightMap wm(w, n_w);
	const int d = cfg->model_dim;
	h->L.resize(cfg->layers);
	for (int l = 0; l < cfg->layers; ++l) {
		const std::string p = "gpt.h." + std::to_string(l) + ".";
		ARLayer& L = h->L[l];
		TTK_TRY(upload_f32(h->arena, wm, p + "ln_1.weight", d, &L.ln1_g));
		TTK_TRY(upload_f32(h->arena, wm, p + "ln_1.bias", d, &L.ln1_b));
		TTK_TRY(upload_f32(h->arena, wm, p + "ln_2.weight", d, &L.ln2_g));
		TTK_TRY(upload_f32(h->arena, wm, p + "ln_2.bias", d, &L.ln2_b));
		TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "attn.c_attn.weight", p + "attn.c_attn.bias", PK_KN, 3 * d, d, true, &L.attn));
		TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "attn.c_proj.weight", p + "attn.c_proj.bias", PK_KN, d, d, true, &L.proj));
		TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", PK_KN, 4 * d, d, true, &L.fc));
		TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "mlp.c_proj.weight", p + "mlp.c_proj.bias", PK_KN, d, 4 * d, true, &L.proj2));
		// (fp8 weights: the fold is taken of the rounded matrices and kept in bf16 -- TTK_FP8W stays "bf16 on the rounded weights")
		TTK_TRY(fold_layernorm(h->arena, wm, h->dt, p + "attn.c_attn.weight", p + "attn.c_attn.bias", p + "ln_1.weight", p + "ln_1.bias", &L.attn));
		TTK_TRY(fold_layernorm(h->arena, wm, h->dt, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", p + "ln_2.weight", p + "ln_2.bias", &L.fc));
	}
	TTK_TRY(upload_f32(h->arena, wm, "gpt.ln_f.weight", d, &h->lnf_g));
	TTK_TRY(upload_f32(h->arena, wm, "gpt.ln_f.bias", d, &h->lnf_b));
	TTK_TRY(upload_f32(h->arena, wm, "final_norm.weight", d, &h->fn_g));
	TTK_TRY(upload_f32(h->arena, wm, "final_norm.bias", d, &h->fn_b));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "mel_head.weight", "mel_head.bias", PK_NK, cfg->number_mel_codes, d, true, &h->head));
	if (wm.find("text_head.weight")) {      // the scoring weights (ttk_ar_score); a handle without them is what it was before that entry existed
		TTK_TRY(upload_mat(h->arena, wm, h->dt, "text_head.weight", "text_head.bias", PK_NK, cfg->number_text_tokens_p1, d, false, &h->text_head));
		h->scoring = true;
	}
	TTK_TRY(upload_f32(h->arena, wm, "text_embedding.weight", (int64_t)cfg->number_text_tokens_p1 * d, &h->text_emb));
	TTK_TRY(upload_f32(h->arena, wm, "mel_embedding.weight", (int64_t)cfg->number_mel_codes * d, &h->mel_emb));
	TTK_TRY(upload_f32(h->arena, wm, "mel_pos_embedding.emb.weight", (int64_t)cfg->max_mel_seq_len * d, &h->mel_pos));
	TTK_TRY(upload_f32(h->arena, wm, "text_pos_embedding.emb.weight", (int64_t)cfg->max_text_seq_len * d, &h->text_pos));
	h->kv_layer_stride = (size_t)cfg->max_batch * cfg->heads * cfg->max_ctx * 64;
	TTK_TRY(h->arena.alloc(&h->kc, h->kv_layer_stride * cfg->layers * h->es));
	TTK_TRY(h->arena.alloc(&h->vc, h->kv_layer_stride * cfg->layers * h->es));
	TTK_TRY(h->arena.alloc((void**)&h->d_pos, (size_t)(4 + 2 * cfg->max_batch) * sizeof(int)));
	h->d_rowinfo = (int2*)(h->d_pos + 4);
	h->d_health = h->d_pos + 2;      // (words 2, 3 of the block are otherwise unused; zeroed with it below)
	if (hipMemset(h->d_pos, 0, (size_t)(4 + 2 * cfg->max_batch) * sizeof(int)) != hipSuccess) return TTK_E_HIP;
	{   // the two position words move into the decode attention's position line when a slot is free (csrc/attn.hip); row_info and the health word stay in the block above
		int* words = nullptr;
		h->pos_slot = attn_pos_slot_acquire(&words);
		if (h->pos_slot >= 0) {
			h->d_pos = words;
			if (hipMemset(h->d_pos, 0, 2 * sizeof(int)) != hipSuccess) return TTK_E_HIP;
		}
	}
	TTK_TRY(h->arena.alloc((void**)&h->d_ring, sizeof(int64_t)));
	if (hipMemset(h->d_ring, 0, sizeof(int64_t)) != hipSuccess) return TTK_E_HIP;
	TTK_TRY(h->arena.alloc((void**)&h->x, (size_t)cfg->max_batch * d * sizeof(float)));
	TTK_TRY(h->arena.alloc((void**)&h->qbuf, (size_t)cfg->max_batch * d * sizeof(float)));
	// Fragment-order operands of the decode launches, [m_tile][k-step][lane]: the kernels are instantiated for 1, 2 or 4 sixteen-row tiles (csrc/gemv.hip:
	// gemv_mt) and request EVERY tile of their instantiation, so 33..48 rows read a fourth tile: it must exist (each buffer is its own allocation; a
	// read past its end is a fault whenever the driver has not mapped anything behind it) and hold zeros, like the padding rows inside a tile.
	const size_t frag_rows = (size_t)16 * decode_row_tiles(cfg->max_batch);      // the SAME function the launchers pick their instantiation with
	h->frag_rows = (int)frag_rows;
	for (int B = 1; B <= cfg->max_batch; ++B)      // every batch this handle accepts: the tiles its launches request exist
		if (16 * decode_row_tiles(B) > h->frag_rows) { set_error("ttk_ar_create: %d rows would request %d fragment rows, %d allocated", B, 16 * decode_row_tiles(B), h->frag_rows); return TTK_E_STATE; }
	TTK_TRY(h->arena.alloc(&h->attn_out, frag_rows * d * h->es));
	if (hipMemset(h->attn_out, 0, frag_rows * d * h->es) != hipSuccess) return TTK_E_HIP;
	TTK_TRY(h->arena.alloc(&h->hbuf, frag_rows * 4 * d * h->es));
	if (hipMemset(h->hbuf, 0, frag_rows * 4 * d * h->es) != hipSuccess) return TTK_E_HIP;
	TTK_TRY(h->arena.alloc(&h->x_frag, frag_rows * d * h->es));
	if (hipMemset(h->x_frag, 0, frag_rows * d * h->es) != hipSuccess) return TTK_E_HIP;
	{
		const char* ep = getenv("TTK_DEBUG_POISON");
		h->poison = ep && atoi(ep) != 0;
		const char* el = getenv("TTK_AR_LNFOLD");
		h->lnfold = el ? (atoi(el) != 0) : 1;
		const char* eg = getenv("TTK_AR_LEAN");
		h->lean = eg ? (atoi(eg) != 0) : 1;
	}
	hipError_t e = hipDeviceSynchronize();
	if (e != hipSuccess) { set_error("ttk_ar_create: %s", hipGetErrorString(e)); return TTK_E_HIP; }
	*out = h.release();
	return TTK_OK;
}

int ttk_ar_destroy(ttk_ar* h) {
	if (!h) return TTK_OK;
	(void)hipDeviceSynchronize();
	delete h;
	return TTK_OK;
}

static int prefill_impl(ttk_ar* h, const float* cond_latent, int Bc, const int64_t* text, int Tt, const int64_t* prompt, int prompt_rows, int n_in, int B, float* logits_out,
						void* stream, const char* who) {
	TTK_REQUIRE(h && cond_latent && text && logits_out, TTK_E_ARG, "%s: null argument", who);
	const ttk_ar_config& c = h->cfg;
	TTK_REQUIRE(B >= 1 && B <= c.max_batch, TTK_E_ARG, "%s: B=%d exceeds max_batch=%d", who, B, c.max_batch);
	TTK_REQUIRE(Bc == 1 || Bc == B, TTK_E_ARG, "%s: cond batch %d must be 1 or B=%d", who, Bc, B);
	TTK_REQUIRE(Tt >= 1 && Tt + 2 <= c.max_text_seq_len, TTK_E_ARG, "%s: %d text tokens exceed the position table (%d)", who, Tt, c.max_text_seq_len - 2);
	TTK_REQUIRE(n_in == 0 || (prompt && (prompt_rows == 1 || prompt_rows == B)), TTK_E_ARG, "%s: %d prompt tokens need 1 or B=%d prompt rows (got %d)", who, n_in, B, prompt_rows);
	TTK_REQUIRE(n_in >= 0 && n_in + 2 < c.max_mel_seq_len, TTK_E_ARG, "%s: %d prompt tokens exceed the mel position table (%d)", who, n_in, c.max_mel_seq_len);
	const int S = Tt + 4 + n_in, d = c.model_dim;
	TTK_REQUIRE(S + 1 <= c.max_ctx, TTK_E_ARG, "%s: prefix of %d rows does not fit max_ctx=%d", who, S, c.max_ctx);
	hipStream_t s = (hipStream_t)stream;
	// One conditioning latent and one text line for all B candidates (what inference_speech passes): the B prefixes are the same rows, so
	// the prefix is run ONCE and its cache rows live in candidate 0's slice only -- the decode attention reads rows [0, S) there for every
	// candidate (AttnDecodeParams.shared_rows) -- and the last row / the logits are replicated.  (A prompt shared by all candidates is part of that
	// prefix; with one prompt per candidate every candidate's rows are run and cached on their own.)
	const bool shared = Bc == 1 && B > 1 && (n_in == 0 || prompt_rows == 1);
	const int Bp = shared ? 1 : B;
	TTK_TRY(h->ws_x.reserve((size_t)Bp * S * d * sizeof(float)));
	float* x = (float*)h->ws_x.p;
	const int64_t total = (int64_t)Bp * S * (d / 4);
	hipLaunchKernelGGL(k_build_prefill_emb, dim3(grid_for(total)), dim3(256), 0, s, cond_latent, Bc, text, Tt, Bp, d,
					   h->text_emb, h->text_pos, h->mel_emb, h->mel_pos, c.start_text_token, c.stop_text_token, c.start_mel_token, x, prompt, prompt_rows, n_in);
	TTK_TRY(dense_forward(h, x, Bp, S, true, s));
	launch_copy_rows(x + (size_t)(S - 1) * d, shared ? 0 : (int64_t)S * d, h->x, d, B, d, s);      // source stride 0: one row to all candidates
	TTK_TRY(head_launch(h, B, logits_out, s));
	launch_set_int(h->d_pos, S, s);
	launch_set_int(h->d_pos + 1, shared ? S : 0, s);      // rows of the shared prefix (AttnDecodeParams.shared_rows): device-resident, like the cache length
	TTK_TRY(poison_scratch(h, s));
	// k = mel tokens behind start_mel that are cached already: the decode step's capacity and position checks count from it (the position itself is taken
	// from the cache length on the device: cached rows - P, the reference's attention_mask.shape[1] - mel_len)
	h->B = B; h->P = h->Pmax = Tt + 3; h->k = n_in; h->ready = 1; h->lines_mode = 0;
	h->shared_rows = shared ? S : 0;
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_ar_prefill(ttk_ar* h, const float* cond_latent, int Bc, const int64_t* text, int Tt, int B, float* logits_out, void* stream) {
	return prefill_impl(h, cond_latent, Bc, text, Tt, nullptr, 0, 0, B, logits_out, stream, "ttk_ar_prefill");
}

int ttk_ar_prefill_prompted(ttk_ar* h, const float* cond_latent, int Bc, const int64_t* text, int Tt, const int64_t* prompt, int prompt_rows, int n_prompt, int B,
							float* logits_out, void* stream) {
	TTK_REQUIRE(n_prompt >= 1 && prompt, TTK_E_ARG, "ttk_ar_prefill_prompted: needs at least one prompt token");
	return prefill_impl(h, cond_latent, Bc, text, Tt, prompt, prompt_rows, n_prompt, B, logits_out, stream, "ttk_ar_prefill_prompted");
}

// Several text lines as ONE decode batch (no reference counterpart: TTS.inference walks its lines one by one, inference.py:244-246, each with
// the weights streamed again for 16 rows): line g occupies candidates [g * rows_per_line, (g + 1) * rows_per_line), its prefix is run once into
// the slice of its first candidate, and the decode step gives every candidate its own cache length -- d_pos + row_off[b] -- so each row's keys
// are dealt to the waves exactly as in a batch of its own and its logits are bit for bit those of ttk_ar_prefill / ttk_ar_decode on that line alone.
int ttk_ar_prefill_lines(ttk_ar* h, const float* cond_latents, const int64_t* text, const int* text_len, int n_lines, int rows_per_line,
						 float* logits_out, void* stream) {
	TTK_REQUIRE(h && cond_latents && text && text_len && logits_out, TTK_E_ARG, "ttk_ar_prefill_lines: null argument");
	const ttk_ar_config& c = h->cfg;
	const int B = n_lines * rows_per_line, d = c.model_dim;
	TTK_REQUIRE(n_lines >= 1 && rows_per_line >= 1 && B <= c.max_batch, TTK_E_ARG, "ttk_ar_prefill_lines: %d lines x %d candidates exceed max_batch=%d", n_lines, rows_per_line, c.max_batch);
	int Smax = 0;
	for (int g = 0; g < n_lines; ++g) {
		const int Tt = text_len[g];
		TTK_REQUIRE(Tt >= 1 && Tt + 2 <= c.max_text_seq_len, TTK_E_ARG, "ttk_ar_prefill_lines: line %d: %d text tokens exceed the position table (%d)", g, Tt, c.max_text_seq_len - 2);
		TTK_REQUIRE(Tt + 5 <= c.max_ctx, TTK_E_ARG, "ttk_ar_prefill_lines: line %d: prefix of %d rows does not fit max_ctx=%d", g, Tt + 4, c.max_ctx);
		Smax = Tt + 4 > Smax ? Tt + 4 : Smax;
	}
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(h->ws_x.reserve((size_t)Smax * d * sizeof(float)));
	float* x = (float*)h->ws_x.p;
	int64_t toff = 0;
	for (int g = 0; g < n_lines; ++g) {
		// prefixes right-aligned at Smax: the cache length is then ONE number for all candidates (the c_attn epilogue appends every row at
		// *d_pos, as for one line) and only the attention needs to know where a candidate's rows begin
		const int Tt = text_len[g], S = Tt + 4, r0 = g * rows_per_line, start = Smax - S;
		const int64_t total = (int64_t)S * (d / 4);
		hipLaunchKernelGGL(k_build_prefill_emb, dim3(grid_for(total)), dim3(256), 0, s, cond_latents + (size_t)g * d, 1, text + toff, Tt, 1, d,
						   h->text_emb, h->text_pos, h->mel_emb, h->mel_pos, c.start_text_token, c.stop_text_token, c.start_mel_token, x);
		TTK_TRY(dense_forward(h, x, 1, S, true, s, r0, start));
		launch_copy_rows(x + (size_t)(S - 1) * d, 0, h->x + (size_t)r0 * d, d, rows_per_line, d, s);      // the line's last prefix row to all its candidates
		launch_fill_int2((int*)(h->d_rowinfo + r0), start, r0, rows_per_line, s);
		toff += Tt;
	}
	TTK_TRY(head_launch(h, B, logits_out, s));
	launch_set_int(h->d_pos, Smax, s);
	launch_set_int(h->d_pos + 1, Smax, s);
	TTK_TRY(poison_scratch(h, s));
	h->B = B; h->P = h->Pmax = Smax - 1; h->k = 0; h->ready = 1; h->lines_mode = 1; h->rows_per_line = rows_per_line;
	h->shared_rows = Smax;
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

static int decode_impl(ttk_ar* h, const int64_t* tok, float* logits_out, float* hidden_out, void* stream, const char* who) {
	TTK_REQUIRE(h && logits_out, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(h->ready, TTK_E_STATE, "%s: call ttk_ar_prefill first", who);
	const ttk_ar_config& c = h->cfg;
	const int B = h->B, d = c.model_dim;
	TTK_REQUIRE(h->Pmax + 1 + h->k + 1 <= c.max_ctx, TTK_E_STATE, "%s: KV cache full (max_ctx=%d)", who, c.max_ctx);
	TTK_REQUIRE(B <= c.max_batch && 16 * decode_row_tiles(B) <= h->frag_rows, TTK_E_STATE, "%s: %d rows request %d fragment rows, the handle holds %d (max_batch=%d)", who, B,
				16 * decode_row_tiles(B), h->frag_rows, c.max_batch);
	TTK_REQUIRE(h->lnfold || B <= 32, TTK_E_STATE, "%s: the LayerNorm-prologue decode kernels (TTK_AR_LNFOLD=0) hold at most 32 candidates' rows in LDS; B=%d", who, B);
	TTK_REQUIRE(h->k + 2 < c.max_mel_seq_len, TTK_E_STATE, "%s: mel position table exhausted (%d rows)", who, c.max_mel_seq_len);
	hipStream_t s = (hipStream_t)stream;
	// x[b] = mel_embedding[tok] + mel_pos[k + 1]; *d_pos = P + k rows are cached  =>  offset 1 - P   (unified_voice.py:213-214)
	// (tok == null: ttk_ar_sample_next has written the rows already)
	if (tok) launch_decode_embed(h->mel_emb, tok, h->mel_pos, h->d_pos, 1 - h->P, c.max_mel_seq_len, h->x, B, d, s, h->lnfold ? h->x_frag : nullptr, elem_kind(h->dt));
	TTK_TRY(decode_rows(h, logits_out, hidden_out, s));
	h->k += 1;
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_ar_decode(ttk_ar* h, const int64_t* tok, float* logits_out, float* hidden_out, void* stream) {
	TTK_REQUIRE(tok, TTK_E_ARG, "ttk_ar_decode: null argument");
	return decode_impl(h, tok, logits_out, hidden_out, stream, "ttk_ar_decode");
}

int ttk_ar_decode_next(ttk_ar* h, float* logits_out, float* hidden_out, void* stream) {
	return decode_impl(h, nullptr, logits_out, hidden_out, stream, "ttk_ar_decode_next");
}

// The token step behind a decode step, on the handle's embedding tables and input row: the sampling launch, its greedy form, or with `x` the one over the
// reference's samplers.
static int sample_next(ttk_ar* h, const ttk_sample_args* a, const ttk_sample_ext* x, bool greedy, void* stream, const char* who) {
	TTK_REQUIRE(h && a, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(h->ready, TTK_E_STATE, "%s: call ttk_ar_prefill first", who);
	TTK_REQUIRE(a->B == h->B && a->V == h->cfg.number_mel_codes, TTK_E_ARG, "%s: shape (B %d, V %d) is not the prefilled one (B %d, V %d)", who, a->B, a->V, h->B,
				h->cfg.number_mel_codes);
	const int d = h->cfg.model_dim, pos_rows = h->cfg.max_mel_seq_len, kind = elem_kind(h->dt);
	void* x_frag = h->lnfold ? h->x_frag : nullptr;
	if (x) return launch_sample_step_ext(a, x, h->mel_emb, h->mel_pos, h->x, d, pos_rows, x_frag, kind, (hipStream_t)stream, who);
	return (greedy ? launch_greedy_step : launch_sample_step)(a, h->mel_emb, h->mel_pos, h->x, d, pos_rows, x_frag, kind, (hipStream_t)stream, who);
}

int ttk_ar_sample_next(ttk_ar* h, const ttk_sample_args* a, void* stream) { return sample_next(h, a, nullptr, false, stream, "ttk_ar_sample_next"); }

int ttk_ar_greedy_next(ttk_ar* h, const ttk_sample_args* a, void* stream) { return sample_next(h, a, nullptr, true, stream, "ttk_ar_greedy_next"); }

int ttk_ar_sample_next_ext(ttk_ar* h, const ttk_sample_args* a, const ttk_sample_ext* x, void* stream) {
	TTK_REQUIRE(x, TTK_E_ARG, "ttk_ar_sample_next_ext: null argument");
	return sample_next(h, a, x, false, stream, "ttk_ar_sample_next_ext");
}

int ttk_ar_reorder_cache(ttk_ar* h, const int64_t* beam_idx, void* stream) {
	TTK_REQUIRE(h && beam_idx, TTK_E_ARG, "ttk_ar_reorder_cache: null argument");
	TTK_REQUIRE(h->ready, TTK_E_STATE, "ttk_ar_reorder_cache: call ttk_ar_prefill first");
	TTK_REQUIRE(!h->lines_mode, TTK_E_STATE, "ttk_ar_reorder_cache: the candidates of a line batch (ttk_ar_prefill_lines) keep their own histories");
	// rows [d_pos[1], d_pos[0]) of every slice; the shared prefix lives in slice 0 alone and is what every beam reads, whatever the order
	return launch_kv_reorder(h->kc, h->vc, h->cfg.layers, h->cfg.max_batch, h->cfg.heads, h->cfg.max_ctx, h->es, h->d_pos, beam_idx, h->B, h->B, (hipStream_t)stream,
							 "ttk_ar_reorder_cache");
}

int ttk_ar_reorder_cache_lines(ttk_ar* h, const int64_t* beam_idx, int rows_per_line, void* stream) {
	TTK_REQUIRE(h && beam_idx, TTK_E_ARG, "ttk_ar_reorder_cache_lines: null argument");
	TTK_REQUIRE(h->ready && h->lines_mode && h->rows_per_line == rows_per_line, TTK_E_STATE,
				"ttk_ar_reorder_cache_lines: call ttk_ar_prefill_lines with rows_per_line=%d first", rows_per_line);
	// rows [d_pos[1], d_pos[0]) of all B slices: d_pos[1] is Smax here -- every line's right-aligned prefix lies below it, in the slice of the line's first
	// candidate, and stays; above it every candidate's rows are its own, and a line's beams exchange them among themselves only
	return launch_kv_reorder(h->kc, h->vc, h->cfg.layers, h->cfg.max_batch, h->cfg.heads, h->cfg.max_ctx, h->es, h->d_pos, beam_idx, h->B, rows_per_line,
							 (hipStream_t)stream, "ttk_ar_reorder_cache_lines");
}

int ttk_ar_set_noise(ttk_ar* h, const int64_t* rng_args, const int64_t* draws, float* q) {
	TTK_REQUIRE(h, TTK_E_ARG, "ttk_ar_set_noise: null handle");
	TTK_REQUIRE((rng_args && draws && q) || (!rng_args && !draws && !q), TTK_E_ARG, "ttk_ar_set_noise: pass all three pointers or none");
	h->rng_args = rng_args; h->rng_draws = draws; h->rng_q = q;
	return TTK_OK;
}

int ttk_ar_set_hidden_ring(ttk_ar* h, float* base, const int64_t* index, int64_t stride, void* stream) {
	TTK_REQUIRE(h, TTK_E_ARG, "ttk_ar_set_hidden_ring: null handle");
	TTK_REQUIRE(!base || (index && stride >= 0), TTK_E_ARG, "ttk_ar_set_hidden_ring: a ring needs its device index and a stride");
	h->ring_base = base; h->ring_idx = base ? index : nullptr; h->ring_stride = base ? stride : 0;
	if (base) {      // the launches read the base from device memory (a captured step is replayed by later generations with their own buffers): stream-ordered upload
		const int64_t v = (int64_t)(uintptr_t)base;
		TTK_HIP(hipMemcpyAsync(h->d_ring, &v, sizeof(v), hipMemcpyHostToDevice, (hipStream_t)stream));
	}
	return TTK_OK;
}

int ttk_ar_decode_geometry(int dtype, int max_batch, int rows, int32_t out[4]) {
	TTK_REQUIRE(out, TTK_E_ARG, "ttk_ar_decode_geometry: null argument");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16 || dtype == TTK_FP8W || dtype == TTK_FP8, TTK_E_ARG, "ttk_ar_decode_geometry: bad dtype %d", dtype);
	const int cap = dtype == TTK_F32 ? 32 : 64;
	TTK_REQUIRE(max_batch >= 1 && max_batch <= cap, TTK_E_ARG, "ttk_ar_decode_geometry: max_batch %d out of range (1..%d)", max_batch, cap);
	TTK_REQUIRE(rows >= 1 && rows <= max_batch, TTK_E_ARG, "ttk_ar_decode_geometry: rows %d outside 1..max_batch=%d", rows, max_batch);
	out[0] = 16 * decode_row_tiles(max_batch);      // rows ttk_ar_create allocates (and zeroes) per fragment-order operand
	out[1] = decode_row_tiles(rows);                // sixteen-row tiles of the instantiation a launch over `rows` rows runs
	out[2] = 16 * out[1];                           // rows that launch requests
	out[3] = max_batch;                             // candidate slices of the KV cache
	return TTK_OK;
}

int ttk_ar_health(ttk_ar* h, int* flags_out, void* stream) {
	TTK_REQUIRE(h && flags_out, TTK_E_ARG, "ttk_ar_health: null argument");
	hipStream_t s = (hipStream_t)stream;
	TTK_HIP(hipMemcpyAsync(flags_out, h->d_health, sizeof(int), hipMemcpyDeviceToHost, s));
	TTK_HIP(hipStreamSynchronize(s));
	if (*flags_out) launch_set_int(h->d_health, 0, s);
	return TTK_OK;
}

int ttk_ar_last_hidden(ttk_ar* h, float* hidden_out, void* stream) {
	TTK_REQUIRE(h && hidden_out, TTK_E_ARG, "ttk_ar_last_hidden: null argument");
	TTK_REQUIRE(h->ready, TTK_E_STATE, "ttk_ar_last_hidden: call ttk_ar_prefill first");
	const int d = h->cfg.model_dim;
	// h->x holds the residual stream of the newest row after the last block; enc = final_norm(ln_f(x))   (unified_voice.py:106, HF GPT2Model ln_f)
	launch_layernorm(h->dt, h->x, d, h->B, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b, hidden_out, d, 1, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_ar_latents(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, float* latents_out, void* stream) {
	TTK_REQUIRE(h && cond && text && codes && latents_out, TTK_E_ARG, "ttk_ar_latents: null argument");
	const ttk_ar_config& c = h->cfg;
	TTK_REQUIRE(B >= 1 && Tt >= 1 && M >= 1, TTK_E_ARG, "ttk_ar_latents: empty input (B=%d Tt=%d M=%d)", B, Tt, M);
	TTK_REQUIRE(Tt + 2 <= c.max_text_seq_len, TTK_E_ARG, "ttk_ar_latents: %d text tokens exceed the position table", Tt);
	TTK_REQUIRE(M + 2 <= c.max_mel_seq_len, TTK_E_ARG, "ttk_ar_latents: %d mel codes exceed the position table (%d)", M, c.max_mel_seq_len - 2);
	const int S = Tt + M + 5, d = c.model_dim;
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(h->ws_x.reserve((size_t)B * S * d * sizeof(float)));
	float* x = (float*)h->ws_x.p;
	const int64_t total = (int64_t)B * S * (d / 4);
	hipLaunchKernelGGL(k_build_latent_emb, dim3(grid_for(total)), dim3(256), 0, s, cond, text, Tt, codes, M, B, d,
					   h->text_emb, h->text_pos, h->mel_emb, h->mel_pos, c.start_text_token, c.stop_text_token, c.start_mel_token, c.stop_mel_token, x);
	TTK_TRY(dense_forward(h, x, B, S, false, s));
	// enc = final_norm(ln_f(h)); mel rows start at 1 + (Tt + 2); keep the first M of the M + 2   (unified_voice.py:518-522,595)
	for (int b = 0; b < B; ++b)
		launch_layernorm(h->dt, x + ((size_t)b * S + Tt + 3) * d, d, M, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b,
						 latents_out + (size_t)b * M * d, d, 1, s);
	TTK_TRY(poison_scratch(h, s));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_ar_score(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, float* loss_out, float* nll_text_out, float* nll_mel_out,
				 float* text_logits_out, float* mel_logits_out, void* stream) {
	TTK_REQUIRE(h && cond && text && codes, TTK_E_ARG, "ttk_ar_score: null argument");
	TTK_REQUIRE(h->scoring, TTK_E_STATE, "ttk_ar_score: this handle was created without text_head.weight / text_head.bias: pass the full state dict to ttk_ar_create");
	const ttk_ar_config& c = h->cfg;
	TTK_REQUIRE(B >= 1 && Tt >= 1 && M >= 1, TTK_E_ARG, "ttk_ar_score: empty input (B=%d Tt=%d M=%d)", B, Tt, M);
	TTK_REQUIRE(Tt + 2 <= c.max_text_seq_len, TTK_E_ARG, "ttk_ar_score: %d text tokens exceed the position table", Tt);
	TTK_REQUIRE(M + 2 <= c.max_mel_seq_len, TTK_E_ARG, "ttk_ar_score: %d mel codes exceed the position table (%d)", M, c.max_mel_seq_len - 2);
	const int S = Tt + M + 5, d = c.model_dim, Rt = Tt + 2, Rm = M + 2;
	const int Ct = c.number_text_tokens_p1, Cm = c.number_mel_codes, ldt = round_up(Ct, 4), ldm = round_up(Cm, 4);      // rows of the logits start on 16 bytes
	const int64_t rows_t = (int64_t)B * Rt, rows_m = (int64_t)B * Rm;
	TTK_REQUIRE((int64_t)B * S * 4 * d * (int64_t)h->es < (1ll << 31) && rows_m * ldm * 4 < (1ll << 31) && rows_t * ldt * 4 < (1ll << 31), TTK_E_ARG,
				"ttk_ar_score: B=%d x (Tt=%d + M=%d) makes a GEMM operand of 2 GiB or more (32-bit buffer offsets): score the batch in parts", B, Tt, M);
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(h->ws_x.reserve((size_t)B * S * d * sizeof(float)));
	// [logits text | logits mel | nll text | nll mel | targets text | targets mel]: every part starts on 16 bytes
	const size_t o_lm = (size_t)rows_t * ldt * 4, o_nt = o_lm + (size_t)rows_m * ldm * 4, o_nm = o_nt + (size_t)round_up((int)rows_t, 4) * 4;
	const size_t o_tt = o_nm + (size_t)round_up((int)rows_m, 4) * 4, o_tm = o_tt + (size_t)round_up((int)rows_t, 2) * 8;
	TTK_TRY(h->ws_score.reserve(o_tm + (size_t)rows_m * 8));
	char* ws = (char*)h->ws_score.p;
	float *lg_t = (float*)ws, *lg_m = (float*)(ws + o_lm);
	float *nll_t = nll_text_out ? nll_text_out : (float*)(ws + o_nt), *nll_m = nll_mel_out ? nll_mel_out : (float*)(ws + o_nm);
	int64_t *tg_t = (int64_t*)(ws + o_tt), *tg_m = (int64_t*)(ws + o_tm);
	float* x = (float*)h->ws_x.p;
	const int64_t total = (int64_t)B * S * (d / 4);
	hipLaunchKernelGGL(k_build_latent_emb, dim3(grid_for(total)), dim3(256), 0, s, cond, text, Tt, codes, M, B, d,
					   h->text_emb, h->text_pos, h->mel_emb, h->mel_pos, c.start_text_token, c.stop_text_token, c.start_mel_token, c.stop_mel_token, x);
	hipLaunchKernelGGL(k_build_score_targets, dim3(grid_for(rows_t + rows_m)), dim3(256), 0, s, text, Tt, c.stop_text_token, codes, M, c.stop_mel_token, B, tg_t, tg_m);
	TTK_TRY(dense_forward(h, x, B, S, false, s));
	// enc = final_norm(ln_f(h))[:, 1:]; the text head reads its first Tt + 2 rows, the mel head its last M + 2   (unified_voice.py:518-530).  ws_a holds
	// B * S rows (dense_forward): the B * (S - 1) normalised rows of both heads fit, T-typed, text rows first
	char* a_t = (char*)h->ws_a.p;
	char* a_m = a_t + (size_t)rows_t * d * h->es;
	for (int b = 0; b < B; ++b) {
		launch_layernorm(h->dt, x + ((size_t)b * S + 1) * d, d, Rt, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b, a_t + (size_t)b * Rt * d * h->es, d, 0, s);
		launch_layernorm(h->dt, x + ((size_t)b * S + Tt + 3) * d, d, Rm, d, h->lnf_g, h->lnf_b, h->fn_g, h->fn_b, a_m + (size_t)b * Rm * d * h->es, d, 0, s);
	}
	struct Head { const Mat* W; const void* a; int rows, C, ld, T; float* lg; const int64_t* tg; float* nll; float* out_t; };
	const Head heads[2] = {{&h->text_head, a_t, (int)rows_t, Ct, ldt, Rt, lg_t, tg_t, nll_t, text_logits_out}, {&h->head, a_m, (int)rows_m, Cm, ldm, Rm, lg_m, tg_m, nll_m, mel_logits_out}};
	for (int i = 0; i < 2; ++i) {
		const Head& q = heads[i];
		GemmParams g = dense_gemm(q.a, d, *q.W, q.rows, q.lg, 1);
		g.ldc = q.ld;
		launch_gemm(h->dt, g, s);
		launch_xent_rows(q.lg, q.ld, q.rows, q.C, q.tg, q.nll, loss_out ? loss_out + i : nullptr, q.out_t, q.T, s);
	}
	TTK_TRY(poison_scratch(h, s));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// the dense pass of ttk_ar_latents with a tap: `sel` = {layer, head, output slot} triples, grouped by layer here; a layer's maps go to out + out_index[layer] * out_stride
static int tapped_pass(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, std::vector<std::array<int, 3>>& sel, bool with_slots,
					   AttnTap& tap, float* out, const std::vector<int>& out_index, int64_t out_stride, void* stream, const char* who) {
	const ttk_ar_config& c = h->cfg;
	TTK_REQUIRE(B >= 1 && B <= 65535 && Tt >= 1 && M >= 1, TTK_E_ARG, "%s: empty input (B=%d Tt=%d M=%d)", who, B, Tt, M);
	TTK_REQUIRE(Tt + 2 <= c.max_text_seq_len, TTK_E_ARG, "%s: %d text tokens exceed the position table", who, Tt);
	TTK_REQUIRE(M + 2 <= c.max_mel_seq_len, TTK_E_ARG, "%s: %d mel codes exceed the position table (%d)", who, M, c.max_mel_seq_len - 2);
	const int S = Tt + M + 5, d = c.model_dim;
	TTK_REQUIRE((int64_t)B * S * 4 * d * (int64_t)h->es < (1ll << 31), TTK_E_ARG, "%s: B=%d x (Tt=%d + M=%d) makes a GEMM operand of 2 GiB or more (32-bit buffer offsets): run the batch in parts",
				who, B, Tt, M);
	std::stable_sort(sel.begin(), sel.end(), [](const std::array<int, 3>& a, const std::array<int, 3>& b) { return a[0] < b[0]; });
	const int n = (int)sel.size();
	tap.layer.assign(c.layers, AttnTap::Layer());
	h->tap_host.assign(2 * (size_t)n, 0);
	for (int i = 0; i < n; ++i) {
		AttnTap::Layer& L = tap.layer[sel[i][0]];
		if (L.count++ == 0) { L.first = i; L.out = out + out_index[sel[i][0]] * out_stride; }
		h->tap_host[i] = sel[i][1]; h->tap_host[n + i] = sel[i][2];
		tap.last = sel[i][0];
	}
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(h->ws_tap.reserve(2 * (size_t)n * sizeof(int)));
	TTK_HIP(hipMemcpyAsync(h->ws_tap.p, h->tap_host.data(), 2 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
	tap.heads = (const int*)h->ws_tap.p;
	tap.slots = with_slots ? tap.heads + n : nullptr;
	TTK_TRY(h->ws_x.reserve((size_t)B * S * d * sizeof(float)));
	float* x = (float*)h->ws_x.p;
	const int64_t total = (int64_t)B * S * (d / 4);
	hipLaunchKernelGGL(k_build_latent_emb, dim3(grid_for(total)), dim3(256), 0, s, cond, text, Tt, codes, M, B, d,
					   h->text_emb, h->text_pos, h->mel_emb, h->mel_pos, c.start_text_token, c.stop_text_token, c.start_mel_token, c.stop_mel_token, x);
	TTK_TRY(dense_forward(h, x, B, S, false, s, 0, 0, &tap));
	TTK_TRY(poison_scratch(h, s));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_ar_attentions(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, const int* layers, int n_layers, float* out, void* stream) {
	TTK_REQUIRE(h && cond && text && codes && layers && out, TTK_E_ARG, "ttk_ar_attentions: null argument");
	const int nl = h->cfg.layers, H = h->cfg.heads;
	TTK_REQUIRE(n_layers >= 1 && n_layers <= nl, TTK_E_ARG, "ttk_ar_attentions: select 1..%d layers, got %d", nl, n_layers);
	std::vector<int> index(nl, -1);
	for (int j = 0; j < n_layers; ++j) {
		TTK_REQUIRE(layers[j] >= 0 && layers[j] < nl, TTK_E_ARG, "ttk_ar_attentions: layer %d is outside [0, %d)", layers[j], nl);
		TTK_REQUIRE(index[layers[j]] < 0, TTK_E_ARG, "ttk_ar_attentions: layer %d is selected twice", layers[j]);
		index[layers[j]] = j;
	}
	const int64_t S = (int64_t)Tt + M + 5, per_layer = (int64_t)B * H * S * S;
	TTK_REQUIRE(Tt >= 1 && M >= 1 && B >= 1, TTK_E_ARG, "ttk_ar_attentions: empty input (B=%d Tt=%d M=%d)", B, Tt, M);
	TTK_REQUIRE(per_layer * n_layers * 4 < (1ll << 31), TTK_E_ARG,
				"ttk_ar_attentions: %d layers x B=%d x %d heads x %lld x %lld f32 is an output of 2 GiB or more: select fewer layers", n_layers, B, H, (long long)S, (long long)S);
	std::vector<std::array<int, 3>> sel;
	for (int j = 0; j < n_layers; ++j)
		for (int hd = 0; hd < H; ++hd) sel.push_back({layers[j], hd, hd});
	AttnTap tap;
	tap.n_out = H; tap.r0 = 0; tap.R = (int)S; tap.c0 = 0; tap.C = (int)S;
	return tapped_pass(h, cond, text, Tt, codes, M, B, sel, false, tap, out, index, per_layer, stream, "ttk_ar_attentions");
}

int ttk_ar_text_attention(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, const int* layer_head, int n, float* out, void* stream) {
	TTK_REQUIRE(h && cond && text && codes && layer_head && out, TTK_E_ARG, "ttk_ar_text_attention: null argument");
	const int nl = h->cfg.layers, H = h->cfg.heads;
	TTK_REQUIRE(n >= 1 && n <= 65535, TTK_E_ARG, "ttk_ar_text_attention: select 1..65535 (layer, head) pairs, got %d", n);
	std::vector<std::array<int, 3>> sel;
	for (int i = 0; i < n; ++i) {
		const int l = layer_head[2 * i], hd = layer_head[2 * i + 1];
		TTK_REQUIRE(l >= 0 && l < nl && hd >= 0 && hd < H, TTK_E_ARG, "ttk_ar_text_attention: pair %d = (layer %d, head %d) is outside %d layers x %d heads", i, l, hd, nl, H);
		sel.push_back({l, hd, i});
	}
	TTK_REQUIRE(Tt >= 1 && M >= 1 && B >= 1, TTK_E_ARG, "ttk_ar_text_attention: empty input (B=%d Tt=%d M=%d)", B, Tt, M);
	TTK_REQUIRE((int64_t)B * n * M * Tt * 4 < (1ll << 31), TTK_E_ARG,
				"ttk_ar_text_attention: B=%d x %d heads x M=%d x Tt=%d f32 is an output of 2 GiB or more: select fewer heads", B, n, M, Tt);
	AttnTap tap;
	tap.n_out = n; tap.r0 = Tt + 3; tap.R = M; tap.c0 = 2; tap.C = Tt;
	return tapped_pass(h, cond, text, Tt, codes, M, B, sel, true, tap, out, std::vector<int>(nl, 0), 0, stream, "ttk_ar_text_attention");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ run-time LoRA adapters
// The reference attaches its adapter as a weight parametrization and evaluates W + (B A) s on every forward (models/lora.py:120-123; inference.py:99-104,
// 204-216).  Here the packed operands of a matrix are rebuilt on the device from a resident f32 master: the update kernel (lora.hip) into the scratch, then
// pack_mat / pack_fold -- the launches ttk_ar_create ran -- into the buffers the handle already has.  Nothing a captured token step points at moves.
namespace {

constexpr int LORA_MAX_RANK = 256;
const char* const LORA_MODULES[4] = {"attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"};

std::string lora_module(int idx) { return "gpt.h." + std::to_string(idx / 4) + "." + LORA_MODULES[idx % 4]; }
Mat* lora_mat(ttk_ar* h, int idx) {
	ARLayer& L = h->L[idx / 4];
	Mat* m[4] = {&L.attn, &L.proj, &L.fc, &L.proj2};
	return m[idx % 4];
}
struct LoraPair { const ttk_weight_view *A = nullptr, *B = nullptr; };

}  // namespace

extern "C" {

int ttk_ar_lora_init(ttk_ar* h, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(h && w && n_w > 0, TTK_E_ARG, "ttk_ar_lora_init: null argument");
	TTK_REQUIRE(h->wdt != DT_FP8W, TTK_E_ARG, "ttk_ar_lora_init: run-time adapters are not implemented for dtype TTK_FP8W: the fp8 scale of a matrix follows the adapted "
				"matrix's absmax, whose reduction synchronises; fold the adapter at load time instead (f32, bf16 and f16 handles take adapters)");
	TTK_REQUIRE(!h->lora_ready, TTK_E_STATE, "ttk_ar_lora_init: this handle holds its adapter masters already");
	WeightMap wm(w, n_w);
	const int d = h->cfg.model_dim, nm = 4 * h->cfg.layers;
	for (int i = 0; i < nm; ++i) {      // everything is checked before the first allocation
		const std::string name = lora_module(i) + ".weight";
		const ttk_weight_view* v = wm.find(name);
		const Mat* m = lora_mat(h, i);
		TTK_REQUIRE(v != nullptr, TTK_E_WEIGHT, "ttk_ar_lora_init: missing weight '%s'", name.c_str());
		TTK_REQUIRE(numel(v) == (int64_t)m->N * m->K, TTK_E_WEIGHT, "ttk_ar_lora_init: weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)numel(v),
					(long long)m->N * m->K);
	}
	std::vector<float*> master(nm, nullptr);
	for (int i = 0; i < nm; ++i) {
		const Mat* m = lora_mat(h, i);
		const size_t bytes = (size_t)m->N * m->K * sizeof(float);
		TTK_TRY(h->arena.alloc((void**)&master[i], bytes));
		TTK_HIP(hipMemcpy(master[i], wm.find(lora_module(i) + ".weight")->data, bytes, hipMemcpyDefault));
	}
	TTK_TRY(h->arena.alloc((void**)&h->lora_scratch, (size_t)4 * d * d * sizeof(float)));
	TTK_TRY(h->arena.alloc(&h->lora_wt, (size_t)round_up(4 * d, 128) * d * h->es));      // the largest Npad x Kpad: c_fc
	h->lora_master.swap(master);
	h->lora_adapted.assign(nm, 0);
	h->lora_ready = true;
	return TTK_OK;
}

int ttk_ar_lora_set(ttk_ar* h, const ttk_weight_view* adapters, int n, float scaling, void* stream) {
	TTK_REQUIRE(h && n >= 0 && (adapters || n == 0), TTK_E_ARG, "ttk_ar_lora_set: null argument");
	TTK_REQUIRE(h->lora_ready, TTK_E_ARG, "ttk_ar_lora_set: this handle keeps no adapter masters: call ttk_ar_lora_init after ttk_ar_create "
				"(UnifiedVoice(..., adapters=True)) before attaching or detaching adapters");
	TTK_REQUIRE(n == 0 || (scaling == scaling && scaling - scaling == 0.f), TTK_E_ARG, "ttk_ar_lora_set: scaling %g is not finite", (double)scaling);
	const int nm = 4 * h->cfg.layers;
	// all or nothing: every view is checked before the first launch
	std::map<std::string, int> index;
	for (int i = 0; i < nm; ++i) index[lora_module(i)] = i;
	std::vector<LoraPair> plan(nm);
	for (int i = 0; i < n; ++i) {
		const ttk_weight_view* v = &adapters[i];
		TTK_REQUIRE(v->name && v->data, TTK_E_ARG, "ttk_ar_lora_set: adapter tensor %d has no name or no data", i);
		const std::string name = v->name;
		const size_t cut = name.size() > 7 ? name.size() - 7 : 0;
		const std::string tail = name.substr(cut);
		TTK_REQUIRE(tail == ".lora_A" || tail == ".lora_B", TTK_E_WEIGHT, "ttk_ar_lora_set: '%s' is not named <module>.lora_A or <module>.lora_B", name.c_str());
		const auto it = index.find(name.substr(0, cut));
		TTK_REQUIRE(it != index.end(), TTK_E_WEIGHT, "ttk_ar_lora_set: '%s': run-time adapters attach to gpt.h.<layer>.{attn.c_attn, attn.c_proj, mlp.c_fc, mlp.c_proj} "
					"of the %d layers only (other modules: fold the adapter at load time)", name.c_str(), h->cfg.layers);
		const ttk_weight_view*& slot = tail == ".lora_A" ? plan[it->second].A : plan[it->second].B;
		TTK_REQUIRE(slot == nullptr, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s' is given twice", name.c_str());
		TTK_REQUIRE(v->ndim == 2, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s' has %d dimensions, expected 2", name.c_str(), v->ndim);
		slot = v;
	}
	for (int i = 0; i < nm; ++i) {
		const LoraPair& p = plan[i];
		if (!p.A && !p.B) continue;
		const std::string mod = lora_module(i);
		TTK_REQUIRE(p.A && p.B, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s.lora_%s' is given without '%s.lora_%s': an adapter is the pair", mod.c_str(), p.A ? "A" : "B", mod.c_str(),
					p.A ? "B" : "A");
		const Mat* m = lora_mat(h, i);
		const int64_t r = p.A->shape[0];
		TTK_REQUIRE(r >= 1 && r <= LORA_MAX_RANK, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s.lora_A' has rank %lld: ranks 1..%d are supported", mod.c_str(), (long long)r, LORA_MAX_RANK);
		TTK_REQUIRE(p.A->shape[1] == m->N, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s.lora_A' is [%lld, %lld], expected [rank, %d] for the weight [%d, %d]", mod.c_str(), (long long)r,
					(long long)p.A->shape[1], m->N, m->K, m->N);
		TTK_REQUIRE(p.B->shape[0] == m->K && p.B->shape[1] == r, TTK_E_WEIGHT, "ttk_ar_lora_set: '%s.lora_B' is [%lld, %lld], expected [%d, %lld] for the weight [%d, %d] and rank %lld",
					mod.c_str(), (long long)p.B->shape[0], (long long)p.B->shape[1], m->K, (long long)r, m->K, m->N, (long long)r);
	}
	hipStream_t s = (hipStream_t)stream;
	for (int i = 0; i < nm; ++i) {
		const LoraPair& p = plan[i];
		const bool adapt = p.A != nullptr;
		if (!adapt && !h->lora_adapted[i]) continue;      // base before, base after: its operands are what they should be
		Mat* m = lora_mat(h, i);
		const ARLayer& L = h->L[i / 4];
		const bool folded = m->wfrag_fold != nullptr;
		const float* src = h->lora_master[i];
		if (adapt) {
			launch_lora_update(h->lora_master[i], p.B->data, p.A->data, m->K, m->N, (int)p.A->shape[0], scaling, h->lora_scratch, s);
			src = h->lora_scratch;
		} else if (folded) {      // pack_fold scales its source in place: the master stays as it is
			TTK_HIP(hipMemcpyAsync(h->lora_scratch, h->lora_master[i], (size_t)m->N * m->K * sizeof(float), hipMemcpyDeviceToDevice, s));
			src = h->lora_scratch;
		}
		pack_mat(h->wdt, src, PK_KN, *m, s);
		if (folded) {
			const bool first = i % 4 == 0;      // c_attn behind ln_1, c_fc behind ln_2
			pack_fold(h->dt, h->lora_scratch, first ? L.ln1_g : L.ln2_g, first ? L.ln1_b : L.ln2_b, m->bias, h->lora_wt, *m, s);
		}
		h->lora_adapted[i] = adapt;
	}
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
