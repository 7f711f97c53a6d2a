// ttk_diff: the diffusion half of the hot path -- DiffusionTTS and the per-step sampler behind the C ABI of include/ttk.h.
// Internal layout is channels-last ([b*T rows][C]) so every 1x1 conv is an NT GEMM on the conv weight as stored and the
// k=3 convs are 3 row-shifted GEMM segments; the boundary stays the reference's [b, C, T].
// The conditioned and the conditioning-free evaluation of a sampler step run as ONE batch of 2b sequences (same x, same t,
// different code embedding) so each weight is read once per step.
// Reference: /root/reference/tortoise_tts/models/diffusion.py:1316-1574 (ResBlock, DiffusionLayer, DiffusionTTS),
//            :325-431,646-694,510-554 (p_mean_variance, ddim_sample, p_sample); arch_utils.py:136-190 (AttentionBlock).
#include <stdlib.h>

#include "ttk_common.h"
#include "ttk_host.h"

using namespace ttk;

namespace {
struct AttnBlk { float *gn_g, *gn_b; Mat qkv, proj; float* relbias; };
struct ResBlk { float *gn1_g, *gn1_b, *gn2_g, *gn2_b; Mat in, out3; int emb_slot; };
struct DLayer { ResBlk res; AttnBlk attn; };
// the scratch a chain of ResBlocks / AttentionBlocks works in; two of them so that the conditioning integrator of the NEXT sampler step
// can run on a side stream beside the main body of the current one
struct Lane {
	WsBuf a, hf, qkv, ao, ms;
	const void* ms_owner = nullptr;   // tensor whose GroupNorm statistics a GEMM epilogue has just written (gemm() sets it, stats_of() takes it)
};
// the A operand of a GEMM: row-shifted / concatenated segments of K columns each
struct Segs { int n, K, rows_per_batch; GemmSeg s[3]; };
// what rides on a GEMM's epilogue beyond the bias.  gn_T > 0: the output is a GroupNorm input of gn_T rows per batch element, whose statistics go to `ms` (null: the
// lane's); residual: f32 in the output's layout (may be the output); transpose: the output is [b][N][rows_per_batch]
struct Epi { int gn_T = 0; const float* residual = nullptr; float* ms = nullptr; int act = ACT_NONE; int transpose = 0; };
// one GroupNorm-apply launch.  next: the GEMM that consumes the output -- its weights are touched into L2 meanwhile, and fp8 weights make the output fp8;
// mod: rows of [scale C | shift C], one per batch element `mod_stride` apart (0: shared); ms: the statistics when computed beforehand (else stats_of);
// out: null = the lane's `a` in the kernel type; row_idx: nearest-neighbour row gather to Tout rows
struct Gn {
	const float *gamma, *beta; int act; const Mat* next = nullptr; const float* mod = nullptr; int64_t mod_stride = 0; const float* ms = nullptr;
	void* out = nullptr; int out_f32 = 0; const int* row_idx = nullptr; int Tout = 0;
};
// one sampler step of a loop.  nb: 2b sequences with the conditioning-free evaluation, else b; emb: its row of emb_all; noise: its block (ancestral sampler) or null;
// layout: the channels-last copy of x is not there yet, the step runs the layout launch; stage_next: its update launch also writes the next step's copy (same batch
// layout in both; not for ragged batches, whose padding frames must read zero)
// ext / pred_xstart: the step runs the extended update (ttk_diff_sample_ext, ttk_diff_step_ext); null on the loops that predate it
// ms / x0_hist: the step runs the multistep update (ttk_diff_sample_ms, ttk_diff_sample_ms_lines, ttk_diff_step_ms) on that history buffer
struct StepPlan {
	const ttk_step* st; int nb; const float* emb; const float* noise; bool layout, stage_next; const ttk_step_ext* ext = nullptr; float* pred_xstart = nullptr;
	const ttk_step_ms* ms = nullptr; float* x0_hist = nullptr;
};
}  // namespace

struct ttk_diff {
	ttk_diff_config cfg;
	int dt, wdt;            // kernel arithmetic type / storage type of the block GEMM weights (== dt, DT_FP8W or DT_FP8)
	size_t es;
	Arena arena;
	AttnBlk lat_attn[4];
	Mat lat_conv, inp_block, integ, out_conv, time0, time2, emb_cat;
	float *code_g, *code_b, *out_g, *out_b, *uncond, *time_freqs;
	// token conditioning (optional: present when the create call was given `code_embedding.weight`): the table in the kernel type, code_converter, mel_head
	void* code_table = nullptr; int in_tokens = 0;
	AttnBlk code_attn[3];
	Mat mel_head;
	DLayer integrator[3];
	std::vector<DLayer> layers;
	ResBlk tail[3];
	int n_emb;               // number of ResBlocks = rows of emb_cat / 2C
	int in_pad;              // in_channels rounded up to 64
	// workspaces
	Lane lane[2];
	Lane* L = &lane[0];      // the lane the block helpers below enqueue into (host code is sequential: flipped around the side-stream work)
	WsBuf cs, cs2, xs, h0, csT, xcl, outb, ecl, ms_ecl, temb, e1, e2, se, emb_all, lat_T;
	WsBuf x0h;              // the x0 history of the multistep sampler's loops (ttk_diff_sample_ms, ttk_diff_sample_ms_lines): [b][in][T] f32, grow-only, written before it is read
	WsBuf hf0, ms_hf0;      // in_layers of the FIRST integrator ResBlock applied to the staged embedding (+ the GroupNorm statistics of the result): the same in every step
	hipStream_t side = nullptr;
	hipEvent_t ev_fork = nullptr, ev_int[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
	int pipe = 1;           // ttk_diff_sample_ddim overlaps step i+1's integrator with step i's body (TTK_DIFF_PIPE=0: sequential)
	int cur_b = 0, cur_T = 0, staged = 0;
	int fuse_stats = 1;
	// ragged batch (ttk_diff_sample_ddim_lines): per-sequence valid rows inside the common slot of cur_T rows, [cond b | uncond b]; d_need marks
	// the sequences whose GroupNorm statistics cannot come from a GEMM epilogue (length not a multiple of its 64-row blocks): they get the
	// separate statistics launch, exactly as a batch of their own length would
	int* d_tlen = nullptr; int* d_need = nullptr;
	const int* tlen = nullptr; const int* need = nullptr;      // = d_tlen / d_need while a ragged loop runs, else null
	~ttk_diff() {            // the side stream and events are made on first use; the workspaces and the arena free themselves after this
		if (side) (void)hipStreamDestroy(side);
		for (hipEvent_t e : {ev_fork, ev_int[0], ev_int[1], ev_free[0], ev_free[1]}) if (e) (void)hipEventDestroy(e);
	}
};

static Segs rows_of(const void* A, const Mat& m) { return {1, m.Kpad, 0, {{A, m.Kpad, 0, 0}}}; }
// k=3 'same' conv over rows inside each batch element of Tper rows: tap j multiplies row t + j - 1
static Segs taps3(const void* A, int64_t lda, const Mat& m, int Tper) {
	const int64_t tap = (int64_t)m.Npad * m.Kpad;
	return {3, m.Kpad, Tper, {{A, lda, -1, 0}, {A, lda, 0, tap}, {A, lda, 1, 2 * tap}}};
}

// Every GEMM of the network: C [M][ldc] = epilogue(A . m^T).  With e.gn_T the statistics of the output are produced in the epilogue when the shape
// allows (gemm_fuses_gn_stats), which saves the separate k_gn_stats launch; stats_of() finds out through ms_owner.
static void gemm(ttk_diff* h, const Mat& m, const Segs& a, int M, void* C, int64_t ldc, int out_f32, hipStream_t s, const Epi& e = {}) {
	GemmParams g = {};
	g.nseg = a.n;
	for (int j = 0; j < a.n; ++j) g.seg[j] = a.s[j];
	g.W = m.w; g.ldw = m.Kpad; g.M = M; g.N = m.N; g.K = a.K; g.rows_per_batch = a.rows_per_batch; g.bias = m.bias;
	g.residual = e.residual; g.ldr = ldc; g.C = C; g.ldc = ldc; g.out_f32 = out_f32; g.act = e.act; g.transpose_out = e.transpose;
	if (m.wes == 1) g.out_scale = m.wscale;      // fp8 operands (A is fp8 too: written by gn() / the attention for exactly these matrices)
	h->L->ms_owner = nullptr;
	if (h->fuse_stats && e.gn_T > 0 && out_f32 && !e.transpose && gemm_fuses_gn_stats(M, m.N, h->cfg.model_channels, e.gn_T)) {
		g.gn_part = e.ms ? e.ms : (float*)h->L->ms.p; g.gn_T = e.gn_T; h->L->ms_owner = C;
	}
	launch_gemm(m.wes == 1 ? DT_FP8 : h->dt, g, s);
}

// The GroupNorm statistics of x (nb sequences in slots of T rows) in `ms` (null: the lane's; the buffer the producing GEMM was given): left there by that
// GEMM's epilogue -- except for the ragged sequences of a batch whose length the epilogue cannot serve, which get the separate launch -- or computed now.
static const float* stats_of(ttk_diff* h, const float* x, int nb, int T, hipStream_t s, float* ms = nullptr) {
	if (!ms) ms = (float*)h->L->ms.p;
	const bool fused = h->L->ms_owner == (const void*)x;
	h->L->ms_owner = nullptr;
	if (!fused || h->need) launch_gn_stats(x, nb, T, h->cfg.model_channels, ms, s, h->tlen, fused ? h->need : nullptr);
	return ms;
}

static void gn(ttk_diff* h, const float* x, int nb, int T, const Gn& d, hipStream_t s) {
	const int C = h->cfg.model_channels;
	GnApplyParams p = {};
	p.row_idx = d.row_idx; p.nb = nb; p.T = T; p.Tout = d.row_idx ? d.Tout : T; p.C = C; p.nchunks = gn_num_chunks(T, C);
	if (h->tlen && !d.row_idx) { p.tlen = h->tlen; p.chunk_rows = gn_rows_per_chunk(C); }
	p.x = x; p.ms = d.ms ? d.ms : stats_of(h, x, nb, T, s); p.gamma = d.gamma; p.beta = d.beta; p.act = d.act;
	if (d.mod) { p.scale = d.mod; p.shift = d.mod + C; p.ss_stride = d.mod_stride; }
	p.out = d.out ? d.out : h->L->a.p; p.out_f32 = d.out_f32;
	if (d.next) { p.pf = d.next->w; p.pf_bytes = (int64_t)d.next->Npad * d.next->Kpad * d.next->wes; p.pf_taps = d.next->ntap; p.out_f8 = d.next->wes == 1; }
	launch_gn_apply(h->dt, p, s);
}

// x (f32 stream, in place) = x + proj_out(attention(qkv(GN(x))))         arch_utils.py:183-190
static void attn_block(ttk_diff* h, const AttnBlk& A, float* x, int nb, int T, hipStream_t s) {
	const int C = h->cfg.model_channels, rows = nb * T;
	gn(h, x, nb, T, {A.gn_g, A.gn_b, ACT_NONE, &A.qkv}, s);
	gemm(h, A.qkv, rows_of(h->L->a.p, A.qkv), rows, h->L->qkv.p, 3 * C, 0, s);
	AttnParams a = {};
	a.qkv = h->L->qkv.p; a.ld = 3 * C; a.q_off = 0; a.k_off = 64; a.v_off = 128; a.head_stride = 192;   // head-major [H][3][64], arch_utils.py:79
	a.out = h->L->ao.p; a.ldo = C; a.nb = nb; a.T = T; a.H = h->cfg.num_heads; a.causal = 0; a.bias = A.relbias; a.scale = 0.125f; a.tlen = h->tlen;
	a.pf = A.proj.w; a.pf_bytes = (int64_t)A.proj.Npad * A.proj.Kpad * A.proj.wes; a.pf_taps = 1;
	a.out_f8 = A.proj.wes == 1;
	launch_attn_fwd(h->dt, a, s);
	gemm(h, A.proj, rows_of(h->L->ao.p, A.proj), rows, x, C, 1, s, {T, x});
}

// x = x + conv3(SiLU(GN(conv1(SiLU(GN(x)))) * (1 + scale) + shift))        diffusion.py:1363-1376, in its two halves: the timestep enters a ResBlock only
// behind the first, as the scale / shift of the second GroupNorm.
// res_in: hf = conv1(SiLU(GN(x))), hf's statistics into ms_hf (null: the lane's); ms_x: x's statistics when computed beforehand
static void res_in(ttk_diff* h, const ResBlk& R, const float* x, int nb, int T, hipStream_t s, float* hf, const float* ms_x = nullptr, float* ms_hf = nullptr) {
	gn(h, x, nb, T, {R.gn1_g, R.gn1_b, ACT_SILU, &R.in, nullptr, 0, ms_x}, s);
	gemm(h, R.in, rows_of(h->L->a.p, R.in), nb * T, hf, h->cfg.model_channels, 1, s, {T, nullptr, ms_hf});
}
// res_out: x = res + conv3(SiLU(GN(hf) * (1 + scale) + shift)); ms_hf: hf's statistics when computed beforehand
static void res_out(ttk_diff* h, const ResBlk& R, const float* hf, const float* ms_hf, const float* res, float* x, int nb, int T, const float* emb_all,
					int64_t emb_stride, hipStream_t s) {
	const int C = h->cfg.model_channels;
	gn(h, hf, nb, T, {R.gn2_g, R.gn2_b, ACT_SILU, &R.out3, emb_all + (int64_t)R.emb_slot * 2 * C, emb_stride, ms_hf}, s);
	gemm(h, R.out3, taps3(h->L->a.p, C, R.out3, T), nb * T, x, C, 1, s, {T, res});
}
static void res_block(ttk_diff* h, const ResBlk& R, float* x, int nb, int T, const float* emb_all, int64_t emb_stride, hipStream_t s) {
	res_in(h, R, x, nb, T, s, (float*)h->L->hf.p);
	res_out(h, R, (const float*)h->L->hf.p, nullptr, x, x, nb, T, emb_all, emb_stride, s);
}

static int reserve_lane(ttk_diff* h, Lane& L, int nb, int T) {
	const size_t rows = (size_t)nb * T, C = h->cfg.model_channels, es = h->es;
	TTK_TRY(L.hf.reserve(rows * C * 4)); TTK_TRY(L.a.reserve(rows * C * es)); TTK_TRY(L.qkv.reserve(rows * 3 * C * es)); TTK_TRY(L.ao.reserve(rows * C * es));
	TTK_TRY(L.ms.reserve((size_t)nb * 32 * gn_num_chunks(T, (int)C) * 3 * 4));
	return TTK_OK;
}
static int reserve_ws(ttk_diff* h, int nb, int T) {
	TTK_REQUIRE(gn_num_chunks(T, h->cfg.model_channels) <= 64, TTK_E_ARG, "%d frames exceed the GroupNorm chunk table (64 chunks)", T);
	const size_t rows = (size_t)nb * T, C = h->cfg.model_channels, es = h->es;
	h->L = &h->lane[0];
	TTK_TRY(reserve_lane(h, h->lane[0], nb, T));
	TTK_TRY(h->cs.reserve(rows * C * 4)); TTK_TRY(h->xs.reserve(rows * C * 4));
	TTK_TRY(h->h0.reserve(rows * C * es)); TTK_TRY(h->csT.reserve(rows * C * es)); TTK_TRY(h->xcl.reserve(rows * h->in_pad * es));
	TTK_TRY(h->outb.reserve(rows * h->cfg.out_channels * 4)); TTK_TRY(h->ecl.reserve(rows * C * 4));
	return TTK_OK;
}

// time_embed MLP + every ResBlock's emb_layers for n timestep rows -> emb_all f32 [n][n_emb * 2C]    diffusion.py:1549, :1365
static int time_path(ttk_diff* h, const int64_t* t_dev, const int64_t* t_host, int n, hipStream_t s) {
	const int C = h->cfg.model_channels;
	const size_t es = h->es;
	TTK_TRY(h->temb.reserve((size_t)n * C * es)); TTK_TRY(h->e1.reserve((size_t)n * C * es)); TTK_TRY(h->e2.reserve((size_t)n * C * 4));
	TTK_TRY(h->se.reserve((size_t)n * C * es)); TTK_TRY(h->emb_all.reserve((size_t)n * h->n_emb * 2 * C * 4));
	if (t_dev) launch_timestep_embedding(h->dt, t_dev, 0, n, C, h->time_freqs, h->temb.p, s);
	else for (int i = 0; i < n; ++i) launch_timestep_embedding(h->dt, nullptr, t_host[i], 1, C, h->time_freqs, (char*)h->temb.p + (size_t)i * C * es, s);
	Epi silu; silu.act = ACT_SILU;
	gemm(h, h->time0, rows_of(h->temb.p, h->time0), n, h->e1.p, C, 0, s, silu);
	gemm(h, h->time2, rows_of(h->e1.p, h->time2), n, h->e2.p, C, 1, s);
	launch_silu_cast(h->dt, (const float*)h->e2.p, h->se.p, (int64_t)n * C, s);
	gemm(h, h->emb_cat, rows_of(h->se.p, h->emb_cat), n, h->emb_all.p, (int64_t)h->n_emb * 2 * C, 1, s);
	return TTK_OK;
}

// One evaluation = integrator (the three conditioning_timestep_integrator layers on the code-embedding stream `cs`; depends on the timestep
// only, not on x) + body (everything that sees x).  Inputs of the body: h->xcl (T-typed [nb*T][in_pad]) and cs (f32 [nb*T][C]); emb rows at
// emb_all + b * emb_stride.  Output: out f32 [nb][out_channels][T].     diffusion.py:1549-1564
// staged: the loop's form -- the first block reads the staged embedding (ttk_diff_begin: ecl, and the first half of that block on it in hf0 / ms_hf0, the same
// in every step) and writes cs; else cs holds the embedding and is integrated in place
static void integrator(ttk_diff* h, int nb, int T, const float* emb_all, int64_t emb_stride, float* cs, hipStream_t s, bool staged) {
	for (int i = 0; i < 3; ++i) {
		const ResBlk& R = h->integrator[i].res;
		if (i == 0 && staged) res_out(h, R, (const float*)h->hf0.p, (const float*)h->ms_hf0.p, (const float*)h->ecl.p, cs, nb, T, emb_all, emb_stride, s);
		else res_block(h, R, cs, nb, T, emb_all, emb_stride, s);
		attn_block(h, h->integrator[i].attn, cs, nb, T, s);
	}
}
static void body(ttk_diff* h, int nb, int T, const float* emb_all, int64_t emb_stride, const float* cs, float* out, hipStream_t s,
				 hipEvent_t cs_consumed = nullptr) {
	const int C = h->cfg.model_channels, rows = nb * T;
	float* x = (float*)h->xs.p;
	gemm(h, h->inp_block, taps3(h->xcl.p, h->in_pad, h->inp_block, T), rows, h->h0.p, C, 0, s);
	launch_cast(h->dt, cs, h->csT.p, (int64_t)rows * C, s);
	if (cs_consumed) (void)hipEventRecord(cs_consumed, s);     // the last reader of `cs`: the side stream may overwrite it from here on
	// integrating_conv over cat([h0, code_emb], channels): two K segments of one [C][2C] matrix
	gemm(h, h->integ, {2, C, 0, {{h->h0.p, C, 0, 0}, {h->csT.p, C, 0, C}}}, rows, x, C, 1, s, {T});
	for (size_t i = 0; i < h->layers.size(); ++i) {
		res_block(h, h->layers[i].res, x, nb, T, emb_all, emb_stride, s);
		attn_block(h, h->layers[i].attn, x, nb, T, s);
	}
	for (int i = 0; i < 3; ++i) res_block(h, h->tail[i], x, nb, T, emb_all, emb_stride, s);
	gn(h, x, nb, T, {h->out_g, h->out_b, ACT_SILU}, s);
	Epi t; t.transpose = 1;
	gemm(h, h->out_conv, taps3(h->L->a.p, C, h->out_conv, T), rows, out, 0, 1, s, t);
}

static int load_attn(ttk_diff* h, const WeightMap& wm, const std::string& p, AttnBlk* A) {
	const int C = h->cfg.model_channels;
	TTK_TRY(upload_f32(h->arena, wm, p + "norm.weight", C, &A->gn_g));
	TTK_TRY(upload_f32(h->arena, wm, p + "norm.bias", C, &A->gn_b));
	// The q / k / v projection stays in the handle's 16-bit type in the fp8 modes, weights and activation operand alike (round 6): e4m3's three significand bits
	// on q and k move scores of +-100 by whole units -- the peaked-attention regime of a trained checkpoint lost 37-42 % of an evaluation to it, against
	// 12 % for bf16 (profiles/r05_stress_errors.json) -- while this GEMM is a seventh of a block's flops.
	TTK_TRY(upload_mat(h->arena, wm, h->dt, p + "qkv.weight", p + "qkv.bias", PK_NK, 3 * C, C, false, &A->qkv));
	TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "proj_out.weight", p + "proj_out.bias", PK_NK, C, C, false, &A->proj));
	TTK_TRY(upload_f32(h->arena, wm, p + "__relbias", (int64_t)h->cfg.num_heads * 129, &A->relbias));
	return TTK_OK;
}
static int load_res(ttk_diff* h, const WeightMap& wm, const std::string& p, ResBlk* R, int slot) {
	const int C = h->cfg.model_channels;
	TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.0.weight", C, &R->gn1_g));
	TTK_TRY(upload_f32(h->arena, wm, p + "in_layers.0.bias", C, &R->gn1_b));
	TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.0.weight", C, &R->gn2_g));
	TTK_TRY(upload_f32(h->arena, wm, p + "out_layers.0.bias", C, &R->gn2_b));
	TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "in_layers.2.weight", p + "in_layers.2.bias", PK_NK, C, C, false, &R->in));
	TTK_TRY(upload_mat(h->arena, wm, h->wdt, p + "out_layers.3.weight", p + "out_layers.3.bias", PK_CONV3, C, C, false, &R->out3));
	R->emb_slot = slot;
	return TTK_OK;
}

// The tail both kinds of aligned conditioning share: code_norm(x) * (1 + scale) + shift, nearest-neighbour expansion M -> T into ecl (f32 channels-last), and the
// channels-first copy the caller gets      diffusion.py:1492,1498,1507
static void precompute_tail(ttk_diff* h, const float* x, const float* cond, const int32_t* interp_idx, int b, int M, int T, float* E_out, hipStream_t s) {
	const int C = h->cfg.model_channels;
	Gn d = {h->code_g, h->code_b, ACT_NONE, nullptr, cond, 2 * C};
	d.out = h->ecl.p; d.out_f32 = 1; d.row_idx = interp_idx; d.Tout = T;
	gn(h, x, b, M, d, s);
	launch_cl_to_cf((const float*)h->ecl.p, b, C, T, E_out, s);
}
// mel_pred [b][in_channels][T] f32 = mel_head(E), a k = 3 convolution over the expanded embedding (diffusion.py:1512): the GEMM form of `out`, its 100 output
// channels padded to the tile the same way.  from_ecl: the operand copy in the kernel type is made from ecl; else the caller has put it into csT.
static void mel_head_of(ttk_diff* h, int b, int T, float* out, hipStream_t s, bool from_ecl) {
	const int C = h->cfg.model_channels;
	if (from_ecl) launch_cast(h->dt, (const float*)h->ecl.p, h->csT.p, (int64_t)b * T * C, s);
	Epi t; t.transpose = 1;
	gemm(h, h->mel_head, taps3(h->csT.p, C, h->mel_head, T), b * T, out, 0, 1, s, t);
}

extern "C" {

int ttk_diff_create(ttk_diff** out, const ttk_diff_config* cfg, const ttk_weight_view* w, int n_w) {
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_diff_create: null argument");
	gemm_roles_refresh();
	TTK_REQUIRE(cfg->model_channels % 64 == 0 && cfg->num_heads * 64 == cfg->model_channels, TTK_E_ARG,
				"ttk_diff_create: head_dim must be 64 (channels %d, heads %d)", cfg->model_channels, cfg->num_heads);
	TTK_REQUIRE(cfg->in_latent_channels % 64 == 0, TTK_E_ARG, "ttk_diff_create: in_latent_channels %% 64 != 0");
	TTK_REQUIRE(cfg->model_channels % 128 == 0 && cfg->model_channels <= 1024 && 1024 % cfg->model_channels == 0, TTK_E_ARG,
				"ttk_diff_create: model_channels %d unsupported (128, 256, 512 or 1024)", cfg->model_channels);
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16 || cfg->dtype == TTK_F16 || cfg->dtype == TTK_FP8W || cfg->dtype == TTK_FP8, TTK_E_ARG, "ttk_diff_create: bad dtype %d", cfg->dtype);
	TTK_REQUIRE(cfg->dtype != TTK_FP8 || cfg->model_channels % 128 == 0, TTK_E_ARG, "ttk_diff_create: fp8 GEMMs need channels %% 128 == 0");
	std::unique_ptr<ttk_diff> h(new ttk_diff());
	h->cfg = *cfg;
	h->wdt = cfg->dtype;              // ResBlock / AttentionBlock GEMM weights: rounded to fp8-e4m3 in DT_FP8W (held exactly in bf16)
	h->dt = kernel_dtype(cfg->dtype);
	h->es = dtype_size(h->dt);
	h->in_pad = round_up(cfg->in_channels, 64);
	h->fuse_stats = getenv("TTK_NO_FUSED_GN") ? 0 : 1;
	{ const char* e = getenv("TTK_DIFF_PIPE"); h->pipe = e ? atoi(e) : 1; }
	const int C = cfg->model_channels;
	WeightMap wm(w, n_w);
	TTK_TRY(upload_f32(h->arena, wm, "unconditioned_embedding", C, &h->uncond));
	TTK_TRY(upload_f32(h->arena, wm, "__time_freqs", C / 2, &h->time_freqs));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "inp_block.weight", "inp_block.bias", PK_CONV3, C, cfg->in_channels, false, &h->inp_block));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "time_embed.0.weight", "time_embed.0.bias", PK_NK, C, C, false, &h->time0));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "time_embed.2.weight", "time_embed.2.bias", PK_NK, C, C, false, &h->time2));
	TTK_TRY(upload_f32(h->arena, wm, "code_norm.weight", C, &h->code_g));
	TTK_TRY(upload_f32(h->arena, wm, "code_norm.bias", C, &h->code_b));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "latent_conditioner.0.weight", "latent_conditioner.0.bias", PK_CONV3, C, cfg->in_latent_channels, false, &h->lat_conv));
	for (int i = 0; i < 4; ++i) TTK_TRY(load_attn(h.get(), wm, "latent_conditioner." + std::to_string(i + 1) + ".", &h->lat_attn[i]));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "integrating_conv.weight", "integrating_conv.bias", PK_NK, C, 2 * C, false, &h->integ));
	TTK_TRY(upload_f32(h->arena, wm, "out.0.weight", C, &h->out_g));
	TTK_TRY(upload_f32(h->arena, wm, "out.0.bias", C, &h->out_b));
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "out.2.weight", "out.2.bias", PK_CONV3, cfg->out_channels, C, false, &h->out_conv));
	int slot = 0;
	for (int i = 0; i < 3; ++i) {
		const std::string p = "conditioning_timestep_integrator." + std::to_string(i) + ".";
		TTK_TRY(load_res(h.get(), wm, p + "resblk.", &h->integrator[i].res, slot++));
		TTK_TRY(load_attn(h.get(), wm, p + "attn.", &h->integrator[i].attn));
	}
	h->layers.resize(cfg->num_layers);
	for (int i = 0; i < cfg->num_layers; ++i) {
		const std::string p = "layers." + std::to_string(i) + ".";
		TTK_TRY(load_res(h.get(), wm, p + "resblk.", &h->layers[i].res, slot++));
		TTK_TRY(load_attn(h.get(), wm, p + "attn.", &h->layers[i].attn));
	}
	for (int i = 0; i < 3; ++i) TTK_TRY(load_res(h.get(), wm, "layers." + std::to_string(cfg->num_layers + i) + ".", &h->tail[i], slot++));
	h->n_emb = slot;
	if (const ttk_weight_view* tv = wm.find("code_embedding.weight")) {
		// in_tokens is the table's own row count: ttk_diff_config stays as it is
		TTK_REQUIRE(tv->ndim == 2 && tv->shape[0] >= 1 && tv->shape[0] < (1LL << 31) && tv->shape[1] == C, TTK_E_WEIGHT,
					"ttk_diff_create: code_embedding.weight must be [in_tokens][%d]", C);
		h->in_tokens = (int)tv->shape[0];
		const int64_t n = (int64_t)h->in_tokens * C;
		if (h->dt == DT_F32) { float* t = nullptr; TTK_TRY(upload_f32(h->arena, wm, "code_embedding.weight", n, &t)); h->code_table = t; }
		else {
			WsBuf tmp;
			TTK_TRY(tmp.reserve((size_t)n * 4));
			TTK_HIP(hipMemcpy(tmp.p, tv->data, (size_t)n * 4, hipMemcpyDefault));
			TTK_TRY(h->arena.alloc(&h->code_table, (size_t)n * h->es));
			launch_cast(h->dt, (const float*)tmp.p, h->code_table, n, 0);
			TTK_HIP(hipDeviceSynchronize());
		}
		for (int i = 0; i < 3; ++i) TTK_TRY(load_attn(h.get(), wm, "code_converter." + std::to_string(i) + ".", &h->code_attn[i]));
		TTK_TRY(upload_mat(h->arena, wm, h->dt, "mel_head.weight", "mel_head.bias", PK_CONV3, cfg->in_channels, C, false, &h->mel_head));
	}
	TTK_TRY(h->arena.alloc((void**)&h->d_tlen, 128 * sizeof(int)));
	TTK_TRY(h->arena.alloc((void**)&h->d_need, 128 * sizeof(int)));
	// all emb_layers.1 linears stacked into one [n_emb * 2C][C] matrix ("__emb_cat.*", built by the Python packer)
	TTK_TRY(upload_mat(h->arena, wm, h->dt, "__emb_cat.weight", "__emb_cat.bias", PK_NK, h->n_emb * 2 * C, C, false, &h->emb_cat));
	hipError_t e = hipDeviceSynchronize();
	if (e != hipSuccess) { set_error("ttk_diff_create: %s", hipGetErrorString(e)); return TTK_E_HIP; }
	*out = h.release();
	return TTK_OK;
}

int ttk_diff_destroy(ttk_diff* h) {
	if (!h) return TTK_OK;
	(void)hipDeviceSynchronize();
	delete h;
	return TTK_OK;
}

int ttk_diff_precompute(ttk_diff* h, const float* latents, const float* cond, const int32_t* interp_idx, int b, int M, int T,
						float* E_out, void* stream) {
	TTK_REQUIRE(h && latents && cond && interp_idx && E_out, TTK_E_ARG, "ttk_diff_precompute: null argument");
	TTK_REQUIRE(b >= 1 && M >= 1 && T >= 1, TTK_E_ARG, "ttk_diff_precompute: empty input (b=%d M=%d T=%d)", b, M, T);
	const int C = h->cfg.model_channels, Cl = h->cfg.in_latent_channels;
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(reserve_ws(h, b, M > T ? M : T));
	h->staged = 0;   // ecl is reused below
	TTK_TRY(h->lat_T.reserve((size_t)b * M * Cl * h->es));
	float* x = (float*)h->xs.p;
	launch_cast(h->dt, latents, h->lat_T.p, (int64_t)b * M * Cl, s);   // latents are already [b][M][Cl] = channels-last
	gemm(h, h->lat_conv, taps3(h->lat_T.p, Cl, h->lat_conv, M), b * M, x, C, 1, s, {M});
	for (int i = 0; i < 4; ++i) attn_block(h, h->lat_attn[i], x, b, M, s);
	precompute_tail(h, x, cond, interp_idx, b, M, T, E_out, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diff_precompute_codes(ttk_diff* h, const int64_t* codes, const float* cond, const int32_t* interp_idx, int b, int M, int T,
							  float* E_out, float* mel_pred_out, void* stream) {
	TTK_REQUIRE(h && codes && cond && interp_idx && E_out, TTK_E_ARG, "ttk_diff_precompute_codes: null argument");
	TTK_REQUIRE(h->code_table, TTK_E_STATE, "ttk_diff_precompute_codes: the handle was created without code_embedding / code_converter / mel_head");
	TTK_REQUIRE(b >= 1 && M >= 1 && T >= 1, TTK_E_ARG, "ttk_diff_precompute_codes: empty input (b=%d M=%d T=%d)", b, M, T);
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(reserve_ws(h, b, M > T ? M : T));
	h->staged = 0;   // ecl is reused below
	float* x = (float*)h->xs.p;
	launch_embed_rows(h->dt, h->code_table, codes, b * M, h->cfg.model_channels, h->in_tokens, x, s);      // diffusion.py:1496
	h->L->ms_owner = nullptr;      // x's statistics come from the separate launch, as for any tensor no GEMM wrote
	for (int i = 0; i < 3; ++i) attn_block(h, h->code_attn[i], x, b, M, s);
	precompute_tail(h, x, cond, interp_idx, b, M, T, E_out, s);
	if (mel_pred_out) mel_head_of(h, b, T, mel_pred_out, s, true);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diff_mel_head(ttk_diff* h, const float* E, int b, int T, float* mel_pred_out, void* stream) {
	TTK_REQUIRE(h && E && mel_pred_out, TTK_E_ARG, "ttk_diff_mel_head: null argument");
	TTK_REQUIRE(h->code_table, TTK_E_STATE, "ttk_diff_mel_head: the handle was created without code_embedding / code_converter / mel_head");
	TTK_REQUIRE(b >= 1 && T >= 1, TTK_E_ARG, "ttk_diff_mel_head: empty input");
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(reserve_ws(h, b, T));
	h->staged = 0;   // the workspaces may have moved
	launch_cf_to_cl(h->dt, E, b, h->cfg.model_channels, T, h->csT.p, h->cfg.model_channels, 1, s);
	mel_head_of(h, b, T, mel_pred_out, s, false);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diff_forward(ttk_diff* h, const float* x, const int64_t* t, const float* E, int b, int T, float* out, void* stream) {
	TTK_REQUIRE(h && x && t && out, TTK_E_ARG, "ttk_diff_forward: null argument");
	TTK_REQUIRE(b >= 1 && T >= 1, TTK_E_ARG, "ttk_diff_forward: empty input");
	const int C = h->cfg.model_channels;
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(reserve_ws(h, b, T));
	h->staged = 0;
	if (E) launch_cf_to_cl(DT_F32, E, b, C, T, h->cs.p, C, 1, s);
	else launch_bcast_rows(DT_F32, h->uncond, b * T, C, h->cs.p, s);            // diffusion.py:1534
	launch_cf_to_cl(h->dt, x, b, h->cfg.in_channels, T, h->xcl.p, h->in_pad, 1, s);
	TTK_TRY(time_path(h, t, nullptr, b, s));
	const int64_t stride = (int64_t)h->n_emb * 2 * C;
	integrator(h, b, T, (const float*)h->emb_all.p, stride, (float*)h->cs.p, s, false);
	body(h, b, T, (const float*)h->emb_all.p, stride, (const float*)h->cs.p, out, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diff_begin(ttk_diff* h, const float* E, int b, int T, void* stream) {
	TTK_REQUIRE(h && E, TTK_E_ARG, "ttk_diff_begin: null argument");
	TTK_REQUIRE(b >= 1 && T >= 1, TTK_E_ARG, "ttk_diff_begin: empty input");
	const int C = h->cfg.model_channels;
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(reserve_ws(h, 2 * b, T));
	float* ecl = (float*)h->ecl.p;
	launch_cf_to_cl(DT_F32, E, b, C, T, ecl, C, 1, s);
	launch_bcast_rows(DT_F32, h->uncond, b * T, C, ecl + (size_t)b * T * C, s);
	// the staged embedding is the same in every step: its GroupNorm statistics once, here
	TTK_TRY(h->ms_ecl.reserve((size_t)2 * b * 32 * gn_num_chunks(T, C) * 3 * 4));
	launch_gn_stats(ecl, 2 * b, T, C, (float*)h->ms_ecl.p, s, h->tlen);
	h->cur_b = b; h->cur_T = T; h->staged = 1;
	// ... and so is the first half of the first integrator ResBlock on it, conv1x1(SiLU(GN(ecl))), with the statistics its second GroupNorm needs: the
	// same launches a step would run (so the same bits), once per utterance instead of once per step
	TTK_TRY(h->hf0.reserve((size_t)2 * b * T * C * 4)); TTK_TRY(h->ms_hf0.reserve((size_t)2 * b * 32 * gn_num_chunks(T, C) * 3 * 4));
	res_in(h, h->integrator[0].res, ecl, 2 * b, T, s, (float*)h->hf0.p, (const float*)h->ms_ecl.p, (float*)h->ms_hf0.p);
	stats_of(h, (const float*)h->hf0.p, 2 * b, T, s, (float*)h->ms_hf0.p);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

static StepCoefs coefs_of(const ttk_step& st) {
	return {st.sqrt_recip_ac, st.sqrt_recipm1_ac, st.sqrt_ac_prev, st.sqrt_1m_ac_prev, st.cfk, st.coef1, st.coef2, st.min_log, st.max_log, st.sampler, st.nonzero};
}
static_assert(sizeof(ttk_step_ext) == 24, "ttk_step_ext is mirrored by tortoise_tts_amd/_lib.py: StepExtC");
static StepExt ext_of(const ttk_step_ext& e) { return {e.sigma, e.dir, e.sqrt_ac_next, e.sqrt_1m_ac_next, e.mode, e.clip}; }
// does the extended update of this step read its noise block?
static bool ext_reads_noise(const ttk_step& st, const ttk_step_ext& e) { return st.nonzero && (e.mode == 1 || (e.mode == 0 && e.sigma != 0.f)); }
static int check_ext(const char* who, const ttk_step_ext& e, int i) {
	TTK_REQUIRE(e.mode >= 0 && e.mode <= 2, TTK_E_ARG, "%s: step %d has mode %d (0 ddim, 1 p, 2 reverse ddim)", who, i, e.mode);
	TTK_REQUIRE(e.sigma >= 0.f, TTK_E_ARG, "%s: step %d has sigma %g", who, i, (double)e.sigma);
	return TTK_OK;
}
static_assert(sizeof(ttk_step_ms) == 16, "ttk_step_ms is mirrored by tortoise_tts_amd/_lib.py: StepMsC");
static StepMs ms_of(const ttk_step_ms& m) { return {m.c_x, m.c_d0, m.c_d1, m.clip}; }
// The steps of a loop in the order they run: steps[n-1], ..., steps[0]; `noise` (ancestral sampler) holds one [b, in, T] draw per step in that order, null for ddim;
// emb_all has one row per schedule index.  One layout launch per run of steps with the same batch layout: each update launch writes the next step's copy of x.
// ascending (the reverse ODE of ttk_diff_sample_ext): steps[0], ..., steps[n-1] instead; ext: the extended update's per-step block, same indexing as steps.
static std::vector<StepPlan> plan_steps(ttk_diff* h, const ttk_step* steps, int n, const float* emb_all, int64_t emb_stride, const float* noise, const ttk_step_ext* ext = nullptr, bool ascending = false,
									const ttk_step_ms* ms = nullptr, float* x0_hist = nullptr) {
	const size_t nz = (size_t)h->cur_b * h->cfg.in_channels * h->cur_T;
	std::vector<StepPlan> plan(n);
	for (int j = 0; j < n; ++j) {
		const int i = ascending ? j : n - 1 - j;
		const int next = ascending ? i + 1 : i - 1;      // the step that runs after this one (outside 0 .. n-1: none)
		const bool cf = steps[i].cfk >= 0.f;
		StepPlan& p = plan[j];
		p.st = &steps[i]; p.nb = cf ? 2 * h->cur_b : h->cur_b; p.emb = emb_all + i * emb_stride; p.noise = noise ? noise + j * nz : nullptr;
		p.layout = j == 0 || !plan[j - 1].stage_next;
		p.stage_next = next >= 0 && next < n && !h->tlen && (steps[next].cfk >= 0.f) == cf;
		p.ext = ext ? ext + i : nullptr;
		p.ms = ms ? ms + i : nullptr; p.x0_hist = x0_hist;
	}
	return plan;
}

// the part of a sampler step that sees x: layout change, network body on the integrated code stream `cs`, the DDIM / ancestral update
static void step_body(ttk_diff* h, float* x, const StepPlan& p, const float* cs, hipEvent_t cs_consumed, hipStream_t s) {
	const int b = h->cur_b, T = h->cur_T, Cin = h->cfg.in_channels, rep = p.nb / b;
	if (p.layout) launch_cf_to_cl(h->dt, x, b, Cin, T, h->xcl.p, h->in_pad, rep, s, h->tlen);
	float* out = (float*)h->outb.p;
	body(h, p.nb, T, p.emb, 0, cs, out, s, cs_consumed);
	const float* out_u = out + (size_t)b * h->cfg.out_channels * T;
	if (p.ms) {
		if (p.stage_next) launch_diffusion_step_ms(out, out_u, x, p.x0_hist, p.pred_xstart, b, Cin, T, coefs_of(*p.st), ms_of(*p.ms), s, h->xcl.p, h->in_pad, rep, elem_kind(h->dt));
		else launch_diffusion_step_ms(out, out_u, x, p.x0_hist, p.pred_xstart, b, Cin, T, coefs_of(*p.st), ms_of(*p.ms), s);
		return;
	}
	if (p.ext) {
		if (p.stage_next) launch_diffusion_step_ext(out, out_u, x, p.noise, p.pred_xstart, b, Cin, T, coefs_of(*p.st), ext_of(*p.ext), s, h->xcl.p, h->in_pad, rep, elem_kind(h->dt));
		else launch_diffusion_step_ext(out, out_u, x, p.noise, p.pred_xstart, b, Cin, T, coefs_of(*p.st), ext_of(*p.ext), s);
		return;
	}
	if (p.stage_next) launch_diffusion_step(out, out_u, x, p.noise, b, Cin, T, coefs_of(*p.st), s, h->xcl.p, h->in_pad, rep, elem_kind(h->dt));      // (its padding columns are already zero)
	else launch_diffusion_step(out, out_u, x, p.noise, b, Cin, T, coefs_of(*p.st), s);
}

int ttk_diff_step(ttk_diff* h, float* x, const ttk_step* st, const float* noise, void* stream) {
	TTK_REQUIRE(h && x && st, TTK_E_ARG, "ttk_diff_step: null argument");
	TTK_REQUIRE(h->staged, TTK_E_STATE, "ttk_diff_step: call ttk_diff_begin first");
	TTK_REQUIRE(st->sampler == 0 || noise, TTK_E_ARG, "ttk_diff_step: the p sampler needs noise");
	TTK_REQUIRE(h->cfg.out_channels == 2 * h->cfg.in_channels, TTK_E_ARG, "ttk_diff_step: learned-range output needs out = 2 * in channels");
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(time_path(h, nullptr, &st->t, 1, s));
	const StepPlan p = plan_steps(h, st, 1, (const float*)h->emb_all.p, 0, noise)[0];
	integrator(h, p.nb, h->cur_T, p.emb, 0, (float*)h->cs.p, s, true);
	step_body(h, x, p, (const float*)h->cs.p, nullptr, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// The whole sampler loop, both samplers (see plan_steps for the order of steps and noise).
// ext (ttk_diff_sample_ext): the extended update with one block per step; `sampler` is then not looked at, the mode of ext[0] decides the order.
// ms (ttk_diff_sample_ms, ttk_diff_sample_ms_lines): the multistep update with one block per step, on the handle's history buffer; `sampler` is not looked at either.
static int sample_loop(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, int n_steps, const float* noise, int sampler, void* stream, const char* who,
					   const ttk_step_ext* ext = nullptr, const ttk_step_ms* ms = nullptr) {
	TTK_REQUIRE(h && x && E && steps && n_steps >= 1, TTK_E_ARG, "%s: bad argument", who);
	if (ext) {
		for (int i = 0; i < n_steps; ++i) {
			TTK_TRY(check_ext(who, ext[i], i));
			TTK_REQUIRE(ext[i].mode == ext[0].mode, TTK_E_ARG, "%s: step %d has mode %d, step 0 mode %d (one mode per loop)", who, i, ext[i].mode, ext[0].mode);
			TTK_REQUIRE(noise || !ext_reads_noise(steps[i], ext[i]), TTK_E_ARG, "%s: step %d adds noise (mode %d, sigma %g) but noise is null", who, i, ext[i].mode, (double)ext[i].sigma);
		}
	}
	else if (!ms) TTK_REQUIRE(sampler == 0 || noise, TTK_E_ARG, "%s: the p sampler needs one noise block per step", who);
	TTK_REQUIRE(h->cfg.out_channels == 2 * h->cfg.in_channels, TTK_E_ARG, "%s: learned-range output needs out = 2 * in channels", who);
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(ttk_diff_begin(h, E, b, T, stream));
	// the timestep-only work of ALL steps in one pass: [n_steps] rows through time_embed + every emb_layers (weights read once)
	std::vector<int64_t> ts(n_steps);
	for (int i = 0; i < n_steps; ++i) { ts[i] = steps[i].t; TTK_REQUIRE(ext || ms || steps[i].sampler == sampler, TTK_E_ARG, "%s: step %d has sampler %d", who, i, steps[i].sampler); }
	TTK_TRY(time_path(h, nullptr, ts.data(), n_steps, s));
	if (ms) TTK_TRY(h->x0h.reserve((size_t)b * h->cfg.in_channels * T * 4));
	const std::vector<StepPlan> plan = plan_steps(h, steps, n_steps, (const float*)h->emb_all.p, (int64_t)h->n_emb * 2 * h->cfg.model_channels, noise, ext, ext && ext[0].mode == 2,
												  ms, ms ? (float*)h->x0h.p : nullptr);
	// Pipelined over two streams.  The integrator of a step depends on its timestep and the staged embedding only, never on x: the one of
	// step j+1 runs on the side stream (own scratch lane, the other `cs` buffer) while the body of step j runs here.  Both are chains of
	// small dependent launches that leave most of the chip idle, so they overlap; one fork and one join edge per step.  Sequential
	// (TTK_DIFF_PIPE=0, or a single step): the same launches, each integrator in front of its body on the caller's stream.
	const bool pipe = h->pipe && n_steps >= 2;
	float* csb[2] = {(float*)h->cs.p, (float*)h->cs.p};
	if (pipe) {
		if (!h->side) {
			TTK_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
			TTK_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
			for (int i = 0; i < 2; ++i) {
				TTK_HIP(hipEventCreateWithFlags(&h->ev_int[i], hipEventDisableTiming));
				TTK_HIP(hipEventCreateWithFlags(&h->ev_free[i], hipEventDisableTiming));
			}
		}
		TTK_TRY(reserve_lane(h, h->lane[1], 2 * b, T));
		TTK_TRY(h->cs2.reserve((size_t)2 * b * T * h->cfg.model_channels * 4));
		csb[1] = (float*)h->cs2.p;
		TTK_HIP(hipEventRecord(h->ev_fork, s));
		TTK_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
	}
	auto enqueue_integrator = [&](int j) {
		if (pipe) h->L = &h->lane[1];
		integrator(h, plan[j].nb, T, plan[j].emb, 0, csb[j & 1], pipe ? h->side : s, true);
		h->L = &h->lane[0];
		if (pipe) (void)hipEventRecord(h->ev_int[j & 1], h->side);
	};
	if (pipe) enqueue_integrator(0);
	for (int j = 0; j < n_steps; ++j) {
		if (!pipe) enqueue_integrator(j);
		else {
			if (j + 1 < n_steps) {
				if (j >= 1) TTK_HIP(hipStreamWaitEvent(h->side, h->ev_free[(j - 1) & 1], 0));   // body j-1 has read the buffer integrator j+1 writes
				enqueue_integrator(j + 1);
			}
			TTK_HIP(hipStreamWaitEvent(s, h->ev_int[j & 1], 0));
		}
		step_body(h, x, plan[j], csb[j & 1], pipe ? h->ev_free[j & 1] : nullptr, s);
	}
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diff_sample_ddim(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, int n_steps, void* stream) {
	return sample_loop(h, x, E, b, T, steps, n_steps, nullptr, 0, stream, "ttk_diff_sample_ddim");
}

// Several utterances of DIFFERENT length as one batch (no reference counterpart: the reference diffuses one line at a time, inference.py:237-422;
// its network is batch-capable, diffusion.py:1517-1574, and its ramped conditioning-free guidance asserts b = 1 only because it indexes t[0], :391-393).
// Element e occupies a slot of Tp frames of which tlen[e] are real: x [b, in, Tp], E [b, C, Tp], padding frames ignored on input and left
// undefined on output.  Every kernel that looks across frames takes the element's own length -- attention masks keys beyond it and skips
// query blocks beyond it, GroupNorm statistics cover exactly its frames, chunked from its first frame, the k = 3 convolutions read zeros beyond
// its last frame -- and everything else is row-wise, so element e comes out BIT FOR BIT as ttk_diff_sample_ddim(b = 1, T = tlen[e]) gives it,
// while every GEMM of a step runs over the rows of all elements (2 b Tp instead of 2 T: more than one tile per CU).
// (`ms`: the same batch under the multistep update, ttk_diff_sample_ms_lines: the update is element-wise, so the property carries over)
static int sample_lines(ttk_diff* h, float* x, const float* E, int b, int Tp, const int* tlen, const ttk_step* steps, int n_steps, void* stream, const char* who,
						const ttk_step_ms* ms = nullptr) {
	TTK_REQUIRE(h && x && E && tlen && steps, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(b >= 1 && 2 * b <= 64, TTK_E_ARG, "%s: %d elements (1..32)", who, b);
	TTK_REQUIRE(Tp >= 64 && Tp % 64 == 0, TTK_E_ARG, "%s: the slot length %d must be a multiple of 64 frames", who, Tp);
	const int C = h->cfg.model_channels;
	for (int i = 0; i < n_steps; ++i) TTK_REQUIRE(steps[i].cfk >= 0.f, TTK_E_ARG, "%s: step %d has no conditioning-free evaluation (the batch is laid out as [cond | uncond])", who, i);
	int host_len[128], host_need[128], any_need = 0;
	for (int e = 0; e < b; ++e) {
		TTK_REQUIRE(tlen[e] >= 1 && tlen[e] <= Tp, TTK_E_ARG, "%s: element %d has %d frames, slot %d", who, e, tlen[e], Tp);
		// a batch of its own length would take its statistics from the GEMM epilogues iff gemm_fuses_gn_stats says so for that length
		const int nd = !(h->fuse_stats && gemm_fuses_gn_stats(2 * tlen[e], C, C, tlen[e]));
		host_len[e] = host_len[b + e] = tlen[e];
		host_need[e] = host_need[b + e] = nd;
		any_need |= nd;
	}
	hipStream_t s = (hipStream_t)stream;
	TTK_HIP(hipMemcpyAsync(h->d_tlen, host_len, (size_t)2 * b * sizeof(int), hipMemcpyHostToDevice, s));
	TTK_HIP(hipMemcpyAsync(h->d_need, host_need, (size_t)2 * b * sizeof(int), hipMemcpyHostToDevice, s));
	TTK_HIP(hipStreamSynchronize(s));      // the staging arrays live on this stack frame
	h->tlen = h->d_tlen;
	h->need = any_need ? h->d_need : nullptr;
	const int rc = sample_loop(h, x, E, b, Tp, steps, n_steps, nullptr, 0, stream, who, nullptr, ms);
	h->tlen = nullptr; h->need = nullptr;
	return rc;
}
int ttk_diff_sample_ddim_lines(ttk_diff* h, float* x, const float* E, int b, int Tp, const int* tlen, const ttk_step* steps, int n_steps, void* stream) {
	return sample_lines(h, x, E, b, Tp, tlen, steps, n_steps, stream, "ttk_diff_sample_ddim_lines");
}

int ttk_diff_sample_p(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, int n_steps, const float* noise, void* stream) {
	return sample_loop(h, x, E, b, T, steps, n_steps, noise, 1, stream, "ttk_diff_sample_p");
}

int ttk_diff_sample_ext(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, const ttk_step_ext* ext, int n_steps, const float* noise, void* stream) {
	TTK_REQUIRE(ext, TTK_E_ARG, "ttk_diff_sample_ext: null argument");
	return sample_loop(h, x, E, b, T, steps, n_steps, noise, 0, stream, "ttk_diff_sample_ext", ext);
}

int ttk_diff_step_ext(ttk_diff* h, float* x, const ttk_step* st, const ttk_step_ext* ext, const float* noise, float* pred_xstart, void* stream) {
	TTK_REQUIRE(h && x && st && ext, TTK_E_ARG, "ttk_diff_step_ext: null argument");
	TTK_REQUIRE(h->staged, TTK_E_STATE, "ttk_diff_step_ext: call ttk_diff_begin first");
	TTK_TRY(check_ext("ttk_diff_step_ext", *ext, 0));
	TTK_REQUIRE(noise || !ext_reads_noise(*st, *ext), TTK_E_ARG, "ttk_diff_step_ext: the step adds noise (mode %d, sigma %g) but noise is null", ext->mode, (double)ext->sigma);
	TTK_REQUIRE(h->cfg.out_channels == 2 * h->cfg.in_channels, TTK_E_ARG, "ttk_diff_step_ext: learned-range output needs out = 2 * in channels");
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(time_path(h, nullptr, &st->t, 1, s));
	StepPlan p = plan_steps(h, st, 1, (const float*)h->emb_all.p, 0, noise, ext)[0];
	p.pred_xstart = pred_xstart;
	integrator(h, p.nb, h->cur_T, p.emb, 0, (float*)h->cs.p, s, true);
	step_body(h, x, p, (const float*)h->cs.p, nullptr, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diffusion_step_ext_rows(const float* out_c, const float* out_u, float* x, const float* noise, float* pred_xstart, int nb, int C, int T, const ttk_step* st,
								const ttk_step_ext* ext, void* xcl, int ldo, int rep, int xcl_dtype, void* stream) {
	TTK_REQUIRE(out_c && x && st && ext, TTK_E_ARG, "ttk_diffusion_step_ext_rows: null argument");
	TTK_REQUIRE(nb >= 1 && C >= 1 && T >= 1, TTK_E_ARG, "ttk_diffusion_step_ext_rows: empty input");
	TTK_TRY(check_ext("ttk_diffusion_step_ext_rows", *ext, 0));
	TTK_REQUIRE(out_u || st->cfk < 0.f, TTK_E_ARG, "ttk_diffusion_step_ext_rows: cfk >= 0 mixes in out_u, which is null");
	TTK_REQUIRE(noise || !ext_reads_noise(*st, *ext), TTK_E_ARG, "ttk_diffusion_step_ext_rows: the step adds noise (mode %d, sigma %g) but noise is null", ext->mode, (double)ext->sigma);
	TTK_REQUIRE(!xcl || (ldo >= C && rep >= 1 && (xcl_dtype == DT_F32 || xcl_dtype == DT_BF16 || xcl_dtype == DT_F16)), TTK_E_ARG,
				"ttk_diffusion_step_ext_rows: the channels-last copy needs ldo >= C, rep >= 1 and an f32 / bf16 / f16 type (ldo %d, rep %d, type %d)", ldo, rep, xcl_dtype);
	launch_diffusion_step_ext(out_c, out_u, x, noise, pred_xstart, nb, C, T, coefs_of(*st), ext_of(*ext), (hipStream_t)stream, xcl, ldo, rep, elem_kind(xcl_dtype));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// ---- DPM-Solver++(2M): the multistep update (k_diffusion_step_ms) behind the same loop machinery.  The argument checks that concern `ms` come first and touch neither
// the handle nor the device.
static int check_ms_loop(const char* who, const ttk_step_ms* ms, int n_steps) {
	TTK_REQUIRE(ms && n_steps >= 1, TTK_E_ARG, "%s: null ms, or no steps", who);
	TTK_REQUIRE(ms[n_steps - 1].c_d1 == 0.f, TTK_E_ARG, "%s: step %d, the first to run, has c_d1 = %g, but there is no history yet", who, n_steps - 1, (double)ms[n_steps - 1].c_d1);
	return TTK_OK;
}

int ttk_diff_sample_ms(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, const ttk_step_ms* ms, int n_steps, void* stream) {
	TTK_TRY(check_ms_loop("ttk_diff_sample_ms", ms, n_steps));
	return sample_loop(h, x, E, b, T, steps, n_steps, nullptr, 0, stream, "ttk_diff_sample_ms", nullptr, ms);
}

int ttk_diff_sample_ms_lines(ttk_diff* h, float* x, const float* E, int b, int Tp, const int* tlen, const ttk_step* steps, const ttk_step_ms* ms, int n_steps, void* stream) {
	TTK_TRY(check_ms_loop("ttk_diff_sample_ms_lines", ms, n_steps));
	return sample_lines(h, x, E, b, Tp, tlen, steps, n_steps, stream, "ttk_diff_sample_ms_lines", ms);
}

int ttk_diff_step_ms(ttk_diff* h, float* x, float* x0_hist, const ttk_step* st, const ttk_step_ms* ms, float* pred_xstart, void* stream) {
	TTK_REQUIRE(ms, TTK_E_ARG, "ttk_diff_step_ms: null ms");
	TTK_REQUIRE(x0_hist || ms->c_d1 == 0.f, TTK_E_ARG, "ttk_diff_step_ms: c_d1 = %g reads the x0 history, which is null", (double)ms->c_d1);
	TTK_REQUIRE(h && x && st, TTK_E_ARG, "ttk_diff_step_ms: null argument");
	TTK_REQUIRE(h->staged, TTK_E_STATE, "ttk_diff_step_ms: call ttk_diff_begin first");
	TTK_REQUIRE(h->cfg.out_channels == 2 * h->cfg.in_channels, TTK_E_ARG, "ttk_diff_step_ms: learned-range output needs out = 2 * in channels");
	hipStream_t s = (hipStream_t)stream;
	TTK_TRY(time_path(h, nullptr, &st->t, 1, s));
	StepPlan p = plan_steps(h, st, 1, (const float*)h->emb_all.p, 0, nullptr, nullptr, false, ms, x0_hist)[0];
	p.pred_xstart = pred_xstart;
	integrator(h, p.nb, h->cur_T, p.emb, 0, (float*)h->cs.p, s, true);
	step_body(h, x, p, (const float*)h->cs.p, nullptr, s);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int ttk_diffusion_step_ms_rows(const float* out_c, const float* out_u, float* x, float* x0_hist, float* pred_xstart, int nb, int C, int T, const ttk_step* st,
							   const ttk_step_ms* ms, void* xcl, int ldo, int rep, int xcl_dtype, void* stream) {
	TTK_REQUIRE(ms, TTK_E_ARG, "ttk_diffusion_step_ms_rows: null ms");
	TTK_REQUIRE(x0_hist || ms->c_d1 == 0.f, TTK_E_ARG, "ttk_diffusion_step_ms_rows: c_d1 = %g reads the x0 history, which is null", (double)ms->c_d1);
	TTK_REQUIRE(out_c && x && st, TTK_E_ARG, "ttk_diffusion_step_ms_rows: null argument");
	TTK_REQUIRE(nb >= 1 && C >= 1 && T >= 1, TTK_E_ARG, "ttk_diffusion_step_ms_rows: empty input");
	TTK_REQUIRE(out_u || st->cfk < 0.f, TTK_E_ARG, "ttk_diffusion_step_ms_rows: cfk >= 0 mixes in out_u, which is null");
	TTK_REQUIRE(!xcl || (ldo >= C && rep >= 1 && (xcl_dtype == DT_F32 || xcl_dtype == DT_BF16 || xcl_dtype == DT_F16)), TTK_E_ARG,
				"ttk_diffusion_step_ms_rows: the channels-last copy needs ldo >= C, rep >= 1 and an f32 / bf16 / f16 type (ldo %d, rep %d, type %d)", ldo, rep, xcl_dtype);
	launch_diffusion_step_ms(out_c, out_u, x, x0_hist, pred_xstart, nb, C, T, coefs_of(*st), ms_of(*ms), (hipStream_t)stream, xcl, ldo, rep, elem_kind(xcl_dtype));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // extern "C"
