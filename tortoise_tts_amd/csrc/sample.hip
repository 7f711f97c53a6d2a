// One sampled token per candidate row, fused: the logits processors and warpers of the reference's sample branch, softmax,
// multinomial(1), finished-row padding, bookkeeping and (AR-aware entry) the next decode step's input embedding.
//
// Reference: HF `_sample` as driven by stream_generator.py (processors / warpers :56-101, then HF:generation/utils.py:2894-2937):
//     scores = top_p(top_k(temperature(suppress(repetition_penalty(input_ids, logits)))))
//     probs = softmax(scores);  next = multinomial(probs, 1);  next = next * unfinished + pad * (1 - unfinished);
//     input_ids = cat(input_ids, next);  unfinished &= next != eos
// and the first lines of the following forward (unified_voice.py:212-214): emb = mel_embedding(next) + mel_pos_embedding[k + 1].
// ATen's multinomial for one sample is `argmax(probs / q)` with q ~ Exp(1) drawn by `exponential_` on the caller's generator
// (aten/src/ATen/native/Distributions.cpp).  The noise q stays a torch op in the caller so the Philox stream is the reference's; this
// kernel is everything around it, i.e. the ~15-40 tiny elementwise / sort / reduction launches per token collapsed into one, with no
// host round trip, so the whole token step stays inside one captured HIP graph for every warper combination of the CLI
// (__main__.py:17-21: temperature 0.8, top-k 16, top-p 1, repetition penalty 1).
//
// Selection without sorting.  top-k needs the k-th largest score, top-p the smallest score whose ascending cumulative probability
// exceeds 1 - top_p: both are a 4-pass radix descent over the order-preserving 32-bit key of the float (256-bin histogram in LDS per
// pass; sample_prims.h) -- counts for top-k, exact fixed-point probability mass for top-p.  Everything at or above the threshold VALUE is kept,
// which is what `scores < kth` / the sorted cumulative sum do except inside a group of exactly equal scores that straddles the top-p boundary
// (and up to the rounding deviation written down at top_p_cut).  The stages themselves are in sample_stages.h, shared with sample_ext.hip and beam.hip.
#include "ttk_common.h"
#include "ttk_kernels.h"
#include "ttk_host.h"
#include "ttk_rng.h"
#include "sample_stages.h"

namespace ttk {

static_assert(sizeof(ttk_sample_args) == 168, "ttk_sample_args layout (tortoise_tts_amd/_lib.py: SampleArgs mirrors it)");

// grid = B rows, 1024 threads.  Rows up to 9216 wide (8194 mel codes = 9 per thread) stay in registers from the one trip to memory
// to the argmax; wider rows take the plain three-pass path, which supports suppress + temperature only.
// GREEDY: the greedy form of the same step (HF `_sample` with do_sample=False, HF:generation/utils.py:2925: next_tokens = torch.argmax(next_token_scores,
// dim=-1)): the processors and the typical warper as below, then a block argmax of the processed scores themselves, lowest index on ties, and the same
// bookkeeping.  It reads no q and runs none of temperature / top-k / top-p / softmax; V <= SAMPLE_MAXV only (the host refuses wider rows).
template <bool GREEDY>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_step(SampleParams p) {
	__shared__ float red[SAMPLE_THREADS / 64];
	__shared__ int redi[SAMPLE_THREADS / 64];
	__shared__ unsigned seen[SAMPLE_MAXV / 32];                  // repetition penalty: bit i = token i occurs in input_ids
	__shared__ unsigned hist32[256];
	__shared__ unsigned long long hist64[256];
	__shared__ int s_bin;
	__shared__ unsigned long long s_before;
	__shared__ long long s_next;
	const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
	const int V = p.V;
	const float* s = p.scores + (int64_t)b * p.ld;
	const float* qq = GREEDY ? nullptr : p.q + (int64_t)b * p.ldq;
	// ATen divides a tensor by a host scalar as `x * (1 / t)` with the reciprocal rounded to f32 (BinaryDivTrueKernel.cu), and that
	// is what TemperatureLogitsWarper's `scores / temperature` runs on the GPU.
	const bool scale = p.inv_t != 1.0f;
	const int64_t c0 = p.col[b];
	float best = -INFINITY;
	int besti = 0x7fffffff;
	if (V <= SAMPLE_MAXV) {
		float v[SAMPLE_NPT], qv[SAMPLE_NPT];
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {       // unconditional clamped loads: all 18 requests leave before the first use
			const int i = tid + j * SAMPLE_THREADS, ic = i < V ? i : V - 1;
			v[j] = s[ic];
			if constexpr (!GREEDY) qv[j] = qq[ic];
		}
		// ---- RepetitionPenaltyLogitsProcessor: every id present in input_ids (prefix ids + tokens generated so far), once
		if (p.penalty != 1.0f && p.history) {
			const int64_t* hrow = p.history + (int64_t)b * p.hist_ld;
			mark_seen(seen, V, p.hist_off + c0, tid, [&](int64_t i) { return hrow[i]; });
			penalize_seen(v, V, seen, p.penalty, p.inv_penalty, tid);
		}
		suppress_mask(v, V, p.suppress, tid);
		if (p.typical_mass > 0.f && p.typical_mass < 1.0f) typical_warper(v, p.typical_mass, tid, lane, red, hist64, &s_bin, &s_before);
		if constexpr (GREEDY) {
			// ---- greedy search (HF `_sample` without do_sample: next_tokens = torch.argmax(next_token_scores, dim=-1)): no warpers, no softmax, no noise
#pragma unroll
			for (int j = 0; j < SAMPLE_NPT; ++j) {
				const int i = tid + j * SAMPLE_THREADS;
				if (i < V && v[j] > best) { best = v[j]; besti = i; }      // strict, ascending i: the lowest index wins a tie (the reduction below keeps that rule)
			}
		} else {
			// ---- TemperatureLogitsWarper
			if (scale) {
#pragma unroll
				for (int j = 0; j < SAMPLE_NPT; ++j) v[j] = v[j] * p.inv_t;
			}
			// ---- TopKLogitsWarper: scores < (k-th largest) -> -inf
			if (p.top_k > 0 && p.top_k < V) drop_below(v, kth_largest_key(v, V, (unsigned)p.top_k, tid, lane, hist32, &s_bin, &s_before));
			float m = -INFINITY;
#pragma unroll
			for (int j = 0; j < SAMPLE_NPT; ++j) m = fmaxf(m, v[j]);
			m = block_max(m, red, tid);
			// ---- TopPLogitsWarper: ascending cumulative softmax <= 1 - top_p -> -inf (the largest score always stays)
			if (p.top_p > 0.f && p.top_p < 1.0f) drop_below(v, top_p_cut(v, m, p.top_p, tid, lane, red, hist64, &s_bin, &s_before));
			draw(v, m, V, tid, red, best, besti, [&](int j) { return qv[j]; });
		}
	} else if constexpr (!GREEDY) {
		const unsigned char* suppress = p.suppress;
		const float inv_t = p.inv_t;
		float m = -INFINITY;
		for (int i = tid; i < V; i += SAMPLE_THREADS) { float v = (suppress && suppress[i]) ? -INFINITY : s[i]; v = scale ? v * inv_t : v; m = fmaxf(m, v); }
		m = block_max(m, red, tid);
		float sum = 0.f;
		for (int i = tid; i < V; i += SAMPLE_THREADS) { float v = (suppress && suppress[i]) ? -INFINITY : s[i]; v = scale ? v * inv_t : v; sum += expf(v - m); }
		sum = block_sum(sum, red, tid);
		for (int i = tid; i < V; i += SAMPLE_THREADS) {
			float v = (suppress && suppress[i]) ? -INFINITY : s[i]; v = scale ? v * inv_t : v;
			const float r = (expf(v - m) / sum) / qq[i];
			if (r > best) { best = r; besti = i; }
		}
	}
	block_argmax<false>(best, besti, red, redi, tid);
	if (tid == 0) s_next = finish_token(p, b, c0, besti);
	next_input_row(p, b, c0, &s_next, tid);
}

// The requirements of every token step (sample_stages.h).  The sampling forms read temperature and top_p besides q; the greedy form reads none of the three.
int check_sample_args(const ttk_sample_args* a, const char* who, bool needs_q, bool max_v_required) {
	TTK_REQUIRE(a && a->scores && (a->q || !needs_q) && a->unfinished && a->tok && a->ids && a->col, TTK_E_ARG, "%s: null argument", who);
	const bool shape = a->B >= 1 && a->V >= 1 && a->ld >= a->V && (a->ldq >= a->V || !needs_q);
	if (max_v_required)
		TTK_REQUIRE(shape && a->V <= SAMPLE_MAXV, TTK_E_ARG, "%s: bad shape (B %d, V %d; a row of at most %d is held in registers)", who, a->B, a->V, SAMPLE_MAXV);
	else
		TTK_REQUIRE(shape, TTK_E_ARG, "%s: bad shape (B %d, V %d)", who, a->B, a->V);
	if (needs_q) {
		TTK_REQUIRE(a->temperature > 0.f, TTK_E_ARG, "%s: temperature must be positive", who);
		TTK_REQUIRE(a->typical_mass >= 0.f, TTK_E_ARG, "%s: negative typical_mass", who);
		TTK_REQUIRE(a->top_p >= 0.f && a->repetition_penalty >= 0.f, TTK_E_ARG, "%s: negative top_p / repetition_penalty", who);
	} else
		TTK_REQUIRE(a->typical_mass >= 0.f && a->repetition_penalty >= 0.f, TTK_E_ARG, "%s: negative typical_mass / repetition_penalty", who);
	TTK_REQUIRE(!(a->repetition_penalty > 0.f && a->repetition_penalty != 1.0f) || a->history, TTK_E_ARG, "%s: the repetition penalty needs the history buffer", who);
	return TTK_OK;
}

SampleParams fill_sample_params(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32) {
	SampleParams p = {};
	p.scores = a->scores; p.ld = a->ld; p.V = a->V; p.q = a->q; p.ldq = a->ldq; p.suppress = a->suppress; p.inv_t = 1.0f / a->temperature;
	p.top_k = a->top_k; p.top_p = a->top_p; p.typical_mass = a->typical_mass;
	p.penalty = a->repetition_penalty > 0.f ? a->repetition_penalty : 1.0f; p.inv_penalty = 1.0f / p.penalty;
	p.stop_token = a->stop_token; p.unfinished = a->unfinished; p.tok = a->tok; p.ids = a->ids; p.ids_ld = a->ids_ld; p.ids_cols = a->ids_cols;
	p.col = a->col; p.history = a->history; p.hist_ld = a->hist_ld; p.hist_off = a->hist_off; p.live_rows = a->live_rows; p.all_done = a->all_done;
	p.emb = emb; p.pos = pos; p.x_out = x_out; p.d = d; p.pos_rows = pos_rows; p.x_frag = x_frag; p.x_frag_f32 = x_frag_f32;
	return p;
}

// The greedy form (ttk_greedy_step / ttk_ar_greedy_next): q, ldq, temperature, top_k and top_p of the arguments are neither checked nor handed to the kernel.
int launch_greedy_step(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32, hipStream_t stream, const char* who) {
	TTK_TRY(check_sample_args(a, who, false, true));
	SampleParams p = fill_sample_params(a, emb, pos, x_out, d, pos_rows, x_frag, x_frag_f32);
	p.q = nullptr; p.ldq = 0; p.inv_t = 1.0f; p.top_k = 0; p.top_p = 1.0f;
	hipLaunchKernelGGL(k_sample_step<true>, dim3(a->B), dim3(SAMPLE_THREADS), 0, stream, p);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

int launch_sample_step(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32, hipStream_t stream, const char* who) {
	TTK_TRY(check_sample_args(a, who, true, false));
	const bool warp = a->top_k > 0 || (a->top_p > 0.f && a->top_p < 1.0f) || (a->repetition_penalty > 0.f && a->repetition_penalty != 1.0f) ||
					  (a->typical_mass > 0.f && a->typical_mass < 1.0f);
	TTK_REQUIRE(!warp || a->V <= SAMPLE_MAXV, TTK_E_ARG, "%s: top-k / top-p / typical sampling / repetition penalty need V <= %d (V %d)", who, SAMPLE_MAXV, a->V);
	const SampleParams p = fill_sample_params(a, emb, pos, x_out, d, pos_rows, x_frag, x_frag_f32);
	hipLaunchKernelGGL(k_sample_step<false>, dim3(a->B), dim3(SAMPLE_THREADS), 0, stream, p);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // namespace ttk

extern "C" int ttk_sample_step(const float* scores, int64_t ld, int B, int V, const float* q, int64_t ldq, const unsigned char* suppress, float temperature,
		int64_t stop_token, int64_t* unfinished, int64_t* tok, int64_t* ids, int64_t ids_ld, int64_t ids_cols, int64_t* col, int64_t* history, int64_t hist_ld,
		int64_t hist_off, int* live_rows, int* all_done, void* stream) {
	ttk_sample_args a = {};
	a.scores = scores; a.ld = ld; a.B = B; a.V = V; a.q = q; a.ldq = ldq; a.suppress = suppress; a.temperature = temperature; a.top_k = 0; a.top_p = 1.0f;
	a.repetition_penalty = 1.0f; a.stop_token = stop_token; a.unfinished = unfinished; a.tok = tok; a.ids = ids; a.ids_ld = ids_ld; a.ids_cols = ids_cols;
	a.col = col; a.history = history; a.hist_ld = hist_ld; a.hist_off = hist_off; a.live_rows = live_rows; a.all_done = all_done;
	return ttk::launch_sample_step(&a, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, (hipStream_t)stream, "ttk_sample_step");
}

extern "C" int ttk_sample_step_warped(const ttk_sample_args* a, void* stream) {
	return ttk::launch_sample_step(a, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, (hipStream_t)stream, "ttk_sample_step_warped");
}

extern "C" int ttk_greedy_step(const ttk_sample_args* a, void* stream) {
	return ttk::launch_greedy_step(a, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, (hipStream_t)stream, "ttk_greedy_step");
}

namespace ttk {
__global__ void k_exponential_like_torch(float* out, int64_t numel, RngArgs a, int64_t draw) {
	const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (li < numel) out[li] = torch_exponential_at(a, draw, li);
}
}  // namespace ttk

extern "C" int ttk_exponential_like_torch(float* out, int64_t numel, int64_t seed, int64_t offset0, int64_t threads, int64_t step, int64_t draw, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(out && numel >= 1 && threads >= 1, TTK_E_ARG, "ttk_exponential_like_torch: bad argument");
	RngArgs a = {seed, offset0, threads, step, 0, 0};
	hipLaunchKernelGGL(k_exponential_like_torch, dim3(grid_for(numel)), dim3(256), 0, (hipStream_t)stream, out, numel, a, draw);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

extern "C" int ttk_graph_launch(void* graph_exec, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(graph_exec, TTK_E_ARG, "ttk_graph_launch: null graph");
	TTK_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
	return TTK_OK;
}
