// The bookkeeping of one beam-search step on its 2 * num_beams picks: steps d to g of HF `_beam_search` (HF:generation/utils.py:3437-3508) for batch
// size 1, early_stopping False, pad = eos.  One definition for the kernel (beam.hip: one thread of the last workgroup runs it on tables in LDS) and
// for the host (tests/diag/beam_book_check.cpp, driven by tests/test_beam_ref.py against the restated loop), so the scalar logic is checked without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TTK_HD __host__ __device__ __forceinline__
#else
#define TTK_HD inline
#endif

namespace ttk {

constexpr int BEAM_MAX = 16;              // beams: the register budget of the reorder's gather, and 2 * BEAM_MAX^2 candidates <= one per thread
constexpr int BEAM_KEEP_MAX = 2 * BEAM_MAX;

// in: the picks in descending order of softmax / q.  out: where the rows of the next iteration's sequences come from.  The small tables in between
// live here too, so that the caller chooses their memory (LDS in the kernel: indexing private arrays would cost scratch).
struct BeamBook {
	int beam[BEAM_KEEP_MAX]; long long tok[BEAM_KEEP_MAX]; float lp[BEAM_KEEP_MAX];      // in: source beam, token, accumulated log-prob of pick j
	float rl[BEAM_KEEP_MAX], fs[BEAM_KEEP_MAX]; int hit[BEAM_KEEP_MAX];
	float new_run[BEAM_MAX], old_fs[BEAM_MAX], new_fs[BEAM_MAX]; int old_flag[BEAM_MAX], old_len[BEAM_MAX], new_flag[BEAM_MAX], new_len[BEAM_MAX];
	int run_src[BEAM_MAX]; long long run_tok[BEAM_MAX];      // out: running row n = old running row run_src[n] + run_tok[n]
	int fin_src[BEAM_MAX]; long long fin_tok[BEAM_MAX];      // out: finished row n = old finished row -1 - fin_src[n] (< 0), or old running row fin_src[n] + fin_tok[n]
};

// c: tokens generated before this step.  scores = {running [N], finished [N]}; state = {is_sent_finished [N], finished lengths [N], heuristic bit}.
// tok_out / beam_idx_out [N]: the next forward's tokens and HF's beam_idx.  Returns 1 when `_beam_search_has_unfinished_sequences` turns false.
// Exact ties go to the lowest index (torch.topk leaves them unspecified).
TTK_HD int beam_bookkeep(BeamBook& k, int N, int64_t c, int max_new, int64_t stop_token, float length_penalty, float* scores, int* state,
						 int64_t* tok_out, int64_t* beam_idx_out) {
	const int K = 2 * N;
	int* fin_flag = state; int* fin_len = state + N; int* unsat_p = state + 2 * N;
	float* run_score = scores; float* fin_score = scores + N;
	const bool unsat = *unsat_p != 0;
	const bool at_max = c + 1 >= max_new;
	bool all_hit = true;
	// x / (len ** length_penalty) as ATen's GPU kernels divide by a host scalar: x * (1 / f32(s)), s the Python float (double) power
	const float inv_len = 1.0f / (float)pow((double)(c + 1), (double)length_penalty);
	for (int j = 0; j < K; ++j) {
		k.hit[j] = k.tok[j] == stop_token || at_max;                    // d. EosTokenCriteria | MaxLengthCriteria
		all_hit &= k.hit[j] != 0;
		k.rl[j] = k.hit[j] ? k.lp[j] + -1.0e9f : k.lp[j];              // e. topk_log_probs + hits * -1e9
		float sc = k.lp[j] * inv_len;                                  // f. length penalty, then the masks, added in HF's order
		if (!unsat) sc = sc + -1.0e9f;
		if (!(k.hit[j] && j < N)) sc = sc + -1.0e9f;
		k.fs[j] = sc;
	}
	// e. `_get_running_beams_for_next_iteration`: the N best of the K running scores
	{
		unsigned used = 0;
		for (int n = 0; n < N; ++n) {
			int w = -1;
			for (int j = 0; j < K; ++j)
				if (!((used >> j) & 1) && (w < 0 || k.rl[j] > k.rl[w])) w = j;
			used |= 1u << w;
			k.new_run[n] = k.rl[w];
			k.run_src[n] = k.beam[w]; k.run_tok[n] = k.tok[w];
			tok_out[n] = k.tok[w]; beam_idx_out[n] = k.beam[w];          // g. running_beam_indices[..., cur_len - decoder_prompt_len]
		}
	}
	// f. `_update_finished_beams`: the N best of {finished so far, the candidates}
	for (int n = 0; n < N; ++n) { k.old_fs[n] = fin_score[n]; k.old_flag[n] = fin_flag[n]; k.old_len[n] = fin_len[n]; }
	{
		unsigned long long used = 0;
		for (int n = 0; n < N; ++n) {
			int w = -1;
			float wv = 0.f;
			for (int j = 0; j < N + K; ++j) {
				const float x = j < N ? k.old_fs[j] : k.fs[j - N];
				if (!((used >> j) & 1) && (w < 0 || x > wv)) { w = j; wv = x; }
			}
			used |= 1ull << w;
			k.new_fs[n] = wv;
			if (w < N) { k.new_flag[n] = k.old_flag[w]; k.new_len[n] = k.old_len[w]; k.fin_src[n] = -1 - w; k.fin_tok[n] = 0; }
			else { const int j = w - N; k.new_flag[n] = k.hit[j] && j < N; k.new_len[n] = (int)(c + 1); k.fin_src[n] = k.beam[j]; k.fin_tok[n] = k.tok[j]; }
		}
	}
	float worst = INFINITY;
	for (int n = 0; n < N; ++n) worst = fminf(worst, k.new_fs[n]);
	// g. `_check_early_stop_heuristic` (early_stopping False: the length is c + 1): can a running beam still beat the worst finished one?
	const float best_running = k.new_run[0] * inv_len;
	bool improve = false;
	for (int n = 0; n < N; ++n) improve |= best_running > (k.new_flag[n] ? worst : -1.0e9f);
	const bool still = unsat && improve;
	for (int n = 0; n < N; ++n) { run_score[n] = k.new_run[n]; fin_score[n] = k.new_fs[n]; fin_flag[n] = k.new_flag[n]; fin_len[n] = k.new_len[n]; }
	*unsat_p = still;
	return !(still && !all_hit);                                       // `_beam_search_has_unfinished_sequences` says no
}

}  // namespace ttk
