// The stages of the fused token steps, one definition each: what k_sample_step<GREEDY> (sample.hip), k_sample_step_ext (sample_ext.hip) and
// k_beam_scores (beam.hip) run on a row held SAMPLE_NPT values per thread in registers -- the processors, the warpers, the draw and the two tails of a
// sampled token.  Every stage is forced inline and works in the LDS words of the calling kernel (sample_prims.h names them), so a kernel body is the
// sequence of its stage calls and nothing of a stage is spelled out twice.
#pragma once
#include "ttk_common.h"
#include "ttk_host.h"
#include "sample_prims.h"

namespace ttk {

struct SampleParams {
	const float* scores; int64_t ld; int V;
	const float* q; int64_t ldq;
	const unsigned char* suppress; float inv_t;
	int top_k; float top_p; float penalty, inv_penalty;          // 0 / >= 1 / 1 = off
	float typical_mass;                                           // TypicalLogitsWarper (unified_voice.py:47-75); 0 / >= 1 = off
	int64_t stop_token;
	int64_t *unfinished, *tok, *ids; int64_t ids_ld, ids_cols; int64_t* col;
	int64_t* history; int64_t hist_ld, hist_off;
	int *live_rows, *all_done;
	// next decode step's input row (AR-aware entry only): x[b] = emb[next] + pos[col + 2]
	const float *emb, *pos; float* x_out; int d, pos_rows;
	void* x_frag; int x_frag_f32;      // optional copy of the same rows in A-fragment order (T-typed; x_frag_f32 = its ttk::ElemKind) for a folded-LayerNorm first launch
};

// sample.hip: the operands every token step takes from the C arguments (1 / temperature, the penalty and its reciprocal included), and the requirements
// its launchers share.  needs_q: the step draws (the greedy form reads none of q, temperature and top_p); max_v_required: the step has no path for
// rows wider than SAMPLE_MAXV, so the width is part of the shape.
SampleParams fill_sample_params(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32);
int check_sample_args(const ttk_sample_args* a, const char* who, bool needs_q, bool max_v_required);

// ---- RepetitionPenaltyLogitsProcessor, first half: the `seen` bitmap (bit t = token t occurs in input_ids) from the n ids id(0) .. id(n - 1)
template <typename Id>
__device__ __forceinline__ void mark_seen(unsigned* seen, int V, int64_t n, int tid, Id id) {
	for (int i = tid; i < SAMPLE_MAXV / 32; i += SAMPLE_THREADS) seen[i] = 0;
	__syncthreads();
	for (int64_t i = tid; i < n; i += SAMPLE_THREADS) {
		const int64_t t = id(i);
		if (t >= 0 && t < V) atomicOr(&seen[t >> 5], 1u << (t & 31));
	}
	__syncthreads();
}

// ---- second half: every id present, once -- a negative score is multiplied by the penalty, another one by its reciprocal (ATen divides a tensor by a
// host scalar as `x * (1 / t)` with the reciprocal rounded to f32, BinaryDivTrueKernel.cu: the `score / penalty` of the processor on the GPU)
__device__ __forceinline__ void penalize_seen(float (&v)[SAMPLE_NPT], int V, const unsigned* seen, float penalty, float inv_penalty, int tid) {
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS;
		if (i < V && ((seen[i >> 5] >> (i & 31)) & 1)) v[j] = v[j] < 0.f ? v[j] * penalty : v[j] * inv_penalty;
	}
}

// ---- SuppressTokensLogitsProcessor; the padding lanes (i >= V) become -inf here as well
__device__ __forceinline__ void suppress_mask(float (&v)[SAMPLE_NPT], int V, const unsigned char* suppress, int tid) {
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS, ic = i < V ? i : V - 1;
		const float t = (suppress && suppress[ic]) ? -INFINITY : v[j];
		v[j] = i < V ? t : -INFINITY;
	}
}

// ---- TypicalLogitsWarper (unified_voice.py:47-75; the reference passes it as a custom processor: after the processors, before the warpers): with
// logp = log_softmax(scores), H = -sum p logp, every token gets the distance |-logp - H|; tokens are taken in ascending distance until their probability
// mass reaches `mass`, the rest becomes -inf.  No sort: the mass descent of top-p, over the order-preserving key of the DISTANCE -- the first key at
// which the running mass reaches mass * total is the threshold, everything at or below it stays.  (The rounding deviation of top_p_cut holds here too.)
__device__ __forceinline__ void typical_warper(float (&v)[SAMPLE_NPT], float mass, int tid, int lane, float* red, unsigned long long* hist64, int* s_bin, unsigned long long* s_before) {
	float m0 = -INFINITY;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) m0 = fmaxf(m0, v[j]);
	m0 = block_max(m0, red, tid);
	float e[SAMPLE_NPT], sum = 0.f;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) { e[j] = expf(v[j] - m0); sum += e[j]; }
	sum = block_sum(sum, red, tid);
	const float lse = m0 + logf(sum);
	float d[SAMPLE_NPT], hpart = 0.f;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const float lp = v[j] - lse, pr = e[j] / sum;
		d[j] = lp;                                        // log p (kept; becomes the distance below)
		if (v[j] != -INFINITY) hpart -= pr * lp;          // nansum: removed tokens contribute (-inf * 0) = nan -> skipped
	}
	const float H = block_sum(hpart, red, tid);
	unsigned long long w[SAMPLE_NPT], tot = 0;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		w[j] = (unsigned long long)((e[j] / sum) * 1099511627776.0f); tot += w[j];
		d[j] = v[j] != -INFINITY ? fabsf(-d[j] - H) : INFINITY;      // |-logp - H|; removed tokens sort last (inf), as abs(inf - H) does
	}
	const unsigned long long total = block_total_u64(tot, tid, hist64);
	// first position (ascending distance) whose cumulative mass is NOT < mass  <=>  running total >= ceil(mass * total)  <=>  > that - 1
	unsigned long long target = (unsigned long long)((double)mass * (double)total);
	if (target >= total && total > 0) target = total - 1;
	if (target > 0) target -= 1;
	__syncthreads();
	const unsigned cut = mass_descent_key(d, w, target, tid, lane, hist64, s_bin, s_before);
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j)
		if (fkey(d[j]) > cut) v[j] = -INFINITY;           // sorted_scores > sorted_scores[last_ind]
}

// ---- TopPLogitsWarper's threshold: the key of the smallest score whose ascending cumulative softmax exceeds 1 - top_p; scores whose key lies below it
// go (the largest score always stays: the target is kept below the total).  m = the row's maximum.  Probability mass is p * 2^40 as 64-bit integers, so
// the sums are exact and independent of the order in which the atomics land: bitwise reproducible.
// Known deviation: HF's TopPLogitsWarper takes the cut from an f32 `cumsum` (a parallel scan) of the sorted f32 probabilities compared with
// 1 - top_p, i.e. from sums that carry f32 rounding; here the masses are exact 2^-40 fixed-point integers.  A row whose ascending cumulative mass at some
// token ties with 1 - top_p within f32 rounding (~1e-6) can therefore keep one token more or less than the torch chain.  Measured
// (tests/test_gpu_parity.py::test_top_p_boundary_stress, 3072 rows x 8 values of top_p): a fraction of a percent of the rows, every one of them such a tie.
// top_p is 1 (off) in TTS.inference's and the CLI's defaults; a caller that needs HF's rounding bit for bit builds the model with hf_exact_top_p=True
// (tortoise_tts_amd/autoregressive.py): the torch warper then runs in front of the sampling kernel.
__device__ __forceinline__ unsigned top_p_cut(const float (&v)[SAMPLE_NPT], float m, float top_p, int tid, int lane, float* red, unsigned long long* hist64, int* s_bin,
												unsigned long long* s_before) {
	float e[SAMPLE_NPT], sum = 0.f;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) { e[j] = expf(v[j] - m); sum += e[j]; }
	sum = block_sum(sum, red, tid);
	unsigned long long w[SAMPLE_NPT], tot = 0;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) { w[j] = (unsigned long long)((e[j] / sum) * 1099511627776.0f); tot += w[j]; }
	const unsigned long long total = block_total_u64(tot, tid, hist64);
	unsigned long long target = (unsigned long long)((1.0f - top_p) * 1099511627776.0f);
	if (total > 0 && target >= total) target = total - 1;
	__syncthreads();
	return mass_descent_key(v, w, target, tid, lane, hist64, s_bin, s_before);
}

// scores whose key lies below `cut` -> -inf (top-k: `scores < kth`; top-p; mirostat's k)
__device__ __forceinline__ void drop_below(float (&v)[SAMPLE_NPT], unsigned cut) {
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j)
		if (fkey(v[j]) < cut) v[j] = -INFINITY;
}

// ---- softmax, multinomial(1) = argmax(p / q): each thread's best (value, index) of its own entries; v becomes exp(v - m).  q_at(j) is the noise of
// entry j of the thread: the callers differ in when they load it.
template <typename Q>
__device__ __forceinline__ void draw(float (&v)[SAMPLE_NPT], float m, int V, int tid, float* red, float& best, int& besti, Q q_at) {
	float sum = 0.f;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) { v[j] = expf(v[j] - m); sum += v[j]; }      // exp(-inf) = 0 for removed / padding lanes
	sum = block_sum(sum, red, tid);
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS;
		const float r = (v[j] / sum) / q_at(j);
		if (i < V && r > best) { best = r; besti = i; }          // strict: the lowest index wins a tie, as in ATen's argmax
	}
}

// ---- the bookkeeping of one row's token, by one thread: finished-row padding, tok, ids, history, col, unfinished and the stopping flag.  Returns the
// token written; besti comes back clamped.
__device__ __forceinline__ int64_t finish_token(const SampleParams& p, int b, int64_t c0, int& besti) {
	if (besti >= p.V) besti = 0;                     // all-NaN / empty row: ATen returns index 0 as well
	const int64_t live = p.unfinished[b];
	const int64_t nxt = (int64_t)besti * live + p.stop_token * (1 - live);
	p.tok[b] = nxt;
	if (c0 < p.ids_cols) p.ids[(int64_t)b * p.ids_ld + c0] = nxt;
	if (p.history) p.history[(int64_t)b * p.hist_ld + p.hist_off + c0] = nxt;
	p.col[b] = c0 + 1;
	const int64_t still = live * (nxt != p.stop_token ? 1 : 0);
	p.unfinished[b] = still;
	// stopping criterion without a host round trip per token: the row that finishes last raises a flag the host can poll (the
	// flag may live in pinned host memory; it changes once within a generation, 0 -> the number of tokens sampled when the last row
	// finished, so a late read is merely late and a reader that runs ahead can still tell WHERE the generation ended)
	if (p.live_rows && live != 0 && still == 0) {
		if (__hip_atomic_fetch_add(p.live_rows, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1 && p.all_done)
			__hip_atomic_store(p.all_done, (int)(c0 + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	return nxt;
}

// ---- the row the following decode step starts from: mel_embedding[next] + mel_pos_embedding[k + 1], k = c0 + 1 tokens generated
// (unified_voice.py:212-214) -- what a separate gather launch did before the first layer.  *s_next: the token finish_token returned, through LDS.
__device__ __forceinline__ void next_input_row(const SampleParams& p, int b, int64_t c0, const long long* s_next, int tid) {
	if (!p.x_out) return;
	__syncthreads();
	const int64_t nxt = *s_next;
	int64_t pi = c0 + 2;
	pi = pi < p.pos_rows ? pi : p.pos_rows - 1;      // guard; the host validates lengths up front
	const float4* e = (const float4*)(p.emb + nxt * p.d);
	const float4* w = (const float4*)(p.pos + pi * p.d);
	float4* o = (float4*)(p.x_out + (int64_t)b * p.d);
	for (int i = tid; i < p.d / 4; i += SAMPLE_THREADS) {
		const float4 a = e[i], c = w[i];
		const float4 v = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
		o[i] = v;
		if (p.x_frag) {   // element (m = b, n = 4i + j) of [m_tile][d/32][lane = (n>>3 & 3) * 16 + (m & 15)][n & 7]: four consecutive n are contiguous
			const int n = 4 * i;
			const int64_t fi = TTK_FRAG_INDEX(b, n, p.d / 32);
			store4_kind(p.x_frag, fi, v, p.x_frag_f32);      // x_frag_f32: ttk::ElemKind of the copy
		}
	}
}

}  // namespace ttk
