// The reference's own samplers (tortoise_tts/samplers.py: reptition_penalize, length_penalize, dynamic_temperature, mirostat_sample) on a second fused
// token step, k_sample_step_ext, beside k_sample_step (sample.hip): the benchmarked token step never launches this kernel.  Same launch shape (one block
// of 1024 threads per row, V <= SAMPLE_MAXV, the row in registers), same operands (a SampleParams inside SampleExtParams), and the same stages wherever
// the chain is HF's: both kernels call the one definition in sample_stages.h.
//
// Chain per row -- "shared" = the stage of sample_stages.h that k_sample_step<false> calls as well; the rest is this file's:
//   1. repetition penalty.  decay == 0: HF's RepetitionPenaltyLogitsProcessor, shared (mark_seen, penalize_seen).  decay != 0: reptition_penalize(factor =
//      penalty, decay, one_time=True) (samplers.py:11-29) INSTEAD: `previous` = history[b, hist_off : hist_off + col[b]] (prompt + sampled tokens, not the
//      two prefix ids); every distinct token of it, with d = 1 + the number of tokens behind its most recent occurrence, gets
//      score *= 1.0f / (float)(penalty * pow(d, decay)) -- a division whatever the sign of the score (unlike HF's), in ATen's reciprocal-multiply form as
//      the shared penalty.  The "latest position" table is 16 bits per token in LDS (the words of the `seen` bitmap of the other form lie in the same array).
//      penalty == 1 is off (the reference returns early).
//   2. stop-length penalty: length_penalize (:35-40) on the stop token, score *= 1.0f / (float)pow(len(previous) + 1, factor); factor 0 = off.
//   3. suppress mask, typical warper: shared (suppress_mask, typical_warper).
//   4. temperature: HF's warper, or with min_temperature >= 0 dynamic_temperature (:78-91, k = 10, centre 0.5) per row: p_max = 1 / sum exp(s - max)
//      (f32 block sums), T_dyn = T - (T - T_min) / (1 + exp(-10 (p_max - 0.5))) in f64, scores *= 1.0f / (float)T_dyn.  It sits where HF's temperature
//      warper sits, in front of top-k: the reference never wired dynamic_temperature into its generate call, so there is no other order to match.
//   5. top-k, top-p: shared (kth_largest_key, top_p_cut, drop_below).
//   6. draw: shared (draw: argmax(softmax / q)), or with mirostat_tau > 0 mirostat v1 (mirostat_sample, :117-158) in front of it, on one f64 `mu` per row
//      (the reference's max_surprise; the caller sets it to 2 tau before the first token): P = softmax(scores); from the 101 largest P, descending,
//      s = sum ln(P_i / P_i+1) ln t_i / sum ln^2 t_i with t_i = (i + 2) / (i + 1), eps = s - 1, k = rint(((eps 2^mu) / (1 - V^-eps))^(1 / s)) + 1 in f64
//      (Python's round is half-to-even, as rint), clamped to [1, V], a non-finite value = V; the k largest scores stay (kth_largest_key: a group of
//      equal scores at the threshold stays whole); token = the shared draw over the kept; mu -= eta (log2(1 / P[token]) - tau).
//      Only the 101 largest VALUES are needed and equal values sort identically: a count-select of the 101st largest score, the at most 100 strictly larger
//      probabilities compacted into LDS and rank-sorted there -- no sort of the row.  Fewer than 101 finite scores (where the reference raises
//      ZeroDivisionError): every survivor stays (k = their number) and mu is still updated.  A finished row's mu may hold anything.
//      Deviation: the reference draws with torch.multinomial over the k sorted entries, whose Philox consumption depends on k and would cost a host round
//      trip per token.  Here q is the same noise row, indexed by token id, that the default draw consumes: the same distribution over the kept tokens, and
//      exactly the noise block per token that k_sample_step consumes, so the caller's generator accounting does not change.
//   7. bookkeeping and the next decode step's input row: shared (block_argmax, finish_token, next_input_row).
// Optional outputs (tests, diagnosis; HF's output_scores in shape): scores_out = the scores behind stage 5 (-inf where removed), temp_out, mirostat_k.
#include "ttk_common.h"
#include "ttk_kernels.h"
#include "ttk_host.h"
#include "sample_stages.h"

namespace ttk {

static_assert(sizeof(ttk_sample_ext) == 64, "ttk_sample_ext layout (tortoise_tts_amd/_lib.py: SampleExt mirrors it)");

constexpr int MIRO_N = 100;              // ratios of compute_k (samplers.py:121): the 101 largest probabilities

struct SampleExtParams {
	SampleParams s;                      // k_sample_step's operands: what the shared stages take
	// the reference's samplers
	float temperature;                   // T of the dynamic temperature
	float decay, stop_len, min_t, tau, eta;
	double* mu; int* miro_k; float* temp_out; float* scores_out; int64_t scores_out_ld;
};

__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_step_ext(SampleExtParams p) {
	__shared__ float red[SAMPLE_THREADS / 64];
	__shared__ int redi[SAMPLE_THREADS / 64];
	__shared__ unsigned last16[SAMPLE_MAXV / 2];                 // decay: 16 bits per token, 1 + its latest position in `previous` (0 = absent); else: the `seen` bitmap
	__shared__ unsigned hist32[256];
	__shared__ unsigned long long hist64[256];
	__shared__ int s_bin;
	__shared__ unsigned long long s_before;
	__shared__ long long s_next;
	__shared__ float miro_p[MIRO_N + 1], miro_raw[MIRO_N];
	__shared__ double miro_num[MIRO_N], miro_den[MIRO_N];
	__shared__ int s_cnt, s_k, s_tok;
	__shared__ float s_pthr, s_ptok;
	const SampleParams& sp = p.s;
	const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
	const int V = sp.V;
	const float* s = sp.scores + (int64_t)b * sp.ld;
	const float* qq = sp.q + (int64_t)b * sp.ldq;
	const bool scale = sp.inv_t != 1.0f;
	const int64_t c0 = sp.col[b];
	float best = -INFINITY;
	int besti = 0x7fffffff;
	unsigned* seen = last16;
	float v[SAMPLE_NPT];
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {       // unconditional clamped loads (the noise row is read at the draw: nine registers fewer across the f64 stages)
		const int i = tid + j * SAMPLE_THREADS, ic = i < V ? i : V - 1;
		v[j] = s[ic];
	}
	if (p.decay == 0.f) {
		// ---- RepetitionPenaltyLogitsProcessor: every id present in input_ids (prefix ids + tokens generated so far), once
		if (sp.penalty != 1.0f && sp.history) {
			const int64_t* hrow = sp.history + (int64_t)b * sp.hist_ld;
			mark_seen(seen, V, sp.hist_off + c0, tid, [&](int64_t i) { return hrow[i]; });
			penalize_seen(v, V, seen, sp.penalty, sp.inv_penalty, tid);
		}
	} else if (sp.penalty != 1.0f && sp.history) {
		// ---- reptition_penalize(one_time=True): the latest position of every token of `previous`, then one division per distinct token
		for (int i = tid; i < SAMPLE_MAXV / 2; i += SAMPLE_THREADS) last16[i] = 0;
		__syncthreads();
		const int64_t* hrow = sp.history + (int64_t)b * sp.hist_ld + sp.hist_off;
		const int n = (int)(c0 < 65534 ? c0 : 65534);            // (16-bit entries; the host refuses id buffers that long)
		for (int i = tid; i < n; i += SAMPLE_THREADS) {
			const int64_t t = hrow[i];
			if (t >= 0 && t < V) {                                    // 16-bit max through a compare-and-swap on the word that holds the entry
				unsigned* w = &last16[t >> 1];
				const int sh = (int)(t & 1) * 16;
				unsigned old = *w;
				while (((old >> sh) & 0xffffu) < (unsigned)(i + 1)) {
					const unsigned nw = (old & ~(0xffffu << sh)) | ((unsigned)(i + 1) << sh);
					const unsigned prev = atomicCAS(w, old, nw);
					if (prev == old) break;
					old = prev;
				}
			}
		}
		__syncthreads();
#pragma unroll 1
		for (int j = 0; j < SAMPLE_NPT; ++j) {                  // (one copy of pow; the row stays in registers through the constant-index select)
			const int i = tid + j * SAMPLE_THREADS;
			const unsigned at = i < V ? (last16[i >> 1] >> ((i & 1) * 16)) & 0xffffu : 0u;
			if (at) {
				const double dist = (double)(n - (int)at + 1);
				const float mul = 1.0f / (float)((double)sp.penalty * pow(dist, (double)p.decay));
#pragma unroll
				for (int jj = 0; jj < SAMPLE_NPT; ++jj)
					if (jj == j) v[jj] = v[jj] * mul;
			}
		}
	}
	// ---- length_penalize on the stop token: its owner thread alone
	if (p.stop_len != 0.f && sp.stop_token >= 0 && sp.stop_token < V && tid == (int)(sp.stop_token % SAMPLE_THREADS)) {
		const int js = (int)(sp.stop_token / SAMPLE_THREADS);
		const float mul = 1.0f / (float)pow((double)(c0 + 1), (double)p.stop_len);
#pragma unroll
		for (int jj = 0; jj < SAMPLE_NPT; ++jj)
			if (jj == js) v[jj] = v[jj] * mul;
	}
	suppress_mask(v, V, sp.suppress, tid);
	if (sp.typical_mass > 0.f && sp.typical_mass < 1.0f) typical_warper(v, sp.typical_mass, tid, lane, red, hist64, &s_bin, &s_before);
	if (p.min_t >= 0.f) {
		// ---- dynamic_temperature: the temperature falls from T to T_min as the row's largest probability rises through 0.5
		float m0 = -INFINITY;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) m0 = fmaxf(m0, v[j]);
		m0 = block_max(m0, red, tid);
		float sum = 0.f;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) sum += expf(v[j] - m0);
		sum = block_sum(sum, red, tid);
		const double pmax = 1.0 / (double)sum, T = (double)p.temperature;
		const float t_dyn = (float)(T - (T - (double)p.min_t) / (1.0 + exp(-10.0 * (pmax - 0.5))));
		const float inv = 1.0f / t_dyn;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) v[j] = v[j] * inv;
		if (p.temp_out && tid == 0) p.temp_out[b] = t_dyn;
	} else {
		// ---- TemperatureLogitsWarper
		if (scale) {
#pragma unroll
			for (int j = 0; j < SAMPLE_NPT; ++j) v[j] = v[j] * sp.inv_t;
		}
		if (p.temp_out && tid == 0) p.temp_out[b] = p.temperature;
	}
	// ---- TopKLogitsWarper: scores < (k-th largest) -> -inf
	if (sp.top_k > 0 && sp.top_k < V) drop_below(v, kth_largest_key(v, V, (unsigned)sp.top_k, tid, lane, hist32, &s_bin, &s_before));
	float m = -INFINITY;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) m = fmaxf(m, v[j]);
	m = block_max(m, red, tid);
	// ---- TopPLogitsWarper: ascending cumulative softmax <= 1 - top_p -> -inf (the largest score always stays)
	if (sp.top_p > 0.f && sp.top_p < 1.0f) drop_below(v, top_p_cut(v, m, sp.top_p, tid, lane, red, hist64, &s_bin, &s_before));
	if (p.scores_out) {
		float* so = p.scores_out + (int64_t)b * p.scores_out_ld;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {
			const int i = tid + j * SAMPLE_THREADS;
			if (i < V) so[i] = v[j];
		}
	}
	float sum0 = 0.f;                                           // mirostat: the softmax denominator of the whole row (prob_original = exp(score - m) / sum0)
	if (p.tau > 0.f) {
		// ---- mirostat v1: k from the slope of the 101 largest probabilities and the row's running surprise budget mu
		int fin = 0;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) { sum0 += expf(v[j] - m); fin += v[j] != -INFINITY ? 1 : 0; }
		sum0 = block_sum(sum0, red, tid);
		const int finite = (int)block_sum((float)fin, red, tid);      // (counts up to 9216: exact in f32)
		if (finite > MIRO_N) {
			const unsigned thr = kth_largest_key(v, V, MIRO_N + 1, tid, lane, hist32, &s_bin, &s_before);
			if (tid == 0) s_cnt = 0;
			__syncthreads();
#pragma unroll
			for (int j = 0; j < SAMPLE_NPT; ++j) {
				const unsigned key = fkey(v[j]);
				if (key >= thr) {
					const float pj = expf(v[j] - m) / sum0;
					if (key > thr) { const int at = atomicAdd(&s_cnt, 1); if (at < MIRO_N) miro_raw[at] = pj; }      // at most 100 scores lie above the 101st largest
					else s_pthr = pj;                                  // equal scores, equal probabilities: every writer stores the same bits
				}
			}
			__syncthreads();
			const int above = s_cnt < MIRO_N ? s_cnt : MIRO_N;
			if (tid <= MIRO_N) {
				if (tid < above) {
					const float x = miro_raw[tid];
					int rank = 0;
					for (int u = 0; u < above; ++u) { const float y = miro_raw[u]; rank += (y > x || (y == x && u < tid)) ? 1 : 0; }
					miro_p[rank] = x;
				} else miro_p[tid] = s_pthr;
			}
			__syncthreads();
			if (tid < MIRO_N) {
				const double bq = (double)miro_p[tid] / (double)miro_p[tid + 1];
				const double lt = log((double)(tid + 2) / (double)(tid + 1));
				miro_num[tid] = log(bq) * lt;
				miro_den[tid] = lt * lt;
			}
			__syncthreads();
			if (tid == 0) {
				double num = 0.0, den = 0.0;
				for (int i = 0; i < MIRO_N; ++i) { num += miro_num[i]; den += miro_den[i]; }      // in the order of the reference's loop
				const double sl = num / den, eps = sl - 1.0;
				// x^y as exp(y ln x): within ~1e-15 relative of libm's pow here, where k is at most V; a negative base gives NaN (Python: a complex number, an error)
				double kk = exp(log((eps * exp2(p.mu[b])) / (1.0 - exp(-eps * log((double)V)))) / sl);
				kk = rint(kk) + 1.0;
				s_k = (kk >= 1.0 && kk <= (double)V) ? (int)kk : (kk < 1.0 ? 1 : V);               // NaN fails all three comparisons: V
			}
			__syncthreads();
			const int keep = s_k;
			__syncthreads();
			// (no instruction: the scores are made opaque here so that the nine radix keys of the descent above are recomputed behind the f64 section
			// instead of being carried across it -- 13 registers, the difference between 125 and a spill at the 128 a 1024-thread block may hold)
#pragma unroll
			for (int j = 0; j < SAMPLE_NPT; ++j) asm volatile("" : "+v"(v[j]));
			if (keep < V) drop_below(v, kth_largest_key(v, V, (unsigned)keep, tid, lane, hist32, &s_bin, &s_before));
			if (p.miro_k && tid == 0) p.miro_k[b] = keep;
		} else if (p.miro_k && tid == 0) p.miro_k[b] = finite;
	}
	draw(v, m, V, tid, red, best, besti, [&](int j) { const int i = tid + j * SAMPLE_THREADS; return qq[i < V ? i : V - 1]; });
	block_argmax<false>(best, besti, red, redi, tid);
	if (tid == 0) {
		s_next = finish_token(sp, b, c0, besti);
		s_tok = besti;
	}
	if (p.tau > 0.f) {
		// ---- mirostat: mu -= eta (surprise of the token drawn - tau), the surprise from the softmax of the WHOLE row (prob_original)
		__syncthreads();
		const int t = s_tok;
		if (tid == t % SAMPLE_THREADS) {
			const int jt = t / SAMPLE_THREADS;
			float x = 0.f;
#pragma unroll
			for (int jj = 0; jj < SAMPLE_NPT; ++jj)
				if (jj == jt) x = v[jj];                           // exp(score - m) of the token drawn: a kept score is the score it was before the cut
			s_ptok = x / sum0;
		}
		__syncthreads();
		if (tid == 0) p.mu[b] -= (double)p.eta * (log2(1.0 / (double)s_ptok) - (double)p.tau);
	}
	next_input_row(sp, b, c0, &s_next, tid);
}

int launch_sample_step_ext(const ttk_sample_args* a, const ttk_sample_ext* x, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32,
						   hipStream_t stream, const char* who) {
	TTK_TRY(check_sample_args(a, who, true, false));
	TTK_REQUIRE(x, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(a->V <= SAMPLE_MAXV, TTK_E_ARG, "%s: V %d exceeds the %d scores a row holds in registers", who, a->V, SAMPLE_MAXV);
	TTK_REQUIRE((x->repetition_penalty_decay == 0.f && x->stop_length_penalty == 0.f) || a->history, TTK_E_ARG,
				"%s: repetition_penalty_decay / stop_length_penalty need the history buffer", who);
	TTK_REQUIRE(x->repetition_penalty_decay == 0.f || a->ids_cols < 65534, TTK_E_ARG, "%s: repetition_penalty_decay keeps 16-bit positions (ids_cols %lld)", who, (long long)a->ids_cols);
	TTK_REQUIRE(!(x->min_temperature > a->temperature), TTK_E_ARG, "%s: min_temperature %g exceeds temperature %g", who, (double)x->min_temperature, (double)a->temperature);
	TTK_REQUIRE(!(x->mirostat_tau < 0.f) && !(x->mirostat_eta < 0.f), TTK_E_ARG, "%s: negative mirostat_tau / mirostat_eta", who);
	TTK_REQUIRE(!(x->mirostat_tau > 0.f) || x->mirostat_mu, TTK_E_ARG, "%s: mirostat needs mirostat_mu, one double per row", who);
	TTK_REQUIRE(!x->scores_out || x->scores_out_ld >= a->V, TTK_E_ARG, "%s: scores_out_ld %lld is below V %d", who, (long long)x->scores_out_ld, a->V);
	SampleExtParams p = {};
	p.s = fill_sample_params(a, emb, pos, x_out, d, pos_rows, x_frag, x_frag_f32);
	p.temperature = a->temperature; p.decay = x->repetition_penalty_decay; p.stop_len = x->stop_length_penalty;
	p.min_t = x->min_temperature >= 0.f ? x->min_temperature : -1.0f;      // (a NaN is off as well)
	p.tau = x->mirostat_tau; p.eta = x->mirostat_eta; p.mu = x->mirostat_mu; p.miro_k = x->mirostat_k; p.temp_out = x->temp_out;
	p.scores_out = x->scores_out; p.scores_out_ld = x->scores_out_ld;
	hipLaunchKernelGGL(k_sample_step_ext, dim3(a->B), dim3(SAMPLE_THREADS), 0, stream, p);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

}  // namespace ttk

extern "C" int ttk_sample_step_ext(const ttk_sample_args* a, const ttk_sample_ext* x, void* stream) {
	return ttk::launch_sample_step_ext(a, x, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, (hipStream_t)stream, "ttk_sample_step_ext");
}
