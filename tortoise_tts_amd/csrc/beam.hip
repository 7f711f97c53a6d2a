// Beam search on the AR decode: the in-place KV-cache reorder and the fused beam step (include/ttk.h: ttk_ar_reorder_cache[_lines], ttk_beam_step[_lines]).
//
// Reference: HF `_beam_search` with do_sample=True (HF:generation/utils.py:3208-3509 and its helpers :2988-3204) -- what the reference's forked
// `generate` runs for `TTS.inference(beam_width > 1)` (inference.py:161,342) -- and `_reorder_cache` (unified_voice.py:257-265).
//
// The step is two launches of num_beams workgroups:
//   k_beam_scores  row b in registers (as in sample.hip, on the stages of sample_stages.h): log_softmax, processors and warpers on the log-probs, + running score; the
//                  accumulated row goes to scratch with its maximum and its sum of exponentials;
//   k_beam_select  softmax over the flat [num_beams * V] from those partials, / q, the row's 2 * num_beams largest (that many rounds of a
//                  block argmax over registers); the workgroup that arrives last merges the num_beams lists and does the bookkeeping of
//                  steps d to g on 2 * num_beams candidates -- a few hundred scalar operations by one thread, then a parallel copy of the
//                  token histories into the other half of the double-buffered sequence store.
// Everything position-dependent (tokens generated, which half is current, the done word) is device state: the pair can be captured.
// Several text lines searched as one decode batch (ttk_beam_step_lines): the same two kernels on n_lines * num_beams workgroups, workgroup x serving line
// x / num_beams with that line's slice of every state array -- the last workgroup OF A LINE to arrive merges that line's lists; lines never read each other's words.
#include "ttk_common.h"
#include "ttk_kernels.h"
#include "ttk_host.h"
#include "sample_stages.h"
#include "beam_book.h"

namespace ttk {

static_assert(sizeof(ttk_beam_args) == 168, "ttk_beam_args layout (tortoise_tts_amd/_lib.py: BeamArgs mirrors it)");

// ------------------------------------------------------------------------------------------------------------------ KV reorder
// grid = 2 (K, V) * layers * heads workgroups of 256 threads = (256 / pieces) cache rows x pieces 16-byte pieces of a 64-element row; a workgroup
// walks the rows [shared, valid) of its (layer, head).  A thread loads its piece from the source slice of every destination, then
// stores: its reads are complete in program order before its first write and no other thread touches those bytes, so no second cache is needed.
struct ReorderParams {
	char *kc, *vc;
	size_t layer_bytes, slice_bytes, head_bytes;      // strides of [layers][max_batch][H][max_ctx][64]
	int layers, H, max_ctx, row_bytes;
	const int* d_pos;                                 // [0] valid cache rows, [1] rows of the shared prefix
	const int64_t* beam_idx; int B;
	int rows_per_line;                                // a source outside its destination's line [g * rows_per_line, (g + 1) * rows_per_line) is out of range (B: one line)
};

// loads of slices I, I + 1, ..., B - 1 on the way down, their stores on the way back: every load of the thread precedes its first store, and each
// piece is a local of its own (an indexed array of B pieces stayed in scratch memory instead of registers)
template <int I, int B>
struct GatherSlices {
	static __device__ __forceinline__ void run(char* row, const int (&src)[B], size_t slice_bytes) {
		const uint4 v = *(const uint4*)(row + (size_t)src[I] * slice_bytes);
		GatherSlices<I + 1, B>::run(row, src, slice_bytes);
		*(uint4*)(row + (size_t)I * slice_bytes) = v;      // (a fixed point gets its own bytes back: no branch per slice)
	}
};
template <int B>
struct GatherSlices<B, B> {
	static __device__ __forceinline__ void run(char*, const int (&)[B], size_t) {}
};

template <int B>
__global__ __launch_bounds__(256) void k_kv_reorder(ReorderParams p) {
	int src[B];
	bool identity = true, bad = false;
	int lo = 0;                                       // first row of destination b's line
#pragma unroll
	for (int b = 0; b < B; ++b) {
		const int64_t s = p.beam_idx[b];
		if (b == lo + p.rows_per_line) lo = b;
		bad |= s < lo || s >= lo + p.rows_per_line;      // (B is a multiple of rows_per_line: inside the line is inside [0, B))
		identity &= s == b;
		src[b] = (int)s;
	}
	if (identity || bad) return;                      // uniform: every thread read the same B words
	int valid = p.d_pos[0], shared = p.d_pos[1];
	valid = valid < p.max_ctx ? valid : p.max_ctx;
	shared = shared > 0 ? shared : 0;
	const int pieces = p.row_bytes >> 4, rows_per_pass = 256 / pieces;
	const int piece = threadIdx.x % pieces, r = threadIdx.x / pieces;
	const int head = blockIdx.x % p.H, layer = (blockIdx.x / p.H) % p.layers, kv = blockIdx.x / (p.H * p.layers);
	char* base = (kv ? p.vc : p.kc) + (size_t)layer * p.layer_bytes + (size_t)head * p.head_bytes + (size_t)piece * 16;
	for (int t = shared + r; t < valid; t += rows_per_pass) {
		char* row = base + (size_t)t * p.row_bytes;
		GatherSlices<0, B>::run(row, src, p.slice_bytes);
	}
}

template <int B>
static void launch_kv_reorder_n(const ReorderParams& p, int n, hipStream_t s) {
	if constexpr (B > 1) {
		if (n < B) { launch_kv_reorder_n<B - 1>(p, n, s); return; }
	}
	hipLaunchKernelGGL(k_kv_reorder<B>, dim3(2 * p.layers * p.H), dim3(256), 0, s, p);
}

int launch_kv_reorder(void* kc, void* vc, int layers, int max_batch, int H, int max_ctx, size_t es, const int* d_pos, const int64_t* beam_idx, int B,
					  int rows_per_line, hipStream_t s, const char* who) {
	TTK_REQUIRE(B >= 1 && B <= BEAM_MAX && B <= max_batch, TTK_E_ARG, "%s: %d rows; the reorder gathers at most %d slices (max_batch %d)", who, B, BEAM_MAX, max_batch);
	TTK_REQUIRE(rows_per_line >= 1 && B % rows_per_line == 0, TTK_E_ARG, "%s: %d rows are not lines of %d", who, B, rows_per_line);
	ReorderParams p = {};
	p.kc = (char*)kc; p.vc = (char*)vc;
	p.row_bytes = (int)(64 * es);
	p.head_bytes = (size_t)max_ctx * p.row_bytes; p.slice_bytes = (size_t)H * p.head_bytes; p.layer_bytes = (size_t)max_batch * p.slice_bytes;
	p.layers = layers; p.H = H; p.max_ctx = max_ctx; p.d_pos = d_pos; p.beam_idx = beam_idx; p.B = B; p.rows_per_line = rows_per_line;
	launch_kv_reorder_n<BEAM_MAX>(p, B, s);      // one instantiation per row count: the gather is B registers wide, fully unrolled
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// ------------------------------------------------------------------------------------------------------------------ beam step
struct BeamParams {
	const float* logits; int64_t ld; int N, V;
	const float* q;
	const unsigned char* suppress; float inv_t;
	int top_k; float top_p; float penalty, inv_penalty;      // top_k 0 / top_p >= 1 / penalty 1 = off
	float length_penalty;
	int64_t stop_token, prefix0, prefix1;
	int max_new;
	int64_t *col, *seqs; float* scores; int* state;
	float* acc; int* work;
	int64_t *tok, *beam_idx; int* all_done;
	int G;                                            // ttk_beam_step_lines: lines in the batch, every array above [G][...]; 0 = ttk_beam_step
};
// The workgroup's line: every per-line pointer of p moved to the slice of line blockIdx.x / N, once, at kernel entry.  Returns the beam blockIdx.x % N and
// leaves the line in *g.  Scalar work on kernel arguments and the workgroup id (a subtraction loop of at most 16 rounds, no division routine): no vector register.
__device__ __forceinline__ int beam_line(BeamParams& p, int* g) {
	const int N = p.N;
	int b = blockIdx.x, line = 0;
	while (b >= N) { b -= N; ++line; }
	const int64_t rows = (int64_t)line * N;
	p.logits += rows * p.ld; p.q += rows * p.V; p.acc += rows * p.V;
	p.col += rows; p.tok += rows; p.beam_idx += rows;
	p.seqs += rows * 4 * p.max_new; p.scores += 2 * rows; p.state += line * (2 * N + 2);
	p.work += line * (4 * N * N + 2 * N + 1);
	*g = line;
	return b;
}
// work: [0, 2N) the rows' {max, sum of exp} as float bits; then N x 2N candidate values (float bits), N x 2N flat indices, the arrival ticket
__device__ __forceinline__ int* work_cand_r(const BeamParams& p) { return p.work + 2 * p.N; }
__device__ __forceinline__ int* work_cand_i(const BeamParams& p) { return p.work + 2 * p.N + 2 * p.N * p.N; }
__device__ __forceinline__ int* work_ticket(const BeamParams& p) { return p.work + 2 * p.N + 4 * p.N * p.N; }
__device__ __forceinline__ int64_t* seq_half(const BeamParams& p, int half, int finished) { return p.seqs + ((int64_t)(half * 2 + finished) * p.N) * p.max_new; }

__global__ __launch_bounds__(SAMPLE_THREADS) void k_beam_scores(BeamParams p) {
	__shared__ float red[SAMPLE_THREADS / 64];
	__shared__ unsigned seen[SAMPLE_MAXV / 32];
	__shared__ unsigned hist32[256];
	__shared__ unsigned long long hist64[256];
	__shared__ int s_bin;
	__shared__ unsigned long long s_before;
	const int N = p.N, V = p.V;
	int g;
	const int b = beam_line(p, &g);                   // from here on p is the line's
	if (p.state[2 * N + 1]) return;                   // the line's search is over (uniform)
	const int tid = threadIdx.x, lane = tid & 63;
	const int64_t c = p.col[0];
	const float* s = p.logits + (int64_t)b * p.ld;
	float v[SAMPLE_NPT];
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS;
		const float x = s[i < V ? i : V - 1];
		v[j] = i < V ? x : -INFINITY;
	}
	// ---- log_softmax: (x - max) - log(sum exp(x - max)), the form of ATen's kernels
	{
		float m = -INFINITY;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) m = fmaxf(m, v[j]);
		m = block_max(m, red, tid);
		float sum = 0.f;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) sum += expf(v[j] - m);
		sum = block_sum(sum, red, tid);
		const float ls = logf(sum);
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) v[j] = (v[j] - m) - ls;
	}
	// ---- RepetitionPenaltyLogitsProcessor over flat_running_sequences[b] = prefix ids + this beam's own tokens (log-probs are <= 0: multiplied)
	if (p.penalty != 1.0f) {
		const int64_t* hrow = seq_half(p, (int)(c & 1), 0) + (int64_t)b * p.max_new;
		mark_seen(seen, V, c + 2, tid, [&](int64_t i) { return i == 0 ? p.prefix0 : (i == 1 ? p.prefix1 : hrow[i - 2]); });
		penalize_seen(v, V, seen, p.penalty, p.inv_penalty, tid);
	}
	// ---- SuppressTokensLogitsProcessor (not the shared suppress_mask: the padding lanes are -inf already, and with it this kernel came out ~90 instructions longer)
	if (p.suppress) {
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {
			const int i = tid + j * SAMPLE_THREADS;
			if (i < V && p.suppress[i]) v[j] = -INFINITY;
		}
	}
	// ---- TemperatureLogitsWarper
	if (p.inv_t != 1.0f) {
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) v[j] = v[j] * p.inv_t;
	}
	// ---- TopKLogitsWarper(top_k = max(top_k, 2)): scores < (k-th largest) -> -inf
	if (p.top_k > 0 && p.top_k < V) drop_below(v, kth_largest_key(v, V, (unsigned)(p.top_k > 2 ? p.top_k : 2), tid, lane, hist32, &s_bin, &s_before));
	// ---- TopPLogitsWarper(min_tokens_to_keep = 2): ascending cumulative softmax <= 1 - top_p -> -inf, the two largest scores always stay
	if (p.top_p > 0.f && p.top_p < 1.0f) {
		float m = -INFINITY;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) m = fmaxf(m, v[j]);
		m = block_max(m, red, tid);
		const unsigned cut = top_p_cut(v, m, p.top_p, tid, lane, red, hist64, &s_bin, &s_before);
		const unsigned second = kth_largest_key(v, V, 2u, tid, lane, hist32, &s_bin, &s_before);
		drop_below(v, cut < second ? cut : second);
	}
	// ---- + running_beam_scores[b]; the row's share of the flat softmax
	const float run = p.scores[b];
	float m = -INFINITY;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS;
		v[j] = v[j] + run;
		if (i < V) p.acc[(int64_t)b * V + i] = v[j];
		m = fmaxf(m, v[j]);
	}
	m = block_max(m, red, tid);
	float sum = 0.f;
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) sum += expf(v[j] - m);
	sum = block_sum(sum, red, tid);
	if (tid == 0) { p.work[2 * b] = __float_as_int(m); p.work[2 * b + 1] = __float_as_int(sum); }
}

__global__ __launch_bounds__(SAMPLE_THREADS) void k_beam_select(BeamParams p) {
	__shared__ float red[SAMPLE_THREADS / 64];
	__shared__ int redi[SAMPLE_THREADS / 64];
	__shared__ int s_last, s_over;
	__shared__ int top_i[BEAM_KEEP_MAX];
	__shared__ BeamBook book;                         // the bookkeeping's small tables (one thread works on them; LDS rather than private: indexing them costs no scratch)
	const int N = p.N, V = p.V, K = 2 * N;
	const int* state0 = p.state;                      // line 0's state: the done words of all lines are read from here when this line ends
	int g;
	const int b = beam_line(p, &g);                   // from here on p is the line's
	if (p.state[2 * N + 1]) return;                   // the line's search is over (uniform; the word is written behind every workgroup's arrival below)
	const int tid = threadIdx.x;
	// ---- softmax over the flat [N * V] from the rows' partials, / q
	float M = -INFINITY;
	for (int i = 0; i < N; ++i) M = fmaxf(M, __int_as_float(p.work[2 * i]));
	float S = 0.f;
	for (int i = 0; i < N; ++i) S += __int_as_float(p.work[2 * i + 1]) * expf(__int_as_float(p.work[2 * i]) - M);
	float r[SAMPLE_NPT];
#pragma unroll
	for (int j = 0; j < SAMPLE_NPT; ++j) {
		const int i = tid + j * SAMPLE_THREADS, ic = i < V ? i : V - 1;
		const float a = p.acc[(int64_t)b * V + ic], qv = p.q[(int64_t)b * V + ic];
		r[j] = i < V ? (expf(a - M) / S) / qv : -1.0f;      // real entries are >= 0
	}
	// ---- the row's K largest, descending, lowest index first among equals
	unsigned removed = 0;
	int* cand_r = work_cand_r(p) + b * K;
	int* cand_i = work_cand_i(p) + b * K;
	for (int it = 0; it < K; ++it) {
		float best = -2.0f;
		int besti = 0x7fffffff;
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {
			const int i = tid + j * SAMPLE_THREADS;
			if (!((removed >> j) & 1) && i < V && r[j] > best) { best = r[j]; besti = i; }
		}
		block_argmax<true>(best, besti, red, redi, tid);
		if (besti < V && (besti & (SAMPLE_THREADS - 1)) == tid) removed |= 1u << (besti / SAMPLE_THREADS);
		if (tid == 0) { cand_r[it] = __float_as_int(best); cand_i[it] = besti < V ? b * V + besti : 0x7fffffff; }
	}
	// ---- arrival: the lists of this workgroup are released, the last one to arrive acquires all of them
	__syncthreads();
	if (tid == 0) {
		__threadfence();
		s_last = atomicAdd(work_ticket(p), 1) == N - 1;
	}
	__syncthreads();
	if (!s_last) return;
	__threadfence();
	float cr = -2.0f;
	int ci = 0x7fffffff;
	if (tid < N * K) {
		cr = __int_as_float(__hip_atomic_load(work_cand_r(p) + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		ci = __hip_atomic_load(work_cand_i(p) + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (ci == 0x7fffffff) cr = -2.0f;
	}
	for (int it = 0; it < K; ++it) {
		float best = cr;
		int besti = ci;
		block_argmax<true>(best, besti, red, redi, tid);
		if (besti == ci) { cr = -2.0f; ci = 0x7fffffff; }      // flat indices are unique: only the owner matches (or nobody is left)
		if (tid == 0) top_i[it] = besti;
	}
	__syncthreads();
	const int64_t c = p.col[0];
	const int half = (int)(c & 1);
	if (tid == 0) {
		for (int j = 0; j < K; ++j) {
			int idx = top_i[j];
			if (idx < 0 || idx >= N * V) idx = 0;                          // (fewer than K real candidates cannot happen: V >= K)
			book.beam[j] = idx / V; book.tok[j] = idx % V;
			book.lp[j] = p.acc[idx];                                       // torch.gather(accumulated_log_probs, topk_indices)
		}
		s_over = beam_bookkeep(book, N, c, p.max_new, p.stop_token, p.length_penalty, p.scores, p.state, p.tok, p.beam_idx);
		if (p.G) {
			// beam_idx is global over the batch: entry g * N + b holds g * N + source beam.  The step that ends the line leaves the stop token and the
			// identity instead: the decode and the reorder go on for the other lines and must find nothing to move or to look up in this line's rows
			for (int n = 0; n < N; ++n) {
				if (s_over) p.tok[n] = p.stop_token;
				p.beam_idx[n] = (int64_t)g * N + (s_over ? n : p.beam_idx[n]);
			}
		}
	}
	__syncthreads();
	// ---- sequences of the next iteration into the other half: running[n] = old running[run_src[n]] + its token; finished[n] likewise or kept
	{
		const int64_t L = p.max_new;
		const int64_t* old_run = seq_half(p, half, 0); const int64_t* old_fin = seq_half(p, half, 1);
		int64_t* nrun = seq_half(p, half ^ 1, 0); int64_t* nfin = seq_half(p, half ^ 1, 1);
		for (int64_t e = tid; e < (int64_t)N * L; e += SAMPLE_THREADS) {
			const int n = (int)(e / L);
			const int64_t pos = e - (int64_t)n * L;
			nrun[e] = pos == c ? (int64_t)book.run_tok[n] : old_run[(int64_t)book.run_src[n] * L + pos];
			const int fsrc = book.fin_src[n];
			nfin[e] = fsrc < 0 ? old_fin[(int64_t)(-1 - fsrc) * L + pos] : (pos == c ? (int64_t)book.fin_tok[n] : old_run[(int64_t)fsrc * L + pos]);
		}
	}
	__syncthreads();
	if (tid == 0) {
		for (int n = 0; n < N; ++n) p.col[n] = c + 1;
		*work_ticket(p) = 0;
		if (s_over) {
			// the batch is over with its last line.  Two lines may end in this launch, in two workgroups: each stores its done word, fences, and only then reads the
			// others' -- of two such store / fence / load sequences at least one sees the other's store, so at least one of them reports the end (both write the same c + 1:
			// the lines of a batch step together).  ttk_beam_step (G = 0) has no other line to read
			__hip_atomic_store(p.state + 2 * N + 1, (int)(c + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__threadfence();
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the store has been acknowledged before the first load is issued, whatever the fence expands to)
			int running = 0;
			for (int l = 0; l < p.G; ++l) running += __hip_atomic_load(state0 + l * (2 * N + 2) + 2 * N + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
			if (!running && p.all_done) __hip_atomic_store(p.all_done, (int)(c + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
		}
	}
}

}  // namespace ttk

// n_lines 0: ttk_beam_step (one line, tok / beam_idx of the ending step as the bookkeeping leaves them)
static int beam_step(const ttk_beam_args* a, int n_lines, void* stream, const char* who) {
	using namespace ttk;
	TTK_REQUIRE(a && a->logits && a->q && a->col && a->seqs && a->scores && a->state && a->acc && a->work && a->tok && a->beam_idx, TTK_E_ARG, "%s: null argument", who);
	TTK_REQUIRE(a->num_beams >= 2 && a->num_beams <= BEAM_MAX, TTK_E_ARG, "%s: num_beams %d outside 2..%d", who, a->num_beams, BEAM_MAX);
	TTK_REQUIRE(a->V >= 2 * a->num_beams && a->V <= SAMPLE_MAXV && a->ld >= a->V, TTK_E_ARG, "%s: V %d outside %d..%d (the row is held in registers), or ld < V", who,
				a->V, 2 * a->num_beams, SAMPLE_MAXV);
	TTK_REQUIRE(a->temperature > 0.f, TTK_E_ARG, "%s: temperature must be positive", who);
	TTK_REQUIRE(a->top_k == 0 || a->top_k >= 2 * a->num_beams, TTK_E_ARG, "%s: top_k %d keeps fewer than the 2 * num_beams = %d continuations a step selects", who,
				a->top_k, 2 * a->num_beams);
	TTK_REQUIRE(a->top_p >= 0.f && a->repetition_penalty >= 0.f, TTK_E_ARG, "%s: negative top_p / repetition_penalty", who);
	TTK_REQUIRE(a->max_new >= 1, TTK_E_ARG, "%s: max_new %d", who, a->max_new);
	const int lines = n_lines ? n_lines : 1;
	TTK_REQUIRE(lines >= 1 && lines * a->num_beams <= BEAM_MAX, TTK_E_ARG, "%s: %d lines x %d beams exceed %d rows", who, n_lines, a->num_beams, BEAM_MAX);
	BeamParams p = {};
	p.logits = a->logits; p.ld = a->ld; p.N = a->num_beams; p.V = a->V; p.q = a->q; p.suppress = a->suppress; p.inv_t = 1.0f / a->temperature;
	p.top_k = a->top_k; p.top_p = a->top_p; p.penalty = a->repetition_penalty > 0.f ? a->repetition_penalty : 1.0f; p.inv_penalty = 1.0f / p.penalty;
	p.length_penalty = a->length_penalty; p.stop_token = a->stop_token; p.prefix0 = a->prefix_ids[0]; p.prefix1 = a->prefix_ids[1]; p.max_new = a->max_new;
	p.col = a->col; p.seqs = a->seqs; p.scores = a->scores; p.state = a->state; p.acc = a->acc; p.work = a->work; p.tok = a->tok; p.beam_idx = a->beam_idx;
	p.all_done = a->all_done; p.G = n_lines;
	hipLaunchKernelGGL(k_beam_scores, dim3(lines * p.N), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, p);
	hipLaunchKernelGGL(k_beam_select, dim3(lines * p.N), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, p);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

extern "C" int ttk_beam_step(const ttk_beam_args* a, void* stream) { return beam_step(a, 0, stream, "ttk_beam_step"); }

extern "C" int ttk_beam_step_lines(const ttk_beam_args* a, int n_lines, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(n_lines >= 1, TTK_E_ARG, "ttk_beam_step_lines: %d lines", n_lines);
	return beam_step(a, n_lines, stream, "ttk_beam_step_lines");
}
