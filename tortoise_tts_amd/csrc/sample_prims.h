// Block-level pieces of the fused sampling launches (sample.hip, sample_ext.hip: one token per candidate; beam.hip: the beam-search step): the 1024-thread
// reductions, the order-preserving float key and the radix descents that stand in for torch.topk / torch.sort in the warpers.  The stages built from
// them are in sample_stages.h.
#pragma once
#include "ttk_common.h"

namespace ttk {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_NPT = 9;          // elements per thread held in registers on the fast path
constexpr int SAMPLE_MAXV = SAMPLE_NPT * SAMPLE_THREADS;

__device__ __forceinline__ float block_max(float v, float* red, int tid) {
	v = wave_max(v);
	__syncthreads();
	if ((tid & 63) == 0) red[tid >> 6] = v;
	__syncthreads();
	float m = red[0];
#pragma unroll
	for (int w = 1; w < SAMPLE_THREADS / 64; ++w) m = fmaxf(m, red[w]);
	return m;
}

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
	v = wave_sum(v);
	__syncthreads();
	if ((tid & 63) == 0) red[tid >> 6] = v;
	__syncthreads();
	float s = 0.f;
#pragma unroll
	for (int w = 0; w < SAMPLE_THREADS / 64; ++w) s += red[w];     // fixed order: the same sum in every thread and every run
	return s;
}

// order-preserving key: a < b  <=>  key(a) < key(b)   (-inf lowest; NaNs sort to the ends and are not expected here).  -0.0 takes +0.0's key:
// the torch chain compares VALUES (`scores < kth`), for which the two zeros are equal; as bit patterns -0.0 would sort below +0.0 and a k-th
// largest score of +0.0 would drop the -0.0 entries torch keeps.
__device__ __forceinline__ unsigned fkey(float f) {
	const unsigned u = __float_as_uint(f + 0.0f);      // -0.0 + 0.0 = +0.0 (round to nearest); every other value unchanged
	return (u >> 31) ? ~u : (u | 0x80000000u);
}

// One level of the radix descent, run by wave 0 over the 256 bins `h` (counts or masses): walking the bins in DESCENDING (top-k) or
// ASCENDING (top-p) order, find the first bin at which the running total reaches past `target` -- descending: total >= target (the
// k-th largest lies in it), ascending: total > target (the first kept element lies in it).  Returns the bin and the total BEFORE it.
template <typename C, bool DESC>
__device__ __forceinline__ void pick_bin(const C* h, C target, int lane, int& bin_out, C& before_out) {
	C g[4], s = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i) { const int b = DESC ? 255 - (4 * lane + i) : 4 * lane + i; g[i] = h[b]; s += g[i]; }
	C incl = s;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const C o = __shfl_up(incl, off);
		if (lane >= off) incl += o;
	}
	const C excl = incl - s;
	const bool hit = DESC ? (incl >= target) : (incl > target);
	const unsigned long long m = __ballot(hit);
	const int first = m ? __ffsll((long long)m) - 1 : 63;        // no lane reaches it (rounding of the total): take the last bin
	int bin = DESC ? 255 - (4 * first + 3) : 4 * first + 3;
	C before = excl + g[0] + g[1] + g[2];
	if (lane == first) {
		C run = excl;
		bool found = false;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const bool here = DESC ? (run + g[i] >= target) : (run + g[i] > target);
			if (!found && (here || i == 3)) { bin = DESC ? 255 - (4 * lane + i) : 4 * lane + i; before = run; found = true; }
			run += g[i];
		}
	}
	bin_out = __shfl(bin, first);
	before_out = __shfl(before, first);
}

// The descents below keep a row of SAMPLE_NPT values per thread in registers and work in the caller's LDS: `hist32` / `hist64` are the 256 bins of a
// pass, `s_bin` / `s_before` the words through which wave 0 hands the chosen bin and the total in front of it to the block.

// key of the k-th largest of the row's V values (k >= 1; TopKLogitsWarper's `torch.topk(scores, k)[0][..., -1]`): 4-pass radix descent over counts
__device__ __forceinline__ unsigned kth_largest_key(const float (&v)[SAMPLE_NPT], int V, unsigned k, int tid, int lane, unsigned* hist32, int* s_bin, unsigned long long* s_before) {
	unsigned prefix = 0, mask = 0, remaining = k;
	for (int pass = 3; pass >= 0; --pass) {
		const int shift = 8 * pass;
		if (tid < 256) hist32[tid] = 0;
		__syncthreads();
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {
			const int i = tid + j * SAMPLE_THREADS;
			const unsigned key = fkey(v[j]);
			if (i < V && (key & mask) == prefix) atomicAdd(&hist32[(key >> shift) & 255], 1u);
		}
		__syncthreads();
		if (tid < 64) {
			int bin; unsigned before;
			pick_bin<unsigned, true>(hist32, remaining, lane, bin, before);
			if (tid == 0) { *s_bin = bin; *s_before = before; }
		}
		__syncthreads();
		prefix |= (unsigned)*s_bin << shift;
		mask |= 0xffu << shift;
		remaining -= (unsigned)*s_before;
	}
	return prefix;
}

// block total of the integer masses `tot` (exact, whatever order the atomics land in); the caller syncs before hist64 is used again
__device__ __forceinline__ unsigned long long block_total_u64(unsigned long long tot, int tid, unsigned long long* hist64) {
	if (tid < 256) hist64[tid] = 0;
	__syncthreads();
	atomicAdd(&hist64[0], tot);
	__syncthreads();
	return hist64[0];
}

// key of x at which the running mass, taken over ascending fkey(x) with the fixed-point weights w (entries of weight 0 do not take part), first passes
// `target`: 4-pass radix descent over masses.  The keys are recomputed in every pass rather than held: nine registers the callers do not have.
__device__ __forceinline__ unsigned mass_descent_key(const float (&x)[SAMPLE_NPT], const unsigned long long (&w)[SAMPLE_NPT], unsigned long long target, int tid, int lane,
													  unsigned long long* hist64, int* s_bin, unsigned long long* s_before) {
	unsigned prefix = 0, mask = 0;
	unsigned long long below = 0;
	for (int pass = 3; pass >= 0; --pass) {
		const int shift = 8 * pass;
		if (tid < 256) hist64[tid] = 0;
		__syncthreads();
#pragma unroll
		for (int j = 0; j < SAMPLE_NPT; ++j) {
			const unsigned k = fkey(x[j]);
			if (w[j] && (k & mask) == prefix) atomicAdd(&hist64[(k >> shift) & 255], w[j]);
		}
		__syncthreads();
		if (tid < 64) {
			int bin; unsigned long long before;
			pick_bin<unsigned long long, false>(hist64, target - below, lane, bin, before);
			if (tid == 0) { *s_bin = bin; *s_before = before; }
		}
		__syncthreads();
		prefix |= (unsigned)*s_bin << shift;
		mask |= 0xffu << shift;
		below += *s_before;
	}
	return prefix;
}

// block argmax of (value, index), the lowest index winning a tie.  EVERY_THREAD: every thread returns the winner; otherwise thread 0 alone does (it holds
// wave 0's pair already and walks the other waves').
template <bool EVERY_THREAD>
__device__ __forceinline__ void block_argmax(float& best, int& besti, float* red, int* redi, int tid) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		const float ov = __shfl_xor(best, off);
		const int oi = __shfl_xor(besti, off);
		if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
	}
	__syncthreads();
	if ((tid & 63) == 0) { red[tid >> 6] = best; redi[tid >> 6] = besti; }
	__syncthreads();
	if (EVERY_THREAD || tid == 0) {
		if (EVERY_THREAD) { best = red[0]; besti = redi[0]; }
#pragma unroll
		for (int w = 1; w < SAMPLE_THREADS / 64; ++w)
			if (red[w] > best || (red[w] == best && redi[w] < besti)) { best = red[w]; besti = redi[w]; }
	}
}

}  // namespace ttk
