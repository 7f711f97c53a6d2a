// Block-level pieces of the fused sampling launches (sample.hip: one token per candidate; beam.hip: the beam-search step): the 1024-thread
// reductions, the order-preserving float key and one level of the radix descent that stands in for torch.topk / torch.sort in the warpers.
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

}  // namespace ttk
