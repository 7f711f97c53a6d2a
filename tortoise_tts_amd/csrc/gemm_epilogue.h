// Dense GEMM (gemm.hip): the epilogues -- the generic one, the role-specialised one and its residual pre-load, the fused GroupNorm statistics.
#pragma once

#include "gemm_prims.h"

namespace ttk {

// Fused GroupNorm32 statistics of a wave's 64-row block (the values just written: the next op on this tensor is always a GroupNorm): NI/2 whole groups of 32
// channels; exact two-pass (mean, then centred squares) in registers, two DPP wave reductions per group, one (count, mean, M2) triple per (batch, group,
// 64-row chunk) for k_gn_apply to merge.  ONE function for the generic and the role epilogues, with the contraction written out (the squares accumulate
// by fma, nothing else is fused): left to the compiler, two instantiations of the same source rounded M2 differently in the last bit -- found by
// tests/diag/role_check.cpp -- and results must not depend on which instantiation a shape happens to select.
template <int MI, int NI>
__device__ __forceinline__ void gn_block_stats(const f32x4 (&acc)[MI][NI], float* part, int b, int group0, int nch, int chunk, int lane) {
#pragma clang fp contract(off)
#pragma unroll
	for (int gq = 0; gq < NI / 2; ++gq) {
		float sum = 0.f;
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int jj = 0; jj < 2; ++jj)
#pragma unroll
				for (int r = 0; r < 4; ++r) sum += acc[i][2 * gq + jj][r];
		const float mean = wave_sum(sum) * (1.0f / 2048.0f);
		float sq = 0.f;
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int jj = 0; jj < 2; ++jj)
#pragma unroll
				for (int r = 0; r < 4; ++r) { const float d = acc[i][2 * gq + jj][r] - mean; sq = __builtin_fmaf(d, d, sq); }
		sq = wave_sum(sq);
		if (lane == 0) {
			float* o = part + (((int64_t)b * 32 + (group0 + gq)) * nch + chunk) * 3;
			o[0] = 2048.0f; o[1] = mean; o[2] = sq;
		}
	}
}

// Accumulator (i, j) register r is row row0 + 16i + 4*(lane>>4) + r, column col0 + 16j + (lane&15).
// MODE 0: T-typed C; 1: f32 C (+ f32 residual, which may alias C); 2: f32 C transposed to [batch][N][rows_per_batch].
// All residual/bias loads are issued before the first store: with C aliasing the residual a load-store-load-store order would
// serialise 64 dependent L2 round trips per lane.  GUARD = tile crosses the M or N edge.
template <typename T, int MODE, bool GUARD, int MI, int NI>
__device__ __forceinline__ void epilogue(const GemmParams& p, f32x4 (&acc)[MI][NI], int row0, int col0, int lane) {
#pragma clang fp contract(off)      // scale, bias and residual stay three rounded operations in every instantiation (the role epilogue writes them the same way)
	const int lr = 4 * (lane >> 4), lc = lane & 15;
	typedef typename OutOf<T>::type OT;
	if (p.out_scale != 0.f) {
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int j = 0; j < NI; ++j) acc[i][j] *= p.out_scale;
	}
	float bj[NI];
#pragma unroll
	for (int j = 0; j < NI; ++j) {
		const int gn = col0 + 16 * j + lc;
		bj[j] = (p.bias && (!GUARD || gn < p.N)) ? p.bias[gn] : 0.f;
	}
	// bias, then the activation under ONE uniform branch (not one per element)
#pragma unroll
	for (int i = 0; i < MI; ++i)
#pragma unroll
		for (int j = 0; j < NI; ++j)
#pragma unroll
			for (int r = 0; r < 4; ++r) acc[i][j][r] += bj[j];
	if (p.act == ACT_GELU_NEW) {
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int j = 0; j < NI; ++j)
#pragma unroll
				for (int r = 0; r < 4; ++r) acc[i][j][r] = gelu_new_f(acc[i][j][r]);
	} else if (p.act == ACT_SILU) {
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int j = 0; j < NI; ++j)
#pragma unroll
				for (int r = 0; r < 4; ++r) acc[i][j][r] = silu_f(acc[i][j][r]);
	}
	// residual loads all issued before the first store: the residual aliases C, so interleaving them serialises load -> store pairs
	float res[MI][4][NI];
	if (MODE == 1 && p.residual) {
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int r = 0; r < 4; ++r)
#pragma unroll
				for (int j = 0; j < NI; ++j) {
					const int gm = row0 + 16 * i + lr + r, gn = col0 + 16 * j + lc;
					res[i][r][j] = (!GUARD || (gm < p.M && gn < p.N)) ? p.residual[(int64_t)gm * p.ldr + gn] : 0.f;
				}
	} else {
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int r = 0; r < 4; ++r)
#pragma unroll
				for (int j = 0; j < NI; ++j) res[i][r][j] = 0.f;
	}
#pragma unroll
	for (int i = 0; i < MI; ++i) {
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int gm = row0 + 16 * i + lr + r;
			int bb = 0, t = 0;
			if (MODE == 2) { bb = gm / p.rows_per_batch; t = gm - bb * p.rows_per_batch; }
#pragma unroll
			for (int j = 0; j < NI; ++j) {
				const int gn = col0 + 16 * j + lc;
				if (GUARD && (gm >= p.M || gn >= p.N)) continue;
				const float v = acc[i][j][r] + res[i][r][j];
				acc[i][j][r] = v;
				if (MODE == 2) ((float*)p.C)[((int64_t)bb * p.N + gn) * p.rows_per_batch + t] = v;
				else if (MODE == 1) ((float*)p.C)[(int64_t)gm * p.ldc + gn] = v;
				else ((OT*)p.C)[(int64_t)gm * p.ldc + gn] = cvt<OT>(v);
			}
		}
	}
	if (MODE == 1 && p.gn_part && MI == 4 && row0 < p.M) {
		const int b = row0 / p.gn_T, chunk = (row0 - b * p.gn_T) / 64, nch = p.gn_T / 64;
		gn_block_stats<MI, NI>(acc, p.gn_part, b, col0 / 32, nch, chunk, lane);
	}
}

// ------------------------------------------------------------------------------------------------ role-specialised form (GemmRole, ttk_kernels.h)
// What the stamps of tests/diag/ddim_chain.cpp showed for the generic kernel inside the DDIM layer chain: 1.16-1.52 us from a wave's first instruction to its
// first DMA request and 1.64-2.44 us of epilogue per launch -- 44 % of the four GEMMs' time outside their k-loops.  The first is ~350 instructions of run-time
// shape arithmetic issued by one wave per SIMD (integer divisions by the m-tile count and by rows_per_batch, 64-bit address products, the segment table);
// a role turns all of it into constants, shifts and three f32-reciprocal divisions, and reads a dozen argument words instead of the segment table.
template <int ROLE> struct GRole { static constexpr bool on = false, RES = false, GN = false, CONV = false; static constexpr int N = 0, NSEG = 1, MODE = 0; };
template <> struct GRole<GR_IN1x1> { static constexpr bool on = true, RES = false, GN = true, CONV = false; static constexpr int N = 1024, NSEG = 1, MODE = 1; };
template <> struct GRole<GR_CONV3_RES> { static constexpr bool on = true, RES = true, GN = true, CONV = true; static constexpr int N = 1024, NSEG = 3, MODE = 1; };
template <> struct GRole<GR_QKV> { static constexpr bool on = true, RES = false, GN = false, CONV = false; static constexpr int N = 3072, NSEG = 1, MODE = 0; };
template <> struct GRole<GR_PROJ_RES> { static constexpr bool on = true, RES = true, GN = true, CONV = false; static constexpr int N = 1024, NSEG = 1, MODE = 1; };
constexpr int GR_K = 1024;      // K = lda = ldw of every role

// floor(x / d) for 0 <= x < 2^23 with inv = 1.0f / d: the f32 product is off by less than one, so one correction step either way makes it exact
__device__ __forceinline__ int div_recip(int x, int d, float inv) {
	int q = (int)((float)x * inv);
	const int r = x - q * d;
	q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
	return q;
}

// The generic epilogue with the role's decisions taken at compile time: bias always, no activation, no scale; ldc = ldr = N; 32-bit element indices
// (M * N < 2^30, checked by the dispatcher).  Same operations on every value in the same order: bit-identical results.
// the residual values of a wave's block, one dword per accumulator register (GUARD: a row beyond M reads the clamped LAST row -- the request must leave, see below --
// and its value is dropped in the epilogue).  The non-PRE load inside epilogue_role differs only in this: there a row beyond M issues no load and reads 0.
template <int ROLE, int MI, int NI, bool GUARD>
__device__ __forceinline__ void load_residual_role(const GemmParams& p, float (&res)[MI][4][NI], int row0, int col0, int lane) {
	constexpr int N = GRole<ROLE>::N;
	const int lr = 4 * (lane >> 4), lc = lane & 15;
#pragma unroll
	for (int i = 0; i < MI; ++i)
#pragma unroll
		for (int r = 0; r < 4; ++r)
#pragma unroll
			for (int j = 0; j < NI; ++j) {
				// GUARD: a row beyond M reads the LAST row instead (its value is dropped in the epilogue).  The request must leave unconditionally: the tail's waits
				// count exactly RESN loads behind the last DMA request, and a wave whose rows all lie beyond M (wm = 1 of the last tile row when M % 128 == 64) would
				// otherwise issue none -- vmcnt(PER_TILE + RESN) then waits for nothing and its barrier passes before the last two k-tiles have landed.
				const int gm = row0 + 16 * i + lr + r;
				const int gr = GUARD ? min(gm, p.M - 1) : gm;
				res[i][r][j] = p.residual[(unsigned)(gr * N + col0 + 16 * j + lc)];
			}
}

// PRE: `res` already holds the residual (requested under the last k-tiles, see the role kernels' tail)
// `bj`: the NI bias values of this lane's columns, requested by the caller in front of the k-loop (round 6: fetched here they were an L2 round trip between the last MFMA and the first store)
template <typename T, int ROLE, bool GUARD, int MI, int NI, bool PRE = false>
__device__ __forceinline__ void epilogue_role(const GemmParams& p, f32x4 (&acc)[MI][NI], float (&res)[MI][4][NI], const float (&bj)[NI], int row0, int col0, int lane) {
#pragma clang fp contract(off)
	typedef GRole<ROLE> R;
	typedef typename OutOf<T>::type OT;
	constexpr int N = R::N;
	const int lr = 4 * (lane >> 4), lc = lane & 15;
	const float os = sizeof(T) == 1 ? p.out_scale : 1.f;      // fp8 operands: the weights' power-of-two tensor scale (16-bit roles have none)
	if constexpr (R::RES && !PRE) {      // all residual loads before the first store: C aliases the residual
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int r = 0; r < 4; ++r)
#pragma unroll
				for (int j = 0; j < NI; ++j) {
					const int gm = row0 + 16 * i + lr + r;
					res[i][r][j] = (!GUARD || gm < p.M) ? p.residual[(unsigned)(gm * N + col0 + 16 * j + lc)] : 0.f;
				}
	}
	if constexpr (R::MODE == 0 && sizeof(OT) == 2 && !R::RES) {
		// 16-bit output (the q / k / v projection): a lane holds four ROWS of one column, so the plain form is 64 two-byte stores per lane (1.6 us of epilogue).  Neighbouring lanes
		// hold neighbouring columns: one DPP swap per row pair gives the even lane both columns of the upper row and the odd lane both of the lower one -- 32 dword stores of the
		// same converted values (round 6).
		const bool odd = lc & 1;
#pragma unroll
		for (int i = 0; i < MI; ++i)
#pragma unroll
			for (int j = 0; j < NI; ++j)
#pragma unroll
				for (int rp = 0; rp < 2; ++rp) {
					float v0 = acc[i][j][2 * rp], v1 = acc[i][j][2 * rp + 1];
					if constexpr (sizeof(T) == 1) { v0 = v0 * os; v1 = v1 * os; }
					v0 = v0 + bj[j]; v1 = v1 + bj[j];
					acc[i][j][2 * rp] = v0; acc[i][j][2 * rp + 1] = v1;
					const float mine = odd ? v1 : v0, give = odd ? v0 : v1;      // the row this lane stores / the row its neighbour stores
					const float got = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(give), 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]: the neighbour's value of MY row
					const uint2 pk = pack4_16<OT>(odd ? got : mine, odd ? mine : got, 0.f, 0.f);      // (column order: even lane's column first)
					const int gm = row0 + 16 * i + lr + 2 * rp + (odd ? 1 : 0);
					if (GUARD && gm >= p.M) continue;
					*(unsigned*)((OT*)p.C + (unsigned)(gm * N + col0 + 16 * j + (lc & ~1))) = pk.x;
				}
	} else {
#pragma unroll
	for (int i = 0; i < MI; ++i)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int gm = row0 + 16 * i + lr + r;
#pragma unroll
			for (int j = 0; j < NI; ++j) {
				float v = acc[i][j][r];
				if constexpr (sizeof(T) == 1) v = v * os;
				v = v + bj[j];
				if constexpr (R::RES) v += (PRE && GUARD && gm >= p.M) ? 0.f : res[i][r][j];      // (PRE: rows beyond M hold the clamped row's value)
				acc[i][j][r] = v;
				if (GUARD && gm >= p.M) continue;
				const unsigned o = (unsigned)(gm * N + col0 + 16 * j + lc);
				if constexpr (R::MODE == 1) ((float*)p.C)[o] = v;
				else ((OT*)p.C)[o] = cvt<OT>(v);
			}
		}
	}
	if constexpr (R::GN) {
		if (MI == 4 && row0 < p.M) {
			const int b = div_recip(row0, p.gn_T, p.inv_gn_T), chunk = (row0 - b * p.gn_T) >> 6, nch = p.gn_T >> 6;
			gn_block_stats<MI, NI>(acc, p.gn_part, b, col0 / 32, nch, chunk, lane);
		}
	}
}

}  // namespace ttk
