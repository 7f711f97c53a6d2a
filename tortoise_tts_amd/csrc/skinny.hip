// Skinny (M <= 64 rows) weight-streaming GEMM for the KV-cached AR decode step -- the HBM-bound half of the path.
//
//   out[M, N] = epilogue( LN?(x)[M, K] * W[N, K]^T + bias )
//
// One workgroup per 16-column n-tile (four per tile, 4 columns each, for the residual projections); its waves split K; every
// wave streams its slice of the weights exactly once, straight from HBM into MFMA B-operand registers (no LDS round trip:
// "GEMV / M <= 16 decode weights" row of cdna_hip_programming.md section 5).  Weights are stored in MFMA-fragment order
// Wp[n_tile][k_step][lane][8] so one wave instruction reads 1 KiB (bf16) of contiguous memory.  The batch rows are the MFMA M
// dimension (16 candidates = one 16x16 tile, MT tiles for bigger shards) and arrive either as f32 rows that the launch
// normalises itself (LayerNorm prologue) or T-typed in A-fragment order (ttk_common.h: TTK_FRAG_INDEX).
//
// This is the generic kernel: any model_dim, any waves per workgroup.  The decode step at the benchmarked geometry runs on the
// compile-time specialisations of gemv.hip, which repeat this kernel's arithmetic operation for operation; k_skinny serves the
// small models, the LayerNorm-prologue form (TTK_AR_LNFOLD=0), the prefill's head, and TTK_AR_LEAN=0 -- the reference
// tests/test_gpu_gemv.py holds k_gemv against.  Forms that measured slower and were removed are listed in DESIGN.md section 5.
//
// Fused prologues/epilogues (one launch per GPT-2 sub-block, reference ops in parentheses):
//   LN1 + c_attn + bias -> q (pre-scaled) / K,V appended to the cache  (HF:models/gpt2/modeling_gpt2.py:144-226,
//        DynamicCache.update)                                                         SK_QKV
//   c_proj + bias + residual add                                                       SK_RESIDUAL
//   LN2 + c_fc + bias + gelu_new  (HF:activations.py:59-66)                            SK_ACT_T
//   ln_f + final_norm + mel_head  (unified_voice.py:106,239)                           SK_STORE_F32, ln_count = 2 (prefill)
//   mel_head over normalised rows (+ multinomial noise, + the cache-length bump)       SK_STORE_F32 (decode)
// Algorithmic bytes per launch: N*K*sizeof(T) weight bytes (+ M*K*4 activations from L2).
#include <hip/hip_ext.h>

#include "ttk_common.h"
#include "ttk_kernels.h"
#include "ttk_rng.h"

namespace ttk {

// Diagnostic builds only (-DTTK_ABL=<bits>, tests/diag/ar_ablate.sh): leave out one part of the kernel to price it in the real decode loop
// (results are then wrong on purpose).  1 LayerNorm statistics + affine, 2 gamma / beta loads, 4 cross-wave reduction, 8 weight loads,
// 16 activation loads, 32 output stores, 64 the whole kernel.  Expands to nothing in the product build.
#ifndef TTK_ABL
#define TTK_ABL 0
#endif

// Diagnostic builds only: -DTTK_STAMPS=2 (tests/diag/ar_chain.cpp) every wave stamps (ttk_common.h); plain -DTTK_STAMPS (tests/diag/skinny_stamps.cpp)
// wave 0 / lane 0 of every workgroup records a 100 MHz timestamp per phase, [workgroup][8].  Expands to nothing in the product build.
#if defined(TTK_STAMPS) && TTK_STAMPS != 2
#define SK_STAMP(i) do { if (p.stamps && threadIdx.x == 0) p.stamps[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SK_STAMPD(i, dep) SK_STAMP(i)
#else
#define SK_STAMP(i) TTK_WSTAMP(p.stamps, blockIdx.x, i)
#define SK_STAMPD(i, dep) TTK_WSTAMPD(p.stamps, blockIdx.x, i, dep)
#endif

// KC = float4 chunks of a row per lane in the LayerNorm prologue (K <= 256 * KC); LN kernels run <= 8 waves (2 per SIMD,
// 256 VGPRs), plain ones up to 16.
// FOLD (plain A operand only): the LayerNorm in front of this matrix folded into it -- see SkinnyParams.g1.  The waves sum x and x^2 of the
// fragments they feed the MFMA (lane = one row x 8 k), the per-wave row partials go through LDS next to the accumulators, and the
// epilogue finishes (acc - mean * csum[n]) * rstd + bias.  No normalised copy of the rows is ever written, no LayerNorm barrier, no
// gamma / beta traffic: the launch is shaped like the plain output projections.
template <typename T, int MT, bool LN, int KC, bool W8, bool FOLD = false>
__global__ __launch_bounds__(LN ? 512 : 1024) void k_skinny(SkinnyParams p) {
	typedef typename Frag<T>::type FragT;
	typedef WFrag<T, W8> WF;
	typedef typename WF::raw WRaw;
	constexpr int ES = sizeof(T);
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
	if (TTK_ABL & 64) return;
	// One workgroup per 16-column n-tile.  The residual projections (N = d: 64 tiles at d = 1024) are "narrow": four workgroups share an n-tile, each
	// owning 4 of its columns over the whole of K -- 4x the workgroups streaming the matrix, no combine between them.  The MFMA still runs
	// 16 columns wide: lane (g, n) fetches the fragment of column 4*sub + (n & 3), so columns 4..15 of the product are copies that the
	// epilogue ignores (matrix throughput is irrelevant here, the weight stream is the work).  The four workgroups of a tile read the
	// same 128-byte lines, so they are given ids that are equal mod 8: round-robin dispatch then puts them on one XCD and its L2
	// fetches every line once (tile counts that are no multiple of 8 keep the plain order).
	const int mode = FOLD ? (p.mode == SK_QKV ? SK_QKV : SK_ACT_T) : p.mode;      // a folded LayerNorm sits in front of c_attn and c_fc only
	const bool narrow = !LN && mode == SK_RESIDUAL;      // (launch_skinny_mt sizes the grid by the same condition)
	int nt = blockIdx.x, sub = 0;
	if (narrow) {
		const int b = blockIdx.x, ntiles = (p.N + 15) / 16;
		if ((ntiles & 7) == 0) { nt = (b >> 5) * 8 + (b & 7); sub = (b >> 3) & 3; }
		else { nt = b >> 2; sub = b & 3; }
	}
	const int KS = p.K / 32;
	const int RS = p.K * ES + 16;                       // padded LDS row stride (bytes), LN mode only
	char* a_lds = smem;
	float* red = (float*)(smem + (LN ? 16 * MT * RS : 0));
	float* rstat = red + nw * MT * 64 * 4;              // FOLD: [wave][m_tile][16 rows][sum, sum of squares]

	// Order of the memory requests matters (vmcnt retires in order): first the activation rows this wave normalises, then
	// its whole first batch of weight fragments, so the HBM latency of the weights hides behind the LayerNorm arithmetic.
	constexpr int RP = 2;                                // rows per LayerNorm pass of a wave
	const int nchunk = p.K / 4;
	float4 v[RP][KC];
	auto ln_load = [&](int r0) {
#pragma unroll
		for (int j = 0; j < RP; ++j) {
			const int r = r0 + j * nw;
			const bool live = r < p.M;
#pragma unroll
			for (int i = 0; i < KC; ++i) {   // unconditional loads (clamped address + select): a branch around a load makes hipcc
				const int c = lane + 64 * i;     // fall back to s_waitcnt vmcnt(0), which would also wait for the weight stream
				const int cc = c < nchunk ? c : nchunk - 1;
				const int rr = live ? r : 0;
				const float4 t = (TTK_ABL & 16) ? make_float4(1.f, 2.f, 3.f, 4.f) : *(const float4*)(p.x + (int64_t)rr * p.ldx + 4 * cc);
				v[j][i] = (live && c < nchunk) ? t : make_float4(0, 0, 0, 0);
			}
		}
	};
	// LayerNorm of RP rows at once: per-lane partial (sum, sum of squares) of every row first, then ONE butterfly in which the
	// 2*RP independent chains interleave (a dependent 6-step cross-lane chain costs ~0.3 us; the first version ran four of them
	// back to back per row and the prologue took 4 us).  Variance = E[x^2] - mean^2 in f32 (K <= 2048, |mean| << rms).
	// gamma/beta of the first LayerNorm are requested together with the rows, BEFORE the weight stream: vmcnt retires in order,
	// so a gamma load issued after the weights would make the normalisation wait for the whole HBM stream.
	float4 g0[KC], b0[KC];
	auto ln_load_affine = [&]() {
#pragma unroll
		for (int i = 0; i < KC; ++i) {
			const int c = lane + 64 * i;
			const int cc = c < nchunk ? c : nchunk - 1;
			const float4 tg = (TTK_ABL & 2) ? make_float4(1.f, 1.f, 1.f, 1.f) : *(const float4*)(p.g1 + 4 * cc), tb = (TTK_ABL & 2) ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)(p.b1 + 4 * cc);
			g0[i] = c < nchunk ? tg : make_float4(0, 0, 0, 0);
			b0[i] = c < nchunk ? tb : make_float4(0, 0, 0, 0);
		}
	};
	auto ln_finish = [&](int r0) {
		for (int pass = 0; pass < ((TTK_ABL & 1) ? 0 : p.ln_count); ++pass) {
			float4 gg[KC], bb[KC];
#pragma unroll
			for (int i = 0; i < KC; ++i) {
				const int c = lane + 64 * i;
				if (pass == 0) { gg[i] = g0[i]; bb[i] = b0[i]; }
				else {
					gg[i] = c < nchunk ? *(const float4*)(p.g2 + 4 * c) : make_float4(0, 0, 0, 0);
					bb[i] = c < nchunk ? *(const float4*)(p.b2 + 4 * c) : make_float4(0, 0, 0, 0);
				}
			}
			float s1[RP], s2[RP];
#pragma unroll
			for (int j = 0; j < RP; ++j) {
				s1[j] = 0.f; s2[j] = 0.f;
#pragma unroll
				for (int i = 0; i < KC; ++i) {
					s1[j] += v[j][i].x + v[j][i].y + v[j][i].z + v[j][i].w;
					s2[j] += v[j][i].x * v[j][i].x + v[j][i].y * v[j][i].y + v[j][i].z * v[j][i].z + v[j][i].w * v[j][i].w;
				}
			}
#pragma unroll
			for (int j = 0; j < RP; ++j) { s1[j] = wave_sum(s1[j]); s2[j] = wave_sum(s2[j]); }   // independent chains: they interleave
#pragma unroll
			for (int j = 0; j < RP; ++j) {
				const float mean = s1[j] / (float)p.K;
				const float var = fmaxf(s2[j] / (float)p.K - mean * mean, 0.f);
				const float rstd = rsqrtf(var + 1e-5f);
#pragma unroll
				for (int i = 0; i < KC; ++i) {   // lanes beyond the row hold zeros and zero gamma/beta: harmless
					v[j][i].x = (v[j][i].x - mean) * rstd * gg[i].x + bb[i].x;
					v[j][i].y = (v[j][i].y - mean) * rstd * gg[i].y + bb[i].y;
					v[j][i].z = (v[j][i].z - mean) * rstd * gg[i].z + bb[i].z;
					v[j][i].w = (v[j][i].w - mean) * rstd * gg[i].w + bb[i].w;
				}
			}
		}
#pragma unroll
		for (int j = 0; j < RP; ++j) {
			const int r = r0 + j * nw;
			if (r >= 16 * MT) continue;
			const bool live = r < p.M;
#pragma unroll
			for (int i = 0; i < KC; ++i) {
				const int c = lane + 64 * i;
				if (c < nchunk) {
					T* dst = (T*)(a_lds + r * RS) + 4 * c;
					dst[0] = cvt<T>(live ? v[j][i].x : 0.f);
					dst[1] = cvt<T>(live ? v[j][i].y : 0.f);
					dst[2] = cvt<T>(live ? v[j][i].z : 0.f);
					dst[3] = cvt<T>(live ? v[j][i].w : 0.f);
				}
			}
		}
	};
	SK_STAMP(0);
	// the cache row the c_attn epilogue appends at: requested now (first in the vmcnt order), not as one more dependent round trip at the end
	int kv_pos = 0;
	if (mode == SK_QKV) kv_pos = *p.d_pos;
	// mel_head launch of a decode step: one thread advances the cache length for the next step.  Every reader of *d_pos (c_attn epilogues, attention) is
	// ahead of this launch on the stream and nothing in it reads the word: one 1-thread launch per token less
	if (mode == SK_STORE_F32 && p.d_pos && blockIdx.x == 0 && threadIdx.x == 0) *(int*)p.d_pos += 1;
	// Epilogue role of the first 256 threads: element (row 4*(l2>>4)+r of each m-tile, column l2&15) of the 16-wide output tile.  Its
	// bias and, for the residual modes, the current value of the output are requested now, ahead of everything else, so the epilogue
	// finds them in registers instead of paying one more dependent L2 round trip after the reduction.
	const int l2 = tid & 63, r = tid >> 6;
	const int n = narrow ? nt * 16 + 4 * sub + (l2 & 3) : nt * 16 + (l2 & 15);
	const bool mine = tid < 256 && (!narrow || (l2 & 15) < 4) && n < p.N;
	float bias = 0.f, fcs = 0.f, res[MT];
	RngArgs rng = {};           // mel head drawing the multinomial noise: generator state and this thread's draw counters
	int64_t draw[MT];
	{
		const int nn = n < p.N ? n : p.N - 1;
		if (p.bias) bias = p.bias[nn];
		if (FOLD) fcs = p.g1[nn];            // column sum of the folded matrix (cold, like the bias: left to the epilogue it is a dependent trip to HBM)
		const bool noise = mode == SK_STORE_F32 && p.noise;
		if (noise) rng = *(const RngArgs*)p.rng;
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) {
			res[mt] = 0.f; draw[mt] = 0;
			int m = mt * 16 + 4 * (l2 >> 4) + (r & 3);
			m = m < p.M ? m : p.M - 1;
			if (mode == SK_RESIDUAL) res[mt] = p.out_f32[(int64_t)m * p.ldc + nn];
			if (noise) draw[mt] = p.draws[m];
		}
	}
	if (LN) { ln_load(wave); ln_load_affine(); }

	// ---- this wave's K slice of the weights; the first PRE fragments are requested now
	const int ks0 = (KS * wave) / nw, ks1 = (KS * (wave + 1)) / nw;
	const WRaw* wp = (const WRaw*)p.Wp + ((int64_t)nt * KS) * 64 + (narrow ? ((lane & ~15) | (4 * sub + (lane & 3))) : lane);
	// Weight fragments requested per batch.  LN mode: 8 x 1 KiB (bf16) per wave.  Plain mode: the A fragments of the same k-steps are requested
	// right beside them (B0 A0 B1 A1 ...), all before the first use -- fetched next to their MFMA instead, every k-step was one more
	// dependent L2 round trip behind a full vmcnt(0) (8 in a row in mlp.c_proj: 4.7 of its 6.9 us) -- so the batch is sized to the register
	// budget of a 1024-thread workgroup (128 VGPRs): <= 64 registers of operands in flight.
	constexpr int OPREGS = (MT + 1) * (ES == 4 ? 8 : 4);                       // A (per m-tile) + B registers of one k-step
	constexpr int PRE = LN ? 8 : (64 / OPREGS >= 8 ? 8 : (64 / OPREGS >= 4 ? 4 : (64 / OPREGS >= 2 ? 2 : 1)));
	WRaw bpre[PRE];
	FragT apre[LN ? 1 : PRE][MT];
	const int npre = min(ks1 - ks0, PRE);
	const int arow = lane & 15, ag = lane >> 4;
	auto load_a_global = [&](int mt, int ks) -> FragT {   // rows in A-fragment order; rows >= M hold zeros
		if (TTK_ABL & 16) return FragT{};
		return *(const FragT*)((const T*)p.a + (((int64_t)mt * KS + ks) * 64 + lane) * 8);
	};
#pragma unroll
	for (int u = 0; u < PRE; ++u) {   // unconditional: slots beyond npre re-read the last fragment (never multiplied)
		const int kk = max(ks0 + (u < npre ? u : npre - 1), 0);
		if (TTK_ABL & 8) bpre[u] = WRaw{}; else bpre[u] = TTK_WLOAD(wp + (int64_t)kk * 64);
		if (!LN) {
#pragma unroll
			for (int mt = 0; mt < MT; ++mt) apre[u][mt] = load_a_global(mt, kk);
		}
	}

	if (LN) {
		ln_finish(wave);
		SK_STAMP(1);
		for (int r0 = wave + RP * nw; r0 < 16 * MT; r0 += RP * nw) { ln_load(r0); ln_finish(r0); }
		__syncthreads();
	}
	SK_STAMP(2);

	f32x4 acc[MT];
#pragma unroll
	for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
	auto load_a_lds = [&](int mt, int ks) -> FragT {
		union { FragT v; uint4 q[ES / 2]; } u;
		const char* src = a_lds + (mt * 16 + arow) * RS + (32 * ks + 8 * ag) * ES;
#pragma unroll
		for (int f = 0; f < ES / 2; ++f) u.q[f] = *(const uint4*)(src + 16 * f);
		return u.v;
	};
	float fs1[MT], fs2[MT];          // FOLD: this lane's sum / sum of squares over the k it multiplies (row lane & 15 of each m-tile)
#pragma unroll
	for (int mt = 0; mt < MT; ++mt) { fs1[mt] = 0.f; fs2[mt] = 0.f; }
	auto mma_step = [&](int mt, const FragT& a, const WRaw& b) {
		if (FOLD) {
#pragma unroll
			for (int j = 0; j < 8; ++j) { const float f = (float)a[j]; fs1[mt] += f; fs2[mt] = fmaf(f, f, fs2[mt]); }
		}
		acc[mt] = mma16<T>(a, WF::dec(b), acc[mt]);
	};
#pragma unroll
	for (int u = 0; u < PRE; ++u)
		if (u < npre) {
#pragma unroll
			for (int mt = 0; mt < MT; ++mt) mma_step(mt, LN ? load_a_lds(mt, ks0 + u) : apre[LN ? 0 : u][mt], bpre[u]);
		}
	constexpr int UN = PRE;
	int ks = ks0 + npre;
	for (; ks + UN <= ks1; ks += UN) {
		WRaw b[UN];
		FragT a[LN ? 1 : UN][MT];
#pragma unroll
		for (int u = 0; u < UN; ++u) {
			if (TTK_ABL & 8) b[u] = WRaw{}; else b[u] = TTK_WLOAD(wp + (int64_t)(ks + u) * 64);
			if (!LN) {
#pragma unroll
				for (int mt = 0; mt < MT; ++mt) a[u][mt] = load_a_global(mt, ks + u);
			}
		}
		__builtin_amdgcn_sched_barrier(0);      // keep the requests in front: sunk next to their MFMAs they become dependent round trips again
#pragma unroll
		for (int u = 0; u < UN; ++u)
#pragma unroll
			for (int mt = 0; mt < MT; ++mt) mma_step(mt, LN ? load_a_lds(mt, ks + u) : a[LN ? 0 : u][mt], b[u]);
	}
	for (; ks < ks1; ++ks) {
		const WRaw b = (TTK_ABL & 8) ? WRaw{} : TTK_WLOAD(wp + (int64_t)ks * 64);
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) mma_step(mt, LN ? load_a_lds(mt, ks) : load_a_global(mt, ks), b);
	}
	if (FOLD) {   // the four lanes of a row (k-groups) -> every one holds the wave's partial; lane group 0 publishes it
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) {
			fs1[mt] = fold16_add(fs1[mt]); fs2[mt] = fold16_add(fs2[mt]);
			fs1[mt] = fold32_add(fs1[mt]); fs2[mt] = fold32_add(fs2[mt]);
			if (lane < 16) *(float2*)(rstat + ((wave * MT + mt) * 16 + lane) * 2) = make_float2(fs1[mt], fs2[mt]);
		}
	}

	SK_STAMPD(3, acc[0][0]);
	// ---- cross-wave reduction through LDS, then epilogue by the first 256 threads
	float vsum[MT];
	if (TTK_ABL & 4) {
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) vsum[mt] = acc[mt][r & 3];
	} else {
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) *(f32x4*)(red + ((wave * MT + mt) * 64 + lane) * 4) = acc[mt];
		__syncthreads();
		SK_STAMP(4);
		if (tid < 256) {
#pragma unroll
			for (int mt = 0; mt < MT; ++mt) {
				float v = 0.f;
				for (int w = 0; w < nw; ++w) v += red[((w * MT + mt) * 64 + l2) * 4 + r];
				vsum[mt] = v;
			}
		}
	}
	float fmean[MT], frstd[MT], fvar[MT], fsq[MT];
	if (FOLD && tid < 256) {
#pragma unroll
		for (int mt = 0; mt < MT; ++mt) {
			float a1 = 0.f, a2 = 0.f;
			for (int w = 0; w < nw; ++w) { const float2 t = *(const float2*)(rstat + ((w * MT + mt) * 16 + 4 * (l2 >> 4) + r) * 2); a1 += t.x; a2 += t.y; }
			const float mean = a1 / (float)p.K;
			fmean[mt] = mean;
			fvar[mt] = fmaxf(a2 / (float)p.K - mean * mean, 0.f);      // E[x^2] - mean^2 in f32, as the LN prologue does
			fsq[mt] = a2;
			frstd[mt] = rsqrtf(fvar[mt] + 1e-5f);
		}
	}
	if (!mine) return;
	if (TTK_ABL & 32) { if (vsum[0] == 1.2345e-30f) p.out_f32[0] = vsum[0]; return; }
#pragma unroll
	for (int mt = 0; mt < MT; ++mt) {
		const int m = mt * 16 + 4 * (l2 >> 4) + r;
		if (m >= p.M) continue;
		const float v = FOLD ? (vsum[mt] - fmean[mt] * fcs) * frstd[mt] + bias : (W8 ? vsum[mt] * p.wscale : vsum[mt]) + bias;
		// what the fold cannot represent well is reported, not hidden: k_gemv's two conditions (one workgroup looks; never taken on a healthy stream)
		if (FOLD && p.health && blockIdx.x == 0 && (l2 & 15) == 0) {
			const int bad = (fmean[mt] * fmean[mt] > 64.f * (fvar[mt] + 1e-5f) ? 1 : 0) | (fsq[mt] - fsq[mt] != 0.f ? 2 : 0);
			if (bad) atomicOr(p.health, bad);
		}
		if (mode == SK_STORE_F32) {
			p.out_f32[(int64_t)m * p.ldc + n] = v;
			// mel head: the multinomial noise of the sampling launch that follows, one value per logit
			if (p.noise) {
				int mrow = m;
				const int grp = (int)rng.group;            // line batch: every line draws the same rows (a handful of subtractions, not a division routine in every instantiation)
				if (grp > 0) while (mrow >= grp) mrow -= grp;
				p.noise[(int64_t)m * p.ldc + n] = torch_exponential_at(rng, draw[mt], (rng.row0 + mrow) * (int64_t)p.N + n);
			}
		} else if (mode == SK_RESIDUAL) {
			p.out_f32[(int64_t)m * p.ldc + n] = res[mt] + v;
			if (p.out_T) ((T*)p.out_T)[TTK_FRAG_INDEX(m, n, p.N / 32)] = cvt<T>(res[mt] + v);
		} else if (mode == SK_ACT_T) {
			((T*)p.out_T)[TTK_FRAG_INDEX(m, n, p.N / 32)] = cvt<T>(apply_act(v, p.act));
		} else {   // SK_QKV
			const int d = p.N / 3;
			const int which = n / d, c = n - which * d;
			if (which == 0) {
				p.qbuf[(int64_t)m * d + c] = v * p.q_scale;
			} else {
				const int h = c >> 6, dd = c & 63;
				T* cache = (T*)(which == 1 ? p.kcache : p.vcache);
				const int pos = kv_pos;
				if (pos < p.max_ctx) cache[(((int64_t)m * p.H + h) * p.max_ctx + pos) * 64 + dd] = cvt<T>(v);   // guard: never write past the cache
			}
		}
	}
	SK_STAMP(5);
#if defined(TTK_STAMPS) && TTK_STAMPS == 2
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // stores acknowledged
	SK_STAMP(6);
#endif
}

// one launch of an instantiation: the LDS it needs is checked against the CU and, past the default limit, granted by the runtime BEFORE the launch
static hipError_t skinny_go(void (*kern)(SkinnyParams), const SkinnyParams& p, int grid, int waves, size_t lds, hipStream_t s, double work) {
	if (lds > CU_LDS_BYTES) return hipErrorInvalidValue;
	if (lds > LDS_DEFAULT_LIMIT) {
		const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e == hipErrorInvalidValue ? hipErrorUnknown : e;      // (hipErrorInvalidValue is kept for "more than a compute unit has")
	}
	// profiling: the event pair travels with the dispatch packet (kernel start / stop timestamps), see prof_pair; taken only now that the launch is certain
	hipEvent_t ea = nullptr, eb = nullptr;
	if (g_prof_on) prof_pair(PROF_SKINNY, work, &ea, &eb);
	hipExtLaunchKernelGGL(kern, dim3(grid), dim3(64 * waves), (unsigned)lds, s, ea, eb, 0, p);
	return hipSuccess;
}

template <typename T, int MT, bool W8>
static hipError_t launch_skinny_mt(int dt, const SkinnyParams& p, int waves, hipStream_t s, double work) {
	const bool fold = p.ln_count == 0 && p.g1 && !W8;
	const int grid = ((p.N + 15) / 16) * (p.mode == SK_RESIDUAL && p.ln_count == 0 && !fold ? 4 : 1);      // the residual projections: four workgroups per n-tile
	waves = skinny_launch_waves(waves, p.ln_count > 0);
	const size_t lds = skinny_lds_bytes(dt, MT, p.K, waves, p.ln_count > 0 ? SKF_PROLOGUE : (fold ? SKF_FOLD : SKF_PLAIN));
	if (p.ln_count > 0) return skinny_go(p.K <= 1024 ? k_skinny<T, MT, true, 4, W8> : k_skinny<T, MT, true, 8, W8>, p, grid, waves, lds, s, work);
	if (fold) return skinny_go(k_skinny<T, MT, false, 1, false, true>, p, grid, waves, lds, s, work);
	return skinny_go(k_skinny<T, MT, false, 1, W8>, p, grid, waves, lds, s, work);
}

template <typename T, bool W8>
static hipError_t launch_skinny_t(int dt, const SkinnyParams& p, int waves, hipStream_t s, double work) {
	const int mt = decode_row_tiles(p.M);
	if (mt == 1) return launch_skinny_mt<T, 1, W8>(dt, p, waves, s, work);
	if (mt == 2) return launch_skinny_mt<T, 2, W8>(dt, p, waves, s, work);
	if (mt == 3) return launch_skinny_mt<T, 3, W8>(dt, p, waves, s, work);
	return launch_skinny_mt<T, 4, W8>(dt, p, waves, s, work);
}

hipError_t launch_skinny(int dt, const SkinnyParams& p_in, int waves, hipStream_t s) {
	SkinnyParams p = p_in;
	if (dt != DT_BF16) p.w8 = 0;                                // fp8 weights exist for the bf16 arithmetic only
	// algorithmic bytes: the weight matrix once + bias + the M activation rows in and out
	const double work = (double)p.N * p.K * (p.w8 ? 1 : dtype_size(dt)) + 4.0 * p.N + 4.0 * p.M * p.K + 4.0 * p.M * p.N;
	if (dt == DT_BF16) return p.w8 ? launch_skinny_t<bf16, true>(dt, p, waves, s, work) : launch_skinny_t<bf16, false>(dt, p, waves, s, work);
	if (dt == DT_F16) return launch_skinny_t<f16, false>(dt, p, waves, s, work);
	return launch_skinny_t<float, false>(dt, p, waves, s, work);
}

}  // namespace ttk
