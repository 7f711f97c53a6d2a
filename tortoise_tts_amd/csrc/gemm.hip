// Dense "NT" GEMM on MFMA for gfx950:  C[M,N] = epi( sum_seg shift(A_seg)[M,K] * W_seg[N,K]^T ).
//
// Serves every GEMM-shaped op of both networks in their channels-last / token-major internal layout:
//   GPT-2 c_attn / c_proj / c_fc / mlp.c_proj (HF Conv1D, HF:pytorch_utils.py:95-120) for prefill + latent pass,
//   mel_head, DiffusionTTS 1x1 convs (qkv, proj_out, in_layers.2, integrating_conv = 2 concatenated segments),
//   k=3 convs (inp_block, latent_conditioner.0, out_layers.3, out.2 = 3 row-shifted segments, zero padded at the
//   edges of each batch element), emb_layers / time_embed linears.   (tortoise_tts/models/diffusion.py:1316-1376,1517-1574)
//
// Tiling: 256 threads = 4 waves (2x2), BMxBN block tile, 128-byte-row LDS tiles (64 bf16 / 32 f32 of K) with XOR-swizzled
// 16-byte chunks, 16x16 MFMA sub-tiles, f32 accumulate.  Operand staging is direct-to-LDS (`global_load_lds_dwordx4`, one
// 1-KiB piece = 8 tile rows per wave instruction) into a 3-stage ring: tile k+3 is requested and tile k+1's fragments are read
// while tile k is multiplied (register ping-pong), a counted `s_waitcnt vmcnt(N)` leaves one tile in flight across the single
// raw `s_barrier` of each k-step
// (cdna_hip_programming.md section 5 "Pipelining across barriers").  The swizzle lives on the per-lane SOURCE address (LDS
// destination of a glds is lane-linear); rows outside M or outside a conv tap's batch element use an out-of-range buffer offset
// (the buffer hardware returns zeros).
// Three forms of the k-loop since round 6: the hand-ordered stream for wave blocks up to 64 x 32 (16-bit operands: `pipe_*` below), the same stream at half-tile granularity for the
// 64 x 64 wave blocks of the 256 x 128 tile, and the compiler-ordered ping-pong (f32, fp8, residual roles at 256 x 128, rings that are not 3 deep).  The k = 3 residual convolution of
// the DDIM loop runs on a shared activation image instead of the ring (conv3_image_tile).  Every k = 3 'same' convolution adds its products tap-inner (see gemm_tile).
// Roofline: by flops these shapes are MFMA-bound (M = b*T ~ 2k rows, N, K in 1k..3k); at one 128 x 64 tile per CU what bounds the k-loop is the L2 -> LDS intake of a CU
// (59 B/clk with four waves) and the chip's L2 bandwidth, 24 KiB per trip either way.
#include <stdlib.h>

#include <type_traits>

#include <hip/hip_ext.h>

#include "gemm_epilogue.h"

namespace ttk {

// ------------------------------------------------------------------------------------------------ k = 3 convolution on a SHARED activation image (round 6)
// The three taps of out_layers.3 multiply the SAME activation rows shifted by -1 / 0 / +1.  The ring kernel stages a 128-row A tile per (tap, k-chunk): 3 x 16 KiB of a
// k-chunk's 72 KiB are the same bytes.  With the hand-ordered loop the k-loop is bound by what a CU takes in from L2 (no-traffic trip 145 ns, with traffic 315: profiles/
// r06_ddim_chain_pipe_ablation.log; fetching A for tap 0 only -- TTK_DIAG_SKIP=16 -- took 2.3 us off a launch), so the bytes are worth removing: here a k-chunk's activation
// rows m0 - 1 .. m0 + BM are staged ONCE as an image of BM + 2 rows (padded to whole 8-row DMA pieces), the taps read their fragments from it at row offsets 0 / 1 / 2 (the
// swizzle is a function of the image row, so each tap has its own lane address), and only the 8 KiB weight tile changes per trip: 40.6 KiB per k-chunk instead of 72.
//   LDS: two image slots (k-chunk parity) + a ring of four weight tiles + a 1-KiB dump for the null pieces = 67 KiB for BM = 128 (two workgroups per CU still fit).
//   Trip t = 3 kc + tap (tap-inner order: see gemm_tile) multiplies tile t from registers, reads tile t + 1's fragments (RPG per MFMA gap), requests weight tile t + 3
//   and, on tap 2, the image of k-chunk kc + 2 into the slot whose last reads ended with the previous trip.  vmcnt retires in order; behind weight tile t + 1 (what the
//   reads of trip t need; the image they need is older) the wave has requested, by tap of t: {image, W} / {W, image} / {W} -> the counted waits B_PC + A_PC, A_PC + B_PC, B_PC.
//   Batch edges: a row whose frame is the first (last) of its batch element must see zeros on tap -1 (+1) although the image holds the neighbouring element's row there
//   (another row's tap 0 needs it) -- those lanes' A fragments are cleared in registers behind the step's lgkmcnt(0), under a wave-uniform branch only waves with such a row take.
template <typename T, int BM, int NWM, int NWN, int ROLE>
__device__ __forceinline__ void conv3_image_tile(const GemmParams& p, const int m0, const int n0, const int wave) {
	typedef GRole<ROLE> R;
	static_assert(R::on && R::CONV && R::RES && sizeof(T) == 2, "the k = 3 residual role on 16-bit operands");
	constexpr int ES = 2, BN = 64, KSTEPS = 2, NW = NWM * NWN;
	constexpr int WM = BM / NWM, WN = BN / NWN, MI = WM / 16, NI = WN / 16;
	static_assert(MI == 4 && NI == 2, "64 x 32 wave blocks");
	constexpr int IMG_ROWS = BM + 8, IMG = IMG_ROWS * 128, NPA = IMG_ROWS / 8;      // image row r = activation row m0 - 1 + r; rows 0 .. BM + 1 are read
	constexpr int A_PC = (NPA + NW - 1) / NW, B_PC = 8 / NW;                         // DMA pieces per wave: per image (the surplus ones are null pieces) / per weight tile
	constexpr int NB = 4, BT = BN * 128, OFF_B = 2 * IMG, OFF_DUMP = OFF_B + NB * BT;
	constexpr int KC = GR_K / 64, NM = KSTEPS * MI * NI, NR = KSTEPS * (MI + NI), RPG = TTK_PIPE_RPG, D0 = TTK_PIPE_D0;
	static_assert(KC % 2 == 0 && (NR + RPG - 1) / RPG <= NM && D0 + B_PC + A_PC <= NM, "reads and DMA pieces must fit the MFMA gaps");
	constexpr unsigned TAPB = (unsigned)(R::N * GR_K * ES);
	constexpr int RESN = MI * 4 * NI;
	constexpr unsigned OOR = 0x80000000u;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane = threadIdx.x & 63, g = lane >> 4, l15 = lane & 15;
#ifdef TTK_STAMPS
	unsigned long long* const stamps_ = p.stamps;
#endif
	const int wm = wave / NWN, wn = wave % NWN;
	const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
	const int Tb = p.rows_per_batch;
	float bias_pre[NI];      // (the oldest requests of the wave: retired by the first counted wait)
#pragma unroll
	for (int j = 0; j < NI; ++j) bias_pre[j] = p.bias[n0 + wn * WN + 16 * j + l15];

	// fragment addresses: tap s reads image row (row in tile) + s; sub-tile i adds 16 rows = 2048 bytes (an immediate), the image slot IMG bytes (an immediate too)
	unsigned fa[3][KSTEPS], fb[KSTEPS];
#pragma unroll
	for (int ks = 0; ks < KSTEPS; ++ks) {
#pragma unroll
		for (int sg = 0; sg < 3; ++sg) {
			const int r = wm * WM + l15 + sg;
			fa[sg][ks] = smem_base + r * 128 + (((4 * ks + g) ^ (r & 7)) << 4);
		}
		const int rowb = wn * WN + l15;
		fb[ks] = smem_base + OFF_B + rowb * 128 + (((4 * ks + g) ^ (rowb & 7)) << 4);
	}
	// staging offsets
	const int prow = lane >> 3, pslot = lane & 7;
	unsigned va[A_PC], vb[B_PC];
#pragma unroll
	for (int i = 0; i < A_PC; ++i) {
		const int q = wave + NW * i, r = 8 * q + prow, gr = m0 - 1 + r;
		const bool ok = q < NPA && r < BM + 2 && gr >= 0 && gr < p.M;
		va[i] = ok ? (unsigned)(gr * (GR_K * ES) + ((pslot ^ (r & 7)) << 4)) : OOR;
	}
#pragma unroll
	for (int i = 0; i < B_PC; ++i) {
		const int row = 8 * (wave + NW * i) + prow;
		vb[i] = (unsigned)((n0 + row) * (GR_K * ES) + ((pslot ^ (row & 7)) << 4));
	}
	const __amdgpu_buffer_rsrc_t srdB = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, 0x7fffffff, 0x00020000);
	const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc((void*)p.seg[0].A, 0, (unsigned)p.M * (unsigned)(GR_K * ES), 0x00020000);
	// batch-edge rows of this lane, one bit per sub-tile i
	int mlo = 0, mhi = 0;
#pragma unroll
	for (int i = 0; i < MI; ++i) {
		const int x = m0 + wm * WM + 16 * i + l15;
		const int t = x - div_recip(x, Tb, p.inv_rpb) * Tb;
		mlo |= (t == 0 ? 1 : 0) << i;
		mhi |= (t == Tb - 1 ? 1 : 0) << i;
	}
	const bool any_lo = __builtin_amdgcn_ballot_w64(mlo != 0) != 0, any_hi = __builtin_amdgcn_ballot_w64(mhi != 0) != 0;

	struct PFrags { u32x4 a[KSTEPS][MI], b[KSTEPS][NI]; };
	f32x4 acc[MI][NI];
#pragma unroll
	for (int i = 0; i < MI; ++i)
#pragma unroll
		for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

	auto issue_image = [&](auto i_, auto slot_, unsigned kc) {
		constexpr int i = decltype(i_)::value, slot = decltype(slot_)::value;
		const int q = wave + NW * i;
		pipe_glds16(va[i], srdA, kc * 128u, q < NPA ? smem_base + slot * IMG + q * 1024 : smem_base + OFF_DUMP);
	};
	auto issue_w = [&](auto i_, unsigned soff, unsigned slot_off) {
		constexpr int i = decltype(i_)::value;
		pipe_glds16(vb[i], srdB, soff, smem_base + OFF_B + slot_off + (wave + NW * i) * 1024);
	};
	// the fragments of one tile: image slot SLOT, tap S, weight ring slot at byte offset wslot
	auto read_one = [&](auto r_, auto slot_, auto s_, PFrags& fr, const unsigned (&rb)[KSTEPS]) {
		constexpr int r = decltype(r_)::value, ks = r / (MI + NI), q = r % (MI + NI), SLOT = decltype(slot_)::value, S = decltype(s_)::value;
		if constexpr (q < MI) pipe_read16<q * 2048 + SLOT * IMG>(fr.a[ks][q], fa[S][ks]);
		else pipe_read16<(q - MI) * 2048>(fr.b[ks][q - MI], rb[ks]);
	};
	auto clear_edges = [&](auto s_, PFrags& fr) {      // behind the lgkmcnt(0) that landed fr
		constexpr int S = decltype(s_)::value;
		if constexpr (S == 0 || S == 2) {
			if (S == 0 ? any_lo : any_hi) {
				const int m = S == 0 ? mlo : mhi;
#pragma unroll
				for (int i = 0; i < MI; ++i) {
					const bool z = (m >> i) & 1;
#pragma unroll
					for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
						for (int e = 0; e < 4; ++e) fr.a[ks][i][e] = z ? 0u : fr.a[ks][i][e];
				}
			}
			TTK_FENCE();
		}
	};
	int tb = 0;      // (trip index) & 3: the weight ring position
	// One trip: MFMAs of `cur`; wait + barrier in front (W loads may stay in flight); reads of the next tile (image slot SLOT_RD, tap S_RD) into `nxt`; weight tile t + 3
	// (tap S_CUR, k-chunk kc_w) and, when IMGI, the image of k-chunk kc_i into slot SLOT_W.
	auto trip = [&](auto w_, auto rd_, auto slot_rd_, auto s_rd_, auto isw_, auto s_cur_, auto isi_, auto slot_w_, const PFrags& cur, PFrags& nxt, unsigned kc_w, unsigned kc_i) {
		constexpr int W = decltype(w_)::value, S_CUR = decltype(s_cur_)::value;
		constexpr bool RD = decltype(rd_)::value, ISW = decltype(isw_)::value, ISI = decltype(isi_)::value;
		constexpr int PER = (ISW ? B_PC : 0) + (ISI ? A_PC : 0);
		const unsigned rd_slot = (unsigned)((tb + 1) & 3) * BT, wr_slot = (unsigned)((tb + 3) & 3) * BT;
		unsigned rb[KSTEPS];
#pragma unroll
		for (int ks = 0; ks < KSTEPS; ++ks) rb[ks] = fb[ks] + rd_slot;
		const unsigned soffW = (unsigned)S_CUR * TAPB + kc_w * 128u;
		if constexpr (RD || PER > 0) { wait_vmcnt<W>(); pipe_barrier(); }
		static_for<0, NM>([&](auto m_) {
			constexpr int m = decltype(m_)::value, ks = m / (MI * NI), i = (m % (MI * NI)) / NI, j = m % NI;
			pipe_mfma<T>(acc[i][j], cur.a[ks][i], cur.b[ks][j]);
			if constexpr (RD) static_for<0, RPG>([&](auto q_) {
				constexpr int r = m * RPG + decltype(q_)::value;
				if constexpr (r < NR) read_one(std::integral_constant<int, r>{}, slot_rd_, s_rd_, nxt, rb);
			});
			if constexpr (PER > 0 && m >= D0 && m - D0 < PER) {
				constexpr int d = m - D0;
				if constexpr (ISW && d < B_PC) issue_w(std::integral_constant<int, d>{}, soffW, wr_slot);
				else issue_image(std::integral_constant<int, d - (ISW ? B_PC : 0)>{}, slot_w_, kc_i);
			}
		});
		if constexpr (RD) { pipe_lgkm0(); clear_edges(s_rd_, nxt); }
		tb = (tb + 1) & 3;
	};
	typedef std::integral_constant<int, 0> I0; typedef std::integral_constant<int, 1> I1; typedef std::integral_constant<int, 2> I2;
	typedef std::true_type Y; typedef std::false_type N;

	PipeScope scope = pipe_begin();
	// prologue, in the steady state's request order: image 0, weight tiles 0 .. 2, image 1
	static_for<0, A_PC>([&](auto i_) { issue_image(i_, I0{}, 0u); });
	static_for<0, 3>([&](auto t_) { static_for<0, B_PC>([&](auto i_) { issue_w(i_, (unsigned)decltype(t_)::value * TAPB, (unsigned)decltype(t_)::value * BT); }); });
	static_for<0, A_PC>([&](auto i_) { issue_image(i_, I1{}, 1u); });
	TTK_WSTAMP(stamps_, blockIdx.x, 1);
	wait_vmcnt<2 * B_PC + A_PC>();      // image 0 and weight tile 0 have landed
	pipe_barrier();
	TTK_WSTAMP(stamps_, blockIdx.x, 2);
	PFrags f0, f1;
	{
		unsigned rb0[KSTEPS];
#pragma unroll
		for (int ks = 0; ks < KSTEPS; ++ks) rb0[ks] = fb[ks];
		static_for<0, NR>([&](auto r_) { read_one(r_, I0{}, I0{}, f0, rb0); });
	}
	pipe_lgkm0();
	clear_edges(I0{}, f0);
	scope.clk = kclock_start();
	typedef std::integral_constant<int, B_PC + A_PC> W01; typedef std::integral_constant<int, B_PC> W2;
	// six trips per round: k-chunks kc (image slot 0) and kc + 1 (slot 1); tile t lives in f[t & 1]
	// arguments of trip: wait count, reads?, image slot / tap of the tile read, weight tile requested?, tap of the current tile (= of the weight tile requested), image requested?, its slot
	const int row0 = m0 + wm * WM, col0 = n0 + wn * WN;
	float res_pre[MI][4][NI];
	for (int kc = 0; kc < KC - 2; kc += 2) {
		trip(W01{}, Y{}, I0{}, I1{}, Y{}, I0{}, N{}, I0{}, f0, f1, (unsigned)kc + 1, 0u);
		trip(W01{}, Y{}, I0{}, I2{}, Y{}, I1{}, N{}, I0{}, f1, f0, (unsigned)kc + 1, 0u);
		trip(W2{}, Y{}, I1{}, I0{}, Y{}, I2{}, Y{}, I0{}, f0, f1, (unsigned)kc + 1, (unsigned)kc + 2);
		trip(W01{}, Y{}, I1{}, I1{}, Y{}, I0{}, N{}, I1{}, f1, f0, (unsigned)kc + 2, 0u);
		trip(W01{}, Y{}, I1{}, I2{}, Y{}, I1{}, N{}, I1{}, f0, f1, (unsigned)kc + 2, 0u);
		trip(W2{}, Y{}, I0{}, I0{}, Y{}, I2{}, Y{}, I1{}, f1, f0, (unsigned)kc + 2, (unsigned)kc + 3);
	}
	{	// the last two k-chunks (KC - 2, KC - 1): no image left to request, weight tiles up to NT - 1 = (KC - 1, tap 2); the residual tile is requested behind the last of them
		constexpr unsigned kc = KC - 2;
		trip(W01{}, Y{}, I0{}, I1{}, Y{}, I0{}, N{}, I0{}, f0, f1, kc + 1, 0u);
		trip(W01{}, Y{}, I0{}, I2{}, Y{}, I1{}, N{}, I0{}, f1, f0, kc + 1, 0u);
		trip(W2{}, Y{}, I1{}, I0{}, Y{}, I2{}, N{}, I0{}, f0, f1, kc + 1, 0u);
		if (m0 + BM <= p.M) load_residual_role<ROLE, MI, NI, false>(p, res_pre, row0, col0, lane);
		else load_residual_role<ROLE, MI, NI, true>(p, res_pre, row0, col0, lane);
		asm volatile("" ::: "memory");
		TTK_FENCE();
		// weight tile NT - 2 has landed; NT - 1 and the residual may be in flight
		trip(std::integral_constant<int, B_PC + RESN>{}, Y{}, I1{}, I1{}, N{}, I0{}, N{}, I1{}, f1, f0, 0u, 0u);
		trip(std::integral_constant<int, RESN>{}, Y{}, I1{}, I2{}, N{}, I1{}, N{}, I1{}, f0, f1, 0u, 0u);              // weight tile NT - 1 has landed
		trip(I0{}, N{}, I0{}, I0{}, N{}, I2{}, N{}, I0{}, f1, f0, 0u, 0u);                                            // the last tile's MFMAs
	}
	pipe_end(scope, TTK_GEMM_STAMPS(p), lane);
	TTK_WSTAMPD(stamps_, blockIdx.x, 3, acc[0][0][0]);
	if (m0 + BM <= p.M) epilogue_role<T, ROLE, false, MI, NI, true>(p, acc, res_pre, bias_pre, row0, col0, lane);
	else epilogue_role<T, ROLE, true, MI, NI, true>(p, acc, res_pre, bias_pre, row0, col0, lane);
	TTK_WSTAMP(stamps_, blockIdx.x, 4);
#if defined(TTK_STAMPS) && TTK_STAMPS == 2
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	TTK_WSTAMP(stamps_, blockIdx.x, 5);
#endif
}

// One output tile [m0, m0 + BM) x [n0, n0 + BN): operand staging, the k-loop and the epilogue.  `wave` = this wave's index among the NWM x NWN waves of the tile.
// LONGK (generic kernel, 64 x 64 wave blocks only): the host promises more k-tiles than ring stages, so the half-tile hand-ordered loop can run without a run-time fallback
template <typename T, int BM, int BN, int NWM, int NWN, int NSTAGE, int ROLE, bool LONGK = false>
__device__ __forceinline__ void gemm_tile(const GemmParams& p, const int m0, const int n0, const int wave) {
	typedef GRole<ROLE> R;
	static_assert(!R::on || (sizeof(T) <= 2 && R::N % BN == 0), "roles are 16-bit or fp8, N a multiple of the tile width");
	constexpr int LDS_AVAIL = NSTAGE * ((BM == 64 && NWM == 1 ? 128 : BM) + BN) * 128;      // (the 64-row half tiles exist only inside k_gemm_mixed, whose launch is sized for its 128-row tiles)
	if constexpr (TTK_CONV_IMAGE && R::on && R::CONV && sizeof(T) == 2 && BN == 64 && NWN == 2 && BM / NWM == 64 && LDS_AVAIL >= 2 * (BM + 8) * 128 + 4 * 8192 + 1024) {
		conv3_image_tile<T, BM, NWM, NWN, ROLE>(p, m0, n0, wave);      // the k = 3 residual convolution on 128 x 64 / 64 x 64 tiles: shared activation image
		return;
	}
	constexpr int ES = sizeof(T);
	constexpr bool F8 = ES == 1;       // fp8 operands: a lane's 16-byte read feeds two 16x16x32 MFMAs (k order is free as long as A and W agree)
	constexpr int BKE = 128 / ES;      // K elements per tile row
	constexpr int KSTEPS = F8 ? 2 : BKE / 32;   // fragment reads per row and tile (one MFMA k-step each; fp8: two)
	constexpr int FCH = F8 ? 1 : 8 * ES / 16;   // 16-byte chunks per fragment
	constexpr int EPC = 16 / ES;       // elements per chunk
	constexpr int NW = NWM * NWN;
	constexpr int WM = BM / NWM, WN = BN / NWN, MI = WM / 16, NI = WN / 16;
	constexpr int A_PC = BM / 8 / NW, B_PC = BN / 8 / NW;   // 1-KiB pieces per wave per tile
	static_assert(A_PC >= 1 && B_PC >= 1 && A_PC * 8 * NW == BM && B_PC * 8 * NW == BN, "tile does not split into 1-KiB pieces per wave");
	constexpr int PER_TILE = A_PC + B_PC;                  // glds instructions per wave per tile
	constexpr int STAGE = (BM + BN) * 128;
	typedef typename Frag<T>::type FragT;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int tid = threadIdx.x, lane = tid & 63;
#ifdef TTK_STAMPS
	unsigned long long* const stamps_ = p.stamps;
#endif
	const int wm = wave / NWN, wn = wave % NWN;
	const int KT = R::on ? GR_K / BKE : p.K / BKE;
	const int NTILES = R::on ? R::NSEG * KT : p.nseg * KT;

	// Staging addresses.  Both operands go through buffer descriptors: the per-lane byte offset inside the matrix (row, swizzled
	// chunk) is fixed for a whole segment, the k advance is the instruction's SCALAR offset, and a lane whose row is outside M or
	// outside its conv tap's batch element gets an out-of-range offset, for which the buffer hardware returns zeros -- so a k-tile
	// costs one s_add per operand instead of 64-bit pointer arithmetic per piece (the first version spent ~600 issue cycles per
	// k-tile on that, next to 256 cycles of MFMA).
	const int prow = lane >> 3, pslot = lane & 7;
	int a_gm[A_PC], a_t[A_PC];
#pragma unroll
	for (int i = 0; i < A_PC; ++i) {
		a_gm[i] = m0 + 8 * (wave + NW * i) + prow;
		if constexpr (R::on) a_t[i] = R::CONV ? a_gm[i] - div_recip(a_gm[i], p.rows_per_batch, p.inv_rpb) * p.rows_per_batch : 0;
		else a_t[i] = p.rows_per_batch > 0 ? a_gm[i] % p.rows_per_batch : 0;
	}
	const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
	constexpr unsigned OOR = 0x80000000u;   // beyond any descriptor's num_records (buffers are < 2 GiB)
	unsigned va[A_PC], vb[B_PC];
#pragma unroll
	for (int i = 0; i < B_PC; ++i) {
		const int row = 8 * (wave + NW * i) + prow;
		const int c = pslot ^ (row & 7);                   // logical chunk landing in this lane's slot
		if constexpr (R::on) vb[i] = (unsigned)((n0 + row) * (GR_K * ES) + c * 16);
		else vb[i] = (unsigned)(((int64_t)(n0 + row) * p.ldw + c * EPC) * ES);
	}
	const __amdgpu_buffer_rsrc_t srdB = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, 0x7fffffff, 0x00020000);
	__amdgpu_buffer_rsrc_t srdA = srdB;
	unsigned b_seg_off = 0;
	int seg_i = 0, kk_i = 0;
	// Tile order of a multi-segment GEMM.  The k = 3 convolutions of the DDIM loop (the CONV role and the generic kernel on the same shape, p.seg_inner) run TAP-INNER since
	// round 6: k-chunk 0 of taps -1 / 0 / +1, then k-chunk 1 of the three taps, ... -- the order in which a staged activation image serves all three taps (conv3_image_tile
	// below), and every other tiling of the same convolution must add its products in that order too (a sequence gives the same bits whatever tile shape its batch selects).
	// Everything else keeps segment-major order (all of segment 0's k, then segment 1's ...).
	const bool seg_in = R::on ? R::CONV : (p.seg_inner != 0);
	const int NSEG = R::on ? R::NSEG : p.nseg;
	unsigned va3[R::CONV ? 3 : 1][A_PC];      // the CONV role: the three taps' staging offsets, computed once
	if constexpr (R::on && R::CONV) {
#pragma unroll
		for (int sg = 0; sg < 3; ++sg)
#pragma unroll
			for (int i = 0; i < A_PC; ++i) {
				const int row = 8 * (wave + NW * i) + prow;
				const int c = pslot ^ (row & 7);
				const int t = a_t[i] + sg - 1;
				const bool ok = a_gm[i] < p.M && t >= 0 && t < p.rows_per_batch;
				va3[sg][i] = ok ? (unsigned)((a_gm[i] + sg - 1) * (GR_K * ES) + c * 16) : OOR;
			}
		srdA = __builtin_amdgcn_make_buffer_rsrc((void*)p.seg[0].A, 0, (unsigned)p.M * (unsigned)(GR_K * ES), 0x00020000);
	}
	auto set_segment = [&](int sg) {
		if constexpr (R::on && R::CONV) {      // one activation tensor, its rows shifted by -1 / 0 / +1 against consecutive [N][K] matrices
			b_seg_off = (unsigned)sg * (unsigned)(R::N * GR_K * ES);
#pragma unroll
			for (int i = 0; i < A_PC; ++i) va[i] = sg == 0 ? va3[0][i] : (sg == 1 ? va3[1][i] : va3[2][i]);
			return;
		}
		if constexpr (R::on) {
			srdA = __builtin_amdgcn_make_buffer_rsrc((void*)p.seg[0].A, 0, (unsigned)p.M * (unsigned)(GR_K * ES), 0x00020000);
			b_seg_off = 0;
#pragma unroll
			for (int i = 0; i < A_PC; ++i) {
				const int row = 8 * (wave + NW * i) + prow;
				const int c = pslot ^ (row & 7);
				va[i] = a_gm[i] < p.M ? (unsigned)(a_gm[i] * (GR_K * ES) + c * 16) : OOR;
			}
			return;
		}
		// (wave-uniform by construction; said explicitly so that the descriptor is built in scalar registers -- the DMA instruction takes it from there only)
		sg = __builtin_amdgcn_readfirstlane(sg);
		const int64_t lda = p.seg[sg].lda;
		const int shift = p.seg[sg].shift;
		srdA = __builtin_amdgcn_make_buffer_rsrc((void*)p.seg[sg].A, 0, (unsigned)((int64_t)p.M * lda * ES), 0x00020000);
		b_seg_off = (unsigned)(p.seg[sg].w_off * ES);
#pragma unroll
		for (int i = 0; i < A_PC; ++i) {
			const int row = 8 * (wave + NW * i) + prow;
			const int c = pslot ^ (row & 7);
			const int t = a_t[i] + shift;
			const bool ok = a_gm[i] < p.M && (shift == 0 || (t >= 0 && t < p.rows_per_batch));
			va[i] = ok ? (unsigned)(((int64_t)(a_gm[i] + shift) * lda + c * EPC) * ES) : OOR;
		}
	};
	auto next_tile = [&] {
		if (seg_in) { if (++seg_i == NSEG) { seg_i = 0; ++kk_i; } }
		else if (++kk_i == KT) { kk_i = 0; ++seg_i; }
		// (wave-uniform by construction; said explicitly: the DMA instruction takes its k offset and descriptor from scalar registers only)
		seg_i = __builtin_amdgcn_readfirstlane(seg_i); kk_i = __builtin_amdgcn_readfirstlane(kk_i);
	};
	auto issue = [&](int stage) {   // requests the next tile of the order above
		if (seg_in || kk_i == 0) set_segment(seg_i);
		const unsigned As = smem_base + stage * STAGE;
		const unsigned Bs = As + BM * 128;
		const unsigned soffA = (unsigned)kk_i * 128u, soffB = b_seg_off + (unsigned)kk_i * 128u;
#pragma unroll
		for (int i = 0; i < A_PC; ++i) {
#ifdef TTK_DIAG_SKIP
			if ((TTK_DIAG_SKIP & 1) && (seg_i > 0 || kk_i > 1)) continue;   // diagnostic: stale A tiles
			// diagnostic 16: the traffic of a k = 3 conv whose taps share ONE staged activation image (A fetched for tap 0 only; results wrong on purpose)
			if ((TTK_DIAG_SKIP & 16) && seg_i > 0) continue;
#endif
			glds16(va[i], srdA, soffA, As + (wave + NW * i) * 1024);
		}
#pragma unroll
		for (int i = 0; i < B_PC; ++i) {
#ifdef TTK_DIAG_SKIP
			if ((TTK_DIAG_SKIP & 2) && (seg_i > 0 || kk_i > 1)) continue;   // diagnostic: stale B tiles
#endif
			glds16(vb[i], srdB, soffB, Bs + (wave + NW * i) * 1024);
		}
		next_tile();
	};

	f32x4 acc[MI][NI];
#pragma unroll
	for (int i = 0; i < MI; ++i)
#pragma unroll
		for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

	const int row0 = m0 + wm * WM, col0 = n0 + wn * WN;
	float res_pre[MI][4][NI];
	float bias_pre[NI];      // roles: the bias of this lane's columns, requested in front of every DMA piece (the wave's oldest requests: retired by the first counted wait)
	if constexpr (R::on) {
#pragma unroll
		for (int j = 0; j < NI; ++j) bias_pre[j] = p.bias[col0 + 16 * j + (lane & 15)];
	}
	constexpr int RESN = MI * 4 * NI;
	constexpr bool PRE_RES = R::on && R::RES && NSTAGE >= 3 && (NSTAGE - 2) * PER_TILE + RESN <= 63 && (NSTAGE == 3 || (TTK_GEMM_PIPE && ES == 2 && MI * NI <= 8));
	// wait until at most `tiles` of this wave's requested tiles are still in flight (vmcnt takes an immediate: uniform branch chain)
	auto wait_tiles = [&](int tiles) {
		if (tiles <= 0) wait_vmcnt<0>();
		else if (tiles == 1) wait_vmcnt<PER_TILE>();
		else if (tiles == 2 || NSTAGE <= 4) wait_vmcnt<2 * PER_TILE>();
		else if (tiles == 3 || NSTAGE <= 5) wait_vmcnt<3 * PER_TILE>();
		else wait_vmcnt<4 * PER_TILE>();
	};
	// the hand-ordered k-step (see pipe_read16 above) for wave blocks up to 64 x 32: two fragment sets of a 64 x 64 block (128 registers) beside its 64 accumulators do not fit
	// 256 registers -- the allocator spills, and a spill between two asm statements may move a fragment before its data has landed; f32 / fp8 operands and the other ring
	// depths keep the compiler's order as well
	constexpr bool PIPE = TTK_GEMM_PIPE && ES == 2 && (NSTAGE == 3 || (R::on && NSTAGE > 3 && NSTAGE <= 6)) && MI * NI <= 8;
	// 64 x 64 wave blocks (the 256 x 128 tile of the q / k / v projection): the same hand-ordered stream at HALF-tile granularity -- a fragment set holds ONE k-step (32 registers),
	// so two sets fit beside the 64 accumulators.  Half-step H0 of tile kt multiplies its k-step 0 (set f0) while k-step 1 of the SAME tile is read into f1 (no barrier: the tile
	// has landed); H1 waits for tile kt + 1, passes the barrier (every wave's reads of tile kt ended with H0), multiplies k-step 1 while k-step 0 of tile kt + 1 is read into f0,
	// and requests tile kt + NSTAGE into the stage tile kt has left.  Same MFMA order per accumulator (k-step 0, then 1): same bits.
	// (the residual roles keep the compiler-ordered loop at this tile: their epilogue needs 64 more registers and the allocator spills inside the hand-ordered stream)
	constexpr bool PIPE_H = TTK_GEMM_PIPE_H && ES == 2 && NSTAGE == 3 && ((R::on && !R::RES) || (!R::on && LONGK)) && MI * NI == 16 && KSTEPS == 2;
	if constexpr (PIPE_H) {
		constexpr int NM = MI * NI, NR = MI + NI, D0 = NM - PER_TILE - 1;      // 16 MFMAs, 8 reads (one per gap from the first), the DMA pieces in the last gaps
		static_assert(NR <= NM && D0 >= 0, "reads and DMA pieces must fit the gaps of a half-step");
		const int NT = NTILES;      // (roles: a compile-time constant; generic: > NSTAGE by LONGK)
		static_assert(!R::on || R::NSEG * (GR_K / BKE) > NSTAGE, "the ring is deeper than the k-loop");
		struct HFrags { u32x4 a[MI], b[NI]; };
		unsigned fa[KSTEPS], fb[KSTEPS];
#pragma unroll
		for (int ks = 0; ks < KSTEPS; ++ks) {
			const int c0 = 4 * ks + (lane >> 4), rowa = wm * WM + (lane & 15), rowb = wn * WN + (lane & 15);
			fa[ks] = smem_base + rowa * 128 + ((c0 ^ (rowa & 7)) << 4);
			fb[ks] = smem_base + BM * 128 + rowb * 128 + ((c0 ^ (rowb & 7)) << 4);
		}
		unsigned pA_dst = 0, pB_dst = 0, p_soffA = 0, p_soffB = 0;
		auto issue_prep = [&](unsigned stage_off) {
			if (seg_in || kk_i == 0) set_segment(seg_i);
			pA_dst = smem_base + stage_off; pB_dst = pA_dst + BM * 128;
			p_soffA = (unsigned)kk_i * 128u; p_soffB = b_seg_off + (unsigned)kk_i * 128u;
			next_tile();
		};
		auto issue_piece = [&](auto d_) {
			constexpr int d = decltype(d_)::value;
			if constexpr (d < A_PC) pipe_glds16(va[d], srdA, p_soffA, pA_dst + (wave + NW * d) * 1024);
			else pipe_glds16(vb[d - A_PC], srdB, p_soffB, pB_dst + (wave + NW * (d - A_PC)) * 1024);
		};
		auto read_one = [&](auto r_, HFrags& fr, unsigned ra, unsigned rb) {
			constexpr int r = decltype(r_)::value;
			if constexpr (r < MI) pipe_read16<r * 2048>(fr.a[r], ra);
			else pipe_read16<(r - MI) * 2048>(fr.b[r - MI], rb);
		};
		// one half-step: [wait for W loads at most + barrier] 16 MFMAs of `cur`; RD: 8 reads into `nxt` (addresses ra / rb), one per gap; ISSUE: the next tile's pieces in the last gaps
		auto htrip = [&](auto bar_, auto w_, auto rd_, auto issue_, const HFrags& cur, HFrags& nxt, unsigned ra, unsigned rb) {
			constexpr bool BAR = decltype(bar_)::value, RD = decltype(rd_)::value, ISSUE = decltype(issue_)::value;
			if constexpr (BAR) { wait_vmcnt<decltype(w_)::value>(); pipe_barrier(); }
			static_for<0, NM>([&](auto m_) {
				constexpr int m = decltype(m_)::value, i = m / NI, j = m % NI;
				pipe_mfma<T>(acc[i][j], cur.a[i], cur.b[j]);
				if constexpr (RD && m < NR) read_one(m_, nxt, ra, rb);
				if constexpr (ISSUE && m >= D0 && m - D0 < PER_TILE) issue_piece(std::integral_constant<int, m - D0>{});
			});
			if constexpr (RD) pipe_lgkm0();
		};
		typedef std::true_type Y; typedef std::false_type N; typedef std::integral_constant<int, 0> W0;
		PipeScope scope = pipe_begin();
#pragma unroll
		for (int st = 0; st < NSTAGE; ++st) { issue_prep(st * STAGE); static_for<0, PER_TILE>(issue_piece); }
		TTK_WSTAMP(stamps_, blockIdx.x, 1);
		wait_vmcnt<(NSTAGE - 1) * PER_TILE>();      // tile 0 has landed
		pipe_barrier();
		TTK_WSTAMP(stamps_, blockIdx.x, 2);
		HFrags f0, f1;
		static_for<0, NR>([&](auto r_) { read_one(r_, f0, fa[0], fb[0]); });
		pipe_lgkm0();
		scope.clk = kclock_start();
		unsigned cur_off = 0, nxt_off = STAGE;      // stages of tile kt and tile kt + 1
		auto advance = [&] { cur_off = nxt_off; nxt_off = nxt_off == (NSTAGE - 1) * STAGE ? 0u : nxt_off + STAGE; };
		for (int kt = 0; kt < NT - NSTAGE; ++kt) {      // tiles whose second half-step requests a tile
			htrip(N{}, W0{}, Y{}, N{}, f0, f1, fa[1] + cur_off, fb[1] + cur_off);
			issue_prep(cur_off);
			htrip(Y{}, std::integral_constant<int, (NSTAGE - 2) * PER_TILE>{}, Y{}, Y{}, f1, f0, fa[0] + nxt_off, fb[0] + nxt_off);
			advance();
		}
		static_for<0, NSTAGE - 1>([&](auto t_) {      // tile NT - NSTAGE + t: nothing left to request; tile + 1 has landed, the NSTAGE - 2 - t younger ones may be in flight
			htrip(N{}, W0{}, Y{}, N{}, f0, f1, fa[1] + cur_off, fb[1] + cur_off);
			htrip(Y{}, std::integral_constant<int, (NSTAGE - 2 - decltype(t_)::value) * PER_TILE>{}, Y{}, N{}, f1, f0, fa[0] + nxt_off, fb[0] + nxt_off);
			advance();
		});
		htrip(N{}, W0{}, Y{}, N{}, f0, f1, fa[1] + cur_off, fb[1] + cur_off);      // the last tile
		htrip(N{}, W0{}, N{}, N{}, f1, f0, 0u, 0u);
		pipe_end(scope, TTK_GEMM_STAMPS(p), lane);
	} else if constexpr (PIPE) {
		constexpr int NM = KSTEPS * MI * NI, NR = KSTEPS * (MI + NI);
		constexpr int PREB = TTK_PIPE_PREB, DPG = TTK_PIPE_DPG;
		constexpr int RPG_MIN = (NR + (NM - PREB) - 1) / (NM - PREB), RPG = TTK_PIPE_RPG > RPG_MIN ? TTK_PIPE_RPG : RPG_MIN;      // (narrow wave blocks have more reads than gaps)
		constexpr int RGAPS = (NR + RPG - 1) / RPG, DGAPS = (PER_TILE + DPG - 1) / DPG;
		constexpr int D0 = TTK_PIPE_DLATE || PREB + TTK_PIPE_D0 > NM - DGAPS ? NM - DGAPS : PREB + TTK_PIPE_D0;
		static_assert(PREB + RGAPS <= NM && D0 >= PREB && D0 + DGAPS <= NM, "reads and DMA pieces must fit the gaps behind the barrier");
		struct PFrags { u32x4 a[KSTEPS][MI], b[KSTEPS][NI]; };
		// this lane's chunk of fragment row (lane & 15) in stage 0, per k-step: chunk (4 ks + (lane >> 4)) ^ (row & 7); sub-tile i / j adds 2048 i (an immediate)
		unsigned fa[KSTEPS], fb[KSTEPS];
#pragma unroll
		for (int ks = 0; ks < KSTEPS; ++ks) {
			const int c0 = 4 * ks + (lane >> 4), rowa = wm * WM + (lane & 15), rowb = wn * WN + (lane & 15);
			fa[ks] = smem_base + rowa * 128 + ((c0 ^ (rowa & 7)) << 4);
			fb[ks] = smem_base + BM * 128 + rowb * 128 + ((c0 ^ (rowb & 7)) << 4);
		}
		unsigned pA_dst = 0, pB_dst = 0, p_soffA = 0, p_soffB = 0;      // the tile being requested in this step
#ifdef TTK_DIAG_SKIP
		bool p_skipA = false, p_skipB = false;
#endif
		auto issue_prep = [&](unsigned stage_off) {   // the next tile in (segment, k) order goes to the stage at byte offset stage_off
			if (seg_in || kk_i == 0) set_segment(seg_i);
#ifdef TTK_DIAG_SKIP
			p_skipA = ((TTK_DIAG_SKIP & 1) && (seg_i > 0 || kk_i > 1)) || ((TTK_DIAG_SKIP & 16) && seg_i > 0);
			p_skipB = (TTK_DIAG_SKIP & 2) && (seg_i > 0 || kk_i > 1);
#endif
			pA_dst = smem_base + stage_off; pB_dst = pA_dst + BM * 128;
			p_soffA = (unsigned)kk_i * 128u; p_soffB = b_seg_off + (unsigned)kk_i * 128u;
			next_tile();
		};
		auto issue_piece = [&](auto d_) {
			constexpr int d = decltype(d_)::value;
			if constexpr (d < A_PC) {
#ifdef TTK_DIAG_SKIP
				if (p_skipA) return;
#endif
				pipe_glds16(va[d], srdA, p_soffA, pA_dst + (wave + NW * d) * 1024);
			} else {
#ifdef TTK_DIAG_SKIP
				if (p_skipB) return;
#endif
				pipe_glds16(vb[d - A_PC], srdB, p_soffB, pB_dst + (wave + NW * (d - A_PC)) * 1024);
			}
		};
		auto read_one = [&](auto r_, PFrags& fr, const unsigned (&ra)[KSTEPS], const unsigned (&rb)[KSTEPS]) {
			constexpr int r = decltype(r_)::value, ks = r / (MI + NI), q = r % (MI + NI);
			if constexpr (q < MI) pipe_read16<q * 2048>(fr.a[ks][q], ra[ks]);
			else pipe_read16<(q - MI) * 2048>(fr.b[ks][q - MI], rb[ks]);
		};
		// One k-step: the MFMAs of tile kt (`cur`) in (ks, i, j) order; behind MFMA number PREB the caller's wait + barrier (tile kt+1 has landed for everyone, and
		// everyone's reads of tile kt ended with the lgkmcnt(0) of the step before, so its stage may be refilled); from there on RPG reads of tile kt+1 into `nxt` per
		// MFMA gap, the DMA pieces of tile kt+3 one per gap in the last gaps; the step ends with this wave's reads drained.
		auto trip = [&](auto issue_, auto&& pre, const PFrags& cur, PFrags& nxt, unsigned rd_off) {
			constexpr bool ISSUE = decltype(issue_)::value;
			unsigned ra[KSTEPS], rb[KSTEPS];
#pragma unroll
			for (int ks = 0; ks < KSTEPS; ++ks) { ra[ks] = fa[ks] + rd_off; rb[ks] = fb[ks] + rd_off; }
			static_for<0, NM>([&](auto m_) {
				constexpr int m = decltype(m_)::value, ks = m / (MI * NI), i = (m % (MI * NI)) / NI, j = m % NI;
				if constexpr (m == PREB) pre();
#if !(defined(TTK_DIAG_SKIP) && (TTK_DIAG_SKIP & 8))
				pipe_mfma<T>(acc[i][j], cur.a[ks][i], cur.b[ks][j]);
#endif
#if !(defined(TTK_DIAG_SKIP) && (TTK_DIAG_SKIP & 4))
				static_for<0, RPG>([&](auto q_) {
					constexpr int r = (m - PREB) * RPG + decltype(q_)::value;
					if constexpr (m >= PREB && r < NR) read_one(std::integral_constant<int, r>{}, nxt, ra, rb);
				});
#endif
				if constexpr (ISSUE) static_for<0, DPG>([&](auto q_) {
					constexpr int d = (m - D0) * DPG + decltype(q_)::value;
					if constexpr (m >= D0 && d < PER_TILE) issue_piece(std::integral_constant<int, d>{});
				});
			});
			pipe_lgkm0();
		};

		auto barrier = [&] { TTK_FENCE(); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); TTK_FENCE(); };
		// (this loop keeps its own barrier lambda, M0 save / restore and clock tail instead of pipe_barrier / pipe_begin / pipe_end: with either shared form the
		// residual roles' instantiations come out with another compiler-placed vmcnt and register assignment; the other two hand-ordered loops do not care)
		const unsigned m0_keep = pipe_m0_save();
#pragma unroll
		for (int st = 0; st < NSTAGE; ++st)
			if (st < NTILES) { issue_prep(st * STAGE); static_for<0, PER_TILE>(issue_piece); }
		TTK_WSTAMP(stamps_, blockIdx.x, 1);
		wait_tiles(min(NSTAGE, NTILES) - 1);                       // tile 0 has landed
		barrier();
		TTK_WSTAMP(stamps_, blockIdx.x, 2);
		PFrags f0, f1;
		static_for<0, NR>([&](auto r_) { read_one(r_, f0, fa, fb); });
		pipe_lgkm0();
#ifdef TTK_CLOCK_STAMPS
		const unsigned long long clk0_ = __builtin_amdgcn_s_memtime(), rt0_ = __builtin_amdgcn_s_memrealtime();
#endif
		unsigned rd_off = STAGE, wr_off = 0;      // stages of tile kt+1 (read in step kt) and of tile kt (refilled in step kt)
		auto advance = [&] { rd_off = rd_off == (NSTAGE - 1) * STAGE ? 0u : rd_off + STAGE; wr_off = wr_off == (NSTAGE - 1) * STAGE ? 0u : wr_off + STAGE; };
		auto mfma_last = [&](const PFrags& cur) {
			static_for<0, NM>([&](auto m_) {
				constexpr int m = decltype(m_)::value, ks = m / (MI * NI), i = (m % (MI * NI)) / NI, j = m % NI;
				pipe_mfma<T>(acc[i][j], cur.a[ks][i], cur.b[ks][j]);
			});
		};
		// the three kinds of step: one that requests a tile (two younger tiles exist and one of them stays in flight: vmcnt(PER_TILE)), and the two of the tail, which
		// request nothing and wait with a constant as well.  ONE body per kind: a run-time "request or not" would give the loop two bodies with their own register
		// assignment and accumulator copies between them.
		auto pstep_i = [&](const PFrags& cur, PFrags& nxt) {
			auto pre = [&] { wait_vmcnt<(NSTAGE - 2) * PER_TILE>(); barrier(); };
			issue_prep(wr_off); trip(std::true_type{}, pre, cur, nxt, rd_off);
			advance();
		};
		auto ptail = [&](auto wtag, const PFrags& cur, PFrags& nxt) {
			auto pre = [&] { wait_vmcnt<decltype(wtag)::value>(); barrier(); };
			trip(std::false_type{}, pre, cur, nxt, rd_off);
			advance();
		};
		if constexpr (R::on) {      // tile count known at compile time: NT - NSTAGE steps that request a tile, NSTAGE - 1 that do not, the last tile's MFMAs; tile kt lives in f[kt & 1]
			constexpr int NT = R::NSEG * (GR_K / BKE), NMAIN = NT - NSTAGE;
			static_assert(NMAIN >= 2, "the ring is deeper than the k-loop");
			for (int kt = 0; kt + 2 <= NMAIN; kt += 2) { pstep_i(f0, f1); pstep_i(f1, f0); }
			if constexpr (NMAIN & 1) pstep_i(f0, f1);      // requests the last tile (NT - 1)
			if constexpr (PRE_RES) {      // (the residual tile is requested right behind the last DMA request: see the compiler-ordered branch below)
				if (m0 + BM <= p.M) load_residual_role<ROLE, MI, NI, false>(p, res_pre, row0, col0, lane);
				else load_residual_role<ROLE, MI, NI, true>(p, res_pre, row0, col0, lane);
				asm volatile("" ::: "memory");
				TTK_FENCE();
			}
			static_for<0, NSTAGE - 1>([&](auto t_) {      // step NMAIN + t: tile NMAIN + t + 1 has landed; the NSTAGE - 2 - t younger ones and the residual may be in flight
				constexpr int t = decltype(t_)::value, W = (NSTAGE - 2 - t) * PER_TILE + (PRE_RES ? RESN : 0);
				if constexpr (((NMAIN + t) & 1) == 0) ptail(std::integral_constant<int, W>{}, f0, f1);
				else ptail(std::integral_constant<int, W>{}, f1, f0);
			});
			if constexpr (((NT - 1) & 1) == 0) mfma_last(f0); else mfma_last(f1);
		} else {
			static_assert(R::on || NSTAGE == 3, "run-time tile counts: 3-stage ring only");
			const int nmain = NTILES > NSTAGE ? NTILES - NSTAGE : 0;      // steps that request a tile
			int kt = 0;
			for (; kt + 2 <= nmain; kt += 2) { pstep_i(f0, f1); pstep_i(f1, f0); }
			if (kt < nmain) { pstep_i(f0, f1); f0 = f1; ++kt; }          // (an odd count: tile kt's fragments move to f0 -- 48 register copies behind the step's lgkmcnt(0))
			if (NTILES - kt >= 3) { ptail(std::integral_constant<int, PER_TILE>{}, f0, f1); ptail(std::integral_constant<int, 0>{}, f1, f0); mfma_last(f0); }
			else if (NTILES - kt == 2) { ptail(std::integral_constant<int, 0>{}, f0, f1); mfma_last(f1); }
			else mfma_last(f0);
		}
		pipe_m0_restore(m0_keep);
#ifdef TTK_CLOCK_STAMPS
		if (stamps_ && lane == 0) {      // shader cycles and 100 MHz ticks of this wave's k-loop (diagnostic build: MI355X_MICROARCH.md, DVFS give-back item 6)
			unsigned long long* st_ = stamps_ + ((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 8;
			st_[6] = ((__builtin_amdgcn_s_memtime() - clk0_) << 32) | ((__builtin_amdgcn_s_memrealtime() - rt0_) & 0xffffffffull);
		}
#endif
	} else {
		// Fragment registers of one k-tile (all k-steps), two sets used ping-pong: the ds_reads of tile k+1 are in flight under the
		// MFMAs of tile k (with one wave per SIMD nothing else hides the ~130-cycle LDS latency; measured 735 cycles per k-tile for
		// 256 cycles of MFMA before this).  Named structs + a 2x unrolled loop: an indexed array of register sets would go to scratch.
		typedef int i32x4 __attribute__((ext_vector_type(4)));
		typedef int i32x8 __attribute__((ext_vector_type(8)));
		struct Frags { uint4 a[F8 ? 1 : KSTEPS][F8 ? 1 : MI][FCH]; uint4 b[F8 ? 1 : KSTEPS][F8 ? 1 : NI][FCH]; i32x8 a8[F8 ? MI : 1], b8[F8 ? NI : 1]; };
		auto read_frags = [&](Frags& fr, int stage) {
			const char* As = smem + stage * STAGE;
			const char* Bs = As + BM * 128;
			if constexpr (F8) {      // a lane's 32 operand bytes of the 128-deep k-tile: chunks g and 4 + g of its row, joined into the instruction's 8-dword operand
				const int g = lane >> 4;
	#pragma unroll
				for (int i = 0; i < MI; ++i) {
					const int row = wm * WM + 16 * i + (lane & 15);
					const i32x4 lo = *(const i32x4*)(As + row * 128 + ((g ^ (row & 7)) << 4)), hi = *(const i32x4*)(As + row * 128 + (((4 + g) ^ (row & 7)) << 4));
					fr.a8[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
				}
	#pragma unroll
				for (int j = 0; j < NI; ++j) {
					const int row = wn * WN + 16 * j + (lane & 15);
					const i32x4 lo = *(const i32x4*)(Bs + row * 128 + ((g ^ (row & 7)) << 4)), hi = *(const i32x4*)(Bs + row * 128 + (((4 + g) ^ (row & 7)) << 4));
					fr.b8[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
				}
				return;
			}
	#pragma unroll
			for (int ks = 0; ks < KSTEPS; ++ks) {
				const int c0 = F8 ? 4 * ks + (lane >> 4) : (ks * 32 + 8 * (lane >> 4)) / EPC;
	#pragma unroll
				for (int i = 0; i < MI; ++i) {
					const int row = wm * WM + 16 * i + (lane & 15);
	#pragma unroll
					for (int f = 0; f < FCH; ++f) fr.a[ks][i][f] = *(const uint4*)(As + row * 128 + (((c0 + f) ^ (row & 7)) << 4));
				}
	#pragma unroll
				for (int j = 0; j < NI; ++j) {
					const int row = wn * WN + 16 * j + (lane & 15);
	#pragma unroll
					for (int f = 0; f < FCH; ++f) fr.b[ks][j][f] = *(const uint4*)(Bs + row * 128 + (((c0 + f) ^ (row & 7)) << 4));
				}
			}
		};
		auto mfma_tile = [&](const Frags& fr) {
			if constexpr (F8) {
				// fp8 operands: ONE block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 per sub-tile and 128-deep k-tile (round 6; unit E8M0 scales: the weights' power-of-two tensor
				// scale stays in the epilogue).  It takes twice the cycles of a 16x16x32 instruction for four times the K: the non-scaled fp8 form this loop ran before runs at
				// the BF16 rate, so the MFMA phase of a trip halves (MI355X_MICROARCH.md, matrix-core table).  A lane's 32 operand bytes are its two 16-byte reads (chunks g and
				// 4 + g of the row); the instruction's own k position of each byte does not matter as long as A and W use the same one, which the identical staging guarantees.
	#pragma unroll
				for (int i = 0; i < MI; ++i)
	#pragma unroll
					for (int j = 0; j < NI; ++j) {
	#if TTK_FP8_SCALED_MFMA
						acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fr.a8[i], fr.b8[j], acc[i][j], 0 /* A: e4m3 */, 0 /* B: e4m3 */, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
	#else
						typedef long l64x4 __attribute__((ext_vector_type(4)));
						const l64x4 la = (l64x4)fr.a8[i], lb = (l64x4)fr.b8[j];
	#pragma unroll
						for (int q = 0; q < 4; ++q) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(la[q], lb[q], acc[i][j], 0, 0, 0);
	#endif
					}
				return;
			}
	#pragma unroll
			for (int ks = 0; ks < KSTEPS; ++ks)
	#pragma unroll
				for (int i = 0; i < MI; ++i)
	#pragma unroll
					for (int j = 0; j < NI; ++j) {
						if constexpr (F8) {
							union { uint4 q; long l[2]; } ua, ub;
							ua.q = fr.a[ks][i][0]; ub.q = fr.b[ks][j][0];
							acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(ua.l[0], ub.l[0], acc[i][j], 0, 0, 0);
							acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(ua.l[1], ub.l[1], acc[i][j], 0, 0, 0);
						} else {
							union { FragT v; uint4 q[FCH]; } ua, ub;
	#pragma unroll
							for (int f = 0; f < FCH; ++f) { ua.q[f] = fr.a[ks][i][f]; ub.q[f] = fr.b[ks][j][f]; }
							acc[i][j] = mma16<typename std::conditional<F8, bf16, T>::type>(ua.v, ub.v, acc[i][j]);
						}
					}
		};
		// One pipeline step for tile kt (not the last) whose fragments are already in `cur`:
		//   wait until tile kt+1 has landed for this wave (tile kt+2 may stay in flight) and this wave's reads of tile kt are done;
		//   barrier: now tile kt+1 has landed for every wave and stage kt%NSTAGE is free everywhere;
		//   request tile kt+NSTAGE into stage kt%NSTAGE, start reading tile kt+1's fragments, multiply tile kt.
		// The fragment reads must NOT sit under a condition: the compiler does not see the hand-written waits, so it protects the
		// MFMAs' operands itself, and with the reads of the next tile in a conditional block it can only do that with lgkmcnt(0) --
		// i.e. the MFMAs of tile kt waited for the reads of tile kt+1 and nothing overlapped (what the first version of this loop
		// did: ~1050 cycles per k-tile for 256 cycles of MFMA and 384 of LDS reads).  Hence the peeled last tile below.
		auto step = [&](int kt, const Frags& cur, Frags& nxt) {
			wait_tiles(min(NSTAGE - 2, NTILES - 2 - kt));          // tile kt+1 has landed; up to NSTAGE-2 younger ones stay in flight
			// diagnostic 32: what the drain of this wave's fragment reads in front of the barrier costs (only meaningful with 3: no DMA overwrites anything)
	#if !(defined(TTK_DIAG_SKIP) && (TTK_DIAG_SKIP & 32))
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	#endif
	#if !(defined(TTK_DIAG_SKIP) && (TTK_DIAG_SKIP & 64))         // diagnostic 64: no workgroup barrier in the k-loop (with 3)
			__builtin_amdgcn_s_barrier();
	#endif
			asm volatile("" ::: "memory");
	#ifdef TTK_DIAG_SKIP
			if ((TTK_DIAG_SKIP & 4) && kt > 0) { if (kt + NSTAGE < NTILES) issue(kt % NSTAGE); mfma_tile(cur); return; }   // diagnostic: no LDS fragment reads (stale registers)
			if ((TTK_DIAG_SKIP & 8) && kt > 0) { if (kt + NSTAGE < NTILES) issue(kt % NSTAGE); read_frags(nxt, (kt + 1) % NSTAGE); return; }   // diagnostic: no MFMAs
	#endif
			// (Pinning the order with sched_barriers -- all reads first, DMA issue between the two k-steps' MFMAs -- won 10% in an L2-hot
			// microbenchmark and LOST 2% in the diffusion loop, where activations and weights arrive cold: tests/diag/ddim_ab.py.)
			if (kt + NSTAGE < NTILES) issue(kt % NSTAGE);
			read_frags(nxt, (kt + 1) % NSTAGE);
			mfma_tile(cur);
		};

	#pragma unroll
		for (int st = 0; st < NSTAGE; ++st)
			if (st < NTILES) issue(st);
		TTK_WSTAMP(stamps_, blockIdx.x, 1);
		wait_tiles(min(NSTAGE, NTILES) - 1);                       // tile 0 has landed
		__builtin_amdgcn_s_barrier();
		asm volatile("" ::: "memory");
		TTK_WSTAMP(stamps_, blockIdx.x, 2);
		Frags f0, f1;
		read_frags(f0, 0);
		// Roles with a residual (the k = 3 conv and proj_out of the DDIM loop, C aliasing the residual): its tile is requested UNDER the last two k-tiles instead of
		// in the epilogue, where its round trip was the longest single item (1.9 us of epilogue against 1.0 without a residual, profiles/r04_ddim_chain_roles.log).
		// The requests leave right behind the LAST DMA request, so they are younger than every piece of the ring: vmcnt retires in order, and the two counted waits
		// that follow simply allow RESN more loads in flight.  (Round 3 requested the tile at the top of the kernel: 32 loads in front of the first DMA request cost more
		// than the epilogue gained.)  Same values into the same additions: same bits.
		if constexpr (PRE_RES) {
			constexpr int NT = R::NSEG * (GR_K / BKE);
			static_assert(!PRE_RES || (NT % 2 == 0 && NT >= 8), "the peeled tail assumes an even tile count");
			auto tail_step = [&](auto wtag, int stage_next, const Frags& cur, Frags& nxt) {
				wait_vmcnt<decltype(wtag)::value>();
	#if !(defined(TTK_DIAG_SKIP) && (TTK_DIAG_SKIP & 32))
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	#endif
				__builtin_amdgcn_s_barrier();
				asm volatile("" ::: "memory");
				read_frags(nxt, stage_next);
				mfma_tile(cur);
			};
			int kt = 0;
			for (; kt < NT - 4; kt += 2) {      // every one of these steps requests a tile
				step(kt, f0, f1);
				step(kt + 1, f1, f0);
			}
			step(NT - 4, f0, f1);                // requests the last tile (NT - 1)
			if (m0 + BM <= p.M) load_residual_role<ROLE, MI, NI, false>(p, res_pre, row0, col0, lane);      // (straight-line: 32 requests back to back)
			else load_residual_role<ROLE, MI, NI, true>(p, res_pre, row0, col0, lane);
			asm volatile("" ::: "memory");
			tail_step(std::integral_constant<int, PER_TILE + RESN>{}, (NT - 2) % NSTAGE, f1, f0);      // tile NT-2 has landed; tile NT-1 and the residual may be in flight
			tail_step(std::integral_constant<int, RESN>{}, (NT - 1) % NSTAGE, f0, f1);                 // tile NT-1 has landed
			mfma_tile(f1);
		} else {
			int kt = 0;
			for (; kt + 2 < NTILES; kt += 2) {      // both tiles of a round have a successor
				step(kt, f0, f1);
				step(kt + 1, f1, f0);
			}
			if (kt + 2 == NTILES) { step(kt, f0, f1); mfma_tile(f1); }
			else mfma_tile(f0);
		}
	}
	TTK_WSTAMPD(stamps_, blockIdx.x, 3, acc[0][0][0]);

	if constexpr (R::on) {
		if (m0 + BM <= p.M) epilogue_role<T, ROLE, false, MI, NI, PRE_RES>(p, acc, res_pre, bias_pre, row0, col0, lane);
		else epilogue_role<T, ROLE, true, MI, NI, PRE_RES>(p, acc, res_pre, bias_pre, row0, col0, lane);
		TTK_WSTAMP(stamps_, blockIdx.x, 4);
#if defined(TTK_STAMPS) && TTK_STAMPS == 2
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		TTK_WSTAMP(stamps_, blockIdx.x, 5);
#endif
		return;
	}
	const bool full = (m0 + BM <= p.M) && (n0 + BN <= p.N);
	if (p.transpose_out) { if (full) epilogue<T, 2, false, MI, NI>(p, acc, row0, col0, lane); else epilogue<T, 2, true, MI, NI>(p, acc, row0, col0, lane); }
	else if (p.out_f32) { if (full) epilogue<T, 1, false, MI, NI>(p, acc, row0, col0, lane); else epilogue<T, 1, true, MI, NI>(p, acc, row0, col0, lane); }
	else { if (full) epilogue<T, 0, false, MI, NI>(p, acc, row0, col0, lane); else epilogue<T, 0, true, MI, NI>(p, acc, row0, col0, lane); }
	TTK_WSTAMP(stamps_, blockIdx.x, 4);
#if defined(TTK_STAMPS) && TTK_STAMPS == 2
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	TTK_WSTAMP(stamps_, blockIdx.x, 5);
#endif
}

// XCD-aware tile order (cdna_hip_programming.md T1, bijective form): workgroups are dealt round-robin over the 8 XCDs, so give
// each XCD label (block % 8) a CONTIGUOUS run of the n-major tile order = a few n-tiles x all m-tiles.  Its private 4 MiB
// L2 then holds that weight slice while the activations stream through once, instead of every XCD caching all of W.
template <typename B> __device__ __forceinline__ int xcd_tile_id(B block, int nwg) {      // (B: blockIdx.x is unsigned, k_gemm_mixed's block index an int)
	const int xcd = block & 7, q = nwg >> 3, r = nwg & 7;
	return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (block >> 3);
}

// NWM x NWN waves per workgroup; 8 waves (2 per SIMD) let one wave's MFMAs run under another's LDS reads and DMA issue.
template <typename T, int BM, int BN, int NWM, int NWN, int NSTAGE, int ROLE = GR_NONE, bool LONGK = false>
__global__ __launch_bounds__(64 * NWM * NWN, 2) void k_gemm(GemmParams p) {
	typedef GRole<ROLE> R;

	// what the prologue and the first segment read, as one batch of scalar loads (the ~500-byte argument block was fetched in six dependent round trips:
	// a wave's first DMA request left 1.8 us after its first instruction, 1.2 us with the batch -- tests/diag/ddim_chain.cpp; pinning the epilogue's
	// fields as well costs more in SGPR pressure than it returns, profiles/r03 notes)
	if constexpr (R::on) {
		if constexpr (R::CONV) TTK_PIN_ARGS(TTK_S(p.M), TTK_S(p.W), TTK_S(p.seg[0].A), TTK_S(p.tiles_m), TTK_S(p.inv_tiles_m), TTK_S(p.rows_per_batch), TTK_S(p.inv_rpb));
		else TTK_PIN_ARGS(TTK_S(p.M), TTK_S(p.W), TTK_S(p.seg[0].A), TTK_S(p.tiles_m), TTK_S(p.inv_tiles_m));
	} else {
		TTK_PIN_ARGS(TTK_S(p.M), TTK_S(p.N), TTK_S(p.K), TTK_S(p.nseg), TTK_S(p.W), TTK_S(p.ldw), TTK_S(p.rows_per_batch), TTK_S(p.m_major),
					 TTK_S(p.seg[0].A), TTK_S(p.seg[0].lda), TTK_S(p.seg[0].shift), TTK_S(p.seg[0].w_off));
	}
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#ifdef TTK_STAMPS
	unsigned long long* const stamps_ = p.stamps;
#endif
	TTK_WSTAMP(stamps_, blockIdx.x, 0);
	const int tiles_m = R::on ? p.tiles_m : (p.M + BM - 1) / BM;
	const int tile_id = xcd_tile_id(blockIdx.x, R::on ? tiles_m * (R::N / BN) : (int)gridDim.x);
	// p.m_major: the XCD's run of tiles is a few m-tiles x ALL n-tiles instead -- its L2 then holds the whole weight matrix plus an eighth of
	// the activations, which is the smaller working set when the matrix (N x K) is smaller than the activation panel (M x K)
	int m0, n0;
	if constexpr (R::on) {      // n-major order, no integer division
		const int tn = div_recip(tile_id, tiles_m, p.inv_tiles_m);
		m0 = (tile_id - tn * tiles_m) * BM; n0 = tn * BN;
	} else {
		const int tiles_n = (p.N + BN - 1) / BN;
		m0 = p.m_major ? (tile_id / tiles_n) * BM : (tile_id % tiles_m) * BM;
		n0 = p.m_major ? (tile_id % tiles_n) * BN : (tile_id / tiles_m) * BN;
	}
	gemm_tile<T, BM, BN, NWM, NWN, NSTAGE, ROLE, LONGK>(p, m0, n0, wave);
}

// Mixed grid for the statistics roles when the 128 x 64 tiling leaves a few tiles more than there are CUs (the DDIM step at T = 1088: 17 x 16 = 272 tiles on 256
// CUs -- the 16 CUs that hold two finish 1.4 x later and set the length of three launches per layer: 25.9 us against 19.5 us for the same k = 3 conv at T = 1024,
// profiles/r04_ddim_chain_T1024_vs_T1088.log).  The first `mix_full` workgroups are the full tiles of the first mix_fm tile rows, one per CU; the remaining rows are cut into
// 64 x 64 tiles run by TWO waves each (the other two leave at once), so the surplus is spread over twice as many CUs in pieces half the size, and
// every wave still owns a 64-row x 32-channel statistics chunk.  Same k order per output element as any other tiling: same bits.
template <typename T, int ROLE>
__global__ __launch_bounds__(256, 2) void k_gemm_mixed(GemmParams p) {
	typedef GRole<ROLE> R;
	static_assert(R::on && R::N == 1024, "mixed grids serve the 1024-wide roles");
	if constexpr (R::CONV) TTK_PIN_ARGS(TTK_S(p.M), TTK_S(p.W), TTK_S(p.seg[0].A), TTK_S(p.mix_full), TTK_S(p.mix_fm), TTK_S(p.inv_tiles_m),
										TTK_S(p.rows_per_batch), TTK_S(p.inv_rpb));
	else TTK_PIN_ARGS(TTK_S(p.M), TTK_S(p.W), TTK_S(p.seg[0].A), TTK_S(p.mix_full), TTK_S(p.mix_fm), TTK_S(p.inv_tiles_m));
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#ifdef TTK_STAMPS
	unsigned long long* const stamps_ = p.stamps;
#endif
	TTK_WSTAMP(stamps_, blockIdx.x, 0);
	const int b = blockIdx.x;
	if (b < p.mix_full) {      // full tiles, XCD-aware n-major order over mix_fm x 16 tiles (p.inv_tiles_m = 1 / mix_fm)
		const int tile_id = xcd_tile_id(b, p.mix_full);
		const int tn = div_recip(tile_id, p.mix_fm, p.inv_tiles_m);
		gemm_tile<T, 128, 64, 2, 2, TTK_ROLE_STAGES, ROLE>(p, (tile_id - tn * p.mix_fm) * 128, tn * 64, wave);
	} else {
		// half-height tiles of the remaining rows: j = row block * 16 + (n-tile & 1) * 8 + XCD, n-tile = 2 * XCD + (n-tile & 1) -- the XCD whose L2 holds that weight slice
		// (64 x 32 tiles on ONE wave each, over 64 CUs, were tried as well: a lone wave's k-loop is slower than the full tile beside it -- 116.0 against 114.5 us per
		// layer, 130.0 against 128.3 ms per loop; profiles/r04_ddim_chain_mixed_quarter.log)
		// HARDWARE RELIANCE: waves 2 and 3 end here while waves 0 and 1 go on to execute s_barrier in every k-step.  HIP leaves a barrier reached by part
		// of a workgroup undefined; on gfx950 a wave that has ENDED leaves the workgroup's barrier count (s_endpgm decrements it), so the two remaining waves
		// synchronise among themselves.  That is what this branch stands on -- pinned by tests/test_gpu_gemm_roles.py at T = 1216 (48 half tiles, bit-identical to
		// the generic kernel) and by every T = 1088 test of the DDIM loop (16 half tiles per launch).  A port to another target must keep the surplus waves alive instead.
		if (wave >= 2) return;
		const int j = b - p.mix_full;
		gemm_tile<T, 64, 64, 1, 2, TTK_ROLE_STAGES, ROLE>(p, p.mix_fm * 128 + (j >> 4) * 64, (2 * (j & 7) + ((j >> 3) & 1)) * 64, wave);
	}
}

// More than 64 KiB of dynamic LDS needs the opt-in, once per kernel.  `done` is a function-static flag of the launcher instantiation, process-wide: assumes ONE
// device per process (this design: one process per GPU); a second device in the same process would need the attribute set again.
static void opt_in_lds_once(bool& done, const void* kernel, int lds) {
	if (done) return;
	if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
	done = true;
}
// the GemmParams fields the host derives for the kernels (reciprocals for div_recip), filled per launch
static void fill_derived(GemmParams& p, int tiles_m) {
	p.tiles_m = tiles_m;
	p.inv_tiles_m = 1.0f / (float)tiles_m;
	p.inv_rpb = p.rows_per_batch > 0 ? 1.0f / (float)p.rows_per_batch : 0.f;
	p.inv_gn_T = p.gn_T > 0 ? 1.0f / (float)p.gn_T : 0.f;
}

template <typename T, int BM, int BN, int NWM, int NWN, int NSTAGE, int ROLE = GR_NONE, bool LONGK = false>
static void launch_tile(const GemmParams& p_in, hipStream_t s, hipEvent_t ea, hipEvent_t eb) {
	constexpr int LDS = NSTAGE * (BM + BN) * 128;
	// the generic 64 x 64-wave-block tile: the half-tile hand-ordered loop when the k-loop is longer than the ring
	if constexpr (!LONGK && ROLE == GR_NONE && sizeof(T) == 2 && BM == 256 && BN == 128 && NSTAGE == 3) {
		if (TTK_GEMM_PIPE_H && (p_in.K / 64) * p_in.nseg > NSTAGE) return launch_tile<T, BM, BN, NWM, NWN, NSTAGE, ROLE, true>(p_in, s, ea, eb);
	}
	static bool attr_set = false;
	opt_in_lds_once(attr_set, (const void*)k_gemm<T, BM, BN, NWM, NWN, NSTAGE, ROLE, LONGK>, LDS);
	GemmParams p = p_in;
	fill_derived(p, (p.M + BM - 1) / BM);
	const int grid = p.tiles_m * ((p.N + BN - 1) / BN);
	hipExtLaunchKernelGGL((k_gemm<T, BM, BN, NWM, NWN, NSTAGE, ROLE, LONGK>), dim3(grid), dim3(64 * NWM * NWN), (unsigned)LDS, s, ea, eb, 0, p);
}

// see k_gemm_mixed: tile rows [0, fm) as full 128 x 64 tiles (fm x 16 = 256 of them), the remaining M - 128 fm rows as 64 x 64 tiles
static int g_mixed_mode = -1;      // TTK_GEMM_MIXED=0 switches the mixed grid off (A/B runs); read again at handle creation
static bool mixed_grid_applies(const GemmParams& p) {
	if (g_mixed_mode < 0) { const char* e = getenv("TTK_GEMM_MIXED"); g_mixed_mode = e ? atoi(e) : 1; }
	if (!g_mixed_mode || p.N != 1024 || p.M % 64 != 0) return false;
	const int tiles_m = (p.M + 127) / 128;
	return tiles_m * 16 > 256 && tiles_m * 16 <= 320;      // 2048 < M <= 2560: at most 64 full tiles' worth of surplus rows
}
template <typename T, int ROLE>
static void launch_mixed(const GemmParams& p_in, hipStream_t s, hipEvent_t ea, hipEvent_t eb) {
	constexpr int LDS = TTK_ROLE_STAGES * (128 + 64) * 128;
	static_assert(LDS > 64 * 1024, "the mixed grid's ring needs the LDS opt-in");
	static bool attr_set = false;
	opt_in_lds_once(attr_set, (const void*)k_gemm_mixed<T, ROLE>, LDS);
	GemmParams p = p_in;
	p.mix_fm = 16; p.mix_full = 256;
	fill_derived(p, p.mix_fm);
	const int blocks64 = (p.M - 128 * p.mix_fm) / 64;
	hipExtLaunchKernelGGL((k_gemm_mixed<T, ROLE>), dim3(p.mix_full + blocks64 * 16), dim3(256), (unsigned)LDS, s, ea, eb, 0, p);
}

// The role of a launch, or GR_NONE: every field a role fixes at compile time must have exactly that value (TTK_GEMM_ROLE=0 switches the roles off: A/B runs and
// the test that the specialised kernels give the generic kernel's bits; read again by gemm_roles_refresh at every handle creation).
int g_gemm_roles = -1;
void gemm_roles_refresh() {      // 0 = off, 1 = all, else a bit mask of GemmRole values
	g_mixed_mode = -1;
	const char* e = getenv("TTK_GEMM_ROLE");
	g_gemm_roles = e ? (atoi(e) == 1 ? 0x1E : atoi(e)) : 0x1E;
}
static int gemm_role_of_unmasked(const GemmParams& p, int es);
static int gemm_role_of(const GemmParams& p, int es) {
	const int r = gemm_role_of_unmasked(p, es);
	return (g_gemm_roles >> r) & 1 ? r : GR_NONE;
}
static int gemm_role_of_unmasked(const GemmParams& p, int es) {
	if (g_gemm_roles < 0) gemm_roles_refresh();
	// (fp8 operands, es == 1: the same roles with the weights' tensor scale in the epilogue; 16-bit launches carry no scale)
	if ((es != 2 && es != 1) || p.K != GR_K || p.ldw != GR_K || !p.bias || p.act != ACT_NONE || (es == 2) != (p.out_scale == 0.f)) return GR_NONE;
	if (p.transpose_out || p.m_major) return GR_NONE;
	if (p.M < 1 || p.M > (1 << 19) || p.seg[0].lda != GR_K || p.seg[0].w_off != 0) return GR_NONE;      // 32-bit byte offsets and M * N < 2^30 element indices
	if (p.nseg == 1 && p.seg[0].shift == 0) {
		if (p.N == 3072 && !p.out_f32 && p.ldc == 3072 && !p.residual && !p.gn_part) return GR_QKV;
		if (p.N == 1024 && p.out_f32 && p.ldc == 1024 && p.gn_part && p.gn_T > 0) return !p.residual ? GR_IN1x1 : (p.ldr == 1024 ? GR_PROJ_RES : GR_NONE);
		return GR_NONE;
	}
	if (p.nseg == 3 && p.N == 1024 && p.out_f32 && p.ldc == 1024 && p.residual && p.ldr == 1024 && p.gn_part && p.gn_T > 0 && p.rows_per_batch > 0) {
		for (int j = 0; j < 3; ++j)
			if (p.seg[j].A != p.seg[0].A || p.seg[j].lda != GR_K || p.seg[j].shift != j - 1 || p.seg[j].w_off != (int64_t)j * 1024 * GR_K) return GR_NONE;
		return GR_CONV3_RES;
	}
	return GR_NONE;
}
// the role ladder, written once: f(std::integral_constant<int, role>) when `role` is one of the three 1024-wide statistics roles
static bool is_stat_role(int role) { return role == GR_IN1x1 || role == GR_CONV3_RES || role == GR_PROJ_RES; }
template <typename F> static void with_stat_role(int role, F&& f) {
	if (role == GR_IN1x1) f(std::integral_constant<int, GR_IN1x1>{});
	else if (role == GR_CONV3_RES) f(std::integral_constant<int, GR_CONV3_RES>{});
	else if (role == GR_PROJ_RES) f(std::integral_constant<int, GR_PROJ_RES>{});
}
template <typename T, int BM, int BN, int NWM, int NWN, int NSTAGE>
static void launch_tile_role(int role, const GemmParams& p, hipStream_t s, hipEvent_t ea, hipEvent_t eb) {
	if constexpr (sizeof(T) <= 2) {
		if constexpr (BM == 128 && BN == 64) {      // a few tiles more than CUs: the surplus rows as half-height tiles (k_gemm_mixed)
			if (is_stat_role(role) && mixed_grid_applies(p)) return with_stat_role(role, [&](auto r) { launch_mixed<T, decltype(r)::value>(p, s, ea, eb); });
		}
		constexpr int NS = (BM == 128 && BN == 64 && sizeof(T) == 2) ? TTK_ROLE_STAGES : NSTAGE;
		if constexpr (BN <= 128) {      // the 1024-wide roles run 128 x 64 (one utterance), 128 x 128 or 256 x 128 tiles (longer utterances, line batches)
			if (is_stat_role(role)) return with_stat_role(role, [&](auto r) { launch_tile<T, BM, BN, NWM, NWN, NS, decltype(r)::value>(p, s, ea, eb); });
		}
		if (role == GR_QKV) return launch_tile<T, BM, BN, NWM, NWN, NS, GR_QKV>(p, s, ea, eb);
	}
	launch_tile<T, BM, BN, NWM, NWN, NSTAGE>(p, s, ea, eb);
}

int g_force_tile = -1;   // TTK_GEMM_TILE=0|1|2 (tuning only)
// read on first use by EITHER of its readers: gemm_fuses_gn_stats may be asked before the first launch (a handle deciding where its statistics come from)
static void read_force_tile() { if (g_force_tile < 0) { const char* e = getenv("TTK_GEMM_TILE"); g_force_tile = e ? atoi(e) + 100 : 99; } }
static int pick_tile(int M, int N) {
	const int t128 = ((M + 127) / 128) * ((N + 127) / 128);
	const int t12864 = ((M + 127) / 128) * ((N + 63) / 64);
	return t128 >= 256 ? 0 : (t12864 >= 128 ? 1 : 2);
}
bool gemm_fuses_gn_stats(int M, int N, int C, int T) {
	read_force_tile();
	if (g_force_tile >= 100 && g_force_tile - 100 == 2) return false;
	return C == 1024 && N == C && T % 64 == 0 && M % 64 == 0 && pick_tile(M, N) != 2;
}

// Tile choice.  Measured (tests/diag/gemm_bench.cpp): on these shapes the kernel is bound by the per-CU LDS-DMA fill rate
// (~70 GB/s from L2), so what matters is bytes staged per flop and an even spread over the 256 CUs: 128x128 x 8 waves once there
// are >= 256 such tiles (575-600 TF/s at M = 5k), else 128x64 x 4 waves with two workgroups per CU (the 2k-row diffusion GEMMs,
// 335-520 TF/s), 64x64 for tiny M.
template <typename T>
static void launch_gemm_t(const GemmParams& p, hipStream_t s, hipEvent_t ea, hipEvent_t eb) {
	read_force_tile();
	int tile;
	if (g_force_tile >= 100) tile = g_force_tile - 100;
	else {
		tile = pick_tile(p.M, p.N);
	}
	// 128 x 128 tiles that need a second, partly filled round (257..511 of them: one 96 KiB workgroup per CU) while 256 x 128 tiles fit one round: the QKV
	// GEMM of a DDIM step at T = 1088 (408 tiles -> 216).  In-kernel stamps inside the replayed chain (tests/diag/ddim_chain.cpp): the second round starts
	// 11.2 us into a 21.1 us launch; 256 x 128 x 8 waves takes 18.5 us.  (2-stage ring, two workgroups per CU: 25.6; 128 x 64: 22.9.)  Same k order per
	// output element, so the same bits.  TTK_GEMM_TILE_WIDE overrides (tuning).
	// Round 4: the same choice by ROUNDS, statistics GEMMs included.  Both tiles run one workgroup per CU (96 / 144 KiB of LDS), so a launch lasts rounds x tile time, a
	// 256 x 128 tile taking ~1.5 x a 128 x 128 one (twice the work at the 64 x 64 wave block's better LDS economy): take the wide tile when ceil(t256 / 256) x 1.5 is
	// more than a tenth below ceil(t128 / 256).  One line of T = 2176 (M = 4352, N = 1024: 272 tiles of 128 x 128 = two rounds for 6 % more than one; QKV 816 = four
	// rounds) runs 40 DDIM steps in 124.7 ms with wide tiles against 133.7 ms (tests/diag/ddim_ab.py, TTK_AB_T=2176); the benchmarked T = 1088 and the latent pass
	// choose as before.
	static const int wide = [] { const char* e = getenv("TTK_GEMM_TILE_WIDE"); return e ? atoi(e) : -2; }();
	if (g_force_tile < 100 && tile == 0) {
		const int t128 = ((p.M + 127) / 128) * ((p.N + 127) / 128), t256 = ((p.M + 255) / 256) * ((p.N + 127) / 128);
		if (wide >= 0) { if (p.N >= 3072) tile = wide; }
		else if (wide == -2 && sizeof(T) <= 2 && t128 > 256) {
			const int r128 = (t128 + 255) / 256, r256 = (t256 + 255) / 256;
			// 1.5 r256 <= 0.9 r128 (round 6: "<=" -- the wide tile runs the half-tile hand-ordered loop now; the latent pass's c_fc, 5 rounds of 128 x 128 against
			// 3 of 256 x 128, 78.9 us, is the case on the line)
			if (15 * r256 <= 9 * r128) tile = 8;
		}
	}
	const int role = gemm_role_of(p, (int)sizeof(T));
	if (tile == 0) launch_tile_role<T, 128, 128, 2, 4, 3>(role, p, s, ea, eb);       // 8 waves, wave block 64 x 32, two workgroups per CU
	else if (tile == 1) launch_tile_role<T, 128, 64, 2, 2, 3>(role, p, s, ea, eb);   // 4 waves, wave block 64 x 32, two workgroups per CU
	else if (tile == 3) launch_tile<T, 128, 128, 2, 4, 4>(p, s, ea, eb);  // as 0 with a 4-stage ring (128 KiB: one workgroup per CU)
	else if (tile == 4) launch_tile<T, 128, 64, 2, 2, 5>(p, s, ea, eb);   // as 1 with a 5-stage ring (120 KiB: one workgroup per CU)
	else if (tile == 5) launch_tile<T, 128, 64, 4, 2, 3>(p, s, ea, eb);   // as 1 with 8 waves (wave block 32 x 32): twice the waves issuing the LDS-DMA pieces
	else if (tile == 6) launch_tile<T, 128, 64, 2, 4, 3>(p, s, ea, eb);   // 8 waves, wave block 64 x 16
	else if (tile == 7) launch_tile<T, 256, 64, 4, 2, 3>(p, s, ea, eb);   // 8 waves, wave block 64 x 32, 120 KiB: one workgroup per CU
	else if (tile == 8) launch_tile_role<T, 256, 128, 4, 2, 3>(role, p, s, ea, eb);  // 8 waves, wave block 64 x 64, 144 KiB: one workgroup per CU
	else if (tile == 9) launch_tile<T, 128, 128, 2, 4, 2>(p, s, ea, eb);  // as 0 with a 2-stage ring (64 KiB: two workgroups per CU)
	// (128 x 64 as TWO waves of 64 x 64 -- a third less fragment traffic out of LDS per flop -- 158.9 ms per DDIM loop against 138.9 for tile 1 everywhere; with a
	// 4-stage ring 213.7: not kept)
	else launch_tile<T, 64, 64, 2, 2, 3>(p, s, ea, eb);
}

void launch_gemm(int dt, const GemmParams& p_in, hipStream_t s) {
	static const int order = [] { const char* e = getenv("TTK_GEMM_ORDER"); return e ? atoi(e) : 0; }();   // tuning knob, see GemmParams.m_major
	GemmParams p = p_in;
	if (order == 1) p.m_major = p.nseg == 1 && (int64_t)p.N < p.M;
	else if (order == 2) p.m_major = (int64_t)p.N * p.nseg < p.M;
	else if (order == 3) p.m_major = 1;
	// every k = 3 'same' convolution (taps -1 / 0 / +1 of ONE activation tensor) runs tap-inner, whatever its shape, epilogue or kernel: the order must be a property of the
	// convolution, not of the launch -- a sequence alone (generic kernel, separate statistics launch) and inside a ragged batch (CONV role) has to give the same bits
	p.seg_inner = p.nseg == 3 && p.seg[0].shift == -1 && p.seg[1].shift == 0 && p.seg[2].shift == 1 && p.seg[1].A == p.seg[0].A && p.seg[2].A == p.seg[0].A &&
				  p.seg[1].lda == p.seg[0].lda && p.seg[2].lda == p.seg[0].lda;
	hipEvent_t ea = nullptr, eb = nullptr;      // kernel start / stop timestamps when profiling (prof_pair)
	if (g_prof_on) prof_pair(PROF_GEMM, 2.0 * p.M * p.N * (double)p.K * p.nseg, &ea, &eb);
	if (dt == DT_FP8) launch_gemm_t<f8>(p, s, ea, eb);          // A and W are fp8-e4m3 bytes, K % 128 == 0
	else if (dt == DT_BF16) launch_gemm_t<bf16>(p, s, ea, eb);
	else if (dt == DT_F16) launch_gemm_t<f16>(p, s, ea, eb);
	else launch_gemm_t<float>(p, s, ea, eb);
}

}  // namespace ttk
