// Dense GEMM (gemm.hip): build knobs and the asm primitives of the k-loops.
#pragma once

#include <type_traits>

#include "ttk_common.h"
#include "ttk_kernels.h"

// ------------------------------------------------------------------------------------------------ build knobs (-DTTK_...=n: tuning and A/B builds)
#ifndef TTK_GEMM_PIPE
#define TTK_GEMM_PIPE 1            // 0: no hand-ordered k-loop for wave blocks up to 64 x 32 (gemm_tile, PIPE); the compiler-ordered loop runs instead
#endif
#ifndef TTK_GEMM_PIPE_H
#define TTK_GEMM_PIPE_H 1          // 0: no half-tile hand-ordered loop for 64 x 64 wave blocks (gemm_tile, PIPE_H)
#endif
#ifndef TTK_CONV_IMAGE
#define TTK_CONV_IMAGE 1           // 0: the k = 3 residual role stages its taps through the ring instead of a shared activation image (conv3_image_tile)
#endif
#ifndef TTK_ROLE_STAGES
#define TTK_ROLE_STAGES 3          // ring depth of the 128 x 64 role tiles
#endif
#ifndef TTK_FP8_SCALED_MFMA
#define TTK_FP8_SCALED_MFMA 1      // 0: the non-scaled 16x16x32 fp8 MFMA
#endif
// placement inside a hand-ordered k-step; gaps are counted in MFMAs of the step, 0 = behind the first one
#ifndef TTK_PIPE_RPG
#define TTK_PIPE_RPG 2             // fragment reads per MFMA gap
#endif
#ifndef TTK_PIPE_PREB
#define TTK_PIPE_PREB 0            // MFMAs issued in front of the step's barrier (reads start behind it)
#endif
#ifndef TTK_PIPE_DPG
#define TTK_PIPE_DPG 1             // DMA pieces per MFMA gap
#endif
#ifndef TTK_PIPE_DLATE
#define TTK_PIPE_DLATE 0           // 1: the DMA pieces fill the LAST gaps of the step; 0: they start TTK_PIPE_D0 gaps behind the barrier (or as late as still fits)
#endif
#ifndef TTK_PIPE_D0
#define TTK_PIPE_D0 6              // first MFMA gap behind the barrier that carries a DMA piece (with TTK_PIPE_DLATE=0)
#endif
// (profiles/r06_chain_pipe_knobs.log, per layer of the replayed chain on hashed operands: 1 read per gap + pieces last 113.1 us; pieces first 113.9; 2 reads per gap 111.1;
//  2 reads per gap + pieces from gap 6 111.6 with the shortest launch spans; 2 MFMAs in front of the barrier 112.8; 2 pieces per gap 114.2 -- the compiler-ordered loop 117.3)

// the stamp buffer of a diagnostic build (GemmParams has the field only there; TTK_WSTAMP drops its arguments in the product build)
#ifdef TTK_STAMPS
#define TTK_GEMM_STAMPS(p) ((p).stamps)
#else
#define TTK_GEMM_STAMPS(p) ((unsigned long long*)nullptr)
#endif

namespace ttk {

// One LDS-DMA piece: 64 lanes x 16 B from buffer offsets (per-lane voff + scalar soff) to LDS bytes [lds_dst, lds_dst + 1024).
// Issued from inline asm on purpose: hipcc's waitcnt pass would otherwise put `s_waitcnt vmcnt(0)` in front of the first ds_read
// of every k-step (it cannot prove that the ring stage being read is not the one being filled) and serialise the ring; hidden
// from it, the only vmcnt waits in the k-loop are the counted ones below (cdna_hip_programming.md section 5.7, items 1-2).
// M0 carries the LDS base; it is compiler-reserved, so it is saved and restored inside the statement.
__device__ __forceinline__ void glds16(unsigned voff, __amdgpu_buffer_rsrc_t srd, unsigned soff, unsigned lds_dst /* wave-uniform */) {
	unsigned keep;
	asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
				 : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(srd), "s"(soff) : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
	return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
	if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// ------------------------------------------------------------------------------------------------ hand-ordered k-loops (16-bit operands): the statements they are made of
// What the compiler made of the C++ ping-pong (profiles/r06_gemm_kloop_isa_*_before.txt): `cur` and `nxt` in the SAME registers, the next tile's 12 ds_read_b128
// sunk behind MFMA 9-16 and drained by lgkmcnt(0) in front of every barrier, all six DMA issues in front of MFMA 1 -- the measured "sum, not maximum" (VERDICT r05
// weak #3).  Here the fragment reads, the DMA pieces and the waits are `asm volatile` statements (invisible to the waitcnt pass, like glds16), the MFMAs stay
// builtins (the compiler knows the matrix pipe's write-back hazards: an all-asm first version let it copy accumulators between two loop bodies with no wait
// states -- 5e-2 errors), and a full scheduling fence (`sched_barrier(0)`) behind every statement pins the order written in the loops: the source order IS the
// instruction stream.  The compiler still allocates the registers (two real fragment sets).  What stays ours: a read's data is used only behind the
// `s_waitcnt lgkmcnt(0)` that ends the step it was issued in (any copy the register allocator might add at a loop edge lands behind that wait too), and M0 (below).
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
#define TTK_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int OFF> __device__ __forceinline__ void pipe_read16(u32x4& d, unsigned addr) {
	static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
	asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
	TTK_FENCE();
}
template <typename T> __device__ __forceinline__ void pipe_mfma(f32x4& c, const u32x4& a, const u32x4& b) {
	union U { u32x4 q; typename Frag<T>::type v; __device__ U() {} } ua, ub;
	ua.q = a; ub.q = b;
	c = mma16<T>(ua.v, ub.v, c);
	TTK_FENCE();
}
__device__ __forceinline__ void pipe_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); TTK_FENCE(); }
// the raw workgroup barrier of a hand-ordered step (the counted vmcnt wait in front of it is the caller's)
__device__ __forceinline__ void pipe_barrier() { TTK_FENCE(); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); TTK_FENCE(); }
// M0 INVARIANT of the hand-ordered loops.  pipe_glds16 writes M0 (the LDS base of the piece) and neither restores nor declares it: a clobber of the reserved
// register is rejected by the compiler ("may lead to undefined behaviour"), and a save / restore per piece is two scalar moves in every MFMA gap.  Instead the
// whole loop is bracketed -- pipe_begin() saves M0 in front of the first piece, pipe_end() restores it behind the last (gemm_tile's PIPE loop: pipe_m0_save / pipe_m0_restore,
// see there) -- and correctness rests on the compiler having no M0 use of its own in between.  tests/test_gemm_resources.py holds it to that: in the built code
// object every instruction of a GEMM kernel that names m0 is one of these scalar moves.
__device__ __forceinline__ void pipe_glds16(unsigned voff, __amdgpu_buffer_rsrc_t srd, unsigned soff, unsigned lds_dst /* wave-uniform */) {
	asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(lds_dst), "v"(voff), "s"(srd), "s"(soff) : "memory");
	TTK_FENCE();
}
// k-loop clock of a -DTTK_CLOCK_STAMPS build: shader cycles and 100 MHz ticks of this wave's steady state into stamp slot 6 (MI355X_MICROARCH.md, DVFS give-back item 6)
#ifdef TTK_CLOCK_STAMPS
struct KClock { unsigned long long clk0, rt0; };
__device__ __forceinline__ KClock kclock_start() { return KClock{__builtin_amdgcn_s_memtime(), __builtin_amdgcn_s_memrealtime()}; }
__device__ __forceinline__ void kclock_stop(const KClock& c, unsigned long long* stamps, int lane) {
	if (stamps && lane == 0) {
		unsigned long long* st_ = stamps + ((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 8;
		st_[6] = ((__builtin_amdgcn_s_memtime() - c.clk0) << 32) | ((__builtin_amdgcn_s_memrealtime() - c.rt0) & 0xffffffffull);
	}
}
#else
struct KClock {};
__device__ __forceinline__ KClock kclock_start() { return KClock{}; }
__device__ __forceinline__ void kclock_stop(const KClock&, unsigned long long*, int) {}
#endif
__device__ __forceinline__ unsigned pipe_m0_save() { unsigned k; asm volatile("s_mov_b32 %0, m0" : "=s"(k)); TTK_FENCE(); return k; }
__device__ __forceinline__ void pipe_m0_restore(unsigned k) { asm volatile("s_mov_b32 m0, %0" :: "s"(k)); TTK_FENCE(); }
struct PipeScope { unsigned m0_keep; KClock clk; };
__device__ __forceinline__ PipeScope pipe_begin() {
	PipeScope s;
	asm volatile("s_mov_b32 %0, m0" : "=s"(s.m0_keep));
	TTK_FENCE();
	return s;
}
__device__ __forceinline__ void pipe_end(const PipeScope& s, unsigned long long* stamps, int lane) {
	asm volatile("s_mov_b32 m0, %0" :: "s"(s.m0_keep));
	TTK_FENCE();
	kclock_stop(s.clk, stamps, lane);
}

}  // namespace ttk
