// Run-time LoRA: W' = W0 + (B A) s for one HF Conv1D weight of a ttk_ar handle (ttk_ar_lora_set, ar.hip).
//   W0 [K][N] f32 row-major: the handle's resident master; lora_B [K][rank]; lora_A [rank][N]; s = alpha / rank.
//   out [K][N] f32: what launch_pack_nk(.., PK_KN, ..) reads, i.e. the matrix a fresh handle would have been created from.
// Reference: models/lora.py:120-123 (ParameterizedLoRA.forward) with from_conv1d's swapped shapes (:136-145).
//
// The arithmetic is part of the interface ("Run-time LoRA"): per element acc = 0, then in rising r
//   acc = fadd(acc, fmul(B[k][r], A[r][n])),  W' = fadd(W0, fmul(acc, s)),
// every product and sum rounded on its own in f32.  A numpy f32 loop gives the same bits (tests/lora_ref.py), so a switched handle is compared
// bit for bit with one created from weights folded on the host.  Hence no MFMA and no FMA here: both round once per product-sum.
#include "ttk_common.h"
#include "ttk_kernels.h"

namespace ttk {

namespace {

constexpr int LT = 64;      // output tile: LT k-rows x LT n-columns per 256-thread workgroup, 4 x 4 elements per thread
constexpr int LR = 32;      // rank strip staged through LDS at a time

// hipcc contracts a * b + c into an FMA by default, __fmul_rn / __fadd_rn included (they are plain operators in its headers): these two are not
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
	return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
	return a + b;
}

__global__ __launch_bounds__(256) void k_lora_update(const float* __restrict__ W0, const float* __restrict__ Bm, const float* __restrict__ Am, int K, int N, int rank,
														 float s, float* __restrict__ out) {
	// Bs[r][k] (the strip transposed; rows padded by one word so that the 32 r of one k land on 32 banks), As[r][n]
	__shared__ float Bs[LR][LT + 1];
	__shared__ __attribute__((aligned(16))) float As[LR][LT];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int k0 = blockIdx.y * LT, n0 = blockIdx.x * LT;
	float acc[4][4];
#pragma unroll
	for (int i = 0; i < 4; ++i)
#pragma unroll
		for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
	for (int r0 = 0; r0 < rank; r0 += LR) {
		const int rc = rank - r0 < LR ? rank - r0 : LR;
#pragma unroll
		for (int i = 0; i < LT * LR / 256; ++i) {
			const int idx = tid + i * 256;
			const int kk = idx / LR, rr = idx % LR;      // B rows are rank-contiguous: 32 lanes read one row's strip
			Bs[rr][kk] = (k0 + kk < K && rr < rc) ? Bm[(int64_t)(k0 + kk) * rank + r0 + rr] : 0.f;
			const int ar = idx / LT, an = idx % LT;
			As[ar][an] = (n0 + an < N && ar < rc) ? Am[(int64_t)(r0 + ar) * N + n0 + an] : 0.f;
		}
		__syncthreads();
		for (int r = 0; r < rc; ++r) {      // rising r: the order is the contract
			const float4 a4 = *(const float4*)&As[r][4 * tx];
			const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const float b = Bs[r][4 * ty + i];
#pragma unroll
				for (int j = 0; j < 4; ++j) acc[i][j] = add_rn(acc[i][j], mul_rn(b, a[j]));
			}
		}
		__syncthreads();
	}
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int k = k0 + 4 * ty + i;
		if (k >= K) continue;
		const int n = n0 + 4 * tx;
		const int64_t o = (int64_t)k * N + n;
		if ((N & 3) == 0 && n + 3 < N) {      // rows start on 16 bytes: one request per thread and row
			const float4 w = *(const float4*)(W0 + o);
			float4 v;
			v.x = add_rn(w.x, mul_rn(acc[i][0], s)); v.y = add_rn(w.y, mul_rn(acc[i][1], s));
			v.z = add_rn(w.z, mul_rn(acc[i][2], s)); v.w = add_rn(w.w, mul_rn(acc[i][3], s));
			*(float4*)(out + o) = v;
		} else {
#pragma unroll
			for (int j = 0; j < 4; ++j)
				if (n + j < N) out[o + j] = add_rn(W0[o + j], mul_rn(acc[i][j], s));
		}
	}
}

}  // namespace

void launch_lora_update(const float* W0, const float* lora_B, const float* lora_A, int K, int N, int rank, float s, float* out, hipStream_t stream) {
	const dim3 grid((N + LT - 1) / LT, (K + LT - 1) / LT);
	hipLaunchKernelGGL(k_lora_update, grid, dim3(256), 0, stream, W0, lora_B, lora_A, K, N, rank, s, out);
}

}  // namespace ttk
