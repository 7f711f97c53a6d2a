// Host-side plumbing shared by the two handles: error reporting, device memory, weight lookup/upload/packing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ttk.h"
#include "ttk_kernels.h"

namespace ttk {

void set_error(const char* fmt, ...);

#define TTK_HIP(expr)                                                                                   \
	do {                                                                                                \
		hipError_t _e = (expr);                                                                         \
		if (_e != hipSuccess) {                                                                         \
			ttk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
			return TTK_E_HIP;                                                                           \
		}                                                                                               \
	} while (0)
#define TTK_TRY(expr)                \
	do {                             \
		int _r = (expr);             \
		if (_r != TTK_OK) return _r; \
	} while (0)
#define TTK_REQUIRE(cond, code, ...)     \
	do {                                 \
		if (!(cond)) {                   \
			ttk::set_error(__VA_ARGS__); \
			return code;                 \
		}                                \
	} while (0)

// owns every device allocation of a handle; freed with it (a handle is deleted, on the failure path of its create as well)
struct Arena {
	std::vector<void*> ptrs;
	size_t bytes = 0;
	Arena() = default;
	Arena(const Arena&) = delete;
	Arena& operator=(const Arena&) = delete;
	~Arena() { release(); }
	int alloc(void** out, size_t n) {
		if (n == 0) n = 16;
		TTK_HIP(hipMalloc(out, n));
		ptrs.push_back(*out);
		bytes += n;
		return TTK_OK;
	}
	void release() {
		for (void* p : ptrs) (void)hipFree(p);
		ptrs.clear();
	}
};

// grow-only workspace buffer
struct WsBuf {
	void* p = nullptr;
	size_t cap = 0;
	WsBuf() = default;
	WsBuf(const WsBuf&) = delete;
	WsBuf& operator=(const WsBuf&) = delete;
	~WsBuf() { release(); }
	int reserve(size_t n) {
		if (n <= cap) return TTK_OK;
		if (p) TTK_HIP(hipFree(p));
		p = nullptr; cap = 0;
		TTK_HIP(hipMalloc(&p, n));
		cap = n;
		return TTK_OK;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct WeightMap {
	std::map<std::string, const ttk_weight_view*> m;
	WeightMap(const ttk_weight_view* w, int n) { for (int i = 0; i < n; ++i) m[w[i].name] = &w[i]; }
	const ttk_weight_view* find(const std::string& k) const { auto it = m.find(k); return it == m.end() ? nullptr : it->second; }
};

inline int64_t numel(const ttk_weight_view* v) { int64_t n = 1; for (int i = 0; i < v->ndim; ++i) n *= v->shape[i]; return n; }

// f32 tensor copied to the device as is (norm scales, biases, embedding tables)
int upload_f32(Arena& ar, const WeightMap& wm, const std::string& name, int64_t expect_numel, float** out);

// a GEMM operand: T-typed [ntap][Npad][Kpad] (+ optional MFMA-fragment copy) and its f32 bias
struct Mat {
	void* w = nullptr;      // [ntap][Npad][Kpad]
	void* wfrag = nullptr;  // [Npad/16][Kpad/32][64][8], decode path only (one byte per element when w8)
	bool w8 = false;        // DT_FP8W: weights rounded to fp8-e4m3 * wscale; `w` holds them exactly in bf16, `wfrag` as fp8 bytes
	float wscale = 1.f;
	int wes = 2;            // bytes per element of `w` (1: DT_FP8, the dense GEMM reads fp8 bytes and applies wscale in its epilogue)
	float* bias = nullptr;
	int N = 0, K = 0, Npad = 0, Kpad = 0, ntap = 1;
	// decode path with the preceding LayerNorm folded in (fold_layernorm): fragment-order gamma o W, its column sums, b + beta W
	void* wfrag_fold = nullptr;
	float *csum = nullptr, *bias_fold = nullptr;
};
// layout: PK_NK / PK_KN / PK_CONV3 ; N, K are the logical sizes checked against the tensor
int upload_mat(Arena& ar, const WeightMap& wm, int dt, const std::string& wname, const std::string& bname, int layout,
			   int N, int K, bool frag, Mat* out, int ntap = 0);   // ntap: kernel size for PK_CONVK / PK_CONVT

// For a PK_KN matrix uploaded with a fragment copy: build the folded-LayerNorm operands of the decode launch (see SkinnyParams.g1) from the
// LayerNorm's gamma / beta.  fp8 weights: folded AFTER the rounding, the folded operand held in the kernel type (see the definition).
int fold_layernorm(Arena& ar, const WeightMap& wm, int dt, const std::string& wname, const std::string& bname, const std::string& gname,
				   const std::string& betaname, Mat* m);

// The launches of the two above on buffers that exist (no allocation, no synchronisation; `s` ordered): create and ttk_ar_lora_set share them.
//   pack_mat:  device f32 `src` in `layout` -> m.w and, where there is one, m.wfrag (fp8 weights: `src` is rounded already, m.wscale set)
//   pack_fold: device f32 [K][N] `w` (scaled by gamma IN PLACE) -> m.wfrag_fold, m.csum, m.bias_fold; `wt` is T-typed scratch of Npad x Kpad elements
void pack_mat(int dt, const float* src, int layout, const Mat& m, hipStream_t s);
void pack_fold(int dt, float* w, const float* gamma, const float* beta, const float* bias, void* wt, const Mat& m, hipStream_t s);

// ---- the weight-streaming launches of the decode step, each described once (ar.hip).  The handle's token step and ttk_gemv_launch (kernel tests on
// caller-provided operands) both go through decode_launch: ONE place chooses the kernel family and the waves per workgroup.
enum DecodeRole { DR_QKV = 0, DR_PROJ, DR_FC, DR_PROJ2, DR_HEAD };      // ln_1 + c_attn, c_proj + residual, ln_2 + c_fc + gelu_new, mlp.c_proj + residual, mel_head
struct DecodeLaunch {
	int role;
	const Mat* W; int N, K;
	const void* a;                   // rows, T-typed in A-fragment order: x_frag (DR_QKV / DR_FC: un-normalised, the LayerNorm is folded into W), attn_out, hbuf
	const float *ln_g, *ln_b;        // the LayerNorm in front: DR_QKV / DR_FC (used as such only without the fold), the prefill's head (ln_f)
	const float *ln2_g, *ln2_b;      // the prefill's head: final_norm behind ln_f
	float* out_f32;                  // DR_PROJ / DR_PROJ2: the residual stream, updated in place; DR_HEAD: logits
	void* out_T;                     // DR_FC: activations; DR_PROJ / DR_PROJ2 (optional): T copy of the updated rows; both in A-fragment order
	void *kc, *vc;                   // DR_QKV: this layer's caches
	bool bump;                       // DR_HEAD: the launch advances the cache length
	const float* x; int64_t ldx;     // f32 rows the LayerNorm-prologue form normalises
	float* qbuf; int* d_pos; int max_ctx, H;      // DR_QKV: scaled queries, cache row to append at, cache geometry; d_pos also DR_HEAD with bump
};
struct DecodeCtx {
	int dt;                          // arithmetic type of the kernels (DT_F32 / DT_BF16 / DT_F16)
	int lnfold, lean, model_dim;     // TTK_AR_LNFOLD, TTK_AR_LEAN, the model's width
	int* health;                     // device word of the folded launches (ttk_ar_health)
	const int64_t* rng_args; const int64_t* rng_draws; float* rng_q;      // DR_HEAD: multinomial noise (ttk_ar_set_noise)
	// kernel tests only (ttk_gemv_launch; a handle leaves both 0): family 1 = k_skinny, 2 = k_gemv instead of the choice below; waves per k_skinny workgroup
	int family, waves;
	int* launched;                   // (optional, host) receives the family that was launched: 1 = k_skinny, 2 = k_gemv
};
int skinny_waves(int role, bool ln_prologue, int dt, int d);
// One launch on M rows: k_gemv where the lean kernels are allowed and have an instantiation for the geometry, else k_skinny on the same operands.
int decode_launch(const DecodeCtx& c, const DecodeLaunch& L, int M, hipStream_t s);

// sample.hip: the fused per-token sampling launch; emb / pos / x_out non-null = also write the next decode step's input rows
int launch_sample_step(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32,
					   hipStream_t stream, const char* who);
int launch_greedy_step(const ttk_sample_args* a, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32,
					   hipStream_t stream, const char* who);
// sample_ext.hip: the same step over the reference's samplers.py (ttk_sample_ext), on a kernel of its own built from the same stages (sample_stages.h)
int launch_sample_step_ext(const ttk_sample_args* a, const ttk_sample_ext* x, const float* emb, const float* pos, float* x_out, int d, int pos_rows, void* x_frag, int x_frag_f32,
						   hipStream_t stream, const char* who);

// beam.hip: the in-place gather of the KV cache's candidate slices that beam search needs per token (ttk_ar_reorder_cache[_lines]); the B rows are lines of
// rows_per_line candidates (B: one line), and a source outside its destination's line counts as out of range
int launch_kv_reorder(void* kc, void* vc, int layers, int max_batch, int H, int max_ctx, size_t es, const int* d_pos, const int64_t* beam_idx, int B,
					  int rows_per_line, hipStream_t s, const char* who);

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace ttk
