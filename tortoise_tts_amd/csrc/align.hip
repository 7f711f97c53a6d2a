// Attention maps of the teacher-forced GPT-2 pass and the text-to-audio alignment built on them (head_dim 64), for gfx950.
//
// k_attn_probs   : the causal softmax probabilities P[q][k] = softmax_{k <= q}(scale q.k) that k_attn_fwd (attn.hip) never materialises --
//                  what HF's eager attention returns with output_attentions (HF:models/gpt2/modeling_gpt2.py:144-226, reached through
//                  /root/reference/tortoise_tts/models/unified_voice.py:508-516, get_logits(get_attns=True)).  f32 output whatever T is.
// k_align_prepare: steps 1-4 of the alignment recipe (standardise over the text axis, median filter along the mel axis, mean over heads, negate):
//                  OpenAI Whisper's word-timestamp recipe with mel codes as the time axis.  No reference counterpart.
// k_dtw          : the dynamic-time-warping cost table and its one-byte trace, one workgroup per sequence walking the anti-diagonals.
#include "ttk_common.h"
#include "ttk_host.h"

namespace ttk {

namespace {
constexpr float PROBS_LOG2E = 1.4426950408889634f;
constexpr float PROBS_NEG_BIG = -1e30f;
}

// One wave owns the 16-query tile qt of one (sequence, selected head); four independent waves per workgroup, no LDS, no barrier.
// S^T = K Q^T as in k_attn_fwd: the K fragment is the A operand (lane li = key row of the tile), the scaled Q fragment the B operand (lane li = query
// column), so lane (li, g) holds the scores of query q0 + li against keys 16 kt + 4 g + r, r = 0..3 -- four consecutive floats of one output row.
// Pass 1, key tiles 0 .. qt: per lane a reference point m (an INTEGER: ceil of the largest log2-domain score seen) and the sum l of exp2(v - m).  A
//   rise of m rescales l by a power of two (v_ldexp_f32): exact, so l carries the roundings of its adds only -- one add per key tile and a two-level
//   tree inside a tile; the four lanes of a query are merged the same way (max, ldexp, two fold adds).
// Pass 2 recomputes the scores of the key tiles that meet the window's columns and stores exp2(v - m) / l, zeros above the diagonal.
// The full map is the window (0, T, 0, T): one code path, so a window's elements are bit for bit the full map's.
template <typename T>
__global__ __launch_bounds__(256) void k_attn_probs(AttnProbsParams p) {
#pragma clang fp contract(off)
	typedef typename Frag<T>::type FragT;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
	const int b = blockIdx.z, sel = blockIdx.y;
	const int h = p.heads[sel], slot = p.slots ? p.slots[sel] : sel;
	if ((unsigned)h >= (unsigned)p.H || (unsigned)slot >= (unsigned)p.n_out) return;      // a bad list entry writes and reads nothing
	const int qt = p.r0 / 16 + blockIdx.x * 4 + wave, q0 = 16 * qt;
	const int r1 = p.r0 + p.R, c1 = p.c0 + p.C;
	if (q0 >= r1) return;      // wave-uniform
	const T* base = (const T*)p.qkv + (int64_t)b * p.T * p.ld;
	const int qc = p.q_off + h * p.head_stride, kc = p.k_off + h * p.head_stride;
	const int qi = q0 + li;
	const int qrow = qi < p.T ? qi : p.T - 1;      // rows past the sequence repeat its last one; they are never stored

	auto load_q = [&](int ks) -> FragT {
		const FragT f = *(const FragT*)(base + (int64_t)qrow * p.ld + qc + 32 * ks + 8 * g);
		FragT o;
#pragma unroll
		for (int j = 0; j < 8; ++j) o[j] = cvt<T>((float)f[j] * p.scale);
		return o;
	};
	const FragT qf0 = load_q(0), qf1 = load_q(1);
	auto scores = [&](int kt) -> f32x4 {
		int krow = 16 * kt + li;
		krow = krow < p.T ? krow : p.T - 1;
		const T* kp = base + (int64_t)krow * p.ld + kc + 8 * g;
		const FragT k0 = *(const FragT*)kp, k1 = *(const FragT*)(kp + 32);
		f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
		s = mma16<T>(k0, qf0, s);
		s = mma16<T>(k1, qf1, s);
		return s;
	};

	// ---- pass 1
	float m = PROBS_NEG_BIG, l = 0.f;
	for (int kt = 0; kt <= qt; ++kt) {
		const f32x4 s = scores(kt);
		float v[4], tmax = PROBS_NEG_BIG;
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int key = 16 * kt + 4 * g + r;
			v[r] = key <= qi ? s[r] * PROBS_LOG2E : PROBS_NEG_BIG;
			tmax = fmaxf(tmax, v[r]);
		}
		const float m_new = fmaxf(m, ceilf(tmax));
		l = ldexpf(l, (int)fmaxf(m - m_new, -200.f));      // (l is 0 while m is still the start value; 2^-200 of an old sum is nothing beside a new term >= 1/2)
		m = m_new;
		float pr[4];
#pragma unroll
		for (int r = 0; r < 4; ++r) pr[r] = 16 * kt + 4 * g + r <= qi ? __builtin_amdgcn_exp2f(v[r] - m) : 0.f;
		l += (pr[0] + pr[1]) + (pr[2] + pr[3]);
	}
	const float mq = fold32_max(fold16_max(m));
	l = ldexpf(l, (int)fmaxf(m - mq, -200.f));
	l = fold32_add(fold16_add(l));
	const float inv = 1.0f / l;

	// ---- pass 2
	const bool row_ok = qi >= p.r0 && qi < r1;
	const int64_t orow = row_ok ? (((int64_t)b * p.n_out + slot) * p.R + (qi - p.r0)) * p.C : 0;
	const int kt_hi = (c1 - 1) / 16;
	for (int kt = p.c0 / 16; kt <= kt_hi; ++kt) {
		float pr[4] = {0.f, 0.f, 0.f, 0.f};
		if (kt <= qt) {
			const f32x4 s = scores(kt);
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int key = 16 * kt + 4 * g + r;
				const float vr = s[r] * PROBS_LOG2E;
				pr[r] = key <= qi ? __builtin_amdgcn_exp2f(vr - mq) * inv : 0.f;
			}
		}
		if (row_ok) {
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int key = 16 * kt + 4 * g + r;
				if (key >= p.c0 && key < c1) p.out[orow + (key - p.c0)] = pr[r];
			}
		}
	}
}

void launch_attn_probs(int dt, const AttnProbsParams& p, hipStream_t s) {
	if (p.n_sel <= 0) return;      // a layer without a selected head launches nothing
	const int tiles = (p.r0 + p.R - 1) / 16 - p.r0 / 16 + 1;
	const dim3 grid((tiles + 3) / 4, p.n_sel, p.nb);
	by_dtype(dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k_attn_probs<T>), grid, dim3(256), 0, s, p); });
}

// ------------------------------------------------------------------------------------------------ standardise, median, mean, negate
// One workgroup per (sequence, mel row m), threads over the text axis.  Per head: the 2 pad + 1 rows of the filter window (reflect padding) get their
// mean and population std from one wave each (two passes: sum, then sum of squared differences), then every thread standardises its column of those
// rows, sorts them (odd-even transposition of 15 register values, unused ones +inf) and adds the median to its running sum over the heads.
// M <= width / 2 has no reflect padding: the filter is then the identity (as Whisper's median_filter returns its input).
constexpr int ALIGN_MAX_WIDTH = 15;
__global__ __launch_bounds__(256) void k_align_prepare(const float* A, int n_sel, int M, int Tt, int width, float* cost, float* matrix) {
#pragma clang fp contract(off)
	const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int pad = M > width / 2 ? width / 2 : 0, w = 2 * pad + 1;
	__shared__ float st_mean[ALIGN_MAX_WIDTH], st_sd[ALIGN_MAX_WIDTH];
	__shared__ int st_row[ALIGN_MAX_WIDTH];
	float acc[2] = {0.f, 0.f};      // columns tid and tid + 256 (Tt <= 512: the launcher's check)
	for (int hs = 0; hs < n_sel; ++hs) {
		const float* Ah = A + ((int64_t)b * n_sel + hs) * M * Tt;
		__syncthreads();      // the previous head's statistics have been read
		for (int j = wave; j < w; j += 4) {
			int mj = m - pad + j;
			mj = mj < 0 ? -mj : (mj >= M ? 2 * (M - 1) - mj : mj);
			const float* row = Ah + (int64_t)mj * Tt;
			float sum = 0.f;
			for (int t = lane; t < Tt; t += 64) sum += row[t];
			const float mean = wave_sum(sum) / (float)Tt;
			float ss = 0.f;
			for (int t = lane; t < Tt; t += 64) { const float d = row[t] - mean; ss += d * d; }
			const float sd = sqrtf(wave_sum(ss) / (float)Tt);
			if (lane == 0) { st_mean[j] = mean; st_sd[j] = sd; st_row[j] = mj; }
		}
		__syncthreads();
#pragma unroll
		for (int c = 0; c < 2; ++c) {
			const int t = tid + 256 * c;
			if (t >= Tt) continue;
			float v[ALIGN_MAX_WIDTH];
#pragma unroll
			for (int j = 0; j < ALIGN_MAX_WIDTH; ++j) {
				v[j] = __builtin_inff();
				if (j < w) { const float sd = st_sd[j]; v[j] = sd > 0.f ? (Ah[(int64_t)st_row[j] * Tt + t] - st_mean[j]) / sd : 0.f; }
			}
#pragma unroll
			for (int round = 0; round < ALIGN_MAX_WIDTH; ++round)
#pragma unroll
				for (int j = round & 1; j + 1 < ALIGN_MAX_WIDTH; j += 2) { const float lo = fminf(v[j], v[j + 1]), hi = fmaxf(v[j], v[j + 1]); v[j] = lo; v[j + 1] = hi; }
			float med = v[0];
#pragma unroll
			for (int j = 1; j <= ALIGN_MAX_WIDTH / 2; ++j) med = j == pad ? v[j] : med;
			acc[c] += med;
		}
	}
#pragma unroll
	for (int c = 0; c < 2; ++c) {
		const int t = tid + 256 * c;
		if (t >= Tt) continue;
		const float mean = acc[c] / (float)n_sel;
		const int64_t o = ((int64_t)b * M + m) * Tt + t;
		cost[o] = -mean;
		if (matrix) matrix[o] = mean;
	}
}

void launch_align_prepare(const float* A, int nb, int n_sel, int M, int Tt, int width, float* cost, float* matrix, hipStream_t s) {
	hipLaunchKernelGGL(k_align_prepare, dim3(M, nb), dim3(256), 0, s, A, n_sel, M, Tt, width, cost, matrix);
}

// ------------------------------------------------------------------------------------------------ DTW
// D[0][0] = 0, borders +inf, D[i][j] = cost[i-1][j-1] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]); on ties the first of (diagonal, mel row - 1, text
// column - 1) wins: trace 0 / 1 / 2.  The cells of anti-diagonal i + j = d depend on diagonals d - 1 and d - 2 only: one barrier per diagonal, every
// loop bound a function of M and Tt alone.
__global__ __launch_bounds__(512) void k_dtw(const float* cost, int M, int Tt, float* Dws, unsigned char* trace, float* total) {
	const int b = blockIdx.x, tid = threadIdx.x, W = Tt + 1;
	float* D = Dws + (int64_t)b * (M + 1) * W;
	cost += (int64_t)b * M * Tt;
	trace += (int64_t)b * M * Tt;
	const float inf = __builtin_inff();
	for (int i = tid; i <= M; i += 512) D[i * W] = i == 0 ? 0.f : inf;
	for (int j = 1 + tid; j <= Tt; j += 512) D[j] = inf;
	__syncthreads();
	for (int d = 2; d <= M + Tt; ++d) {
		const int ilo = d - Tt > 1 ? d - Tt : 1, ihi = d - 1 < M ? d - 1 : M;
		for (int i = ilo + tid; i <= ihi; i += 512) {
			const int j = d - i;
			const float c0 = D[(i - 1) * W + j - 1], c1 = D[(i - 1) * W + j], c2 = D[i * W + j - 1];
			float best; unsigned char tr;
			if (c0 <= c1 && c0 <= c2) { best = c0; tr = 0; }
			else if (c1 <= c2) { best = c1; tr = 1; }
			else { best = c2; tr = 2; }
			D[i * W + j] = cost[(i - 1) * Tt + j - 1] + best;
			trace[(i - 1) * Tt + j - 1] = tr;
		}
		__syncthreads();
	}
	if (tid == 0) total[b] = D[M * W + Tt];
}

void launch_dtw(const float* cost, int nb, int M, int Tt, float* D, unsigned char* trace, float* total, hipStream_t s) {
	hipLaunchKernelGGL(k_dtw, dim3(nb), dim3(512), 0, s, cost, M, Tt, D, trace, total);
}

const char* align_shape_refusal(int nb, int M, int Tt) {
	if (nb < 1 || nb > 65535) return "the batch must hold 1..65535 sequences";
	if (M < 1 || M > ALIGN_MAX_M) return "M must lie in 1..606 (max_mel_tokens + 2 of the largest configuration)";
	if (Tt < 1 || Tt > ALIGN_MAX_TT) return "Tt must lie in 1..404 (max_text_tokens + 2 of the largest configuration)";
	return nullptr;
}

}  // namespace ttk

using namespace ttk;

static_assert(sizeof(ttk_attn_probs_desc) == 80, "ttk_attn_probs_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_attn_probs(int dtype, const ttk_attn_probs_desc* d, void* stream) {
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_attn_probs: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16, TTK_E_ARG, "ttk_attn_probs: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", dtype);
	const int epc = dtype == TTK_F32 ? 4 : 8;      // elements per 16 bytes: every fragment is read as whole 16-byte words
	TTK_REQUIRE(d->qkv && d->out && (d->heads || d->n_sel == 0), TTK_E_ARG, "ttk_attn_probs: null qkv, out or heads");
	TTK_REQUIRE(d->T >= 1 && d->nb >= 1 && d->nb <= 65535 && d->H >= 1 && d->n_sel >= 0 && d->n_sel <= 65535, TTK_E_ARG,
				"ttk_attn_probs: need T >= 1, 1 <= nb <= 65535, H >= 1, 0 <= n_sel <= 65535 (got T=%d nb=%d H=%d n_sel=%d)", d->T, d->nb, d->H, d->n_sel);
	TTK_REQUIRE(((uintptr_t)d->qkv & 15) == 0 && d->ld > 0 && d->ld % epc == 0 && d->q_off >= 0 && d->k_off >= 0 && d->head_stride >= 0 && d->q_off % epc == 0 &&
				d->k_off % epc == 0 && d->head_stride % epc == 0, TTK_E_ARG,
				"ttk_attn_probs: qkv must be 16-byte aligned, ld, q_off, k_off and head_stride multiples of %d elements (ld=%lld q_off=%d k_off=%d head_stride=%d)", epc,
				(long long)d->ld, d->q_off, d->k_off, d->head_stride);
	const int64_t last_col = (int64_t)(d->H - 1) * d->head_stride + 64;
	TTK_REQUIRE(d->q_off + last_col <= d->ld && d->k_off + last_col <= d->ld, TTK_E_ARG, "ttk_attn_probs: a head's 64 columns end past ld");
	TTK_REQUIRE(d->r0 >= 0 && d->R >= 1 && d->r0 + (int64_t)d->R <= d->T && d->c0 >= 0 && d->C >= 1 && d->c0 + (int64_t)d->C <= d->T, TTK_E_ARG,
				"ttk_attn_probs: the window rows [%d, %d + %d) and columns [%d, %d + %d) must be non-empty and lie inside [0, T=%d)", d->r0, d->r0, d->R, d->c0, d->c0, d->C, d->T);
	TTK_REQUIRE(((uintptr_t)d->out & 3) == 0 && ((uintptr_t)d->heads & 3) == 0, TTK_E_ARG, "ttk_attn_probs: out and heads must be 4-byte aligned");
	AttnProbsParams p = {};
	p.qkv = d->qkv; p.ld = d->ld; p.q_off = d->q_off; p.k_off = d->k_off; p.head_stride = d->head_stride; p.scale = d->scale;
	p.nb = d->nb; p.T = d->T; p.H = d->H; p.heads = d->heads; p.slots = nullptr; p.n_sel = d->n_sel; p.n_out = d->n_sel;
	p.r0 = d->r0; p.R = d->R; p.c0 = d->c0; p.C = d->C; p.out = d->out;
	launch_attn_probs(dtype, p, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

extern "C" int ttk_align_prepare(const float* A, int nb, int n_sel, int M, int Tt, int width, float* cost, float* matrix, void* stream) {
	TTK_REQUIRE(A && cost, TTK_E_ARG, "ttk_align_prepare: null A or cost");
	const char* why = align_shape_refusal(nb, M, Tt);
	TTK_REQUIRE(!why, TTK_E_ARG, "ttk_align_prepare: %s (nb=%d M=%d Tt=%d)", why, nb, M, Tt);
	TTK_REQUIRE(n_sel >= 1, TTK_E_ARG, "ttk_align_prepare: no head selected (n_sel=%d)", n_sel);
	TTK_REQUIRE(width >= 1 && width <= ALIGN_MAX_WIDTH && (width & 1), TTK_E_ARG, "ttk_align_prepare: the median width must be odd and in 1..%d, got %d", ALIGN_MAX_WIDTH, width);
	TTK_REQUIRE((((uintptr_t)A | (uintptr_t)cost | (uintptr_t)matrix) & 3) == 0, TTK_E_ARG, "ttk_align_prepare: A, cost and matrix must be 4-byte aligned");
	launch_align_prepare(A, nb, n_sel, M, Tt, width, cost, matrix, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

extern "C" int ttk_dtw(const float* cost, int nb, int M, int Tt, float* D, unsigned char* trace, float* total, void* stream) {
	TTK_REQUIRE(cost && D && trace && total, TTK_E_ARG, "ttk_dtw: null cost, D, trace or total");
	const char* why = align_shape_refusal(nb, M, Tt);
	TTK_REQUIRE(!why, TTK_E_ARG, "ttk_dtw: %s (nb=%d M=%d Tt=%d)", why, nb, M, Tt);
	TTK_REQUIRE((((uintptr_t)cost | (uintptr_t)D | (uintptr_t)total) & 3) == 0, TTK_E_ARG, "ttk_dtw: cost, D and total must be 4-byte aligned");
	launch_dtw(cost, nb, M, Tt, D, trace, total, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}
