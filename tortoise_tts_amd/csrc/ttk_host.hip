#include "ttk_conv.h"

#include <stdarg.h>

namespace ttk {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}
const char* get_error() { return g_err; }

int upload_f32(Arena& ar, const WeightMap& wm, const std::string& name, int64_t expect_numel, float** out) {
	const ttk_weight_view* v = wm.find(name);
	TTK_REQUIRE(v != nullptr, TTK_E_WEIGHT, "missing weight '%s'", name.c_str());
	TTK_REQUIRE(numel(v) == expect_numel, TTK_E_WEIGHT, "weight '%s' has %lld elements, expected %lld", name.c_str(),
				(long long)numel(v), (long long)expect_numel);
	TTK_TRY(ar.alloc((void**)out, (size_t)expect_numel * sizeof(float)));
	TTK_HIP(hipMemcpy(*out, v->data, (size_t)expect_numel * sizeof(float), hipMemcpyDefault));
	return TTK_OK;
}

// The launches behind upload_mat and fold_layernorm, on buffers that exist: what ttk_ar_create runs once per matrix and ttk_ar_lora_set (ar.hip) runs again,
// on the same Mat, whenever an adapter is attached or detached -- one routine, so that a switched matrix has the bits of a created one.
void pack_mat(int dt, const float* src, int layout, const Mat& m, hipStream_t s) {
	const int kdt = kernel_dtype(dt);
	if (dt == DT_FP8) launch_pack_nk_f8(src, layout, m.N, m.K, m.Npad, m.Kpad, m.wscale, m.w, s, m.ntap);
	else launch_pack_nk(kdt, src, layout, m.N, m.K, m.Npad, m.Kpad, m.w, s, m.ntap);
	if (m.wfrag) {
		if (m.w8) launch_pack_frag_fp8(m.w, m.Npad, m.Kpad, m.wscale, m.wfrag, s);
		else launch_pack_frag(kdt, m.w, m.Npad, m.Kpad, m.wfrag, s);
	}
}
void pack_fold(int dt, float* w, const float* gamma, const float* beta, const float* bias, void* wt, const Mat& m, hipStream_t s) {
	if (m.w8) launch_fp8_roundtrip(w, (int64_t)m.N * m.K, m.wscale, s);
	launch_bias_fold(w, beta, bias, m.K, m.N, m.bias_fold, s);               // from the unscaled weights
	launch_scale_kn(w, gamma, m.K, m.N, s);
	launch_pack_nk(dt, w, PK_KN, m.N, m.K, m.Npad, m.Kpad, wt, s, 1);
	launch_pack_frag(dt, wt, m.Npad, m.Kpad, m.wfrag_fold, s);
	launch_rowsum(dt, wt, m.Kpad, m.N, m.K, m.csum, s);
}

int upload_mat(Arena& ar, const WeightMap& wm, int dt, const std::string& wname, const std::string& bname, int layout,
			   int N, int K, bool frag, Mat* out, int ntap_in) {
	const ttk_weight_view* v = wm.find(wname);
	TTK_REQUIRE(v != nullptr, TTK_E_WEIGHT, "missing weight '%s'", wname.c_str());
	const int ntap = ntap_in > 0 ? ntap_in : (layout == PK_CONV3 ? 3 : 1);
	TTK_REQUIRE(numel(v) == (int64_t)N * K * ntap, TTK_E_WEIGHT, "weight '%s' has %lld elements, expected %lld", wname.c_str(),
				(long long)numel(v), (long long)N * K * ntap);
	out->N = N; out->K = K; out->ntap = ntap;
	out->Npad = round_up(N, 128);
	out->Kpad = round_up(K, dt == DT_FP8 ? 128 : 64);
	const bool w8 = dt == DT_FP8W || dt == DT_FP8;
	const int kdt = kernel_dtype(dt);
	const size_t es = dt == DT_FP8 ? 1 : dtype_size(kdt);
	out->wes = (int)es;
	float* tmp = nullptr;
	TTK_HIP(hipMalloc((void**)&tmp, (size_t)numel(v) * sizeof(float)));
	hipError_t e = hipMemcpy(tmp, v->data, (size_t)numel(v) * sizeof(float), hipMemcpyDefault);
	if (e != hipSuccess) { (void)hipFree(tmp); set_error("hipMemcpy of '%s' failed: %s", wname.c_str(), hipGetErrorString(e)); return TTK_E_HIP; }
	if (w8) {   // round the weights to the fp8 grid first: every copy made below then holds the same values
		float amax = 0.f;
		if (device_absmax(tmp, numel(v), &amax) != 0) { (void)hipFree(tmp); set_error("absmax of '%s' failed", wname.c_str()); return TTK_E_HIP; }
		out->w8 = true;
		out->wscale = fp8_scale_for(amax);
		launch_fp8_roundtrip(tmp, numel(v), out->wscale, 0);
	}
	const size_t wbytes = (size_t)ntap * out->Npad * out->Kpad * es;
	int rc = ar.alloc(&out->w, wbytes);
	if (rc == TTK_OK && frag && ntap == 1 && dt != DT_FP8) rc = ar.alloc(&out->wfrag, w8 ? wbytes / 2 : wbytes);
	if (rc == TTK_OK) pack_mat(dt, tmp, layout, *out, 0);
	e = hipDeviceSynchronize();
	(void)hipFree(tmp);
	if (rc != TTK_OK) return rc;
	if (e != hipSuccess) { set_error("weight packing of '%s' failed: %s", wname.c_str(), hipGetErrorString(e)); return TTK_E_HIP; }
	if (!bname.empty()) TTK_TRY(upload_f32(ar, wm, bname, N, &out->bias));
	return TTK_OK;
}

int fold_layernorm(Arena& ar, const WeightMap& wm, int dt, const std::string& wname, const std::string& bname, const std::string& gname,
				   const std::string& betaname, Mat* m) {
	TTK_REQUIRE(m->wfrag && m->ntap == 1, TTK_E_ARG, "fold_layernorm('%s'): needs a fragment-order matrix", wname.c_str());
	const ttk_weight_view *vw = wm.find(wname), *vb = wm.find(bname), *vg = wm.find(gname), *vbe = wm.find(betaname);
	TTK_REQUIRE(vw && vb && vg && vbe, TTK_E_WEIGHT, "fold_layernorm: missing one of '%s', '%s', '%s', '%s'", wname.c_str(), bname.c_str(), gname.c_str(), betaname.c_str());
	const int N = m->N, K = m->K;
	TTK_REQUIRE(numel(vw) == (int64_t)N * K && numel(vb) == N && numel(vg) == K && numel(vbe) == K, TTK_E_WEIGHT, "fold_layernorm('%s'): shape mismatch", wname.c_str());
	const size_t es = dtype_size(dt);
	float *w = nullptr, *g = nullptr, *be = nullptr, *b = nullptr;
	void* wt = nullptr;
	auto cleanup = [&]() { for (void* p : {(void*)w, (void*)g, (void*)be, (void*)b, wt}) if (p) (void)hipFree(p); };
	hipError_t e = hipMalloc((void**)&w, (size_t)N * K * 4);
	if (e == hipSuccess) e = hipMalloc((void**)&g, (size_t)K * 4);
	if (e == hipSuccess) e = hipMalloc((void**)&be, (size_t)K * 4);
	if (e == hipSuccess) e = hipMalloc((void**)&b, (size_t)N * 4);
	if (e == hipSuccess) e = hipMalloc(&wt, (size_t)m->Npad * m->Kpad * es);
	if (e == hipSuccess) e = hipMemcpy(w, vw->data, (size_t)N * K * 4, hipMemcpyDefault);
	if (e == hipSuccess) e = hipMemcpy(g, vg->data, (size_t)K * 4, hipMemcpyDefault);
	if (e == hipSuccess) e = hipMemcpy(be, vbe->data, (size_t)K * 4, hipMemcpyDefault);
	if (e == hipSuccess) e = hipMemcpy(b, vb->data, (size_t)N * 4, hipMemcpyDefault);
	if (e != hipSuccess) { cleanup(); set_error("fold_layernorm('%s'): %s", wname.c_str(), hipGetErrorString(e)); return TTK_E_HIP; }
	int rc = ar.alloc(&m->wfrag_fold, (size_t)m->Npad * m->Kpad * es);
	if (rc == TTK_OK) rc = ar.alloc((void**)&m->csum, (size_t)N * 4);
	if (rc == TTK_OK) rc = ar.alloc((void**)&m->bias_fold, (size_t)N * 4);
	if (rc != TTK_OK) { cleanup(); return rc; }
	// fp8 weights: the mode is defined on the reference's matrices, so those are rounded first (same scale as upload_mat) and the fold is taken
	// of the ROUNDED matrix, in the kernel arithmetic -- what a bf16 handle built from the rounded weights computes, bit for bit.  The folded
	// operand is a bf16 matrix (gamma o W^ is not on the fp8 grid): these two launches stream 2 bytes per weight, the decode step being bound by
	// its launch chain, not by weight bytes
	pack_fold(dt, w, g, be, b, wt, *m, 0);
	e = hipDeviceSynchronize();
	cleanup();
	if (e != hipSuccess) { set_error("fold_layernorm('%s'): %s", wname.c_str(), hipGetErrorString(e)); return TTK_E_HIP; }
	return TTK_OK;
}

bool g_prof_on = false;
namespace {
struct ProfRec { hipEvent_t a, b; int kind; double work; };
std::vector<ProfRec> g_recs;
std::vector<hipEvent_t> g_pool;
size_t g_pool_used = 0;
hipEvent_t pool_get() {
	if (g_pool_used == g_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); g_pool.push_back(e); }
	return g_pool[g_pool_used++];
}
}  // namespace
void prof_start(int kind, double work, hipStream_t s) {
	ProfRec r; r.a = pool_get(); r.b = pool_get(); r.kind = kind; r.work = work;
	(void)hipEventRecord(r.a, s);
	g_recs.push_back(r);
}
void prof_stop(hipStream_t s) { (void)hipEventRecord(g_recs.back().b, s); }
void prof_pair(int kind, double work, hipEvent_t* start, hipEvent_t* stop) {
	ProfRec r; r.a = pool_get(); r.b = pool_get(); r.kind = kind; r.work = work;
	g_recs.push_back(r);
	*start = r.a; *stop = r.b;
}

}  // namespace ttk

extern "C" {
int ttk_prof_begin(void) {
	ttk::g_recs.clear();
	ttk::g_pool_used = 0;
	ttk::g_prof_on = true;
	return TTK_OK;
}
int ttk_prof_end(ttk_prof_result* out, int n_kinds) {
	ttk::g_prof_on = false;
	TTK_REQUIRE(out && n_kinds >= ttk::PROF_KINDS, TTK_E_ARG, "ttk_prof_end: need room for %d kinds", (int)ttk::PROF_KINDS);
	TTK_HIP(hipDeviceSynchronize());
	for (int i = 0; i < n_kinds; ++i) { out[i].ms = 0; out[i].launches = 0; out[i].work = 0; }
	for (const auto& r : ttk::g_recs) {
		float ms = 0.f;
		TTK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
		out[r.kind].ms += ms; out[r.kind].launches += 1; out[r.kind].work += r.work;
	}
	ttk::g_recs.clear();
	return TTK_OK;
}
int ttk_version(void) { return TTK_VERSION; }
const char* ttk_last_error(void) { return ttk::get_error(); }
}

extern "C" int ttk_fp8_round_weights(float* x, int64_t n, float* scale_out, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(x && n > 0, TTK_E_ARG, "ttk_fp8_round_weights: null or empty array");
	TTK_HIP(hipStreamSynchronize((hipStream_t)stream));
	float amax = 0.f;
	TTK_REQUIRE(device_absmax(x, n, &amax) == 0, TTK_E_HIP, "ttk_fp8_round_weights: absmax reduction failed");
	const float s = fp8_scale_for(amax);
	launch_fp8_roundtrip(x, n, s, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	if (scale_out) *scale_out = s;
	return TTK_OK;
}

// The dense NT GEMM on caller-provided operands: kernel-level numerics tests (a plain f32 matmul of the same operands is the reference) and tuning.
extern "C" int ttk_gemm_nt(int dtype, const void* A, const void* W, int M, int N, int K, float out_scale, const float* bias, float* C, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(A && W && C, TTK_E_ARG, "ttk_gemm_nt: null argument");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16 || dtype == TTK_FP8, TTK_E_ARG, "ttk_gemm_nt: dtype must be TTK_F32, TTK_BF16, TTK_F16 or TTK_FP8 (fp8-e4m3 bytes), got %d", dtype);
	const int kmul = dtype == TTK_FP8 ? 128 : (dtype == TTK_F32 ? 32 : 64);
	TTK_REQUIRE(M >= 1 && N >= 128 && N % 128 == 0 && K >= kmul && K % kmul == 0, TTK_E_ARG,
				"ttk_gemm_nt: need M >= 1, N %% 128 == 0, K %% %d == 0 (got M=%d N=%d K=%d)", kmul, M, N, K);
	Mat m;
	m.w = const_cast<void*>(W); m.N = N; m.Kpad = K; m.bias = const_cast<float*>(bias);
	GemmParams g = dense_gemm(A, K, m, M, C, 1);
	g.out_scale = out_scale;
	launch_gemm(dtype, g, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// Every form of the dense GEMM on caller-provided operands (include/ttk.h): the descriptor is GemmParams field for field, and launch_gemm picks tile and role
// exactly as for the handles' launches.  What is checked here is what the kernels take for granted and cannot check themselves.
static_assert(sizeof(ttk_gemm_seg) == 32 && sizeof(ttk_gemm_desc) == 496, "ttk_gemm_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_gemm(int dtype, const ttk_gemm_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_gemm: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16 || dtype == TTK_FP8, TTK_E_ARG, "ttk_gemm: dtype must be TTK_F32, TTK_BF16, TTK_F16 or TTK_FP8 (fp8-e4m3 bytes), got %d", dtype);
	const int es = dtype == TTK_FP8 ? 1 : (dtype == TTK_F32 ? 4 : 2);
	const int kmul = dtype == TTK_FP8 ? 128 : (dtype == TTK_F32 ? 32 : 64);
	const int epc = 16 / es;      // elements per 16-byte staging chunk: row strides and offsets are whole chunks
	auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
	TTK_REQUIRE(d->nseg >= 1 && d->nseg <= 12, TTK_E_ARG, "ttk_gemm: nseg must be 1..12, got %d", d->nseg);
	TTK_REQUIRE(d->M >= 1 && d->N >= 1 && d->K >= kmul && d->K % kmul == 0, TTK_E_ARG, "ttk_gemm: need M >= 1, N >= 1, K %% %d == 0 (got M=%d N=%d K=%d)", kmul, d->M, d->N, d->K);
	TTK_REQUIRE(d->act >= 0 && d->act <= 2, TTK_E_ARG, "ttk_gemm: act must be 0 (none), 1 (gelu_new) or 2 (SiLU), got %d", d->act);
	TTK_REQUIRE(d->W && al16(d->W) && d->ldw >= d->K && d->ldw % epc == 0, TTK_E_ARG, "ttk_gemm: W must be 16-byte aligned with ldw >= K and ldw %% %d == 0 (ldw=%lld)", epc, (long long)d->ldw);
	TTK_REQUIRE(d->rows_per_batch >= 0, TTK_E_ARG, "ttk_gemm: rows_per_batch < 0");
	const int64_t npad = ((int64_t)d->N + 127) / 128 * 128;      // the kernels read W rows up to the next multiple of 128 (buffer offsets are 32-bit)
	bool shifted = false;
	for (int j = 0; j < d->nseg; ++j) {
		const ttk_gemm_seg& sg = d->seg[j];
		TTK_REQUIRE(sg.A && al16(sg.A) && sg.lda >= d->K && sg.lda % epc == 0, TTK_E_ARG, "ttk_gemm: segment %d: A must be 16-byte aligned with lda >= K and lda %% %d == 0 (lda=%lld)", j, epc, (long long)sg.lda);
		TTK_REQUIRE(sg.w_off >= 0 && sg.w_off % epc == 0, TTK_E_ARG, "ttk_gemm: segment %d: w_off must be >= 0 and a multiple of %d", j, epc);
		TTK_REQUIRE((int64_t)d->M * sg.lda * es < (1ll << 31) && (sg.w_off + (npad - 1) * d->ldw + d->K) * es < (1ll << 31), TTK_E_ARG,
					"ttk_gemm: segment %d: A or W spans 2 GiB or more (32-bit buffer offsets)", j);
		shifted |= sg.shift != 0;
	}
	TTK_REQUIRE(!(shifted || d->transpose_out) || d->rows_per_batch > 0, TTK_E_ARG, "ttk_gemm: shifted segments and transpose_out need rows_per_batch > 0");
	TTK_REQUIRE(d->C && ((uintptr_t)d->C & 3) == 0, TTK_E_ARG, "ttk_gemm: C must be 4-byte aligned");
	if (d->transpose_out) {
		TTK_REQUIRE(d->out_f32 && d->M % d->rows_per_batch == 0 && !d->residual, TTK_E_ARG,
					"ttk_gemm: transpose_out writes f32 [M / rows_per_batch][N][rows_per_batch]: needs out_f32, M %% rows_per_batch == 0 and no residual");
	} else {
		TTK_REQUIRE(d->ldc >= d->N, TTK_E_ARG, "ttk_gemm: ldc < N");
	}
	TTK_REQUIRE(!d->residual || (d->out_f32 && d->ldr >= d->N), TTK_E_ARG, "ttk_gemm: a residual needs out_f32 and ldr >= N (the 16-bit epilogue has none)");
	if (d->gn_part) {
		TTK_REQUIRE(d->gn_T > 0 && d->out_f32 && !d->transpose_out && gemm_fuses_gn_stats(d->M, d->N, d->N, d->gn_T), TTK_E_ARG,
					"ttk_gemm: gn_part needs f32 row-major output and a shape whose tiles produce the statistics (N == 1024, M %% 64 == 0, gn_T %% 64 == 0, "
					"no 64-row tile; got M=%d N=%d gn_T=%d)", d->M, d->N, d->gn_T);
	}
	GemmParams g = {};
	g.nseg = d->nseg;
	for (int j = 0; j < d->nseg; ++j) g.seg[j] = {d->seg[j].A, d->seg[j].lda, d->seg[j].shift, d->seg[j].w_off};
	g.W = d->W; g.ldw = d->ldw; g.M = d->M; g.N = d->N; g.K = d->K; g.rows_per_batch = d->rows_per_batch; g.act = d->act;
	g.bias = d->bias; g.residual = d->residual; g.ldr = d->ldr; g.C = d->C; g.ldc = d->ldc;
	g.out_scale = d->out_scale; g.out_f32 = d->out_f32; g.transpose_out = d->transpose_out;
	g.gn_T = d->gn_part ? d->gn_T : 0; g.gn_part = d->gn_part;
	launch_gemm(dtype, g, (hipStream_t)stream);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// Every launch form of the attention kernels on caller-provided operands (include/ttk.h): the descriptors are AttnParams / AttnDecodeParams without the prefetch and
// diagnostic fields, plus the host-only form / variant.  With form = 0 / variant = 0 the launchers choose exactly as for the handles' launches.
static_assert(sizeof(ttk_attn_desc) == 96 && sizeof(ttk_attn_decode_desc) == 80, "ttk_attn_desc / ttk_attn_decode_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_attn_fwd(int dtype, const ttk_attn_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_attn_fwd: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16, TTK_E_ARG, "ttk_attn_fwd: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", dtype);
	const int epc = dtype == TTK_F32 ? 4 : 8;      // elements per 16 bytes: every fragment and staging chunk is read as whole 16-byte words
	auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
	TTK_REQUIRE(d->qkv && d->out, TTK_E_ARG, "ttk_attn_fwd: null qkv or out");
	TTK_REQUIRE(d->T >= 1 && d->nb >= 1 && d->H >= 1, TTK_E_ARG, "ttk_attn_fwd: need T >= 1, nb >= 1, H >= 1 (got T=%d nb=%d H=%d)", d->T, d->nb, d->H);
	TTK_REQUIRE(al16(d->qkv) && d->ld > 0 && d->ld % epc == 0 && d->q_off >= 0 && d->k_off >= 0 && d->v_off >= 0 && d->head_stride >= 0 &&
				d->q_off % epc == 0 && d->k_off % epc == 0 && d->v_off % epc == 0 && d->head_stride % epc == 0, TTK_E_ARG,
				"ttk_attn_fwd: qkv must be 16-byte aligned, ld, q_off, k_off, v_off and head_stride multiples of %d elements (ld=%lld q_off=%d k_off=%d v_off=%d head_stride=%d)",
				epc, (long long)d->ld, d->q_off, d->k_off, d->v_off, d->head_stride);
	const int64_t last_col = (int64_t)(d->H - 1) * d->head_stride + 64;
	TTK_REQUIRE(d->q_off + last_col <= d->ld && d->k_off + last_col <= d->ld && d->v_off + last_col <= d->ld, TTK_E_ARG, "ttk_attn_fwd: a head's 64 columns end past ld");
	TTK_REQUIRE(d->ldo >= (int64_t)64 * d->H, TTK_E_ARG, "ttk_attn_fwd: ldo < 64 H");
	TTK_REQUIRE(!d->out_f8 || dtype == TTK_BF16, TTK_E_ARG, "ttk_attn_fwd: out_f8 only with TTK_BF16");
	TTK_REQUIRE(d->out_f8 ? (((uintptr_t)d->out & 3) == 0 && d->ldo % 4 == 0) : ((uintptr_t)d->out & (dtype == TTK_F32 ? 3 : 1)) == 0, TTK_E_ARG,
				"ttk_attn_fwd: out is misaligned (out_f8 stores 4 bytes at a time: out and ldo multiples of 4)");
	TTK_REQUIRE(!(d->causal && d->bias), TTK_E_ARG, "ttk_attn_fwd: causal together with bias: there is no such kernel (the launcher would drop the bias)");
	AttnParams a = {};
	a.qkv = d->qkv; a.ld = d->ld; a.q_off = d->q_off; a.k_off = d->k_off; a.v_off = d->v_off; a.head_stride = d->head_stride;
	a.out = d->out; a.ldo = d->ldo; a.out_f8 = d->out_f8; a.nb = d->nb; a.T = d->T; a.H = d->H; a.causal = d->causal ? 1 : 0;
	a.tlen = d->tlen; a.bias = d->bias; a.scale = d->scale;
	const char* why = attn_fwd_form_refusal(a, d->form);
	TTK_REQUIRE(!why, TTK_E_ARG, "ttk_attn_fwd: %s (form=%d causal=%d tlen=%s nb=%d H=%d T=%d)", why, d->form, a.causal, a.tlen ? "set" : "null", a.nb, a.H, a.T);
	launch_attn_fwd(dtype, a, (hipStream_t)stream, d->form);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// Every launch form of GroupNorm-apply on caller-provided operands (include/ttk.h): the descriptor is GnApplyParams plus the host-only form, and `stats` for the
// statistics launch in front.  With form = 0 the launcher chooses exactly as for the handles' launches.
static_assert(sizeof(ttk_gn_desc) == 144, "ttk_gn_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_gn_apply(int dtype, const ttk_gn_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_gn_apply: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16, TTK_E_ARG, "ttk_gn_apply: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", dtype);
	TTK_REQUIRE(d->x && d->ms && d->gamma && d->beta && d->out, TTK_E_ARG, "ttk_gn_apply: null x, ms, gamma, beta or out");
	TTK_REQUIRE(d->C == 128 || d->C == 256 || d->C == 512 || d->C == 1024, TTK_E_ARG, "ttk_gn_apply: C must be 128, 256, 512 or 1024 (C %% 128 == 0, C <= 1024), got %d", d->C);
	TTK_REQUIRE(d->nb >= 1 && d->T >= 1 && d->Tout >= 1, TTK_E_ARG, "ttk_gn_apply: need nb >= 1, T >= 1, Tout >= 1 (got nb=%d T=%d Tout=%d)", d->nb, d->T, d->Tout);
	TTK_REQUIRE(d->row_idx || d->Tout == d->T, TTK_E_ARG, "ttk_gn_apply: Tout != T needs row_idx");
	TTK_REQUIRE(!d->tlen || (!d->row_idx && d->Tout == d->T), TTK_E_ARG, "ttk_gn_apply: tlen needs Tout == T and no row_idx");
	TTK_REQUIRE(gn_num_chunks(d->T, d->C) <= 64, TTK_E_ARG, "ttk_gn_apply: %d rows are more than 64 statistics chunks", d->T);
	TTK_REQUIRE(!d->scale == !d->shift && d->ss_stride >= 0 && d->ss_stride % 4 == 0, TTK_E_ARG, "ttk_gn_apply: scale and shift come together, ss_stride >= 0 and %% 4 == 0");
	for (const void* q : {(const void*)d->x, (const void*)d->gamma, (const void*)d->beta, (const void*)d->scale, (const void*)d->shift, (const void*)d->out})
		TTK_REQUIRE(((uintptr_t)q & 15) == 0, TTK_E_ARG, "ttk_gn_apply: x, gamma, beta, scale, shift and out must be 16-byte aligned");
	TTK_REQUIRE(d->act == 0 || d->act == 2, TTK_E_ARG, "ttk_gn_apply: act must be 0 (none) or 2 (SiLU), got %d", d->act);
	TTK_REQUIRE(!d->out_f8 || dtype == TTK_BF16, TTK_E_ARG, "ttk_gn_apply: out_f8 only with TTK_BF16");
	TTK_REQUIRE(!d->pf || (d->pf_bytes >= 0 && d->pf_taps >= 1), TTK_E_ARG, "ttk_gn_apply: pf needs pf_bytes >= 0 and pf_taps >= 1");
	GnApplyParams p = {};
	p.x = d->x; p.ms = d->ms; p.gamma = d->gamma; p.beta = d->beta; p.scale = d->scale; p.shift = d->shift; p.ss_stride = d->ss_stride;
	p.row_idx = d->row_idx; p.nb = d->nb; p.T = d->T; p.Tout = d->Tout; p.C = d->C; p.nchunks = gn_num_chunks(d->T, d->C); p.act = d->act;
	p.out = d->out; p.out_f32 = d->out_f32 ? 1 : 0; p.out_f8 = d->out_f8 ? 1 : 0;
	if (d->tlen) { p.tlen = d->tlen; p.chunk_rows = gn_rows_per_chunk(d->C); }
	if (d->pf) { p.pf = d->pf; p.pf_bytes = d->pf_bytes; p.pf_taps = d->pf_taps; }
	const char* why = gn_apply_form_refusal(p, d->form);
	TTK_REQUIRE(!why, TTK_E_ARG, "ttk_gn_apply: %s (form=%d C=%d nb=%d T=%d Tout=%d tlen=%s row_idx=%s)", why, d->form, p.C, p.nb, p.T, p.Tout, p.tlen ? "set" : "null", p.row_idx ? "set" : "null");
	if (d->stats) launch_gn_stats(d->x, d->nb, d->T, d->C, d->ms, (hipStream_t)stream, d->tlen);
	launch_gn_apply(dtype, p, (hipStream_t)stream, d->form);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// LayerNorm on caller-provided operands (include/ttk.h): the descriptor is launch_layernorm's argument list, the launch is launch_layernorm.  Everything
// k_layernorm takes for granted is checked here: float4 loads of x and the affine vectors and float4 stores to out2 (16-byte alignment, d, ldx and the ring stride
// multiples of 4), 4 / 16 float4 slots per lane (d <= 4096), whole 32-column k-steps in fragment order, rows that do not overlap.
static_assert(sizeof(ttk_ln_desc) == 112, "ttk_ln_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_layernorm_rows(int dtype, const ttk_ln_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_layernorm_rows: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16, TTK_E_ARG, "ttk_layernorm_rows: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", dtype);
	TTK_REQUIRE(d->x && d->g1 && d->b1 && d->out, TTK_E_ARG, "ttk_layernorm_rows: null x, g1, b1 or out");
	TTK_REQUIRE(!d->g2 == !d->b2, TTK_E_ARG, "ttk_layernorm_rows: g2 and b2 come together");
	TTK_REQUIRE(d->rows >= 1, TTK_E_ARG, "ttk_layernorm_rows: need rows >= 1, got %d", d->rows);
	TTK_REQUIRE(d->d >= 4 && d->d % 4 == 0 && d->d <= 4096, TTK_E_ARG, "ttk_layernorm_rows: d must be a multiple of 4 in 4 .. 4096 (one wave holds a row), got %d", d->d);
	TTK_REQUIRE(!d->frag || d->d % 32 == 0, TTK_E_ARG, "ttk_layernorm_rows: frag needs d %% 32 == 0 (whole k-steps), got %d", d->d);
	TTK_REQUIRE(d->ldx >= d->d && d->ldx % 4 == 0, TTK_E_ARG, "ttk_layernorm_rows: ldx must be >= d and %% 4 == 0, got %lld", (long long)d->ldx);
	TTK_REQUIRE(d->frag || d->ldo >= d->d, TTK_E_ARG, "ttk_layernorm_rows: ldo < d (row-major output)");
	for (const void* q : {(const void*)d->x, (const void*)d->g1, (const void*)d->b1, (const void*)d->g2, (const void*)d->b2, (const void*)d->out2})
		TTK_REQUIRE(((uintptr_t)q & 15) == 0, TTK_E_ARG, "ttk_layernorm_rows: x, g1, b1, g2, b2 and out2 must be 16-byte aligned");
	TTK_REQUIRE(((uintptr_t)d->out & ((d->out_f32 || dtype == TTK_F32) ? 3 : 1)) == 0, TTK_E_ARG, "ttk_layernorm_rows: out is misaligned for its element type");
	TTK_REQUIRE(((uintptr_t)d->out2_idx & 7) == 0 && ((uintptr_t)d->out2_base & 7) == 0, TTK_E_ARG, "ttk_layernorm_rows: out2_idx and out2_base must be 8-byte aligned");
	TTK_REQUIRE(!d->out2_idx || d->out2 || d->out2_base, TTK_E_ARG, "ttk_layernorm_rows: out2_idx without out2 or out2_base: a ring slot of nothing");
	TTK_REQUIRE(d->out2_stride >= 0 && d->out2_stride % 4 == 0, TTK_E_ARG, "ttk_layernorm_rows: out2_stride must be >= 0 and %% 4 == 0, got %lld", (long long)d->out2_stride);
	launch_layernorm(dtype, d->x, d->ldx, d->rows, d->d, d->g1, d->b1, d->g2, d->b2, d->out, d->ldo, d->out_f32 ? 1 : 0, (hipStream_t)stream, d->frag ? 1 : 0,
					 d->out2, d->out2_idx, d->out2_stride, d->out2_base);
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

extern "C" int ttk_attn_decode(int dtype, const ttk_attn_decode_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(d, TTK_E_ARG, "ttk_attn_decode: null descriptor");
	TTK_REQUIRE(dtype == TTK_F32 || dtype == TTK_BF16 || dtype == TTK_F16, TTK_E_ARG, "ttk_attn_decode: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", dtype);
	TTK_REQUIRE(d->qbuf && d->kcache && d->vcache && d->d_pos && d->out, TTK_E_ARG, "ttk_attn_decode: null qbuf, kcache, vcache, d_pos or out");
	TTK_REQUIRE(d->B >= 1 && d->H >= 1 && d->max_ctx >= 1, TTK_E_ARG, "ttk_attn_decode: need B >= 1, H >= 1, max_ctx >= 1 (got B=%d H=%d max_ctx=%d)", d->B, d->H, d->max_ctx);
	TTK_REQUIRE(d->B <= 65535, TTK_E_ARG, "ttk_attn_decode: B > 65535 (the grid's y dimension)");
	TTK_REQUIRE(((uintptr_t)d->qbuf & 15) == 0 && ((uintptr_t)d->kcache & 15) == 0 && ((uintptr_t)d->vcache & 15) == 0 && ((uintptr_t)d->d_pos & 7) == 0 &&
				((uintptr_t)d->out & (dtype == TTK_F32 ? 3 : 1)) == 0 && ((uintptr_t)d->row_info & 7) == 0, TTK_E_ARG,
				"ttk_attn_decode: qbuf, kcache and vcache must be 16-byte aligned, d_pos and row_info 8-byte aligned (both words are one request)");
	TTK_REQUIRE(!d->out_frag || (64 * d->H) % 32 == 0, TTK_E_ARG, "ttk_attn_decode: out_frag needs 64 H %% 32 == 0");
	TTK_REQUIRE(d->variant >= 0 && d->variant <= 2, TTK_E_ARG, "ttk_attn_decode: variant must be 0 (default), 1 (4 x 4) or 2 (8 x 6), got %d", d->variant);
	TTK_REQUIRE(d->variant == 0 || dtype == TTK_BF16, TTK_E_ARG, "ttk_attn_decode: variants 1 and 2 are bf16 only");
	AttnDecodeParams a = {};
	a.qbuf = d->qbuf; a.kcache = d->kcache; a.vcache = d->vcache; a.d_pos = d->d_pos; a.B = d->B; a.H = d->H; a.max_ctx = d->max_ctx; a.ctx_hint = d->max_ctx;
	a.out = d->out; a.out_frag = d->out_frag ? 1 : 0; a.row_info = (const int2*)d->row_info; a.shared_rows = d->shared_rows ? 1 : 0;
	int slot = -1;
	if (d->pos_line) {      // the two words through a slot of the position line, as a handle that owns one keeps them
		int* words = nullptr;
		slot = attn_pos_slot_acquire(&words);
		TTK_REQUIRE(slot >= 0, TTK_E_ARG, "ttk_attn_decode: pos_line: no free slot in the position line (8 decode handles hold them)");
		const hipError_t e = hipMemcpyAsync(words, d->d_pos, 2 * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream);
		if (e != hipSuccess) { attn_pos_slot_release(slot); set_error("ttk_attn_decode: copy into the position line failed: %s", hipGetErrorString(e)); return TTK_E_HIP; }
		a.d_pos = words; a.pos_slot_p1 = slot + 1;
	}
	launch_attn_decode(dtype, a, (hipStream_t)stream, d->variant);
	if (slot >= 0) attn_pos_slot_release(slot);      // enqueued: a later user of the slot writes it behind this launch on the same stream
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}

// One decode matrix and one weight-streaming launch on caller-provided operands (include/ttk.h).  The matrix goes through upload_mat / fold_layernorm, the launch through
// decode_launch (ar.hip): what the token step of a ttk_ar handle runs.  What is checked here is what the kernels take for granted and cannot check themselves.
struct ttk_gemv_mat {
	ttk::Arena arena;
	ttk::Mat m;
	int dtype = 0, dt = 0;      // as created / the arithmetic type of the kernels
	bool folded = false;
};
static_assert(sizeof(ttk_gemv_mat_config) == 16 && sizeof(ttk_gemv_desc) == 184, "ttk_gemv_mat_config / ttk_gemv_desc layout (tortoise_tts_amd/_lib.py mirrors it)");
extern "C" int ttk_gemv_mat_create(ttk_gemv_mat** out, const ttk_gemv_mat_config* cfg, const ttk_weight_view* w, int n_w) {
	using namespace ttk;
	TTK_REQUIRE(out && cfg && w, TTK_E_ARG, "ttk_gemv_mat_create: null argument");
	TTK_REQUIRE(cfg->dtype == TTK_F32 || cfg->dtype == TTK_BF16 || cfg->dtype == TTK_F16 || cfg->dtype == TTK_FP8W, TTK_E_ARG, "ttk_gemv_mat_create: bad dtype %d", cfg->dtype);
	TTK_REQUIRE(cfg->layout == PK_NK || cfg->layout == PK_KN, TTK_E_ARG, "ttk_gemv_mat_create: layout must be 0 ([N][K]) or 1 ([K][N]), got %d", cfg->layout);
	// the packers pad K to 64 while the kernels index fragments by K / 32: any other K and the two disagree
	TTK_REQUIRE(cfg->N >= 1 && cfg->K >= 64 && cfg->K % 64 == 0, TTK_E_ARG, "ttk_gemv_mat_create: need N >= 1 and K %% 64 == 0 (got N=%d K=%d)", cfg->N, cfg->K);
	std::unique_ptr<ttk_gemv_mat> h(new ttk_gemv_mat());
	h->dtype = cfg->dtype; h->dt = kernel_dtype(cfg->dtype);
	WeightMap wm(w, n_w);
	TTK_TRY(upload_mat(h->arena, wm, cfg->dtype, "weight", "bias", cfg->layout, cfg->N, cfg->K, true, &h->m));
	const bool g = wm.find("gamma") != nullptr, b = wm.find("beta") != nullptr;
	TTK_REQUIRE(g == b, TTK_E_ARG, "ttk_gemv_mat_create: gamma and beta come together");
	if (g) {
		TTK_REQUIRE(cfg->layout == PK_KN, TTK_E_ARG, "ttk_gemv_mat_create: the LayerNorm fold is defined on HF Conv1D matrices (layout 1)");
		TTK_TRY(fold_layernorm(h->arena, wm, h->dt, "weight", "bias", "gamma", "beta", &h->m));
		h->folded = true;
	}
	*out = h.release();
	return TTK_OK;
}
extern "C" int ttk_gemv_mat_destroy(ttk_gemv_mat* h) {
	if (!h) return TTK_OK;
	(void)hipDeviceSynchronize();
	delete h;
	return TTK_OK;
}
extern "C" int ttk_gemv_launch(const ttk_gemv_mat* W, const ttk_gemv_desc* d, void* stream) {
	using namespace ttk;
	TTK_REQUIRE(W && d, TTK_E_ARG, "ttk_gemv_launch: null matrix or descriptor");
	const int N = W->m.N, K = W->m.K, dt = W->dt;
	TTK_REQUIRE(d->dtype == TTK_F32 || d->dtype == TTK_BF16 || d->dtype == TTK_F16, TTK_E_ARG, "ttk_gemv_launch: dtype must be TTK_F32, TTK_BF16 or TTK_F16, got %d", d->dtype);
	TTK_REQUIRE(!(W->m.w8 && d->dtype != TTK_BF16), TTK_E_ARG, "ttk_gemv_launch: an fp8 matrix runs under bf16 arithmetic only (dtype %d)", d->dtype);
	TTK_REQUIRE(d->dtype == dt, TTK_E_ARG, "ttk_gemv_launch: dtype %d is not the arithmetic type the matrix was packed for (%d)", d->dtype, dt);
	TTK_REQUIRE(d->role >= 0 && d->role <= 3, TTK_E_ARG, "ttk_gemv_launch: role must be 0 (qkv), 1 (proj), 2 (fc) or 3 (head), got %d", d->role);
	TTK_REQUIRE(d->form >= 0 && d->form <= 2, TTK_E_ARG, "ttk_gemv_launch: form must be 0 (plain), 1 (folded LayerNorm) or 2 (LayerNorm prologue), got %d", d->form);
	const bool qkv = d->role == 0, proj = d->role == 1, fc = d->role == 2, head = d->role == 3;
	const bool fold = d->form == 1, prologue = d->form == 2;
	const int cap = dt == DT_F32 ? 32 : 64;
	TTK_REQUIRE(d->M >= 1 && d->M <= cap, TTK_E_ARG, "ttk_gemv_launch: M=%d outside 1..%d", d->M, cap);
	TTK_REQUIRE(!(prologue && !head && d->M > 32), TTK_E_ARG, "ttk_gemv_launch: the LayerNorm-prologue form outside the head holds at most 32 rows in LDS; M=%d", d->M);
	TTK_REQUIRE(!fold || qkv || fc, TTK_E_ARG, "ttk_gemv_launch: a folded LayerNorm sits in front of qkv and fc only (role %d)", d->role);
	TTK_REQUIRE(!fold || W->folded, TTK_E_ARG, "ttk_gemv_launch: the folded form needs a matrix created with gamma and beta");
	TTK_REQUIRE(d->form != 0 || proj || head, TTK_E_ARG, "ttk_gemv_launch: qkv and fc take the folded or the prologue form (no decode launch multiplies them plainly)");
	TTK_REQUIRE(!(prologue && proj), TTK_E_ARG, "ttk_gemv_launch: the residual projections have no LayerNorm in front");
	auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
	if (prologue) {
		TTK_REQUIRE(d->x && d->g1 && d->b1 && (!d->g2 == !d->b2), TTK_E_ARG, "ttk_gemv_launch: the prologue form needs x, g1 and b1 (null), and g2 with b2 or neither");
		TTK_REQUIRE(al(d->x, 16) && al(d->g1, 16) && al(d->b1, 16) && al(d->g2, 16) && al(d->b2, 16), TTK_E_ARG, "ttk_gemv_launch: x, g1, b1, g2 and b2 must be 16-byte aligned");
	} else {
		TTK_REQUIRE(d->a, TTK_E_ARG, "ttk_gemv_launch: null a");
		TTK_REQUIRE(al(d->a, 16), TTK_E_ARG, "ttk_gemv_launch: a must be 16-byte aligned");
	}
	TTK_REQUIRE(al(d->out_T, 16) && al(d->out_f32, 4), TTK_E_ARG, "ttk_gemv_launch: out_T must be 16-byte aligned, out_f32 4-byte aligned");
	TTK_REQUIRE(!d->out_T || N % 32 == 0, TTK_E_ARG, "ttk_gemv_launch: out_T is in fragment order: needs N %% 32 == 0 (N=%d)", N);
	if (qkv) {
		TTK_REQUIRE(d->qbuf && d->kcache && d->vcache && d->d_pos, TTK_E_ARG, "ttk_gemv_launch: qkv: null qbuf, kcache, vcache or d_pos");
		TTK_REQUIRE(al(d->qbuf, 16) && al(d->kcache, 16) && al(d->vcache, 16) && al(d->d_pos, 4), TTK_E_ARG, "ttk_gemv_launch: qbuf, kcache and vcache must be 16-byte aligned, d_pos 4-byte aligned");
		TTK_REQUIRE(N == 3 * K && d->H >= 1 && K == 64 * d->H, TTK_E_ARG, "ttk_gemv_launch: qkv needs N == 3 K and K == 64 H (N=%d K=%d H=%d)", N, K, d->H);
		TTK_REQUIRE(d->max_ctx >= 1, TTK_E_ARG, "ttk_gemv_launch: qkv needs max_ctx >= 1");
		TTK_REQUIRE(d->q_scale == 0.125f, TTK_E_ARG, "ttk_gemv_launch: q_scale must be 0.125 (head dim 64), got %g", (double)d->q_scale);
	} else if (fc) {
		TTK_REQUIRE(d->out_T, TTK_E_ARG, "ttk_gemv_launch: fc: null out_T");
	} else {
		TTK_REQUIRE(d->out_f32, TTK_E_ARG, "ttk_gemv_launch: %s: null out_f32", proj ? "proj" : "head");
	}
	if (head) {
		TTK_REQUIRE((d->noise && d->rng && d->draws) || (!d->noise && !d->rng && !d->draws), TTK_E_ARG, "ttk_gemv_launch: head: pass noise, rng and draws or none of them");
		TTK_REQUIRE(al(d->noise, 4) && al(d->rng, 8) && al(d->draws, 8), TTK_E_ARG, "ttk_gemv_launch: noise must be 4-byte aligned, rng and draws 8-byte aligned");
		TTK_REQUIRE(!d->bump || (d->d_pos && al(d->d_pos, 4)), TTK_E_ARG, "ttk_gemv_launch: bump needs a 4-byte aligned d_pos");
	}
	TTK_REQUIRE(al(d->health, 4), TTK_E_ARG, "ttk_gemv_launch: health must be 4-byte aligned");
	TTK_REQUIRE(d->family >= 0 && d->family <= 2, TTK_E_ARG, "ttk_gemv_launch: family must be 0 (the decode step's choice), 1 (k_skinny) or 2 (k_gemv), got %d", d->family);
	TTK_REQUIRE(d->waves == 0 || (d->waves >= 4 && d->waves <= (prologue ? 8 : 16)), TTK_E_ARG, "ttk_gemv_launch: waves must be 0 or 4..%d, got %d", prologue ? 8 : 16, d->waves);
	const int drole = qkv ? DR_QKV : (fc ? DR_FC : (head ? DR_HEAD : (K == N ? DR_PROJ : DR_PROJ2)));
	DecodeCtx c = {};
	TTK_REQUIRE(d->model_dim >= 0 && d->model_dim % 64 == 0, TTK_E_ARG, "ttk_gemv_launch: model_dim must be 0 or a multiple of 64, got %d", d->model_dim);
	c.dt = dt; c.lean = 1; c.lnfold = !(prologue && !head); c.model_dim = d->model_dim ? d->model_dim : (proj ? N : K); c.health = d->health; c.launched = d->launched;
	c.rng_args = d->rng; c.rng_draws = d->draws; c.rng_q = d->noise; c.family = d->family; c.waves = d->waves;
	if (d->family == 2) {
		TTK_REQUIRE(!prologue, TTK_E_ARG, "ttk_gemv_launch: family 2: k_gemv has no LayerNorm-prologue form");
		GemvParams g = {};
		g.M = d->M; g.N = N; g.K = K; g.w8 = fold ? 0 : W->m.w8;
		TTK_REQUIRE(gemv_supported(dt, qkv ? GV_QKV : (fc ? GV_FC : (head ? GV_HEAD : GV_PROJ)), g), TTK_E_ARG,
					"ttk_gemv_launch: family 2: k_gemv has no instantiation for role %d at N=%d K=%d M=%d%s", d->role, N, K, d->M, g.w8 ? " with fp8 weights" : "");
	}
	{   // k_skinny, if this launch falls to it: its LDS against the compute unit's
		const int waves = skinny_launch_waves(d->waves ? d->waves : skinny_waves(drole, prologue, dt, c.model_dim), prologue);
		const size_t lds = skinny_lds_bytes(dt, decode_row_tiles(d->M), K, waves, prologue ? SKF_PROLOGUE : (fold ? SKF_FOLD : SKF_PLAIN));
		TTK_REQUIRE(d->family == 2 || lds <= CU_LDS_BYTES, TTK_E_ARG, "ttk_gemv_launch: M=%d K=%d with %d waves needs %zu bytes of LDS, a compute unit has %zu", d->M, K, waves, lds, CU_LDS_BYTES);
	}
	DecodeLaunch L = {};
	L.role = drole; L.W = &W->m; L.N = N; L.K = K; L.a = d->a;
	if (prologue) { L.ln_g = d->g1; L.ln_b = d->b1; L.ln2_g = d->g2; L.ln2_b = d->b2; L.x = d->x; L.ldx = K; }
	L.out_f32 = d->out_f32; L.out_T = d->out_T; L.kc = d->kcache; L.vc = d->vcache; L.bump = head && d->bump != 0;
	L.qbuf = d->qbuf; L.d_pos = d->d_pos; L.max_ctx = d->max_ctx; L.H = d->H;
	TTK_TRY(decode_launch(c, L, d->M, (hipStream_t)stream));
	TTK_HIP(hipGetLastError());
	return TTK_OK;
}
