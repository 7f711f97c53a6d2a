// How far is the device's __sinf (v_sin_f32 behind a multiply by 1 / 2 pi) from the sine of its f32 argument?  The bf16 form of csrc/voc.hip's k_snake_aa takes
// its sin(up * a) from it, and tests/voc_ref.py needs the absolute error over the argument range its snake cases produce.  The intrinsic alone is measured, not
// the kernel: N arguments evenly spaced over [-R, R] (default R = 16, N = 2^26: every 4.8e-7, an f32 ulp at 4 .. 8), each compared on the host with sin() of the
// same f32 value in double.  Prints the worst absolute error, its argument, and the worst error per unit interval of |x|.  The sweep samples the range, it does
// not visit every float: voc_ref.py doubles the figure.
//   hipcc --offload-arch=gfx950 -O3 tests/diag/sinf_probe.cpp -o tests/diag/sinf_probe.bin && tests/diag/sinf_probe.bin [R [log2 N]]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define CHECK(e)                                                                                   \
	do {                                                                                           \
		hipError_t _e = (e);                                                                       \
		if (_e != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } \
	} while (0)

__global__ void k_sin(const float* x, float* fast, float* accurate, int n) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	fast[i] = __sinf(x[i]);
	accurate[i] = sinf(x[i]);
}

int main(int argc, char** argv) {
	const double R = argc > 1 ? atof(argv[1]) : 16.0;
	const int lg = argc > 2 ? atoi(argv[2]) : 26;
	if (!(R > 0 && R <= 1024) || lg < 10 || lg > 26) { fprintf(stderr, "usage: sinf_probe [R in (0, 1024]] [log2 N in 10..26]\n"); return 2; }
	const int n = 1 << lg, chunk = 1 << 22;
	const int buckets = (int)ceil(R);
	std::vector<double> worst_fast(buckets, 0.0), worst_acc(buckets, 0.0);
	std::vector<float> hx(chunk), hf(chunk), ha(chunk);
	float *dx = nullptr, *df = nullptr, *da = nullptr;
	CHECK(hipMalloc(&dx, chunk * sizeof(float)));
	CHECK(hipMalloc(&df, chunk * sizeof(float)));
	CHECK(hipMalloc(&da, chunk * sizeof(float)));
	double wf = 0, wa = 0, xf = 0, xa = 0;
	for (int base = 0; base < n; base += chunk) {
		const int m = n - base < chunk ? n - base : chunk;
		for (int i = 0; i < m; ++i) hx[i] = (float)(-R + 2.0 * R * ((double)(base + i) + 0.5) / (double)n);
		CHECK(hipMemcpy(dx, hx.data(), m * sizeof(float), hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_sin, dim3((m + 255) / 256), dim3(256), 0, 0, dx, df, da, m);
		CHECK(hipGetLastError());
		CHECK(hipMemcpy(hf.data(), df, m * sizeof(float), hipMemcpyDeviceToHost));
		CHECK(hipMemcpy(ha.data(), da, m * sizeof(float), hipMemcpyDeviceToHost));
		for (int i = 0; i < m; ++i) {
			const double want = sin((double)hx[i]);
			const double ef = fabs((double)hf[i] - want), ea = fabs((double)ha[i] - want);
			int b = (int)fabs((double)hx[i]);
			if (b >= buckets) b = buckets - 1;
			if (ef > worst_fast[b]) worst_fast[b] = ef;
			if (ea > worst_acc[b]) worst_acc[b] = ea;
			if (ef > wf) { wf = ef; xf = hx[i]; }
			if (ea > wa) { wa = ea; xa = hx[i]; }
			if (!(ef == ef)) { fprintf(stderr, "__sinf(%.9g) is not a number\n", hx[i]); return 1; }
		}
	}
	printf("arguments: %d evenly spaced over [-%g, %g]\n", n, R, R);
	printf("__sinf: worst |error| %.6e at x = %.9g\n", wf, xf);
	printf("sinf:   worst |error| %.6e at x = %.9g\n", wa, xa);
	for (int b = 0; b < buckets; ++b) printf("  %2d <= |x| < %2d: __sinf %.3e   sinf %.3e\n", b, b + 1, worst_fast[b], worst_acc[b]);
	(void)hipFree(dx); (void)hipFree(df); (void)hipFree(da);
	return 0;
}
