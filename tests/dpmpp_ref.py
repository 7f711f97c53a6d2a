"""Helper of test_dpmpp_ref.py / test_gpu_dpmpp.py (not a test module): DPM-Solver++(2M) (Lu et al. 2022, data prediction, multistep) restated twice -- the loop in float64
over `O.DiffusionOracle` with `sampler_ref.mean_variance` for x0, written from the formulas alone (no import from the package), and the update kernel in numpy f32 with the
kernel's own operation order (csrc/elementwise.hip: k_diffusion_step_ms)."""
import numpy as np
import torch

import sampler_ref as R


def coefs(s, i, first_order=False):
	"""(c_x, c_d0, c_d1) of step i (level i -> level i - 1) in float64 on the schedule `s`: alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma);
	h = lambda_{i-1} - lambda_i, c_x = sigma_{i-1} / sigma_i, c_d = -alpha_{i-1} expm1(-h); no history at i = n-1; (0, 1, 0) at i = 0, where the target is alpha_bar = 1."""
	n = s.num_timesteps
	if i == 0:
		return 0.0, 1.0, 0.0
	ab = np.asarray(s.alphas_cumprod, np.float64)
	alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
	lam = np.log(alpha) - np.log(sigma)
	h = lam[i - 1] - lam[i]
	c_x = sigma[i - 1] / sigma[i]
	c_d = -alpha[i - 1] * np.expm1(-h)
	if i == n - 1 or first_order:
		return float(c_x), float(c_d), 0.0
	r = (lam[i] - lam[i + 1]) / h
	return float(c_x), float(c_d * (1.0 + 0.5 / r)), float(-c_d * 0.5 / r)


def loop_progressive(s, model, x, E, clip=True, first_order=False, f32_coefs=False):
	"""every step's {"sample", "pred_xstart"}, index n-1 .. 0.  The network and x0 are the oracle's f32 (`sampler_ref.mean_variance`); the update is made in float64 and x
	rounded to f32 once per step.  first_order: every c_d1 = 0, which is DDIM.  f32_coefs: the coefficients rounded to f32 first, as the product passes them."""
	outs, prev = [], None
	for i in reversed(range(s.num_timesteps)):
		_, _, x0 = R.mean_variance(s, model, x, i, E, clip)
		c_x, c_d0, c_d1 = coefs(s, i, first_order)
		if f32_coefs:
			c_x, c_d0, c_d1 = (float(np.float32(v)) for v in (c_x, c_d0, c_d1))
		xn = c_x * x.double() + c_d0 * x0.double()
		if c_d1 != 0.0:
			xn = xn + c_d1 * prev.double()
		prev = x0
		x = xn.float()
		outs.append(dict(sample=x, pred_xstart=x0))
	return outs


def loop(s, model, x, E, **kw):
	return loop_progressive(s, model, x, E, **kw)[-1]["sample"]


def step_ms_numpy(out_c, out_u, x, hist, st, ms):
	"""k_diffusion_step_ms on numpy f32 arrays with the kernel's operation order: the guidance mix and c_x x rounded singly, x0 and the two accumulations as exact fmaf.
	out_c / out_u [nb, 2C, T], x / hist [nb, C, T] (hist is not looked at when c_d1 == 0); st / ms: the ctypes structs.  Returns (x_new, x0): x0 is pred_xstart and the
	history after the call."""
	f = np.float32
	C = x.shape[1]
	eps = out_c[:, :C].astype(f)
	cfk = f(st.cfk)
	if cfk >= 0:
		eps = (f(1) + cfk) * eps - cfk * out_u[:, :C].astype(f)
	rx = f(st.sqrt_recip_ac) * x
	x0 = R.fma32(-f(st.sqrt_recipm1_ac), eps, rx)
	if ms.clip:
		x0 = np.minimum(np.maximum(x0, f(-1)), f(1))
	xn = R.fma32(f(ms.c_d0), x0, f(ms.c_x) * x)
	if ms.c_d1 != 0:
		xn = R.fma32(f(ms.c_d1), hist, xn)
	return xn.astype(f), x0.astype(f)
