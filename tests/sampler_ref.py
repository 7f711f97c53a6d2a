"""Helper of test_sampler_ref.py / test_gpu_sampler_ext.py (not a test module): the sampler forms the oracle's `SpacedSchedule` does not carry -- DDIM with eta,
clip_denoised=False, ddim_reverse_sample, the loops over them -- restated in plain torch over `O.DiffusionOracle` (reference: models/diffusion.py:325-431, 510-554,
646-732), and the update kernel restated in numpy f32 with the kernel's own operation order (csrc/elementwise.hip: k_diffusion_step_ext)."""
import numpy as np
import torch

import tortoise_oracle as O


def schedule(steps, cond_free):
	s = O.SpacedSchedule(steps=steps, cond_free=cond_free)
	s.alphas_cumprod_next = np.append(s.alphas_cumprod[1:], 0.0)      # diffusion.py:227
	return s


def mean_variance(s, model, x, i, E, clip=True):
	"""`SpacedSchedule.p_mean_variance` with clip_denoised as an argument (diffusion.py:398-403) -> (mean, log_var, pred_xstart)."""
	b, C = x.shape[:2]
	t = torch.tensor([s.timestep_map[i]] * b)
	eps, var_values = torch.split(model.forward(x, t, E), C, dim=1)
	frac = (var_values + 1) / 2
	log_var = frac * s._f(np.log(s.betas), i) + (1 - frac) * s._f(s.posterior_log_variance_clipped, i)
	if s.conditioning_free:
		eps_u, _ = torch.split(model.forward(x, t, E, conditioning_free=True), C, dim=1)
		cfk = s.conditioning_free_k * (1 - i / s.num_timesteps)
		eps = (1 + cfk) * eps - cfk * eps_u
	x0 = s._f(s.sqrt_recip_alphas_cumprod, i) * x - s._f(s.sqrt_recipm1_alphas_cumprod, i) * eps
	if clip:
		x0 = x0.clamp(-1, 1)
	mean = s._f(s.posterior_mean_coef1, i) * x0 + s._f(s.posterior_mean_coef2, i) * x
	return mean, log_var, x0


def coefs(s, i, eta):
	"""(sigma, sqrt(1 - ab_prev - sigma^2), sqrt(ab_next), sqrt(1 - ab_next)) as 0-dim f32 tensors (:677-688, :724-729)."""
	ab, ab_prev, ab_next = s._f(s.alphas_cumprod, i), s._f(s.alphas_cumprod_prev, i), s._f(s.alphas_cumprod_next, i)
	sigma = eta * torch.sqrt((1 - ab_prev) / (1 - ab)) * torch.sqrt(1 - ab / ab_prev)
	return sigma, torch.sqrt(1 - ab_prev - sigma ** 2), torch.sqrt(ab_next), torch.sqrt(1 - ab_next)


def _eps(s, x, i, x0):
	return (s._f(s.sqrt_recip_alphas_cumprod, i) * x - x0) / s._f(s.sqrt_recipm1_alphas_cumprod, i)


def ddim_step(s, model, x, i, E, eta=0.0, clip=True, noise=None):
	"""ddim_sample (:646-694); noise None draws the step's randn_like where the reference does."""
	_, _, x0 = mean_variance(s, model, x, i, E, clip)
	eps = _eps(s, x, i, x0)
	sigma, direction, _, _ = coefs(s, i, eta)
	if noise is None:
		noise = torch.randn_like(x)
	sample = x0 * torch.sqrt(s._f(s.alphas_cumprod_prev, i)) + direction * eps + (0.0 if i == 0 else 1.0) * sigma * noise
	return dict(sample=sample, pred_xstart=x0)


def p_step(s, model, x, i, E, clip=True, noise=None):
	"""p_sample (:510-554)."""
	mean, log_var, x0 = mean_variance(s, model, x, i, E, clip)
	if noise is None:
		noise = torch.randn_like(x)
	return dict(sample=mean + (0.0 if i == 0 else 1.0) * torch.exp(0.5 * log_var) * noise, pred_xstart=x0)


def reverse_step(s, model, x, i, E, clip=True):
	"""ddim_reverse_sample (:696-732)."""
	_, _, x0 = mean_variance(s, model, x, i, E, clip)
	eps = _eps(s, x, i, x0)
	_, _, sq_next, sq_1m_next = coefs(s, i, 0.0)
	return dict(sample=x0 * sq_next + sq_1m_next * eps, pred_xstart=x0)


def loop_progressive(s, model, x, E, sampler="ddim", eta=0.0, clip=True, noises=None):
	"""every step's dict, index n-1 .. 0 (:602-644, :768-810); noises: [n, ...] blocks in loop order, None draws them"""
	outs = []
	for j, i in enumerate(reversed(range(s.num_timesteps))):
		nz = None if noises is None else noises[j]
		out = ddim_step(s, model, x, i, E, eta, clip, nz) if sampler == "ddim" else p_step(s, model, x, i, E, clip, nz)
		outs.append(out)
		x = out["sample"]
	return outs


def loop(s, model, x, E, **kw):
	return loop_progressive(s, model, x, E, **kw)[-1]["sample"]


def reverse_loop(s, model, x, E, clip=True):
	"""ddim_reverse_sample at index 0 .. n-1 (the reference has the step but no loop over it)."""
	for i in range(s.num_timesteps):
		x = reverse_step(s, model, x, i, E, clip)["sample"]
	return x


# ------------------------------------------------------------------------------------------------ the update kernel in numpy f32
def fma32(a, b, c):
	"""fmaf(a, b, c) on f32 arrays, exactly: the product of two f32 is exact in f64; the f64 sum is made round-to-odd from its exact error term (two-sum), and a
	round-to-odd f64 rounds to the nearest f32 as the infinitely precise value does (53 >= 2 * 24 + 2)."""
	p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
	c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
	s = p + c
	bb = s - p
	err = (p - (s - bb)) + (c - bb)
	inexact_even = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
	toward = np.where((err > 0), np.inf, -np.inf)
	s = np.where(inexact_even, np.nextafter(s, toward), s)
	return s.astype(np.float32)


def step_ext_numpy(out_c, out_u, x, noise, st, ext):
	"""k_diffusion_step_ext on numpy f32 arrays with the kernel's operation order: every product and sum rounded on its own, except the two sums the kernel fuses by
	name (x0 and the posterior mean).  out_c / out_u [nb, 2C, T], x / noise [nb, C, T]; st / ext: the ctypes structs.  Returns (x_new, pred_xstart).
	Mode 1 with noise multiplies it by expf(0.5 log_var), which the device evaluates with its exp2 instruction (not correctly rounded, so no host can restate its last
	bit): that case returns (posterior mean, pred_xstart, 0.5 * log_var) and the caller finishes x_new = mean + e * noise for the candidate values e of the exponential."""
	f = np.float32
	C = x.shape[1]
	eps = out_c[:, :C].astype(f)
	cfk = f(st.cfk)
	if cfk >= 0:
		eps = (f(1) + cfk) * eps - cfk * out_u[:, :C].astype(f)
	rx = f(st.sqrt_recip_ac) * x
	x0 = fma32(-f(st.sqrt_recipm1_ac), eps, rx)
	if ext.clip:
		x0 = np.minimum(np.maximum(x0, f(-1)), f(1))
	if ext.mode == 1:
		frac = (out_c[:, C:].astype(f) + f(1)) / f(2)
		log_var = frac * f(st.max_log) + (f(1) - frac) * f(st.min_log)
		mean = fma32(f(st.coef2), x, f(st.coef1) * x0)
		half = f(0.5) * log_var
		if not st.nonzero:
			return mean + f(0), x0
		return mean, x0, half
	e2 = (rx - x0) / f(st.sqrt_recipm1_ac)
	if ext.mode == 0:
		xn = x0 * f(st.sqrt_ac_prev) + f(ext.dir) * e2
		if st.nonzero and ext.sigma != 0:
			xn = xn + f(ext.sigma) * noise
	else:
		xn = x0 * f(ext.sqrt_ac_next) + f(ext.sqrt_1m_ac_next) * e2
	return xn.astype(f), x0
