"""DPM-Solver++(2M) on the CPU: the coefficient identities of `SpacedDiffusion.step_coefs_ms` in float64, the restatement of tests/dpmpp_ref.py over the oracle -- first
order is DDIM, second order converges as second order -- and the host side of the product (C ABI symbols, struct, argument errors), which needs no GPU.

Fixtures: tests/golden/diff_sampler_small*.npz (start noise and E; T = 40 and 136), DIFF_SMALL, network in f32.  Tolerances: TOL = 2e-4 is what test_sampler_ref.py holds
the DDIM restatement to on clamped outputs; unclamped the same figure relative to max|ref|.  The convergence bounds (0.5, 0.5, 2.5) are loose forms of what a second-order
solver does against a first-order one: measured 0.40 and 0.25 for the error ratios at 16 and 32 steps, 3.1-3.2 for halving the step (DDIM: 2.0)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpmpp_ref as M
import sampler_ref as R
import tortoise_oracle as O
from tortoise_tts_amd import _lib
from tortoise_tts_amd import diffusion as D
from tortoise_tts_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-4
FIXTURES = ["diff_sampler_small", "diff_sampler_small_t136"]


def t(a):
	return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
	a, b = a.double(), b.double()
	return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module", params=FIXTURES)
def case(request, golden):
	g = golden(request.param)
	return g, O.DiffusionOracle(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(g["seed"])), W.DIFF_SMALL)


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("n", [4, 6, 30, 80])
def test_coefficient_identities_in_f64(n):
	"""A constant x0 = 1 with x = alpha_i must land on alpha_{i-1}: c_x alpha_i + c_d0 + c_d1 == alpha_{i-1}; the first and the last step carry no history term."""
	d = D.get_diffuser(steps=n)
	s = R.schedule(n, True)
	alpha = np.sqrt(d.alphas_cumprod)
	alpha_prev = np.sqrt(d.alphas_cumprod_prev)
	for i in range(n):
		c = (0.0, 1.0, 0.0) if i == 0 else d._coefs_ms_f64(i)
		assert all(np.isfinite(c)), (i, c)
		assert abs(c[0] * alpha[i] + c[1] + c[2] - alpha_prev[i]) <= 1e-12, (i, c)
		assert np.allclose(c, M.coefs(s, i), rtol=1e-12, atol=1e-15), (i, c, M.coefs(s, i))      # the product's tables and the restatement's agree
		m = d.step_coefs_ms(i, True)
		got = (m.c_x, m.c_d0, m.c_d1)
		assert all(np.isfinite(got)) and np.array_equal(np.float32(c), np.float32(got)) and m.clip == 1
		if i in (0, n - 1):
			assert c[2] == 0.0 and m.c_d1 == 0.0
		else:
			assert c[2] < 0.0 < c[1]          # extrapolation: more than c_d of this x0, less of the previous one
	m = d.step_coefs_ms(0, False)
	assert (m.c_x, m.c_d0, m.c_d1, m.clip) == (0.0, 1.0, 0.0, 0)
	with pytest.raises(IndexError):
		d.step_coefs_ms(n, True)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("clip", [True, False])
def test_first_order_is_ddim(case, clip, cf):
	g, model = case
	s = R.schedule(6, cf)
	x, E = t(g["start"]), t(g["E"])
	with torch.inference_mode():
		ref = R.loop(s, model, x, E, eta=0.0, clip=clip, noises=[0.0] * 6)
		got = M.loop(s, model, x, E, clip=clip, first_order=True)
		second = M.loop(s, model, x, E, clip=clip)
	scale = 1.0 if clip else max(1.0, ref.abs().max().item())
	err = (got.double() - ref.double()).abs().max().item()
	print(f"first order vs ddim T={x.shape[-1]} clip={clip} cf={cf}: max|err| {err:.3e}, max|ref| {ref.abs().max().item():.3e}")
	assert err <= TOL * scale, (err, scale)
	assert (second.double() - ref.double()).abs().max().item() > 10 * TOL * scale      # ... and the history term is not nothing


@pytest.fixture(scope="module")
def truth(case):
	"""the 500-step DDIM restatement, unclamped, no guidance: computed once per fixture"""
	g, model = case
	with torch.inference_mode():
		return R.loop(R.schedule(500, False), model, t(g["start"]), t(g["E"]), eta=0.0, clip=False, noises=[0.0] * 500)


def test_convergence_is_second_order(case, truth):
	g, model = case
	x, E = t(g["start"]), t(g["E"])
	err = {}
	with torch.inference_mode():
		for n in (16, 32):
			s = R.schedule(n, False)
			err["ddim", n] = rel_l2(R.loop(s, model, x, E, eta=0.0, clip=False, noises=[0.0] * n), truth)
			err["2m", n] = rel_l2(M.loop(s, model, x, E, clip=False), truth)
	print(f"T={x.shape[-1]}: " + ", ".join(f"{k[0]}({k[1]}) {v:.3e}" for k, v in err.items()))
	assert err["2m", 16] <= 0.5 * err["ddim", 16], err
	assert err["2m", 32] <= 0.5 * err["ddim", 32], err
	assert err["2m", 16] / err["2m", 32] >= 2.5, err


def test_f32_coefficients_follow_the_f64_form(case):
	"""the product hands the kernel f32 scalars: over 6 steps that moves the result by no more than the DDIM restatement's own tolerance"""
	g, model = case
	s = R.schedule(6, True)
	x, E = t(g["start"]), t(g["E"])
	with torch.inference_mode():
		for clip in (True, False):
			a, b = M.loop(s, model, x, E, clip=clip), M.loop(s, model, x, E, clip=clip, f32_coefs=True)
			assert (a.double() - b.double()).abs().max().item() <= TOL * (1.0 if clip else max(1.0, a.abs().max().item()))


def test_kernel_restatement_reduces_to_its_parts():
	"""step_ms_numpy: c_d1 == 0 never looks at the history (NaN there stays out), (0, 1, 0) returns x0, and x0 is step_ext_numpy's"""
	gen = np.random.default_rng(0)
	out_c, out_u = gen.standard_normal((2, 8, 5)).astype(np.float32), gen.standard_normal((2, 8, 5)).astype(np.float32)
	x = gen.standard_normal((2, 4, 5)).astype(np.float32)
	d = D.get_diffuser(steps=6)
	st = d.step_coefs(3, "ddim")
	nan = np.full_like(x, np.nan)
	first = d.step_coefs_ms(5, True)
	xn, x0 = M.step_ms_numpy(out_c, out_u, x, nan, st, first)
	assert np.isfinite(xn).all() and np.array_equal(x0, R.step_ext_numpy(out_c, out_u, x, None, st, d.step_coefs_ext(3, 0, 0.0, True))[1])
	last = d.step_coefs_ms(0, True)
	xn, x0 = M.step_ms_numpy(out_c, out_u, x, nan, st, last)
	assert np.array_equal(xn, x0 + np.float32(0) * x)
	mid = d.step_coefs_ms(3, True)
	hist = gen.standard_normal(x.shape).astype(np.float32)
	xn = M.step_ms_numpy(out_c, out_u, x, hist, st, mid)[0]
	want = mid.c_x * x.astype(np.float64) + mid.c_d0 * x0.astype(np.float64) + mid.c_d1 * hist.astype(np.float64)
	assert np.abs(xn - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ the product's host side
NEW = {"ttk_diff_sample_ms", "ttk_diff_sample_ms_lines", "ttk_diff_step_ms", "ttk_diffusion_step_ms_rows"}


def test_header_symbols_and_struct_size_agree():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert NEW <= declared and declared == set(_lib.SYMBOLS)
	lib = _lib.load()
	for name in NEW:
		assert hasattr(lib, name)
	body = re.search(r"typedef struct \{([^}]*)\} ttk_step_ms;", header).group(1)
	body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
	fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
	assert fields == [n for n, _ in _lib.StepMsC._fields_] == ["c_x", "c_d0", "c_d1", "clip"]
	assert ctypes.sizeof(_lib.StepMsC) == 16                   # static_assert'ed in csrc/diff.hip
	assert ctypes.sizeof(_lib.StepC) == 56 and ctypes.sizeof(_lib.StepExtC) == 24      # the existing structs are not touched


def test_argument_errors_without_a_gpu():
	d = D.get_diffuser(steps=4)
	x = torch.zeros(1, 100, 8)
	kw = {"precomputed_aligned_embeddings": x}
	with pytest.raises(ValueError, match="eta must be 0"):
		d.sample_loop(None, (1, 100, 8), sampler="dpm++2m", eta=0.5, model_kwargs=kw)
	for name in ("dpm++2s", "heun", "dpm++2m_sde"):
		with pytest.raises(RuntimeError, match="Sampler not implemented"):
			d.sample_loop(None, (1, 100, 8), sampler=name, model_kwargs=kw)
	with pytest.raises(_lib.TTKError, match="no fallback"):
		d.sample_loop(object(), (1, 100, 8), sampler="DPM++2M", model_kwargs=kw)      # the name is accepted (any case): the next check is the model's
	with pytest.raises(NotImplementedError, match="host round trip"):
		d.dpmpp_sample_loop_progressive(None, (1, 100, 8), denoised_fn=lambda v: v)
	with pytest.raises(RuntimeError, match="Sampler not implemented"):
		d.sample_loop_lines(None, [x], [x], sampler="p")
	from tortoise_tts_amd.inference import check_sampler_eta
	check_sampler_eta("ddim", 0.5), check_sampler_eta("p", 1.0), check_sampler_eta("dpm++2m", 0.0)
	with pytest.raises(ValueError, match="diffusion_eta must be 0"):
		check_sampler_eta("dpm++2m", 0.5)
	# the library refuses what concerns `ms` before it looks at the handle or the device (the buffers are never read: any non-null address will do)
	lib = _lib.load()
	buf = (ctypes.c_float * 4)()
	p = ctypes.addressof(buf)
	st = d.step_coefs(3, "ddim")
	st.cfk = -1.0
	steps = (_lib.StepC * 4)(*[d.step_coefs(i, "ddim") for i in range(4)])
	ms = (_lib.StepMsC * 4)(*[d.step_coefs_ms(i, True) for i in range(4)])
	tlen = (ctypes.c_int * 1)(1)
	assert lib.ttk_diff_sample_ms(None, p, p, 1, 1, steps, None, 4, None) != 0 and b"null ms" in lib.ttk_last_error()
	assert lib.ttk_diff_sample_ms_lines(None, p, p, 1, 64, tlen, steps, None, 4, None) != 0 and b"null ms" in lib.ttk_last_error()
	assert lib.ttk_diff_step_ms(None, p, p, ctypes.byref(st), None, None, None) != 0 and b"null ms" in lib.ttk_last_error()
	assert lib.ttk_diffusion_step_ms_rows(p, None, p, p, None, 1, 1, 1, ctypes.byref(st), None, None, 0, 0, 0, None) != 0 and b"null ms" in lib.ttk_last_error()
	ms[3].c_d1 = -0.25                  # the first step to run has no history
	assert lib.ttk_diff_sample_ms(None, p, p, 1, 1, steps, ms, 4, None) != 0 and b"no history yet" in lib.ttk_last_error()
	assert lib.ttk_diff_sample_ms_lines(None, p, p, 1, 64, tlen, steps, ms, 4, None) != 0 and b"no history yet" in lib.ttk_last_error()
	mid = d.step_coefs_ms(2, True)
	assert mid.c_d1 != 0.0
	assert lib.ttk_diff_step_ms(None, p, None, ctypes.byref(st), ctypes.byref(mid), None, None) != 0 and b"history, which is null" in lib.ttk_last_error()
	assert lib.ttk_diffusion_step_ms_rows(p, None, p, None, None, 1, 1, 1, ctypes.byref(st), ctypes.byref(mid), None, 0, 0, 0, None) != 0
	assert b"history, which is null" in lib.ttk_last_error()
	# with a good `ms` the remaining checks are the existing ones
	ms[3].c_d1 = 0.0
	assert lib.ttk_diff_sample_ms(None, p, p, 1, 1, steps, ms, 4, None) != 0 and b"bad argument" in lib.ttk_last_error()
	st.cfk = 1.0
	assert lib.ttk_diffusion_step_ms_rows(p, None, p, p, None, 1, 1, 1, ctypes.byref(st), ctypes.byref(mid), None, 0, 0, 0, None) != 0 and b"out_u" in lib.ttk_last_error()
