"""The extended sampler on the CPU: tests/sampler_ref.py (plain torch over the oracle) against vectors the reference's own `SpacedDiffusion` produced
(tools/make_golden_sampler.py -> tests/golden/diff_sampler_small*.npz), and the host side of the product -- the per-step scalars, the C ABI's structs and symbols,
argument errors -- which needs no GPU.

Tolerance of the restatement: 2e-4, what test_oracle_golden.py::test_diff_small holds the oracle's DDIM / p loops to against diff_small.npz (same model size, 4 steps,
outputs bounded by 1).  The *_noclip outputs are not bounded by 1 (the unclamped x0 of a synthetic network grows to ~2e3): there the same number is taken relative
to max|ref|, the form `close(..., rtol)` of that file has."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

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


def close(a, b, tol=TOL, rel=False):
	a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
	err = (a - b).abs().max().item()
	bound = tol * (max(1.0, b.abs().max().item()) if rel else 1.0)
	assert err <= bound, f"max abs err {err:.3e} > {bound:.3e}"
	return err


@pytest.fixture(scope="module", params=FIXTURES)
def case(request, golden):
	g = golden(request.param)
	model = O.DiffusionOracle(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(g["seed"])), W.DIFF_SMALL)
	with torch.inference_mode():
		close(model.timestep_independent(t(g["latents"]), t(g["cond"]), int(g["T"])), g["E"], 2e-5)
	return g, model


def test_fixture_lengths_cover_less_than_a_tile_and_two_tiles_plus_a_remainder(golden):
	assert [int(golden(n)["T"]) for n in FIXTURES] == [40, 136]


@pytest.mark.parametrize("key,steps,cf,eta", [("ddim_eta05", 5, True, 0.5), ("ddim_eta1", 6, False, 1.0)])
def test_ddim_eta_restatement(case, key, steps, cf, eta):
	g, model = case
	s = R.schedule(steps, cf)
	with torch.inference_mode():
		close(R.loop(s, model, t(g["start"]), t(g["E"]), eta=eta, noises=t(g["step_noise"])), g[key])
		close(R.loop(s, model, t(g["start"]), t(g["E"]), eta=0.0, noises=t(g["step_noise"])), g[key + "_eta0"])
		# the bank is what the reference drew: the same loop drawing from the seeded generator itself
		torch.manual_seed(int(g["sampler_seed"]))
		close(R.loop(s, model, t(g["start"]), t(g["E"]), eta=eta), g[key])


@pytest.mark.parametrize("key,sampler", [("ddim_noclip", "ddim"), ("p_noclip", "p")])
def test_unclipped_restatement(case, key, sampler):
	g, model = case
	s = R.schedule(5, True)
	x = float(g["noclip_scale"]) * t(g["start"])
	with torch.inference_mode():
		outs = R.loop_progressive(s, model, x, t(g["E"]), sampler=sampler, clip=False, noises=t(g["step_noise"]))
		close(outs[-1]["sample"], g[key], rel=True)
		assert max((o["pred_xstart"].abs() > 1).float().mean().item() for o in outs) >= 0.10      # the clamp would bite: the fixture's own condition
		clipped = R.loop(s, model, x, t(g["E"]), sampler=sampler, clip=True, noises=t(g["step_noise"]))
		assert (clipped - t(g[key])).abs().max() > 1.0


@pytest.mark.parametrize("cf", [False, True])
def test_reverse_restatement(case, cf):
	g, model = case
	with torch.inference_mode():
		close(R.reverse_loop(R.schedule(5, cf), model, t(g["mel"]), t(g["E"])), g[f"reverse_cf{int(cf)}"])


def test_roundtrip_restatement(case):
	"""reverse then ddim, unclamped: the restatement's reconstruction error is the reference's own (a synthetic network is no denoiser: the error is large, and equal)"""
	g, model = case
	s = R.schedule(5, False)
	with torch.inference_mode():
		xT = R.reverse_loop(s, model, t(g["mel"]), t(g["E"]), clip=False)
		back = R.loop(s, model, xT, t(g["E"]), eta=0.0, clip=False, noises=t(g["step_noise"]))
	err = (back - t(g["mel"])).abs().max().item()
	assert abs(err - float(g["roundtrip_err"])) <= TOL * max(1.0, float(g["roundtrip_err"]))


def test_progressive_restatement(golden):
	g = golden("diff_sampler_small")
	model = O.DiffusionOracle(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(g["seed"])), W.DIFF_SMALL)
	with torch.inference_mode():
		outs = R.loop_progressive(R.schedule(4, True), model, t(g["start"]), t(g["E"]), eta=0.5, noises=t(g["step_noise"]))
	assert len(outs) == 4
	for j, o in enumerate(outs):
		close(o["sample"], g["prog_sample"][j])
		close(o["pred_xstart"], g["prog_pred_xstart"][j])


# ------------------------------------------------------------------------------------------------ the product's host side
def bits(x):
	return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n,eta", [(4, 0.5), (5, 0.5), (5, 0.0), (6, 1.0)])
def test_step_coefs_ext_equal_the_references_f32_scalars_bit_for_bit(golden, n, eta):
	g = golden("diff_sampler_small")
	ref = g[f"coef_{n}_eta{eta}"]
	d = D.get_diffuser(steps=n)
	s = R.schedule(n, True)
	for i in range(n):
		e = d.step_coefs_ext(i, 0, eta, True)
		got = [e.sigma, e.dir, e.sqrt_ac_next, e.sqrt_1m_ac_next]
		assert np.array_equal(bits(got), bits(ref[i])), (i, got, ref[i])
		assert np.array_equal(bits([float(v) for v in R.coefs(s, i, eta)]), bits(ref[i]))      # ... and so does the restatement
	assert np.array_equal(d.alphas_cumprod_next, np.append(d.alphas_cumprod[1:], 0.0))


@pytest.mark.parametrize("n", [4, 5, 6, 80])
def test_eta_zero_is_the_existing_step_and_index_zero_adds_no_noise(n):
	d = D.get_diffuser(steps=n)
	for i in range(n):
		e = d.step_coefs_ext(i, 0, 0.0, True)
		assert e.sigma == 0.0 and bits(e.dir) == bits(d.step_coefs(i, "ddim").sqrt_1m_ac_prev)
		assert (e.mode, e.clip) == (0, 1) and d.step_coefs_ext(i, 2, 0.0, False).clip == 0
	for eta in (0.3, 0.7, 1.0):
		assert d.step_coefs_ext(0, 0, eta, True).sigma == 0.0
		assert d.step_coefs_ext(n - 1, 0, eta, True).sigma > 0.0


def test_header_symbols_and_struct_sizes_agree():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	new = {"ttk_diff_sample_ext", "ttk_diff_step_ext", "ttk_diffusion_step_ext_rows"}
	assert new <= declared and declared == set(_lib.SYMBOLS)
	lib = _lib.load()
	for name in new:
		assert hasattr(lib, name)
	body = re.search(r"typedef struct \{([^}]*)\} ttk_step_ext;", header).group(1)
	body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
	fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
	assert fields == [n for n, _ in _lib.StepExtC._fields_] == ["sigma", "dir", "sqrt_ac_next", "sqrt_1m_ac_next", "mode", "clip"]
	assert ctypes.sizeof(_lib.StepExtC) == 4 * 4 + 2 * 4       # static_assert'ed in csrc/diff.hip
	assert ctypes.sizeof(_lib.StepC) == 56                     # ttk_step is not touched


def test_argument_errors():
	d = D.get_diffuser(steps=4)
	x = torch.zeros(1, 100, 8)
	with pytest.raises(AssertionError, match="deterministic"):
		d.ddim_reverse_sample(None, x, torch.tensor([1]), eta=0.5)
	for call in (lambda: d.sample_loop(None, (1, 100, 8), denoised_fn=lambda v: v),
				 lambda: d.sample_loop(None, (1, 100, 8), cond_fn=lambda *a: 0),
				 lambda: d.ddim_sample(None, x, torch.tensor([1]), denoised_fn=lambda v: v),
				 lambda: d.p_sample_loop_progressive(None, (1, 100, 8), cond_fn=lambda *a: 0)):
		with pytest.raises(NotImplementedError, match="host round trip"):
			call()
	with pytest.raises(_lib.TTKError, match="no fallback"):
		d.sample_loop(object(), (1, 100, 8), eta=0.5, model_kwargs={"precomputed_aligned_embeddings": x})
	with pytest.raises(ValueError, match="repeated"):
		d._index_of(torch.tensor([1, 2]), 2)
	with pytest.raises(IndexError):
		d._index_of(torch.tensor([4]), 1)
	# the library refuses a step that adds noise without a noise block, before anything is launched (the buffers are never read: any non-null address will do)
	lib = _lib.load()
	buf = (ctypes.c_float * 4)()
	p = ctypes.addressof(buf)
	st = d.step_coefs(3, "ddim")

	def rows(ext, noise, step=st):
		return lib.ttk_diffusion_step_ext_rows(p, None, p, noise, None, 1, 1, 1, ctypes.byref(step), ctypes.byref(ext), None, 0, 0, 0, None)
	st.cfk = -1.0
	assert rows(d.step_coefs_ext(3, 0, 0.5, True), None) != 0 and b"noise is null" in lib.ttk_last_error()
	assert rows(d.step_coefs_ext(3, 1, 0.0, True), None) != 0 and b"noise is null" in lib.ttk_last_error()
	bad = d.step_coefs_ext(3, 0, 0.0, True)
	bad.mode = 3
	assert rows(bad, None) != 0 and b"mode 3" in lib.ttk_last_error()
	st.cfk = 1.0
	assert rows(d.step_coefs_ext(3, 2, 0.0, True), None) != 0 and b"out_u" in lib.ttk_last_error()      # guidance mix without the second evaluation
	assert lib.ttk_diff_sample_ext(None, p, p, 1, 1, ctypes.byref(st), None, 1, None, None) != 0
