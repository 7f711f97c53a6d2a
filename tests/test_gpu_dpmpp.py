"""DPM-Solver++(2M) on the GPU (include/ttk.h: ttk_step_ms, ttk_diff_sample_ms, ttk_diff_sample_ms_lines, ttk_diff_step_ms, ttk_diffusion_step_ms_rows;
tortoise_tts_amd/diffusion.py: sample_loop(sampler="dpm++2m"), dpmpp_sample_loop_progressive, sample_loop_lines(sampler=)): the update kernel alone bit for bit against
the numpy f32 restatement of tests/dpmpp_ref.py, the f32 loop against the float64 restatement over the oracle, the bit-for-bit identities between the entries, forced
first order against the DDIM entry, convergence order on the device, bf16 beside the existing bf16 loop, the generator position, and `TTS.inference`.
DIFF_SMALL, T = 40 and 136 (less than a tile; two tiles and a remainder), the start noise and E of tests/golden/diff_sampler_small*.npz.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import dpmpp_ref as M
import sampler_ref as R
import tortoise_oracle as O
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W
from test_gpu_sampler_ext import DEV, F32_TOL, FIXTURES, clip, diffuser, fx, kw, maxerr, models, relerr, t, tts      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
	return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def ms_array(d, clip_, first_order=False):
	n = d.num_timesteps
	ms = (_lib.StepMsC * n)(*[d.step_coefs_ms(i, clip_) for i in range(n)])
	if first_order:      # c_d1 = 0 and this step's x0 takes the whole weight c_d = c_d0 + c_d1 (summed in float64)
		for i in range(1, n - 1):
			_, c_d0, c_d1 = d._coefs_ms_f64(i)
			ms[i].c_d0, ms[i].c_d1 = np.float32(c_d0 + c_d1), 0.0
	return ms


def run(d, model, g, clip_=True, **extra):
	return d.sample_loop(model, (1, 100, g["start"].shape[-1]), noise=g["start"], sampler="dpm++2m", clip_denoised=clip_, model_kwargs=kw(g), **extra)


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("cfk", [1.25, -1.0])
@pytest.mark.parametrize("clip_", [1, 0])
@pytest.mark.parametrize("nb,T", [(1, 40), (2, 136)])
def test_update_kernel_bit_for_bit(nb, T, clip_, cfk):
	"""nb C T = 4000 (15 blocks of 256 and a tail of 160) and 27200 (106 blocks and a tail of 64).  x, pred_xstart, the history after the call and the channels-last copy
	in f32 / f16 / bf16 equal the numpy f32 restatement (tests/dpmpp_ref.py: step_ms_numpy) bit for bit: at the first step (c_d1 = 0: the history holds NaN and must not
	be read), at a middle step (c_d1 != 0), and at index 0 ((0, 1, 0))."""
	lib = _lib.load()
	C, ldo, rep = 100, 128, 2
	gen = torch.Generator().manual_seed(1000 * nb + 10 * clip_ + int(cfk > 0))
	out_c, out_u = torch.randn(nb, 2 * C, T, generator=gen), torch.randn(nb, 2 * C, T, generator=gen)
	x0, hist0 = 1.5 * torch.randn(nb, C, T, generator=gen), torch.randn(nb, C, T, generator=gen)
	d = diffuser(6, True)
	dc, du = out_c.to(DEV), out_u.to(DEV)
	for i in (5, 3, 0):
		st, ms = d.step_coefs(i, "ddim"), d.step_coefs_ms(i, bool(clip_))
		st.cfk = cfk
		assert (ms.c_d1 != 0.0) == (i == 3)
		h_in = hist0 if ms.c_d1 != 0.0 else torch.full_like(hist0, float("nan"))
		ref_x, ref_x0 = M.step_ms_numpy(out_c.numpy(), out_u.numpy(), x0.numpy(), h_in.numpy(), st, ms)
		assert np.isfinite(ref_x).all()
		if clip_ == 0:
			assert (np.abs(ref_x0) > 1).mean() > 0.1          # the clamp would have bitten
		for dt, tdt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
			x, hist = x0.to(DEV).clone(), h_in.to(DEV).clone()
			px = torch.full_like(x, 7.0)
			xcl = torch.full((rep * nb * T, ldo), 9.0, device=DEV, dtype=tdt)
			_lib.check(lib.ttk_diffusion_step_ms_rows(dc.data_ptr(), du.data_ptr() if cfk >= 0 else None, x.data_ptr(), hist.data_ptr(), px.data_ptr(), nb, C, T, ctypes.byref(st),
													  ctypes.byref(ms), xcl.data_ptr(), ldo, rep, _lib.DTYPES[dt], _lib.stream_ptr()), "ttk_diffusion_step_ms_rows")
			torch.cuda.synchronize()
			got = x.cpu().numpy()
			assert bits_equal(px.cpu().numpy(), ref_x0), (i, dt, "pred_xstart")
			assert bits_equal(hist.cpu().numpy(), ref_x0), (i, dt, "history")
			assert bits_equal(got, ref_x), (i, dt, np.abs(got - ref_x).max())
			want = x.permute(0, 2, 1).reshape(1, nb * T, C).expand(rep, -1, -1).reshape(rep * nb * T, C).to(tdt)      # row (q nb + b) T + t, column c
			assert torch.equal(xcl[:, :C], want) and bool((xcl[:, C:] == 9.0).all()), (i, dt, "channels-last copy")
		# without the optional outputs; without a history where the step reads none
		x, hist = x0.to(DEV).clone(), h_in.to(DEV).clone()
		_lib.check(lib.ttk_diffusion_step_ms_rows(dc.data_ptr(), du.data_ptr() if cfk >= 0 else None, x.data_ptr(), hist.data_ptr() if ms.c_d1 != 0.0 else None, None, nb, C, T,
												  ctypes.byref(st), ctypes.byref(ms), None, 0, 0, 0, _lib.stream_ptr()), "ttk_diffusion_step_ms_rows")
		assert bits_equal(x.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ f32 against the float64 restatement
@pytest.fixture(scope="module")
def oracle(golden):
	return O.DiffusionOracle(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(golden(FIXTURES[0])["seed"])), W.DIFF_SMALL)


@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("clip_", [True, False])
def test_f32_loop_against_the_f64_restatement(models, oracle, fx, clip_, cf):
	"""n = 6; bound F32_TOL = 3e-3 (what the project holds f32 DDIM loops to at this size), times max(1, max|ref|) unclamped.  Measured on an MI355X, max|err| at T = 40 | T = 136:
	  clamped, guidance      2.96e-5 | 7.00e-5
	  clamped, none          8.01e-5 | 1.28e-4
	  unclamped, guidance    4.27e-4 at max|ref| 8.1e2 | 4.88e-4 at 7.1e2
	  unclamped, none        3.36e-4 at max|ref| 7.3e2 | 4.88e-4 at 6.8e2"""
	g = fx
	with torch.inference_mode():
		ref = M.loop(R.schedule(6, cf), oracle, g["start"].cpu(), g["E"].cpu(), clip=clip_)
	got = run(diffuser(6, cf), models["f32"], g, clip_)
	scale = 1.0 if clip_ else max(1.0, float(ref.abs().max()))
	err = maxerr(got, ref)
	print(f"dpm++2m f32 vs f64 restatement T={ref.shape[-1]} clip={clip_} cf={cf}: max|err| {err:.3e}, max|ref| {float(ref.abs().max()):.3e}")
	assert torch.isfinite(got).all() and err <= F32_TOL * scale, (err, scale)


# ------------------------------------------------------------------------------------------------ identities between the entries
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_whole_loop_equals_the_step_entry_and_the_generator(models, fx, dtype):
	model, g = models[dtype], fx
	T = g["start"].shape[-1]
	lib = model.lib
	for cf, clip_ in ((True, True), (False, False)):
		d = diffuser(5, cf)
		whole = run(d, model, g, clip_)
		# ttk_diff_step_ms in a loop, the history in a buffer of the caller's, poisoned: the first step must not read it
		x, hist = g["start"].clone(), torch.full_like(g["start"], float("nan"))
		_lib.check(lib.ttk_diff_begin(model._h, g["E"].data_ptr(), 1, T, _lib.stream_ptr()), "ttk_diff_begin")
		for i in reversed(range(5)):
			_lib.check(lib.ttk_diff_step_ms(model._h, x.data_ptr(), hist.data_ptr(), d.step_coefs(i, "ddim"), d.step_coefs_ms(i, clip_), None, _lib.stream_ptr()), "ttk_diff_step_ms")
		assert torch.isfinite(whole).all() and torch.equal(whole, x), (dtype, T, cf, maxerr(whole, x))
		steps = list(d.dpmpp_sample_loop_progressive(model, (1, 100, T), noise=g["start"], clip_denoised=clip_, model_kwargs=kw(g)))
		assert len(steps) == 5 and torch.equal(steps[-1]["sample"], whole)
		assert all(set(s) == {"sample", "pred_xstart"} and torch.isfinite(s["pred_xstart"]).all() for s in steps)
		assert torch.equal(steps[-1]["sample"], steps[-1]["pred_xstart"])            # index 0 is (0, 1, 0): x = x0
		if clip_:
			assert all(float(s["pred_xstart"].abs().max()) <= 1.0 for s in steps)


def test_ragged_batch_equals_the_single_loops(models, golden):
	"""T = 40, 136, 72 in slots of Tp = 192: each element bit for bit its own loop, in f32 and bf16"""
	gs = [golden(n) for n in FIXTURES]
	starts = [t(gs[0]["start"]).to(DEV), t(gs[1]["start"]).to(DEV), t(gs[1]["start"])[:, :, 30:102].contiguous().to(DEV)]
	Es = [t(gs[0]["E"]).to(DEV), t(gs[1]["E"]).to(DEV), t(gs[1]["E"])[:, :, 30:102].contiguous().to(DEV)]
	assert [s.shape[-1] for s in starts] == [40, 136, 72]
	d = diffuser(5, True)
	for dt in ("f32", "bf16"):
		for clip_ in (True, False):
			batch = d.sample_loop_lines(models[dt], starts, Es, sampler="dpm++2m", clip_denoised=clip_)
			for s, E, got in zip(starts, Es, batch):
				one = d.sample_loop(models[dt], tuple(s.shape), noise=s, sampler="dpm++2m", clip_denoised=clip_, model_kwargs={"precomputed_aligned_embeddings": E})
				assert got.shape == one.shape and torch.isfinite(one).all() and torch.equal(got, one), (dt, clip_, s.shape[-1], maxerr(got, one))
	# the DDIM batch is what it was: element by element its own DDIM loop
	batch = d.sample_loop_lines(models["f32"], starts, Es)
	for s, E, got in zip(starts, Es, batch):
		assert torch.equal(got, d.sample_loop(models["f32"], tuple(s.shape), noise=s, model_kwargs={"precomputed_aligned_embeddings": E}, consume_rng=False))


def test_history_buffer_carries_nothing_over_and_ddim_keeps_its_bits(models, golden):
	"""small call, large call (the history buffer grows), small call again, with a DDIM call in between: equal calls give equal bits, and DDIM's are those of a fresh handle"""
	from tortoise_tts_amd.diffusion import DiffusionTTS
	small, large = [{k: (t(v).to(DEV) if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim >= 3 else v) for k, v in golden(n).items()} for n in FIXTURES]
	model, d = models["f32"], diffuser(5, True)
	fresh = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(small["seed"])), W.DIFF_SMALL, dtype="f32", device=DEV)
	ddim_fresh = d.sample_loop(fresh, (1, 100, 40), noise=small["start"], model_kwargs=kw(small), consume_rng=False)
	a = run(d, model, small)
	b = run(d, model, small)
	big = run(d, model, large)
	ddim = d.sample_loop(model, (1, 100, 40), noise=small["start"], model_kwargs=kw(small), consume_rng=False)
	c = run(d, model, small)
	assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(big, run(d, model, large))
	assert torch.equal(ddim, ddim_fresh) and not torch.equal(ddim, a)


# ------------------------------------------------------------------------------------------------ first order is DDIM; second order is not
@pytest.mark.parametrize("cf", [True, False])
def test_forced_first_order_is_the_ddim_entry(models, fx, cf):
	"""every c_d1 = 0: the DDIM entry's result within F32_TOL (x max(1, max|ref|) unclamped; DDIM's unclamped form is ttk_diff_sample_ext's).  The true second-order result
	differs from DDIM by more than 100 x F32_TOL, unclamped: the history term is what is tested.  (100 x the tolerance figure, 0.3, as test_gpu_sampler_ext.py asks of the
	eta cases -- not 100 x the scaled bound, ~2e2: the float64 restatements of the two solvers over the oracle themselves differ by 24 - 31 at max|x| 7e2 - 8e2 here,
	so no correct solver could meet that.)"""
	g, model, d = fx, models["f32"], diffuser(6, cf)
	T = g["start"].shape[-1]
	for clip_ in (True, False):
		ddim = d.sample_loop(model, (1, 100, T), noise=g["start"], sampler="ddim", clip_denoised=clip_, model_kwargs=kw(g), consume_rng=False)
		first = d._sample_ms(model, g["start"].clone(), g["E"], clip_, ms_array(d, clip_, first_order=True))
		bound = F32_TOL * (1.0 if clip_ else max(1.0, float(ddim.abs().max())))
		err = maxerr(first, ddim)
		print(f"forced first order vs ddim T={T} cf={cf} clip={clip_}: max|err| {err:.3e}, bound {bound:.3e}")
		assert err <= bound, (clip_, err, bound)
		if not clip_:
			second = run(d, model, g, False)
			print(f"  second order vs ddim: max|diff| {maxerr(second, ddim):.3e}")
			assert maxerr(second, ddim) > 100 * F32_TOL


# ------------------------------------------------------------------------------------------------ convergence on the device
def test_convergence_is_second_order_on_the_device(models, fx):
	"""f32, unclamped, no guidance; truth: the existing sample_loop(sampler="ddim", clip_denoised=False) at 500 steps.  The assertions of tests/test_dpmpp_ref.py:
	err_2m(16) <= 0.5 err_ddim(16), err_2m(32) <= 0.5 err_ddim(32), err_2m(16) / err_2m(32) >= 2.5 (relative L2).
	Measured on an MI355X: T = 40 ddim 6.970e-2 / 3.513e-2, 2m 2.766e-2 / 8.891e-3 (0.40, 0.25, 3.11); T = 136 ddim 6.859e-2 / 3.433e-2, 2m 2.771e-2 / 8.656e-3 (0.40, 0.25, 3.20)."""
	g, model = fx, models["f32"]
	T = g["start"].shape[-1]
	args = dict(noise=g["start"], clip_denoised=False, model_kwargs=kw(g))
	truth = diffuser(500, False).sample_loop(model, (1, 100, T), sampler="ddim", consume_rng=False, **args)
	err = {}
	for n in (16, 32):
		d = diffuser(n, False)
		err["ddim", n] = relerr(d.sample_loop(model, (1, 100, T), sampler="ddim", consume_rng=False, **args), truth)
		err["2m", n] = relerr(d.sample_loop(model, (1, 100, T), sampler="dpm++2m", **args), truth)
	print(f"T={T}: " + ", ".join(f"{k[0]}({k[1]}) {v:.3e}" for k, v in err.items()))
	assert err["2m", 16] <= 0.5 * err["ddim", 16], err
	assert err["2m", 32] <= 0.5 * err["ddim", 32], err
	assert err["2m", 16] / err["2m", 32] >= 2.5, err


# ------------------------------------------------------------------------------------------------ bf16
def test_bf16_deviation_beside_the_existing_bf16_loop(models, fx):
	"""Clamped, n = 6, guidance on: relative L2 of bf16 against our f32 for the new loop, beside the same figure for the existing DDIM loop on the same run; bound 2 x
	the parent's figure (the extrapolation weights 1 + 1/(2r) and 1/(2r) sum to about 2 on a near-uniform grid, so an x0 error can enter a step twice as large).
	Measured on an MI355X, parent -> ours (ratio): T = 40 1.515e-2 -> 1.740e-2 (1.15), T = 136 1.652e-2 -> 1.606e-2 (0.97)."""
	g, d = fx, diffuser(6, True)
	T = g["start"].shape[-1]
	parent = [d.sample_loop(models[dt], (1, 100, T), noise=g["start"], sampler="ddim", model_kwargs=kw(g), consume_rng=False) for dt in ("f32", "bf16")]
	ours = [run(d, models[dt], g) for dt in ("f32", "bf16")]
	par, our = relerr(parent[1], parent[0]), relerr(ours[1], ours[0])
	print(f"bf16 T={T} dpm++2m: parent {par:.4e} ours {our:.4e} ratio {our / par:.3f}")
	assert our <= 2 * par, (T, par, our, our / par)


# ------------------------------------------------------------------------------------------------ generator
def test_generator_stands_behind_the_start_noise_draw(models, fx):
	g, d = fx, diffuser(5, True)
	T = g["start"].shape[-1]
	torch.manual_seed(11)
	a = d.sample_loop(models["f32"], (1, 100, T), sampler="dpm++2m", model_kwargs=kw(g))
	after_a = torch.rand(4, device=DEV)
	torch.manual_seed(11)
	x = torch.randn(1, 100, T, device=DEV)
	after_b = torch.rand(4, device=DEV)
	assert torch.equal(after_a, after_b)
	assert torch.equal(a, run(d, models["f32"], dict(g, start=x)))
	# with the start noise given, nothing is drawn
	torch.manual_seed(11)
	run(d, models["f32"], g)
	torch.randn(1, 100, T, device=DEV)
	assert torch.equal(torch.rand(4, device=DEV), after_b)


# ------------------------------------------------------------------------------------------------ TTS level
def test_tts_inference_dpmpp(tts):
	enc = tts.encode_audio(clip(), 22050)
	args = dict(max_ar_steps=10, max_diffusion_steps=4, candidates=2, seed=1234)
	lines = ["Hello there.", "The end!"]
	one, sr = tts.inference(lines[0], enc, diffusion_sampler="dpm++2m", **args)
	assert sr == 24000 and torch.isfinite(one).all() and torch.equal(one, tts.inference(lines[0], enc, diffusion_sampler="dpm++2m", **args)[0])
	assert not torch.equal(one, tts.inference(lines[0], enc, **args)[0])
	# one line is TTSHotPath.inference plus the vocoder
	ar_latent, diff_latent = enc["latent"]
	from tortoise_tts_amd.tts import set_seed
	set_seed(1234)
	tokens = tts.encode_text(lines[0]).to(tts.device)[None]
	mels, _ = tts.hot.inference(tokens, ar_latent, diff_latent, diffusion_sampler="dpm++2m", max_ar_steps=10, max_diffusion_steps=4, candidates=2)
	assert torch.equal(one, tts.hot.vocoder.inference(mels))
	# two lines (TTSHotPath.inference_lines, the ragged multistep batch) are the two single-line calls
	both, _ = tts.inference("\n".join(lines), enc, diffusion_sampler="dpm++2m", **args)
	two, _ = tts.inference(lines[1], enc, diffusion_sampler="dpm++2m", **args)
	assert torch.equal(both, torch.concat([one, two], dim=-1))
	with pytest.raises(ValueError, match="diffusion_eta must be 0"):
		tts.inference(lines[0], enc, diffusion_sampler="dpm++2m", diffusion_eta=0.5, **args)


def test_decode_codes_dpmpp(tts):
	enc = tts.encode_audio(clip(), 22050)
	gen = torch.Generator().manual_seed(4)
	rows = [torch.randint(0, W.DIFF_CODE_TOKENS, (1, M_), generator=gen).to(DEV) for M_ in (12, 9)]
	args = dict(max_diffusion_steps=4, seed=77, diffusion_sampler="dpm++2m")
	a = tts.decode_codes(rows[0], enc, **args)[0]
	assert torch.isfinite(a).all() and torch.equal(a, tts.decode_codes(rows[0], enc, **args)[0])
	assert not torch.equal(a, tts.decode_codes(rows[0], enc, max_diffusion_steps=4, seed=77)[0])
	both = tts.decode_codes(rows, enc, **args)[0]                  # a list of rows: one ragged batch, each row what its own call gives
	assert torch.equal(both, torch.concat([a, tts.decode_codes(rows[1], enc, **args)[0]], dim=-1))
	with pytest.raises(ValueError, match="diffusion_eta must be 0"):
		tts.decode_codes(rows[0], enc, diffusion_eta=1.0, **args)
