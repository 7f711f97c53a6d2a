"""The rest of the reference sampler's argument space on the GPU (include/ttk.h: ttk_step_ext, ttk_diff_sample_ext, ttk_diff_step_ext, ttk_diffusion_step_ext_rows;
tortoise_tts_amd/diffusion.py: eta, clip_denoised, ddim_reverse_sample, the progressive forms): the update kernel alone bit for bit against a numpy f32 restatement, the
existing loops bit for bit through the new entry, every case of tests/golden/diff_sampler_small*.npz (made by the reference itself, tools/make_golden_sampler.py) in f32,
the generator position, the single-step forms, the round trip, bf16 beside the existing bf16 loop, and `TTS.inference(diffusion_eta=)`.  DIFF_SMALL, T <= 136, <= 6 steps.
GPU only; calls go through the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import sampler_ref as R
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = 3e-3       # what tests/test_gpu_configs.py holds the f32 DDIM loop to against reference fixtures at this model size (6 steps, DIFF_SMALL)
FIXTURES = ["diff_sampler_small", "diff_sampler_small_t136"]


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def relerr(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def models(golden):
	from tortoise_tts_amd.diffusion import DiffusionTTS
	sd = W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), int(golden(FIXTURES[0])["seed"]))
	return {dt: DiffusionTTS(sd, W.DIFF_SMALL, dtype=dt, device=DEV) for dt in ("f32", "bf16")}


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request, golden):
	g = golden(request.param)
	return {k: (t(v).to(DEV) if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim >= 3 else v) for k, v in g.items()}


def diffuser(steps, cf):
	from tortoise_tts_amd.diffusion import get_diffuser
	return get_diffuser(steps=steps, cond_free=cf)


def kw(g):
	return {"precomputed_aligned_embeddings": g["E"]}


# the fixture's cases: key -> (steps, cond_free, sampler, eta, clip, start)
CASES = {
	"ddim_eta05": (5, True, "ddim", 0.5, True, "start"),
	"ddim_eta1": (6, False, "ddim", 1.0, True, "start"),
	"ddim_noclip": (5, True, "ddim", 0.0, False, "scaled"),
	"p_noclip": (5, True, "p", 0.0, False, "scaled"),
}


def run_case(model, g, key):
	"""a fixture case through the public sample_loop where it can take the fixture's draws (step_noise=), else through the loop entry it would call"""
	steps, cf, sampler, eta, clip, start = CASES[key]
	d = diffuser(steps, cf)
	x = g["start"] * float(g["noclip_scale"]) if start == "scaled" else g["start"]
	T = x.shape[-1]
	if sampler == "ddim":
		return d.sample_loop(model, (1, 100, T), noise=x, sampler="ddim", eta=eta, clip_denoised=clip, model_kwargs=kw(g), step_noise=g["step_noise"][:steps], consume_rng=False)
	return d._sample_ext(model, x.clone(), g["E"], 1, 0.0, clip, g["step_noise"][:steps])


# ------------------------------------------------------------------------------------------------ the kernel alone
def exp_candidates(half):
	"""the f32 values within 2 ulp of exp(half): expf is OCML's range reduction around the exp2 instruction, 1 ulp each"""
	e = np.exp(half.astype(np.float64)).astype(np.float32)
	up1 = np.nextafter(e, np.float32(np.inf)); dn1 = np.nextafter(e, np.float32(-np.inf))
	return [e, up1, dn1, np.nextafter(up1, np.float32(np.inf)), np.nextafter(dn1, np.float32(-np.inf))]


@pytest.mark.parametrize("cfk", [1.25, -1.0])
@pytest.mark.parametrize("clip", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_update_kernel_bit_for_bit(mode, clip, cfk):
	"""nb = 2, C = 100, T = 70: 14000 elements = 54 blocks of 256 and a tail of 176.  Every output -- x, pred_xstart, the channels-last copy in f32 / f16 / bf16 -- equals the
	numpy f32 restatement of the kernel's operation order (tests/sampler_ref.py: step_ext_numpy) bit for bit, at a step that adds noise and at index 0.  One exception, by
	necessity: the ancestral step's noise factor expf(0.5 log_var) ends in the hardware's exp2 instruction, whose last bit no host can restate; there x must equal
	mean + e * noise bit for bit for one of the f32 values e within 2 ulp of the exponential, with mean and pred_xstart exact (and the loop test below holds the whole of
	it to the existing kernel's bits)."""
	lib = _lib.load()
	nb, C, T, ldo, rep = 2, 100, 70, 128, 2
	gen = torch.Generator().manual_seed(100 * mode + 10 * clip + int(cfk > 0))
	out_c, out_u = torch.randn(nb, 2 * C, T, generator=gen), torch.randn(nb, 2 * C, T, generator=gen)
	x0, noise = 1.5 * torch.randn(nb, C, T, generator=gen), torch.randn(nb, C, T, generator=gen)
	d = diffuser(5, True)
	for i in (3, 0):
		st, ext = d.step_coefs(i, "p" if mode == 1 else "ddim"), d.step_coefs_ext(i, mode, 0.5, bool(clip))
		st.cfk = cfk
		ref = R.step_ext_numpy(out_c.numpy(), out_u.numpy(), x0.numpy(), noise.numpy(), st, ext)
		if clip == 0:
			assert (np.abs(ref[1]) > 1).mean() > 0.1          # the clamp would have bitten
		for dt, tdt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
			x = x0.to(DEV).clone()
			px = torch.full_like(x, 7.0)
			xcl = torch.full((rep * nb * T, ldo), 9.0, device=DEV, dtype=tdt)
			dc, du, dn = out_c.to(DEV), out_u.to(DEV), noise.to(DEV)
			_lib.check(lib.ttk_diffusion_step_ext_rows(dc.data_ptr(), du.data_ptr() if cfk >= 0 else None, x.data_ptr(), dn.data_ptr(), px.data_ptr(), nb, C, T, ctypes.byref(st),
													   ctypes.byref(ext), xcl.data_ptr(), ldo, rep, _lib.DTYPES[dt], _lib.stream_ptr()), "ttk_diffusion_step_ext_rows")
			torch.cuda.synchronize()
			got, gpx = x.cpu().numpy(), px.cpu().numpy()
			assert np.array_equal(gpx.view(np.uint32), ref[1].view(np.uint32)), (mode, clip, cfk, i, dt, "pred_xstart")
			if len(ref) == 2:
				assert np.array_equal(got.view(np.uint32), ref[0].view(np.uint32)), (mode, clip, cfk, i, dt, np.abs(got - ref[0]).max())
			else:
				mean, _, half = ref
				hit = np.zeros(got.shape, bool)
				for e in exp_candidates(half):
					hit |= (mean + e * noise.numpy()).view(np.uint32) == got.view(np.uint32)
				assert hit.all(), (mode, clip, cfk, i, dt, int((~hit).sum()))
			want = x.permute(0, 2, 1).reshape(1, nb * T, C).expand(rep, -1, -1).reshape(rep * nb * T, C).to(tdt)      # row (q nb + b) T + t, column c
			assert torch.equal(xcl[:, :C], want) and bool((xcl[:, C:] == 9.0).all()), (mode, clip, cfk, i, dt, "channels-last copy")
		# without the optional outputs, and without noise where the step reads none
		x = x0.to(DEV).clone()
		reads = st.nonzero and (mode == 1 or (mode == 0 and ext.sigma != 0))
		_lib.check(lib.ttk_diffusion_step_ext_rows(dc.data_ptr(), du.data_ptr() if cfk >= 0 else None, x.data_ptr(), dn.data_ptr() if reads else None, None, nb, C, T,
												   ctypes.byref(st), ctypes.byref(ext), None, 0, 0, 0, _lib.stream_ptr()), "ttk_diffusion_step_ext_rows")
		assert np.array_equal(x.cpu().numpy().view(np.uint32), got.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the existing loops do not move
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_new_loop_entry_equals_the_existing_entries_bit_for_bit(models, fx, dtype):
	model, g = models[dtype], fx
	T = g["start"].shape[-1]
	for cf in (True, False):
		d = diffuser(5, cf)
		ddim = d.sample_loop(model, (1, 100, T), noise=g["start"], sampler="ddim", model_kwargs=kw(g), consume_rng=False)
		ext = d._sample_ext(model, g["start"].clone(), g["E"], 0, 0.0, True, None)
		assert torch.isfinite(ddim).all() and torch.equal(ddim, ext), (dtype, T, cf, "ddim", maxerr(ddim, ext))
		torch.manual_seed(5)
		p = d.sample_loop(model, (1, 100, T), noise=g["start"], sampler="p", model_kwargs=kw(g))
		torch.manual_seed(5)
		nz = torch.stack([torch.randn_like(g["start"]) for _ in range(5)])
		ext = d._sample_ext(model, g["start"].clone(), g["E"], 1, 0.0, True, nz)
		assert torch.isfinite(p).all() and torch.equal(p, ext), (dtype, T, cf, "p", maxerr(p, ext))


# ------------------------------------------------------------------------------------------------ f32 against the reference's vectors
@pytest.mark.parametrize("key", list(CASES))
def test_f32_loops_against_the_reference(models, fx, key):
	g = fx
	ref = g[key]
	got = run_case(models["f32"], g, key)
	scale = float(ref.abs().max()) if key.endswith("_noclip") else 1.0       # unclamped: x is not bounded by 1, the same number relative to max|ref|
	err = maxerr(got, ref)
	print(f"{key} T={ref.shape[-1]}: max|err| {err:.3e}, max|ref| {float(ref.abs().max()):.3e}")
	assert err < F32_TOL * scale, (key, err, scale)
	if key.startswith("ddim_eta"):
		assert maxerr(got, g[key + "_eta0"]) > 100 * F32_TOL      # the noise term is what is being tested


@pytest.mark.parametrize("cf", [False, True])
def test_f32_reverse_ode_against_the_references_step_in_a_loop(models, fx, cf):
	g = fx
	got = diffuser(5, cf).ddim_reverse_sample_loop(models["f32"], g["mel"], model_kwargs=kw(g))
	err = maxerr(got, g[f"reverse_cf{int(cf)}"])
	print(f"reverse cf={cf} T={got.shape[-1]}: max|err| {err:.3e}")
	assert err < F32_TOL and got.data_ptr() != g["mel"].data_ptr()


def test_round_trip_error_is_the_references(models, fx):
	"""mel -> reverse ODE -> DDIM, both unclamped, cond_free False: no worse than twice the reference's own reconstruction error (two f32 runs of one ODE; the factor
	covers the network's summation order, nothing else).  With synthetic weights the network is no denoiser and that error is large; it is the same error."""
	g, d = fx, diffuser(5, False)
	T = g["mel"].shape[-1]
	xT = d.ddim_reverse_sample_loop(models["f32"], g["mel"], clip_denoised=False, model_kwargs=kw(g))
	back = d.sample_loop(models["f32"], (1, 100, T), noise=xT, sampler="ddim", clip_denoised=False, model_kwargs=kw(g), consume_rng=False)
	err = maxerr(back, g["mel"])
	print(f"roundtrip T={T}: ours {err:.4f}, reference {float(g['roundtrip_err']):.4f}")
	assert err <= 2 * float(g["roundtrip_err"])


# ------------------------------------------------------------------------------------------------ generator, single steps
def test_generator_stands_where_the_references_loop_leaves_it(models, fx):
	g, d = fx, diffuser(5, True)
	T = g["start"].shape[-1]
	torch.manual_seed(11)
	a = d.sample_loop(models["f32"], (1, 100, T), noise=g["start"], sampler="ddim", eta=0.5, model_kwargs=kw(g))
	after_a = torch.rand(4, device=DEV)
	torch.manual_seed(11)
	nz = torch.stack([torch.randn_like(g["start"]) for _ in range(5)])      # the restatement: one randn_like per step, in loop order (diffusion.py:685)
	after_b = torch.rand(4, device=DEV)
	assert torch.equal(after_a, after_b)
	assert torch.equal(a, d._sample_ext(models["f32"], g["start"].clone(), g["E"], 0, 0.5, True, nz))
	# eta = 0 with clip_denoised=False: the draws are made and ignored, as before
	torch.manual_seed(11)
	d.sample_loop(models["f32"], (1, 100, T), noise=g["start"], sampler="ddim", clip_denoised=False, model_kwargs=kw(g))
	assert torch.equal(torch.rand(4, device=DEV), after_b)
	# no start noise given: drawn first, then the steps'
	torch.manual_seed(11)
	b = d.sample_loop(models["f32"], (1, 100, T), sampler="ddim", eta=0.5, model_kwargs=kw(g))
	torch.manual_seed(11)
	x = torch.randn(1, 100, T, device=DEV)
	nz = torch.stack([torch.randn_like(x) for _ in range(5)])
	assert torch.equal(b, d._sample_ext(models["f32"], x, g["E"], 0, 0.5, True, nz))


def test_progressive_and_single_steps_equal_the_loop_entry(models, golden):
	g = {k: (t(v).to(DEV) if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim >= 3 else v) for k, v in golden(FIXTURES[0]).items()}
	model, d = models["f32"], diffuser(4, True)
	T = g["start"].shape[-1]
	# single steps on the fixture's draws: every step's dict against the reference's, the last sample the loop entry's bits
	x, outs = g["start"], []
	for j, i in enumerate(reversed(range(4))):
		out = d._single_step(model, x, torch.tensor([i]), 0, 0.5, True, kw(g), noise=g["step_noise"][j])
		outs.append(out)
		x = out["sample"]
	for j, out in enumerate(outs):
		assert maxerr(out["sample"], g["prog_sample"][j]) < F32_TOL and maxerr(out["pred_xstart"], g["prog_pred_xstart"][j]) < F32_TOL, j
	whole = d._sample_ext(model, g["start"].clone(), g["E"], 0, 0.5, True, g["step_noise"][:4])
	assert torch.equal(outs[-1]["sample"], whole)
	# the generator forms draw where the loop does
	for sampler, prog, extra in (("ddim", d.ddim_sample_loop_progressive, dict(eta=0.5)), ("p", d.p_sample_loop_progressive, {})):
		torch.manual_seed(3)
		whole = d.sample_loop(model, (1, 100, T), sampler=sampler, clip_denoised=False, model_kwargs=kw(g), **extra)
		after = torch.rand(4, device=DEV)
		torch.manual_seed(3)
		steps = list(prog(model, (1, 100, T), clip_denoised=False, model_kwargs=kw(g), **extra))
		assert len(steps) == 4 and torch.equal(steps[-1]["sample"], whole) and torch.equal(torch.rand(4, device=DEV), after), sampler
		assert all(s["pred_xstart"].shape == (1, 100, T) and torch.isfinite(s["pred_xstart"]).all() for s in steps)
	# the reverse step in a Python loop is the reverse loop
	x = g["mel"]
	for i in range(4):
		x = d.ddim_reverse_sample(model, x, torch.tensor([i]), model_kwargs=kw(g))["sample"]
	assert torch.equal(x, d.ddim_reverse_sample_loop(model, g["mel"], model_kwargs=kw(g)))


# ------------------------------------------------------------------------------------------------ bf16
def test_bf16_deviation_beside_the_existing_bf16_loop(models, fx):
	"""Each case in bf16 against our f32 result (relative L2), beside the same figure for the EXISTING DDIM loop (eta 0, clamped) at the same T, step count and guidance,
	on the same run; bound: 1.5 x that parent figure.  Measured on an MI355X, parent -> case (ratio), T = 40 | T = 136:
	  ddim_eta05    2.03e-2 -> 1.32e-2 (0.65) | 1.81e-2 -> 1.13e-2 (0.62)
	  ddim_eta1     1.93e-2 -> 4.97e-3 (0.26) | 1.61e-2 -> 5.07e-3 (0.31)
	  ddim_noclip   2.03e-2 -> 6.81e-4 (0.03) | 1.81e-2 -> 6.93e-4 (0.04)
	  p_noclip      2.03e-2 -> 7.58e-4 (0.04) | 1.81e-2 -> 7.71e-4 (0.04)
	  reverse_cf0   2.10e-2 -> 4.54e-3 (0.22) | 1.56e-2 -> 4.31e-3 (0.28)
	  reverse_cf1   2.03e-2 -> 5.87e-3 (0.29) | 1.81e-2 -> 5.62e-3 (0.31)
	No eta case exceeds the bound."""
	g = fx
	T = g["start"].shape[-1]
	rows = []
	for key, (steps, cf, sampler, eta, clip, start) in CASES.items():
		d = diffuser(steps, cf)
		parent = [d.sample_loop(models[dt], (1, 100, T), noise=g["start"], sampler="ddim", model_kwargs=kw(g), consume_rng=False) for dt in ("f32", "bf16")]
		ours = [run_case(models[dt], g, key) for dt in ("f32", "bf16")]
		rows.append((key, relerr(parent[1], parent[0]), relerr(ours[1], ours[0])))
	for cf in (False, True):
		d = diffuser(5, cf)
		parent = [d.sample_loop(models[dt], (1, 100, T), noise=g["start"], sampler="ddim", model_kwargs=kw(g), consume_rng=False) for dt in ("f32", "bf16")]
		ours = [d.ddim_reverse_sample_loop(models[dt], g["mel"], model_kwargs=kw(g)) for dt in ("f32", "bf16")]
		rows.append((f"reverse_cf{int(cf)}", relerr(parent[1], parent[0]), relerr(ours[1], ours[0])))
	for key, par, our in rows:
		print(f"bf16 T={T} {key}: parent {par:.4e} ours {our:.4e} ratio {our / par:.3f}")
	for key, par, our in rows:
		assert our <= 1.5 * par, (key, T, par, our, our / par)


# ------------------------------------------------------------------------------------------------ TTS level
@pytest.fixture(scope="module")
def tts(golden):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t_): i for i, t_ in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	sd = dict(ar=W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), df=W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32),
			  voc=W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33), arc=W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35),
			  dfc=W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36))
	sd["df"].update(W.synth_state_dict(W.diffusion_code_shapes(W.DIFF_SMALL), 32))      # token conditioning as well: decode_codes
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	return TTS(UnifiedVoice(sd["ar"], W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=128), DiffusionTTS(sd["df"], W.DIFF_SMALL, dtype="f32", device=DEV), tok,
			   vocoder=BigVGAN(sd["voc"], W.VOC_SMALL, dtype="f32", device=DEV),
			   conditioning_encoder=ConditioningEncoder(sd["arc"], W.AR_SMALL, dtype="f32", device=DEV), contextual_embedder=ContextualEmbedder(sd["dfc"], W.DIFF_SMALL, dtype="f32", device=DEV),
			   tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV))


def clip():
	n = torch.arange(30000) / 22050
	return (0.3 * torch.sin(2 * np.pi * 180 * n) + 0.1 * torch.sin(2 * np.pi * 1250 * n))[None].to(DEV)


def test_decode_codes_diffusion_eta(tts):
	enc = tts.encode_audio(clip(), 22050)
	gen = torch.Generator().manual_seed(4)
	rows = [torch.randint(0, W.DIFF_CODE_TOKENS, (1, M), generator=gen).to(DEV) for M in (12, 9)]
	args = dict(max_diffusion_steps=3, seed=77)
	plain = tts.decode_codes(rows[0], enc, **args)[0]
	assert torch.equal(plain, tts.decode_codes(rows[0], enc, diffusion_eta=0.0, **args)[0])
	one = tts.decode_codes(rows[0], enc, diffusion_eta=1.0, **args)[0]
	assert one.shape == plain.shape and torch.isfinite(one).all() and not torch.equal(one, plain)
	assert torch.equal(one, tts.decode_codes(rows[0], enc, diffusion_eta=1.0, **args)[0])
	both = tts.decode_codes(rows, enc, diffusion_eta=1.0, **args)[0]                  # a list of rows: each what its own call gives
	assert torch.equal(both, torch.concat([one, tts.decode_codes(rows[1], enc, diffusion_eta=1.0, **args)[0]], dim=-1))


@pytest.mark.parametrize("text", ["Hello there.", "Hello there.\nThe end!"])
def test_tts_inference_diffusion_eta(tts, text):
	"""one line (TTSHotPath.inference) and two (inference_lines: the per-step draws are made by the main thread, each line diffuses in its own loop)"""
	enc = tts.encode_audio(clip(), 22050)
	args = dict(max_ar_steps=10, max_diffusion_steps=3, candidates=2, seed=1234)
	plain, sr = tts.inference(text, enc, **args)
	zero, _ = tts.inference(text, enc, diffusion_eta=0.0, **args)
	one, _ = tts.inference(text, enc, diffusion_eta=1.0, **args)
	again, _ = tts.inference(text, enc, diffusion_eta=1.0, **args)
	assert sr == 24000 and torch.equal(plain, zero)
	assert one.shape == plain.shape and torch.isfinite(one).all() and not torch.equal(one, plain)
	assert torch.equal(one, again)
	# a text's lines are what each line alone gives, with eta as without
	if "\n" in text:
		alone = [tts.inference(line, enc, diffusion_eta=1.0, **args)[0] for line in text.split("\n")]
		assert torch.equal(one, torch.concat(alone, dim=-1))
	# the ancestral sampler ignores eta
	p0, _ = tts.inference(text, enc, diffusion_sampler="p", **args)
	p1, _ = tts.inference(text, enc, diffusion_sampler="p", diffusion_eta=1.0, **args)
	assert torch.equal(p0, p1)
