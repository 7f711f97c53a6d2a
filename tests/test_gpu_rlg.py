"""Random voices on the GPU: `ttk_linear_rows` (csrc/rlg.hip) on its own against float64, its row independence and argument checks; the
RandomLatentConverter chain against the reference's own class (tests/golden/rlg_*.npz); the generator contract of `forward`; and
`TTS.inference(text, None)` against its own parts.

Kernel bound: |out - out64| <= (K + 8) * 2^-24 * gain * (sum_k |x W| + |bias|) -- the standard bound of an f32 dot product of K terms in any
summation order (gamma_K with unit roundoff 2^-24), the 8 covering the bias add, the activation and the gain; derived, not tuned.
Chain bound: max|y_gpu - y64| <= 4 * max|y - y64|, four times the reference's own f32 deviation from its float64 run -- the margin the
DiscreteVAE fixtures use for "another summation order".  The measured ratios are in DESIGN.md section 15."""
import numpy as np
import pytest
import torch

import rlg_oracle as RO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 4, 1), (1, 64, 64), (3, 260, 65), (16, 1024, 1024), (5, 2048, 2048), (16, 2052, 7))      # rows, K, N
SLOPE, GAIN = float(np.float32(0.2)), float(np.float32(2 ** 0.5))      # as the C ABI receives them
NAN = float("nan")
_inputs, _chains = {}, {}


@pytest.fixture(scope="module")
def lib():
	return _lib.load()


def inputs(shape):
	"""seeded operands of one shape, on the host and on the device, made once: x sits in a [rows, K + 4] buffer whose padding is NaN"""
	if shape not in _inputs:
		rows, K, N = shape
		g = torch.Generator().manual_seed(1000003 * rows + 1009 * K + N)
		x, w, b = torch.randn((rows, K), generator=g), torch.randn((N, K), generator=g) / K ** 0.5, torch.randn((N,), generator=g)
		xb = torch.full((rows, K + 4), NAN)
		xb[:, :K] = x
		pre = x.double() @ w.double().T
		mag = x.double().abs() @ w.double().abs().T
		_inputs[shape] = dict(x=x, w=w, b=b, pre=pre, mag=mag, dx=xb.to(DEV), dw=w.to(DEV), db=b.to(DEV))
	return _inputs[shape]


def call(lib, dx, rows, K, N, dw, db, act, out, gain=GAIN):
	return lib.ttk_linear_rows(dx.data_ptr(), dx.stride(0), dw.data_ptr(), _lib.ptr(db), rows, K, N, act, SLOPE, gain, out.data_ptr(), out.stride(0), _lib.stream_ptr())


def guarded(rows, N):
	"""[rows + 1, N + 3] of NaN: three guard columns behind every row and a guard row behind the last"""
	return torch.full((rows + 1, N + 3), NAN, device=DEV)


def guard_intact(out, rows, N):
	o = out.cpu()
	return bool(torch.isnan(o[:rows, N:]).all() and torch.isnan(o[rows:]).all())


@pytest.mark.parametrize("with_bias", (True, False))
@pytest.mark.parametrize("act", (0, 1))
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_float64(lib, shape, act, with_bias):
	rows, K, N = shape
	d = inputs(shape)
	out = guarded(rows, N)
	_lib.check(call(lib, d["dx"], rows, K, N, d["dw"], d["db"] if with_bias else None, act, out), "ttk_linear_rows")
	torch.cuda.synchronize()
	got = out[:rows, :N].cpu()
	pre = d["pre"] + (d["b"].double() if with_bias else 0.0)
	want = (torch.where(pre > 0, pre, pre * SLOPE) if act else pre) * GAIN
	bound = (K + 8) * 2.0 ** -24 * GAIN * (d["mag"] + (d["b"].double().abs() if with_bias else 0.0))
	err = (got.double() - want).abs()
	print(f"rows={rows} K={K} N={N} act={act} bias={with_bias}: worst |out - out64| / bound = {(err / bound).max().item():.4f} (max err {err.max().item():.3e})")
	assert torch.isfinite(got).all(), "a padding column of x (NaN) was read"
	assert (err <= bound).all(), (shape, act, with_bias, (err / bound).max().item())
	assert guard_intact(out, rows, N), "the kernel wrote past a row's N columns or past the last row"
	again = guarded(rows, N)
	_lib.check(call(lib, d["dx"], rows, K, N, d["dw"], d["db"] if with_bias else None, act, again), "ttk_linear_rows")
	assert torch.equal(again[:rows, :N].view(torch.int32), out[:rows, :N].view(torch.int32))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == 16])
def test_a_row_has_the_same_bits_alone_and_in_a_batch(lib, shape):
	rows, K, N = shape
	d = inputs(shape)
	batch = guarded(rows, N)
	_lib.check(call(lib, d["dx"], rows, K, N, d["dw"], d["db"], 1, batch), "ttk_linear_rows")
	alone = guarded(rows, N)
	for r in range(rows):
		_lib.check(call(lib, d["dx"][r:], 1, K, N, d["dw"], d["db"], 1, alone[r:]), "ttk_linear_rows")
	half = guarded(rows, N)
	_lib.check(call(lib, d["dx"], 7, K, N, d["dw"], d["db"], 1, half), "ttk_linear_rows")
	_lib.check(call(lib, d["dx"][7:], 9, K, N, d["dw"], d["db"], 1, half[7:]), "ttk_linear_rows")
	torch.cuda.synchronize()
	assert torch.isfinite(batch[:rows, :N]).all()
	assert torch.equal(alone[:rows, :N], batch[:rows, :N]) and torch.equal(half[:rows, :N], batch[:rows, :N])
	assert guard_intact(alone, rows, N) and guard_intact(half, rows, N)


@pytest.mark.parametrize("rows,K,named", [(17, 64, "17"), (1, 6, "6"), (1, 8196, "8196")])
def test_bad_arguments_are_refused_on_the_host(lib, rows, K, named):
	N = 8
	x = torch.zeros((rows, K + 2 if K % 4 else K), device=DEV)
	w = torch.zeros((N, K), device=DEV)
	out = guarded(rows, N)
	rc = lib.ttk_linear_rows(x.data_ptr(), x.stride(0), w.data_ptr(), None, rows, K, N, 0, SLOPE, 1.0, out.data_ptr(), out.stride(0), _lib.stream_ptr())
	torch.cuda.synchronize()
	assert rc == -1 and named in lib.ttk_last_error().decode(), (rc, lib.ttk_last_error())
	assert torch.isnan(out).all()


def chain(golden, name, tag):
	"""(fixture case, converter) built once per case"""
	from tortoise_tts_amd.random_latent import RandomLatentConverter
	if (name, tag) not in _chains:
		g = golden(name)
		channels, B = (int(v) for v in tag.split("x"))
		_chains[(name, tag)] = (RO.case(g, tag), RandomLatentConverter(W.rlg_state_dict(channels, int(g[f"seed_{tag}"])), device=DEV))
	return _chains[(name, tag)]


@pytest.mark.parametrize("name,tag", [(n, tag) for n, tags in RO.CASES.items() for tag in tags])
def test_chain_against_the_reference(golden, name, tag):
	(channels, B, folded, noise, y, y64), rlg = chain(golden, name, tag)
	assert rlg.channels == channels
	got = rlg.forward(torch.zeros(B, 1), noise.to(DEV))
	assert got.shape == (B, channels) and got.dtype == torch.float32 and got.device == torch.device(DEV)
	own = (y.double() - y64).abs().max().item()
	err = (got.cpu().double() - y64).abs().max().item()
	print(f"{name} {tag}: max|y_gpu - y64| = {err:.3e}, the reference's own max|y - y64| = {own:.3e}, ratio {err / own:.3f}")
	assert err <= 4 * own
	assert rlg(torch.zeros(B, 1), noise.to(DEV)).equal(got)      # __call__, and the same bits on every run


def test_more_rows_than_max_rows_run_in_chunks_and_f32_is_the_only_mode(golden):
	from tortoise_tts_amd.random_latent import RandomLatentConverter
	(channels, B, folded, noise, y, y64), rlg = chain(golden, "rlg_small", "64x5")
	sd = W.rlg_state_dict(channels, int(golden("rlg_small")["seed_64x5"]))
	two = RandomLatentConverter(sd, channels, device=DEV, max_rows=2)
	assert torch.equal(two(torch.zeros(B, 1), noise.to(DEV)), rlg(torch.zeros(B, 1), noise.to(DEV)))
	big = torch.randn(37, channels, generator=torch.Generator().manual_seed(3)).to(DEV)
	whole = rlg(big, big)
	assert whole.shape == (37, channels) and torch.equal(whole[32:], rlg(big[32:], big[32:])) and torch.equal(whole[:5], two(big[:5], big[:5]))
	for dtype in ("bf16", "f16", "fp8w"):
		with pytest.raises(_lib.TTKError, match="f32"):
			RandomLatentConverter(sd, channels, device=DEV, dtype=dtype)
	with pytest.raises(_lib.TTKError, match="noise"):
		rlg(torch.zeros(2, 1), noise.to(DEV))
	with pytest.raises(_lib.TTKError, match="layers.5.bias"):
		RandomLatentConverter({k: v for k, v in sd.items() if k != "layers.5.bias"}, device=DEV)


def test_a_saved_file_loads_into_the_same_converter(golden, tmp_path):
	import tortoise_tts_amd as ttk
	(channels, B, folded, noise, y, y64), rlg = chain(golden, "rlg_small", "64x5")
	path = tmp_path / "rlg_auto.pth"
	torch.save(W.rlg_state_dict(channels, int(golden("rlg_small")["seed_64x5"])), path)
	loaded = ttk.load_random_latent_generator(path, device=DEV)
	assert isinstance(loaded, ttk.RandomLatentConverter) and loaded.channels == channels
	assert torch.equal(loaded(torch.zeros(B, 1), noise.to(DEV)), rlg(torch.zeros(B, 1), noise.to(DEV)))


def test_forward_draws_what_torch_randn_draws(golden):
	_, rlg = chain(golden, "rlg_small", "132x1")
	ref = torch.zeros(3, 1)
	torch.manual_seed(77)
	v = rlg(ref)
	state = torch.cuda.get_rng_state(DEV)
	torch.manual_seed(77)
	noise = torch.randn(3, rlg.channels, device=DEV)
	v2 = rlg(ref, noise=noise)
	assert torch.equal(v, v2) and torch.equal(state, torch.cuda.get_rng_state(DEV))
	torch.manual_seed(78)
	assert not torch.equal(rlg(ref), v)


@pytest.fixture(scope="module")
def tts(golden):
	"""the small TTS of tests/test_gpu_tts.py (same parts, sizes and seeds) plus two converters at the widths of the small models' latents"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.random_latent import RandomLatentConverter
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	sd = dict(ar=W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), df=W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32),
			  voc=W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33), arc=W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35),
			  dfc=W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36))
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	parts = dict(vocoder=BigVGAN(sd["voc"], W.VOC_SMALL, dtype="f32", device=DEV),
				 conditioning_encoder=ConditioningEncoder(sd["arc"], W.AR_SMALL, dtype="f32", device=DEV), contextual_embedder=ContextualEmbedder(sd["dfc"], W.DIFF_SMALL, dtype="f32", device=DEV),
				 tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV))
	ar, df = UnifiedVoice(sd["ar"], W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=128), DiffusionTTS(sd["df"], W.DIFF_SMALL, dtype="f32", device=DEV)
	rlg = dict(rlg_auto=RandomLatentConverter(W.rlg_state_dict(W.AR_SMALL.model_dim, 37), device=DEV),
			   rlg_diffuser=RandomLatentConverter(W.rlg_state_dict(2 * W.DIFF_SMALL.model_channels, 38), device=DEV))
	return TTS(ar, df, tok, **parts, **rlg), TTS(ar, df, tok, **parts)


def test_text_to_waveform_in_a_random_voice(tts):
	from tortoise_tts_amd.tts import set_seed
	with_rlg, without = tts
	text = "Hello there, Mr. Fox."
	kw = dict(max_ar_steps=10, max_diffusion_steps=3)
	out, sr = with_rlg.inference(text, None, seed=7, **kw)
	out2, _ = with_rlg.inference(text, seed=7, **kw)
	assert sr == 24000 and out.dim() == 3 and out.shape[:2] == (1, 1) and torch.isfinite(out).all() and torch.equal(out, out2)
	set_seed(7)
	v7 = with_rlg.random_voice()
	a, d = v7["latent"]
	assert a.shape == (1, W.AR_SMALL.model_dim) and d.shape == (1, 2 * W.DIFF_SMALL.model_channels) and with_rlg.encode_audio(v7) is v7
	out3, _ = with_rlg.inference(text, v7, seed=7, **kw)
	assert torch.equal(out, out3)
	# the autoregressive latent is drawn first, then the diffusion one
	set_seed(7)
	assert torch.equal(with_rlg.rlg_auto(torch.zeros(1, 1)), a) and torch.equal(with_rlg.rlg_diffuser(torch.zeros(1, 1)), d)
	set_seed(8)
	v8 = with_rlg.random_voice()
	assert not torch.equal(v8["latent"][0], a) and not torch.equal(v8["latent"][1], d)
	three = with_rlg.random_voice(rows=3)["latent"]
	assert three[0].shape == (3, W.AR_SMALL.model_dim) and three[1].shape == (3, 2 * W.DIFF_SMALL.model_channels)
	with pytest.raises(ValueError, match="rlg_auto"):
		without.inference(text, None, seed=7, **kw)
	with pytest.raises(ValueError, match="rlg_auto"):
		without.random_voice()
