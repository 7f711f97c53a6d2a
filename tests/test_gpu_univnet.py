"""UnivNet vocoder on libttk (`ttk_univnet_*`, vocoder_type="vocoder") against the reference's waveforms (tests/golden/univnet_*.npz, written by
tools/make_golden_univnet.py from models/vocoder.py) and the CPU oracle (tests/univnet_oracle.py); the `TTS` wiring of its noise.  GPU only."""
import math

import numpy as np
import pytest
import torch

import univnet_oracle as UO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFGS = {"univnet_small": W.UNIVNET_SMALL, "univnet_full": W.UNIVNET_FULL}


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def rel_l2(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def make(cfg, seed, dtype):
	from tortoise_tts_amd.univnet import UnivNet
	sd = W.synth_state_dict(W.univnet_shapes(cfg), seed)
	return UnivNet(sd, cfg, dtype=dtype, device=DEV), sd


@pytest.mark.parametrize("name", sorted(CFGS))
def test_f32_equals_reference_waveform(golden, name):
	g = golden(name)
	voc, _ = make(CFGS[name], int(g["seed"]), "f32")
	audio = voc.inference(t(g["mel"]).to(DEV), t(g["z"]))
	assert audio.shape == g["audio"].shape and audio.dtype == torch.float32
	assert maxerr(audio, g["audio"]) < 1e-4


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (3, 5), (2, 64)])
def test_f32_edge_shapes_vs_oracle(B, T):
	"""one-frame mels (the reflect pads and every segment next to a sequence end), several batch elements"""
	cfg = W.UNIVNET_SMALL
	voc, sd = make(cfg, 81, "f32")
	gen = torch.Generator().manual_seed(100 * B + T)
	mel = torch.randn(B, 100, T, generator=gen) * 2 - 5
	z = torch.randn(B, cfg.noise_dim, T + 10, generator=gen)
	with torch.inference_mode():
		ref = UO.UnivNetOracle(sd, cfg).inference(mel, z)
	audio = voc.inference(mel.to(DEV), z)
	assert audio.shape == ref.shape == (B, 1, T * cfg.hop_length) and maxerr(audio, ref) < 1e-4


@pytest.mark.parametrize("name", sorted(CFGS))
def test_bf16_within_stated_distance_of_reference(golden, name):
	g = golden(name)
	voc, _ = make(CFGS[name], int(g["seed"]), "bf16")
	audio = voc.inference(t(g["mel"]).to(DEV), t(g["z"]))
	# bf16 operands (8-bit mantissa, 2^-9 relative rounding) in every GEMM and in the predicted kernels, f32 accumulation and residual stream:
	# a few 1e-3 relative per layer over 3 blocks x 4 layers; the synthetic weights drive conv_post into tanh's steep region, so single
	# samples move more than the waveform as a whole
	assert rel_l2(audio, g["audio"]) < 3e-2 and maxerr(audio, g["audio"]) < 0.15, (rel_l2(audio, g["audio"]), maxerr(audio, g["audio"]))


@pytest.mark.parametrize("B,T", [(1, 1), (3, 5)])
def test_bf16_mfma_lvc_edge_shapes_vs_oracle(B, T):
	"""the published config in bf16 runs the MFMA form of the LVC (c_g = 32): one-frame mels, 16-row tiles spanning two hop-8 segments,
	tiles cut by the sequence end, several batch elements -- against the f64 oracle, with the bound of the fixture test above"""
	cfg = W.UNIVNET_FULL
	voc, sd = make(cfg, 85, "bf16")
	mel, z = UO.fixture_inputs(B, T, 10 * B + T, 20 * B + T)
	with torch.inference_mode():
		ref = UO.UnivNetOracle(sd, cfg, torch.float64).inference(mel, z)
	audio = voc.inference(mel.to(DEV), z)
	assert audio.shape == ref.shape == (B, 1, T * cfg.hop_length)
	assert rel_l2(audio, ref) < 3e-2 and maxerr(audio, ref) < 0.15, (rel_l2(audio, ref), maxerr(audio, ref))


def cfg1_reference(g):
	n = int(g["audio_shape"][-1])
	return n, g["audio_head"], g["audio_tail"], g["audio_every4"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cfg1_length(golden, dtype):
	"""configs[1] length: T = 1088 frames, 278,528 samples"""
	g = golden("univnet_cfg1")
	mel, z = UO.fixture_inputs(1, int(g["T"]), int(g["mel_seed"]), int(g["z_seed"]))
	voc, _ = make(W.UNIVNET_FULL, int(g["seed"]), dtype)
	audio = voc.inference(mel.to(DEV), z).cpu()
	n, head, tail, every4 = cfg1_reference(g)
	assert audio.shape == (1, 1, n) == (1, 1, 1088 * 256)
	got = torch.cat([audio[..., :2560], audio[..., -2560:], audio[..., ::4]], dim=-1)
	ref = torch.cat([t(head), t(tail), t(every4)], dim=-1)
	if dtype == "f32":
		assert maxerr(got, ref) < 1e-4
	else:
		assert rel_l2(got, ref) < 3e-2, rel_l2(got, ref)       # the bound of the short fixtures: the error does not grow with length


def test_weight_norm_input_and_checkpoint_equal_plain_weights(golden, tmp_path):
	from tortoise_tts_amd.checkpoint import load_univnet
	from tortoise_tts_amd.univnet import UnivNet
	g = golden("univnet_small")
	cfg = W.UNIVNET_SMALL
	voc, sd = make(cfg, int(g["seed"]), "f32")
	mel, z = t(g["mel"]).to(DEV), t(g["z"])
	plain = voc.inference(mel, z)
	def weight_norm(scale):
		out = {}
		for k, v in sd.items():
			if k.endswith(".weight") and v.dim() == 3:
				out[k[:-len("weight")] + "weight_v"] = v * scale
				out[k[:-len("weight")] + "weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1)
			else:
				out[k] = v
		return out
	wn = weight_norm(1.0)                   # g = ||v|| exactly: the fold multiplies by g / ||v|| = 1, so the weights are the plain ones bit for bit
	assert torch.equal(UnivNet(wn, cfg, dtype="f32", device=DEV).inference(mel, z), plain)
	assert maxerr(UnivNet(weight_norm(3.0), cfg, dtype="f32", device=DEV).inference(mel, z), plain) < 1e-5
	path = tmp_path / "vocoder.pth"
	torch.save({"model_g": wn}, path)
	assert torch.equal(load_univnet(path, cfg=cfg, dtype="f32", device=DEV).inference(mel, z), plain)


def test_default_noise_is_the_cpu_generator_draw():
	voc, _ = make(W.UNIVNET_SMALL, 82, "f32")
	mel = (torch.randn(2, 100, 7, generator=torch.Generator().manual_seed(3)) * 2 - 5).to(DEV)
	torch.manual_seed(11)
	a = voc.inference(mel)
	torch.manual_seed(11)
	z = torch.randn(2, 64, 17)
	assert torch.equal(a, voc.inference(mel, z)) and torch.equal(a, voc.inference(mel, z))


@pytest.mark.parametrize("field,value,message", [("conv_kernel_size", 5, "LVC kernel size 5 unsupported"), ("channel_size", 24, "channel_size 24 unsupported"),
											   ("hop_length", 128, "strides multiply to 16, not the hop length 128")])
def test_create_rejects_unsupported_config(field, value, message):
	import dataclasses
	cfg = dataclasses.replace(W.UNIVNET_SMALL, **{field: value})
	sd = W.synth_state_dict(W.univnet_shapes(W.UNIVNET_SMALL), 83)
	from tortoise_tts_amd.univnet import UnivNet
	with pytest.raises(_lib.TTKError, match=message):
		UnivNet(sd, cfg, dtype="f32", device=DEV)


def test_inference_rejects_lengths_past_the_buffer_range():
	voc, _ = make(W.UNIVNET_SMALL, 84, "f32")
	rc = voc.lib.ttk_univnet_inference(voc._h, 1, 1, 1 << 20, 1 << 12, 1, _lib.stream_ptr())
	assert rc == -1 and b"too long" in voc.lib.ttk_last_error()


# ------------------------------------------------------------------------------------------------------------ TTS(vocoder_type="vocoder")
@pytest.fixture(scope="module")
def parts(golden):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.univnet import UnivNet
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	sd = dict(ar=W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), df=W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32),
			  uv=W.synth_state_dict(W.univnet_shapes(W.UNIVNET_SMALL), 34), arc=W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35),
			  dfc=W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36))
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	common = dict(conditioning_encoder=ConditioningEncoder(sd["arc"], W.AR_SMALL, dtype="f32", device=DEV),
				  contextual_embedder=ContextualEmbedder(sd["dfc"], W.DIFF_SMALL, dtype="f32", device=DEV),
				  tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV))
	ar = UnifiedVoice(sd["ar"], W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=128)
	df = DiffusionTTS(sd["df"], W.DIFF_SMALL, dtype="f32", device=DEV)
	uv = UnivNet(sd["uv"], W.UNIVNET_SMALL, dtype="f32", device=DEV)
	return TTS(ar, df, tok, univnet=uv, **common), TTS(ar, df, tok, **common)


def clip():
	n, sr = 30000, 22050
	tt = torch.arange(n) / sr
	return (0.3 * torch.sin(2 * math.pi * 180 * tt) + 0.02 * torch.randn(n, generator=torch.Generator().manual_seed(9)))[None]


# The contract: the reference's `generate` calls setup_seed(0) once per line (stream_generator.py:36-45, 296), which reseeds the CPU
# generator; nothing draws from it afterwards until `vocoder.inference` (AR sampling and the diffusion noise use the device generator,
# inference.py:404), whose `torch.randn(B, 64, T + 10)` (models/vocoder.py:309) is therefore the first draw after torch.manual_seed(0).
KW = dict(max_ar_steps=10, max_diffusion_steps=3, candidates=2)


def first_draw(T):
	return torch.randn(1, W.UNIVNET_SMALL.noise_dim, T + 10, generator=torch.Generator().manual_seed(0))


def test_tts_vocoder_type_vocoder_single_line(parts):
	from tortoise_tts_amd.tts import set_seed
	tts, _ = parts
	enc = tts.encode_audio(clip().to(DEV), 22050)
	torch.manual_seed(5)                                              # the global generator's state must not matter
	out, sr = tts.inference("Hello there, Mr. Fox.", enc, seed=1234, vocoder_type="vocoder", **KW)
	set_seed(1234)
	tokens = tts.encode_text("Hello there, Mr. Fox.").to(DEV)[None]
	mels, _ = tts.hot.inference(tokens, enc["latent"][0], enc["latent"][1], **KW)
	by_hand = tts.univnet.inference(mels, first_draw(mels.shape[-1]))
	assert sr == 24000 and out.shape == (1, 1, mels.shape[-1] * W.UNIVNET_SMALL.hop_length) and torch.equal(out, by_hand)
	assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0


def test_tts_vocoder_type_vocoder_lines(parts):
	"""the inference_lines branch: each line gets the same-state draw at its own length and equals its single-line call bit for bit"""
	tts, _ = parts
	enc = tts.encode_audio(clip().to(DEV), 22050)
	lines = ["Hello there, Mr. Fox.", "The end!"]
	out, _ = tts.inference("\n".join(lines), enc, seed=1234, vocoder_type="vocoder", **KW)
	singles = [tts.inference(line, enc, seed=1234, vocoder_type="vocoder", **KW)[0] for line in lines]
	assert out.shape[-1] == sum(s.shape[-1] for s in singles) and torch.equal(out, torch.concat(singles, dim=-1))


def test_tts_vocoder_type_needs_univnet(parts):
	_, bare = parts
	enc = bare.encode_audio(clip().to(DEV), 22050)
	with pytest.raises(ValueError, match="univnet"):
		bare.inference("Hello.", enc, vocoder_type="vocoder", **KW)
	with pytest.raises(NotImplementedError):
		bare.inference("Hello.", enc, vocoder_type="hifigan", **KW)
