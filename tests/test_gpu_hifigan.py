"""HiFiGAN vocoder on libttk (`ttk_hifigan_*`, vocoder_type="hifigan") against the reference's waveforms (tests/golden/hifigan_*.npz, written by
tools/make_golden_hifigan.py from models/hifigan.py) and the CPU oracle (tests/hifigan_oracle.py); the streaming loop; the `TTS` wiring.  GPU only.

bf16 bounds.  The bf16 path rounds every convolution's weights and input to bf16 and accumulates in f32 (conv_post and cond_layer stay f32).  The
oracle run that way on the CPU (`HiFiGANOracle(round=bf16)`) has, against the reference's f32 waveform (relative L2, max |error|):
    hifigan_small n = 13: 3.67e-3, 5.15e-3    n = 2: 4.01e-3, 4.20e-3
    hifigan_full  n = 13: 6.03e-3, 6.14e-3    n = 2: 6.21e-3, 5.37e-3
    hifigan_cfg1 (n = 250, the stored samples): 7.55e-3, 5.79e-3
and against the f64 oracle at the edge shapes n = 1, 2, 3, 7, 61:
    HIFIGAN_SMALL (seed 95): 4.81e-3, 3.05e-3 | 4.76e-3, 3.76e-3 | 3.62e-3, 3.67e-3 | 3.66e-3, 5.66e-3 | 2.77e-3, 4.56e-3
    HIFIGAN_FULL  (seed 96): 6.52e-3, 3.67e-3 | 6.11e-3, 4.93e-3 | 6.54e-3, 5.40e-3 | 6.35e-3, 5.63e-3 | 6.60e-3, 5.52e-3
The GPU path is allowed 2 x these (summation order; the stored operand copy is rounded at a different point), case by case.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

import hifigan_oracle as HO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFGS = {"hifigan_small": W.HIFIGAN_SMALL, "hifigan_full": W.HIFIGAN_FULL}
# (relative L2, max |error|) of the bf16-operand model, see the module docstring
BF16_FIXTURE = {("hifigan_small", 13): (3.67e-3, 5.15e-3), ("hifigan_small", 2): (4.01e-3, 4.20e-3),
				("hifigan_full", 13): (6.03e-3, 6.14e-3), ("hifigan_full", 2): (6.21e-3, 5.37e-3), "hifigan_cfg1": (7.55e-3, 5.79e-3)}
BF16_EDGE = {("small", 1): (4.81e-3, 3.05e-3), ("small", 2): (4.76e-3, 3.76e-3), ("small", 3): (3.62e-3, 3.67e-3), ("small", 7): (3.66e-3, 5.66e-3),
			 ("small", 61): (2.77e-3, 4.56e-3), ("full", 1): (6.52e-3, 3.67e-3), ("full", 2): (6.11e-3, 4.93e-3), ("full", 3): (6.54e-3, 5.40e-3),
			 ("full", 7): (6.35e-3, 5.63e-3), ("full", 61): (6.60e-3, 5.52e-3)}
EDGE_CFG = {"small": (W.HIFIGAN_SMALL, 95), "full": (W.HIFIGAN_FULL, 96)}


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def rel_l2(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def make(cfg, seed, dtype):
	from tortoise_tts_amd.hifigan import HiFiGAN
	sd = W.synth_state_dict(W.hifigan_shapes(cfg), seed)
	return HiFiGAN(sd, cfg, dtype=dtype, device=DEV), sd


def within_bf16(audio, ref, model):
	r, m = rel_l2(audio, ref), maxerr(audio, ref)
	print(f"bf16: rel_l2 {r:.3e} (bound {2 * model[0]:.3e}), max {m:.3e} (bound {2 * model[1]:.3e})")
	return r < 2 * model[0] and m < 2 * model[1]


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("n", [13, 2])
def test_f32_equals_reference_waveform(golden, name, n):
	g = golden(name)
	voc, _ = make(CFGS[name], int(g["seed"]), "f32")
	audio = voc.inference(t(g[f"latents_{n}"]).to(DEV), t(g[f"g_{n}"]).to(DEV))
	assert audio.shape == g[f"audio_{n}"].shape and audio.dtype == torch.float32
	print("f32 max error", maxerr(audio, g[f"audio_{n}"]))
	assert maxerr(audio, g[f"audio_{n}"]) < 1e-4


@pytest.mark.parametrize("which", sorted(EDGE_CFG))
@pytest.mark.parametrize("n", [1, 2, 3, 7, 61])
def test_f32_edge_shapes_vs_oracle(which, n):
	"""n = 1, 2: the second interpolation is a copy; every stage has rows next to both sequence ends, and the short ones are nothing else"""
	cfg, seed = EDGE_CFG[which]
	voc, sd = make(cfg, seed, "f32")
	lat, cond = HO.fixture_inputs(n, 100 + n, cfg)
	with torch.inference_mode():
		ref = HO.HiFiGANOracle(sd, cfg, torch.float64).inference(lat, cond)
	audio = voc.inference(lat.to(DEV), cond.to(DEV))
	print("f32 max error", maxerr(audio, ref))
	assert audio.shape == ref.shape == (1, 1, cfg.frames(n) * cfg.hop_length) and maxerr(audio, ref) < 1e-4


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("n", [13, 2])
def test_bf16_within_stated_distance_of_reference(golden, name, n):
	g = golden(name)
	voc, _ = make(CFGS[name], int(g["seed"]), "bf16")
	audio = voc.inference(t(g[f"latents_{n}"]).to(DEV), t(g[f"g_{n}"]).to(DEV))
	assert within_bf16(audio, g[f"audio_{n}"], BF16_FIXTURE[(name, n)])


@pytest.mark.parametrize("which", sorted(EDGE_CFG))
@pytest.mark.parametrize("n", [1, 2, 3, 7, 61])
def test_bf16_mfma_conv_edge_shapes_vs_oracle(which, n, monkeypatch):
	"""bf16 with the narrow-channel MFMA convolution on (the stages of 64 and 32 channels -- both stages of the small config): sequences shorter than
	one 256-row tile, tiles cut by the sequence end, halos of up to 25 rows that reach past both ends -- against the f64 oracle"""
	monkeypatch.setenv("TTK_HIFI_NARROW", "1")
	cfg, seed = EDGE_CFG[which]
	voc, sd = make(cfg, seed, "bf16")
	lat, cond = HO.fixture_inputs(n, 100 + n, cfg)
	with torch.inference_mode():
		ref = HO.HiFiGANOracle(sd, cfg, torch.float64).inference(lat, cond)
	audio = voc.inference(lat.to(DEV), cond.to(DEV))
	assert audio.shape == ref.shape and within_bf16(audio, ref, BF16_EDGE[(which, n)])


def test_bf16_segment_gemm_route_meets_the_same_bound(golden, monkeypatch):
	"""TTK_HIFI_NARROW=0 (read at create) keeps every ResBlock on the segment GEMM: the route the MFMA convolution is timed against"""
	g = golden("hifigan_small")
	monkeypatch.setenv("TTK_HIFI_NARROW", "0")
	voc, _ = make(W.HIFIGAN_SMALL, int(g["seed"]), "bf16")
	monkeypatch.setenv("TTK_HIFI_NARROW", "1")
	nar, _ = make(W.HIFIGAN_SMALL, int(g["seed"]), "bf16")
	lat, cond = t(g["latents_13"]).to(DEV), t(g["g_13"]).to(DEV)
	a, b = voc.inference(lat, cond), nar.inference(lat, cond)
	assert within_bf16(a, g["audio_13"], BF16_FIXTURE[("hifigan_small", 13)]) and within_bf16(b, g["audio_13"], BF16_FIXTURE[("hifigan_small", 13)])
	# (both routes feed the same MFMA the same products in the same order -- tap, then input-channel block -- so the two waveforms may well be equal bit for
	# bit; that the switch switches is what tests/diag/hifigan_time.py shows, by the clock)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cfg1_length(golden, dtype):
	"""configs[1] length: 250 latents, F = 1088 frames, 278,528 samples"""
	g = golden("hifigan_cfg1")
	lat, cond = HO.fixture_inputs(int(g["n"]), int(g["input_seed"]))
	voc, _ = make(W.HIFIGAN_FULL, int(g["seed"]), dtype)
	audio = voc.inference(lat.to(DEV), cond.to(DEV)).cpu()
	assert audio.shape == tuple(g["audio_shape"]) == (1, 1, 1088 * 256)
	got = torch.cat([audio[..., :2560], audio[..., -2560:], audio[..., ::4]], dim=-1)
	ref = torch.cat([t(g["audio_head"]), t(g["audio_tail"]), t(g["audio_every4"])], dim=-1)
	if dtype == "f32":
		print("f32 max error", maxerr(got, ref))
		assert maxerr(got, ref) < 1e-4
	else:
		assert within_bf16(got, ref, BF16_FIXTURE["hifigan_cfg1"])


def test_weight_norm_input_and_checkpoint_equal_plain_weights(golden, tmp_path):
	from tortoise_tts_amd.checkpoint import load_hifigan
	from tortoise_tts_amd.hifigan import HiFiGAN
	g = golden("hifigan_small")
	cfg = W.HIFIGAN_SMALL
	voc, sd = make(cfg, int(g["seed"]), "f32")
	lat, cond = t(g["latents_13"]).to(DEV), t(g["g_13"]).to(DEV)
	plain = voc.inference(lat, cond)
	def weight_norm(scale):
		out = {}
		for k, v in sd.items():
			if k.endswith(".weight") and v.dim() == 3 and not k.startswith("cond_layer."):      # ups.*: dimension 0 is the INPUT channel, as in torch
				out[k[:-len("weight")] + "weight_v"] = v * scale
				out[k[:-len("weight")] + "weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1)
			else:
				out[k] = v
		return out
	wn = weight_norm(1.0)                   # g = ||v|| exactly: the fold multiplies by g / ||v|| = 1, so the weights are the plain ones bit for bit
	assert sorted(wn) == sorted(str(k) for k in g["keys"])
	assert torch.equal(HiFiGAN(wn, cfg, dtype="f32", device=DEV).inference(lat, cond), plain)
	assert maxerr(HiFiGAN(weight_norm(3.0), cfg, dtype="f32", device=DEV).inference(lat, cond), plain) < 1e-5
	path = tmp_path / "hifigan.pth"
	torch.save(wn, path)                    # a plain state dict, no sub-key
	assert torch.equal(load_hifigan(path, cfg=cfg, dtype="f32", device=DEV).inference(lat, cond), plain)


@pytest.mark.parametrize("change,message", [(dict(resblock_type="2"), 'resblock_type "2" unsupported'),
											(dict(upsample_kernel_sizes=(7, 4)), "the stride must divide the kernel"),
											(dict(cond_channels=0), "without a cond_layer is not built"),
											(dict(resblock_kernel_sizes=(3, 13, 11)), "resblock kernel 13 unsupported")])
def test_create_rejects_unsupported_config(change, message):
	from tortoise_tts_amd.hifigan import HiFiGAN
	cfg = dataclasses.replace(W.HIFIGAN_SMALL, **change)
	sd = W.synth_state_dict(W.hifigan_shapes(W.HIFIGAN_SMALL), 83)
	with pytest.raises(_lib.TTKError, match=message):
		HiFiGAN(sd, cfg, dtype="f32", device=DEV)


def test_inference_rejects_bad_input():
	voc, _ = make(W.HIFIGAN_SMALL, 84, "f32")
	with pytest.raises(_lib.TTKError, match="latents must be"):
		voc.inference(torch.zeros(1, 0, 128), torch.zeros(1, 128))
	with pytest.raises(_lib.TTKError, match="g must be"):
		voc.inference(torch.zeros(1, 3, 128), torch.zeros(1, 64))
	rc = voc.lib.ttk_hifigan_inference(voc._h, 1, 1 << 20, 1, _lib.stream_ptr())
	assert rc == -1 and b"too long" in voc.lib.ttk_last_error()


# ------------------------------------------------------------------------------------------------------------ the streaming loop
OVERLAP = 32       # HIFIGAN_SMALL has hop 8: one more latent is 4 frames = 32 samples, and a chunk shorter than the cross-fade fails here as in the reference


@pytest.fixture(scope="module")
def stream_setup(golden):
	g = golden("hifigan_stream")
	cfg = W.HIFIGAN_SMALL
	voc, _ = make(cfg, int(g["seed"]), "f32")
	lat, cond = HO.fixture_inputs(117, int(g["input_seed"]), cfg)
	pairs = [(torch.tensor([i]), lat[0, i:i + 1].to(DEV)) for i in range(117)]      # (codes, latent [1, C]) as get_generator yields them
	return g, voc, pairs, cond.to(DEV)


@pytest.mark.parametrize("count,calls", [(117, [60, 100, 117]), (100, [60, 100]), (61, [60, 61]), (60, [60]), (59, [59])])
def test_stream_equals_the_reference_chunks(stream_setup, count, calls):
	"""chunks of `stream` = inference.py:300-310 applied to the reference generator's waveforms on the first 60 / 100 / 117 latents (59, 61: the oracle's).
	Ending exactly on a boundary (60, 100) emits nothing more and does not run the vocoder again."""
	g, voc, pairs, cond = stream_setup
	assert HO.stream_plan(count) == calls
	seen = []
	inner = voc.inference
	voc.inference = lambda c, gg: (seen.append(c.shape[1]), inner(c, gg))[1]
	try:
		chunks = list(voc.stream(iter(pairs[:count]), cond, overlap=OVERLAP))
	finally:
		del voc.inference
	assert seen == calls
	wavs = []
	for n in calls:
		if f"wav_{n}" in g:
			wavs.append(t(g[f"wav_{n}"]))
		else:
			sd = W.synth_state_dict(W.hifigan_shapes(W.HIFIGAN_SMALL), int(g["seed"]))
			with torch.inference_mode():
				wavs.append(HO.HiFiGANOracle(sd, W.HIFIGAN_SMALL).inference(torch.cat([p[1] for p in pairs[:n]], 0)[None].cpu(), cond.cpu()).reshape(-1))
	want = HO.stream_chunks(wavs, overlap=OVERLAP)
	assert len(chunks) == len(want)
	for c, w in zip(chunks, want):
		assert c.shape == (1, w.shape[0]) and maxerr(c[0], w) < 1e-4
	assert sum(c.shape[-1] for c in chunks) == W.HIFIGAN_SMALL.frames(count) * W.HIFIGAN_SMALL.hop_length - OVERLAP


def test_stream_yields_the_first_chunk_before_the_iterator_is_exhausted(stream_setup):
	_, voc, pairs, cond = stream_setup
	taken = []
	def feed():
		for p in pairs:
			taken.append(1)
			yield p
	s = voc.stream(feed(), cond, overlap=OVERLAP)
	first = next(s)
	assert len(taken) == 60 and first.shape == (1, W.HIFIGAN_SMALL.frames(60) * 8 - OVERLAP)
	s.close()


# ------------------------------------------------------------------------------------------------------------ TTS(vocoder_type="hifigan")
# hop 256 as published (a chunk of 10 latents is 43 frames = 11,008 samples, more than the 1024-sample cross-fade), AR_SMALL's latent width
TTS_CFG = W.HiFiGANConfig(in_channels=128, cond_channels=128, upsample_initial_channel=128)
KW = dict(max_ar_steps=70, ar_temp=0.9, top_k=40, top_p=0.95, repetition_penalty=1.5)


@pytest.fixture(scope="module")
def parts(golden):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.hifigan import HiFiGAN
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	sd = dict(ar=W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), df=W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32),
			  hg=W.synth_state_dict(W.hifigan_shapes(TTS_CFG), 37), arc=W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35),
			  dfc=W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36))
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	common = dict(conditioning_encoder=ConditioningEncoder(sd["arc"], W.AR_SMALL, dtype="f32", device=DEV),
				  contextual_embedder=ContextualEmbedder(sd["dfc"], W.DIFF_SMALL, dtype="f32", device=DEV),
				  tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV))
	ar = UnifiedVoice(sd["ar"], W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=160)
	df = DiffusionTTS(sd["df"], W.DIFF_SMALL, dtype="f32", device=DEV)
	hg = HiFiGAN(sd["hg"], TTS_CFG, dtype="f32", device=DEV)
	return TTS(ar, df, tok, hifigan=hg, **common), TTS(ar, df, tok, **common)


def clip():
	n, sr = 30000, 22050
	tt = torch.arange(n) / sr
	return (0.3 * torch.sin(2 * math.pi * 180 * tt) + 0.02 * torch.randn(n, generator=torch.Generator().manual_seed(9)))[None]


def by_hand(tts, line, enc):
	ar, al = tts.hot.autoregressive, enc["latent"][0]
	tokens = tts.encode_text(line).to(DEV)[None]
	with torch.inference_mode():           # as TTS.inference runs: the model's generation state was made there
		inputs = ar.compute_embeddings(al, tokens)
		gen = ar.get_generator(inputs=inputs, max_length=min(500, inputs.shape[1] + KW["max_ar_steps"]), top_k=KW["top_k"], top_p=KW["top_p"],
							   temperature=KW["ar_temp"], repetition_penalty=KW["repetition_penalty"], length_penalty=1.0, do_sample=True, num_return_sequences=1)
		pairs = [(c.clone(), l.clone()) for c, l in gen]
		chunks = list(tts.hifigan.stream(iter(pairs), al))
	return torch.concat(chunks, dim=-1)[None], len(pairs), len(chunks)


def test_tts_vocoder_type_hifigan_single_line(parts):
	tts, _ = parts
	enc = tts.encode_audio(clip().to(DEV), 22050)
	torch.manual_seed(5)                                              # the global generator's state must not matter
	out, sr = tts.inference("Hello there, Mr. Fox.", enc, seed=1234, vocoder_type="hifigan", max_diffusion_steps=3, candidates=2, **KW)
	want, n_pairs, n_chunks = by_hand(tts, "Hello there, Mr. Fox.", enc)
	assert 1 <= n_pairs <= 70 and n_chunks == len(HO.stream_plan(n_pairs))
	assert sr == 24000 and out.shape == (1, 1, TTS_CFG.frames(n_pairs) * 256 - 1024) and torch.equal(out, want)
	assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
	# neither `seed` nor the generators' state reach the result: the token loop reseeds to 0 per line and nothing else draws
	torch.manual_seed(77)
	torch.cuda.manual_seed(78)
	again, _ = tts.inference("Hello there, Mr. Fox.", enc, seed=99, vocoder_type="hifigan", **KW)
	assert torch.equal(again, out)                                    # and the AR handle was idle again after the first stream


def test_tts_vocoder_type_hifigan_lines(parts):
	tts, _ = parts
	enc = tts.encode_audio(clip().to(DEV), 22050)
	lines = ["Hello there, Mr. Fox.", "The end!"]
	out, _ = tts.inference("\n".join(lines), enc, seed=1234, vocoder_type="hifigan", **KW)
	singles = [tts.inference(line, enc, seed=4321, vocoder_type="hifigan", **KW)[0] for line in lines]
	assert out.shape[-1] == sum(s.shape[-1] for s in singles) and torch.equal(out, torch.concat(singles, dim=-1))
	tts.hot.autoregressive._require_idle()                            # the other generation entry points work on the same model afterwards
	# the chunks as they come, outside inference mode: the same samples
	tokens = tts.encode_text(lines[1]).to(DEV)[None]
	chunks = list(tts.hifigan_chunks(tokens, enc["latent"][0], **KW))
	assert all(c.dim() == 2 and c.shape[0] == 1 for c in chunks) and torch.equal(torch.concat(chunks, dim=-1)[None], singles[1])


def test_tts_hifigan_needs_the_part_and_no_beams(parts):
	tts, bare = parts
	enc = bare.encode_audio(clip().to(DEV), 22050)
	with pytest.raises(NotImplementedError, match="hifigan="):
		bare.inference("Hello.", enc, vocoder_type="hifigan", **KW)
	with pytest.raises(NotImplementedError, match="beam"):
		tts.inference("Hello.", enc, vocoder_type="hifigan", beam_width=2, **KW)
