"""The HiFiGAN CPU oracle (tests/hifigan_oracle.py) against the reference's own generator (tests/golden/hifigan_*.npz, written by
tools/make_golden_hifigan.py): the interpolated latents, conv_pre + cond_layer, the first transposed conv, the first stage's MRF mean and the
audio; the interpolation rule; the boundaries of the streaming loop.  CPU only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_oracle as HO
from tortoise_tts_amd import weights as W

CFGS = {"hifigan_small": (W.HIFIGAN_SMALL, ""), "hifigan_full": (W.HIFIGAN_FULL, "sub")}


def maxerr(a, b):
	return (torch.as_tensor(np.asarray(a)).double() - torch.as_tensor(np.asarray(b)).double()).abs().max().item()


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("n", [13, 2])
def test_oracle_equals_reference(golden, name, n):
	g, (cfg, sub) = golden(name), CFGS[name]
	fs, ss = (2, 4) if sub else (1, 1)
	sf, sx = (f"_{fs}", f"_{ss}") if sub else ("", "")
	sd = W.synth_state_dict(W.hifigan_shapes(cfg), int(g["seed"]))
	lat, cond = HO.fixture_inputs(n, int(g[f"input_seed_{n}"]), cfg)
	assert torch.equal(lat, torch.from_numpy(g[f"latents_{n}"])) and torch.equal(cond, torch.from_numpy(g[f"g_{n}"]))
	o = HO.HiFiGANOracle(sd, cfg, torch.float32)
	with torch.inference_mode():
		audio = o.inference(lat, cond)
	tr = o.trace
	assert audio.shape == g[f"audio_{n}"].shape == (1, 1, cfg.frames(n) * cfg.hop_length)
	# same operations as the reference in f32, in a different order at most
	assert maxerr(tr["interp"][..., ::fs], g[f"interp{sf}_{n}"]) < 1e-5
	assert maxerr(tr["conv_pre"][..., ::fs], g[f"conv_pre{sf}_{n}"]) < 1e-5
	assert maxerr(tr["ups0"][..., ::ss], g[f"ups0{sx}_{n}"]) < 1e-5
	assert maxerr(tr["stage0"][..., ::ss], g[f"stage0{sx}_{n}"]) < 1e-5
	assert maxerr(audio, g[f"audio_{n}"]) < 1e-5


def test_oracle_equals_reference_cfg1(golden):
	"""configs[1] length: 250 latents, F = 1088 frames, 278,528 samples"""
	g = golden("hifigan_cfg1")
	cfg = W.HIFIGAN_FULL
	lat, cond = HO.fixture_inputs(int(g["n"]), int(g["input_seed"]), cfg)
	with torch.inference_mode():
		audio = HO.HiFiGANOracle(W.synth_state_dict(W.hifigan_shapes(cfg), int(g["seed"])), cfg).inference(lat, cond)
	assert tuple(audio.shape) == tuple(g["audio_shape"]) == (1, 1, 1088 * 256)
	assert maxerr(audio[..., :2560], g["audio_head"]) < 1e-5 and maxerr(audio[..., -2560:], g["audio_tail"]) < 1e-5
	assert maxerr(audio[..., ::4], g["audio_every4"]) < 1e-5


def test_oracle_equals_reference_stream_waveforms(golden):
	g = golden("hifigan_stream")
	cfg = W.HIFIGAN_SMALL
	lat, cond = HO.fixture_inputs(117, int(g["input_seed"]), cfg)
	o = HO.HiFiGANOracle(W.synth_state_dict(W.hifigan_shapes(cfg), int(g["seed"])), cfg)
	with torch.inference_mode():
		for n in (60, 100, 117):
			assert maxerr(o.inference(lat[:, :n], cond).reshape(-1), g[f"wav_{n}"]) < 1e-5


@pytest.mark.parametrize("n", [1, 2, 3, 7, 60, 100, 250])
def test_interpolation_rule(n):
	"""the written-out rule equals F.interpolate twice (f64), n = 1, 2 being the equal-length copy of the second stage; frame and sample counts"""
	x = torch.randn(1, 5, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
	want = F.interpolate(F.interpolate(x, scale_factor=[1024 / 256], mode="linear"), scale_factor=[24000 / 22050], mode="linear")
	got = HO.interp_linear(HO.interp_linear(x, HO.SCALES[0]), HO.SCALES[1])
	assert got.shape == want.shape == (1, 5, W.HIFIGAN_FULL.frames(n)) and maxerr(got, want) < 1e-12
	if n <= 2:
		assert got.shape[-1] == 4 * n and torch.equal(got, HO.interp_linear(x, HO.SCALES[0]))
	samples = {1: 1024, 2: 2048, 7: 7680, 60: 66816, 100: 111360, 250: 278528}
	if n in samples:
		assert W.HIFIGAN_FULL.frames(n) * W.HIFIGAN_FULL.hop_length == samples[n]


@pytest.mark.parametrize("pairs,calls", [(59, [59]), (60, [60]), (61, [60, 61]), (100, [60, 100]), (117, [60, 100, 117]), (1, [1]), (140, [60, 100, 140])])
def test_stream_plan_boundaries(pairs, calls):
	assert HO.stream_plan(pairs) == calls


def test_stream_chunks_compose(golden):
	"""chunk k is wav_k[len_{k-1} - overlap : -overlap] with its head cross-faded against the previous call's tail; total = last length - overlap"""
	g = golden("hifigan_stream")
	ov = 256
	wavs = [torch.from_numpy(g[f"wav_{n}"]) for n in (60, 100, 117)]
	chunks = HO.stream_chunks(wavs, overlap=ov)
	assert [c.shape[0] for c in chunks] == [wavs[0].shape[0] - ov, wavs[1].shape[0] - wavs[0].shape[0], wavs[2].shape[0] - wavs[1].shape[0]]
	assert sum(c.shape[0] for c in chunks) == W.HIFIGAN_SMALL.frames(117) * W.HIFIGAN_SMALL.hop_length - ov
	assert torch.equal(chunks[0], wavs[0][:-ov])
	L0 = wavs[0].shape[0]
	assert torch.equal(chunks[1][ov:], wavs[1][L0:-ov])
	# cross-fade ends: the first sample is the previous waveform's, the last one the new waveform's
	assert chunks[1][0] == wavs[0][L0 - ov] and chunks[1][ov - 1] == wavs[1][L0 - 1]
	assert all(torch.equal(w, torch.from_numpy(g[f"wav_{n}"])) for w, n in zip(wavs, (60, 100, 117)))      # the inputs are left as they were


def test_key_list_is_the_reference_state_dict(golden):
	keys = sorted(str(k) for k in golden("hifigan_full")["keys"])
	names = W.weight_norm_names({k: v for k, v in W.hifigan_shapes(W.HIFIGAN_FULL).items() if not k.startswith("cond_layer.")})
	names.update({k: v for k, v in W.hifigan_shapes(W.HIFIGAN_FULL).items() if k.startswith("cond_layer.")})
	assert keys == sorted(names) and len(keys) == 236
	assert sum(math.prod(s) for s in names.values()) == 17844226


def test_small_fixture_config():
	c = W.HIFIGAN_SMALL
	assert c.in_channels == c.cond_channels == W.AR_SMALL.model_dim == 128
	assert [c.upsample_initial_channel // 2 ** (i + 1) for i in range(len(c.upsample_factors))] == [64, 32] and c.hop_length == 8
	assert W.HIFIGAN_FULL.hop_length == 256 and W.HIFIGAN_FULL.frames(250) == 1088
