"""The UnivNet CPU oracle (tests/univnet_oracle.py) against the reference's own generator (tests/golden/univnet_*.npz, written by
tools/make_golden_univnet.py): predicted kernels and biases, convt_pre, the first location-variable convolution and the audio.  CPU only."""
import math

import numpy as np
import pytest
import torch

import univnet_oracle as UO
from tortoise_tts_amd import weights as W

CFGS = {"univnet_small": W.UNIVNET_SMALL, "univnet_full": W.UNIVNET_FULL}


def maxerr(a, b):
	"""max |a - b| in units of max(1, max |b|): 1e-5 is then f32 rounding, also for the predicted biases (|b| up to ~30 with the synthetic weights)"""
	b = torch.as_tensor(np.asarray(b)).double()
	return (torch.as_tensor(np.asarray(a)).double() - b).abs().max().item() / max(1.0, b.abs().max().item())


@pytest.mark.parametrize("name", sorted(CFGS))
def test_oracle_equals_reference(golden, name):
	g, cfg = golden(name), CFGS[name]
	sd = W.synth_state_dict(W.univnet_shapes(cfg), int(g["seed"]))
	o = UO.UnivNetOracle(sd, cfg, torch.float64)      # f64: what remains is the reference's own f32 rounding
	mel, z = torch.from_numpy(g["mel"]), torch.from_numpy(g["z"])
	with torch.inference_mode():
		melp = torch.cat([mel, torch.full((mel.shape[0], mel.shape[1], 10), UO.MEL_PAD_VALUE)], dim=2)
		fwd = o.forward(melp, z)
		tr = dict(o.trace)
		audio = o.inference(mel, z)
	frames = list(g["kernels_frames"])
	assert maxerr(tr["kernels"][..., frames], g["kernels"]) < 1e-5
	assert maxerr(tr["bias"], g["bias"]) < 1e-5
	assert maxerr(tr["convt_pre"], g["convt_pre"]) < 1e-5
	assert maxerr(tr["lvc0"], g["lvc0"]) < 1e-5
	# forward includes the hops of the 10 padding frames (inference trims them); there the reference's own f32 rounding reaches 2.4e-5
	assert fwd.shape == g["forward"].shape and maxerr(fwd, g["forward"]) < 5e-5
	assert audio.shape == g["audio"].shape == (mel.shape[0], 1, mel.shape[2] * cfg.hop_length) and maxerr(audio, g["audio"]) < 1e-5


def test_key_list_is_the_reference_state_dict(golden):
	keys = sorted(str(k) for k in golden("univnet_full")["keys"])
	assert keys == sorted(W.weight_norm_names(W.univnet_shapes(W.UNIVNET_FULL)))


def test_published_config_parameter_count():
	assert sum(math.prod(s) for s in W.weight_norm_names(W.univnet_shapes(W.UNIVNET_FULL)).values()) == 14865506


def test_small_fixture_config():
	assert (W.UNIVNET_SMALL.channel_size, W.UNIVNET_SMALL.strides, W.UNIVNET_SMALL.dilations, W.UNIVNET_SMALL.hop_length) == (16, (4, 4), (1, 3), 16)
	assert W.UNIVNET_FULL.cond_hops() == [8, 64, 256] and W.UNIVNET_SMALL.cond_hops() == [4, 16]
