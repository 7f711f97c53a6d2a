"""The RandomLatentConverter off the GPU: the plain-torch restatement (tests/rlg_oracle.py) on the folded operands against the reference's own class
(tests/golden/rlg_*.npz, written by tools/make_golden_rlg.py), the synthetic weights, the checkpoint loader and the C ABI's declarations.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import rlg_oracle as RO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, tag) for n, tags in RO.CASES.items() for tag in tags]
NEW_SYMBOLS = ("ttk_linear_rows", "ttk_rlg_create", "ttk_rlg_destroy", "ttk_rlg_forward")


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_on_folded_operands_reproduces_the_reference(golden, name, tag):
	g = golden(name)
	assert [str(t) for t in g["tags"]] == list(RO.CASES[name])
	channels, B, folded, noise, y, y64 = RO.case(g, tag)
	assert noise.shape == y.shape == y64.shape == (B, channels) and y.dtype == torch.float32 and y64.dtype == torch.float64
	torch.manual_seed(int(g[f"noise_seed_{tag}"]))
	assert torch.equal(torch.randn(B, channels), noise)      # the stored noise is the reference's own draw
	with torch.inference_mode():
		got = RO.forward(folded, noise)
		got64 = RO.forward(folded, noise.double())
	rel = (got - y).abs().max().item() / y.abs().max().item()
	print(f"{name} {tag}: max|restatement - y| / max|y| = {rel:.2e}; max|y - y64| = {(y.double() - y64).abs().max().item():.2e}")
	assert rel <= 1e-6
	# the float64 run of the reference multiplies the f32 weight by its scale in float64, the restatement widens the folded f32 product: both are
	# within f32 rounding of the operands of each other, far inside the deviation of any f32 run
	assert (got64 - y64).abs().max().item() <= 1e-5 * y64.abs().max().item()
	# layers do something: no layer passes its bias through, and the latent is neither constant nor tiny
	assert y.std().item() > 0.1 and (y - folded[f"layers.{W.RLG_LAYERS - 1}.bias"]).abs().max().item() > 0.1


def test_rlg_state_dict_is_deterministic_and_at_the_reference_scales():
	a, b, c = W.rlg_state_dict(64, 5), W.rlg_state_dict(64, 5), W.rlg_state_dict(64, 6)
	assert list(a) == list(W.rlg_shapes(64)) and len(a) == 12
	assert all(torch.equal(a[k], b[k]) for k in a) and not any(torch.equal(a[k], c[k]) for k in a)
	assert all(tuple(a[k].shape) == W.rlg_shapes(64)[k] and a[k].dtype == torch.float32 for k in a)
	big = W.rlg_state_dict(256, 1)
	for i in range(5):
		assert 9.5 < big[f"layers.{i}.weight"].std().item() < 10.5 and 0.8 < big[f"layers.{i}.bias"].std().item() < 1.2
	assert 0.9 / 16 < big["layers.5.weight"].std().item() < 1.1 / 16 and 0.03 < big["layers.5.bias"].std().item() < 0.07
	assert not torch.equal(big["layers.0.weight"], big["layers.1.weight"])


def test_fold_uses_the_references_expressions_and_refuses_bad_state_dicts():
	import math
	from tortoise_tts_amd.random_latent import fold_equal_linear
	sd = W.rlg_state_dict(68, 3)
	f = fold_equal_linear(sd)
	for i in range(5):
		assert torch.equal(f[f"layers.{i}.weight"], sd[f"layers.{i}.weight"] * ((1 / math.sqrt(68)) * .1))
		assert torch.equal(f[f"layers.{i}.bias"], sd[f"layers.{i}.bias"] * .1)
	assert torch.equal(f["layers.5.weight"], sd["layers.5.weight"]) and torch.equal(f["layers.5.bias"], sd["layers.5.bias"])
	missing = {k: v for k, v in sd.items() if k != "layers.3.bias"}
	with pytest.raises(_lib.TTKError, match="layers.3.bias"):
		fold_equal_linear(missing)
	skew = dict(sd)
	skew["layers.2.weight"] = torch.zeros(68, 64)
	with pytest.raises(_lib.TTKError, match="layers.2.weight"):
		fold_equal_linear(skew)
	with pytest.raises(_lib.TTKError, match="layers.0.weight"):
		fold_equal_linear({})


def test_loader_round_trips_a_saved_file_and_refuses_a_missing_layer(tmp_path):
	from tortoise_tts_amd.checkpoint import CheckpointError, load_rlg_state
	sd = W.rlg_state_dict(132, 9)
	path = tmp_path / "rlg_auto.pth"
	torch.save(sd, path)
	got, channels = load_rlg_state(path)
	assert channels == 132 and sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
	torch.save({"model": sd}, path)
	assert load_rlg_state(path, state_dict_key="model")[1] == 132
	short = {k: v for k, v in sd.items() if not k.startswith("layers.4.")}
	torch.save(short, path)
	with pytest.raises(CheckpointError, match="layers.4.weight"):
		load_rlg_state(path)
	torch.save({k: v for k, v in sd.items() if not k.startswith("layers.0.")}, path)
	with pytest.raises(CheckpointError, match="layers.0.weight"):
		load_rlg_state(path)


def test_new_symbols_are_declared_listed_and_exported():
	import tortoise_tts_amd
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
	assert "ttk_rlg_config" in header and len(_lib.SYMBOLS["ttk_linear_rows"][1]) == 13
	lib = ctypes.CDLL(_lib.build())
	assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
	from tortoise_tts_amd.random_latent import RLGConfigC
	assert ctypes.sizeof(RLGConfigC) == 3 * 4 + 2 * 4      # ttk_rlg_config: 3 ints, 2 floats
	assert "RandomLatentConverter" in tortoise_tts_amd.__all__ and "load_random_latent_generator" in tortoise_tts_amd.__all__
	assert tortoise_tts_amd.RandomLatentConverter.__name__ == "RandomLatentConverter" and callable(tortoise_tts_amd.load_random_latent_generator)
