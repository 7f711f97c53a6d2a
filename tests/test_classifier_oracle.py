"""The TorToiSe detector off the GPU: the plain-torch restatement (tests/classifier_oracle.py) against the reference's own class
(tests/golden/classifier_*.npz, written by tools/make_golden_classifier.py), the weight table, the configuration refusals, the checkpoint loader and
the C ABI's declarations.  No GPU."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import classifier_oracle as CO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, tag) for n, (_, tags) in CO.CFGS.items() for tag in tags]
NEW_SYMBOLS = ("ttk_cls_create", "ttk_cls_destroy", "ttk_cls_forward", "ttk_cls_forward_taps", "ttk_cls_conv5_rows", "ttk_cls_stats_rows", "ttk_cls_gn_stats")
_cache = {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def setup(golden, name):
	if name not in _cache:
		g = golden(name)
		cfg = CO.CFGS[name][0]
		assert int(g["seed"]) == CO.SEEDS[name] and [str(x) for x in g["tags"]] == list(CO.CFGS[name][1])
		sd = W.synth_state_dict(W.classifier_shapes(cfg), int(g["seed"]))
		_cache[name] = (g, sd, CO.ClassifierOracle(sd, cfg, torch.float32))
	return _cache[name]


def audio_of(g, tag):
	B, T = (int(v) for v in tag.split("x"))
	x = CO.fixture_audio(B, T, int(g[f"input_seed_{tag}"]))
	if f"audio_{tag}" in g:
		assert torch.equal(x, t(g[f"audio_{tag}"]))
	return x


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_reproduces_the_reference(golden, name, tag):
	"""every stored array within 4 x the reference's own max |f32 - float64| for that array"""
	g, _, o = setup(golden, name)
	cfg = CO.CFGS[name][0]
	B, T = (int(v) for v in tag.split("x"))
	with torch.inference_mode():
		emb, logits, acts = o.forward(audio_of(g, tag))
	lengths = cfg.stage_lengths(T)
	assert lengths == [T] + [-(-T // 4 ** (l + 1)) for l in range(cfg.depth)]      # ceil(L / 4) per stage composes to ceil(T / 4^l)
	assert list(acts) == CO.activation_names(cfg)
	assert [a.shape[2] for a in acts.values()] == lengths + [lengths[-1]]
	assert emb.shape == (B, cfg.embedding_dim) and logits.shape == (B, cfg.classes)
	got = dict(acts, emb=emb, logits=logits)
	for k, a in got.items():
		step = int(g[f"step_{k}_{tag}"]) if k in acts else 1
		ref, bound = t(g[f"{k}_{tag}"]), 4.0 * float(g[f"err_{k}_{tag}"])
		if k in acts:
			assert step == CO.time_step(a.shape)
			a = a[..., ::step]
		e = (a.double() - ref.double()).abs().max().item()
		print(f"{name} {tag} {k}: max |restatement - reference| {e:.3e} (bound {bound:.3e})")
		assert a.shape == ref.shape and e <= bound
	assert emb.std().item() > 0.1


def test_stage_lengths_of_the_issue():
	assert W.CLASSIFIER_FULL.stage_lengths(4099) == [4099, 1025, 257, 65, 17, 5]
	assert W.CLASSIFIER_FULL.stage_lengths(240000) == [240000, 60000, 15000, 3750, 938, 235]
	assert W.CLASSIFIER_FULL.stage_lengths(1) == [1] * 6


@pytest.mark.parametrize("name", sorted(CO.CFGS))
def test_shapes_cover_exactly_the_reference_keys_and_the_logits_differ(golden, name):
	g, sd, _ = setup(golden, name)
	cfg, tags = CO.CFGS[name]
	assert sorted(W.classifier_shapes(cfg).keys()) == [str(k) for k in g["keys"]]
	rows = [tuple(np.round(g[f"logits_{tag}"][0], 4)) for tag in tags]
	assert len(set(rows)) == len(rows)
	for tag in tags:
		assert g[f"emb_{tag}"].std() > 0.1 and g[f"emb_f64_{tag}"].dtype == np.float64


def test_full_configuration_is_the_published_one():
	shapes = W.classifier_shapes(W.CLASSIFIER_FULL)
	assert len(shapes) == 122 and W.n_params(shapes) == 15224002
	c = W.CLASSIFIER_SMALL
	assert (c.embedding_dim, c.depth, c.resnet_blocks, c.attn_blocks, c.num_attn_heads, c.base_channels, c.kernel_size) == (128, 3, 1, 2, 1, 32, 5)


def test_unsupported_configurations_are_refused_by_name():
	from tortoise_tts_amd.classifier import check_config
	check_config(W.CLASSIFIER_FULL)
	check_config(W.CLASSIFIER_SMALL)
	for change, word in ((dict(spec_dim=80), "spec_dim"), (dict(kernel_size=3), "kernel_size"), (dict(downsample_factor=2), "downsample_factor"),
						 (dict(base_channels=128), "base_channels"), (dict(depth=0), "depth"), (dict(depth=7), "depth"), (dict(num_attn_heads=2), "num_attn_heads"),
						 (dict(num_attn_heads=16), "num_attn_heads"), (dict(classes=0), "classes"), (dict(classes=17), "classes")):
		with pytest.raises(NotImplementedError, match="AudioMiniEncoderWithClassifierHead: " + word):
			check_config(dataclasses.replace(W.CLASSIFIER_FULL, **change))


def test_forward_with_labels_is_refused_before_anything_runs():
	"""host only: the refusal comes before the handle is touched"""
	from tortoise_tts_amd.classifier import AudioMiniEncoderWithClassifierHead
	m = object.__new__(AudioMiniEncoderWithClassifierHead)
	with pytest.raises(NotImplementedError, match="training loss"):
		m.forward(torch.zeros(1, 1, 8), torch.zeros(1, dtype=torch.int64))
	with pytest.raises(NotImplementedError, match="training loss"):
		m(torch.zeros(1, 1, 8), labels=torch.zeros(1, dtype=torch.int64))


def test_load_classifier_state_round_trips_a_saved_state_dict(tmp_path):
	from tortoise_tts_amd.checkpoint import CheckpointError, load_classifier_state
	cfg = W.CLASSIFIER_SMALL
	sd = W.synth_state_dict(W.classifier_shapes(cfg), 7)
	path = tmp_path / "classifier.pth"
	torch.save(sd, path)
	got, got_cfg = load_classifier_state(path, cfg=cfg)
	assert got_cfg == cfg and sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
	with pytest.raises(CheckpointError, match="enc.res"):      # the small file does not fit the published configuration
		load_classifier_state(path)
	short = {k: v for k, v in sd.items() if k != "head.bias"}
	torch.save(short, path)
	with pytest.raises(CheckpointError, match="head.bias"):
		load_classifier_state(path, cfg=cfg)


def test_classify_audio_clip_without_a_classifier_is_refused():
	from tortoise_tts_amd.tts import TTS
	tts = object.__new__(TTS)
	tts.classifier = None
	with pytest.raises(ValueError, match="classifier="):
		tts.classify_audio_clip(torch.zeros(1, 100))


def test_new_symbols_are_declared_listed_and_exported():
	import tortoise_tts_amd
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
	assert "ttk_cls_config" in header and len(_lib.SYMBOLS["ttk_cls_conv5_rows"][1]) == 14 and len(_lib.SYMBOLS["ttk_cls_forward"][1]) == 7
	lib = ctypes.CDLL(_lib.build())
	assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
	from tortoise_tts_amd.classifier import ClassifierConfigC
	assert ctypes.sizeof(ClassifierConfigC) == 11 * 4      # ttk_cls_config: 11 ints
	for name in ("AudioMiniEncoderWithClassifierHead", "ClassifierConfig", "load_classifier"):
		assert name in tortoise_tts_amd.__all__ and getattr(tortoise_tts_amd, name) is not None
