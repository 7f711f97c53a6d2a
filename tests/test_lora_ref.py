"""Run-time LoRA adapters, host side: the numpy statement of the update kernel's arithmetic (tests/lora_ref.py) against the reference's own
effective weights, and the argument checks of `UnifiedVoice.load_lora` / `enable_lora` that need no device.  The device side is
tests/test_gpu_lora.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lora_ref as LR
from tortoise_tts_amd import _lib, checkpoint as ck, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ttk_ar_lora_init", "ttk_ar_lora_set")


def _golden_adapter(golden):
	g = golden("lora_small")
	sd = W.synth_state_dict(W.ar_shapes(W.AR_SMALL), int(g["seed"]))
	lora = {str(k): torch.from_numpy(np.asarray(g["lora::" + str(k)])) for k in g["lora_keys"]}
	return g, sd, lora, float(g["alpha"]) / float(g["rank"])


def test_fold_equals_the_reference_effective_weights(golden):
	g, sd, lora, s = _golden_adapter(golden)
	eff = {k[5:]: g[k] for k in g if k.startswith("eff::")}
	assert set(eff) == {m + ".weight" for m in LR.modules(W.AR_SMALL.layers)}
	folded = LR.fold_state_dict(sd, lora, s)
	for k, v in eff.items():
		err = float(np.abs(folded[k].numpy() - v).max())
		assert err <= 1e-6, (k, err)
		assert float(np.abs(sd[k].numpy() - v).max()) > 1e-3, k      # the adapter matters: the base weight is far away
	assert all(torch.equal(folded[k], sd[k]) for k in sd if k not in eff)


def test_fold_is_the_stated_loop_and_zero_lora_b_returns_the_base():
	rng = np.random.default_rng(5)
	W0, A, B = (rng.standard_normal(s).astype(np.float32) for s in ((3, 5), (7, 5), (3, 7)))
	s = np.float32(0.3)
	want = np.empty_like(W0)
	for k in range(3):
		for n in range(5):
			acc = np.float32(0)
			for r in range(7):
				acc = np.float32(acc + np.float32(B[k, r] * A[r, n]))
			want[k, n] = np.float32(W0[k, n] + np.float32(acc * s))
	got = LR.fold(W0, A, B, s)
	assert got.dtype == np.float32 and np.array_equal(got, want)
	f64 = W0.astype(np.float64) + (B.astype(np.float64) @ A.astype(np.float64)) * float(s)
	assert np.abs(got - f64).max() < 1e-5
	assert np.array_equal(LR.fold(W0, A, np.zeros_like(B), s), W0)
	ad = LR.synth_adapter(W.ar_shapes(W.AR_SMALL), 3, 1, ["gpt.h.0.attn.c_attn"])
	assert set(ad) == {"gpt.h.0.attn.c_attn" + LR.PARAM + "lora_A", "gpt.h.0.attn.c_attn" + LR.PARAM + "lora_B"}
	assert ad["gpt.h.0.attn.c_attn" + LR.PARAM + "lora_B"].shape == (128, 3) and float(ad["gpt.h.0.attn.c_attn" + LR.PARAM + "lora_B"].abs().min()) > 0


def test_normalize_lora_reads_the_keys_materialize_lora_reads(golden):
	g, sd, lora, s = _golden_adapter(golden)
	pairs = ck.normalize_lora(lora)
	assert set(pairs) == set(LR.modules(W.AR_SMALL.layers))
	m = "gpt.h.1.mlp.c_proj"
	assert pairs[m][0] is lora[m + LR.PARAM + "lora_A"] and pairs[m][1] is lora[m + LR.PARAM + "lora_B"]
	# plain names, and a parametrised state_dict with its base weights (`.weight` or `...original`) beside the adapter: the base is passed over
	plain = {m + ".lora_A": lora[m + LR.PARAM + "lora_A"], m + ".lora_B": lora[m + LR.PARAM + "lora_B"], m + ".weight": sd[m + ".weight"],
			 "gpt.h.0.mlp.c_fc.parametrizations.weight.original": sd["gpt.h.0.mlp.c_fc.weight"]}
	assert set(ck.normalize_lora(plain)) == {m}
	with pytest.raises(ck.CheckpointError, match=r"'gpt\.h\.0\.attn\.c_attn': lora_A / lora_B are not both present"):
		ck.normalize_lora({"gpt.h.0.attn.c_attn" + LR.PARAM + "lora_A": torch.zeros(2, 384)})
	stacked = dict(lora) | {m + ".parametrizations.weight.1.lora_A": torch.zeros(2, 128), m + ".parametrizations.weight.1.lora_B": torch.zeros(512, 2)}
	with pytest.raises(ck.CheckpointError, match=r"'gpt\.h\.1\.mlp\.c_proj': 2 stacked adapters"):
		ck.normalize_lora(stacked)
	with pytest.raises(ck.CheckpointError, match="no 'lora_' tensors"):
		ck.normalize_lora({m + ".weight": sd[m + ".weight"]})
	with pytest.raises(ck.CheckpointError, match="floating-point"):
		ck.normalize_lora({m + ".lora_A": torch.zeros(2, 128, dtype=torch.int32), m + ".lora_B": torch.zeros(512, 2)})


def _bare_model(adapters=True):
	"""a UnifiedVoice without a device handle, in the manner of tests/test_beam_ref.py: every check below is raised before the first device call"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	m = object.__new__(UnifiedVoice)
	m.cfg, m.max_batch, m.max_ctx, m._streaming, m.hf_exact_top_p = W.AR_SMALL, 4, 128, False, False
	m.device = torch.device("cuda:0")
	m._adapters, m._loras, m.active_lora = adapters, {}, None
	return m


def test_load_and_enable_checks_need_no_device(golden, tmp_path):
	g, sd, lora, s = _golden_adapter(golden)
	shapes = W.ar_shapes(W.AR_SMALL)
	m = _bare_model()
	c_attn = "gpt.h.0.attn.c_attn"
	with pytest.raises(ck.CheckpointError, match=r"'mel_head': adapters attach at run time to gpt\.h\.<layer>"):
		m.load_lora("a", {"mel_head.lora_A": torch.zeros(2, 128), "mel_head.lora_B": torch.zeros(8194, 2)})
	with pytest.raises(ck.CheckpointError, match=r"'gpt\.h\.2\.attn\.c_attn': adapters attach"):      # a layer the model does not have
		m.load_lora("a", {"gpt.h.2.attn.c_attn.lora_A": torch.zeros(2, 384), "gpt.h.2.attn.c_attn.lora_B": torch.zeros(128, 2)})
	with pytest.raises(ck.CheckpointError, match=r"'gpt\.h\.0\.attn\.c_attn': rank 257 is outside 1\.\.256"):
		m.load_lora("a", LR.synth_adapter(shapes, 257, 1, [c_attn]))
	with pytest.raises(ck.CheckpointError, match=r"lora shapes \(128, 4\) x \(4, 383\) do not match weight \(128, 384\)"):
		m.load_lora("a", {c_attn + ".lora_A": torch.zeros(4, 383), c_attn + ".lora_B": torch.zeros(128, 4)})
	with pytest.raises(ck.CheckpointError, match="not both present"):
		m.load_lora("a", {c_attn + ".lora_B": torch.zeros(128, 4)})
	with pytest.raises(ck.CheckpointError, match="stacked adapters"):
		m.load_lora("a", dict(lora) | {c_attn + ".parametrizations.weight.1.lora_A": torch.zeros(2, 384), c_attn + ".parametrizations.weight.1.lora_B": torch.zeros(128, 2)})
	torch.save({"lora": {c_attn + LR.PARAM + "lora_A": torch.zeros(2, 384)}, "config": {"rank": 2, "alpha": 4}}, tmp_path / "half.pth")
	with pytest.raises(ck.CheckpointError, match="not both present"):
		m.load_lora("a", tmp_path / "half.pth")
	assert m._loras == {} and m.active_lora is None
	with pytest.raises(_lib.TTKError, match="no adapter is loaded"):
		m.enable_lora()
	with pytest.raises(_lib.TTKError, match=r"no adapter named 'b' is loaded \(loaded: \[\]\)"):
		m.enable_lora("b")
	m._streaming = True
	with pytest.raises(_lib.TTKError, match="streamed generation is still open"):
		m.enable_lora("b")
	with pytest.raises(_lib.TTKError, match="streamed generation is still open"):
		m.disable_lora()
	plain = _bare_model(adapters=False)
	for call in (lambda: plain.load_lora("a", lora), lambda: plain.enable_lora(), lambda: plain.disable_lora()):
		with pytest.raises(_lib.TTKError, match="built without adapters=True"):
			call()


def test_tts_forwards_and_refuses_without_adapters():
	from tortoise_tts_amd.tts import TTS
	calls = []

	class AR:
		_adapters = True
		device = torch.device("cuda:0")
		def load_lora(self, name, path, scaling=None): calls.append(("load", name, path, scaling))
		def enable_lora(self, name=None): calls.append(("enable", name))
		def disable_lora(self): calls.append(("disable",))
	tts = TTS(AR(), None, None)
	tts.load_lora("v", "file.pth", scaling=0.5)
	tts.enable_lora()
	tts.enable_lora("v")
	tts.enable_lora(False)
	tts.disable_lora()
	assert calls == [("load", "v", "file.pth", 0.5), ("enable", None), ("enable", "v"), ("disable",), ("disable",)]
	AR._adapters = False
	for call in (lambda: tts.load_lora("v", "file.pth"), tts.enable_lora, tts.disable_lora):
		with pytest.raises(NotImplementedError, match="built without adapters=True"):
			call()


def test_new_symbols_are_declared_listed_exported_and_public():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
	assert len(_lib.SYMBOLS["ttk_ar_lora_init"][1]) == 3 and len(_lib.SYMBOLS["ttk_ar_lora_set"][1]) == 5
	_lib.build()
	lib = ctypes.CDLL(_lib.LIB_PATH)
	assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
	import tortoise_tts_amd
	for name in ("read_lora", "normalize_lora"):
		assert name in tortoise_tts_amd.__all__ and getattr(tortoise_tts_amd, name) is getattr(ck, name)
