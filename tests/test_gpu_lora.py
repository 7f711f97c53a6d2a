"""Run-time LoRA adapters on a live autoregressive handle (include/ttk.h: ttk_ar_lora_init / ttk_ar_lora_set; csrc/lora.hip): a handle switched at
run time against a fresh handle created from weights folded on the host by tests/lora_ref.py -- the update kernel's arithmetic restated in numpy --
bit for bit, in every dtype; detaching; a captured token step across switches; the reference's own adapted logits; the refusals; `TTS`."""
import functools

import numpy as np
import pytest
import torch

import lora_ref as LR
from tortoise_tts_amd import _lib, checkpoint as ck, weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ODD = W.ARConfig(layers=2, model_dim=192, heads=3)      # tests/test_gpu_gemv.py: N = 576 pads to 640, K = 192 and 768
CFGS = {"small": W.AR_SMALL, "odd": ODD}
DTYPES = ("f32", "bf16", "f16")
S = 0.75                                                # alpha / rank of the synthetic adapters


@functools.lru_cache(maxsize=None)
def base_sd(cfg_name):
	return W.synth_state_dict(W.ar_score_shapes(CFGS[cfg_name]), 7)      # with the text head: f32 handles also run the teacher-forced losses


def model(sd, cfg_name, dtype, **kw):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	return UnifiedVoice(sd, CFGS[cfg_name], dtype=dtype, device=DEV, max_batch=4, max_ctx=64, **kw)


def outputs(m):
	"""what the tests compare: prefill logits, sampled ids at a fixed seed, the latent pass, and in f32 the three outputs of the teacher-forced forward
	(the dense path over Mat::w and the text head)"""
	cfg = m.cfg
	g = torch.Generator().manual_seed(11)
	text = torch.randint(1, 255, (1, 6), generator=g).to(DEV)
	cond = torch.randn(1, cfg.model_dim, generator=g).to(DEV)
	codes = torch.randint(0, cfg.number_mel_codes - 2, (2, 9), generator=g).to(DEV)
	fw = (cond.expand(2, -1), text.expand(2, -1), torch.tensor([6, 6]), codes, torch.tensor([9 * 1024] * 2))
	with torch.inference_mode():
		out = {"prefill": m._prefill(cond, text, 4).clone()}
		out["ids"] = m.inference_speech(cond, text, do_sample=True, num_return_sequences=4, max_generate_length=12, temperature=0.9, top_k=0)
		out["latent"] = m.forward(*fw, return_latent=True, clip_inputs=False)
		if m.dtype == _lib.TTK_F32:
			out["loss_text"], out["loss_mel"], out["mel_logits"] = m.forward(*fw, return_latent=False, clip_inputs=False)
	torch.cuda.synchronize()
	return {k: v.cpu() for k, v in out.items()}


def bits(t):
	return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(got, want, what=""):
	assert set(got) == set(want)
	for k in want:
		assert got[k].shape == want[k].shape and torch.equal(bits(got[k]), bits(want[k])), (what, k)


def differs(a, b):
	return not torch.equal(a["prefill"], b["prefill"])


@functools.lru_cache(maxsize=None)
def plain_outputs(cfg_name, dtype):
	return outputs(model(base_sd(cfg_name), cfg_name, dtype))


def adapter(cfg_name, rank, seed=3, mods=None):
	cfg = CFGS[cfg_name]
	return LR.synth_adapter(W.ar_shapes(cfg), rank, seed, LR.modules(cfg.layers) if mods is None else mods)


def fresh_outputs(cfg_name, dtype, ad):
	return outputs(model(LR.fold_state_dict(base_sd(cfg_name), ad, S), cfg_name, dtype))


CASES = [(c, r) for c in ("small", "odd") for r in (1, 3, 4)] + [("small", 128), ("small", 256)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg_name,rank", CASES)
def test_switched_handle_equals_fresh_handle_bit_for_bit(cfg_name, rank, dtype):
	ad = adapter(cfg_name, rank)
	m = model(base_sd(cfg_name), cfg_name, dtype, adapters=True)
	m.load_lora("a", ad, scaling=S)
	m.enable_lora("a")
	assert m.active_lora == "a"
	got = outputs(m)
	assert_same(got, fresh_outputs(cfg_name, dtype, ad), (cfg_name, rank, dtype))
	assert differs(got, plain_outputs(cfg_name, dtype))      # and the adapter is not a no-op


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_adapter_and_swap_put_uncovered_matrices_back(dtype):
	first = adapter("small", 4, seed=5, mods=["gpt.h.1.mlp.c_proj", "gpt.h.0.attn.c_attn"])
	second = adapter("small", 3, seed=6, mods=["gpt.h.0.mlp.c_fc", "gpt.h.1.attn.c_proj", "gpt.h.1.mlp.c_proj"])
	m = model(base_sd("small"), "small", dtype, adapters=True)
	m.load_lora("first", first, scaling=S)
	m.load_lora("second", second, scaling=S)
	m.enable_lora("first")
	assert_same(outputs(m), fresh_outputs("small", dtype, first), "first")
	m.enable_lora()                                          # None: the last loaded
	assert m.active_lora == "second"
	assert_same(outputs(m), fresh_outputs("small", dtype, second), "second: c_attn of layer 0 is back at its base")
	m.enable_lora("first")
	assert_same(outputs(m), fresh_outputs("small", dtype, first), "and back")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg_name", ["small", "odd"])
def test_detach_restores_the_base(cfg_name, dtype):
	want = plain_outputs(cfg_name, dtype)
	m = model(base_sd(cfg_name), cfg_name, dtype, adapters=True)
	assert m.active_lora is None
	assert_same(outputs(m), want, "an adapters=True handle that never enabled anything")
	m.load_lora("a", adapter(cfg_name, 4), scaling=S)
	assert_same(outputs(m), want, "loaded, not enabled")
	m.enable_lora()
	assert differs(outputs(m), want)
	m.disable_lora()
	assert m.active_lora is None
	assert_same(outputs(m), want, "enable -> disable")
	m.disable_lora()                                         # nothing attached: nothing to do, nothing changes
	assert_same(outputs(m), want, "disable twice")


def test_captured_step_survives_the_switches():
	"""the operands are rewritten in place, so the HIP graph of the token step (UnifiedVoice._capture_step) captured before a switch computes with the
	adapted weights after it"""
	ad = adapter("small", 4)
	m = model(base_sd("small"), "small", "bf16", adapters=True)
	assert m.use_graph
	m.load_lora("a", ad, scaling=S)
	g = torch.Generator().manual_seed(12)
	text, cond = torch.randint(1, 255, (1, 6), generator=g).to(DEV), torch.randn(1, 128, generator=g).to(DEV)
	kw = dict(do_sample=True, num_return_sequences=4, max_generate_length=20, temperature=0.9, top_k=0)
	with torch.inference_mode():
		a = m.inference_speech(cond, text, **kw).cpu()       # captures the step
		states = dict(m._states)
		m.enable_lora("a")
		b = m.inference_speech(cond, text, **kw).cpu()
		m.disable_lora()
		c = m.inference_speech(cond, text, **kw).cpu()
		assert states and all(m._states.get(k) is v for k, v in states.items())      # the same generation state, hence the same capture, throughout
		want_b = model(LR.fold_state_dict(base_sd("small"), ad, S), "small", "bf16").inference_speech(cond, text, **kw).cpu()
	assert torch.equal(a, c) and torch.equal(b, want_b) and not torch.equal(a, b)


def test_reference_adapter_attached_at_run_time(golden, tmp_path):
	"""tests/golden/lora_small.npz: the reference's own adapter (models/lora.py apply_lora) and the adapted REFERENCE model's logits, f32"""
	g = golden("lora_small")
	t = lambda a: torch.from_numpy(np.asarray(a))
	sd = W.synth_state_dict(W.ar_shapes(W.AR_SMALL), int(g["seed"]))
	lora = {str(k): t(g["lora::" + str(k)]) for k in g["lora_keys"]}
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	m = UnifiedVoice(sd, W.AR_SMALL, dtype="f32", device=DEV, max_batch=4, adapters=True)
	want = t(g["prefill_logits"])
	with torch.inference_mode():
		base_err = (m._prefill(t(g["cond"]), t(g["text"]), int(g["B"])).cpu() - want).abs().max().item()
		m.load_lora("ref", lora, scaling=float(g["alpha"]) / float(g["rank"]))
		m.enable_lora()
		err = (m._prefill(t(g["cond"]), t(g["text"]), int(g["B"])).cpu() - want).abs().max().item()
	print(f"adapted at run time: max abs error {err:.3e} against the reference's logits; un-adapted {base_err:.3e}")
	assert err <= 2e-4 and base_err > 2e-4
	# the same through files: the base uploaded unmerged, the adapter loaded as "lora" with the file's alpha / rank, and enabled
	ck.save_state_dict(sd, tmp_path / "autoregressive.safetensors")
	torch.save({"lora": lora, "config": {"rank": int(g["rank"]), "alpha": int(g["alpha"])}}, tmp_path / "lora.pth")
	ar = ck.load_autoregressive(tmp_path / "autoregressive.safetensors", tmp_path / "lora.pth", dtype="f32", device=DEV, max_batch=4, adapters=True)
	assert ar.active_lora == "lora" and ar._loras["lora"][1] == 2.0
	with torch.inference_mode():
		assert (ar._prefill(t(g["cond"]), t(g["text"]), int(g["B"])).cpu() - want).abs().max().item() <= 2e-4
		ar.disable_lora()
		assert (ar._prefill(t(g["cond"]), t(g["text"]), int(g["B"])).cpu() - want).abs().max().item() == base_err


def test_refusals_leave_the_handle_as_it_was():
	sd = base_sd("small")
	plain = model(sd, "small", "bf16")
	with pytest.raises(_lib.TTKError, match="built without adapters=True"):
		plain.enable_lora()
	with pytest.raises(_lib.TTKError, match="ttk_ar_lora_set: this handle keeps no adapter masters: call ttk_ar_lora_init"):
		plain._lora_set({}, 1.0)
	with pytest.raises(_lib.TTKError, match="ttk_ar_lora_init: run-time adapters are not implemented for dtype TTK_FP8W"):
		model(sd, "small", "fp8w", adapters=True)
	m = model(sd, "small", "bf16", adapters=True)
	ad = adapter("small", 4)
	m.load_lora("a", ad, scaling=S)
	m.enable_lora("a")
	want = outputs(m)
	dev = lambda *shape: torch.full(shape, 0.5, device=DEV)
	c_attn, ok = "gpt.h.0.attn.c_attn", {"gpt.h.1.mlp.c_fc.lora_A": dev(2, 512), "gpt.h.1.mlp.c_fc.lora_B": dev(128, 2)}
	refused = [
		({c_attn + ".lora_A": dev(4, 384)}, r"'gpt\.h\.0\.attn\.c_attn\.lora_A' is given without 'gpt\.h\.0\.attn\.c_attn\.lora_B'"),
		({"mel_head.lora_A": dev(4, 128), "mel_head.lora_B": dev(8194, 4)}, r"'mel_head\.lora_[AB]': run-time adapters attach to gpt\.h\.<layer>"),
		({c_attn + ".lora_A": dev(257, 384), c_attn + ".lora_B": dev(128, 257)}, r"'gpt\.h\.0\.attn\.c_attn\.lora_A' has rank 257: ranks 1\.\.256"),
		({c_attn + ".lora_A": dev(5, 384), c_attn + ".lora_B": dev(128, 4)}, r"'gpt\.h\.0\.attn\.c_attn\.lora_B' is \[128, 4\], expected \[128, 5\]"),
		({c_attn + ".lora_A": dev(4, 383), c_attn + ".lora_B": dev(128, 4)}, r"'gpt\.h\.0\.attn\.c_attn\.lora_A' is \[4, 383\], expected \[rank, 384\]"),
		({c_attn + ".weight": dev(128, 384)}, r"'gpt\.h\.0\.attn\.c_attn\.weight' is not named <module>\.lora_A or <module>\.lora_B"),
	]
	for tensors, msg in refused:
		with pytest.raises(_lib.TTKError, match=msg):
			m._lora_set(ok | tensors, 1.0)                   # the good pair in front: nothing of a refused call may be applied
	with pytest.raises(_lib.TTKError, match="adapter tensors go to the device as f32"):
		m._lora_set({k: v.to(torch.bfloat16) for k, v in ok.items()}, 1.0)
	with pytest.raises(_lib.TTKError, match="scaling inf is not finite"):
		m._lora_set(ok, float("inf"))
	with pytest.raises(_lib.TTKError, match=r"no adapter named 'nope' is loaded \(loaded: \['a'\]\)"):
		m.enable_lora("nope")
	with pytest.raises(ck.CheckpointError, match="rank 257"):
		m.load_lora("big", adapter("small", 257, mods=[c_attn]))
	assert sorted(m._loras) == ["a"] and m.active_lora == "a"
	assert_same(outputs(m), want, "after the refused switches")
	# a switch while a streamed generation is open
	g = torch.Generator().manual_seed(13)
	text, cond = torch.randint(1, 255, (1, 6), generator=g).to(DEV), torch.randn(1, 128, generator=g).to(DEV)
	with torch.inference_mode():
		ids = m.compute_embeddings(cond, text)
		stream = m.get_generator(inputs=ids, max_length=ids.shape[1] + 6, do_sample=True, num_return_sequences=2, temperature=0.9, top_k=0)
		next(stream)
		for call in (m.disable_lora, lambda: m.enable_lora("a")):
			with pytest.raises(_lib.TTKError, match="streamed generation is still open"):
				call()
		stream.close()
	assert m.active_lora == "a"
	assert_same(outputs(m), want, "after the refusal during a stream")


def test_tts_enable_and_disable_lora(golden):
	"""in the style of tests/test_gpu_tts.py, small models: the adapter changes the waveform of a seeded call, detaching gives the first one back"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	tk = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(tk["vocab"])}, merges=[str(m) for m in tk["merges"]], special_tokens=[str(s) for s in tk["special"]])
	sd = dict(ar=W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), df=W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32),
			  voc=W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33))
	mk = lambda **kw: UnifiedVoice(sd["ar"], W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=128, **kw)
	diff, voc = DiffusionTTS(sd["df"], W.DIFF_SMALL, dtype="f32", device=DEV), BigVGAN(sd["voc"], W.VOC_SMALL, dtype="f32", device=DEV)
	tts = TTS(mk(adapters=True), diff, tok, vocoder=voc)
	g = torch.Generator().manual_seed(14)
	voice = {"latent": (torch.randn(1, W.AR_SMALL.model_dim, generator=g).to(DEV), torch.randn(1, 2 * W.DIFF_SMALL.model_channels, generator=g).to(DEV))}
	text = "Hello there, Mr. Fox."
	kw = dict(max_ar_steps=10, max_diffusion_steps=3, candidates=2, seed=1234)
	base, sr = tts.inference(text, voice, **kw)
	tts.load_lora("v", adapter("small", 4), scaling=S)
	assert tts.hot.autoregressive.active_lora is None
	tts.enable_lora()
	adapted, _ = tts.inference(text, voice, **kw)
	assert tts.hot.autoregressive.active_lora == "v" and sr == 24000
	assert adapted.shape[:2] == (1, 1) and torch.isfinite(adapted).all()
	assert adapted.shape != base.shape or not torch.equal(adapted, base)
	tts.disable_lora()
	again, _ = tts.inference(text, voice, **kw)
	assert torch.equal(bits(again), bits(base))
	tts.enable_lora("v")
	assert torch.equal(bits(tts.inference(text, voice, **kw)[0]), bits(adapted))
	tts.enable_lora(False)
	assert tts.hot.autoregressive.active_lora is None
	with pytest.raises(NotImplementedError, match="built without adapters=True"):
		TTS(mk(), diff, tok, vocoder=voc).enable_lora()
