"""`UnifiedVoice.forward(..., return_latent=False)` -- the teacher-forced losses and logits (ttk_ar_score) -- against the reference's own forward
(tests/golden/ar_score_*.npz, tools/make_golden_ar_score.py).

f32: the project's bounds for this dense pass (test_gpu_parity.py: 1e-4 on the small model's logits, 5e-4 at full size); a cross-entropy row moves by at most twice
the largest logit change of its row, hence 2e-4 / 1e-3 on the rows and on their means.
bf16 / f16: the logits within the existing relative L2 bounds (3e-2, f16 an eighth of it); the rows within 2 * max_c |logit - logit_ref| of the SAME row plus the
kernel's own bound (tests/test_gpu_xent.py) -- an inequality that holds for any two logit rows, so no number is invented for the 16-bit losses.
Every mode, fp8w included: the rows agree, within the kernel bound, with the float64 cross-entropy of the logits the same call returned.

Measured on MI355X (text and mel head; DESIGN.md's parity table has the same figures):
  f32   logits max-abs: a 2.9e-6, b 2.4e-6, c62 2.2e-6, c63 2.2e-6, peaked 9.5e-5 (|logit| to 35), full 8.1e-6; rows <= 3.8e-6 (peaked 3.8e-5, full 5.7e-6); losses <= 1.9e-6
  bf16  a: logits rel L2 3.7e-3 / 3.6e-3, rows max 6.8e-3 / 7.6e-3, losses 1.3e-3 / 1.9e-4      peaked: 1.2e-2 / 9.3e-3, rows 5.8e-2 / 2.1e-1, losses 2.0e-3 / 6.4e-3
  f16   a: logits rel L2 4.7e-4 / 4.4e-4, rows max 8.9e-4 / 1.2e-3, losses 1.7e-4 / 9.3e-5      peaked: 1.4e-3 / 1.1e-3, rows 2.4e-3 / 2.5e-2, losses 2.0e-4 / 1.2e-3
  rows against float64 of the returned logits: at most 0.15 of the kernel bound in every mode (f32, bf16, f16, fp8w)
"""
import gc

import numpy as np
import pytest
import torch

from tortoise_tts_amd import _lib, weights as W
from tortoise_tts_amd.autoregressive import UnifiedVoice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_CASES = ("a", "b", "c62", "c63")
_models = {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def state_dict(which, scoring=True):
	cfg, seed = (W.AR_FULL, 32) if which == "full" else (W.AR_SMALL, 31)
	sd = W.synth_state_dict((W.ar_score_shapes if scoring else W.ar_shapes)(cfg), seed)
	return (W.stress_ar(sd, cfg, "peaked") if which == "peaked" else sd), cfg


@pytest.fixture(scope="module", autouse=True)
def release_handles():
	"""the handles this module keeps are gone when it ends: each holds device memory and one of the decode attention's eight position slots"""
	yield
	_models.clear()
	gc.collect()


def model_for(which, dtype, scoring=True):
	"""one handle per (weights, dtype), a few at a time"""
	key = (which, dtype, scoring)
	if key not in _models:
		if which == "full" or len(_models) >= 4:
			_models.clear()
		sd, cfg = state_dict(which, scoring)
		_models[key] = UnifiedVoice(sd, cfg, dtype=dtype, device=DEV, max_batch=4, max_ctx=96)
	return _models[key]


def inputs(g, case):
	"""the clipped / padded inputs the reference's forward ran on: its targets without the two stop positions"""
	return t(g[f"{case}_cond"]).to(DEV), t(g[f"{case}_text_targets"])[:, :-2].contiguous().to(DEV), t(g[f"{case}_mel_targets"])[:, :-2].contiguous().to(DEV)


def kernel_bound(logits_bct):
	return 1e-5 + 8 * 2.0 ** -24 * logits_bct.double().abs().amax(dim=1).clamp(min=1.0)


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def relerr(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def score(model, g, case):
	cond, text, codes = inputs(g, case)
	r = model._score(cond, text, codes, text_logits=True)
	torch.cuda.synchronize()
	return {k: v.cpu() for k, v in r.items()}


def ref_mel_logits(g, case, got):
	"""(got, want) on the classes the fixture stores"""
	if f"{case}_mel_logits" in g:
		return got, t(g[f"{case}_mel_logits"])
	return got[:, t(g[f"{case}_logit_cols"])], t(g[f"{case}_mel_logits_cols"])


def check_rows_against_own_logits(r, g, case, tag):
	"""the rows are the float64 cross-entropy of the logits this very call returned, within the kernel bound"""
	worst = 0.0
	for name in ("text", "mel"):
		logits, targets = r[f"{name}_logits"], t(g[f"{case}_{name}_targets"])
		x64 = logits.double()
		want = torch.logsumexp(x64, dim=1) - x64.gather(1, targets[:, None, :])[:, 0]
		ratio = ((r[f"nll_{name}"].double() - want).abs() / kernel_bound(logits)).max().item()
		worst = max(worst, ratio)
		assert ratio <= 1.0, (tag, case, name, ratio)
		assert abs(float(r["loss"][0 if name == "text" else 1]) - float(want.mean())) <= float(kernel_bound(logits).max())
	print(f"{tag} {case}: rows against float64 of the returned logits at {worst:.3f} of the kernel bound")


# ------------------------------------------------------------------------------------------------ f32 parity
@pytest.mark.parametrize("case", SMALL_CASES + ("peaked",))
def test_f32_small_against_the_reference(golden, case):
	g = golden("ar_score_peaked" if case == "peaked" else "ar_score_small")
	r = score(model_for("peaked" if case == "peaked" else "small", "f32"), g, case)
	got_mel, want_mel = ref_mel_logits(g, case, r["mel_logits"])
	e_logits = max(maxerr(r["text_logits"], g[f"{case}_text_logits"]), maxerr(got_mel, want_mel))
	e_rows = max(maxerr(r["nll_text"], g[f"{case}_nll_text"]), maxerr(r["nll_mel"], g[f"{case}_nll_mel"]))
	e_loss = max(abs(float(r["loss"][0]) - float(g[f"{case}_loss_text"])), abs(float(r["loss"][1]) - float(g[f"{case}_loss_mel"])))
	print(f"f32 {case}: logits {e_logits:.2e}, nll rows {e_rows:.2e}, losses {e_loss:.2e}")
	assert r["mel_logits"].shape == (r["nll_mel"].shape[0], 8194, r["nll_mel"].shape[1]) and r["nll_mel"].shape == g[f"{case}_mel_targets"].shape
	assert e_logits < 1e-4
	assert e_rows < 2e-4 and e_loss < 2e-4
	check_rows_against_own_logits(r, g, case, "f32")


def test_f32_full_size_against_the_reference(golden):
	g = golden("ar_score_full")
	r = score(model_for("full", "f32"), g, "full")
	_models.clear()
	got_mel, want_mel = ref_mel_logits(g, "full", r["mel_logits"])
	e_logits = max(maxerr(r["text_logits"], g["full_text_logits"]), maxerr(got_mel, want_mel))
	e_rows = max(maxerr(r["nll_text"], g["full_nll_text"]), maxerr(r["nll_mel"], g["full_nll_mel"]))
	e_loss = max(abs(float(r["loss"][0]) - float(g["full_loss_text"])), abs(float(r["loss"][1]) - float(g["full_loss_mel"])))
	print(f"f32 full: logits {e_logits:.2e}, nll rows {e_rows:.2e}, losses {e_loss:.2e}")
	assert e_logits < 5e-4
	assert e_rows < 1e-3 and e_loss < 1e-3
	check_rows_against_own_logits(r, g, "full", "f32")


# ------------------------------------------------------------------------------------------------ 16-bit parity
@pytest.mark.parametrize("case", ("a", "peaked"))
@pytest.mark.parametrize("dtype,logit_bound", [("bf16", 3e-2), ("f16", 3e-2 / 8)])
def test_16bit_against_the_reference(golden, dtype, logit_bound, case):
	g = golden("ar_score_peaked" if case == "peaked" else "ar_score_small")
	r = score(model_for("peaked" if case == "peaked" else "small", dtype), g, case)
	devs = {}
	for name in ("text", "mel"):
		got, want = r[f"{name}_logits"], t(g[f"{case}_{name}_logits"])
		rel = relerr(got, want)
		row_move = (got.double() - want.double()).abs().amax(dim=1)                       # [B, T]: max_c |logit - logit_ref| of each row
		row_err = (r[f"nll_{name}"].double() - t(g[f"{case}_nll_{name}"]).double()).abs()
		loss_err = abs(float(r["loss"][0 if name == "text" else 1]) - float(g[f"{case}_loss_{name}"]))
		devs[name] = (rel, row_err.max().item(), loss_err)
		assert rel < logit_bound, (dtype, case, name, rel)
		assert (row_err <= 2 * row_move + kernel_bound(want)).all(), (dtype, case, name, (row_err - 2 * row_move).max().item())
		assert loss_err <= float((2 * row_move).mean()) + float(kernel_bound(want).max())
	print(f"{dtype} {case}: " + ", ".join(f"{n}: logits rel L2 {d[0]:.2e}, nll rows max {d[1]:.2e}, loss {d[2]:.2e}" for n, d in devs.items()))
	check_rows_against_own_logits(r, g, case, dtype)


# ------------------------------------------------------------------------------------------------ every arithmetic mode: the kernel inside the pipeline
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "fp8w"])
def test_rows_are_the_cross_entropy_of_the_returned_logits(golden, dtype):
	g = golden("ar_score_small")
	m = model_for("small", dtype)
	for case in ("b", "c63"):
		r = score(m, g, case)
		assert all(torch.isfinite(v).all() for v in r.values())
		check_rows_against_own_logits(r, g, case, dtype)


# ------------------------------------------------------------------------------------------------ surface
def forward_args(g, case):
	return (t(g[f"{case}_cond"]).to(DEV), t(g[f"{case}_text"]).to(DEV), t(g[f"{case}_text_lengths"]), t(g[f"{case}_codes"]).to(DEV), t(g[f"{case}_wav_lengths"]))


def bits(x):
	return x.contiguous().view(torch.int32)


def test_forward_returns_losses_and_logits_and_records_them(golden):
	g = golden("ar_score_small")
	m = model_for("small", "f32")
	loss_text, loss_mel, mel_logits = m.forward(*forward_args(g, "a"))
	assert loss_text.shape == () and loss_mel.shape == () and loss_text.dtype == torch.float32 and loss_text.is_cuda and mel_logits.is_cuda
	assert mel_logits.shape == (2, 8194, 11) and mel_logits.dtype == torch.float32 and mel_logits.is_contiguous()
	assert abs(float(loss_text) - float(g["a_loss_text"])) < 2e-4 and abs(float(loss_mel) - float(g["a_loss_mel"])) < 2e-4
	assert set(m.loss) == {"text", "mel"} and torch.equal(m.loss["text"], loss_text) and torch.equal(m.loss["mel"], loss_mel)
	assert m.last_nll["text"].shape == (2, 9) and m.last_nll["mel"].shape == (2, 11)
	assert maxerr(m.last_nll["mel"], g["a_nll_mel"]) < 2e-4 and maxerr(m.last_nll["text"], g["a_nll_text"]) < 2e-4
	again = m(*forward_args(g, "a"))
	assert all(torch.equal(bits(x), bits(y)) for x, y in zip(again, (loss_text, loss_mel, mel_logits)))          # deterministic, and __call__ is forward
	for kw in (dict(text_first=False), dict(raw_mels=torch.zeros(2, 80, 44)), dict(return_attentions=True)):
		with pytest.raises(NotImplementedError):
			m.forward(*forward_args(g, "a"), **kw)
	with pytest.raises(IndexError):
		m.forward(*forward_args(g, "a"), types=torch.tensor([1, 1]))          # ids up to 2 * 254 leave the 256-row table, as nn.Embedding would say
	zero = m.forward(*forward_args(g, "a"), types=torch.tensor([0, 0]))
	assert torch.equal(bits(zero[2]), bits(mel_logits))


def test_clip_inputs_equals_the_preclipped_call_bit_for_bit(golden):
	g = golden("ar_score_small")
	m = model_for("small", "f32")
	cond, text, lengths, codes, wav = forward_args(g, "b")
	_, text_c, codes_c = inputs(g, "b")
	clipped = m.forward(cond, text, lengths, codes, wav, clip_inputs=True)
	nll_clipped = {k: v.clone() for k, v in m.last_nll.items()}
	pre = m.forward(cond, text_c, lengths, codes_c, wav, clip_inputs=False)
	assert clipped[2].shape == (3, 8194, 14)
	assert all(torch.equal(bits(x), bits(y)) for x, y in zip(clipped, pre))
	assert all(torch.equal(bits(nll_clipped[k]), bits(m.last_nll[k])) for k in nll_clipped)
	assert maxerr(nll_clipped["mel"], g["b_nll_mel"]) < 2e-4
	lat_clipped = m.forward(cond, text, lengths, codes, wav, return_latent=True, clip_inputs=True)
	lat_pre = m.forward(cond, text_c, lengths, codes_c, wav, return_latent=True, clip_inputs=False)
	assert lat_clipped.shape == (3, 12, W.AR_SMALL.model_dim) and torch.equal(bits(lat_clipped), bits(lat_pre))
	with pytest.raises(ValueError):
		m.forward(cond, text, lengths, codes, torch.tensor([100, 200, 300]))


def test_scoring_handle_keeps_the_latent_path_and_a_plain_handle_refuses_to_score(golden):
	g = golden("ar_score_small")
	args = forward_args(g, "b")
	scoring, plain = model_for("small", "f32"), model_for("small", "f32", scoring=False)
	assert scoring.scoring and not plain.scoring
	a = scoring.forward(*args, return_latent=True, clip_inputs=False)
	b = plain.forward(*args, return_latent=True, clip_inputs=False)
	assert a.shape == (3, 17, W.AR_SMALL.model_dim) and torch.equal(bits(a), bits(b))
	with pytest.raises(NotImplementedError, match="scoring=True"):
		plain.forward(*args)
	cond, text, codes = inputs(g, "b")
	out = torch.empty(2, device=DEV)
	rc = plain.lib.ttk_ar_score(plain._h, cond.data_ptr(), text.data_ptr(), text.shape[1], codes.data_ptr(), codes.shape[1], 3, out.data_ptr(), None, None, None, None,
								_lib.stream_ptr())
	assert rc != 0 and b"text_head" in plain.lib.ttk_last_error()


def test_scoring_between_two_generations_leaves_them_alone(golden):
	g = golden("ar_score_small")
	sd, cfg = state_dict("small")
	text = torch.randint(1, 255, (1, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
	cond = torch.randn(1, cfg.model_dim, generator=torch.Generator().manual_seed(2)).to(DEV)
	kw = dict(num_return_sequences=3, max_generate_length=16, temperature=0.8, top_k=50, do_sample=True)
	m = UnifiedVoice(sd, cfg, dtype="f32", device=DEV, max_batch=4, max_ctx=96)
	first = m.inference_speech(cond, text, **kw)
	loss = m.forward(*forward_args(g, "c63"))
	second = m.inference_speech(cond, text, **kw)
	fresh = UnifiedVoice(sd, cfg, dtype="f32", device=DEV, max_batch=4, max_ctx=96).inference_speech(cond, text, **kw)
	assert torch.equal(second, fresh) and torch.equal(first, fresh)
	assert abs(float(loss[1]) - float(g["c63_loss_mel"])) < 2e-4
