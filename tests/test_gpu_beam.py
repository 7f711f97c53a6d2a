"""Beam search on the device (csrc/beam.hip; include/ttk.h: ttk_ar_reorder_cache, ttk_beam_step) against torch and the restated HF loop
(tests/beam_ref.py, itself pinned to the installed `_beam_search` by tests/test_beam_ref.py):
  * the in-place KV reorder: logits after it equal, bit for bit, those of a handle fed the permuted token histories directly;
  * the beam step alone on given logits: its 2 * num_beams picks are `torch.multinomial(softmax(acc), 2 * num_beams)` on the same generator state,
    and the state it leaves is the restated loop's, step by step;
  * the loop: `inference_speech(num_beams=N)` ids equal `beam_ref.beam_search` on the CPU oracle sampled on the device, and the generator ends
    where the reference's does;
  * `TTS.inference(beam_width=)`.
GPU only; every call goes through the C ABI."""
import types

import pytest
import torch

import beam_ref as BR
import tortoise_oracle as O
from test_gpu_tts import parts, speechlike  # noqa: F401  (the tiny `TTS` of the text-to-waveform tests)
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = W.AR_SMALL
V, STOP = CFG.number_mel_codes, CFG.stop_mel_token


def make_ar(dtype, sd=None, **kw):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	sd = W.synth_state_dict(W.ar_shapes(CFG), 11) if sd is None else sd
	return UnifiedVoice(sd, CFG, dtype=dtype, device=DEV, **kw), sd


def inputs(n_text=9):
	text = torch.randint(1, 255, (1, n_text), generator=torch.Generator().manual_seed(1))
	cond = torch.randn(1, CFG.model_dim, generator=torch.Generator().manual_seed(2))
	return cond, text


# ------------------------------------------------------------------------------------------------ the KV reorder
def _history(B, steps, seed):
	"""distinct tokens per row and step"""
	return torch.randperm(8000, generator=torch.Generator().manual_seed(seed))[:B * steps].view(B, steps)


def _run(model, toks, B, reorder=None, after=None):
	"""prefill B rows, decode the columns of `toks`; then optionally ttk_ar_reorder_cache(reorder) and one more step fed `after`: the last logits"""
	from tortoise_tts_amd import _lib
	cond, text = inputs()
	logits = model._prefill(cond.to(DEV), text.to(DEV), B).clone()
	toks = toks.to(DEV)
	for k in range(toks.shape[1]):
		model._decode(toks[:, k].contiguous(), logits)
	if reorder is not None:
		idx = torch.tensor(reorder, dtype=torch.long, device=DEV)
		_lib.check(model.lib.ttk_ar_reorder_cache(model._h, idx.data_ptr(), _lib.stream_ptr()), "ttk_ar_reorder_cache")
	if after is not None:
		model._decode(after.to(DEV).contiguous(), logits)
	torch.cuda.synchronize()
	return logits.cpu()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("beam_idx", [[1, 0, 3, 3], [2, 2, 0], [5, 5, 0, 3, 15, 14, 1, 7, 8, 2, 2, 11, 9, 13, 6, 4]], ids=["B4", "B3", "B16"])
def test_reorder_equals_feeding_the_permuted_histories(dtype, beam_idx):
	B = len(beam_idx)
	hist, nxt = _history(B, 3, 5), _history(B, 1, 6)[:, 0]
	a, _ = make_ar(dtype, max_batch=16, max_ctx=64)
	b, _ = make_ar(dtype, max_batch=16, max_ctx=64)
	got = _run(a, hist, B, reorder=beam_idx, after=nxt)
	want = _run(b, hist[beam_idx], B, after=nxt)                 # row b was fed row beam_idx[b]'s history from the start
	assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got - want).abs().max()
	plain = _run(b, hist, B, after=nxt)
	if beam_idx[0] != 0:
		assert not torch.equal(got[0], plain[0])                 # (the reorder did something)
	same = _run(a, hist, B, reorder=list(range(B)), after=nxt)   # identity: as if the call had not been made
	assert torch.equal(same.view(torch.int32), plain.view(torch.int32))


def test_reorder_is_refused_without_a_prefill_and_in_lines_mode():
	from tortoise_tts_amd import _lib
	m, _ = make_ar("f32", max_batch=4, max_ctx=64)
	idx = torch.arange(4, dtype=torch.long, device=DEV)
	assert m.lib.ttk_ar_reorder_cache(m._h, idx.data_ptr(), _lib.stream_ptr()) == -4          # TTK_E_STATE
	cond, text = inputs()
	m._prefill_lines(cond.to(DEV), [text.to(DEV), text[:, :5].to(DEV)], 2)
	assert m.lib.ttk_ar_reorder_cache(m._h, idx.data_ptr(), _lib.stream_ptr()) == -4
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the beam step alone
class _TableAR:
	"""the oracle interface over given logits: step k's rows are table[k], whatever was fed (tests/beam_ref.py drives it)"""

	def __init__(self, table):
		self.table = table
		self.cfg = types.SimpleNamespace(stop_mel_token=STOP, start_mel_token=CFG.start_mel_token, max_mel_tokens=CFG.max_mel_tokens)

	def prefix_embeddings(self, cond, text):
		return torch.zeros(1, 12, 1)

	def prefill(self, prefix, B):
		return self.table[0][:, None], None, None

	def decode(self, nxt, k, past):
		return self.table[k], None, None


@pytest.mark.parametrize("kw", [dict(temperature=0.8, top_k=0), dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=2.0, length_penalty=2.0)],
						 ids=["plain", "warpers"])
def test_beam_step_picks_equal_torch_multinomial_and_state_follows_the_reference(kw):
	from tortoise_tts_amd import _lib
	lib = _lib.load()
	N, steps = 4, 3
	max_new = steps                                               # the reference below runs with max_length = prompt + steps: the same MaxLengthCriteria
	K = 2 * N
	g = torch.Generator().manual_seed(21)
	table = torch.randn(steps, N, V, generator=g) * 2.0
	table[:, :, STOP] += 7.5                                      # some of the picks are the stop token: beams finish within the three steps
	trace = []
	with torch.inference_mode():
		BR.beam_search(_TableAR(table), None, None, num_beams=N, num_return_sequences=1, max_generate_length=steps, sample_device=DEV, step_trace=trace, **kw)
	assert len(trace) == steps and any(bool(t["finished"].any()) for t in trace[:-1])
	# the kernel on the same logits, torch's own exponential_ noise for the flat [1, N * V] tensor, the same generator state
	torch.manual_seed(0); torch.cuda.manual_seed_all(0)
	logits = torch.empty((N, V), device=DEV)
	q = torch.empty((1, N * V), device=DEV)
	col = torch.zeros(N, dtype=torch.long, device=DEV)
	seqs = torch.full((2, 2, N, max_new), STOP, dtype=torch.long, device=DEV)
	scores = torch.full((2, N), -1e9, device=DEV)
	scores[0, 0] = 0.0
	state = torch.zeros(2 * N + 2, dtype=torch.int32, device=DEV)
	state[2 * N] = 1
	acc = torch.empty(N * V, device=DEV)
	work = torch.zeros(4 * N * N + 2 * N + 1, dtype=torch.int32, device=DEV)
	tok, beam_idx = torch.zeros(N, dtype=torch.long, device=DEV), torch.zeros(N, dtype=torch.long, device=DEV)
	a = _lib.BeamArgs()
	a.logits, a.ld, a.num_beams, a.V, a.q = logits.data_ptr(), V, N, V, q.data_ptr()
	a.temperature, a.top_k, a.top_p = kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0)
	a.repetition_penalty, a.length_penalty = kw.get("repetition_penalty", 1.0), kw.get("length_penalty", 1.0)
	a.stop_token, a.max_new = STOP, max_new
	a.prefix_ids[0], a.prefix_ids[1] = 1, CFG.start_mel_token
	a.col, a.seqs, a.scores, a.state = col.data_ptr(), seqs.data_ptr(), scores.data_ptr(), state.data_ptr()
	a.acc, a.work, a.tok, a.beam_idx = acc.data_ptr(), work.data_ptr(), tok.data_ptr(), beam_idx.data_ptr()
	for k in range(steps):
		logits.copy_(table[k])
		q.exponential_(1)
		_lib.check(lib.ttk_beam_step(_lib.C.byref(a), _lib.stream_ptr()), "ttk_beam_step")
		torch.cuda.synchronize()
		t = trace[k]
		cr = work[2 * N:2 * N + N * K].view(torch.float32).cpu()
		ci = work[2 * N + N * K:2 * N + 2 * N * K].cpu().long()
		order = sorted(range(N * K), key=lambda i: (-float(cr[i]), int(ci[i])))[:K]
		picks = ci[order]
		print(f"\n[beam step {k}] picks {picks.tolist()} torch {t['picks'].tolist()}")
		assert torch.equal(picks, t["picks"]), k
		# (the last step is at max_length: every pick hits MaxLengthCriteria, the running scores all tie at -1e9 and which of them torch.topk keeps is
		# unspecified -- and unused, the search is over; before it at least num_beams picks are not the stop token)
		at_max = k == steps - 1
		if not at_max:
			assert torch.equal(tok.cpu(), t["tok"]) and torch.equal(beam_idx.cpu(), t["beam_idx"]), k
		st = state.cpu()
		assert st[:N].bool().tolist() == t["finished"].tolist() and bool(st[2 * N]) == t["unsatisfied"], k
		fin = t["finished"]
		assert st[N:2 * N][fin].tolist() == t["lengths"][fin].tolist(), k
		half = (k + 1) & 1
		if not at_max:
			assert torch.equal(seqs[half, 0, :, :steps].cpu(), t["running"][:, :steps]), k
		assert torch.equal(seqs[half, 1][fin.to(DEV)][:, :steps].cpu(), t["sequences"][fin][:, :steps]), k
		sc = scores.cpu()
		# sums of f32 log-probs computed by two implementations of log_softmax: a few ulp of values of magnitude <= ~40 (-1e9 entries: ulp 64)
		assert torch.allclose(sc[0], t["running_scores"], rtol=2e-6, atol=1e-4) and torch.allclose(sc[1], t["beam_scores"], rtol=2e-6, atol=1e-4), k
		assert int(col[0]) == k + 1 and int(st[2 * N + 1]) == (steps if k == steps - 1 else 0)
	# a call after the end changes nothing
	before = (seqs.clone(), scores.clone(), state.clone(), tok.clone())
	_lib.check(lib.ttk_beam_step(_lib.C.byref(a), _lib.stream_ptr()), "ttk_beam_step")
	torch.cuda.synchronize()
	assert all(torch.equal(x, y) for x, y in zip(before, (seqs, scores, state, tok)))


# ------------------------------------------------------------------------------------------------ the loop
def first_divergence(a, b):
	"""per row: first column where a and b differ (the common width when they never do)"""
	n = min(a.shape[1], b.shape[1])
	ne = a[:, :n] != b[:, :n]
	return torch.where(ne.any(dim=1), ne.float().argmax(dim=1), torch.full((a.shape[0],), n)).tolist()


LOOP_CASES = {
	"four_beams_two_returned": (6.0, dict(num_beams=4, num_return_sequences=2, max_generate_length=24, temperature=0.8, top_k=0)),
	"two_beams_warpers": (5.0, dict(num_beams=2, num_return_sequences=2, max_generate_length=24, temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=2.0)),
	"length_penalty": (6.0, dict(num_beams=4, num_return_sequences=3, max_generate_length=24, temperature=0.9, top_k=0, length_penalty=2.0)),
	"runs_to_max_length": (0.0, dict(num_beams=3, num_return_sequences=1, max_generate_length=12, temperature=0.8, top_k=0)),
}


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_inference_speech_beams_equal_the_restated_loop_f32(name):
	bias, kw = LOOP_CASES[name]
	sd = W.synth_state_dict(W.ar_shapes(CFG), 11)
	sd["mel_head.bias"] = sd["mel_head.bias"].clone()
	sd["mel_head.bias"][STOP] += bias                             # makes beams finish before max_generate_length
	model, _ = make_ar("f32", sd=sd, max_batch=4, max_ctx=96)
	cond, text = inputs()
	gen = torch.cuda.default_generators[0]
	with torch.inference_mode():
		want, tr = BR.beam_search(O.AROracle(sd, CFG), cond, text, sample_device=DEV, return_trace=True, **kw)
		off_ref = gen.get_offset()
		got = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=True, **kw).cpu()
		off_got = gen.get_offset()
	print(f"\n[beam loop {name}] steps {tr['steps']} lengths {tr['lengths'].tolist()} returned {tuple(want.shape)}; product {tuple(got.shape)} steps {model.last_generate['steps']}")
	assert got.shape == want.shape and torch.equal(got, want), ("first divergence per row", first_divergence(got, want), got.tolist(), want.tolist())
	assert model.last_generate["steps"] == tr["steps"] and off_got == off_ref
	if name == "runs_to_max_length":
		assert tr["steps"] == kw["max_generate_length"]
	if name == "four_beams_two_returned":
		assert tr["steps"] < kw["max_generate_length"]            # (ended on the heuristic, with every finished slot filled)
		# the sampling path right after a beam search on the same handle: its ids are what they were (the noise arming and the cache are per call)
		skw = dict(num_return_sequences=3, max_generate_length=10, temperature=0.8, top_k=0)
		with torch.inference_mode():
			ref = O.inference_speech(O.AROracle(sd, CFG), cond, text, sample_device="cuda", **skw)
			ids = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=True, num_beams=1, **skw).cpu()
		assert torch.equal(ids, ref)


# ------------------------------------------------------------------------------------------------ TTS.inference(beam_width=)
def test_tts_beam_width(parts):  # noqa: F811
	tts, sd, norms = parts
	enc = tts.encode_audio(speechlike(9, 30000, 22050).to(DEV), 22050)
	kw = dict(max_ar_steps=10, max_diffusion_steps=3, candidates=2)
	base, sr = tts.inference("Hello there.", enc, seed=1234, **kw)
	one, _ = tts.inference("Hello there.", enc, seed=1234, beam_width=1, **kw)
	assert torch.equal(base, one)                                 # beam_width=1 is the sampling path, untouched
	by_hand = tts.hot.inference_to_wav(tts.encode_text("Hello there.").to(DEV)[None], enc["latent"][0], enc["latent"][1], **kw)[0]
	assert torch.equal(one, by_hand)
	out, sr = tts.inference("Hello there.\nThe end!", enc, seed=1234, beam_width=2, **kw)
	assert sr == 24000 and out.dim() == 3 and out.shape[:2] == (1, 1) and out.shape[-1] > 0
	assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
	again, _ = tts.inference("Hello there.\nThe end!", enc, seed=1234, beam_width=2, **kw)
	assert torch.equal(out, again)
	with pytest.raises(ValueError, match="num_return_sequences"):
		tts.inference("Hello.", enc, beam_width=2, max_ar_steps=10, max_diffusion_steps=3, candidates=3)
