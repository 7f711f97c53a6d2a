"""Greedy search on the device: the argmax form of the token-step kernel (ttk_greedy_step / ttk_ar_greedy_next) against the processor chain run as
torch ops, the loop of `UnifiedVoice.inference_speech` with `do_sample` false or omitted against the restated HF loop on the CPU oracle
(tests/greedy_ref.py), lines, prompts, state hygiene next to the sampling path, and `TTS.inference(do_sample=False)` end to end on small models.

Oracle comparisons of ids need the oracle's pick to be safe from rounding: every such test asserts first that the top-2 margin of the oracle's processed
scores is >= 1e-2 at every generated step -- ten times the f32 logit tolerance the README states.  The weight seeds and mel-head bias edits below were
picked on the CPU so that the oracle alone satisfies it (margins measured then are noted next to each case)."""
import warnings

import pytest
import torch

import greedy_ref as GR
import tortoise_oracle as O
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = W.AR_SMALL
STOP = CFG.stop_mel_token
MARGIN = 1e-2
NEG = -float("inf")


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. the kernel against torch ops
class _Step:
	"""device state of a token step as a caller of ttk_greedy_step holds it, and the same bookkeeping as torch ops"""

	def __init__(self, B, V, steps, off, stop, ids_cols=None, finished=()):
		from tortoise_tts_amd import _lib
		self.B, self.V, self.off, self.stop = B, V, off, stop
		self.unf = torch.ones(B, dtype=torch.long, device=DEV)
		self.unf[list(finished)] = 0
		self.tok = torch.full((B,), -1, dtype=torch.long, device=DEV)
		self.ids = torch.full((B, steps), -1, dtype=torch.long, device=DEV)
		self.col = torch.zeros(B, dtype=torch.long, device=DEV)
		self.hist = torch.ones((B, off + steps), dtype=torch.long, device=DEV)
		self.hist[:, off - 1] = 8192
		self.live = torch.full((1,), int(self.unf.sum()), dtype=torch.int32, device=DEV)
		self.done = torch.zeros(1, dtype=torch.int32, device=DEV)
		a = _lib.SampleArgs()
		a.ld, a.B, a.V = V, B, V                                    # q / ldq / temperature / top_k / top_p stay zero: not read
		a.stop_token, a.unfinished, a.tok, a.ids, a.ids_ld, a.col = stop, self.unf.data_ptr(), self.tok.data_ptr(), self.ids.data_ptr(), steps, self.col.data_ptr()
		a.ids_cols = steps if ids_cols is None else ids_cols
		a.history, a.hist_ld, a.hist_off = self.hist.data_ptr(), self.hist.stride(0), off
		a.live_rows, a.all_done = self.live.data_ptr(), self.done.data_ptr()
		self.args = a

	def clone_for_reference(self):
		r = object.__new__(_Step)
		r.__dict__.update({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items() if k != "args"})
		r.ids_cols = self.args.ids_cols
		return r

	def reference_step(self, picks):
		"""the bookkeeping of ttk_sample_step (include/ttk.h) on the argmax `picks`"""
		rows = torch.arange(self.B, device=DEV)
		nxt = picks * self.unf + self.stop * (1 - self.unf)
		self.tok = nxt.clone()
		c = int(self.col[0])
		if c < self.ids_cols:
			self.ids[:, c] = nxt
		self.hist[rows, self.off + self.col] = nxt
		self.col = self.col + 1
		still = self.unf * (nxt != self.stop).long()
		newly = int((self.unf - still).sum())
		self.unf = still
		if newly:
			self.live -= newly
			if int(self.live[0]) == 0:
				self.done[0] = c + 1

	def same_as(self, r):
		torch.cuda.synchronize()
		for name in ("tok", "ids", "hist", "col", "unf", "live", "done"):
			assert torch.equal(getattr(self, name), getattr(r, name)), (name, getattr(self, name).tolist(), getattr(r, name).tolist())


def _processed(input_ids, lg, pen, mask, mass=None):
	s = lg
	if pen != 1.0:
		s = O.warp_repetition_penalty(input_ids, s, pen)
	if mask is not None:
		s = torch.where(mask, NEG, s)
	if mass is not None:
		s = O.warp_typical(s, mass)
	return s


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("case", ["plain", "penalty", "suppress", "finished_row", "short_ids"])
def test_greedy_kernel_equals_the_processor_chain_and_argmax_as_torch_ops(lib, B, case):
	"""tok, ids, history, col, unfinished, live_rows and all_done after each of three consecutive steps (the history the penalty reads grows), exact"""
	from tortoise_tts_amd import _lib
	V, steps, off = 8194, 3, 2
	g = torch.Generator().manual_seed(100 * B + len(case))
	pen = 2.0 if case == "penalty" else 1.0
	st = _Step(B, V, steps, off, STOP, ids_cols=2 if case == "short_ids" else None, finished=(B - 1,) if case == "finished_row" else ())
	ref = st.clone_for_reference()
	logits = [(torch.randn((B, V), generator=g) * 4).to(DEV) for _ in range(steps)]
	if case == "plain":
		logits[1][0, STOP] = 50.0                                  # row 0 finishes with the second token; it is padded from then on
	mask = None
	if case == "suppress":                                        # the mask covers the unprocessed maximum of every row at every step
		mask = torch.zeros(V, dtype=torch.bool, device=DEV)
		for lg in logits:
			mask[lg.argmax(dim=-1)] = True
		mask[STOP] = True
		st.args.suppress = mask.data_ptr()
	st.args.repetition_penalty = pen
	for n, lg in enumerate(logits):
		if case == "penalty":
			# repeated ids with positive scores (halved: they lose although they were the maximum) and with negative ones (doubled), in one batch:
			# odd rows are shifted below zero; id 1 (in every prefix) and, from the second step on, the row's previous pick are its raw maximum
			lg[1::2] -= lg[1::2].max(dim=-1, keepdim=True).values + 1.0
			top = lg.max(dim=-1).values
			lg[:, 1] = torch.where(top > 0, top + 1.0, top * 0.75)
			if n:
				prev = ref.tok.clamp(max=V - 1)
				top = lg.max(dim=-1).values
				lg[torch.arange(B, device=DEV), prev] = torch.where(top > 0, top + 0.5, top * 0.9)
			raw = lg.argmax(dim=-1)
		input_ids = ref.hist[:, :off + n]
		picks = GR.argmax_lowest(_processed(input_ids, lg, pen, mask))
		if case == "penalty":
			assert bool((picks != raw).any())                       # the penalty decided somewhere in this step
		if case == "suppress":
			assert bool((picks != lg.argmax(dim=-1)).all())
		ref.reference_step(picks)
		st.args.scores = lg.data_ptr()
		_lib.check(lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_greedy_step")
		st.same_as(ref)
	if case == "plain":
		assert int(st.ids[0, 1]) == STOP and int(st.ids[0, 2]) == STOP and int(st.unf[0]) == 0
		assert int(st.done[0]) == (2 if B == 1 else 0)
	if case == "short_ids":
		assert bool((st.ids[:, 2] == -1).all()) and bool((st.hist[:, off + 2] >= 0).all())
	if case == "finished_row":
		assert bool((st.ids[B - 1] == STOP).all())


def test_exact_ties_go_to_the_lowest_index(lib):
	from tortoise_tts_amd import _lib
	V = 8194
	lg = (torch.randn((2, V), generator=torch.Generator().manual_seed(3)) * 2).to(DEV)
	lg[:, [5, 4000, 8193]] = 40.0
	st = _Step(2, V, 1, 2, V + 5)
	st.args.scores = lg.data_ptr()
	_lib.check(lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_greedy_step")
	torch.cuda.synchronize()
	assert st.tok.tolist() == [5, 5]
	# with the first two maxima suppressed the third one, in the last column, is what is left
	mask = torch.zeros(V, dtype=torch.bool, device=DEV)
	mask[[5, 4000]] = True
	st = _Step(2, V, 1, 2, V + 5)
	st.args.scores, st.args.suppress = lg.data_ptr(), mask.data_ptr()
	_lib.check(lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_greedy_step")
	torch.cuda.synchronize()
	assert st.tok.tolist() == [8193, 8193]


def test_typical_warper_acts_in_front_of_the_argmax(lib):
	"""a row whose most likely token is far from typical: the warper removes it and the pick is the best token it keeps"""
	from tortoise_tts_amd import _lib
	V, mass, B = 8194, 0.3, 3
	lg = torch.randn((B, V), generator=torch.Generator().manual_seed(9)) * 0.5
	peak = torch.tensor([17, 4242, 8000])
	lg[torch.arange(B), peak] = torch.logsumexp(lg, dim=-1) + torch.log(torch.tensor(0.4 / 0.6))       # p(peak) ~ 0.4
	assert lg.argmax(dim=-1).tolist() == peak.tolist()
	kept = O.warp_typical(lg, mass)
	assert bool((kept[torch.arange(B), peak] == NEG).all())         # the precondition: the unprocessed argmax is masked
	want = GR.argmax_lowest(kept)
	assert not bool((want == peak).any())
	d = lg.to(DEV)
	st = _Step(B, V, 1, 2, V + 5)
	st.args.scores, st.args.typical_mass = d.data_ptr(), mass
	_lib.check(lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_greedy_step")
	torch.cuda.synchronize()
	assert st.tok.cpu().tolist() == want.tolist()
	assert st.tok.cpu().tolist() == GR.argmax_lowest(O.warp_typical(d, mass)).cpu().tolist()           # and the chain as torch ops on the device


def test_greedy_entries_refuse_what_they_cannot_do(lib):
	from tortoise_tts_amd import _lib
	V = 8194
	lg = torch.zeros((1, 9217), device=DEV)
	st = _Step(1, V, 1, 2, STOP)
	st.args.scores, st.args.ld = lg.data_ptr(), 9217
	assert st.args.q is None                                       # q = NULL is not an error here
	assert lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()) == 0
	st.args.V = 9217
	assert lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()) == -1 and b"ttk_greedy_step" in lib.ttk_last_error()       # TTK_E_ARG
	st.args.V = V
	for field in ("scores", "tok", "col", "unfinished"):
		keep = getattr(st.args, field)
		setattr(st.args, field, None)
		assert lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()) == -1, field
		setattr(st.args, field, keep)
	st.args.repetition_penalty, st.args.history = 2.0, None
	assert lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()) == -1 and b"history" in lib.ttk_last_error()
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the AR-aware entry
def make_ar(seed, dtype, edit=None, **kw):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	sd = W.synth_state_dict(W.ar_shapes(CFG), seed)
	if edit is not None:
		edit(sd)
	kw = dict(dict(max_batch=4, max_ctx=96), **kw)
	return UnifiedVoice(sd, CFG, dtype=dtype, device=DEV, **kw), sd


def line(seed=1, n=9):
	text = torch.randint(1, 255, (1, n), generator=torch.Generator().manual_seed(seed))
	cond = torch.randn(1, CFG.model_dim, generator=torch.Generator().manual_seed(2))
	return cond, text


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_greedy_next_and_decode_next_equal_greedy_step_and_decode(lib, dtype, B):
	"""the launch that also writes the next step's input row, then the decode step that starts from it == the plain launch, then ttk_ar_decode of its
	token: the logits of the following steps bit for bit"""
	from tortoise_tts_amd import _lib
	model, _ = make_ar(12, dtype)
	cond, text = line()
	V = CFG.number_mel_codes
	runs = []
	for fused in (True, False):
		with torch.cuda.device(model.device):
			logits = model._prefill(cond, text, B).clone()
			if B > 1:
				logits[1:] += torch.randn((B - 1, V), generator=torch.Generator().manual_seed(4)).to(DEV)      # rows that pick different tokens
			st = _Step(B, V, 4, 2, STOP)
			st.args.suppress = None
			st.args.scores, st.args.ld = logits.data_ptr(), logits.stride(0)
			out = []
			for _ in range(3):
				if fused:
					_lib.check(lib.ttk_ar_greedy_next(model._h, _lib.C.byref(st.args), _lib.stream_ptr()), "ttk_ar_greedy_next")
					model._decode_next(logits)
				else:
					_lib.check(lib.ttk_greedy_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_greedy_step")
					model._decode(st.tok, logits)
				out.append(logits.clone())
			torch.cuda.synchronize()
			runs.append((st.ids.clone(), torch.stack(out)))
	assert torch.equal(runs[0][0], runs[1][0]) and bool((runs[0][0][:, :3] >= 0).all())
	assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the loop against the oracle
def oracle_ids(sd, cond, text, **kw):
	with torch.inference_mode():
		ids, margins = GR.greedy_search(O.AROracle(sd, CFG), cond, text, return_margins=True, **kw)
	print(f"\n[greedy] oracle: {ids.shape[1]} tokens, smallest top-2 margin {min(margins):.4f}")
	assert min(margins) >= MARGIN, margins                          # the precondition: no pick of the oracle is within rounding of another
	return ids


def _bias_stop(by):
	def edit(sd):
		sd["mel_head.bias"] = sd["mel_head.bias"].clone()
		sd["mel_head.bias"][STOP] += by
	return edit


def _boost_four(sd):
	"""four dominant mel codes: greedy search keeps repeating them unless the penalty acts"""
	sd["mel_head.bias"] = sd["mel_head.bias"].clone()
	sd["mel_head.bias"][100:104] += 4.0


# (weight seed, edit of the synthetic weights, keywords): picked on the CPU; margins measured then: 0.033 (10 tokens) and 0.039 (24 tokens)
LOOP_CASES = {
	"ends_early": (18, _bias_stop(2.5), dict()),
	"runs_to_max_length": (12, None, dict(suppress_tokens=[STOP])),
}


@pytest.fixture(scope="module")
def loop_refs():
	"""the oracle's greedy ids of the loop cases, computed once"""
	cond, text = line()
	refs = {}
	for name, (seed, edit, kw) in LOOP_CASES.items():
		sd = W.synth_state_dict(W.ar_shapes(CFG), seed)
		if edit is not None:
			edit(sd)
		refs[name] = oracle_ids(sd, cond, text, max_generate_length=24, **kw)
	return refs


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_inference_speech_without_do_sample_is_greedy_search_f32(lib, loop_refs, name):
	from tortoise_tts_amd.sampling import setup_seed
	seed, edit, kw = LOOP_CASES[name]
	ref = loop_refs[name]
	assert (ref.shape[1] < 24 and int(ref[0, -1]) == STOP and ref.shape[1] > 1) if name == "ends_early" else (ref.shape[1] == 24 and not bool((ref == STOP).any()))
	cond, text = line()
	gen = torch.cuda.default_generators[0]
	setup_seed(0)
	behind_reseed = gen.get_offset()
	got = {}
	for use_graph in (True, False):
		model, _ = make_ar(seed, "f32", edit, use_graph=use_graph)
		torch.rand(7, device=DEV)                                   # the generator is somewhere else when the call starts
		with warnings.catch_warnings():
			warnings.filterwarnings("error", message=".*greedy.*")   # nothing to warn about: no ignored warper was passed
			ids = model.inference_speech(cond.to(DEV), text.to(DEV), max_generate_length=24, **kw)      # do_sample omitted
		assert gen.get_offset() == behind_reseed and gen.initial_seed() == 0
		assert model.last_generate["rng_step"] == 0 and model.last_generate["steps"] == ids.shape[1]
		assert ids.shape == ref.shape and torch.equal(ids.cpu(), ref), (use_graph, ids.tolist(), ref.tolist())
		again = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=False, max_generate_length=24, **kw)
		assert torch.equal(again, ids)
		got[use_graph] = ids
	assert torch.equal(got[True], got[False])


# ------------------------------------------------------------------------------------------------ 4. ignored warpers, acting processors
def test_warpers_are_ignored_with_one_warning_and_the_penalty_acts(lib):
	cond, text = line()
	model, sd = make_ar(12, "f32", _boost_four)
	base = dict(max_generate_length=24, suppress_tokens=[STOP])
	ref_plain = oracle_ids(sd, cond, text, **base)                  # margins measured on the CPU: 0.056 plain, 0.038 with the penalty
	ref_pen = oracle_ids(sd, cond, text, repetition_penalty=2.0, **base)
	assert not torch.equal(ref_plain, ref_pen)
	plain = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=False, **base)
	with pytest.warns(UserWarning, match="temperature.*top_k.*top_p") as rec:
		warped = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=False, temperature=0.5, top_k=5, top_p=0.5, **base)
	assert len([w for w in rec if issubclass(w.category, UserWarning) and "greedy" in str(w.message)]) == 1
	assert torch.equal(plain, warped) and torch.equal(plain.cpu(), ref_plain)
	assert len(model._states) == 1                                  # ignored keywords are not part of what a state is keyed by
	pen = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=False, repetition_penalty=2.0, **base)
	assert torch.equal(pen.cpu(), ref_pen) and not torch.equal(pen, plain)
	# the typical warper acts as well.  On these weights its kept set is a band of near-equal scores (oracle margins ~1e-5), so the ids are not pinned
	# here; the kernel's pick behind the warper is, in test_typical_warper_acts_in_front_of_the_argmax
	typ = model.inference_speech(cond.to(DEV), text.to(DEV), do_sample=False, typical_sampling=True, typical_mass=0.2, max_generate_length=6, suppress_tokens=[STOP])
	assert typ.shape == (1, 6) and not torch.equal(typ, plain[:, :6])


# ------------------------------------------------------------------------------------------------ 5. prompted continuation
def test_prompted_continuation_is_greedy_behind_the_prompt(lib):
	cond, text = line()
	prompt = torch.randint(0, 8192, (1, 4), generator=torch.Generator().manual_seed(5))
	model, sd = make_ar(12, "f32")
	kw = dict(max_generate_length=24, suppress_tokens=[STOP])
	ref = oracle_ids(sd, cond, text, input_tokens=prompt, **kw)     # margin measured on the CPU: 0.019
	got = model.inference_speech(cond.to(DEV), text.to(DEV), input_tokens=prompt.to(DEV), num_return_sequences=1, do_sample=False, **kw)
	assert got.shape == (1, 24) and torch.equal(got[:, :4].cpu(), prompt) and torch.equal(got.cpu(), ref)
	assert model.last_generate["rng_step"] == 0 and model.last_generate["steps"] == 20
	with pytest.raises(ValueError, match="stop token"):
		model.inference_speech(cond.to(DEV), text.to(DEV), input_tokens=torch.tensor([[3, STOP]]), do_sample=False)


# ------------------------------------------------------------------------------------------------ 6. lines
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lines_as_one_batch_equal_the_per_line_calls(lib, dtype):
	model, _ = make_ar(18, dtype, _bias_stop(2.5))
	cond = line()[0].to(DEV)
	texts = [line(seed=20 + n, n=n)[1].to(DEV) for n in (5, 8, 13)]
	kw = dict(do_sample=False, max_generate_length=24)
	batch = model.inference_speech_lines(cond, texts, **kw)
	assert [g["rng_step"] for g in model.last_generate_lines] == [0, 0, 0]
	lens = []
	for g, t in enumerate(texts):
		alone = model.inference_speech(cond, t, **kw)
		assert batch[g].shape == alone.shape and torch.equal(batch[g], alone), (g, batch[g].tolist(), alone.tolist())
		assert model.last_generate_lines[g]["steps"] == alone.shape[1]
		lens.append(alone.shape[1])
	print(f"\n[greedy] line lengths {lens}")
	with pytest.raises(ValueError, match="num_return_sequences"):
		model.inference_speech_lines(cond, texts, do_sample=False, num_return_sequences=2)


# ------------------------------------------------------------------------------------------------ 7. state hygiene
def test_greedy_between_two_sampling_calls_leaves_them_equal(lib):
	cond, text = line()
	model, _ = make_ar(12, "f32")
	skw = dict(do_sample=True, num_return_sequences=3, max_generate_length=16, temperature=0.8, top_k=0)
	c, t = cond.to(DEV), text.to(DEV)
	first = model.inference_speech(c, t, **skw)
	off = torch.cuda.default_generators[0].get_offset()
	greedy = model.inference_speech(c, t, do_sample=False, max_generate_length=16)
	second = model.inference_speech(c, t, **skw)
	assert torch.equal(first, second) and torch.cuda.default_generators[0].get_offset() == off       # no noise left armed, no graph shared
	assert torch.equal(greedy, model.inference_speech(c, t, max_generate_length=16))
	assert len({k[2][6] for k in model._states}) == 2               # a sampling state and a greedy state, each with its own captured step


def test_greedy_bf16_is_deterministic_across_fresh_handles(lib):
	cond, text = line()
	out = []
	for _ in range(2):
		model, _ = make_ar(12, "bf16")
		out.append(model.inference_speech(cond.to(DEV), text.to(DEV), max_generate_length=24, suppress_tokens=[STOP]))
	assert out[0].shape == (1, 24) and torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------ 8. end to end, small models
@pytest.fixture(scope="module")
def small_tts(golden):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	sd_ar = W.synth_state_dict(W.ar_shapes(CFG), 18)
	_bias_stop(2.5)(sd_ar)
	sd_df = W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32)
	sd_voc = W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33)
	tts = TTS(UnifiedVoice(sd_ar, CFG, dtype="f32", device=DEV, max_batch=8, max_ctx=128), DiffusionTTS(sd_df, W.DIFF_SMALL, dtype="f32", device=DEV), tok,
			  vocoder=BigVGAN(sd_voc, W.VOC_SMALL, dtype="f32", device=DEV))
	dl = torch.randn(1, 2 * W.DIFF_SMALL.model_channels, generator=torch.Generator().manual_seed(6)).to(DEV)
	return tts, sd_ar, dl


def test_tts_inference_greedy_ignores_the_sampling_arguments(small_tts):
	tts, _, dl = small_tts
	voice = {"latent": (line()[0].to(DEV), dl)}
	kw = dict(max_ar_steps=10, max_diffusion_steps=3, do_sample=False, seed=77)
	with warnings.catch_warnings():
		warnings.filterwarnings("error", message=".*greedy.*")       # the orchestration does not hand ignored defaults on
		a, sr = tts.inference("Hello there.\nThe end!", voice, **kw)
	b, _ = tts.inference("Hello there.\nThe end!", voice, ar_temp=0.3, top_k=7, top_p=0.6, **kw)
	assert sr == 24000 and a.dim() == 3 and torch.isfinite(a).all() and torch.equal(a, b)
	c, _ = tts.inference("Hello there.", voice, **kw)               # one line: the per-line path
	d, _ = tts.inference("Hello there.", voice, ar_temp=0.3, **kw)
	assert torch.equal(c, d) and torch.equal(c, a[..., :c.shape[-1]])


def test_hot_path_greedy_diffuses_the_oracle_checked_codes(small_tts, loop_refs):
	from tortoise_tts_amd.diffusion import get_diffuser
	from tortoise_tts_amd.inference import fix_stop_tokens, trim_calm_tokens
	from tortoise_tts_amd.sampling import setup_seed
	tts, sd_ar, dl = small_tts
	hot, ar, diff = tts.hot, tts.hot.autoregressive, tts.hot.diffusion
	cond, text = line()
	cond, text = cond.to(DEV), text.to(DEV)
	torch.rand(5, device=DEV)
	mels, seconds, aux = hot.inference(text, cond, dl, max_ar_steps=24, max_diffusion_steps=3, do_sample=False, return_all=True)
	codes = fix_stop_tokens(loop_refs["ends_early"], STOP)          # the same weights, line and budget as the loop test's early end
	assert torch.equal(aux["codes"].cpu(), codes) and aux["scores"] is None and aux["best"] == 0
	with torch.inference_mode():
		setup_seed(0)                                               # where `generate` leaves the generators: reseeded, nothing drawn
		codes = codes.to(DEV)
		latents = ar.forward(cond, text, torch.tensor([text.shape[1]], dtype=torch.int32), codes, torch.tensor([codes.shape[1] * ar.mel_length_compression]),
							 return_latent=True, clip_inputs=False)
		latents = trim_calm_tokens(codes, latents)
		T = latents.shape[1] * 4 * 24000 // 22050
		E = diff.timestep_independent(latents, dl, T, False)
		noise = torch.randn((1, 100, T), device=DEV)
		mel = get_diffuser(steps=3, cond_free=True).sample_loop(diff, (1, 100, T), sampler="ddim", noise=noise, model_kwargs={"precomputed_aligned_embeddings": E}, progress=False)
	assert torch.equal(aux["noise"], noise) and torch.equal(aux["mel"], mel) and mels.shape == (1, 100, T) and seconds > 0
