"""Beam search over a batch of lines (csrc/beam.hip; include/ttk.h: ttk_beam_step_lines, ttk_ar_reorder_cache_lines; UnifiedVoice.beam_search_lines) against
the single-line entries, which tests/test_gpu_beam.py pins to the restated HF loop -- every line's result is bit for bit that of its own call:
  * the KV reorder in lines mode: logits after it equal those of a handle fed the permuted histories directly; identity and line-crossing entries move nothing;
  * the step alone: G lines on given logit tables, word for word the state ttk_beam_step leaves on each line alone, lines ending at different steps;
  * the loop: `beam_search_lines` against `inference_speech(num_beams=N)` per line, f32 and bf16, noise from the mel-head launch and from torch;
  * `TTSHotPath.inference_lines(beam_width=)` and `TTS.inference` on a text of several lines.
GPU only; every call goes through the C ABI."""
import pytest
import torch

import beam_ref as BR
import tortoise_oracle as O
from test_gpu_beam import LOOP_CASES, first_divergence
from test_gpu_tts import parts, speechlike  # noqa: F401  (the tiny `TTS` of the text-to-waveform tests)
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = W.AR_SMALL
V, STOP = CFG.number_mel_codes, CFG.stop_mel_token
E_STATE = -4


def make_ar(dtype, sd=None, **kw):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	sd = W.synth_state_dict(W.ar_shapes(CFG), 11) if sd is None else sd
	return UnifiedVoice(sd, CFG, dtype=dtype, device=DEV, max_batch=16, max_ctx=96, **kw)


def texts_of(lens, seed):
	g = torch.Generator().manual_seed(seed)
	return [torch.randint(1, 255, (1, n), generator=g).to(DEV) for n in lens]


def cond_latent():
	return torch.randn(1, CFG.model_dim, generator=torch.Generator().manual_seed(2)).to(DEV)


def bits(t):
	return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ the KV reorder in lines mode
ROWS = 3                                                          # rows per line: two lines of 9 and 5 text tokens


def _run_lines(model, toks, reorder=None, after=None):
	"""prefill 2 lines x ROWS rows, decode the columns of `toks`; then optionally ttk_ar_reorder_cache_lines(reorder) and one more step fed `after`: the last logits"""
	logits = model._prefill_lines(cond_latent(), texts_of([9, 5], 1), ROWS).clone()
	toks = toks.to(DEV)
	for k in range(toks.shape[1]):
		model._decode(toks[:, k].contiguous(), logits)
	if reorder is not None:
		idx = torch.tensor(reorder, dtype=torch.long, device=DEV)
		_lib.check(model.lib.ttk_ar_reorder_cache_lines(model._h, idx.data_ptr(), ROWS, _lib.stream_ptr()), "ttk_ar_reorder_cache_lines")
	if after is not None:
		model._decode(after.to(DEV).contiguous(), logits)
	torch.cuda.synchronize()
	return logits.cpu()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reorder_in_lines_mode_equals_feeding_the_permuted_histories(dtype):
	beam_idx = [1, 0, 2, 5, 5, 3]
	perm = torch.randperm(8000, generator=torch.Generator().manual_seed(5))
	hist, nxt = perm[:2 * ROWS * 3].view(2 * ROWS, 3), perm[100:100 + 2 * ROWS]                 # distinct tokens per row and step
	a, b = make_ar(dtype), make_ar(dtype)
	got = _run_lines(a, hist, reorder=beam_idx, after=nxt)
	want = _run_lines(b, hist[beam_idx], after=nxt)                                           # row r was fed row beam_idx[r]'s history from the start
	assert torch.equal(bits(got), bits(want)), (got - want).abs().max()
	plain = _run_lines(b, hist, after=nxt)
	assert not torch.equal(got[0], plain[0]) and not torch.equal(got[4], plain[4])            # (the reorder did something, in both lines)
	assert torch.equal(bits(got[2]), bits(plain[2]))                                          # (and left a fixed point alone)
	same = _run_lines(a, hist, reorder=list(range(2 * ROWS)), after=nxt)                      # identity: as if the call had not been made
	assert torch.equal(bits(same), bits(plain))
	crossing = _run_lines(a, hist, reorder=[1, 0, 3, 5, 5, 3], after=nxt)                     # entry 2 names a row of the other line: nothing moves
	assert torch.equal(bits(crossing), bits(plain))
	crossing = _run_lines(a, hist, reorder=[1, 0, 2, 2, 5, 3], after=nxt)
	assert torch.equal(bits(crossing), bits(plain))


def test_reorder_lines_is_refused_without_a_lines_prefill():
	m = make_ar("f32")
	idx = torch.arange(2 * ROWS, dtype=torch.long, device=DEV)
	call = lambda rows: m.lib.ttk_ar_reorder_cache_lines(m._h, idx.data_ptr(), rows, _lib.stream_ptr())
	assert call(ROWS) == E_STATE                                                              # no prefill at all
	m._prefill(cond_latent(), texts_of([9], 1)[0], 2 * ROWS)
	assert call(ROWS) == E_STATE                                                              # one line's prefill
	m._prefill_lines(cond_latent(), texts_of([9, 5], 1), ROWS)
	assert call(2) == E_STATE                                                                 # lines of another row count
	assert call(ROWS) == 0
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the beam step alone
class _Beam:
	"""the arrays of ttk_beam_args for G lines of N beams (G = None: the arrays of ttk_beam_step, without the leading dimension)"""
	NAMES = ("col", "seqs", "scores", "state", "tok", "beam_idx")

	def __init__(self, G, N, max_new, kw):
		lead = () if G is None else (G,)
		rows = N * (G or 1)
		self.G, self.N = G, N
		self.logits = torch.empty((rows, V), device=DEV)
		self.q = torch.empty(lead + (N * V,), device=DEV)
		self.col = torch.zeros(lead + (N,), dtype=torch.long, device=DEV)
		self.seqs = torch.full(lead + (2, 2, N, max_new), STOP, dtype=torch.long, device=DEV)
		self.scores = torch.full(lead + (2, N), -1e9, device=DEV)
		self.scores[..., 0, 0] = 0.0
		self.state = torch.zeros(lead + (2 * N + 2,), dtype=torch.int32, device=DEV)
		self.state[..., 2 * N] = 1
		self.acc = torch.empty(lead + (N * V,), device=DEV)
		self.work = torch.zeros(lead + (4 * N * N + 2 * N + 1,), dtype=torch.int32, device=DEV)
		self.tok = torch.zeros(rows, dtype=torch.long, device=DEV)
		self.beam_idx = torch.zeros(rows, dtype=torch.long, device=DEV)
		self.done = torch.zeros(1, dtype=torch.int32, device=DEV)
		a = _lib.BeamArgs()
		a.logits, a.ld, a.num_beams, a.V, a.q = self.logits.data_ptr(), V, N, V, self.q.data_ptr()
		a.temperature, a.top_k, a.top_p = kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0)
		a.repetition_penalty, a.length_penalty = kw.get("repetition_penalty", 1.0), kw.get("length_penalty", 1.0)
		a.stop_token, a.max_new = STOP, max_new
		a.prefix_ids[0], a.prefix_ids[1] = 1, CFG.start_mel_token
		a.col, a.seqs, a.scores, a.state = self.col.data_ptr(), self.seqs.data_ptr(), self.scores.data_ptr(), self.state.data_ptr()
		a.acc, a.work, a.tok, a.beam_idx = self.acc.data_ptr(), self.work.data_ptr(), self.tok.data_ptr(), self.beam_idx.data_ptr()
		a.all_done = self.done.data_ptr()
		self.args = a

	def step(self, lib):
		if self.G is None:
			_lib.check(lib.ttk_beam_step(_lib.C.byref(self.args), _lib.stream_ptr()), "ttk_beam_step")
		else:
			_lib.check(lib.ttk_beam_step_lines(_lib.C.byref(self.args), self.G, _lib.stream_ptr()), "ttk_beam_step_lines")
		torch.cuda.synchronize()

	def words(self, g=None):
		"""the state words of line g (of the single line: g None), tok and beam_idx as that line's N entries"""
		N = self.N
		out = {}
		for name in self.NAMES:
			t = getattr(self, name)
			if name in ("tok", "beam_idx"):
				t = t if g is None else t[g * N:(g + 1) * N]
			else:
				t = t if g is None else t[g]
			out[name] = bits(t).clone()
		return out


@pytest.mark.parametrize("biases", [(14.0, 7.5, 0.0), (7.5,)], ids=["G3", "G1"])
def test_step_lines_leaves_on_every_line_the_state_of_its_own_step(biases):
	lib = _lib.load()
	G, N, steps = len(biases), 4, 4
	max_new = steps
	kw = dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=2.0, length_penalty=2.0)
	gen = torch.Generator().manual_seed(21)
	table = torch.randn(steps, G, N, V, generator=gen) * 2.0
	for g, bias in enumerate(biases):
		table[:, g, :, STOP] += bias                              # a line whose stop token is likelier ends sooner
	torch.manual_seed(0); torch.cuda.manual_seed_all(0)
	batch, single = _Beam(G, N, max_new, kw), [_Beam(None, N, max_new, kw) for _ in range(G)]
	ident = torch.arange(N, device=DEV)
	ended, frozen = [0] * G, [None] * G
	for k in range(steps + 1):                                     # (one call more than any line can take)
		if k < steps:
			batch.logits.copy_(table[k].reshape(G * N, V))
			noise = torch.empty((1, N * V), device=DEV).exponential_(1)
			batch.q.copy_(noise.expand(G, -1))                    # every line draws the flat tensor of its own call
		batch.step(lib)
		was_done = int(batch.done[0])
		for g in range(G):
			got = batch.words(g)
			if ended[g]:                                          # a line that has ended: later calls change none of its words
				assert all(torch.equal(got[n], frozen[g][n]) for n in got), (k, g)
				continue
			if k < steps:
				single[g].logits.copy_(table[k, g])
				single[g].q.copy_(noise[0])
			single[g].step(lib)
			want = single[g].words()
			over = int(want["state"][2 * N + 1])
			for name in ("col", "seqs", "scores", "state"):
				assert torch.equal(got[name], want[name]), (k, g, name)
			if over:                                              # the step that ends the line: stop tokens and the identity for the launches that go on
				assert over == k + 1
				assert (got["tok"] == STOP).all() and torch.equal(got["beam_idx"] - g * N, ident), (k, g)
				ended[g], frozen[g] = k + 1, got
			else:
				assert torch.equal(got["tok"], want["tok"]) and torch.equal(got["beam_idx"] - g * N, want["beam_idx"]), (k, g)
		# the done word: non-zero exactly from the step that ends the last line
		assert bool(was_done) == all(ended), (k, ended, was_done)
	print(f"\n[beam step lines G={G}] lines ended after {ended} steps")
	assert all(ended) and max(ended) <= steps
	if G > 1:
		assert len(set(ended)) > 1, ended                         # lines ended at different steps: finished ones rode along


# ------------------------------------------------------------------------------------------------ the loop
TEXT_LENS = (5, 9, 7)
# text seeds per case of tests/test_gpu_beam.py's LOOP_CASES, chosen on the device (the noise is drawn there) so that the lines' searches end at different steps
# where they can: f32 and bf16 alike, the own calls of the three lines take 7 / 5 / 6 steps and 5 / 3 / 5 steps in the first two cases.  In the other two
# every line runs to max_generate_length whatever the text (no stop bias; length_penalty 2 with these weights): they cover the end at the limit
TEXT_SEEDS = {"four_beams_two_returned": 5, "two_beams_warpers": 1, "length_penalty": 1, "runs_to_max_length": 1}
ENDS_EARLY = ("four_beams_two_returned", "two_beams_warpers")
SAMPLED = dict(do_sample=True, num_return_sequences=3, max_generate_length=10, temperature=0.8, top_k=0)


def biased_sd(bias):
	sd = W.synth_state_dict(W.ar_shapes(CFG), 11)
	sd["mel_head.bias"] = sd["mel_head.bias"].clone()
	sd["mel_head.bias"][STOP] += bias                             # makes beams finish before max_generate_length
	return sd


@pytest.mark.parametrize("own", ["1", "0"], ids=["head_noise", "torch_noise"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_beam_search_lines_equals_the_per_line_calls(name, dtype, own, monkeypatch):
	monkeypatch.setenv("TTK_AR_OWN_RNG", own)
	bias, kw = LOOP_CASES[name]
	kw = dict(kw)
	N = kw.pop("num_beams")
	sd = biased_sd(bias)
	model = make_ar(dtype, sd=sd)
	cond, texts = cond_latent(), texts_of(TEXT_LENS, TEXT_SEEDS[name])
	gen = torch.cuda.default_generators[0]
	with_more = name == "four_beams_two_returned" and dtype == "f32" and own == "1"
	with torch.inference_mode():
		if with_more:
			sampled = model.inference_speech_lines(cond, texts, **SAMPLED)
		want, steps, after = [], [], []
		for t in texts:
			want.append(model.inference_speech(cond, t, do_sample=True, num_beams=N, **kw))
			steps.append(model.last_generate["steps"])
			off_last = gen.get_offset()
			after.append(torch.rand(3, device=DEV))
		got = model.beam_search_lines(cond, texts, N, **kw)
		off_got = gen.get_offset()
		print(f"\n[beam lines {name} {dtype} own_rng={own}] steps per line {steps}, shapes {[tuple(w.shape) for w in want]}")
		assert len(got) == len(texts)
		for g, (a, b) in enumerate(zip(got, want)):
			assert a.shape == b.shape and torch.equal(a, b), (g, "first divergence per row", first_divergence(a.cpu(), b.cpu()), a.tolist(), b.tolist())
			assert model.last_generate_lines[g]["steps"] == steps[g], g
		assert off_got == off_last                                # the generators where the last line's own call leaves them
		for g in range(len(texts)):
			model.position_rng_after_line(g)
			assert torch.equal(torch.rand(3, device=DEV), after[g]), g
		if name in ENDS_EARLY:                                    # the searches end at different steps, all before the limit: finished lines rode along
			assert len(set(steps)) > 1 and min(steps) < max(steps) < kw["max_generate_length"], steps
		else:
			assert set(steps) == {kw["max_generate_length"]}, steps
		if with_more:
			# against the restated HF loop per line as well (tests/beam_ref.py), and the sampling path right after on the same handle: its ids are what they were
			oracle = O.AROracle(sd, CFG)
			for g, t in enumerate(texts):
				ref = BR.beam_search(oracle, cond.cpu(), t.cpu(), sample_device=DEV, num_beams=N, **kw)
				assert torch.equal(got[g].cpu(), ref), g
			again = model.inference_speech_lines(cond, texts, **SAMPLED)
			assert all(torch.equal(x, y) for x, y in zip(again, sampled))


# ------------------------------------------------------------------------------------------------ orchestration
def test_inference_lines_and_tts_with_beam_width(parts):  # noqa: F811
	tts, sd, norms = parts
	enc = tts.encode_audio(speechlike(9, 30000, 22050).to(DEV), 22050)
	al, dl = enc["latent"]
	kw = dict(max_ar_steps=10, max_diffusion_steps=3, candidates=2, beam_width=2)
	text = "Hello there.\nThe end!"
	lines = [tts.encode_text(t).to(DEV)[None] for t in text.split("\n")]
	single = [tts.hot.inference(t, al, dl, return_all=True, **kw) for t in lines]
	batch = tts.hot.inference_lines(lines, al, dl, **kw)
	assert len(batch) == len(lines)
	for (mels, seconds, codes), (want_mels, want_seconds, aux) in zip(batch, single):
		assert codes.shape == aux["codes"].shape and torch.equal(codes, aux["codes"])
		assert mels.shape == want_mels.shape and torch.equal(bits(mels), bits(want_mels)) and seconds == want_seconds
	out, sr = tts.inference(text, enc, seed=1234, **kw)
	by_hand = torch.concat([tts.hot.inference_to_wav(t, al, dl, **kw)[0] for t in lines], dim=-1)
	assert sr == 24000 and out.shape == by_hand.shape and torch.equal(bits(out), bits(by_hand))
	with pytest.raises(ValueError, match="num_return_sequences"):
		tts.inference(text, enc, beam_width=2, max_ar_steps=10, max_diffusion_steps=3, candidates=3)
