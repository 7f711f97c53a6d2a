"""The reference's samplers on the device: the second token-step kernel (include/ttk.h: ttk_sample_ext, ttk_sample_step_ext / ttk_ar_sample_next_ext;
csrc/sample_ext.hip) against ttk_sample_step_warped with every field off and against the restatement of tests/samplers_ref.py with each of them on, and
the keywords of `UnifiedVoice.inference_speech` / `get_generator` on small synthetic models.

Bounds.  Penalised scores: 2 ulp (the device's pow may sit one ulp from libm's before the cast to f32, and the cast reciprocal then moves the product by at
most one more).  temp_out: 1e-5 relative (an f32 tree sum of at most 9216 exponentials is within about 1e-6 of the f64 sum, and |dT/dp| <= 2.5 (T - T_min));
the scaled scores 1 ulp of scores * (1.0f / temp_out).  Mirostat: k and the token equal the restatement's under the same noise, mu 1e-6 relative -- on
inputs whose unrounded k stays at least 0.02 from a half-integer at every step, which every such test asserts on the restatement itself (the seeds below were
checked on the CPU; a seed that breaks the condition fails loudly, no row is ever left out)."""
import numpy as np
import pytest
import torch

import samplers_ref as SR
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = W.AR_SMALL
STOP = CFG.stop_mel_token
SHAPES = [(16, 8194), (3, 8194), (16, 1000), (16, 9216)]
MARGIN = 0.02


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load()


class _Step:
	"""device state of a token step as a caller of ttk_sample_step_ext holds it: ttk_sample_args, ttk_sample_ext and the optional outputs"""

	def __init__(self, B, V, steps, off, stop, prompt=None, **ext):
		from tortoise_tts_amd import _lib
		self.B, self.V, self.off = B, V, off
		self.unf = torch.ones(B, dtype=torch.long, device=DEV)
		self.tok = torch.full((B,), -1, dtype=torch.long, device=DEV)
		self.ids = torch.full((B, steps), -1, dtype=torch.long, device=DEV)
		self.col = torch.zeros(B, dtype=torch.long, device=DEV)
		self.hist = torch.ones((B, off + steps), dtype=torch.long, device=DEV)
		self.hist[:, off - 1] = 8192
		if prompt is not None:                                  # prompt columns: filled id columns in front of the first sampled token
			n0 = prompt.shape[1]
			self.ids[:, :n0] = prompt.to(DEV)
			self.hist[:, off:off + n0] = prompt.to(DEV)
			self.col.fill_(n0)
		self.q = torch.empty((B, V), device=DEV)
		self.mu = torch.full((B,), 2.0 * ext.get("mirostat_tau", 0.0), dtype=torch.float64, device=DEV)
		self.k = torch.full((B,), -1, dtype=torch.int32, device=DEV)
		self.temp = torch.full((B,), -1.0, device=DEV)
		self.scores_out = torch.full((B, V + 3), 7.0, device=DEV)       # (a leading dimension above V; the padding must stay untouched)
		a = _lib.SampleArgs()
		a.ld, a.B, a.V, a.q, a.ldq = V, B, V, self.q.data_ptr(), V
		a.temperature, a.top_k, a.top_p, a.repetition_penalty = 1.0, 0, 1.0, 1.0
		a.stop_token, a.unfinished, a.tok, a.ids, a.ids_ld, a.ids_cols, a.col = stop, self.unf.data_ptr(), self.tok.data_ptr(), self.ids.data_ptr(), steps, steps, self.col.data_ptr()
		a.history, a.hist_ld, a.hist_off = self.hist.data_ptr(), self.hist.stride(0), off
		x = _lib.SampleExt()
		x.min_temperature = -1.0
		x.mirostat_mu, x.mirostat_k, x.temp_out = self.mu.data_ptr(), self.k.data_ptr(), self.temp.data_ptr()
		x.scores_out, x.scores_out_ld = self.scores_out.data_ptr(), self.scores_out.stride(0)
		for name, v in ext.items():
			setattr(x, name, v)
		self.args, self.ext = a, x

	def launch(self, lib, scores, entry="ttk_sample_step_ext"):
		from tortoise_tts_amd import _lib
		self.args.scores = scores.data_ptr()
		if entry == "ttk_sample_step_ext":
			_lib.check(lib.ttk_sample_step_ext(_lib.C.byref(self.args), _lib.C.byref(self.ext), _lib.stream_ptr()), entry)
		else:
			_lib.check(lib.ttk_sample_step_warped(_lib.C.byref(self.args), _lib.stream_ptr()), entry)


def ulp_distance(a, b):
	def key(x):
		i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
		return np.where(i < 0, -(i & 0x7fffffff), i)
	return np.abs(key(a) - key(b))


def same_scores(got, want, ulps):
	"""-inf in the same places, finite entries within `ulps` f32 steps"""
	gi, wi = np.isneginf(got), np.isneginf(want)
	assert np.array_equal(gi, wi), (int(gi.sum()), int(wi.sum()))
	d = ulp_distance(got[~gi], want[~wi])
	assert d.size == 0 or int(d.max()) <= ulps, int(d.max())
	return int(d.max()) if d.size else 0


# ------------------------------------------------------------------------------------------------ 1. every field off == ttk_sample_step_warped
ALL_OFF = [((0.8, 16, 1.0, 1.0, 0.0), (16, 8194)), ((0.7, 16, 0.9, 2.0, 0.0), (16, 8194)), ((1.3, 50, 0.5, 1.2, 0.0), (16, 8194)), ((0.8, 0, 1.0, 2.0, 0.6), (16, 8194)),
		   ((0.7, 16, 0.9, 2.0, 0.0), (3, 8194)), ((0.7, 16, 0.9, 2.0, 0.0), (16, 1000)), ((0.7, 16, 0.9, 2.0, 0.0), (16, 9216))]


@pytest.mark.parametrize("warp,shape", ALL_OFF)
def test_every_field_off_equals_the_warped_step_bit_for_bit(lib, warp, shape):
	"""ids, history, col, unfinished, the done word and the generator state behind 8 steps, over the warper combinations of
	test_warpers_inside_the_sampling_kernel_equal_the_torch_op_chain (and one with the typical warper), with rows that finish on the way"""
	temp, top_k, top_p, pen, mass = warp
	B, V = shape
	steps, off, stop = 8, 2, V - 1
	g = torch.Generator().manual_seed(int(temp * 100) + top_k + V)
	logits = [(torch.randn((B, V), generator=g) * 4).to(DEV) for _ in range(steps)]
	for n, lg in enumerate(logits):
		lg[:, :40] += 5.0                                      # dominant ids: the penalty meets repeats
		if n >= 3:
			lg[: B // 2, stop] += 40.0                           # half of the rows finish with the fourth token
	mask = torch.zeros(V, dtype=torch.bool, device=DEV)
	mask[7] = True
	runs = []
	for entry in ("ttk_sample_step_warped", "ttk_sample_step_ext"):
		torch.manual_seed(3); torch.cuda.manual_seed_all(3)
		st = _Step(B, V, steps, off, stop)
		live = torch.full((1,), B, dtype=torch.int32, device=DEV)
		done = torch.zeros(1, dtype=torch.int32, device=DEV)
		a = st.args
		a.suppress, a.temperature, a.top_k, a.top_p, a.repetition_penalty, a.typical_mass = mask.data_ptr(), temp, top_k, top_p, pen, mass
		a.live_rows, a.all_done = live.data_ptr(), done.data_ptr()
		for lg in logits:
			st.q.exponential_(1)
			st.launch(lib, lg, entry)
		torch.cuda.synchronize()
		runs.append((st.ids, st.hist, st.col, st.unf, st.tok, live, done, torch.rand(4, device=DEV), st))
	for x, y in zip(runs[0][:8], runs[1][:8]):
		assert torch.equal(x, y)
	assert int(runs[1][3].sum()) < B and bool((runs[1][0] >= 0).all())
	st = runs[1][8]
	assert bool((st.temp == np.float32(temp)).all()) and bool((st.scores_out[:, V:] == 7.0).all()) and bool((st.k == -1).all())
	assert bool((st.mu == 0).all())                             # mirostat off: its state is not touched


# ------------------------------------------------------------------------------------------------ 2. decayed repetition penalty, stop-length penalty
@pytest.mark.parametrize("decay,stop_len,shape", [(0.5, 0.5, (16, 8194)), (-0.5, -0.5, (16, 8194)), (1.0, 0.0, (16, 8194)), (0.0, 0.5, (16, 8194)),
												  (0.5, -0.5, (3, 8194)), (0.5, -0.5, (16, 1000)), (0.5, -0.5, (16, 9216))])
def test_decayed_and_stop_length_penalties_equal_the_restatement_within_2_ulp(lib, decay, stop_len, shape):
	B, V = shape
	steps, off, stop, pen, temp = 10, 2, V - 1, 2.0, 0.75
	g = torch.Generator().manual_seed(int(decay * 10) + int(stop_len * 100) + V)
	prompt = torch.stack([torch.randint(2, 42, (2,), generator=g) for _ in range(B)])
	prompt[0, 1] = prompt[0, 0]                                 # a repeat inside the prompt columns
	st = _Step(B, V, steps, off, stop, prompt=prompt, repetition_penalty_decay=decay, stop_length_penalty=stop_len)
	st.args.temperature, st.args.repetition_penalty = temp, pen
	logits = [(torch.randn((B, V), generator=g) * 4) for _ in range(steps - 2)]
	worst, unpenalised_prefix = 0, 0
	for n, lg in enumerate(logits):
		lg[:, 2:42] += 6.0                                     # dominant ids: sampled tokens repeat at growing distances
		hist = st.hist.cpu().tolist()
		history = [row[:off + 2 + n] for row in hist]
		torch.manual_seed(5 + n); torch.cuda.manual_seed_all(5 + n)
		st.q.exponential_(1)
		want = SR.token_step(lg.numpy(), st.q.cpu().numpy(), history, off, temperature=temp, repetition_penalty=pen, repetition_penalty_decay=decay,
							 stop_length_penalty=stop_len, stop_token=stop)
		st.launch(lib, lg.to(DEV))
		torch.cuda.synchronize()
		got = st.scores_out[:, :V].cpu().numpy()
		worst = max(worst, same_scores(got, want["scores_out"], 2))
		inv = np.float32(1.0) / np.float32(temp)
		for b in range(B):
			previous = history[b][off:]
			assert len(previous) == 2 + n                       # two prompt columns, then the sampled tokens
			if decay != 0.0 and 1 not in previous:             # id 1 fills the prefix: not part of `previous`, so not penalised until it is sampled
				assert got[b, 1] == lg[b, 1].numpy() * inv
				unpenalised_prefix += 1
			if decay != 0.0:
				t = previous[-1]
				assert got[b, t] != lg[b, t].numpy() * inv      # the newest token is penalised at distance 1: divided by the factor itself
			if stop_len != 0.0 and stop not in previous:
				assert got[b, stop] != lg[b, stop].numpy() * inv      # length >= 3 here: the stop token's score moved (by how much: the 2-ulp comparison above)
	assert decay == 0.0 or unpenalised_prefix > 0
	hist = st.hist[:, off:].cpu()
	assert any(len(set(r)) < len(r) for r in hist.tolist())      # the histories did hold repeats
	print(f"\n[samplers] decay {decay} stop_len {stop_len} {shape}: largest distance {worst} ulp")


# ------------------------------------------------------------------------------------------------ 3. dynamic temperature
@pytest.mark.parametrize("shape", SHAPES)
def test_dynamic_temperature_hits_both_ends_and_the_slope_of_the_sigmoid(lib, shape):
	B, V = shape
	T, Tmin = SR.f32(0.8), SR.f32(0.1)
	g = torch.Generator().manual_seed(V + B)
	lg = torch.randn((B, V), generator=g) * 4
	for b in range(B):
		if b % 3 == 0:
			lg[b, (97 * b + 5) % V] += 60.0                      # peaked: p_max ~ 1
		elif b % 3 == 1:
			lg[b] *= 0.001                                       # flat: p_max ~ 1 / V
		else:
			j = (97 * b + 5) % V
			lg[b, j] = -1e9
			lg[b, j] = torch.logsumexp(lg[b].double(), 0).float()      # middle: as much mass as all the others together
	st = _Step(B, V, 1, 2, V + 5, min_temperature=Tmin)
	st.args.temperature = T
	st.q.exponential_(1)
	st.launch(lib, lg.to(DEV))
	torch.cuda.synchronize()
	temp = st.temp.cpu().numpy()
	got = st.scores_out[:, :V].cpu().numpy()
	for b in range(B):
		want = SR.dynamic_temperature_value(lg[b].numpy(), T, Tmin)
		frac = (T - want) / (T - Tmin)
		assert (frac > 0.99, frac < 0.01, 0.4 < frac < 0.6)[b % 3], (b, frac)
		assert abs(float(temp[b]) - want) <= 1e-5 * want, (b, temp[b], want)
		same_scores(got[b], lg[b].numpy() * (np.float32(1.0) / temp[b]), 1)
	with pytest.raises(Exception, match="min_temperature"):
		st.ext.min_temperature = 0.9
		st.launch(lib, lg.to(DEV))


# ------------------------------------------------------------------------------------------------ 4. mirostat
def miro_inputs(row_seeds, V, steps):
	"""fixed score tables and noise, one seed per row (a row's trajectory depends on nothing but its own tables, noise and mu), drawn on the CPU so that the
	restatement can be run on them without a device: (logits, q), each a list over the steps of [B, V] f32"""
	rows = []
	for seed in row_seeds:
		g = torch.Generator().manual_seed(seed)
		rows.append(((torch.randn((steps, V), generator=g) * 4).numpy(), torch.empty((steps, V)).exponential_(1, generator=g).numpy()))
	return [np.stack([r[0][n] for r in rows]) for n in range(steps)], [np.stack([r[1][n] for r in rows]) for n in range(steps)]


def miro_reference(logits, q, tau, eta, top_k=0):
	"""the restatement's loop with feedback; asserts the seed condition at every step of every row"""
	B = logits[0].shape[0]
	mu = np.full(B, 2.0 * tau)
	hist = [[1, 8192] for _ in range(B)]
	out = []
	for lg, qq in zip(logits, q):
		r = SR.token_step(lg, qq, hist, 2, mirostat_tau=tau, mirostat_eta=eta, mu=mu, top_k=top_k)
		if top_k == 0:
			margins = [SR.half_integer_margin(ku) for ku in r["k_unrounded"]]
			assert min(margins) >= MARGIN, ("the seed puts an unrounded k within 0.02 of a half-integer: choose another", margins)
		mu = r["mu"]
		for b in range(B):
			hist[b].append(int(r["tokens"][b]))
		out.append(r)
	return out


# Row seeds, checked on the CPU with the restatement (every row alone, then together): (tau, V, seeds).  Smallest half-integer margins found then: 0.039, 0.022,
# 0.18, 0.038, 0.041 for the single steps (k from 1 to 115 on these rows) and 0.020 for the loop, whose k runs from 1 up to the clamp at V as mu drifts.
MIRO_SINGLE = [(3.0, 8194, list(range(1000, 1016))), (5.0, 8194, [2000, 2001] + list(range(2003, 2017))), (5.0, 8194, [3000, 3001, 3002]),
			   (3.0, 1000, list(range(4000, 4007)) + list(range(4008, 4017))), (5.0, 9216, list(range(5000, 5013)) + [5014, 5015, 5016])]
MIRO_LOOP = (5.0, 24, [6002, 6007, 6009, 6010, 6015, 6017, 6018, 6020, 6022, 6024, 6028, 6032, 6035, 6039, 6040, 6042])


@pytest.mark.parametrize("tau,V,seeds", MIRO_SINGLE, ids=lambda v: str(len(v)) if isinstance(v, list) else str(v))
def test_mirostat_single_step_equals_the_restatement(lib, tau, V, seeds):
	B = len(seeds)
	eta = SR.f32(0.1)
	logits, q = miro_inputs(seeds, V, 1)
	want = miro_reference(logits, q, tau, eta)[0]
	st = _Step(B, V, 1, 2, V + 5, mirostat_tau=tau, mirostat_eta=eta)
	st.q.copy_(torch.from_numpy(q[0]))
	st.launch(lib, torch.from_numpy(logits[0]).to(DEV))
	torch.cuda.synchronize()
	assert st.k.cpu().tolist() == want["k"].tolist()
	assert st.tok.cpu().tolist() == want["tokens"].tolist()
	mu = st.mu.cpu().numpy()
	assert np.all(np.abs(mu - want["mu"]) <= 1e-6 * np.abs(want["mu"])) and np.all(mu != 2.0 * tau)
	kept = (st.scores_out[:, :V] > -float("inf")).sum(dim=1).cpu().tolist()
	assert kept == [V] * B                                      # scores_out is the row behind top-p, in front of mirostat's cut
	print(f"\n[samplers] mirostat tau {tau} B {B} V {V}: k {sorted(want['k'].tolist())}")


def test_mirostat_loop_with_feedback_equals_the_restatement_on_every_row(lib):
	tau, steps, seeds = MIRO_LOOP
	B, V, eta = len(seeds), 8194, SR.f32(0.1)
	logits, q = miro_inputs(seeds, V, steps)
	want = miro_reference(logits, q, tau, eta)
	st = _Step(B, V, steps, 2, V + 5, mirostat_tau=tau, mirostat_eta=eta)
	ks = []
	for lg, qq in zip(logits, q):
		st.q.copy_(torch.from_numpy(qq))
		st.launch(lib, torch.from_numpy(lg).to(DEV))
		ks.append(st.k.clone())
	torch.cuda.synchronize()
	ref_ids = np.stack([r["tokens"] for r in want], 1)
	ref_k = np.stack([r["k"] for r in want], 1)
	assert np.array_equal(st.ids.cpu().numpy(), ref_ids)
	assert np.array_equal(torch.stack(ks, 1).cpu().numpy(), ref_k)
	mu = st.mu.cpu().numpy()
	assert np.all(np.abs(mu - want[-1]["mu"]) <= 1e-6 * np.abs(want[-1]["mu"]))
	assert ref_k.min() >= 1 and len(np.unique(ref_k)) > 8           # the feedback moved k around
	print(f"\n[samplers] mirostat loop: k from {ref_k.min()} to {ref_k.max()}, final mu {mu.min():.3f} .. {mu.max():.3f}")


def test_fewer_than_101_survivors_keep_all_of_them_and_still_update_mu(lib):
	B, V, tau, eta = 16, 8194, 5.0, SR.f32(0.1)
	logits, q = miro_inputs(list(range(7000, 7000 + B)), V, 1)
	want = miro_reference(logits, q, tau, eta, top_k=50)[0]
	st = _Step(B, V, 1, 2, V + 5, mirostat_tau=tau, mirostat_eta=eta)
	st.args.top_k = 50                                         # (the Python surface refuses this combination; the C level defines it)
	st.q.copy_(torch.from_numpy(q[0]))
	lg = torch.from_numpy(logits[0]).to(DEV)
	st.launch(lib, lg)
	torch.cuda.synchronize()
	assert st.k.cpu().tolist() == [50] * B == want["k"].tolist()
	top50 = lg.topk(50, dim=1).indices
	assert bool((top50 == st.tok[:, None]).any(dim=1).all()) and st.tok.cpu().tolist() == want["tokens"].tolist()
	mu = st.mu.cpu().numpy()
	assert np.all(mu != 2.0 * tau) and np.all(np.abs(mu - want["mu"]) <= 1e-6 * np.abs(want["mu"]))


def test_ext_entry_refuses_what_it_cannot_do(lib):
	from tortoise_tts_amd import _lib
	wide = torch.zeros((1, 9217), device=DEV)

	def refused(st, scores, word):
		st.args.scores = scores.data_ptr()
		rc = lib.ttk_sample_step_ext(_lib.C.byref(st.args), _lib.C.byref(st.ext), _lib.stream_ptr())
		assert rc == -1 and word in lib.ttk_last_error(), (rc, lib.ttk_last_error())          # TTK_E_ARG, with a message
	st = _Step(1, 9217, 1, 2, 5)
	st.args.ld = st.args.ldq = 9217
	st.q = torch.ones((1, 9217), device=DEV)
	st.args.q = st.q.data_ptr()
	refused(st, wide, b"9216")
	st = _Step(1, 8194, 1, 2, 5, mirostat_tau=3.0)
	st.ext.mirostat_mu = None
	refused(st, wide, b"mirostat_mu")
	st = _Step(1, 8194, 1, 2, 5, mirostat_tau=3.0, mirostat_eta=-0.5)
	refused(st, wide, b"mirostat_eta")
	st = _Step(1, 8194, 1, 2, 5, min_temperature=1.5)
	refused(st, wide, b"min_temperature")
	for knob in (dict(repetition_penalty_decay=0.5), dict(stop_length_penalty=0.5)):
		st = _Step(1, 8194, 1, 2, 5, **knob)
		st.args.history = None
		refused(st, wide, b"history")
	assert lib.ttk_sample_step_ext(_lib.C.byref(st.args), None, _lib.stream_ptr()) == -1
	torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. the keywords on a small model
def make_ar(seed, edit=None, **kw):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	sd = W.synth_state_dict(W.ar_shapes(CFG), seed)
	if edit is not None:
		edit(sd)
	kw = dict(dict(max_batch=4, max_ctx=96), **kw)
	return UnifiedVoice(sd, CFG, dtype="f32", device=DEV, **kw)


def _bias(index, by):
	def edit(sd):
		sd["mel_head.bias"] = sd["mel_head.bias"].clone()
		sd["mel_head.bias"][index] += by
	return edit


def line(seed=1, n=9):
	text = torch.randint(1, 255, (1, n), generator=torch.Generator().manual_seed(seed))
	cond = torch.randn(1, CFG.model_dim, generator=torch.Generator().manual_seed(2))
	return cond.to(DEV), text.to(DEV)


# knob -> (weight seed, edit, the call without the knob, the knob).  Settings under which the knob decides, found with the restatement on the CPU oracle:
# four boosted codes dominate the rows (the decayed penalty and the dynamic temperature then act on what is drawn; mirostat cuts the row to a few
# tokens), a boosted stop token ends the plain call within ~13 tokens while dividing its score by length^2 lets the rows run on.
MODEL_CASES = {
	"repetition_penalty_decay": (12, _bias(slice(100, 104), 8.0), dict(temperature=0.8, top_k=0, repetition_penalty=2.0), dict(repetition_penalty_decay=1.0)),
	"stop_length_penalty": (18, _bias(STOP, 4.0), dict(temperature=0.8, top_k=4), dict(stop_length_penalty=2.0)),
	"min_temperature": (12, _bias(slice(100, 104), 8.0), dict(temperature=0.8, top_k=0), dict(min_temperature=0.1)),
	"mirostat_tau": (12, _bias(slice(100, 104), 4.0), dict(temperature=0.8, top_k=0), dict(mirostat_tau=3.0, mirostat_eta=0.1)),
}


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_each_keyword_on_a_small_model(lib, name):
	"""use_graph on and off give the same ids; they differ from the call without the keyword; a second call on the same handle repeats the first (mirostat's
	mu is reset); explicit defaults are the plain call, generator offset included; the streaming generator yields the same ids"""
	seed, edit, base, knob = MODEL_CASES[name]
	cond, text = line()
	gen = torch.cuda.default_generators[0]
	kw = dict(do_sample=True, num_return_sequences=4, max_generate_length=24, **base)
	got = {}
	for use_graph in (True, False):
		model = make_ar(seed, edit, use_graph=use_graph)
		torch.rand(7, device=DEV)
		plain = model.inference_speech(cond, text, **kw)
		off_plain, step_plain = gen.get_offset(), model.last_generate["rng_step"]
		explicit = model.inference_speech(cond, text, repetition_penalty_decay=0.0, stop_length_penalty=0.0, min_temperature=None, mirostat_tau=0.0, mirostat_eta=0.1, **kw)
		assert torch.equal(plain, explicit) and gen.get_offset() == off_plain and len(model._states) == 1
		ids = model.inference_speech(cond, text, **kw, **knob)
		steps, off = model.last_generate["steps"], gen.get_offset()
		assert model.last_generate["rng_step"] == step_plain == (off - model.last_generate["rng_start"]) // steps and steps == ids.shape[1]      # the plain draw's noise per token
		assert ids.shape != plain.shape or not torch.equal(ids, plain)
		again = model.inference_speech(cond, text, **kw, **knob)
		assert torch.equal(again, ids) and gen.get_offset() == off and len(model._states) == 2
		got[use_graph] = ids
	assert torch.equal(got[True], got[False])
	# the streaming generator: one row, the same keywords
	skw = dict(do_sample=True, **base, **knob)
	model = make_ar(seed, edit)
	ref = model.inference_speech(cond, text, num_return_sequences=1, max_generate_length=24, **skw)
	inputs = model.compute_embeddings(cond, text)
	toks = [t.clone() for t, _ in model.get_generator(inputs, max_length=inputs.shape[1] + 24, num_return_sequences=1, **skw)]
	assert torch.equal(torch.stack(toks, 1), ref)


def test_lines_with_a_keyword_are_sampled_line_by_line(lib):
	seed, edit, base, knob = MODEL_CASES["mirostat_tau"]
	model = make_ar(seed, edit)
	cond = line()[0]
	texts = [line(seed=20 + n, n=n)[1] for n in (5, 8)]
	kw = dict(do_sample=True, num_return_sequences=2, max_generate_length=12, **base, **knob)
	batch = model.inference_speech_lines(cond, texts, **kw)
	for g, t in enumerate(texts):
		assert torch.equal(batch[g], model.inference_speech(cond, t, **kw))
		assert model.last_generate_lines[g]["steps"] == batch[g].shape[1]
