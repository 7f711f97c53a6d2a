"""The reference's samplers, CPU side: the restatement the GPU tests compare the kernel with (tests/samplers_ref.py) against results of the reference's own
tortoise_tts/samplers.py (tests/golden/samplers_ref.npz, written by tools/make_golden_samplers.py; inputs regenerated from the stored seeds); the two new
entry points' place in the header, the ctypes table and the built library, with the struct sizes; and every refusal of the Python surface, on a model without a
device handle.

Bounds: penalised scores within 2 ulp -- the CPU reference divides (x / f32(c), one rounding), the restatement multiplies by the f32 reciprocal as ATen does
on a GPU (two roundings: 1.5 ulp at most); T_dyn 1e-12 relative (f64 on both sides; the sums of the exponentials differ in their order); mirostat's k exact;
mirostat's state 1e-12 after the reference's own token, given that token's f32 probability as the reference's softmax rounded it (the update is f64 arithmetic
on an f32 value; the restatement's own numpy softmax is separately held within 1e-5 of it, the rounding of an f32 denominator of 8194 terms)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import samplers_ref as SR
from tortoise_tts_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
	spec = importlib.util.spec_from_file_location("_make_golden_samplers", os.path.join(ROOT, "tools", "make_golden_samplers.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


TOOL = _tool()


def ulp_distance(a, b):
	"""distance in f32 representation steps (finite values)"""
	def key(x):
		i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
		return np.where(i < 0, -(i & 0x7fffffff), i)
	return np.abs(key(a) - key(b))


def test_fixture_holds_the_cases_the_tool_lists(golden):
	g = golden("samplers_ref")
	for fam, cases in (("pen", TOOL.PEN_CASES), ("len", TOOL.LEN_CASES), ("dyn", TOOL.DYN_CASES), ("miro", TOOL.MIRO_CASES)):
		assert np.array_equal(g[fam + "_params"], np.asarray(cases, dtype=np.float64))
	assert {c[3] for c in TOOL.PEN_CASES} >= {0.5, -0.5, 1.0} and {c[3] for c in TOOL.LEN_CASES} >= {0.5, -0.5}
	assert {int(c[4]) for c in TOOL.DYN_CASES} == {0, 1, 2} and {c[2] for c in TOOL.MIRO_CASES} == {3.0, 5.0}


@pytest.mark.parametrize("i", range(len(TOOL.PEN_CASES)))
def test_decayed_repetition_penalty_is_the_references_within_2_ulp(golden, i):
	g = golden("samplers_ref")
	c = TOOL.PEN_CASES[i]
	logits, previous = TOOL.case_inputs("pen", c)
	want = g[f"pen_out_{i}"]
	got = SR.decay_penalize(logits, previous.tolist(), c[2], c[3])
	touched = want != logits
	assert touched.sum() == len(set(previous.tolist())) and np.array_equal(got != logits, touched)      # one division per distinct token, nothing else moves
	assert int(ulp_distance(got, want).max()) <= 2
	# a division whatever the sign (HF's processor multiplies negative scores): negative scores move towards zero for a divisor above 1
	d = SR.latest_distances(previous.tolist())
	assert all(abs(got[t]) < abs(logits[t]) for t, dist in d.items() if c[2] * dist ** c[3] > 1)
	assert (logits[list(d)] < 0).any() and (logits[list(d)] > 0).any()


def test_latest_occurrence_decides_the_distance():
	assert SR.latest_distances([5, 7, 5, 9]) == {5: 2, 7: 3, 9: 1}
	s = SR.decay_penalize(np.ones(10, np.float32), [5, 7, 5, 9], 2.0, 1.0)
	assert s[5] == np.float32(0.25) and s[7] == np.float32(1 / 6) and s[9] == np.float32(0.5) and s[0] == 1
	assert np.array_equal(SR.decay_penalize(np.ones(10, np.float32), [5], 1.0, 0.5), np.ones(10, np.float32))      # factor 1: the reference returns early


@pytest.mark.parametrize("i", range(len(TOOL.LEN_CASES)))
def test_stop_length_penalty_is_the_references_within_2_ulp(golden, i):
	g = golden("samplers_ref")
	c = TOOL.LEN_CASES[i]
	logits, _ = TOOL.case_inputs("len", c)
	want = g[f"len_out_{i}"]
	got = SR.stop_length_penalize(logits, int(c[2]), c[3], int(c[4]))
	stop = int(c[4])
	assert np.array_equal(np.delete(got, stop), np.delete(logits, stop)) and np.array_equal(np.delete(want, stop), np.delete(logits, stop))
	assert int(ulp_distance(got[stop], want[stop])) <= 2
	assert (got[stop] != logits[stop]) == (int(c[2]) != 1)


@pytest.mark.parametrize("i", range(len(TOOL.DYN_CASES)))
def test_dynamic_temperature_is_the_references(golden, i):
	g = golden("samplers_ref")
	c = TOOL.DYN_CASES[i]
	logits, _ = TOOL.case_inputs("dyn", c)
	T, Tmin, kind = c[2], c[3], int(c[4])
	want = float(g["dyn_t"][i])
	got = SR.dynamic_temperature_value(logits, T, Tmin)
	assert abs(got - want) <= 1e-12 * abs(want)
	# the three kinds reach both ends and the slope of the sigmoid
	frac = (T - want) / (T - Tmin)
	assert (frac > 0.99, frac < 0.01, 0.4 < frac < 0.6)[kind]
	out = logits * (np.float32(1.0) / np.float32(got))
	assert int(ulp_distance(out, g[f"dyn_out_{i}"]).max()) <= 2


@pytest.mark.parametrize("i", range(len(TOOL.MIRO_CASES)))
def test_mirostat_k_and_state_are_the_references(golden, i):
	g = golden("samplers_ref")
	c = TOOL.MIRO_CASES[i]
	logits, _ = TOOL.case_inputs("miro", c)
	V, tau, eta, mu0 = int(c[1]), c[2], c[3], c[4]
	_, P = SR.softmax_f32(logits)
	k, ku = SR.mirostat_k(np.sort(P)[::-1][:SR.MIRO_N + 1], V, mu0)
	assert SR.half_integer_margin(ku) >= 0.02, ku                       # the case does not sit on a rounding boundary
	assert k == int(g["miro_k"][i])
	tok, p_ref = int(g["miro_token"][i]), g["miro_p_token"][i]
	assert tok in np.argsort(-logits, kind="stable")[:k]                # the reference drew among its k most likely
	# two f32 softmaxes of 8194 terms differ by the rounding of their denominators: about sqrt(n) 2^-24 ~ 5e-6 for a sum that carries f32 partial sums
	assert abs(float(P[tok]) - float(p_ref)) <= 1e-5 * float(p_ref)
	want = float(g["miro_mu"][i])
	got = SR.mirostat_update(mu0, p_ref, tau, eta)
	assert abs(got - want) <= 1e-12 * abs(want)


def test_mirostat_draw_keeps_the_k_most_likely_and_all_survivors_below_101():
	rs = np.random.RandomState(5)
	s = (rs.standard_normal(2000) * 4).astype(np.float32)
	q = np.ones(2000, np.float32)
	tok, k, mu, ku = SR.mirostat_draw(s, q, 10.0, 5.0, 0.125)
	assert tok == int(np.argmax(s)) and 1 <= k <= 2000 and np.isfinite(ku)      # flat noise: the most likely token
	q[np.argsort(-s)[k - 1]] = 1e-30                                              # the least likely kept token wins with a vanishing noise value ...
	assert SR.mirostat_draw(s, q, 10.0, 5.0, 0.125)[0] == int(np.argsort(-s)[k - 1])
	q[:] = 1
	q[np.argsort(-s)[k]] = 1e-30                                                  # ... the most likely removed one cannot
	assert SR.mirostat_draw(s, q, 10.0, 5.0, 0.125)[0] == int(np.argmax(s))
	few = SR.keep_top(s, 50)
	tok, k, mu2, ku = SR.mirostat_draw(few, np.ones(2000, np.float32), 10.0, 5.0, 0.125)
	assert k == 50 and np.isnan(ku) and mu2 != 10.0


def test_token_step_chains_the_stages_in_the_kernels_order():
	rs = np.random.RandomState(6)
	V, stop = 300, 299
	s = (rs.standard_normal((2, V)) * 4).astype(np.float32)
	q = rs.exponential(size=(2, V)).astype(np.float32)
	hist = [[1, 298, 4, 9, 4], [1, 298, 9, 9, 7]]
	r = SR.token_step(s, q, hist, 2, temperature=0.75, top_k=20, repetition_penalty=2.0, repetition_penalty_decay=0.5, stop_length_penalty=0.5, stop_token=stop)
	assert ((r["scores_out"] > -np.inf).sum(axis=1) == 20).all() and (r["temp"] == 0.75).all()
	inv = np.float32(1.0) / np.float32(0.75)
	for b in range(2):
		pen = SR.stop_length_penalize(SR.decay_penalize(s[b], hist[b][2:], 2.0, 0.5), 4, 0.5, stop)
		assert pen[1] == s[b, 1] and pen[298] == s[b, 298]                  # the prefix ids are not part of `previous`
		kept = r["scores_out"][b] > -np.inf
		assert np.array_equal(r["scores_out"][b][kept], (pen * inv)[kept])
	plain = SR.token_step(s, q, hist, 2, temperature=0.75, top_k=20, repetition_penalty=2.0, stop_token=stop)
	assert plain["scores_out"][0, 1] != (s[0, 1] * inv)                    # HF's processor penalises the prefix ids as well


# ---------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_listed_and_exported_and_the_struct_sizes_are_pinned():
	from tortoise_tts_amd import _lib
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_\w+)\s*\(", header))
	new = ("ttk_sample_step_ext", "ttk_ar_sample_next_ext")
	assert set(new) <= declared and set(new) <= set(_lib.SYMBOLS)
	assert re.search(r"int ttk_sample_step_ext\(const ttk_sample_args\* a, const ttk_sample_ext\* x, void\* stream\);", header)
	assert re.search(r"int ttk_ar_sample_next_ext\(ttk_ar\* h, const ttk_sample_args\* a, const ttk_sample_ext\* x, void\* stream\);", header)
	assert len(_lib.SYMBOLS["ttk_sample_step_ext"][1]) == 3 and len(_lib.SYMBOLS["ttk_ar_sample_next_ext"][1]) == 4
	assert ctypes.sizeof(_lib.SampleArgs) == 168 and ctypes.sizeof(_lib.SampleExt) == 64
	src = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "sample_ext.hip")).read()
	assert "static_assert(sizeof(ttk_sample_ext) == 64" in src
	assert "static_assert(sizeof(ttk_sample_args) == 168" in open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "sample.hip")).read()
	fields = re.search(r"typedef struct \{([^}]*)\} ttk_sample_ext;", header).group(1)
	names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
	assert names == [n for n, _ in _lib.SampleExt._fields_]
	_lib.build()
	lib = ctypes.CDLL(_lib.LIB_PATH)
	assert all(hasattr(lib, s) for s in new)


# ---------------------------------------------------------------------- the Python surface, without a device
def _bare_model(max_batch=8, **attrs):
	"""a UnifiedVoice without a device handle (as tests/test_greedy_ref.py builds one): every check below is raised before the first device call"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	m = object.__new__(UnifiedVoice)
	m.cfg, m.max_batch, m.max_ctx, m._streaming, m.hf_exact_top_p = W.AR_SMALL, max_batch, 128, False, False
	m.device = torch.device("cuda:0")
	for k, v in attrs.items():
		setattr(m, k, v)
	return m


KNOBS = (dict(repetition_penalty_decay=0.5, repetition_penalty=2.0), dict(stop_length_penalty=0.5), dict(min_temperature=0.2), dict(mirostat_tau=5.0))
COND, TEXT = torch.zeros(1, 128), torch.ones(1, 5, dtype=torch.long)


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: next(iter(k)))
def test_beams_and_shards_do_not_take_the_samplers(knob):
	m = _bare_model()
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech(COND, TEXT, do_sample=True, num_beams=2, top_k=0, **knob)
	with pytest.raises(NotImplementedError, match="candidate_shard"):
		m.inference_speech(COND, TEXT, do_sample=True, num_return_sequences=4, candidate_shard=(0, 2), top_k=0, **knob)


def test_greedy_search_refuses_the_samplers_each_for_its_reason():
	m = _bare_model()
	for knob in (dict(mirostat_tau=5.0), dict(min_temperature=0.2)):
		with pytest.raises(ValueError, match="samplers"):
			m.inference_speech(COND, TEXT, do_sample=False, **knob)
		with pytest.raises(ValueError, match="samplers"):
			m.inference_speech(COND, TEXT, **knob)                            # do_sample omitted: greedy
	for knob in (dict(repetition_penalty_decay=0.5, repetition_penalty=2.0), dict(stop_length_penalty=-0.5)):
		with pytest.raises(NotImplementedError, match="greedy"):
			m.inference_speech(COND, TEXT, do_sample=False, **knob)
	with pytest.raises(NotImplementedError, match="greedy"):
		m.inference_speech_lines(COND, [TEXT, TEXT], do_sample=False, stop_length_penalty=0.5)


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: next(iter(k)))
def test_hf_exact_top_p_and_wide_vocabularies_refuse_the_samplers(knob):
	import dataclasses
	m = _bare_model(hf_exact_top_p=True)
	with pytest.raises(NotImplementedError, match="hf_exact_top_p"):
		m.inference_speech(COND, TEXT, do_sample=True, top_k=0, top_p=0.9, **knob)
	with pytest.raises(NotImplementedError, match="hf_exact_top_p"):
		m.inference_speech(COND, TEXT, do_sample=True, top_k=0, typical_sampling=True, **knob)
	wide = _bare_model(cfg=dataclasses.replace(W.AR_SMALL, number_mel_codes=9217))
	with pytest.raises(NotImplementedError, match="9216"):
		wide.inference_speech(COND, TEXT, do_sample=True, top_k=0, **knob)


def test_mirostat_needs_101_tokens_behind_top_k_and_sane_parameters():
	m = _bare_model()
	with pytest.raises(ValueError, match="top_k=100"):
		m.inference_speech(COND, TEXT, do_sample=True, top_k=100, mirostat_tau=5.0)
	with pytest.raises(ValueError, match="top_k=50"):
		m.inference_speech(COND, TEXT, do_sample=True, mirostat_tau=5.0)      # an omitted top_k is HF's default 50
	with pytest.raises(ValueError, match="mirostat_eta"):
		m.inference_speech(COND, TEXT, do_sample=True, top_k=0, mirostat_tau=5.0, mirostat_eta=-0.1)
	with pytest.raises(ValueError, match="min_temperature"):
		m.inference_speech(COND, TEXT, do_sample=True, top_k=0, temperature=0.5, min_temperature=0.8)
	m._prefix = (COND, TEXT)
	with pytest.raises(ValueError, match="top_k=16"):
		m.get_generator(torch.ones(1, 9, dtype=torch.long), max_length=20, do_sample=True, top_k=16, mirostat_tau=3.0)


def test_the_knobs_follow_the_existing_entries_of_the_state_key_and_off_has_one_spelling():
	from tortoise_tts_amd.autoregressive import NO_KNOBS, pop_sampler_knobs
	m = _bare_model()
	kw = dict(temperature=0.5, top_k=5, top_p=0.5, repetition_penalty=2.0, suppress_tokens=[3])
	before, _ = m._pipe_key(kw, 0.9)
	assert before[:7] == (0.5, 5, 0.5, 2.0, (3,), 0.9, False) and before[7:] == NO_KNOBS
	kw2 = dict(kw, repetition_penalty_decay=0.5, stop_length_penalty=-0.5, min_temperature=0.1, mirostat_tau=3.0, mirostat_eta=0.25)
	knobs = pop_sampler_knobs(kw2)
	assert kw2 == kw and knobs == (0.5, -0.5, 0.1, 3.0, 0.25)
	assert m._pipe_key(kw, 0.9, False, knobs)[0] == before[:7] + knobs
	for off in (dict(), dict(min_temperature=None), dict(min_temperature=-1.0, mirostat_eta=0.7), dict(repetition_penalty_decay=None, mirostat_tau=0)):
		assert pop_sampler_knobs(dict(off)) == NO_KNOBS


def test_orchestration_signatures_carry_the_references_argument_names():
	import inspect
	from tortoise_tts_amd.inference import TTSHotPath, ar_sampler_knobs
	from tortoise_tts_amd.tts import TTS
	want = dict(min_ar_temp=None, repetition_penalty_decay=0.0, stop_length_penalty=0.0, mirostat_tau=0.0, mirostat_eta=0.1)
	for fn in (TTS.inference, TTS.hifigan_chunks, TTSHotPath.inference, TTSHotPath.inference_lines):
		params = inspect.signature(fn).parameters
		assert {k: params[k].default for k in want} == want, fn
	assert ar_sampler_knobs() == {} and ar_sampler_knobs(**want) == {}      # the default call hands on nothing: it is the call it was
	assert ar_sampler_knobs(min_ar_temp=0.2, mirostat_tau=3.0) == dict(min_temperature=0.2, mirostat_tau=3.0, mirostat_eta=0.1)
