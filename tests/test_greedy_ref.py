"""Greedy search, CPU side: the restated HF `_sample(do_sample=False)` (tests/greedy_ref.py) against the ids of the installed HuggingFace loop on the
model-free stub (tests/golden/hf_greedy_loop.npz, written by tools/make_golden_greedy.py) and, when transformers is importable, against that loop
live; what the fixture's cases cover; the argument checks of the product's greedy path that need no device; and the two new entry points' place in
the header, the ctypes table and the built library."""
import ctypes
import json
import os
import re
import types

import pytest
import torch

import greedy_ref as GR
import stub_lm
from tortoise_tts_amd import weights as W

NAMES = [c[0] for c in GR.CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", NAMES)
def test_restated_greedy_search_equals_huggingface_on_stub_model(golden, name):
	g = golden("hf_greedy_loop")
	ids, (seed, bias, L, kw) = GR.stub_case(name)
	assert json.loads(str(g["kw::" + name])) == json.loads(json.dumps(dict(seed=seed, stop_bias=bias, max_generate_length=L, kwargs=kw)))
	want = torch.from_numpy(g["ids::" + name])
	assert ids.shape == want.shape and torch.equal(ids, want), (ids.tolist(), want.tolist())
	pytest.importorskip("transformers")
	assert torch.equal(GR.hf_case(name), want)                # live: the loop the fixture came from


def test_fixture_covers_max_length_an_early_stop_the_penalty_the_suppressed_stop_and_ignored_warpers(golden):
	g = golden("hf_greedy_loop")
	ids = {n: torch.from_numpy(g["ids::" + n]) for n in NAMES}
	L = {c[0]: c[3] for c in GR.CASES}
	stop = stub_lm.STOP
	assert ids["runs_to_max_length"].shape == (1, L["runs_to_max_length"]) and not bool((ids["runs_to_max_length"] == stop).any())
	early = ids["stops_early"]
	assert 1 < early.shape[1] < L["stops_early"] and int(early[0, -1]) == stop and not bool((early[0, :-1] == stop).any())
	# the penalty decides: the same table without it gives other ids
	seed, bias, Lp, kw = next(c[1:] for c in GR.CASES if c[0] == "repetition_penalty")
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(seed, bias))
	text = torch.zeros(1, stub_lm.PREFIX - 3, dtype=torch.long)
	plain = GR.greedy_search(ar, torch.zeros(1, 1), text, max_generate_length=Lp)
	assert plain.shape != ids["repetition_penalty"].shape or not torch.equal(plain, ids["repetition_penalty"])
	sup = ids["suppress_stop"]
	assert sup.shape == (1, L["suppress_stop"]) and not bool(torch.isin(sup, torch.tensor([stop, 5, 17])).any())
	# suppressing the stop token decides as well: without the mask this table ends early
	seed, bias, Ls, _ = next(c[1:] for c in GR.CASES if c[0] == "suppress_stop")
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(seed, bias))
	assert GR.greedy_search(ar, torch.zeros(1, 1), text, max_generate_length=Ls).shape[1] < Ls
	# temperature, top_k and top_p play no part: HF's ids with them are the restated ids without them
	seed, bias, Li, kw = next(c[1:] for c in GR.CASES if c[0] == "ignored_warpers")
	assert set(kw) == {"temperature", "top_k", "top_p"}
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(seed, bias))
	assert torch.equal(GR.greedy_search(ar, torch.zeros(1, 1), text, max_generate_length=Li), ids["ignored_warpers"])


def test_ties_go_to_the_lowest_index_in_the_restatement():
	s = torch.full((2, 10), -1.0)
	s[0, [7, 3, 9]] = 2.0
	s[1] = -float("inf")
	assert GR.argmax_lowest(s).tolist() == [3, 0]


def _bare_model(max_batch=8):
	"""a UnifiedVoice without a device handle (as tests/test_beam_ref.py builds one): every check below is raised before the first device call"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	m = object.__new__(UnifiedVoice)
	m.cfg, m.max_batch, m.max_ctx, m._streaming, m.hf_exact_top_p = W.AR_SMALL, max_batch, 128, False, False
	m.device = torch.device("cuda:0")
	return m


def test_more_than_one_returned_sequence_is_hfs_value_error():
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(1, 0.0))
	with pytest.raises(ValueError, match="num_return_sequences"):
		GR.greedy_search(ar, torch.zeros(1, 1), torch.zeros(1, 9, dtype=torch.long), num_return_sequences=2, max_generate_length=4)
	m = _bare_model()
	cond, text = torch.zeros(1, 128), torch.ones(1, 5, dtype=torch.long)
	with pytest.raises(ValueError, match="num_return_sequences"):
		m.inference_speech(cond, text, num_return_sequences=2)                                 # do_sample omitted: greedy
	with pytest.raises(ValueError, match="num_return_sequences"):
		m.inference_speech(cond, text, do_sample=False, num_return_sequences=2)
	with pytest.raises(ValueError, match="num_return_sequences"):
		m.inference_speech_lines(cond, [text, text], do_sample=False, num_return_sequences=2)
	with pytest.raises(ValueError, match="candidate_shard"):
		m.inference_speech(cond, text, do_sample=False, candidate_shard=(0, 2))                 # one candidate: only (0, 1) is a range inside it


def test_orchestration_refusals_need_no_device():
	from tortoise_tts_amd.inference import TTSHotPath
	from tortoise_tts_amd.tts import TTS
	stub = types.SimpleNamespace(device=torch.device("cuda:0"))
	tts = TTS(stub, None, None, hifigan=object())
	voice = {"latent": (None, None)}
	with pytest.raises(ValueError, match="candidates"):
		tts.inference("Hello.", voice, do_sample=False, candidates=2)
	with pytest.raises(ValueError, match="beam_width"):
		tts.inference("Hello.", voice, do_sample=False, beam_width=2)
	with pytest.raises(NotImplementedError, match="greedy"):
		tts.inference("Hello.", voice, do_sample=False, vocoder_type="hifigan")
	hot = TTSHotPath(stub, types.SimpleNamespace(in_tokens=0))
	text = torch.ones(1, 5, dtype=torch.long)
	with pytest.raises(ValueError, match="candidates"):
		hot.inference(text, None, None, do_sample=False, candidates=2)
	with pytest.raises(ValueError, match="beam_width"):
		hot.inference(text, None, None, do_sample=False, beam_width=2)
	with pytest.raises(ValueError, match="candidates"):
		hot.inference_lines([text, text], None, None, do_sample=False, candidates=2)


def test_ignored_warpers_get_one_warning_that_names_them():
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	with pytest.warns(UserWarning, match="temperature=0.5.*top_k=5.*top_p=0.5") as rec:
		UnifiedVoice._warn_ignored_warpers(dict(temperature=0.5, top_k=5, top_p=0.5, repetition_penalty=2.0))
	assert len(rec) == 1
	import warnings
	with warnings.catch_warnings():
		warnings.simplefilter("error")
		UnifiedVoice._warn_ignored_warpers(dict(repetition_penalty=2.0, temperature=1.0))      # nothing that greedy search ignores was set


def test_the_greedy_flag_is_part_of_the_state_key_and_the_ignored_warpers_are_not():
	m = _bare_model()
	kw = dict(temperature=0.5, top_k=5, top_p=0.5, repetition_penalty=2.0, suppress_tokens=[3])
	sampling, _ = m._pipe_key(kw, None)
	greedy, can_stop = m._pipe_key(kw, None, True)
	assert sampling != greedy and greedy[6] is True and sampling[6] is False and can_stop
	assert greedy == m._pipe_key(dict(repetition_penalty=2.0, suppress_tokens=[3]), None, True)[0]
	assert not m._pipe_key(dict(suppress_tokens=[W.AR_SMALL.stop_mel_token]), None, True)[1]


def test_entry_points_are_declared_listed_and_exported():
	from tortoise_tts_amd import _lib
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_\w+)\s*\(", header))
	new = ("ttk_greedy_step", "ttk_ar_greedy_next")
	assert set(new) <= declared and set(new) <= set(_lib.SYMBOLS)
	assert re.search(r"int ttk_greedy_step\(const ttk_sample_args\* a, void\* stream\);", header)
	assert re.search(r"int ttk_ar_greedy_next\(ttk_ar\* h, const ttk_sample_args\* a, void\* stream\);", header)
	assert len(_lib.SYMBOLS["ttk_greedy_step"][1]) == 2 and len(_lib.SYMBOLS["ttk_ar_greedy_next"][1]) == 3
	assert _lib.SYMBOLS["ttk_ar_greedy_next"] == _lib.SYMBOLS["ttk_ar_sample_next"] and _lib.SYMBOLS["ttk_greedy_step"] == _lib.SYMBOLS["ttk_sample_step_warped"]
	assert "lowest index" in header.lower()          # the tie rule is stated where the entry is declared
	_lib.build()
	lib = ctypes.CDLL(_lib.LIB_PATH)
	assert all(hasattr(lib, s) for s in new)
