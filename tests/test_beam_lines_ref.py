"""Beam search over a batch of lines, CPU side: the two C entries (ttk_beam_step_lines, ttk_ar_reorder_cache_lines) are declared, listed and exported, and the
argument checks and refusals of `UnifiedVoice.beam_search_lines` and `TTSHotPath.inference_lines(beam_width=)` are raised before the first device call (a
model without a handle, as in tests/test_beam_ref.py)."""
import ctypes
import os
import re
import types

import pytest
import torch

from test_beam_ref import _bare_model
from tortoise_tts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ttk_beam_step_lines", "ttk_ar_reorder_cache_lines")


def test_new_symbols_are_declared_listed_and_exported():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert set(NEW_SYMBOLS) <= declared and declared == set(_lib.SYMBOLS)
	assert len(_lib.SYMBOLS["ttk_beam_step_lines"][1]) == 3 and len(_lib.SYMBOLS["ttk_ar_reorder_cache_lines"][1]) == 4
	assert len(_lib.SYMBOLS["ttk_beam_step"][1]) == 2 and len(_lib.SYMBOLS["ttk_ar_reorder_cache"][1]) == 3      # the existing entries are not touched
	assert ctypes.sizeof(_lib.BeamArgs) == 168                                                                   # one struct for both steps
	lib = ctypes.CDLL(_lib.build())
	assert all(hasattr(lib, s) for s in NEW_SYMBOLS)


def _inputs():
	return torch.zeros(1, 128), [torch.ones(1, 5, dtype=torch.long), torch.ones(1, 7, dtype=torch.long)]


def test_argument_checks_need_no_device():
	m = _bare_model(max_batch=8)
	cond, texts = _inputs()
	with pytest.raises(ValueError, match=r"`num_return_sequences` \(3\) has to be smaller or equal to `num_beams` \(2\)"):
		m.beam_search_lines(cond, texts, 2, num_return_sequences=3)
	with pytest.raises(ValueError, match="top_k"):
		m.beam_search_lines(cond, texts, 4, top_k=7)                          # 0 < top_k < 2 * num_beams
	with pytest.raises(_lib.TTKError, match=r"3 lines x 4 beams exceed min\(16, max_batch=8\)"):
		m.beam_search_lines(cond, texts + texts[:1], 4, top_k=0)
	with pytest.raises(_lib.TTKError, match=r"2 lines x 9 beams exceed min\(16, max_batch=32\)"):
		_bare_model(max_batch=32).beam_search_lines(cond, texts, 9, top_k=0)
	with pytest.raises(ValueError, match="num_beams >= 2"):
		m.beam_search_lines(cond, texts, 1)
	with pytest.raises(NotImplementedError, match="list of"):
		m.beam_search_lines(cond, [torch.ones(2, 5, dtype=torch.long)], 2)


def test_refusals_name_beam_search():
	m = _bare_model(max_batch=8)
	cond, texts = _inputs()
	for kw in (dict(input_tokens=torch.ones(1, 2, dtype=torch.long)), dict(typical_sampling=True), dict(do_sample=False), dict(candidate_shard=(0, 1)),
			   dict(repetition_penalty_decay=0.5), dict(mirostat_tau=3.0, top_k=0), dict(min_temperature=0.3), dict(stop_length_penalty=1.0)):
		with pytest.raises(NotImplementedError, match="beam"):
			m.beam_search_lines(cond, texts, 2, **kw)
	with pytest.raises(NotImplementedError, match="beam_search_lines"):
		m.inference_speech_lines(cond, texts, do_sample=True, num_beams=2)      # the sampling entry points at the beam one


def test_inference_lines_beam_width_checks_need_no_device():
	from tortoise_tts_amd.inference import TTSHotPath
	hot = object.__new__(TTSHotPath)
	hot.autoregressive, hot.diffusion = _bare_model(max_batch=8), types.SimpleNamespace()
	cond, texts = _inputs()
	with pytest.raises(ValueError, match="beam_width must be 1"):
		hot.inference_lines(texts, cond, None, do_sample=False, beam_width=2)
	with pytest.raises(NotImplementedError, match="ancestral"):
		hot.inference_lines(texts, cond, None, diffusion_sampler="p", beam_width=2)
