"""Beam search, CPU side: the restated HF `_beam_search(do_sample=True)` (tests/beam_ref.py) against the ids of the installed HuggingFace loop on
the model-free stub (tests/golden/hf_beam_loop.npz, written by tools/make_golden_beam.py) and, when transformers is importable, against that loop
live; what the fixture's cases cover; and the argument checks of the product's beam path that need no device."""
import json
import os
import shutil
import subprocess
import types

import pytest
import torch

import beam_ref as BR
import stub_lm
from tortoise_tts_amd import weights as W

NAMES = [c[0] for c in BR.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_restated_beam_search_equals_huggingface_on_stub_model(golden, name):
	g = golden("hf_beam_loop")
	ids, (seed, bias, N, R, L, kw) = BR.stub_case(name)
	made_with = json.loads(str(g["kw::" + name]))
	assert made_with == json.loads(json.dumps(dict(seed=seed, stop_bias=bias, num_beams=N, num_return_sequences=R, max_generate_length=L, kwargs=kw)))
	want = torch.from_numpy(g["ids::" + name])
	assert ids.shape == want.shape and torch.equal(ids, want), (ids.tolist(), want.tolist())
	pytest.importorskip("transformers")
	assert torch.equal(BR.hf_case(name), want)                # live: the loop the fixture came from


def test_fixture_covers_early_ends_max_length_several_returns_and_the_finished_path(golden):
	g = golden("hf_beam_loop")
	early, at_max, several, not_top_running = [], [], [], []
	for name, _, _, N, R, L, _ in BR.CASES:
		want = torch.from_numpy(g["ids::" + name])
		(ids, tr), _ = BR.stub_case(name, return_trace=True)
		assert torch.equal(ids, want)
		assert bool(tr["finished"][:R].all())                 # `sequences` is filled only by beams that hit a stopping criterion
		if tr["steps"] < L:
			early.append(name)
		else:
			at_max.append(name)
		if R > 1:
			several.append(name)
		# the best running beam after the last step: its tokens are not what comes back (a finished beam is returned even where a running one outscores it)
		top = tr["running"][0]
		if top.shape[0] != ids.shape[1] or not torch.equal(top, ids[0]):
			not_top_running.append(name)
		if tr["steps"] < L:
			assert float(tr["running_scores"][0]) > -1e8          # (an early end leaves real running beams behind)
	assert len(early) >= 2 and len(at_max) >= 1 and len(several) >= 1 and len(not_top_running) >= 1, (early, at_max, several, not_top_running)
	# and in one of the early ends the surviving running beam has the better raw score: the is_sent_finished path decides, not the score
	(ids, tr), _ = BR.stub_case("four_beams", return_trace=True)
	assert ids.shape[1] < tr["steps"]


def test_rows_are_padded_with_the_stop_token_to_the_longest_returned_beam():
	(ids, tr), (_, _, N, R, L, _) = BR.stub_case("two_beams_warpers", return_trace=True)
	lens = tr["lengths"][:R].tolist()
	assert ids.shape == (R, max(lens)) and len(set(lens)) > 1
	for row, n in zip(ids, lens):
		assert int(row[n - 1]) == stub_lm.STOP and (row[n:] == stub_lm.STOP).all() and not (row[:n - 1] == stub_lm.STOP).any()


def test_more_returned_sequences_than_beams_is_hfs_value_error():
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(1, 0.0))
	with pytest.raises(ValueError, match="num_return_sequences"):
		BR.beam_search(ar, torch.zeros(1, 1), torch.zeros(1, 9, dtype=torch.long), num_beams=2, num_return_sequences=3, max_generate_length=4)


@pytest.fixture(scope="module")
def book_check(tmp_path_factory):
	"""the kernel's bookkeeping function (csrc/beam_book.h) as a stand-alone host program, built with the address and undefined-behaviour sanitizers"""
	cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
	if cxx is None:
		pytest.skip("no host C++ compiler")
	root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	exe = str(tmp_path_factory.mktemp("beam_book") / "beam_book_check")
	src = os.path.join(root, "tests", "diag", "beam_book_check.cpp")
	san = subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True)
	if san.returncode != 0:           # a compiler without the sanitizer runtimes: the same program, unchecked
		subprocess.run([cxx, "-O1", "-std=c++17", src, "-o", exe], check=True, capture_output=True)
	return exe


@pytest.mark.parametrize("name", NAMES)
def test_kernel_bookkeeping_on_the_host_follows_the_restated_loop(book_check, name):
	"""steps d to g as the kernel runs them, fed the picks (flat index, accumulated log-prob) of every step of the restated loop: tokens, beam_idx, flags,
	lengths, the heuristic bit, both sequence stores and the step at which the search ends are equal; scores to f32 rounding of one division"""
	trace = []
	(ids, tr), (seed, bias, N, R, L, kw) = BR.stub_case(name, return_trace=True, step_trace=trace)
	lines = [f"{N} {stub_lm.V} {L} {stub_lm.STOP} {kw.get('length_penalty', 1.0)!r}"]
	for t in trace:
		lines.append(" ".join(f"{int(i)} {float(v)!r}" for i, v in zip(t["picks"], t["pick_lp"])))
	out = subprocess.run([book_check], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().splitlines()
	assert len(out) == len(trace) == tr["steps"]
	for k, (line, t) in enumerate(zip(out, trace)):
		f = [x.split() for x in line.split("|")]
		assert int(f[0][0]) == (k == len(trace) - 1), k
		# at max_length every pick hits MaxLengthCriteria: all running scores tie at -1e9 and which of them torch.topk keeps is unspecified (and unused:
		# the search is over); everywhere else at least num_beams picks are not the stop token and the running side is determined
		at_max = k + 1 == L
		if not at_max:
			assert [int(x) for x in f[1]] == t["tok"].tolist() and [int(x) for x in f[2]] == t["beam_idx"].tolist(), k
			assert torch.tensor([int(x) for x in f[8]]).view(N, k + 1).tolist() == t["running"][:, :k + 1].tolist(), k
		assert torch.allclose(torch.tensor([float(x) for x in f[3]]), t["running_scores"], rtol=1e-6, atol=0), k
		assert torch.allclose(torch.tensor([float(x) for x in f[4]]), t["beam_scores"], rtol=1e-6, atol=0), k
		fin = t["finished"]
		assert [bool(int(x)) for x in f[5]] == fin.tolist() and bool(int(f[7][0])) == t["unsatisfied"], k
		assert torch.tensor([int(x) for x in f[6]])[fin].tolist() == t["lengths"][fin].tolist(), k
		assert torch.tensor([int(x) for x in f[9]]).view(N, L)[fin].tolist() == t["sequences"][fin][:, :L].tolist(), k


def _bare_model(max_batch=8):
	"""a UnifiedVoice without a device handle: every check below is raised before the first device call"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	m = object.__new__(UnifiedVoice)
	m.cfg, m.max_batch, m.max_ctx, m._streaming, m.hf_exact_top_p = W.AR_SMALL, max_batch, 128, False, False
	m.device = torch.device("cuda:0")
	return m


def test_product_argument_checks_need_no_device():
	from tortoise_tts_amd import _lib
	m = _bare_model()
	cond, text = torch.zeros(1, 128), torch.ones(1, 5, dtype=torch.long)
	with pytest.raises(ValueError, match=r"`num_return_sequences` \(3\) has to be smaller or equal to `num_beams` \(2\)"):
		m.inference_speech(cond, text, do_sample=True, num_beams=2, num_return_sequences=3)
	with pytest.raises(ValueError, match="top_k"):
		m.inference_speech(cond, text, do_sample=True, num_beams=4, top_k=7)              # 0 < top_k < 2 * num_beams
	with pytest.raises(_lib.TTKError, match="beams exceed"):
		_bare_model(max_batch=4).inference_speech(cond, text, do_sample=True, num_beams=8, top_k=0)
	with pytest.raises(_lib.TTKError, match="beams exceed"):
		_bare_model(max_batch=32).inference_speech(cond, text, do_sample=True, num_beams=17, top_k=0)


def test_kept_refusals_name_beam_search():
	from tortoise_tts_amd.tts import TTS
	m = _bare_model()
	cond, text = torch.zeros(1, 128), torch.ones(1, 5, dtype=torch.long)
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech(cond, text, do_sample=True, num_beams=2, input_tokens=torch.ones(1, 2, dtype=torch.long))
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech(cond, text, do_sample=True, num_beams=2, candidate_shard=(0, 1))
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech(cond, text, do_sample=True, num_beams=2, typical_sampling=True)
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech(cond, text, num_beams=2)                                         # greedy beam search (do_sample False)
	with pytest.raises(NotImplementedError, match="beam"):
		m.inference_speech_lines(cond, [text, text], do_sample=True, num_beams=2)
	tts = TTS(types.SimpleNamespace(device=torch.device("cuda:0")), None, None, hifigan=object())
	with pytest.raises(NotImplementedError, match="beam"):
		tts.inference("Hello.", {"latent": (None, None)}, vocoder_type="hifigan", beam_width=2)
