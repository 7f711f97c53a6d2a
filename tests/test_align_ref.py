"""CPU checks of tests/align_ref.py and of the host side of the alignment feature: the derived bound of the attention map holds for a float32 emulation of
k_attn_probs and sees each of five planted faults; a float64 GPT-2 pass written out in align_ref reproduces the fixtures' maps; the numpy restatements of the
cost and of DTW recover the planted monotone paths (test_planted_paths_are_recovered says which) and break ties in the stated order; words and their times; the new symbols and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_ref as A
import attn_ref as R
from tortoise_tts_amd import _lib, alignment
from tortoise_tts_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = {"ttk_attn_probs", "ttk_align_prepare", "ttk_dtw", "ttk_ar_attentions", "ttk_ar_text_attention"}
CPU_CASES = [c for c in A.PROBS_CASES if c.layout == "gpt"]      # the layout is an addressing matter of the GPU buffers: the arithmetic does not see it


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.id for c in CPU_CASES])
def test_bound_holds_for_the_emulation_and_sees_every_fault(case):
	c = case
	q, k, _, _ = R.fwd_operands(c)
	ref, tol = A.probs_reference(c, q, k)
	above = torch.triu(torch.ones(c.T, c.T, dtype=torch.bool), 1)
	assert (ref[..., above] == 0).all() and (tol[..., above] == 0).all() and (ref.sum(-1) - 1).abs().max() < 1e-12
	r = A.worst_ratio(A.emulate_probs(c, q, k), ref, tol)
	print(f"{c.id}: emulation err / tol {r:.3f}")
	assert r <= 1.0
	for win in A.windows(c.T):
		r0, Rn, c0, Cn = win
		got = A.emulate_probs(c, q, k, window=win, heads=[1])
		assert A.worst_ratio(got, ref[:, 1:2, r0:r0 + Rn, c0:c0 + Cn], tol[:, 1:2, r0:r0 + Rn, c0:c0 + Cn]) <= 1.0
	for fault in A.PROBS_FAULTS:
		if not A.probs_fault_applies(c, fault):
			continue
		r = A.worst_ratio(A.emulate_probs(c, q, k, fault=fault), ref, tol)
		assert r > 1.0, f"{c.id}: the bound does not see {fault} (err / tol {r:.3f})"


def _fixture(name):
	return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name,tag,cfg,seed,variant", [("ar_attn_small", "a", W.AR_SMALL, 41, None), ("ar_attn_small", "c", W.AR_SMALL, 41, None),
													  ("ar_attn_small", "d", W.AR_SMALL, 41, None), ("ar_attn_peaked", "peaked", W.AR_SMALL, 41, "peaked"),
													  ("ar_attn_full", "full", W.AR_FULL, 42, None)])
def test_float64_gpt2_pass_reproduces_the_fixture_maps(name, tag, cfg, seed, variant):
	"""tolerance: the stored max |P32 - P64| of the layer -- the reference's own f32 pass against its own f64 pass -- plus 1e-12 for two f64 passes"""
	g = _fixture(name)
	assert int(g["seed"]) == seed
	sd = W.synth_state_dict(W.ar_score_shapes(cfg), seed)
	if variant:
		sd = W.stress_ar(sd, cfg, variant)
	t = lambda k: torch.from_numpy(g[f"{tag}_{k}"])
	maps = t("maps")
	S = t("text").shape[1] + t("codes").shape[1] + 5
	assert maps.shape == (cfg.layers, t("codes").shape[0], cfg.heads, S, S) and maps.dtype == torch.float32
	assert (torch.triu(maps, 1) == 0).all() and (maps.sum(-1) - 1).abs().max() <= 4e-7
	mine = A.gpt2_maps_f64(sd, cfg, t("cond"), t("text"), t("codes"))
	dev = (mine - maps.double()).abs().amax(dim=(1, 2, 3, 4))
	print(f"{tag}: max |P64 - P32 stored| per layer up to {dev.max():.3e}, stored deviation up to {t('dev32').max():.3e}")
	assert (dev <= t("dev32") + 1e-12).all(), (dev, t("dev32"))
	assert (t("devbf16") > t("dev32")).all()


def test_planted_paths_are_recovered():
	"""200 seeded planted paths (align_ref.planted_case: 3 .. 11 tokens, 4 .. 8 rows per token, 3 heads).  Measured: 199 of 200 are recovered exactly; the miss
	(seed 7) has 11 tokens.  At 11 tokens a planted row's mean, (0.6 + 10 * 0.05) / 11 = 0.1, equals the noise ceiling, so a noise cell can standardise to a
	value above 0; where the three heads' median-filtered mean is positive beside the path its cost is negative and the recurrence gains by taking that cell as an
	extra text step: the planted path is then NOT the optimum of the stated recurrence.  So: with at most 10 tokens every path must be recovered exactly, with token
	starts at each run's first row; in every case the found path must cost no more than the planted one, and strictly less where it differs from it."""
	hits, n10, misses = 0, 0, []
	for seed in range(200):
		blocks, tok = A.planted_case(seed)
		ti, mi, starts, total = A.align_reference(blocks)
		ok = ti.shape == tok.shape and (ti == tok).all() and (mi == np.arange(tok.size)).all()
		matrix, _ = A.prepare_reference(blocks[None], 7)
		planted = float((-matrix[0][np.arange(tok.size), tok]).sum())
		assert total <= planted + 1e-4 * abs(planted)
		if ok:
			first = np.concatenate([[0], np.flatnonzero(np.diff(tok)) + 1])
			assert (starts == first).all()
		else:
			assert blocks.shape[2] == 11 and total < planted - 1e-6, f"seed {seed}: a path other than the planted one that is not cheaper"
		hits += bool(ok)
		misses += [] if ok else [seed]
		n10 += blocks.shape[2] <= 10
	print(f"{hits} of 200 planted paths recovered exactly ({n10} cases with at most 10 tokens, all of them); misses {misses}")
	assert hits == 199 and misses == [7]


def test_dtw_ties_take_the_diagonal_then_the_mel_step_then_the_text_step():
	trace, total = A.dtw_reference(np.zeros((4, 4), dtype=np.float32))
	assert total == 0 and (trace.diagonal() == 0).all()
	ti, mi = alignment.backtrace(trace)
	assert ti.tolist() == mi.tolist() == [0, 1, 2, 3]
	trace, _ = A.dtw_reference(np.zeros((5, 2), dtype=np.float32))      # more mel rows than tokens: the diagonal while it lasts, then mel steps
	assert trace[0, 0] == 0 and (trace[1:, 0] == 1).all() and trace[0, 1] == 2      # borders: only one finite neighbour
	assert trace[1, 1] == 0 and trace[2, 1] == 0      # all three equal: the diagonal; and D[1][1] == D[1][2] == D[2][1]: the diagonal again
	ti, mi = alignment.backtrace(trace)
	assert mi.tolist() == [0, 1, 2, 3, 4] and ti.tolist() == [0, 0, 0, 0, 1]      # read back from the end: diagonal into (3, 0), then mel steps
	trace, _ = A.dtw_reference(np.zeros((2, 5), dtype=np.float32))
	ti, mi = alignment.backtrace(trace)
	assert ti.tolist() == [0, 1, 2, 3, 4] and mi.tolist() == [0, 0, 0, 0, 1]
	c = np.zeros((3, 3), dtype=np.float32)
	c[1, 1] = 1.0      # diagonal blocked in the middle: D[1][2] == D[2][1] == 0 tie between the mel step and the text step -> mel step (from above)
	trace, _ = A.dtw_reference(c)
	assert trace[2, 2] == 1


def test_prepare_reference_edges():
	rng = np.random.default_rng(5)
	blocks = rng.uniform(0, 1, size=(1, 2, 3, 1)).astype(np.float32)      # Tt = 1: std 0 everywhere -> zeros
	m, tol = A.prepare_reference(blocks, 7)
	assert (m == 0).all() and (tol == 0).all()
	blocks = rng.uniform(0, 1, size=(1, 1, 3, 4)).astype(np.float32)      # M = 3 <= 7 // 2: no filter
	m7, _ = A.prepare_reference(blocks, 7)
	m1, _ = A.prepare_reference(blocks, 1)
	assert np.array_equal(m7, m1)
	blocks = rng.uniform(0, 1, size=(1, 1, 8, 4)).astype(np.float32)
	m3, _ = A.prepare_reference(blocks, 3)
	z, _ = A.prepare_reference(blocks, 1)
	assert np.allclose(m3[0, 0], np.median(z[0, [1, 0, 1]], axis=0)) and np.allclose(m3[0, 7], np.median(z[0, [6, 7, 6]], axis=0))      # reflect


class _Tok:
	"""one token per character, `_` for [SPACE]"""

	def get_vocab(self):
		return {"[SPACE]": 2}

	def decode(self, ids):
		return "".join(chr(i) for i in ids)


def _ids(s):
	return [2 if ch == " " else ord(ch) for ch in s]


def test_words_and_timings():
	tok = _Tok()
	assert alignment.words_from_tokens(tok, _ids("hi there")) == [("hi", 0, 2), ("there", 3, 8)]
	assert alignment.words_from_tokens(tok, _ids(" hi  there ")) == [("hi", 1, 3), ("there", 5, 10)]      # leading, doubled and trailing spaces
	assert alignment.words_from_tokens(tok, _ids("word")) == [("word", 0, 4)]
	assert alignment.words_from_tokens(tok, _ids("  ")) == []
	ids = _ids(" hi  there ")
	starts = [0, 2, 4, 6, 7, 9, 10, 12, 14, 15, 18]
	per = 1024 / 22050
	got = alignment.word_timings(tok, ids, starts, 20)
	assert got == [("hi", 2 * per, 6 * per), ("there", 9 * per, 18 * per)]      # a word ends where the token behind it starts
	assert alignment.word_timings(tok, _ids("word"), [0, 3, 5, 9], 12) == [("word", 0.0, 12 * per)]      # the last word ends at M
	assert alignment.clip_and_offset([("a", 0.5, 2.0)], 1.5, 10.0) == [("a", 10.5, 11.5)]
	assert alignment.default_heads(30, 16)[0] == (15, 0) and len(alignment.default_heads(30, 16)) == 240 and alignment.default_heads(2, 2) == [(1, 0), (1, 1)]
	ti, mi = alignment.backtrace(np.array([[0, 2], [1, 0], [1, 1]], dtype=np.uint8))
	assert ti.tolist() == [0, 1, 1] and mi.tolist() == [0, 1, 2] and alignment.token_starts(ti, mi, 2).tolist() == [0, 1]


def test_header_symbols_and_struct_size_agree():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert NEW <= declared and declared == set(_lib.SYMBOLS)
	lib = _lib.load()
	assert all(hasattr(lib, n) for n in NEW)
	assert ctypes.sizeof(_lib.AttnProbsDesc) == 80      # static_assert'ed in csrc/align.hip
	assert ctypes.sizeof(_lib.AttnDesc) == 96 and ctypes.sizeof(_lib.ARConfigC) == 56      # the existing structs are not touched
	assert len(_lib.SYMBOLS["ttk_ar_attentions"][1]) == 11 and len(_lib.SYMBOLS["ttk_ar_text_attention"][1]) == 11


def test_refusals_without_a_gpu():
	"""the library refuses these before it looks at the device (the buffers are never read: any aligned non-null address will do)"""
	lib = _lib.load()
	buf = (ctypes.c_float * 8)()
	p = ctypes.addressof(buf) & ~15
	err = lambda: lib.ttk_last_error().decode()
	assert lib.ttk_dtw(p, 1, 607, 4, p, p, p, None) != 0 and "M must lie in 1..606" in err()
	assert lib.ttk_dtw(p, 1, 4, 405, p, p, p, None) != 0 and "Tt must lie in 1..404" in err()
	assert lib.ttk_dtw(None, 1, 4, 4, p, p, p, None) != 0 and "null" in err()
	assert lib.ttk_align_prepare(p, 1, 0, 4, 4, 7, p, None, None) != 0 and "no head selected" in err()
	for width in (0, 4, 17):
		assert lib.ttk_align_prepare(p, 1, 1, 4, 4, width, p, None, None) != 0 and "must be odd and in 1..15" in err()
	assert lib.ttk_align_prepare(p, 1, 1, 700, 4, 7, p, None, None) != 0 and "M must lie" in err()
	d = _lib.AttnProbsDesc(qkv=p, ld=384, q_off=0, k_off=128, head_stride=64, nb=1, T=8, H=2, scale=0.125, n_sel=1, heads=p, out=p, r0=0, R=8, c0=0, C=8)
	assert lib.ttk_attn_probs(7, ctypes.byref(d), None) != 0 and "dtype must be" in err()
	d.R = 9
	assert lib.ttk_attn_probs(1, ctypes.byref(d), None) != 0 and "must be non-empty and lie inside" in err()
	d.R, d.C, d.c0 = 8, 0, 3
	assert lib.ttk_attn_probs(1, ctypes.byref(d), None) != 0 and "must be non-empty and lie inside" in err()
	d.C, d.c0, d.k_off = 8, 0, 260
	assert lib.ttk_attn_probs(1, ctypes.byref(d), None) != 0 and "multiples of 8" in err()
	d.k_off, d.ld = 128, 248
	assert lib.ttk_attn_probs(1, ctypes.byref(d), None) != 0 and "end past ld" in err()
	assert lib.ttk_ar_attentions(None, p, p, 4, p, 4, 1, None, 0, p, None) != 0 and "null argument" in err()
	assert lib.ttk_ar_text_attention(None, p, p, 4, p, 4, 1, None, 0, p, None) != 0 and "null argument" in err()
