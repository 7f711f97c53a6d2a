"""tests/voc_ref.py checked on the CPU: the float64 references equal independent evaluations of the same definitions (a row-by-row loop for the LVC, torch's
conv_transpose1d / conv1d Activation1d for the snake; the narrow conv's reference is F.conv1d itself), the case lists cover what the kernels branch on, the
operand conditions hold (unsaturated gate, finite positive bounds, f32 bounds below 1e-4 (1 + |v|), the snake's sine argument inside the measured range and past
pi), the faultless float32 replica of every kernel stays inside the derived bound on every case test_gpu_voc_forms.py runs, every named fault is caught on at
least one case, and the three caller-operand entry points are declared, listed and exported."""
import collections
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import voc_ref as R
from tortoise_tts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ttk_lvc_rows", "ttk_hifi_conv_rows", "ttk_snake_rows")


def test_case_lists_cover_what_the_issue_names():
	for dt, cg in R.LVC_FORMS:
		cs = [c for c in R.LVC_CASES if (c.dt, c.CG) == (dt, cg)]
		assert {(c.hop, c.Tc, c.L) for c in cs} == set(R.LVC_SHAPES) and {(c.n_layers, c.layer) for c in cs} == {(4, 0), (4, 3), (1, 0)}
	assert {c.mfma for c in R.LVC_CASES} == {False, True}
	assert any(c.L < c.Tc * c.hop for c in R.LVC_CASES) and any(c.L % 16 for c in R.LVC_CASES)
	assert any(16 // c.hop >= 3 and (64 % c.hop) for c in R.LVC_CASES)              # three or more segments per tile, one of them across the workgroup edge
	cs = R.HIFI_CASES
	assert {c.C for c in cs} == {32, 64} and {(c.k, c.dil) for c in cs} == set(R.HIFI_KD) and {c.L for c in cs} == set(R.HIFI_LS)
	assert {(c.mode, c.L) for c in cs} >= {(m, L) for m in range(4) for L in R.HIFI_LS}
	assert {(c.C, c.k, c.dil) for c in cs} >= {(C, k, d) for C in (32, 64) for k, d in R.HIFI_KD}
	assert all(c.ld == 64 for c in cs if c.C == 32) and all(c.ld % 8 == 0 and c.ld >= c.C for c in cs)
	assert all(c.k * c.C * c.C * 2 + (256 + (c.k - 1) * c.dil) * (c.C + 8) * 2 <= 160 * 1024 for c in cs)
	assert {(c.dt, c.L, c.C) for c in R.SNAKE_CASES} == {(dt, L, C) for dt in ("f32", "bf16") for L in (1, 2, 3, 4, 6, 7, 13, 70) for C in (4, 32, 36)}
	assert R.B == 2 and R.LVC_LDA == 64


@pytest.mark.parametrize("c", [c for c in R.LVC_CASES if c.L <= 90 and c.dt == "f32"][:6], ids=lambda c: c.id)
def test_lvc_reference_is_the_definition_row_by_row(c):
	o, r = R.lvc_operands(c), R.lvc_reference(c)
	CG, L = c.CG, c.L
	y = R.lrelu64(o["y"].double(), R.S02).view(R.B, L, CG)
	kern = o["kern"].double().view(R.B, c.Tc, c.n_layers, CG, 2 * CG, 3)
	kb = o["kbias"].double().view(R.B, c.Tc, c.n_layers, 2 * CG)
	for b in range(R.B):
		for t in sorted({0, 1, c.hop - 1, c.hop, 15, 16, 63, 64, L - 2, L - 1} & set(range(L))):
			pre = kb[b, t // c.hop, c.layer].clone()
			for k in range(3):
				if 0 <= t + k - 1 < L:
					pre += y[b, t + k - 1] @ kern[b, t // c.hop, c.layer, :, :, k]
			x = o["x"].double()[b * L + t] + torch.sigmoid(pre[:CG]) * torch.tanh(pre[CG:])
			assert torch.allclose(r["x"][b * L + t], x, rtol=1e-12, atol=1e-12)
			assert torch.allclose(r["at"][b * L + t], torch.where(x > 0, x, x * R.S02), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", [c for c in R.SNAKE_CASES if c.dt == "f32" and c.C == 4], ids=lambda c: c.id)
def test_snake_reference_is_activation1d_in_f64(c):
	"""UpSample1d (replicate pad 5, zero-stuffing transposed conv, gain 2, trim 15), SnakeBeta, DownSample1d (replicate pad 5 / 6, stride 2)"""
	o, r = R.snake_operands(c), R.snake_reference(c)
	g = o["filt"].double()
	x = o["x"].double().view(R.B, c.L, c.C).permute(0, 2, 1)
	filt = g[None, None].expand(c.C, 1, 12)
	up = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), filt, stride=2, groups=c.C)[..., 15:-15]
	z = up + o["invb"].double()[None, :, None] * torch.sin(up * o["a"].double()[None, :, None]) ** 2
	y = F.conv1d(F.pad(z, (5, 6), mode="replicate"), filt, stride=2, groups=c.C)
	assert torch.allclose(r["y"], y.permute(0, 2, 1).reshape(R.B * c.L, c.C), rtol=1e-11, atol=1e-11)
	assert abs(float(g.sum()) - 1) < 1e-6


def test_hifi_pack_is_a_bijection_onto_the_rounded_weights():
	for c in (R.HifiCase(32, 3, 1, 7, 0), R.HifiCase(64, 7, 3, 7, 0)):
		w = R.hifi_operands(c)["w"]
		marks = (torch.arange(w.numel(), dtype=torch.float32) % 251).view_as(w)          # integers below 256: exact in bf16
		frag = R.hifi_pack(c, marks)
		assert frag.numel() == w.numel() and sorted(frag.tolist()) == sorted(marks.flatten().tolist())
		assert not torch.equal(R.hifi_pack(c, w, "kb_and_nt_swapped_in_fragment_order"), R.hifi_pack(c, w)) or c.C == 32


def test_operand_conditions():
	"""no case can pass for lack of signal"""
	for c in R.LVC_CASES:
		r = R.lvc_reference(c)
		live = (r["a"].abs() < 2) & (r["g"].abs() < 1.5)
		assert float(live.float().mean()) >= 0.5, f"{c.id}: the gate is saturated on most outputs"
		for k in ("tol_x", "tol_at"):
			assert torch.isfinite(r[k]).all() and (r[k] > 0).all(), f"{c.id}: an element without a finite bound"
		assert (r["tol_x"] < 1e-4 * (1 + r["x"].abs())).all(), f"{c.id}: the bound of x is not below 1e-4 (1 + |v|): {float((r['tol_x'] / (1 + r['x'].abs())).max()):.3g}"
		if c.dt == "f32":
			assert (r["tol_at"] < 1e-4 * (1 + r["at"].abs())).all(), c.id
	for c in R.HIFI_CASES:
		for name, (v, tol) in R.hifi_reference(c).items():
			assert torch.isfinite(tol).all() and (tol > 0).all(), f"{c.id}: {name} has an element without a finite bound"
			if name != "at_out":
				assert (tol < 1e-4 * (1 + v.abs())).all(), f"{c.id}: the bound of {name} is not below 1e-4 (1 + |v|): {float((tol / (1 + v.abs())).max()):.3g}"
	for c in R.SNAKE_CASES:
		r = R.snake_reference(c)
		assert torch.isfinite(r["tol"]).all() and (r["tol"] > 0).all(), c.id
		amax = float(r["arg"].abs().max())
		assert math.pi <= amax <= R.SNAKE_ARG_MAX, f"{c.id}: max |up a| = {amax:.3f} outside [pi, {R.SNAKE_ARG_MAX}]"
		if c.dt == "f32":
			assert (r["tol"] < 1e-4 * (1 + r["y"].abs())).all(), c.id
	assert R.SIN_FAST_ERR == 2 * R.SIN_FAST_MEASURED and R.MFMA == 1e-5 and R.TRANS == 2e-6


@pytest.mark.parametrize("kernel", list(R.CASES))
def test_replica_is_inside_the_bound(kernel):
	worst = collections.defaultdict(float)
	for c in R.CASES[kernel]:
		for k, r in R.CHECK[kernel](c, R.EMULATE[kernel](c)).items():
			assert r <= 1, f"{c.id}: the kernel's own arithmetic is {r:.3g}x the bound on {k}: the bound misses a term"
			worst[f"{c.group} {k}"] = max(worst[f"{c.group} {k}"], r)
	for k in sorted(worst):
		print(f"replica worst err / bound, {k}: {worst[k]:.3f}")


@pytest.mark.parametrize("kernel,fault", [(k, f) for k in R.FAULTS for f in R.FAULTS[k]])
def test_fault_is_caught(kernel, fault):
	"""over every case where the fault applies: caught by the bound or by a canary on at least one -- and, for the LVC, in each of its two kernels"""
	applies, hits, first = 0, collections.Counter(), None
	for c in R.CASES[kernel]:
		if not R.FAULT_APPLIES[kernel](c, fault):
			continue
		applies += 1
		how = None
		try:
			w = R.CHECK[kernel](c, R.EMULATE[kernel](c, fault))
			if max(w.values()) > 1:
				how = f"{max(w.values()):.3g}x the bound"
		except AssertionError as e:
			how = "canary: " + str(e).split(": ", 1)[-1][:70]
		if how:
			hits[c.group] += 1
			first = first or f"{c.id} ({how})"
	print(f"{kernel} {fault}: caught on {sum(hits.values())} of {applies} cases where it applies, first on {first}")
	assert applies > 0 and first, f"{kernel} {fault}: not caught on any of {applies} cases"
	if kernel == "lvc":
		assert all(hits[g] for g in R.GROUPS if g.startswith("lvc")), f"{fault}: not caught in every LVC kernel form: {dict(hits)}"


def test_new_symbols_are_declared_listed_and_exported():
	header = open(os.path.join(ROOT, "include", "ttk.h")).read()
	declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", header))
	assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
	assert "ttk_lvc_desc" in header and "ttk_hifi_conv_desc" in header
	assert len(_lib.SYMBOLS["ttk_lvc_rows"][1]) == 3 and len(_lib.SYMBOLS["ttk_hifi_conv_rows"][1]) == 2 and len(_lib.SYMBOLS["ttk_snake_rows"][1]) == 10
	assert ctypes.sizeof(_lib.LvcDesc) == 5 * 8 + 8 * 4 and ctypes.sizeof(_lib.HifiConvDesc) == 12 * 8      # ttk_lvc_desc: 5 pointers, 8 ints; ttk_hifi_conv_desc: 12 eight-byte slots
	lib = ctypes.CDLL(_lib.build())
	assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
