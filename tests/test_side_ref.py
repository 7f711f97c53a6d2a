"""tests/side_ref.py checked on the CPU: the float64 references equal torch's own group_norm / softmax attention / unfold-free gather / erf-GELU in f64, the case
lists hold the shapes the issue names, every bound is finite (zero only where an element is owed exactly) and small enough to matter, the float32 emulation of every
kernel stays inside its bound on every case tests/test_gpu_side_forms.py runs, every seeded fault leaves the bound (or trips a canary) on at least one case it
applies to, the operand conditions the GPU test relies on hold, and the new entry points are declared in include/ttk.h and in _lib.py's symbol table."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import side_ref as R

NEW_SYMBOLS = ("ttk_block_gn_rows", "ttk_attn_rowwave", "ttk_cond_im2col_rows", "ttk_cond_pool_rows", "ttk_clvp_embed_rows", "ttk_clvp_rmsnorm_rows",
			   "ttk_clvp_rotary_rows", "ttk_clvp_geglu_rows", "ttk_clvp_mean_rows", "ttk_clvp_latent_score")
# A dropped term (a bias, a clamp, a factor, a wrong operand) moves an element by the order of the output's own size.  Ceilings on max(bound) / max|ref| per
# case: f32 two orders below that; T-typed outputs add bf16's half ulp (2^-8 relative at the bound's own argument).
CEILING = {"f32": 1e-2, "rounded": 1e-2 + 2.0 ** -7}


def emulate(c, fault=None):
	rows = R.emu_rows(c)
	k = R.KERNELS[c.kernel]
	return (k.emu(c, fault, rows=rows) if rows else k.emu(c, fault)), rows


def test_entry_points_are_declared():
	from tortoise_tts_amd import _lib
	header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ttk.h")).read()
	declared = set(re.findall(r"^(?:int|const char\*)\s+(ttk_\w+)\s*\(", header, re.M))
	assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
	n_args = {"ttk_block_gn_rows": 10, "ttk_attn_rowwave": 3, "ttk_cond_im2col_rows": 15, "ttk_cond_pool_rows": 7, "ttk_clvp_embed_rows": 9,
			  "ttk_clvp_rmsnorm_rows": 7, "ttk_clvp_rotary_rows": 7, "ttk_clvp_geglu_rows": 6, "ttk_clvp_mean_rows": 7, "ttk_clvp_latent_score": 8}
	for s, n in n_args.items():
		assert len(_lib.SYMBOLS[s][1]) == n, s
		decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", header, re.M | re.S).group(1)
		assert decl.count(",") + 1 == n, s


def test_case_lists_hold_the_shapes_the_kernels_branch_on():
	ps = lambda k: [c.p for c in R.KERNELS[k].cases]
	dts = lambda k: {c.dt for c in R.KERNELS[k].cases}
	assert {(p.T, p.C, p.groups) for p in ps("gn")} == {(1, 128, 32), (5, 48, 16), (67, 1024, 32), (130, 2048, 32)} and dts("gn") == {"f32", "bf16"}
	assert all(p.nb == 2 for p in ps("gn")) and any(p.offset for p in ps("gn"))
	for dt in ("f32", "bf16"):
		for b in (0, 1):
			assert {c.p.T for c in R.RW_CASES if c.dt == dt and c.p.bias == b and c.p.H == 2 and c.p.nb == 2} >= {1, 3, 4, 5, 63, 64, 65, 130, 200}
		assert any(c.dt == dt and c.p.ld_extra and c.p.ldo_extra for c in R.RW_CASES) and any(c.dt == dt and c.p.hot for c in R.RW_CASES)
	assert [(c.dt, c.p.nb, c.p.H) for c in R.RW_CASES if c.p.T == R.ROWWAVE_MAX_T] == [("f32", 1, 1)]
	for dt in ("f32", "bf16"):
		for lay in ("cf", "cl"):
			cs = [c.p for c in R.IM_CASES if c.dt == dt and c.p.layout == lay]
			assert {p.Tin for p in cs if (p.taps, p.stride, p.pad) == (3, 2, 1) and p.Cin == 5} == {1, 2, 5, 6}
			assert any((p.taps, p.Tin) == (1, 5) for p in cs)
		assert any(c.dt == dt and c.p.Cin == 100 and c.p.Kpad == 320 for c in R.IM_CASES)
	assert {(p.mode, p.T, p.C) for p in ps("pool")} == {(m, T, C) for m in (0, 1) for T in (1, 2, 130) for C in (128, 300)}
	assert {(p.rows, p.d) for p in ps("rmsnorm")} == {(r, d) for r in (1, 5) for d in (64, 256, 768)} and dts("rmsnorm") == {"f32", "bf16"}
	assert {(p.B, p.S, p.H) for p in ps("rotary")} == {(2, S, H) for S in (1, 5, 250) for H in (1, 12)} and dts("rotary") == {"f32", "bf16"}
	assert {(p.rows, p.inner) for p in ps("geglu")} == {(3, 64), (3, 1536)} and dts("geglu") == {"f32", "bf16"}
	assert {(p.S, p.d) for p in ps("mean")} == {(1, 64), (7, 64), (250, 64)} and dts("mean") == {"f32", "bf16"}
	assert {(p.Bt, p.B, p.d) for p in ps("score")} == {(1, 3, 64), (1, 3, 768), (3, 3, 64), (3, 3, 768)} and R.TEMPERATURE != 0
	p = ps("embed")[0]
	ids = R.embed_ops(R.EMBED_CASES[0])["ids"][:, :p.S]
	assert p.stride > p.S and p.d == 64 and bool((ids < 0).any()) and bool((ids >= p.vocab).any())


def test_references_are_torch_in_f64():
	for c in R.GN_CASES:
		o, (y, _) = R.gn_ops(c), R.gn_ref(c)
		want = F.group_norm(o["x"].double().transpose(1, 2), c.p.groups, o["gamma"].double(), o["beta"].double(), R.EPS).transpose(1, 2)
		assert torch.allclose(y, want, rtol=1e-10, atol=1e-10), c.id
	for c in R.RW_CASES:
		if c.p.T > 200 or c.dt != "f32":
			continue
		o, (y, _) = R.rw_ops(c), R.KERNELS["rowwave"].ref(c)
		p = c.p
		q, k, v = (o[n].double() for n in "qkv")
		s = torch.einsum("bhqd,bhkd->bhqk", q, k) * R.SCALE128
		if p.bias:
			rel = (torch.arange(p.T)[None, :] - torch.arange(p.T)[:, None]).clamp(-64, 64) + 64
			s = s + o["bias"].double()[:, rel]
		want = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s, -1), v).reshape(p.nb * p.T, p.H * 128)
		assert torch.allclose(y[:, :p.H * 128], want, rtol=1e-10, atol=1e-12), c.id
		assert torch.isnan(y[:, p.H * 128:]).all()
	for c in R.IM_CASES:      # against Conv1d itself: the gathered rows times a weight matrix are the convolution
		p, o = c.p, R.im_ops(c)
		if c.dt != "f32":
			continue
		x = o["src"].double().reshape(p.nb, p.Cin, p.Tin) if p.layout == "cf" else o["src"].double().reshape(p.nb, p.Tin, p.Cin).transpose(1, 2)
		w = torch.randn(4, p.Cin, p.taps, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
		want = F.conv1d(x, w, stride=p.stride, padding=p.pad).transpose(1, 2).reshape(p.nb * p.Tout, 4)
		y = R.im_ref(c)[0]
		assert torch.allclose(y[:, :p.Cin * p.taps] @ w.reshape(4, -1).t(), want, rtol=1e-10, atol=1e-10), c.id
		assert not y[:, p.Cin * p.taps:].any(), c.id
	for c in R.GEGLU_CASES:
		h = R.geglu_ops(c)["h"].double()
		assert torch.allclose(R.geglu_ref(c)[0], h[:, :c.p.inner] * F.gelu(h[:, c.p.inner:]), rtol=1e-10, atol=1e-12), c.id
	for c in R.RMS_CASES:
		o = R.rms_ops(c)
		x = o["x"].double()
		want = x / (x.norm(dim=1, keepdim=True) * c.p.d ** -0.5).clamp(min=1e-8) * o["g"].double()      # xtransformers RMSNorm
		assert torch.allclose(R.rms_ref(c)[0], want, rtol=1e-12, atol=0), c.id
	for c in R.SCORE_CASES:
		o, p = R.score_ops(c), c.p
		t = (o["text"][:p.Bt].expand(p.B, -1) if p.Bt == 1 else o["text"]).double()
		want = (F.normalize(t, dim=1) * F.normalize(o["speech"].double(), dim=1)).sum(1) * o["temperature"].double().exp()      # the f32 operand's value
		assert torch.allclose(R.score_ref(c)[0], want, rtol=1e-10, atol=1e-12), c.id


@pytest.mark.parametrize("group", R.GROUPS)
def test_emulation_is_inside_the_bound_and_the_bound_is_tight_enough_to_matter(group):
	worst = tight = 0.0
	for c in (c for c in R.ALL_CASES if c.group == group):
		y, tol = R.KERNELS[c.kernel].ref(c)
		owed = ~torch.isnan(y)
		assert torch.isfinite(tol[owed]).all() and (tol[owed] >= 0).all(), f"{c.id}: an element without a finite bound"
		if c.kernel in R.EXACT_KERNELS or (c.kernel == "pool" and c.p.mode == 0):
			assert not tol[owed].any(), f"{c.id}: an exact kernel with a tolerance"
		else:
			computed = owed & (y != 0)
			if c.kernel == "rotary":      # features 32..63 of a head are owed exactly
				computed &= (torch.arange(y.shape[1]) % 64 < 32)[None, :]
				assert not tol[:, torch.arange(y.shape[1]) % 64 >= 32].any(), f"{c.id}: an untouched feature with a tolerance"
			assert (tol[computed] > 0).all(), f"{c.id}: a computed element without a bound"
			rel = float(tol[owed].max() / y[owed].abs().max())
			assert rel <= CEILING[group.split()[1]], f"{c.id}: the bound is {rel:.3g} of the largest output: too loose to see a dropped term"
			tight = max(tight, rel)
		img, rows = emulate(c)
		r = R.check(c, img, ref=(y, tol), rows=rows)
		assert r <= 1, f"{c.id}: the kernel's own arithmetic is {r:.3g}x the bound: the bound misses a term"
		worst = max(worst, r)
	print(f"{group}: emulation worst err / bound {worst:.3f}, largest bound / max|ref| {tight:.3g}")


@pytest.mark.parametrize("kernel,fault", [(k, f) for k in R.FAULTS for f in R.FAULTS[k]])
def test_fault_is_caught(kernel, fault):
	applies = hits = 0
	for c in R.KERNELS[kernel].cases:
		if not R.FAULTS[kernel][fault](c):
			continue
		applies += 1
		try:
			img, rows = emulate(c, fault)
			hits += R.check(c, img, rows=rows) > 1
		except AssertionError:
			hits += 1      # a canary: a non-finite owed value, or a write where nothing is owed
	print(f"{kernel} {fault}: caught on {hits} of {applies} cases where it applies")
	assert applies > 0 and hits > 0, fault


def test_operand_conditions_the_gpu_test_relies_on():
	# row-wave: the first-order softmax model holds, the hot case overflows without the maximum and nowhere else, the clamp matters
	for c in R.RW_CASES:
		facts = R.rw_ref(c)[2]
		assert facts["Emax"] < 2.0 ** -6, c.id
		if c.p.hot:
			assert 89.0 < facts["max_lo"] and facts["max_hi"] < 110.0, (c.id, facts)      # every row above ln(FLT_MAX) = 88.72
		else:
			assert facts["max_hi"] < 40.0, (c.id, facts)
		if c.p.bias and c.p.T >= 130:
			rel = torch.arange(c.p.T)[None, :] - torch.arange(c.p.T)[:, None]
			assert float((rel.abs() > 64).float().mean()) >= 0.2, c.id      # T = 130: 25 % of the (q, k) pairs, T = 200: 46 %
			b = R.rw_ops(c)["bias"]
			assert float((b[:, 0] - b[:, 1]).abs().min()) > 1e-2 and float((b[:, 128] - b[:, 127]).abs().min()) > 1e-2      # +-64 and +-63 differ
	assert 4 * R.ROWWAVE_MAX_T * 4 + 4 * 128 * 4 <= 64 * 1024      # the strip of the largest case fits the 64 KiB a workgroup may ask for
	# T-typed operands lie on the bf16 grid
	for c in R.RW_CASES + R.ROT_CASES + R.GEGLU_CASES:
		if c.dt == "bf16":
			o = {"rowwave": R.rw_ops, "rotary": R.rot_ops, "geglu": R.geglu_ops}[c.kernel](c)
			for n in ("q", "k", "v", "qkv", "h"):
				if n in o:
					assert torch.equal(o[n], o[n].bfloat16().float()), (c.id, n)
	# GroupNorm: the offset case has mean 30, deviation 0.1; GEGLU gates cover [-6, 6] and most are not saturated; rotary angles stay below 250
	for c in R.GN_CASES:
		if c.p.offset:
			x = R.gn_ops(c)["x"]
			assert abs(float(x[0].mean()) - 30) < 0.01 and abs(float(x[0].std()) - 0.1) < 0.01
	for c in R.GEGLU_CASES:
		g = R.geglu_ops(c)["h"][:, c.p.inner:]
		assert float(g.min()) <= -5.9 and float(g.max()) >= 5.9 and float((g.abs() < 3).float().mean()) > 0.45 and float(((g < -2.5) & (g > -4)).float().mean()) > 0.05
	assert all(c.p.S <= 250 for c in R.ROT_CASES) and float(R.INV_FREQ.max()) == 1.0
	# RMSNorm and score: one all-zero row each, owed exactly
	for c in R.RMS_CASES:
		if c.p.rows > 1:
			assert not R.rms_ops(c)["x"][3].any() and not R.rms_ref(c)[1][3].any()
	for c in R.SCORE_CASES:
		assert not R.score_ops(c)["speech"][1].any() and float(R.score_ref(c)[1][1]) == 0 and float(R.score_ref(c)[0].abs()[[0, 2]].min()) > 0.2
