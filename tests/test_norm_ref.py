"""tests/norm_ref.py checked on the CPU: the float64 references equal torch's layer_norm / group_norm (+ modulation, + silu) in f64 and the directly computed
chunk statistics, the fragment-order index is the macro's and a bijection, every bound of every case is finite and positive, the float32 emulation of
k_layernorm, k_gn_stats and k_gn_apply stays inside the derived bound on every case test_gpu_norm_forms.py runs, and every fault the bound and the canaries
are there to see is caught on at least one case."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R


def test_frag_index_is_the_macro_and_a_bijection():
	def macro(row, col, ksteps):      # TTK_FRAG_INDEX of csrc/ttk_common.h, shifts and masks as written there
		return ((((row >> 4) * ksteps + (col >> 5)) * 64 + ((col >> 3) & 3) * 16 + (row & 15)) * 8 + (col & 7))
	for rows, d in ((16, 64), (32, 192), (16, 1056)):
		idx = [R.frag_index(r, c, d // 32) for r in range(rows) for c in range(d)]
		assert idx == [macro(r, c, d // 32) for r in range(rows) for c in range(d)]
		assert sorted(idx) == list(range(rows * d))


def test_case_lists_cover_what_the_kernels_branch_on():
	for ni, ds in ((4, {64, 192, 768, 1024}), (16, {1056, 2048, 4096})):
		cs = [c for c in R.LN_CASES if c.ni == ni]
		assert {c.d for c in cs} == ds and {c.rows for c in cs} == {1, 3, 4, 5, 17}
		assert {c.ldx_extra for c in cs} == {0, 8} and {c.ldo_extra for c in cs if not c.frag} == {0, 8}
		assert {c.norms for c in cs} == {1, 2} and {c.out for c in cs} == {"f32", "bf16", "f16", "bf16-f32out"}
		assert {c.frag for c in cs} == {0, 1} and {c.out2 for c in cs} == {"none", "direct", "ring"}
	for d in (1024, 2048):      # the decode step's launch
		assert any(c.d == d and c.norms == 2 and c.frag and c.out2 == "ring" for c in R.LN_CASES)
	for C in (128, 256, 512, 1024):
		cs = [c for c in R.GN_CASES if c.C == C]
		Rr = 65536 // C
		assert {1, 3} <= {c.nb for c in cs}
		assert any(c.T < Rr for c in cs) and any(c.T == Rr for c in cs) and any(c.T == Rr + 1 and not c.Tout for c in cs)
		assert any(c.nchunks > 8 and c.T % Rr == 1 for c in cs) and any(c.nchunks > 24 for c in cs)
		assert any(c.tlen and 1 in c.tlen and any(t % Rr == 0 for t in c.tlen) for c in cs)
		assert any(c.Tout > c.T for c in cs) and any(0 < c.Tout < c.T for c in cs)
	assert (128, 4609) in {(c.C, c.T) for c in R.GN_CASES} and (1024, 1601) in {(c.C, c.T) for c in R.GN_CASES}
	assert [c.nb for c in R.GN_CASES if c.nchunks == 64] == [1]
	vs = [v for c in R.GN_CASES for v in c.variants]
	assert {v[0] for v in vs} == set(R.OUT_KINDS) and {v[1] for v in vs} == set(R.GN_MODS) and {v[2] for v in vs} == {0, 2}


@pytest.mark.parametrize("c", [c for c in R.LN_CASES if c.d in (192, 1056)], ids=lambda c: c.id)
def test_layernorm_reference_is_torch_in_f64(c):
	o, y, dy32, dyo = R.ln_reference(c)
	want = F.layer_norm(o["x"].double(), (c.d,), o["g1"].double(), o["b1"].double(), R.EPS)
	if c.norms == 2:
		want = F.layer_norm(want, (c.d,), o["g2"].double(), o["b2"].double(), R.EPS)
	assert torch.allclose(y, want, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("c", [c for c in R.GN_CASES if c.C in (128, 512) and c.nchunks <= 10], ids=lambda c: c.id)
def test_groupnorm_reference_is_torch_in_f64(c):
	o, st = R.gn_statistics(c)
	x = o["x"].double()
	Rr, cpg = c.chunk_rows, c.C // 32
	for b, Tl in enumerate(c.lens()):      # the triples against count / mean / sum (x - mean)^2 computed directly
		for ch in range(c.nchunks):
			rows = x[b, ch * Rr:min(Tl, ch * Rr + Rr)]
			assert bool(st["valid"][b, 0, ch]) == (rows.shape[0] > 0)
			for g in (0, 13, 31):
				blk = rows[:, g * cpg:(g + 1) * cpg]
				if blk.numel():
					assert st["cnt"][b, g, ch] == blk.numel() == rows.shape[0] * c.C // 32
					assert abs(st["mean"][b, g, ch] - blk.sum() / blk.numel()) <= 1e-11 and abs(st["m2"][b, g, ch] - ((blk - blk.sum() / blk.numel()) ** 2).sum()) <= 1e-11 * blk.numel()
	for variant in c.variants:
		kind, mod, act = variant
		y, tol = R.gn_reference(c, variant)
		for b, Tl in enumerate(c.lens()):
			want = F.group_norm(x[b, :Tl].t()[None], 32, o["gamma"].double(), o["beta"].double(), R.EPS)[0].t()
			if R.GN_MODS[mod][0]:
				m = o["mod"].double()[b if R.GN_MODS[mod][1] else 0]
				want = want * (1 + m[:c.C]) + m[c.C:]
			if act == 2:
				want = F.silu(want)
			if c.Tout:
				want = F.interpolate(want.t()[None], size=c.Tout, mode="nearest")[0].t()
			assert torch.allclose(y[b, :None if c.Tout else Tl], want, rtol=1e-11, atol=1e-11), variant
			assert not y[b, Tl:].any() if not c.Tout else True


@pytest.mark.parametrize("group", R.GROUPS)
def test_emulation_is_inside_the_bound_and_every_bound_is_finite(group):
	worst = {}
	for c in (c for c in R.LN_CASES if c.group == group):
		_, y, dy32, dyo = R.ln_reference(c)
		for tol in (dy32, dyo):
			assert torch.isfinite(tol).all() and (tol > 0).all(), f"{c.id}: an element without a finite bound"
		assert float((y.abs() + dyo).max()) < 448
		for k, r in R.ln_check(c, R.ln_emulate(c)).items():
			assert r <= 1, f"{c.id}: the kernel's own arithmetic is {r:.3g}x the bound on {k}: the bound misses a term"
			worst[k] = max(worst.get(k, 0.0), r)
	for c in (c for c in R.GN_CASES if c.group == group):
		o, st = R.gn_statistics(c)
		for k in ("dmean", "dm2"):
			assert torch.isfinite(st[k]).all() and (st[k][st["valid"]] > 0).all(), f"{c.id}: a statistic without a finite bound"
		ms = R.gn_emulate_stats(c, o)
		for variant in c.variants:
			y, tol = R.gn_reference(c, variant)
			assert torch.isfinite(tol).all() and (tol >= 0).all() and float((y.abs() + tol).max()) < 448, f"{c.id} {variant}: an element without a finite bound"
			for b, Tl in enumerate(c.lens()):
				assert (tol[b, :None if c.Tout else Tl] > 0).all()
			w = R.gn_check(c, variant, *R.gn_emulate(c, variant, stats=(o, ms)), ref=(y, tol))
			for k, r in w.items():
				assert r <= 1, f"{c.id} {variant}: the kernel's own arithmetic is {r:.3g}x the bound on {k}: the bound misses a term"
				worst[k] = max(worst.get(k, 0.0), r)
	print(f"{group}: emulation worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("fault", R.LN_FAULTS)
def test_layernorm_fault_is_caught(fault):
	applies = hits = 0
	for c in R.LN_CASES:
		if not R.ln_fault_applies(c, fault) or c.d > 2048:
			continue
		applies += 1
		try:
			hits += max(R.ln_check(c, R.ln_emulate(c, fault)).values()) > 1
		except AssertionError:
			hits += 1      # a canary: a non-finite owed value, or a write where nothing is owed
	print(f"{fault}: caught on {hits} of {applies} cases where it applies")
	assert applies > 0 and hits > 0, fault


@pytest.mark.parametrize("fault", R.GN_FAULTS)
def test_groupnorm_fault_is_caught(fault):
	"""over the cases of at most 10 chunks where the fault applies (the long ones add nothing a short one does not show)"""
	applies = hits = 0
	for c in R.GN_CASES:
		if c.nchunks > 10:
			continue
		for variant in c.variants:
			if not R.gn_fault_applies(c, variant, fault):
				continue
			applies += 1
			try:
				hits += max(R.gn_check(c, variant, *R.gn_emulate(c, variant, fault)).values()) > 1
			except AssertionError:
				hits += 1
	print(f"{fault}: caught on {hits} of {applies} launches where it applies")
	assert applies > 0 and hits > 0, fault
