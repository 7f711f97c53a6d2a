"""tests/skinny_ref.py checked on the CPU: the float64 reference equals torch's layer_norm / linear / gelu(tanh) in f64, the fragment-order index is the
macro's and a bijection, the fp8 rounding is idempotent and on the e4m3 grid, the float32 emulation of both kernels' arithmetic stays inside the derived
bound on every case test_gpu_skinny_forms.py runs, and every fault the bound and the canaries are there to see is caught on at least one case."""
import collections

import pytest
import torch
import torch.nn.functional as F

import skinny_ref as R



def test_frag_index_is_the_macro_and_a_bijection():
	def macro(row, col, ksteps):      # TTK_FRAG_INDEX of csrc/ttk_common.h, shifts and masks as written there
		return ((((row >> 4) * ksteps + (col >> 5)) * 64 + ((col >> 3) & 3) * 16 + (row & 15)) * 8 + (col & 7))
	for rows, K in ((16, 64), (48, 192), (64, 1088)):
		idx = [R.frag_index(r, c, K // 32) for r in range(rows) for c in range(K)]
		assert idx == [macro(r, c, K // 32) for r in range(rows) for c in range(K)]
		assert sorted(idx) == list(range(rows * K))
	x = torch.arange(37 * 192, dtype=torch.float64).reshape(37, 192)
	back = R.from_frag(R.to_frag(x, 48), 48, 192)
	assert torch.equal(back[:37], x) and torch.isnan(back[37:]).all()


def test_fp8_rounding_is_on_the_grid_and_idempotent():
	w = R.grid(torch.randn(64, 128, generator=torch.Generator().manual_seed(1)), 2.0 ** -3)
	r, s = R.fp8_round_weights(w)
	assert s == 2.0 ** -9 or s == 2.0 ** -10      # absmax of |N(0, 1)| / 8 over 8192 values, / 448, rounded up to a power of two
	assert float(w.abs().max()) / 448 <= s < 2 * float(w.abs().max()) / 448
	q = r / s
	assert torch.equal(q.float().to(torch.float8_e4m3fn).double(), q) and q.abs().max() <= 448
	assert ((r - w).abs() <= 2.0 ** -4 * w.abs() + s * 2.0 ** -10).all()      # half an e4m3 ulp (4 significand bits), subnormal spacing 2^-9
	r2, s2 = R.fp8_round_weights(r)
	assert s2 == s and torch.equal(r2, r) and torch.equal(r.bfloat16().double(), r)


@pytest.mark.parametrize("cid", ["head-f32-K192-w0", "proj-f32-N192-K64", "fold-fc-f32-N256-K64", "fold-qkv-f32-K192", "pro-fc-f32-K192-w4", "pro-head2-f32-K192", "fold-fc-fp8-K192"])
def test_reference_is_torch_in_f64(cid):
	c = next(c for c in R.CASES if c.id == cid)
	o = R.operands(c)
	ref = R.reference(c, o)
	W, b = o["W"], o["bias"]
	if c.form == "plain":
		z = F.linear(o["a"], W, b)
	elif c.form == "fold":
		z = F.linear(F.layer_norm(o["a"], (c.K,), o["gamma"], o["beta"], R.EPS), W, b)
	else:
		y = F.layer_norm(o["x"], (c.K,), o["g1"], o["b1"], R.EPS)
		if c.norms == 2:
			y = F.layer_norm(y, (c.K,), o["g2"], o["b2"], R.EPS)
		z = F.linear(y, W, b)
	want = {"head": {"out_f32": z}, "proj": {"out_f32": o.get("res", 0) + z, "out_T": o.get("res", 0) + z}, "fc": {"out_T": F.gelu(z, approximate="tanh")},
			"qkv": {"qbuf": z[:, :c.K] * 0.125, "k": z[:, c.K:2 * c.K], "v": z[:, 2 * c.K:]}}[c.role]
	for name, (val, tol) in ref.items():
		assert torch.allclose(val, want[name], rtol=1e-11, atol=1e-11), name
		assert (tol > 0).all() and torch.isfinite(tol).all()      # (none of these cases holds a row the fold cannot represent)


def caught(c, M, pos, o, ref, fault):
	try:
		return R.check_outputs(c, M, pos, R.emulate(c, o, M, pos, fault=fault), ref) > 1
	except AssertionError:
		return True      # a canary: a non-finite owed value, or a write where nothing is owed


@pytest.mark.parametrize("group", R.GROUPS)
def test_emulation_is_inside_the_bound_and_faults_are_outside(group):
	worst = 0.0
	for c in (c for c in R.CASES if c.group == group):
		o = R.operands(c)
		ref = R.reference(c, o)
		for M in c.ms():
			for pos in c.pos:
				for fam in ((1, 2) if c.family == 2 else (1,)):
					r = R.check_outputs(c, M, pos, R.emulate(c, o, M, pos, family=fam), ref)
					worst = max(worst, r)
					assert r <= 1, f"{c.id} M={M} pos={pos} family {fam}: the kernel's own arithmetic is {r:.3g}x the bound: the bound misses a term"
		# a row without a bound is a row nothing holds: only the near-constant row of the "fold-unfit" cases may be one
		for name, (val, tol) in ref.items():
			unbounded = ~torch.isfinite(tol).all(1)
			want = torch.zeros_like(unbounded)
			if c.special == "nearconst":
				want[1] = True
			assert torch.equal(unbounded, want) and (tol > 0).all(), f"{c.id} {name}: rows {unbounded.nonzero().flatten().tolist()} have no finite bound"
	print(f"{group}: emulation worst err / bound {worst:.3f}")


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fault_is_caught(fault):
	"""the fault exceeds the bound or breaks a canary on cases where it applies (at the largest M, every position): counted over up to 3 applicable cases per group"""
	applies = hits = 0
	per_group = collections.Counter()
	for c in R.CASES:
		Mf = max(c.ms())
		poss = [pos for pos in c.pos if R.fault_applies(c, fault, Mf, pos)]
		if not poss or per_group[c.group] >= 3:
			continue
		per_group[c.group] += 1
		o = R.operands(c)
		ref = R.reference(c, o)
		for pos in poss:
			applies += 1
			hits += caught(c, Mf, pos, o, ref, fault)
	print(f"{fault}: caught on {hits} of {applies} launches where it applies")
	assert applies > 0 and hits > 0, fault
