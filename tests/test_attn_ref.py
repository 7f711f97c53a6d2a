"""tests/attn_ref.py checked on the CPU: the float64 references equal torch's scaled_dot_product_attention in f64 with an explicit additive mask, the
float32 emulation of the kernels' arithmetic stays inside the derived bound on every case test_gpu_attn_forms.py runs, and every fault the bound
is there to see (a shifted or unsaturated bias bucket, a dropped last key, an admitted padding key, a strict causal mask, a skipped key group,
shared rows from the wrong slice, an ignored start row) exceeds it on every case where the fault changes the definition's result at all."""
import collections

import pytest
import torch
import torch.nn.functional as F

import attn_ref as R

FWD_GROUPS = sorted({c.group for c in R.FWD_CASES})
DEC_GROUPS = sorted({c.group for c in R.DEC_CASES})


def sdpa_mask(c, b, bias):
	"""additive f64 mask [H][T][T] of sequence b: bias, -inf on padding keys and above the causal diagonal"""
	TL = c.tlen[b] if c.tlen else c.T
	i = torch.arange(c.T)
	m = torch.zeros(c.H, c.T, c.T, dtype=torch.float64)
	if bias is not None:
		m = m + bias[:, (i[None, :] - i[:, None]).clamp(-64, 64) + 64]
	dead = (i[None, :] >= TL).expand(c.T, c.T)
	if c.causal:
		dead = dead | (i[None, :] > i[:, None])
	return m.masked_fill(dead[None], float("-inf"))


@pytest.mark.parametrize("case", [R.Fwd("plain", "f32", 2, 3, 70), R.Fwd("causal", "f32", 2, 2, 131, "causal"), R.Fwd("bias", "f32", 1, 2, 150, "bias"),
								  R.Fwd("ragged-bias", "f32", 3, 2, 90, "bias", tlen=(1, 90, 37)), R.Fwd("ragged-causal", "f32", 2, 2, 70, "causal", tlen=(70, 5))],
						 ids=lambda c: c.id)
def test_forward_reference_is_sdpa_in_f64(case):
	c = case
	c.seed = 11
	q, k, v, bias = R.fwd_operands(c)
	ref, tol = R.fwd_reference(c, q, k, v, bias, chunk=32)      # several query chunks
	for b in range(c.nb):
		TL = c.tlen[b] if c.tlen else c.T
		want = F.scaled_dot_product_attention(q[b], k[b], v[b], attn_mask=sdpa_mask(c, b, bias), scale=R.SCALE)      # [H][T][64]
		want = want.permute(1, 0, 2).reshape(c.T, c.H * 64)
		assert torch.allclose(ref[b, :TL], want[:TL], rtol=1e-12, atol=1e-13)
		assert torch.isnan(ref[b, TL:]).all() and torch.isnan(tol[b, TL:]).all()
		assert (tol[b, :TL] > 0).all()


@pytest.mark.parametrize("case", [R.Dec("plain", "f32", 3, 2, 40, 30), R.Dec("clamp", "f32", 2, 2, 20, 25), R.Dec("shared", "f32", 3, 2, 40, 30, 11, 1),
								  R.Dec("lines", "f32", 5, 2, 40, 30, 12, 1, lines=((3, 0), (2, 7)))], ids=lambda c: c.id)
def test_decode_reference_is_sdpa_in_f64(case):
	c = case
	c.seed = 12
	q, kc, vc = R.dec_operands(c)
	ref, _ = R.dec_reference(c, q, kc, vc)
	ri = c.row_info()
	n_end = min(c.pos + 1, c.max_ctx)
	for b in range(c.B):
		start, first = ri[b] if ri else (0, 0)
		sh = c.shared if c.shared_rows else 0
		kk, vv = kc[b].clone(), vc[b].clone()
		kk[:, :sh], vv[:, :sh] = kc[first, :, :sh], vc[first, :, :sh]
		mask = torch.zeros(c.max_ctx, dtype=torch.float64)
		mask[:start] = float("-inf")
		mask[n_end:] = float("-inf")
		want = F.scaled_dot_product_attention(q[b][:, None, :], kk, vv, attn_mask=mask[None, None, :].expand(c.H, 1, -1), scale=1.0)
		assert torch.allclose(ref[b], want.reshape(-1), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("group", FWD_GROUPS)
def test_forward_emulation_is_inside_the_bound_and_every_fault_is_outside(group):
	worst, best_case, seen = 0.0, 0.0, collections.Counter()
	for c in (c for c in R.FWD_CASES if c.group == group):
		ops = R.fwd_operands(c)
		ref, tol = R.fwd_reference(c, *ops)
		emu = R.emulate_fwd(c, *ops)
		r = R.worst_ratio(emu, ref, tol)
		worst = max(worst, r)
		assert r <= 1, f"{c.id}: the kernel's own arithmetic is {r:.3g}x the bound: the bound misses a term"
		assert torch.equal(torch.isnan(emu), torch.isnan(ref))
		if c.nb * c.H * c.T * c.T > 1 << 27:      # the one long case: its emulation alone (each fault would cost as much again)
			continue
		best_case = max(best_case, R.worst_ratio(emu, ref, R.fwd_reference(c, *ops, p_round=R.P_ROUND_BEST_CASE)[1]))
		for fault in R.FWD_FAULTS:
			if R.fwd_fault_applies(c, fault):
				rf = R.worst_ratio(R.emulate_fwd(c, *ops, fault=fault), ref, tol)
				assert rf > 1, f"{c.id}: {fault} stays inside the bound ({rf:.3g}x): the inputs are too tame"
				seen[fault] += 1
	print(f"forward {group}: emulation worst err / tol {worst:.3f} (with P rounding taken as 2^-9 / 2^-12: {best_case:.3f}); faults seen {dict(seen)}")


def test_every_forward_fault_meets_a_case():
	for fault in R.FWD_FAULTS:
		assert any(R.fwd_fault_applies(c, fault) for c in R.FWD_CASES), fault


@pytest.mark.parametrize("group", DEC_GROUPS)
def test_decode_emulation_is_inside_the_bound_and_every_fault_is_outside(group):
	worst, seen = 0.0, collections.Counter()
	for c in (c for c in R.DEC_CASES if c.group == group):
		ops = R.dec_operands(c)
		ref, tol = R.dec_reference(c, *ops)
		for var in c.variants:
			r = R.worst_ratio(R.emulate_dec(c, *ops, variant=var), ref, tol)
			worst = max(worst, r)
			assert r <= 1, f"{c.id} variant {var}: the kernel's own arithmetic is {r:.3g}x the bound: the bound misses a term"
		for fault in R.DEC_FAULTS:
			if R.dec_fault_applies(c, fault):
				rf = R.worst_ratio(R.emulate_dec(c, *ops, variant=c.variants[0], fault=fault), ref, tol)
				assert rf > 1, f"{c.id}: {fault} stays inside the bound ({rf:.3g}x): the inputs are too tame"
				seen[fault] += 1
	print(f"decode {group}: emulation worst err / tol {worst:.3f}; faults seen {dict(seen)}")


def test_every_decode_fault_meets_a_case():
	for fault in R.DEC_FAULTS:
		assert any(R.dec_fault_applies(c, fault) for c in R.DEC_CASES), fault


def test_half_ulp():
	x = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -20, 300.0], dtype=torch.float64)
	assert R.half_ulp(x, "bf16").tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -28, 2.0 ** 0]
	assert R.half_ulp(x, "f16").tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -25, 2.0 ** -3]
	assert R.half_ulp(x, "e4m3").tolist() == [2.0 ** -4, 2.0 ** -4, 2.0 ** -3, 2.0 ** -5, 2.0 ** -10, 2.0 ** 4]
	for fmt, t in (("bf16", torch.bfloat16), ("f16", torch.float16), ("e4m3", torch.float8_e4m3fn)):      # rounding never errs by more
		y = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 3
		assert ((y.float().to(t).double() - y).abs() <= R.half_ulp(y, fmt) + 2.0 ** -24 * y.abs()).all()
