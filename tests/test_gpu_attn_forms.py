"""Every launch form of the attention kernels (csrc/attn.hip) through `ttk_attn_fwd` / `ttk_attn_decode` against the float64 reference and the derived
bound of tests/attn_ref.py (where the bound's model is written out and tests/test_attn_ref.py shows on the CPU that it sees a subtle fault).

Forward: each case runs form 0 (the launcher's choice) and every explicit form that is legal for it -- 64-query blocks, 128-query blocks, 8 waves x 16
queries, balanced -- on the same operands.  The code says every form computes a 16-query tile with the same arithmetic (attn.hip at NWV = 9, at the XCD
remap and at the per-16-query band test): all forms must give the same bits, form 0 must give the bits of the form the launcher is meant to choose at
that shape, and each sequence of a ragged batch the bits of a batch of its own length.  Decode: the three (waves, unroll) variants, row_info,
shared_rows, the fragment-order output and the position line; variants sum in different orders and are compared through the bound only.

`out` starts as NaN with canary rows and padding columns: what the kernel owes must be finite and inside the bound, everything else must still be
NaN.  Rows of qkv past tlen[b], cache rows outside [start, pos] and the private copies of shared-prefix rows are NaN: a kernel that reads them and
merely masks them fails.  One process, no environment knobs."""
import ctypes as C
import collections
import hashlib
import time

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
DT = {"f32": 0, "bf16": 1, "f16": 4}
CANARY_ROWS = 16
DEV = "cuda:0"
RATIOS = collections.defaultdict(float)      # case group -> worst err / tol seen (printed by the last test)


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def digest(t):
	return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def nan_like(shape, dtype):
	if dtype == torch.uint8:
		return torch.full(shape, 0x7F, device=DEV, dtype=torch.uint8)      # e4m3 NaN
	return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def is_nan(t):
	return (t & 0x7F) == 0x7F if t.dtype == torch.uint8 else torch.isnan(t)


# ----------------------------------------------------------------------------------------------------------- forward
def fwd_buffers(c, q, k, v, tlen):
	"""qkv [nb*T][ld] of the kernel's type in the case's layout, rows past tlen[b] NaN"""
	tdt = R.TDT[c.dt]
	frag = 4 if c.dt == "f32" else 8
	if c.layout == "gpt":
		ld, hs, offs = 3 * 64 * c.H, 64, (0, 64 * c.H, 2 * 64 * c.H)
	else:
		ld, hs, offs = 3 * 64 * c.H + frag, 192, (0, 64, 128)
	qkv = torch.full((c.nb, c.T, ld), float("nan"), dtype=tdt)
	for x, off in zip((q, k, v), offs):
		for h in range(c.H):
			qkv[:, :, off + h * hs: off + h * hs + 64] = x[:, h].to(tdt)
	if tlen:
		for b, tl in enumerate(tlen):
			qkv[b, tl:] = float("nan")
	return qkv.view(c.nb * c.T, ld).to(DEV), ld, hs, offs


def run_fwd(lib, c, qkv, ld, hs, offs, bias_d, tlen_d, form, nb=None, T=None, row0=0):
	"""one launch; returns (out [nb][T][64 H] on the CPU, stray) -- stray: something outside the owed rows and columns was written"""
	l, _lib = lib
	nb, T = nb or c.nb, T or c.T
	ldo = 64 * c.H + 8
	odt = torch.uint8 if c.f8 else R.TDT[c.dt]
	out = nan_like((nb * T + CANARY_ROWS, ldo), odt)
	d = _lib.AttnDesc()
	d.qkv = qkv.data_ptr() + row0 * ld * qkv.element_size()
	d.ld, d.q_off, d.k_off, d.v_off, d.head_stride = ld, offs[0], offs[1], offs[2], hs
	d.out, d.ldo, d.out_f8 = out.data_ptr(), ldo, int(c.f8)
	d.nb, d.T, d.H, d.causal = nb, T, c.H, int(c.causal)
	d.tlen = tlen_d.data_ptr() if tlen_d is not None else None
	d.bias = bias_d.data_ptr() if bias_d is not None else None
	d.scale, d.form = R.SCALE, form
	rc = l.ttk_attn_fwd(DT[c.dt], C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id} form {form}: ttk_attn_fwd refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	stray = bool((~is_nan(out[nb * T:])).any()) or bool((~is_nan(out[:nb * T, 64 * c.H:])).any())
	return out[:nb * T, :64 * c.H].cpu().view(nb, T, 64 * c.H), stray


def decode_f8(t):
	return t.view(torch.float8_e4m3fn).double()


@pytest.mark.parametrize("case", R.FWD_CASES, ids=[c.id for c in R.FWD_CASES])
def test_forward_form_against_f64(lib, case):
	c = case
	t0 = time.time()
	q, k, v, bias = R.fwd_operands(c)
	ref, tol = R.fwd_reference(c, q, k, v, bias)
	t_ref = time.time() - t0
	qkv, ld, hs, offs = fwd_buffers(c, q, k, v, c.tlen)
	bias_d = bias.float().to(DEV).contiguous() if bias is not None else None
	tlen_d = torch.tensor(c.tlen, dtype=torch.int32, device=DEV) if c.tlen else None
	owed = ~torch.isnan(ref)
	outs = {}
	for form in (0,) + c.legal_forms():
		out, stray = run_fwd(lib, c, qkv, ld, hs, offs, bias_d, tlen_d, form)
		assert not stray, f"{c.id} form {form}: a canary row or a padding column of out was written"
		assert is_nan(out)[~owed].all(), f"{c.id} form {form}: rows past tlen[b] were written"
		got = decode_f8(out) if c.f8 else out.double()
		assert torch.isfinite(got[owed]).all(), f"{c.id} form {form}: non-finite outputs (unwritten values, or padding read) at {(~torch.isfinite(got) & owed).nonzero()[:5].tolist()}"
		r = R.worst_ratio(got, ref, tol)
		RATIOS["fwd " + c.group] = max(RATIOS["fwd " + c.group], r)
		print(f"{c.id} form {form}: err / tol {r:.3f} (reference {t_ref:.2f} s)")
		if r > 1:
			i = int(((got - ref).abs() / tol).masked_fill(~owed, 0).argmax())
			b, rem = divmod(i, c.T * 64 * c.H)
			row, col = divmod(rem, 64 * c.H)
			pytest.fail(f"{c.id} form {form}: |got - ref| is {r:.3g}x the bound at sequence {b} row {row} head {col // 64} dim {col % 64}: got {got[b, row, col].item()!r} "
						f"ref {ref[b, row, col].item()!r} tol {tol[b, row, col].item():.3g}")
		outs[form] = out
	d0 = digest(outs[0].masked_fill(~owed, 0))
	for form, out in outs.items():
		assert digest(out.masked_fill(~owed, 0)) == d0, (f"{c.id}: form {form} is inside the bound but does not give form 0's bits "
			f"(max |diff| {((decode_f8(out) if c.f8 else out.double()) - (decode_f8(outs[0]) if c.f8 else outs[0].double()))[owed].abs().max().item():.3g}): every form computes a 16-query tile the same way")
	if c.expect0:
		assert c.expect0 in outs      # the launcher's choice at this shape is among the forms that ran, with form 0's bits
	if c.tlen:      # each sequence alone, as a batch of its own length: the same bits
		for b, tl in enumerate(c.tlen):
			alone, stray = run_fwd(lib, c, qkv, ld, hs, offs, bias_d, None, 0, nb=1, T=tl, row0=b * c.T)
			assert not stray
			assert digest(alone[0]) == digest(outs[0][b, :tl]), f"{c.id}: sequence {b} (tlen {tl}) of the ragged batch does not have the bits of a batch of its own length"


def test_form0_is_the_launchers_choice():
	"""the shapes of the balanced and the 128-query cases are the ones where attn.hip's launcher picks those forms (its conditions restated)"""
	for c in R.FWD_CASES:
		if not c.expect0:
			continue
		big = (c.T + 127) // 128 * c.H * c.nb >= 512
		G, tiles = 256 // (c.nb * c.H), (c.T + 15) // 16
		bal = not c.causal and not c.tlen and 256 % (c.nb * c.H) == 0 and (tiles + G - 1) // G <= 9 and tiles // G >= 6
		assert (4 if bal else (2 if big else 1)) == c.expect0, c.id


# ----------------------------------------------------------------------------------------------------------- decode
def frag_index(H, b, n):
	return ((((b >> 4) * (H * 64 // 32) + (n >> 5)) * 64 + ((n >> 3) & 3) * 16 + (b & 15)) * 8 + (n & 7))


def run_dec(lib, c, q, kc, vc, variant, out_frag=False, pos_line=False, row_info="case", shared_rows=None, pos=None, shared=None):
	"""one launch; returns (out [B][64 H] on the CPU, stray)"""
	l, _lib = lib
	tdt = R.TDT[c.dt]
	B = q.shape[0]
	d_pos = torch.tensor([c.pos if pos is None else pos, c.shared if shared is None else shared], dtype=torch.int32, device=DEV)
	ri = c.row_info() if row_info == "case" else row_info
	ri_d = torch.tensor(ri, dtype=torch.int32, device=DEV) if ri else None
	n = 64 * c.H
	rows = (B + 15) // 16 * 16 if out_frag else B
	out = nan_like((rows * n + 256,), tdt)
	qd, kd, vd = q.float().to(DEV).contiguous(), kc.to(tdt).to(DEV).contiguous(), vc.to(tdt).to(DEV).contiguous()
	d = _lib.AttnDecodeDesc()
	d.qbuf, d.kcache, d.vcache, d.d_pos = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), d_pos.data_ptr()
	d.B, d.H, d.max_ctx, d.out_frag, d.out = B, c.H, kc.shape[2], int(out_frag), out.data_ptr()
	d.row_info = ri_d.data_ptr() if ri_d is not None else None
	d.shared_rows, d.variant, d.pos_line = c.shared_rows if shared_rows is None else shared_rows, variant, int(pos_line)
	rc = l.ttk_attn_decode(DT[c.dt], C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id} variant {variant}: ttk_attn_decode refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	o = out.cpu()
	if out_frag:
		idx = torch.tensor([[frag_index(c.H, b, e) for e in range(n)] for b in range(B)])
		got = o[idx]
		rest = torch.ones(o.numel(), dtype=torch.bool)
		rest[idx.view(-1)] = False
		stray = bool((~torch.isnan(o[rest])).any())      # rows >= B of the last 16-row tile and what follows
	else:
		got, stray = o[:B * n].view(B, n), bool((~torch.isnan(o[B * n:])).any())
	return got, stray


def poisoned_cache(c, kc, vc):
	"""the caches with NaN in every row the definition does not read: before start, past pos, past the cache's end nothing exists; the private copies
	of shared rows in candidates other than their line's first"""
	kc, vc = kc.clone(), vc.clone()
	n_end = min(c.pos + 1, c.max_ctx)
	ri = c.row_info()
	for b in range(c.B):
		start, first = ri[b] if ri else (0, 0)
		for x in (kc, vc):
			x[b, :, :start] = float("nan")
			x[b, :, n_end:] = float("nan")
			if c.shared_rows and b != first:
				x[b, :, start:c.shared] = float("nan")
	return kc, vc


@pytest.mark.parametrize("case", R.DEC_CASES, ids=[c.id for c in R.DEC_CASES])
def test_decode_variant_against_f64(lib, case):
	c = case
	q, kc, vc = R.dec_operands(c)
	ref, tol = R.dec_reference(c, q, kc, vc)
	kp, vp = poisoned_cache(c, kc, vc)
	for variant in c.variants:
		for out_frag in (False, True):
			got, stray = run_dec(lib, c, q, kp, vp, variant, out_frag=out_frag)
			what = f"{c.id} variant {variant}{' out_frag' if out_frag else ''}"
			assert not stray, f"{what}: something outside the owed outputs was written"
			assert torch.isfinite(got.double()).all(), f"{what}: non-finite outputs (unwritten values, or rows outside [start, pos] or private shared rows read)"
			r = R.worst_ratio(got.double(), ref, tol)
			RATIOS["dec " + c.group] = max(RATIOS["dec " + c.group], r)
			print(f"{what}: err / tol {r:.3f}")
			assert r <= 1, f"{what}: |got - ref| is {r:.3g}x the bound at (candidate, column) {divmod(int(((got.double() - ref).abs() / tol).argmax()), 64 * c.H)}"
			if not out_frag:
				base = got
			else:
				assert digest(got) == digest(base), f"{what}: the fragment-order output holds other bits than the row-major one"
		line, stray = run_dec(lib, c, q, kp, vp, variant, pos_line=True)
		assert not stray and digest(line) == digest(base), f"{c.id} variant {variant}: the position line gives other bits than d_pos"
	if c.lines:      # each candidate on its own contiguous keys through the plain variant: the same bits
		sh = c.shared if c.shared_rows else 0
		ri = c.row_info()
		for variant in c.variants:
			rowsv, _ = run_dec(lib, c, q, kp, vp, variant)
			for b in range(c.B):
				start, fst = ri[b]
				n = min(c.pos + 1, c.max_ctx) - start
				kk, vv = kc[b:b + 1, :, start:start + n].clone(), vc[b:b + 1, :, start:start + n].clone()
				kk[0, :, :max(sh - start, 0)], vv[0, :, :max(sh - start, 0)] = kc[fst, :, start:max(sh, start)], vc[fst, :, start:max(sh, start)]
				alone, _ = run_dec(lib, c, q[b:b + 1], kk, vv, variant, row_info=None, shared_rows=0, pos=n - 1, shared=0)
				assert digest(alone[0]) == digest(rowsv[b]), f"{c.id} variant {variant}: candidate {b} differs in bits from the plain variant on its own contiguous keys"


# ----------------------------------------------------------------------------------------------------------- refusals
def test_preconditions_are_refused(lib):
	"""what the kernels take for granted comes back as TTK_E_ARG with a message"""
	l, _lib = lib
	qkv = torch.zeros(256, 3 * 64 * 16 + 8, device=DEV, dtype=torch.bfloat16)
	out = torch.zeros(256, 64 * 16 + 8, device=DEV, dtype=torch.bfloat16)
	aux = torch.zeros(16 * 129, device=DEV)
	tl = torch.ones(16, device=DEV, dtype=torch.int32)

	def fdesc(**kw):
		d = _lib.AttnDesc()
		d.qkv, d.ld, d.q_off, d.k_off, d.v_off, d.head_stride = qkv.data_ptr(), 384, 0, 128, 256, 64
		d.out, d.ldo, d.nb, d.T, d.H, d.scale = out.data_ptr(), 128, 2, 100, 2, 0.125
		for k, v in kw.items():
			setattr(d, k, v)
		return d

	def refused(d, match, dt=1, fn=None):
		assert (fn or l.ttk_attn_fwd)(dt, C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	assert l.ttk_attn_fwd(1, C.byref(fdesc()), _lib.stream_ptr()) == 0      # the base descriptor itself is fine
	refused(fdesc(qkv=None), "null")
	refused(fdesc(out=None), "null")
	refused(fdesc(T=0), "T >= 1")
	refused(fdesc(nb=0), "nb >= 1")
	refused(fdesc(H=0), "H >= 1")
	refused(fdesc(ld=388), "multiples of 8")
	refused(fdesc(q_off=4), "multiples of 8")
	refused(fdesc(k_off=132), "multiples of 8")
	refused(fdesc(v_off=260), "multiples of 8")
	refused(fdesc(head_stride=68), "multiples of 8")
	refused(fdesc(q_off=2, ld=386), "multiples of 4", dt=0)
	refused(fdesc(qkv=qkv.data_ptr() + 8), "16-byte aligned")
	refused(fdesc(ldo=127), "ldo < 64 H")
	refused(fdesc(out_f8=1), "out_f8 only with TTK_BF16", dt=4)
	refused(fdesc(out_f8=1), "out_f8 only with TTK_BF16", dt=0)
	refused(fdesc(causal=1, bias=aux.data_ptr()), "causal together with bias")
	refused(fdesc(), "dtype", dt=3)
	refused(fdesc(form=5), "form must be")
	refused(fdesc(form=3, causal=1), "form 3")
	refused(fdesc(form=4, causal=1), "form 4")
	refused(fdesc(form=4, tlen=tl.data_ptr()), "form 4")
	refused(fdesc(form=4, nb=3), "256 % (nb * H)")      # nb * H = 6
	refused(fdesc(form=4, nb=8, H=16, ld=3080, q_off=0, k_off=1024, v_off=2048, ldo=1032, T=16 * 9 * 2 + 1), "at most 9")      # G = 2, 19 tiles
	assert l.ttk_attn_fwd(1, C.byref(fdesc(form=4, nb=1, H=16, ld=3080, k_off=1024, v_off=2048, ldo=1032, T=256)), _lib.stream_ptr()) == 0      # G = 16, one tile each: legal

	qb = torch.zeros(2 * 16 * 64 + 8, device=DEV)
	kc = torch.zeros(2 * 16 * 32 * 64 + 8, device=DEV, dtype=torch.bfloat16)
	dp = torch.tensor([5, 0, 0, 0], device=DEV, dtype=torch.int32)
	ob = torch.zeros(16 * 16 * 64, device=DEV, dtype=torch.bfloat16)

	def ddesc(**kw):
		d = _lib.AttnDecodeDesc()
		d.qbuf, d.kcache, d.vcache, d.d_pos, d.B, d.H, d.max_ctx, d.out = qb.data_ptr(), kc.data_ptr(), kc.data_ptr(), dp.data_ptr(), 2, 16, 32, ob.data_ptr()
		for k, v in kw.items():
			setattr(d, k, v)
		return d
	dec = l.ttk_attn_decode
	assert dec(1, C.byref(ddesc()), _lib.stream_ptr()) == 0
	for name in ("qbuf", "kcache", "vcache", "d_pos", "out"):
		refused(ddesc(**{name: None}), "null", fn=dec)
	refused(ddesc(B=0), "B >= 1", fn=dec)
	refused(ddesc(H=0), "H >= 1", fn=dec)
	refused(ddesc(max_ctx=0), "max_ctx >= 1", fn=dec)
	refused(ddesc(kcache=kc.data_ptr() + 8), "16-byte aligned", fn=dec)
	refused(ddesc(d_pos=dp.data_ptr() + 4), "8-byte aligned", fn=dec)
	refused(ddesc(variant=3), "variant must be", fn=dec)
	refused(ddesc(variant=1), "bf16 only", dt=4, fn=dec)
	refused(ddesc(variant=2), "bf16 only", dt=0, fn=dec)
	refused(ddesc(), "dtype", dt=3, fn=dec)
	torch.cuda.synchronize()


def test_zz_report(lib):
	"""(runs last in this module) the worst err / tol per case group, for the record"""
	for k in sorted(RATIOS):
		print(f"worst err / tol, {k}: {RATIOS[k]:.3f}")
	assert all(v <= 1 for v in RATIOS.values())
