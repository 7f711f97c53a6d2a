"""The side networks' own kernels on caller-provided operands -- k_cond_gn and k_attn_rowwave (csrc/ttk_attn_block.h: the AttentionBlock of the conditioning encoders
and the classifier), k_cond_im2col and k_cond_pool (csrc/cond.hip), k_embed_rows, k_rmsnorm, k_rotary, k_geglu, k_mean_rows and k_clvp_score (csrc/clvp.hip) --
through the entry points of include/ttk.h that run the product's own launch functions, against the float64 references and the derived per-element bounds of
tests/side_ref.py (where the bounds are written out and tests/test_side_ref.py shows on the CPU that they and the canaries see a subtle fault).

Every output buffer starts as NaN with TAIL canary elements behind it; the pad columns of strided rows (the row-wave's qkv and out) and the text rows a Bt = 1 score
must not read are NaN as well.  What a launch owes must be finite and inside the bound (equal, byte for byte, where the kernel only moves data), everything else must
still be NaN.  No element is exempt.  Every buffer is sized from the case before the launch.  One process, no environment knobs."""
import collections
import ctypes as C

import pytest
import torch

import side_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = collections.defaultdict(float)      # case group -> worst err / bound seen (printed by the last test)
TAIL = 256                                   # canary elements behind a flat buffer
IDS = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def nan_buffer(n, dt):
	return torch.full((n + TAIL,), float("nan"), dtype=R.TDT[dt], device=DEV)


def filled(values, dt):
	"""a NaN buffer whose first elements are `values` (f32 values of T), for inputs and for the in-place rotary"""
	buf = nan_buffer(values.numel(), dt)
	buf[:values.numel()] = values.reshape(-1).to(DEV).to(R.TDT[dt])
	return buf


def read_back(buf, n):
	"""the first n elements as f64 on the host; the canary tail must still be NaN"""
	t = buf.cpu().float().double()
	assert torch.isnan(t[n:]).all(), "the canary elements behind a buffer were written"
	return t[:n]


def same_bytes(got, want_values, what):
	"""got: device tensor of T; want_values: the f32 values owed.  Equality of bytes, no tolerance."""
	want = want_values.to(got.dtype)
	ity = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
	assert torch.equal(got.cpu().view(ity), want.view(ity)), f"{what}: not the bytes owed"


def ok(lib, rc, c):
	assert rc == 0, f"{c.id}: refused: {lib[0].ttk_last_error().decode()}"
	torch.cuda.synchronize()


def record(c, r):
	RATIOS[c.group] = max(RATIOS[c.group], r)
	print(f"{c.id}: err / bound {r:.3f}")
	assert r <= 1, f"{c.id}: |got - ref| is {r:.3g}x the bound"


def refusals(lib, call, base, cases, outs):
	"""call(**base) succeeds; call(**{**base, **kw}) returns TTK_E_ARG with `match` in the message for every (kw, match); nothing was launched into `outs` before the
	one good call at the end"""
	l, _ = lib
	for kw, match in cases:
		assert call(**{**base, **kw}) == -1, (kw, match)
		assert match in l.ttk_last_error().decode(), (kw, l.ttk_last_error().decode())
	torch.cuda.synchronize()
	for o in outs:
		assert bool(torch.isnan(o).all()), "a refused call launched something"
	assert call(**base) == 0, l.ttk_last_error().decode()
	torch.cuda.synchronize()
	for o in outs:
		assert bool(torch.isfinite(o[:-TAIL]).any()) and bool(torch.isnan(o[-TAIL:]).all())


# ----------------------------------------------------------------------------------------------------------- k_cond_gn
@pytest.mark.parametrize("c", R.GN_CASES, ids=IDS(R.GN_CASES))
def test_block_groupnorm_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.gn_ops(c)
	x, gamma, beta = (o[k].to(DEV).contiguous() for k in ("x", "gamma", "beta"))
	n = p.nb * p.T * p.C
	out = nan_buffer(n, c.dt)
	ok(lib, l.ttk_block_gn_rows(R.DT_CODE[c.dt], x.data_ptr(), p.nb, p.T, p.C, p.groups, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, n).view(p.nb, p.T, p.C)))


def test_block_groupnorm_preconditions_are_refused(lib):
	l, _lib = lib
	x, v, out = torch.zeros(2 * 5 * 48 + 4, device=DEV), torch.ones(48 + 4, device=DEV), nan_buffer(2 * 5 * 48, "f32")
	call = lambda dt=0, x=x.data_ptr(), nb=2, T=5, C=48, groups=16, gamma=v.data_ptr(), beta=v.data_ptr(), out=out.data_ptr(): \
		l.ttk_block_gn_rows(dt, x, nb, T, C, groups, gamma, beta, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"dt": 4}, "dtype"), ({"dt": 2}, "dtype"), ({"x": None}, "null"), ({"gamma": None}, "null"), ({"beta": None}, "null"), ({"out": None}, "null"),
							 ({"groups": 5}, "not a multiple"), ({"groups": 0}, "out of range"), ({"T": 0}, "out of range"), ({"nb": 0}, "out of range"), ({"nb": 65536}, "out of range"),
							 ({"C": 0}, "out of range"), ({"x": x.data_ptr() + 2}, "misaligned"), ({"out": out.data_ptr() + 1, "dt": 1}, "misaligned")], [out])


# ----------------------------------------------------------------------------------------------------------- k_attn_rowwave
def rowwave_desc(_lib, c, qkv, out, bias):
	p = c.p
	ld, ldo, qo, ko, vo, hs = R.rw_layout(c)
	d = _lib.AttnDesc()
	d.qkv, d.ld, d.q_off, d.k_off, d.v_off, d.head_stride = qkv.data_ptr(), ld, qo, ko, vo, hs
	d.out, d.ldo, d.nb, d.T, d.H, d.scale = out.data_ptr(), ldo, p.nb, p.T, p.H, R.SCALE128
	d.bias = bias.data_ptr() if bias is not None else None
	return d


@pytest.mark.parametrize("c", R.RW_CASES, ids=IDS(R.RW_CASES))
def test_rowwave_attention_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.rw_ops(c)
	ld, ldo, *_ = R.rw_layout(c)
	qkv = filled(R.rw_pack(c, o), c.dt)      # exactly nb * T * ld elements, NaN between the rows' heads and the next row, NaN behind
	bias = o["bias"].to(DEV).contiguous() if o["bias"] is not None else None
	n = p.nb * p.T * ldo
	out = nan_buffer(n, c.dt)
	ok(lib, l.ttk_attn_rowwave(R.DT_CODE[c.dt], C.byref(rowwave_desc(_lib, c, qkv, out, bias)), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, n).view(p.nb * p.T, ldo)))


def test_rowwave_attention_preconditions_are_refused(lib):
	l, _lib = lib
	c = next(c for c in R.RW_CASES if c.p.T == 5 and c.p.bias and c.dt == "f32")
	big = R.ROWWAVE_MAX_T + 1
	qkv = torch.zeros(max(2 * 5 * 768, big * 768) + 16, device=DEV)      # room for every shape a refused descriptor names
	bias = torch.zeros(2 * 129 + 4, device=DEV)
	out = nan_buffer(max(2 * 5 * 256, big * 256), "f32")

	def call(dt=0, null=False, **kw):
		d = rowwave_desc(_lib, c, qkv, out, bias)
		for k, v in kw.items():
			setattr(d, k, v)
		return l.ttk_attn_rowwave(dt, None if null else C.byref(d), _lib.stream_ptr())
	tl = torch.ones(2, dtype=torch.int32, device=DEV)
	refusals(lib, call, {}, [({"null": True}, "null descriptor"), ({"dt": 4}, "dtype"), ({"dt": 3}, "dtype"), ({"qkv": None}, "null"), ({"out": None}, "null"),
							 ({"causal": 1}, "not served"), ({"tlen": tl.data_ptr()}, "not served"), ({"out_f8": 1}, "not served"), ({"form": 1}, "not served"),
							 ({"T": big, "nb": 1, "H": 1}, "outside 1.."), ({"T": 0}, "outside 1.."), ({"nb": 0}, "out of range"), ({"H": 0}, "out of range"),
							 ({"head_stride": 64}, "head_stride < 128"), ({"k_off": -8}, "negative offset"), ({"ld": 760}, "does not hold"), ({"v_off": 264}, "does not hold"),
							 ({"ldo": 255}, "ldo ="), ({"qkv": qkv.data_ptr() + 16}, "8 elements"), ({"ld": 772}, "8 elements"), ({"k_off": 132}, "8 elements"),
							 ({"head_stride": 380, "H": 1}, "8 elements"), ({"out": out.data_ptr() + 2}, "misaligned"), ({"bias": bias.data_ptr() + 2}, "misaligned"),
							 ({"out": qkv.data_ptr() + 32}, "overlap")], [out])


# ----------------------------------------------------------------------------------------------------------- k_cond_im2col (exact)
@pytest.mark.parametrize("c", R.IM_CASES, ids=IDS(R.IM_CASES))
def test_im2col_gives_the_bytes_owed(lib, c):
	l, _lib = lib
	p, o = c.p, R.im_ops(c)
	src = o["src"].to(DEV)
	n = p.nb * p.Tout * p.Kpad
	out = nan_buffer(n, c.dt)
	ok(lib, l.ttk_cond_im2col_rows(R.DT_CODE[c.dt], src.data_ptr(), o["sb"], o["sc"], o["st"], p.nb, p.Cin, p.Tin, p.Tout, p.taps, p.stride, p.pad, p.Kpad, out.data_ptr(),
									_lib.stream_ptr()), c)
	y, _ = R.im_ref(c)
	record(c, R.check(c, read_back(out, n).view(p.nb * p.Tout, p.Kpad), ref=(y, torch.zeros_like(y))))
	same_bytes(out[:n], y.float().reshape(-1), c.id)


def test_im2col_preconditions_are_refused(lib):
	l, _lib = lib
	src, out = torch.ones(2 * 5 * 5 + 4, device=DEV), nan_buffer(2 * 3 * 32, "f32")
	call = lambda dt=0, src=src.data_ptr(), sb=25, sc=5, st=1, nb=2, Cin=5, Tin=5, Tout=3, taps=3, stride=2, pad=1, Kpad=32, out=out.data_ptr(): \
		l.ttk_cond_im2col_rows(dt, src, sb, sc, st, nb, Cin, Tin, Tout, taps, stride, pad, Kpad, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"dt": 4}, "dtype"), ({"src": None}, "null"), ({"out": None}, "null"), ({"Kpad": 14}, "Kpad ="), ({"nb": 0}, "out of range"), ({"Cin": 0}, "out of range"),
							 ({"Tin": 0}, "out of range"), ({"Tout": 0}, "out of range"), ({"taps": 0}, "out of range"), ({"stride": 0}, "out of range"), ({"pad": -1}, "out of range"),
							 ({"sc": 0}, "strides"), ({"st": -1}, "strides"), ({"sb": -25}, "strides"), ({"src": src.data_ptr() + 2}, "misaligned"),
							 ({"out": out.data_ptr() + 1, "dt": 1}, "misaligned")], [out])


# ----------------------------------------------------------------------------------------------------------- k_cond_pool
@pytest.mark.parametrize("c", R.POOL_CASES, ids=IDS(R.POOL_CASES))
def test_pool_against_f64(lib, c):
	l, _lib = lib
	p = c.p
	x = R.pool_ops(c)["x"].to(DEV).contiguous()
	out = nan_buffer(p.nb * p.C, "f32")
	ok(lib, l.ttk_cond_pool_rows(x.data_ptr(), p.nb, p.T, p.C, p.mode, out.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, p.nb * p.C).view(p.nb, p.C)))
	if p.mode == 0:
		same_bytes(out[:p.nb * p.C], x[:, 0].cpu().reshape(-1), c.id)


def test_pool_preconditions_are_refused(lib):
	l, _lib = lib
	x, out = torch.ones(2 * 2 * 128 + 4, device=DEV), nan_buffer(2 * 128, "f32")
	call = lambda x=x.data_ptr(), nb=2, T=2, C=128, mode=1, out=out.data_ptr(): l.ttk_cond_pool_rows(x, nb, T, C, mode, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"x": None}, "null"), ({"out": None}, "null"), ({"mode": 2}, "bad mode"), ({"mode": -1}, "bad mode"), ({"nb": 0}, "out of range"), ({"nb": 65536}, "out of range"),
							 ({"T": 0}, "out of range"), ({"C": 0}, "out of range"), ({"x": x.data_ptr() + 2}, "misaligned")], [out])


# ----------------------------------------------------------------------------------------------------------- k_embed_rows (exact)
@pytest.mark.parametrize("c", R.EMBED_CASES, ids=IDS(R.EMBED_CASES))
def test_embed_rows_gives_the_bytes_owed(lib, c):
	l, _lib = lib
	p, o = c.p, R.embed_ops(c)
	emb, ids = o["emb"].to(DEV).contiguous(), o["ids"].to(DEV).contiguous()
	n = p.B * p.S * p.d
	out = nan_buffer(n, "f32")
	ok(lib, l.ttk_clvp_embed_rows(emb.data_ptr(), p.vocab, p.d, ids.data_ptr(), p.B, p.S, p.stride, out.data_ptr(), _lib.stream_ptr()), c)
	y, tol = R.embed_ref(c)
	record(c, R.check(c, read_back(out, n).view(p.B * p.S, p.d), ref=(y, tol)))
	same_bytes(out[:n], y.float().reshape(-1), c.id)


def test_embed_rows_preconditions_are_refused(lib):
	l, _lib = lib
	emb, ids, out = torch.ones(11 * 64 + 4, device=DEV), torch.zeros(2 * 9 + 2, dtype=torch.int64, device=DEV), nan_buffer(2 * 5 * 64, "f32")
	call = lambda emb=emb.data_ptr(), vocab=11, d=64, ids=ids.data_ptr(), B=2, S=5, stride=9, out=out.data_ptr(): \
		l.ttk_clvp_embed_rows(emb, vocab, d, ids, B, S, stride, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"emb": None}, "null"), ({"ids": None}, "null"), ({"out": None}, "null"), ({"vocab": 0}, "out of range"), ({"B": 0}, "out of range"), ({"S": 0}, "out of range"),
							 ({"d": 60}, "multiple of 64"), ({"d": 0}, "multiple of 64"), ({"stride": 4}, "batch_stride_ids"), ({"emb": emb.data_ptr() + 4}, "16-byte aligned"),
							 ({"out": out.data_ptr() + 8}, "16-byte aligned"), ({"ids": ids.data_ptr() + 4}, "8-byte aligned")], [out])


# ----------------------------------------------------------------------------------------------------------- k_rmsnorm
@pytest.mark.parametrize("c", R.RMS_CASES, ids=IDS(R.RMS_CASES))
def test_rmsnorm_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.rms_ops(c)
	x, g = o["x"].to(DEV).contiguous(), o["g"].to(DEV).contiguous()
	n = p.rows * p.d
	y = nan_buffer(n, c.dt)
	ok(lib, l.ttk_clvp_rmsnorm_rows(R.DT_CODE[c.dt], x.data_ptr(), p.rows, p.d, g.data_ptr(), y.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(y, n).view(p.rows, p.d)))


def test_rmsnorm_preconditions_are_refused(lib):
	l, _lib = lib
	x, g, y = torch.ones(5 * 64 + 4, device=DEV), torch.ones(64 + 4, device=DEV), nan_buffer(5 * 64, "f32")
	call = lambda dt=0, x=x.data_ptr(), rows=5, d=64, g=g.data_ptr(), y=y.data_ptr(): l.ttk_clvp_rmsnorm_rows(dt, x, rows, d, g, y, _lib.stream_ptr())
	refusals(lib, call, {}, [({"dt": 4}, "dtype"), ({"x": None}, "null"), ({"g": None}, "null"), ({"y": None}, "null"), ({"rows": 0}, "out of range"), ({"d": 62}, "multiple of 64"),
							 ({"d": 0}, "multiple of 64"), ({"x": x.data_ptr() + 4}, "16-byte aligned"), ({"g": g.data_ptr() + 8}, "16-byte aligned"),
							 ({"y": y.data_ptr() + 1, "dt": 1}, "16-byte aligned")], [y])


# ----------------------------------------------------------------------------------------------------------- k_rotary (in place)
@pytest.mark.parametrize("c", R.ROT_CASES, ids=IDS(R.ROT_CASES))
def test_rotary_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.rot_ops(c)
	rows, w = p.B * p.S, 3 * p.H * 64
	qkv = filled(o["qkv"], c.dt)
	before = qkv[:rows * w].clone()
	inv = o["inv_freq"].to(DEV).contiguous()
	ok(lib, l.ttk_clvp_rotary_rows(R.DT_CODE[c.dt], qkv.data_ptr(), p.B, p.S, p.H, inv.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(qkv, rows * w).view(rows, w)))
	ity = torch.int16 if c.dt == "bf16" else torch.int32      # features 32..63 of every head of q, k and v keep their bytes
	assert torch.equal(qkv[:rows * w].view(ity).view(rows, 3 * p.H, 64)[..., 32:], before.view(ity).view(rows, 3 * p.H, 64)[..., 32:]), f"{c.id}: features 32..63 were touched"


def test_rotary_preconditions_are_refused(lib):
	l, _lib = lib
	qkv = nan_buffer(2 * 5 * 192, "f32")
	inv = R.INV_FREQ.to(DEV)
	call = lambda dt=0, qkv=qkv.data_ptr(), B=2, S=5, H=1, inv=inv.data_ptr(): l.ttk_clvp_rotary_rows(dt, qkv, B, S, H, inv, _lib.stream_ptr())
	for kw, match in [({"dt": 4}, "dtype"), ({"qkv": None}, "null"), ({"inv": None}, "null"), ({"B": 0}, "out of range"), ({"S": 0}, "out of range"), ({"H": 0}, "out of range"),
					  ({"H": 1025}, "out of range"), ({"qkv": qkv.data_ptr() + 2}, "misaligned"), ({"qkv": qkv.data_ptr() + 1, "dt": 1}, "misaligned")]:
		assert call(**kw) == -1 and match in l.ttk_last_error().decode(), (kw, l.ttk_last_error().decode())
	torch.cuda.synchronize()
	assert bool(torch.isnan(qkv).all()), "a refused call launched something"
	qkv[:2 * 5 * 192] = 1.0      # the base call itself is fine: it rotates the buffer and leaves the tail alone
	assert call() == 0, l.ttk_last_error().decode()
	torch.cuda.synchronize()
	assert bool(torch.isfinite(qkv[:-TAIL]).all()) and bool((qkv[:-TAIL] != 1.0).any()) and bool(torch.isnan(qkv[-TAIL:]).all())


# ----------------------------------------------------------------------------------------------------------- k_geglu
@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=IDS(R.GEGLU_CASES))
def test_geglu_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.geglu_ops(c)
	h = filled(o["h"], c.dt)
	n = p.rows * p.inner
	out = nan_buffer(n, c.dt)
	ok(lib, l.ttk_clvp_geglu_rows(R.DT_CODE[c.dt], h.data_ptr(), p.rows, p.inner, out.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, n).view(p.rows, p.inner)))


def test_geglu_preconditions_are_refused(lib):
	l, _lib = lib
	h, out = torch.ones(3 * 128 + 4, device=DEV), nan_buffer(3 * 64, "f32")
	call = lambda dt=0, h=h.data_ptr(), rows=3, inner=64, out=out.data_ptr(): l.ttk_clvp_geglu_rows(dt, h, rows, inner, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"dt": 4}, "dtype"), ({"h": None}, "null"), ({"out": None}, "null"), ({"rows": 0}, "out of range"), ({"inner": 0}, "out of range"),
							 ({"h": h.data_ptr() + 2}, "misaligned"), ({"out": out.data_ptr() + 1, "dt": 1}, "misaligned"), ({"out": h.data_ptr() + 256}, "overlap")], [out])


# ----------------------------------------------------------------------------------------------------------- k_mean_rows
@pytest.mark.parametrize("c", R.MEAN_CASES, ids=IDS(R.MEAN_CASES))
def test_mean_rows_against_f64(lib, c):
	l, _lib = lib
	p = c.p
	x = R.mean_ops(c)["x"].to(DEV).contiguous()
	out = nan_buffer(p.B * p.d, c.dt)
	ok(lib, l.ttk_clvp_mean_rows(R.DT_CODE[c.dt], x.data_ptr(), p.B, p.S, p.d, out.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, p.B * p.d).view(p.B, p.d)))


def test_mean_rows_preconditions_are_refused(lib):
	l, _lib = lib
	x, out = torch.ones(2 * 7 * 64 + 4, device=DEV), nan_buffer(2 * 64, "f32")
	call = lambda dt=0, x=x.data_ptr(), B=2, S=7, d=64, out=out.data_ptr(): l.ttk_clvp_mean_rows(dt, x, B, S, d, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"dt": 4}, "dtype"), ({"x": None}, "null"), ({"out": None}, "null"), ({"B": 0}, "out of range"), ({"S": 0}, "out of range"), ({"d": 60}, "out of range"),
							 ({"x": x.data_ptr() + 2}, "misaligned"), ({"out": out.data_ptr() + 1, "dt": 1}, "misaligned")], [out])


# ----------------------------------------------------------------------------------------------------------- k_clvp_score
@pytest.mark.parametrize("c", R.SCORE_CASES, ids=IDS(R.SCORE_CASES))
def test_latent_score_against_f64(lib, c):
	l, _lib = lib
	p, o = c.p, R.score_ops(c)
	text = o["text"].clone()
	text[p.Bt:] = float("nan")      # the rows a Bt = 1 launch must not read
	text, speech, temp = text.to(DEV).contiguous(), o["speech"].to(DEV).contiguous(), o["temperature"].to(DEV)
	out = nan_buffer(p.B, "f32")
	ok(lib, l.ttk_clvp_latent_score(text.data_ptr(), p.Bt, speech.data_ptr(), p.B, p.d, temp.data_ptr(), out.data_ptr(), _lib.stream_ptr()), c)
	record(c, R.check(c, read_back(out, p.B)))


def test_latent_score_preconditions_are_refused(lib):
	l, _lib = lib
	t, s, temp, out = torch.ones(3 * 64 + 4, device=DEV), torch.ones(3 * 64 + 4, device=DEV), torch.zeros(2, device=DEV), nan_buffer(3, "f32")
	call = lambda t=t.data_ptr(), Bt=3, s=s.data_ptr(), B=3, d=64, temp=temp.data_ptr(), out=out.data_ptr(): l.ttk_clvp_latent_score(t, Bt, s, B, d, temp, out, _lib.stream_ptr())
	refusals(lib, call, {}, [({"t": None}, "null"), ({"s": None}, "null"), ({"temp": None}, "null"), ({"out": None}, "null"), ({"Bt": 2}, "bad shape"), ({"Bt": 0}, "bad shape"),
							 ({"B": 0, "Bt": 1}, "bad shape"), ({"d": 60}, "multiple of 64"), ({"d": 0}, "multiple of 64"), ({"t": t.data_ptr() + 2}, "misaligned"),
							 ({"temp": temp.data_ptr() + 2}, "misaligned")], [out])


def test_zz_report(lib):
	"""(runs last in this module) the worst err / bound per case group, for the record"""
	for k in sorted(RATIOS):
		print(f"worst err / bound, {k}: {RATIOS[k]:.3f}")
	assert all(v <= 1 for v in RATIOS.values())
