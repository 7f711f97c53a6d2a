"""The vocoders' own kernels on caller-provided operands -- k_lvc<T, 16 / 32> and k_lvc_mfma (csrc/univnet.hip) through `ttk_lvc_rows`, k_hifi_pack_frag and
k_hifi_conv_mfma<32 / 64> (csrc/hifigan.hip) through `ttk_hifi_conv_rows`, k_snake_aa<float / bf16> (csrc/voc.hip) through `ttk_snake_rows` -- against the float64
references and the derived per-element bounds of tests/voc_ref.py (where the bounds are written out and tests/test_voc_ref.py shows on the CPU that they and the
canaries see a subtle fault).

Every output buffer starts as NaN with canary rows and a canary tail behind it; the inputs sit inside NaN guards -- a row in front of y[0] / x[0] / a[0] and one
behind the last, the columns [C, lda) of the narrow conv's `a`, a frame behind the last of `kern` and `kbias`, rows behind the residual -- so that a read outside
what the definition allows becomes a NaN in an output.  What a launch owes must be finite and inside the bound; everything else must still be NaN: the columns
[CG, lda) of `at`, [C, ldo) of `at_out`, `xout` and `at_out` in the MRF modes, `mrf` in modes 0 and 1, the canaries.  One process, no environment knobs."""
import collections
import ctypes as C

import pytest
import torch

import voc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = collections.defaultdict(float)      # case group and output class -> worst err / bound seen (printed by the last test)
TAIL = 256                                   # canary elements behind a flat buffer
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def nan_buffer(n, dt):
	return torch.full((n + TAIL,), NAN, dtype=R.TDT[dt], device=DEV)


def image(rows, width, dt, top=None):
	"""a NaN buffer of rows x width elements (+ TAIL) whose first rows hold `top` (f32 [r][w], w <= width)"""
	buf = nan_buffer(rows * width, dt)
	if top is not None:
		buf[:rows * width].view(rows, width)[:top.shape[0], :top.shape[1]] = top.to(DEV).to(R.TDT[dt])
	return buf


def read_back(buf, rows, width):
	"""the image as f64 [rows][width] on the host; the canary tail must still be NaN"""
	t = buf.cpu().float().double()
	assert torch.isnan(t[rows * width:]).all(), "the canary elements behind a buffer were written"
	return t[:rows * width].view(rows, width)


def guarded(rows, dt, width=None):
	"""(buffer, pointer to its row 1): `rows` [r][w] f32 between one NaN row in front and one behind, columns [w, width) NaN as well"""
	r, w = rows.shape
	width = width or w
	buf = torch.full((r + 2, width), NAN, dtype=R.TDT[dt], device=DEV)
	buf[1:r + 1, :w] = rows.to(DEV).to(R.TDT[dt])
	return buf, buf.data_ptr() + width * buf.element_size()


def record(c, w):
	for k, r in w.items():
		RATIOS[f"{c.group} {k}"] = max(RATIOS[f"{c.group} {k}"], r)
	print(f"{c.id}: err / bound " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(w.items())))
	for k, r in w.items():
		assert r <= 1, f"{c.id}: |got - ref| is {r:.3g}x the bound ({k})"


# ----------------------------------------------------------------------------------------------------------- LVC
def lvc_launch(lib, c, o):
	l, _lib = lib
	rows = R.B * c.L
	ybuf, yp = guarded(o["y"], "f32")
	kern = torch.cat([o["kern"], torch.full((1, c.kstride), NAN)]).to(DEV).to(R.TDT[c.dt])
	kbias = torch.cat([o["kbias"], torch.full((1, c.bstride), NAN)]).to(DEV)
	x = image(rows + R.LVC_CANARY_ROWS, c.CG, "f32", o["x"])
	at = image(rows + R.LVC_CANARY_ROWS, R.LVC_LDA, c.dt)
	d = _lib.LvcDesc()
	d.y, d.kern, d.kbias, d.x, d.at = yp, kern.data_ptr(), kbias.data_ptr(), x.data_ptr(), at.data_ptr()
	d.B, d.L, d.CG, d.hop, d.Tc, d.layer, d.n_layers, d.lda = R.B, c.L, c.CG, c.hop, c.Tc, c.layer, c.n_layers, R.LVC_LDA
	rc = l.ttk_lvc_rows(_lib.DTYPES[c.dt], C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id}: ttk_lvc_rows refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	return {"x": read_back(x, rows + R.LVC_CANARY_ROWS, c.CG), "at": read_back(at, rows + R.LVC_CANARY_ROWS, R.LVC_LDA)}


@pytest.mark.parametrize("case", R.LVC_CASES, ids=[c.id for c in R.LVC_CASES])
def test_lvc_against_f64(lib, case):
	c = case
	record(c, R.lvc_check(c, lvc_launch(lib, c, R.lvc_operands(c))))


# ----------------------------------------------------------------------------------------------------------- narrow conv
def hifi_launch(lib, c, o):
	l, _lib = lib
	rows = c.L + R.HIFI_CANARY_ROWS
	abuf, ap = guarded(o["a"], "bf16", c.ld)
	w, bias = o["w"].to(DEV).contiguous(), o["bias"].to(DEV)
	at_out = image(rows, c.ld, "bf16")
	xout = image(rows, c.C, "f32", o["xres"] if c.mode == 1 else None)      # mode 1: the residual, updated in place as the model does
	mrf = image(rows, c.C, "f32", o["mrf0"] if c.mode == 3 else None)
	xres = image(rows, c.C, "f32", o["xres"]) if c.mode >= 2 else None
	d = _lib.HifiConvDesc()
	d.a, d.lda, d.w, d.bias = ap, c.ld, w.data_ptr(), bias.data_ptr()
	d.L, d.C, d.k, d.dil, d.mode = c.L, c.C, c.k, c.dil, c.mode
	d.xres = None if c.mode == 0 else (xout.data_ptr() if c.mode == 1 else xres.data_ptr())
	d.xout, d.at_out, d.ldo, d.mrf = xout.data_ptr(), at_out.data_ptr(), c.ld, mrf.data_ptr()
	rc = l.ttk_hifi_conv_rows(C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id}: ttk_hifi_conv_rows refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	if xres is not None:
		assert torch.equal(read_back(xres, rows, c.C)[:c.L], o["xres"].double()), f"{c.id}: the residual was written in a mode that only reads it"
	return {"at_out": read_back(at_out, rows, c.ld), "xout": read_back(xout, rows, c.C), "mrf": read_back(mrf, rows, c.C)}


@pytest.mark.parametrize("case", R.HIFI_CASES, ids=[c.id for c in R.HIFI_CASES])
def test_narrow_conv_against_f64(lib, case):
	c = case
	record(c, R.hifi_check(c, hifi_launch(lib, c, R.hifi_operands(c))))


# ----------------------------------------------------------------------------------------------------------- snake
def snake_launch(lib, c, o):
	l, _lib = lib
	rows = R.B * c.L
	xbuf, xp = guarded(o["x"], "f32")
	a, invb, filt = o["a"].to(DEV), o["invb"].to(DEV), o["filt"].to(DEV)
	y = image(rows + R.SNAKE_CANARY_ROWS, c.C, c.dt)
	rc = l.ttk_snake_rows(_lib.DTYPES[c.dt], xp, R.B, c.L, c.C, a.data_ptr(), invb.data_ptr(), filt.data_ptr(), y.data_ptr(), _lib.stream_ptr())
	assert rc == 0, f"{c.id}: ttk_snake_rows refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	return {"y": read_back(y, rows + R.SNAKE_CANARY_ROWS, c.C)}


@pytest.mark.parametrize("case", R.SNAKE_CASES, ids=[c.id for c in R.SNAKE_CASES])
def test_snake_against_f64(lib, case):
	c = case
	record(c, R.snake_check(c, snake_launch(lib, c, R.snake_operands(c))))


# ----------------------------------------------------------------------------------------------------------- refusals
def test_lvc_preconditions_are_refused(lib):
	"""what k_lvc / k_lvc_mfma take for granted comes back as TTK_E_ARG with a message, before anything is launched: x keeps its values, at its NaN"""
	l, _lib = lib
	Bn, L, CG, hop, Tc, nl, lda = 2, 24, 16, 8, 3, 2, 64
	y = torch.zeros(Bn * L * CG + 8, device=DEV)
	kern = torch.zeros(Bn * Tc * nl * CG * 2 * CG * 3 + 8, device=DEV)
	kbias = torch.zeros(Bn * Tc * nl * 2 * CG + 8, device=DEV)
	x = torch.ones(Bn * L * CG + 8, device=DEV)
	at = torch.full((Bn * L * lda + 8,), NAN, device=DEV)

	def desc(**kw):
		d = _lib.LvcDesc()
		d.y, d.kern, d.kbias, d.x, d.at = y.data_ptr(), kern.data_ptr(), kbias.data_ptr(), x.data_ptr(), at.data_ptr()
		d.B, d.L, d.CG, d.hop, d.Tc, d.layer, d.n_layers, d.lda = Bn, L, CG, hop, Tc, 1, nl, lda
		for k, v in kw.items():
			setattr(d, k, v)
		return d

	def refused(d, match, dt=0):
		assert l.ttk_lvc_rows(dt, C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	assert l.ttk_lvc_rows(0, None, _lib.stream_ptr()) == -1 and "null descriptor" in l.ttk_last_error().decode()
	for name in ("y", "kern", "kbias", "x", "at"):
		refused(desc(**{name: None}), "null argument")
	for dt in (2, 3, 4, -1):
		refused(desc(), "bad dtype", dt=dt)
	for cg in (0, 8, 24, 64):
		refused(desc(CG=cg), "no instantiation")
	refused(desc(B=0), "out of range")
	refused(desc(B=65536), "out of range")
	refused(desc(L=0), "out of range")
	refused(desc(hop=0), "hop = 0")
	refused(desc(hop=-8), "hop = -8")
	refused(desc(Tc=2), "need 3 frames")
	refused(desc(hop=7), "need 4 frames")
	refused(desc(Tc=0), "frames")
	refused(desc(layer=2), "layer 2 of n_layers 2")
	refused(desc(layer=-1), "out of range")
	refused(desc(n_layers=5, layer=0), "n_layers 5")
	refused(desc(n_layers=0, layer=0), "n_layers 0")
	refused(desc(lda=CG - 1), "lda < CG")
	for name in ("y", "kbias", "x", "kern", "at"):
		refused(desc(**{name: getattr(desc(), name) + 2}), "misaligned")
	refused(desc(kern=kern.data_ptr() + 1), "misaligned", dt=1)
	refused(desc(at=at.data_ptr() + 1), "misaligned", dt=1)
	refused(desc(y=x.data_ptr()), "x overlaps an input")
	refused(desc(y=x.data_ptr() + 4 * CG), "x overlaps an input")
	refused(desc(kbias=x.data_ptr()), "x overlaps an input")
	refused(desc(at=x.data_ptr()), "at overlaps")
	refused(desc(at=y.data_ptr()), "at overlaps")
	refused(desc(at=kern.data_ptr()), "at overlaps")
	torch.cuda.synchronize()
	assert bool((x == 1).all()) and bool(torch.isnan(at).all()), "a refused call launched something"
	for dt in (0, 1):      # the base descriptor itself is fine, in both types (the f32 buffers are large enough for either)
		assert l.ttk_lvc_rows(dt, C.byref(desc()), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()
	torch.cuda.synchronize()
	assert bool(torch.isfinite(x[:Bn * L * CG]).all()) and bool((x[Bn * L * CG:] == 1).all())


def test_narrow_conv_preconditions_are_refused(lib):
	"""what k_hifi_conv_mfma takes for granted comes back as TTK_E_ARG with a message, before anything is packed or launched: the outputs keep their NaN"""
	l, _lib = lib
	L, Cn, k, ld = 20, 32, 3, 64
	a = torch.zeros(L * ld + 16, dtype=torch.bfloat16, device=DEV)
	w = torch.zeros(Cn * Cn * 11 + 4, device=DEV)
	bias = torch.zeros(Cn + 4, device=DEV)
	xres = torch.zeros(L * Cn + 64, device=DEV)
	xout = torch.full((L * Cn + 64,), NAN, device=DEV)
	mrf = torch.full((L * Cn + 64,), NAN, device=DEV)
	at_out = torch.full((L * ld + 16,), NAN, dtype=torch.bfloat16, device=DEV)

	def desc(**kw):
		d = _lib.HifiConvDesc()
		d.a, d.lda, d.w, d.bias, d.L, d.C, d.k, d.dil, d.mode = a.data_ptr(), ld, w.data_ptr(), bias.data_ptr(), L, Cn, k, 1, 1
		d.xres, d.xout, d.at_out, d.ldo, d.mrf = xres.data_ptr(), xout.data_ptr(), at_out.data_ptr(), ld, mrf.data_ptr()
		for key, v in kw.items():
			setattr(d, key, v)
		return d

	def refused(d, match):
		assert l.ttk_hifi_conv_rows(C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	assert l.ttk_hifi_conv_rows(None, _lib.stream_ptr()) == -1 and "null descriptor" in l.ttk_last_error().decode()
	for name in ("a", "w", "bias"):
		refused(desc(**{name: None}), "null argument")
	for cn in (0, 16, 48, 128):
		refused(desc(C=cn), "no instantiation")
	for kk in (0, 2, 4, 13, -3):
		refused(desc(k=kk), "kernel size")
	refused(desc(dil=0), "dilation")
	refused(desc(dil=5000), "dilation")
	refused(desc(C=64, lda=64, ldo=64, k=11, dil=40), "bytes of LDS")           # 88 KiB of weights + a 656-row window of 144 bytes a row
	refused(desc(L=0), "L = 0")
	refused(desc(lda=Cn - 8), "lda must be")
	refused(desc(lda=Cn + 4), "lda must be")
	refused(desc(a=a.data_ptr() + 8), "16-byte aligned")
	refused(desc(a=a.data_ptr() + 2), "16-byte aligned")
	refused(desc(mode=4), "mode 4")
	refused(desc(mode=-1), "mode -1")
	for mode in (1, 2, 3):
		refused(desc(mode=mode, xres=None), "needs xres")
	refused(desc(mode=1, xout=None), "needs xout")
	for mode in (0, 1):
		refused(desc(mode=mode, at_out=None), "needs at_out")
	for mode in (2, 3):
		refused(desc(mode=mode, mrf=None), "needs mrf")
	refused(desc(ldo=Cn - 1), "ldo < C")
	for name in ("w", "bias", "xres", "xout"):
		refused(desc(**{name: getattr(desc(), name) + 2}), "misaligned")
	refused(desc(mode=3, mrf=mrf.data_ptr() + 2), "misaligned")
	refused(desc(at_out=at_out.data_ptr() + 1), "misaligned")
	refused(desc(at_out=a.data_ptr()), "at_out overlaps a")
	refused(desc(at_out=a.data_ptr() + 2 * ld), "at_out overlaps a")
	refused(desc(mode=0, at_out=a.data_ptr()), "at_out overlaps a")
	refused(desc(xout=a.data_ptr()), "xout overlaps a")
	refused(desc(mode=2, mrf=a.data_ptr()), "mrf overlaps a")
	refused(desc(xout=xres.data_ptr() + 4 * Cn), "xout overlaps xres")
	refused(desc(mode=3, mrf=xres.data_ptr()), "mrf overlaps xres")
	refused(desc(at_out=xres.data_ptr()), "at_out overlaps xres or xout")
	torch.cuda.synchronize()
	assert bool(torch.isnan(xout).all()) and bool(torch.isnan(mrf).all()) and bool(torch.isnan(at_out).all()) and not bool(xres.any()), "a refused call launched something"
	# the base descriptor itself is fine; so are the modes that need fewer buffers, without them, and the in-place residual
	assert l.ttk_hifi_conv_rows(C.byref(desc()), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()
	assert l.ttk_hifi_conv_rows(C.byref(desc(mode=0, xres=None, xout=None, mrf=None)), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()
	assert l.ttk_hifi_conv_rows(C.byref(desc(mode=2, xout=None, at_out=None, ldo=0)), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()
	assert l.ttk_hifi_conv_rows(C.byref(desc(mode=1, xres=xout.data_ptr())), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()
	torch.cuda.synchronize()
	assert bool(torch.isfinite(xout[:L * Cn]).all()) and bool(torch.isnan(xout[L * Cn:]).all()) and bool(torch.isfinite(mrf[:L * Cn]).all())


def test_snake_preconditions_are_refused(lib):
	"""what k_snake_aa takes for granted comes back as TTK_E_ARG with a message, before anything is launched: y keeps its NaN"""
	l, _lib = lib
	Bn, L, Cn = 2, 5, 8
	x = torch.zeros(Bn * L * Cn + 8, device=DEV)
	v = torch.ones(Cn + 16, device=DEV)
	y = torch.full((2 * Bn * L * Cn + 8,), NAN, device=DEV)      # room for the f32 result and, behind it, the bf16 one
	base = dict(dtype=0, x=x.data_ptr(), B=Bn, L=L, C=Cn, a=v.data_ptr(), invb=v.data_ptr(), filt=v.data_ptr(), y=y.data_ptr())

	def call(**kw):
		p = dict(base, **kw)
		return l.ttk_snake_rows(p["dtype"], p["x"], p["B"], p["L"], p["C"], p["a"], p["invb"], p["filt"], p["y"], _lib.stream_ptr())

	def refused(match, **kw):
		assert call(**kw) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	for dt in (2, 3, 4, -1):
		refused("bad dtype", dtype=dt)
	for name in ("x", "a", "invb", "filt", "y"):
		refused("null argument", **{name: None})
	refused("out of range", B=0)
	refused("out of range", L=0)
	refused("out of range", B=1 << 16, L=1 << 16)
	for cn in (0, 2, 6, 9, -4, 8196):
		refused("unsupported", C=cn)
	refused("too many", B=1 << 10, L=1 << 10, C=8192)
	for name in ("x", "a", "invb"):
		refused("16-byte aligned", **{name: base[name] + 4})
		refused("16-byte aligned", **{name: base[name] + 8})
	refused("misaligned", filt=v.data_ptr() + 2)
	refused("misaligned", y=y.data_ptr() + 2)
	refused("misaligned", y=y.data_ptr() + 1, dtype=1)
	refused("x and y overlap", y=x.data_ptr())
	refused("x and y overlap", y=x.data_ptr() + 4 * Cn)
	refused("x and y overlap", y=x.data_ptr() + 16, dtype=1)
	torch.cuda.synchronize()
	assert bool(torch.isnan(y).all()), "a refused call launched something"
	assert call() == 0, l.ttk_last_error().decode()
	assert call(dtype=1, y=y.data_ptr() + 4 * Bn * L * Cn) == 0, l.ttk_last_error().decode()      # bf16: 2 bytes per element, behind the f32 result
	torch.cuda.synchronize()
	assert bool(torch.isfinite(y[:Bn * L * Cn]).all())


def test_zz_report(lib):
	"""(runs last in this module) the worst err / bound per kernel and output class, for the record"""
	for k in sorted(RATIOS):
		print(f"worst err / bound, {k}: {RATIOS[k]:.3f}")
	assert RATIOS and all(v <= 1 for v in RATIOS.values())
