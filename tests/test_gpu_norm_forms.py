"""The normalisation kernels of csrc/norm.hip on caller-provided operands -- k_layernorm (both instantiations) through `ttk_layernorm_rows`, k_gn_stats and the
generic k_gn_apply through `ttk_gn_apply` with stats = 1 and form = 1 -- against the float64 references and the derived per-element bounds of tests/norm_ref.py
(where the bounds are written out and tests/test_norm_ref.py shows on the CPU that they and the canaries see a subtle fault).  tests/test_gpu_gn_forms.py
ties the other GroupNorm-apply forms to the generic form's bytes, so holding the generic form to float64 here holds all of them; at C = 1024 form 0 (the
launcher's own choice) is run as well and owes form 1's bytes.

Every output and statistics buffer starts as NaN (0x7F bytes for fp8) with canary elements behind it, the columns behind d of a strided input row as well:
what a launch owes must be finite and inside the bound, everything else must still be NaN -- rows >= `rows` of a fragment-order tile, the columns behind d of
a strided output row, ring slots 0, 1 and 3, the triples of chunks past a ragged sequence's end.  Every buffer is sized from the descriptor before the launch.
One process, no environment knobs."""
import collections
import ctypes as C

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = collections.defaultdict(float)      # case group and output class -> worst err / bound seen (printed by the last test)
TAIL = 256                                   # canary elements behind a flat buffer


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def nan_buffer(n, elem):
	"""n + TAIL elements of NaN (fp8: 0x7F bytes, e4m3's NaN)"""
	if elem == "f8":
		return torch.full((n + TAIL,), 0x7F, dtype=torch.uint8, device=DEV)
	return torch.full((n + TAIL,), float("nan"), dtype=R.TDT[elem], device=DEV)


def read_back(buf, n):
	"""the first n elements as f64 on the host; the canary tail must still be NaN"""
	t = buf.cpu()
	t = (t.view(torch.float8_e4m3fn) if t.dtype == torch.uint8 else t).float().double()
	assert torch.isnan(t[n:]).all(), "the canary elements behind a buffer were written"
	return t[:n]


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def ln_launch(lib, c, o):
	"""one ttk_layernorm_rows call; returns the images of norm_ref.ln_blank's layout as read back"""
	l, _lib = lib
	dt, out_f32, _, elem, _ = R.OUT_KINDS[c.out]
	x = torch.full((c.rows, c.ldx), float("nan"), device=DEV)      # exactly rows * ldx floats: the last row ends where the kernel's reads end
	x[:, :c.d] = o["x"].to(DEV)
	dev = {k: o[k].to(DEV) for k in ("g1", "b1", "g2", "b2") if k in o}
	n_out = c.pad_rows * c.d if c.frag else (c.rows + R.CANARY_ROWS) * c.ldo
	out = nan_buffer(n_out, elem)
	d = _lib.LnDesc()
	d.x, d.ldx, d.rows, d.d = x.data_ptr(), c.ldx, c.rows, c.d
	d.g1, d.b1 = dev["g1"].data_ptr(), dev["b1"].data_ptr()
	if c.norms == 2:
		d.g2, d.b2 = dev["g2"].data_ptr(), dev["b2"].data_ptr()
	d.out, d.ldo, d.out_f32, d.frag = out.data_ptr(), c.ldo, out_f32, c.frag
	stride = (c.rows + R.CANARY_ROWS) * c.d      # floats per ring slot; % 4 == 0 with d
	if c.out2 == "direct":
		out2 = nan_buffer(stride, "f32")
		d.out2 = out2.data_ptr()
	elif c.out2 == "ring":      # as the decode step passes it: no out2, the base and the slot index in device memory
		out2 = nan_buffer(R.RING_SLOTS * stride, "f32")
		base = torch.tensor([out2.data_ptr()], dtype=torch.int64, device=DEV)
		slot = torch.tensor([R.RING_SLOT], dtype=torch.int64, device=DEV)
		d.out2_base, d.out2_idx, d.out2_stride = base.data_ptr(), slot.data_ptr(), stride
	rc = l.ttk_layernorm_rows(dt, C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id}: ttk_layernorm_rows refused the case: {l.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	flat = read_back(out, n_out)
	img = {"out": R.from_frag(flat, c.pad_rows, c.d) if c.frag else flat.view(c.rows + R.CANARY_ROWS, c.ldo)}
	if c.out2 == "direct":
		img["out2"] = read_back(out2, stride).view(c.rows + R.CANARY_ROWS, c.d)
	elif c.out2 == "ring":
		img["out2"] = read_back(out2, R.RING_SLOTS * stride).view(R.RING_SLOTS, c.rows + R.CANARY_ROWS, c.d)
	return img


@pytest.mark.parametrize("case", R.LN_CASES, ids=[c.id for c in R.LN_CASES])
def test_layernorm_against_f64(lib, case):
	c = case
	o = R.ln_reference(c)[0]
	w = R.ln_check(c, ln_launch(lib, c, o))
	for k, r in w.items():
		RATIOS[f"{c.group} {k}"] = max(RATIOS[f"{c.group} {k}"], r)
		print(f"{c.id}: err / bound {k} {r:.3f}")
	for k, r in w.items():
		assert r <= 1, f"{c.id}: |got - ref| is {r:.3g}x the bound ({k})"


# ----------------------------------------------------------------------------------------------------------- GroupNorm
class GnOperands:
	def __init__(self, c, o):
		self.c = c
		self.x, self.gamma, self.beta, self.mod = (o[k].to(DEV).contiguous() for k in ("x", "gamma", "beta", "mod"))
		self.tlen = torch.tensor(c.tlen, dtype=torch.int32, device=DEV) if c.tlen else None
		self.idx = c.row_idx().to(DEV) if c.Tout else None

	def launch(self, lib, variant, form):
		"""one ttk_gn_apply call with stats = 1 into fresh NaN buffers: (out f64 [nb][rows_out][C], ms f64 [nb][32][nchunks][3], the raw output buffer)"""
		l, _lib = lib
		c = self.c
		kind, mod, act = variant
		dt, out_f32, out_f8, elem, _ = R.OUT_KINDS[kind]
		n_out, n_ms = c.nb * c.rows_out * c.C, c.nb * 32 * c.nchunks * 3
		out, ms = nan_buffer(n_out, elem), nan_buffer(n_ms, "f32")
		d = _lib.GnDesc()
		d.x, d.ms, d.gamma, d.beta = self.x.data_ptr(), ms.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr()
		has, per_b = R.GN_MODS[mod]
		if has:
			d.scale, d.shift, d.ss_stride = self.mod.data_ptr(), self.mod.data_ptr() + 4 * c.C, 2 * c.C if per_b else 0
		d.tlen = self.tlen.data_ptr() if self.tlen is not None else None
		d.row_idx = self.idx.data_ptr() if self.idx is not None else None
		d.nb, d.T, d.Tout, d.C, d.act = c.nb, c.T, c.rows_out, c.C, act
		d.out, d.out_f32, d.out_f8 = out.data_ptr(), out_f32, out_f8
		d.stats, d.form = 1, form
		rc = l.ttk_gn_apply(dt, C.byref(d), _lib.stream_ptr())
		assert rc == 0, f"{c.id} {variant} form {form}: ttk_gn_apply refused the case: {l.ttk_last_error().decode()}"
		torch.cuda.synchronize()
		return read_back(out, n_out).view(c.nb, c.rows_out, c.C), read_back(ms, n_ms).view(c.nb, 32, c.nchunks, 3), out


@pytest.mark.parametrize("case", R.GN_CASES, ids=[c.id for c in R.GN_CASES])
def test_groupnorm_against_f64(lib, case):
	c = case
	ops = GnOperands(c, R.gn_statistics(c)[0])
	for variant in c.variants:
		out, ms, raw = ops.launch(lib, variant, 1)
		w = R.gn_check(c, variant, out, ms)
		for k, r in w.items():
			RATIOS[f"{c.group} {k}"] = max(RATIOS[f"{c.group} {k}"], r)
		print(f"{c.id} ({c.what}) {variant}: err / bound " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(w.items())))
		for k, r in w.items():
			assert r <= 1, f"{c.id} {variant}: |got - ref| is {r:.3g}x the bound ({k})"
		if c.C == 1024:      # the launcher's own choice owes the generic form's bytes (and the same statistics)
			out0, ms0, raw0 = ops.launch(lib, variant, 0)
			assert torch.equal(raw0.view(torch.uint8), raw.view(torch.uint8)), f"{c.id} {variant}: form 0 does not give form 1's bytes"
			assert torch.equal(ms0.nan_to_num(nan=-1.0), ms.nan_to_num(nan=-1.0)), f"{c.id} {variant}: form 0 left other statistics than form 1"


# ----------------------------------------------------------------------------------------------------------- refusals
def test_layernorm_preconditions_are_refused(lib):
	"""what k_layernorm takes for granted comes back as TTK_E_ARG with a message, before anything is launched: `out` and `out2` keep their NaN"""
	l, _lib = lib
	rows, dd = 5, 64
	x = torch.zeros(rows * (dd + 8) + 8, device=DEV)
	v = torch.ones(dd + 8, device=DEV)
	out = torch.full((16 * (dd + 8),), float("nan"), device=DEV)
	out2 = torch.full((4 * (rows * dd + 8),), float("nan"), device=DEV)
	i64 = torch.tensor([0, out2.data_ptr()], dtype=torch.int64, device=DEV)

	def desc(**kw):
		d = _lib.LnDesc()
		d.x, d.ldx, d.rows, d.d, d.g1, d.b1, d.out, d.ldo = x.data_ptr(), dd, rows, dd, v.data_ptr(), v.data_ptr(), out.data_ptr(), dd
		for k, val in kw.items():
			setattr(d, k, val)
		return d

	def refused(d, match, dt=1):
		assert l.ttk_layernorm_rows(dt, C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	assert l.ttk_layernorm_rows(1, None, _lib.stream_ptr()) == -1 and "null descriptor" in l.ttk_last_error().decode()
	for name in ("x", "g1", "b1", "out"):
		refused(desc(**{name: None}), "null")
	refused(desc(), "dtype", dt=3)
	refused(desc(), "dtype", dt=2)
	refused(desc(g2=v.data_ptr()), "come together")
	refused(desc(b2=v.data_ptr()), "come together")
	refused(desc(rows=0), "rows >= 1")
	refused(desc(rows=-3), "rows >= 1")
	refused(desc(d=62, ldx=64), "multiple of 4")
	refused(desc(d=0), "multiple of 4")
	refused(desc(d=4100, ldx=4100, ldo=4100), "4 .. 4096")
	refused(desc(d=48, frag=1), "d % 32 == 0")
	refused(desc(ldx=dd - 4), "ldx must be")
	refused(desc(ldx=dd + 2), "ldx must be")
	refused(desc(ldo=dd - 1), "ldo < d")
	for name in ("x", "g1", "b1"):
		refused(desc(**{name: getattr(desc(), name) + 4}), "16-byte aligned")
	refused(desc(g2=v.data_ptr() + 8, b2=v.data_ptr()), "16-byte aligned")
	refused(desc(g2=v.data_ptr(), b2=v.data_ptr() + 4), "16-byte aligned")
	refused(desc(out2=out2.data_ptr() + 4), "16-byte aligned")
	refused(desc(out=out.data_ptr() + 2), "out is misaligned", dt=0)
	refused(desc(out=out.data_ptr() + 2, out_f32=1), "out is misaligned")
	refused(desc(out=out.data_ptr() + 1), "out is misaligned")
	refused(desc(out2=out2.data_ptr(), out2_idx=i64.data_ptr() + 4), "8-byte aligned")
	refused(desc(out2_base=i64.data_ptr() + 12), "8-byte aligned")
	refused(desc(out2_idx=i64.data_ptr()), "out2_idx without")
	refused(desc(out2=out2.data_ptr(), out2_idx=i64.data_ptr(), out2_stride=rows * dd + 2), "out2_stride")
	refused(desc(out2=out2.data_ptr(), out2_idx=i64.data_ptr(), out2_stride=-4), "out2_stride")
	torch.cuda.synchronize()
	assert bool(torch.isnan(out).all()) and bool(torch.isnan(out2).all()), "a refused call launched something"
	# the base descriptor itself is fine, with and without the ring
	assert l.ttk_layernorm_rows(1, C.byref(desc(out_f32=1)), _lib.stream_ptr()) == 0
	assert l.ttk_layernorm_rows(1, C.byref(desc(out_f32=1, out2_base=i64.data_ptr() + 8, out2_idx=i64.data_ptr(), out2_stride=rows * dd + 8)), _lib.stream_ptr()) == 0
	torch.cuda.synchronize()
	assert bool(torch.isfinite(out[:rows * dd]).all()) and bool(torch.isnan(out[rows * dd:]).all())
	assert bool(torch.isfinite(out2[:rows * dd]).all()) and bool(torch.isnan(out2[rows * dd:]).all())


def test_zz_report(lib):
	"""(runs last in this module) the worst err / bound per case group and output class, for the record"""
	for k in sorted(RATIOS):
		print(f"worst err / bound, {k}: {RATIOS[k]:.3f}")
	assert all(v <= 1 for v in RATIOS.values())
