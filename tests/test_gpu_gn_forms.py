"""Every launch form of GroupNorm-apply (csrc/norm.hip) through `ttk_gn_apply`: the generic kernel (form 1), the 4-row strips of k_gn_apply_c1024 (form 2) and the
three instantiations of k_gn_apply_c1024_even (forms 3, 4, 5: up to 9, 12, 18 rows per thread).  norm.hip says of each that it does the generic kernel's arithmetic
in the generic kernel's order: on the same input and the same statistics every form owes the generic form's BYTES.  That is all this file asserts -- exact equality
and finiteness, no tolerance anywhere; how accurate the generic form is, and with it every other, is held to a float64 reference by tests/test_gpu_norm_forms.py.

`out` starts as NaN with canary rows behind it, the statistics buffer as NaN in front of the statistics launch (chunks past a ragged sequence's end stay NaN: a
kernel that uses them fails).  One process, no environment knobs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 1024
CHUNK = 2048 // (CH // 32)      # rows per statistics chunk (gn_rows_per_chunk)
DT = {"f32": 0, "bf16": 1, "f16": 4}
GENERIC, STRIPS, EVEN9, EVEN12, EVEN18 = 1, 2, 3, 4, 5
MAXR = {EVEN9: 9, EVEN12: 12, EVEN18: 18}
CANARY = 8 * CH
# output kinds: (name, dtype code, out_f32, out_f8, torch type)
OUTS = [("f32", 0, 0, 0, torch.float32), ("bf16", 1, 0, 0, torch.bfloat16), ("f16", 4, 0, 0, torch.float16), ("f8", 1, 0, 1, torch.uint8), ("bf16-f32out", 1, 1, 0, torch.float32)]
# modulation: (name, has scale / shift, ss_stride)
MODS = [("plain", False, 0), ("mod-shared", True, 0), ("mod-per-batch", True, 2 * CH)]


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def geometry(nb, T):
	"""(q, rem, nchunks) as the launcher computes them"""
	strips = 256 // nb
	return T // strips, T % strips, (T + CHUNK - 1) // CHUNK


def legal_forms(nb, T, ragged):
	"""gn_apply_form_refusal of csrc/norm.hip at C = 1024, no row_idx, Tout == T"""
	forms = [GENERIC, STRIPS]
	q, rem, nch = geometry(nb, T)
	if not ragged and nb <= 64:
		forms += [f for f in (EVEN9, EVEN12, EVEN18) if q >= 4 and q + (rem != 0) <= MAXR[f] and (f == EVEN18 or nch <= 24)]
	return forms


class Operands:
	"""one input with its statistics (computed once, by the first generic launch) shared by every form and variant of a case"""

	def __init__(self, nb, T, tlen=None):
		g = torch.Generator().manual_seed(1000 * nb + T)
		self.nb, self.T = nb, T
		self.x = (torch.randn(nb, T, CH, generator=g) * 1.5 + 0.25).to(DEV)
		self.gamma = (1 + 0.2 * torch.randn(CH, generator=g)).to(DEV)
		self.beta = (0.2 * torch.randn(CH, generator=g)).to(DEV)
		self.mod = (0.3 * torch.randn(nb, 2 * CH, generator=g)).to(DEV)      # rows of [scale | shift]
		self.tlen = torch.tensor(tlen, dtype=torch.int32, device=DEV) if tlen else None
		self.ms = torch.full((nb * 32 * geometry(nb, T)[2] * 3,), float("nan"), device=DEV)
		self.pf = torch.randn(3 * 8 * 128 * 40 // 4, generator=g).to(DEV)      # 3 taps of 8 slices of 40 lines
		self.have_stats = False

	def run(self, lib, form, out_kind, mod, act, pf):
		l, _lib = lib
		_, dt, out_f32, out_f8, tdt = out_kind
		n = self.nb * self.T * CH
		out = torch.full((n + CANARY,), 0x7F, dtype=torch.uint8, device=DEV) if out_f8 else torch.full((n + CANARY,), float("nan"), dtype=tdt, device=DEV)
		d = _lib.GnDesc()
		d.x, d.ms, d.gamma, d.beta = self.x.data_ptr(), self.ms.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr()
		if mod[1]:
			d.scale, d.shift, d.ss_stride = self.mod.data_ptr(), self.mod.data_ptr() + 4 * CH, mod[2]
		d.tlen = self.tlen.data_ptr() if self.tlen is not None else None
		d.nb, d.T, d.Tout, d.C, d.act = self.nb, self.T, self.T, CH, act
		d.out, d.out_f32, d.out_f8 = out.data_ptr(), out_f32, out_f8
		if pf:
			d.pf, d.pf_bytes, d.pf_taps = self.pf.data_ptr(), 8 * 128 * 40, 3
		d.stats, d.form = int(not self.have_stats), form
		rc = l.ttk_gn_apply(dt, C.byref(d), _lib.stream_ptr())
		assert rc == 0, f"form {form}: ttk_gn_apply refused the case: {l.ttk_last_error().decode()}"
		torch.cuda.synchronize()
		self.have_stats = True
		tail = out[n:]
		assert bool(((tail & 0x7F) == 0x7F).all() if out_f8 else torch.isnan(tail).all()), f"form {form}: rows behind the output were written"
		return out[:n].view(self.nb, self.T, CH)


def finite(t):
	return bool(((t & 0x7F) != 0x7F).all()) if t.dtype == torch.uint8 else bool(torch.isfinite(t).all())


def same_bytes(a, b):
	return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_case(lib, nb, T, expect0, tlen=None):
	"""every legal form and form 0 against the generic form, over the output types, modulation, activation and the weight touch"""
	forms = legal_forms(nb, T, tlen is not None)
	assert expect0 in forms, f"the launcher's form {expect0} is not legal at nb={nb} T={T}: the example tests the wrong form"
	ops = Operands(nb, T, tlen)
	variants = [(o, MODS[1], 2, True) for o in OUTS]                                     # every output type, modulated SiLU with the touch (the DDIM loop's launch)
	variants += [(OUTS[1], m, a, p) for m in MODS for a in (0, 2) for p in (False, True)]      # bf16: modulation x activation x touch
	for out_kind, mod, act, pf in variants:
		what = f"nb={nb} T={T} out={out_kind[0]} {mod[0]} act={act} pf={pf}"
		ref = ops.run(lib, GENERIC, out_kind, mod, act, False)
		assert finite(ref), f"{what}: the generic form gives non-finite output"
		if tlen:
			for b, tl in enumerate(tlen):
				assert not ref[b, tl:].view(torch.uint8).any(), f"{what}: generic form, padding rows of sequence {b} are not zero"
		for form in [0] + forms:
			got = ops.run(lib, form, out_kind, mod, act, pf)
			assert finite(got), f"{what}: form {form} gives non-finite output"
			assert same_bytes(got, ref), f"{what}: form {form} does not give the generic form's bytes ({int((got.view(torch.uint8) != ref.view(torch.uint8)).sum())} bytes differ)"


# (nb, T, q, rem, nchunks, the launcher's form): the even instantiations, each with rem == 0 and rem != 0
EVEN_CASES = [
	(64, 32, 8, 0, 1, EVEN9),
	(8, 150, 4, 22, 3, EVEN9),
	(2, 1088, 8, 64, 17, EVEN9),        # the product's own shape
	(64, 48, 12, 0, 1, EVEN12),
	(64, 37, 9, 1, 1, EVEN12),
	(2, 2304, 18, 0, 36, EVEN18),
	(2, 1600, 12, 64, 25, EVEN18),      # 13 rows would fit no (., 3) form anyway; 25 chunks rule them out as well
]


@pytest.mark.parametrize("nb,T,q,rem,nch,form", EVEN_CASES, ids=[f"nb{c[0]}-T{c[1]}" for c in EVEN_CASES])
def test_even_forms_give_the_generic_bytes(lib, nb, T, q, rem, nch, form):
	assert geometry(nb, T) == (q, rem, nch)
	mr = q + (rem != 0)
	want = EVEN9 if nch <= 24 and mr <= 9 else (EVEN12 if nch <= 24 and mr <= 12 else EVEN18)      # the launcher's conditions restated
	assert q >= 4 and mr <= 18 and want == form
	check_case(lib, nb, T, form)


@pytest.mark.parametrize("T", [64, 65, 67])
def test_strip_form_gives_the_generic_bytes(lib, T):
	"""T % 4 in {0, 1, 3}; three sequences make 85 strips of less than 4 rows, so the launcher itself takes the 4-row strips"""
	assert geometry(3, T)[0] < 4 and T % 4 in (0, 1, 3)
	check_case(lib, 3, T, STRIPS)


def test_ragged_batch_gives_the_generic_bytes_and_zero_padding(lib):
	"""sequences of 128, 70 and 5 rows in slots of 128: the even forms are out (legal_forms), padding rows are zeros in both forms (check_case)"""
	assert legal_forms(3, 128, True) == [GENERIC, STRIPS]
	check_case(lib, 3, 128, STRIPS, tlen=[128, 70, 5])
	assert legal_forms(2, 1088, True) == [GENERIC, STRIPS]      # the product's shape, ragged: strips where a full batch takes the even form
	check_case(lib, 2, 1088, STRIPS, tlen=[1088, 1000])


def test_preconditions_and_illegal_forms_are_refused(lib):
	"""what the kernels take for granted comes back as TTK_E_ARG with a message, before anything is launched: `out` keeps its NaN"""
	l, _lib = lib
	x = torch.zeros(2 * 1100 * CH, device=DEV)
	ms = torch.zeros(2 * 32 * 64 * 3, device=DEV)
	v = torch.ones(2 * CH + 8, device=DEV)
	out = torch.full((2 * 1100 * CH,), float("nan"), device=DEV)
	idx = torch.zeros(1100, dtype=torch.int32, device=DEV)
	tl = torch.ones(64, dtype=torch.int32, device=DEV)

	def desc(**kw):
		d = _lib.GnDesc()
		d.x, d.ms, d.gamma, d.beta, d.out = x.data_ptr(), ms.data_ptr(), v.data_ptr(), v.data_ptr(), out.data_ptr()
		d.nb, d.T, d.Tout, d.C, d.stats = 2, 1088, 1088, CH, 1
		for k, val in kw.items():
			setattr(d, k, val)
		return d

	def refused(d, match, dt=1):
		assert l.ttk_gn_apply(dt, C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), l.ttk_last_error().decode()
	for name in ("x", "ms", "gamma", "beta", "out"):
		refused(desc(**{name: None}), "null")
	refused(desc(), "dtype", dt=3)
	refused(desc(C=1152), "C must be")
	refused(desc(C=64), "C must be")
	refused(desc(C=384), "C must be")
	refused(desc(nb=0), "nb >= 1")
	refused(desc(T=0, Tout=0), "T >= 1")
	refused(desc(Tout=1000), "needs row_idx")
	refused(desc(tlen=tl.data_ptr(), row_idx=idx.data_ptr()), "tlen needs")
	refused(desc(nb=1, T=64 * 64 + 1, Tout=64 * 64 + 1), "64 statistics chunks")
	refused(desc(scale=v.data_ptr()), "come together")
	refused(desc(scale=v.data_ptr(), shift=v.data_ptr(), ss_stride=1026), "% 4 == 0")
	for name in ("x", "gamma", "beta", "out"):
		refused(desc(**{name: getattr(desc(), name) + 4}), "16-byte aligned")
	refused(desc(scale=v.data_ptr() + 4, shift=v.data_ptr()), "16-byte aligned")
	refused(desc(act=1), "act must be")
	refused(desc(out_f8=1), "out_f8 only with TTK_BF16", dt=0)
	refused(desc(out_f8=1), "out_f8 only with TTK_BF16", dt=4)
	refused(desc(pf=v.data_ptr(), pf_bytes=1024, pf_taps=0), "pf_taps >= 1")
	refused(desc(form=6), "form must be")
	refused(desc(form=-1), "form must be")
	for form in (STRIPS, EVEN9, EVEN12, EVEN18):
		refused(desc(form=form, C=512), "C == 1024")
		refused(desc(form=form, row_idx=idx.data_ptr()), "no row_idx")
		refused(desc(form=form, row_idx=idx.data_ptr(), Tout=1000), "Tout == T")
	for form in (EVEN9, EVEN12, EVEN18):
		refused(desc(form=form, tlen=tl.data_ptr()), "no tlen")
		refused(desc(form=form, nb=65, T=16, Tout=16), "nb <= 64")
		refused(desc(form=form, nb=2, T=500, Tout=500), "at least 4 rows")      # q = 3
	refused(desc(form=EVEN9, nb=64, T=37, Tout=37), "at most 9 / 12 / 18")        # 10 rows
	refused(desc(form=EVEN12, nb=2, T=1600, Tout=1600), "at most 9 / 12 / 18")    # 13 rows
	refused(desc(form=EVEN18, nb=2, T=2305, Tout=2305), "at most 9 / 12 / 18")    # 19 rows
	refused(desc(form=EVEN12, nb=1, T=1600, Tout=1600), "24 statistics chunks")   # 7 rows, 25 chunks
	refused(desc(form=EVEN9, nb=1, T=1600, Tout=1600), "24 statistics chunks")
	torch.cuda.synchronize()
	assert bool(torch.isnan(out).all()), "a refused call launched something"
	assert l.ttk_gn_apply(1, C.byref(desc()), _lib.stream_ptr()) == 0      # the base descriptor itself is fine
	torch.cuda.synchronize()
