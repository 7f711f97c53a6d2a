"""Float64 references of the side networks' own kernels -- the AttentionBlock of the conditioning encoders and the classifier (csrc/ttk_attn_block.h: k_cond_gn,
k_attn_rowwave), the conditioning stem and pooling (csrc/cond.hip: k_cond_im2col, k_cond_pool) and CLVP's small kernels (csrc/clvp.hip: k_embed_rows, k_rmsnorm,
k_rotary, k_geglu, k_mean_rows, k_clvp_score) -- written from the definition over the kernels' own operands, with a derived per-element error bound, the operands
and case lists that tests/test_side_ref.py (CPU) and tests/test_gpu_side_forms.py (GPU, through the ttk_*_rows entry points of include/ttk.h) share, and a float32
emulation of each kernel's arithmetic with switchable faults that shows the bound and the canaries can see them.

A reference is an IMAGE of the buffer a launch writes into: the float64 value where the launch owes one, NaN where it owes nothing (the pad columns of a strided
output row); the bound has the same shape.  A bound of 0 means the element is owed EXACTLY: every element of im2col, embed_rows and pool mode 0, features 32..63
of every rotary head, the outputs of an all-zero RMSNorm row or score latent.

THE BOUNDS, per element.  u = 2^-24, one rounding per f32 operation in the order the kernel performs it; a sum is bounded by the kernel's ACTUAL DEPTH (the
additions on a path from an element to the result: a thread's or lane's partial sum in order, then the balanced tree of wave_sum / block_sum256), as norm_ref.py
argues.  TRANS = 2e-6 relative for erff, sincosf, expf, sqrtf and rsqrtf (the project's constant for a transcendental); out_rounding = norm_ref.out_rounding, half an
ulp of bf16 at |v| + tol.  1.01 / 1.02 cover second order.  No term is fitted to a GPU result.
  k_cond_gn, n = T C / groups values per (batch element, group), D1 = ceil(n / 256) + 8 (thread partial, 6 DPP / readlane levels, 2 levels over the 4 waves), D2 = D1 + 1:
    mean = s / n           dmean = 1.01 D1 u sum|x| / n + u |mean|
    q = sum (x - mean)^2   dq = n dmean^2 + 1.01 (D2 + 3) u (q + n dmean^2)              (two-pass: sum (x - mean) = 0, no cancellation term; norm_ref.py)
    var = q / n            dvar = dq / n + u var
    rstd = rsqrtf(var+eps) drel = 1.02 (dvar + u (var + eps)) / (2 (var + eps)) + TRANS
    a = x - mean: da = dmean + u |a|;  e = a rstd: de = da rstd + |e| (drel + u);  f = e gamma: df = (de + u |e|) |gamma|;  y = f + beta: dy = df + u |y|
  k_attn_rowwave (head width 128), per query q of head h; v_j = score + bias, w_j the softmax weights, mag_j = scale sum_d |q_d| |k_jd|, Mabs = max_j |v_j|:
    qs_d = q_d scale (u), s_j = sum_d qs_d k_jd: 128 sequential steps       ds_j = 1.01 * 130 u mag_j
    v_j = s_j + bias[h][clamp(j - q, -64, 64) + 64]                          dv_j = ds_j + u |v_j|
    e_j = __expf(v_j - m): the maximum m cancels in e_j / l, so only the rounding of the difference (u 2 Mabs) and the intrinsic count.  __expf(a) is
          v_exp_f32(a LOG2E): the product's rounding and LOG2E as an f32 constant (2u |a| in the exponent, |a| <= 2 Mabs) and v_exp_f32 at one ulp, 2^-23 = 2u, as
          attn_ref.py states it:            E_j = 1.01 (dv_j + 6 u Mabs + 2u)       relative; derived, not measured.  An e_j below 2^-126 is flushed to 0: 1e-37 absolute.
    l = sum_j e_j: a lane's keys in order, then the tree                     EL = 1.01 (ceil(T / 64) + 6) u     relative (all terms positive)
    o_d = sum_j e_j v_jd: T sequential steps                                 EA = 1.01 T u                      relative to sum_j w_j |v_jd|
    out_d = o_d (1 / l)   |d out_d| <= 1.02 sum_j w_j [(E_j + EA) |v_jd| + (E_j + EL) |out_d|] + 3u |out_d| + 1e-37
          (first order in the weights' relative errors; test_side_ref.py asserts E_j < 2^-6 on every case)
  k_rmsnorm, D = ceil(d / 256) + 4 + 6 (four squares per slot, the lane's slots in order, the tree), all terms positive:
    ss: relative 1.01 (D + 1) u;   norm = max(sqrtf(ss) rsqrtf(d), 1e-8): dn = 1.01 ((D + 1) u / 2 + 2 TRANS + u) relative;   y = x / norm g: dy = |y| (dn + 3u).
    An all-zero row is 0 / 1e-8 g = 0: owed exactly.  (The rows of the cases have norm >= 0.1 or are zero: the clamp never sits on the edge.)
  k_rotary: a = (row % S) inv_freq[i] (u |a|);  sincosf: ds = u |a| + TRANS |sin a|, dc = u |a| + TRANS |cos a| (voc_ref.py's form: the argument's rounding, then the
    function's own error);  x1 c - x2 s and x2 c + x1 s: |x1| dc + |x2| ds + 1.01 * 2u (|x1 c| + |x2 s|), and the mirror image.  Features 32..63: exact.
  k_geglu: a = g 0.70710678f (2u |a|: the constant and the product);  r = erff(a): dr = 1.01 (2 / sqrt(pi)) exp(-a^2) 2u |a| + TRANS |r|;  t = 1 + r: dt = dr + u |t|;
    m = (0.5 g) t: dm = |0.5 g| dt + u |m|;  out = v m: |v| dm + u |out|.
  k_mean_rows, k_cond_pool mode 1: S sequential additions and one division: 1.01 S u sum|x| / S + u |y|.
  k_clvp_score, D = ceil(d / 64) + 6: tt, ss relative 1.01 (D + 1) u, ts absolute 1.01 (D + 1) u sum|t s|;  each norm max(sqrtf(.), 1e-12): (D + 1) u / 2 + TRANS;
    the product of the norms u, the division 2u, expf(temperature) TRANS, the last product u:
    dscore = 1.01 (D + 1) u sum|t s| / (|t| |s|) exp(temp) + |score| 1.01 ((D + 1) u + 3 TRANS + 4u).  A zero latent gives 0 / (1e-12 |t|) = 0: owed exactly.
Every output in T is rounded once more: + out_rounding.

OPERANDS (seeded CPU generator; T-typed inputs -- the row-wave qkv, the rotary's qkv, the GEGLU's h -- lie on the bf16 grid, so the reference sees the kernel's own
inputs).  GroupNorm: N(0, 1) around a different mean per batch element, one case with mean 30 and deviation 0.1 (a one-pass variance fails there).  Row-wave: q, k, v
N(0, 1) in the head-major layout the AttentionBlock uses (q_off 0, k_off 128, v_off 256, head_stride 384), scale 128^-1/2, bias N(0, 1.5); the "hot" case makes every
query's largest score HOT_SCORE = 96 (within 2 %): above ln(FLT_MAX) = 88.7, where a softmax without the maximum subtracted overflows (the issue's "near 80" does
not overflow: expf(80) = 5.5e34 is finite, so the case sits where the fault it names can show; test_side_ref.py asserts the range).  GEGLU gates are spread evenly over [-6, 6].

THE EMULATIONS follow the code: k_cond_gn's thread tid owns elements tid + 256 i, partials in order, block_sum256 as the balanced tree it is (quad swaps, half mirror,
mirror, the four rows, the four waves: neighbours, pairs, quads ... in lane order; a + b commutes, so the mirrored steps add the same pairs); k_rmsnorm's and
k_clvp_score's lanes own slots lane + 64 i; the row-wave's passes in order (q scale, the 128-step dot product, bias, max, __expf, the lane-strided l, the T-step P V,
one reciprocal).  Products that feed a sum are contracted into fma (the compiler's default); either choice lies inside the bound, which counts one rounding per
written operation.  Faults are switched on by name (FAULTS[kernel]).  The T = 3584 row-wave case is emulated on EMU_ROWS query rows only (the full 3584 x 3584 x 128
sequential dot product is minutes of CPU time and shows nothing the first, middle and last rows do not).
"""
import functools
import math
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from norm_ref import U, EPS, TDT, away, out_rounding, _tree_sum, _fma, _rsqrt

TRANS = 2e-6
NAN = float("nan")
SCALE128 = float(torch.tensor(1.0 / math.sqrt(128.0), dtype=torch.float32))      # attn_blocks: 1.f / sqrtf((float)hd)
ROWWAVE_MAX_T = 3584
EMU_ROWS = (0, 1, 2, 3, 63, 64, 1791, 3519, 3520, 3582, 3583)
TEMPERATURE = 0.7
HOT_SCORE = 96.0                       # the largest score of every query row of the "hot" row-wave case: above ln(FLT_MAX) = 88.72
DT_CODE = {"f32": 0, "bf16": 1}


@dataclass(frozen=True)
class Case:
	kernel: str
	name: str
	dt: str                    # the kernel's T: "f32" | "bf16"
	items: tuple               # the shape parameters, (key, value) pairs

	@property
	def p(self):
		return SimpleNamespace(**dict(self.items))

	@property
	def id(self):
		return f"{self.kernel}-{self.name}-{self.dt}"

	@property
	def group(self):
		return f"{self.kernel} {'f32' if self.dt == 'f32' else 'rounded'}"

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())


def case(kernel, name, dt, **kw):
	return Case(kernel, name, dt, tuple(sorted(kw.items())))


def gen(c):
	return torch.Generator().manual_seed(c.seed)


def to_T(v, dt):
	"""an f32 result as the kernel stores it in T, read back as f64"""
	return v.float().to(TDT[dt]).double()


def on_grid(t, dt):
	"""operand values of type T as f32: the bf16 grid for bf16, untouched for f32"""
	return t.to(TDT[dt]).float()


def rounded(y, tol, dt):
	return tol + out_rounding(y, tol, dt)


def _f32(v):
	return torch.tensor(float(v), dtype=torch.float32)


def _lane_tree(v, lanes):
	"""sum over the last dimension the way a strided loop + tree does it: element e belongs to lane e % lanes, a lane adds its elements in order, then the balanced tree"""
	n = v.shape[-1]
	pad = (n + lanes - 1) // lanes * lanes
	z = torch.zeros(*v.shape[:-1], pad, dtype=torch.float32)
	z[..., :n] = v
	z = z.reshape(*v.shape[:-1], pad // lanes, lanes)
	s = torch.zeros(*v.shape[:-1], lanes, dtype=torch.float32)
	for i in range(pad // lanes):
		s = s + z[..., i, :]
	return _tree_sum(s)


# =========================================================================================================== k_cond_gn
GN_SHAPES = ((1, 128, 32), (5, 48, 16), (67, 1024, 32), (130, 2048, 32))      # (T, C, groups): n = 4 < 256 threads; cpg 3; n % 256 != 0; the product's cpg 64
GN_CASES = [case("gn", f"T{T}-C{C}-g{g}", dt, T=T, C=C, groups=g, nb=2, offset=0) for (T, C, g) in GN_SHAPES for dt in ("f32", "bf16")] + \
		   [case("gn", "T67-C1024-g32-mean30", dt, T=67, C=1024, groups=32, nb=2, offset=1) for dt in ("f32", "bf16")]


def gn_ops(c):
	p, g = c.p, gen(c)
	x = torch.randn(p.nb, p.T, p.C, generator=g)
	if p.offset:
		x = x * 0.1 + torch.tensor([30.0, -30.0])[:p.nb, None, None]
	else:
		x = x + torch.tensor([0.75, -2.0])[:p.nb, None, None]
	return {"x": x, "gamma": away(g, p.C, 1.4, 2.2), "beta": away(g, p.C, 0.3, 0.8)}


@functools.lru_cache(maxsize=None)
def gn_ref(c):
	p, o = c.p, gn_ops(c)
	cpg = p.C // p.groups
	n = p.T * cpg
	x = o["x"].double().reshape(p.nb, p.T, p.groups, cpg)
	gamma, beta = o["gamma"].double().reshape(1, 1, p.groups, cpg), o["beta"].double().reshape(1, 1, p.groups, cpg)
	D1 = (n + 255) // 256 + 8
	D2 = D1 + 1
	mean = x.mean((1, 3), keepdim=True)
	a = x - mean
	q = (a * a).sum((1, 3), keepdim=True)
	var = q / n
	rstd = 1 / torch.sqrt(var + EPS)
	dmean = 1.01 * D1 * U * x.abs().sum((1, 3), keepdim=True) / n + U * mean.abs()
	dq = n * dmean ** 2 + 1.01 * (D2 + 3) * U * (q + n * dmean ** 2)
	dvar = dq / n + U * var
	drel = 1.02 * (dvar + U * (var + EPS)) / (2 * (var + EPS)) + TRANS
	assert float(drel.max()) < 0.25
	e = a * rstd
	y = e * gamma + beta
	da = dmean + U * a.abs()
	de = da * rstd + e.abs() * (drel + U)
	dy = (de + U * e.abs()) * gamma.abs() + U * y.abs()
	y, dy = y.reshape(p.nb, p.T, p.C), dy.reshape(p.nb, p.T, p.C)
	return y, rounded(y, dy, c.dt)


def gn_emu(c, fault=None):
	p, o = c.p, gn_ops(c)
	cpg = p.C // p.groups
	n = p.T * cpg
	x = o["x"].reshape(p.nb, p.T, p.groups, cpg).permute(0, 2, 1, 3).reshape(p.nb, p.groups, n)      # element e = t * cpg + c
	nn = _f32((n + 255) // 256 * 256 if fault == "n_counted_as_a_multiple_of_256" else n)
	live = torch.arange((n + 255) // 256 * 256) < n
	mean = _lane_tree(x, 256) / nn
	if fault == "one_pass_variance":
		var = _lane_tree(x * x, 256) / nn - mean * mean
	else:
		pad = torch.zeros(p.nb, p.groups, live.numel(), dtype=torch.float32)
		pad[..., :n] = x
		dd = torch.where(live, pad - mean[..., None], torch.zeros(1)).reshape(p.nb, p.groups, -1, 256)
		qq = torch.zeros(p.nb, p.groups, 256, dtype=torch.float32)
		for i in range(dd.shape[2]):
			qq = _fma(dd[:, :, i], dd[:, :, i], qq)
		var = _tree_sum(qq) / nn
	rstd = _rsqrt(var + _f32(EPS))
	ch = torch.arange(cpg) if fault == "affine_indexed_within_the_group" else torch.arange(p.C).reshape(p.groups, cpg)
	gamma, beta = o["gamma"][ch], o["beta"][ch]                                       # [groups][cpg] (or [cpg]: broadcast over the groups)
	xg = o["x"].reshape(p.nb, p.T, p.groups, cpg)
	y = _fma((xg - mean[:, None, :, None]) * rstd[:, None, :, None], gamma, beta)
	return to_T(y.reshape(p.nb, p.T, p.C), c.dt)


# =========================================================================================================== k_attn_rowwave
def _rw(name, dt, T, **kw):
	d = dict(T=T, nb=2, H=2, bias=0, ld_extra=0, ldo_extra=0, hot=0)
	d.update(kw)
	return case("rowwave", name, dt, **d)


RW_T = (1, 3, 4, 5, 63, 64, 65, 130, 200)
RW_CASES = [_rw(f"T{T}-{'bias' if b else 'plain'}", dt, T, bias=b) for T in RW_T for b in (0, 1) for dt in ("f32", "bf16")] + \
		   [_rw("T65-strided-bias", dt, 65, bias=1, ld_extra=16, ldo_extra=8) for dt in ("f32", "bf16")] + \
		   [_rw("T130-hot-bias", dt, 130, bias=1, hot=1) for dt in ("f32", "bf16")] + \
		   [_rw("T3584-limit-bias", "f32", ROWWAVE_MAX_T, nb=1, H=1, bias=1)]


def rw_layout(c):
	"""(ld, ldo, q_off, k_off, v_off, head_stride) of the AttentionBlock's head-major qkv"""
	p = c.p
	return 3 * 128 * p.H + p.ld_extra, 128 * p.H + p.ldo_extra, 0, 128, 256, 384


@functools.lru_cache(maxsize=None)
def rw_ops(c):
	"""q, k, v f32 [nb][H][T][128] (values of T), bias f32 [H][129] or None"""
	p, g = c.p, gen(c)
	q, k, v = (on_grid(torch.randn(p.nb, p.H, p.T, 128, generator=g), c.dt) for _ in range(3))
	if p.hot:      # every query scaled to |q|^2 = HOT_SCORE / scale and the keys a permutation of the queries: each row's largest score is q.q scale ~ HOT_SCORE,
		# the others HOT_SCORE cos(q, q') ~ N(0, 8.5)
		q = on_grid(q * torch.sqrt(HOT_SCORE / SCALE128 / q.pow(2).sum(-1, keepdim=True)), c.dt)
		k = torch.stack([torch.stack([q[b, h][torch.randperm(p.T, generator=g)] for h in range(p.H)]) for b in range(p.nb)])
	bias = (torch.randn(p.H, 129, generator=g) * 1.5) if p.bias else None
	return {"q": q, "k": k, "v": v, "bias": bias}


def rw_pack(c, o):
	"""the qkv buffer as f32 values [nb * T][ld], NaN in the pad columns"""
	p = c.p
	ld, _, qo, ko, vo, hs = rw_layout(c)
	buf = torch.full((p.nb, p.T, ld), NAN)
	for h in range(p.H):
		for off, t in ((qo, o["q"]), (ko, o["k"]), (vo, o["v"])):
			buf[:, :, off + h * hs:off + h * hs + 128] = t[:, h]
	return buf.reshape(p.nb * p.T, ld)


def rw_rel_index(T, rows=None):
	qi = torch.arange(T) if rows is None else torch.tensor(rows)
	return (torch.arange(T)[None, :] - qi[:, None]).clamp(-64, 64) + 64


@functools.lru_cache(maxsize=None)
def rw_ref(c):
	"""(image f64 [nb * T][ldo], tol, facts): facts = the largest E_j, the largest and smallest per-query maximum score"""
	p, o = c.p, rw_ops(c)
	_, ldo, *_ = rw_layout(c)
	T = p.T
	img = torch.full((p.nb, T, ldo), NAN, dtype=torch.float64)
	tol = torch.full((p.nb, T, ldo), NAN, dtype=torch.float64)
	EA, EL = 1.01 * T * U, 1.01 * ((T + 63) // 64 + 6) * U
	Emax, mhi, mlo = 0.0, -1e30, 1e30
	for b in range(p.nb):
		for h in range(p.H):
			k, v = o["k"][b, h].double(), o["v"][b, h].double()
			for q0 in range(0, T, 512):
				q = o["q"][b, h, q0:q0 + 512].double()
				s = SCALE128 * (q @ k.t())
				mag = SCALE128 * (q.abs() @ k.abs().t())
				if o["bias"] is not None:
					s = s + o["bias"][h].double()[rw_rel_index(T, list(range(q0, min(T, q0 + 512))))]
				Mabs = s.abs().max(1, keepdim=True).values
				E = 1.01 * (1.01 * 130 * U * mag + U * s.abs() + 6 * U * Mabs + 2 * U)
				w = torch.softmax(s, 1)
				out = w @ v
				wE = w * E
				t = 1.02 * (wE @ v.abs() + EA * (w @ v.abs()) + out.abs() * (wE.sum(1, keepdim=True) + EL)) + 3 * U * out.abs() + 1e-37
				img[b, q0:q0 + 512, h * 128:(h + 1) * 128], tol[b, q0:q0 + 512, h * 128:(h + 1) * 128] = out, t
				Emax, mhi, mlo = max(Emax, float(E.max())), max(mhi, float(s.max(1).values.max())), min(mlo, float(s.max(1).values.min()))
	img, tol = img.reshape(p.nb * T, ldo), tol.reshape(p.nb * T, ldo)
	owed = ~torch.isnan(img)
	tol[owed] = rounded(img[owed], tol[owed], c.dt)
	return img, tol, {"Emax": Emax, "max_hi": mhi, "max_lo": mlo}


def _expf(a):
	return torch.exp(a.double()).float()


def rw_emu(c, fault=None, rows=None):
	"""the out image f64 [nb * T][ldo]; with `rows`, only those query rows are computed (the others stay NaN)"""
	p, o = c.p, rw_ops(c)
	_, ldo, *_ = rw_layout(c)
	T = p.T
	rows = list(range(T)) if rows is None else list(rows)
	img = torch.full((p.nb, T, ldo), NAN, dtype=torch.float64)
	scale = _f32(SCALE128)
	for b in range(p.nb):
		for h in range(p.H):
			k, v = o["k"][b, h], o["v"][b, h]
			if fault == "v_read_at_the_k_offset":
				v = k
			qs = o["q"][b, h][rows] * scale
			s = torch.zeros(len(rows), T, dtype=torch.float32)
			for d in range(128):
				s = _fma(qs[:, d:d + 1], k[None, :, d], s)
			if fault == "scale_applied_twice":
				s = s * scale
			if o["bias"] is not None:
				idx = rw_rel_index(T, rows)
				if fault == "bias_at_q_minus_k":
					idx = 128 - idx
				elif fault == "clamp_at_63":
					idx = idx.clamp(1, 127)
				bb = o["bias"].reshape(-1)[idx + (0 if fault == "bias_index_without_head" else h * 129)]
				s = s + bb
			m = torch.zeros(len(rows), 1) if fault == "no_max_subtraction" else s.max(1, keepdim=True).values
			e = _expf(s - m)
			l = _lane_tree(e, 64)
			if fault == "l_over_padded_keys":      # the lanes past T add what the strip holds there: zeros, e = exp(0 - m)
				l = l + _f32((T + 63) // 64 * 64 - T) * _expf(-m[:, 0])
			acc = torch.zeros(len(rows), 128, dtype=torch.float32)
			for j in range(T):
				acc = _fma(e[:, j:j + 1], v[j][None, :], acc)
			out = acc * (_f32(1.0) / l)[:, None]
			img[b, rows, h * 128:(h + 1) * 128] = to_T(out, c.dt)
	return img.reshape(p.nb * T, ldo)


# =========================================================================================================== k_cond_im2col (exact)
def _im(name, dt, layout, Tin, **kw):
	d = dict(layout=layout, Tin=Tin, nb=2, Cin=5, taps=3, stride=2, pad=1, Kpad=32)
	d.update(kw)
	d["Tout"] = (Tin + 2 * d["pad"] - d["taps"]) // d["stride"] + 1
	return case("im2col", f"{name}-{layout}", dt, **d)


IM_CASES = [_im(f"Tin{Tin}", dt, lay, Tin) for Tin in (1, 2, 5, 6) for lay in ("cf", "cl") for dt in ("f32", "bf16")] + \
		   [_im("taps1-Tin5", dt, lay, 5, taps=1, stride=1, pad=0) for lay in ("cf", "cl") for dt in ("f32", "bf16")] + \
		   [_im(f"Cin100-Tin{Tin}", dt, lay, Tin, Cin=100, Kpad=320) for Tin, lay in ((5, "cf"), (6, "cl")) for dt in ("f32", "bf16")]
assert all(c.p.Tout == (c.p.Tin - 1) // 2 + 1 for c in IM_CASES if c.p.taps == 3)


def im_ops(c):
	"""src f32 flat, with its element strides: channels-first [nb][Cin][Tin] or channels-last [nb][Tin][Cin]"""
	p = c.p
	src = torch.randn(p.nb * p.Cin * p.Tin, generator=gen(c))
	sb, sc, st = (p.Cin * p.Tin, p.Tin, 1) if p.layout == "cf" else (p.Tin * p.Cin, 1, p.Cin)
	return {"src": src, "sb": sb, "sc": sc, "st": st}


def _im_gather(c, o, order="c_taps", pad=None, guard_right=True):
	p = c.p
	pad = p.pad if pad is None else pad
	flat = torch.cat([o["src"], torch.full((p.taps * max(o["st"], 1) + 1,), NAN)])      # what lies behind the source stands in as NaN
	out = torch.zeros(p.nb, p.Tout, p.Kpad, dtype=torch.float32)
	b, t, k = torch.meshgrid(torch.arange(p.nb), torch.arange(p.Tout), torch.arange(p.Cin * p.taps), indexing="ij")
	ch, j = (k // p.taps, k % p.taps) if order == "c_taps" else (k % p.Cin, k // p.Cin)
	ts = t * p.stride + j - pad
	ok = (ts >= 0) & ((ts < p.Tin) if guard_right else (ts <= p.Tin))
	idx = (b * o["sb"] + ch * o["sc"] + ts * o["st"]).clamp(0, flat.numel() - 1)
	out[:, :, :p.Cin * p.taps] = torch.where(ok, flat[idx], torch.zeros(1))
	return out.reshape(p.nb * p.Tout, p.Kpad)


def im_ref(c):
	o = im_ops(c)
	y = to_T(_im_gather(c, o), c.dt)
	want = torch.zeros_like(y)      # the definition, with F.unfold's indexing spelled out as loops over the few taps
	p = c.p
	x = o["src"].reshape(p.nb, p.Cin, p.Tin) if p.layout == "cf" else o["src"].reshape(p.nb, p.Tin, p.Cin).transpose(1, 2)
	for t in range(p.Tout):
		for j in range(p.taps):
			ts = t * p.stride + j - p.pad
			if 0 <= ts < p.Tin:
				want.view(p.nb, p.Tout, p.Kpad)[:, t, j:p.Cin * p.taps:p.taps] = to_T(x[:, :, ts], c.dt)
	assert torch.equal(y, want)
	return y, torch.zeros_like(y)


def im_emu(c, fault=None):
	o = im_ops(c)
	return to_T(_im_gather(c, o, order="taps_c" if fault == "k_is_tap_major" else "c_taps", pad=0 if fault == "pad_0" else None,
						   guard_right=fault != "right_edge_read_past_Tin"), c.dt)


# =========================================================================================================== k_cond_pool
POOL_CASES = [case("pool", f"mode{m}-T{T}-C{C}", "f32", mode=m, T=T, C=C, nb=2) for m in (0, 1) for T in (1, 2, 130) for C in (128, 300)]


def pool_ops(c):
	p = c.p
	return {"x": torch.randn(p.nb, p.T, p.C, generator=gen(c)) + torch.tensor([1.5, -0.75])[:, None, None]}


def _mean_ref(x, dt):
	"""the mean over dimension 1 of x f64 [B][S][d] and the bound of S sequential f32 additions and one division"""
	S = x.shape[1]
	y = x.mean(1)
	return y, rounded(y, 1.01 * S * U * x.abs().sum(1) / S + U * y.abs(), dt)


def _mean_emu(x, div):
	s = torch.zeros(x.shape[0], x.shape[2], dtype=torch.float32)
	for t in range(x.shape[1]):
		s = s + x[:, t]
	return s / _f32(div)


def pool_ref(c):
	x = pool_ops(c)["x"].double()
	if c.p.mode == 0:
		return x[:, 0].clone(), torch.zeros(x.shape[0], x.shape[2], dtype=torch.float64)
	return _mean_ref(x, "f32")


def pool_emu(c, fault=None):
	x = pool_ops(c)["x"]
	if c.p.mode == 0 and fault != "mean_where_position_0_is_asked":
		return x[:, 0].double()
	return _mean_emu(x, c.p.T).double()      # s = base[0], then rows 1 .. T-1: the same additions as from 0.f


# =========================================================================================================== k_embed_rows (exact)
EMBED_CASES = [case("embed", "B2-S5-stride9", "f32", B=2, S=5, stride=9, d=64, vocab=11)]


def embed_ops(c):
	p, g = c.p, gen(c)
	ids = torch.randint(0, p.vocab, (p.B, p.stride), generator=g)
	ids[0, 1], ids[1, 3] = -3, p.vocab + 2      # both clamped
	ids[:, p.S:] = 10 ** 12                     # what lies behind a row's S ids is never an index
	return {"emb": torch.randn(p.vocab, p.d, generator=g), "ids": ids}


def embed_ref(c):
	o, p = embed_ops(c), c.p
	y = o["emb"][o["ids"][:, :p.S].clamp(0, p.vocab - 1).reshape(-1)].double()
	return y, torch.zeros_like(y)


def embed_emu(c, fault=None):
	o, p = embed_ops(c), c.p
	ids = o["ids"].reshape(-1)[:p.B * p.S] if fault == "ids_read_densely" else o["ids"][:, :p.S].reshape(-1)
	return o["emb"][ids.clamp(0, p.vocab - 1)].double()


# =========================================================================================================== k_rmsnorm
RMS_CASES = [case("rmsnorm", f"r{r}-d{d}", dt, rows=r, d=d) for r in (1, 5) for d in (64, 256, 768) for dt in ("f32", "bf16")]


def rms_ops(c):
	p, g = c.p, gen(c)
	x = torch.randn(p.rows, p.d, generator=g) * (0.25 + torch.arange(p.rows).float())[:, None]
	if p.rows > 1:
		x[3] = 0      # the guard row of the second workgroup's neighbours: an all-zero row owes zeros
	return {"x": x, "g": away(g, p.d, 0.6, 1.8)}


def rms_ref(c):
	p, o = c.p, rms_ops(c)
	x, g = o["x"].double(), o["g"].double()
	D = (p.d + 255) // 256 + 10
	norm = (x.pow(2).sum(1, keepdim=True).sqrt() * p.d ** -0.5).clamp_min(1e-8)
	assert all(float(n) == 1e-8 or float(n) >= 0.1 for n in norm)
	y = x / norm * g
	dn = 1.01 * ((D + 1) * U / 2 + 2 * TRANS + U)
	dy = y.abs() * (dn + 3 * U)
	return y, torch.where(y == 0, torch.zeros_like(dy), rounded(y, dy, c.dt))


def rms_emu(c, fault=None):
	p, o = c.p, rms_ops(c)
	x = o["x"]
	pad = (p.d + 255) // 256 * 256
	z = torch.zeros(p.rows, pad)
	z[:, :p.d] = x
	z = z.reshape(p.rows, pad // 256, 64, 4)      # lane l owns the float4 slots l + 64 i
	ss = torch.zeros(p.rows, 64, dtype=torch.float32)
	for i in range(z.shape[1]):
		v = z[:, i]
		ss = ss + _fma(v[..., 3], v[..., 3], _fma(v[..., 2], v[..., 2], _fma(v[..., 1], v[..., 1], v[..., 0] * v[..., 0])))
	ss = _tree_sum(ss)
	norm = torch.sqrt(ss.double()).float()
	if fault != "mean_square_without_d_to_the_minus_half":
		norm = norm * _rsqrt(_f32(p.d))
	if fault != "clamp_dropped":
		norm = norm.clamp_min(_f32(1e-8))
	return to_T(x / norm[:, None] * o["g"], c.dt)


# =========================================================================================================== k_rotary
ROT_CASES = [case("rotary", f"S{S}-H{H}", dt, B=2, S=S, H=H) for S in (1, 5, 250) for H in (1, 12) for dt in ("f32", "bf16")]
INV_FREQ = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).float()      # RotaryEmbedding(32).inv_freq


def rot_ops(c):
	p = c.p
	return {"qkv": on_grid(torch.randn(p.B * p.S, 3 * p.H, 64, generator=gen(c)), c.dt), "inv_freq": INV_FREQ}


def rot_ref(c):
	p, o = c.p, rot_ops(c)
	x = o["qkv"].double()
	pos = (torch.arange(p.B * p.S) % p.S).double()
	a = pos[:, None, None] * INV_FREQ.double()[None, None, :]
	sn, cs = torch.sin(a), torch.cos(a)
	dsn, dcs = U * a.abs() + TRANS * sn.abs(), U * a.abs() + TRANS * cs.abs()
	x1, x2 = x[..., :16], x[..., 16:32]
	y, tol = x.clone(), torch.zeros_like(x)
	y[..., :16], y[..., 16:32] = x1 * cs - x2 * sn, x2 * cs + x1 * sn
	tol[..., :16] = x1.abs() * dcs + x2.abs() * dsn + 1.01 * 2 * U * ((x1 * cs).abs() + (x2 * sn).abs())
	tol[..., 16:32] = x2.abs() * dcs + x1.abs() * dsn + 1.01 * 2 * U * ((x2 * cs).abs() + (x1 * sn).abs())
	tol[..., :32] = rounded(y[..., :32], tol[..., :32], c.dt)
	return y.reshape(p.B * p.S, -1), tol.reshape(p.B * p.S, -1)


def rot_emu(c, fault=None):
	p, o = c.p, rot_ops(c)
	x = o["qkv"].clone()
	row = torch.arange(p.B * p.S)
	pos = (row if fault == "position_is_the_row" else row % p.S).float()
	a = pos[:, None, None] * INV_FREQ[None, None, :]
	sn, cs = torch.sin(a.double()).float(), torch.cos(a.double()).float()
	if fault == "sin_sign_flipped":
		sn = -sn
	hi = 32 if fault == "pair_partner_at_32" else 16
	x1, x2 = x[..., :16].clone(), x[..., hi:hi + 16].clone()
	y = x.double()
	y[..., :16], y[..., hi:hi + 16] = to_T(_fma(x1, cs, -(x2 * sn)), c.dt), to_T(_fma(x2, cs, x1 * sn), c.dt)
	if fault == "v_left_unrotated":
		y[:, 2 * p.H:] = x[:, 2 * p.H:].double()
	return y.reshape(p.B * p.S, -1)


# =========================================================================================================== k_geglu
GEGLU_CASES = [case("geglu", f"r3-i{i}", dt, rows=3, inner=i) for i in (64, 1536) for dt in ("f32", "bf16")]


def geglu_ops(c):
	p, g = c.p, gen(c)
	val = torch.randn(p.rows, p.inner, generator=g)
	gate = torch.linspace(-6, 6, p.rows * p.inner)[torch.randperm(p.rows * p.inner, generator=g)].reshape(p.rows, p.inner)
	return {"h": on_grid(torch.cat([val, gate], 1), c.dt)}


def geglu_ref(c):
	p, o = c.p, geglu_ops(c)
	v, g = o["h"][:, :p.inner].double(), o["h"][:, p.inner:].double()
	a = g * math.sqrt(0.5)
	r = torch.erf(a)
	dr = 1.01 * (2 / math.sqrt(math.pi)) * torch.exp(-a * a) * 2 * U * a.abs() + TRANS * r.abs()
	t = 1 + r
	dt_ = dr + U * t.abs()
	m = 0.5 * g * t
	dm = (0.5 * g).abs() * dt_ + U * m.abs()
	y = v * m
	return y, rounded(y, v.abs() * dm + U * y.abs(), c.dt)


def geglu_emu(c, fault=None):
	p, o = c.p, geglu_ops(c)
	v, g = o["h"][:, :p.inner], o["h"][:, p.inner:]
	if fault == "halves_swapped":
		v, g = g, v
	if fault == "tanh_form_gelu":
		act = (0.5 * g.double() * (1 + torch.tanh(0.7978845608028654 * (g.double() + 0.044715 * g.double() ** 3)))).float()
	else:
		act = (0.5 * g) * (1.0 + torch.erf((g * _f32(0.70710678118654752)).double()).float())
	return to_T(v * act, c.dt)


# =========================================================================================================== k_mean_rows
MEAN_CASES = [case("mean", f"S{S}-d64", dt, B=2, S=S, d=64) for S in (1, 7, 250) for dt in ("f32", "bf16")]


def mean_ops(c):
	p = c.p
	return {"x": torch.randn(p.B, p.S, p.d, generator=gen(c)) + torch.tensor([1.5, -0.75])[:, None, None]}


def mean_ref(c):
	return _mean_ref(mean_ops(c)["x"].double(), c.dt)


def mean_emu(c, fault=None):
	return to_T(_mean_emu(mean_ops(c)["x"], c.p.S - 1 if fault == "divide_by_S_minus_1" else c.p.S), c.dt)


# =========================================================================================================== k_clvp_score
SCORE_CASES = [case("score", f"Bt{Bt}-d{d}", "f32", Bt=Bt, B=3, d=d) for Bt in (1, 3) for d in (64, 768)]


def score_ops(c):
	"""text f32 [B][d] (the launch sees the first Bt rows; with Bt == 1 the others stand for what lies behind), speech f32 [B][d] with row 1 all zero"""
	p, g = c.p, gen(c)
	text, speech = torch.randn(p.B, p.d, generator=g), torch.randn(p.B, p.d, generator=g) * 3
	speech = speech + 0.35 * text[0 if p.Bt == 1 else slice(None)] * 3      # a cosine well away from 0
	speech[1] = 0
	return {"text": text, "speech": speech, "temperature": torch.tensor([TEMPERATURE])}


def score_ref(c):
	p, o = c.p, score_ops(c)
	t = (o["text"][:1].expand(p.B, -1) if p.Bt == 1 else o["text"]).double()
	s = o["speech"].double()
	D = (p.d + 63) // 64 + 6
	E = math.exp(float(o["temperature"][0]))
	den = t.norm(dim=1).clamp_min(1e-12) * s.norm(dim=1).clamp_min(1e-12)
	y = (t * s).sum(1) / den * E
	dy = 1.01 * (D + 1) * U * (t * s).abs().sum(1) / den * E + y.abs() * 1.01 * ((D + 1) * U + 3 * TRANS + 4 * U)
	return y, torch.where(s.abs().sum(1) == 0, torch.zeros_like(dy), dy)


def score_emu(c, fault=None):
	p, o = c.p, score_ops(c)
	t = o["text"] if (p.Bt != 1 or fault == "text_row_b_where_Bt_is_1") else o["text"][:1].expand(p.B, -1)
	s = o["speech"]

	def dot(a, b):
		n = a.shape[1]
		acc = torch.zeros(a.shape[0], 64, dtype=torch.float32)
		for i in range((n + 63) // 64):
			acc = _fma(a[:, 64 * i:64 * i + 64], b[:, 64 * i:64 * i + 64], acc)
		return _tree_sum(acc)
	tt, ss, ts = dot(t, t), dot(s, s), dot(t, s)
	sq = lambda v: torch.sqrt(v.double()).float().clamp_min(_f32(1e-12))
	temp = o["temperature"][0]
	return (ts / (sq(tt) * sq(ss)) * (temp if fault == "temperature_not_exponentiated" else _expf(temp))).double()


# =========================================================================================================== the tables
KERNELS = {
	"gn": SimpleNamespace(cases=GN_CASES, ref=gn_ref, emu=gn_emu),
	"rowwave": SimpleNamespace(cases=RW_CASES, ref=lambda c: rw_ref(c)[:2], emu=rw_emu),
	"im2col": SimpleNamespace(cases=IM_CASES, ref=im_ref, emu=im_emu),
	"pool": SimpleNamespace(cases=POOL_CASES, ref=pool_ref, emu=pool_emu),
	"embed": SimpleNamespace(cases=EMBED_CASES, ref=embed_ref, emu=embed_emu),
	"rmsnorm": SimpleNamespace(cases=RMS_CASES, ref=rms_ref, emu=rms_emu),
	"rotary": SimpleNamespace(cases=ROT_CASES, ref=rot_ref, emu=rot_emu),
	"geglu": SimpleNamespace(cases=GEGLU_CASES, ref=geglu_ref, emu=geglu_emu),
	"mean": SimpleNamespace(cases=MEAN_CASES, ref=mean_ref, emu=mean_emu),
	"score": SimpleNamespace(cases=SCORE_CASES, ref=score_ref, emu=score_emu),
}
EXACT_KERNELS = ("im2col", "embed")
ALL_CASES = [c for k in KERNELS.values() for c in k.cases]
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
GROUPS = sorted({c.group for c in ALL_CASES})

# fault name -> the cases it can show on
FAULTS = {
	"gn": {"one_pass_variance": lambda c: c.p.offset == 1, "n_counted_as_a_multiple_of_256": lambda c: (c.p.T * c.p.C // c.p.groups) % 256 != 0,
		   "affine_indexed_within_the_group": lambda c: True},
	"rowwave": {"bias_at_q_minus_k": lambda c: c.p.bias and c.p.T > 1, "clamp_at_63": lambda c: c.p.bias and c.p.T >= 130,
				"bias_index_without_head": lambda c: c.p.bias and c.p.H > 1, "no_max_subtraction": lambda c: c.p.hot == 1,
				"l_over_padded_keys": lambda c: c.p.T % 64 != 0, "scale_applied_twice": lambda c: c.p.T > 1, "v_read_at_the_k_offset": lambda c: True},
	"rmsnorm": {"mean_square_without_d_to_the_minus_half": lambda c: True, "clamp_dropped": lambda c: c.p.rows > 1},
	"rotary": {"position_is_the_row": lambda c: c.p.S > 1, "v_left_unrotated": lambda c: c.p.S > 1, "pair_partner_at_32": lambda c: True,
			   "sin_sign_flipped": lambda c: c.p.S > 1},
	"geglu": {"tanh_form_gelu": lambda c: True, "halves_swapped": lambda c: True},
	"mean": {"divide_by_S_minus_1": lambda c: c.p.S > 1},
	"score": {"text_row_b_where_Bt_is_1": lambda c: c.p.Bt == 1, "temperature_not_exponentiated": lambda c: True},
	"im2col": {"k_is_tap_major": lambda c: c.p.taps > 1, "pad_0": lambda c: c.p.pad > 0,
			   "right_edge_read_past_Tin": lambda c: (c.p.Tout - 1) * c.p.stride + c.p.taps - 1 - c.p.pad >= c.p.Tin},
	"pool": {"mean_where_position_0_is_asked": lambda c: c.p.mode == 0 and c.p.T > 1},
	"embed": {"ids_read_densely": lambda c: True},
}


def emu_rows(c):
	"""the query rows the CPU emulation of a row-wave case computes: all, but for the case at the LDS limit"""
	return EMU_ROWS if c.kernel == "rowwave" and c.p.T > 1024 else None


def check(c, got, ref=None, rows=None):
	"""worst |got - ref| / tol over what the launch owes (inf when an exactly owed element differs); AssertionError when an owed value is not finite or anything
	else was written.  got: f64, the shape of the reference image.  rows: compare these rows of the image only."""
	y, tol = ref if ref is not None else KERNELS[c.kernel].ref(c)
	assert got.shape == y.shape, f"{c.id}: image of shape {tuple(got.shape)}, reference {tuple(y.shape)}"
	if rows is not None:
		sel = torch.cat([torch.arange(b * c.p.T, (b + 1) * c.p.T)[list(rows)] for b in range(c.p.nb)])
		got, y, tol = got[sel], y[sel], tol[sel]
	owed = ~torch.isnan(y)
	assert torch.isnan(got[~owed]).all(), f"{c.id}: written where the launch owes nothing ({int((~torch.isnan(got[~owed])).sum())} elements)"
	assert torch.isfinite(got[owed]).all(), f"{c.id}: non-finite values where the launch owes a result"
	err, t = (got - y).abs()[owed], tol[owed]
	exact = t == 0
	worst = float((err[~exact] / t[~exact]).max()) if bool((~exact).any()) else 0.0
	if bool((err[exact] != 0).any()):
		worst = float("inf")
	return worst
