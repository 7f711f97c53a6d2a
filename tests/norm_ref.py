"""Float64 references of the normalisation kernels (csrc/norm.hip: k_layernorm, k_gn_stats, k_gn_apply), written from the definition over the kernels' own
operands, with a derived per-element error bound, the operands and case lists that tests/test_norm_ref.py (CPU) and tests/test_gpu_norm_forms.py (GPU,
through ttk_layernorm_rows and ttk_gn_apply) share, and a float32 emulation of the kernels' arithmetic with switchable faults that shows the bound and the
canaries can see them.

LayerNorm, per row of d f32 values:   y = (x - mean) rstd g1 + b1,   rstd = 1 / sqrt(var + 1e-5),   var = mean_k (x_k - mean)^2,
and with (g2, b2) the same again over y.  The result is written in the output type, row-major or in the decode GEMV's A-fragment order, and optionally
once more as f32 rows (out2: direct, or a slot of a ring whose base and index are read on the device).
GroupNorm32 over x f32 [nb][T][C], 32 groups of (rows x C / 32), the rows being the first tlen[b] of a sequence:
    v = act((gn(x) gamma + beta) [(1 + scale[b]) + shift[b]]),   out[b][to] = v[b][row_idx[to]],   out[b][to >= tlen[b]] = 0,
and the chunk statistics it is computed from: for every (b, group, chunk of 65536 / C rows) the triple (count, mean, M2 = sum (x - mean)^2), laid out as
include/ttk.h documents `ms`: f32 [nb][32][nchunks][3].

THE BOUND, per element.  u = 2^-24, one rounding per f32 operation.  The summations are bounded by the kernels' ACTUAL DEPTH, not by the project's habitual
"twice the worst case, any order" (2 n u sum|x|): at n = 2048 or 4096 that habit allows 5e-4 sum|x| / n, i.e. on a row whose mean is 100 sigma an error of
0.05 sigma in the mean -- an order of magnitude more than a one-pass variance loses there (about 1e-3 of |y|), so the fault this file is there to catch would pass.  The depth is fixed by the
code (lane partials in slot order, the DPP tree, the readlane sums) and zero slots add exactly, so it is a property of the kernel and not of a GPU result.
  LayerNorm statistics of a row, s = ceil(d / 256) live float4 slots per lane, D1 = 4 s + 6 additions on any path from an element to the sum (4 per slot,
  4 DPP levels, 2 readlane levels), D2 = D1 + 1 for the sum of squares (the square's own rounding):
    mean = s1 / d            dmean = 1.01 D1 u sum|x| / d + u |mean|
    a_k = x_k - mean         computed: (a_k - delta)(1 + e), |delta| <= dmean, |e| <= u.  sum_k (a_k - delta)^2 = q + d delta^2 EXACTLY (sum a_k = 0: two-pass
                             statistics have no cancellation term), so
    q = sum a_k^2            dq = d dmean^2 + 1.01 (D2 + 3) u (q + d dmean^2)                 (2u from a_k's rounding squared, D2 + 1 from product and sum)
    var = q / d              dvar = dq / d + u var
    rstd = rsqrt(var + eps)  drstd / rstd = 1.02 (dvar + u (var + eps)) / (2 (var + eps)) + 2u        (rsqrtf at one ulp = 2^-23; 1.02: second order)
  y = ((x - mean) rstd) g + b, one rounding per operation (the compiler contracts e g + b into one fma: fewer roundings, inside the same bound):
    d = x - mean: dd = dmean + u |d|;  e = d rstd: de = dd rstd + |d| rstd (drstd / rstd) + u |e|;  f = e g: df = de |g| + u |f|;  y = f + b: dy = df + u |y|
  A second norm over an input that is off by dx (skinny_ref.ln_stage): the first derivative of the LayerNorm times 1.02,
    rstd |g| (dx_k + mean_j dx_j) + |g| |x_k - mean| rstd^3 mean_j (|x_j - mean| dx_j),
  plus its own terms with every magnitude taken over |x| + dx.
  GroupNorm chunk statistics (k_gn_stats: 8 values per thread in order, the wave tree of 6 levels, 4 wave partials in order: D1 = 8 + 6 + 3 = 17, D2 = 18),
  n values per chunk:  count exact;  dmean_c = 1.01 D1 u sum|x| / n + u |mean_c|;  dM2_c = n dmean_c^2 + 1.01 (D2 + 3) u (M2_c + n dmean_c^2)   (as above).
  The merge (gn_merge_loaded: a lane's 8 chunks in order, 3 DPP levels: depth 11), N = sum n_c exact (integers below 2^24):
    W = sum n_c mean_c       dW = sum n_c dmean_c + 1.01 * 11 u sum n_c (|mean_c| + dmean_c)                         (fma: one rounding per term)
    mean = W / N             dmean = dW / N + u |mean|
    d_c = mean_c - mean      dd_c = dmean_c + dmean + u |d_c|
    t_c = M2_c + n_c d_c^2   dt_c = dM2_c + n_c (2 |d_c| dd_c + dd_c^2) + 1.01 * 3 u (M2_c + n_c (|d_c| + dd_c)^2)           (n d, the fma, the accumulate)
    M2 = sum t_c             dM2 = sum dt_c + 1.01 * 11 u sum (t_c + dt_c)
    var = M2 / N             dvar = dM2 / N + u var;   drstd / rstd as for the LayerNorm
  The fold y = x A + D (gn_fold_coef / gn_fold_apply, contraction as written there), S = 1 + scale (one rounding; exactly 1 without modulation):
    A = (rstd gamma) S                 dA = 1.01 |A| (drstd / rstd + 3u)
    p = (mean rstd) gamma              dp = 1.01 (|p| (drstd / rstd + 2u) + dmean rstd |gamma|)
    c = beta - p                       dc = dp + u |c|
    D = fma(c, S, shift)               dD = dc |S| + u |c S| + u |D|
    y = fma(x, A, D)                   dy = |x| dA + dD + u |y|              (every term absolute: the cancellation between x A and D is covered)
  SiLU          2e-6 |y| + 1.01 |f'(y)| dy           the activation's own error on top of the propagated one (test_gpu_gemm_forms.py's constant)
  output        uT (|v| + tol) + 2^-25 (f16), uT = 2^-8 (bf16), 2^-11 (f16); fp8-e4m3: 2^-4 (|v| + tol) with the subnormal floor 2^-10; |v| + tol < 448 everywhere
  padding rows of a ragged batch owe exact zeros.
No term is fitted to a GPU result.  Two-pass statistics leave no row without a bound: drstd / rstd stays far below the 1 / 4 at which the first-order model would
end, and test_norm_ref.py asserts that every bound of every case is finite and positive.

OPERANDS (seeded CPU generator).  LayerNorm rows cycle through three kinds: N(0, 1)-like; a large common offset (mean = 100 sigma: a one-pass variance fails);
tiny variance (sigma^2 = 1e-5, the order of eps: eps itself is visible).  GroupNorm inputs drift along T (a ramp of +-4 sigma) with an offset per group, so that
chunk means differ by several sigma and the between-chunk term of the merge dominates.  gamma, beta, scale and shift keep away from 0 and 1.

THE EMULATION follows the code: lane `l` owns the float4 slots l + 64 i, lane partials in slot order, the wave sum as its pairwise tree (the DPP steps and the
readlane sums add neighbours, pairs, quads ... : a balanced tree in lane order), k_gn_stats' four wave partials in order, the merge's 8 lanes per group taking
chunks sub + 8 i, the fold with its written fmaf contraction.  Where the source leaves contraction to the compiler the emulation follows the gfx950 machine
code: k_layernorm's squares are plain products and its e g + b one fma, k_gn_stats' d d + sq is one fma (either choice lies inside the bound, which counts one
rounding per written operation).  Faults are switched on by name (LN_FAULTS, GN_FAULTS).
"""
import functools
import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from skinny_ref import frag_index, from_frag

U = 2.0 ** -24
EPS = 1e-5
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f8": torch.float8_e4m3fn}
# output kinds: name -> (dtype code, out_f32, out_f8, element type of the buffer, type the value is rounded to)
OUT_KINDS = {"f32": (0, 0, 0, "f32", "f32"), "bf16": (1, 0, 0, "bf16", "bf16"), "f16": (4, 0, 0, "f16", "f16"), "f8": (1, 0, 1, "f8", "f8"),
			 "bf16-f32out": (1, 1, 0, "f32", "f32")}
CANARY_ROWS = 3
RING_SLOTS, RING_SLOT = 4, 2


def out_rounding(v, tol, kind):
	"""half an output ulp at the largest value the bound admits"""
	t = OUT_KINDS[kind][4]
	if t == "f32":
		return torch.zeros_like(tol)
	if t == "f8":
		return (2.0 ** -4 * (v.abs() + tol)).clamp_min(2.0 ** -10)
	return {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[t] * (v.abs() + tol) + (2.0 ** -25 if t == "f16" else 0.0)


def out_key(kind):
	"""the group a ratio is reported under: an f32 result shows the arithmetic, a rounded one mostly its own half ulp"""
	return "f32" if OUT_KINDS[kind][4] == "f32" else "rounded"


def to_out_type(v, kind):
	"""an f32 result as the kernel stores it, read back as f64"""
	return v.float().to(TDT[OUT_KINDS[kind][4]]).double()


def away(gen, n, lo, hi, signed=True):
	"""n values with magnitude in [lo, hi] and a random sign: nowhere near 0, and (with lo, hi chosen so) nowhere near 1"""
	m = lo + (hi - lo) * torch.rand(n, generator=gen)
	return m * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1) if signed else m


# =========================================================================================================== LayerNorm
@dataclass(frozen=True)
class LnCase:
	d: int
	rows: int
	ldx_extra: int = 0
	ldo_extra: int = 0
	norms: int = 1
	out: str = "f32"
	frag: int = 0
	out2: str = "none"             # none, direct, ring

	@property
	def id(self):
		return f"ln-d{self.d}-r{self.rows}-x{self.ldx_extra}-o{self.ldo_extra}-n{self.norms}-{self.out}-frag{self.frag}-{self.out2}"

	@property
	def ni(self):
		return 4 if self.d <= 1024 else 16

	@property
	def group(self):
		return f"layernorm-NI{self.ni}"

	@property
	def ldx(self):
		return self.d + self.ldx_extra

	@property
	def ldo(self):
		return self.d + self.ldo_extra

	@property
	def pad_rows(self):
		return (self.rows + 15) // 16 * 16

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())


LN_CASES = [
	# NI = 4 (d <= 1024): 64 leaves 48 lanes wholly idle, 192 sixteen, 768 fills 3 of 4 slots
	LnCase(64, 1), LnCase(64, 17, 8, 8, 2, "bf16", 0, "direct"),
	LnCase(192, 3, 8, 0, 1, "f16", 1), LnCase(192, 5, 0, 8, 2, "bf16-f32out", 0, "ring"),
	LnCase(768, 4, 0, 0, 1, "bf16", 1, "direct"), LnCase(768, 17, 8, 8, 2, "f32"),
	LnCase(1024, 5, 0, 0, 2, "bf16", 1, "ring"),                  # the decode step's launch: ln_f + final_norm, fragment order, the hidden ring
	LnCase(1024, 17, 0, 0, 2, "f16", 1, "ring"), LnCase(1024, 1, 8, 0, 1, "bf16-f32out", 1), LnCase(1024, 3, 0, 8, 1, "f16", 0, "direct"),
	LnCase(1024, 4, 0, 0, 2, "f32"),
	# NI = 16 (d > 1024): 1056 is one slot and 8 lanes past NI = 4's reach
	LnCase(1056, 1, 8, 8, 1, "f32"), LnCase(1056, 5, 0, 0, 2, "bf16", 1, "direct"), LnCase(1056, 3, 0, 8, 1, "f16", 0, "ring"),
	LnCase(2048, 5, 0, 0, 2, "bf16", 1, "ring"),                  # the decode step's launch at model_dim 2048
	LnCase(2048, 17, 8, 0, 2, "bf16-f32out"), LnCase(2048, 4, 0, 0, 1, "f16", 1),
	LnCase(4096, 3, 8, 0, 2, "f32", 0, "direct"), LnCase(4096, 17, 0, 8, 1, "bf16"), LnCase(4096, 1, 0, 0, 2, "f16", 1, "ring"),
	LnCase(4096, 4, 0, 0, 1, "bf16-f32out"),
]
assert len({c.id for c in LN_CASES}) == len(LN_CASES)


def ln_operands(c):
	"""x f32 [rows][d] (row r of kind (r + seed) % 3), g1, b1, g2, b2 f32 [d]"""
	g = torch.Generator().manual_seed(c.seed)
	x = torch.randn(c.rows, c.d, generator=g)
	for r in range(c.rows):
		kind = (r + c.seed) % 3
		if kind == 1:
			x[r] = x[r] * 0.5 + 50.0 * (1 if r % 2 else -1)            # mean = 100 sigma
		elif kind == 2:
			x[r] = x[r] * math.sqrt(1e-5) + 0.0625                     # sigma^2 = eps
	o = {"x": x, "g1": away(g, c.d, 1.4, 2.2), "b1": away(g, c.d, 0.3, 0.8)}
	if c.norms == 2:
		o["g2"], o["b2"] = away(g, c.d, 1.3, 2.0), away(g, c.d, 0.25, 0.7)
	return o


def ln_stage(x, dx, g, b):
	"""y = LN(x) g + b in f64 and the bound dy on k_layernorm's f32 evaluation of it when its input is off by dx"""
	d = x.shape[1]
	D1 = 4 * ((d + 255) // 256) + 6
	D2 = D1 + 1
	mean = x.mean(1, keepdim=True)
	a = x - mean
	var = (a * a).mean(1, keepdim=True)
	rstd = 1 / torch.sqrt(var + EPS)
	dmean = 1.01 * D1 * U * (x.abs() + dx).sum(1, keepdim=True) / d + U * mean.abs()
	aa = a.abs() + dx + dx.mean(1, keepdim=True)                     # |x - mean| of the perturbed row
	q = (aa * aa).sum(1, keepdim=True)
	dq = d * dmean ** 2 + 1.01 * (D2 + 3) * U * (q + d * dmean ** 2)
	dvar = dq / d + U * q / d
	drel = 1.02 * (dvar + U * (var + EPS)) / (2 * (var + EPS)) + 2 * U
	y = a * rstd * g + b
	prop = rstd * g.abs() * (dx + dx.mean(1, keepdim=True)) + g.abs() * a.abs() * rstd ** 3 * (a.abs() * dx).mean(1, keepdim=True)
	dd = dmean + U * aa
	e = aa * rstd
	de = dd * rstd + e * drel + U * e
	df = de * g.abs() + U * e * g.abs()
	return y, 1.02 * prop + df + U * y.abs(), drel


@functools.lru_cache(maxsize=8)
def ln_reference(c):
	"""(operands, y f64 [rows][d], tol of the f32 result, tol of `out`)"""
	o = ln_operands(c)
	x = o["x"].double()
	y, dy, drel = ln_stage(x, torch.zeros_like(x), o["g1"].double(), o["b1"].double())
	if c.norms == 2:
		y, dy, drel2 = ln_stage(y, dy, o["g2"].double(), o["b2"].double())
		drel = torch.maximum(drel, drel2)
	assert float(drel.max()) < 0.25
	return o, y, dy, dy + out_rounding(y, dy, c.out)


def ln_blank(c):
	"""the images a launch writes into, logical [row][col], all NaN: out (fragment order: every row of the 16-row tiles; row-major: canary rows behind, ldo columns)
	and out2 (direct: canary rows behind; ring: RING_SLOTS slots of rows + CANARY_ROWS rows)"""
	nan = float("nan")
	b = {"out": torch.full((c.pad_rows, c.d) if c.frag else (c.rows + CANARY_ROWS, c.ldo), nan, dtype=torch.float64)}
	if c.out2 == "direct":
		b["out2"] = torch.full((c.rows + CANARY_ROWS, c.d), nan, dtype=torch.float64)
	elif c.out2 == "ring":
		b["out2"] = torch.full((RING_SLOTS, c.rows + CANARY_ROWS, c.d), nan, dtype=torch.float64)
	return b


def ln_check(c, got):
	"""worst |got - ref| / tol over what the launch owes, {"f32": the f32 results, "rounded": the 16-bit ones}; AssertionError when an owed value is not finite or
	anything else was written"""
	_, y, dy32, dyo = ln_reference(c)
	worst = {}

	def owed(name, g, tol, key="f32"):
		assert torch.isfinite(g).all(), f"{c.id}: {name} holds non-finite values where the launch owes a result"
		worst[key] = max(worst.get(key, 0.0), float(((g - y).abs() / tol).max()))

	def untouched(name, g):
		assert torch.isnan(g).all(), f"{c.id}: {name} was written where the launch owes nothing ({int((~torch.isnan(g)).sum())} elements)"

	out = got["out"]
	owed("out", out[:c.rows, :c.d], dyo, out_key(c.out))
	untouched("out behind the rows", out[c.rows:])
	untouched("out behind the columns", out[:c.rows, c.d:])
	if c.out2 == "direct":
		owed("out2", got["out2"][:c.rows], dy32)
		untouched("out2 behind the rows", got["out2"][c.rows:])
	elif c.out2 == "ring":
		ring = got["out2"].clone()
		owed("out2 ring slot", ring[RING_SLOT, :c.rows], dy32)
		ring[RING_SLOT, :c.rows] = float("nan")
		untouched("out2 ring outside the slot", ring)
	return worst


LN_FAULTS = ("one_pass_variance", "idle_slots_in_sum_of_squares", "padded_lane_count", "eps_1e-6", "second_norm_reuses_statistics", "second_norm_on_input",
			 "frag_row_and_kgroup_swapped")


def ln_fault_applies(c, fault):
	return {"one_pass_variance": True, "idle_slots_in_sum_of_squares": c.d % 256 != 0, "padded_lane_count": c.d % 256 != 0, "eps_1e-6": True,
			"second_norm_reuses_statistics": c.norms == 2, "second_norm_on_input": c.norms == 2, "frag_row_and_kgroup_swapped": bool(c.frag)}[fault]


def _tree_sum(v):
	"""the wave sum (and the merge's 3 DPP steps): pairwise tree over the last dimension, a power of two"""
	while v.shape[-1] > 1:
		v = v[..., 0::2] + v[..., 1::2]
	return v[..., 0]


def _fma(a, b, c):
	"""one rounding (a b is exact in f64; the f64 sum's own rounding is 2^-29 of an f32 ulp)"""
	return (a.double() * b.double() + c.double()).float()


def _rsqrt(v):
	return (1 / torch.sqrt(v.double())).float()


def _ln_pass(v, live, d, g, b, fault, stats=None):
	"""one pass of k_layernorm over the lane image v [rows][NI][64][4] (slot i of lane l = float4 chunk l + 64 i; idle slots hold zeros)"""
	rows, ni = v.shape[0], v.shape[1]
	s = torch.zeros(rows, 64, dtype=torch.float32)
	for i in range(ni):
		s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
	dn = torch.tensor(float(d if fault != "padded_lane_count" else (d + 255) // 256 * 256), dtype=torch.float32)
	mean = (_tree_sum(s) / dn)[:, None, None, None]
	sq = torch.zeros(rows, 64, dtype=torch.float32)
	for i in range(ni):
		if fault == "one_pass_variance":
			a = v[:, i]
		else:
			a = v[:, i] - mean[:, 0]
			if fault != "idle_slots_in_sum_of_squares":
				a = torch.where(live[None, i], a, torch.zeros_like(a))
		a = a * a      # (packed multiplies in the machine code: the squares are not contracted into the sums)
		sq = sq + (((a[..., 0] + a[..., 1]) + a[..., 2]) + a[..., 3])
	var = _tree_sum(sq) / dn
	if fault == "one_pass_variance":
		var = var - mean[:, 0, 0, 0] * mean[:, 0, 0, 0]
	eps = torch.tensor(1e-6 if fault == "eps_1e-6" else EPS, dtype=torch.float32)
	rstd = _rsqrt(var + eps)[:, None, None, None]
	if stats is not None:
		mean, rstd = stats
	y = _fma((v - mean) * rstd, g, b)
	return torch.where(live[None], y, torch.zeros_like(y)), (mean, rstd)


def ln_emulate(c, fault=None):
	"""the images of one launch (ln_blank's layout) computed the way k_layernorm computes them"""
	o = ln_operands(c)
	ni, d, rows = c.ni, c.d, c.rows

	def lanes(t):      # [.., d] -> [.., NI][64][4], zeros in idle slots
		p = torch.zeros(*t.shape[:-1], ni * 256, dtype=torch.float32)
		p[..., :d] = t
		return p.reshape(*t.shape[:-1], ni, 64, 4)

	live = lanes(torch.ones(d)).bool()
	x = lanes(o["x"])
	y, st = _ln_pass(x, live, d, lanes(o["g1"]), lanes(o["b1"]), fault)
	if c.norms == 2:
		y, _ = _ln_pass(x if fault == "second_norm_on_input" else y, live, d, lanes(o["g2"]), lanes(o["b2"]), fault,
						st if fault == "second_norm_reuses_statistics" else None)
	y = y.reshape(rows, -1)[:, :d]
	img = ln_blank(c)
	yo = to_out_type(y, c.out)
	if c.frag:
		flat = torch.full((c.pad_rows * d,), float("nan"), dtype=torch.float64)
		r, col = torch.meshgrid(torch.arange(rows), torch.arange(d), indexing="ij")
		if fault == "frag_row_and_kgroup_swapped":
			idx = (((r // 16) * (d // 32) + col // 32) * 64 + (r % 16) * 4 + (col // 8) % 4) * 8 + col % 8
		else:
			idx = frag_index(r, col, d // 32)
		flat[idx] = yo
		img["out"] = from_frag(flat, c.pad_rows, d)
	else:
		img["out"][:rows, :d] = yo
	if c.out2 == "direct":
		img["out2"][:rows] = y.double()
	elif c.out2 == "ring":
		img["out2"][RING_SLOT, :rows] = y.double()
	return img


# =========================================================================================================== GroupNorm32
GN_MODS = {"plain": (False, False), "mod-shared": (True, False), "mod-per-batch": (True, True)}      # name -> (has scale / shift, one row per batch element)


@dataclass(frozen=True)
class GnCase:
	C: int
	nb: int
	T: int
	what: str                                  # the chunk structure the case is there for
	tlen: Optional[Tuple[int, ...]] = None
	Tout: int = 0                              # != 0: row_idx, nearest-neighbour gather to Tout rows
	variants: Tuple[Tuple[str, str, int], ...] = ()      # (output kind, modulation, act)

	@property
	def id(self):
		return f"gn-C{self.C}-nb{self.nb}-T{self.T}" + (f"-tlen{'_'.join(map(str, self.tlen))}" if self.tlen else "") + (f"-to{self.Tout}" if self.Tout else "")

	@property
	def group(self):
		return f"groupnorm-C{self.C}"

	@property
	def chunk_rows(self):
		return 65536 // self.C

	@property
	def nchunks(self):
		return (self.T + self.chunk_rows - 1) // self.chunk_rows

	@property
	def rows_out(self):
		return self.Tout or self.T

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())

	def lens(self):
		return list(self.tlen) if self.tlen else [self.T] * self.nb

	def row_idx(self):
		"""F.interpolate(mode="nearest") from T to Tout rows: floor(to * T / Tout)"""
		return (torch.arange(self.Tout) * self.T // self.Tout).to(torch.int32) if self.Tout else None


def _gn_cases():
	kinds = list(OUT_KINDS)
	mods = list(GN_MODS)
	cs = []

	def add(C, nb, T, what, **kw):
		i = len(cs)      # two variants per case, walking through output kinds x modulation x activation
		v = ((kinds[i % 5], mods[i % 3], 2 * (i % 2)), (kinds[(i + 2) % 5], mods[(i + 1) % 3], 2 * ((i + 1) % 2)))
		cs.append(GnCase(C, nb, T, what, variants=v, **kw))

	for C in (128, 256, 512, 1024):
		R = 65536 // C
		add(C, 3, R // 2 + 3, "one partial chunk")
		add(C, 1, R, "exactly one chunk")
		add(C, 3, R + 1, "one chunk and one row")
		add(C, 1, 9 * R + 1, "more than 8 chunks, the last of one row")            # C = 128: T = 4609
		add(C, 1, 25 * R + 1, "more than 24 chunks")                               # C = 1024: T = 1601
		add(C, 3, 2 * R + 5, "ragged: full, ending on a chunk edge, one row", tlen=(2 * R + 5, R, 1))
		add(C, 3, R + 1, "row_idx, Tout > T", Tout=2 * R + 5)
		add(C, 1, R + 9, "row_idx, Tout < T", Tout=R // 2 + 1)
	add(1024, 1, 64 * 64, "the limit of 64 chunks")
	assert len({c.id for c in cs}) == len(cs)
	return cs


GN_CASES = _gn_cases()
GROUPS = sorted({c.group for c in LN_CASES} | {c.group for c in GN_CASES})


def gn_operands(c):
	"""x f32 [nb][T][C] with a ramp along T and an offset per group; gamma, beta f32 [C]; mod f32 [nb][2 C], rows of [scale | shift]"""
	g = torch.Generator().manual_seed(c.seed)
	ramp = torch.linspace(-4.0, 4.0, c.T)[None, :, None] if c.T > 1 else torch.zeros(1, 1, 1)
	goff = ((torch.arange(c.C) // (c.C // 32)) % 5 - 2).float() * 0.7
	x = torch.randn(c.nb, c.T, c.C, generator=g) + ramp * (1 + 0.25 * torch.arange(c.nb).float())[:, None, None] + goff
	mod = torch.cat([away(g, c.nb * c.C, 0.3, 0.8, signed=False).view(c.nb, c.C), away(g, c.nb * c.C, 0.3, 0.8).view(c.nb, c.C)], 1)
	return {"x": x, "gamma": away(g, c.C, 1.4, 2.2), "beta": away(g, c.C, 0.3, 0.8), "mod": mod.contiguous()}


def silu(y):
	s = torch.sigmoid(y)
	return y * s, s * (1 + y * (1 - s))


@functools.lru_cache(maxsize=2)
def gn_statistics(c):
	"""(operands, dict of f64 tensors): per chunk [nb][32][nchunks] cnt, mean, m2, dmean, dm2, valid; per group [nb][32] mean, rstd, dmean, drel"""
	o = gn_operands(c)
	x = o["x"].double()
	R, nch, cpg = c.chunk_rows, c.nchunks, c.C // 32
	z = lambda: torch.zeros(c.nb, 32, nch, dtype=torch.float64)
	cnt, mean, m2, sabs = z(), z(), z(), z()
	for b, Tl in enumerate(c.lens()):
		for ch in range((Tl + R - 1) // R):
			blk = x[b, ch * R:min(Tl, ch * R + R)].reshape(-1, 32, cpg).permute(1, 0, 2).reshape(32, -1)
			cnt[b, :, ch] = blk.shape[1]
			mean[b, :, ch] = blk.mean(1)
			m2[b, :, ch] = ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1)
			sabs[b, :, ch] = blk.abs().sum(1)
	valid = cnt > 0
	n = cnt.clamp_min(1)
	D1, D2 = 17, 18
	dmean = 1.01 * D1 * U * sabs / n + U * mean.abs()
	dm2 = n * dmean ** 2 + 1.01 * (D2 + 3) * U * (m2 + n * dmean ** 2)
	# the merge
	N = cnt.sum(2)
	W = (cnt * mean).sum(2)
	dW = (cnt * dmean).sum(2) + 1.01 * 11 * U * (cnt * (mean.abs() + dmean)).sum(2)
	gmean = W / N
	dgmean = dW / N + U * gmean.abs()
	dc = (mean - gmean[..., None]).abs()
	ddc = dmean + dgmean[..., None] + U * dc
	t = m2 + cnt * dc ** 2
	dt = dm2 + cnt * (2 * dc * ddc + ddc ** 2) + 1.01 * 3 * U * (m2 + cnt * (dc + ddc) ** 2)
	M2 = t.sum(2)
	dM2 = (dt * valid).sum(2) + 1.01 * 11 * U * ((t + dt) * valid).sum(2)
	var = M2 / N
	dvar = dM2 / N + U * var
	drel = 1.02 * (dvar + U * (var + EPS)) / (2 * (var + EPS)) + 2 * U
	assert float(drel.max()) < 0.25
	return o, {"cnt": cnt, "mean": mean, "m2": m2, "dmean": dmean, "dm2": dm2, "valid": valid, "gmean": gmean, "rstd": 1 / torch.sqrt(var + EPS), "dgmean": dgmean,
			   "drel": drel}


def gn_reference(c, variant):
	"""(out f64 [nb][rows_out][C], tol) for one (output kind, modulation, act); padding rows: value 0, tol 0"""
	kind, mod, act = variant
	o, st = gn_statistics(c)
	x = o["x"].double()
	cpg = c.C // 32
	per_c = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]                  # [nb][32] -> [nb][1][C]
	mean, rstd, dmean, drel = per_c(st["gmean"]), per_c(st["rstd"]), per_c(st["dgmean"]), per_c(st["drel"])
	gamma, beta = o["gamma"].double()[None, None], o["beta"].double()[None, None]
	has, per_b = GN_MODS[mod]
	if has:
		m = o["mod"].double() if per_b else o["mod"].double()[:1].expand(c.nb, -1)
		S, shift, us = 1 + m[:, None, :c.C], m[:, None, c.C:], U
	else:
		S, shift, us = torch.ones(1, 1, 1, dtype=torch.float64), torch.zeros(1, 1, 1, dtype=torch.float64), 0.0
	A = rstd * gamma * S
	dA = 1.01 * A.abs() * (drel + 2 * U + us)
	p = mean * rstd * gamma
	dp = 1.01 * (p.abs() * (drel + 2 * U) + dmean * rstd * gamma.abs())
	cc = beta - p
	dcc = dp + U * cc.abs()
	D = cc * S + shift
	dD = dcc * S.abs() + (us + U) * (cc * S).abs() + U * D.abs()
	y = x * A + D
	dy = x.abs() * dA + dD + U * y.abs()
	if act == 2:
		f, df = silu(y)
		dy = 2e-6 * y.abs() + 1.01 * df.abs() * dy
		y = f
	if c.Tout:
		idx = c.row_idx().long()
		y, dy = y[:, idx], dy[:, idx]
	tol = dy + out_rounding(y, dy, kind)
	for b, Tl in enumerate(c.tlen or ()):
		y[b, Tl:] = 0
		tol[b, Tl:] = 0
	return y, tol


def gn_check(c, variant, out, ms, ref=None):
	"""out f64 [nb][rows_out][C], ms f64 [nb][32][nchunks][3] as read back (the canary elements behind both are the caller's to look at): worst ratios {"f32" or "rounded", "mean", "m2"}; AssertionError on a canary"""
	_, st = gn_statistics(c)
	y, tol = ref if ref is not None else gn_reference(c, variant)
	what = f"{c.id} {variant}"
	got = out
	assert torch.isfinite(got).all(), f"{what}: non-finite values where the launch owes a result"
	live = tol > 0
	assert not got[~live].any(), f"{what}: padding rows of a ragged batch are not zero"
	w = {out_key(kind := variant[0]): float(((got - y).abs()[live] / tol[live]).max())}
	valid = st["valid"]
	assert torch.isnan(ms[~valid]).all(), f"{what}: a statistics triple past a sequence's end was written"
	assert torch.isfinite(ms[valid]).all(), f"{what}: a statistics triple the launch owes is not finite"
	assert torch.equal(ms[..., 0][valid], st["cnt"][valid]), f"{what}: chunk counts are not rows * C / 32"
	w["mean"] = float(((ms[..., 1] - st["mean"]).abs()[valid] / st["dmean"][valid]).max())
	w["m2"] = float(((ms[..., 2] - st["m2"]).abs()[valid] / st["dm2"][valid]).max())
	return w


GN_FAULTS = ("last_chunk_counted_full", "merge_without_between_chunk_term", "merge_reads_nchunks", "group_index_of_C1024", "row_idx_ignored", "scale_for_1_plus_scale",
			 "silu_before_modulation", "padding_rows_not_zeroed")


def gn_fault_applies(c, variant, fault):
	kind, mod, act = variant
	R = c.chunk_rows
	return {"last_chunk_counted_full": any(Tl % R for Tl in c.lens()), "merge_without_between_chunk_term": c.nchunks > 1,
			"merge_reads_nchunks": c.tlen is not None and any((Tl + R - 1) // R < c.nchunks for Tl in c.tlen), "group_index_of_C1024": c.C != 1024,
			"row_idx_ignored": bool(c.Tout), "scale_for_1_plus_scale": GN_MODS[mod][0], "silu_before_modulation": GN_MODS[mod][0] and act == 2,
			"padding_rows_not_zeroed": c.tlen is not None and any(Tl < c.T for Tl in c.tlen)}[fault]


def gn_emulate_stats(c, o, fault=None):
	"""k_gn_stats: the ms image f32 [nb][32][nchunks][3], NaN where nothing is written"""
	R, nch, cpg = c.chunk_rows, c.nchunks, c.C // 32
	ms = torch.full((c.nb, 32, nch, 3), float("nan"), dtype=torch.float32)
	for b, Tl in enumerate(c.lens()):
		for ch in range((Tl + R - 1) // R):
			blk = o["x"][b, ch * R:min(Tl, ch * R + R)].reshape(-1, 32, cpg).permute(1, 0, 2).reshape(32, -1)      # element e = t * cpg + c
			n = blk.shape[1]
			v = torch.zeros(32, 2048, dtype=torch.float32)
			v[:, :n] = blk
			v = v.reshape(32, 8, 256)                                        # thread tid holds e = tid + 256 i
			live = (torch.arange(2048) < n).reshape(8, 256)
			s = torch.zeros(32, 256, dtype=torch.float32)
			for i in range(8):
				s = s + v[:, i]
			wp = _tree_sum(s.reshape(32, 4, 64))
			nn = torch.tensor(float(R * cpg if fault == "last_chunk_counted_full" else n), dtype=torch.float32)
			mean = (((wp[:, 0] + wp[:, 1]) + wp[:, 2]) + wp[:, 3]) / nn
			sq = torch.zeros(32, 256, dtype=torch.float32)
			for i in range(8):
				dd = torch.where(live[i][None], v[:, i] - mean[:, None], torch.zeros(1))
				sq = _fma(dd, dd, sq)
			wq = _tree_sum(sq.reshape(32, 4, 64))
			ms[b, :, ch, 0], ms[b, :, ch, 1], ms[b, :, ch, 2] = nn, mean, ((wq[:, 0] + wq[:, 1]) + wq[:, 2]) + wq[:, 3]
	return ms


def gn_emulate_merge(c, ms, fault=None):
	"""gn_merge_loaded for every (b, group): mean, rstd f32 [nb][32]"""
	R, nch = c.chunk_rows, c.nchunks
	tri = torch.zeros(c.nb, 32, 64, 3, dtype=torch.float32)
	for b, Tl in enumerate(c.lens()):
		k = nch if (fault == "merge_reads_nchunks" or c.tlen is None) else (Tl + R - 1) // R
		tri[b, :, :k] = ms[b, :, :k]
	tri = tri.reshape(c.nb, 32, 8, 8, 3)                                     # chunk k = sub + 8 i -> [i][sub]
	cn, cm, c2 = tri[..., 0], tri[..., 1], tri[..., 2]
	nt = torch.zeros(c.nb, 32, 8, dtype=torch.float32)
	ws = torch.zeros(c.nb, 32, 8, dtype=torch.float32)
	for i in range(8):
		nt = nt + cn[:, :, i]
		ws = _fma(cn[:, :, i], cm[:, :, i], ws)
	nt, ws = _tree_sum(nt), _tree_sum(ws)
	mean = ws / nt
	m2 = torch.zeros(c.nb, 32, 8, dtype=torch.float32)
	for i in range(8):
		d = cm[:, :, i] - mean[..., None]
		m2 = m2 + (c2[:, :, i] if fault == "merge_without_between_chunk_term" else _fma(cn[:, :, i] * d, d, c2[:, :, i]))
	return mean, _rsqrt(_tree_sum(m2) / nt + torch.tensor(EPS, dtype=torch.float32))


def gn_emulate(c, variant, fault=None, stats=None):
	"""(out image f64 [nb][rows_out][C], ms image f64) of one ttk_gn_apply call with stats = 1, the way k_gn_stats and k_gn_apply compute them"""
	kind, mod, act = variant
	o = gn_operands(c) if stats is None else stats[0]
	ms = gn_emulate_stats(c, o, fault) if stats is None else stats[1]
	mean, rstd = gn_emulate_merge(c, ms, fault)
	cpg = c.C // 32
	grp = torch.arange(c.C) // (32 if fault == "group_index_of_C1024" else cpg)
	mean, rstd = mean[:, grp][:, None], rstd[:, grp][:, None]                   # [nb][1][C]
	gamma, beta = o["gamma"][None, None], o["beta"][None, None]
	has, per_b = GN_MODS[mod]
	if has:
		m = o["mod"] if per_b else o["mod"][:1].expand(c.nb, -1)
		sc, sh = m[:, None, :c.C], m[:, None, c.C:]
	else:
		sc = sh = torch.zeros(1, 1, 1)
	sil = lambda t: t * (1 / (1 + torch.exp(-t)))
	x = o["x"]
	if c.Tout:
		idx = c.row_idx().long() if fault != "row_idx_ignored" else torch.arange(c.Tout).clamp_max(c.T - 1)
		x = x[:, idx]
	if fault == "silu_before_modulation":
		y = _fma(x, rstd * gamma, beta - mean * rstd * gamma)
		y = _fma(sil(y) if act == 2 else y, 1 + sc, sh)
	else:
		s1 = sc if fault == "scale_for_1_plus_scale" else 1 + sc
		y = _fma(x, rstd * gamma * s1, _fma(beta - mean * rstd * gamma, s1, sh))
		if act == 2:
			y = sil(y)
	if fault != "padding_rows_not_zeroed":
		for b, Tl in enumerate(c.tlen or ()):
			y[b, Tl:] = 0
	return to_out_type(y, kind), ms.double()
