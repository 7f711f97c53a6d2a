"""Float64 reference of the weight-streaming decode launches (csrc/skinny.hip: k_skinny, csrc/gemv.hip: k_gemv), written from the definition over the
kernels' own operands, with a derived per-element error bound, the operands and case lists that tests/test_skinny_ref.py (CPU) and
tests/test_gpu_skinny_forms.py (GPU, through ttk_gemv_launch) share, and a float32 emulation of both kernels' arithmetic with switchable faults that
shows the bound and the canaries can see them.

One launch computes, for rows m < M and columns n < N,
    z[m][n] = sum_k A[m][k] W[n][k] + b[n]
with A one of
    plain      the rows `a` as given (T-typed, fragment order);
    fold       LN(x) with the LayerNorm folded into the matrix: W' = gamma o W, csum[n] = sum_k W'[n][k], b' = b + beta W, and on the T-typed
               un-normalised rows x the identity the kernel uses:  z = rstd (x W'^T - mean csum) + b',  mean / var over the K channels, eps 1e-5;
    prologue   LN(x; g1, b1), optionally LN(.; g2, b2) on top, of f32 rows x, rounded to T before the product;
and an epilogue per role
    head       out_f32 = z                      (+ noise and the position bump, which are not arithmetic)
    proj       out_f32 = res + z, out_T = T(res + z)
    fc         out_T = T(gelu_new(z))            (HF: 0.5 z (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3))))
    qkv        qbuf = 0.125 z[:, :d];  kcache / vcache row d_pos[0] = T(z[:, d:2d]) / T(z[:, 2d:]) when d_pos[0] < max_ctx.

Operands are on the bf16 grid (|x| >= 2^-10 or 0) times powers of two, so they are exact in every kernel type and every product a w is exact in f32; the
fold's gamma is a power of two, so gamma o W is exact in T as well; fp8 matrices are rounded by ttk_fp8_round_weights' definition restated below (the
smallest power-of-two scale >= absmax / 448, e4m3 round to nearest even), so the reference multiplies what the kernel multiplies.

THE BOUND, per element.  u = 2^-24; S = sum_k |A_k| |W_nk| over the operands the MFMA sees; uT = 2^-8 (bf16), 2^-11 (f16), 0 (f32).
  product     1e-5 S                               f32 accumulation of a K-term MFMA dot product, the cross-wave sum included (test_gpu_gemm_forms.py's constant)
  bias        u |z|                                one rounding; wscale is a power of two: exact
  residual    u |res + z|
  q           u |q|                                the product with 0.125 is exact; kept as the one rounding the issue allots per epilogue operation
  gelu_new    2e-6 |z| + 1.01 |f'(z)| dz           the activation's own error on top of the propagated pre-activation error dz (test_gpu_gemm_forms.py)
  T output    uT (|v| + tol) + 2^-25 (f16)         half an output ulp at the largest value the bound admits, f16's subnormal floor (attn_ref.py)
Row statistics (fold: over the T-typed row; prologue: over the f32 row or the first norm's f32 output).  s1 = sum x, s2 = sum x^2 (x^2 exact in f32):
  ds1 = 2 K u sum|x|,  ds2 = 2 K u sum x^2         twice the worst-case summation bound: any order, and the v_dot2 forms whose inner rounding is undocumented
  mean = s1 / K                                    dmean = ds1 / K + u |mean|
  m2 = s2 / K                                      dm2 = ds2 / K + u m2
  var = max(m2 - mean^2, 0)                        dvar = dm2 + 2 |mean| dmean + u mean^2 + u |m2 - mean^2|     (the cancellation: dm2 and dmean are absolute)
  rstd = rsqrt(var + 1e-5)                         drstd / rstd = 1.02 (dvar + u (var + eps)) / (2 (var + eps)) + 2u     (rsqrtf at one ulp = 2^-23; 1.02: second order)
Fold epilogue, t = acc - mean csum, v = t rstd + b':
  dt = 1e-5 S + dmean |csum| + 2u |mean csum| + u |t|     csum is the f32 rounding of an f64 sum (u |csum|), the product, the difference
  dv = dt rstd + |t| rstd (drstd / rstd) + u |t rstd| + u |b'| + u |v|                                    b' is the f32 rounding of an f64 sum
Prologue, y = (x - mean) rstd g + b, one rounding per operation, with an input error dx (zero for the first norm, the first norm's dy for the second):
  propagated  rstd |g| (dx_k + mean_j dx_j) + |g| |x_k - mean| rstd^3 mean_j(|x_j - mean| dx_j)           first derivative of the LayerNorm, times 1.02
  own         d = x - mean: dmean + u |d|;  e = d rstd: dd rstd + |d| rstd (drstd / rstd) + u |e|;  f = e g: de |g| + u |f|;  y = f + b: df + u |y|
  the statistics of a second norm are taken over |x| + dx.  Then the rounding of y to T before the MFMA: dy += uT (|y| + dy) + 2^-25 (f16), and
  dz = sum_k dy_k |W_nk| + 1e-5 sum_k (|y_k| + dy_k) |W_nk| + u |z|.
No term is fitted to a GPU result, and none had to grow for the emulation below to pass (test_skinny_ref.py prints its worst error / bound per group).
A row the fold cannot represent (the near-constant row of the "fold-unfit" cases: |mean| > 8 std, the variance below what E[x^2] - mean^2 resolves) makes
drstd / rstd large: above 1 / 4 the first-order model no longer holds and the row's bound is infinite -- the finiteness canary and the health word
are what is asserted on that row.

THE EMULATION follows the code: wave w multiplies k-steps [KS w / nw, KS (w + 1) / nw) in order, one f32 rounding per MFMA (f32 operands: per 16x16x4
instruction, k = {8 g + j}), the waves' tiles summed in wave order, the narrow tiles' column map under both block-id orders, the statistics in the
kernels' lane / wave order (k_gemv: dot2 pairs), the epilogues in f32.  Faults are switched on by name (FAULTS).
"""
import math
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

U = 2.0 ** -24
EPS = 1e-5
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
FLOOR = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25}
M_LIST = (1, 5, 16, 17, 33, 49, 64)
CANARY_ROWS = 3
ROLE = {"qkv": 0, "proj": 1, "fc": 2, "head": 3}
FORM = {"plain": 0, "fold": 1, "prologue": 2}
Q_SCALE = 0.125


def row_tiles(M):
	"""decode_row_tiles of csrc/ttk_kernels.h: the sixteen-row tiles a launch over M rows is instantiated for"""
	return 1 if M <= 16 else (2 if M <= 32 else (3 if M <= 48 else 4))


def frag_index(row, col, ksteps):
	"""A-fragment order [m_tile][k_step][lane = k_group * 16 + row][8] of a [rows][32 * ksteps] operand: a k-step is 32 columns, a lane holds 8 consecutive
	columns (its k-group) of one of the tile's 16 rows.  Works on ints and on integer tensors."""
	m_tile, r = row // 16, row % 16
	k_step, k_group, j = col // 32, (col // 8) % 4, col % 8
	return ((m_tile * ksteps + k_step) * 64 + k_group * 16 + r) * 8 + j


def to_frag(rows, pad_rows, fill=float("nan")):
	"""[M][K] -> flat fragment-order buffer of pad_rows rows, the padding rows holding `fill`"""
	M, K = rows.shape
	out = torch.full((pad_rows * K,), fill, dtype=rows.dtype)
	r, c = torch.meshgrid(torch.arange(M), torch.arange(K), indexing="ij")
	out[frag_index(r, c, K // 32)] = rows
	return out


def from_frag(flat, pad_rows, N):
	"""flat fragment-order buffer -> logical [pad_rows][N]"""
	r, c = torch.meshgrid(torch.arange(pad_rows), torch.arange(N), indexing="ij")
	return flat[frag_index(r, c, N // 32)]


def grid(t, mul=1.0):
	"""bf16 values without the tiny ones, times a power of two: exactly representable in bf16, f16 and f32"""
	t = t.bfloat16().float()
	return (torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t) * mul).double()


def fp8_round_weights(w):
	"""ttk_fp8_round_weights' definition: scale = the smallest power of two >= absmax / 448, w <- e4m3(w / scale) * scale (round to nearest even)"""
	amax = float(w.abs().max())
	if not (amax > 0) or not math.isfinite(amax):
		return w.clone(), 1.0
	fr, e = math.frexp(amax / 448.0)
	scale = math.ldexp(1.0, e - 1 if fr == 0.5 else e)
	return (w / scale).float().to(torch.float8_e4m3fn).double() * scale, scale


def half_ulp_T(v, tol, dt):
	return UT[dt] * (v.abs() + tol) + FLOOR[dt]


def gelu_new(z):
	c = math.sqrt(2.0 / math.pi)
	th = torch.tanh(c * (z + 0.044715 * z ** 3))
	return 0.5 * z * (1 + th), 0.5 * (1 + th) + 0.5 * z * (1 - th ** 2) * c * (1 + 3 * 0.044715 * z ** 2)


# ----------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
	id: str
	group: str
	dt: str
	role: str
	form: str
	N: int
	K: int
	w8: bool = False
	family: int = 1
	waves: int = 0                 # 0: the decode step's choice
	Ms: Tuple[int, ...] = M_LIST
	out_T: bool = True             # proj: also the T copy
	norms: int = 1
	max_ctx: int = 6
	pos: Tuple[int, ...] = (0,)
	noise: bool = False
	bump: bool = False
	special: str = ""              # nearconst: a row the fold cannot represent (health bit 0), whose f32 variance comes out negative without the clamp
	expect_family: int = 0         # what family 0 must give the bits of (0: not asserted)
	model_dim: int = 0             # the model's width where it is not N (proj) / K (the others): mlp.c_proj's N x 4N
	seed: int = 0

	@property
	def H(self):
		return self.K // 64

	@property
	def layout(self):
		return 0 if self.role == "head" else 1

	def ms(self):
		cap = 32 if self.dt == "f32" or (self.form == "prologue" and self.role != "head") else 64
		return tuple(m for m in self.Ms if m <= cap)

	@property
	def narrow(self):
		return self.role == "proj"


DTS = ("f32", "bf16", "f16")
CU_LDS_BYTES = 160 * 1024


def prologue_lds(dt, M, K, waves):
	"""skinny_lds_bytes of csrc/ttk_kernels.h for the LayerNorm-prologue form: 16 MT rows of K T-typed values, padded by 16 bytes, and the reduce area"""
	mt = row_tiles(M)
	return 16 * mt * (K * (4 if dt == "f32" else 2) + 16) + waves * mt * 64 * 4 * 4


def fitting_ms(dt, K, waves):
	return tuple(m for m in M_LIST if prologue_lds(dt, m, K, waves) <= CU_LDS_BYTES)


def _cases():
	cs = []
	add = cs.append
	for dt in DTS:
		# head, plain operand: N = 34 (the last of 3 tiles has 2 live columns); K picks the wave slices
		for K, waves in ((64, 0), (192, 0), (320, 0), (1024, 4), (1024, 16), (1088, 0), (2112, 0)):
			add(Case(f"head-{dt}-K{K}-w{waves}", "head", dt, "head", "plain", 34, K, waves=waves, family=1, bump=(K == 192)))
		add(Case(f"head-{dt}-K192-noise", "head", dt, "head", "plain", 34, 192, noise=True, bump=True, Ms=(5, 17, 33, 64)))
		add(Case(f"head-{dt}-N642-K64-bump", "head", dt, "head", "plain", 642, 64, bump=True, Ms=(5, 17)))      # 41 workgroups, one bump
		# residual: 4 / 12 tiles plain order, 8 / 16 tiles XCD order
		for N in (64, 192, 128, 256):
			for K in (64, 1088):
				add(Case(f"proj-{dt}-N{N}-K{K}", "narrow", dt, "proj", "plain", N, K, out_T=(N != 192 or K != 64)))
		add(Case(f"proj-{dt}-N128-K64-noT", "narrow", dt, "proj", "plain", 128, 64, out_T=False))
		# folded LayerNorm
		for N in (64, 256):
			add(Case(f"fold-fc-{dt}-N{N}-K64", "fold", dt, "fc", "fold", N, 64))
		add(Case(f"fold-qkv-{dt}-K64", "fold", dt, "qkv", "fold", 192, 64, pos=(0, 6, 5)))
		add(Case(f"fold-qkv-{dt}-K192", "fold", dt, "qkv", "fold", 576, 192, pos=(0, 6, 5)))
		add(Case(f"fold-qkv-{dt}-K1024", "fold", dt, "qkv", "fold", 3072, 1024, Ms=(17,), pos=(5,)))
		add(Case(f"fold-fc-{dt}-K1088-nearconst", "fold-unfit", dt, "fc", "fold", 64, 1088, Ms=(5,), special="nearconst"))
		# LayerNorm prologue
		for K in (64, 192, 1024, 1088, 2048):
			for waves in (4, 8):
				# every M of the list whose 16 MT normalised rows fit a compute unit's LDS (prologue_lds): at K = 2048 one m-tile in f32, two in 16-bit (more
				# than 64 KiB from M = 16 on, about 140 KiB at M = 17: the prefill head of a model_dim 2048 handle); ms() caps f32 and the roles but the head at 32
				add(Case(f"pro-fc-{dt}-K{K}-w{waves}", "prologue", dt, "fc", "prologue", 64, K, waves=waves, Ms=fitting_ms(dt, K, waves)))
				if waves == 4:
					add(Case(f"pro-head2-{dt}-K{K}", "prologue", dt, "head", "prologue", 34, K, norms=2, Ms=fitting_ms(dt, K, 4)))
		add(Case(f"pro-qkv-{dt}-K64", "prologue", dt, "qkv", "prologue", 192, 64, Ms=(5, 17), pos=(2,)))
		# k_gemv: every role at the geometry it is instantiated for
		add(Case(f"gemv-qkv-{dt}", "gemv", dt, "qkv", "fold", 3072, 1024, family=2, pos=(3,), expect_family=2))
		add(Case(f"gemv-proj-{dt}-K1024", "gemv", dt, "proj", "plain", 128, 1024, family=2, expect_family=2))
		add(Case(f"gemv-proj-{dt}-K4096", "gemv", dt, "proj", "plain", 128, 4096, family=2, expect_family=2, model_dim=1024))
		add(Case(f"gemv-fc-{dt}-N64", "gemv", dt, "fc", "fold", 64, 1024, family=2, expect_family=2))
		add(Case(f"gemv-fc-{dt}-N4096", "gemv", dt, "fc", "fold", 4096, 1024, family=2, expect_family=2))
		add(Case(f"gemv-head-{dt}", "gemv", dt, "head", "plain", 34, 1024, family=2, noise=True, bump=True, expect_family=2))
	# fp8 weights under bf16 arithmetic
	for N, K in ((64, 64), (128, 1088)):
		add(Case(f"proj-fp8-N{N}-K{K}", "narrow", "bf16", "proj", "plain", N, K, w8=True))
	add(Case("fold-fc-fp8-K192", "fold", "bf16", "fc", "fold", 64, 192, w8=True))
	add(Case("fold-qkv-fp8-K64", "fold", "bf16", "qkv", "fold", 192, 64, w8=True, pos=(1,)))
	for K in (64, 1088):
		add(Case(f"pro-fc-fp8-K{K}", "prologue", "bf16", "fc", "prologue", 64, K, w8=True, waves=8, Ms=(5, 17)))
	add(Case("pro-head2-fp8-K192", "prologue", "bf16", "head", "prologue", 34, 192, w8=True, norms=2, Ms=(5, 17)))
	add(Case("gemv-proj-fp8-K1024", "gemv", "bf16", "proj", "plain", 128, 1024, w8=True, family=2, expect_family=2))
	add(Case("gemv-proj-fp8-K4096", "gemv", "bf16", "proj", "plain", 128, 4096, w8=True, family=2, expect_family=2, model_dim=1024))
	for c in cs:
		c.seed = zlib.crc32(c.id.encode())      # a case keeps its operands when cases come and go
	assert len({c.id for c in cs}) == len(cs)
	return cs


CASES = _cases()
GROUPS = sorted({c.group for c in CASES})


def default_waves(c):
	"""skinny_waves of csrc/ar.hip restated (what waves = 0 runs); the LayerNorm prologue caps at 8"""
	d = c.model_dim or (c.N if c.role == "proj" else c.K)
	if d < 1024 or c.role == "head":
		return 4
	if c.form == "prologue" or c.dt == "f32":
		return 8
	return 8 if (c.role == "proj" and c.K != c.N) else 4


def waves_of(c):
	w = max(c.waves or default_waves(c), 4)
	return min(w, 8) if c.form == "prologue" else w


# ----------------------------------------------------------------------------------------------------------- operands
def operands(c):
	"""everything a case's launches read, f64, exact in the case's types; rows for the largest M (a launch over M rows takes the first M)"""
	g = torch.Generator().manual_seed(c.seed)
	Mx = max(c.ms())
	o = {}
	W = grid(torch.randn(c.N, c.K, generator=g), 2.0 ** -3)
	o["W_raw"] = W
	o["W"], o["wscale"] = fp8_round_weights(W) if c.w8 else (W, 1.0)
	o["bias"] = grid(torch.randn(c.N, generator=g))
	if c.form == "plain":
		o["a"] = grid(torch.randn(Mx, c.K, generator=g))
	elif c.form == "fold":
		off = torch.linspace(-1.0, 1.0, Mx).double()[:, None] if Mx > 1 else torch.zeros(1, 1, dtype=torch.float64)
		o["a"] = grid(torch.randn(Mx, c.K, generator=g) + off.float())      # |mean| up to one std
		if c.special == "nearconst":      # 1016 with four channels at 1020: the true variance (0.06) is below what E[x^2] - mean^2 resolves in f32 at this offset
			o["a"][1] = 1016.0
			o["a"][1, 0:250:83] = 1020.0
		o["gamma"] = torch.exp2(torch.randint(-1, 2, (c.K,), generator=g).double()) * (torch.randint(0, 2, (c.K,), generator=g).double() * 2 - 1)
		o["beta"] = grid(torch.randn(c.K, generator=g))
	else:
		off = torch.linspace(-1.0, 1.0, Mx).double()[:, None] if Mx > 1 else torch.zeros(1, 1, dtype=torch.float64)
		o["x"] = grid(torch.randn(Mx, c.K, generator=g) * 2 + off.float())
		o["g1"], o["b1"] = grid(1 + 0.3 * torch.randn(c.K, generator=g)), grid(0.5 * torch.randn(c.K, generator=g))
		if c.norms == 2:
			o["g2"], o["b2"] = grid(1 + 0.3 * torch.randn(c.K, generator=g)), grid(0.5 * torch.randn(c.K, generator=g))
	if c.role == "proj":
		o["res"] = grid(torch.randn(Mx, c.N, generator=g), 4.0)
	return o


def create_weights(c, o):
	"""the named f32 tensors ttk_gemv_mat_create takes: fp8 matrices are handed over UN-rounded (the library rounds them), in the case's layout"""
	w = o["W_raw"].float()
	sd = {"weight": (w if c.layout == 0 else w.t()).contiguous(), "bias": o["bias"].float()}
	if c.form == "fold":
		sd["gamma"], sd["beta"] = o["gamma"].float(), o["beta"].float()
	return sd


# ----------------------------------------------------------------------------------------------------------- reference and bound
def row_stats(x, dx):
	"""mean, var, rstd (f64, [M][1]) of the rows and the bound on what f32 statistics of them can be off by: (dmean, drstd / rstd)"""
	K = x.shape[1]
	mean = x.mean(1, keepdim=True)
	m2 = (x * x).mean(1, keepdim=True)
	var = (m2 - mean * mean).clamp_min(0)
	rstd = 1 / torch.sqrt(var + EPS)
	xa = x.abs() + dx
	ds1 = 2 * K * U * xa.sum(1, keepdim=True)
	ds2 = 2 * K * U * (xa * xa).sum(1, keepdim=True)
	dmean = ds1 / K + U * mean.abs()
	dm2 = ds2 / K + U * m2
	dvar = dm2 + 2 * mean.abs() * dmean + U * mean * mean + U * (m2 - mean * mean).abs()
	drel = 1.02 * (dvar + U * (var + EPS)) / (2 * (var + EPS)) + 2 * U
	drel = torch.where(drel > 0.25, torch.full_like(drel, float("inf")), drel)      # the first-order model ends: no bound on such a row, only the canaries
	return mean, var, rstd, dmean, drel


def ln_stage(x, dx, g, b):
	"""y = LN(x) g + b in f64 and the bound dy on an f32 evaluation of it whose input is off by dx"""
	mean, var, rstd, dmean, drel = row_stats(x, dx)
	d = x - mean
	y = d * rstd * g + b
	prop = rstd * g.abs() * (dx + dx.mean(1, keepdim=True)) + g.abs() * d.abs() * rstd ** 3 * (d.abs() * dx).mean(1, keepdim=True)
	dd = dmean + U * d.abs()
	e = d * rstd
	de = dd * rstd + d.abs() * rstd * drel + U * e.abs()
	f = e * g
	df = de * g.abs() + U * f.abs()
	return y, 1.02 * prop + df + U * y.abs()


def reference(c, o):
	"""the launch's outputs in f64 with their bounds, for the largest M: dict name -> (value, tol); cache rows as [M][d]"""
	W, bias = o["W"], o["bias"]
	dt = c.dt
	if c.form == "plain":
		A = o["a"]
		S = A.abs() @ W.abs().t()
		z = A @ W.t() + bias
		dz = 1e-5 * S + U * z.abs()
	elif c.form == "fold":
		x = o["a"]
		Wf = W * o["gamma"]                                    # gamma o W: exact in T
		csum = Wf.sum(1)
		bf = bias + W @ o["beta"]
		mean, var, rstd, dmean, drel = row_stats(x, torch.zeros_like(x))
		acc = x @ Wf.t()
		S = x.abs() @ Wf.abs().t()
		t = acc - mean * csum
		z = t * rstd + bf
		dt_ = 1e-5 * S + dmean * csum.abs() + 2 * U * (mean * csum).abs() + U * t.abs()
		dz = dt_ * rstd + t.abs() * rstd * drel + U * (t * rstd).abs() + U * bf.abs() + U * z.abs()
	else:
		y, dy = ln_stage(o["x"], torch.zeros_like(o["x"]), o["g1"], o["b1"])
		if c.norms == 2:
			y, dy = ln_stage(y, dy, o["g2"], o["b2"])
		dy = dy + half_ulp_T(y, dy, dt)
		z = y @ W.t() + bias
		dz = dy @ W.abs().t() + 1e-5 * ((y.abs() + dy) @ W.abs().t()) + U * z.abs()
	out = {}
	if c.role == "head":
		out["out_f32"] = (z, dz)
	elif c.role == "proj":
		v = o["res"] + z
		dv = dz + U * v.abs()
		out["out_f32"] = (v, dv)
		if c.out_T:
			out["out_T"] = (v, dv + half_ulp_T(v, dv, dt))
	elif c.role == "fc":
		f, df = gelu_new(z)
		dv = 2e-6 * z.abs() + 1.01 * df.abs() * dz
		out["out_T"] = (f, dv + half_ulp_T(f, dv, dt))
	else:
		d = c.K
		q = z[:, :d] * Q_SCALE
		out["qbuf"] = (q, dz[:, :d] * Q_SCALE + U * q.abs())
		for name, sl in (("k", slice(d, 2 * d)), ("v", slice(2 * d, 3 * d))):
			out[name] = (z[:, sl], dz[:, sl] + half_ulp_T(z[:, sl], dz[:, sl], dt))
	inf = float("inf")      # a row without a bound (row_stats) stays without one through every later term (0 * inf)
	return {k: (v, torch.where(torch.isfinite(tol), tol, torch.full_like(tol, inf))) for k, (v, tol) in out.items()}


# ----------------------------------------------------------------------------------------------------------- output images and their check
def blank_outputs(c, M, o):
	"""what a launch over M rows writes into, in logical layout, everything NaN except the residual stream's live rows: out_f32 [M + canary][N], out_T
	[16 MT][N], qbuf [M + canary][d], kcache / vcache [M + canary][H][max_ctx][64], d_pos"""
	nan = float("nan")
	b = {}
	if c.role in ("head", "proj"):
		b["out_f32"] = torch.full((M + CANARY_ROWS, c.N), nan, dtype=torch.float64)
		if c.role == "proj":
			b["out_f32"][:M] = o["res"][:M]
	if c.role == "fc" or (c.role == "proj" and c.out_T):
		b["out_T"] = torch.full((16 * row_tiles(M), c.N), nan, dtype=torch.float64)
	if c.role == "qkv":
		b["qbuf"] = torch.full((M + CANARY_ROWS, c.K), nan, dtype=torch.float64)
		for n in ("kcache", "vcache"):
			b[n] = torch.full((M + CANARY_ROWS, c.H, c.max_ctx, 64), nan, dtype=torch.float64)
	return b


def check_outputs(c, M, pos, got, ref):
	"""worst |got - ref| / tol over what the launch owes; raises AssertionError when an owed value is not finite or anything else was written"""
	worst = 0.0

	def owed(name, g, key=None):
		nonlocal worst
		r, tol = ref[key or name]
		r, tol = r[:M], tol[:M]
		assert torch.isfinite(g).all(), f"{c.id} M={M}: {name} holds non-finite values where the launch owes a result (unwritten, or padding reached a live element)"
		ratio = ((g - r).abs() / tol)
		w = float(ratio.max())
		if w > worst:
			worst = w
		return w

	def untouched(name, g):
		assert torch.isnan(g).all(), f"{c.id} M={M}: {name} was written where the launch owes nothing ({int((~torch.isnan(g)).sum())} elements)"

	if "out_f32" in got:
		owed("out_f32", got["out_f32"][:M])
		untouched("out_f32 canary rows", got["out_f32"][M:])
	if "out_T" in got:
		owed("out_T", got["out_T"][:M])
		untouched("out_T padding rows", got["out_T"][M:])
	if "qbuf" in got:
		owed("qbuf", got["qbuf"][:M])
		untouched("qbuf canary rows", got["qbuf"][M:])
		for name, key in (("kcache", "k"), ("vcache", "v")):
			cache = got[name].clone()
			if pos < c.max_ctx:
				owed(name, cache[:M, :, pos, :].reshape(M, c.K), key)
				cache[:M, :, pos, :] = float("nan")
			untouched(name + " outside the appended row", cache)
	return worst


# ----------------------------------------------------------------------------------------------------------- the float32 emulation
FAULTS = ("drop_last_kstep", "empty_slice_multiplies", "narrow_without_sub", "xcd_order_any_tile_count", "csum_unrounded", "mean_over_padded_k",
		  "var_without_clamp", "wscale_left_out", "q_scale_on_k", "append_at_pos_plus_1", "append_unguarded", "second_norm_skipped",
		  "second_m_tile_reads_first", "erf_gelu")


def fault_applies(c, fault, M, pos):
	nw, KS = waves_of(c), c.K // 32
	sl = [(KS * w // nw, KS * (w + 1) // nw) for w in range(nw)]
	return {
		"drop_last_kstep": True,
		"empty_slice_multiplies": any(a == b for a, b in sl),
		"narrow_without_sub": c.narrow,
		"xcd_order_any_tile_count": c.narrow and ((c.N + 15) // 16) % 8 != 0,
		"csum_unrounded": c.form == "fold" and c.w8,
		"mean_over_padded_k": c.form != "plain" and c.K % 128 != 0 and c.special == "",
		"var_without_clamp": c.special == "nearconst",
		"wscale_left_out": c.w8 and c.form != "fold",
		"q_scale_on_k": c.role == "qkv" and pos < c.max_ctx,
		"append_at_pos_plus_1": c.role == "qkv" and pos < c.max_ctx,
		"append_unguarded": c.role == "qkv" and pos >= c.max_ctx,
		"second_norm_skipped": c.form == "prologue" and c.norms == 2,
		"second_m_tile_reads_first": M > 16 and c.form != "prologue",
		"erf_gelu": c.role == "fc",
	}[fault]


def f32(t):
	return t.float()


def _seq_sum(vals):
	"""f32 running sum over the last dimension, in order"""
	s = torch.zeros(vals.shape[:-1], dtype=torch.float32)
	for i in range(vals.shape[-1]):
		s = s + vals[..., i]
	return s


def _tree_sum(v):
	"""the wave butterfly: pairwise tree over the last dimension (a power of two)"""
	while v.shape[-1] > 1:
		v = v[..., 0::2] + v[..., 1::2]
	return v[..., 0]


def _rsqrt(v):
	return (1 / torch.sqrt(v.double())).float()


def _products(c, A, Wm, nw, fault):
	"""sum over the waves (in wave order) of each wave's accumulator: A [M][K] and Wm [N][K] hold T-exact values (f64)"""
	KS = c.K // 32
	M, N = A.shape[0], Wm.shape[0]
	total = torch.zeros(M, N, dtype=torch.float32)
	for w in range(nw):
		ks0, ks1 = KS * w // nw, KS * (w + 1) // nw
		steps = list(range(ks0, ks1))
		if fault == "drop_last_kstep" and w == nw - 1 and steps:
			steps = steps[:-1]
		if fault == "empty_slice_multiplies" and not steps:
			steps = [max(ks0 - 1, 0)]              # the slot that re-reads the last fragment
		acc = torch.zeros(M, N, dtype=torch.float32)
		for ks in steps:
			a, b = A[:, 32 * ks:32 * ks + 32], Wm[:, 32 * ks:32 * ks + 32]
			if c.dt == "f32":                     # eight 16x16x4 instructions, instruction j contracts k = 8 g + j
				for j in range(8):
					acc = (acc.double() + a[:, j::8] @ b[:, j::8].t()).float()
			else:
				acc = (acc.double() + a @ b.t()).float()
		total = total + acc
	return total


def _fold_stats(c, x, nw, family, fault):
	"""mean, var (before the clamp), sum of squares as the kernels gather them from the fragments: [M]"""
	KS, M = c.K // 32, x.shape[0]
	xf = x.float()
	a1 = torch.zeros(M, dtype=torch.float32)
	a2 = torch.zeros(M, dtype=torch.float32)
	for w in range(nw):
		ks0, ks1 = KS * w // nw, KS * (w + 1) // nw
		if ks1 == ks0:
			continue
		seg = xf[:, 32 * ks0:32 * ks1].reshape(M, ks1 - ks0, 4, 8).permute(0, 2, 1, 3).reshape(M, 4, -1)      # lane (row, k-group): its elements in order
		if family == 2 and c.dt != "f32":        # dot2: one rounding per pair
			p1 = (seg[..., 0::2].double() + seg[..., 1::2].double())
			p2 = (seg[..., 0::2].double() ** 2 + seg[..., 1::2].double() ** 2)
			s1 = torch.zeros(M, 4, dtype=torch.float32)
			s2 = torch.zeros(M, 4, dtype=torch.float32)
			for i in range(p1.shape[-1]):
				s1 = (s1.double() + p1[..., i]).float()
				s2 = (s2.double() + p2[..., i]).float()
		else:
			s1 = _seq_sum(seg)
			s2 = torch.zeros(M, 4, dtype=torch.float32)
			for i in range(seg.shape[-1]):
				s2 = (s2.double() + seg[..., i].double() ** 2).float()      # fma
		s1 = (s1[:, 0] + s1[:, 1]) + (s1[:, 2] + s1[:, 3])
		s2 = (s2[:, 0] + s2[:, 1]) + (s2[:, 2] + s2[:, 3])
		a1, a2 = a1 + s1, a2 + s2
	Kd = float(c.K if fault != "mean_over_padded_k" else (c.K + 127) // 128 * 128)
	mean = a1 / Kd
	var = ((a2 / Kd).double() - mean.double() * mean.double()).float()      # fma(-mean, mean, a2 / K): k_gemv writes it, k_skinny's expression contracts to it
	return mean, var, a2


def _ln_f32(c, x, g, b, fault):
	"""the prologue's LayerNorm of f32 rows [M][K]: lane partials over the lane's float4 chunks, the wave butterfly, then the affine, one rounding per operation"""
	M, K = x.shape
	nchunk = K // 4
	per = (nchunk + 63) // 64
	pad = torch.zeros(M, per * 64 * 4, dtype=torch.float32)
	pad[:, :K] = x
	ch = pad.reshape(M, per, 64, 4).permute(0, 2, 1, 3)            # [M][lane][i][4]
	s1 = torch.zeros(M, 64, dtype=torch.float32)
	s2 = torch.zeros(M, 64, dtype=torch.float32)
	for i in range(per):
		v = ch[:, :, i]
		s1 = s1 + (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
		s2 = s2 + (((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) + v[..., 3] * v[..., 3])
	s1, s2 = _tree_sum(s1), _tree_sum(s2)
	Kd = float(K if fault != "mean_over_padded_k" else (K + 127) // 128 * 128)
	mean = s1 / Kd
	var = s2 / Kd - mean * mean
	if fault != "var_without_clamp":
		var = var.clamp_min(0)
	rstd = _rsqrt(var + f32(torch.tensor(EPS)))
	return ((x - mean[:, None]) * rstd[:, None]) * g.float() + b.float()


def emulate(c, o, M, pos=0, fault=None, family=None, waves=None):
	"""the outputs of one launch over the first M rows, in blank_outputs' layout, computed the way the kernels compute them"""
	family = family or c.family
	nw = waves or waves_of(c)
	if family == 2:
		nw = {True: 8, False: 4}[c.K == 4096 or (c.dt == "f32" and c.role != "head")]
	tdt = TDT[c.dt]
	out = blank_outputs(c, M, o)
	W = o["W"]
	bias = o["bias"].float()
	wscale = 1.0
	if c.form == "fold":
		Wm = W * o["gamma"]
		src = (o["W_raw"] * o["gamma"]) if fault == "csum_unrounded" else Wm
		csum = src.sum(1).float()
		bias = (o["bias"] + W @ o["beta"]).float()
	elif c.w8:
		Wm, wscale = W / o["wscale"], o["wscale"]              # the fp8 bytes, widened exactly
	else:
		Wm = W
	if c.form == "prologue":
		y = _ln_f32(c, o["x"][:M].float(), o["g1"], o["b1"], fault)
		if c.norms == 2 and fault != "second_norm_skipped":
			y = _ln_f32(c, y, o["g2"], o["b2"], fault)
		A = y.to(tdt).double()
	else:
		A = o["a"][:M]
	Mp = 16 * row_tiles(M)
	Ap = torch.zeros(Mp, c.K, dtype=torch.float64)
	Ap[:M] = A
	ntiles = (c.N + 15) // 16
	Wp = torch.zeros(ntiles * 16, c.K, dtype=torch.float64)
	Wp[:c.N] = Wm
	# which weight column every output column's workgroup fetches
	col = torch.arange(ntiles * 16)
	written = torch.ones(ntiles * 16, dtype=torch.bool)
	if c.narrow:
		nblk = ntiles * 4
		b = torch.arange(nblk)
		xcd = ntiles % 8 == 0 or fault == "xcd_order_any_tile_count"
		nt = (b // 32) * 8 + (b % 8) if xcd else b // 4
		sub = (b // 8) % 4 if xcd else b % 4
		src_col = torch.full((ntiles * 16,), -1, dtype=torch.long)
		for j in range(4):
			n = nt * 16 + 4 * sub + j
			ok = nt < ntiles
			src_col[n[ok]] = (nt * 16 + (0 if fault == "narrow_without_sub" else 4 * sub) + j)[ok]
		written = src_col >= 0
		col = src_col.clamp_min(0)
	if fault == "second_m_tile_reads_first":      # rows 16.. of the operand fetched with the first tile's index
		Ap = Ap.clone()
		Ap[16:min(M, 32)] = Ap[:min(M, 32) - 16]
	acc = _products(c, Ap, Wp[col], nw, fault)[:M, :c.N]
	written = written[:c.N]
	if c.form == "fold":
		mean, var, a2 = _fold_stats(c, Ap[:M], nw, family, fault)
		if fault != "var_without_clamp":
			var = var.clamp_min(0)
		rstd = _rsqrt(var + f32(torch.tensor(EPS)))
		z = (acc - mean[:, None] * csum) * rstd[:, None] + bias
	else:
		z = (acc * wscale if (c.w8 and fault != "wscale_left_out") else acc) + bias
	nan = torch.full_like(z, float("nan"))
	if c.role == "head":
		out["out_f32"][:M] = torch.where(written, z, nan).double()
	elif c.role == "proj":
		v = o["res"][:M].float() + z
		out["out_f32"][:M] = torch.where(written, v, o["res"][:M].float()).double()
		if c.out_T:
			out["out_T"][:M] = torch.where(written, v.to(tdt).float(), nan).double()
	elif c.role == "fc":
		if fault == "erf_gelu":
			act = 0.5 * z * (1 + torch.erf(z * f32(torch.tensor(math.sqrt(0.5)))))
		else:
			u = f32(torch.tensor(0.7978845608028654)) * (z + f32(torch.tensor(0.044715)) * z * z * z)
			act = 0.5 * z * (1 + (1 - 2 / (1 + torch.exp(2 * u))))
		out["out_T"][:M] = act.to(tdt).double()
	else:
		d = c.K
		out["qbuf"][:M] = (z[:, :d] * Q_SCALE).double()
		row = pos + 1 if fault == "append_at_pos_plus_1" else pos
		for name, sl in (("kcache", slice(d, 2 * d)), ("vcache", slice(2 * d, 3 * d))):
			v = z[:, sl] * (Q_SCALE if (fault == "q_scale_on_k" and name == "kcache") else 1.0)
			v = v.to(tdt).double().reshape(M, c.H, 64)
			flat = out[name].reshape(-1, 64)                    # [(m, h, row)][64]: an unguarded row index runs on into the next head's rows
			if row < c.max_ctx or fault == "append_unguarded":
				m, h = torch.meshgrid(torch.arange(M), torch.arange(c.H), indexing="ij")
				flat[(m * c.H + h) * c.max_ctx + row] = v
	return out
