"""Float64 references of the vocoders' own kernels -- the location-variable convolution with its gated update (csrc/univnet.hip: k_lvc<T, 16 / 32>, k_lvc_mfma),
the narrow-channel MFMA convolution with its weight packing (csrc/hifigan.hip: k_hifi_conv_mfma<32 / 64>, k_hifi_pack_frag) and the anti-aliased snake activation
(csrc/voc.hip: k_snake_aa<float / bf16>) -- written from the definitions in the kernel comments over the kernels' own operands, with a derived per-element error
bound, the case lists and seeded CPU operands that tests/test_voc_ref.py (CPU) and tests/test_gpu_voc_forms.py (GPU, through ttk_lvc_rows, ttk_hifi_conv_rows and
ttk_snake_rows) share, and a float32 replica of each kernel's indexing with faults switchable by name, which shows that the bound and the canaries see them.

DEFINITIONS.  lrelu_s(v) = v > 0 ? v : v s with the kernels' f32 slope constants (0.2f in univnet.hip, 0.1f in hifigan.hip).
  LVC, layer `layer` of `n_layers`, B sequences of L rows, frame f = t / hop:
      o[t][n] = kbias[f][layer][n] + sum_i sum_k lrelu_0.2(y)[t + k - 1][i] kern[f][layer][i][n][k]        rows outside [0, L) of the sequence are zero
      x[t][c] += sigmoid(o[t][c]) tanh(o[t][c + CG]);      at[t][c] = T(lrelu_0.2(x[t][c]))
  k_lvc_mfma stores bf16(lrelu(y)) as its A operand: that rounding (of the f32 product y 0.2f) is part of its definition and the reference applies it.
  Narrow conv, one sequence of L rows, K taps, dilation d:
      v[t][n] = bias[n] + sum_k sum_i a[t + (k - (K - 1) / 2) d][i] bf16(w[n][i][k])                         the packer rounds w to bf16: part of the definition
      mode 0: at_out = bf16(lrelu_0.1(v));  1: xout = v + xres, at_out = bf16(lrelu_0.1(xout));  2: mrf = v + xres;  3: mrf += v + xres
  Snake (Activation1d with SnakeBeta), g the 12-tap low-pass, every clamp within one sequence:
      up[2q] = 2 sum_j x[clamp(q - 3 + j)] g[11 - 2j],   up[2q + 1] = 2 sum_j x[clamp(q - 2 + j)] g[10 - 2j]      (j = 0 .. 5)
      z[s] = up[s] + invb sin(up[s] a)^2,   y[t] = sum_k z[clamp(2t + k - 5, 0, 2L - 1)] g[k]

THE BOUND, per element.  u = 2^-24, one rounding per f32 operation, second-order terms covered by the factors 1.01.
  sums        Products of two bf16 values are exact in f32 and the sum of n of them, in any order, is within 1.01 n u sum|a_i b_i| (n = 3 CG for the LVC); f32
              operands add one rounding for the product (n + 1), and k_lvc's lrelu(y) = y 0.2f one more on its operand (n + 2 in f32, n + 1 in bf16).  The real
              magnitudes sum|a_i b_i| are taken per output element.
  MFMA        v_mfma_f32_16x16x32_bf16 accumulation (k_lvc_mfma, k_hifi_conv_mfma): 1e-5 sum|a_i b_i|, the allowance tests/test_gpu_gemm_forms.py uses for that
              instruction -- not a new one.
  epilogue    bias, residual, MRF add, the gated update's product and add, lrelu: one rounding each, u |result|.
  gate        sigma(a) tanh(g) with a, g off by da, dg: 1.01 (0.25 da + dg) (|sigma'| <= 1 / 4, |tanh'| <= 1, |sigma|, |tanh| <= 1) plus the functions' own error.
              HIP's documentation here states no accuracy for expf / tanhf / sinf, so each call gets the project's existing constant for a transcendental, the
              2e-6 |f| of the SiLU in test_gpu_gemm_forms.py and norm_ref.py: sigma = 1 / (1 + expf(-a)) is (2e-6 + 2u) |sigma| (expf, the add, the division: the
              error of e in 1 / (1 + e) is damped by e / (1 + e) < 1), tanhf is 2e-6 |tanh|.
  snake       up: 6 products, their sum and the doubling, 1.01 * 8 u * 2 sum|x g|;  arg = up a: |a| dup + u |arg|;  s = sin(arg): ds = darg + DELTA, DELTA = 2e-6 |s|
              for sinf (f32 form) and SIN_FAST_ERR for __sinf (bf16 form);  s^2: 2.02 |s| ds + u s^2;  z: dup + |invb| ds2 + u |invb s^2| + u |z|;
              y: sum_k |g_k| dz_k + 1.01 * 13 u sum|z_k g_k|.  The intrinsic's term is therefore 2 |invb| |sin| SIN_FAST_ERR sum|g| per output.
  output      as norm_ref.out_rounding: 2^-8 (|v| + tol) for bf16, nothing for f32.
No term is fitted to a result of the kernels under test.

__sinf (v_sin_f32 behind a multiply by 1 / 2 pi) is the one figure that cannot be derived here.  It was measured once, on an MI355X, on 2026-10-21, by the
stand-alone probe tests/diag/sinf_probe.cpp (the intrinsic alone, not k_snake_aa): 2^26 arguments evenly spaced over [-16, 16] against sin() of the same f32
argument in double; worst |error| 1.415e-6 (at x = -15.757; below |x| = 4: 3.9e-7).  The probe samples the range and does not sweep it, so SIN_FAST_ERR is twice
the measured figure, 2.83e-6, and the snake operands keep |up a| <= SNAKE_ARG_MAX = 16 (asserted in test_voc_ref.py, together with max |up a| >= pi).

OPERANDS (seeded CPU generator).  bf16 operands lie on the bf16 grid (`a` of the narrow conv, `kern` of the bf16 LVC).  The LVC kernels are scaled by 1 / sqrt(3 CG):
the pre-activations have unit order, the gate is not saturated (test_voc_ref.py: at least half of the outputs have |a| < 2 and |g| < 1.5), and an error in either half
reaches x.  The narrow conv's `a` has standard deviation 1 / 4 so that the f32 outputs' bounds stay below 1e-4 (1 + |v|) at k C = 704 products, three orders below
a single dropped product.  B = 2 everywhere a batch exists, with different values per element.

THE REPLICAS follow the code: workgroup windows with their zero fill, k_lvc's row per lane and its i-ascending accumulation, k_lvc_mfma's 16-row tiles with the
segment loop and the `own` mask, one f32 rounding per MFMA, k_hifi_pack_frag's index decomposition and k_hifi_conv_mfma's read of it, the epilogues' row cuts, k_snake_aa's
13 clamped rows in registers with k0 / k1.  Memory the kernel must not read is NaN in the replicas' view as it is in the GPU test's buffers.
"""
import functools
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from norm_ref import out_rounding as _norm_out_rounding

U = 2.0 ** -24
MFMA = 1e-5                                    # test_gpu_gemm_forms.py: f32 accumulation of v_mfma_f32_16x16x32_bf16, per unit of sum|a||w|
TRANS = 2e-6                                   # test_gpu_gemm_forms.py / norm_ref.py: a transcendental's own relative error
SIN_FAST_MEASURED = 1.415251e-06               # tests/diag/sinf_probe.cpp, MI355X, 2026-10-21, [-16, 16]
SIN_FAST_ERR = 2 * SIN_FAST_MEASURED
SNAKE_ARG_MAX = 16.0
S02 = float(torch.tensor(0.2, dtype=torch.float32))      # the slope constants as the kernels hold them
S01 = float(torch.tensor(0.1, dtype=torch.float32))
B = 2
NAN = float("nan")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def bf(t):
	"""round to the bf16 grid (nearest even), held as f32"""
	return t.float().bfloat16().float()


def lrelu64(v, s):
	return torch.where(v > 0, v, v * s)


def out_rounding(v, tol, dt):
	return _norm_out_rounding(v, tol, dt)


def to_out(v, dt):
	"""an f32 result as the kernel stores it, read back as f64"""
	return v.float().to(TDT[dt]).double()


def _gen(seed):
	return torch.Generator().manual_seed(seed)


def _ratio(got, ref, tol):
	return float(((got - ref).abs() / tol).max())


def _owed(what, g):
	assert torch.isfinite(g).all(), f"{what}: non-finite values where the launch owes a result"


def _untouched(what, g):
	assert torch.isnan(g).all(), f"{what}: written where the launch owes nothing ({int((~torch.isnan(g)).sum())} elements)"


# =========================================================================================================== LVC
LVC_CANARY_ROWS = 3
LVC_LDA = 64


@dataclass(frozen=True)
class LvcCase:
	dt: str
	CG: int
	hop: int
	Tc: int
	L: int
	n_layers: int
	layer: int

	@property
	def id(self):
		return f"lvc-{self.dt}-cg{self.CG}-hop{self.hop}-Tc{self.Tc}-L{self.L}-layer{self.layer}of{self.n_layers}"

	@property
	def mfma(self):
		return self.dt == "bf16" and self.CG == 32

	@property
	def group(self):
		return f"lvc-{self.dt}-cg{self.CG}" + ("-mfma" if self.mfma else "")

	@property
	def kstride(self):
		return self.n_layers * self.CG * 2 * self.CG * 3

	@property
	def bstride(self):
		return self.n_layers * 2 * self.CG

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())


LVC_SHAPES = ((1, 37, 37), (3, 23, 69), (4, 19, 76), (8, 11, 88), (64, 3, 192), (256, 2, 512), (8, 12, 90))      # (hop, Tc, L)
LVC_FORMS = (("f32", 16), ("f32", 32), ("bf16", 16), ("bf16", 32))
LVC_LAYERS = ((4, 0), (4, 3), (1, 0))                                                                           # (n_layers, layer)
LVC_CASES = [LvcCase(dt, cg, hop, Tc, L, *LVC_LAYERS[(i + j) % 3]) for j, (dt, cg) in enumerate(LVC_FORMS) for i, (hop, Tc, L) in enumerate(LVC_SHAPES)]
assert len({c.id for c in LVC_CASES}) == len(LVC_CASES)


@functools.lru_cache(maxsize=4)
def lvc_operands(c):
	"""y, x f32 [B L][CG]; kern f32 [B Tc][kstride] (on the bf16 grid in bf16 mode); kbias f32 [B Tc][bstride]"""
	g = _gen(c.seed)
	rows = B * c.L
	kern = torch.randn(B * c.Tc, c.kstride, generator=g) / math.sqrt(3 * c.CG)
	return {"y": torch.randn(rows, c.CG, generator=g), "x": torch.randn(rows, c.CG, generator=g), "kern": bf(kern) if c.dt == "bf16" else kern,
			"kbias": 0.3 * torch.randn(B * c.Tc, c.bstride, generator=g)}


@functools.lru_cache(maxsize=4)
def lvc_reference(c):
	"""dict: x, at f64 [B L][CG] with their bounds tol_x, tol_at, and the pre-activations a, g"""
	o = lvc_operands(c)
	CG, L = c.CG, c.L
	y = o["y"]
	if c.mfma:
		yl = bf(torch.where(y > 0, y, y * 0.2)).double()
	else:
		yl = lrelu64(y.double(), S02)
	ylp = F.pad(yl.view(B, L, CG), (0, 0, 1, 1))
	win = torch.stack([ylp[:, k:k + L] for k in range(3)], 2)                                       # [B][L][tap][i]
	f = torch.arange(L) // c.hop
	W = o["kern"].double().view(B, c.Tc, c.n_layers, CG, 2 * CG, 3)[:, f, c.layer]                  # [B][L][i][n][tap]
	acc = torch.einsum("blki,blink->bln", win, W)
	mag = torch.einsum("blki,blink->bln", win.abs(), W.abs())
	pre = acc + o["kbias"].double().view(B, c.Tc, c.n_layers, 2 * CG)[:, f, c.layer]
	n = 3 * CG
	dacc = MFMA * mag if c.mfma else 1.01 * (n + (2 if c.dt == "f32" else 1)) * U * mag
	dpre = (dacc + U * pre.abs()).view(B * L, 2 * CG)
	pre = pre.view(B * L, 2 * CG)
	a, gg, da, dg = pre[:, :CG], pre[:, CG:], dpre[:, :CG], dpre[:, CG:]
	s, th = torch.sigmoid(a), torch.tanh(gg)
	v = s * th
	dv = 1.01 * (0.25 * da + dg) + (TRANS + 2 * U) * s * th.abs() + TRANS * s * th.abs() + U * v.abs()
	x = o["x"].double() + v
	tol_x = dv + U * x.abs()
	at = lrelu64(x, S02)
	tol_at = tol_x + U * at.abs()
	return {"x": x, "tol_x": tol_x, "at": at, "tol_at": tol_at + out_rounding(at, tol_at, c.dt), "a": a, "g": gg}


def lvc_blank(c, o):
	"""the images of one launch, before it: x holds the operand with NaN canary rows behind it, at is all NaN"""
	x = torch.full((B * c.L + LVC_CANARY_ROWS, c.CG), NAN, dtype=torch.float64)
	x[:B * c.L] = o["x"].double()
	return {"x": x, "at": torch.full((B * c.L + LVC_CANARY_ROWS, LVC_LDA), NAN, dtype=torch.float64)}


def lvc_check(c, got):
	"""worst |got - ref| / tol, {"x f32": ..., "at f32" or "at rounded": ...}; AssertionError when an owed value is not finite or anything else was written"""
	r = lvc_reference(c)
	rows = B * c.L
	_owed(f"{c.id}: x", got["x"][:rows])
	_owed(f"{c.id}: at", got["at"][:rows, :c.CG])
	_untouched(f"{c.id}: x behind the rows", got["x"][rows:])
	_untouched(f"{c.id}: at behind the rows", got["at"][rows:])
	_untouched(f"{c.id}: at columns [CG, lda)", got["at"][:rows, c.CG:])
	return {"x f32": _ratio(got["x"][:rows], r["x"], r["tol_x"]), "at f32" if c.dt == "f32" else "at rounded": _ratio(got["at"][:rows, :c.CG], r["at"], r["tol_at"])}


LVC_FAULTS = ("straddling_tile_takes_first_segments_kernel", "end_halo_not_zeroed", "bias_of_frame_t0", "tanh_partner_one_ntile_early", "taps_reversed",
			  "layer_offset_ignores_layer")


def lvc_fault_applies(c, fault):
	return {"straddling_tile_takes_first_segments_kernel": c.hop < 16 or c.hop % 16 != 0, "end_halo_not_zeroed": True, "bias_of_frame_t0": c.hop < 16 or c.hop % 16 != 0,
			"tanh_partner_one_ntile_early": True, "taps_reversed": True, "layer_offset_ignores_layer": c.layer > 0}[fault]


def _f32_acc(acc, a, b):
	"""acc + a @ b with one f32 rounding (the products and their sum held exactly enough in f64)"""
	return (acc.double() + a.double() @ b.double()).float()


def lvc_emulate(c, fault=None):
	"""the images of one launch (lvc_blank's layout) computed the way k_lvc / k_lvc_mfma compute them: grid (ceil(L / 64), B), a 66-row window per workgroup"""
	o = lvc_operands(c)
	CG, L, hop = c.CG, c.L, c.hop
	img = lvc_blank(c, o)
	y = o["y"]
	guard = torch.full((1, CG), NAN)
	yflat = torch.cat([guard, y, guard])                          # row -1 and row B L are memory the kernel must not read
	layer = 0 if fault == "layer_offset_ignores_layer" else c.layer
	kern = o["kern"].view(B * c.Tc, c.n_layers, CG, 2 * CG, 3)
	kbias = o["kbias"].view(B * c.Tc, c.n_layers, 2 * CG)
	if fault == "taps_reversed":
		kern = kern.flip(-1)
	part = CG // 2 if fault == "tanh_partner_one_ntile_early" else CG          # (n-tile nt + 1 of k_lvc_mfma; the same channel distance in k_lvc)
	xin = o["x"]
	slope = torch.tensor(0.2, dtype=torch.float32)
	for b in range(B):
		for t0 in range(0, L, 64):
			ys = torch.zeros(66, CG)
			for r in range(66):
				t = t0 - 1 + r
				if 0 <= t < L or (fault == "end_halo_not_zeroed" and t in (-1, L)):
					v = yflat[1 + b * L + t]
					ys[r] = torch.where(v > 0, v, v * slope)
			nrow = min(64, L - t0)
			tt = t0 + torch.arange(nrow)
			if c.mfma:
				ys = bf(ys)
				pre = torch.zeros(nrow, 2 * CG)
				for w in range(4):
					r0 = t0 + 16 * w
					if r0 >= L:
						break
					rlast = min(r0 + 15, L - 1)
					ta = r0 + torch.arange(16)
					acc = torch.zeros(16, 2 * CG)
					segs = [r0 // hop] if fault == "straddling_tile_takes_first_segments_kernel" else range(r0 // hop, rlast // hop + 1)
					for seg in segs:
						own = (ta < L) if fault == "straddling_tile_takes_first_segments_kernel" else (ta < L) & (ta // hop == seg)
						wl = kern[b * c.Tc + seg, layer]
						for tap in range(3):
							a = torch.where(own[:, None], ys[16 * w + tap:16 * w + tap + 16], torch.zeros(1))
							acc = _f32_acc(acc, a, wl[:, :, tap])
					k = rlast - r0 + 1
					pre[16 * w:16 * w + k] = acc[:k]
				tile0 = t0 + 16 * (torch.arange(nrow) // 16)
			else:
				frame = tt // hop
				tile0 = torch.full((nrow,), t0)
				if fault == "straddling_tile_takes_first_segments_kernel":
					frame = (t0 + 16 * (torch.arange(nrow) // 16)) // hop
				wl = kern[b * c.Tc + frame, layer]                                       # [row][i][n][tap]
				pre = torch.zeros(nrow, 2 * CG)
				for i in range(CG):
					pre = pre + ((ys[0:nrow, i, None] * wl[:, i, :, 0] + ys[1:nrow + 1, i, None] * wl[:, i, :, 1]) + ys[2:nrow + 2, i, None] * wl[:, i, :, 2])
			bframe = (tile0 if fault == "bias_of_frame_t0" else tt) // hop
			pre = pre + kbias[b * c.Tc + bframe, layer]
			a, gg = pre[:, :CG], pre[:, part:part + CG]
			rows = b * L + tt
			v = xin[rows] + (1 / (1 + torch.exp(-a))) * torch.tanh(gg)
			img["x"][rows] = v.double()
			img["at"][rows, :CG] = to_out(torch.where(v > 0, v, v * slope), c.dt)
	return img


# =========================================================================================================== narrow conv
HIFI_CANARY_ROWS = 64                          # a wave's last 16-row tile reaches at most 63 rows past L
HIFI_MODES = {0: "act", 1: "res", 2: "mrf_set", 3: "mrf_add"}


@dataclass(frozen=True)
class HifiCase:
	C: int
	k: int
	dil: int
	L: int
	mode: int

	@property
	def id(self):
		return f"hifi-C{self.C}-k{self.k}-d{self.dil}-L{self.L}-{HIFI_MODES[self.mode]}"

	@property
	def group(self):
		return f"hifi-conv-C{self.C}"

	@property
	def ld(self):
		"""lda = ldo: 64 at C = 32 (32 columns the kernel must neither read into a result nor write), 72 at C = 64"""
		return 64 if self.C == 32 else 72

	@property
	def halo(self):
		return (self.k - 1) // 2 * self.dil

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())


HIFI_KD = ((3, 1), (3, 5), (7, 3), (11, 1), (11, 5))
HIFI_LS = (1, 7, 257, 530)


def _hifi_cases():
	cs = []
	for i, (mode, L) in enumerate((m, L) for m in range(4) for L in HIFI_LS):      # every (mode, L) pair; C and (k, dil) walk through their values
		cs.append(HifiCase((32, 64)[(i + i // 4) % 2], *HIFI_KD[i % 5], L, mode))
	# k = 11 with dil = 5 at C = 64, the largest window, in the two epilogues that write two buffers / accumulate; and every (k, dil) at both widths
	cs += [HifiCase(64, 11, 5, 530, 1), HifiCase(64, 11, 5, 257, 3), HifiCase(32, 11, 5, 530, 0), HifiCase(64, 3, 5, 257, 2), HifiCase(32, 7, 3, 7, 1),
		   HifiCase(64, 3, 1, 530, 3), HifiCase(32, 11, 1, 257, 2), HifiCase(32, 3, 5, 1, 3)]
	return list(dict.fromkeys(cs))                                 # (an extra that the walk already produced appears once)


HIFI_CASES = _hifi_cases()


@functools.lru_cache(maxsize=4)
def hifi_operands(c):
	"""a f32 [L][C] on the bf16 grid; w f32 [C][C][k] (Conv1d's layout, NOT rounded: the packer does that); bias f32 [C]; xres, mrf0 f32 [L][C]"""
	g = _gen(c.seed)
	return {"a": bf(0.25 * torch.randn(c.L, c.C, generator=g)), "w": torch.randn(c.C, c.C, c.k, generator=g) / math.sqrt(c.k * c.C),
			"bias": 0.3 * torch.randn(c.C, generator=g), "xres": torch.randn(c.L, c.C, generator=g), "mrf0": torch.randn(c.L, c.C, generator=g)}


@functools.lru_cache(maxsize=4)
def hifi_reference(c):
	"""dict name -> (value f64 [L][C], tol) for what the mode writes: at_out, xout, mrf"""
	o = hifi_operands(c)
	a = o["a"].double().t()[None]
	wb = bf(o["w"]).double()
	conv = F.conv1d(a, wb, None, 1, c.halo, c.dil)[0].t()
	mag = F.conv1d(a.abs(), wb.abs(), None, 1, c.halo, c.dil)[0].t()
	v = conv + o["bias"].double()
	tol = MFMA * mag + U * v.abs()
	if c.mode != 0:
		v = v + o["xres"].double()
		tol = tol + U * v.abs()
	out = {}
	if c.mode >= 2:
		if c.mode == 3:
			v = o["mrf0"].double() + v
			tol = tol + U * v.abs()
		out["mrf"] = (v, tol)
	else:
		if c.mode == 1:
			out["xout"] = (v, tol)
		at = lrelu64(v, S01)
		tat = tol + U * at.abs()
		out["at_out"] = (at, tat + out_rounding(at, tat, "bf16"))
	return out


def hifi_blank(c, o):
	"""the images of one launch, before it: xout is the residual itself in mode 1 (the model updates it in place), mrf holds the running sum in mode 3; all else NaN"""
	rows = c.L + HIFI_CANARY_ROWS
	img = {"at_out": torch.full((rows, c.ld), NAN, dtype=torch.float64), "xout": torch.full((rows, c.C), NAN, dtype=torch.float64),
		   "mrf": torch.full((rows, c.C), NAN, dtype=torch.float64)}
	if c.mode == 1:
		img["xout"][:c.L] = o["xres"].double()
	if c.mode == 3:
		img["mrf"][:c.L] = o["mrf0"].double()
	return img


def hifi_check(c, got):
	"""worst |got - ref| / tol per output class; AssertionError when an owed value is not finite or anything else was written"""
	ref = hifi_reference(c)
	w = {}
	for name, width in (("at_out", c.C), ("xout", c.C), ("mrf", c.C)):
		g = got[name]
		if name in ref:
			v, tol = ref[name]
			_owed(f"{c.id}: {name}", g[:c.L, :width])
			_untouched(f"{c.id}: {name} behind the rows", g[c.L:])
			_untouched(f"{c.id}: {name} behind the columns", g[:c.L, width:])
			w["at_out rounded" if name == "at_out" else f"{name} f32"] = _ratio(g[:c.L, :width], v, tol)
		else:
			_untouched(f"{c.id}: {name}, which mode {c.mode} does not write", g)
	return w


HIFI_FAULTS = ("halo_forgets_dil", "kb_and_nt_swapped_in_fragment_order", "last_mt_tile_not_cut_at_L", "mrf_add_sets", "slope_0.2", "residual_dropped_in_mode_2")


def hifi_fault_applies(c, fault):
	return {"halo_forgets_dil": c.dil > 1 and c.k > 1, "kb_and_nt_swapped_in_fragment_order": c.C == 64, "last_mt_tile_not_cut_at_L": c.L % 64 != 0, "mrf_add_sets": c.mode == 3,
			"slope_0.2": c.mode < 2, "residual_dropped_in_mode_2": c.mode == 2}[fault]


def hifi_pack(c, w, fault=None):
	"""upload_mat(PK_CONVK) + k_hifi_pack_frag: f32 [C][C][k] -> bf16 values in B-fragment order, flat [k C C]"""
	C, k = c.C, c.k
	NT, KB = C // 16, C // 32
	wt = bf(w).permute(2, 0, 1).contiguous()                       # [tap][n][k]: W_tap[n][i] = w[n][i][tap] (Npad, Kpad hold zeros beyond C)
	idx = torch.arange(k * C * C)
	j, lane, rest = idx & 7, (idx >> 3) & 63, idx >> 9
	if fault == "kb_and_nt_swapped_in_fragment_order":
		kb = rest % KB; rest = rest // KB
		nt, tap = rest % NT, rest // NT
	else:
		nt = rest % NT; rest = rest // NT
		kb, tap = rest % KB, rest // KB
	l15, g = lane & 15, lane >> 4
	return wt[tap, 16 * nt + l15, 32 * kb + 8 * g + j]


def hifi_emulate(c, fault=None):
	"""the images of one launch (hifi_blank's layout) computed the way k_hifi_pack_frag and k_hifi_conv_mfma compute them: grid ceil(L / 256), 4 waves of 64 rows"""
	o = hifi_operands(c)
	C, k, dil, L = c.C, c.k, c.dil, c.L
	NT, KB = C // 16, C // 32
	img = hifi_blank(c, o)
	frag = hifi_pack(c, o["w"], fault)
	# the kernel's read: fragment (tap, kb, nt), lane (l15, g), element j is B[k = 8 g + j][n = l15]
	Bm = frag.view(k, KB, NT, 4, 16, 8).permute(0, 1, 2, 3, 5, 4).reshape(k, KB, NT, 32, 16)
	halo = (k - 1) // 2 * (1 if fault == "halo_forgets_dil" else dil)
	R = 256 + 2 * halo
	span = 256 + (k - 1) * dil                                     # rows the taps reach; beyond R the LDS was never staged
	slope = torch.tensor(0.2 if fault == "slope_0.2" else 0.1, dtype=torch.float32)
	for t0 in range(0, L, 256):
		ys = torch.full((max(R, span), C), NAN)
		for r in range(R):
			t = t0 - halo + r
			ys[r] = o["a"][t] if 0 <= t < L else 0.0
		acc = torch.zeros(256, C)
		for tap in range(k):
			for kb in range(KB):
				av = ys[tap * dil:tap * dil + 256, 32 * kb:32 * kb + 32]
				for nt in range(NT):
					acc[:, 16 * nt:16 * nt + 16] = _f32_acc(acc[:, 16 * nt:16 * nt + 16], av, Bm[tap, kb, nt])
		v = acc + o["bias"]
		for w in range(4):
			r0 = t0 + 64 * w
			if r0 >= L:
				break
			for mt in range(4):
				lo = r0 + 16 * mt
				hi = lo + 16 if (fault == "last_mt_tile_not_cut_at_L" and mt == 3) else min(lo + 16, L)
				if hi <= lo:
					continue
				t = torch.arange(lo, hi)
				vv = v[t - t0]
				if c.mode != 0 and not (fault == "residual_dropped_in_mode_2" and c.mode == 2):
					xr = torch.full((hi - lo, C), NAN)
					live = t < L
					xr[live] = o["xres"][t[live]]
					vv = vv + xr
				if c.mode == 2 or (c.mode == 3 and fault == "mrf_add_sets"):
					img["mrf"][t] = vv.double()
				elif c.mode == 3:
					img["mrf"][t] = (img["mrf"][t].float() + vv).double()
				else:
					if c.mode == 1:
						img["xout"][t] = vv.double()
					img["at_out"][t, :C] = to_out(torch.where(vv > 0, vv, vv * slope), "bf16")
	return img


# =========================================================================================================== snake
SNAKE_CANARY_ROWS = 3
SNAKE_LS = (1, 2, 3, 4, 6, 7, 13, 70)
SNAKE_CS = (4, 32, 36)


@dataclass(frozen=True)
class SnakeCase:
	dt: str
	L: int
	C: int

	@property
	def id(self):
		return f"snake-{self.dt}-L{self.L}-C{self.C}"

	@property
	def group(self):
		return f"snake-{self.dt}"

	@property
	def seed(self):
		return zlib.crc32(self.id.encode())


SNAKE_CASES = [SnakeCase(dt, L, C) for dt in ("f32", "bf16") for L in SNAKE_LS for C in SNAKE_CS]


def kaiser_sinc_filter12():
	"""the 12-tap Kaiser-windowed sinc low-pass of Activation1d (cutoff 0.25, half width 0.3), f32, sum 1"""
	half = 6
	A = 2.285 * (half - 1) * math.pi * (4 * 0.3) + 7.95
	beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21) if A >= 21 else 0.0)
	win = torch.kaiser_window(12, periodic=False, beta=beta, dtype=torch.float64)
	t = torch.arange(-half, half, dtype=torch.float64) + 0.5
	f = 2 * 0.25 * win * torch.sinc(2 * 0.25 * t)
	return (f / f.sum()).float()


@functools.lru_cache(maxsize=4)
def snake_operands(c):
	"""x f32 [B L][C] within [-3, 3]; a in [1, 3], invb in [0.3, 1.2] f32 [C], as the kernel reads them; filt f32 [12]"""
	g = _gen(c.seed)
	x = torch.randn(B * c.L, c.C, generator=g).clamp(-3, 3)
	x[0] = x[0].sign() * 2.5                                       # one row per case that brings |up a| past pi whatever L is
	return {"x": x, "a": 1 + 2 * torch.rand(c.C, generator=g), "invb": 0.3 + 0.9 * torch.rand(c.C, generator=g), "filt": kaiser_sinc_filter12()}


def _snake_up(x, g, L):
	"""(up f64 [B][2L][C], sum|x g| of each) from x f64 [B][L][C]: the two phases of the definition"""
	q = torch.arange(L)
	up = torch.zeros(x.shape[0], 2 * L, x.shape[2], dtype=torch.float64)
	mag = torch.zeros_like(up)
	for j in range(6):
		e0, e1 = (q - 3 + j).clamp(0, L - 1), (q - 2 + j).clamp(0, L - 1)
		up[:, 0::2] += 2 * x[:, e0] * g[11 - 2 * j]
		up[:, 1::2] += 2 * x[:, e1] * g[10 - 2 * j]
		mag[:, 0::2] += 2 * (x[:, e0] * g[11 - 2 * j]).abs()
		mag[:, 1::2] += 2 * (x[:, e1] * g[10 - 2 * j]).abs()
	return up, mag


@functools.lru_cache(maxsize=4)
def snake_reference(c):
	"""dict: y f64 [B L][C], tol, and arg = up a (for the operand conditions)"""
	o = snake_operands(c)
	L = c.L
	x = o["x"].double().view(B, L, c.C)
	g, a, ib = o["filt"].double(), o["a"].double(), o["invb"].double()
	up, mag = _snake_up(x, g, L)
	dup = 1.01 * 8 * U * mag
	arg = up * a
	darg = a * dup + U * arg.abs()
	s = torch.sin(arg)
	ds = darg + (TRANS * s.abs() if c.dt == "f32" else SIN_FAST_ERR)
	s2 = s * s
	ds2 = 2.02 * s.abs() * ds + U * s2
	z = up + ib * s2
	dz = dup + ib * ds2 + U * ib * s2 + U * z.abs()
	y = torch.zeros(B, L, c.C, dtype=torch.float64)
	dy = torch.zeros_like(y)
	zmag = torch.zeros_like(y)
	t = torch.arange(L)
	for k in range(12):
		sidx = (2 * t + k - 5).clamp(0, 2 * L - 1)
		y += z[:, sidx] * g[k]
		dy += dz[:, sidx] * g[k].abs()
		zmag += (z[:, sidx] * g[k]).abs()
	tol = dy + 1.01 * 13 * U * zmag
	y, tol = y.view(B * L, c.C), tol.view(B * L, c.C)
	return {"y": y, "tol": tol + out_rounding(y, tol, c.dt), "arg": arg}


def snake_blank(c):
	return {"y": torch.full((B * c.L + SNAKE_CANARY_ROWS, c.C), NAN, dtype=torch.float64)}


def snake_check(c, got):
	r = snake_reference(c)
	rows = B * c.L
	_owed(f"{c.id}: y", got["y"][:rows])
	_untouched(f"{c.id}: y behind the rows", got["y"][rows:])
	return {"y f32" if c.dt == "f32" else "y rounded": _ratio(got["y"][:rows], r["y"], r["tol"])}


SNAKE_FAULTS = ("upsampled_signal_zero_padded", "k0_off_by_one", "k1_off_by_one", "odd_phase_shifted_by_a_tap", "times_2_missing", "clamp_across_the_batch_boundary")


def snake_fault_applies(c, fault):
	return True


def snake_emulate(c, fault=None):
	"""the image of one launch computed the way k_snake_aa computes it: one thread per row and four channels, 13 clamped rows in registers, 12 samples z[k]"""
	o = snake_operands(c)
	L, rows = c.L, B * c.L
	x, g, a, ib = o["x"], o["filt"], o["a"], o["invb"]
	row = torch.arange(rows)
	t = row % L
	base = row - t
	xr = []
	for j in range(13):
		if fault == "clamp_across_the_batch_boundary":
			xr.append(x[(row - 6 + j).clamp(0, rows - 1)])
		else:
			xr.append(x[base + (t - 6 + j).clamp(0, L - 1)])
	z = []
	for k in range(12):
		fl, odd = (k - 5) >> 1, (k - 5) & 1
		up = torch.zeros(rows, c.C)
		for j in range(6):
			up = up + xr[fl + 3 + odd + j] * g[11 - 2 * j if fault == "odd_phase_shifted_by_a_tap" else 11 - odd - 2 * j]
		if fault != "times_2_missing":
			up = up * 2
		s = torch.sin(up * a)
		z.append(up + ib * (s * s))
	z = torch.stack(z)                                                                    # [k][row][c]
	k0 = 5 - 2 * t + (1 if fault == "k0_off_by_one" else 0)
	k1 = 2 * L + 4 - 2 * t - (1 if fault == "k1_off_by_one" else 0)
	kk = torch.arange(12)[:, None]
	zlo = z[k0.clamp(0, 11), row]                                                          # z[k0] where 1 <= k0 <= 11 (z[0] is only ever "replaced" by itself)
	zhi = z[k1.clamp(0, 11), row]
	pad_lo, pad_hi = (kk < k0[None])[..., None], (kk > k1[None])[..., None]
	if fault == "upsampled_signal_zero_padded":
		zlo, zhi = torch.zeros_like(zlo), torch.zeros_like(zhi)
	z = torch.where(pad_lo, zlo[None], torch.where(pad_hi, zhi[None], z))
	acc = torch.zeros(rows, c.C)
	for k in range(12):
		acc = acc + z[k] * g[k]
	img = snake_blank(c)
	img["y"][:rows] = to_out(acc, c.dt)
	return img


CASES = {"lvc": LVC_CASES, "hifi": HIFI_CASES, "snake": SNAKE_CASES}
FAULTS = {"lvc": LVC_FAULTS, "hifi": HIFI_FAULTS, "snake": SNAKE_FAULTS}
FAULT_APPLIES = {"lvc": lvc_fault_applies, "hifi": hifi_fault_applies, "snake": snake_fault_applies}
EMULATE = {"lvc": lvc_emulate, "hifi": hifi_emulate, "snake": snake_emulate}
CHECK = {"lvc": lvc_check, "hifi": hifi_check, "snake": snake_check}
GROUPS = sorted({c.group for cs in CASES.values() for c in cs})
