"""Float64 references of the two attention operations of csrc/attn.hip, written from the definition, with a derived per-element error bound, the
operands and the case lists that tests/test_attn_ref.py (CPU) and tests/test_gpu_attn_forms.py (GPU) share, and a float32 emulation of the kernels'
arithmetic with switchable faults that shows the bound can see them.

Forward (k_attn_fwd), per sequence b, head h, query q < tlen[b]:
    out[q] = sum_k softmax_k(scale q.k + bias[h][clamp(k - q, -64, 64) + 64]) v_k     over k < tlen[b] (and k <= q when causal)
Decode (k_attn_decode), per candidate b, head h, one already scaled f32 query over the cache rows r in [start_b, min(pos + 1, max_ctx)):
    out = sum_r softmax_r(q.k_r) v_r,  row r read from the slice of b's line's first candidate when r < shared rows, else from b's own.

Operands are exactly representable in every kernel type (bf16-grid values, |x| >= 2^-10 or 0, times powers of two), the forward scale is 0.125 and
q * scale is exact in T: the reference sees the kernel's own inputs, and every product q k is exact in f32.

THE BOUND.  u = 2^-24 (f32 unit roundoff); s2, b2, v2 = score, bias, their sum in the log2 domain (the kernels use exp2); Mabs = max_k |v2| over a
query's valid keys (it bounds the running maximum m and |v2 - m| <= 2 Mabs); w_k = the softmax weights; mag_k = scale sum_d |q_d| |k_d|.
  score     dv_k = log2e 1e-5 mag_k                     f32 accumulation of the 64-term dot product (the constant of test_gpu_gemm_forms.py)
                 + u (|s2| + 3 |b2| + 4 Mabs)            LOG2E as an f32 constant, bias * LOG2E (constant + product), the fma's rounding, the rounding of
                                                          the difference to the running maximum (either softmax path: fma(s, LOG2E, b2) - m, or
                                                          fma(s, LOG2E, fl(b2 - m))); taken with |s2| <= log2e mag_k and |b2| <= log2e max |bias[h]|
  p_k       relative ln2 dv_k + 2u                       v_exp_f32 at one ulp (2^-23)
  P -> T    relative RP = 2^-8 (bf16), 2^-11 (f16), 0 (f32): the unit roundoff of T, see below; f16 also an absolute 2^-25 per key (half the
            subnormal spacing) in units of l, where l >= 1 after every rescale because the running maximum never exceeds the true one
  PV, l     relative EA = (T / 16 + 2 T / 64 + 24) u     one f32 rounding per MFMA (16 keys) and per deferred rescale of a 64-key tile for O; 16 + 2
                                                          sequential adds, one add and one rescale per tile for l
  out       |d out_d| <= 1.02 sum_k w_k [(e_k + RP + EA) |v_kd| + (e_k + EA) |out_d|] + F16 floor 2^-25 sum_k |v_kd|,   e_k = ln2 dv_k + 2u
            (first order in the weights' relative errors; they stay below 2^-6, so 1.02 covers the second order)
            + 3u |out_d|                                 1 / l and the product
            + half an ulp of T (or of e4m3, round to nearest even as pinned in test_gpu_fp8.py) at |out_d| + the bound so far
Decode is f32 throughout: dv = log2e (1e-5 + 2u) mag (the query times LOG2E is rounded per element) + 4u Mabs; the online softmax rescales at every
key: ES = ceil(n / 32) + 26 sequential steps (keys of one (wave, slot) in the narrowest variant, 8 + 16 merge steps, the division) of at most 6u
each (alpha's exp2 at one ulp, its argument, a product and a sum for O and for l); then the output rounding as above.

The issue that asked for this module gives the P rounding as "half an ulp relative, 2^-9 for bf16 and 2^-12 for f16".  Half an ulp relative to the
value is between 2^-9 and 2^-8 (bf16: 8 significand bits; the worst case is a value just above a power of two), so 2^-9 is the best case, not a
bound: the kernel's own arithmetic emulated in float32 (emulate_fwd below, no fault switched on) exceeds a bound built with 2^-9 / 2^-12
(up to 1.4 times it on the cases below; test_attn_ref.py prints the ratio per group), which is the test the issue itself sets for the bound.  RP is
therefore the unit roundoff.  No term of the bound is fitted to a measurement.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

U = 2.0 ** -24
LOG2E = 1.4426950408889634
LOG2E_F32 = float(torch.tensor(LOG2E, dtype=torch.float32))
LN2 = math.log(2.0)
NEG_BIG = -1e30
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# (significand bits, smallest normal exponent)
FMT = {"f32": (24, -126), "bf16": (8, -126), "f16": (11, -14), "e4m3": (4, -6)}
P_ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
P_ROUND_BEST_CASE = {"f32": 0.0, "bf16": 2.0 ** -9, "f16": 2.0 ** -12}      # the issue's figures (module docstring): reported, not asserted
SCALE = 0.125


def half_ulp(x, fmt):
	"""half the spacing of `fmt` at |x| (f64 tensor), subnormal range included"""
	bits, emin = FMT[fmt]
	_, e = torch.frexp(x.abs().clamp_min(2.0 ** -200))      # |x| = m 2^e, m in [0.5, 1)
	return torch.exp2((e - 1).clamp_min(emin).double() - bits)


def grid(t, mul=1.0):
	"""bf16 values without the tiny ones, times a power of two: exactly representable in bf16, f16 and f32"""
	t = t.bfloat16().float()
	return (torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t) * mul).double()


# ----------------------------------------------------------------------------------------------------------- forward: cases and operands
@dataclass
class Fwd:
	id: str
	dt: str
	nb: int
	H: int
	T: int
	mode: str = "plain"          # plain | causal | bias
	layout: str = "gpt"          # gpt: q|k|v, head_stride 64, ld = 3*64*H;  hm: head-major, head_stride 192, ld = 3*64*H + one fragment
	tlen: Optional[Tuple[int, ...]] = None
	forms: Tuple[int, ...] = (1, 2, 3, 4)   # explicit forms run besides form 0, where legal (legal_forms)
	expect0: int = 0             # the form that form 0 must give the bits of (the launcher's choice at this shape), 0: any
	f8: bool = False
	ramp: float = 0.0            # k[..., 0] = ramp * (key // 64), q[..., 0] = 8: the log2-domain maximum rises by ramp * log2e per 64-key tile
	qmul: float = 2.0            # scores ~ N(0, (qmul)^2): spread over a few units
	group: str = "edges"
	seed: int = 0

	@property
	def causal(self):
		return self.mode == "causal"

	def legal_forms(self):
		"""attn_fwd_form_refusal of csrc/attn.hip: 3 and 4 are non-causal; 4 takes no tlen, needs 256 % (nb H) == 0 and at most 9 tiles per workgroup"""
		G = 256 // (self.nb * self.H) if 256 % (self.nb * self.H) == 0 else 0
		bal = not self.causal and not self.tlen and G > 0 and -(-((self.T + 15) // 16) // G) <= 9
		return tuple(f for f in self.forms if not (self.causal and f == 3) and (f != 4 or bal))


def _fwd_cases():
	cs = []
	for T in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200):
		for mode in ("plain", "causal", "bias"):
			for dt in ("bf16", "f16", "f32"):
				for layout in ("gpt", "hm"):
					cs.append(Fwd(f"edge-{dt}-T{T}-{mode}-{layout}", dt, 2, 2, T, mode, layout))
	for dt in ("bf16", "f16", "f32"):      # far-left, far-right and band key tiles for some query tile; causal: the diagonal path
		cs.append(Fwd(f"paths-{dt}-T320-bias", dt, 2, 2, 320, "bias", group="paths"))
		cs.append(Fwd(f"paths-{dt}-T320-causal", dt, 2, 2, 320, "causal", group="paths"))
	for dt in ("bf16", "f16"):
		cs.append(Fwd(f"rescale-{dt}-T512-rise6", dt, 2, 2, 512, "plain", ramp=4.0, qmul=0.5, group="rescale"))
		cs.append(Fwd(f"rescale-{dt}-T512-rise9", dt, 2, 2, 512, "bias", ramp=6.0, qmul=0.5, group="rescale"))
		cs.append(Fwd(f"rescale-{dt}-T512-pm100", dt, 2, 2, 512, "plain", qmul=64.0, group="rescale"))
		cs.append(Fwd(f"rescale-{dt}-T512-pm100-causal", dt, 2, 2, 512, "causal", qmul=64.0, group="rescale"))
	for dt in ("bf16", "f16", "f32"):      # sequence 0: one row; sequence 2: query block 128.. is padding throughout
		cs.append(Fwd(f"ragged-{dt}-T200-bias", dt, 3, 2, 200, "bias", tlen=(1, 200, 77), group="ragged"))
		cs.append(Fwd(f"ragged-{dt}-T200-causal", dt, 3, 2, 200, "causal", tlen=(1, 200, 77), group="ragged"))
	bal = dict(expect0=4, group="balanced")
	cs.append(Fwd("bal-bf16-nb16-H16-T100-G1-7tiles", "bf16", 16, 16, 100, "bias", **bal))
	cs.append(Fwd("bal-f16-nb8-H16-T200-G2-7+6", "f16", 8, 16, 200, "bias", **bal))
	cs.append(Fwd("bal-bf16-nb8-H16-T277-G2-9+9", "bf16", 8, 16, 277, "plain", "hm", **bal))
	cs.append(Fwd("bal-bf16-nb2-H16-T1088-G8", "bf16", 2, 16, 1088, "bias", **bal))
	cs.append(Fwd("bal-f32-nb8-H16-T200-G2", "f32", 8, 16, 200, "bias", **bal))
	cs.append(Fwd("bal-bf16-nb1-H4-T6200-G64-noremap", "bf16", 1, 4, 6200, "bias", **bal))
	cs.append(Fwd("big-bf16-nb32-H16-T128", "bf16", 32, 16, 128, "bias", expect0=2, group="big"))
	cs.append(Fwd("big-bf16-nb32-H16-T130-causal", "bf16", 32, 16, 130, "causal", expect0=2, group="big"))
	cs.append(Fwd("big-f16-nb32-H16-T130", "f16", 32, 16, 130, "plain", expect0=2, group="big"))
	cs.append(Fwd("f8-bf16-T200-bias", "bf16", 2, 2, 200, "bias", f8=True, group="f8"))
	cs.append(Fwd("f8-bf16-nb8-H16-T200-bal", "bf16", 8, 16, 200, "bias", expect0=4, f8=True, group="f8"))
	cs.append(Fwd("f8-bf16-ragged-T200-causal", "bf16", 3, 2, 200, "causal", tlen=(1, 200, 77), f8=True, group="f8"))
	for i, c in enumerate(cs):
		c.seed = 5000 + i
	assert len({c.id for c in cs}) == len(cs)
	return cs


FWD_CASES = _fwd_cases()


def fwd_operands(c):
	"""q, k, v f64 [nb][H][T][64] (finite everywhere: what lies past tlen[b] must not matter) and the bias f64 [H][129] or None"""
	g = torch.Generator().manual_seed(c.seed)
	shp = (c.nb, c.H, c.T, 64)
	q = grid(torch.randn(shp, generator=g), c.qmul)
	k = grid(torch.randn(shp, generator=g))
	v = grid(torch.randn(shp, generator=g))
	if c.ramp:
		q[..., 0] = 8.0
		k[..., 0] = (c.ramp * (torch.arange(c.T) // 64)).double()[None, None, :]
	for b in range(c.nb):      # the last valid key matters to the last query (the only one that sees it in a causal case): same signs, a dominant score
		TL = c.tlen[b] if c.tlen else c.T
		k[b, :, TL - 1] = k[b, :, TL - 1].abs() * torch.where(q[b, :, TL - 1] < 0, -1.0, 1.0)
	bias = None
	if c.mode == "bias":      # distinct values of magnitude 1 .. 3, f32 (the kernel's bias table is f32)
		mag = 1.0 + 2.0 * torch.rand((c.H, 129), generator=g)
		sign = torch.where(torch.rand((c.H, 129), generator=g) < 0.5, -1.0, 1.0)
		bias = (mag * sign).float().double()
	return q, k, v, bias


def fwd_reference(c, q, k, v, bias, p_round=None, chunk=512):
	"""(ref, tol) f64 [nb][T][H*64]; rows >= tlen[b] are NaN in both"""
	RP = P_ROUND[c.dt] if p_round is None else p_round[c.dt]
	EA = (c.T / 16 + 2 * c.T / 64 + 24) * U
	ref = torch.full((c.nb, c.T, c.H * 64), float("nan"), dtype=torch.float64)
	tol = torch.full_like(ref, float("nan"))
	for b in range(c.nb):
		TL = c.tlen[b] if c.tlen else c.T
		kk, vv = k[b, :, :TL], v[b, :, :TL]      # [H][TL][64]
		ki = torch.arange(TL)
		bmax = bias.abs().amax(-1)[:, None, None] if bias is not None else 0.0
		for q0 in range(0, TL, chunk):
			q1 = min(q0 + chunk, TL)
			qq = q[b, :, q0:q1]
			qi = torch.arange(q0, q1)
			s = SCALE * (qq @ kk.transpose(1, 2))      # [H][nq][TL]
			mag = SCALE * (qq.abs() @ kk.abs().transpose(1, 2))
			if bias is not None:
				rel = (ki[None, :] - qi[:, None]).clamp(-64, 64) + 64
				bb = bias[:, rel]
			z = s.add_(bb) if bias is not None else s
			if c.causal:
				z.masked_fill_((ki[None, :] > qi[:, None])[None], float("-inf"))
			w = torch.softmax(z, dim=-1)
			out = w @ vv      # [H][nq][64]
			mabs = z.masked_fill_(torch.isinf(z), 0.0).abs_().amax(-1, keepdim=True) * LOG2E
			# e_k = ln2 dv_k + 2u with |s2| <= log2e mag and |b2| <= log2e max|bias[h]|: a multiple of mag_k plus a per-query constant
			e0 = LN2 * U * (3 * LOG2E * bmax + 4 * mabs) + 2 * U
			wv, wm = w @ vv.abs(), LN2 * LOG2E * (1e-5 + U) * mag.mul_(w)
			t = 1.02 * (wm @ vv.abs() + (e0 + RP + EA) * wv + (wm.sum(-1, keepdim=True) + e0 + EA) * out.abs())
			if c.dt == "f16":
				t = t + 2.0 ** -25 * vv.abs().sum(1, keepdim=True)
			t = t + 3 * U * out.abs()
			t = t + half_ulp(out.abs() + t, "e4m3" if c.f8 else c.dt)
			ref[b, q0:q1] = out.permute(1, 0, 2).reshape(q1 - q0, c.H * 64)
			tol[b, q0:q1] = t.permute(1, 0, 2).reshape(q1 - q0, c.H * 64)
	return ref, tol


def _to_t(x, dt):
	return x.to(TDT[dt]).float()


def emulate_fwd(c, q, k, v, bias, fault=None):
	"""The kernel's arithmetic in float32 torch, in its tile order: 64-key tiles, log2-domain scores, the running maximum kept until a tile exceeds it by more
	than 8 for some query of the 16-query tile, P rounded to T before the PV product, l summed from the unrounded P.  `fault`: None or one of
	bias_off_by_one, bias_unsaturated, drop_last_key, admit_first_pad, causal_strict.  Returns f64 [nb][T][H*64], NaN rows past tlen[b]."""
	out = torch.full((c.nb, c.T, c.H * 64), float("nan"), dtype=torch.float64)
	l2e = torch.tensor(LOG2E_F32, dtype=torch.float32)
	for b in range(c.nb):
		TL = c.tlen[b] if c.tlen else c.T
		nq = (TL + 15) // 16 * 16
		qq = _to_t((q[b, :, :TL] * SCALE).float(), c.dt)      # [H][TL][64]
		qq = torch.cat([qq, qq[:, -1:].expand(-1, nq - TL, -1)], 1)      # clamped reads of the last query tile
		qi = torch.arange(nq)
		kend = TL - 1 if fault == "drop_last_key" else (min(TL + 1, c.T) if fault == "admit_first_pad" else TL)
		m = torch.full((c.H, nq), NEG_BIG, dtype=torch.float32)
		l = torch.zeros(c.H, nq, dtype=torch.float32)
		o = torch.zeros(c.H, nq, 64, dtype=torch.float32)
		for k0 in range(0, (TL + 63) // 64 * 64, 64):
			ki = torch.arange(k0, k0 + 64)
			kc = ki.clamp_max(max(kend, TL) - 1)
			kt, vt = k[b, :, kc].float(), v[b, :, kc].float()      # [H][64][64]
			s = qq @ kt.transpose(1, 2)      # [H][nq][64]
			if bias is not None:
				d = ki[None, :] - qi[:, None] + (1 if fault == "bias_off_by_one" else 0)
				bt = (bias.float() * l2e)[:, d.clamp(-64, 64) + 64]
				if fault == "bias_unsaturated":      # the table read linearly continued: the end values' slope instead of the end values
					bf = bias.float() * l2e
					over = (d.abs() - 64).clamp_min(0).float()
					bt = bt + over[None] * torch.where(d > 0, (bf[:, 128] - bf[:, 127])[:, None, None], (bf[:, 0] - bf[:, 1])[:, None, None])
				val = s * l2e + bt
			else:
				val = s * l2e
			mask = ki[None, :] >= kend
			if c.causal:
				mask = mask | ((ki[None, :] >= qi[:, None]) if fault == "causal_strict" else (ki[None, :] > qi[:, None]))
			val = val.masked_fill(mask[None], NEG_BIG)
			tmax = val.amax(-1)      # [H][nq]
			need = (tmax > m + 8.0).view(c.H, nq // 16, 16).any(-1, keepdim=True).expand(-1, -1, 16).reshape(c.H, nq)
			m_new = torch.where(need, torch.maximum(m, tmax), m)
			alpha = torch.exp2(m - m_new)
			m = m_new
			l = l * alpha
			o = o * alpha[..., None]
			p = torch.exp2(val - m[..., None])
			l = l + p.sum(-1)
			o = o + _to_t(p, c.dt) @ vt
		r = o * (1.0 / l)[..., None]
		r = r.to(torch.float8_e4m3fn).double() if c.f8 else _to_t(r, c.dt).double()
		out[b, :TL] = r[:, :TL].permute(1, 0, 2).reshape(TL, c.H * 64)
	return out


FWD_FAULTS = ("bias_off_by_one", "bias_unsaturated", "drop_last_key", "admit_first_pad", "causal_strict")


def fwd_fault_applies(c, fault):
	"""whether the fault changes the definition's result at all: one key gets weight 1 whatever its score; a causal mask hides the first padding key"""
	if fault in ("bias_off_by_one", "bias_unsaturated"):
		return c.mode == "bias" and (c.T >= 2 if fault == "bias_off_by_one" else c.T > 66)
	if fault == "admit_first_pad":
		return c.tlen is not None and any(t < c.T for t in c.tlen) and not c.causal
	if fault == "causal_strict":
		return c.causal and c.T >= 2
	return fault == "drop_last_key" and c.T >= 2


# ----------------------------------------------------------------------------------------------------------- decode: cases and operands
DEC_SHAPE = {0: {"bf16": (16, 3), "f16": (16, 3), "f32": (8, 6)}, 1: {"bf16": (4, 4)}, 2: {"bf16": (8, 6)}}      # variant -> dtype -> (waves, unroll)


@dataclass
class Dec:
	id: str
	dt: str
	B: int
	H: int
	max_ctx: int
	pos: int                     # d_pos[0]: last valid row
	shared: int = 0              # d_pos[1]
	shared_rows: int = 0
	variants: Tuple[int, ...] = (0,)
	lines: Optional[Tuple[Tuple[int, int], ...]] = None      # row_info as (candidates, start) per line
	group: str = "keys"
	seed: int = 0

	def row_info(self):
		"""[(start, first candidate of the line)] per candidate, or None"""
		if not self.lines:
			return None
		ri, first = [], 0
		for ncand, start in self.lines:
			ri += [(start, first)] * ncand
			first += ncand
		assert len(ri) == self.B
		return ri


def _dec_cases():
	cs = []
	for dt, variants in (("bf16", (0, 1, 2)), ("f16", (0,)), ("f32", (0,))):
		for var in variants:
			NW, UN = DEC_SHAPE[var][dt]
			for n in sorted({1, 7, 8, 9, 8 * NW - 1, 8 * NW + 1, 8 * NW * UN - 1, 8 * NW * UN, 8 * NW * UN + 1, 2 * 8 * NW * UN + 1}):
				cs.append(Dec(f"keys-{dt}-v{var}-n{n}", dt, 2, 16, n + 3, n - 1, variants=(var,)))
	for dt in ("bf16", "f32"):      # pos + 1 > max_ctx: the kernel clamps to the cache
		cs.append(Dec(f"clamp-{dt}-ctx40-pos44", dt, 2, 16, 40, 44, variants=(0, 1, 2) if dt == "bf16" else (0,)))
	for B in (1, 16, 17, 33):
		cs.append(Dec(f"shape-bf16-B{B}", "bf16", B, 16, 60, 52, variants=(0, 1, 2), group="shapes"))
	cs.append(Dec("shape-f16-B17", "f16", 17, 16, 60, 52, group="shapes"))
	cs.append(Dec("shape-f32-B17", "f32", 17, 16, 60, 52, group="shapes"))
	for sh in (0, 5, 52):
		cs.append(Dec(f"shared-bf16-B5-rows{sh}", "bf16", 5, 16, 60, 52, sh, 1, variants=(0, 1, 2), group="shared"))
	cs.append(Dec("shared-f32-B5-rows5", "f32", 5, 16, 60, 52, 5, 1, group="shared"))
	cs.append(Dec("shared-bf16-B5-rows5-off", "bf16", 5, 16, 60, 52, 5, 0, group="shared"))      # shared_rows = 0: d_pos[1] is ignored
	# two lines, prefixes right-aligned: line 0 (3 candidates) starts at row 0, line 1 (2 candidates) at row 7; shared rows end at 20
	cs.append(Dec("lines-bf16-3+2-start0+7-shared20", "bf16", 5, 16, 450, 420, 20, 1, variants=(0, 1, 2), lines=((3, 0), (2, 7)), group="lines"))
	cs.append(Dec("lines-f16-2+3-start9+0-noshared", "f16", 5, 16, 60, 52, 0, 0, lines=((2, 9), (3, 0)), group="lines"))
	cs.append(Dec("lines-f32-3+2-start0+7-shared20", "f32", 5, 16, 60, 52, 20, 1, lines=((3, 0), (2, 7)), group="lines"))
	for i, c in enumerate(cs):
		c.seed = 9000 + i
	assert len({c.id for c in cs}) == len(cs)
	return cs


DEC_CASES = _dec_cases()


def dec_operands(c):
	"""q f64 [B][H][64] (f32 values), K and V caches f64 [B][H][max_ctx][64], finite everywhere.  With shared rows every candidate holds its own
	(different) values there: only the owner's may be read."""
	g = torch.Generator().manual_seed(c.seed)
	q = (torch.randn((c.B, c.H, 64), generator=g) * 0.25).float().double()      # scores ~ N(0, 2^2)
	kc = grid(torch.randn((c.B, c.H, c.max_ctx, 64), generator=g))
	vc = grid(torch.randn((c.B, c.H, c.max_ctx, 64), generator=g))
	return q, kc, vc


def dec_rows(c, b, fault=None):
	"""(cache rows, candidate whose slice each row is read from) for candidate b"""
	ri = c.row_info()
	start, first = ri[b] if ri else (0, 0)
	if fault == "start_ignored":
		start = 0
	n_end = min(c.pos + 1, c.max_ctx)
	rows = torch.arange(start, n_end)
	sh = c.shared if c.shared_rows else 0
	src = torch.where(rows < sh, first, b)
	if fault == "shared_from_own":
		src = torch.full_like(rows, b)
	return rows, src


def dec_reference(c, q, kc, vc):
	"""(ref, tol) f64 [B][H*64]"""
	ref = torch.zeros(c.B, c.H * 64, dtype=torch.float64)
	tol = torch.zeros_like(ref)
	for b in range(c.B):
		rows, src = dec_rows(c, b)
		kk, vv = kc[src, :, rows].transpose(0, 1), vc[src, :, rows].transpose(0, 1)      # [H][n][64]
		n = rows.numel()
		s = (kk @ q[b][:, :, None])[..., 0]      # [H][n]
		mag = (kk.abs() @ q[b].abs()[:, :, None])[..., 0]
		w = torch.softmax(s, dim=-1)
		out = (w[:, None, :] @ vv)[:, 0]      # [H][64]
		mabs = (s * LOG2E).abs().amax(-1, keepdim=True)
		e = LN2 * (LOG2E * (1e-5 + 2 * U) * mag + 4 * U * mabs) + 2 * U
		ES = (math.ceil(n / 32) + 26) * 6 * U
		t = 1.02 * (((e + ES) * w)[:, None, :] @ vv.abs())[:, 0] + 1.02 * ((e + ES) * w).sum(-1, keepdim=True) * out.abs()
		t = t + half_ulp(out.abs() + t, c.dt)
		ref[b], tol[b] = out.reshape(-1), t.reshape(-1)
	return ref, tol


def emulate_dec(c, q, kc, vc, variant=0, fault=None):
	"""The kernel's arithmetic in float32: keys dealt in groups of 8 round-robin to NW waves, an online softmax per (wave, slot) that rescales at every key, the
	two-level merge.  `fault`: None, skip_group (one 8-key group never read), shared_from_own, start_ignored.  Returns f64 [B][H*64]."""
	NW, _ = DEC_SHAPE[variant][c.dt]
	l2e = torch.tensor(LOG2E_F32, dtype=torch.float32)
	res = torch.zeros(c.B, c.H * 64, dtype=torch.float64)
	for b in range(c.B):
		rows, src = dec_rows(c, b, fault)
		kk, vv = kc[src, :, rows].transpose(0, 1).float(), vc[src, :, rows].transpose(0, 1).float()      # [H][n][64]
		n = rows.numel()
		q2 = q[b].float() * l2e
		s = (kk @ q2[:, :, None])[..., 0]      # [H][n]
		NP = NW * 8
		idx = torch.arange(n)
		part = ((idx // 8) % NW) * 8 + idx % 8      # (wave, slot) of key idx
		keep = torch.ones(n, dtype=torch.bool)
		if fault == "skip_group":
			gsk = (n // 8) // 2      # a middle group
			keep = (idx // 8) != gsk
		m = torch.full((c.H, NP), NEG_BIG, dtype=torch.float32)
		l = torch.zeros(c.H, NP, dtype=torch.float32)
		acc = torch.zeros(c.H, NP, 64, dtype=torch.float32)
		for i in range(n):
			if not keep[i]:
				continue
			pi = int(part[i])
			m_new = torch.maximum(m[:, pi], s[:, i])
			alpha, pv = torch.exp2(m[:, pi] - m_new), torch.exp2(s[:, i] - m_new)
			l[:, pi] = l[:, pi] * alpha + pv
			acc[:, pi] = acc[:, pi] * alpha[:, None] + pv[:, None] * vv[:, i]
			m[:, pi] = m_new
		mw = m.view(c.H, NW, 8)
		mn = mw.amax(-1)      # [H][NW]
		a = torch.exp2(mw - mn[..., None])
		lt = (l.view(c.H, NW, 8) * a).sum(-1)
		ot = (acc.view(c.H, NW, 8, 64) * a[..., None]).sum(2)
		mn2 = mn.amax(-1)
		a2 = torch.exp2(mn - mn2[:, None])
		lt2 = (lt * a2).sum(-1)
		ot2 = (ot * a2[..., None]).sum(1)
		res[b] = _to_t(ot2 / lt2[:, None], c.dt).double().reshape(-1)
	return res


DEC_FAULTS = ("skip_group", "shared_from_own", "start_ignored")


def dec_fault_applies(c, fault):
	if fault == "shared_from_own":
		return bool(c.shared_rows and c.shared > 0 and c.B > 1)
	if fault == "start_ignored":
		return bool(c.lines) and any(s > 0 for _, s in c.lines)
	return min(c.pos + 1, c.max_ctx) >= 8      # skip_group: at least one whole group


def worst_ratio(got, ref, tol):
	"""max |got - ref| / tol over the elements the reference owes; a NaN where a number is owed counts as infinite"""
	owed = ~torch.isnan(ref)
	r = ((got - ref).abs() / tol)[owed]
	if r.numel() == 0:
		return 0.0
	return float("inf") if torch.isnan(r).any() else r.max().item()
