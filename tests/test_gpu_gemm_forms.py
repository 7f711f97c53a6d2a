"""Every form of the dense GEMM (csrc/gemm.hip) through `ttk_gemm` against a float64 reference of the same operands: each tile (64 x 64, 128 x 64,
128 x 128, 256 x 128 with the half-tile loop), each k-loop form (hand-ordered stream, half-tile stream, compiler-ordered ring, the k = 3 conv's
shared image, the mixed grid), each role, and each epilogue form (scale, bias, gelu_new / SiLU, residual -- also aliasing C -- 16-bit output,
transposed output, ldc > N, guarded edge tiles) with the fused GroupNorm32 statistics.

The operands are exactly representable and every product is exact in f32, so the kernel differs from the f64 reference by its f32 accumulation
(1e-5 of sum|a||w|; fp8: 2e-4, see test_gpu_gemm.py) plus one f32 rounding per epilogue operation (scale, bias, residual), the activation's
own error (2e-6 of |z|) on top of the pre-activation's error times |f'(z)|, and half an output ulp for 16-bit output.  C's padding columns, a
block of rows past M and the statistics buffer start as NaN: every value the kernel owes must be written, and nothing else.

TTK_GEMM_TILE and TTK_GEMM_ROLE are read once per process, so each configuration runs every case in a fresh child process (one after another; a
child that dies or hangs fails the module at once).  The code says that every tiling of the same operands adds its products in the same k order
(gemm.hip at the wide-tile rule, launch_gemm's seg_inner): every configuration must give the auto configuration's bits."""
import ctypes as C
import hashlib
import math
import os
import pickle
import subprocess
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": 0, "bf16": 1, "fp8": 3, "f16": 4}
CANARY_ROWS = 64
FP8_SCALE = 2.0 ** -7


@dataclass
class Case:
	id: str                   # dtype-shape-form-tile: the tile / loop the case is meant to reach under the auto configuration
	dt: str
	M: int
	N: int
	K: int
	shifts: Tuple[int, ...] = (0,)
	distinct_a: bool = False  # one A tensor per segment (else every segment reads the same tensor)
	concat: bool = False      # segments side by side in W (ldw = nseg * K, w_off = j * K) instead of stacked [Npad][K] matrices
	rpb: int = 0
	act: int = 0
	bias: bool = True
	residual: Optional[str] = None    # None, "sep" or "alias" (residual == C)
	out_f32: bool = True
	transpose: bool = False
	ldc_extra: int = 0
	npad_extra: int = 0       # W rows beyond round_up(N, 128)
	gn_T: int = 0
	seed: int = 0

	@property
	def nseg(self):
		return len(self.shifts)


def roles(dt, M, T, tile):
	"""the four DDIM roles' exact signatures at model_channels = 1024 (gemm_role_of_unmasked): K = lda = ldw = 1024, bias, no activation"""
	b = M // T
	return [Case(f"{dt}-M{M}-in1x1-gnT{T}-{tile}", dt, M, 1024, 1024, gn_T=T),
			Case(f"{dt}-M{M}-conv3res-alias-gnT{T}-b{b}-{tile}", dt, M, 1024, 1024, shifts=(-1, 0, 1), rpb=T, residual="alias", gn_T=T),
			Case(f"{dt}-M{M}-qkv-out16-{tile}", dt, M, 3072, 1024, out_f32=False),
			Case(f"{dt}-M{M}-projres-gnT{T}-{tile}", dt, M, 1024, 1024, residual="sep", gn_T=T)]


CASES = [
	# the 64 x 64 tile (tiny M), every K of the ring, guarded rows and columns
	Case("bf16-M1-N128-K64-t2", "bf16", 1, 128, 64),
	Case("f16-M63-N192w256-K128-gelu-ldc200-t2-guardcols", "f16", 63, 192, 128, act=1, ldc_extra=8),
	Case("bf16-M65-N128-K192-silu-nobias-t2", "bf16", 65, 128, 192, act=2, bias=False),
	Case("f32-M127-N1024-K256-t2", "f32", 127, 1024, 256),
	Case("bf16-M129-N3072-K64-out16-t2", "bf16", 129, 3072, 64, out_f32=False),
	Case("f16-M255-N3072-K128-t2", "f16", 255, 3072, 128, residual="sep"),
	# 128 x 64 (hand-ordered stream, 64 x 32 wave block)
	Case("bf16-M257-N3072-K1024-gelu-t1", "bf16", 257, 3072, 1024, act=1),
	Case("bf16-M2000-N1024-K1024-res-t1-guardrows", "bf16", 2000, 1024, 1024, residual="sep"),
	Case("f16-M2000-N1024-K192-silu-ldc1040-t1", "f16", 2000, 1024, 192, act=2, ldc_extra=16),
	Case("bf16-M2432-N1024-K64-out16-t1", "bf16", 2432, 1024, 64, out_f32=False),
	# 128 x 128 (hand-ordered stream, 64 x 32 wave block)
	Case("bf16-M2816-N3072-K64-t0", "bf16", 2816, 3072, 64),
	Case("f16-M4096-N1024-K128-res-alias-ldc1088-t0", "f16", 4096, 1024, 128, residual="alias", ldc_extra=64),
	# 256 x 128: half-tile hand-ordered loop when the k-loop is longer than the ring (LONGK), compiler-ordered ring when it is not
	Case("bf16-M4352-N1024-K256-t8-longk", "bf16", 4352, 1024, 256),
	Case("f16-M4352-N1024-K192-t8-ring3", "f16", 4352, 1024, 192, act=1),
	Case("bf16-M1281-N3072-K1024-gelu-out16-t8-longk-guardrows", "bf16", 1281, 3072, 1024, act=1, out_f32=False),
	# f32 and fp8 operands (compiler-ordered loops)
	Case("f32-M4352-N1024-K64-silu-t0", "f32", 4352, 1024, 64, act=2),
	Case("f32-M600-N192w256-K96-res-t2", "f32", 600, 192, 96, residual="sep"),
	Case("fp8-M2000-N1024-K1024-scale-t1", "fp8", 2000, 1024, 1024),
	Case("fp8-M4352-N1024-K256-scale-out16-t8", "fp8", 4352, 1024, 256, out_f32=False),
	Case("fp8-M65-N192w256-K128-scale-gelu-t2", "fp8", 65, 192, 128, act=1),
	# k = 3 'same' convolutions (taps -1 / 0 / +1 of one tensor, tap-inner order), zeros outside each batch element
	Case("bf16-conv3-rpb1000-b2-N1024-K1024-res-t1-edgeintile", "bf16", 2000, 1024, 1024, shifts=(-1, 0, 1), rpb=1000, residual="sep"),
	Case("f16-conv3-rpb1088-b2-N128-K128-t2", "f16", 2176, 128, 128, shifts=(-1, 0, 1), rpb=1088, act=2),
	Case("f32-conv3-rpb100-b3-N128-K64-silu-t2", "f32", 300, 128, 64, shifts=(-1, 0, 1), rpb=100, act=2),
	Case("bf16-conv3-rpb1088-b4-N1024-K256-t8-longk", "bf16", 4352, 1024, 256, shifts=(-1, 0, 1), rpb=1088),
	# vocoder-like: distinct A per segment, dilated shifts; a two-segment channel concatenation
	Case("bf16-5seg-dil3-rpb500-b2-N128-K128-t2", "bf16", 1000, 128, 128, shifts=(-6, -3, 0, 3, 6), distinct_a=True, rpb=500, act=2),
	Case("f32-11seg-dil5-rpb300-b2-N256-K64-t2", "f32", 600, 256, 64, shifts=tuple(5 * (j - 5) for j in range(11)), distinct_a=True, rpb=300),
	Case("bf16-concat2-N1024-K512-t1", "bf16", 2176, 1024, 512, shifts=(0, 0), distinct_a=True, concat=True),
	# transposed output [b][N][rows_per_batch]
	Case("bf16-conv3-transpose-rpb1088-b2-N100w128-K1024-t2", "bf16", 2176, 100, 1024, shifts=(-1, 0, 1), rpb=1088, transpose=True),
	Case("f32-transpose-rpb300-b2-N256-K64-t2", "f32", 600, 256, 64, rpb=300, transpose=True),
	# the roles: t128 == 256 keeps 128 x 128 (the hand-ordered GR_CONV3_RES kernel), M = 2176 / 2432 the mixed grid (QKV: 256 x 128), M = 4352 256 x 128
	*roles("bf16", 4096, 2048, "t0"),
	*roles("f16", 4096, 2048, "t0"),
	*roles("bf16", 2176, 1088, "mixed"),
	Case("bf16-M2432-conv3res-alias-gnT1216-b2-mixed48", "bf16", 2432, 1024, 1024, shifts=(-1, 0, 1), rpb=1216, residual="alias", gn_T=1216),
	Case("bf16-M4352-conv3res-alias-gnT2176-b2-t8", "bf16", 4352, 1024, 1024, shifts=(-1, 0, 1), rpb=2176, residual="alias", gn_T=2176),
	Case("f16-M4352-conv3res-alias-gnT2176-b2-t8", "f16", 4352, 1024, 1024, shifts=(-1, 0, 1), rpb=2176, residual="alias", gn_T=2176),
	Case("bf16-M4352-projres-alias-gnT2176-t8", "bf16", 4352, 1024, 1024, residual="alias", gn_T=2176),
	Case("fp8-M2176-conv3res-alias-gnT1088-b2-scale-mixed", "fp8", 2176, 1024, 1024, shifts=(-1, 0, 1), rpb=1088, residual="alias", gn_T=1088),
	Case("fp8-M4352-conv3res-alias-gnT2176-b2-scale-t8", "fp8", 4352, 1024, 1024, shifts=(-1, 0, 1), rpb=2176, residual="alias", gn_T=2176),
	Case("fp8-M4352-projres-gnT2176-scale-t8", "fp8", 4352, 1024, 1024, residual="sep", gn_T=2176),
	# GroupNorm statistics on the generic kernel (no role: K = 256)
	Case("bf16-M4096-N1024-K256-gnT1024-t0", "bf16", 4096, 1024, 256, gn_T=1024),
]
for _i, _c in enumerate(CASES):
	_c.seed = 1000 + _i
assert len({c.id for c in CASES}) == len(CASES)

# configuration -> environment of the child; "roles, no mixed grid" runs the statistics roles of M = 2176 / 2432 on plain 128 x 64 tiles (the shared-image conv)
CONFIGS = {"auto": {}, "tile0": {"TTK_GEMM_TILE": "0"}, "tile1": {"TTK_GEMM_TILE": "1"}, "tile2": {"TTK_GEMM_TILE": "2"}, "tile8": {"TTK_GEMM_TILE": "8"},
		   "roles": {"TTK_GEMM_ROLE": "1"}, "roles-nomixed": {"TTK_GEMM_ROLE": "1", "TTK_GEMM_MIXED": "0"}, "noroles": {"TTK_GEMM_ROLE": "0"}}
CHILD_TIMEOUT = 300


def round_up(x, m):
	return (x + m - 1) // m * m


def pick_tile(M, N):      # csrc/gemm.hip pick_tile
	t128 = ((M + 127) // 128) * ((N + 127) // 128)
	return 0 if t128 >= 256 else (1 if ((M + 127) // 128) * ((N + 63) // 64) >= 128 else 2)


def gn_valid(c, config):
	"""ttk_gemm accepts gn_part iff gemm_fuses_gn_stats (the test want_stats applies in diff.hip)"""
	if CONFIGS[config].get("TTK_GEMM_TILE") == "2":
		return False
	return c.N == 1024 and c.gn_T % 64 == 0 and c.M % 64 == 0 and pick_tile(c.M, c.N) != 2


# ----------------------------------------------------------------------------------------------------------- operands (CPU, deterministic per case)
def operands(c):
	"""A list (one per distinct tensor), W [nmat][Npad][K] (or [Npad][nseg K] for a concatenation), bias, residual -- as float64 holding the values the
	kernel sees, and the kernel-typed tensors"""
	g = torch.Generator().manual_seed(c.seed)
	npad = round_up(c.N, 128) + c.npad_extra
	na = c.nseg if c.distinct_a else 1
	if c.dt == "fp8":
		A = [(torch.randn(c.M, c.K, generator=g) * 1.5).to(torch.float8_e4m3fn) for _ in range(na)]
		Wm = [(torch.randn(npad, c.K, generator=g) * 20).to(torch.float8_e4m3fn) for _ in range(c.nseg)]
	else:
		def q(t):      # bf16 values without the tiny ones: exactly representable in bf16, f16 and f32, products exact in f32
			t = t.bfloat16().float()
			return torch.where(t.abs() < 2.0 ** -10, torch.zeros_like(t), t)
		tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c.dt]
		A = [q(torch.randn(c.M, c.K, generator=g)).to(tdt) for _ in range(na)]
		Wm = [q(torch.randn(npad, c.K, generator=g) * 0.5).to(tdt) for _ in range(c.nseg)]
	bias = torch.randn(c.N, generator=g) if c.bias else None
	res = torch.randn(c.M, c.N, generator=g) * 4 if c.residual else None
	return A, Wm, bias, res


def shifted(a, shift, rpb):
	"""row m of the result = row m + shift of a when that stays inside m's batch element of rpb rows, else zeros"""
	if shift == 0:
		return a
	M = a.shape[0]
	out = torch.zeros_like(a)
	t = torch.arange(M) % rpb
	src = torch.arange(M) + shift
	ok = (t + shift >= 0) & (t + shift < rpb) & (src < M)
	out[ok] = a[src[ok]]
	return out


def act_f64(z, act):
	if act == 1:      # gelu_new
		u = math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)
		th = torch.tanh(u)
		f = 0.5 * z * (1 + th)
		df = 0.5 * (1 + th) + 0.5 * z * (1 - th ** 2) * math.sqrt(2.0 / math.pi) * (1 + 3 * 0.044715 * z ** 2)
		return f, df
	if act == 2:      # SiLU
		s = torch.sigmoid(z)
		return z * s, s * (1 + z * (1 - s))
	return z, torch.ones_like(z)


def reference(c):
	"""(ref f64 [M][N], tol f64 [M][N]) of the f32 value the epilogue produces before any 16-bit conversion, and the conversion's tolerance"""
	A, Wm, bias, res = operands(c)
	acc = torch.zeros(c.M, c.N, dtype=torch.float64)
	mag = torch.zeros(c.M, c.N, dtype=torch.float64)
	for j, s in enumerate(c.shifts):
		a = shifted(A[j if c.distinct_a else 0].double(), s, c.rpb)
		w = Wm[j][:c.N].double()
		acc += a @ w.t()
		mag += a.abs() @ w.abs().t()
	eps = 2.0 ** -24
	scale = FP8_SCALE if c.dt == "fp8" else 1.0
	tol = (2e-4 if c.dt == "fp8" else 1e-5) * mag * scale
	v = acc * scale
	if c.dt == "fp8":
		tol = tol + eps * v.abs()
	if bias is not None:
		v = v + bias.double()
		tol = tol + eps * v.abs()
	if c.act:
		f, df = act_f64(v, c.act)
		tol = df.abs() * tol * 1.01 + 2e-6 * v.abs()
		v = f
	if res is not None:
		v = v + res.double()
		tol = tol + eps * v.abs()
	if not c.out_f32:
		tol = tol + (2.0 ** -8 if c.dt in ("bf16", "fp8") else 2.0 ** -11) * (v.abs() + tol) + (2.0 ** -25 if c.dt == "f16" else 0.0)
	return v, tol


# ----------------------------------------------------------------------------------------------------------- the child: every case under one configuration
def digest(*ts):
	h = hashlib.sha256()
	for t in ts:
		if t is not None:
			h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
	return h.hexdigest()


def run_case(lib, _lib, c, dev):
	A, Wm, bias, res = operands(c)
	npad = Wm[0].shape[0]
	Ad = [a.to(dev).contiguous() for a in A]
	if c.concat:
		Wd = torch.cat(Wm, dim=1).to(dev).contiguous()
		ldw, w_off = c.nseg * c.K, [j * c.K for j in range(c.nseg)]
	else:
		Wd = torch.stack(Wm).to(dev).contiguous()
		ldw, w_off = c.K, [j * npad * c.K for j in range(c.nseg)]
	out_dt = torch.float32 if c.out_f32 else (torch.float16 if c.dt == "f16" else torch.bfloat16)
	ldc = c.N + c.ldc_extra
	if c.transpose:
		Cbuf = torch.full(((c.M + CANARY_ROWS) * c.N,), float("nan"), device=dev, dtype=out_dt)
	else:
		Cbuf = torch.full((c.M + CANARY_ROWS, ldc), float("nan"), device=dev, dtype=out_dt)
	resd = None
	if c.residual == "alias":
		Cbuf[:c.M, :c.N] = res.to(dev)
	elif c.residual == "sep":
		resd = res.to(dev).contiguous()
	biasd = bias.to(dev) if bias is not None else None
	part = None
	if c.gn_T:
		nb, nch = (c.M + c.gn_T - 1) // c.gn_T, c.gn_T // 64
		part = torch.full((nb * 32 * nch * 3 + 1024,), float("nan"), device=dev)
	d = _lib.GemmDesc()
	d.nseg = c.nseg
	for j, s in enumerate(c.shifts):
		d.seg[j].A = Ad[j if c.distinct_a else 0].data_ptr()
		d.seg[j].lda = c.K
		d.seg[j].shift = s
		d.seg[j].w_off = w_off[j]
	d.W, d.ldw, d.M, d.N, d.K, d.rows_per_batch, d.act = Wd.data_ptr(), ldw, c.M, c.N, c.K, c.rpb, c.act
	d.bias = biasd.data_ptr() if biasd is not None else None
	d.residual = Cbuf.data_ptr() if c.residual == "alias" else (resd.data_ptr() if resd is not None else None)
	d.ldr = ldc if c.residual == "alias" else c.N
	d.C, d.ldc = Cbuf.data_ptr(), ldc
	d.out_scale = FP8_SCALE if c.dt == "fp8" else 0.0
	d.out_f32, d.transpose_out = int(c.out_f32), int(c.transpose)
	d.gn_T, d.gn_part = c.gn_T, part.data_ptr() if part is not None else None
	rc = lib.ttk_gemm(DT[c.dt], C.byref(d), _lib.stream_ptr())
	if rc != 0:
		return {"error": lib.ttk_last_error().decode()}
	torch.cuda.synchronize()
	if c.transpose:
		out = Cbuf[:c.M * c.N].view(c.M // c.rpb, c.N, c.rpb).cpu()
		canary_ok = bool(torch.isnan(Cbuf[c.M * c.N:]).all())
	else:
		out = Cbuf[:c.M, :c.N].cpu()
		canary_ok = bool(torch.isnan(Cbuf[c.M:]).all()) and bool(torch.isnan(Cbuf[:c.M, c.N:]).all())
	stats = None
	if part is not None:
		n = (part.numel() - 1024)
		stats = part[:n].view(-1, 32, c.gn_T // 64, 3).cpu()
		canary_ok = canary_ok and bool(torch.isnan(part[n:]).all())
	return {"digest": digest(out, stats), "canary_ok": canary_ok, "out": out, "stats": stats}


def child(config, outdir, auto_digests_path):
	sys.path.insert(0, ROOT)
	from tortoise_tts_amd import _lib
	lib = _lib.load()
	auto = pickle.load(open(auto_digests_path, "rb")) if auto_digests_path else None
	results = {}
	for c in CASES:
		r = run_case(lib, _lib, c, "cuda:0")
		if "digest" in r and auto is not None and auto.get(c.id) == r["digest"]:
			r["out"] = r["stats"] = None      # same bits as the auto configuration: nothing more to keep
		if r.get("out") is not None:
			torch.save({"out": r.pop("out"), "stats": r.pop("stats")}, os.path.join(outdir, f"{config}.{c.id}.pt"))
		else:
			r.pop("out", None), r.pop("stats", None)
		results[c.id] = r
		print(f"{config} {c.id}: {r.get('digest', r.get('error'))[:16]}", flush=True)
	pickle.dump(results, open(os.path.join(outdir, f"{config}.pkl"), "wb"))


# ----------------------------------------------------------------------------------------------------------- the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
	outdir = str(tmp_path_factory.mktemp("gemm_forms"))
	results = {}
	auto_path = None
	for config, env_add in CONFIGS.items():
		env = {k: v for k, v in os.environ.items() if not k.startswith(("TTK_GEMM_TILE", "TTK_GEMM_ROLE", "TTK_GEMM_MIXED"))}
		env.update(env_add)
		args = [sys.executable, os.path.abspath(__file__), "child", config, outdir] + ([auto_path] if auto_path else [])
		try:
			p = subprocess.run(args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
		except subprocess.TimeoutExpired:
			pytest.fail(f"configuration {config}: the child ran longer than {CHILD_TIMEOUT} s; no further configuration started")
		if p.returncode != 0:
			pytest.fail(f"configuration {config}: the child ended with {p.returncode}; no further configuration started\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}")
		results[config] = pickle.load(open(os.path.join(outdir, f"{config}.pkl"), "rb"))
		if config == "auto":
			auto_path = os.path.join(outdir, "auto.digests.pkl")
			pickle.dump({k: r["digest"] for k, r in results["auto"].items() if "digest" in r}, open(auto_path, "wb"))
	return outdir, results


def check_values(c, out, stats, ref, tol, what):
	got = out.double()
	if c.transpose:      # [b][N][rpb] -> [M][N]
		got = got.permute(0, 2, 1).reshape(c.M, c.N)
	assert torch.isfinite(got).all(), f"{what}: non-finite outputs (unwritten values?) at {(~torch.isfinite(got)).nonzero()[:5].tolist()}"
	err = (got - ref).abs()
	worst = (err / tol).max().item()
	if worst > 1:
		i = int((err / tol).argmax())
		r, n = divmod(i, c.N)
		pytest.fail(f"{what}: |got - ref| exceeds the bound {worst:.3g}x, worst at row {r} col {n}: got {got[r, n].item()!r} ref {ref[r, n].item()!r} tol {tol[r, n].item():.3g}")
	if stats is None:
		return
	nch = c.gn_T // 64
	assert stats.shape[0] == c.M // c.gn_T
	assert torch.isfinite(stats).all(), f"{what}: statistics triples left unwritten at {(~torch.isfinite(stats[..., 0])).nonzero()[:5].tolist()}"
	assert (stats[..., 0] == 2048.0).all(), f"{what}: a triple's count is not 2048"
	# (b, group, chunk) blocks of 64 rows x 32 channels of the f64 output
	blk = ref.view(c.M // c.gn_T, nch, 64, 32, 32).permute(0, 3, 1, 2, 4).reshape(c.M // c.gn_T, 32, nch, 2048)
	btol = tol.view(c.M // c.gn_T, nch, 64, 32, 32).permute(0, 3, 1, 2, 4).reshape(c.M // c.gn_T, 32, nch, 2048)
	mean = blk.mean(-1)
	# the mean: the values' own error plus an f32 sum of 2048 terms (32 sequential per lane, a 64-lane tree)
	mtol = btol.mean(-1) + 64 * 2.0 ** -24 * blk.abs().mean(-1)
	dev = blk - mean[..., None]
	m2 = (dev ** 2).sum(-1)
	e = btol + mtol[..., None]
	m2tol = 2 * (dev.abs() * e).sum(-1) + (e ** 2).sum(-1) + 66 * 2.0 ** -24 * m2
	em = (stats[..., 1].double() - mean).abs() / mtol
	e2 = (stats[..., 2].double() - m2).abs() / m2tol
	assert em.max() <= 1, f"{what}: chunk mean off by {em.max().item():.3g}x its bound at (b, group, chunk) {divmod(int(em.argmax()), 32 * nch)}"
	assert e2.max() <= 1, f"{what}: chunk M2 off by {e2.max().item():.3g}x its bound at (b, group, chunk) {divmod(int(e2.argmax()), 32 * nch)}"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_form_against_f64_on_every_configuration(runs, case):
	outdir, results = runs
	c = case
	ref, tol = None, None
	for config in CONFIGS:
		r = results[config][c.id]
		if c.gn_T and not gn_valid(c, config):
			assert "error" in r and "gn_part" in r["error"], f"{config}: gn_part accepted on a shape whose tiles do not produce the statistics"
			continue
		assert "error" not in r, f"{config}: ttk_gemm refused the case: {r.get('error')}"
		assert r["canary_ok"], f"{config}: a value was written outside C's [M][N] (padding columns, rows past M) or past the statistics"
		path = os.path.join(outdir, f"{config}.{c.id}.pt")
		if config != "auto" and not os.path.exists(path):
			continue      # same digest as auto
		if ref is None:
			ref, tol = reference(c)
		saved = torch.load(path)
		check_values(c, saved["out"], saved["stats"], ref, tol, config)
		if config != "auto":
			auto = torch.load(os.path.join(outdir, f"auto.{c.id}.pt"))
			diff = (saved["out"].double() - auto["out"].double()).abs().max().item()
			pytest.fail(f"{config}: within the f64 bound but not the auto configuration's bits (max |diff| {diff:.3g}): every tiling must add in the same k order")
	assert ref is not None or not any("digest" in results[k][c.id] for k in CONFIGS), "no configuration's output was checked"


def test_every_case_ran_under_auto(runs):
	_, results = runs
	assert set(results["auto"]) == {c.id for c in CASES}


def test_preconditions_are_refused():
	"""what the kernels take for granted comes back as TTK_E_ARG with a message"""
	sys.path.insert(0, ROOT)
	from tortoise_tts_amd import _lib
	lib = _lib.load()
	dev = "cuda:0"
	A = torch.zeros(128, 128, device=dev, dtype=torch.bfloat16)
	W = torch.zeros(128, 128, device=dev, dtype=torch.bfloat16)
	Cb = torch.zeros(128, 1024, device=dev)

	def desc(**kw):
		d = _lib.GemmDesc()
		d.nseg, d.W, d.ldw, d.M, d.N, d.K, d.C, d.ldc, d.out_f32 = 1, W.data_ptr(), 128, 128, 128, 128, Cb.data_ptr(), 128, 1
		d.seg[0].A, d.seg[0].lda = A.data_ptr(), 128
		for k, v in kw.items():
			setattr(d, k, v)
		return d

	def refused(d, match, dt=1):
		assert lib.ttk_gemm(dt, C.byref(d), _lib.stream_ptr()) == -1
		assert match in lib.ttk_last_error().decode()
	refused(desc(K=96), "K % 64")
	refused(desc(K=64), "K % 128", dt=3)
	refused(desc(ldw=120), "ldw")
	refused(desc(ldc=100), "ldc < N")
	refused(desc(nseg=13), "nseg")
	refused(desc(act=3), "act")
	refused(desc(transpose_out=1), "rows_per_batch")
	d = desc(); d.seg[0].shift = 1
	refused(d, "rows_per_batch")
	refused(desc(residual=Cb.data_ptr(), ldr=128, out_f32=0), "residual")
	refused(desc(gn_part=Cb.data_ptr(), gn_T=128), "gn_part")      # N = 128: no tile produces the statistics
	refused(desc(gn_part=Cb.data_ptr(), gn_T=64, N=1024, ldc=1024, M=64), "gn_part")      # M = 64: the 64 x 64 tile, waves of 32 rows


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
	child(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None)
