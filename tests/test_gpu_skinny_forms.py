"""Every launch form of the weight-streaming decode kernels (csrc/skinny.hip: k_skinny, csrc/gemv.hip: k_gemv) through `ttk_gemv_mat_create` /
`ttk_gemv_launch` against the float64 reference and the derived per-element bound of tests/skinny_ref.py (where the bound is written out and
tests/test_skinny_ref.py shows on the CPU that it and the canaries see a subtle fault).  The matrices go through the packers ttk_ar_create uses, the
launches through the decode step's own decision code.

Every output buffer starts as NaN -- out_f32 with canary rows behind row M, out_T in all 16 MT rows, qbuf, both caches, noise -- and so do the padding
rows of the fragment-order operand and the rows behind the M rows of x: what the launch owes must be finite and inside the bound, everything else must
still be NaN.  The equalities the code and include/ttk.h promise are asserted bit for bit: two runs; row r whatever the batch (and with it the m-tile
count of the instantiation) it is launched in; k_gemv's projections and head against k_skinny's, the folded launches in f32; family 0 against the family
the decode step is meant to choose.  One process, no environment knobs."""
import collections
import ctypes as C

import pytest
import torch

import skinny_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": 0, "bf16": 1, "f16": 4}
TTK_FP8W = 2
RATIOS = collections.defaultdict(float)      # case group -> worst err / bound seen (printed by the last test)
TAIL = 256                                   # canary elements behind a flat fragment-order buffer


@pytest.fixture(scope="module")
def lib():
	from tortoise_tts_amd import _lib
	return _lib.load(), _lib


def make_mat(lib, c, o):
	_, _lib = lib

	class GemvMat(_lib.Handle):
		def __init__(self):
			super().__init__(DEV)
			sd = R.create_weights(c, o)
			cfg = _lib.GemvMatConfigC(TTK_FP8W if c.w8 else DT[c.dt], c.layout, c.N, c.K)
			self._create("gemv_mat", cfg, sd, list(sd))
	return GemvMat()


def bits(t):
	return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
	return a.keys() == b.keys() and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


RNG = dict(seed=1234, offset0=8, threads=512, step=4, row0=2, group=5)


def launch(lib, mat, c, o, M, pos=0, family=None, waves=None, a_rows=None, health_in=0):
	"""one launch over the first M rows; returns (raw: the device buffers on the CPU as written, logical: skinny_ref.blank_outputs' layout in f64, aux)"""
	l, _lib = lib
	tdt = R.TDT[c.dt]
	MT = R.row_tiles(M)
	nan = float("nan")
	d = _lib.GemvDesc()
	d.dtype, d.role, d.form, d.M = DT[c.dt], R.ROLE[c.role], R.FORM[c.form], M
	d.family, d.waves, d.model_dim = c.family if family is None else family, c.waves if waves is None else waves, c.model_dim
	launched = C.c_int(0)
	d.launched = C.pointer(launched)
	keep = []

	def dev(t):
		t = t.to(DEV).contiguous()
		keep.append(t)
		return t
	if c.form == "prologue":
		x = torch.full((M + R.CANARY_ROWS, c.K), nan)
		x[:M] = o["x"][:M].float()
		d.x = dev(x).data_ptr()
		d.g1, d.b1 = dev(o["g1"].float()).data_ptr(), dev(o["b1"].float()).data_ptr()
		if c.norms == 2:
			d.g2, d.b2 = dev(o["g2"].float()).data_ptr(), dev(o["b2"].float()).data_ptr()
	else:
		rows = (o["a"] if a_rows is None else a_rows)[:M]
		d.a = dev(R.to_frag(rows.to(tdt), 16 * MT)).data_ptr()      # padding rows NaN
	buf = {}
	if c.role in ("head", "proj"):
		out = torch.full((M + R.CANARY_ROWS, c.N), nan)
		if c.role == "proj":
			out[:M] = o["res"][:M].float()
		buf["out_f32"] = dev(out)
		d.out_f32 = buf["out_f32"].data_ptr()
	if c.role == "fc" or (c.role == "proj" and c.out_T):
		buf["out_T"] = dev(torch.full((16 * MT * c.N + TAIL,), nan, dtype=tdt))
		d.out_T = buf["out_T"].data_ptr()
	d_pos = dev(torch.tensor([pos, 0], dtype=torch.int32))
	if c.role == "qkv":
		buf["qbuf"] = dev(torch.full((M + R.CANARY_ROWS, c.K), nan))
		buf["kcache"] = dev(torch.full((M + R.CANARY_ROWS, c.H, c.max_ctx, 64), nan, dtype=tdt))
		buf["vcache"] = dev(torch.full((M + R.CANARY_ROWS, c.H, c.max_ctx, 64), nan, dtype=tdt))
		d.qbuf, d.kcache, d.vcache, d.d_pos = buf["qbuf"].data_ptr(), buf["kcache"].data_ptr(), buf["vcache"].data_ptr(), d_pos.data_ptr()
		d.max_ctx, d.H, d.q_scale = c.max_ctx, c.H, R.Q_SCALE
	if c.bump:
		d.bump, d.d_pos = 1, d_pos.data_ptr()
	draws = None
	if c.noise:
		buf["noise"] = dev(torch.full((M + R.CANARY_ROWS, c.N), nan))
		draws = torch.arange(M, dtype=torch.int64) % 3 + 1
		rng = dev(torch.tensor([RNG[k] for k in ("seed", "offset0", "threads", "step", "row0", "group")], dtype=torch.int64))
		d.noise, d.rng, d.draws = buf["noise"].data_ptr(), rng.data_ptr(), dev(draws).data_ptr()
	health = dev(torch.tensor([health_in], dtype=torch.int32))
	d.health = health.data_ptr()
	rc = l.ttk_gemv_launch(mat._h, C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id} M={M} family {d.family} waves {d.waves}: ttk_gemv_launch refused the case: {l.ttk_last_error().decode()}"
	try:
		torch.cuda.synchronize()
	except RuntimeError as e:      # a device fault: nothing more is started on this GPU
		pytest.exit(f"{c.id} M={M} pos={pos} family {d.family} waves {d.waves}: the device reported {e}", returncode=3)
	raw = {k: v.cpu() for k, v in buf.items()}
	log = {}
	for k, v in raw.items():
		if k == "out_T":
			assert torch.isnan(v[16 * MT * c.N:]).all(), f"{c.id} M={M}: out_T was written behind its {16 * MT} rows"
			log[k] = R.from_frag(v[:16 * MT * c.N], 16 * MT, c.N).double()
		elif k != "noise":
			log[k] = v.double()
	aux = {"d_pos": d_pos.cpu().tolist(), "health": int(health.cpu()[0]), "draws": draws, "launched": launched.value}
	return raw, log, aux


def live(c, M, raw):
	"""the part of the raw buffers that is a function of the launch's first M rows alone (rows [0, M) of every row-indexed buffer)"""
	out = {}
	for k, v in raw.items():
		if k == "out_T":
			out[k] = R.from_frag(v[:16 * R.row_tiles(M) * c.N], 16 * R.row_tiles(M), c.N)[:M]
		else:
			out[k] = v[:M]
	return out


def rows_of(c, m, raw_big, M_big):
	"""rows [0, m) of a launch over M_big >= m rows, comparable with live(c, m, ...)"""
	out = {}
	for k, v in raw_big.items():
		if k == "out_T":
			out[k] = R.from_frag(v[:16 * R.row_tiles(M_big) * c.N], 16 * R.row_tiles(M_big), c.N)[:m]
		else:
			out[k] = v[:m]
	return out


def gemv_has(c, M):
	"""gemv_supported of csrc/gemv.hip restated: the launches k_gemv has an instantiation for"""
	if c.form == "prologue" or M > (32 if c.dt == "f32" else 64):
		return False
	if c.w8 and c.form != "fold" and c.role != "proj":
		return False
	if c.role == "head":
		return c.K == 1024
	if c.role == "proj":
		return c.K in (1024, 4096) and c.N % 128 == 0
	if c.role == "qkv":
		return c.K == 1024 and c.N == 3 * c.K
	return c.K == 1024 and c.N % 32 == 0


def gemv_waves(c):
	return 8 if (c.K == 4096 or (c.dt == "f32" and c.role != "head")) else 4


def expected_noise(lib, c, M, draws):
	l, _lib = lib
	n_el = (RNG["row0"] + RNG["group"]) * c.N
	want = torch.empty(M, c.N)
	for dr in sorted(set(draws.tolist())):
		e = torch.empty(n_el, device=DEV)
		_lib.check(l.ttk_exponential_like_torch(e.data_ptr(), n_el, RNG["seed"], RNG["offset0"], RNG["threads"], RNG["step"], dr, _lib.stream_ptr()), "ttk_exponential_like_torch")
		torch.cuda.synchronize()
		e = e.cpu().view(-1, c.N)
		for m in range(M):
			if draws[m] == dr:
				want[m] = e[RNG["row0"] + m % RNG["group"]]
	return want


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_launch_against_f64(lib, case):
	c = case
	o = R.operands(c)
	ref = R.reference(c, o)
	mat = make_mat(lib, c, o)
	prev = None
	for M in c.ms():
		for pos in c.pos:
			raw, log, aux = launch(lib, mat, c, o, M, pos)
			what = f"{c.id} M={M} pos={pos}"
			r = R.check_outputs(c, M, pos, log, ref)
			RATIOS[c.group] = max(RATIOS[c.group], r)
			print(f"{what}: err / bound {r:.3f}")
			assert r <= 1, f"{what}: |got - ref| is {r:.3g}x the bound"
			assert aux["d_pos"] == [pos + (1 if c.bump else 0), 0], f"{what}: d_pos is {aux['d_pos']} after the launch"
			assert aux["health"] == (1 if c.special == "nearconst" else 0), f"{what}: health word {aux['health']}"
			if c.noise:
				n = raw["noise"]
				assert torch.isnan(n[M:]).all(), f"{what}: noise was written behind row M"
				assert torch.equal(bits(n[:M]), bits(expected_noise(lib, c, M, aux["draws"]))), f"{what}: the noise is not ttk_exponential_like_torch's, bit for bit"
		# (the last position of the case from here on) row r has the same bits whatever batch it is launched in
		if prev is not None:
			pM, praw = prev
			assert same_bits(live(c, pM, praw), rows_of(c, pM, raw, M)), f"{c.id}: rows [0, {pM}) of the {M}-row launch ({R.row_tiles(M)} m-tiles) differ in bits from the {pM}-row launch's"
		prev = (M, raw)
	M, pos = max(c.ms()), c.pos[-1]
	again, _, _ = launch(lib, mat, c, o, M, pos)
	assert same_bits(raw, again), f"{c.id}: two runs give different bits"
	# family 0 is the family the decode step is meant to choose at this shape, on the same operands
	exp = 2 if gemv_has(c, M) else 1
	raw0, _, aux0 = launch(lib, mat, c, o, M, pos, family=0)
	assert aux0["launched"] == exp, f"{c.id}: family 0 launched family {aux0['launched']}, the decode step is meant to choose {exp} here"
	rawe, _, auxe = (raw, None, aux) if exp == c.family else launch(lib, mat, c, o, M, pos, family=exp)
	assert auxe["launched"] == exp
	assert same_bits(raw0, rawe), f"{c.id}: family 0 does not give the bits of family {exp}"
	if c.expect_family:
		assert exp == c.expect_family, c.id


@pytest.mark.parametrize("case", [c for c in R.CASES if c.family == 2], ids=[c.id for c in R.CASES if c.family == 2])
def test_gemv_equals_skinny(lib, case):
	"""k_gemv repeats k_skinny operation for operation: the projections and the head bit for bit in every type and for every M, the folded launches in f32 (in
	16-bit the lane sums of the statistics differ: both are held against the bound)"""
	c = case
	o = R.operands(c)
	ref = R.reference(c, o)
	mat = make_mat(lib, c, o)
	for M in c.ms():
		pos = c.pos[0]
		g, _, ga = launch(lib, mat, c, o, M, pos, family=2)
		s, slog, sa = launch(lib, mat, c, o, M, pos, family=1, waves=gemv_waves(c))
		assert (ga["launched"], sa["launched"]) == (2, 1)
		if c.model_dim or c.role != "proj":      # with the model's width known, waves = 0 is the wave count k_gemv repeats
			assert same_bits(s, launch(lib, mat, c, o, M, pos, family=1, waves=0)[0]), f"{c.id} M={M}: waves = 0 is not k_gemv's wave count"
		r = R.check_outputs(c, M, pos, slog, ref)
		RATIOS["gemv (k_skinny on its operands)"] = max(RATIOS["gemv (k_skinny on its operands)"], r)
		assert r <= 1, f"{c.id} M={M}: k_skinny on k_gemv's operands is {r:.3g}x the bound"
		if c.form != "fold" or c.dt == "f32":
			assert same_bits(g, s), f"{c.id} M={M}: k_gemv and k_skinny differ in bits"


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("family", [1, 2])
def test_health_word(lib, dt, family):
	"""the folded launch reports what it cannot represent, in both families: every channel offset by 40 std gives bit 0, an f16 row holding +inf bit 1; healthy
	rows leave the word alone (also a bit that is already set)"""
	c = next(c for c in R.CASES if c.id == f"gemv-fc-{dt}-N64")
	o = R.operands(c)
	mat = make_mat(lib, c, o)
	M = 17
	_, _, aux = launch(lib, mat, c, o, M, family=family, health_in=0)
	assert aux["health"] == 0
	_, _, aux = launch(lib, mat, c, o, M, family=family, health_in=4)
	assert aux["health"] == 4
	off = R.grid((o["a"] + 40.0).float())
	_, log, aux = launch(lib, mat, c, o, M, family=family, a_rows=off)
	assert aux["health"] == 1, f"common offset of 40 std: health word {aux['health']}, expected bit 0"
	assert torch.isfinite(log["out_T"][:M]).all()
	one = o["a"].clone()
	one[16] = (one[16] + 40.0).float().bfloat16().double()      # one row of the second m-tile only
	_, _, aux = launch(lib, mat, c, o, M, family=family, a_rows=one)
	assert aux["health"] == 1, "a row of the second m-tile with |mean| > 8 std was not reported"
	if dt == "f16":
		inf = o["a"].clone()
		inf[3, 100] = float("inf")
		_, log, aux = launch(lib, mat, c, o, M, family=family, a_rows=inf)
		assert aux["health"] & 2, f"an f16 row holding +inf: health word {aux['health']}, expected bit 1"
		others = torch.arange(M) != 3
		assert torch.isfinite(log["out_T"][:M][others]).all(), "the +inf row reached other rows"


def test_preconditions_are_refused(lib):
	"""what the kernels take for granted comes back as TTK_E_ARG with a message; nothing is launched"""
	l, _lib = lib
	byid = {c.id: c for c in R.CASES}
	z = lambda n, dt=torch.float32: torch.zeros(n, device=DEV, dtype=dt)

	def base(c, M=5):
		d = _lib.GemvDesc()
		d.dtype, d.role, d.form, d.M = DT[c.dt], R.ROLE[c.role], R.FORM[c.form], M
		tdt = R.TDT[c.dt]
		keep = [z(64 * max(c.K, c.N), tdt), z(64 * max(c.K, c.N)), z(64 * c.N, tdt), z(c.K), z(64 * c.K), z(64 * c.K * 8, tdt), z(4, torch.int32), z(64 * c.N), z(8, torch.int64), z(64, torch.int64)]
		if c.form == "prologue":
			d.x, d.g1, d.b1 = keep[1].data_ptr(), keep[3].data_ptr(), keep[3].data_ptr()
		else:
			d.a = keep[0].data_ptr()
		if c.role in ("head", "proj"):
			d.out_f32 = keep[1].data_ptr()
		if c.role in ("fc", "proj"):
			d.out_T = keep[2].data_ptr()
		if c.role == "qkv":
			d.qbuf, d.kcache, d.vcache, d.d_pos, d.max_ctx, d.H, d.q_scale = keep[4].data_ptr(), keep[5].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr(), 8, c.H, 0.125
		return d, keep

	def refused(mat, d, match):
		assert l.ttk_gemv_launch(mat._h if mat else None, C.byref(d), _lib.stream_ptr()) == -1, match
		assert match in l.ttk_last_error().decode(), (match, l.ttk_last_error().decode())

	def variants(cid):
		c = byid[cid]
		mat = make_mat(lib, c, R.operands(c))
		d, keep = base(c)
		assert l.ttk_gemv_launch(mat._h, C.byref(d), _lib.stream_ptr()) == 0, l.ttk_last_error().decode()      # the base descriptor itself is fine

		def v(**kw):
			d, keep2 = base(c)
			keep.extend(keep2)
			for k, val in kw.items():
				setattr(d, k, val)
			return d
		return c, mat, v

	c, mat, v = variants("proj-bf16-N64-K64")
	refused(None, v(), "null matrix")
	refused(mat, v(a=None), "null a")
	refused(mat, v(a=v().a + 8), "a must be 16-byte aligned")
	refused(mat, v(out_f32=None), "null out_f32")
	refused(mat, v(out_f32=v().out_f32 + 2), "out_f32 4-byte aligned")
	refused(mat, v(out_T=v().out_T + 8), "out_T must be 16-byte aligned")
	refused(mat, v(M=0), "outside 1..64")
	refused(mat, v(M=65), "outside 1..64")
	refused(mat, v(form=1), "qkv and fc only")
	refused(mat, v(form=2), "no LayerNorm in front")
	refused(mat, v(form=3), "form must be")
	refused(mat, v(role=4), "role must be")
	refused(mat, v(dtype=4), "not the arithmetic type")
	refused(mat, v(dtype=3), "dtype must be")
	refused(mat, v(family=3), "family must be")
	refused(mat, v(family=2), "no instantiation")
	refused(mat, v(waves=3), "waves must be")
	refused(mat, v(waves=17), "waves must be")
	refused(mat, v(model_dim=100), "model_dim must be")
	c, mat, v = variants("proj-f32-N64-K64")
	refused(mat, v(M=33), "outside 1..32")
	c, mat, v = variants("proj-fp8-N64-K64")
	refused(mat, v(dtype=4), "fp8 matrix runs under bf16 arithmetic only")
	refused(mat, v(dtype=0), "fp8 matrix runs under bf16 arithmetic only")
	c, mat, v = variants("head-bf16-K192-w0")      # N = 34
	refused(mat, v(out_T=v().out_f32), "N % 32 == 0")
	refused(mat, v(role=2, form=1, out_T=v().out_f32), "created with gamma and beta")
	refused(mat, v(noise=v().out_f32), "noise, rng and draws or none")
	refused(mat, v(bump=1), "bump needs")
	c, mat, v = variants("fold-qkv-bf16-K192")
	for name in ("qbuf", "kcache", "vcache", "d_pos"):
		refused(mat, v(**{name: None}), "null qbuf, kcache, vcache or d_pos")
	refused(mat, v(qbuf=v().qbuf + 8), "16-byte aligned")
	refused(mat, v(kcache=v().kcache + 8), "16-byte aligned")
	refused(mat, v(vcache=v().vcache + 2), "16-byte aligned")
	refused(mat, v(H=2), "K == 64 H")
	refused(mat, v(max_ctx=0), "max_ctx >= 1")
	refused(mat, v(q_scale=1.0), "q_scale must be 0.125")
	refused(mat, v(form=0), "folded or the prologue form")
	refused(mat, v(role=3, out_f32=v().qbuf), "qkv and fc only")
	c, mat, v = variants("fold-fc-bf16-N64-K64")      # an fc matrix is no qkv matrix
	refused(mat, v(role=0, qbuf=v().a, kcache=v().a, vcache=v().a, d_pos=v().a, H=1, max_ctx=8, q_scale=0.125), "N == 3 K")
	refused(mat, v(out_T=None), "null out_T")
	c, mat, v = variants("pro-fc-bf16-K192-w4")
	refused(mat, v(x=None), "needs x, g1 and b1")
	refused(mat, v(g1=None), "needs x, g1 and b1")
	refused(mat, v(g2=v().g1), "g2 with b2 or neither")
	refused(mat, v(x=v().x + 4), "16-byte aligned")
	refused(mat, v(M=33), "at most 32 rows")
	refused(mat, v(waves=9), "waves must be 0 or 4..8")
	refused(mat, v(family=2), "no LayerNorm-prologue form")
	# more LDS than a compute unit has: refused here, never launched (f32 rows of K = 2048: 16 MT (4 K + 16) bytes, 262 KiB at two m-tiles)
	c, mat, v = variants("pro-fc-f32-K2048-w4")
	refused(mat, v(M=17), "a compute unit has")
	c, mat, v = variants("pro-head2-bf16-K2048")
	refused(mat, v(M=49), "a compute unit has")
	# the matrix itself
	w = torch.zeros(64, 96)
	views, keepw = _lib.weight_views({"weight": w, "bias": torch.zeros(64)}, ["weight", "bias"])
	h = C.c_void_p()
	assert l.ttk_gemv_mat_create(C.byref(h), C.byref(_lib.GemvMatConfigC(1, 0, 64, 96)), views, 2) == -1 and "K % 64 == 0" in l.ttk_last_error().decode()
	assert l.ttk_gemv_mat_create(C.byref(h), C.byref(_lib.GemvMatConfigC(3, 0, 64, 64)), views, 2) == -1 and "bad dtype" in l.ttk_last_error().decode()
	assert l.ttk_gemv_mat_create(C.byref(h), C.byref(_lib.GemvMatConfigC(1, 2, 64, 64)), views, 2) == -1 and "layout" in l.ttk_last_error().decode()
	torch.cuda.synchronize()


def test_zz_report(lib):
	"""(runs last in this module) the worst err / bound per case group, for the record"""
	for k in sorted(RATIOS):
		print(f"worst err / bound, {k}: {RATIOS[k]:.3f}")
	assert all(v <= 1 for v in RATIOS.values())
