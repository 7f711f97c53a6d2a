"""Float64 restatements of what csrc/align.hip computes -- the causal attention map, the alignment cost, the DTW table -- written from the definitions,
with derived error bounds, the operands and case lists that tests/test_align_ref.py (CPU) and tests/test_gpu_align.py (GPU) share, a float32 emulation
of k_attn_probs with switchable faults that shows the bound can see them, and a float64 GPT-2 dense pass that reproduces the fixtures' maps.

THE MAP.  Per sequence b, head h, query q:  P[q][k] = softmax over k <= q of (0.125 q_q . k_k), exactly 0 for k > q.  Operands are attn_ref.grid values
(exact in bf16, f16 and f32; 0.125 q exact in T; every product exact in f32), so the reference sees the kernel's own inputs.

THE BOUND, per element.  u = 2^-24; s2 = log2e s, the score in the log2 domain (the kernel uses exp2); Mabs = max_k |s2_k| over the query's keys k <= q;
mag_k = 0.125 sum_d |q_d| |k_d|.
  e_k   = ln2 (log2e 1e-5 mag_k + u (|s2_k| + 4 Mabs)) + 2u
          f32 accumulation of the 64-term dot product (the constant of attn_ref.py); LOG2E as an f32 constant (0.24 u relative) and the product s * LOG2E
          (u), both relative to |s2_k|; the rounding of the difference to the reference point m, u |s2_k - m| with |s2_k - m| <= 2 Mabs + 1; v_exp_f32 at
          one ulp (2u).  The kernel's m is an INTEGER (ceil of the largest score), which is where the "+ 1" comes from: ln2 u < u relative, paid from the
          3u P_k term below, of which the kernel spends 2u (one correctly rounded 1 / l, one product).
  EL    = (nt + 4 + 2) u,  nt = q // 16 + 1 key tiles
          k_attn_probs sums l per lane over its 4 keys of a 16-key tile as (p0 + p1) + (p2 + p3), adds that to the running sum once per tile, and merges the
          query's four lanes with two fold adds: the longest chain of f32 adds behind any term is nt + 2 + 2.  A rise of m rescales l by a power of two
          (v_ldexp_f32): exact.  All terms are positive, so the sum's relative error is at most (chain length) u to first order.
  |dP_k| <= 1.02 P_k (e_k + sum_j P_j e_j + EL) + 3u P_k       first order in the relative errors of p_k and l; they stay far below 2^-6, 1.02 covers the rest
  + 2^-125 for k <= q: underflow of the output format.  v_exp_f32 returns 0 for a result below 2^-126, the smallest normal float32, and P_k = p_k / l with
          l >= 1/2 (the largest term is exp2(s2 - ceil(s2)) > 1/2), so any P_k below 2^-125 may come out as 0; float32 has no relative accuracy there in
          any case.  The peaked operands, with scores hundreds of units apart, reach such values.
No term is fitted to a measurement.  P is never rounded to T: the bound is the same for the three dtypes.

THE COST.  A f32 [nb][n][M][Tt] -> matrix [nb][M][Tt]: z = (A - mean) / std per row over the text axis (population std, zeros where std == 0), the median
over a window of `width` rows along M with reflect padding (no filter when M <= width // 2), the mean over the heads; cost = -matrix.  Kernel arithmetic and
its tolerance (prepare_reference): with g = (ceil(Tt / 64) + 6) u for a 64-lane strided sum followed by the wave reduction,
  |d mean| <= (g + u) max|x|;  |d z| <= 1.01 [(g + u) max|x| / std + |z| (g / 2 + 6u)]   (the difference, the sum of squares, the division by Tt, the
  square root and the final division, one rounding each; the mean's error enters the variance at second order);
  the median is 1-Lipschitz in the sup norm: its tolerance is the largest of its window's; the mean over n heads adds (n + 1) u sum_h |median_h| / n.

DTW.  D[0][0] = 0, borders +inf, D[i][j] = cost[i-1][j-1] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) in float32, on ties the first of (diagonal, i - 1, j - 1):
dtw_reference walks the anti-diagonals in numpy float32 and is owed bit for bit."""
import math

import numpy as np
import torch

import attn_ref as R

U, LOG2E, LN2, SCALE = R.U, R.LOG2E, R.LN2, R.SCALE
NEG_BIG = -1e30
S_EDGES = (1, 15, 16, 17, 63, 64, 65, 129, 200)


def _probs_cases():
	cs = []
	for T in S_EDGES:
		for dt in ("bf16", "f16", "f32"):
			for layout in ("gpt", "hm"):
				cs.append(R.Fwd(f"probs-{dt}-S{T}-{layout}", dt, 2, 2, T, "causal", layout, group="probs"))
	for dt in ("bf16", "f16", "f32"):
		cs.append(R.Fwd(f"probs-{dt}-S200-peaked", dt, 2, 2, 200, "causal", qmul=64.0, group="probs-peaked"))
	for i, c in enumerate(cs):
		c.seed = 7000 + i
	return cs


PROBS_CASES = _probs_cases()


def windows(T):
	"""(r0, R, c0, C): the whole matrix, a 1 x 1 window below the diagonal, and windows whose rows and columns start and end off the 16-tile grid"""
	w = [(0, T, 0, T), (T // 2, 1, T // 3, 1)]
	if T >= 4:
		w.append((1, T - 2, 2, T - 3))
	if T >= 40:
		w.append((17, T - 22, 3, 30))
	return list(dict.fromkeys(w))


def probs_reference(c, q, k):
	"""(P, tol) f64 [nb][H][T][T] from q, k f64 [nb][H][T][64]"""
	T = c.T
	qi, ki = torch.arange(T)[:, None], torch.arange(T)[None, :]
	mask = ki > qi
	s = SCALE * (q @ k.transpose(-1, -2))
	mag = SCALE * (q.abs() @ k.abs().transpose(-1, -2))
	P = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
	s2 = (s * LOG2E).masked_fill(mask, 0.0)
	mabs = s2.abs().amax(-1, keepdim=True)
	e = LN2 * (LOG2E * 1e-5 * mag + U * (s2.abs() + 4 * mabs)) + 2 * U
	EL = ((qi // 16 + 1) + 4 + 2).double() * U
	tol = 1.02 * P * (e + (P * e).sum(-1, keepdim=True) + EL) + 3 * U * P + 2.0 ** -125
	return P, tol.masked_fill(mask, 0.0)


PROBS_FAULTS = ("causal_strict", "drop_last_key", "window_row_off_by_one", "window_col_off_by_one", "wrong_head")


def probs_fault_applies(c, fault):
	"""whether the fault changes the definition's result: a 1 x 1 map is 1 for every head and has nowhere to move a window to"""
	if fault == "wrong_head":
		return c.H >= 2 and c.T >= 2
	return c.T >= 2 if fault in ("window_row_off_by_one", "window_col_off_by_one") else True


def emulate_probs(c, q, k, fault=None, window=None, heads=None):
	"""k_attn_probs' arithmetic in float32 torch: per query four lanes (g) that each own keys 16 kt + 4 g + r, an integer reference point per lane, power-of-two
	rescales, the tile sum as (p0 + p1) + (p2 + p3), the lanes merged by two fold adds, exp2(v - m) * (1 / l).  Returns f64 [nb][n_sel][R][C]."""
	T = c.T
	r0, Rn, c0, Cn = window or (0, T, 0, T)
	hs = list(heads) if heads is not None else list(range(c.H))
	if fault == "wrong_head":
		hs = [(h + 1) % c.H for h in hs]
	l2e = torch.tensor(R.LOG2E_F32, dtype=torch.float32)
	qq = R._to_t((q * SCALE).float(), c.dt)[:, hs]
	kk = k.float()[:, hs]
	nt = (T + 15) // 16
	s = torch.zeros(c.nb, len(hs), T, 16 * nt, dtype=torch.float32)
	s[..., :T] = qq @ kk.transpose(-1, -2)
	qi, ki = torch.arange(T)[:, None], torch.arange(16 * nt)[None, :]
	valid = ((ki < qi) if fault == "causal_strict" else (ki <= qi)) & (ki < T)
	if fault == "drop_last_key":
		valid = valid & (ki != T - 1)
	v = (s * l2e).masked_fill(~valid, NEG_BIG)
	v4, val4 = v.view(c.nb, len(hs), T, nt, 4, 4), valid.view(T, nt, 4, 4)
	m = torch.full((c.nb, len(hs), T, 4), NEG_BIG, dtype=torch.float32)
	l = torch.zeros_like(m)
	for kt in range(nt):
		vt = v4[..., kt, :, :]
		m_new = torch.maximum(m, torch.ceil(vt.amax(-1)))
		l = torch.ldexp(l, (m - m_new).clamp_min(-200.0).int())
		m = m_new
		p = torch.where(val4[:, kt], torch.exp2(vt - m[..., None]), torch.zeros((), dtype=torch.float32))
		l = l + ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))
	mq = m.amax(-1, keepdim=True)
	l = torch.ldexp(l, (m - mq).clamp_min(-200.0).int())
	L = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
	inv = (1.0 / L)[..., None]
	P = torch.where(valid, torch.exp2(v - mq) * inv, torch.zeros((), dtype=torch.float32))[..., :T].double()
	if fault == "window_row_off_by_one":
		P = torch.roll(P, -1, dims=-2)
	if fault == "window_col_off_by_one":
		P = torch.roll(P, -1, dims=-1)
	return P[..., r0:r0 + Rn, c0:c0 + Cn]


def worst_ratio(got, ref, tol):
	"""max |got - ref| / tol; where the tolerance is 0 (above the diagonal) the value is owed exactly; a NaN counts as infinite"""
	d = (got - ref).abs()
	if torch.isnan(d).any() or bool((d[tol == 0] != 0).any()):
		return float("inf")
	nz = tol > 0
	return (d[nz] / tol[nz]).max().item() if nz.any() else 0.0


# ----------------------------------------------------------------------------------------------------------- GPT-2 dense pass in float64
def gpt2_maps_f64(sd, cfg, cond, text, codes):
	"""The attention maps [layers][B][H][S][S] of the teacher-forced pass over [cond | start_text, text, stop_text | start_mel, codes, stop_mel] in float64, from the
	state dict: HF's GPT-2 block (pre-LN, Conv1D x W + b, gelu_new, eps 1e-5) written out.  Reproduces the stored float32 maps of tests/golden/ar_attn_*.npz
	within the stored max |P32 - P64| of each layer (+ 1e-12 for the two float64 passes' own difference)."""
	F = torch.nn.functional
	g = lambda n: sd[n].double()
	B, Tt, M, d, H = text.shape[0], text.shape[1], codes.shape[1], cfg.model_dim, cfg.heads
	col = lambda v: torch.full((B, 1), v, dtype=torch.int64)
	tt = torch.cat([col(cfg.start_text_token), text, col(cfg.stop_text_token)], 1)
	mm = torch.cat([col(cfg.start_mel_token), codes, col(cfg.stop_mel_token)], 1)
	x = torch.cat([cond.double()[:, None], g("text_embedding.weight")[tt] + g("text_pos_embedding.emb.weight")[:Tt + 2],
				   g("mel_embedding.weight")[mm] + g("mel_pos_embedding.emb.weight")[:M + 2]], 1)
	S = x.shape[1]
	ln = lambda x, p: F.layer_norm(x, (d,), g(p + ".weight"), g(p + ".bias"), 1e-5)
	lin = lambda x, p: x @ g(p + ".weight") + g(p + ".bias")
	above = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
	maps = []
	for l in range(cfg.layers):
		p = f"gpt.h.{l}."
		q, k, v = (t.view(B, S, H, 64).transpose(1, 2) for t in lin(ln(x, p + "ln_1"), p + "attn.c_attn").split(d, -1))
		P = torch.softmax((0.125 * (q @ k.transpose(-1, -2))).masked_fill(above, float("-inf")), -1)
		maps.append(P)
		x = x + lin((P @ v).transpose(1, 2).reshape(B, S, d), p + "attn.c_proj")
		hdn = lin(ln(x, p + "ln_2"), p + "mlp.c_fc")
		hdn = 0.5 * hdn * (1 + torch.tanh(math.sqrt(2 / math.pi) * (hdn + 0.044715 * hdn ** 3)))
		x = x + lin(hdn, p + "mlp.c_proj")
	return torch.stack(maps)


# ----------------------------------------------------------------------------------------------------------- cost and DTW
def _window_rows(M, width):
	pad = width // 2 if M > width // 2 else 0
	idx = np.arange(M)[:, None] + np.arange(-pad, pad + 1)[None, :]
	idx = np.where(idx < 0, -idx, idx)
	return np.where(idx >= M, 2 * (M - 1) - idx, idx)      # [M][2 pad + 1], reflect


def prepare_reference(A, width):
	"""(matrix, tol) f64 [nb][M][Tt] from A [nb][n][M][Tt] (the kernel's float32 input values); cost = -matrix"""
	A = np.asarray(A, dtype=np.float64)
	nb, n, M, Tt = A.shape
	mean = A.mean(-1, keepdims=True)
	sd = np.sqrt(((A - mean) ** 2).mean(-1, keepdims=True))
	safe = np.where(sd > 0, sd, 1.0)
	z = np.where(sd > 0, (A - mean) / safe, 0.0)
	g = (math.ceil(Tt / 64) + 6) * U
	tz = np.where(sd > 0, 1.01 * ((g + U) * np.abs(A).max(-1, keepdims=True) / safe + np.abs(z) * (g / 2 + 6 * U)), 0.0)
	rows = _window_rows(M, width)
	med = np.median(z[:, :, rows, :], axis=3)      # [nb][n][M][Tt]
	tmed = tz[:, :, rows, :].max(axis=3)
	matrix = med.sum(1) / n
	tol = (tmed.sum(1) + (n + 1) * U * np.abs(med).sum(1)) / n
	return matrix, tol


def dtw_reference(cost):
	"""(trace u8 [M][Tt], total f32) of cost f32 [M][Tt], in float32, anti-diagonal by anti-diagonal"""
	cost = np.asarray(cost, dtype=np.float32)
	M, Tt = cost.shape
	D = np.full((M + 1, Tt + 1), np.inf, dtype=np.float32)
	D[0, 0] = 0
	trace = np.zeros((M, Tt), dtype=np.uint8)
	for d in range(2, M + Tt + 1):
		i = np.arange(max(1, d - Tt), min(M, d - 1) + 1)
		j = d - i
		c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
		t = np.where((c0 <= c1) & (c0 <= c2), 0, np.where(c1 <= c2, 1, 2)).astype(np.uint8)
		best = np.where(t == 0, c0, np.where(t == 1, c1, c2))
		D[i, j] = cost[i - 1, j - 1] + best
		trace[i - 1, j - 1] = t
	return trace, D[M, Tt]


def planted_case(seed):
	"""A f32 [3][M][Tt] with a planted monotone path: 3 .. 11 text tokens, 4 .. 8 mel rows per token, 0.6 on the path, uniform noise in [0, 0.1] elsewhere, every
	row scaled by a factor in [0.05, 1].  Returns (A, token of every mel row)."""
	rng = np.random.default_rng(seed)
	Tt = int(rng.integers(3, 12))
	runs = rng.integers(4, 9, size=Tt)
	tok = np.repeat(np.arange(Tt), runs)
	M = tok.size
	A = rng.uniform(0.0, 0.1, size=(3, M, Tt))
	A[:, np.arange(M), tok] = 0.6
	A *= rng.uniform(0.05, 1.0, size=(3, M, 1))
	return A.astype(np.float32), tok


def align_reference(A, width=7):
	"""numpy alignment of one sequence's per-head blocks A [n][M][Tt]: (text indices, mel indices, token starts, total)"""
	from tortoise_tts_amd import alignment
	matrix, _ = prepare_reference(np.asarray(A)[None], width)
	trace, total = dtw_reference((-matrix[0]).astype(np.float32))
	ti, mi = alignment.backtrace(trace)
	return ti, mi, alignment.token_starts(ti, mi, trace.shape[1]), total
