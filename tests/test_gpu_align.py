"""The attention maps of the teacher-forced pass and the text-to-audio alignment on the GPU (csrc/align.hip, ttk_ar_attentions, ttk_ar_text_attention,
UnifiedVoice.attentions / text_alignment) against tests/align_ref.py: the float64 restatements and their derived bounds,
where the bound's model is written out and tests/test_align_ref.py shows on the CPU that it sees a planted fault.

Kernel level: k_attn_probs on grid operands, both layouts, three dtypes, every sequence edge of the 16-query / 16-key tiles; windows and head subsets bit for
bit the full map's; P @ V consistent with ttk_attn_fwd on the same buffer; the cost kernel within its derived tolerance; the DTW kernel bit for bit numpy's.
Model level: the maps against the reference's own (tests/golden/ar_attn_*.npz, tools/make_golden_ar_attn.py) -- f32 within 4 x the reference's stored
max |P32 - P64| of the layer, bf16 within 1.5 x its stored max |Pbf16 - P64| -- the text blocks bit for bit a region of the maps, the alignment equal to
numpy's on the kernel's own blocks, and nothing else on the handle changed by any of it.

Measured on MI355X: k_attn_probs at most 0.011 of the bound on the edge cases (rows sum to 1 within 2.1e-7), 0.97 on the peaked S = 200 operands (entries
in [2^-126, 2^-125) stored as 0: the bound's underflow floor); P @ V against ttk_attn_fwd at 0.72 (bf16), 0.54 (f16), 0.002 (f32) of the allowed difference;
the maps against the reference: see test_attention_maps_against_the_reference."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

import align_ref as A
import attn_ref as R
from tortoise_tts_amd import _lib, alignment, weights as W
from tortoise_tts_amd.autoregressive import UnifiedVoice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": 0, "bf16": 1, "f16": 4}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_models = {}


@pytest.fixture(scope="module")
def lib():
	return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def release_handles():
	yield
	_models.clear()
	gc.collect()


def qkv_buffer(c, q, k, v):
	"""qkv [nb*T][ld] of the kernel's type in the case's layout (tests/test_gpu_attn_forms.py: fwd_buffers), NaN where no operand lies"""
	tdt = R.TDT[c.dt]
	frag = 4 if c.dt == "f32" else 8
	if c.layout == "gpt":
		ld, hs, offs = 3 * 64 * c.H, 64, (0, 64 * c.H, 2 * 64 * c.H)
	else:
		ld, hs, offs = 3 * 64 * c.H + frag, 192, (0, 64, 128)
	qkv = torch.full((c.nb, c.T, ld), float("nan"), dtype=tdt)
	for x, off in zip((q, k, v), offs):
		for h in range(c.H):
			qkv[:, :, off + h * hs: off + h * hs + 64] = x[:, h].to(tdt)
	return qkv.view(c.nb * c.T, ld).to(DEV), ld, hs, offs


def run_probs(lib, c, qkv, ld, hs, offs, heads, window):
	"""one launch into a NaN buffer with canary rows behind it; returns f32 [nb][n_sel][R][C] on the CPU"""
	r0, Rn, c0, Cn = window
	n = len(heads)
	numel = c.nb * n * Rn * Cn
	out = torch.full((numel + 64,), float("nan"), device=DEV, dtype=torch.float32)
	hd = torch.tensor(heads, dtype=torch.int32, device=DEV)
	d = _lib.AttnProbsDesc(qkv=qkv.data_ptr(), ld=ld, q_off=offs[0], k_off=offs[1], head_stride=hs, nb=c.nb, T=c.T, H=c.H, scale=R.SCALE, n_sel=n,
						   heads=hd.data_ptr(), out=out.data_ptr(), r0=r0, R=Rn, c0=c0, C=Cn)
	rc = lib.ttk_attn_probs(DT[c.dt], C.byref(d), _lib.stream_ptr())
	assert rc == 0, f"{c.id}: ttk_attn_probs refused the case: {lib.ttk_last_error().decode()}"
	torch.cuda.synchronize()
	assert torch.isnan(out[numel:]).all(), f"{c.id} window {window}: something behind the output was written"
	return out[:numel].cpu().view(c.nb, n, Rn, Cn)


@pytest.mark.parametrize("case", A.PROBS_CASES, ids=[c.id for c in A.PROBS_CASES])
def test_attn_probs_against_f64(lib, case):
	c = case
	q, k, v, _ = R.fwd_operands(c)
	ref, tol = A.probs_reference(c, q, k)
	qkv, ld, hs, offs = qkv_buffer(c, q, k, v)
	full = run_probs(lib, c, qkv, ld, hs, offs, list(range(c.H)), (0, c.T, 0, c.T))
	assert torch.isfinite(full).all(), f"{c.id}: unwritten or non-finite entries"
	above = torch.triu(torch.ones(c.T, c.T, dtype=torch.bool), 1)
	assert (full[..., above] == 0).all(), f"{c.id}: entries above the diagonal are not exactly 0"
	r = A.worst_ratio(full.double(), ref, tol)
	print(f"{c.id}: err / tol {r:.3f}, rows sum to 1 within {(full.double().sum(-1) - 1).abs().max():.2e}")
	assert r <= 1.0, f"{c.id}: |got - ref| is {r:.3g}x the bound"
	for win in A.windows(c.T):      # windows and a head subset: bit for bit the full map's region
		r0, Rn, c0, Cn = win
		for heads in ([1], [1, 0]):
			got = run_probs(lib, c, qkv, ld, hs, offs, heads, win)
			assert torch.equal(got, full[:, heads, r0:r0 + Rn, c0:c0 + Cn]), f"{c.id}: window {win} of heads {heads} is not the full map's region bit for bit"


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_probs_times_v_is_what_the_pass_computed(lib, dt):
	"""P @ V in float64 against ttk_attn_fwd(causal) on the same buffer; allowed: fwd_reference's bound + sum_k tol(P_k) |v_kd|"""
	c = R.Fwd(f"pv-{dt}", dt, 2, 2, 200, "causal", seed=7100)
	q, k, v, _ = R.fwd_operands(c)
	fref, ftol = R.fwd_reference(c, q, k, v, None)
	_, ptol = A.probs_reference(c, q, k)
	qkv, ld, hs, offs = qkv_buffer(c, q, k, v)
	P = run_probs(lib, c, qkv, ld, hs, offs, list(range(c.H)), (0, c.T, 0, c.T)).double()
	out = torch.full((c.nb * c.T, 64 * c.H), float("nan"), device=DEV, dtype=R.TDT[dt])
	d = _lib.AttnDesc()
	d.qkv, d.ld, d.q_off, d.k_off, d.v_off, d.head_stride = qkv.data_ptr(), ld, offs[0], offs[1], offs[2], hs
	d.out, d.ldo, d.nb, d.T, d.H, d.causal, d.scale, d.form = out.data_ptr(), 64 * c.H, c.nb, c.T, c.H, 1, R.SCALE, 0
	assert lib.ttk_attn_fwd(DT[dt], C.byref(d), _lib.stream_ptr()) == 0, lib.ttk_last_error().decode()
	torch.cuda.synchronize()
	fwd = out.cpu().double().view(c.nb, c.T, c.H, 64).permute(0, 2, 1, 3)      # [nb][H][T][64]
	pv = P @ v
	allowed = ftol.view(c.nb, c.T, c.H, 64).permute(0, 2, 1, 3) + ptol @ v.abs()
	r = ((pv - fwd).abs() / allowed).max().item()
	print(f"pv-{dt}: |P @ V - attn_fwd| / allowed {r:.3f}")
	assert r <= 1.0


@pytest.mark.parametrize("width", [1, 3, 7])
@pytest.mark.parametrize("Tt", [1, 2, 9])
@pytest.mark.parametrize("M", [1, 3, 7, 8, 37])
def test_align_prepare_against_f64(lib, M, Tt, width):
	rng = np.random.default_rng(1000 * M + 10 * Tt + width)
	blocks = rng.uniform(0.0, 1.0, size=(2, 3, M, Tt)).astype(np.float32)
	ref, tol = A.prepare_reference(blocks, width)
	a = torch.from_numpy(blocks).to(DEV)
	cost = torch.full((2, M, Tt), float("nan"), device=DEV)
	matrix = torch.full((2, M, Tt), float("nan"), device=DEV)
	assert lib.ttk_align_prepare(a.data_ptr(), 2, 3, M, Tt, width, cost.data_ptr(), matrix.data_ptr(), _lib.stream_ptr()) == 0, lib.ttk_last_error().decode()
	torch.cuda.synchronize()
	cost, matrix = cost.cpu().double().numpy(), matrix.cpu().double().numpy()
	assert np.array_equal(cost, -matrix)
	if Tt == 1:
		assert (matrix == 0).all()      # std 0: zeros
	err = np.abs(matrix - ref)
	assert (err <= tol).all(), f"M={M} Tt={Tt} width={width}: max err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}"


def run_dtw(lib, cost):
	"""cost f32 numpy [nb][M][Tt] -> (trace u8 [nb][M][Tt], total f32 [nb])"""
	nb, M, Tt = cost.shape
	c = torch.from_numpy(cost).to(DEV)
	D = torch.full((nb, (M + 1) * (Tt + 1)), float("nan"), device=DEV)
	trace = torch.full((nb, M, Tt), 255, device=DEV, dtype=torch.uint8)
	total = torch.full((nb,), float("nan"), device=DEV)
	assert lib.ttk_dtw(c.data_ptr(), nb, M, Tt, D.data_ptr(), trace.data_ptr(), total.data_ptr(), _lib.stream_ptr()) == 0, lib.ttk_last_error().decode()
	torch.cuda.synchronize()
	return trace.cpu().numpy(), total.cpu().numpy()


@pytest.mark.parametrize("M,Tt", [(1, 1), (1, 9), (9, 1), (37, 9), (255, 64), (257, 65), (606, 404)])
def test_dtw_is_numpy_bit_for_bit(lib, M, Tt):
	rng = np.random.default_rng(100 * M + Tt)
	blocks = rng.uniform(0.0, 1.0, size=(2, 2, M, Tt)).astype(np.float32)
	a = torch.from_numpy(blocks).to(DEV)
	cost = torch.empty((2, M, Tt), device=DEV)
	assert lib.ttk_align_prepare(a.data_ptr(), 2, 2, M, Tt, 7, cost.data_ptr(), None, _lib.stream_ptr()) == 0, lib.ttk_last_error().decode()
	cost = cost.cpu().numpy()      # the kernel's own cost
	cost[1] = np.round(cost[1] * 4) / 4      # sequence 1: a coarse grid, so that ties occur
	trace, total = run_dtw(lib, cost)
	for b in range(2):
		want_trace, want_total = A.dtw_reference(cost[b])
		assert np.array_equal(trace[b], want_trace), f"({M}, {Tt}) sequence {b}: {(trace[b] != want_trace).sum()} trace bytes differ"
		assert total[b].tobytes() == np.float32(want_total).tobytes()


def test_dtw_recovers_planted_paths(lib):
	"""all 200 planted cases of tests/test_align_ref.py: the kernels' path is numpy's on the kernel's own cost, and the planted one wherever numpy recovers it"""
	exact = 0
	for seed in range(200):
		blocks, tok = A.planted_case(seed)
		a = torch.from_numpy(blocks[None]).to(DEV)
		M, Tt = blocks.shape[1:]
		cost = torch.empty((1, M, Tt), device=DEV)
		assert lib.ttk_align_prepare(a.data_ptr(), 1, 3, M, Tt, 7, cost.data_ptr(), None, _lib.stream_ptr()) == 0
		cost = cost.cpu().numpy()
		trace, total = run_dtw(lib, cost)
		want_trace, want_total = A.dtw_reference(cost[0])
		assert np.array_equal(trace[0], want_trace) and total[0].tobytes() == np.float32(want_total).tobytes()
		ti, mi = alignment.backtrace(trace[0])
		nti, nmi, _, _ = A.align_reference(blocks)      # all numpy, float64 cost
		assert np.array_equal(ti, nti) and np.array_equal(mi, nmi), f"seed {seed}: the kernels' path is not numpy's"
		planted = ti.tolist() == tok.tolist() and mi.tolist() == list(range(M))
		assert planted or seed == 7, f"seed {seed}: the planted path is not recovered"      # (seed 7, 11 tokens: not the recurrence's optimum, test_align_ref.py)
		exact += planted
	assert exact == 199


# ----------------------------------------------------------------------------------------------------------- model level
FIXTURES = {"a": ("ar_attn_small", "small"), "c": ("ar_attn_small", "small"), "d": ("ar_attn_small", "small"), "peaked": ("ar_attn_peaked", "peaked"),
			"full": ("ar_attn_full", "full")}


def model_for(which, dtype):
	key = (which, dtype)
	if key not in _models:
		if which == "full" or len(_models) >= 4:
			_models.clear()
			gc.collect()
		cfg, seed = (W.AR_FULL, 42) if which == "full" else (W.AR_SMALL, 41)
		sd = W.synth_state_dict(W.ar_score_shapes(cfg), seed)
		if which == "peaked":
			sd = W.stress_ar(sd, cfg, "peaked")
		_models[key] = UnifiedVoice(sd, cfg, dtype=dtype, device=DEV, max_batch=4, max_ctx=160)
	return _models[key]


def fixture(case):
	g = np.load(os.path.join(GOLDEN, FIXTURES[case][0] + ".npz"))
	return {k: torch.from_numpy(g[f"{case}_{k}"]) for k in ("cond", "text", "codes", "maps", "dev32", "devbf16")}


@pytest.mark.parametrize("case,dtype", [("a", "f32"), ("a", "bf16"), ("c", "f32"), ("c", "bf16"), ("d", "f32"), ("d", "bf16"), ("peaked", "f32"), ("peaked", "bf16"),
										("full", "f32"), ("full", "bf16")])
def test_attention_maps_against_the_reference(case, dtype):
	"""f32: max |P - P_ref32| <= 4 x the stored max |P32 - P64| of that layer; bf16: <= 1.5 x the stored max |Pbf16 - P64|.
	Measured on MI355X, max |P - P_ref32| over the layers and the worst layer's share of its allowance: f32 a 4.2e-7 (0.30), c 4.5e-7 (0.34), d 4.8e-7 (0.32),
	peaked 1.0e-5 (0.32), full 1.9e-6 (0.80); bf16 a 2.8e-3 (0.49), c 2.8e-3 (0.48), d 2.9e-3 (0.60), peaked 6.9e-2 (0.64), full 7.8e-3 (0.77)."""
	f = fixture(case)
	model = model_for(FIXTURES[case][1], dtype)
	B, Tt = f["text"].shape
	M = f["codes"].shape[1]
	maps = model.attentions(f["cond"].to(DEV), f["text"].to(DEV), f["codes"].to(DEV))
	torch.cuda.synchronize()
	assert isinstance(maps, tuple) and len(maps) == model.cfg.layers
	got = torch.stack([m.cpu() for m in maps])
	S = Tt + M + 5
	assert got.shape == f["maps"].shape == (model.cfg.layers, B, model.cfg.heads, S, S) and got.dtype == torch.float32
	assert (torch.triu(got, 1) == 0).all() and (got.sum(-1) - 1).abs().max() < 1e-5
	dev = (got.double() - f["maps"].double()).abs().amax(dim=(1, 2, 3, 4))
	allowed = 4 * f["dev32"] if dtype == "f32" else 1.5 * f["devbf16"]
	print(f"{case} {dtype}: max |P - P_ref32| per layer up to {dev.max():.3e}; worst layer at {(dev / allowed).max():.3f} of its allowance")
	assert (dev <= allowed).all(), f"{case} {dtype}: layers {(dev > allowed).nonzero().flatten().tolist()} exceed their allowance: {dev.tolist()} vs {allowed.tolist()}"
	sub = model.attentions(f["cond"].to(DEV), f["text"].to(DEV), f["codes"].to(DEV), layers=[model.cfg.layers - 1, 0])      # a subset, in the caller's order
	assert len(sub) == 2 and torch.equal(sub[0].cpu(), got[-1]) and torch.equal(sub[1].cpu(), got[0])


@pytest.mark.parametrize("case", ["a", "d"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_text_attention_is_a_region_of_the_maps_and_alignment_is_numpys(case, dtype):
	f = fixture(case)
	model = model_for("small", dtype)
	cond, text, codes = f["cond"].to(DEV), f["text"].to(DEV), f["codes"].to(DEV)
	B, Tt = text.shape
	M = codes.shape[1]
	maps = torch.stack(model.attentions(cond, text, codes))      # [L][B][H][S][S]
	for heads in ([(1, 1), (0, 0), (1, 0), (1, 1)], None):
		sel = alignment.default_heads(model.cfg.layers, model.cfg.heads) if heads is None else heads
		blocks = model._text_attention(*model._dense_inputs(cond, text, codes), sel)
		want = torch.stack([maps[l, :, h, Tt + 3:Tt + 3 + M, 2:2 + Tt] for l, h in sel], 1)
		assert torch.equal(blocks, want), f"{case}: the text blocks of {sel} are not the maps' [Tt+3+m][2+t] region bit for bit"
		r = model.text_alignment(cond, text, codes, heads=heads)
		assert r["matrix"].shape == (B, M, Tt) and r["token_start"].shape == (B, Tt) and r["total"].shape == (B,)
		bl = blocks.cpu().numpy()
		for b in range(B):
			ti, mi, starts, total = A.align_reference(bl[b])
			# numpy on the kernel's own blocks: the f64 matrix decides the same path unless two candidate costs lie within the cost kernel's tolerance, so the
			# path is compared on the kernel's own cost, bit for bit, and the matrix against the restatement within its tolerance
			ref_m, tol_m = A.prepare_reference(bl[b:b + 1], 7)
			mat = r["matrix"][b].cpu().double().numpy()
			assert (np.abs(mat - ref_m[0]) <= tol_m[0]).all()
			trace, want_total = A.dtw_reference((-mat).astype(np.float32))
			wti, wmi = alignment.backtrace(trace)
			assert np.array_equal(r["path"][b][0], wti) and np.array_equal(r["path"][b][1], wmi)
			assert np.array_equal(r["token_start"][b], alignment.token_starts(wti, wmi, Tt)) and r["total"][b].tobytes() == np.float32(want_total).tobytes()
			assert (r["token_start"][b] >= 0).all() and (np.diff(r["token_start"][b]) >= 0).all() and r["token_start"][b][0] == 0
			assert np.array_equal(ti, wti) and np.array_equal(mi, wmi) and np.array_equal(starts, r["token_start"][b])      # ... and the all-numpy path is the same one
			assert abs(float(total) - float(want_total)) <= 1e-4 * max(1.0, abs(float(total)))


def test_nothing_else_changes(lib):
	"""forward(return_latent=True) and ids sampled with the captured token step are bit for bit the same before and after the maps and an alignment were taken"""
	f = fixture("a")
	model = model_for("small", "bf16")
	cond, text, codes = f["cond"].to(DEV), f["text"].to(DEV), f["codes"].to(DEV)
	B, Tt = text.shape
	args = (cond, text, torch.tensor([Tt] * B), codes, torch.tensor([codes.shape[1] * 1024] * B))
	lat0 = model.forward(*args, return_latent=True, clip_inputs=False).clone()
	ids0 = model.inference_speech(cond[:1], text[:1], do_sample=True, temperature=0.8, top_k=50, num_return_sequences=2, max_generate_length=12).clone()
	model.text_alignment(cond, text, codes)
	model.attentions(cond, text, codes)
	lat1 = model.forward(*args, return_latent=True, clip_inputs=False)
	ids1 = model.inference_speech(cond[:1], text[:1], do_sample=True, temperature=0.8, top_k=50, num_return_sequences=2, max_generate_length=12)
	assert torch.equal(lat0, lat1) and torch.equal(ids0, ids1)


def test_refusals(lib):
	f = fixture("a")
	model = model_for("small", "f32")
	cond, text, codes = f["cond"].to(DEV), f["text"].to(DEV), f["codes"].to(DEV)
	with pytest.raises(ValueError, match="head list is empty"):
		model.text_alignment(cond, text, codes, heads=[])
	with pytest.raises(ValueError, match="outside 2 layers x 2 heads"):
		model.text_alignment(cond, text, codes, heads=[(2, 0)])
	with pytest.raises(ValueError, match="median_width"):
		model.text_alignment(cond, text, codes, median_width=4)
	with pytest.raises(ValueError, match="layer list is empty"):
		model.attentions(cond, text, codes, layers=[])
	with pytest.raises(_lib.TTKError, match="selected twice"):
		model.attentions(cond, text, codes, layers=[1, 1])
	with pytest.raises(_lib.TTKError, match="outside"):
		model.attentions(cond, text, codes, layers=[2])
	with pytest.raises(NotImplementedError, match="return_attentions are not"):      # forward keeps its refusal (tests/test_gpu_ar_score.py pins it): the maps are `attentions`
		model.forward(cond, text, torch.tensor([7, 7]), codes, torch.tensor([9 * 1024] * 2), return_attentions=True)
	big = torch.zeros((1, 590), dtype=torch.int64)
	with pytest.raises(_lib.TTKError, match="select fewer layers"):      # 2 layers x 1 x 2 heads x 602^2 x 4 bytes is small: ask the C entry with a B that is not
		arr = (C.c_int * 2)(0, 1)
		_lib.check(lib.ttk_ar_attentions(model._h, cond.data_ptr(), text.data_ptr(), 7, big.to(DEV).data_ptr(), 590, 400, arr, 2, cond.data_ptr(), None), "ttk_ar_attentions")
	scores = model.rank_alignment_heads(cond, text, codes)
	assert sorted(h for h, _ in scores) == [(0, 0), (0, 1), (1, 0), (1, 1)] and all(a[1] >= b[1] for a, b in zip(scores, scores[1:]))


# ----------------------------------------------------------------------------------------------------------- TTS.inference(return_timings=True), TTS.align
HIFI_CFG = W.HiFiGANConfig(in_channels=128, cond_channels=128, upsample_initial_channel=128)      # tests/test_gpu_hifigan.py: hop 256 on AR_SMALL's latent width


@pytest.fixture(scope="module")
def small_tts():
	"""the small synthetic models of tests/test_gpu_tts.py (same shapes and seeds) plus the small HiFiGAN of tests/test_gpu_hifigan.py, a voice given as latents"""
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.hifigan import HiFiGAN
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	g = np.load(os.path.join(GOLDEN, "tokenizer.npz"))
	tok = VoiceBpeTokenizer(vocab={str(t): i for i, t in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	tts = TTS(UnifiedVoice(W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=160),
			  DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32), W.DIFF_SMALL, dtype="f32", device=DEV), tok,
			  vocoder=BigVGAN(W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33), W.VOC_SMALL, dtype="f32", device=DEV),
			  hifigan=HiFiGAN(W.synth_state_dict(W.hifigan_shapes(HIFI_CFG), 37), HIFI_CFG, dtype="f32", device=DEV))
	gen = torch.Generator().manual_seed(6)
	voice = {"latent": (torch.randn(1, W.AR_SMALL.model_dim, generator=gen).to(DEV), torch.randn(1, 2 * W.DIFF_SMALL.model_channels, generator=gen).to(DEV))}
	yield tts, voice
	del tts
	gc.collect()


@pytest.mark.parametrize("vocoder_type,text", [("bigvgan", "Hello there, Mr. Fox.\nThe end!"), ("bigvgan", "Hello there."), ("hifigan", "Hello there, Mr. Fox.\nThe end!")])
def test_tts_inference_returns_word_timings(small_tts, vocoder_type, text):
	tts, voice = small_tts
	kw = dict(max_ar_steps=12, max_diffusion_steps=3, seed=1234, vocoder_type=vocoder_type)
	if vocoder_type == "hifigan":
		kw.update(max_ar_steps=70, ar_temp=0.9, top_k=40, top_p=0.95, repetition_penalty=1.5)      # (tests/test_gpu_hifigan.py: long enough for a first chunk)
	wav0, sr0 = tts.inference(text, voice, **kw)
	wav, sr, timings = tts.inference(text, voice, return_timings=True, **kw)
	assert sr == sr0 == 24000 and torch.equal(wav, wav0)      # the audio is the call's without the argument, bit for bit
	lines = text.split("\n")
	assert len(timings) == len(lines) == len(tts.last_alignments)
	one = [tts.inference(line, voice, **kw)[0].shape[-1] for line in lines]      # each line's own samples
	assert sum(one) == wav.shape[-1]
	offset, per = 0.0, 1024 / 22050
	for line, t, al, n in zip(lines, timings, tts.last_alignments, one):
		words = tts.tokenizer.decode(tts.tokenizer.encode(line)).split()
		assert [w for w, _, _ in t] == words and len(words) >= 1      # one entry per word
		secs = n / 24000
		starts = [s for _, s, _ in t]
		assert all(b >= a for a, b in zip(starts, starts[1:]))
		assert all(offset <= s <= e <= offset + secs + 1e-9 for _, s, e in t)      # inside the line's audio, behind the lines before it
		codes = al["codes"]      # the row as it was sampled: stop tokens, if any, are still stop tokens
		assert codes.dim() == 2 and codes.shape[0] == 1 and al["token_start"].shape == (1, len(tts.tokenizer.encode(line)))
		alone = tts.align(line, codes, voice)
		assert t == [(w, min(s, secs) + offset, min(e, secs) + offset) for w, s, e in alone]
		assert alone[0][1] == 0.0 and alone[-1][2] == codes.shape[1] * per
		offset += secs
	if vocoder_type == "bigvgan":      # the hot path's own arguments: the same alignment, and the row is the sampled one, not the rewritten one
		from tortoise_tts_amd.inference import fix_stop_tokens
		from tortoise_tts_amd.tts import set_seed
		set_seed(1234)
		tokens = [tts.encode_text(line).to(DEV)[None] for line in lines]
		hk = dict(max_ar_steps=12, max_diffusion_steps=3, return_timings=True)
		res = tts.hot.inference_lines(tokens, *voice["latent"], **hk) if len(lines) > 1 else [tts.hot.inference(tokens[0], *voice["latent"], return_all=True, **hk)]
		for r, al in zip(res, tts.last_alignments):
			assert torch.equal(r[-1]["codes"], al["codes"]) and np.array_equal(r[-1]["token_start"], al["token_start"])
			fixed = r[2] if len(lines) > 1 else r[2]["codes"]
			assert torch.equal(fix_stop_tokens(al["codes"], tts.hot.autoregressive.stop_mel_token), fixed[:1])
		heads = [(1, 0)]
		_, _, t1 = tts.inference(text, voice, return_timings=True, alignment_heads=heads, **kw)
		assert t1[0] == [(w, min(s, one[0] / 24000), min(e, one[0] / 24000)) for w, s, e in tts.align(lines[0], tts.last_alignments[0]["codes"], voice, alignment_heads=heads)]
	with pytest.raises(ValueError, match="one line"):
		tts.align("a\nb", tts.last_alignments[0]["codes"], voice)
