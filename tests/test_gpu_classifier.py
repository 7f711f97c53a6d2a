"""The TorToiSe detector on libttk (`ttk_cls_*`, csrc/classifier.hip) against the reference's own class (tests/golden/classifier_*.npz, written by
tools/make_golden_classifier.py from models/classifier.py); the fused k = 5 convolution and the split GroupNorm statistics alone; repeatability;
`TTS.classify_audio_clip`.  GPU only.

Tolerances.
  f32: the convention of tests/test_gpu_cond.py for this block chain -- max |error| <= 5e-4 x max(1, max |reference|), on the embedding, the logits and
       every stored activation (the stem, each stage behind its Downsample, enc.final).
  bf16: relative L2 of the embedding <= 1.5 x the relative L2 of the reference's OWN torch.autocast(bfloat16) embedding against its f32 one, and the
       logits' maximum deviation <= 1.5 x the reference's own; both from the fixture.  1.5 is the margin this project gives a 16-bit mode.
  the convolution alone: against F.conv1d in float64 on silu(groupnorm(x)) built from the SAME f32 statistics; f32 as above, bf16 relative L2 <= 1.5 x
       that of the same float64 convolution on operands rounded to bf16.
  statistics: (mean, rstd) against torch.var_mean in float64 within 1e-6 relative, the mean with a 1e-6 absolute floor.
"""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_oracle as CO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(n, tag) for n, (_, tags) in CO.CFGS.items() for tag in tags]
_sd, _handles, _runs = {}, {}, {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def rel_l2(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def f32_close(got, ref, what):
	ref = torch.as_tensor(ref)
	e, bound = maxerr(got, ref), 5e-4 * max(1.0, ref.abs().max().item())
	print(f"{what}: f32 max error {e:.3e} (bound {bound:.3e})")
	return tuple(got.shape) == tuple(ref.shape) and e <= bound


def weights_of(golden, name):
	if name not in _sd:
		g = golden(name)
		_sd[name] = (g, W.synth_state_dict(W.classifier_shapes(CO.CFGS[name][0]), int(g["seed"])))
	return _sd[name]


def handle(golden, name, dtype):
	"""one handle per (config, dtype) for the whole module"""
	from tortoise_tts_amd.classifier import AudioMiniEncoderWithClassifierHead
	if (name, dtype) not in _handles:
		_, sd = weights_of(golden, name)
		_handles[(name, dtype)] = AudioMiniEncoderWithClassifierHead(sd, CO.CFGS[name][0], dtype=dtype, device=DEV)
	return _handles[(name, dtype)]


def audio_of(g, tag):
	B, T = (int(v) for v in tag.split("x"))
	return CO.fixture_audio(B, T, int(g[f"input_seed_{tag}"]))


def run(golden, name, tag, dtype):
	"""(emb, logits, activations) of one fixture case, computed once per module"""
	key = (name, tag, dtype)
	if key not in _runs:
		g, _ = weights_of(golden, name)
		emb, logits, acts = handle(golden, name, dtype).forward_with_intermediates(audio_of(g, tag).to(DEV))
		_runs[key] = (emb.cpu(), logits.cpu(), [a.cpu() for a in acts])
	return _runs[key]


# ------------------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("name,tag", CASES)
def test_f32_matches_the_reference_stage_by_stage(golden, name, tag):
	g, _ = weights_of(golden, name)
	cfg = CO.CFGS[name][0]
	B, T = (int(v) for v in tag.split("x"))
	emb, logits, acts = run(golden, name, tag, "f32")
	assert emb.dtype == logits.dtype == torch.float32 and len(acts) == cfg.depth + 2
	ok = f32_close(emb, g[f"emb_{tag}"], f"{name} {tag} emb") & f32_close(logits, g[f"logits_{tag}"], f"{name} {tag} logits")
	for k, a in zip(CO.activation_names(cfg), acts):
		ok &= f32_close(a[..., ::int(g[f"step_{k}_{tag}"])], g[f"{k}_{tag}"], f"{name} {tag} {k}")
	assert ok
	dv = handle(golden, name, "f32")
	x = audio_of(g, tag).to(DEV)
	assert torch.equal(dv(x).cpu(), logits) and torch.equal(dv.encode(x).cpu(), emb)      # forward / encode are the same launches without the copies


@pytest.mark.parametrize("name,tag", CASES)
def test_bf16_within_the_references_autocast_error(golden, name, tag):
	g, _ = weights_of(golden, name)
	emb, logits, _ = run(golden, name, tag, "bf16")
	ref_e, ref_l = t(g[f"emb_{tag}"]), t(g[f"logits_{tag}"])
	e, be = rel_l2(emb, ref_e), 1.5 * rel_l2(g[f"emb_bf16_{tag}"], ref_e)
	d, bd = maxerr(logits, ref_l), 1.5 * maxerr(g[f"logits_bf16_{tag}"], ref_l)
	print(f"{name} {tag} bf16: emb rel L2 {e:.3e} (bound {be:.3e}), logits max deviation {d:.3e} (bound {bd:.3e}); both bounds 1.5 x the reference's autocast error")
	assert e <= be and d <= bd


# ------------------------------------------------------------------------------------------------------------ the fused convolution alone
def conv_case(C, L, B, seed):
	gen = torch.Generator().manual_seed(seed)
	x = torch.randn(B, L, C, generator=gen) * 1.3 + 0.4 * torch.randn(1, 1, C, generator=gen)
	w = torch.randn(C, C, 5, generator=gen) / math.sqrt(5 * C)
	bias, gamma, beta = 0.1 * torch.randn(C, generator=gen), 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
	res = torch.randn(B, L, C, generator=gen)
	return x, w, bias, gamma, beta, res


def conv_reference(x, w, bias, stats, gamma, beta, res, round_bf16):
	"""float64 F.conv1d on channels-first operands; with `stats` (f32 [B, G, 2]) the input is silu(gn(x)) from exactly those statistics"""
	a = x.double()
	if stats is not None:
		B, L, C = x.shape
		G = stats.shape[1]
		mean, rstd = (stats.double()[:, :, i].repeat_interleave(C // G, dim=1)[:, None, :] for i in (0, 1))
		a = F.silu((a - mean) * rstd * gamma.double() + beta.double())
	wd = w.double()
	if round_bf16:
		a, wd = a.float().bfloat16().double(), w.bfloat16().double()
	y = F.conv1d(a.transpose(1, 2), wd, bias.double(), padding=2).transpose(1, 2)
	return y if res is None else y + res.double()


@pytest.mark.parametrize("L", [1, 3, 255, 257])
@pytest.mark.parametrize("C", [32, 64])
def test_conv5_rows_alone(C, L):
	"""B = 2: a halo read across the batch boundary would show in row 0 / row L - 1 of either element; 255 / 257 straddle the tile edges"""
	from tortoise_tts_amd.classifier import conv5_rows, gn_stats
	x, w, bias, gamma, beta, res = conv_case(C, L, 2, 100 * C + L)
	d = lambda v: v.to(DEV)
	stats = gn_stats(d(x), CO.groups_of(C))
	ok = True
	for use_gn in (True, False):
		for use_res in (True, False):
			kw = dict(residual=d(res) if use_res else None)
			if use_gn:
				kw.update(stats=stats, gamma=d(gamma), beta=d(beta))
			ref = conv_reference(x, w, bias, stats.cpu() if use_gn else None, gamma, beta, res if use_res else None, False)
			low = conv_reference(x, w, bias, stats.cpu() if use_gn else None, gamma, beta, res if use_res else None, True)
			what = f"C={C} L={L} gn={use_gn} residual={use_res}"
			got = conv5_rows(d(x), d(w), d(bias), dtype="f32", **kw)
			assert torch.equal(got, conv5_rows(d(x), d(w), d(bias), dtype="f32", **kw))
			ok &= f32_close(got.cpu(), ref, what)
			got16 = conv5_rows(d(x), d(w), d(bias), dtype="bf16", **kw)
			e, bound = rel_l2(got16, ref), 1.5 * rel_l2(low, ref)
			print(f"{what}: bf16 rel L2 {e:.3e} (bound {bound:.3e} = 1.5 x the bf16-rounded float64 convolution's)")
			ok &= e <= bound
	assert ok


def test_conv5_rows_refuses_what_it_has_no_instantiation_for():
	from tortoise_tts_amd.classifier import conv5_rows
	x, w, b = torch.zeros(1, 8, 128, device=DEV), torch.zeros(128, 128, 5, device=DEV), torch.zeros(128, device=DEV)
	with pytest.raises(_lib.TTKError, match="32 or 64"):
		conv5_rows(x, w, b)


# ------------------------------------------------------------------------------------------------------------ split statistics
@pytest.mark.parametrize("C,G,T", [(32, 16, 1), (32, 16, 5), (32, 16, 24000), (64, 16, 1), (64, 16, 5), (64, 16, 24000), (128, 32, 5), (128, 32, 700), (256, 32, 700),
								   (512, 32, 5), (512, 32, 700), (1024, 32, 1), (1024, 32, 5), (1024, 32, 700)])
def test_split_statistics_vs_float64(C, G, T):
	"""channels per group 2, 4, 8, 16, 32; T below one chunk and over many (24000 rows of 32 channels are 12 chunks, 700 of 1024 are 11)"""
	from tortoise_tts_amd.classifier import gn_stats
	gen = torch.Generator().manual_seed(C + T)
	x = (torch.randn(2, T, C, generator=gen) * 1.5 + 0.7 + torch.randn(1, 1, C, generator=gen)).to(DEV)
	got = gn_stats(x, G)
	assert torch.equal(got, gn_stats(x, G))
	var, mean = torch.var_mean(x.double().reshape(2, T, G, C // G), dim=(1, 3), unbiased=False)
	rstd = 1 / torch.sqrt(var + 1e-5)
	em = ((got[..., 0].double() - mean).abs() / (1e-6 + 1e-6 * mean.abs())).max().item()
	er = ((got[..., 1].double() - rstd).abs() / (1e-6 * rstd)).max().item()
	print(f"C={C} G={G} T={T}: mean error {em:.3f} x bound, rstd error {er:.3f} x bound")
	assert got.shape == (2, G, 2) and em <= 1.0 and er <= 1.0


# ------------------------------------------------------------------------------------------------------------ repeatability
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_repeatable_and_independent_of_the_batch(golden, dtype):
	g, _ = weights_of(golden, "classifier_small")
	dv = handle(golden, "classifier_small", dtype)
	x = audio_of(g, "2x4099").to(DEV)
	emb, logits, _ = run(golden, "classifier_small", "2x4099", dtype)
	e2, l2, _ = dv.forward_with_intermediates(x)
	assert torch.equal(e2.cpu(), emb) and torch.equal(l2.cpu(), logits)
	for b in range(2):
		assert torch.equal(dv(x[b:b + 1]).cpu(), logits[b:b + 1]) and torch.equal(dv.encode(x[b:b + 1]).cpu(), emb[b:b + 1])


# ------------------------------------------------------------------------------------------------------------ TTS.classify_audio_clip
def tts_with(classifier):
	from tortoise_tts_amd.tts import TTS
	return TTS(types.SimpleNamespace(device=torch.device(DEV)), None, None, classifier=classifier)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_classify_audio_clip_is_softmax_of_the_logits(golden, dtype):
	g, _ = weights_of(golden, "classifier_small")
	tts = tts_with(handle(golden, "classifier_small", dtype))
	tag = "1x24000"
	clip = audio_of(g, tag)[0]
	ref = torch.softmax(t(g[f"logits_{tag}"]).double(), dim=-1)[0, 0].item()
	p, p1 = tts.classify_audio_clip(clip), tts.classify_audio_clip(clip[0], sr=24000)
	# |d softmax| <= max |d logit| / 2 for two classes and <= max |d logit| in general: the logits' bound carries over
	bound = 5e-4 * max(1.0, float(np.abs(g[f"logits_{tag}"]).max())) if dtype == "f32" else 1.5 * maxerr(g[f"logits_bf16_{tag}"], g[f"logits_{tag}"])
	print(f"{dtype}: P(generated) {p:.6f}, reference {ref:.6f} (bound {bound:.3e})")
	assert isinstance(p, float) and p == p1 and abs(p - ref) <= bound


def test_classify_audio_clip_resamples_and_refuses(golden):
	g, _ = weights_of(golden, "classifier_small")
	dv = handle(golden, "classifier_small", "f32")
	tts = tts_with(dv)
	n = 11025
	clip = (0.3 * torch.sin(2 * math.pi * 220 * torch.arange(n) / 22050))[None]
	p = tts.classify_audio_clip(clip, sr=22050)
	assert 0.0 < p < 1.0
	with pytest.raises(ValueError, match="classifier="):
		tts_with(None).classify_audio_clip(clip)
	from tortoise_tts_amd.classifier import MAX_POSITIONS
	limit = MAX_POSITIONS * 4 ** W.CLASSIFIER_SMALL.depth      # the longest clip whose last stage fits the row-wave attention
	with pytest.raises(_lib.TTKError, match=str(MAX_POSITIONS)):
		dv(torch.zeros(1, 1, limit + 1))
	with pytest.raises(NotImplementedError, match="training loss"):
		dv(clip[None], torch.zeros(1, dtype=torch.int64))
	with pytest.raises(_lib.TTKError):
		dv(torch.zeros(1, 2, 100))
