"""DiscreteVAE on libttk (`ttk_dvae_*`, csrc/dvae.hip) against the reference's own class (tests/golden/dvae_*.npz, written by tools/make_golden_dvae.py
from models/dvae.py) and the CPU oracle (tests/dvae_oracle.py); the quantizer alone on adversarial rows; the `mel.encode` / `TTS` wiring.  GPU only.

Tolerances.
  f32: the convention of test_gpu_hifigan / test_gpu_univnet for the f32 result of a chain of segment-GEMM convolutions -- max |error| < 1e-4 of full
       scale.  Their waveforms have full scale 1; z, the decoded mel and the hidden activation do not, so the bound is 1e-4 x max |reference|.
  bf16 / f16: relative L2 against the reference's f32 result <= 1.5 x the relative L2 of the reference's OWN torch.autocast result, stored in the fixture.
  codes: the near-tie criterion of tests/dvae_oracle.py (gap / tau from the fixture; for the quantizer-alone cases derived the same way in the test).
"""
import math

import numpy as np
import pytest
import torch

import dvae_oracle as DO
from tortoise_tts_amd import _lib
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFGS = {"dvae_small": (W.DVAE_SMALL, ("1x5", "1x61", "3x64")), "dvae_full": (W.DVAE_FULL, ("1x517", "2x64"))}
CASES = [(n, tag) for n, (_, tags) in CFGS.items() for tag in tags]
_sd, _handles = {}, {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def rel_l2(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def weights_of(golden, name):
	if name not in _sd:
		g = golden(name)
		cfg = CFGS[name][0]
		sd = W.synth_state_dict(W.dvae_shapes(cfg), int(g["seed"]))
		sd["codebook.embed"] = W.dvae_codebook(t(g["cb_mean"]), t(g["cb_std"]), cfg.num_tokens, int(g["cb_seed"]))
		_sd[name] = (g, sd)
	return _sd[name]


def handle(golden, name, dtype):
	"""one handle per (config, dtype) for the whole module"""
	from tortoise_tts_amd.dvae import DiscreteVAE
	if (name, dtype) not in _handles:
		_, sd = weights_of(golden, name)
		_handles[(name, dtype)] = DiscreteVAE(sd, CFGS[name][0], dtype=dtype, device=DEV)
	return _handles[(name, dtype)]


def f32_close(got, ref, what):
	e, bound = maxerr(got, ref), 1e-4 * float(np.abs(np.asarray(ref)).max())
	print(f"{what}: f32 max error {e:.3e} (bound {bound:.3e})")
	return e < bound


def low_close(got, ref, ref_low, what):
	e, bound = rel_l2(got, ref), 1.5 * rel_l2(ref_low, ref)
	print(f"{what}: rel L2 {e:.3e} (bound {bound:.3e} = 1.5 x the reference's autocast error)")
	return e <= bound


def fixture_mel(g, cfg, tag):
	B, T = (int(v) for v in tag.split("x"))
	return DO.fixture_mel(B, T, int(g[f"input_seed_{tag}"]), cfg.channels)


# ------------------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("name,tag", CASES)
def test_encoder_f32_matches_the_reference(golden, name, tag):
	g, _ = weights_of(golden, name)
	cfg = CFGS[name][0]
	codes, z = handle(golden, name, "f32").encode(fixture_mel(g, cfg, tag).to(DEV))
	B, T = (int(v) for v in tag.split("x"))
	assert z.shape == (B, cfg.code_frames(T), cfg.codebook_dim) and codes.shape == z.shape[:2] and codes.dtype == torch.int64
	assert f32_close(z[:, ::int(g["z_step"])], g[f"z_{tag}"], f"{name} {tag} z")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,tag", CASES)
def test_encoder_16bit_within_the_references_autocast_error(golden, name, tag, dtype):
	g, _ = weights_of(golden, name)
	cfg = CFGS[name][0]
	_, z = handle(golden, name, dtype).encode(fixture_mel(g, cfg, tag).to(DEV))
	assert low_close(z[:, ::int(g["z_step"])], g[f"z_{tag}"], g[f"z_{dtype}_{tag}"], f"{name} {tag} {dtype} z")


@pytest.mark.parametrize("name,tag", CASES)
def test_codes_f32_equal_the_references_outside_near_ties(golden, name, tag):
	g, sd = weights_of(golden, name)
	cfg = CFGS[name][0]
	dv = handle(golden, name, "f32")
	mel = fixture_mel(g, cfg, tag).to(DEV)
	codes = dv.get_codebook_indices(mel).cpu().reshape(-1)
	ref = t(g[f"codes_{tag}"]).reshape(-1)
	gap, tau, tie = t(g[f"gap_{tag}"]), float(g[f"tau_{tag}"]), t(g[f"tie_idx_{tag}"]).long()
	assert codes.min() >= 0 and codes.max() < cfg.num_tokens
	clear = gap >= tau
	wrong = int((codes[clear] != ref[clear]).sum())
	share = float((~clear).double().mean())
	excess = 0.0
	if tie.numel():       # the chosen code's float64 distance from the FIXTURE's z rows, against the best
		d64 = DO.distances64(t(g[f"z_tie_{tag}"]), sd["codebook.embed"])
		excess = (d64.gather(1, codes[tie].reshape(-1, 1)).squeeze(1) - d64.min(1).values).max().item()
	print(f"{name} {tag}: {wrong} of {int(clear.sum())} clear positions differ; near ties {share:.4f}, worst excess {excess:.3e} (tau {tau:.3e})")
	assert wrong == 0 and excess <= tau and share <= 0.02


# ------------------------------------------------------------------------------------------------------------ quantizer alone
def copy_codes(cfg):
	"""codes 0, num_tokens - 1 and one inside every workgroup's 64-code range (a different offset in each)"""
	from tortoise_tts_amd.dvae import QUANT_CODES_PER_WORKGROUP as R
	per_range = [min(R * w + (7 * w + 3) % R, cfg.num_tokens - 1) for w in range((cfg.num_tokens + R - 1) // R)]
	return [0, cfg.num_tokens - 1] + per_range


def quant_check(dv, z, embed, what):
	"""codes of ttk_dvae_quantize == float64 argmin wherever its margin is at least 4 x the f32 distance error on these rows; two runs bit-identical"""
	codes = dv.quantize(z.to(DEV))
	again = dv.quantize(z.to(DEV))
	assert torch.equal(codes, again)
	codes = codes.cpu()
	d64 = DO.distances64(z, embed)
	gap, thr = DO.gap_and_tau(z, embed)
	best = d64.argmin(1)
	clear = gap >= thr
	print(f"{what}: {int((codes[clear] != best[clear]).sum())} of {int(clear.sum())} clear rows differ from the float64 argmin (threshold {thr:.3e}, min gap {gap.min().item():.3e})")
	assert codes.shape == (z.shape[0],) and codes.min() >= 0 and codes.max() < embed.shape[1]
	assert torch.equal(codes[clear], best[clear])
	excess = d64.gather(1, codes.reshape(-1, 1)).squeeze(1) - d64.min(1).values
	assert (excess[~clear] <= thr).all()
	return codes


@pytest.mark.parametrize("M", [1, 15, 17, 63, 65, 130])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_quantizer_alone_seeded_rows(golden, name, M):
	g, sd = weights_of(golden, name)
	cfg = CFGS[name][0]
	embed = sd["codebook.embed"]
	gen = torch.Generator().manual_seed(1000 + M)
	z = t(g["cb_mean"])[None] + t(g["cb_std"])[None] * torch.randn(M, cfg.codebook_dim, generator=gen)
	ends = [cfg.num_tokens - 1, 0][:min(2, M)]
	for i, j in enumerate(ends):              # the last rows: exact copies of the last and the first code vector
		z[M - 1 - i] = embed[:, j]
	codes = quant_check(handle(golden, name, "f32"), z.contiguous(), embed, f"{name} M={M}")
	assert [int(codes[M - 1 - i]) for i in range(len(ends))] == ends


@pytest.mark.parametrize("name", sorted(CFGS))
def test_quantizer_alone_copies_of_code_vectors(golden, name):
	_, sd = weights_of(golden, name)
	cfg = CFGS[name][0]
	embed = sd["codebook.embed"]
	want = copy_codes(cfg)
	z = embed[:, want].t().contiguous()
	codes = quant_check(handle(golden, name, "f32"), z, embed, f"{name} copies")
	assert codes.tolist() == want


def test_quantizer_ties_go_to_the_lowest_index(golden):
	"""identical columns j < k in one 16-code tile, in two waves of one workgroup, and in two workgroups: every row nearest to them returns j"""
	from tortoise_tts_amd.dvae import DiscreteVAE
	_, sd = weights_of(golden, "dvae_small")
	cfg = W.DVAE_SMALL
	sd = dict(sd)
	embed = sd["codebook.embed"].clone()
	pairs = [(17, 20), (70, 100), (5, 150), (64, 199)]
	for j, k in pairs:
		embed[:, k] = embed[:, j]
	sd["codebook.embed"] = embed
	dv = DiscreteVAE(sd, cfg, dtype="f32", device=DEV)
	gen = torch.Generator().manual_seed(5)
	rows = [embed[:, j] for j, _ in pairs] + [embed[:, j] + 1e-3 * torch.randn(cfg.codebook_dim, generator=gen) for j, _ in pairs]
	z = torch.stack(rows).contiguous()
	codes = dv.quantize(z.to(DEV))
	assert torch.equal(codes, dv.quantize(z.to(DEV)))
	assert codes.cpu().tolist() == [j for j, _ in pairs] * 2


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_16bit_handles_quantize_in_f32(golden, name, dtype):
	"""the z a 16-bit handle's encoder returns, fed back through the quantizer alone, reproduces the codes the encode call returned"""
	g, _ = weights_of(golden, name)
	cfg, tags = CFGS[name]
	dv = handle(golden, name, dtype)
	codes, z = dv.encode(fixture_mel(g, cfg, tags[-1]).to(DEV))
	assert torch.equal(dv.quantize(z), codes)
	assert torch.equal(handle(golden, name, "f32").quantize(z), codes)         # and it is the same f32 quantizer in every handle


# ------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name,tag", CASES)
def test_decode_matches_the_reference(golden, name, tag, dtype):
	g, _ = weights_of(golden, name)
	cfg = CFGS[name][0]
	codes = t(g[f"codes_{tag}"])
	mel, hidden = handle(golden, name, dtype).decode(codes.to(DEV))
	B, n = codes.shape
	assert mel.shape == (B, cfg.channels, 4 * n) and hidden.shape == (B, cfg.hidden_dim, 4 * n) and mel.dtype == hidden.dtype == torch.float32
	mel, hidden = mel[..., ::int(g["mel_step"])], hidden[..., ::int(g["hidden_step"])]
	if dtype == "f32":
		assert f32_close(mel, g[f"dec_mel_{tag}"], f"{name} {tag} mel") and f32_close(hidden, g[f"dec_hidden_{tag}"], f"{name} {tag} hidden")
	else:
		assert low_close(mel, g[f"dec_mel_{tag}"], g[f"dec_mel_{dtype}_{tag}"], f"{name} {tag} {dtype} mel")
		assert low_close(hidden, g[f"dec_hidden_{tag}"], g[f"dec_hidden_{dtype}_{tag}"], f"{name} {tag} {dtype} hidden")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 16])
def test_decode_edge_shapes_vs_oracle(golden, n, B):
	"""n = 1: both neighbours of both upsampled convolutions are padding; B = 3: the tap shifts must not cross batch elements"""
	_, sd = weights_of(golden, "dvae_small")
	cfg = W.DVAE_SMALL
	codes = DO.fixture_codes(B, n, 10 * n + B, cfg.num_tokens)
	with torch.inference_mode():
		ref_mel, ref_hidden = DO.DVAEOracle(sd, cfg, torch.float64).decode(codes)
	mel, hidden = handle(golden, "dvae_small", "f32").decode(codes.to(DEV))
	assert mel.shape == ref_mel.shape == (B, cfg.channels, 4 * n) and hidden.shape == ref_hidden.shape == (B, cfg.hidden_dim, 4 * n)
	assert f32_close(mel, ref_mel.numpy(), f"n={n} B={B} mel") and f32_close(hidden, ref_hidden.numpy(), f"n={n} B={B} hidden")


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 9])
def test_encode_edge_lengths_vs_oracle(golden, T):
	"""the shortest clips: odd and even lengths through both stride-2 layers, down to one frame"""
	_, sd = weights_of(golden, "dvae_small")
	cfg = W.DVAE_SMALL
	mel = DO.fixture_mel(3, T, 50 + T, cfg.channels)
	with torch.inference_mode():
		ref = DO.DVAEOracle(sd, cfg, torch.float64).encode(mel)
	_, z = handle(golden, "dvae_small", "f32").encode(mel.to(DEV))
	assert z.shape == ref.shape == (3, cfg.code_frames(T), cfg.codebook_dim) and f32_close(z, ref.numpy(), f"T={T} z")


def test_infer_is_decode_of_the_codes(golden):
	g, _ = weights_of(golden, "dvae_small")
	dv = handle(golden, "dvae_small", "f32")
	mel = t(g["mel_3x64"]).to(DEV)
	a, b = dv.infer(mel), dv.decode(dv.get_codebook_indices(mel))
	assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (3, 80, 64)


@pytest.mark.parametrize("bad", ["num_tokens", -1])
def test_decode_refuses_a_code_out_of_range(golden, bad):
	dv = handle(golden, "dvae_small", "f32")
	codes = torch.zeros((2, 5), dtype=torch.int64)
	codes[1, 3] = dv.cfg.num_tokens if bad == "num_tokens" else bad
	with pytest.raises(_lib.TTKError, match="outside"):
		dv.decode(codes.to(DEV))
	mel = torch.full((2, 80, 20), 7.0, device=DEV)         # and through the C ABI: the outputs are untouched, nothing was launched
	rc = dv.lib.ttk_dvae_decode(dv._h, codes.to(DEV).data_ptr(), 2, 5, mel.data_ptr(), None, _lib.stream_ptr())
	torch.cuda.synchronize()
	assert rc == -1 and bool((mel == 7.0).all())
	good = dv.decode(torch.zeros((2, 5), dtype=torch.int64, device=DEV))[0]
	assert torch.isfinite(good).all()


def test_forward_and_bad_arguments_are_refused(golden):
	dv = handle(golden, "dvae_small", "f32")
	with pytest.raises(NotImplementedError, match="training"):
		dv(torch.zeros(1, 80, 8))
	with pytest.raises(_lib.TTKError):
		dv.get_codebook_indices(torch.zeros(1, 79, 8))
	with pytest.raises(_lib.TTKError):
		dv.quantize(torch.zeros(4, 31))
	assert dv.eval() is dv and dv.to("cuda") is dv


# ------------------------------------------------------------------------------------------------------------ mel.encode / TTS
def clip(seed=9, n=30000):
	tt = torch.arange(n) / 22050
	return (0.3 * torch.sin(2 * math.pi * 180 * tt) + 0.02 * torch.randn(n, generator=torch.Generator().manual_seed(seed)))[None]


@pytest.fixture(scope="module")
def parts(golden):
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(v): i for i, v in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	common = dict(conditioning_encoder=ConditioningEncoder(W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35), W.AR_SMALL, dtype="f32", device=DEV),
				  contextual_embedder=ContextualEmbedder(W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36), W.DIFF_SMALL, dtype="f32", device=DEV),
				  tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV))
	ar = UnifiedVoice(W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), W.AR_SMALL, dtype="f32", device=DEV, max_batch=4, max_ctx=96)
	df = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 32), W.DIFF_SMALL, dtype="f32", device=DEV)
	dv = handle(golden, "dvae_small", "f32")
	return TTS(ar, df, tok, dvae=dv, **common), TTS(ar, df, tok, **common), dv


def test_tts_encode_audio_returns_the_clips_codes(parts):
	from tortoise_tts_amd import mel as M
	tts, bare, dv = parts
	enc = tts.encode_audio(clip(), 22050)
	whole = M.format_autoregressive_conditioning(M.resample(clip(), 22050, 22050, device=DEV), tts.tms, cond_length=0)
	assert whole.shape == (1, 80, 30000 // 256 + 1)
	assert enc["codes"].shape == (1, W.DVAE_SMALL.code_frames(whole.shape[-1])) and torch.equal(enc["codes"], dv.get_codebook_indices(whole))
	plain = bare.encode_audio(clip(), 22050)
	assert sorted(plain) == ["conds", "latent", "metadata"] and sorted(enc) == ["codes", "conds", "latent", "metadata"]
	assert torch.equal(plain["latent"][0], enc["latent"][0]) and torch.equal(plain["conds"][1], enc["conds"][1])
	several = tts.encode_audio([clip(), clip(11, 20000)], 22050)
	assert isinstance(several["codes"], list) and len(several["codes"]) == 2 and torch.equal(several["codes"][0], enc["codes"])
	assert several["codes"][1].shape == (1, W.DVAE_SMALL.code_frames(20000 // 256 + 1))


def test_continuation_from_a_waveform(parts):
	"""the codes of a clip are a prompt `inference_speech(input_tokens=)` continues from"""
	tts, _, _ = parts
	enc = tts.encode_audio(clip(), 22050)
	prompt = enc["codes"][:, :8]
	ar = tts.hot.autoregressive
	text = torch.randint(1, 255, (1, 7), generator=torch.Generator().manual_seed(1)).to(DEV)
	with torch.inference_mode():
		ids = ar.inference_speech(enc["latent"][0], text, input_tokens=prompt, num_return_sequences=1, max_generate_length=20, do_sample=True, temperature=0.8,
								  top_k=0, suppress_tokens=[8193])
	assert ids.shape[1] > 8 and torch.equal(ids[:, :8], prompt.expand(ids.shape[0], -1))
