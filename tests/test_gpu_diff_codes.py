"""Token conditioning of the diffusion model on the HIP path: `DiffusionTTS.timestep_independent` / `forward` on integer mel codes and `mel_head`
(ttk_diff_precompute_codes, ttk_diff_mel_head) against the reference's own results (tests/golden/diff_codes_*.npz) and the CPU restatement
(tests/diff_codes_oracle.py), and the user level built on it: `TTSHotPath.inference(diffusion_conditioning="codes")`, `TTS.decode_codes`, `TTS.resynthesize`.
GPU only.  Bounds are the latent path's (tests/test_gpu_parity.py, test_gpu_fp16.py, test_gpu_fp8.py): the same block kinds, one block fewer."""
import numpy as np
import pytest
import torch

import diff_codes_oracle as DC
from test_gpu_tts import speechlike
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_models, _sds = {}, {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item()


def relerr(a, b):
	a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
	return ((a - b).norm() / b.norm()).item()


def weights_of(cfg, seed, in_tokens):
	key = (cfg, seed, in_tokens)
	if key not in _sds:
		_sds[key] = DC.state_dict(cfg, seed, in_tokens)
	return _sds[key]


def model_of(cfg, seed, in_tokens, dtype):
	"""one handle per (config, seed, table size, dtype) for the whole module"""
	from tortoise_tts_amd.diffusion import DiffusionTTS
	key = (cfg, seed, in_tokens, dtype)
	if key not in _models:
		_models[key] = DiffusionTTS(weights_of(cfg, seed, in_tokens), cfg, dtype=dtype, device=DEV, codes=True)
	return _models[key]


def fixture_model(golden, name, cfg, dtype):
	g = golden(name)
	return g, model_of(cfg, int(g["seed"]), int(g["in_tokens"]), dtype)


# ------------------------------------------------------------------------------------------------ f32 against the reference
@pytest.mark.parametrize("name,cfg,latent_name,bE,bY", [("diff_codes_small", W.DIFF_SMALL, "diff_small", 1e-4, 2e-4), ("diff_codes_full", W.DIFF_FULL, "diff_full", 5e-4, 1e-3)])
def test_f32_vs_reference_fixture(golden, name, cfg, latent_name, bE, bY):
	from tortoise_tts_amd.diffusion import get_diffuser
	g, model = fixture_model(golden, name, cfg, "f32")
	codes, cond, T = t(g["codes"]).to(DEV), t(g["cond"]).to(DEV), int(g["T"])
	assert codes.shape[1] == (10 if cfg is W.DIFF_SMALL else 19) and T == (43 if cfg is W.DIFF_SMALL else 80)
	E, mel_pred = model.timestep_independent(codes, cond, T, True)
	x, ts = t(g["x"]).to(DEV), t(g["t"]).to(DEV)
	y, mel_pred_fwd = model(x, ts, aligned_conditioning=codes, conditioning_latent=cond, return_code_pred=True)
	lg = golden(latent_name)
	El, mel_pred_latent = model.timestep_independent(t(lg["latents"]).to(DEV), t(lg["cond"]).to(DEV), int(lg["T"]), True)
	errs = dict(E=maxerr(E, g["E"]), y_cond=maxerr(y, g["y_cond"]), mel_pred=maxerr(mel_pred, g["mel_pred"]), mel_pred_latent=maxerr(mel_pred_latent, g["mel_pred_latent"]),
				E_latent=maxerr(El, lg["E"]))
	print(name, errs)
	assert errs["E"] < bE and errs["E_latent"] < bE
	assert errs["y_cond"] < bY and errs["mel_pred"] < bY and errs["mel_pred_latent"] < bY
	assert torch.equal(mel_pred_fwd, mel_pred)
	for cf in (True, False):
		torch.manual_seed(int(g["sampler_seed"]))
		mel = get_diffuser(steps=4, cond_free=cf).sample_loop(model, (1, 100, T), sampler="ddim", noise=t(g["noise"]).to(DEV),
															  model_kwargs={"precomputed_aligned_embeddings": E[:1]}, progress=False)
		e = maxerr(mel, g[f"ddim_cf{int(cf)}"])
		print(name, f"ddim_cf{int(cf)}", e)
		assert e < 1e-3


# ------------------------------------------------------------------------------------------------ 16-bit and fp8 modes
@pytest.mark.parametrize("dtype,bE,bM", [("bf16", 3e-2, 5e-2), ("f16", 4e-3, 7e-3)])
def test_16_bit_modes(golden, dtype, bE, bM):
	g, model = fixture_model(golden, "diff_codes_small", W.DIFF_SMALL, dtype)
	E, mel_pred = model.timestep_independent(t(g["codes"]).to(DEV), t(g["cond"]).to(DEV), int(g["T"]), True)
	lg = golden("diff_small")
	mel_pred_latent = model.timestep_independent(t(lg["latents"]).to(DEV), t(lg["cond"]).to(DEV), int(lg["T"]), True)[1]
	eE, eM, eL = relerr(E, g["E"]), relerr(mel_pred, g["mel_pred"]), relerr(mel_pred_latent, g["mel_pred_latent"])
	print(dtype, "rel L2: E", eE, "mel_pred", eM, "mel_pred_latent", eL)
	assert eE < bE and eM < bM and eL < bM


def test_fp8_modes(golden):
	g = golden("diff_codes_small")
	Es = {}
	for dtype in ("fp8w", "fp8"):
		model = model_of(W.DIFF_SMALL, int(g["seed"]), int(g["in_tokens"]), dtype)
		E, mel_pred = model.timestep_independent(t(g["codes"]).to(DEV), t(g["cond"]).to(DEV), int(g["T"]), True)
		assert torch.isfinite(E).all() and torch.isfinite(mel_pred).all()
		Es[dtype] = E
		print(dtype, "rel L2: E", relerr(E, g["E"]), "mel_pred", relerr(mel_pred, g["mel_pred"]))
		assert relerr(E, g["E"]) < 0.15
	assert relerr(Es["fp8"], Es["fp8w"]) < 0.1


# ------------------------------------------------------------------------------------------------ shapes against the CPU restatement
def _rows(kind, n_tok, b, M):
	if kind == "random":
		return torch.stack([DC.fixture_codes(1, M, 100 * M + r, n_tok)[0] for r in range(b)])
	assert kind == "edges" and b == 3          # rows of id 0, of the last id, of one id repeated
	return torch.stack([torch.zeros(M, dtype=torch.long), torch.full((M,), n_tok - 1), torch.full((M,), n_tok // 3)])


@pytest.mark.parametrize("n_tok", [200, 8193])
@pytest.mark.parametrize("kind,b,M,T", [("random", 1, 1, 4), ("random", 1, 7, 43), ("random", 1, 33, 20), ("random", 2, 65, 282), ("edges", 3, 7, 30)])
def test_shapes_vs_restatement_f32(n_tok, kind, b, M, T):
	cfg, seed = W.DIFF_SMALL, 21
	model = model_of(cfg, seed, n_tok, "f32")
	assert model.in_tokens == n_tok
	codes = _rows(kind, n_tok, b, M)
	cond = torch.randn(b, 2 * cfg.model_channels, generator=torch.Generator().manual_seed(M))
	with torch.inference_mode():
		ref_E, ref_mel = DC.DiffCodesOracle(weights_of(cfg, seed, n_tok), cfg).timestep_independent_codes(codes, cond, T, True)
	E, mel_pred = model.timestep_independent(codes.to(DEV), cond.to(DEV), T, True)
	assert E.shape == ref_E.shape and mel_pred.shape == ref_mel.shape == (b, 100, T)
	eE, eM = maxerr(E, ref_E), maxerr(mel_pred, ref_mel)
	print(n_tok, kind, b, M, T, eE, eM)
	assert eE < 1e-4 and eM < 2e-4
	if b > 1:      # rows are independent: each equals its own call, bit for bit
		for r in range(b):
			Er, mr = model.timestep_independent(codes[r:r + 1].to(DEV), cond[r:r + 1].to(DEV), T, True)
			assert torch.equal(Er, E[r:r + 1]) and torch.equal(mr, mel_pred[r:r + 1])
	if kind == "random" and b == 1:      # the ids matter
		assert not torch.equal(E, model.timestep_independent(((codes + 1) % n_tok).to(DEV), cond.to(DEV), T, False))
	assert torch.equal(model.timestep_independent(codes.to(torch.int32).to(DEV), cond.to(DEV), T, False), E)      # any integer type, two calls equal


# ------------------------------------------------------------------------------------------------ bit equalities
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_equals_precomputed_and_feeds_the_samplers(golden, dtype):
	from tortoise_tts_amd.diffusion import get_diffuser
	g, model = fixture_model(golden, "diff_codes_small", W.DIFF_SMALL, dtype)
	codes, cond, T = t(g["codes"]).to(DEV), t(g["cond"]).to(DEV), int(g["T"])
	x, ts = t(g["x"]).to(DEV), t(g["t"]).to(DEV)
	E, mel_pred = model.timestep_independent(codes, cond, T, True)
	assert torch.equal(E, model.timestep_independent(codes, cond, T, False))
	y = model(x, ts, aligned_conditioning=codes, conditioning_latent=cond)
	assert torch.equal(y, model(x, ts, precomputed_aligned_embeddings=E))
	y2, mp2 = model(x, ts, aligned_conditioning=codes, conditioning_latent=cond, return_code_pred=True)
	assert torch.equal(y2, y) and torch.equal(mp2, mel_pred)
	with pytest.raises(AssertionError):
		model(x, ts, precomputed_aligned_embeddings=E, return_code_pred=True)
	# E from codes is an E like any other: the single loop and the ragged batch take it unchanged
	diffuser = get_diffuser(steps=3, cond_free=True)
	E2 = model.timestep_independent(codes[1:, :7], cond[1:], 30, False)
	noises = [torch.randn(1, 100, n, generator=torch.Generator().manual_seed(n)).to(DEV) for n in (T, 30)]
	single = [diffuser.sample_loop(model, (1, 100, n.shape[-1]), sampler="ddim", noise=n, model_kwargs={"precomputed_aligned_embeddings": e}, progress=False)
			  for n, e in zip(noises, (E[:1], E2))]
	lines = diffuser.sample_loop_lines(model, noises, [E[:1], E2])
	assert all(torch.isfinite(m).all() for m in single) and all(torch.equal(a, b) for a, b in zip(single, lines))


def test_refusals_on_the_device(golden):
	from tortoise_tts_amd import _lib
	from tortoise_tts_amd.diffusion import DiffusionTTS
	g = golden("diff_codes_small")
	cfg, sd = W.DIFF_SMALL, weights_of(W.DIFF_SMALL, int(g["seed"]), int(g["in_tokens"]))
	codes, cond, T = t(g["codes"]).to(DEV), t(g["cond"]).to(DEV), int(g["T"])
	bare = DiffusionTTS(sd, cfg, dtype="f32", device=DEV, codes=False)
	assert bare.in_tokens == 0
	with pytest.raises(NotImplementedError, match="codes=True"):
		bare.timestep_independent(codes, cond, T)
	# the handle itself refuses too, with a clean error
	E = torch.empty(2, cfg.model_channels, T, device=DEV)
	idx = torch.zeros(T, dtype=torch.int32, device=DEV)
	rc = bare.lib.ttk_diff_precompute_codes(bare._h, codes.data_ptr(), cond.data_ptr(), idx.data_ptr(), 2, codes.shape[1], T, E.data_ptr(), None, _lib.stream_ptr())
	assert rc == -4 and b"code_embedding" in bare.lib.ttk_last_error()
	assert bare.lib.ttk_diff_mel_head(bare._h, E.data_ptr(), 2, T, E.data_ptr(), _lib.stream_ptr()) == -4
	# ... and behaves as before everywhere else
	lg = golden("diff_small")
	full = model_of(cfg, int(g["seed"]), int(g["in_tokens"]), "f32")
	lat, lc = t(lg["latents"]).to(DEV), t(lg["cond"]).to(DEV)
	assert torch.equal(bare.timestep_independent(lat, lc, int(lg["T"]), False), full.timestep_independent(lat, lc, int(lg["T"]), False))
	with pytest.raises(_lib.TTKError, match="codes=True"):
		DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(cfg), 21), cfg, dtype="f32", device=DEV, codes=True)
	model = model_of(cfg, int(g["seed"]), 200, "f32")
	for bad in (-1, 200):
		with pytest.raises(IndexError):
			model.timestep_independent(torch.tensor([[3, bad]]).to(DEV), cond[:1], 8)


# ------------------------------------------------------------------------------------------------ user level
@pytest.fixture(scope="module")
def tts(golden):
	"""the tiny TTS of tests/test_gpu_tts.py (same seeds), its diffusion model with token conditioning, plus the DVAE and the random-voice pair"""
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.conditioning import ConditioningEncoder, ContextualEmbedder
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.dvae import DiscreteVAE
	from tortoise_tts_amd.mel import TacotronSTFT, TorchMelSpectrogram
	from tortoise_tts_amd.random_latent import RandomLatentConverter
	from tortoise_tts_amd.tokenizer import VoiceBpeTokenizer
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN
	g = golden("tokenizer")
	tok = VoiceBpeTokenizer(vocab={str(v): i for i, v in enumerate(g["vocab"])}, merges=[str(m) for m in g["merges"]], special_tokens=[str(s) for s in g["special"]])
	norms = torch.rand(80, generator=torch.Generator().manual_seed(2)) * 3 + 1
	gd = golden("dvae_small")
	dsd = W.synth_state_dict(W.dvae_shapes(W.DVAE_SMALL), int(gd["seed"]))
	dsd["codebook.embed"] = W.dvae_codebook(t(gd["cb_mean"]), t(gd["cb_std"]), W.DVAE_SMALL.num_tokens, int(gd["cb_seed"]))
	common = dict(vocoder=BigVGAN(W.synth_state_dict(W.vocoder_shapes(W.VOC_SMALL), 33), W.VOC_SMALL, dtype="f32", device=DEV),
				  conditioning_encoder=ConditioningEncoder(W.synth_state_dict(W.ar_conditioning_shapes(W.AR_SMALL), 35), W.AR_SMALL, dtype="f32", device=DEV),
				  contextual_embedder=ContextualEmbedder(W.synth_state_dict(W.diffusion_conditioning_shapes(W.DIFF_SMALL), 36), W.DIFF_SMALL, dtype="f32", device=DEV),
				  tms=TorchMelSpectrogram(mel_norms=norms, device=DEV), stft=TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000, device=DEV),
				  dvae=DiscreteVAE(dsd, W.DVAE_SMALL, dtype="f32", device=DEV),
				  rlg_auto=RandomLatentConverter(W.rlg_state_dict(W.AR_SMALL.model_dim, 37), device=DEV),
				  rlg_diffuser=RandomLatentConverter(W.rlg_state_dict(2 * W.DIFF_SMALL.model_channels, 38), device=DEV))
	ar = UnifiedVoice(W.synth_state_dict(W.ar_shapes(W.AR_SMALL), 31), W.AR_SMALL, dtype="f32", device=DEV, max_batch=8, max_ctx=128)
	sd = weights_of(W.DIFF_SMALL, 32, W.DIFF_CODE_TOKENS)
	with_codes = TTS(ar, DiffusionTTS(sd, W.DIFF_SMALL, dtype="f32", device=DEV), tok, **common)
	without = TTS(ar, DiffusionTTS(sd, W.DIFF_SMALL, dtype="f32", device=DEV, codes=False), tok, **common)
	return with_codes, without


def test_decode_codes_and_resynthesize(tts):
	tts, bare = tts
	assert tts.hot.diffusion.in_tokens == W.DIFF_CODE_TOKENS and bare.hot.diffusion.in_tokens == 0
	clip = speechlike(9, 30000, 22050).to(DEV)
	enc = tts.encode_audio(clip, 22050)
	codes = enc["codes"]
	M = codes.shape[1]
	kw = dict(max_diffusion_steps=3, seed=77)
	wav, sr = tts.decode_codes(codes, enc, **kw)
	T = M * 4 * 24000 // 22050
	assert sr == 24000 and wav.shape == (1, 1, T * W.VOC_SMALL.hop_size) and torch.isfinite(wav).all()
	assert torch.equal(wav, tts.decode_codes(codes, enc, **kw)[0])                     # seed-deterministic
	assert not torch.equal(wav, tts.decode_codes(codes, enc, max_diffusion_steps=3, seed=78)[0])
	assert torch.equal(wav, tts.decode_codes(codes[0], clip, **kw)[0])                 # a bare row; the clip instead of its dict
	# a list of rows: the rows' own calls, concatenated (the two rows differ in length: one ragged DDIM batch)
	rows = [codes, codes[:, 5:16]]
	both = tts.decode_codes(rows, enc, **kw)[0]
	assert torch.equal(both, torch.concat([tts.decode_codes(r, enc, **kw)[0] for r in rows], dim=-1))
	# the round trip, in the clip's own voice and in another
	assert torch.equal(tts.resynthesize(clip, 22050, **kw)[0], wav)
	other = speechlike(10, 26000, 22050).to(DEV)
	w2 = tts.resynthesize(clip, 22050, other, **kw)[0]
	assert torch.equal(w2, tts.decode_codes(codes, other, **kw)[0]) and w2.shape == wav.shape and not torch.equal(w2, wav)
	# a random voice: the seed fixes it
	r1 = tts.decode_codes(codes, None, **kw)[0]
	assert torch.equal(r1, tts.decode_codes(codes, None, **kw)[0]) and not torch.equal(r1, wav)
	# refusals, each with its reason
	with pytest.raises(NotImplementedError, match="HiFiGAN"):
		tts.decode_codes(codes, enc, vocoder_type="hifigan")
	with pytest.raises(NotImplementedError, match="codes=True"):
		bare.decode_codes(codes, enc, **kw)
	with pytest.raises(IndexError):
		tts.decode_codes(torch.tensor([[1, W.DIFF_CODE_TOKENS]]), enc, **kw)
	with pytest.raises(ValueError, match="codes"):
		tts.decode_codes(torch.zeros(1, 4), enc, **kw)


def test_hot_path_diffuses_from_the_sampled_codes(tts):
	from tortoise_tts_amd.diffusion import denormalize_tacotron_mel, get_diffuser
	from tortoise_tts_amd.inference import trim_calm_tokens
	tts, bare = tts
	hot, diff = tts.hot, tts.hot.diffusion
	al, dl = tts.encode_audio(speechlike(9, 30000, 22050).to(DEV), 22050)["latent"]
	text = tts.encode_text("Hello there.").to(DEV)[None]
	kw = dict(max_ar_steps=12, max_diffusion_steps=3, candidates=2, return_all=True)
	torch.manual_seed(5)
	mels, seconds, aux = hot.inference(text, al, dl, diffusion_conditioning="codes", **kw)
	row = trim_calm_tokens(aux["codes"][:1], aux["codes"][:1])
	T = row.shape[1] * 4 * 24000 // 22050
	assert aux["latents"] is None and torch.equal(aux["aligned"], row) and mels.shape == (1, 100, T)
	E = diff.timestep_independent(row, dl, T, False)
	assert torch.equal(E, aux["E"])
	mel = get_diffuser(steps=3).sample_loop(diff, (1, 100, T), sampler="ddim", noise=aux["noise"], model_kwargs={"precomputed_aligned_embeddings": E}, progress=False)
	assert torch.equal(mel, aux["mel"]) and torch.equal(mels, denormalize_tacotron_mel(mel)) and torch.isfinite(mels).all()
	# the default is the latent path, unchanged: the same bits with and without the keyword, and other bits than from codes
	torch.manual_seed(5)
	m_lat, _, a_lat = hot.inference(text, al, dl, diffusion_conditioning="latents", **kw)
	torch.manual_seed(5)
	m_def, _, a_def = hot.inference(text, al, dl, **kw)
	assert torch.equal(m_lat, m_def) and torch.equal(a_lat["codes"], aux["codes"]) and a_def["latents"] is not None and not torch.equal(m_def, mels)
	assert sorted(a_def) == sorted(a_lat) and "aligned" not in a_def
	# several lines: each line what its own call gives
	lines = [text, tts.encode_text("The end!").to(DEV)[None]]
	lkw = dict(max_ar_steps=12, max_diffusion_steps=3)
	got = hot.inference_lines(lines, al, dl, diffusion_conditioning="codes", **lkw)
	for line, (m, _, _) in zip(lines, got):
		assert torch.equal(m, hot.inference(line, al, dl, diffusion_conditioning="codes", **lkw)[0])
	# what cannot support it refuses with a reason, before anything is sampled
	with pytest.raises(NotImplementedError, match="codes=True"):
		bare.hot.inference(text, al, dl, diffusion_conditioning="codes", **kw)
	with pytest.raises(ValueError, match="diffusion_conditioning"):
		hot.inference(text, al, dl, diffusion_conditioning="tokens", **kw)
	with pytest.raises(NotImplementedError, match="sharded"):
		hot.inference_sharded(text, al, dl, candidates=2, diffusion_conditioning="codes")
