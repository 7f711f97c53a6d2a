"""The DiscreteVAE CPU oracle (tests/dvae_oracle.py) against the reference's own class (tests/golden/dvae_*.npz, written by tools/make_golden_dvae.py),
the weight table, the checkpoint loader and `mel.encode` without a DVAE.  No GPU."""
import numpy as np
import pytest
import torch

import dvae_oracle as DO
from tortoise_tts_amd import weights as W

CFGS = {"dvae_small": (W.DVAE_SMALL, ("1x5", "1x61", "3x64")), "dvae_full": (W.DVAE_FULL, ("1x517", "2x64"))}
CASES = [(n, tag) for n, (_, tags) in CFGS.items() for tag in tags]
_cache = {}


def t(a):
	return torch.from_numpy(np.asarray(a))


def setup(golden, name):
	"""(fixture, state_dict with the fixture's codebook, f32 oracle), built once per config"""
	if name not in _cache:
		g = golden(name)
		cfg = CFGS[name][0]
		sd = W.synth_state_dict(W.dvae_shapes(cfg), int(g["seed"]))
		sd["codebook.embed"] = W.dvae_codebook(t(g["cb_mean"]), t(g["cb_std"]), cfg.num_tokens, int(g["cb_seed"]))
		_cache[name] = (g, sd, DO.DVAEOracle(sd, cfg, torch.float32))
	return _cache[name]


def maxerr(a, b):
	return (torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max().item()


@pytest.mark.parametrize("name,tag", CASES)
def test_oracle_reproduces_the_reference(golden, name, tag):
	g, sd, o = setup(golden, name)
	cfg = CFGS[name][0]
	B, T = (int(v) for v in tag.split("x"))
	mel = DO.fixture_mel(B, T, int(g[f"input_seed_{tag}"]), cfg.channels)
	if f"mel_{tag}" in g:
		assert torch.equal(mel, t(g[f"mel_{tag}"]))
	zs, ms, hs = int(g["z_step"]), int(g["mel_step"]), int(g["hidden_step"])
	with torch.inference_mode():
		z = o.encode(mel)
		codes = o.quantize(z)
		dec_mel, dec_hidden = o.decode(t(g[f"codes_{tag}"]))
	assert z.shape == (B, cfg.code_frames(T), cfg.codebook_dim) and dec_mel.shape == (B, cfg.channels, 4 * z.shape[1]) and dec_hidden.shape == (B, cfg.hidden_dim, 4 * z.shape[1])
	# f32 round-off of a chain of K <= 3072 convolutions on O(1) activations
	assert maxerr(z[:, ::zs], g[f"z_{tag}"]) < 1e-4
	assert maxerr(dec_mel[..., ::ms], g[f"dec_mel_{tag}"]) < 1e-4 and maxerr(dec_hidden[..., ::hs], g[f"dec_hidden_{tag}"]) < 1e-4
	tie = t(g[f"tie_idx_{tag}"])
	gap, tau = t(g[f"gap_{tag}"]), float(g[f"tau_{tag}"])
	assert torch.equal(torch.nonzero(gap < tau).reshape(-1), tie) and tie.numel() <= 0.02 * gap.numel()
	wrong, excess, share = DO.check_codes(codes, g[f"codes_{tag}"], z.reshape(-1, cfg.codebook_dim), sd["codebook.embed"], gap, tau)
	print(f"{name} {tag}: {wrong} mismatches outside near ties, worst near-tie excess {excess:.3e} (tau {tau:.3e}), near-tie share {share:.4f}")
	assert wrong == 0 and excess <= tau and share <= 0.02


@pytest.mark.parametrize("name", sorted(CFGS))
def test_dvae_shapes_cover_exactly_the_reference_keys(golden, name):
	g = golden(name)
	assert sorted(W.dvae_shapes(CFGS[name][0]).keys()) == [str(k) for k in g["keys"]]


def test_load_dvae_state_round_trips_and_drops_the_ema_buffers(tmp_path):
	from tortoise_tts_amd.checkpoint import CheckpointError, load_dvae_state
	cfg = W.DVAE_SMALL
	sd = W.synth_state_dict(W.dvae_shapes(cfg), 7)
	saved = dict(sd)
	saved["codebook.cluster_size"] = torch.zeros(cfg.num_tokens)
	saved["codebook.embed_avg"] = sd["codebook.embed"].clone()
	path = tmp_path / "dvae.pth"
	torch.save(saved, path)
	got, got_cfg = load_dvae_state(path, cfg=cfg)
	assert got_cfg == cfg and sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
	del saved["decoder.0.bias"]
	torch.save(saved, path)
	with pytest.raises(CheckpointError, match="decoder.0.bias"):
		load_dvae_state(path, cfg=cfg)


def test_unsupported_configurations_are_refused_with_a_reason():
	import dataclasses
	from tortoise_tts_amd.dvae import check_config
	check_config(W.DVAE_FULL)
	check_config(W.DVAE_SMALL)
	for change in (dict(positional_dims=2), dict(use_lr_quantizer=True), dict(encoder_norm=True), dict(use_transposed_convs=True), dict(activation="silu"),
				   dict(normalization=((0.5,), (0.5,))), dict(record_codes=True), dict(num_layers=1), dict(num_resnet_blocks=0)):
		with pytest.raises(NotImplementedError, match="DiscreteVAE"):
			check_config(dataclasses.replace(W.DVAE_FULL, **change))


def test_mel_encode_without_a_dvae_returns_no_codes(monkeypatch):
	"""host only: the mel front-ends and the two conditioning encoders are stubs"""
	from tortoise_tts_amd import mel as M

	class Front:
		device = "cpu"

		def __call__(self, wav):
			return torch.zeros(wav.shape[0], 80, wav.shape[-1] // 256 + 1)

		def mel_spectrogram(self, wav):
			return torch.zeros(wav.shape[0], 100, wav.shape[-1] // 256 + 1)

	class Enc:
		def get_conditioning(self, c):
			return torch.zeros(1, 4)

	class Codes:
		def get_codebook_indices(self, mel):
			return torch.full((mel.shape[0], (((mel.shape[-1] - 1) // 2 + 1) - 1) // 2 + 1), 3, dtype=torch.int64)

	monkeypatch.setattr(M, "resample", lambda wav, a, b, device=None: wav)
	wav = torch.zeros(1, 40000)
	parts = dict(tms=Front(), stft=Front(), conditioning_encoder=Enc(), contextual_embedder=Enc())
	out = M.encode(wav, 22050, **parts)
	assert sorted(out) == ["conds", "latent", "metadata"]
	both = M.encode(wav, 22050, dvae=Codes(), **parts)
	assert sorted(both) == ["codes", "conds", "latent", "metadata"]
	assert both["codes"].shape == (1, W.DVAE_FULL.code_frames(40000 // 256 + 1))       # the whole clip, neither cropped nor padded to 132300 samples
	assert both["conds"][0].shape == out["conds"][0].shape == (1, 1, 80, 132300 // 256 + 1)
