"""Token conditioning of the diffusion model, the part that needs no device: the CPU restatement (tests/diff_codes_oracle.py) against the reference's own
results (tests/golden/diff_codes_*.npz, tools/make_golden_diff_codes.py), the weight table against the reference's state_dict, and the argument checks."""
import numpy as np
import pytest
import torch

import diff_codes_oracle as DC
from tortoise_tts_amd import weights as W

CASES = [("diff_codes_small", W.DIFF_SMALL, "diff_small"), ("diff_codes_full", W.DIFF_FULL, "diff_full")]


def t(a):
	return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
	return (torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max().item()


@pytest.mark.parametrize("name,cfg,latent_name", CASES)
def test_restatement_equals_reference_fixture(golden, name, cfg, latent_name):
	g = golden(name)
	o = DC.DiffCodesOracle(DC.state_dict(cfg, int(g["seed"]), int(g["in_tokens"])), cfg)
	codes, cond, T = t(g["codes"]), t(g["cond"]), int(g["T"])
	with torch.inference_mode():
		E, mel_pred = o.timestep_independent_codes(codes, cond, T, True)
		y, mel_pred_fwd = o.forward_codes(t(g["x"]), t(g["t"]), codes, cond, True)
		lg = golden(latent_name)
		mel_pred_latent = o.mel_head(o.timestep_independent(t(lg["latents"]), t(lg["cond"]), int(lg["T"])))
	errs = dict(E=maxerr(E, g["E"]), mel_pred=maxerr(mel_pred, g["mel_pred"]), y_cond=maxerr(y, g["y_cond"]),
				mel_pred_latent=maxerr(mel_pred_latent, g["mel_pred_latent"]))
	print(name, errs)
	assert all(e < 2e-5 for e in errs.values()), errs
	assert torch.equal(mel_pred_fwd, mel_pred)
	# the reference's own two routes to the same tensors agree with each other
	assert np.array_equal(g["y_cond_rcp"], g["y_cond"]) and np.array_equal(g["mel_pred_fwd"], g["mel_pred"])


@pytest.mark.parametrize("name,cfg,latent_name", CASES)
def test_code_shapes_are_the_reference_state_dict(golden, name, cfg, latent_name):
	g = golden(name)
	ref = {str(k): tuple(int(d) for d in s if d) for k, s in zip(g["code_keys"], g["code_shapes"])}
	ours = {k: tuple(v) for k, v in W.diffusion_code_shapes(cfg, int(g["in_tokens"])).items()}
	assert ours == ref
	assert not set(ours) & set(W.diffusion_shapes(cfg))
	assert W.diffusion_code_shapes(cfg, 200)["code_embedding.weight"] == (200, cfg.model_channels)


def test_existing_synthetic_tensors_keep_their_bits(golden):
	seed, cfg = int(golden("diff_codes_small")["seed"]), W.DIFF_SMALL
	plain = W.synth_state_dict(W.diffusion_shapes(cfg), seed)
	both = DC.state_dict(cfg, seed)
	assert set(both) == set(plain) | set(W.diffusion_code_shapes(cfg))
	assert all(torch.equal(both[k], plain[k]) for k in plain)


def test_argument_checks_need_no_device():
	from tortoise_tts_amd.diffusion import DiffusionTTS, check_aligned_conditioning
	n = 200
	ok = torch.tensor([[0, 5, n - 1]])
	assert check_aligned_conditioning(ok, n) is True
	assert check_aligned_conditioning(ok.to(torch.int32), n) is True
	assert check_aligned_conditioning(torch.zeros(1, 3, 128), 0) is False
	for bad in (-1, n):
		with pytest.raises(IndexError):
			check_aligned_conditioning(torch.tensor([[0, bad, 1]]), n)
	with pytest.raises(NotImplementedError, match="codes=True"):
		check_aligned_conditioning(ok, 0)
	with pytest.raises(NotImplementedError, match="codes=True"):
		check_aligned_conditioning(torch.zeros(1, 3, 128), 0, return_code_pred=True)
	# the model's own entry points run these checks before they touch the device: an object that never had one shows it
	m = DiffusionTTS.__new__(DiffusionTTS)
	m.cfg, m.in_tokens = W.DIFF_SMALL, n
	x, ts, cond = torch.zeros(1, 100, 8), torch.zeros(1, dtype=torch.long), torch.zeros(1, 256)
	with pytest.raises(AssertionError):
		m.forward(x, ts, precomputed_aligned_embeddings=torch.zeros(1, 128, 8), return_code_pred=True)
	with pytest.raises(IndexError):
		m.forward(x, ts, aligned_conditioning=torch.tensor([[n]]), conditioning_latent=cond)
	with pytest.raises(IndexError):
		m.timestep_independent(torch.tensor([[-1, 3]]), cond, 8)
	m.in_tokens = 0
	with pytest.raises(NotImplementedError, match="codes=True"):
		m.timestep_independent(ok, cond, 8)
	with pytest.raises(NotImplementedError, match="codes=True"):
		m.forward(x, ts, aligned_conditioning=torch.zeros(1, 2, 128), conditioning_latent=cond, return_code_pred=True)


def test_codes_argument_resolution(tmp_path):
	from tortoise_tts_amd import _lib, checkpoint as ck
	from tortoise_tts_amd.diffusion import _resolve_codes
	cfg = W.DIFF_SMALL
	plain = W.synth_state_dict(W.diffusion_shapes(cfg), 3)
	both = DC.state_dict(cfg, 3, in_tokens=200)
	assert _resolve_codes(plain, cfg, None) == 0 and _resolve_codes(both, cfg, None) == 200
	assert _resolve_codes(both, cfg, False) == 0 and _resolve_codes(both, cfg, True) == 200
	with pytest.raises(_lib.TTKError, match="codes=True"):
		_resolve_codes(plain, cfg, True)
	partial = dict(both)
	del partial["mel_head.bias"]
	assert _resolve_codes(partial, cfg, None) == 0
	ck.save_state_dict(both, tmp_path / "d.pth")
	code_names = set(W.diffusion_code_shapes(cfg))
	assert set(ck.load_diffusion_state(tmp_path / "d.pth")[0]) == set(plain) | code_names
	assert set(ck.load_diffusion_state(tmp_path / "d.pth", codes=False)[0]) == set(plain)
	ck.save_state_dict(partial, tmp_path / "p.pth")
	assert set(ck.load_diffusion_state(tmp_path / "p.pth")[0]) == set(plain)
	with pytest.raises(ck.CheckpointError, match="mel_head.bias"):
		ck.load_diffusion_state(tmp_path / "p.pth", codes=True)
