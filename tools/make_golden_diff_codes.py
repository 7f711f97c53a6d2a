"""Regenerate the token-conditioning fixtures of tests/golden/ from the reference's own `DiffusionTTS` (models/diffusion.py, imported through
oracle/ref_shim.py).  The reference checkout is $TTK_REFERENCE (default /root/reference).

Weights are seeds only: `weights.synth_state_dict(diffusion_shapes(cfg), seed)` merged with `synth_state_dict(diffusion_code_shapes(cfg), seed)` -- the
seed of the latent-path fixture of the same size (diff_small.npz / diff_full.npz), so `mel_pred_latent` is `return_code_pred=True` on THAT fixture's
latents and embeddings.  The reference's `contextual_embedder` keeps its random initialisation: nothing here runs it.  CPU, one thread: a rerun
reproduces every array bit for bit.

Each file (diff_codes_small.npz: DIFF_SMALL, b = 2, M = 10, T = 43; diff_codes_full.npz: DIFF_FULL, b = 1, M = 19, T = 80 -- small enough to commit):
  seed, in_tokens, codes [b, M] int64 (seed + 11), cond [b, 2C] (seed + 12), T
  E, mel_pred         timestep_independent(codes, cond, T, True)
  x (seed + 13), t    and y_cond = forward(x, t, aligned_conditioning=codes, conditioning_latent=cond); y_cond_rcp / mel_pred_fwd: the pair the same
                      call returns with return_code_pred=True (the reference's own check that both are what the two lines above hold)
  noise (seed + 15), sampler_seed, ddim_cf1, ddim_cf0    get_diffuser(steps=4, cond_free=...).sample_loop(sampler="ddim") from `noise` on E[:1]
  mel_pred_latent     timestep_independent(latents, cond, T, True)[1] on the latents / cond / T of diff_small.npz (diff_full.npz for the full file)
  code_keys, code_shapes   names and (zero-padded) shapes of the reference state_dict's code_embedding / code_converter / mel_head tensors
  versions            "torch a.b.c" of the run
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402
from tortoise_tts_amd import weights as W  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CODE_PREFIXES = ("code_embedding.", "code_converter.", "mel_head.")


def gen(seed):
	return torch.Generator(device="cpu").manual_seed(seed)


def make(d_mod, name, cfg, latent_fixture, b, M, T):
	lat_g = dict(np.load(os.path.join(GOLDEN, latent_fixture + ".npz")))
	seed = int(lat_g["seed"])
	in_tokens = W.DIFF_CODE_TOKENS
	m = d_mod.DiffusionTTS(model_channels=cfg.model_channels, num_layers=cfg.num_layers, in_channels=cfg.in_channels,
						   in_latent_channels=cfg.in_latent_channels, in_tokens=in_tokens, out_channels=cfg.out_channels, num_heads=cfg.num_heads)
	sd = W.synth_state_dict(W.diffusion_shapes(cfg), seed)
	sd.update(W.synth_state_dict(W.diffusion_code_shapes(cfg, in_tokens), seed))
	missing, unexpected = m.load_state_dict(sd, strict=False)
	assert not unexpected and all(k.startswith("contextual_embedder.") for k in missing), (missing, unexpected)
	m.eval()
	ref_code = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(CODE_PREFIXES)}
	codes = torch.randint(0, in_tokens, (b, M), generator=gen(seed + 11))
	cond = torch.randn(b, 2 * cfg.model_channels, generator=gen(seed + 12))
	x = torch.randn(b, cfg.in_channels, T, generator=gen(seed + 13))
	t = torch.tensor([1333, 2666][:b])
	noise = torch.randn(1, cfg.in_channels, T, generator=gen(seed + 15))
	keys = sorted(ref_code)
	out = dict(seed=np.int64(seed), in_tokens=np.int64(in_tokens), codes=codes.numpy(), cond=cond.numpy(), T=np.int64(T), x=x.numpy(), t=t.numpy(),
			   noise=noise.numpy(), sampler_seed=np.int64(seed + 16), code_keys=np.asarray(keys),
			   code_shapes=np.asarray([list(ref_code[k]) + [0] * (3 - len(ref_code[k])) for k in keys], dtype=np.int64),
			   versions=np.array(f"torch {torch.__version__}"))
	with torch.inference_mode():
		E, mel_pred = m.timestep_independent(codes, cond, T, True)
		y = m(x, t, aligned_conditioning=codes, conditioning_latent=cond)
		y2, mp2 = m(x, t, aligned_conditioning=codes, conditioning_latent=cond, return_code_pred=True)
		out.update(E=E.numpy(), mel_pred=mel_pred.numpy(), y_cond=y.numpy(), y_cond_rcp=y2.numpy(), mel_pred_fwd=mp2.numpy())
		for cf in (True, False):
			torch.manual_seed(seed + 16)
			mel = d_mod.get_diffuser(steps=4, cond_free=cf).sample_loop(m, (1, cfg.in_channels, T), sampler="ddim", noise=noise,
																		model_kwargs={"precomputed_aligned_embeddings": E[:1]}, progress=False)
			out[f"ddim_cf{int(cf)}"] = mel.numpy()
		El, mpl = m.timestep_independent(torch.from_numpy(lat_g["latents"]), torch.from_numpy(lat_g["cond"]), int(lat_g["T"]), True)
		assert torch.equal(El, torch.from_numpy(lat_g["E"])) or (El - torch.from_numpy(lat_g["E"])).abs().max() < 1e-5, "not the latent fixture's model"
		out["mel_pred_latent"] = mpl.numpy()
	path = os.path.join(GOLDEN, name + ".npz")
	np.savez(path, **out)
	print(f"{name}: b {b} M {M} T {T}, E rms {E.pow(2).mean().sqrt():.3f}, mel_pred rms {mel_pred.pow(2).mean().sqrt():.3f}, y rms {y.pow(2).mean().sqrt():.3f}, "
		  f"{os.path.getsize(path)} bytes")


def main():
	torch.set_num_threads(1)
	d_mod, _ = ref_shim.load()
	os.makedirs(GOLDEN, exist_ok=True)
	make(d_mod, "diff_codes_small", W.DIFF_SMALL, "diff_small", 2, 10, 43)
	make(d_mod, "diff_codes_full", W.DIFF_FULL, "diff_full", 1, 19, 80)


if __name__ == "__main__":
	main()
