"""Regenerate the RandomLatentConverter fixtures of tests/golden/ from the reference's own class (models/random_latent_generator.py, imported by
file path).  The reference checkout is $TTK_REFERENCE (default /root/reference).

Weights are `weights.rlg_state_dict(channels, seed)` -- at the reference's own scales, see its docstring -- loaded strictly.  CPU, one thread: a
rerun reproduces every array bit for bit.  Only inputs and outputs are stored; the tests rebuild the weights from the seed.

Per case (tag = "<channels>x<B>"):
  seed_<tag>, noise_seed_<tag>
  y_<tag>      f32 [B, channels]: `torch.manual_seed(noise_seed); model(ref)` with ref = zeros [B, 1] -- the reference's forward draws its own noise
  noise_<tag>  f32 [B, channels]: that draw, recorded by setting the same seed again: torch.randn(B, channels) on the CPU
  y64_<tag>    f64 [B, channels]: the same module `.double()`, its layers applied to noise.double()

Fixtures
  rlg_small.npz  channels 64 with B = 5, channels 132 with B = 1
  rlg_full.npz   channels 1024 with B = 3 (the autoregressive latent), channels 2048 with B = 2 (the diffusion latent)
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import weights as W  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_module():
	ref = os.environ.get("TTK_REFERENCE", "/root/reference")
	spec = importlib.util.spec_from_file_location("_ref_rlg", os.path.join(ref, "tortoise_tts", "models", "random_latent_generator.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


def make(mod, name, cases):
	out = {"tags": np.asarray([f"{c}x{B}" for c, B, _, _ in cases])}
	for channels, B, seed, noise_seed in cases:
		tag = f"{channels}x{B}"
		model = mod.RandomLatentConverter(channels)
		model.load_state_dict(W.rlg_state_dict(channels, seed), strict=True)
		model.eval()
		ref = torch.zeros(B, 1)
		with torch.no_grad():
			torch.manual_seed(noise_seed)
			y = model(ref)
			torch.manual_seed(noise_seed)
			noise = torch.randn(ref.shape[0], channels, device=ref.device)
			y64 = copy.deepcopy(model).double().layers(noise.double())
		assert y.dtype == torch.float32 and y.shape == noise.shape == y64.shape == (B, channels) and y64.dtype == torch.float64
		dev = (y.double() - y64).abs().max().item()
		assert 0 < dev < 1e-3 * y64.abs().max().item(), (tag, dev)      # the recorded noise is the draw the forward made
		out.update({f"seed_{tag}": np.int64(seed), f"noise_seed_{tag}": np.int64(noise_seed), f"noise_{tag}": noise.numpy(), f"y_{tag}": y.numpy(),
					f"y64_{tag}": y64.numpy()})
		print(f"{name} {tag}: y rms {y.pow(2).mean().sqrt():.3f} max {y.abs().max():.3f}, max|y - y64| {dev:.3e}")
	np.savez(os.path.join(GOLDEN, name + ".npz"), **out)
	print(name, os.path.getsize(os.path.join(GOLDEN, name + ".npz")), "bytes")


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	os.makedirs(GOLDEN, exist_ok=True)
	make(mod, "rlg_small", ((64, 5, 141, 1), (132, 1, 142, 2)))
	make(mod, "rlg_full", ((1024, 3, 143, 3), (2048, 2, 144, 4)))


if __name__ == "__main__":
	main()
