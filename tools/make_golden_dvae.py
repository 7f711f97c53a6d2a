"""Regenerate the DiscreteVAE fixtures of tests/golden/ from the reference's own class (models/dvae.py, imported by file path).  The reference
checkout is $TTK_REFERENCE (default /root/reference).

models/dvae.py imports `vector_quantize_pytorch` at its top, a package the `use_lr_quantizer` option needs and nothing else does.  This tool puts a
stub module of that name with an empty `VectorQuantize` class into `sys.modules` first: the default configuration never instantiates it.

Weights are `weights.synth_state_dict(dvae_shapes(cfg), seed)`, except the codebook.  `Quantize` initialises it with randn, and against a randomly
initialised encoder |e|^2 then decides every distance: each frame gets the same code and a broken quantizer passes.  So the tool runs the reference
encoder on the fixture inputs and draws the codebook's columns with that output's per-channel mean and standard deviation
(`weights.dvae_codebook(mean, std, num_tokens, seed)`; `cb_mean`, `cb_std` are stored, the tests rebuild the codebook from them).  It asserts that
the reference's codes take at least T4 / 2 distinct values on every stored input.  CPU, one thread: a rerun reproduces every array bit for bit.

Near ties (tests/dvae_oracle.py has the criterion): per input, `gap` = float64 margin between the best and second-best code per position, computed
from the reference's f32 z; `tau` = 4 x max |dist_f32 - dist_f64| with dist_f32 the reference's own expression (dvae.py:31-35) as it evaluates it --
a multiple of the reference's own rounding noise, four being the margin for another summation order on top of it.  The tool asserts
mean(gap < tau) <= 0.02 on every input.  `tie_idx` / `z_tie` are the positions with gap < tau and their z rows.

Fixtures (tag = "<B>x<T>"; inputs are `dvae_oracle.fixture_mel(B, T, input_seed)`, decode inputs are the reference's own codes)
  dvae_small.npz  DVAE_SMALL, (B, T) = (1, 5), (1, 61), (3, 64): seed, cb_seed, cb_mean, cb_std, keys, and per tag input_seed, mel, z, codes, gap, tau,
                  tie_idx, z_tie, dec_mel, dec_hidden, and the reference's own results under torch.autocast("cpu", bfloat16 / float16):
                  z_bf16, dec_mel_bf16, dec_hidden_bf16, z_f16, dec_mel_f16, dec_hidden_f16.
  dvae_full.npz   DVAE_FULL, (1, 517) (a 6 s clip) and (2, 64): the same without `mel`, and with the big arrays subsampled: every `z_step`-th code
                  frame of z*, every `mel_step`-th / `hidden_step`-th frame of dec_mel* / dec_hidden*.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tortoise_tts_amd import weights as W  # noqa: E402
import dvae_oracle as DO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EMA = ("codebook.cluster_size", "codebook.embed_avg")


def reference_module():
	stub = types.ModuleType("vector_quantize_pytorch")
	stub.VectorQuantize = type("VectorQuantize", (), {})
	sys.modules.setdefault("vector_quantize_pytorch", stub)
	ref = os.environ.get("TTK_REFERENCE", "/root/reference")
	spec = importlib.util.spec_from_file_location("_ref_dvae", os.path.join(ref, "tortoise_tts", "models", "dvae.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


def encoder_z(model, mel):
	return model.encoder(mel).permute(0, 2, 1)


def make(mod, name, cfg, seed, cb_seed, shapes, steps):
	model = mod.DiscreteVAE(positional_dims=1, num_tokens=cfg.num_tokens, codebook_dim=cfg.codebook_dim, num_layers=cfg.num_layers,
							num_resnet_blocks=cfg.num_resnet_blocks, hidden_dim=cfg.hidden_dim, channels=cfg.channels, stride=cfg.stride,
							kernel_size=cfg.kernel_size)
	sd = W.synth_state_dict(W.dvae_shapes(cfg), seed)
	missing = model.load_state_dict(sd, strict=False)
	assert sorted(missing.missing_keys) == sorted(EMA) and not missing.unexpected_keys, missing
	model.eval()
	mels = {f"{B}x{T}": DO.fixture_mel(B, T, s, cfg.channels) for (B, T, s) in shapes}
	with torch.no_grad():
		rows = torch.cat([encoder_z(model, m).reshape(-1, cfg.codebook_dim) for m in mels.values()], 0)
		mean, std = rows.mean(0), rows.std(0)
		embed = W.dvae_codebook(mean, std, cfg.num_tokens, cb_seed)
		model.codebook.embed.copy_(embed)
	zs, ms, hs = steps
	out = dict(seed=np.int64(seed), cb_seed=np.int64(cb_seed), cb_mean=mean.numpy(), cb_std=std.numpy(),
			   keys=np.asarray(sorted(k for k in model.state_dict().keys() if k not in EMA)), z_step=np.int64(zs), mel_step=np.int64(ms), hidden_step=np.int64(hs))
	for (B, T, s) in shapes:
		tag = f"{B}x{T}"
		mel = mels[tag]
		with torch.no_grad():
			z = encoder_z(model, mel)
			codes = model.get_codebook_indices(mel)
			dec_mel, dec_hidden = model.decode(codes)
			low = {}
			for dn, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
				with torch.autocast("cpu", dtype=dt):
					zl = encoder_z(model, mel)
					ml, hl = model.decode(codes)
				low[dn] = (zl.float(), ml.float(), hl.float())
		T4 = codes.shape[1]
		assert T4 == cfg.code_frames(T)
		distinct = codes.unique().numel()
		assert distinct >= T4 / 2, f"{name} {tag}: only {distinct} distinct codes over {T4} positions"
		zf = z.reshape(-1, cfg.codebook_dim)
		gap, tau = DO.gap_and_tau(zf, embed)
		share = float((gap < tau).double().mean())
		assert share <= 0.02, f"{name} {tag}: {share:.3f} of the positions are near ties (tau {tau:.3e})"
		tie = torch.nonzero(gap < tau).reshape(-1)
		out.update({f"input_seed_{tag}": np.int64(s), f"codes_{tag}": codes.numpy(), f"gap_{tag}": gap.numpy(), f"tau_{tag}": np.float64(tau),
					f"tie_idx_{tag}": tie.numpy(), f"z_tie_{tag}": zf[tie].numpy(),
					f"z_{tag}": z[:, ::zs].numpy(), f"dec_mel_{tag}": dec_mel[..., ::ms].numpy(), f"dec_hidden_{tag}": dec_hidden[..., ::hs].numpy()})
		if name == "dvae_small":
			out[f"mel_{tag}"] = mel.numpy()
		for dn, (zl, ml, hl) in low.items():
			out.update({f"z_{dn}_{tag}": zl[:, ::zs].numpy(), f"dec_mel_{dn}_{tag}": ml[..., ::ms].numpy(), f"dec_hidden_{dn}_{tag}": hl[..., ::hs].numpy()})
		rel = lambda a, b: ((a - b).norm() / b.norm()).item()
		print(f"{name} {tag}: T4 {T4}, {distinct} distinct codes, near ties {share:.4f} (tau {tau:.3e}, min gap {gap.min().item():.3e}), z rms {z.pow(2).mean().sqrt():.3f}, "
			  f"autocast rel L2 z bf16 {rel(low['bf16'][0], z):.2e} f16 {rel(low['f16'][0], z):.2e}, mel bf16 {rel(low['bf16'][1], dec_mel):.2e} f16 {rel(low['f16'][1], dec_mel):.2e}")
	np.savez(os.path.join(GOLDEN, name + ".npz"), **out)
	print(name, os.path.getsize(os.path.join(GOLDEN, name + ".npz")), "bytes")


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	os.makedirs(GOLDEN, exist_ok=True)
	make(mod, "dvae_small", W.DVAE_SMALL, 121, 122, ((1, 5, 1), (1, 61, 2), (3, 64, 3)), (1, 1, 1))
	make(mod, "dvae_full", W.DVAE_FULL, 123, 124, ((1, 517, 4), (2, 64, 5)), (4, 4, 16))


if __name__ == "__main__":
	main()
