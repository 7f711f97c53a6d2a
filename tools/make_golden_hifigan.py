"""Regenerate the HiFiGAN fixtures of tests/golden/ from the reference's own generator class (models/hifigan.py, imported by file path;
it needs nothing but torch).  The reference checkout is $TTK_REFERENCE (default /root/reference).

Weights are `weights.synth_state_dict(hifigan_shapes(cfg), seed)` loaded into the reference's weight-normed modules as `weight_v = w`,
`weight_g = ||w||` (norm over every dimension but the first; `cond_layer` carries no weight norm).  Inputs are seeded CPU draws
(`hifigan_oracle.fixture_inputs`, tests/hifigan_oracle.py).  The generator's `device` is set to the CPU and everything runs on one
thread, so a rerun reproduces every array bit for bit.

Fixtures
  hifigan_small.npz   HIFIGAN_SMALL, n = 13 and n = 2 latents.  Per n (suffix _13 / _2): latents [1, n, 128], g [1, 128], input_seed,
                      interp [1, 128, F] (after the two interpolations), conv_pre [1, 128, F] (conv_pre + cond_layer(g)),
                      ups0 [1, 64, 4 F] (the first transposed conv), stage0 [1, 64, 4 F] (the first stage's MRF mean), audio [1, 1, 8 F];
                      seed; keys (the reference state_dict's sorted key list).
  hifigan_full.npz    HIFIGAN_FULL (the config of models/__init__.py:126-138), n = 13 and n = 2: seed, keys, and per n latents, g, audio and
                      every 2nd frame (`interp_2_<n>`, `conv_pre_2_<n>`) / every 4th sample (`ups0_4_<n>`, `stage0_4_<n>`) of the intermediates,
                      which whole would not fit the size limit of a committed file.
  hifigan_cfg1.npz    HIFIGAN_FULL, n = 250 (BASELINE configs[1]: F = 1088 frames, 278,528 samples): the inputs are not stored
                      (`input_seed` regenerates them); the f32 waveform is stored as every 4th sample (`audio_every4`) plus the
                      first and last 2,560 samples whole (`audio_head`, `audio_tail`).
  hifigan_stream.npz  HIFIGAN_SMALL: the generator's waveform on the first 60, 100 and 117 latents of one seeded sequence of 117
                      (`wav_60`, `wav_100`, `wav_117`; `input_seed`, `seed`), from which tests compose the chunks of the streaming loop.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tortoise_tts_amd import weights as W  # noqa: E402
from hifigan_oracle import fixture_inputs as inputs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EDGE = 2560


def reference_module():
	ref = os.environ.get("TTK_REFERENCE", "/root/reference")
	spec = importlib.util.spec_from_file_location("_ref_hifigan", os.path.join(ref, "tortoise_tts", "models", "hifigan.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


def build(mod, cfg, seed):
	g = mod.HifiganGenerator(in_channels=cfg.in_channels, out_channels=1, resblock_type=cfg.resblock_type,
							 resblock_dilation_sizes=[list(d) for d in cfg.resblock_dilation_sizes], resblock_kernel_sizes=list(cfg.resblock_kernel_sizes),
							 upsample_kernel_sizes=list(cfg.upsample_kernel_sizes), upsample_initial_channel=cfg.upsample_initial_channel,
							 upsample_factors=list(cfg.upsample_factors), cond_channels=cfg.cond_channels)
	g.device = torch.device("cpu")
	sd = W.synth_state_dict(W.hifigan_shapes(cfg), seed)
	wn = {}
	for k, v in sd.items():
		if k.endswith(".weight") and v.dim() == 3 and not k.startswith("cond_layer."):
			wn[k[:-len("weight")] + "weight_v"] = v
			wn[k[:-len("weight")] + "weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1)
		else:
			wn[k] = v
	g.load_state_dict(wn, strict=True)
	g.eval()
	return g


def run(g, cfg, n, seed, sub=None):
	"""the waveform and the intermediates of one call, through hooks on the reference's own modules; sub = (frame step, sample step) of the stored intermediates"""
	lat, cond = inputs(n, seed, cfg)
	got = {}
	hooks = [g.conv_pre.register_forward_hook(lambda m, i, o: got.update(interp=i[0].clone())),
			 g.ups[0].register_forward_hook(lambda m, i, o: got.update(ups0=o.clone()))]
	with torch.no_grad():
		audio = g.inference(lat, cond)
		for h in hooks:
			h.remove()
		conv_pre = g.conv_pre(got["interp"]) + g.cond_layer(cond.unsqueeze(0).transpose(1, 2))          # forward :252-254
		z = g.resblocks[0](got["ups0"])
		for j in range(1, g.num_kernels):
			z += g.resblocks[j](got["ups0"])
		stage0 = z / g.num_kernels                                                                         # forward :258-264, i = 0
	fs, ss = sub or (1, 1)
	sf, sx = ("", "") if sub is None else (f"_{fs}", f"_{ss}")
	res = {f"latents_{n}": lat.numpy(), f"g_{n}": cond.numpy(), f"audio_{n}": audio.numpy(),
		   f"interp{sf}_{n}": got["interp"][..., ::fs].numpy(), f"conv_pre{sf}_{n}": conv_pre[..., ::fs].numpy(),
		   f"ups0{sx}_{n}": got["ups0"][..., ::ss].numpy(), f"stage0{sx}_{n}": stage0[..., ::ss].numpy()}
	return res, audio


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	os.makedirs(GOLDEN, exist_ok=True)
	for name, cfg, seed, sub in (("hifigan_small", W.HIFIGAN_SMALL, 91, None), ("hifigan_full", W.HIFIGAN_FULL, 92, (2, 4))):
		g = build(mod, cfg, seed)
		out = dict(seed=np.int64(seed), keys=np.asarray(sorted(g.state_dict().keys())))
		for n, s in ((13, 1), (2, 2)):
			res, audio = run(g, cfg, n, s, sub)
			out[f"input_seed_{n}"] = np.int64(s)
			out.update(res)
			print(name, n, "audio", tuple(audio.shape), "rms %.3f max %.3f" % (audio.pow(2).mean().sqrt(), audio.abs().max()))
		np.savez(os.path.join(GOLDEN, name + ".npz"), **out)
	g = build(mod, W.HIFIGAN_FULL, 93)
	lat, cond = inputs(250, 5)
	with torch.no_grad():
		a = g.inference(lat, cond).numpy()
	print("hifigan_cfg1 audio", a.shape, "rms %.3f max %.3f" % (float(np.sqrt((a ** 2).mean())), float(np.abs(a).max())))
	np.savez(os.path.join(GOLDEN, "hifigan_cfg1.npz"), seed=np.int64(93), input_seed=np.int64(5), n=np.int64(250),
			 audio_shape=np.asarray(a.shape, dtype=np.int64), audio_every4=a[..., ::4], audio_head=a[..., :EDGE], audio_tail=a[..., -EDGE:])
	g = build(mod, W.HIFIGAN_SMALL, 94)
	lat, cond = inputs(117, 7, W.HIFIGAN_SMALL)
	out = dict(seed=np.int64(94), input_seed=np.int64(7))
	with torch.no_grad():
		for n in (60, 100, 117):
			out[f"wav_{n}"] = g.inference(lat[:, :n], cond).numpy().reshape(-1)
	np.savez(os.path.join(GOLDEN, "hifigan_stream.npz"), **out)
	for n in ("hifigan_small", "hifigan_full", "hifigan_cfg1", "hifigan_stream"):
		print(n, os.path.getsize(os.path.join(GOLDEN, n + ".npz")), "bytes")


if __name__ == "__main__":
	main()
