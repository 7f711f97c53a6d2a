"""Regenerate the UnivNet fixtures of tests/golden/ from the reference's own generator class (models/vocoder.py, imported by file path;
it needs nothing but torch).  The reference checkout is $TTK_REFERENCE (default /root/reference).

Weights are `weights.synth_state_dict(univnet_shapes(cfg), seed)` loaded into the reference's weight-normed modules as
`weight_v = w`, `weight_g = ||w||` (norm over every dimension but the first).  Inputs are seeded CPU draws: mel = 2 randn - 5,
z = randn (`univnet_oracle.fixture_inputs`, tests/univnet_oracle.py).  Everything runs on one CPU thread, so a rerun reproduces every array bit for bit.

Fixtures
  univnet_small.npz  UNIVNET_SMALL, B = 2, T = 13: seed, mel [2, 100, 13], z [2, 64, 23], forward [2, 1, 23 * 16] (of the padded mel),
                     audio [2, 1, 13 * 16] (`inference(mel, z)`), and the block-0 intermediates listed for the full fixture.
  univnet_full.npz   UNIVNET_FULL (the published config), B = 2, T = 13: the arrays above plus
                       kernels_frames [3]          the frames whose predicted kernels are stored
                       kernels [2, 4, 32, 64, 3, 3] block 0's predicted kernels at those frames
                       bias    [2, 4, 64, 23]       block 0's predicted biases (all frames)
                       convt_pre [2, 32, 184]       block 0's convt_pre output
                       lvc0    [2, 64, 184]         the first location-variable convolution's output (block 0, layer 0, before the gate)
                       keys                         the reference state_dict's sorted key list
  univnet_cfg1.npz   UNIVNET_FULL, B = 1, T = 1088 (BASELINE configs[1]): mel and z are not stored (2 x 0.3 MB); `mel_seed` / `z_seed`
                     regenerate them with `univnet_oracle.fixture_inputs`.  The f32 waveform (278,528 samples) is stored as every 4th sample (`audio_every4`)
                     plus the first and last 2,560 samples whole (`audio_head`, `audio_tail`).
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
from univnet_oracle import fixture_inputs as inputs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EDGE = 2560


def reference_module():
	ref = os.environ.get("TTK_REFERENCE", "/root/reference")
	spec = importlib.util.spec_from_file_location("_ref_univnet", os.path.join(ref, "tortoise_tts", "models", "vocoder.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


def build(mod, cfg, seed):
	g = mod.UnivNetGenerator(noise_dim=cfg.noise_dim, channel_size=cfg.channel_size, dilations=list(cfg.dilations), strides=list(cfg.strides),
							 lReLU_slope=cfg.lrelu_slope, kpnet_conv_size=cfg.kpnet_conv_size, hop_length=cfg.hop_length, n_mel_channels=cfg.num_mels)
	sd = W.synth_state_dict(W.univnet_shapes(cfg), seed)
	wn = {}
	for k, v in sd.items():
		if k.endswith(".weight") and v.dim() == 3:
			wn[k[:-len("weight")] + "weight_v"] = v
			wn[k[:-len("weight")] + "weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1)
		else:
			wn[k] = v
	g.load_state_dict(wn, strict=True)
	g.eval()
	return g


def pad_mel(mel):
	return torch.cat([mel, torch.full((mel.shape[0], mel.shape[1], 10), -11.5129)], dim=2)


def fixture(mod, cfg, seed, B, T, mel_seed, z_seed, frames):
	g = build(mod, cfg, seed)
	mel, z = inputs(B, T, mel_seed, z_seed, cfg)
	with torch.no_grad():
		melp = pad_mel(mel)
		blk = g.res_stack[0]
		kern, bias = blk.kernel_predictor(melp)
		x = blk.convt_pre(g.conv_pre(z))
		lvc0 = blk.location_variable_convolution(blk.conv_blocks[0](x), kern[:, 0], bias[:, 0], hop_size=blk.cond_hop_length)
		out = dict(seed=np.int64(seed), mel=mel.numpy(), z=z.numpy(), forward=g.forward(melp, z).numpy(), audio=g.inference(mel, z).numpy(),
				   kernels_frames=np.asarray(frames, dtype=np.int64), kernels=kern[..., list(frames)].numpy(), bias=bias.numpy(),
				   convt_pre=x.numpy(), lvc0=lvc0.numpy(), keys=np.asarray(sorted(g.state_dict().keys())))
	return out


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	os.makedirs(GOLDEN, exist_ok=True)
	np.savez(os.path.join(GOLDEN, "univnet_small.npz"), **fixture(mod, W.UNIVNET_SMALL, 71, 2, 13, 1, 2, (0, 22)))
	np.savez(os.path.join(GOLDEN, "univnet_full.npz"), **fixture(mod, W.UNIVNET_FULL, 72, 2, 13, 3, 4, (0, 11, 22)))
	g = build(mod, W.UNIVNET_FULL, 73)
	mel, z = inputs(1, 1088, 5, 6)
	with torch.no_grad():
		a = g.inference(mel, z).numpy()
	np.savez(os.path.join(GOLDEN, "univnet_cfg1.npz"), seed=np.int64(73), mel_seed=np.int64(5), z_seed=np.int64(6), T=np.int64(1088),
			 audio_shape=np.asarray(a.shape, dtype=np.int64), audio_every4=a[..., ::4], audio_head=a[..., :EDGE], audio_tail=a[..., -EDGE:])
	for n in ("univnet_small", "univnet_full", "univnet_cfg1"):
		print(n, os.path.getsize(os.path.join(GOLDEN, n + ".npz")), "bytes")


if __name__ == "__main__":
	main()
