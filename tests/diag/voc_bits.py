"""Diagnostic: digest of the three vocoders' waveforms under the library TTK_LIB selects, so that two builds of libttk can be compared bit for bit on
ONE box:   TTK_LIB=a.so python tests/diag/voc_bits.py > a.txt;  TTK_LIB=b.so python tests/diag/voc_bits.py > b.txt;  diff a.txt b.txt
Synthetic weights, seeded inputs.  BigVGAN and UnivNet (channel_size 32 and 16: the two LVC kernels) at batch 1 and 3, HiFiGAN with the narrow-channel
MFMA convolution and without (TTK_HIFI_NARROW, read at create), each in f32 and bf16, at 1, 5 and a few hundred frames / latents: the single-tile, the
ragged-tile and the many-tile paths of the GEMM and of the LVC / narrow-conv kernels.  Usage: python tests/diag/voc_bits.py [bigvgan] [univnet] [hifigan]"""
import dataclasses, hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.hifigan import HiFiGAN
from tortoise_tts_amd.univnet import UnivNet
from tortoise_tts_amd.vocoder import BigVGAN
dev = "cuda:0"
which = sys.argv[1:] or ["bigvgan", "univnet", "hifigan"]
LENGTHS = (1, 5, 300)


def report(label, wav):
	torch.cuda.synchronize()
	print(f"{label}: wav {hashlib.sha256(wav.float().cpu().numpy().tobytes()).hexdigest()[:16]} finite {bool(torch.isfinite(wav).all())}", flush=True)


def mels(B, T, seed):
	return (torch.randn(B, 100, T, generator=torch.Generator().manual_seed(seed)) * 2 - 5).to(dev)


if "bigvgan" in which:
	sd = W.synth_state_dict(W.vocoder_shapes(W.VOC_FULL), 0)
	for dtype in ("f32", "bf16"):
		v = BigVGAN(sd, W.VOC_FULL, dtype=dtype, device=dev)
		for B in (1, 3):
			for T in LENGTHS:
				report(f"bigvgan {dtype} B={B} T={T}", v.inference(mels(B, T, 1)))
		del v
if "univnet" in which:
	for ch in (32, 16):
		cfg = dataclasses.replace(W.UNIVNET_FULL, channel_size=ch)
		sd = W.synth_state_dict(W.univnet_shapes(cfg), 73)
		for dtype in ("f32", "bf16"):
			v = UnivNet(sd, cfg, dtype=dtype, device=dev)
			for B in (1, 3):
				for T in LENGTHS:
					z = torch.randn(B, cfg.noise_dim, T + 10, generator=torch.Generator().manual_seed(6))
					report(f"univnet c={ch} {dtype} B={B} T={T}", v.inference(mels(B, T, 5), z))
			del v
if "hifigan" in which:
	cfg = W.HIFIGAN_FULL
	sd = W.synth_state_dict(W.hifigan_shapes(cfg), 93)
	for narrow in ("1", "0"):
		os.environ["TTK_HIFI_NARROW"] = narrow
		for dtype in ("f32", "bf16"):
			v = HiFiGAN(sd, cfg, dtype=dtype, device=dev)
			for n in LENGTHS:
				gen = torch.Generator().manual_seed(5)
				lat, g = torch.randn(1, n, cfg.in_channels, generator=gen), torch.randn(1, cfg.cond_channels, generator=gen)
				report(f"hifigan narrow={narrow} {dtype} n={n}", v.inference(lat, g))
			del v
