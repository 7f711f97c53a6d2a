"""TorToiSe detector time per clip (published config, synthetic weights): `forward` on one 10 s clip (T = 240 000 samples at 24 kHz) and on a 1 s clip,
in f32 and bf16.  Usage: python tests/diag/classifier_time.py [--iters N] [--only f32|bf16].  Prints one line per measurement: ms (mean and best of
N, HIP events, 3 warm-up calls)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.classifier import AudioMiniEncoderWithClassifierHead  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters):
	for _ in range(3):
		fn()
	torch.cuda.synchronize()
	ts = []
	for _ in range(iters):
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		e0.record()
		fn()
		e1.record()
		torch.cuda.synchronize()
		ts.append(e0.elapsed_time(e1))
	return sum(ts) / len(ts), min(ts)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--only", default="", help="one of f32, bf16")
	a = ap.parse_args()
	cfg = W.CLASSIFIER_FULL
	sd = W.synth_state_dict(W.classifier_shapes(cfg), 133)
	gen = torch.Generator().manual_seed(5)
	for dtype in ("f32", "bf16"):
		if a.only and a.only != dtype:
			continue
		m = AudioMiniEncoderWithClassifierHead(sd, cfg, dtype=dtype, device=DEV)
		for T in (240000, 24000):
			x = (0.1 * torch.randn(1, 1, T, generator=gen)).to(DEV)
			mean, best = timed(lambda: m(x), a.iters)
			print(f"classifier {dtype} B=1 T={T} ({T / 24000:.0f} s, {cfg.stage_lengths(T)[-1]} positions) forward: {mean:.3f} ms mean, {best:.3f} ms best of {a.iters}", flush=True)
		del m


if __name__ == "__main__":
	main()
