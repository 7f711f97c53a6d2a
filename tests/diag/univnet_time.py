"""UnivNet vocoder time per utterance at configs[1] length (T = 1088 mel frames -> 278,528 samples), published config, both modes.
Usage: python tests/diag/univnet_time.py [--iters N].  Prints one line per mode: ms per call (mean and best of N, HIP events)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.univnet import UnivNet  # noqa: E402


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--T", type=int, default=1088)
	a = ap.parse_args()
	sd = W.synth_state_dict(W.univnet_shapes(W.UNIVNET_FULL), 73)
	g = torch.Generator().manual_seed(5)
	mel = (torch.randn(1, 100, a.T, generator=g) * 2 - 5).to("cuda:0")
	z = torch.randn(1, 64, a.T + 10, generator=g).to("cuda:0")
	for dtype in ("f32", "bf16"):
		voc = UnivNet(sd, W.UNIVNET_FULL, dtype=dtype, device="cuda:0")
		for _ in range(3):
			voc.inference(mel, z)
		torch.cuda.synchronize()
		ts = []
		for _ in range(a.iters):
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			voc.inference(mel, z)
			e1.record()
			torch.cuda.synchronize()
			ts.append(e0.elapsed_time(e1))
		print(f"univnet {dtype} T={a.T}: {sum(ts) / len(ts):.3f} ms mean, {min(ts):.3f} ms best of {a.iters}", flush=True)
		del voc


if __name__ == "__main__":
	main()
