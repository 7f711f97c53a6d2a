"""Random-voice time per latent batch (synthetic weights): `ttk_rlg_forward` for channels 1024 (the autoregressive latent) and 2048 (the diffusion
latent) at rows 1 and 16, warm -- the 25 MB / 101 MB of weights have been read by the warm-up calls, so what the 256 MB cache behind HBM keeps of
them is served from there.
Usage: python tests/diag/rlg_time.py [--iters N] [--reps R].  Two lines per shape, HIP events, 3 warm-up calls:
  call   one ttk_rlg_forward (six launches enqueued by the host) between the events: mean and best of N, in microseconds
  graph  R forwards captured once into a HIP graph, one replay between the events, divided by R: the device's time per forward without the host's
         launch pacing (mean and best of N replays)
Next to each: the floor of DESIGN.md section 15 (6 x 1.45 us of launch boundaries + the weights once at 6.4 TB/s)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import _lib, weights as W  # noqa: E402
from tortoise_tts_amd.random_latent import RandomLatentConverter  # noqa: E402

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
		ts.append(e0.elapsed_time(e1) * 1e3)
	return sum(ts) / len(ts), min(ts)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--reps", type=int, default=50)
	a = ap.parse_args()
	for channels in (1024, 2048):
		rlg = RandomLatentConverter(W.rlg_state_dict(channels, 0), channels, device=DEV)
		floor = W.RLG_LAYERS * 1.45 + W.RLG_LAYERS * channels * channels * 4 / 6.4e12 * 1e6
		for rows in (1, 16):
			noise = torch.randn(rows, channels, generator=torch.Generator().manual_seed(rows)).to(DEV)
			out = torch.empty_like(noise)
			fwd = lambda: _lib.check(rlg.lib.ttk_rlg_forward(rlg._h, noise.data_ptr(), rows, out.data_ptr(), _lib.stream_ptr()), "ttk_rlg_forward")
			mean, best = timed(fwd, a.iters)
			print(f"rlg channels={channels} rows={rows} call : {mean:.1f} us mean, {best:.1f} us best of {a.iters} (floor {floor:.1f} us)", flush=True)
			graph = torch.cuda.CUDAGraph()
			with torch.cuda.graph(graph):
				for _ in range(a.reps):
					fwd()
			mean, best = timed(graph.replay, a.iters)
			print(f"rlg channels={channels} rows={rows} graph: {mean / a.reps:.1f} us mean, {best / a.reps:.1f} us best of {a.iters} replays of {a.reps} forwards (floor {floor:.1f} us)", flush=True)
			del graph
		del rlg


if __name__ == "__main__":
	main()
