"""DiscreteVAE time per call (published config, synthetic weights): `get_codebook_indices` and `decode` of one 6 s clip (517 mel frames -> 130 codes)
and of a batch of 16 such clips, in f32, bf16 and f16, and the quantizer alone on the same row counts (130 and 2080 rows against 8192 codes).
Usage: python tests/diag/dvae_time.py [--iters N] [--only f32|bf16|f16].  Prints one line per measurement: ms (mean and best of N, HIP events,
3 warm-up calls; decode includes its host-side check of the codes, which synchronises)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.dvae import DiscreteVAE  # noqa: E402

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
	ap.add_argument("--only", default="", help="one of f32, bf16, f16")
	a = ap.parse_args()
	cfg = W.DVAE_FULL
	sd = W.synth_state_dict(W.dvae_shapes(cfg), 123)
	gen = torch.Generator().manual_seed(5)
	sd["codebook.embed"] = torch.randn(cfg.codebook_dim, cfg.num_tokens, generator=gen)
	for dtype in ("f32", "bf16", "f16"):
		if a.only and a.only != dtype:
			continue
		dv = DiscreteVAE(sd, cfg, dtype=dtype, device=DEV)
		for B in (1, 16):
			mel = (torch.randn(B, cfg.channels, 517, generator=gen) * 2 - 4).to(DEV)
			codes, z = dv.encode(mel)
			for label, fn in (("get_codebook_indices", lambda: dv.get_codebook_indices(mel)), ("decode", lambda: dv.decode(codes)),
							  ("quantizer alone", lambda: dv.quantize(z))):
				if label == "quantizer alone" and dtype != "f32":
					continue          # the same f32 kernel in every handle
				mean, best = timed(fn, a.iters)
				print(f"dvae {dtype} B={B} T=517 ({codes.shape[1]} codes per clip) {label}: {mean:.3f} ms mean, {best:.3f} ms best of {a.iters}", flush=True)
		del dv


if __name__ == "__main__":
	main()
