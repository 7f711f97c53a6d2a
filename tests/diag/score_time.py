"""Teacher-forced scoring time per call (AR_FULL, synthetic weights): `UnifiedVoice.forward(..., return_latent=False)` on B = 16 sequences of 64 text tokens and
250 mel codes, in bf16 and f32, next to `forward(..., return_latent=True)` on the same inputs (the dense pass both share) and the cross-entropy kernel alone on the
mel head's 16 x 252 rows of 8194 logits.
Usage: python tests/diag/score_time.py [--iters N] [--only bf16|f32].  Prints one line per measurement: ms (mean and best of N, HIP events, 3 warm-up calls; the
forward calls include their host-side id checks, which synchronise)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import _lib, weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice  # noqa: E402

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
	ap.add_argument("--iters", type=int, default=10)
	ap.add_argument("--only", default="", help="one of bf16, f32")
	a = ap.parse_args()
	cfg, B, Tt, M = W.AR_FULL, 16, 64, 250
	sd = W.synth_state_dict(W.ar_score_shapes(cfg), 0)
	gen = torch.Generator().manual_seed(7)
	cond = torch.randn(B, cfg.model_dim, generator=gen).to(DEV)
	text = torch.randint(1, 255, (B, Tt), generator=gen).to(DEV)
	codes = torch.randint(0, 8192, (B, M), generator=gen).to(DEV)
	lengths, wav = torch.full((B,), Tt), torch.full((B,), M * cfg.mel_length_compression)
	for dtype in ("bf16", "f32"):
		if a.only and a.only != dtype:
			continue
		m = UnifiedVoice(sd, cfg, dtype=dtype, device=DEV, max_batch=1, max_ctx=16)      # scoring does not use the KV cache
		for label, fn in (("forward(return_latent=False)", lambda: m.forward(cond, text, lengths, codes, wav, clip_inputs=False)),
						  ("forward(return_latent=True)", lambda: m.forward(cond, text, lengths, codes, wav, return_latent=True, clip_inputs=False))):
			mean, best = timed(fn, a.iters)
			print(f"score {dtype} B={B} Tt={Tt} M={M} {label}: {mean:.3f} ms mean, {best:.3f} ms best of {a.iters}", flush=True)
		del m
	rows, C, ld = B * (M + 2), cfg.number_mel_codes, 8196
	logits = torch.randn(rows, ld, generator=gen).to(DEV)
	target = torch.randint(0, C, (rows,), generator=gen).to(DEV)
	nll, mean_out, out_t = torch.empty(rows, device=DEV), torch.empty(1, device=DEV), torch.empty(B, C, M + 2, device=DEV)
	lib = _lib.load()
	for label, tp in (("rows + mean", None), ("rows + mean + transposed copy", out_t)):
		fn = lambda: _lib.check(lib.ttk_xent_rows(logits.data_ptr(), ld, rows, C, target.data_ptr(), nll.data_ptr(), mean_out.data_ptr(), _lib.ptr(tp), M + 2, _lib.stream_ptr()), "ttk_xent_rows")
		mean, best = timed(fn, a.iters)
		print(f"xent {rows} rows x {C} classes, {label}: {mean:.3f} ms mean, {best:.3f} ms best of {a.iters}", flush=True)


if __name__ == "__main__":
	main()
