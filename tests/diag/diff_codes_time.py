"""Diagnostic: what the diffusion model's token conditioning costs next to its latent conditioning (synthetic weights, bf16, one process).
Usage: python tests/diag/diff_codes_time.py [--iters N] [--runs R] [--skip-e2e]
  pre-pass   `ttk_diff_precompute_codes` (gather + 3 attention blocks + shared tail; also with mel_head) against `ttk_diff_precompute` (cast + k = 3 conv + 4
             attention blocks + the same tail) at DIFF_FULL, M = 272 codes / latent rows -> T = 1088 frames: HIP events around one call, 3 warm-up calls, mean
             and best of N, in microseconds
  e2e        `TTSHotPath.inference` at the benchmark's second configuration (64 text tokens, 16 candidates, 250 AR steps at most, 80 DDIM steps) with
             diffusion_conditioning="codes" against "latents": wall time around the call with a device sync, 1 warm-up run, best of R, in milliseconds"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import _lib, weights as W  # noqa: E402
from tortoise_tts_amd.diffusion import DiffusionTTS, nearest_index  # noqa: E402

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
	ap.add_argument("--runs", type=int, default=3)
	ap.add_argument("--skip-e2e", action="store_true")
	a = ap.parse_args()
	cfg = W.DIFF_FULL
	sd = W.synth_state_dict(W.diffusion_shapes(cfg), 0)
	sd.update(W.synth_state_dict(W.diffusion_code_shapes(cfg), 0))
	df = DiffusionTTS(sd, cfg, dtype="bf16", device=DEV, codes=True)
	M, T, C = 272, 1088, cfg.model_channels
	g = torch.Generator().manual_seed(1)
	codes = torch.randint(0, df.in_tokens, (1, M), generator=g).to(DEV)
	lat = torch.randn(1, M, cfg.in_latent_channels, generator=g).to(DEV)
	cond = torch.randn(1, 2 * C, generator=g).to(DEV)
	idx = nearest_index(M, T).to(DEV)
	E, mp = torch.empty(1, C, T, device=DEV), torch.empty(1, cfg.in_channels, T, device=DEV)
	s = _lib.stream_ptr()
	calls = {
		"latents  ttk_diff_precompute              ": lambda: _lib.check(df.lib.ttk_diff_precompute(df._h, lat.data_ptr(), cond.data_ptr(), idx.data_ptr(), 1, M, T, E.data_ptr(), s), "precompute"),
		"codes    ttk_diff_precompute_codes        ": lambda: _lib.check(df.lib.ttk_diff_precompute_codes(df._h, codes.data_ptr(), cond.data_ptr(), idx.data_ptr(), 1, M, T, E.data_ptr(), None, s), "precompute_codes"),
		"codes    ttk_diff_precompute_codes + mel  ": lambda: _lib.check(df.lib.ttk_diff_precompute_codes(df._h, codes.data_ptr(), cond.data_ptr(), idx.data_ptr(), 1, M, T, E.data_ptr(), mp.data_ptr(), s), "precompute_codes"),
		"         ttk_diff_mel_head                ": lambda: _lib.check(df.lib.ttk_diff_mel_head(df._h, E.data_ptr(), 1, T, mp.data_ptr(), s), "mel_head"),
	}
	for name, fn in calls.items():
		mean, best = timed(fn, a.iters)
		print(f"pre-pass M={M} T={T} bf16  {name}: {mean:.1f} us mean, {best:.1f} us best of {a.iters}", flush=True)
	if a.skip_e2e:
		return
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.inference import TTSHotPath
	ar = UnifiedVoice(W.synth_state_dict(W.ar_shapes(W.AR_FULL), 0), W.AR_FULL, dtype="bf16", device=DEV, max_batch=16, max_ctx=64 + 4 + 250 + 8)
	hot = TTSHotPath(ar, df)
	g = torch.Generator().manual_seed(1234)
	text = torch.randint(1, 255, (1, 64), generator=g).to(DEV)
	al, dl = torch.randn(1, 1024, generator=g).to(DEV), torch.randn(1, 2048, generator=g).to(DEV)
	kw = dict(max_ar_steps=250, max_diffusion_steps=80, ar_temp=0.8, candidates=16, suppress_tokens=[8193])
	for mode in ("latents", "codes", "latents", "codes"):
		hot.inference(text, al, dl, diffusion_conditioning=mode, **kw)
		torch.cuda.synchronize()
		ts = []
		for _ in range(a.runs):
			t0 = time.perf_counter()
			mels, sec = hot.inference(text, al, dl, diffusion_conditioning=mode, **kw)
			torch.cuda.synchronize()
			ts.append(time.perf_counter() - t0)
		print(f"e2e configs[1] bf16  diffusion_conditioning={mode:8s}: {1e3 * min(ts):.1f} ms best of {a.runs} ({1e3 * sum(ts) / len(ts):.1f} mean) for {sec:.2f} s of audio", flush=True)


if __name__ == "__main__":
	main()
