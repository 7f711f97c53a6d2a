"""Diagnostic: what the extended loop entry costs next to the existing DDIM loop (synthetic weights, bf16, one process; informational, gates nothing).
Usage: python tests/diag/sampler_ext_time.py [--iters N] [--steps S] [--T frames]
  `ttk_diff_sample_ddim` against `ttk_diff_sample_ext` at the benchmark's second configuration -- DIFF_FULL, T = 1088 frames, 80 steps, conditioning-free guidance --
  with mode 0 at eta = 0 (the same arithmetic through the new kernel), mode 0 at eta = 1 (one more [1, 100, T] f32 read per step) and mode 2 (the reverse ODE): HIP
  events around one whole-loop call, 3 warm-up calls, best and mean of N, in milliseconds.  The four are interleaved round by round so that clock drift meets all alike."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import _lib, weights as W  # noqa: E402
from tortoise_tts_amd.diffusion import DiffusionTTS, get_diffuser  # noqa: E402

DEV = "cuda:0"


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--steps", type=int, default=80)
	ap.add_argument("--T", type=int, default=1088)
	a = ap.parse_args()
	cfg = W.DIFF_FULL
	df = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(cfg), 0), cfg, dtype="bf16", device=DEV)
	n, T = a.steps, a.T
	g = torch.Generator().manual_seed(1)
	E = torch.randn(1, cfg.model_channels, T, generator=g).to(DEV)
	start = torch.randn(1, cfg.in_channels, T, generator=g).to(DEV)
	noise = torch.randn(n, 1, cfg.in_channels, T, generator=g).to(DEV)
	d = get_diffuser(steps=n, cond_free=True)
	steps = (_lib.StepC * n)(*[d.step_coefs(i, "ddim") for i in range(n)])
	ext = {name: (_lib.StepExtC * n)(*[d.step_coefs_ext(i, mode, eta, True) for i in range(n)]) for name, mode, eta in (("eta0", 0, 0.0), ("eta1", 0, 1.0), ("reverse", 2, 0.0))}
	x = torch.empty_like(start)
	s = _lib.stream_ptr()

	def ddim():
		x.copy_(start)
		_lib.check(df.lib.ttk_diff_sample_ddim(df._h, x.data_ptr(), E.data_ptr(), 1, T, steps, n, s), "ttk_diff_sample_ddim")

	def ext_loop(name):
		def run():
			x.copy_(start)
			_lib.check(df.lib.ttk_diff_sample_ext(df._h, x.data_ptr(), E.data_ptr(), 1, T, steps, ext[name], n, noise.data_ptr() if name == "eta1" else None, s), "ttk_diff_sample_ext")
		return run
	calls = {"ttk_diff_sample_ddim               ": ddim, "ttk_diff_sample_ext  eta = 0       ": ext_loop("eta0"), "ttk_diff_sample_ext  eta = 1       ": ext_loop("eta1"),
			 "ttk_diff_sample_ext  reverse ODE   ": ext_loop("reverse")}
	for fn in calls.values():
		for _ in range(3):
			fn()
	torch.cuda.synchronize()
	ts = {name: [] for name in calls}
	for _ in range(a.iters):
		for name, fn in calls.items():
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			fn()
			e1.record()
			torch.cuda.synchronize()
			ts[name].append(e0.elapsed_time(e1))
	base = min(ts["ttk_diff_sample_ddim               "])
	for name, v in ts.items():
		print(f"T={T} steps={n} bf16  {name}: {min(v):.3f} ms best, {sum(v) / len(v):.3f} ms mean of {a.iters}  ({min(v) / n * 1e3:.1f} us / step, {min(v) / base:.4f} x ddim)", flush=True)


if __name__ == "__main__":
	main()
