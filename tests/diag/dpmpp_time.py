"""Diagnostic: what a DPM-Solver++(2M) loop costs next to the existing DDIM loop at equal step count, and what fewer steps buy (synthetic weights, bf16, one process;
informational, gates nothing).
Usage: python tests/diag/dpmpp_time.py [--iters N] [--steps S1,S2] [--T frames]
  `ttk_diff_sample_ddim` and `ttk_diff_sample_ms` at the benchmark's second configuration -- DIFF_FULL, T = 1088 frames, conditioning-free guidance -- at 80 and at 30
  steps: HIP events around one whole-loop call, 3 warm-up calls, best and mean of N, in milliseconds.  The four are interleaved round by round so that clock drift meets
  all alike.  The multistep update adds one f32 read and one f32 write of [100, T] per step to the update launch; more than 1 % over DDIM at equal steps wants a reason."""
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
	ap.add_argument("--steps", type=str, default="80,30")
	ap.add_argument("--T", type=int, default=1088)
	a = ap.parse_args()
	cfg = W.DIFF_FULL
	df = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(cfg), 0), cfg, dtype="bf16", device=DEV)
	T = a.T
	g = torch.Generator().manual_seed(1)
	E = torch.randn(1, cfg.model_channels, T, generator=g).to(DEV)
	start = torch.randn(1, cfg.in_channels, T, generator=g).to(DEV)
	x = torch.empty_like(start)
	s = _lib.stream_ptr()
	calls = {}
	for n in [int(v) for v in a.steps.split(",")]:
		d = get_diffuser(steps=n, cond_free=True)
		steps = (_lib.StepC * n)(*[d.step_coefs(i, "ddim") for i in range(n)])
		ms = (_lib.StepMsC * n)(*[d.step_coefs_ms(i, True) for i in range(n)])

		def ddim(n=n, steps=steps):
			x.copy_(start)
			_lib.check(df.lib.ttk_diff_sample_ddim(df._h, x.data_ptr(), E.data_ptr(), 1, T, steps, n, s), "ttk_diff_sample_ddim")

		def multistep(n=n, steps=steps, ms=ms):
			x.copy_(start)
			_lib.check(df.lib.ttk_diff_sample_ms(df._h, x.data_ptr(), E.data_ptr(), 1, T, steps, ms, n, s), "ttk_diff_sample_ms")
		calls[("ttk_diff_sample_ddim", n)] = ddim
		calls[("ttk_diff_sample_ms  ", n)] = multistep
	for fn in calls.values():
		for _ in range(3):
			fn()
	torch.cuda.synchronize()
	ts = {key: [] for key in calls}
	for _ in range(a.iters):
		for key, fn in calls.items():
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			fn()
			e1.record()
			torch.cuda.synchronize()
			ts[key].append(e0.elapsed_time(e1))
	for (name, n), v in ts.items():
		base = min(ts[("ttk_diff_sample_ddim", n)])
		print(f"T={T} bf16  {name} steps={n:3d}: {min(v):.3f} ms best, {sum(v) / len(v):.3f} ms mean of {a.iters}  ({min(v) / n * 1e3:.1f} us / step, {min(v) / base:.4f} x ddim at "
			  f"{n} steps)", flush=True)


if __name__ == "__main__":
	main()
