"""Run-time LoRA switch time (AR_FULL, synthetic weights, bf16, rank 128 on all 120 block matrices): `enable_lora` between two loaded adapters and `disable_lora`
on a live handle, next to what changing the voice costs without run-time adapters -- the adapter folded on the host and a second handle built from the result
(`checkpoint.materialize_lora` + `select_hot_path` + `UnifiedVoice(...)`; the checkpoint is in memory here, so the file read `load_autoregressive_state` would add
is not in the figure) -- and one `inference_speech` of the benchmark's shape (64 text tokens, 16 candidates x 250 mel tokens, stop token suppressed) before and
after a switch, interleaved, with the spread of both: the decode step reads the same buffers, so the two must agree within it.
Usage: python tests/diag/lora_time.py [--iters N] [--rank R] [--rounds K] [--no-rebuild]  (--rounds 0 --no-rebuild: the switches alone, e.g. under a kernel trace).  HIP events for the switches (3 warm-up switches, mean and best of N),
wall time for the rebuild (it synchronises by itself) and for the generations."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import checkpoint as ck, weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice, lora_modules  # noqa: E402

DEV = "cuda:0"


def synth_adapter(cfg, rank, seed):
	g = torch.Generator().manual_seed(seed)
	shapes, out = W.ar_shapes(cfg), {}
	for m in lora_modules(cfg):
		K, N = shapes[m + ".weight"]
		out[m + ".parametrizations.weight.0.lora_A"] = torch.randn(rank, N, generator=g) * (0.02 / rank ** 0.5)
		out[m + ".parametrizations.weight.0.lora_B"] = torch.randn(K, rank, generator=g) * 0.1
	return out


def event_ms(fn, before=None):
	if before:
		before()
	torch.cuda.synchronize()
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	fn()
	e1.record()
	torch.cuda.synchronize()
	return e0.elapsed_time(e1)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--rank", type=int, default=128)
	ap.add_argument("--rounds", type=int, default=5, help="generations before and after a switch, interleaved")
	ap.add_argument("--no-rebuild", action="store_true", help="skip the host fold + second handle")
	a = ap.parse_args()
	cfg = W.AR_FULL
	sd = W.synth_state_dict(W.ar_shapes(cfg), 0)
	ads = [synth_adapter(cfg, a.rank, s) for s in (1, 2)]
	print(f"adapter: rank {a.rank} on {len(lora_modules(cfg))} matrices, {sum(t.numel() for t in ads[0].values()) * 4 / 1e6:.1f} MB", flush=True)
	t0 = time.perf_counter()
	m = UnifiedVoice(sd, cfg, dtype="bf16", device=DEV, max_batch=16, adapters=True)
	torch.cuda.synchronize()
	print(f"UnifiedVoice(adapters=True) from memory: {time.perf_counter() - t0:.2f} s", flush=True)
	t0 = time.perf_counter()
	m.load_lora("a", ads[0])
	m.load_lora("b", ads[1])
	torch.cuda.synchronize()
	print(f"load_lora x 2 (check + upload): {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
	for i in range(3):
		m.enable_lora("ab"[i & 1])
	m.enable_lora("b")
	swap = [event_ms(lambda: m.enable_lora("ab"[i & 1])) for i in range(a.iters)]
	off = [event_ms(m.disable_lora, before=lambda: m.enable_lora("a")) for _ in range(a.iters)]
	on = [event_ms(lambda: m.enable_lora("a"), before=m.disable_lora) for _ in range(a.iters)]
	for label, ts in (("enable_lora, adapter -> adapter", swap), ("disable_lora", off), ("enable_lora, base -> adapter", on)):
		print(f"{label}: {sum(ts) / len(ts):.3f} ms mean, {min(ts):.3f} ms best of {len(ts)}", flush=True)
	best_swap = min(swap)

	gen = torch.Generator().manual_seed(7)
	cond = torch.randn(1, cfg.model_dim, generator=gen).to(DEV)
	text = torch.randint(1, 255, (1, 64), generator=gen).to(DEV)
	kw = dict(do_sample=True, num_return_sequences=16, max_generate_length=250, temperature=0.8, top_k=0, suppress_tokens=[cfg.stop_mel_token])

	def generate():
		torch.cuda.synchronize()
		t = time.perf_counter()
		with torch.inference_mode():
			m.inference_speech(cond, text, **kw)
		torch.cuda.synchronize()
		return (time.perf_counter() - t) * 1e3
	times = {"base": [], "adapted": []}
	if a.rounds:
		m.disable_lora()
		generate()                                           # warm-up: captures the step
	for _ in range(a.rounds):
		m.disable_lora()
		times["base"].append(generate())
		m.enable_lora("a")
		times["adapted"].append(generate())
	for k, ts in times.items():
		ts = sorted(ts)
		if not ts:
			continue
		print(f"inference_speech 16 x 250, {k}: median {ts[len(ts) // 2]:.2f} ms, min {ts[0]:.2f}, max {ts[-1]:.2f} over {len(ts)} interleaved runs", flush=True)
	del m
	if a.no_rebuild:
		return
	t0 = time.perf_counter()
	merged = ck.materialize_lora(sd, ads[0])
	t1 = time.perf_counter()
	picked = ck.select_hot_path(merged, W.ar_shapes(cfg), "autoregressive")
	fresh = UnifiedVoice(picked, cfg, dtype="bf16", device=DEV, max_batch=16)
	torch.cuda.synchronize()
	t2 = time.perf_counter()
	print(f"rebuild: materialize_lora {t1 - t0:.2f} s + UnifiedVoice {t2 - t1:.2f} s = {t2 - t0:.2f} s  ({(t2 - t0) * 1e3 / best_swap:.0f} x the best adapter -> adapter switch)", flush=True)
	del fresh


if __name__ == "__main__":
	main()
