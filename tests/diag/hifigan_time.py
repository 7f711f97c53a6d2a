"""HiFiGAN vocoder time per call at configs[1] length (250 latents -> 1088 frames -> 278,528 samples), published config: f32, bf16 with the
narrow-channel MFMA convolution (the default) and bf16 with every ResBlock on the segment GEMM (TTK_HIFI_NARROW=0, read at create).  Then the
time from the start of a streamed line to its first chunk (60 tokens, small AR model of the tests + the published vocoder geometry at the AR
model's width), against the time of the whole line.
Usage: python tests/diag/hifigan_time.py [--iters N] [--n LATENTS] [--no-stream].  Prints one line per measurement: ms (mean and best of N, HIP events)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.hifigan import HiFiGAN  # noqa: E402

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
	ap.add_argument("--n", type=int, default=250)
	ap.add_argument("--no-stream", action="store_true")
	ap.add_argument("--only", default="", help="one of f32, bf16, bf16-gemm: time that mode alone (for a kernel trace)")
	a = ap.parse_args()
	cfg = W.HIFIGAN_FULL
	sd = W.synth_state_dict(W.hifigan_shapes(cfg), 93)
	gen = torch.Generator().manual_seed(5)
	lat = torch.randn(1, a.n, cfg.in_channels, generator=gen).to(DEV)
	g = torch.randn(1, cfg.cond_channels, generator=gen).to(DEV)
	for label, dtype, narrow in (("f32", "f32", "1"), ("bf16", "bf16", "1"), ("bf16-gemm", "bf16", "0")):
		if a.only and a.only != label:
			continue
		os.environ["TTK_HIFI_NARROW"] = narrow
		voc = HiFiGAN(sd, cfg, dtype=dtype, device=DEV)
		mean, best = timed(lambda: voc.inference(lat, g), a.iters)
		print(f"hifigan {label} n={a.n} ({voc.samples(a.n)} samples): {mean:.3f} ms mean, {best:.3f} ms best of {a.iters}", flush=True)
		del voc
	os.environ["TTK_HIFI_NARROW"] = "1"
	if a.no_stream or a.only:
		return
	# time to the first chunk of a streamed line
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	acfg = W.AR_SMALL
	hcfg = W.HiFiGANConfig(in_channels=acfg.model_dim, cond_channels=acfg.model_dim)
	ar = UnifiedVoice(W.synth_state_dict(W.ar_shapes(acfg), 31), acfg, dtype="bf16", device=DEV, max_batch=1, max_ctx=320)
	voc = HiFiGAN(W.synth_state_dict(W.hifigan_shapes(hcfg), 37), hcfg, dtype="bf16", device=DEV)
	text = torch.randint(1, 255, (1, 20), generator=gen).to(DEV)
	cond = torch.randn(1, acfg.model_dim, generator=gen).to(DEV)
	firsts, totals, counts = [], [], []
	for it in range(a.iters + 2):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		ids = ar.compute_embeddings(cond, text)
		pairs = ar.get_generator(inputs=ids, max_length=ids.shape[1] + 250, temperature=0.8, top_k=0, do_sample=True, num_return_sequences=1)
		t_first, n = None, 0
		for chunk in voc.stream(pairs, cond):
			chunk.cpu()                      # the consumer has the samples
			if t_first is None:
				t_first = time.perf_counter() - t0
			n += chunk.shape[-1]
		t_all = time.perf_counter() - t0
		if it >= 2:
			firsts.append(t_first * 1e3); totals.append(t_all * 1e3); counts.append(n)
	print(f"hifigan stream (AR_SMALL bf16, 250 tokens max): first chunk after {sum(firsts) / len(firsts):.2f} ms mean / {min(firsts):.2f} ms best, "
		  f"whole line {sum(totals) / len(totals):.2f} ms mean, {counts[0]} samples", flush=True)


if __name__ == "__main__":
	main()
