"""Beam search over a batch of lines against line by line, at the benchmark's AR shape (AR_FULL, bf16, 64 text tokens, 250 mel tokens, stop token suppressed so
every search runs its full length): `beam_search_lines` on G = 2 and G = 4 lines of 4 beams against G calls of `inference_speech(num_beams=4)`, on ONE handle,
the two routes alternating, timed with HIP events, best of --iters (20).
Usage: python tests/diag/beam_lines_time.py [--iters N] [--tokens T] [--beams B].  One line per group size: ms per group on either route and their ratio."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice  # noqa: E402

DEV = "cuda:0"


def once(fn):
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	fn()
	e1.record()
	torch.cuda.synchronize()
	return e0.elapsed_time(e1)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--tokens", type=int, default=250)
	ap.add_argument("--beams", type=int, default=4)
	a = ap.parse_args()
	cfg, N, T = W.AR_FULL, a.beams, a.tokens
	sd = W.synth_state_dict(W.ar_shapes(cfg), 0)
	g = torch.Generator().manual_seed(1234)
	texts = [torch.randint(1, 255, (1, 64), generator=g).to(DEV) for _ in range(4)]
	cond = torch.randn(1, cfg.model_dim, generator=g).to(DEV)
	model = UnifiedVoice(sd, cfg, dtype="bf16", device=DEV, max_batch=16, max_ctx=64 + 4 + T + 8)
	kw = dict(do_sample=True, temperature=0.8, top_k=0, max_generate_length=T, suppress_tokens=[cfg.stop_mel_token])
	with torch.inference_mode():
		for G in (2, 4):
			if G * N > 16:
				continue
			group = texts[:G]
			by_line = lambda: [model.inference_speech(cond, t, num_beams=N, num_return_sequences=1, **kw) for t in group]
			batch = lambda: model.beam_search_lines(cond, group, N, num_return_sequences=1, **kw)
			want, got = by_line(), batch()                        # warm both routes; the batch's lines are their own calls' results
			assert all(torch.equal(x, y) for x, y in zip(got, want))
			t_line, t_batch = [], []
			for _ in range(a.iters):                              # alternating: both routes see the same clocks
				t_line.append(once(by_line))
				t_batch.append(once(batch))
			bl, bb = min(t_line), min(t_batch)
			print(f"G = {G} lines x {N} beams, {T} tokens, bf16: line by line {bl:8.2f} ms   beam_search_lines {bb:8.2f} ms   ratio {bb / bl:5.2f}   "
				  f"(per token {bl / T:6.4f} vs {bb / T:6.4f} ms; one line's step x {bb / (bl / G):4.2f})", flush=True)


if __name__ == "__main__":
	main()
