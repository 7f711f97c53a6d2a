"""Per-token time of greedy search at the benchmark's AR shape (AR_FULL, 64 text tokens, 250 mel tokens, stop token suppressed so every loop runs its
full length), bf16, one row: `inference_speech(do_sample=False)` against the sampling loop at `num_return_sequences=1` on the same build, and the two
token-step launches -- ttk_greedy_step and ttk_sample_step_warped with the CLI's warpers off (temperature 0.8) -- timed on their own with HIP events.
On a build without greedy search the script says so and times the sampling loop only (for the record of the commit before).
Usage: python tests/diag/greedy_time.py [--iters N] [--tokens T].  One line per measurement: ms per token (mean and best of N)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import _lib  # noqa: E402
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warm=2):
	for _ in range(warm):
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
	ap.add_argument("--tokens", type=int, default=250)
	a = ap.parse_args()
	cfg, T = W.AR_FULL, a.tokens
	sd = W.synth_state_dict(W.ar_shapes(cfg), 0)
	g = torch.Generator().manual_seed(1234)
	text = torch.randint(1, 255, (1, 64), generator=g).to(DEV)
	cond = torch.randn(1, cfg.model_dim, generator=g).to(DEV)
	model = UnifiedVoice(sd, cfg, dtype="bf16", device=DEV, max_batch=4, max_ctx=64 + 4 + T + 8)
	base = dict(max_generate_length=T, suppress_tokens=[cfg.stop_mel_token])
	has_greedy = hasattr(model.lib, "ttk_greedy_step")
	with torch.inference_mode():
		loops = [("sampling loop, 1 candidate", lambda: model.inference_speech(cond, text, do_sample=True, temperature=0.8, top_k=0, num_return_sequences=1, **base))]
		if has_greedy:
			loops.append(("greedy loop, 1 row", lambda: model.inference_speech(cond, text, do_sample=False, **base)))
		else:
			print("greedy search: not in this build")
		for label, fn in loops:
			ids = fn()
			assert ids.shape == (1, T), ids.shape
			mean, best = timed(fn, a.iters)
			print(f"{label:34s} {mean / T:8.4f} ms/token mean  {best / T:8.4f} best   ({T} tokens, bf16)")
		# the token-step launches on their own: one row of 8194 scores
		V, n = cfg.number_mel_codes, 50
		lg = (torch.randn((1, V), generator=g) * 4).to(DEV)
		q = torch.empty((1, V), device=DEV).exponential_(1)
		mask = torch.zeros(V, dtype=torch.bool, device=DEV)
		mask[cfg.stop_mel_token] = True
		unf, tok, col = torch.ones(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV)
		ids = torch.zeros((1, n), dtype=torch.long, device=DEV)
		s = _lib.SampleArgs()
		s.scores, s.ld, s.B, s.V, s.q, s.ldq, s.suppress = lg.data_ptr(), V, 1, V, q.data_ptr(), V, mask.data_ptr()
		s.temperature, s.top_k, s.top_p, s.repetition_penalty = 0.8, 0, 1.0, 1.0
		s.stop_token, s.unfinished, s.tok, s.ids, s.ids_ld, s.ids_cols, s.col = cfg.stop_mel_token, unf.data_ptr(), tok.data_ptr(), ids.data_ptr(), n, n, col.data_ptr()

		def calls(entry, name):
			def run():
				col.zero_()
				for _ in range(n):
					_lib.check(entry(_lib.C.byref(s), _lib.stream_ptr()), name)
			return run
		entries = [("ttk_sample_step_warped", model.lib.ttk_sample_step_warped)] + ([("ttk_greedy_step", model.lib.ttk_greedy_step)] if has_greedy else [])
		for name, entry in entries:
			mean, best = timed(calls(entry, name), a.iters)
			print(f"{name:34s} {mean / n * 1000:8.2f} us/call mean  {best / n * 1000:8.2f} best   ({n} back-to-back launches, one row)")


if __name__ == "__main__":
	main()
