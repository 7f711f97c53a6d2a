"""What the reference's samplers cost per utterance at the benchmark's AR shape (AR_FULL, synthetic weights, bf16, 64 text tokens, 16 candidates x 250 mel tokens,
stop token suppressed so every loop runs its full length): one `inference_speech` with today's token step (ttk_ar_sample_next), with each keyword alone
(ttk_ar_sample_next_ext) and with all of them on, HIP events around the whole call, best and median of N, the variants interleaved round by round on one handle.
Usage: python tests/diag/sample_ext_time.py [--iters N] [--plain-only].  One line per variant.  --plain-only times today's step alone (a build without the
second kernel, for the record of the commit before)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

DEV = "cuda:0"
VARIANTS = [
	("today's step (ttk_ar_sample_next)", {}),
	("today's step, repetition_penalty 2", dict(repetition_penalty=2.0)),
	("repetition_penalty 2, decay 0.5", dict(repetition_penalty=2.0, repetition_penalty_decay=0.5)),
	("stop_length_penalty 0.5", dict(stop_length_penalty=0.5)),
	("min_temperature 0.1", dict(min_temperature=0.1)),
	("mirostat tau 5 eta 0.1", dict(mirostat_tau=5.0, mirostat_eta=0.1)),
	("all four", dict(repetition_penalty=2.0, repetition_penalty_decay=0.5, stop_length_penalty=0.5, min_temperature=0.1, mirostat_tau=5.0, mirostat_eta=0.1)),
]


def measure(UnifiedVoice, W, variants, iters, tokens=250):
	cfg = W.AR_FULL
	sd = W.synth_state_dict(W.ar_shapes(cfg), 0)
	gen = torch.Generator().manual_seed(7)
	cond = torch.randn(1, cfg.model_dim, generator=gen).to(DEV)
	text = torch.randint(1, 255, (1, 64), generator=gen).to(DEV)
	m = UnifiedVoice(sd, cfg, dtype="bf16", device=DEV, max_batch=16)
	# (the decayed penalty replaces HF's, so it is timed next to HF's at the same factor; the first variant is the call tests/diag/lora_time.py times)
	kw = dict(do_sample=True, num_return_sequences=16, max_generate_length=tokens, temperature=0.8, top_k=0, suppress_tokens=[cfg.stop_mel_token])
	# each variant is interleaved with today's step alone: a handle keeps four generation states, and a round over more variants than that would rebuild and
	# re-capture a state per call and time that instead
	out = {}
	with torch.inference_mode():
		for pair in ([variants[:1]] if len(variants) == 1 else [[variants[0], v] for v in variants[1:]]):
			times = {label: [] for label, _ in pair}
			for label, knob in pair:                               # warm-up: each variant captures its own step
				assert m.inference_speech(cond, text, **kw, **knob).shape == (16, tokens)
			for _ in range(iters):
				for label, knob in pair:
					e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
					torch.cuda.synchronize()
					e0.record()
					m.inference_speech(cond, text, **kw, **knob)
					e1.record()
					torch.cuda.synchronize()
					times[label].append(e0.elapsed_time(e1))
			for label, ts in times.items():
				ts = sorted(ts)
				print(f"inference_speech 16 x {tokens}, {label:36s}: best {ts[0]:8.2f} ms  median {ts[len(ts) // 2]:8.2f}  max {ts[-1]:8.2f}  over {len(ts)} interleaved runs", flush=True)
			print(flush=True)
			out.update(times)
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--iters", type=int, default=20)
	ap.add_argument("--plain-only", action="store_true")
	a = ap.parse_args()
	from tortoise_tts_amd import weights as W
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	measure(UnifiedVoice, W, VARIANTS[:1] if a.plain_only else VARIANTS, a.iters)


if __name__ == "__main__":
	main()
