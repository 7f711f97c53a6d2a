"""Per-token time of beam search at the benchmark's AR shape (AR_FULL, 64 text tokens, 250 mel tokens, stop token suppressed so every loop runs its
full length), bf16: `inference_speech(num_beams=4)` against the plain sampling loop at `num_return_sequences=4`, and the share of the two
beam launches -- the beam step (ttk_beam_step) and the KV reorder (ttk_ar_reorder_cache) -- timed on their own with HIP events over the
same cache lengths (reorder: a rotation of the four slices, every slice moves, after a prefill and `--tokens` decode steps; the time is per call
at that length, the loop's average is the value at about half of it).
Usage: python tests/diag/beam_time.py [--iters N] [--tokens T] [--beams B].  One line per measurement: ms per token (mean and best of N)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import _lib  # noqa: E402
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice, _BeamState  # noqa: E402

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
	ap.add_argument("--iters", type=int, default=5)
	ap.add_argument("--tokens", type=int, default=250)
	ap.add_argument("--beams", type=int, default=4)
	a = ap.parse_args()
	cfg, N, T = W.AR_FULL, a.beams, a.tokens
	sd = W.synth_state_dict(W.ar_shapes(cfg), 0)
	g = torch.Generator().manual_seed(1234)
	text = torch.randint(1, 255, (1, 64), generator=g).to(DEV)
	cond = torch.randn(1, cfg.model_dim, generator=g).to(DEV)
	model = UnifiedVoice(sd, cfg, dtype="bf16", device=DEV, max_batch=max(N, 4), max_ctx=64 + 4 + T + 8)
	kw = dict(do_sample=True, temperature=0.8, top_k=0, max_generate_length=T, suppress_tokens=[cfg.stop_mel_token])
	with torch.inference_mode():
		for label, fn in ((f"sampling loop, {N} candidates", lambda: model.inference_speech(cond, text, num_return_sequences=N, **kw)),
						  (f"beam search, {N} beams", lambda: model.inference_speech(cond, text, num_beams=N, num_return_sequences=1, **kw))):
			mean, best = timed(fn, a.iters)
			print(f"{label:34s} {mean / T:8.4f} ms/token mean  {best / T:8.4f} best   ({T} tokens, bf16)")
		# the two beam launches on their own
		st = _BeamState(model, N, T, kw)
		st.logits.copy_(model._prefill(cond, text, N))
		st.q.exponential_(1)
		tok = torch.randint(0, 8000, (N,), device=DEV)
		for _ in range(T // 2):
			model._decode(tok, st.logits)
		rot = torch.roll(torch.arange(N, device=DEV), 1)

		def step():
			st.col.zero_(); st.state.zero_(); st.state[2 * N] = 1
			_lib.check(model.lib.ttk_beam_step(_lib.C.byref(st.args), _lib.stream_ptr()), "ttk_beam_step")

		def step_resets_only():
			st.col.zero_(); st.state.zero_(); st.state[2 * N] = 1

		def reorder():
			_lib.check(model.lib.ttk_ar_reorder_cache(model._h, rot.data_ptr(), _lib.stream_ptr()), "ttk_ar_reorder_cache")

		def many(fn, n=20):
			return lambda: [fn() for _ in range(n)]
		m_step, b_step = timed(many(step), a.iters)
		m_rst, b_rst = timed(many(step_resets_only), a.iters)
		m_re, b_re = timed(many(reorder), a.iters)
		print(f"{'ttk_beam_step (2 launches)':34s} {(m_step - m_rst) / 20:8.4f} ms/call mean  {(b_step - b_rst) / 20:8.4f} best   (state resets subtracted)")
		print(f"{'ttk_ar_reorder_cache':34s} {m_re / 20:8.4f} ms/call mean  {b_re / 20:8.4f} best   (rotation of {N} slices, {T // 2} generated rows)")


if __name__ == "__main__":
	main()
