"""Cost of the text-to-audio alignment on AR_FULL in bf16 at Tt = 64, M = 250: `UnifiedVoice.text_alignment` (default heads) against
`forward(return_latent=True)` alone, HIP events, best of 20, the two interleaved; then `TTS.inference` of one line (full-size models, synthetic weights,
token ids as the text, 250 sampled codes) with and without `return_timings`, wall clock around a synchronised call, best of 5, interleaved.  No threshold: the
numbers belong in README.md.
Run on an MI355X:  python tests/diag/align_time.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.autoregressive import UnifiedVoice  # noqa: E402

DEV, TT, M, REPS = "cuda:0", 64, 250, 20


def timed(fn):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	fn()
	b.record()
	torch.cuda.synchronize()
	return a.elapsed_time(b)


def main():
	cfg = W.AR_FULL
	model = UnifiedVoice(W.synth_state_dict(W.ar_shapes(cfg), 42), cfg, dtype="bf16", device=DEV, max_batch=1)
	g = torch.Generator().manual_seed(1)
	cond = torch.randn(1, cfg.model_dim, generator=g).to(DEV)
	text = torch.randint(1, 255, (1, TT), generator=g).to(DEV)
	codes = torch.randint(0, 8192, (1, M), generator=g).to(DEV)
	lengths = (torch.tensor([TT]), codes, torch.tensor([M * cfg.mel_length_compression]))
	latents = lambda: model.forward(cond, text, lengths[0], lengths[1], lengths[2], return_latent=True, clip_inputs=False)
	align = lambda: model.text_alignment(cond, text, codes)
	for _ in range(3):
		latents(), align()
	best = {"latent pass": float("inf"), "text_alignment": float("inf")}
	for _ in range(REPS):
		best["latent pass"] = min(best["latent pass"], timed(latents))
		best["text_alignment"] = min(best["text_alignment"], timed(align))
	for k, v in best.items():
		print(f"{k}: {v:.3f} ms (best of {REPS}, Tt={TT}, M={M}, bf16, {cfg.layers} layers)")
	tts_inference(model, cond, text)


def tts_inference(ar, cond, text):
	import time
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.tts import TTS
	from tortoise_tts_amd.vocoder import BigVGAN

	class Ids:      # a tokenizer that answers every line with the ids above; words are runs between id 2 ([SPACE] of the TorToiSe vocabulary)
		def encode(self, line):
			return text[0].tolist()

		def get_vocab(self):
			return {"[SPACE]": 2}

		def decode(self, ids):
			return " ".join(str(int(i)) for i in ids)
	df = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(W.DIFF_FULL), 0), W.DIFF_FULL, dtype="bf16", device=DEV)
	voc = BigVGAN(W.synth_state_dict(W.vocoder_shapes(W.VOC_FULL), 0), W.VOC_FULL, dtype="bf16", device=DEV)
	tts = TTS(ar, df, Ids(), vocoder=voc)
	voice = {"latent": (cond, torch.randn(1, 2 * W.DIFF_FULL.model_channels, generator=torch.Generator().manual_seed(2)).to(DEV))}
	kw = dict(max_ar_steps=M, seed=3)

	def run(**extra):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		tts.inference("one line", voice, **kw, **extra)
		torch.cuda.synchronize()
		return (time.perf_counter() - t0) * 1e3
	run(), run(return_timings=True)
	best = [float("inf"), float("inf")]
	for _ in range(5):
		best = [min(best[0], run()), min(best[1], run(return_timings=True))]
	print(f"TTS.inference: {best[0]:.1f} ms, with return_timings {best[1]:.1f} ms (one line, Tt={TT}, up to {M} codes, 80 DDIM steps, bf16, best of 5)")


if __name__ == "__main__":
	main()
