"""Regenerate the attention-map fixtures of tests/golden/ from the reference's own class: `UnifiedVoice.get_logits(..., get_attns=True)`
(models/unified_voice.py:508-516) on inputs prepared exactly as `forward` prepares them (:576-590), imported through oracle/ref_shim.load().  The
reference checkout is $TTK_REFERENCE (default /root/reference).

The model is `UnifiedVoice(layers, model_dim, heads, checkpointing=False)` loaded with `weights.synth_state_dict(weights.ar_score_shapes(cfg), seed)`
(file `peaked`: moved by `weights.stress_ar(.., "peaked")`).  With current transformers GPT-2 defaults to SDPA attention, which returns an empty
attentions tuple; the tool sets `model.gpt.config._attn_implementation = "eager"` (a setting, no code change) and gets `layers` tensors [B, H, S, S],
S = Tt + M + 5.  It asserts what the tests rely on: rows sum to 1 within 4e-7 and every entry above the diagonal is exactly 0.  The pass then runs on
`model.double()` and, on the f32 model again, under `torch.autocast("cpu", torch.bfloat16)`.  CPU, one thread, fixed zip timestamps: a rerun
reproduces every file byte for byte.

Per case `<c>` (keys `<c>_<name>`)
  cond [B, D] f32, text [B, Tt], codes [B, M] int64       the inputs (clipped and padded already: text_lengths and wav_lengths are full)
  layers [n] int64                                          the layers whose maps are stored
  maps [n, B, H, S, S] f32                                  the reference's f32 maps
  dev32 [n], devbf16 [n] float64                            max |P32 - P64| and max |Pbf16 - P64| of that layer: the reference's own deviations

Files
  ar_attn_small.npz    AR_SMALL, seed 41.  a: B=2 Tt=7 M=9 (S=21).  c: B=1 Tt=5 M=62 (S=72).  d: B=1 Tt=20 M=110 (S=135: past the 64- and
                       128-key edges).
  ar_attn_peaked.npz   AR_SMALL, seed 41 on the `peaked` stress weights, the inputs of case a.
  ar_attn_full.npz     AR_FULL, seed 42.  B=1 Tt=4 M=8 (S=17), all 30 x 16 maps.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tortoise_tts_amd import weights as W  # noqa: E402
import ref_shim  # noqa: E402
from make_golden_ar_score import gen, save  # noqa: E402


def attention_maps(model, cond, text, codes):
	"""forward's own preparation (unified_voice.py:576-590) and then get_logits(get_attns=True)"""
	F = torch.nn.functional
	with torch.no_grad():
		B, M = codes.shape
		mel = model.set_mel_padding(codes.clone(), torch.tensor([M * model.mel_length_compression] * B))
		text_in = F.pad(text, (0, 1), value=model.stop_text_token)
		mel = F.pad(mel, (0, 1), value=model.stop_mel_token)
		text_in, _ = model.build_aligned_inputs_and_targets(text_in, model.start_text_token, model.stop_text_token)
		text_emb = model.text_embedding(text_in) + model.text_pos_embedding(text_in)
		mel, _ = model.build_aligned_inputs_and_targets(mel, model.start_mel_token, model.stop_mel_token)
		mel_emb = model.mel_embedding(mel) + model.mel_pos_embedding(mel)
		attns = model.get_logits(cond.unsqueeze(1), text_emb, model.text_head, mel_emb, model.mel_head, get_attns=True)
	return torch.stack(list(attns))      # [layers, B, H, S, S]


def case(uv_mod, cfg, sd, tag, seed, B, Tt, M, inputs=None):
	model = uv_mod.UnifiedVoice(layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, checkpointing=False)
	missing, unexpected = model.load_state_dict(sd, strict=False)
	assert not unexpected and not [k for k in missing if k.startswith("gpt.h.") or k.endswith("embedding.weight")], (missing, unexpected)
	model.eval()
	model.gpt.config._attn_implementation = "eager"
	if inputs is None:
		cond = torch.randn(B, cfg.model_dim, generator=gen(seed + 1))
		text = torch.randint(1, 255, (B, Tt), generator=gen(seed + 2))
		codes = torch.randint(0, 8192, (B, M), generator=gen(seed + 3))
	else:
		cond, text, codes = inputs
	S = Tt + M + 5
	p32 = attention_maps(model, cond, text, codes)
	assert p32.shape == (cfg.layers, B, cfg.heads, S, S) and p32.dtype == torch.float32, (p32.shape, p32.dtype)
	assert (p32.sum(-1) - 1).abs().max() <= 4e-7, (p32.sum(-1) - 1).abs().max()
	assert (torch.triu(p32, diagonal=1) == 0).all()
	with torch.autocast("cpu", dtype=torch.bfloat16):
		pbf = attention_maps(model, cond, text, codes).double()
	model.double()
	p64 = attention_maps(model, cond.double(), text, codes)
	assert p64.dtype == torch.float64
	dev32 = (p32.double() - p64).abs().amax(dim=(1, 2, 3, 4))
	devbf = (pbf - p64).abs().amax(dim=(1, 2, 3, 4))
	print(f"  {tag}: maps {tuple(p32.shape)}, max |P32 - P64| {dev32.max():.3e}, max |Pbf16 - P64| {devbf.max():.3e}, largest entry off the first column "
		  f"{p32[..., 1:].max():.3f}")
	out = {"cond": cond, "text": text, "codes": codes, "layers": torch.arange(cfg.layers), "maps": p32, "dev32": dev32, "devbf16": devbf}
	return {f"{tag}_{k}": v.numpy() for k, v in out.items()}


def main():
	torch.set_num_threads(1)
	_, uv_mod = ref_shim.load()
	cfg, seed = W.AR_SMALL, 41
	sd = W.synth_state_dict(W.ar_score_shapes(cfg), seed)
	small = {"seed": np.int64(seed)}
	small.update(case(uv_mod, cfg, sd, "a", seed + 10, 2, 7, 9))
	small.update(case(uv_mod, cfg, sd, "c", seed + 30, 1, 5, 62))
	small.update(case(uv_mod, cfg, sd, "d", seed + 50, 1, 20, 110))
	save("ar_attn_small", small)
	a_inputs = tuple(torch.from_numpy(small[k].copy()) for k in ("a_cond", "a_text", "a_codes"))
	peaked = {"seed": np.int64(seed)}
	peaked.update(case(uv_mod, cfg, W.stress_ar(sd, cfg, "peaked"), "peaked", seed + 10, 2, 7, 9, inputs=a_inputs))
	save("ar_attn_peaked", peaked)
	cfg, seed = W.AR_FULL, 42
	full = {"seed": np.int64(seed)}
	full.update(case(uv_mod, cfg, W.synth_state_dict(W.ar_score_shapes(cfg), seed), "full", seed + 10, 1, 4, 8))
	save("ar_attn_full", full)


if __name__ == "__main__":
	main()
