"""Regenerate the teacher-forced scoring fixtures of tests/golden/ from the reference's own class: `UnifiedVoice.forward(..., return_latent=False)`
(models/unified_voice.py:544-612), imported through oracle/ref_shim.load().  The reference checkout is $TTK_REFERENCE (default /root/reference).

The model is `UnifiedVoice(layers, model_dim, heads, checkpointing=False)` loaded with `weights.synth_state_dict(weights.ar_score_shapes(cfg), seed)`
(case `peaked`: moved by `weights.stress_ar(.., "peaked")`, logits of standard deviation ~8).  The forward returns the two mean losses and the mel
logits only; the tool stands a recording proxy in for the module's `F` while the forward runs, so the logits and targets it stores are the very tensors
the reference hands to `F.cross_entropy` (:604-605) -- [B, C, T] logits and [B, T] targets of both heads.  The forward then runs a second time on
`model.double()`.  CPU, one thread, fixed zip timestamps: a rerun reproduces every file byte for byte.

Per case `<c>` (keys `<c>_<name>`)
  cond, text, text_lengths, codes, wav_lengths, clip    the inputs of the call (codes before set_mel_padding)
  text_targets [B, Tt'+2], mel_targets [B, M'+2]          the reference's targets; [:, :-2] of them are its clipped / padded text and codes
  loss_text, loss_mel                                    the returned f32 means
  nll_text, nll_mel                                      F.cross_entropy(reduction="none") of the reference's f32 logits, f32
  nll_text64, nll_mel64, loss_text64, loss_mel64         the same from model.double()
  lse_text64, lse_mel64                                  float64 logsumexp per row of the f32 logits
  text_logits [B, 256, Tt'+2]                            whole
  mel_logits [B, 8194, M'+2]                             whole (cases a, peaked)   or
  logit_cols [256], mel_logits_cols [B, 256, M'+2]       256 classes that include 0, 8191, 8192 (start) and 8193 (stop, in the ragged last tile)

For every stored row the tool asserts that the reference's own f32 cross-entropy lies within the bound the kernel is held to
(tests/test_gpu_xent.py: 1e-5 + 8 * 2^-24 * max(1, max|x_row|)) of the float64 cross-entropy of the same f32 logits.

Files
  ar_score_small.npz   AR_SMALL, seed 31.  a: B=2 Tt=7 M=9 full lengths, logits whole.  b: B=3 Tt=9 M=17, text_lengths (7, 5, 7), wav_lengths
                       (12 * 1024, 11 * 1024 + 500, 3 * 1024): clips to Tt'=7, M'=12, row 2 is padded with the stop token from position 4.
                       c62 / c63: B=1 Tt=5, M=62 / 63 (M + 2 = 64 / 65: the transposed tile exactly full / one frame past).
  ar_score_peaked.npz  AR_SMALL, seed 31 on the `peaked` stress weights, the inputs of case a, logits whole (a file of its own: two whole
                       [2, 8194, 11] logit tensors do not fit the 1 MiB a committed file may have).
  ar_score_full.npz    AR_FULL, seed 32.  B=2 Tt=6 M=10, clip_inputs=False, logit_cols slices.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from tortoise_tts_amd import weights as W  # noqa: E402
import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXED_COLS = (0, 8191, 8192, 8193)


def gen(seed):
	g = torch.Generator(device="cpu")
	g.manual_seed(seed)
	return g


def kernel_bound(logits_bct):
	"""per row [B, T]: 1e-5 + 8 * 2^-24 * max(1, max_c |x|)"""
	return 1e-5 + 8 * 2.0 ** -24 * logits_bct.double().abs().amax(dim=1).clamp(min=1.0)


class RecordingF:
	"""`torch.nn.functional` with `cross_entropy` recording what it is called with"""

	def __init__(self, real):
		self.real, self.calls = real, []

	def __getattr__(self, name):
		return getattr(self.real, name)

	def cross_entropy(self, logits, targets, **kw):
		self.calls.append((logits.detach().clone(), targets.detach().clone()))
		return self.real.cross_entropy(logits, targets, **kw)


def run_forward(uv_mod, model, cond, text, text_lengths, codes, wav_lengths, clip):
	rec, real = RecordingF(uv_mod.F), uv_mod.F
	uv_mod.F = rec
	try:
		with torch.no_grad():
			loss_text, loss_mel, mel_logits = model.forward(cond, text.clone(), text_lengths, codes.clone(), wav_lengths, clip_inputs=clip)
	finally:
		uv_mod.F = real
	(text_logits, text_targets), (mel_logits2, mel_targets) = rec.calls
	assert torch.equal(mel_logits, mel_logits2)
	return loss_text, loss_mel, text_logits, text_targets, mel_logits, mel_targets


def case(uv_mod, cfg, sd, tag, seed, B, Tt, M, text_lengths=None, wav_lengths=None, clip=True, whole=False, inputs=None):
	F = torch.nn.functional
	model = uv_mod.UnifiedVoice(layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, checkpointing=False)
	missing, unexpected = model.load_state_dict(sd, strict=False)
	assert not unexpected and not [k for k in missing if k.startswith("text_head") or k.startswith("mel_head")], (missing, unexpected)
	model.eval()
	if inputs is None:
		cond = torch.randn(B, cfg.model_dim, generator=gen(seed + 1))
		text = torch.randint(1, 255, (B, Tt), generator=gen(seed + 2))
		codes = torch.randint(0, 8192, (B, M), generator=gen(seed + 3))
	else:
		cond, text, codes = inputs
	text_lengths = torch.tensor(text_lengths if text_lengths is not None else [Tt] * B, dtype=torch.int64)
	wav_lengths = torch.tensor(wav_lengths if wav_lengths is not None else [M * cfg.mel_length_compression] * B, dtype=torch.int64)
	for b in range(B):      # what a padded micro-batch holds behind a text's length
		text[b, int(text_lengths[b]):] = 0
	lt, lm, tl, tt, ml, mt = run_forward(uv_mod, model, cond, text, text_lengths, codes, wav_lengths, clip)
	model.double()
	lt64, lm64, tl64, tt64, ml64, mt64 = run_forward(uv_mod, model, cond.double(), text, text_lengths, codes, wav_lengths, clip)
	assert torch.equal(tt, tt64) and torch.equal(mt, mt64)
	out = {"cond": cond, "text": text, "text_lengths": text_lengths, "codes": codes, "wav_lengths": wav_lengths, "clip": torch.tensor(int(clip)),
		   "text_targets": tt, "mel_targets": mt, "loss_text": lt, "loss_mel": lm, "loss_text64": lt64, "loss_mel64": lm64, "text_logits": tl}
	for name, logits, targets, logits64 in (("text", tl, tt, tl64), ("mel", ml, mt, ml64)):
		rows = F.cross_entropy(logits, targets, reduction="none")
		rows_of_f32 = F.cross_entropy(logits.double(), targets, reduction="none")
		bound = kernel_bound(logits)
		worst = ((rows.double() - rows_of_f32).abs() / bound).max().item()
		assert worst <= 1.0, f"{tag} {name}: the reference's f32 cross-entropy is {worst:.2f} of the kernel bound away from float64"
		out.update({f"nll_{name}": rows, f"nll_{name}64": F.cross_entropy(logits64, targets, reduction="none"), f"lse_{name}64": torch.logsumexp(logits.double(), dim=1)})
		print(f"  {tag} {name}: logits {tuple(logits.shape)} std {logits.std():.2f} max|x| {logits.abs().max():.1f}, mean nll {rows.mean():.4f}, f32 vs f64-of-f32 rows at {worst:.2f} of the bound, "
			  f"f32 vs double model: logits {(logits.double() - logits64).abs().max():.2e}")
	if whole:
		out["mel_logits"] = ml
	else:
		cols = torch.cat([torch.randperm(8190, generator=gen(seed + 4))[:256 - len(FIXED_COLS)] + 1, torch.tensor(FIXED_COLS)]).sort().values
		assert cols.unique().numel() == 256
		out.update({"logit_cols": cols, "mel_logits_cols": ml[:, cols]})
	if cfg.stop_mel_token in mt[:, :-2]:
		print(f"  {tag}: {int((mt[:, :-2] == cfg.stop_mel_token).sum())} padded positions have the stop token as target")
	return {f"{tag}_{k}": v.numpy() for k, v in out.items()}


def save(name, arrays):
	"""an .npz np.load reads, with fixed member timestamps: the file's bytes depend on the arrays alone"""
	path = os.path.join(GOLDEN, name + ".npz")
	with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
		for k, v in arrays.items():
			buf = io.BytesIO()
			a = np.asarray(v)
			np.lib.format.write_array(buf, a if a.flags.c_contiguous else np.ascontiguousarray(a), allow_pickle=False)
			info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
			info.external_attr = 0o644 << 16
			z.writestr(info, buf.getvalue())
	size = os.path.getsize(path)
	assert size < 1_000_000, f"{name}: {size} bytes"
	print(name, size, "bytes")


def main():
	torch.set_num_threads(1)
	_, uv_mod = ref_shim.load()
	os.makedirs(GOLDEN, exist_ok=True)
	cfg, seed = W.AR_SMALL, 31
	sd = W.synth_state_dict(W.ar_score_shapes(cfg), seed)
	small = {"seed": np.int64(seed)}
	small.update(case(uv_mod, cfg, sd, "a", seed + 10, 2, 7, 9, whole=True))
	small.update(case(uv_mod, cfg, sd, "b", seed + 20, 3, 9, 17, text_lengths=(7, 5, 7), wav_lengths=(12 * 1024, 11 * 1024 + 500, 3 * 1024)))
	small.update(case(uv_mod, cfg, sd, "c62", seed + 30, 1, 5, 62))
	small.update(case(uv_mod, cfg, sd, "c63", seed + 40, 1, 5, 63))
	assert small["b_text_targets"].shape == (3, 9) and small["b_mel_targets"].shape == (3, 14) and (small["b_mel_targets"][2, 4:] == cfg.stop_mel_token).all()
	save("ar_score_small", small)
	a_inputs = tuple(torch.from_numpy(small[k].copy()) for k in ("a_cond", "a_text", "a_codes"))
	peaked = {"seed": np.int64(seed)}
	peaked.update(case(uv_mod, cfg, W.stress_ar(sd, cfg, "peaked"), "peaked", seed + 10, 2, 7, 9, whole=True, inputs=a_inputs))
	save("ar_score_peaked", peaked)
	cfg, seed = W.AR_FULL, 32
	full = {"seed": np.int64(seed)}
	full.update(case(uv_mod, cfg, W.synth_state_dict(W.ar_score_shapes(cfg), seed), "full", seed + 10, 2, 6, 10, clip=False))
	save("ar_score_full", full)


if __name__ == "__main__":
	main()
