"""Regenerate the classifier fixtures of tests/golden/ from the reference's own class (models/classifier.py, loaded through oracle/ref_shim.py).  The
reference checkout is $TTK_REFERENCE (oracle/ref_shim.py has the default).

models/classifier.py:111 passes `do_checkpoint=False` to arch_utils.AttentionBlock, which does not take that keyword: instantiating the class as
written raises TypeError.  This tool rebinds the name `AttentionBlock` inside the loaded classifier module to a wrapper that drops the keyword and
calls the reference's own AttentionBlock; nothing else is changed.

Weights are `weights.synth_state_dict(classifier_shapes(cfg), seed)` (the reference zero-initialises every ResBlock's second conv and every proj_out;
with those the network would be its skip path).  Inputs are `classifier_oracle.fixture_audio(B, T, input_seed)`.  CPU, one thread: a rerun reproduces
every array bit for bit.

Per fixture: seed, keys (the reference's state_dict keys), tags.  Per case (tag = "<B>x<T>"): input_seed; the activations `stem`, `stage<l>` (behind
each Downsample) and `final` as f32 [B, C, L], longer ones with every `step_<name>`-th frame only; `emb`, `logits`; `emb_f64`, `logits_f64` from the
model in float64 with the GroupNorm parameters kept f32 (GroupNorm32 casts its input to f32); `emb_bf16`, `logits_bf16` from the reference's run under
torch.autocast("cpu", bfloat16); and `err_<name>` = max |f32 - float64| of the reference itself over the WHOLE array, for every activation, emb and
logits -- the yardstick of tests/test_classifier_oracle.py.
  classifier_small.npz  CLASSIFIER_SMALL, (B, T) = (1, 1), (1, 5), (1, 4096), (2, 4099), (1, 24000), with the audio stored
  classifier_full.npz   CLASSIFIER_FULL, (1, 5000), (2, 66000); the audio is regenerated from the seed
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from tortoise_tts_amd import weights as W  # noqa: E402
import classifier_oracle as CO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_module():
	import ref_shim
	ref_shim.load()
	mod = importlib.import_module("tortoise_tts.models.classifier")
	ref_block = mod.AttentionBlock

	def attention_block(*a, do_checkpoint=None, **k):
		return ref_block(*a, **k)
	mod.AttentionBlock = attention_block
	return mod


def run(model, x):
	"""the reference's forward, module by module, keeping the activations the fixtures store"""
	enc, acts = model.enc, {}
	h = acts["stem"] = enc.init(x)
	l = 0
	for m in enc.res:
		h = m(h)
		if hasattr(m, "op"):
			acts[f"stage{l}"] = h
			l += 1
	h = acts["final"] = enc.final(h)
	for blk in enc.attn:
		h = blk(h)
	emb = h[:, :, 0]
	return emb, model.head(emb), acts


def make(mod, name):
	cfg, tags = CO.CFGS[name]
	seed = CO.SEEDS[name]
	model = mod.AudioMiniEncoderWithClassifierHead(cfg.classes, spec_dim=cfg.spec_dim, embedding_dim=cfg.embedding_dim, depth=cfg.depth,
												   downsample_factor=cfg.downsample_factor, resnet_blocks=cfg.resnet_blocks, attn_blocks=cfg.attn_blocks,
												   num_attn_heads=cfg.num_attn_heads, base_channels=cfg.base_channels, dropout=cfg.dropout, kernel_size=cfg.kernel_size,
												   distribute_zero_label=cfg.distribute_zero_label)
	model.load_state_dict(W.synth_state_dict(W.classifier_shapes(cfg), seed), strict=True)
	model.eval()
	model64 = copy.deepcopy(model).double()
	for m in model64.modules():
		if isinstance(m, torch.nn.GroupNorm):
			m.float()
	out = dict(seed=np.int64(seed), keys=np.asarray(sorted(model.state_dict().keys())), tags=np.asarray(tags))
	rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
	for i, tag in enumerate(tags):
		B, T = (int(v) for v in tag.split("x"))
		s = 10 * seed + i
		x = CO.fixture_audio(B, T, s)
		with torch.no_grad():
			assert torch.equal(model(x), run(model, x)[1])      # the stepwise run is the reference's forward
			emb, logits, acts = run(model, x)
			emb64, logits64, acts64 = run(model64, x.double())
			with torch.autocast("cpu", dtype=torch.bfloat16):
				emb16, logits16, _ = run(model, x)
		assert [a.shape[2] for a in acts.values()] == cfg.stage_lengths(T) + [cfg.stage_lengths(T)[-1]]
		out[f"input_seed_{tag}"] = np.int64(s)
		if name == "classifier_small":
			out[f"audio_{tag}"] = x.numpy()
		for k, a in acts.items():
			step = CO.time_step(a.shape)
			out[f"{k}_{tag}"], out[f"step_{k}_{tag}"] = a[..., ::step].contiguous().numpy(), np.int64(step)
			out[f"err_{k}_{tag}"] = np.float64((a.double() - acts64[k]).abs().max().item())
		out.update({f"emb_{tag}": emb.numpy(), f"logits_{tag}": logits.numpy(), f"emb_f64_{tag}": emb64.numpy(), f"logits_f64_{tag}": logits64.numpy(),
					f"emb_bf16_{tag}": emb16.float().numpy(), f"logits_bf16_{tag}": logits16.float().numpy(),
					f"err_emb_{tag}": np.float64((emb.double() - emb64).abs().max().item()), f"err_logits_{tag}": np.float64((logits.double() - logits64).abs().max().item())})
		print(f"{name} {tag}: lengths {cfg.stage_lengths(T)}, emb rms {emb.pow(2).mean().sqrt():.3f} std {emb.std():.3f}, logits {logits.flatten().tolist()}, "
			  f"rel L2 emb f32 {rel(emb, emb64):.2e} bf16 {rel(emb16.float(), emb):.2e}, logits max dev bf16 {(logits16.float() - logits).abs().max():.2e}")
	path = os.path.join(GOLDEN, name + ".npz")
	np.savez(path, **out)
	print(name, os.path.getsize(path), "bytes")


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	os.makedirs(GOLDEN, exist_ok=True)
	for name in CO.CFGS:
		make(mod, name)


if __name__ == "__main__":
	main()
