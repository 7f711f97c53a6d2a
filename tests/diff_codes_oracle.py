"""CPU restatement of the diffusion model's token conditioning (diffusion.py:1487-1515, the `else` of :1493, and `mel_head`, :1456 / :1512) in plain
torch, on the blocks of `tortoise_oracle.DiffusionOracle`: code_embedding rows -> three `code_converter` AttentionBlocks -> the code_norm / modulation /
nearest expansion every aligned conditioning shares; `mel_head` is one k = 3 convolution over the expanded embedding.  A helper, like dvae_oracle.py:
tests/test_diff_codes_oracle.py pins it against the reference's own results (tests/golden/diff_codes_*.npz), the GPU tests compare the HIP path with it."""
import torch
import torch.nn.functional as F

import tortoise_oracle as O
from tortoise_tts_amd import weights as W


def state_dict(cfg, seed, in_tokens=W.DIFF_CODE_TOKENS, bf16_exact=False):
	"""the seeded synthetic weights of a DiffusionTTS with token conditioning: the hot-path tensors exactly as without it, the code tensors from their own call"""
	sd = W.synth_state_dict(W.diffusion_shapes(cfg), seed, bf16_exact=bf16_exact)
	sd.update(W.synth_state_dict(W.diffusion_code_shapes(cfg, in_tokens), seed, bf16_exact=bf16_exact))
	return sd


def fixture_codes(b, M, seed, in_tokens):
	return torch.randint(0, in_tokens, (b, M), generator=torch.Generator().manual_seed(seed))


class DiffCodesOracle(O.DiffusionOracle):
	def mel_head(self, E):
		return F.conv1d(E, self.w["mel_head.weight"], self.w["mel_head.bias"], padding=1)

	def timestep_independent_codes(self, codes, cond, T, return_code_pred=False):
		"""codes [b, M] int64, cond [b, 2C] -> E [b, C, T] (and mel_pred [b, in_channels, T]); eval mode, so no unconditioned masking"""
		w, heads = self.w, self.cfg.num_heads
		scale, shift = torch.chunk(cond, 2, dim=1)
		h = F.embedding(codes, w["code_embedding.weight"]).permute(0, 2, 1)
		for i in range(3):
			h = O.attention_block(w, f"code_converter.{i}.", h, heads)
		h = O.group_norm32(h, w["code_norm.weight"], w["code_norm.bias"]) * (1 + scale.unsqueeze(-1)) + shift.unsqueeze(-1)
		E = F.interpolate(h, size=T, mode="nearest")
		return (E, self.mel_head(E)) if return_code_pred else E

	def forward_codes(self, x, t, codes, cond, return_code_pred=False):
		"""forward(x, t, aligned_conditioning=codes, conditioning_latent=cond[, return_code_pred=True]), diffusion.py:1517-1574"""
		E, mel_pred = self.timestep_independent_codes(codes, cond, x.shape[-1], True)
		out = self.forward(x, t, E)
		return (out, mel_pred) if return_code_pred else out
