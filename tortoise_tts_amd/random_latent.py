"""Random voices on libttk: the reference's `rlg` pair (`models/__init__.py:97-103`: `RandomLatentConverter(1024)` from `rlg_auto.pth` for the
autoregressive conditioning latent, `RandomLatentConverter(2048)` from `rlg_diffuser.pth` for the diffusion one; `models/random_latent_generator.py`)
over `ttk_rlg_*`: a Gaussian row through five EqualLinear layers and one nn.Linear, each layer one launch of the fused f32 linear kernel
(csrc/rlg.hip).

EqualLinear's forward multiplies its weight by `(1 / sqrt(in_dim)) * lr_mul` and its bias by `lr_mul` on every call; `fold_equal_linear` does that
once on the host with the reference's own torch expressions, so the kernel's operands are the reference's operands bit for bit.  f32 is the only
mode: the chain runs once per voice, and a 16-bit latent would move every later stage's input.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Mapping, Optional

import torch

from . import _lib
from .weights import RLG_LAYERS, RLG_LR_MUL, rlg_shapes

NEGATIVE_SLOPE, SCALE = 0.2, 2 ** 0.5      # fused_leaky_relu's defaults (random_latent_generator.py:10)


class RLGConfigC(C.Structure):
	_fields_ = [("channels", C.c_int), ("n_layers", C.c_int), ("max_rows", C.c_int), ("slope", C.c_float), ("gain", C.c_float)]


def infer_channels(state_dict: Mapping[str, torch.Tensor]) -> int:
	w = state_dict.get("layers.0.weight")
	if w is None or w.dim() != 2:
		raise _lib.TTKError("not a RandomLatentConverter state_dict: 'layers.0.weight' [channels, channels] is missing")
	return int(w.shape[0])


def fold_equal_linear(state_dict: Mapping[str, torch.Tensor], channels: Optional[int] = None) -> Dict[str, torch.Tensor]:
	"""The operands the reference's forward multiplies with, f32 on the host: layers 0-4 `weight * ((1 / math.sqrt(in_dim)) * lr_mul)` and
	`bias * lr_mul` (random_latent_generator.py:33, 37-38, lr_mul = .1); layer 5 (nn.Linear) as it is.  Missing keys and weights that are not
	[channels, channels] are refused."""
	channels = channels or infer_channels(state_dict)
	problems = []
	for name, shape in rlg_shapes(channels).items():
		t = state_dict.get(name)
		if t is None:
			problems.append(f"missing {name}")
		elif tuple(t.shape) != shape:
			problems.append(f"{name}: shape {tuple(t.shape)} != expected {shape}" + (" (the layers are square)" if t.dim() == 2 else ""))
	if problems:
		raise _lib.TTKError(f"not a RandomLatentConverter({channels}) state_dict: " + "; ".join(problems[:8]))
	out = {}
	for i in range(RLG_LAYERS):
		weight = state_dict[f"layers.{i}.weight"].detach().to("cpu", torch.float32)
		bias = state_dict[f"layers.{i}.bias"].detach().to("cpu", torch.float32)
		if i < RLG_LAYERS - 1:
			in_dim, lr_mul = weight.shape[1], RLG_LR_MUL
			weight, bias = weight * ((1 / math.sqrt(in_dim)) * lr_mul), bias * lr_mul
		out[f"layers.{i}.weight"], out[f"layers.{i}.bias"] = weight.contiguous(), bias.contiguous()
	return out


class RandomLatentConverter(_lib.Handle):
	"""`RandomLatentConverter(channels)` of the reference with its `state_dict` ("layers.{0..5}.weight|bias")."""

	def __init__(self, state_dict: Mapping[str, torch.Tensor], channels: Optional[int] = None, device: str = "cuda:0", max_rows: int = 16, dtype: str = "f32"):
		if _lib.DTYPES.get(dtype) != _lib.TTK_F32:
			raise _lib.TTKError("the RandomLatentConverter runs in 'f32' only: its output is the input of every later stage")
		if not 1 <= int(max_rows) <= 16:
			raise _lib.TTKError(f"max_rows must be 1..16 (the rows of one launch), got {max_rows}")
		folded = fold_equal_linear(state_dict, channels)
		self.channels, self.max_rows = folded["layers.0.weight"].shape[0], int(max_rows)
		super().__init__(device)
		c = RLGConfigC(self.channels, RLG_LAYERS, self.max_rows, NEGATIVE_SLOPE, SCALE)
		self._create("rlg", c, folded, list(folded))

	@torch.inference_mode()
	def forward(self, ref: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
		"""random_latent_generator.py:49-52: one latent f32 [B, channels] per row of `ref` (only `ref.shape[0]` is read).  Without `noise` the rows are
		`torch.randn(B, channels, device=self.device)` from the default device generator -- the reference's own draw on a GPU, consuming the
		generator alike; a given `noise` [B, channels] is used as it is."""
		B = int(ref.shape[0])
		if noise is None:
			noise = torch.randn(B, self.channels, device=self.device)
		elif noise.dim() != 2 or tuple(noise.shape) != (B, self.channels):
			raise _lib.TTKError(f"noise must be [{B}, {self.channels}], got {tuple(noise.shape)}")
		noise = noise.to(self.device, torch.float32).contiguous()
		out = torch.empty((B, self.channels), device=self.device, dtype=torch.float32)
		with torch.cuda.device(self.device):
			for r0 in range(0, B, self.max_rows):
				rows = min(self.max_rows, B - r0)
				_lib.check(self.lib.ttk_rlg_forward(self._h, noise[r0:].data_ptr(), rows, out[r0:].data_ptr(), _lib.stream_ptr()), "ttk_rlg_forward")
		return out

	__call__ = forward
