"""DiscreteVAE on libttk: the reference's `dvae = load_model("dvae")` (`models/dvae.py:116-219`, `models/__init__.py`) over `ttk_dvae_*` --
`get_codebook_indices` (mel -> mel codes, what `emb/mel.py:95` calls on a clip), `decode` (mel codes -> mel) and `infer`.

The encoder and decoder convolutions run on the hot path's segment GEMM in the handle's dtype; the quantizer, a fused distance + argmin kernel on
the f32 MFMA (csrc/dvae.hip), runs in f32 whatever the dtype: codes are ids.  The default dtype is f32 for the same reason.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Tuple

import torch

from . import _lib
from .weights import DVAE_FULL, DVAEConfig, dvae_shapes

QUANT_CODES_PER_WORKGROUP = 64      # kQuantCodes of csrc/dvae.hip: the code range one workgroup of the quantizer folds (tests place rows in each)


class DVAEConfigC(C.Structure):
	_fields_ = [(n, C.c_int) for n in ("channels", "hidden_dim", "codebook_dim", "num_tokens", "num_resnet_blocks", "dtype")]


def check_config(cfg: DVAEConfig) -> None:
	"""Only the default structure of models/dvae.py:117-137 is built; everything else is refused with the reason."""
	refused = [
		(cfg.positional_dims != 1, "positional_dims=2 (the image DVAE): the kernels are 1-D convolutions over mel frames"),
		(cfg.use_lr_quantizer, "use_lr_quantizer: needs vector_quantize_pytorch's VectorQuantize, which no published dvae.pth uses"),
		(cfg.encoder_norm, "encoder_norm: the GroupNorm(8) between the encoder layers is not built (dvae.pth has none)"),
		(cfg.use_transposed_convs, "use_transposed_convs: the decoder is built as nearest x2 + conv, the form dvae.pth was trained with"),
		(cfg.activation != "relu", f"activation={cfg.activation!r}: only 'relu' is built"),
		(cfg.normalization is not None, "normalization: the per-channel input normalisation is not built (the mel DVAE has none)"),
		(cfg.record_codes, "record_codes: a training-time histogram of the codes"),
		(cfg.num_layers != 2 or cfg.stride != 2 or cfg.kernel_size != 3, "only num_layers=2, stride=2, kernel_size=3 (the mel DVAE's 4x compression) is built"),
		(cfg.num_resnet_blocks < 1, "num_resnet_blocks=0: the reference then builds a different decoder (no 1x1 conv behind the codebook)"),
	]
	for bad, why in refused:
		if bad:
			raise NotImplementedError("DiscreteVAE: " + why)


class DiscreteVAE(_lib.Handle):
	"""`DiscreteVAE()` of the reference with its `state_dict` ("encoder.N...", "decoder.N...", "codebook.embed"), inference side."""

	def __init__(self, state_dict: Mapping[str, torch.Tensor], cfg: DVAEConfig = DVAE_FULL, dtype: str = "f32", device: str = "cuda:0"):
		check_config(cfg)
		self.cfg = cfg
		super().__init__(device)
		if _lib.DTYPES.get(dtype) not in (_lib.TTK_F32, _lib.TTK_BF16, _lib.TTK_F16):
			raise _lib.TTKError("the DiscreteVAE runs in 'f32', 'bf16' or 'f16'")
		self.num_tokens, self.num_layers, self.positional_dims = cfg.num_tokens, cfg.num_layers, cfg.positional_dims
		c = DVAEConfigC(cfg.channels, cfg.hidden_dim, cfg.codebook_dim, cfg.num_tokens, cfg.num_resnet_blocks, _lib.DTYPES[dtype])
		names = [n for n in dvae_shapes(cfg) if n in state_dict]      # ttk_dvae_create names a missing tensor
		self._create("dvae", c, state_dict, names)

	def forward(self, *a, **k):
		raise NotImplementedError("DiscreteVAE.forward is the training pass (reconstruction and commitment losses, EMA codebook update); "
								  "use get_codebook_indices / decode / infer")

	__call__ = forward

	def _mel(self, mel: torch.Tensor) -> torch.Tensor:
		if mel.dim() != 3 or mel.shape[1] != self.cfg.channels or mel.shape[0] < 1 or mel.shape[2] < 1:
			raise _lib.TTKError(f"mel must be [B, {self.cfg.channels}, T >= 1], got {tuple(mel.shape)}")
		return mel.to(self.device, torch.float32).contiguous()

	@torch.inference_mode()
	def encode(self, mel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
		"""mel [B, channels, T] -> (codes int64 [B, T4], z f32 [B, T4, codebook_dim]: the encoder output the codes were taken from)"""
		mel = self._mel(mel)
		B, _, T = mel.shape
		T4 = self.cfg.code_frames(T)
		codes = torch.empty((B, T4), device=self.device, dtype=torch.int64)
		z = torch.empty((B, T4, self.cfg.codebook_dim), device=self.device, dtype=torch.float32)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_dvae_encode(self._h, mel.data_ptr(), B, T, codes.data_ptr(), z.data_ptr(), _lib.stream_ptr()), "ttk_dvae_encode")
		return codes, z

	@torch.inference_mode()
	def get_codebook_indices(self, mel: torch.Tensor) -> torch.Tensor:
		"""dvae.py:239-246: mel [B, channels, T] -> codes int64 [B, T4]"""
		mel = self._mel(mel)
		B, _, T = mel.shape
		codes = torch.empty((B, self.cfg.code_frames(T)), device=self.device, dtype=torch.int64)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_dvae_encode(self._h, mel.data_ptr(), B, T, codes.data_ptr(), None, _lib.stream_ptr()), "ttk_dvae_encode")
		return codes

	@torch.inference_mode()
	def quantize(self, z: torch.Tensor) -> torch.Tensor:
		"""`Quantize.forward`'s index alone (dvae.py:29-39): z [..., codebook_dim] f32 -> codes int64 [...]"""
		if z.dim() < 1 or z.shape[-1] != self.cfg.codebook_dim or z.numel() == 0:
			raise _lib.TTKError(f"z must be [..., {self.cfg.codebook_dim}] and not empty, got {tuple(z.shape)}")
		z = z.to(self.device, torch.float32).contiguous()
		M = z.numel() // self.cfg.codebook_dim
		codes = torch.empty(z.shape[:-1], device=self.device, dtype=torch.int64)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_dvae_quantize(self._h, z.data_ptr(), M, codes.data_ptr(), _lib.stream_ptr()), "ttk_dvae_quantize")
		return codes

	@torch.inference_mode()
	def decode(self, codes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
		"""dvae.py:248-270: codes int64 [B, n] -> (mel [B, channels, 4 n], the last hidden activation [B, hidden_dim, 4 n]).  A code outside
		[0, num_tokens) raises TTKError before anything is launched."""
		if codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] < 1 or codes.dtype not in (torch.int64, torch.int32):
			raise _lib.TTKError(f"codes must be an integer tensor [B, n >= 1], got {tuple(codes.shape)} {codes.dtype}")
		codes = codes.to(self.device, torch.int64).contiguous()
		B, n = codes.shape
		mel = torch.empty((B, self.cfg.channels, 4 * n), device=self.device, dtype=torch.float32)
		hidden = torch.empty((B, self.cfg.hidden_dim, 4 * n), device=self.device, dtype=torch.float32)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_dvae_decode(self._h, codes.data_ptr(), B, n, mel.data_ptr(), hidden.data_ptr(), _lib.stream_ptr()), "ttk_dvae_decode")
		return mel, hidden

	def infer(self, mel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
		"""dvae.py:272-276"""
		return self.decode(self.get_codebook_indices(mel))
