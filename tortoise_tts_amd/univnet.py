"""UnivNet vocoder on libttk: the reference's `vocoder.inference(mels)` for `vocoder_type="vocoder"` (`inference.py:417`,
`models/vocoder.py:302-314`) over `ttk_univnet_*`.  Every convolution runs on the hot path's segment GEMM; the location-variable
convolution and its gated update are one kernel of csrc/univnet.hip.

The noise z is the only host-side draw: when the caller passes none, it is `torch.randn(B, noise_dim, T + 10)` from the CPU default
generator, as the reference draws it (:309), copied to the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional

import torch

from . import _lib
from .vocoder import Vocoder
from .weights import UnivNetConfig, univnet_shapes

MEL_PAD_FRAMES = 10          # inference :305-306


class UnivNetConfigC(C.Structure):
	_fields_ = [("num_mels", C.c_int), ("noise_dim", C.c_int), ("channels", C.c_int), ("n_blocks", C.c_int), ("strides", C.c_int * 4),
				("n_layers", C.c_int), ("dilations", C.c_int * 4), ("kpnet_hidden", C.c_int), ("kpnet_conv_size", C.c_int),
				("conv_kernel_size", C.c_int), ("hop_length", C.c_int), ("dtype", C.c_int)]


def config_c(cfg: UnivNetConfig, dtype: str) -> UnivNetConfigC:
	if len(cfg.strides) > 4 or len(cfg.dilations) > 4:
		raise _lib.TTKError(f"UnivNet with {len(cfg.strides)} blocks / {len(cfg.dilations)} dilations is unsupported (at most 4 each)")
	if cfg.lrelu_slope != 0.2:
		raise _lib.TTKError(f"LeakyReLU slope {cfg.lrelu_slope} is unsupported (0.2)")
	c = UnivNetConfigC()
	c.num_mels, c.noise_dim, c.channels = cfg.num_mels, cfg.noise_dim, cfg.channel_size
	c.n_blocks, c.n_layers = len(cfg.strides), len(cfg.dilations)
	for i, s in enumerate(cfg.strides):
		c.strides[i] = s
	for i, d in enumerate(cfg.dilations):
		c.dilations[i] = d
	c.kpnet_hidden, c.kpnet_conv_size, c.conv_kernel_size, c.hop_length = cfg.kpnet_hidden, cfg.kpnet_conv_size, cfg.conv_kernel_size, cfg.hop_length
	c.dtype = _lib.DTYPES[dtype]
	return c


class UnivNet(Vocoder):
	"""`vocoder = load_model("vocoder")` of the reference (UnivNetGenerator, inference side only)."""
	_abi, _lacks, _config_c, _shapes = "univnet", "UnivNet", staticmethod(config_c), staticmethod(univnet_shapes)

	def __init__(self, state_dict: Mapping[str, torch.Tensor], cfg: UnivNetConfig = UnivNetConfig(), dtype: str = "bf16", device: str = "cuda:0"):
		super().__init__(state_dict, cfg, dtype, device)
		self.hop_length = cfg.hop_length
		self.mel_channel = cfg.num_mels
		self.noise_dim = cfg.noise_dim

	def draw_noise(self, B: int, T: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
		"""The z of inference :309 for a [B, num_mels, T] mel: [B, noise_dim, T + 10] from `generator` (default: the CPU default generator)."""
		return torch.randn(B, self.noise_dim, T + MEL_PAD_FRAMES, generator=generator)

	@torch.inference_mode()
	def inference(self, c: torch.Tensor, z: Optional[torch.Tensor] = None) -> torch.Tensor:
		"""vocoder.py:302-314: c [B, num_mels, T] log-mel (+ z [B, noise_dim, T + 10]) -> audio [B, 1, T * hop_length] in [-1, 1]."""
		if c.dim() != 3 or c.shape[1] != self.cfg.num_mels:
			raise _lib.TTKError(f"mel must be [B, {self.cfg.num_mels}, T], got {tuple(c.shape)}")
		B, _, T = c.shape
		if z is None:
			z = self.draw_noise(B, T)
		if tuple(z.shape) != (B, self.noise_dim, T + MEL_PAD_FRAMES):
			raise _lib.TTKError(f"z must be [{B}, {self.noise_dim}, {T + MEL_PAD_FRAMES}], got {tuple(z.shape)}")
		c = c.to(self.device, torch.float32).contiguous()
		z = z.to(self.device, torch.float32).contiguous()
		audio = torch.empty((B, 1, T * self.hop_length), device=self.device, dtype=torch.float32)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_univnet_inference(self._h, c.data_ptr(), z.data_ptr(), B, T, audio.data_ptr(), _lib.stream_ptr()),
					   "ttk_univnet_inference")
		return audio
