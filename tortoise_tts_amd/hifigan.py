"""HiFiGAN vocoder on libttk: the reference's `vocoder.inference(latents, autoregressive_latents)` for `vocoder_type="hifigan"`
(`inference.py:297`, `models/hifigan.py:270-296`) over `ttk_hifigan_*`, and the streaming loop the reference keeps inline in
`TTS.inference` (`inference.py:250-329`) as a generator, `HiFiGAN.stream`.

This branch skips the diffusion model: the generator is conditioned on the AR model's `final_norm` latents, one per mel token, as they
leave the token loop.  conv_pre, the transposed convolutions and the wide ResBlock stages run on the hot path's segment GEMM; the
interpolation, the narrow-channel (C <= 64) ResBlock convolution on the MFMA and conv_post are kernels of csrc/hifigan.hip.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Iterator, Mapping, Tuple

import torch

from . import _lib
from .vocoder import Vocoder
from .weights import HiFiGANConfig, hifigan_shapes


class HiFiGANConfigC(C.Structure):
	_fields_ = [("in_channels", C.c_int), ("cond_channels", C.c_int), ("upsample_initial_channel", C.c_int), ("n_ups", C.c_int),
				("up_rate", C.c_int * 8), ("up_kernel", C.c_int * 8), ("n_kernels", C.c_int), ("rb_kernel", C.c_int * 4),
				("rb_dil", (C.c_int * 3) * 4), ("resblock_type", C.c_int), ("dtype", C.c_int)]


def config_c(cfg: HiFiGANConfig, dtype: str) -> HiFiGANConfigC:
	if len(cfg.upsample_factors) != len(cfg.upsample_kernel_sizes) or len(cfg.upsample_factors) > 8:
		raise _lib.TTKError(f"HiFiGAN with {len(cfg.upsample_factors)} upsamplers / {len(cfg.upsample_kernel_sizes)} kernel sizes is unsupported (equal, at most 8)")
	if len(cfg.resblock_kernel_sizes) != len(cfg.resblock_dilation_sizes) or len(cfg.resblock_kernel_sizes) > 4:
		raise _lib.TTKError(f"HiFiGAN with {len(cfg.resblock_kernel_sizes)} resblock kernels is unsupported (at most 4, one dilation list each)")
	if str(cfg.resblock_type) not in ("1", "2"):
		raise _lib.TTKError(f"resblock_type {cfg.resblock_type!r} is unknown")
	c = HiFiGANConfigC()
	c.in_channels, c.cond_channels, c.upsample_initial_channel = cfg.in_channels, cfg.cond_channels, cfg.upsample_initial_channel
	c.n_ups, c.n_kernels, c.resblock_type = len(cfg.upsample_factors), len(cfg.resblock_kernel_sizes), int(cfg.resblock_type)
	for i, (u, k) in enumerate(zip(cfg.upsample_factors, cfg.upsample_kernel_sizes)):
		c.up_rate[i], c.up_kernel[i] = u, k
	for j, (k, ds) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
		if c.resblock_type == 1 and len(ds) != 3:
			raise _lib.TTKError(f"ResBlock1 takes three dilations, got {tuple(ds)}")
		c.rb_kernel[j] = k
		for m, d in enumerate(ds[:3]):
			c.rb_dil[j][m] = d
	c.dtype = _lib.DTYPES[dtype]
	return c


class HiFiGAN(Vocoder):
	"""`vocoder = load_model("hifigan")` of the reference (HifiganGenerator, inference side only).  A tensor the state dict lacks is
	named by `ttk_hifigan_create`.  (The weight-norm fold of a ConvTranspose1d: dimension 0 is the input channel, and weight_norm's
	dim=0 norms over the others there too.)"""
	_abi, _config_c, _shapes = "hifigan", staticmethod(config_c), staticmethod(hifigan_shapes)

	def __init__(self, state_dict: Mapping[str, torch.Tensor], cfg: HiFiGANConfig = HiFiGANConfig(), dtype: str = "bf16", device: str = "cuda:0"):
		super().__init__(state_dict, cfg, dtype, device)
		self.hop_length = cfg.hop_length

	def samples(self, n: int) -> int:
		"""samples `inference` returns for n latents"""
		return self.cfg.frames(n) * self.hop_length

	@torch.inference_mode()
	def inference(self, c: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
		"""hifigan.py:270-296: c [1, n, in_channels] latents, g [1, cond_channels] the AR conditioning latent -> audio [1, 1, hop * F],
		F = floor(4 n * 24000 / 22050) frames (the two linear interpolations)."""
		if c.dim() != 3 or c.shape[0] != 1 or c.shape[1] < 1 or c.shape[2] != self.cfg.in_channels:
			raise _lib.TTKError(f"latents must be [1, n >= 1, {self.cfg.in_channels}], got {tuple(c.shape)}")
		if g.numel() != self.cfg.cond_channels:
			raise _lib.TTKError(f"g must be [1, {self.cfg.cond_channels}], got {tuple(g.shape)}")
		n = c.shape[1]
		c = c.to(self.device, torch.float32).contiguous()
		g = g.to(self.device, torch.float32).contiguous()
		audio = torch.empty((1, 1, self.samples(n)), device=self.device, dtype=torch.float32)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_hifigan_set_cond(self._h, g.data_ptr(), _lib.stream_ptr()), "ttk_hifigan_set_cond")
			_lib.check(self.lib.ttk_hifigan_inference(self._h, c.data_ptr(), n, audio.data_ptr(), _lib.stream_ptr()), "ttk_hifigan_inference")
		return audio

	@torch.inference_mode()
	def stream(self, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], g: torch.Tensor, first_buffer: int = 60, chunk: int = 40,
			   overlap: int = 1024) -> Iterator[torch.Tensor]:
		"""The streaming loop of inference.py:250-329 over the `(codes, latent [1, in_channels])` pairs of `UnifiedVoice.get_generator`, as a
		generator of waveform chunks [1, samples] (the reference's commented-out `yield wav_chunk`, :313-316).

		Pairs are collected until `max(chunk, first_buffer)` of them are new (`first_buffer` counts for the first chunk only) or the iterator is
		exhausted (:291); then the vocoder runs on ALL latents so far (:296-297), and the chunk is `wav[prev_len - overlap : -overlap]` (the first:
		`wav[:-overlap]`, :300-302), its first `overlap` samples cross-faded with the last `overlap` samples of the previous call's waveform
		(`linspace(0, 1)` / `linspace(1, 0)`, :303-307).  The last `overlap` samples of the final call are never emitted.

		One departure: when the iterator ends exactly where a chunk has just been emitted (60, 100, 140, ... pairs) the reference runs the vocoder
		again on the same latents, gets an empty chunk and fails in the cross-fade with a shape error.  Here that call is skipped and nothing more
		is emitted."""
		latents, new, prev_len, wav_overlap = [], 0, None, None
		it = iter(pairs)
		is_end = False
		while not is_end:
			try:
				_, latent = next(it)
				latents.append(latent.reshape(1, -1))
				new += 1
			except StopIteration:
				is_end = True
			if not (is_end or (chunk > 0 and new >= max(chunk, first_buffer))):
				continue
			if not latents or (is_end and new == 0 and prev_len is not None):
				break
			first_buffer, new = 0, 0
			wav = self.inference(torch.cat(latents, dim=0)[None], g).reshape(-1)
			piece = (wav[:-overlap] if prev_len is None else wav[prev_len - overlap:-overlap]).clone()
			if wav_overlap is not None:
				up = torch.linspace(0.0, 1.0, overlap, device=wav.device)
				down = torch.linspace(1.0, 0.0, overlap, device=wav.device)
				piece[:overlap] = wav_overlap * down + piece[:overlap] * up
			wav_overlap, prev_len = wav[-overlap:], wav.shape[0]
			yield piece[None]
