"""The TorToiSe detector on libttk: `AudioMiniEncoderWithClassifierHead` (`models/classifier.py:79-149`), the network behind upstream's
`classify_audio_clip` and its published `classifier.pth`, over `ttk_cls_*` -- raw 24 kHz audio -> embedding -> logits.

The 32- and 64-channel stages, where ~94 % of the rows sit, run on a fused GroupNorm + SiLU + k = 5 convolution kernel with split GroupNorm
statistics; the wider stages and the Downsamples run on the hot path's segment GEMM; the AttentionBlocks are those of the conditioning encoders
(csrc/classifier.hip).  The residual stream and every GroupNorm are f32 in both dtypes; 'bf16' rounds only the operands of the matrix products.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Optional, Tuple

import torch

from . import _lib
from .weights import CLASSIFIER_FULL, ClassifierConfig, classifier_shapes

MAX_POSITIONS = 3584      # kRowWaveMaxT of csrc/ttk_attn_block.h: positions of the last stage at head width 128


class ClassifierConfigC(C.Structure):
	_fields_ = [(n, C.c_int) for n in ("classes", "spec_dim", "embedding_dim", "depth", "downsample_factor", "resnet_blocks", "attn_blocks", "num_attn_heads",
									   "base_channels", "kernel_size", "dtype")]


def check_config(cfg: ClassifierConfig) -> None:
	"""The refusals of `ttk_cls_create`, with the reason, before anything touches the GPU."""
	heads_ok = cfg.num_attn_heads >= 1 and cfg.embedding_dim % max(cfg.num_attn_heads, 1) == 0
	refused = [
		(cfg.spec_dim != 1, f"spec_dim={cfg.spec_dim}: the stem kernel reads one channel of raw audio (spec_dim=1)"),
		(cfg.kernel_size != 5, f"kernel_size={cfg.kernel_size}: the ResBlock convolutions are built for kernel_size=5"),
		(cfg.downsample_factor != 4, f"downsample_factor={cfg.downsample_factor}: the Downsample is built as stride 4 over a four-row view (downsample_factor=4)"),
		(cfg.base_channels != 32, f"base_channels={cfg.base_channels}: the fused convolution is instantiated for the 32- and 64-channel stages of base_channels=32"),
		(not 1 <= cfg.depth <= 6, f"depth={cfg.depth}: 1..6 stages are built"),
		(not heads_ok or cfg.embedding_dim // cfg.num_attn_heads not in (64, 128) or cfg.embedding_dim % 128 != 0,
		 f"num_attn_heads={cfg.num_attn_heads} with embedding_dim={cfg.embedding_dim}: the head width must be 64 or 128 and embedding_dim a multiple of 128"),
		(not 1 <= cfg.classes <= 16, f"classes={cfg.classes}: the head kernel serves 1..16 classes"),
		(cfg.dropout != 0, f"dropout={cfg.dropout}: inference only"),
	]
	for bad, why in refused:
		if bad:
			raise NotImplementedError("AudioMiniEncoderWithClassifierHead: " + why)


class AudioMiniEncoderWithClassifierHead(_lib.Handle):
	"""`AudioMiniEncoderWithClassifierHead(classes, **kwargs)` of the reference with its `state_dict` ("enc.init...", "enc.res.N...", "enc.final...",
	"enc.attn.N...", "head..."), inference side."""

	def __init__(self, state_dict: Mapping[str, torch.Tensor], cfg: ClassifierConfig = CLASSIFIER_FULL, dtype: str = "f32", device: str = "cuda:0"):
		check_config(cfg)
		self.cfg = cfg
		super().__init__(device)
		if _lib.DTYPES.get(dtype) not in (_lib.TTK_F32, _lib.TTK_BF16):
			raise _lib.TTKError("the classifier runs in 'f32' or 'bf16'")
		self.num_classes, self.distribute_zero_label = cfg.classes, cfg.distribute_zero_label
		c = ClassifierConfigC(cfg.classes, cfg.spec_dim, cfg.embedding_dim, cfg.depth, cfg.downsample_factor, cfg.resnet_blocks, cfg.attn_blocks, cfg.num_attn_heads,
							  cfg.base_channels, cfg.kernel_size, _lib.DTYPES[dtype])
		names = [n for n in classifier_shapes(cfg) if n in state_dict]      # ttk_cls_create names a missing tensor
		self._create("cls", c, state_dict, names)

	def _audio(self, x: torch.Tensor) -> torch.Tensor:
		if x.dim() != 3 or x.shape[1] != 1 or x.shape[0] < 1 or x.shape[2] < 1:
			raise _lib.TTKError(f"audio must be [B, 1, T >= 1], got {tuple(x.shape)}")
		return x.to(self.device, torch.float32).contiguous()

	def _run(self, x: torch.Tensor, taps: bool = False):
		x = self._audio(x)
		B, _, T = x.shape
		emb = torch.empty((B, self.cfg.embedding_dim), device=self.device, dtype=torch.float32)
		logits = torch.empty((B, self.cfg.classes), device=self.device, dtype=torch.float32)
		outs: List[torch.Tensor] = []
		with torch.cuda.device(self.device):
			if taps:
				L, ch = self.cfg.stage_lengths(T), self.cfg.base_channels
				shapes = [(B, T, ch)] + [(B, L[l + 1], ch * 2 ** (l + 1)) for l in range(self.cfg.depth)] + [(B, L[-1], self.cfg.embedding_dim)]
				outs = [torch.empty(s, device=self.device, dtype=torch.float32) for s in shapes]
				arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
				_lib.check(self.lib.ttk_cls_forward_taps(self._h, x.data_ptr(), B, T, emb.data_ptr(), logits.data_ptr(), arr, len(outs), _lib.stream_ptr()),
						   "ttk_cls_forward_taps")
			else:
				_lib.check(self.lib.ttk_cls_forward(self._h, x.data_ptr(), B, T, emb.data_ptr(), logits.data_ptr(), _lib.stream_ptr()), "ttk_cls_forward")
		return emb, logits, outs

	@torch.inference_mode()
	def forward(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
		"""classifier.py:132-136: audio f32 [B, 1, T] at 24 kHz -> logits [B, classes]"""
		if labels is not None:
			raise NotImplementedError("AudioMiniEncoderWithClassifierHead.forward(x, labels) is the training loss (cross entropy against the labels, "
									  "classifier.py:137-149); call forward(x) for the logits")
		return self._run(x)[1]

	__call__ = forward

	@torch.inference_mode()
	def encode(self, x: torch.Tensor) -> torch.Tensor:
		"""`self.enc(x)` (classifier.py:115-121): audio [B, 1, T] -> embedding [B, embedding_dim], position 0 behind the AttentionBlocks"""
		return self._run(x)[0]

	@torch.inference_mode()
	def forward_with_intermediates(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
		"""(embedding, logits, [stem, stage 0 .. depth - 1 behind its Downsample, enc.final]) with the intermediates channels-first [B, C, L] like the
		reference's activations: what the tests compare stage by stage."""
		emb, logits, outs = self._run(x, taps=True)
		return emb, logits, [o.transpose(1, 2) for o in outs]


def gn_stats(x: torch.Tensor, groups: int) -> torch.Tensor:
	"""The split GroupNorm statistics alone (`ttk_cls_gn_stats`): x f32 [B, L, C] channels-last on the GPU -> (mean, rstd) f32 [B, groups, 2]"""
	_lib.require_cuda(x)
	lib = _lib.load()
	x = x.to(torch.float32).contiguous()
	B, L, Cn = x.shape
	rows = lib.ttk_cls_stats_rows(Cn)
	n = B * ((L + rows - 1) // rows) * groups * 3
	part = torch.empty(n, device=x.device, dtype=torch.float32)
	out = torch.empty((B, groups, 2), device=x.device, dtype=torch.float32)
	with torch.cuda.device(x.device):
		_lib.check(lib.ttk_cls_gn_stats(x.data_ptr(), B, L, Cn, groups, part.data_ptr(), n, out.data_ptr(), _lib.stream_ptr()), "ttk_cls_gn_stats")
	return out


def conv5_rows(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, stats: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
			   beta: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, dtype: str = "f32") -> torch.Tensor:
	"""The fused ResBlock convolution alone (`ttk_cls_conv5_rows`): x f32 [B, L, C] channels-last (C = 32 | 64), weight [C, C, 5], bias [C]; with `stats`
	[B, groups, 2] the input is silu(groupnorm(x)) with gamma / beta [C], without it x itself.  Returns f32 [B, L, C]."""
	_lib.require_cuda(x, weight, bias, stats, gamma, beta, residual)
	lib = _lib.load()
	f = lambda t: None if t is None else t.to(torch.float32).contiguous()
	x, weight, bias, stats, gamma, beta, residual = (f(t) for t in (x, weight, bias, stats, gamma, beta, residual))
	B, L, Cn = x.shape
	if tuple(weight.shape) != (Cn, Cn, 5) or tuple(bias.shape) != (Cn,) or (residual is not None and residual.shape != x.shape):
		raise _lib.TTKError(f"conv5_rows: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not fit rows {tuple(x.shape)}")
	groups = 0 if stats is None else int(stats.shape[1])
	out = torch.empty_like(x)
	with torch.cuda.device(x.device):
		_lib.check(lib.ttk_cls_conv5_rows(_lib.DTYPES[dtype], x.data_ptr(), B, L, Cn, _lib.ptr(stats), groups, _lib.ptr(gamma), _lib.ptr(beta), weight.data_ptr(),
										  bias.data_ptr(), _lib.ptr(residual), out.data_ptr(), _lib.stream_ptr()), "ttk_cls_conv5_rows")
	return out
