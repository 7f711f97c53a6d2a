"""CPU oracle of the TorToiSe detector (models/classifier.py:79-149 over arch_utils.py:24-44, 59-94, 136-190, 220-245): a functional restatement of
`AudioMiniEncoderWithClassifierHead.forward` on the reference's state_dict keys, in f32 or f64, that also returns the activations the fixtures
(tools/make_golden_classifier.py) store: the stem, every stage behind its Downsample, and `enc.final`.  The GPU tests use it where a fixture holds
only every n-th frame of an activation.  A helper, not a test.
"""
import math

import torch
import torch.nn.functional as F

from tortoise_tts_amd.weights import CLASSIFIER_FULL, CLASSIFIER_SMALL, ClassifierConfig

CFGS = {"classifier_small": (CLASSIFIER_SMALL, ("1x1", "1x5", "1x4096", "2x4099", "1x24000")), "classifier_full": (CLASSIFIER_FULL, ("1x5000", "2x66000"))}
SEEDS = {"classifier_small": 131, "classifier_full": 133}      # weight seeds; the input seed of case i of a fixture is 10 * weight seed + i
MAX_STORED = 8000                                              # elements of one stored activation: longer ones keep every `step`-th frame


def fixture_audio(B, T, seed):
	"""the seeded input of the fixtures [B, 1, T]: a 220 Hz tone at 24 kHz plus noise"""
	g = torch.Generator().manual_seed(seed)
	t = torch.arange(T, dtype=torch.float32)
	return (0.3 * torch.sin(2 * math.pi * 220 * t / 24000)[None] + 0.05 * torch.randn(B, T, generator=g))[:, None].contiguous()


def time_step(shape):
	"""the frame step at which an activation [B, C, L] is stored"""
	n = 1
	for s in shape:
		n *= int(s)
	return max(1, -(-n // MAX_STORED))


def groups_of(channels):
	"""arch_utils.py:29-44"""
	g = 32
	if channels <= 16:
		g = 8
	elif channels <= 64:
		g = 16
	while channels % g:
		g //= 2
	return g


def activation_names(cfg: ClassifierConfig):
	return ["stem"] + [f"stage{l}" for l in range(cfg.depth)] + ["final"]


class ClassifierOracle:
	def __init__(self, sd, cfg: ClassifierConfig, dtype=torch.float32):
		self.cfg, self.dtype = cfg, dtype
		self.sd = {k: v.to(dtype) for k, v in sd.items()}

	def _conv(self, x, name, stride=1, padding=0):
		return F.conv1d(x, self.sd[name + ".weight"], self.sd[name + ".bias"], stride=stride, padding=padding)

	def _gn(self, x, name):
		return F.group_norm(x, groups_of(x.shape[1]), self.sd[name + ".weight"], self.sd[name + ".bias"], 1e-5)

	def _res(self, x, p):
		h = self._conv(F.silu(self._gn(x, p + ".in_layers.0")), p + ".in_layers.2", padding=2)
		return x + self._conv(F.silu(self._gn(h, p + ".out_layers.0")), p + ".out_layers.3", padding=2)

	def _attn(self, x, p):
		B, Cn, L = x.shape
		H = self.cfg.num_attn_heads
		ch = Cn // H
		q, k, v = self._conv(self._gn(x, p + ".norm"), p + ".qkv").reshape(B * H, 3 * ch, L).split(ch, dim=1)
		scale = 1 / math.sqrt(math.sqrt(ch))
		w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale), dim=-1)
		a = torch.einsum("bts,bcs->bct", w, v).reshape(B, Cn, L)
		return x + self._conv(a, p + ".proj_out")

	def forward(self, audio):
		"""audio [B, 1, T] -> (emb [B, E], logits [B, classes], {"stem", "stage<l>", "final": activations [B, C, L]})"""
		c = self.cfg
		acts = {}
		h = acts["stem"] = self._conv(audio.to(self.dtype), "enc.init.0", padding=1)
		n = 0
		for l in range(c.depth):
			for _ in range(c.resnet_blocks):
				h = self._res(h, f"enc.res.{n}")
				n += 1
			h = acts[f"stage{l}"] = self._conv(h, f"enc.res.{n}.op", stride=4, padding=2)
			n += 1
		h = acts["final"] = self._conv(F.silu(self._gn(h, "enc.final.0")), "enc.final.2")
		for i in range(c.attn_blocks):
			h = self._attn(h, f"enc.attn.{i}")
		emb = h[:, :, 0]
		return emb, emb @ self.sd["head.weight"].t() + self.sd["head.bias"], acts
