"""CPU oracle of the HiFiGAN generator (models/hifigan.py:17-98, 161-296) and of the streaming loop around it (inference.py:250-329),
written from the equations rather than the reference's module code: plain weights (weight norm folded), channels-first tensors, any
float dtype.

The two interpolations of `inference` (:285-294) are written out: `F.interpolate(x, scale_factor=[s], mode="linear")` has output
length floor(len * s) (double arithmetic) and, with align_corners=False and a given scale factor, reads

    src = max((i + 0.5) * (1 / s) - 0.5, 0),  i0 = floor(src),  i1 = min(i0 + 1, len - 1),  out[i] = (1 - (src - i0)) x[i0] + (src - i0) x[i1]

-- the scale factor itself, not len_in / len_out -- and copies when the output length equals the input length (the second stage for
n = 1, 2 latents).
"""
import math

import torch
import torch.nn.functional as F

from tortoise_tts_amd.weights import HiFiGANConfig

SLOPE = 0.1                      # LRELU_SLOPE, hifigan.py:10
SCALES = (1024 / 256, 24000 / 22050)


def fixture_inputs(n, seed, cfg: HiFiGANConfig = HiFiGANConfig()):
	"""the seeded latents [1, n, in_channels] and conditioning latent g [1, cond_channels] of the fixtures (tools/make_golden_hifigan.py draws them here)"""
	gen = torch.Generator().manual_seed(seed)
	return torch.randn(1, n, cfg.in_channels, generator=gen), torch.randn(1, cfg.cond_channels, generator=gen)


def interp_linear(x, scale):
	"""x [B, C, L] -> [B, C, floor(L * scale)], see the module docstring"""
	L = x.shape[-1]
	out_len = int(math.floor(float(L) * scale))
	if out_len == L:
		return x.clone()
	i = torch.arange(out_len, dtype=x.dtype)
	src = (torch.tensor(1.0 / scale, dtype=x.dtype) * (i + 0.5) - 0.5).clamp(min=0)      # ATen multiplies by 1 / scale rounded to the tensor's type
	i0 = src.floor().long().clamp(max=L - 1)
	i1 = (i0 + 1).clamp(max=L - 1)
	l1 = src - i0.to(x.dtype)
	return x[..., i0] * (1 - l1) + x[..., i1] * l1


def stream_plan(n_pairs, first_buffer=60, chunk=40):
	"""latent counts at which the loop of inference.py:283-318 runs the vocoder when the token generator yields n_pairs pairs.  The call the
	reference would make on unchanged latents when the generator ends exactly on a boundary (it fails there) is left out."""
	calls, new, total = [], 0, 0
	while True:
		end = total == n_pairs
		if not end:
			total += 1
			new += 1
		if end or (chunk > 0 and new >= max(chunk, first_buffer)):
			if total and not (end and new == 0 and calls):
				calls.append(total)
			first_buffer, new = 0, 0
		if end:
			return calls


def stream_chunks(wavs, overlap=1024):
	"""inference.py:300-310 on the successive full waveforms [samples] of the vocoder calls: the emitted chunks"""
	out, prev_len, wav_overlap = [], None, None
	for wav in wavs:
		wav = wav.reshape(-1).clone()
		piece = wav[:-overlap] if prev_len is None else wav[prev_len - overlap:-overlap]          # :300-302
		if wav_overlap is not None:                                                                # :303-307
			cross = piece[:overlap] * torch.linspace(0.0, 1.0, overlap, dtype=wav.dtype)
			piece[:overlap] = wav_overlap * torch.linspace(1.0, 0.0, overlap, dtype=wav.dtype)
			piece[:overlap] += cross
		wav_overlap, prev_len = wav[-overlap:].clone(), wav.shape[0]                               # :309-310
		out.append(piece.clone())
	return out


class HiFiGANOracle:
	"""round: None, or a function applied to every convolution's weight and input (e.g. rounding to bf16) -- the model of a 16-bit operand path
	with f32 accumulation, used to set the bf16 tests' bounds"""

	def __init__(self, sd, cfg: HiFiGANConfig, dtype=torch.float32, round=None):
		self.cfg, self.dtype, self.round = cfg, dtype, round
		self.w = {k: v.detach().to(dtype) for k, v in sd.items()}
		self.trace = {}

	def _r(self, t):
		return t if self.round is None else self.round(t)

	def conv(self, x, name, dilation=1):
		w = self.w[name + ".weight"]
		return F.conv1d(self._r(x), self._r(w), self.w[name + ".bias"], padding=(w.shape[-1] - 1) // 2 * dilation, dilation=dilation)

	def resblock(self, x, p, dilations):
		for m, d in enumerate(dilations):                    # ResBlock1.forward :92-97
			xt = self.conv(F.leaky_relu(x, SLOPE), p + f"convs1.{m}", d)
			xt = self.conv(F.leaky_relu(xt, SLOPE), p + f"convs2.{m}", 1)
			x = xt + x
		return x

	def forward(self, x, g):
		"""x [B, in, F], g [B, cond, 1] -> [B, 1, hop F]   (forward :252-268)"""
		cfg = self.cfg
		o = self.conv(x, "conv_pre") + F.conv1d(g, self.w["cond_layer.weight"], self.w["cond_layer.bias"])
		self.trace["conv_pre"] = o
		nk = len(cfg.resblock_kernel_sizes)
		for i, (u, k) in enumerate(zip(cfg.upsample_factors, cfg.upsample_kernel_sizes)):
			o = F.conv_transpose1d(self._r(F.leaky_relu(o, SLOPE)), self._r(self.w[f"ups.{i}.weight"]), self.w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
			if i == 0:
				self.trace["ups0"] = o
			z = None
			for j in range(nk):
				r = self.resblock(o, f"resblocks.{i * nk + j}.", cfg.resblock_dilation_sizes[j])
				z = r if z is None else z + r
			o = z / nk
			if i == 0:
				self.trace["stage0"] = o
		o = F.leaky_relu(o)                                    # default slope 0.01, :265
		w = self.w["conv_post.weight"]
		return torch.tanh(F.conv1d(o, w, self.w["conv_post.bias"], padding=3))

	def inference(self, c, g):
		"""c [1, n, in] latents, g [1, cond] -> [1, 1, hop F]   (inference :285-296)"""
		x = c.to(self.dtype).transpose(1, 2)
		for s in SCALES:
			x = interp_linear(x, s)
		self.trace["interp"] = x
		return self.forward(x, g.to(self.dtype).unsqueeze(0).transpose(1, 2))
