"""CPU oracle of the UnivNet generator (models/vocoder.py:9-314), written from the equations rather than the reference's module code:
plain weights (weight norm folded), channels-first [B, C, L] tensors, any float dtype.  The location-variable convolution is a
per-segment contraction over a zero-padded copy of the sequence:

    o[b, n, l h + t] = bias[b, n, l] + sum_i sum_k y_pad[b, i, l h + t + k] * kern[b, i, n, k, l]      (y_pad: one zero row each side)
"""
import torch
import torch.nn.functional as F

from tortoise_tts_amd.weights import UnivNetConfig

SLOPE = 0.2
MEL_PAD_FRAMES, MEL_PAD_VALUE = 10, -11.5129


def fixture_inputs(B, T, mel_seed, z_seed, cfg: UnivNetConfig = UnivNetConfig()):
	"""the seeded mel [B, mels, T] (2 randn - 5) and z [B, noise, T + 10] of the fixtures (tools/make_golden_univnet.py draws them here)"""
	mel = torch.randn(B, cfg.num_mels, T, generator=torch.Generator().manual_seed(mel_seed)) * 2 - 5
	z = torch.randn(B, cfg.noise_dim, T + MEL_PAD_FRAMES, generator=torch.Generator().manual_seed(z_seed))
	return mel, z


def lrelu(x):
	return F.leaky_relu(x, SLOPE)


class UnivNetOracle:
	def __init__(self, sd, cfg: UnivNetConfig, dtype=torch.float32):
		self.cfg, self.dtype = cfg, dtype
		self.w = {k: v.detach().to(dtype) for k, v in sd.items()}
		self.trace = {}

	def conv(self, x, name, pad=0, dilation=1, mode="zeros"):
		if mode == "reflect":
			x, pad = F.pad(x, (pad, pad), mode="reflect"), 0
		return F.conv1d(x, self.w[name + ".weight"], self.w[name + ".bias"], padding=pad, dilation=dilation)

	def kernel_predictor(self, c, p):
		"""[B, mels, T] -> kernels [B, layers, C, 2C, 3, T], bias [B, layers, 2C, T]"""
		cfg = self.cfg
		kp, pad = p + "kernel_predictor.", (cfg.kpnet_conv_size - 1) // 2
		h = lrelu(self.conv(c, kp + "input_conv.0", 2))
		for j in range(3):
			r = lrelu(self.conv(h, kp + f"residual_convs.{j}.1", pad))
			h = h + lrelu(self.conv(r, kp + f"residual_convs.{j}.3", pad))
		B, T, C, nl = c.shape[0], c.shape[-1], cfg.channel_size, len(cfg.dilations)
		k = self.conv(h, kp + "kernel_conv", pad).reshape(B, nl, C, 2 * C, cfg.conv_kernel_size, T)
		b = self.conv(h, kp + "bias_conv", pad).reshape(B, nl, 2 * C, T)
		return k, b

	@staticmethod
	def lvc(y, kern, bias, hop):
		"""y [B, C, T h], kern [B, C, 2C, 3, T], bias [B, 2C, T] -> [B, 2C, T h]"""
		B, C, L = y.shape
		T = kern.shape[-1]
		assert L == T * hop
		ypad = F.pad(y, (1, 1))
		out = torch.empty(B, kern.shape[2], L, dtype=y.dtype)
		for l in range(T):
			win = ypad[:, :, l * hop:l * hop + hop + 2]                               # [B, C, h + 2]
			taps = torch.stack([win[:, :, k:k + hop] for k in range(kern.shape[3])], dim=-1)   # [B, C, h, 3]
			out[:, :, l * hop:(l + 1) * hop] = torch.einsum("bitk,biok->bot", taps, kern[..., l]) + bias[:, :, l, None]
		return out

	def block(self, x, c, i):
		cfg = self.cfg
		p, s, C = f"res_stack.{i}.", cfg.strides[i], cfg.channel_size
		x = F.conv_transpose1d(lrelu(x), self.w[p + "convt_pre.1.weight"], self.w[p + "convt_pre.1.bias"], stride=s,
							   padding=s // 2 + s % 2, output_padding=s % 2)
		kern, bias = self.kernel_predictor(c, p)
		if i == 0:
			self.trace.update(convt_pre=x, kernels=kern, bias=bias)
		for n, d in enumerate(cfg.dilations):
			y = lrelu(self.conv(lrelu(x), p + f"conv_blocks.{n}.1", d, d))
			o = self.lvc(y, kern[:, n], bias[:, n], cfg.cond_hops()[i])
			if i == 0 and n == 0:
				self.trace["lvc0"] = o
			x = x + torch.sigmoid(o[:, :C]) * torch.tanh(o[:, C:])
		return x

	def forward(self, c, z):
		c, z = c.to(self.dtype), z.to(self.dtype)
		x = self.conv(z, "conv_pre", 3, mode="reflect")
		for i in range(len(self.cfg.strides)):
			x = self.block(x, c, i)
		return torch.tanh(self.conv(lrelu(x), "conv_post.1", 3, mode="reflect"))

	def inference(self, c, z):
		"""c [B, mels, T], z [B, noise, T + 10] -> [B, 1, T hop]"""
		mel = torch.cat([c.to(self.dtype), torch.full((c.shape[0], c.shape[1], MEL_PAD_FRAMES), MEL_PAD_VALUE, dtype=self.dtype)], dim=2)
		audio = self.forward(mel, z)
		return audio[:, :, :-(self.cfg.hop_length * MEL_PAD_FRAMES)].clamp(-1, 1)
