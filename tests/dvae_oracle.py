"""CPU oracle of the DiscreteVAE (models/dvae.py:12-72, 89-114, 116-276 in its default configuration): a functional restatement over the
reference's state_dict keys, in f32 or f64, and the float64 distance bookkeeping of the near-tie criterion the DVAE tests share.

Near ties.  An 8192-way argmin over f32 distances has positions whose best two candidates are closer than the distances' own rounding noise; the
reference resolves those by that noise (it adds |z|^2 to every candidate, so its distances carry the ulp of about |z|^2 + |e|^2).  The fixtures
(tools/make_golden_dvae.py) store per position `gap` -- the float64 margin between the best and the second-best code -- and per input `tau` =
4 x max |dist_f32 - dist_f64| of the reference's own expression.  Codes must agree where gap >= tau; elsewhere the chosen code's float64 distance
must be within tau of the minimum.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tortoise_tts_amd.weights import DVAEConfig


def fixture_mel(B, T, seed, channels=80):
	"""the seeded input of the fixtures: a log-mel-like tensor [B, channels, T] (smooth along time, so neighbouring frames are related as in speech)"""
	g = torch.Generator().manual_seed(seed)
	x = torch.randn(B, channels, T + 4, generator=g)
	x = F.avg_pool1d(x, 5, stride=1) * 2.0 + torch.randn(B, channels, 1, generator=g)
	return (x * 1.5 - 4.0).contiguous()


def fixture_codes(B, n, seed, num_tokens):
	return torch.randint(0, num_tokens, (B, n), generator=torch.Generator().manual_seed(seed))


class DVAEOracle:
	def __init__(self, sd, cfg: DVAEConfig, dtype=torch.float32):
		self.cfg, self.dtype = cfg, dtype
		self.sd = {k: v.to(dtype) for k, v in sd.items()}

	def _conv(self, x, name, stride=1, padding=0):
		return F.conv1d(x, self.sd[name + ".weight"], self.sd[name + ".bias"], stride=stride, padding=padding)

	def _res(self, x, p):
		h = torch.relu(self._conv(x, p + ".net.0", padding=1))
		h = torch.relu(self._conv(h, p + ".net.2", padding=1))
		return self._conv(h, p + ".net.4") + x

	def encode(self, mel):
		"""mel [B, channels, T] -> z [B, T4, codebook_dim]"""
		R = self.cfg.num_resnet_blocks
		x = torch.relu(self._conv(mel.to(self.dtype), "encoder.0.0", 2, 1))
		x = torch.relu(self._conv(x, "encoder.1.0", 2, 1))
		for i in range(R):
			x = self._res(x, f"encoder.{2 + i}")
		return self._conv(x, f"encoder.{2 + R}").transpose(1, 2)

	def codebook(self):
		"""[num_tokens, codebook_dim]"""
		return self.sd["codebook.embed"].t()

	def scores(self, z):
		"""|e_j|^2 - 2 z . e_j: the distance less the row constant, [M, num_tokens]"""
		e = self.codebook()
		z = z.reshape(-1, e.shape[1]).to(self.dtype)
		return e.pow(2).sum(1)[None] - 2 * (z @ e.t())

	def quantize(self, z):
		return self.scores(z).argmin(1).view(z.shape[:-1])

	def get_codebook_indices(self, mel):
		return self.quantize(self.encode(mel))

	def decode(self, codes):
		"""codes [B, n] -> (mel [B, channels, 4 n], hidden [B, hidden_dim, 4 n])"""
		R = self.cfg.num_resnet_blocks
		x = self.codebook()[codes].transpose(1, 2)
		x = self._conv(x, "decoder.0")
		for i in range(R):
			x = self._res(x, f"decoder.{1 + i}")
		for i in (1 + R, 2 + R):
			x = torch.relu(self._conv(x.repeat_interleave(2, dim=2), f"decoder.{i}.0.conv", padding=1))
		return self._conv(x, f"decoder.{3 + R}"), x


def distances64(z, embed):
	"""float64 distances |z - e_j|^2 as the reference's expression in exact-enough arithmetic: z [M, D], embed [D, V] -> [M, V]"""
	z, e = torch.as_tensor(z).double(), torch.as_tensor(embed).double()
	return z.pow(2).sum(1, keepdim=True) - 2 * z @ e + e.pow(2).sum(0, keepdim=True)


def reference_distances32(z, embed):
	"""dvae.py:31-35 evaluated as the reference evaluates it, in f32"""
	z, e = torch.as_tensor(z).float(), torch.as_tensor(embed).float()
	return z.pow(2).sum(1, keepdim=True) - 2 * z @ e + e.pow(2).sum(0, keepdim=True)


def gap_and_tau(z, embed):
	"""(gap [M] float64: second-best minus best float64 distance; tau: 4 x max |dist_f32 - dist_f64| over the reference's own f32 distances)"""
	d64 = distances64(z, embed)
	two = d64.topk(2, dim=1, largest=False).values if d64.shape[1] > 1 else torch.cat([d64, d64 + np.inf], 1)
	tau = 4.0 * (reference_distances32(z, embed).double() - d64).abs().max().item()
	return (two[:, 1] - two[:, 0]), tau


def check_codes(codes, ref_codes, z, embed, gap, tau):
	"""The near-tie criterion.  codes / ref_codes [M]; z [M, D] the f32 rows both were taken from.  Returns (mismatches where gap >= tau, worst excess
	float64 distance over the minimum among the rest, share of positions with gap < tau)."""
	codes, ref_codes, gap = torch.as_tensor(codes).reshape(-1), torch.as_tensor(ref_codes).reshape(-1), torch.as_tensor(gap).reshape(-1)
	clear = gap >= tau
	wrong = int((codes[clear] != ref_codes[clear]).sum())
	d64 = distances64(z, embed)
	excess = (d64.gather(1, codes.reshape(-1, 1).long()).squeeze(1) - d64.min(1).values)[~clear]
	return wrong, (excess.max().item() if excess.numel() else 0.0), float((~clear).double().mean())
