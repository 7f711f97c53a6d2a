"""Drop-in for the reference's diffusion module object and its diffuser:
`DiffusionTTS` (timestep_independent / forward) and `get_diffuser(...).sample_loop(...)`
(/root/reference/tortoise_tts/models/diffusion.py:1389-1590, 188-810, 1110-1267), as `TTS.inference` calls them
(tortoise_tts/inference.py:183, 402-412), backed by libttk (HIP, gfx950).  No torch fallback exists.

Host logic kept here (it is host logic in the reference too): the float64 beta/alpha tables of the spaced schedule,
the timestep map, the per-step scalar coefficients, the ramped conditioning-free weight -- all numpy float64, converted to
f32 scalars exactly where the reference converts (`_extract_into_tensor(...).float()`, diffusion.py:1264).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .weights import DiffusionConfig, diffusion_code_shapes, diffusion_shapes

TACOTRON_MEL_MAX = 2.3143386840820312
TACOTRON_MEL_MIN = -11.512925148010254


def denormalize_tacotron_mel(norm_mel):
	"""/root/reference/tortoise_tts/models/arch_utils.py:532-537 (a17)."""
	return ((norm_mel + 1) / 2) * (TACOTRON_MEL_MAX - TACOTRON_MEL_MIN) + TACOTRON_MEL_MIN


# ------------------------------------------------------------------------------------------------ derived tables
def _relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 64) -> torch.Tensor:
	"""T5 bucket of rel = k - q, bidirectional (xtransformers.py:157-177 with causal=False, arch_utils.py:174)."""
	n = -rel
	nb = num_buckets // 2
	ret = (n < 0).long() * nb
	n = torch.abs(n)
	max_exact = nb // 2
	is_small = n < max_exact
	val = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
	val = torch.min(val, torch.full_like(val, nb - 1))
	return ret + torch.where(is_small, n, val)


def relbias_table(emb: torch.Tensor, head_dim: int) -> torch.Tensor:
	"""[H, 129] additive attention bias for clamp(k - q, -64, 64): the bucket is constant beyond +-64 (it saturates at
	max_distance), so this table reproduces `RelativePositionBias.forward` (xtransformers.py:179-188) for any length."""
	rel = torch.arange(-64, 65)
	assert int(_relative_position_bucket(torch.tensor([-64]))) == int(_relative_position_bucket(torch.tensor([-100000])))
	assert int(_relative_position_bucket(torch.tensor([64]))) == int(_relative_position_bucket(torch.tensor([100000])))
	return (emb.float().cpu()[_relative_position_bucket(rel)] * (head_dim ** 0.5)).t().contiguous()


def time_freqs(dim: int, max_period: int = 10000) -> torch.Tensor:
	"""diffusion.py:1287-1290."""
	half = dim // 2
	return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


def nearest_index(M: int, T: int) -> torch.Tensor:
	"""Source row of each output frame for F.interpolate(..., size=T, mode='nearest') (diffusion.py:1507):
	floor(dst * scale) with the f32 scale = M / T, clamped (ATen nearest_neighbor_compute_source_index)."""
	scale = np.float32(M) / np.float32(T)
	idx = np.floor(np.arange(T, dtype=np.float32) * scale).astype(np.int64)
	return torch.from_numpy(np.minimum(idx, M - 1).astype(np.int32))


def pack_state_dict(sd: Dict[str, torch.Tensor], cfg: DiffusionConfig, codes: bool = False) -> Dict[str, torch.Tensor]:
	"""Reference-layout tensors + the derived host tables ttk_diff_create expects (include/ttk.h).  codes: the token-conditioning tensors as well."""
	out = {k: sd[k] for k in diffusion_shapes(cfg)}
	if codes:
		out.update({k: sd[k] for k in diffusion_code_shapes(cfg)})
	out["__time_freqs"] = time_freqs(cfg.model_channels)
	res_prefixes = [f"conditioning_timestep_integrator.{i}.resblk." for i in range(3)]
	res_prefixes += [f"layers.{i}.resblk." for i in range(cfg.num_layers)]
	res_prefixes += [f"layers.{i}." for i in range(cfg.num_layers, cfg.num_layers + 3)]
	out["__emb_cat.weight"] = torch.cat([sd[p + "emb_layers.1.weight"].float().cpu() for p in res_prefixes], dim=0)
	out["__emb_cat.bias"] = torch.cat([sd[p + "emb_layers.1.bias"].float().cpu() for p in res_prefixes], dim=0)
	for k in list(sd.keys()):
		if k.endswith("relative_pos_embeddings.relative_attention_bias.weight") and k in out:
			prefix = k[: -len("relative_pos_embeddings.relative_attention_bias.weight")]
			out[prefix + "__relbias"] = relbias_table(sd[k], cfg.head_dim)
	return out


# ------------------------------------------------------------------------------------------------ the network
def _resolve_codes(state_dict, cfg: DiffusionConfig, codes: Optional[bool]) -> int:
	"""`DiffusionTTS(codes=...)`: in_tokens when the token-conditioning tensors are to be built, else 0."""
	names = list(diffusion_code_shapes(cfg))
	missing = [n for n in names if n not in state_dict]
	if codes is False or (codes is None and missing):
		return 0
	if missing:
		raise _lib.TTKError(f"codes=True, but the state_dict lacks {len(missing)} token-conditioning tensors, e.g. {missing[:3]}")
	table = state_dict["code_embedding.weight"]
	if table.dim() != 2 or table.shape[1] != cfg.model_channels:
		raise _lib.TTKError(f"code_embedding.weight is {tuple(table.shape)}, expected [in_tokens, {cfg.model_channels}]")
	return int(table.shape[0])


def check_aligned_conditioning(aligned_conditioning, in_tokens: int, return_code_pred: bool = False) -> bool:
	"""Host-side argument checks of `timestep_independent`, before any launch.  Returns True for mel codes, False for latents (`is_latent`,
	diffusion.py:1269: float tensors are latents).  Codes outside [0, in_tokens) raise IndexError, as `nn.Embedding` does."""
	tokens = not aligned_conditioning.dtype.is_floating_point
	if (tokens or return_code_pred) and in_tokens <= 0:
		what = "token conditioning (code_embedding / code_converter)" if tokens else "return_code_pred (mel_head)"
		raise NotImplementedError(f"{what} needs the token-conditioning tensors: build the model with DiffusionTTS(..., codes=True) from a state "
								  f"dict that holds code_embedding, code_converter and mel_head")
	if tokens:
		if aligned_conditioning.dim() != 2 or aligned_conditioning.numel() == 0:
			raise ValueError(f"mel codes must be [b, M], got {tuple(aligned_conditioning.shape)}")
		if aligned_conditioning.dtype == torch.bool:
			raise TypeError("mel codes must be an integer tensor")
		lo, hi = int(aligned_conditioning.min()), int(aligned_conditioning.max())
		if lo < 0 or hi >= in_tokens:
			raise IndexError(f"mel code {lo if lo < 0 else hi} is outside the code embedding's [0, {in_tokens})")
	elif aligned_conditioning.dim() != 3:
		raise ValueError(f"latents must be [b, M, C], got {tuple(aligned_conditioning.shape)}")
	return tokens


class DiffusionTTS(_lib.Handle):
	def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: DiffusionConfig = DiffusionConfig(), dtype: str = "bf16",
				 device: str = "cuda:0", codes: Optional[bool] = None):
		"""codes: token conditioning (`code_embedding`, `code_converter`, `mel_head`; diffusion.py:1427-1432, 1456) -- None: built when the state dict
		holds all of those tensors, True: required, False: left out."""
		self.cfg = cfg
		self.in_tokens = _resolve_codes(state_dict, cfg, codes)
		super().__init__(device)
		self.dtype = _lib.DTYPES[dtype]
		self.in_channels, self.out_channels, self.model_channels = cfg.in_channels, cfg.out_channels, cfg.model_channels
		missing = [n for n in diffusion_shapes(cfg) if n not in state_dict]
		if missing:
			raise _lib.TTKError(f"state_dict lacks {len(missing)} hot-path tensors, e.g. {missing[:3]}")
		packed = pack_state_dict(state_dict, cfg, codes=self.in_tokens > 0)
		c = _lib.DiffConfigC(cfg.model_channels, cfg.num_layers, cfg.in_channels, cfg.in_latent_channels, cfg.out_channels,
							 cfg.num_heads, self.dtype)
		self._create("diff", c, packed, list(packed.keys()))
		self._idx_cache: Dict[tuple, torch.Tensor] = {}

	def parameters(self):
		"""`next(model.parameters()).device` is queried by the sampler (diffusion.py:788)."""
		yield torch.empty(0, device=self.device)

	def _index(self, M: int, T: int) -> torch.Tensor:
		key = (M, T)
		if key not in self._idx_cache:
			self._idx_cache[key] = nearest_index(M, T).to(self.device)
		return self._idx_cache[key]

	def timestep_independent(self, aligned_conditioning, conditioning_latent, expected_seq_len, return_code_pred=False):
		"""diffusion.py:1487-1515.  aligned_conditioning: AR latents [b, M, C_latent] f32, or mel codes [b, M] of an integer type (`is_latent`, :1269);
		conditioning_latent [b, 2C] -> E [b, C, T] f32, with return_code_pred (E, mel_pred [b, in_channels, T] f32)."""
		tokens = check_aligned_conditioning(aligned_conditioning, self.in_tokens, return_code_pred)
		cond = conditioning_latent.to(self.device, torch.float32).contiguous()
		b, M = aligned_conditioning.shape[:2]
		if cond.shape[0] != b:
			cond = cond.expand(b, -1).contiguous()
		T = int(expected_seq_len)
		idx = self._index(M, T)
		with torch.cuda.device(self.device):
			E = torch.empty((b, self.cfg.model_channels, T), device=self.device, dtype=torch.float32)
			mel_pred = torch.empty((b, self.cfg.in_channels, T), device=self.device, dtype=torch.float32) if return_code_pred else None
			if tokens:
				codes = aligned_conditioning.to(self.device, torch.int64).contiguous()
				_lib.check(self.lib.ttk_diff_precompute_codes(self._h, codes.data_ptr(), cond.data_ptr(), idx.data_ptr(), b, M, T, E.data_ptr(),
															  _lib.ptr(mel_pred), _lib.stream_ptr()), "ttk_diff_precompute_codes")
			else:
				lat = aligned_conditioning.to(self.device, torch.float32).contiguous()
				_lib.check(self.lib.ttk_diff_precompute(self._h, lat.data_ptr(), cond.data_ptr(), idx.data_ptr(), b, M, T,
														E.data_ptr(), _lib.stream_ptr()), "ttk_diff_precompute")
				if return_code_pred:
					_lib.check(self.lib.ttk_diff_mel_head(self._h, E.data_ptr(), b, T, mel_pred.data_ptr(), _lib.stream_ptr()), "ttk_diff_mel_head")
		return (E, mel_pred) if return_code_pred else E

	def forward(self, x, timesteps, aligned_conditioning=None, conditioning_latent=None, precomputed_aligned_embeddings=None,
				conditioning_free=False, return_code_pred=False):
		"""diffusion.py:1517-1574: [b, 100, T], [b] -> [b, 200, T] f32; with return_code_pred (out, mel_pred).  The reference runs `mel_head` whenever it is
		given aligned conditioning and drops the result unless asked; here it runs when asked."""
		assert not (return_code_pred and precomputed_aligned_embeddings is not None)  # mutually exclusive (diffusion.py:1530)
		if not conditioning_free and precomputed_aligned_embeddings is None and (aligned_conditioning is None or conditioning_latent is None):
			raise ValueError("need precomputed_aligned_embeddings or (aligned_conditioning, conditioning_latent)")
		if return_code_pred and conditioning_free:
			raise NotImplementedError("return_code_pred with conditioning_free: the reference has no mel_pred to return there (diffusion.py:1533-1573)")
		if not conditioning_free and precomputed_aligned_embeddings is None:      # argument checks first: they need no device
			check_aligned_conditioning(aligned_conditioning, self.in_tokens, return_code_pred)
		x = x.to(self.device, torch.float32).contiguous()
		b, _, T = x.shape
		t = timesteps.to(self.device, torch.int64).contiguous()
		E = mel_pred = None
		if not conditioning_free:
			if precomputed_aligned_embeddings is None:
				precomputed_aligned_embeddings = self.timestep_independent(aligned_conditioning, conditioning_latent, T, return_code_pred)
				if return_code_pred:
					precomputed_aligned_embeddings, mel_pred = precomputed_aligned_embeddings
			E = precomputed_aligned_embeddings.to(self.device, torch.float32).contiguous()
			if E.shape[0] != b:
				E = E.expand(b, -1, -1).contiguous()
		out = torch.empty((b, self.cfg.out_channels, T), device=self.device, dtype=torch.float32)
		_lib.check(self.lib.ttk_diff_forward(self._h, x.data_ptr(), t.data_ptr(), _lib.ptr(E), b, T, out.data_ptr(),
											 _lib.stream_ptr()), "ttk_diff_forward")
		return (out, mel_pred) if return_code_pred else out

	__call__ = forward


# ------------------------------------------------------------------------------------------------ schedule + samplers
def get_named_beta_schedule(schedule_name: str, num_diffusion_timesteps: int) -> np.ndarray:
	"""diffusion.py:107-131 ('linear' is the only schedule get_diffuser uses)."""
	if schedule_name != "linear":
		raise NotImplementedError(f"unknown beta schedule: {schedule_name}")
	scale = 1000 / num_diffusion_timesteps
	return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)


def space_timesteps(num_timesteps: int, section_counts) -> set:
	"""diffusion.py:1169-1222."""
	if isinstance(section_counts, str):
		if section_counts.startswith("ddim"):
			desired = int(section_counts[len("ddim"):])
			for i in range(1, num_timesteps):
				if len(range(0, num_timesteps, i)) == desired:
					return set(range(0, num_timesteps, i))
			raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
		section_counts = [int(x) for x in section_counts.split(",")]
	size_per = num_timesteps // len(section_counts)
	extra = num_timesteps % len(section_counts)
	start_idx = 0
	all_steps: List[int] = []
	for i, section_count in enumerate(section_counts):
		size = size_per + (1 if i < extra else 0)
		if size < section_count:
			raise ValueError(f"cannot divide section of {size} steps into {section_count}")
		frac_stride = 1 if section_count <= 1 else (size - 1) / (section_count - 1)
		cur_idx = 0.0
		for _ in range(section_count):
			all_steps.append(start_idx + round(cur_idx))
			cur_idx += frac_stride
		start_idx += size
	return set(all_steps)


class SpacedDiffusion:
	"""diffusion.py:1110-1166 over GaussianDiffusion.__init__ :205-262, epsilon model / learned-range variance."""

	def __init__(self, use_timesteps, betas, conditioning_free=False, conditioning_free_k=1, ramp_conditioning_free=True):
		self.use_timesteps = set(use_timesteps)
		self.original_num_steps = len(betas)
		base = np.cumprod(1.0 - np.array(betas, dtype=np.float64), axis=0)
		last = 1.0
		new_betas, self.timestep_map = [], []
		for i, ac in enumerate(base):
			if i in self.use_timesteps:
				new_betas.append(1 - ac / last)
				last = ac
				self.timestep_map.append(i)
		betas = np.array(new_betas, dtype=np.float64)
		self.betas = betas
		self.num_timesteps = int(betas.shape[0])
		self.conditioning_free = conditioning_free
		self.conditioning_free_k = conditioning_free_k
		self.ramp_conditioning_free = ramp_conditioning_free
		alphas = 1.0 - betas
		self.alphas_cumprod = np.cumprod(alphas, axis=0)
		self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
		self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
		self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
		self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
		self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
		self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
		self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
		self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)

	def step_coefs(self, i: int, sampler: str) -> _lib.StepC:
		"""Scalars of step i.  float64 table -> f32 (`.float()`, :1264); the DDIM square roots are taken in f32 on the
		f32 alpha_bar_prev as `torch.sqrt` does on the extracted tensor (:677-688)."""
		f = np.float32
		ab_prev = f(self.alphas_cumprod_prev[i])
		if self.conditioning_free:
			cfk = self.conditioning_free_k * (1 - i / self.num_timesteps) if self.ramp_conditioning_free else self.conditioning_free_k
		else:
			cfk = -1.0
		s = _lib.StepC()
		s.t = int(self.timestep_map[i])
		s.sqrt_recip_ac = f(self.sqrt_recip_alphas_cumprod[i])
		s.sqrt_recipm1_ac = f(self.sqrt_recipm1_alphas_cumprod[i])
		s.sqrt_ac_prev = np.sqrt(ab_prev, dtype=f)
		s.sqrt_1m_ac_prev = np.sqrt(f(1) - ab_prev, dtype=f)
		s.coef1 = f(self.posterior_mean_coef1[i])
		s.coef2 = f(self.posterior_mean_coef2[i])
		s.min_log = f(self.posterior_log_variance_clipped[i])
		s.max_log = f(np.log(self.betas)[i])
		s.cfk = float(cfk)
		s.sampler = 0 if sampler == "ddim" else 1
		s.nonzero = int(i != 0)
		return s

	def step_coefs_ext(self, i: int, mode: int, eta: float = 0.0, clip: bool = True) -> _lib.StepExtC:
		"""The scalars of step i that `step_coefs` does not carry (include/ttk.h: ttk_step_ext).  mode 0 ddim with eta, 1 p, 2 reverse ddim.  As torch computes them
		on the f32 tensors `_extract_into_tensor` returns: sigma and sqrt(1 - alpha_bar_prev - sigma ** 2) of ddim_sample (:677-688), the square roots of
		alpha_bar_next of ddim_reverse_sample (:724-729) -- every operation in f32, in the reference's order."""
		f = np.float32
		ab, ab_prev, ab_next = f(self.alphas_cumprod[i]), f(self.alphas_cumprod_prev[i]), f(self.alphas_cumprod_next[i])
		sigma = f(eta) * np.sqrt((f(1) - ab_prev) / (f(1) - ab), dtype=f) * np.sqrt(f(1) - ab / ab_prev, dtype=f)
		e = _lib.StepExtC()
		e.sigma = sigma
		e.dir = np.sqrt(f(1) - ab_prev - sigma * sigma, dtype=f)
		e.sqrt_ac_next = np.sqrt(ab_next, dtype=f)
		e.sqrt_1m_ac_next = np.sqrt(f(1) - ab_next, dtype=f)
		e.mode = int(mode)
		e.clip = int(bool(clip))
		return e

	def step_coefs_ms(self, i: int, clip: bool = True) -> _lib.StepMsC:
		"""The three scalars of step i of DPM-Solver++(2M) (Lu et al. 2022; include/ttk.h: ttk_step_ms), x_new = c_x x + c_d0 x0 + c_d1 x0_prev, on the respaced schedule:
		alpha_i = sqrt(alphas_cumprod[i]), sigma_i = sqrt(1 - alphas_cumprod[i]), lambda_i = log(alpha_i / sigma_i); the step goes from level i to level i - 1 with
		h = lambda_{i-1} - lambda_i, c_x = sigma_{i-1} / sigma_i, c_d = -alpha_{i-1} expm1(-h).  Index n-1 has no history: (c_x, c_d, 0), DDIM's step.  In between
		r = (lambda_i - lambda_{i+1}) / h and (c_x, c_d (1 + 1 / 2r), -c_d / 2r).  Index 0 targets alpha_bar = 1, where lambda is infinite: (0, 1, 0), x = x0 as
		DDIM's last step gives it (the "lower order final" rule).  Float64 throughout, f32 at the end, like `step_coefs_ext`."""
		n = self.num_timesteps
		if not 0 <= i < n:
			raise IndexError(f"schedule index {i} is outside [0, {n})")
		m = _lib.StepMsC()
		m.clip = int(bool(clip))
		if i == 0:
			m.c_x, m.c_d0, m.c_d1 = 0.0, 1.0, 0.0
			return m
		c_x, c_d0, c_d1 = self._coefs_ms_f64(i)
		m.c_x, m.c_d0, m.c_d1 = np.float32(c_x), np.float32(c_d0), np.float32(c_d1)
		return m

	def _coefs_ms_f64(self, i: int):
		"""(c_x, c_d0, c_d1) of `step_coefs_ms` in float64, for 0 < i < n"""
		n = self.num_timesteps
		alpha, sigma = np.sqrt(self.alphas_cumprod), np.sqrt(1.0 - self.alphas_cumprod)
		lam = np.log(alpha / sigma)
		h = lam[i - 1] - lam[i]
		c_x = sigma[i - 1] / sigma[i]
		c_d = -alpha[i - 1] * np.expm1(-h)
		if i == n - 1:
			return c_x, c_d, 0.0
		r = (lam[i] - lam[i + 1]) / h
		return c_x, c_d * (1.0 + 1.0 / (2.0 * r)), -c_d / (2.0 * r)

	@staticmethod
	def _check_hooks(denoised_fn, cond_fn):
		if denoised_fn is not None or cond_fn is not None:
			raise NotImplementedError("denoised_fn / cond_fn are not supported: a Python callable between the network and the update would put a host round trip "
									  "into every step of a loop that otherwise runs without one")

	def _model_inputs(self, model, model_kwargs, b: int):
		if not isinstance(model, DiffusionTTS):
			raise _lib.TTKError("the samplers need the libttk-backed DiffusionTTS (no fallback path)")
		E = (model_kwargs or {}).get("precomputed_aligned_embeddings")
		if E is None:
			raise ValueError("model_kwargs['precomputed_aligned_embeddings'] is required")
		if self.conditioning_free and self.ramp_conditioning_free:
			assert b == 1, "ramped conditioning-free guidance is batch-1 in the reference (diffusion.py:392)"
		return E.to(model.device, torch.float32).contiguous()

	def _sample_ext(self, model: DiffusionTTS, x, E, mode: int, eta: float, clip: bool, noise):
		"""The whole loop of one mode through ttk_diff_sample_ext, x [b, 100, T] f32 on the device in place.  noise: [n, b, 100, T] f32, block j for the j-th
		executed step, or None when no step reads one (mode 2, mode 0 at eta 0; the library refuses a missing block otherwise)."""
		n = self.num_timesteps
		b, _, T = x.shape
		sampler = "p" if mode == 1 else "ddim"
		steps = (_lib.StepC * n)(*[self.step_coefs(i, sampler) for i in range(n)])
		ext = (_lib.StepExtC * n)(*[self.step_coefs_ext(i, mode, eta, clip) for i in range(n)])
		if noise is not None:
			noise = noise.to(x.device, torch.float32).contiguous()
			if tuple(noise.shape) != (n,) + tuple(x.shape):
				raise ValueError(f"noise must be {(n,) + tuple(x.shape)}, one block per step in running order, got {tuple(noise.shape)}")
		with torch.cuda.device(x.device):
			_lib.check(model.lib.ttk_diff_sample_ext(model._h, x.data_ptr(), E.data_ptr(), b, T, steps, ext, n, _lib.ptr(noise), _lib.stream_ptr()),
					   "ttk_diff_sample_ext")
		return x

	def _steps_ms(self, clip: bool):
		n = self.num_timesteps
		return (_lib.StepC * n)(*[self.step_coefs(i, "ddim") for i in range(n)]), (_lib.StepMsC * n)(*[self.step_coefs_ms(i, clip) for i in range(n)])

	def _sample_ms(self, model: DiffusionTTS, x, E, clip: bool, ms=None):
		"""The whole DPM-Solver++(2M) loop through ttk_diff_sample_ms, x [b, 100, T] f32 on the device in place.  ms: the per-step blocks when the caller has its own
		(tests force every c_d1 to 0 to get the first-order solver)."""
		n = self.num_timesteps
		b, _, T = x.shape
		steps, own = self._steps_ms(clip)
		with torch.cuda.device(x.device):
			_lib.check(model.lib.ttk_diff_sample_ms(model._h, x.data_ptr(), E.data_ptr(), b, T, steps, own if ms is None else ms, n, _lib.stream_ptr()), "ttk_diff_sample_ms")
		return x

	def sample_loop(self, model: DiffusionTTS, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
					model_kwargs=None, device=None, progress=False, eta=0.0, sampler="ddim", consume_rng=True, step_noise=None):
		"""diffusion.py:500-508 -> ddim_sample_loop :734-810 / p_sample_loop :556-644.  Returns f32 [b, 100, T].  `eta` and `clip_denoised` act for "ddim",
		`clip_denoised` for "p" (which ignores eta, as p_sample_loop does not take it); the defaults run the entries they always ran.
		step_noise (ddim with eta != 0 only): [n, b, 100, T], the per-step randn_like draws in loop order when the caller has made them already (as
		TTSHotPath.inference_lines does, to keep them in the reference's place in the generator stream); nothing is drawn here then.
		sampler="dpm++2m" (no reference counterpart: the reference raises on it as on any other name): DPM-Solver++(2M), the second-order multistep solver, through
		ttk_diff_sample_ms; `clip_denoised` acts, `eta` must be 0 (ValueError: the solver is deterministic).  It draws nothing per step -- there is no reference stream to
		stay aligned with -- so the generator is left where the start-noise draw (if `noise` is None) leaves it; `consume_rng` and `step_noise` play no part."""
		sampler = sampler.lower()
		if sampler not in ("ddim", "p", "dpm++2m"):
			raise RuntimeError(f"Sampler not implemented: {sampler}")
		if sampler == "dpm++2m" and eta != 0.0:
			raise ValueError(f"sampler 'dpm++2m' is a deterministic solver: eta must be 0, got {eta}")
		self._check_hooks(denoised_fn, cond_fn)
		b, C, T = shape
		E = self._model_inputs(model, model_kwargs, b)
		dev = model.device
		x = (noise if noise is not None else torch.randn(*shape, device=dev)).to(dev, torch.float32).contiguous().clone()
		n = self.num_timesteps
		if sampler == "dpm++2m":
			return self._sample_ms(model, x, E, bool(clip_denoised))
		with torch.cuda.device(dev):
			if sampler == "ddim":
				# ddim_sample draws one randn_like(x) per step (:685).  With eta they are read: drawn here in loop order (or handed in as step_noise) and consumed by
				# the whole-loop entry.  Without, they are ignored: drawn behind the loop to keep the generator stream aligned (consume_rng=False: the caller
				# already made these draws, see TTSHotPath.inference_lines)
				nz = None
				if eta != 0.0:
					nz = step_noise if step_noise is not None else torch.stack([torch.randn_like(x) for _ in range(n)])
				if eta != 0.0 or not clip_denoised:
					self._sample_ext(model, x, E, 0, float(eta), bool(clip_denoised), nz)
				else:
					steps = (_lib.StepC * n)(*[self.step_coefs(i, "ddim") for i in range(n)])
					_lib.check(model.lib.ttk_diff_sample_ddim(model._h, x.data_ptr(), E.data_ptr(), b, T, steps, n, _lib.stream_ptr()),
							   "ttk_diff_sample_ddim")
				if eta == 0.0 and consume_rng:
					for _ in range(n):
						torch.randn_like(x)
			else:
				# p_sample draws one randn_like(x) per step (:545), in loop order: drawn here, consumed by the whole-loop entry
				nz = torch.stack([torch.randn_like(x) for _ in range(n)])
				if not clip_denoised:
					self._sample_ext(model, x, E, 1, 0.0, False, nz)
				else:
					steps = (_lib.StepC * n)(*[self.step_coefs(i, "p") for i in range(n)])
					_lib.check(model.lib.ttk_diff_sample_p(model._h, x.data_ptr(), E.data_ptr(), b, T, steps, n, nz.data_ptr(), _lib.stream_ptr()),
							   "ttk_diff_sample_p")
		return x

	# ---- single steps and the generator forms (diffusion.py:510-554, 602-644, 646-732, 768-810): the same update launch behind ttk_diff_begin, with pred_xstart
	def _index_of(self, t, b: int) -> int:
		"""`t`: a tensor of one repeated schedule index (or an int), as the reference's loops pass it."""
		if torch.is_tensor(t):
			if t.numel() != b or (t != t.reshape(-1)[0]).any():
				raise ValueError(f"t must hold one schedule index repeated for the batch of {b}, got {t.tolist()}")
			t = int(t.reshape(-1)[0])
		if not 0 <= int(t) < self.num_timesteps:
			raise IndexError(f"schedule index {t} is outside [0, {self.num_timesteps})")
		return int(t)

	def _single_step(self, model, x, t, mode: int, eta: float, clip: bool, model_kwargs, noise=None) -> Dict[str, torch.Tensor]:
		"""One step on a copy of x.  noise: the step's randn_like(x); None draws it here exactly where the reference does (ddim_sample :685 and p_sample :545 draw
		whether or not the value is used; ddim_reverse_sample draws nothing)."""
		b = x.shape[0]
		E = self._model_inputs(model, model_kwargs, b)
		i = self._index_of(t, b)
		dev = model.device
		x = x.to(dev, torch.float32).contiguous().clone()
		T = x.shape[-1]
		with torch.cuda.device(dev):
			if mode != 2 and noise is None:
				noise = torch.randn_like(x)
			st = self.step_coefs(i, "p" if mode == 1 else "ddim")
			ext = self.step_coefs_ext(i, mode, eta, clip)
			reads = mode == 1 or (mode == 0 and ext.sigma != 0.0)
			nz = noise.to(dev, torch.float32).contiguous() if reads else None
			px = torch.empty_like(x)
			_lib.check(model.lib.ttk_diff_begin(model._h, E.data_ptr(), b, T, _lib.stream_ptr()), "ttk_diff_begin")
			_lib.check(model.lib.ttk_diff_step_ext(model._h, x.data_ptr(), st, ext, _lib.ptr(nz), px.data_ptr(), _lib.stream_ptr()), "ttk_diff_step_ext")
		return {"sample": x, "pred_xstart": px}

	def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None):
		"""diffusion.py:510-554: x_{t-1} from x_t by the ancestral step -> {"sample", "pred_xstart"}."""
		self._check_hooks(denoised_fn, cond_fn)
		return self._single_step(model, x, t, 1, 0.0, bool(clip_denoised), model_kwargs)

	def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
		"""diffusion.py:646-694: x_{t-1} from x_t by DDIM -> {"sample", "pred_xstart"}."""
		self._check_hooks(denoised_fn, cond_fn)
		return self._single_step(model, x, t, 0, float(eta), bool(clip_denoised), model_kwargs)

	def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0):
		"""diffusion.py:696-732: x_{t+1} from x_t by the reverse ODE -> {"sample", "pred_xstart"}."""
		assert eta == 0.0, "Reverse ODE only for deterministic path"
		self._check_hooks(denoised_fn, None)
		return self._single_step(model, x, t, 2, 0.0, bool(clip_denoised), model_kwargs)

	def _loop_progressive(self, step, model, shape, noise, model_kwargs, **kw):
		img = noise if noise is not None else torch.randn(*shape, device=model.device)
		for i in reversed(range(self.num_timesteps)):
			out = step(model, img, torch.tensor([i] * shape[0]), model_kwargs=model_kwargs, **kw)
			yield out
			img = out["sample"]

	def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
								  progress=False):
		"""diffusion.py:602-644: a generator over p_sample's dicts, index n-1 .. 0; the last `sample` equals sample_loop(sampler="p") bit for bit."""
		self._check_hooks(denoised_fn, cond_fn)
		return self._loop_progressive(self.p_sample, model, shape, noise, model_kwargs, clip_denoised=clip_denoised)

	def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
									 progress=False, eta=0.0):
		"""diffusion.py:768-810: a generator over ddim_sample's dicts, index n-1 .. 0; the last `sample` equals sample_loop(sampler="ddim") bit for bit."""
		self._check_hooks(denoised_fn, cond_fn)
		return self._loop_progressive(self.ddim_sample, model, shape, noise, model_kwargs, clip_denoised=clip_denoised, eta=eta)

	def dpmpp_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None, progress=False):
		"""A generator over the steps of `sample_loop(sampler="dpm++2m")`, index n-1 .. 0, in the form of ddim_sample_loop_progressive: {"sample", "pred_xstart"} per step
		through ttk_diff_step_ms, the x0 history kept here between the steps; the last `sample` equals the whole loop's bit for bit.  Draws the start noise when `noise` is
		None and nothing else."""
		self._check_hooks(denoised_fn, cond_fn)
		return self._ms_progressive(model, shape, noise, bool(clip_denoised), model_kwargs)

	def _ms_progressive(self, model, shape, noise, clip, model_kwargs):
		b, _, T = shape
		E = self._model_inputs(model, model_kwargs, b)
		dev = model.device
		x = (noise if noise is not None else torch.randn(*shape, device=dev)).to(dev, torch.float32).contiguous()
		hist = torch.empty_like(x)      # written by the first step (c_d1 == 0 there: not read)
		for i in reversed(range(self.num_timesteps)):
			x, px = x.clone(), torch.empty_like(x)
			with torch.cuda.device(dev):
				_lib.check(model.lib.ttk_diff_begin(model._h, E.data_ptr(), b, T, _lib.stream_ptr()), "ttk_diff_begin")
				_lib.check(model.lib.ttk_diff_step_ms(model._h, x.data_ptr(), hist.data_ptr(), self.step_coefs(i, "ddim"), self.step_coefs_ms(i, clip), px.data_ptr(),
													  _lib.stream_ptr()), "ttk_diff_step_ms")
			yield {"sample": x, "pred_xstart": px}

	def ddim_reverse_sample_loop(self, model, x, clip_denoised=True, model_kwargs=None):
		"""The DDIM encoder: x_0 (a mel in [-1, 1], [b, 100, T]) -> x_n by ddim_reverse_sample at index 0, 1, ..., n-1, as one ttk_diff_sample_ext loop of mode 2.
		The reference has the step (diffusion.py:696-732) but no loop over it; this is the step called in a Python loop, which is what the fixture of
		tests/golden/diff_sampler_small.npz records.  Ramped conditioning-free guidance takes the current index i, as p_mean_variance would (:391-393).
		Draws nothing from the generator.  Returns a new tensor."""
		E = self._model_inputs(model, model_kwargs, x.shape[0])
		x = x.to(model.device, torch.float32).contiguous().clone()
		return self._sample_ext(model, x, E, 2, 0.0, bool(clip_denoised), None)


def _sample_loop_lines(self, model: DiffusionTTS, noises, embeddings, sampler="ddim", clip_denoised=True):
	"""sampler "ddim" (ttk_diff_sample_ddim_lines) or "dpm++2m" (ttk_diff_sample_ms_lines, where `clip_denoised` acts; element i then equals
	`sample_loop(..., sampler="dpm++2m")` bit for bit).  For "ddim":
	DDIM loops of several utterances of different length as ONE batch (include/ttk.h: ttk_diff_sample_ddim_lines; no reference counterpart --
	the reference diffuses a text's lines one after the other, inference.py:237-422).  noises: list of [1, 100, T_i] start noises, embeddings:
	list of [1, C, T_i] precomputed aligned embeddings.  Returns a list of [1, 100, T_i] f32, element i bit for bit what
	`sample_loop(model, (1, 100, T_i), noise=noises[i], ...)` returns.  Draws nothing from the torch generator: the caller makes the reference's
	per-line draws (start noise, DDIM's ignored per-step randn_like) in line order, as TTSHotPath.inference_lines does."""
	sampler = sampler.lower()
	if sampler not in ("ddim", "dpm++2m"):
		raise RuntimeError(f"Sampler not implemented for line batches: {sampler}")
	if sampler == "ddim" and not clip_denoised:
		raise NotImplementedError("the ragged DDIM entry clamps x0 (clip_denoised=True); use sample_loop per line")
	if not self.conditioning_free:
		raise NotImplementedError("line batches run the conditioned and the conditioning-free evaluation as one [cond | uncond] batch")
	if not isinstance(model, DiffusionTTS):
		raise _lib.TTKError("sample_loop_lines needs the libttk-backed DiffusionTTS (no fallback path)")
	dev = model.device
	b = len(noises)
	if b == 0 or len(embeddings) != b:
		raise ValueError("one start noise and one embedding per line")
	Ts = [int(n.shape[-1]) for n in noises]
	if any(e.shape[-1] != t or n.shape[0] != 1 or e.shape[0] != 1 for n, e, t in zip(noises, embeddings, Ts)):
		raise ValueError("noises[i] [1, 100, T_i] and embeddings[i] [1, C, T_i] must agree in T_i")
	Tp = (max(Ts) + 63) // 64 * 64
	C = embeddings[0].shape[1]
	with torch.cuda.device(dev):
		x = torch.zeros((b, noises[0].shape[1], Tp), device=dev, dtype=torch.float32)
		E = torch.zeros((b, C, Tp), device=dev, dtype=torch.float32)
		for i, (n, e, t) in enumerate(zip(noises, embeddings, Ts)):
			x[i, :, :t] = n[0].to(dev, torch.float32)
			E[i, :, :t] = e[0].to(dev, torch.float32)
		n_steps = self.num_timesteps
		steps = (_lib.StepC * n_steps)(*[self.step_coefs(i, "ddim") for i in range(n_steps)])
		tlen = (_lib.C.c_int * b)(*Ts)
		if sampler == "dpm++2m":
			ms = (_lib.StepMsC * n_steps)(*[self.step_coefs_ms(i, bool(clip_denoised)) for i in range(n_steps)])
			_lib.check(model.lib.ttk_diff_sample_ms_lines(model._h, x.data_ptr(), E.data_ptr(), b, Tp, tlen, steps, ms, n_steps, _lib.stream_ptr()),
					   "ttk_diff_sample_ms_lines")
		else:
			_lib.check(model.lib.ttk_diff_sample_ddim_lines(model._h, x.data_ptr(), E.data_ptr(), b, Tp, tlen, steps, n_steps, _lib.stream_ptr()),
					   "ttk_diff_sample_ddim_lines")
		return [x[i:i + 1, :, :t].contiguous() for i, t in enumerate(Ts)]


SpacedDiffusion.sample_loop_lines = _sample_loop_lines


def get_diffuser(steps=80, cond_free=True, cond_free_k=2, trained_diffusion_steps=4000) -> SpacedDiffusion:
	"""diffusion.py:1576-1590."""
	return SpacedDiffusion(use_timesteps=space_timesteps(trained_diffusion_steps, [steps]),
						   betas=get_named_beta_schedule("linear", trained_diffusion_steps),
						   conditioning_free=cond_free, conditioning_free_k=cond_free_k)
