"""Drop-in for the reference's autoregressive module object: same method names, arguments and return values as
`UnifiedVoice` (/root/reference/tortoise_tts/models/unified_voice.py:334-679) for the calls `TTS.inference` makes
(tortoise_tts/inference.py:266-285, 334-346, 371-379) and for `forward`'s teacher-forced losses (:544-612), backed by libttk (HIP, gfx950).  No torch fallback exists:
every forward goes through the C ABI or raises.

What runs where
  * GPT-2 stack, embeddings, final norms, mel head, KV cache ........ libttk  (csrc/ar.hip and kernels)
  * forward's losses: both heads, the row cross-entropy, the [B, C, T] logits  libttk  (ttk_ar_score; csrc/xent.hip); the clipping and padding of its
    integer inputs is `score_inputs`, index work on the host side
  * logits processors / warpers, softmax, multinomial(1) given its noise, stop/pad bookkeeping, the next step's input
    embedding ......................................................... libttk  (csrc/sample.hip, one launch per token)
  * the Exp(1) noise of torch.multinomial ............................ libttk, inside the mel-head launch: torch's own Philox
    stream restated (csrc/ttk_rng.h), used only after a bitwise comparison with `exponential_` on this device and shape
    (else torch `exponential_` on the same stream) -- the generator stream is part of the reference's observable behaviour
    (seed 0 on every call) and is left where torch's draws would have left it; typical sampling (rare, off by default)
    runs inside the kernel too since round 3 (sampling.py keeps the torch-op forms for `hf_exact_top_p`).
  * the per-token loop .............................................. here; one HIP-graph replay per token.
  * greedy search (do_sample false or omitted, num_beams 1) ........ libttk  (csrc/sample.hip: the argmax form of the token step, ttk_ar_greedy_next); the
    same loop and captured step as sampling, no noise armed, nothing drawn from the generator behind the reseed.
  * the reference's own samplers (tortoise_tts/samplers.py: decayed repetition penalty, stop-length penalty, dynamic temperature, mirostat; keywords of
    `inference_speech` / `get_generator`) ............................ libttk  (csrc/sample_ext.hip: a second token-step kernel, ttk_ar_sample_next_ext, launched in
    ttk_ar_sample_next's place only when one of them is on; same loop, same captured step, same noise per token).
  * beam search (num_beams > 1) ..................................... libttk  (csrc/beam.hip: the beam step -- log-softmax, warpers, the
    multinomial without replacement over num_beams * V, HF's running / finished bookkeeping -- and the in-place KV-cache reorder); the loop
    here enqueues {beam step, reorder, decode} per token and polls the done word; `beam_search_lines` does so for several lines as one decode batch
    (ttk_beam_step_lines, ttk_ar_reorder_cache_lines: a search state per line, lines x beams <= 16 rows).

How the host layer is laid out: five drivers -- `_generate` (+ `_token_loop`), `_generate_lines`, `_beam_generate`, `beam_search_lines`, `_loop_stream` -- differ in their loop and
in how they account for the torch generator; what they share is written once:
  * `_session` ........ one generation on the handle: refusal while a stream is open, device guard, reseed, state reset, noise armed; disarmed again
                        however the body ends, health flags read
  * `_capture_step` ... the token step into a HIP graph (the non-streamed and the streamed loop each keep their own capture per state)
  * `_StopPoll` ....... the look, LAG steps late, at the end-of-generation word the device writes
  * `_max_new`, `_pipe_key` ... the new-token budget; what of the sampling keywords a state is keyed by
  * `_NoiseState` ..... base of `_GenState` and `_BeamState`: the self-check of the head-drawn noise against torch, arming and disarming it
The handle itself (creation from named tensors, destruction) is `_lib.Handle`'s, as for every other libttk wrapper.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import sys
import warnings
from typing import Dict, Iterator, Optional, Tuple

import torch

from . import _lib
from .sampling import LogitsPipeline, multinomial1, setup_seed
from .weights import ARConfig, ar_score_shapes, ar_shapes

LAG = 2      # steps the host runs ahead of the device-side end-of-generation word it polls


def check_ids(ids: torch.Tensor, n: int, what: str):
	"""token ids index embedding rows on the device: an id outside the table must be the IndexError nn.Embedding raises in the
	reference, not an out-of-bounds read"""
	if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
		raise IndexError(f"{what} ids must lie in [0, {n}); got [{int(ids.min())}, {int(ids.max())}]")


def score_inputs(cfg: ARConfig, text_inputs, text_lengths, mel_codes, wav_lengths, types=None, clip_inputs=True):
	"""What `UnifiedVoice.forward` does to its integer inputs before the embeddings (unified_voice.py:561-583), as plain index work on the tensors'
	own device: the `types` product, the clip to the longest text / clip of the batch, `set_mel_padding` (:494-506: codes past
	wav_lengths // mel_length_compression + 1 become the stop token), and the targets of `build_aligned_inputs_and_targets` on the padded rows.
	Returns (text [B, Tt'], codes [B, M'], text_targets [B, Tt' + 2], mel_targets [B, M' + 2]), all int64; the inputs are left as they are."""
	text = torch.as_tensor(text_inputs).to(torch.int64)
	codes = torch.as_tensor(mel_codes).to(torch.int64)
	if text.dim() != 2 or codes.dim() != 2:
		raise ValueError("text_inputs and mel_codes are [B, T] id tensors")
	B, M = codes.shape
	if types is not None:
		text = text * (1 + torch.as_tensor(types).to(text.device, torch.int64)).unsqueeze(-1)
	wav_lengths = torch.as_tensor(wav_lengths).view(-1).to("cpu")
	mel_lengths = torch.div(wav_lengths, cfg.mel_length_compression, rounding_mode="trunc")
	if mel_lengths.numel() not in (1, B):
		raise ValueError("wav_lengths must have 1 or B entries")
	if clip_inputs:
		max_text_len, max_mel_len = int(torch.as_tensor(text_lengths).max()), int(mel_lengths.max())
		if max_mel_len < 1:
			raise ValueError(f"wav_lengths clip the mel codes to {max_mel_len} (the longest clip has fewer than mel_length_compression = {cfg.mel_length_compression} samples)")
		if max_text_len < 1:
			raise ValueError(f"text_lengths clip the text to {max_text_len} tokens")
		text, codes = text[:, :max_text_len], codes[:, :max_mel_len]
		M = codes.shape[1]
	check_ids(text, cfg.number_text_tokens + 1, "text token")
	check_ids(codes, cfg.number_mel_codes, "mel code")
	if int(mel_lengths.min()) + 1 < M:
		codes = codes.clone()
		for b in range(B):
			end = int(mel_lengths[b if mel_lengths.numel() == B else 0]) + 1
			if end < M:
				codes[b, end:] = cfg.stop_mel_token
	pad = torch.nn.functional.pad
	return text, codes, pad(text, (0, 2), value=cfg.stop_text_token), pad(codes, (0, 2), value=cfg.stop_mel_token)


# The reference's own samplers (tortoise_tts/samplers.py; the commented-out arguments of its inference, inference.py:154-163): keyword, value that means "off".
# Any of them on moves the token step to the second sampling kernel (include/ttk.h: ttk_sample_ext, ttk_ar_sample_next_ext); all off is the launch it always was.
SAMPLER_KNOBS = (("repetition_penalty_decay", 0.0), ("stop_length_penalty", 0.0), ("min_temperature", None), ("mirostat_tau", 0.0), ("mirostat_eta", 0.1))
NO_KNOBS = tuple(default for _, default in SAMPLER_KNOBS)
MIROSTAT_RANKS = 101      # probabilities mirostat's estimate of the Zipf slope reads (samplers.py:121-125)


def pop_sampler_knobs(kw) -> tuple:
	"""take the sampler knobs out of a generate keyword dict: (decay, stop-length penalty, min_temperature or None, tau, eta), normalised so that every way of
	saying "off" gives NO_KNOBS' entry (a state is keyed by them)"""
	decay, stop_len, min_t, tau, eta = (kw.pop(name, default) for name, default in SAMPLER_KNOBS)
	decay, stop_len, tau = float(decay or 0.0), float(stop_len or 0.0), float(tau or 0.0)
	min_t = None if min_t is None or float(min_t) < 0 else float(min_t)
	eta = 0.1 if eta is None else float(eta)
	if tau < 0 or eta < 0:
		raise ValueError(f"mirostat_tau ({tau}) and mirostat_eta ({eta}) must not be negative")
	return decay, stop_len, min_t, tau, (eta if tau > 0 else 0.1)


LORA_MAX_RANK = 256      # csrc/ar.hip: ttk_ar_lora_set


def lora_modules(cfg: ARConfig) -> Tuple[str, ...]:
	"""the 4 x layers HF Conv1D modules run-time adapters attach to (include/ttk.h: ttk_ar_lora_init)"""
	return tuple(f"gpt.h.{l}.{m}" for l in range(cfg.layers) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"))


class UnifiedVoice(_lib.Handle):
	def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: ARConfig = ARConfig(), dtype: str = "bf16",
				 device: str = "cuda:0", max_batch: int = 16, max_ctx: Optional[int] = None, use_graph: bool = True,
				 hf_exact_top_p: bool = False, adapters: bool = False):
		"""adapters: keep f32 masters of the GPT-2 block matrices on the device (12 * model_dim^2 * layers * 4 bytes) so that LoRA adapters can be attached,
		swapped and detached on the live handle (`load_lora` / `enable_lora` / `disable_lora`); not available with fp8 weights.  Off: the handle is what it
		always was, and an adapter is folded into the weights before they get here (checkpoint.materialize_lora).
		hf_exact_top_p: run HF's TopPLogitsWarper as torch ops in front of the sampling kernel when top_p < 1 (its f32 cumsum rounding, bit for
		bit) instead of the kernel's exact fixed-point cut -- the two differ only on rows whose cumulative mass ties with 1 - top_p within f32
		rounding (csrc/sample.hip; tests/test_gpu_parity.py::test_top_p_boundary_stress); costs the per-token torch launches the kernel removed."""
		self.hf_exact_top_p = hf_exact_top_p
		self.cfg = cfg
		super().__init__(device)
		self.dtype = _lib.DTYPES[dtype]
		if self.dtype == _lib.TTK_FP8:      # the decode GEMVs have 16 rows: fp8 activations buy nothing there; 'fp8' means fp8 weights
			self.dtype = _lib.TTK_FP8W
		self.max_batch = max_batch
		self.max_ctx = max_ctx or (cfg.max_text_seq_len + 2 + cfg.max_mel_seq_len)
		self.use_graph = use_graph
		# attributes TTS.inference reads (inference.py:354,368)
		self.stop_mel_token, self.start_mel_token = cfg.stop_mel_token, cfg.start_mel_token
		self.mel_length_compression = cfg.mel_length_compression
		self.max_mel_tokens, self.max_text_tokens = cfg.max_mel_tokens, cfg.max_text_tokens
		self.model_dim, self.layers, self.heads = cfg.model_dim, cfg.layers, cfg.heads
		self.number_mel_codes = cfg.number_mel_codes

		# the text head is read by the teacher-forced losses only (forward(return_latent=False)): uploaded when the state dict holds it
		self.scoring = "text_head.weight" in state_dict and "text_head.bias" in state_dict
		names = list((ar_score_shapes if self.scoring else ar_shapes)(cfg).keys())
		missing = [n for n in names if n not in state_dict]
		if missing:
			raise _lib.TTKError(f"state_dict lacks {len(missing)} hot-path tensors, e.g. {missing[:3]}")
		c = _lib.ARConfigC(cfg.layers, cfg.model_dim, cfg.heads, cfg.max_mel_seq_len, cfg.max_text_seq_len,
						   cfg.number_text_tokens + 1, cfg.number_mel_codes, cfg.start_text_token, cfg.stop_text_token,
						   cfg.start_mel_token, cfg.stop_mel_token, self.dtype, max_batch, self.max_ctx)
		self._create("ar", c, state_dict, names)
		self._adapters, self._loras, self.active_lora = bool(adapters), {}, None
		if adapters:
			mats = lora_modules(cfg)
			views, keep = _lib.weight_views(state_dict, [m + ".weight" for m in mats])
			with torch.cuda.device(self.device):
				_lib.check(self.lib.ttk_ar_lora_init(self._h, views, len(mats)), "ttk_ar_lora_init")
			del keep
		self._states: Dict[tuple, "_GenState"] = {}
		self._prefix = None
		self._streaming = False          # a streamed generation is open on this handle (its KV cache, noise and latent ring belong to it)

	def parameters(self):
		yield torch.empty(0, device=self.device)

	# ------------------------------------------------------------------ C-ABI calls
	def _check_ids(self, ids: torch.Tensor, n: int, what: str):
		check_ids(ids, n, what)

	def _prefill(self, cond: torch.Tensor, text: torch.Tensor, B: int, prompt: Optional[torch.Tensor] = None) -> torch.Tensor:
		"""prompt [1 or B, n] int64: the mel tokens of a prompted continuation, cached behind start_mel (include/ttk.h: ttk_ar_prefill_prompted)"""
		cond = cond.to(self.device, torch.float32).contiguous()
		text = text.to(self.device, torch.int64).contiguous().view(-1)
		_lib.require_cuda(cond, text)
		self._check_ids(text, self.cfg.number_text_tokens + 1, "text token")
		logits = torch.empty((B, self.cfg.number_mel_codes), device=self.device, dtype=torch.float32)
		if prompt is not None and prompt.shape[1]:
			prompt = prompt.to(self.device, torch.int64).contiguous()
			self._check_ids(prompt, self.cfg.number_mel_codes, "prompt mel code")
			_lib.check(self.lib.ttk_ar_prefill_prompted(self._h, cond.data_ptr(), cond.shape[0], text.data_ptr(), text.numel(), prompt.data_ptr(), prompt.shape[0],
														prompt.shape[1], B, logits.data_ptr(), _lib.stream_ptr()), "ttk_ar_prefill_prompted")
			return logits
		_lib.check(self.lib.ttk_ar_prefill(self._h, cond.data_ptr(), cond.shape[0], text.data_ptr(), text.numel(), B,
										   logits.data_ptr(), _lib.stream_ptr()), "ttk_ar_prefill")
		return logits

	def _prefill_lines(self, cond: torch.Tensor, texts, rows_per_line: int) -> torch.Tensor:
		"""several text lines as one decode batch (include/ttk.h: ttk_ar_prefill_lines): line g -> candidates [g * rows, (g + 1) * rows)"""
		G = len(texts)
		cond = cond.to(self.device, torch.float32)
		cond = (cond.expand(G, -1) if cond.shape[0] == 1 else cond).contiguous()
		if cond.shape[0] != G:
			raise ValueError("one conditioning latent, or one per line")
		flat = torch.cat([t.to(self.device, torch.int64).reshape(-1) for t in texts]).contiguous()
		_lib.require_cuda(cond, flat)
		self._check_ids(flat, self.cfg.number_text_tokens + 1, "text token")
		lens = (_lib.C.c_int * G)(*[int(t.numel()) for t in texts])
		logits = torch.empty((G * rows_per_line, self.cfg.number_mel_codes), device=self.device, dtype=torch.float32)
		_lib.check(self.lib.ttk_ar_prefill_lines(self._h, cond.data_ptr(), flat.data_ptr(), lens, G, rows_per_line, logits.data_ptr(),
												 _lib.stream_ptr()), "ttk_ar_prefill_lines")
		return logits

	def _decode(self, tok: torch.Tensor, logits: torch.Tensor, hidden: Optional[torch.Tensor] = None):
		"""one KV-cached step fed with `tok` (callers pass ids this module sampled, or teacher-forced ones they validated)"""
		_lib.check(self.lib.ttk_ar_decode(self._h, tok.data_ptr(), logits.data_ptr(), _lib.ptr(hidden), _lib.stream_ptr()),
				   "ttk_ar_decode")

	def _decode_next(self, logits: torch.Tensor, hidden: Optional[torch.Tensor] = None):
		"""the same step started from the input row the fused sampling launch (ttk_ar_sample_next) left in the handle"""
		_lib.check(self.lib.ttk_ar_decode_next(self._h, logits.data_ptr(), _lib.ptr(hidden), _lib.stream_ptr()), "ttk_ar_decode_next")

	def _check_health(self):
		"""after a generation: did the decode step's folded LayerNorm meet rows it cannot represent well (include/ttk.h: ttk_ar_health)?  The
		reference has no such failure mode -- it normalises in f32 before the matmul -- so the deviation is reported where it can occur."""
		flags = _lib.C.c_int(0)
		_lib.check(self.lib.ttk_ar_health(self._h, _lib.C.byref(flags), _lib.stream_ptr()), "ttk_ar_health")
		self.last_health = flags.value
		if flags.value & 1:
			warnings.warn("tortoise_tts_amd: a row of the GPT-2 residual stream had |mean| > 8 std during decoding; the folded-LayerNorm launches lose "
						  "precision on such rows (set TTK_AR_LNFOLD=0 before building the model for the form that normalises in f32 first)", RuntimeWarning)
		if flags.value & 2:
			warnings.warn("tortoise_tts_amd: non-finite LayerNorm statistics during decoding (an fp16 operand above 65504?); "
						  "use dtype='bf16' or TTK_AR_LNFOLD=0", RuntimeWarning)
		return flags.value

	# ------------------------------------------------------------------ reference surface
	def forward(self, speech_conditioning_latent, text_inputs, text_lengths, mel_codes, wav_lengths, types=None,
				text_first=True, raw_mels=None, return_attentions=False, return_latent=False, clip_inputs=True):
		"""unified_voice.py:544-612, text first.  return_latent=True (what inference uses, with clip_inputs=False: inference.py:371-379): f32
		[B, M', model_dim].  return_latent=False, the reference's default: (loss_text, loss_mel, mel_logits) -- the mean teacher-forced
		cross-entropies as 0-dim f32 device tensors and the mel logits [B, number_mel_codes, M' + 2] f32; `self.loss` holds the two losses as in the
		reference and `self.last_nll` the per-token rows {"text": [B, Tt' + 2], "mel": [B, M' + 2]} (F.cross_entropy(reduction="none")).
		return_attentions=True stays refused here: the reference's `forward` unpacks the tuple of maps that `get_logits(get_attns=True)` returns (:508-516) into
		two names (:593), so it returns layer 1's map on a 2-layer model and raises at any other depth -- not an interface to copy.  The maps themselves, all
		layers or a subset, come from `attentions(latent, text, codes)`."""
		if raw_mels is not None or not text_first or return_attentions:
			raise NotImplementedError("forward is implemented text first on mel codes: text_first=False, raw_mels and return_attentions are not")
		if not return_latent and not self.scoring:
			raise NotImplementedError("this model was built without text_head.weight / text_head.bias, which the losses need: pass the full state dict "
									  "(weights.ar_score_shapes), or scoring=True to checkpoint.load_autoregressive")
		B = mel_codes.shape[0]
		cond = speech_conditioning_latent.to(self.device, torch.float32)
		if cond.shape[0] != B:
			cond = cond.expand(B, -1)
		cond = cond.contiguous()
		text = text_inputs.to(self.device, torch.int64)
		if text.shape[0] != B:
			text = text.expand(B, -1)
		text, codes, _, _ = score_inputs(self.cfg, text, text_lengths, mel_codes.to(self.device, torch.int64), wav_lengths, types, clip_inputs)
		text, codes = text.contiguous(), codes.contiguous()
		if not return_latent:
			r = self._score(cond, text, codes)
			self.loss = dict(text=r["loss"][0], mel=r["loss"][1])
			self.last_nll = dict(text=r["nll_text"], mel=r["nll_mel"])
			return r["loss"][0], r["loss"][1], r["mel_logits"]
		M = codes.shape[1]
		out = torch.empty((B, M, self.cfg.model_dim), device=self.device, dtype=torch.float32)
		_lib.check(self.lib.ttk_ar_latents(self._h, cond.data_ptr(), text.data_ptr(), text.shape[1], codes.data_ptr(), M, B,
										   out.data_ptr(), _lib.stream_ptr()), "ttk_ar_latents")
		return out

	def _score(self, cond: torch.Tensor, text: torch.Tensor, codes: torch.Tensor, text_logits: bool = False) -> Dict[str, torch.Tensor]:
		"""include/ttk.h: ttk_ar_score on clipped and padded device inputs (cond [B, D] f32, text [B, Tt], codes [B, M] int64, contiguous)"""
		_lib.require_cuda(cond, text, codes)
		c, B, Tt, M = self.cfg, codes.shape[0], text.shape[1], codes.shape[1]
		new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)
		r = dict(loss=new(2), nll_text=new(B, Tt + 2), nll_mel=new(B, M + 2), mel_logits=new(B, c.number_mel_codes, M + 2))
		if text_logits:
			r["text_logits"] = new(B, c.number_text_tokens + 1, Tt + 2)
		_lib.check(self.lib.ttk_ar_score(self._h, cond.data_ptr(), text.data_ptr(), Tt, codes.data_ptr(), M, B, r["loss"].data_ptr(), r["nll_text"].data_ptr(),
										 r["nll_mel"].data_ptr(), _lib.ptr(r.get("text_logits")), r["mel_logits"].data_ptr(), _lib.stream_ptr()), "ttk_ar_score")
		return r

	__call__ = forward

	# ------------------------------------------------------------------ attention maps and the text-to-audio alignment
	def _dense_inputs(self, latent, text_inputs, mel_codes):
		"""(cond [B, D] f32, text [B, Tt], codes [B, M] int64), contiguous on the device; one latent / one text row serve every code row.  The ids are
		validated where they live, as `forward` does (an id outside its table must not reach the embedding kernels): for device tensors that is a min and a
		max reduction and a host read each, for host tensors plain host work; with B > 1 the shared latent / text row is copied B times on the device."""
		codes = torch.as_tensor(mel_codes)
		text = torch.as_tensor(text_inputs)
		codes, text = (codes[None] if codes.dim() == 1 else codes), (text[None] if text.dim() == 1 else text)
		if codes.dim() != 2 or text.dim() != 2 or codes.dtype.is_floating_point or text.dtype.is_floating_point or not codes.shape[1] or not text.shape[1]:
			raise ValueError("text_inputs and mel_codes are non-empty [B, T] (or [T]) integer id tensors")
		check_ids(text, self.cfg.number_text_tokens + 1, "text token")
		check_ids(codes, self.cfg.number_mel_codes, "mel code")
		B = codes.shape[0]
		cond = latent.to(self.device, torch.float32)
		cond = cond[None] if cond.dim() == 1 else cond
		if text.shape[0] not in (1, B) or cond.shape[0] not in (1, B):
			raise ValueError(f"one latent and one text row, or one per code row (B={B}); got {cond.shape[0]} and {text.shape[0]}")
		text = text.to(self.device, torch.int64).expand(B, -1).contiguous()
		return cond.expand(B, -1).contiguous(), text, codes.to(self.device, torch.int64).contiguous()

	def _attentions(self, cond, text, codes, layers):
		_lib.require_cuda(cond, text, codes)
		layers = list(range(self.cfg.layers)) if layers is None else [int(l) for l in layers]
		if not layers:
			raise ValueError("attentions: the layer list is empty")
		B, Tt, M = codes.shape[0], text.shape[1], codes.shape[1]
		S = Tt + M + 5
		if len(layers) * B * self.cfg.heads * S * S * 4 >= 2 ** 31:      # (the C entry refuses the same; here before the allocation)
			raise _lib.TTKError(f"attentions: {len(layers)} layers x B={B} x {self.cfg.heads} heads x {S} x {S} f32 is an output of 2 GiB or more: select fewer layers")
		out = torch.empty((len(layers), B, self.cfg.heads, S, S), device=self.device, dtype=torch.float32)
		arr = (_lib.C.c_int * len(layers))(*layers)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_ar_attentions(self._h, cond.data_ptr(), text.data_ptr(), Tt, codes.data_ptr(), M, B, arr, len(layers), out.data_ptr(),
												  _lib.stream_ptr()), "ttk_ar_attentions")
		return tuple(out[j] for j in range(len(layers)))

	def attentions(self, latent, text_inputs, mel_codes, layers=None):
		"""The GPT-2 attention maps of the teacher-forced pass -- what the reference's `get_logits(get_attns=True)` returns (unified_voice.py:508-516) -- on ids
		that are clipped and padded as `forward` leaves them, for a subset of the layers (None: all): a tuple with one f32 tensor [B, heads, S, S] per entry of `layers`, S = Tt + M + 5 (include/ttk.h: ttk_ar_attentions names the rows).  The dense
		pass stops behind the last selected layer."""
		return self._attentions(*self._dense_inputs(latent, text_inputs, mel_codes), layers)

	def _alignment_heads(self, heads):
		from .alignment import default_heads
		heads = default_heads(self.cfg.layers, self.cfg.heads) if heads is None else [(int(l), int(h)) for l, h in heads]
		if not heads:
			raise ValueError("text_alignment: the head list is empty")
		for l, h in heads:
			if not (0 <= l < self.cfg.layers and 0 <= h < self.cfg.heads):
				raise ValueError(f"text_alignment: (layer {l}, head {h}) is outside {self.cfg.layers} layers x {self.cfg.heads} heads")
		return heads

	def _text_attention(self, cond, text, codes, heads):
		"""f32 [B, n, M, Tt]: the text-alignment block A[m][t] = P[Tt + 3 + m][2 + t] of every (layer, head) of `heads` (include/ttk.h: ttk_ar_text_attention)"""
		_lib.require_cuda(cond, text, codes)
		B, Tt, M, n = codes.shape[0], text.shape[1], codes.shape[1], len(heads)
		out = torch.empty((B, n, M, Tt), device=self.device, dtype=torch.float32)
		arr = (_lib.C.c_int * (2 * n))(*[v for lh in heads for v in lh])
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_ar_text_attention(self._h, cond.data_ptr(), text.data_ptr(), Tt, codes.data_ptr(), M, B, arr, n, out.data_ptr(), _lib.stream_ptr()),
					   "ttk_ar_text_attention")
		return out

	def _align_blocks(self, blocks, median_width, keep_matrix=True):
		"""blocks f32 [nb, n, M, Tt] on the device -> (matrix [nb, M, Tt] device or None, traces u8 numpy [nb, M, Tt], totals f32 numpy [nb]): the cost
		(csrc/align.hip: k_align_prepare), the DTW table and trace (k_dtw), and ONE copy to the host that carries trace and totals together"""
		import numpy as np
		median_width = int(median_width)
		if median_width < 1 or median_width > 15 or median_width % 2 == 0:
			raise ValueError(f"median_width must be odd and in 1..15, got {median_width}")
		nb, n, M, Tt = blocks.shape
		new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)
		cost, matrix, D = new(nb, M, Tt), (new(nb, M, Tt) if keep_matrix else None), new(nb, (M + 1) * (Tt + 1))
		nt = (nb * M * Tt + 3) // 4 * 4
		packed = torch.empty(nt + 4 * nb, device=self.device, dtype=torch.uint8)      # [trace | totals]
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_align_prepare(blocks.data_ptr(), nb, n, M, Tt, median_width, cost.data_ptr(), _lib.ptr(matrix), _lib.stream_ptr()), "ttk_align_prepare")
			_lib.check(self.lib.ttk_dtw(cost.data_ptr(), nb, M, Tt, D.data_ptr(), packed.data_ptr(), packed.data_ptr() + nt, _lib.stream_ptr()), "ttk_dtw")
		host = packed.cpu().numpy()      # the one synchronisation
		return matrix, host[:nb * M * Tt].reshape(nb, M, Tt), host[nt:].view(np.float32).copy()

	def text_alignment(self, latent, text_inputs, mel_codes, heads=None, median_width=7):
		"""Which text token each mel code came from: the monotone text-to-audio path through the attention of the teacher-forced pass (no reference
		counterpart; OpenAI Whisper's word-timestamp recipe with mel codes as the time axis -- the steps are listed in include/ttk.h at ttk_align_prepare and
		ttk_dtw).  heads: a list of (layer, head), None = every head of layers >= layers / 2 -- a guess from similar models that nothing here can check on a
		trained checkpoint (`rank_alignment_heads` scores the heads of one).  median_width: odd, <= 15.
		Returns {"matrix": f32 [B, M, Tt] on the device (the negated cost), "path": per sequence (text indices, mel indices) int64 numpy arrays,
		"token_start": int64 numpy [B, Tt] in mel-code units, "total": f32 numpy [B], the path's cost}.  One dense pass that stops behind the last selected
		layer, the map kernel on the selected heads, two small kernels and one copy to the host that carries trace and totals; the backtrace runs there.  In
		front of the pass: the id validation and input copies of `_dense_inputs` (device reductions with host reads when the ids are device tensors; pass host
		tensors to keep that on the host) and the upload of the head list from pageable host memory, which the host waits for.  Sequences of one call share Tt
		and M: lines of different length take one call each."""
		import numpy as np
		from . import alignment as A
		heads = self._alignment_heads(heads)
		cond, text, codes = self._dense_inputs(latent, text_inputs, mel_codes)
		matrix, traces, totals = self._align_blocks(self._text_attention(cond, text, codes, heads), median_width)
		paths = [A.backtrace(t) for t in traces]
		starts = np.stack([A.token_starts(ti, mi, text.shape[1]) for ti, mi in paths])
		return {"matrix": matrix, "path": paths, "token_start": starts, "total": totals, "heads": heads}

	def rank_alignment_heads(self, latent, text_inputs, mel_codes, median_width=7):
		"""[((layer, head), score)] over every head, best first: the mean of that head's own standardised and median-filtered block along its own DTW path,
		averaged over the sequences -- high where a head's attention follows one monotone path through the text.  For picking `heads` on a trained
		checkpoint.  The blocks and the per-head cost / DTW run on the device (each head as a sequence of its own); the ranking is host logic."""
		from . import alignment as A
		heads = [(l, h) for l in range(self.cfg.layers) for h in range(self.cfg.heads)]
		cond, text, codes = self._dense_inputs(latent, text_inputs, mel_codes)
		blocks = self._text_attention(cond, text, codes, heads)
		B, n, M, Tt = blocks.shape
		scores = [0.0] * n
		per = max(1, 65535 // n)      # sequences per launch: a launch takes at most 65535 (sequence, head) pairs
		for b0 in range(0, B, per):
			part = blocks[b0:b0 + per].reshape(-1, 1, M, Tt)
			matrix, traces, _ = self._align_blocks(part, median_width)
			matrix = matrix.cpu().numpy()
			for i, trace in enumerate(traces):
				ti, mi = A.backtrace(trace)
				scores[i % n] += float(matrix[i, mi, ti].mean()) / B
		return sorted(zip(heads, scores), key=lambda hs: -hs[1])

	def inference_speech(self, speech_conditioning_latent, text_inputs, input_tokens=None, num_return_sequences=1,
						 max_generate_length=None, typical_sampling=False, typical_mass=.9, kv_cache=True, candidate_shard=None,
						 **hf_generate_kwargs):
		"""unified_voice.py:632-668 + the sample branch of `generate` (stream_generator.py:213-639, HF `_sample`).
		Returns int64 [B, L <= max_generate_length], rows padded with stop_mel_token after their EOS.

		do_sample false or omitted (HF's GenerationConfig default) with num_beams 1 is greedy search: the token is the argmax of the processed scores, exact
		ties to the lowest index.  repetition_penalty, suppress_tokens and typical_sampling / typical_mass act; temperature, top_k and top_p are ignored with
		one warning, as HF builds no warpers without do_sample; num_return_sequences must be 1.  `generate` reseeds and then draws nothing: the device
		generator is left at the offset it had directly behind the reseed, and `last_generate["rng_step"]` is 0.

		The reference's own samplers (tortoise_tts/samplers.py; the controls of its web UI, never wired into its `generate` call) are keywords here, sampling branch
		only: repetition_penalty_decay (reptition_penalize: `repetition_penalty` divided in, grown by distance ** decay from a token's latest occurrence, over the
		sampled and prompt tokens), stop_length_penalty (length_penalize on the stop token: > 0 longer, < 0 shorter; `length_penalty` stays HF's beam ranking),
		min_temperature (dynamic_temperature: from `temperature` down to it as the row's largest probability rises), mirostat_tau / mirostat_eta (mirostat v1 in
		the place of the plain draw; needs top_k 0 or >= 101).  Defaults (0, 0, None, 0, 0.1) are the call without them, bit for bit.  With any of them on the
		token step runs on a second kernel (csrc/sample_ext.hip); the noise consumed per token, and so the generator offset afterwards, does not change.

		candidate_shard=(lo, hi) (no reference counterpart; tortoise_tts_amd/dist.py): sample only candidates lo..hi-1 of the
		`num_return_sequences`, as one rank of a candidate-sharded run.  RNG contract: the rank draws the multinomial noise of ALL
		candidates per token (the same Philox stream on every rank: `generate` reseeds to 0) and consumes its own rows, so the ids it
		returns are bit for bit the rows lo..hi-1 of the unsharded call -- up to the length, which here ends with the shard's own last
		row (the gather pads with the stop token, as the unsharded loop does for finished rows)."""
		if text_inputs.shape[0] != 1:
			raise NotImplementedError("one text line per call, as inference.py:244-246 does")
		num_beams = hf_generate_kwargs.get("num_beams", 1) or 1
		knobs = pop_sampler_knobs(hf_generate_kwargs)
		self._check_sampler_knobs(knobs, hf_generate_kwargs, greedy=not hf_generate_kwargs.get("do_sample", False), num_beams=num_beams, shard=candidate_shard,
								  typical=typical_sampling)
		if num_beams != 1:
			# the beam-sample branch of `generate` (HF `_beam_search`, do_sample=True): csrc/beam.hip
			if not hf_generate_kwargs.get("do_sample", False):
				raise NotImplementedError("beam search is implemented for the sampling branch only (do_sample=True, as TTS.inference passes it)")
			if input_tokens is not None:
				raise NotImplementedError("beam search takes no input_tokens (prompted continuation runs on the sampling branch, num_beams=1)")
			if candidate_shard is not None:
				raise NotImplementedError("beam search is not sharded over ranks: the beams of a line exchange histories every token (candidate_shard needs num_beams=1)")
			if typical_sampling:
				raise NotImplementedError("typical_sampling together with beam search is not implemented (num_beams=1 has it)")
			return self._beam_generate(speech_conditioning_latent, text_inputs, int(num_beams), num_return_sequences, max_generate_length, hf_generate_kwargs)
		greedy = not hf_generate_kwargs.get("do_sample", False)
		if greedy and num_return_sequences != 1:
			# HF: "Greedy methods without beam search do not support `num_return_sequences` different than 1"; the reference's fork (stream_generator.py):
			# "num_return_sequences has to be 1 ... when doing greedy search"
			raise ValueError(f"greedy search (do_sample=False, num_beams=1) does not support `num_return_sequences` different than 1 (got {num_return_sequences})")
		prompt = None
		if input_tokens is not None:
			# Prompted continuation (unified_voice.py:651-656; `TTS.inference` never passes it).  The reference tiles the fake prefix and the prompts to
			# num_return_sequences rows (:653-655) and then hands generate() num_return_sequences AGAIN, which expands every row that many times
			# (HF _expand_inputs_for_generation: repeat_interleave): num_return_sequences ** 2 sequences come back, row i * nrs + j = sample j of prompt row
			# i % R, the prompt tokens in front (:668 cuts at trunc_index only) and counted in max_generate_length (:660).  Restated from source; the loop on
			# such rows is pinned by the reference's own sample_stream (tests/golden/sample_stream.npz, "prompted").
			if candidate_shard is not None:
				raise NotImplementedError("a prompted continuation is not sharded over ranks")
			if input_tokens.dim() != 2 or input_tokens.shape[0] < 1 or num_return_sequences % input_tokens.shape[0] != 0:
				raise ValueError("The number of return sequences must be divisible by the number of input sequences")
			prompt = input_tokens.to(self.device, torch.int64).repeat(num_return_sequences // input_tokens.shape[0], 1).repeat_interleave(num_return_sequences, 0)
			if bool((prompt == self.stop_mel_token).any()):
				raise ValueError("input_tokens must not contain the stop token")
		# omitted keywords mean HF GenerationConfig defaults in the reference (stream_generator.py:262-276): do_sample False (greedy
		# search; TTS.inference always samples, inference.py:336), top_k 50, temperature / top_p / penalty 1
		if greedy:
			self._warn_ignored_warpers(hf_generate_kwargs)
		gen, _ = self._generate(speech_conditioning_latent, text_inputs, num_return_sequences if prompt is None else prompt.shape[0], max_generate_length,
								typical_mass if typical_sampling else None, hf_generate_kwargs, stream=False, shard=candidate_shard, prompt=prompt, greedy=greedy, knobs=knobs)
		return gen

	def _check_sampler_knobs(self, knobs, kw, greedy=False, num_beams=1, shard=None, typical=False):
		"""what the reference's samplers (SAMPLER_KNOBS) do not combine with, refused before anything is sampled; nothing to check when all are off"""
		if knobs == NO_KNOBS:
			return
		decay, stop_len, min_t, tau, _ = knobs
		on = ", ".join(f"{name}={v!r}" for (name, default), v in zip(SAMPLER_KNOBS[:4], knobs) if v != default)
		if num_beams != 1:
			raise NotImplementedError(f"{on}: the reference's samplers run in the token step of the sampling branch (num_beams=1); the beam step does not take them")
		if greedy and (tau > 0 or min_t is not None):
			raise ValueError(f"{on}: mirostat and the dynamic temperature are samplers -- they shape a draw, and greedy search (do_sample false or omitted) draws nothing; pass do_sample=True")
		if greedy:
			raise NotImplementedError(f"{on}: the decayed repetition penalty and the stop-length penalty are built into the sampling token step only; greedy search "
									  "(do_sample false or omitted) takes repetition_penalty without a decay")
		if shard is not None:
			raise NotImplementedError(f"{on}: a candidate-sharded run does not take the reference's samplers (candidate_shard needs them off)")
		temperature, top_k, top_p = kw.get("temperature", 1.0) or 1.0, kw.get("top_k", 50) or 0, kw.get("top_p", 1.0)
		if self.cfg.number_mel_codes > 9216:
			raise NotImplementedError(f"{on}: the sampling kernel that runs the reference's samplers holds a row of at most 9216 scores in registers "
									  f"(number_mel_codes = {self.cfg.number_mel_codes})")
		if self.hf_exact_top_p and (typical or (top_p is not None and top_p < 1.0)):
			raise NotImplementedError(f"{on}: with hf_exact_top_p the top-p / typical warpers run as torch ops in FRONT of the sampling kernel, behind which these samplers "
									  "would come too late (their place is before the warpers); build the model without hf_exact_top_p, or leave top_p / typical_sampling off")
		if min_t is not None and min_t > temperature:
			raise ValueError(f"min_temperature={min_t} exceeds temperature={temperature}: the dynamic temperature falls from `temperature` to `min_temperature`")
		if tau > 0 and 0 < top_k < MIROSTAT_RANKS:
			raise ValueError(f"mirostat_tau={tau} with top_k={top_k}: mirostat estimates the slope of the distribution from its {MIROSTAT_RANKS} most likely tokens, and "
							 f"fewer survive top_k (the reference divides by zero there; an omitted top_k is HF's default 50): pass top_k=0 or top_k >= {MIROSTAT_RANKS}")

	@staticmethod
	def _warn_ignored_warpers(kw):
		"""HF's GenerationConfig.validate: sampling-only flags that are set while do_sample is false get a warning and play no part"""
		given = [f"{k}={kw[k]!r}" for k, default in (("temperature", 1.0), ("top_k", 50), ("top_p", 1.0)) if kw.get(k) is not None and kw[k] != default]
		if given:
			warnings.warn(f"`do_sample` is false (greedy search): {', '.join(given)} only act in the sampling branches and are ignored", UserWarning, stacklevel=3)

	def inference_speech_lines(self, speech_conditioning_latent, texts, num_return_sequences=1, max_generate_length=None, **hf_generate_kwargs):
		"""`inference_speech` for several text lines as ONE decode batch (no reference counterpart: TTS.inference walks its lines one by one,
		inference.py:244-246, and every line streams the GPT-2 weights again for its 16 candidates; a token step over 2 / 4 lines costs 1.36x /
		2.05x the step over one).  texts: list of [1, Tt_g] id tensors.  Returns a list of int64 [num_return_sequences, L_g]: element g is bit for
		bit what `inference_speech(latent, texts[g], ...)` returns -- each row keeps the cache length of its own line, every line draws the same
		[num_return_sequences, V] multinomial noise (the reference reseeds to 0 per line), and line g is cut where its own last row finished.
		`self.last_generate_lines[g]` says where the generator stands after line g's sampling in the reference (steps, rng_start, rng_step):
		a caller that draws per line afterwards (TTSHotPath.inference_lines) re-positions it with `position_rng_after_line(g)`.
		do_sample false or omitted: greedy search as in `inference_speech`, one row per line (num_return_sequences must be 1, up to max_batch lines)."""
		if hf_generate_kwargs.get("num_beams", 1) not in (None, 1):
			raise NotImplementedError("this entry samples: beam search over a batch of lines is beam_search_lines(latent, texts, num_beams=N)")
		greedy = not hf_generate_kwargs.get("do_sample", False)
		if greedy and num_return_sequences != 1:
			raise ValueError(f"greedy search (do_sample=False, num_beams=1) does not support `num_return_sequences` different than 1 (got {num_return_sequences})")
		texts = list(texts)
		if any(t.dim() != 2 or t.shape[0] != 1 for t in texts):
			raise NotImplementedError("texts: a list of [1, Tt] id tensors, one per line")
		if hf_generate_kwargs.get("input_tokens") is not None:
			raise NotImplementedError("input_tokens (prompted continuation) is not on the inference hot path")
		hf_generate_kwargs.pop("input_tokens", None)
		hf_generate_kwargs.pop("kv_cache", None)
		typical = bool(hf_generate_kwargs.get("typical_sampling", False))
		knobs_on = pop_sampler_knobs(dict(hf_generate_kwargs)) != NO_KNOBS      # the reference's samplers: line by line (each line's mirostat state is its own call's)
		if not knobs_on:
			pop_sampler_knobs(hf_generate_kwargs)
		if len(texts) == 1 or (typical and self.hf_exact_top_p) or knobs_on:      # one line, or HF's warpers as torch ops in front of the kernel (built per call): the per-line calls
			out, self.last_generate_lines = [], []
			for t in texts:
				out.append(self.inference_speech(speech_conditioning_latent, t, num_return_sequences=num_return_sequences,
												 max_generate_length=max_generate_length, **hf_generate_kwargs))
				self.last_generate_lines.append(dict(self.last_generate, seed=hf_generate_kwargs.get("seed", 0)))
			return out
		ts, tm = hf_generate_kwargs.pop("typical_sampling", False), hf_generate_kwargs.pop("typical_mass", .9)
		typical_mass = tm if ts else None
		if greedy:
			self._warn_ignored_warpers(hf_generate_kwargs)
		return self._generate_lines(speech_conditioning_latent, texts, num_return_sequences, max_generate_length, hf_generate_kwargs, typical_mass, greedy)

	def position_rng_after_line(self, g: int):
		"""leave the torch generators as the reference's `generate` on line g alone leaves them (reseeded, advanced by that line's draws)"""
		info = self.last_generate_lines[g]
		setup_seed(info["seed"])
		torch.cuda.default_generators[self.device.index or 0].set_offset(info["rng_start"] + info["steps"] * info["rng_step"])

	def _max_new(self, prefix_tokens, max_generate_length):
		"""the number of new tokens a call may generate behind a prefix of `prefix_tokens` cached rows"""
		c = self.cfg
		max_new = (c.max_mel_tokens - 1) if max_generate_length is None else int(max_generate_length)
		if prefix_tokens + max_new > self.max_ctx or max_new + 2 > c.max_mel_seq_len:
			raise _lib.TTKError(f"prefix {prefix_tokens} + {max_new} new tokens exceed max_ctx={self.max_ctx} or the mel position table ({c.max_mel_seq_len})")
		return max_new

	def _pipe_key(self, kw, typical_mass, greedy=False, knobs=NO_KNOBS):
		"""(what of the keywords is baked into a generation state, whether the stop token can be sampled at all).  The greedy flag is part of the key: a
		sampling state's captured step is never replayed for greedy search or the reverse; the warpers greedy search ignores are not.  The reference's samplers
		(`pop_sampler_knobs`) follow at indices 7..11."""
		suppress = tuple(kw.get("suppress_tokens") or ())
		warpers = (None, None, None) if greedy else (kw.get("temperature", 1.0), kw.get("top_k", 50), kw.get("top_p", 1.0))
		pipe_key = warpers + (kw.get("repetition_penalty", 1.0), suppress, typical_mass, bool(greedy)) + tuple(knobs)
		return pipe_key, self.cfg.stop_mel_token not in suppress

	@contextlib.contextmanager
	def _session(self, seed, make_state, prompt=None, arm=(), streamed=False):
		"""One generation on the handle, from the reseed to the noise switched off again: yields (state, the device's torch generator, its offset
		behind the reseed).  The body runs the loop and does its own accounting of what the reference's draws would have consumed; the noise is disarmed
		however the body ends, and the health flags are read when it ends well (`streamed`: always -- a consumer may walk away from a stream)."""
		self._require_idle()            # (a generator body runs at its first next(): two generators may have been created, only one may run)
		with torch.cuda.device(self.device):
			st = make_state()
			setup_seed(seed)
			gen = torch.cuda.default_generators[self.device.index or 0]
			off_start = gen.get_offset()
			st.reset(self.cfg, prompt)
			if st.own_rng:
				st.arm_noise(gen, *arm)
			health = streamed
			try:
				yield st, gen, off_start
				health = True
			finally:
				st.disarm_noise()
				if health:
					self._check_health()

	def _generate_lines(self, cond, texts, C, max_generate_length, kw, typical_mass=None, greedy=False):
		c = self.cfg
		self._require_idle()            # a line batch rewrites the KV cache, the noise arming and (through the ring) an open stream's latent buffer
		G = len(texts)
		B = G * C
		if B > self.max_batch:
			raise _lib.TTKError(f"{G} lines x {C} candidates exceed max_batch={self.max_batch}")
		max_new = self._max_new(max(int(t.shape[1]) for t in texts) + 4, max_generate_length)
		pipe_key, can_stop = self._pipe_key(kw, typical_mass, greedy)
		seed = kw.get("seed", 0)
		with self._session(seed, lambda: self._gen_state(B, max_new, pipe_key, C, 0, lines=G), arm=(0,)) as (st, gen, off_start):
			n = self._token_loop(st, gen, off_start, lambda: self._prefill_lines(cond, texts, C), max_new, can_stop)
			step = st.noise_step if st.own_rng else (gen.get_offset() - off_start) // max(n, 1)
			ids = st.ids[:, :n]
			first_stop = torch.where((ids == c.stop_mel_token).any(dim=1), (ids == c.stop_mel_token).float().argmax(dim=1), torch.full((B,), n, device=ids.device)).view(G, C)
			done = bool(can_stop) & (first_stop < n).all(dim=1)
			n_line = torch.where(done, first_stop.max(dim=1).values + 1, torch.full((G,), n, device=ids.device)).tolist()
			out, self.last_generate_lines = [], []
			for g in range(G):
				out.append(ids[g * C:(g + 1) * C, :int(n_line[g])].clone())
				self.last_generate_lines.append(dict(steps=int(n_line[g]), rng_start=off_start, rng_step=step, seed=seed))
			self.position_rng_after_line(G - 1)
			self.last_generate = dict(self.last_generate_lines[-1])
			return out

	def _beam_generate(self, cond, text, N, R, max_generate_length, kw):
		"""HF `_beam_search` with do_sample=True (HF:generation/utils.py:3208-3509) for one text line: N beams prefilled on the shared prefix, then per
		token {ttk_beam_step; ttk_ar_reorder_cache; ttk_ar_decode of the chosen tokens}.  Returns `sequences[:R]` behind the prompt, cropped to the
		longest returned beam and padded with the stop token (step 5, :3510-3523).  The search ends on the device (the done word of ttk_beam_step);
		the host looks at it LAG tokens late, and the steps enqueued past the end are no-ops that draw nothing from the torch generator."""
		self._require_idle()
		self._check_beams(N, R, kw)
		max_new = self._max_new(text.shape[1] + 4, max_generate_length)
		if max_new < 1:
			raise ValueError("max_generate_length must be at least 1")
		with self._session(kw.get("seed", 0), lambda: _BeamState(self, N, max_new, kw)) as (st, gen, off_start):
			st.logits.copy_(self._prefill(cond, text, N))
			self._beam_loop(st, max_new)
			state = st.state.tolist()
			steps = state[2 * N + 1]
			if steps <= 0:
				raise _lib.TTKError("beam search did not end within max_generate_length steps (the done word of ttk_beam_step is unset)")
			if st.own_rng:
				gen.set_offset(off_start + steps * st.noise_step)      # what the torch.multinomial of every step would have consumed
			self.last_generate = dict(steps=steps, rng_start=off_start, rng_step=(gen.get_offset() - off_start) // steps)
			length = max(state[N:N + R])
			return st.seqs[steps & 1, 1, :R, :length].clone()

	def _beam_loop(self, st, max_new):
		"""the token loop of a beam search, one line or several, from the prefill's logits in `st.logits` until the device reports the end of the (last) search or
		max_new steps are enqueued; returns when the device has finished"""
		n, poll = 0, _StopPoll()
		while True:
			st.step()
			n += 1
			if n >= max_new:
				break
			if st.own_rng:
				ended = poll.step_complete() and int(st.done[0])
			else:                                        # torch draws the noise: a step past the end would consume generator state
				torch.cuda.synchronize(self.device)
				ended = int(st.done[0])
			if ended:
				break
			st.reorder_cache()
			self._decode(st.tok, st.logits)
		torch.cuda.synchronize(self.device)

	def _check_beams(self, N, R, kw, G=1):
		"""what a beam search of G lines x N beams returning R sequences per line cannot be asked for; raised before the first device call"""
		if R > N:
			raise ValueError(f"`num_return_sequences` ({R}) has to be smaller or equal to `num_beams` ({N}).")
		if G * N > min(16, self.max_batch):
			raise _lib.TTKError(f"{N} beams exceed min(16, max_batch={self.max_batch})" if G == 1 else
								f"{G} lines x {N} beams exceed min(16, max_batch={self.max_batch})")
		top_k = kw.get("top_k", 50) or 0
		if 0 < top_k < 2 * N:
			raise ValueError(f"top_k={top_k} keeps fewer tokens than the 2 * num_beams = {2 * N} continuations a beam step selects; which of the removed "
							 "(probability 0) ones torch.multinomial would pick is unspecified: use top_k=0 or top_k >= 2 * num_beams")

	def beam_search_lines(self, speech_conditioning_latent, texts, num_beams, num_return_sequences=1, max_generate_length=None, **hf_generate_kwargs):
		"""`inference_speech(..., num_beams=N)` for several text lines as ONE decode batch of G lines x N beams <= 16 rows (no reference counterpart: the
		reference searches line by line, and every line streams the GPT-2 weights once per token for its N rows).  texts: list of [1, Tt_g] id tensors.  Returns a
		list of int64 [num_return_sequences, L_g]: element g is bit for bit what `inference_speech(latent, texts[g], num_beams=N, ...)` returns.  Per token
		{ttk_beam_step_lines; ttk_ar_reorder_cache_lines; ttk_ar_decode}: every line has its own search state and draws the flat [1, N * V] noise of its own call; a
		line whose search is over rides along (stop tokens, identity reorder) until the last one ends.  `last_generate_lines[g]` is line g's own (steps,
		rng_start, rng_step, seed), for `position_rng_after_line`; the generators are left where the last line's own call leaves them.  One line is that call.
		This is the beam-sample branch: do_sample may be omitted (it is True); False, input_tokens, typical_sampling, candidate_shard and the reference's sampler
		knobs are refused as `inference_speech(num_beams=N)` refuses them."""
		N, R = int(num_beams), num_return_sequences
		kw = hf_generate_kwargs
		texts = list(texts)
		if any(t.dim() != 2 or t.shape[0] != 1 for t in texts) or not texts:
			raise NotImplementedError("texts: a list of [1, Tt] id tensors, one per line")
		if N < 2:
			raise ValueError(f"beam search needs num_beams >= 2 (got {num_beams}): inference_speech_lines samples a batch of lines without beams")
		if kw.get("num_beams", N) not in (None, N):
			raise ValueError(f"num_beams is given twice ({num_beams} and {kw['num_beams']})")
		kw.pop("num_beams", None)
		kw.pop("kv_cache", None)
		knobs = pop_sampler_knobs(kw)
		self._check_sampler_knobs(knobs, kw, num_beams=N)
		if not kw.pop("do_sample", True):
			raise NotImplementedError("beam search is implemented for the sampling branch only (do_sample=True, as TTS.inference passes it)")
		if kw.pop("input_tokens", None) is not None:
			raise NotImplementedError("beam search takes no input_tokens (prompted continuation runs on the sampling branch, num_beams=1)")
		if kw.pop("candidate_shard", None) is not None:
			raise NotImplementedError("beam search is not sharded over ranks: the beams of a line exchange histories every token (candidate_shard needs num_beams=1)")
		typical = kw.pop("typical_sampling", False)
		kw.pop("typical_mass", None)
		if typical:
			raise NotImplementedError("typical_sampling together with beam search is not implemented (num_beams=1 has it)")
		G = len(texts)
		self._require_idle()
		self._check_beams(N, R, kw, G)
		max_new = self._max_new(max(int(t.shape[1]) for t in texts) + 4, max_generate_length)
		if max_new < 1:
			raise ValueError("max_generate_length must be at least 1")
		seed = kw.get("seed", 0)
		if G == 1:
			out = [self.inference_speech(speech_conditioning_latent, texts[0], num_return_sequences=R, max_generate_length=max_generate_length, do_sample=True,
										 num_beams=N, **kw)]
			self.last_generate_lines = [dict(self.last_generate, seed=seed)]
			return out
		with self._session(seed, lambda: _BeamState(self, N, max_new, kw, lines=G)) as (st, gen, off_start):
			st.logits.copy_(self._prefill_lines(speech_conditioning_latent, texts, N))
			self._beam_loop(st, max_new)
			state = st.state.tolist()
			if any(row[2 * N + 1] <= 0 for row in state):
				raise _lib.TTKError("beam search did not end within max_generate_length steps (a done word of ttk_beam_step_lines is unset)")
			# one torch.multinomial per step of a line's own call: what every line's own search would have consumed
			rng_step = st.noise_step if st.own_rng else (gen.get_offset() - off_start) // max(row[2 * N + 1] for row in state)
			out, self.last_generate_lines = [], []
			for g, row in enumerate(state):
				steps, length = row[2 * N + 1], max(row[N:N + R])
				out.append(st.seqs[g, steps & 1, 1, :R, :length].clone())
				self.last_generate_lines.append(dict(steps=steps, rng_start=off_start, rng_step=rng_step, seed=seed))
			self.position_rng_after_line(G - 1)
			self.last_generate = {k: v for k, v in self.last_generate_lines[-1].items() if k != "seed"}
			return out

	def _require_idle(self):
		"""one generation at a time per handle: the KV cache, the noise arming and the latent ring of an open streamed generation are the handle's (the
		reference's module is re-entrant because HF keeps all of that per call); starting another one would corrupt both silently, so it is refused"""
		if self._streaming:
			raise _lib.TTKError("a streamed generation is still open on this model: exhaust or close() its generator before starting another generation")

	# ------------------------------------------------------------------ run-time LoRA adapters (inference.py:99-104, 204-216; models/lora.py:120-145)
	def _require_adapters(self):
		if not getattr(self, "_adapters", False):
			raise _lib.TTKError("this model was built without adapters=True: it keeps no f32 masters to attach an adapter to (build it with "
								"UnifiedVoice(..., adapters=True) or load_autoregressive(..., adapters=True); without it a LoRA file is folded in at load time)")

	def load_lora(self, name: str, tensors_or_path, scaling: Optional[float] = None):
		"""Read an adapter (a LoRA file as `TTS` reads it, or a dict of its tensors), check it against this model and keep it on the device under `name`;
		`enable_lora(name)` attaches it.  Keys as in `checkpoint.normalize_lora`; scaling: the argument, else the file's alpha / rank, else 1.0 (the
		reference's default adapter has alpha == rank).  Loading under the name of the enabled adapter re-attaches the new tensors."""
		from .checkpoint import CheckpointError, normalize_lora, read_lora
		self._require_adapters()
		file_scaling = None
		if isinstance(tensors_or_path, (str, os.PathLike)):
			tensors, file_scaling = read_lora(tensors_or_path)
		else:
			tensors = dict(tensors_or_path)
		shapes = ar_shapes(self.cfg)
		known = lora_modules(self.cfg)
		flat = {}
		for mod, (A, Bm) in normalize_lora(tensors).items():
			if mod not in known:
				raise CheckpointError(f"'{mod}': adapters attach at run time to gpt.h.<layer>.{{attn.c_attn, attn.c_proj, mlp.c_fc, mlp.c_proj}} of the "
									  f"{self.cfg.layers} layers only; fold an adapter on another module at load time (materialize_lora)")
			K, N = shapes[mod + ".weight"]
			rank = int(A.shape[0])
			if tuple(Bm.shape) != (K, rank) or tuple(A.shape) != (rank, N):
				raise CheckpointError(f"'{mod}': lora shapes {tuple(Bm.shape)} x {tuple(A.shape)} do not match weight {(K, N)}")
			if not 1 <= rank <= LORA_MAX_RANK:
				raise CheckpointError(f"'{mod}': rank {rank} is outside 1..{LORA_MAX_RANK}")
			flat[mod + ".lora_A"], flat[mod + ".lora_B"] = A, Bm
		s = float(scaling if scaling is not None else (file_scaling if file_scaling is not None else 1.0))
		dev = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in flat.items()}
		self._loras.pop(name, None)          # a reloaded name becomes the last loaded
		self._loras[name] = (dev, s)
		if self.active_lora == name:
			self.enable_lora(name)

	def _lora_set(self, tensors: Dict[str, torch.Tensor], scaling: float):
		"""include/ttk.h: ttk_ar_lora_set on named f32 device tensors (`<module>.lora_A` / `<module>.lora_B`); none = every matrix back to its base"""
		_lib.require_cuda(*tensors.values())
		for k, t in tensors.items():
			if t.dtype != torch.float32:
				raise _lib.TTKError(f"'{k}' is {t.dtype}: adapter tensors go to the device as f32")
		names = list(tensors)
		views, keep = _lib.weight_views(tensors, names)
		with torch.cuda.device(self.device):
			_lib.check(self.lib.ttk_ar_lora_set(self._h, views if names else None, len(names), float(scaling), _lib.stream_ptr()), "ttk_ar_lora_set")
		del keep

	def enable_lora(self, name: Optional[str] = None):
		"""Attach a loaded adapter (None: the only or the last-loaded one): every matrix it covers computes with W + (lora_B lora_A) * scaling from here on,
		every other one with its base weight -- also those a previously enabled adapter covered.  Refused while a streamed generation is open."""
		self._require_adapters()
		self._require_idle()
		if name is None:
			if not self._loras:
				raise _lib.TTKError("no adapter is loaded: call load_lora(name, tensors_or_path) first")
			name = next(reversed(self._loras))
		if name not in self._loras:
			raise _lib.TTKError(f"no adapter named {name!r} is loaded (loaded: {sorted(self._loras)})")
		tensors, scaling = self._loras[name]
		self._lora_set(tensors, scaling)
		self.active_lora = name

	def disable_lora(self):
		"""Detach: every matrix back to its base weight, bit for bit what a model built without adapters computes."""
		self._require_adapters()
		self._require_idle()
		self._lora_set({}, 1.0)
		self.active_lora = None

	def compute_embeddings(self, cond_latents, text_inputs, kv_cache=True):
		"""unified_voice.py:614-630: remembers the prefix, returns the fake id row [b, P+1]."""
		self._prefix = (cond_latents, text_inputs)
		P1 = text_inputs.shape[1] + 4
		ids = torch.ones((cond_latents.shape[0], P1), dtype=torch.long, device=self.device)
		ids[:, -1] = self.start_mel_token
		return ids

	def get_generator(self, inputs, max_length=500, **hf_generate_kwargs) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
		"""unified_voice.py:670-679 / stream_generator.py:911-1190: yields (codes [B], latent [B, model_dim]) per token,
		latent = final_norm(last hidden) (:1172).  Always the sampling loop, whatever `do_sample` says: the reference's `sample_stream` draws every
		token with torch.multinomial (stream_generator.py:1161) and has no greedy branch."""
		if self._prefix is None:
			raise _lib.TTKError("call compute_embeddings first")
		cond, text = self._prefix
		n_new = max_length - inputs.shape[1]
		B = hf_generate_kwargs.pop("num_return_sequences", 1) or 1
		knobs = pop_sampler_knobs(hf_generate_kwargs)          # the reference's samplers, as in `inference_speech`
		self._check_sampler_knobs(knobs, hf_generate_kwargs)
		return self._generate(cond, text, B, n_new, None, hf_generate_kwargs, stream=True, knobs=knobs)

	# ------------------------------------------------------------------ the token loop
	def _generate(self, cond, text, num_return_sequences, max_generate_length, typical_mass, kw, stream, shard=None, prompt=None, greedy=False, knobs=NO_KNOBS):
		self._require_idle()
		n_in = 0 if prompt is None else int(prompt.shape[1])
		if stream and n_in:
			raise NotImplementedError("the streaming generator takes no prompt tokens")
		C = num_return_sequences * text.shape[0]          # candidates the noise is drawn for
		lo, hi = (0, C) if shard is None else (int(shard[0]), int(shard[1]))
		if not (0 <= lo < hi <= C):
			raise ValueError(f"candidate_shard {shard} is not a non-empty range inside [0, {C})")
		if stream and shard is not None:
			raise NotImplementedError("the streaming generator is not sharded")
		B = hi - lo
		if B > self.max_batch:
			raise _lib.TTKError(f"{B} candidates exceed max_batch={self.max_batch}")
		max_new = self._max_new(text.shape[1] + 4, max_generate_length)
		if n_in >= max_new:      # HF's stopping criterion is only looked at after a token has been appended: the reference would still sample one
			raise ValueError(f"{n_in} prompt tokens leave no room below max_generate_length={max_new}")
		pipe_key, can_stop = self._pipe_key(kw, typical_mass, greedy, knobs)
		if stream:
			return self._loop_stream(cond, text, B, max_new, pipe_key, can_stop)
		with self._session(kw.get("seed", 0), lambda: self._gen_state(B, max_new, pipe_key, C, lo), prompt, arm=(lo, n_in)) as (st, gen, off_start):
			n = self._token_loop(st, gen, off_start, lambda: self._prefill(cond, text, B, prompt), max_new, can_stop, n_in)
			if st.own_rng:
				gen.set_offset(off_start + (n - n_in) * st.noise_step)        # what the n - n_in torch draws would have consumed
			# what the sampling consumed from the generator: dist.py aligns a shard's stream with the unsharded run's from this
			self.last_generate = dict(steps=n - n_in, rng_start=off_start, rng_step=(gen.get_offset() - off_start) // max(n - n_in, 1))
			return st.ids[:, :n].clone(), None

	def _capture_step(self, st):
		"""the token step {ttk_ar_decode_next; [typical warper]; exponential_; ttk_ar_sample_next} -- greedy search: {ttk_ar_decode_next; ttk_ar_greedy_next} --
		as it is issued right now (with or without the hidden ring set), captured into a HIP graph.  The caller has run the step eagerly before (warm kernels)."""
		torch.cuda.synchronize(self.device)
		g = torch.cuda.CUDAGraph()
		# thread-local capture mode: another host thread may be enqueuing (and allocating for) the previous
		# line's diffusion meanwhile (TTSHotPath.inference_lines); in the default global mode its hipMalloc /
		# hipFree would invalidate this capture.
		# capture_begin / capture_end run OUTSIDE inference mode whatever the caller's mode: torch creates the
		# generator's graph-side seed / offset tensors at the first capture and updates them in place at every
		# later capture and replay -- created under inference_mode they would make any later capture from a
		# caller without it fail ("inplace update to inference tensor outside InferenceMode").
		ctx = torch.cuda.graph(g, capture_error_mode="thread_local")
		with torch.inference_mode(False):
			ctx.__enter__()
		try:
			self._decode_next(st.logits)
			st.sample(0)
		except BaseException:
			with torch.inference_mode(False):
				ctx.__exit__(*sys.exc_info())
			raise
		with torch.inference_mode(False):
			ctx.__exit__(None, None, None)
		return g

	def _token_loop(self, st, gen, off_start, prefill, max_new, can_stop, n0=0):
		"""n0: id columns that are filled already (the prompt tokens of a prompted continuation); returns the filled columns at the end"""
		c = self.cfg
		st.logits.copy_(prefill())
		n = n0
		if not (self.use_graph and st.graphable):
			while True:
				st.sample(n)
				n += 1
				if n >= max_new or (can_stop and int(st.unfinished.max()) == 0):
					break
				self._decode_next(st.logits)
		else:
			# tokens 1 and 2 eagerly (the second pass also warms every kernel before a capture), then one HIP-graph
			# replay per token: {ttk_ar_decode_next; [typical warper]; exponential_; ttk_ar_sample_next}.  Every position-dependent
			# quantity (cache length, mel position, output column, length of the token history the repetition penalty reads) lives in
			# device memory, so ONE graph serves all tokens and every text length.
			# HF's stopping test (`unfinished_sequences.max() == 0` after every token, a host round trip that idles the GPU)
			# becomes a flag the sampling kernel raises in pinned memory; the host looks at it LAG replays late, so the GPU
			# always has work queued.  The <= LAG tokens generated past the true end are all padding; they are cut off below
			# and the generator offset they consumed is handed back, so ids AND the RNG stream equal the reference's.
			st.sample(n0)
			if st.rng_step is None:
				st.rng_step = gen.get_offset() - off_start
			n = n0 + 1
			poll = _StopPoll()
			stopped = can_stop and int(st.unfinished.max()) == 0
			while n < max_new and not stopped:
				if st.graph is None:
					self._decode_next(st.logits)
					st.sample(n)
					n += 1
					stopped = can_stop and int(st.unfinished.max()) == 0
					if n < max_new and not stopped:
						st.graph = self._capture_step(st)
						# no random numbers are drawn inside the captured step when the mel head draws the noise: launch the instantiated
						# graph directly then -- CUDAGraph.replay() first refills the generator's seed / offset tensors, two launches per token
						# (greedy search draws nothing at all)
						st.graph_exec = st.graph.raw_cuda_graph_exec() if (st.own_rng or st.greedy) and os.environ.get("TTK_AR_RAW_REPLAY", "1") != "0" else None
					continue
				if st.graph_exec:
					_lib.check(self.lib.ttk_graph_launch(st.graph_exec, _lib.stream_ptr()), "ttk_graph_launch")
				else:
					st.graph.replay()
				n += 1
				if can_stop and poll.step_complete():      # the replay LAG tokens back is complete: its flag is visible
					stopped = int(st.done[0]) != 0
			if can_stop:
				# exact end: HF stops right after the token with which the last row finishes
				torch.cuda.synchronize(self.device)
				ids = st.ids[:, :n]
				is_stop = ids == c.stop_mel_token
				if bool(is_stop.any(dim=1).all()):
					n_true = max(int(is_stop.float().argmax(dim=1).max()) + 1, n0 + 1)
					if n_true < n:
						if not st.own_rng:
							gen.set_offset(gen.get_offset() - (n - n_true) * st.rng_step)
						n = n_true
		return n

	def _gen_state(self, B, max_new, pipe_key, C=None, lo=0, lines=1):
		"""generation states (device buffers + the captured token step) keyed by what is baked into them; a few are kept so that
		alternating shapes (e.g. `TTS.inference` lines with different max lengths) do not re-capture every call"""
		C = B if C is None else C
		key = (B, max_new, pipe_key, C, lo, lines)
		states = self._states
		if key in states:
			states[key] = states.pop(key)             # most recently used last
		else:
			while len(states) >= 4:
				states.pop(next(iter(states)))
			states[key] = _GenState(self, B, max_new, pipe_key, C, lo, lines)
		return states[key]

	def _loop_stream(self, cond, text, B, max_new, pipe_key, can_stop):
		"""stream_generator.py:1106-1190, pinned by the reference's own loop (tests/golden/sample_stream.npz): token k is yielded with
		final_norm(hidden) of the forward it was sampled from -- the prefill's last row for the first token -- and every token is
		yielded, the last one included; the loop ends after the token with which the last row finishes or after max_new tokens.

		Same machinery as the non-streaming loop: the fused sampling launch (processors, warpers, multinomial, padding, next input row), the noise
		drawn in the mel-head launch, ONE captured token step replayed per token.  Between two yields nothing runs on the host but a graph launch
		and an event wait: the yielded tokens are a column of the state's id buffer, the latents a slot of a per-call [max_new, B, d] buffer that
		the step's LayerNorm launch fills directly (ttk_ar_set_hidden_ring: the slot index is the device-side token counter, so the captured launch
		serves every step).  The host runs LAG steps ahead of the consumer; HF's `unfinished_sequences.max() == 0` test (a host round trip per
		token) is the pinned word the sampling kernel leaves -- the token count at which the last row finished -- read after the event of the
		token about to be yielded.  The yielded tensors are slots of two per-call buffers (tokens [max_new, B], latents [max_new, B, d]): like the
		reference's fresh tensors they stay valid whatever runs on the model afterwards."""
		c = self.cfg
		with self._session(0, lambda: self._gen_state(B, max_new, pipe_key, B, 0), arm=(0,), streamed=True) as (st, gen, off_start):
			hid = torch.empty((max_new, B, c.model_dim), device=self.device, dtype=torch.float32)
			# the yielded tokens get this call's lifetime too, as the reference's fresh tensors have (stream_generator.py:1172): `st.ids` belongs to the
			# cached generation state, which the next generation of the same shape -- streamed or not -- refills
			toks = torch.empty((max_new, B), device=self.device, dtype=torch.long)
			fast = self.use_graph and st.graphable and st.own_rng        # captured step; else the same launches issued eagerly
			n_done = 0
			self._streaming = True
			try:
				st.logits.copy_(self._prefill(cond, text, B))
				_lib.check(self.lib.ttk_ar_last_hidden(self._h, hid[0].data_ptr(), _lib.stream_ptr()), "ttk_ar_last_hidden")
				_lib.check(self.lib.ttk_ar_set_hidden_ring(self._h, hid.data_ptr(), st.col.data_ptr(), B * c.model_dim, _lib.stream_ptr()), "ttk_ar_set_hidden_ring")
				events, produced = [], 0
				while True:
					while produced < min(max_new, n_done + 1 + LAG):       # tokens n_done .. n_done + LAG sampled or in flight
						if produced == 0:
							st.sample(0)
							if st.rng_step is None:
								st.rng_step = gen.get_offset() - off_start       # what one torch-drawn token consumes (0 with the head-drawn noise)
						elif fast and st.stream_graph is not None:
							_lib.check(self.lib.ttk_graph_launch(st.stream_graph_exec, _lib.stream_ptr()), "ttk_graph_launch")
						elif fast and produced >= 2:
							# capture {decode_next into the ring; sample}: step 1 ran eagerly (warm kernels), the stream is idle of other work
							st.stream_graph = self._capture_step(st)
							st.stream_graph_exec = st.stream_graph.raw_cuda_graph_exec()
							continue
						else:
							self._decode_next(st.logits)
							st.sample(produced)
						ev = torch.cuda.Event()
						ev.record()
						events.append(ev)
						produced += 1
					events[n_done].synchronize()                               # token n_done and its flag are there
					toks[n_done].copy_(st.ids[:, n_done])
					yield toks[n_done], hid[n_done]
					n_done += 1
					end = int(st.done[0]) if can_stop else 0                   # tokens sampled when the last row finished (0: still running)
					if n_done >= max_new or (end and end <= n_done):
						return
			finally:
				self._streaming = False
				_lib.check(self.lib.ttk_ar_set_hidden_ring(self._h, None, None, 0, _lib.stream_ptr()), "ttk_ar_set_hidden_ring")
				# the generator where the reference's loop leaves it: one draw per token it produced (steps sampled ahead of an early end drew nothing
				# from torch; without the head-drawn noise they did, and are handed back)
				if st.own_rng:
					gen.set_offset(off_start + n_done * st.noise_step)
				elif st.rng_step:
					gen.set_offset(off_start + n_done * st.rng_step)


class _StopPoll:
	"""The late look at a device-written end-of-generation word: the loop records an event behind every step it enqueues and waits for the one LAG
	steps back, so the GPU always has work queued while the host reads a word that step has certainly written."""

	def __init__(self):
		self.events = []

	def step_complete(self) -> bool:
		"""call once behind each enqueued step; True when the step LAG back has completed (then its done word is visible)"""
		ev = torch.cuda.Event()
		ev.record()
		self.events.append(ev)
		if len(self.events) <= LAG:
			return False
		self.events.pop(0).synchronize()
		return True


class _NoiseState:
	"""What a generation state owns of the multinomial noise: torch's `q.exponential_(1)` restated inside the mel-head launch (include/ttk.h:
	ttk_ar_set_noise) -- one launch per token less.  Relied on (`own_rng`) only after a bitwise comparison with torch's own draw on this device, for the
	very [rows, cols] tensor torch would draw; TTK_AR_OWN_RNG=0 leaves the draw to torch."""

	def _init_noise(self, model: UnifiedVoice, rows, cols):
		self.model, self.noise_rows = model, rows
		self.rng = torch.zeros(6, dtype=torch.long, device=model.device)          # RngArgs {seed, offset0, threads, step, row0, candidates per line or 0}
		self.own_rng = os.environ.get("TTK_AR_OWN_RNG", "1") != "0" and self._noise_matches_torch(rows, cols)

	@staticmethod
	def _signed_seed(gen):
		"""the generator's seed as the int64 the C ABI takes"""
		seed = gen.initial_seed()
		return seed - (1 << 64) if seed >= (1 << 63) else seed

	def _noise_geometry(self, numel):
		"""(threads, offset step per draw) of ATen's launch for `exponential_()` on `numel` values (ATen/native/cuda/DistributionTemplates.h:
		distribution_nullary_kernel -- 256-thread blocks, a grid capped at the resident blocks of the device, four values per Philox call)"""
		props = torch.cuda.get_device_properties(self.model.device)
		grid = min(props.multi_processor_count * (props.max_threads_per_multi_processor // 256), (numel + 255) // 256)
		threads = 256 * grid
		return threads, ((numel - 1) // (threads * 4) + 1) * 4

	def _noise_matches_torch(self, rows, cols):
		dev = self.model.device
		gen = torch.cuda.default_generators[dev.index or 0]
		keep = gen.get_state()
		try:
			threads, step = self._noise_geometry(rows * cols)
			seed, off = self._signed_seed(gen), gen.get_offset()
			want = [torch.empty((rows, cols), device=dev).exponential_(1) for _ in range(2)]
			if gen.get_offset() - off != 2 * step:
				return False
			got = torch.empty((rows, cols), device=dev)
			for draw in range(2):
				_lib.check(self.model.lib.ttk_exponential_like_torch(got.data_ptr(), got.numel(), seed, off, threads, step, draw, _lib.stream_ptr()),
						   "ttk_exponential_like_torch")
				if not torch.equal(got.view(torch.int32), want[draw].view(torch.int32)):
					return False
			self.noise_threads, self.noise_step = threads, step
			return True
		finally:
			gen.set_state(keep)

	def _arm(self, gen, offset, row0, per_line, q: torch.Tensor):
		"""point the mel-head launches at q: draws numbered by the column counter `self.col`, the first one at generator offset `offset`"""
		self.rng.copy_(torch.tensor([self._signed_seed(gen), offset, self.noise_threads, self.noise_step, row0, per_line], dtype=torch.long))
		_lib.check(self.model.lib.ttk_ar_set_noise(self.model._h, self.rng.data_ptr(), self.col.data_ptr(), q.data_ptr()), "ttk_ar_set_noise")

	def disarm_noise(self):
		if self.own_rng:
			_lib.check(self.model.lib.ttk_ar_set_noise(self.model._h, None, None, None), "ttk_ar_set_noise")


class _GenState(_NoiseState):
	"""Persistent device buffers of one generation shape, so a captured token step can be replayed across calls (and across text
	lengths: nothing in it depends on the prefix length)."""

	def __init__(self, model: UnifiedVoice, B, max_new, pipe_key, C=None, lo=0, lines=1):
		c, dev = model.cfg, model.device
		C = B if C is None else C
		self.lines = lines                                              # lines > 1: B = lines * C rows, every line draws the same [C, V] noise
		self.B, self.max_new = B, max_new
		self.greedy = bool(pipe_key[6])                                 # greedy search: the argmax launch, no noise tensor, nothing armed, nothing drawn
		self.pipe = LogitsPipeline(temperature=pipe_key[0], top_k=pipe_key[1], top_p=pipe_key[2], repetition_penalty=pipe_key[3],
								   suppress_tokens=pipe_key[4], typical_mass=pipe_key[5], vocab=c.number_mel_codes, device=dev)
		self.stop = c.stop_mel_token
		self.logits = torch.empty((B, c.number_mel_codes), device=dev, dtype=torch.float32)
		self.ids = torch.empty((B, max_new), dtype=torch.long, device=dev)
		self.tok = torch.empty(B, dtype=torch.long, device=dev)
		self.unfinished = torch.ones(B, dtype=torch.long, device=dev)
		self.col = torch.zeros(B, dtype=torch.long, device=dev)         # per-row output column (all rows move together)
		# Exp(1) noise of multinomial for ALL C candidates of the call (C == B unless this is one shard of a candidate-sharded run:
		# every rank draws the same [C, V] block and reads its rows lo..lo+B-1, see inference_speech)
		self.q = None if self.greedy else torch.empty((B if lines > 1 else C, c.number_mel_codes), device=dev, dtype=torch.float32)
		self.qc = torch.empty((C, c.number_mel_codes), device=dev, dtype=torch.float32) if lines > 1 and not self.greedy else None      # torch-drawn fallback of a line batch
		self.live = torch.zeros(1, dtype=torch.int32, device=dev)        # unfinished rows, decremented on the device
		self.done = torch.zeros(1, dtype=torch.int32).pin_memory()       # raised by the row that finishes last; polled by the host
		self.rng_step = None                                             # generator offset consumed by one sample() call
		if self.greedy:
			self.model, self.own_rng = model, False                     # (`_session` arms and disarms the noise of states that own it)
		else:
			self._init_noise(model, C, c.number_mel_codes)
		# input_ids as the repetition penalty sees them: the fake prefix ids are all 1 with start_mel last (unified_voice.py:647-649),
		# i.e. the SET {1, start_mel} whatever the text length (the penalty acts once per distinct id), then the sampled tokens
		# the reference's samplers (SAMPLER_KNOBS): any of them on, and the token step is the second kernel's (ttk_ar_sample_next_ext); the decayed penalty and
		# the stop-length penalty read the history behind the two prefix ids, mirostat keeps one f64 surprise budget per row
		decay, stop_len, min_t, self.tau, eta = pipe_key[7:12]
		self.ext = None
		self.history = None
		if self.pipe.needs_history or decay != 0.0 or stop_len != 0.0:
			self.history = torch.ones((B, 2 + max_new), dtype=torch.long, device=dev)
		if tuple(pipe_key[7:12]) != NO_KNOBS:
			self.mu = torch.zeros(B, dtype=torch.float64, device=dev)
			x = _lib.SampleExt()
			x.repetition_penalty_decay, x.stop_length_penalty, x.min_temperature = decay, stop_len, -1.0 if min_t is None else min_t
			x.mirostat_tau, x.mirostat_eta, x.mirostat_mu = self.tau, eta, self.mu.data_ptr()
			self.ext = x
		# every processor and warper runs inside the fused kernel (V <= 9216: the row lives in registers), the typical-sampling warper included
		# (round 3).  With hf_exact_top_p the cumulative-mass warpers (top-p, typical) run as torch ops in front of it instead, in HF's order, which
		# means the processors then run as torch ops too and the kernel sees finished scores for that part
		p = self.pipe
		self.in_kernel = c.number_mel_codes <= 9216 and not (model.hf_exact_top_p and (p.top_p is not None or p.typical_mass is not None))
		self.graphable = self.in_kernel or not p.needs_history      # torch-op penalty: its history slice grows with the host's step count
		a = _lib.SampleArgs()
		a.ld, a.B, a.V = self.logits.stride(0), B, c.number_mel_codes
		if not self.greedy:
			a.q, a.ldq = self.q[lo].data_ptr(), self.q.stride(0)
		a.stop_token = self.stop
		a.unfinished, a.tok, a.ids = self.unfinished.data_ptr(), self.tok.data_ptr(), self.ids.data_ptr()
		a.ids_ld, a.ids_cols, a.col = self.ids.stride(0), self.ids.shape[1], self.col.data_ptr()
		if self.history is not None:
			a.history, a.hist_ld, a.hist_off = self.history.data_ptr(), self.history.stride(0), 2
		a.live_rows, a.all_done = self.live.data_ptr(), self.done.data_ptr()
		if self.in_kernel:
			a.scores = self.logits.data_ptr()
			a.suppress = _lib.ptr(p.suppress_mask)
			a.temperature = p.temperature or 1.0
			a.top_k, a.top_p, a.repetition_penalty = p.top_k or 0, p.top_p or 1.0, p.repetition_penalty or 1.0
			a.typical_mass = float(p.typical_mass or 0.0)
		else:
			a.temperature, a.top_k, a.top_p, a.repetition_penalty = 1.0, 0, 1.0, 1.0
		self.args = a
		self.graph = None
		self.graph_exec = None
		self.stream_graph = None          # the streaming generator's captured step (it also fills the hidden ring)
		self.stream_graph_exec = None

	def arm_noise(self, gen, lo, n0=0):
		"""point the mel-head launches of this call at q, starting from the generator's current state.  n0: id columns filled before the first draw (prompt
		tokens): the launches number their draws by the column counter, so the first offset is moved back by n0 draws"""
		self._arm(gen, gen.get_offset() - n0 * self.noise_step, lo, self.noise_rows if self.lines > 1 else 0, self.q[lo])

	def reset(self, c, prompt=None):
		self.ids.fill_(self.stop)
		self.unfinished.fill_(1)
		self.col.zero_()
		self.live.fill_(self.B)
		self.done.zero_()
		if self.ext is not None:
			self.mu.fill_(2.0 * self.tau)         # mirostat's max_surprise starts at 2 tau (samplers.py:133-134): a reused state never starts from the previous call's value
		if self.history is not None:
			self.history.fill_(1)
			self.history[:, 1] = c.start_mel_token
		if prompt is not None and prompt.shape[1]:      # a prompted continuation: the prompt tokens are the first id columns (and part of what the repetition penalty sees)
			n0 = prompt.shape[1]
			self.ids[:, :n0] = prompt
			self.col.fill_(n0)
			if self.history is not None:
				self.history[:, 2:2 + n0] = prompt

	def sample(self, n):
		"""one token from self.logits: process / warp, sample, pad finished rows, record, and write the next step's input row
		(HF:generation/utils.py:2894-2937; unified_voice.py:212-214)"""
		a = self.args
		if not self.in_kernel:
			hist = None if self.history is None else self.history[:, :2 + n]
			scores = self.pipe(hist, self.logits)
			self.scores = scores if scores.is_contiguous() else scores.contiguous()      # kept alive until the launch has run
			a.scores, a.ld = self.scores.data_ptr(), self.scores.stride(0)
		# multinomial(softmax(scores), 1) == argmax(softmax(scores) / q), q ~ Exp(1) from the torch generator (see sampling.multinomial1)
		# (own_rng: the mel-head launch that produced self.logits has written q already)
		if self.greedy:       # HF `_sample` without do_sample: argmax of the processed scores, nothing drawn
			_lib.check(self.model.lib.ttk_ar_greedy_next(self.model._h, _lib.C.byref(a), _lib.stream_ptr()), "ttk_ar_greedy_next")
			return
		if not self.own_rng:
			if self.lines > 1:
				self.qc.exponential_(1)
				self.q.view(self.lines, *self.qc.shape).copy_(self.qc)
			else:
				self.q.exponential_(1)
		if self.ext is not None:      # the reference's samplers: the same launch shape on the second kernel, its state (mu) in device memory -- capturable as the other
			_lib.check(self.model.lib.ttk_ar_sample_next_ext(self.model._h, _lib.C.byref(a), _lib.C.byref(self.ext), _lib.stream_ptr()), "ttk_ar_sample_next_ext")
			return
		_lib.check(self.model.lib.ttk_ar_sample_next(self.model._h, _lib.C.byref(a), _lib.stream_ptr()), "ttk_ar_sample_next")


class _BeamState(_NoiseState):
	"""Device state of one beam search (include/ttk.h: ttk_beam_args) and the noise arming of its flat [num_beams * V] multinomial.  lines = G > 1: the state
	of G searches stepped together (ttk_beam_step_lines), every array with a leading [G]."""

	def __init__(self, model: UnifiedVoice, N, max_new, kw, lines=1):
		c, dev = model.cfg, model.device
		V = c.number_mel_codes
		self.N, self.lines = N, lines
		G = lines
		self.logits = torch.empty((G * N, V), device=dev, dtype=torch.float32)
		self.q = torch.empty((G, N * V), device=dev, dtype=torch.float32)      # per line the tensor torch.multinomial draws its noise for: [batch 1, N * V]
		self.col = torch.zeros(G * N, dtype=torch.long, device=dev)
		self.seqs = torch.full((G, 2, 2, N, max_new), c.stop_mel_token, dtype=torch.long, device=dev)
		self.scores = torch.full((G, 2, N), -1e9, dtype=torch.float32, device=dev)
		self.scores[:, 0, 0] = 0.0
		self.state = torch.zeros((G, 2 * N + 2), dtype=torch.int32, device=dev)
		self.state[:, 2 * N] = 1
		self.acc = torch.empty(G * N * V, dtype=torch.float32, device=dev)
		self.work = torch.zeros((G, 4 * N * N + 2 * N + 1), dtype=torch.int32, device=dev)
		self.tok = torch.zeros(G * N, dtype=torch.long, device=dev)
		self.beam_idx = torch.arange(G * N, dtype=torch.long, device=dev)
		if G == 1:                                                              # one line: the arrays of ttk_beam_step, as `_beam_generate` reads them
			self.seqs, self.scores, self.state, self.work = self.seqs[0], self.scores[0], self.state[0], self.work[0]
		self.done = torch.zeros(1, dtype=torch.int32).pin_memory()
		self._init_noise(model, 1, N * V)
		suppress = tuple(kw.get("suppress_tokens") or ())
		self.suppress_mask = None
		if suppress:
			self.suppress_mask = torch.zeros(V, dtype=torch.uint8, device=dev)
			self.suppress_mask[list(suppress)] = 1
		a = _lib.BeamArgs()
		a.logits, a.ld, a.num_beams, a.V = self.logits.data_ptr(), self.logits.stride(0), N, V
		a.q, a.suppress = self.q.data_ptr(), _lib.ptr(self.suppress_mask)
		a.temperature = float(kw.get("temperature", 1.0) or 1.0)
		a.top_k = int(kw.get("top_k", 50) or 0)
		top_p, penalty = kw.get("top_p", 1.0), kw.get("repetition_penalty", 1.0)
		a.top_p = 1.0 if top_p is None else float(top_p)
		a.repetition_penalty = 1.0 if penalty is None else float(penalty)
		lp = kw.get("length_penalty", 1.0)
		a.length_penalty = 1.0 if lp is None else float(lp)
		a.stop_token = c.stop_mel_token
		a.prefix_ids[0], a.prefix_ids[1] = 1, c.start_mel_token      # the fake prefix ids are all 1 with start_mel last (unified_voice.py:647-649)
		a.max_new = max_new
		a.col, a.seqs, a.scores, a.state = self.col.data_ptr(), self.seqs.data_ptr(), self.scores.data_ptr(), self.state.data_ptr()
		a.acc, a.work, a.tok, a.beam_idx = self.acc.data_ptr(), self.work.data_ptr(), self.tok.data_ptr(), self.beam_idx.data_ptr()
		a.all_done = self.done.data_ptr()
		self.args = a

	def reset(self, c, prompt=None):
		"""(a beam state is built per call, in its start state)"""

	def arm_noise(self, gen):
		"""the mel-head launches of this search write q for their logits: N rows of V = the flat tensor, numbered by the step counter (several lines: groups
		of N rows, every line drawing the flat tensor of its own call)"""
		self._arm(gen, gen.get_offset(), 0, self.N if self.lines > 1 else 0, self.q)

	def reorder_cache(self):
		"""the KV cache follows the beams the step kept (`_reorder_cache`): inside every line when there are several"""
		m = self.model
		if self.lines > 1:
			_lib.check(m.lib.ttk_ar_reorder_cache_lines(m._h, self.beam_idx.data_ptr(), self.N, _lib.stream_ptr()), "ttk_ar_reorder_cache_lines")
			return
		_lib.check(m.lib.ttk_ar_reorder_cache(m._h, self.beam_idx.data_ptr(), _lib.stream_ptr()), "ttk_ar_reorder_cache")

	def step(self):
		if not self.own_rng:
			self.q[:1].exponential_(1)                   # one line's [1, N * V] draw ...
			if self.lines > 1:
				self.q[1:].copy_(self.q[:1].expand(self.lines - 1, -1))      # ... is every line's: each call of its own reseeds and draws the same
		if self.lines > 1:
			_lib.check(self.model.lib.ttk_beam_step_lines(_lib.C.byref(self.args), self.lines, _lib.stream_ptr()), "ttk_beam_step_lines")
			return
		_lib.check(self.model.lib.ttk_beam_step(_lib.C.byref(self.args), _lib.stream_ptr()), "ttk_beam_step")
