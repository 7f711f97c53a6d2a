"""`TTS` of the reference (inference.py:40-425), inference side, assembled from the libttk-backed parts: text -> tokens, reference clip ->
conditioning latents, then the hot path (AR sampling, latents, [CLVP], diffusion) and the vocoder, per line.  No config system, model
download, engine wrappers or file IO (out of scope) -- the parts are passed in, audio goes in and out as tensors.
"""
from __future__ import annotations

import random
import time
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import mel as M
from .inference import SAMPLE_RATE, TTSHotPath


def set_seed(seed=None) -> int:
	"""utils/utils.py:124-132."""
	if not seed:
		seed = int(time.time())
	random.seed(seed)
	np.random.seed(seed)
	torch.manual_seed(seed)
	return seed


def _collect_codes(pairs, sink):
	for codes, latent in pairs:
		sink.append(codes)
		yield codes, latent


class TTS:
	def __init__(self, autoregressive, diffusion, tokenizer, *, vocoder=None, clvp=None, conditioning_encoder=None, contextual_embedder=None,
				 tms: Optional[M.TorchMelSpectrogram] = None, stft: Optional[M.TacotronSTFT] = None, univnet=None, hifigan=None, dvae=None,
				 rlg_auto=None, rlg_diffuser=None, classifier=None):
		self.hot = TTSHotPath(autoregressive, diffusion, vocoder=vocoder, clvp=clvp)
		self.univnet = univnet          # tortoise_tts_amd.UnivNet: the vocoder of vocoder_type="vocoder"
		self.hifigan = hifigan          # tortoise_tts_amd.HiFiGAN: the vocoder of vocoder_type="hifigan" (AR latents -> audio, no diffusion)
		self.dvae = dvae                # tortoise_tts_amd.DiscreteVAE: `encode_audio` then returns the clip's mel codes as well (emb/mel.py:95)
		self.rlg_auto, self.rlg_diffuser = rlg_auto, rlg_diffuser      # tortoise_tts_amd.RandomLatentConverter pair: the voice of `references=None`
		self.classifier = classifier    # tortoise_tts_amd.AudioMiniEncoderWithClassifierHead: `classify_audio_clip`, the TorToiSe detector
		self.tokenizer = tokenizer
		self.conditioning_encoder, self.contextual_embedder, self.tms, self.stft = conditioning_encoder, contextual_embedder, tms, stft
		self.device = autoregressive.device

	def _adapter_model(self):
		ar = self.hot.autoregressive
		if not getattr(ar, "_adapters", False):
			raise NotImplementedError("the autoregressive model of this TTS was built without adapters=True (UnifiedVoice(..., adapters=True) or "
									  "load_autoregressive(..., adapters=True)): adapters cannot be attached, swapped or detached on it; a LoRA file given "
									  "at load time is folded into its weights")
		return ar

	def load_lora(self, name: str, path, scaling: Optional[float] = None):
		"""The LoRA block of the reference's `TTS.__init__` (inference.py:204-216) at any time: read the adapter file (or tensor dict) and keep it on the
		device under `name`; `enable_lora` attaches it."""
		self._adapter_model().load_lora(name, path, scaling=scaling)

	def enable_lora(self, enabled: Union[bool, str] = True):
		"""inference.py:99-101.  True: attach the only / last-loaded adapter; a name: attach that one; False: `disable_lora()`."""
		ar = self._adapter_model()
		if isinstance(enabled, str):
			return ar.enable_lora(enabled)
		return ar.enable_lora() if enabled else ar.disable_lora()

	def disable_lora(self):
		"""inference.py:103-104: the base voice again, bit for bit."""
		self._adapter_model().disable_lora()

	def encode_text(self, text: Union[str, torch.Tensor], language: str = "en") -> torch.Tensor:
		"""inference.py:104-111 over `tokenize` (data.py:279-282: a list of pieces is joined first)."""
		if isinstance(text, torch.Tensor):
			return text
		if isinstance(text, list):
			text = "".join(text)
		return torch.tensor(self.tokenizer.encode(text), dtype=torch.int64)

	def encode_audio(self, wav: Union[dict, torch.Tensor, Sequence[torch.Tensor]], sr: int = 22050) -> dict:
		"""inference.py:113-124 over emb/mel.py:84-137 (`encode` / `encode_from_files`): a mono clip [1, n] (or a list of them, concatenated
		in time like `encode_from_files`) -> {"conds", "latent", "metadata"}; a dict produced earlier is passed through.  Built with `dvae=`, the
		dict also has "codes": the mel codes [1, F4] of the clip, or for a list of clips a list with one entry per clip (emb/mel.py:95; each clip stays usable as a
		continuation prompt of its own, where the reference codes the concatenation)."""
		if isinstance(wav, dict):
			return wav
		if any(p is None for p in (self.tms, self.stft, self.conditioning_encoder, self.contextual_embedder)):
			raise ValueError("TTS was built without the conditioning parts (tms, stft, conditioning_encoder, contextual_embedder)")
		clips = None
		if not isinstance(wav, torch.Tensor):
			clips = [w[:1] if w.dim() == 2 else w[None] for w in wav]
			wav = torch.cat(clips, dim=-1)
		if wav.dim() == 1:
			wav = wav[None]
		parts = dict(tms=self.tms, stft=self.stft, conditioning_encoder=self.conditioning_encoder, contextual_embedder=self.contextual_embedder)
		out = M.encode(wav[:1], sr, dvae=None if clips is not None else self.dvae, **parts)
		if clips is not None and self.dvae is not None:
			codes = [self.dvae.get_codebook_indices(M.format_autoregressive_conditioning(M.resample(c, sr, 22050, device=str(self.tms.device)), self.tms, cond_length=0))
					 for c in clips]
			out = {"codes": codes, **out}
		return out

	def random_voice(self, rows: int = 1) -> dict:
		"""TorToiSe's random voices (the reference's `rlg` pair, models/__init__.py:97-103): {"latent": (ar_latent [rows, C_ar], diff_latent
		[rows, C_diff])} drawn from the default device generator, the autoregressive latent first, then the diffusion one -- the original order.
		`encode_audio` passes the dict through, so it can be kept and given as `references` again."""
		if self.rlg_auto is None or self.rlg_diffuser is None:
			raise ValueError("TTS was built without the random latent converters (rlg_auto=, rlg_diffuser=)")
		ref = torch.empty((int(rows), 0))
		ar_latent = self.rlg_auto(ref)
		return {"latent": (ar_latent, self.rlg_diffuser(ref))}

	@torch.inference_mode()
	def classify_audio_clip(self, clip: torch.Tensor, sr: int = 24000) -> float:
		"""Upstream's `classify_audio_clip`: the probability that a clip ([1, T] or [T], resampled to 24 kHz when `sr` differs) was generated by
		TorToiSe -- `softmax(logits)[0][0]` of the detector passed as `classifier=`."""
		if self.classifier is None:
			raise ValueError("TTS was built without the TorToiSe detector (classifier=)")
		if clip.dim() == 1:
			clip = clip[None]
		clip = clip[:1].to(torch.float32)
		if int(sr) != 24000:
			clip = M.resample(clip, int(sr), 24000, device=str(self.classifier.device))
		logits = self.classifier(clip[None])
		return float(torch.softmax(logits, dim=-1)[0][0])

	@torch.inference_mode()
	def inference(self, text: str, references=None, max_ar_steps=500, max_diffusion_steps=80, ar_temp=0.8, diffusion_temp=1.0, top_p=1.0, top_k=0,
				  repetition_penalty=1.0, length_penalty=1.0, beam_width=1, diffusion_sampler="ddim", cond_free=True, vocoder_type="bigvgan",
				  seed=None, candidates=1, references_sr: int = 22050, do_sample=True, *, diffusion_eta=0.0, min_ar_temp=None, repetition_penalty_decay=0.0,
				  stop_length_penalty=0.0, mirostat_tau=0.0, mirostat_eta=0.1, return_timings=False,
				  alignment_heads=None) -> Union[Tuple[torch.Tensor, int], Tuple[torch.Tensor, int, list]]:
		"""inference.py:142-425: every line of `text` spoken in the voice of `references` (clip tensor(s), or the dict `encode_audio` returns) ->
		(wav [1, 1, samples] -- the lines concatenated in time -- , 24000).  vocoder_type "bigvgan" runs the `vocoder=` part, "vocoder" the
		`univnet=` part (see `_univnet_wav` for its noise), "hifigan" the `hifigan=` part on the AR latents as they are sampled, without the
		diffusion model (see `_hifigan_wav`; the reference returns [1, samples] on that branch, here the shape is that of the other two).
		beam_width > 1 (inference.py:342: num_beams) samples every line by beam search -- `candidates` <= beam_width finished beams come back, ranked
		with `length_penalty` -- on the "bigvgan" and "vocoder" branches; several lines are searched together as one decode batch (TTSHotPath.inference_lines), each
		line's result what its own search gives; the streaming "hifigan" branch takes no beams.
		references=None speaks in a random voice (`random_voice`; needs `rlg_auto=` and `rlg_diffuser=`): `set_seed(seed)` then runs BEFORE the voice
		is drawn, so `seed` fixes the voice, and once more behind it, so the line is sampled as `inference(text, that_voice, seed=seed)` samples it.
		With references given the order is the reference's: the clip is encoded first, then the seed is set.
		do_sample (the reference's `TTS.inference` has no such argument: it always samples, inference.py:336): False speaks every line by greedy search -- the
		mel codes are then a pure function of (voice, text, weights), whatever `ar_temp`, `top_k`, `top_p` and `seed` are; `seed` still fixes the diffusion
		noise.  Needs candidates == 1 and beam_width == 1 (ValueError); not available with vocoder_type="hifigan", whose token generator always samples.
		diffusion_eta (keyword only; DDIM's eta, diffusion.py:745, which the reference's `TTS.inference` leaves at 0): above 0 the sampler reads its
		per-step noise -- 1.0 is the DDPM-variance sampler -- so the same text and voice render differently per `seed`; 0.0 is the call without it, bit
		for bit.  The ancestral sampler ignores it; the "hifigan" branch has no diffusion.
		diffusion_sampler: "ddim", "p" (the reference's two), or "dpm++2m": DPM-Solver++(2M), a second-order multistep solver meant for fewer
		`max_diffusion_steps` (SpacedDiffusion.sample_loop; the default sampler and step count are unchanged).  It is deterministic: diffusion_eta != 0 with it is
		a ValueError.  Several lines go through `TTSHotPath.inference_lines` as they do for DDIM.
		min_ar_temp, repetition_penalty_decay, mirostat_tau, mirostat_eta (keyword only; the arguments the reference's `inference` keeps commented out,
		inference.py:154-163, for the samplers of its tortoise_tts/samplers.py) and stop_length_penalty (its length_penalize; `length_penalty` is HF's beam
		ranking): the dynamic temperature's lower end, the distance decay of `repetition_penalty`, mirostat v1's target surprise and learning rate, the power
		of the length that divides the stop token's score (> 0 longer lines).  Off by default (None, 0, 0, 0.1, 0): the call without them, bit for bit.  They
		act on the sampling branch on every vocoder branch; not with beam_width > 1 or do_sample=False (see `UnifiedVoice.inference_speech`).
		return_timings (keyword; no reference counterpart): True returns (wav, 24000, timings) -- one list of (word, start_s, end_s) per line, from
		`UnifiedVoice.text_alignment` (heads: `alignment_heads`, a list of (layer, head); None = its default set) on the line's chosen code row as it was sampled,
		before the stop-token rewrite; a word is a run of tokens between `[SPACE]` tokens, seconds = code index * mel_length_compression / 22050.  Entries are
		clipped to the line's audio length (what the calm-token trim left of it) and offset by the samples of the lines before it.  Available on all three vocoder
		branches: "bigvgan" / "vocoder" align behind each line's latent pass (`TTSHotPath.inference` / `inference_lines`), "hifigan" runs one dense pass on the
		streamed codes after the line's stream has ended.  `self.last_alignments` then holds, per line, the `text_alignment` dict plus "codes" (the aligned row
		[1, M]): `align(line, codes, voice)` gives that line's entries without clip and offset.  wav and sr are bit for bit those of the call without the
		argument, which issues the launches it always did."""
		from .inference import check_greedy, check_sampler_eta
		knobs = dict(min_ar_temp=min_ar_temp, repetition_penalty_decay=repetition_penalty_decay, stop_length_penalty=stop_length_penalty, mirostat_tau=mirostat_tau,
					 mirostat_eta=mirostat_eta)
		check_greedy(do_sample, candidates, beam_width)
		check_sampler_eta(diffusion_sampler, diffusion_eta)
		if vocoder_type not in ("bigvgan", "vocoder", "hifigan"):
			raise NotImplementedError(f"vocoder_type {vocoder_type!r} is unknown ('bigvgan', 'vocoder', 'hifigan')")
		if not do_sample and vocoder_type == "hifigan":
			raise NotImplementedError("greedy search (do_sample=False) is not available on the HiFiGAN streaming branch: the reference's streaming generator draws every token "
									  "(stream_generator.py:1161)")
		if vocoder_type == "hifigan" and self.hifigan is None:
			raise NotImplementedError("TTS was built without a HiFiGAN vocoder (hifigan=): the streaming branch, inference.py:250-329, needs one")
		beam_width = max(1, int(beam_width))                  # inference.py:342
		if beam_width != 1 and vocoder_type == "hifigan":
			raise NotImplementedError("beam search is not available on the HiFiGAN streaming branch: its token generator yields one sequence as it is sampled (beam_width=1)")
		if vocoder_type == "hifigan":
			pass
		elif vocoder_type == "vocoder":
			if self.univnet is None:
				raise ValueError("TTS was built without a UnivNet vocoder (univnet=)")
		elif self.hot.vocoder is None:
			raise ValueError("TTS was built without a vocoder")
		if references is None:
			seed = set_seed(seed)
			references = self.random_voice()
		ar_latent, diff_latent = self.encode_audio(references, references_sr)["latent"]
		set_seed(seed)
		lines = []
		for line in text.split("\n"):
			tokens = self.encode_text(line).to(self.device)[None]
			if tokens.shape[1] == 0:
				raise ValueError("empty line (the reference fails inside the embedding here)")
			lines.append(tokens)
		align_kw = dict(return_timings=True, alignment_heads=alignment_heads) if return_timings else {}
		if vocoder_type == "hifigan":
			wavs, alignments = [], []
			for tokens in lines:
				streamed = [] if return_timings else None
				wavs.append(self._hifigan_wav(tokens, ar_latent, max_ar_steps=max_ar_steps, ar_temp=ar_temp, top_p=top_p, top_k=top_k,
											  repetition_penalty=repetition_penalty, length_penalty=length_penalty, codes_out=streamed, **knobs))
				if return_timings:      # one dense pass on the streamed codes, after the stream has ended
					from .inference import line_alignment
					alignments.append(line_alignment(self.hot.autoregressive, ar_latent, tokens, torch.stack(streamed, dim=1), 0, alignment_heads))
			return self._with_timings(torch.concat(wavs, dim=-1), wavs, lines, alignments) if return_timings else (torch.concat(wavs, dim=-1), SAMPLE_RATE)
		kw = dict(max_ar_steps=max_ar_steps, max_diffusion_steps=max_diffusion_steps, ar_temp=ar_temp, diffusion_temp=diffusion_temp, top_p=top_p, top_k=top_k,
				  repetition_penalty=repetition_penalty, length_penalty=length_penalty, cond_free=cond_free, candidates=candidates, do_sample=do_sample,
				  diffusion_eta=diffusion_eta, **knobs, **align_kw)
		to_wav = self._univnet_wav if vocoder_type == "vocoder" else self.hot.vocoder.inference     # a line's mel [1, 100, T] -> its waveform
		if len(lines) > 1 and diffusion_sampler in ("ddim", "dpm++2m"):
			# several lines: their sampling as one decode batch -- beam_width > 1: the beams of a line exchange histories among themselves, the lines of a batch are
			# searched together -- , the diffusion of a line under the sampling of later ones (TTSHotPath.inference_lines: the same waveforms as the line-by-line
			# loop of inference.py:237-422, which is what the else branch runs)
			res = self.hot.inference_lines(lines, ar_latent, diff_latent, diffusion_sampler=diffusion_sampler, beam_width=beam_width, **kw)
		else:
			res = [self.hot.inference(tokens, ar_latent, diff_latent, diffusion_sampler=diffusion_sampler, beam_width=beam_width, **kw) for tokens in lines]
		wavs = [to_wav(r[0]) for r in res]
		wav = torch.concat(wavs, dim=-1)
		return self._with_timings(wav, wavs, lines, [r[-1] for r in res]) if return_timings else (wav, SAMPLE_RATE)

	def _with_timings(self, wav, wavs, lines, alignments):
		"""(wav, 24000, timings): each line's alignment as words, clipped to the line's audio and offset by the samples before it"""
		from . import alignment as AL
		self.last_alignments = alignments
		timings, offset = [], 0
		for tokens, w, r in zip(lines, wavs, alignments):
			t = AL.word_timings(self.tokenizer, tokens[0].tolist(), r["token_start"][0], r["codes"].shape[1], self.hot.autoregressive.mel_length_compression)
			timings.append(AL.clip_and_offset(t, w.shape[-1] / SAMPLE_RATE, offset / SAMPLE_RATE))
			offset += w.shape[-1]
		return wav, SAMPLE_RATE, timings

	def _word_timings(self, tokens: torch.Tensor, codes: torch.Tensor, ar_latent: torch.Tensor, heads=None, median_width: int = 7):
		"""[(word, start_s, end_s)] of one line: tokens [1, Tt], codes [1, M]"""
		from . import alignment as AL
		ar = self.hot.autoregressive
		r = ar.text_alignment(ar_latent, tokens, codes, heads=heads, median_width=median_width)
		return AL.word_timings(self.tokenizer, tokens[0].tolist(), r["token_start"][0], codes.shape[1], ar.mel_length_compression)

	@torch.inference_mode()
	def align(self, text_line: Union[str, torch.Tensor], codes: torch.Tensor, references=None, *, references_sr: int = 22050, alignment_heads=None, median_width: int = 7):
		"""Word timings of mel codes that exist already (for `decode_codes` / `resynthesize` users, or the "codes" of `last_alignments`): [(word, start_s, end_s)] of ONE
		line of text against codes [1, M] (or [M]), seconds = code index * mel_length_compression / 22050, in the voice of `references` (clip tensor(s) or an
		`encode_audio` dict; None: a random voice from the current generator state).  See `UnifiedVoice.text_alignment`; `alignment_heads` is its `heads`."""
		if isinstance(text_line, str) and "\n" in text_line:
			raise ValueError("align takes one line of text: lines of different length are aligned one call each")
		tokens = self.encode_text(text_line).to(self.device)
		tokens = tokens[None] if tokens.dim() == 1 else tokens
		codes = torch.as_tensor(codes)
		codes = codes[None] if codes.dim() == 1 else codes
		if tokens.shape[1] == 0 or codes.dim() != 2 or codes.shape[0] != 1 or codes.shape[1] == 0:
			raise ValueError("align: one non-empty line of text and codes [1, M]")
		if references is None:
			references = self.random_voice()
		ar_latent = self.encode_audio(references, references_sr)["latent"][0]
		return self._word_timings(tokens, codes.to(self.device), ar_latent, alignment_heads, median_width)

	@torch.inference_mode()
	def decode_codes(self, codes, references=None, *, max_diffusion_steps=80, diffusion_temp=1.0, diffusion_sampler="ddim", cond_free=True,
					 vocoder_type="bigvgan", seed=None, references_sr: int = 22050, diffusion_eta=0.0) -> Tuple[torch.Tensor, int]:
		"""Mel codes -> waveform without the autoregressive model: the diffusion model's token branch (diffusion.py:1493-1497) on `codes`, the sampler and
		the vocoder as in `inference`.  codes: [1, M] integers (what `encode_audio(...)["codes"]` or the AR sampling give), or a list of such rows --
		the rows' waveforms come back concatenated in time, each what its own call with the same `seed` gives; with the DDIM sampler and conditioning-free guidance several
		rows are diffused as one ragged batch (SpacedDiffusion.sample_loop_lines).  The voice is the diffusion latent of `references` (clip tensor(s) or an
		`encode_audio` dict), or a random voice when None, seeded as in `inference`.  T = M * 4 * 24000 // 22050 frames per row (inference.py:400).
		diffusion_eta: DDIM's eta as in `inference`; above 0 every row diffuses in a loop of its own.
		diffusion_sampler: as in `inference`; with "dpm++2m" a row draws its start noise only, several rows diffuse as one ragged batch, and diffusion_eta != 0 is a ValueError.
		Returns (wav [1, 1, samples], 24000).  vocoder_type "bigvgan" or "vocoder"; "hifigan" is refused: it reads AR latents, which codes alone do not give."""
		from .diffusion import denormalize_tacotron_mel, get_diffuser
		from .inference import check_diffusion_conditioning, check_sampler_eta
		check_sampler_eta(diffusion_sampler, diffusion_eta)
		if vocoder_type == "hifigan":
			raise NotImplementedError("decode_codes cannot use vocoder_type='hifigan': HiFiGAN turns the autoregressive model's latents into audio (inference.py:250-329), "
									  "and mel codes alone do not give those; use 'bigvgan' or 'vocoder'")
		if vocoder_type not in ("bigvgan", "vocoder"):
			raise NotImplementedError(f"vocoder_type {vocoder_type!r} is unknown ('bigvgan', 'vocoder')")
		if vocoder_type == "vocoder":
			if self.univnet is None:
				raise ValueError("TTS was built without a UnivNet vocoder (univnet=)")
		elif self.hot.vocoder is None:
			raise ValueError("TTS was built without a vocoder")
		diff = self.hot.diffusion
		check_diffusion_conditioning("codes", diff)
		rows = [codes] if isinstance(codes, torch.Tensor) else list(codes)
		rows = [r[None] if r.dim() == 1 else r for r in rows]
		if not rows or any(r.dim() != 2 or r.shape[0] != 1 or r.shape[1] == 0 or r.dtype.is_floating_point for r in rows):
			raise ValueError("codes: an integer tensor [1, M], or a list of such rows")
		if references is None:
			seed = set_seed(seed)
			references = self.random_voice()
		diff_latent = self.encode_audio(references, references_sr)["latent"][1]
		seed = set_seed(seed)
		diffuser = get_diffuser(steps=max_diffusion_steps, cond_free=cond_free)
		eta = float(diffusion_eta)
		prepared = []
		for r in rows:
			# every row draws from the generators as `seed` leaves them -- the start noise, then DDIM's ignored per-step draws (diffusion.py:685) -- so a row of a
			# list is what its own call gives (`inference` has the same property: the reference reseeds per line, stream_generator.py:296)
			set_seed(seed)
			T = r.shape[1] * 4 * 24000 // 22050
			E = diff.timestep_independent(r.to(self.device), diff_latent, T, False)
			noise = torch.randn((1, 100, T), device=self.device) * diffusion_temp
			step_noise = None
			if diffusion_sampler == "ddim" and eta != 0.0:      # ... which are read then
				step_noise = torch.stack([torch.randn_like(noise) for _ in range(diffuser.num_timesteps)])
			elif diffusion_sampler == "ddim":
				for _ in range(diffuser.num_timesteps):
					torch.randn_like(noise)
			prepared.append((E, noise, T, step_noise))
		if len(prepared) > 1 and diffusion_sampler in ("ddim", "dpm++2m") and cond_free and eta == 0.0:
			mels = diffuser.sample_loop_lines(diff, [n for _, n, _, _ in prepared], [E for E, _, _, _ in prepared], sampler=diffusion_sampler)
		else:
			mels = [diffuser.sample_loop(diff, (1, 100, T), sampler=diffusion_sampler, noise=n, model_kwargs={"precomputed_aligned_embeddings": E},
										 progress=False, eta=eta, step_noise=sn, consume_rng=diffusion_sampler != "ddim") for E, n, T, sn in prepared]
		to_wav = self._univnet_wav if vocoder_type == "vocoder" else self.hot.vocoder.inference
		return torch.concat([to_wav(denormalize_tacotron_mel(m)) for m in mels], dim=-1), SAMPLE_RATE

	def resynthesize(self, wav, sr: int = 22050, references=None, **kw) -> Tuple[torch.Tensor, int]:
		"""A clip -> its mel codes (`encode_audio`, needs `dvae=`) -> waveform (`decode_codes`): the round trip through the 8192-way code stream.
		references=None speaks in the source clip's own voice; else in that of `references`.  `kw` goes to `decode_codes`."""
		if self.dvae is None:
			raise ValueError("TTS was built without a DiscreteVAE (dvae=): resynthesize needs the clip's mel codes")
		enc = self.encode_audio(wav, sr)
		if "codes" not in enc:
			raise ValueError("the voice dict holds no mel codes: pass the clip, or a dict that `encode_audio` made with dvae=")
		if references is None:
			references = enc
		return self.decode_codes(enc["codes"], references, **kw)

	def _univnet_wav(self, mels: torch.Tensor) -> torch.Tensor:
		"""UnivNet on one line's mel [1, 100, T] with the noise the reference draws for that line: `generate` reseeds every generator to 0 per
		line (`setup_seed(0)`, stream_generator.py:36-45, 296), nothing after it draws from the CPU generator (AR sampling and the diffusion noise
		use the device one), so `vocoder.inference`'s `torch.randn` (models/vocoder.py:309) is the first draw after `torch.manual_seed(0)`.
		The batched-lines path does not reseed per line, so the draw is made here from a generator in that state, on every path."""
		z = self.univnet.draw_noise(mels.shape[0], mels.shape[-1], generator=torch.Generator().manual_seed(0))
		return self.univnet.inference(mels, z)

	def hifigan_chunks(self, tokens: torch.Tensor, ar_latent: torch.Tensor, *, max_ar_steps=500, ar_temp=0.8, top_p=1.0, top_k=0, repetition_penalty=1.0,
					   length_penalty=1.0, min_ar_temp=None, repetition_penalty_decay=0.0, stop_length_penalty=0.0, mirostat_tau=0.0, mirostat_eta=0.1, codes_out=None):
		"""One line of the HiFiGAN branch (inference.py:250-320) as a generator of waveform chunks [1, samples]: `compute_embeddings` ->
		`get_generator` -> `HiFiGAN.stream`.  The first chunk is there after 60 tokens, while sampling goes on.  `max_length` is
		min(500, prefix + max_ar_steps): the reference hard-codes 500 in total (stream_generator defaults) and ignores `max_ar_steps`; the
		default call is the same.  min_ar_temp ... mirostat_eta: the reference's own samplers, as in `inference`; off by default.
		codes_out: a list that receives every streamed code tensor [1] as it is yielded (views of the generator's own buffer: no launch is added)."""
		from .inference import ar_sampler_knobs
		ar = self.hot.autoregressive
		inputs = ar.compute_embeddings(ar_latent, tokens)
		pairs = ar.get_generator(inputs=inputs, max_length=min(500, inputs.shape[1] + max_ar_steps), top_k=top_k, top_p=top_p, temperature=ar_temp,
								 do_sample=True, num_return_sequences=1, length_penalty=length_penalty, repetition_penalty=repetition_penalty,
								 **ar_sampler_knobs(min_ar_temp, repetition_penalty_decay, stop_length_penalty, mirostat_tau, mirostat_eta))
		if codes_out is not None:
			pairs = _collect_codes(pairs, codes_out)
		chunks = self.hifigan.stream(pairs, ar_latent)
		while True:
			with torch.inference_mode():      # per step, not around the yield: the consumer's own mode is its own between two chunks
				try:
					chunk = next(chunks)
				except StopIteration:
					return
			yield chunk

	def _hifigan_wav(self, tokens: torch.Tensor, ar_latent: torch.Tensor, **kw) -> torch.Tensor:
		"""a line's chunks concatenated, [1, 1, samples].  `candidates` and `max_diffusion_steps` play no part (one sequence, no diffusion), nor
		does `seed`: the token loop reseeds to 0 per line (stream_generator.py:36-45, 296) and nothing else draws."""
		return torch.concat(list(self.hifigan_chunks(tokens, ar_latent, **kw)), dim=-1)[None]
