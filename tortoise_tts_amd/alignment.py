"""Host side of the text-to-audio alignment (`UnifiedVoice.text_alignment`, `TTS.inference(return_timings=True)`, `TTS.align`): the backtrace of the
DTW trace that csrc/align.hip writes, token starts, and words with their times.  No reference counterpart: the reference hands out the attention maps
(models/unified_voice.py:508-516) and stops there; the recipe is OpenAI Whisper's word-timestamp recipe with mel codes as the time axis.  Pure numpy and
Python: nothing here touches the device.

Definitions.  The path runs from (mel 0, text 0) to (mel M - 1, text Tt - 1) in steps that raise the mel index, the text index or both by one, so every
text token lies on it.  The start of text token t is the first mel index on the path whose text index is t.  A word is a maximal run of tokens between
`[SPACE]` tokens; it starts at its first token's start and ends at the start of the first token behind it (the `[SPACE]`, or M for the last word).
seconds = mel index * mel_length_compression / 22050."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

AR_SAMPLE_RATE = 22050      # the rate mel_length_compression counts samples at (unified_voice.py:501)


def backtrace(trace: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
	"""trace u8 [M, Tt] (0 diagonal, 1 mel row - 1, 2 text column - 1: include/ttk.h, ttk_dtw) -> (text indices, mel indices) of the path, rising"""
	trace = np.asarray(trace)
	i, j = trace.shape
	text, mel = [], []
	while i > 0 and j > 0:
		text.append(j - 1)
		mel.append(i - 1)
		t = int(trace[i - 1, j - 1])
		if t == 0:
			i, j = i - 1, j - 1
		elif t == 1:
			i -= 1
		else:
			j -= 1
	return np.asarray(text[::-1], dtype=np.int64), np.asarray(mel[::-1], dtype=np.int64)


def token_starts(text_idx: np.ndarray, mel_idx: np.ndarray, n_text: int) -> np.ndarray:
	"""int64 [n_text]: the first mel index on the path whose text index is t (-1 for a token the path does not visit: a trace that left the table)"""
	out = np.full(n_text, -1, dtype=np.int64)
	for t, m in zip(text_idx.tolist(), mel_idx.tolist()):
		if out[t] < 0:
			out[t] = m
	return out


def default_heads(layers: int, heads: int) -> List[Tuple[int, int]]:
	"""every head of layers >= layers / 2"""
	return [(l, h) for l in range(layers // 2, layers) for h in range(heads)]


def words_from_tokens(tokenizer, ids: Sequence[int]) -> List[Tuple[str, int, int]]:
	"""[(word, first token index, index of the first token behind the word)] for the maximal runs of tokens between `[SPACE]` tokens; leading, doubled and
	trailing spaces make no words"""
	space = tokenizer.get_vocab().get("[SPACE]")
	ids = [int(i) for i in ids]
	words, start = [], None
	for k, tok in enumerate(ids + [space]):
		if tok == space or k == len(ids):
			if start is not None:
				words.append((tokenizer.decode(ids[start:k]), start, k))
			start = None
		elif start is None:
			start = k
	return words


def word_timings(tokenizer, ids: Sequence[int], token_start: Sequence[int], n_codes: int, mel_length_compression: int = 1024,
				 sample_rate: int = AR_SAMPLE_RATE) -> List[Tuple[str, float, float]]:
	"""[(word, start seconds, end seconds)]: token_start [len(ids)] in mel-code units, n_codes = M"""
	per_code = mel_length_compression / sample_rate
	out = []
	for word, a, b in words_from_tokens(tokenizer, ids):
		end = int(token_start[b]) if b < len(ids) else int(n_codes)
		out.append((word, int(token_start[a]) * per_code, end * per_code))
	return out


def clip_and_offset(timings: List[Tuple[str, float, float]], line_seconds: float, offset_seconds: float) -> List[Tuple[str, float, float]]:
	"""a line's timings clipped to its audio length and moved behind the lines before it"""
	return [(w, min(s, line_seconds) + offset_seconds, min(e, line_seconds) + offset_seconds) for w, s, e in timings]
