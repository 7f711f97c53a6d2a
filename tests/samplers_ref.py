"""The reference's samplers (tortoise_tts/samplers.py: reptition_penalize :11-29, length_penalize :35-40, dynamic_temperature :78-91, mirostat_sample :117-158)
restated the way csrc/sample_ext.hip: k_sample_step_ext runs them: numpy f32 where the device computes in f32 (the scores, the softmax), Python floats (f64)
where the reference computes with Python floats (the divisors, T_dyn, mirostat's k and state).  Parameters are taken as given: a caller that compares with the
device passes them rounded to f32 (`f32(x)`), which is what the C ABI carries.

`token_step` is the whole chain of one token for a batch of rows, in the kernel's order: penalty (HF's, or the decayed one), stop-length penalty, suppress,
temperature (plain or dynamic), top-k, then the draw argmax(softmax / q) -- or mirostat's.  top-p and the typical warper are not restated here (the tests that
use them compare the device with ttk_sample_step_warped)."""
import math

import numpy as np

F32 = np.float32
MIRO_N = 100


def f32(x):
	"""a parameter as the C ABI carries it"""
	return float(np.float32(x))


def recip_mul(score, divisor):
	"""ATen's GPU form of `tensor / python_scalar`: x * (1 / s) with the reciprocal rounded to f32 (the device's form; the CPU reference divides)"""
	return F32(score) * (F32(1.0) / F32(divisor))


def latest_distances(previous):
	"""{token: 1 + the number of tokens behind its most recent occurrence} -- what `reversed(previous)` with one_time=True visits"""
	out = {}
	n = len(previous)
	for i, t in enumerate(previous):
		out[int(t)] = n - i
	return out


def decay_penalize(scores, previous, factor, decay):
	"""reptition_penalize(one_time=True): scores f32 [V] (a copy is returned); previous: the tokens behind the prefix ids"""
	s = np.array(scores, dtype=F32)
	if factor == 1.0:
		return s
	for t, d in latest_distances(previous).items():
		if 0 <= t < s.shape[0]:
			s[t] = recip_mul(s[t], float(factor) * float(d) ** float(decay))
	return s


def hf_penalize(scores, input_ids, penalty):
	"""HF's RepetitionPenaltyLogitsProcessor in the kernel's form: every distinct id of input_ids (prefix ids included), < 0 multiplied, else divided"""
	s = np.array(scores, dtype=F32)
	if penalty == 1.0:
		return s
	for t in set(int(t) for t in input_ids):
		if 0 <= t < s.shape[0]:
			s[t] = s[t] * F32(penalty) if s[t] < 0 else s[t] * (F32(1.0) / F32(penalty))
	return s


def stop_length_penalize(scores, length, factor, stop_token):
	"""length_penalize: length = len(previous) + 1"""
	s = np.array(scores, dtype=F32)
	if factor != 0.0 and 0 <= stop_token < s.shape[0]:
		s[stop_token] = recip_mul(s[stop_token], float(length) ** float(factor))
	return s


def dynamic_temperature_value(scores, temperature, min_temperature, k=10, centre=0.5):
	"""T_dyn of one row, in f64 as the reference's Python loop computes it (the device sums the exponentials in f32: within ~1e-6 of this)"""
	s = np.asarray(scores, dtype=F32)
	sum_exp = float(np.exp((s - s.max()).astype(np.float64)).sum())
	p_max = 1.0 / sum_exp
	return temperature - (temperature - min_temperature) / (1 + math.exp(-k * (p_max - centre)))


def softmax_f32(scores):
	s = np.asarray(scores, dtype=F32)
	e = np.exp(s - s.max())
	return e, e / e.sum(dtype=F32)


def mirostat_k_unrounded(p_sorted, n, mu):
	"""compute_k (samplers.py:118-131) before the rounding: p_sorted = the 101 largest probabilities, descending (f32 values, used as Python floats)"""
	prob = [float(x) for x in p_sorted]
	num = den = 0
	for i in range(MIRO_N):
		b = prob[i] / prob[i + 1]
		t = (i + 2) / (i + 1)
		num += math.log(b) * math.log(t)
		den += math.log(t) ** 2
	s = num / den
	eps = s - 1
	return ((eps * (2 ** mu)) / (1 - n ** (-eps))) ** (1 / s)


def mirostat_k(p_sorted, n, mu):
	"""the reference's k (`compute_k(...) + 1`), clamped to [1, n]; whatever Python cannot round (nan, inf, a complex power) is n, as on the device"""
	try:
		ku = mirostat_k_unrounded(p_sorted, n, mu)
		k = round(ku) + 1
	except (ValueError, OverflowError, TypeError, ZeroDivisionError):
		return n, float("nan")
	return min(max(k, 1), n), ku


def mirostat_update(mu, p_token, tau, eta):
	"""max_surprise after a token of probability p_token (under the softmax of the whole row) was drawn"""
	return mu - eta * (math.log2(1 / float(p_token)) - tau)


def keep_top(scores, k):
	"""scores below the k-th largest become -inf (a group of equal scores at the threshold stays whole)"""
	s = np.array(scores, dtype=F32)
	if 0 < k < s.shape[0]:
		kth = np.sort(s)[-k]
		s[s < kth] = -np.inf
	return s


def mirostat_draw(scores, q, mu, tau, eta):
	"""one mirostat step on the scores behind the warpers: (token, k, mu', unrounded k or nan).  Fewer than 101 finite scores: all of them stay."""
	s = np.asarray(scores, dtype=F32)
	V = s.shape[0]
	e, P = softmax_f32(s)
	finite = int((s > -np.inf).sum())
	ku = float("nan")
	if finite > MIRO_N:
		k, ku = mirostat_k(np.sort(P)[::-1][:MIRO_N + 1], V, mu)
		kept = keep_top(s, k)
	else:
		k, kept = finite, s
	ek = np.where(kept > -np.inf, e, F32(0))
	r = (ek / ek.sum(dtype=F32)) / np.asarray(q, dtype=F32)
	tok = int(np.argmax(r))
	return tok, k, mirostat_update(mu, P[tok], tau, eta), ku


def plain_draw(scores, q):
	e, _ = softmax_f32(scores)
	return int(np.argmax((e / e.sum(dtype=F32)) / np.asarray(q, dtype=F32)))


def token_step(scores, q, history, n_prefix, *, temperature=1.0, top_k=0, repetition_penalty=1.0, repetition_penalty_decay=0.0, stop_length_penalty=0.0,
			   min_temperature=None, mirostat_tau=0.0, mirostat_eta=0.1, mu=None, stop_token=-1, suppress=()):
	"""One token for rows scores [B, V] with noise q [B, V].  history: per row the list of ids so far, the n_prefix prefix ids first (not modified).
	Returns dict(tokens [B], scores_out [B, V] (behind top-k), temp [B], k [B], k_unrounded [B], mu [B])."""
	scores = np.asarray(scores, dtype=F32)
	B, V = scores.shape
	out = dict(tokens=np.zeros(B, np.int64), scores_out=np.empty((B, V), F32), temp=np.zeros(B, np.float64), k=np.zeros(B, np.int64),
			   k_unrounded=np.full(B, np.nan), mu=None if mu is None else np.array(mu, dtype=np.float64))
	for b in range(B):
		s = scores[b]
		previous = list(history[b][n_prefix:])
		if repetition_penalty_decay != 0.0:
			s = decay_penalize(s, previous, repetition_penalty, repetition_penalty_decay)
		else:
			s = hf_penalize(s, history[b], repetition_penalty)
		s = stop_length_penalize(s, len(previous) + 1, stop_length_penalty, stop_token)
		for t in suppress:
			s[t] = -np.inf
		if min_temperature is not None and min_temperature >= 0:
			T = dynamic_temperature_value(s, temperature, min_temperature)
			s = s * (F32(1.0) / F32(T))
		else:
			T = temperature
			if F32(1.0) / F32(T) != F32(1.0):
				s = s * (F32(1.0) / F32(T))
		s = keep_top(s, top_k)
		out["temp"][b] = T
		out["scores_out"][b] = s
		if mirostat_tau > 0:
			tok, k, m2, ku = mirostat_draw(s, q[b], out["mu"][b], mirostat_tau, mirostat_eta)
			out["k"][b], out["mu"][b], out["k_unrounded"][b] = k, m2, ku
		else:
			tok = plain_draw(s, q[b])
		out["tokens"][b] = tok
	return out


def half_integer_margin(ku):
	"""distance of an unrounded k from the nearest half-integer (where round() changes its answer)"""
	return abs((ku - math.floor(ku)) - 0.5)
