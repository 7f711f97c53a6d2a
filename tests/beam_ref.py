"""TEST INFRASTRUCTURE (a helper, not a test): HF `GenerationMixin._beam_search` with do_sample=True restated in plain torch on the oracle's
`prefix_embeddings` / `prefill` / `decode` interface, the one `stub_lm.StubAR` and `tortoise_oracle.AROracle` both implement.

What `TTS.inference(beam_width=N)` runs in the reference is its fork of HF's `generate` with num_beams=N (inference.py:161,342); the fork does
not run on the installed transformers, what it forks does.  So the behaviour restated here is the installed
`_beam_search` (HF:generation/utils.py:3208-3509, helpers :2988-3204), batch size 1, early_stopping False, pad = eos = the stop token, and it
is pinned against that loop on the model-free stub (tests/golden/hf_beam_loop.npz, tests/test_beam_ref.py).  Line numbers below are HF's.

CASES are the fixture's cases (tools/make_golden_beam.py writes them from `stub_lm.hf_generate`)."""
import torch
import torch.nn.functional as F

import tortoise_oracle as O

# name, table seed, stop-token bias, num_beams, num_return_sequences, max_generate_length, generate kwargs
CASES = [
	("four_beams", 11, 6.0, 4, 1, 24, dict(temperature=0.8, top_k=0)),
	("length_penalty", 12, 6.0, 4, 3, 24, dict(top_k=0, length_penalty=2.0)),
	("two_beams_warpers", 13, 6.0, 2, 2, 30, dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=2.0)),
	("runs_to_max_length", 14, -4.0, 8, 1, 12, dict(temperature=0.9, top_k=0)),
	("sixteen_beams", 15, 6.0, 16, 1, 40, dict(temperature=0.8, top_k=0)),
]


def process_log_probs(input_ids, log_probs, *, temperature=1.0, top_k=50, top_p=1.0, repetition_penalty=1.0, suppress_tokens=None):
	"""`logits_processor(flat_running_sequences, log_probs)` (:3389): the processors and warpers of the sample branch applied to the LOG-PROBS, in
	the order `_get_logits_processor` builds them; top-k and top-p with min_tokens_to_keep = 2 (one EOS token + 1, :1297-1322)."""
	s = log_probs
	if repetition_penalty is not None and repetition_penalty != 1.0:
		s = O.warp_repetition_penalty(input_ids, s, repetition_penalty)
	if suppress_tokens:
		s = O.warp_suppress(s, suppress_tokens)
	if temperature is not None and temperature != 1.0:
		s = O.warp_temperature(s, temperature)
	if top_k is not None and top_k != 0:
		s = O.warp_top_k(s, top_k, min_tokens_to_keep=2)
	if top_p is not None and top_p < 1.0:
		s = O.warp_top_p(s, top_p, min_tokens_to_keep=2)
	return s


def _gather(t, idx):
	return t[idx]


def reorder_cache(past, beam_idx):
	"""`_reorder_cache` (unified_voice.py:257-265): every layer's (k, v) index_select'ed along the batch"""
	if past is None:
		return None
	return [tuple(s.index_select(0, beam_idx.to(s.device)) for s in layer) for layer in past]


def beam_search(ar, cond_latent, text, *, num_beams, num_return_sequences=1, max_generate_length=None, length_penalty=1.0, temperature=1.0, top_k=50,
				top_p=1.0, repetition_penalty=1.0, suppress_tokens=None, sample_device="cpu", seed=0, return_trace=False, step_trace=None):
	"""ids [num_return_sequences, L]: `sequences[:R]` behind the prompt, cropped to the longest returned beam and padded with the stop token
	(step 5, :3510-3523).  `sample_device`: where softmax + torch.multinomial run (CPU and GPU generator streams differ), as in
	`tortoise_oracle.inference_speech`; everything else is computed where the oracle computes.  return_trace: also a dict with the number of
	steps, the final running / finished scores and `is_sent_finished`.  step_trace: a list that receives one dict per step (the 2 * num_beams picks as
	flat indices, then the state the step leaves behind)."""
	c = ar.cfg
	N, R = num_beams, num_return_sequences
	if R > N:
		raise ValueError(f"`num_return_sequences` ({R}) has to be smaller or equal to `num_beams` ({N}).")
	stop = c.stop_mel_token
	prefix = ar.prefix_embeddings(cond_latent, text)
	trunc = prefix.shape[1] + 1
	max_new = (c.max_mel_tokens - 1) if max_generate_length is None else max_generate_length
	max_length = trunc + max_new
	torch.manual_seed(seed)
	if sample_device != "cpu":
		torch.cuda.manual_seed_all(seed)
	K = 2 * N                                                    # beams_to_keep = max(2, 1 + n_eos_tokens) * num_beams (:3286)
	top_mask = torch.arange(K) < N
	running = torch.full((N, max_length), stop, dtype=torch.long)
	running[:, :trunc] = 1
	running[:, trunc - 1] = c.start_mel_token
	sequences = running.clone()
	running_scores = torch.zeros(N)
	running_scores[1:] = -1e9
	beam_scores = torch.full((N,), -1e9)
	finished = torch.zeros(N, dtype=torch.bool)
	unsatisfied = torch.ones((), dtype=torch.bool)
	lengths = torch.zeros(N, dtype=torch.long)                    # generated tokens of each finished beam (HF reads them off beam_indices, :3520)
	cur_len = trunc
	logits, past, _ = ar.prefill(prefix, N)
	logits = logits[:, -1]
	steps = 0
	while True:
		log_probs = F.log_softmax(logits.float(), dim=-1)                                           # b. (:3388)
		log_probs = process_log_probs(running[:, :cur_len], log_probs, temperature=temperature, top_k=top_k, top_p=top_p,
									  repetition_penalty=repetition_penalty, suppress_tokens=suppress_tokens)
		V = log_probs.shape[-1]
		acc = (log_probs + running_scores[:, None]).reshape(1, N * V)
		probs = F.softmax(acc.to(sample_device), dim=-1)                                             # c. (:3107-3111)
		topk_idx = torch.multinomial(probs, num_samples=K).cpu()[0]
		topk_lp = acc[0][topk_idx]
		beam = topk_idx // V
		topk_seq = _gather(running, beam).clone()
		topk_seq[:, cur_len] = topk_idx % V
		hits = (topk_seq[:, cur_len] == stop) | (cur_len + 1 >= max_length)                        # d. EosTokenCriteria | MaxLengthCriteria
		run_lp = topk_lp + hits.to(torch.float32) * -1.0e9                                          # e. (:3145-3150)
		nxt = torch.topk(run_lp, k=N)[1]
		running, running_scores, beam_idx = _gather(topk_seq, nxt), _gather(run_lp, nxt), _gather(beam, nxt)
		just = hits & top_mask                                                                      # f. (:3178-3203)
		fin_lp = topk_lp / ((cur_len + 1 - trunc) ** length_penalty)
		fin_lp = fin_lp + (~unsatisfied).to(torch.float32) * -1.0e9
		fin_lp = fin_lp + (~just) * -1.0e9
		merged = torch.topk(torch.cat((beam_scores, fin_lp)), k=N)[1]
		sequences = _gather(torch.cat((sequences, topk_seq)), merged)
		beam_scores = _gather(torch.cat((beam_scores, fin_lp)), merged)
		lengths = _gather(torch.cat((lengths, torch.full((K,), cur_len + 1 - trunc))), merged)
		finished = _gather(torch.cat((finished, just)), merged)
		past = reorder_cache(past, beam_idx)                                                        # g. (:3477-3489)
		cur_len += 1
		steps += 1
		best = running_scores[:1] / ((cur_len - trunc) ** length_penalty)                           # `_check_early_stop_heuristic` (:3044-3052)
		worst = torch.where(finished, beam_scores.min(), torch.tensor(-1.0e9))
		unsatisfied = unsatisfied & torch.any(best > worst)
		if step_trace is not None:
			step_trace.append(dict(picks=topk_idx.clone(), pick_lp=topk_lp.clone(), tok=running[:, cur_len - 1].clone(), beam_idx=beam_idx.clone(), running_scores=running_scores.clone(),
								   beam_scores=beam_scores.clone(), finished=finished.clone(), lengths=lengths.clone(), unsatisfied=bool(unsatisfied),
								   sequences=sequences[:, trunc:].clone(), running=running[:, trunc:].clone()))
		if not bool(unsatisfied & ~torch.all(hits)):                                                # `_beam_search_has_unfinished_sequences` (:3065-3075)
			break
		tok = running[:, cur_len - 1]
		logits, past, _ = ar.decode(tok, cur_len - trunc, past)
	n = int(lengths[:R].max())
	ids = sequences[:R, trunc:trunc + n]
	if return_trace:
		return ids, dict(steps=steps, running=running[:, trunc:trunc + steps], running_scores=running_scores, beam_scores=beam_scores, finished=finished,
						 lengths=lengths)
	return ids


def stub_case(name, sample_device="cpu", return_trace=False, step_trace=None):
	"""(ids of `beam_search` on the model-free stub for CASES[name], the case's parameters)"""
	import stub_lm
	from tortoise_tts_amd import weights as W
	seed, bias, N, R, L, kw = next(c[1:] for c in CASES if c[0] == name)
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(seed, bias))
	with torch.inference_mode():
		out = beam_search(ar, torch.zeros(1, 1), torch.zeros(1, stub_lm.PREFIX - 3, dtype=torch.long), num_beams=N, num_return_sequences=R,
						  max_generate_length=L, sample_device=sample_device, return_trace=return_trace, step_trace=step_trace, **kw)
	return out, (seed, bias, N, R, L, kw)


def hf_case(name):
	"""the installed HF loop on the same stub (needs transformers)"""
	import stub_lm
	seed, bias, N, R, L, kw = next(c[1:] for c in CASES if c[0] == name)
	return stub_lm.hf_generate(stub_lm.make_table(seed, bias), R, L, dict(num_beams=N, **kw))
