"""TEST INFRASTRUCTURE (a helper, not a test): greedy search -- HF `GenerationMixin._sample` with do_sample=False -- restated in plain torch on the
oracle's `prefix_embeddings` / `prefill` / `decode` interface, the one `stub_lm.StubAR` and `tortoise_oracle.AROracle` both implement.

What `UnifiedVoice.inference_speech` runs in the reference when no `do_sample` is passed is the greedy branch of its fork of HF's `generate`; the fork
does not run on the installed transformers, what it forks does.  So the behaviour restated here is the installed `_sample`
(HF:generation/utils.py:2783-2960; the greedy line is :2925, `next_tokens = torch.argmax(next_token_scores, dim=-1)`), pinned against that loop on the
model-free stub (tests/golden/hf_greedy_loop.npz, tests/test_greedy_ref.py):
  * processors: RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor, then the caller's custom processor (the typical warper of
    `inference_speech(typical_sampling=True)`); NO warpers: temperature, top_k and top_p are ignored without do_sample (HF only warns);
  * finished rows are padded with the stop token; the loop ends right after the token with which the last row finishes, or at max_length;
  * num_return_sequences != 1 is a ValueError;
  * `generate` reseeds and then draws nothing.
Exact ties: `torch.argmax` leaves the order among equal values unspecified; the product picks the lowest index, and so does `argmax_lowest` here.

CASES are the fixture's cases (tools/make_golden_greedy.py writes them from `hf_greedy`)."""
import warnings

import torch

import tortoise_oracle as O

# name, table seed, stop-token bias, max_generate_length, generate kwargs
CASES = [
	("runs_to_max_length", 21, 0.0, 20, dict()),
	("stops_early", 30, 6.0, 40, dict()),
	("repetition_penalty", 23, 3.0, 30, dict(repetition_penalty=2.0)),      # (without the penalty this table stops after 28 tokens)
	("suppress_stop", 24, 9.0, 16, dict(suppress_tokens=[8193, 5, 17])),
	("ignored_warpers", 25, 5.0, 30, dict(temperature=0.5, top_k=5, top_p=0.5)),
]


def argmax_lowest(scores):
	"""argmax over the last dim with exact ties going to the lowest index (an all -inf row gives 0, as ATen does)"""
	m = scores.max(dim=-1, keepdim=True).values
	return (scores == m).to(torch.uint8).argmax(dim=-1)


def process_scores(input_ids, logits, *, repetition_penalty=1.0, suppress_tokens=None, typical_mass=None):
	"""the processors that act without do_sample, in HF's order; the custom processor last"""
	s = logits
	if repetition_penalty is not None and repetition_penalty != 1.0:
		s = O.warp_repetition_penalty(input_ids, s, repetition_penalty)
	if suppress_tokens:
		s = O.warp_suppress(s, suppress_tokens)
	if typical_mass is not None:
		s = O.warp_typical(s, typical_mass)
	return s


def greedy_search(ar, cond_latent, text, *, num_return_sequences=1, max_generate_length=None, repetition_penalty=1.0, suppress_tokens=None,
				  typical_sampling=False, typical_mass=0.9, input_tokens=None, temperature=None, top_k=None, top_p=None, return_margins=False):
	"""ids [1, L] behind the fake prefix (the prompt tokens of `input_tokens` [1, n] in front, counted in max_generate_length, as in
	`tortoise_oracle.inference_speech`).  temperature / top_k / top_p are accepted and ignored.  return_margins: also the top-1 minus top-2 gap of the
	processed scores at every generated step -- what decides whether another implementation's rounding could pick another token."""
	if num_return_sequences != 1:
		raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {num_return_sequences}).")
	c = ar.cfg
	stop = c.stop_mel_token
	prefix = ar.prefix_embeddings(cond_latent, text)
	trunc = prefix.shape[1] + 1
	max_len = trunc + (c.max_mel_tokens - 1 if max_generate_length is None else max_generate_length)
	input_ids = torch.ones((1, trunc), dtype=torch.long)
	input_ids[:, -1] = c.start_mel_token
	prompt = None
	if input_tokens is not None:
		assert input_tokens.shape[0] == 1, "one prompt row: greedy search returns one sequence"
		prompt = input_tokens
		input_ids = torch.cat([input_ids, prompt], dim=1)
	unfinished = torch.ones(1, dtype=torch.long)
	logits, past, _ = ar.prefill(prefix, 1) if prompt is None else ar.prefill(prefix, 1, prompt)
	logits = logits[:, -1]
	k = 0 if prompt is None else prompt.shape[1]
	margins = []
	while True:
		scores = process_scores(input_ids, logits.float(), repetition_penalty=repetition_penalty, suppress_tokens=suppress_tokens,
								typical_mass=typical_mass if typical_sampling else None)
		top2 = torch.topk(scores, 2, dim=-1).values
		margins.append(float((top2[:, 0] - top2[:, 1]).min()))
		nxt = argmax_lowest(scores)
		nxt = nxt * unfinished + stop * (1 - unfinished)
		input_ids = torch.cat([input_ids, nxt[:, None]], dim=-1)
		k += 1
		done = (nxt == stop) | (input_ids.shape[1] >= max_len)
		unfinished = unfinished & ~done
		if unfinished.max() == 0:
			break
		logits, past, _ = ar.decode(nxt, k, past)
	gen = input_ids[:, trunc:]
	return (gen, margins) if return_margins else gen


def hf_greedy(table, N, kw):
	"""the installed HuggingFace loop on the model-free stub with do_sample=False, num_return_sequences=1 (`stub_lm.hf_generate` hard-codes
	do_sample=True, so this is its twin); the warnings HF raises about ignored sampling flags are dropped"""
	import stub_lm
	from transformers import GenerationMixin, GPT2Config, LogitsProcessorList, PreTrainedModel
	from transformers.modeling_outputs import CausalLMOutput
	trunc = stub_lm.PREFIX + 1

	class StubLM(PreTrainedModel, GenerationMixin):
		config_class = GPT2Config

		def __init__(self, config):
			super().__init__(config)
			self.dummy = torch.nn.Parameter(torch.zeros(1))

		def forward(self, input_ids=None, attention_mask=None, **unused):
			lg = torch.zeros(input_ids.shape[0], input_ids.shape[1], stub_lm.V)
			lg[:, -1] = stub_lm.stub_logits(table, input_ids[:, -1], input_ids.shape[1] - trunc)
			return CausalLMOutput(logits=lg)

	model = StubLM(GPT2Config(vocab_size=stub_lm.V, n_layer=1, n_head=1, n_embd=8)).eval()
	inputs = torch.ones(1, trunc, dtype=torch.long)
	inputs[:, -1] = stub_lm.START
	torch.manual_seed(0)
	with torch.inference_mode(), warnings.catch_warnings():
		warnings.simplefilter("ignore")
		out = model.generate(inputs, bos_token_id=stub_lm.START, pad_token_id=stub_lm.STOP, eos_token_id=stub_lm.STOP, max_length=trunc + N,
							 logits_processor=LogitsProcessorList(), num_return_sequences=1, do_sample=False, use_cache=False, **kw)
	return out[:, trunc:]


def stub_case(name, **extra):
	"""(ids of `greedy_search` on the model-free stub for CASES[name], the case's parameters)"""
	import stub_lm
	from tortoise_tts_amd import weights as W
	seed, bias, L, kw = next(c[1:] for c in CASES if c[0] == name)
	ar = stub_lm.StubAR(W.AR_SMALL, stub_lm.make_table(seed, bias))
	with torch.inference_mode():
		out = greedy_search(ar, torch.zeros(1, 1), torch.zeros(1, stub_lm.PREFIX - 3, dtype=torch.long), max_generate_length=L, **kw, **extra)
	return out, (seed, bias, L, kw)


def hf_case(name):
	"""the installed HF loop on the same stub (needs transformers)"""
	import stub_lm
	seed, bias, L, kw = next(c[1:] for c in CASES if c[0] == name)
	return hf_greedy(stub_lm.make_table(seed, bias), L, kw)
