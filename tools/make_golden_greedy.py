"""Regenerate tests/golden/hf_greedy_loop.npz: the ids of the INSTALLED HuggingFace greedy loop (`GenerationMixin._sample` with do_sample=False,
num_return_sequences=1) on the model-free stub of oracle/stub_lm.py -- `greedy_ref.hf_greedy` (tests/greedy_ref.py) -- one entry per case of
`greedy_ref.CASES` next to the case's parameters.  Needs transformers; nothing else.

  ids::<case>   int64 [1, L]   what `generate` returned behind the prompt
  kw::<case>    JSON of {seed, stop_bias, max_generate_length, kwargs}
  versions      "transformers x.y.z / torch a.b.c" of the run
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
	sys.path.insert(0, p)
import greedy_ref  # noqa: E402


def main():
	import transformers
	torch.set_num_threads(1)
	out = {"versions": np.array(f"transformers {transformers.__version__} / torch {torch.__version__}")}
	for name, seed, bias, L, kw in greedy_ref.CASES:
		ids = greedy_ref.hf_case(name)
		out["ids::" + name] = ids.numpy().astype(np.int64)
		out["kw::" + name] = np.array(json.dumps(dict(seed=seed, stop_bias=bias, max_generate_length=L, kwargs=kw)))
		print(name, tuple(ids.shape), ids[0, -3:].tolist())
	np.savez(os.path.join(ROOT, "tests", "golden", "hf_greedy_loop.npz"), **out)


if __name__ == "__main__":
	main()
