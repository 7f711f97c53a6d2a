"""Regenerate tests/golden/hf_beam_loop.npz: the ids of the INSTALLED HuggingFace beam-sample loop (`GenerationMixin._beam_search`,
do_sample=True) on the model-free stub of oracle/stub_lm.py -- `stub_lm.hf_generate` with `num_beams` among its keyword arguments -- on the CPU
generator, one entry per case of `beam_ref.CASES` (tests/beam_ref.py) next to the case's parameters.  Needs transformers; nothing else.

  ids::<case>   int64 [num_return_sequences, L]   what `generate` returned behind the prompt
  kw::<case>    JSON of {seed, stop_bias, num_beams, num_return_sequences, max_generate_length, kwargs}
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
import beam_ref  # noqa: E402


def main():
	import transformers
	torch.set_num_threads(1)
	out = {"versions": np.array(f"transformers {transformers.__version__} / torch {torch.__version__}")}
	for name, seed, bias, N, R, L, kw in beam_ref.CASES:
		ids = beam_ref.hf_case(name)
		out["ids::" + name] = ids.numpy().astype(np.int64)
		out["kw::" + name] = np.array(json.dumps(dict(seed=seed, stop_bias=bias, num_beams=N, num_return_sequences=R, max_generate_length=L, kwargs=kw)))
		print(name, tuple(ids.shape))
	np.savez(os.path.join(ROOT, "tests", "golden", "hf_beam_loop.npz"), **out)


if __name__ == "__main__":
	main()
