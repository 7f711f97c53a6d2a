"""A plain `bench.py` run (no --full) on the small models -- a plumbing check, not the metric: ONE result line whose --full fields are null, and with
--dump-outputs DIR the arrays the last timed step returned; two runs with the same arguments write the same arrays.  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
	env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TTK_BENCH_REHEARSAL", "TTK_BENCH_PROBE")}
	r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--small", "--steps", "2", "--warmup", "1", "--dump-outputs", out_dir],
					   env=env, capture_output=True, text=True, timeout=600)
	assert r.returncode == 0, r.stderr[-3000:]
	lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
	assert len(lines) == 1, r.stdout[-2000:]
	return json.loads(lines[0])


def test_plain_bench_run_dumps_the_last_step_and_repeats_it(tmp_path):
	a, b = str(tmp_path / "a"), str(tmp_path / "b")
	line = _bench(a)
	assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "bf16" and line["higher_is_better"] is True
	assert all(line[k] is None for k in ("roofline", "cpu_baseline", "latent_k1_variant", "pipelined_lines", "stop_live"))
	names = sorted(os.listdir(a))
	assert {"mels.npy", "codes.npy", "latents.npy", "E.npy", "noise.npy", "mel.npy", "best.npy"} <= set(names)
	assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
	mels, codes = np.load(os.path.join(a, "mels.npy")), np.load(os.path.join(a, "codes.npy"))
	assert mels.dtype == np.float32 and mels.shape[:2] == (1, 100) and np.isfinite(mels).all()
	assert abs(line["value"] - mels.shape[-1] * 256 / 24000 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]      # the audio of the dumped mel per timed step
	assert codes.dtype == np.float64 and codes.shape == (16, 250) and (codes == np.round(codes)).all()
	_bench(b)
	assert sorted(os.listdir(b)) == names
	for n in names:
		assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n))), n
