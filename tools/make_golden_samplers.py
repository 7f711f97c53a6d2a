"""Regenerate tests/golden/samplers_ref.npz from the reference's own tortoise_tts/samplers.py, imported by file path.  The reference checkout is
$TTK_REFERENCE (default /root/reference).  CPU, one thread: a rerun reproduces every array bit for bit.

Inputs are regenerated from seeds (`case_inputs` below, which tests/test_samplers_ref.py imports): only seeds, parameters and results are stored.
The reference's functions return the scores or the state; the two values they keep in locals -- dynamic_temperature's T_dyn and mirostat_sample's k -- are
read from the returning frame (sys.setprofile), so they are the reference's own f64 / int values and not ones recovered from f32 outputs.

Keys (i = case number per family):
  pen_params [n, 5]     f64: seed, V, factor, decay, history length          pen_out_<i>  f32 [V]: reptition_penalize(logits, previous, factor, decay)
  len_params [n, 5]     f64: seed, V, length, factor, stop token             len_out_<i>  f32 [V]: length_penalize(logits, length, factor, token)
  dyn_params [n, 5]     f64: seed, V, temperature, min_temperature, kind     dyn_t [n] f64: T_dyn;  dyn_out_<i> f32 [V]
                        kind 0 = peaked (p_max ~ 1), 1 = flat (~ 1 / V), 2 = middle (~ 0.5)
  miro_params [n, 6]    f64: seed, V, tau, eta, max_surprise before, torch seed of the draw
  miro_k [n] i64: the reference's k (compute_k + 1);  miro_token [n] i64;  miro_p_token [n] f32: prob_original of that token;  miro_mu [n] f64: max_surprise after
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# every parameter is exact in f32, so the reference's Python floats and the f32 fields of the C ABI name the same numbers
PEN_CASES = ((11, 1024, 2.0, 0.5, 40), (12, 1024, 1.5, -0.5, 40), (13, 1024, 1.25, 1.0, 7), (14, 8194, 2.0, 0.5, 300))
LEN_CASES = ((21, 1024, 1, 0.5, 1023), (22, 1024, 37, 0.5, 1023), (23, 1024, 37, -0.5, 1023), (24, 8194, 250, 2.0, 8193))
DYN_CASES = ((31, 1024, 0.75, 0.25, 0), (32, 1024, 0.75, 0.25, 1), (33, 1024, 0.75, 0.25, 2), (34, 8194, 1.0, 0.0, 2), (35, 8194, 1.5, 0.5, 1))
MIRO_CASES = ((41, 8194, 3.0, 0.125, 6.0, 1), (42, 8194, 5.0, 0.25, 10.0, 2), (43, 8194, 5.0, 0.125, 7.5, 3), (44, 1000, 3.0, 0.25, 5.0, 4), (45, 8194, 3.0, 0.125, 9.0, 5))


def case_inputs(family, case):
	"""the inputs of a case from its seed: (logits f32 [V], previous int64 [n] or None)"""
	seed, V = int(case[0]), int(case[1])
	rs = np.random.RandomState(seed)
	logits = (rs.standard_normal(V) * 4).astype(np.float32)
	if family == "pen":
		previous = rs.randint(0, 24, size=int(case[4])).astype(np.int64)      # 24 ids over the history: repeats, with their latest occurrence at every distance
		return logits, previous
	if family == "dyn":
		kind = int(case[4])
		if kind == 0:
			logits[rs.randint(V)] += 60.0
		elif kind == 1:
			logits *= np.float32(0.001)
		else:
			logits[rs.randint(V)] = logits.max() + np.float32(np.log(np.exp((logits - logits.max()).astype(np.float64)).sum()))      # as much mass as all the others
	return logits, None


def reference_module():
	ref = os.environ.get("TTK_REFERENCE", "/root/reference")
	spec = importlib.util.spec_from_file_location("_ref_samplers", os.path.join(ref, "tortoise_tts", "samplers.py"))
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


def call_with_local(fn, name, local, *args, **kw):
	"""fn(*args, **kw) and the value its local variable `local` holds when the function called `name` returns"""
	seen = {}

	def prof(frame, event, arg):
		if event == "return" and frame.f_code.co_name == name and local in frame.f_locals:
			seen[local] = frame.f_locals[local]
	sys.setprofile(prof)
	try:
		out = fn(*args, **kw)
	finally:
		sys.setprofile(None)
	return out, seen[local]


def main():
	torch.set_num_threads(1)
	mod = reference_module()
	out = {}
	out["pen_params"] = np.asarray(PEN_CASES, dtype=np.float64)
	for i, c in enumerate(PEN_CASES):
		logits, previous = case_inputs("pen", c)
		y = mod.reptition_penalize(torch.from_numpy(logits.copy())[None], torch.from_numpy(previous), factor=c[2], decay=c[3], one_time=True)
		out[f"pen_out_{i}"] = y[0].numpy().copy()
		print("pen", c, "changed", int((out[f"pen_out_{i}"] != logits).sum()))
	out["len_params"] = np.asarray(LEN_CASES, dtype=np.float64)
	for i, c in enumerate(LEN_CASES):
		logits, _ = case_inputs("len", c)
		y = mod.length_penalize(torch.from_numpy(logits.copy())[None], int(c[2]), factor=c[3], token=int(c[4]))
		out[f"len_out_{i}"] = y[0].numpy().copy()
	out["dyn_params"] = np.asarray(DYN_CASES, dtype=np.float64)
	ts = []
	for i, c in enumerate(DYN_CASES):
		logits, _ = case_inputs("dyn", c)
		y, t = call_with_local(mod.dynamic_temperature, "dynamic_temperature", "dynamic_temperature", torch.from_numpy(logits.copy())[None], temperature=c[2], min_temperature=c[3])
		out[f"dyn_out_{i}"] = y[0].numpy().copy()
		ts.append(float(t))
		print("dyn", c, "T_dyn", t)
	out["dyn_t"] = np.asarray(ts, dtype=np.float64)
	out["miro_params"] = np.asarray(MIRO_CASES, dtype=np.float64)
	ks, toks, pts, mus = [], [], [], []
	for c in MIRO_CASES:
		logits, _ = case_inputs("miro", c)
		state = dict(n=int(c[1]), tau=c[2], eta=c[3], max_surprise=c[4])
		torch.manual_seed(int(c[5]))
		state, k = call_with_local(mod.mirostat_sample, "mirostat_sample", "k", torch.from_numpy(logits.copy())[None], state)
		tok = int(state["token"])
		p_tok = 2.0 ** (-state["index_surprise"])                       # prob_original[prev_i], an f32 value: recovered exactly up to the last bit of the f64 log2
		ks.append(int(k)); toks.append(tok); pts.append(np.float32(p_tok)); mus.append(float(state["max_surprise"]))
		print("miro", c, "k", k, "token", tok, "p", p_tok, "mu", state["max_surprise"])
	out.update(miro_k=np.asarray(ks, np.int64), miro_token=np.asarray(toks, np.int64), miro_p_token=np.asarray(pts, np.float32), miro_mu=np.asarray(mus, np.float64))
	os.makedirs(GOLDEN, exist_ok=True)
	path = os.path.join(GOLDEN, "samplers_ref.npz")
	np.savez(path, **out)
	print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
	main()
