#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's config, on N MI355X of one node.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

metric   audio-sec/wall-sec (RTF^-1): seconds of 24 kHz audio whose mel spectrogram the hot path produces per wall second
workload configs[1]: one utterance per GPU, 64 text tokens, 16 AR candidates x 250 mel tokens (stop token suppressed so the
         length is fixed), latent pass on the 16 candidates, 80 DDIM steps with conditioning-free guidance at T = 1088
         frames (11.6 s of audio), bf16 weights/MFMA operands with f32 accumulation.  Full-size synthetic weights (no
         checkpoints exist offline), inputs resident in HBM before the timed region.
step     one utterance through the whole hot path (tortoise_tts_amd/inference.py: inference.py:331-413 of the reference).
N > 1    weak scaling: every rank runs its own utterance (BASELINE configs[2]); the only exchange is one RCCL all-gather of
         the sampled candidate ids per utterance (the hand-off to candidate scoring); value = N * audio / max-rank time.
A plain run sets up, warms up, times the K steps and prints the result line; nothing else runs.  With --full it also reports
`roofline` of the dominant kernel (HIP events inside libttk, see ttk_prof_*) with `roofline.phases` (AR decode
against the HBM peak, latent pass and DDIM loop against the MFMA peak, from device events around the phases of one more
un-instrumented step and SURVEY.md section 8d's algorithmic work), the informational `latent_k1_variant`, `pipelined_lines` and
`stop_live` lines (rank 0, N = 1), and `cpu_baseline` (the CPU oracle on a bounded sample of the same workload, rank 0, N = 1 only);
--no-roofline / --no-cpu-baseline leave parts of that out.  Those fields are null in a plain run.
--dump-outputs DIR  after the timed steps, rank 0 writes what the last timed step returned (the mels and the aux arrays of
         TTSHotPath.inference, per line with --shard candidates, the waveform with --with-vocoder) as DIR/<name>.npy: floats as float32,
         integers as float64, at most 64 MB in all (a seeded sample of each array past its share).  The inputs, the weights and the
         sampling RNG (torch's default seeds) are the same from run to run with the same arguments.

N > 1 failure behaviour: a first multi-GPU run either prints its line or ends non-zero within minutes WITH a reason.
         Every rank logs to stderr and to gpurun_out/rank{r}.err; a stage watchdog (a daemon thread per rank, STAGE_BUDGET_S below) ends a rank that does not reach
         its next stage marker in time after dumping every thread's stack and the tail of RCCL's log (NCCL_DEBUG=WARN -> gpurun_out/rccl.rank{r}.log, never
         stdout); `python bench.py --gpus N` (self-launch) adds a parent-side watchdog over the same markers that terminates the CHILD process group and prints
         each rank's last lines.  Before any model is built every rank runs a ONE-collective pre-flight in a FRESH child process (`--preflight`: rendezvous on
         its own port, all_reduce of the rank ids, sum checked), first with HSA_ENABLE_IPC_MODE_LEGACY as inherited (0 = dmabuf IPC, what this pool's driver
         needs), then -- only if that fails -- with the other value; the setting that passed is the one the real process group is created under (120 s timeout).

--shard candidates   BASELINE configs[3] instead (not the headline line): ONE long-form utterance at a time, 2 lines x 256 text
         tokens, 32 candidates per GPU (256 at N = 8) x 500 mel tokens, 200 DDIM steps at T = 2176; candidates sharded over the ranks
         (tortoise_tts_amd/dist.py: ids all-gathered over RCCL, scores all-gathered, the lines' diffusions spread over the ranks, mels broadcast).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TEXT_TOKENS, CANDIDATES, MEL_TOKENS, DDIM_STEPS = 64, 16, 250, 80


def parse():
	ap = argparse.ArgumentParser()
	ap.add_argument("--gpus", type=int, default=1)
	ap.add_argument("--steps", type=int, default=3)
	ap.add_argument("--warmup", type=int, default=1)
	ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32", "fp8w", "fp8"],
					help="BASELINE config 5 -- fp8w: bf16 arithmetic, block GEMM weights in fp8-e4m3; fp8: also fp8 activations into the diffusion block GEMMs (fp8 MFMA)")
	ap.add_argument("--with-vocoder", action="store_true", help="BASELINE config 5's tail: the BigVGAN vocoder (bf16) inside the step; off for the headline metric")
	ap.add_argument("--full", action="store_true", help="also the roofline / phase passes, the informational variants and the CPU baseline after the timed steps (off: the headline line only)")
	ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, <= 64 MB in all)")
	ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
	ap.add_argument("--no-roofline", action="store_true", help="with --full: leave the roofline pass and the informational variants out")
	ap.add_argument("--small", action="store_true", help="tiny models (plumbing check only; the number is NOT the metric)")
	ap.add_argument("--no-graph", action="store_true", help="eager token loop (counter passes under rocprofv3 --pmc, which crashes on captured graphs); never the timed configuration")
	ap.add_argument("--preflight", action="store_true", help="internal: the one-collective pre-flight child of an N > 1 rank (see the docstring)")
	ap.add_argument("--shard", default="utterances", choices=["utterances", "candidates"],
					help="utterances: configs[1]/[2], one utterance per GPU (the headline metric); candidates: configs[3], one utterance's candidates over the GPUs")
	return ap.parse_args()


def cpu_baseline(seed, n_text=TEXT_TOKENS, n_cand=CANDIDATES, n_mel=MEL_TOKENS, n_ddim=DDIM_STEPS, n_lines=1, light=False):
	"""The CPU oracle (oracle/tortoise_oracle.py, kind 'port') on a bounded sample of the same workload, on this box's host cores, as
	BASELINE.md section 3 lays out: phases timed separately with time.perf_counter after a warm-up, medians of repeated samples --
	prefill at B = n_cand (second run timed), KV-cached decode steps (median of 3 groups of 8 steps, scaled to n_mel), the latent
	pass on the candidates at its full length (one run), DDIM steps at the FULL T (1 warm-up + median of 8 steps, each a
	conditioned + a conditioning-free evaluation, scaled to n_ddim).  light (configs[3], where one DDIM step at T = 2176 is tens of seconds
	of CPU time): groups of 4 decode steps, the latent pass on 4 candidates scaled to n_cand, 1 warm-up + 2 DDIM steps."""
	sys.path.insert(0, os.path.join(ROOT, "oracle"))
	import statistics
	import tortoise_oracle as O
	from tortoise_tts_amd import weights as W
	# the GPU box gives a 1-GPU job a 16-core share whatever os.cpu_count() says; oversubscribing it is pathologically slow
	try:
		cores = len(os.sched_getaffinity(0))
	except AttributeError:
		cores = os.cpu_count() or 1
	cores = max(1, min(cores, 16))
	torch.set_num_threads(cores)
	g = torch.Generator().manual_seed(seed)
	T = n_mel * 4 * 24000 // 22050
	grp, n_lat, n_steps = (4, min(4, n_cand), 2) if light else (8, n_cand, 8)
	with torch.inference_mode():
		ar = O.AROracle(W.synth_state_dict(W.ar_shapes(W.AR_FULL), 0), W.AR_FULL)
		text = torch.randint(1, 255, (1, n_text), generator=g)
		cond = torch.randn(1, 1024, generator=g)
		prefix = ar.prefix_embeddings(cond, text)
		ar.prefill(prefix, n_cand)                                       # warm-up
		t0 = time.perf_counter()
		logits, past, _ = ar.prefill(prefix, n_cand)
		t_prefill = time.perf_counter() - t0
		tok = torch.randint(0, 8192, (n_cand,), generator=g)
		k = 0
		for _ in range(2):                                               # warm-up steps
			k += 1
			_, past, _ = ar.decode(tok, k, past)
		groups = []
		for _ in range(3):
			t0 = time.perf_counter()
			for _ in range(grp):
				k += 1
				_, past, _ = ar.decode(tok, k, past)
			groups.append((time.perf_counter() - t0) / grp)
		t_dec = statistics.median(groups)
		del past
		codes = torch.randint(0, 8192, (n_lat, n_mel), generator=g)
		t0 = time.perf_counter()
		ar.forward_latents(cond.repeat(n_lat, 1), text.repeat(n_lat, 1), codes)
		t_lat = (time.perf_counter() - t0) * n_cand / n_lat
		del ar
		d = O.DiffusionOracle(W.synth_state_dict(W.diffusion_shapes(W.DIFF_FULL), 0), W.DIFF_FULL)
		x = torch.randn(1, 100, T, generator=g)
		E = torch.randn(1, 1024, T, generator=g)
		sched = O.SpacedSchedule(steps=n_ddim)
		x = sched.ddim_step(d, x, n_ddim - 1, E)                          # warm-up
		steps = []
		for i in range(n_steps):
			t0 = time.perf_counter()
			x = sched.ddim_step(d, x, n_ddim - 2 - i, E)
			steps.append(time.perf_counter() - t0)
		t_step = statistics.median(steps)
	est = n_lines * (t_prefill + n_mel * t_dec + t_lat + n_ddim * t_step)
	audio = n_lines * T * 256 / 24000
	return {"value": audio / est, "unit": "audio-sec/wall-sec", "cores": cores, "kind": "port",
			"torch": torch.__version__, "seconds_per_utterance": est,
			"sample": f"B={n_cand}: prefill (2nd run) {t_prefill:.2f} s + decode {t_dec * 1e3:.0f} ms/step (median of 3 groups of {grp}, scaled to {n_mel}) + "
					  f"latent pass on {n_lat} candidates x {n_mel} tokens" + (f" scaled to {n_cand}" if n_lat != n_cand else "") + f" {t_lat:.2f} s (one run) + DDIM {t_step:.2f} s/step at T={T} "
					  f"(cond + cond-free evaluation; 1 warm-up, median of {n_steps} steps, scaled to {n_ddim})" + (f"; x {n_lines} lines" if n_lines > 1 else "") + f"; fp32, {cores} threads"}


def phase_roofline(marks_per_line, dtype_name, n_text=TEXT_TOKENS, n_cand=CANDIDATES, n_mel=MEL_TOKENS, n_ddim=DDIM_STEPS):
	"""Per-phase roofline fractions (SURVEY.md section 8d / BASELINE.md section 4): AR decode is HBM-bound (weights streamed once per
	token + the KV cache read), the latent pass and the DDIM loop are MFMA-bound.  `marks_per_line`: one list of (name, event) pairs per text
	line, from TTSHotPath.inference(phase_marks=...) / inference_sharded(phase_marks=...) of one step run exactly as the timed ones (captured
	graph, no instrumentation); n_cand = candidates decoded on THIS GPU.  Peaks: 8 TB/s HBM; dense MFMA 2.5 PFLOP/s bf16 / f16, 157.3 TFLOP/s
	f32; dtype fp8: the DDIM loop is graded against the 5 PFLOP/s fp8 peak (its ResBlock convolutions and proj_out run the block-scaled 16x16x128 fp8 MFMA, the instruction that
	reaches that peak; q / k / v, QK^T, PV and the remaining convs run bf16 -- the stricter denominator is used for the whole phase), the latent pass against 2.5 (the AR handle's fp8 is
	fp8 WEIGHTS on the bf16 MFMA)."""
	ms = {}
	for marks in marks_per_line:
		for i in range(len(marks) - 1):
			ms[marks[i + 1][0]] = ms.get(marks[i + 1][0], 0.0) + marks[i][1].elapsed_time(marks[i + 1][1])
	L = len(marks_per_line)
	# candidate shards with several lines: the lines' diffusions are spread over the ranks (dist.assign_diffusers), so THIS rank's "ddim" interval covers the
	# lines it diffused (one ragged batch) -- possibly none; "_"-prefixed marks bracket time that belongs to no phase of the line that carries them
	L_ddim = sum((m[2] if len(m) > 2 else 1) for marks in marks_per_line for m in marks if m[0] == "ddim")
	e_w = {"bf16": 2, "f16": 2, "f32": 4, "fp8w": 1, "fp8": 1}[dtype_name]
	e_kv = 4 if dtype_name == "f32" else 2
	peak_f = 157.3e12 if dtype_name == "f32" else 2.5e15
	peak_ddim = 5.0e15 if dtype_name == "fp8" else peak_f
	P1 = n_text + 4                                    # prefix rows incl. start_mel
	# prefill: dense pass over P1 rows (once: the candidates share the prefix); decode step k (k = 1..M-1) reads a cache of P1 + k - 1 rows and writes one
	blocks, head = 377_886_720, 8_398_850 + 4_096
	ar_bytes = 0.0
	for k in range(1, n_mel):
		ctx = P1 + k
		ar_bytes += blocks * e_w + head * (2 if e_w == 1 else e_w) + n_cand * 30 * 2 * ctx * 1024 * e_kv + n_cand * 8194 * 4
	ar_bytes *= L
	prefill_flop = L * (2.0 * blocks * P1 * n_cand + 2.0 * P1 * P1 * 1024 * 30 * n_cand)
	S = n_text + n_mel + 5
	lat_flop = L * (2.0 * blocks * S * n_cand + 2.0 * S * S * 1024 * 30 * n_cand)
	T = n_mel * 4 * 24000 // 22050
	F = 236 * 1024 ** 2 * T + 52 * 1024 * T * T + 1_843_200 * T
	ddim_flop = L_ddim * n_ddim * 2.0 * F
	ar_floor = ar_bytes / 8.0e12 * 1e3 + prefill_flop / peak_f * 1e3
	def phase(bound, work_key, work, name, peak, unit_key, unit_scale, **extra):
		t = ms.get(name)
		if not t or not work:           # the phase did not run on this rank (a candidate shard whose lines are all diffused elsewhere)
			return {"bound": bound, work_key: work, "ms": t, "frac": None, "floor_ms": work / peak * 1e3, "note": "did not run on this rank", **extra}
		return {"bound": bound, work_key: work, "ms": t, unit_key: work / (t * 1e-3) / unit_scale, "frac": work / (t * 1e-3) / peak, "floor_ms": work / peak * 1e3, **extra}
	out = {
		"ar_decode": phase("hbm", "algorithmic_bytes", ar_bytes, "ar_decode", 8.0e12, "achieved_GBps", 1e9, prefill_flop=prefill_flop,
						   note=f"prefill + {n_mel} sampled tokens; bytes = {n_mel - 1} KV-cached steps (weights once per step + KV read + logits)"),
		"latent_pass": phase("mfma", "flop", lat_flop, "latent_pass", peak_f, "achieved_TFLOPs", 1e12),
		"ddim": phase("mfma", "flop", ddim_flop, "ddim", peak_ddim, "achieved_TFLOPs", 1e12, peak_TFLOPs=peak_ddim / 1e12, lines_diffused_here=L_ddim,
					  note=f"timestep-independent conditioning + {n_ddim} steps x (cond + cond-free evaluation); flop = {2 * n_ddim} F(T) per line diffused on this rank"),
	}
	out["ar_decode"]["floor_ms"] = ar_floor
	eff = effective_floor(dtype_name, n_text, n_cand, n_mel, n_ddim, L, L_ddim)
	chain = effective_floor(dtype_name, n_text, n_cand, n_mel, n_ddim, L, L_ddim, model="launch_chain")
	for key, name in (("ar_decode", "ar_decode_ms"), ("latent_pass", "latent_pass_ms"), ("ddim", "ddim_ms")):
		out[key]["effective_floor_ms"] = eff[name]
		out[key]["frac_of_effective_floor"] = eff[name] / out[key]["ms"] if out[key].get("ms") else None
		out[key]["launch_chain_model_ms"] = chain[name]          # round 5's "effective floor": calibrated on this implementation, kept one round for comparison, NOT a bound
		out[key]["frac_of_launch_chain_model"] = chain[name] / out[key]["ms"] if out[key].get("ms") else None
	out["effective_floor"] = {"formula": "sum over dependent launches of [boundary + max(hbm_bytes / hbm_stream, flop / peak; GEMMs: MFMA phase of the tile at the in-kernel clock, "
										 "bytes_per_CU / (cu_l2_intake x clock), staged bytes / l2_chip)] (bench.py, DESIGN.md section 6); every constant is a hardware rate from "
										 "MI355X_MICROARCH.md or from a microbenchmark that does not run csrc/gemm.hip",
							  "constants": eff["constants"], "launches": eff["launches"], "ddim_step_us": eff["ddim_step_us"], "decode_token_us": eff["decode_token_us_at_mean_ctx"],
							  "launch_chain_model": {"note": "round 5's pricing: GEMM k-loops at the 68 GB/s per CU this implementation's trip chain was measured at -- a model of the launch chain, not a floor",
													 "constants": chain["constants"], "ddim_step_us": chain["ddim_step_us"]}}
	if L > 1:
		out["lines"] = L
	out["whole_step_floor_ms"] = out["ar_decode"]["floor_ms"] + out["latent_pass"]["floor_ms"] + out["ddim"]["floor_ms"]
	out["whole_step_ms"] = sum(v for k, v in ms.items() if not k.startswith("_"))
	out["whole_step_frac_of_floor"] = out["whole_step_floor_ms"] / out["whole_step_ms"] if out["whole_step_ms"] else None
	out["whole_step_effective_floor_ms"] = eff["ar_decode_ms"] + eff["latent_pass_ms"] + eff["ddim_ms"]
	out["whole_step_frac_of_effective_floor"] = out["whole_step_effective_floor_ms"] / out["whole_step_ms"] if out["whole_step_ms"] else None
	out["whole_step_launch_chain_model_ms"] = chain["ar_decode_ms"] + chain["latent_pass_ms"] + chain["ddim_ms"]
	return out


_RANK_FILE = None


def out_dir():
	d = os.path.join(ROOT, "gpurun_out")
	os.makedirs(d, exist_ok=True)
	return d


def rank_file(rank):
	return os.path.join(out_dir(), f"rank{rank}.err")


# ---- the floor that applies.  The spec-peak fractions above measure the distance to bounds neither loop can reach at B = 16 / b = 2: the token
# loop is a chain of ~150 DEPENDENT launches per token, and a DDIM step's GEMMs have one tile per CU, whose k-loop runs at what one CU takes in from L2.  The
# effective floor prices exactly that, from stated constants of MI355X_MICROARCH.md's price table and the launch list of the path:
#     effective_floor = sum over the phase's dependent launches of [ BOUNDARY_US + max( hbm_bytes / HBM_STREAM , bytes_per_CU / CU_L2_INTAKE , flop / peak ) ]
#   BOUNDARY_US   1.45   "boundary": dependent kernel boundary on one stream, eager = graph
#   HBM_STREAM    6.4e12 "ldsdma-fill": what the chip streams from HBM with every CU loading (default policy; 8.0e12 is the spec figure the `frac` fields use)
#   CU_L2_INTAKE  68e9   "ring-gemm": the median CU takes in 68 GB/s through LDS-DMA (for csrc/gemm.hip it is the rate its trip chain runs at per staged byte rather than a bandwidth
#                        limit -- DESIGN.md section 5's traffic ablation -- i.e. this term prices a k-loop trip); a GEMM tile of BM x BN over K (x taps) stages (BM + BN) * K * taps * sizeof(T) bytes
#                        per CU and launch-round (rounds = max(1, tiles / 256)); tile shapes as csrc/gemm.hip picks them (`pick_tile`)
# Launch lists (include/ttk.h entry points -> csrc/ar.hip, csrc/diff.hip): a decode token = 30 x (ln_1+c_attn, attention, c_proj, ln_2+c_fc, mlp.c_proj) + mel_head + sampler
# = 152 launches over 805 MB of weights + the KV cache; the dense passes (prefill, latent pass) = 30 x (2 LayerNorm + 4 GEMM + attention) + 4; a DDIM step on the cond +
# cond-free batch = 16 ResBlocks x (2 GroupNorm-apply + 1x1 conv + k=3 conv) + 13 AttentionBlocks x (GroupNorm-apply + qkv + attention + proj_out) + 8 others
# (layout changes, input / integrating / output convs, out norm, the sampler update) = 124 launches (123 since round 6: the sampler update writes the next step's channels-last copy of x).  Reported NEXT TO `frac`, never instead of it.
BOUNDARY_US, HBM_STREAM, CU_L2_INTAKE = 1.45, 6.4e12, 68e9
# Round 6: a GEMM k-loop is no longer priced with CU_L2_INTAKE -- that constant reproduced the measured k-loops because it was READ OFF them.
# Its floor is now the largest of three hardware rates, none of them taken from csrc/gemm.hip:
#   the MFMA phase of the tile at the clock the chip holds INSIDE these kernels: rounds x 2 BM BN K taps / (peak / 256 CUs) x (2.4 GHz / CLOCK_HZ); CLOCK_HZ 2.3e9 from s_memtime / s_memrealtime
#       around the k-loops of the replayed chain on hashed operands (profiles/r06_clock.log: 2.26-2.36 GHz in the GEMMs, 2.34-2.41 in the attention -- the spec arithmetic's 2.4 GHz was 4 % high)
#   the L2 -> LDS intake of one CU: 59 B/clk with 4 waves, 72 B/clk with 8 (tests/diag/l2_intake.cpp on an L2-resident region, profiles/r06_l2_intake.log: LDS-DMA, loads to registers and
#       loads + ds_write all reach the same rate, so it is the texture path's, not an instruction's)
#   the chip's L2 bandwidth: 34.5 TB/s over the bytes ALL tiles stage in the launch (MI355X_MICROARCH.md, L2)
# and nothing for staging latency or the barrier per trip (what a perfect ring hides).  The old pricing stays in the line for one round as `launch_chain_model_ms`: a MODEL of this
# implementation's launch chain (its constants are measured on it), not a bound -- it is what the round-5 lines called effective_floor.
CLOCK_HZ, CU_INTAKE_BPC, L2_CHIP = 2.3e9, {4: 59.0, 8: 72.0}, 34.5e12


def _gemm_floor_us(M, N, K, taps, e, peak, model="hardware"):
	t128, t12864 = -(-M // 128) * -(-N // 128), -(-M // 128) * -(-N // 64)
	waves = 8
	if t128 >= 256:
		bm, bn, tiles = 128, 128, t128
		t256 = -(-M // 256) * -(-N // 128)
		if e <= 2 and t128 > 256 and 15 * -(-t256 // 256) <= 9 * -(-t128 // 256):
			bm, bn, tiles = 256, 128, t256
	elif t12864 >= 128:
		bm, bn, tiles, waves = 128, 64, t12864, 4
	else:
		bm, bn, tiles, waves = 64, 64, -(-M // 64) * -(-N // 64), 4
	rounds = max(1.0, tiles / 256)        # a floor: surplus tiles spread evenly (the mixed grid of csrc/gemm.hip approaches this), never a whole second round
	cu_bytes = rounds * (bm + bn) * K * taps * e
	if model == "launch_chain":
		return max(cu_bytes / CU_L2_INTAKE, 2.0 * M * N * K * taps / peak) * 1e6
	mfma = rounds * 2.0 * bm * bn * K * taps / (peak / 256) * (2.4e9 / CLOCK_HZ)
	intake = cu_bytes / (CU_INTAKE_BPC[waves] * CLOCK_HZ)
	l2 = tiles * (bm + bn) * K * taps * e / L2_CHIP
	return max(mfma, intake, l2) * 1e6


def effective_floor(dtype_name, n_text=TEXT_TOKENS, n_cand=CANDIDATES, n_mel=MEL_TOKENS, n_ddim=DDIM_STEPS, lines=1, lines_ddim=1, model="hardware"):
	"""{phase: effective_floor_ms, ...} by the formula above; `ar_bytes` etc. as phase_roofline counts them.  model="launch_chain": round 5's pricing of the GEMM k-loops (see CLOCK_HZ)"""
	_g = lambda M_, N_, K_, taps_, e_, peak_: _gemm_floor_us(M_, N_, K_, taps_, e_, peak_, model)
	e = {"bf16": 2, "f16": 2, "f32": 4, "fp8w": 2, "fp8": 2}[dtype_name]      # operand bytes staged per element by the dense GEMMs (fp8w widens at load; fp8 block GEMMs: 1, below)
	e_w = {"bf16": 2, "f16": 2, "f32": 4, "fp8w": 1, "fp8": 1}[dtype_name]
	e_kv = 4 if dtype_name == "f32" else 2
	peak = 157.3e12 if dtype_name == "f32" else 2.5e15
	P1, d = n_text + 4, 1024
	blocks, head = 377_886_720, 8_398_850 + 4_096
	# token loop
	tok_launches = 30 * 5 + 2
	ar_us = 0.0
	for k in range(1, n_mel):
		ctx = P1 + k
		hbm = blocks * e_w + head * (2 if e_w == 1 else e_w) + n_cand * 30 * 2 * ctx * d * e_kv + n_cand * 8194 * 4
		ar_us += tok_launches * BOUNDARY_US + hbm / HBM_STREAM * 1e6
	def dense_pass_us(rows_per_seq, seqs):
		M = rows_per_seq * seqs
		g = sum(_g(M, n, k, 1, e, peak) for n, k in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d)))
		attn = 2.0 * 2 * rows_per_seq * rows_per_seq * d * seqs / peak * 1e6 / 2      # causal: half the score matrix
		ln = 2 * (M * d * (4 + e) / 256 / CU_L2_INTAKE) * 1e6
		return 30 * (7 * BOUNDARY_US + g + attn + ln) + 4 * BOUNDARY_US
	tok_us = ar_us / max(n_mel - 1, 1)
	ar_us += dense_pass_us(P1, 1)                                     # the prefill runs the shared prefix once
	lat_us = dense_pass_us(n_text + n_mel + 5, n_cand)
	# DDIM step on the batch of 2 sequences (cond + cond-free) of T frames
	T = n_mel * 4 * 24000 // 22050
	M = 2 * T
	e_blk = 1 if dtype_name == "fp8" else e
	peak_blk = 5.0e15 if dtype_name == "fp8" else peak
	gn = M * d * (4 + e_blk) / 256 / CU_L2_INTAKE * 1e6
	res = 2 * gn + _g(M, d, d, 1, e_blk, peak_blk) + _g(M, d, d, 3, e_blk, peak_blk) + 4 * BOUNDARY_US
	att = gn + _g(M, 3 * d, d, 1, e, peak) + 2.0 * 2 * T * T * d * 2 / peak * 1e6 + _g(M, d, d, 1, e_blk, peak_blk) + 4 * BOUNDARY_US      # (the q / k / v projection keeps 16-bit operands in the fp8 modes)
	other = 7 * BOUNDARY_US + _g(M, d, 100, 3, e, peak) + _g(M, d, 2 * d, 1, e, peak) + _g(M, 200, d, 3, e, peak) + gn
	step_us = 16 * res + 13 * att + other
	step_launches = 16 * 4 + 13 * 4 + 7
	pre_us = 4 * (att - gn) + 8 * BOUNDARY_US                          # timestep_independent: 4 AttentionBlocks on the M latent rows (small), conv, norm, interpolate
	consts = {"boundary_us": BOUNDARY_US, "hbm_stream_Bps": HBM_STREAM, "cu_stream_Bps (LayerNorm / GroupNorm-apply launches)": CU_L2_INTAKE}
	consts.update({"gemm_kloop_Bps_per_CU (measured on this implementation)": CU_L2_INTAKE} if model == "launch_chain" else
				  {"in_kernel_clock_Hz": CLOCK_HZ, "cu_l2_intake_B_per_clk": CU_INTAKE_BPC, "l2_chip_Bps": L2_CHIP})
	return {"constants": consts,
			"launches": {"decode_token": tok_launches, "ddim_step": step_launches},
			"ar_decode_ms": lines * ar_us * 1e-3, "latent_pass_ms": lines * lat_us * 1e-3, "ddim_ms": lines_ddim * (n_ddim * step_us + pre_us) * 1e-3,
			"ddim_step_us": step_us, "decode_token_us_at_mean_ctx": tok_us}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(outputs, d, limit=DUMP_LIMIT_BYTES):
	"""--dump-outputs: every tensor or number of `outputs` (name -> value; None is skipped) as d/<name>.npy -- floating point as float32 (float64 stays
	float64), integers and booleans as float64 (exact for ids).  When the whole exceeds `limit` bytes, every array larger than an even share of it is
	replaced by a fixed sample of its flattened elements (sorted indices from numpy's Generator seeded 0: the same for every build at the same shape).
	Returns {name: shape written}."""
	import numpy as np
	import torch
	arrs = {}
	for k, v in outputs.items():
		if isinstance(v, torch.Tensor):
			x = v.detach().cpu()
			arrs[k] = (x.float() if x.is_floating_point() and x.dtype != torch.float64 else x.double()).numpy()
		elif isinstance(v, (int, float)):
			arrs[k] = np.array(v, dtype=np.float64)
	if sum(x.nbytes for x in arrs.values()) > limit:
		share = limit // len(arrs)
		for k, x in arrs.items():
			if x.nbytes > share:
				idx = np.sort(np.random.default_rng(0).choice(x.size, share // x.itemsize, replace=False))
				arrs[k] = x.reshape(-1)[idx]
	os.makedirs(d, exist_ok=True)
	for k, x in arrs.items():
		np.save(os.path.join(d, f"{k}.npy"), x)
	return {k: tuple(x.shape) for k, x in arrs.items()}


def log(msg):
	line = f"[bench] {msg}"
	print(line, file=sys.stderr, flush=True)
	if _RANK_FILE is not None:
		try:
			with open(_RANK_FILE, "a") as f:
				f.write(f"{time.strftime('%H:%M:%S')} {line}\n")
		except OSError:
			pass


# Stage markers a rank logs, in order, with the seconds it may take to reach each one from the previous (TTK_BENCH_STAGE_BUDGET overrides every entry: tests).
# "rendezvous" includes the first `import torch` of a fresh box (1-2 min) and the pre-flight children; the parent-side watchdog allows PARENT_GRACE_S more.
STAGE_BUDGET_S = (("preflight ok", 420.0), ("rendezvous ok", 150.0), ("models built", 240.0), ("timed region", 120.0), ("timed done", 240.0), ("result", 900.0))
PARENT_GRACE_S = float(os.environ.get("TTK_BENCH_PARENT_GRACE", "20"))
EXIT_STAGE_OVERRUN, EXIT_PREFLIGHT = 75, 76


def stage_budgets(a=None):
	"""the budgets for THIS run: the two stages that execute steps grow with what was asked for (a healthy --steps 100 run must not be ended by a constant) --
	warm-up + graph capture / the timed steps at a generous per-step time (2 s per utterance step, 10 s per configs[3] shard step: 6-7x what one GPU measures)"""
	o = os.environ.get("TTK_BENCH_STAGE_BUDGET")
	if o:
		return tuple((n, float(o)) for n, _ in STAGE_BUDGET_S)
	if a is None:
		return STAGE_BUDGET_S
	per = 10.0 if getattr(a, "shard", "") == "candidates" else 2.0
	grow = {"timed region": per * max(0, getattr(a, "warmup", 0)), "timed done": per * max(0, getattr(a, "steps", 0))}
	return tuple((n, b + grow.get(n, 0.0)) for n, b in STAGE_BUDGET_S)


def tail_of(path, n=25):
	try:
		with open(path, errors="replace") as f:
			return "".join(f.readlines()[-n:])
	except OSError:
		return ""


class StageWatchdog:
	"""One per rank.  `reached(marker)` logs the marker and arms the budget of the NEXT one; a daemon thread ends the process (exit 75) when the armed marker
	is overdue, after writing where every thread stands (faulthandler) and the tail of RCCL's log -- a rank stuck in a rendezvous, a collective or a kernel
	becomes a message and an exit status instead of a run killed at the driver's limit with nothing to read."""

	def __init__(self, rank, world, a=None):
		import threading
		self.rank, self.world = rank, world
		self.budgets = list(stage_budgets(a))
		if os.environ.get("TTK_BENCH_STALL_AT") and int(os.environ.get("TTK_BENCH_STALL_RANK", "-1")) != rank:
			# tests only: the ranks NOT made to stall wait in a collective for the one that is, with budgets armed at about the same instant; twice
			# the budget makes the stalled rank's own watchdog the one that speaks, instead of whichever thread happens to poll first
			self.budgets = [(n, 2 * b) for n, b in self.budgets]
		self.elapsed = {}                      # marker -> seconds from the previous marker (goes into the result line: the first real N > 1 run calibrates the budgets)
		self.last = time.monotonic()
		self.i = 0
		self.lock = threading.Lock()
		self.deadline = time.monotonic() + self.budgets[0][1]
		self.t0 = time.monotonic()
		self.off = False
		threading.Thread(target=self._run, daemon=True, name="stage-watchdog").start()

	def reached(self, marker):
		with self.lock:
			names = [n for n, _ in self.budgets]
			now = time.monotonic()
			self.elapsed[marker] = round(now - self.last, 2)
			self.last = now
			if marker in names:
				self.i = names.index(marker) + 1
				self.deadline = time.monotonic() + self.budgets[self.i][1] if self.i < len(self.budgets) else None
		log(f"[reached] {marker} (rank {self.rank}, +{time.monotonic() - self.t0:.1f}s)")

	def stop(self):
		self.off = True

	def _run(self):
		import faulthandler
		while not self.off:
			time.sleep(0.25)
			with self.lock:
				dl, i = self.deadline, self.i
			if dl is None or time.monotonic() <= dl:
				continue
			name, budget = self.budgets[i]
			log(f"[watchdog] rank {self.rank}/{self.world}: marker '{name}' not reached within {budget:.0f}s of the previous one; thread stacks follow, then exit {EXIT_STAGE_OVERRUN}")
			try:
				faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
				if _RANK_FILE is not None:
					with open(_RANK_FILE, "a") as f:
						faulthandler.dump_traceback(file=f, all_threads=True)
			except Exception:
				pass
			rl = tail_of(os.path.join(out_dir(), f"rccl.rank{self.rank}.log"))
			if rl:
				log(f"[watchdog] tail of RCCL's log:\n{rl}")
			os._exit(EXIT_STAGE_OVERRUN)


def preflight_child(a):
	"""`bench.py --gpus N --preflight`, started by every rank as a FRESH child before it touches the GPU: rendezvous on the port it is given, ONE all_reduce of the
	rank ids on the backend the bench will use, the sum checked.  Exit 0 = this IPC setting works."""
	import datetime
	import signal
	rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
	rehearsal = os.environ.get("TTK_BENCH_REHEARSAL") == "1"
	probe = os.environ.get("TTK_BENCH_PROBE") == "1"
	if os.environ.get("TTK_BENCH_PREFLIGHT_FAIL_IPC") == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"):      # tests only: make one IPC setting "not work"
		print(f"[preflight] rank {rank}: failing on purpose (TTK_BENCH_PREFLIGHT_FAIL_IPC)", file=sys.stderr, flush=True)
		sys.exit(5)
	import torch
	import torch.distributed as dist
	signal.alarm(int(float(os.environ.get("TTK_BENCH_PREFLIGHT_S", "90"))))         # from here on (torch is imported): rendezvous + one collective, or SIGALRM ends the child
	if probe or rehearsal:
		dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
		x = torch.tensor([float(rank)])
	else:
		torch.cuda.set_device(local)
		dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"), timeout=datetime.timedelta(seconds=60))
		x = torch.tensor([float(rank)], device=f"cuda:{local}")
	dist.all_reduce(x)
	got = float(x.item())
	dist.destroy_process_group()
	want = world * (world - 1) / 2
	print(f"[preflight] rank {rank}: all_reduce of the rank ids = {got} (want {want}), HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}", file=sys.stderr, flush=True)
	sys.exit(0 if got == want else 4)


def preflight(rank, world):
	"""The pre-flight of this rank: a fresh child per attempt (the rank itself has not touched the GPU yet), HSA_ENABLE_IPC_MODE_LEGACY first as inherited
	(default 0: dmabuf IPC), then the other value.  Returns the value that passed; exits EXIT_PREFLIGHT with the children's output when neither does."""
	if os.environ.get("TTK_BENCH_NO_PREFLIGHT") == "1":
		return os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
	first = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
	order = [first, "1" if first == "0" else "0"]
	base = int(os.environ.get("MASTER_PORT", "29500"))
	for attempt, val in enumerate(order):
		env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=val, MASTER_PORT=str(base + 17 * (attempt + 1)))
		env.pop("TORCHELASTIC_USE_AGENT_STORE", None)          # the child rendezvouses on its own TCP store (rank 0 of the attempt hosts it), not the agent's
		t0 = time.monotonic()
		child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--preflight"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
		log(f"[pid] rank {rank} preflight child pid {child.pid}")
		try:
			_, err = child.communicate(timeout=400)
			rc = child.returncode
		except subprocess.TimeoutExpired:
			child.kill()
			_, err = child.communicate()
			rc = -9
		log(f"[preflight] rank {rank} attempt {attempt} (HSA_ENABLE_IPC_MODE_LEGACY={val}): exit {rc} after {time.monotonic() - t0:.1f}s")
		if rc == 0:
			return val
		log(f"[preflight] child output (last lines):\n" + "\n".join(err.splitlines()[-15:]))
	log(f"[preflight] rank {rank}: the one-collective pre-flight failed under both IPC settings {order}; not building models")
	sys.exit(EXIT_PREFLIGHT)


def recorded_pids(gpus):
	"""the pids the ranks (and their pre-flight children) logged to their rank files ("[pid] ... pid P"): only processes this run started"""
	import re
	pids = []
	for r in range(gpus):
		try:
			with open(rank_file(r), errors="replace") as f:
				pids += [int(m.group(1)) for ln in f if "[pid] " in ln for m in [re.search(r" pid (\d+)", ln)] if m]
		except OSError:
			pass
	return pids


def alive(pid):
	try:
		os.kill(pid, 0)
	except ProcessLookupError:
		return False
	except PermissionError:
		return True
	try:      # a zombie (exited, not yet reaped by its parent) no longer holds anything
		with open(f"/proc/{pid}/stat") as f:
			return f.read().rsplit(")", 1)[1].split()[0] != "Z"
	except OSError:
		return False


def teardown(proc, gpus, term_wait=None):
	"""End the launcher AND the ranks.  `os.killpg(proc.pid)` reaches only the torch.distributed.run agent: the elastic agent starts every worker with
	start_new_session=True, so the ranks and their pre-flight children live in other process groups; on SIGTERM the agent forwards the signal and waits up to 30 s
	before it kills its workers.  So: SIGTERM to the agent's group and to every pid the ranks recorded; wait longer than the agent's 30 s; SIGKILL whatever recorded
	pid is still alive (a rank wedged in the driver ignores SIGTERM), then the agent; report any pid that survives even that."""
	import signal
	term_wait = float(os.environ.get("TTK_BENCH_TERM_WAIT", "35")) if term_wait is None else term_wait
	pids = recorded_pids(gpus)

	def send(pid, sig, group=False):
		try:
			(os.killpg if group else os.kill)(pid, sig)
		except (ProcessLookupError, PermissionError):
			pass
	send(proc.pid, signal.SIGTERM, group=True)               # the process group this function started (start_new_session), nothing else
	for pid in pids:
		send(pid, signal.SIGTERM)
	t0 = time.monotonic()
	while time.monotonic() - t0 < term_wait and (proc.poll() is None or any(alive(p) for p in pids)):
		time.sleep(0.25)
	left = [p for p in pids if alive(p)]
	for pid in left:
		log(f"[parent watchdog] pid {pid} ignored SIGTERM for {term_wait:.0f}s: SIGKILL")
		send(pid, signal.SIGKILL)
	if proc.poll() is None:
		send(proc.pid, signal.SIGKILL, group=True)
		try:
			proc.wait(timeout=10)
		except subprocess.TimeoutExpired:
			pass
	time.sleep(0.5)
	still = [p for p in pids if alive(p)]
	if still:
		log(f"[parent watchdog] pids still alive after SIGKILL (they may hold a GPU): {still}")
	return still


def launcher_command(gpus, argv, port):
	"""the command `python bench.py --gpus N` turns itself into when it was started WITHOUT a torch.distributed environment: one child rank per
	GPU under torch.distributed.run (the same line the driver would use for N > 1), rendezvous on 127.0.0.1"""
	return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
			"--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def self_launch(a):
	"""`python bench.py --gpus N` (N > 1) as the driver starts the bench for N = 1: this process never touches the GPU (no torch import, no
	HIP call) -- it starts N fresh ranks as CHILD processes in their own process group (never an exec of a process that initialised the GPU), relays
	rank 0's JSON line and exits with the children's status.  While they run it is their watchdog: it follows the stage markers the ranks append to
	gpurun_out/rank{r}.err and, when a rank is overdue by its stage budget + PARENT_GRACE_S (the rank's own watchdog gets to speak first), terminates
	the child process group, prints every rank's last lines and exits non-zero."""
	import signal
	import threading
	with socket.socket() as sk:
		sk.bind(("127.0.0.1", 0))
		port = sk.getsockname()[1]
	env = dict(os.environ)
	env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver (the ranks' pre-flight tries the other value if this one fails)
	env.setdefault("OMP_NUM_THREADS", "4")
	cmd = launcher_command(a.gpus, sys.argv[1:], port)
	for r in range(a.gpus):
		try:
			os.remove(rank_file(r))
		except OSError:
			pass
	log(f"no torch.distributed environment and --gpus {a.gpus}: starting {a.gpus} ranks: {' '.join(cmd)}")
	proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
	lines = []

	def relay():
		for line in proc.stdout:
			line = line.rstrip("\n")
			if line.startswith("{") and '"metric"' in line:
				lines.append(line)
			else:
				print(line, file=sys.stderr, flush=True)      # anything else the ranks print is not the result line
	th = threading.Thread(target=relay, daemon=True)
	th.start()
	budgets = stage_budgets(a)
	names = [n for n, _ in budgets]
	reached = [0] * a.gpus                 # markers seen per rank
	since = [time.monotonic()] * a.gpus    # when the last one was seen
	overdue = None
	while proc.poll() is None and overdue is None:
		time.sleep(0.5)
		now = time.monotonic()
		for r in range(a.gpus):
			try:
				with open(rank_file(r), errors="replace") as f:
					n = sum(1 for ln in f if "[reached] " in ln and any(f"[reached] {m} " in ln for m in names))
			except OSError:
				n = 0
			if n > reached[r]:
				reached[r], since[r] = n, now
			if reached[r] < len(budgets) and now - since[r] > budgets[reached[r]][1] + PARENT_GRACE_S:
				overdue = (r, budgets[reached[r]][0], budgets[reached[r]][1])
	if overdue is not None:
		r, marker, budget = overdue
		log(f"[parent watchdog] rank {r} has not logged '{marker}' within {budget:.0f}s (+{PARENT_GRACE_S:.0f}s grace) of its previous marker: terminating the {a.gpus} child ranks")
		teardown(proc, a.gpus)
	rc = proc.wait()
	th.join(timeout=5)
	if overdue is not None:
		rc = EXIT_STAGE_OVERRUN
	if rc == 0 and len(lines) != 1:
		log(f"expected ONE result line from rank 0, got {len(lines)}")
		rc = 1
	if rc != 0:
		for r in range(a.gpus):
			log(f"---- last lines of rank {r} ({rank_file(r)}) ----\n{tail_of(rank_file(r)) or '(nothing logged)'}")
		return rc if 0 < rc < 256 else 1
	for line in lines[-1:]:
		print(line, flush=True)
	return rc


def launch_probe(a, mark):
	"""TTK_BENCH_PROBE=1 (tests/test_host_logic.py, no GPU): the ranks only rendezvous (gloo), count themselves and rank 0 prints a line --
	the launcher branch, the environment hand-over, the pre-flight, the stage markers / watchdogs and the relay of ONE line, exercised on a box without a
	GPU.  Not a measurement."""
	import datetime
	import torch.distributed as dist
	world = int(os.environ.get("WORLD_SIZE", "1"))
	if world > 1:
		dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
	mark("rendezvous ok")
	one = torch.ones(1)
	mark("models built")
	mark("timed region")
	if world > 1:
		dist.all_reduce(one)
	mark("timed done")
	if int(os.environ.get("RANK", "0")) == 0:
		print(json.dumps({"metric": "launcher probe (no measurement)", "value": None, "n_gpus": a.gpus, "n_ranks_seen": int(one.item()),
						  "world_size_env": world, "steps": a.steps, "warmup": a.warmup, "ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}), flush=True)
	mark("result")
	if world > 1:
		dist.destroy_process_group()


def main():
	a = parse()
	if a.preflight:
		return preflight_child(a)
	if "WORLD_SIZE" not in os.environ and a.gpus > 1:
		sys.exit(self_launch(a))
	rank = int(os.environ.get("RANK", "0"))
	world = int(os.environ.get("WORLD_SIZE", "1"))
	local = int(os.environ.get("LOCAL_RANK", "0"))
	wd = None
	if world > 1:      # nothing below this line has touched the GPU or imported torch yet
		global _RANK_FILE
		_RANK_FILE = rank_file(rank)
		open(_RANK_FILE, "w").close()
		log(f"[pid] rank {rank} pid {os.getpid()} pgid {os.getpgid(0)}")      # the parent's teardown signals these itself: the elastic agent starts its workers in sessions of their own
		os.environ.setdefault("NCCL_DEBUG", "WARN")
		os.environ.setdefault("NCCL_DEBUG_FILE", os.path.join(out_dir(), f"rccl.rank{rank}.log"))       # RCCL's own messages: a file per rank, never stdout (ONE JSON line goes there)
		if os.environ.get("TTK_BENCH_NO_RANK_WATCHDOG") != "1":      # (the parent-side watchdog's test switches the ranks' own off)
			wd = StageWatchdog(rank, world, a)
		os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = preflight(rank, world)
		log(f"[ipc] rank {rank} will rendezvous with HSA_ENABLE_IPC_MODE_LEGACY={os.environ['HSA_ENABLE_IPC_MODE_LEGACY']}")      # a disagreement between ranks is readable in the rank files, not inferred from a rendezvous timeout

	def mark(name):
		"""a stage marker: logged (stderr + the rank's file), and the budget of the next one armed.  TTK_BENCH_STALL_RANK / TTK_BENCH_STALL_AT make one rank
		hang in front of a marker -- the watchdogs' test (tests/test_host_logic.py), never set otherwise."""
		if os.environ.get("TTK_BENCH_STALL_AT") == name and int(os.environ.get("TTK_BENCH_STALL_RANK", "-1")) == rank:
			log(f"rank {rank}: stalling in front of '{name}' (TTK_BENCH_STALL_AT)")
			if os.environ.get("TTK_BENCH_STALL_IGNORE_TERM") == "1":      # tests only: a rank wedged so that SIGTERM does not end it (the case the parent's SIGKILL pass exists for)
				import signal
				signal.signal(signal.SIGTERM, signal.SIG_IGN)
				log(f"rank {rank}: ignoring SIGTERM")
			while True:
				time.sleep(1.0)
		if wd is not None:
			wd.reached(name)
		elif world > 1:
			log(f"[reached] {name} (rank {rank}, no rank watchdog)")
		elif name != "preflight ok":
			log(name)
	mark("preflight ok")
	global torch
	import torch
	if os.environ.get("TTK_BENCH_PROBE") == "1":
		return launch_probe(a, mark)
	import datetime
	if world != a.gpus:
		raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: start one rank per GPU (python bench.py --gpus N does it by itself)")
	# TTK_BENCH_REHEARSAL=1: every rank on cuda:0 with the gloo backend -- lets the N>1 control flow run on a 1-GPU box
	# (RCCL refuses two ranks on one device).  Never used by the driver; the number it prints is not a scaling result.
	rehearsal = os.environ.get("TTK_BENCH_REHEARSAL") == "1"
	if rehearsal:
		local = 0
	torch.cuda.set_device(local)
	dev = f"cuda:{local}"
	import torch.distributed as dist
	if world > 1:
		os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
		# 120 s, not the default 10 min (the driver's whole limit): a rendezvous that has not formed by then will not
		if rehearsal:
			dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
		else:
			dist.init_process_group("nccl", device_id=torch.device(dev), timeout=datetime.timedelta(seconds=120))
	mark("rendezvous ok")

	from tortoise_tts_amd import _lib, weights as W
	from tortoise_tts_amd.autoregressive import UnifiedVoice
	from tortoise_tts_amd.diffusion import DiffusionTTS
	from tortoise_tts_amd.inference import TTSHotPath
	_lib.load()
	ar_cfg, df_cfg = (W.AR_SMALL, W.DIFF_SMALL) if a.small else (W.AR_FULL, W.DIFF_FULL)
	by_cand = a.shard == "candidates"
	# configs[3]: per-GPU shard of 32 candidates, 2 lines x 256 text tokens, 500 mel tokens (T = 2176), 200 DDIM steps
	n_text, n_cand, n_mel, n_ddim, n_lines = (256, 32, 500, 200, 2) if by_cand else (TEXT_TOKENS, CANDIDATES, MEL_TOKENS, DDIM_STEPS, 1)
	if by_cand and world == 1:
		os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
		os.environ.setdefault("MASTER_PORT", "29533")
		os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
		dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(dev), timeout=datetime.timedelta(seconds=120))      # the sharded entry runs on a group of any size
	ar = UnifiedVoice(W.synth_state_dict(W.ar_shapes(ar_cfg), 0), ar_cfg, dtype=a.dtype, device=dev, max_batch=n_cand,
					  max_ctx=n_text + 4 + n_mel + 8)
	if a.no_graph:
		ar.use_graph = False
	df = DiffusionTTS(W.synth_state_dict(W.diffusion_shapes(df_cfg), 0), df_cfg, dtype=a.dtype, device=dev)
	voc = None
	if a.with_vocoder:
		from tortoise_tts_amd.vocoder import BigVGAN
		vcfg = W.VOC_SMALL if a.small else W.VOC_FULL
		voc = BigVGAN(W.synth_state_dict(W.vocoder_shapes(vcfg), 0), vcfg, dtype="f32" if a.dtype == "f32" else "bf16", device=dev)
	tts = TTSHotPath(ar, df, vocoder=voc)
	g = torch.Generator().manual_seed(1234 + (0 if by_cand else rank))     # candidate shards: every rank holds the SAME utterance
	lines = [torch.randint(1, 255, (1, n_text), generator=g).to(dev) for _ in range(n_lines)]
	text = lines[0]
	ar_lat = torch.randn(1, ar_cfg.model_dim, generator=g).to(dev)
	df_lat = torch.randn(1, 2 * df_cfg.model_channels, generator=g).to(dev)
	kw = dict(max_ar_steps=n_mel, max_diffusion_steps=n_ddim, ar_temp=0.8, candidates=n_cand,
			  suppress_tokens=[ar_cfg.stop_mel_token], return_all=True)
	gdev = "cpu" if rehearsal else dev
	gathered = [torch.empty((CANDIDATES, MEL_TOKENS), dtype=torch.long, device=gdev) for _ in range(world)] if world > 1 and not by_cand else None

	last = {}        # --dump-outputs: what the latest step returned, name -> tensor

	def step(exchange=True, marks=None):
		if by_cand:     # one long-form utterance: its lines sampled one after the other, each with its candidates sharded over the ranks; the lines' winners
			# are diffused as one ragged batch on their owner (TTSHotPath.inference_sharded_lines: each line's mel equals its own call's)
			skw = {k: v for k, v in kw.items() if k != "candidates"}
			res = tts.inference_sharded_lines(lines, ar_lat, df_lat, candidates=n_cand * world, phase_marks=marks, **skw)
			if a.dump_outputs:
				last.clear()
				for i, (m, _, x) in enumerate(res):
					last.update({f"line{i}_mels": m, **{f"line{i}_{k}": v for k, v in x.items()}})
			return sum(r[1] for r in res)
		mels, seconds, aux = tts.inference(text, ar_lat, df_lat, phase_marks=marks, **kw)
		wav = None
		if voc is not None:
			wav = voc.inference(mels)
		if a.dump_outputs:
			last.clear()
			last.update(mels=mels, wav=wav, **aux)
		if world > 1 and exchange:   # hand the candidate ids to the scoring rank (RCCL all-gather over xGMI, 32 KB per rank)
			dist.all_gather(gathered, aux["codes"].contiguous().to(gdev))
		return seconds

	def fence():
		if world > 1:
			dist.barrier()
		torch.cuda.synchronize()

	mark("models built")
	for _ in range(a.warmup):
		step()
	fence()
	mark("timed region")
	t0 = time.perf_counter()
	audio = 0.0
	for _ in range(a.steps):
		audio += step()
	fence()
	dt = time.perf_counter() - t0
	tmax = torch.tensor([dt], dtype=torch.float64, device=gdev)
	if world > 1:
		dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
	dt = float(tmax.item())

	mark("timed done")
	log(f"timed {a.steps} steps in {dt:.3f}s")
	if a.dump_outputs and rank == 0:
		log(f"outputs of the last timed step: {dump_outputs(last, a.dump_outputs)}")
	roof = None
	if a.full and not a.no_roofline and (rank == 0 or by_cand):
		# configs[1]/[2]: rank 0 alone (no collective in these passes).  configs[3]: the sharded step IS collectives, so every rank runs the two
		# extra steps and rank 0 reports its own GPU's phases (it owns the diffused candidate: no scorer is attached, candidate 0 wins).
		from tortoise_tts_amd import profiling
		marks = []
		step(exchange=False, marks=marks)                  # one more step, run exactly as the timed ones, with events at the phase boundaries
		torch.cuda.synchronize()
		roof = profiling.dominant_kernel_roofline(lambda: step(exchange=False), ar, df)
		if not a.small and rank == 0:      # only rank 0 reports; a shard that diffused no line has no "ddim" interval (phase_roofline says so instead of raising)
			roof["phases"] = phase_roofline(marks, a.dtype, n_text, n_cand, n_mel, n_ddim) if by_cand else phase_roofline([marks], a.dtype)
	# informational, never `value`: the k = 1 variant SURVEY.md 8d row 2 asks to be reported beside the headline -- the candidate is chosen first and
	# only its row goes through the dense latent pass (same bits out; the reference runs all 16, inference.py:370-379, and so does `value`)
	k1 = None
	if a.full and rank == 0 and world == 1 and not a.no_roofline and not by_cand:
		kw1 = dict(kw, latents_for="winner")
		tts.inference(text, ar_lat, df_lat, **kw1)
		torch.cuda.synchronize()
		t1 = time.perf_counter()
		sec = sum(tts.inference(text, ar_lat, df_lat, **kw1)[1] for _ in range(2))
		torch.cuda.synchronize()
		d1 = time.perf_counter() - t1
		k1 = {"value": sec / d1, "unit": "audio-sec/wall-sec", "ms_per_step": 1e3 * d1 / 2, "note": "latent pass on the diffused candidate only; not the headline metric"}
	# informational, never `value`: a stream of utterances through TTSHotPath.inference_lines -- the sampling of 4 consecutive lines as ONE
	# decode batch (weights streamed once per token for all of them), line i's diffusion overlapped with later lines' sampling; results
	# identical to the per-line calls.  Built on its own handle (max_batch = 4 x candidates) AFTER the headline was measured; `value` above
	# stays the one-utterance-at-a-time figure of configs[1].
	piped = None
	if a.full and rank == 0 and world == 1 and not a.no_roofline and not by_cand:
		n_lines, per_batch = 8, 4
		lens = [64, 48, 88, 56, 72, 40, 80, 64][:n_lines]          # text lengths vary from line to line (mean 64): one captured token step serves them all
		gl = torch.Generator().manual_seed(4321)
		ltexts = [torch.randint(1, 255, (1, n), generator=gl).to(dev) for n in lens]
		ar4 = UnifiedVoice(W.synth_state_dict(W.ar_shapes(ar_cfg), 0), ar_cfg, dtype=a.dtype, device=dev, max_batch=per_batch * n_cand,
						   max_ctx=max(lens) + 4 + n_mel + 8)
		tts4 = TTSHotPath(ar4, df)
		lkw = {k: v for k, v in kw.items() if k != "return_all"}
		tts4.inference_lines(ltexts[:per_batch], ar_lat, df_lat, ar_batch_lines=per_batch, **lkw)
		torch.cuda.synchronize()
		t1 = time.perf_counter()
		res = tts4.inference_lines(ltexts, ar_lat, df_lat, ar_batch_lines=per_batch, **lkw)
		torch.cuda.synchronize()
		dl = time.perf_counter() - t1
		piped = {"value": sum(r[1] for r in res) / dl, "unit": "audio-sec/wall-sec", "lines": n_lines, "text_tokens": lens, "ar_batch_lines": per_batch, "ms_per_line": 1e3 * dl / n_lines,
				 "note": "stream of utterances: 4 lines sampled as one decode batch, diffusion pipelined under the next batch; not the headline metric"}
		del tts4, ar4
	# informational, never `value`: the loop real utterances run.  The headline suppresses the stop token (fixed length), so
	# HF's stopping test is compiled out of its loop (`can_stop` False).  Here the stop token is NOT suppressed but unreachable -- mel_head.bias[stop] = -1e9 in
	# a second handle's synthetic weights, so its probability is exactly 0, the length stays 250 and the ids must equal the headline's -- and the loop runs
	# with the stopping test live: one event per token, the pinned flag read LAG tokens late (autoregressive.py `_token_loop`).
	live = None
	if a.full and rank == 0 and world == 1 and not a.no_roofline and not by_cand:
		sd = W.synth_state_dict(W.ar_shapes(ar_cfg), 0)
		sd["mel_head.bias"] = sd["mel_head.bias"].clone()
		sd["mel_head.bias"][ar_cfg.stop_mel_token] = -1e9
		ar_l = UnifiedVoice(sd, ar_cfg, dtype=a.dtype, device=dev, max_batch=n_cand, max_ctx=n_text + 4 + n_mel + 8)
		del sd
		tts_l = TTSHotPath(ar_l, df, vocoder=voc)
		kwl = {k: v for k, v in kw.items() if k != "suppress_tokens"}
		ref_codes = tts.inference(text, ar_lat, df_lat, **kw)[2]["codes"]
		got_codes = tts_l.inference(text, ar_lat, df_lat, **kwl)[2]["codes"]      # (also the warm-up: captures this handle's token step)
		torch.cuda.synchronize()
		n_live = max(2, min(a.steps, 5))
		t1 = time.perf_counter()
		sec = sum(tts_l.inference(text, ar_lat, df_lat, **kwl)[1] for _ in range(n_live))
		torch.cuda.synchronize()
		dl = time.perf_counter() - t1
		live = {"value": sec / dl, "unit": "audio-sec/wall-sec", "ms_per_step": 1e3 * dl / n_live, "steps": n_live,
				"ids_equal_headline": bool(got_codes.shape == ref_codes.shape and torch.equal(got_codes, ref_codes)), "mel_tokens": int(got_codes.shape[1]),
				"note": "stop token live (not suppressed, unreachable through mel_head.bias[stop] = -1e9): HF's per-token stopping test runs as the lagged pinned flag; not the headline metric"}
		del tts_l, ar_l
	cpu = None
	if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline and not a.small:
		log("roofline pass done; cpu baseline")
		cpu = cpu_baseline(1234, n_text, n_cand, n_mel, n_ddim, n_lines, light=True) if by_cand else cpu_baseline(1234)

	if rank == 0:
		cfg_line = {"workload": "configs[1]: 1 utterance/GPU, 64 text tokens, 16 AR candidates x 250 mel tokens (KV-cached decode), "
								"latent pass on 16 candidates, 80 DDIM steps with cond-free guidance at T=1088 (11.6 s audio)",
					"text_tokens": TEXT_TOKENS, "candidates": CANDIDATES, "mel_tokens": MEL_TOKENS, "ddim_steps": DDIM_STEPS,
					"mel_frames": MEL_TOKENS * 4 * 24000 // 22050, "parallelism": f"utterances x{world}" if world > 1 else "single GPU",
					"small_models": bool(a.small), "vocoder_in_step": bool(a.with_vocoder)}
		if a.dtype in ("fp8", "fp8w"):      # BASELINE config 5: say exactly which contractions are fp8
			cfg_line["workload"] += ("; config 5 arithmetic: " + (
				"diffusion ResBlock convolutions (in_layers.2, out_layers.3) and AttentionBlock proj_out on the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales "
				"(e4m3 weights x power-of-two tensor scale in the epilogue, e4m3 activations); the q / k / v projection, QK^T / PV, the k=3 input/output convs and the time-embedding "
				"linears on the bf16 MFMA; autoregressive side: fp8 WEIGHT bytes widened next to the bf16 MFMA (16-row GEMVs), bf16 KV cache" if a.dtype == "fp8" else
				"fp8-e4m3 block-GEMM WEIGHTS in both networks (power-of-two tensor scale; the diffusion q / k / v projection keeps bf16 weights), every contraction on the bf16 MFMA"))
			cfg_line["fp8_contractions"] = "diffusion ResBlock convolutions + proj_out (scaled 16x16x128 MFMA)" if a.dtype == "fp8" else "none (weights only)"
			cfg_line["ar_handle_dtype"] = "fp8w"
		if by_cand:
			cfg_line = {"workload": f"configs[3]: one long-form utterance = 2 lines x 256 text tokens, {n_cand * world} AR candidates ({n_cand} per GPU) x 500 mel "
									"tokens, latent pass + candidate choice on every shard, 200 DDIM steps with cond-free guidance at T=2176 (23.2 s audio per line), "
									"the lines' diffusions spread over the GPUs (latents + start noise broadcast from the winner's GPU); ids / scores all-gathered and the mels broadcast over RCCL",
						"text_tokens": n_text, "candidates": n_cand * world, "mel_tokens": n_mel, "ddim_steps": n_ddim, "lines": n_lines,
						"mel_frames": n_mel * 4 * 24000 // 22050, "parallelism": f"candidates x{world}", "small_models": bool(a.small)}
		line = {
			"metric": "audio-sec/wall-sec (RTF^-1), 16 AR candidates x 80 DDIM steps" if not by_cand else "audio-sec/wall-sec (RTF^-1), 32 AR candidates per GPU x 200 DDIM steps (configs[3])",
			"value": (1 if by_cand else world) * audio / dt,
			"unit": "audio-sec/wall-sec", "n_gpus": world, "n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
			"backend": dist.get_backend() if dist.is_initialized() else None, "steps": a.steps, "warmup": a.warmup,
			"ms_per_step": 1e3 * dt / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
			"dtype": a.dtype, "data": "synthetic",
			"config": cfg_line,
			"roofline": roof, "cpu_baseline": cpu, "latent_k1_variant": k1, "pipelined_lines": piped, "stop_live": live,
		}
		print(json.dumps(line), flush=True)
	mark("result")
	if wd is not None:
		wd.stop()
	if dist.is_initialized():
		dist.destroy_process_group()


if __name__ == "__main__":
	main()
