"""Diagnostic: digest of the diffusion network's outputs under the library TTK_LIB selects, so that two builds of libttk can be compared bit for bit on ONE box:
    TTK_LIB=a.so python tests/diag/lib_bits.py > a.txt;  TTK_LIB=b.so python tests/diag/lib_bits.py > b.txt;  diff a.txt b.txt
Per (dtype, T): one evaluation and a 3-step DDIM loop.  Then every other way into csrc/diff.hip: the small configuration (C < 1024: the generic GroupNorm-apply), the fp8
modes, loops without and with mixed conditioning-free guidance, the p sampler, timestep_independent (the row gather), a ragged line batch (one length no multiple of 64),
the begin + step loop and the sequential loop (TTK_DIFF_PIPE=0).  Arguments `dtype:T ...` restrict the run to the first part with those cases."""
import ctypes, hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import _lib, weights as W
from tortoise_tts_amd.diffusion import DiffusionTTS, get_diffuser
dev = "cuda:0"
for name in [n for n in _lib.SYMBOLS if not hasattr(ctypes.CDLL(_lib.LIB_PATH), n)]: del _lib.SYMBOLS[name]      # an older build under TTK_LIB: what this script calls, it has
h = lambda t: hashlib.sha256(t.float().cpu().numpy().tobytes()).hexdigest()[:16]


def rnd(seed, *shape):
	return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def show(tag, **outs):
	torch.cuda.synchronize()
	print(f"{tag}: " + " ".join(f"{k} {h(v)}" for k, v in outs.items()) + f" finite {all(bool(torch.isfinite(v).all()) for v in outs.values())}", flush=True)


def loop(m, d, noise, E, sampler="ddim"):
	torch.manual_seed(11)      # the p sampler draws its noise from the device generator
	return d.sample_loop(m, tuple(noise.shape), sampler=sampler, noise=noise, model_kwargs={"precomputed_aligned_embeddings": E})


def steps_loop(m, steps, noise, E, entry="loop"):
	"""a hand-built ttk_step array through the whole-loop entry, or one ttk_diff_step call per step behind ttk_diff_begin"""
	x, T, n = noise.clone(), noise.shape[-1], len(steps)
	if entry == "loop":
		_lib.check(m.lib.ttk_diff_sample_ddim(m._h, x.data_ptr(), E.data_ptr(), 1, T, (_lib.StepC * n)(*steps), n, _lib.stream_ptr()), "ttk_diff_sample_ddim")
	else:
		_lib.check(m.lib.ttk_diff_begin(m._h, E.data_ptr(), 1, T, _lib.stream_ptr()), "ttk_diff_begin")
		for st in reversed(steps):
			_lib.check(m.lib.ttk_diff_step(m._h, x.data_ptr(), ctypes.byref(st), None, _lib.stream_ptr()), "ttk_diff_step")
	return x


def mixed(n=5, off=(1, 2)):
	"""an n-step schedule whose entries `off` have no conditioning-free evaluation: both batch layouts, and every change between them"""
	d = get_diffuser(steps=n, cond_free=True)
	steps = [d.step_coefs(i, "ddim") for i in range(n)]
	for i in off:
		steps[i].cfk = -1.0
	return steps


def basic(m, tag, T, C=1024):
	noise, E = rnd(3, 1, 100, T), rnd(4, 1, C, T)
	y = m(noise, torch.tensor([900], device=dev), precomputed_aligned_embeddings=E)
	show(tag, eval=y, ddim3=loop(m, get_diffuser(steps=3, cond_free=True), noise, E))


sd = W.synth_state_dict(W.diffusion_shapes(W.DIFF_FULL), 1)
cases = [("bf16", 1088), ("bf16", 1000), ("bf16", 320), ("bf16", 1216), ("bf16", 2176), ("f16", 1088), ("f32", 320), ("fp8w", 1088), ("fp8", 1088)]
only_basic = len(sys.argv) > 1
if only_basic: cases = [(c.split(":")[0], int(c.split(":")[1])) for c in sys.argv[1:]]
with torch.inference_mode():
	m, have = None, None
	for dtype, T in cases:
		if dtype != have:
			del m
			m, have = DiffusionTTS(sd, W.DIFF_FULL, dtype=dtype, device=dev), dtype
		basic(m, f"{dtype} T={T}", T)
	del m
	if only_basic: sys.exit(0)
	small = W.synth_state_dict(W.diffusion_shapes(W.DIFF_SMALL), 6)
	for dtype in ("f32", "bf16"):
		basic(DiffusionTTS(small, W.DIFF_SMALL, dtype=dtype, device=dev), f"small {dtype} T=100", 100, W.DIFF_SMALL.model_channels)
	for pipe in ("1", "0"):
		os.environ["TTK_DIFF_PIPE"] = pipe      # read when the handle is made
		m = DiffusionTTS(sd, W.DIFF_FULL, dtype="bf16", device=dev)
		tag = f"bf16 pipe={pipe}"
		for T in (1088, 200):
			noise, E = rnd(3, 1, 100, T), rnd(4, 1, 1024, T)
			show(f"{tag} T={T}", no_cf=loop(m, get_diffuser(steps=3, cond_free=False), noise, E), mixed=steps_loop(m, mixed(), noise, E),
				 p=loop(m, get_diffuser(steps=3, cond_free=True), noise, E, "p"), p_no_cf=loop(m, get_diffuser(steps=2, cond_free=False), noise, E, "p"),
				 step_calls=steps_loop(m, mixed(4, (2,)), noise, E, "steps"), ddim3=loop(m, get_diffuser(steps=3, cond_free=True), noise, E))
		Ts = [320, 200, 128]
		lines = get_diffuser(steps=3, cond_free=True).sample_loop_lines(m, [rnd(20 + i, 1, 100, t) for i, t in enumerate(Ts)], [rnd(30 + i, 1, 1024, t) for i, t in enumerate(Ts)])
		show(f"{tag} lines {Ts}", **{f"T{t}": x for t, x in zip(Ts, lines)})
		show(f"{tag} timestep_independent", M250_T1088=m.timestep_independent(rnd(5, 1, 250, 1024), rnd(6, 1, 2048), 1088), b2_M33_T150=m.timestep_independent(rnd(7, 2, 33, 1024), rnd(8, 2, 2048), 150))
		del m
