"""Host statement of the run-time LoRA update (csrc/lora.hip; DESIGN.md "Run-time LoRA"), bit for bit: numpy f32, every product and every
sum rounded on its own, the rank walked upwards.  `fold` is what ttk_ar_lora_set leaves in a matrix; `fold_state_dict` builds the weights a
fresh handle is created from when a switched handle is compared with it; `synth_adapter` makes adapters whose lora_B is not the reference's
zero initialisation (which would hide every mistake)."""
import numpy as np
import torch

PARAM = ".parametrizations.weight.0."
MODULES = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")


def fold(W0, A, B, s):
	"""W0 [K, N], A = lora_A [rank, N], B = lora_B [K, rank], s = alpha / rank  ->  W0 + (B A) s as the kernel rounds it"""
	W0, A, B = (np.ascontiguousarray(np.asarray(x, dtype=np.float32)) for x in (W0, A, B))
	assert A.shape[0] == B.shape[1] and W0.shape == (B.shape[0], A.shape[1])
	acc = np.zeros_like(W0)
	for r in range(A.shape[0]):
		acc = acc + B[:, r:r + 1] * A[r:r + 1, :]      # two ufuncs: the product is rounded to f32 before the sum
	return W0 + acc * np.float32(s)


def modules(layers):
	return [f"gpt.h.{l}.{m}" for l in range(layers) for m in MODULES]


def synth_adapter(shapes, rank, seed, modules):
	"""{<module>.parametrizations.weight.0.lora_A: [rank, N], ...lora_B: [K, rank]} for the given modules of a model with `shapes`
	(weights.ar_shapes); (B A) has a standard deviation of about 0.02 at every rank"""
	g = torch.Generator().manual_seed(seed)
	out = {}
	for m in modules:
		K, N = shapes[m + ".weight"]
		out[m + PARAM + "lora_A"] = torch.randn(rank, N, generator=g) * (0.2 / rank ** 0.5)
		out[m + PARAM + "lora_B"] = torch.randn(K, rank, generator=g) * 0.1
	return out


def fold_state_dict(sd, adapter, s):
	"""`sd` with `fold` applied to every module `adapter` covers"""
	out = dict(sd)
	for k in adapter:
		if k.endswith("lora_A"):
			m = k[:-len(PARAM + "lora_A")]
			out[m + ".weight"] = torch.from_numpy(fold(sd[m + ".weight"].numpy(), adapter[k].numpy(), adapter[m + PARAM + "lora_B"].numpy(), s))
	return out
