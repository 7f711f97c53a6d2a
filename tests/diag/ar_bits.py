"""Diagnostic: digests of the AR handle's forced decode under the library TTK_LIB selects, so that two builds of libttk can be compared bit for bit on ONE box:
   TTK_LIB=a.so python tests/diag/ar_bits.py > a.txt;  TTK_LIB=b.so python tests/diag/ar_bits.py > b.txt;  diff a.txt b.txt
Per case: SHA-256 of the prefill logits and of each of 6 forced decode steps' logits, and of a 7th step's.  The C ABI has no accessor for the KV cache (and an older
library could not be given one), so the K / V rows the six steps append are digested through their reader: every row appended by steps 1..6 is a key and a value of
step 7's attention in all layers, whose logits are the `kv7` digest.  Cases: AR_FULL in every dtype at 16 rows and 17 (second row tile, padding rows), AR_SMALL
(k_skinny only), the LayerNorm-prologue form (TTK_AR_LNFOLD=0), and one two-line batch through ttk_ar_prefill_lines."""
import hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.autoregressive import UnifiedVoice
dev = "cuda:0"
STEPS, NTEXT = 6, 24
# (model, dtype, rows, TTK_AR_LNFOLD, lines)
cases = [("full", dt, B, "1", 1) for dt in ("bf16", "f16", "fp8w", "f32") for B in (16, 17)]
cases += [("small", "bf16", 3, "1", 1), ("small", "f32", 3, "1", 1), ("full", "bf16", 16, "0", 1), ("small", "f32", 3, "0", 1), ("full", "bf16", 16, "1", 2)]
cfgs = {"full": W.AR_FULL, "small": W.AR_SMALL}
sds = {}
h = lambda t: hashlib.sha256(t.float().cpu().numpy().tobytes()).hexdigest()[:16]
for name, dtype, B, fold, lines in cases:
	cfg = cfgs[name]
	if name not in sds: sds[name] = W.synth_state_dict(W.ar_shapes(cfg), 0)
	os.environ["TTK_AR_LNFOLD"] = fold      # read by ttk_ar_create
	m = UnifiedVoice(sds[name], cfg, dtype=dtype, device=dev, max_batch=B, max_ctx=NTEXT + 9 + 4 + STEPS + 4)
	g = torch.Generator().manual_seed(5)
	cond = torch.randn(1, cfg.model_dim, generator=g).to(dev)
	texts = [torch.randint(1, 255, (1, NTEXT + 9 * i), generator=g).to(dev) for i in range(lines)]
	toks = torch.randint(0, 8192, (B, STEPS + 1), generator=g).to(dev)
	with torch.inference_mode():
		logits = m._prefill(cond, texts[0], B) if lines == 1 else m._prefill_lines(cond, texts, B // lines)
		d = [h(logits)]
		for k in range(STEPS + 1):
			m._decode(toks[:, k].contiguous(), logits)
			d.append(h(logits))
		torch.cuda.synchronize()
		ok = bool(torch.isfinite(logits).all())
	print(f"{name} {dtype} B={B} lnfold={fold} lines={lines}: prefill {d[0]} steps {' '.join(d[1:-1])} kv7 {d[-1]} finite {ok}", flush=True)
	del m
