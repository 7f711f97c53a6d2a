"""ctypes binding of libttk.so (include/ttk.h).  The product path has NO fallback: if the library is missing or a
call fails, an exception is raised -- nothing here or above ever routes through torch ops or the oracle instead."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, List, Sequence

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTK_LIB") or os.path.join(HERE, "libttk.so")   # TTK_LIB: A/B runs of an experimental build

TTK_F32, TTK_BF16 = 0, 1
TTK_F16 = 4
TTK_FP8W = 2
TTK_FP8 = 3      # diffusion handle only: fp8 activations into the block GEMMs as well (fp8 MFMA); elsewhere it means fp8w
DTYPES = {"f32": TTK_F32, "fp32": TTK_F32, "float32": TTK_F32, "bf16": TTK_BF16, "bfloat16": TTK_BF16, "f16": TTK_F16, "fp16": TTK_F16, "float16": TTK_F16, "half": TTK_F16, "fp8w": TTK_FP8W, "fp8": TTK_FP8}


class TTKError(RuntimeError):
	pass


class WeightView(C.Structure):
	_fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4)]


class ARConfigC(C.Structure):
	_fields_ = [(n, C.c_int) for n in (
		"layers", "model_dim", "heads", "max_mel_seq_len", "max_text_seq_len", "number_text_tokens_p1", "number_mel_codes",
		"start_text_token", "stop_text_token", "start_mel_token", "stop_mel_token", "dtype", "max_batch", "max_ctx")]


class DiffConfigC(C.Structure):
	_fields_ = [(n, C.c_int) for n in (
		"model_channels", "num_layers", "in_channels", "in_latent_channels", "out_channels", "num_heads", "dtype")]


class CondConfigC(C.Structure):
	_fields_ = [(n, C.c_int) for n in ("in_channels", "channels", "num_heads", "num_blocks", "stem", "relpos", "pool", "dtype")]


class StepC(C.Structure):
	_fields_ = [("t", C.c_int64)] + [(n, C.c_float) for n in (
		"sqrt_recip_ac", "sqrt_recipm1_ac", "sqrt_ac_prev", "sqrt_1m_ac_prev", "coef1", "coef2", "min_log", "max_log", "cfk")] + [
		("sampler", C.c_int), ("nonzero", C.c_int)]


class StepExtC(C.Structure):
	"""ttk_step_ext (include/ttk.h; static_assert'ed in csrc/diff.hip)"""
	_fields_ = [(n, C.c_float) for n in ("sigma", "dir", "sqrt_ac_next", "sqrt_1m_ac_next")] + [("mode", C.c_int), ("clip", C.c_int)]


class StepMsC(C.Structure):
	"""ttk_step_ms (include/ttk.h; static_assert'ed in csrc/diff.hip)"""
	_fields_ = [(n, C.c_float) for n in ("c_x", "c_d0", "c_d1")] + [("clip", C.c_int)]


class SampleArgs(C.Structure):
	"""ttk_sample_args (include/ttk.h)"""
	_fields_ = [("scores", C.c_void_p), ("ld", C.c_int64), ("B", C.c_int), ("V", C.c_int), ("q", C.c_void_p), ("ldq", C.c_int64),
				("suppress", C.c_void_p), ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float),
				("repetition_penalty", C.c_float), ("stop_token", C.c_int64), ("unfinished", C.c_void_p), ("tok", C.c_void_p),
				("ids", C.c_void_p), ("ids_ld", C.c_int64), ("ids_cols", C.c_int64), ("col", C.c_void_p), ("history", C.c_void_p),
				("hist_ld", C.c_int64), ("hist_off", C.c_int64), ("live_rows", C.c_void_p), ("all_done", C.c_void_p), ("typical_mass", C.c_float)]


class SampleExt(C.Structure):
	"""ttk_sample_ext (include/ttk.h; static_assert'ed in csrc/sample_ext.hip)"""
	_fields_ = [(n, C.c_float) for n in ("repetition_penalty_decay", "stop_length_penalty", "min_temperature", "mirostat_tau", "mirostat_eta")] + [
		("mirostat_mu", C.c_void_p), ("mirostat_k", C.c_void_p), ("temp_out", C.c_void_p), ("scores_out", C.c_void_p), ("scores_out_ld", C.c_int64)]


class BeamArgs(C.Structure):
	"""ttk_beam_args (include/ttk.h)"""
	_fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("num_beams", C.c_int), ("V", C.c_int), ("q", C.c_void_p), ("suppress", C.c_void_p),
				("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("repetition_penalty", C.c_float), ("length_penalty", C.c_float),
				("stop_token", C.c_int64), ("prefix_ids", C.c_int64 * 2), ("max_new", C.c_int), ("col", C.c_void_p), ("seqs", C.c_void_p),
				("scores", C.c_void_p), ("state", C.c_void_p), ("acc", C.c_void_p), ("work", C.c_void_p), ("tok", C.c_void_p), ("beam_idx", C.c_void_p),
				("all_done", C.c_void_p)]


class GemmSeg(C.Structure):
	"""ttk_gemm_seg (include/ttk.h)"""
	_fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("shift", C.c_int), ("w_off", C.c_int64)]


class GemmDesc(C.Structure):
	"""ttk_gemm_desc (include/ttk.h)"""
	_fields_ = [("nseg", C.c_int), ("seg", GemmSeg * 12), ("W", C.c_void_p), ("ldw", C.c_int64), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
				("rows_per_batch", C.c_int), ("act", C.c_int), ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int64),
				("C", C.c_void_p), ("ldc", C.c_int64), ("out_scale", C.c_float), ("out_f32", C.c_int), ("transpose_out", C.c_int),
				("gn_T", C.c_int), ("gn_part", C.c_void_p)]


class AttnDesc(C.Structure):
	"""ttk_attn_desc (include/ttk.h)"""
	_fields_ = [("qkv", C.c_void_p), ("ld", C.c_int64), ("q_off", C.c_int), ("k_off", C.c_int), ("v_off", C.c_int), ("head_stride", C.c_int),
				("out", C.c_void_p), ("ldo", C.c_int64), ("out_f8", C.c_int), ("nb", C.c_int), ("T", C.c_int), ("H", C.c_int), ("causal", C.c_int),
				("tlen", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_float), ("form", C.c_int)]


class AttnDecodeDesc(C.Structure):
	"""ttk_attn_decode_desc (include/ttk.h)"""
	_fields_ = [("qbuf", C.c_void_p), ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("d_pos", C.c_void_p),
				("B", C.c_int), ("H", C.c_int), ("max_ctx", C.c_int), ("out_frag", C.c_int), ("out", C.c_void_p), ("row_info", C.c_void_p),
				("shared_rows", C.c_int), ("variant", C.c_int), ("pos_line", C.c_int)]


class AttnProbsDesc(C.Structure):
	"""ttk_attn_probs_desc (include/ttk.h; static_assert'ed in csrc/align.hip)"""
	_fields_ = [("qkv", C.c_void_p), ("ld", C.c_int64), ("q_off", C.c_int), ("k_off", C.c_int), ("head_stride", C.c_int), ("nb", C.c_int), ("T", C.c_int),
				("H", C.c_int), ("scale", C.c_float), ("n_sel", C.c_int), ("heads", C.c_void_p), ("out", C.c_void_p), ("r0", C.c_int), ("R", C.c_int),
				("c0", C.c_int), ("C", C.c_int)]


class GnDesc(C.Structure):
	"""ttk_gn_desc (include/ttk.h)"""
	_fields_ = [("x", C.c_void_p), ("ms", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
				("ss_stride", C.c_int64), ("row_idx", C.c_void_p), ("tlen", C.c_void_p), ("nb", C.c_int), ("T", C.c_int), ("Tout", C.c_int), ("C", C.c_int),
				("act", C.c_int), ("out", C.c_void_p), ("out_f32", C.c_int), ("out_f8", C.c_int), ("pf", C.c_void_p), ("pf_bytes", C.c_int64),
				("pf_taps", C.c_int), ("stats", C.c_int), ("form", C.c_int)]


class LnDesc(C.Structure):
	"""ttk_ln_desc (include/ttk.h)"""
	_fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("rows", C.c_int), ("d", C.c_int), ("g1", C.c_void_p), ("b1", C.c_void_p), ("g2", C.c_void_p),
				("b2", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64), ("out_f32", C.c_int), ("frag", C.c_int), ("out2", C.c_void_p),
				("out2_idx", C.c_void_p), ("out2_stride", C.c_int64), ("out2_base", C.c_void_p)]


class LvcDesc(C.Structure):
	"""ttk_lvc_desc (include/ttk.h)"""
	_fields_ = [("y", C.c_void_p), ("kern", C.c_void_p), ("kbias", C.c_void_p), ("x", C.c_void_p), ("at", C.c_void_p)] + \
			   [(n, C.c_int) for n in ("B", "L", "CG", "hop", "Tc", "layer", "n_layers", "lda")]


class HifiConvDesc(C.Structure):
	"""ttk_hifi_conv_desc (include/ttk.h)"""
	_fields_ = [("a", C.c_void_p), ("lda", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p), ("L", C.c_int), ("C", C.c_int), ("k", C.c_int), ("dil", C.c_int),
				("mode", C.c_int), ("xres", C.c_void_p), ("xout", C.c_void_p), ("at_out", C.c_void_p), ("ldo", C.c_int), ("mrf", C.c_void_p)]


class GemvMatConfigC(C.Structure):
	"""ttk_gemv_mat_config (include/ttk.h)"""
	_fields_ = [(n, C.c_int) for n in ("dtype", "layout", "N", "K")]


class GemvDesc(C.Structure):
	"""ttk_gemv_desc (include/ttk.h)"""
	_fields_ = [("dtype", C.c_int), ("role", C.c_int), ("form", C.c_int), ("M", C.c_int), ("a", C.c_void_p), ("x", C.c_void_p),
				("g1", C.c_void_p), ("b1", C.c_void_p), ("g2", C.c_void_p), ("b2", C.c_void_p), ("out_f32", C.c_void_p), ("out_T", C.c_void_p),
				("qbuf", C.c_void_p), ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("max_ctx", C.c_int), ("H", C.c_int), ("q_scale", C.c_float),
				("bump", C.c_int), ("d_pos", C.c_void_p), ("noise", C.c_void_p), ("rng", C.c_void_p), ("draws", C.c_void_p), ("health", C.c_void_p),
				("launched", C.POINTER(C.c_int)), ("family", C.c_int), ("waves", C.c_int), ("model_dim", C.c_int)]


class ProfResult(C.Structure):
	_fields_ = [("ms", C.c_double), ("launches", C.c_int64), ("work", C.c_double)]


# every symbol include/ttk.h declares: (restype, argtypes)
_P, _I, _L = C.c_void_p, C.c_int, C.c_int64
SYMBOLS = {
	"ttk_version": (_I, []),
	"ttk_last_error": (C.c_char_p, []),
	"ttk_prof_begin": (_I, []),
	"ttk_prof_end": (_I, [C.POINTER(ProfResult), _I]),
	"ttk_ar_create": (_I, [C.POINTER(_P), C.POINTER(ARConfigC), C.POINTER(WeightView), _I]),
	"ttk_ar_destroy": (_I, [_P]),
	"ttk_ar_prefill": (_I, [_P, _P, _I, _P, _I, _I, _P, _P]),
	"ttk_ar_prefill_prompted": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P]),
	"ttk_ar_decode": (_I, [_P, _P, _P, _P, _P]),
	"ttk_ar_decode_next": (_I, [_P, _P, _P, _P]),
	"ttk_ar_last_hidden": (_I, [_P, _P, _P]),
	"ttk_ar_set_hidden_ring": (_I, [_P, _P, _P, _L, _P]),
	"ttk_ar_health": (_I, [_P, C.POINTER(C.c_int), _P]),
	"ttk_ar_set_noise": (_I, [_P, _P, _P, _P]),
	"ttk_ar_prefill_lines": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
	"ttk_graph_launch": (_I, [_P, _P]),
	"ttk_exponential_like_torch": (_I, [_P, _L, _L, _L, _L, _L, _L, _P]),
	"ttk_ar_sample_next": (_I, [_P, C.POINTER(SampleArgs), _P]),
	"ttk_ar_greedy_next": (_I, [_P, C.POINTER(SampleArgs), _P]),
	"ttk_greedy_step": (_I, [C.POINTER(SampleArgs), _P]),
	"ttk_ar_reorder_cache": (_I, [_P, _P, _P]),
	"ttk_beam_step": (_I, [C.POINTER(BeamArgs), _P]),
	"ttk_ar_reorder_cache_lines": (_I, [_P, _P, _I, _P]),
	"ttk_beam_step_lines": (_I, [C.POINTER(BeamArgs), _I, _P]),
	"ttk_sample_step_warped": (_I, [C.POINTER(SampleArgs), _P]),
	"ttk_sample_step_ext": (_I, [C.POINTER(SampleArgs), C.POINTER(SampleExt), _P]),
	"ttk_ar_sample_next_ext": (_I, [_P, C.POINTER(SampleArgs), C.POINTER(SampleExt), _P]),
	"ttk_ar_latents": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, _P]),
	"ttk_ar_score": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
	"ttk_ar_attentions": (_I, [_P, _P, _P, _I, _P, _I, _I, C.POINTER(C.c_int), _I, _P, _P]),
	"ttk_ar_text_attention": (_I, [_P, _P, _P, _I, _P, _I, _I, C.POINTER(C.c_int), _I, _P, _P]),
	"ttk_attn_probs": (_I, [_I, C.POINTER(AttnProbsDesc), _P]),
	"ttk_align_prepare": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
	"ttk_dtw": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
	"ttk_ar_lora_init": (_I, [_P, C.POINTER(WeightView), _I]),
	"ttk_ar_lora_set": (_I, [_P, C.POINTER(WeightView), _I, C.c_float, _P]),
	"ttk_xent_rows": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _I, _P]),
	"ttk_voc_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_voc_destroy": (_I, [_P]),
	"ttk_voc_inference": (_I, [_P, _P, _I, _I, _P, _P]),
	"ttk_univnet_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_univnet_destroy": (_I, [_P]),
	"ttk_univnet_inference": (_I, [_P, _P, _P, _I, _I, _P, _P]),
	"ttk_hifigan_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_hifigan_destroy": (_I, [_P]),
	"ttk_hifigan_set_cond": (_I, [_P, _P, _P]),
	"ttk_hifigan_inference": (_I, [_P, _P, _I, _P, _P]),
	"ttk_dvae_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_dvae_destroy": (_I, [_P]),
	"ttk_dvae_encode": (_I, [_P, _P, _I, _I, _P, _P, _P]),
	"ttk_dvae_quantize": (_I, [_P, _P, _I, _P, _P]),
	"ttk_dvae_decode": (_I, [_P, _P, _I, _I, _P, _P, _P]),
	"ttk_linear_rows": (_I, [_P, _L, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _P, _L, _P]),
	"ttk_rlg_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_rlg_destroy": (_I, [_P]),
	"ttk_rlg_forward": (_I, [_P, _P, _I, _P, _P]),
	"ttk_cls_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_cls_destroy": (_I, [_P]),
	"ttk_cls_forward": (_I, [_P, _P, _I, _I, _P, _P, _P]),
	"ttk_cls_forward_taps": (_I, [_P, _P, _I, _I, _P, _P, C.POINTER(_P), _I, _P]),
	"ttk_cls_conv5_rows": (_I, [_I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
	"ttk_cls_stats_rows": (_I, [_I]),
	"ttk_cls_gn_stats": (_I, [_P, _I, _I, _I, _I, _P, _L, _P, _P]),
	"ttk_clvp_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_clvp_destroy": (_I, [_P]),
	"ttk_clvp_score": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P]),
	"ttk_cond_create": (_I, [C.POINTER(_P), C.POINTER(CondConfigC), C.POINTER(WeightView), _I]),
	"ttk_cond_destroy": (_I, [_P]),
	"ttk_cond_encode": (_I, [_P, _P, _I, _I, _P, _P]),
	"ttk_mel_create": (_I, [C.POINTER(_P), _P, C.POINTER(WeightView), _I]),
	"ttk_mel_destroy": (_I, [_P]),
	"ttk_mel_forward": (_I, [_P, _P, _I, _I, _P, _P]),
	"ttk_resample_fir": (_I, [_P, _I, _I, _P, _I, _I, _I, _P, _I, _P]),
	"ttk_gemm_nt": (_I, [_I, _P, _P, _I, _I, _I, C.c_float, _P, _P, _P]),
	"ttk_gemm": (_I, [_I, C.POINTER(GemmDesc), _P]),
	"ttk_attn_fwd": (_I, [_I, C.POINTER(AttnDesc), _P]),
	"ttk_attn_decode": (_I, [_I, C.POINTER(AttnDecodeDesc), _P]),
	"ttk_gn_apply": (_I, [_I, C.POINTER(GnDesc), _P]),
	"ttk_layernorm_rows": (_I, [_I, C.POINTER(LnDesc), _P]),
	"ttk_lvc_rows": (_I, [_I, C.POINTER(LvcDesc), _P]),
	"ttk_hifi_conv_rows": (_I, [C.POINTER(HifiConvDesc), _P]),
	"ttk_snake_rows": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
	"ttk_block_gn_rows": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
	"ttk_attn_rowwave": (_I, [_I, C.POINTER(AttnDesc), _P]),
	"ttk_cond_im2col_rows": (_I, [_I, _P, _L, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
	"ttk_cond_pool_rows": (_I, [_P, _I, _I, _I, _I, _P, _P]),
	"ttk_clvp_embed_rows": (_I, [_P, _I, _I, _P, _I, _I, _I, _P, _P]),
	"ttk_clvp_rmsnorm_rows": (_I, [_I, _P, _L, _I, _P, _P, _P]),
	"ttk_clvp_rotary_rows": (_I, [_I, _P, _I, _I, _I, _P, _P]),
	"ttk_clvp_geglu_rows": (_I, [_I, _P, _L, _I, _P, _P]),
	"ttk_clvp_mean_rows": (_I, [_I, _P, _I, _I, _I, _P, _P]),
	"ttk_clvp_latent_score": (_I, [_P, _I, _P, _I, _I, _P, _P, _P]),
	"ttk_gemv_mat_create": (_I, [C.POINTER(_P), C.POINTER(GemvMatConfigC), C.POINTER(WeightView), _I]),
	"ttk_gemv_mat_destroy": (_I, [_P]),
	"ttk_gemv_launch": (_I, [_P, C.POINTER(GemvDesc), _P]),
	"ttk_fp8_round_weights": (_I, [_P, _L, C.POINTER(C.c_float), _P]),
	"ttk_sample_step": (_I, [_P, _L, _I, _I, _P, _L, _P, C.c_float, _L, _P, _P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P]),
	"ttk_ar_decode_geometry": (_I, [_I, _I, _I, C.POINTER(C.c_int32)]),
	"ttk_diff_create": (_I, [C.POINTER(_P), C.POINTER(DiffConfigC), C.POINTER(WeightView), _I]),
	"ttk_diff_destroy": (_I, [_P]),
	"ttk_diff_precompute": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
	"ttk_diff_precompute_codes": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
	"ttk_diff_mel_head": (_I, [_P, _P, _I, _I, _P, _P]),
	"ttk_diff_forward": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
	"ttk_diff_begin": (_I, [_P, _P, _I, _I, _P]),
	"ttk_diff_step": (_I, [_P, _P, C.POINTER(StepC), _P, _P]),
	"ttk_diff_sample_ddim": (_I, [_P, _P, _P, _I, _I, C.POINTER(StepC), _I, _P]),
	"ttk_diff_sample_p": (_I, [_P, _P, _P, _I, _I, C.POINTER(StepC), _I, _P, _P]),
	"ttk_diff_sample_ddim_lines": (_I, [_P, _P, _P, _I, _I, C.POINTER(C.c_int), C.POINTER(StepC), _I, _P]),
	"ttk_diff_sample_ext": (_I, [_P, _P, _P, _I, _I, C.POINTER(StepC), C.POINTER(StepExtC), _I, _P, _P]),
	"ttk_diff_step_ext": (_I, [_P, _P, C.POINTER(StepC), C.POINTER(StepExtC), _P, _P, _P]),
	"ttk_diffusion_step_ext_rows": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(StepC), C.POINTER(StepExtC), _P, _I, _I, _I, _P]),
	"ttk_diff_sample_ms": (_I, [_P, _P, _P, _I, _I, C.POINTER(StepC), C.POINTER(StepMsC), _I, _P]),
	"ttk_diff_sample_ms_lines": (_I, [_P, _P, _P, _I, _I, C.POINTER(C.c_int), C.POINTER(StepC), C.POINTER(StepMsC), _I, _P]),
	"ttk_diff_step_ms": (_I, [_P, _P, _P, C.POINTER(StepC), C.POINTER(StepMsC), _P, _P]),
	"ttk_diffusion_step_ms_rows": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(StepC), C.POINTER(StepMsC), _P, _I, _I, _I, _P]),
}

_lib = None


def build(force: bool = False) -> str:
	"""Compile libttk.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
	if force:
		subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "clean"], check=True, capture_output=True)
	r = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j8"], capture_output=True, text=True)
	if r.returncode != 0:
		raise TTKError("building libttk.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
	return LIB_PATH


def load():
	global _lib
	if _lib is not None:
		return _lib
	if not os.path.exists(LIB_PATH):
		raise TTKError(f"{LIB_PATH} is missing: build it with `make -C tortoise_tts_amd/csrc` "
					   "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
	lib = C.CDLL(LIB_PATH)
	for name, (res, args) in SYMBOLS.items():
		fn = getattr(lib, name)   # AttributeError if the ABI lost a symbol
		fn.restype, fn.argtypes = res, args
	if lib.ttk_version() != 1:
		raise TTKError(f"libttk ABI version {lib.ttk_version()} != 1")
	_lib = lib
	return lib


def check(rc: int, what: str):
	if rc != 0:
		raise TTKError(f"{what} failed ({rc}): {load().ttk_last_error().decode()}")


def stream_ptr() -> int:
	return torch.cuda.current_stream().cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
	return None if t is None else t.data_ptr()


def require_cuda(*tensors: torch.Tensor):
	for t in tensors:
		if t is not None and not t.is_cuda:
			raise TTKError("libttk takes device tensors; got a CPU tensor (the HIP path has no CPU fallback)")


def cuda_device(device) -> torch.device:
	dev = torch.device(device)
	if dev.type != "cuda":
		raise TTKError("tortoise_tts_amd runs on an MI355X only (device must be cuda:N)")
	return dev


class Handle:
	"""What every wrapper of a libttk handle shares: the device it lives on, the library, the handle `ttk_<abi>_create` makes from a config struct
	and named f32 tensors, and its lifetime.  The subclass prepares its weights, says which tensors are missing in its own words and calls `_create`."""

	def __init__(self, device):
		self.device = cuda_device(device)
		self.lib = load()

	def _create(self, abi: str, config: C.Structure, tensors: Dict[str, torch.Tensor], names: Sequence[str]):
		views, keep = weight_views(tensors, names)      # `keep` lives until the create call has copied the tensors
		self._abi, self._h = abi, C.c_void_p()
		create = f"ttk_{abi}_create"
		with torch.cuda.device(self.device):
			check(getattr(self.lib, create)(C.byref(self._h), C.byref(config), views, len(names)), create)

	def __del__(self):
		h = getattr(self, "_h", None)          # absent when __init__ raised before `_create`, empty when the create call failed
		if h:
			getattr(self.lib, f"ttk_{self._abi}_destroy")(h)
			self._h = None

	def eval(self, *a, **k):
		return self

	def to(self, *a, **k):
		return self


def weight_views(sd: Dict[str, torch.Tensor], names: Sequence[str]):
	"""(array of ttk_weight_view, keepalive list) for f32 contiguous tensors (host or device)."""
	keep: List[torch.Tensor] = []
	arr = (WeightView * len(names))()
	for i, n in enumerate(names):
		t = sd[n].detach().to(torch.float32).contiguous()
		keep.append(t)
		arr[i].name = n.encode()
		arr[i].data = t.data_ptr()
		arr[i].ndim = min(t.dim(), 4)
		for j in range(4):
			arr[i].shape[j] = t.shape[j] if j < t.dim() else 1
	return arr, keep
