"""`autoregressive.score_inputs` -- the index work `UnifiedVoice.forward` does on its integer inputs (types, clipping, set_mel_padding, targets) -- against the
shapes and targets the reference's own forward produced (tests/golden/ar_score_small.npz, tools/make_golden_ar_score.py), and `weights.ar_score_shapes`."""
import numpy as np
import pytest
import torch

from tortoise_tts_amd import weights as W
from tortoise_tts_amd.autoregressive import score_inputs

CFG = W.AR_SMALL


def t(a):
	return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("case", ["a", "b", "c63"])
def test_score_inputs_match_the_reference_targets(golden, case):
	g = golden("ar_score_small")
	text_in, codes_in = t(g[f"{case}_text"]), t(g[f"{case}_codes"])
	keep = (text_in.clone(), codes_in.clone())
	text, codes, tt, mt = score_inputs(CFG, text_in, t(g[f"{case}_text_lengths"]), codes_in, t(g[f"{case}_wav_lengths"]), None, bool(g[f"{case}_clip"]))
	want_tt, want_mt = t(g[f"{case}_text_targets"]), t(g[f"{case}_mel_targets"])
	assert tt.dtype == mt.dtype == text.dtype == codes.dtype == torch.int64
	assert tt.shape == want_tt.shape and torch.equal(tt, want_tt)
	assert mt.shape == want_mt.shape and torch.equal(mt, want_mt)
	assert torch.equal(text, want_tt[:, :-2]) and torch.equal(codes, want_mt[:, :-2])
	assert (tt[:, -2:] == CFG.stop_text_token).all() and (mt[:, -2:] == CFG.stop_mel_token).all()
	assert torch.equal(text_in, keep[0]) and torch.equal(codes_in, keep[1])      # the caller's tensors are left alone (the reference pads in place)


def test_case_b_clips_and_pads(golden):
	g = golden("ar_score_small")
	text, codes, _, mt = score_inputs(CFG, t(g["b_text"]), t(g["b_text_lengths"]), t(g["b_codes"]), t(g["b_wav_lengths"]))
	assert text.shape == (3, 7) and codes.shape == (3, 12)
	assert (codes[2, 4:] == CFG.stop_mel_token).all() and (codes[2, :4] == t(g["b_codes"])[2, :4]).all()
	assert (codes[:2] == t(g["b_codes"])[:2, :12]).all()          # 12 + 1 and 11 + 1 frames: nothing to pad inside 12 columns
	assert int((mt == CFG.stop_mel_token).sum()) == 8 + 3 * 2
	# clip_inputs=False keeps the widths and still pads
	text2, codes2, tt2, mt2 = score_inputs(CFG, t(g["b_text"]), t(g["b_text_lengths"]), t(g["b_codes"]), t(g["b_wav_lengths"]), None, False)
	assert text2.shape == (3, 9) and codes2.shape == (3, 17) and tt2.shape == (3, 11) and mt2.shape == (3, 19)
	assert (codes2[0, 13:] == CFG.stop_mel_token).all() and (codes2[1, 12:] == CFG.stop_mel_token).all() and (codes2[2, 4:] == CFG.stop_mel_token).all()
	# one wav length for the whole batch
	_, codes3, _, _ = score_inputs(CFG, t(g["b_text"]), t(g["b_text_lengths"]), t(g["b_codes"]), torch.tensor([5 * 1024]), None, False)
	assert (codes3[:, 6:] == CFG.stop_mel_token).all() and torch.equal(codes3[:, :6], t(g["b_codes"])[:, :6])


def test_types_multiply_the_text_ids():
	text = torch.tensor([[1, 2, 3], [4, 5, 6]])
	codes = torch.zeros((2, 4), dtype=torch.int64)
	out, _, tt, _ = score_inputs(CFG, text, torch.tensor([3, 3]), codes, torch.tensor([4096, 4096]), torch.tensor([0, 2]))
	assert out.tolist() == [[1, 2, 3], [12, 15, 18]]
	assert tt.tolist() == [[1, 2, 3, 0, 0], [12, 15, 18, 0, 0]]
	with pytest.raises(IndexError, match="text token"):          # 100 * 3 leaves the 256-row table
		score_inputs(CFG, torch.tensor([[100]]), torch.tensor([1]), codes[:1], torch.tensor([4096]), torch.tensor([2]))


def test_errors():
	text, codes = torch.ones((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)
	with pytest.raises(ValueError, match="clip the mel codes to 0"):
		score_inputs(CFG, text, torch.tensor([3, 3]), codes, torch.tensor([1023, 500]))
	with pytest.raises(IndexError, match="mel code"):
		score_inputs(CFG, text, torch.tensor([3, 3]), torch.full((2, 4), CFG.number_mel_codes), torch.tensor([4096, 4096]))
	with pytest.raises(IndexError, match="text token"):
		score_inputs(CFG, torch.full((2, 3), 256), torch.tensor([3, 3]), codes, torch.tensor([4096, 4096]))
	with pytest.raises(IndexError, match="text token"):
		score_inputs(CFG, -text, torch.tensor([3, 3]), codes, torch.tensor([4096, 4096]))
	# an id that the clip removes is not looked at, as in the reference
	bad = codes.clone()
	bad[:, 3] = 99999
	_, c, _, _ = score_inputs(CFG, text, torch.tensor([3, 3]), bad, torch.tensor([3 * 1024, 2 * 1024]))
	assert c.shape == (2, 3)
	with pytest.raises(ValueError, match="1 or B"):
		score_inputs(CFG, text, torch.tensor([3, 3]), codes, torch.tensor([4096, 4096, 4096]))


@pytest.mark.parametrize("cfg", [W.AR_SMALL, W.AR_FULL], ids=["small", "full"])
def test_ar_score_shapes_adds_the_text_head_only(cfg):
	base, score = W.ar_shapes(cfg), W.ar_score_shapes(cfg)
	assert set(score) - set(base) == {"text_head.weight", "text_head.bias"} and all(score[k] == v for k, v in base.items())
	assert score["text_head.weight"] == (cfg.number_text_tokens + 1, cfg.model_dim) and score["text_head.bias"] == (cfg.number_text_tokens + 1,)
	if cfg is W.AR_SMALL:
		a, b = W.synth_state_dict(base, 31), W.synth_state_dict(score, 31)
		assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
		assert float(b["text_head.weight"].std()) > 0
