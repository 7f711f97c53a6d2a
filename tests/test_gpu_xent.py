"""`ttk_xent_rows` (csrc/xent.hip) on its own against float64: the row cross-entropy, its deterministic mean and the transposed [rows / T][C][T] copy.

Bound per row: |nll - nll64| <= 1e-5 + 8 * 2^-24 * max(1, max|x_row|) -- f32 rounding of the max-plus-log form (the sum of exponentials is at most C = 8194
terms in [0, 1], its log is taken once; what remains is the rounding of max + log(sum) - x[target] at the magnitude of the logits).  torch's own f32
cross-entropy on the CPU sits at 0.21 of it on these inputs."""
import numpy as np
import pytest
import torch

from tortoise_tts_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = (1, 63, 64, 65, 256, 8194)
SCALES = (1.0, 8.0, 100.0, 1e4)


def bound(x64):
	"""x64 [rows, C] -> [rows]"""
	return 1e-5 + 8 * 2.0 ** -24 * x64.abs().amax(dim=1).clamp(min=1.0)


def make_rows(rows, C, scale, seed, ld):
	"""seeded normal logits inside a [rows, ld] buffer whose padding columns are NaN; row 0's target is the last class, 3 scales below the row's maximum"""
	g = torch.Generator().manual_seed(seed)
	x = torch.randn((rows, C), generator=g) * scale
	target = torch.randint(0, C, (rows,), generator=g)
	target[0] = C - 1
	if C > 1:
		x[0, C - 1] = x[0, :C - 1].max() - 3 * scale
	buf = torch.full((rows, ld), float("nan"))
	buf[:, :C] = x
	return x, target, buf


def run(lib, buf, rows, C, target, mean=False, T=0):
	d = buf.to(DEV)
	tg = target.to(DEV)
	nll = torch.full((rows,), float("nan"), device=DEV)
	m = torch.full((1,), float("nan"), device=DEV) if mean else None
	out_t = torch.full((rows // T, C, T), float("nan"), device=DEV) if T else None
	_lib.check(lib.ttk_xent_rows(d.data_ptr(), d.stride(0), rows, C, tg.data_ptr(), nll.data_ptr(), _lib.ptr(m), _lib.ptr(out_t), T, _lib.stream_ptr()), "ttk_xent_rows")
	torch.cuda.synchronize()
	return nll.cpu(), (m.cpu() if mean else None), (out_t.cpu() if T else None)


def nll64(x, target):
	x64 = x.double()
	return torch.logsumexp(x64, dim=1) - x64.gather(1, target[:, None])[:, 0]


def host_mean(nll):
	"""the order include/ttk.h documents, in f32"""
	a = nll.numpy().astype(np.float32)
	part = np.zeros(256, dtype=np.float32)
	for i in range(a.shape[0]):
		part[i % 256] = np.float32(part[i % 256] + a[i])
	o = 128
	while o > 0:
		part[:o] = part[:o] + part[o:2 * o]
		o //= 2
	return np.float32(part[0] / np.float32(a.shape[0]))


@pytest.fixture(scope="module")
def lib():
	return _lib.load()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("C", CLASSES)
def test_rows_against_float64(lib, C, scale):
	for rows in (1, 57):
		# ld = C + 3: rows start at every 4-byte phase of a 16-byte chunk; ld a multiple of 4 behind C: every row starts on 16 bytes
		for ld in (C + 3, (C + 3) // 4 * 4 + 4):
			x, target, buf = make_rows(rows, C, scale, 1000 * C + rows, ld)
			got, mean, _ = run(lib, buf, rows, C, target, mean=True)
			want = nll64(x, target)
			err, b = (got.double() - want).abs(), bound(x.double())
			print(f"C={C} rows={rows} ld={ld} scale={scale:g}: worst |nll - nll64| / bound = {(err / b).max().item():.3f}  (max err {err.max().item():.3e})")
			assert torch.isfinite(got).all(), "a padding column (NaN) was read, or the exponential overflowed"
			assert (err <= b).all(), (C, rows, ld, scale, (err / b).max().item())
			assert np.float32(mean.item()) == host_mean(got) and np.float32(mean.item()).tobytes() == host_mean(got).tobytes()
			again, mean2, _ = run(lib, buf, rows, C, target, mean=True)
			assert torch.equal(again.view(torch.int32), got.view(torch.int32)) and torch.equal(mean2.view(torch.int32), mean.view(torch.int32))


def test_extreme_logits_neither_overflow_nor_nan(lib):
	C = 8194
	x = torch.full((3, C), -1e4)
	x[0, 5] = 1e4; x[1, :] = 1e4; x[2, C - 1] = 1e4
	target = torch.tensor([5, 7, 0])
	got, _, _ = run(lib, x, 3, C, target)
	want = nll64(x, target)
	assert torch.isfinite(got).all() and ((got.double() - want).abs() <= bound(x.double())).all(), (got, want)


@pytest.mark.parametrize("T", (11, 64, 65))
@pytest.mark.parametrize("C", (1, 65, 8194))
def test_transposed_copy_is_bit_exact(lib, C, T):
	rows = 2 * T
	x, target, buf = make_rows(rows, C, 8.0, 7 * C + T, C + 3)
	got, mean, out_t = run(lib, buf, rows, C, target, mean=True, T=T)
	want = x.view(2, T, C).permute(0, 2, 1).contiguous()
	assert out_t.shape == want.shape and torch.equal(out_t.view(torch.int32), want.view(torch.int32))
	assert ((got.double() - nll64(x, target)).abs() <= bound(x.double())).all()
	assert np.float32(mean.item()).tobytes() == host_mean(got).tobytes()


def test_mean_over_more_rows_than_threads(lib):
	rows, C = 600, 64
	x, target, buf = make_rows(rows, C, 8.0, 99, C + 4)
	got, mean, _ = run(lib, buf, rows, C, target, mean=True)
	assert np.float32(mean.item()).tobytes() == host_mean(got).tobytes()
	assert abs(float(mean) - float(nll64(x, target).mean())) <= float(bound(x.double()).max())
	_, mean2, _ = run(lib, buf, rows, C, target, mean=True)
	assert torch.equal(mean.view(torch.int32), mean2.view(torch.int32))


def test_arguments_are_checked(lib):
	x = torch.zeros((4, 8), device=DEV)
	tg = torch.zeros(4, dtype=torch.int64, device=DEV)
	nll = torch.empty(4, device=DEV)
	out = torch.empty(4 * 8, device=DEV)
	assert lib.ttk_xent_rows(x.data_ptr(), 4, 4, 8, tg.data_ptr(), nll.data_ptr(), None, None, 0, _lib.stream_ptr()) != 0          # ld < C
	assert lib.ttk_xent_rows(x.data_ptr(), 8, 4, 8, tg.data_ptr(), nll.data_ptr(), None, out.data_ptr(), 3, _lib.stream_ptr()) != 0  # rows % T
	assert lib.ttk_xent_rows(None, 8, 4, 8, tg.data_ptr(), nll.data_ptr(), None, None, 0, _lib.stream_ptr()) != 0
	# a target outside the row is not read: NaN for that row, the others are unaffected
	tg[2] = 8
	_lib.check(lib.ttk_xent_rows(x.data_ptr(), 8, 4, 8, tg.data_ptr(), nll.data_ptr(), None, None, 0, _lib.stream_ptr()), "ttk_xent_rows")
	r = nll.cpu()
	assert torch.isnan(r[2]) and torch.allclose(r[[0, 1, 3]], torch.full((3,), float(np.log(8.0))), atol=1e-6)
