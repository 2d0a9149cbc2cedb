"""Self-tests of tests/guarded.py against a fake "kernel" written in torch on CPU buffers: y[b][r][c] = 2 x[b][r][c] addressed
through (pointer offset, ld, stride) like a device kernel, with one fault planted at a time.  Each of the four planted faults the
helper exists for must be detected, for fp32, bf16 and int64 results; the clean kernel must pass."""
import pytest
import torch

from guarded import (BAD_ID, GUARD_BYTES, Guarded, assert_finite_where, assert_pair_within_atomic_bound, assert_same_bits,
                     assert_within_atomic_bound, report_mismatch)

DTYPES = [torch.float32, torch.bfloat16, torch.int64]


def fake_kernel(x, y, fault=None):
    """Flat-buffer row scaling.  x, y: Guarded on the CPU."""
    X, Y = x.buf, y.buf
    for b in range(x.batch):
        for r in range(x.rows):
            xo, yo = x.guard + b * x.stride + r * x.ld, y.guard + b * y.stride + r * y.ld
            v = X[xo:xo + x.cols] * 2
            if fault == 'consume_nan' and r == x.rows - 1:
                v = v + X[xo + x.cols] * 0  # "multiplied by zero": still NaN
            Y[yo:yo + y.cols] = v.to(Y.dtype)
            if fault == 'past_row' and r == 1:
                Y[yo + y.cols] = 1
    last = y.guard + (y.batch - 1) * y.stride + (y.rows - 1) * y.ld
    if fault == 'past_end':
        Y[last + y.ld:last + y.ld + y.cols] = 1
    if fault == 'in_front':
        Y[y.guard - 1] = 1
    if fault == 'write_input':
        X[x.guard + x.cols] = 3
    if fault == 'skip_store':
        Y[y.guard + y.ld + 2] = Y[0]  # one element of the window keeps what the buffer was filled with


def operands(dtype, padded, batch=2, rows=5, cols=8):
    g = torch.Generator().manual_seed(3)
    data = torch.randint(-4, 5, (batch, rows, cols), generator=g).to(dtype)
    ld = -(-(cols + 3) // 8) * 8 if padded else None  # the next multiple of 8 above the natural one
    x = Guarded(data, ld=ld, stride=(rows * ld + 16 if padded else None), device='cpu')
    y = Guarded(role='out', shape=(batch, rows, cols), dtype=dtype, ld=(ld + 8 if padded else None),
                stride=(rows * (ld + 8) + 24 if padded else None), device='cpu')
    return data, x, y


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_clean_kernel_passes_and_matches_dense(dtype):
    res = []
    for padded in (True, False):
        data, x, y = operands(dtype, padded)
        fake_kernel(x, y)
        x.check('x')
        res.append(y.check('y'))
        assert torch.equal(res[-1], data * 2)
    assert_same_bits(res[0], res[1], 'fake')
    assert_finite_where(res[0], res[1], 'fake')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('fault,words', [('past_row', 'row gap'), ('past_end', 'BEHIND'), ('in_front', 'FRONT')])
def test_planted_stray_store_is_detected(dtype, fault, words):
    """One element past a row, one row past the end, one element in front of the buffer."""
    _, x, y = operands(dtype, True)
    fake_kernel(x, y, fault)
    with pytest.raises(AssertionError, match='stray store') as e:
        y.check('y')
    assert words in str(e.value)


def test_stray_store_past_end_is_detected_on_a_dense_output():
    """With natural strides the row gap does not exist, but front and back guards do."""
    for fault in ('past_end', 'in_front'):
        _, x, y = operands(torch.float32, False)
        fake_kernel(x, y, fault)
        with pytest.raises(AssertionError, match='stray store'):
            y.check('y')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
def test_consumed_nan_is_detected(dtype):
    """The faulty kernel adds 0 * (the element behind the last row's end): the back guard's NaN, dense or padded."""
    _, xd, yd = operands(dtype, False, batch=1)
    fake_kernel(xd, yd)  # a clean dense result to compare with
    _, xp, yp = operands(dtype, True, batch=1)
    fake_kernel(xp, yp, 'consume_nan')
    with pytest.raises(AssertionError, match='non-finite in the padded call only'):
        assert_finite_where(yp.check('y'), yd.check('y'), 'fake')
    with pytest.raises(AssertionError, match='differ'):
        assert_same_bits(yp.check('y'), yd.check('y'), 'fake')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_element_never_stored_is_detected(dtype):
    """The sentinel is finite and the same in a padded and a dense call: an element the kernel forgot must not pass as a value."""
    _, x, y = operands(dtype, True)
    fake_kernel(x, y, 'skip_store')
    with pytest.raises(AssertionError, match='never stored'):
        y.check('y')
    part = Guarded(role='out', shape=(3, 8), dtype=dtype, device='cpu', partial=True)  # a workspace may stay partly unwritten
    part.check('workspace')


def test_pair_bound_for_atomics():
    mag = torch.full((4,), 1000.0, dtype=torch.float64)
    a = torch.full((4,), 100.0)
    assert_pair_within_atomic_bound(a, a + 2 * 10 * 2.0**-23 * 999, mag, 10, 'x')
    with pytest.raises(AssertionError, match='bound'):
        assert_pair_within_atomic_bound(a, a + 1e-2, mag, 10, 'x')
    with pytest.raises(AssertionError, match='non-finite'):
        assert_pair_within_atomic_bound(a * float('nan'), a, mag, 10, 'x')


def test_modified_input_is_detected():
    _, x, y = operands(torch.float32, True)
    fake_kernel(x, y, 'write_input')
    with pytest.raises(AssertionError, match='input buffer was modified'):
        x.check('x')


def test_layout_of_the_buffer():
    """Guards of at least 64 KiB on both sides, poison in every gap of an input, sentinel everywhere in an output, and the window
    ends where the back guard begins."""
    data = torch.arange(2 * 3 * 8, dtype=torch.float32).view(2, 3, 8)
    x = Guarded(data, ld=12, stride=40, device='cpu')
    assert x.guard * 4 >= GUARD_BYTES and x.buf.numel() == 2 * x.guard + 40 + 2 * 12 + 8
    assert bool(torch.isnan(x.buf[~x.inside]).all()) and int(x.inside.sum()) == data.numel()
    assert bool(x.inside[x.guard + x.span - 1]) and not bool(x.inside[x.guard + x.span])
    assert torch.equal(x.window(), data)
    ids = Guarded(torch.arange(6).view(1, 6), device='cpu')
    assert bool((ids.buf[~ids.inside] == BAD_ID).all())
    for dt in (torch.float32, torch.bfloat16, torch.int64, torch.float16):
        y = Guarded(role='out', shape=(3, 8), dtype=dt, ld=16, device='cpu')
        assert y.guard * y.buf.element_size() >= GUARD_BYTES
        assert len(set(y.buf.view(-1).tolist())) == 1 and bool(torch.isfinite(y.buf.float()).all())
    acc = Guarded(base=torch.ones(3, 8), ld=16, device='cpu')
    assert acc.role == 'out' and torch.equal(acc.window(), torch.ones(3, 8)) and float(acc.buf[acc.guard + 8]) != 1.0


def test_report_mismatch_lists_triples_and_atomic_bound():
    a = torch.zeros(4, 4)
    b = a.clone()
    b[2, 3] = 1
    with pytest.raises(AssertionError, match=r'1 of 16 elements differ.*\(2, 3\)'):
        report_mismatch(a, b, 'x')
    report_mismatch(torch.tensor([0.0]), torch.tensor([-0.0]), 'signed zero')
    ref = torch.full((4,), 100.0, dtype=torch.float64)
    mag = torch.full((4,), 1000.0, dtype=torch.float64)
    ok = (ref + 10 * 2.0**-23 * 999).float()
    assert_within_atomic_bound(ok, ok, ref, mag, 10, 'x')
    with pytest.raises(AssertionError, match='bound'):
        assert_within_atomic_bound((ref + 1).float(), ok, ref, mag, 10, 'x')
