"""Guarded buffers for tests of the C-ABI (include/mmvid_hip.h): every operand and every result of a call lives inside a larger flat
buffer, so that a store or a load outside the window the arguments declare becomes visible.

    [ front guard | batch 0: rows x ld ......... | gap | batch 1 ... | last row: only `cols` elements | back guard ]

The window is `[batch][rows][cols]` with `ld` elements between rows and `stride` elements between batch entries; it ENDS with the
last element of its last row, where the back guard begins.  Guards are GUARD_BYTES (64 KiB) each: more than one tile of any kernel.

* an OUTPUT is pre-filled with a sentinel bit pattern (also inside the window, unless `base` gives the values the call adds to);
  `check()` reads the whole buffer back and demands that every element outside the window still holds the sentinel's bits;
* an INPUT holds quiet NaN (fp32, bf16, fp16) or an out-of-range id (integers) everywhere outside the window; `check()` demands
  that the call left the whole buffer as it was.  A kernel that consumes what lies outside its operand turns its result into
  NaN (or reads an id no table has): `assert_same_bits` / `assert_finite_where` then fail.

Everything here is ordinary data: no fault is provoked.  The module is a plain helper (no fixtures, no pytest settings); its own
tests are tests/test_guarded_host.py and run without a GPU."""
import ctypes

import torch

GUARD_BYTES = 64 * 1024
BAD_ID = 0x3FFFFFF1  # an id no table of the tests has
# sentinel bit patterns, as the signed integer of the element's width; none is a value a test produces
SENTINEL_BITS = {torch.float32: -0x39BF1949,            # 0xC640E6B7 = -12345.678f
                 torch.bfloat16: -0x395B,               # 0xC6A5     = -21120 (bf16)
                 torch.float16: -0x0A5B,                # 0xF5A5     = -23120 (fp16)
                 torch.int64: -0x5A5A5A5A5A5A5A5B,
                 torch.int32: -0x5A5A5A5B,
                 torch.uint8: 0xA5}
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.int64: torch.int64,
             torch.int32: torch.int32, torch.uint8: torch.uint8}


def bits(t):
    """The tensor's elements as integers of the same width (NaN payloads and signed zeros compare as what they are)."""
    return t.contiguous().view(_INT_VIEW[t.dtype])


def _fill_value(dtype, role):
    """A 1-element tensor of `dtype` holding the fill of a guard."""
    if role == 'out':
        return torch.tensor([SENTINEL_BITS[dtype]], dtype=_INT_VIEW[dtype]).view(dtype)
    if dtype.is_floating_point:
        return torch.tensor([float('nan')], dtype=dtype)
    return torch.tensor([0xFF if dtype == torch.uint8 else BAD_ID], dtype=dtype)


class Guarded:
    """One operand of a call.  `data`: CPU tensor [rows, cols] or [batch, rows, cols] (or 1-D: one row) -- the window's contents; for
    an output give `shape` and `dtype` instead (or `base` = the values the call accumulates into).  `ld` / `stride` in elements
    (default: dense).  `.ptr` is the ctypes pointer of the window's first element, `.ld` and `.stride` what to pass with it."""

    def __init__(self, data=None, *, role='in', shape=None, dtype=None, ld=None, stride=None, base=None, device='cuda',
                 guard_bytes=GUARD_BYTES, partial=False):
        assert role in ('in', 'out')
        # an output without base values must be written EVERYWHERE inside its window (check() finds elements that still hold the
        # sentinel), unless `partial` says that the call fills only part of it (a workspace, a cache, a skipped slot)
        self.must_fill = role == 'out' and base is None and data is None and not partial
        if base is not None:
            data, role = base, 'out'
        if data is not None:
            shape, dtype = tuple(data.shape), data.dtype
        self.user_shape = tuple(shape)
        shape3 = (1,) * (3 - len(shape)) + tuple(shape)
        assert len(shape3) == 3
        self.batch, self.rows, self.cols = shape3
        self.role, self.dtype = role, dtype
        self.ld = self.cols if ld is None else int(ld)
        self.stride = self.rows * self.ld if stride is None else int(stride)
        assert self.ld >= self.cols and (self.batch == 1 or self.stride >= (self.rows - 1) * self.ld + self.cols)
        esz = torch.empty(0, dtype=dtype).element_size()
        self.guard = -(-guard_bytes // esz)
        assert self.guard * esz >= GUARD_BYTES or guard_bytes < GUARD_BYTES
        self.span = (self.batch - 1) * self.stride + (self.rows - 1) * self.ld + self.cols
        fill = _fill_value(dtype, role)
        self.fill_bits = bits(fill)[0].clone()
        host = fill.repeat(self.guard + self.span + self.guard)
        self.inside = torch.zeros(host.numel(), dtype=torch.bool)
        self._window(self.inside).fill_(True)
        if data is not None:
            self._window(host).copy_(data.reshape(shape3))
        self.host = host
        self.buf = host.to(device, copy=True)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.guard * esz)

    def _window(self, flat):
        return flat.as_strided((self.batch, self.rows, self.cols), (self.stride, self.ld, 1), self.guard)

    def window(self):
        """The window's current contents on the CPU, in the shape the operand was given in."""
        return self._window(self.buf.cpu()).clone().reshape(self.user_shape)

    def check(self, what=''):
        """Outside the window nothing may have changed (an output: still the sentinel; an input: still the poison), and an input's
        window is unchanged too; a plain output's window holds no sentinel any more (every element was stored).  Returns the window."""
        now = self.buf.cpu()
        nb, hb = bits(now), bits(self.host)
        touched = nb != hb
        if self.role == 'out':
            touched &= ~self.inside
            assert bool((hb[~self.inside] == self.fill_bits).all())
        if bool(touched.any()):
            idx = touched.nonzero().view(-1)
            where = [self.describe(int(i)) for i in idx[:4]]
            kind = 'stray store outside the declared window of an output' if self.role == 'out' else 'an input buffer was modified'
            raise AssertionError(f'{what}: {kind}: {idx.numel()} elements, first at {"; ".join(where)}')
        if self.must_fill:
            unwritten = (nb == self.fill_bits) & self.inside
            if bool(unwritten.any()):
                idx = unwritten.nonzero().view(-1)
                raise AssertionError(f'{what}: {idx.numel()} elements INSIDE the window of an output were never stored (they still hold the '
                                     f'sentinel), first at {"; ".join(self.describe(int(i)) for i in idx[:4])}')
        return self._window(now).clone().reshape(self.user_shape)

    def describe(self, flat_index):
        """Where a flat element of the buffer lies, in words."""
        i = flat_index - self.guard
        if i < 0:
            return f'{-i} elements in FRONT of the window'
        if i >= self.span:
            return f'{i - self.span + 1} elements BEHIND the window (row {(i - (self.batch - 1) * self.stride) // self.ld} of {self.rows} in the last batch entry)'
        b, r = divmod(i, self.stride) if self.batch > 1 else (0, i)
        if r >= self.rows * self.ld:
            return f'the gap behind batch entry {b}'
        return f'batch {b} row {r // self.ld} column {r % self.ld} (row gap: cols = {self.cols}, ld = {self.ld})'


def report_mismatch(got, want, what, limit=5):
    """torch.equal on values whose bits must agree; on failure the count and the first few (index, got, want)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if got.dtype.is_floating_point:  # +0 and -0 are the same number
        bad &= ~((got == 0) & (want == 0))
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    triples = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:limit]]
    raise AssertionError(f'{what}: {idx.shape[0]} of {bad.numel()} elements differ; first (index, got, want): {triples}')


def assert_same_bits(padded, dense, what):
    """The padded call's window against the dense call's: bit for bit."""
    report_mismatch(padded, dense, what + ': padded-and-poisoned call differs from the dense call')


def assert_finite_where(padded, dense, what):
    bad = ~torch.isfinite(padded.float()) & torch.isfinite(dense.float())
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements are non-finite in the padded call only (a poisoned element was consumed); first {bad.nonzero()[:3].tolist()}'


def assert_within_atomic_bound(padded, dense, ref64, mag64, K, what):
    """For results accumulated with fp32 atomics (free order): both calls within K * 2^-23 * sum|terms| of the fp64 value, and the
    padded one finite wherever the dense one is."""
    assert_finite_where(padded, dense, what)
    bound = K * 2.0**-23 * mag64 + 1e-30
    for name, t in (('padded', padded), ('dense', dense)):
        r = ((t.double() - ref64).abs() / bound).max().item()
        print(f'{what}: {name} worst |err| / (K 2^-23 sum|terms|) = {r:.3f} (K = {K})')
        assert r <= 1.0, f'{what}: {name} call is {r:.2f} x the K 2^-23 sum|terms| bound away from fp64'


def assert_pair_within_atomic_bound(padded, dense, mag64, K, what):
    """The padded and the dense call add the SAME fp32 terms, in an order the atomics leave free: each is within K 2^-23 sum |terms|
    of the exact sum of those terms, so |padded - dense| <= 2 K 2^-23 sum |terms| -- with no reference value in between, hence no
    allowance for how a reference was rebuilt.  mag64: sum |terms| (an fp64 evaluation)."""
    assert_finite_where(padded, dense, what)
    bound = 2 * K * 2.0**-23 * mag64 + 1e-30
    r = ((padded.double() - dense.double()).abs() / bound).max().item()
    print(f'{what}: worst |padded - dense| / (2 K 2^-23 sum|terms|) = {r:.3f} (K = {K})')
    assert r <= 1.0, f'{what}: the padded and the dense call differ by {r:.2f} x the 2 K 2^-23 sum|terms| bound'


# ---- what the test modules share ------------------------------------------------------------------------------------------------
def seeded(*key):
    """A CPU generator seeded from the case's parameters."""
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * sum(map(ord, str(k))) for i, k in enumerate(key)) % (2**31)))


def call_abi(name, *args):
    """mmvid_amd._lib.call on the current stream, synchronised."""
    from mmvid_amd import _lib, ops
    _lib.call(name, *args, ops._stream())
    torch.cuda.synchronize()


def ptr_of(g):
    """The window pointer of a Guarded operand, NULL for None (an optional argument left out)."""
    return None if g is None else g.ptr
