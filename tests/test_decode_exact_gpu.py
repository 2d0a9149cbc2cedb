"""The production decode step, bit for bit at every kernel boundary (construction and reference: tests/decode_exact.py; its own
conditions: tests/test_decode_exact_host.py).

mmvid_tower_decode_fused_slice (3..64 sequences: gemv16_mfma_kernel + attn_decode2_kernel<4,2> / <8,3> / <8,2>; 1-2 sequences with
fused='launches': gemv_rows_kernel) and mmvid_tower_decode_persistent (1-2 sequences) run ONE step on a crafted tower and a cache the
test wrote itself; the hidden state and the WHOLE cache after the step are compared with the exact reference by bit equality:

  * 'census' (q = 0, one-hot values): every cached key counted exactly once, the denominator exactly n;
  * 'spot'   (one key per (sequence, head) carries all the weight): score k is paired with value row k -- at key 0, the last cached key,
    the new row and both sides of every batch / wave / range / pass edge of the kernels;
  * cache rows from `pos` on are NaN before the step (a read at or beyond the position poisons the output), row `pos` must come back as
    (k_new | v_new), every other element bit-unchanged, NaN guard rows behind the last sequence included;
  * cache lengths n = pos + 1 sit on both sides of every path switch: 4 -> 8 waves at 512 keys, the register batches' end (1,536 keys
    for <8,3>, 1,024 for <8,2>: the loop beyond them), Lmax = 4,096; the persistent step's empty ranges (n < 4), its second 256-key
    pass (n > 1,024), eager and captured-and-replayed (the device-side position drives every bound);
  * the linear layers in every form the step launches: 16 x 16 tiles with 1 / 2 / 4 row blocks, the 8 x 8 tile with 8 / 16 input rows,
    bf16 rows read as fragments, K|V append, position advance, slices of a shared cache (batch 70 = 64 + 6), two layers.
No tolerance anywhere."""
import functools

import pytest
import torch

import decode_exact as dx

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16


@functools.lru_cache(maxsize=4)
def _tower(E, layers, mode, rich):
    return dx.build_tower(E, layers, mode, rich, DEV), dx.params_to(dx.tower_params(E, layers, mode, rich), DEV)


def _same(got, want, what):
    got, want = got.contiguous(), want.contiguous()
    if got.dtype == BF:  # bit patterns: the poison must come back as the poison
        bad = got.view(torch.int16) != want.view(torch.int16)
    else:
        bad = ~(got == want)  # (a NaN in the hidden state is a mismatch)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[:6].tolist()
        first = [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]
        raise AssertionError(f'{what}: {nbad} of {bad.numel()} elements differ; first (index, got, want): {first}')


class Rig:
    """A crafted tower, its cache on the device (`cache`: what the kernels see; `want`: what the reference expects it to become)."""

    def __init__(self, E, layers, rich, B, Lmax, mode, ranges_first=False):
        self.E, self.layers, self.B, self.Lmax, self.mode, self.ranges_first = E, layers, B, Lmax, mode, ranges_first
        self.tw, self.P = _tower(E, layers, mode, rich)
        self.master = dx.cache_master(layers, B, Lmax, E, mode, DEV)
        # both caches end in a guard of eight NaN rows: a read one row past the last sequence meets the poison, a store there is seen
        numel, guard = self.master.numel(), 8 * 2 * E
        self.buf, self.wbuf = (torch.full((numel + guard,), float('nan'), dtype=BF, device=DEV) for _ in range(2))
        self.cache, self.want = self.buf[:numel].view(self.master.shape), self.wbuf[:numel].view(self.master.shape)
        self.x = dx.step_input(B, E, rich, DEV)
        self.lit = None

    def _light(self, pos):
        if self.mode != 'spot':
            return
        if self.lit is not None:
            dx.light(self.cache, self.lit, -128.0), dx.light(self.want, self.lit, -128.0)
        self.lit = dx.spot_keys(self.layers, self.B, self.E // 64, pos + 1, ranges_first=self.ranges_first)
        dx.light(self.cache, self.lit, 0.0), dx.light(self.want, self.lit, 0.0)

    def prepare(self, pos):
        """Rows < pos valid, rows >= pos NaN (row pos too: the step must overwrite it and never read it)."""
        self.cache.copy_(self.master)
        dx.poison_from(self.cache, pos)
        self.want.copy_(self.cache)
        self.lit = None
        self._light(pos)

    def advance(self, pos):
        """After a checked step at pos - 1: the cache stays as the step left it; (spot) the spotlights move to this position's keys."""
        self._light(pos)

    def check(self, sess, pos, what):
        y = sess.step(self.x).clone()
        info = {}
        ref = dx.reference_step(self.P, self.want, self.x, pos, info)
        dx.assert_exact_conditions(info, what)
        _same(y, ref, f'{what}: hidden state')
        _same(self.cache, self.want, f'{what}: cache after the step [layer, sequence, position, K|V]')
        _same(self.buf[self.cache.numel():], self.wbuf[self.cache.numel():], f'{what}: the guard rows behind the cache')
        assert int(sess.pos) == pos + 1 and sess.host_pos == pos + 1, f'{what}: the device position did not advance by exactly one'


def _launch_positions(rig, ns, what):
    """Five-launch form: one step per cache length n, the cache rebuilt in between."""
    sess = rig.tw.decode_session(rig.cache, 0, graph=False, fused='launches')
    assert not sess.persistent
    for n in ns:
        pos = n - 1
        rig.prepare(pos)
        sess.seek(pos)
        rig.check(sess, pos, f'{what} n={n}')


def _attn_params():
    return [pytest.param(name, B, id=f'{name}-B{B}') for name, c in dx.ATTN_CASES.items() for B in c['B']]


@pytest.mark.parametrize('mode', dx.MODES)
@pytest.mark.parametrize('name,B', _attn_params())
def test_five_launch_step_attention_boundaries(name, B, mode):
    """attn_decode2_kernel<4,2> (Lmax 512), <8,3> (Lmax 4,096; batch 1 on the vector-ALU linear layers) and <8,2> (12 heads x 43 / 64
    sequences, Lmax 1,152) at the cache lengths around every switch of theirs."""
    c = dx.ATTN_CASES[name]
    rig = Rig(c['E'], 1, False, B, c['Lmax'], mode)
    _launch_positions(rig, c['n'], f'{name} B={B} {mode}')


@pytest.mark.parametrize('mode', dx.MODES)
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'replayed'])
@pytest.mark.parametrize('Lmax', sorted(dx.PERSISTENT_RUNS))
@pytest.mark.parametrize('B', [1, 2])
def test_persistent_step_attention_boundaries(B, Lmax, graph, mode):
    """decode_persistent_kernel<1> / <2>: runs of consecutive positions (empty key ranges at n < 4; the second 256-key pass from
    n = 1,025; four passes at n = 4,096), eager and captured once then replayed; no poll timed out."""
    rig = Rig(768, 1, False, B, Lmax, mode, ranges_first=True)
    for run in dx.PERSISTENT_RUNS[Lmax]:
        rig.prepare(run[0] - 1)
        sess = rig.tw.decode_session(rig.cache, run[0] - 1, graph=graph, fused=True)
        assert sess.persistent
        for i, n in enumerate(run):
            if i:
                rig.advance(n - 1)
            rig.check(sess, n - 1, f'persistent B={B} Lmax={Lmax} {"replayed" if graph and i else "eager"} {mode} n={n}')
        assert (sess.graph is not None) == graph
        assert int(sess.ws[1]) == 0 and int(sess.ws[0]) == len(run)
        sess.check()


def _linear_params():
    out = []
    for E, Bs in dx.LINEAR_B.items():
        for B in Bs:
            forms = ['launches'] + (['persistent'] if B <= 2 and E == 768 else [])
            out += [pytest.param(E, B, f, id=f'E{E}-B{B}-{f}') for f in forms]
    return out


@pytest.mark.parametrize('mode', dx.MODES)
@pytest.mark.parametrize('E,B,form', _linear_params())
def test_full_exact_step_every_linear_form(E, B, form, mode):
    """Two layers with the richer parameters on a 64-position cache, at n = 33 and at the last row n = Lmax: every row-block / tile
    form of gemv16_mfma_kernel (batches 3..64), gemv_rows_kernel and the persistent step (1-2), the layer stride of a slice of a shared
    cache (batch 70 = 64 + 6), the K|V append of both layers and the position advance."""
    rig = Rig(E, 2, True, B, dx.LINEAR_LMAX, mode)
    what = f'E={E} B={B} {form} {mode}'
    if form == 'launches':
        _launch_positions(rig, dx.LINEAR_N, what)
        return
    for n in dx.LINEAR_N:
        rig.prepare(n - 1)
        sess = rig.tw.decode_session(rig.cache, n - 1, graph=False, fused=True)
        assert sess.persistent
        rig.check(sess, n - 1, f'{what} n={n}')
        assert int(sess.ws[1]) == 0
        sess.check()
