"""Trainer telemetry on the GPU.  Kernel level, in the guarded, padded, poisoned buffers of tests/guarded.py: mmvid_segment_stats
against its host replica (tests/telemetry_ref.py) bit for bit -- segment lengths around every boundary of the chunking, NaN between the
segments, planted non-finite gradients, the lazy table, the skip verdict, the ring and its gate, device scalars, a corrupted table,
every refusal.  Trainer level, on the small BERT of tests/test_guard_gpu.py in deterministic mode: telemetry only reads, a trainer
without it launches what it always launched, a record restated from the gradients and the weights, a skipped step located, captured
against eager, the ring's wrap.  NaN and inf in a gradient buffer are ordinary data: no test provokes a fault."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

import mmvid_amd
import optim_ref
import telemetry_ref as R
from guarded import Guarded, call_abi, ptr_of
from test_deterministic_step_gpu import small_case
from test_guard_gpu import forward_backward, make, one_step, same_bits
from test_models_gpu import DEV

pytestmark = pytest.mark.gpu
F32 = np.float32
CH = R.CHUNK
ALIGN = 128
U = 2.0**-24
ENTRY = 'mmvid_segment_stats'
# every boundary of the chunking, and one segment of more than 256 chunks (pass 2 takes a second trip)
LENGTHS = (1, 3, 4, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 5, 257 * CH + 11)
SMALL = (5, 3 * CH + 2, 1, 300)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if bad.any():
        i = np.argwhere(bad)[:4]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits; first (index, got, want): '
                             f'{[(tuple(k), got[tuple(k)], want[tuple(k)]) for k in i]}')


# -------------------------------------------------------------------------------------------------------------- kernel level
def make_case(numels, seed):
    """Flat buffers g, p, m, v (numpy fp32) holding the segments at multiples of 128, NaN in the padding between them."""
    rng = np.random.default_rng(seed)
    offs, tot = [], 0
    for n in numels:
        offs.append(tot)
        tot += -(-n // ALIGN) * ALIGN
    tot = offs[-1] + numels[-1]  # the buffers end with the last segment: the back guard begins there
    g = (rng.standard_normal(tot) * np.exp(rng.uniform(-6, 2, tot))).astype(F32)
    p = rng.standard_normal(tot).astype(F32)
    m = (rng.standard_normal(tot) * 1e-2).astype(F32)
    v = (rng.uniform(0, 1, tot)**4 * 1e-3).astype(F32)
    inside = np.zeros(tot, bool)
    for o, n in zip(offs, numels):
        inside[o:o + n] = True
    for a in (g, p, m, v):
        a[~inside] = np.nan
    return dict(offs=offs, numels=list(numels), n=tot, g=g, p=p, m=m, v=v, tables=R.plan(offs, numels))


def fresh_state(segments, chunks, slots):
    rng = np.random.default_rng(segments * 1000 + slots)  # rings that hold something: a slot that is not written must keep it
    return dict(count=np.zeros(1, np.int32), partials_f=None, partials_i=None,
                ring_f=rng.standard_normal((slots, segments, 4)).astype(F32), ring_i=rng.integers(0, 99, (slots, segments, 2)).astype(np.int32),
                head_i=np.zeros((slots, 4), np.int32), head_f=np.zeros((slots, 2), F32))


def launch(case, state=None, *, step=7, lr=1e-3, step_dev=None, lr_dev=None, lazy=None, skip=None, every=1, slots=1, tables=None,
           expect_error=None, shift=None, override=None):
    """One call of mmvid_segment_stats on guarded copies of the case's buffers and of `state` (what an earlier call left; None: a fresh
    ring, count 0).  Every guard zone of every operand is checked.  -> the new state, as numpy."""
    off, ln, c0, chunks = tables if tables is not None else case['tables']
    S = len(off)
    state = dict(state) if state is not None else fresh_state(S, chunks, slots)
    t = torch.from_numpy
    G, P, M, V = (Guarded(t(case[k])) for k in 'gpmv')
    OFF, LEN, C0 = (Guarded(torch.tensor(x, dtype=torch.int64)) for x in (off, ln, c0))
    SD = None if step_dev is None else Guarded(torch.tensor([float(step_dev)]))
    LR = None if lr_dev is None else Guarded(torch.tensor([float(lr_dev)]))
    SK = None if skip is None else Guarded(torch.tensor([int(skip)], dtype=torch.int32))
    fl, lo, rows, rowlen = lazy if lazy is not None else (None, 0, 0, 0)
    FL = None if fl is None else Guarded(t(np.asarray(fl, np.uint8)))
    count = int(state['count'][0])
    gated = expect_error is not None or count % every != 0
    if state['partials_f'] is None:
        if gated:
            state['partials_f'], state['partials_i'] = np.full((chunks, 4), 7.0, F32), np.full((chunks, 2), 7, np.int32)
        else:  # plain outputs: check() demands that every element was stored
            PF, PI = Guarded(role='out', shape=(chunks, 4), dtype=torch.float32), Guarded(role='out', shape=(chunks, 2), dtype=torch.int32)
    if state['partials_f'] is not None:
        PF, PI = Guarded(base=t(state['partials_f'])), Guarded(base=t(state['partials_i']))
    CNT = Guarded(base=t(state['count']))
    RF, RI = Guarded(base=t(state['ring_f']).reshape(slots * S, 4)), Guarded(base=t(state['ring_i']).reshape(slots * S, 2))
    HI, HF = Guarded(base=t(state['head_i'])), Guarded(base=t(state['head_f']))
    a = dict(g=G.ptr, p=P.ptr, m=M.ptr, v=V.ptr, n=case['n'], off=OFF.ptr, len=LEN.ptr, c0=C0.ptr, segments=S, chunks=chunks, lr=float(lr),
             lr_dev=ptr_of(LR), b1=BETA1, b2=BETA2, eps=EPS, step=int(step), step_dev=ptr_of(SD), flags=ptr_of(FL), lo=lo, rows=rows, rowlen=rowlen,
             skip=ptr_of(SK), every=every, slots=slots, count=CNT.ptr, pf=PF.ptr, pi=PI.ptr, rf=RF.ptr, ri=RI.ptr, hi=HI.ptr, hf=HF.ptr)
    a.update(override or {})  # arguments as the call gets them, whatever the buffers above were sized for
    for k, by in (shift or {}).items():  # a pointer moved by a few bytes: misaligned
        a[k] = ctypes.c_void_p(a[k].value + by)
    what = f'{ENTRY} S={S} chunks={chunks} count={count} every={every} slots={slots} skip={skip} lazy={lazy is not None}'
    if expect_error is not None:
        from mmvid_amd import _lib
        with pytest.raises(_lib.MMVIDError, match=expect_error):
            call_abi(ENTRY, *a.values())
    else:
        call_abi(ENTRY, *a.values())
    for name, op in (('g', G), ('p', P), ('m', M), ('v', V), ('seg_off', OFF), ('seg_len', LEN), ('seg_chunk0', C0), ('step_dev', SD),
                     ('lr_dev', LR), ('skip_dev', SK), ('row_flags', FL)):
        if op is not None:
            op.check(f'{what}: {name}')
    return dict(count=CNT.check(what + ': count_dev').numpy(), partials_f=PF.check(what + ': partials_f').numpy(),
                partials_i=PI.check(what + ': partials_i').numpy(), ring_f=RF.check(what + ': ring_f').numpy().reshape(slots, S, 4),
                ring_i=RI.check(what + ': ring_i').numpy().reshape(slots, S, 2), head_i=HI.check(what + ': head_i').numpy(),
                head_f=HF.check(what + ': head_f').numpy())


def assert_record(state, slot, want, what, d_exact=True):
    rf, ri, total = want
    cols = slice(0, 4) if d_exact else slice(0, 3)
    assert_bits(state['ring_f'][slot][:, cols], rf[:, cols], f'{what}: ring_f (sums bit for bit, absmax equal)')
    assert np.array_equal(state['ring_i'][slot], ri), f'{what}: ring_i {state["ring_i"][slot].tolist()} != {ri.tolist()}'
    assert_bits(state['head_f'][slot][1:], np.array([total], F32), f'{what}: the total')


@pytest.fixture(scope='module')
def big():
    """The eleven-segment case and its replica record at host scalars (t = 7): computed once, shared, unchanged."""
    case = make_case(LENGTHS, 11)
    stepsz, bc2s = R.host_scalars(1e-3, BETA1, BETA2, 7)
    return case, R.record(case['g'], case['p'], case['m'], case['v'], case['tables'], stepsz, bc2s, EPS), (stepsz, bc2s)


def test_records_equal_the_replica_on_every_length(big):
    case, want, _ = big
    assert case['tables'][3] == 1 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 + 258 and max(LENGTHS) > 256 * CH
    got = launch(case)
    assert_record(got, 0, want, 'eleven segments')
    assert got['head_i'].tolist() == [[0, 7, 0, 1]] and got['count'].tolist() == [1]
    assert_bits(got['head_f'][0][:1], np.array([1e-3], F32), 'head_f: lr')
    assert want[1][:, 0].tolist() == [0] * len(LENGTHS) and want[1][:, 1].tolist() == list(LENGTHS)
    assert np.isfinite(got['ring_f']).all()  # the NaN between the segments reached no statistic


def test_planted_nonfinite_values_stay_in_their_segment(big):
    case, clean, (stepsz, bc2s) = big
    for s in (3, 7, 10):  # lengths 255, CHUNK and 257 CHUNK + 11
        c = dict(case, g=case['g'].copy())
        o, n = case['offs'][s], LENGTHS[s]
        c['g'][o], c['g'][o + n - 1], c['g'][o + n // 2] = np.nan, np.inf, -np.inf
        got = launch(c)
        want = R.record(c['g'], c['p'], c['m'], c['v'], c['tables'], stepsz, bc2s, EPS)
        assert_record(got, 0, want, f'NaN, +inf, -inf planted in segment {s}')
        assert got['ring_i'][0][:, 0].tolist() == [3 if k == s else 0 for k in range(len(LENGTHS))]
        others = [k for k in range(len(LENGTHS)) if k != s]
        assert_bits(got['ring_f'][0][others], clean[0][others], f'planted in segment {s}: the other segments')
        assert np.isfinite(got['ring_f']).all() and float(got['ring_f'][0][s, 0]) < float(clean[0][s, 0])


@pytest.mark.parametrize('rowlen,rows', [(8, 5), (12, 9), (8, 6), (12, 7)])
def test_lazy_table(rowlen, rows):
    lo = 128  # (a multiple of 4: the table is the second segment)
    case = make_case((7, rows * rowlen, 6), rowlen * 100 + rows)
    assert case['offs'][1] == lo
    stepsz, bc2s = R.host_scalars(1e-3, BETA1, BETA2, 7)
    for name, flags in (('all', np.ones(rows, np.uint8)), ('none', np.zeros(rows, np.uint8)), ('alternating', (np.arange(rows) % 2).astype(np.uint8))):
        c = dict(case, g=case['g'].copy(), m=case['m'].copy(), v=case['v'].copy())
        for r in np.nonzero(flags == 0)[0]:  # poison where Adam did not go: it must not show
            for k, poison in (('g', np.inf), ('m', np.nan), ('v', np.nan)):
                c[k][lo + r * rowlen:lo + (r + 1) * rowlen] = poison
        lazy = (flags, lo, rows, rowlen)
        got = launch(c, lazy=lazy)
        want = R.record(c['g'], c['p'], c['m'], c['v'], c['tables'], stepsz, bc2s, EPS, lazy=lazy)
        assert_record(got, 0, want, f'lazy table {rows} x {rowlen}, flags {name}')
        assert np.isfinite(got['ring_f']).all() and got['ring_i'][0][:, 0].tolist() == [0, 0, 0]
        assert got['ring_i'][0][1, 1] == int(flags.sum()) * rowlen
        p64 = case['p'][lo:lo + rows * rowlen].astype(np.float64)
        assert abs(float(got['ring_f'][0][1, 2]) - float((p64**2).sum())) <= (R.sum_depth(rows * rowlen) + 2) * U * float((p64**2).sum())  # every row
        if name == 'none':
            assert got['ring_f'][0][1].tolist()[0:2] == [0.0, 0.0] and float(got['ring_f'][0][1, 3]) == 0.0


def test_skip_verdict():
    case = make_case(SMALL, 5)
    case['g'][case['offs'][1] + 17] = np.nan
    case['g'][case['offs'][3]] = -np.inf
    stepsz, bc2s = R.host_scalars(1e-3, BETA1, BETA2, 7)
    runs = {skip: launch(case, skip=skip) for skip in (None, 0, 1)}
    for skip, got in runs.items():
        want = R.record(case['g'], case['p'], case['m'], case['v'], case['tables'], stepsz, bc2s, EPS, skip=bool(skip))
        assert_record(got, 0, want, f'skip_dev {skip}')
        assert got['head_i'].tolist() == [[0, 7, int(bool(skip)), 1]]
    for k in ('ring_f', 'ring_i', 'head_f', 'partials_f', 'partials_i'):
        assert_bits(runs[0][k], runs[None][k], f'skip_dev = 0 against no skip_dev: {k}')
    assert bits(runs[1]['ring_f'][0][:, 3]).tolist() == [0] * len(SMALL)  # +0 everywhere: no update happened
    assert (runs[0]['ring_f'][0][:, 3] > 0).all()
    assert_bits(runs[1]['ring_f'][0][:, :3], runs[0]['ring_f'][0][:, :3], 'the g statistics and p_sumsq with skip = 1 against skip = 0')
    assert np.array_equal(runs[1]['ring_i'], runs[0]['ring_i']) and runs[1]['ring_i'][0][:, 0].tolist() == [0, 1, 0, 1]
    assert_bits(runs[1]['head_f'], runs[0]['head_f'], 'the header floats')


@pytest.mark.parametrize('every', [1, 2, 3])
def test_ring_and_gate_over_seven_calls(every):
    slots = 2
    case = make_case(SMALL, 6)
    ring = None
    state = None
    for call in range(7):
        t, lr = call + 1, 1e-3 * (call + 1)
        before = state
        state = launch(case, state, step=t, lr=lr, every=every, slots=slots, skip=call % 2)
        if ring is None:
            ring = R.Ring(len(SMALL), every, slots)
            ring.ring_f[:], ring.ring_i[:] = fresh_state(len(SMALL), case['tables'][3], slots)['ring_f'], fresh_state(len(SMALL), case['tables'][3], slots)['ring_i']
        stepsz, bc2s = R.host_scalars(lr, BETA1, BETA2, t)
        rec = R.record(case['g'], case['p'], case['m'], case['v'], case['tables'], stepsz, bc2s, EPS, skip=bool(call % 2))
        k = ring.call(rec, t, call % 2, lr)
        what = f'every={every} call {call}'
        assert (k is None) == (call % every != 0) and state['count'].tolist() == [call + 1] == [ring.count]  # a gated call still counts
        assert_bits(state['ring_f'], ring.ring_f, what + ': ring_f')
        assert_bits(state['ring_i'], ring.ring_i, what + ': ring_i')
        assert_bits(state['head_i'], ring.head_i, what + ': head_i')
        assert_bits(state['head_f'], ring.head_f, what + ': head_f')
        if k is None:  # gated: byte for byte what the call found
            for key in ('ring_f', 'ring_i', 'head_i', 'head_f', 'partials_f', 'partials_i'):
                assert_bits(state[key], before[key], f'{what} (gated): {key}')
    assert state['head_i'][:, 3].tolist() == [1, 1]


def rel_update(t, pow_ulps):
    """How far two fp32 evaluations of d = ((lr / bc1) m) / (sqrtf(v) / bc2s + eps) can lie apart, relative to d, when their powers
    b^t carry pow_ulps ulps of error BETWEEN them: bc1 = 1 - b1^t moves by pow_ulps ulp(b1^t) / bc1 (+ 2 u: its subtraction, rounded
    on either side), lr / bc1 adds 2 u; bc2 = 1 - b2^t likewise, halved by the root (+ u each for the root): d is linear in lr / bc1
    and moves by at most the relative change of bc2s (d = (lr / bc1) m bc2s / (sqrt(v) + eps bc2s)); the four operations per element
    that follow round on either side: 8 u.  First-order terms, all below 1e-3, so (1 + 1e-3) covers the products."""
    p1, p2 = float(F32(BETA1))**t, float(F32(BETA2))**t
    d1 = pow_ulps * optim_ref.ulp32(p1) / (1.0 - p1) + 2 * U + 2 * U
    d2 = 0.5 * (pow_ulps * optim_ref.ulp32(p2) / (1.0 - p2) + 2 * U) + 2 * U
    return (d1 + d2 + 8 * U) * (1 + 1e-3)


@pytest.mark.parametrize('t', [1, 3, 1000])
def test_device_scalars_against_host_arguments(t):
    case = make_case(SMALL, 7)
    lr = float(F32(3e-4))
    host = launch(case, step=t, lr=lr)
    dev = launch(case, step=0, lr=123.0, step_dev=t, lr_dev=lr)  # the host arguments are overridden (step < 1 is allowed with step_dev)
    for k in ('ring_i', 'head_i', 'head_f', 'partials_i'):
        assert_bits(dev[k], host[k], f't={t}: {k} with device scalars against host arguments')
    assert_bits(dev['ring_f'][0][:, :3], host['ring_f'][0][:, :3], f't={t}: g and p statistics')
    # d_sumsq: the device's powf against the host's (POW_ULPS_DEVICE + POW_ULPS_HOST between them), squared (twice the relative change),
    # plus the two summations
    for s, n in enumerate(SMALL):
        a, b = float(dev['ring_f'][0][s, 3]), float(host['ring_f'][0][s, 3])
        bound = 2 * rel_update(t, optim_ref.POW_ULPS_DEVICE + optim_ref.POW_ULPS_HOST) + 2 * (R.sum_depth(n) + 2) * U
        print(f't={t} segment {s}: d_sumsq device {a!r} host {b!r} relative difference {abs(a - b) / b:.3e} bound {bound:.3e}')
        assert abs(a - b) <= bound * b


def test_corrupted_table_stays_inside_the_buffers(big):
    case, want, _ = big
    off, ln, c0, chunks = (list(x) if isinstance(x, list) else x for x in case['tables'])
    n = case['n']
    off[1], ln[1] = n + 4096, 3              # an offset beyond n
    off[4], ln[4] = -999, 256                # a negative offset
    ln[6] = 1 << 50                          # a huge length
    off[8], ln[8] = (1 << 62) + 2, -5        # a huge offset that is no multiple of 4, a negative length
    intact = [0, 2, 3, 5, 7, 9, 10]
    got = launch(case, tables=(off, ln, c0, chunks))  # the call returns; every guard zone is intact (checked in there)
    assert_bits(got['ring_f'][0][intact], want[0][intact], 'segments whose entries were left intact')
    assert np.array_equal(got['ring_i'][0][intact], want[1][intact])
    assert got['count'].tolist() == [1] and got['head_i'][0, 3] == 1
    c0 = list(case['tables'][2])
    c0[2], c0[5], c0[9] = -7, 1 << 40, 3     # chunk indices out of range and out of order: wrong numbers, no stray access
    launch(case, tables=(off, ln, c0, chunks))


def test_every_refusal_returns_an_error_and_writes_nothing():
    case = make_case(SMALL, 8)
    S, chunks = len(SMALL), case['tables'][3]
    refusals = [(dict([(k, None)]), 'NULL') for k in ('g', 'p', 'm', 'v', 'off', 'len', 'c0', 'count', 'pf', 'pi', 'rf', 'ri', 'hi', 'hf')]
    shifts = [({k: 8}, '16-byte') for k in ('g', 'p', 'm', 'v')] + [({k: 4}, '8-byte') for k in ('off', 'len', 'c0')]
    shifts += [({k: 2}, '4-byte') for k in ('count', 'pf', 'pi', 'rf', 'ri', 'hi', 'hf')]
    refusals += [(dict(n=-1), 'negative'), (dict(segments=0), 'segments'), (dict(segments=65537), 'segments'), (dict(chunks=S - 1), 'chunks'),
                 (dict(chunks=case['n'] // CH + S + 1), 'chunks'), (dict(every=0), 'every'), (dict(slots=0), 'slots'), (dict(step=0), 'step'),
                 (dict(b1=1.0), 'beta'), (dict(b2=float('nan')), 'beta'), (dict(b2=-0.5), 'beta')]
    state = fresh_state(S, chunks, 2)
    state['partials_f'], state['partials_i'] = np.full((chunks, 4), 7.0, F32), np.full((chunks, 2), 7, np.int32)
    for kw, sh, word in [(kw, None, word) for kw, word in refusals] + [(None, sh, word) for sh, word in shifts]:
        after = launch(case, state, slots=2, expect_error=word, override=kw, shift=sh)  # (every guard zone is checked in there)
        for k in state:
            assert_bits(after[k], state[k], f'refused ({kw or sh}): {k} must keep every byte')
    flags = np.ones(4, np.uint8)
    for lazy in ((flags, 8, 4, 10), (flags, 6, 4, 12), (flags, 8, 4, 1 << 20), (flags, -4, 4, 12)):
        after = launch(case, state, slots=2, lazy=lazy, expect_error='lazy')
        for k in state:
            assert_bits(after[k], state[k], f'refused (lazy {lazy[1:]}): {k} must keep every byte')
    for k in ('lr_dev', 'step_dev', 'skip'):
        kw = dict(lr_dev=1e-3) if k == 'lr_dev' else dict(step_dev=3) if k == 'step_dev' else dict(skip=0)
        after = launch(case, state, slots=2, expect_error='4-byte', shift={k: 2}, **kw)
        for key in state:
            assert_bits(after[key], state[key], f'refused (misaligned {k}): {key} must keep every byte')
    # the wrapper: buffers that do not fit the plan are refused before the call
    from mmvid_amd import ops
    z, zi = torch.zeros(256, device=DEV), torch.zeros(16, device=DEV, dtype=torch.int32)
    tabs = tuple(torch.zeros(2, device=DEV, dtype=torch.int64) for _ in range(3))
    with pytest.raises(ValueError, match='do not fit'):
        ops.segment_stats(z, z, z, z, tabs, 2, 1, 1e-3, (0.9, 0.999), 1e-8, 1, 1, zi[:1], z[:8], zi[:4], z[:4], zi[:4], zi[:4], z[:2])


# ------------------------------------------------------------------------------------------------------------- trainer level
STEPS = 5
PROBE = 2  # the step (from 0) whose record is restated from the gradients and the weights


@pytest.fixture(scope='module')
def case():
    base, inps = small_case(False, steps=STEPS)
    return base, [dict(inp, gain=torch.tensor(1.0, device=DEV)) for inp in inps]


def tstate(tr):
    return {k: getattr(tr, k).clone() for k in ('P', 'M', 'V', 'E', 'S')}


def ring_bytes(tr):
    return {k: tr._tel[k].cpu().numpy().copy() for k in ('ring_f', 'ring_i', 'head_i', 'head_f', 'count')}


@pytest.fixture(scope='module')
def runs(case):
    """Per lazy-row mode, eager, deterministic mode, guard and EMA on: five steps with telemetry_every=1 (three slots with lazy rows,
    the default 64 without) and the same five without telemetry.  Around step PROBE the gradients and the weights are taken to the host
    in fp64.  Shared, unchanged."""
    base, inps = case
    before = mmvid_amd.set_deterministic(True)
    out = {}
    try:
        for lazy in (True, False):
            r = {}
            m, tr, fn = make(base, lazy_rows=lazy, skip_nonfinite=True, telemetry_every=1, **(dict(telemetry_slots=3) if lazy else {}))
            assert (tr._lazy is not None) == lazy and tr._tel is not None
            r['names'], r['numels'], r['numel'], r['S'] = list(tr.names), [p.numel() for p in tr.params], tr.numel, len(tr.names)
            for i, inp in enumerate(inps):
                forward_backward(tr, fn, inp)
                if i == PROBE:
                    r['grads'] = [p.grad.detach().double().cpu().reshape(-1) for p in tr.params]
                    r['p_before'] = [p.detach().double().cpu().reshape(-1) for p in tr.params]
                tr.step()
                if i == PROBE:
                    r['p_after'] = [p.detach().double().cpu().reshape(-1) for p in tr.params]
                    r['record'], r['layers'] = tr.telemetry(last=1)[0], tr.telemetry(last=1, by='layer')[0]
                    r['guard'] = tr.guard_stats()
                    r['counted'] = tr._tel['ring_i'].view(-1, len(tr.names), 2)[PROBE % tr.telemetry_slots, :, 1].tolist()
                    if lazy:
                        z = tr._lazy
                        r['table'] = (z['name'], int(z['flags'].sum().item()) * z['rowlen'], z['rows'] * z['rowlen'])
            r['state'], r['all'], r['newest'], r['nonfinite'] = tstate(tr), tr.telemetry(), tr.telemetry(last=1), tr.first_nonfinite()
            with tr.ema_weights():  # the readers touch the ring only, nothing the scope re-points: allowed inside it
                r['in_scope'] = tr.telemetry()
            r['sd_keys'] = sorted(map(str, tr.state_dict()))
            r['tr'], r['keep'] = tr, (m, fn)  # (test_ring_wraps loads a checkpoint into it: nothing else reads it)
            m2, tr2, fn2 = make(base, lazy_rows=lazy, skip_nonfinite=True)
            assert tr2._tel is None
            for inp in inps:
                one_step(tr2, fn2, inp)
            r['state_off'], r['sd_off'] = tstate(tr2), tr2.state_dict()
            del m2, tr2, fn2
            out[lazy] = r
    finally:
        mmvid_amd.set_deterministic(before)
    yield out
    out.clear()


@pytest.fixture
def deterministic_mode():
    before = mmvid_amd.set_deterministic(True)
    yield
    mmvid_amd.set_deterministic(before)


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_telemetry_only_reads(runs, lazy):
    r = runs[lazy]
    for k in ('P', 'M', 'V', 'S', 'E'):
        same_bits(r['state'][k], r['state_off'][k], f'five steps with telemetry_every=1 against None: {k}')
    assert r['sd_keys'] == sorted(map(str, r['sd_off'])) == ['ema', 'frontend', 'guard', 'names', 'param_groups', 'state']  # no ring in a checkpoint
    assert r['in_scope'] == r['all'] and r['nonfinite'] == []


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_a_record_restated_from_the_gradients_and_the_weights(runs, lazy):
    r = runs[lazy]
    rec = r['record']
    assert rec['record'] == PROBE and rec['step'] == PROBE + 1 and rec['skipped'] is False and rec['lr'] == float(F32(1e-4))
    assert list(rec['params']) == r['names']
    gsq_total = 0.0
    for s, name in enumerate(r['names']):
        got, n = rec['params'][name], r['numels'][s]
        # a sum of n non-negative squares through at most d = sum_depth(n) additions: (d + 2) u relative (tests/test_telemetry_host.py:
        # sums_bound), halved by the square root; + u for the fp64 reference
        rel = 0.5 * (R.sum_depth(n) + 2) * U * (1 + 1e-3) + 2.0**-50
        gn, wn = float(r['grads'][s].norm()), float(r['p_after'][s].norm())
        assert abs(got['grad_norm'] - gn) <= rel * gn, (name, got['grad_norm'], gn)
        assert abs(got['weight_norm'] - wn) <= rel * wn, (name, got['weight_norm'], wn)
        assert got['grad_absmax'] == float(r['grads'][s].abs().max()) and got['grad_nonfinite'] == 0
        # update_norm against |P_before - P_after|: Adam formed p' = fl(p - d), so (p - p') - d is the rounding of that subtraction,
        # at most half an ulp of the larger of |p|, |p'| per element: sqrt(sum (ulp_i / 2)^2) in the norm.  The record's d is the
        # kernel's own evaluation of the same formula (rel_update: the device's powf on both sides), summed with the pass-1/2 tree.
        pb, pa = r['p_before'][s], r['p_after'][s]
        big_ = torch.maximum(pb.abs(), pa.abs()).clamp_min(2.0**-126)
        half_ulp = torch.exp2(torch.floor(torch.log2(big_)) - 23) / 2
        term1 = float(half_ulp.pow(2).sum().sqrt())
        moved = float((pb - pa).norm())
        term2 = (rel_update(PROBE + 1, 2 * optim_ref.POW_ULPS_DEVICE) + rel) * (moved + term1)
        print(f'{name}: update_norm {got["update_norm"]:.6e} |dP| {moved:.6e} subtraction term {term1:.3e} formula term {term2:.3e}')
        assert abs(got['update_norm'] - moved) <= term1 + term2, name
        assert got['update_ratio'] == got['update_norm'] / got['weight_norm']
        gsq_total += gn * gn
    # the record's norm against the guard's: two fp32 sums of the same squares, each within its depth of the exact one (optim_ref.
    # sqnorm_depth for grad_sqnorm_rows; the record's total adds ceil(S / 256) + 8 additions to the deepest segment), halved by the
    # roots, + 2 u for the guard's sqrtf and product
    k, kb = optim_ref.sqnorm_depth(r['numel'], False)
    d_total = R.sum_depth(max(r['numels'])) + 2 + -(-r['S'] // 256) + 8
    exact = math.sqrt(gsq_total)
    assert abs(rec['grad_norm'] - exact) <= 0.5 * d_total * U * (1 + 1e-3) * exact
    assert abs(rec['grad_norm'] - r['guard']['grad_norm']) <= (0.5 * (k + kb + d_total) + 2) * U * (1 + 1e-3) * exact
    # by='layer': squares summed, maxima taken, counts added, over the groups of telemetry_group
    from mmvid_amd.engine import telemetry_group
    layers = r['layers']['params']
    assert sorted(layers) == ['heads', 'layer.0', 'layer.1', 'tables']
    for key, got in layers.items():
        members = [rec['params'][n] for n in r['names'] if telemetry_group(n) == key]
        assert abs(got['grad_norm'] - math.sqrt(sum(x['grad_norm']**2 for x in members))) <= 1e-12 * got['grad_norm']
        assert abs(got['update_norm'] - math.sqrt(sum(x['update_norm']**2 for x in members))) <= 1e-12 * got['update_norm']
        assert got['grad_absmax'] == max(x['grad_absmax'] for x in members) and got['grad_nonfinite'] == 0
    if lazy:  # the table's statistics cover only the rows the step touched
        name, touched, whole = r['table']
        s = r['names'].index(name)
        assert r['counted'][s] == touched and 0 < touched < whole
        assert [c for k, c in enumerate(r['counted']) if k != s] == [n for k, n in enumerate(r['numels']) if k != s]
        assert rec['params'][name]['update_norm'] > 0
    else:
        assert r['counted'] == r['numels']


def test_ring_wraps(runs):
    r = runs[True]  # three slots, five steps
    assert [x['record'] for x in r['all']] == [2, 3, 4] and [x['step'] for x in r['all']] == [3, 4, 5]
    assert r['newest'] == r['all'][-1:] and len(r['newest']) == 1
    assert [x['record'] for x in runs[False]['all']] == [0, 1, 2, 3, 4]  # 64 slots: nothing was overwritten
    assert r['all'][0] == r['record']
    # the ring is diagnostics, not state: loading a checkpoint -- here one from a trainer without telemetry -- empties it
    tr = r['tr']
    tr.load_state_dict(r['sd_off'])
    assert tr.telemetry() == [] and tr.first_nonfinite() == [] and tr._tel['count'].item() == 0


def test_without_telemetry_a_step_launches_what_it_always_launched(case, deterministic_mode, monkeypatch):
    from mmvid_amd import _lib, ops
    base, inps = case
    seen = []
    real = _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', recorder)
    monkeypatch.setattr(ops, 'call', recorder)  # (ops binds the function by name at import)

    def step_launches(tr, fn):
        del seen[:]
        forward_backward(tr, fn, inps[0])
        k = len(seen)
        tr.step()
        return list(seen), [s for s in seen[k:] if s != 'mmvid_get_option']

    m, tr, fn = make(base)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_counter_add', 'mmvid_grad_sqnorm_rows', 'mmvid_adam_step_rows', 'mmvid_ema_update'] and ENTRY not in whole
    m, tr, fn = make(base, ema=False, lazy_rows=False)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_counter_add', 'mmvid_grad_sqnorm_det', 'mmvid_adam_step_rows'] and ENTRY not in whole
    m, tr, fn = make(base, skip_nonfinite=True)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_grad_sqnorm_rows', 'mmvid_step_guard', 'mmvid_adam_step_guarded', 'mmvid_ema_update_guarded'] and ENTRY not in whole
    # with telemetry: one more entry, behind the optimiser
    m, tr, fn = make(base, skip_nonfinite=True, telemetry_every=50)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_grad_sqnorm_rows', 'mmvid_step_guard', 'mmvid_adam_step_guarded', ENTRY, 'mmvid_ema_update_guarded']
    assert whole.count(ENTRY) == 1


def test_a_skipped_step_is_located(case, deterministic_mode):
    base, inps = case
    m, tr, fn = make(base, skip_nonfinite=True, telemetry_every=1)
    name = 'transformer.transformer.resblocks.1.mlp.c_fc.weight'
    one_step(tr, fn, inps[0])
    assert tr.first_nonfinite() == []
    forward_backward(tr, fn, inps[1])
    dict(m.named_parameters())[name].grad[5, 7] = float('inf')  # ordinary data in a gradient buffer
    tr.step()
    assert tr.first_nonfinite() == [name]
    rec = tr.telemetry(last=1)[0]
    assert rec['skipped'] is True and rec['record'] == 1 and rec['step'] == 1  # (one applied step so far)
    assert [n for n, x in rec['params'].items() if x['grad_nonfinite']] == [name] and rec['params'][name]['grad_nonfinite'] == 1
    assert all(x['update_norm'] == 0.0 for x in rec['params'].values())
    assert all(math.isfinite(x['grad_norm']) for x in rec['params'].values()) and rec['params'][name]['grad_norm'] > 0
    assert tr.telemetry(last=1, by='layer')[0]['params']['layer.1']['grad_nonfinite'] == 1
    assert tr.guard_stats()['last_skipped'] is True
    one_step(tr, fn, inps[2])
    rec = tr.telemetry(last=1)[0]
    assert rec['skipped'] is False and rec['record'] == 2 and rec['step'] == 2 and tr.first_nonfinite() == []
    assert rec['params'][name]['update_norm'] > 0 and all(x['update_norm'] > 0 for x in rec['params'].values() if x['grad_norm'] > 0)
    assert [x['skipped'] for x in tr.telemetry()] == [False, True, False]


def test_captured_run_equals_the_eager_run(case, deterministic_mode):
    from mmvid_amd.engine import GraphedStep
    base, inps = case
    kw = dict(skip_nonfinite=True, telemetry_every=2, telemetry_slots=4)
    m, tr, fn = make(base, **kw)
    step = GraphedStep(tr, fn, inps[0], warmup=2)  # two eager steps on inps[0], then the capture: it enqueues nothing, the counter stays
    assert step.graph is not None, step.capture_error
    assert tr._tel['count'].item() == 2 and tr._tel['head_i'].view(4, 4)[:, 3].tolist() == [1, 0, 0, 0]
    for inp in inps[1:3]:
        step(**inp)
    captured = ring_bytes(tr)
    records = tr.telemetry()
    m2, tr2, fn2 = make(base, **kw)
    for inp in (inps[0], inps[0], inps[1], inps[2]):
        one_step(tr2, fn2, inp)
    eager = ring_bytes(tr2)
    for k in eager:
        assert_bits(captured[k], eager[k], f'four steps, captured against eager: {k}')
    assert captured['count'].tolist() == [4] and [x['record'] for x in records] == [0, 2] and [x['step'] for x in records] == [1, 3]
    assert records == tr2.telemetry()
    for k in ('P', 'M', 'V', 'E', 'S'):
        same_bits(getattr(tr, k), getattr(tr2, k), f'captured against eager: {k}')
    # the readers read the device: refused while a stream captures
    x = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match='capture'):
            tr.telemetry()
        with pytest.raises(RuntimeError, match='capture'):
            tr.first_nonfinite()
    torch.cuda.synchronize()
