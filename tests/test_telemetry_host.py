"""Trainer telemetry without a GPU: the chunk plan, the host replica of mmvid_segment_stats (tests/telemetry_ref.py) against fp64 and
on hand-made cases of the lazy-row and skip rules, the header entry and its binding, its refusals (checked before any launch), and the
FlatTrainer side on a CPU trainer -- the keywords, the refusals of the readers, the unchanged checkpoint and the layer grouping."""
import ctypes
import re

import numpy as np
import pytest
import torch

import telemetry_ref as R
from test_host_logic import tiny_bert

F32 = np.float32
P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
ENTRY = 'mmvid_segment_stats'
ARGS = [P, P, P, P, I64, P, P, P, I, I64, F, P, F, F, F, I, P, P, I64, I64, I, P, I, I, P, P, P, P, P, P, P, P]
CH = R.CHUNK
ALIGN = 128


def bits(x):
    return np.asarray(x, F32).view(np.int32)


def layout(numels):
    offs, tot = [], 0
    for n in numels:
        offs.append(tot)
        tot += -(-n // ALIGN) * ALIGN
    return offs, tot


# ------------------------------------------------------------------------------------------------------------------- the plan
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return tiny_bert()


def trainer(model, **kw):
    from mmvid_amd.engine import FlatTrainer, backward_order
    return FlatTrainer(model, order=backward_order, **kw)


def check_plan(offsets, numels, total, chunk):
    from mmvid_amd import ops
    off, ln, c0, chunks = ops.telemetry_plan(offsets, numels, chunk)
    assert (off, ln, c0, chunks) == tuple(R.plan(offsets, numels, chunk))
    owner = np.full(total, -1, np.int64)  # the chunk every element of the flat buffer lies in; -1: none
    seen = 0
    for s in range(len(off)):
        n_chunks = (c0[s + 1] if s + 1 < len(off) else chunks) - c0[s]
        assert n_chunks == -(-ln[s] // chunk) >= 1
        for k in range(n_chunks):
            lo, hi = off[s] + k * chunk, off[s] + min(ln[s], (k + 1) * chunk)
            assert hi > lo and bool((owner[lo:hi] == -1).all())  # in exactly one chunk
            owner[lo:hi] = c0[s] + k
            seen += 1
    assert seen == chunks and c0[0] == 0 and c0 == sorted(c0)
    inside = np.zeros(total, bool)
    for o, n in zip(offsets, numels):
        inside[o:o + n] = True
    assert bool((owner[inside] >= 0).all()) and bool((owner[~inside] == -1).all())  # every element of a segment; no padding
    assert sum(-(-n // chunk) for n in numels) == chunks


def test_plan_covers_every_segment_element_once_and_no_padding(model):
    from mmvid_amd import _lib, ops
    assert ops.TELEMETRY_CHUNK == _lib.HEADER.constants['MMVID_TELEMETRY_CHUNK'] == CH == 4096
    for numels in ([1], [CH - 1], [CH], [CH + 1], [1, CH - 1, CH, CH + 1, 3, 2 * CH + 5], [257, 1, 300 * CH + 7]):
        offs, tot = layout(numels)
        check_plan(offs, numels, tot, CH)
    offs, tot = layout([5, 9, 1, 200])
    check_plan(offs, [5, 9, 1, 200], tot, 8)  # (the chunk is an argument of the planner)
    tr = trainer(model)  # the real flat layout of the tiny BERT
    numels = [p.numel() for p in tr.params]
    check_plan(tr.offsets, numels, tr.numel, CH)
    assert len(numels) == 44 and max(numels) > 256 * CH  # its table alone takes pass 2 into a second trip
    for bad in (([0], [0]), ([0, 128], [200, 5]), ([], []), ([0], [1, 2])):
        with pytest.raises(ValueError, match='telemetry_plan'):
            ops.telemetry_plan(*bad)


# ------------------------------------------------------------------------------------------------------------------ the replica
def sums_bound(L):
    """A sum of L non-negative terms t_i = fl(x_i^2), each term passing through at most d = sum_depth(L) additions: every rounding
    multiplies what it holds by (1 + e), |e| <= u = 2^-24, and the terms have one sign, so |sum_fp32 - sum| <= ((1 + u)^(d + 1) - 1) sum
    (d additions and the square).  (1 + u)^k - 1 <= k u / (1 - k u) < (k + 1) u for k u < 1e-5: (d + 2) u relative."""
    return (R.sum_depth(L) + 2) * 2.0**-24


def random_case(numels, seed, plant=True):
    rng = np.random.default_rng(seed)
    offs, tot = layout(numels)
    g = (rng.standard_normal(tot) * np.exp(rng.uniform(-6, 2, tot))).astype(F32)
    p = rng.standard_normal(tot).astype(F32)
    m = (rng.standard_normal(tot) * 1e-2).astype(F32)
    v = (rng.uniform(0, 1, tot)**4 * 1e-3).astype(F32)
    inside = np.zeros(tot, bool)
    for o, n in zip(offs, numels):
        inside[o:o + n] = True
    for a in (g, p, m, v):
        a[~inside] = np.nan  # padding belongs to no segment
    planted = {}
    if plant:
        for s, (o, n) in enumerate(zip(offs, numels)):
            if s % 2 == 1 and n >= 3:
                g[o], g[o + n - 1], g[o + n // 2] = np.nan, np.inf, -np.inf
                planted[s] = 3
    return offs, tot, g, p, m, v, planted


def test_replica_against_fp64():
    numels = [1, 3, 4, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 5, 257 * CH + 11]
    offs, tot, g, p, m, v, planted = random_case(numels, 1)
    tables = R.plan(offs, numels)
    stepsz, bc2s = R.host_scalars(1e-3, 0.9, 0.999, 7)
    rf, ri, total = R.record(g, p, m, v, tables, stepsz, bc2s, 1e-8)
    assert rf.dtype == F32 and ri.dtype == np.int32
    want_total = 0.0
    for s, (o, n) in enumerate(zip(offs, numels)):
        gs, ps = g[o:o + n].astype(np.float64), p[o:o + n].astype(np.float64)
        fin = np.isfinite(gs)
        gsq, psq = float((gs[fin]**2).sum()), float((ps**2).sum())
        d = R.update(stepsz, m[o:o + n], v[o:o + n], bc2s, 1e-8).astype(np.float64)  # the fp32 updates, summed in fp64
        dsq = float((d**2).sum())
        for k, want in ((0, gsq), (2, psq), (3, dsq)):
            err = abs(float(rf[s, k]) - want) / want if want else abs(float(rf[s, k]))
            print(f'segment {s} (length {n}) stat {k}: relative error {err:.3e}, bound {sums_bound(n):.3e}')
            assert err <= sums_bound(n), (s, k)
        assert float(rf[s, 1]) == (float(np.abs(gs[fin]).max()) if fin.any() else 0.0)  # exact
        assert ri[s].tolist() == [planted.get(s, 0), n]  # NaN, +inf and -inf are counted and left out of the sums
        assert np.isfinite(rf[s]).all()
        want_total += gsq
    assert abs(float(total) - want_total) / want_total <= (R.sum_depth(max(numels)) + 2 + 1 + 6 + 2) * 2.0**-24
    again = R.record(g, p, m, v, tables, stepsz, bc2s, 1e-8)  # the replica against itself
    assert np.array_equal(bits(rf), bits(again[0])) and np.array_equal(ri, again[1]) and bits(total) == bits(again[2])


def test_replica_order_is_the_documented_one():
    """Small enough to restate by hand: 4 elements are one thread's (x0^2 + x1^2) + (x2^2 + x3^2); the trips, the wave tree and pass 2
    follow -- with values chosen so that another order gives other bits."""
    e = F32(2.0**-24)
    sq = np.array([1.0, e, e, e], F32)  # (1 + e) + (e + e) = 1 + 2^-23; one after the other, every e is rounded away
    assert bits(R.sum_in_order(R.chunk_sums(sq))) == bits((sq[0] + sq[1]) + (sq[2] + sq[3])) == bits(F32(1.0 + 2.0**-23))
    assert bits(((sq[0] + sq[1]) + sq[2]) + sq[3]) == bits(F32(1.0))
    t = np.zeros(CH, F32)
    t[[0, 128, 1024, 4 * 64]] = [1.0, 2.0**-24, 2.0**-24, 3.0]  # threads 0 and 32 (one wave), thread 0's second trip, thread 64
    a0 = F32(1.0) + F32(2.0**-24)  # thread 0: its trips in order (rounds to 1)
    assert bits(R.chunk_sums(t)[0]) == bits((a0 + F32(2.0**-24)) + F32(3.0))
    c = np.zeros(300, F32)
    c[[0, 256, 1]] = [1.0, 2.0**-24, 2.0**-24]  # pass 2: thread 0 adds c[0] + c[256] first
    assert bits(R.sum_in_order(c)) == bits((F32(1.0) + F32(2.0**-24)) + F32(2.0**-24)) == bits(F32(1.0))


def test_lazy_rule_and_skip_rule_on_hand_made_cases():
    rowlen, rows, lo = 8, 5, 128
    numels = [7, rows * rowlen, 6]
    offs, tot = layout(numels)
    assert offs[1] == lo
    tables = R.plan(offs, numels)
    g, p, m, v = (np.full(tot, np.nan, F32) for _ in range(4))
    for o, n in zip(offs, numels):
        g[o:o + n], p[o:o + n], m[o:o + n], v[o:o + n] = 2.0, 3.0, 0.5, 0.25
    flags = np.array([1, 0, 1, 0, 0], np.uint8)
    for r in np.nonzero(flags == 0)[0]:  # unflagged rows: poison in g, m, v must not show
        for a in (g, m, v):
            a[lo + r * rowlen:lo + (r + 1) * rowlen] = np.nan
    stepsz, bc2s, eps = F32(0.5), F32(0.5), F32(1.0)
    d = (F32(0.5) * F32(0.5)) / (np.sqrt(F32(0.25)) / F32(0.5) + F32(1.0))  # 0.125
    rf, ri, total = R.record(g, p, m, v, tables, stepsz, bc2s, eps, lazy=(flags, lo, rows, rowlen))
    assert rf[:, 0].tolist() == [28.0, 64.0, 24.0] and rf[:, 1].tolist() == [2.0, 2.0, 2.0]  # the table: 2 flagged rows x 8 x 2^2
    assert rf[:, 2].tolist() == [63.0, 360.0, 54.0]                                            # p_sumsq counts every row
    assert rf[:, 3].tolist() == [7 * d * d, 16 * d * d, 6 * d * d] and float(d) == 0.125
    assert ri.tolist() == [[0, 7], [0, 16], [0, 6]] and float(total) == 116.0
    none = R.record(g, p, m, v, tables, stepsz, bc2s, eps, lazy=(np.zeros(rows, np.uint8), lo, rows, rowlen))
    assert none[0][1].tolist() == [0.0, 0.0, 360.0, 0.0] and none[1][1].tolist() == [0, 0]
    # the skip rule: d_sumsq is +0 everywhere, the g statistics and p_sumsq are what they were
    g[offs[2] + 1] = np.inf
    on = R.record(g, p, m, v, tables, stepsz, bc2s, eps, lazy=(flags, lo, rows, rowlen), skip=True)
    off_ = R.record(g, p, m, v, tables, stepsz, bc2s, eps, lazy=(flags, lo, rows, rowlen), skip=False)
    assert np.array_equal(bits(on[0][:, :3]), bits(off_[0][:, :3])) and np.array_equal(on[1], off_[1]) and bits(on[2]) == bits(off_[2])
    assert bits(on[0][:, 3]).tolist() == [0, 0, 0] and on[1][:, 0].tolist() == [0, 0, 1] and float(on[0][2, 0]) == 20.0


def test_slot_arithmetic_and_ring():
    assert [R.slot_of(c, 1, 2) for c in range(5)] == [0, 1, 0, 1, 0]
    assert [R.slot_of(c, 2, 2) for c in range(7)] == [0, None, 1, None, 0, None, 1]
    assert [R.slot_of(c, 3, 2) for c in range(7)] == [0, None, None, 1, None, None, 0]
    ring = R.Ring(2, 2, 2)
    rec = (np.ones((2, 4), F32), np.ones((2, 2), np.int32), F32(2.0))
    assert [ring.call(rec, t, t == 3, 0.5) for t in range(1, 6)] == [0, None, 1, None, 0] and ring.count == 5
    assert ring.head_i.tolist() == [[4, 5, 0, 1], [2, 3, 1, 1]] and ring.head_f.tolist() == [[0.5, 2.0], [0.5, 2.0]]


def test_host_scalars_are_the_c_librarys():
    stepsz, bc2s = R.host_scalars(1e-3, 0.9, 0.999, 1)
    assert stepsz.dtype == F32 and bc2s.dtype == F32
    assert bits(stepsz) == bits(F32(1e-3) / (F32(1.0) - F32(0.9))) and bits(bc2s) == bits(np.sqrt(F32(1.0) - F32(0.999)))


# ------------------------------------------------------------------------------------------------- the header and the binding
def test_telemetry_entry_point_is_declared_bound_and_built():
    from mmvid_amd import _cdecl, _lib, build
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)  # the strict reader: anything it does not know raises
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    assert 'telemetry' in build.SOURCES and 'Trainer telemetry' in text
    lib = _lib.load()
    assert ENTRY in hdr.functions and hdr.functions[ENTRY][0] is ctypes.c_int
    assert len(re.findall(r'\b%s\s*\(' % ENTRY, bare)) == 1
    assert _lib.EXT_SIGNATURES[ENTRY] == hdr.functions[ENTRY][1] == ARGS
    assert ENTRY not in _lib.SIGNATURES and ENTRY not in _lib.OTHER and ENTRY not in lib._mmvid_missing
    fn = getattr(lib, ENTRY)
    assert list(fn.argtypes) == ARGS and fn.restype is ctypes.c_int
    assert not hdr.constants and _lib.HEADER.constants['MMVID_TELEMETRY_MAX_SEGMENTS'] == 65536
    assert _lib.ABI_VERSION == _lib.HEADER.constants['MMVID_ABI_VERSION'] == lib.mmvid_abi_version()


def made_up_call(**kw):
    """mmvid_segment_stats through _lib.call with made-up addresses: the checks come before the launch, so nothing is dereferenced."""
    from mmvid_amd import _lib
    V = ctypes.c_void_p
    a = dict(g=V(1 << 20), p=V(2 << 20), m=V(3 << 20), v=V(4 << 20), n=10000, off=V(5 << 20), len=V(6 << 20), c0=V(7 << 20), segments=3,
             chunks=5, lr=1e-3, lr_dev=None, b1=0.9, b2=0.999, eps=1e-8, step=1, step_dev=None, flags=None, lo=0, rows=0, rowlen=0, skip=None,
             every=1, slots=2, count=V(8 << 20), pf=V(9 << 20), pi=V(10 << 20), rf=V(11 << 20), ri=V(12 << 20), hi=V(13 << 20), hf=V(14 << 20))
    assert set(kw) <= set(a)
    a.update(kw)
    _lib.call(ENTRY, *a.values(), None)


REFUSALS = [(dict([(k, None)]), 'NULL') for k in ('g', 'p', 'm', 'v', 'off', 'len', 'c0', 'count', 'pf', 'pi', 'rf', 'ri', 'hi', 'hf')]
REFUSALS += [(dict([(k, ctypes.c_void_p((1 << 20) + 8))]), '16-byte') for k in ('g', 'p', 'm', 'v')]
REFUSALS += [(dict([(k, ctypes.c_void_p((5 << 20) + 4))]), '8-byte') for k in ('off', 'len', 'c0')]
REFUSALS += [(dict([(k, ctypes.c_void_p((9 << 20) + 2))]), '4-byte')
             for k in ('lr_dev', 'step_dev', 'skip', 'count', 'pf', 'pi', 'rf', 'ri', 'hi', 'hf')]
REFUSALS += [(dict(n=-1), 'negative'), (dict(segments=0), 'segments'), (dict(segments=-3), 'segments'), (dict(segments=65537, chunks=70000), 'segments'),
             (dict(chunks=2), 'chunks'), (dict(chunks=6), 'chunks'), (dict(every=0), 'every'), (dict(every=-1), 'every'), (dict(slots=0), 'slots'),
             (dict(step=0), 'step'), (dict(step=-5), 'step'), (dict(b1=1.0), 'beta'), (dict(b1=-0.1), 'beta'), (dict(b2=1.0), 'beta'),
             (dict(b2=float('nan')), 'beta'), (dict(b1=float('nan')), 'beta'),
             (dict(flags=ctypes.c_void_p(15 << 20), lo=8, rows=5, rowlen=10), 'lazy'), (dict(flags=ctypes.c_void_p(15 << 20), lo=6, rows=5, rowlen=12), 'lazy'),
             (dict(flags=ctypes.c_void_p(15 << 20), lo=8, rows=5, rowlen=12, n=67, chunks=3), 'lazy'),
             (dict(flags=ctypes.c_void_p(15 << 20), lo=-4, rows=5, rowlen=12), 'lazy')]


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from mmvid_amd import _lib
    for kw, word in REFUSALS:
        with pytest.raises(_lib.MMVIDError, match=word):
            made_up_call(**kw)
    made_up_call(n=0, chunks=3)  # nothing to look at: no launch, no error
    made_up_call(n=0, chunks=3, step=0, step_dev=ctypes.c_void_p(16 << 20))


# ----------------------------------------------------------------------------------------------------------- the CPU trainer
def test_trainer_validates_the_telemetry_keywords(model):
    for bad in (True, False, 0, -1, 1.0, 2.5, '1', [1], np.bool_(True)):
        with pytest.raises(ValueError, match='telemetry_every'):
            trainer(model, telemetry_every=bad)
    for bad in (True, 0, -2, 64.0, None, '64'):
        with pytest.raises(ValueError, match='telemetry_slots'):
            trainer(model, telemetry_every=1, telemetry_slots=bad)
        with pytest.raises(ValueError, match='telemetry_slots'):
            trainer(model, telemetry_slots=bad)
    with pytest.raises(ValueError, match='host trainer'):  # it has no optimiser kernel
        trainer(model, telemetry_every=1)
    with pytest.raises(ValueError, match='host trainer'):
        trainer(model, telemetry_every=50, telemetry_slots=3)
    off = trainer(model)
    assert off.telemetry_every is None and off.telemetry_slots == 64 and off._tel is None


def test_readers_refuse_on_a_trainer_without_telemetry(model):
    tr = trainer(model)
    with pytest.raises(RuntimeError, match='telemetry'):
        tr.telemetry()
    with pytest.raises(RuntimeError, match='telemetry'):
        tr.telemetry(last=1, by='layer')
    with pytest.raises(RuntimeError, match='telemetry'):
        tr.first_nonfinite()
    for kw in (dict(by='block'), dict(last=0), dict(last=True), dict(last=1.5)):
        with pytest.raises(ValueError):
            tr.telemetry(**kw)


def test_state_dict_of_a_cpu_trainer_has_the_keys_it_had(model):
    sd = trainer(model).state_dict()
    assert sorted(map(str, sd)) == ['frontend', 'names', 'param_groups', 'state']
    assert all(sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in sd['state'].values())
    assert sorted(sd['param_groups'][0]) == ['amsgrad', 'betas', 'eps', 'lr', 'params', 'weight_decay']
    trainer(model).load_state_dict(sd)


def test_layer_grouping_on_the_tiny_models_names(model):
    from mmvid_amd.engine import telemetry_group
    names = trainer(model).names
    groups = [telemetry_group(n) for n in names]
    assert sorted(set(groups)) == ['heads', 'layer.0', 'layer.1', 'tables']
    assert groups.count('layer.0') == groups.count('layer.1') == 12 and groups.count('heads') == 12 and groups.count("tables") == 8
    for n, g in zip(names, groups):
        if n.startswith('transformer.transformer.resblocks.'):
            assert g == 'layer.' + n.split('.')[3]
        else:
            assert g == ('heads' if n.startswith('to_logits') else 'tables')
    assert telemetry_group('transformer.transformer.resblocks.11.mlp.c_fc.weight') == 'layer.11'
    assert telemetry_group('text_emb.weight') == 'tables' and telemetry_group('to_logits_rel.1.bias') == 'heads'
