"""Weight EMA without a GPU: the host replica of the rule (tests/ema_ref.py), the header entry and its binding, and the FlatTrainer
side on a CPU trainer -- arguments, the checkpoint entry, priming, and the `ema_weights()` scope (which needs no kernel on a CPU
trainer: it has no bf16 shadows)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ema_ref as R
from test_host_logic import tiny_bert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(x):
    return np.asarray(x, F32).view(np.int32)


def weights(n, seed, lo=-40, hi=40):
    """Signed fp32 values with magnitudes 2^lo .. 2^hi."""
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)


# ------------------------------------------------------------------------------------------------------------- the replica
def test_replica_is_the_identity_where_ema_equals_p():
    """ema == p gives p, bit for bit -- the lazy-row skip rests on it.  The one value whose BITS change is -0: IEEE gives
    -0 - -0 = +0 and a (+0) + (-0) = +0, on the host and on the device alike; the number is the same."""
    p = np.concatenate([weights(4096, 0), F32([0.0, 2.0**100, -2.0**-100, 1.0, -1.0])])
    assert not (bits(p) == bits(F32(-0.0))).any()
    for decay, warmup, t in ((0.0, False, 1), (0.9, False, 3), (0.9999, True, 2), (0.9999, True, 100000)):
        R.assert_condition(p, p, decay, warmup, t)
        assert np.array_equal(bits(R.update(p, p, decay, warmup, t)), bits(p))
        z = R.update(F32([-0.0]), F32([-0.0]), decay, warmup, t)
        assert z[0] == 0 and bits(z)[0] == 0


def test_replica_with_decay_zero_is_fmaf_of_one():
    from frontend_ref import fma32
    p, e = weights(4096, 1, -20, 20), weights(4096, 2, -20, 20)
    R.assert_condition(e, p, 0.0, False, 1)
    assert R.alpha_at(0.0, False, 1) == F32(1)
    want = fma32(np.ones(p.shape, F32), (p - e).astype(F32), e)
    assert np.array_equal(bits(R.update(e, p, 0.0, False, 1)), bits(want))
    close = p * F32(1.25)  # p / 2 <= e <= 2 p: the subtraction is exact (Sterbenz) and fmaf(1, p - e, e) is p
    assert np.array_equal(bits(R.update(close, p, 0.0, False, 1)), bits(p))


def test_replica_is_within_one_and_a_half_ulp_of_fp64():
    """The error is a/2 ulp(p - ema) from the subtraction plus 1/2 ulp of the result from the fmaf.  For weights of one sign with
    |p| >= |ema|, or with decay >= 0.5, a |p - ema| <= |result|, so a ulp(p - ema) <= 2 ulp(result): 1.5 ulp in all.  (Outside that
    domain the subtraction can lose what the result consists of: decay 0, ema = 1, p = 2^-30 gives 0.)"""
    rng = np.random.default_rng(3)
    n = 1 << 16
    sign = rng.choice([-1.0, 1.0], n)
    big, small = np.exp2(rng.uniform(-30, 30, n)), np.exp2(rng.uniform(-30, 30, n))
    big, small = np.maximum(big, small), np.minimum(big, small)
    near = big * rng.uniform(0.5, 1.0, n)  # the everyday case: the average is close to the weight
    worst = 0.0
    for decay, warmup, t in ((0.0, False, 1), (0.3, False, 1), (0.9, False, 5), (0.9999, False, 7), (0.9999, True, 1), (0.9999, True, 500)):
        cases = [(small, big), (near, big)]  # (ema, p): the weight is the larger one
        if float(R.decay_at(decay, warmup, t)) >= 0.5:
            cases += [(big, small), (big, near)]
        for e, p in cases:
            e, p = (sign * e).astype(F32), (sign * p).astype(F32)
            R.assert_condition(e, p, decay, warmup, t)
            got, ref = R.update(e, p, decay, warmup, t).astype(np.float64), R.update64(e, p, decay, warmup, t)
            worst = max(worst, float((np.abs(got - ref) / R.ulp32(ref)).max()))
    print(f'worst |replica - fp64| = {worst:.3f} ulp')
    assert worst <= 1.5


def test_warmup_reaches_the_decay_where_fp32_says_so():
    """decay = 0.9999.  In real numbers (1 + t) / (10 + t) reaches 0.9999 at t = 89,990.  The rule is fp32: the decay is the fp32
    nearest 0.9999 (a little below it) and the quotient near 1 moves in steps of 2^-24, so the switch comes 42 steps sooner -- the
    quotient is below the decay up to t = 89,948 and at or above it from t = 89,949 on.  Asserted over every t, not assumed; the
    steps 89,990 and 89,991 the GPU tests also use lie behind the switch."""
    dec = F32(0.9999)
    ts = np.arange(1, 200001)
    ramp = (F32(1) + ts.astype(F32)) / (F32(10) + ts.astype(F32))
    assert ramp.dtype == F32
    below = ramp < dec
    assert below[:89948].all() and not below[89948:].any()  # (index t - 1)
    assert R.decay_at(0.9999, True, 89948) < dec and R.decay_at(0.9999, True, 89949) == dec
    assert R.decay_at(0.9999, True, 89990) == R.decay_at(0.9999, True, 89991) == dec == R.decay_at(0.9999, True, 10**6)
    assert float(dec) < 0.9999 and (1 + 89990) / (10 + 89990) == 0.9999
    assert R.decay_at(0.9999, True, 1) == F32(2) / F32(11) and R.decay_at(0.9999, False, 1) == dec
    assert R.alpha_at(0.9999, True, 89991) == F32(1) - dec
    for t in (1, 2, 9, 89948, 89949, 89990, 89991, 100000):  # one element of the replica against the scalar statement
        e, p = F32(0.75), F32(-1.5)
        a = F32(1) - min(dec, (F32(1) + F32(t)) / (F32(10) + F32(t)))
        want = F32(np.float64(a) * np.float64(F32(p - e)) + np.float64(e))  # (exact in fp64 for these values: one rounding)
        assert R.update(F32([e]), F32([p]), 0.9999, True, t)[0] == want


def test_condition_helper_refuses_what_the_replica_does_not_cover():
    ok = F32([1.0, -2.0, 0.0])
    R.assert_condition(ok, ok * F32(3), 0.9, False, 1)
    R.assert_condition(F32([1.0]), F32([1.0 + 2.0**-23]), 0.9, False, 1)  # (a difference of one ulp is far above 2^-100)
    R.assert_condition(F32([0.0]), F32([2.0**-99]), 0.0, False, 1)
    for e, p in ((F32([2.0**101]), F32([1.0])), (F32([1.0]), F32([-2.0**101])), (F32([1.0]), F32([np.inf])), (F32([np.nan]), F32([1.0])),
                 (F32([0.0]), F32([2.0**-101])), (F32([2.0**-101]), F32([2.0**-101]))):
        with pytest.raises(AssertionError):
            R.assert_condition(e, p, 0.9, False, 1)
    with pytest.raises(AssertionError):  # |p - ema| is large enough, a |p - ema| is not
        R.assert_condition(F32([0.0]), F32([2.0**-99]), 0.9999, False, 1)


def test_replica_rows_leave_unflagged_rows_alone():
    e, p = weights(8 + 5 * 12 + 7, 4, -4, 4), weights(8 + 5 * 12 + 7, 5, -4, 4)
    flags = [1, 0, 0, 1, 0]
    got, full = R.update_rows(e, p, 0.9, False, 1, flags, 8, 5, 12), R.update(e, p, 0.9, False, 1)
    for r, f in enumerate(flags):
        sl = slice(8 + 12 * r, 8 + 12 * (r + 1))
        assert np.array_equal(bits(got[sl]), bits(full[sl] if f else e[sl]))
    assert np.array_equal(bits(got[:8]), bits(full[:8])) and np.array_equal(bits(got[68:]), bits(full[68:]))
    assert not np.array_equal(bits(full), bits(e))


# ------------------------------------------------------------------------------------------------- the header and the binding
def test_ema_entry_point_is_declared_bound_and_built():
    from mmvid_amd import _cdecl, _lib, build
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)
    assert 'mmvid_ema_update' in hdr.functions and hdr.functions['mmvid_ema_update'][0] is ctypes.c_int
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    assert len(re.findall(r'\bmmvid_ema_update\s*\(', bare)) == 1
    P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.EXT_SIGNATURES['mmvid_ema_update'] == hdr.functions['mmvid_ema_update'][1] == [P, P, I64, F, I, I, P, P, I64, I64, I, P]
    assert 'mmvid_ema_update' not in _lib.SIGNATURES and 'mmvid_ema_update' not in _lib.OTHER
    assert 'ema' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'ema.hip'))
    lib = _lib.load()
    assert 'mmvid_ema_update' not in lib._mmvid_missing
    fn = lib.mmvid_ema_update
    assert list(fn.argtypes) == list(_lib.EXT_SIGNATURES['mmvid_ema_update']) and fn.restype is ctypes.c_int
    assert _lib.ABI_VERSION == _lib.HEADER.constants['MMVID_ABI_VERSION'] == lib.mmvid_abi_version()


def test_ema_entry_point_refuses_bad_arguments_without_a_launch():
    """Every refusal of the header through _lib.call.  The pointers are never dereferenced: the checks come first."""
    from mmvid_amd import _lib
    V = ctypes.c_void_p
    ok = dict(ema=V(1 << 20), p=V(2 << 20), n=1000, decay=0.9, warmup=0, step=1, sdev=None, flags=None, lo=0, rows=0, rowlen=0)

    def call(**kw):
        a = dict(ok, **kw)
        _lib.call('mmvid_ema_update', a['ema'], a['p'], a['n'], a['decay'], a['warmup'], a['step'], a['sdev'], a['flags'], a['lo'], a['rows'],
                  a['rowlen'], None)

    fl = V(3 << 20)
    for kw, word in ((dict(ema=None), 'NULL'), (dict(p=None), 'NULL'), (dict(p=V(1 << 20)), 'overlap'), (dict(p=V((1 << 20) + 3984)), 'overlap'),
                     (dict(ema=V((2 << 20) + 3984)), 'overlap'), (dict(n=-1), 'negative'), (dict(ema=V((1 << 20) + 4)), 'aligned'),
                     (dict(p=V((2 << 20) + 8)), 'aligned'), (dict(decay=1.0), 'decay'), (dict(decay=-0.1), 'decay'),
                     (dict(decay=float('nan')), 'decay'), (dict(decay=float('inf')), 'decay'), (dict(step=0), 'step'), (dict(step=-3), 'step'),
                     (dict(flags=fl, lo=8, rows=5, rowlen=12, n=67), 'lazy'), (dict(flags=fl, lo=6, rows=5, rowlen=12), 'lazy'),
                     (dict(flags=fl, lo=8, rows=5, rowlen=10), 'lazy'), (dict(flags=fl, lo=-4, rows=5, rowlen=12), 'lazy'),
                     (dict(flags=fl, lo=8, rows=-1, rowlen=12), 'lazy'), (dict(flags=fl, lo=8, rows=5, rowlen=0), 'lazy'),
                     (dict(flags=fl, lo=1004, rows=0, rowlen=4), 'lazy'), (dict(flags=fl, lo=0, rows=1 << 62, rowlen=4), 'lazy')):
        with pytest.raises(_lib.MMVIDError, match=word):
            call(**kw)
    call(n=0)  # nothing to update: no launch, no error
    call(n=0, flags=fl, lo=0, rows=0, rowlen=4)
    call(n=0, step=0, sdev=V(4 << 20))  # (a device step count stands in for the host's)


# ------------------------------------------------------------------------------------------------------------ the CPU trainer
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return tiny_bert()


def trainer(model, **kw):
    from mmvid_amd.engine import FlatTrainer, backward_order
    return FlatTrainer(model, order=backward_order, **kw)


def inside(t, flat):
    lo = flat.data_ptr()
    return lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= lo + 4 * flat.numel()


def test_trainer_rejects_bad_ema_arguments(model):
    for bad in (1.0, -0.01, 1.5, float('nan'), float('inf'), True, False, '0.9', [0.9]):
        with pytest.raises(ValueError, match='ema_decay'):
            trainer(model, ema_decay=bad)
    with pytest.raises(ValueError, match='ema_warmup'):
        trainer(model, ema_warmup=True)
    off = trainer(model)
    assert off.E is None and off.ES is None and off.ema_decay is None
    for fn in (off.ema_state_dict, off.ema_reset, lambda: off.ema_decay_at(1), lambda: off.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match='no EMA'):
            fn()


def test_state_dict_is_unchanged_with_ema_off_and_round_trips_with_it_on(model):
    off = trainer(model)
    sd_off = off.state_dict()
    assert sorted(map(str, sd_off)) == ['frontend', 'names', 'param_groups', 'state']
    on = trainer(model, ema_decay=0.99, ema_warmup=True)
    assert on.E.dtype == torch.float32 and on.E.shape == on.P.shape and on.E.device == on.P.device and on.ES is None
    sd = on.state_dict()
    assert sorted(map(str, sd)) == ['ema', 'frontend', 'names', 'param_groups', 'state']
    assert {k: sd[k] for k in ('names', 'param_groups', 'frontend')} == {k: sd_off[k] for k in ('names', 'param_groups', 'frontend')}
    assert sorted(sd['state']) == sorted(sd_off['state']) and all(sorted(sd['state'][i]) == sorted(sd_off['state'][i]) for i in sd['state'])
    ema = sd['ema']
    assert sorted(ema) == ['decay', 'warmup', 'weights'] and ema['decay'] == 0.99 and ema['warmup'] is True
    assert list(ema['weights']) == on.names
    for (n, w), p in zip(ema['weights'].items(), on.params):
        assert w.shape == p.shape and torch.equal(w, p.detach()) and not inside(w, on.E)  # primed by this read; clones
    # the entry comes back: E as saved (not P), primed
    saved = {n: w + 1.0 for n, w in ema['weights'].items()}
    on2 = trainer(model, ema_decay=0.99, ema_warmup=True)
    assert not on2._ema_primed
    on2.load_state_dict(dict(sd, ema=dict(ema, weights=saved)))
    assert on2._ema_primed
    for (n, w), (n2, w2), p in zip(on2.ema_state_dict().items(), saved.items(), on2.params):
        assert n == n2 and torch.equal(w, w2) and not torch.equal(w, p.detach())
    # a state without the entry un-primes: the next reader sees the weights as they stand then
    on2.load_state_dict(sd_off)
    assert not on2._ema_primed
    with torch.no_grad():
        on2.params[0].add_(0.5)
    assert torch.equal(on2.ema_state_dict()[on2.names[0]], on2.params[0].detach())
    # an entry given to a trainer without EMA is ignored
    off.load_state_dict(sd)
    assert off.E is None and sorted(map(str, off.state_dict())) == ['frontend', 'names', 'param_groups', 'state']
    # wrong names and shapes are refused, before anything is written
    before = on2.E.clone()
    name = on2.names[3]
    renamed = {('other.' + n if n == name else n): w for n, w in saved.items()}
    with pytest.raises(ValueError, match='different set of parameters'):
        on2.load_state_dict(dict(sd, ema=dict(ema, weights=renamed)))
    with pytest.raises(ValueError, match='different set of parameters'):
        on2.load_state_dict(dict(sd, ema=dict(ema, weights={n: w for n, w in saved.items() if n != name})))
    reshaped = dict(saved)
    reshaped[name] = saved[name].reshape(-1)[:-1].clone() if saved[name].numel() > 1 else saved[name].reshape(1, 1)
    with pytest.raises(ValueError, match='shape'):
        on2.load_state_dict(dict(sd, ema=dict(ema, weights=reshaped)))
    assert torch.equal(on2.E, before)


def test_priming_happens_at_the_first_reader_and_reset_undoes_it(model):
    tr = trainer(model, ema_decay=0.9)
    assert not tr._ema_primed and not tr.E.any()
    with torch.no_grad():
        tr.params[1].mul_(1.5)  # weights rewritten after construction, before the first reader (a load, a broadcast)
    first = tr.ema_state_dict()
    assert tr._ema_primed and torch.equal(tr.E, tr.P) and tr.E.data_ptr() != tr.P.data_ptr()
    with torch.no_grad():
        tr.params[1].mul_(2.0)
    assert torch.equal(tr.ema_state_dict()[tr.names[1]], first[tr.names[1]])  # primed once: later writes to P are not copied
    tr.ema_reset()
    assert not tr._ema_primed
    assert torch.equal(tr.ema_state_dict()[tr.names[1]], tr.params[1].detach()) and tr._ema_primed
    assert tr.ema_decay_at(1) == float(R.decay_at(0.9, False, 1)) == float(F32(0.9))
    warm = trainer(model, ema_decay=0.9999, ema_warmup=True)
    for t in (1, 2, 9, 89948, 89949, 89990, 89991, 100000):
        assert warm.ema_decay_at(t) == float(R.decay_at(0.9999, True, t))
    assert warm.ema_decay_at(89948) < warm.ema_decay_at(89949) == warm.ema_decay_at(89991) == float(F32(0.9999))


def test_scope_points_the_model_at_the_average_and_back(model):
    tr = trainer(model, ema_decay=0.9)
    with torch.no_grad():
        tr.ema_state_dict()
        tr.E.add_(1.0)  # an average that differs from the weights
    frozen = [(p, p.data_ptr()) for p in model.parameters() if not p.requires_grad]
    assert frozen
    x = tr.params[2].detach().clone()
    with tr.ema_weights() as got:
        assert got is tr
        for p, o in zip(tr.params, tr.offsets):
            assert p.data_ptr() == tr.E.data_ptr() + 4 * o and p.grad.data_ptr() == tr.G.data_ptr() + 4 * o
            assert inside(p, tr.E) and inside(p.grad, tr.G) and p.requires_grad
        assert torch.equal(tr.params[2].detach(), x + 1.0)
        assert all(p.data_ptr() == at for p, at in frozen)
        for refused in (tr.step, tr.zero_grad, tr.refresh_shadows, tr.ema_reset, lambda: tr.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match='ema_weights'):
                refused()
        assert tr._ema_scope
    assert not tr._ema_scope
    for p, o in zip(tr.params, tr.offsets):
        assert p.data_ptr() == tr.P.data_ptr() + 4 * o and inside(p, tr.P) and p.grad.data_ptr() == tr.G.data_ptr() + 4 * o
    tr._check_bindings()
    assert torch.equal(tr.params[2].detach(), x) and all(p.data_ptr() == at for p, at in frozen)
    tr.zero_grad()  # allowed again
    with pytest.raises(ZeroDivisionError):  # an exception inside the scope still restores the weights
        with tr.ema_weights():
            1 / 0
    assert not tr._ema_scope
    tr._check_bindings()
    assert tr.ES is None  # a CPU trainer has no shadows
