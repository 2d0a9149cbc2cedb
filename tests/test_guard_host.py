"""Non-finite guard without a GPU: the three header entries and their binding, their refusals (checked before any launch), the host
replica of mmvid_step_guard (tests/guard_ref.py) against the rule stated value by value, and the FlatTrainer side on a CPU trainer --
the keyword, the refusals of guard_stats(), and the unchanged checkpoint of a trainer without the guard."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guard_ref as R
from test_host_logic import tiny_bert

F32 = np.float32
P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
ENTRIES = {'mmvid_step_guard': [P, F, P, P, P, P],
           'mmvid_adam_step_guarded': [P, P, P, P, P, I64, F, P, F, F, F, F, I, P, F, P, F, P, I64, I64, I, P, P],
           'mmvid_ema_update_guarded': [P, P, I64, F, I, I, P, P, I64, I64, I, P, P]}


def bits(x):
    return np.asarray(x, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------- the header and the binding
def test_guard_entry_points_are_declared_bound_and_built():
    from mmvid_amd import _cdecl, _lib
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)  # the strict reader: anything it does not know raises
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    lib = _lib.load()
    for name, args in ENTRIES.items():
        assert name in hdr.functions and hdr.functions[name][0] is ctypes.c_int, name
        assert len(re.findall(r'\b%s\s*\(' % name, bare)) == 1
        assert _lib.EXT_SIGNATURES[name] == hdr.functions[name][1] == args, name
        assert name not in _lib.SIGNATURES and name not in _lib.OTHER
        assert name not in lib._mmvid_missing
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    # "the argument list of the unguarded entry plus skip_dev before stream"
    assert ENTRIES['mmvid_adam_step_guarded'] == _lib.SIGNATURES['mmvid_adam_step_rows'][:-1] + [P, P]
    assert ENTRIES['mmvid_ema_update_guarded'] == _lib.EXT_SIGNATURES['mmvid_ema_update'][:-1] + [P, P]
    assert _lib.ABI_VERSION == _lib.HEADER.constants['MMVID_ABI_VERSION'] == lib.mmvid_abi_version()


def test_guard_entry_points_refuse_bad_arguments_without_a_launch():
    """Through _lib.call with made-up addresses: the checks come before the launch, so nothing is ever dereferenced."""
    from mmvid_amd import _lib
    V = ctypes.c_void_p
    a, b, c, d, e, f = (V(k << 20) for k in range(1, 7))

    def guard(sq=a, sdev=b, gi=c, gf=d):
        _lib.call('mmvid_step_guard', sq, 1.0, sdev, gi, gf, None)

    for kw in (dict(sq=None), dict(sdev=None), dict(gi=None), dict(gf=None)):
        with pytest.raises(_lib.MMVIDError, match='NULL'):
            guard(**kw)
    for kw in (dict(sq=V((1 << 20) + 2)), dict(sdev=V((2 << 20) + 1)), dict(gi=V((3 << 20) + 2)), dict(gf=V((4 << 20) + 3))):
        with pytest.raises(_lib.MMVIDError, match='aligned'):
            guard(**kw)

    def adam(p=a, g=b, m=c, v=d, n=1000, step=1, wd=0.0, flags=None, lo=0, rows=0, rowlen=0, skip=e):
        _lib.call('mmvid_adam_step_guarded', p, g, m, v, None, n, 1e-3, None, 0.9, 0.999, 1e-8, wd, step, None, 1.0, None, 1.0, flags, lo,
                  rows, rowlen, skip, None)

    for kw, word in ((dict(skip=V((5 << 20) + 2)), 'skip_dev'), (dict(skip=V((5 << 20) + 1)), 'skip_dev'), (dict(p=None), 'bad arguments'),
                     (dict(g=None), 'bad arguments'), (dict(n=-1), 'bad arguments'), (dict(step=0), 'bad arguments'),
                     (dict(p=V((1 << 20) + 4)), 'aligned'), (dict(flags=f, lo=8, rows=5, rowlen=12, wd=0.1), 'weight decay'),
                     (dict(flags=f, lo=8, rows=5, rowlen=10), 'lazy'), (dict(flags=f, lo=8, rows=5, rowlen=12, n=67), 'lazy'),
                     (dict(flags=f, lo=0, rows=1 << 62, rowlen=4), 'lazy')):  # (the last: rows * rowlen wraps to 0)
        with pytest.raises(_lib.MMVIDError, match=word):
            adam(**kw)
    adam(n=0)  # nothing to update: no launch, no error
    adam(n=0, skip=None)

    def ema(ema_=a, p=b, n=1000, decay=0.9, step=1, flags=None, lo=0, rows=0, rowlen=0, skip=e):
        _lib.call('mmvid_ema_update_guarded', ema_, p, n, decay, 0, step, None, flags, lo, rows, rowlen, skip, None)

    for kw, word in ((dict(skip=V((5 << 20) + 2)), 'skip_dev'), (dict(ema_=None), 'NULL'), (dict(p=None), 'NULL'), (dict(p=a), 'overlap'),
                     (dict(n=-1), 'negative'), (dict(ema_=V((1 << 20) + 4)), 'aligned'), (dict(decay=1.0), 'decay'),
                     (dict(decay=float('nan')), 'decay'), (dict(step=0), 'step'), (dict(flags=f, lo=6, rows=5, rowlen=12), 'lazy'),
                     (dict(flags=f, lo=0, rows=1 << 62, rowlen=4), 'lazy')):
        with pytest.raises(_lib.MMVIDError, match=word):
            ema(**kw)
    ema(n=0)
    ema(n=0, skip=None)


# ------------------------------------------------------------------------------------------------------------- the replica
def test_replica_states_the_rule_on_each_kind_of_sum():
    """One call from a state in which every counter already holds something, for sq in {0, 1, 2^127, inf, NaN}."""
    gs = F32(0.25)
    start = (F32(7.0), np.array([1, 3, 2, 10], np.int32), F32([5.0, 6.0]))
    want_norm = {0: F32(0.0), 1: F32(0.25), 2: F32(2.0**63.5) * gs, 3: F32(np.inf), 4: F32(np.nan)}
    assert F32(np.sqrt(F32(2.0**127))) == F32(2.0**63.5)  # (the correctly rounded fp32 root)
    for k, sq in enumerate(R.SQS):
        sdev, gi, gf = R.step_guard(sq, gs, *start)
        assert sdev.dtype == F32 and gi.dtype == np.int32 and gf.dtype == F32
        assert bits(gf[0]) == bits(want_norm[k]) or (k == 4 and np.isnan(gf[0]))
        if k < 3:  # finite: applied
            assert gi.tolist() == [0, 3, 0, 11] and sdev == F32(8.0) and bits(gf[1]) == bits(gf[0])
        else:      # inf, NaN: skipped
            assert gi.tolist() == [1, 4, 3, 11] and sdev == F32(7.0) and gf[1] == F32(6.0)
        assert start[1].tolist() == [1, 3, 2, 10] and start[2].tolist() == [5.0, 6.0]  # the arguments are left alone


def test_replica_chain_counts_runs_and_totals():
    sqs = [F32(4.0), F32(np.nan), F32(np.inf), F32(9.0), F32(np.inf), F32(2.0**127)]
    states = R.chain(sqs, 0.5)
    assert [s[1].tolist() for s in states] == [[0, 0, 0, 1], [1, 1, 1, 2], [1, 2, 2, 3], [0, 2, 0, 4], [1, 3, 1, 5], [0, 3, 0, 6]]
    assert [float(s[0]) for s in states] == [1.0, 1.0, 1.0, 2.0, 2.0, 3.0]
    assert [float(s[2][1]) for s in states] == [1.0, 1.0, 1.0, 1.5, 1.5, float(F32(2.0**63.5) * F32(0.5))]
    assert np.isnan(states[1][2][0]) and np.isinf(states[2][2][0]) and states[3][2][0] == F32(1.5)
    again = R.chain(sqs, 0.5)  # the replica against itself
    for x, y in zip(states, again):
        assert bits(x[0]) == bits(y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(bits(x[2]), bits(y[2]))


# ------------------------------------------------------------------------------------------------------------ the CPU trainer
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return tiny_bert()


def trainer(model, **kw):
    from mmvid_amd.engine import FlatTrainer, backward_order
    return FlatTrainer(model, order=backward_order, **kw)


def test_trainer_validates_skip_nonfinite(model):
    for bad in (1, 0, None, 'yes', 1.0, [True], np.bool_(True)):
        with pytest.raises(ValueError, match='skip_nonfinite'):
            trainer(model, skip_nonfinite=bad)
    assert trainer(model).skip_nonfinite is False and trainer(model, skip_nonfinite=False).guard_i is None
    on = trainer(model, skip_nonfinite=True)  # a host trainer has no optimiser kernel to guard: no buffers
    assert on.skip_nonfinite is True and on.guard_i is None and on.guard_f is None


def test_guard_stats_is_refused_without_the_guard(model):
    for tr in (trainer(model), trainer(model, skip_nonfinite=True)):
        with pytest.raises(RuntimeError, match='guard'):
            tr.guard_stats()


def test_state_dict_without_the_guard_has_the_keys_it_had(model):
    off = trainer(model)
    sd = off.state_dict()
    assert sorted(map(str, sd)) == ['frontend', 'names', 'param_groups', 'state']
    assert all(sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in sd['state'].values())
    assert sorted(map(str, trainer(model, ema_decay=0.9).state_dict())) == ['ema', 'frontend', 'names', 'param_groups', 'state']
    off.load_state_dict(dict(sd, guard={'skipped': 3, 'seen': 9}))  # an entry given to a trainer without the guard is ignored
    assert off.guard_i is None and 'guard' not in off.state_dict()
