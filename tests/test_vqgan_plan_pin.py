"""The VQGAN planner's output, pinned: every op list `mmvid_vqgan_run` executes is compared with tests/golden/vqgan_plans.json.

A plan is a flat array of `mmvid_vqgan_op_t` plus an arena size, and the C side does nothing but walk it, so two planners that
produce the same bytes launch the same kernels with the same arguments in the same order.  The fixture holds, per plan, the number
of ops, the arena size, the `patches` list, the kept offsets / shapes and one 8-hex-digit digest per op over every field except
the four pointers, with the rank of first appearance of the op's `w` pointer in their place (the weight-sharing pattern).

The fixture was written by the planner of the commit named in its `meta.commit`, not by the code it now checks.  A pull request
that changes a plan on purpose regenerates it and shows the diff:

    python tests/test_vqgan_plan_pin.py --write [--commit HASH]
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'vqgan_plans.json')

SETTINGS = [(False, 'bf16'), (False, 'f32'), (False, 'bf16_all'), (True, 'bf16'), ('split', 'bf16'), ('mixed', 'bf16')]
SHAPES = [('enc', 4, 128), ('enc', 1, 256), ('enc', 3, 64), ('dec', 2, 8), ('dec', 1, 16), ('dec_z', 2, 8)]
CASES = [(strict, stream) + shape for shape in SHAPES for strict, stream in SETTINGS]
CASES.sort(key=lambda c: c[4] if c[2] == 'enc' else 16 * c[4])  # by model size: each model is built once
FIELDS = ('op', 'mode', 'N', 'H', 'W', 'C', 'Cout', 'flags', 'in0', 'in1', 'in2', 'out_bf16', 'out_f32', 'scratch', 'eps', 'pad')

_model = {}  # one model at a time (construction is most of this module's run time; the cases are ordered by shape)


def case_id(strict, stream, kind, n, size_or_hw):
    return f'{kind}-{n}-{size_or_hw}-strict={strict}-stream={stream}'


def _vae(size):
    if size not in _model:
        from mmvid_amd.vae import VQGanVAE1024
        _model.clear()
        v = VQGanVAE1024(None, size)
        v._ee = lambda: torch.zeros(1024)  # the codebook norms are a device kernel; their values are not part of a plan
        _model[size] = v
    return _model[size]


def planned(strict, stream, kind, n, size_or_hw):
    """One plan through vae._plan(), on the CPU (tests/test_vqgan_oplist_host.py shows the same plans to mmvid_vqgan_check)."""
    v = _vae(size_or_hw if kind == 'enc' else 16 * size_or_hw)
    v.strict, v.stream = strict, stream
    v._prepared().clear()  # (prepared weights and arenas of the case before: nothing of a plan depends on them)
    plan = v._plan(kind, n, size_or_hw)
    v._prepared().clear()
    return plan


def describe(strict, stream, kind, n, size_or_hw):
    """One plan -> (the fixture's record of it, the ops as printable rows)."""
    plan = planned(strict, stream, kind, n, size_or_hw)
    rank, rows = {}, []
    for o in plan.ops:
        w = rank.setdefault(o.w, len(rank)) if o.w else -1
        rows.append(tuple(getattr(o, f) for f in FIELDS) + (w, ))
    rec = {'nops': len(plan.ops), 'arena': plan.arena.numel(), 'patches': [list(p) for p in plan.patches],
           'kept': {k: [off, list(shape)] for k, (off, shape) in plan.kept.items()},
           'ops': [hashlib.sha256(repr(r).encode()).hexdigest()[:8] for r in rows]}
    return rec, rows


@pytest.mark.parametrize('strict,stream,kind,n,size_or_hw', CASES, ids=[case_id(*c) for c in CASES])
def test_vqgan_plan_is_pinned(strict, stream, kind, n, size_or_hw):
    with open(FIXTURE) as f:
        want = json.load(f)['plans'][case_id(strict, stream, kind, n, size_or_hw)]
    got, rows = describe(strict, stream, kind, n, size_or_hw)
    for i, (a, b) in enumerate(zip(got['ops'], want['ops'])):
        assert a == b, f'op {i} differs from the pinned plan: ' + ', '.join(f'{k}={x}' for k, x in zip(FIELDS + ('w_rank', ), rows[i]))
    assert got['nops'] == want['nops'] and got['ops'] == want['ops']
    assert got['arena'] == want['arena']
    assert got['patches'] == want['patches']
    assert got['kept'] == want['kept']


def test_vqgan_plan_fixture_is_complete():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert len(CASES) == 36 and sorted(fx['plans']) == sorted(case_id(*c) for c in CASES)
    assert len(fx['meta']['commit']) == 40 and fx['meta']['fields'] == list(FIELDS) + ['w_rank']


if __name__ == '__main__':
    assert sys.argv[1:2] == ['--write'], __doc__
    commit = sys.argv[3] if sys.argv[2:3] == ['--commit'] else os.popen(f'git -C {ROOT} rev-parse HEAD').read().strip()
    out = {'meta': {'commit': commit, 'fields': list(FIELDS) + ['w_rank'],
                    'digest': 'first 8 hex digits of sha256(repr(tuple of the fields))'},
           'plans': {case_id(*c): describe(*c)[0] for c in CASES}}
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', FIXTURE, 'from', commit)
