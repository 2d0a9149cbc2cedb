"""The contract between the VQGAN planner and its executor: the flag bits and op codes of `mmvid_vqgan_op_t` have one spelling, the
one of include/mmvid_hip.h, and `mmvid_vqgan_check` (csrc/vqgan.hip) accepts every planned list and refuses a record outside the
header's legality table before `mmvid_vqgan_run` enqueues anything.  No GPU: the checker is a host loop, and a refused run launches
nothing."""
import ast
import ctypes

import pytest

from mmvid_amd import _lib, vqgan_plan as P
from test_vqgan_plan_pin import CASES, case_id, planned

CONSTANTS = _lib.HEADER.constants


def check(ops_arr, n=None):
    lib = _lib.load()
    rc = lib.mmvid_vqgan_check(ops_arr, len(ops_arr) if n is None else n)
    return rc, lib.mmvid_last_error().decode()


def test_planner_names_are_the_headers():
    flags = {k[len('MMVID_VQFLAG_'):]: v for k, v in CONSTANTS.items() if k.startswith('MMVID_VQFLAG_')}
    codes = {k[len('MMVID_VQOP_'):]: v for k, v in CONSTANTS.items() if k.startswith('MMVID_VQOP_')}
    assert len(flags) == 11 and sorted(set(flags.values())) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert sorted(codes.values()) == list(range(9))
    assert set(P.FLAG_NAMES) == set(flags) and all(getattr(P, name) == v for name, v in flags.items())
    assert set(P.OP_NAMES.values()) == set(codes)
    for short, name in P.OP_NAMES.items():
        assert getattr(P._Planner, short) == codes[name], short
    assert (P._Planner.STRICT, P._Planner.SPLIT, P._Planner.F16) == (flags['STRICT'], flags['SPLIT'], flags['F16'])
    # the module defines neither family by an integer (nor by range()): every name is bound from the header's table
    names = set(P.FLAG_NAMES) | set(P.OP_NAMES)
    for node in ast.walk(ast.parse(open(P.__file__).read())):
        if isinstance(node, ast.Assign) and names & {n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)}:
            assert not any(isinstance(n, ast.Constant) and isinstance(n.value, int) for n in ast.walk(node.value)), ast.unparse(node)
            assert 'range' not in ast.dump(node.value), ast.unparse(node)


def test_a_name_the_header_lacks_fails_the_planners_import(monkeypatch):
    for gone in ('MMVID_VQFLAG_SPLITK', 'MMVID_VQOP_NHWC2NCHW'):
        monkeypatch.setattr(_lib, 'HEADER', _lib.HEADER._replace(constants={k: v for k, v in CONSTANTS.items() if k != gone}))
        with pytest.raises(KeyError, match=gone):  # the module's own text, run as a second module of the package
            exec(compile(open(P.__file__).read(), P.__file__, 'exec'), {'__name__': 'mmvid_amd._vqgan_plan_again', '__package__': 'mmvid_amd'})


@pytest.mark.parametrize('strict,stream,kind,n,size_or_hw', CASES, ids=[case_id(*c) for c in CASES])
def test_check_accepts_every_pinned_plan(strict, stream, kind, n, size_or_hw):
    plan = planned(strict, stream, kind, n, size_or_hw)
    rc, msg = check(plan.ops)
    assert rc == 0, msg


# ---- one mutation of one record per rule of the header's table: (name, which record, what to do to it, what the message must name)
def _is(op, has=0, lacks=0, **fields):
    return lambda o: (o.op == op and o.flags & has == has and not o.flags & lacks and all(getattr(o, k) == v for k, v in fields.items()))


def _set(**fields):
    return lambda o: [setattr(o, k, v(o) if callable(v) else v) for k, v in fields.items()]


CONV, GN, VQ = P._Planner.OP_CONV, P._Planner.OP_GN, P._Planner.OP_VQ
MUTATIONS = [
    # rule 1: a flag outside the table's cell for the operator and the op
    ('bf16 conv with F16', _is(CONV), _set(flags=lambda o: o.flags | P.F16), ['F16']),
    ('bf16 groupnorm with EMIT_STATS', _is(GN), _set(flags=lambda o: o.flags | P.EMIT_STATS), ['EMIT_STATS']),
    ('pair conv with RES_F32', _is(CONV), _set(flags=P.SPLIT | P.RES_F32), ['RES_F32']),
    ('strict conv with STRIP', _is(CONV), _set(flags=P.STRICT | P.STRIP), ['STRIP']),
    ('strict groupnorm with STATS_GIVEN', _is(GN), _set(flags=P.STRICT | P.STATS_GIVEN), ['STATS_GIVEN']),
    ('another op with a flag', _is(VQ), _set(flags=P.CLAMP01), ['CLAMP01']),
    ('a bit above F16', _is(CONV), _set(flags=lambda o: o.flags | 256), ['without a name']),
    # rule 2: the ops an operator has
    ('no split form', _is(VQ), _set(flags=P.SPLIT), ['SPLIT', 'no split form']),
    ('no strict form', _is(VQ), _set(flags=P.STRICT), ['STRICT', 'no strict form']),
    # rule 3
    ('STRICT with SPLIT', _is(P._Planner.OP_IMG), _set(flags=P.STRICT | P.SPLIT), ['STRICT', 'SPLIT']),
    ('EMIT_STATS with SPLITK', _is(CONV, has=P.EMIT_STATS), _set(flags=lambda o: o.flags | P.SPLITK), ['EMIT_STATS', 'SPLITK']),
    ('EMIT_STATS without scratch', _is(CONV, has=P.EMIT_STATS), _set(scratch=-1), ['EMIT_STATS', 'scratch']),
    ('SPLITK without scratch', _is(CONV, has=P.SPLITK), _set(scratch=-1), ['SPLITK', 'scratch']),
    ('STRIP with CLAMP01', _is(CONV, has=P.STRIP), _set(flags=lambda o: o.flags | P.CLAMP01), ['STRIP', 'CLAMP01']),
    ('STRIP with SPLITK', _is(CONV, has=P.STRIP, lacks=P.EMIT_STATS), _set(flags=lambda o: o.flags | P.SPLITK, scratch=0), ['STRIP', 'SPLITK']),
    ('STRIP with mode 1', _is(CONV, has=P.STRIP), _set(mode=1), ['STRIP', 'mode']),
    ('F16 without STRIP', _is(CONV, lacks=P.STRIP | P.RES_F32), _set(flags=lambda o: o.flags | P.SPLIT | P.F16), ['F16', 'STRIP']),
    ('RES_F32 without a residual', _is(CONV, in1=-1), _set(flags=lambda o: o.flags | P.RES_F32), ['RES_F32', 'in1']),
    ('conv without an output', _is(CONV), _set(out_bf16=-1, out_f32=-1), ['out_bf16', 'out_f32']),
    ('BLOCKS64 without STATS_GIVEN', _is(GN, lacks=P.STATS_GIVEN), _set(flags=lambda o: o.flags | P.BLOCKS64), ['BLOCKS64', 'STATS_GIVEN']),
    ('groupnorm without scratch', _is(GN), _set(scratch=-1), ['GROUPNORM', 'scratch']),
    ('op code 9', _is(VQ), _set(op=9), ['unknown op code']),
    ('op code -1', _is(VQ), _set(op=-1), ['unknown op code']),
]


@pytest.fixture(scope='module')
def small_plan():
    return planned(False, 'bf16', 'enc', 1, 64).ops


@pytest.mark.parametrize('which,mutate,words', [m[1:] for m in MUTATIONS], ids=[m[0] for m in MUTATIONS])
def test_check_refuses_one_bad_record_and_run_enqueues_nothing(small_plan, which, mutate, words):
    n = len(small_plan)
    arr = (_lib.VqganOp * n).from_buffer_copy(small_plan)
    i = next(i for i in range(n) if which(arr[i]))
    mutate(arr[i])
    rc, msg = check(arr)
    assert rc == 1 and f'op {i} ' in msg  # (MMVID_ERR_ARG)
    assert all(w in msg for w in words), msg
    assert check(arr, i) == (0, msg)  # the records in front of it are fine (and a passing check leaves the message alone)
    # the run refuses the same list with the same words, before it touches the arena or the stream: neither exists here
    lib = _lib.load()
    assert lib.mmvid_vqgan_run(arr, n, ctypes.c_void_p(256), None) == rc and lib.mmvid_last_error().decode() == msg
