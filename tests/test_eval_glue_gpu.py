"""The evaluation encoders' fp32 glue kernels against the fp64 references of tests/eval_glue_ref.py, on guarded buffers
(tests/guarded.py): mmvid_clip_image_assemble, mmvid_clip_pool_project, mmvid_clip_pair_scores, mmvid_i3d_head, mmvid_i3d_fold.
These produce the numbers of the CLIP-score and FVD / PRD tables and were seen before only through whole encoders, at bars sized for
bf16 towers.

Every operand lies between 64-KiB guards: inputs are surrounded by NaN (out-of-range ids for `rows`), outputs are pre-filled with a
sentinel, and check() demands that nothing outside a window changed, that inputs came back as they were and that every output
element was stored.  Inputs are the seeded CPU generators of eval_glue_ref.py, whose hard rows (large mean, variance near and below
eps, sequences whose norms differ by 3) tests/test_eval_glue_ref_host.py verifies without a GPU.

BARS.  Neither is a number picked in advance.
* worst case (pool-project, pair scores, head; hard assert in every case): |got - fp64| <= K 2^-23 sum |terms|, K = the fp32
  operations feeding one output + 1: D + 1 (pair scores), 98 + C + To + 2 (head), and for pool-project
  (E + 1) 2^-23 |h| @ |proj| + e_LN sum_k |proj[k][d]| with e_LN the tight bar of that pooled row's LayerNorm.  l2norm = 1 is held to
  the same call's l2norm = 0 window normalised in fp64, within (D + 4) 2^-23 |value|.
* tight (the assemble, and every case with at least 256 outputs): the case's worst |got - fp64| is at most 8 x the worst
  |fp32 evaluation of the reference formula on the CPU - fp64| of the same case, floored at 2^-22 max |fp64|.  The kernels differ
  from that evaluation in summation order, rsqrtf and fma contraction only; a wrong eps, divisor or row moves the hard rows by 50 x
  the bar or more.  The assemble has this bar alone: a K 2^-23 bound of a LayerNorm is orders of magnitude wider than it.
* the fold equals its replica bit for bit.

MEASURED (MI355X; `-s` prints both ratios per case).  Worst over the cases of each entry point:
  image_assemble   tight 0.50 to 1.00 x the fp32 evaluation (the hard rows set the case's worst error in both: 8e-6 to 3e-5)
  pool_project     worst case 0.0005 to 0.0082 of the bound; l2norm 0.0048 of (D + 4) 2^-23 |value|;
                   tight 0.75 to 1.42 x (l2norm = 0), 0.82 to 3.88 x (l2norm = 1; 3.88 at 5 x 257 x 1024 x 768, 2.27 next: the
                   kernel's projection is one fmaf chain over k ascending, E = 1,024 long, the CPU's matmul sums in blocks)
  pair_scores      worst case 0.142 of the bound at D = 1 (K = 2), at most 0.0055 elsewhere
  i3d_head         worst case at most 0.0016 of the bound; tight 0.53 and 0.67 x
  i3d_fold         equal
No bar had to be widened.  The nine one-line mutants (eps x 0.1, variance / (E - 1), class row + pos[1], rows ignored, the
block's first sequence's norm for all, txt[f % B], / 100, / To, front pad 3) each fail at least two of these tests.

Nothing here provokes a fault: poison and sentinels are ordinary data, the refused calls return before any launch."""
import pytest
import torch

import eval_glue_ref as ref
from eval_glue_ref import EPS, U23
from guarded import SENTINEL_BITS, Guarded, bits, report_mismatch
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen

pytestmark = pytest.mark.gpu
BF, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32


def out(shape, dtype=F32, partial=False):
    return Guarded(role='out', shape=shape, dtype=dtype, partial=partial)


def checked(operands, what):
    """check() of every operand -> the windows."""
    return {k: g.check(f'{what} {k}') for k, g in operands.items() if g is not None}


def worst_case(got, ref64, bound, what):
    assert bool(torch.isfinite(got).all()), f'{what}: non-finite output (a poisoned element was consumed)'
    r = float(((got.double() - ref64).abs() / bound).max())
    print(f'{what}: worst |err| / worst-case bound = {r:.4f}')
    assert r <= 1.0, f'{what}: {r:.2f} x the worst-case bound away from fp64'


def tight(got, ref64, y32, what):
    assert bool(torch.isfinite(got).all()), f'{what}: non-finite output (a poisoned element was consumed)'
    bar = ref.tight_bar(y32, ref64)
    err = float((got.double() - ref64).abs().max())
    r = err / (bar / ref.TIGHT_MARGIN)
    print(f'{what}: worst |err| = {err:.3e} = {r:.3f} x the fp32 evaluation\'s (floored), bar {ref.TIGHT_MARGIN:.0f} x')
    assert err <= bar, f'{what}: {r:.2f} x the error of an fp32 evaluation of the reference formula (bar {ref.TIGHT_MARGIN:.0f} x)'


# ========================================================================================================= mmvid_clip_image_assemble
@pytest.mark.parametrize('N,T,E', ref.ASSEMBLE_CASES)
def test_clip_image_assemble(N, T, E):
    c = ref.assemble_inputs(N, T, E)
    o = dict(feat=Guarded(c['feat']), cls=Guarded(c['cls']), pos=Guarded(c['pos']), w=Guarded(c['w']), b=Guarded(c['b']),
             out=out((N * T, E)))
    _call('mmvid_clip_image_assemble', o['feat'].ptr, o['cls'].ptr, o['pos'].ptr, o['w'].ptr, o['b'].ptr, EPS, N, T, E, o['out'].ptr)
    what = f'clip_image_assemble {N}x{T}x{E}'
    got = checked(o, what)['out']
    args = (c['feat'], c['cls'], c['pos'], c['w'], c['b'], EPS, N, T)
    y64, y32 = ref.image_assemble(*args), ref.fp32_eval('image_assemble', *args)
    tight(got, y64, y32, what)
    for name, rows in c['hard'].items():  # (covered by the line above: the hard rows by themselves, for the print)
        print(f'{what}: {name} rows worst |err| = {float((got[rows].double() - y64[rows]).abs().max()):.3e}')


# =========================================================================================================== mmvid_clip_pool_project
@pytest.mark.parametrize('B,L,E,D,given', ref.POOL_CASES)
def test_clip_pool_project(B, L, E, D, given):
    c = ref.pool_inputs(B, L, E, D, given)
    what = f'clip_pool_project {B}x{L}x{E}x{D} rows {"given" if given else "NULL"}'
    got = {}
    for l2norm in (0, 1):
        o = dict(x=Guarded(c['x']), rows=Guarded(c['rows']) if given else None, w=Guarded(c['w']), b=Guarded(c['b']),
                 proj=Guarded(c['proj']), out=out((B, D)))
        _call('mmvid_clip_pool_project', o['x'].ptr, B, L, E, _ptr(o['rows']), o['w'].ptr, o['b'].ptr, EPS, o['proj'].ptr, D, l2norm, o['out'].ptr)
        got[l2norm] = checked(o, f'{what} l2norm={l2norm}')['out']
    args = (c['x'], c['rows'], c['w'], c['b'], EPS, c['proj'])
    y64, mag = ref.pool_project(*args, 0)
    bound = ref.pool_bound(c, ref.pool_hidden(*args[:5]), ref.pool_hidden(*args[:5], F32), mag)
    worst_case(got[0], y64, bound, what)
    # l2norm = 1 against this call's own un-normalised window, normalised in fp64
    assert bool(torch.isfinite(got[1]).all()), f'{what}: non-finite output (a poisoned element was consumed)'
    want = got[0].double() / (got[0].double()**2).sum(-1, keepdim=True).sqrt()
    r = float(((got[1].double() - want).abs() / ((D + 4) * U23 * want.abs() + 1e-300)).max())
    print(f'{what} l2norm: worst |err| / ((D + 4) 2^-23 |value|) = {r:.4f}')
    assert r <= 1.0, f'{what}: the normalised output is {r:.2f} x (D + 4) 2^-23 |value| away from its own un-normalised window'
    if B * D >= ref.TIGHT_MIN_OUTPUTS:
        tight(got[0], y64, ref.fp32_eval('pool_project', *args, 0)[0], what)
        tight(got[1], ref.pool_project(*args, 1)[0], ref.fp32_eval('pool_project', *args, 1)[0], what + ' l2norm')


# ============================================================================================================ mmvid_clip_pair_scores
@pytest.mark.parametrize('B,T,D', ref.PAIR_CASES)
def test_clip_pair_scores(B, T, D):
    c = ref.pair_inputs(B, T, D)
    o = dict(img=Guarded(c['img']), txt=Guarded(c['txt']), out=out((B * T,)))
    _call('mmvid_clip_pair_scores', o['img'].ptr, o['txt'].ptr, B, T, D, o['out'].ptr)
    what = f'clip_pair_scores {B}x{T}x{D}'
    got = checked(o, what)['out']
    y64, mag = ref.pair_scores(c['img'], c['txt'], B, T)
    worst_case(got, y64, (D + 1) * U23 * mag, what)
    if B * T >= ref.TIGHT_MIN_OUTPUTS:
        tight(got, y64, ref.fp32_eval('pair_scores', c['img'], c['txt'], B, T)[0], what)


# ==================================================================================================================== mmvid_i3d_head
@pytest.mark.parametrize('N,To,C,ncls', ref.HEAD_CASES)
def test_i3d_head(N, To, C, ncls):
    c = ref.head_inputs(N, To, C, ncls)
    o = dict(x=Guarded(c['x'].reshape(N * To * 49, C)), w=Guarded(c['w']), b=Guarded(c['b']), out=out((N, ncls)))
    _call('mmvid_i3d_head', o['x'].ptr, N, To, C, o['w'].ptr, o['b'].ptr, ncls, o['out'].ptr)
    what = f'i3d_head {N}x{To}x{C}x{ncls}'
    got = checked(o, what)['out']
    y64, mag = ref.i3d_head(c['x'], c['w'], c['b'])
    worst_case(got, y64, ref.head_K(To, C) * U23 * mag, what)
    if N * ncls >= ref.TIGHT_MIN_OUTPUTS:
        tight(got, y64, ref.fp32_eval('i3d_head', c['x'], c['w'], c['b'])[0], what)


# ==================================================================================================================== mmvid_i3d_fold
@pytest.mark.parametrize('n,t', ref.FOLD_CASES)
def test_i3d_fold_bit_for_bit(n, t):
    v, _ = ref.fold_inputs(n, t)
    o = dict(v=Guarded(v.reshape(n * t * 224, 224 * 3)), out=out((n * t * 224 * 112, 24), BF))
    _call('mmvid_i3d_fold', o['v'].ptr, n, t, o['out'].ptr)
    got = checked(o, f'i3d_fold {n}x{t}')['out']
    report_mismatch(got.view(n, t, 224, 112, 24), ref.i3d_fold(v), f'i3d_fold {n}x{t}')


# ========================================================================================================================== refusals
def _r(*shape):
    return torch.randn(*shape, generator=_gen('refusal', *shape))


def _refusals():
    """id -> (entry point, input tensors, output shape, arguments from (input pointers, output pointer)).  Every buffer has the size
    the arguments declare (a width or count of 0 gets one of 256 / 1)."""
    t = {}
    for E in (0, 320, 1280):
        a = max(E, 256)
        t[f'image_assemble E={E}'] = ('mmvid_clip_image_assemble', [_r(2 * 4, a), _r(a), _r(5, a), _r(a), _r(a)], (2 * 5, a),
                                      lambda i, o, E=E: (*i, EPS, 2, 5, E, o))
        t[f'text_embed E={E}'] = ('mmvid_clip_text_embed', [torch.arange(6, dtype=I64).view(2, 3), _r(8, a), _r(3, a)], (2 * 3, a),
                                  lambda i, o, E=E: (i[0], 2, 3, i[1], 8, i[2], E, o, None))
        t[f'pool_project E={E}'] = ('mmvid_clip_pool_project', [_r(2, 3, a), _r(a), _r(a), _r(a, 8)], (2, 8),
                                    lambda i, o, E=E: (i[0], 2, 3, E, None, i[1], i[2], EPS, i[3], 8, 1, o))
    t['image_assemble T=1'] = ('mmvid_clip_image_assemble', [_r(1, 256), _r(256), _r(1, 256), _r(256), _r(256)], (2, 256),
                               lambda i, o: (*i, EPS, 2, 1, 256, o))
    for D in (0, 1025):
        t[f'pool_project D={D}'] = ('mmvid_clip_pool_project', [_r(2, 3, 256), _r(256), _r(256), _r(256, max(D, 1))], (2, max(D, 1)),
                                    lambda i, o, D=D: (i[0], 2, 3, 256, None, i[1], i[2], EPS, i[3], D, 0, o))
    t['pool_project B=0'] = ('mmvid_clip_pool_project', [_r(1, 3, 256), _r(256), _r(256), _r(256, 8)], (1, 8),
                             lambda i, o: (i[0], 0, 3, 256, None, i[1], i[2], EPS, i[3], 8, 0, o))
    t['pair_scores B=0'] = ('mmvid_clip_pair_scores', [_r(3, 64), _r(1, 64)], (3,), lambda i, o: (i[0], i[1], 0, 3, 64, o))
    for To in (1, 10):
        t[f'i3d_head To={To}'] = ('mmvid_i3d_head', [_r(To * 49, 8).to(BF), _r(3, 8), _r(3)], (1, 3),
                                  lambda i, o, To=To: (i[0], 1, To, 8, i[1], i[2], 3, o))
    t['i3d_head C=1032'] = ('mmvid_i3d_head', [_r(2 * 49, 1032).to(BF), _r(3, 1032), _r(3)], (1, 3),
                            lambda i, o: (i[0], 1, 2, 1032, i[1], i[2], 3, o))
    t['i3d_head ncls=0'] = ('mmvid_i3d_head', [_r(2 * 49, 8).to(BF), _r(1, 8), _r(1)], (1, 1), lambda i, o: (i[0], 1, 2, 8, i[1], i[2], 0, o))
    return t


REFUSAL_IDS = ([f'{n} E={E}' for E in (0, 320, 1280) for n in ('image_assemble', 'text_embed', 'pool_project')] +
               ['image_assemble T=1', 'pool_project D=0', 'pool_project D=1025', 'pool_project B=0', 'pair_scores B=0', 'i3d_head To=1',
                'i3d_head To=10', 'i3d_head C=1032', 'i3d_head ncls=0'])


def _untouched(gout, what):
    """Nothing was stored: the whole buffer of the output, window included, still holds the sentinel."""
    window = gout.check(what)
    assert bool((bits(window) == SENTINEL_BITS[gout.dtype]).all()), f'{what}: a refused / empty call stored into its output'


def _raw_call(name, *args):
    from mmvid_amd import _lib, ops
    lib = _lib.load()
    rc = getattr(lib, name)(*args, ops._stream())
    torch.cuda.synchronize()
    return rc, lib.mmvid_last_error().decode()


@pytest.mark.parametrize('case', REFUSAL_IDS)
def test_refusals_return_an_error_and_store_nothing(case):
    table = _refusals()
    assert sorted(table) == sorted(REFUSAL_IDS)
    name, inputs, out_shape, argf = table[case]
    gin = [Guarded(x) for x in inputs]
    gout = out(out_shape, partial=True)
    rc, msg = _raw_call(name, *argf([g.ptr for g in gin], gout.ptr))
    assert rc != 0 and name[len('mmvid_'):] in msg, (rc, msg)
    for k, g in enumerate(gin):
        g.check(f'{case}: input {k}')
    _untouched(gout, case)


def test_empty_batches_return_ok_and_store_nothing():
    gin = [Guarded(x) for x in (_r(2 * 49, 8).to(BF), _r(3, 8), _r(3))]
    gout = out((1, 3), partial=True)
    rc, msg = _raw_call('mmvid_i3d_head', gin[0].ptr, 0, 2, 8, gin[1].ptr, gin[2].ptr, 3, gout.ptr)
    assert rc == 0, msg
    gv, gfold = Guarded(_r(224, 224 * 3)), out((224 * 112, 24), BF, partial=True)
    rc, msg = _raw_call('mmvid_i3d_fold', gv.ptr, 0, 1, gfold.ptr)
    assert rc == 0, msg
    for k, g in enumerate(gin + [gv]):
        g.check(f'empty batch: input {k}')
    _untouched(gout, 'i3d_head N=0')
    _untouched(gfold, 'i3d_fold n=0')
