"""The loss kernels through the C ABI on guarded buffers (tests/guarded.py), element by element against the fp64 references and derived
bounds of tests/loss_ref.py: mmvid_cross_entropy_fwd / _bwd (csrc/embed.hip) and mmvid_head_bce_fwd / _bwd (csrc/sample.hip).

Every leading dimension is larger than the natural one, inputs are surrounded by quiet NaN / out-of-range ids, outputs by a sentinel.
No tolerance here is a literal: every comparison is worst_fraction(got, reference) <= 1 with the running bound of loss_ref (one
rounding per fp32 operation, the reduction depths counted from the kernels, the documented allowances for the transcendental
functions, half a bf16 spacing for the stored gradient), and each test prints its worst fraction per output.
tests/test_loss_ref_host.py shows on the CPU that a correct fp32 evaluation meets these bounds and that the plausible wrong kernels
miss them by more than 10 x.

Cross entropy: one wave per row, four rows per block, a lane takes float4 c = lane, lane + 64, ...: V = 4 (one float4, 63 idle lanes),
252 (one lane idle), 256 (exactly one sweep), 260 (one lane has a second sweep), 1000 (ragged last sweep), 1024; rows 1, 5, 37 (partial
blocks).  The backward runs on a GIVEN lse (the fp64 value rounded to fp32), at gscale 1 / count, 0.37, -2 and 0.
Heads: one block, wave r % 4 takes row r, a lane holds up to four float4: E = 4 ... 1024, R = 1 ... 256.  The backward runs on the
forward's own saved z, mean, rstd as exact inputs: once into zero bases (the contribution against its own bound: this is what makes
the two LayerNorm-backward terms visible), once into randn bases (fl(base + contribution)).

Poison and sentinels are ordinary data: nothing here provokes a fault."""
import pytest
import torch

import loss_ref as L
from guarded import Guarded, bits
from guarded import call_abi as _call, ptr_of as _ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def out(shape, dtype, ld=None, partial=False):
    return Guarded(role='out', shape=shape, dtype=dtype, ld=ld, partial=partial)


def opt(t):
    return None if t is None else Guarded(t)


def report(what, worst):
    print(f'FRACTION-OF-BOUND {what}: ' + ' '.join(f'{k} {x:.3f}' for k, x in worst.items()))


def hold(got, ref, what, worst, key):
    fr = L.worst_fraction(got, ref)
    worst[key] = max(worst.get(key, 0.0), fr)
    assert fr <= 1.0, f'{what}: {key} is {fr:.3f} x its bound away from fp64 (inf: a non-finite value)'


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = (bits(got) != bits(want)).nonzero()
    assert bad.shape[0] == 0, f'{what}: {bad.shape[0]} of {got.numel()} elements differ; first {[tuple(i.tolist()) for i in bad[:5]]}'


# ========================================================================================================================= cross entropy
@pytest.mark.parametrize('family,rows,nv,with_select', L.ce_cases(), ids=lambda v: str(v))
def test_cross_entropy_element_by_element(family, rows, nv, with_select):
    """lse and the row terms within their bound; every element of dlogits within its bound at every gscale; unselected rows (NaN logits,
    out-of-range targets) exactly 0 in lse and dlogits; guards intact; the out-of-range counter stays at zero."""
    from mmvid_amd import _lib
    c = L.ce_inputs(family, rows, nv, with_select)
    what = 'cross_entropy ' + c['tag']
    logits, target, sel = c['logits'], c['target'], c['select']
    on, lse_ref, term_ref = L.ce_fwd_ref(logits, target, sel)
    off = torch.ones(rows, dtype=torch.bool)
    off[on] = False
    ldl, ldd, loss0 = nv + 4, nv + 12, 0.75
    lg, tg, sg = Guarded(logits, ld=ldl), Guarded(target), opt(sel)
    lse, loss = out((rows,), F32), Guarded(base=torch.tensor([loss0]))
    worst = {}
    _lib.device_faults(reset=True)
    _call('mmvid_cross_entropy_fwd', lg.ptr, ldl, tg.ptr, _ptr(sg), rows, nv, lse.ptr, loss.ptr)
    got_lse, got_loss = lse.check(what + ': lse'), loss.check(what + ': loss_sum')
    hold(got_lse[on], lse_ref, what, worst, 'lse')
    assert bool((got_lse[off] == 0).all()), what + ': lse of an unselected row is not 0'
    # the term is not an output of its own: what the kernel adds is fl(lse - logit[target]) of the lse it stored
    terms = got_lse[on] - logits[on, target[on]]
    hold(terms, term_ref, what, worst, 'term')
    hold(got_loss, L.ce_loss_sum_ref(loss0, terms), what, worst, 'loss_sum')
    if family == 'shifted':
        share = (L.U * lse_ref.x.abs() / lse_ref.e).min().item()
        print(f'{what}: U |mx| is {share:.3f} of the bound of lse')
    lin = Guarded(c['lse32'])
    for gs in c['gscales']:
        gsc, d = Guarded(torch.tensor([gs], dtype=F32)), out((rows, nv), BF, ldd)
        _call('mmvid_cross_entropy_bwd', lg.ptr, ldl, tg.ptr, _ptr(sg), lin.ptr, gsc.ptr, rows, nv, d.ptr, ldd)
        gsc.check(what + ': gscale')
        got = d.check(f'{what} gscale={gs}: dlogits')
        hold(got[on].float(), L.ce_bwd_ref(logits, target, sel, c['lse32'], gs)[1], f'{what} gscale={gs}', worst, 'dlogits')
        assert bool((bits(got[off]) == 0).all()), f'{what} gscale={gs}: the dlogits row of an unselected row is not +0'
    for name, gd in (('logits', lg), ('target', tg), ('select', sg), ('lse_in', lin)):
        if gd is not None:
            gd.check(f'{what}: {name}')
    assert _lib.device_faults(reset=True)[:2] == [0, 0], what + ': a target was counted as out of range'
    report(what, worst)


# ================================================================================================================================= heads
def head_operands(c):
    E = c['x'].shape[1]
    return dict(x=Guarded(c['x'], ld=E + 4), rows=Guarded(c['rows']), ln_w=Guarded(c['ln_w']), ln_b=Guarded(c['ln_b']), w=Guarded(c['w']),
                b=Guarded(c['b']), label=Guarded(c['label']), rw=opt(c['rw']), den=opt(c['den']), gloss=Guarded(c['gloss']))


def head_fwd(o, c, with_label=True):
    R, E = c['rows'].numel(), c['x'].shape[1]
    r = dict(z=out((R,), F32), mean=out((R,), F32), rstd=out((R,), F32), loss=out((1,), F32, partial=not with_label))
    _call('mmvid_head_bce_fwd', o['x'].ptr, E + 4, o['rows'].ptr, R, E, o['ln_w'].ptr, o['ln_b'].ptr, L.HEAD_EPS, o['w'].ptr, o['b'].ptr,
          o['label'].ptr if with_label else None, _ptr(o['rw']), _ptr(o['den']), 0 if c['den'] is None else c['den'].numel(), L.HEAD_DEN_CONST,
          r['z'].ptr, r['mean'].ptr, r['rstd'].ptr, r['loss'].ptr)
    return r


def head_bwd(o, c, saved, bases, accumulators=True):
    """One backward call into guarded copies of `bases` -> dict of the windows (dx whole)."""
    R, E = c['rows'].numel(), c['x'].shape[1]
    lddx = E + 12
    g = dict(dx=Guarded(base=bases['dx'], ld=lddx))
    if accumulators:
        g.update({k: Guarded(base=bases[k]) for k in ('dw', 'db', 'dln_w', 'dln_b')})
    _call('mmvid_head_bce_bwd', o['x'].ptr, E + 4, o['rows'].ptr, R, E, o['ln_w'].ptr, o['ln_b'].ptr, o['w'].ptr, saved['z'].ptr,
          saved['mean'].ptr, saved['rstd'].ptr, o['label'].ptr, _ptr(o['rw']), _ptr(o['den']), 0 if c['den'] is None else c['den'].numel(),
          L.HEAD_DEN_CONST, o['gloss'].ptr, g['dx'].ptr, lddx, _ptr(g.get('dw')), _ptr(g.get('db')), _ptr(g.get('dln_w')), _ptr(g.get('dln_b')))
    return {k: gd.check(f'head_bce_bwd {c["tag"]}: {k}') for k, gd in g.items()}


@pytest.mark.parametrize('E,R,with_rw,den_sum,z_shift,x_mean', L.head_cases(), ids=lambda v: str(v))
def test_head_bce_element_by_element(E, R, with_rw, den_sum, z_shift, x_mean):
    c = L.head_inputs(E, R, with_rw, den_sum, z_shift, x_mean)
    what = 'head_bce ' + c['tag']
    rows = c['rows']
    o = head_operands(c)
    worst = {}
    # forward
    ref = L.head_fwd_ref(*L.head_fwd_args(c))
    f = head_fwd(o, c)
    got = {k: gd.check(f'{what}: {k}') for k, gd in f.items()}
    for k in ('z', 'mean', 'rstd', 'loss'):
        hold(got[k], ref[k], what, worst, k)
    # without labels: the same logits, and loss keeps its sentinel
    f0 = head_fwd(o, c, with_label=False)
    for k in ('z', 'mean', 'rstd'):
        same_bits(f0[k].check(f'{what} label=NULL: {k}'), got[k], f'{what} label=NULL: {k}')
    assert bool((bits(f0['loss'].check(what + ' label=NULL: loss')) == f0['loss'].fill_bits).all()), what + ': loss written without labels'
    # backward, from the forward's own saved outputs as exact inputs
    con = L.head_bwd_ref(*L.head_bwd_args(c, got['z'], got['mean'], got['rstd']))
    other = torch.ones(c['x'].shape[0], dtype=torch.bool)
    other[rows] = False
    zero = {k: torch.zeros_like(v) for k, v in c['bases'].items()}
    last = None
    for name, bases in (('zero bases', zero), ('randn bases', c['bases'])):
        res = head_bwd(o, c, f, bases)
        for k in ('dx', 'dw', 'db', 'dln_w', 'dln_b'):
            g, b = (res[k][rows], bases[k][rows]) if k == 'dx' else (res[k], bases[k])
            hold(g, L.accumulate(b, con[k]), f'{what} into {name}', worst, f'{k} ({name})')
        same_bits(res['dx'][other], bases['dx'][other], f'{what} into {name}: dx rows that `rows` does not name')
        last = res
    # NULL accumulators are accepted, and dx does not depend on them
    same_bits(head_bwd(o, c, f, c['bases'], accumulators=False)['dx'], last['dx'], what + ': dx with dw = db = dln_w = dln_b = NULL')
    for k, gd in list(o.items()) + [(k, f[k]) for k in ('z', 'mean', 'rstd')]:
        if gd is not None:
            gd.check(f'{what}: {k} after the backward')
    report(what, worst)
