"""tests/loss_ref.py checked without a GPU: the bounds the GPU tests (tests/test_loss_exact_gpu.py) hold the loss kernels to can be met by
a correct fp32 implementation, and cannot be met by the plausible wrong ones.

* the formulas evaluated in fp32 on the GPU tests' own cases stay within 1.0 x every bound: summed sequentially and pairwise, with
  every multiply-add rounded twice and with every one rounded once;
* each wrong variant (loss_ref.WRONG_VARIANTS) is more than 10 x outside at least one bound on at least one case; the test prints the
  case and the output that catches it;
* the first two cross-entropy variants and the first two head variants PASS the tolerances the suite had for these kernels (recomputed
  here from their formulas): that is the gap the bounds close;
* the inputs meet the conditions the references need: selected rows exist and are finite, no divisor or logarithm argument is within its
  own error of zero (asserted inside the (x, e) operations), every reference and every bound is finite."""
import functools
import itertools

import pytest
import torch

import loss_ref as L

CE_CASES, HEAD_CASES = L.ce_cases(), L.head_cases()
EVALS = list(itertools.product(L.ORDERS, (False, True)))


@functools.lru_cache(maxsize=None)
def ce_case(key):
    c = L.ce_inputs(*key)
    on, lse, term = L.ce_fwd_ref(c['logits'], c['target'], c['select'])
    c.update(on=on, ref=dict(lse=lse, term=term))
    for gs in c['gscales']:
        c['ref']['d', gs] = L.ce_bwd_ref(c['logits'], c['target'], c['select'], c['lse32'], gs)[1]
    return c


def ce_fractions(c, order='pairwise', fused=False, variant=None):
    """-> {output: fraction of its bound} of one fp32 evaluation of a cross-entropy case."""
    on, ref = c['on'], c['ref']
    lse, term = L.ce_fwd_fp32(c['logits'], c['target'], c['select'], order, fused, variant)
    fr = dict(lse=L.worst_fraction(lse[on], ref['lse']), term=L.worst_fraction(term, ref['term']))
    for gs in c['gscales']:
        d = L.ce_bwd_fp32(c['logits'], c['target'], c['select'], c['lse32'], gs, order, fused, variant)
        fr[f'dlogits gscale={gs:.4g}'] = L.worst_fraction(d[on].float(), ref['d', gs])
    return fr


@functools.lru_cache(maxsize=None)
def head_case(key):
    c = L.head_inputs(*key)
    fwd = L.head_fwd_ref(*L.head_fwd_args(c))
    saved = {k: fwd[k].x.float() for k in ('z', 'mean', 'rstd')}     # the fp32 values a forward hands to the backward
    con = L.head_bwd_ref(*L.head_bwd_args(c, **{k + '32': v for k, v in saved.items()}))
    rows = c['rows']
    based = {k: L.accumulate(c['bases'][k][rows] if k == 'dx' else c['bases'][k], v) for k, v in con.items()}
    c.update(fwd=fwd, saved=saved, con=con, based=based)
    return c


def head_fractions(c, order='pairwise', fused=False, variant=None):
    fr = {}
    got = L.head_fwd_fp32(*L.head_fwd_args(c), order=order, fused=fused, variant=variant)
    for k in ('z', 'mean', 'rstd', 'loss'):
        fr[k] = L.worst_fraction(got[k], c['fwd'][k])
    args = L.head_bwd_args(c, c['saved']['z'], c['saved']['mean'], c['saved']['rstd'])
    bases = dict(c['bases'], dx=c['bases']['dx'][c['rows']])
    for name, b, ref in (('zero bases', None, c['con']), ('randn bases', bases, c['based'])):
        got = L.head_bwd_fp32(*args, bases=b, order=order, fused=fused, variant=variant)
        for k in ('dx', 'dw', 'db', 'dln_w', 'dln_b'):
            fr[f'{k} ({name})'] = L.worst_fraction(got[k], ref[k])
    return fr


def test_depths_are_counted_from_the_kernels():
    assert [L.ce_depth(v) for v in L.CE_SIZES] == [2 + 1 + 6, 2 + 1 + 6, 2 + 1 + 6, 2 + 2 + 6, 2 + 4 + 6, 2 + 4 + 6]
    assert L.HEAD_DEPTH == 2 + 4 + 6
    assert [L.head_rows_depth(r) for r in L.HEAD_ROWS] == [1 + 2, 1 + 2, 1 + 2, 2 + 2, 3 + 2, 64 + 2]


def test_allowances_are_the_documented_ones():
    assert (L.EXP_ULPS_DEVICE, L.LOG1P_ULPS_DEVICE, L.RSQRT_ULPS_DEVICE, L.NATIVE_ULPS) == (3.0, 2.0, 2.0, 4.0)
    assert L.f32(L.LOG2E_F32) == L.LOG2E_F32 and L.f32(L.LN2_F32) == L.LN2_F32
    assert 0 < L.LOG2E_REL < 2.0**-24 and 0 < L.LN2_REL < 2.0**-24
    x = torch.tensor([0.75, 1.0, 1.5, 2.0**-130, 0.0], dtype=torch.float64)
    assert L.ulp32(x).tolist() == [2.0**-24, 2.0**-23, 2.0**-23, 2.0**-149, 2.0**-149]
    assert L.half_spacing_bf16(x[:3]).tolist() == [2.0**-9, 2.0**-8, 2.0**-8]     # at most 2^-8 relative
    # one bf16 rounding of an exact fp32 value stays within its bound, ties included
    v = torch.cat([torch.randn(4096, generator=torch.Generator().manual_seed(3)), torch.tensor([1.00390625, 1.01171875, 0.998046875])])
    assert L.worst_fraction(v.bfloat16().float(), L.vbf16(L.V(v.double()))) <= 1.0


def test_cases_cover_what_the_kernels_branch_on():
    keys = set(CE_CASES)
    assert {k[2] for k in keys if k[0] == 'randn3'} == set(L.CE_SIZES) and {k[1] for k in keys} == set(L.CE_ROWS)
    assert {k[:1] + k[2:3] for k in keys} >= set(itertools.product(L.CE_FAMILIES, (256, 1000)))
    assert {k[3] for k in keys} == {False, True}
    hk = HEAD_CASES
    assert {k[:2] for k in hk} == {(E, R) for E in L.HEAD_SIZES for R in L.HEAD_ROWS if R != 256 or E == 768}
    assert {k[2:] for k in hk} == set(L.HEAD_OPTIONS) == {k[2:] for k in hk if k[:2] == (768, 9)}


def test_inputs_meet_the_conditions_of_the_references():
    for key in CE_CASES:
        c = ce_case(key)
        on, nv = c['on'], c['logits'].shape[1]
        off = torch.ones(c['logits'].shape[0], dtype=torch.bool)
        off[on] = False
        assert len(on) > 0 and bool(torch.isfinite(c['logits'][on]).all()), c['tag']
        assert bool(((c['target'][on] >= 0) & (c['target'][on] < nv)).all())
        edge = [t for t in (0, 3, 4, nv - 1) if t < nv][:len(on)]
        assert c['target'][on][:len(edge)].tolist() == edge, c['tag']
        assert bool(torch.isnan(c['logits'][off]).all()) and bool((c['target'][off] >= nv).all())
        assert (c['select'] is None) == (not bool(off.any()))
        assert sorted(c['gscales'])[:2] == [-2.0, 0.0] and L.f32(0.37) in c['gscales']
        for k, r in c['ref'].items():
            assert bool(torch.isfinite(r.x).all()) and bool(torch.isfinite(r.e).all()) and bool((r.e > 0).all()), (c['tag'], k)
    for key in HEAD_CASES:
        c = head_case(key)
        named = torch.zeros(c['x'].shape[0], dtype=torch.bool)
        named[c['rows']] = True
        assert bool(torch.isfinite(c['x'][named]).all()) and bool(torch.isnan(c['x'][~named]).all())
        assert bool((c['rows'][1:] > c['rows'][:-1]).all()) and set(c['label'].tolist()) <= {0.0, 1.0}
        assert c['rw'] is None or (c['rw'].numel() < 2 or bool((c['rw'] == 0).any()))
        assert c['den'] is None or abs(float(c['den'].double().sum()) - key[3]) < 1e-6
        for group in ('fwd', 'con', 'based'):
            for k, r in c[group].items():
                assert bool(torch.isfinite(r.x).all()) and bool(torch.isfinite(r.e).all()) and bool((r.e > 0).all()), (c['tag'], group, k)
        z = c['fwd']['z'].x
        assert float((z - key[4]).abs().max()) < 12, (c['tag'], z)     # z lies near the shift the case names


def test_shifted_rows_are_bounded_by_the_rounding_of_the_maximum():
    """On rows shifted by +-3e4 the bound of lse is dominated by U |mx|: the last addition, mx + log s."""
    c = ce_case(('shifted', 37, 1000, False))
    share = (L.U * c['ref']['lse'].x.abs() / c['ref']['lse'].e).min().item()
    print(f'{c["tag"]}: U |lse| is at least {share:.3f} of the bound of lse')
    assert share > 0.5


def _collect(worst, fr):
    for k, v in fr.items():
        k = k.split(' gscale')[0]
        worst[k] = max(worst.get(k, 0.0), v)


def test_fp32_cross_entropy_is_within_every_bound():
    worst = {}
    for key in CE_CASES:
        c = ce_case(key)
        for order, fused in EVALS:
            fr = ce_fractions(c, order, fused)
            _collect(worst, fr)
            for k, v in fr.items():
                assert v <= 1.0, f'{c["tag"]} {order} fused={fused}: fp32 {k} is {v:.3f} x its bound'
    print('cross entropy, fp32 worst fraction of the bound: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def test_fp32_heads_are_within_every_bound():
    worst = {}
    for key in HEAD_CASES:
        c = head_case(key)
        for order, fused in EVALS:
            fr = head_fractions(c, order, fused)
            _collect(worst, fr)
            for k, v in fr.items():
                assert v <= 1.0, f'{c["tag"]} {order} fused={fused}: fp32 {k} is {v:.3f} x its bound'
    print('heads, fp32 worst fraction of the bound: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def _applies(variant, key):
    if variant == 'onehot_only':
        return key[0] == 'flat'
    if variant == 'den_without_max1':
        return key[3] == 0.25
    if variant == 'den_const_despite_den_from':
        return key[3] is not None
    if variant == 'bce_without_max_z_0':
        return key[4] == -100.0
    if variant == 'row_weight_ignored_in_bwd':
        return key[2]
    return True


def _caught(variant, cases, case_of, fractions):
    best = (0.0, None, None)
    for key in cases:
        if not _applies(variant, key):
            continue
        c = case_of(key)
        for k, v in fractions(c, variant=variant).items():
            if v > best[0]:
                best = (v, c['tag'], k)
        if best[0] == float('inf'):
            break
    print(f'wrong variant {variant}: {best[0]:.3g} x the bound of {best[2]} on {best[1]}')
    assert best[0] > 10.0, f'wrong variant {variant} is at most {best[0]:.2f} x a bound away on every case'


@pytest.mark.parametrize('variant', L.CE_WRONG)
def test_wrong_cross_entropy_misses_a_bound_by_more_than_10x(variant):
    _caught(variant, CE_CASES, ce_case, ce_fractions)


@pytest.mark.parametrize('variant', L.HEAD_WRONG)
def test_wrong_head_misses_a_bound_by_more_than_10x(variant):
    _caught(variant, HEAD_CASES, head_case, head_fractions)


# ---- the gap: what the tolerances the suite had for these kernels let through ----------------------------------------------------------
@pytest.mark.parametrize('variant,key', [('drop_p_below_1e-3', ('randn3', 37, 1024, False)), ('onehot_only', ('flat', 37, 1000, False))])
def test_old_cross_entropy_tolerances_pass_what_the_bound_refuses(variant, key):
    """tests/test_kernels_gpu.py::test_cross_entropy: max |d - ref| <= 1e-2 max |ref| at gscale = 1 / count;
    tests/test_abi_contract_gpu.py: max |d - ref| < 4e-3 at gscale = 0.37."""
    c = ce_case(key)
    on = c['on']
    count, abi = c['gscales'][0], L.f32(0.37)
    for gs, passes in ((count, lambda err, ref: err <= 1e-2 * ref.abs().max().item()), (abi, lambda err, ref: err < 4e-3)):
        d = L.ce_bwd_fp32(c['logits'], c['target'], c['select'], c['lse32'], gs, variant=variant)[on].double()
        ref = c['ref']['d', gs]
        err, fr = (d - ref.x).abs().max().item(), L.worst_fraction(d, ref)
        print(f'{variant} on {c["tag"]} gscale={gs:.4g}: largest error {err:.3g} passes the old tolerance, and is {fr:.3g} x the bound')
        assert passes(err, ref.x), 'the old tolerance was expected to let this through'
        assert fr > 10.0


@pytest.mark.parametrize('variant', L.HEAD_WRONG[:2])
def test_old_head_checks_pass_what_the_bound_refuses(variant):
    """tests/test_abi_contract_gpu.py: every gradient finite; the model-level comparison: the head's weight gradient within 5e-2 of its
    largest element.  Both LayerNorm-backward terms only reach dx."""
    c = head_case((768, 9, False, None, 0.0, 0.0))
    args = L.head_bwd_args(c, c['saved']['z'], c['saved']['mean'], c['saved']['rstd'])
    bases = dict(c['bases'], dx=c['bases']['dx'][c['rows']])
    got = L.head_bwd_fp32(*args, bases=bases, variant=variant)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    dw = c['based']['dw'].x
    assert float((got['dw'].double() - dw).abs().max()) <= 5e-2 * float(dw.abs().max())
    zero = L.head_bwd_fp32(*args, bases=None, variant=variant)
    fr0, fr1 = L.worst_fraction(zero['dx'], c['con']['dx']), L.worst_fraction(got['dx'], c['based']['dx'])
    rel = float((got['dx'].double() - c['based']['dx'].x).abs().max() / c['based']['dx'].x.abs().max())
    print(f'{variant} on {c["tag"]}: passes the old checks; dx is {fr0:.3g} x its bound into zero bases, {fr1:.3g} x into randn bases '
          f'({rel:.2g} of the largest dx)')
    assert fr0 > 10.0
