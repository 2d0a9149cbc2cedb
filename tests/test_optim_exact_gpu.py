"""The optimiser kernels through the C ABI on guarded buffers (tests/guarded.py), against the fp64 references and derived bounds of
tests/optim_ref.py: csrc/optim.hip (mmvid_adam_step / _lr / _rows, mmvid_grad_sqnorm / _det / _rows, mmvid_cast_f32_to_bf16) and the two
scalar kernels of csrc/frontend.hip (mmvid_lr_schedule, mmvid_counter_add).

Every Adam case is ONE step from a live state (optim_ref.adam_inputs: values over 11 to 22 decades, zeros mixed in), so no error
accumulates and any step number can be tested.  No tolerance here is a literal: p, m and v are held to the running bound of
optim_ref.adam_ref (with the 1-ulp host powf / 16-ulp OpenCL device pow allowance for the bias corrections), the norm to
K 2^-24 sum g^2 with K counted from the reduction tree, the learning rate to the running bound with the 3-ulp OpenCL log allowance;
the shadow, the bf16 cast, the lazy-row skip and the counter are compared bit for bit.  tests/test_optim_ref_host.py shows on the CPU
that a correct fp32 evaluation meets these bounds and that the plausible wrong ones miss them by more than 10 x.

The large size, 2 * 2,097,152 + 3 * 1024 + 7, is the smallest that takes every path of the grid-stride loop (grid_for caps the grid at
2048 blocks of 1024 elements): three sweeps, the last one ragged, and a 3-element scalar tail.

Poison and sentinels are ordinary data; the argument-contract tests launch nothing."""
import ctypes
import functools
import gc
import itertools

import pytest
import torch

import optim_ref as R
from guarded import Guarded, bits
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen

pytestmark = pytest.mark.gpu
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
SWEEP = R.GRID_CAP * R.BLOCK_ELEMS                 # 2,097,152 elements per trip of the grid-stride loop
LARGE = 2 * SWEEP + 3 * 1024 + 7
SIZES = (1, 3, 4, 5, 1023, 1025, 100003)
NAN = float('nan')
DEV = 'cuda'


@functools.lru_cache(maxsize=4)
def inputs(n):
    return R.adam_inputs(n)


@functools.lru_cache(maxsize=3)
def _shared_ref(n, key):
    """The reference of a case that several tests use (the large size, the lazy-row cases): computed once, never modified."""
    case = R.adam_case(**dict(key))
    p, g, m, v = inputs(n)
    return R.adam_ref(p, g, m, v, pow_ulps=case['pow_ulps'], **case['hyper'])


def shared_ref(n, t, combo):
    return _shared_ref(n, tuple(sorted(dict(combo, t=t, shadow=True).items())))


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    """The large cases hold a few hundred MB of references on the host and leave as much in torch's caching allocator on the device:
    both are given back when the module is done, so that the tests that follow in the same process start from what they always had."""
    yield
    inputs.cache_clear()
    _shared_ref.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def scalar(x):
    return Guarded(torch.tensor([x], dtype=F32))


def launch_adam(entry, x, case, *, shadow_base=None, lazy=None):
    """One call of an Adam entry point on guarded copies of x = (p, g, m, v).  With step_dev / lr_dev the host arguments `step` / `lr`
    hold OTHER values: the device scalars must win.  lazy = (flags uint8, lo, rows, rowlen).  Checks every guard, that g, the flags
    and every scalar input came back unchanged, and that the shadow is bf16-RNE of the p the kernel stored (outside `keep`, the
    elements the lazy rows skip).  -> dict of the windows."""
    p, g, m, v = x
    n, h = p.numel(), case['hyper']
    P, M, Vv, G = Guarded(base=p), Guarded(base=m), Guarded(base=v), Guarded(g)
    S = None
    if case['shadow']:  # (partial: a stored bf16 may legitimately equal the sentinel's bits; every element is compared below)
        S = Guarded(base=shadow_base) if shadow_base is not None else Guarded(role='out', shape=(n,), dtype=BF, partial=True)
    sq = scalar(h['sqnorm']) if h['sqnorm'] is not None else None
    sd = scalar(float(h['t'])) if case['step_dev'] else None
    ld = scalar(h['lr']) if case['lr_dev'] else None
    step = h['t'] + 3 if case['step_dev'] else h['t']
    lr = R.f32(7e-3) if case['lr_dev'] else h['lr']
    tail = (h['beta1'], h['beta2'], h['eps'], h['weight_decay'], int(step), _ptr(sd), h['max_norm'], _ptr(sq), h['grad_scale'])
    F = None
    if entry == 'mmvid_adam_step':
        assert ld is None and lazy is None
        args = (lr,) + tail
    elif entry == 'mmvid_adam_step_lr':
        assert lazy is None
        args = (lr, _ptr(ld)) + tail
    else:
        fl, lo, rows, rowlen = lazy if lazy is not None else (None, 0, 0, 0)
        F = Guarded(fl) if fl is not None else None
        args = (lr, _ptr(ld)) + tail + (_ptr(F), int(lo), int(rows), int(rowlen))
    _call(entry, P.ptr, G.ptr, M.ptr, Vv.ptr, _ptr(S), n, *args)
    what = f'{entry} n={n} {case["tag"]}'
    for name, gd in (('g', G), ('sqnorm', sq), ('step_dev', sd), ('lr_dev', ld), ('row_flags', F)):
        if gd is not None:
            gd.check(f'{what}: {name}')
    res = {'p': P.check(f'{what}: p'), 'm': M.check(f'{what}: m'), 'v': Vv.check(f'{what}: v')}
    if S is not None:
        res['shadow'] = S.check(f'{what}: shadow')
    return res


def assert_shadow(res, what, keep=None, kept_bits=None):
    """The shadow is bf16 round-to-nearest-even of the p the kernel itself stored, bit for bit; at `keep` it holds `kept_bits`."""
    want = R.bf16_rne_bits(R.u32_bits(res['p']))
    if keep is not None:
        want = torch.where(keep, kept_bits, want)
    got = R.u16_bits(res['shadow'])
    bad = (got != want).nonzero().view(-1)
    assert bad.numel() == 0, f'{what}: shadow differs from bf16-RNE of the stored p at {bad.numel()} elements, first ' \
                             f'{[(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:4]]}'


def assert_adam(res, ref, what, worst, only=None):
    """p, m, v within the running bound (elements `only`); `worst` collects the largest fraction of the bound per tensor."""
    for k in 'pmv':
        got, r = res[k], ref[k]
        if only is not None:
            got, r = got[only], R.V(r.x[only], r.e[only])
        fr = R.worst_fraction(got, r)
        worst[k] = max(worst.get(k, 0.0), fr)
        assert fr <= 1.0, f'{what}: {k} is {fr:.3f} x its bound away from fp64 (inf: a non-finite value)'


def same_bits(got, want, what):
    """Identical bit patterns (-0 is not +0, a NaN equals only the same NaN)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (bits(got) != bits(want)).nonzero()
    assert bad.shape[0] == 0, f'{what}: {bad.shape[0]} of {got.numel()} elements differ; first (index, got, want): ' \
                              f'{[(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:5]]}'


def assert_same(a, b, what):
    for k in a:
        same_bits(a[k], b[k], f'{what}: {k}')


def report(what, worst):
    print(f'FRACTION-OF-BOUND {what}: ' + ' '.join(f'{k} {x:.3f}' for k, x in worst.items()))


# ============================================================================================= mmvid_adam_step_rows: the cross product
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('step_dev', [False, True], ids=['step', 'step_dev'])
@pytest.mark.parametrize('t', R.STEPS)
def test_adam_cross_product(t, step_dev, wd):
    """n = 100003: lr | lr_dev x sqnorm NULL | not clipping | clipping | max_norm 0 x grad_scale 1 | 1/8 x shadow | NULL.  Two identical
    calls give identical bits."""
    n = 100003
    x = inputs(n)
    worst = {}
    for lr_dev, clip, gs in itertools.product((False, True), R.CLIPS, (1.0, 0.125)):
        case = R.adam_case(t, step_dev, lr_dev, wd, clip, gs)
        ref = R.adam_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper'])
        for shadow in (True, False):
            case = R.adam_case(t, step_dev, lr_dev, wd, clip, gs, shadow)
            res = launch_adam('mmvid_adam_step_rows', x, case)
            assert_adam(res, ref, case['tag'], worst)
            if shadow:
                assert_shadow(res, case['tag'])
                if step_dev and not lr_dev and clip == 'none' and gs == 1.0:
                    # a MEASUREMENT, not a check: p against the bound a 1-ulp powf would get (the assertion above allows 16)
                    one = R.adam_ref(*x, pow_ulps=R.POW_ULPS_HOST, **case['hyper'])
                    print(f'MEASURED t={t} wd={wd}: device powf, p is {R.worst_fraction(res["p"], one["p"]):.3f} x the bound with a '
                          f'1-ulp allowance for the power')
                assert_same(res, launch_adam('mmvid_adam_step_rows', x, case), case['tag'] + ': second call')
    report(f'adam n={n} t={t} {"step_dev" if step_dev else "host-step"} wd={wd}', worst)


# ================================================================================================ the other sizes, and the forwarding
@pytest.mark.parametrize('which', ['representative', 'production'])
@pytest.mark.parametrize('n', SIZES[:-1] + (LARGE,))
def test_adam_sizes(n, which):
    """Vector body only, scalar tail only, both, more than one block, and the large size: three sweeps of the grid-stride loop."""
    combo = R.PRODUCTION if which == 'production' else R.REPRESENTATIVE
    t = 1000 if which == 'production' else 3
    case = R.adam_case(t=t, **combo)
    x = inputs(n)
    ref = shared_ref(n, t, combo) if n == LARGE else R.adam_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper'])
    worst = {}
    res = launch_adam('mmvid_adam_step_rows', x, case)
    assert_adam(res, ref, case['tag'], worst)
    if case['shadow']:
        assert_shadow(res, case['tag'])
    assert_same(res, launch_adam('mmvid_adam_step_rows', x, case), case['tag'] + ': second call')
    report(f'adam n={n} {which}', worst)


@pytest.mark.parametrize('entry', ['mmvid_adam_step', 'mmvid_adam_step_lr'])
def test_adam_forwarding(entry):
    """mmvid_adam_step and mmvid_adam_step_lr hand every argument on in the right place: all of them away from their defaults."""
    n = 1025
    case = R.adam_case(t=10, step_dev=True, lr_dev=entry == 'mmvid_adam_step_lr', wd=0.01, clip='clip', gs=0.125, shadow=True)
    x = inputs(n)
    ref = R.adam_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper'])
    worst = {}
    res = launch_adam(entry, x, case)
    assert_adam(res, ref, f'{entry} {case["tag"]}', worst)
    assert_shadow(res, entry)
    case = R.adam_case(t=2, step_dev=False, lr_dev=False, wd=0.0, clip='max_norm_0', gs=1.0, shadow=False)
    res = launch_adam(entry, x, case)
    assert_adam(res, R.adam_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper']), f'{entry} {case["tag"]}', worst)
    report(f'{entry} n={n}', worst)


# ========================================================================================================================== lazy rows
def lazy_flags(gen, rows, ends, special=()):
    """Mixed flags; the first and the last row (and the rows `special`) hold `ends`, their neighbours the opposite."""
    fl = torch.randint(0, 2, (rows,), generator=gen).to(U8)
    for r in (0, rows - 1) + tuple(special):
        for d in (-1, 1):
            if 0 <= r + d < rows:
                fl[r + d] = 1 - ends
    for r in (0, rows - 1) + tuple(special):
        fl[r] = ends
    assert 0 < int(fl.sum()) < rows
    return fl


def skipped(n, fl, lo, rowlen):
    s = torch.zeros(n, dtype=torch.bool)
    s[lo:lo + fl.numel() * rowlen] = (fl == 0).repeat_interleave(rowlen)
    return s


def sqnorm_rows(g, base, lazy):
    """mmvid_grad_sqnorm_rows on guarded buffers -> out_accum (fp32 [1])."""
    fl, lo, rows, rowlen = lazy if lazy is not None else (None, 0, 0, 0)
    G, acc, part = Guarded(g), Guarded(base=torch.tensor([base], dtype=F32)), Guarded(role='out', shape=(2048,), dtype=F32, partial=True)
    F = Guarded(fl) if fl is not None else None
    _call('mmvid_grad_sqnorm_rows', G.ptr, g.numel(), part.ptr, acc.ptr, _ptr(F), int(lo), int(rows), int(rowlen))
    G.check('sqnorm_rows: g'), part.check('sqnorm_rows: partials')
    if F is not None:
        F.check('sqnorm_rows: row_flags')
    return acc.check('sqnorm_rows: out_accum')


def run_lazy(n, lo, rows, rowlen, ends, special=()):
    """(1) skipped rows hold quiet NaN in g, m and v: their p, m, v and shadow keep their bits, the norm is finite and within its bound,
    everything else is within the Adam bound.  (2) skipped rows hold g = m = v = 0 and the shadow is in step with p: the flagged call
    equals the unflagged call bit for bit -- p, m, v, shadow and the norm."""
    t, what = 1000, f'lazy n={n} lo={lo} rows={rows} rowlen={rowlen} ends={ends}'
    case = R.adam_case(t=t, **R.PRODUCTION)
    fl = lazy_flags(_gen('lazy', n, lo, rows, rowlen, ends), rows, ends, special)
    lazy = (fl, lo, rows, rowlen)
    skip = skipped(n, fl, lo, rowlen)
    p, g, m, v = inputs(n)
    ref = shared_ref(n, t, R.PRODUCTION)        # elementwise: valid wherever the inputs are the originals
    # (1) NaN in the skipped rows
    gn, mn, vn = (torch.where(skip, torch.full_like(a, NAN), a) for a in (g, m, v))
    base = (p * 3).bfloat16()                    # NOT the cast of p: a skipped row that were rewritten would show
    res = launch_adam('mmvid_adam_step_rows', (p, gn, mn, vn), case, shadow_base=base, lazy=lazy)
    worst = {}
    assert_adam(res, ref, what, worst, only=~skip)
    assert_shadow(res, what, keep=skip, kept_bits=R.u16_bits(base))
    for k, orig in (('p', p), ('m', mn), ('v', vn)):
        same_bits(res[k][skip], orig[skip], f'{what}: {k} of the skipped rows')
    got = sqnorm_rows(gn, 3.5, lazy)
    want, bound, K = R.sqnorm_ref(g, 3.5, atomic=False, skip=skip)
    fr = abs(got.double().item() - want) / bound if bool(torch.isfinite(got).all()) else float('inf')
    worst['norm'] = fr
    assert fr <= 1.0, f'{what}: the norm is {fr:.3f} x its K 2^-24 sum g^2 bound away (K = {K}; inf: NaN of a skipped row was read)'
    report(what, worst)
    # (2) zeros in the skipped rows: skipping is exact
    zero = torch.zeros(())
    gz, mz, vz = (torch.where(skip, zero, a) for a in (g, m, v))
    base = p.bfloat16()
    a = launch_adam('mmvid_adam_step_rows', (p, gz, mz, vz), case, shadow_base=base, lazy=lazy)
    b = launch_adam('mmvid_adam_step_rows', (p, gz, mz, vz), case, shadow_base=base, lazy=None)
    assert_same(a, b, what + ': flagged against unflagged')
    same_bits(sqnorm_rows(gz, 3.5, lazy), sqnorm_rows(gz, 3.5, None), what + ': norm, flagged against unflagged')


LAZY_ROWS = {4: 1500, 8: 700, 768: 40}


@pytest.mark.parametrize('ends', [0, 1])
@pytest.mark.parametrize('place', ['start', 'mid', 'end'])
@pytest.mark.parametrize('rowlen', [4, 8, 768])
def test_lazy_rows(rowlen, place, ends):
    """The table at element 0, at a start that is no multiple of 1024 (2052), and ending exactly at n."""
    rows = LAZY_ROWS[rowlen]
    n = 100000 if place == 'end' else 100003
    lo = {'start': 0, 'mid': 2052, 'end': n - rows * rowlen}[place]
    assert lo % 4 == 0 and (place != 'mid' or lo % 1024) and lo + rows * rowlen <= n
    run_lazy(n, lo, rows, rowlen, ends)


@pytest.mark.parametrize('ends', [0, 1])
@pytest.mark.parametrize('rowlen', [8, 768])
def test_lazy_rows_straddle_two_sweeps(rowlen, ends):
    """A row across element 2,097,152: the same row is met in the first and in the second trip of the grid-stride loop.  (A row of 4
    cannot straddle: rows start at multiples of 4.)"""
    rows, r = (100, 50) if rowlen == 8 else (12, 5)
    lo = SWEEP - r * rowlen - (4 if rowlen == 8 else 100)
    assert lo % 4 == 0 and lo + r * rowlen < SWEEP < lo + (r + 1) * rowlen
    run_lazy(LARGE, lo, rows, rowlen, ends, special=(r,))


# ============================================================================================================== the three sums of squares
@pytest.mark.parametrize('n', SIZES + (LARGE,))
def test_grad_sqnorm_forms(n):
    g = inputs(n)[1]
    base = 3.5
    worst = {}
    # atomic form: free order
    want, bound, K = R.sqnorm_ref(g, base, atomic=True)
    for _ in range(2):
        G, acc = Guarded(g), Guarded(base=torch.tensor([base]))
        _call('mmvid_grad_sqnorm', G.ptr, n, acc.ptr)
        G.check('g')
        got = acc.check('out_accum')
        assert bool(torch.isfinite(got).all())
        worst['atomic'] = max(worst.get('atomic', 0.0), abs(got.double().item() - want) / bound)
    assert worst['atomic'] <= 1.0, f'grad_sqnorm n={n}: {worst["atomic"]:.3f} x the K 2^-24 sum g^2 bound (K = {K})'
    # fixed-order forms: padded (guards of NaN around g, sentinels around partials and out_accum) twice, and dense
    want, bound, K = R.sqnorm_ref(g, base, atomic=False)
    res = {}
    for form in ('det', 'rows'):
        for rep in range(2):
            G, acc = Guarded(g), Guarded(base=torch.tensor([base]))
            part = Guarded(role='out', shape=(2048,), dtype=F32, partial=True)
            if form == 'det':
                _call('mmvid_grad_sqnorm_det', G.ptr, n, part.ptr, acc.ptr)
            else:
                _call('mmvid_grad_sqnorm_rows', G.ptr, n, part.ptr, acc.ptr, None, 0, 0, 0)
            G.check('g'), part.check('partials')
            res[form, rep] = acc.check('out_accum')
        gd, accd, partd = g.to(DEV), torch.tensor([base], device=DEV), torch.zeros(2048, device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        if form == 'det':
            _call('mmvid_grad_sqnorm_det', p(gd), n, p(partd), p(accd))
        else:
            _call('mmvid_grad_sqnorm_rows', p(gd), n, p(partd), p(accd), None, 0, 0, 0)
        res[form, 'dense'] = accd.cpu()
        assert bool(torch.isfinite(res[form, 0]).all())
        worst[form] = abs(res[form, 0].double().item() - want) / bound
        assert worst[form] <= 1.0, f'grad_sqnorm_{form} n={n}: {worst[form]:.3f} x the K 2^-24 sum g^2 bound (K = {K})'
        same_bits(res[form, 1], res[form, 0], f'grad_sqnorm_{form} n={n}: second call')
        same_bits(res[form, 'dense'], res[form, 0], f'grad_sqnorm_{form} n={n}: dense against padded')
    same_bits(res['rows', 0], res['det', 0], f'n={n}: grad_sqnorm_rows without a table against grad_sqnorm_det')
    report(f'sqnorm n={n} (K = {K})', worst)


def test_grad_sqnorm_of_nothing_leaves_the_accumulator():
    g = inputs(4)[1]
    for form in ('atomic', 'det', 'rows'):
        G, acc = Guarded(g), Guarded(base=torch.tensor([3.5]))
        part = Guarded(role='out', shape=(2048,), dtype=F32, partial=True)
        if form == 'atomic':
            _call('mmvid_grad_sqnorm', G.ptr, 0, acc.ptr)
        elif form == 'det':
            _call('mmvid_grad_sqnorm_det', G.ptr, 0, part.ptr, acc.ptr)
        else:
            _call('mmvid_grad_sqnorm_rows', G.ptr, 0, part.ptr, acc.ptr, None, 0, 0, 0)
        G.check('g')
        assert bool((bits(part.check('partials')) == part.fill_bits).all()), f'{form}: partials written for n = 0'
        same_bits(acc.check('out_accum'), torch.tensor([3.5]), f'{form}: out_accum changed for n = 0')


# ============================================================================================================================ bf16 cast
@pytest.mark.parametrize('tile,drop', [(1, 0), (1, 1), (1, 2), (1, 3), (7, 0), (7, 3)])
def test_cast_f32_to_bf16_every_high_half(tile, drop):
    """All 65,536 high halves x the low halves {0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF}; n - 1 .. n - 3 for the scalar tails; tiled 7 x
    (2,293,760 elements) for the second sweep.  Bit for bit, except that NaN is compared as a class: it must stay NaN (never
    infinity, never a number); its payload is not a value, and torch's own conversions do not agree on one either."""
    xb = R.cast_patterns().repeat(tile)
    xb = xb[:xb.numel() - drop]
    n = xb.numel()
    assert tile == 1 or n > SWEEP
    x = R.f32_from_bits(xb)
    X, Y = Guarded(x), Guarded(role='out', shape=(n,), dtype=BF, partial=True)   # (partial: 0xC6A5, the sentinel, is one of the results)
    _call('mmvid_cast_f32_to_bf16', X.ptr, Y.ptr, n)
    X.check('x')
    got, want = R.u16_bits(Y.check('y')), R.bf16_rne_bits(xb)
    nan = torch.isnan(x)
    bad = ((got != want) & ~nan).nonzero().view(-1)
    assert bad.numel() == 0, f'{bad.numel()} values differ from RNE, first (fp32 bits, got, want) ' \
                             f'{[(hex(int(xb[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]}'
    lost = (nan & ~R.bf16_is_nan(got)).nonzero().view(-1)
    assert lost.numel() == 0, f'{lost.numel()} NaN did not stay NaN, first {[(hex(int(xb[i])), hex(int(got[i]))) for i in lost[:5]]}'
    print(f'cast n={n}: {int(nan.sum())} NaN inputs, {int((got[nan] == R.BF16_NAN).sum())} of them come out as 0x7FC0')


# ===================================================================================================================== lr schedule, counter
def lr_launch(it, kind, lo, hi, warmup, every):
    sd, out = scalar(float(it)), Guarded(role='out', shape=(1,), dtype=F32)
    assert int(sd.window().item()) == it
    _call('mmvid_lr_schedule', sd.ptr, kind, lo, hi, warmup, every, out.ptr)
    sd.check('step_dev')
    return out.check('lr_out').double().item()


@pytest.mark.parametrize('every', [0, 1, 3])
@pytest.mark.parametrize('lo,hi', [(1e-6, 1e-4), (0.0, 1e-3)])
def test_lr_schedule(lo, hi, every):
    """Against the fp64 closed form and engine.WarmupLR.lr_at, within the running bound (one rounding per fp32 operation, 3 ulp for
    each of the two logf: the OpenCL C requirement).  lr_max exactly while no scheduler step has happened (ns == 0) and for kind 0.
    From the first scheduler step on the rate never falls (before it the optimiser runs at its construction rate lr_max, by the
    reference's design, so the drop from ns = 0 to ns = 1 is the schedule and not an error)."""
    from mmvid_amd.engine import WarmupLR
    lo, hi = R.f32(lo), R.f32(hi)
    e = max(every, 1)
    worst = 0.0
    for warmup in (0, 1, 2, 8, 5000):
        sched = WarmupLR(lo, hi, warmup, every)
        its = sorted({i for i in (0, 1, 2, every - 1, every, every + 1, every * (warmup - 1), every * warmup, every * (warmup + 1),
                                  2**24 - 1) if i >= 0})
        prev = None
        for it in its:
            got = lr_launch(it, 1, lo, hi, warmup, every)
            want, bound = R.lr_ref(it, 1, lo, hi, warmup, every)
            what = f'lr_schedule it={it} warmup={warmup} every={every} ({lo}, {hi})'
            assert lr_launch(it, 0, lo, hi, warmup, every) == hi, what + ': kind 0'
            if it // e == 0:
                assert got == hi, what + f': {got} before the first scheduler step'
                continue
            fr = abs(got - want) / bound
            worst = max(worst, fr)
            assert fr <= 1.0, what + f': {got} is {fr:.3f} x the bound away from {want}'
            assert abs(got - sched.lr_at(it)) <= bound + 2.0**-50 * hi, what + ': differs from WarmupLR.lr_at'
            assert prev is None or got >= prev, what + f': the rate fell from {prev} to {got}'
            prev = got
    report(f'lr every={every} ({lo}, {hi})', {'lr': worst})


def test_counter_add_is_exact_on_small_integers():
    """Up to 2^24 - 1.  (The counter is an fp32 scalar: at 2^24 = 16,777,216 steps c + 1 rounds back to c and the count stops; the bias
    corrections are 1 long before, and a finished warm-up does not depend on the count.)"""
    for c0, v in itertools.product((0.0, 1.0, 5.0, 4095.0, 2.0**24 - 4), (1.0, 2.0, 3.0)):
        C = Guarded(base=torch.tensor([c0]))
        _call('mmvid_counter_add', C.ptr, v)
        assert C.check('counter').item() == c0 + v, (c0, v)      # check(): the neighbours on both sides keep their sentinel


# ================================================================================================================== argument contract
def test_adam_argument_contract():
    """Each of these must raise before anything is launched, and leave every buffer as it was."""
    from mmvid_amd._lib import MMVIDError
    n = 1024
    p, g, m, v = inputs(n)
    fl = torch.ones(8, dtype=U8)
    buf = dict(p=Guarded(base=p), g=Guarded(g), m=Guarded(base=m), v=Guarded(base=v),
               shadow=Guarded(base=p.bfloat16()), flags=Guarded(fl), step_dev=scalar(3.0))

    def off(name, nbytes):
        return ctypes.c_void_p(buf[name].ptr.value + nbytes)

    def call(ptrs=None, count=n, wd=0.0, step=3, step_dev=None, flags=None, lo=0, rows=0, rowlen=0):
        q = {k: buf[k].ptr for k in ('p', 'g', 'm', 'v', 'shadow')}
        q.update(ptrs or {})
        _call('mmvid_adam_step_rows', q['p'], q['g'], q['m'], q['v'], q['shadow'], count, R.LR_HOST, None, R.BETA1, R.BETA2, R.EPS,
              R.f32(wd), step, step_dev, R.f32(0.0), None, R.f32(1.0), flags, lo, rows, rowlen)

    F = buf['flags'].ptr
    bad = {f'{k} 4 bytes off a 16-byte boundary': dict(ptrs={k: off(k, 4)}, count=n - 1) for k in 'pgmv'}
    bad.update({f'{k} 8 bytes off a 16-byte boundary': dict(ptrs={k: off(k, 8)}, count=n - 2) for k in 'pgmv'})
    bad.update({
        'shadow 2 bytes off an 8-byte boundary': dict(ptrs={'shadow': off('shadow', 2)}, count=n - 1),
        'shadow 4 bytes off an 8-byte boundary': dict(ptrs={'shadow': off('shadow', 4)}, count=n - 2),
        'lazy rows with weight decay': dict(wd=0.01, flags=F, lo=0, rows=8, rowlen=8),
        'table_lo % 4 != 0': dict(flags=F, lo=6, rows=8, rowlen=8),
        'rowlen % 4 != 0': dict(flags=F, lo=0, rows=8, rowlen=6),
        'a table reaching past n': dict(flags=F, lo=n - 60, rows=8, rowlen=8),
        'a table whose rows * rowlen wraps to a size that fits': dict(flags=F, lo=n - 64, rows=(1 << 62) + 8, rowlen=8),
        'step < 1 without step_dev': dict(step=0),
    })
    for what, kw in bad.items():
        with pytest.raises(MMVIDError):
            call(**kw)
            pytest.fail(f'{what}: accepted')
        orig = dict(p=p, g=g, m=m, v=v, shadow=p.bfloat16(), flags=fl, step_dev=torch.tensor([3.0]))
        for k, gd in buf.items():
            same_bits(gd.check(f'{what}: {k}'), orig[k], f'{what}: {k} was modified')
    # the same arguments without the defect are accepted (the refusals above are not refusals of everything)
    call(step=0, step_dev=buf['step_dev'].ptr, flags=F, lo=n - 64, rows=8, rowlen=8)
