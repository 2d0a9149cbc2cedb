"""mmvid_adam_step_decoupled (torch.optim.AdamW on the device) on the GPU.

Kernel level, through the C ABI on the guarded, padded, poisoned buffers of tests/guarded.py: p, m and v against the fp64 replica of
tests/adamw_ref.py within its derived bound (tests/test_adamw_ref_host.py shows what that bound tells apart); the relations that hold
byte for byte -- with wd = 0 everything equals mmvid_adam_step_guarded, at any wd the moments equal those of that entry launched with
wd = 0, the shadow is bf16-RNE of the stored p --; the verdict, the lazy rows, every refusal.  One step from a live state per case
(optim_ref.adam_inputs), so any step number can be tested and no error accumulates.

Trainer level: the `bert_tiny` case of tests/test_models_gpu.py against one live torch.optim.AdamW at that test's bars, and on the small
BERT of tests/test_deterministic_step_gpu.py (width 768) in deterministic mode captured against eager, resumed against uninterrupted,
and a NaN loss under the guard against the run that leaves the step out.  NaN in a buffer is ordinary data: no test provokes a fault."""
import copy
import ctypes
import functools
import gc
import itertools

import pytest
import torch

import adamw_ref as A
import mmvid_amd
import optim_ref as R
from guarded import Guarded
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen
from test_deterministic_step_gpu import small_case
from test_guard_gpu import forward_backward, make, one_step
from test_models_gpu import DEV, _bert_case, _with_tokens
from test_optim_exact_gpu import SWEEP, assert_adam, assert_same, assert_shadow, lazy_flags, report, same_bits, scalar, skipped

pytestmark = pytest.mark.gpu
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NAN = float('nan')
LARGE = SWEEP + 5                        # the grid's second sweep: one float4 and a scalar tail of one element
SIZES = (1, 3, 4, 5, 1023, 1025, LARGE)
STEPS = (1, 2, 10, 1000)
NEW, OLD = 'mmvid_adam_step_decoupled', 'mmvid_adam_step_guarded'


@functools.lru_cache(maxsize=4)
def inputs(n):
    return R.adam_inputs(n)


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    yield
    inputs.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def launch(entry, x, case, *, skip=None, lazy=None, shadow_base=None):
    """One call of `entry` (the argument list of mmvid_adam_step_guarded) on guarded copies of x = (p, g, m, v).  With step_dev / lr_dev
    the host arguments hold OTHER values: the device scalars must win.  Every guard, and g, the flags and every scalar input, are
    checked.  -> the windows of p, m, v, shadow."""
    p, g, m, v = x
    n, h = p.numel(), case['hyper']
    P, M, Vv, G = Guarded(base=p), Guarded(base=m), Guarded(base=v), Guarded(g)
    S = None
    if case['shadow']:
        S = Guarded(base=shadow_base) if shadow_base is not None else Guarded(role='out', shape=(n,), dtype=BF, partial=True)
    sq = scalar(h['sqnorm']) if h['sqnorm'] is not None else None
    sd = scalar(float(h['t'])) if case['step_dev'] else None
    ld = scalar(h['lr']) if case['lr_dev'] else None
    SK = None if skip is None else Guarded(torch.tensor([skip], dtype=torch.int32))
    fl, lo, rows, rowlen = lazy if lazy is not None else (None, 0, 0, 0)
    FL = Guarded(fl) if fl is not None else None
    step = h['t'] + 3 if case['step_dev'] else h['t']
    lr = R.f32(7e-3) if case['lr_dev'] else h['lr']
    _call(entry, P.ptr, G.ptr, M.ptr, Vv.ptr, _ptr(S), n, lr, _ptr(ld), h['beta1'], h['beta2'], h['eps'], h['weight_decay'], int(step),
          _ptr(sd), h['max_norm'], _ptr(sq), h['grad_scale'], _ptr(FL), int(lo), int(rows), int(rowlen), _ptr(SK))
    what = f'{entry} n={n} {case["tag"]}'
    for name, gd in (('g', G), ('sqnorm', sq), ('step_dev', sd), ('lr_dev', ld), ('row_flags', FL), ('skip_dev', SK)):
        if gd is not None:
            gd.check(f'{what}: {name}')
    res = {'p': P.check(f'{what}: p'), 'm': M.check(f'{what}: m'), 'v': Vv.check(f'{what}: v')}
    if S is not None:
        res['shadow'] = S.check(f'{what}: shadow')
    return res


def cases_of(n, t):
    """(device scalars?, wd, clip): the cross product below the large size, there one case per weight decay."""
    if n == LARGE:
        return [(False, 0.01, 'none'), (True, 0.1, 'clip'), (True, 0.0, 'loose')]
    return list(itertools.product((False, True), A.WDS, R.CLIPS))


# ============================================================================================================ against the replica
@pytest.mark.parametrize('t', STEPS)
@pytest.mark.parametrize('n', SIZES)
def test_decoupled_against_the_replica(n, t):
    """Step count and learning rate as host arguments (grad_scale 1) and as device scalars (grad_scale 1/8) x wd x the clip forms."""
    x = inputs(n)
    worst = {}
    for dev, wd, clip in cases_of(n, t):
        case = R.adam_case(t, dev, dev, wd, clip, 0.125 if dev else 1.0)
        ref = A.adamw_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper'])
        res = launch(NEW, x, case)
        assert_adam(res, ref, f'n={n} {case["tag"]}', worst)
        assert_shadow(res, f'n={n} {case["tag"]}')
    report(f'adamw n={n} t={t}', worst)


# ======================================================================================================= byte-for-byte relations
@pytest.mark.parametrize('n', SIZES)
def test_decoupled_relations_to_the_guarded_entry(n):
    """wd = 0: p, m, v and the shadow are the bytes of mmvid_adam_step_guarded.  Any wd: m and v are the bytes of that entry launched
    with wd = 0 (the decay never enters the gradient), a second call gives the same bytes, and without a shadow nothing else changes."""
    x = inputs(n)
    for dev, clip in ((False, 'none'), (True, 'clip')):
        plain = R.adam_case(10, dev, dev, 0.0, clip, 0.125 if dev else 1.0)
        old = launch(OLD, x, plain)
        assert_same(launch(NEW, x, plain), old, f'n={n} {plain["tag"]}: decoupled against guarded at wd = 0')
        for wd in A.WDS[1:]:
            case = R.adam_case(10, dev, dev, wd, clip, 0.125 if dev else 1.0)
            new = launch(NEW, x, case)
            for k in 'mv':
                same_bits(new[k], old[k], f'n={n} {case["tag"]}: {k} against the guarded entry at wd = 0')
            assert n < 4 or not torch.equal(new['p'], old['p']), 'the decay did nothing'
            assert_shadow(new, case['tag'])
            assert_same(launch(NEW, x, case), new, f'n={n} {case["tag"]}: second call')
            bare = launch(NEW, x, dict(case, shadow=False))
            assert_same(bare, {k: new[k] for k in 'pmv'}, f'n={n} {case["tag"]}: without a shadow')


@pytest.mark.parametrize('n', (5, 1025, LARGE))
def test_decoupled_with_the_verdict_one_writes_nothing(n):
    """skip_dev = 1 on a gradient of NaN: p, m, v and the shadow keep every byte; skip_dev = 0 and NULL write the same bytes."""
    p, g, m, v = inputs(n)
    case = R.adam_case(10, True, True, 0.1, 'clip', 0.125)
    base = (p * 3).bfloat16()  # NOT the cast of p: a rewritten shadow would show
    res = launch(NEW, (p, torch.full_like(g, NAN), m, v), case, skip=1, shadow_base=base)
    for k, want in (('p', p), ('m', m), ('v', v), ('shadow', base)):
        same_bits(res[k], want, f'n={n} verdict 1: {k}')
    assert_same(launch(NEW, (p, g, m, v), case, skip=0), launch(NEW, (p, g, m, v), case), f'n={n}: verdict 0 against NULL')


@pytest.mark.parametrize('n,lo,rows,rowlen', [(100003, 2052, 40, 768), (100000, 100000 - 1500 * 4, 1500, 4), (SWEEP + 2053, SWEEP - 5 * 8 - 4, 100, 8)],
                         ids=['mid', 'end', 'second_sweep'])
def test_decoupled_lazy_rows_without_decay(n, lo, rows, rowlen):
    """A lazy table with wd = 0: rows whose flag is 0 hold NaN in g, m and v and keep every byte of p, m, v and the shadow; everything
    else is within the bound.  The last table has a row across the first element of the grid's second sweep."""
    case = R.adam_case(1000, True, True, 0.0, 'clip', 0.125)
    fl = lazy_flags(_gen('adamw-lazy', n, lo, rows, rowlen), rows, 0)
    skip = skipped(n, fl, lo, rowlen)
    p, g, m, v = inputs(n)
    gn, mn, vn = (torch.where(skip, torch.full_like(a, NAN), a) for a in (g, m, v))
    base = (p * 3).bfloat16()
    res = launch(NEW, (p, gn, mn, vn), case, shadow_base=base, lazy=(fl, lo, rows, rowlen))
    ref = A.adamw_ref(p, g, m, v, pow_ulps=case['pow_ulps'], **case['hyper'])
    worst = {}
    assert_adam(res, ref, f'lazy n={n}', worst, only=~skip)
    assert_shadow(res, f'lazy n={n}', keep=skip, kept_bits=R.u16_bits(base))
    for k, orig in (('p', p), ('m', mn), ('v', vn)):
        same_bits(res[k][skip], orig[skip], f'lazy n={n}: {k} of the unflagged rows')
    report(f'adamw lazy n={n}', worst)


def test_decoupled_refusals_return_an_error_and_launch_nothing():
    from mmvid_amd._lib import MMVIDError
    n = 1024
    p, g, m, v = inputs(n)
    fl = torch.ones(8, dtype=U8)
    buf = dict(p=Guarded(base=p), g=Guarded(g), m=Guarded(base=m), v=Guarded(base=v), shadow=Guarded(base=p.bfloat16()), flags=Guarded(fl),
               step_dev=scalar(3.0), skip=Guarded(torch.tensor([0], dtype=torch.int32)))

    def off(name, nbytes):
        return ctypes.c_void_p(buf[name].ptr.value + nbytes)

    def call(ptrs=None, count=n, wd=0.0, step=3, step_dev=None, flags=None, lo=0, rows=0, rowlen=0, skip=None):
        q = {k: buf[k].ptr for k in ('p', 'g', 'm', 'v', 'shadow')}
        q.update(ptrs or {})
        _call(NEW, q['p'], q['g'], q['m'], q['v'], q['shadow'], count, R.LR_HOST, None, R.BETA1, R.BETA2, R.EPS, R.f32(wd), step, step_dev,
              R.f32(0.0), None, R.f32(1.0), flags, lo, rows, rowlen, skip)

    FL = buf['flags'].ptr
    bad = {f'{k} 4 bytes off a 16-byte boundary': dict(ptrs={k: off(k, 4)}, count=n - 1) for k in 'pgmv'}
    bad.update({
        'shadow 2 bytes off an 8-byte boundary': dict(ptrs={'shadow': off('shadow', 2)}, count=n - 1),
        'a NULL p': dict(ptrs={'p': None}), 'a NULL g': dict(ptrs={'g': None}), 'a negative size': dict(count=-1),
        'lazy rows with weight decay': dict(wd=0.01, flags=FL, lo=0, rows=8, rowlen=8),
        'table_lo % 4 != 0': dict(flags=FL, lo=6, rows=8, rowlen=8),
        'rowlen % 4 != 0': dict(flags=FL, lo=0, rows=8, rowlen=6),
        'a table reaching past n': dict(flags=FL, lo=n - 60, rows=8, rowlen=8),
        'a table whose rows * rowlen wraps to a size that fits': dict(flags=FL, lo=n - 64, rows=(1 << 62) + 8, rowlen=8),
        'step < 1 without step_dev': dict(step=0),
        'a negative weight decay': dict(wd=-0.01), 'a NaN weight decay': dict(wd=NAN), 'an infinite weight decay': dict(wd=float('inf')),
        'skip_dev 2 bytes off a 4-byte boundary': dict(skip=off('skip', 2)),
    })
    orig = dict(p=p, g=g, m=m, v=v, shadow=p.bfloat16(), flags=fl, step_dev=torch.tensor([3.0]), skip=torch.tensor([0], dtype=torch.int32))
    for what, kw in bad.items():
        with pytest.raises(MMVIDError):
            call(**kw)
            pytest.fail(f'{what}: accepted')
        for k, gd in buf.items():
            same_bits(gd.check(f'{what}: {k}'), orig[k], f'{what}: {k} was modified')
    # the same arguments without the defect are accepted
    call(step=0, step_dev=buf['step_dev'].ptr, flags=FL, lo=n - 64, rows=8, rowlen=8, skip=buf['skip'].ptr)


# ================================================================================================================== the trainer
def test_flat_trainer_matches_torch_adamw(golden):
    """Six steps of the `bert_tiny` case with FlatTrainer(**optimizer_kwargs('adamw', 0.01)) against ONE live torch.optim.AdamW (betas
    (0.9, 0.95), weight decay 0.01) + clip_grad_norm_, fed each step's gradients as read from the trainer: rtol 1e-5, atol 1e-6, the
    bars of test_flat_trainer_matches_torch_adam.  The bf16 shadow equals bfloat16 of the weights after every step."""
    from mmvid_amd.engine import FlatTrainer, backward_order, optimizer_kwargs
    g, m = _bert_case(golden, 'bert_tiny', 0, False)
    tr = FlatTrainer(m, lr=1e-3, max_grad_norm=1.0, order=backward_order, **optimizer_kwargs('adamw', 0.01))
    assert tr.decoupled and tr._lazy is None
    text, frames = g['text'].to(DEV), g['frames'].to(DEV)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    ps = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    opt = torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01)
    for it in range(6):
        tr.zero_grad()
        lm, lr, lv = _with_tokens(m, g, lambda: m(text, target=frames, return_loss=True, rel=True, vid=True, rel_no_fully_masked=True,
                                                  _mask1=g['mask1'], _target_warp=g['warped_frames']))
        (7 * lm + 0.5 * lr + 0.5 * lv).backward()
        for q, (_, p) in zip(ps, named):
            q.grad = p.grad.detach().clone()
        tr.step()
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        opt.step()
        for (n, p), q in zip(named, ps):
            assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-6), (it + 1, n, (p.detach() - q.detach()).abs().max().item())
        assert torch.equal(tr.S, tr.P.bfloat16()), f'step {it + 1}: the shadow is not bfloat16 of the weights'
    # the decay is there: against the same run's L2 form the weights would differ by far more than the bars
    assert tr.state_dict()['param_groups'][0]['decoupled_weight_decay'] is True


ADAMW = dict(betas=(0.9, 0.95), weight_decay=0.01, decoupled_weight_decay=True)


def snap(tr):
    return {k: getattr(tr, k).clone() for k in ('P', 'M', 'V', 'S', '_step_dev') + (('E',) if tr.E is not None else ())}


def assert_snaps(a, b, what, keys=('P', 'M', 'V', 'S', '_step_dev')):
    for k in keys:
        same_bits(a[k].cpu(), b[k].cpu(), f'{what}: {k}')


@pytest.fixture(scope='module')
def case():
    return small_case(False, steps=6)  # (base model -- never run --, six input batches)


@pytest.fixture
def deterministic_mode():
    before = mmvid_amd.set_deterministic(True)
    yield
    mmvid_amd.set_deterministic(before)


def gained(inps, gains):
    return [dict(inp, gain=torch.tensor(g, device=DEV)) for inp, g in zip(inps, gains)]


@pytest.fixture(scope='module')
def eager_run(case):
    """Six eager AdamW steps in deterministic mode at width 768: the final state, shared and unchanged."""
    base, inps = case
    before = mmvid_amd.set_deterministic(True)
    try:
        m, tr, fn = make(base, ema=False, **ADAMW)
        assert tr.decoupled and tr._lazy is None
        losses = [one_step(tr, fn, inp) for inp in gained(inps, [1.0] * 6)]
        return snap(tr), losses
    finally:
        mmvid_amd.set_deterministic(before)


def test_adamw_captured_equals_eager(case, eager_run, deterministic_mode):
    from mmvid_amd.engine import GraphedStep
    base, inps = case
    inps = gained(inps, [1.0] * 6)
    m, tr, fn = make(base, ema=False, **ADAMW)
    step = GraphedStep(tr, fn, inps[0], warmup=1)  # one eager step on inps[0], then the capture
    assert step.graph is not None, step.capture_error
    losses = [step(**inp).clone() for inp in inps[1:]]
    assert_snaps(snap(tr), eager_run[0], 'captured against eager')
    for x, y in zip(losses, eager_run[1][1:]):
        same_bits(x.cpu(), y.cpu(), 'captured against eager: loss')
    assert tr.step_count == 6


def test_adamw_resumed_equals_uninterrupted(case, eager_run, deterministic_mode):
    base, inps = case
    inps = gained(inps, [1.0] * 6)
    m1, tr1, fn1 = make(base, ema=False, **ADAMW)
    for inp in inps[:3]:
        one_step(tr1, fn1, inp)
    model_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    opt_sd = copy.deepcopy(tr1.state_dict())
    assert opt_sd['param_groups'][0]['decoupled_weight_decay'] is True and opt_sd['param_groups'][0]['betas'] == (0.9, 0.95)
    del m1, tr1, fn1
    m2, tr2, fn2 = make(base, ema=False, **ADAMW)
    m2.frontend.seed = 1
    m2.load_state_dict(model_sd)  # the documented order: the model, the shadows, the trainer
    tr2.refresh_shadows()
    tr2.load_state_dict(opt_sd)
    for inp in inps[3:]:
        one_step(tr2, fn2, inp)
    assert_snaps(snap(tr2), eager_run[0], 'resumed against uninterrupted', ('P', 'M', 'V', '_step_dev'))
    # a trainer built for the other rule refuses the checkpoint
    m3, tr3, fn3 = make(base, ema=False, betas=(0.9, 0.95), weight_decay=0.01)
    with pytest.raises(ValueError, match='decoupled_weight_decay'):
        tr3.load_state_dict(opt_sd)


@pytest.mark.parametrize('wd', [0.01, 0.0], ids=['decay', 'lazy_rows'])
def test_adamw_step_through_a_nan_loss_equals_the_run_that_leaves_it_out(case, deterministic_mode, wd):
    """skip_nonfinite=True with the EMA on: the guard's verdict, the EMA and (wd = 0) the lazy rows with the decoupled entry."""
    base, inps = case
    kw = dict(ADAMW, weight_decay=wd)
    m, tr, fn = make(base, skip_nonfinite=True, **kw)
    assert (tr._lazy is not None) == (wd == 0.0) and tr.E is not None
    for inp in gained(inps, [1.0, 1.0, NAN, 1.0]):
        one_step(tr, fn, inp)
    st = tr.guard_stats()
    assert st['skipped'] == 1 and st['seen'] == 4 and tr.step_count == 3
    got = snap(tr)
    del m, tr, fn
    m, tr, fn = make(base, **kw)
    for i, inp in enumerate(gained(inps, [1.0] * 4)):
        if i == 2:  # forward and backward (the front end draws as in the other run), then the gradient is dropped
            forward_backward(tr, fn, inp)
            tr.zero_grad()
        else:
            one_step(tr, fn, inp)
    assert_snaps(got, snap(tr), f'wd={wd}: through a NaN loss against leaving the step out', ('P', 'M', 'V', 'S', 'E', '_step_dev'))
    assert bool(torch.isfinite(got['P']).all()) and got['_step_dev'].item() == 3.0


def test_adamw_step_names_the_decoupled_entry_and_the_default_step_does_not(case, deterministic_mode, monkeypatch):
    from mmvid_amd import _lib, ops
    base, inps = case
    inps = gained(inps, [1.0] * 6)
    seen = []
    real = _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', recorder)
    monkeypatch.setattr(ops, 'call', recorder)  # (ops binds the function by name at import)

    def tail(tr, fn):
        forward_backward(tr, fn, inps[0])
        del seen[:]
        tr.step()
        return [s for s in seen if s != 'mmvid_get_option']

    m, tr, fn = make(base, ema=False, **ADAMW)
    assert tail(tr, fn) == ['mmvid_counter_add', 'mmvid_grad_sqnorm_det', 'mmvid_adam_step_decoupled']
    m, tr, fn = make(base, ema=False, betas=(0.9, 0.95), weight_decay=0.01)
    assert tail(tr, fn) == ['mmvid_counter_add', 'mmvid_grad_sqnorm_det', 'mmvid_adam_step_rows']
