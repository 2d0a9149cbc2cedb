"""Non-finite guard on the GPU.  Kernel level, in the guarded, padded, poisoned buffers of tests/guarded.py: mmvid_step_guard against its
host replica (tests/guard_ref.py), the guarded Adam and EMA entries against the unguarded ones byte for byte (skip = 0, skip = NULL) and
against "nothing was written" (skip = 1 on a gradient of NaN), every refusal.  Trainer level, on the small BERT of
tests/test_ema_gpu.py in deterministic mode with the EMA on and lazy rows on and off: a finite run with the guard equals one without
it; a run with a NaN and an inf loss equals the run that left those steps out; captured equals eager; resume; and a trainer without the
guard launches what it always launched.  NaN in a gradient buffer is ordinary data: no test provokes a fault."""
import copy
import ctypes
import gc

import numpy as np
import pytest
import torch

import guard_ref as R
import mmvid_amd
from guarded import Guarded, bits, call_abi, ptr_of
from test_deterministic_step_gpu import KW, SEED, small_case
from test_models_gpu import DEV

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN, INF = float('nan'), float('inf')
DECAY, WARMUP = 0.3, True
GAINS = (1.0, 1.0, NAN, 1.0, INF, 1.0)
SKIPPED = (2, 4)  # (indices into GAINS)
ADAM_SIZES = (1, 3, 4, 1023, 1025, 2048 * 1024 + 4)  # (the last: the 2,048-block grid takes a second trip; the EMA's 512 blocks a fifth)


def same_bits(got, want, what):
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.as_tensor(want).cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        i = bad.nonzero()[:4].view(-1).tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first (index, got, want): '
                             f'{[(k, got.view(-1)[k].item(), want.view(-1)[k].item()) for k in i]}')


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------- mmvid_step_guard
def guard_call(sq, gs, state):
    """One launch on guarded copies of the state -> the new (step_dev, guard_i, guard_f) as numpy; sqnorm must come back untouched."""
    sdev, gi, gf = state
    SQ = Guarded(torch.tensor([sq], dtype=torch.float32))
    SD = Guarded(base=torch.tensor([float(sdev)], dtype=torch.float32))
    GI, GF = Guarded(base=torch.from_numpy(np.array(gi, np.int32))), Guarded(base=torch.from_numpy(np.array(gf, F32)))
    call_abi('mmvid_step_guard', SQ.ptr, float(gs), SD.ptr, GI.ptr, GF.ptr)
    what = f'step_guard sq={sq}'
    SQ.check(what + ': sqnorm')
    return F32(SD.check(what + ': step_dev').item()), GI.check(what + ': guard_i').numpy(), GF.check(what + ': guard_f').numpy()


def assert_state(got, want, what):
    assert got[0].view(np.int32) == want[0].view(np.int32), f'{what}: step_dev {got[0]} != {want[0]}'
    assert got[1].tolist() == want[1].tolist(), f'{what}: guard_i {got[1].tolist()} != {want[1].tolist()}'
    assert got[2].view(np.int32).tolist() == want[2].view(np.int32).tolist(), f'{what}: guard_f {got[2].tolist()} != {want[2].tolist()}'


@pytest.mark.parametrize('k', range(len(R.SQS)), ids=['zero', 'one', 'two_to_127', 'inf', 'nan'])
def test_step_guard_equals_the_replica(k):
    sq = R.SQS[k]
    for gs, start in ((1.0, R.fresh()), (0.125, (F32(7.0), np.array([1, 3, 2, 10], np.int32), F32([5.0, 6.0])))):
        got, want = guard_call(float(sq), gs, start), R.step_guard(sq, gs, *start)
        assert_state(got, want, f'sq={sq} grad_scale={gs}')
        assert int(got[1][0]) == int(k >= 3)


def test_step_guard_over_a_chain_of_six_calls():
    sqs = [F32(4.0), F32(np.nan), F32(np.inf), F32(3.0), F32(np.inf), F32(2.0**127)]
    want = R.chain(sqs, 0.5)
    state = R.fresh()
    for i, sq in enumerate(sqs):
        state = guard_call(float(sq), 0.5, state)
        assert_state(state, want[i], f'call {i + 1} of the chain')
    assert state[1].tolist() == [0, 3, 0, 6] and state[0] == F32(3.0)


# --------------------------------------------------------------------------------- mmvid_adam_step_guarded, mmvid_ema_update_guarded
def lazy_table(n):
    """(flags, lo, rows, rowlen) of a table inside [0, n): every other row flagged; below four elements a table of no rows."""
    rowlen, lo = (4, 0) if n < 64 else (12, 8)
    rows = (n - lo) // rowlen
    flags = (torch.arange(max(rows, 1)) % 2 == 0).to(torch.uint8)
    return flags, lo, rows, rowlen


def adam_inputs(n, nan_grad=False):
    gen = torch.Generator().manual_seed(4000 + n)
    p, m = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    g, v = torch.randn(n, generator=gen), torch.rand(n, generator=gen) * 0.01
    if nan_grad:
        g = torch.full((n,), NAN)
    return p, g, m, v


def skip_operand(skip):
    return None if skip is None else Guarded(torch.tensor([skip], dtype=torch.int32))


def launch_adam(entry, x, full, skip=None):
    """One call on guarded copies of x = (p, g, m, v); `full`: with a lazy table and the bf16 shadow.  -> the windows of p, m, v, shadow."""
    p, g, m, v = x
    n = p.numel()
    P, M, V, G = Guarded(base=p), Guarded(base=m), Guarded(base=v), Guarded(g)
    S = Guarded(base=p.bfloat16()) if full else None
    fl, lo, rows, rowlen = lazy_table(n) if full else (None, 0, 0, 0)
    FL = Guarded(fl) if fl is not None else None
    sq, sd = Guarded(torch.tensor([float(n) * 4.0])), Guarded(torch.tensor([3.0]))  # (clipped: sqrt(4 n) > max_norm = 1)
    SK = skip_operand(skip)
    args = (P.ptr, G.ptr, M.ptr, V.ptr, ptr_of(S), n, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0, sd.ptr, 1.0, sq.ptr, 1.0, ptr_of(FL), lo, rows, rowlen)
    call_abi(entry, *args, *(() if entry == 'mmvid_adam_step_rows' else (ptr_of(SK),)))
    what = f'{entry} n={n} full={full} skip={skip}'
    for name, op in (('g', G), ('sqnorm', sq), ('step_dev', sd), ('row_flags', FL), ('skip_dev', SK)):
        if op is not None:
            op.check(f'{what}: {name}')
    out = {'p': P.check(what + ': p'), 'm': M.check(what + ': m'), 'v': V.check(what + ': v')}
    if S is not None:
        out['shadow'] = S.check(what + ': shadow')
    return out


@pytest.mark.parametrize('full', [False, True], ids=['plain', 'lazy_and_shadow'])
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_guarded_adam(n, full):
    x = adam_inputs(n)
    want = launch_adam('mmvid_adam_step_rows', x, full)
    assert not torch.equal(want['p'], x[0]) or (full and n < 4)  # (the update does something, but where the table covers no row)
    for skip in (0, None):
        got = launch_adam('mmvid_adam_step_guarded', x, full, skip)
        for k in want:
            same_bits(got[k], want[k], f'n={n} full={full} skip={skip}: {k} against mmvid_adam_step_rows')
    p, g, m, v = adam_inputs(n, nan_grad=True)
    kept = launch_adam('mmvid_adam_step_guarded', (p, g, m, v), full, 1)  # (every guard zone is checked in there)
    for k, orig in (('p', p), ('m', m), ('v', v)) + ((('shadow', p.bfloat16()),) if full else ()):
        same_bits(kept[k], orig, f'n={n} full={full} skip=1: {k} must keep every byte')
        assert bool(torch.isfinite(kept[k].float()).all())


def ema_inputs(n):
    gen = torch.Generator().manual_seed(5000 + n)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen)


def launch_ema(entry, e, p, full, skip=None):
    n = e.numel()
    E, P = Guarded(base=e), Guarded(p)
    fl, lo, rows, rowlen = lazy_table(n) if full else (None, 0, 0, 0)
    FL = Guarded(fl) if fl is not None else None
    sd, SK = Guarded(torch.tensor([3.0])), skip_operand(skip)
    args = (E.ptr, P.ptr, n, 0.9, 1, 0, sd.ptr, ptr_of(FL), lo, rows, rowlen)
    call_abi(entry, *args, *(() if entry == 'mmvid_ema_update' else (ptr_of(SK),)))
    what = f'{entry} n={n} full={full} skip={skip}'
    for name, op in (('p', P), ('step_dev', sd), ('row_flags', FL), ('skip_dev', SK)):
        if op is not None:
            op.check(f'{what}: {name}')
    return E.check(what + ': ema')


@pytest.mark.parametrize('full', [False, True], ids=['plain', 'lazy'])
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_guarded_ema(n, full):
    e, p = ema_inputs(n)
    want = launch_ema('mmvid_ema_update', e, p, full)
    assert not torch.equal(want, e) or (full and n < 4)
    for skip in (0, None):
        same_bits(launch_ema('mmvid_ema_update_guarded', e, p, full, skip), want, f'n={n} full={full} skip={skip}: ema against mmvid_ema_update')
    poisoned = torch.full((n,), NAN)
    same_bits(launch_ema('mmvid_ema_update_guarded', e, poisoned, full, 1), e, f'n={n} full={full} skip=1: ema must keep every byte')


def test_every_refusal_returns_an_error_and_launches_nothing():
    from mmvid_amd import _lib, ops
    lib = _lib.load()
    V = ctypes.c_void_p
    n = 1000
    p, g, m, v = adam_inputs(n)
    e = ema_inputs(n)[0]
    buf = dict(p=Guarded(base=p), g=Guarded(g), m=Guarded(base=m), v=Guarded(base=v), s=Guarded(base=p.bfloat16()), e=Guarded(base=e),
               fl=Guarded(torch.ones(8, dtype=torch.uint8)), sq=Guarded(torch.tensor([4.0])), sd=Guarded(base=torch.tensor([3.0])),
               gi=Guarded(base=torch.tensor([0, 1, 0, 5], dtype=torch.int32)), gf=Guarded(base=torch.tensor([1.0, 1.0])),
               skip=Guarded(torch.tensor([0, 0], dtype=torch.int32)))
    q = {k: b.ptr for k, b in buf.items()}
    off = lambda k, by: V(q[k].value + by)  # noqa: E731
    refused = []

    def expect(rc, word, what):
        msg = lib.mmvid_last_error().decode()
        assert rc != 0 and word in msg, (what, rc, msg)
        refused.append(what)

    ok = dict(sq=q['sq'], sd=q['sd'], gi=q['gi'], gf=q['gf'])
    for kw, word in ((dict(sq=None), 'NULL'), (dict(sd=None), 'NULL'), (dict(gi=None), 'NULL'), (dict(gf=None), 'NULL'),
                     (dict(sq=off('sq', 2)), 'aligned'), (dict(sd=off('sd', 1)), 'aligned'), (dict(gi=off('gi', 2)), 'aligned'),
                     (dict(gf=off('gf', 3)), 'aligned')):
        a = dict(ok, **kw)
        expect(lib.mmvid_step_guard(a['sq'], 1.0, a['sd'], a['gi'], a['gf'], ops._stream()), word, ('step_guard', tuple(kw)))

    ok = dict(p=q['p'], g=q['g'], m=q['m'], v=q['v'], n=n, wd=0.0, step=0, sd=q['sd'], fl=None, lo=0, rows=0, rowlen=0, skip=q['skip'])
    for kw, word in ((dict(skip=off('skip', 2)), 'skip_dev'), (dict(skip=off('skip', 1)), 'skip_dev'), (dict(p=None), 'bad arguments'),
                     (dict(g=None), 'bad arguments'), (dict(m=None), 'bad arguments'), (dict(v=None), 'bad arguments'), (dict(n=-1), 'bad arguments'),
                     (dict(sd=None), 'bad arguments'), (dict(p=off('p', 4), n=n - 4), 'aligned'), (dict(fl=q['fl'], lo=8, rows=8, rowlen=12, wd=0.1), 'weight decay'),
                     (dict(fl=q['fl'], lo=8, rows=8, rowlen=124, n=999), 'lazy'), (dict(fl=q['fl'], lo=6, rows=8, rowlen=12), 'lazy'),
                     (dict(fl=q['fl'], lo=8, rows=8, rowlen=10), 'lazy')):
        a = dict(ok, **kw)
        rc = lib.mmvid_adam_step_guarded(a['p'], a['g'], a['m'], a['v'], q['s'], a['n'], 1e-3, None, 0.9, 0.999, 1e-8, a['wd'], a['step'], a['sd'],
                                         1.0, q['sq'], 1.0, a['fl'], a['lo'], a['rows'], a['rowlen'], a['skip'], ops._stream())
        expect(rc, word, ('adam_step_guarded', tuple(kw)))

    ok = dict(e=q['e'], p=q['p'], n=n, decay=0.9, step=1, fl=None, lo=0, rows=0, rowlen=0, skip=q['skip'])
    for kw, word in ((dict(skip=off('skip', 2)), 'skip_dev'), (dict(e=None), 'NULL'), (dict(p=None), 'NULL'), (dict(p=q['e']), 'overlap'),
                     (dict(p=off('e', 16)), 'overlap'), (dict(n=-1), 'negative'), (dict(e=off('e', 4), n=n - 4), 'aligned'), (dict(decay=1.0), 'decay'),
                     (dict(decay=NAN), 'decay'), (dict(step=0), 'step'), (dict(fl=q['fl'], lo=6, rows=8, rowlen=12), 'lazy'),
                     (dict(fl=q['fl'], lo=8, rows=8, rowlen=124, n=999), 'lazy')):
        a = dict(ok, **kw)
        rc = lib.mmvid_ema_update_guarded(a['e'], a['p'], a['n'], a['decay'], 0, a['step'], None, a['fl'], a['lo'], a['rows'], a['rowlen'], a['skip'],
                                          ops._stream())
        expect(rc, word, ('ema_update_guarded', tuple(kw)))
    torch.cuda.synchronize()
    assert len(refused) == 8 + 13 + 12
    for k, orig in (('p', p), ('m', m), ('v', v), ('s', p.bfloat16()), ('e', e), ('sd', torch.tensor([3.0])),
                    ('gi', torch.tensor([0, 1, 0, 5], dtype=torch.int32)), ('gf', torch.tensor([1.0, 1.0]))):
        same_bits(buf[k].check(f'after the refusals: {k}'), orig, f'a refused call changed {k}')
    for k in ('g', 'fl', 'sq', 'skip'):
        buf[k].check(f'after the refusals: {k}')
    # the wrappers: a verdict of another type is refused before the call, and so are guard buffers of the wrong size
    z = torch.zeros(8, device=DEV)
    with pytest.raises(TypeError, match='skip_dev'):
        ops.ema_update(z, z.clone(), 0.9, False, 1, skip_dev=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError, match='guard_i'):
        ops.step_guard(z[:1], 1.0, z[1:2], torch.zeros(3, device=DEV, dtype=torch.int32), z[2:4])


# ------------------------------------------------------------------------------------------------------------ the trainer
def make(base, ema=True, **kw):
    """tests/test_ema_gpu.py's `make` with the EMA on and a loss that carries a gain: a device scalar among the static inputs, so that
    a NaN or an inf enters a captured step without touching the data."""
    from mmvid_amd.engine import FlatTrainer, backward_order
    m = copy.deepcopy(base)
    m.frontend.seed, m.frontend.step = SEED, None
    if ema:
        kw = dict(kw, ema_decay=DECAY, ema_warmup=WARMUP)
    tr = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order, **kw)

    def fn(text, frames, gain):
        lm, lr, lv = m(text, target=frames, **KW)
        return (7.0 * lm + 0.5 * lr + 0.5 * lv) * gain
    return m, tr, fn


def forward_backward(tr, fn, inp):
    tr.zero_grad()
    loss = fn(**inp)
    loss.backward()
    return loss.detach().clone()


def one_step(tr, fn, inp):
    loss = forward_backward(tr, fn, inp)
    tr.step()
    return loss


def state(tr):
    out = {k: getattr(tr, k).clone() for k in ('P', 'M', 'V', 'E', 'S')}
    out['step_dev'] = tr._step_dev.clone()
    if tr.guard_i is not None:
        out['guard_i'], out['guard_f'] = tr.guard_i.clone(), tr.guard_f.clone()
    return out


def assert_states(a, b, what, keys=('P', 'M', 'V', 'E', 'S')):
    for k in keys:
        same_bits(a[k], b[k], f'{what}: {k}')


@pytest.fixture(scope='module')
def case():
    base, inps = small_case(False, steps=6)  # (base model -- never run --, six input batches)
    return base, [dict(inp, gain=torch.tensor(g, device=DEV)) for inp, g in zip(inps, GAINS)]


@pytest.fixture(scope='module')
def runs(case):
    """Per lazy-row mode, eager and in deterministic mode: the poisoned six-step run with the guard (its statistics after step 3 and at
    the end, its state after every step count the other tests need) and the unguarded run that leaves the two steps out.  Shared,
    unchanged."""
    base, inps = case
    before = mmvid_amd.set_deterministic(True)
    out = {}
    try:
        for lazy in (True, False):
            m, tr, fn = make(base, lazy_rows=lazy, skip_nonfinite=True)
            assert (tr._lazy is not None) == lazy and tr.guard_i.dtype == torch.int32 and tr.guard_f.dtype == torch.float32
            assert tuple(tr.guard_i.shape) == (4,) and tuple(tr.guard_f.shape) == (2,)
            r = {'losses': []}
            for i, inp in enumerate(inps):
                r['losses'].append(one_step(tr, fn, inp))
                if i == 2:
                    r['stats3'], r['count3'] = tr.guard_stats(), tr.step_count
            r['sq'] = tr._sq.cpu().numpy().copy()
            r['count_before'] = tr.step_count
            r['stats'], r['count'] = tr.guard_stats(), tr.step_count
            r['guarded'] = state(tr)
            del m, tr, fn
            m, tr, fn = make(base, lazy_rows=lazy)
            assert tr.guard_i is None and tr.guard_f is None
            for i, inp in enumerate(inps):
                if i in SKIPPED:  # forward and backward (the front end draws as in the other run), then the gradient is dropped
                    forward_backward(tr, fn, inp)
                    tr.zero_grad()
                else:
                    one_step(tr, fn, inp)
            r['left_out'] = state(tr)
            del m, tr, fn
            out[lazy] = r
    finally:
        mmvid_amd.set_deterministic(before)
    return out


@pytest.fixture
def deterministic_mode():
    before = mmvid_amd.set_deterministic(True)
    yield
    mmvid_amd.set_deterministic(before)


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_finite_run_with_the_guard_equals_the_run_without_it(case, deterministic_mode, lazy):
    base, inps = case
    finite = [dict(inp, gain=torch.tensor(1.0, device=DEV)) for inp in inps[:5]]
    got = {}
    for on in (True, False):
        m, tr, fn = make(base, lazy_rows=lazy, skip_nonfinite=on)
        losses = [one_step(tr, fn, inp) for inp in finite]
        got[on] = (state(tr), losses)
        if on:
            st = tr.guard_stats()
            assert st['skipped'] == 0 and st['seen'] == 5 and st['run'] == 0 and st['last_skipped'] is False and tr.step_count == 5
            assert st['grad_norm'] == st['last_finite_grad_norm'] == float(np.sqrt(tr._sq.cpu().numpy()[0], dtype=F32))
        del m, tr, fn
    assert_states(got[True][0], got[False][0], 'five finite steps, guard on against off', ('P', 'M', 'V', 'E', 'S', 'step_dev'))
    assert got[True][0]['step_dev'].item() == 5.0
    for x, y in zip(got[True][1], got[False][1]):
        assert torch.equal(x, y) and bool(torch.isfinite(x))


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_poisoned_run_equals_the_run_that_leaves_the_steps_out(runs, lazy):
    r = runs[lazy]
    assert_states(r['guarded'], r['left_out'], 'guarded run with a NaN and an inf loss against the run without those steps')
    for k in ('P', 'M', 'V', 'E', 'S'):
        assert bool(torch.isfinite(r['guarded'][k].float()).all()), f'{k} holds a non-finite value'
    assert r['guarded']['step_dev'].item() == r['left_out']['step_dev'].item() == 4.0
    assert not bool(torch.isfinite(r['losses'][2])) and not bool(torch.isfinite(r['losses'][4])) and bool(torch.isfinite(r['losses'][5]))
    s3, s = r['stats3'], r['stats']
    assert s3['run'] == 1 and s3['last_skipped'] is True and s3['skipped'] == 1 and s3['seen'] == 3 and r['count3'] == 2
    assert not np.isfinite(s3['grad_norm']) and np.isfinite(s3['last_finite_grad_norm'])
    assert s['skipped'] == 2 and s['seen'] == 6 and s['run'] == 0 and s['last_skipped'] is False
    assert r['count_before'] == 5 and r['count'] == 4  # (the host count: an upper bound until guard_stats() reconciles it)
    want = np.sqrt(r['sq'], dtype=F32)[0] * F32(1.0)  # sqrtf(_sq) * gscale of the last step (world 1)
    assert F32(s['grad_norm']).view(np.int32) == want.view(np.int32) and s['last_finite_grad_norm'] == s['grad_norm']
    assert r['guarded']['guard_i'].tolist() == [0, 2, 0, 6]


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_captured_run_equals_the_eager_run(case, runs, deterministic_mode, lazy):
    from mmvid_amd.engine import GraphedStep
    base, inps = case
    m, tr, fn = make(base, lazy_rows=lazy, skip_nonfinite=True)
    step = GraphedStep(tr, fn, inps[0], warmup=1)  # one eager step on inps[0], then the capture
    assert step.graph is not None, step.capture_error
    assert tr.guard_i.tolist() == [0, 0, 0, 1] and tr._step_dev.item() == 1.0  # the capture left the counters as they were
    losses = [step(**inp).clone() for inp in inps[1:]]
    want = runs[lazy]
    assert_states(state(tr), want['guarded'], 'captured against eager', ('P', 'M', 'V', 'E', 'S', 'step_dev', 'guard_i', 'guard_f'))
    for x, y in zip(losses, want['losses'][1:]):
        same_bits(x, y, 'captured against eager: loss')
    assert tr.step_count == 6
    assert tr.guard_stats() == want['stats'] and tr.step_count == 4
    # guard_stats() reads the device: refused while a stream captures
    x = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match='capture'):
            tr.guard_stats()
    torch.cuda.synchronize()


@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_rows', 'all_rows'])
def test_resume_after_a_skipped_step(case, runs, deterministic_mode, lazy):
    base, inps = case
    want = runs[lazy]
    m1, tr1, fn1 = make(base, lazy_rows=lazy, skip_nonfinite=True)
    for inp in inps[:3]:
        one_step(tr1, fn1, inp)
    assert tr1.step_count == 3
    model_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    opt_sd = copy.deepcopy(tr1.state_dict())
    assert tr1.step_count == 2 and opt_sd['guard'] == {'skipped': 1, 'seen': 3}
    assert {float(st['step']) for st in opt_sd['state'].values()} == {2.0}
    del m1, tr1, fn1
    m2, tr2, fn2 = make(base, lazy_rows=lazy, skip_nonfinite=True)
    m2.frontend.seed = 1
    m2.load_state_dict(model_sd)  # the documented order: the model, the shadows, the trainer
    tr2.refresh_shadows()
    tr2.load_state_dict(opt_sd)
    assert tr2.guard_i.tolist() == [0, 1, 0, 3] and tr2._step_dev.item() == 2.0 and tr2.step_count == 2
    for inp in inps[3:]:
        one_step(tr2, fn2, inp)
    assert_states(state(tr2), want['guarded'], 'resumed after the skipped step 3 against the uninterrupted run', ('P', 'M', 'V', 'E', 'step_dev'))
    st = tr2.guard_stats()
    assert st['skipped'] == 2 and st['seen'] == 6 and st['run'] == 0 and tr2.step_count == 4
    # a checkpoint in torch.optim.Adam's shape, without the entry: the counters start from zero
    plain = {k: v for k, v in opt_sd.items() if k in ('state', 'param_groups')}
    order = [n for n, p in m2.named_parameters() if p.requires_grad]
    plain['state'] = {j: opt_sd['state'][tr2.names.index(n)] for j, n in enumerate(order)}
    tr2.load_state_dict(plain)
    st = tr2.guard_stats()
    assert st['skipped'] == 0 and st['seen'] == 0 and st['run'] == 0 and st['last_skipped'] is False and tr2.step_count == 2
    # and a trainer without the guard ignores the entry and saves none
    m3, tr3, fn3 = make(base, lazy_rows=lazy)
    tr3.load_state_dict(opt_sd)
    assert tr3.guard_i is None and 'guard' not in tr3.state_dict() and tr3.step_count == 2
    with pytest.raises(RuntimeError, match='guard'):
        tr3.guard_stats()


def test_without_the_guard_a_step_launches_what_it_always_launched(case, deterministic_mode, monkeypatch):
    from mmvid_amd import _lib, ops
    base, inps = case
    new = {'mmvid_step_guard', 'mmvid_adam_step_guarded', 'mmvid_ema_update_guarded'}
    seen = []
    real = _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', recorder)
    monkeypatch.setattr(ops, 'call', recorder)  # (ops binds the function by name at import)

    def step_launches(tr, fn):
        """The entries one whole step names, and those of its tr.step() alone (but the option query of the mode, which launches nothing)."""
        del seen[:]
        forward_backward(tr, fn, inps[0])
        k = len(seen)
        tr.step()
        return list(seen), [s for s in seen[k:] if s != 'mmvid_get_option']

    # the trainers without the guard: the lists of the code before the guard existed, entry for entry
    m, tr, fn = make(base)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_counter_add', 'mmvid_grad_sqnorm_rows', 'mmvid_adam_step_rows', 'mmvid_ema_update'] and not new & set(whole)
    m, tr, fn = make(base, lazy_rows=False)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_counter_add', 'mmvid_grad_sqnorm_det', 'mmvid_adam_step_rows', 'mmvid_ema_update'] and not new & set(whole)
    m, tr, fn = make(base, ema=False)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_counter_add', 'mmvid_grad_sqnorm_rows', 'mmvid_adam_step_rows'] and not new & set(whole)
    # with the guard: the verdict stands where the counter stood, behind the norm it reads, and the guarded entries follow
    m, tr, fn = make(base, skip_nonfinite=True)
    whole, tail = step_launches(tr, fn)
    assert tail == ['mmvid_grad_sqnorm_rows', 'mmvid_step_guard', 'mmvid_adam_step_guarded', 'mmvid_ema_update_guarded']
    assert whole.count('mmvid_step_guard') == 1  # (mmvid_counter_add still occurs in `whole`: the front end counts its forwards)
