"""Weight EMA on the GPU: mmvid_ema_update against its host replica (tests/ema_ref.py) bit for bit in guarded buffers, the lazy
table, every refusal; FlatTrainer with ema_decay -- the sequence of averages against the replica, captured against eager, resume --
and the `ema_weights()` scope of BERT and ART-V against a fresh copy of the model that loaded `ema_state_dict()`."""
import copy
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import ema_ref as R
import mmvid_amd
from guarded import Guarded, call_abi
from test_deterministic_step_gpu import KW, SEED, small_case
from test_host_logic import tiny_vae
from test_models_gpu import DEV

pytestmark = pytest.mark.gpu
F32 = np.float32
DECAY, WARMUP = 0.3, True  # the trainers: d = 2/11, 3/12 (warm-up), then 0.3 from t = 3 on -- both branches within five steps
TS = (1, 2, 9, 89948, 89949, 89990, 89991, 100000)  # (89,948 / 89,949: where fp32 switches to decay = 0.9999, test_ema_host.py)


@pytest.fixture
def deterministic_mode():
    before = mmvid_amd.set_deterministic(True)
    yield
    mmvid_amd.set_deterministic(before)


def same_bits(got, want, what):
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.as_tensor(want).cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        i = bad.nonzero()[:4].view(-1).tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first (index, got, want): '
                             f'{[(k, got.view(-1)[k].item(), want.view(-1)[k].item()) for k in i]}')


# ------------------------------------------------------------------------------------------------ the kernel against the replica
def inputs(n, seed):
    """(ema, p): magnitudes 2^-40 .. 2^40 of both signs, and -- cyclically, shifted by n so that the small sizes hit different ones --
    ema == p, p == -ema, +0 and -0 on either side and on both."""
    rng = np.random.default_rng(seed)
    e = (np.exp2(rng.uniform(-40, 40, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    p = (np.exp2(rng.uniform(-40, 40, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    kind = (np.arange(n) + n) % 16
    p = np.where(kind == 0, e, p)
    p = np.where(kind == 1, -e, p)
    p = np.where(kind == 2, F32(0.0), p)
    p = np.where(kind == 3, F32(-0.0), p)
    e = np.where(kind == 4, F32(0.0), e)
    e = np.where(kind == 5, F32(-0.0), e)
    for k, (ze, zp) in zip((6, 7, 8, 9), ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0))):
        e, p = np.where(kind == k, F32(ze), e), np.where(kind == k, F32(zp), p)
    near = (e * F32(1 + 2.0**-20)).astype(F32)  # a weight next to its average: the everyday case
    p = np.where(kind == 10, near, p)
    return e.astype(F32), p.astype(F32)


def run_kernel(e, p, decay, warmup, t, on_device, lazy=None):
    """One launch in guarded buffers -> the new ema (CPU).  Guards, p and the flags must come back untouched."""
    n = e.size
    E, P = Guarded(base=torch.from_numpy(e.copy())), Guarded(torch.from_numpy(p.copy()))
    sdev = torch.tensor([float(t)], device=DEV, dtype=torch.float32) if on_device else None
    fl, lo, rows, rowlen = (None, 0, 0, 0)
    if lazy is not None:
        flags, lo, rows, rowlen = lazy
        fl = Guarded(torch.tensor(flags, dtype=torch.uint8))
    call_abi('mmvid_ema_update', E.ptr, P.ptr, n, float(decay), int(warmup), 0 if on_device else int(t),
             None if sdev is None else ctypes.c_void_p(sdev.data_ptr()), None if fl is None else fl.ptr, lo, rows, rowlen)
    what = f'n={n} decay={decay} warmup={warmup} t={t} step_dev={on_device}'
    P.check(what + ': p')
    if fl is not None:
        fl.check(what + ': flags')
    if sdev is not None:
        assert sdev.item() == float(t)
    return E.check(what + ': ema').reshape(-1), what


def combos(n):
    if n > 1 << 19:  # the large sizes: every decay and both forms, a few step counts (d and a do not depend on n)
        return [(0.0, False, 1, False), (0.9, True, 2, True), (0.9999, True, 89990, True), (0.9999, False, 7, False), (0.9, True, 100000, False)]
    out = []
    for decay in (0.0, 0.9, 0.9999):
        for on_device in (False, True):
            out.append((decay, False, 3, on_device))
            out += [(decay, True, t, on_device) for t in TS]
    return out


# (512 * 1024 + 5: the first size with a tail at which the kernel's 512-block grid takes a second trip; the last size: several trips)
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1025, 4099, 512 * 1024 + 5, 2 * 1024 * 1024 + 1029])
def test_kernel_equals_the_replica_bit_for_bit(n):
    e, p = inputs(n, 1000 + n)
    if n >= 1023:
        assert set(range(11)) <= set(((np.arange(n) + n) % 16).tolist())
    for decay, warmup, t, on_device in combos(n):
        R.assert_condition(e, p, decay, warmup, t)
        got, what = run_kernel(e, p, decay, warmup, t, on_device)
        same_bits(got, torch.from_numpy(R.update(e, p, decay, warmup, t)), what)


def test_small_sizes_cover_every_special_value():
    seen = set()
    for n in (1, 3, 4, 5):
        seen |= set(((np.arange(n) + n) % 16).tolist())
    assert {1, 3, 4, 5, 6, 7, 8, 9} <= seen


def test_lazy_table_rows_without_a_flag_are_not_touched():
    lo, rows, rowlen, flags = 8, 5, 12, [1, 0, 0, 1, 0]
    n = lo + rows * rowlen + 7
    e, p = inputs(n, 77)
    rng = np.random.default_rng(78)
    for r, f in enumerate(flags):  # E != P planted in every element of the unflagged rows
        if not f:
            sl = slice(lo + r * rowlen, lo + (r + 1) * rowlen)
            e[sl], p[sl] = rng.uniform(1, 2, rowlen).astype(F32), rng.uniform(3, 4, rowlen).astype(F32)
    for decay, warmup, t, on_device in ((0.9, False, 1, False), (0.9999, True, 9, True), (0.0, False, 2, True)):
        R.assert_condition(e, p, decay, warmup, t)
        got, what = run_kernel(e, p, decay, warmup, t, on_device, lazy=(flags, lo, rows, rowlen))
        same_bits(got, torch.from_numpy(R.update_rows(e, p, decay, warmup, t, flags, lo, rows, rowlen)), what + ' lazy')
        for r, f in enumerate(flags):
            sl = slice(lo + r * rowlen, lo + (r + 1) * rowlen)
            if not f:
                same_bits(got[sl], torch.from_numpy(e[sl]), what + f': unflagged row {r}')
            else:
                assert not np.array_equal(got[sl].numpy().view(np.int32), e[sl].view(np.int32))
        full, _ = run_kernel(e, p, decay, warmup, t, on_device)  # the same buffers without the table: every row is updated
        same_bits(full, torch.from_numpy(R.update(e, p, decay, warmup, t)), what + ' no table')


def test_every_refusal_returns_an_error_and_launches_nothing():
    from mmvid_amd import _lib, ops
    lib = _lib.load()
    n = 1000
    e, p = inputs(n, 5)
    E, P = Guarded(base=torch.from_numpy(e.copy())), Guarded(torch.from_numpy(p.copy()))
    fl = torch.ones(8, dtype=torch.uint8, device=DEV)
    sdev = torch.ones(1, device=DEV)
    V = ctypes.c_void_p
    ok = dict(ema=E.ptr, p=P.ptr, n=n, decay=0.9, warmup=0, step=1, sdev=None, flags=None, lo=0, rows=0, rowlen=0)
    flp = V(fl.data_ptr())
    cases = [(dict(ema=None), 'NULL'), (dict(p=None), 'NULL'), (dict(p=E.ptr), 'overlap'), (dict(p=V(E.ptr.value + 16)), 'overlap'),
             (dict(ema=V(P.ptr.value + 4 * n - 16)), 'overlap'), (dict(n=-1), 'negative'), (dict(ema=V(E.ptr.value + 4), n=n - 4), 'aligned'),
             (dict(p=V(P.ptr.value + 8), n=n - 4), 'aligned'), (dict(decay=1.0), 'decay'), (dict(decay=-0.5), 'decay'),
             (dict(decay=float('nan')), 'decay'), (dict(step=0), 'step'), (dict(step=-1), 'step'),
             (dict(flags=flp, lo=8, rows=8, rowlen=124, n=999), 'lazy'), (dict(flags=flp, lo=6, rows=8, rowlen=12), 'lazy'),
             (dict(flags=flp, lo=8, rows=8, rowlen=10), 'lazy'), (dict(flags=flp, lo=-4, rows=8, rowlen=12), 'lazy'),
             (dict(flags=flp, lo=1004, rows=0, rowlen=4), 'lazy')]
    for kw, word in cases:
        a = dict(ok, **kw)
        rc = lib.mmvid_ema_update(a['ema'], a['p'], a['n'], a['decay'], a['warmup'], a['step'], a['sdev'], a['flags'], a['lo'], a['rows'],
                                  a['rowlen'], ops._stream())
        msg = lib.mmvid_last_error().decode()
        assert rc != 0 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    same_bits(E.check('after the refusals: ema'), torch.from_numpy(e), 'a refused call changed ema')
    P.check('after the refusals: p')
    # n == 0 launches nothing and is no error; and the accepted call still works afterwards
    assert lib.mmvid_ema_update(E.ptr, P.ptr, 0, 0.9, 0, 1, None, None, 0, 0, 0, ops._stream()) == 0
    assert lib.mmvid_ema_update(E.ptr, P.ptr, 0, 0.9, 0, 0, V(sdev.data_ptr()), None, 0, 0, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    same_bits(E.check('n = 0: ema'), torch.from_numpy(e), 'n = 0 changed ema')
    with pytest.raises(ValueError, match='elements'):
        ops.ema_update(torch.zeros(8, device=DEV), torch.zeros(12, device=DEV), 0.9, False, 1)
    with pytest.raises(TypeError):
        ops.ema_update(torch.zeros(8, device=DEV, dtype=torch.bfloat16), torch.zeros(8, device=DEV), 0.9, False, 1)


# ------------------------------------------------------------------------------------------------------------ the trainer
def make(base, **kw):
    """tests/test_deterministic_step_gpu.py's `make` (pixel path) with the trainer's keywords open."""
    from mmvid_amd.engine import FlatTrainer, backward_order
    m = copy.deepcopy(base)
    m.frontend.seed, m.frontend.step = SEED, None
    tr = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order, **kw)

    def fn(text, frames):
        lm, lr, lv = m(text, target=frames, **KW)
        return 7.0 * lm + 0.5 * lr + 0.5 * lv
    return m, tr, fn


def one_step(tr, fn, inp):
    tr.zero_grad()
    loss = fn(**inp)
    loss.backward()
    tr.step()
    return loss.detach().clone()


def replica_steps(E0, Ps, t0, changed):
    """The replica applied to the elements `changed` (an index array) for the weights Ps[0], Ps[1], ... at steps t0, t0 + 1, ...; in
    slices on a few threads (numpy releases the lock).  Elements outside `changed` keep E0: there every P equals E0 (asserted by the
    caller), where the update is the identity."""
    e = E0[changed]
    cuts = np.linspace(0, e.size, 9).astype(np.int64)

    def piece(k):
        a, b = cuts[k], cuts[k + 1]
        x = e[a:b]
        for i, P in enumerate(Ps):
            q = P[changed[a:b]]
            R.assert_condition(x, q, DECAY, WARMUP, t0 + i)
            x = R.update(x, q, DECAY, WARMUP, t0 + i)
        return x

    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(piece, range(8)))
    out = E0.copy()
    out[changed] = np.concatenate(parts)
    return out


@pytest.fixture(scope='module')
def case():
    return small_case(False)  # (base model -- never run --, five input batches)


@pytest.fixture(scope='module')
def runs(case):
    """Five eager deterministic steps with EMA, lazy rows on and off: P after every step, and the final state.  Shared, unchanged."""
    base, inps = case
    before = mmvid_amd.set_deterministic(True)
    out = {}
    try:
        for lazy in (True, False):
            m, tr, fn = make(base, ema_decay=DECAY, ema_warmup=WARMUP, lazy_rows=lazy)
            assert (tr._lazy is not None) == lazy
            Ps, losses = [tr.P.cpu().numpy().copy()], []
            for inp in inps:
                losses.append(one_step(tr, fn, inp))
                Ps.append(tr.P.cpu().numpy().copy())
            flags = tr._lazy['flags'].cpu().clone() if lazy else None
            if not lazy:  # (kept as the comparison with the first run's: six copies of the weights once, not twice)
                Ps = [np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(Ps, out[True]['Ps'])]
            out[lazy] = dict(Ps=Ps, P=tr.P.clone(), M=tr.M.clone(), V=tr.V.clone(), E=tr.E.clone(), losses=losses, flags=flags,
                             lazy=dict(tr._lazy, flags=None) if lazy else None, names=list(tr.names), offsets=list(tr.offsets))
            del m, tr, fn
    finally:
        mmvid_amd.set_deterministic(before)
    return out


def test_trainer_average_equals_the_replica_over_five_steps(runs):
    a, b = runs[True], runs[False]
    assert len(b['Ps']) == 6 and all(b['Ps']), f'P after steps 0 .. 5, lazy rows on against off, equal: {b["Ps"]}'
    same_bits(a['E'], b['E'], 'E after five steps: lazy rows on against off')
    Ps = a['Ps']
    moved = np.zeros(Ps[0].size, bool)
    for P in Ps[1:]:
        moved |= P.view(np.int32) != Ps[0].view(np.int32)
    changed = np.flatnonzero(moved)
    assert 0 < changed.size < Ps[0].size  # the untouched rows of text_emb (and the alignment padding) never move
    assert not (Ps[0][~moved].view(np.int32) == np.int32(-2**31)).any()  # (no -0 among them: the identity there is bit for bit)
    want = replica_steps(Ps[0], Ps[1:], 1, changed)
    same_bits(a['E'], torch.from_numpy(want), 'E after five steps against the replica applied to P_0 .. P_5')
    assert not torch.equal(a['E'], a['P'])
    # rows of the lazy table without a flag hold E == P
    z, flags = a['lazy'], a['flags']
    lo, hi = z['lo'], z['lo'] + z['rows'] * z['rowlen']
    assert z['name'] == 'text_emb.weight' and 0 < int(flags.sum()) < z['rows']
    rowsE, rowsP = a['E'][lo:hi].view(z['rows'], -1).cpu(), a['P'][lo:hi].view(z['rows'], -1).cpu()
    same_bits(rowsE[flags == 0], rowsP[flags == 0], 'unflagged rows of text_emb: E against P')
    assert not torch.equal(rowsE[flags == 1], rowsP[flags == 1])


def test_no_ema_launch_without_ema(case, deterministic_mode, monkeypatch):
    from mmvid_amd import _lib, ops
    base, inps = case
    seen = []
    real = _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', recorder)
    monkeypatch.setattr(ops, 'call', recorder)  # (ops binds the function by name at import)
    m, tr, fn = make(base)
    assert tr.E is None and tr.ES is None and 'ema' not in tr.state_dict()
    one_step(tr, fn, inps[0])
    assert 'mmvid_adam_step_rows' in seen and 'mmvid_ema_update' not in seen
    del seen[:]
    m, tr, fn = make(base, ema_decay=DECAY)
    one_step(tr, fn, inps[0])
    assert seen.count('mmvid_ema_update') == 1 and seen.index('mmvid_ema_update') > seen.index('mmvid_adam_step_rows')


def test_captured_step_equals_eager_step_with_ema(case, runs, deterministic_mode):
    from mmvid_amd.engine import GraphedStep
    base, inps = case
    m, tr, fn = make(base, ema_decay=DECAY, ema_warmup=True)
    step = GraphedStep(tr, fn, inps[0], warmup=1)
    assert step.graph is not None, step.capture_error
    losses = [step(**inp).clone() for inp in inps[1:]]
    want = runs[True]
    for name in ('P', 'M', 'V', 'E'):
        assert torch.equal(getattr(tr, name), want[name]), f'captured against eager: {name} differs'
    for x, y in zip(losses, want['losses'][1:]):
        assert torch.equal(x, y)
    assert tr.step_count == 5
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match='ema_weights'):
            step(**inps[1])
    assert torch.equal(tr.P, want['P']) and torch.equal(tr.E, want['E'])  # nothing ran


def test_resumed_run_equals_uninterrupted_run_with_ema(case, runs, deterministic_mode):
    base, inps = case
    want = runs[True]
    m1, tr1, fn1 = make(base, ema_decay=DECAY, ema_warmup=WARMUP)
    for inp in inps[:3]:
        one_step(tr1, fn1, inp)
    model_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    opt_sd = copy.deepcopy(tr1.state_dict())
    assert not torch.equal(opt_sd['ema']['weights'][tr1.names[-1]].cpu(), model_sd[tr1.names[-1]])
    for with_ema in (True, False):
        m2, tr2, fn2 = make(base, ema_decay=DECAY, ema_warmup=WARMUP)
        m2.frontend.seed = 1
        m2.load_state_dict(model_sd)  # the documented order: the model, the shadows, the trainer
        tr2.refresh_shadows()
        tr2.load_state_dict(opt_sd if with_ema else {k: v for k, v in opt_sd.items() if k != 'ema'})
        assert tr2._ema_primed == with_ema
        if not with_ema:  # documented: E starts again from the loaded weights
            tr2.ema_state_dict()
            assert tr2._ema_primed and torch.equal(tr2.E, tr2.P)
            assert np.array_equal(tr2.P.cpu().numpy().view(np.int32), want['Ps'][3].view(np.int32))
        for inp in inps[3:]:
            one_step(tr2, fn2, inp)
        for name in ('P', 'M', 'V'):
            assert torch.equal(getattr(tr2, name), want[name]), f'resumed (ema entry: {with_ema}): {name} differs'
        assert tr2.step_count == 5
        if with_ema:
            assert torch.equal(tr2.E, want['E']), 'resumed: E differs from the uninterrupted run'
        else:
            assert not torch.equal(tr2.E, want['E'])
            Ps = want['Ps']
            moved = (Ps[4].view(np.int32) != Ps[3].view(np.int32)) | (Ps[5].view(np.int32) != Ps[3].view(np.int32))
            same_bits(tr2.E, torch.from_numpy(replica_steps(Ps[3], Ps[4:], 4, np.flatnonzero(moved))), 'E re-primed at step 3, then two steps')


# -------------------------------------------------------------------------------------------------------------- the scope
def fresh(base, sd):
    """A copy of the never-run base model that loaded `sd`; it has no trainer."""
    m = copy.deepcopy(base)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    return m


def bert_tokens(m, text, mp):
    images, _, seq = m.generate_images(text, mask_predict_steps=4, mp_config=mp, dynamic=False, seeds=[5, 2**40 + 6])
    return seq.clone(), images.clone()


def msm_logits(m, text, tok):
    with torch.no_grad():
        ctrl = m(text, return_loss=False)
        emb = m.image_emb.weight[tok] + m.target_pos_emb.table()
        out = m.transformer_forward(torch.cat([ctrl, emb], 1))
        return m.to_logits_rows(out[:, m.control_seq_len:]).clone()


def test_scope_bert_samples_from_the_average(case, golden, deterministic_mode):
    base, inps = case
    mp = dict(golden('mask_predict').meta['mp_config'], B=2, N1_t=1.0, N2_t=0.0)
    text = inps[0]['text'][:2].contiguous()
    tok = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(9)).to(DEV)
    m, tr, fn = make(base, ema_decay=DECAY, ema_warmup=WARMUP)
    twin_m, twin, twin_fn = make(base, ema_decay=DECAY, ema_warmup=WARMUP)  # the same steps and the same calls, never inside the scope
    for inp in inps[:3]:
        one_step(tr, fn, inp), one_step(twin, twin_fn, inp)
    frozen = [(p, p.data_ptr()) for p in m.parameters() if not p.requires_grad]

    def both(model):
        seq, images = bert_tokens(model, text, mp)
        return seq, images, msm_logits(model, text, tok)

    def check(got, want, what):
        assert torch.equal(got[0], want[0]), f'{what}: tokens differ in {(got[0] != want[0]).sum().item()} of {got[0].numel()}'
        assert torch.equal(got[1], want[1]), f'{what}: decoded frames differ'
        same_bits(got[2], want[2], f'{what}: MSM logits')

    outside = both(m)
    both(twin_m)
    with tr.ema_weights():
        assert all(p.data_ptr() == at for p, at in frozen) and tr.ES is not None
        inside1 = both(m)
    both(twin_m)
    check(inside1, both(fresh(base, tr.ema_state_dict())), 'inside the scope against a copy that loaded ema_state_dict()')
    assert not torch.equal(inside1[2], outside[2])  # the average is not the iterate
    after = both(m)
    both(twin_m)
    check(after, outside, 'after the scope against before it')
    check(after, both(fresh(base, m.state_dict())), 'after the scope against a copy that loaded state_dict()')
    tr._check_bindings()
    # one more step, a second entry: nothing may be older than the new average
    one_step(tr, fn, inps[3]), one_step(twin, twin_fn, inps[3])
    with tr.ema_weights():
        inside2 = both(m)
    both(twin_m)
    check(inside2, both(fresh(base, tr.ema_state_dict())), 'second entry against a copy that loaded the NEW ema_state_dict()')
    assert not torch.equal(inside2[2], inside1[2])
    with tr.ema_weights():  # and a third, straight after: the same again
        check(both(m), inside2, 'third entry against the second')
    both(twin_m)
    # training goes on as if the scope had never been entered
    la, lb = one_step(tr, fn, inps[4]), one_step(twin, twin_fn, inps[4])
    assert torch.equal(la, lb)
    for name in ('P', 'M', 'V', 'E', 'S'):
        assert torch.equal(getattr(tr, name), getattr(twin, name)), f'the step after the scope: {name} differs from the trainer that never entered it'


def test_scope_artv_samples_from_the_average():
    from mmvid_amd.dalle_artv import DALLE
    from mmvid_amd.engine import FlatTrainer, backward_order
    torch.manual_seed(19)
    base = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
                 num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).train()
    gen = torch.Generator().manual_seed(20)
    text = torch.randint(1, 49408, (4, 16), generator=gen)
    text[1, 11:] = 0
    text, vis = text.to(DEV), torch.randint(0, 256, (4, 16), generator=gen).to(DEV)
    target = torch.randint(0, 256, (4, 32), generator=gen).to(DEV)
    seeds = [901, 2**40 + 2, 903, 904]
    m = copy.deepcopy(base)
    tr = FlatTrainer(m, lr=1e-3, max_grad_norm=1.0, order=backward_order, ema_decay=0.5)

    def step():
        tr.zero_grad()
        loss, _, _ = m(text, visual=vis, target=target, return_loss=True)
        loss.backward()
        tr.step()

    def sample(model, rows):
        return model.sample_tokens(text[:rows], visual=vis[:rows], seeds=seeds[:rows])[1].clone()

    def check(what):
        with tr.ema_weights():
            got = {rows: sample(m, rows) for rows in (1, 4)}  # (one video: the one-launch token path; four: the captured step)
            images = m.generate_images(text[:1], visual=vis[:1], seeds=seeds[:1])[0].clone()
        copy_ = fresh(base, tr.ema_state_dict())
        for rows in (1, 4):
            want = sample(copy_, rows)
            assert got[rows].shape == (rows, 32) and torch.equal(got[rows], want), \
                f'{what}, batch {rows}: {(got[rows] != want).sum().item()} of {want.numel()} tokens differ'
        assert torch.equal(images, copy_.generate_images(text[:1], visual=vis[:1], seeds=seeds[:1])[0])
        return got

    step(), step()
    first = check('inside the scope against a copy that loaded ema_state_dict()')
    plain = sample(m, 4)
    assert torch.equal(plain, sample(fresh(base, m.state_dict()), 4)), 'after the scope against a copy that loaded state_dict()'
    tr._check_bindings()
    step()
    second = check('second entry, after one more step')
    assert not torch.equal(tr.E, tr.P)
    assert not (torch.equal(first[4], second[4]) and torch.equal(first[4], plain))  # (the three weight sets do not all sample alike)
