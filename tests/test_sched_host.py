"""AdamW and the learning-rate schedules without a GPU: the host views of the schedule classes against torch's own schedulers stepped
as train.py:373-374 steps them, the plateau rule in fp64 against torch and in fp32 against fp64, the two factories against the
reference's constants, the three header entries with their bindings and refusals (checked before any launch), and the FlatTrainer
side on a CPU trainer -- keywords, refusals, checkpoints."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import sched_ref as S
from optim_ref import f32
from test_host_logic import tiny_bert

P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
ENTRIES = {'mmvid_adam_step_decoupled': [P, P, P, P, P, I64, F, P, F, F, F, F, I, P, F, P, F, P, I64, I64, I, P, P],
           'mmvid_lr_schedule_ext': [P, I, F, F, I, I64, I64, F, P, P],
           'mmvid_lr_plateau': [P, P, I, F, I, I, F, F, F, P, P, P, P]}


# --------------------------------------------------------------------------------------------- closed forms against torch
def torch_rates(make, lr, every, iters):
    """The learning rate of iterations 0 .. iters - 1 when torch's scheduler is stepped after every `every`-th iteration
    (train.py:373-374: `if (i + 1) % every == 0: scheduler.step()`)."""
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=lr)
    sched = make(opt)
    out = []
    for i in range(iters):
        out.append(opt.param_groups[0]['lr'])
        opt.step()
        if (i + 1) % every == 0:
            sched.step()
    return out


@pytest.mark.parametrize('every', [1, 3])
def test_step_lr_equals_torch(every):
    from mmvid_amd.engine import StepLR
    size = 3
    want = torch_rates(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=size, gamma=0.5), 1e-4, every, every * (3 * size + 5))
    sc = StepLR(1e-4, size, gamma=0.5, every=every)
    assert [sc.lr_at(i) for i in range(len(want))] == want
    assert want[0] == 1e-4 and want[-1] == 1e-4 * 0.5**4


@pytest.mark.parametrize('T', [7, 100])
@pytest.mark.parametrize('every', [1, 3])
def test_cosine_lr_follows_torch(every, T):
    """Within 1e-12 relative: a hundred times what torch's own recursion deviates from the closed form at these sizes."""
    from mmvid_amd.engine import CosineAnnealingLR
    want = torch_rates(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T, eta_min=1e-6), 1e-4, every, every * (3 * T + 5))
    sc = CosineAnnealingLR(1e-4, T, eta_min=1e-6, every=every)
    worst = max(abs(sc.lr_at(i) - w) / w for i, w in enumerate(want))
    print(f'cosine T_max={T} every={every}: worst relative deviation from torch {worst:.3e}')
    assert worst <= 1e-12
    assert sc.lr_at(0) == 1e-4 and abs(sc.lr_at(every * T) - 1e-6) <= 1e-18 and abs(sc.lr_at(every * 2 * T) - 1e-4) <= 1e-18


def test_warmup_decay_lr_at_hand_computed_points():
    from mmvid_amd.engine import WarmupDecayLR
    lo, hi, warm, total = 1e-6, 1e-4, 8, 40
    for every in (1, 3):
        sc = WarmupDecayLR(total, lo, hi, warm, every=every)
        at = lambda ns: sc.lr_at(ns * every)
        assert at(0) == hi and sc.lr_at(every - 1) == hi                   # before the first scheduler step: the construction rate
        assert at(1) == lo                                                 # k = 0: log(1) = 0
        assert abs(at(2) - (lo + (hi - lo) * math.log(2) / math.log(8))) <= 1e-20
        assert at(warm) == hi                                              # k = warm - 1: log(warm) / log(warm)
        assert at(warm + 1) == hi                                          # k = warm: (total - warm) / (total - warm)
        assert abs(at(warm + 2) - (lo + (hi - lo) * 31 / 32)) <= 1e-20
        assert abs(at(total) - (lo + (hi - lo) / 32)) <= 1e-20             # k = total - 1
        assert at(total + 1) == lo and at(total + 50) == lo                # k >= total: clamped at 0
    assert WarmupDecayLR(10, lo, hi, 1).warmup == 2                        # the clamp of WarmupLR


# ------------------------------------------------------------------------------------------------------------------ plateau
def test_plateau_rule_in_fp64_equals_torch():
    losses = S.plateau_losses()
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='min', factor=0.5, patience=2, cooldown=5, min_lr=1e-6)
    want = []
    for x in losses:
        sched.step(x)
        want.append(opt.param_groups[0]['lr'])
    got, (sf, si) = S.plateau_run(losses, lr=1e-4, dtype=np.float64, **S.REFERENCE_PLATEAU)
    assert got == want
    assert want[0] == 1e-4 and want[-1] == 1e-6 and len(set(want)) == 8 and si[2] == 7
    assert sf[1] == sched.best and si[0] == sched.num_bad_epochs and si[1] == sched.cooldown_counter
    assert any(math.isnan(x) for x in losses) and any(math.isinf(x) for x in losses)


def test_plateau_rule_in_fp32_equals_fp64_away_from_ties():
    """On fp32 inputs the two precisions take the same decisions -- and, the factor being 0.5, reach the same rates -- provided no
    comparison is closer to a tie than the rounding of its sides.  The condition is asserted on this sequence, not assumed."""
    from mmvid_amd.engine import ReduceLROnPlateau
    losses = [f32(x) for x in S.plateau_losses()]
    cfg = {k: f32(v) if isinstance(v, float) else v for k, v in S.REFERENCE_PLATEAU.items()}
    trace = []
    want, end64 = S.plateau_run(losses, lr=f32(1e-4), dtype=np.float64, trace=trace, **cfg)
    assert len(trace) > len(losses) and S.no_near_ties(trace)
    got, end32 = S.plateau_run(losses, lr=f32(1e-4), dtype=np.float32, **cfg)
    assert got == want and end32[1] == end64[1] and end32[0][0] == end64[0][0]
    assert got[-1] == f32(1e-6) and end32[1][2] == 7
    # the class's host view is the same fp32 rule, and continues from a state
    sc = ReduceLROnPlateau(1e-4)
    assert sc.replay(losses)[0] == got
    half, state = sc.replay(losses[:40])
    assert half + sc.replay(losses[40:], state)[0] == got
    # near a tie the helper says so
    assert not S.no_near_ties([(1.0, 1.0 + 2.0**-23)]) and S.no_near_ties([(1.0, 1.001), (float('nan'), 1.0), (float('inf'), 1.0)])


# ---------------------------------------------------------------------------------------------------------------- factories
def test_lr_scheduler_from_args_mirrors_prepare_lr_scheduler():
    from mmvid_amd import engine as E
    mk = lambda name: E.lr_scheduler_from_args(name, 3e-4, iters=2000, step_size=50, warmup=100, every=4)
    sc = mk('reducelronplateau')
    assert isinstance(sc, E.ReduceLROnPlateau)
    assert (sc.lr, sc.factor, sc.patience, sc.cooldown, sc.min_lr, sc.threshold, sc.eps, sc.every) == (3e-4, 0.5, 2, 5, 1e-6, 1e-4, 1e-8, 4)
    sc = mk('steplr')
    assert isinstance(sc, E.StepLR) and (sc.lr, sc.step_size, sc.gamma, sc.every) == (3e-4, 50, 0.5, 4)
    sc = mk('cosineannealinglr')
    assert isinstance(sc, E.CosineAnnealingLR) and (sc.lr, sc.T_max, sc.eta_min, sc.every) == (3e-4, 50, 1e-6, 4)
    sc = mk('warmupdecaylr')
    assert isinstance(sc, E.WarmupDecayLR) and (sc.total, sc.min_lr, sc.max_lr, sc.warmup, sc.every) == (2000, 1e-6, 3e-4, 100, 4)
    sc = mk('warmuplr')
    assert type(sc) is E.WarmupLR and (sc.min_lr, sc.max_lr, sc.warmup, sc.every) == (1e-6, 3e-4, 100, 4)
    for name in ('linear', '', None):
        with pytest.raises(NotImplementedError):
            mk(name)


def test_optimizer_kwargs_mirrors_get_optimizer():
    from mmvid_amd.engine import optimizer_kwargs
    assert optimizer_kwargs('adam', 0.01) == dict(betas=(0.9, 0.999), weight_decay=0.01, decoupled_weight_decay=False)
    assert optimizer_kwargs('adamw', 0.01) == dict(betas=(0.9, 0.95), weight_decay=0.01, decoupled_weight_decay=True)
    assert optimizer_kwargs('adamw')['weight_decay'] == 0.0
    for name in ('sgd', 'AdamW', None):
        with pytest.raises(NotImplementedError):
            optimizer_kwargs(name)


def test_schedule_constructors_refuse_bad_arguments():
    from mmvid_amd import engine as E
    for make in (lambda: E.StepLR(1e-4, 0), lambda: E.StepLR(1e-4, 3, gamma=0.0), lambda: E.StepLR(1e-4, 3, gamma=1.5),
                 lambda: E.StepLR(1e-4, 3, every=0), lambda: E.StepLR(-1e-4, 3), lambda: E.StepLR(1e-4, 2.5),
                 lambda: E.CosineAnnealingLR(1e-4, 0), lambda: E.CosineAnnealingLR(1e-4, 7, eta_min=float('nan')),
                 lambda: E.CosineAnnealingLR(1e-4, 7, every=True),
                 lambda: E.WarmupDecayLR(10, 1e-6, 1e-4, 20), lambda: E.WarmupDecayLR(0, 1e-6, 1e-4, 0), lambda: E.WarmupDecayLR(10, 1e-6, 1e-4, 5, every=0),
                 lambda: E.ReduceLROnPlateau(1e-4, factor=1.0), lambda: E.ReduceLROnPlateau(1e-4, factor=0.0),
                 lambda: E.ReduceLROnPlateau(1e-4, patience=-1), lambda: E.ReduceLROnPlateau(1e-4, cooldown=1.5),
                 lambda: E.ReduceLROnPlateau(1e-4, threshold=1.0), lambda: E.ReduceLROnPlateau(1e-4, min_lr=-1e-6),
                 lambda: E.ReduceLROnPlateau(float('inf')), lambda: E.ReduceLROnPlateau(1e-4, every=0)):
        with pytest.raises(ValueError):
            make()


# ------------------------------------------------------------------------------------------------- the header and the binding
def test_entry_points_are_declared_bound_and_built():
    from mmvid_amd import _cdecl, _lib
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    lib = _lib.load()
    for name, args in ENTRIES.items():
        assert name in hdr.functions and hdr.functions[name][0] is ctypes.c_int, name
        assert len(re.findall(r'\b%s\s*\(' % name, bare)) == 1
        assert _lib.EXT_SIGNATURES[name] == hdr.functions[name][1] == args, name
        assert name not in _lib.SIGNATURES and name not in _lib.OTHER and name not in lib._mmvid_missing
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    assert ENTRIES['mmvid_adam_step_decoupled'] == _lib.EXT_SIGNATURES['mmvid_adam_step_guarded']
    assert _lib.ABI_VERSION == 3 == lib.mmvid_abi_version()
    # each entry's comment cites the reference lines it replaces
    for cite in ('utils_train.py:173-179', 'utils_train.py:332-343', 'utils_train.py:345-356', 'utils_train.py:358-371', 'utils_train.py:315-330',
                 'train.py:373-374'):
        assert cite in text, cite


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Through _lib.call with made-up addresses: the checks come before the launch, so nothing is ever dereferenced."""
    from mmvid_amd import _lib
    V = ctypes.c_void_p
    a, b, c, d, e, f = (V(k << 20) for k in range(1, 7))
    nan, inf = float('nan'), float('inf')

    def adam(p=a, g=b, m=c, v=d, n=1000, step=1, wd=0.0, flags=None, lo=0, rows=0, rowlen=0, skip=e):
        _lib.call('mmvid_adam_step_decoupled', p, g, m, v, None, n, 1e-3, None, 0.9, 0.95, 1e-8, wd, step, None, 1.0, None, 1.0, flags, lo,
                  rows, rowlen, skip, None)

    for kw, word in ((dict(skip=V((5 << 20) + 2)), 'skip_dev'), (dict(p=None), 'bad arguments'), (dict(g=None), 'bad arguments'),
                     (dict(m=None), 'bad arguments'), (dict(v=None), 'bad arguments'), (dict(n=-1), 'bad arguments'),
                     (dict(step=0), 'bad arguments'), (dict(p=V((1 << 20) + 4)), 'aligned'),
                     (dict(flags=f, lo=8, rows=5, rowlen=12, wd=0.1), 'weight decay'), (dict(flags=f, lo=8, rows=5, rowlen=10), 'lazy'),
                     (dict(flags=f, lo=8, rows=5, rowlen=12, n=67), 'lazy'), (dict(flags=f, lo=0, rows=1 << 62, rowlen=4), 'lazy'),
                     (dict(wd=-0.01), 'weight_decay'), (dict(wd=nan), 'weight_decay'), (dict(wd=inf), 'weight_decay')):
        with pytest.raises(_lib.MMVIDError, match=word):
            adam(**kw)
    adam(n=0)  # nothing to update: no launch, no error
    adam(n=0, skip=None, wd=0.1)

    def ext(sdev=a, kind=3, every=1, A=7, B=0, gamma=0.5, out=b):
        _lib.call('mmvid_lr_schedule_ext', sdev, kind, 1e-6, 1e-4, every, A, B, gamma, out, None)

    for kw, word in ((dict(sdev=None), 'null'), (dict(out=None), 'null'), (dict(out=V((2 << 20) + 2)), 'aligned'), (dict(kind=0), 'kind'),
                     (dict(kind=1), 'kind'), (dict(kind=5), 'kind'), (dict(kind=-1), 'kind'), (dict(every=0), 'every'), (dict(A=0), 'a ='),
                     (dict(A=-3), 'a ='), (dict(A=(1 << 24) + 1), 'a ='), (dict(kind=4, A=8, B=7), 'total'),
                     (dict(kind=4, A=8, B=(1 << 24) + 1), 'total'), (dict(kind=2, gamma=0.0), 'gamma'), (dict(kind=2, gamma=1.5), 'gamma'),
                     (dict(kind=2, gamma=-0.5), 'gamma'), (dict(kind=2, gamma=nan), 'gamma')):
        with pytest.raises(_lib.MMVIDError, match=word):
            ext(**kw)

    def plateau(loss=a, sdev=b, every=1, factor=0.5, patience=2, cooldown=5, threshold=1e-4, min_lr=1e-6, eps=1e-8, sf=c, si=d, skip=e):
        _lib.call('mmvid_lr_plateau', loss, sdev, every, factor, patience, cooldown, threshold, min_lr, eps, sf, si, skip, None)

    for kw, word in ((dict(loss=None), 'NULL'), (dict(sdev=None), 'NULL'), (dict(sf=None), 'NULL'), (dict(si=None), 'NULL'),
                     (dict(skip=V((5 << 20) + 2)), 'aligned'), (dict(sf=V((3 << 20) + 1)), 'aligned'), (dict(every=0), 'every'),
                     (dict(factor=1.0), 'factor'), (dict(factor=0.0), 'factor'), (dict(factor=nan), 'factor'), (dict(patience=-1), 'patience'),
                     (dict(cooldown=-1), 'cooldown'), (dict(threshold=-0.1), 'threshold'), (dict(threshold=1.0), 'threshold'),
                     (dict(threshold=nan), 'threshold'), (dict(min_lr=-1e-6), 'min_lr'), (dict(min_lr=inf), 'min_lr'), (dict(eps=-1e-8), 'eps'),
                     (dict(eps=nan), 'eps')):
        with pytest.raises(_lib.MMVIDError, match=word):
            plateau(**kw)


def test_ops_wrappers_check_their_arguments():
    from mmvid_amd import _lib, ops
    z = torch.zeros(4)
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.lr_schedule_ext(z[:1], 3, 1e-6, 1e-4, 1, 7, 0, 1.0, z[1:2])
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.lr_plateau(z[:1], z[1:2], 1, 0.5, 2, 5, 1e-4, 1e-6, 1e-8, z[2:4], torch.zeros(3, dtype=torch.int32))
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.adam_step(z, z, z, z, None, 1, 1e-3, decoupled=True)
    assert (ops.LR_STEP, ops.LR_COSINE, ops.LR_WARMUP_DECAY) == (S.KIND_STEP, S.KIND_COSINE, S.KIND_WARMUP_DECAY) == (2, 3, 4)


# ------------------------------------------------------------------------------------------------------------ the CPU trainer
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return tiny_bert()


def trainer(model, **kw):
    from mmvid_amd.engine import FlatTrainer, backward_order
    return FlatTrainer(model, order=backward_order, **kw)


def test_trainer_refusals(model, monkeypatch):
    from mmvid_amd import engine as E
    for bad in (1, 0, None, 'yes', np.bool_(True)):
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            trainer(model, decoupled_weight_decay=bad)
    for bad in (-0.01, float('nan'), float('inf'), '0.1', True):
        for dec in (False, True):
            with pytest.raises(ValueError, match='weight_decay'):
                trainer(model, weight_decay=bad, decoupled_weight_decay=dec)
    with pytest.raises(ValueError, match='telemetry'):
        trainer(model, decoupled_weight_decay=True, weight_decay=0.01, telemetry_every=2)
    with pytest.raises(ValueError, match='host trainer'):
        trainer(model, lr_schedule=E.ReduceLROnPlateau(1e-4))
    # a process group of two ranks (stood in for: the refusal comes before anything touches the group)
    monkeypatch.setattr(E.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(E.dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(ValueError, match='more than one rank'):
        trainer(model, lr_schedule=E.ReduceLROnPlateau(1e-4))
    monkeypatch.undo()
    # what stays allowed
    assert trainer(model).decoupled is False and trainer(model, weight_decay=0.01).wd == 0.01
    tr = trainer(model, lr_schedule=E.CosineAnnealingLR(1e-4, 7), **E.optimizer_kwargs('adamw', 0.01))
    assert tr.decoupled is True and tr.betas == (0.9, 0.95) and tr.wd == 0.01 and tr.plateau_f is None and tr.plateau_i is None


def test_state_dict_keys_without_and_with_the_keywords(model):
    from mmvid_amd import engine as E
    group_keys = ['amsgrad', 'betas', 'eps', 'lr', 'params', 'weight_decay']
    for kw in ({}, dict(weight_decay=0.01), dict(lr_schedule=E.WarmupLR(1e-6, 1e-4, 10)), dict(lr_schedule=E.StepLR(1e-4, 3)),
               dict(lr_schedule=E.CosineAnnealingLR(1e-4, 7)), dict(lr_schedule=E.WarmupDecayLR(40, 1e-6, 1e-4, 8))):
        sd = trainer(model, **kw).state_dict()
        assert sorted(map(str, sd)) == ['frontend', 'names', 'param_groups', 'state'], kw
        assert len(sd['param_groups']) == 1 and sorted(sd['param_groups'][0]) == group_keys, kw
        assert all(sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in sd['state'].values())
    sd = trainer(model, decoupled_weight_decay=True, weight_decay=0.01).state_dict()
    assert sorted(map(str, sd)) == ['frontend', 'names', 'param_groups', 'state']
    assert sorted(sd['param_groups'][0]) == sorted(group_keys + ['decoupled_weight_decay']) and sd['param_groups'][0]['decoupled_weight_decay'] is True


def test_adamw_checkpoint_of_torch_loads_and_the_flag_must_agree(model):
    """torch.optim.AdamW over the reference's parameter order (utils_train.py:173-179), one step on the CPU, its state_dict() loaded:
    the moments land on the parameters of the same name, and the flag torch saves is held against the constructor's."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    gen = torch.Generator().manual_seed(3)
    clones = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    for q in clones:
        q.grad = torch.randn(q.shape, generator=gen) * 1e-3
    opt = torch.optim.AdamW(clones, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01)
    opt.step()
    sd = opt.state_dict()
    assert sd['param_groups'][0].get('decoupled_weight_decay') is True and 'names' not in sd
    tr = trainer(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, decoupled_weight_decay=True)
    tr.load_state_dict(sd)
    assert tr.step_count == 1 and tr.betas == (0.9, 0.95) and tr.wd == 0.01
    for j, (n, _) in enumerate(named):
        i = tr.names.index(n)
        assert torch.equal(tr._view(tr.M, i), sd['state'][j]['exp_avg']) and torch.equal(tr._view(tr.V, i), sd['state'][j]['exp_avg_sq']), n
    assert float(tr.M.abs().max()) > 0
    again = trainer(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.01, decoupled_weight_decay=True)
    again.load_state_dict(tr.state_dict())  # and its own
    assert torch.equal(again.M, tr.M) and torch.equal(again.V, tr.V)
    with pytest.raises(ValueError, match='decoupled_weight_decay'):
        trainer(model, weight_decay=0.01).load_state_dict(sd)
    adam_sd = trainer(model, weight_decay=0.01).state_dict()
    with pytest.raises(ValueError, match='decoupled_weight_decay'):
        tr.load_state_dict(adam_sd)
    trainer(model, weight_decay=0.01).load_state_dict(adam_sd)
