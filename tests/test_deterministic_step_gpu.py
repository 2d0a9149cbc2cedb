"""Deterministic mode, step level: with `mmvid_amd.set_deterministic(True)` a FlatTrainer step gives the same bits twice, a captured
step (GraphedStep) gives the bits of the eagerly launched one, and a run resumed from `model.state_dict()` +
`FlatTrainer.state_dict()` gives the bits of the uninterrupted run -- `torch.equal` on the flat parameters, both Adam moments and
every loss, never a tolerance.  World size 1 (the order of RCCL's reductions is out of scope)."""
import copy

import pytest
import torch

import mmvid_amd
from test_models_gpu import DEV
from test_token_step_gpu import batch, small_bert, unit_frames

pytestmark = pytest.mark.gpu
KW = dict(return_loss=True, rel=True, vid=True, rel_no_fully_masked=True)
SEED = 77


@pytest.fixture(autouse=True)
def deterministic_mode():
    before = mmvid_amd.set_deterministic(True)
    yield
    mmvid_amd.set_deterministic(before)


def make(base, token_path):
    """A fresh model (copy of `base`), its trainer and the step function of the pixel or the token path."""
    from mmvid_amd.engine import FlatTrainer, backward_order
    m = copy.deepcopy(base)
    m.frontend.seed, m.frontend.step = SEED, None
    tr = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order)
    if token_path:
        def fn(text, target, target_frames):
            lm, lr, lv = m(text, target=target, target_frames=target_frames, **KW)
            return 7.0 * lm + 0.5 * lr + 0.5 * lv
    else:
        def fn(text, frames):
            lm, lr, lv = m(text, target=frames, **KW)
            return 7.0 * lm + 0.5 * lr + 0.5 * lv
    return m, tr, fn


def eager(tr, fn, inputs):
    losses = []
    for inp in inputs:
        tr.zero_grad()
        loss = fn(**inp)
        loss.backward()
        tr.step()
        losses.append(loss.detach().clone())
    return losses


def same(a, b, what):
    (ta, la), (tb, lb) = a, b
    for name in ('P', 'M', 'V'):
        x, y = getattr(ta, name), getattr(tb, name)
        assert torch.equal(x, y), f'{what}: {name} differs in {(x != y).sum().item()} of {x.numel()} elements (max {(x - y).abs().max().item():.3e})'
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.isfinite(x).all() and torch.equal(x, y), f'{what}: loss {i}: {x.item()!r} vs {y.item()!r}'


def small_case(token_path, steps=5, B=4, T=2):
    base = small_bert(T)
    tokenizer = copy.deepcopy(base).vae  # (on a copy: a VQGAN that has run holds its plan, and a plan cannot be deep-copied)
    text, _ = batch(B, T)
    inputs = []
    for i in range(steps):
        _, u8 = batch(B, T, seed=10 + i)
        if token_path:
            with torch.no_grad():
                tok = tokenizer.get_codebook_indices(unit_frames(u8).view(B * T, 3, 64, 64)).view(B, -1).contiguous()
            inputs.append(dict(text=text, target=tok, target_frames=u8.to(DEV)))
        else:
            inputs.append(dict(text=text, frames=unit_frames(u8)))
    return base, inputs


@pytest.mark.parametrize('token_path', [False, True], ids=['pixels', 'tokens'])
def test_two_runs_from_one_seed_are_bit_equal(token_path):
    base, inputs = small_case(token_path)
    runs = []
    for _ in range(2):
        m, tr, fn = make(base, token_path)
        runs.append((tr, eager(tr, fn, inputs)))
    same(runs[0], runs[1], 'second run vs first')
    assert runs[0][0].M.abs().max() > 0 and not torch.equal(runs[0][1][0], runs[0][1][-1])


@pytest.mark.parametrize('token_path', [False, True], ids=['pixels', 'tokens'])
def test_graphed_step_equals_eager_step(token_path):
    from mmvid_amd.engine import GraphedStep
    base, inputs = small_case(token_path)
    m, tr, fn = make(base, token_path)
    le = eager(tr, fn, inputs)
    mg, trg, fng = make(base, token_path)
    step = GraphedStep(trg, fng, inputs[0], warmup=1)  # one eager step on inputs[0], then the capture
    assert step.graph is not None, step.capture_error
    assert step.deterministic is True
    lg = [step(**inp).clone() for inp in inputs[1:]]
    same((tr, le[1:]), (trg, lg), 'graphed vs eager')
    assert trg.step_count == tr.step_count == len(inputs)


def test_graphed_step_refuses_the_other_mode():
    from mmvid_amd.engine import GraphedStep
    base, inputs = small_case(False, steps=2)
    m, tr, fn = make(base, False)
    step = GraphedStep(tr, fn, inputs[0], warmup=1)
    assert step.graph is not None, step.capture_error
    before = tr.P.clone()
    with mmvid_amd.deterministic(False):
        with pytest.raises(RuntimeError, match='captured with deterministic=True'):
            step(**inputs[1])
    assert torch.equal(tr.P, before)  # nothing ran
    step(**inputs[1])
    assert not torch.equal(tr.P, before)


@pytest.mark.parametrize('token_path', [False, True], ids=['pixels', 'tokens'])
def test_resumed_run_equals_uninterrupted_run(token_path):
    base, inputs = small_case(token_path)
    m, tr, fn = make(base, token_path)
    whole = eager(tr, fn, inputs)
    m1, tr1, fn1 = make(base, token_path)
    first = eager(tr1, fn1, inputs[:3])
    model_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    opt_sd = copy.deepcopy(tr1.state_dict())
    m2, tr2, fn2 = make(base, token_path)
    m2.frontend.seed = 1  # (the checkpoint must bring the seed and the forward count back)
    m2.load_state_dict(model_sd)
    tr2.refresh_shadows()
    tr2.load_state_dict(opt_sd)
    rest = eager(tr2, fn2, inputs[3:])
    same((tr, whole), (tr2, first + rest), 'resumed vs uninterrupted')
    assert tr2.step_count == 5


def test_config2_full_size_graphed_step_is_bit_equal_to_eager():
    """Config 2 at full size (12 layers, L = 579, per-GPU batch 6), the front-end's own draws, three steps: the exact-equality
    counterpart of test_parity_gpu.py::test_config2_full_size_graphed_step_matches_eager (which accepts 2e-3 in the default mode)."""
    from mmvid_amd.engine import GraphedStep
    from test_parity_gpu import _full_bert
    base = _full_bert(0)
    assert base.total_seq_len == 579
    B = 6
    gen = torch.Generator().manual_seed(1)
    text = torch.randint(1, 49408, (B, 64), generator=gen)
    text[0, 40:] = 0
    inputs = [dict(text=text.to(DEV), frames=torch.rand(B, 8, 3, 128, 128, generator=gen).to(DEV)) for _ in range(3)]
    m, tr, fn = make(base, False)
    le = eager(tr, fn, inputs)
    mg, trg, fng = make(base, False)
    step = GraphedStep(trg, fng, inputs[0], warmup=1)
    assert step.graph is not None, step.capture_error
    lg = [step(**inp).clone() for inp in inputs[1:]]
    print('config 2 full size, deterministic: eager losses', [x.item() for x in le], 'graphed', [x.item() for x in lg])
    same((tr, le[1:]), (trg, lg), 'config 2 graphed vs eager')
    assert torch.equal(tr.G, trg.G)
