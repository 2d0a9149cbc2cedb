"""Classifier-free guidance on the device: the guided token race (csrc/sample.hip) against the unguided kernel on the torch-composed
logits and against oracle.sampling, the guided sampler against the unguided one (scale 0) and against a step-by-step restatement,
`given` under guidance, the public path's unconditional control, and the training-side condition drop (csrc/frontend.hip) with
injected and with free-running decisions.  Every comparison of tokens, masks, losses and gradients is an equality."""
import copy

import numpy as np
import pytest
import torch

import mmvid_amd
from guarded import Guarded, call_abi, report_mismatch
from test_host_logic import tiny_vae

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG_INF = float('-inf')
T, N_TOK, FMAP, SIZE = 2, 16, 4, 64  # config 1 of the survey: 2 frames of 64 x 64, a 4 x 4 token grid, codebook 256
TS = T * N_TOK
STEPS, NB, BEAMS = 4, 3, 2  # refinement steps, videos, candidates per video
SCALES = (0.0, 0.5, 3.0, -1.0)


# ------------------------------------------------------------------------------------------------- helpers (copied, unchanged)
class Recorder:
    """A `_race` that draws from the device generator and keeps what it drew, by name (tests/test_long_video_gpu.py)."""

    def __init__(self):
        self.drawn = {}

    def __call__(self, name, shape):
        assert name not in self.drawn
        t = torch.rand(shape, device=DEV) if name.endswith('_noise_u') else torch.empty(shape, device=DEV).exponential_()
        self.drawn[name] = t
        return t


def replay(drawn):
    """A `_race` that hands back recorded variates (tests/test_completion_gpu.py)."""
    def race(name, shape):
        got = drawn[name]
        assert tuple(got.shape) == tuple(shape), (name, tuple(got.shape), tuple(shape))
        return got
    return race


def build_model(num_visuals=0, seed=20):
    from mmvid_amd.dalle_bert import BERT
    torch.manual_seed(seed)
    m = BERT(dim=768, vae=tiny_vae(), cvae=tiny_vae() if num_visuals else None, num_text_tokens=49408, text_seq_len=16,
             which_transformer='openai_clip_visual', num_visuals=num_visuals, num_targets=T, transformer_layers=2)
    return m.to(DEV).eval()


# ---------------------------------------------------------------------------------------------------------- 1-3. the kernel
CASES = {  # R, V, rows_per_scale, temperature, logit_div
    'odd': (7, 100, 1, 0.0, 1.0),  # V no multiple of 64, R no multiple of the 4 rows of a block
    'noise': (12, 1024, 3, 0.7, 1.0),  # a scale group across a block boundary, Gumbel noise on
    'divisor': (8, 1088, 4, 0.0, 0.5),  # the divisor form
}


def race_case(name):
    """-> dict of device tensors: lc (every seventh column -inf), lu, the scales of the groups (all four values where there are
    four groups, 0 and -1 first: the two at which lc == -inf would give NaN), w per row, E, noise_u | None."""
    R, V, rps, temp, div = CASES[name]
    gen = torch.Generator().manual_seed(7000 + R * V)
    lc = torch.randn(R, V, generator=gen) * 3
    lc[:, ::7] = NEG_INF
    lu = torch.randn(R, V, generator=gen) * 3
    groups = R // rps
    scale = torch.tensor([SCALES[(0, 3, 2, 1)[i % 4]] for i in range(groups)])
    E = torch.empty(R, V).exponential_(generator=gen)
    u = torch.rand(R, V, generator=gen) if temp else None
    to = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return dict(R=R, V=V, rps=rps, temp=temp, div=div, lc=to(lc), lu=to(lu), scale=to(scale), w=to(scale.repeat_interleave(rps)),
                E=to(E), u=to(u))


def composed(lc, lu, w):
    """lc + w * (lc - lu) as three elementwise tensor operations on the device, each rounded to fp32; where the conditional branch
    rules a class out it stays ruled out (w <= 0 would make the three operations give NaN there)."""
    d = lc - lu
    m = w.view(-1, 1) * d
    g = lc + m
    return torch.where(lc == NEG_INF, lc, g)


@pytest.mark.parametrize('name', list(CASES))
def test_guided_race_equals_the_plain_race_on_composed_logits(name):
    from mmvid_amd import ops
    c = race_case(name)
    g = composed(c['lc'], c['lu'], c['w'])
    assert not bool(torch.isnan(g).any()) and bool((g[:, ::7] == NEG_INF).all())
    want_tok, want_y = ops.sample_race(g, c['E'], c['u'], c['temp'], logit_div=c['div'])
    tok, y = ops.sample_race_guided(c['lc'], c['lu'], c['scale'], c['rps'], c['E'], c['u'], c['temp'], logit_div=c['div'])
    report_mismatch(tok.cpu(), want_tok.cpu(), f'{name}: tokens, guided kernel against the plain kernel on lc + w (lc - lu)')
    report_mismatch(y.cpu(), want_y.cpu(), f'{name}: y, guided kernel against the plain kernel on lc + w (lc - lu)')
    assert torch.equal(tok, want_tok) and torch.equal(y, want_y)
    assert bool((tok % 7 != 0).all()), 'a token landed on a class the conditional branch rules out'
    assert bool(torch.isfinite(y).all()) and bool((y > 0).all())
    assert len(set(c['scale'].tolist())) == min(4, c['R'] // c['rps'])


def test_guided_race_on_a_strided_view_through_guarded_buffers():
    """ld > V: both logit tensors are windows of wider buffers whose other elements are NaN (a read outside the window shows in y or
    moves a token), and tok / y are windows behind which nothing may be stored."""
    from mmvid_amd import ops
    c = race_case('noise')
    R, V, ld = c['R'], c['V'], c['V'] + 192
    g = composed(c['lc'], c['lu'], c['w'])
    want_tok, want_y = ops.sample_race(g, c['E'], c['u'], c['temp'])
    glc, glu = Guarded(c['lc'].cpu(), role='in', ld=ld), Guarded(c['lu'].cpu(), role='in', ld=ld)
    gs, gE, gu = Guarded(c['scale'].cpu(), role='in'), Guarded(c['E'].cpu(), role='in'), Guarded(c['u'].cpu(), role='in')
    gtok, gy = Guarded(role='out', shape=(R, ), dtype=torch.int64), Guarded(role='out', shape=(R, ), dtype=torch.float32)
    call_abi('mmvid_sample_race_guided', glc.ptr, glu.ptr, ld, gs.ptr, c['rps'], gE.ptr, gu.ptr, c['temp'], 1.0, R, V, 0, gtok.ptr, gy.ptr)
    for gb, what in ((glc, 'logits_c'), (glu, 'logits_u'), (gs, 'scale'), (gE, 'E'), (gu, 'noise_u')):
        gb.check(f'sample_race_guided {what}')
    report_mismatch(gtok.check('sample_race_guided tok'), want_tok.cpu(), 'strided: tokens')
    report_mismatch(gy.check('sample_race_guided y'), want_y.cpu(), 'strided: y')
    # and through ops on views of wider tensors
    wide_c, wide_u = torch.full((R, ld), float('nan'), device=DEV), torch.full((R, ld), float('nan'), device=DEV)
    wide_c[:, 64:64 + V], wide_u[:, 64:64 + V] = c['lc'], c['lu']
    tok, y = ops.sample_race_guided(wide_c[:, 64:64 + V], wide_u[:, 64:64 + V], c['scale'], c['rps'], c['E'], c['u'], c['temp'])
    assert torch.equal(tok, want_tok) and torch.equal(y, want_y)
    with pytest.raises(ValueError, match='row stride'):
        ops.sample_race_guided(wide_c[:, 64:64 + V], c['lu'], c['scale'], c['rps'], c['E'], c['u'], c['temp'])
    with pytest.raises(ValueError, match='scales'):
        ops.sample_race_guided(c['lc'], c['lu'], c['scale'][:-1].contiguous(), c['rps'], c['E'], c['u'], c['temp'])
    with pytest.raises(ValueError, match='scales'):
        ops.sample_race_guided(c['lc'], c['lu'], c['scale'], 5, c['E'], c['u'], c['temp'])  # 12 rows are no multiple of 5


@pytest.mark.filterwarnings('ignore:overflow encountered in divide')  # (E / P of a class far below the maximum is inf on both sides)
@pytest.mark.parametrize('name', ['odd', 'noise'])
def test_guided_race_matches_the_oracle(name):
    from mmvid_amd import ops
    from oracle import sampling as S
    c = race_case(name)
    g = composed(c['lc'], c['lu'], c['w'])
    tok, y = ops.sample_race_guided(c['lc'], c['lu'], c['scale'], c['rps'], c['E'], c['u'], c['temp'])
    otok, oy, _ = S.token_race(g, c['E'], c['temp'], c['u'])
    assert np.array_equal(tok.cpu().numpy(), otok), name
    assert np.allclose(y.cpu().numpy(), oy, rtol=2e-6, atol=1e-12)


@pytest.mark.parametrize('name', list(CASES))
def test_scale_zero_is_the_unguided_kernel(name):
    from mmvid_amd import ops
    c = race_case(name)
    zero = torch.zeros_like(c['scale'])
    want_tok, want_y = ops.sample_race(c['lc'], c['E'], c['u'], c['temp'], logit_div=c['div'])
    tok, y = ops.sample_race_guided(c['lc'], c['lu'], zero, c['rps'], c['E'], c['u'], c['temp'], logit_div=c['div'])
    assert torch.equal(tok, want_tok) and torch.equal(y, want_y)


# ------------------------------------------------------------------------------------------------------------ the sampler
@pytest.fixture(scope='module')
def model():
    return build_model()


@pytest.fixture(scope='module')
def mp(golden):
    return dict(golden('mask_predict').meta['mp_config'], B=BEAMS)


@pytest.fixture(scope='module')
def controls(model):
    """Text and control of NB videos, and an unconditional control of the same shape.  The sampler takes any [b, csl, E]: this one is
    the all-pad text's with its text rows replaced by noise of four times their spread, because a freshly initialised tower hardly
    reads its control and the tests below want the two branches' logits to differ by more than a rounding."""
    gen = torch.Generator().manual_seed(41)
    text = torch.randint(1, 49408, (NB, 16), generator=gen)
    text[0, 9:] = 0
    text = text.to(DEV)
    with torch.no_grad():
        control = model(text, return_loss=False)
        uncond = model(torch.zeros_like(text), return_loss=False)
    noise = torch.randn(uncond[:, 1:17].shape, generator=gen).to(DEV)
    uncond[:, 1:17] = noise * 4 * float(control.std())
    return text, control, uncond.contiguous()


@pytest.fixture(scope='module')
def unguided(model, mp, controls):
    """One unguided run with recorded variates and its trace, shared by the tests below (and left unchanged by them)."""
    _, control, _ = controls
    rec, trace = Recorder(), []
    seq = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, _race=rec, _trace=trace)[0]
    return dict(seq=seq, drawn=rec.drawn, trace=trace)


def test_sampler_at_scale_zero_is_the_unguided_sampler(model, mp, controls, unguided):
    _, control, uncond = controls
    assert not torch.equal(control, uncond)
    trace = []
    seq = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, _race=replay(unguided['drawn']), _trace=trace,
                             uncond_emb=uncond, guidance_scale=0.0)[0]
    report_mismatch(seq.cpu(), unguided['seq'].cpu(), 'scale 0: tokens')
    assert len(trace) == len(unguided['trace']) == STEPS
    for got, want in zip(trace, unguided['trace']):
        for key in ('Y', 'I_tok') + (('mask1', ) if got['t'] else ()):
            report_mismatch(got[key].cpu(), want[key].cpu(), f'scale 0, step {got["t"]}, {key}')
        report_mismatch(got['logits'].cpu(), want['logits'].cpu(), f'scale 0, step {got["t"]}: the conditional logits')
        assert not torch.equal(got['logits_u'], got['logits']) and 'logits_u' not in want


@pytest.fixture(scope='module')
def guided(model, mp, controls, unguided):
    """One guided run on the unguided run's variates: a scale per step and video, all distinct, video 1 at 0 throughout."""
    _, control, uncond = controls
    scale = torch.tensor([[8.0 + 2.0 * t + 0.5 * i for i in range(NB)] for t in range(STEPS)])
    scale[:, 1] = 0.0
    scale[2, 2] = -6.5
    trace = []
    seq = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, _race=replay(unguided['drawn']), _trace=trace,
                             uncond_emb=uncond, guidance_scale=scale.to(DEV))[0]
    return dict(seq=seq, trace=trace, scale=scale)


def test_sampler_against_a_step_by_step_restatement(mp, unguided, guided):
    """Every step's tokens recomputed by oracle.sampling.token_race from the step's recorded logits of both branches, its scale row and
    its variates; video i's candidates (rows i * BEAMS * TS .. of the step) read scale [t, i]."""
    from mmvid_amd import sampling
    from oracle import sampling as S
    temp = sampling.schedule(mp, TS)[1]
    scale, drawn = guided['scale'], unguided['drawn']
    assert len(guided['trace']) == STEPS
    moved = 0
    for rec in guided['trace']:
        t = rec['t']
        nb = 1 if t == 0 else BEAMS
        report_mismatch(rec['scale'].cpu(), scale[t], f'step {t}: the scale row')
        w = scale[t].to(DEV).repeat_interleave(nb * TS)
        assert tuple(rec['logits'].shape) == tuple(rec['logits_u'].shape) == (NB * nb * TS, 256)
        g = composed(rec['logits'], rec['logits_u'], w)
        u = drawn.get(f'tok{t}_noise_u') if temp[t] != 0.0 else None
        otok, _, _ = S.token_race(g, rec['E_tok'], temp[t], u)
        got = (rec['I_tok'] if t == 0 else rec['Inew']).reshape(-1).cpu().numpy()
        assert np.array_equal(got, otok), f'step {t}: {(got != otok).sum()} of {got.size} tokens differ from the restatement'
        # (what the restatement can tell apart: the tokens that a scale of 0 on every row would have given)
        flat, _, _ = S.token_race(rec['logits'], rec['E_tok'], temp[t], u)
        moved += int((got != flat).sum())
        print(f'step {t}: guidance moved {int((got != flat).sum())} of {got.size} tokens; max |lc - lu| = '
              f'{float((rec["logits"] - rec["logits_u"]).abs().max()):.3g}, max |lc| = {float(rec["logits"].abs().max()):.3g}')
    assert moved > 0, 'guidance moved no token at any step: the restatement above told nothing apart'
    # the video at scale 0 is the unguided call's, at every step; the others are not
    for got, want in zip(guided['trace'], unguided['trace']):
        assert torch.equal(got['I_tok'][1], want['I_tok'][1]) and torch.equal(got['Y'][1], want['Y'][1]), f'step {got["t"]}'
    assert torch.equal(guided['seq'][1], unguided['seq'][1])
    differ = [not torch.equal(guided['seq'][i], unguided['seq'][i]) for i in range(NB)]
    assert differ == [True, False, True], differ
    assert 0 <= int(guided['seq'].min()) and int(guided['seq'].max()) < 256


def test_given_with_guidance(model, mp, controls):
    _, control, uncond = controls
    gen = torch.Generator().manual_seed(42)
    tokens = torch.randint(0, 256, (NB, TS), generator=gen).to(DEV)
    mask = torch.zeros(NB, TS, dtype=torch.uint8, device=DEV)
    mask[:, :N_TOK] = 1  # the first frame is given
    known = mask.bool()
    rec = Recorder()
    plain = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, given=(mask, tokens), _race=rec)[0]
    zero = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, given=(mask, tokens), _race=replay(rec.drawn),
                              uncond_emb=uncond, guidance_scale=0.0)[0]
    assert torch.equal(zero, plain)
    trace = []
    seq = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, given=(mask, tokens), _race=replay(rec.drawn),
                             _trace=trace, uncond_emb=uncond, guidance_scale=[16.0, 12.0, 8.0, 4.0])[0]
    assert torch.equal(seq[known], tokens[known])
    assert not torch.equal(seq, plain)  # (guidance did something to the unknown positions)
    for r in trace:
        assert torch.equal(r['I_tok'][known], tokens[known]), f'step {r["t"]}: a given token changed'
        assert torch.equal(r['scale'].cpu(), torch.full((NB, ), [16.0, 12.0, 8.0, 4.0][r['t']]))


# ---------------------------------------------------------------------------------------------------------- 7. the public path
def test_generate_images_builds_the_unconditional_control(monkeypatch, mp):
    from mmvid_amd import sampling
    model = build_model(num_visuals=1, seed=23)
    gen = torch.Generator().manual_seed(43)
    text = torch.randint(1, 49408, (2, 16), generator=gen).to(DEV)
    t2 = torch.randint(1, 49408, (2, 16), generator=gen).to(DEV)
    visual = torch.rand(2, 1, 3, SIZE, SIZE, generator=gen).to(DEV)
    seen = []
    inner = sampling.mask_predict

    def spy(model, control_emb, **kw):
        seen.append((control_emb, kw.get('uncond_emb'), kw.get('guidance_scale')))
        return inner(model, control_emb, **kw)

    monkeypatch.setattr(sampling, 'mask_predict', spy)
    with torch.no_grad():
        want_cond = model(text, visual=visual, return_loss=False)
        want_null_visual = model(text, visual=None, return_loss=False)
        want_negative = model(t2, visual=visual, return_loss=False)
        want_all = model(torch.zeros_like(text), visual=None, return_loss=False)
    kw = dict(visual=visual, mask_predict_steps=STEPS, mp_config=mp, dynamic=False)
    images, _, seq = model.generate_images(text, guidance_scale=2.0, guidance_drop=('visual', ), **kw)
    assert images.shape == (2, T, 3, SIZE, SIZE) and seq.shape == (2 * T, N_TOK)
    model.generate_images(text, guidance_scale=2.0, guidance_drop=(), negative_text=t2, **kw)
    model.generate_images(text, guidance_scale=2.0, **kw)  # the default: both dropped
    model.generate_images(text, **kw)  # unguided: the sampler gets no second control
    assert len(seen) == 4
    for (cond, uncond, scale), want in zip(seen, (want_null_visual, want_negative, want_all, None)):
        assert torch.equal(cond, want_cond)
        if want is None:
            assert uncond is None and scale is None
        else:
            assert scale == 2.0 and uncond.shape == cond.shape and torch.equal(uncond, want)
    assert not torch.equal(want_null_visual, want_cond) and not torch.equal(want_negative, want_cond)


# ------------------------------------------------------------------------------------------------- 8-9. the condition drop
def _cond_drop(text, vis, p_text, p_visual, inject, mask_id, state):
    """mmvid_cond_drop on guarded and poisoned buffers -> (text_out, vis_out | None, decided) on the host."""
    B, Tt = text.shape
    Vs = 0 if vis is None else vis.shape[1]
    gt = Guarded(text, role='in')
    gv = None if vis is None else Guarded(vis, role='in')
    gi = None if inject is None else Guarded(inject, role='in')
    gto = Guarded(role='out', shape=(B, Tt), dtype=torch.int64)
    gvo = None if vis is None else Guarded(role='out', shape=(B, Vs), dtype=torch.int64)
    gd = Guarded(role='out', shape=(B, 2), dtype=torch.uint8)
    import ctypes
    call_abi('mmvid_cond_drop', gt.ptr, None if gv is None else gv.ptr, B, Tt, Vs, ctypes.c_void_p(state.data_ptr()), 0, p_text, p_visual,
             None if gi is None else gi.ptr, mask_id, gto.ptr, None if gvo is None else gvo.ptr, gd.ptr)
    for g, what in ((gt, 'text'), (gv, 'vis_tok'), (gi, 'inject')):
        if g is not None:
            g.check(f'cond_drop {what}')
    return gto.check('cond_drop text_out'), None if gvo is None else gvo.check('cond_drop vis_out'), gd.check('cond_drop decided')


def _state(seed, step):
    from mmvid_amd.frontend import Frontend
    fe = Frontend(seed=seed)
    fe._state(DEV)[0:1].fill_(float(step))
    return fe


def test_condition_drop_injected_and_boundary_cases():
    B, Tt, Vs, MASK = 6, 8, 5, 256
    gen = torch.Generator().manual_seed(44)
    text = torch.randint(1, 49408, (B, Tt), generator=gen)
    text[2, 5:] = 0
    vis = torch.randint(0, 256, (B, Vs), generator=gen)
    inject = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1], [0, 1], [1, 0]], dtype=torch.uint8)
    state = _state(5, 0).state
    # p = 1 with an injection: the injection decides
    t_out, v_out, decided = _cond_drop(text, vis, 1.0, 1.0, inject, MASK, state)
    assert torch.equal(decided, inject)
    assert torch.equal(t_out, torch.where(inject[:, :1].bool(), torch.zeros_like(text), text))
    assert torch.equal(v_out, torch.where(inject[:, 1:].bool(), torch.full_like(vis, MASK), vis))
    # p = 0 drops nothing, p = 1 everything
    t_out, v_out, decided = _cond_drop(text, vis, 0.0, 0.0, None, MASK, state)
    assert int(decided.sum()) == 0 and torch.equal(t_out, text) and torch.equal(v_out, vis)
    t_out, v_out, decided = _cond_drop(text, vis, 1.0, 1.0, None, MASK, state)
    assert int(decided.min()) == 1 and int(t_out.abs().max()) == 0 and bool((v_out == MASK).all())
    t_out, v_out, decided = _cond_drop(text, vis, 1.0, 0.0, None, MASK, state)
    assert decided.tolist() == [[1, 0]] * B and int(t_out.abs().max()) == 0 and torch.equal(v_out, vis)
    # no visual control: the visual half is a no-op (nothing to store), the text half as before
    t_out, v_out, decided = _cond_drop(text, None, 0.0, 0.0, inject, MASK, state)
    assert v_out is None and torch.equal(decided, inject)
    assert torch.equal(t_out, torch.where(inject[:, :1].bool(), torch.zeros_like(text), text))
    # the wrapper: new tensors, the inputs untouched, the decisions kept
    fe = _state(5, 0)
    td, vd = text.to(DEV), vis.to(DEV)
    t2, v2 = fe.cond_drop(td, vd, 0.3, 0.3, MASK, inject.to(DEV))
    assert torch.equal(td.cpu(), text) and torch.equal(vd.cpu(), vis) and torch.equal(fe.last_null.cpu(), inject)
    assert torch.equal(t2.cpu(), torch.where(inject[:, :1].bool(), torch.zeros_like(text), text))
    assert torch.equal(v2.cpu(), torch.where(inject[:, 1:].bool(), torch.full_like(vis, MASK), vis))
    t3, v3 = fe.cond_drop(td, None, 1.0, 1.0, MASK)
    assert v3 is None and int(t3.abs().max()) == 0
    with pytest.raises(ValueError, match=r'\[B, 2\]'):
        fe.cond_drop(td, vd, 0.3, 0.3, MASK, inject[:3].to(DEV))


def test_condition_drop_free_running_draws():
    B, Tt, Vs, MASK = 4096, 8, 5, 256
    gen = torch.Generator().manual_seed(45)
    text = torch.randint(1, 49408, (B, Tt), generator=gen).to(DEV)
    vis = torch.randint(0, 256, (B, Vs), generator=gen).to(DEV)

    def run(seed, step, p_text=0.1, p_visual=0.3):
        fe = _state(seed, step)
        t_out, v_out = fe.cond_drop(text, vis, p_text, p_visual, MASK)
        d = fe.last_null.bool()
        assert torch.equal(t_out, torch.where(d[:, :1], torch.zeros_like(text), text))
        assert torch.equal(v_out, torch.where(d[:, 1:], torch.full_like(vis, MASK), vis))
        return fe.last_null.cpu()

    first = run(9, 3)
    assert torch.equal(run(9, 3), first)  # same seed and step
    assert not torch.equal(run(9, 4), first)  # the next step
    assert not torch.equal(run(10, 3), first)  # another seed
    # binomial counts within 6 sigma: 410 +- 115 and 1229 +- 176
    for col, p in ((0, 0.1), (1, 0.3)):
        n, sigma = int(first[:, col].sum()), (B * p * (1 - p)) ** 0.5
        print(f'column {col}: {n} of {B} dropped at p = {p} (expected {B * p:.0f} +- {6 * sigma:.0f})')
        assert abs(n - B * p) <= 6 * sigma
    assert not torch.equal(first[:, 0], first[:, 1])
    # the two streams are their own: at equal probabilities the columns still differ
    same_p = run(9, 3, 0.3, 0.3)
    assert not torch.equal(same_p[:, 0], same_p[:, 1]) and torch.equal(same_p[:, 1], first[:, 1])


# ------------------------------------------------------------------------------------------------------ 10. the training forward
def _train_case():
    B = 4
    base = build_model(num_visuals=1, seed=24).train()
    gen = torch.Generator().manual_seed(46)
    text = torch.randint(1, 49408, (B, 16), generator=gen)
    text[0, 10:] = 0
    vis = torch.randint(0, 256, (B, base.visual_seq_len), generator=gen)
    target = torch.randint(0, 256, (B, TS), generator=gen)
    warp = torch.randint(0, 256, (B, TS), generator=gen)
    mask1 = (torch.rand(B, TS, generator=gen) < 0.4).to(torch.uint8)
    return base, tuple(t.to(DEV) for t in (text, vis, target, warp, mask1))


def test_training_forward_with_injected_drops_equals_hand_dropped_inputs():
    from mmvid_amd.engine import FlatTrainer, backward_order
    base, (text, vis, target, warp, mask1) = _train_case()
    MASK = base.image_token_lut['[MASK]']
    inj = torch.tensor([[1, 0], [0, 1], [1, 1], [0, 0]], dtype=torch.uint8, device=DEV)
    text_hand = torch.where(inj[:, :1].bool(), torch.zeros_like(text), text)
    vis_hand = torch.where(inj[:, 1:].bool(), torch.full_like(vis, MASK), vis)

    def run(text, vis, **kw):
        m = copy.deepcopy(base)
        m.frontend.seed, m.frontend.step = 77, None
        tr = FlatTrainer(m, lr=1e-4, order=backward_order)
        tr.zero_grad()
        losses = m(text, visual=vis, target=target, return_loss=True, rel=True, vid=True, _mask1=mask1, _target_warp=warp, **kw)
        (7.0 * losses[0] + 0.5 * losses[1] + 0.5 * losses[2]).backward()
        torch.cuda.synchronize()
        return [x.detach().clone() for x in losses], tr.G.clone(), m

    with mmvid_amd.deterministic():
        want_l, want_g, _ = run(text_hand, vis_hand)
        got_l, got_g, m = run(text, vis, null_text_prob=0.5, null_visual_prob=0.5, _null=inj)
        plain_l, plain_g, m0 = run(text, vis)
    assert torch.equal(m.frontend.last_null, inj) and m0.frontend.last_null is None
    for name, a, b in zip(('msm', 'rel', 'vid'), got_l, want_l):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f'loss {name}: {a.item()!r} vs {b.item()!r}'
    report_mismatch(got_g.cpu(), want_g.cpu(), 'flat gradient, injected drop against hand-dropped inputs')
    assert float(got_g.abs().max()) > 0
    assert not torch.equal(plain_l[0], got_l[0]) and not torch.equal(plain_g, got_g)  # (the drop did something)


def test_the_new_streams_disturb_no_existing_decision():
    """Free-running draws, equal seed and step: the MSM masks (and the VID negative's tokens) of a forward with null_text_prob = 0.3 are
    those of a forward with 0."""
    base, (text, vis, target, _, _) = _train_case()
    kept = []
    for p in (0.0, 0.3):
        base.frontend.seed, base.frontend.step = 78, None
        base._debug_keep = {}
        with torch.no_grad():
            base(text, visual=vis, target=target, return_loss=True, rel=True, vid=True, vid_strategy_prob=[0.5, 0.5, 0.0, 0.0],
                 null_text_prob=p, null_visual_prob=p)
        keep, base._debug_keep = base._debug_keep, None
        kept.append((keep['mask1'].clone(), keep['target_warp'].clone(), keep['ids'].clone(),
                     None if base.frontend.last_null is None else base.frontend.last_null.clone()))
    (mask_a, warp_a, ids_a, null_a), (mask_b, warp_b, ids_b, null_b) = kept
    assert torch.equal(mask_a, mask_b) and torch.equal(warp_a, warp_b)
    assert 0 < int(mask_a.sum()) < mask_a.numel()
    assert null_a is None and null_b is not None  # probability 0: the kernel was not launched at all
    dropped = null_b[:, 0].bool()
    if bool(dropped.any()):  # the ids of the MSM sequence: pad ids where the text was dropped
        pad_base = base.num_text_tokens - base.text_seq_len
        rows = ids_b[:text.shape[0]][dropped][:, 1:1 + base.text_seq_len]
        assert torch.equal(rows, (pad_base + torch.arange(base.text_seq_len, device=DEV)).expand_as(rows))
    else:
        assert torch.equal(ids_a[:, 1:1 + base.text_seq_len], ids_b[:, 1:1 + base.text_seq_len])
