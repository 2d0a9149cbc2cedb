"""Truncated sampling on the device: mmvid_logits_truncate (csrc/sample.hip) against the fp64 restatement of its rule
(tests/truncate_ref.py) on guarded, padded and poisoned buffers -- equality for top-k and for every crafted tie, the derived sandwich for
the nucleus -- and the two samplers with the new keywords: every truncated step of a recorded BERT run recomputed from its own logits,
the ART-V production path (pre-drawn variates, captured step) against the eager one."""
import functools

import numpy as np
import pytest
import torch

import truncate_ref as T
from guarded import SENTINEL_BITS, Guarded, bits, call_abi, ptr_of, report_mismatch
from test_guidance_gpu import BEAMS, NB, STEPS, TS, Recorder, build_model, composed, replay
from test_host_logic import tiny_vae

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG_INF = float('-inf')
f32 = torch.float32


# --------------------------------------------------------------------------------------------------------------------- helpers
def run_abi(g, top_k=None, top_p=None, *, div=1.0, pad=24, pad_out=8, lu=None, scale=None, rps=1):
    """One call on guarded buffers: g (and lu) [R, V] with ld = V + pad, out with ld_out = V + pad_out -> (out, kept) on the host."""
    g = torch.as_tensor(g)
    R, V = g.shape
    gl = Guarded(g, role='in', ld=V + pad)
    glu = None if lu is None else Guarded(torch.as_tensor(lu), role='in', ld=V + pad)
    gs = None if scale is None else Guarded(torch.as_tensor(scale), role='in')
    gout = Guarded(role='out', shape=(R, V), dtype=f32, ld=V + pad_out)
    gk = Guarded(role='out', shape=(R, ), dtype=torch.int32)
    call_abi('mmvid_logits_truncate', gl.ptr, ptr_of(glu), V + pad, ptr_of(gs), rps, div, 0 if top_k is None else top_k,
             1.0 if top_p is None else top_p, R, V, gout.ptr, V + pad_out, gk.ptr)
    for gb, what in ((gl, 'logits'), (glu, 'logits_u'), (gs, 'scale')):
        if gb is not None:
            gb.check(f'logits_truncate {what}')
    return gout.check('logits_truncate out'), gk.check('logits_truncate kept')


def assert_output(out, kept, g, keep, what):
    """out == g where `keep`, -inf elsewhere, bit for bit; kept == the number of finite outputs."""
    want = torch.from_numpy(T.truncated(np.asarray(g), keep))
    report_mismatch(out, want, what)
    assert torch.equal(bits(out), bits(want)), f'{what}: a kept value changed its bits (a signed zero)'
    report_mismatch(kept, torch.isfinite(want).sum(1).to(torch.int32), f'{what}: kept')


def randn_rows(R, V, seed, spread=3.0):
    g = spread * torch.randn(R, V, generator=torch.Generator().manual_seed(seed))
    g[:, ::7] = NEG_INF
    return g


# ------------------------------------------------------------------------------------------------------------- 1. top-k
@pytest.mark.parametrize('R,V,k', [(7, 100, 1), (7, 100, 37), (9, 256, 64), (6, 1000, 250), (5, 1024, 1000), (3, 2048, 5), (4, 1, 1)])
def test_top_k_equals_the_rule(R, V, k):
    g = randn_rows(R, V, 6000 + V + k)
    out, kept = run_abi(g, top_k=k)
    assert_output(out, kept, g.numpy(), T.topk_set(g.numpy(), k), f'top-k R={R} V={V} k={k}')
    assert bool((out[:, ::7] == NEG_INF).all()) and int(kept.max()) <= k


# -------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize('row', T.tie_rows(), ids=lambda r: r[0].replace(' ', '_'))
def test_top_k_ties_go_to_the_lower_index(row):
    name, g, k, want = row
    out, kept = run_abi(g.reshape(1, -1), top_k=k)
    assert torch.isfinite(out[0]).nonzero().view(-1).tolist() == want, name
    assert_output(out, kept, g.reshape(1, -1), T.topk_set(g, k).reshape(1, -1), name)
    assert int(kept[0]) == len(want)


# ------------------------------------------------------------------------------------------------------------- 3. top-p
@functools.lru_cache(maxsize=None)
def nucleus_reference(V, p, div):
    g = T.nucleus_input(V)
    return g, T.sandwich(g, p, T.DELTA, div)


def assert_sandwich(out, g, lo, hi, what):
    """Every row: S_lo <= K <= S_hi, K a head of the order, kept values bit-equal, -inf elsewhere -> the share of rows not tight."""
    K = torch.isfinite(out).numpy()
    below, above = (lo & ~K).any(axis=1), (K & ~hi).any(axis=1)
    assert not below.any(), f'{what}: rows {np.flatnonzero(below)[:5]} lack a class of the nucleus at top_p - delta'
    assert not above.any(), f'{what}: rows {np.flatnonzero(above)[:5]} keep a class outside the nucleus at top_p + delta'
    assert T.is_head(g, K).all(), f'{what}: a kept set is no head of the order'
    want = torch.from_numpy(T.truncated(g, K))
    assert torch.equal(bits(out), bits(want)), f'{what}: a kept value differs from its input, or a dropped one is not -inf'
    loose = (lo != hi).any(axis=1)
    assert np.array_equal(K[~loose], lo[~loose])  # (a tight row: equality with the fp64 rule)
    return float(loose.mean())


@pytest.mark.parametrize('V,p,div', T.NUCLEUS_CASES)
def test_top_p_lies_between_the_nuclei_at_the_derived_margin(V, p, div):
    g, (lo, hi) = nucleus_reference(V, p, div)
    out, kept = run_abi(g, top_p=p, div=div)
    loose = assert_sandwich(out, g, lo, hi, f'top-p V={V} p={p} div={div}')
    n = torch.isfinite(out).sum(1)
    print(f'V = {V}, top_p = {p}, logit_div = {div}: {100 * loose:.2f} % of {len(g)} rows not tight; kept {int(n.min())}..{int(n.max())} classes')
    assert loose <= T.MAX_LOOSE_SHARE
    assert torch.equal(kept, n.to(torch.int32))


# --------------------------------------------------------------------------------------------------- 4. top-p ties and edges
def test_top_p_ties_and_edges():
    V = 1024
    gen = torch.Generator().manual_seed(6100)
    base = torch.randn(V, generator=gen)
    four = base.clone()
    peaks = [5, 70, 300, 900]  # four equal maxima, 40 above the rest: P = 1 each, and the fp32 sum of the row is exactly 4
    four[peaks] = float(base.max()) + 40.0
    out, kept = run_abi(four.view(1, V), top_p=0.6)  # M_before = 0, 1, 2 < 2.4 <= 3
    assert torch.isfinite(out[0]).nonzero().view(-1).tolist() == peaks[:3] and int(kept[0]) == 3
    out, kept = run_abi(four.view(1, V), top_p=0.5)  # M_before = 0, 1 < 2.0 <= 2
    assert torch.isfinite(out[0]).nonzero().view(-1).tolist() == peaks[:2] and int(kept[0]) == 2
    # top_p = 1.0 with top_k off copies the row (no mass test), -inf columns included
    g = randn_rows(5, 200, 6101)
    out, kept = run_abi(g, top_p=1.0)
    assert torch.equal(bits(out), bits(g)) and torch.equal(kept, torch.isfinite(g).sum(1).to(torch.int32))
    out, kept = run_abi(g, top_k=200, top_p=1.0)  # top_k == V: off as well
    assert torch.equal(bits(out), bits(g))
    # one dominant class
    dom = base.clone()
    dom[77] += 30.0
    out, kept = run_abi(dom.view(1, V), top_p=0.99)
    assert torch.isfinite(out[0]).nonzero().view(-1).tolist() == [77] and int(kept[0]) == 1
    assert float(out[0, 77]) == float(dom[77])


# ------------------------------------------------------------------------------------------------------- 5. both filters
@pytest.mark.parametrize('V,k,p', [(1024, 12, 0.9), (1024, 3, 0.5), (200, 15, 0.95)])
def test_both_filters_are_the_intersection(V, k, p):
    g = torch.from_numpy(T.nucleus_input(V)[:9])
    out_k, _ = run_abi(g, top_k=k)
    out_p, _ = run_abi(g, top_p=p)
    out, kept = run_abi(g, top_k=k, top_p=p)
    both = torch.isfinite(out_k) & torch.isfinite(out_p)
    want = torch.where(both, g, torch.full_like(g, NEG_INF))
    assert torch.equal(bits(out), bits(want)) and torch.equal(kept, both.sum(1).to(torch.int32))
    n_k, n_p = torch.isfinite(out_k).sum(1), torch.isfinite(out_p).sum(1)
    assert bool((n_k < n_p).any()) and bool((n_p < n_k).any()), 'one filter alone decided every row'


# ------------------------------------------------------------------------------------------------------------ 6. guided
@pytest.mark.parametrize('top_k,top_p', [(17, None), (None, 0.9), (30, 0.8)])
def test_guided_form_is_the_unguided_form_on_composed_logits(top_k, top_p):
    R, V, rps = 12, 1000, 3  # four scale groups of three rows: a group crosses the boundary of a four-row block
    gen = torch.Generator().manual_seed(6200)
    lc, lu = randn_rows(R, V, 6201), 3 * torch.randn(R, V, generator=gen)
    scale = torch.tensor([0.0, -1.0, 3.0, 0.5])
    g = composed(lc.to(DEV), lu.to(DEV), scale.repeat_interleave(rps).to(DEV)).cpu()
    assert not bool(torch.isnan(g).any()) and bool((g[:, ::7] == NEG_INF).all())
    want, want_kept = run_abi(g, top_k, top_p)
    out, kept = run_abi(lc, top_k, top_p, lu=lu, scale=scale, rps=rps)
    assert torch.equal(bits(out), bits(want)) and torch.equal(kept, want_kept)
    assert int(kept.min()) >= 1
    # both filters off: the guided value is copied through
    out, _ = run_abi(lc, lu=lu, scale=scale, rps=rps)
    assert torch.equal(bits(out), bits(g))


# ----------------------------------------------------------------------------------- 7. in place, repeatability, refusals
def test_in_place_and_through_views():
    from mmvid_amd import ops
    g = torch.from_numpy(T.nucleus_input(1024)[:11]).to(DEV)
    for kw in (dict(top_k=12), dict(top_p=0.9), dict(top_k=5, top_p=0.95)):
        want, want_kept = ops.logits_truncate(g, want_kept=True, **kw)
        again = ops.logits_truncate(g, **kw)
        assert torch.equal(bits(again), bits(want))  # two runs
        buf = g.clone()
        got, kept = ops.logits_truncate(buf, out=buf, want_kept=True, **kw)
        assert got is buf and torch.equal(bits(buf), bits(want)) and torch.equal(kept, want_kept)
        host, _ = run_abi(g.cpu(), kw.get('top_k'), kw.get('top_p'))
        assert torch.equal(bits(host), bits(want.cpu()))
        # windows of wider tensors whose other elements are NaN, in and out
        wide = torch.full((11, 1024 + 192), float('nan'), device=DEV)
        wide[:, 64:64 + 1024] = g
        wide_out = torch.full((11, 1024 + 64), float('nan'), device=DEV)
        ops.logits_truncate(wide[:, 64:64 + 1024], out=wide_out[:, 32:32 + 1024], **kw)
        assert torch.equal(bits(wide_out[:, 32:32 + 1024]), bits(want))
        assert bool(torch.isnan(wide_out[:, :32]).all()) and bool(torch.isnan(wide_out[:, 32 + 1024:]).all())
    assert ops.logits_truncate(g[:0], 4).shape == (0, 1024)  # R == 0: nothing launched
    with pytest.raises(ValueError, match='come together'):
        ops.logits_truncate(g, 4, logits_u=g)
    with pytest.raises(ValueError, match='scales'):
        ops.logits_truncate(g, 4, logits_u=g, scale=torch.ones(3, device=DEV), rows_per_scale=3)  # 11 rows are no multiple of 3
    with pytest.raises(ValueError, match='out'):
        ops.logits_truncate(g, 4, out=torch.empty(11, 1000, device=DEV))


def test_every_refusal_leaves_the_output_alone():
    from mmvid_amd import _lib
    R, V = 6, 64
    g = randn_rows(R, V, 6300)
    gl, glu, gs = Guarded(g, role='in'), Guarded(g + 1, role='in'), Guarded(torch.ones(2), role='in')
    gout = Guarded(role='out', shape=(R, V), dtype=f32, partial=True)
    gk = Guarded(role='out', shape=(R, ), dtype=torch.int32, partial=True)
    nan = float('nan')
    ok = dict(logits=gl.ptr, logits_u=None, ld=V, scale=None, rps=1, div=1.0, k=4, p=0.9, R=R, V=V, out=gout.ptr, ld_out=V)
    bad = [dict(V=0), dict(V=2049, ld=2049, ld_out=2049), dict(div=0.0), dict(div=-1.0), dict(p=0.0), dict(p=-0.5), dict(p=nan),
           dict(logits_u=glu.ptr, scale=gs.ptr, rps=0), dict(logits_u=glu.ptr, scale=gs.ptr, rps=4),  # 6 rows are no multiple of 4
           dict(logits_u=glu.ptr), dict(scale=gs.ptr), dict(logits=None), dict(out=None)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(_lib.MMVIDError, match=r'rc=[1-9-].*logits_truncate: \S') as err:  # a nonzero status with its text
            call_abi('mmvid_logits_truncate', a['logits'], a['logits_u'], a['ld'], a['scale'], a['rps'], a['div'], a['k'], a['p'], a['R'],
                     a['V'], a['out'], a['ld_out'], gk.ptr)
        assert 'launch failed' not in str(err.value), change
        for gb in (gl, glu, gs, gout, gk):
            gb.check(f'refused call {change}')
        assert bool((bits(gout.window()) == SENTINEL_BITS[f32]).all()) and bool((bits(gk.window()) == SENTINEL_BITS[torch.int32]).all()), change
    # R == 0 is no refusal: status 0, nothing stored
    call_abi('mmvid_logits_truncate', gl.ptr, None, V, None, 1, 1.0, 4, 0.9, 0, V, gout.ptr, V, gk.ptr)
    assert bool((bits(gout.window()) == SENTINEL_BITS[f32]).all())
    # and the accepted call, guided, on the same buffers (rows_per_scale = 3: two groups)
    call_abi('mmvid_logits_truncate', gl.ptr, glu.ptr, V, gs.ptr, 3, 1.0, 4, 0.9, R, V, gout.ptr, V, gk.ptr)
    assert bool(torch.isfinite(gout.check('accepted call')).any(dim=1).all())


# ------------------------------------------------------------------------------------------------------ 8. the BERT sampler
@pytest.fixture(scope='module')
def model():
    return build_model()


@pytest.fixture(scope='module')
def mp(golden):
    return dict(golden('mask_predict').meta['mp_config'], B=BEAMS)


@pytest.fixture(scope='module')
def controls(model):
    """Text, control and an unconditional control that differs by more than a rounding (as tests/test_guidance_gpu.py builds it)."""
    gen = torch.Generator().manual_seed(61)
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
def plain(model, mp, controls):
    """One run without the keywords, its variates recorded: shared by the tests below and left unchanged by them."""
    rec, trace = Recorder(), []
    seq = model.mask_predict(controls[1], dynamic=False, steps=STEPS, mp_config=mp, _race=rec, _trace=trace)[0]
    return dict(seq=seq, drawn=rec.drawn, trace=trace)


def check_truncated_steps(trace, drawn, mp, k_steps, p_steps, guided_scale=None, known=None):
    """Every truncated step of a trace, recomputed from the step's own records: logits_t is the rule applied to the recorded logits
    (equality for top-k, the sandwich for top-p), the step's tokens and confidences are the plain race on logits_t, kept <= k, and no
    drawn token is an excluded class (`known` [NB, TS] bool: positions whose step-0 token is given, not drawn).  -> the number of
    truncated steps."""
    from mmvid_amd import ops, sampling
    temp = sampling.schedule(mp, TS)[1]
    seen = 0
    for rec in trace:
        t = rec['t']
        k, p = k_steps[t], p_steps[t]
        if k is None and p is None:
            assert 'logits_t' not in rec and 'kept' not in rec, f'step {t}: no filter on, but a truncated tensor was recorded'
            continue
        seen += 1
        nb = 1 if t == 0 else BEAMS
        g = rec['logits']
        if guided_scale is not None:
            w = torch.full((NB, ), guided_scale, device=DEV).repeat_interleave(nb * TS)
            g = composed(rec['logits'], rec['logits_u'], w)
        g = g.cpu()
        lt, kept = rec['logits_t'].cpu(), rec['kept'].cpu()
        assert lt.shape == g.shape == (NB * nb * TS, 256) and kept.shape == (g.shape[0], )
        K = torch.isfinite(lt)
        assert torch.equal(kept, K.sum(1).to(torch.int32))
        if p is None:
            assert torch.equal(bits(lt), bits(torch.from_numpy(T.truncated(g.numpy(), T.topk_set(g.numpy(), k))))), f'step {t}'
        else:
            assert float(T.mean_distance(g.numpy()).max()) <= T.MAX_MEAN_DISTANCE  # (the margin's condition holds for these logits)
            lo, hi = T.sandwich(g.numpy(), p)
            if k is not None:
                lo, hi = lo & T.topk_set(g.numpy(), k), hi & T.topk_set(g.numpy(), k)
            assert_sandwich(lt, g.numpy(), lo, hi, f'step {t}')
        if k is not None:
            assert int(kept.max()) <= k
        u = drawn.get(f'tok{t}_noise_u') if temp[t] != 0.0 else None
        tok, y = ops.sample_race(rec['logits_t'], rec['E_tok'], u, temp[t])
        got_tok = (rec['I_tok'] if t == 0 else rec['Inew']).reshape(-1)
        got_y = (rec['Y'] if t == 0 else rec['Ynew']).reshape(-1)
        drawn_here = torch.ones_like(tok, dtype=torch.bool) if (known is None or t > 0) else ~known.reshape(-1)
        assert torch.equal(got_tok[drawn_here], tok[drawn_here]) and torch.equal(got_y[drawn_here], y[drawn_here]), \
            f'step {t}: not the plain race on the truncated logits'
        assert bool(K[torch.arange(len(tok)), got_tok.cpu()][drawn_here.cpu()].all()), f'step {t}: a drawn token is an excluded class'
    return seen


def test_bert_with_filters_that_keep_everything_is_the_unkeyworded_call(model, mp, controls, plain):
    trace = []
    seq = model.mask_predict(controls[1], dynamic=False, steps=STEPS, mp_config=mp, _race=replay(plain['drawn']), _trace=trace, top_k=256,
                             top_p=1.0)[0]
    report_mismatch(seq.cpu(), plain['seq'].cpu(), 'top_k = V, top_p = 1: tokens')
    for got, want in zip(trace, plain['trace']):
        assert torch.equal(got['I_tok'], want['I_tok']) and torch.equal(got['Y'], want['Y']), f'step {got["t"]}'


def test_bert_top_k_per_step(model, mp, controls, plain):
    ks = (None, 8, 3, 1)
    trace = []
    seq = model.mask_predict(controls[1], dynamic=False, steps=STEPS, mp_config=mp, _race=replay(plain['drawn']), _trace=trace, top_k=ks)[0]
    assert len(trace) == STEPS and check_truncated_steps(trace, plain['drawn'], mp, ks, [None] * STEPS) == 3
    assert torch.equal(trace[0]['I_tok'], plain['trace'][0]['I_tok'])  # step 0 has no filter: the unkeyworded step
    assert not torch.equal(seq, plain['seq'])  # (the filters did something)
    assert 0 <= int(seq.min()) and int(seq.max()) < 256


def test_bert_top_p_under_guidance(model, mp, controls, plain):
    _, control, uncond = controls
    trace = []
    seq = model.mask_predict(control, dynamic=False, steps=STEPS, mp_config=mp, _race=replay(plain['drawn']), _trace=trace,
                             uncond_emb=uncond, guidance_scale=2.0, top_p=0.9)[0]
    assert check_truncated_steps(trace, plain['drawn'], mp, [None] * STEPS, [0.9] * STEPS, guided_scale=2.0) == STEPS
    assert all(int(r['kept'].max()) < 256 for r in trace)  # (the nucleus removed something at every step)
    assert 0 <= int(seq.min()) and int(seq.max()) < 256


def test_bert_top_k_1_without_noise_is_greedy(model, mp, controls):
    cold = dict(mp, N1_t=0.0, N2_t=0.0, N3_t=0.0, N4_t=0.0)  # temperature schedule 0: no Gumbel noise
    trace = []
    model.mask_predict(controls[1], dynamic=False, steps=STEPS, mp_config=cold, _race=Recorder(), _trace=trace, top_k=1)
    assert len(trace) == STEPS
    for rec in trace:
        got = (rec['I_tok'] if rec['t'] == 0 else rec['Inew']).reshape(-1).cpu()
        want = torch.from_numpy(T.order(rec['logits'].cpu().numpy())[:, 0].copy())
        assert torch.equal(got, want), f'step {rec["t"]}: a token is not the argmax of its row'
        assert bool((rec['kept'] == 1).all())
        y = (rec['Y'] if rec['t'] == 0 else rec['Ynew']).reshape(-1)
        assert bool((y == 1.0).all())  # the confidence under the truncated distribution


def test_completion_with_top_k(model, mp, controls):
    from mmvid_amd import completion
    text = controls[0]
    gen = torch.Generator().manual_seed(62)
    tokens = torch.randint(0, 256, (NB, TS), generator=gen).to(DEV)
    given = torch.tensor([[1, 0]] * NB, dtype=torch.uint8)  # the first frame of every video is known
    known = torch.zeros(NB, TS, dtype=torch.bool, device=DEV)
    known[:, :TS // 2] = True
    rec, trace = Recorder(), []
    _, seq = completion.complete(model, text, tokens, given, mask_predict_steps=STEPS, mp_config=mp, dynamic=False, decode=False,
                                 top_k=4, _race=rec, _trace=trace)
    seq = seq.reshape(NB, TS)
    assert torch.equal(seq[known], tokens[known])
    for r in trace:
        assert torch.equal(r['I_tok'][known], tokens[known]), f'step {r["t"]}: a given token changed'
    assert check_truncated_steps(trace, rec.drawn, mp, [4] * STEPS, [None] * STEPS, known=known) == STEPS


# ----------------------------------------------------------------------------------------------------- 9. the ART-V sampler
@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(63)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(64)
    text = torch.randint(1, 49408, (4, 16), generator=gen).to(DEV)  # batch 4: the five-launch decode step
    vis = torch.randint(0, 256, (4, 16), generator=gen).to(DEV)
    return m, text, vis


def artv_tokens(m, text, vis, monkeypatch, **kw):
    """generate_images -> the token sequence [B, steps] it decoded."""
    seen = []
    decode = m.vae.decode
    monkeypatch.setattr(m.vae, 'decode', lambda seq: (seen.append(seq.clone()), decode(seq))[1])
    m.generate_images(text, visual=vis, **kw)
    monkeypatch.setattr(m.vae, 'decode', decode)
    return seen[0].reshape(text.shape[0], -1)


def stored_race():
    gen, store = torch.Generator().manual_seed(65), {}

    def race(name, shape):
        if name not in store:
            store[name] = torch.empty(shape).exponential_(generator=gen).to(DEV)
        return store[name]
    return race


def test_artv_top_k_1_production_path_equals_the_eager_one(artv, monkeypatch):
    m, text, vis = artv
    replays = []
    inner = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), inner(self))[1])
    produced = artv_tokens(m, text, vis, monkeypatch, top_k=1)  # pre-drawn variates, [truncate -> draw -> advance] captured
    n_replays = len(replays)
    eager = artv_tokens(m, text, vis, monkeypatch, top_k=1, _race=stored_race())
    assert produced.shape == (4, m.target_seq_len) and 0 <= int(produced.min()) and int(produced.max()) < 256
    report_mismatch(produced.cpu(), eager.cpu(), 'top_k = 1: the captured step against the eager one (both greedy)')
    assert n_replays >= m.target_seq_len - 4 and len(replays) == n_replays, 'the truncated call did not run its captured step'
    # the reference's loop (the whole prefix per token, through _draw): greedy too, so the variates do not matter
    a = artv_tokens(m, text, vis, monkeypatch, top_k=1, use_cache=False)
    b = artv_tokens(m, text, vis, monkeypatch, top_k=1, _race=stored_race(), use_cache=False)
    assert torch.equal(a, b) and 0 <= int(a.min()) and int(a.max()) < 256


def test_artv_batch_2_with_a_keyword_takes_the_separate_launches(artv, monkeypatch):
    """Batch 1-2 is where the one-launch-per-token path lives; it has no truncation in it, so a call with a keyword must go through
    draw / advance (captured) on a session that could have taken it, and give the eager call's tokens (both greedy)."""
    from mmvid_amd import _lib
    m, text, vis = artv
    launched = []
    inner = _lib.DecodeToken
    monkeypatch.setattr(_lib, 'DecodeToken', lambda *a, **k: (launched.append(1), inner(*a, **k))[1])
    replays = []
    replay_inner = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), replay_inner(self))[1])
    produced = artv_tokens(m, text[:2], vis[:2], monkeypatch, top_k=1)
    n_replays = len(replays)
    eager = artv_tokens(m, text[:2], vis[:2], monkeypatch, top_k=1, _race=stored_race())
    assert not launched, 'a truncated call set up the one-launch-per-token path'
    assert produced.shape == (2, m.target_seq_len) and 0 <= int(produced.min()) and int(produced.max()) < 256
    report_mismatch(produced.cpu(), eager.cpu(), 'batch 2, top_k = 1: the captured step against the eager one')
    assert n_replays >= m.target_seq_len - 4 and len(replays) == n_replays


def test_artv_sampling_probs_and_the_filter_that_keeps_everything(artv, monkeypatch):
    m, text, vis = artv
    lg = 3 * torch.randn(5, 256, generator=torch.Generator().manual_seed(66))
    probs = m.sampling_probs(lg.to(DEV), filter_thres=0.5, temperature=0.8, top_k=8)
    assert bool(((probs > 0).sum(1) == 8).all())
    assert torch.allclose(probs.sum(1), torch.ones(5, device=DEV), atol=1e-6)
    want = T.topk_set(lg.numpy(), 8)
    assert np.array_equal((probs > 0).cpu().numpy(), want)
    nucleus = m.sampling_probs(lg.to(DEV), temperature=0.5, top_p=0.5)  # (a power of two: the margin's derivation covers it)
    lo, hi = T.sandwich(lg.numpy(), 0.5, logit_div=0.5)
    K = (nucleus > 0).cpu().numpy()
    assert (lo <= K).all() and (K <= hi).all()
    base = artv_tokens(m, text, vis, monkeypatch, _race=stored_race())
    same = artv_tokens(m, text, vis, monkeypatch, _race=stored_race(), top_k=256)
    assert torch.equal(same, base)
    fewer = artv_tokens(m, text, vis, monkeypatch, _race=stored_race(), top_k=2)
    assert not torch.equal(fewer, base)
