"""Classifier-free guidance for ART-V on the device: the guided block-per-row draw (mmvid_sample_race_guided_at) against the guided
wave-per-row kernel and against the plain draw on torch-composed logits, the grouped embedding launch (mmvid_decode_embed_record_groups)
against the existing one, both on guarded, padded and poisoned buffers; then DALLE.generate_images with the guidance keywords -- the
stacked prompt, the conditional branch at scale 0, every token restated from its own trace record, the captured production path against
the eager one -- and the training-side condition drop of DALLE.forward.  Every comparison is an equality."""
import pytest
import torch

import mmvid_amd
from guarded import SENTINEL_BITS, Guarded, bits, call_abi, ptr_of, report_mismatch
from test_guidance_gpu import composed
from test_host_logic import tiny_vae
from test_truncate_gpu import artv_tokens, stored_race

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG_INF = float('-inf')
f32, i32, i64 = torch.float32, torch.int32, torch.int64
SCALES = (0.0, 2.0, -0.5, 7.5)
DIVS = (1.0, 0.7)
PAD = 24


# ------------------------------------------------------------------------------------------------- 1. the guided row draw
def race_rows(R, V, seed, draws=None):
    """lc (columns 3, 10, 17, ... -inf: classes the conditional branch rules out, with a finite lu), lu, E [R, V] or [draws, R, V]."""
    gen = torch.Generator().manual_seed(seed)
    lc, lu = 3 * torch.randn(R, V, generator=gen), 3 * torch.randn(R, V, generator=gen)
    lc[:, 3::7] = NEG_INF
    E = torch.empty((R, V) if draws is None else (draws, R, V)).exponential_(generator=gen)
    return lc, lu, E


def guided_at(lc, lu, scale, rps, E, *, div=1.0, tok_offset=0, step=None, step0=0, pad=PAD):
    """One call of the entry on guarded buffers (ld = V + pad) -> tok [R] on the host."""
    R, V = lc.shape
    glc, glu = Guarded(lc, role='in', ld=V + pad), Guarded(lu, role='in', ld=V + pad)
    gs, gE = Guarded(scale, role='in'), Guarded(E, role='in')
    gstep = None if step is None else Guarded(torch.tensor([step], dtype=i32), role='in')
    gtok = Guarded(role='out', shape=(R, ), dtype=i64)
    call_abi('mmvid_sample_race_guided_at', glc.ptr, glu.ptr, V + pad, gs.ptr, rps, gE.ptr, ptr_of(gstep), step0, R * V, div, R, V, tok_offset,
             gtok.ptr)
    for gb, what in ((glc, 'logits_c'), (glu, 'logits_u'), (gs, 'scale'), (gE, 'E'), (gstep, 'step')):
        if gb is not None:
            gb.check(f'sample_race_guided_at {what}')
    return gtok.check('sample_race_guided_at tok')


def references(lc, lu, scale, rps, E, div):
    """-> (the guided wave-per-row kernel without noise at temperature 0, the plain draw on lc + w (lc - lu)): tokens on the host."""
    from mmvid_amd import ops
    lc, lu, scale, E = lc.to(DEV), lu.to(DEV), scale.to(DEV), E.to(DEV)
    wave, _ = ops.sample_race_guided(lc, lu, scale, rps, E, None, 0.0, logit_div=div)
    g = composed(lc, lu, scale.repeat_interleave(rps))
    assert not bool(torch.isnan(g).any())
    plain, _ = ops.sample_race(g, E, None, 0.0, logit_div=div)
    return wave.cpu(), plain.cpu(), g


@pytest.mark.parametrize('R,rps', [(1, 1), (5, 1), (6, 1), (6, 3)])
@pytest.mark.parametrize('V', [1, 63, 255, 256, 257, 1000, 2047, 2048, 2049, 4100])  # the thread-stride and outer-trip edges of 256 x 8
def test_guided_row_draw_equals_the_wave_kernel_and_the_plain_draw(V, R, rps):
    from mmvid_amd import ops
    lc, lu, E = race_rows(R, V, 8000 + 16 * V + R + rps)
    groups = R // rps
    for div in DIVS:
        for rot in range(len(SCALES)):  # every scale reaches every group
            scale = torch.tensor([SCALES[(g + rot) % len(SCALES)] for g in range(groups)])
            tok = guided_at(lc, lu, scale, rps, E, div=div)
            wave, plain, g = references(lc, lu, scale, rps, E, div)
            what = f'V={V} R={R} rows_per_scale={rps} logit_div={div} scales={scale.tolist()}'
            report_mismatch(tok, wave, f'{what}: against mmvid_sample_race_guided')
            report_mismatch(tok, plain, f'{what}: against mmvid_sample_race on the composed logits')
            assert 0 <= int(tok.min()) and int(tok.max()) < V
            if V > 3:
                assert bool((tok % 7 != 3).all()), f'{what}: a token landed on a class the conditional branch rules out'
            # the token-only form of the plain draw (the production kernel of the unguided loop) at logit_div = 1 only: the compiler fuses
            # that kernel's first slot's x * (1 / logit_div) - max, which is exact at 1 and may move a key by an ulp elsewhere
            if div == 1.0:
                row, _ = ops.sample_race(g, E.to(DEV), None, 0.0, want_y=False)
                report_mismatch(tok, row.cpu(), f'{what}: against the block-per-row plain draw')


def test_guided_row_draw_crafted_rows():
    R, V = 3, 2049
    # an all-equal row under equal variates: every key ties, and the tie goes to the lower index
    lc, lu, E = torch.full((R, V), 1.25), torch.full((R, V), -0.5), torch.ones(R, V)
    scale = torch.tensor([2.0, 0.0, -0.5])
    assert guided_at(lc, lu, scale, 1, E).tolist() == [0, 0, 0]
    E2 = E.clone()
    E2[0, :100], E2[1, :2048], E2[2, :257] = 2.0, 2.0, 2.0  # the smallest key starts at class 100 / 2048 (the second trip) / 257
    assert guided_at(lc, lu, scale, 1, E2).tolist() == [100, 2048, 257]
    assert guided_at(lc, lu, scale, 1, E2, tok_offset=1000, div=0.7).tolist() == [1100, 3048, 1257]
    # classes the conditional branch rules out stay out at every scale, also where they hold the smallest variate
    lc, lu, E = race_rows(4, 1000, 8100)
    E[:, 3::7] = 1e-30
    for w in SCALES:
        scale = torch.full((4, ), w)
        tok = guided_at(lc, lu, scale, 1, E, tok_offset=-7)
        wave, plain, _ = references(lc, lu, scale, 1, E, 1.0)
        assert torch.equal(tok + 7, wave) and torch.equal(tok + 7, plain) and bool(((tok + 7) % 7 != 3).all())
    # a row the conditional branch rules out entirely draws class 0, as the wave kernel does
    lc[1] = NEG_INF
    scale = torch.tensor([2.0, 2.0, 0.0, 7.5])
    tok = guided_at(lc, lu, scale, 1, E)
    assert int(tok[1]) == 0 and torch.equal(tok, references(lc, lu, scale, 1, E, 1.0)[0])


@pytest.mark.parametrize('V', [257, 2049])
def test_guided_row_draw_reads_the_draw_the_device_position_names(V):
    R, rps, draws, step0 = 6, 3, 3, 5
    lc, lu, E = race_rows(R, V, 8200 + V, draws=draws)
    scale = torch.tensor([2.0, -0.5])
    toks = []
    for n in (0, 2):
        tok = guided_at(lc, lu, scale, rps, E, div=0.7, step=step0 + n, step0=step0)
        wave, plain, _ = references(lc, lu, scale, rps, E[n].contiguous(), 0.7)
        report_mismatch(tok, wave, f'draw {n} of {draws}')
        report_mismatch(tok, plain, f'draw {n} of {draws}: composed')
        toks.append(tok)
    assert not torch.equal(toks[0], toks[1])  # (the two blocks hold different variates)
    tok = guided_at(lc, lu, scale, rps, E[1].contiguous(), div=0.7)  # step_dev == NULL: the [R][V] block itself
    report_mismatch(tok, references(lc, lu, scale, rps, E[1].contiguous(), 0.7)[0], 'step_dev == NULL')


def test_guided_row_draw_through_ops_and_views():
    from mmvid_amd import ops
    R, V = 5, 1000
    lc, lu, E = (t.to(DEV) for t in race_rows(R, V, 8300, draws=2))
    scale = torch.tensor(SCALES + (2.0, ), device=DEV)
    wide = torch.full((2 * R, V), float('nan'), device=DEV)  # the sampler's layout: the two branches are the halves of one tensor
    wide[:R], wide[R:] = lc, lu
    want, _ = ops.sample_race_guided(lc, lu, scale, 1, E[1].contiguous(), None, 0.0, logit_div=0.7)
    pos = torch.tensor([11], dtype=i32, device=DEV)
    out = torch.full((R, ), -1, dtype=i64, device=DEV)
    got = ops.sample_race_guided_at(wide[:R], wide[R:], scale, 1, E, logit_div=0.7, tok_out=out, step_dev=pos, step0=10)
    assert got is out and torch.equal(out, want)
    assert torch.equal(ops.sample_race_guided_at(lc, lu, scale, 1, E[1].contiguous(), logit_div=0.7), want)
    with pytest.raises(ValueError, match='row stride'):
        ops.sample_race_guided_at(lc, torch.zeros(R, V + 8, device=DEV)[:, :V], scale, 1, E[0].contiguous())
    with pytest.raises(ValueError, match='scales'):
        ops.sample_race_guided_at(lc, lu, scale[:-1].contiguous(), 1, E[0].contiguous())
    with pytest.raises(ValueError, match='scales'):
        ops.sample_race_guided_at(lc, lu, scale, 2, E[0].contiguous())  # 5 rows are no multiple of 2


def test_every_refusal_of_the_guided_row_draw_leaves_tok_alone():
    from mmvid_amd import _lib
    R, V = 6, 64
    lc, lu, E = race_rows(R, V, 8400)
    glc, glu, gs, gE = Guarded(lc, role='in'), Guarded(lu, role='in'), Guarded(torch.ones(2), role='in'), Guarded(E, role='in')
    gtok = Guarded(role='out', shape=(R, ), dtype=i64, partial=True)
    ok = dict(lc=glc.ptr, lu=glu.ptr, ld=V, scale=gs.ptr, rps=3, E=gE.ptr, div=1.0, R=R, V=V, tok=gtok.ptr)
    bad = [dict(lc=None), dict(lu=None), dict(scale=None), dict(E=None), dict(tok=None), dict(ld=V - 1), dict(R=1025, rps=1), dict(rps=0),
           dict(rps=-3), dict(rps=4), dict(div=0.0), dict(div=-1.0), dict(V=0)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(_lib.MMVIDError, match=r'rc=[1-9-].*sample_race_guided_at: \S') as err:  # a nonzero status with its text
            call_abi('mmvid_sample_race_guided_at', a['lc'], a['lu'], a['ld'], a['scale'], a['rps'], a['E'], None, 0, R * V, a['div'], a['R'],
                     a['V'], 0, a['tok'])
        assert 'launch failed' not in str(err.value), change
        for gb in (glc, glu, gs, gE, gtok):
            gb.check(f'refused call {change}')
        assert bool((bits(gtok.window()) == SENTINEL_BITS[i64]).all()), change
    call_abi('mmvid_sample_race_guided_at', glc.ptr, glu.ptr, V, gs.ptr, 3, gE.ptr, None, 0, R * V, 1.0, 0, V, 0, gtok.ptr)  # R == 0: no refusal
    assert bool((bits(gtok.window()) == SENTINEL_BITS[i64]).all())
    call_abi('mmvid_sample_race_guided_at', glc.ptr, glu.ptr, V, gs.ptr, 3, gE.ptr, None, 0, R * V, 1.0, R, V, 0, gtok.ptr)  # the accepted call
    tok = gtok.check('accepted call')
    assert 0 <= int(tok.min()) and int(tok.max()) < V


# --------------------------------------------------------------------------------------------- 2. the grouped embedding launch
EMB, TABLE, NPOS, POS, POS0, REC_LD = 768, 256, 40, 21, 18, 8


def embed_operands(B, seed):
    gen = torch.Generator().manual_seed(seed)
    table, pos_rows = torch.randn(TABLE, EMB, generator=gen), torch.randn(NPOS, EMB, generator=gen)
    tok = torch.randint(0, TABLE, (B, ), generator=gen)
    return dict(tok=Guarded(tok, role='in'), table=Guarded(table, role='in'), pos_rows=Guarded(pos_rows, role='in'),
                pos=Guarded(torch.tensor([POS], dtype=i32), role='in')), tok


def embed_call(name, ops_in, B, rows, extra, pos_off=2, with_record=True):
    """The existing entry (extra = ()) or the grouped one (extra = (groups, )) on fresh guarded outputs -> (x window, record window)."""
    gx = Guarded(role='out', shape=(rows, EMB), dtype=f32)
    grec = Guarded(role='out', shape=(B, REC_LD), dtype=i64, partial=True)
    call_abi(name, ops_in['tok'].ptr, ops_in['table'].ptr, TABLE, ops_in['pos_rows'].ptr, ops_in['pos'].ptr, pos_off, B, *extra, EMB, gx.ptr,
             grec.ptr if with_record else None, REC_LD if with_record else 0, POS0)
    for k, gb in ops_in.items():
        gb.check(f'{name} {k}')
    return gx.check(f'{name} x'), grec.check(f'{name} record')


@pytest.mark.parametrize('groups', [1, 2, 3])
@pytest.mark.parametrize('B', [1, 3])
def test_grouped_embed_writes_the_existing_launch_per_group(B, groups):
    ops_in, tok = embed_operands(B, 8500 + B)
    want_x, want_rec = embed_call('mmvid_decode_embed_record', ops_in, B, B, ())
    x, rec = embed_call('mmvid_decode_embed_record_groups', ops_in, B, groups * B, (groups, ))
    for g in range(groups):
        assert torch.equal(bits(x[g * B:(g + 1) * B]), bits(want_x)), f'group {g} of {groups}'
    assert torch.equal(rec, want_rec)  # one column written, the sentinel elsewhere
    assert torch.equal(rec[:, POS - POS0], tok) and int((bits(rec) != SENTINEL_BITS[i64]).sum()) == B
    x, rec = embed_call('mmvid_decode_embed_record_groups', ops_in, B, groups * B, (groups, ), with_record=False)  # record == NULL
    assert torch.equal(bits(x[-B:]), bits(want_x)) and bool((bits(rec) == SENTINEL_BITS[i64]).all())


def test_grouped_embed_refuses_no_groups_and_runs_through_ops():
    from mmvid_amd import _lib, ops
    B = 3
    ops_in, tok = embed_operands(B, 8600)
    gx = Guarded(role='out', shape=(B, EMB), dtype=f32, partial=True)
    for groups in (0, -1):
        with pytest.raises(_lib.MMVIDError, match=r'rc=[1-9-].*decode_embed_groups: \S'):
            call_abi('mmvid_decode_embed_record_groups', ops_in['tok'].ptr, ops_in['table'].ptr, TABLE, ops_in['pos_rows'].ptr, ops_in['pos'].ptr,
                     0, B, groups, EMB, gx.ptr, None, 0, 0)
        assert bool((bits(gx.check('refused call')) == SENTINEL_BITS[f32]).all())
    gen = torch.Generator().manual_seed(8601)
    table, pos_rows = torch.randn(TABLE, EMB, generator=gen).to(DEV), torch.randn(NPOS, EMB, generator=gen).to(DEV)
    tok, pos = tok.to(DEV), torch.tensor([POS], dtype=i32, device=DEV)
    rec1, rec2 = torch.full((B, REC_LD), -1, device=DEV), torch.full((B, REC_LD), -1, device=DEV)
    want = ops.decode_embed(tok, table, pos_rows, pos, torch.empty(B, EMB, device=DEV), record=rec1, record_pos0=POS0)
    got = ops.decode_embed_groups(tok, table, pos_rows, pos, torch.empty(2 * B, EMB, device=DEV), 2, record=rec2, record_pos0=POS0)
    assert torch.equal(got[:B], want) and torch.equal(got[B:], want) and torch.equal(rec1, rec2)
    with pytest.raises(ValueError, match='groups'):
        ops.decode_embed_groups(tok, table, pos_rows, pos, torch.empty(2 * B + 1, EMB, device=DEV), 2)


# ------------------------------------------------------------------------------------------------------------ 3. the sampler
B, TT, V = 4, 16, 256


@pytest.fixture(scope='module')
def artv():
    """The tiny ART-V model of tests/test_truncate_gpu.py: dim 768, 2 layers, 16 text positions, 2 targets of 16 tokens, 256 codes."""
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(83)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(84)
    text = torch.randint(1, 49408, (B, TT), generator=gen)
    text[1, 11:] = 0
    vis = torch.randint(0, 256, (B, 16), generator=gen)
    return m, text.to(DEV), vis.to(DEV)


def stacked_race(seed=85):
    """A `_race` whose variates for a call of B rows are the first B rows of those for a call of 2B rows, by name."""
    gen, store = torch.Generator().manual_seed(seed), {}

    def race(name, shape):
        if name not in store:
            store[name] = torch.empty(2 * B, shape[1]).exponential_(generator=gen).to(DEV)
        return store[name][:shape[0]]
    return race


def traced(m, text, vis, monkeypatch_cls, **kw):
    """generate_images with a trace -> (tokens [rows, steps], trace)."""
    trace = []
    with monkeypatch_cls.context() as mp:
        tokens = artv_tokens(m, text, vis, mp, _trace=trace, **kw)
    return tokens, trace


@pytest.fixture(scope='module')
def runs(artv):
    """The runs the tests below share (and leave unchanged): the unguided call on the stacked batch [text; 0], [vis; -1] of 2B rows, and
    the guided call at scale 0 with the default drop, on the same variates for rows 0..B-1."""
    m, text, vis = artv
    race = stacked_race()
    text2, vis2 = torch.cat((text, torch.zeros_like(text))), torch.cat((vis, torch.full_like(vis, -1)))
    stacked = traced(m, text2, vis2, pytest.MonkeyPatch, _race=race)
    zero = traced(m, text, vis, pytest.MonkeyPatch, _race=race, guidance_scale=0.0)
    return dict(race=race, stacked=stacked, zero=zero)


def test_the_stacked_prompt_and_its_prefill(artv, runs):
    m = artv[0]
    (tok_s, trace_s), (tok_g, trace_g) = runs['stacked'], runs['zero']
    assert len(trace_s) == len(trace_g) == m.target_seq_len and tok_s.shape == (2 * B, m.target_seq_len) and tok_g.shape == (B, m.target_seq_len)
    assert trace_g[0]['logits'].shape == (2 * B, V)
    report_mismatch(trace_g[0]['logits'].cpu(), trace_s[0]['logits'].cpu(), 'token 0: the logits of the guided call against the stacked batch')
    assert not torch.equal(trace_g[0]['logits'][:B], trace_g[0]['logits'][B:])  # (the two prompts differ)
    assert 'scale' not in trace_s[0] and torch.equal(trace_g[0]['scale'], torch.zeros(B, device=DEV))
    assert 'logits_t' not in trace_g[0] and 'kept' not in trace_g[0]


def test_scale_zero_leaves_the_conditional_branch_undisturbed(artv, runs):
    """Rests on the decode step being independent from row to row at a fixed batch: rows B..2B-1 carry other tokens in the two calls."""
    (tok_s, trace_s), (tok_g, trace_g) = runs['stacked'], runs['zero']
    for n, (g, s) in enumerate(zip(trace_g, trace_s)):
        report_mismatch(g['tok'].cpu(), s['tok'][:B].cpu(), f'token {n}: guided at scale 0 against rows 0..B-1 of the stacked unguided call')
        assert torch.equal(g['E'], s['E'][:B])
    report_mismatch(tok_g.cpu(), tok_s[:B].cpu(), 'the decoded sequences')
    assert not torch.equal(tok_s[B:], tok_s[:B])  # (the unconditional rows of the stacked call drew tokens of their own)


def test_the_unconditional_rows_get_the_drawn_token(artv, runs):
    m = artv[0]
    for tok, trace in (runs['zero'], runs['stacked']):
        assert [('x_in' in r) for r in trace] == [True] * (m.target_seq_len - 1) + [False]  # the last token is never embedded
    for n, r in enumerate(runs['zero'][1][:-1]):
        assert r['x_in'].shape == (2 * B, 768) and torch.equal(bits(r['x_in'][B:]), bits(r['x_in'][:B])), f'token {n}'
    differ = [not torch.equal(r['x_in'][B:], r['x_in'][:B]) for r in runs['stacked'][1][:-1]]
    assert any(differ)  # (where the halves draw separately they do differ)


@pytest.mark.parametrize('top_k,top_p', [(None, None), (5, None), (None, 0.9)])
def test_every_guided_token_is_its_records_restatement(artv, runs, top_k, top_p):
    from mmvid_amd import ops
    m, text, vis = artv
    scale = torch.tensor([2.0, 2.0, 0.0, 2.0], device=DEV)  # video 2 is unguided
    tokens, trace = traced(m, text, vis, pytest.MonkeyPatch, _race=runs['race'], guidance_scale=scale, top_k=top_k, top_p=top_p)
    assert len(trace) == m.target_seq_len
    for n, r in enumerate(trace):
        lc, lu = r['logits'][:B], r['logits'][B:]
        assert torch.equal(r['scale'], scale) and r['E'].shape == (B, V)
        if top_k is None and top_p is None:
            assert 'logits_t' not in r and 'kept' not in r
            lg = composed(lc, lu, scale)
        else:
            lg, kept = ops.logits_truncate(lc, top_k, top_p, logits_u=lu, scale=scale, rows_per_scale=1, want_kept=True)
            assert torch.equal(bits(r['logits_t']), bits(lg)) and torch.equal(r['kept'], kept), f'token {n}'
            assert int(kept.max()) < V and (top_k is None or int(kept.max()) <= top_k)
        want, _ = ops.sample_race(lg, r['E'], None, 0.0, want_y=False)
        report_mismatch(r['tok'].cpu(), want.cpu(), f'token {n}: the plain race on the guided {"and truncated " if r.get("kept") is not None else ""}logits')
        assert torch.equal(tokens[:, n], r['tok'])
    if top_k is None and top_p is None:
        report_mismatch(tokens[2].cpu(), runs['zero'][0][2].cpu(), 'the video at scale 0 against its tokens at scale 0 for every video')
        assert not torch.equal(tokens, runs['zero'][0])  # (scale 2 moved a token of another video)


def count_replays(monkeypatch):
    replays = []
    inner = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), inner(self))[1])
    return replays


def test_production_path_equals_the_eager_one(artv, monkeypatch):
    m, text, vis = artv
    replays = count_replays(monkeypatch)
    produced = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0, top_k=1)  # [truncate -> draw -> embed -> advance] captured
    n_replays = len(replays)
    eager = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0, top_k=1, _race=stored_race())
    assert produced.shape == (B, m.target_seq_len) and 0 <= int(produced.min()) and int(produced.max()) < V
    report_mismatch(produced.cpu(), eager.cpu(), 'guided, top_k = 1: the captured step against the eager one (both greedy)')
    assert n_replays >= m.target_seq_len - 4 and len(replays) == n_replays, 'the guided call did not run its captured step'
    torch.manual_seed(86)
    a = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0)  # the guided row draw on pre-drawn variates, captured
    assert len(replays) >= 2 * (m.target_seq_len - 4)
    torch.manual_seed(86)
    b = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0)
    assert torch.equal(a, b) and a.shape == (B, m.target_seq_len) and 0 <= int(a.min()) and int(a.max()) < V


def test_batch_1_runs_two_tower_rows_through_the_separate_launches(artv, monkeypatch):
    from mmvid_amd import _lib
    m, text, vis = artv
    launched = []
    inner = _lib.DecodeToken
    monkeypatch.setattr(_lib, 'DecodeToken', lambda *a, **k: (launched.append(1), inner(*a, **k))[1])
    replays = count_replays(monkeypatch)
    produced = artv_tokens(m, text[:1], vis[:1], monkeypatch, guidance_scale=2.0, top_k=1)
    n_replays = len(replays)
    eager = artv_tokens(m, text[:1], vis[:1], monkeypatch, guidance_scale=2.0, top_k=1, _race=stored_race())
    plain = artv_tokens(m, text[:1], vis[:1], monkeypatch, guidance_scale=2.0)
    assert not launched, 'a guided call set up the one-launch-per-token path'
    assert produced.shape == (1, m.target_seq_len) and 0 <= int(produced.min()) and int(produced.max()) < V
    report_mismatch(produced.cpu(), eager.cpu(), 'batch 1, guided, top_k = 1: the captured step against the eager one')
    assert n_replays >= m.target_seq_len - 4 and 0 <= int(plain.min()) and int(plain.max()) < V


def test_the_reference_loop_without_the_cache(artv, monkeypatch):
    m, text, vis = artv
    a = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0, top_k=1, use_cache=False)
    b = artv_tokens(m, text, vis, monkeypatch, guidance_scale=2.0, top_k=1, use_cache=False, _race=stored_race())
    assert torch.equal(a, b) and a.shape == (B, m.target_seq_len) and 0 <= int(a.min()) and int(a.max()) < V
    zero = artv_tokens(m, text, vis, monkeypatch, guidance_scale=0.0, use_cache=False, _race=stored_race())
    three = artv_tokens(m, text, vis, monkeypatch, guidance_scale=3.0, use_cache=False, _race=stored_race())
    unguided = artv_tokens(m, text, vis, monkeypatch, use_cache=False, _race=stored_race())
    assert 0 <= int(three.min()) and int(three.max()) < V
    assert not torch.equal(three, zero), 'scale 3 moved no token'
    print(f'use_cache=False: {int((three != zero).sum())} of {zero.numel()} tokens differ between scale 3 and scale 0; '
          f'{int((zero != unguided).sum())} between scale 0 and the unguided call')


def test_negative_text_equal_to_the_text_makes_both_branches_one(artv):
    m, text, vis = artv
    tokens, trace = traced(m, text, vis, pytest.MonkeyPatch, _race=stored_race(), guidance_scale=2.0, guidance_drop=(), negative_text=text)
    assert len(trace) == m.target_seq_len
    for n, r in enumerate(trace):
        assert torch.equal(bits(r['logits'][B:]), bits(r['logits'][:B])), f'token {n}'
    other = text.roll(1, 0)
    _, trace = traced(m, text, vis, pytest.MonkeyPatch, _race=stored_race(), guidance_scale=2.0, guidance_drop=(), negative_text=other)
    assert not torch.equal(trace[0]['logits'][B:], trace[0]['logits'][:B])  # (a negative prompt of its own is read)


def test_sampling_probs_of_the_guided_value(artv):
    m = artv[0]
    gen = torch.Generator().manual_seed(87)
    lc, lu = 3 * torch.randn(5, V, generator=gen).to(DEV), 3 * torch.randn(5, V, generator=gen).to(DEV)
    scale = torch.tensor([0.0, 2.0, -0.5, 7.5, 2.0], device=DEV)
    g = composed(lc, lu, scale)
    probs = m.sampling_probs(lc, temperature=0.8, logits_u=lu, guidance_scale=scale)
    assert torch.equal(probs, torch.softmax(g / 0.8, dim=-1))
    probs = m.sampling_probs(lc, temperature=0.8, top_k=8, logits_u=lu, guidance_scale=2.0)
    g2 = composed(lc, lu, torch.full((5, ), 2.0, device=DEV))
    assert bool(((probs > 0).sum(1) == 8).all())
    assert torch.equal((probs > 0), torch.zeros_like(g2, dtype=torch.bool).scatter_(1, g2.topk(8).indices, True))
    with pytest.raises(ValueError, match='come together'):
        m.sampling_probs(lc, logits_u=lu)


# ------------------------------------------------------------------------------------------------------- 4. the training drop
# (the losses are compared bit for bit, so the forwards run in the deterministic mode: outside it the cross-entropy adds its rows with
# fp32 atomics in a free order, and two forwards of the same ids may differ in the last bits)
def test_forward_with_injected_drop_decisions(artv):
    m, text, vis = artv
    fe = m.frontend
    target = torch.randint(0, 256, (B, m.target_seq_len), generator=torch.Generator().manual_seed(88)).to(DEV)
    inject = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=torch.uint8)  # the four combinations
    text_d, vis_d = text.clone(), vis.clone()
    text_d[inject[:, 0].bool().to(DEV)] = 0
    vis_d[inject[:, 1].bool().to(DEV)] = -1

    def counter():
        return 0.0 if fe.state is None else float(fe.state[0])

    with torch.no_grad(), mmvid_amd.deterministic():
        fe.last_null = None
        at = counter()
        plain = m(text, visual=vis, target=target, return_loss=True)[0]
        off = m(text, visual=vis, target=target, return_loss=True, null_text_prob=0.0, null_visual_prob=0.0)[0]
        assert fe.last_null is None and counter() == at, 'a forward with the drop off launched cond_drop or advanced the counter'
        want = m(text_d, visual=vis_d, target=target, return_loss=True)[0]
        assert counter() == at
        got = m(text, visual=vis, target=target, return_loss=True, _null=inject)[0]
        assert counter() == at + 1, 'the forward with the drop on did not advance the front-end counter by one'
        assert torch.equal(fe.last_null.cpu(), inject)
        again = m(text, visual=vis, target=target, return_loss=True, null_text_prob=0.5, null_visual_prob=0.5, _null=inject)[0]
        assert counter() == at + 2
    assert torch.equal(bits(off), bits(plain))
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(again), bits(want)), (float(got), float(want))
    assert not torch.equal(want, plain)  # (the drop changed the loss)
    assert bool(torch.isfinite(got))


def test_forward_with_free_running_drop_decisions(artv):
    """Probability 1 on both streams drops everything; the decisions of two calls differ once the counter has moved."""
    m, text, vis = artv
    fe = m.frontend
    target = torch.randint(0, 256, (B, m.target_seq_len), generator=torch.Generator().manual_seed(89)).to(DEV)
    with torch.no_grad(), mmvid_amd.deterministic():
        want = m(torch.zeros_like(text), visual=None, target=target, return_loss=True)[0]
        got = m(text, visual=vis, target=target, return_loss=True, null_text_prob=1.0, null_visual_prob=1.0)[0]
        assert bool(fe.last_null.bool().all()) and torch.equal(bits(got), bits(want))
        seen = []
        for _ in range(6):
            m(text, visual=vis, target=target, return_loss=True, null_text_prob=0.5, null_visual_prob=0.5)
            seen.append(fe.last_null.cpu().clone())
    assert any(not torch.equal(s, seen[0]) for s in seen[1:]), 'six steps at probability 0.5 repeated one set of decisions'
