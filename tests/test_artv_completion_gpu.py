"""ART-V video prediction on the device: DALLE.generate_images(given=(mask, tokens)), completion.complete_artv and
long_video.generate_long_artv on the tiny model (dim 768, 2 layers, 16 text positions, one visual, 4 targets of 16 tokens on 64 x 64
frames, 256 codes, seeded random weights).  Known frames come back verbatim; every generated token is restated from its own trace record
(the race on the recorded logits and variates, the embedding row at the position the token stands at, the logits against the full
forward over the same prefix within the bound of the cached-against-recomputed tests, tests/test_parity_gpu.py: relative error 2e-2)."""
import pytest
import torch

from conftest import relerr
from guarded import bits, report_mismatch
from test_host_logic import tiny_vae
from test_truncate_gpu import artv_tokens

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, TT, T, N, V = 3, 16, 4, 16, 256
CACHED_VS_RECOMPUTED = 2e-2  # tests/test_parity_gpu.py::test_config5_full_size_artv_forward_and_cached_decode (and test_models_gpu.py's tiny form)
MASKS = ('1000', '1100', '1110', '1010', '0110')


def row(mask):
    return torch.tensor([int(c) for c in mask], dtype=torch.uint8)


def known_columns(mask):
    """bool [T * N] on the device: the columns of the target sequence under a known frame."""
    return row(mask).bool().repeat_interleave(N).to(DEV)


@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(93)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=T, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(94)
    text = torch.randint(1, 49408, (2 * B, TT), generator=gen)
    text[1, 11:] = 0
    vis = torch.randint(0, V, (2 * B, N), generator=gen)
    known = torch.randint(0, V, (2 * B, T * N), generator=gen)
    return m, text.to(DEV), vis.to(DEV), known.to(DEV)


def stacked_race(rows, seed=95):
    """A `_race` whose variates for a call of fewer rows are the first rows of those for `rows` rows, by name; `.names`: the names asked for."""
    gen, store = torch.Generator().manual_seed(seed), {}

    def race(name, shape):
        if name not in store:
            store[name] = torch.empty(rows, shape[1]).exponential_(generator=gen).to(DEV)
        return store[name][:shape[0]]
    race.names = store
    return race


def run(m, text, vis, **kw):
    """generate_images -> the token sequence [rows, T * N] it decoded."""
    with pytest.MonkeyPatch.context() as mp:
        return artv_tokens(m, text, vis, mp, **kw)


def restate(m, text, vis, mask, tokens, trace, *, truncated=False, scale=None, what=''):
    """Every record of a traced call with the frame mask `mask` against its own content and against the full forward (see the module's
    docstring).  text / vis: the rows the tower ran (2b under guidance, with `scale` [b]); tokens [b, T * N]: the call's result."""
    from mmvid_amd import ops
    from test_guidance_gpu import composed
    b = tokens.shape[0]
    cl = m.control_seq_len
    c0, c1 = m._allowed_range(cl)
    flags = [c == '1' for c in mask for _ in range(N)]
    js = [j for j in range(T * N) if not flags[j]]
    assert len(trace) == len(js), f'{what}: {len(trace)} records for {len(js)} generated tokens'
    pos_rows, table = m._pos_rows().detach(), m.image_emb.weight.detach()
    run_start = [j for j in js if j == 0 or flags[j - 1]]
    compare = set()
    for j0 in run_start:  # the first token after every known run (and of a run at the start), and two more tokens of the run
        compare |= {j0, j0 + 5, j0 + N - 1}
    worst = 0.0
    for rec, j in zip(trace, js):
        lc = rec['logits'][:b]
        if truncated:
            lg = rec['logits_t']
        elif scale is not None:
            lg = composed(lc, rec['logits'][b:], scale)
        else:
            assert 'logits_t' not in rec
            lg = lc
        want, _ = ops.sample_race(lg.contiguous(), rec['E'], None, 0.0, want_y=False)
        report_mismatch(rec['tok'].cpu(), want.cpu(), f'{what} token {j}: the race on the record\'s own logits and variates')
        assert torch.equal(tokens[:, j], rec['tok']), f'{what} token {j}: the returned token is not the recorded one'
        last_of_run = j == T * N - 1 or flags[j + 1]
        assert ('x_in' in rec) == (not last_of_run), f'{what} token {j}: the last token of a run is embedded by the prefill, every other by the loop'
        if not last_of_run:
            x = table[rec['tok']] + pos_rows[cl + 1 + j]
            for half in range(rec['x_in'].shape[0] // b):
                assert torch.equal(bits(rec['x_in'][half * b:(half + 1) * b]), bits(x)), f'{what} token {j}: x_in is not image_emb[tok] + pos_rows[{cl + 1 + j}]'
        if j in compare:
            target = tokens[:, :j] if rec['logits'].shape[0] == b else tokens[:, :j].repeat(2, 1)
            full = m(text, visual=vis, target=target)[:, -1, c0:c1]
            e = relerr(rec['logits'].cpu(), full.cpu())
            worst = max(worst, e)
            assert e <= CACHED_VS_RECOMPUTED, f'{what} token {j}: cached logits against the full forward over the same prefix: relerr {e}'
    assert compare <= set(js)
    print(f'{what}: {len(js)} tokens restated, {len(compare)} logit rows against the full forward, worst relative error {worst:.3e}')


# ---------------------------------------------------------------------------------------------------------------- 1, 4: B = 3, traced
@pytest.fixture(scope='module')
def traced_runs(artv):
    """One traced call per mask at B = 3 under one `_race` (shared by the tests below, which leave it unchanged)."""
    m, text, vis, known = artv
    race = stacked_race(2 * B)
    out = {}
    for mask in MASKS:
        trace = []
        out[mask] = (run(m, text[:B], vis[:B], given=(row(mask), known[:B]), _race=race, _trace=trace), trace)
    return race, out


@pytest.mark.parametrize('mask', MASKS)
def test_known_frames_come_back_verbatim(artv, traced_runs, mask):
    known = artv[3][:B]
    tokens, _ = traced_runs[1][mask]
    cols = known_columns(mask)
    assert tokens.shape == (B, T * N) and tokens.dtype == torch.int64
    report_mismatch(tokens[:, cols].cpu(), known[:, cols].cpu(), f'mask {mask}: the known columns of the result against the given tokens')
    assert 0 <= int(tokens.min()) and int(tokens.max()) < V
    assert not torch.equal(tokens[:, ~cols], known[:, ~cols])  # (the unknown columns were drawn, not copied)


@pytest.mark.parametrize('mask', MASKS)
def test_every_generated_token_is_its_records_restatement(artv, traced_runs, mask):
    m, text, vis, _ = artv
    tokens, trace = traced_runs[1][mask]
    restate(m, text[:B], vis[:B], mask, tokens, trace, what=f'mask {mask}')


def test_known_positions_consume_no_variates(artv, traced_runs):
    race = traced_runs[0]
    asked = set(race.names)
    for mask in MASKS:
        cols = known_columns(mask).tolist()
        assert {f'tok{j}' for j in range(T * N) if not cols[j]} <= asked
    always_known = [j for j in range(T * N) if all(known_columns(mask)[j] for mask in MASKS)]
    assert not always_known or not ({f'tok{j}' for j in always_known} & asked)
    names = []
    m, text, vis, known = artv
    run(m, text[:B], vis[:B], given=(row('0110'), known[:B]), _race=lambda name, shape: (names.append(name), race(name, shape))[1])
    assert names == [f'tok{j}' for j in list(range(N)) + list(range(3 * N, 4 * N))]


# ------------------------------------------------------------------------------------------------------------------------ 2, 3
def test_all_known_draws_nothing(artv):
    m, text, vis, known = artv
    called = []
    tokens = run(m, text[:B], vis[:B], given=(row('1111'), known[:B]), _race=lambda name, shape: called.append(name))
    assert torch.equal(tokens, known[:B]) and not called
    tokens = run(m, text[:B], vis[:B], given=(row('1111'), known[:B]), use_cache=False, _race=lambda name, shape: called.append(name))
    assert torch.equal(tokens, known[:B]) and not called


def test_nothing_known_is_the_plain_call(artv):
    m, text, vis, known = artv
    race = stacked_race(B, seed=96)
    plain = run(m, text[:B], vis[:B], _race=race)
    given = run(m, text[:B], vis[:B], given=(torch.zeros(B, T, dtype=torch.bool), known[:B]), _race=race)
    report_mismatch(given.cpu(), plain.cpu(), 'given with an all-zero mask against the call without given')
    torch.manual_seed(97)
    a = run(m, text[:B], vis[:B])  # production: pre-drawn variates, captured step
    torch.manual_seed(97)
    b = run(m, text[:B], vis[:B], given=(row('0000'), known[:B]))
    assert torch.equal(a, b)


def test_the_reference_loop_appends_known_frames_without_drawing(artv):
    """use_cache=False (the whole prefix per token): known frames join the prefix as they are, guided and unguided."""
    m, text, vis, known = artv
    cols = known_columns('1010')
    want = [f'tok{j}' for j in list(range(N, 2 * N)) + list(range(3 * N, 4 * N))]
    for kw in ({}, dict(guidance_scale=2.0)):
        names = []
        race = stacked_race(2, seed=106)
        tokens = run(m, text[:2], vis[:2], given=(row('1010'), known[:2]), use_cache=False, top_k=1, **kw,
                     _race=lambda name, shape: (names.append(name), race(name, shape))[1])
        assert tokens.shape == (2, T * N) and torch.equal(tokens[:, cols], known[:2][:, cols]), kw
        assert names == want and 0 <= int(tokens.min()) and int(tokens.max()) < V, kw


# -------------------------------------------------------------------------------------------------------------------- 5: B = 2
@pytest.mark.parametrize('mask', ['1000', '1010'])
def test_batch_2_without_a_trace(artv, mask):
    """Production at batch 2: the one-launch token per run where the device allows it (a timed-out poll falls back by design: tokens only)."""
    m, text, vis, known = artv
    cols = known_columns(mask)
    torch.manual_seed(98)
    a = run(m, text[:2], vis[:2], given=(row(mask), known[:2]))
    torch.manual_seed(98)
    b = run(m, text[:2], vis[:2], given=(row(mask), known[:2]))
    assert a.shape == (2, T * N) and torch.equal(a[:, cols], known[:2][:, cols])
    assert 0 <= int(a.min()) and int(a.max()) < V
    report_mismatch(b.cpu(), a.cpu(), f'mask {mask}: two calls under one torch seed')


# --------------------------------------------------------------------------------------------------------- 6: two masks, one batch
def test_two_masks_in_one_batch(artv):
    """Rows 0 and 2 know frames 0-1, row 1 frames 0 and 2.  Greedy (top_k = 1), so the variates do not matter: the mixed production call
    equals each group's traced call, which is restated; then sampled: the mixed call equals the chain of its groups' calls on one generator."""
    m, text, vis, known = artv
    masks = ['1100', '1010', '1100']
    mixed = torch.stack([row(k) for k in masks])
    groups = [('1100', [0, 2]), ('1010', [1])]
    tokens = run(m, text[:B], vis[:B], given=(mixed, known[:B]), top_k=1)
    assert tokens.shape == (B, T * N)
    for mask, rows in groups:
        cols = known_columns(mask)
        assert torch.equal(tokens[rows][:, cols], known[rows][:, cols]), f'rows {rows}: known columns'
        trace = []
        alone = run(m, text[rows], vis[rows], given=(row(mask), known[rows]), top_k=1, _race=stacked_race(B), _trace=trace)
        report_mismatch(tokens[rows].cpu(), alone.cpu(), f'rows {rows} of the mixed call against the call of the group alone (both greedy)')
        restate(m, text[rows], vis[rows], mask, alone, trace, truncated=True, what=f'group {mask}')
    torch.manual_seed(99)
    sampled = run(m, text[:B], vis[:B], given=(mixed, known[:B]))
    torch.manual_seed(99)
    for mask, rows in groups:  # the groups in order of first appearance, as the mixed call runs them
        alone = run(m, text[rows], vis[rows], given=(row(mask), known[rows]))
        report_mismatch(sampled[rows].cpu(), alone.cpu(), f'rows {rows} of the sampled mixed call against the group alone on the same generator')
        cols = known_columns(mask)
        assert torch.equal(sampled[rows][:, cols], known[rows][:, cols])
    assert 0 <= int(sampled.min()) and int(sampled.max()) < V


# ------------------------------------------------------------------------------------------------------------------- 7: guidance
def test_guidance_at_scale_zero_equals_the_unguided_call_on_the_stacked_batch(artv):
    """The form of tests/test_artv_guidance_gpu.py: rows 0..B-1 of the unguided call on [text; 0], [vis; -1] against the guided call at
    scale 0 on the same variates (rests on the tower being independent from row to row at a fixed batch)."""
    m, text, vis, known = artv
    text, vis, known = text[:B], vis[:B], known[:B]
    mask = '1010'
    race = stacked_race(2 * B, seed=100)
    text2, vis2 = torch.cat((text, torch.zeros_like(text))), torch.cat((vis, torch.full_like(vis, -1)))
    trace_s, trace_g = [], []
    stacked = run(m, text2, vis2, given=(row(mask), known.repeat(2, 1)), _race=race, _trace=trace_s)
    guided = run(m, text, vis, given=(row(mask), known), _race=race, _trace=trace_g, guidance_scale=0.0)
    assert len(trace_s) == len(trace_g) == 2 * N and guided.shape == (B, T * N)
    for n, (g, s) in enumerate(zip(trace_g, trace_s)):
        assert g['logits'].shape == (2 * B, V) and torch.equal(g['E'], s['E'][:B])
        report_mismatch(g['tok'].cpu(), s['tok'][:B].cpu(), f'record {n}: guided at scale 0 against rows 0..B-1 of the stacked unguided call')
        if 'x_in' in g:
            assert torch.equal(bits(g['x_in'][B:]), bits(g['x_in'][:B])), f'record {n}: both halves carry the drawn token'
    report_mismatch(trace_g[0]['logits'].cpu(), trace_s[0]['logits'].cpu(), 'the first token after the known frame: both halves of the prefill')
    report_mismatch(guided.cpu(), stacked[:B].cpu(), 'the decoded sequences')
    cols = known_columns(mask)
    assert torch.equal(guided[:, cols], known[:, cols]) and torch.equal(stacked[:, cols], known.repeat(2, 1)[:, cols])
    scale = torch.tensor([2.0, 0.0, -0.5], device=DEV)
    trace = []
    tokens = run(m, text, vis, given=(row(mask), known), _race=race, _trace=trace, guidance_scale=scale)
    restate(m, torch.cat((text, torch.zeros_like(text))), torch.cat((vis, torch.full_like(vis, -1))), mask, tokens, trace, scale=scale,
            what='guided, scales 2 / 0 / -0.5')
    report_mismatch(tokens[1].cpu(), guided[1].cpu(), 'the video at scale 0 against its tokens at scale 0 for every video')


# ---------------------------------------------------------------------------------------------------------------------- 8: top_k
def test_top_k_with_given(artv):
    m, text, vis, known = artv
    mask = '1100'
    trace = []
    tokens = run(m, text[:B], vis[:B], given=(row(mask), known[:B]), top_k=5, _race=stacked_race(B, seed=101), _trace=trace)
    for rec in trace:
        assert int(rec['kept'].max()) <= 5 and torch.equal(rec['kept'], torch.isfinite(rec['logits_t']).sum(1).to(torch.int32))
        top = rec['logits'].topk(5).indices
        assert bool((rec['tok'].view(-1, 1) == top).any(1).all())  # the token is one of its row's five largest logits
    restate(m, text[:B], vis[:B], mask, tokens, trace, truncated=True, what='top_k = 5')
    cols = known_columns(mask)
    assert torch.equal(tokens[:, cols], known[:B][:, cols])
    # production: captured, greedy, against the eager call
    produced = run(m, text[:B], vis[:B], given=(row(mask), known[:B]), top_k=1)
    eager = run(m, text[:B], vis[:B], given=(row(mask), known[:B]), top_k=1, _race=stacked_race(B, seed=102))
    report_mismatch(produced.cpu(), eager.cpu(), 'top_k = 1 with given: the captured step against the eager one (both greedy)')


# -------------------------------------------------------------------------------------------------------------- 9: complete_artv
def test_complete_artv_on_fp32_frames(artv):
    from mmvid_amd import completion, ops
    m, text, vis, _ = artv
    gen = torch.Generator().manual_seed(103)
    frames = torch.rand(B, T, 3, 64, 64, generator=gen).to(DEV)
    given = torch.tensor([[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.bool)
    torch.manual_seed(104)
    out, tokens = completion.complete_artv(m, text[:B], frames, given, visual=vis[:B])
    assert out.shape == (B, T, 64, 64, 3) and out.dtype == torch.uint8 and tokens.shape == (B, T * N) and tokens.dtype == torch.int64
    real = ops.frames_to_u8(frames.view(B * T, 3, 64, 64)).view(B, T, 64, 64, 3)
    decoded = ops.frames_to_u8(m.vae.decode(tokens.reshape(B * T, N))).view(B, T, 64, 64, 3)
    own = m.get_image_tokens(frames, reshape=True).view(B, T, N)
    g = given.to(DEV)
    assert torch.equal(out[g], real[g]), 'known frames are not the input\'s own bytes'
    assert torch.equal(out[~g], decoded[~g]), 'generated frames are not the decode of the returned tokens'
    assert torch.equal(tokens.view(B, T, N)[g], own[g]), 'known frames did not keep the tokens of their pixels'
    assert not torch.equal(real[g], decoded[g])  # (the paste is visible: the tiny VQGAN does not reproduce noise)
    torch.manual_seed(104)
    plain, tokens2 = completion.complete_artv(m, text[:B], frames, given, visual=vis[:B], paste=False)
    assert torch.equal(tokens2, tokens) and torch.equal(plain, decoded)
    torch.manual_seed(104)
    out3, tokens3 = completion.complete_artv(m, text[:B], tokens, given, visual=vis[:B])  # token input: nothing to paste
    assert torch.equal(tokens3, tokens) and torch.equal(out3, decoded)


# --------------------------------------------------------------------------------------------------------- 10: generate_long_artv
def test_generate_long_artv_equals_the_chain_of_windows(artv):
    from mmvid_amd import long_video, ops
    m, text, vis, _ = artv
    text, vis = text[:B], vis[:B]
    race = stacked_race(B, seed=105)
    frames, tokens = long_video.generate_long_artv(m, text, visual=vis, t_repeat=3, t_overlap=1, _race=race)
    assert tokens.shape == (B, T + 2 * (T - 1), N) and frames.shape == (B, 10, 64, 64, 3) and frames.dtype == torch.uint8
    chain, prev = [], None
    for k in range(3):
        prefixed = (lambda k: lambda name, shape: race(f'L{k}c0/{name}', shape))(k)
        if prev is None:
            win = run(m, text, vis, _race=prefixed)
        else:
            start = torch.zeros(B, T * N, dtype=torch.long, device=DEV)
            start[:, :N] = prev[:, (T - 1) * N:]
            win = run(m, text, vis, given=(row('1000'), start), _race=prefixed)
            assert torch.equal(win[:, :N], prev[:, (T - 1) * N:])
        chain.append(win.view(B, T, N) if prev is None else win.view(B, T, N)[:, 1:])
        prev = win
    report_mismatch(tokens.cpu(), torch.cat(chain, 1).cpu(), 'generate_long_artv against the chain of per-window generate_images(given=...) calls')
    assert torch.equal(frames.view(-1, 64, 64, 3), ops.frames_to_u8(m.vae.decode(tokens.reshape(-1, N))))
    assert sorted(race.names) == sorted([f'L0c0/tok{j}' for j in range(T * N)] + [f'L{k}c0/tok{j}' for k in (1, 2) for j in range(N, T * N)])
