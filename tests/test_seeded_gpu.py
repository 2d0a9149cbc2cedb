"""Seeded sampling on the device (csrc/variates.hip, mmvid_amd/seeded.py, the `seeds` keyword of both samplers).

1. the fill kernel against the host replica (tests/variates_ref.py) through guarded and poisoned buffers: uniforms bit for bit, Exp(1)
   within the bound of logf; 2. a video's block does not depend on where it is filled; 3. BERT mask-predict, 4. ART-V, 5. long videos:
   a video's tokens do not depend on its row, its batch mates or the chunking, and `seeds` is exactly "`_race` filled by the kernel";
6. `seeds=None` is untouched and a seeded call leaves torch's generators alone.  Every token comparison is an equality."""
import numpy as np
import pytest
import torch

import variates_ref as R
from guarded import Guarded, call_abi, report_mismatch
from test_host_logic import tiny_vae
from test_long_video_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HIGH = (0x5EADBEEF << 32) | 17  # a seed with a non-zero high word
SEEDS = [HIGH, 5, 2**63 - 1]
SUBS = [3, 0, (2 << 16) | 1]
# The bound of the Exp(1) variates.  No HIP math accuracy table ships with the ROCm installation the tests were written on, so this
# is the fallback the specification names: the OpenCL full-profile bound for `log`, <= 3 ulp (The OpenCL C Specification 3.0, section
# 7.4 "Relative error as ULPs", table "ULP values for single precision built-in math functions": log 3 ulp), taken against -log in fp64
# of the exact argument, ulp as that section defines it for the infinitely precise result.  The negation is exact.
LOGF_ULP = 3.0


# ----------------------------------------------------------------------------------------------------------- 1. the kernel
def fill_guarded(seeds, sub, rpv, n, purpose, kind, draw_first, draws, draw_dev=None):
    """mmvid_variates_fill with every operand in a guarded buffer -> out [draws, videos * rpv, n] float32 (host)."""
    videos = len(seeds)
    gS = Guarded(torch.tensor(seeds, dtype=torch.int64), role='in')
    gU = None if sub is None else Guarded(torch.tensor(sub, dtype=torch.int32), role='in')
    gD = None if draw_dev is None else Guarded(torch.tensor([draw_dev], dtype=torch.int32), role='in')
    gO = Guarded(role='out', shape=(draws, videos * rpv, n), dtype=torch.float32)
    call_abi('mmvid_variates_fill', gS.ptr, None if gU is None else gU.ptr, videos, rpv, n, purpose, kind, None if gD is None else gD.ptr,
             draw_first, draws, gO.ptr)
    for g, what in ((gS, 'seeds'), (gU, 'substream'), (gD, 'draw_dev')):
        if g is not None:
            g.check(f'variates_fill {what}')
    return gO.check('variates_fill out')


def check_against_replica(got, w24, kind, what):
    got = got.numpy()
    if kind == R.UNIFORM:
        report_mismatch(torch.from_numpy(got), torch.from_numpy(R.uniform_of(w24)), f'{what}: uniforms against the replica')
        assert got.min() >= 0.0 and got.max() < 1.0
        return
    want = R.exp1_of(w24)
    assert np.isfinite(got).all() and got.min() >= 0.0, f'{what}: an Exp(1) variate is negative or not finite'
    err = np.abs(got.astype(np.float64) - want) / R.ulp32(want)
    print(f'{what}: worst Exp(1) error {err.max():.3f} ulp (bound {LOGF_ULP})')
    assert err.max() <= LOGF_ULP, f'{what}: {err.max():.2f} ulp from -log in fp64'
    assert (got[w24 == 2**24 - 1] == 0.0).all()


@pytest.mark.parametrize('videos', [1, 3])
@pytest.mark.parametrize('rpv', [1, 5])
@pytest.mark.parametrize('n', [1, 3, 64, 1026])
def test_fill_matches_the_replica(n, rpv, videos):
    """rpv * n = 64 and 320 take the 16-byte stores, every other size the dword stores with a ragged last Philox block; 5 rows of 3
    put row starts inside a block; 1026 and 5130 need more than one 256-thread block per segment."""
    seeds = SEEDS[:videos]
    case = 0
    for draws, draw_first, sub in ((1, 0, None), (4, 1023, SUBS[:videos]), (1, 1023, SUBS[:videos]), (4, 0, None)):
        for kind in (R.UNIFORM, R.EXP1):
            purpose = 1 + case % 3
            case += 1
            got = fill_guarded(seeds, sub, rpv, n, purpose, kind, draw_first, draws)
            w24 = R.block_words(seeds, sub, rpv, n, purpose, draw_first, draws)
            check_against_replica(got, w24, kind, f'n={n} rpv={rpv} videos={videos} draws={draws} first={draw_first} sub={sub} purpose={purpose}')


def test_device_draw_number_equals_the_host_scalar():
    """draw_dev = 7 against draw_first = 7, and draw_dev + draw_first with a negative draw_first (the captured ART-V step passes
    tok0 - first_pos < 0 and the position)."""
    for kind in (R.UNIFORM, R.EXP1):
        host = fill_guarded(SEEDS, SUBS, 5, 3, R.TOKEN_RACE, kind, 7, 1)
        dev = fill_guarded(SEEDS, SUBS, 5, 3, R.TOKEN_RACE, kind, 0, 1, draw_dev=7)
        report_mismatch(dev, host, f'draw_dev = 7 against draw_first = 7, kind {kind}')
        shifted = fill_guarded(SEEDS, SUBS, 5, 3, R.TOKEN_RACE, kind, -18, 1, draw_dev=25)
        report_mismatch(shifted, host, f'draw_dev = 25, draw_first = -18 against draw 7, kind {kind}')
        check_against_replica(host, R.block_words(SEEDS, SUBS, 5, 3, R.TOKEN_RACE, 7, 1), kind, 'draw 7')


def test_exp1_is_zero_at_the_largest_word_and_finite_at_the_smallest():
    """Variate 672 of (seed 12345, token race, substream 0, draw 16831) has w >> 8 = 2^24 - 1 (found by a search with the replica):
    the argument of logf is exactly 1 and E exactly 0.  The smallest word any of these 4 x 4096 variates has gives the largest E."""
    seed, draw, i = 12345, 16831, 672
    assert int(R.words(seed, R.TOKEN_RACE, 0, draw, 1, first=i)[0]) == 2**24 - 1
    got = fill_guarded([seed], None, 1, 4096, R.TOKEN_RACE, R.EXP1, draw - 1, 4)
    w24 = R.block_words([seed], None, 1, 4096, R.TOKEN_RACE, draw - 1, 4)
    assert float(got[1, 0, i]) == 0.0 and int(w24[1, 0, i]) == 2**24 - 1
    check_against_replica(got, w24, R.EXP1, 'the block around the largest word')
    assert float(got.max()) <= 24 * np.log(2.0) * (1 + 2.0**-22)


def test_unaligned_output_takes_the_dword_stores():
    """rows_per_video * n % 4 == 0 on a pointer that is 4 bytes past a 16-byte boundary, through ops.variates_fill."""
    from mmvid_amd import ops
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=DEV)
    buf = torch.full((4 + 2 * 3 * 2 * 64 + 4, ), -1.0, device=DEV)
    out = buf[1:1 + 2 * 3 * 2 * 64].view(2, 6, 64)
    assert out.data_ptr() % 16 == 4
    ops.variates_fill(out, seeds, 2, R.KEEP_RACE, R.UNIFORM, draw_first=9)
    torch.cuda.synchronize()
    want = torch.from_numpy(R.uniform_of(R.block_words(SEEDS, None, 2, 64, R.KEEP_RACE, 9, 2)))
    report_mismatch(out.cpu(), want, 'unaligned output')
    assert buf[0].item() == -1.0 and bool((buf[1 + 2 * 3 * 2 * 64:] == -1.0).all())


# ------------------------------------------------------------------------------------------- 2. placement independence
@pytest.mark.parametrize('kind', [R.UNIFORM, R.EXP1])
def test_a_videos_block_does_not_depend_on_where_it_is_filled(kind):
    """(seed, purpose, draw) alone as row 0 of 1, as video 2 of 5, as block 2 of a draws = 4 launch and as a draws = 1 launch."""
    from mmvid_amd import ops
    rpv, n, draw = 5, 3, 40
    mates = torch.tensor([11, 22, HIGH, 33, 44], dtype=torch.int64, device=DEV)
    alone = ops.variates_fill(torch.empty(rpv, n, device=DEV), mates[2:3].contiguous(), rpv, R.TOKEN_NOISE, kind, draw_first=draw)
    five = ops.variates_fill(torch.empty(5 * rpv, n, device=DEV), mates, rpv, R.TOKEN_NOISE, kind, draw_first=draw)
    many = ops.variates_fill(torch.empty(4, 5 * rpv, n, device=DEV), mates, rpv, R.TOKEN_NOISE, kind, draw_first=draw - 2)
    report_mismatch(five[2 * rpv:3 * rpv].cpu(), alone.cpu(), 'video 2 of 5 against the video alone')
    report_mismatch(many[2, 2 * rpv:3 * rpv].cpu(), alone.cpu(), 'block 2 of a draws = 4 launch against a draws = 1 launch')
    report_mismatch(many[2].cpu(), five.cpu(), 'block 2 of a draws = 4 launch: all five videos')
    assert not torch.equal(many[1], many[2]) and not torch.equal(five[:rpv], five[rpv:2 * rpv])


# ----------------------------------------------------------------------------------------------------- 3. BERT mask-predict
T, N_TOK = 4, 16
A, Bs, C = 1001, HIGH, 77


@pytest.fixture(scope='module')
def bert():
    return build_model()


@pytest.fixture(scope='module')
def mp(golden):
    # the golden schedule with Bm = 2 candidates and a temperature that falls from 1 to 0 over the first ten steps (noise at steps 0-8)
    return dict(golden('mask_predict').meta['mp_config'], B=2, N1_t=1.0, N2_t=0.0)


@pytest.fixture(scope='module')
def bert_inputs(bert):
    gen = torch.Generator().manual_seed(41)
    text = torch.randint(1, 49408, (3, 16), generator=gen)
    text[0, 9:] = 0
    text = text.to(DEV)
    with torch.no_grad():
        return text, bert(text, return_loss=False), bert(torch.zeros_like(text), return_loss=False)


VARIANTS = {'plain': {}, 'guided': dict(guidance_scale=1.5), 'truncated': dict(top_k=5)}


def bert_run(bert, mp, inputs, rows, seeds, variant, **kw):
    _, control, uncond = inputs
    idx = torch.tensor(rows, device=DEV)
    extra = dict(VARIANTS[variant])
    if variant == 'guided':
        extra['uncond_emb'] = uncond.index_select(0, idx)
    return bert.mask_predict(control.index_select(0, idx), dynamic=False, steps=4, mp_config=mp, seeds=seeds, **extra, **kw)[0]


@pytest.fixture(scope='module')
def bert_batches(bert, mp, bert_inputs):
    """The b = 3 run of every variant, with its trace; shared and left unchanged."""
    out = {}
    for variant in VARIANTS:
        trace = []
        out[variant] = (bert_run(bert, mp, bert_inputs, [0, 1, 2], [A, Bs, C], variant, _trace=trace), trace)
    return out


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_bert_video_alone_and_reordered(bert, mp, bert_inputs, bert_batches, variant):
    batch, trace = bert_batches[variant]
    assert batch.shape == (3, T * N_TOK) and len(trace) == 4
    for i, seed in enumerate([A, Bs, C]):
        alone = bert_run(bert, mp, bert_inputs, [i], [seed], variant)
        report_mismatch(alone.cpu(), batch[i:i + 1].cpu(), f'{variant}: video {i} alone against video {i} of the batch')
    moved = bert_run(bert, mp, bert_inputs, [2, 0, 1], [C, A, Bs], variant)
    report_mismatch(moved.cpu(), batch[[2, 0, 1]].cpu(), f'{variant}: the batch in the order (c, a, b)')
    again = bert_run(bert, mp, bert_inputs, [0, 1, 2], torch.tensor([A, Bs, C]), variant)  # (a tensor of seeds; and the process history)
    assert torch.equal(again, batch)


def test_bert_seeds_are_race_filled_by_the_kernel(bert, mp, bert_inputs, bert_batches):
    """The variates the seeded run's trace recorded (the noise, which the trace does not keep, re-filled by the hook), injected through
    `_race`: the same tokens.  And the recorded variates are the replica's, placed by video."""
    from mmvid_amd import seeded
    batch, trace = bert_batches['plain']
    _, control, _ = bert_inputs
    refill = seeded.SeededRace([A, Bs, C], DEV)
    asked = []

    def race(name, shape):
        asked.append(name)
        purpose, _, t = seeded.parse_name(name)
        got = refill(name, shape) if purpose == R.TOKEN_NOISE else trace[t]['E_tok' if purpose == R.TOKEN_RACE else 'E_keep']
        assert tuple(got.shape) == tuple(shape)
        return got

    replayed = bert.mask_predict(control, dynamic=False, steps=4, mp_config=mp, _race=race)[0]
    report_mismatch(replayed.cpu(), batch.cpu(), 'the seeded run replayed through _race')
    assert sorted(asked) == sorted([f'tok{t}' for t in range(4)] + [f'tok{t}_noise_u' for t in range(4)] + [f'keep{t}' for t in range(1, 4)])
    V = bert.num_image_tokens
    want = R.exp1_of(R.block_words([A, Bs, C], None, 2 * T * N_TOK, V, R.TOKEN_RACE, 2, 1))[0]
    got = trace[2]['E_tok'].cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and (np.abs(got - want) <= LOGF_ULP * R.ulp32(want)).all()
    want = R.exp1_of(R.block_words([A, Bs, C], None, 2, T * N_TOK, R.KEEP_RACE, 3, 1))[0]
    got = trace[3]['E_keep'].cpu().numpy().astype(np.float64).reshape(want.shape)
    assert (np.abs(got - want) <= LOGF_ULP * R.ulp32(want)).all()


def test_bert_a_changed_seed_changes_that_video_only(bert, mp, bert_inputs, bert_batches):
    batch, _ = bert_batches['plain']
    other = bert_run(bert, mp, bert_inputs, [0, 1, 2], [A, Bs + 1, C], 'plain')
    assert torch.equal(other[0], batch[0]) and torch.equal(other[2], batch[2])
    assert not torch.equal(other[1], batch[1])


# ------------------------------------------------------------------------------------------------------------------ 4. ART-V
TT, V_ART = 16, 256
ART_SEEDS = [901, HIGH, 903, 904, 905, 906, 907, 908]


@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(43)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=T, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(44)
    text = torch.randint(1, 49408, (8, TT), generator=gen)
    text[1, 11:] = 0
    vis = torch.randint(0, V_ART, (8, N_TOK), generator=gen)
    known = torch.randint(0, V_ART, (8, T * N_TOK), generator=gen)
    return m, text.to(DEV), vis.to(DEV), known.to(DEV)


def art_run(artv, videos, **kw):
    m, text, vis, _ = artv
    idx = torch.tensor(videos, device=DEV)
    return m.sample_tokens(text.index_select(0, idx), visual=vis.index_select(0, idx), seeds=[ART_SEEDS[v] for v in videos], **kw)[1]


@pytest.fixture(scope='module')
def art_batch(artv):
    """Videos 0-3 at B = 4 through the production path (captured step, one fill launch); shared and left unchanged."""
    return art_run(artv, [0, 1, 2, 3])


def test_artv_rows_permuted_among_other_batch_mates(artv, art_batch):
    assert art_batch.shape == (4, T * N_TOK) and 0 <= int(art_batch.min()) and int(art_batch.max()) < V_ART
    moved = art_run(artv, [5, 2, 0, 7])
    report_mismatch(moved[1:3].cpu(), art_batch[[2, 0]].cpu(), 'videos 2 and 0 in other rows, among other batch mates')
    assert not torch.equal(moved[0], art_batch[0]) and not torch.equal(art_batch[0], art_batch[1])
    report_mismatch(art_run(artv, [0, 1, 2, 3]).cpu(), art_batch.cpu(), 'the same call once more')


def test_artv_captured_step_equals_the_eager_one(artv, art_batch):
    """A trace takes the eager loop, whose draw fills the variates of one token per launch from the position on the device."""
    trace = []
    eager = art_run(artv, [0, 1, 2, 3], _trace=trace)
    assert len(trace) == T * N_TOK
    report_mismatch(eager.cpu(), art_batch.cpu(), 'the eager loop against the captured step')
    for j in (0, 17, T * N_TOK - 1):  # the recorded variates of token j are the replica's block j of each video
        want = R.exp1_of(R.block_words(ART_SEEDS[:4], None, 1, V_ART, R.TOKEN_RACE, j, 1))[0]
        got = trace[j]['E'].cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= LOGF_ULP * R.ulp32(want)).all(), j


def test_artv_per_step_fill_equals_the_one_launch_block(artv, art_batch, monkeypatch):
    from mmvid_amd import artv_sampling
    monkeypatch.setattr(artv_sampling, 'E_ALL_MAX', 0)  # no call fits: the captured step fills its own variates
    report_mismatch(art_run(artv, [0, 1, 2, 3]).cpu(), art_batch.cpu(), 'the per-step fill against the one-launch block')


def test_artv_batch_1_twice(artv):
    """The one-launch token at batch 1 reads the block filled from the seed."""
    a = art_run(artv, [1])
    b = art_run(artv, [1])
    assert a.shape == (1, T * N_TOK) and 0 <= int(a.min()) and int(a.max()) < V_ART
    report_mismatch(b.cpu(), a.cpu(), 'batch 1, two calls')
    assert not torch.equal(art_run(artv, [2]), a)


def test_artv_guided(artv):
    scale = torch.tensor([2.0, 0.5, 1.0], device=DEV)
    a = art_run(artv, [0, 1, 2], guidance_scale=scale)
    b = art_run(artv, [2, 0, 1], guidance_scale=scale[[2, 0, 1]])
    report_mismatch(b.cpu(), a[[2, 0, 1]].cpu(), 'guided: the batch reordered')
    trace = []
    eager = art_run(artv, [0, 1, 2], guidance_scale=scale, _trace=trace)
    report_mismatch(eager.cpu(), a.cpu(), 'guided: the eager loop against the captured step')


def test_artv_prediction_with_two_masks_in_the_batch(artv):
    """Rows 0 and 2 know frames 0-1, row 1 frames 0 and 2: the mixed call runs one pass per mask, each with the seeds of its rows, and
    equals the call of each group alone."""
    m, text, vis, known = artv
    masks = torch.tensor([[1, 1, 0, 0], [1, 0, 1, 0], [1, 1, 0, 0]], dtype=torch.uint8)
    mixed = art_run(artv, [0, 1, 2], given=(masks, known[:3]))
    for mask, rows in (([1, 1, 0, 0], [0, 2]), ([1, 0, 1, 0], [1])):
        alone = art_run(artv, rows, given=(torch.tensor(mask, dtype=torch.uint8), known[rows]))
        report_mismatch(mixed[rows].cpu(), alone.cpu(), f'rows {rows} of the mixed call against the group alone')
        cols = torch.tensor(mask).bool().repeat_interleave(N_TOK).to(DEV)
        assert torch.equal(mixed[rows][:, cols], known[rows][:, cols])
    # a generated position draws block (its index in the target sequence) of its video whatever the mask: the eager loop of one group
    trace = []
    art_run(artv, [0, 2], given=(torch.tensor([1, 1, 0, 0], dtype=torch.uint8), known[[0, 2]]), _trace=trace)
    assert len(trace) == 2 * N_TOK
    want = R.exp1_of(R.block_words([ART_SEEDS[0], ART_SEEDS[2]], None, 1, V_ART, R.TOKEN_RACE, 2 * N_TOK + 3, 1))[0]
    got = trace[3]['E'].cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= LOGF_ULP * R.ulp32(want)).all()


def test_complete_artv_with_seeds(artv):
    from mmvid_amd import completion
    m, text, vis, known = artv
    given = torch.tensor([[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.bool)
    kw = dict(visual=vis[:3], paste=False)
    _, a = completion.complete_artv(m, text[:3], known[:3], given, seeds=ART_SEEDS[:3], **kw)
    _, b = completion.complete_artv(m, text[:3], known[:3], given, seeds=ART_SEEDS[:3], **kw)
    _, c = completion.complete_artv(m, text[:3], known[:3], given, seeds=[ART_SEEDS[0], 4242, ART_SEEDS[2]], **kw)
    report_mismatch(b.cpu(), a.cpu(), 'complete_artv, two calls')
    g = given.repeat_interleave(N_TOK, 1).to(DEV)
    assert torch.equal(a[g], known[:3][g])
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and not torch.equal(c[1], a[1])


# ------------------------------------------------------------------------------------------------------------- 5. long videos
def test_generate_long_does_not_depend_on_max_rows_or_b(bert, mp, bert_inputs):
    from mmvid_amd import long_video as lv
    text = bert_inputs[0][:2]
    kw = dict(mode='interp', t_repeat=3, mask_predict_steps=4, mp_config=mp, decode=False)
    trace = []
    whole = lv.generate_long_seeded(bert, text, [A, Bs], trace=trace, **kw)[1]
    assert whole.shape == (2, 4 * T, N_TOK) and [r['rows'] for r in trace] == [[(0, 2)], [(0, 4)], [(0, 8)]]
    trace = []
    chunked = lv.generate_long_seeded(bert, text, [A, Bs], max_rows=3, trace=trace, **kw)[1]
    assert trace[2]['rows'] == [(0, 3), (3, 6), (6, 8)]
    report_mismatch(chunked.cpu(), whole.cpu(), 'generate_long: max_rows = 3 against one call per level')
    for i, seed in enumerate([A, Bs]):
        alone = lv.generate_long_seeded(bert, text[i:i + 1], [seed], **kw)[1]
        report_mismatch(alone.cpu(), whole[i:i + 1].cpu(), f'generate_long: video {i} at b = 1 against b = 2')
    assert not torch.equal(whole[0], lv.generate_long_seeded(bert, text[:1], [A + 1], **kw)[1][0])


def test_generate_long_artv_does_not_depend_on_max_rows_or_b(artv):
    """b = 1 and b = 2, and chunks of 1 and 2 rows: all on the one-launch-token side of the decode kernels' batch boundary."""
    from mmvid_amd import long_video as lv
    m, text, vis, _ = artv
    kw = dict(t_repeat=3, t_overlap=1, decode=False)
    whole = lv.generate_long_artv(m, text[:2], visual=vis[:2], seeds=ART_SEEDS[:2], **kw)[1]
    assert whole.shape == (2, T + 2 * (T - 1), N_TOK)
    chunked = lv.generate_long_artv(m, text[:2], visual=vis[:2], seeds=ART_SEEDS[:2], max_rows=1, **kw)[1]
    report_mismatch(chunked.cpu(), whole.cpu(), 'generate_long_artv: max_rows = 1 against one call per level')
    for i in range(2):
        alone = lv.generate_long_artv(m, text[i:i + 1], visual=vis[i:i + 1], seeds=ART_SEEDS[i:i + 1], **kw)[1]
        report_mismatch(alone.cpu(), whole[i:i + 1].cpu(), f'generate_long_artv: video {i} at b = 1 against b = 2')
    # the first clip is the clip of a plain call with the same seed (level 0, window 0 is substream 0); the later clips draw elsewhere
    plain = m.sample_tokens(text[:2], visual=vis[:2], seeds=ART_SEEDS[:2])[1]
    report_mismatch(whole[:, :T].reshape(2, -1).cpu(), plain.cpu(), 'the first clip against sample_tokens')


# ------------------------------------------------------------------------------------------------------------ 6. compatibility
def test_unseeded_calls_are_untouched_and_seeded_calls_leave_the_generators_alone(bert, mp, bert_inputs, artv):
    _, control, _ = bert_inputs
    m, text, vis, _ = artv

    def unseeded():
        torch.manual_seed(6)
        return (bert.mask_predict(control, dynamic=False, steps=4, mp_config=mp)[0],
                m.sample_tokens(text[:3], visual=vis[:3])[1], m.sample_tokens(text[:1], visual=vis[:1])[1])

    before = unseeded()
    dev_state, cpu_state = torch.cuda.get_rng_state(), torch.get_rng_state()
    bert_run(bert, mp, bert_inputs, [0, 1, 2], [A, Bs, C], 'plain')
    art_run(artv, [0, 1, 2])
    art_run(artv, [0])
    art_run(artv, [0, 1, 2], _trace=[])
    assert torch.equal(torch.cuda.get_rng_state(), dev_state) and torch.equal(torch.get_rng_state(), cpu_state)
    after = unseeded()
    for a, b, what in zip(before, after, ('BERT mask-predict', 'ART-V at batch 3', 'ART-V at batch 1')):
        report_mismatch(b.cpu(), a.cpu(), f'{what}: seeds=None after seeded calls against the same call before them')
