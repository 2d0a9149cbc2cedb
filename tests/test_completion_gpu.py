"""Video completion on the device (mmvid_amd/completion.py, the `given` path of mmvid_amd/sampling.py, csrc/sample.hip, csrc/frames.hip).
Every comparison is an equality: the generalised selection kernel against oracle.sampling.keep_race through guarded buffers, the
given path against the two pinned shared patterns (`preserve` with long_mode 'long' and 'interp') on the same variates, rows of one
batch against single-row calls, what happens at given positions, the paste kernel bit for bit, and `complete` end to end."""
import numpy as np
import pytest
import torch

from guarded import Guarded, call_abi, report_mismatch
from test_long_video_gpu import Recorder, _planted, build_model, rows_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T, N_TOK, FMAP, SIZE = 4, 16, 4, 64  # num_targets, tokens per 64 x 64 frame, token grid, pixels
TS = T * N_TOK


# --------------------------------------------------------------------------------------------------- 1. the selection kernel
def _select_rows(Y, E, given, k):
    """mmvid_mp_select_keep_rows on guarded and poisoned buffers -> mask1 [b, Bm, TS] uint8 (host)."""
    b, Bm, n = E.shape
    gY, gE = Guarded(Y, role='in'), Guarded(E.view(b * Bm, n), role='in')
    gG, gK = Guarded(given, role='in'), Guarded(k, role='in')
    gM = Guarded(role='out', shape=(b * Bm, n), dtype=torch.uint8)
    call_abi('mmvid_mp_select_keep_rows', gY.ptr, gE.ptr, gG.ptr, gK.ptr, b, Bm, n, gM.ptr)
    for g, what in ((gY, 'Y'), (gE, 'E'), (gG, 'given'), (gK, 'k_rows')):
        g.check(f'mp_select_keep_rows {what}')
    return gM.check('mp_select_keep_rows mask1').view(b, Bm, n)


def _oracle_rows(Y, E, given, k):
    from oracle import sampling as S
    b, Bm, n = E.shape
    want = np.zeros((b, Bm, n), bool)
    for i in range(b):
        for j in range(Bm):
            want[i, j] = S.keep_race(Y[i], E[i, j], given[i].bool(), int(k[i]))
    return torch.from_numpy(want).to(torch.uint8)


@pytest.mark.parametrize('n', [32, 257, 512])
def test_select_keep_rows_matches_the_oracle(n):
    """b = 3 rows per launch, so the cases of the issue go through three launches per size, each with three different masks and three
    different keep counts: (k = 0, 1, a middle value), (#valid, #valid + 1, above the non-zero weights), (an all-given row, a
    none-given row, a row with ties across its k boundary).  n = 257: the tail of the 256-thread loop."""
    b, Bm = 3, 2
    gen = torch.Generator().manual_seed(100 + n)
    Y = torch.rand(b, n, generator=gen) * 0.9 + 0.05
    E = torch.empty(b, Bm, n).exponential_(generator=gen)
    given = (torch.rand(b, n, generator=gen) < 0.25).to(torch.uint8)
    given[:, :2] = torch.tensor([1, 0], dtype=torch.uint8)  # both kinds in every row
    nv = (given == 0).sum(1)
    # launch A
    k = torch.tensor([0, 1, int(nv[2]) // 2], dtype=torch.int32)
    got, want = _select_rows(Y, E, given, k), _oracle_rows(Y, E, given, k)
    report_mismatch(got, want, f'rows, TS = {n}, k = {k.tolist()}')
    assert [int(v) for v in got[:, 0].sum(1) - given.sum(1)] == [1, 1, int(nv[2]) // 2]  # (k = 0 falls back to one position)
    # launch B: zeros planted in the weights of row 2 at valid positions, k above what is left
    Yz = Y.clone()
    valid2 = (given[2] == 0).nonzero().view(-1)
    Yz[2, valid2[::3]] = 0.0
    nnz2 = int(((given[2] == 0) & (Yz[2] > 0)).sum())
    assert nnz2 + 1 <= int(nv[2])
    k = torch.tensor([int(nv[0]), int(nv[1]) + 1, nnz2 + 1], dtype=torch.int32)
    got, want = _select_rows(Yz, E, given, k), _oracle_rows(Yz, E, given, k)
    report_mismatch(got, want, f'rows, TS = {n}, k = {k.tolist()}')
    assert int(got[0].min()) == 1  # k = #valid keeps everything
    assert [int(v) for v in got[1:, 1].sum(1) - given[1:].sum(1)] == [1, 1]  # both fall back to one position
    # launch C: all given, none given, ties
    g3 = given.clone()
    g3[0], g3[1] = 1, 0
    ties = torch.tensor([3, n // 4, n // 4 + 1, n // 2 + 3, n - 1])
    g3[2, ties] = 0
    Yt, Et = Y.clone(), E.clone()
    Et[2, 1] = Et[2, 0]  # (k is per video: both candidates of the tie row race on the same variates, so one k straddles both)
    Yt[2, ties], Et[2, :, ties] = 0.5, 0.375  # equal E and equal Y: the fp32 quotients are the same number
    keys = torch.where(g3[2] == 0, Et[2, 0] / Yt[2], torch.tensor(float('inf')))
    below = int((keys < 0.75).sum())
    assert int((keys == 0.75).sum()) == len(ties)
    k = torch.tensor([-1, n // 3, below + 2], dtype=torch.int32)  # two of the five tied positions are kept: the lower indices
    got, want = _select_rows(Yt, Et, g3, k), _oracle_rows(Yt, Et, g3, k)
    report_mismatch(got, want, f'rows, TS = {n}, k = {k.tolist()}')
    assert int(got[0].min()) == 1 and [int(v) for v in got[1].sum(1)] == [n // 3, n // 3]
    assert got[2, 0, ties].tolist() == [1, 1, 0, 0, 0] and got[2, 1, ties].tolist() == [1, 1, 0, 0, 0]


@pytest.mark.parametrize('n', [32, 257, 512])
def test_shared_entry_equals_rows_entry_on_a_repeated_mask(n):
    """mmvid_mp_select_keep (one [TS] mask, k by value) against mmvid_mp_select_keep_rows on that mask and that k repeated."""
    from mmvid_amd import ops
    b, Bm = 3, 2
    gen = torch.Generator().manual_seed(200 + n)
    Y = torch.rand(b, n, generator=gen)
    Y[0, 5:5 + n // 8] = 0.0
    E = torch.empty(b, Bm, n).exponential_(generator=gen)
    shared = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
    nv = int((shared == 0).sum())
    Yd, Ed, sd = Y.to(DEV), E.to(DEV), shared.to(DEV)
    for k in (0, 1, nv // 2, nv, nv + 1):
        old = ops.mp_select_keep(Yd, Ed, sd, k).cpu()
        rows = _select_rows(Y, E, shared.repeat(b, 1), torch.full((b, ), k, dtype=torch.int32))
        report_mismatch(rows, old, f'shared against rows, TS = {n}, k = {k}')
        via_ops = ops.mp_select_keep(Yd, Ed, sd.repeat(b, 1).contiguous(), torch.full((b, ), k, dtype=torch.int32, device=DEV)).cpu()
        report_mismatch(via_ops, old, f'ops.mp_select_keep per-video form, TS = {n}, k = {k}')
    none = ops.mp_select_keep(Yd, Ed, None, n // 2).cpu()  # no mask at all against an all-zero mask per row
    rows = _select_rows(Y, E, torch.zeros(b, n, dtype=torch.uint8), torch.full((b, ), n // 2, dtype=torch.int32))
    report_mismatch(rows, none, f'no mask against zero masks, TS = {n}')


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope='module')
def model():
    return build_model()


@pytest.fixture(scope='module')
def mp(golden):
    return dict(golden('mask_predict').meta['mp_config'], B=2)


@pytest.fixture(scope='module')
def setup(model):
    """Text, control rows, and a video's worth of valid tokens per row (three rows)."""
    gen = torch.Generator().manual_seed(31)
    text = torch.randint(1, 49408, (3, 16), generator=gen)
    text[0, 9:] = 0
    text = text.to(DEV)
    tokens = torch.randint(0, model.num_image_tokens, (3, TS), generator=gen).to(DEV)
    with torch.no_grad():
        control = model(text, return_loss=False)
    return text, control, tokens


def replay(drawn, rows=None, row=None):
    """A `_race` that hands back recorded variates: all of them, or row `row` of the `rows` rows they were drawn for."""
    def race(name, shape):
        got = drawn[name] if rows is None else rows_of(drawn, name, rows, row, row + 1)
        assert tuple(got.shape) == tuple(shape), (name, tuple(got.shape), tuple(shape))
        return got
    return race


STEP_KEYS = ('mask1', 'Y', 'I_tok', 'S', 'jmax', 'Imax', 'active')


def same_trace(a, b, what):
    """Every record of every step.  S and jmax of a video that had stopped before the step are not part of it: the update kernel leaves
    a stopped video alone, so those two entries of the step's fresh buffers were never stored (which videos had stopped is compared)."""
    assert len(a) == len(b), (what, len(a), len(b))
    for ra, rb in zip(a, b):
        assert ra['t'] == rb['t']
        if ra['t'] == 0:
            for key in ('Y', 'I_tok'):
                report_mismatch(ra[key].cpu(), rb[key].cpu(), f'{what}, step 0, {key}')
            continue
        assert torch.equal(ra['active_before'], rb['active_before'])
        ran = ra['active_before'].bool().cpu()
        for key in STEP_KEYS:
            ga, gb = ra[key].cpu(), rb[key].cpu()
            if key in ('S', 'jmax'):
                ga, gb = ga[ran], gb[ran]
            report_mismatch(ga, gb, f'{what}, step {ra["t"]}, {key}')


# -------------------------------------------------------------------------------------------- 2. anchor to the pinned path
@pytest.mark.parametrize('dynamic,steps', [(False, 5), (True, 9)])
@pytest.mark.parametrize('pattern', ['long1', 'long3', 'interp'])
def test_given_equals_the_pinned_shared_patterns(model, mp, setup, pattern, dynamic, steps):
    """`given` = the first o frames of every row (o = 1, 3) is `preserve` with long_mode 'long' and t_overlap = o; `given` = the even
    frame slots is long_mode 'interp'.  Same variates: the tokens and every trace record of every step are bit-equal."""
    _, control, tokens = setup
    b = 2
    control, prev = control[:b], tokens[:b]
    frame_of = torch.arange(TS, device=DEV) // N_TOK
    gtok = torch.zeros(b, TS, dtype=torch.int64, device=DEV)
    if pattern == 'interp':
        preserve = torch.full((b, TS), model.image_token_lut['[MASK]'], dtype=torch.long, device=DEV)
        preserve[:, :TS // 2] = prev[:, :TS // 2]  # the given half first, the reference's calling convention
        kw = dict(preserve=preserve, long_mode='interp', t_overlap=1)
        mask = (frame_of % 2 == 0).to(torch.uint8).repeat(b, 1)
        gtok.view(b, T, N_TOK)[:, ::2] = prev[:, :TS // 2].view(b, T // 2, N_TOK)
    else:
        o = int(pattern[4:])
        kw = dict(preserve=prev.reshape(b * T, N_TOK), long_mode='long', t_overlap=o)  # code_: (b t) n; its last o frames are kept
        mask = (frame_of < o).to(torch.uint8).repeat(b, 1)
        gtok[:, :N_TOK * o] = prev[:, TS - N_TOK * o:]
    rec, want_trace, got_trace = Recorder(), [], []
    want = model.mask_predict(control, dynamic=dynamic, steps=steps, mp_config=mp, _race=rec, _trace=want_trace, **kw)[0]
    got = model.mask_predict(control, dynamic=dynamic, steps=steps, mp_config=mp, given=(mask, gtok), _race=replay(rec.drawn),
                             _trace=got_trace)[0]
    report_mismatch(got.cpu(), want.cpu(), f'{pattern} dynamic={dynamic}: tokens')
    same_trace(got_trace, want_trace, f'{pattern} dynamic={dynamic}')
    # a mask on the host (the row counts then cost no device read) gives the same run
    again = model.mask_predict(control, dynamic=dynamic, steps=steps, mp_config=mp, given=(mask.cpu().bool(), gtok),
                               _race=replay(rec.drawn))[0]
    assert torch.equal(again, want)


# ----------------------------------------------------------------------------------------------------- 3. row independence
def three_masks():
    """First frame; the same 2 x 2 token box in every frame; a seeded Bernoulli half."""
    m = torch.zeros(3, T, FMAP, FMAP, dtype=torch.uint8)
    m[0, 0] = 1
    m[1, :, 1:3, 2:4] = 1
    m[2] = (torch.rand(T, FMAP, FMAP, generator=torch.Generator().manual_seed(32)) < 0.5).to(torch.uint8)
    return m.view(3, TS).to(DEV)


@pytest.fixture(scope='module')
def batch_of_three(model, mp, setup):
    """One b = 3 run per `dynamic` with recorded variates and its trace, shared by the tests below (and left unchanged by them)."""
    _, control, tokens = setup
    mask = three_masks()
    out = {}
    for dynamic, steps in ((False, 5), (True, 9)):
        rec, trace = Recorder(), []
        seq = model.mask_predict(control, dynamic=dynamic, steps=steps, mp_config=mp, given=(mask, tokens), _race=rec, _trace=trace)[0]
        out[dynamic] = dict(seq=seq, drawn=rec.drawn, trace=trace, steps=steps, mask=mask)
    return out


@pytest.mark.parametrize('dynamic', [False, True])
def test_rows_do_not_depend_on_their_batch_mates(model, mp, setup, batch_of_three, dynamic):
    _, control, tokens = setup
    run = batch_of_three[dynamic]
    for i in range(3):
        one = model.mask_predict(control[i:i + 1], dynamic=dynamic, steps=run['steps'], mp_config=mp,
                                 given=(run['mask'][i:i + 1], tokens[i:i + 1]), _race=replay(run['drawn'], 3, i))[0]
        report_mismatch(one.cpu(), run['seq'][i:i + 1].cpu(), f'row {i} alone against row {i} of the batch, dynamic={dynamic}')


# -------------------------------------------------------------------------------------------------------- 4. given positions
@pytest.mark.parametrize('dynamic', [False, True])
def test_given_positions_hold_their_tokens_at_every_step(setup, batch_of_three, dynamic):
    _, _, tokens = setup
    run = batch_of_three[dynamic]
    known = run['mask'].bool()
    assert len(run['trace']) >= 2
    for rec in run['trace']:
        assert torch.equal(rec['I_tok'][known], tokens[known]), f'step {rec["t"]}: a given token changed'
        if rec['t'] > 0:
            Bm = rec['mask1'].shape[1]
            assert bool((rec['mask1'][known.unsqueeze(1).expand(-1, Bm, -1)] == 1).all()), f'step {rec["t"]}: a given position was masked'
            assert torch.equal(rec['Imax'][known], tokens[known])
            assert rec['k'].dtype == torch.int32 and tuple(rec['k'].shape) == (3, )
    assert torch.equal(run['seq'][known], tokens[known])
    assert 0 <= int(run['seq'].min()) and int(run['seq'].max()) < 256


@pytest.mark.parametrize('dynamic,steps', [(False, 5), (True, 9)])
def test_all_given_and_none_given_rows(model, mp, setup, dynamic, steps):
    """In one batch: a row with everything given comes back unchanged, a row with nothing given is the plain sampler's row."""
    _, control, tokens = setup
    mask = three_masks()
    mask[0], mask[1] = 1, 0
    rec = Recorder()
    seq = model.mask_predict(control, dynamic=dynamic, steps=steps, mp_config=mp, given=(mask, tokens), _race=rec)[0]
    assert torch.equal(seq[0], tokens[0])
    plain = model.mask_predict(control[1:2], dynamic=dynamic, steps=steps, mp_config=mp, _race=replay(rec.drawn, 3, 1))[0]
    report_mismatch(seq[1:2].cpu(), plain.cpu(), f'none-given row against the plain sampler, dynamic={dynamic}')
    known = mask[2].bool()
    assert torch.equal(seq[2][known], tokens[2][known])


# ------------------------------------------------------------------------------------------------------- 5. the paste kernel
def _to_pixels(given, H, W):
    h, w = given.shape[1:]
    return given.bool().repeat_interleave(H // h, 1).repeat_interleave(W // w, 2)


@pytest.mark.parametrize('N,H,W,h,w', [(3, 16, 16, 4, 4), (2, 64, 64, 4, 4), (1, 16, 48, 2, 6)])
def test_frames_paste_u8_bit_for_bit(N, H, W, h, w):
    from mmvid_amd import ops
    gen = torch.Generator().manual_seed(1000 * N + H + W + h)
    x = _planted((N, 3, H, W), gen)
    real = torch.randint(0, 256, (N, H, W, 3), generator=gen, dtype=torch.uint8)
    given = (torch.rand(N, h, w, generator=gen) < 0.5).to(torch.uint8)
    given.view(-1)[:2] = torch.tensor([1, 0], dtype=torch.uint8)
    given = given * 3  # any non-zero value means given
    px = _to_pixels(given, H, W).unsqueeze(-1).expand(N, H, W, 3)

    def paste(img, real, start):
        gin, greal, ggiven = Guarded(img.view(N * 3, H * W), role='in'), Guarded(real.view(N * H, W * 3), role='in'), \
            Guarded(given.view(N * h, w), role='in')
        gout = Guarded(base=start.view(N * H, W * 3))
        call_abi('mmvid_frames_paste_u8', gin.ptr, greal.ptr, ggiven.ptr, N, H, W, h, w, gout.ptr)
        for g, what in ((gin, 'img'), (greal, 'real'), (ggiven, 'given')):
            g.check(f'frames_paste_u8 {what}')
        return gout.check('frames_paste_u8 out').view(N, H, W, 3)

    q = ops.frames_to_u8(x.to(DEV)).cpu()
    assert torch.equal(q, (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1))
    want = torch.where(px, real, q)
    # (the window starts as the complement of what is expected: an element that was never stored differs from it)
    report_mismatch(paste(x, real, want ^ 0xFF), want, f'frames_paste_u8 {N}x{H}x{W} grid {h}x{w}')
    assert torch.equal(ops.frames_paste_u8(x.to(DEV), real.to(DEV), given.to(DEV)).cpu(), want)
    # NaN under a given token leaves real, NaN elsewhere gives 0, and the neighbours of a NaN are untouched by it
    y = x.clone()
    nan_at = torch.randperm(y.numel(), generator=gen)[:97]
    y.view(-1)[nan_at] = float('nan')
    isnan = torch.isnan(y).permute(0, 2, 3, 1)
    assert bool((isnan & px).any()) and bool((isnan & ~px).any())
    real1 = real.clamp(min=1)  # (no zero byte in real: a NaN that was quantised under a given token would show)
    got = paste(y, real1, torch.full((N, H, W, 3), 7, dtype=torch.uint8))
    assert torch.equal(got[isnan & px], real1[isnan & px])
    assert int(got[isnan & ~px].max()) == 0
    assert torch.equal(got[~isnan], torch.where(px, real1, q)[~isnan])


@pytest.mark.parametrize('H,W,h,w,rule', [(16, 16, 4, 8, b'(W / w) % 4'), (16, 16, 3, 4, b'H % h'), (16, 18, 4, 4, b'W % w')])
def test_frames_paste_u8_refuses_what_it_cannot_tile(H, W, h, w, rule):
    from mmvid_amd import _lib, ops
    N = 2
    gen = torch.Generator().manual_seed(H + W + h + w)
    gin = Guarded(torch.rand(N * 3, H * W, generator=gen), role='in')
    greal = Guarded(torch.randint(0, 256, (N * H, W * 3), generator=gen, dtype=torch.uint8), role='in')
    ggiven = Guarded(torch.ones(N * h, w, dtype=torch.uint8), role='in')
    gout = Guarded(role='out', shape=(N * H, W * 3), dtype=torch.uint8, partial=True)
    rc = _lib.load().mmvid_frames_paste_u8(gin.ptr, greal.ptr, ggiven.ptr, N, H, W, h, w, gout.ptr, ops._stream())
    torch.cuda.synchronize()
    assert rc == 1 and rule in _lib.load().mmvid_last_error(), _lib.load().mmvid_last_error()  # MMVID_ERR_ARG
    for g in (gin, greal, ggiven):
        g.check('refused call')
    assert int((gout.check('refused call, out') != 0xA5).sum()) == 0  # nothing was launched: the window still holds the sentinel


# --------------------------------------------------------------------------------------------------------- 6. end to end
def test_complete_end_to_end(model, mp, setup):
    from mmvid_amd import completion, ops
    text, _, _ = setup
    text = text[:2]
    gen = torch.Generator().manual_seed(33)
    frames = torch.randint(0, 256, (2, T, SIZE, SIZE, 3), generator=gen, dtype=torch.uint8).to(DEV)
    given = torch.zeros(2, T, FMAP, FMAP, dtype=torch.uint8)
    given[0, 0] = 1  # video 0: its first frame
    given[1, :, 0:2, 1:4] = 1  # video 1: a region of every frame
    rec = Recorder()
    out, tok = completion.complete(model, text, frames, given, mask_predict_steps=4, mp_config=mp, _race=rec)
    assert out.shape == (2, T, SIZE, SIZE, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert tok.shape == (2, T, N_TOK) and tok.dtype == torch.int64 and int(tok.min()) >= 0 and int(tok.max()) < model.num_image_tokens
    px = _to_pixels(given.view(2 * T, FMAP, FMAP), SIZE, SIZE).view(2, T, SIZE, SIZE).to(DEV)
    assert torch.equal(out[px], frames[px]), 'a known pixel is not the input byte'
    plain = ops.frames_to_u8(model.vae.decode(tok.view(2 * T, N_TOK))).view(2, T, SIZE, SIZE, 3)
    assert torch.equal(out[~px], plain[~px])
    assert not torch.equal(out[px], plain[px])  # (the reconstruction of random bytes is not those bytes: the paste did something)
    with torch.no_grad():
        real_tok = model.get_image_tokens(ops.frames_u8_to_f32(frames.view(2 * T, SIZE, SIZE, 3)).view(2, T, 3, SIZE, SIZE))
    known = given.view(2, TS).bool().to(DEV)
    assert torch.equal(tok.view(2, TS)[known], real_tok[known])
    # no decode: None and the same tokens
    none, tok2 = completion.complete(model, text, frames, given, mask_predict_steps=4, mp_config=mp, decode=False, _race=replay(rec.drawn))
    assert none is None and torch.equal(tok2, tok)
    # token input: the same tokens; nothing to paste, the plain bytes
    out3, tok3 = completion.complete(model, text, real_tok, given, mask_predict_steps=4, mp_config=mp, _race=replay(rec.drawn))
    assert torch.equal(tok3, tok) and torch.equal(out3, plain)
    # fp32 frames and a pixel mask of the same content: the same tokens again
    f32 = ops.frames_u8_to_f32(frames.view(2 * T, SIZE, SIZE, 3)).view(2, T, 3, SIZE, SIZE)
    _, tok4 = completion.complete(model, text, f32, px, mask_predict_steps=4, mp_config=mp, decode=False, _race=replay(rec.drawn))
    assert torch.equal(tok4, tok)
    assert not model.training
