"""The device draws of csrc/frontend.hip through the C ABI on guarded buffers (tests/guarded.py), against the host replica of its
Philox stream (tests/frontend_ref.py): every decision is demanded sample by sample -- strategy, Bernoulli field token by token, box,
preserved frames, warp parameters, erase choices and boxes, colour jitter, condition drop -- and so are the key and step handling
of the device state.

Three places are not reproducible bit for bit (contraction of the Bernoulli threshold, the rounding of the box sides after logf /
expf / sqrtf, the affine matrix after cosf / sinf); the replica flags the samples and tokens they could move, the tests leave those
out, print how many there were and FAIL when a case flags more than frontend_ref.SAMPLE_CAP (0.1 % of its samples) or
frontend_ref.TOKEN_CAP (10 per million tokens of a Bernoulli field).  tests/test_frontend_ref_host.py proves on the CPU that the seeds
used here keep the replica inside those caps.

Flagged counts observed on the MI355X (each test prints its own; the flags come from the replica, so they are the same on any
machine): the largest is 0 -- no sample of any mmvid_msm_masks or mmvid_random_erase_tokens case and no Bernoulli token was flagged,
and every device decision equalled the replica's.  The affine matrix was within 1.4e-7 of its fp64 value (bound 2.1e-6).

Sentinels and poison are ordinary data; every launch is a few thousand threads."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import frontend_ref as R
from guarded import Guarded
from guarded import call_abi as _call

pytestmark = pytest.mark.gpu
DEV = 'cuda'
I32, I64, F32, U8 = torch.int32, torch.int64, torch.float32, torch.uint8


def _farr(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def _iarr(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _state(step, seed):
    """A front-end state on the device, as an input operand: word 0 the fp32 counter, words 1 and 2 the seed's BITS (written as
    integers: a float copy could quieten a NaN pattern)."""
    w = np.array(R.state_words(step, seed), np.uint32).view(np.int32)
    return Guarded(torch.from_numpy(w.copy()), role='in')


def _placements(seed, other):
    """(name, seed argument, state seed) -> the key is their XOR in every case."""
    return (('state', 0, seed), ('argument', seed, 0), ('both', other, seed))


def _eq(got, want, what, keep=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if keep is not None:
        bad &= keep
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f'{what}: {len(idx)} of {bad.size} differ from the replica; first (index, device, replica): '
                             f'{[(tuple(i), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:5]]}')


def _cap(flagged, total, cap, what):
    print(f'{what}: {int(flagged)} of {int(total)} flagged as ambiguous by the replica (cap {cap * total:.2f})')
    assert flagged <= cap * total, f'{what}: {int(flagged)} of {int(total)} flagged: more than the cap {cap:g} allows'


# ---- state and key ----------------------------------------------------------------------------------------------------------------------
def _draw_cond(seed_arg, state, B, p_text=0.5, p_visual=0.5):
    text = Guarded(torch.arange(B * 3, dtype=I64).view(B, 3) + 1, role='in')
    t_out, dec = Guarded(role='out', shape=(B, 3), dtype=I64), Guarded(role='out', shape=(B, 2), dtype=U8)
    _call('mmvid_cond_drop', text.ptr, None, B, 3, 0, None if state is None else state.ptr, seed_arg, float(p_text), float(p_visual), None,
          77, t_out.ptr, None, dec.ptr)
    text.check('cond_drop text')
    if state is not None:
        state.check('cond_drop state')
    return t_out.check('cond_drop text_out').numpy(), dec.check('cond_drop decided').numpy(), text.window().numpy()


def _draw_warp(seed_arg, state, B, T, prob):
    scratch = Guarded(role='out', shape=(B, R.WARP_PARAMS_BYTES), dtype=U8, partial=True)  # (a parameter byte may equal the sentinel)
    _call('mmvid_vid_warp_draw', seed_arg, None if state is None else state.ptr, B, T, _farr(prob), scratch.ptr)
    if state is not None:
        state.check('vid_warp_draw state')
    return scratch.check('vid_warp_draw params_scratch').numpy().reshape(-1)


def _check_warp(raw, want, B, T, what):
    got = R.read_warp_params(raw, B)
    for k in ('mode', 'j1', 'src_b', 'src_t', 'chan'):
        _eq(got[k], want[k], f'{what}: {k}')
    _eq(got['perm'][:, :T], want['perm'][:, :T], f'{what}: perm[:T]')
    _eq(got['shift'].view(np.uint32), want['shift'].view(np.uint32), f'{what}: shift (bits)')
    err = np.abs(got['th'].astype(np.float64) - want['th'])
    print(f'{what}: worst |th - fp64| = {err.max():.3e} (bound {R.TH_TOL:.3e})')
    assert err.max() <= R.TH_TOL, f'{what}: th differs from the fp64 value by {err.max():.3e} > 2^-19 * 1.1 at {np.argwhere(err > R.TH_TOL)[:4].tolist()}'


@pytest.mark.parametrize('place', ('state', 'argument', 'both'))
def test_key_and_step_handling(place):
    """Every seed x every step, with the seed in the state words, as the by-value argument, and split over both: the condition drop
    (two streams) and the warp draw (two more) follow key = argument XOR state words and step = (uint32) state[0]."""
    B, T = 64, 4
    for n, (seed, step) in enumerate(itertools.product(R.STATE_SEEDS, R.STATE_STEPS)):
        other = R.STATE_SEEDS[(n + 1) % len(R.STATE_SEEDS)] ^ 0x9E3779B97F4A7C15
        arg, st_seed = dict((name, (a, s)) for name, a, s in _placements(seed, other))[place]
        key = R.key64(arg, *R.state_words(step, st_seed)[1:3])
        assert key == (arg ^ st_seed)
        what = f'seed {seed:#x} step {step} ({place})'
        _, dec, _ = _draw_cond(arg, _state(step, st_seed), B)
        _eq(dec, R.cond_drop(key, step, B, 0.5, 0.5), f'{what}: cond_drop decided')
        raw = _draw_warp(arg, _state(step, st_seed), B, T, [0.25] * 4)
        _check_warp(raw, R.warp_params(key, step, B, T, [0.25] * 4), B, T, f'{what}: vid_warp_draw')


def test_null_state_is_step_zero_and_key_is_the_argument():
    B, T = 64, 4
    for seed in R.STATE_SEEDS:
        _, dec, _ = _draw_cond(seed, None, B)
        _eq(dec, R.cond_drop(seed, 0, B, 0.5, 0.5), f'seed {seed:#x}, step_dev = NULL: cond_drop decided')
        _check_warp(_draw_warp(seed, None, B, T, [0.25] * 4), R.warp_params(seed, 0, B, T, [0.25] * 4), B, T,
                    f'seed {seed:#x}, step_dev = NULL: vid_warp_draw')


def test_seeds_that_differ_only_in_the_high_word_draw_differently():
    """Ranks whose seeds differ only above bit 31 must not share masks (the replica agrees: compared in the tests above; here the
    property itself, on the device alone)."""
    a = _draw_cond(0, _state(3, 0x0000000100000001), 256)[1]
    b = _draw_cond(0, _state(3, 0x0000000200000001), 256)[1]
    assert (a != b).mean() > 0.3


# ---- mmvid_msm_masks --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _msm_ref(shape, prob, pc):
    B, T, f = shape
    return R.msm_mask(R.MSM_SEED, R.MSM_STEP, B, T, f, prob, R.MSM_BERN[0], R.MSM_BERN[1], pc)


@pytest.mark.parametrize('pc', R.MSM_PC)
@pytest.mark.parametrize('prob', R.MSM_PROBS, ids=('p7111', 'p2525'))
@pytest.mark.parametrize('shape', R.MSM_SHAPES, ids=lambda s: 'B%dT%df%d' % s)
def test_msm_masks_equal_the_replica(shape, prob, pc):
    B, T, f = shape
    TS = T * f * f
    mask_w, nfm_w, dec, tok_amb, smp_amb = _msm_ref(shape, prob, pc)
    state = _state(R.MSM_STEP, R.MSM_SEED)
    mask, nfm, strat = (Guarded(role='out', shape=(B, TS), dtype=U8), Guarded(role='out', shape=(B,), dtype=F32),
                        Guarded(role='out', shape=(B,), dtype=I32))
    _call('mmvid_msm_masks', 0, state.ptr, B, T, f, _farr(prob), R.MSM_BERN[0], R.MSM_BERN[1], float(pc), mask.ptr, nfm.ptr, strat.ptr)
    state.check('msm_masks state')
    what = f'msm_masks {shape} {prob} pc {pc}'
    _eq(strat.check(what + ' strategy_out').numpy(), dec['strategy'].astype(np.int32), what + ': strategy_out')
    _eq(nfm.check(what + ' not_fully_masked').numpy(), nfm_w, what + ': not_fully_masked')
    got = mask.check(what + ' mask1').numpy()
    field = int((dec['strategy'] == 1).sum()) * TS
    _cap(smp_amb.sum(), B, R.SAMPLE_CAP, what + ' samples (box)')
    _cap(tok_amb.sum(), max(field, 1), R.TOKEN_CAP, what + ' Bernoulli tokens')
    _eq(got, mask_w, what + ': mask1', keep=~tok_amb & ~smp_amb[:, None])
    assert set(np.unique(dec['strategy'])) == {1, 2, 3, 4} and dec['has_box'].any()  # the case reaches every branch
    if pc > 0:
        assert dec['keep_frame'].any()


# ---- mmvid_vid_warp_draw and the entry points that draw the same parameters --------------------------------------------------------------
@pytest.mark.parametrize('B,T', ((1024, 8), (1, 4), (65, 32), (65, 2), (65, 1)))
def test_vid_warp_draw_equals_the_replica(B, T):
    from mmvid_amd import _lib
    assert _lib.load().mmvid_warp_params_bytes() == R.WARP_PARAMS_BYTES == 176
    seed, prob = 0xA5A5F00D0000BEEF, [0.25] * 4
    for step in ((0, 9) if B > 1 else range(24)):  # B = 1: enough steps to meet mode 0, the branch with no other sample
        want = R.warp_params(seed, step, B, T, prob)
        _check_warp(_draw_warp(0, _state(step, seed), B, T, prob), want, B, T, f'vid_warp_draw B {B} T {T} step {step}')
        if B == 1:
            assert not (want['mode'] == 0).any() or want['src_b'][0] == 0
    if B == 1:
        modes = {int(R.warp_params(seed, s, 1, T, prob)['mode'][0]) for s in range(24)}
        assert 0 in modes, modes


def test_every_warp_entry_point_leaves_the_same_parameters():
    """mmvid_vid_warp, _new_frames and _new_frames_u8 with draw_params = 1 write the bytes mmvid_vid_warp_draw writes."""
    B, T, C, H, W = 70, 3, 3, 4, 4
    seed, step, prob = 0x1234567800000007, 11, [0.4, 0.3, 0.2, 0.1]
    want = _draw_warp(0, _state(step, seed), B, T, prob)
    _check_warp(want, R.warp_params(seed, step, B, T, prob), B, T, 'vid_warp_draw, unequal probabilities')
    g = torch.Generator().manual_seed(1)
    x8 = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=U8)
    x = (x8.permute(0, 1, 4, 2, 3).float() / 255).contiguous()
    for name in ('mmvid_vid_warp', 'mmvid_vid_warp_new_frames', 'mmvid_vid_warp_new_frames_u8'):
        state, scratch = _state(step, seed), Guarded(role='out', shape=(B, R.WARP_PARAMS_BYTES), dtype=U8, partial=True)  # (a parameter byte may equal the sentinel)
        if name == 'mmvid_vid_warp':
            xin, out = Guarded(x.view(B * T, C, H * W), role='in'), Guarded(role='out', shape=(B * T, C, H * W), dtype=F32)
            _call(name, 0, state.ptr, xin.ptr, B, T, C, H, W, _farr(prob), scratch.ptr, 1, out.ptr)
        elif name == 'mmvid_vid_warp_new_frames':
            xin, out = Guarded(x.view(B * T, C, H * W), role='in'), Guarded(role='out', shape=(B, C, H * W), dtype=F32)
            _call(name, 0, state.ptr, xin.ptr, B, T, C, H, W, _farr(prob), scratch.ptr, 1, out.ptr)
        else:
            xin, out = Guarded(x8.view(B * T, H * W, 3), role='in'), Guarded(role='out', shape=(B, 3, H * W), dtype=F32)
            _call(name, 0, state.ptr, xin.ptr, B, T, H, W, _farr(prob), scratch.ptr, 1, out.ptr)
        state.check(name + ' state'), xin.check(name + ' x'), out.check(name + ' out')
        _eq(scratch.check(name + ' params_scratch').numpy().reshape(-1), want, name + ': bytes of params_scratch')


# ---- mmvid_cond_drop --------------------------------------------------------------------------------------------------------------------
def test_cond_drop_equals_the_replica_and_its_streams_are_independent():
    B, seed, step = 512, 0x00C0FFEE00000000, 6
    text_dec = {}
    for pt, pv in itertools.product((0.0, 0.1, 0.5, 1.0), repeat=2):
        vis = Guarded(torch.arange(B * 5, dtype=I64).view(B, 5) + 100, role='in')
        text = Guarded(torch.arange(B * 3, dtype=I64).view(B, 3) + 1, role='in')
        t_out, v_out, dec = (Guarded(role='out', shape=(B, 3), dtype=I64), Guarded(role='out', shape=(B, 5), dtype=I64),
                             Guarded(role='out', shape=(B, 2), dtype=U8))
        state = _state(step, seed)
        _call('mmvid_cond_drop', text.ptr, vis.ptr, B, 3, 5, state.ptr, 0, pt, pv, None, 77, t_out.ptr, v_out.ptr, dec.ptr)
        for g in (vis, text, state):
            g.check('cond_drop input')
        want = R.cond_drop(seed, step, B, pt, pv)
        what = f'cond_drop p_text {pt} p_visual {pv}'
        got = dec.check(what).numpy()
        _eq(got, want, what + ': decided')
        _eq(t_out.check(what).numpy(), np.where(want[:, :1] != 0, 0, text.window().numpy()), what + ': text_out')
        _eq(v_out.check(what).numpy(), np.where(want[:, 1:] != 0, 77, vis.window().numpy()), what + ': vis_out')
        assert text_dec.setdefault(pt, got[:, 0].tolist()) == got[:, 0].tolist(), f'{what}: p_visual moved a text decision'
    assert sum(text_dec[0.0]) == 0 and sum(text_dec[1.0]) == B and 0 < sum(text_dec[0.5]) < B


# ---- mmvid_visual_color_jitter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first_frame', (0, 1))
def test_visual_color_jitter_equals_the_replica(first_frame):
    B, Tv, C, H, W = 5, 3, 3, 5, 7  # 1575 elements: six full blocks of 256 and a ragged one
    seed = 0x7E57000000C0104
    x = torch.rand(B, Tv, C, H, W, generator=torch.Generator().manual_seed(2))
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = 1.0
    xn = x.numpy()
    gates = []
    for p, step in itertools.product((0.0, 0.9, 1.0), range(6)):
        state = _state(step, seed)
        buf, prm = Guarded(base=x.view(B * Tv, C, H * W)), Guarded(role='out', shape=(B, 3), dtype=F32)
        _call('mmvid_visual_color_jitter', 0, state.ptr, buf.ptr, B, Tv, C, H, W, float(p), first_frame, prm.ptr)
        state.check('visual_color_jitter state')
        want = R.color_jitter_params(seed, step, B, p)
        what = f'visual_color_jitter p {p} step {step} first_frame {first_frame}'
        _eq(prm.check(what).numpy().view(np.uint32), want.view(np.uint32), what + ': params_out (bits)')
        m = np.zeros((B, Tv, C, 1, 1), np.float32)
        for b in range(B):
            ch = int(want[b, 2])
            m[b, first_frame:, (slice(None) if ch == 0 else ch - 1)] = want[b, 1] * want[b, 0]
        ref = np.where(want[0, 0] != 0, np.minimum(np.maximum(xn + m, np.float32(0)), np.float32(1)), xn)
        ref[:, :first_frame] = xn[:, :first_frame]
        _eq(buf.check(what).numpy().reshape(xn.shape), ref.astype(np.float32), what + ': pixels')
        gates.append((p, bool(want[0, 0])))
    assert {g for p, g in gates if p == 0.0} == {False} and {g for p, g in gates if p == 1.0} == {True}


# ---- mmvid_erase_tokens_choice ----------------------------------------------------------------------------------------------------------
ERASE_CHOICE_CASES = (('n1', [2.0]), ('n2', [0.5, 2.0]), ('n3', [0.5, 0.75, 2.0]), ('n4', [0.25, 0.5, 0.75, 2.0]),
                      ('n3_last_below_1', [0.3, 0.5, 0.6]), ('n4_last_below_1', [0.2, 0.4, 0.6, 0.7]))


@pytest.mark.parametrize('name,cum', ERASE_CHOICE_CASES, ids=[c[0] for c in ERASE_CHOICE_CASES])
def test_erase_tokens_choice_equals_the_replica(name, cum):
    """Alternative i erases rows 0..i of a 4 x 4 map (mode 2), so the number of erased tokens names the alternative drawn."""
    B, Tv, f, n, seed = 3, 2, 4, len(cum), 0xFACE0000000000FF
    tok = torch.arange(B * Tv * f * f, dtype=I64).view(B, Tv * f * f)
    boxes = [v for i in range(n) for v in (0, i + 1, 0, f)]
    want = R.erase_choice(seed, np.arange(64), cum)
    got = []
    for step in range(64):
        state, buf = _state(step, seed), Guarded(base=tok)
        _call('mmvid_erase_tokens_choice', 0, state.ptr, n, _farr(cum), _iarr([2] * n), _iarr(boxes), 0, B, Tv, f, -1, buf.ptr)
        state.check('erase_tokens_choice state')
        out = buf.check(f'erase_tokens_choice {name} step {step}').view(B, Tv, f, f)
        rows = (out == -1).all(3)
        assert bool(((out == -1) == rows[..., None]).all()) and bool((rows == rows[0, 0]).all()), 'not whole rows, the same everywhere'
        assert torch.equal(out[out != -1], tok.view(B, Tv, f, f)[out != -1])
        k = int(rows[0, 0].sum())
        assert bool(rows[0, 0, :k].all())
        got.append(k - 1)
    _eq(np.array(got), want, f'erase_tokens_choice {name}: alternative drawn at steps 0..63')
    assert set(want.tolist()) == set(range(n)), f'{name}: 64 steps did not reach every alternative'


# ---- mmvid_random_erase_tokens ----------------------------------------------------------------------------------------------------------
def _boxes_of(out, B, Tv, f, value):
    """The erased rectangle of every sample from the token map: (on, [i, j, h, w]); the same on every frame."""
    hid = (out.view(B, Tv, f, f) == value).numpy()
    assert (hid == hid[:, :1]).all(), 'the box differs between frames'
    hid = hid[:, 0]
    rows, cols = hid.any(2), hid.any(1)
    on = rows.any(1)
    box = np.stack([rows.argmax(1), cols.argmax(1), rows.sum(1), cols.sum(1)], 1) * on[:, None]
    assert (hid == (rows[:, :, None] & cols[:, None, :])).all(), 'not a rectangle'
    return on, box


@pytest.mark.parametrize('p', R.ERASE_P)
@pytest.mark.parametrize('scale', R.ERASE_SCALES, ids=('bert', 'artv'))
def test_random_erase_tokens_equals_the_replica(scale, p):
    B, Tv, f = R.ERASE_B, 2, R.ERASE_F
    tok = torch.arange(B * Tv * f * f, dtype=I64).view(B, Tv * f * f)
    state, buf = _state(R.ERASE_STEP, R.ERASE_SEED), Guarded(base=tok)
    _call('mmvid_random_erase_tokens', 0, state.ptr, B, Tv, f, float(p), scale[0], scale[1], 0.5, 2.0, 0, -1, buf.ptr)
    state.check('random_erase_tokens state')
    what = f'random_erase_tokens scale {scale} p {p}'
    out = buf.check(what)
    assert torch.equal(out[out != -1], tok[out != -1])
    on, box = _boxes_of(out, B, Tv, f, -1)
    on_w, box_w, amb = R.random_erase_box(R.ERASE_SEED, R.ERASE_STEP, B, f, p, scale, (0.5, 2.0))
    _cap(amb.sum(), B, R.SAMPLE_CAP, what)
    _eq(on, on_w, what + ': erased at all', keep=~amb)
    _eq(box, box_w, what + ': box (i, j, h, w)', keep=~amb[:, None])
    assert on_w.any() and (p == 1.0 or not on_w.all())


def test_random_erase_tokens_erase_half():
    """erase_half: rows f/2.. of every frame, no draw at all (f odd: the larger half)."""
    for f in (8, 5):
        B, Tv = 9, 3
        tok = torch.arange(B * Tv * f * f, dtype=I64).view(B, Tv * f * f)
        state, buf = _state(R.ERASE_STEP, R.ERASE_SEED), Guarded(base=tok)
        _call('mmvid_random_erase_tokens', 0, state.ptr, B, Tv, f, 0.0, 0.55, 0.85, 0.5, 2.0, 1, -1, buf.ptr)
        state.check('random_erase_tokens state')
        want = tok.view(B, Tv, f, f).clone()
        want[:, :, f // 2:] = -1
        assert torch.equal(buf.check(f'erase_half f {f}').view(B, Tv, f, f), want)
