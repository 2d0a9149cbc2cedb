"""tests/frontend_ref.py, the host replica of the front-end's Philox stream, checked on the CPU: Philox4x32-10 against published
known answers, the variate's grid, and -- because the GPU tests (tests/test_frontend_draws_gpu.py) demand the device's decisions
sample by sample from this replica -- the DISTRIBUTION question in full: N = 2^18 draws per statistic, fixed seeds, every frequency
within 5 standard deviations of its binomial / multinomial expectation (the bar is that formula, not a constant), the erasing box
against oracle/frontend.py::erasing_box on a numpy generator with a two-sample bar, and the separation of the streams.

The last test proves that the seeds of the GPU cases keep the replica's ambiguity flags inside the caps those tests enforce."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import frontend_ref as R

N = 2**18
KEY = 0x243F6A8885A308D3  # every statistic below: this key (digits of pi), steps and samples as stated
SIGMAS = 5.0


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


def assert_binomial(count, n, p, what):
    """|count / n - p| <= 5 sqrt(p (1 - p) / n)."""
    bar = SIGMAS * math.sqrt(p * (1 - p) / n)
    print(f'{what}: {count / n:.5f} expected {p:.5f} bar {bar:.5f} (n = {n})')
    assert abs(count / n - p) <= bar, f'{what}: frequency {count / n:.6f} is more than 5 sigma ({bar:.6f}) from {p:.6f} over {n} draws'


def assert_multinomial(values, probs, what):
    """Each category of integer `values` (0..len(probs)-1) within its own binomial bar; nothing outside the categories."""
    values = np.asarray(values)
    counts = np.bincount(values, minlength=len(probs))
    assert len(counts) == len(probs) and values.min() >= 0, f'{what}: a value outside 0..{len(probs) - 1}'
    for k, p in enumerate(probs):
        if p == 0:
            assert counts[k] == 0, f'{what}: category {k} has probability 0 and was drawn {counts[k]} times'
        else:
            assert_binomial(int(counts[k]), len(values), p, f'{what} [{k}]')


def assert_mean(x, mean, var, what):
    """|mean(x) - mean| <= 5 sqrt(var / n)."""
    bar = SIGMAS * math.sqrt(var / len(x))
    print(f'{what}: mean {np.mean(x):.5f} expected {mean:.5f} bar {bar:.5f}')
    assert abs(float(np.mean(x)) - mean) <= bar, what


def assert_two_sample(a, b, what):
    """|mean(a) - mean(b)| <= 5 sqrt(var(a) / n_a + var(b) / n_b): the standard error comes from both samples."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bar = SIGMAS * math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print(f'{what}: replica {a.mean():.5f} oracle {b.mean():.5f} bar {bar:.5f}')
    assert abs(a.mean() - b.mean()) <= bar, f'{what}: {a.mean():.6f} against {b.mean():.6f}, bar {bar:.6f}'


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
                 ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
                 ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), 'd16cfe09 94fdcceb 5001e420 24126ea1'))


def test_philox4x32_10_known_answers():
    """The vectors of the Random123 distribution (kat_vectors: philox4x32 10)."""
    for ctr, key, want in KNOWN_ANSWERS:
        assert _hex(R.philox4x32_10(*ctr, *key)) == want
    c = np.array([k[0] for k in KNOWN_ANSWERS], np.uint64).T  # ... and vectorised: three at once
    k = np.array([k[1] for k in KNOWN_ANSWERS], np.uint64).T
    out = np.stack(R.philox4x32_10(*c, *k), 1)
    assert [_hex(r) for r in out] == [k[2] for k in KNOWN_ANSWERS]


def test_u01_range_grid_and_word_selection():
    assert R.u01(0) == 0 and R.u01(0xFF) == 0 and R.u01(0x100) == np.float32(2.0**-24)
    assert R.u01(0xFFFFFFFF) == np.float32(1 - 2.0**-24) and R.u01(0xFFFFFFFF).dtype == np.float32
    u = R.uniform(KEY, 3, 5, R.P_WARP, np.arange(N))
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert (u.astype(np.float64) * 2.0**24 == np.floor(u.astype(np.float64) * 2.0**24)).all()  # the 24-bit grid
    assert_mean(u.astype(np.float64), 0.5, 1 / 12, 'mean of u01')
    # draw i = word i & 3 of block i >> 2, counter {block, purpose, sample, step}, key {low, high}
    for i in range(12):
        blk = R.philox4x32_10(i >> 2, R.P_WARP, 5, 3, KEY & 0xFFFFFFFF, KEY >> 32)
        assert u[i] == R.u01(blk[i & 3])
    assert R.key64(0x1111222233334444, 0x0F0F0F0F, 0xF0F0F0F0) == 0x1111222233334444 ^ 0xF0F0F0F00F0F0F0F
    assert R.state_words(7, 0x7FC000017F800001) == [0x40E00000, 0x7F800001, 0x7FC00001, 0]
    assert R.state_words(2**24 - 1, 0)[0] == 0x4B7FFFFF


def test_fma32_is_the_exactly_rounded_fused_value():
    rng = np.random.RandomState(0)
    a, c = rng.uniform(0, 1, 4000).astype(np.float32), rng.uniform(0, 1, 4000).astype(np.float32)
    b = (rng.randint(0, 2**24, 4000) * 2.0**-24).astype(np.float32)
    # crafted: the fp64 sum IS an fp32 tie and only its error term says which neighbour is nearer -- rounding the fp64 sum gives the
    # other one.  (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46 below the tie; (1 + 2^-12)(1 - 2^-12 + 2^-24) = 1 + 2^-36 above it
    a = np.concatenate([a, np.float32([1 + 2.0**-23, 1 + 2.0**-12])])
    b = np.concatenate([b, np.float32([2.0**-4 * (1 - 2.0**-23), 2.0**-4 * (1 - 2.0**-12 + 2.0**-24)])])
    c = np.concatenate([c, np.float32([2.0**20 + 2.0**-3, 2.0**20])])
    got = R.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))  # within one fp32 step of the answer: pick the nearer neighbour exactly, ties to even
        cands = sorted({float(lo), float(np.nextafter(lo, np.float32(-np.inf))), float(np.nextafter(lo, np.float32(np.inf)))})
        best = min(cands, key=lambda f: (abs(Fraction(f) - v), int(np.float32(f).view(np.uint32)) & 1))
        return np.float32(best)

    want = np.array([exact(*t) for t in zip(a, b, c)], np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    unfused = (a * b + c).astype(np.float32)
    assert got[-2] == np.float32(2.0**20 + 2.0**-3) and got[-1] == np.float32(2.0**20 + 2.0**-3)
    assert (unfused != got).any()  # the two compilations do differ: the reason the replica carries both


# ---- distributions of the replica -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def msm():
    """2^18 samples of one step with frame preservation always on; strategies by the production probabilities."""
    return R.msm_decisions(KEY, 11, N, 8, 8, (0.7, 0.1, 0.1, 0.1), 0.2, 0.5, 1.0)


def test_strategy_and_warp_mode_frequencies(msm):
    assert_multinomial(msm['strategy'] - 1, (0.7, 0.1, 0.1, 0.1), 'MSM strategy')
    d = R.msm_decisions(KEY, 12, N, 2, 2, (0.25, 0.25, 0.25, 0.25), 0.2, 0.5, 0.0)
    assert_multinomial(d['strategy'] - 1, (0.25,) * 4, 'MSM strategy, equal probabilities')
    w = R.warp_params(KEY, 13, N, 8, (0.4, 0.3, 0.2, 0.1))
    assert_multinomial(w['mode'], (0.4, 0.3, 0.2, 0.1), 'warp mode')
    w = R.warp_params(KEY, 14, N, 8, (0.0, 1.0, 0.0, 0.0))
    assert_multinomial(w['mode'], (0.0, 1.0, 0.0, 0.0), 'warp mode, one strategy only')


def test_warp_frame_sample_and_channel_choices_are_uniform():
    T, B = 8, 5
    w = R.warp_params(KEY, 15, N, T, (0.25,) * 4)
    assert_multinomial(w['j1'], (1 / T,) * T, 'j1')
    assert_multinomial(w['src_t'][w['mode'] == 0], (1 / T,) * T, 'src_t of mode 0')
    assert (w['src_t'][w['mode'] != 0] == w['j1'][w['mode'] != 0]).all()
    assert_multinomial(w['chan'][w['mode'] == 2], (0.25,) * 4, 'chan of mode 2')
    sh = w['shift'][w['mode'] == 2].astype(np.float64)
    assert sh.min() >= -0.5 and sh.max() < 0.5
    assert_mean(sh, 0.0, 1 / 12, 'shift of mode 2')
    assert (w['shift'][w['mode'] != 2] == 0).all() and (w['th'][w['mode'] != 3] == 0).all()
    th = w['th'][w['mode'] == 3]
    sc, ang = np.hypot(th[:, 0], th[:, 3]), np.arctan2(th[:, 3], th[:, 0])
    assert sc.min() >= 0.9 - 1e-6 and sc.max() <= 1.1 + 1e-6 and np.abs(ang).max() <= math.pi / 6 + 1e-6
    assert (th[:, 1] == -th[:, 3]).all() and (th[:, 0] == th[:, 4]).all() and np.abs(th[:, [2, 5]]).max() <= 0.1 + 1e-6
    assert_mean(sc, 1.0, 0.2**2 / 12, 'affine scale')
    assert_mean(ang, 0.0, (math.pi / 3)**2 / 12, 'affine angle')
    # the other sample: 2^18 draws of a batch of 5 (sample b of step n // 5), all in mode 0
    smp, stp = np.arange(N) % B, np.arange(N) // B
    w = R.warp_params(KEY, stp, B, T, (1.0, 0.0, 0.0, 0.0), samples=smp)
    assert (w['src_b'] != smp).all() and w['src_b'].min() >= 0 and w['src_b'].max() < B
    for b in range(B):
        others = [o for o in range(B) if o != b]
        assert_multinomial(np.searchsorted(others, w['src_b'][smp == b]), (1 / (B - 1),) * (B - 1), f'src_b of sample {b}')
    one = R.warp_params(KEY, np.arange(64), 1, T, (1.0, 0.0, 0.0, 0.0), samples=np.zeros(64, int))  # a batch of one: no other sample
    assert (one['src_b'] == 0).all() and len(set(one['src_t'].tolist())) > 1


@pytest.mark.parametrize('T', (3, 4))
def test_every_non_identity_permutation_equally_often(T):
    w = R.warp_params(KEY, 16 + T, N, T, (0.0, 1.0, 0.0, 0.0))
    assert (w['perm'][:, T:] == np.arange(T, 32)).all()
    perms = list(itertools.permutations(range(T)))
    code = (w['perm'][:, :T] * (T ** np.arange(T))).sum(1)
    index = {sum(v * T**i for i, v in enumerate(p)): k for k, p in enumerate(perms)}
    values = np.array([index[c] for c in code.tolist()])  # KeyError: not a permutation
    k = len(perms) - 1
    assert perms[0] == tuple(range(T))
    assert_multinomial(values, (0.0,) + (1 / k,) * k, f'permutation of {T} frames')


def test_preserved_frames_are_a_uniform_subset(msm):
    T = 8
    cnt, keep = msm['kept_count'], msm['keep_frame']
    assert (keep.sum(1) == cnt).all()
    assert_multinomial(cnt - 1, (1 / (T // 2),) * (T // 2), 'preserved-frame count')
    for c in range(1, T // 2 + 1):
        sel = keep[cnt == c]
        for t in range(T):
            assert_binomial(int(sel[:, t].sum()), len(sel), c / T, f'count {c}: frame {t} kept')
        if c >= 2:
            for t, q in itertools.combinations(range(T), 2):
                assert_binomial(int((sel[:, t] & sel[:, q]).sum()), len(sel), c * (c - 1) / (T * (T - 1)), f'count {c}: frames {t}, {q} kept')
    gate = R.msm_decisions(KEY, 21, N, 8, 2, (0.0, 1.0, 0.0, 0.0), 0.2, 0.5, 0.5)['kept_count'] > 0
    assert_binomial(int(gate.sum()), N, 0.5, 'frame-preservation gate at pc_prob 0.5')
    assert not R.msm_decisions(KEY, 21, 4096, 1, 2, (0.0, 1.0, 0.0, 0.0), 0.2, 0.5, 1.0)['keep_frame'].any()  # T = 1: nothing to keep


def test_bernoulli_field_keep_rate_given_its_threshold(msm):
    sp = msm['s_p_fused'][:4096].astype(np.float64)
    assert sp.min() >= 0.2 and sp.max() <= 0.5
    assert_mean(msm['s_p_fused'].astype(np.float64), 0.35, 0.3**2 / 12, 'Bernoulli probability U(0.2, 0.5)')
    assert np.abs(msm['s_p_fused'].astype(np.float64) - msm['s_p_unfused']).max() <= 2.0**-25  # one ulp below 0.5
    keep, amb = R.bernoulli_field(KEY, 11, np.arange(4096), 64, msm['s_p_fused'][:4096], msm['s_p_unfused'][:4096])
    n = keep.size
    assert n == N
    bar = SIGMAS * math.sqrt((64 * sp * (1 - sp)).sum())
    print(f'Bernoulli field: kept {keep.sum()} expected {64 * sp.sum():.1f} bar {bar:.1f}; {amb.sum()} ambiguous')
    assert abs(keep.sum() - 64 * sp.sum()) <= bar
    lo = sp < 0.3  # ... and it follows the sample's own threshold
    assert_mean(keep[lo].mean(1) - sp[lo], 0.0, float((sp[lo] * (1 - sp[lo])).mean()) / 64, 'keep rate minus threshold, low thresholds')
    assert_mean(keep[~lo].mean(1) - sp[~lo], 0.0, float((sp[~lo] * (1 - sp[~lo])).mean()) / 64, 'keep rate minus threshold, high thresholds')
    # neighbouring tokens do not share a variate (the four words of a block are four draws)
    u = R.uniform(KEY, 11, 0, R.P_BERNOULLI, np.arange(N))
    assert (u[0::4] != u[1::4]).mean() > 0.999
    r = np.corrcoef(u[:-1], u[1:])[0, 1]
    assert abs(r) <= SIGMAS / math.sqrt(N - 1), r


def test_gates_and_drops():
    steps = np.arange(N)
    for p in (0.1, 0.5):
        d = R.cond_drop(KEY, 31, N, p, 1 - p)
        assert_binomial(int(d[:, 0].sum()), N, p, f'text drop at {p}')
        assert_binomial(int(d[:, 1].sum()), N, 1 - p, f'visual drop at {1 - p}')
        assert_binomial(int((d[:, 0] & d[:, 1]).sum()), N, p * (1 - p), 'both dropped (independent streams)')
    assert R.cond_drop(KEY, 31, 4096, 0.0, 1.0).T.tolist() == [[0] * 4096, [1] * 4096]
    gate = np.array([R.color_jitter_params(KEY, s, 3, 0.9)[:, 0] for s in range(512)])
    assert (gate == gate[:, :1]).all()  # one gate for the whole batch
    assert_binomial(int(gate[:, 0].sum()), 512, 0.9, 'colour-jitter gate, one per step')
    prm = R.color_jitter_params(KEY, 32, N, 1.0)
    assert (prm[:, 0] == 1).all()
    assert_multinomial(prm[:, 2].astype(int), (0.25,) * 4, 'colour-jitter channel choice')
    assert_mean(prm[:, 1].astype(np.float64), 0.0, 1 / 12, 'colour-jitter shift')
    assert_multinomial(R.erase_choice(KEY, steps, [0.5, 0.75, 2.0]), (0.5, 0.25, 0.25), 'erase choice of mask_8x8')
    assert_multinomial(R.erase_choice(KEY, steps, [0.3, 0.5, 0.6]), (0.3, 0.2, 0.5), 'erase choice, last cumulative entry below 1')
    on, box, _ = R.random_erase_box(KEY, 33, N, 8, 0.5, (0.4, 0.8), (0.5, 2.0))
    gate = R.uniform(KEY, 33, np.arange(N), R.P_ERASE, 0) < np.float32(0.5)
    assert (on <= gate).all() and on[gate].mean() > 0.9 and (box[~on] == 0).all()
    assert_binomial(int(gate.sum()), N, 0.5, 'random-erase gate at p 0.5')
    full, fbox, _ = R.random_erase_box(KEY, 33, 4096, 8, 1.0, (0.4, 0.8), (0.5, 2.0))  # the gate does not move the box
    assert (full[gate[:4096]] == on[:4096][gate[:4096]]).all() and (fbox[gate[:4096]] == box[:4096][gate[:4096]]).all()


# ---- the erasing box against the reference semantics on a numpy generator ----------------------------------------------------------------
def test_erasing_box_statistics_match_the_oracle():
    from oracle.frontend import erasing_box
    H = W = 8
    has, box, amb, detail = R.erasing_box(KEY, 41, np.arange(N), R.P_BOX, 0, H, W, (0.2, 0.8), (0.5, 2.0))
    rng = np.random.RandomState(12345)
    n_o = 2**16
    ob = [erasing_box(rng, H, W, (0.2, 0.8), (0.5, 2.0)) for _ in range(n_o)]
    has_o = np.array([b is not None for b in ob])
    box_o = np.array([b if b is not None else (0, 0, 0, 0) for b in ob])
    assert (box[has, 2] < H).all() and (box[has, 3] < W).all() and (box[has, 2:] > 0).all() and (box[~has] == 0).all()
    assert (box[:, 0] >= 0).all() and (box[:, 0] + box[:, 2] <= H).all() and (box[:, 1] >= 0).all() and (box[:, 1] + box[:, 3] <= W).all()
    assert_two_sample(~has, ~has_o, 'no-box rate')
    a, ao = box[has], box_o[has_o]
    assert_two_sample(a[:, 2] * a[:, 3] / (H * W), ao[:, 2] * ao[:, 3] / (H * W), 'area fraction')
    assert_two_sample(np.log(a[:, 2] / a[:, 3]), np.log(ao[:, 2] / ao[:, 3]), 'log aspect')
    assert_two_sample(np.log(a[:, 2] / a[:, 3])**2, np.log(ao[:, 2] / ao[:, 3])**2, 'log aspect squared')
    for col, side, name in ((0, 2, 'row'), (1, 3, 'column')):
        v, vo = (a[:, col] + 0.5) / (H - a[:, side] + 1), (ao[:, col] + 0.5) / (H - ao[:, side] + 1)
        assert_two_sample(v, vo, f'{name} offset, as a fraction of its range')
        assert_two_sample(v**2, vo**2, f'{name} offset squared')
        for s in range(2, H):  # uniform over 0 .. H - side, for every side length that occurs often
            sel = a[a[:, side] == s, col]
            if len(sel) >= 4096:
                assert_multinomial(sel, (1 / (H - s + 1),) * (H - s + 1), f'{name} offset of a box with side {s}')
    # (0.2, 0.8) on an 8 x 8 map always finds a box within ten attempts; BERT's visual eraser (0.55, 0.85) sometimes does not
    has2 = R.erasing_box(KEY, 42, np.arange(2**16), R.P_ERASE, 4, H, W, (0.55, 0.85), (0.5, 2.0))[0]
    has2_o = np.array([erasing_box(rng, H, W, (0.55, 0.85), (0.5, 2.0)) is not None for _ in range(2**14)])
    assert not has2.all() and not has2_o.all()
    assert_two_sample(~has2, ~has2_o, 'no-box rate, scale (0.55, 0.85)')
    near = int(detail['amb'].sum())
    print(f'box roundings within 2^-19 of a tie or of an acceptance flip, f = 8: {near} of {detail["amb"].size} attempts '
          f'({near / detail["amb"].size:.2e} per attempt); ambiguous samples {int(amb.sum())} of {N}')


# ---- stream separation ------------------------------------------------------------------------------------------------------------------
def test_streams_are_uncorrelated_and_no_counter_is_used_twice():
    n = 2**16
    steps = np.arange(n)
    first = {(p, s): R.uniform(KEY, steps, s, p, 0).astype(np.float64) for p in R.PURPOSES.values() for s in (0, 1)}
    bar = SIGMAS / math.sqrt(n)
    worst = 0.0
    for pa, pb in itertools.combinations(R.PURPOSES.values(), 2):
        r = np.corrcoef(first[pa, 0], first[pb, 0])[0, 1]
        worst = max(worst, abs(r))
        assert abs(r) <= bar, f'purposes {pa} and {pb}: correlation {r:.4f} of their first draws over {n} steps (bar {bar:.4f})'
    for p in R.PURPOSES.values():
        r = np.corrcoef(first[p, 0], first[p, 1])[0, 1]
        worst = max(worst, abs(r))
        assert abs(r) <= bar, f'purpose {p}: samples 0 and 1 correlate, {r:.4f} (bar {bar:.4f})'
        r = np.corrcoef(first[p, 0][:-1], first[p, 0][1:])[0, 1]
        assert abs(r) <= SIGMAS / math.sqrt(n - 1), f'purpose {p}: steps s and s + 1 correlate, {r:.4f}'
    print(f'worst correlation between two streams {worst:.4f} (bar {bar:.4f})')
    # every use of a variate in one step has its own (counter block, word)
    for B, T, TS in ((4, 8, 512), (3, 32, 128), (2, 64, 256)):
        d = R.step_draws(B, T, TS)
        c = R.counter_of(7, d[:, 1], d[:, 0], d[:, 2])
        tuples = set(zip(*(np.broadcast_to(v, (len(d),)).tolist() for v in c)))
        assert len(tuples) == len(d), f'B {B} T {T}: {len(d) - len(tuples)} variates are read for two purposes'
        blocks = {(t[0], t[1], t[2], t[3]) for t in tuples}
        streams = {(t[1], t[2]) for t in tuples}
        assert {(t[1], t[2]) for t in blocks} == streams and all(t[3] == 7 for t in blocks)
        assert (d[:, 2] < 2**31).all() and len({(int(p), int(s)) for p, s, _ in d}) == len(streams)


# ---- the GPU cases stay inside their caps -------------------------------------------------------------------------------------------------
def test_gpu_cases_stay_inside_the_ambiguity_caps():
    for shape, prob, pc in itertools.product(R.MSM_SHAPES, R.MSM_PROBS, R.MSM_PC):
        B, T, f = shape
        mask, nfm, dec, tok_amb, smp_amb = R.msm_mask(R.MSM_SEED, R.MSM_STEP, B, T, f, prob, R.MSM_BERN[0], R.MSM_BERN[1], pc)
        field = max(int((dec['strategy'] == 1).sum()) * T * f * f, 1)
        print(f'msm {shape} {prob} pc {pc}: {int(smp_amb.sum())} of {B} samples, {int(tok_amb.sum())} of {field} tokens flagged')
        assert smp_amb.sum() <= R.SAMPLE_CAP * B and tok_amb.sum() <= R.TOKEN_CAP * field
        assert set(np.unique(dec['strategy'])) == {1, 2, 3, 4} and dec['has_box'].any() and (pc == 0 or dec['keep_frame'].any())
        assert ((nfm == 0) == (dec['strategy'] == 2)).all()
    for scale, p in itertools.product(R.ERASE_SCALES, R.ERASE_P):
        on, box, amb = R.random_erase_box(R.ERASE_SEED, R.ERASE_STEP, R.ERASE_B, R.ERASE_F, p, scale, (0.5, 2.0))
        print(f'random erase {scale} p {p}: {int(amb.sum())} of {R.ERASE_B} samples flagged, {int(on.sum())} erased')
        assert amb.sum() <= R.SAMPLE_CAP * R.ERASE_B and on.any()


def test_msm_mask_assembly_follows_the_pinned_oracle():
    """The replica's mask from its own decisions = oracle/frontend.py::build_msm_mask (pinned to the reference's MSM loop by
    tests/test_oracle_golden.py) on those decisions."""
    from oracle.frontend import build_msm_mask
    B, T, f = 257, 5, 4
    mask, nfm, d, _, _ = R.msm_mask(R.MSM_SEED, R.MSM_STEP, B, T, f, (0.25,) * 4, 0.2, 0.5, 0.5)
    for b in range(B):
        s = int(d['strategy'][b])
        bern = mask[b] if s == 1 else None  # (strategy 1: the field is the replica's own; the frames kept on top are what is checked)
        box = tuple(int(v) for v in d['box'][b]) if d['has_box'][b] else None
        m, n = build_msm_mask(s, T, f, bern=bern, box=box, keep_frames=np.nonzero(d['keep_frame'][b])[0])
        assert (m == (mask[b] == 1)).all() and n == nfm[b], b
