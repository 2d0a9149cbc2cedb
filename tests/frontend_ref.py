"""Host replica of the Philox stream of csrc/frontend.hip: every decision of the stochastic front-end as a function of
(key, step, sample, purpose, draw index), in numpy alone.  A plain helper like tests/optim_ref.py and tests/truncate_ref.py (no
fixtures, no pytest settings, nothing imported from mmvid_amd); its own tests are tests/test_frontend_ref_host.py and run without a
GPU, tests/test_frontend_draws_gpu.py holds the kernels to it sample by sample.

THE STREAM ("The front end's draws", has the table of purposes and draw indices):

    draw i of stream (key, step, sample, purpose) = word (i & 3) of Philox4x32-10(counter = {i >> 2, purpose, sample, step}, key)
    variate = float32((word >> 8) * 2^-24)                                          in [0, 1), on the 24-bit grid
    key     = the by-value seed argument XOR (state word 1 | state word 2 << 32),   step = (uint32) of the fp32 counter state[0]

WHAT IS EXACT.  A decision that is one fp32 multiply followed by truncation, a compare, or an fp32 sum of kernel arguments
(`p0 + p1`) has one correct value: it is computed here in np.float32 and the device must give the same.  `u - 0.5f` is exact.

WHAT IS NOT, and how it is fenced (nothing below is taken from observing the kernel):
  * the Bernoulli threshold `bern_lo + (bern_hi - bern_lo) * u`: hipcc may contract it.  Both the fused value (one rounding, exact
    here: fma32) and the unfused one are returned; a token whose variate is not on the same side of both is AMBIGUOUS.
  * erasing_box: logf, expf and sqrtf on the device are not correctly rounded.  sqrt(ea * ar) and sqrt(ea / ar) are evaluated in
    fp64; an attempt is AMBIGUOUS when either lies within BOX_BAND = 2^-19 relative of a rounding tie k + 0.5 (then also the acceptance
    h < H && w < W, a function of the rounded values, could flip).  2^-19 = 16 ulp of fp32: the chain (two logf, a multiply-add, expf,
    a multiply-add, a multiply or a division, sqrtf) is about six operations of at most 1 to 2 ulp each, and the band is that bound
    doubled.  A sample with an ambiguous attempt at or before its accepted one is ambiguous as a whole.
  * the affine matrix th[6] (cosf, sinf, contraction): returned in fp64, compared within TH_TOL = 2^-19 * 1.1 absolute (1.1 is the
    largest scale).
Every function returns its ambiguity flags next to its decisions."""
import numpy as np

U64 = np.uint64
F32 = np.float32
M32 = U64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)

(P_STRATEGY, P_BERNOULLI, P_BOX, P_PC, P_WARP, P_PERM, P_ERASE, P_FACE, P_VCOLOR, P_NULL_TEXT, P_NULL_VISUAL) = range(1, 12)
PURPOSES = dict(P_STRATEGY=1, P_BERNOULLI=2, P_BOX=3, P_PC=4, P_WARP=5, P_PERM=6, P_ERASE=7, P_FACE=8, P_VCOLOR=9, P_NULL_TEXT=10,
                P_NULL_VISUAL=11)

BOX_BAND = 2.0**-19
TH_TOL = 2.0**-19 * 1.1
WARP_PARAMS_BYTES = 176  # {int mode, j1, src_b, src_t, chan; float shift, th[6]; int perm[32]}
BOX_ATTEMPTS = 10
PERM_ATTEMPTS = 16


def _w(x):
    """Anything integer -> uint64 array holding the low 32 bits."""
    x = np.asarray(x)
    return (x if x.dtype == U64 else x.astype(np.int64).astype(U64)) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), vectorised: counters and key
    words are uint64 arrays (broadcast against each other) masked to 32 bits -> the four output words, same type."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_w(c0), _w(c1), _w(c2), _w(c3), _w(k0), _w(k1))
    s32 = U64(32)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def key64(seed_argument=0, state_word1=0, state_word2=0):
    """The 64-bit key of a call: its by-value seed XOR the seed words of the device state (0, 0 for step_dev = NULL)."""
    return (int(seed_argument) ^ (int(state_word1) & 0xFFFFFFFF) ^ ((int(state_word2) & 0xFFFFFFFF) << 32)) & 0xFFFFFFFFFFFFFFFF


def state_words(step, seed):
    """The four 32-bit words of a front-end state holding `step` (as fp32: the counter) and `seed`."""
    return [int(np.array([step], F32).view(np.uint32)[0]), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, 0]


def counter_of(step, sample, purpose, i):
    """(c0, c1, c2, c3, word) of draw i: the Philox counter block it comes from and which of the block's four words it is."""
    i = _w(i)
    return i >> U64(2), _w(purpose), _w(sample), _w(step), i & U64(3)


def u01(word):
    """The kernel's u01: float32((word >> 8) * 2^-24): exact, the 24 high bits of the word."""
    return (_w(word) >> U64(8)).astype(F32) * F32(2.0**-24)


def uniform(key, step, sample, purpose, i):
    """Draw i of stream (key, step, sample, purpose) -> float32 in [0, 1).  Every argument but `key` broadcasts."""
    c0, c1, c2, c3, word = counter_of(step, sample, purpose, i)
    r = philox4x32_10(c0, c1, c2, c3, int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF)
    word = np.broadcast_to(word, r[0].shape)
    return u01(np.where(word == 0, r[0], np.where(word == 1, r[1], np.where(word == 2, r[2], r[3]))))


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product is exact in fp64, the sum comes with its error term (TwoSum), and the
    one case where rounding the fp64 sum to fp32 differs from rounding the exact value -- the fp64 sum is an fp32 tie and the
    error term is not zero -- is decided by the error term's sign."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    rd = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > rd, F32(np.inf), F32(-np.inf)).astype(F32)).astype(np.float64)
    tie = (rd != s) & (np.abs(s - rd) == np.abs(other - s)) & (e != 0)
    return np.where(tie & (np.sign(e) == np.sign(other - s)), other, rd).astype(F32)


def _trunc_scaled(u, n):
    """(int)(u * (float)n) as the kernels write it: one fp32 multiply, truncation."""
    return (np.asarray(u, F32) * F32(n)).astype(np.int64)


def _choice(u, probs):
    """np.random.choice as the kernels write it: the index of the first k with u < p[0] + ... + p[k], the sums taken in fp32 from the
    left; the last alternative takes the rest (its probability is never read)."""
    acc, out = F32(0), np.full(np.shape(u), len(probs) - 1, np.int64)
    found = np.zeros(np.shape(u), bool)
    for k, p in enumerate(probs[:-1]):
        acc = F32(acc + F32(p)) if k else F32(p)
        hit = ~found & (u < acc)
        out[hit], found = k, found | hit
    return out


# ---- torchvision RandomErasing.get_params as csrc/frontend.hip::erasing_box draws it -----------------------------------------------------
def erasing_box(key, step, sample, purpose, base, H, W, scale, ratio):
    """-> (has_box [B] bool, box [B, 4] = (i, j, h, w) (zeros without a box), ambiguous [B] bool, detail).  Attempt a uses draws
    base + 4 a + {0: area, 1: aspect, 2: row offset, 3: column offset}; the first attempt with h < H and w < W is taken.
    detail: dict of the per-attempt fp64 values (hh, ww [B, 10]) and flags, for the host tests."""
    sample = np.asarray(sample).reshape(-1, 1)
    step = np.asarray(step).reshape(-1, 1) if np.ndim(step) else step
    a = np.arange(BOX_ATTEMPTS).reshape(1, -1)
    u = [uniform(key, step, sample, purpose, base + 4 * a + k) for k in range(4)]
    s0, s1, r0, r1 = (float(F32(v)) for v in (scale[0], scale[1], ratio[0], ratio[1]))
    ea = float(H * W) * (s0 + (s1 - s0) * u[0].astype(np.float64))
    ar = np.exp(np.log(r0) + (np.log(r1) - np.log(r0)) * u[1].astype(np.float64))
    hh, ww = np.sqrt(ea * ar), np.sqrt(ea / ar)
    h, w = np.rint(hh).astype(np.int64), np.rint(ww).astype(np.int64)  # rintf: ties to even, as np.rint
    ok = (h < H) & (w < W)
    amb = np.zeros(h.shape, bool)
    for sh in (1 - BOX_BAND, 1 + BOX_BAND):
        for sw in (1 - BOX_BAND, 1 + BOX_BAND):
            h2, w2 = np.rint(hh * sh).astype(np.int64), np.rint(ww * sw).astype(np.int64)
            amb |= (h2 != h) | (w2 != w) | (((h2 < H) & (w2 < W)) != ok)
    has = ok.any(1)
    first = np.where(has, ok.argmax(1), BOX_ATTEMPTS - 1)
    rows = np.arange(h.shape[0])
    ambiguous = (amb & (a <= first[:, None])).any(1)
    hb, wb = h[rows, first], w[rows, first]
    bi = np.minimum((u[2][rows, first] * (H - hb + 1).astype(F32)).astype(np.int64), H - hb)
    bj = np.minimum((u[3][rows, first] * (W - wb + 1).astype(F32)).astype(np.int64), W - wb)
    box = np.stack([bi, bj, hb, wb], 1) * has[:, None]
    return has, box, ambiguous, dict(hh=hh, ww=ww, ok=ok, amb=amb, first=first)


# ---- mmvid_msm_masks ------------------------------------------------------------------------------------------------------------------
def msm_decisions(key, step, B, T, f, strategy_prob, bern_lo, bern_hi, pc_prob):
    """Thread 0 of msm_mask_kernel for samples 0..B-1 (`step` a scalar or [B]) -> dict:
    strategy [B] 1..4; s_p_fused, s_p_unfused [B] float32; has_box [B], box [B, 4] (i, j, h, w), box_ambiguous [B] (all three only for
    strategies 3 and 4, False / 0 otherwise); kept_count [B] (0 = the gate failed); keep_frame [B, T] bool."""
    b = np.arange(B)
    strategy = 1 + _choice(uniform(key, step, b, P_STRATEGY, 0), list(strategy_prob)[:3] + [None])
    u1 = uniform(key, step, b, P_STRATEGY, 1)
    lo, d = F32(bern_lo), F32(F32(bern_hi) - F32(bern_lo))
    s_p_unfused, s_p_fused = (d * u1 + lo).astype(F32), fma32(d, u1, lo)
    has, box, amb = np.zeros(B, bool), np.zeros((B, 4), np.int64), np.zeros(B, bool)
    boxed = np.nonzero(strategy >= 3)[0]  # only strategies 3 and 4 draw a box
    if len(boxed):
        stp = np.asarray(step)[boxed] if np.ndim(step) else step
        has[boxed], box[boxed], amb[boxed], _ = erasing_box(key, stp, boxed, P_BOX, 0, f, f, (0.2, 0.8), (0.5, 2.0))
    keep_frame, count = np.zeros((B, T), bool), np.zeros(B, np.int64)
    if float(pc_prob) > 0 and T >= 2:
        gate = uniform(key, step, b, P_PC, 0) < F32(pc_prob)
        count = np.minimum(1 + _trunc_scaled(uniform(key, step, b, P_PC, 1), T // 2), T // 2) * gate
        stp = np.asarray(step).reshape(-1, 1) if np.ndim(step) else step
        ut = uniform(key, stp, b[:, None], P_PC, 2 + np.arange(T)[None, :])  # [B, T]: the count smallest are kept
        q = np.arange(T)
        before = (ut[:, None, :] < ut[:, :, None]) | ((ut[:, None, :] == ut[:, :, None]) & (q[None, None, :] < q[None, :, None]))
        keep_frame = before.sum(2) < count[:, None]
    return dict(strategy=strategy, s_p_fused=s_p_fused, s_p_unfused=s_p_unfused, has_box=has, box=box, box_ambiguous=amb,
                kept_count=count, keep_frame=keep_frame)


def bernoulli_field(key, step, samples, TS, s_p_fused, s_p_unfused):
    """torch.bernoulli(ones * p) of strategy 1: token p of sample b is visible iff draw p of stream (b, P_BERNOULLI) < s_p.
    -> (keep [n, TS] bool by the fused threshold, ambiguous [n, TS] bool: the unfused threshold decides otherwise)."""
    samples = np.asarray(samples).reshape(-1, 1)
    step = np.asarray(step).reshape(-1, 1) if np.ndim(step) else step
    u = uniform(key, step, samples, P_BERNOULLI, np.arange(TS)[None, :])
    keep = u < np.asarray(s_p_fused, F32).reshape(-1, 1)
    return keep, keep != (u < np.asarray(s_p_unfused, F32).reshape(-1, 1))


def msm_mask(key, step, B, T, f, strategy_prob, bern_lo, bern_hi, pc_prob):
    """The whole output of mmvid_msm_masks -> (mask1 [B, T*f*f] uint8, not_fully_masked [B] float32, decisions, token_ambiguous
    [B, T*f*f] bool, sample_ambiguous [B] bool).  A flagged sample's mask may differ anywhere, a flagged token's only there."""
    d = msm_decisions(key, step, B, T, f, strategy_prob, bern_lo, bern_hi, pc_prob)
    n = f * f
    mask = np.zeros((B, T, f, f), bool)
    tok_amb = np.zeros((B, T * n), bool)
    s1 = np.nonzero(d['strategy'] == 1)[0]
    if len(s1):
        stp = np.asarray(step)[s1] if np.ndim(step) else step
        keep, amb = bernoulli_field(key, stp, s1, T * n, d['s_p_fused'][s1], d['s_p_unfused'][s1])
        mask[s1], tok_amb[s1] = keep.reshape(-1, T, f, f), amb
    y, x = np.arange(f)[None, :, None], np.arange(f)[None, None, :]
    bx = d['box'][:, :, None, None]
    inside = d['has_box'][:, None, None] & (y >= bx[:, 0]) & (y < bx[:, 0] + bx[:, 2]) & (x >= bx[:, 1]) & (x < bx[:, 1] + bx[:, 3])
    s3, s4 = d['strategy'] == 3, d['strategy'] == 4
    mask[s3] = ~inside[s3][:, None]
    mask[s4] = inside[s4][:, None]
    mask |= d['keep_frame'][:, :, None, None]
    tok_amb &= ~np.repeat(d['keep_frame'], n, 1)
    nfm = np.where(d['strategy'] == 2, F32(0), F32(1)).astype(F32)
    return mask.reshape(B, T * n).astype(np.uint8), nfm, d, tok_amb, d['box_ambiguous'].copy()


# ---- mmvid_vid_warp_draw --------------------------------------------------------------------------------------------------------------
WARP_ANGLE = F32(F32(F32(3.14159265358979323846) * F32(30.0)) / F32(180.0))


def warp_params(key, step, B, T, strategy_prob, samples=None):
    """warp_params_kernel for samples 0..B-1 of a batch of B (or for `samples`, each with its entry of `step`: many steps of a small
    batch at once) -> dict of arrays: mode, j1, src_b, src_t, chan [n] int; shift [n] float32 (exact); th [n, 6] float64 (compare
    within TH_TOL); perm [n, 32] int (identity outside mode 1 and beyond T)."""
    b = np.arange(B) if samples is None else np.asarray(samples)
    n = len(b)
    g = lambda i: uniform(key, step, b, P_WARP, i)  # noqa: E731
    mode = _choice(g(0), list(strategy_prob)[:3] + [None])
    j1 = np.minimum(_trunc_scaled(g(1), T), T - 1)
    src_b, src_t, chan = b.copy(), j1.copy(), np.zeros(n, np.int64)
    perm = np.tile(np.arange(32), (n, 1))
    m0, m1, m2, m3 = (mode == k for k in range(4))
    if B > 1:  # a frame of ANOTHER sample: uniform over the B - 1 others
        o = np.minimum(_trunc_scaled(g(2), B - 1), B - 2)
        src_b = np.where(m0, np.where(o >= b, o + 1, o), src_b)
    src_t = np.where(m0, np.minimum(_trunc_scaled(g(3), T), T - 1), src_t)
    # a non-identity permutation: Fisher-Yates from stream P_PERM, draw attempt * 32 + t bounds position t; up to 16 attempts
    todo = np.nonzero(m1)[0]
    for attempt in range(PERM_ATTEMPTS):
        if not len(todo):
            break
        cand = np.tile(np.arange(T), (len(todo), 1))
        rows = np.arange(len(todo))
        stp = np.asarray(step)[todo] if np.ndim(step) else step
        for t in range(T - 1, 0, -1):
            r = np.minimum(_trunc_scaled(uniform(key, stp, b[todo], P_PERM, attempt * 32 + t), t + 1), t)
            cand[rows, t], cand[rows, r] = cand[rows, r].copy(), cand[rows, t].copy()
        perm[todo, :T] = cand
        again = (cand == np.arange(T)).all(1) & (T >= 2)
        todo = todo[again]
    shift = np.where(m2, g(2) - F32(0.5), F32(0)).astype(F32)
    chan = np.where(m2, np.minimum(_trunc_scaled(g(3), 4), 3), chan)
    ang = float(WARP_ANGLE)
    a = -ang + 2.0 * ang * g(2).astype(np.float64)
    t1, t2 = (float(F32(-0.1)) + float(F32(0.2)) * g(i).astype(np.float64) for i in (3, 4))
    sc = float(F32(0.9)) + float(F32(0.2)) * g(5).astype(np.float64)
    th = np.stack([sc * np.cos(a), sc * np.sin(-a), t1, sc * np.sin(a), sc * np.cos(a), t2], 1) * m3[:, None]
    return dict(mode=mode, j1=j1, src_b=src_b, src_t=src_t, chan=chan, shift=shift, th=th, perm=perm)


def read_warp_params(raw, B):
    """The bytes of params_scratch (uint8 array of B * 176) in the shape of warp_params()'s result (th as float32)."""
    raw = np.ascontiguousarray(np.asarray(raw, np.uint8)[:B * WARP_PARAMS_BYTES])
    i, f = raw.view(np.int32).reshape(B, 44), raw.view(F32).reshape(B, 44)
    return dict(mode=i[:, 0].astype(np.int64), j1=i[:, 1].astype(np.int64), src_b=i[:, 2].astype(np.int64), src_t=i[:, 3].astype(np.int64),
                chan=i[:, 4].astype(np.int64), shift=f[:, 5].copy(), th=f[:, 6:12].copy(), perm=i[:, 12:44].astype(np.int64))


# ---- token erasing, colour jitter, condition drop --------------------------------------------------------------------------------------
def erase_choice(key, step, cumprob):
    """erase_choice_kernel's one draw per call (sample 0, P_FACE, draw 0): the first alternative whose fp32 cumulative probability is
    above it, the LAST one when none is.  `step` may be an array -> array of choices."""
    u = uniform(key, step, 0, P_FACE, 0)
    cum = np.asarray(cumprob, F32)
    below = u[..., None] < cum
    return np.where(below.any(-1), below.argmax(-1), len(cum) - 1)


def random_erase_box(key, step, B, f, p, scale, ratio):
    """random_erase_tokens_kernel without erase_half -> (on [B] bool, box [B, 4] (i, j, h, w), ambiguous [B] bool): draw 0 of stream
    (b, P_ERASE) is torchvision's `torch.rand(1) < p`, the box attempts start at draw 4."""
    b = np.arange(B)
    gate = np.nonzero(uniform(key, step, b, P_ERASE, 0) < F32(p))[0]  # only these samples go on to draw a box
    on, box, amb = np.zeros(B, bool), np.zeros((B, 4), np.int64), np.zeros(B, bool)
    if len(gate):
        stp = np.asarray(step)[gate] if np.ndim(step) else step
        on[gate], box[gate], amb[gate], _ = erasing_box(key, stp, gate, P_ERASE, 4, f, f, scale, ratio)
    return on, box, amb


def color_jitter_params(key, step, B, p):
    """visual_color_kernel -> [B, 3] float32 as params_out: {gate, shift, channel choice}.  The gate is ONE draw per call (sample 0 of
    P_VCOLOR), sample b's own stream is sample b + 1: shift = draw 0 - 0.5 (exact), choice = (int)(draw 1 * 4)."""
    b = np.arange(B)
    gate = uniform(key, step, 0, P_VCOLOR, 0) < F32(p)
    shift = uniform(key, step, b + 1, P_VCOLOR, 0) - F32(0.5)
    chan = np.minimum(_trunc_scaled(uniform(key, step, b + 1, P_VCOLOR, 1), 4), 3)
    return np.stack([np.broadcast_to(gate, (B,)).astype(F32), shift.astype(F32), chan.astype(F32)], 1)


def cond_drop(key, step, B, p_text, p_visual):
    """cond_drop_kernel -> decided [B, 2] uint8 = {text dropped, visual dropped}: draw 0 of (b, P_NULL_TEXT) / (b, P_NULL_VISUAL)."""
    b = np.arange(B)
    return np.stack([uniform(key, step, b, P_NULL_TEXT, 0) < F32(p_text), uniform(key, step, b, P_NULL_VISUAL, 0) < F32(p_visual)],
                    1).astype(np.uint8)


def step_draws(B, T, TS):
    """Every (purpose, sample, draw index) a step with B samples, T frames and TS target tokens per sample can read, one row per USE
    (two uses of one variate would be two rows) -> int array [n, 3].  The layout table of DESIGN.md as data."""
    rows = []

    def use(purpose, samples, draws):
        s, d = np.meshgrid(np.asarray(samples), np.asarray(draws), indexing='ij')
        rows.append(np.stack([np.full(s.size, purpose), s.reshape(-1), d.reshape(-1)], 1))

    b = np.arange(B)
    use(P_STRATEGY, b, [0, 1])                                     # strategy, Bernoulli probability
    use(P_BERNOULLI, b, np.arange(TS))                             # one per token
    use(P_BOX, b, np.arange(4 * BOX_ATTEMPTS))                     # attempt a: 4a .. 4a + 3
    use(P_PC, b, np.arange(2 + T))                                 # gate, count, one per frame
    use(P_WARP, b, np.arange(6))                                   # mode, j1, then 2..5 by mode
    use(P_PERM, b, [a * 32 + t for a in range(PERM_ATTEMPTS) for t in range(1, min(T, 32))])  # (the warp takes T <= 32)
    use(P_ERASE, b, [0] + list(range(4, 4 + 4 * BOX_ATTEMPTS)))    # gate, then the box attempts
    use(P_FACE, [0], [0])                                          # one per call
    use(P_VCOLOR, [0], [0])                                        # the gate, one per call ...
    use(P_VCOLOR, b + 1, [0, 1])                                   # ... and sample b's shift and channel on stream b + 1
    use(P_NULL_TEXT, b, [0])
    use(P_NULL_VISUAL, b, [0])
    return np.concatenate(rows)


# ---- the cases of tests/test_frontend_draws_gpu.py: kept here so that tests/test_frontend_ref_host.py can prove, without a GPU, that
# the replica's own flags stay inside the cap at exactly these seeds ---------------------------------------------------------------------
SAMPLE_CAP = 1e-3   # share of flagged samples a case may have
TOKEN_CAP = 10e-6   # share of flagged tokens a Bernoulli field may have
STATE_SEEDS = (0, 1234, 0xFFFFFFFFFFFFFFFF, 0x7FC000017F800001, 0x0000000100000001)  # the last two: NaN / inf / denormal fp32 bit patterns
STATE_STEPS = (0, 1, 7, 2**24 - 1)
MSM_SHAPES = ((1024, 8, 8), (257, 5, 4), (64, 64, 2))
MSM_PROBS = ((0.7, 0.1, 0.1, 0.1), (0.25, 0.25, 0.25, 0.25))
MSM_PC = (0.0, 0.5, 1.0)
MSM_BERN = (0.2, 0.5)
MSM_SEED, MSM_STEP = 0x5EED0001C0FFEE11, 3
ERASE_SCALES = ((0.55, 0.85), (0.4, 0.8))  # BERT's visual_eraser, ART-V's eraser
ERASE_P = (0.5, 1.0)
ERASE_B, ERASE_F = 1024, 8
ERASE_SEED, ERASE_STEP = 0x0BADC0DE12345678, 5
