"""The truncation rule of csrc/sample.hip (top-k and nucleus) restated in numpy fp64, and the inputs the two test files share.  A plain
helper (no fixtures, no pytest settings); its own tests are in tests/test_truncate_host.py and run without a GPU.

The rule, per row of fp32 values g: the classes are ordered by g descending, ties to the lower index, -0.0 == +0.0.  top-k keeps the
first k of the order (1 <= k < V, anything else: off).  With P_c = exp(g_c / logit_div - max), S = sum P and M_before(c) the mass
ordered before c, top-p keeps c iff M_before(c) < top_p * S (top_p >= 1: off).  Kept classes hold their value, the others -inf.

The margin `DELTA` of the nucleus comparison.  The device evaluates M_before(c) < top_p * S in fp32, this file in fp64 from the same
fp32 g, so a row whose edge lies within the device's rounding of the threshold may legitimately keep one class more or less.  The
test therefore demands  nucleus(p - DELTA) <= device set <= nucleus(p + DELTA)  (`sandwich`), which is equality wherever the two
agree (a "tight" row).  DELTA is derived, not measured on the kernel:

* one device P_j = expf(g_j * (1 / logit_div) - max).  Every logit_div of the cases below is a power of two, so the reciprocal and the
  product are exact (a fused multiply-add changes nothing) and the maximum is the exact maximum of the products; the subtraction
  rounds once, at most |d_j| 2^-24 absolute in the argument, d_j = g_j / logit_div - max, which is a relative error of the same size in
  the exponential; expf is within 2 ulp.  So the relative error of P_j is at most (|d_j| + 2) 2^-24; the bound used is the more generous
  (2 |d_j| + 2) 2^-24.  (A logit_div that is no power of two would add the roundings of the two products, |g_j / logit_div| 2^-24 and
  |max| 2^-24: such a case needs its own margin and is not among the inputs.)
* weighted by P_j / S, any sum of P's is off by at most (2 A + 2) 2^-24 relative to S, A = sum_j P_j |d_j| / S (`mean_distance`).
* the summation the kernel builds: every lane adds its <= V / 64 = 32 slots in slot order, then one butterfly of 6 levels (four DPP
  steps and two lane swaps; a different pairing than the shuffle butterfly, the same depth).  Each term passes through at most
  32 + 6 = 38 fp32 additions of non-negative numbers: at most 38 * 2^-24 relative.
* M_before and S both carry these two terms, and the product top_p * S one more rounding, 2^-24.
* ties at the nucleus edge: the j-th class at the edge key is admitted while m_above + j * P < top_p * S, m_above the masked sum of the
  classes above the key.  The product j * P (j < 2^24: exact as a float) and the addition round once each, 2 * 2^-24 more on the left
  side (one rounding when the two fuse).  The inputs below are tie free, where j = 0 and the term vanishes; it is counted all the same.
* for the inputs below A <= 4 (asserted by the host test), so the threshold comparison is off by at most
  2 * ((2 * 4 + 2) + 38) * 2^-24 + 2^-24 + 2 * 2^-24 = 99 * 2^-24 < 2^-17 of S.
DELTA = 2^-16 is that bound with a factor of two in hand."""
import numpy as np
import torch

DELTA = 2.0**-16
NEG_INF = float('-inf')

# ---- the nucleus inputs: 4 * randn from fixed seeds, 512 rows per case
NUCLEUS_ROWS = 512
NUCLEUS_CASES = [(V, p, 1.0) for V in (200, 256, 1024) for p in (0.5, 0.9, 0.95)] + \
                [(256, p, div) for div in (0.5, 2.0) for p in (0.5, 0.9, 0.95)]  # (V, top_p, logit_div)
MAX_LOOSE_SHARE = 0.05  # of the rows of a case may be not tight
MAX_MEAN_DISTANCE = 4.0  # the A of the derivation above


def nucleus_input(V):
    """fp32 [NUCLEUS_ROWS, V] = 4 * randn, seeded by V (every case of one V reads the same rows)."""
    gen = torch.Generator().manual_seed(9100 + V)
    return (4.0 * torch.randn(NUCLEUS_ROWS, V, generator=gen)).numpy()


def _rows(g):
    g = np.asarray(g, dtype=np.float32)
    return g.reshape(-1, g.shape[-1]), g.shape


def order(g):
    """The rank order: order(g)[..., n] is the class at rank n (value descending, ties to the lower index, -0.0 == +0.0)."""
    g2, shape = _rows(g)
    v = g2.astype(np.float64) + 0.0  # (-0.0 + 0.0 = +0.0)
    return np.argsort(-v, axis=1, kind='stable').reshape(shape)


def _from_ranks(g, keep_rank):
    """keep_rank [rows, V] bool by RANK -> bool by class."""
    g2, shape = _rows(g)
    o = order(g2)
    keep = np.zeros(g2.shape, dtype=bool)
    np.put_along_axis(keep, o, keep_rank, axis=1)
    return keep.reshape(shape)


def topk_set(g, k):
    """bool like g: the classes top-k keeps (all of them when k is outside [1, V))."""
    g2, shape = _rows(g)
    V = g2.shape[1]
    if k is None or not 1 <= k < V:
        return np.ones(shape, dtype=bool)
    return _from_ranks(g, np.broadcast_to(np.arange(V) < k, g2.shape))


def masses(g, logit_div=1.0):
    """-> (P [rows, V] fp64 in class order, d = g / logit_div - max) from the fp32 g; a row of -inf has no mass."""
    g2, _ = _rows(g)
    x = g2.astype(np.float64) / float(logit_div)
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        d = np.where(np.isneginf(mx), NEG_INF, x - mx)
    return np.exp(d), d


def nucleus_set(g, q, logit_div=1.0):
    """bool like g: the classes top-p keeps at threshold q (all of them when q >= 1)."""
    g2, shape = _rows(g)
    if q is None or q >= 1.0:
        return np.ones(shape, dtype=bool)
    P, _ = masses(g2, logit_div)
    Po = np.take_along_axis(P, order(g2), axis=1)
    before = np.cumsum(Po, axis=1) - Po
    return _from_ranks(g, before < q * Po.sum(axis=1, keepdims=True))


def mean_distance(g, logit_div=1.0):
    """A per row: sum_j P_j |d_j| / S."""
    P, d = masses(g, logit_div)
    return (P * np.abs(np.where(P > 0, d, 0.0))).sum(axis=1) / P.sum(axis=1)


def sandwich(g, p, delta=DELTA, logit_div=1.0):
    """-> (S_lo, S_hi): the nucleus sets at p - delta and at p + delta.  A row is tight when the two are equal."""
    return nucleus_set(g, p - delta, logit_div), nucleus_set(g, p + delta, logit_div)


def truncated(g, keep):
    """The kernel's output for a kept set: g where kept, -inf elsewhere."""
    g = np.asarray(g, dtype=np.float32)
    return np.where(keep, g, np.float32(NEG_INF)).astype(np.float32)


def is_head(g, keep):
    """Per row: is the kept set a head of order(g)?"""
    g2, _ = _rows(g)
    ko = np.take_along_axis(np.asarray(keep).reshape(g2.shape), order(g2), axis=1)
    return (ko[:, 1:] <= ko[:, :-1]).all(axis=1)


# ---- crafted rows: ties at the top-k edge.  V = 256; the background is distinct and below every crafted value.
TIE_V = 256


def _background():
    return (-10.0 - 0.01 * np.arange(TIE_V)).astype(np.float32)


def tie_rows():
    """[(name, g fp32 [256], k, the kept indices)]"""
    rows = []
    rows.append(('all equal', np.full(TIE_V, 1.5, np.float32), 5, [0, 1, 2, 3, 4]))
    top3 = _background()
    top3[[0, 1, 2]] = (5.0, 4.0, 3.0)
    g = top3.copy()
    g[62:67] = 1.0  # lanes 62, 63 of slot 0, then lanes 0-2 of slot 1 (class lane + 64 i is slot i of its lane)
    rows.append(('ties 62-66 straddle k', g, 6, [0, 1, 2, 62, 63, 64]))
    g = top3.copy()
    g[126:131] = 1.0  # lanes 62, 63 of slot 1, then lanes 0-2 of slot 2: k ends before the slot edge 127 | 128 is crossed
    rows.append(('ties 126-130 straddle k', g, 5, [0, 1, 2, 126, 127]))
    g = top3.copy()
    g[62:67] = 1.0
    g[126:131] = 1.0
    rows.append(('both tie groups, k inside the second', g, 10, [0, 1, 2, 62, 63, 64, 65, 66, 126, 127]))
    g = _background()
    g[3], g[5], g[7] = -0.0, 0.0, 0.0
    rows.append(('-0.0 beside +0.0', g, 2, [3, 5]))
    g = _background()
    g[[10, 100, 200]] = 9.0
    rows.append(('the maximum three times', g, 2, [10, 100]))
    rows.append(('all -inf', np.full(TIE_V, NEG_INF, np.float32), 5, []))
    return rows
