"""Host replica of mmvid_segment_stats (trainer telemetry), in numpy fp32, written from the section "Trainer telemetry" of
include/mmvid_hip_ext.h alone: the chunking, the per-chunk and per-segment summation order, the finite filter, the lazy-row rule, the
skip rule, the formula of the update d and the slot arithmetic of the ring.  A plain helper like tests/guarded.py (no fixtures, no
pytest settings); tests/test_telemetry_host.py holds it to fp64, tests/test_telemetry_gpu.py holds the kernels to it bit for bit.

Every numpy operation below on float32 arrays is one correctly rounded fp32 operation (numpy never contracts), which is what the
header demands of the kernel."""
import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
CHUNK = 4096  # MMVID_TELEMETRY_CHUNK (include/mmvid_hip.h); tests/test_telemetry_host.py holds the two together
_libm = ctypes.CDLL(ctypes.util.find_library('m'))
_libm.powf.argtypes, _libm.powf.restype = [ctypes.c_float, ctypes.c_float], ctypes.c_float


def plan(offsets, numels, chunk=CHUNK):
    """(seg_off, seg_len, seg_chunk0, chunks): segment s has ceil(len / chunk) chunks, numbered from seg_chunk0[s] on."""
    chunk0, total = [], 0
    for n in numels:
        chunk0.append(total)
        total += -(-int(n) // chunk)
    return [int(o) for o in offsets], [int(n) for n in numels], chunk0, total


def host_scalars(lr, beta1, beta2, t):
    """(lr / bc1, bc2s) as the C entry computes them on the host when the step is an argument: bc1 = 1.f - powf(beta1, (float)t),
    bc2s = sqrtf(1.f - powf(beta2, (float)t)) with the C library's powf; lr / bc1 is the one fp32 division the kernel performs."""
    bc1 = F32(1.0) - F32(_libm.powf(float(F32(beta1)), float(t)))
    bc2s = np.sqrt(F32(1.0) - F32(_libm.powf(float(F32(beta2)), float(t))))
    return F32(lr) / bc1, F32(bc2s)


def _block_tree(a):
    """[..., 256] -> [...]: each wave of 64 by the halving tree (x[i] + x[i + 32], then 16 ... 1), then (w0 + w1) + (w2 + w3)."""
    w = a.reshape(a.shape[:-1] + (4, 64))
    h = 32
    while h >= 1:
        w = w[..., :h] + w[..., h:2 * h]
        h //= 2
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def chunk_sums(terms):
    """Pass 1.  terms: fp32 [L], the squares of a segment's elements with +0 where an element does not count -> fp32 [ceil(L / CHUNK)]."""
    L = terms.shape[0]
    nc = -(-L // CHUNK)
    t = np.zeros(nc * CHUNK, F32)
    t[:L] = terms
    t = t.reshape(nc, 4, 256, 4)  # [chunk][trip r][thread T][lane e]: element 1024 r + 4 T + e
    q = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    a = np.zeros((nc, 256), F32)
    for r in range(4):
        a = a + q[:, r]
    return _block_tree(a)


def sum_in_order(c):
    """Pass 2.  c: fp32 [C] -> the sum: thread T adds c[T], c[T + 256], ... in order, then the block tree."""
    C = c.shape[0]
    trips = max(-(-C // 256), 1)
    t = np.zeros(trips * 256, F32)
    t[:C] = c
    t = t.reshape(trips, 256)
    a = np.zeros(256, F32)
    for r in range(trips):
        a = a + t[r]
    return _block_tree(a)


def sum_depth(L):
    """The largest number of fp32 ADDITIONS between one term of a segment of length L and its sum, counted from the header text:
    2 (a thread's four elements) + 4 (its four trips) + 6 (wave) + 2 (four waves) in pass 1; ceil(C / 256) + 6 + 2 in pass 2."""
    C = -(-L // CHUNK)
    return 2 + 4 + 6 + 2 + max(-(-C // 256), 1) + 6 + 2


def lazy_mask(lazy, lo, hi):
    """bool [hi - lo]: the elements of [lo, hi) that sit in an unflagged row of the lazy table.  lazy = (flags uint8 [rows], table_lo,
    rows, rowlen) or None."""
    out = np.zeros(hi - lo, bool)
    if lazy is None:
        return out
    flags, tlo, rows, rowlen = lazy
    i = np.arange(lo, hi)
    inside = (i >= tlo) & (i < tlo + rows * rowlen)
    row = np.clip((i - tlo) // rowlen, 0, max(rows - 1, 0))
    out[inside] = np.asarray(flags)[row[inside]] == 0
    return out


def update(stepsz, m, v, bc2s, eps):
    """d = ((lr / bc1) * m) / (sqrtf(v) / bc2s + eps), every operation one fp32 operation."""
    with np.errstate(all='ignore'):
        return (F32(stepsz) * m) / (np.sqrt(v) / F32(bc2s) + F32(eps))


def record(g, p, m, v, tables, stepsz, bc2s, eps, lazy=None, skip=False):
    """One record: (ring_f fp32 [S, 4] = g_sumsq, g_absmax, p_sumsq, d_sumsq; ring_i int32 [S, 2] = g_nonfinite, g_count; the total)."""
    off, ln, _, _ = tables
    S = len(off)
    rf, ri = np.zeros((S, 4), F32), np.zeros((S, 2), np.int32)
    with np.errstate(all='ignore'):
        for s in range(S):
            lo, hi = off[s], off[s] + ln[s]
            gs, ps = g[lo:hi].astype(F32), p[lo:hi].astype(F32)
            untouched = lazy_mask(lazy, lo, hi)
            counts = np.isfinite(gs) & ~untouched
            gz = np.where(counts, gs, F32(0))
            rf[s, 0] = sum_in_order(chunk_sums(gz * gz))
            rf[s, 1] = np.abs(gz).max()
            rf[s, 2] = sum_in_order(chunk_sums(ps * ps))
            if not skip:
                d = np.where(untouched, F32(0), update(stepsz, m[lo:hi].astype(F32), v[lo:hi].astype(F32), bc2s, eps))
                rf[s, 3] = sum_in_order(chunk_sums(d * d))
            ri[s, 0] = int((~np.isfinite(gs) & ~untouched).sum())
            ri[s, 1] = int((~untouched).sum())
    return rf, ri, sum_in_order(rf[:, 0].copy())


def slot_of(count, every, slots):
    """The ring slot call number `count` writes, or None where it is gated (count % every != 0)."""
    return None if count % every != 0 else (count // every) % slots


class Ring:
    """The device state of the ring and what a sequence of calls leaves in it."""

    def __init__(self, segments, every, slots):
        self.every, self.slots, self.count = every, slots, 0
        self.ring_f, self.ring_i = np.zeros((slots, segments, 4), F32), np.zeros((slots, segments, 2), np.int32)
        self.head_i, self.head_f = np.zeros((slots, 4), np.int32), np.zeros((slots, 2), F32)

    def call(self, rec, t, skip, lr):
        """rec: what record() returns for this call's buffers.  -> the slot written, or None."""
        k = slot_of(self.count, self.every, self.slots)
        if k is not None:
            self.ring_f[k], self.ring_i[k] = rec[0], rec[1]
            self.head_i[k] = [self.count, int(t), int(bool(skip)), 1]
            self.head_f[k] = [F32(lr), rec[2]]
        self.count += 1
        return k
