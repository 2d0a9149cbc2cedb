"""Host replica of the weight-EMA rule (include/mmvid_hip_ext.h: mmvid_ema_update; csrc/ema.hip), bit for bit in numpy:

    t = the count of finished optimiser steps, this one included, as an fp32
    d = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay        a = 1.f - d
    ema' = fmaf(a, p - ema, ema)

Every operation is one correctly rounded fp32 operation: numpy's float32 add / subtract / divide are, and the fmaf is
frontend_ref.fma32 (an exact product in fp64, TwoSum, the tie decided by the error term).  fma32 is exact while nothing leaves the
normal ranges of fp32 and fp64, and the header leaves denormal intermediates unspecified: `assert_condition` states the input
condition under which the replica and the device agree, and the tests call it on their inputs instead of hoping."""
import numpy as np

from frontend_ref import fma32

F32 = np.float32
BIG, SMALL = 2.0**100, 2.0**-100


def decay_at(decay, warmup, t):
    """d as the fp32 value (np.float32)."""
    d = F32(decay)
    if warmup:
        t = F32(t)
        with np.errstate(all='raise'):
            d = min(d, (F32(1) + t) / (F32(10) + t))  # fminf: neither side is NaN here
    return F32(d)


def alpha_at(decay, warmup, t):
    return F32(F32(1) - decay_at(decay, warmup, t))


def update(ema, p, decay, warmup, t):
    """One update of the whole buffer: the new ema (a new float32 array)."""
    ema, p = np.asarray(ema, F32), np.asarray(p, F32)
    a = alpha_at(decay, warmup, t)
    diff = (p - ema).astype(F32)  # an fp32 subtraction of its own, never contracted into the fmaf
    return fma32(np.full(p.shape, a, F32), diff, ema)


def update_rows(ema, p, decay, warmup, t, flags, lo, rows, rowlen):
    """update() with the lazy table: the rows of ema[lo : lo + rows * rowlen] whose flag is 0 are left as they are."""
    out = update(ema, p, decay, warmup, t)
    keep = np.zeros(out.shape, bool)
    keep[lo:lo + rows * rowlen] = np.repeat(np.asarray(flags) == 0, rowlen)
    return np.where(keep, np.asarray(ema, F32), out)


def assert_condition(ema, p, decay, warmup, t):
    """The input condition of the bit-for-bit statement: everything finite with |x| <= 2^100, and every nonzero |p - ema| and
    |a (p - ema)| at least 2^-100 -- no intermediate is denormal in fp32, no fp64 operation of fma32 leaves its exact range."""
    ema, p = np.asarray(ema, F32), np.asarray(p, F32)
    assert np.isfinite(ema).all() and np.isfinite(p).all()
    assert np.abs(ema).max(initial=0) <= BIG and np.abs(p).max(initial=0) <= BIG
    diff = np.abs((p - ema).astype(F32).astype(np.float64))
    a = float(alpha_at(decay, warmup, t))
    for what, v in (('p - ema', diff), ('a (p - ema)', a * diff)):
        nz = v[v != 0]
        assert nz.size == 0 or nz.min() >= SMALL, f'{what}: a nonzero magnitude below 2^-100 ({nz.min()!r})'
    nz = np.abs(ema[ema != 0].astype(np.float64))
    assert nz.size == 0 or nz.min() >= SMALL


def update64(ema, p, decay, warmup, t):
    """The same expression with d and a as the fp32 values but the element arithmetic in fp64 (the yardstick of the 1.5 ulp test)."""
    a = float(alpha_at(decay, warmup, t))
    e, q = np.asarray(ema, F32).astype(np.float64), np.asarray(p, F32).astype(np.float64)
    return e + a * (q - e)


def ulp32(x):
    """The spacing of fp32 at |x| (of the binade |x| lies in)."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0**-126)))
    return 2.0**(e - 23)
