"""Host replicas of the learning-rate schedules that run on the device (csrc/optim.hip: mmvid_lr_schedule_ext, mmvid_lr_plateau;
include/mmvid_hip_ext.h states the rules).  A plain helper like tests/optim_ref.py, whose V (value, running error bound) it reuses.

CLOSED FORMS.  ext_ref() follows lr_schedule_ext_kernel operation by operation in fp64 and returns (lr, bound).  Every fp32 product,
sum and quotient of the kernel is charged one rounding (optim_ref.V); the three library functions are charged the accuracy the OpenCL C
specification requires of them, which the ROCm device library is specified to meet -- 3 ulp for log (optim_ref.LOG_ULPS_DEVICE), 4 ulp
for cos, 16 ulp for pow (optim_ref.POW_ULPS_DEVICE) -- NOT what a kernel was seen to deliver.  The cosine's argument x = (PI r) / a
carries |fp32(pi) - pi|, two roundings, and reaches the result through |d cos| <= |dx|.  Integers are below 2^24 (the entry refuses
larger periods and the fp32 step count stops there): their conversion to fp32 is exact.

PLATEAU.  plateau_run() is ReduceLROnPlateau(mode='min', threshold_mode='rel') in the order the header states, in np.float64 (what
torch computes, on Python floats) or np.float32 (what the device computes: multiplies, subtractions and comparisons, each rounded
once, so numpy's fp32 scalars replay it bit for bit).  With `trace` it also records both sides of every comparison it makes, so that a
test can state when the two precisions must agree: when no comparison is closer to a tie than the fp32 rounding of its sides."""
import math

import numpy as np

import optim_ref as R
from optim_ref import V, f32, ulp32

COS_ULPS_DEVICE = 4.0      # OpenCL C accuracy requirement for cos
KIND_STEP, KIND_COSINE, KIND_WARMUP_DECAY = 2, 3, 4
PI32 = f32(math.pi)
MAX_PERIOD = 2**24


def ext_ref(it, kind, lr_min, lr_max, every, a, b=0, gamma=1.0):
    """mmvid_lr_schedule_ext at step count `it` -> (lr, bound).  lr_min, lr_max, gamma: fp32 values.  bound = 0 where the kernel only
    copies lr_max (kind 4 before the first scheduler step)."""
    assert f32(lr_min) == lr_min and f32(lr_max) == lr_max and f32(gamma) == gamma
    assert kind in (2, 3, 4) and every >= 1 and 1 <= a <= MAX_PERIOD and 0 <= it < 2**24
    ns = it // every
    lo, hi, one = V(lr_min), V(lr_max), V(1.0)
    if kind == KIND_STEP:
        pw = float(gamma)**(ns // a)
        lr = hi * V(pw, R.POW_ULPS_DEVICE * ulp32(pw))
    elif kind == KIND_COSINE:
        r = ns % (2 * a)
        x = (V(math.pi, abs(PI32 - math.pi)) * V(float(r))) / V(float(a))
        c = math.cos(float(x.x))
        cos = V(c, float(x.e) + COS_ULPS_DEVICE * ulp32(abs(c) + float(x.e)))
        lr = lo + ((hi - lo) * (one + cos)) * V(0.5)
    else:
        assert a <= b <= MAX_PERIOD
        if ns == 0:
            return lr_max, 0.0
        k, wu = ns - 1, max(a, 2)
        if k < wu:
            l1, l2 = math.log(k + 1), math.log(wu)
            g = V(l1, R.LOG_ULPS_DEVICE * ulp32(l1)) / V(l2, R.LOG_ULPS_DEVICE * ulp32(l2))
        else:
            q = V(float(b - k)) / V(float(max(1, b - wu)))
            g = V(q.x.clamp_min(0.0), q.e)          # fmaxf(0, .): 1-Lipschitz, no rounding
        lr = lo + (hi - lo) * g
    return float(lr.x), float(lr.e)


# ---- ReduceLROnPlateau ------------------------------------------------------------------------------------------------------------------
REFERENCE_PLATEAU = dict(factor=0.5, patience=2, cooldown=5, threshold=1e-4, min_lr=1e-6, eps=1e-8)   # utils_train.py:317-325 + torch's defaults


def plateau_initial(lr):
    """(state_f, state_i) before the first scheduler step: lr, best = +inf; bad, cool-down left, reductions = 0."""
    return [lr, float('inf')], [0, 0, 0]


def plateau_run(losses, *, lr, factor, patience, cooldown, threshold, min_lr, eps, dtype, state=None, trace=None):
    """One scheduler step per entry of `losses`, in `dtype` (np.float64 or np.float32) -> (lr after each step as Python floats,
    final (state_f, state_i)).  trace: a list that receives (lhs, rhs) of every `<` / `>` on floating-point values, as Python floats."""
    f = dtype
    sf, si = state if state is not None else plateau_initial(lr)
    cur, best = f(sf[0]), f(sf[1])
    bad, cool, reductions = (int(x) for x in si)
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for loss in losses:
            loss = f(loss)
            bar = best * (f(1) - f(threshold))
            if trace is not None:
                trace.append((float(loss), float(bar)))
            if loss < bar:                     # (NaN compares false: a bad epoch)
                best, bad = loss, 0
            else:
                bad += 1
            if cool > 0:
                cool, bad = cool - 1, 0
            if bad > patience:
                nw = max(cur * f(factor), f(min_lr))
                if trace is not None:
                    trace.append((float(cur - nw), float(f(eps))))
                if cur - nw > f(eps):
                    cur, reductions = nw, reductions + 1
                cool, bad = cooldown, 0
            out.append(float(cur))
    return out, ([float(cur), float(best)], [bad, cool, reductions])


def plateau_losses():
    """The sequence of the plateau tests: it falls, stalls with noise, holds a NaN and an inf, then stays flat for long enough to
    reach min_lr from 1e-4 at the reference's constants (seven halvings, each after 3 bad epochs and a cool-down of 5)."""
    fall = [4.0 * 0.9**i for i in range(12)]
    rng = np.random.RandomState(7)
    stall = [fall[-1] * (1.0 + 0.02 * float(u)) for u in rng.uniform(-1.0, 1.0, 14)]   # (some of these are new bests)
    flat = 1.03 * min(fall + stall)
    return fall + stall + [float('nan'), flat, float('inf')] + [flat] * 70


def no_near_ties(trace, ulps=4.0):
    """True where no recorded comparison has |lhs - rhs| within `ulps` fp32 roundings of its sides (NaN and inf sides: decided
    alike in every precision)."""
    for lhs, rhs in trace:
        if not (math.isfinite(lhs) and math.isfinite(rhs)):
            continue
        if abs(lhs - rhs) <= ulps * 2.0**-24 * (abs(lhs) + abs(rhs)):
            return False
    return True
