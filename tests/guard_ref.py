"""Host replica of mmvid_step_guard (include/mmvid_hip_ext.h, "Non-finite guard"): the verdict on one step's sum of squared gradients
and the counters it keeps, every floating-point operation one numpy fp32 operation.  A plain helper: no fixtures, no tests."""
import numpy as np

F32 = np.float32
# the values the tests walk through: zero, an ordinary one, the largest power of two fp32 holds, and the two kinds of non-finite
SQS = (F32(0.0), F32(1.0), F32(2.0**127), F32(np.inf), F32(np.nan))


def fresh():
    """(step_dev, guard_i, guard_f) as a trainer allocates them: all zero."""
    return F32(0.0), np.zeros(4, np.int32), np.zeros(2, F32)


def step_guard(sq, grad_scale, step_dev, guard_i, guard_f):
    """One call -> the new (step_dev, guard_i, guard_f); the arguments are left as they are."""
    sq, gs = F32(sq), F32(grad_scale)
    gi, gf = np.array(guard_i, np.int32), np.array(guard_f, F32)
    skip = int(not np.isfinite(sq))
    with np.errstate(invalid='ignore', over='ignore'):
        norm = F32(np.sqrt(sq, dtype=F32) * gs)
    gi[0] = skip
    gi[1] += skip
    gi[2] = gi[2] + 1 if skip else 0
    gi[3] += 1
    gf[0] = norm
    step_dev = F32(step_dev)
    if not skip:
        gf[1] = norm
        step_dev = F32(step_dev + F32(1.0))
    return step_dev, gi, gf


def chain(sqs, grad_scale, state=None):
    """step_guard over a sequence of sums -> the list of states after each call."""
    state = fresh() if state is None else state
    out = []
    for sq in sqs:
        state = step_guard(sq, grad_scale, *state)
        out.append(state)
    return out
