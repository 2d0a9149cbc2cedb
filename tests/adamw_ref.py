"""fp64 reference with a derived error bound for mmvid_adam_step_decoupled (csrc/optim.hip: adam_kernel<true>), torch.optim.AdamW's
rule.  A plain helper like tests/optim_ref.py, from which everything but the formula comes: V (a value and its running error bound, one
rounding charged per fp32 operation, which covers a contracted and an uncontracted compilation alike), the 1-ulp host / 16-ulp device
allowance for the powf of the bias corrections, the inputs and the cases.

What is restated (include/mmvid_hip_ext.h), on the fp32-rounded hyperparameters the C ABI receives:

    coef = grad_scale * min(1, max_norm / (sqrt(sqnorm) * grad_scale + 1e-6))      (clip only if sqnorm is given and max_norm > 0)
    gr   = g * coef ;  m' = b1 m + (1 - b1) gr ;  v' = b2 v + (1 - b2) gr^2
    keep = 1 - lr * wd
    p'   = p * keep - (lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps) ,   bc_i = 1 - b_i^t

adamw_fp32 evaluates the same in fp32 on the CPU, and the two nearest wrong forms: 'l2' is optim_ref.adam_fp32 as it stands (the decay
added to the gradient: what every other Adam entry computes) and 'swapped' applies the decay after the update, (p - update) * keep.
tests/test_adamw_ref_host.py shows that both fall outside the bound on the inputs the GPU test uses."""
import numpy as np
import torch

import optim_ref as R
from optim_ref import V, f32

WDS = (0.0, 0.01, 0.1)


def adamw_ref(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, t, max_norm, sqnorm, grad_scale, pow_ulps):
    """One AdamW step; arguments and result as optim_ref.adam_ref."""
    for h in (lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale):
        assert f32(h) == h, 'hyperparameters must be given as the fp32 values the ABI receives'
    one = V(1.0)
    bc1 = one - R._pow(beta1, t, pow_ulps)
    bc2s = (one - R._pow(beta2, t, pow_ulps)).sqrt()
    coef = V(grad_scale)
    if sqnorm is not None and max_norm > 0.0:
        assert f32(sqnorm) == sqnorm
        c = V(max_norm) / (V(sqnorm).sqrt() * V(grad_scale) + V(f32(1e-6)))
        coef = coef * c.min1()
    step = V(lr) / bc1
    keep = one - V(lr) * V(weight_decay)
    b1, b2, omb1, omb2 = V(beta1), V(beta2), one - V(beta1), one - V(beta2)
    P, G, M, Vv = V(p.double()), V(g.double()), V(m.double()), V(v.double())
    gr = G * coef
    m1 = b1 * M + omb1 * gr
    v1 = b2 * Vv + (omb2 * gr) * gr
    p1 = P * keep - (step * m1) / (v1.sqrt() / bc2s + V(eps))
    return {'p': p1, 'm': m1, 'v': v1}


def adamw_fp32(p, g, m, v, *, fused=False, form='decoupled', **hyper):
    """fp32 on the CPU -> (p', m', v').  form 'decoupled': the rule (optim_ref.adam_fp32 lists it among the wrong forms of the OTHER
    entries and evaluates it correctly); 'l2': the other entries' rule; 'swapped': (p - update) * keep."""
    if form == 'decoupled':
        return R.adam_fp32(p, g, m, v, fused=fused, variant='decoupled_decay', **hyper)
    if form == 'l2':
        return R.adam_fp32(p, g, m, v, fused=fused, **hyper)
    assert form == 'swapped'
    p1, m1, v1 = R.adam_fp32(p, g, m, v, fused=fused, **dict(hyper, weight_decay=f32(0.0)))
    keep = np.float32(1) - np.float32(hyper['lr']) * np.float32(hyper['weight_decay'])
    return p1 * torch.tensor(float(keep), dtype=torch.float32), m1, v1
