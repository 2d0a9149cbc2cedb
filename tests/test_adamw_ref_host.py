"""tests/adamw_ref.py without a GPU: its fp64 value against torch.optim.AdamW + clip_grad_norm_ run in fp64 over several steps, and
its bound against fp32 evaluations on the inputs of tests/test_adamw_gpu.py -- a correct one (contracted or not) lies inside, the L2
form of the other Adam entries and the swapped order lie outside, so the GPU test can tell them apart."""
import itertools

import pytest
import torch

import adamw_ref as A
import optim_ref as R

F64 = torch.float64


def test_replica_equals_torch_adamw_in_fp64():
    """Six steps of torch.optim.AdamW after clip_grad_norm_(1.0), everything fp64, hyperparameters the fp32-rounded values the ABI
    receives.  The gradients lie on a grid of 2^-8 with |k| <= 64, so the sum of their squares is an integer multiple of 2^-16 below
    2^24 of them: exact in any order and an fp32 value, which is what the kernel's sqnorm argument is.

    THE BAR, from fp64 rounding only.  Per step and element either side makes fewer than 32 roundings of 2^-53 relative (the replica: 10
    elementwise operations and about as many for the scalars; torch: the same formula in another order), and 1 - b^t magnifies the
    rounding of b^t by b^t / (1 - b^t) <= 9 (b1 = 0.9) and 19 (b2 = 0.95) at t = 1: K = 2 * 32 + 2 * (9 + 19) = 120 roundings per
    step, charged against |p| + |update| and summed over the steps (moments carry their error on, first order).  One constant
    differs by design: the kernel adds the fp32 value of 1e-6 to the norm, torch the fp64 one; |f32(1e-6) - 1e-6| / norm enters the
    clip coefficient and with it the update."""
    n, steps = 512, 6
    gen = torch.Generator().manual_seed(11)
    lr, b1, b2, eps, wd, mx = (R.f32(x) for x in (1e-3, 0.9, 0.95, 1e-8, 0.01, 1.0))
    p0 = torch.randn(n, generator=gen, dtype=F64) * 0.05
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    bar, m_mag = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for t in range(1, steps + 1):
        g = torch.randint(-64, 65, (n,), generator=gen).double() * 2.0**-8
        if t % 2 == 0:
            g = g / 64                                      # (every other step the norm is below 1: no clipping)
        sq = float((g * g).sum())
        assert R.f32(sq) == sq and (sq > 1.0) == (t % 2 == 1)
        w.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([w], mx)
        opt.step()
        ref = A.adamw_ref(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, t=t, max_norm=mx, sqnorm=sq, grad_scale=1.0,
                          pow_ulps=R.POW_ULPS_HOST)
        update = (ref['p'].x - p * (1.0 - lr * wd)).abs()
        bar += (120 * 2.0**-53 + abs(R.f32(1e-6) - 1e-6) / sq**0.5) * (p.abs() + update)
        p, m, v = ref['p'].x, ref['m'].x, ref['v'].x
        st = opt.state[w]
        worst = ((w.detach() - p).abs() / bar).max().item()
        print(f'step {t}: p is {worst:.3f} x the fp64 bar from torch.optim.AdamW')
        assert worst <= 1.0
        # the moments: v is a sum of non-negative terms; m may cancel, so its error is charged against the sum of its terms' magnitudes
        m_mag = b1 * m_mag + (1.0 - b1) * g.abs() * min(1.0, mx / sq**0.5)
        rel = t * (120 * 2.0**-53 + abs(R.f32(1e-6) - 1e-6) / sq**0.5)
        assert ((st['exp_avg'] - m).abs() <= rel * m_mag).all() and ((st['exp_avg_sq'] - v).abs() <= 2 * rel * v).all()
    assert float((p - p0).abs().max()) > 1e-3  # the weights moved


CASES = [dict(t=t, step_dev=dev, lr_dev=dev, wd=wd, clip=clip, gs=1.0)
         for t, dev, wd, clip in itertools.product((1, 2, 10, 1000), (False, True), A.WDS[1:], R.CLIPS)]


def swap_is_resolved(case):
    """Can the bound tell (p - update) * keep from p * keep - update?  The two differ by lr * wd of the update.  The bound on the update
    holds, relative to it, the allowance for the two powers -- ulps 2^-24-spacings of b^t magnified by 1 / (1 - b^t), halved for b2 by
    the square root -- and its own roundings (fewer than 8).  Where lr * wd exceeds twice that, the swapped form must lie outside; where
    it does not (b2^t near 1: the first steps, above all with the 16-ulp device power) no bound that honours the allowance can
    resolve it, and the test of those cases rests on the L2 form alone."""
    h = case['hyper']

    def pow_term(b):
        x = b**h['t']
        return case['pow_ulps'] * R.ulp32(x) / (1.0 - x)

    return h['lr'] * h['weight_decay'] > 2.0 * (pow_term(h['beta1']) + 0.5 * pow_term(h['beta2']) + 8 * 2.0**-24)


def test_bound_holds_correct_fp32_and_excludes_the_two_wrong_forms():
    """On optim_ref.adam_inputs(1025), the inputs of the GPU test, for every case with weight decay and with the allowance for the
    power that the GPU test grants the case: a correct fp32 evaluation, contracted or not, lies inside the bound of p, m and v; the L2
    form lies outside the bound of p in EVERY case; the swapped order lies outside it in every case that swap_is_resolved names, and
    those include every weight decay, the host and the device step count, and every clip form."""
    x = R.adam_inputs(1025)
    least = {'l2': float('inf'), 'swapped': float('inf')}
    most, resolved = 0.0, set()
    for kw in CASES:
        case = R.adam_case(**kw)
        ref = A.adamw_ref(*x, pow_ulps=case['pow_ulps'], **case['hyper'])
        for fused in (False, True):
            got = A.adamw_fp32(*x, fused=fused, **case['hyper'])
            for k, t in zip('pmv', got):
                fr = R.worst_fraction(t, ref[k])
                most = max(most, fr)
                assert fr <= 1.0, f'{case["tag"]} fused={fused}: a correct fp32 {k} is {fr:.3f} x the bound away'
        for form in least:
            if form == 'swapped' and not swap_is_resolved(case):
                continue
            got = A.adamw_fp32(*x, form=form, **case['hyper'])
            fr = R.worst_fraction(got[0], ref['p'])
            least[form] = min(least[form], fr)
            assert fr > 1.0, f'{case["tag"]}: the {form} form stays within the bound of p ({fr:.3f} x): the GPU test could not tell it apart'
            if form == 'swapped':
                resolved.add((kw['step_dev'], kw['wd'], kw['clip']))
    assert resolved == set(itertools.product((False, True), A.WDS[1:], R.CLIPS))
    print(f'correct fp32: at most {most:.3f} x the bound; wrong forms: at least ' + ', '.join(f'{k} {x:.1f} x' for k, x in least.items()))


def test_without_decay_the_three_forms_coincide():
    """wd = 0: keep = 1 exactly and the L2 term is 0 * p -- nothing is left to tell apart, which is why the GPU test demands the
    bytes of mmvid_adam_step_guarded there."""
    x = R.adam_inputs(1025)
    hyper = R.adam_case(t=10, step_dev=False, lr_dev=False, wd=0.0, clip='clip', gs=0.125)['hyper']
    want = A.adamw_fp32(*x, **hyper)
    for form in ('l2', 'swapped'):
        for a, b in zip(want, A.adamw_fp32(*x, form=form, **hyper)):
            assert torch.equal(a, b)
