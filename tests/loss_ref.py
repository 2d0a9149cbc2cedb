"""fp64 references, each with a derived error bound, for the loss kernels: the MSM cross entropy of csrc/embed.hip (ce_fwd_kernel,
ce_bwd_kernel) and the REL / VID heads of csrc/sample.hip (head_bce_fwd_kernel, head_bce_bwd_kernel).  A plain helper like
tests/optim_ref.py (no fixtures, no pytest settings); its own tests are tests/test_loss_ref_host.py and run without a GPU,
tests/test_loss_exact_gpu.py holds the kernels to it.

THE BOUND is the running error of tests/optim_ref.py (its docstring has the rules): a value is a pair (x, e), x in fp64 and
e >= |any correct fp32 evaluation - x|, pushed through the kernel's own sequence of operations; every fp32 operation propagates the
errors of its operands and adds one rounding U (|x| + e) + ETA.  Added here, with the same rules:

* vexp, vlog, vlog1p, vrsqrt: the propagated error is the larger one-sided deviation of the function over [x - e, x + e]; the
  function's own error is an allowance in ulp of the result (an ulp: the spacing of fp32 at the largest magnitude the result can have).
* vabs, vmax0, vmaxc: 1-Lipschitz, exact.
* vsum(a, axis, depth): a sum of fp32 terms in ANY tree in which no term passes through more than `depth` additions is within
  ((1 + U)^depth - 1) sum (|x_i| + e_i) of the sum of the terms (Higham, section 4.2).  The depths are counted from the kernels:
      ce_fwd     2 ((a + b) + (c + d) of a float4) + ceil(V / 256) (s += ..., once per sweep of the wave over the row) + 6 (wave_sum)
      heads      2 (the float4) + 4 (HEAD_MAXV trips of `+=`) + 6 (wave_sum) = 12 for every sum over E
                 R for the loss (thread 0, one chain), nden for den_from (one chain)
                 ceil(R / 4) (a wave's `+=` over its rows r = wave, wave + 4, ...) + 2 ((red0 + red1) + (red2 + red3)) for dw, db,
                 dln_w, dln_b
* vbf16: one bf16 rounding, half a bf16 spacing (8 significant bits: at most 2^-8 relative) taken at |x| + e, the largest magnitude the
  fp32 value can have, so that an fp32 error which carries the value into the next binade is covered; plus ETA, the same absolute
  floor as fp32 (bf16 has fp32's exponent range, and a result below 2^-126 may be flushed).

TRANSCENDENTAL ALLOWANCES.  The heads call expf, log1pf and rsqrtf, the precise device-library functions: the OpenCL C accuracy
requirements, 3, 2 and 2 ulp, which the ROCm device library is specified to meet (as optim_ref.LOG_ULPS_DEVICE; NOT taken from
observing the kernels).  The cross-entropy kernels call __expf and __logf.  In the HIP headers (__clang_hip_math.h)

    __expf(x) = __builtin_amdgcn_exp2f(0x1.715476p+0f * x)         one fp32 product around the hardware exp2 (v_exp_f32)
    __logf(x) = __builtin_logf(x)                                  the compiler's logf: hardware log2 times ln 2, refined or not

* __expf: the constant is log2 e rounded to fp32 (LOG2E_REL off) and the product rounds once, so the exponent moves by at most
  |x| (LOG2E_REL + U): a relative error of that size in the result, the (|d| + c) form of tests/truncate_ref.py.  v_exp_f32 itself:
  the CDNA ISA manual gives 1 ulp.  That figure cannot be verified without the hardware, so it is charged at NATIVE_ULPS = 4: the
  manual's figure with a factor of four in hand.  A result below 2^-126 is flushed by the instruction: ETA.
* __logf: charged as the looser of (a) the native form, hardware log2 at NATIVE_ULPS ulp of log2 x, times fp32 ln 2 (LN2_REL off), one
  rounding; (b) the precise logf at LOG_ULPS_DEVICE.  (a) is never below 3.27 ulp of the result, so it is the one that counts; the
  refined expansion the compiler chooses for __builtin_logf without fast-math flags (v_log_f32, then the product by ln 2 carried in
  two words) lies inside it.
The factor of four is harmless because tests/test_loss_ref_host.py shows every listed wrong variant more than 10 x outside a bound
with the factor in place.

WHAT IS RESTATED (include/mmvid_hip.h; F.cross_entropy and F.binary_cross_entropy_with_logits of the reference model):

    lse_r = mx + log sum_c exp(v_rc - mx), mx = max_c v_rc exactly;   term_r = lse_r - v_r,t(r);   loss_sum += term_r
    dlogits_rc = bf16((exp(v_rc - lse_r) - [c == t(r)]) * gscale)     on selected rows, exactly 0 on the others
    z_r = LN(x[rows[r]]) . w + b,  LN two-pass: mean, then var = mean((x - mean)^2), rstd = rsqrt(var + eps)
    loss = sum_r rw_r (max(z_r, 0) - z_r y_r + log1p(exp(-|z_r|))) / den,   den = den_from ? max(1, sum den_from) : den_const
    dz_r = gloss / den * rw_r * (1 / (1 + exp(-z_r)) - y_r);  dw += sum_r dz_r LN(x)_r;  db += sum_r dz_r;  dln_w += sum_r dz_r w xhat_r;
    dln_b += sum_r dz_r w;  dx[rows[r]] += rstd_r (g - mean(g) - xhat_r mean(g xhat_r)),  g = dz_r w ln_w

The backward references take the fp32 lse / z, mean, rstd handed to the backward as EXACT inputs: the backward is tested on what it
is given, not on the forward's error."""
import itertools
import math

import torch

from guarded import BAD_ID, seeded
from optim_ref import ETA, LOG_ULPS_DEVICE, U, V, f32, worst_fraction  # noqa: F401  (worst_fraction: re-exported for the tests)

F64, F32 = torch.float64, torch.float32
NAN = float('nan')
EXP_ULPS_DEVICE = 3.0      # OpenCL C accuracy requirement for exp
LOG1P_ULPS_DEVICE = 2.0    # ... for log1p
RSQRT_ULPS_DEVICE = 2.0    # ... for rsqrt
NATIVE_ULPS = 4.0          # v_exp_f32 / v_log_f32: 1 ulp in the CDNA ISA manual, charged four times (see above)
LOG2E_F32 = float.fromhex('0x1.715476p+0')
LN2_F32 = float.fromhex('0x1.62e430p-1')
LOG2E_REL = abs(LOG2E_F32 * math.log(2.0) - 1.0)
LN2_REL = abs(LN2_F32 / math.log(2.0) - 1.0)
HEAD_MAXV = 4              # csrc/sample.hip: float4 per lane
HEAD_DEPTH = 2 + HEAD_MAXV + 6


def ce_depth(nv):
    return 2 + -(-nv // 256) + 6


def head_rows_depth(R):
    return -(-R // 4) + 2


# ---- (x, e) operations on top of optim_ref.V -------------------------------------------------------------------------------------------
def _pow2_of(x, shift):
    """2^(exponent of |x| + shift) with |x| = m 2^exponent, m in [0.5, 1); 2^-149 for x == 0."""
    ex = torch.frexp(x.abs())[1].to(F64)
    return torch.where(x == 0, torch.full_like(x, 2.0**-149), torch.exp2(ex + shift).clamp_min(2.0**-149))


def ulp32(x):
    """Spacing of fp32 at |x| (fp64 tensor)."""
    return _pow2_of(x, -24)


def half_spacing_bf16(x):
    """Half the spacing of bf16 (8 significant bits) at |x|: at most 2^-8 |x|."""
    return _pow2_of(x, -9)


def col(a):
    """[R] -> [R, 1]."""
    return V(a.x[:, None], a.e.expand_as(a.x)[:, None])


def vneg(a):
    return V(-a.x, a.e)


def vabs(a):
    return V(a.x.abs(), a.e)


def vmaxc(a, c):
    """max(a, c) with an exact c: 1-Lipschitz, no rounding."""
    return V(a.x.clamp_min(c), a.e)


def vmax0(a):
    return vmaxc(a, 0.0)


def vexp(a, ulps, native=False):
    r = a.x.exp()
    shift = a.e
    if native:
        shift = shift + (a.x.abs() + a.e) * (LOG2E_REL + U)
    prop = r * torch.expm1(shift)
    return V(r, prop + ulps * ulp32(r + prop) + ETA)


def vlog(a):
    """__logf: the looser of the native form and the precise function (module docstring)."""
    assert bool((a.x > a.e).all()), 'the argument of a logarithm is not bounded away from zero'
    r = a.x.log()
    prop = -torch.log1p(-a.e / a.x)
    mag = r.abs() + prop
    fn = torch.maximum(LOG_ULPS_DEVICE * ulp32(mag), math.log(2.0) * NATIVE_ULPS * ulp32(mag / math.log(2.0)) + mag * (LN2_REL + U))
    return V(r, prop + fn + ETA)


def vlog1p(a, ulps):
    assert bool((a.x - a.e > -1).all())
    r = torch.log1p(a.x)
    prop = -torch.log1p(-a.e / (1.0 + a.x))
    return V(r, prop + ulps * ulp32(r.abs() + prop) + ETA)


def vrsqrt(a, ulps):
    assert bool((a.x > a.e).all()), 'the argument of rsqrt is not bounded away from zero'
    r = a.x.rsqrt()
    prop = (a.x - a.e).rsqrt() - r
    return V(r, prop + ulps * ulp32(r + prop) + ETA)


def vsum(a, axis, depth):
    e = a.e.expand_as(a.x)
    mag = (a.x.abs() + e).sum(axis)
    return V(a.x.sum(axis), e.sum(axis) + ((1.0 + U)**depth - 1.0) * mag + depth * ETA)


def vbf16(a):
    return V(a.x, a.e + half_spacing_bf16(a.x.abs() + a.e) + ETA)


def vwhere(c, a, b):
    return V(torch.where(c, a.x, b.x), torch.where(c, a.e, b.e))


def vsigmoid(z):
    """1 / (1 + expf(-z)).  Where exp(-z) is beyond 2^126 its fp32 value may be anything up to infinity; the quotient is then in
    [0, 2^-125], and so is the exact one."""
    t = vexp(vneg(z), EXP_ULPS_DEVICE)
    big = t.x > 2.0**126
    s = V(1.0) / (V(1.0) + vwhere(big, V(torch.ones_like(t.x)), t))
    return vwhere(big, V(1.0 / (1.0 + t.x), torch.full_like(t.x, 2.0**-125)), s)


def select_rows(select, rows):
    return torch.arange(rows) if select is None else (select != 0).nonzero().view(-1)


# ---- cross entropy -----------------------------------------------------------------------------------------------------------------------
def ce_fwd_ref(logits, target, select):
    """-> (on, lse, term): the selected rows' indices and, for those rows, V pairs following ce_fwd_kernel line by line."""
    on = select_rows(select, logits.shape[0])
    x, t = logits[on].double(), target[on]
    mx = x.max(1, keepdim=True).values
    p = vexp(V(x) - V(mx), NATIVE_ULPS, native=True)
    s = vsum(p, 1, ce_depth(logits.shape[1]))
    lse = V(mx[:, 0]) + vlog(s)
    term = lse - V(x.gather(1, t[:, None])[:, 0])
    return on, lse, term


def ce_loss_sum_ref(loss0, terms32):
    """loss_sum after the call: loss0 plus the device's own fp32 terms, one atomic each in a free order: K 2^-23 sum |terms| with
    K = number of terms + 1, as tests/test_abi_contract_gpu.py holds it."""
    t = terms32.double()
    return V(torch.tensor([loss0 + float(t.sum())]), torch.tensor([(t.numel() + 1) * 2.0**-23 * (abs(loss0) + float(t.abs().sum())) + ETA]))


def ce_bwd_ref(logits, target, select, lse32, gscale32):
    """-> (on, d): V pair [len(on), V] of the bf16 gradient rows, following ce_bwd_kernel.  lse32 [rows] fp32 and gscale32 (an fp32
    value) are exact inputs."""
    assert f32(gscale32) == gscale32 and lse32.dtype == F32
    on = select_rows(select, logits.shape[0])
    x, t = logits[on].double(), target[on]
    p = vexp(V(x) - V(lse32[on].double()[:, None]), NATIVE_ULPS, native=True)
    hot = torch.zeros_like(x, dtype=torch.bool)
    hot[torch.arange(len(on)), t] = True
    o = vwhere(hot, p - V(1.0), p)
    return on, vbf16(o * V(gscale32))


# ---- heads -------------------------------------------------------------------------------------------------------------------------------
def _den_ref(den_from, den_const):
    if den_from is None:
        assert f32(den_const) == den_const
        return V(den_const)
    return vmaxc(vsum(V(den_from.double()), 0, den_from.numel()), 1.0)


def _ones_if_none(rw, R):
    return torch.ones(R, dtype=F64) if rw is None else rw.double()


def head_fwd_ref(x, rows, ln_w, ln_b, eps, w, b, label, rw, den_from, den_const):
    """-> dict of V: z, mean, rstd [R] and loss [1], following head_bce_fwd_kernel."""
    assert f32(eps) == eps
    R, E = rows.numel(), x.shape[1]
    X = V(x[rows].double())
    mean = vsum(X, 1, HEAD_DEPTH) / V(float(E))
    a = X - col(mean)
    rstd = vrsqrt(vsum(a * a, 1, HEAD_DEPTH) / V(float(E)) + V(eps), RSQRT_ULPS_DEVICE)
    y = ((a * col(rstd)) * V(ln_w.double()) + V(ln_b.double())) * V(w.double())
    z = vsum(y, 1, HEAD_DEPTH) + V(b.double())
    l = (vmax0(z) - z * V(label.double())) + vlog1p(vexp(vneg(vabs(z)), EXP_ULPS_DEVICE), LOG1P_ULPS_DEVICE)
    s = vsum(l * V(_ones_if_none(rw, R)), 0, R) / _den_ref(den_from, den_const)
    return dict(z=z, mean=mean, rstd=rstd, loss=V(s.x.view(1), s.e.view(1)))


def head_bwd_ref(x, rows, ln_w, ln_b, w, z32, mean32, rstd32, label, rw, den_from, den_const, gloss):
    """-> dict of V: the CONTRIBUTIONS dx [R, E] (to dx[rows]), dw, dln_w, dln_b [E], db [1], following head_bce_bwd_kernel from the saved
    fp32 z, mean, rstd as exact inputs.  What the call leaves in a buffer that held `a` is accumulate(a, contribution)."""
    R, E = rows.numel(), x.shape[1]
    lw, wv = V(ln_w.double()), V(w.double())
    dz = ((V(gloss.double()) / _den_ref(den_from, den_const)) * V(_ones_if_none(rw, R))) * (vsigmoid(V(z32.double())) - V(label.double()))
    rs = col(V(rstd32.double()))
    xh = (V(x[rows].double()) - col(V(mean32.double()))) * rs
    dh = col(dz) * wv
    K = head_rows_depth(R)
    db = vsum(dz, 0, K)
    g = dh * lw
    m1 = vsum(g, 1, HEAD_DEPTH) / V(float(E))
    m2 = vsum(g * xh, 1, HEAD_DEPTH) / V(float(E))
    return dict(dx=rs * ((g - col(m1)) - xh * col(m2)), dw=vsum(col(dz) * (xh * lw + V(ln_b.double())), 0, K),
                dln_w=vsum(dh * xh, 0, K), dln_b=vsum(dh, 0, K), db=V(db.x.view(1), db.e.view(1)))


def accumulate(base, contribution):
    """fl(base + contribution): one more rounding."""
    return V(base.double()) + contribution


# ---- fp32 evaluation on the CPU: what a correct kernel may compute, and the listed WRONG variants ---------------------------------------
ORDERS = ('sequential', 'pairwise')
CE_WRONG = ('drop_p_below_1e-3', 'onehot_only', 'onehot_at_t_plus_1', 'onehot_at_t_and_not_3', 'gscale_not_on_onehot',
            'partial_sweep_skipped', 'lse_without_max', 'lse_in_log2')
HEAD_WRONG = ('no_mean_g_term', 'no_xhat_term', 'row_weight_ignored_in_bwd', 'den_without_max1', 'den_const_despite_den_from',
              'bce_without_max_z_0', 'label_minus_sigmoid', 'dln_b_times_ln_w', 'variance_over_E_minus_1', 'eps_outside_rsqrt',
              'assign_dw', 'assign_db', 'assign_dln_w', 'assign_dln_b', 'assign_dx')
WRONG_VARIANTS = CE_WRONG + HEAD_WRONG


class Fp32:
    """fp32 arithmetic with a choice of summation order and of contraction (fused: a * b + c rounds once; through fp64, where the
    product of two fp32 values is exact).  Both orders are trees no deeper than the depth the bound charges:
      sequential   the kernels' own chains in their own order.  kind 'lanes' (a sum over V or E): float4 c belongs to lane c % 64, a lane
                   adds (a + b) + (c + d) of its float4s one after the other, then the xor butterfly 32 ... 1; 'waves' (a sum over the
                   rows): wave r % 4 chains its rows, then (w0 + w1) + (w2 + w3); 'chain': one chain.
      pairwise     neighbours first: ceil(log2 n) levels.
    (ONE chain over all V or E terms has depth n - 1: no kernel here sums that way, and the bound is not derived for it.)"""

    def __init__(self, order, fused):
        assert order in ORDERS
        self.order, self.fused = order, fused

    def muladd(self, a, b, c):
        if self.fused:
            return (a.double() * b.double() + c.double()).float()
        return a * b + c

    @staticmethod
    def _pad(t, multiple):
        n = -(-t.shape[0] // multiple) * multiple
        return torch.cat([t, t.new_zeros((n - t.shape[0],) + t.shape[1:])])

    @staticmethod
    def _chain(t, step):
        s = torch.zeros_like(t[0])
        for i in range(t.shape[0]):
            s = step(s, i)
        return s

    def _lanes(self, t, group):
        """t [n, ...]: `group` consecutive elements are what is left of one float4."""
        t = self._pad(t, 64 * group)
        t = t.reshape((-1, 64, group) + t.shape[1:])
        t = (t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3]) if group == 4 else t[:, :, 0] + t[:, :, 1]
        w = self._chain(t, lambda s, i: s + t[i])
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[lane ^ o]
        return w[0]

    def _pairwise(self, t):
        t = self._pad(t, 1 << max(t.shape[0] - 1, 0).bit_length())
        while t.shape[0] > 1:
            t = t[0::2] + t[1::2]
        return t[0]

    def sum(self, t, axis, kind='lanes'):
        t = t.movedim(axis, 0)
        if self.order == 'pairwise':
            return self._pairwise(t)
        if kind == 'lanes':
            return self._lanes(t, 4)
        if kind == 'chain':
            return self._chain(t, lambda s, i: s + t[i])
        t = self._pad(t, 4)
        t = t.reshape((-1, 4) + t.shape[1:])
        w = self._chain(t, lambda s, i: s + t[i])
        return (w[0] + w[1]) + (w[2] + w[3])

    def sum_prod(self, a, b, axis, kind='lanes'):
        """sum of a * b.  Contracted: along E every second product is fused into the addition of its neighbour, along the rows every
        product into the chain."""
        if not self.fused:
            return self.sum(a * b, axis, kind)
        a, b = a.movedim(axis, 0), b.movedim(axis, 0)
        if kind == 'lanes' or self.order == 'pairwise':
            a, b = self._pad(a, 4), self._pad(b, 4)
            t = self.muladd(a[0::2], b[0::2], a[1::2] * b[1::2])
            return self._pairwise(t) if self.order == 'pairwise' else self._lanes(t, 2)
        a, b = self._pad(a, 4), self._pad(b, 4)
        a, b = a.reshape((-1, 4) + a.shape[1:]), b.reshape((-1, 4) + b.shape[1:])
        w = self._chain(a, lambda s, i: self.muladd(a[i], b[i], s))
        return (w[0] + w[1]) + (w[2] + w[3])


def _swept(nv, variant):
    """Columns a row's sweeps cover: all, or without the last partial sweep of 64 float4."""
    if variant != 'partial_sweep_skipped':
        return nv
    return (nv // 4) // 64 * 64 * 4


def ce_fwd_fp32(logits, target, select, order='pairwise', fused=False, variant=None):
    """-> (lse fp32 [rows] with 0 at unselected rows, term fp32 [len(on)]).  (The kernel has no multiply-add: `fused` changes nothing.)"""
    k = Fp32(order, fused)
    on = select_rows(select, logits.shape[0])
    nv = _swept(logits.shape[1], variant)
    x, t = logits[on], target[on]
    xs = x[:, :nv]
    mx = xs.max(1, keepdim=True).values if nv else torch.full((len(on), 1), -math.inf)
    if variant == 'lse_without_max':
        mx = torch.zeros_like(mx)
    s = k.sum(torch.exp(xs - mx), 1) if nv else torch.zeros(len(on))
    l = mx[:, 0] + (torch.log2(s) if variant == 'lse_in_log2' else torch.log(s))
    lse = torch.zeros(logits.shape[0])
    lse[on] = l
    return lse, l - x.gather(1, t[:, None])[:, 0]


def ce_bwd_fp32(logits, target, select, lse32, gscale32, order='pairwise', fused=False, variant=None):
    """-> bf16 [rows, V]."""
    on = select_rows(select, logits.shape[0])
    x, t = logits[on], target[on]
    gs = torch.tensor(gscale32, dtype=F32)
    p = torch.exp(x - lse32[on][:, None])
    if variant == 'drop_p_below_1e-3':
        p = torch.where(p < 1e-3, torch.zeros(()), p)
    if variant == 'onehot_only':
        p = torch.zeros_like(p)
    if variant == 'onehot_at_t_plus_1':
        t = t + 1
    if variant == 'onehot_at_t_and_not_3':
        t = t & ~3
    hot = torch.zeros_like(x)
    ok = t < x.shape[1]
    hot[torch.arange(len(on))[ok], t[ok]] = 1
    o = p * gs - hot if variant == 'gscale_not_on_onehot' else (p - hot) * gs
    o[:, _swept(x.shape[1], variant):] = 0
    d = torch.zeros(logits.shape, dtype=torch.bfloat16)
    d[on] = o.bfloat16()
    return d


def _den_fp32(k, den_from, den_const, variant):
    if den_from is None or variant == 'den_const_despite_den_from':
        return torch.tensor(den_const, dtype=F32)
    s = k.sum(den_from, 0, 'chain')
    return s if variant == 'den_without_max1' else s.clamp_min(1.0)


def head_fwd_fp32(x, rows, ln_w, ln_b, eps, w, b, label, rw, den_from, den_const, order='pairwise', fused=False, variant=None):
    """-> dict of fp32: z, mean, rstd [R], loss [1]."""
    k = Fp32(order, fused)
    R, E = rows.numel(), x.shape[1]
    X = x[rows]
    nE, e32 = torch.tensor(float(E), dtype=F32), torch.tensor(eps, dtype=F32)
    mean = k.sum(X, 1) / nE
    a = X - mean[:, None]
    q = k.sum_prod(a, a, 1)
    var = q / (nE - 1 if variant == 'variance_over_E_minus_1' else nE)
    rstd = torch.rsqrt(var) + e32 if variant == 'eps_outside_rsqrt' else torch.rsqrt(var + e32)
    y = k.muladd(a * rstd[:, None], ln_w, ln_b)
    z = k.sum_prod(y, w.expand_as(y), 1) + b
    if variant == 'bce_without_max_z_0':
        l = k.muladd(-z, label, z) + torch.log1p(torch.exp(-z))
    else:
        l = k.muladd(-z, label, z.clamp_min(0)) + torch.log1p(torch.exp(-z.abs()))
    if rw is not None:
        l = l * rw
    return dict(z=z, mean=mean, rstd=rstd, loss=(k.sum(l, 0, 'chain') / _den_fp32(k, den_from, den_const, variant)).view(1))


def head_bwd_fp32(x, rows, ln_w, ln_b, w, z32, mean32, rstd32, label, rw, den_from, den_const, gloss, bases=None, order='pairwise',
                  fused=False, variant=None):
    """bases: None (zero bases) or dict dx [R, E] (the named rows of dx), dw, dln_w, dln_b [E], db [1] -> dict of fp32 results: what the
    buffers hold after the call."""
    k = Fp32(order, fused)
    R, E = rows.numel(), x.shape[1]
    nE = torch.tensor(float(E), dtype=F32)
    scale = gloss[0] / _den_fp32(k, den_from, den_const, variant)
    sig = 1.0 / (1.0 + torch.exp(-z32))
    diff = label - sig if variant == 'label_minus_sigmoid' else sig - label
    dz = (scale * (rw if rw is not None and variant != 'row_weight_ignored_in_bwd' else torch.ones(R))) * diff
    assert dz.dtype == F32
    rs = rstd32[:, None]
    xh = (x[rows] - mean32[:, None]) * rs
    dh = dz[:, None] * w
    g = dh * ln_w
    con = dict(dw=k.sum_prod(dz[:, None].expand_as(xh), k.muladd(xh, ln_w, ln_b), 0, 'waves'), dln_w=k.sum_prod(dh, xh, 0, 'waves'),
               dln_b=k.sum(g if variant == 'dln_b_times_ln_w' else dh, 0, 'waves'), db=k.sum(dz, 0, 'waves').view(1))
    m1 = k.sum(g, 1) / nE
    m2 = k.sum_prod(g, xh, 1) / nE
    if variant == 'no_mean_g_term':
        m1 = torch.zeros_like(m1)
    if variant == 'no_xhat_term':
        m2 = torch.zeros_like(m2)
    inner = k.muladd(-xh, m2[:, None], g - m1[:, None])
    out = {}
    for name in ('dw', 'dln_w', 'dln_b', 'db'):
        out[name] = con[name] if bases is None or variant == 'assign_' + name else bases[name] + con[name]
    out['dx'] = rs * inner if bases is None or variant == 'assign_dx' else k.muladd(rs.expand_as(inner), inner, bases['dx'])
    return out


# ---- the cases (CPU and GPU tests use the same) ------------------------------------------------------------------------------------------
CE_SIZES = (4, 252, 256, 260, 1000, 1024)
CE_ROWS = (1, 5, 37)
CE_FAMILIES = ('randn3', 'flat', 'randn30', 'shifted', 'target_up_40', 'target_down_40')
GSCALES = ('1/count', 0.37, -2.0, 0.0)


def ce_cases():
    """(family, rows, V, with_select): every V and row count on 3 * randn; every family at V = 256 and 1000."""
    out = []
    for nv, rows in itertools.product(CE_SIZES, CE_ROWS):
        out += [('randn3', rows, nv, False)] + ([('randn3', rows, nv, True)] if rows > 1 else [])
    for fam, nv, sel in itertools.product(CE_FAMILIES[1:], (256, 1000), (False, True)):
        out.append((fam, 37, nv, sel))
    return out


def ce_inputs(family, rows, nv, with_select):
    """-> dict: logits fp32 [rows, V] (NaN in unselected rows), target int64 (out of range in unselected rows; 0, 3, 4, V - 1 in the
    first selected rows: the float4 boundaries of the one-hot compare), select uint8 or None, lse32 (the fp64 lse rounded to fp32, 0 at
    unselected rows), gscales (fp32 values)."""
    g = seeded('loss-ce', family, rows, nv, with_select)
    scale = {'flat': 0.01, 'randn30': 30.0}.get(family, 3.0)
    logits = (torch.randn(rows, nv, generator=g, dtype=F64) * scale).float()
    target = torch.randint(0, nv, (rows,), generator=g)
    sel = torch.ones(rows, dtype=torch.uint8)
    if with_select:
        sel = (torch.rand(rows, generator=g) < 0.6).to(torch.uint8)
        sel[0], sel[-1] = 1, 0
    on = (sel != 0).nonzero().view(-1)
    edge = [t for t in (0, 3, 4, nv - 1) if t < nv]
    target[on[:len(edge)]] = torch.tensor(edge[:len(on)])
    ar = torch.arange(rows)
    if family == 'shifted':
        logits = (logits.double() + torch.where(ar % 2 == 0, 3e4, -3e4)[:, None]).float()
    if family == 'target_up_40':
        logits[ar, target] += 40
    if family == 'target_down_40':
        logits[ar, target] -= 40
    lse32 = torch.logsumexp(logits.double(), 1).float()
    off = sel == 0
    logits[off], target[off], lse32[off] = NAN, BAD_ID, 0.0
    return dict(tag=f'{family} {rows}x{nv} select={with_select}', family=family, logits=logits, target=target,
                select=sel if with_select else None, lse32=lse32, gscales=[f32(1.0 / len(on)) if s == '1/count' else f32(s) for s in GSCALES])


HEAD_SIZES = (4, 200, 256, 260, 768, 1024)
HEAD_ROWS = (1, 3, 4, 5, 9, 256)       # 256 only at E = 768
HEAD_OPTIONS = tuple(itertools.product((False, True), (None, 5.0, 0.25), (0.0, 30.0, -100.0), (0.0, 1000.0)))
HEAD_EPS, HEAD_DEN_CONST = f32(1e-5), f32(4.0)


def head_cases():
    """(E, R, with_row_weight, den_sum, z_shift, x_mean): every (E, R) with the 36 option tuples dealt round, and all 36 at the model's
    width with R = 9."""
    shapes = [(E, R) for E in HEAD_SIZES for R in HEAD_ROWS if R != 256 or E == 768]
    out = [(E, R) + HEAD_OPTIONS[(7 * i) % len(HEAD_OPTIONS)] for i, (E, R) in enumerate(shapes)]
    out += [(768, 9) + o for o in HEAD_OPTIONS if (768, 9) + o not in out]
    return out


def head_inputs(E, R, with_rw, den_sum, z_shift, x_mean):
    """-> dict.  x [T, E] is NaN outside the R named rows (T = 40; 300 for R = 256); row_weight has zeros; den_from sums to den_sum;
    b is shifted so that z lies near z_shift; dx0 and the four accumulator bases are randn."""
    g = seeded('loss-head', E, R, with_rw, den_sum, z_shift, x_mean)
    T = 300 if R > 40 else 40
    rows = torch.randperm(T, generator=g)[:R].sort().values

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=F64)

    x = torch.full((T, E), NAN)
    x[rows] = (rn(R, E) + x_mean).float()
    ln_w, ln_b, w = (rn(E) * 0.1 + 1).float(), (rn(E) * 0.1).float(), (rn(E) * 0.05).float()
    b = (rn(1) + z_shift).float()
    label = (torch.rand(R, generator=g) < 0.5).float()
    rw = None
    if with_rw:
        rw = torch.rand(R, generator=g)
        rw[1::3] = 0
    den = None
    if den_sum is not None:
        den = torch.tensor([0.6, 0.0, 0.4]) * den_sum
        assert abs(float(den.double().sum()) - den_sum) < 1e-6
    bases = dict(dx=rn(T, E).float(), dw=rn(E).float(), db=rn(1).float(), dln_w=rn(E).float(), dln_b=rn(E).float())
    return dict(tag=f'E={E} R={R} rw={with_rw} den={den_sum} z~{z_shift} mean={x_mean}', x=x, rows=rows, ln_w=ln_w, ln_b=ln_b, w=w, b=b,
                label=label, rw=rw, den=den, gloss=torch.tensor([1.3]), bases=bases)


def head_fwd_args(c):
    return (c['x'], c['rows'], c['ln_w'], c['ln_b'], HEAD_EPS, c['w'], c['b'], c['label'], c['rw'], c['den'], HEAD_DEN_CONST)


def head_bwd_args(c, z32, mean32, rstd32):
    return (c['x'], c['rows'], c['ln_w'], c['ln_b'], c['w'], z32, mean32, rstd32, c['label'], c['rw'], c['den'], HEAD_DEN_CONST, c['gloss'])
