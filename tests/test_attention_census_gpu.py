"""Attention visibility census: which keys does every query row see?  A yes/no property per (query, key), tested as one.

With Q = 0 every score is 0, so every visible key of row i gets probability exactly 1 / n_i (n_i = number of visible keys) and
    lse2[b][h][i] = log2 n_i                                  -- an exact count, in an fp32 output;
    out[i][d] n_i = number of visible keys j with V[j][d] = 1 -- a small integer over n_i.
Three V patterns pin the visible SET of every row: V[j][d] = 1 iff j mod 64 = d (residue classes), iff (j div 64) mod 64 = d (key
tiles), and V = 1.  Bars: round(2^lse2) == n_i and |lse2 - log2 n_i| < 1/4 log2(1 + 1/n_i) (>= 8.8e-5 for n <= 4096: far above the
fp32 log2 error, and log2 n +- 3e-6 still rounds back to n over 1..4096); out within 2^-8 relative of count / n_i (P = 1 and the
0/1 values are exact in bf16, their fp32 sum is an exact integer, then one fp32 division and one bf16 rounding: 2^-9 + 2^-24), and
exactly 0 for an absent class.  The expected sets come from the header's words, evaluated on the CPU:
    key j is visible to row q  iff  j < L,  j <= q when causal,  j >= c0 when q == r0,  j >= c1 when q == r1   (rows mode)
    j < clamp(key_len[b], 1, L)                                                                               (mmvid_attention_fwd_keylen)
    j <= pos                                                                                                   (mmvid_attention_decode)
No case masks every key of a row: the header does not define that result (the Python layer only ever passes first-allowed columns
inside the sequence).  K is random and the buffers are guarded (tests/guarded.py): with Q = 0 it must not matter, and a key read from
outside the sequence is NaN.

The backward census (same Q = 0, indicator dO, random K) is described at test_attention_bwd_census."""
import pytest
import torch

from guarded import Guarded
from guarded import call_abi as _call

pytestmark = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NAN = float('nan')


def v_pattern(kind, L):
    j = torch.arange(L)
    if kind == 'ones':
        return torch.ones(L, 64, dtype=torch.float64)
    cls = j % 64 if kind == 'residue' else (j // 64) % 64
    return torch.nn.functional.one_hot(cls, 64).double()


def visible(L, mask):
    """[L, L] bool from the header's definition of the mask modes."""
    mode, r0, c0, r1, c1 = mask
    q, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    vis = torch.ones(L, L, dtype=torch.bool)
    if mode == 1:
        vis &= j <= q
    if mode == 2:
        vis &= ~((q == r0) & (j < c0)) & ~((q == r1) & (j < c1))
    assert bool(vis.any(1).all()), 'a case may not mask every key of a row'
    return vis


def check_counts(lse2, n, what):
    """lse2, n: [..., L]."""
    n = n.double().expand_as(lse2)
    got = torch.round(torch.exp2(lse2.double()))
    bad = ~(got == n)  # (a NaN is bad)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} rows see a wrong NUMBER of keys; first (index, seen, expected): ' + \
        str([(tuple(i.tolist()), int(got[tuple(i)]), int(n[tuple(i)])) for i in bad.nonzero()[:5]])
    margin = 0.25 * torch.log2(1 + 1 / n)
    assert bool(((lse2.double() - torch.log2(n)).abs() < margin).all()), f'{what}: lse2 is off log2 n by more than 1/4 log2(1 + 1/n)'


def check_classes(out, counts, n, what):
    """out [..., L, 64] (bf16) against counts / n."""
    want = counts.double() / n.double()[..., None]
    want = want.expand_as(out)
    got = out.double()
    bad = ~((got - want).abs() <= 2.0**-8 * want)  # (a NaN is bad)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} (row, class) entries see the wrong keys; first (index, got, expected count / n): ' + \
        str([(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad.nonzero()[:5]])


def run_fwd(L, mask, B=2, kinds=('residue', 'tile'), key_len=None):
    """One forward call with Q = 0, K random, head h carrying V pattern kinds[h]; padded leading dimensions, guards.  -> out
    [B, L, H, 64], lse2 [B, H, L]."""
    H = len(kinds)
    E = 64 * H
    g = torch.Generator().manual_seed(L * 7 + sum(mask))
    qkv = torch.zeros(B, L, 3, H, 64)
    qkv[:, :, 1] = torch.randn(B, L, H, 64, generator=g)
    for h, kind in enumerate(kinds):
        qkv[:, :, 2, h] = v_pattern(kind, L).float()
    ld, ldo = 3 * E + 8, E + 16
    x = Guarded(qkv.view(B * L, 3 * E).to(BF), ld=ld)
    o, lse = Guarded(role='out', shape=(B * L, E), dtype=BF, ld=ldo), Guarded(role='out', shape=(B, H, L), dtype=F32)
    if key_len is None:
        _call('mmvid_attention_fwd', x.ptr, ld, B, L, H, E, 0.125, *mask, o.ptr, ldo, lse.ptr)
    else:
        kl = Guarded(key_len)
        _call('mmvid_attention_fwd_keylen', x.ptr, ld, B, L, H, E, 0.125, kl.ptr, o.ptr, ldo, lse.ptr)
        kl.check('key_len')
    x.check('qkv')
    return o.check('out').view(B, L, H, 64), lse.check('lse2')


def census(L, mask, what):
    vis = visible(L, mask)
    n = vis.sum(1)
    kinds = ('residue', 'tile')
    out, lse2 = run_fwd(L, mask, kinds=kinds)
    check_counts(lse2, n[None, None, :], what)
    for h, kind in enumerate(kinds):
        check_classes(out[:, :, h], (vis.double() @ v_pattern(kind, L))[None], n[None], f'{what} [{kind} classes]')


LENGTHS = [1, 31, 64, 65, 130, 579, 1152]


@pytest.mark.parametrize('L', LENGTHS)
@pytest.mark.parametrize('mode', [0, 1], ids=['none', 'causal'])
def test_census_no_mask_and_causal(L, mode):
    census(L, (mode, -1, 0, -1, 0), f'attention_fwd L={L} mode={mode}')


def rows_specs(L):
    """(r0, c0, r1, c1): one restricted row with r and c on both sides of the kernels' tile boundaries, c != r, c = 0, c = L - 1, the
    unused form r = -1; then pairs of rows, among them the production (65, 65), (66, 66)."""
    edge = [v for v in (0, 1, 17, 30, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1151) if v < L]
    rs = [r for r in (63, 64, 65, 127, 128) if r < L] or [L - 1]
    if L <= 64:
        rs = sorted({0, L // 2, L - 1})
    specs = [(r, c, -1, 0) for r in rs for c in sorted(set(edge + [r, L - 1]))]
    specs += [(-1, 0, r, c) for r in rs for c in (r, L - 1, max(0, r - 1))]      # the first slot unused, the second in use
    specs += [(-1, 0, -1, 0)]                                                    # both unused: no restriction at all
    if L > 66:
        specs += [(65, 65, 66, 66), (63, 64, 64, 63), (64, 65, 65, 64), (127, L - 1, 128, 0), (64, 10, 64, 70), (128, 129, 0, 1)]
    elif L > 2:
        specs += [(L - 2, L - 2, L - 1, L - 1), (0, L - 1, L - 1, 1)]
    return [s for s in dict.fromkeys(specs) if max(s[0], s[2]) < L and max(s[1], s[3]) < L]


@pytest.mark.parametrize('L', LENGTHS)
def test_census_rows_mode(L):
    specs = rows_specs(L)
    assert len(specs) >= 3
    for r0, c0, r1, c1 in specs:
        census(L, (2, r0, c0, r1, c1), f'attention_fwd L={L} rows ({r0}, {c0}), ({r1}, {c1})')


@pytest.mark.parametrize('L', [65, 130, 579])
def test_census_keylen(L):
    """Key lengths 0 (clamped to 1), 1, 63, 64, 65, L and L + 5 (clamped), one per sequence in the same call."""
    kl = torch.tensor([0, 1, 63, 64, 65, L, L + 5], dtype=I32)
    n = kl.clamp(1, L).long()
    kinds = ('residue', 'tile')
    out, lse2 = run_fwd(L, (0, 0, 0, 0, 0), B=7, kinds=kinds, key_len=kl)
    check_counts(lse2, n[:, None, None], f'attention_fwd_keylen L={L}')
    vis = torch.arange(L)[None, :] < n[:, None]  # [B, L keys], the same for every query row
    for h, kind in enumerate(kinds):
        counts = (vis.double() @ v_pattern(kind, L))[:, None, :]
        check_classes(out[:, :, h], counts, n[:, None], f'attention_fwd_keylen L={L} [{kind} classes]')


@pytest.mark.parametrize('Lmax', [130, 4096])
@pytest.mark.parametrize('from_device', [False, True])
def test_census_decode(Lmax, from_device):
    """mmvid_attention_decode has no lse2: the residue and tile patterns plus V = 1 (a row that saw n keys of weight 1/n' sums to
    n / n').  Cache rows beyond pos are NaN."""
    kinds = ('residue', 'tile', 'ones')
    H, B = len(kinds), 2
    E = 64 * H
    for pos in (0, 63, 64, 65, Lmax - 1):
        g = torch.Generator().manual_seed(pos)
        cache = torch.zeros(B, Lmax, 2, H, 64)
        cache[:, :, 0] = torch.randn(B, Lmax, H, 64, generator=g)
        for h, kind in enumerate(kinds):
            cache[:, :, 1, h] = v_pattern(kind, Lmax).float()
        cache[:, pos + 1:] = NAN
        qkv = torch.zeros(B, 3 * E)
        qkv[:, E:] = NAN  # the header: only the Q part of the row is read
        ldq, ldo = 3 * E + 8, E + 8
        x, c = Guarded(qkv.to(BF), ld=ldq), Guarded(cache.view(B * Lmax, 2 * E).to(BF))
        p = Guarded(torch.tensor([pos], dtype=I32)) if from_device else None
        o = Guarded(role='out', shape=(B, E), dtype=BF, ld=ldo)
        _call('mmvid_attention_decode', x.ptr, ldq, c.ptr, B, Lmax, H, E, None if p is None else p.ptr, -3 if from_device else pos, 0.125, o.ptr, ldo)
        x.check('qkv'), c.check('cache')
        out = o.check('out').view(B, H, 64)
        n = torch.tensor(pos + 1)
        vis = (torch.arange(Lmax) <= pos).double()
        for h, kind in enumerate(kinds):
            check_classes(out[:, h], (vis @ v_pattern(kind, Lmax))[None], n[None], f'attention_decode Lmax={Lmax} pos={pos} [{kind}]')


# ======================================================================================================================== backward
BWD_CASES = [(L, m) for L in (1, 31, 64, 65, 130, 579) for m in ((0, -1, 0, -1, 0), (1, -1, 0, -1, 0))] + \
            [(31, (2, 17, 18, 30, 9)), (65, (2, 63, 64, 64, 1)), (130, (2, 64, 65, 128, 127)), (130, (2, 127, 0, 65, 129)),
             (579, (2, 65, 65, 66, 66)), (579, (2, 128, 578, 63, 64))]
C_BWD = 2.63  # twice the staged reference's worst ratio 1.3145: see test_attention_bwd_census (pinned by tests/test_attention_census_host.py)


def _bf(x64):
    return x64.float().bfloat16().double()


def bwd_inputs(L, mask):
    """K ~ N(0,1) (bf16), V = the residue-class indicator, dO[i][d] = 1 iff (i + 3) mod 64 = d."""
    g = torch.Generator().manual_seed(1000 + L * 7 + sum(mask))
    K = torch.randn(L, 64, generator=g).bfloat16().double()
    V = v_pattern('residue', L)
    dO = torch.nn.functional.one_hot((torch.arange(L) + 3) % 64, 64).double()
    return K, V, dO


def bwd_reference(L, mask, K, V, dO, scale=0.125, staged=False):
    """dQ, dK, dV of one (batch, head) at Q = 0 in fp64, and T = the sum of absolute terms of each element's final contraction.
    staged: rounded to bf16 exactly where csrc/attn.hip rounds -- the stored O (forward), P in front of the dV product, dS in front of
    the dQ / dK products, the three outputs -- with lse2 kept as the fp32 value of log2 n."""
    vis = visible(L, mask).double()
    n = vis.sum(1, keepdim=True)
    P = vis / n
    if staged:
        lse2 = torch.log2(n).float().double()
        P = vis * torch.exp2(-lse2)
    O = P @ V
    if staged:
        O = _bf(O)
    delta = (O * dO).sum(1, keepdim=True)
    dS = P * (dO @ V.t() - delta)
    Q = torch.zeros(L, 64, dtype=torch.float64)
    Pm, dSm = (_bf(P), _bf(dS)) if staged else (P, dS)
    dQ, dK, dV = scale * dSm @ K, scale * dSm.t() @ Q, Pm.t() @ dO
    if staged:
        dQ, dK, dV = _bf(dQ), _bf(dK), _bf(dV)
    T = (scale * dS.abs() @ K.abs(), scale * dS.abs().t() @ Q.abs(), P.t() @ dO.abs())
    return (dQ, dK, dV), T


def staged_worst_ratio():
    """Worst |staged - plain| / (2^-8 T) over BWD_CASES (CPU only)."""
    worst = 0.0
    for L, mask in BWD_CASES:
        K, V, dO = bwd_inputs(L, mask)
        plain, T = bwd_reference(L, mask, K, V, dO)
        staged, _ = bwd_reference(L, mask, K, V, dO, staged=True)
        for a, b, t in zip(staged, plain, T):
            live = t > 0
            if bool(live.any()):
                worst = max(worst, float(((a - b).abs()[live] / (2.0**-8 * t[live])).max()))
            assert bool((a[~live] == 0).all())
    return worst


@pytest.mark.parametrize('L,mask', BWD_CASES, ids=str)
def test_attention_bwd_census(L, mask):
    """Q = 0, indicator dO, random K, on the forward kernel's own O and lse2: dQ, dK, dV element by element against plain fp64.
    Bar per element: C_BWD 2^-8 T, T = the fp64 sum of absolute terms of that element's final contraction (dQ: scale sum_j |dS_ij K_jd|,
    dV: sum_i |P_ij dO_id|, dK: scale sum_i |dS_ij Q_id| = 0, so dK must be exactly 0).  C_BWD is twice the worst error / (2^-8 T) of
    the STAGED reference (fp64 arithmetic rounded to bf16 where attn.hip rounds: stored O, P, dS, the outputs) against plain fp64 over
    these very cases.  With Q = 0 every term of dK = scale dS^T Q is zero, so this test only demands dK == 0: the dS^T Q contraction of the
    dK/dV kernel gets no non-zero term here and its term coverage stays with the tolerance tests (tests/test_kernels_gpu.py,
    tests/test_attention_bwd_pipeline_gpu.py).  Measured worst ratio of the staged reference: 1.3145 (staged_worst_ratio(), CPU; the dS terms next to a delta close to 1 carry the
    rounding of the stored O), hence C_BWD = 2.63."""
    B, H, E = 2, 1, 64
    K, V, dO = bwd_inputs(L, mask)
    qkv = torch.zeros(B, L, 3, 64, dtype=torch.float64)
    qkv[:, :, 1], qkv[:, :, 2] = K, V
    ld, ldo, lddo, ldg = 3 * E + 8, E + 16, E + 24, 3 * E + 32
    x = Guarded(qkv.view(B * L, 3 * E).to(BF), ld=ld)
    o, lse = Guarded(role='out', shape=(B * L, E), dtype=BF, ld=ldo), Guarded(role='out', shape=(B, H, L), dtype=F32)
    _call('mmvid_attention_fwd', x.ptr, ld, B, L, H, E, 0.125, *mask, o.ptr, ldo, lse.ptr)
    O, lse2 = Guarded(o.check('out'), ld=ldo), Guarded(lse.check('lse2'))
    d = Guarded(dO.repeat(B, 1).to(BF), ld=lddo)
    delta, dqkv = Guarded(role='out', shape=(B, H, L), dtype=F32), Guarded(role='out', shape=(B * L, 3 * E), dtype=BF, ld=ldg)
    _call('mmvid_attention_bwd_bias', x.ptr, ld, O.ptr, ldo, d.ptr, lddo, lse2.ptr, delta.ptr, B, L, H, E, 0.125, *mask, dqkv.ptr, ldg, None)
    for gd in (x, O, lse2, d):
        gd.check('attention_bwd input')
    delta.check('delta')
    got = dqkv.check('dqkv').double().view(B, L, 3, 64)
    want, T = bwd_reference(L, mask, K, V, dO)
    worst = 0.0
    for i, name in enumerate(('dQ', 'dK', 'dV')):
        err = (got[:, :, i] - want[i][None]).abs()
        bar = C_BWD * 2.0**-8 * T[i][None].expand_as(err)
        live = bar > 0
        if bool(live.any()):
            worst = max(worst, float((err[live] / bar[live]).max()))
        bad = ~(err <= bar)
        assert not bool(bad.any()), f'attention_bwd census L={L} mask={mask} {name}: {int(bad.sum())} elements outside C 2^-8 T; first (index, got, want, bar): ' + \
            str([(tuple(j.tolist()), float(got[:, :, i][tuple(j)]), float(want[i][None].expand_as(err)[tuple(j)]), float(bar[tuple(j)])) for j in bad.nonzero()[:5]])
    print(f'attention_bwd census L={L} mask={mask}: worst err / (C 2^-8 T) = {worst:.3f}')
