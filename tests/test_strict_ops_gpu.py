"""Per-kernel tests of the fp32 strict VQGAN operators (mmvid_amd/csrc/strict.hip) through the C-ABI.

The file promises that every convolution / matmul output is ONE k-ordered fp32 fmaf chain, independent of tiling, batch size and
launch geometry; GroupNorm statistics in fp64; exp is expf.  The bars, none of which comes from the code under test:

* mmvid_gemm_f32, mmvid_conv2d_nhwc_f32, mmvid_image_to_nhwc4_f32: `torch.equal` with the CPU chain of oracle/f32_chain.c followed by
  the kernel's epilogue in torch fp32 on the CPU, one rounding per operation: v = chain + bias; v = v + residual;
  v = (clamp(v, -1, 1) + 1) * 0.5.  (alpha = 1 multiplies exactly; fma(acc, 1, bias) == acc + bias, so contraction cannot show.)
  Output buffers are sentinel-filled and compared whole: what lies beyond N in a row, between batches or behind the last row must
  keep the sentinel.  A bitwise failure reports whether the device output still satisfies the K-term fp32 bound
  gamma_K * sum |terms| against fp64 ("another summation order") or not ("wrong value").
* alpha != 1: the compiler may contract acc * alpha + bias into one fma (one rounding) or not (two), so the bar is
  |out - (alpha * chain + bias) in fp64| <= 0.5 ulp32(alpha * chain) + 0.5 ulp32(result).
* GroupNorm, softmax, attention: elementwise bounds written out from u = 2^-24 in the docstrings of the tests.

Inputs are seeded CPU randn / randint: finite normal numbers only."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0**-24
SENTINEL = -12345.678


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2**31)))


def _call(name, *args):
    from mmvid_amd import _lib
    _lib.call(name, *args)
    torch.cuda.synchronize()


def _p(t):
    from mmvid_amd import ops
    return ops._p(t)


def _stream():
    from mmvid_amd import ops
    return ops._stream()


def _ulp32(v):
    """fp32 spacing at |v| (v fp64 tensor)."""
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32)).astype(np.float64))


def assert_bits(got, want, what, ref64=None, mag64=None, K=None):
    """torch.equal, with a diagnosis on failure: how many elements differ, by how many fp32 ulps, and (given the fp64 value and
    sum |terms|) whether the device output is still a valid K-term fp32 sum -- another order -- or simply wrong."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    if torch.equal(got, want):
        return
    bad = got != want
    d = (got.double() - want.double()).abs()
    msg = (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fmaf chain, worst {float((d / _ulp32(want.double())).max()):.1f} ulp '
           f'at flat index {int(d.view(-1).argmax())}')
    if ref64 is not None:
        gk = K * U / (1 - K * U)
        inside = bool(((got.double() - ref64).abs() <= gk * mag64).all())
        msg += ('; the device output is inside gamma_K * sum|terms| of fp64: ANOTHER SUMMATION ORDER' if inside else
                '; the device output is outside gamma_K * sum|terms| of fp64: WRONG VALUE')
    raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------------------------ (a) gemm
def run_gemm(M, N, K, *, kmajor=False, lda=None, ldb=None, ldc=None, batch=1, sA=None, sB=None, sC=None, bias=False,
             residual=False, alpha=1.0, seed=0):
    """One mmvid_gemm_f32 call on flat, padded buffers.  -> (C buffer from the device, expected buffer, chain [batch,M,N], bias)."""
    from oracle.f32_chain import chain_gemm
    brows, bcols = (K, N) if kmajor else (N, K)
    lda, ldb, ldc = lda or K, ldb or bcols, ldc or N
    sA = M * lda if sA is None else sA
    sB = brows * ldb if sB is None else sB
    sC = M * ldc if sC is None else sC
    g = _gen(M, N, K, kmajor, lda, ldb, ldc, batch, seed)
    Abuf = torch.randn((batch - 1) * sA + M * lda, generator=g)
    Bbuf = torch.randn((batch - 1) * sB + brows * ldb, generator=g)
    Cbuf = torch.full(((batch - 1) * sC + M * ldc,), SENTINEL)
    Rbuf = torch.randn(Cbuf.numel(), generator=g) if residual else None
    bvec = torch.randn(N, generator=g) if bias else None
    dA, dB, dC = Abuf.to(DEV), Bbuf.to(DEV), Cbuf.to(DEV)
    dR, db = (Rbuf.to(DEV) if residual else None), (bvec.to(DEV) if bias else None)
    _call('mmvid_gemm_f32', int(kmajor), M, N, K, _p(dA), lda, _p(dB), ldb, batch, sA, sB, sC, float(alpha), _p(db), _p(dR), _p(dC),
          ldc, _stream())
    want, chains = Cbuf.clone(), []
    for b in range(batch):
        Av = Abuf.as_strided((M, K), (lda, 1), b * sA)
        Bv = Bbuf.as_strided((brows, bcols), (ldb, 1), b * sB)
        v = chain_gemm(Av, Bv, kmajor)
        chains.append(v)
        if alpha == 1.0:  # otherwise the caller derives its own bar
            if bias:
                v = v + bvec
            if residual:
                v = v + Rbuf.as_strided((M, N), (ldc, 1), b * sC)
            want.as_strided((M, N), (ldc, 1), b * sC).copy_(v)
    return dC.cpu(), want, torch.stack(chains), bvec


ROW_MAJOR = [(1, 1, 4), (5, 3, 8), (63, 4, 12), (64, 64, 16), (65, 67, 20), (300, 132, 36), (257, 512, 1024), (130, 260, 4608)]
K_MAJOR = [(64, 32, 16), (100, 68, 52), (256, 256, 256), (70, 516, 1028)]
ALL_GEMMS = [(s, False) for s in ROW_MAJOR] + [(s, True) for s in K_MAJOR]


@pytest.mark.parametrize('shape,kmajor', ALL_GEMMS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('kmajor' if v else 'rowmajor'))
def test_gemm_f32_is_the_fmaf_chain(shape, kmajor):
    """Tile edges in M, N and K (K below one 16-wide tile, K % 16 != 0, M and N ragged against 64) for both layouts of B."""
    M, N, K = shape
    got, want, _, _ = run_gemm(M, N, K, kmajor=kmajor)
    assert_bits(got, want, f'gemm_f32 {shape} kmajor={kmajor}')


@pytest.mark.parametrize('shape,kmajor', ALL_GEMMS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('kmajor' if v else 'rowmajor'))
def test_gemm_f32_leading_dimensions(shape, kmajor):
    """lda = K+4, ldb = K+8 (N+4 for a k-major B), ldc = N+5 into a sentinel-filled C: the same chain, and columns >= N of every
    row of C keep the sentinel (the buffers are compared whole)."""
    M, N, K = shape
    got, want, _, _ = run_gemm(M, N, K, kmajor=kmajor, lda=K + 4, ldb=(N + 4 if kmajor else K + 8), ldc=N + 5)
    assert int((want == SENTINEL).sum()) == 5 * M
    assert_bits(got, want, f'gemm_f32 {shape} kmajor={kmajor} with leading dimensions')


@pytest.mark.parametrize('kmajor', [False, True])
@pytest.mark.parametrize('shared_b', [False, True])
def test_gemm_f32_batched(kmajor, shared_b):
    """Three batches, each operand with a stride of its own (gaps between the batches of C keep the sentinel); strideB = 0 shares B."""
    M, N, K = 70, 68, 52
    brows, ldb = (K, N + 4) if kmajor else (N, K + 8)
    got, want, _, _ = run_gemm(M, N, K, kmajor=kmajor, lda=K + 4, ldb=ldb, ldc=N + 5, batch=3, sA=M * (K + 4) + 12,
                               sB=0 if shared_b else brows * ldb + 20, sC=M * (N + 5) + 7)
    assert_bits(got, want, f'gemm_f32 batched kmajor={kmajor} shared_b={shared_b}')


@pytest.mark.parametrize('HW,C', [(16, 32), (64, 128), (256, 512)])
def test_gemm_f32_attention_call_shapes(HW, C):
    """The two calls of mmvid_spatial_attention_f32, argument for argument: S = q k^T (row-major k, batch stride HW*HW of C) and
    o = P v (k-major v)."""
    hw2 = HW * HW
    got, want, _, _ = run_gemm(HW, HW, C, kmajor=False, lda=C, ldb=C, ldc=HW, batch=2, sA=HW * C, sB=HW * C, sC=hw2)
    assert_bits(got, want, f'gemm_f32 q k^T HW={HW} C={C}')
    got, want, _, _ = run_gemm(HW, C, HW, kmajor=True, lda=HW, ldb=C, ldc=C, batch=2, sA=hw2, sB=HW * C, sC=HW * C)
    assert_bits(got, want, f'gemm_f32 P v HW={HW} C={C}')


@pytest.mark.parametrize('shape,kmajor', [((65, 67, 20), False), ((300, 132, 36), False), ((100, 68, 52), True)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('kmajor' if v else 'rowmajor'))
@pytest.mark.parametrize('bias,residual', [(True, False), (False, True), (True, True)])
def test_gemm_f32_epilogue(shape, kmajor, bias, residual):
    M, N, K = shape
    got, want, _, _ = run_gemm(M, N, K, kmajor=kmajor, bias=bias, residual=residual)
    assert_bits(got, want, f'gemm_f32 {shape} bias={bias} residual={residual}')


def test_gemm_f32_residual_uses_the_strides_of_c():
    """The residual is addressed like C: ldc > N and a batch stride with a gap."""
    M, N, K = 65, 67, 20
    got, want, _, _ = run_gemm(M, N, K, ldc=N + 5, batch=2, sC=M * (N + 5) + 7, bias=True, residual=True)
    assert_bits(got, want, 'gemm_f32 residual, batch 2, ldc > N')


def test_gemm_f32_alpha():
    """alpha = float32(0.37) with a bias.  acc * alpha + bias is one fma or a multiply and an add, as the compiler likes, so the
    bar is the worse of the two: half an ulp of the product (absent when contracted) plus half an ulp of the result, against the
    expression in fp64 on the fp32 chain and the fp32 value of alpha."""
    M, N, K = 65, 67, 20
    alpha = float(np.float32(0.37))
    got, _, chain, bvec = run_gemm(M, N, K, bias=True, alpha=alpha)
    prod = chain[0].double() * alpha
    ref = prod + bvec.double()
    bar = 0.5 * _ulp32(prod) + 0.5 * _ulp32(ref)
    err = (got.view(M, N).double() - ref).abs()
    print(f'gemm_f32 alpha: worst err / bar = {float((err / bar).max()):.3f}')
    assert bool((err <= bar).all()), f'worst err / bar = {float((err / bar).max()):.3f}'


# ------------------------------------------------------------------------------------------------------------------ (b) conv
# (mode, N, H, W, Cin, Cout)
CONVS = [(0, 2, 32, 32, 4, 128),   # the stem: K = 36
         (0, 1, 6, 6, 64, 72),     # M = 36: less than one tile; ragged N
         (0, 3, 6, 10, 32, 40),    # a 64-row tile spans two images; ragged tail
         (0, 1, 16, 16, 128, 3),   # conv_out
         (0, 1, 8, 8, 512, 512),   # K = 4608
         (1, 2, 16, 12, 128, 128),
         (1, 1, 2, 2, 8, 8),       # one output pixel, every tap but four padded
         (2, 1, 8, 6, 256, 64),
         (2, 2, 3, 5, 16, 36),
         (3, 3, 8, 8, 512, 256),
         (3, 1, 5, 7, 4, 3)]
TAIL = 64  # sentinel floats behind the output


@functools.lru_cache(maxsize=4)
def conv_case(case, wscale):
    """(x, w, bias, residual, chain) of a case; w ~ wscale / sqrt(K) * randn, so the chain has a standard deviation of wscale."""
    from oracle.f32_chain import chain_conv2d_nhwc
    mode, N, H, W, cin, cout = case
    taps = 1 if mode == 3 else 9
    g = _gen(*case)
    x = torch.randn(N, H, W, cin, generator=g)
    w = torch.randn(cout, taps, cin, generator=g) * (wscale / (taps * cin)**0.5)
    chain = chain_conv2d_nhwc(x, w, mode)
    bias = 0.1 * torch.randn(cout, generator=g)
    res = 0.5 * torch.randn(chain.shape, generator=g)
    return x, w, bias, res, chain


def run_conv(case, x, w, bias=None, residual=None, clamp01=0):
    mode, N, H, W, cin, cout = case
    from oracle.f32_chain import conv_out_hw
    Ho, Wo = conv_out_hw(mode, H, W)
    numel = N * Ho * Wo * cout
    out = torch.full((numel + TAIL,), SENTINEL, device=DEV)
    dx, dw = x.to(DEV), w.to(DEV)
    db, dr = (bias.to(DEV) if bias is not None else None), (residual.to(DEV) if residual is not None else None)
    _call('mmvid_conv2d_nhwc_f32', mode, _p(dx), N, H, W, cin, _p(dw), _p(db), cout, _p(dr), clamp01, _p(out), _stream())
    out = out.cpu()
    assert bool((out[numel:] == SENTINEL).all()), 'conv2d_nhwc_f32 wrote behind its output'
    return out[:numel].view(N, Ho, Wo, cout)


def _conv_ref64(case, x, w):
    import torch.nn.functional as F
    mode, cout, cin = case[0], case[5], case[4]
    k = 1 if mode == 3 else 3
    xn, wn = x.double().permute(0, 3, 1, 2), w.double().view(cout, k, k, cin).permute(0, 3, 1, 2)
    if mode == 0:
        y = F.conv2d(xn, wn, padding=1)
    elif mode == 1:
        y = F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, stride=2)
    elif mode == 2:
        y = F.conv2d(F.interpolate(xn, scale_factor=2.0, mode='nearest'), wn, padding=1)
    else:
        y = F.conv2d(xn, wn)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('epilogue', ['plain', 'bias_residual', 'bias_residual_clamp'])
@pytest.mark.parametrize('case', CONVS, ids=lambda c: 'm{}_n{}_{}x{}_{}to{}'.format(*c))
def test_conv2d_nhwc_f32_is_the_fmaf_chain(case, epilogue):
    """Every mode at tile edges, with no epilogue, with bias + residual, and with bias + residual + clamp01 on weights scaled until
    a good share of v lies outside [-1, 1] on both sides (asserted on the oracle, so that the clamp is really exercised)."""
    x, w, bias, res, chain = conv_case(case, 1.5 if epilogue == 'bias_residual_clamp' else 1.0)
    K = w.shape[1] * w.shape[2]
    if epilogue == 'plain':
        got, want = run_conv(case, x, w), chain
        assert_bits(got, want, f'conv2d_nhwc_f32 {case}', _conv_ref64(case, x, w), _conv_ref64(case, x.abs(), w.abs()), K)
        return
    v = chain + bias
    v = v + res
    if epilogue == 'bias_residual_clamp':
        lo, hi = float((v < -1).float().mean()), float((v > 1).float().mean())
        assert 0.10 <= lo + hi <= 0.90, f'the clamp is not exercised: {lo:.2f} below -1, {hi:.2f} above 1'
        assert v.numel() < 64 or (lo >= 0.05 and hi >= 0.05), f'one side of the clamp is not exercised: {lo:.2f}, {hi:.2f}'
        v = (v.clamp(-1.0, 1.0) + 1.0) * 0.5
    got = run_conv(case, x, w, bias, res, clamp01=int(epilogue == 'bias_residual_clamp'))
    assert_bits(got, v, f'conv2d_nhwc_f32 {case} {epilogue}')


@pytest.mark.parametrize('case', [(0, 3, 6, 10, 32, 40), (1, 3, 6, 10, 16, 24), (2, 3, 3, 5, 16, 36), (3, 3, 5, 7, 64, 8)],
                         ids=lambda c: 'm{}_n{}_{}x{}_{}to{}'.format(*c))
def test_conv2d_nhwc_f32_batch_independent(case):
    """Image n of an N = 3 launch, where 64-row tiles straddle the images, equals the same image launched alone, bit for bit."""
    x, w, _, _, _ = conv_case(case, 1.0)
    full = run_conv(case, x, w)
    for n in range(3):
        alone = run_conv((case[0], 1) + case[2:], x[n:n + 1].contiguous(), w)
        assert torch.equal(full[n:n + 1], alone), f'image {n} depends on its batch'


# ------------------------------------------------------------------------------------------------------------- (c) GroupNorm
def run_groupnorm(x, w, b, eps, swish):
    N, hw, C = x.shape
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    stats = torch.full((N * C * 2 + TAIL,), SENTINEL, device=DEV)
    y = torch.full((x.numel() + TAIL,), SENTINEL, device=DEV)
    _call('mmvid_groupnorm_swish_nhwc_f32', _p(dx), N, hw, C, _p(dw), _p(db), eps, int(swish), _p(stats), _p(y), _stream())
    stats, y = stats.cpu(), y.cpu()
    assert bool((stats[N * C * 2:] == SENTINEL).all()) and bool((y[x.numel():] == SENTINEL).all()), 'groupnorm_f32 wrote out of bounds'
    return y[:x.numel()].view(N, hw, C), stats[:N * C * 2].view(N, C, 2)


def _gn_inputs(N, hw, C, offset, seed=0):
    g = _gen(N, hw, C, int(offset * 10) + 1000, seed)
    x = 1.5 * torch.randn(N, hw, C, generator=g) + offset
    return x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


GN_CASES = [(2, 4096, 128, 0.3, 0), (1, 16384, 128, 30, 0), (1, 16384, 128, 30, 1), (3, 64, 512, 5, 1), (2, 1, 64, 0, 1),
            (1, 16, 32, -30, 1), (1, 1024, 256, 100, 0)]


@pytest.mark.parametrize('N,hw,C,offset,swish', GN_CASES)
def test_groupnorm_f32_against_fp64(N, hw, C, offset, swish):
    """GroupNorm(32) [+ swish] against fp64 on the same fp32 x, elementwise, on data with a large mean -- where fp64 statistics are
    the whole point: fp32 one-pass statistics miss this bar by 20-250 x on the offset cases.

    Bound, u = 2^-24.  The kernel evaluates ((x - mean32) * rstd32) * w + b in fp32, with n = (x - mean) rstd and ref = n w + b:
      mean32 = mean (1 + d), |d| <= u     -> an absolute error u |mean| on x - mean, i.e. u |mean| rstd |w| on the result;
      the subtraction, rstd32, two multiplies (or one and an fma) -> at most 4 relative roundings of n w: 4 u |n w|;
      the final add                                               -> u |ref|.
    B0 = u (|mean| rstd |w| + 4 |n w| + |ref|); the bar is 2 B0 (second-order terms and the statistics' own 1e-12 are inside the
    factor 2).  With swish s(y) = y sigma(y): |s'| <= 1.1 carries B0 through, and expf (<= 2 ulp), the add, the divide and the
    multiply of o * (1 / (1 + expf(-o))) add 8 u |s(ref)|: the bar is 2 (1.1 B0 + 8 u |ref sigma(ref)|).
    Also: the (mean, rstd) pairs left in stats_scratch are the fp64 values rounded to fp32, within 1 ulp."""
    eps = 1e-6
    x, w, b = _gn_inputs(N, hw, C, offset)
    y, stats = run_groupnorm(x, w, b, eps, swish)
    cpg = C // 32
    xg = x.double().view(N, hw, 32, cpg)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean)**2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    n = ((xg - mean) * rstd).view(N, hw, C)
    mean_c, rstd_c = mean.expand(N, 1, 32, cpg).reshape(N, 1, C), rstd.expand(N, 1, 32, cpg).reshape(N, 1, C)
    wd, bd = w.double(), b.double()
    ref = n * wd + bd
    B0 = U * (mean_c.abs() * rstd_c * wd.abs() + 4 * (n * wd).abs() + ref.abs())
    if swish:
        sw = ref * torch.sigmoid(ref)
        bar, ref = 2 * (1.1 * B0 + 8 * U * sw.abs()), sw
    else:
        bar = 2 * B0
    err = (y.double() - ref).abs()
    print(f'groupnorm_f32 {(N, hw, C, offset, swish)}: worst err / bar = {float((err / bar).max()):.3f}')
    assert bool((err <= bar).all()), f'worst err / bar = {float((err / bar).max()):.3f}'
    for i, (name, val) in enumerate((('mean', mean_c), ('rstd', rstd_c))):
        want = val.reshape(N, C).float()
        d = (stats[:, :, i].double() - want.double()).abs()
        assert bool((d <= _ulp32(want.double())).all()), f'{name} in stats_scratch is more than 1 ulp from fp64'


def test_groupnorm_f32_batch_independent():
    x, w, b = _gn_inputs(3, 64, 512, 5)
    y, stats = run_groupnorm(x, w, b, 1e-6, 1)
    for n in range(3):
        y1, s1 = run_groupnorm(x[n:n + 1].contiguous(), w, b, 1e-6, 1)
        assert torch.equal(y[n:n + 1], y1) and torch.equal(stats[n:n + 1], s1), f'image {n} depends on its batch'


# ----------------------------------------------------------------------------------------------- (d) softmax and attention
def run_attention(q, k, v):
    """-> (out [N,HW,C], S [N,HW,HW], P [N,HW,HW]) of mmvid_spatial_attention_f32 with scale = float32(C^-0.5)."""
    N, HW, C = q.shape
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    scratch = torch.full((2 * N * HW * HW + TAIL,), SENTINEL, device=DEV)
    out = torch.full((N * HW * C + TAIL,), SENTINEL, device=DEV)
    _call('mmvid_spatial_attention_f32', _p(dq), _p(dk), _p(dv), N, HW, C, float(np.float32(C**-0.5)), _p(scratch), _p(out), _stream())
    scratch, out = scratch.cpu(), out.cpu()
    assert bool((scratch[2 * N * HW * HW:] == SENTINEL).all()) and bool((out[N * HW * C:] == SENTINEL).all()), 'attention_f32 wrote out of bounds'
    S, P = scratch[:2 * N * HW * HW].view(2, N, HW, HW)
    return out[:N * HW * C].view(N, HW, C), S, P


def _softmax_bar(t):
    """Relative bar of one softmax element, t = S * scale in fp64 [.., rows, cols] (see test_softmax_f32_through_identity_v)."""
    tmax = t.max(dim=-1, keepdim=True).values
    return 2 * U * (t.abs() + tmax.abs() + (t - tmax).abs() + 32)


@pytest.mark.parametrize('N,HW,C,a', [(2, 16, 32, 2), (1, 64, 128, 2), (3, 256, 256, 1), (1, 256, 512, 3), (1, 64, 128, 8)])
def test_softmax_f32_through_identity_v(N, HW, C, a):
    """The softmax kernel read exactly through the public interface: q, k integer-valued in [-a, a], so S = q k^T is an exact
    integer below 2^24 and its chain has no rounding; v = eye(HW, C), so out[:, :, :HW] == P and out[:, :, HW:] == 0 exactly.
    Reference: fp64 softmax of t = S * float32(C^-0.5).  Bar per element, relative to P_ref (P_ref < 1e-30 skipped: subnormal
    results are out of scope), u = 2^-24:
      e = expf(fl(fl(S scale) - mx)): the roundings of t, of mx and of the difference move the exponent by u (|t| + |t_max| +
          |t - t_max|), which is the relative error of e; expf itself <= 2 u;                                  -> |t|+|t_max|+|t-t_max| + 2
      the row sum: each term carries the same kind of error (bounded by the row's worst, counted once more in the factor 2), at
          most 15 additions per lane over a 1024-column row and 6 more across the 64 lanes                    -> 21 + ...
      the divide                                                                                              -> 1
    first order: u (|t| + |t_max| + |t - t_max| + 24 + the sum's share of the argument error); the bar is
    2 u (|t| + |t_max| + |t - t_max| + 32).  a = 8 drives |t| to ~90 and saturates most rows above 0.99."""
    g = _gen(N, HW, C, a)
    q = torch.randint(-a, a + 1, (N, HW, C), generator=g).float()
    k = torch.randint(-a, a + 1, (N, HW, C), generator=g).float()
    v = torch.eye(HW, C).expand(N, HW, C).contiguous()
    out, S, P = run_attention(q, k, v)
    S64 = q.double() @ k.double().transpose(1, 2)
    assert float(S64.abs().max()) < 2.0**24
    assert torch.equal(S.double(), S64), 'S = q k^T is not exact on small integers'
    assert torch.equal(out[:, :, :HW], P) and bool((out[:, :, HW:] == 0).all()), 'P v with v = eye does not return P'
    t = S64 * float(np.float32(C**-0.5))
    Pref = torch.softmax(t, dim=-1)
    if a == 8:
        assert float((Pref.max(dim=-1).values > 0.99).float().mean()) > 0.5, 'the saturated case is not saturated'
    keep = Pref >= 1e-30
    rel = ((P.double() - Pref).abs() / Pref.clamp_min(1e-300))[keep]
    bar = _softmax_bar(t)[keep]
    print(f'softmax_f32 {(N, HW, C, a)}: worst rel / bar = {float((rel / bar).max()):.3f}, |t| up to {float(t.abs().max()):.1f}')
    assert bool((rel <= bar).all()), f'worst rel / bar = {float((rel / bar).max()):.3f}'
    assert bool((P[~keep] <= 1e-29).all())


@pytest.mark.parametrize('HW,C', [(16, 32), (64, 128), (256, 256), (256, 512)])
def test_attention_f32_random_operands_against_fp64(HW, C):
    """softmax(q k^T C^-0.5) v on randn operands against fp64 end to end.  Composed bound, u = 2^-24, gamma_n = n u / (1 - n u):
      S:   |S32 - S| <= eS = gamma_C sum_c |q k|  (a C-term fp32 chain), so the exponent of element j is off by d_j = scale eS_j;
      P:   the numerator moves by exp(d_j), the row sum by at most exp(max_j d_j), and the softmax kernel adds its own relative
           error r_j (the bar of test_softmax_f32_through_identity_v, with the arguments known to d only: + 4 d_max inside):
           rho_j = (1 + r_j) exp(d_j + d_max) - 1;
      out: |out32 - out| <= sum_j P_j rho_j |v_j|  +  gamma_HW sum_j P_j (1 + rho_j) |v_j|   (the second chain, HW terms).
    Also: S in the scratch is bit-equal to the CPU chain, and every image of the batch is bit-equal to the image run alone."""
    from oracle.f32_chain import chain_gemm
    N = 3
    g = _gen(HW, C)
    q, k, v = (torch.randn(N, HW, C, generator=g) for _ in range(3))
    out, S, P = run_attention(q, k, v)
    for n in range(N):
        assert_bits(S[n], chain_gemm(q[n], k[n]), f'attention_f32 S of image {n}')
        assert_bits(out[n], chain_gemm(P[n].contiguous(), v[n], True), f'attention_f32 P v of image {n}')
    scale = float(np.float32(C**-0.5))
    qd, kd, vd = q.double(), k.double(), v.double()
    S64 = qd @ kd.transpose(1, 2)
    d = scale * (C * U / (1 - C * U)) * (qd.abs() @ kd.abs().transpose(1, 2))
    dmax = d.max(dim=-1, keepdim=True).values
    t = S64 * scale
    tmax = t.max(dim=-1, keepdim=True).values
    r = 2 * U * (t.abs() + tmax.abs() + (t - tmax).abs() + 32 + 4 * dmax)
    rho = (1 + r) * torch.exp(d + dmax) - 1
    P64 = torch.softmax(t, dim=-1)
    ref = P64 @ vd
    bar = (P64 * rho) @ vd.abs() + (HW * U / (1 - HW * U)) * ((P64 * (1 + rho)) @ vd.abs())
    err = (out.double() - ref).abs()
    print(f'attention_f32 HW={HW} C={C}: worst err / bar = {float((err / bar).max()):.3f}')
    assert bool((err <= bar).all()), f'worst err / bar = {float((err / bar).max()):.3f}'
    for n in range(N):
        o1, S1, P1 = run_attention(q[n:n + 1].contiguous(), k[n:n + 1].contiguous(), v[n:n + 1].contiguous())
        assert torch.equal(o1[0], out[n]) and torch.equal(S1[0], S[n]) and torch.equal(P1[0], P[n]), f'image {n} depends on its batch'


# ------------------------------------------------------------------------------------------------------------------ (e) image
@pytest.mark.parametrize('N,H,W', [(1, 1, 1), (3, 5, 7), (2, 16, 17), (1, 31, 9)])
def test_image_to_nhwc4_f32(N, H, W):
    """2 img - 1 in NHWC with a zero fourth channel, N H W not a multiple of the 256-thread block.  2 s is exact, so 2 s - 1 has
    one rounding whether or not the compiler contracts it: bitwise."""
    assert (N * H * W) % 256 != 0
    img = torch.rand(N, 3, H, W, generator=_gen(N, H, W))
    out = torch.full((N * H * W * 4 + TAIL,), SENTINEL, device=DEV)
    dimg = img.to(DEV)
    _call('mmvid_image_to_nhwc4_f32', _p(dimg), N, H, W, _p(out), _stream())
    out = out.cpu()
    assert bool((out[N * H * W * 4:] == SENTINEL).all()), 'image_to_nhwc4_f32 wrote behind its output'
    want = torch.zeros(N, H, W, 4)
    want[..., :3] = (2.0 * img - 1.0).permute(0, 2, 3, 1)
    assert_bits(out[:N * H * W * 4].view(N, H, W, 4), want, 'image_to_nhwc4_f32')


# --------------------------------------------------------------------------------------------------------- (f) argument checks
def test_strict_argument_checks():
    from mmvid_amd._lib import MMVIDError
    buf = torch.zeros(4096, device=DEV)
    p, s = _p(buf), _stream()

    def gemm(kmajor, M, N, K, lda, ldb):
        _call('mmvid_gemm_f32', kmajor, M, N, K, p, lda, p, ldb, 1, 0, 0, 0, 1.0, None, None, p, N, s)

    def conv(mode, H, W, cin):
        _call('mmvid_conv2d_nhwc_f32', mode, p, 1, H, W, cin, p, None, 4, None, 0, p, s)

    with pytest.raises(MMVIDError):
        gemm(0, 4, 4, 6, 8, 8)  # K % 4
    with pytest.raises(MMVIDError):
        gemm(0, 4, 4, 8, 10, 8)  # lda % 4
    with pytest.raises(MMVIDError):
        gemm(0, 4, 4, 8, 8, 10)  # ldb % 4
    with pytest.raises(MMVIDError):
        gemm(1, 4, 6, 8, 8, 8)  # k-major B with N % 4
    with pytest.raises(MMVIDError):
        conv(0, 4, 4, 12)  # Cin not a power of two
    with pytest.raises(MMVIDError):
        conv(0, 4, 4, 2)  # Cin below 4
    with pytest.raises(MMVIDError):
        conv(1, 5, 4, 8)  # downsample of an odd H
    with pytest.raises(MMVIDError):
        conv(4, 4, 4, 8)  # no such mode
    with pytest.raises(MMVIDError):
        _call('mmvid_groupnorm_swish_nhwc_f32', p, 1, 4, 48, p, p, 1e-6, 0, p, p, s)  # C % 32
    with pytest.raises(MMVIDError):
        _call('mmvid_spatial_attention_f32', p, p, p, 1, 6, 8, 0.35, p, p, s)  # HW % 4
    gemm(0, 4, 4, 8, 8, 8)  # and the checks are not simply refusing everything
    assert float(buf.abs().sum()) == 0.0
