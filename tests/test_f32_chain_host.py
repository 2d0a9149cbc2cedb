"""The k-ordered fmaf-chain oracle (oracle/f32_chain.c) checked on the CPU, so that the yardstick of tests/test_strict_ops_gpu.py
is itself tested where there is no GPU.

Bars.  A K-term fp32 sum of exact products, in any order, is within gamma_K * sum |terms| of the exact sum, gamma_K = K u / (1 - K u)
with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The bar asserted is K * 2^-24 * sum |terms| --
a hair below gamma_K, which errs on the strict side -- against the same operation in fp64, whose own error (K * 2^-53) is nine orders
below.  sum |terms| is the same fp64 operation on |x|, |w|.  Where every partial sum is an integer below 2^24 no rounding happens and
the chain must equal the fp64 result exactly."""
import pytest
import torch
import torch.nn.functional as F

from oracle.f32_chain import chain_conv2d_nhwc, chain_gemm, conv_out_hw

U = 2.0**-24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def conv_ref64(x, w, mode):
    """fp64 torch form of the four modes.  x [N,H,W,Cin], w [Cout,taps,Cin] -> [N,Hout,Wout,Cout]."""
    xn = x.double().permute(0, 3, 1, 2)
    cout, taps, cin = w.shape
    k = 1 if mode == 3 else 3
    wn = w.double().view(cout, k, k, cin).permute(0, 3, 1, 2)
    if mode == 0:
        y = F.conv2d(xn, wn, padding=1)
    elif mode == 1:
        y = F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, stride=2)
    elif mode == 2:
        y = F.conv2d(F.interpolate(xn, scale_factor=2.0, mode='nearest'), wn, padding=1)
    else:
        y = F.conv2d(xn, wn)
    return y.permute(0, 2, 3, 1).contiguous()


def im2col(x, mode):
    """[N*Hout*Wout, taps*Cin] with k = (ky, kx, ci) ascending and zeros where a tap falls into the padding."""
    N, H, W, C = x.shape
    Ho, Wo = conv_out_hw(mode, H, W)
    taps = 1 if mode == 3 else 9
    cols = torch.zeros(N, Ho, Wo, taps, C, dtype=x.dtype)
    for oy in range(Ho):
        for ox in range(Wo):
            for t in range(taps):
                ky, kx = divmod(t, 3)
                if mode == 0:
                    iy, ix = oy + ky - 1, ox + kx - 1
                    ok = 0 <= iy < H and 0 <= ix < W
                elif mode == 1:
                    iy, ix = 2 * oy + ky, 2 * ox + kx
                    ok = iy < H and ix < W
                elif mode == 2:
                    uy, ux = oy + ky - 1, ox + kx - 1
                    ok = 0 <= uy < 2 * H and 0 <= ux < 2 * W
                    iy, ix = uy // 2, ux // 2
                else:
                    iy, ix, ok = oy, ox, True
                if ok:
                    cols[:, oy, ox, t] = x[:, iy, ix]
    return cols.view(N * Ho * Wo, taps * C)


GEMMS = [(1, 1, 4), (5, 3, 8), (65, 67, 20), (33, 70, 1028), (9, 12, 4608)]


@pytest.mark.parametrize('M,N,K', GEMMS)
@pytest.mark.parametrize('kmajor', [False, True])
def test_chain_gemm_within_gamma_of_fp64(M, N, K, kmajor):
    g = _gen(M * 7 + N * 3 + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    Bk = B.t().contiguous() if kmajor else B
    C = chain_gemm(A, Bk, kmajor)
    ref = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    assert C.shape == (M, N) and C.dtype == torch.float32
    assert bool(((C.double() - ref).abs() <= K * U * mag).all())


@pytest.mark.parametrize('M,N,K', GEMMS)
def test_chain_gemm_row_major_and_k_major_bit_equal(M, N, K):
    g = _gen(K + N)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    assert torch.equal(chain_gemm(A, B), chain_gemm(A, B.t().contiguous(), True))


def test_chain_gemm_leading_dimensions():
    """Row-strided views give the bits of their contiguous copies; what lies beyond K / N in a row is never read into the sum."""
    g = _gen(5)
    M, N, K = 37, 29, 52
    Abuf, Bbuf, Bkbuf = torch.randn(M, K + 4, generator=g), torch.randn(N, K + 8, generator=g), torch.randn(K, N + 4, generator=g)
    A, B, Bk = Abuf[:, :K], Bbuf[:, :K], Bkbuf[:, :N]
    assert torch.equal(chain_gemm(A, B), chain_gemm(A.contiguous(), B.contiguous()))
    assert torch.equal(chain_gemm(A, Bk, True), chain_gemm(A.contiguous(), Bk.contiguous(), True))


def test_chain_is_k_ordered_not_just_accurate():
    """2^24 + 1 + 1 ... : added in ascending k every +1 is lost to the rounding (ties to even); any pairwise or reversed
    order would keep some.  This pins the ORDER of the oracle, which no accuracy bound can."""
    K = 65
    A = torch.ones(1, K)
    B = torch.ones(1, K)
    B[0, 0] = 2.0**24
    assert chain_gemm(A, B).item() == 2.0**24
    assert chain_gemm(A.flip(1), B.flip(1)).item() == 2.0**24 + 64  # 64 ones first, then 2^24 + 64 is representable


@pytest.mark.parametrize('M,N,K', [(7, 9, 36), (20, 11, 1024)])
def test_chain_gemm_exact_on_small_integers(M, N, K):
    g = _gen(K)
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    B = torch.randint(-8, 9, (N, K), generator=g).float()  # |partial sums| <= 64 K < 2^24
    assert torch.equal(chain_gemm(A, B).double(), A.double() @ B.double().t())


CONVS = [(0, 2, 5, 7, 4, 3), (0, 1, 6, 10, 32, 40), (1, 2, 6, 4, 4, 3), (1, 1, 2, 2, 8, 8), (2, 2, 3, 5, 4, 3), (2, 1, 4, 2, 16, 36),
         (3, 1, 5, 7, 4, 3), (3, 2, 3, 4, 64, 8), (0, 1, 4, 4, 512, 5)]


def _conv_case(mode, N, H, W, cin, cout, integer=False):
    g = _gen(mode * 1000 + H * 37 + W * 11 + cin + cout)
    taps = 1 if mode == 3 else 9
    if integer:
        return (torch.randint(-8, 9, (N, H, W, cin), generator=g).float(),
                torch.randint(-8, 9, (cout, taps, cin), generator=g).float())
    return torch.randn(N, H, W, cin, generator=g), torch.randn(cout, taps, cin, generator=g)


@pytest.mark.parametrize('mode,N,H,W,cin,cout', CONVS)
def test_chain_conv_within_gamma_of_fp64(mode, N, H, W, cin, cout):
    x, w = _conv_case(mode, N, H, W, cin, cout)
    y = chain_conv2d_nhwc(x, w, mode)
    ref, mag = conv_ref64(x, w, mode), conv_ref64(x.abs(), w.abs(), mode)
    K = w.shape[1] * cin
    assert y.shape == ref.shape
    assert bool(((y.double() - ref).abs() <= K * U * mag).all())


@pytest.mark.parametrize('mode,N,H,W,cin,cout', CONVS)
def test_chain_conv_exact_on_small_integers(mode, N, H, W, cin, cout):
    x, w = _conv_case(mode, N, H, W, cin, cout, integer=True)  # |partial sums| <= 64 * 4608 < 2^24
    assert torch.equal(chain_conv2d_nhwc(x, w, mode).double(), conv_ref64(x, w, mode))


@pytest.mark.parametrize('mode,N,H,W,cin,cout', CONVS)
def test_chain_conv_equals_chain_gemm_on_im2col(mode, N, H, W, cin, cout):
    """The convolution skips padded taps, the unfolded matrix feeds them as zeros: the same bits (fmaf(0, w, acc) == acc)."""
    x, w = _conv_case(mode, N, H, W, cin, cout)
    y = chain_conv2d_nhwc(x, w, mode)
    cols = im2col(x, mode)
    assert torch.equal(y.view(-1, cout), chain_gemm(cols, w.view(cout, -1)))
