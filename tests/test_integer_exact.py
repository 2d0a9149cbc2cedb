"""Integer-exact term coverage of the bf16 matrix kernels, through the C-ABI on guarded, padded buffers (tests/guarded.py).

bf16 products of small integers are exact, and so is their fp32 sum IN ANY ORDER while sum |terms| < 2^24: whatever a kernel's
tiling, split-K, atomics or pipelining, it must reproduce an integer reference bit for bit.  The bar is `torch.equal` (reported as
count + the first (index, got, want) triples): fp32 outputs against the exact value computed in fp64 on the CPU (every
intermediate is an integer -- or a multiple of 2^-8 -- below 2^24 in magnitude, hence exact there too), bf16 outputs against
round-to-nearest-even of that value.  A dropped, duplicated or misplaced term fails it; no tolerance is involved.

The condition on the inputs -- for every output element sum_k |a_k b_k| + |bias| + |residual| (+ |base| when accumulating) < 2^24,
likewise for every fused column sum and GroupNorm partial SUM -- is asserted from the actual tensors of every case by the host
tests at the top (they run without a GPU); the GPU tests use the same cached tensors.  Sums of squares of the GroupNorm partials
are not exact under that bound: they are compared with n 2^-23 sum(v^2) (n fp32 additions of non-negative terms in any order).

Every call also has all leading dimensions padded and all different, operands embedded in quiet NaN / sentinel guards: the padded
call equal to the exact reference is a stronger statement than "equal to the dense call"."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from guarded import Guarded, bits, report_mismatch
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen

gpu = pytest.mark.gpu
LIMIT = float(2**24)
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


def ints(g, shape, r, dtype=torch.float64):
    return torch.randint(-r, r + 1, tuple(shape), generator=g).to(dtype)


def rne_bf16(x64):
    """Round-to-nearest-even of an exactly fp32-representable fp64 value."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64)
    return x32.bfloat16()


def exact_f32(x64):
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), 'the reference itself is not exact in fp32: the case violates its own condition'
    return x32


def _in(t, padded_ld=None, stride=None):
    return None if t is None else Guarded(t, ld=padded_ld, stride=stride)


# =================================================================================================================== mmvid_gemm_bf16
LAYOUTS = [(0, 0), (0, 1), (1, 1)]
LAYOUT_SHAPES = [(128, 128, 64), (300, 136, 200), (1000, 768, 768), (579, 2304, 768)]  # tests/test_kernels_gpu.py::test_gemm_layouts


def _gemm_cases():
    cases = []

    def add(akm, bkm, M, N, K, r=3, **kw):
        if akm and M % 8:
            M = M // 8 * 8 + 8
        c = dict(akm=akm, bkm=bkm, M=M, N=N, K=K, r=r, batch=1, bias=False, residual=False, accumulate=False, save_pre=False, colsum=False,
                 out='f32', alpha=1.0, splitk=1)
        c.update(kw)
        extras = [k for k in ('bias', 'residual', 'accumulate', 'save_pre', 'colsum') if c[k]]
        c['id'] = '-'.join([f'{"T" if akm else "N"}{"T" if bkm else "N"}', f'{M}x{N}x{K}', c['out']] + extras +
                           ([f'batch{c["batch"]}'] if c['batch'] > 1 else []) + ([f'alpha{c["alpha"]}'] if c['alpha'] != 1 else []) +
                           ([f'splitk{c["splitk"]}'] if c['splitk'] > 1 else []))
        cases.append(c)

    for akm, bkm in LAYOUTS:
        for M, N, K in LAYOUT_SHAPES:
            add(akm, bkm, M, N, K)
            add(akm, bkm, M, N, K, out='bf16')
        add(akm, bkm, 72, 40, 8)                   # K below one tile
        add(akm, bkm, 72, 40, 8, out='bf16', bias=True)
        for sk in (3, 8):                          # atomics: the order is free and the sum still exact
            add(akm, bkm, 300, 136, 200, splitk=sk, accumulate=True)
            add(akm, bkm, 579, 2304, 768, splitk=sk, accumulate=True, bias=True)
        add(akm, bkm, 300, 136, 200, batch=3)
        add(akm, bkm, 300, 136, 200, batch=3, out='bf16', bias=True)
        add(akm, bkm, 300, 136, 200, bias=True, residual=True)
        add(akm, bkm, 300, 136, 200, out='both', bias=True, residual=True, save_pre=True)
        add(akm, bkm, 300, 136, 200, accumulate=True, bias=True)
        add(akm, bkm, 1000, 768, 768, r=2, colsum=True, bias=True)     # column sums over 1000 rows: operands in [-2, 2]
        add(akm, bkm, 579, 2304, 768, out='bf16', bias=True, save_pre=True)  # the packed store forms (N % 128 == 0)
        add(akm, bkm, 579, 2304, 768, colsum=True, residual=True)
        add(akm, bkm, 300, 136, 200, alpha=0.25, bias=True)
        add(akm, bkm, 1000, 768, 768, alpha=4.0, out='both', residual=True)
    for sk in (1, 3, 8):                           # the ragged shape of test_gemm_k_reduction_not_multiple_of_tile_and_splitk
        add(1, 1, 776, 264, 1043, splitk=sk, accumulate=True)
    add(1, 1, 776, 264, 1043, out='bf16')
    return cases


GEMM_CASES = _gemm_cases()


@functools.lru_cache(maxsize=2)
def gemm_data(cid):
    """CPU tensors of a case, the exact results (fp64) and sum |terms| per output element."""
    c = next(x for x in GEMM_CASES if x['id'] == cid)
    g = _gen('gemm', cid)
    M, N, K, nb, r = c['M'], c['N'], c['K'], c['batch'], c['r']
    A = ints(g, (nb, K, M) if c['akm'] else (nb, M, K), r)
    B = ints(g, (nb, K, N) if c['bkm'] else (nb, N, K), r)
    d = dict(A=A.to(BF), B=B.to(BF))
    Am = A.transpose(1, 2) if c['akm'] else A
    Bm = B if c['bkm'] else B.transpose(1, 2)
    acc, mag = Am @ Bm, Am.abs() @ Bm.abs()
    v, mag = c['alpha'] * acc, max(1.0, abs(c['alpha'])) * mag
    if c['bias']:
        d['bias'] = ints(g, (N,), 50, F32)
        v, mag = v + d['bias'].double(), mag + d['bias'].double().abs()
    d['pre'] = v
    if c['residual']:
        d['residual'] = ints(g, (nb, M, N), 100, F32)
        v, mag = v + d['residual'].double(), mag + d['residual'].double().abs()
    if c['accumulate']:
        d['base'] = ints(g, (nb, M, N), 100, F32)
        v, mag = v + d['base'].double(), mag + d['base'].double().abs()
    d['out'], d['mag'] = v, mag
    if c['colsum']:
        d['cs_base'] = ints(g, (N,), 1000, F32)
        d['cs'] = d['cs_base'].double() + v.sum((0, 1))
        d['cs_mag'] = d['cs_base'].double().abs() + mag.sum((0, 1))
    return d


@pytest.mark.parametrize('cid', [c['id'] for c in GEMM_CASES])
def test_gemm_inputs_keep_every_sum_exact(cid):
    d = gemm_data(cid)
    assert float(d['mag'].max()) < LIMIT, f'{cid}: sum |terms| reaches {float(d["mag"].max()):.0f}'
    assert float(d['mag'].max()) > 0
    if 'cs' in d:
        assert float(d['cs_mag'].max()) < LIMIT, f'{cid}: column sums reach {float(d["cs_mag"].max()):.0f}'
    assert all(torch.equal(d[k].double().to(BF).double(), d[k].double()) for k in ('A', 'B'))


def run_gemm(c, d, padded=True):
    """One mmvid_gemm_bf16 call with every operand guarded (padded: every leading dimension larger than natural and different,
    batch strides with gaps).  -> dict of result windows."""
    M, N, K, nb = c['M'], c['N'], c['K'], c['batch']
    ra, ca = (K, M) if c['akm'] else (M, K)
    rb, cb = (K, N) if c['bkm'] else (N, K)
    p = int(padded)
    lda, ldb, ldc, ldr, ldp = ca + 8 * p, cb + 16 * p, N + 12 * p, N + 20 * p, N + 28 * p
    sA, sB, sC = ra * lda + 16 * p, rb * ldb + 24 * p, M * ldc + 12 * p
    A, B = Guarded(d['A'], ld=lda, stride=sA), Guarded(d['B'], ld=ldb, stride=sB)
    bias, res = _in(d.get('bias')), _in(d.get('residual'), ldr)
    assert not (c['residual'] and nb > 1)
    o32 = o16 = save = cs = None
    if c['out'] in ('f32', 'both'):
        o32 = Guarded(base=d['base'], ld=ldc, stride=sC) if c['accumulate'] else Guarded(role='out', shape=(nb, M, N), dtype=F32, ld=ldc, stride=sC)
    if c['out'] in ('bf16', 'both'):
        o16 = Guarded(role='out', shape=(nb, M, N), dtype=BF, ld=ldc, stride=sC)
    if c['save_pre']:
        save = Guarded(role='out', shape=(nb, M, N), dtype=BF, ld=ldp)
    if c['colsum']:
        cs = Guarded(base=d['cs_base'])
    one = nb == 1
    _call('mmvid_gemm_bf16', c['akm'], c['bkm'], M, N, K, A.ptr, lda, B.ptr, ldb, nb, 0 if one else sA, 0 if one else sB, 0 if one else sC,
          c['splitk'], float(c['alpha']), _ptr(bias), _ptr(res), ldr, None, _ptr(save), ldp, 0, int(c['accumulate']), _ptr(o32), _ptr(o16),
          ldc, _ptr(cs))
    out = {}
    for name, gd in (('A', A), ('B', B), ('bias', bias), ('residual', res), ('out_f32', o32), ('out_bf16', o16), ('save_pre', save), ('colsum', cs)):
        if gd is not None:
            out[name] = gd.check(f'gemm {c["id"]} {name}')
    return out


@gpu
@pytest.mark.parametrize('cid', [c['id'] for c in GEMM_CASES])
def test_gemm_bf16_integer_exact(cid):
    c = next(x for x in GEMM_CASES if x['id'] == cid)
    d = gemm_data(cid)
    got = run_gemm(c, d)
    if 'out_f32' in got:
        report_mismatch(got['out_f32'], exact_f32(d['out']), f'gemm {cid} out_f32')
    if 'out_bf16' in got:
        report_mismatch(got['out_bf16'], rne_bf16(d['out']), f'gemm {cid} out_bf16')
    if 'save_pre' in got:
        report_mismatch(got['save_pre'], rne_bf16(d['pre']), f'gemm {cid} save_pre')
    if 'colsum' in got:
        report_mismatch(got['colsum'], exact_f32(d['cs']), f'gemm {cid} out_colsum')


# ======================================================================================= mmvid_gemm_bf16_dw, _dw_grouped, _dw_multi
#            M (tokens)  N     K     two kinds of different N and K; M = 579 * 6 and a ragged M
DW_SHAPES = [(579 * 6, 768, 256), (579 * 6, 264, 136), (1043, 768, 256), (1043, 264, 136), (8, 8, 8)]
DW_CASES = [(M, N, K, sk, acc) for (M, N, K) in DW_SHAPES for sk, acc in ((1, False), (5, True), ('pick', True))]


@functools.lru_cache(maxsize=8)
def dw_data(M, N, K, groups=1, r=3):
    g = _gen('dw', M, N, K, groups)
    dY, X = ints(g, (groups, M, N), r), ints(g, (groups, M, K), r)
    base = ints(g, (groups, N, K), 100, F32)
    dW = dY.transpose(1, 2) @ X
    mag = dY.abs().transpose(1, 2) @ X.abs() + base.double().abs()
    return dict(dY=dY.to(BF), X=X.to(BF), base=base, dW=dW, mag=mag)


@pytest.mark.parametrize('M,N,K', DW_SHAPES)
def test_dw_inputs_keep_every_sum_exact(M, N, K):
    for groups in (1, 3):
        d = dw_data(M, N, K, groups)
        assert 0 < float(d['mag'].max()) < LIMIT


@gpu
@pytest.mark.parametrize('M,N,K,sk,acc', DW_CASES, ids=lambda v: str(v))
def test_gemm_bf16_dw_integer_exact(M, N, K, sk, acc):
    from mmvid_amd import _lib
    d = dw_data(M, N, K)
    if sk == 'pick':
        sk = _lib.load().mmvid_gemm_dw_pick_splitk(M, N, K)
        print(f'dw {M}x{N}x{K}: the library picks split-K {sk}')
    ldy, ldx = N + 8, K + 24
    dY, X = Guarded(d['dY'][0], ld=ldy), Guarded(d['X'][0], ld=ldx)
    dW = Guarded(base=d['base'][0]) if acc else Guarded(role='out', shape=(N, K), dtype=F32)
    ws = Guarded(role='out', shape=(sk, N * K), dtype=F32, partial=True) if sk > 1 else None
    _call('mmvid_gemm_bf16_dw', M, N, K, dY.ptr, ldy, X.ptr, ldx, sk, _ptr(ws), dW.ptr, int(acc))
    dY.check('dY'), X.check('X')
    if ws is not None:
        ws.check('dw workspace')
    want = d['dW'][0] + (d['base'][0].double() if acc else 0)
    report_mismatch(dW.check('dW'), exact_f32(want), f'dw {M}x{N}x{K} splitk={sk} accumulate={acc}')


def _dw_operands(d, N, K, groups, k):
    M = d['dY'].shape[1]
    ldy, ldx = N + 8 * (k + 1), K + 24 + 8 * k
    dY = Guarded(d['dY'], ld=ldy, stride=M * ldy + 16)
    X = Guarded(d['X'], ld=ldx, stride=M * ldx + 40)
    return dY, X


@gpu
@pytest.mark.parametrize('M', [579 * 6, 1043])
@pytest.mark.parametrize('accumulate', [False, True])
def test_gemm_bf16_dw_grouped_integer_exact_and_null_entry(M, accumulate):
    """Three groups with gaps between them; the middle entry of dW_list is NULL: its slot keeps the sentinel, bit for bit."""
    N, K, G = 264, 136, 3
    d = dw_data(M, N, K, G)
    dY, X = _dw_operands(d, N, K, G, 0)
    dW = Guarded(base=d['base'], stride=N * K + 64) if accumulate else Guarded(role='out', shape=(G, N, K), dtype=F32, stride=N * K + 64, partial=True)
    before = dW.window()
    esz = 4
    ptrs = (ctypes.c_void_p * G)(*[None if g == 1 else dW.ptr.value + g * dW.stride * esz for g in range(G)])
    _call('mmvid_gemm_bf16_dw_grouped', M, N, K, dY.ptr, dY.ld, dY.stride, X.ptr, X.ld, X.stride, G, ptrs, int(accumulate))
    dY.check('dY'), X.check('X')
    got = dW.check('dW')
    assert torch.equal(bits(got[1]), bits(before[1])), 'the NULL entry of dW_list was written'
    want = exact_f32(d['dW'] + (d['base'].double() if accumulate else 0))
    for g in (0, 2):
        report_mismatch(got[g], want[g], f'dw_grouped M={M} group {g}')


@gpu
@pytest.mark.parametrize('M', [579 * 6, 1043])
def test_gemm_bf16_dw_multi_integer_exact_and_null_entry(M):
    """Two kinds of different N and K x three groups in one launch; one NULL entry per kind."""
    from mmvid_amd import _lib
    G, shapes = 3, [(768, 256), (264, 136)]
    arr = (_lib.DwKind * len(shapes))()
    keep, outs = [], []
    for k, (N, K) in enumerate(shapes):
        d = dw_data(M, N, K, G)
        dY, X = _dw_operands(d, N, K, G, k)
        dW = Guarded(base=d['base'], stride=N * K + 64)
        null = k + 1
        ptrs = (ctypes.c_void_p * G)(*[None if g == null else dW.ptr.value + g * dW.stride * 4 for g in range(G)])
        a = arr[k]
        a.N, a.K, a.dY, a.ldy, a.strideY = N, K, dY.ptr.value, dY.ld, dY.stride
        a.X, a.ldx, a.strideX, a.dW_list = X.ptr.value, X.ld, X.stride, ctypes.cast(ptrs, ctypes.c_void_p)
        keep.append(ptrs)
        outs.append((d, dY, X, dW, null))
    _call('mmvid_gemm_bf16_dw_multi', M, len(shapes), arr, G, 1)
    for k, (d, dY, X, dW, null) in enumerate(outs):
        dY.check('dY'), X.check('X')
        got = dW.check('dW')
        want = exact_f32(d['dW'] + d['base'].double())
        for g in range(G):
            report_mismatch(got[g], d['base'][g] if g == null else want[g], f'dw_multi M={M} kind {k} group {g}')


# =============================================================================================================== mmvid_colsum_bf16
COLSUM_SHAPES = [(10422, 768), (300, 3072), (1, 8), (257, 264)]  # tests/test_kernels_gpu.py::test_colsum_and_dw_workspace


@functools.lru_cache(maxsize=4)
def colsum_data(M, N):
    g = _gen('colsum', M, N)
    dy, base = ints(g, (M, N), 100), ints(g, (N,), 1000, F32)
    return dict(dy=dy.to(BF), base=base, want=base.double() + dy.sum(0), mag=base.double().abs() + dy.abs().sum(0))


@pytest.mark.parametrize('M,N', COLSUM_SHAPES)
def test_colsum_inputs_keep_every_sum_exact(M, N):
    d = colsum_data(M, N)
    assert 0 < float(d['mag'].max()) < LIMIT
    assert torch.equal(d['dy'].double().to(BF), d['dy'])


@gpu
@pytest.mark.parametrize('M,N', COLSUM_SHAPES)
def test_colsum_bf16_integer_exact(M, N):
    d = colsum_data(M, N)
    dy, db = Guarded(d['dy'], ld=N + 24), Guarded(base=d['base'])
    _call('mmvid_colsum_bf16', dy.ptr, dy.ld, M, N, db.ptr)
    dy.check('dy')
    report_mismatch(db.check('db'), exact_f32(d['want']), f'colsum {M}x{N}')


# ================================================================================================================= mmvid_gemv_rows
GEMV_CASES = [(NB, K, N, ri, ro) for NB in (1, 2, 3, 16, 17, 64) for (K, N) in ((512, 2048), (768, 768), (768, 2304))
              for ri, ro in ((1, 0), (1, 1))] + [(NB, 768, 768, 0, 0) for NB in (1, 2, 3)] + [(2, 3072, 768, 1, 1), (2, 512, 512, 0, 1)]


@functools.lru_cache(maxsize=4)
def gemv_data(NB, K, N):
    g = _gen('gemv', NB, K, N)
    x, W = ints(g, (NB, K), 3), ints(g, (N, K), 3)
    bias, res = ints(g, (N,), 50, F32), ints(g, (NB, N), 100, F32)
    want = x @ W.t() + bias.double() + res.double()
    mag = x.abs() @ W.abs().t() + bias.double().abs() + res.double().abs()
    return dict(x=x.float(), W=W.to(BF), bias=bias, res=res, want=want, mag=mag)


@pytest.mark.parametrize('NB,K,N', sorted({c[:3] for c in GEMV_CASES}))
def test_gemv_inputs_keep_every_sum_exact(NB, K, N):
    assert 0 < float(gemv_data(NB, K, N)['mag'].max()) < LIMIT


@gpu
@pytest.mark.parametrize('NB,K,N,round_in,round_out', GEMV_CASES)
def test_gemv_rows_integer_exact(NB, K, N, round_in, round_out):
    """Both forms (NB <= 2: the vector-ALU kernel; 3..64 bf16-exact rows: the matrix-pipe kernel, csrc/decode.hip -- no atomics in
    either), without LayerNorm or activation, bias and residual given and NULL.  round_in is a no-op on integer rows; round_out
    rounds the fp32 result to bf16 precision."""
    d = gemv_data(NB, K, N)
    for with_epilogue in (True, False):
        x, W = Guarded(d['x'], ld=K + 8), Guarded(d['W'])
        bias, res = (Guarded(d['bias']), Guarded(d['res'], ld=N + 12)) if with_epilogue else (None, None)
        out = Guarded(role='out', shape=(NB, N), dtype=F32, ld=N + 20)
        _call('mmvid_gemv_rows', x.ptr, x.ld, NB, K, None, None, 1e-5, W.ptr, _ptr(bias), N, 0, _ptr(res), N + 12, round_in, round_out,
              out.ptr, out.ld)
        for gd in (x, W, bias, res):
            if gd is not None:
                gd.check('gemv input')
        want = d['want'] if with_epilogue else d['want'] - d['bias'].double() - d['res'].double()
        want = rne_bf16(want).float() if round_out else exact_f32(want)
        report_mismatch(out.check('gemv out'), want, f'gemv_rows NB={NB} K={K} N={N} round_in={round_in} round_out={round_out} epilogue={with_epilogue}')


# ============================================================================================ mmvid_conv2d_nhwc, strip, first layer
# (mode, N, H, W, Cin, Cout): the shapes of test_conv_modes, test_conv_split_k and test_conv_fused_groupnorm_statistics
CONV_MODES_SHAPES = [(2, 16, 128, 128), (1, 8, 256, 512), (3, 4, 32, 64), (1, 32, 8, 128), (1, 16, 128, 8)]
CONV_SPLITK = [(0, 54, 8, 512, 512), (0, 3, 8, 256, 512), (0, 5, 8, 64, 264), (1, 2, 16, 128, 128), (3, 7, 8, 512, 256), (0, 1, 8, 8, 8)]
CONV_GN = [(0, 3, 16, 128, 128), (0, 2, 32, 64, 256), (1, 5, 32, 128, 128), (3, 2, 16, 256, 512), (0, 1, 48, 128, 128)]
CONV_CASES = ([(m, n, h, h, ci, co, 1, False) for m in range(4) for (n, h, ci, co) in CONV_MODES_SHAPES] +
              [(m, n, h, h, ci, co, sk, False) for (m, n, h, ci, co) in CONV_SPLITK for sk in (1, 2, 4)] +
              [(m, n, h, h, ci, co, 1, True) for (m, n, h, ci, co) in CONV_GN] +
              [(0, 2, 6, 128, 8, 128, 1, False), (0, 1, 4, 128, 8, 128, 1, True)])  # the first-layer kernel (Cin = 8, W = 128)
CONV_CASES = list(dict.fromkeys(CONV_CASES))
STRIP_SHAPES = [(2, 32, 32, 128, 128), (1, 64, 64, 128, 128), (3, 32, 32, 256, 256), (1, 128, 128, 128, 128), (2, 32, 32, 128, 256),
                (5, 16, 16, 256, 256), (3, 16, 16, 64, 128), (7, 8, 8, 512, 512), (1, 64, 32, 32, 128)]  # test_conv3x3_strip_vs_torch


def conv_ref(x, w, mode):
    """x [N,H,W,Cin], w [Cout,taps,Cin] fp64 -> [N,Ho,Wo,Cout] fp64.  Zero padding at all four borders (mode 0), zero pad right /
    bottom then stride 2 (mode 1), nearest x2 upsample then mode 0 (mode 2), 1x1 (mode 3)."""
    Cout, Cin = w.shape[0], w.shape[2]
    xn = x.permute(0, 3, 1, 2)
    wn = w.view(Cout, Cin, 1, 1) if mode == 3 else w.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    if mode == 0:
        y = F.conv2d(xn, wn, padding=1)
    elif mode == 1:
        y = F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, stride=2)
    elif mode == 2:
        y = F.conv2d(xn.repeat_interleave(2, 2).repeat_interleave(2, 3), wn, padding=1)
    else:
        y = F.conv2d(xn, wn)
    return y.permute(0, 2, 3, 1).contiguous()


def gn_partial_ref(v, block):
    """[N,Ho,Wo,C] -> sums and sums of squares [N][Ho*Wo/block][32] over (block pixels x C/32 channels), and the term count."""
    N, C = v.shape[0], v.shape[-1]
    t = v.reshape(N, -1, block, 32, C // 32)
    return t.sum((2, 4)), (t * t).sum((2, 4)), block * (C // 32)


@functools.lru_cache(maxsize=3)
def conv_data(mode, N, H, W, Cin, Cout, r=3, tag='conv'):
    g = _gen(tag, mode, N, H, W, Cin, Cout)
    x, w = ints(g, (N, H, W, Cin), r), ints(g, (Cout, 1 if mode == 3 else 9, Cin), r)
    bias = ints(g, (Cout,), 8, F32)
    acc, mag = conv_ref(x, w, mode), conv_ref(x.abs(), w.abs(), mode)
    res = ints(g, acc.shape, 8)
    pre = acc + bias.double()
    return dict(x=x, w=w, bias=bias, res=res, pre=pre, out=pre + res, mag=mag + bias.double().abs() + res.abs())


@pytest.mark.parametrize('case', CONV_CASES, ids=str)
def test_conv_inputs_keep_every_sum_exact(case):
    mode, N, H, W, Cin, Cout, sk, gn = case
    d = conv_data(mode, N, H, W, Cin, Cout)
    assert 0 < float(d['mag'].max()) < LIMIT
    if gn:
        s, _, _ = gn_partial_ref(d['mag'], 128)
        assert float(s.max()) < LIMIT, f'GroupNorm partial sums reach {float(s.max()):.0f}'


@pytest.mark.parametrize('shape', STRIP_SHAPES, ids=str)
def test_strip_conv_inputs_keep_every_sum_exact(shape):
    N, H, W, Cin, Cout = shape
    d = conv_data(0, N, H, W, Cin, Cout)
    s, _, _ = gn_partial_ref(d['mag'], 64)
    assert 0 < float(d['mag'].max()) < LIMIT and float(s.max()) < LIMIT


def check_gn(got, v, block, what):
    """got [N][blocks][32][2] against the exact sums (bit for bit) and sums of squares (n 2^-23 sum v^2: n fp32 additions of
    non-negative terms in any order, each product v*v rounded once)."""
    s, q, n = gn_partial_ref(v, block)
    report_mismatch(got[..., 0], exact_f32(s), what + ' GroupNorm partial sums')
    err = (got[..., 1].double() - q).abs()
    bound = n * 2.0**-23 * q
    assert bool((err <= bound).all()), f'{what} GroupNorm partial sums of squares: worst err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}'


@gpu
@pytest.mark.parametrize('case', CONV_CASES, ids=str)
def test_conv2d_nhwc_integer_exact(case):
    """fp32 output with a bf16 residual, bf16 output with an fp32 residual, and no residual into both outputs; guards and NaN poison
    around x, w, bias, the residual, the outputs, the split-K workspace and gn_partial."""
    mode, N, H, W, Cin, Cout, sk, gn = case
    d = conv_data(mode, N, H, W, Cin, Cout)
    Ho, Wo = d['out'].shape[1:3]
    first_layer = mode == 0 and Cin == 8 and W == 128  # conv_in_kernel: no residual, one output precision
    for variant in ('f32+res16', 'bf16+res32', 'both') + (('f32', 'bf16') if first_layer else ()):
        x, w, bias = Guarded(d['x'].to(BF).view(-1)), Guarded(d['w'].to(BF).view(-1)), Guarded(d['bias'])
        r16 = Guarded(d['res'].to(BF).view(-1)) if variant == 'f32+res16' else None
        r32 = Guarded(d['res'].float().view(-1)) if variant == 'bf16+res32' else None
        o32 = Guarded(role='out', shape=(N * Ho * Wo, Cout), dtype=F32) if variant in ('f32+res16', 'both', 'f32') else None
        o16 = Guarded(role='out', shape=(N * Ho * Wo, Cout), dtype=BF) if variant in ('bf16+res32', 'both', 'bf16') else None
        gnp = Guarded(role='out', shape=(N, Ho * Wo // 128, 64), dtype=F32) if gn and (o32 is not None or variant == 'bf16') else None
        ws = Guarded(role='out', shape=(sk, N * Ho * Wo * Cout), dtype=F32, partial=True) if sk > 1 else None
        _call('mmvid_conv2d_nhwc_splitk', mode, x.ptr, N, H, W, Cin, w.ptr, bias.ptr, Cout, _ptr(r16), _ptr(r32), 0, _ptr(o16), _ptr(o32),
              _ptr(gnp), sk, _ptr(ws))
        for gd in (x, w, bias, r16, r32, ws):
            if gd is not None:
                gd.check(f'conv {case} {variant}')
        want = d['out'] if 'res' in variant else d['pre']
        what = f'conv2d {case} {variant}'
        if o32 is not None:
            report_mismatch(o32.check(what).view(want.shape), exact_f32(want), what + ' out_f32')
        if o16 is not None:
            report_mismatch(o16.check(what).view(want.shape), rne_bf16(want), what + ' out_bf16')
        if gnp is not None:  # the statistics of the values the GroupNorm will read: bf16-rounded unless fp32 is stored
            check_gn(gnp.check(what).view(N, -1, 32, 2), want if o32 is not None else rne_bf16(want).double(), 128, what)


@gpu
@pytest.mark.parametrize('shape', STRIP_SHAPES, ids=str)
def test_conv3x3_strip_integer_exact(shape):
    N, H, W, Cin, Cout = shape
    d = conv_data(0, N, H, W, Cin, Cout)
    for variant in ('f32+res32+bf16', 'bf16+res16', 'f32'):
        x, w, bias = Guarded(d['x'].to(BF).view(-1)), Guarded(d['w'].to(BF).view(-1)), Guarded(d['bias'])
        r32 = Guarded(d['res'].float().view(-1)) if variant == 'f32+res32+bf16' else None
        r16 = Guarded(d['res'].to(BF).view(-1)) if variant == 'bf16+res16' else None
        o32 = Guarded(role='out', shape=(N * H * W, Cout), dtype=F32) if variant != 'bf16+res16' else None
        o16 = Guarded(role='out', shape=(N * H * W, Cout), dtype=BF) if variant != 'f32' else None
        gnp = Guarded(role='out', shape=(N, H * W // 64, 64), dtype=F32) if o32 is not None else None
        _call('mmvid_conv3x3_strip_nhwc', x.ptr, N, H, W, Cin, w.ptr, bias.ptr, Cout, _ptr(r16), _ptr(r32), _ptr(o16), _ptr(o32), _ptr(gnp))
        for gd in (x, w, bias, r16, r32):
            if gd is not None:
                gd.check(f'strip {shape} {variant}')
        want = d['pre'] if variant == 'f32' else d['out']
        what = f'strip conv {shape} {variant}'
        if o32 is not None:
            report_mismatch(o32.check(what).view(want.shape), exact_f32(want), what + ' out_f32')
        if o16 is not None:
            report_mismatch(o16.check(what).view(want.shape), rne_bf16(want), what + ' out_bf16')
        if gnp is not None:
            check_gn(gnp.check(what).view(N, -1, 32, 2), want, 64, what)


@gpu
@pytest.mark.parametrize('shape', STRIP_SHAPES[:3] + STRIP_SHAPES[-2:], ids=str)
def test_conv3x3_strip_f16_integer_exact(shape):
    """The IEEE-half operand form: the same integers as fp16."""
    N, H, W, Cin, Cout = shape
    d = conv_data(0, N, H, W, Cin, Cout)
    x, w, bias = Guarded(d['x'].to(F16).view(-1)), Guarded(d['w'].to(F16).view(-1)), Guarded(d['bias'])
    r32 = Guarded(d['res'].float().view(-1))
    o32 = Guarded(role='out', shape=(N * H * W, Cout), dtype=F32)
    gnp = Guarded(role='out', shape=(N, H * W // 64, 64), dtype=F32)
    _call('mmvid_conv3x3_strip_nhwc_f16', x.ptr, N, H, W, Cin, w.ptr, bias.ptr, Cout, r32.ptr, o32.ptr, gnp.ptr, None)
    for gd in (x, w, bias, r32):
        gd.check(f'strip f16 {shape}')
    what = f'strip conv f16 {shape}'
    report_mismatch(o32.check(what).view(d['out'].shape), exact_f32(d['out']), what)
    check_gn(gnp.check(what).view(N, -1, 32, 2), d['out'], 64, what)


@functools.lru_cache(maxsize=2)
def split3_data(mode, N, H, W, Cin, Cout):
    """x = x_hi + 2^-8 x_lo, w = w_hi + 2^-8 w_lo with small-integer planes.  The operator keeps x_hi.w_hi + x_lo.w_hi + x_hi.w_lo;
    the x_lo.w_lo term (2^-16 here) is DROPPED by design and therefore absent from the reference."""
    d = conv_data(mode, N, H, W, Cin, Cout)
    g = _gen('split3', mode, N, H, W, Cin, Cout)
    xl, wl = ints(g, d['x'].shape, 3), ints(g, d['w'].shape, 3)
    cross = (conv_ref(xl, d['w'], mode) + conv_ref(d['x'], wl, mode)) / 256.0
    mag3 = d['mag'] + (conv_ref(xl.abs(), d['w'].abs(), mode) + conv_ref(d['x'].abs(), wl.abs(), mode)) / 256.0
    return dict(d, x_lo=xl / 256.0, w_lo=wl / 256.0, out3=d['out'] + cross, mag3=mag3)


SPLIT3_STRIP = [STRIP_SHAPES[0], STRIP_SHAPES[6], STRIP_SHAPES[8]]
SPLIT3_CONV = [(0, 3, 4, 4, 32, 64, 1), (1, 2, 16, 16, 128, 128, 1), (2, 3, 4, 4, 32, 64, 1), (3, 7, 8, 8, 512, 256, 2), (0, 3, 8, 8, 256, 512, 4)]


@pytest.mark.parametrize('case', [(0,) + s for s in SPLIT3_STRIP] + [c[:6] for c in SPLIT3_CONV], ids=str)
def test_split3_inputs_keep_every_sum_exact(case):
    """Every term is a multiple of 2^-8: in those units the sum of absolute terms stays below 2^24."""
    d = split3_data(*case)
    assert 0 < float(d['mag3'].max()) * 256 < LIMIT
    for k in ('x_lo', 'w_lo'):
        assert torch.equal(d[k].to(BF).double(), d[k])


@gpu
@pytest.mark.parametrize('shape', SPLIT3_STRIP, ids=str)
def test_conv3x3_strip_split3_integer_exact(shape):
    N, H, W, Cin, Cout = shape
    d = split3_data(0, N, H, W, Cin, Cout)
    xp = Guarded(torch.stack([d['x'], d['x_lo']]).to(BF).view(-1))
    w3 = Guarded(torch.stack([d['w'], d['w'], d['w_lo']], 1).to(BF).view(-1))  # [Cout][3][taps][Cin] = (w_hi | w_hi | w_lo)
    bias, r32 = Guarded(d['bias']), Guarded(d['res'].float().view(-1))
    o32 = Guarded(role='out', shape=(N * H * W, Cout), dtype=F32)
    _call('mmvid_conv3x3_strip_nhwc_split3', xp.ptr, N, H, W, Cin, w3.ptr, bias.ptr, Cout, r32.ptr, o32.ptr, None, None)
    for gd in (xp, w3, bias, r32):
        gd.check(f'strip split3 {shape}')
    report_mismatch(o32.check('split3').view(d['out3'].shape), exact_f32(d['out3']), f'strip conv split3 {shape}')


@gpu
@pytest.mark.parametrize('case', SPLIT3_CONV, ids=str)
def test_conv2d_nhwc_split3_integer_exact(case):
    mode, N, H, W, Cin, Cout, sk = case
    d = split3_data(mode, N, H, W, Cin, Cout)
    Ho, Wo = d['out'].shape[1:3]
    xp = Guarded(torch.stack([d['x'], d['x_lo']]).to(BF).view(-1))
    w3 = Guarded(torch.stack([d['w'], d['w'], d['w_lo']], 1).to(BF).view(-1))
    bias, r32 = Guarded(d['bias']), Guarded(d['res'].float().view(-1))
    o32 = Guarded(role='out', shape=(N * Ho * Wo, Cout), dtype=F32)
    ws = Guarded(role='out', shape=(sk, N * Ho * Wo * Cout), dtype=F32, partial=True) if sk > 1 else None
    _call('mmvid_conv2d_nhwc_split3', mode, xp.ptr, N, H, W, Cin, w3.ptr, bias.ptr, Cout, r32.ptr, 0, o32.ptr, None, sk, _ptr(ws))
    for gd in (xp, w3, bias, r32):
        gd.check(f'conv split3 {case}')
    report_mismatch(o32.check('split3').view(d['out3'].shape), exact_f32(d['out3']), f'conv2d split3 {case}')


# =============================================================================================================== mmvid_conv3d_ndhwc
def _same_pad(n, k, s):
    total = max((-(-n // s) - 1) * s + k - n, 0)
    return total // 2, total - total // 2


# name -> (N, T, H, W, Cin, kernel, stride, pads or None (= TF SAME), relu, segments [(width, ldo, c_off)])
CONV3D_CASES = {
    'stem': (1, 6, 20, 12, 24, (7, 7, 1), (2, 2, 1), None, 1, [(64, 72, 8)]),                     # (kw, c) folded into 24 channels
    '3x3x3': (2, 4, 7, 7, 64, (3, 3, 3), (1, 1, 1), None, 1, [(192, 200, 0)]),                    # M = 392: ragged against every tile
    '3x3x3_into_concat': (1, 3, 5, 6, 32, (3, 3, 3), (1, 1, 1), None, 0, [(48, 128, 64)]),
    'three_segment_1x1x1': (2, 4, 7, 7, 192, (1, 1, 1), (1, 1, 1), None, 0, [(64, 256, 0), (96, 104, 0), (16, 32, 8)]),
}


@functools.lru_cache(maxsize=4)
def conv3d_data(name):
    N, T, H, W, Cin, k, s, pads, relu, segs = CONV3D_CASES[name]
    Cout = sum(w for w, _, _ in segs)
    pads = pads or [_same_pad(n, kk, ss) for n, kk, ss in zip((T, H, W), k, s)]
    g = _gen('conv3d', name)
    x, w, bias = ints(g, (N, T, H, W, Cin), 3), ints(g, (Cout, *k, Cin), 3), ints(g, (Cout,), 20, F32)

    def ref(xx, ww):
        xn = F.pad(xx.permute(0, 4, 1, 2, 3), (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
        return F.conv3d(xn, ww.permute(0, 4, 1, 2, 3), stride=s).permute(0, 2, 3, 4, 1)

    v = ref(x, w) + bias.double()
    mag = ref(x.abs(), w.abs()) + bias.double().abs()
    return dict(x=x, w=w, bias=bias, pads=pads, Cout=Cout, out=v.clamp_min(0) if relu else v, mag=mag)


@pytest.mark.parametrize('name', list(CONV3D_CASES))
def test_conv3d_inputs_keep_every_sum_exact(name):
    d = conv3d_data(name)
    assert 0 < float(d['mag'].max()) < LIMIT
    if not CONV3D_CASES[name][8]:
        assert float(d['out'].min()) < 0  # without the ReLU the sign must survive


@gpu
@pytest.mark.parametrize('name', list(CONV3D_CASES))
def test_conv3d_ndhwc_integer_exact(name):
    """The I3D convolution: TF-SAME pads in front and behind, strides, ReLU on and off, and the output split into column segments
    that land at a channel offset of wider rows (the Inception concat): the rest of those rows keeps the sentinel."""
    from mmvid_amd import _lib
    N, T, H, W, Cin, k, s, _, relu, segs = CONV3D_CASES[name]
    d = conv3d_data(name)
    M = d['out'][..., 0].numel()
    x, w, bias = Guarded(d['x'].to(BF).view(-1)), Guarded(d['w'].to(BF).view(-1)), Guarded(d['bias'])
    cfg = _lib.Conv3dCfg()
    cfg.N, cfg.T, cfg.H, cfg.W, cfg.Cin, cfg.Cout = N, T, H, W, Cin, d['Cout']
    (cfg.kt, cfg.kh, cfg.kw), (cfg.st, cfg.sh, cfg.sw) = k, s
    (cfg.pt0, cfg.pt1), (cfg.ph0, cfg.ph1), (cfg.pw0, cfg.pw1) = d['pads']
    cfg.relu, cfg.nseg = relu, len(segs)
    outs, end = [], 0
    for i, (width, ldo, c_off) in enumerate(segs):
        end += width
        o = Guarded(role='out', shape=(M, width), dtype=BF, ld=ldo)  # the window = this segment's columns of the wider rows
        cfg.seg_end[i], cfg.ldo[i], cfg.c_off[i], cfg.out[i] = end, ldo, c_off, o.ptr.value - 2 * c_off
        outs.append(o)
    _call('mmvid_conv3d_ndhwc', ctypes.byref(cfg), x.ptr, w.ptr, bias.ptr)
    for gd in (x, w, bias):
        gd.check(f'conv3d {name}')
    want, c0 = d['out'].reshape(M, -1), 0
    for o, (width, _, _) in zip(outs, segs):
        report_mismatch(o.check(f'conv3d {name}'), rne_bf16(want[:, c0:c0 + width]), f'conv3d {name} columns {c0}..{c0 + width - 1}')
        c0 += width
