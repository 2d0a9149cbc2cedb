"""k-ordered fp32 fmaf chains: ctypes wrapper over f32_chain.c, the bit-exact yardstick of csrc/strict.hip.

TEST INFRASTRUCTURE.  Everything here is CPU fp32 in one fixed order; rows are spread over a few threads (each output
element is its own chain, so the split cannot change a bit).
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import torch

from .build import build

_lib = None
THREADS = max(1, min(16, os.cpu_count() or 1))


def _load():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        P, I64 = ctypes.c_void_p, ctypes.c_int64
        _lib.oracle_chain_gemm.argtypes = [P, I64, P, I64, ctypes.c_int, I64, I64, I64, P, I64]
        _lib.oracle_chain_gemm.restype = None
        _lib.oracle_chain_conv2d_nhwc.argtypes = [ctypes.c_int, P, I64, I64, I64, I64, P, I64, P, I64, I64]
        _lib.oracle_chain_conv2d_nhwc.restype = None
    return _lib


def _rows2d(t, name):
    """fp32 CPU [rows, cols] whose columns are contiguous; the row stride is the leading dimension."""
    assert t.dtype == torch.float32 and t.device.type == 'cpu' and t.dim() == 2, name
    assert t.shape[1] == 1 or t.stride(1) == 1, f'{name}: columns must be contiguous'
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _spread(fn, rows, work_per_row):
    """fn(r0, r1) over [0, rows) in chunks, on threads when the work is worth it (ctypes releases the GIL)."""
    nthr = THREADS if rows * work_per_row >= 1 << 22 else 1
    nthr = min(nthr, rows)
    if nthr <= 1:
        fn(0, rows)
        return
    step = -(-rows // nthr)
    with ThreadPoolExecutor(max_workers=nthr) as ex:
        list(ex.map(lambda r0: fn(r0, min(rows, r0 + step)), range(0, rows, step)))


def chain_gemm(A, B, b_kmajor=False):
    """C[m][n] = fmaf(A[m][K-1], B(n,K-1), ... fmaf(A[m][0], B(n,0), 0.0f)).  A [M,K]; B [N,K] or, with b_kmajor, [K,N].
    Row-strided views are taken as they are (their row stride is the leading dimension).  -> contiguous [M,N]."""
    lda, ldb = _rows2d(A, 'A'), _rows2d(B, 'B')
    M, K = A.shape
    N = B.shape[1] if b_kmajor else B.shape[0]
    assert (B.shape[0] if b_kmajor else B.shape[1]) == K
    C = torch.empty(M, N, dtype=torch.float32)
    lib = _load()

    def part(r0, r1):
        lib.oracle_chain_gemm(A.data_ptr() + 4 * r0 * lda, lda, B.data_ptr(), ldb, int(b_kmajor), r1 - r0, N, K,
                              C.data_ptr() + 4 * r0 * N, N)

    _spread(part, M, N * K)
    return C


def conv_out_hw(mode, H, W):
    return (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)


def chain_conv2d_nhwc(x, w, mode):
    """The four modes of mmvid_conv2d_nhwc (0: 3x3 pad 1; 1: pad (0,1,0,1) + stride 2; 2: nearest x2 then 3x3 pad 1; 3: 1x1) as
    one chain per output, k = (ky, kx, ci) ascending.  x [N,H,W,Cin], w [Cout,taps,Cin] -> [N,Hout,Wout,Cout]."""
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_contiguous() and w.is_contiguous()
    N, H, W, Cin = x.shape
    Cout, taps = w.shape[0], w.shape[1]
    assert mode in (0, 1, 2, 3) and taps == (1 if mode == 3 else 9) and w.shape[2] == Cin
    assert mode != 1 or (H % 2 == 0 and W % 2 == 0)
    Ho, Wo = conv_out_hw(mode, H, W)
    out = torch.empty(N, Ho, Wo, Cout, dtype=torch.float32)
    lib = _load()
    _spread(lambda r0, r1: lib.oracle_chain_conv2d_nhwc(mode, x.data_ptr(), N, H, W, Cin, w.data_ptr(), Cout,
                                                        out.data_ptr(), r0, r1), N * Ho * Wo, Cout * taps * Cin)
    return out
