"""Tensor-level wrappers over the C-ABI (mmvid_amd/_lib.py).  PyTorch here is plumbing only: it owns the
device memory and the stream; every computation below runs in the hand-written HIP kernels.

All tensors must live on a HIP device and be contiguous (strided views are passed through explicit ld
arguments where a kernel supports them)."""
import ctypes

import torch

from . import _lib
from ._lib import call

bf16, f32, i64 = torch.bfloat16, torch.float32, torch.int64


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def capture_graph(fn):
    """fn() recorded as a hipGraph on a side stream (nothing runs; whatever fn launches must have run eagerly before, so that every
    kernel variant is loaded) -> the torch.cuda.CUDAGraph to replay on the current stream."""
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    return g


_DET_WS = {}  # (operator, device, bytes) -> uint8 workspace of a deterministic form, cached per shape


def _det_ws(op, device, nbytes):
    """The workspace of a `_det` entry point.  One buffer per (operator, size): launches are stream-ordered and every form
    overwrites its workspace before reading it.  First use allocates -- during the warm-up steps that precede a capture
    (engine.GraphedStep), never inside one."""
    key = (op, str(device), int(nbytes))
    ws = _DET_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MMVIDError(f'{op}: the deterministic workspace ({nbytes} bytes) would be allocated inside a graph capture: '
                                  'run the step once in deterministic mode before capturing it')
        ws = _DET_WS[key] = torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)
    return ws


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise _lib.MMVIDError(f'{name}: tensor is on {t.device}; the MMVID kernels run on an MI355X only (no CPU path)')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: tensor must be contiguous')
    return t


# ------------------------------------------------------------------------------------------------ VQ
def vq_sqnorm(codebook):
    _chk(codebook, f32, 'codebook')
    ee = torch.empty(codebook.shape[0], device=codebook.device, dtype=f32)
    call('mmvid_vq_sqnorm', _p(codebook), codebook.shape[0], codebook.shape[1], _p(ee), _stream())
    return ee


def vq_argmin(z, codebook, ee=None, return_dmin=False):
    """z [rows, 256] f32, codebook [n, 256] f32 -> idx int64 [rows] (first argmin of the reference expression)."""
    _chk(z, f32, 'z'), _chk(codebook, f32, 'codebook')
    if ee is None:
        ee = vq_sqnorm(codebook)
    rows = z.shape[0]
    idx = torch.empty(rows, device=z.device, dtype=i64)
    dmin = torch.empty(rows, device=z.device, dtype=f32) if return_dmin else None
    if rows == 0:
        return (idx, dmin) if return_dmin else idx
    call('mmvid_vq_argmin_l2', _p(z), _p(codebook), _p(ee), rows, codebook.shape[0], codebook.shape[1], _p(idx),
         _p(dmin), _stream())
    return (idx, dmin) if return_dmin else idx


def gather_rows(table, idx, out_dtype=f32):
    _chk(table, f32, 'table'), _chk(idx, i64, 'idx')
    rows, dim = idx.numel(), table.shape[1]
    out = torch.empty(*idx.shape, dim, device=table.device, dtype=out_dtype)
    call('mmvid_gather_rows', _p(table), table.shape[0], _p(idx), rows, dim, _p(out) if out_dtype == f32 else None,
         _p(out) if out_dtype == bf16 else None, _stream())
    return out


def frames_u8_to_f32(frames_u8, out=None):
    """[N, H, W, 3] uint8 (decoder layout) -> [N, 3, H, W] f32 = u8 / 255 (the division of ToTensor / data._load_frame, bit for bit)."""
    _chk(frames_u8, torch.uint8, 'frames_u8')
    N, H, W, C = frames_u8.shape
    assert C == 3, f'frames_u8: expected [N, H, W, 3], got {tuple(frames_u8.shape)}'
    if out is None:
        out = torch.empty(N, 3, H, W, device=frames_u8.device, dtype=f32)
    assert out.shape == (N, 3, H, W) and out.dtype == f32 and out.is_contiguous()
    call('mmvid_frames_u8_to_f32', _p(frames_u8), N, H, W, _p(out), _stream())
    return out


def frames_to_u8(img, out=None):
    """[N, 3, H, W] f32 (what vae.decode returns) -> [N, H, W, 3] uint8 = trunc(clamp(x, 0, 1) * 255): the quantisation of
    data.save_image_tensor (utils_html.py:157-186) bit for bit, NaN -> 0.  H * W must be a multiple of 4."""
    _chk(img, f32, 'img')
    N, C, H, W = img.shape
    assert C == 3, f'img: expected [N, 3, H, W], got {tuple(img.shape)}'
    if out is None:
        out = torch.empty(N, H, W, 3, device=img.device, dtype=torch.uint8)
    _chk(out, torch.uint8, 'out')
    assert out.shape == (N, H, W, 3)
    call('mmvid_frames_to_u8', _p(img), N, H, W, _p(out), _stream())
    return out


def frames_paste_u8(img, real, given, out=None):
    """frames_to_u8 with the known pixels pasted over their reconstruction: img [N, 3, H, W] f32, real [N, H, W, 3] uint8, given
    [N, h, w] uint8 (non-zero = the token's patch is known) -> [N, H, W, 3] uint8 = given[token of the pixel] ? real : q(img).
    Needs H % h == 0, W % w == 0 and (W / w) % 4 == 0."""
    _chk(img, f32, 'img'), _chk(real, torch.uint8, 'real'), _chk(given, torch.uint8, 'given')
    N, C, H, W = img.shape
    assert C == 3, f'img: expected [N, 3, H, W], got {tuple(img.shape)}'
    assert tuple(real.shape) == (N, H, W, 3), f'real: expected {(N, H, W, 3)}, got {tuple(real.shape)}'
    assert given.dim() == 3 and given.shape[0] == N, f'given: expected [{N}, h, w], got {tuple(given.shape)}'
    if out is None:
        out = torch.empty(N, H, W, 3, device=img.device, dtype=torch.uint8)
    _chk(out, torch.uint8, 'out')
    assert out.shape == (N, H, W, 3)
    call('mmvid_frames_paste_u8', _p(img), _p(real), _p(given), N, H, W, given.shape[1], given.shape[2], _p(out), _stream())
    return out


def token_rows_gather(table, frame_index):
    """table [F, n] uint16 on the device (TokenCache.to_device), frame_index [B, T] int64 -> target [B, T*n] int64.  An index
    outside [0, F) reads row 0 and is counted (_lib.check_device_faults)."""
    _chk(table, torch.uint16, 'table'), _chk(frame_index, i64, 'frame_index')
    n = table.shape[1]
    out = torch.empty(*frame_index.shape[:-1], frame_index.shape[-1] * n, device=table.device, dtype=i64)
    call('mmvid_token_rows_gather', _p(table), table.shape[0], _p(frame_index), frame_index.numel(), n, _p(out), _stream())
    return out


# ---------------------------------------------------------------------------------------------- GEMM
def gemm(A, B, *, a_kmajor=False, b_kmajor=False, bias=None, residual=None, dact_pre=None, save_pre=None, act=0,
         out_dtype=bf16, out=None, accumulate=False, splitk=1, alpha=1.0, colsum=None):
    """C[m,n] = sum_k A(m,k) B(n,k).  A: [M,K] (or [K,M] when a_kmajor), B: [N,K] (or [K,N] when b_kmajor), 2-D
    bf16; or 3-D batched with identical leading batch size."""
    _chk(A, bf16, 'A'), _chk(B, bf16, 'B')
    batch = 1
    sA = sB = 0
    if A.dim() == 3:
        batch = A.shape[0]
        sA, sB = A.stride(0), B.stride(0)
        A2, B2 = A[0], B[0]
    else:
        A2, B2 = A, B
    K, M = (A2.shape if a_kmajor else A2.shape[::-1])
    Kb, N = (B2.shape if b_kmajor else B2.shape[::-1])
    assert K == Kb, (A.shape, B.shape)
    if out is None:
        shape = (batch, M, N) if A.dim() == 3 else (M, N)
        out = torch.empty(shape, device=A.device, dtype=out_dtype)
    sC = M * N if batch > 1 else 0
    is32 = out.dtype == f32
    for t, n in ((bias, 'bias'), (residual, 'residual')):
        if t is not None:
            _chk(t, f32, n)
    if _lib.is_deterministic() and (colsum is not None or splitk > 1):  # the two fp32 atomic sums of this GEMM, in a fixed order
        nb = _lib.load().mmvid_gemm_bf16_det_workspace_bytes(M, N, splitk, int(colsum is not None))
        ws = _det_ws('gemm_bf16', A.device, nb)
        call('mmvid_gemm_bf16_det', int(a_kmajor), int(b_kmajor), M, N, K, _p(A), A2.stride(0), _p(B), B2.stride(0), batch,
             sA, sB, sC, splitk, float(alpha), _p(bias), _p(residual), N, _p(dact_pre), _p(save_pre), N, act,
             int(accumulate), _p(out) if is32 else None, None if is32 else _p(out), N, _p(colsum), _p(ws), ws.numel(), _stream())
        return out
    call('mmvid_gemm_bf16', int(a_kmajor), int(b_kmajor), M, N, K, _p(A), A2.stride(0), _p(B), B2.stride(0), batch,
         sA, sB, sC, splitk, float(alpha), _p(bias), _p(residual), N, _p(dact_pre), _p(save_pre), N, act,
         int(accumulate), _p(out) if is32 else None, None if is32 else _p(out), N, _p(colsum), _stream())
    return out


def gemm_dw(dY, X, dW, accumulate=True, splitk=None):
    """dW[N,K] (+)= dY[M,N]^T X[M,K] (weight gradient), deterministic split-K through a scratch workspace."""
    _chk(dY, bf16, 'dY'), _chk(X, bf16, 'X'), _chk(dW, f32, 'dW')
    M, N = dY.shape
    K = X.shape[1]
    if splitk is None:
        splitk = _lib.load().mmvid_gemm_dw_pick_splitk(M, N, K)
    ws = torch.empty(splitk * N * K, device=dY.device, dtype=f32) if splitk > 1 else None
    call('mmvid_gemm_bf16_dw', M, N, K, _p(dY), N, _p(X), K, splitk, _p(ws), _p(dW), int(accumulate), _stream())
    return dW


def gemm_dw_grouped(dY, X, dWs, accumulate=True):
    """dWs[g][N,K] (+)= dY[g]^T X[g] for all groups in one launch, no split-K (the tower backward's weight gradients of all layers of
    a kind).  dY [G,M,N], X [G,M,K] bf16, contiguous; dWs: list of G fp32 [N,K] tensors or None (skipped)."""
    _chk(dY, bf16, 'dY'), _chk(X, bf16, 'X')
    G, M, N = dY.shape
    K = X.shape[2]
    assert X.shape[:2] == (G, M) and len(dWs) == G
    ptrs = (ctypes.c_void_p * G)(*[(_chk(w, f32, 'dW').data_ptr() if w is not None else None) for w in dWs])
    call('mmvid_gemm_bf16_dw_grouped', M, N, K, _p(dY), dY.stride(1), dY.stride(0), _p(X), X.stride(1), X.stride(0), G, ptrs,
         int(accumulate), _stream())
    return dWs


def _dw_kinds(kinds):
    """[(dY [G,M,N], X [G,M,K], [dW or None] * G)] -> (mmvid_dw_kind_t array, keep-alive list, M, G)."""
    arr = (_lib.DwKind * len(kinds))()
    keep = []
    G, M = kinds[0][0].shape[:2]
    for a, (dY, X, dWs) in zip(arr, kinds):
        _chk(dY, bf16, 'dY'), _chk(X, bf16, 'X')
        assert dY.shape[:2] == (G, M) and X.shape[:2] == (G, M) and len(dWs) == G
        ptrs = (ctypes.c_void_p * G)(*[(_chk(w, f32, 'dW').data_ptr() if w is not None else None) for w in dWs])
        keep.append(ptrs)
        a.N, a.K, a.dY, a.ldy, a.strideY = dY.shape[2], X.shape[2], dY.data_ptr(), dY.stride(1), dY.stride(0)
        a.X, a.ldx, a.strideX, a.dW_list = X.data_ptr(), X.stride(1), X.stride(0), ctypes.cast(ptrs, ctypes.c_void_p)
    return arr, keep, M, G


def gemm_dw_multi(kinds, accumulate=True):
    """Weight gradients of several Linear shapes x several layers in one launch: kinds = [(dY [G,M,N_k], X [G,M,K_k], [dW [N_k,K_k]
    fp32 or None] * G)], at most 4 kinds.  dW (+)= dY[g]^T X[g]."""
    arr, keep, M, G = _dw_kinds(kinds)
    call('mmvid_gemm_bf16_dw_multi', M, len(kinds), arr, G, int(accumulate), _stream())


def gemm_dw_multi_fill(shapes, groups):
    """[(N, K)] -> share of the chip one grouped launch of those weight gradients x `groups` layers keeps busy (host-side policy)."""
    arr = (_lib.DwKind * len(shapes))()
    for a, (N, K) in zip(arr, shapes):
        a.N, a.K, a.dW_list = N, K, None
    return _lib.load().mmvid_gemm_dw_multi_fill(len(shapes), arr, groups)


def gemm_f32(A, B, *, b_kmajor=False, bias=None, residual=None, alpha=1.0):
    """Exact-fp32 GEMM (k-ordered fmaf chains on the f32 matrix pipe): C = alpha * A @ (B if b_kmajor else B^T).
    A [M,K] f32; B [N,K] (row-major) or [K,N] (b_kmajor)."""
    _chk(A, f32, 'A'), _chk(B, f32, 'B')
    M, K = A.shape
    N = B.shape[1] if b_kmajor else B.shape[0]
    out = torch.empty(M, N, device=A.device, dtype=f32)
    call('mmvid_gemm_f32', int(b_kmajor), M, N, K, _p(A), K, _p(B), B.shape[1], 1, 0, 0, 0, float(alpha), _p(bias),
         _p(residual), _p(out), N, _stream())
    return out


# ---------------------------------------------------------------------------------------------- norms
def layernorm_fwd(x, w, b, eps=1e-5, out_dtype=bf16, save_stats=True):
    _chk(x, f32, 'x')
    rows, E = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    mean = torch.empty(rows, device=x.device, dtype=f32) if save_stats else None
    rstd = torch.empty(rows, device=x.device, dtype=f32) if save_stats else None
    call('mmvid_layernorm_fwd', _p(x), E, rows, E, _p(w), _p(b), float(eps), _p(y) if out_dtype == bf16 else None,
         _p(y) if out_dtype == f32 else None, E, _p(mean), _p(rstd), _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, w, dx=None, add=False, dw=None, db=None, dx_colsum=None, workspace=None):
    """workspace (fp32, >= 3*E*64 elements): two-stage deterministic reduction of dw / db / dx_colsum instead of atomics."""
    _chk(dy, f32, 'dy'), _chk(x, f32, 'x')
    rows, E = x.numel() // x.shape[-1], x.shape[-1]
    if dx is None:
        dx = torch.empty_like(x)
        add = False
    if workspace is None and _lib.is_deterministic() and (dw is not None or db is not None or dx_colsum is not None):
        workspace = _det_ws('layernorm_bwd', x.device, 512 * 3 * E * 4).view(f32)  # (the library refuses the atomic branch in this mode)
    call('mmvid_layernorm_bwd_ws', _p(dy), E, _p(x), E, _p(mean), _p(rstd), _p(w), rows, E, _p(dx), E, int(add), None,
         _p(dw), _p(db), _p(dx_colsum), _p(workspace), workspace.numel() if workspace is not None else 0, _stream())
    return dx


def layernorm_bwd_partial(dy, x, mean, rstd, w, workspace, dx=None, add=False, dx_bf16=None, want=(True, True, True)):
    """Stage 1 of the LayerNorm backward: dx (added into `dx` when add) and the partial rows of dw / db / colsum(dx) in `workspace`
    (fp32, this call's own, >= 64 * 3 * E floats).  dy fp32 or bf16.  Returns (dx, blocks)."""
    _chk(x, f32, 'x'), _chk(workspace, f32, 'workspace')
    rows, E = x.numel() // x.shape[-1], x.shape[-1]
    if dx is None:
        dx, add = torch.empty_like(x), False
    nb = ctypes.c_int()
    call('mmvid_layernorm_bwd_partial', _p(dy), int(dy.dtype == bf16), E, _p(x), E, _p(mean), _p(rstd), _p(w), rows, E, _p(dx), E, int(add),
         _p(dx_bf16), int(want[0]), int(want[1]), int(want[2]), _p(workspace), workspace.numel(), ctypes.byref(nb), _stream())
    return dx, nb.value


def layernorm_bwd_reduce_multi(items, blocks, E):
    """items: [(workspace, dw or None, db or None, dx_colsum or None)] -> targets += column sums of each workspace's partial rows."""
    arr = (_lib.LnReduce * len(items))()
    for a, (ws, dw, db, cs) in zip(arr, items):
        a.partial, a.dw, a.db, a.dx_colsum = ws.data_ptr(), _p(dw), _p(db), _p(cs)
    call('mmvid_layernorm_bwd_reduce_multi', len(items), arr, blocks, E, _stream())


def gn_stats_floats(N, hw, C):
    """Size of a GroupNorm statistics area: [N][C][2] per-channel pairs, then partial sums [N][blocks][32][2] (blocks of 128 pixels,
    or of 64 for the strip convolution: sized for the finer one).  The one statement of the layout on the Python side, with
    _gn_stats_partials; csrc/common.h has the C side."""
    return N * (2 * C + 64 * ((hw + 63) // 64))


def _gn_stats_partials(stats, N, C):
    """Pointer to the partial sums of a statistics area for N images of C channels (None without an area)."""
    return ctypes.c_void_p(stats.data_ptr() + N * C * 2 * 4) if stats is not None else None


def gn_stats_buffer(N, hw, C, device):
    """fp32 scratch of mmvid_groupnorm_swish_nhwc (gn_stats_floats)."""
    return torch.empty(gn_stats_floats(N, hw, C), device=device, dtype=f32)


def conv3x3_strip(x, w, bias, residual=None, out_dtype=bf16, also_bf16=False, gn_stats=None):
    """3x3 / stride 1 / pad 1 on NHWC bf16 in strip form (csrc/conv_strip.hip).  x [N,H,W,Cin], w [Cout,9,Cin] bf16.
    Returns out (and a bf16 copy when out is fp32 and also_bf16).  gn_stats: a gn_stats_buffer (partials per 64 pixels)."""
    _chk(x, bf16, 'x'), _chk(w, bf16, 'w')
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    out = torch.empty(N, H, W, Cout, device=x.device, dtype=out_dtype)
    o16 = torch.empty(N, H, W, Cout, device=x.device, dtype=bf16) if (also_bf16 and out_dtype == f32) else None
    rb = residual if (residual is not None and residual.dtype == bf16) else None
    rf = residual if (residual is not None and residual.dtype == f32) else None
    call('mmvid_conv3x3_strip_nhwc', _p(x), N, H, W, Cin, _p(w), _p(bias), Cout, _p(rb), _p(rf),
         _p(out) if out_dtype == bf16 else _p(o16), _p(out) if out_dtype == f32 else None, _gn_stats_partials(gn_stats, N, Cout), _stream())
    return (out, o16) if o16 is not None else out


def groupnorm_swish(x, w, b, eps=1e-6, swish=True, out_dtype=bf16, stats=None, stats_block=128):
    """x NHWC [N,H,W,C] bf16 or f32 -> same shape.  `stats`: a gn_stats_buffer whose partial sums were already
    written by the convolution that produced x (conv2d_nhwc(..., gn_stats=...))."""
    N, H, W, C = x.shape
    assert x.is_contiguous() and x.dtype in (bf16, f32)
    blocks = 0
    if stats is None:
        stats = gn_stats_buffer(N, H * W, C, x.device)
    else:
        assert (H * W) % stats_block == 0
        blocks = H * W // stats_block
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    call('mmvid_groupnorm_swish_nhwc', _p(x), int(x.dtype == bf16), N, H * W, C, _p(w), _p(b), float(eps), int(swish),
         _p(stats), blocks, _p(y) if out_dtype == bf16 else None, _p(y) if out_dtype == f32 else None, _stream())
    return y


# ------------------------------------------------------------------------------------------ attention
def _mask_args(mask):
    """mask: None | 'causal' | ('rows', [(row, first_allowed_col), ...])."""
    if mask is None:
        return 0, -1, 0, -1, 0
    if mask == 'causal':
        return 1, -1, 0, -1, 0
    kind, rows = mask
    assert kind == 'rows' and len(rows) <= 2
    rows = list(rows) + [(-1, 0)] * (2 - len(rows))
    return 2, rows[0][0], rows[0][1], rows[1][0], rows[1][1]


def attention_fwd(qkv, B, L, H, mask=None, scale=0.125):
    """qkv [B*L, 3E] bf16 -> (out [B*L, E] bf16, lse2 [B,H,L] f32)."""
    _chk(qkv, bf16, 'qkv')
    E = H * 64
    out = torch.empty(B * L, E, device=qkv.device, dtype=bf16)
    lse2 = torch.empty(B, H, L, device=qkv.device, dtype=f32)
    call('mmvid_attention_fwd', _p(qkv), 3 * E, B, L, H, E, float(scale), *_mask_args(mask), _p(out), E, _p(lse2),
         _stream())
    return out, lse2


def attention_bwd(qkv, out, dout, lse2, B, L, H, mask=None, scale=0.125, dbias=None):
    """-> dqkv [B*L, 3E] bf16; dbias [3E] f32 (optional) += its column sums."""
    E = H * 64
    delta = torch.empty(B, H, L, device=qkv.device, dtype=f32)
    dqkv = torch.empty_like(qkv)
    if dbias is not None and _lib.is_deterministic():
        ws = _det_ws('attention_bwd_bias', qkv.device, _lib.load().mmvid_attention_bwd_bias_det_workspace_bytes(B, L, E))
        call('mmvid_attention_bwd_bias_det', _p(qkv), 3 * E, _p(out), E, _p(dout), E, _p(lse2), _p(delta), B, L, H, E, float(scale),
             *_mask_args(mask), _p(dqkv), 3 * E, _p(dbias), _p(ws), ws.numel(), _stream())
        return dqkv
    call('mmvid_attention_bwd_bias', _p(qkv), 3 * E, _p(out), E, _p(dout), E, _p(lse2), _p(delta), B, L, H, E, float(scale),
         *_mask_args(mask), _p(dqkv), 3 * E, _p(dbias) if dbias is not None else None, _stream())
    return dqkv


# --------------------------------------------------------------------------------- sequence / losses
def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else 0 for t in tensors])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def assemble_sequence(tables, ids, seg, pos):
    """x[b,l,:] = tables[seg[l]][ids[b,l]] + pos[l].  tables: list of [V_i, E] f32; ids [B,L] i64; seg [L] i32."""
    B, L = ids.shape
    E = pos.shape[-1]
    for t in tables:
        _chk(t, f32, 'table')
    _chk(ids, i64, 'ids'), _chk(pos, f32, 'pos')
    assert seg.dtype == torch.int32 and seg.is_cuda
    out = torch.empty(B, L, E, device=ids.device, dtype=f32)
    tp, keep = _ptr_array(tables)
    rows = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
    call('mmvid_assemble_sequence', tp, rows, len(tables), _p(ids), _p(seg), _p(pos), B, L, E, _p(out), _stream())
    return out


def assemble_sequence_bwd(grad_tables, table_rows, ids, seg, dx, dpos=None, accumulate_dpos=False):
    B, L = ids.shape
    E = dx.shape[-1]
    _chk(dx, f32, 'dx')
    tp, keep = _ptr_array(grad_tables)
    rows = (ctypes.c_int64 * len(grad_tables))(*table_rows)
    if _lib.is_deterministic():  # inverted index + two-level fixed-order sums instead of the atomic scatter
        nb = _lib.load().mmvid_assemble_sequence_bwd_det_workspace_bytes(B, L, E, len(grad_tables), rows)
        if nb < 0:
            raise _lib.MMVIDError('assemble_sequence_bwd: tables / batch too large for the deterministic form (2^31 destinations)')
        ws = _det_ws('assemble_sequence_bwd', dx.device, nb)
        call('mmvid_assemble_sequence_bwd_det', tp, rows, len(grad_tables), _p(ids), _p(seg), _p(dx), B, L, E, _p(dpos),
             int(accumulate_dpos), _p(ws), ws.numel(), _stream())
        return
    call('mmvid_assemble_sequence_bwd', tp, rows, len(grad_tables), _p(ids), _p(seg), _p(dx), B, L, E, _p(dpos),
         int(accumulate_dpos), _stream())


def cross_entropy_fwd(logits, target, select):
    """Returns (lse [rows], loss_sum [1]) over rows with select != 0 (select uint8 or None)."""
    _chk(logits, f32, 'logits'), _chk(target, i64, 'target')
    rows, V = logits.shape
    lse = torch.empty(rows, device=logits.device, dtype=f32)
    loss = torch.zeros(1, device=logits.device, dtype=f32)
    if _lib.is_deterministic():
        ws = _det_ws('cross_entropy_fwd', logits.device, rows * 4)
        call('mmvid_cross_entropy_fwd_det', _p(logits), V, _p(target), _p(select), rows, V, _p(lse), _p(loss), _p(ws), ws.numel(),
             _stream())
        return lse, loss
    call('mmvid_cross_entropy_fwd', _p(logits), V, _p(target), _p(select), rows, V, _p(lse), _p(loss), _stream())
    return lse, loss


def cross_entropy_bwd(logits, target, select, lse, gscale):
    rows, V = logits.shape
    d = torch.empty(rows, V, device=logits.device, dtype=bf16)
    call('mmvid_cross_entropy_bwd', _p(logits), V, _p(target), _p(select), _p(lse), _p(gscale), rows, V, _p(d), V,
         _stream())
    return d


def colsum_bf16(dy, db):
    M, N = dy.shape
    if _lib.is_deterministic():
        ws = _det_ws('colsum_bf16', dy.device, _lib.load().mmvid_colsum_bf16_det_workspace_bytes(M, N))
        call('mmvid_colsum_bf16_det', _p(dy), N, M, N, _p(db), _p(ws), ws.numel(), _stream())
        return
    call('mmvid_colsum_bf16', _p(dy), N, M, N, _p(db), _stream())


# ------------------------------------------------------------------------------------------ optimiser
def _lazy_args(lazy):
    """lazy = (row_flags uint8 [rows], table_lo, rows, rowlen), or None for no table: the four arguments every entry takes for it."""
    fl, lo, rows, rowlen = lazy if lazy is not None else (None, 0, 0, 0)
    return (None if fl is None else _p(_chk(fl, torch.uint8, 'row_flags'))), int(lo), int(rows), int(rowlen)


def grad_sqnorm(g, out, partials=None, lazy=None):
    """out[0] += sum g^2.  With `partials` (fp32 [2048] scratch) the reduction order is fixed (deterministic).
    lazy (_lazy_args): skip the rows of that table whose flag is 0 (they are all-zero)."""
    _chk(g, f32, 'g'), _chk(out, f32, 'out')
    if lazy is not None:
        assert partials is not None
        call('mmvid_grad_sqnorm_rows', _p(g), g.numel(), _p(partials), _p(out), *_lazy_args(lazy), _stream())
    elif partials is not None:
        call('mmvid_grad_sqnorm_det', _p(g), g.numel(), _p(partials), _p(out), _stream())
    else:
        call('mmvid_grad_sqnorm', _p(g), g.numel(), _p(out), _stream())


def adam_step(p, g, m, v, shadow, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.0,
              sqnorm=None, grad_scale=1.0, step_dev=None, lr_dev=None, lazy=None, skip_dev=None, decoupled=False):
    """skip_dev: the verdict of step_guard (int32 on the device) -- where it is non-zero at execution the kernel writes nothing
    (mmvid_adam_step_guarded).  None: the unguarded entry, as ever.  decoupled: torch.optim.AdamW's rule -- the decay scales the
    weight by 1 - lr * weight_decay and stays out of the gradient (mmvid_adam_step_decoupled; skip_dev may be None)."""
    for t, n in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
        _chk(t, f32, n)
    args = (_p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), float(lr), _p(lr_dev), float(betas[0]), float(betas[1]), float(eps),
            float(weight_decay), int(step), _p(step_dev), float(max_norm), _p(sqnorm), float(grad_scale), *_lazy_args(lazy))
    if decoupled:
        if not 0.0 <= float(weight_decay) < float('inf'):  # (NaN: False)
            raise ValueError(f'adam_step: decoupled weight_decay={weight_decay!r} must be finite and >= 0')
        call('mmvid_adam_step_decoupled', *args, None if skip_dev is None else _p(_chk(skip_dev, torch.int32, 'skip_dev')), _stream())
    elif skip_dev is None:
        call('mmvid_adam_step_rows', *args, _stream())
    else:
        call('mmvid_adam_step_guarded', *args, _p(_chk(skip_dev, torch.int32, 'skip_dev')), _stream())


def ema_update(ema, p, decay, warmup, step, step_dev=None, lazy=None, skip_dev=None):
    """ema <- fmaf(1 - d, p - ema, ema) over the flat fp32 buffers, d = decay or (warmup) min(decay, (1 + t) / (10 + t)) with t the
    count of finished steps (`step`, or the device scalar step_dev); lazy as in adam_step: unflagged rows are not touched
    (include/mmvid_hip_ext.h: mmvid_ema_update).  skip_dev as in adam_step (mmvid_ema_update_guarded)."""
    _chk(ema, f32, 'ema'), _chk(p, f32, 'p')
    if ema.numel() != p.numel():
        raise ValueError(f'ema_update: ema has {ema.numel()} elements, p {p.numel()}')
    args = (_p(ema), _p(p), p.numel(), float(decay), int(bool(warmup)), int(step), _p(step_dev), *_lazy_args(lazy))
    if skip_dev is None:
        call('mmvid_ema_update', *args, _stream())
    else:
        call('mmvid_ema_update_guarded', *args, _p(_chk(skip_dev, torch.int32, 'skip_dev')), _stream())


TELEMETRY_CHUNK = _lib.HEADER.constants['MMVID_TELEMETRY_CHUNK']  # elements of one chunk of a segment (include/mmvid_hip.h)


def telemetry_plan(offsets, numels, chunk=TELEMETRY_CHUNK):
    """The tables of mmvid_segment_stats for the segments [offsets[s], offsets[s] + numels[s]) of a flat buffer: (seg_off, seg_len,
    seg_chunk0, chunks) -- three lists of ints, one entry per segment, and the total number of chunks.  Segment s is cut into
    ceil(numels[s] / chunk) chunks, numbered from seg_chunk0[s] on; what lies between two segments is in no chunk.  Pure host code."""
    offsets, numels, chunk = [int(o) for o in offsets], [int(n) for n in numels], int(chunk)
    if len(offsets) != len(numels) or not offsets:
        raise ValueError(f'telemetry_plan: {len(offsets)} offsets for {len(numels)} lengths (at least one segment)')
    if chunk < 1 or any(n < 1 for n in numels) or any(o < 0 for o in offsets):
        raise ValueError('telemetry_plan: the chunk and every length must be >= 1, every offset >= 0')
    if any(offsets[s] + numels[s] > offsets[s + 1] for s in range(len(offsets) - 1)):
        raise ValueError('telemetry_plan: the segments must be ascending and must not overlap')
    chunk0, total = [], 0
    for n in numels:
        chunk0.append(total)
        total += (n + chunk - 1) // chunk
    return offsets, numels, chunk0, total


def segment_stats(g, p, m, v, tables, chunks, step, lr, betas, eps, every, slots, count, partials_f, partials_i, ring_f, ring_i, head_i,
                  head_f, step_dev=None, lr_dev=None, lazy=None, skip_dev=None):
    """One telemetry record (include/mmvid_hip_ext.h: mmvid_segment_stats): per segment of the flat buffers sum g^2, max |g| and the
    count of non-finite g, sum p^2 and the sum of squares of the update Adam just applied, into slot (count / every) % slots of the
    ring -- or, where count % every != 0, nothing; count (int32 on the device) advances either way.  tables = (seg_off, seg_len,
    seg_chunk0), int64 on the device, as telemetry_plan lays them out; step_dev, lr_dev, lazy and skip_dev are what adam_step got."""
    for t, n in ((g, 'g'), (p, 'p'), (m, 'm'), (v, 'v'), (partials_f, 'partials_f'), (ring_f, 'ring_f'), (head_f, 'head_f')):
        _chk(t, f32, n)
    for t, n in ((count, 'count'), (partials_i, 'partials_i'), (ring_i, 'ring_i'), (head_i, 'head_i')):
        _chk(t, torch.int32, n)
    off, ln, c0 = (_chk(t, i64, 'segment table') for t in tables)
    S = off.numel()
    if not (g.numel() == m.numel() == v.numel() == p.numel()) or ln.numel() != S or c0.numel() != S:
        raise ValueError('segment_stats: g, p, m, v must have one size and the three tables one length')
    if (partials_f.numel() < 4 * chunks or partials_i.numel() < 2 * chunks or ring_f.numel() != slots * S * 4 or ring_i.numel() != slots * S * 2
            or head_i.numel() != slots * 4 or head_f.numel() != slots * 2 or count.numel() < 1):
        raise ValueError(f'segment_stats: buffers do not fit {S} segments, {chunks} chunks and {slots} slots')
    if skip_dev is not None:
        _chk(skip_dev, torch.int32, 'skip_dev')
    call('mmvid_segment_stats', _p(g), _p(p), _p(m), _p(v), p.numel(), _p(off), _p(ln), _p(c0), S, int(chunks), float(lr), _p(lr_dev),
         float(betas[0]), float(betas[1]), float(eps), int(step), _p(step_dev), *_lazy_args(lazy), _p(skip_dev),
         int(every), int(slots), _p(count), _p(partials_f), _p(partials_i), _p(ring_f), _p(ring_i), _p(head_i), _p(head_f), _stream())


def step_guard(sqnorm, grad_scale, step_dev, guard_i, guard_f):
    """The non-finite guard's verdict on the device (include/mmvid_hip_ext.h: mmvid_step_guard): guard_i (int32 [4]) = skip, skipped,
    run, seen; guard_f (fp32 [2]) = gradient norm, last finite gradient norm; step_dev advances only where the step is applied."""
    _chk(sqnorm, f32, 'sqnorm'), _chk(step_dev, f32, 'step_dev'), _chk(guard_f, f32, 'guard_f'), _chk(guard_i, torch.int32, 'guard_i')
    if guard_i.numel() != 4 or guard_f.numel() != 2 or sqnorm.numel() < 1 or step_dev.numel() < 1:
        raise ValueError('step_guard: guard_i holds 4 int32, guard_f 2 fp32, sqnorm and step_dev one fp32 each')
    call('mmvid_step_guard', _p(sqnorm), float(grad_scale), _p(step_dev), _p(guard_i), _p(guard_f), _stream())


def lr_schedule(step_dev, kind, lr_min, lr_max, warmup, every, lr_out):
    call('mmvid_lr_schedule', _p(step_dev), int(kind), float(lr_min), float(lr_max), int(warmup), int(every), _p(lr_out),
         _stream())


LR_STEP, LR_COSINE, LR_WARMUP_DECAY = 2, 3, 4  # the kinds of mmvid_lr_schedule_ext (0 constant and 1 WarmupLR: mmvid_lr_schedule)


def lr_schedule_ext(step_dev, kind, lr_min, lr_max, every, a, b, gamma, lr_out):
    """lr_out[0] <- the closed-form schedule `kind` at the device step count (include/mmvid_hip_ext.h: mmvid_lr_schedule_ext):
    2 StepLR(step_size=a, gamma), 3 CosineAnnealingLR(T_max=a, eta_min=lr_min), 4 WarmupDecayLR(total=b, warmup=a)."""
    _chk(step_dev, f32, 'step_dev'), _chk(lr_out, f32, 'lr_out')
    if step_dev.numel() < 1 or lr_out.numel() < 1:
        raise ValueError('lr_schedule_ext: step_dev and lr_out hold one fp32 each')
    call('mmvid_lr_schedule_ext', _p(step_dev), int(kind), float(lr_min), float(lr_max), int(every), int(a), int(b), float(gamma),
         _p(lr_out), _stream())


def lr_plateau(loss_dev, step_dev, every, factor, patience, cooldown, threshold, min_lr, eps, state_f, state_i, skip_dev=None):
    """One scheduler step of ReduceLROnPlateau(mode='min', threshold_mode='rel') on the device (include/mmvid_hip_ext.h:
    mmvid_lr_plateau): state_f (fp32 [2]) = lr, best; state_i (int32 [3]) = bad epochs, cool-down left, reductions.  After the
    optimiser; it does nothing where skip_dev says the step was skipped or the step count is no multiple of `every`."""
    _chk(loss_dev, f32, 'loss_dev'), _chk(step_dev, f32, 'step_dev'), _chk(state_f, f32, 'state_f'), _chk(state_i, torch.int32, 'state_i')
    if loss_dev.numel() != 1 or step_dev.numel() < 1 or state_f.numel() != 2 or state_i.numel() != 3:
        raise ValueError('lr_plateau: loss_dev and step_dev hold one fp32 each, state_f 2 fp32, state_i 3 int32')
    call('mmvid_lr_plateau', _p(loss_dev), _p(step_dev), int(every), float(factor), int(patience), int(cooldown), float(threshold),
         float(min_lr), float(eps), _p(state_f), _p(state_i), None if skip_dev is None else _p(_chk(skip_dev, torch.int32, 'skip_dev')),
         _stream())


def counter_add(counter, value=1.0):
    call('mmvid_counter_add', _p(counter), float(value), _stream())


def cast_bf16(x, out=None):
    _chk(x, f32, 'x')
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=bf16)
    call('mmvid_cast_f32_to_bf16', _p(x), _p(out), x.numel(), _stream())
    return out


# ---------------------------------------------------------------------------------------------- VQGAN
def conv2d_nhwc(x, w, bias, mode, residual=None, clamp01=False, out_dtype=bf16, gn_stats=None, splitk=1):
    """x [N,H,W,Cin] bf16; w [Cout,taps,Cin] bf16 (taps 9 or 1); mode 0 3x3 | 1 down | 2 up | 3 1x1.
    gn_stats: a gn_stats_buffer for the OUTPUT shape; its partial-sum area is filled by the epilogue.
    splitk > 1: the reduction is cut into that many ranges, added in a fixed order (deep layers on small maps)."""
    _chk(x, bf16, 'x'), _chk(w, bf16, 'w')
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    out = torch.empty(N, Ho, Wo, Cout, device=x.device, dtype=out_dtype)
    rb = residual if (residual is not None and residual.dtype == bf16) else None
    rf = residual if (residual is not None and residual.dtype == f32) else None
    ws = torch.empty(splitk * N * Ho * Wo * Cout, device=x.device, dtype=f32) if splitk > 1 else None
    call('mmvid_conv2d_nhwc_splitk', mode, _p(x), N, H, W, Cin, _p(w), _p(bias), Cout, _p(rb), _p(rf), int(clamp01),
         _p(out) if out_dtype == bf16 else None, _p(out) if out_dtype == f32 else None, _gn_stats_partials(gn_stats, N, Cout), int(splitk), _p(ws),
         _stream())
    return out


# ---- the split operator (vae.strict = 'split'): bf16 pair planes, three products per convolution -------------------------
def split_planes(x):
    """fp32 [...] -> bf16 pair planes [2, ...]: hi = bf16(x), lo = bf16(x - hi)."""
    _chk(x, f32, 'x')
    out = torch.empty((2, ) + tuple(x.shape), device=x.device, dtype=bf16)
    call('mmvid_split_f32_bf16x2', _p(x.contiguous()), x.numel(), _p(out), _stream())
    return out


def split_weights(w):
    """fp32 [Cout, taps, Cin] -> bf16 [Cout, 3, taps, Cin] = (w_hi | w_hi | w_lo)."""
    hi = w.to(bf16)
    lo = (w - hi.float()).to(bf16)
    return torch.stack([hi, hi, lo], 1).contiguous()


def conv2d_nhwc_split3(x_planes, w3, bias, mode, residual=None, clamp01=False, splitk=1, strip=False, planes_out=None):
    """x_planes [2,N,H,W,Cin] bf16, w3 [Cout,3,taps,Cin] bf16 -> fp32 [N,Ho,Wo,Cout] = conv of (x_hi + x_lo) with (w_hi + w_lo)
    without the lo.lo term, fp32 accumulate (mmvid_conv2d_nhwc_split3 / the strip form for mode 0)."""
    _chk(x_planes, bf16, 'x_planes'), _chk(w3, bf16, 'w3')
    _, N, H, W, Cin = x_planes.shape
    Cout = w3.shape[0]
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    out = torch.empty(N, Ho, Wo, Cout, device=x_planes.device, dtype=f32)
    if strip:
        assert mode == 0 and not clamp01 and splitk == 1
        call('mmvid_conv3x3_strip_nhwc_split3', _p(x_planes), N, H, W, Cin, _p(w3), _p(bias), Cout, _p(residual), _p(out), None, _p(planes_out),
             _stream())
        return out
    ws = torch.empty(splitk * N * Ho * Wo * Cout, device=out.device, dtype=f32) if splitk > 1 else None
    call('mmvid_conv2d_nhwc_split3', mode, _p(x_planes), N, H, W, Cin, _p(w3), _p(bias), Cout, _p(residual), int(clamp01), _p(out),
         None, int(splitk), _p(ws), _stream())
    return out


def groupnorm_swish_split(x, w, b, eps=1e-6, swish=True):
    """x NHWC fp32 -> bf16 pair planes [2,N,H,W,C] of GroupNorm(32)(x) [* sigmoid]."""
    _chk(x, f32, 'x')
    N, H, W, C = x.shape
    out = torch.empty(2, N, H, W, C, device=x.device, dtype=bf16)
    st = gn_stats_buffer(N, H * W, C, x.device)
    call('mmvid_groupnorm_swish_nhwc_split', _p(x), N, H * W, C, _p(w), _p(b), float(eps), int(swish), _p(st), 0, _p(out), _stream())
    return out


def groupnorm_swish_f16(x, w, b, eps=1e-6, swish=True):
    """x NHWC fp32 -> fp16 [N,H,W,C] of GroupNorm(32)(x) [* sigmoid] (the input of conv3x3_strip_f16)."""
    _chk(x, f32, 'x')
    N, H, W, C = x.shape
    out = torch.empty(N, H, W, C, device=x.device, dtype=torch.float16)
    st = gn_stats_buffer(N, H * W, C, x.device)
    call('mmvid_groupnorm_swish_nhwc_f16out', _p(x), N, H * W, C, _p(w), _p(b), float(eps), int(swish), _p(st), 0, _p(out), _stream())
    return out


def conv3x3_strip_f16(x, w, bias, residual=None, planes_out=None):
    """x fp16 [N,H,W,Cin], w fp16 [Cout,9,Cin] -> fp32 [N,H,W,Cout]: one product of IEEE-half operands, fp32 accumulate (+ fp32 residual)."""
    _chk(x, torch.float16, 'x'), _chk(w, torch.float16, 'w')
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    out = torch.empty(N, H, W, Cout, device=x.device, dtype=f32)
    call('mmvid_conv3x3_strip_nhwc_f16', _p(x), N, H, W, Cin, _p(w), _p(bias), Cout, _p(residual), _p(out), None, _p(planes_out), _stream())
    return out


def image_to_nhwc8(img):
    _chk(img, f32, 'img')
    N, C, H, W = img.shape
    assert C == 3
    out = torch.empty(N, H, W, 8, device=img.device, dtype=bf16)
    call('mmvid_image_to_nhwc8', _p(img), N, H, W, _p(out), _stream())
    return out


def nhwc_to_nchw(x, c_use=None):
    _chk(x, f32, 'x')
    N, H, W, C = x.shape
    c_use = c_use or C
    out = torch.empty(N, c_use, H, W, device=x.device, dtype=f32)
    call('mmvid_nhwc_to_nchw_f32', _p(x), N, H, W, C, c_use, _p(out), _stream())
    return out


def spatial_attention(q, k, v):
    """q,k,v [N,HW,C] bf16 -> softmax(q k^T C^-0.5) v, bf16."""
    N, HW, C = q.shape
    scratch = torch.empty(N * HW * HW * 3 // 2 + 16, device=q.device, dtype=f32)
    out = torch.empty_like(q)
    call('mmvid_spatial_attention', _p(q), _p(k), _p(v), N, HW, C, float(C)**-0.5, _p(scratch), _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------- samplers
u8 = torch.uint8


def exponential_like(shape, device):
    """Exp(1) race variates for the samplers (what torch.multinomial draws internally), from torch's device generator."""
    return torch.empty(shape, device=device, dtype=f32).exponential_()


VARIATE_PURPOSES = {'tok': 1, 'noise': 2, 'keep': 3}  # token race, token noise, keep race (include/mmvid_hip_ext.h)


def variates_fill(out, seeds, rows_per_video, purpose, kind, draw_first=0, draw_dev=None, substream=None):
    """Seeded race variates into `out` (f32, contiguous): [R, n], or [draws, R, n] for draws draw_first .. draw_first + draws - 1 in one
    launch, R = len(seeds) * rows_per_video rows of which rows_per_video consecutive ones belong to each video.  seeds int64 [videos],
    substream int32 [videos] or None (0), draw_dev an int32 device scalar or None: with it `out` is one draw, number draw_dev +
    draw_first.  purpose 1..3 (VARIATE_PURPOSES), kind 0 = uniform [0, 1), 1 = Exp(1).  The value of (video, index) is a function of
    (seed, substream, purpose, draw, index) alone: include/mmvid_hip_ext.h.  -> out"""
    _chk(out, f32, 'out')
    _chk(seeds, i64, 'seeds')
    if substream is not None:
        _chk(substream, torch.int32, 'substream')
        assert substream.shape == seeds.shape
    if draw_dev is not None:
        _chk(draw_dev, torch.int32, 'draw_dev')
    assert seeds.dim() == 1 and out.dim() in (2, 3) and (out.dim() == 2 or draw_dev is None)
    videos, rpv, n = seeds.shape[0], int(rows_per_video), out.shape[-1]
    draws = out.shape[0] if out.dim() == 3 else 1
    if out.shape[-2] != videos * rpv:
        raise ValueError(f'variates_fill: {out.shape[-2]} rows for {videos} videos of {rpv} rows')
    call('mmvid_variates_fill', _p(seeds), _p(substream), videos, rpv, n, int(purpose), int(kind), _p(draw_dev), int(draw_first), draws,
         _p(out), _stream())
    return out


def sample_race(logits, E, noise_u=None, temperature=0.0, logit_div=1.0, tok_offset=0, want_y=True, tok_out=None, step_dev=None, step0=0):
    """logits [R, V] f32 (row stride = logits.stride(0)), E [R, V] f32 Exp(1) variates -> (tok int64 [R] (tok_out if given), y f32 [R]).
    step_dev (int32 device scalar): E is [draws, R, V] and draw number step_dev - step0 is used (token-only form: want_y False, no noise)."""
    _chk(E, f32, 'E')
    assert logits.dtype == f32 and logits.is_cuda and logits.stride(1) == 1
    R, V = logits.shape
    assert E.shape[-2:] == (R, V) and E.is_contiguous() and (E.dim() == 2 or (E.dim() == 3 and step_dev is not None))
    if tok_out is not None:
        _chk(tok_out, i64, 'tok_out')
        assert tok_out.shape == (R, )
    tok = tok_out if tok_out is not None else torch.empty(R, device=logits.device, dtype=i64)
    y = torch.empty(R, device=logits.device, dtype=f32) if want_y else None
    if noise_u is not None:
        _chk(noise_u, f32, 'noise_u')
    call('mmvid_sample_race_at', _p(logits), logits.stride(0), _p(E), _p(step_dev) if step_dev is not None else None, int(step0), R * V,
         _p(noise_u), float(temperature), float(logit_div), R, V, int(tok_offset), _p(tok), _p(y), _stream())
    return tok, y


def _guided_operands(name, logits_c, logits_u, scale, rows_per_scale):
    """The operand checks of the guided form of `name` (one row stride; one f32 scale per rows_per_scale rows) -> (R, V, int(rows_per_scale))."""
    _chk(scale, f32, 'scale')
    assert all(t.dtype == f32 and t.is_cuda and t.stride(1) == 1 for t in (logits_c, logits_u))
    R, V = logits_c.shape
    if tuple(logits_u.shape) != (R, V) or logits_u.stride(0) != logits_c.stride(0):
        if name in ('logits_truncate', 'logits_truncate_rows'):  # (its `rows` check has taken the shape, and it calls the conditional operand `logits`)
            raise ValueError(f'{name}: logits_u (row stride {logits_u.stride(0)}) must have the row stride of logits ({logits_c.stride(0)})')
        raise ValueError(f'{name}: logits_u {tuple(logits_u.shape)} (row stride {logits_u.stride(0)}) must have the shape and '
                         f'the row stride of logits_c {(R, V)} ({logits_c.stride(0)})')
    rows_per_scale = int(rows_per_scale)
    if rows_per_scale <= 0 or R % rows_per_scale or scale.numel() != R // rows_per_scale:
        raise ValueError(f'{name}: {scale.numel()} scales for R = {R} rows in groups of {rows_per_scale}')
    return R, V, rows_per_scale


def sample_race_guided(logits_c, logits_u, scale, rows_per_scale, E, noise_u=None, temperature=0.0, logit_div=1.0):
    """sample_race on lc + w * (lc - lu) (three rounded fp32 operations, lc == -inf stays -inf), w = scale[r // rows_per_scale]: logits_c,
    logits_u [R, V] f32 with one row stride, scale f32 [R // rows_per_scale] on the device -> (tok int64 [R], y f32 [R])."""
    _chk(E, f32, 'E')
    R, V, rows_per_scale = _guided_operands('sample_race_guided', logits_c, logits_u, scale, rows_per_scale)
    assert E.shape == (R, V) and E.is_contiguous()
    tok, y = torch.empty(R, device=logits_c.device, dtype=i64), torch.empty(R, device=logits_c.device, dtype=f32)
    if noise_u is not None:
        _chk(noise_u, f32, 'noise_u')
    call('mmvid_sample_race_guided', _p(logits_c), _p(logits_u), logits_c.stride(0), _p(scale), rows_per_scale, _p(E), _p(noise_u),
         float(temperature), float(logit_div), R, V, 0, _p(tok), _p(y), _stream())
    return tok, y


def sample_race_guided_at(logits_c, logits_u, scale, rows_per_scale, E, logit_div=1.0, tok_offset=0, tok_out=None, step_dev=None, step0=0):
    """The token-only draw of sample_race (want_y False, no noise; R <= 1024) on the guided value of sample_race_guided: logits_c, logits_u
    [R, V] f32 with one row stride, scale f32 [R // rows_per_scale] on the device, E [R, V], or [draws, R, V] with step_dev (int32 device
    scalar: draw number step_dev - step0 is used) -> tok int64 [R] (tok_out if given)."""
    _chk(E, f32, 'E')
    R, V, rows_per_scale = _guided_operands('sample_race_guided_at', logits_c, logits_u, scale, rows_per_scale)
    assert E.shape[-2:] == (R, V) and E.is_contiguous() and (E.dim() == 2 or (E.dim() == 3 and step_dev is not None))
    if tok_out is not None:
        _chk(tok_out, i64, 'tok_out')
        assert tok_out.shape == (R, )
    tok = tok_out if tok_out is not None else torch.empty(R, device=logits_c.device, dtype=i64)
    call('mmvid_sample_race_guided_at', _p(logits_c), _p(logits_u), logits_c.stride(0), _p(scale), rows_per_scale, _p(E),
         _p(step_dev) if step_dev is not None else None, int(step0), R * V, float(logit_div), R, V, int(tok_offset), _p(tok), _stream())
    return tok


def logits_truncate(logits, top_k=None, top_p=None, *, logits_u=None, scale=None, rows_per_scale=None, logit_div=1.0, out=None,
                    want_kept=False):
    """Top-k / nucleus truncation of logits [R, V] f32 (row stride = logits.stride(0), V <= 2048) -> out [R, V] (`out` if given; it may
    be `logits` itself; the header promises that for the unguided form, and the guided one is as safe: a wave holds its row of
    both tensors before it stores), or (out, kept int32 [R]: the finite entries per row) with want_kept.  Classes by value
    descending, ties to the lower index: top_k (1 <= top_k < V, else off) keeps the first top_k; top_p (< 1, else off) keeps a class
    iff the mass before it, of P = exp(g / logit_div - max), is below top_p * sum P.  Kept entries hold their value (not divided),
    the others -inf, so sample_race(out, E, noise_u, temperature, logit_div) is the truncated draw.  With logits_u, scale f32
    [R // rows_per_scale] and rows_per_scale the value truncated (and written) is lc + w * (lc - lu) as sample_race_guided reads it."""
    def rows(t, name, shape=None):  # _chk for a tensor that may be a column window of a wider one (a row stride of its own)
        _chk(t[:1], f32, name)
        if t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f'logits_truncate: {name} must be f32 {shape or "[R, V]"} with unit column stride, got {tuple(t.shape)}')

    rows(logits, 'logits')
    R, V = logits.shape
    k = 0 if top_k is None else min(int(top_k), V)  # (top_k >= V is off: no huge value reaches the C int)
    p = 1.0 if top_p is None else float(top_p)
    if (logits_u is None) != (scale is None) or (logits_u is None) != (rows_per_scale is None):
        raise ValueError('logits_truncate: logits_u, scale and rows_per_scale come together (the guided form)')
    if logits_u is not None:
        rows(logits_u, 'logits_u', (R, V))
        rows_per_scale = _guided_operands('logits_truncate', logits, logits_u, scale, rows_per_scale)[2]
    if out is None:
        out = torch.empty(R, V, device=logits.device, dtype=f32)
    else:
        rows(out, 'out', (R, V))
    kept = torch.empty(R, device=logits.device, dtype=torch.int32) if want_kept else None
    if R == 0:  # (an empty tensor has no address to pass)
        return (out, kept) if want_kept else out
    call('mmvid_logits_truncate', _p(logits), _p(logits_u), logits.stride(0) if R > 1 else V, _p(scale),
         rows_per_scale if logits_u is not None else 1, float(logit_div), k, p, R, V, _p(out), out.stride(0) if R > 1 else V, _p(kept),
         _stream())
    return (out, kept) if want_kept else out


def logits_truncate_rows(logits, *, top_k=None, top_p=None, rows_k=None, rows_p=None, rows_inv_div=None, rows_per_param, divide_out=False,
                         logits_u=None, scale=None, rows_per_scale=None, logit_div=1.0, out=None, want_kept=False):
    """logits_truncate with the filter settings of a row read on the device (include/mmvid_hip_ext.h): rows_k int32, rows_p f32, rows_inv_div
    f32, each [R // rows_per_param] on the device of `logits` or None, entry r // rows_per_param for row r.  None: the scalar (top_k,
    top_p, 1 / logit_div) holds for every row.  Device values: a k outside [1, V) and a p >= 1 switch their filter off for the row;
    rows_inv_div holds 1 / temperature as the host rounds it in fp32.  divide_out: a kept entry is g * inv_div (one rounded product),
    so the race that follows runs with logit_div = 1.  With no array and divide_out False the result is logits_truncate's, byte for byte."""
    def rows(t, name, shape=None):
        _chk(t[:1], f32, name)
        if t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f'logits_truncate_rows: {name} must be f32 {shape or "[R, V]"} with unit column stride, got {tuple(t.shape)}')

    rows(logits, 'logits')
    R, V = logits.shape
    k = 0 if top_k is None else min(int(top_k), V)
    p = 1.0 if top_p is None else float(top_p)
    rows_per_param = int(rows_per_param)
    if rows_per_param <= 0 or R % rows_per_param:
        raise ValueError(f'logits_truncate_rows: R = {R} rows is no multiple of rows_per_param = {rows_per_param}')
    for t, name, dt in ((rows_k, 'rows_k', torch.int32), (rows_p, 'rows_p', f32), (rows_inv_div, 'rows_inv_div', f32)):
        if t is None:
            continue
        _chk(t, dt, name)
        if t.device != logits.device or tuple(t.shape) != (R // rows_per_param, ):
            raise ValueError(f'logits_truncate_rows: {name} must be {dt} [R // rows_per_param] = [{R // rows_per_param}] on {logits.device}, '
                             f'got {tuple(t.shape)} on {t.device}')
    if (logits_u is None) != (scale is None) or (logits_u is None) != (rows_per_scale is None):
        raise ValueError('logits_truncate_rows: logits_u, scale and rows_per_scale come together (the guided form)')
    if logits_u is not None:
        rows(logits_u, 'logits_u', (R, V))
        rows_per_scale = _guided_operands('logits_truncate_rows', logits, logits_u, scale, rows_per_scale)[2]
    if out is None:
        out = torch.empty(R, V, device=logits.device, dtype=f32)
    else:
        rows(out, 'out', (R, V))
    kept = torch.empty(R, device=logits.device, dtype=torch.int32) if want_kept else None
    if R == 0:  # (an empty tensor has no address to pass)
        return (out, kept) if want_kept else out
    call('mmvid_logits_truncate_rows', _p(logits), _p(logits_u), logits.stride(0) if R > 1 else V, _p(scale),
         rows_per_scale if logits_u is not None else 1, float(logit_div), k, p, _p(rows_k), _p(rows_p), _p(rows_inv_div), rows_per_param,
         int(bool(divide_out)), R, V, _p(out), out.stride(0) if R > 1 else V, _p(kept), _stream())
    return (out, kept) if want_kept else out


def mp_select_keep(Y, E, preserve, k):
    """Y [b, TS], E [b, Bm, TS], preserve [TS] uint8 or None -> mask1 [b, Bm, TS] uint8 (1 = position stays visible).
    A 2-D preserve [b, TS] with a tensor k (int32 [b] on the device) is the per-video form: row i has its own mask and keep count."""
    _chk(Y, f32, 'Y'), _chk(E, f32, 'E')
    b, Bm, TS = E.shape
    mask1 = torch.empty(b, Bm, TS, device=Y.device, dtype=u8)
    if torch.is_tensor(k) or (preserve is not None and preserve.dim() == 2):
        if not torch.is_tensor(k) or preserve is None or preserve.dim() != 2:
            raise ValueError('mp_select_keep: the per-video form takes preserve [b, TS] uint8 AND k int32 [b] on the device')
        _chk(preserve, u8, 'preserve'), _chk(k, torch.int32, 'k')
        assert tuple(preserve.shape) == (b, TS) and tuple(k.shape) == (b, ), (tuple(preserve.shape), tuple(k.shape), (b, TS))
        call('mmvid_mp_select_keep_rows', _p(Y), _p(E), _p(preserve), _p(k), b, Bm, TS, _p(mask1), _stream())
        return mask1
    call('mmvid_mp_select_keep', _p(Y), _p(E), _p(preserve), b, Bm, TS, int(k), _p(mask1), _stream())
    return mask1


def mp_build_input(control_emb, image_emb, tpos, I_tok, mask1, Bm, mask_id):
    _chk(control_emb, f32, 'control_emb'), _chk(image_emb, f32, 'image_emb'), _chk(tpos, f32, 'tpos'), _chk(I_tok, i64, 'I_tok')
    b, csl, E = control_emb.shape
    TS = I_tok.shape[1]
    out = torch.empty(b * Bm, csl + TS, E, device=control_emb.device, dtype=f32)
    call('mmvid_mp_build_input', _p(control_emb), _p(image_emb), image_emb.shape[0], _p(tpos), _p(I_tok), _p(mask1), b, Bm, csl,
         TS, E, int(mask_id), _p(out), _stream())
    return out


def mp_update(mask1, Ynew, Inew, rel_logit, vid_logit, t, dynamic, Y, I_tok, Imax, Smax, tmax, active, S_out=None,
              jmax_out=None):
    b, Bm, TS = mask1.shape
    call('mmvid_mp_update', _p(mask1), _p(Ynew), _p(Inew), _p(rel_logit), _p(vid_logit), b, Bm, TS, int(t), int(dynamic),
         _p(Y), _p(I_tok), _p(Imax), _p(Smax), _p(tmax), _p(active), _p(S_out), _p(jmax_out), _stream())


def head_rows_fwd(x2d, rows, ln_w, ln_b, w, b, eps=1e-5, label=None, row_weight=None, den_from=None, den_const=1.0):
    """z[r] = LN(x2d[rows[r]]) . w + b (the 768 -> 1 heads); with `label` also the BCE loss [1].  Returns
    (z, mean, rstd, loss|None)."""
    _chk(x2d, f32, 'x'), _chk(rows, i64, 'rows')
    R, E = rows.numel(), x2d.shape[1]
    dev = x2d.device
    z, mean, rstd = (torch.empty(R, device=dev, dtype=f32) for _ in range(3))
    loss = torch.empty(1, device=dev, dtype=f32) if label is not None else None
    call('mmvid_head_bce_fwd', _p(x2d), x2d.stride(0), _p(rows), R, E, _p(ln_w), _p(ln_b), float(eps), _p(w), _p(b),
         _p(label), _p(row_weight), _p(den_from), den_from.numel() if den_from is not None else 0, float(den_const), _p(z),
         _p(mean), _p(rstd), _p(loss), _stream())
    return z, mean, rstd, loss


def head_rows_bwd(x2d, rows, ln_w, ln_b, w, z, mean, rstd, label, row_weight, den_from, den_const, gloss, dx2d, dw, db,
                  dln_w, dln_b):
    R, E = rows.numel(), x2d.shape[1]
    call('mmvid_head_bce_bwd', _p(x2d), x2d.stride(0), _p(rows), R, E, _p(ln_w), _p(ln_b), _p(w), _p(z), _p(mean), _p(rstd),
         _p(label), _p(row_weight), _p(den_from), den_from.numel() if den_from is not None else 0, float(den_const),
         _p(gloss), _p(dx2d), dx2d.stride(0), _p(dw), _p(db), _p(dln_w), _p(dln_b), _stream())


def bert_build_ids(text, visual_tok, nvis, target, target_warp, mask1, pad_base, mask_id, has_rel, has_vid, text_neg=None):
    """-> (ids [(1+rel+vid)*B, L] int64, select_full [B*L] uint8, target_full [B*L] int64, select_count [1] f32)."""
    _chk(text, i64, 'text'), _chk(target, i64, 'target')
    B, Ttxt = text.shape
    TS = target.shape[1]
    Nvis = int(nvis)  # visual_tok None with nvis > 0: the visual segment is all [MASK] (dalle_bert.py:954-957)
    assert visual_tok is None or visual_tok.shape == (B, Nvis)
    L = 1 + Ttxt + Nvis + 2 + TS
    nseq = 1 + int(has_rel) + int(has_vid)
    dev = text.device
    ids = torch.empty(nseq * B, L, device=dev, dtype=i64)
    sel = torch.empty(B * L, device=dev, dtype=u8)
    tfull = torch.empty(B * L, device=dev, dtype=i64)
    cnt = torch.empty(1, device=dev, dtype=f32)
    m1 = mask1 if mask1.dtype == u8 else mask1.to(u8)
    call('mmvid_bert_build_ids', _p(text), _p(text_neg), _p(visual_tok), _p(target), _p(target_warp), _p(m1.contiguous()), B,
         Ttxt, Nvis, TS, int(pad_base), int(mask_id), int(has_rel), int(has_vid), _p(ids), _p(sel), _p(tfull), _p(cnt),
         _stream())
    return ids, sel, tfull, cnt


def gemv_rows(x, W, bias=None, ln=None, act=0, residual=None, round_in=False, round_out=False, out=None):
    """Decode-time linear layer on a few rows: y = act(LN?(x) @ W^T + bias) (+ residual).  x [NB, K] f32 (contiguous), W [N, K] bf16."""
    _chk(x, f32, 'x'), _chk(W, bf16, 'W')
    NB, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(NB, N, device=x.device, dtype=f32)
    lw, lb, eps = (ln[0], ln[1], ln[2]) if ln is not None else (None, None, 0.0)
    mfma = round_in and K % 256 == 0 and N % 16 == 0 and (K <= 1024 or (K == 4096 and N <= 1024 and ln is None))
    step = 64 if mfma else (16 if round_in and K <= 3072 else 8 if (round_in or K <= 3072) else 4)  # rows per launch: 64 bf16-exact rows on the MFMA form, 16 / 8 on the vector-ALU kernel (K = 4,096: 8 bf16-staged rows = 64 KiB, 4 fp32 rows); larger batches in slices
    for r0 in range(0, NB, step):
        nb = min(step, NB - r0)
        res = residual[r0:r0 + nb] if residual is not None else None
        call('mmvid_gemv_rows', _p(x[r0:r0 + nb]), K, nb, K, _p(lw), _p(lb), float(eps), _p(W), _p(bias), N, int(act), _p(res), N,
             int(round_in), int(round_out), _p(out[r0:r0 + nb]), N, _stream())
    return out


def decode_embed(tok, table, pos_rows, pos_dev, out, pos_off=0, record=None, record_pos0=0):
    """out[b] = table[tok[b]] + pos_rows[pos_dev + pos_off] (the embedding row of a freshly sampled token); record (int64 [B, n],
    optional): record[b, pos_dev - record_pos0] = tok[b]."""
    _chk(tok, i64, 'tok'), _chk(table, f32, 'table'), _chk(pos_rows, f32, 'pos_rows')
    B, E = out.shape
    if record is not None:
        _chk(record, i64, 'record')
        assert record.shape[0] == B and record.stride(1) == 1
    call('mmvid_decode_embed_record', _p(tok), _p(table), table.shape[0], _p(pos_rows), _p(pos_dev), int(pos_off), B, E, _p(out),
         _p(record) if record is not None else None, record.stride(0) if record is not None else 0, int(record_pos0), _stream())
    return out


def decode_embed_groups(tok, table, pos_rows, pos_dev, out, groups, pos_off=0, record=None, record_pos0=0):
    """decode_embed for `groups` copies of the batch: tok [B], out [groups * B, E], out[g * B + b] = table[tok[b]] + pos_rows[pos_dev + pos_off]
    for every g (the guided ART-V sampler's two tower rows per video); record (int64 [B, n], optional) is written once per b."""
    _chk(tok, i64, 'tok'), _chk(table, f32, 'table'), _chk(pos_rows, f32, 'pos_rows'), _chk(out, f32, 'out')
    B, groups = tok.shape[0], int(groups)
    if groups < 1 or out.dim() != 2 or out.shape[0] != groups * B:
        raise ValueError(f'decode_embed_groups: out {tuple(out.shape)} is not [groups * B, E] = [{groups} * {B}, E]')
    E = out.shape[1]
    if record is not None:
        _chk(record, i64, 'record')
        assert record.shape[0] == B and record.stride(1) == 1
    call('mmvid_decode_embed_record_groups', _p(tok), _p(table), table.shape[0], _p(pos_rows), _p(pos_dev), int(pos_off), B, groups, E, _p(out),
         _p(record) if record is not None else None, record.stride(0) if record is not None else 0, int(record_pos0), _stream())
    return out
