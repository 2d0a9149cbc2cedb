"""C-ABI contract of the bf16-path entry points (include/mmvid_hip.h) on guarded buffers (tests/guarded.py).

Each test runs the same call twice: once PADDED AND POISONED -- every leading dimension larger than the natural one and different
from the others (within the entry point's MMVID_REQUIRE alignment rules), every operand inside 64-KiB guards, inputs surrounded by
quiet NaN / out-of-range ids, outputs pre-filled with a sentinel -- and once on dense, naturally strided buffers (guards kept).

* every element outside a declared [rows][cols] window must keep its bits (front guard, row gaps, batch gaps, back guard); inputs
  must come back unchanged;
* for the deterministic entry points the padded call's windows equal the dense call's bit for bit;
* results accumulated with fp32 atomics (mmvid_gemm_bf16 with splitk > 1, mmvid_layernorm_bwd without a workspace, the loss_sum of
  mmvid_cross_entropy_fwd, mmvid_grad_sqnorm) are compared with K 2^-23 sum |terms| around an fp64 evaluation instead (K = number
  of terms + 1) and must be finite wherever the dense result is.  Where the fp32 terms themselves are not an output (the dbias of
  mmvid_attention_bwd_bias and the out_colsum of mmvid_gemm_bf16 with a bf16 result: sums of registers in front of a bf16 store)
  the padded and the dense call, which add the same terms in a free order, are compared with each other:
  |padded - dense| <= 2 K 2^-23 sum |terms|.  No allowance had to be widened on hardware.

A window ends with the last element of its last row: the back guard's NaN starts right behind the last sequence of an attention
operand, so a key tile that runs past B*L rows reads NaN if it is read at all.  The matrix kernels (GEMM, weight gradients,
convolutions, gemv_rows, colsum) get the same embedding in tests/test_integer_exact.py, where the padded call must equal an exact
reference, which includes equality with the dense call.

Inputs are seeded CPU randn; nothing here provokes a fault: poison and sentinels are ordinary data."""
import ctypes

import pytest
import torch

from guarded import (BAD_ID, Guarded, assert_pair_within_atomic_bound, assert_same_bits, assert_within_atomic_bound, report_mismatch)
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen

pytestmark = pytest.mark.gpu
BF, F32, I64, I32, U8 = torch.bfloat16, torch.float32, torch.int64, torch.int32, torch.uint8
NAN = float('nan')


def randn(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def both(build, what, loose=()):
    """build(padded) -> (dict name -> Guarded | None, launch()).  Runs padded and dense, checks every guard, and demands bit-identical
    output windows except for the names in `loose` (atomics: the caller bounds them).  -> {True: windows, False: windows}."""
    res, roles = {}, {}
    for padded in (True, False):
        operands, launch = build(padded)
        launch()
        tag = 'padded' if padded else 'dense'
        res[padded] = {k: gd.check(f'{what} [{tag}] {k}') for k, gd in operands.items() if gd is not None}
        roles = {k: gd.role for k, gd in operands.items() if gd is not None}
    for k, role in roles.items():
        if role == 'out' and k not in loose:
            assert_same_bits(res[True][k], res[False][k], f'{what} {k}')
    return res


def out(shape, dtype, ld=None, stride=None, partial=False):
    """A pure output (every element of its window must be stored); partial: a workspace / cache the call fills only in part."""
    return Guarded(role='out', shape=shape, dtype=dtype, ld=ld, stride=stride, partial=partial)


# ================================================================================================= mmvid_gemm_bf16 on N(0,1) operands
# (the exact-term coverage is in test_integer_exact.py; here: the activation epilogues, and split-K against its atomic bound)
GEMM_SHAPES = [(300, 136, 200), (579, 2304, 768)]  # ragged in M, N and K against every tile; the qkv projection at B*L = 579


def _m_for(akm, M):
    """A k-major A needs M % 8 == 0 (MMVID_REQUIRE); the row-major layouts keep the ragged M."""
    return -(-M // 8) * 8 if akm else M


@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
@pytest.mark.parametrize('variant', ['gelu_save_pre', 'erf_gelu_f32', 'dact_pre', 'dact_pre_colsum', 'bias_residual_both', 'batch3_bf16'])
def test_gemm_bf16_padded_equals_dense(akm, bkm, M, N, K, variant):
    M = _m_for(akm, M)
    g = _gen('gemm', akm, bkm, M, N, K, variant)
    nb = 3 if variant.startswith('batch') else 1
    A = randn(g, nb, *((K, M) if akm else (M, K)), dtype=BF)
    B = randn(g, nb, *((K, N) if bkm else (N, K)), dtype=BF, scale=0.05)
    bias, resid, pre = randn(g, N), randn(g, nb, M, N), randn(g, nb, M, N, dtype=BF)
    cs0 = randn(g, N)

    def build(padded):
        p = int(padded)
        lda, ldb, ldc, ldr, ldp = A.shape[2] + 8 * p, B.shape[2] + 16 * p, N + 12 * p, N + 20 * p, N + 28 * p
        sA, sB, sC = A.shape[1] * lda + 16 * p, B.shape[1] * ldb + 24 * p, M * ldc + 12 * p
        o = dict(A=Guarded(A, ld=lda, stride=sA), B=Guarded(B, ld=ldb, stride=sB), bias=None, residual=None, dact=None, save=None, out_f32=None,
                 out_bf16=None, colsum=None)
        act = 0
        if variant == 'gelu_save_pre':
            o.update(bias=Guarded(bias), save=out((nb, M, N), BF, ldp), out_bf16=out((nb, M, N), BF, ldc))
            act = 1
        elif variant == 'erf_gelu_f32':
            o.update(bias=Guarded(bias), out_f32=out((nb, M, N), F32, ldc))
            act = 2
        elif variant.startswith('dact_pre'):
            o.update(dact=Guarded(pre, ld=ldp), out_bf16=out((nb, M, N), BF, ldc))
            if variant.endswith('colsum'):
                o.update(colsum=Guarded(base=cs0))
        elif variant == 'bias_residual_both':
            o.update(bias=Guarded(bias), residual=Guarded(resid, ld=ldr), out_f32=out((nb, M, N), F32, ldc), out_bf16=out((nb, M, N), BF, ldc))
        else:
            o.update(bias=Guarded(bias), out_bf16=out((nb, M, N), BF, ldc, sC))
        one = nb == 1

        def launch():
            _call('mmvid_gemm_bf16', akm, bkm, M, N, K, o['A'].ptr, lda, o['B'].ptr, ldb, nb, 0 if one else sA, 0 if one else sB, 0 if one else sC, 1,
                  1.0, _ptr(o['bias']), _ptr(o['residual']), ldr, _ptr(o['dact']), _ptr(o['save']), ldp, act, 0, _ptr(o['out_f32']),
                  _ptr(o['out_bf16']), ldc, _ptr(o['colsum']))
        return o, launch

    what = f'gemm {akm}{bkm} {M}x{N}x{K} {variant}'
    res = both(build, what, loose=('colsum',))
    for k in ('out_f32', 'out_bf16', 'save'):
        if k in res[True]:
            assert bool(torch.isfinite(res[True][k].float()).all()), f'{what}: {k} is not finite'
    if 'colsum' in res[True]:
        # one fp32 atomic per row block and column.  Both calls add the same fp32 values (those in front of the bf16 store) in a free
        # order: |padded - dense| <= 2 K 2^-23 sum |terms|, K = M + 1 terms, sum |terms| evaluated in fp64 from the stored result
        # (each stored value is its term to 2^-9 relative: sum |terms| <= (1 + 2^-8) sum |stored|)
        stored = res[False]['out_bf16'].double()[0]
        mag = cs0.double().abs() + (1 + 2.0**-8) * stored.abs().sum(0)
        assert_pair_within_atomic_bound(res[True]['colsum'], res[False]['colsum'], mag, M + 1, what + ' out_colsum')
        # a second, looser line against fp64: the reference is rebuilt from the bf16 copies, 2^-9 per term away from the fp32 terms
        ref = cs0.double() + stored.sum(0)
        for tag in (True, False):
            err = (res[tag]['colsum'].double() - ref).abs()
            assert bool((err <= ((M + 1) * 2.0**-23 + 2.0**-9) * mag).all()), f'{what}: column sums far from the stored result\'s'


@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('M,N,K', GEMM_SHAPES + [(776, 264, 1043)])
@pytest.mark.parametrize('splitk', [3, 8])
def test_gemm_bf16_splitk_atomics_within_bound(akm, bkm, M, N, K, splitk):
    """fp32 atomicAdd into out_f32 (which holds the base value): the order is free, so the bar is K 2^-23 sum |terms| around fp64."""
    M = _m_for(akm, M)
    if K % 8 and not (akm and bkm):  # a row-major operand needs K % 8 == 0 (MMVID_REQUIRE)
        K = K // 8 * 8
    g = _gen('gemm_splitk', akm, bkm, M, N, K, splitk)
    A = randn(g, *((K, M) if akm else (M, K)), dtype=BF)
    B = randn(g, *((K, N) if bkm else (N, K)), dtype=BF)
    base = randn(g, M, N)

    def build(padded):
        p = int(padded)
        lda, ldb, ldc = A.shape[1] + 8 * p, B.shape[1] + 16 * p, N + 12 * p
        o = dict(A=Guarded(A, ld=lda), B=Guarded(B, ld=ldb), out_f32=Guarded(base=base, ld=ldc))

        def launch():
            _call('mmvid_gemm_bf16', akm, bkm, M, N, K, o['A'].ptr, lda, o['B'].ptr, ldb, 1, 0, 0, 0, splitk, 1.0, None, None, 0, None, None, 0, 0, 1,
                  o['out_f32'].ptr, None, ldc, None)
        return o, launch

    what = f'gemm {akm}{bkm} {M}x{N}x{K} splitk={splitk}'
    res = both(build, what, loose=('out_f32',))
    Am, Bm = (A.double().t() if akm else A.double()), (B.double() if bkm else B.double().t())
    ref, mag = base.double() + Am @ Bm, base.double().abs() + Am.abs() @ Bm.abs()
    assert_within_atomic_bound(res[True]['out_f32'], res[False]['out_f32'], ref, mag, K + 1, what)


# ========================================================================================================================= LayerNorm
# the towers' widths (the pipelined instance) and the generic kernel, ragged rows; the widest row (1024, the ViT-L/14 towers: every lane
# of the generic kernel live, no guard false) and a single row (the second row of every forward wave dead)
LN_SHAPES = [(10, 768), (1158, 768), (77, 512), (37, 200), (5, 1024), (1, 8)]


def _ln_inputs(rows, E):
    g = _gen('ln', rows, E)
    x = randn(g, rows, E) * 2 + 0.5
    w, b = randn(g, E) * 0.1 + 1, randn(g, E) * 0.1
    dy = randn(g, rows, E)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()
    return x, w, b, dy, mean.float(), rstd.float(), randn(g, rows, E), randn(g, E), randn(g, E), randn(g, E)


@pytest.mark.parametrize('rows,E', LN_SHAPES)
@pytest.mark.parametrize('outputs', ['both', 'bf16', 'f32'])
def test_layernorm_fwd_padded_equals_dense(rows, E, outputs):
    x, w, b = _ln_inputs(rows, E)[:3]

    def build(padded):
        p = int(padded)
        ldx, ldy = E + 4 * p, E + 12 * p
        o = dict(x=Guarded(x, ld=ldx), w=Guarded(w), b=Guarded(b), y16=out((rows, E), BF, ldy) if outputs != 'f32' else None,
                 y32=out((rows, E), F32, ldy) if outputs != 'bf16' else None, mean=out((rows,), F32), rstd=out((rows,), F32))
        return o, lambda: _call('mmvid_layernorm_fwd', o['x'].ptr, ldx, rows, E, o['w'].ptr, o['b'].ptr, 1e-5, _ptr(o['y16']), _ptr(o['y32']), ldy,
                                o['mean'].ptr, o['rstd'].ptr)

    res = both(build, f'layernorm_fwd {rows}x{E} {outputs}')[True]
    assert all(bool(torch.isfinite(v.float()).all()) for v in res.values())
    ref = torch.nn.functional.layer_norm(x.double(), (E,), w.double(), b.double(), 1e-5)
    y = res['y32'] if 'y32' in res else res['y16']
    assert float((y.double() - ref).abs().max()) < (1e-4 if 'y32' in res else 4e-2)


@pytest.mark.parametrize('rows,E', LN_SHAPES)
@pytest.mark.parametrize('form', ['ws', 'ex_f32_dy', 'ws_bf16_dy', 'ws_no_dx16_no_add', 'ws_only_colsum', 'partial_reduce', 'atomics'])
def test_layernorm_bwd_padded_equals_dense(rows, E, form):
    """mmvid_layernorm_bwd_ws / _bwd_ex (fp32 and bf16 dy) / _bwd_partial + _reduce_multi: deterministic, bit-identical between the
    padded and the dense call; _partial + _reduce_multi also bit-identical to _bwd_ex with a workspace (header).  mmvid_layernorm_bwd
    without a workspace adds dw / db / dx_colsum with atomics: K 2^-23 sum |terms| with the terms taken in fp64 from the kernel's own
    dx (column sums) and from dy, x, mean, rstd (dw, db)."""
    from mmvid_amd import _lib
    x, w, b, dy, mean, rstd, dx0, dw0, db0, cs0 = _ln_inputs(rows, E)
    dy_bf16 = form == 'ws_bf16_dy'
    dyv = dy.to(BF) if dy_bf16 else dy
    add = form != 'ws_no_dx16_no_add'
    want16 = form not in ('ws_no_dx16_no_add', 'atomics')
    only_cs = form == 'ws_only_colsum'
    nws = 3 * E * 256

    def build(padded):
        p = int(padded)
        lddy, ldx, lddx = E + 8 * p, E + 4 * p, E + 12 * p
        o = dict(dy=Guarded(dyv, ld=lddy), x=Guarded(x, ld=ldx), mean=Guarded(mean), rstd=Guarded(rstd), w=Guarded(w),
                 dx=Guarded(base=dx0, ld=lddx) if add else out((rows, E), F32, lddx), dx16=out((rows, E), BF, lddx) if want16 else None,
                 dw=None if only_cs else Guarded(base=dw0), db=None if only_cs else Guarded(base=db0), cs=Guarded(base=cs0),
                 ws=None if form == 'atomics' else out((nws,), F32, partial=True))
        head = (o['dy'].ptr, int(dy_bf16), lddy, o['x'].ptr, ldx, o['mean'].ptr, o['rstd'].ptr, o['w'].ptr, rows, E, o['dx'].ptr, lddx, int(add),
                _ptr(o['dx16']))

        def launch():
            if form == 'atomics':
                _call('mmvid_layernorm_bwd', head[0], *head[2:], o['dw'].ptr, o['db'].ptr, o['cs'].ptr)
            elif form == 'partial_reduce':
                blocks = ctypes.c_int(0)
                _call('mmvid_layernorm_bwd_partial', *head, 1, 1, 1, o['ws'].ptr, nws, ctypes.byref(blocks))
                item = (_lib.LnReduce * 1)()
                item[0].partial, item[0].dw, item[0].db, item[0].dx_colsum = o['ws'].ptr.value, o['dw'].ptr.value, o['db'].ptr.value, o['cs'].ptr.value
                _call('mmvid_layernorm_bwd_reduce_multi', 1, item, blocks.value, E)
            elif dy_bf16 or form == 'ex_f32_dy':  # mmvid_layernorm_bwd_ex itself, with both kinds of dy
                _call('mmvid_layernorm_bwd_ex', *head, _ptr(o['dw']), _ptr(o['db']), o['cs'].ptr, o['ws'].ptr, nws)
            else:
                _call('mmvid_layernorm_bwd_ws', head[0], *head[2:], _ptr(o['dw']), _ptr(o['db']), o['cs'].ptr, o['ws'].ptr, nws)
        return o, launch

    what = f'layernorm_bwd {rows}x{E} {form}'
    res = both(build, what, loose=('dw', 'db', 'cs') if form == 'atomics' else ())
    r = res[True]
    assert all(bool(torch.isfinite(v.float()).all()) for k, v in r.items() if k != 'ws')
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    if form == 'atomics':
        dxk = res[False]['dx'].double()
        for name, ref, mag in (('dw', dw0.double() + (dy.double() * xh).sum(0), dw0.double().abs() + (dy.double() * xh).abs().sum(0)),
                               ('db', db0.double() + dy.double().sum(0), db0.double().abs() + dy.double().abs().sum(0)),
                               ('cs', cs0.double() + dxk.sum(0), cs0.double().abs() + dxk.abs().sum(0))):
            # (each term of dw is itself a few fp32 operations on (x - mean) rstd dy: 4 more roundings per term)
            assert_within_atomic_bound(r[name], res[False][name], ref, mag, rows + 1 + (4 if name == 'dw' else 0), f'{what} {name}')
    if form == 'partial_reduce':  # bit-identical to the single-call two-stage form
        o2 = dict(dy=Guarded(dy), x=Guarded(x), mean=Guarded(mean), rstd=Guarded(rstd), w=Guarded(w), dx=Guarded(base=dx0), dx16=out((rows, E), BF),
                  dw=Guarded(base=dw0), db=Guarded(base=db0), cs=Guarded(base=cs0), ws=out((nws,), F32, partial=True))
        _call('mmvid_layernorm_bwd_ex', o2['dy'].ptr, 0, E, o2['x'].ptr, E, o2['mean'].ptr, o2['rstd'].ptr, o2['w'].ptr, rows, E, o2['dx'].ptr, E, 1,
              o2['dx16'].ptr, o2['dw'].ptr, o2['db'].ptr, o2['cs'].ptr, o2['ws'].ptr, nws)
        for k in ('dx', 'dx16', 'dw', 'db', 'cs'):
            report_mismatch(r[k], o2[k].check(k), f'{what}: {k} against mmvid_layernorm_bwd_ex with a workspace')
    # a loose sanity bar on the values themselves (the numeric bars are tests/test_kernels_gpu.py's)
    g1 = dy.double() * w.double()
    dxr = (g1 - g1.mean(1, keepdim=True) - xh * (g1 * xh).mean(1, keepdim=True)) * rstd.double()[:, None] + (dx0.double() if add else 0)
    assert float((r['dx'].double() - dxr).abs().max()) < (5e-2 if dy_bf16 else 1e-3)


# ========================================================================================================================= attention
def _mask_args(mode, L):
    if mode == 'none':
        return (0, -1, 0, -1, 0)
    if mode == 'causal':
        return (1, -1, 0, -1, 0)
    if L >= 579:
        return (2, 65, 65, 66, 66)
    r0 = min(L - 1, 17)
    return (2, r0, min(L - 1, 18), (r0 + 1 if r0 + 1 < L else -1), min(L - 1, 9))


ATTN_SHAPES = [(2, 1, 2), (2, 33, 2), (3, 65, 2), (2, 579, 12)]


@pytest.mark.parametrize('B,L,H', ATTN_SHAPES)
@pytest.mark.parametrize('mode', ['none', 'causal', 'rows'])
def test_attention_fwd_bwd_padded_equals_dense(B, L, H, mode):
    """mmvid_attention_fwd and mmvid_attention_bwd_bias (dbias given and NULL): ld, ldo, lddo, ldg padded; the last sequence of every
    operand ends at its back guard."""
    E = 64 * H
    g = _gen('attn', B, L, H, mode)
    qkv, dO = randn(g, B * L, 3 * E, dtype=BF), randn(g, B * L, E, dtype=BF)
    db0 = randn(g, 3 * E)
    m = _mask_args(mode, L)

    def build_fwd(padded):
        p = int(padded)
        ld, ldo = 3 * E + 8 * p, E + 16 * p
        o = dict(qkv=Guarded(qkv, ld=ld), out=out((B * L, E), BF, ldo), lse2=out((B, H, L), F32))
        return o, lambda: _call('mmvid_attention_fwd', o['qkv'].ptr, ld, B, L, H, E, 0.125, *m, o['out'].ptr, ldo, o['lse2'].ptr)

    what = f'attention B={B} L={L} H={H} {mode}'
    fwd = both(build_fwd, what + ' fwd')[True]
    assert bool(torch.isfinite(fwd['out'].float()).all()) and bool(torch.isfinite(fwd['lse2']).all()), what + ': forward not finite'
    O, lse2 = fwd['out'], fwd['lse2']

    for with_bias in (True, False):
        def build_bwd(padded):
            p = int(padded)
            ld, ldo, lddo, ldg = 3 * E + 8 * p, E + 16 * p, E + 24 * p, 3 * E + 32 * p
            o = dict(qkv=Guarded(qkv, ld=ld), O=Guarded(O, ld=ldo), dO=Guarded(dO, ld=lddo), lse2=Guarded(lse2), delta=out((B, H, L), F32),
                     dqkv=out((B * L, 3 * E), BF, ldg), dbias=Guarded(base=db0) if with_bias else None)
            return o, lambda: _call('mmvid_attention_bwd_bias', o['qkv'].ptr, ld, o['O'].ptr, ldo, o['dO'].ptr, lddo, o['lse2'].ptr, o['delta'].ptr,
                                    B, L, H, E, 0.125, *m, o['dqkv'].ptr, ldg, _ptr(o['dbias']))

        bwd = both(build_bwd, what + f' bwd dbias={with_bias}', loose=('dbias',))
        assert bool(torch.isfinite(bwd[True]['dqkv'].float()).all()), what + ': dqkv not finite'
        if with_bias:
            # dbias += column sums of dq / dk / dv from the fp32 registers in front of the bf16 store (fp32 atomics).  The padded and the
            # dense call add the same B*L fp32 terms per column in a free order: |padded - dense| <= 2 K 2^-23 sum |terms|, K = B*L + 1,
            # sum |terms| in fp64 from the stored dqkv (equal to the registers' to 2^-9 relative: sum |terms| <= (1 + 2^-8) sum |stored|)
            d = bwd[False]['dqkv'].double()
            mag = db0.double().abs() + (1 + 2.0**-8) * d.abs().sum(0)
            assert_pair_within_atomic_bound(bwd[True]['dbias'], bwd[False]['dbias'], mag, B * L + 1, what + ' dbias')
            # a second, looser line against fp64 rebuilt from the bf16 copies (2^-9 per term away from the fp32 terms)
            ref = db0.double() + d.sum(0)
            for tag in (True, False):
                err = (bwd[tag]['dbias'].double() - ref).abs()
                assert bool((err <= ((B * L + 1) * 2.0**-23 + 2.0**-9) * mag).all()), f'{what}: dbias far from the column sums of the stored dqkv'


@pytest.mark.parametrize('B,L,H', [(4, 33, 2), (7, 65, 2), (3, 579, 12)])
@pytest.mark.parametrize('with_lse', [True, False])
def test_attention_fwd_keylen_padded_equals_dense(B, L, H, with_lse):
    E = 64 * H
    g = _gen('keylen', B, L, H)
    qkv = randn(g, B * L, 3 * E, dtype=BF)
    kl = torch.tensor([L, 1, L - 1, 0, L + 5, 17, 32][:B], dtype=I32)

    def build(padded):
        p = int(padded)
        ld, ldo = 3 * E + 8 * p, E + 16 * p
        o = dict(qkv=Guarded(qkv, ld=ld), key_len=Guarded(kl), out=out((B * L, E), BF, ldo), lse2=out((B, H, L), F32) if with_lse else None)
        return o, lambda: _call('mmvid_attention_fwd_keylen', o['qkv'].ptr, ld, B, L, H, E, 0.125, o['key_len'].ptr, o['out'].ptr, ldo, _ptr(o['lse2']))

    res = both(build, f'attention_fwd_keylen B={B} L={L} H={H}')[True]
    assert all(bool(torch.isfinite(v.float()).all()) for v in res.values())


# ======================================================================================================= kv_store / attention_decode
@pytest.mark.parametrize('from_device', [False, True])
def test_kv_store_writes_only_its_rows(from_device):
    B, L, E, Lmax, pos = 2, 3, 128, 16, 5
    g = _gen('kv_store')
    qkv = randn(g, B * L, 3 * E, dtype=BF)

    def build(padded):
        ldq = 3 * E + 8 * int(padded)
        o = dict(qkv=Guarded(qkv, ld=ldq), pos=Guarded(torch.tensor([pos], dtype=I32)) if from_device else None, cache=out((B * Lmax, 2 * E), BF, partial=True))
        return o, lambda: _call('mmvid_kv_store', o['qkv'].ptr, ldq, B, L, E, _ptr(o['pos']), -7 if from_device else pos, Lmax, o['cache'].ptr)

    cache = both(build, 'kv_store')[True]['cache'].view(B, Lmax, 2 * E)
    want = Guarded(role='out', shape=(B, Lmax, 2 * E), dtype=BF, device='cpu').window()  # the sentinel everywhere ...
    want[:, pos:pos + L] = qkv.view(B, L, 3 * E)[:, :, E:]                                 # ... but rows pos .. pos + L - 1 = K | V
    report_mismatch(cache, want, 'kv_store: cache rows')


@pytest.mark.parametrize('pos', [0, 5, 64, 129])
@pytest.mark.parametrize('from_device', [False, True])
def test_attention_decode_padded_equals_dense_and_ignores_rows_beyond_pos(pos, from_device):
    """Cache rows beyond `pos` are NaN: the one-query attention over positions 0..pos must not consume them."""
    B, H, Lmax = 3, 2, 130
    E = 64 * H
    g = _gen('decode', pos)
    qkv = randn(g, B, 3 * E, dtype=BF)
    cache = randn(g, B, Lmax, 2 * E, dtype=BF)
    cache[:, pos + 1:] = NAN

    def build(padded):
        p = int(padded)
        ldq, ldo = 3 * E + 8 * p, E + 8 * p
        o = dict(qkv=Guarded(qkv, ld=ldq), cache=Guarded(cache.view(B * Lmax, 2 * E)), pos=Guarded(torch.tensor([pos], dtype=I32)) if from_device else None,
                 out=out((B, E), BF, ldo))
        return o, lambda: _call('mmvid_attention_decode', o['qkv'].ptr, ldq, o['cache'].ptr, B, Lmax, H, E, _ptr(o['pos']), 0 if from_device else pos,
                                0.125, o['out'].ptr, ldo)

    got = both(build, f'attention_decode pos={pos}')[True]['out']
    q = qkv[:, :E].double().view(B, H, 64)
    k, v = (cache[:, :pos + 1, i * E:(i + 1) * E].double().view(B, pos + 1, H, 64) for i in (0, 1))
    pr = torch.softmax(torch.einsum('bhd,bkhd->bhk', q, k) * 0.125, -1)
    ref = torch.einsum('bhk,bkhd->bhd', pr, v).reshape(B, E)
    assert bool(torch.isfinite(got.float()).all()), 'attention_decode consumed a cache row beyond pos'
    assert float((got.double() - ref).abs().max()) < 2e-2 * float(ref.abs().max())


# ===================================================================================================================== cross entropy
@pytest.mark.parametrize('rows,V', [(37, 1024), (37, 1000), (5, 8)])  # 1000 / 4 = 250 float4 per row: not a multiple of the wave's 64
@pytest.mark.parametrize('with_select', [True, False])
def test_cross_entropy_padded_equals_dense_and_skips_unselected_rows(rows, V, with_select):
    """Rows with select == 0 are not read (header): their logits are NaN and their targets out of range here, lse is 0 and the gradient
    row is zero; the out-of-range counter of mmvid_device_faults stays at zero.  loss_sum is one fp32 atomic per selected row."""
    from mmvid_amd import _lib
    g = _gen('ce', rows, V)
    logits = randn(g, rows, V) * 3
    target = torch.randint(0, V, (rows,), generator=g)
    sel = (torch.rand(rows, generator=g) < 0.6).to(U8)
    sel[0], sel[-1] = 1, 0
    if with_select:
        logits[sel == 0] = NAN
        target[sel == 0] = BAD_ID
    else:
        sel[:] = 1
    loss0, gscale = torch.tensor([0.75]), torch.tensor([0.37])
    lse_ref = torch.logsumexp(torch.where(sel[:, None] != 0, logits, torch.zeros(())).double(), 1).float()
    _lib.device_faults(reset=True)

    def build(padded):
        p = int(padded)
        ldl, ldd = V + 4 * p, V + 12 * p
        o = dict(logits=Guarded(logits, ld=ldl), target=Guarded(target), select=Guarded(sel) if with_select else None, lse=out((rows,), F32),
                 loss=Guarded(base=loss0), lse_in=Guarded(lse_ref), gscale=Guarded(gscale), d=out((rows, V), BF, ldd))

        def launch():
            _call('mmvid_cross_entropy_fwd', o['logits'].ptr, ldl, o['target'].ptr, _ptr(o['select']), rows, V, o['lse'].ptr, o['loss'].ptr)
            _call('mmvid_cross_entropy_bwd', o['logits'].ptr, ldl, o['target'].ptr, _ptr(o['select']), o['lse_in'].ptr, o['gscale'].ptr, rows, V,
                  o['d'].ptr, ldd)
        return o, launch

    what = f'cross_entropy {rows}x{V} select={with_select}'
    res = both(build, what, loose=('loss',))
    assert _lib.device_faults(reset=True)[:2] == [0, 0], 'a target of an unselected row was read (and counted as out of range)'
    r = res[True]
    on = sel != 0
    assert bool((r['lse'][~on] == 0).all()) and bool((r['d'][~on] == 0).all()), what + ': unselected rows'
    assert bool(torch.isfinite(r['lse']).all()) and bool(torch.isfinite(r['d'].float()).all()) and bool(torch.isfinite(r['loss']).all())
    assert float((r['lse'][on] - lse_ref[on]).abs().max()) < 1e-4
    rows_on = on.nonzero().view(-1)
    terms = r['lse'][on] - logits[rows_on, target[rows_on]]  # one fp32 subtraction per selected row, as the kernel forms it
    ref, mag = loss0.double() + terms.double().sum(), loss0.double().abs() + terms.double().abs().sum()
    assert_within_atomic_bound(r['loss'], res[False]['loss'], ref, mag, int(on.sum()) + 1, what + ' loss_sum')
    p = torch.softmax(logits[on].double(), 1)
    p[torch.arange(len(rows_on)), target[rows_on]] -= 1
    assert float((r['d'][on].double() - p * 0.37).abs().max()) < 4e-3


# ======================================================================================================================== head + BCE
@pytest.mark.parametrize('E', [768, 200])
@pytest.mark.parametrize('optional', [True, False])
def test_head_bce_padded_equals_dense_and_reads_only_named_rows(E, optional):
    """Rows of x (and of dx) not named in `rows` are NaN / must keep the sentinel.  optional: row_weight and den_from given, or NULL."""
    T, R = 40, 9
    g = _gen('head', E)
    rows = torch.randperm(T, generator=g)[:R].sort().values
    x = torch.full((T, E), NAN)
    x[rows] = randn(g, R, E)
    ln_w, ln_b, w, b = randn(g, E) * 0.1 + 1, randn(g, E) * 0.1, randn(g, E) * 0.05, randn(g, 1)
    label, rw, den = (torch.rand(R, generator=g) < 0.5).float(), torch.rand(R, generator=g), torch.tensor([3.0, 0.0, 2.0])
    gloss = torch.tensor([1.3])
    dx0, acc0 = randn(g, T, E), [randn(g, n) for n in (E, 1, E, E)]

    def build(padded):
        p = int(padded)
        ldx, lddx = E + 4 * p, E + 12 * p
        o = dict(x=Guarded(x, ld=ldx), rows=Guarded(rows), ln_w=Guarded(ln_w), ln_b=Guarded(ln_b), w=Guarded(w), b=Guarded(b), label=Guarded(label),
                 rw=Guarded(rw) if optional else None, den=Guarded(den) if optional else None, gloss=Guarded(gloss), z=out((R,), F32),
                 mean=out((R,), F32), rstd=out((R,), F32), loss=out((1,), F32), dx=Guarded(base=dx0, ld=lddx), dw=Guarded(base=acc0[0]),
                 db=Guarded(base=acc0[1]), dln_w=Guarded(base=acc0[2]), dln_b=Guarded(base=acc0[3]))
        nden = 3 if optional else 0

        def launch():
            _call('mmvid_head_bce_fwd', o['x'].ptr, ldx, o['rows'].ptr, R, E, o['ln_w'].ptr, o['ln_b'].ptr, 1e-5, o['w'].ptr, o['b'].ptr,
                  o['label'].ptr, _ptr(o['rw']), _ptr(o['den']), nden, 4.0, o['z'].ptr, o['mean'].ptr, o['rstd'].ptr, o['loss'].ptr)
            # the backward reads z, mean, rstd where the forward has just written them
            _call('mmvid_head_bce_bwd', o['x'].ptr, ldx, o['rows'].ptr, R, E, o['ln_w'].ptr, o['ln_b'].ptr, o['w'].ptr, o['z'].ptr, o['mean'].ptr,
                  o['rstd'].ptr, o['label'].ptr, _ptr(o['rw']), _ptr(o['den']), nden, 4.0, o['gloss'].ptr, o['dx'].ptr, lddx, o['dw'].ptr,
                  o['db'].ptr, o['dln_w'].ptr, o['dln_b'].ptr)
        return o, launch

    r = both(build, f'head_bce E={E} optional={optional}')[True]
    assert all(bool(torch.isfinite(r[k]).all()) for k in ('z', 'mean', 'rstd', 'loss', 'dx', 'dw', 'db', 'dln_w', 'dln_b'))
    other = torch.ones(T, dtype=torch.bool)
    other[rows] = False
    assert torch.equal(r['dx'][other], dx0[other]), 'head_bce_bwd touched a dx row that `rows` does not name'
    zr = torch.nn.functional.layer_norm(x[rows].double(), (E,), ln_w.double(), ln_b.double(), 1e-5) @ w.double() + b.double()
    assert float((r['z'].double() - zr).abs().max()) < 1e-4
    wt = rw.double() if optional else torch.ones(R, dtype=torch.float64)
    lr = (torch.nn.functional.binary_cross_entropy_with_logits(zr, label.double(), reduction='none') * wt).sum() / (5.0 if optional else 4.0)
    assert abs(float(r['loss']) - float(lr)) < 1e-4 * max(1.0, abs(float(lr)))


# ================================================================================================================ spatial attention
@pytest.mark.parametrize('N,HW,C', [(2, 256, 256), (3, 16, 128)])
def test_spatial_attention_ld_padded_equals_dense(N, HW, C):
    """q, k, v as the column blocks of one [N*HW, ld] tensor: ld = 3C (the fused q|k|v convolution) and larger."""
    g = _gen('spatial', N, HW, C)
    qkv = randn(g, N * HW, 3 * C, dtype=BF)
    nscr = N * HW * HW * 3 // 2 + 16

    def build(padded):
        ld = 3 * C + 8 * int(padded)
        o = dict(qkv=Guarded(qkv, ld=ld), scratch=out((nscr,), F32, partial=True), out=out((N * HW, C), BF))
        q = o['qkv'].ptr.value

        def launch():
            _call('mmvid_spatial_attention_ld', ctypes.c_void_p(q), ctypes.c_void_p(q + 2 * C), ctypes.c_void_p(q + 4 * C), ld, N, HW, C, C**-0.5,
                  o['scratch'].ptr, o['out'].ptr)
        return o, launch

    got = both(build, f'spatial_attention_ld {N}x{HW}x{C}', loose=('scratch',))[True]['out']
    q, k, v = (qkv[:, i * C:(i + 1) * C].double().view(N, HW, C) for i in range(3))
    ref = torch.softmax(q @ k.transpose(1, 2) * C**-0.5, -1) @ v
    assert bool(torch.isfinite(got.float()).all())
    assert float((got.double().view(N, HW, C) - ref).abs().max()) < 1.5e-2 * float(ref.abs().max())


# ========================================================================================================================= GroupNorm
@pytest.mark.parametrize('N,hw,C', [(3, 100, 128), (2, 2304, 128), (1, 64 * 5 + 8, 64), (5, 256, 512)])  # N*hw ragged against the 256-pixel tile
@pytest.mark.parametrize('x_bf16', [True, False])
def test_groupnorm_swish_guards_and_poison(N, hw, C, x_bf16):
    """No leading dimensions: guards and poison around x, w, b, the statistics scratch and both outputs, against the same call on
    plain tensors (bit for bit)."""
    from mmvid_amd import ops
    g = _gen('gn', N, hw, C)
    x = randn(g, N, hw, C, dtype=BF if x_bf16 else F32)
    w, b = randn(g, C) * 0.1 + 1, randn(g, C) * 0.1
    nst = N * (2 * C + 64 * ((hw + 63) // 64))
    o = dict(x=Guarded(x.view(-1)), w=Guarded(w), b=Guarded(b), st=out((nst,), F32, partial=True), y16=out((N * hw, C), BF), y32=out((N * hw, C), F32))
    _call('mmvid_groupnorm_swish_nhwc', o['x'].ptr, int(x_bf16), N, hw, C, o['w'].ptr, o['b'].ptr, 1e-6, 1, o['st'].ptr, 0, o['y16'].ptr, o['y32'].ptr)
    r = {k: gd.check(f'groupnorm {k}') for k, gd in o.items()}
    plain = ops.groupnorm_swish(x.view(N, hw, 1, C).cuda(), w.cuda(), b.cuda(), out_dtype=F32).cpu().view(N * hw, C)
    report_mismatch(r['y32'], plain, 'groupnorm: guarded call against the call on plain tensors')
    plain16 = ops.groupnorm_swish(x.view(N, hw, 1, C).cuda(), w.cuda(), b.cuda(), out_dtype=BF).cpu().view(N * hw, C)
    report_mismatch(r['y16'], plain16, 'groupnorm: bf16 output, guarded call against the call on plain tensors')
    assert bool(torch.isfinite(r['y32']).all())


@pytest.mark.parametrize('N,hw,C', [(3, 100, 128), (2, 2304, 128)])
def test_groupnorm_swish_split_guards_and_poison(N, hw, C):
    from mmvid_amd import ops
    g = _gen('gn_split', N, hw, C)
    x = randn(g, N, hw, C)
    w, b = randn(g, C) * 0.1 + 1, randn(g, C) * 0.1
    nst = N * (2 * C + 64 * ((hw + 63) // 64))
    o = dict(x=Guarded(x.view(-1)), w=Guarded(w), b=Guarded(b), st=out((nst,), F32, partial=True), planes=out((2, N * hw * C), BF))
    _call('mmvid_groupnorm_swish_nhwc_split', o['x'].ptr, N, hw, C, o['w'].ptr, o['b'].ptr, 1e-6, 1, o['st'].ptr, 0, o['planes'].ptr)
    r = {k: gd.check(f'groupnorm_split {k}') for k, gd in o.items()}
    plain = ops.groupnorm_swish_split(x.view(N, hw, 1, C).cuda(), w.cuda(), b.cuda()).cpu()
    report_mismatch(r['planes'].view(-1), plain.reshape(-1), 'groupnorm_split: guarded call against the call on plain tensors')
    assert bool(torch.isfinite(r['planes'].float()).all())


# ====================================================================================================================== grad_sqnorm
@pytest.mark.parametrize('n', [1, 4099, 1 << 20])
def test_grad_sqnorm_guards_and_atomic_bound(n):
    """mmvid_grad_sqnorm adds its block sums with fp32 atomics: n 2^-23 sum g^2 around fp64; mmvid_grad_sqnorm_det is the fixed-order
    form: two calls agree bit for bit.  NaN in front of and behind g in both."""
    g = randn(_gen('sqnorm', n), n)
    base = torch.tensor([3.5])
    ref, mag = base.double() + (g.double()**2).sum(), base.double() + (g.double()**2).sum()
    res = []
    for _ in range(2):
        gg, acc = Guarded(g), Guarded(base=base)
        _call('mmvid_grad_sqnorm', gg.ptr, n, acc.ptr)
        gg.check('g')
        res.append(acc.check('out_accum'))
    assert_within_atomic_bound(res[0], res[1], ref, mag, n + 1, f'grad_sqnorm n={n}')
    det = []
    for _ in range(2):
        gg, acc, part = Guarded(g), Guarded(base=base), out((2048,), F32, partial=True)
        _call('mmvid_grad_sqnorm_det', gg.ptr, n, part.ptr, acc.ptr)
        gg.check('g'), part.check('partials')
        det.append(acc.check('out_accum'))
    assert_same_bits(det[0], det[1], f'grad_sqnorm_det n={n}')
    assert_within_atomic_bound(det[0], det[1], ref, mag, n + 1, f'grad_sqnorm_det n={n}')


# ============================================================================================= gathers and the other guards-only kernels
def test_gather_rows_guards():
    g = _gen('gather')
    T, dim, rows = 50, 256, 77
    table, idx = randn(g, T, dim), torch.randint(0, T, (rows,), generator=g)
    for which in ('f32', 'bf16', 'both'):
        o = dict(table=Guarded(table), idx=Guarded(idx), o32=out((rows, dim), F32) if which != 'bf16' else None,
                 o16=out((rows, dim), BF) if which != 'f32' else None)
        _call('mmvid_gather_rows', o['table'].ptr, T, o['idx'].ptr, rows, dim, _ptr(o['o32']), _ptr(o['o16']))
        r = {k: gd.check(f'gather_rows {k}') for k, gd in o.items() if gd is not None}
        if 'o32' in r:
            report_mismatch(r['o32'], table[idx], 'gather_rows f32')
        if 'o16' in r:
            report_mismatch(r['o16'], table[idx].bfloat16(), 'gather_rows bf16')


def test_assemble_sequence_guards():
    from mmvid_amd import _lib
    g = _gen('assemble')
    B, L, E = 3, 11, 64
    tables = [randn(g, n, E) for n in (7, 13)]
    seg = torch.tensor([0] * 4 + [1] * 7, dtype=I32)
    ids = torch.cat([torch.randint(0, 7, (B, 4), generator=g), torch.randint(0, 13, (B, 7), generator=g)], 1)
    pos = randn(g, L, E)
    gt = [Guarded(t) for t in tables]
    o = dict(ids=Guarded(ids), seg=Guarded(seg), pos=Guarded(pos), out=out((B * L, E), F32))
    tp = (ctypes.c_void_p * 2)(*[t.ptr.value for t in gt])
    nrows = (ctypes.c_int64 * 2)(7, 13)
    _lib.device_faults(reset=True)
    _call('mmvid_assemble_sequence', ctypes.cast(tp, ctypes.POINTER(ctypes.c_void_p)), nrows, 2, o['ids'].ptr, o['seg'].ptr, o['pos'].ptr, B, L, E,
          o['out'].ptr)
    assert _lib.device_faults(reset=True)[:2] == [0, 0]
    for t in gt:
        t.check('table')
    r = {k: gd.check(f'assemble_sequence {k}') for k, gd in o.items()}
    want = torch.stack([torch.stack([tables[int(seg[l])][int(ids[bb, l])] + pos[l] for l in range(L)]) for bb in range(B)]).view(B * L, E)
    report_mismatch(r['out'], want, 'assemble_sequence')


@pytest.mark.parametrize('with_record', [True, False])
def test_decode_embed_record_guards(with_record):
    g = _gen('embed_record')
    B, E, T, P = 5, 768, 30, 20
    table, pos_rows = randn(g, T, E), randn(g, P, E)
    tok = torch.randint(0, T, (B,), generator=g)
    posv, off, rec0, rld = 9, 3, 4, 16
    o = dict(tok=Guarded(tok), table=Guarded(table), pos_rows=Guarded(pos_rows), pos=Guarded(torch.tensor([posv], dtype=I32)), x=out((B, E), F32),
             record=out((B, 8), I64, rld, partial=True) if with_record else None)
    _call('mmvid_decode_embed_record', o['tok'].ptr, o['table'].ptr, T, o['pos_rows'].ptr, o['pos'].ptr, off, B, E, o['x'].ptr, _ptr(o['record']),
          rld, rec0)
    r = {k: gd.check(f'decode_embed_record {k}') for k, gd in o.items() if gd is not None}
    report_mismatch(r['x'], table[tok] + pos_rows[posv + off], 'decode_embed_record x')
    if with_record:
        want = Guarded(role='out', shape=(B, 8), dtype=I64, device='cpu').window()
        want[:, posv - rec0] = tok
        report_mismatch(r['record'], want, 'decode_embed_record record')


def test_rows_pack_and_merge_guards():
    g = _gen('rows_pack')
    V, E, n = 40, 64, 12
    W = randn(g, V, E)
    ids = torch.tensor([5, 9, 5, 0, 39, 9, 9, 17, 3, 3, 21, 0])
    o = dict(W=Guarded(W), ids=Guarded(ids), uid=out((n,), I64), rows=out((n, E), F32))
    _call('mmvid_rows_pack', o['W'].ptr, V, E, o['ids'].ptr, n, o['uid'].ptr, o['rows'].ptr)
    r = {k: gd.check(f'rows_pack {k}') for k, gd in o.items()}
    uid = r['uid']
    live = uid[uid >= 0]
    assert sorted(live.tolist()) == sorted(set(ids.tolist())) and int((uid == -1).sum()) == n - live.numel() and bool((uid >= -1).all())
    report_mismatch(r['rows'], torch.where((uid >= 0)[:, None], W[uid.clamp_min(0)], torch.zeros(())), 'rows_pack rows')
    W2 = randn(g, V, E)
    m = dict(W=Guarded(base=W2), ids=Guarded(uid), rows=Guarded(r['rows']))
    _call('mmvid_rows_merge', m['W'].ptr, V, E, m['ids'].ptr, m['rows'].ptr, n)
    r2 = {k: gd.check(f'rows_merge {k}') for k, gd in m.items()}
    want = W2.clone()
    want[live] += W[live]
    report_mismatch(r2['W'], want, 'rows_merge')
