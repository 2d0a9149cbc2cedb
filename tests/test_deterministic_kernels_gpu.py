"""Deterministic mode, kernel level.

Ordered pins: the embedding-table gradient, mmvid_colsum_bf16_det and the loss sum of mmvid_cross_entropy_fwd_det are compared BIT
FOR BIT with a numpy restatement of the order include/mmvid_hip.h documents; each pin also shows, on the CPU, that the same
restatement taken in reversed order gives other bits (a pin that could not tell two orders apart would prove nothing).
Repeatability pins: where the addends live in registers (attention dbias, the dX GEMM's out_colsum, split-K into out_f32, the
LayerNorm backward's dw / db / dx_colsum) three calls on equal inputs -- one of them next to a busy side stream -- give
byte-identical outputs, and the atomic path agrees within the tolerance the operator's existing test uses.

Inputs make the order matter: randn * 2^k, k uniform in [-6, 6] (bf16-rounded where the operand is bf16)."""
import numpy as np
import pytest
import torch

import mmvid_amd
from test_kernels_gpu import DEV, close

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(autouse=True)
def restore_mode():
    before = mmvid_amd.is_deterministic()
    yield
    mmvid_amd.set_deterministic(before)


def wild(*shape, seed, bf16=False):
    """randn * 2^k, k uniform in [-6, 6], as fp32 on the host (bf16-rounded when the operand is bf16)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())
    return v.bfloat16().float() if bf16 else v


def chain(rows, start=None):
    """((start + rows[0]) + rows[1]) + ... in fp32, vectorised over the trailing axes; start = 0.0f when None."""
    acc = np.zeros(rows.shape[1:], f32) if start is None else start.astype(f32).copy()
    for r in rows:
        acc = (acc + r).astype(f32)
    return acc


class Busy:
    """Keeps an unrelated elementwise kernel running on a side stream while the body runs: perturbs the arrival order of blocks."""

    def __init__(self):
        self.side = torch.cuda.Stream()
        self.buf = torch.ones(1 << 26, device=DEV)

    def __enter__(self):
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            for _ in range(40):
                self.buf.mul_(1.0001)
        return self

    def __exit__(self, *exc):
        torch.cuda.current_stream().wait_stream(self.side)
        torch.cuda.synchronize()
        return False


def three_runs(fn):
    """fn() -> tuple of tensors; three calls, the second next to a busy side stream: byte-identical."""
    a = [t.clone() for t in fn()]
    with Busy():
        b = [t.clone() for t in fn()]
    c = [t.clone() for t in fn()]
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        assert torch.equal(x, y), f'output {i}: {(x != y).sum().item()} elements differ next to a busy stream'
        assert torch.equal(x, z), f'output {i}: {(x != z).sum().item()} elements differ between two quiet runs'
    return a


# ------------------------------------------------------------------------------------------------- ordered pins
def embedding_reference(prior, table_rows, ids, seg, dx, L, reverse=False):
    """include/mmvid_hip.h, mmvid_assemble_sequence_bwd_det: list ascending in r, chunks of 64 chained in list order, chunk sums
    chained in chunk order, added once to the gradient."""
    out = [None if p is None else p.copy() for p in prior]
    flat, n = ids.reshape(-1), ids.size
    table = seg[np.arange(n) % L]
    for s, rows_s in enumerate(table_rows):
        if out[s] is None:
            continue
        mine = np.nonzero((table == s) & (flat >= 0) & (flat < rows_s))[0]
        for d in np.unique(flat[mine]):
            lst = mine[flat[mine] == d]  # ascending r
            if reverse:
                lst = lst[::-1]
            sums = np.stack([chain(dx[lst[c:c + 64]]) for c in range(0, len(lst), 64)])
            out[s][d] = (out[s][d] + chain(sums)).astype(f32)
    return out


def test_embedding_gradient_is_the_documented_order():
    from mmvid_amd import ops
    B, L, E = 80, 200, 768
    table_rows = [20000, 17, 64, 50]  # (20,000 destinations: the exclusive scan runs over several of its 8,192-wide tiles)
    rng = np.random.RandomState(5)
    seg = np.repeat(np.arange(4), 50).astype(np.int32)  # 50 positions per table
    ids = np.stack([rng.randint(0, table_rows[s], B) for s in seg], 1).astype(np.int64)  # [B, L]
    heavy = rng.rand(B, L) < 0.85
    ids[:, 50:100][heavy[:, 50:100]] = 16  # one row of table 1 carries most of its positions (as [MASK] does)
    ids[:, 100:150][heavy[:, 100:150] & (rng.rand(B, 50) < 0.5)] = 3
    ids[0, 0], ids[1, 60], ids[2, 110], ids[3, 61] = -1, 17, 64, 1 << 40  # blank / one past the table / far outside
    n_heavy = int(((ids[:, 50:100] == 16)).sum())
    assert n_heavy > 3000  # one id carries thousands of rows: more than 47 chunks at the second level
    dx = wild(B, L, E, seed=1).numpy()
    prior = [wild(r, E, seed=10 + s).numpy() for s, r in enumerate(table_rows)]
    prior[3] = None  # a frozen table
    want = embedding_reference(prior, table_rows, ids, seg, dx.reshape(-1, E), L)
    other = embedding_reference(prior, table_rows, ids, seg, dx.reshape(-1, E), L, reverse=True)
    assert any(not np.array_equal(a, b) for a, b in zip(want[:3], other[:3])), 'the reversed order gives the same bits: the pin is blind'
    assert not np.array_equal(want[1][16], other[1][16])
    ids_d, seg_d, dx_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(seg).to(DEV), torch.from_numpy(dx).to(DEV)
    mmvid_amd.set_deterministic(True)

    def run():
        gts = [None if p is None else torch.from_numpy(p).to(DEV) for p in prior]
        dpos = torch.empty(L, E, device=DEV)
        ops.assemble_sequence_bwd(gts, table_rows, ids_d, seg_d, dx_d, dpos)
        return [g for g in gts if g is not None] + [dpos]

    got = three_runs(run)
    for s in range(3):
        diff = got[s].cpu().numpy() != want[s]
        assert not diff.any(), f'table {s}: {diff.sum()} elements differ from the documented order (rows {np.nonzero(diff.any(1))[0][:8]})'
    assert np.array_equal(got[3].cpu().numpy(), chain(dx))  # dpos: a chain over b
    mmvid_amd.set_deterministic(False)
    for s, g in enumerate(run()[:3]):
        close(g, got[s], 1e-5, f'embedding gradient, table {s}: atomic path vs deterministic')


def colsum_reference(dy, prior, reverse=False):
    sums = []
    for m0 in range(0, dy.shape[0], 256):
        blk = dy[m0:m0 + 256]
        groups = [chain(blk[j::8][::-1] if reverse else blk[j::8]) for j in range(8)]
        sums.append(chain(np.stack(groups[::-1] if reverse else groups)))
    sums = np.stack(sums[::-1] if reverse else sums)
    return (prior + chain(sums)).astype(f32)


@pytest.mark.parametrize('M,N', [(3000, 768), (8, 3072), (257, 264)])
def test_colsum_bf16_det_is_the_documented_order(M, N):
    from mmvid_amd import ops
    dy = wild(M, N, seed=M + N, bf16=True)
    prior = wild(N, seed=3).numpy()
    want = colsum_reference(dy.numpy(), prior)
    flipped = (want != colsum_reference(dy.numpy(), prior, reverse=True)).mean()
    print(f'colsum {M}x{N}: the reversed order changes {flipped:.0%} of the columns')
    assert flipped > 0, 'the reversed order gives the same bits: the pin is blind'
    dy_d = dy.to(DEV).bfloat16()
    mmvid_amd.set_deterministic(True)

    def run():
        db = torch.from_numpy(prior).to(DEV)
        ops.colsum_bf16(dy_d, db)
        return (db, )

    got = three_runs(run)[0]
    assert np.array_equal(got.cpu().numpy(), want), f'{(got.cpu().numpy() != want).sum()} of {N} columns differ from the documented order'
    mmvid_amd.set_deterministic(False)
    close(run()[0], got, 2e-5, f'colsum {M}x{N}: atomic path vs deterministic')


def test_cross_entropy_loss_sum_is_the_documented_order():
    from mmvid_amd import _lib, ops
    rows, V = 3474, 1024
    logits = wild(rows, V, seed=7)
    g = torch.Generator().manual_seed(8)
    target = torch.randint(0, V, (rows, ), generator=g)
    for name, select in (('mask', torch.rand(rows, generator=g) < 0.4), ('all', None), ('few', torch.arange(rows) % 97 == 5)):
        lg, tg = logits.to(DEV), target.to(DEV)
        sel = select.to(torch.uint8).to(DEV) if select is not None else None
        prior = 3.25

        def run(det=True):
            lse = torch.empty(rows, device=DEV)
            loss = torch.full((1, ), prior, device=DEV)
            if det:
                ws = torch.empty(rows, device=DEV)
                _lib.call('mmvid_cross_entropy_fwd_det', ops._p(lg), V, ops._p(tg), ops._p(sel), rows, V, ops._p(lse), ops._p(loss),
                          ops._p(ws), ws.numel() * 4, ops._stream())
            else:
                _lib.call('mmvid_cross_entropy_fwd', ops._p(lg), V, ops._p(tg), ops._p(sel), rows, V, ops._p(lse), ops._p(loss), ops._stream())
            return lse, loss

        lse, loss = three_runs(run)
        # the addends, recomputed from the lse the kernel returned: the same fp32 expression
        term = (lse.cpu().numpy() - logits.numpy()[np.arange(rows), target.numpy()]).astype(f32)
        if select is not None:
            term[~select.numpy()] = 0
            assert (lse.cpu().numpy()[~select.numpy()] == 0).all()

        def total(t, start=prior):
            parts = np.array([chain(t[k::256]) for k in range(256)], f32)
            return (f32(start) + chain(parts)).astype(f32)

        want = total(term)
        assert want != total(term[::-1].copy()), f'{name}: the reversed order gives the same bits: the pin is blind'
        assert loss.item() == want.item(), f'{name}: loss_sum {loss.item()!r} != documented order {want.item()!r}'
        lse0, loss0 = run(det=False)
        assert torch.equal(lse0, lse)
        close(loss0, loss, 1e-5, f'cross entropy loss sum ({name}): atomic path vs deterministic')
        # and through the wrapper the training step uses
        mmvid_amd.set_deterministic(True)
        lse_w, loss_w = ops.cross_entropy_fwd(lg, tg, sel)
        mmvid_amd.set_deterministic(False)
        assert torch.equal(lse_w, lse) and loss_w.item() == total(term, 0.0).item()


# ------------------------------------------------------------------------------------------------- repeatability pins
def both_modes(fn, tols, what):
    """fn() -> tuple of tensors.  Mode 1: three byte-identical runs; mode 0 agrees within tols (the existing tests' tolerances)."""
    mmvid_amd.set_deterministic(True)
    det = three_runs(fn)
    mmvid_amd.set_deterministic(False)
    atomic = fn()
    for i, tol in enumerate(tols):
        close(atomic[i], det[i], tol, f'{what}, output {i}: atomic path vs deterministic')
    return det


def test_attention_dbias_repeats():
    from mmvid_amd import ops
    B, L, H, E = 3, 579, 12, 768
    qkv = (torch.randn(B * L, 3 * E, generator=torch.Generator().manual_seed(0)) * 0.5).to(DEV).bfloat16()
    dO = wild(B * L, E, seed=1, bf16=True).to(DEV).bfloat16()
    prior = wild(3 * E, seed=2).to(DEV)
    mask = ('rows', [(65, 65), (66, 66)])
    out, lse2 = ops.attention_fwd(qkv, B, L, H, mask)

    def run():
        db = prior.clone()
        dqkv = ops.attention_bwd(qkv, out, dO, lse2, B, L, H, mask, dbias=db)
        return db, dqkv

    db, dqkv = both_modes(run, (1e-2, 0.0), 'attention backward')
    close(db - prior, dqkv.float().sum(0), 1e-2, 'dbias against the column sums of the stored dqkv')


@pytest.mark.parametrize('M,N,K', [(3474, 3072, 768), (333, 3072, 768), (100, 264, 72)])
def test_gemm_out_colsum_repeats(M, N, K):
    """The dX GEMM of c_proj (QuickGELU' of the saved pre-activation, packed bf16 result, column sums = c_fc's bias gradient) on the
    256 x 128 persistent blocks (M = 3474), the 128-row blocks (M = 333), and a plain fp32 result with column sums (LDS epilogue)."""
    from mmvid_amd import ops
    dY = wild(M, K, seed=M, bf16=True).to(DEV).bfloat16()
    W = (torch.randn(K, N, generator=torch.Generator().manual_seed(N)) * 0.05).to(DEV).bfloat16()
    pre = torch.randn(M, N, generator=torch.Generator().manual_seed(K)).to(DEV).bfloat16()
    prior = wild(N, seed=4).to(DEV)

    def run():
        cs, cs32 = prior.clone(), prior.clone()
        out = ops.gemm(dY, W, b_kmajor=True, dact_pre=pre, colsum=cs)
        o32 = ops.gemm(dY, W, b_kmajor=True, out_dtype=torch.float32, colsum=cs32)
        return cs, cs32, out, o32

    cs, cs32, out, o32 = both_modes(run, (2e-3, 2e-3, 0.0, 0.0), f'dX GEMM {M}x{N}x{K}')
    close(cs - prior, out.float().sum(0), 5e-3, 'out_colsum against the column sums of the stored bf16 result')
    close(cs32 - prior, o32.sum(0), 1e-4, 'out_colsum against the column sums of the fp32 result')


@pytest.mark.parametrize('splitk', [3, 8])
def test_gemm_splitk_repeats(splitk):
    from mmvid_amd import ops
    M, N, K = 776, 264, 1043
    A = wild(K, M, seed=3, bf16=True).to(DEV).bfloat16()
    Bm = wild(K, N, seed=4, bf16=True).to(DEV).bfloat16()
    base = wild(M, N, seed=5).to(DEV)
    bias = wild(N, seed=6).to(DEV)

    def run():
        out, outb = base.clone(), base.clone()
        ops.gemm(A, Bm, a_kmajor=True, b_kmajor=True, out=out, accumulate=True, splitk=splitk)
        ops.gemm(A, Bm, a_kmajor=True, b_kmajor=True, out=outb, accumulate=True, splitk=splitk, bias=bias)
        return out, outb

    out, outb = both_modes(run, (2e-4, 2e-4), f'split-K {splitk}')
    ref = base + A.float().t() @ Bm.float()
    close(out, ref, 2e-4, 'split-K through slabs against fp32 torch')
    close(outb, ref + bias, 2e-4, 'split-K through slabs with a bias against fp32 torch')


@pytest.mark.parametrize('rows,E', [(3474, 768), (77, 512), (10, 768)])
def test_layernorm_backward_repeats(rows, E):
    from mmvid_amd import ops
    x = (torch.randn(rows, E, generator=torch.Generator().manual_seed(1)) * 2 + 0.5).to(DEV)
    w = (torch.randn(E, generator=torch.Generator().manual_seed(2)) * 0.1 + 1).to(DEV)
    b = torch.zeros(E, device=DEV)
    _, mean, rstd = ops.layernorm_fwd(x, w, b, out_dtype=torch.float32)
    dy = wild(rows, E, seed=4).to(DEV)
    base, prior = wild(rows, E, seed=5).to(DEV), wild(3, E, seed=6).to(DEV)

    def run():
        dx, dw, db, cs = base.clone(), prior[0].clone(), prior[1].clone(), prior[2].clone()
        ops.layernorm_bwd(dy, x, mean, rstd, w, dx=dx, add=True, dw=dw, db=db, dx_colsum=cs)
        return dw, db, cs, dx

    both_modes(run, (1e-4, 1e-4, 1e-5, 0.0), f'LayerNorm backward {rows}x{E}')


def test_layernorm_atomic_branch_is_refused():
    from mmvid_amd import _lib, ops
    rows, E = 40, 768
    x = torch.randn(rows, E, device=DEV)
    w = torch.ones(E, device=DEV)
    _, mean, rstd = ops.layernorm_fwd(x, w, torch.zeros(E, device=DEV), out_dtype=torch.float32)
    dy, dx, dw = torch.randn(rows, E, device=DEV), torch.zeros(rows, E, device=DEV), torch.zeros(E, device=DEV)
    args = (ops._p(dy), E, ops._p(x), E, ops._p(mean), ops._p(rstd), ops._p(w), rows, E, ops._p(dx), E, 0, None, ops._p(dw), None, None)
    mmvid_amd.set_deterministic(True)
    with pytest.raises(_lib.MMVIDError, match='deterministic mode refuses the atomic'):
        _lib.call('mmvid_layernorm_bwd', *args, ops._stream())
    with pytest.raises(_lib.MMVIDError, match='mmvid_layernorm_bwd_ws'):
        _lib.call('mmvid_layernorm_bwd_ws', *args, None, 0, ops._stream())
    assert not dw.any()  # refused before any launch
    _lib.call('mmvid_layernorm_bwd', *args[:13], None, None, None, ops._stream())  # no sums asked for: nothing to refuse
    ops.layernorm_bwd(dy, x, mean, rstd, w, dx=dx, dw=dw)  # the wrapper brings its workspace
    assert dw.any()
    mmvid_amd.set_deterministic(False)
    _lib.call('mmvid_layernorm_bwd', *args, ops._stream())  # mode 0: the atomic branch as before


def test_tower_backward_on_a_workspace_sized_before_the_switch():
    """mmvid_tower_workspace reports the same bytes in both modes (the slabs live in an idle region of the scratch arena), so a tower
    whose arenas were sized and used in mode 0 runs its deterministic backward in place: repeatable, and close to mode 0.
    (1e-4 of the largest element: the two modes add the same <= 450 fp32 terms per bias element in another order, an error of at most
    450 * 2^-24 = 2.7e-5 of the sum of their magnitudes; everything that is not a bias gradient runs the same kernels.)"""
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    torch.manual_seed(0)
    L = 150
    tw = OpenAICLIPTransformer(L, 'openai_clip_visual', causal=True, layers=2).to(DEV).train()
    x0 = torch.randn(3, L, 768, device=DEV) * 0.5
    gy = wild(3, L, 768, seed=9).to(DEV)
    names = [n for n, _ in tw.named_parameters()]

    def run():
        tw.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        tw(x).backward(gy)
        return [x.grad] + [p.grad for _, p in tw.named_parameters()]

    mmvid_amd.set_deterministic(False)
    atomic = [t.clone() for t in run()]
    mmvid_amd.set_deterministic(True)
    det = three_runs(run)
    for n, a, d in zip(['dx'] + names, atomic, det):
        close(a, d, 1e-4, f'tower backward {n}: atomic path vs deterministic')
    biases = [i + 1 for i, n in enumerate(names) if n.endswith('bias')]
    assert len(biases) >= 8 and all(det[i].abs().max() > 0 for i in biases)
