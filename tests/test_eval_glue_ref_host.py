"""tests/eval_glue_ref.py against independent torch routes in fp64, and the conditions the GPU tests (tests/test_eval_glue_gpu.py)
rest on: the fp32 evaluation of each reference formula sits inside the worst-case bound of every GPU case (the reference alone
stays within the cap), and every hard row of the generators has the property it is there for.  No GPU, nothing read from outside
the repository."""
import pytest
import torch
import torch.nn.functional as F

import eval_glue_ref as ref
from eval_glue_ref import EPS, U23

F64 = torch.float64


def _close(a, b, rel, what):
    err = float((a - b).abs().max())
    assert err <= rel * float(b.abs().max()), f'{what}: {err:.3e} against {rel:.0e} x {float(b.abs().max()):.3e}'


# ------------------------------------------------------------------------------------------------ references against torch, fp64
@pytest.mark.parametrize('N,T,E', ref.ASSEMBLE_CASES)
def test_image_assemble_against_torch(N, T, E):
    c = ref.assemble_inputs(N, T, E)
    seq = torch.cat([c['cls'].double().expand(N, 1, E), c['feat'].double().view(N, T - 1, E)], 1) + c['pos'].double()
    want = F.layer_norm(seq, (E,), c['w'].double(), c['b'].double(), EPS).view(N * T, E)
    _close(ref.image_assemble(c['feat'], c['cls'], c['pos'], c['w'], c['b'], EPS, N, T), want, 1e-12, 'image_assemble')


@pytest.mark.parametrize('B,L,E,D,given', ref.POOL_CASES)
@pytest.mark.parametrize('l2norm', [0, 1])
def test_pool_project_against_torch(B, L, E, D, given, l2norm):
    c = ref.pool_inputs(B, L, E, D, given)
    x = c['x'].double()
    picked = torch.stack([x[s, 0 if c['rows'] is None else min(max(int(c['rows'][s]), 0), L - 1)] for s in range(B)])
    h = F.layer_norm(picked, (E,), c['w'].double(), c['b'].double(), EPS)
    want = h @ c['proj'].double()
    if l2norm:
        want = F.normalize(want, dim=-1, eps=0.0)
    got, mag = ref.pool_project(c['x'], c['rows'], c['w'], c['b'], EPS, c['proj'], l2norm)
    _close(got, want, 1e-12, 'pool_project')
    _close(mag, torch.einsum('bk,kd->bd', h.abs(), c['proj'].double().abs()), 1e-12, 'pool_project sum |terms|')
    if l2norm:
        _close((got * got).sum(-1), torch.ones(B, dtype=F64), 1e-12, 'unit norm')


def test_pool_rows_clamp_and_default():
    x = torch.arange(2 * 4 * 3, dtype=torch.float32).view(2, 4, 3)
    assert torch.equal(ref.pooled_rows(x, None), x[:, 0])
    assert torch.equal(ref.pooled_rows(x, torch.tensor([-3, 9], dtype=torch.int32)), torch.stack([x[0, 0], x[1, 3]]))
    rows = ref.pool_inputs(5, 77, 512, 512, True)['rows'].tolist()
    assert rows[0] == -3 and rows[-1] == 77 + 5 and {0, 76}.issubset(rows) and any(0 < r < 76 for r in rows)
    assert all(-8 <= r < 77 + 8 for r in rows)  # an unclamped read stays inside the guard around x


@pytest.mark.parametrize('B,T,D', ref.PAIR_CASES)
def test_pair_scores_against_torch(B, T, D):
    c = ref.pair_inputs(B, T, D)
    got, mag = ref.pair_scores(c['img'], c['txt'], B, T)
    txt = c['txt'].double().repeat_interleave(T, 0)
    _close(got, torch.einsum('fd,fd->f', c['img'].double(), txt), 1e-12, 'pair_scores')
    _close(mag, torch.einsum('fd,fd->f', c['img'].double().abs(), txt.abs()), 1e-12, 'pair_scores sum |terms|')
    assert len({tuple(r.tolist()) for r in c['txt']}) == B  # every txt row is distinct


@pytest.mark.parametrize('N,To,C,ncls', ref.HEAD_CASES)
def test_i3d_head_against_torch(N, To, C, ncls):
    """The expression of tests/i3d_oracle.py::forward: avg_pool3d (2, 7, 7), the 1x1x1 logits convolution with bias, mean over time."""
    c = ref.head_inputs(N, To, C, ncls)

    def torch_route(x, w, b):
        y = F.avg_pool3d(x.permute(0, 4, 1, 2, 3), (2, 7, 7), 1)
        y = F.conv3d(y, w.view(ncls, C, 1, 1, 1), b)
        return y.squeeze(3).squeeze(3).mean(2)

    got, mag = ref.i3d_head(c['x'], c['w'], c['b'])
    _close(got, torch_route(c['x'].double(), c['w'].double(), c['b'].double()), 1e-12, 'i3d_head')
    _close(mag, torch_route(c['x'].double().abs(), c['w'].double().abs(), c['b'].double().abs()), 1e-12, 'i3d_head |terms|')


def test_i3d_fold_is_the_stem_convolution_operand():
    """In fp64 the stride-2 7x7x7 TF-SAME convolution of the raw clip equals the (7, 7, 1)-window, stride (2, 2, 1) convolution over
    the folded 24-channel operand: this pins the front pad of 2 columns and the 3 kw + c channel order."""
    g = torch.Generator().manual_seed(5)
    clip = torch.randn(1, 3, 3, 224, 224, generator=g).bfloat16().float()  # [n, c, t, y, x], bf16-representable
    k = torch.randn(2, 3, 7, 7, 7, generator=g, dtype=F64)  # [o, c, kt, kh, kw]
    want = F.conv3d(F.pad(clip.double(), (2, 3, 2, 3, 3, 3)), k, stride=2)  # TF-SAME: t 3 + 3, y and x 2 + 3
    folded = ref.i3d_fold(clip.permute(0, 2, 3, 4, 1).contiguous())  # [1, 3, 224, 112, 24] bf16
    assert folded.dtype == torch.bfloat16 and folded.shape == (1, 3, 224, 112, 24)
    assert int((folded[..., 21:] != 0).sum()) == 0
    k24 = torch.zeros(2, 24, 7, 7, 1, dtype=F64)
    k24[:, :21, :, :, 0] = k.permute(0, 4, 1, 2, 3).reshape(2, 21, 7, 7)  # channel 3 kw + c
    got = F.conv3d(F.pad(folded.double().permute(0, 4, 1, 2, 3), (0, 0, 2, 3, 3, 3)), k24, stride=(2, 2, 1))
    assert got.shape == want.shape == (1, 2, 2, 112, 112)
    _close(got, want, 1e-12, 'folded convolution')


def test_i3d_fold_inputs_hold_ties_and_signed_zeros():
    v, ties = ref.fold_inputs(1, 1)
    flat = v.view(-1)
    tb = flat[ties].view(torch.int32)
    assert bool(((tb & 0xFFFF) == 0x8000).all())
    lo = (tb >> 16 << 16).view(torch.float32).double()
    hi = ((tb >> 16) + 1 << 16).view(torch.float32).double()
    assert bool(((flat[ties].double() - lo) == (hi - flat[ties].double())).all())  # half-way between two bf16 values
    r = flat[ties].bfloat16().view(torch.int16)
    assert bool((r & 1 == 0).all())  # the cast rounds a tie to the even neighbour ...
    up = int((r.to(torch.int32) & 0xFFFF != ((tb >> 16) & 0xFFFF)).sum())
    assert ref.N_TIES // 4 < up < 3 * ref.N_TIES // 4  # ... which is the upper one for about half of them
    zero_bits = flat[flat == 0].view(torch.int32)
    assert int((zero_bits == 0).sum()) >= ref.N_TIES // 2 and int((zero_bits != 0).sum()) >= ref.N_TIES // 2


# --------------------------------------------------------------------------------------- the fp32 yardstick inside every case's cap
@pytest.mark.parametrize('B,L,E,D,given', ref.POOL_CASES)
def test_pool_project_fp32_eval_within_the_bound(B, L, E, D, given):
    c = ref.pool_inputs(B, L, E, D, given)
    args = (c['x'], c['rows'], c['w'], c['b'], EPS, c['proj'])
    y64, mag = ref.pool_project(*args, 0)
    y32, _ = ref.fp32_eval('pool_project', *args, 0)
    assert y32.dtype == torch.float32
    bound = ref.pool_bound(c, ref.pool_hidden(*args[:5]), ref.pool_hidden(*args[:5], torch.float32), mag)
    used = float(((y32.double() - y64).abs() / bound).max())
    print(f'pool_project {B}x{L}x{E}x{D}: the fp32 evaluation uses {used:.4f} of the worst-case bound')
    assert used <= 1.0
    # l2norm = 1 against the un-normalised fp32 values normalised in fp64
    n32, _ = ref.fp32_eval('pool_project', *args, 1)
    want = y32.double() / (y32.double()**2).sum(-1, keepdim=True).sqrt()
    used = float(((n32.double() - want).abs() / ((D + 4) * U23 * want.abs() + 1e-300)).max())
    print(f'pool_project {B}x{L}x{E}x{D} l2norm: the fp32 evaluation uses {used:.4f} of (D + 4) 2^-23 |value|')
    assert used <= 1.0


@pytest.mark.parametrize('B,T,D', ref.PAIR_CASES)
def test_pair_scores_fp32_eval_within_the_bound(B, T, D):
    c = ref.pair_inputs(B, T, D)
    y64, mag = ref.pair_scores(c['img'], c['txt'], B, T)
    y32, _ = ref.fp32_eval('pair_scores', c['img'], c['txt'], B, T)
    used = float(((y32.double() - y64).abs() / ((D + 1) * U23 * mag)).max())
    print(f'pair_scores {B}x{T}x{D}: the fp32 evaluation uses {used:.4f} of the worst-case bound')
    assert y32.dtype == torch.float32 and used <= 1.0


@pytest.mark.parametrize('N,To,C,ncls', ref.HEAD_CASES)
def test_i3d_head_fp32_eval_within_the_bound(N, To, C, ncls):
    c = ref.head_inputs(N, To, C, ncls)
    y64, mag = ref.i3d_head(c['x'], c['w'], c['b'])
    y32, _ = ref.fp32_eval('i3d_head', c['x'], c['w'], c['b'])
    used = float(((y32.double() - y64).abs() / (ref.head_K(To, C) * U23 * mag)).max())
    print(f'i3d_head {N}x{To}x{C}x{ncls}: the fp32 evaluation uses {used:.2e} of the worst-case bound')
    assert y32.dtype == torch.float32 and used <= 1.0


@pytest.mark.parametrize('N,T,E', ref.ASSEMBLE_CASES)
def test_image_assemble_fp32_eval_is_a_yardstick(N, T, E):
    """The assemble has the tight bar alone: its yardstick must be an fp32 evaluation (not fp64 in disguise) and far below what a
    wrong eps does to the hard rows, or the bar would pass it."""
    c = ref.assemble_inputs(N, T, E)
    args = (c['feat'], c['cls'], c['pos'], c['w'], c['b'])
    y64 = ref.image_assemble(*args, EPS, N, T)
    y32 = ref.fp32_eval('image_assemble', *args, EPS, N, T)
    bar = ref.tight_bar(y32, y64)
    assert y32.dtype == torch.float32 and 0 < float((y32.double() - y64).abs().max())
    moved = (ref.image_assemble(*args, 0.1 * EPS, N, T) - y64).abs()
    for name, rows in c['hard'].items():
        if name != 'cls':
            print(f'image_assemble {N}x{T}x{E}: eps / 10 moves the {name} row by {float(moved[rows].max()):.3f}, the bar is {bar:.2e}')
            assert float(moved[rows].max()) >= 50 * bar


# ------------------------------------------------------------------------------------------------------ the hard rows are hard
@pytest.mark.parametrize('N,T,E', ref.ASSEMBLE_CASES)
def test_image_assemble_hard_rows(N, T, E):
    c = ref.assemble_inputs(N, T, E)
    seq = torch.cat([c['cls'].double().expand(N, 1, E), c['feat'].double().view(N, T - 1, E)], 1) + c['pos'].double()
    seq = seq.view(N * T, E)
    mean, var = seq.mean(1), seq.var(1, unbiased=False)
    hard = c['hard']
    assert hard['cls'] == [n * T for n in range(N)] and 'std1e-3' in hard and ('std1e-2' in hard or N * (T - 1) == 1)
    for r in hard['cls']:
        assert float(mean[r].abs() / var[r].sqrt()) >= 50  # E[x^2] - mean^2 in fp32 keeps no digit of this variance
    for r in hard['std1e-3']:
        assert 0.05 <= float(var[r]) / EPS <= 0.2  # the variance is below eps
    for r in hard.get('std1e-2', []):
        assert 5 <= float(var[r]) / EPS <= 20  # eps is about 10 % of the variance
    # rows differ from each other by much more than any bar: a row taken from the wrong place shows
    assert len({round(float(m), 6) for m in c['pos'].double().mean(1)}) == T
    assert len({round(float(m), 6) for m in c['feat'].double().mean(1)}) == N * (T - 1)


@pytest.mark.parametrize('B,L,E,D,given', ref.POOL_CASES)
def test_pool_project_hard_rows(B, L, E, D, given):
    c = ref.pool_inputs(B, L, E, D, given)
    picked = ref.pooled_rows(c['x'], c['rows']).double()
    var = picked.var(1, unbiased=False)
    assert c['hard']['std1e-3'] == 0 and 0.05 <= float(var[0]) / EPS <= 0.2
    if B >= 3:
        assert c['hard']['std1e-2'] == B - 1 and 5 <= float(var[B - 1]) / EPS <= 20
    if given:
        eff = c['rows'].clamp(0, L - 1).tolist()
        assert L - 1 in eff and (B < 3 or 0 in eff) and (B < 2 or L < 3 or any(0 < r < L - 1 for r in eff))
    if D > 1:  # (a single output column has the norm of that one value)
        norm = ref.pool_project(c['x'], c['rows'], c['w'], c['b'], EPS, c['proj'], 0)[0].norm(dim=1)
        for s in range(B - 1):
            ratio = float(norm[s + 1] / norm[s])
            assert max(ratio, 1 / ratio) >= 2, (s, norm.tolist())
    # every row the kernel would read if it ignored `rows`, or took a neighbour, is an ordinary draw over the whole width
    at = ref.pooled_rows(torch.arange(L)[None, :, None].expand(B, L, 1), c['rows'])[:, 0]
    others = torch.ones(B, L, dtype=torch.bool)
    others[torch.arange(B), at] = False
    if L > 1:
        assert float(c['x'][others].double().var(-1, unbiased=False).min()) > 0.1


@pytest.mark.parametrize('N,To,C,ncls', ref.HEAD_CASES)
def test_i3d_head_inputs(N, To, C, ncls):
    c = ref.head_inputs(N, To, C, ncls)
    means = c['x'].double().mean((0, 2, 3, 4))
    assert bool((means[1:] - means[:-1] > 0.25).all())  # the time steps differ: a window one step off shows
    pooled = (c['x'].double().view(N, To, 49, C)[:, :-1].mean(2) + c['x'].double().view(N, To, 49, C)[:, 1:].mean(2)) / 2
    wp = (pooled @ c['w'].double().t()).abs().mean()
    assert 0.1 <= float(c['b'].double().abs().mean() / wp) <= 10 or ncls == 1  # b is not small against W . pooled
