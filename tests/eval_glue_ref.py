"""Plain references of the evaluation encoders' fp32 glue kernels, written from the contract in include/mmvid_hip.h and not from the
kernels: mmvid_clip_image_assemble, mmvid_clip_pool_project, mmvid_clip_pair_scores (csrc/clip.hip), mmvid_i3d_head and
mmvid_i3d_fold (csrc/i3d.hip).  A plain helper like tests/optim_ref.py and tests/frontend_ref.py (no fixtures, no pytest settings,
nothing imported from mmvid_amd, no GPU); its own tests are tests/test_eval_glue_ref_host.py, and tests/test_eval_glue_gpu.py holds
the kernels to it.

Every formula is written ONCE, over a dtype: the public functions evaluate it in fp64 (the reference), `fp32_eval(name, ...)`
evaluates the same lines with CPU torch.float32 operations (the yardstick of the tight bar: what an fp32 evaluation of the contract
costs in accuracy, measured on the reference formula and never on a kernel).

The module also holds the cases of the GPU tests and their seeded CPU generators, so that the host tests can check, without a GPU,
that every hard row has the property it is there for and that the fp32 yardstick itself sits inside each case's worst-case bound."""
import torch

from guarded import seeded

F32, F64, BF, I32 = torch.float32, torch.float64, torch.bfloat16, torch.int32
EPS = 1e-5  # every CLIP LayerNorm (clip_model.py: nn.LayerNorm's default)
U23 = 2.0**-23

# ---- the cases of tests/test_eval_glue_gpu.py ------------------------------------------------------------------------------------
ASSEMBLE_CASES = [(1, 2, 256), (3, 5, 512), (2, 50, 768), (5, 17, 1024), (1, 257, 1024)]  # (N, T, E): N*T = 2, 15, 100, 85, 257
POOL_CASES = [(1, 1, 256, 1, False), (4, 3, 512, 255, True), (5, 77, 512, 512, True), (7, 50, 768, 512, False), (3, 2, 768, 257, True),
              (2, 5, 256, 1000, True), (5, 257, 1024, 768, False), (6, 3, 1024, 1024, True)]  # (B, L, E, D, rows given)
PAIR_CASES = [(1, 1, 1), (3, 1, 63), (2, 3, 64), (5, 7, 65), (3, 16, 512), (2, 5, 768), (1, 9, 1000)]  # (B, T, D)
HEAD_CASES = [(1, 2, 8, 1), (3, 3, 1000, 3), (2, 5, 64, 401), (1, 2, 1024, 5), (2, 9, 1024, 400)]  # (N, To, C, ncls)
FOLD_CASES = [(1, 1), (2, 3)]  # (n, t)
TIGHT_MIN_OUTPUTS = 256  # below this a maximum over the case's outputs is a few draws, not a yardstick
TIGHT_MARGIN = 8.0


# ---- the formulas ----------------------------------------------------------------------------------------------------------------
def layer_norm(v, w, b, eps, dt=F64):
    """Rows of v [..., E]: (v - mean) / sqrt(var + eps) * w + b with the biased variance (nn.LayerNorm), two passes."""
    v, w, b = v.to(dt), w.to(dt), b.to(dt)
    d = v - v.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    return d * torch.rsqrt(var + eps) * w + b


def _image_assemble(dt, feat, cls, pos, w, b, eps, N, T):
    E = cls.numel()
    seq = torch.empty(N, T, E, dtype=dt)
    seq[:, 0] = cls.to(dt)
    seq[:, 1:] = feat.to(dt).reshape(N, T - 1, E)
    return layer_norm(seq + pos.to(dt), w, b, eps, dt).reshape(N * T, E)


def image_assemble(feat, cls, pos, w, b, eps, N, T):
    """out [N*T, E] = layer_norm(cat([cls, feat rows of frame n]) + pos), fp64."""
    return _image_assemble(F64, feat, cls, pos, w, b, eps, N, T)


def pooled_rows(x, rows):
    """x [B, L, E] -> [B, E]: row rows[b] of sequence b, clamped to [0, L - 1]; row 0 when rows is None."""
    B, L, _ = x.shape
    r = torch.zeros(B, dtype=torch.int64) if rows is None else rows.to(torch.int64).clamp(0, L - 1)
    return x[torch.arange(B), r]


def pool_hidden(x, rows, w, b, eps, dt=F64):
    """The LayerNorm h [B, E] of the pooled rows."""
    return layer_norm(pooled_rows(x, rows), w, b, eps, dt)


def _pool_project(dt, x, rows, w, b, eps, proj, l2norm):
    h = pool_hidden(x, rows, w, b, eps, dt)
    y = h @ proj.to(dt)
    mag = h.abs() @ proj.to(dt).abs()
    if l2norm:
        y = y / (y * y).sum(-1, keepdim=True).sqrt()
    return y, mag


def pool_project(x, rows, w, b, eps, proj, l2norm):
    """(out [B, D], |h| @ |proj|) in fp64: h = LN(x[b, rows[b]]), out = h @ proj, divided by its L2 norm if l2norm.  The second
    value is sum |terms| of the projection (of the un-normalised product in either form)."""
    return _pool_project(F64, x, rows, w, b, eps, proj, l2norm)


def _pair_scores(dt, img, txt, B, T):
    D = txt.shape[1]
    a, t = img.to(dt).reshape(B, T, D), txt.to(dt).reshape(B, 1, D)
    return (a * t).sum(-1).reshape(B * T), (a * t).abs().sum(-1).reshape(B * T)


def pair_scores(img, txt, B, T):
    """(out [B*T], sum_k |a_k t_k|) in fp64: out[b*T + t] = <img[b*T + t], txt[b]>."""
    return _pair_scores(F64, img, txt, B, T)


def _i3d_head(dt, x, w, b):
    N, To = x.shape[:2]
    C = x.shape[-1]

    def run(xv, wv, bv):
        xv = xv.reshape(N, To, 49, C)
        pooled = torch.cat([xv[:, :-1], xv[:, 1:]], 2).mean(2)  # [N, To - 1, C]: the (2, 7, 7) window of each time step
        return (pooled @ wv.t() + bv).mean(1)

    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    return run(x, w, b), run(x.abs(), w.abs(), b.abs())


def i3d_head(x_bf16, w, b):
    """(out [N, ncls], the same expression on absolute values) in fp64: x [N, To, 7, 7, C] bf16; mean of the (2, 7, 7) window per time
    step, pooled @ w^T + b, mean over the To - 1 steps."""
    return _i3d_head(F64, x_bf16, w, b)


def i3d_fold(v):
    """v [n, t, 224, 224, 3] fp32 -> [n, t, 224, 112, 24] bf16: folded[n][t][y][wo][3 kw + c] = v[n][t][y][2 wo - 2 + kw][c] for
    kw < 7, zero outside the frame, channels 21..23 zero."""
    n, t = v.shape[:2]
    padded = torch.zeros(n, t, 224, 2 + 224 + 3, 3, dtype=v.dtype)  # column x of the frame at index x + 2
    padded[:, :, :, 2:226] = v
    taps = [padded[:, :, :, kw:kw + 223:2] for kw in range(7)]  # index 2 wo + kw = column 2 wo - 2 + kw, wo < 112
    out = torch.zeros(n, t, 224, 112, 24, dtype=v.dtype)
    out[..., :21] = torch.stack(taps, 4).reshape(n, t, 224, 112, 21)
    return out.to(BF)


_FORMULAS = dict(image_assemble=_image_assemble, pool_project=_pool_project, pair_scores=_pair_scores, i3d_head=_i3d_head)


def fp32_eval(name, *args):
    """The formula of `name` (image_assemble, pool_project, pair_scores, i3d_head) with CPU torch.float32 operations; same arguments
    and results as the fp64 function."""
    return _FORMULAS[name](F32, *args)


# ---- the bars --------------------------------------------------------------------------------------------------------------------
def tight_bar(y32, ref64):
    """TIGHT_MARGIN x the worst |fp32 evaluation - fp64| of the case, floored at 2^-22 max |fp64|."""
    return max(TIGHT_MARGIN * float((y32.double() - ref64).abs().max()), 2.0**-22 * float(ref64.abs().max()))


def pool_bound(case, h64, h32, mag64):
    """Worst-case bar of pool-project with l2norm = 0, [B, D]: (E + 1) 2^-23 |h| @ |proj| for the projection of an exact h, plus
    e_LN[b] sum_k |proj[k][d]| for an h that is e_LN away: e_LN = the tight bar of that pooled row's LayerNorm."""
    E = h64.shape[1]
    e_ln = torch.tensor([tight_bar(h32[s], h64[s]) for s in range(h64.shape[0])], dtype=F64)
    return (E + 1) * U23 * mag64 + e_ln[:, None] * case['proj'].double().abs().sum(0)[None, :]


def head_K(To, C):
    return 98 + C + To + 2


# ---- seeded inputs of the cases --------------------------------------------------------------------------------------------------
def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _ln_params(g, E):
    return 1 + 0.1 * _randn(g, E), 0.1 * _randn(g, E)


def assemble_inputs(N, T, E):
    """Every row of cls / pos / feat is its own draw around its own offset, so a row taken from the wrong place shows.  Hard rows
    (named by their OUTPUT row): the class rows have a mean of 100 at a standard deviation near 1 (a one-pass variance loses them);
    the last patch row SUMS with its pos row to a standard deviation of 1e-3 (variance 0.1 eps), the middle one to 1e-2 (variance 10
    eps).  N = 1, T = 2 has a single patch row: it is the 1e-3 one."""
    g = seeded('assemble', N, T, E)
    R = N * (T - 1)
    cls = 100 + _randn(g, E)
    pos = 0.5 * _randn(g, T, E) + (0.01 * torch.arange(T) - 1)[:, None]
    off = 2.0**-7 * torch.arange(R) - 1
    feat = _randn(g, R, E) + off[:, None]
    w, b = _ln_params(g, E)
    hard = {'cls': [n * T for n in range(N)]}
    for name, r, std in (('std1e-3', R - 1, 1e-3), ('std1e-2', (R - 1) // 2, 1e-2)):
        if name == 'std1e-2' and r == R - 1:
            continue
        n, t = divmod(r, T - 1)
        target = off[r].double() + std * _randn(g, E).double()
        feat[r] = (target - pos[t + 1].double()).float()
        hard[name] = [n * T + t + 1]
    return dict(feat=feat, cls=cls, pos=pos, w=w, b=b, hard=hard)


def _given_rows(B, L):
    order = [L - 1, L // 2, 0, min(1, L - 1), max(L - 2, 0)]
    return [order[s % len(order)] for s in range(B)]


def pool_inputs(B, L, E, D, given):
    """The width is cut into B blocks; the pooled row of sequence s lives in block s (1e-5 elsewhere) and the LayerNorm weight of
    block j is 3^j times (1 + 0.1 randn), so the norms of neighbouring sequences' outputs differ by about 3 and a norm taken from
    another sequence shows.  Sequence 0's pooled row has a standard deviation of 1e-3 (variance 0.1 eps), the last one's (B >= 3) of
    1e-2.  Every other row of x is an ordinary draw over the whole width.  rows (given): L - 1, interior and 0 in turn; the
    (5, 77, 512, 512) case asks for -3 in the first and L + 5 in the last sequence, which the kernel clamps to 0 and L - 1 (unclamped,
    either read would land in the guard around x)."""
    g = seeded('pool', B, L, E, D, given)
    x = _randn(g, B, L, E) * (1 + torch.arange(L) % 3)[None, :, None]
    rows = None
    if given:
        rows = _given_rows(B, L)
        if (B, L, E, D) == (5, 77, 512, 512):
            rows = [-3, 0, L // 2, L - 1, L + 5]
        rows = torch.tensor(rows, dtype=I32)
    at = torch.zeros(B, dtype=torch.int64) if rows is None else rows.to(torch.int64).clamp(0, L - 1)
    edges = [j * E // B for j in range(B + 1)]
    gain = torch.empty(E)
    hard = {}
    for s in range(B):
        lo, hi = edges[s], edges[s + 1]
        gain[lo:hi] = 3.0**s
        row = 1e-5 * _randn(g, E)
        blk = _randn(g, hi - lo).double()
        row[lo:hi] = (blk - blk.mean()).float()  # (a mean would be subtracted from the other blocks too, under their larger weights)
        std = 1e-3 if s == 0 else 1e-2 if s == B - 1 and B >= 3 else None
        if std is not None:
            hard['std1e-3' if s == 0 else 'std1e-2'] = s
        scale = (1.0 + s) if std is None else std / float(row.double().std(unbiased=False))
        x[s, at[s]] = (row.double() * scale).float()
    w, b = _ln_params(g, E)
    return dict(x=x, rows=rows, w=w * gain, b=b, proj=_randn(g, E, D) * E**-0.5, hard=hard)


def pair_inputs(B, T, D):
    g = seeded('pair', B, T, D)
    return dict(img=_randn(g, B * T, D), txt=_randn(g, B, D) + 0.5 * torch.arange(B)[:, None])


def head_inputs(N, To, C, ncls):
    """The time steps of a clip have means 0.5, 1, 1.5, ... (a window that starts one step off, or a wrong divisor, shows); b is
    N(0, 1) against W . pooled of the same order."""
    g = seeded('head', N, To, C, ncls)
    x = (_randn(g, N, To, 7, 7, C) + (0.5 + 0.5 * torch.arange(To))[None, :, None, None, None]).to(BF)
    return dict(x=x, w=_randn(g, ncls, C) * C**-0.5, b=_randn(g, ncls))


N_TIES = 4096


def fold_inputs(n, t):
    """randn * 3 with N_TIES exact bf16 ties (fp32 values half-way between two neighbouring bf16 values: low 16 bits 0x8000) and
    N_TIES / 2 each of +0.0 and -0.0 at seeded places.  -> (v, flat indices of the ties)."""
    g = seeded('fold', n, t)
    v = _randn(g, n, t, 224, 224, 3) * 3
    flat = v.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:2 * N_TIES]
    ties, zeros = idx[:N_TIES], idx[N_TIES:]
    flat[ties] = ((flat[ties].view(I32) >> 16 << 16) | 0x8000).view(F32)
    flat[zeros[:N_TIES // 2]] = 0.0
    flat[zeros[N_TIES // 2:]] = -0.0
    return v, ties
