"""A causal tower and a key/value cache on which ONE decode step is exact in fp32 under any summation order, and its reference.

The production decode step (csrc/decode.hip: mmvid_tower_decode_fused_slice, csrc/decode_persistent.hip) has no entry point per kernel,
so the kernels are pinned through the whole step: parameters and cache rows are chosen so that every stage has one possible fp32 result.

  LayerNorm       gain 0, bias = small integers: the staged row IS the bias row, whatever x is (x only travels on the residual path)
  in-projection   q rows of in_w are 0 (q = in_b); k / v rows are sparse small integers, in_b shifts them to chosen integer targets
  attention       'census': q = 0 -> every score 0, every p exactly 1; V[k] one-hot in dimension census_dim(layer, seq, head, k):
                            o = bf16(fp32(count + v_new) / fp32(n)) -- a key dropped / read twice / a wrong n moves the bf16 bits
                  'spot':   q = 16 in dimension 0 of each head, K[k][0] = -128 for every key but one (k*): the other scores are 2048 / 8
                            * log2(e) = 369 binades down, exp2 gives exactly 0, o = V[k*] bit for bit; V[k] spells (layer, seq, head, k)
                            in small integers: a score paired with another key's value row shows
  out-proj        identity + a few small integers per row
  fc              sparse; fc_b shifts every pre-activation into {<= -64, 0, integer in [16, 128]} where x * sigmoid(1.702 x) rounds to
                  -0, 0, x in bf16 whatever the last bit of the hardware exp / rcp
  c_proj          small integers on few columns
All matrix entries are small integers (bf16-exact: the bf16 shadow of the weights is lossless).  The residual chain x -> x_mid -> y
carries the census fractions (multiples of the smallest o's last bf16 bit), so the magnitudes shrink with the cache length: `rich`
parameters (more terms, activations up to 128, two layers) for caches of <= 64 positions, the lean ones for up to 4,096 positions;
tests/test_decode_exact_host.py asserts sum |terms| < 2^24 x (last bit of the smallest term) from the actual tensors of every case.

Everything is a function of integer hashes (no random generator): the host tests and the GPU tests see the same tensors."""
import functools

import torch
import torch.nn.functional as F

BF = torch.bfloat16
SCALE_LOG2 = 0.125 * 1.4426950408889634  # head_dim 64: scores in log2 units, as the kernels scale them
MODES = ('census', 'spot')
# key indices at which the decode attention kernels change batch / wave / loop (attn_decode2_kernel: 8 NW keys per step, 64 NW per
# register batch, NB batches, 4 waves up to 512 keys; decode_persistent: four key ranges, 256 keys per pass)
EDGES = (8, 32, 64, 128, 256, 512, 768, 1024, 1088, 1280, 1536, 2048, 2560, 3072)


def hsh(*xs):
    """31-bit integer hash of a tuple of ints / int64 tensors (broadcast); use the bits above bit 8."""
    h = 0x2545F491
    for x in xs:
        h = ((h ^ x) * 1103515245 + 12345) & 0x7fffffff
        h = h ^ (h >> 11)
    return h


def pick(seed, mod, *xs):
    return (hsh(seed, *xs) >> 8) % mod


def census_dim(l, s, h, k):
    """The dimension key k of (layer, sequence, head) counts in: a different shift per head (k & 63 at h % 7 == 0, (k >> 6) & 63 at
    h % 7 == 6: no two keys below 4,096 share a dimension in every head), permuted per layer and sequence."""
    return (((k >> (h % 7)) ^ (11 * h)) ^ (5 * s + 23 * l)) & 63


def spot_value(l, s, h, k, d):
    """V[k][d] of the 'spot' cache, integers 0..3: d 0-5 the base-4 digits of k, 6-7 of the head, 8-11 of the sequence, 12 the layer,
    hashed above."""
    z = torch.zeros_like(d)
    dig = lambda v, lo: (v >> (2 * torch.maximum(d - lo, z))) & 3
    r = pick(9, 4, l, s, h, k, d)
    r = torch.where(d == 12, (l & 3) + z, r)
    r = torch.where((d >= 8) & (d < 12), dig(s, 8), r)
    r = torch.where((d >= 6) & (d < 8), dig(h, 6), r)
    return torch.where(d < 6, dig(k, 0), r)


def new_row_head(h):
    """'spot': heads whose NEW key has K[0] = 0: their spotlight is the position the step appends (for every sequence)."""
    return h % 4 == 3


def _sparse(seed, l, N, K, nz, vals=(-2, -1, 1, 2)):
    W = torch.zeros(N, K, dtype=torch.int64)
    r = torch.arange(N)
    vt = torch.tensor(vals)
    for t in range(nz):
        W.index_put_((r, pick(seed, K, l, r, t)), vt[pick(seed + 1, len(vals), l, r, t)], accumulate=True)
    return W


@functools.lru_cache(maxsize=None)
def tower_params(E, layers, mode, rich):
    """Per layer a dict of float64 CPU tensors (all integers): ln1_b, ln2_b, in_w, in_b, out_w, out_b, fc_w, fc_b, pj_w, pj_b, and the
    targets k_new, v_new, pre (the fc pre-activation row)."""
    assert mode in MODES and E % 64 == 0
    H, Fd = E // 64, 4 * E
    P = []
    for l in range(layers):
        j, c = torch.arange(E), torch.arange(Fd)
        ln1_b, ln2_b = pick(11, 5, l, j) - 2, pick(12, 5, l, j) - 2
        in_w = _sparse(13, l, 3 * E, E, 4)
        in_w[:E] = 0
        in_w[E + 64 * torch.arange(H)] = 0  # K[0] of every head is set by the bias alone
        raw = in_w @ ln1_b
        k_new = pick(21, 9, l, j) - 4
        heads = torch.arange(H)
        k_new[64 * heads] = torch.where(new_row_head(heads), 0, -128)
        v_new = pick(22, 16, l, j)
        in_b = torch.cat([torch.zeros(E, dtype=torch.int64), k_new, v_new]) - raw
        if mode == 'spot':
            in_b[64 * heads] = 16
        out_w = _sparse(15, l, E, E, 6 if rich else 2) + torch.eye(E, dtype=torch.int64)
        out_b = pick(16, 9, l, j) - 4 if rich else pick(16, 3, l, j) - 1
        fc_w = _sparse(17, l, Fd, E, 4)
        # activation alphabet: columns c % 4 == 0 are active (c % 2 == 0 when rich), the others hold <= -64 or 0
        off = torch.tensor([-64, -80, 0, -96])[pick(19, 4, l, c)]
        if rich:
            pre = torch.where(c % 2 == 0, 16 + pick(20, 113, l, c), off)
        else:
            pre = torch.where(c % 4 == 0, 16 + 0 * c, off)
        fc_b = pre - fc_w @ ln2_b
        # c_proj row j: column 4 j (active) and a few at c % 4 in {1, 2, 3} (lean: never active; rich: c % 4 == 2 is)
        pj_w = torch.zeros(E, Fd, dtype=torch.int64)
        pj_w[j, 4 * j] = 2 * pick(23, 2, l, j) - 1
        for t in range(5 if rich else 3):
            col = 4 * pick(24, E, l, j, t) + 1 + pick(25, 3, l, j, t)
            pj_w.index_put_((j, col), 2 * pick(26, 2, l, j, t) - 1, accumulate=True)
        pj_b = pick(27, 9, l, j) - 4 if rich else pick(27, 3, l, j) - 1
        d = dict(ln1_b=ln1_b, ln2_b=ln2_b, in_w=in_w, in_b=in_b, out_w=out_w, out_b=out_b, fc_w=fc_w, fc_b=fc_b, pj_w=pj_w, pj_b=pj_b,
                 k_new=k_new, v_new=v_new, pre=pre)
        P.append({k: v.double() for k, v in d.items()})
    return P


def params_to(P, device):
    return [{k: v.to(device) for k, v in p.items()} for p in P]


def step_input(B, E, rich, device='cpu', s0=0):
    """x [B, E]: small integers, a different row per sequence (s0: number of the first sequence)."""
    s, j = torch.arange(s0, s0 + B).view(B, 1), torch.arange(E).view(1, E)
    r = 8 if rich else 2
    return (pick(31, 2 * r + 1, s, j) - r).float().to(device)


def build_tower(E, layers, mode, rich, device, seq_len=0):
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    tw = OpenAICLIPTransformer(seq_len=seq_len, which_model='openai_clip_visual', causal=True, layers=layers, width=E, heads=E // 64)
    with torch.no_grad():
        for blk, p in zip(tw.transformer.resblocks, tower_params(E, layers, mode, rich)):
            blk.ln_1.weight.zero_(), blk.ln_2.weight.zero_()
            blk.ln_1.bias.copy_(p['ln1_b']), blk.ln_2.bias.copy_(p['ln2_b'])
            blk.attn.in_proj_weight.copy_(p['in_w']), blk.attn.in_proj_bias.copy_(p['in_b'])
            blk.attn.out_proj.weight.copy_(p['out_w']), blk.attn.out_proj.bias.copy_(p['out_b'])
            blk.mlp.c_fc.weight.copy_(p['fc_w']), blk.mlp.c_fc.bias.copy_(p['fc_b'])
            blk.mlp.c_proj.weight.copy_(p['pj_w']), blk.mlp.c_proj.bias.copy_(p['pj_b'])
    return tw.to(device).eval()


def cache_master(layers, B, Lmax, E, mode, device='cpu'):
    """[layers, B, Lmax, 2E] bf16 with EVERY row filled: K[k][0] = -128 and small hashed integers elsewhere; V one-hot ('census') or
    the (layer, seq, head, k) digits ('spot').  A test copies it, poisons the rows from `pos` on, and (spot) lights its k*."""
    H = E // 64
    out = torch.empty(layers, B, Lmax, 2 * E, dtype=BF, device=device)
    ar = lambda n, shape: torch.arange(n, device=device).view(shape)
    s, k, h, d = ar(B, (B, 1, 1, 1)), ar(Lmax, (1, Lmax, 1, 1)), ar(H, (1, 1, H, 1)), ar(64, (1, 1, 1, 64))
    for l in range(layers):
        Kv = torch.where(d == 0, -128, pick(7, 5, l, s, k, h * 64 + d) - 2)
        Vv = (d == census_dim(l, s, h, k)).to(torch.int64) if mode == 'census' else spot_value(l, s, h, k, d + 0 * (s + k + h))
        out[l, :, :, :E] = Kv.reshape(B, Lmax, E).to(BF)
        out[l, :, :, E:] = Vv.reshape(B, Lmax, E).to(BF)
    return out


def spot_candidates(n, ranges_first=False):
    """Cached key indices worth a spotlight at cache length n, most telling first (the new position n - 1 belongs to new_row_head):
    last cached, first, both sides of every kernel edge (from the top) and of the persistent step's range starts / 256-key passes
    (ranges_first: those before the kernel edges -- a batch of one or two sequences has few (sequence, head) pairs to spend)."""
    kern = [x for e in sorted(EDGES, reverse=True) for x in (e - 1, e)]
    rng = [lo + off for off in (-1, 0, 255, 256, 511, 512, 767, 768) for lo in (3 * n // 4, 2 * n // 4, n // 4)]
    out = []
    for x in [n - 2, 0] + (rng + kern if ranges_first else kern + rng):
        if 0 <= x <= n - 2 and x not in out:
            out.append(x)
    return out


def spot_keys(layers, B, H, n, s0=0, ranges_first=False):
    """k* [layers, B, H] (int64, CPU) for a step at cache length n; -1: the head's spotlight is the new row (or nothing is cached)."""
    cand = torch.tensor(spot_candidates(n, ranges_first) or [-1])
    l, s, h = torch.arange(layers).view(-1, 1, 1), torch.arange(s0, s0 + B).view(1, -1, 1), torch.arange(H).view(1, 1, -1)
    slot = s * (H - H // 4) + h - h // 4 + 5 * l  # (the new-row heads take no slot)
    return torch.where(new_row_head(h), -1, cand[slot % len(cand)])


def light(cache, ks, value):
    """K[k*][0] of every (layer, sequence, head) with a cached spotlight := value (0 to light it, -128 to put it out)."""
    L, B, H = ks.shape
    l, s, h = torch.meshgrid(torch.arange(L), torch.arange(B), torch.arange(H), indexing='ij')
    on = ks >= 0
    dev = cache.device
    cache[l[on].to(dev), s[on].to(dev), ks[on].to(dev), (64 * h[on]).to(dev)] = value


def poison_from(cache, pos):
    cache[:, :, pos:] = float('nan')


def bf16_ulp(v):
    """Last bit of a bf16 value (8 significant bits), as fp64."""
    return torch.exp2(torch.floor(torch.log2(v.abs().double())) - 7)


def reference_step(P, cache, x, pos, info=None):
    """One decode step at position `pos` in fp64 (every intermediate is exact there): reads rows < pos of `cache` ([layers, B, Lmax,
    2E] bf16), WRITES row pos (k_new | v_new) into it, returns y [B, E] fp32.  info (a dict) receives, per layer, the quantities the
    exactness conditions are stated on."""
    B, E = x.shape
    H, n = E // 64, pos + 1
    y = x.double()
    mag, quantum = x.double().abs(), 1.0
    for l, p in enumerate(P):
        qkv = p['in_w'] @ p['ln1_b'] + p['in_b']
        q, kn, vn = qkv[:E], qkv[E:2 * E], qkv[2 * E:]
        assert torch.equal(kn.to(BF).double(), kn) and torch.equal(vn.to(BF).double(), vn) and torch.equal(q.to(BF).double(), q)
        cache[l, :, pos, :E], cache[l, :, pos, E:] = kn.to(BF), vn.to(BF)
        K, V = cache[l, :, :n, :E].double().view(B, n, H, 64), cache[l, :, :n, E:].double().view(B, n, H, 64)
        sc = torch.einsum('hd,bkhd->bhk', q.view(H, 64), K)
        gap = (sc - sc.amax(-1, keepdim=True)) * SCALE_LOG2
        assert bool(((gap == 0) | (gap < -200)).all()), 'a score is neither the maximum nor far enough below it for exp2 to give 0'
        pr = (gap == 0).double()
        num, den = torch.einsum('bhk,bkhd->bhd', pr, V), pr.sum(-1, keepdim=True)
        assert torch.equal(num.float().double(), num)
        o = (num.float() / den.float()).to(BF).double().reshape(B, E)  # one fp32 division, one rounding to bf16
        xmid = y + o @ p['out_w'].t() + p['out_b']
        pre = p['fc_w'] @ p['ln2_b'] + p['fc_b']
        act = torch.where(pre >= 16, pre, torch.zeros_like(pre))  # the alphabet: <= -64 -> -0, 0 -> 0, [16, 128] -> itself
        y = xmid + act @ p['pj_w'].t() + p['pj_b']
        nzo = o[o != 0]
        if nzo.numel():
            quantum = min(quantum, float(bf16_ulp(nzo).min()))
        mag = mag + o.abs() @ p['out_w'].abs().t() + p['out_b'].abs() + act @ p['pj_w'].abs().t() + p['pj_b'].abs()
        if info is not None:
            info.setdefault('layers', []).append(dict(
                o=o, pre=pre, den=den, num=num,
                in_mag=p['in_w'].abs() @ p['ln1_b'].abs() + p['in_b'].abs(), fc_mag=p['fc_w'].abs() @ p['ln2_b'].abs() + p['fc_b'].abs()))
    if info is not None:
        info['residual_mag'], info['quantum'] = mag, quantum
    y32 = y.float()
    assert torch.equal(y32.double(), y), 'the reference itself is not exact in fp32: the case violates its own condition'
    return y32 + 0.0


def torch_fp32_step(P, cache, x, pos):
    """The same step as plain torch fp32 operators (layer_norm, linear, exp, sigmoid) with the rounding points of the kernels."""
    B, E = x.shape
    H, n = E // 64, pos + 1
    rb = lambda t: t.to(BF).float()
    y = x.float()
    for l, p in enumerate(P):
        f = {k: v.float() for k, v in p.items()}
        ln = rb(F.layer_norm(y, (E,), torch.zeros(E), f['ln1_b']))
        qkv = rb(F.linear(ln, f['in_w'], f['in_b']))
        q, kn, vn = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        K = torch.cat([cache[l, :, :pos, :E].float(), kn[:, None]], 1).view(B, n, H, 64)
        V = torch.cat([cache[l, :, :pos, E:].float(), vn[:, None]], 1).view(B, n, H, 64)
        sc = torch.einsum('bhd,bkhd->bhk', q.view(B, H, 64), K) * 0.125
        e = torch.exp(sc - sc.amax(-1, keepdim=True))
        o = rb(torch.einsum('bhk,bkhd->bhd', e, V) / e.sum(-1, keepdim=True)).reshape(B, E)
        xmid = y + F.linear(o, f['out_w'], f['out_b'])
        a = F.linear(rb(F.layer_norm(xmid, (E,), torch.zeros(E), f['ln2_b'])), f['fc_w'], f['fc_b'])
        a = rb(a * torch.sigmoid(1.702 * a))
        y = xmid + F.linear(a, f['pj_w'], f['pj_b'])
    return y, torch.cat([kn, vn], 1)  # (the last layer's new row)


def assert_exact_conditions(info, what=''):
    """The conditions under which reference_step's result is the only possible fp32 result (module docstring), from the actual tensors."""
    lim = float(2**24)
    for l, d in enumerate(info['layers']):
        pre = d['pre']
        ok = (pre <= -64) | (pre == 0) | ((pre >= 16) & (pre <= 128) & (pre == pre.round()))
        assert bool(ok.all()), f'{what}: layer {l}: a pre-activation outside the exact alphabet'
        assert float(d['in_mag'].max()) < lim and float(d['fc_mag'].max()) < lim, f'{what}: layer {l}: in-projection / fc terms'
    worst = float(info['residual_mag'].max())
    assert worst < lim * info['quantum'], f'{what}: residual chain: sum |terms| {worst} >= 2^24 x {info["quantum"]}'


# ---- the cases of tests/test_decode_exact_gpu.py (shared with the host checks).  n = pos + 1 = keys the step attends.
ATTN_CASES = {
    # attn_decode2_kernel<4, 2>: Lmax <= 512
    'nw4_nb2': dict(E=512, Lmax=512, B=(3,), n=(1, 2, 31, 32, 33, 255, 256, 257, 511, 512)),
    # <8, 3>: Lmax > 512 and H * B <= 512; batch 1 on the vector-ALU linear layers (fused='launches')
    'nw8_nb3': dict(E=768, Lmax=4096, B=(1, 3), n=(1, 511, 512, 513, 1023, 1024, 1025, 1151, 1152, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096)),
    # <8, 2>: H * B > 512 (batch 43 and up at 12 heads); keys from 1,024 on go through the loop beyond the register batches
    'nw8_nb2': dict(E=768, Lmax=1152, B=(43, 64), n=(512, 513, 1023, 1024, 1025, 1087, 1088, 1089, 1151, 1152)),
}
# persistent step: runs of consecutive cache lengths (a captured step is replayed along a run: the device position drives nw / loops)
PERSISTENT_RUNS = {
    1152: ((1, 2, 3, 4, 5, 6, 7), (1023, 1024, 1025, 1026, 1027, 1028, 1029), (1150, 1151, 1152)),
    4096: ((1, 2, 3, 4, 5, 6, 7), (1023, 1024, 1025, 1026, 1027, 1028, 1029), (1150, 1151, 1152), (2047, 2048, 2049), (3071, 3072, 3073),
           (4094, 4095, 4096)),
}
LINEAR_LMAX, LINEAR_N = 64, (33, 64)
LINEAR_B = {768: (1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 70), 512: (1, 3, 17, 64)}
