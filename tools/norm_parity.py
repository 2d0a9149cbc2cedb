#!/usr/bin/env python3
"""SHA-256 digests of everything csrc/norm.hip writes, on seeded inputs, through the C ABI: run it once per built checkout (in
separate processes) and compare the two JSON files -- a behaviour-preserving change of the file leaves every digest equal.

    python tools/norm_parity.py --out this.json
    python tools/norm_parity.py --root PATH_TO_ANOTHER_CHECKOUT --out parent.json
    python tools/norm_parity.py --compare parent.json this.json        (no GPU; exit status 1 if a digest differs or is missing)

LayerNorm: forward (both output types); backward through _ws, _ex (fp32 and bf16 dy) and _partial + _reduce_multi, add on / off, with
and without dx_bf16, every null-target combination; the form without a workspace contributes only its dx (its sums are atomic: their
order is free).  GroupNorm: both input types, both output types, swish on / off (one launch on small maps, three on larger ones); the
split and fp16-out forms."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out')
ap.add_argument('--compare', nargs=2)
args = ap.parse_args()
if args.compare:
    a, b = (json.load(open(p)) for p in args.compare)
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f'{len(a)} / {len(b)} digests, {len(bad)} differ or are missing' + ''.join(f'\n  {k}' for k in bad))
    sys.exit(1 if bad or not a else 0)
sys.path.insert(0, args.root)
import torch

from mmvid_amd import _lib, ops

P, S, BF, F32 = ops._p, ops._stream, torch.bfloat16, torch.float32
LN_SHAPES = [(10, 768), (1158, 768), (77, 512), (37, 200), (5, 1024), (1, 8), (3001, 768)]
GN_SHAPES = [(2, 16, 128), (1, 8, 512), (3, 4, 32), (1, 32, 256)]
digests = {}


def rnd(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def note(key, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        if t is not None:
            raw = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()
            digests[f'{key} {name}'] = hashlib.sha256(raw).hexdigest()


for rows, E in LN_SHAPES:
    g = torch.Generator().manual_seed(rows * 4099 + E)
    x, w, b, dy = rnd(g, rows, E) * 2 + 0.5, rnd(g, E) * 0.1 + 1, rnd(g, E) * 0.1, rnd(g, rows, E)
    dx0, t0 = rnd(g, rows, E), [rnd(g, E) for _ in range(3)]
    mean, rstd = torch.empty(rows, device='cuda'), torch.empty(rows, device='cuda')
    for dt in (BF, F32):
        y = torch.empty(rows, E, device='cuda', dtype=dt)
        _lib.call('mmvid_layernorm_fwd', P(x), E, rows, E, P(w), P(b), 1e-5, P(y) if dt == BF else None, P(y) if dt == F32 else None, E,
                  P(mean), P(rstd), S())
        note(f'ln_fwd {rows}x{E} {dt}', y=y, mean=mean, rstd=rstd)
    nws = 3 * E * (512 if rows == 3001 else 256)  # (3001 rows against 512 blocks: the reduction's 16-deep loop runs)
    for form in ('ws', 'ex_f32', 'ex_bf16', 'partial', 'atomics'):
        dyv = dy.to(BF) if form == 'ex_bf16' else dy
        for add in (0, 1):
            for want16 in (0, 1):
                for want in ((1, 1, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0)):
                    if form == 'atomics' and (want16 or want != (1, 1, 1)):
                        continue
                    dx, dx16 = dx0.clone(), torch.empty(rows, E, device='cuda', dtype=BF) if want16 else None
                    tg = [t.clone() if k else None for t, k in zip(t0, want)]
                    ws = torch.zeros(nws, device='cuda')
                    head = (P(dyv), int(form == 'ex_bf16'), E, P(x), E, P(mean), P(rstd), P(w), rows, E, P(dx), E, add, P(dx16))
                    if form == 'atomics':
                        _lib.call('mmvid_layernorm_bwd', head[0], *head[2:], *(P(t) for t in tg), S())
                        tg = [None] * 3
                    elif form == 'ws':
                        _lib.call('mmvid_layernorm_bwd_ws', head[0], *head[2:], *(P(t) for t in tg), P(ws), nws, S())
                    elif form == 'partial':
                        blocks = ctypes.c_int(0)
                        _lib.call('mmvid_layernorm_bwd_partial', *head, *want, P(ws), nws, ctypes.byref(blocks), S())
                        if any(want):
                            ops.layernorm_bwd_reduce_multi([(ws, *tg)], blocks.value, E)
                    else:
                        _lib.call('mmvid_layernorm_bwd_ex', *head, *(P(t) for t in tg), P(ws), nws, S())
                    note(f'ln_bwd {rows}x{E} {form} add={add} dx16={want16} want={want}', dx=dx, dx16=dx16, dw=tg[0], db=tg[1], cs=tg[2])

for N, H, C in GN_SHAPES:
    g = torch.Generator().manual_seed(N * 65537 + H * 257 + C)
    x32, w, b = rnd(g, N, H, H, C) * 1.5 + 0.3, rnd(g, C) * 0.1 + 1, rnd(g, C) * 0.1
    for x in (x32, x32.to(BF)):
        for dt in (BF, F32):
            for swish in (True, False):
                note(f'gn {N}x{H}x{H}x{C} in={x.dtype} out={dt} swish={swish}', y=ops.groupnorm_swish(x, w, b, swish=swish, out_dtype=dt))
    if (N, H, C) in ((2, 16, 128), (1, 32, 256)):
        for swish in (True, False):
            note(f'gn_split {N}x{H}x{H}x{C} swish={swish}', planes=ops.groupnorm_swish_split(x32, w, b, swish=swish))
            note(f'gn_f16out {N}x{H}x{H}x{C} swish={swish}', y=ops.groupnorm_swish_f16(x32, w, b, swish=swish))

json.dump(digests, open(args.out, 'w') if args.out else sys.stdout, indent=0, sort_keys=True)
print(f'{len(digests)} digests from {args.root}', file=sys.stderr)
