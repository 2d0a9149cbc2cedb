#!/usr/bin/env python3
"""InceptionI3d.embed (mmvid_amd.fvd, csrc/i3d.hip) on clips of 16 frames of 128^2 resized to 224^2, at batch 16 and 64, against a
stock-PyTorch eager I3D with the same weights (F.conv3d with explicit TF-SAME pads, BatchNorm folded, F.max_pool3d, NCDHW) in fp32
and under bf16 autocast.  Random weights (timing only).  One JSON line per (path, B): ms per call (HIP events around `reps` calls after
a warm-up), clips/s and TFLOP/s of the algorithmic 55.6 GFLOP per clip.  `--layers` adds one line per layer group of the native path
(stem, 2b + 2c, Mixed_3b/3c, the rest; events around each launch group, synchronised: shares only).  Per-kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/bench_fvd_embed.py --sizes 16 --reps 5` run.

    python tools/bench_fvd_embed.py [--reps 10] [--sizes 16,64] [--layers]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from mmvid_amd.fvd import INCEPTION, POOL_BEFORE, InceptionI3d, same_pad

DEV = 'cuda'


def random_model():
    torch.manual_seed(0)
    m = InceptionI3d()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith('conv3d.weight'):
                v.normal_(0, (2.0 / v[0].numel())**0.5)
            elif k.endswith('running_var') or k.endswith('bn.weight'):
                v.uniform_(0.8, 1.2)
            elif v.is_floating_point():
                v.normal_(0, 0.05)
    return m.requires_grad_(False).eval().to(DEV)


_FOLDED = {}  # Unit3D -> (weight, bias) with BatchNorm folded: done once, outside the timed calls


def stock_forward(m, x):
    """x [B, 3, T, 224, 224] -> [B, 400]: pytorch_i3d's forward in eager PyTorch with BatchNorm folded (the same arithmetic per layer
    a framework's inference path would run)."""
    def pad(x, k, s):
        p = []
        for n, kk, ss in reversed(list(zip(x.shape[2:], k, s))):
            p += list(same_pad(n, kk, ss))
        return F.pad(x, p)

    def unit(u, x, k, s=(1, 1, 1)):
        if id(u) not in _FOLDED:
            _FOLDED[id(u)] = InceptionI3d.fold_bn(u)
        w, b = _FOLDED[id(u)]
        return F.relu(F.conv3d(pad(x, k, s), w, b, stride=s))

    def pool(x, k, s):
        return F.max_pool3d(pad(x, k, s), k, s)

    x = unit(m.Conv3d_1a_7x7, x, (7, 7, 7), (2, 2, 2))
    x = pool(x, (1, 3, 3), (1, 2, 2))
    x = unit(m.Conv3d_2c_3x3, unit(m.Conv3d_2b_1x1, x, (1, 1, 1)), (3, 3, 3))
    x = pool(x, (1, 3, 3), (1, 2, 2))
    for name, *_ in INCEPTION:
        if name in POOL_BEFORE:
            x = pool(x, *POOL_BEFORE[name])
        b = getattr(m, name)
        x = torch.cat([unit(b.b0, x, (1, 1, 1)), unit(b.b1b, unit(b.b1a, x, (1, 1, 1)), (3, 3, 3)),
                       unit(b.b2b, unit(b.b2a, x, (1, 1, 1)), (3, 3, 3)), unit(b.b3b, pool(x, (3, 3, 3), (1, 1, 1)), (1, 1, 1))], 1)
    x = F.avg_pool3d(x, (2, 7, 7), 1)
    x = F.conv3d(x, m.logits.conv3d.weight, m.logits.conv3d.bias)
    return x.squeeze(3).squeeze(3).mean(2)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def layer_groups(model, v, reps):
    """Time the native plan's launch groups.  Plan order: stem conv + pool, 2b + 2c + pool, then five launches per Inception block
    (and a pool in front of 4b and 5b)."""
    arena = model._arena(v.shape[0], 16, v.device)
    plan = arena['plan']
    groups = {'stem (1a + pool)': plan[:2], '2b + 2c + pool': plan[2:5], 'Mixed_3b + 3c': plan[5:15], 'Mixed_4b .. 5c': plan[15:]}
    out = {g: timed(lambda: model._run_plan(arena, ops_), reps) for g, ops_ in groups.items()}
    out['head'] = timed(lambda: model._head(arena), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='16,64')
    ap.add_argument('--layers', action='store_true')
    ap.add_argument('--no-stock', action='store_true')
    args = ap.parse_args()
    model = random_model()
    gflop = model.flops(16) / 1e9
    for B in (int(s) for s in args.sizes.split(',')):
        g = torch.Generator(device=DEV).manual_seed(B)
        v = torch.rand(B, 16, 3, 128, 128, device=DEV, generator=g)
        pre = F.interpolate(v.flatten(0, 1), size=(224, 224), mode='bilinear').view(B, 16, 3, 224, 224) * 2 - 1
        pre = pre.permute(0, 2, 1, 3, 4).contiguous()  # NCDHW for the stock path
        paths = [('native_embed', lambda: model.embed(v, 16))]
        if not args.no_stock:
            def s32():
                with torch.no_grad():
                    return stock_forward(model, pre)

            def s16():
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    return stock_forward(model, pre)
            paths += [('stock_eager_fp32', s32), ('stock_eager_bf16_autocast', s16)]
        for path, fn in paths:
            ms = timed(fn, args.reps)
            print(json.dumps(dict(tool='bench_fvd_embed', path=path, B=B, frames=16, input_hw=128, ms=round(ms, 3),
                                  clips_per_s=round(B / ms * 1e3, 1), tflops=round(gflop * B / ms, 2))), flush=True)
        if args.layers:
            t = layer_groups(model, v, args.reps)
            tot = sum(t.values())
            for gname, ms in t.items():
                print(json.dumps(dict(tool='bench_fvd_embed', path='native_layer_group', B=B, group=gname, ms=round(ms, 3),
                                      share=round(ms / tot, 3))), flush=True)


if __name__ == '__main__':
    main()
