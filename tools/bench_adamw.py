"""mmvid_adam_step_decoupled against mmvid_adam_step_rows at the size of BERT's flat buffer: both move 30 B per parameter (p, m, v read
and written, g read, the bf16 shadow written), so the AdamW variant should cost what Adam costs.  One process, the two entries taken
in turn after a warm-up (rows, decoupled, rows, decoupled, ...), `--samples` samples of `--launches` launches each between two
events; per entry the median, the spread (max - min) / median and the bytes per second.  Prints one JSON line.

    python tools/bench_adamw.py [--elements 124700032] [--samples 15] [--launches 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from mmvid_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--elements', type=int, default=124700032)  # BERT's flat buffer: about 124.7 M fp32, a multiple of 128
ap.add_argument('--samples', type=int, default=15)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--weight-decay', type=float, default=0.01)
args = ap.parse_args()

n, dev = args.elements, 'cuda'
gen = torch.Generator(device=dev).manual_seed(0)
P = torch.randn(n, device=dev, generator=gen) * 0.05
G = torch.randn(n, device=dev, generator=gen) * 1e-3
M = torch.randn(n, device=dev, generator=gen) * 1e-3
V = torch.rand(n, device=dev, generator=gen) * 1e-6
S = torch.empty(n, device=dev, dtype=torch.bfloat16)
sq = torch.full((1,), 4.0, device=dev)              # norm 2: the step is clipped
step_dev = torch.full((1,), 1000.0, device=dev)
lr_dev = torch.full((1,), 1e-4, device=dev)
common = dict(step=1000, lr=1e-4, eps=1e-8, weight_decay=args.weight_decay, max_norm=1.0, sqnorm=sq, grad_scale=1.0, step_dev=step_dev,
              lr_dev=lr_dev)
calls = {'adam_step_rows': lambda: ops.adam_step(P, G, M, V, S, betas=(0.9, 0.999), **common),
         'adam_step_decoupled': lambda: ops.adam_step(P, G, M, V, S, betas=(0.9, 0.95), decoupled=True, **common)}


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.launches


for fn in calls.values():
    for _ in range(3):
        sample(fn)
times = {k: [] for k in calls}
for _ in range(args.samples):
    for k, fn in calls.items():
        times[k].append(sample(fn))
out = {'elements': n, 'samples': args.samples, 'launches': args.launches, 'weight_decay': args.weight_decay}
for k, t in times.items():
    med = statistics.median(t)
    out[k] = {'median_ms': round(med, 4), 'min_ms': round(min(t), 4), 'max_ms': round(max(t), 4),
              'spread': round((max(t) - min(t)) / med, 4), 'tb_per_s': round(30.0 * n / med / 1e9, 3)}
r, d = out['adam_step_rows'], out['adam_step_decoupled']
out['decoupled_within_rows_spread'] = bool(r['min_ms'] <= d['median_ms'] <= r['max_ms'])
out['ratio_decoupled_to_rows'] = round(d['median_ms'] / r['median_ms'], 4)
print(json.dumps(out))
