#!/usr/bin/env python3
"""Cost of seeded sampling in the ART-V sampler at full size (config-5 model, 12 layers, 16 frames, 1,024 sampled tokens per video over
the KV cache, random weights): DALLE.sample_tokens unseeded and with `seeds=` at each batch size.  Up to batch 64 the variates of the
whole call are one block (one `exponential_` unseeded, one fill launch seeded); above it (steps * B * V > 2^26) the captured step draws
per token (an `exponential_` unseeded, a fill with the position read on the device seeded).

    python tools/bench_seeded.py [--batches 16,64,72] [--runs 5] [--tag NAME] [--log profiles/seeded_cost.log]
    python tools/bench_seeded.py --root PATH_TO_ANOTHER_CHECKOUT --unseeded-only --tag parent

All calls warm (2 calls each), then alternated `runs` times in this process, a host clock around a device synchronise; median, min and
max per call, and the ratio of the medians.  `--root` imports `bench` and `mmvid_amd` from another checkout that has been built (the
parent commit's; `--unseeded-only` there, the keyword does not exist yet): run the two trees in alternating processes.  One JSON line
per process, to stdout and appended to the log."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--batches', default='16,64,72')
ap.add_argument('--unseeded-only', action='store_true')
ap.add_argument('--tag', default='this')
ap.add_argument('--log', default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import mmvid_amd  # noqa: E402

assert os.path.abspath(mmvid_amd.__file__).startswith(ROOT), (mmvid_amd.__file__, ROOT)
dev = torch.device('cuda', 0)
gen = torch.Generator().manual_seed(42)
batches = [int(v) for v in args.batches.split(',')]
top = max(batches)
model = bench.build_model(5, dev, 12).eval()
text = bench.synth_batch(top, 1, dev, gen, visuals=1)['text']
vis_tok = torch.randint(0, 1024, (top, 64), generator=gen).to(dev)
kinds = {}
for b in batches:
    kinds[f'unseeded_{b}'] = (b, {})
    if not args.unseeded_only:
        kinds[f'seeded_{b}'] = (b, dict(seeds=list(range(1000, 1000 + b))))


def call(kind):
    n, kw = kind
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.sample_tokens(text[:n], visual=vis_tok[:n], **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):
    for kind in kinds.values():
        call(kind)
times = {k: [] for k in kinds}
for _ in range(args.runs):
    for k, kind in kinds.items():
        times[k].append(call(kind))
out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'runs': args.runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
for b in batches:
    if f'seeded_{b}' in out:
        out[f'ratio_seeded_to_unseeded_{b}'] = round(out[f'seeded_{b}']['median_ms'] / out[f'unseeded_{b}']['median_ms'], 4)
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
