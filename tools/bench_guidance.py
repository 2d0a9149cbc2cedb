#!/usr/bin/env python3
"""Cost of classifier-free guidance at full size (config-2 shapes, 12 layers, 64 text tokens, T = 8, 128 x 128, random weights; b = 4,
mp_config defaults T = 20, B = 1, dynamic off): BERT.generate_images against the same call with guidance_scale = 2.0.

    python tools/bench_guidance.py [--runs 12] [--tag NAME] [--log profiles/guidance_cost.log]
    python tools/bench_guidance.py --root PATH_TO_ANOTHER_CHECKOUT --unguided-only --tag parent

Both calls warm (3 calls each), then alternated `runs` times in this process, a host clock around a device synchronise; median, min
and max per call, and the ratio of the medians.  `--root` imports `bench` and `mmvid_amd` from another checkout that has been built
(the parent commit's, for the same-box comparison of the unguided path; `--unguided-only` there, the keyword does not exist yet):
run the two trees in alternating processes.  One JSON line per process, to stdout and appended to the log."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=12)
ap.add_argument('--batch', type=int, default=4)
ap.add_argument('--scale', type=float, default=2.0)
ap.add_argument('--unguided-only', action='store_true')
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
model = bench.build_model(2, dev, 12).eval()
batch = bench.synth_batch(args.batch, 8, dev, torch.Generator().manual_seed(42))
cfg = dict(bench.MP_CONFIG)
kinds = {'unguided': {}}
if not args.unguided_only:
    kinds['guided'] = dict(guidance_scale=args.scale, guidance_drop=('text', ))  # (config 2 has no visual control)


def call(kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate_images(batch['text'], mask_predict_steps=0, mp_config=cfg, dynamic=False, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(3):
    for kw in kinds.values():
        call(kw)
times = {k: [] for k in kinds}
for _ in range(args.runs):
    for k, kw in kinds.items():
        times[k].append(call(kw))
out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'runs': args.runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
if 'guided' in out:
    out['scale'] = args.scale
    out['ratio_of_medians'] = round(out['guided']['median_ms'] / out['unguided']['median_ms'], 4)
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
