#!/usr/bin/env python3
"""Cost of classifier-free guidance in the ART-V sampler at full size (config-5 model, 12 layers, 16 frames, 1,024 sampled tokens per
video over the KV cache, random weights): DALLE.generate_images at batch B unguided, at batch B with guidance_scale = 2.0 and the default
drop (2B tower rows, B draws), and unguided at batch 2B (the same tower rows, twice the draws).

    python tools/bench_artv_guidance.py [--batch 16] [--runs 5] [--tag NAME] [--log profiles/artv_guidance_cost.log]
    python tools/bench_artv_guidance.py --root PATH_TO_ANOTHER_CHECKOUT --unguided-only --tag parent

All calls warm (2 calls each), then alternated `runs` times in this process, a host clock around a device synchronise; median, min and
max per call, and the ratios of the medians.  `--root` imports `bench` and `mmvid_amd` from another checkout that has been built (the
parent commit's, for the same-box comparison of the unguided path; `--unguided-only` there, the keyword does not exist yet): run the two
trees in alternating processes.  One JSON line per process, to stdout and appended to the log."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--batch', type=int, default=16)
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
gen = torch.Generator().manual_seed(42)
b = args.batch
model = bench.build_model(5, dev, 12).eval()
text = bench.synth_batch(2 * b, 1, dev, gen, visuals=1)['text']
vis_tok = torch.randint(0, 1024, (2 * b, 64), generator=gen).to(dev)
kinds = {'unguided_B': (b, {})}
if not args.unguided_only:
    kinds['guided_B'] = (b, dict(guidance_scale=args.scale))
    kinds['unguided_2B'] = (2 * b, {})


def call(kind):
    n, kw = kind
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate_images(text[:n], visual=vis_tok[:n], **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):
    for kind in kinds.values():
        call(kind)
times = {k: [] for k in kinds}
for _ in range(args.runs):
    for k, kind in kinds.items():
        times[k].append(call(kind))
out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'batch': b, 'runs': args.runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
if 'guided_B' in out:
    out['scale'] = args.scale
    out['ratio_guided_B_to_unguided_2B'] = round(out['guided_B']['median_ms'] / out['unguided_2B']['median_ms'], 4)
    out['ratio_guided_B_to_unguided_B'] = round(out['guided_B']['median_ms'] / out['unguided_B']['median_ms'], 4)
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
