#!/usr/bin/env python3
"""Cost of per-video sampling parameters (csrc/sample.hip::logits_truncate_rows_kernel) against the scalar keywords, at full size,
random weights.

  bert   config-2 model (12 layers, 64 text tokens, T = 8, 128 x 128), b = 4, mp_config defaults (T = 20, B = 1), dynamic off:
         BERT.generate_images with top_k = 64, top_p = 0.9 against video_top_k = [64] * b, video_top_p = [0.9] * b (the same filters,
         read per row on the device) and against a mixed batch (every video its own values).
  artv   config-5 model (16 frames, 1,024 sampled tokens per video over the KV cache), batch 16: DALLE.generate_images with top_k = 64,
         top_p = 0.9, temperature = 0.9 (the captured token step with the scalar truncation launch in it) against the three video_*
         vectors with the same values, and against a mixed batch.

    python tools/bench_truncate_rows.py bert|artv [--runs N] [--batch B] [--log profiles/truncate_rows_cost.log]

The scalar call is the parent commit's path, launch for launch (tests/test_video_params_gpu.py compares the launch lists), and is timed
TWICE, as two kinds of its own (`scalar`, `scalar_again`): the distance between their medians is the box's run-to-run spread, the
yardstick beside every ratio.  Every kind warm (2 calls each), then alternated `runs` times in this process, a host clock around a
device synchronise; median, min and max per call.  One JSON line per process, to stdout and appended to the log."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('which', choices=('bert', 'artv'))
ap.add_argument('--runs', type=int, default=None)
ap.add_argument('--batch', type=int, default=None)
ap.add_argument('--log', default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

dev = torch.device('cuda', 0)
gen = torch.Generator().manual_seed(42)
if args.which == 'bert':
    b, runs = args.batch or 4, args.runs or 12
    model = bench.build_model(2, dev, 12).eval()
    batch = bench.synth_batch(b, 8, dev, gen)
    cfg = dict(bench.MP_CONFIG)
    scalar = dict(top_k=64, top_p=0.9)
    kinds = {'scalar': scalar, 'scalar_again': scalar,
             'video_uniform': dict(video_top_k=[64] * b, video_top_p=[0.9] * b),
             'video_mixed': dict(video_top_k=[(64, 0, 8, 256)[i % 4] for i in range(b)], video_top_p=[(0.9, 0.5, 1.0, 0.95)[i % 4] for i in range(b)])}
    run = lambda kw: model.generate_images(batch['text'], mask_predict_steps=0, mp_config=cfg, dynamic=False, **kw)  # noqa: E731
else:
    b, runs = args.batch or 16, args.runs or 5
    model = bench.build_model(5, dev, 12).eval()
    batch = bench.synth_batch(b, 1, dev, gen, visuals=1)
    vis_tok = torch.randint(0, 1024, (b, 64), generator=gen).to(dev)
    scalar = dict(top_k=64, top_p=0.9, temperature=0.9)
    kinds = {'scalar': scalar, 'scalar_again': scalar,
             'video_uniform': dict(video_top_k=[64] * b, video_top_p=[0.9] * b, video_temperature=[0.9] * b),
             'video_mixed': dict(video_top_k=[(64, 0, 8, 256)[i % 4] for i in range(b)], video_top_p=[(0.9, 0.5, 1.0, 0.95)[i % 4] for i in range(b)],
                                 video_temperature=[(0.9, 1.0, 0.7, 1.3)[i % 4] for i in range(b)])}
    run = lambda kw: model.generate_images(batch['text'], visual=vis_tok, **kw)  # noqa: E731


def call(kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):
    for kw in kinds.values():
        call(kw)
times = {k: [] for k in kinds}
for _ in range(runs):
    for k, kw in kinds.items():
        times[k].append(call(kw))
out = {'which': args.which, 'device': torch.cuda.get_device_name(0), 'batch': b, 'runs': runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
base = out['scalar']['median_ms']
out['spread_scalar_again_to_scalar'] = round(out['scalar_again']['median_ms'] / base, 4)
for k in ('video_uniform', 'video_mixed'):
    out[f'ratio_{k}_to_scalar'] = round(out[k]['median_ms'] / base, 4)
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
