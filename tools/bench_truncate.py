#!/usr/bin/env python3
"""Cost of truncated sampling (top-k / nucleus, csrc/sample.hip::logits_truncate_kernel) at full size, random weights.

  bert   config-2 model (12 layers, 64 text tokens, T = 8, 128 x 128), b = 4, mp_config defaults (T = 20, B = 1), dynamic off:
         BERT.generate_images against the same call with top_p = 0.9.
  artv   config-5 model (16 frames, 1,024 sampled tokens per video over the KV cache), batch 16: DALLE.generate_images unfiltered
         (the captured token step), with filter_thres = 1 - 64 / total_tokens (the eager torch.topk path: 64 classes) and with
         top_k = 64 (one more launch inside the captured step).

    python tools/bench_truncate.py bert|artv [--runs N] [--tag NAME] [--log profiles/truncate_cost.log]
    python tools/bench_truncate.py bert|artv --root PATH_TO_ANOTHER_CHECKOUT --no-keywords --tag parent

Every kind warm (2 calls each), then alternated `runs` times in this process, a host clock around a device synchronise; median, min
and max per call.  `--root` imports `bench` and `mmvid_amd` from another checkout that has been built (the parent commit's, where the
keywords do not exist: `--no-keywords`); run the two trees in alternating processes.  One JSON line per process, to stdout and
appended to the log."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('which', choices=('bert', 'artv'))
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=None)
ap.add_argument('--batch', type=int, default=None)
ap.add_argument('--no-keywords', action='store_true')
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
if args.which == 'bert':
    b, runs = args.batch or 4, args.runs or 12
    model = bench.build_model(2, dev, 12).eval()
    batch = bench.synth_batch(b, 8, dev, gen)
    cfg = dict(bench.MP_CONFIG)
    kinds = {'plain': {}}
    if not args.no_keywords:
        kinds['top_p_0.9'] = dict(top_p=0.9)
        kinds['top_k_64'] = dict(top_k=64)
    run = lambda kw: model.generate_images(batch['text'], mask_predict_steps=0, mp_config=cfg, dynamic=False, **kw)  # noqa: E731
else:
    b, runs = args.batch or 16, args.runs or 5
    model = bench.build_model(5, dev, 12).eval()
    batch = bench.synth_batch(b, 1, dev, gen, visuals=1)
    vis_tok = torch.randint(0, 1024, (b, 64), generator=gen).to(dev)
    kinds = {'plain': {}, 'filter_thres_64': dict(filter_thres=1.0 - 64.5 / model.total_tokens)}
    assert max(int((1 - kinds['filter_thres_64']['filter_thres']) * model.total_tokens), 1) == 64
    if not args.no_keywords:
        kinds['top_k_64'] = dict(top_k=64)
        kinds['top_p_0.9'] = dict(top_p=0.9)
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
out = {'tag': args.tag, 'which': args.which, 'device': torch.cuda.get_device_name(0), 'batch': b, 'runs': runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
for k in kinds:
    if k != 'plain':
        out[f'ratio_{k}_to_plain'] = round(out[k]['median_ms'] / out['plain']['median_ms'], 4)
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
