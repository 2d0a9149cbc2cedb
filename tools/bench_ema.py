#!/usr/bin/env python3
"""Cost of the weight EMA (FlatTrainer(ema_decay=...)) at config 2 (BERT, 12 layers, per-GPU batch 6), on one box, alternated.

    python tools/bench_ema.py [--runs 7] [--tag this] [--log profiles/ema_bench.log]
    python tools/bench_ema.py --root PATH_TO_ANOTHER_CHECKOUT --off-only --tag parent

Three comparisons, every timed thing warm, the alternatives taken in turn `runs` times in this process:

  kernel   mmvid_ema_update over the trainer's flat buffer (E and P as the trainer holds them, the lazy-row flags as three training steps
           left them), without and with the lazy table, next to torch's `E.lerp_(P, a)` on the same buffers: `--launches` launches
           between two device events, per launch; bytes = 12 per element the launch touches.
  eager    the training step launched from Python, EMA off and on (two trainers on two copies of the model): a host clock around
           `--steps` steps that end in a device synchronise, per step.
  graphed  the same step as one replayed hipGraph (GraphedStep), EMA off and on.

Per alternative: median, min, max and every sample; per comparison the ratio of the medians and the SPREAD = (max - min) / median of the
reference alternative's samples, which is what a difference has to exceed to mean anything.  `--root` imports `bench` and `mmvid_amd`
from another built checkout (the parent commit's, which has no `ema_decay`: `--off-only`); run the two trees in alternating processes
to compare the EMA-less step of this tree with the parent's.  One JSON line per process, to stdout and appended to the log."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=7)
ap.add_argument('--steps', type=int, default=10, help='training steps per sample')
ap.add_argument('--launches', type=int, default=20, help='kernel launches per sample')
ap.add_argument('--batch', type=int, default=6)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--decay', type=float, default=0.9999)
ap.add_argument('--off-only', action='store_true', help='time the EMA-less eager and graphed step only (a tree without the feature)')
ap.add_argument('--tag', default='this')
ap.add_argument('--log', default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import mmvid_amd  # noqa: E402
from mmvid_amd import _lib, ops  # noqa: E402
from mmvid_amd.engine import FlatTrainer, GraphedStep, backward_order  # noqa: E402

assert os.path.abspath(mmvid_amd.__file__).startswith(ROOT), (mmvid_amd.__file__, ROOT)
dev = torch.device('cuda', 0)
gen = torch.Generator().manual_seed(42)
torch.manual_seed(0)
base = bench.build_model(2, dev, args.layers).train()
batch = bench.synth_batch(args.batch, 8, dev, gen)
kinds = ['off'] if args.off_only else ['off', 'on']
models, trainers, fns = {}, {}, {}
for kind in kinds:
    m = copy.deepcopy(base)
    kw = dict(ema_decay=args.decay, ema_warmup=True) if kind == 'on' else {}
    models[kind], fns[kind] = m, bench.loss_fn(m, 2)
    trainers[kind] = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order, **kw)
del base


def summary(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4),
            'spread': round((max(v) - min(v)) / statistics.median(v), 4), 'all_ms': [round(x, 4) for x in v]}


def alternate(calls):
    """calls: {name: fn() -> ms}.  Two warm rounds, then `runs` rounds in turn."""
    for _ in range(2):
        for fn in calls.values():
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.runs):
        for k, fn in calls.items():
            times[k].append(fn())
    return {k: summary(v) for k, v in times.items()}


def steps_ms(step):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps
    return run


out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'steps': args.steps, 'batch': args.batch,
       'layers': args.layers, 'numel': trainers['off'].numel}

# ---- eager step, EMA off / on
for kind in kinds:
    for _ in range(3):
        bench.eager_step(trainers[kind], fns[kind], batch)
out['eager'] = alternate({kind: steps_ms(lambda kind=kind: bench.eager_step(trainers[kind], fns[kind], batch)) for kind in kinds})

# ---- the kernel alone, on the buffers of the trainer that keeps the average
if not args.off_only:
    tr = trainers['on']
    E, P, n = tr.E, tr.P, tr.numel
    lazy = tr._lazy_arg()
    a = 1.0 - tr.ema_decay_at(10**6)
    rows_live = int(lazy[0].sum().item()) if lazy is not None else None
    touched = n if lazy is None else n - (lazy[2] - rows_live) * lazy[3]

    def launches_ms(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.launches
        return run

    calls = {'torch_lerp': launches_ms(lambda: E.lerp_(P, a)),
             'ema_update': launches_ms(lambda: ops.ema_update(E, P, args.decay, False, 10**6))}
    if lazy is not None:
        calls['ema_update_lazy'] = launches_ms(lambda: ops.ema_update(E, P, args.decay, False, 10**6, lazy=lazy))
    saved = E.clone()
    k = alternate(calls)
    E.copy_(saved)  # (the timed launches moved the average: put it back before the steps below)
    for name, s in k.items():
        s['gb_per_s'] = round(12.0 * (touched if name == 'ema_update_lazy' else n) / s['median_ms'] / 1e6, 1)
    out['kernel'] = dict(k, elements=n, lazy_rows_flagged=rows_live, lazy_elements_touched=touched,
                         ratio_ema_update_to_torch_lerp=round(k['ema_update']['median_ms'] / k['torch_lerp']['median_ms'], 4))
    out['eager']['ratio_on_to_off'] = round(out['eager']['on']['median_ms'] / out['eager']['off']['median_ms'], 4)

# ---- the captured step, EMA off / on
graphed = {}
for kind in kinds:
    graphed[kind] = GraphedStep(trainers[kind], fns[kind], batch, warmup=2)
    if graphed[kind].graph is None:
        raise SystemExit(f'the step was not captured ({kind}): {graphed[kind].capture_error}')
out['graphed'] = alternate({kind: steps_ms(lambda kind=kind: graphed[kind]()) for kind in kinds})
if not args.off_only:
    out['graphed']['ratio_on_to_off'] = round(out['graphed']['on']['median_ms'] / out['graphed']['off']['median_ms'], 4)
_lib.check_device_faults()
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
