#!/usr/bin/env python3
"""Cost of the trainer telemetry (FlatTrainer(telemetry_every=...)) at config 2 (BERT, per-GPU batch 6), on one box, alternated.

    python tools/bench_telemetry.py [--layers 12] [--runs 7] [--tag this] [--log profiles/telemetry_cost.log]
    python tools/bench_telemetry.py --root PATH_TO_ANOTHER_CHECKOUT --off-only --tag parent

Three comparisons, every timed thing warm, the alternatives taken in turn `runs` times in this process:

  kernel   on the trainer's flat buffers (G, P, M, V and the lazy-row flags as three training steps left them): mmvid_segment_stats
           with every = 1, the gated call (count % every != 0: three launches that return at once), and mmvid_adam_step_rows -- each
           without and with the lazy table; `--launches` calls between two device events, per call.  Bytes: 16 per element the
           statistics read (4 where a lazy row is unflagged: p only), 28 per element Adam touches (30 with the bf16 shadow, which the
           trainer passes and this comparison passes too).
  eager    the training step launched from Python with telemetry off, every = 1 and every = 50 (three trainers on three copies of
           the model): a host clock around `--steps` steps that end in a device synchronise, per step.
  graphed  the same step as one replayed hipGraph (GraphedStep).

Per alternative: median, min, max and every sample, and SPREAD = (max - min) / median of its own samples, which is what a difference
has to exceed to mean anything.  `--root` imports `bench` and `mmvid_amd` from another built checkout (the parent commit's, which has no
`telemetry_every`: `--off-only`); run the two trees in alternating processes to compare the telemetry-less step of this tree with the
parent's.  One JSON line per process, to stdout and appended to the log."""
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
ap.add_argument('--launches', type=int, default=20, help='kernel calls per sample')
ap.add_argument('--batch', type=int, default=6)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--off-only', action='store_true', help='time the telemetry-less eager and graphed step only (a tree without the feature)')
ap.add_argument('--no-steps', action='store_true', help='the kernel comparison only')
ap.add_argument('--tag', default='this')
ap.add_argument('--log', default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import mmvid_amd  # noqa: E402
from mmvid_amd import ops  # noqa: E402
from mmvid_amd.engine import FlatTrainer, GraphedStep, backward_order  # noqa: E402

assert os.path.abspath(mmvid_amd.__file__).startswith(ROOT), (mmvid_amd.__file__, ROOT)
dev = torch.device('cuda', 0)
gen = torch.Generator().manual_seed(42)
torch.manual_seed(0)
base = bench.build_model(2, dev, args.layers).train()
batch = bench.synth_batch(args.batch, 8, dev, gen)
KW = {'off': {}, 'every_1': dict(telemetry_every=1), 'every_50': dict(telemetry_every=50)}
kinds = ['off'] if args.off_only else ['every_1'] if args.no_steps else list(KW)
models, trainers, fns = {}, {}, {}
for kind in kinds:
    m = copy.deepcopy(base)
    models[kind], fns[kind] = m, bench.loss_fn(m, 2)
    trainers[kind] = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order, **KW[kind])
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


out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'steps': args.steps, 'batch': args.batch,
       'layers': args.layers, 'numel': trainers[kinds[0]].numel}
for kind in kinds:
    for _ in range(3):
        bench.eager_step(trainers[kind], fns[kind], batch)

# ---- the kernels alone, on the buffers of the trainer that takes a record every step
if not args.off_only:
    tr = trainers['every_1']
    t, n = tr._tel, tr.numel
    lazy = tr._lazy_arg()
    rows_live = int(lazy[0].sum().item()) if lazy is not None else None
    touched = n if lazy is None else n - (lazy[2] - rows_live) * lazy[3]
    saved = {k: getattr(tr, k).clone() for k in ('P', 'M', 'V', 'S')}
    count_was = t['count'].clone()

    def stats(every, lz):
        def call():
            ops.segment_stats(tr.G, tr.P, tr.M, tr.V, t['tables'], t['chunks'], 1000, tr.lr, tr.betas, tr.eps, every, tr.telemetry_slots,
                              t['count'], t['partials_f'], t['partials_i'], t['ring_f'], t['ring_i'], t['head_i'], t['head_f'], lazy=lz)
        return call

    def gated():
        t['count'].fill_(1)  # 1 % 2^30 != 0, and so for every count the timed calls reach
        return stats(1 << 30, lazy)

    def adam(lz):
        return lambda: ops.adam_step(tr.P, tr.G, tr.M, tr.V, tr.S, 1000, tr.lr, tr.betas, tr.eps, 0.0, 0.0, None, 1.0, lazy=lz)

    calls = {'segment_stats': launches_ms(stats(1, None)), 'adam_step_rows': launches_ms(adam(None))}
    if lazy is not None:
        calls['segment_stats_lazy'] = launches_ms(stats(1, lazy))
        calls['adam_step_rows_lazy'] = launches_ms(adam(lazy))
    k = alternate(calls)
    k.update(alternate({'segment_stats_gated': launches_ms(gated())}))  # (on its own: it needs the counter off the multiples of every)
    for name, val in saved.items():  # the timed Adam launches moved the weights: put them back before the steps below
        getattr(tr, name).copy_(val)
    t['count'].copy_(count_was)
    t['head_i'].zero_()
    t['count'].zero_()
    stat_bytes = {'segment_stats': 16.0 * n, 'segment_stats_lazy': 16.0 * touched + 4.0 * (n - touched)}
    adam_bytes = {'adam_step_rows': 30.0 * n, 'adam_step_rows_lazy': 30.0 * touched}
    for name, s in k.items():
        b = stat_bytes.get(name, adam_bytes.get(name))
        if b is not None:
            s['bytes'], s['tb_per_s'] = int(b), round(b / s['median_ms'] / 1e9, 3)
    out['kernel'] = dict(k, elements=n, segments=len(tr.names), chunks=t['chunks'], lazy_rows_flagged=rows_live, lazy_elements_touched=touched,
                         ratio_stats_to_adam=round(k['segment_stats']['median_ms'] / k['adam_step_rows']['median_ms'], 4))
    if lazy is not None:
        out['kernel']['ratio_stats_to_adam_lazy'] = round(k['segment_stats_lazy']['median_ms'] / k['adam_step_rows_lazy']['median_ms'], 4)

if not args.no_steps:
    # ---- eager step
    out['eager'] = alternate({kind: steps_ms(lambda kind=kind: bench.eager_step(trainers[kind], fns[kind], batch)) for kind in kinds})
    # ---- the captured step
    graphed = {}
    for kind in kinds:
        graphed[kind] = GraphedStep(trainers[kind], fns[kind], batch, warmup=2)
        if graphed[kind].graph is None:
            out.setdefault('capture_error', {})[kind] = graphed[kind].capture_error
    out['graphed'] = alternate({kind: steps_ms(graphed[kind]) for kind in kinds})
    for part in ('eager', 'graphed'):
        for kind in kinds[1:]:
            out[part][f'ratio_{kind}_to_off'] = round(out[part][kind]['median_ms'] / out[part]['off']['median_ms'], 4)
    if not args.off_only:
        out['records'] = {kind: len(trainers[kind].telemetry()) for kind in kinds[1:]}

line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
