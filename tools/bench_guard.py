#!/usr/bin/env python3
"""Cost of the non-finite guard (FlatTrainer(skip_nonfinite=True)) on the config-2 captured step (BERT, 12 layers, per-GPU batch 6).

    python tools/bench_guard.py [--pairs 3] [--log profiles/guard_bench.log]      the comparison: alternating processes on one box
    python tools/bench_guard.py --leg off|on                                      one process, one leg, one JSON line

The comparison starts `2 * pairs` fresh processes one after the other -- off, on, on, off, off, on, ... -- each of which builds the
model from the same seed, captures the step (GraphedStep) with the guard off or on, warms it, and times `--rounds` samples of
`--steps` replays: a host clock around replays that end in a device synchronise, per step.  Per leg: the median over all of its
samples, min, max, and each process's median.  What a difference has to exceed to mean anything is the SPREAD of the off leg: the
distance between the medians of its processes.  One JSON line, to stdout and appended to the log."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--leg', choices=['off', 'on'], default=None)
ap.add_argument('--pairs', type=int, default=3)
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--steps', type=int, default=20, help='replays per sample')
ap.add_argument('--batch', type=int, default=6)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--log', default=None)
args = ap.parse_args()


def leg():
    sys.path.insert(0, ROOT)
    import torch

    import bench
    from mmvid_amd import _lib
    from mmvid_amd.engine import FlatTrainer, GraphedStep, backward_order
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(42)
    torch.manual_seed(0)
    model = bench.build_model(2, dev, args.layers).train()
    batch = bench.synth_batch(args.batch, 8, dev, gen)
    trainer = FlatTrainer(model, lr=1e-4, max_grad_norm=1.0, order=backward_order, skip_nonfinite=args.leg == 'on')
    step = GraphedStep(trainer, bench.loss_fn(model, 2), batch, warmup=2)
    if step.graph is None:
        raise SystemExit(f'the step was not captured: {step.capture_error}')
    for _ in range(args.steps):
        step()
    samples = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3 / args.steps)
    assert bool(torch.isfinite(loss))
    out = {'leg': args.leg, 'samples_ms': [round(x, 4) for x in samples], 'loss': float(loss)}
    if args.leg == 'on':
        st = trainer.guard_stats()
        assert st['skipped'] == 0 and st['seen'] == trainer.step_count, st
        out['seen'] = st['seen']
    _lib.check_device_faults()
    print(json.dumps(out))


def compare():
    order = [('off', 'on') if i % 2 == 0 else ('on', 'off') for i in range(args.pairs)]
    runs = []
    for name in (x for pair in order for x in pair):
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--rounds', str(args.rounds), '--steps', str(args.steps),
               '--batch', str(args.batch), '--layers', str(args.layers)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:  # (nothing more is started after a process that failed)
            raise SystemExit(f'leg {name} ended with status {res.returncode}')
        runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = {'metric': 'guard_bench', 'config': 2, 'batch': args.batch, 'layers': args.layers, 'rounds': args.rounds, 'steps': args.steps,
           'order': [r['leg'] for r in runs]}
    for name in ('off', 'on'):
        mine = [r['samples_ms'] for r in runs if r['leg'] == name]
        every = [x for s in mine for x in s]
        meds = [round(statistics.median(s), 4) for s in mine]
        out[name] = {'median_ms': round(statistics.median(every), 4), 'min_ms': min(every), 'max_ms': max(every), 'process_medians_ms': meds,
                     'spread_ms': round(max(meds) - min(meds), 4)}
    out['on_minus_off_ms'] = round(out['on']['median_ms'] - out['off']['median_ms'], 4)
    out['losses'] = [r['loss'] for r in runs]
    line = json.dumps(out)
    print(line)
    if args.log:
        with open(args.log, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    leg() if args.leg else compare()
