#!/usr/bin/env python3
"""Whole config-2 training step of ONE library / mode per process, timed in groups of replays of the captured step:

    [MMVID_LIB=<other build>] [MMVID_DETERMINISTIC=1] python tools/step_groups.py [--groups 8] [--eager N]

Prints one line per process: median and every group's ms/step.  Alternate processes of two builds on one box and compare the
difference of the medians with the spread between groups of the SAME build (tools/gpu_ab_lib.sh does the alternation).
--eager N: no capture; N eagerly launched steps (for `rocprofv3 --kernel-trace --stats -- python tools/step_groups.py --eager 4`)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from mmvid_amd import _lib
from mmvid_amd.engine import FlatTrainer, GraphedStep, backward_order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=8)
    ap.add_argument('--eager', type=int, default=0)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0), np.random.seed(0)
    model = bench.build_model(2, dev, 12).train()
    tr = FlatTrainer(model, lr=1e-4, max_grad_norm=1.0, order=backward_order)
    inputs = bench.synth_batch(6, 8, dev, torch.Generator().manual_seed(0))
    fn = bench.loss_fn(model, 2)
    tag = f'{os.path.basename(_lib.LIB_PATH)} deterministic={int(_lib.is_deterministic())}'
    for _ in range(2 + a.eager):
        bench.eager_step(tr, fn, inputs)
    torch.cuda.synchronize()
    if a.eager:
        print(f'{tag}: {a.eager} eager steps done')
        return
    step = GraphedStep(tr, fn, inputs, warmup=1)
    assert step.graph is not None, step.capture_error
    groups = []
    for _ in range(a.groups):
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        groups.append((time.perf_counter() - t0) / 5 * 1e3)
    print(f'{tag}: median {np.median(groups):7.3f} ms/step  min {min(groups):7.3f}  max {max(groups):7.3f}  groups {[round(x, 3) for x in groups]}')


if __name__ == '__main__':
    main()
