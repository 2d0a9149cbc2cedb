#!/usr/bin/env python3
"""Same-box comparison of the training step from pixels and from cached tokens (config 2, per-GPU batch 6, set up as bench.py does).

    python tools/bench_token_step.py [--rounds 9] [--reps 20]

Four captured steps (engine.GraphedStep) on one model and one trainer, replayed in alternation:
  (a) pixel step, default bf16 tokeniser      54 frames through the encoder: the headline step of bench.py
  (b) pixel step, vae.strict = 'split'        54 frames through the index-exact encoder
  (c) token step, vae.strict = 'split'        48 frames' tokens gathered from a device-resident uint16 table by frame index
                                              (ops.token_rows_gather), uint8 frames, 6 new frames through the index-exact encoder
  (d) token step, default bf16 tokeniser      the same with the bf16 encoder for the 6 new frames
A round times every leg once (`reps` replays between two device synchronisations), the order reversing every round so that drift
of the box cancels; the median over the rounds is reported per leg.  Then the encoder alone (eager launches, device events) at 6
and at 54 frames in both modes: where a token step's remaining encoder time goes.  Prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from mmvid_amd import _lib, ops
from mmvid_amd.engine import FlatTrainer, GraphedStep, WarmupLR, backward_order
from mmvid_amd.functional import weighted_loss


def encoder_alone(vae, frames, calls=20):
    """ms per get_codebook_indices call on `frames`, launched eagerly (device events around `calls` calls, after 3 warm ones)."""
    for _ in range(3):
        vae.get_codebook_indices(frames)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        vae.get_codebook_indices(frames)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20, help='replays per leg and round')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    seed = 42
    torch.manual_seed(seed), np.random.seed(seed)
    model = bench.build_model(2, dev, 12)
    model.frontend.seed = seed
    model.train()
    tr = FlatTrainer(model, lr=1e-4, max_grad_norm=1.0, order=backward_order, lr_schedule=WarmupLR(1e-6, 1e-4, 5000, every=1))
    B, T = 6, 8
    gen = torch.Generator().manual_seed(seed)
    pix = bench.synth_batch(B, T, dev, gen)
    u8 = torch.randint(0, 256, (B, T, bench.SIZE, bench.SIZE, 3), generator=gen, dtype=torch.uint8).to(dev)
    pix['frames'] = ops.frames_u8_to_f32(u8.view(B * T, bench.SIZE, bench.SIZE, 3)).view(B, T, 3, bench.SIZE, bench.SIZE)  # the same frames
    rows = torch.arange(B * T, device=dev).view(B, T)
    fn_pix = bench.loss_fn(model, 2)
    tables = {}

    def fn_tok(text, rows, target_frames):
        lm, lr, lv = model(text, target=ops.token_rows_gather(tables[model.vae.strict], rows), target_frames=target_frames,
                           return_loss=True, rel=True, vid=True, rel_no_fully_masked=True, msm_strategy_prob=bench.MSM_PROB,
                           msm_bernoulli_prob=bench.MSM_BERN, vid_strategy_prob=bench.VID_PROB)
        return weighted_loss((lm, lr, lv), (7.0, 0.5, 0.5))

    for _ in range(2):
        bench.eager_step(tr, fn_pix, pix)
    tok_in = dict(text=pix['text'], rows=rows, target_frames=u8)
    legs = [('a', 'pixel step, bf16 tokeniser (54 frames)', False, fn_pix, pix),
            ('b', "pixel step, vae.strict = 'split' (54 frames)", 'split', fn_pix, pix),
            ('c', "token step, vae.strict = 'split' (6 frames, uint8)", 'split', fn_tok, tok_in),
            ('d', 'token step, bf16 tokeniser (6 frames, uint8)', False, fn_tok, tok_in)]
    steps = {}
    for tag, what, mode, fn, inp in legs:
        model.vae.strict = mode
        if mode not in tables:  # the cache of these 48 frames in this mode, resident on the device
            tables[mode] = model.vae.get_codebook_indices(pix['frames'].view(B * T, 3, bench.SIZE, bench.SIZE)).to(torch.int16).view(torch.uint16)
        steps[tag] = GraphedStep(tr, fn, inp, warmup=2)
        assert steps[tag].graph is not None, f'leg {tag}: capture failed: {steps[tag].capture_error}'
    model.vae.strict = False
    for tag in steps:  # every graph warm before the first timed round
        for _ in range(5):
            steps[tag]()
    torch.cuda.synchronize()
    res = {tag: [] for tag in steps}
    for r in range(args.rounds):
        order = list(steps) if r % 2 == 0 else list(steps)[::-1]
        for tag in order:
            steps[tag]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                loss = steps[tag]()
            torch.cuda.synchronize()
            res[tag].append((time.perf_counter() - t0) / args.reps * 1e3)
            assert torch.isfinite(loss).item(), f'leg {tag}: loss {loss.item()}'
    _lib.check_device_faults()
    print(f'config 2, per-GPU batch {B}, one process, {args.rounds} rounds x {args.reps} replays per leg, order reversed every round')
    med = {}
    for tag, what, _, _, _ in legs:
        med[tag] = float(np.median(res[tag]))
        print(f'({tag}) {what:52s} median {med[tag]:7.3f} ms/step  min {min(res[tag]):7.3f}  max {max(res[tag]):7.3f}  '
              f'rounds {[round(x, 3) for x in res[tag]]}')
    print(f'(c) - (a) = {med["c"] - med["a"]:+.3f} ms/step: the index-exact token step is '
          f'{"FASTER" if med["c"] < med["a"] else "NOT faster"} than the bf16 pixel step;  (d) - (a) = {med["d"] - med["a"]:+.3f};  '
          f'(c) - (b) = {med["c"] - med["b"]:+.3f}')
    enc = {}
    for mode in (False, 'split'):
        model.vae.strict = mode
        name = 'split' if mode else 'bf16'
        for n in (B, B * T + B):
            enc[f'{name}_{n}'] = encoder_alone(model.vae, pix['frames'].view(B * T, 3, bench.SIZE, bench.SIZE)[:1].expand(n, -1, -1, -1).contiguous())
    model.vae.strict = False
    print('encoder alone, eager launches (ms per call): ' + '  '.join(f'{k} frames: {v:.3f}' for k, v in enc.items()))
    print(json.dumps({'metric': 'token_step_same_box', 'batch': B, 'rounds': args.rounds, 'reps': args.reps, 'median_ms_per_step': med,
                      'rounds_ms_per_step': res, 'token_exact_faster_than_pixel_bf16': med['c'] < med['a'],
                      'encoder_alone_eager_ms': enc}))


if __name__ == '__main__':
    main()
