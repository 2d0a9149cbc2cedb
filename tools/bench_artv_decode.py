#!/usr/bin/env python3
"""ART-V sampling (BASELINE config 5: 16 frames of 128x128 = 1,024 tokens, L = 1,152): seconds per video with the
reference's algorithm (full transformer over the growing prefix for every token) and with the KV-cache decoder.

    bench_artv_decode.py                                   the 12-layer, 768-wide tower at batch 1 and 16, both algorithms
    bench_artv_decode.py --width 1024 --layers 24 --batches 1,4,16,64 --cached-only
                                                           a ViT-L/14-sized tower (heads = width / 64): sampled tokens/s
    bench_artv_decode.py --width 1024 --layers 24 --batches 1,4,16,64 --step [--gemm-step]
                                                           the tower's decode step alone on a raw OpenAICLIPTransformer (hipGraph
                                                           replays at the last positions of the 1,152-long cache): us per step and the
                                                           fraction of the weight-streaming floor (layers x 12 E^2 bf16 at --hbm-tbs);
                                                           --gemm-step: the GEMM-based step (mmvid_tower_decode), what widths other
                                                           than 512 / 768 ran before the decode kernels took 1,024
One JSON line per measurement follows the readable one."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--width', type=int, default=768)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--batches', default='1,16')
ap.add_argument('--cached-only', action='store_true', help='skip the reference\'s loop (the whole prefix per token)')
ap.add_argument('--step', action='store_true', help='time the tower decode step alone')
ap.add_argument('--gemm-step', action='store_true', help='with --step: the GEMM-based step (decode_session(fused=False))')
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--hbm-tbs', type=float, default=6.3, help='HBM rate the weight-streaming floor is stated against, TB/s (measured copy rate)')
args = ap.parse_args()
batches = [int(b) for b in args.batches.split(',')]
dev = torch.device('cuda', 0)
torch.manual_seed(0)
L, P = 1152, 128  # cache length of config 5; prompt: 64 text positions + 64 visual tokens

if args.step:
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    tw = OpenAICLIPTransformer(seq_len=L, which_model='openai_clip_visual', causal=True, layers=args.layers, width=args.width,
                               heads=args.width // 64).to(dev).eval()
    floor_us = args.layers * 12 * args.width**2 * 2 / (args.hbm_tbs * 1e12) * 1e6
    for B in batches:
        with torch.no_grad():
            cache = tw.new_kv_cache(B, L, dev)
            cache.zero_()
            tw.prefill(torch.randn(B, P, args.width, device=dev) * 0.5, cache)
            first = L - args.reps - 8
            sess = tw.decode_session(cache, first, fused=not args.gemm_step)
            x = torch.randn(B, args.width, device=dev) * 0.5
            for _ in range(4):  # eager step, capture, two replays
                sess.step(x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                sess.step(x)
            e1.record()
            torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        form = 'gemm' if args.gemm_step else ('persistent' if sess.persistent else 'fused')
        print(f'step width={args.width} layers={args.layers} B={B} form={form}: {us:8.1f} us per step = {B / us * 1e6:9.1f} tokens/s, '
              f'weight floor {floor_us:.1f} us ({floor_us / us:.3f} of the step)')
        print(json.dumps(dict(kind='step', width=args.width, layers=args.layers, B=B, form=form, us=us, floor_us=floor_us)))
    sys.exit(0)

from mmvid_amd.dalle_artv import DALLE
from mmvid_amd.vae import VQGanVAE1024

vae = VQGanVAE1024(None, 128)
vae.image_size = 128
cvae = VQGanVAE1024(None, 128)
cvae.image_size = 128
wide = {} if (args.width, args.layers) == (768, 12) else dict(transformer_width=args.width, transformer_layers=args.layers)
m = DALLE(dim=args.width, vae=vae, cvae=cvae, num_text_tokens=49408, text_seq_len=64, which_transformer='openai_clip_visual',
          num_visuals=1, num_targets=16, **wide).to(dev).eval()
for B in batches:
    text = torch.randint(1, 49408, (B, 64), device=dev)
    visual = torch.rand(B, 1, 3, 128, 128, device=dev)
    for cached in ((True, ) if args.cached_only else (True, False)):
        for rep in range(2):  # the first call pays one-time costs (VQGAN plans, weight re-layout, kernel loading)
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images, _, _ = m.generate_images(text, visual=visual, use_cache=cached)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print(f'B={B} use_cache={cached}: {dt:7.2f} s for {B} video(s) of 1024 tokens = {B * 1024 / dt:8.1f} tokens/s, images {tuple(images.shape)}')
        print(json.dumps(dict(kind='sample', width=args.width, layers=args.layers, B=B, use_cache=cached, seconds=dt, tokens_per_s=B * 1024 / dt)))
