#!/usr/bin/env python
"""Build a token cache of a frame-folder dataset (mmvid_amd/token_cache.py): every frame through the frozen VQGAN once, in an
index-exact tokeniser mode, so that training encodes only the one warped frame per sample of the VID negative.

    python tools/tokenize_dataset.py --folder data/mmvoxceleb --vae_path vqgan.ckpt --image_size 128 --out data/mmvoxceleb_tokens

--mode: split (default; the reference's indices except ties at its own fp32 resolution) | fp32 | mixed | bf16.
--random_resize_crop_lower_ratio below 1 is refused: such a recipe crops at random and has to train from pixels."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--folder', required=True, help='dataset root: video/<key>/<frames> + txt/<key>.txt')
    ap.add_argument('--out', required=True, help='directory of the cache (created)')
    ap.add_argument('--vae_path', required=True, help='VQGAN checkpoint (the frozen tokeniser of the training run)')
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--mode', default='split', choices=['split', 'fp32', 'mixed', 'bf16'])
    ap.add_argument('--no-frames', action='store_true', help='tokens only: training can then draw only the two VID strategies that '
                    'move whole frames (vid_strategy_prob[2] = [3] = 0)')
    ap.add_argument('--chunk', type=int, default=64, help='frames per encoder call')
    ap.add_argument('--random_resize_crop_lower_ratio', type=float, default=1.0, help="the recipe's value (utils/utils_args.py:52-55)")
    args = ap.parse_args()

    import torch

    from mmvid_amd.token_cache import build_token_cache
    from mmvid_amd.vae import VQGanVAE1024
    vae = VQGanVAE1024(args.vae_path, args.image_size)
    vae.image_size = args.image_size
    vae = vae.to(torch.device('cuda', 0))
    t0 = time.perf_counter()
    cache = build_token_cache(args.folder, vae, args.out, mode={'fp32': True, 'bf16': False}.get(args.mode, args.mode),
                              with_frames=not args.no_frames, chunk=args.chunk, resize_ratio=args.random_resize_crop_lower_ratio)
    dt = time.perf_counter() - t0
    print(f'{len(cache)} frames of {len(cache.videos)} videos -> {args.out} ({cache.strict} tokeniser, {len(cache) / dt:.0f} frames/s, '
          f'fingerprint {cache.fingerprint[:12]}...)')


if __name__ == '__main__':
    main()
