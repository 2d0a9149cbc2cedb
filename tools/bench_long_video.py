#!/usr/bin/env python3
"""Long-video generation at full size (config-2 shapes, 12 layers, 64 text tokens, T = 8, 128 x 128, random weights; mp_config
defaults T = 20, B = 1, dynamic off): one batched level per sampler call against the reference's chain of per-window calls.

    python tools/bench_long_video.py [--repeats 3] [--log profiles/long_video_levels.log]

(1) `interp`, t_repeat = 4, b = 1 (levels of 1, 2, 4 and 8 windows): long_video.generate_long against the chain of the 15
    per-window generate_images calls of utils_train.py:1374-1432.  Both forms warm, alternated `repeats` times in this process, a
    host clock around a device synchronise; the spread of the repeats is the noise.
(2) the last level (8 windows) at b = 8 = 64 sampler rows, at max_rows 8, 16, 32 and 64: time per window.
(3) 4 x 64 decoded frames of 128 x 128 to bytes on the host: frames_to_u8 + the copy of the bytes, against the copy of the fp32
    frames + the conversion of data.save_image_tensor.
Every line goes to stdout and to the log."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from mmvid_amd import long_video as lv, ops


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def chain(model, text, levels, mp):
    """The reference's loop: one generate_images call (control forward, mask-predict, decode of its 8 frames) per window."""
    T, n, MASK = model.num_targets, model.image_seq_len, model.image_token_lut['[MASK]']
    b = text.shape[0]
    prev, frames = None, []
    for lev in levels:
        nxt = []
        for given, passes, emits in lev.windows:
            preserve = None
            if given is not None:
                preserve = torch.full((b, T * n), MASK, dtype=torch.long, device=text.device)
                preserve[:, :T * n // 2] = prev[:, given[0]:given[1]].reshape(b, -1)
            images, _, seq = model.generate_images(text, mask_predict_steps=0, mp_config=mp, dynamic=False, preserve=preserve,
                                                   t_overlap=lev.t_overlap, long_mode=lev.long_mode)
            nxt.append(seq.view(b, T, n)[:, passes[0]:passes[1]])
            if emits[1] > emits[0]:
                frames.append(images[:, emits[0]:emits[1]])
        prev = torch.cat(nxt, dim=1)
    return torch.cat(frames, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'long_video_levels.log'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(42)
    model = bench.build_model(2, dev, 12).eval()
    mp = dict(bench.MP_CONFIG)
    gen = torch.Generator().manual_seed(42)
    text = bench.synth_batch(8, 8, dev, gen)['text']
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f'long video, config-2 model (12 layers, L = {model.total_seq_len}), T = 8, 128 x 128, mp T = {mp["T"]} B = {mp["B"]}, dynamic off, '
        f'{torch.cuda.get_device_name(0)}')
    # ---- (1) batched levels against the chain
    levels = lv.plan('interp', 8, 4)
    one = text[:1]
    batched = lambda: lv.generate_long(model, one, mode='interp', t_repeat=4, mp_config=mp, dynamic=False)[0]  # noqa: E731
    chained = lambda: chain(model, one, levels, mp)  # noqa: E731
    with torch.no_grad():
        for _ in range(2):
            fb, fc = batched(), chained()
        assert fb.shape == (1, 64, 128, 128, 3) and fc.shape == (1, 64, 3, 128, 128)
        tb, tc = [], []
        for _ in range(args.repeats):
            tb.append(timed(batched)[0])
            tc.append(timed(chained)[0])
    spread = max(max(tb) - min(tb), max(tc) - min(tc))
    say(f'(1) interp t_repeat=4 b=1, 15 windows in 4 levels (1, 2, 4, 8), {args.repeats} alternated repeats, ms per 64-frame video')
    say(f'    generate_long (4 sampler calls, 64 frames decoded once, bytes out): {[round(x, 1) for x in tb]}  min {min(tb):.1f}')
    say(f'    chain of 15 generate_images calls (120 frames decoded, fp32 out):   {[round(x, 1) for x in tc]}  min {min(tc):.1f}')
    say(f'    spread of the repeats {spread:.1f} ms; batched - chain = {min(tb) - min(tc):+.1f} ms (min), ratio {min(tc) / min(tb):.2f}x')
    # ---- (2) the last level at b = 8: rows per sampler call
    last = levels[-1:]
    b = 8
    start = torch.randint(0, model.num_image_tokens, (b, 32, model.image_seq_len), device=dev)  # a level-2 timeline
    res = {}
    with torch.no_grad():
        sample = lv.bert_sampler(model, text, mask_predict_steps=0, mp_config=mp, dynamic=False)
        level = lambda m: lv.run(last, sample, b=b, num_targets=8, mask_id=model.image_token_lut['[MASK]'], start=start, max_rows=m)  # noqa: E731
        for m in (8, 16, 32, 64):
            level(m)
        for _ in range(args.repeats):
            for m in (8, 16, 32, 64):
                res.setdefault(m, []).append(timed(lambda: level(m))[0])
    say(f'(2) last level of interp t_repeat=4 at b=8: 8 windows x 8 videos = 64 sampler rows, {args.repeats} alternated repeats')
    sp2 = max(max(v) - min(v) for v in res.values()) / 8
    for m, v in res.items():
        say(f'    max_rows {m:3d}: {64 // m} calls, ms per level {[round(x, 1) for x in v]}  min per window (8 videos) {min(v) / 8:.2f} ms')
    say(f'    spread of the repeats, per window: {sp2:.2f} ms')
    # ---- (3) frames to bytes on the host
    dec = torch.rand(4 * 64, 3, 128, 128, device=dev) * 1.2 - 0.1
    dev_path = lambda: ops.frames_to_u8(dec).cpu()  # noqa: E731
    host_path = lambda: (dec.cpu().clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    kernel = lambda: ops.frames_to_u8(dec)  # noqa: E731
    for f in (dev_path, host_path, kernel):
        f()
    td, th, tk = [], [], []
    for _ in range(args.repeats):
        td.append(timed(dev_path)[0])
        th.append(timed(host_path)[0])
        tk.append(timed(kernel)[0])
    assert torch.equal(dev_path(), host_path())
    say(f'(3) 256 decoded frames of 128 x 128 (50.3 MB fp32 -> 12.6 MB bytes) to host memory, {args.repeats} alternated repeats, ms')
    say(f'    frames_to_u8 + copy of the bytes:               {[round(x, 2) for x in td]}  (the kernel alone, launch to sync: {[round(x, 3) for x in tk]})')
    say(f'    copy of the fp32 frames + host clamp * 255 -> u8: {[round(x, 2) for x in th]}')
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
