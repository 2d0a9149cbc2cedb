#!/usr/bin/env python3
"""Cost of ART-V video prediction at full size (config-5 model, 12 layers, 16 frames of 64 tokens, random weights): DALLE.generate_images
at batch B plain (1,024 sampled tokens over the KV cache), with the first 4 and the first 8 frames known (768 / 512 sampled tokens behind
one re-prefill of the prompt and the known frames), and one re-prefill alone (the tower's prefill over <bos>, text, visual and 4 / 8
known frames, with the embedding of those ids).

    python tools/bench_artv_completion.py [--batch 4] [--runs 5] [--tag NAME] [--log profiles/artv_completion_cost.log]
    python tools/bench_artv_completion.py --root PATH_TO_ANOTHER_CHECKOUT --plain-only --tag parent

All calls warm (2 calls each), then alternated `runs` times in this process, a host clock around a device synchronise; median, min and
max per call.  `--root` imports `bench` and `mmvid_amd` from another checkout that has been built (the parent commit's, for the same-box
comparison of the plain call; `--plain-only` there, the keyword does not exist yet): run the two trees in alternating processes.  One
JSON line per process, to stdout and appended to the log.  Forcing known tokens through the decode step is not built and not timed."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--batch', type=int, default=4)
ap.add_argument('--plain-only', action='store_true')
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
b = args.batch
model = bench.build_model(5, dev, 12).eval()
text = bench.synth_batch(b, 1, dev, gen, visuals=1)['text']
vis_tok = torch.randint(0, 1024, (b, 64), generator=gen).to(dev)
T, n = model.num_targets, model.image_seq_len
known = torch.randint(0, 1024, (b, T * n), generator=gen).to(dev)


def first(frames):
    return torch.tensor([1] * frames + [0] * (T - frames), dtype=torch.uint8), known


def generate(**kw):
    return lambda: model.generate_images(text, visual=vis_tok, **kw)


def prefill(frames):
    prompt = torch.cat(model._prompt_ids(text, vis_tok), 1)
    ids = torch.cat((prompt, known[:, :frames * n]), 1)
    cache = model.transformer.new_kv_cache(b, model.total_seq_len, dev)
    with torch.no_grad():
        return lambda: model.transformer.prefill(model._embed_rows(ids, 0), cache)


kinds = {'plain': generate()}
if not args.plain_only:
    kinds.update({'known_4': generate(given=first(4)), 'known_8': generate(given=first(8)), 'prefill_4': prefill(4), 'prefill_8': prefill(8)})


def call(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):
    for fn in kinds.values():
        call(fn)
times = {k: [] for k in kinds}
for _ in range(args.runs):
    for k, fn in kinds.items():
        times[k].append(call(fn))
out = {'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'batch': b, 'runs': args.runs}
for k, v in times.items():
    out[k] = {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
              'all_ms': [round(x, 2) for x in v]}
line = json.dumps(out)
print(line)
if args.log:
    with open(args.log, 'a') as f:
        f.write(line + '\n')
