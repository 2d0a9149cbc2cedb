#!/usr/bin/env python3
"""The calls of both samplers on the tiny models of the tests, for a kernel-trace run: the kernel list of this tree must be the parent
commit's (no launch added, none changed).  Every form of the token draw (mmvid_amd/token_draw.py) in both samplers: BERT plain, guided,
with top_k = 8 and guided with top_p = 0.9; ART-V on every path of its token loop (mmvid_amd/artv_sampling.py): batch 4 captured, batch 4
with a `filter_thres` that filters (eager), batch 4 with top_k = 8 (captured with the truncation launch), batch 4 guided, batch 4 guided
with top_k = 8, and batch 2 (one launch per token).  Every call runs under a fixed seed and prints a digest of the tokens it sampled
(BERT: img_seq): the two trees' outputs must be equal line for line.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/truncate_launch_list.py [--root OTHER_CHECKOUT]

then compare the (kernel name, calls) columns of the two DIR/**/NAME_kernel_stats.csv: `python tools/truncate_launch_list.py --diff A B`."""
import argparse
import csv
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--diff', nargs=2, metavar='CSV')
args = ap.parse_args()

if args.diff:
    def calls(path):
        with open(path) as f:
            return {row['Name']: int(row['Calls']) for row in csv.DictReader(f)}
    a, b = calls(args.diff[0]), calls(args.diff[1])
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f'{len(a)} kernels / {sum(a.values())} launches in {args.diff[0]}; {len(b)} / {sum(b.values())} in {args.diff[1]}; '
          f'{len(differ)} kernels differ in name or count')
    for k in differ:
        print(f'  {a.get(k)} vs {b.get(k)}  {k}')
    sys.exit(1 if differ else 0)

ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import mmvid_amd  # noqa: E402
from mmvid_amd.dalle_artv import DALLE  # noqa: E402
from mmvid_amd.dalle_bert import BERT  # noqa: E402
from mmvid_amd.vae import VQGanVAE1024  # noqa: E402

assert os.path.abspath(mmvid_amd.__file__).startswith(ROOT), (mmvid_amd.__file__, ROOT)
dev = torch.device('cuda', 0)


def tiny_vae():
    v = VQGanVAE1024(None, 64, ddconfig={'ch': 32}, n_embed=256)
    v.image_size, v.num_tokens = 64, 256
    return v


kw = dict(dim=768, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual', num_targets=2, transformer_layers=2)
torch.manual_seed(0)
bert = BERT(vae=tiny_vae(), num_visuals=0, **kw).to(dev).eval()
artv = DALLE(vae=tiny_vae(), cvae=None, num_visuals=1, **kw).to(dev).eval()
text = torch.randint(1, 49408, (4, 16), device=dev)
vis = torch.randint(0, 256, (4, 16), device=dev)
mp = {'T1_n': 2, 'T2_n': 1, 'T3_n': 1, 'N1_n': 0.9, 'N2_n': 0.1, 'N3_n': 0.125, 'N4_n': 0.0625, 'T1_t': 2, 'T2_t': 1, 'T3_t': 1,
      'N1_t': 0.5, 'N2_t': 0.2, 'N3_t': 0., 'N4_t': 0., 'T': 4, 'B': 2}
decode = artv.vae.decode
artv.vae.decode = lambda seq: (sampled.append(seq.clone()), decode(seq))[1]
sampled = []


def artv_call(what, B, **kw):
    torch.manual_seed(7)
    artv.generate_images(text[:B], visual=vis[:B], **kw)
    tokens = sampled.pop().cpu()
    print(f'artv {what}: tokens {tuple(tokens.shape)} sha256 {hashlib.sha256(tokens.numpy().tobytes()).hexdigest()[:16]}')


def bert_call(what, **kw):
    torch.manual_seed(7)
    img_seq = bert.generate_images(text, mask_predict_steps=0, mp_config=mp, dynamic=False, **kw)[2].cpu()
    print(f'bert {what}: img_seq {tuple(img_seq.shape)} sha256 {hashlib.sha256(img_seq.numpy().tobytes()).hexdigest()[:16]}')


for _ in range(2):
    bert_call('plain')
    bert_call('guided', guidance_scale=2.0, guidance_drop=('text', ))
    bert_call('top_k 8', top_k=8)  # [truncate -> plain race] at every step
    bert_call('guided, top_p 0.9', guidance_scale=2.0, guidance_drop=('text', ), top_p=0.9)  # the guided truncation, then the plain race
    artv_call('batch 4', 4)  # the captured five-launch step
    artv_call('batch 4, filter_thres 0.999', 4, filter_thres=0.999)  # a filter_thres that filters: the eager torch.topk path
    artv_call('batch 4, top_k 8', 4, top_k=8)  # [head -> truncate -> draw -> embed -> tower] captured
    artv_call('batch 4, guided', 4, guidance_scale=2.0)  # 8 tower rows, the guided token-only race, captured
    artv_call('batch 4, guided, top_k 8', 4, guidance_scale=2.0, top_k=8)  # the guided truncation into its own buffer, then the plain race
    artv_call('batch 2', 2)  # one persistent launch per token
torch.cuda.synchronize()
print('done')
