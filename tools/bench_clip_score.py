#!/usr/bin/env python3
"""clip_score (mmvid_amd.clip_model) at N = 8, 128 and 1,024 frames of 128 x 128 (videos of 8 frames, one description each), and
the same weights through a stock-PyTorch eager CLIP built here (F.interpolate, F.conv2d, nn.MultiheadAttention, bf16 autocast) as a
same-box yardstick.  Prints one JSON line per (path, N): ms per call (HIP events around `reps` calls after a warm-up), frames/s and
TFLOP/s of the algorithmic count: per frame, layers x T tokens x 2 x 12 x width^2 + the patch GEMM ((T - 1) x 2 x 3 P^2 x width); per
description, layers x 77 tokens x 2 x 12 x width^2 (attention scores not counted).  At ViT-B/32: 12 x 50 x 2 x 12 x 768^2 +
49 x 2 x 3072 x 768 and 12 x 77 x 2 x 12 x 512^2.  --arch picks the shape of an OpenAI ViT checkpoint (random weights).

    python tools/bench_clip_score.py [--reps 10] [--sizes 8,128,1024] [--arch B/32|B/16|L/14|L/14@336]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

from mmvid_amd.clip_model import CLIP, clip_score

DEV = 'cuda'
ARCHS = {  # CLIP's constructor arguments (clip_model.py:298-311) of OpenAI's ViT checkpoints
    'B/32': (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    'B/16': (512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    'L/14': (768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    'L/14@336': (768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
}
MEAN = [0.48145466, 0.4578275, 0.40821073]
STD = [0.26862954, 0.26130258, 0.27577711]


class StockBlock(nn.Module):
    def __init__(self, w, h):
        super().__init__()
        self.attn = nn.MultiheadAttention(w, h)
        self.ln_1, self.ln_2 = nn.LayerNorm(w), nn.LayerNorm(w)
        self.mlp = nn.Sequential()
        self.mlp.add_module('c_fc', nn.Linear(w, 4 * w))
        self.mlp.add_module('c_proj', nn.Linear(4 * w, w))

    def forward(self, x, mask):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        h = self.mlp.c_fc(self.ln_2(x))
        return x + self.mlp.c_proj(h * torch.sigmoid(1.702 * h))


class StockTower(nn.Module):
    def __init__(self, w, layers, h):
        super().__init__()
        self.resblocks = nn.ModuleList([StockBlock(w, h) for _ in range(layers)])

    def forward(self, x, mask=None):
        for b in self.resblocks:
            x = b(x, mask)
        return x


class StockCLIP(nn.Module):
    """Eager CLIP with the reference's structure (clip_model.py:249-432), for timing only."""

    def __init__(self, m):
        super().__init__()
        sd = m.state_dict()
        vis, txt = m.visual.tower, m.text_tower
        self.R, self.P, self.vw, self.tw = m._shape['R'], m._shape['P'], vis.width, txt.width
        self.conv1 = sd['visual.conv1.weight']
        self.cls, self.vpos = sd['visual.class_embedding'], sd['visual.positional_embedding']
        self.ln_pre, self.ln_post, self.proj = (sd['visual.ln_pre.weight'], sd['visual.ln_pre.bias']), (sd['visual.ln_post.weight'], sd['visual.ln_post.bias']), sd['visual.proj']
        self.visual = StockTower(vis.width, vis.layers, vis.heads)
        self.visual.load_state_dict({k[len('visual.transformer.'):]: v for k, v in sd.items() if k.startswith('visual.transformer.')})
        self.text = StockTower(txt.width, txt.layers, txt.heads)
        self.text.load_state_dict({k[len('transformer.'):]: v for k, v in sd.items() if k.startswith('transformer.')})
        self.tok, self.tpos, self.ln_final, self.tproj = sd['token_embedding.weight'], sd['positional_embedding'], (sd['ln_final.weight'], sd['ln_final.bias']), sd['text_projection']
        self.mask = torch.full((77, 77), float('-inf'), device=self.tok.device).triu_(1)

    def score(self, videos, text):
        B, T = videos.shape[:2]
        x = F.interpolate(videos.reshape(B * T, *videos.shape[2:]), (self.R, self.R))
        x = (x - torch.tensor(MEAN, device=x.device)[:, None, None]) / torch.tensor(STD, device=x.device)[:, None, None]
        x = F.conv2d(x, self.conv1, stride=self.P).flatten(2).transpose(1, 2)
        x = torch.cat([self.cls.to(x.dtype).expand(x.shape[0], 1, -1), x], 1) + self.vpos
        x = F.layer_norm(x, (self.vw, ), *self.ln_pre)
        x = self.visual(x.permute(1, 0, 2)).permute(1, 0, 2)
        img = F.layer_norm(x[:, 0], (self.vw, ), *self.ln_post) @ self.proj
        t = self.tok[text] + self.tpos
        t = self.text(t.permute(1, 0, 2), self.mask).permute(1, 0, 2)
        txt = F.layer_norm(t, (self.tw, ), *self.ln_final)[torch.arange(B), text.argmax(-1)] @ self.tproj
        img = img.float() / img.float().norm(dim=-1, keepdim=True)
        txt = txt.float() / txt.float().norm(dim=-1, keepdim=True)
        return (img.view(B, T, -1) * txt[:, None]).sum(-1)


class IdTokenizer:
    """Stands in for SimpleTokenizer (whose merge table is not needed to time the model): fixed ids, 20 per description."""

    def tokenize(self, texts, context_length, truncate_text=False):
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i in range(len(texts)):
            out[i, :20] = torch.arange(1000 + 20 * i, 1020 + 20 * i)
        return out


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='8,128,1024')
    ap.add_argument('--arch', default='B/32', choices=list(ARCHS))
    args = ap.parse_args()
    torch.manual_seed(0)
    shape = ARCHS[args.arch]
    m = CLIP(*shape).requires_grad_(False).eval().to(DEV)
    tokens = (shape[1] // shape[4])**2 + 1
    frame_flop = shape[2] * tokens * 2 * 12 * shape[3]**2 + (tokens - 1) * 2 * 3 * shape[4]**2 * shape[3]
    text_flop = shape[9] * 77 * 2 * 12 * shape[7]**2
    stock = StockCLIP(m).to(DEV).eval()
    tok = IdTokenizer()
    for n in (int(s) for s in args.sizes.split(',')):
        B, T = max(1, n // 8), min(8, n)
        videos = torch.rand(B, T, 3, 128, 128, device=DEV)
        desc = [f'video {i}' for i in range(B)]
        text = tok.tokenize(desc, 77).to(DEV)
        ours = clip_score(m, tok, videos, desc)
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            ref = stock.score(videos, text)
        diff = (ours - ref.float()).abs().max().item()
        flop = B * T * frame_flop + B * text_flop
        for path, fn in (('mmvid_amd.clip_score', lambda: clip_score(m, tok, videos, desc)),
                         ('stock_pytorch_bf16_autocast', lambda: stock.score(videos, text))):
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=path.startswith('stock')):
                ms = timeit(fn, args.reps)
            print(json.dumps(dict(path=path, arch=args.arch, frames=B * T, videos=B, size=128, ms=round(ms, 3), frames_per_s=round(B * T / ms * 1e3, 1),
                                  tflops=round(flop / ms / 1e9, 2), max_abs_score_diff_vs_stock=round(diff, 5))), flush=True)


if __name__ == '__main__':
    main()
