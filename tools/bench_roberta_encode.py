#!/usr/bin/env python3
"""encode_text of `--fixed_language_model roberta-large` (mmvid_amd.roberta.get_fixed_language_model) at 24 x 50 tokens (the
text_augment recipe's batch and text_seq_len) and 64 x 50, and the same weights through a stock-PyTorch eager restatement of
transformers' RobertaModel (nn.Linear, F.scaled_dot_product_attention with the key-padding mask, F.layer_norm, F.gelu) in fp32 -- the
reference's precision -- and under bf16 autocast, as same-box yardsticks.  roberta-large's configuration with random weights (timing
only); captions of the vox_text grammar tokenised with the tests' synthetic BPE vocabulary, one of them long enough to pad every
batch to 50.  One JSON line per (path, B): ms per call (HIP events around `reps` calls after a warm-up) and TFLOP/s of
2 x 302 M non-embedding parameters x B x L (attention scores not counted).

    python tools/bench_roberta_encode.py [--reps 20] [--sizes 24,64]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from mmvid_amd.roberta import RobertaConfig, RobertaModel, RobertaTokenizer, mean_pooling
from mmvid_amd.vox_text import generate_random_sentences

DEV = 'cuda'
L_MAX = 50


def random_model():
    torch.manual_seed(0)
    m = RobertaModel(RobertaConfig())
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(1 + 0.1 * torch.randn_like(p) if k.endswith('LayerNorm.weight') else 0.02 * torch.randn_like(p))
    return m.requires_grad_(False).eval().to(DEV)


def stock_forward(sd, c, ids, mask):
    """transformers' RobertaModel forward (post-LN layers, additive-mask attention) restated in eager PyTorch."""
    E, H = c.hidden_size, c.num_attention_heads
    pos = torch.where(ids != 1, torch.cumsum((ids != 1).long(), 1) + 1, torch.ones_like(ids))
    x = sd['embeddings.word_embeddings.weight'][ids] + sd['embeddings.token_type_embeddings.weight'][0] + sd['embeddings.position_embeddings.weight'][pos]
    x = F.layer_norm(x, (E, ), sd['embeddings.LayerNorm.weight'], sd['embeddings.LayerNorm.bias'], c.layer_norm_eps)
    B, L = ids.shape
    keep = mask.bool()[:, None, None, :]
    for i in range(c.num_hidden_layers):
        p = lambda n: sd[f'encoder.layer.{i}.{n}']
        q, k, v = (F.linear(x, p(f'attention.self.{n}.weight'), p(f'attention.self.{n}.bias')).view(B, L, H, 64).transpose(1, 2)
                   for n in ('query', 'key', 'value'))
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=keep).transpose(1, 2).reshape(B, L, E)
        x = F.layer_norm(F.linear(o, p('attention.output.dense.weight'), p('attention.output.dense.bias')) + x, (E, ),
                         p('attention.output.LayerNorm.weight'), p('attention.output.LayerNorm.bias'), c.layer_norm_eps)
        h = F.gelu(F.linear(x, p('intermediate.dense.weight'), p('intermediate.dense.bias')))
        x = F.layer_norm(F.linear(h, p('output.dense.weight'), p('output.dense.bias')) + x, (E, ), p('output.LayerNorm.weight'),
                         p('output.LayerNorm.bias'), c.layer_norm_eps)
    m = mask[..., None].to(x.dtype)
    return (x * m).sum(1) / m.sum(1).clamp(min=1e-9)


def timed(fn, reps):
    for _ in range(3):
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='24,64')
    args = ap.parse_args()
    tok = RobertaTokenizer.from_pretrained(os.path.join(ROOT, 'tests', 'golden', 'roberta_bpe'))
    model = random_model()
    c = model.config
    sd = {k: v for k, v in model.state_dict().items()}
    flop_per_token = 2 * c.num_hidden_layers * (4 * c.hidden_size**2 + 2 * c.hidden_size * c.intermediate_size)
    rng = random.Random(0)
    for B in (int(s) for s in args.sizes.split(',')):
        texts = generate_random_sentences(n_attr=8, n_sent=B - 1, rng=rng) + [' '.join(generate_random_sentences(n_attr=12, n_sent=4, rng=rng))]

        @torch.no_grad()
        def encode_text():  # get_fixed_language_model's encode_text: tokenise, upload, encode, pool
            e = tok(texts, return_tensors='pt', padding=True, truncation=True, max_length=L_MAX)
            ids, mask = e['input_ids'].to(DEV), e['attention_mask'].to(DEV)
            return mean_pooling(model(input_ids=ids, attention_mask=mask), mask)

        e = tok(texts, return_tensors='pt', padding=True, truncation=True, max_length=L_MAX)
        ids, mask = e['input_ids'].to(DEV), e['attention_mask'].to(DEV)
        L = ids.shape[1]
        tokens = B * L
        ref = stock_forward(sd, c, ids, mask)
        got = encode_text()
        cos = torch.nn.functional.cosine_similarity(got.double(), ref.double(), dim=-1).min().item()

        def native():
            with torch.no_grad():
                return mean_pooling(model(input_ids=ids, attention_mask=mask), mask)

        def stock32():
            with torch.no_grad():
                return stock_forward(sd, c, ids, mask)

        def stock16():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return stock_forward(sd, c, ids, mask)

        for path, fn in (('encode_text', encode_text), ('native_ids_to_features', native), ('stock_eager_fp32', stock32),
                         ('stock_eager_bf16_autocast', stock16)):
            ms = timed(fn, args.reps)
            print(json.dumps(dict(tool='bench_roberta_encode', path=path, B=B, L=L, live_tokens=int(mask.sum()), ms=round(ms, 4),
                                  tflops=round(flop_per_token * tokens / ms / 1e9, 2),
                                  **({'min_cosine_vs_stock_fp32': round(cos, 6)} if path == 'encode_text' else {}))), flush=True)


if __name__ == '__main__':
    main()
