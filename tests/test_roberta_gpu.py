"""mmvid_amd.roberta on the MI355X: the kernels of csrc/roberta.hip, the erf-GELU epilogue of the GEMM and the key-length attention
against torch restatements, and the whole encoder (2 layers at width 128; roberta-large's 24 x 1024 configuration) against
transformers' RobertaModel driven through the reference's own get_fixed_language_model (tests/golden/roberta_{tiny,large24}.npz,
tools/make_golden.py::_roberta_case).

Bars: every encoder GEMM rounds its operands to bf16 (2^-9 relative per operand) and accumulates in fp32; LayerNorm, the residual
stream and pooling are fp32.  Post-LN renormalises every sublayer, so the error does not grow with depth the way a pre-LN tower's
does.  Measured on the MI355X (worst row): 2 layers -- last_hidden_state cosine 0.999983, pooled cosine 0.9999903 (relative error
4.4e-3); 24 layers -- 0.999827 and 0.9998118 (1.9e-2).  Bars 0.9999 / 0.9995.  A sentence alone and padded into a longer batch:
bitwise equal (key tiles past key_len are skipped, the GEMMs are row-independent, pooling skips padded rows)."""
import json
import os
import shutil
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BPE = os.path.join(GOLDEN, 'roberta_bpe')


def _model(g):
    from mmvid_amd.roberta import RobertaConfig, RobertaModel
    from oracle.synth import synth_state_dict
    m = RobertaModel(RobertaConfig(**g.meta['config']))
    m.load_state_dict(synth_state_dict(g.manifest, g.meta['seed']))
    return m.requires_grad_(False).eval().to(DEV)


def _cos(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).min().item()


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('M,N,K,f32out', [(1200, 4096, 1024, False), (350, 512, 128, False), (77, 136, 64, True), (1200, 256, 1024, True)])
def test_gemm_erf_gelu_epilogue(M, N, K, f32out):
    """act = 2: 0.5 x (1 + erf(x / sqrt 2)) of the fp32 accumulator (+ bias), against F.gelu on the same bf16 operands."""
    from mmvid_amd import _lib, ops
    torch.manual_seed(M + N)
    A = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    W = (torch.randn(N, K, device=DEV) * K**-0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV) * 0.5
    ref = F.gelu(A.float() @ W.float().t() + b)
    got = ops.gemm(A, W, bias=b, act=2, out_dtype=torch.float32 if f32out else torch.bfloat16).float()
    if f32out:
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
    else:
        torch.testing.assert_close(got, ref.to(torch.bfloat16).float(), rtol=8e-3, atol=2e-3)
    with pytest.raises(_lib.MMVIDError, match='forward only'):
        ops.gemm(A, W, act=2, dact_pre=torch.zeros(M, N, device=DEV, dtype=torch.bfloat16))


def _attn(qkv, B, L, H, E, key_len):
    from mmvid_amd import _lib, ops
    out = torch.full((B * L, E), float('nan'), device=DEV, dtype=torch.bfloat16)
    _lib.call('mmvid_attention_fwd_keylen', ops._p(qkv), 3 * E, B, L, H, E, 0.125, ops._p(key_len), ops._p(out), E, None, ops._stream())
    return out


@pytest.mark.parametrize('L', [7, 50, 64, 77, 130])
def test_keylen_attention_vs_sdpa(L):
    """Keys >= key_len[b] excluded for every query row (transformers' key-padding mask), against SDPA on the same bf16 operands;
    padded keys / values hold NaN (never read: their tiles are skipped or zero-filled); padded query rows are finite."""
    B, H = 5, 4
    E = 64 * H
    torch.manual_seed(L)
    lens = [2, L, max(1, L // 2), min(L, 3 + L // 3), max(1, L - 1)]
    qkv = torch.randn(B, L, 3 * E, device=DEV).to(torch.bfloat16)
    ref_in = qkv.float().clone()
    for b, n in enumerate(lens):
        qkv[b, n:, E:] = float('nan')
    kl = torch.tensor(lens, device=DEV, dtype=torch.int32)
    got = _attn(qkv.view(B * L, 3 * E), B, L, H, E, kl).view(B, L, H, 64).float()
    assert torch.isfinite(got).all()
    q, k, v = (ref_in[..., i * E:(i + 1) * E].view(B, L, H, 64).transpose(1, 2) for i in range(3))
    keep = torch.arange(L, device=DEV)[None, :] < kl[:, None].long()
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=keep[:, None, None, :]).transpose(1, 2)
    torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2)


def test_embedding_positions_and_layernorm():
    """Position ids of create_position_ids_from_input_ids, bit for bit: a one-hot position table (row p = 8 e_p) makes the position
    each row used the argmax of its LayerNorm output; then random tables against torch in fp32, the bf16 copy = bf16(fp32 copy)."""
    from mmvid_amd import _lib, ops
    B, L, E, V, P = 4, 70, 1024, 300, 514
    torch.manual_seed(0)
    ids = torch.randint(3, V, (B, L))
    lens = [L, 1, 33, 64]
    for b, n in enumerate(lens):
        ids[b, n:] = 1
    ids[2, 5] = 1  # a pad id inside the live prefix: position pad, and it stays attended (the mask, not the id, decides)
    mask = (torch.arange(L)[None] < torch.tensor(lens)[:, None]).long()
    pos_ids = torch.where(ids != 1, torch.cumsum((ids != 1).long(), 1) + 1, torch.ones_like(ids))

    def run(word, pos, type0, w, b, m):
        x = torch.empty(B * L, E, device=DEV)
        xb = torch.empty(B * L, E, device=DEV, dtype=torch.bfloat16)
        kl = torch.empty(B, device=DEV, dtype=torch.int32)
        _lib.call('mmvid_roberta_embed', ops._p(ids.to(DEV)), ops._p(m), B, L, ops._p(word), V, ops._p(pos), P, ops._p(type0), ops._p(w),
                  ops._p(b), 1e-5, E, 1, ops._p(x), ops._p(xb), ops._p(kl), ops._stream())
        return x.view(B, L, E), xb.view(B, L, E), kl

    onehot = torch.zeros(P, E, device=DEV)
    onehot[torch.arange(P), torch.arange(P)] = 8.0
    zeros = torch.zeros(V, E, device=DEV)
    x, _, kl = run(zeros, onehot, torch.zeros(1, E, device=DEV), torch.ones(E, device=DEV), torch.zeros(E, device=DEV), mask.to(DEV))
    assert torch.equal(x.argmax(-1).cpu(), pos_ids)
    assert kl.cpu().tolist() == lens
    word, pos, type0 = torch.randn(V, E, device=DEV) * 0.05, torch.randn(P, E, device=DEV) * 0.05, torch.randn(1, E, device=DEV) * 0.05
    w, b = 1 + 0.1 * torch.randn(E, device=DEV), 0.02 * torch.randn(E, device=DEV)
    x, xb, kl = run(word, pos, type0, w, b, mask.to(DEV))
    ref = F.layer_norm(word[ids.to(DEV)] + type0[0] + pos[pos_ids.to(DEV)], (E, ), w, b, 1e-5)
    torch.testing.assert_close(x, ref, rtol=1e-5, atol=2e-5)
    assert torch.equal(xb, x.to(torch.bfloat16))
    assert kl.cpu().tolist() == lens
    with pytest.raises(_lib.MMVIDError, match='prefix'):  # no mask: key_len counts the non-pad ids, and row 2 has a pad inside
        run(word, pos, type0, w, b, None)
    bad = mask.clone()
    bad[0, 3] = 0  # a hole: not expressible as a key length
    with pytest.raises(_lib.MMVIDError, match='prefix'):
        run(word, pos, type0, w, b, bad.to(DEV))


def test_masked_mean_pooling():
    """utils/utils.py:53-59 on the kernel; padded rows hold NaN and are skipped, not multiplied by 0; an all-zero mask gives 0."""
    from mmvid_amd.roberta import mean_pooling
    torch.manual_seed(1)
    B, L, E = 6, 50, 1024
    x = torch.randn(B, L, E, device=DEV)
    lens = [50, 1, 2, 17, 49, 0]
    mask = (torch.arange(L)[None] < torch.tensor(lens)[:, None]).long().to(DEV)
    ref = (x * mask[..., None].float()).sum(1) / mask.sum(1, keepdim=True).float().clamp(min=1e-9)
    x[mask == 0] = float('nan')
    got = mean_pooling((x, ), mask)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    assert (got[5] == 0).all()


# ---------------------------------------------------------------------------------------------- whole encoder
@pytest.mark.parametrize('name,cos_bar', [('roberta_tiny', 0.9999), ('roberta_large24', 0.9995)])
def test_encoder_vs_reference(golden, name, cos_bar, tmp_path):
    """last_hidden_state (valid rows) and the pooled features of the reference's encode_text; then the same through this package's
    get_fixed_language_model from a local checkpoint directory, which must equal model + mean_pooling bit for bit."""
    from mmvid_amd.roberta import get_fixed_language_model, mean_pooling
    g = golden(name)
    m = _model(g)
    ids, mask = g['input_ids'].to(DEV), g['attention_mask'].to(DEV)
    h = m(input_ids=ids, attention_mask=mask)[0]
    assert h.shape == (*ids.shape, g.meta['config']['hidden_size']) and h.dtype == torch.float32
    hs = h[:, :, ::8].cpu()
    valid = g['attention_mask'].bool()
    cos_h = _cos(hs[valid], g['last_hidden_state_s'][valid])
    pooled = mean_pooling((h, ), mask)
    cos_p = _cos(pooled, g['pooled'])
    rel = ((pooled.cpu().double() - g['pooled'].double()).norm(dim=-1) / g['pooled'].double().norm(dim=-1)).max().item()
    print(f'{name}: last_hidden_state cosine {cos_h:.6f}, pooled cosine {cos_p:.7f}, pooled relative error {rel:.2e}')
    assert cos_h >= cos_bar and cos_p >= cos_bar
    # the reference's entry point, from a directory that looks like a hub download
    d = tmp_path / 'roberta'
    d.mkdir()
    (d / 'config.json').write_text(json.dumps(dict(g.meta['config'], model_type='roberta')))
    torch.save({'roberta.' + k: v.cpu() for k, v in m.state_dict().items()}, str(d / 'pytorch_model.bin'))
    for f in ('vocab.json', 'merges.txt'):
        shutil.copy(os.path.join(BPE, f), str(d / f))
    args = types.SimpleNamespace(fixed_language_model=str(d), text_seq_len=g.meta['text_seq_len'])
    tok2, lm, dim, encode_text = get_fixed_language_model(args)
    assert dim == g.meta['config']['hidden_size']  # (the reference hard-codes 1024: roberta-large's width)
    if name == 'roberta_large24':
        assert dim == g.meta['text_feature_dim']
    enc = tok2(g.meta['descriptions'], return_tensors='pt', padding=True, truncation=True, max_length=args.text_seq_len)
    assert torch.equal(enc['input_ids'], g['input_ids']) and torch.equal(enc['attention_mask'], g['attention_mask'])
    feats = encode_text(g.meta['descriptions'])
    assert torch.equal(feats, pooled)


def test_sentence_alone_equals_in_padded_batch(golden):
    """A sentence's feature does not depend on the batch it is padded into (RoBERTa masks padded keys; pooling skips padded rows)."""
    from mmvid_amd.roberta import RobertaTokenizer, mean_pooling
    g = golden('roberta_large24')
    m = _model(g)
    tok = RobertaTokenizer.from_pretrained(BPE)
    d = g.meta['descriptions']
    short = d[2]

    def feat(texts):
        e = tok(texts, max_length=50)
        ids, mask = e['input_ids'].to(DEV), e['attention_mask'].to(DEV)
        return mean_pooling(m(input_ids=ids, attention_mask=mask), mask)
    alone = feat([short])[0]
    batched = feat([d[3], short, d[6]])[1]  # padded from its own length to 50
    diff = (alone - batched).abs().max().item()
    print('alone vs batched: max |diff|', diff, 'bitwise' if torch.equal(alone, batched) else 'not bitwise')
    assert diff <= 1e-5 * max(1.0, alone.abs().max().item())


def test_encode_text_feeds_bert_training_step(golden, tmp_path):
    """train.py:274-290 end to end: encode_text's features as BERT's `text` (fixed_language_model='roberta-large',
    text_feature_dim=1024): finite losses and gradients, equal to the losses of the same features passed in directly."""
    from test_host_logic import tiny_bert
    from test_models_gpu import load_synth

    from mmvid_amd.roberta import RobertaTokenizer, mean_pooling
    gr = golden('roberta_large24')
    lm = _model(gr)
    tok = RobertaTokenizer.from_pretrained(BPE)
    gb = golden('bert_flm')
    B = gb['target_tok'].shape[0]
    with torch.no_grad():
        e = tok(gr.meta['descriptions'][:B], max_length=50)
        ids, mask = e['input_ids'].to(DEV), e['attention_mask'].to(DEV)
        feat = mean_pooling(lm(input_ids=ids, attention_mask=mask), mask)
    assert feat.shape == (B, 1024) and torch.isfinite(feat).all()

    def step(text):
        m = load_synth(tiny_bert(fixed_language_model='roberta-large', text_feature_dim=1024, text_emb_bottleneck=None), gb, 23).train()
        lm_, lr_, lv_ = m(text, target=gb['target_tok'].to(DEV), return_loss=True, rel=True, vid=True, rel_no_fully_masked=True,
                          _mask1=gb['mask1'], _target_warp=gb['warp_tok'])
        loss = 7 * lm_ + 0.5 * lr_ + 0.5 * lv_
        loss.backward()
        g = m.text_feature_mapping.weight.grad
        return loss.detach(), g
    l1, g1 = step(feat)
    l2, g2 = step(feat.clone())
    assert torch.isfinite(l1) and g1 is not None and torch.isfinite(g1).all() and g1.abs().sum() > 0
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
