"""mmvid_amd.clip_model on the MI355X: the kernels of csrc/clip.hip against torch restatements, and the whole CLIP (ViT-B/32 shapes,
2 and 12 layers) against the reference's own outputs (tests/golden/clip_vit{2,12}.npz, tools/make_golden.py::_clip_case).

Bars from the bf16 error model: the patch GEMM and every tower GEMM round their operands to bf16 (relative 2^-9 per operand) and
accumulate in fp32; LayerNorm, pooling, projection and the scores are fp32.  A 12-layer tower measured 1-2 % relative error on its
output (tests/test_round3_gpu.py::test_tower_12_layers_at_training_length_vs_reference); a projected, pooled row averages that error over
its 512 features, so its direction (cosine >= 0.999) and norm (within 2 %) are held to the tower12 bars.  Cosine scores of unit
vectors move by at most |d cos| <= |e_img| + |e_txt| ~ 2 x (1 - 0.999)^0.5 x |cos| in the worst case and far less for random error:
5e-3 absolute; logits are 100 x scores: 0.1 absolute.
Measured on the MI355X (worst of the two goldens): encode_image cosine 0.99998, norm 0.034 %; encode_text cosine 0.99997, norm
0.026 %; logits 9.1e-3; clip_similarity 6.2e-4; ln_final token features 0.60 % relative; the assembled image sequence 1.3e-2 max,
0.23 % relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073])[:, None, None]
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711])[:, None, None]


def _tokenizer(tmp_path_factory):
    import lzma
    import os

    from conftest import GOLDEN
    from mmvid_amd.data import SimpleTokenizer
    path = tmp_path_factory.mktemp('bpe') / 'bpe_simple_vocab_16e6.txt'
    with lzma.open(os.path.join(GOLDEN, 'bpe_merges.txt.xz'), 'rb') as src:
        path.write_bytes(src.read())
    return SimpleTokenizer(str(path))


@pytest.fixture(scope='module')
def tok(tmp_path_factory):
    return _tokenizer(tmp_path_factory)


def _golden_model(g):
    """The golden case's CLIP: synthetic weights of its seed keyed by the reference manifest, logit_scale = log(1 / 0.07)."""
    from mmvid_amd.clip_model import CLIP
    from oracle.synth import synth_state_dict
    L = g.meta['layers']
    m = CLIP(512, 224, L, 768, 32, 77, 49408, 512, 8, L)
    sd = synth_state_dict(g.manifest, g.meta['seed'])
    sd['logit_scale'] = torch.tensor(g.meta['logit_scale'], dtype=torch.float32)
    m.load_state_dict(sd)
    return m.requires_grad_(False).eval().to(DEV)


def _golden_inputs(g):
    from oracle.synth import synth_input
    seed = g.meta['seed']
    frames = synth_input('clip_frames128', (6, 3, 128, 128), seed, 'uniform')
    frames224 = synth_input('clip_frames224', (2, 3, 224, 224), seed)
    images = torch.cat([(F.interpolate(frames, (224, 224)) - MEAN) / STD, frames224])
    return frames, images


def _unfold(x, P=32):
    N, C, S, _ = x.shape
    G = S // P
    return x.reshape(N, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(N * G * G, C * P * P)


def _cos_norm(got, ref):
    got, ref = got.double().cpu(), ref.double()
    cos = (got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))
    return cos.min().item(), (got.norm(dim=-1) / ref.norm(dim=-1) - 1).abs().max().item()


@pytest.mark.parametrize('normalize', [1, 0])
@pytest.mark.parametrize('N', [1, 7])
@pytest.mark.parametrize('S', [96, 128, 224, 256])
def test_patchify_bit_exact(S, N, normalize):
    """Patch matrix = torch's F.interpolate (nearest) -> (x - mean) / std in fp32 -> unfold -> bf16, bit for bit (the resize and the
    normalisation on the CPU: ATen's nearest index rule and IEEE fp32 division)."""
    from mmvid_amd.clip_model import patchify
    if not normalize and S != 224:
        with pytest.raises(Exception, match='input resolution'):
            patchify(torch.rand(N, 3, S, S, device=DEV), 224, 32, 0)
        return
    g = torch.Generator().manual_seed(S * 10 + N)
    x = torch.rand(N, 3, S, S, generator=g) if normalize else torch.randn(N, 3, S, S, generator=g)
    ref = x
    if normalize:
        if S != 224:
            ref = F.interpolate(ref, (224, 224))
        ref = (ref - MEAN) / STD
    ref = _unfold(ref).to(torch.bfloat16)
    got = patchify(x.to(DEV), 224, 32, normalize).cpu()
    assert got.shape == ref.shape == (N * 49, 3072)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_image_sequence_vs_fp32_torch(golden):
    """Patch GEMM (bf16 operands, fp32 accumulation), class token, positional embedding and ln_pre against conv2d / cat / add /
    layer_norm in fp32."""
    m = _golden_model(golden('clip_vit2'))
    frames = torch.rand(5, 3, 128, 128, generator=torch.Generator().manual_seed(3))
    got = m._image_sequence(frames.to(DEV), True).cpu()
    v = {k: p.detach().cpu() for k, p in m.visual.named_parameters()}
    x = F.conv2d((F.interpolate(frames, (224, 224)) - MEAN) / STD, v['conv1.weight'], stride=32).flatten(2).transpose(1, 2)
    x = torch.cat([v['class_embedding'].expand(5, 1, 768), x], 1) + v['positional_embedding']
    ref = F.layer_norm(x, (768, ), v['ln_pre.weight'], v['ln_pre.bias'], 1e-5)
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f'MEASURED image sequence: max |err| {err:.3e}, relative {rel:.3e}')
    assert got.shape == (5, 50, 768) and err < 5e-2 and rel < 5e-3


def test_text_pool_index_first_maximum():
    """The pooling index of the text embedding kernel = torch.argmax (first maximum): repeated maximum, all-zero row, a row filled to
    the context length, a maximum at the last position."""
    from mmvid_amd import _lib, ops
    from mmvid_amd.clip_model import CLIP
    g = torch.Generator().manual_seed(5)
    text = torch.zeros(5, 77, dtype=torch.long)
    text[0, :10] = torch.tensor([320, 2533, 533, 49000, 12, 49000, 7, 49000, 3, 1])
    text[2] = torch.randint(1, 49408, (77, ), generator=g)  # truncated: every position holds an id
    text[3, :40] = torch.randint(1, 30000, (40, ), generator=g)
    text[3, 76] = 40000
    text[4, 5:9] = 777
    m = CLIP(512, 224, 1, 768, 32, 77, 49408, 512, 8, 1).requires_grad_(False).to(DEV)
    E = 512
    out = torch.empty(5, 77, E, device=DEV)
    pool = torch.full((5, ), -1, device=DEV, dtype=torch.int32)
    _lib.call('mmvid_clip_text_embed', ops._p(text.to(DEV)), 5, 77, ops._p(m.token_embedding.weight), 49408, ops._p(m.positional_embedding),
              E, ops._p(out), ops._p(pool), ops._stream())
    assert pool.cpu().long().tolist() == text.argmax(-1).tolist() == [3, 0, int(text[2].argmax()), 76, 5]
    ref = m.token_embedding.weight.cpu()[text] + m.positional_embedding.cpu()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize('name', ['clip_vit2', 'clip_vit12'])
def test_clip_vs_reference(golden, tok, name):
    from mmvid_amd.clip_model import clip_encode_image, clip_similarity
    g = golden(name)
    m = _golden_model(g)
    frames, images = _golden_inputs(g)
    text = g['text'].to(DEV)
    meas = {}
    for what, got, ref in (('encode_image', m.encode_image(images.to(DEV)), g['encode_image']),
                           ('encode_text', m.encode_text(text), g['encode_text'])):
        cos, dn = _cos_norm(got, ref)
        meas[what] = (cos, dn)
        assert cos >= 0.999 and dn <= 2e-2, (what, cos, dn)
    # clip_encode_image = the normalised encode_image of its own resize / normalise
    ci = clip_encode_image(m, frames.to(DEV)).cpu().double()
    ref6 = g['encode_image'][:6].double()
    assert (ci * (ref6 / ref6.norm(dim=-1, keepdim=True))).sum(-1).min() >= 0.999
    lpi, lpt = m(images.to(DEV), text)
    meas['logits'] = max((lpi.cpu() - g['logits_per_image']).abs().max().item(), (lpt.cpu() - g['logits_per_text']).abs().max().item())
    assert meas['logits'] <= 0.1
    sims = np.stack([clip_similarity(m, tok, frames[3 * v:3 * v + 3].to(DEV), [g.meta['descriptions'][v]]) for v in range(2)])
    ref = g['similarity'].numpy()
    meas['similarity'] = float(np.abs(sims - ref).max())
    assert sims.shape == ref.shape and meas['similarity'] <= 5e-3
    for row, rrow in zip(sims, ref):
        top = np.sort(rrow)[::-1]
        if top[0] - top[1] > 2e-2:
            assert row.argmax() == rrow.argmax()
    feats = m.encode_text_tokens(text)[:, :, ::8].cpu()
    meas['token_features'] = ((feats - g['token_features_s']).norm() / g['token_features_s'].norm()).item()
    assert feats.shape == g['token_features_s'].shape and meas['token_features'] < 2e-2
    print(f'MEASURED {name}: ' + ', '.join(f'{k} {v}' for k, v in meas.items()))


def test_clip_score_equals_per_video_calls(golden, tok):
    """clip_score over B = 16 videos of T = 8 frames = 16 clip_similarity calls, and a 300-frame video = its slices, bit for bit (every
    kernel on the path computes a row from that row alone, in a fixed order)."""
    from mmvid_amd.clip_model import clip_score, clip_similarity
    m = _golden_model(golden('clip_vit2'))
    gen = torch.Generator().manual_seed(11)
    videos = torch.rand(16, 8, 3, 128, 128, generator=gen).to(DEV)
    desc = [f'a person number {i} is talking' + ' and smiling' * (i % 3) for i in range(16)]
    s = clip_score(m, tok, videos, desc)
    assert s.shape == (16, 8) and s.dtype == torch.float32
    each = np.stack([clip_similarity(m, tok, videos[b], [desc[b]]) for b in range(16)])
    assert np.array_equal(s.cpu().numpy(), each)
    long = torch.rand(1, 300, 3, 96, 96, generator=gen).to(DEV)
    whole = clip_score(m, tok, long, ['a long video'])
    parts = torch.cat([clip_score(m, tok, long[:, a:b], ['a long video']) for a, b in ((0, 100), (100, 257), (257, 300))], 1)
    assert torch.equal(whole, parts)
