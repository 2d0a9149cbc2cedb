"""CLIP beyond ViT-B/32 on the MI355X: the patch kernel at patch sizes that are no multiple of 8 (ViT-L/14's 14, and 7, 2), the tower
at width 1024 with 16 heads, and two whole models against the reference's own outputs (tests/golden/clip_p14_tiny.npz,
clip_vitl14_2.npz: tools/make_golden.py::_clip_case).

The patch matrix is exact: rows of Kp = 3*P*P rounded up to a multiple of 64 columns, the first 3*P*P the bits of torch's
F.interpolate (nearest) -> (x - mean) / std -> unfold -> bf16, the rest +0.0.  Every other bar is copied from the test of the same
quantity at ViT-B/32: the image sequence and the whole model from tests/test_clip_gpu.py (its bf16 error model does not depend on the
patch GEMM's K = 588 or on the width 1024: operands rounded to bf16 at relative 2^-9, fp32 accumulation), the two-layer tower from
tests/test_models_gpu.py::test_tower_forward_backward_vs_reference (max |error| <= 2e-2 max |reference|)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr
from guarded import Guarded, bits, call_abi
from test_clip_gpu import MEAN, STD, _cos_norm, _tokenizer, _unfold

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def tok(tmp_path_factory):
    return _tokenizer(tmp_path_factory)


_MODELS = {}


def _golden_model(g, name):
    """The golden case's CLIP (constructor arguments in its meta), synthetic weights of its seed keyed by the reference manifest."""
    if name not in _MODELS:
        from mmvid_amd.clip_model import CLIP
        from oracle.synth import synth_state_dict
        m = CLIP(*g.meta['shape'])
        sd = synth_state_dict(g.manifest, g.meta['seed'])
        sd['logit_scale'] = torch.tensor(g.meta['logit_scale'], dtype=torch.float32)
        m.load_state_dict(sd)
        _MODELS[name] = m.requires_grad_(False).eval().to(DEV)
    return _MODELS[name]


def _patch_reference(x, R, P, normalize):
    """The restatement of tests/test_clip_gpu.py::test_patchify_bit_exact at any (P, R), zero-padded to Kp columns."""
    ref = x
    if normalize:
        if x.shape[-1] != R:
            ref = F.interpolate(ref, (R, R))
        ref = (ref - MEAN) / STD
    ref = _unfold(ref, P).to(torch.bfloat16)
    Kp = -(-3 * P * P // 64) * 64
    return torch.cat([ref, torch.zeros(ref.shape[0], Kp - ref.shape[1], dtype=torch.bfloat16)], 1), Kp


PATCH_CASES = [(P, R, S, N, nz) for P, R in ((14, 28), (14, 56), (7, 28), (2, 8)) for S in (R, 40, 96) for N in (1, 3)
               for nz in (1, 0) if nz or S == R]


@pytest.mark.parametrize('P,R,S,N,normalize', PATCH_CASES)
def test_patchify_any_patch_bit_exact(P, R, S, N, normalize):
    """Bit for bit at P = 14, 7 and 2 (P = 2: 12 columns of data, 52 of padding), same size / upsampled by a non-integer factor /
    downsampled, through guarded buffers: the output starts as the guard's sentinel, so every element of [N*G*G][Kp] was stored,
    the pad columns hold +0.0 (not -0.0, not a leftover), and nothing outside the window was written or read."""
    g = torch.Generator().manual_seed(1000 * P + 10 * S + N)
    x = torch.rand(N, 3, S, S, generator=g) if normalize else torch.randn(N, 3, S, S, generator=g)
    ref, Kp = _patch_reference(x, R, P, normalize)
    rows = N * (R // P)**2
    assert ref.shape == (rows, Kp) and Kp % 64 == 0 and 0 < Kp - 3 * P * P < 64
    fin = Guarded(x.reshape(N * 3 * S, S))
    out = Guarded(role='out', shape=(rows, Kp), dtype=torch.bfloat16)
    call_abi('mmvid_clip_patchify', fin.ptr, N, S, R, P, normalize, out.ptr)
    fin.check('frames')
    got = out.check('patch matrix')
    assert torch.equal(bits(got), bits(ref))
    assert bool((bits(got[:, 3 * P * P:]) == 0).all())


@pytest.mark.parametrize('P,R', [(16, 32), (32, 64)])
@pytest.mark.parametrize('S', [None, 40])
def test_patchify_multiple_of_8_has_no_pad(P, R, S):
    """P a multiple of 8: Kp == 3*P*P, the kernel and the bytes of before."""
    from mmvid_amd.clip_model import patchify
    S = S or R
    x = torch.rand(3, 3, S, S, generator=torch.Generator().manual_seed(P + S))
    ref, Kp = _patch_reference(x, R, P, 1)
    assert Kp == 3 * P * P
    fin = Guarded(x.reshape(9 * S, S))
    out = Guarded(role='out', shape=ref.shape, dtype=torch.bfloat16)
    call_abi('mmvid_clip_patchify', fin.ptr, 3, S, R, P, 1, out.ptr)
    fin.check('frames')
    assert torch.equal(bits(out.check('patch matrix')), bits(ref))
    got = patchify(x.to(DEV), R, P, 1).cpu()
    assert got.shape == ref.shape and torch.equal(bits(got), bits(ref))


def test_patchify_refuses():
    from mmvid_amd.clip_model import patchify
    with pytest.raises(Exception, match='bad sizes'):
        patchify(torch.rand(1, 3, 30, 30, device=DEV), 30, 14, 1)  # 14 does not divide 30
    with pytest.raises(Exception, match='input resolution'):
        patchify(torch.rand(1, 3, 40, 40, device=DEV), 28, 14, 0)


def test_image_sequence_p14_vs_fp32_torch(golden):
    """Patch GEMM over K = 588 data + 52 zero columns, class token, positional embedding and ln_pre against conv2d (stride 14) / cat /
    add / layer_norm in fp32; the bars of tests/test_clip_gpu.py::test_image_sequence_vs_fp32_torch."""
    m = _golden_model(golden('clip_p14_tiny'), 'clip_p14_tiny')
    frames = torch.rand(5, 3, 40, 40, generator=torch.Generator().manual_seed(3))
    got = m._image_sequence(frames.to(DEV), True).cpu()
    assert m._conv_weight().shape == (256, 640) and not bool(m._conv_weight()[:, 588:].any())
    v = {k: p.detach().cpu() for k, p in m.visual.named_parameters()}
    x = F.conv2d((F.interpolate(frames, (56, 56)) - MEAN) / STD, v['conv1.weight'], stride=14).flatten(2).transpose(1, 2)
    x = torch.cat([v['class_embedding'].expand(5, 1, 256), x], 1) + v['positional_embedding']
    ref = F.layer_norm(x, (256, ), v['ln_pre.weight'], v['ln_pre.bias'], 1e-5)
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f'MEASURED image sequence P=14: max |err| {err:.3e}, relative {rel:.3e}')
    assert got.shape == (5, 17, 256) and err < 5e-2 and rel < 5e-3


def _block_fp32(x, blk, H):
    """clip_model.py's ResidualAttentionBlock (x + attn(ln_1(x)); x + c_proj(QuickGELU(c_fc(ln_2(x))))), no mask, fp32 on the CPU."""
    B, L, E = x.shape
    h = F.layer_norm(x, (E, ), blk.ln_1.weight, blk.ln_1.bias, 1e-5)
    q, k, v = (t.view(B, L, H, E // H).transpose(1, 2) for t in F.linear(h, blk.attn.in_proj_weight, blk.attn.in_proj_bias).chunk(3, -1))
    a = torch.softmax(q @ k.transpose(-1, -2) * (E // H)**-0.5, -1) @ v
    x = x + F.linear(a.transpose(1, 2).reshape(B, L, E), blk.attn.out_proj.weight, blk.attn.out_proj.bias)
    h = F.linear(F.layer_norm(x, (E, ), blk.ln_2.weight, blk.ln_2.bias, 1e-5), blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
    return x + F.linear(h * torch.sigmoid(1.702 * h), blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)


@pytest.fixture(scope='module')
def wide_tower():
    """Two layers at E = 1024, H = 16, F = 4096, no mask: the matrices at CLIP's initial scales, every bias and LayerNorm parameter
    random (their defaults, 0 and 1, would hide a bias or a scale that is not applied)."""
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    torch.manual_seed(1024)
    tw = OpenAICLIPTransformer(257, 'openai_clip_visual', causal=False, layers=2, width=1024, heads=16)
    with torch.no_grad():
        for k, p in tw.named_parameters():
            if k.endswith('bias'):
                p.normal_(0, 0.1 if '.ln_' in k else 0.02)
            elif '.ln_' in k:
                p.normal_(1, 0.1)
    tw.requires_grad_(False)
    return copy.deepcopy(tw).to(DEV), tw  # (the runner on the device, its fp32 parameters on the CPU)


@pytest.mark.parametrize('L', [17, 257])
def test_tower_width_1024_vs_fp32_torch(wide_tower, L):
    """mmvid_tower_forward at E = 1024, H = 16 (ViT-L/14's visual tower; T = 17 and T = 257) against the fp32 restatement.  Bar of the
    two-layer tower of tests/test_models_gpu.py: max |error| <= 2e-2 max |reference|."""
    x = torch.randn(2, L, 1024, generator=torch.Generator().manual_seed(L))
    tw, host = wide_tower
    ref = x
    with torch.no_grad():
        for blk in host.transformer.resblocks:
            ref = _block_fp32(ref, blk, 16)
    got, _ = tw._run_forward(x.to(DEV), keep=False)
    e = relerr(got.cpu(), ref)
    print(f'MEASURED tower E=1024 H=16 L={L}: relerr {e:.3e} (tol 2e-2)')
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and e <= 2e-2


def _golden_inputs(g):
    from oracle.synth import synth_input
    seed, (R, small) = g.meta['seed'], (g.meta['shape'][1], g.meta['small'])
    frames = synth_input(f'clip_frames{small}', (6, 3, small, small), seed, 'uniform')
    at_r = synth_input(f'clip_frames{R}', (2, 3, R, R), seed)
    return frames, torch.cat([(F.interpolate(frames, (R, R)) - MEAN) / STD, at_r])


@pytest.mark.parametrize('name', ['clip_p14_tiny', 'clip_vitl14_2'])
def test_clip_archs_vs_reference(golden, tok, name):
    """The checks and bars of tests/test_clip_gpu.py::test_clip_vs_reference on the patch-14 models."""
    from mmvid_amd.clip_model import clip_encode_image, clip_similarity
    g = golden(name)
    m = _golden_model(g, name)
    frames, images = _golden_inputs(g)
    text = g['text'].to(DEV)
    meas = {}
    for what, got, ref in (('encode_image', m.encode_image(images.to(DEV)), g['encode_image']),
                           ('encode_text', m.encode_text(text), g['encode_text'])):
        cos, dn = _cos_norm(got, ref)
        meas[what] = (cos, dn)
        assert cos >= 0.999 and dn <= 2e-2, (what, cos, dn)
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


def test_clip_score_l14_equals_its_slices(golden, tok):
    """A 60-frame video through the L/14 shape (49 frames per tower pass at T = 257: two passes) = the concatenation of three parts
    whose cuts do not fall on the pass boundary, bit for bit."""
    from mmvid_amd.clip_model import clip_score, frames_per_pass
    m = _golden_model(golden('clip_vitl14_2'), 'clip_vitl14_2')
    assert frames_per_pass(257) == 49
    video = torch.rand(1, 60, 3, 96, 96, generator=torch.Generator().manual_seed(14)).to(DEV)
    whole = clip_score(m, tok, video, ['a long video'])
    parts = torch.cat([clip_score(m, tok, video[:, a:b], ['a long video']) for a, b in ((0, 20), (20, 51), (51, 60))], 1)
    assert whole.shape == (1, 60) and bool(torch.isfinite(whole).all())
    assert torch.equal(whole, parts)
