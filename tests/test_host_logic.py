"""CPU-side checks of the product package: checkpoint layout (state_dict keys/shapes) against the manifests
captured from the reference, mask predicates, C-ABI library exports, and that nothing silently falls back to
the CPU.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def tiny_vae():
    from mmvid_amd.vae import VQGanVAE1024
    v = VQGanVAE1024(None, 64, ddconfig={'ch': 32}, n_embed=256)
    v.image_size, v.num_tokens = 64, 256
    return v


def tiny_bert(num_visuals=0, use_cvae=False, **kw):
    from mmvid_amd.dalle_bert import BERT
    return BERT(dim=768, vae=tiny_vae(), cvae=tiny_vae() if use_cvae else None, num_text_tokens=49408, text_seq_len=16,
                which_transformer='openai_clip_visual', num_visuals=num_visuals, num_targets=2, transformer_layers=2, **kw)


def manifest(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


@pytest.mark.parametrize('name,tiny', [('vqgan_tiny', True), ('vqgan_full', False)])
def test_vae_state_dict_layout_matches_reference(golden, name, tiny):
    from mmvid_amd.vae import VQGanVAE1024
    v = tiny_vae() if tiny else VQGanVAE1024(None, 128)
    assert manifest(v) == golden(name).manifest


def test_tower_state_dict_layout_matches_reference(golden):
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    t = OpenAICLIPTransformer(51, 'openai_clip_visual', causal=True, mask_type='mask_prev', mask_kwargs={'index': [17, 18]}, layers=2)
    assert manifest(t) == golden('tower').manifest
    assert t.mask_spec == ('rows', [(17, 17), (18, 18)])
    from oracle.tower import build_attention_mask
    assert torch.equal(t.dense_attention_mask(), build_attention_mask(51, 'mask_prev', [17, 18]))
    c = OpenAICLIPTransformer(40, 'openai_clip_visual', layers=2)
    assert c.mask_spec == 'causal' and torch.equal(c.dense_attention_mask(), build_attention_mask(40, 'causal'))


@pytest.mark.parametrize('name,bn', [('bert_flm', None), ('bert_flm_bottleneck', '256')])
def test_bert_fixed_language_model_layout(golden, name, bn):
    """dalle_bert.py:307-322: one text token fed by `text_feature_mapping`; no text table, no text position."""
    import torch.nn as nn
    m = tiny_bert(fixed_language_model='roberta-large', text_feature_dim=1024, text_emb_bottleneck=bn)
    assert manifest(m) == golden(name).manifest
    assert m.text_seq_len == 1 and m.num_text_tokens == 1 and m.text_emb is None and m.text_pos_emb is None
    assert m.total_seq_len == 1 + 1 + 2 + 32 and m.st1_tok_index == 2 and m.vid_tok_index == 3
    assert m._seg.tolist()[:4] == [0, 1, 0, 0]
    assert m.sparse_grad_rows() == {}
    extra = [m.text_feature_mapping] if bn is None else [m.text_feature_mapping[1], m.text_feature_mapping[3]]
    assert m.head_shadow_targets() == [m.to_logits[1]] + extra and all(isinstance(x, nn.Linear) for x in extra)
    pos = m._pos_table()
    assert pos.shape == (m.total_seq_len, 768) and float(pos[1].detach().abs().max()) == 0.0
    for bad in (dict(text_feature_dim=1020), dict(text_feature_dim=1024, text_emb_bottleneck='0'),
                dict(text_feature_dim=1024, text_emb_bottleneck=False), dict(text_feature_dim=2048, text_emb_bottleneck='256')):
        with pytest.raises(ValueError):
            tiny_bert(fixed_language_model='roberta-large', **bad)
    with pytest.raises(AssertionError):
        tiny_bert(fixed_language_model='roberta-large')  # text_feature_dim > 0 (dalle_bert.py:308)


@pytest.mark.parametrize('name,nv,cvae', [('bert_tiny', 0, False), ('bert_tiny_visual', 1, True)])
def test_bert_state_dict_layout_and_indices(golden, name, nv, cvae):
    m = tiny_bert(nv, cvae)
    assert manifest(m) == golden(name).manifest
    assert m.total_seq_len == 1 + 16 + nv * 16 + 2 + 32
    assert m.st1_tok_index == 17 + nv * 16 and m.vid_tok_index == 18 + nv * 16
    assert m.image_token_lut == {'[MASK]': 256, '[SEP]': 257}
    assert m.transformer.mask_spec == ('rows', [(m.st1_tok_index, m.st1_tok_index), (m.vid_tok_index, m.vid_tok_index)])
    assert all(not p.requires_grad for p in m.vae.parameters())
    seg = m._seg.tolist()
    assert seg[0] == 0 and seg[1:17] == [1] * 16 and seg[-32:] == [3] * 32 and len(seg) == m.total_seq_len


def test_bert_full_config_sizes():
    """Config 2 of BASELINE.json: L = 579, 124.7 M trainable parameters."""
    from mmvid_amd.dalle_bert import BERT
    from mmvid_amd.vae import VQGanVAE1024
    with torch.device('meta'):
        vae = VQGanVAE1024(None, 128)
        vae.image_size = 128
        m = BERT(dim=768, vae=vae, num_text_tokens=49408, text_seq_len=64, which_transformer='openai_clip_visual',
                 num_visuals=0, num_targets=8)
    assert m.total_seq_len == 579 and (m.st1_tok_index, m.vid_tok_index) == (65, 66)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 124705794
    assert sum(p.numel() for p in vae.parameters()) == 68201859


def test_artv_state_dict_layout(golden):
    from mmvid_amd.dalle_artv import DALLE
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16,
              which_transformer='openai_clip_visual', num_visuals=1, num_targets=2, transformer_layers=2)
    assert manifest(m) == golden('artv_tiny').manifest
    assert m.total_tokens == 49952 and m.total_seq_len == 64
    from oracle.artv import Cfg
    sd = {k: torch.empty(s) for k, s in golden('artv_tiny').manifest if 'emb.weight' in k or 'quantize' in k}
    assert torch.equal(m.logits_mask, Cfg(sd, 16, 1, 2, 64).logits_mask)
    assert m._allowed_range(0) == (0, 49424) and m._allowed_range(16) == (49424, 49424 + 272) and m._allowed_range(32)[1] == 49952


def test_erasing_box_restatement_statistics():
    """oracle/frontend.py::erasing_box (torchvision RandomErasing.get_params restated; parity unpinned): a rectangle that
    fits strictly inside the map, area fraction in the requested band."""
    from oracle.frontend import erasing_box
    rng = np.random.RandomState(0)
    fr = []
    for _ in range(2000):
        box = erasing_box(rng, 8, 8, (0.2, 0.8), (0.5, 2.0))
        if box is None:
            fr.append(0.0)
            continue
        i, j, h, w = box
        assert 0 < h < 8 and 0 < w < 8 and 0 <= i <= 8 - h and 0 <= j <= 8 - w
        fr.append(h * w / 64.0)
    assert 0.15 < np.mean(fr) < 0.6


def test_msm_mask_restatement_cpu():
    """oracle/frontend.py::msm_masks follows dalle_bert.py:992-1029: strategy 2 <=> not_fully_masked == 0 <=> nothing
    visible; strategies 3 / 4 are complementary box masks shared by all frames."""
    from oracle.frontend import msm_masks
    rng = np.random.RandomState(1)
    mask, nfm, strat = msm_masks(rng, 400, 2, 4, [0.4, 0.2, 0.2, 0.2], [0.2, 0.5])
    assert mask.shape == (400, 32) and mask.dtype == torch.bool
    assert ((nfm == 0).numpy() == (strat == 2)).all() and (~mask[strat == 2]).all()
    m3 = mask[strat == 3].view(-1, 2, 16)
    assert (m3[:, 0] == m3[:, 1]).all()  # the same box on every frame
    keep1 = mask[strat == 1].float().mean().item()
    assert 0.25 < keep1 < 0.45  # Bernoulli keep probability ~ U(0.2, 0.5)
    freq = np.bincount(strat, minlength=5)[1:] / 400.0
    assert np.allclose(freq, [0.4, 0.2, 0.2, 0.2], atol=0.08)


def test_warmup_lr_schedule_host_form():
    """engine.WarmupLR (deepspeed WarmupLR restated; utils_train.py:373-385 + the stepping rule of train.py:373-374)."""
    import math

    from mmvid_amd.engine import WarmupLR
    sc = WarmupLR(1e-6, 1e-4, 5000, every=1)
    assert sc.lr_at(0) == 1e-4  # before the scheduler's first step the optimiser keeps its construction lr
    assert abs(sc.lr_at(1) - 1e-6) < 1e-12  # first scheduler step: gamma = log(1)/log(W) = 0
    assert abs(sc.lr_at(11) - (1e-6 + (1e-4 - 1e-6) * math.log(11) / math.log(5000))) < 1e-12
    assert sc.lr_at(5001) == 1e-4 and sc.lr_at(10 ** 6) == 1e-4
    lrs = [sc.lr_at(i) for i in range(1, 5002)]
    assert all(b >= a for a, b in zip(lrs, lrs[1:]))
    assert WarmupLR(1e-6, 1e-4, 5000, every=10).lr_at(9) == 1e-4 and abs(WarmupLR(1e-6, 1e-4, 5000, every=10).lr_at(10) - 1e-6) < 1e-12


def test_face_region_tables():
    """frontend.face_choices against dalle_bert.py:796-848 / dalle_artv.py:356-416."""
    from mmvid_amd.frontend import face_choices
    ch, f0 = face_choices('face_8x8', None)
    assert [c[2] for c in ch] == [(2, 5, 1, 7), (5, 7, 2, 6)] and [c[1] for c in ch] == [1, 1] and not f0
    assert face_choices('face_8x8', 'mouth')[0] == [(1.0, 1, (5, 7, 2, 6))]
    assert face_choices('face2_8x8', None) == ([(1.0, 1, (2, 6, 2, 6))], True)
    ch, _ = face_choices('mask_8x8', None)
    assert [c[0] for c in ch] == [0.5, 0.25, 0.25] and [c[1] for c in ch] == [0, 1, 1]
    assert face_choices('mask2_8x8', 'x')[0] == [(1.0, 1, (1, 7, 1, 7))]
    assert face_choices('shape_4x4', None)[0] == [(1.0, 2, (1, 3, 1, 3))]
    with pytest.raises(NotImplementedError):
        face_choices('nope', None)


def test_clip_torchscript_archive_loads(tmp_path):
    """clip_model.py:535-559: the tower weights come out of OpenAI's TorchScript archive (fp16) -> fp32 parameters.
    A scripted stand-in archive with the same key layout and fp16 storage is written and loaded back."""
    from torch import nn

    from mmvid_amd.clip_tower import OpenAICLIPTransformer

    width, layers = 768, 2
    torch.manual_seed(0)

    class Blk(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = nn.MultiheadAttention(width, 12)
            self.ln_1, self.ln_2 = nn.LayerNorm(width), nn.LayerNorm(width)
            self.mlp = nn.Sequential()
            self.mlp.add_module('c_fc', nn.Linear(width, 4 * width))
            self.mlp.add_module('c_proj', nn.Linear(4 * width, width))

        def forward(self, x):
            return x

    class Tower(nn.Module):
        def __init__(self):
            super().__init__()
            self.resblocks = nn.ModuleList([Blk() for _ in range(layers)])

        def forward(self, x):
            for b in self.resblocks:
                x = b(x)
            return x

    class Visual(nn.Module):
        def __init__(self):
            super().__init__()
            self.transformer = Tower()

        def forward(self, x):
            return self.transformer(x)

    class Archive(nn.Module):
        def __init__(self):
            super().__init__()
            self.visual = Visual()
            self.transformer = Tower()  # the text tower (other width in the real archive; same key layout)

        def forward(self, x):
            return self.visual(x)

    arch = Archive().half()
    path = str(tmp_path / 'ViT-B-32.pt')
    torch.jit.script(arch).save(path)
    tw = OpenAICLIPTransformer(51, 'openai_clip_visual', model_path=path, causal=True, mask_type='mask_prev',
                               mask_kwargs={'index': [17, 18]}, layers=layers)
    src = arch.state_dict()
    for k, v in tw.transformer.state_dict().items():
        ref = src['visual.transformer.' + k]
        assert v.dtype == torch.float32 and torch.equal(v, ref.float()), k
    tw2 = OpenAICLIPTransformer(51, 'openai_clip_text', layers=layers, width=768, heads=12)
    tw2.load_clip_checkpoint(path, 'openai_clip_text')
    assert torch.equal(tw2.transformer.resblocks[1].mlp.c_fc.weight, src['transformer.resblocks.1.mlp.c_fc.weight'].float())


def test_divide_max_stable_option():
    """utils/utils.py:18-25 (x / amax over the last dim), wired into both models only under stable=True
    (dalle_bert.py:1000-1001, dalle_artv.py:496-497)."""
    from mmvid_amd.dalle_bert import DivideMax
    x = torch.tensor([[1.0, -4.0, 2.0], [3.0, 0.5, -2.0]])
    y = DivideMax(dim=-1)(x)
    assert torch.equal(y, x / x.amax(dim=-1, keepdim=True)) and torch.equal(y.amax(-1), torch.ones(2))
    assert tiny_bert(0, False).stable is False and not hasattr(tiny_bert(0, False), 'norm_by_max')


def test_api_surface_matches_reference_classes():
    """Every public method of the reference's BERT / DALLE / VQGanVAE1024 exists here (names captured from the reference in
    the build container), and the one helper no forward path uses behaves as dalle_bert.py:854-866."""
    from mmvid_amd.dalle_artv import DALLE
    from mmvid_amd.dalle_bert import BERT
    from mmvid_amd.vae import VQGanVAE1024
    ref = {BERT: ['decode_images', 'decode_masks', 'erase_codebook_face', 'forward', 'generate_images', 'get_codebook_emb',
                  'get_image_tokens', 'get_special_token', 'mask_predict', 'random_erase_codebook', 'recon_images',
                  'swap_one_frame_along_batch', 'transformer_forward'],
           DALLE: ['erase_codebook_face', 'forward', 'generate_images', 'get_image_tokens', 'random_erase_codebook', 'recon_images'],
           VQGanVAE1024: ['decode', 'decode_train', 'forward', 'get_codebook_indices']}
    for cls, names in ref.items():
        missing = [n for n in names if not callable(getattr(cls, n, None))]
        assert not missing, (cls.__name__, missing)
    m = tiny_bert(0, False)
    for b in (4, 5):
        x = torch.arange(b * 6 * 2.).view(b, 6, 2)
        torch.manual_seed(b)
        y = m.swap_one_frame_along_batch(x, t=3).view(b, 3, 2, 2)
        torch.manual_seed(b)
        idx = torch.randint(0, 3, (b, ))  # the helper's only draw
        xv = x.view(b, 3, 2, 2)
        partner = torch.cat(torch.chunk(torch.arange(b), 2, dim=0)[::-1], dim=0)  # the reference's half swap of the batch
        for i in range(b):
            for t in range(3):  # slot idx[i] receives the partner's picked frame, every other slot is untouched
                want = xv[partner[i], idx[partner[i]]] if t == idx[i] else xv[i, t]
                assert torch.equal(y[i, t], want), (b, i, t)


def test_half_keeps_fp32_master_weights():
    """train.py:194-195 calls `.half()` under --fp16.  Compute here is always bf16 MFMA over fp32 master weights; `.half()`
    must not strand the kernels with fp16 parameters: it warns and leaves the module as it is."""
    m = tiny_bert()
    with pytest.warns(UserWarning, match='fp32 master'):
        out = m.half()
    assert out is m and all(p.dtype == torch.float32 for p in m.parameters())
    # an fp16 checkpoint (what a --fp16 run of the reference saves) still loads: values are widened on copy
    sd = {k: (v.half() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected and m.text_emb.weight.dtype == torch.float32


def test_library_exports_every_declared_symbol():
    from mmvid_amd import _lib
    from mmvid_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    declared = set(re.findall(r'\b(mmvid_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'mmvid_tower_layer_t', 'mmvid_tower_cfg_t'}
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/mmvid_hip.h but not exported'
    assert set(_lib.SIGNATURES) | set(_lib.OTHER) == declared
    assert lib.mmvid_abi_version() == _lib.ABI_VERSION == 3
    assert ctypes.sizeof(_lib.TowerLayer) == 24 * 8 and ctypes.sizeof(_lib.TowerCfg) == 12 * 4


def test_no_cpu_fallback():
    """Host tensors must be refused loudly: the kernels are the only implementation."""
    from mmvid_amd import ops
    from mmvid_amd._lib import MMVIDError
    with pytest.raises(MMVIDError):
        ops.vq_argmin(torch.zeros(4, 256), torch.zeros(32, 256))
    with pytest.raises(MMVIDError):
        ops.layernorm_fwd(torch.zeros(4, 768), torch.ones(768), torch.zeros(768))
    m = tiny_bert()
    with pytest.raises(MMVIDError):
        m(torch.ones(2, 16, dtype=torch.long), return_loss=False)
    # the product package never imports the oracle
    import subprocess
    out = subprocess.run(['grep', '-rlE', r'^\s*(from|import)\s+oracle', os.path.join(ROOT, 'mmvid_amd')], capture_output=True, text=True)
    assert out.stdout.strip() == ''


def test_checkpoint_wire_formats_round_trip(tmp_path):
    """SURVEY next-row N3: the reference's files load unchanged.  `dalle.pt` is a dict {'iter', 'hparams', 'vae_params',
    'weights', 'optimizer'} whose 'weights' is the module state_dict (train.py:341-354, loaded with strict=False at
    test.py:134-150); a VQGAN `.ckpt` is {'state_dict': ...} loaded with strict=False (vae.py:28-30)."""
    from mmvid_amd.vae import VQGanVAE1024
    torch.manual_seed(0)
    a = tiny_bert()
    opt = torch.optim.Adam([p for p in a.parameters() if p.requires_grad], lr=1e-4)
    path = tmp_path / 'dalle.pt'
    torch.save({'iter': 7, 'hparams': {'dim': 768, 'num_targets': 2}, 'vae_params': None, 'weights': a.state_dict(),
                'optimizer': opt.state_dict()}, path)
    torch.manual_seed(1)
    b = tiny_bert()
    ckpt = torch.load(str(path), weights_only=False)
    missing, unexpected = b.load_state_dict(ckpt['weights'], strict=False)
    assert not missing and not unexpected and ckpt['iter'] == 7
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    vpath = tmp_path / 'vae.ckpt'
    torch.save({'state_dict': a.vae.model.state_dict(), 'global_step': 3}, vpath)
    v = VQGanVAE1024(str(vpath), 64, ddconfig={'ch': 32}, n_embed=256)
    for (ka, va), (kb, vb) in zip(a.vae.model.state_dict().items(), v.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_library_host_side_policies():
    """Entry points that need no GPU: the dW split-K policy and the tuning-knob table."""
    from mmvid_amd import _lib
    lib = _lib.load()
    # one wave of 256x128 blocks on 256 CUs, at least 6 K tiles per split, at most 16 splits
    assert lib.mmvid_gemm_dw_pick_splitk(10422, 2304, 768) == 4    # 54 tiles
    assert lib.mmvid_gemm_dw_pick_splitk(10422, 768, 768) == 14    # 18 tiles
    assert lib.mmvid_gemm_dw_pick_splitk(10422, 3072, 768) == 3    # 72 tiles
    assert lib.mmvid_gemm_dw_pick_splitk(100, 768, 768) == 1       # too few tokens to split
    assert lib.mmvid_gemm_dw_pick_splitk(10 ** 6, 8192, 8192) == 1  # already more tiles than CUs
    # grouped weight gradients: output tiles over whole rounds of the 256 CUs; the tower groups them at >= 0.7
    from mmvid_amd import ops
    four = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]  # c_proj, c_fc, out_proj, in_proj of ViT-B/32
    assert abs(ops.gemm_dw_multi_fill(four, 12) - 2592 / (11 * 256)) < 1e-12   # the training step: 10.1 -> 11 rounds
    assert abs(ops.gemm_dw_multi_fill(four, 3) - 648 / (3 * 256)) < 1e-12     # chunks of 3 layers (multi-GPU engine)
    assert abs(ops.gemm_dw_multi_fill([(768, 768)], 12) - 216 / 256) < 1e-12
    assert ops.gemm_dw_multi_fill([(768, 768)], 3) < 0.7 and ops.gemm_dw_multi_fill([(512, 512)], 2) < 0.7
    _lib.call('mmvid_set_option', b'graphs', 0)
    with pytest.raises(_lib.MMVIDError, match='unknown option'):
        _lib.call('mmvid_set_option', b'no_such_knob', 1)


def test_vqgan_plan_structure_config2(monkeypatch):
    """The planned op list of one full-size encode (what mmvid_vqgan_run executes): 39 convolutions (45 in the reference's
    graph; the q, k, v 1x1 convs of each of the 3 AttnBlocks are one launch with stacked weights), no cast passes
    (convs store the precisions their consumers read), GroupNorm statistics fused into the producing conv wherever
    the geometry allows, and a matching stats area on both sides of every fused pair."""
    from mmvid_amd import vae as V, vqgan_plan as P
    v = V.VQGanVAE1024(None, 128)
    v.image_size = 128
    monkeypatch.setattr(v, '_ee', lambda: torch.zeros(1024))  # the codebook norms are a device kernel; not needed here
    pl = P.Bf16Planner(v)
    P.plan_encode(pl, v.model, 4, 128)
    ops_ = pl.ops
    kinds = [o.op for o in ops_]
    assert kinds.count(pl.OP_CONV) == 39 and kinds.count(pl.OP_CAST) == 0
    attn = [o for o in ops_ if o.op == pl.OP_ATTN]
    for o in attn:  # q | k | v are column blocks of one [n, hw, 3C] buffer: byte offsets 2C apart, row stride 3C
        assert o.pad == 3 * o.C and o.in1 - o.in0 == 2 * o.C and o.in2 - o.in1 == 2 * o.C
    qkv = [o for o in ops_ if o.op == pl.OP_CONV and o.mode == 3 and o.Cout == 3 * o.C]
    assert len(qkv) == 3 and {o.out_bf16 for o in qkv} == {o.in0 for o in attn}
    assert kinds.count(pl.OP_GN) == 28 and kinds.count(pl.OP_ATTN) == 3 and kinds[-1] == pl.OP_VQ
    fused_gn = [o for o in ops_ if o.op == pl.OP_GN and o.flags & P.STATS_GIVEN]
    emitting = [o for o in ops_ if o.op == pl.OP_CONV and o.flags & P.EMIT_STATS]
    # every level but 8x8 (64 pixels) fuses: 128^2, 64^2, 32^2, 16^2 have hw % 128 == 0 and >= 128 channels
    assert len(fused_gn) == sum(1 for o in ops_ if o.op == pl.OP_GN and (o.H * o.W) % 128 == 0 and o.C % 128 == 0)
    assert len(fused_gn) >= 18 and {o.scratch for o in fused_gn} <= {o.scratch for o in emitting}
    for o in ops_:
        if o.op == pl.OP_CONV:
            assert o.out_bf16 >= 0 or o.out_f32 >= 0
            assert max(o.in0, o.in1, o.out_bf16, o.out_f32, o.scratch) < pl.top
    # dual stores only where a 1x1 shortcut reads the stream in bf16 as well (the two channel-widening blocks)
    both = [o for o in ops_ if o.op == pl.OP_CONV and o.out_bf16 >= 0 and o.out_f32 >= 0]
    assert len(both) == 2


def test_vqgan_plan_structure_split_mode(monkeypatch):
    """vae.strict = 'split': every convolution is the pair operator (flag SPLIT) on pair planes and writes fp32; GroupNorm and the
    image layout write planes; attention is the fp32 operator; no bf16-operator op is left in the plan."""
    from mmvid_amd import vae as V, vqgan_plan as P
    v = V.VQGanVAE1024(None, 128)
    v.image_size, v.strict = 128, 'split'
    monkeypatch.setattr(v, '_ee', lambda: torch.zeros(1024))
    pl = P.PairPlanner(v)
    assert pl.split and not pl.strict
    P.plan_encode(pl, v.model, 4, 128)
    ops_ = pl.ops
    convs = [o for o in ops_ if o.op == pl.OP_CONV]
    assert len(convs) == 45 and all(o.flags & pl.SPLIT for o in convs)
    # every convolution writes fp32, except the last one of levels 0-2 (strip form, read only by the level's Downsample convolution): it
    # stores the bf16 pair itself -- no fp32 store, no cast pass in front of the Downsample
    planes_only = [o for o in convs if o.out_f32 < 0]
    assert len(planes_only) == 3 and all(o.out_bf16 >= 0 and o.flags & P.STRIP and o.in1 >= 0 for o in planes_only)
    assert all(o.out_bf16 < 0 for o in convs if o.out_f32 >= 0)
    assert sum(1 for o in ops_ if o.op == pl.OP_CAST) == 7     # fp32 -> pair planes in front of the remaining non-GroupNorm readers
    assert sum(1 for o in convs if o.flags & P.STRIP) == 12    # the strip form at 32x32 and above
    assert sum(1 for o in convs if o.flags & P.SPLITK) >= 4    # split-K on the 8x8 layers
    assert all(o.flags & pl.SPLIT for o in ops_ if o.op in (pl.OP_GN, pl.OP_CAST, pl.OP_IMG))
    assert all(o.flags & pl.STRICT for o in ops_ if o.op == pl.OP_ATTN)
    w3, b, cout = v._cw(v.model.encoder.conv_in, 'pair')
    assert w3.shape == (128, 3, 9, 8) and w3.dtype == torch.bfloat16 and cout == 128
    w = v.model.encoder.conv_in.weight.detach().permute(0, 2, 3, 1).reshape(128, 9, 3)
    assert torch.equal(w3[:, 0], w3[:, 1]) and (w3[:, 0, :, :3].float() + w3[:, 2, :, :3].float() - w).abs().max() < 2.0**-16
    for o in ops_:
        assert max(o.in0, o.in1, o.in2, o.out_bf16, o.out_f32, o.scratch) < pl.top


def test_vqgan_plan_structure_mixed_mode(monkeypatch):
    """vae.strict = 'mixed': the plan of 'split' with the F16 flag on exactly the 3x3 residual-block convolutions of the 128x128,
    64x64 and 32x32 levels and on the GroupNorms that feed them -- 12 of the encoder's 45 convolutions, 82 % of its multiply-adds; the
    decoder's plan is the pair operator's."""
    from mmvid_amd import vae as V, vqgan_plan as P
    v = V.VQGanVAE1024(None, 128)
    v.image_size, v.strict = 128, 'mixed'
    monkeypatch.setattr(v, '_ee', lambda: torch.zeros(1024))
    pl = P.PairPlanner(v, f16_side=v.mixed_f16_side)
    P.plan_encode(pl, v.model, 4, 128)
    convs = [o for o in pl.ops if o.op == pl.OP_CONV]
    f16 = [o for o in convs if o.flags & pl.F16]
    assert len(convs) == 45 and len(f16) == 12 and all(o.flags & pl.SPLIT and o.flags & P.STRIP and o.H >= 32 and o.C in (128, 256) for o in f16)
    gns = [o for o in pl.ops if o.op == pl.OP_GN and o.flags & pl.F16]
    assert len(gns) == 12 and {o.out_bf16 for o in gns} == {o.in0 for o in f16}  # each reads the plane its GroupNorm wrote

    def work(o):
        return o.N * (o.H // (2 if o.mode == 1 else 1))**2 * o.Cout * o.C * (9 if o.mode in (0, 1, 2) else 1)
    assert 0.81 < sum(work(o) for o in f16) / sum(work(o) for o in convs) < 0.84
    w16, b, cout = v._cw(v.model.encoder.down[0].block[0].conv1, 'f16')
    assert w16.shape == (128, 9, 128) and w16.dtype == torch.float16 and cout == 128
    pd = P.PairPlanner(v, f16_side=0)
    P.plan_decode(pd, v.model, 2, 8)
    assert not any(o.flags & pd.F16 for o in pd.ops)


def test_vqgan_weight_layouts_equal_the_plain_expression():
    """The four encodings of a conv holder's weights (vae._cw) are permute to [Cout][ky*kx][Cin], zero-pad, cast -- for a 3x3 and a
    1x1 layer, conv_in (Cin = 3) and the decoder's conv_out (Cout = 3); the stacked q | k | v weights are their concatenation."""
    import torch.nn.functional as F
    from mmvid_amd import vae as V
    torch.manual_seed(0)
    v = V.VQGanVAE1024(None, 128)
    enc = v.model.encoder
    blk = enc.down[2].block[0]  # 128 -> 256 channels: conv1 3x3, nin_shortcut 1x1
    # holder, (Cin_p, Cout_p) of the bf16 / pair / fp16 forms, (Cin_p, Cout_p) of the fp32 form
    for h, (cin_p, cout_p), (cin_p32, cout_p32) in ((blk.conv1, (128, 256), (128, 256)), (blk.nin_shortcut, (128, 256), (128, 256)),
                                                    (enc.conv_in, (8, 128), (4, 128)), (v.model.decoder.conv_out, (128, 8), (128, 3))):
        w, bias = h.weight.detach(), h.bias.detach()
        cout, cin, kh, kw = w.shape

        def plain(ci, co):
            return (F.pad(w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin), (0, ci - cin, 0, 0, 0, co - cout)), F.pad(bias, (0, co - cout)))
        wp, bp = plain(cin_p, cout_p)
        hi = wp.to(torch.bfloat16)
        want = {'bf16': hi, 'f16': wp.to(torch.float16), 'pair': torch.stack([hi, hi, (wp - hi.float()).to(torch.bfloat16)], 1)}
        for form, ww in want.items():
            got_w, got_b, got_cout = v._cw(h, form)
            assert got_w.dtype == ww.dtype and got_w.is_contiguous() and torch.equal(got_w, ww), (form, tuple(w.shape))
            assert got_b.dtype == torch.float32 and torch.equal(got_b, bp) and got_cout == cout
        wp32, bp32 = plain(cin_p32, cout_p32)
        got_w, got_b, got_cout = v._cw(h, 'f32')
        assert got_w.dtype == torch.float32 and got_w.is_contiguous() and torch.equal(got_w, wp32)
        assert torch.equal(got_b, bp32) and got_cout == cout
        assert v._cw(h)[0] is v._cw(h, 'bf16')[0] and v._cw(h, 'pair')[0] is v._cw(h, 'pair')[0]  # cached, per form
    a = enc.mid.attn_1
    wq, bq = v._cw_qkv(a)
    assert torch.equal(wq, torch.cat([v._cw(x)[0] for x in (a.q, a.k, a.v)])) and wq.shape == (1536, 1, 512)
    assert torch.equal(bq, torch.cat([x.bias.detach() for x in (a.q, a.k, a.v)]))
