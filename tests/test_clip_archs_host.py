"""mmvid_amd.clip_model beyond ViT-B/32, on the host: the ViT-L/14 shape and a tiny patch-14 shape construct with the reference's
state_dict layout (tests/golden/clip_vitl14_2.npz, clip_p14_tiny.npz: tools/make_golden.py::_clip_case), build_model reads the
configuration of ViT-B/16, ViT-L/14 and ViT-L/14@336 state dicts, what is still refused, the frames-per-pass rule, and the C ABI
the feature had to fit into.  No GPU: every check here ends before a kernel."""
import pytest
import torch

L14_2 = (768, 224, 2, 1024, 14, 77, 49408, 768, 12, 2)
P14_TINY = (256, 56, 2, 256, 14, 77, 49408, 256, 4, 2)


@pytest.mark.parametrize('name,shape', [('clip_vitl14_2', L14_2), ('clip_p14_tiny', P14_TINY)])
def test_patch14_shapes_construct_with_the_reference_layout(golden, name, shape):
    from mmvid_amd.clip_model import CLIP
    g = golden(name)
    assert tuple(g.meta['shape']) == shape
    m = CLIP(*shape)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == g.manifest
    assert (m.input_resolution.item(), m.context_length.item(), m.vocab_size.item()) == (shape[1], 77, 49408)
    assert m._shape == dict(R=shape[1], P=14, L=77, V=49408, D=shape[0])
    assert (m.visual.tower.width, m.visual.tower.heads, m.visual.tower.layers) == (shape[3], shape[3] // 64, 2)
    assert (m.text_tower.width, m.text_tower.heads, m.text_tower.layers) == (shape[7], shape[8], 2)


def _vit_state_dict(embed, grid, vis_layers, vis_width, patch, ctx, vocab, txt_width, txt_layers):
    """Zero tensors under the keys and shapes of an OpenAI ViT CLIP checkpoint (clip_model.py:249-348), written out by hand."""
    def tower(prefix, width, layers):
        out = {}
        for i in range(layers):
            b = f'{prefix}resblocks.{i}.'
            out.update({b + 'attn.in_proj_weight': (3 * width, width), b + 'attn.in_proj_bias': (3 * width, ),
                        b + 'attn.out_proj.weight': (width, width), b + 'attn.out_proj.bias': (width, ),
                        b + 'ln_1.weight': (width, ), b + 'ln_1.bias': (width, ),
                        b + 'mlp.c_fc.weight': (4 * width, width), b + 'mlp.c_fc.bias': (4 * width, ),
                        b + 'mlp.c_proj.weight': (width, 4 * width), b + 'mlp.c_proj.bias': (width, ),
                        b + 'ln_2.weight': (width, ), b + 'ln_2.bias': (width, )})
        return out

    shapes = {'positional_embedding': (ctx, txt_width), 'text_projection': (txt_width, embed), 'logit_scale': (),
              'visual.class_embedding': (vis_width, ), 'visual.positional_embedding': (grid * grid + 1, vis_width),
              'visual.proj': (vis_width, embed), 'visual.conv1.weight': (vis_width, 3, patch, patch),
              'visual.ln_pre.weight': (vis_width, ), 'visual.ln_pre.bias': (vis_width, ),
              'visual.ln_post.weight': (vis_width, ), 'visual.ln_post.bias': (vis_width, ),
              'token_embedding.weight': (vocab, txt_width), 'ln_final.weight': (txt_width, ), 'ln_final.bias': (txt_width, )}
    shapes.update(tower('visual.transformer.', vis_width, vis_layers))
    shapes.update(tower('transformer.', txt_width, txt_layers))
    sd = {k: torch.zeros(s, dtype=torch.float16) for k, s in shapes.items()}
    sd.update(input_resolution=torch.tensor(grid * patch), context_length=torch.tensor(ctx), vocab_size=torch.tensor(vocab))
    return sd


@pytest.mark.parametrize('arch,grid,patch,vis,txt,embed', [
    ('ViT-B/16', 14, 16, (768, 12, 3), (512, 8, 2), 512),
    ('ViT-L/14', 16, 14, (1024, 16, 2), (768, 12, 3), 768),
    ('ViT-L/14@336', 24, 14, (1024, 16, 2), (768, 12, 1), 768),
])
def test_build_model_reads_the_checkpoint_shape(arch, grid, patch, vis, txt, embed):
    """Width, depth, patch and grid come from the state dict (clip_model.py:461-512); the resolution from the positional table
    (197, 257 and 577 rows).  Depths are cut (and differ between the towers) to keep the test quick; vocabulary 1000."""
    from mmvid_amd.clip_model import CLIP, build_model
    m = build_model(_vit_state_dict(embed, grid, vis[2], vis[0], patch, 77, 1000, txt[0], txt[2]))
    assert isinstance(m, CLIP) and not m.training and not any(p.requires_grad for p in m.parameters())
    assert m._shape == dict(R=grid * patch, P=patch, L=77, V=1000, D=embed)
    assert m.input_resolution.item() == grid * patch
    assert m.visual.positional_embedding.shape == (grid * grid + 1, vis[0])
    assert (m.visual.tower.width, m.visual.tower.heads, m.visual.tower.layers) == vis
    assert (m.text_tower.width, m.text_tower.heads, m.text_tower.layers) == txt
    assert m.visual.tower.mask_spec is None and m.text_tower.mask_spec == 'causal'
    assert all(p.dtype == torch.float32 for p in m.parameters())


def test_what_is_still_refused():
    from mmvid_amd.clip_model import CLIP
    with pytest.raises(NotImplementedError, match='ModifiedResNet'):
        CLIP(1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12)
    with pytest.raises(NotImplementedError, match='patch size 14 / resolution 230.*divides the resolution'):
        CLIP(768, 230, 2, 1024, 14, 77, 49408, 768, 12, 2)
    with pytest.raises(NotImplementedError, match='width 768 with 8 heads.*head dimension 64'):
        CLIP(768, 224, 2, 1024, 14, 77, 49408, 768, 8, 2)
    with pytest.raises(NotImplementedError, match='width 1000 with 15 heads.*head dimension 64'):
        CLIP(768, 224, 2, 1000, 14, 77, 49408, 768, 12, 2)  # a visual width that is not 64 x heads


def test_frames_per_pass_and_patch_columns():
    """The rows of a tower pass stay at ViT-B/32's 256 x 50; the patch matrix's row length is 3*P*P rounded up to 64."""
    from mmvid_amd import clip_model
    assert clip_model.IMAGE_SLICE == 256
    assert [clip_model.frames_per_pass(T) for T in (50, 197, 257, 577)] == [256, 64, 49, 22]
    assert clip_model.frames_per_pass(10**6) == 1
    assert all(clip_model.frames_per_pass(T) * T <= 256 * 50 for T in range(2, 600))
    assert [clip_model.patch_columns(P) for P in (32, 16, 8, 14, 7, 2, 1)] == [3072, 768, 192, 640, 192, 64, 64]


def test_the_abi_stands():
    """No new entry point, struct or version: the feature lives behind mmvid_clip_patchify's existing argument list."""
    import ctypes

    from mmvid_amd import _lib
    assert len(_lib.SIGNATURES) + len(_lib.OTHER) == 144
    assert _lib.ABI_VERSION == _lib.HEADER.constants['MMVID_ABI_VERSION'] == 3
    res, args = _lib.HEADER.functions['mmvid_clip_patchify']
    I, V = ctypes.c_int, ctypes.c_void_p
    assert res is I and args == [V, I, I, I, I, I, V, V]  # (frames, N, S, R, P, normalize, out_bf16, stream)
