"""mmvid_amd.clip_model on the host: the CLIP state_dict layout against the reference's (tests/golden/clip_vit2.npz, written by
tools/make_golden.py::case_clip_vit2 from mmvid_pytorch/transformers/clip_model.py:298-348), loading an OpenAI-style TorchScript
archive (clip_model.py:438-497), and the guards of the inference-only surface.  No GPU: every check here fails before a kernel."""
import pytest
import torch
from torch import nn


def vit(layers=2):
    from mmvid_amd.clip_model import CLIP
    return CLIP(512, 224, layers, 768, 32, 77, 49408, 512, 8, layers)


def test_clip_state_dict_manifest_matches_reference(golden):
    g = golden('clip_vit2')
    m = vit(2)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == g.manifest
    for k in ('input_resolution', 'context_length', 'vocab_size'):  # non-persistent 0-d buffers, as the TorchScript model carries them
        assert k not in m.state_dict() and getattr(m, k).dtype == torch.int64 and getattr(m, k).dim() == 0
    assert (m.input_resolution.item(), m.context_length.item(), m.vocab_size.item()) == (224, 77, 49408)
    assert m.dtype == torch.float32


class _Node(nn.Module):
    """A scriptable tree of parameters (identity forward) with the key layout of a given state_dict."""

    def __init__(self, tensors):
        super().__init__()
        kids = {}
        for k, v in tensors.items():
            head, _, rest = k.partition('.')
            if rest:
                kids.setdefault(head, {})[rest] = v
            else:
                self.register_parameter(head, nn.Parameter(v, requires_grad=False))
        for name, sub in kids.items():
            self.add_module(name, _Node(sub))

    def forward(self, x):
        return x


def test_clip_torchscript_archive_loads(tmp_path):
    """A scripted stand-in ViT-B-32.pt (2 layers, fp16 storage, the real key layout, and the archive's input_resolution /
    context_length / vocab_size attributes) comes back through load() as fp32 parameters, frozen, in eval mode."""
    from mmvid_amd import clip_model

    torch.manual_seed(0)
    src = {k: (torch.randn(v.shape) * 0.02).half() for k, v in vit(2).state_dict().items()}
    arch = _Node(src)
    for k, v in (('input_resolution', 224), ('context_length', 77), ('vocab_size', 49408)):
        arch.register_buffer(k, torch.tensor(v))
    path = str(tmp_path / 'ViT-B-32.pt')
    torch.jit.script(arch).save(path)
    m = clip_model.load(path, device='cpu')
    assert isinstance(m, clip_model.CLIP) and not m.training
    assert m.input_resolution.item() == 224 and m.context_length.item() == 77 and m.vocab_size.item() == 49408
    got = m.state_dict()
    assert set(got) == set(src)
    for k, v in got.items():
        assert v.dtype == torch.float32 and torch.equal(v, src[k].float()), k
    assert not any(p.requires_grad for p in m.parameters())
    # the towers' runners see the loaded weights (they hold the same parameter objects)
    assert m.visual.tower.transformer.resblocks[1].mlp.c_fc.weight is m.visual.transformer.resblocks[1].mlp.c_fc.weight
    assert torch.equal(m.text_tower.transformer.resblocks[0].attn.in_proj_weight, src['transformer.resblocks.0.attn.in_proj_weight'].float())


def test_clip_helpers_reject_foreign_models():
    from mmvid_amd import clip_model

    class Stock(nn.Module):
        input_resolution = torch.tensor(224)

    frames = torch.rand(2, 3, 64, 64)
    with pytest.raises(TypeError):
        clip_model.clip_similarity(Stock(), None, frames, ['a person is talking'])
    with pytest.raises(TypeError):
        clip_model.clip_encode_image(Stock(), frames)
    with pytest.raises(TypeError):
        clip_model.clip_score(Stock(), None, frames[None], ['a person is talking'])


def test_clip_is_inference_only():
    """With grad enabled, an input or a parameter that requires grad is an error (not a silently detached result)."""
    from mmvid_amd import clip_model
    m = vit(2)
    img = torch.zeros(1, 3, 224, 224)
    text = torch.zeros(1, 77, dtype=torch.long)
    with pytest.raises(RuntimeError, match='inference only'):
        m.encode_image(img)  # trainable parameters
    with pytest.raises(RuntimeError, match='inference only'):
        m(img, text)
    m.requires_grad_(False)
    with pytest.raises(RuntimeError, match='inference only'):
        m.encode_image(img.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='inference only'):
        clip_model.clip_encode_image(m, torch.rand(1, 3, 64, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match='inference only'):
        clip_model.clip_score(m, None, torch.rand(1, 2, 3, 64, 64, requires_grad=True), ['x'])


def test_clip_resnet_configuration_not_implemented():
    from mmvid_amd.clip_model import CLIP, build_model
    with pytest.raises(NotImplementedError, match='ModifiedResNet'):
        CLIP(1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12)
    with pytest.raises(NotImplementedError, match='ModifiedResNet'):
        build_model({'visual.layer1.0.conv1.weight': torch.zeros(64, 64, 1, 1)})
