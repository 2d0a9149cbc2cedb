"""BERT and ART-V on the tower a CLIP checkpoint holds (clip_model.py:535-543 builds whatever the archive carries): the shape is
read from the archive, `dim` is checked against it, and what the kernels do not take is refused at construction with the limit in the
message.  Scripted stand-in archives with the key layout and fp16 storage of OpenAI's files (as tests/test_host_logic.py writes
one); the reference's state_dict manifests at dim 1024 are tests/golden/wide_models.npz (tools/make_golden.py::case_wide_models)."""
import pytest
import torch
from torch import nn

from test_host_logic import manifest, tiny_vae


def _tower(width, layers):
    class Blk(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = nn.MultiheadAttention(width, width // 64 if width % 64 == 0 else 8)
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

    return Tower()


def write_archive(path, visual=(1024, 2), text=(768, 3), seed=0):
    """A TorchScript archive with `visual.transformer.resblocks.*` (None: a ResNet-style archive, `visual.layer1.*` only) and
    `transformer.resblocks.*`, stored in fp16.  Returns its state dict."""
    torch.manual_seed(seed)

    class Visual(nn.Module):
        def __init__(self):
            super().__init__()
            if visual is None:
                self.layer1 = nn.Linear(8, 8)
            else:
                self.transformer = _tower(*visual)

        def forward(self, x):
            return x

    class Archive(nn.Module):
        def __init__(self):
            super().__init__()
            self.visual = Visual()
            self.transformer = _tower(*text)

        def forward(self, x):
            return self.visual(x)

    arch = Archive().half()
    torch.jit.script(arch).save(str(path))
    return arch.state_dict()


@pytest.fixture(scope='module')
def vitl(tmp_path_factory):
    path = tmp_path_factory.mktemp('clip') / 'ViT-L-14.pt'
    return str(path), write_archive(path)


@pytest.mark.parametrize('which,shape,prefix', [('openai_clip_visual', (1024, 2, 16), 'visual.transformer.'),
                                                ('openai_clip_text', (768, 3, 12), 'transformer.')])
def test_tower_shape_comes_from_the_archive(vitl, which, shape, prefix):
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    path, src = vitl
    tw = OpenAICLIPTransformer(51, which, model_path=path, causal=True, mask_type='mask_prev', mask_kwargs={'index': [17, 18]})
    assert (tw.width, tw.layers, tw.heads) == shape
    sd = tw.transformer.state_dict()
    assert len(sd) == 12 * shape[1]
    for k, v in sd.items():
        assert v.dtype == torch.float32 and torch.equal(v, src[prefix + k].float()), k


def test_explicit_layers_keep_the_first_blocks(vitl):
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    path, src = vitl
    tw = OpenAICLIPTransformer(51, 'openai_clip_text', model_path=path, layers=2)
    assert (tw.width, tw.layers, tw.heads) == (768, 2, 12)
    for k, v in tw.transformer.state_dict().items():
        assert torch.equal(v, src['transformer.' + k].float()), k
    with pytest.raises(ValueError, match=r'layers=4.*has 3'):
        OpenAICLIPTransformer(51, 'openai_clip_text', model_path=path, layers=4)


def _bert(**kw):
    from mmvid_amd.dalle_bert import BERT
    return BERT(vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual', num_visuals=0,
                num_targets=2, **kw)


def _artv(**kw):
    from mmvid_amd.dalle_artv import DALLE
    return DALLE(vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual', num_visuals=1,
                 num_targets=2, **kw)


@pytest.mark.parametrize('build,key', [(_bert, 'manifest'), (_artv, 'manifest_artv')])
def test_models_on_a_vitl14_checkpoint_have_the_reference_layout(golden, vitl, build, key):
    """dim = 1024 with the archive's visual tower: the reference's state_dict keys and shapes at the same settings, and the tower's
    weights are the archive's."""
    path, src = vitl
    g = golden('wide_models')
    m = build(dim=1024, openai_clip_path=path)
    assert (m.transformer.width, m.transformer.layers, m.transformer.heads) == (g.meta['dim'], g.meta['layers'], g.meta['heads'])
    assert manifest(m) == [(k, tuple(s)) for k, s in g.json(key)]
    k = 'transformer.resblocks.1.mlp.c_proj.weight'
    assert torch.equal(m.transformer.state_dict()[k], src['visual.' + k].float())


@pytest.mark.parametrize('build,key', [(_bert, 'manifest'), (_artv, 'manifest_artv')])
def test_transformer_width_builds_the_same_layout_without_a_checkpoint(golden, build, key):
    g = golden('wide_models')
    m = build(dim=1024, transformer_width=1024, transformer_layers=2)
    assert (m.transformer.width, m.transformer.layers, m.transformer.heads) == (1024, 2, 16)
    assert manifest(m) == [(k, tuple(s)) for k, s in g.json(key)]


@pytest.mark.parametrize('build', [_bert, _artv])
def test_refusals_name_the_limit(vitl, tmp_path, build):
    path, _ = vitl
    with pytest.raises(ValueError, match=r'dim=768.*1024'):  # both numbers
        build(dim=768, openai_clip_path=path)
    with pytest.raises(ValueError, match=r'dim=768.*1024'):
        build(dim=768, transformer_width=1024, transformer_layers=2)
    with pytest.raises(ValueError, match=r'1280.*above 1024'):
        build(dim=1280, transformer_width=1280, transformer_layers=2)
    with pytest.raises(ValueError, match=r'1000.*multiple of 64'):
        build(dim=1000, transformer_width=1000, transformer_layers=2)
    wide = tmp_path / 'ViT-H-14.pt'
    write_archive(wide, visual=(1280, 1), text=(64, 1))
    with pytest.raises(ValueError, match=r'1280.*above 1024'):
        build(dim=1280, openai_clip_path=str(wide))
    odd = tmp_path / 'odd.pt'
    write_archive(odd, visual=(1000, 1), text=(64, 1))
    with pytest.raises(ValueError, match=r'1000.*multiple of 64'):
        build(dim=1000, openai_clip_path=str(odd))
    rn = tmp_path / 'RN50.pt'
    write_archive(rn, visual=None, text=(64, 1))
    with pytest.raises(ValueError, match=r'no visual\.transformer\.resblocks.*openai_clip_visual'):
        build(dim=1024, openai_clip_path=str(rn))


def test_the_default_table_is_what_it_was():
    """No checkpoint and no transformer_width: the ViT-B/32 table, whatever `dim` says (today's behaviour)."""
    from mmvid_amd.clip_tower import TOWER_SHAPES, OpenAICLIPTransformer
    assert TOWER_SHAPES == {'openai_clip_visual': (768, 12, 12), 'openai_clip_text': (512, 12, 8)}
    m = _bert(dim=768, transformer_layers=2)
    assert (m.transformer.width, m.transformer.layers, m.transformer.heads) == (768, 2, 12)
    t = OpenAICLIPTransformer(8, 'openai_clip_text', layers=1)
    assert (t.width, t.layers, t.heads) == (512, 1, 8)


def test_decode_sessions_of_width_1024_take_the_fused_step(monkeypatch):
    """DecodeSession._enqueue: width 1024 goes through mmvid_tower_decode_fused_slice in slices of 64 sequences (the last one advances
    the position), as widths 512 and 768 do; other widths keep the GEMM-based step."""
    from mmvid_amd import _lib, clip_tower
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name, a)))

    class T:
        shape = (70, 1024)

        def __getitem__(self, i):
            return self

        def data_ptr(self):
            return 0

    class C(T):
        shape = (2, 70, 32, 2048)

    class Tw:
        def _cfg(self, B, L):
            return _lib.TowerCfg(B=B, L=L)

    s = object.__new__(clip_tower.DecodeSession)
    s.persistent, s.fused, s.x, s.y, s.cache, s.pos, s.scratch = False, True, T(), T(), C(), T(), T()
    s.cfg, s._slice_cfgs, s.layers, s.tower = _lib.TowerCfg(B=70, L=32), {}, None, Tw()
    monkeypatch.setattr(clip_tower.ops, '_p', lambda t: 0)
    monkeypatch.setattr(clip_tower.ops, '_stream', lambda: 0)
    s._enqueue()
    assert [c[0] for c in calls] == ['mmvid_tower_decode_fused_slice'] * 2
    assert [(c[1][0]._obj.B, c[1][9]) for c in calls] == [(64, 0), (6, 1)]  # (slice batch, advance_pos)


def test_captured_and_deterministic_trainer_steps_are_refused_above_width_768():
    """engine.GraphedStep and a deterministic-mode FlatTrainer.step on a tower wider than 768: refused with the limit and the reason in the
    message (the one run of that combination at width 1024 ended in a GPU memory-access fault of unknown cause); width 768 passes the gate."""
    import types

    from mmvid_amd import engine
    wide = types.SimpleNamespace(transformer=types.SimpleNamespace(width=1024))
    for what in ('a captured trainer step (GraphedStep)', 'a deterministic-mode trainer step'):
        with pytest.raises(NotImplementedError, match=r'1024 wide.*above width 768.*fault'):
            engine.refuse_unproven_width(wide, what)
    with pytest.raises(NotImplementedError, match=r'GraphedStep.*1024 wide'):
        engine.GraphedStep(types.SimpleNamespace(model=wide), lambda: None, {})
    engine.refuse_unproven_width(types.SimpleNamespace(transformer=types.SimpleNamespace(width=768)), 'x')
    engine.refuse_unproven_width(types.SimpleNamespace(), 'x')  # (a model without a tower)
    import inspect
    assert 'refuse_unproven_width' in inspect.getsource(engine.FlatTrainer.step)
