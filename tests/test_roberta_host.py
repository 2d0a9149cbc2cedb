"""mmvid_amd.roberta on the host: the byte-level BPE tokenizer against transformers' RobertaTokenizer (tests/golden/roberta_bpe +
roberta_tokenizer.npz, tools/make_golden.py::case_roberta_tokenizer), the RobertaModel state_dict layout against transformers'
(roberta_tiny.npz), checkpoint loading and the guards of the local-only, inference-only surface.  No GPU: nothing here reaches a kernel."""
import json
import os
import types

import pytest
import torch

from conftest import GOLDEN

BPE = os.path.join(GOLDEN, 'roberta_bpe')


def tiny_config(g):
    from mmvid_amd.roberta import RobertaConfig
    return RobertaConfig(**g.meta['config'])


@pytest.mark.parametrize('full', [False, True])
def test_tokenizer_matches_transformers(golden, full):
    from mmvid_amd.roberta import RobertaTokenizer
    g = golden('roberta_tokenizer')
    tok = RobertaTokenizer.from_pretrained(BPE)
    sfx = '_full' if full else ''
    kw = {} if full else dict(max_length=g.meta['max_length'])
    enc = tok(g.meta['sentences'], return_tensors='pt', padding=True, truncation=True, **kw)
    assert enc['input_ids'].dtype == torch.int64 and enc['attention_mask'].dtype == torch.int64
    assert torch.equal(enc['input_ids'], g['input_ids' + sfx])
    assert torch.equal(enc['attention_mask'], g['attention_mask' + sfx])


def test_tokenizer_truncation_keeps_eos_and_pads_right(golden):
    from mmvid_amd.roberta import RobertaTokenizer
    tok = RobertaTokenizer.from_pretrained(BPE)
    enc = tok(['', 'a person is talking ' * 20], max_length=10)
    ids, mask = enc['input_ids'], enc['attention_mask']
    assert ids.shape == (2, 10)
    assert ids[0, :2].tolist() == [0, 2] and (ids[0, 2:] == 1).all() and mask[0].tolist() == [1, 1] + [0] * 8
    assert ids[1, 0] == 0 and ids[1, -1] == 2 and mask[1].all()


def test_model_state_dict_manifest_matches_transformers(golden):
    from mmvid_amd.roberta import RobertaModel
    for name in ('roberta_tiny', 'roberta_large24'):
        g = golden(name)
        m = RobertaModel(tiny_config(g)) if name == 'roberta_tiny' else None
        if m is None:  # (the 24-layer model's manifest without allocating its 355 M parameters)
            with torch.device('meta'):
                m = RobertaModel(tiny_config(g))
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == g.manifest, name


def _write_checkpoint(tmp_path, g, sd, fmt):
    cfg = dict(g.meta['config'], architectures=['RobertaForMaskedLM'], model_type='roberta')
    (tmp_path / 'config.json').write_text(json.dumps(cfg))
    if fmt == 'safetensors':
        from safetensors.torch import save_file
        save_file(sd, str(tmp_path / 'model.safetensors'))
    else:
        torch.save(sd, str(tmp_path / 'pytorch_model.bin'))


@pytest.mark.parametrize('fmt', ['safetensors', 'bin'])
def test_loader_strips_prefix_and_ignores_lm_head(golden, tmp_path, fmt):
    """A hub-style RobertaForMaskedLM checkpoint: `roberta.` keys, an lm_head, the legacy position_ids buffer, no pooler."""
    from mmvid_amd.roberta import RobertaModel
    from oracle.synth import synth_state_dict
    g = golden('roberta_tiny')
    ref = synth_state_dict(g.manifest, 5)
    E, V = g.meta['config']['hidden_size'], g.meta['config']['vocab_size']
    sd = {'roberta.' + k: v for k, v in ref.items() if not k.startswith('pooler.')}
    sd['roberta.embeddings.position_ids'] = torch.arange(514)[None]
    sd.update({'lm_head.dense.weight': torch.zeros(E, E), 'lm_head.dense.bias': torch.zeros(E), 'lm_head.bias': torch.zeros(V),
               'lm_head.layer_norm.weight': torch.ones(E), 'lm_head.layer_norm.bias': torch.zeros(E)})
    _write_checkpoint(tmp_path, g, sd, fmt)
    m = RobertaModel.from_pretrained(str(tmp_path))
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    got = m.state_dict()
    for k, v in ref.items():
        if not k.startswith('pooler.'):
            assert torch.equal(got[k], v), k
    assert not any(k.startswith('lm_head') for k in got)


def test_unsupported_configs_raise(golden):
    from mmvid_amd.roberta import RobertaConfig, RobertaModel
    base = golden('roberta_tiny').meta['config']
    with pytest.raises(NotImplementedError, match='hidden_act'):
        RobertaModel(RobertaConfig(**dict(base, hidden_act='gelu_new')))
    with pytest.raises(NotImplementedError, match='head'):
        RobertaModel(RobertaConfig(**dict(base, num_attention_heads=4)))  # head dimension 32
    m = RobertaModel(RobertaConfig(**dict(base, type_vocab_size=2))).requires_grad_(False)
    ids = torch.tensor([[0, 5, 2]])
    with pytest.raises(NotImplementedError, match='token_type_ids'):
        m(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.tensor([[0, 1, 1]]))


def test_model_is_inference_only(golden):
    from mmvid_amd.roberta import RobertaModel
    m = RobertaModel(tiny_config(golden('roberta_tiny')))
    ids = torch.tensor([[0, 5, 2]])
    with pytest.raises(RuntimeError, match='inference only'):
        m(input_ids=ids, attention_mask=torch.ones_like(ids))


def test_hub_names_raise_without_network(monkeypatch, tmp_path):
    """'roberta-large' without a local directory fails at once, naming the files it needs; no socket is ever opened."""
    import socket

    from mmvid_amd import roberta

    def no_net(*a, **k):
        raise AssertionError('network access attempted')

    monkeypatch.setattr(socket, 'socket', no_net)
    monkeypatch.setattr(socket, 'create_connection', no_net)
    monkeypatch.chdir(tmp_path)  # (no ./roberta-large directory either)
    for call in (lambda: roberta.RobertaTokenizer.from_pretrained('roberta-large'),
                 lambda: roberta.RobertaModel.from_pretrained('roberta-large'),
                 lambda: roberta.get_fixed_language_model(types.SimpleNamespace(fixed_language_model='roberta-large', text_seq_len=50))):
        with pytest.raises(FileNotFoundError, match='vocab.json|config.json'):
            call()
    with pytest.raises(NotImplementedError):
        roberta.get_fixed_language_model(types.SimpleNamespace(fixed_language_model='bert-base-uncased', text_seq_len=50))
