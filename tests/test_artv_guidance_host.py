"""Classifier-free guidance for ART-V, host side: the two C-ABI entries are declared and bound and nothing else moved, the new kernels
add no atomic and restate no arithmetic of guided_logit, and every argument rule of DALLE.generate_images / DALLE.forward raises on a
CPU-resident model before anything reaches the device.  No GPU: nothing here launches a kernel."""
import os
import re

import pytest
import torch

from test_host_logic import tiny_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TT = 4, 16


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# --------------------------------------------------------------------------------------------------------------- declarations
def test_the_two_entries_are_declared_and_bound():
    from mmvid_amd import _lib
    hdr = read('include', 'mmvid_hip.h')
    assert re.search(r'\bint\s+mmvid_sample_race_guided_at\s*\(const float\* logits_c, const float\* logits_u, int64_t ld, const float\* scale_dev, '
                     r'int64_t rows_per_scale,\s*const float\* E, const int32_t\* step_dev, int step0, int64_t e_step_stride, float logit_div, '
                     r'int64_t R,\s*int V, int64_t tok_offset, int64_t\* tok, void\* stream\);', hdr)
    assert re.search(r'\bint\s+mmvid_decode_embed_record_groups\s*\(const int64_t\* tok, const float\* table, int64_t table_rows, '
                     r'const float\* pos_rows,\s*const int32_t\* pos_dev, int pos_off, int B, int groups, int E, float\* x, int64_t\* record,\s*'
                     r'int64_t record_ld, int record_pos0, void\* stream\);', hdr)
    for name in ('mmvid_sample_race_guided_at', 'mmvid_decode_embed_record_groups'):
        comment = hdr[:hdr.index(f'int {name}')].rsplit('/*', 1)[1]
        assert 'dalle_artv.py:274-281' in comment, name  # the reference lines it serves
    P, I, I64, F = _lib.P, _lib.I, _lib.I64, _lib.F
    assert _lib.SIGNATURES['mmvid_sample_race_guided_at'] == [P, P, I64, P, I64, P, P, I, I64, F, I64, I, I64, P, P]
    assert _lib.SIGNATURES['mmvid_decode_embed_record_groups'] == [P, P, I64, P, P, I, I, I, I, P, P, I64, I, P]
    # the groups entry is the record entry with `int groups` after B
    rec = _lib.SIGNATURES['mmvid_decode_embed_record']
    assert _lib.SIGNATURES['mmvid_decode_embed_record_groups'] == rec[:7] + [I] + rec[7:]


def test_symbols_were_only_added():
    from mmvid_amd import _lib
    hdr = read('include', 'mmvid_hip.h')
    declared = set(re.findall(r'\b(mmvid_[a-z0-9_]+)\s*\(', hdr)) - {'mmvid_tower_layer_t', 'mmvid_tower_cfg_t'}
    assert set(_lib.SIGNATURES) | set(_lib.OTHER) == declared
    assert _lib.ABI_VERSION == 3
    P, I, I64, F = _lib.P, _lib.I, _lib.I64, _lib.F
    assert _lib.SIGNATURES['mmvid_sample_race_at'] == [P, I64, P, P, I, I64, P, F, F, I64, I, I64, P, P, P]
    assert _lib.SIGNATURES['mmvid_sample_race_guided'] == [P, P, I64, P, I64, P, P, F, F, I64, I, I64, P, P, P]
    assert _lib.SIGNATURES['mmvid_decode_embed'] == [P, P, I64, P, P, I, I, I, P, P]
    assert _lib.SIGNATURES['mmvid_decode_embed_record'] == [P, P, I64, P, P, I, I, I, P, P, I64, I, P]


def test_the_new_kernels_use_no_atomics_and_the_draw_reuses_guided_logit():
    sample, decode = read('mmvid_amd', 'csrc', 'sample.hip'), read('mmvid_amd', 'csrc', 'decode.hip')
    row = re.search(r'void sample_race_guided_row_kernel\(.*?\n\}', sample, re.S).group(0)
    assert 'atomic' not in row
    assert row.count('guided_logit(') == 2  # both passes: the maximum and the keys
    assert 'fmaf' not in row and '_rn(' not in row  # no arithmetic of the guided value of its own
    assert len(re.findall(r'float guided_logit\(', sample)) == 1  # reused, not restated
    assert 'c0 += 256 * 8' in row and '__launch_bounds__(256) void sample_race_guided_row_kernel' in sample
    entry = re.search(r'extern "C" int mmvid_sample_race_guided_at\(.*?\n\}', sample, re.S).group(0)
    assert 'atomic' not in entry and 'sample_race_guided_row_kernel' in entry
    groups = re.search(r'void dec_embed_groups_kernel\(.*?\n\}', decode, re.S).group(0)
    assert 'atomic' not in groups
    entry = re.search(r'extern "C" int mmvid_decode_embed_record_groups\(.*?\n\}', decode, re.S).group(0)
    assert 'atomic' not in entry and 'dec_embed_groups_kernel' in entry
    # the two existing embed entries still launch the existing kernel
    old = re.search(r'extern "C" int mmvid_decode_embed_record\(.*?\n\}', decode, re.S).group(0)
    assert 'hipLaunchKernelGGL(dec_embed_kernel,' in old


# ------------------------------------------------------------------------------------------------------------ argument rules
@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(70)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).eval()
    gen = torch.Generator().manual_seed(71)
    return m, torch.randint(1, 49408, (B, TT), generator=gen), torch.randint(0, 256, (B, 16), generator=gen)


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library fails the test: the rules below come before device work."""
    from mmvid_amd import _lib

    def refuse(name, *args):
        raise AssertionError(f'{name} was called before the arguments were checked')
    monkeypatch.setattr(_lib, 'call', refuse)
    monkeypatch.setattr('mmvid_amd.ops.call', refuse)


STEPS = 32
BAD_SAMPLING = {
    'negative_text without a scale': (dict(negative_text=torch.ones(B, TT, dtype=torch.long)), 'negative_text without guidance_scale'),
    'a sequence scale': (dict(guidance_scale=[2.0] * STEPS), 'per-token schedule'),
    'a [steps, B] scale tensor': (dict(guidance_scale=torch.full((STEPS, B), 2.0)), 'per-token schedule'),
    'a [B + 1] scale tensor': (dict(guidance_scale=torch.full((B + 1, ), 2.0)), r'must be \[B\]'),
    'a non-finite scale': (dict(guidance_scale=float('inf')), 'finite'),
    'a non-finite scale in a tensor': (dict(guidance_scale=torch.tensor([1.0, float('nan'), 1.0, 1.0])), 'finite'),
    'an empty guidance_drop without negative_text': (dict(guidance_scale=2.0, guidance_drop=()), 'empty guidance_drop'),
    'an unknown drop': (dict(guidance_scale=2.0, guidance_drop=('audio', )), 'not among'),
    'negative_text of the wrong shape': (dict(guidance_scale=2.0, negative_text=torch.ones(B + 1, TT, dtype=torch.long)), 'negative_text'),
    'negative_text too short': (dict(guidance_scale=2.0, negative_text=torch.ones(B, TT - 1, dtype=torch.long)), 'negative_text'),
    'a filtering filter_thres with a scale': (dict(guidance_scale=2.0, filter_thres=0.999), 'top_k'),
}


@pytest.mark.parametrize('name', list(BAD_SAMPLING))
@pytest.mark.parametrize('use_cache', [True, False])
def test_generate_images_refuses_before_any_device_work(artv, no_device, name, use_cache):
    m, text, vis = artv
    kw, match = BAD_SAMPLING[name]
    with pytest.raises(ValueError, match=match):
        m.generate_images(text, visual=vis, use_cache=use_cache, **kw)


def test_the_filtering_threshold_is_the_one_that_removes_image_classes(artv):
    from mmvid_amd.artv_sampling import k_keep
    m = artv[0]
    assert m.target_seq_len == STEPS
    assert k_keep(0.999, m.total_tokens) < m.num_image_tokens <= k_keep(0.5, m.total_tokens)  # (the default keeps the block)
    assert m._guidance(B, None, ('text', 'visual'), None, 0.999) is None  # unguided: the filter is today's
    drop, scale = m._guidance(B, 2.0, 'text', None, 0.5)
    assert drop == ('text', ) and scale == 2.0
    per_video = torch.tensor([0.0, 1.0, 2.0, 3.0])
    assert torch.equal(m._guidance(B, per_video, ('visual', ), None, 0.5)[1], per_video)
    assert m._guidance(B, torch.tensor(1.5), (), torch.ones(B, TT, dtype=torch.long), 0.5)[0] == ()
    assert torch.equal(m._scale_vector(1.5, 3, 'cpu'), torch.full((3, ), 1.5))
    assert torch.equal(m._scale_vector(torch.tensor(1.5, dtype=torch.float64), 3, 'cpu'), torch.full((3, ), 1.5))


BAD_TRAINING = {
    'a probability above 1': (dict(return_loss=True, null_text_prob=1.5), 'null_text_prob'),
    'a negative probability': (dict(return_loss=True, null_visual_prob=-0.1), 'null_visual_prob'),
    'the drop without the loss': (dict(return_loss=False, null_text_prob=0.5), 'training forward'),
    'the visual drop without the loss': (dict(return_loss=False, null_visual_prob=0.5), 'training forward'),
    'injected decisions without the loss': (dict(return_loss=False, _null=torch.zeros(B, 2, dtype=torch.uint8)), 'training forward'),
}


@pytest.mark.parametrize('name', list(BAD_TRAINING))
def test_forward_refuses_before_any_device_work(artv, no_device, name):
    m, text, vis = artv
    kw, match = BAD_TRAINING[name]
    with pytest.raises(ValueError, match=match):
        m(text, visual=vis, target=torch.zeros(B, STEPS, dtype=torch.long), **kw)


def test_the_operators_refuse_host_tensors():
    from mmvid_amd import _lib, ops
    lc = torch.zeros(2, 256)
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.sample_race_guided_at(lc, lc, torch.ones(2), 1, lc)
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.decode_embed_groups(torch.zeros(2, dtype=torch.long), lc, lc, torch.zeros(1, dtype=torch.int32), torch.zeros(4, 256), 2)
