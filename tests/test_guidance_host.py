"""Classifier-free guidance, the host side (mmvid_amd/sampling.py, frontend.py, dalle_bert.py, completion.py): the scale table, every
rejected argument combination before any device work, and the declarations of the two entry points.  No GPU: nothing here launches a
kernel."""
import os
import re

import numpy as np
import pytest
import torch

from test_host_logic import tiny_bert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX, NB = 4, 3


# ------------------------------------------------------------------------------------------------------------ the scale table
def test_the_four_forms_of_guidance_scale_give_one_table():
    from mmvid_amd.sampling import guidance_table
    want = torch.full((TMAX, NB), 1.5)
    forms = [1.5, [1.5] * TMAX, torch.full((NB, ), 1.5), torch.full((TMAX, NB), 1.5)]
    for form in forms:
        got = guidance_table(form, TMAX, NB)
        assert got.dtype == torch.float32 and tuple(got.shape) == (TMAX, NB) and got.is_contiguous(), form
        assert torch.equal(got, want), form
    # the forms that vary: per step down the rows (step 0 included), per video along them
    per_step = guidance_table((0.0, 1.0, 2.0, 3.0), TMAX, NB)
    assert torch.equal(per_step, torch.arange(4.0).view(4, 1).expand(4, 3))
    per_video = guidance_table(torch.tensor([0.0, 0.5, 3.0], dtype=torch.float64), TMAX, NB)
    assert per_video.dtype == torch.float32 and torch.equal(per_video, torch.tensor([0.0, 0.5, 3.0]).expand(4, 3))
    full = torch.arange(12.0).view(TMAX, NB)
    assert torch.equal(guidance_table(full.t().contiguous().t(), TMAX, NB), full)  # (a strided tensor comes out contiguous)
    assert torch.equal(guidance_table(np.float32(2.0), TMAX, NB), torch.full((TMAX, NB), 2.0))
    assert torch.equal(guidance_table(torch.tensor(2.0), TMAX, NB), torch.full((TMAX, NB), 2.0))
    assert torch.equal(guidance_table(np.arange(4.0), TMAX, NB), per_step)


@pytest.mark.parametrize('bad', [[1.0] * (TMAX - 1), [1.0] * (TMAX + 1), [], torch.zeros(NB + 1), torch.zeros(TMAX), torch.zeros(NB, TMAX),
                                 torch.zeros(TMAX, NB, 1), torch.zeros(1, NB), 'high', float('nan'), [1.0, float('inf'), 1.0, 1.0]])
def test_guidance_scale_of_a_wrong_length_or_shape_is_refused(bad):
    from mmvid_amd.sampling import guidance_table
    with pytest.raises(ValueError, match='guidance_scale'):
        guidance_table(bad, TMAX, NB)


def test_mask_predict_wants_both_or_neither():
    from mmvid_amd import sampling
    control = torch.zeros(2, 18, 768)
    with pytest.raises(ValueError, match='come together'):
        sampling.mask_predict(None, control, steps=4, mp_config={'B': 2}, guidance_scale=2.0)
    with pytest.raises(ValueError, match='come together'):
        sampling.mask_predict(None, control, steps=4, mp_config={'B': 2}, uncond_emb=control)


# ------------------------------------------------------------------------------------------------------ rejected arguments
def test_check_guidance_rules():
    from mmvid_amd.sampling import check_guidance
    t2 = torch.ones(2, 16, dtype=torch.int64)
    assert check_guidance(0, False, None, ('text', 'visual'), None) is None  # unguided: the drop is not looked at
    assert check_guidance(1, False, 2.0, ('text', 'visual'), None) == ('text', 'visual')
    assert check_guidance(0, False, 2.0, ['text'], None) == ('text', )
    assert check_guidance(1, False, 2.0, 'visual', None) == ('visual', )
    assert check_guidance(1, False, 2.0, (), t2) == ()
    assert check_guidance(0, True, 2.0, ('text', ), t2) == ('text', )  # a fixed language model with a negative feature
    assert check_guidance(1, True, 2.0, ('visual', ), None) == ('visual', )
    with pytest.raises(ValueError, match='num_visuals == 0'):
        check_guidance(0, False, 2.0, ('text', 'visual'), None)
    with pytest.raises(ValueError, match='empty guidance_drop'):
        check_guidance(1, False, 2.0, (), None)
    with pytest.raises(ValueError, match='fixed language model'):
        check_guidance(1, True, 2.0, ('text', ), None)
    with pytest.raises(ValueError, match='without guidance_scale'):
        check_guidance(1, False, None, ('text', ), t2)
    with pytest.raises(ValueError, match='not among'):
        check_guidance(1, False, 2.0, ('text', 'audio'), None)


@pytest.fixture(scope='module')
def cpu_models():
    torch.manual_seed(3)
    return {0: tiny_bert(), 1: tiny_bert(num_visuals=1)}


def test_generate_images_and_complete_refuse_before_any_device_work(cpu_models, golden):
    """A model on the CPU: the first kernel call would raise MMVIDError, so a ValueError shows that the check came first."""
    from mmvid_amd import completion
    mp = golden('mask_predict').meta['mp_config']
    text = torch.ones(2, 16, dtype=torch.int64)
    t2 = torch.full((2, 16), 5, dtype=torch.int64)
    plain, vis = cpu_models[0], cpu_models[1]
    cases = [(plain, dict(guidance_scale=2.0), 'num_visuals == 0'),  # the default drop names 'visual'
             (vis, dict(guidance_scale=2.0, guidance_drop=()), 'empty guidance_drop'),
             (vis, dict(negative_text=t2), 'without guidance_scale'),
             (vis, dict(guidance_scale=2.0, guidance_drop=('motion', )), 'not among')]
    for model, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            model.generate_images(text, mask_predict_steps=4, mp_config=mp, **kw)
        frames = torch.zeros(2, model.target_seq_len, dtype=torch.int64)
        given = torch.zeros(2, model.num_targets, dtype=torch.uint8)
        with pytest.raises(ValueError, match=match):
            completion.complete(model, text, frames, given, mask_predict_steps=4, mp_config=mp, **kw)
    plain.fixed_language_model = 'roberta-large'  # (only the flag is read before the check)
    try:
        with pytest.raises(ValueError, match='fixed language model'):
            plain.generate_images(torch.zeros(2, 1024), mask_predict_steps=4, mp_config=mp, guidance_scale=2.0, guidance_drop=('text', ))
        with pytest.raises(ValueError, match='no defined null sentence feature'):
            plain(torch.zeros(2, 1024), target=torch.zeros(2, plain.target_seq_len, dtype=torch.int64), return_loss=True, null_text_prob=0.1)
    finally:
        plain.fixed_language_model = None


@pytest.mark.parametrize('kw', [dict(null_text_prob=-0.01), dict(null_text_prob=1.5), dict(null_visual_prob=-1.0),
                                dict(null_visual_prob=1.0001), dict(null_text_prob=float('nan'))])
def test_probabilities_outside_the_unit_interval_are_refused(cpu_models, kw):
    from mmvid_amd.frontend import Frontend, check_condition_drop
    full = dict(dict(null_text_prob=0.0, null_visual_prob=0.0), **kw)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        check_condition_drop(full['null_text_prob'], full['null_visual_prob'])
    model = cpu_models[0]
    text = torch.ones(2, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        model(text, target=torch.zeros(2, model.target_seq_len, dtype=torch.int64), return_loss=True, **kw)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        Frontend(seed=1).cond_drop(text, None, full['null_text_prob'], full['null_visual_prob'], 256)


def test_condition_drop_rules():
    from mmvid_amd.frontend import check_condition_drop
    assert check_condition_drop(0.0, 0.0) is False  # nothing to launch
    assert check_condition_drop(0, 0, return_loss=False) is False  # the control-only call with the defaults is untouched
    assert check_condition_drop(0.0, 0.0, injected=True) is True
    assert check_condition_drop(1.0, 0.0) is True and check_condition_drop(0.0, 0.25) is True
    assert check_condition_drop(0.0, 0.5, fixed_language_model=True) is True  # the visual half has a defined null
    with pytest.raises(ValueError, match='no defined null sentence feature'):
        check_condition_drop(0.5, 0.0, fixed_language_model=True)
    with pytest.raises(ValueError, match='control-only'):
        check_condition_drop(0.5, 0.0, return_loss=False)
    with pytest.raises(ValueError, match='control-only'):
        check_condition_drop(0.0, 0.0, return_loss=False, injected=True)


def test_the_control_only_forward_does_not_take_the_drop(cpu_models):
    text = torch.ones(2, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match='control-only'):
        cpu_models[0](text, return_loss=False, null_text_prob=0.5)


# --------------------------------------------------------------------------------------------------------------- declarations
def test_the_two_entries_are_declared_and_bound():
    from mmvid_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    assert re.search(r'\bint\s+mmvid_sample_race_guided\s*\(const float\* logits_c, const float\* logits_u, int64_t ld, '
                     r'const float\* scale_dev, int64_t rows_per_scale,\s*const float\* E, const float\* noise_u, float temperature, '
                     r'float logit_div, int64_t R, int V,\s*int64_t tok_offset, int64_t\* tok, float\* y, void\* stream\);', hdr)
    assert re.search(r'\bint\s+mmvid_cond_drop\s*\(const int64_t\* text, const int64_t\* vis_tok, int B, int Tt, int Vs, '
                     r'const float\* state_dev, uint64_t seed,\s*float p_text, float p_visual, const uint8_t\* inject, int64_t mask_id, '
                     r'int64_t\* text_out, int64_t\* vis_out,\s*uint8_t\* decided, void\* stream\);', hdr)
    assert 'dalle_bert.py:527-534' in hdr  # the reference lines the guided draw serves
    declared = set(re.findall(r'\b(mmvid_[a-z0-9_]+)\s*\(', hdr))  # the manifest the ABI test reads
    for name, nargs in (('mmvid_sample_race_guided', 15), ('mmvid_cond_drop', 15)):
        assert name in declared and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
    # the unguided entries keep their signatures, and symbols were only added
    assert len(_lib.SIGNATURES['mmvid_sample_race']) == 12 and len(_lib.SIGNATURES['mmvid_sample_race_at']) == 15
    assert _lib.ABI_VERSION == 3


def test_the_new_kernels_use_no_atomics_and_no_fused_guidance():
    """The guided value is three rounded operations: the function that computes it switches contraction off and uses plain operators
    (the rounding-mode wrappers fuse).  Neither new kernel adds an atomic (the census of test_deterministic_host.py stays as it is)."""
    src = open(os.path.join(ROOT, 'mmvid_amd', 'csrc', 'sample.hip')).read()
    body = re.search(r'float guided_logit\(float lc, float lu, float w\) \{(.*?)\n\}', src, re.S).group(1)
    assert '#pragma clang fp contract(off)' in body and 'fmaf' not in body and '_rn(' not in body
    assert 'return -INFINITY' in body
    fe = open(os.path.join(ROOT, 'mmvid_amd', 'csrc', 'frontend.hip')).read()
    drop = re.search(r'void cond_drop_kernel\(.*?\n\}', fe, re.S).group(0)
    assert 'atomic' not in drop and 'P_NULL_TEXT' in drop and 'P_NULL_VISUAL' in drop
    purposes = re.search(r'enum \{ P_STRATEGY.*?\};', fe, re.S).group(0)
    values = [int(v) for v in re.findall(r'=\s*(\d+)', purposes)]
    assert len(values) == len(set(values)) == 11  # the two new purposes collide with no existing stream
