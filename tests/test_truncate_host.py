"""Truncated sampling (top-k and nucleus), the host side: the keyword rules of sampling.check_truncation, every refusal before any
device work, the declaration of mmvid_logits_truncate, and the fp64 restatement of the rule (tests/truncate_ref.py) checked against
itself and against the condition its nucleus inputs must meet.  No GPU: nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

import truncate_ref as T
from test_host_logic import tiny_bert, tiny_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX, V = 4, 256


# ------------------------------------------------------------------------------------------------------ the keyword rules
def test_check_truncation_accepted_forms():
    from mmvid_amd.sampling import check_truncation
    assert check_truncation(None, None, TMAX, V) is None
    assert check_truncation(8, None, TMAX, V) == ([8] * TMAX, [None] * TMAX)
    assert check_truncation(None, 0.9, TMAX, V) == ([None] * TMAX, [0.9] * TMAX)
    assert check_truncation(np.int64(3), np.float32(0.5), TMAX, V) == ([3] * TMAX, [0.5] * TMAX)
    assert check_truncation((None, 8, 3, 1), 0.9, TMAX, V) == ([None, 8, 3, 1], [0.9] * TMAX)  # one per step, step 0 included
    assert check_truncation(5, [1.0, None, 0.25, 1], TMAX, V) == ([5] * TMAX, [1.0, None, 0.25, 1.0])
    assert check_truncation(np.array([1, 2, 3, 4]), None, TMAX, V) == ([1, 2, 3, 4], [None] * TMAX)
    assert check_truncation(V, 1.0, TMAX, V) == ([V] * TMAX, [1.0] * TMAX)  # both legal, both keep every class
    assert check_truncation(10 * V, None, TMAX, V) == ([10 * V] * TMAX, [None] * TMAX)
    k, p = check_truncation([7], [0.5], 1, V)  # the ART-V sampler: one step
    assert (k, p) == ([7], [0.5])
    assert all(type(v) is int for v in check_truncation(np.int32(3), None, TMAX, V)[0])
    assert all(type(v) is float for v in check_truncation(None, np.float64(0.5), TMAX, V)[1])


@pytest.mark.parametrize('kw', [dict(top_k=0), dict(top_k=-3), dict(top_k=2.0), dict(top_k=2.5), dict(top_k=True), dict(top_k='8'),
                                dict(top_k=[8, 8, 8]), dict(top_k=[8] * 5), dict(top_k=[]), dict(top_k=[8, 0, 8, 8]),
                                dict(top_k=[8, True, 8, 8]), dict(top_k=torch.tensor(8)), dict(top_k=torch.tensor([8, 8, 8, 8])),
                                dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=float('nan')), dict(top_p=float('inf')),
                                dict(top_p=True), dict(top_p='0.9'), dict(top_p=[0.9] * 3), dict(top_p=[0.9] * 5),
                                dict(top_p=[0.9, 0.0, 0.9, 0.9]), dict(top_p=[0.9, float('nan'), 0.9, 0.9]),
                                dict(top_p=torch.tensor(0.9)), dict(top_p=torch.full((3, ), 0.9))])
def test_check_truncation_refusals(kw):
    from mmvid_amd.sampling import check_truncation
    name = next(iter(kw))
    with pytest.raises(ValueError, match=name):
        check_truncation(kw.get('top_k'), kw.get('top_p'), TMAX, V)
    with pytest.raises(ValueError, match=name):  # ... whatever the other keyword holds
        check_truncation(kw.get('top_k', 4), kw.get('top_p', 0.5), TMAX, V)


@pytest.fixture(scope='module')
def cpu_bert():
    torch.manual_seed(3)
    return tiny_bert()


BAD = [(dict(top_k=0), 'top_k'), (dict(top_k=1.5), 'top_k'), (dict(top_k=True), 'top_k'), (dict(top_k=[4, 4, 4]), 'top_k'),
       (dict(top_k=torch.tensor([4, 4])), 'top_k'), (dict(top_p=0.0), 'top_p'), (dict(top_p=1.5), 'top_p'),
       (dict(top_p=float('nan')), 'top_p'), (dict(top_p=[0.9] * 5), 'top_p'), (dict(top_k=4, top_p=-1.0), 'top_p')]


def test_bert_and_complete_refuse_before_any_device_work(cpu_bert, golden):
    """A model on the CPU: the first kernel call would raise MMVIDError, so a ValueError shows that the check came first."""
    from mmvid_amd import completion
    mp = golden('mask_predict').meta['mp_config']
    text = torch.ones(2, 16, dtype=torch.int64)
    frames = torch.zeros(2, cpu_bert.target_seq_len, dtype=torch.int64)
    given = torch.zeros(2, cpu_bert.num_targets, dtype=torch.uint8)
    for kw, match in BAD:
        with pytest.raises(ValueError, match=match):
            cpu_bert.generate_images(text, mask_predict_steps=4, mp_config=mp, **kw)
        with pytest.raises(ValueError, match=match):
            completion.complete(cpu_bert, text, frames, given, mask_predict_steps=4, mp_config=mp, **kw)
    with pytest.raises(ValueError, match='top_k'):  # steps <= 0: the schedule's own length counts
        cpu_bert.generate_images(text, mask_predict_steps=0, mp_config=mp, top_k=[4] * (mp['T'] + 1))
    with pytest.raises(ValueError, match='top_p'):
        completion.complete(cpu_bert, text, frames, given, mask_predict_steps=0, mp_config=mp, top_p=[0.5] * (mp['T'] - 1))


def test_artv_refuses_before_any_device_work():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(4)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2)
    text = torch.ones(2, 16, dtype=torch.int64)
    for kw, match in BAD + [(dict(top_k=[4, 4]), 'top_k'), (dict(top_p=[0.5, 0.5]), 'top_p')]:  # (scalars: one step)
        with pytest.raises(ValueError, match=match):
            m.generate_images(text, **kw)
        with pytest.raises(ValueError, match=match):
            m.sampling_probs(torch.zeros(2, 256), **kw)
    # with the keywords absent (or unable to remove a class) sampling_probs is the expression it was
    lg = torch.randn(3, 256)
    want = torch.softmax(lg / 0.8, dim=-1)
    assert torch.equal(m.sampling_probs(lg, temperature=0.8), want)
    assert torch.equal(m.sampling_probs(lg, temperature=0.8, top_k=256, top_p=1.0), want)


def test_the_operator_refuses_host_tensors():
    from mmvid_amd import _lib, ops
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.logits_truncate(torch.zeros(2, 256), 4)


# --------------------------------------------------------------------------------------------------------------- declarations
def test_the_entry_is_declared_and_bound():
    from mmvid_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    assert re.search(r'\bint\s+mmvid_logits_truncate\s*\(const float\* logits, const float\* logits_u, int64_t ld, const float\* scale_dev, '
                     r'int64_t rows_per_scale,\s*float logit_div, int top_k, float top_p, int64_t R, int V,\s*float\* out, int64_t ld_out, '
                     r'int32_t\* kept, void\* stream\);', hdr)
    comment = hdr[:hdr.index('int mmvid_logits_truncate')].rsplit('/*', 1)[1]
    assert 'dalle_bert.py:527-534' in comment and 'dalle_artv.py:61-67' in comment  # the reference lines it serves
    declared = set(re.findall(r'\b(mmvid_[a-z0-9_]+)\s*\(', hdr))
    assert 'mmvid_logits_truncate' in declared and len(_lib.SIGNATURES['mmvid_logits_truncate']) == 14
    P, I, I64, F = _lib.P, _lib.I, _lib.I64, _lib.F
    assert _lib.SIGNATURES['mmvid_logits_truncate'] == [P, P, I64, P, I64, F, I, F, I64, I, P, I64, P, P]
    # the races keep their signatures, and symbols were only added
    assert _lib.SIGNATURES['mmvid_sample_race'] == [P, I64, P, P, F, F, I64, I, I64, P, P, P]
    assert _lib.SIGNATURES['mmvid_sample_race_at'] == [P, I64, P, P, I, I64, P, F, F, I64, I, I64, P, P, P]
    assert _lib.SIGNATURES['mmvid_sample_race_guided'] == [P, P, I64, P, I64, P, P, F, F, I64, I, I64, P, P, P]
    assert _lib.ABI_VERSION == 3


def test_the_new_kernel_uses_no_atomics_and_reuses_the_guided_value():
    src = open(os.path.join(ROOT, 'mmvid_amd', 'csrc', 'sample.hip')).read()
    kernel = re.search(r'void logits_truncate_kernel\(.*?\n\}', src, re.S).group(0)
    assert 'atomic' not in kernel and '__shared__' not in kernel and '__syncthreads' not in kernel
    assert 'guided_logit(x[c], xu[c], w)' in kernel
    assert len(re.findall(r'float guided_logit\(', src)) == 1  # reused, not restated
    entry = re.search(r'extern "C" int mmvid_logits_truncate\(.*?\n\}', src, re.S).group(0)
    assert 'atomic' not in entry
    assert 'Truncation rule' in src[:src.index('#include')]  # the rule stands in the header comment


# --------------------------------------------------------------------------------------------------- the helper, against itself
def test_topk_set_against_torch_topk_on_tie_free_rows():
    gen = torch.Generator().manual_seed(51)
    for Vv, k in ((100, 1), (100, 37), (256, 64), (1000, 250), (1024, 1000)):
        g = torch.randn(9, Vv, generator=gen)
        assert all(len(np.unique(row)) == Vv for row in g.numpy())  # tie free
        want = torch.zeros(9, Vv, dtype=torch.bool).scatter_(1, torch.topk(g, k).indices, True)
        assert np.array_equal(T.topk_set(g.numpy(), k), want.numpy()), (Vv, k)
        assert np.array_equal(T.order(g.numpy()), torch.sort(g, dim=1, descending=True).indices.numpy())
    g = torch.randn(2, 50, generator=gen).numpy()
    for off in (None, 0, -1, 50, 51):
        assert T.topk_set(g, off).all()


def test_nucleus_set_against_a_sort_and_cumsum_restatement():
    gen = torch.Generator().manual_seed(52)
    for Vv, p, div in ((100, 0.5, 1.0), (256, 0.9, 0.5), (1000, 0.95, 2.0), (64, 0.999, 1.0)):
        g = (4 * torch.randn(11, Vv, generator=gen))
        g[:, ::7] = T.NEG_INF
        probs = torch.softmax(g.double() / div, dim=1)
        sp, idx = torch.sort(probs, dim=1, descending=True, stable=True)
        keep_sorted = (torch.cumsum(sp, 1) - sp) < p
        want = torch.zeros_like(keep_sorted).scatter_(1, idx, keep_sorted)
        got = T.nucleus_set(g.numpy(), p, div)
        assert np.array_equal(got, want.numpy()), (Vv, p, div)
        assert got[np.arange(11), g.argmax(1).numpy()].all() and not got[:, ::7].any()  # rank 0 stays; no mass, not kept
        assert T.is_head(g.numpy(), got).all()
        # the smallest head whose mass reaches p
        mass = (probs.numpy() * got).sum(1)
        smallest = np.where(got, probs.numpy(), np.inf).min(1)
        assert (mass >= p - 1e-12).all() and (mass - smallest < p).all()
    assert T.nucleus_set(g.numpy(), 1.0).all()
    lo, hi = T.sandwich(g.numpy(), 0.9, 0.01, 2.0)
    assert (lo <= hi).all() and np.array_equal(lo, T.nucleus_set(g.numpy(), 0.89, 2.0))


def test_the_crafted_tie_rows_give_the_sets_written_with_them():
    for name, g, k, want in T.tie_rows():
        out = T.truncated(g, T.topk_set(g, k))
        assert list(np.flatnonzero(np.isfinite(out))) == want, name
        assert np.array_equal(out[want].view(np.int32), g[want].view(np.int32)), name  # kept values keep their bits
        assert T.is_head(g, T.topk_set(g, k)).all(), name


@pytest.mark.parametrize('Vv,p,div', T.NUCLEUS_CASES)
def test_the_nucleus_inputs_meet_the_condition_of_the_margin(Vv, p, div):
    """What the derivation of DELTA assumes (A <= 4) and what the sandwich needs to say something (few rows that are not tight)."""
    g = T.nucleus_input(Vv)
    assert g.shape == (T.NUCLEUS_ROWS, Vv) and T.NUCLEUS_ROWS == 512
    A = T.mean_distance(g, div)
    lo, hi = T.sandwich(g, p, T.DELTA, div)
    loose = float((lo != hi).any(axis=1).mean())
    print(f'V = {Vv}, top_p = {p}, logit_div = {div}: max A = {A.max():.3f}, {100 * loose:.2f} % of the rows not tight')
    assert A.max() <= T.MAX_MEAN_DISTANCE
    assert loose <= T.MAX_LOOSE_SHARE
    assert (lo <= hi).all() and T.DELTA == 2.0**-16 and T.MAX_LOOSE_SHARE == 0.05 and T.MAX_MEAN_DISTANCE == 4.0


def test_the_cases_are_the_ones_the_margin_was_derived_for():
    want = {(Vv, p, 1.0) for Vv in (200, 256, 1024) for p in (0.5, 0.9, 0.95)} | {(256, p, d) for d in (0.5, 2.0) for p in (0.5, 0.9, 0.95)}
    assert set(T.NUCLEUS_CASES) == want and len(T.NUCLEUS_CASES) == 15
    for _, _, div in T.NUCLEUS_CASES:  # powers of two: the division of the logits is exact (see the helper's docstring)
        assert np.log2(div) == int(np.log2(div))
