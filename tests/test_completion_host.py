"""Video completion without a device (mmvid_amd/completion.py, the `given` path of mmvid_amd/sampling.py): the token mask of the three
input shapes, the per-row keep-count table against the schedule, the rejected arguments, and the declarations of the two entry points."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

T, F, S = 4, 4, 64  # frames, token grid, pixels: the tiny model of tests/test_long_video_gpu.py
TS = T * F * F


# ------------------------------------------------------------------------------------------------------------------ token_mask
def test_token_mask_of_whole_frames():
    from mmvid_amd.completion import token_mask
    g = torch.tensor([[1, 0, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.bool)
    m = token_mask(g, T, F, S)
    assert m.shape == (3, TS) and m.dtype == torch.uint8
    assert torch.equal(m.view(3, T, F * F), g.to(torch.uint8).view(3, T, 1).expand(3, T, F * F))


def test_token_mask_of_a_token_grid():
    from mmvid_amd.completion import token_mask
    gen = torch.Generator().manual_seed(1)
    g = torch.rand(2, T, F, F, generator=gen) < 0.5
    m = token_mask(g, T, F, S)
    assert m.shape == (2, TS) and m.dtype == torch.uint8 and torch.equal(m, g.reshape(2, TS).to(torch.uint8))
    assert torch.equal(token_mask(g.to(torch.uint8) * 7, T, F, S), m)  # any non-zero value means known


def test_token_mask_of_pixels_needs_the_whole_patch():
    from mmvid_amd.completion import token_mask
    p = S // F
    g = torch.zeros(2, T, S, S, dtype=torch.uint8)
    g[0, 1, p:3 * p, 2 * p:4 * p] = 1  # frame 1 of video 0: tokens (1..2, 2..3)
    g[1] = 1
    g[1, 3, 2 * p + 5, 3 * p - 1] = 0  # one pixel of token (2, 2) of frame 3 is missing: the token is not given
    g[0, 2, p:2 * p - 1, 0:p] = 1  # a patch that lacks its last row of pixels
    m = token_mask(g, T, F, S).view(2, T, F, F)
    want = torch.zeros(2, T, F, F, dtype=torch.uint8)
    want[0, 1, 1:3, 2:4] = 1
    want[1] = 1
    want[1, 3, 2, 2] = 0
    assert torch.equal(m, want)


@pytest.mark.parametrize('shape', [(2, ), (2, 3), (2, T, F), (2, T, F, F + 1), (2, T, S, S, 3), (2, T, 8, 8)])
def test_token_mask_refuses_other_shapes(shape):
    from mmvid_amd.completion import token_mask
    with pytest.raises(ValueError) as e:
        token_mask(torch.ones(shape, dtype=torch.uint8), T, F, S)
    for form in ('[b, T]', '[b, T, h, w]', '[b, T, H, W]'):
        assert form in str(e.value)


# ------------------------------------------------------------------------------------------------------------- the keep counts
def test_keep_table_is_the_schedule_of_each_row(golden):
    from mmvid_amd import sampling
    mp = golden('mask_predict').meta['mp_config']
    unknown = [0, 3, 16, 64, 16]
    for Tmax in (2, 6, mp['T']):
        table = sampling.keep_table(mp, unknown, Tmax)
        assert table.shape == (Tmax - 1, len(unknown)) and table.dtype.name == 'int32'
        for i, N in enumerate(unknown):
            n = sampling.schedule(mp, N)[0]
            assert [int(v) for v in table[:, i]] == [N - n[t - 1] for t in range(1, Tmax)]
    assert sampling.schedule(mp, 64)[1] == sampling.schedule(mp, 3)[1]  # the temperature schedule does not depend on N


# ------------------------------------------------------------------------------------------------------- rejected arguments
def stub_model():
    m = SimpleNamespace(target_seq_len=TS, image_seq_len=F * F, num_targets=T, image_size=S, image_fmap_size=F, num_image_tokens=256,
                        image_token_lut={'[MASK]': 256}, training=False)
    m.eval = lambda: m
    m.train = lambda mode=True: m
    return m


def test_given_is_exclusive_with_preserve_and_interp(golden):
    from mmvid_amd import sampling
    mp = golden('mask_predict').meta['mp_config']
    control = torch.zeros(2, 18, 768)
    given = (torch.zeros(2, TS, dtype=torch.uint8), torch.zeros(2, TS, dtype=torch.int64))
    with pytest.raises(ValueError, match='exclusive'):
        sampling.mask_predict(stub_model(), control, steps=4, mp_config=mp, given=given, preserve=torch.zeros(2 * T, F * F, dtype=torch.int64))
    with pytest.raises(ValueError, match='exclusive'):
        sampling.mask_predict(stub_model(), control, steps=4, mp_config=mp, given=given, long_mode='interp')


@pytest.mark.parametrize('mask_shape,tok_shape,mask_dtype,tok_dtype', [
    ((2, TS - 1), (2, TS), torch.uint8, torch.int64), ((3, TS), (2, TS), torch.uint8, torch.int64),
    ((2, TS), (2, TS + 1), torch.bool, torch.int64), ((2, TS), (1, TS), torch.uint8, torch.int64),
    ((2, T, F * F), (2, TS), torch.uint8, torch.int64), ((2, TS), (2, TS), torch.float32, torch.int64),
    ((2, TS), (2, TS), torch.uint8, torch.int32)])
def test_given_shapes_must_match_the_rows(golden, mask_shape, tok_shape, mask_dtype, tok_dtype):
    from mmvid_amd import sampling
    mp = golden('mask_predict').meta['mp_config']
    given = (torch.zeros(mask_shape, dtype=mask_dtype), torch.zeros(tok_shape, dtype=tok_dtype))
    with pytest.raises(ValueError, match=r'\[b, TS\]'):
        sampling.mask_predict(stub_model(), torch.zeros(2, 18, 768), steps=4, mp_config=mp, given=given)


def test_complete_refuses_a_given_token_outside_the_table(golden):
    from mmvid_amd import completion
    mp = golden('mask_predict').meta['mp_config']
    text = torch.ones(2, 16, dtype=torch.int64)
    tokens = torch.randint(0, 256, (2, TS), generator=torch.Generator().manual_seed(2))
    given = torch.zeros(2, T, dtype=torch.uint8)
    given[1, 2] = 1
    for bad in (256, -1):
        t = tokens.clone()
        t[1, 2 * F * F + 3] = bad  # inside the given frame
        with pytest.raises(ValueError, match='outside'):
            completion.complete(stub_model(), text, t, given, mask_predict_steps=4, mp_config=mp)
    with pytest.raises(ValueError, match=r'\[b, T \* n\]'):
        completion.complete(stub_model(), text, tokens[:, :-1], given, mask_predict_steps=4, mp_config=mp)
    with pytest.raises(ValueError, match='mp_config'):
        completion.complete(stub_model(), text, tokens, given)


# --------------------------------------------------------------------------------------------------------------- declarations
def test_the_two_entries_are_declared_and_bound():
    from mmvid_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    assert re.search(r'\bint\s+mmvid_mp_select_keep_rows\s*\(const float\* Y, const float\* E, const uint8_t\* given, const int32_t\* k_rows, '
                     r'int b, int Bm, int TS,\s*uint8_t\* mask1, void\* stream\);', hdr)
    assert re.search(r'\bint\s+mmvid_frames_paste_u8\s*\(const float\* img, const uint8_t\* real, const uint8_t\* given, int64_t N, int H, '
                     r'int W, int h, int w,\s*uint8_t\* out, void\* stream\);', hdr)
    # the old entries keep their signatures
    assert re.search(r'\bint\s+mmvid_mp_select_keep\s*\(const float\* Y, const float\* E, const uint8_t\* preserve, int b, int Bm, int TS, '
                     r'int k,\s*uint8_t\* mask1, void\* stream\);', hdr)
    assert re.search(r'\bint\s+mmvid_frames_to_u8\s*\(const float\* img, int64_t N, int H, int W, uint8_t\* out, void\* stream\);', hdr)
    assert len(_lib.SIGNATURES['mmvid_mp_select_keep_rows']) == 9 and len(_lib.SIGNATURES['mmvid_frames_paste_u8']) == 10
    assert _lib.ABI_VERSION == 3  # symbols were only added
