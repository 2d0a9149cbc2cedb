"""ART-V video prediction, host side: the runs of a frame mask, the grouping of a batch by mask and the scatter back, every refusal of
`given` on a CPU-resident model before anything reaches the device, the refusal of the interp modes, and what must not have moved: the
signatures of `complete` and `generate_long`, the entry count and the ABI number.  No GPU: nothing here launches a kernel."""
import inspect
import itertools

import pytest
import torch

from test_host_logic import tiny_vae

B, TT, T, N, V = 3, 16, 4, 16, 256


# --------------------------------------------------------------------------------------------------------------------- segments
def runs_by_hand(row):
    """[(known, frame0, frames)] by the definition: a run ends where the next frame's flag differs."""
    out, t = [], 0
    while t < len(row):
        e = t
        while e < len(row) and bool(row[e]) == bool(row[t]):
            e += 1
        out.append((bool(row[t]), t, e - t))
        t = e
    return out


def test_segments_on_every_mask_of_four_frames():
    from mmvid_amd.artv_sampling import segments
    for row in itertools.product((0, 1), repeat=T):
        segs = segments(row)
        assert segs == runs_by_hand(row), row
        assert sum(nf for _, _, nf in segs) == T and [f0 for _, f0, _ in segs] == [sum(nf for _, _, nf in segs[:i]) for i in range(len(segs))]
        assert all(a[0] != b[0] for a, b in zip(segs, segs[1:])), row  # neighbours alternate
        for k, f0, nf in segs:
            assert all(bool(v) == k for v in row[f0:f0 + nf]), row
        for form in (torch.tensor(row, dtype=torch.uint8), torch.tensor(row, dtype=torch.bool), list(row)):
            assert segments(form) == segs
    assert segments((0, 0, 0, 0)) == [(False, 0, 4)] and segments((1, 1, 1, 1)) == [(True, 0, 4)]
    assert segments((1, 0, 1, 0)) == [(True, 0, 1), (False, 1, 1), (True, 2, 1), (False, 3, 1)]
    assert segments((0, 1, 1, 0)) == [(False, 0, 1), (True, 1, 2), (False, 3, 1)]
    assert segments(()) == []


def test_rows_are_grouped_by_mask_and_scattered_back():
    from mmvid_amd.artv_sampling import group_rows, scatter_rows
    mask = torch.tensor([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0]], dtype=torch.uint8)
    groups = group_rows(mask)
    assert groups == [((1, 0, 0, 0), [0, 2, 5]), ((1, 1, 0, 0), [1, 4]), ((0, 0, 0, 0), [3])]
    assert group_rows(mask.bool()) == groups
    assert sorted(r for _, rows in groups for r in rows) == list(range(6))
    want = torch.arange(6 * 5).view(6, 5)
    parts = [(rows, want[rows] + 0) for _, rows in groups]
    assert torch.equal(scatter_rows(parts, 6), want)
    assert torch.equal(scatter_rows(parts[::-1], 6), want)
    one = [(list(range(6)), want)]
    assert scatter_rows(one, 6) is want  # one group over the whole batch: nothing is copied
    with pytest.raises(ValueError, match='rows'):
        scatter_rows(parts[:2], 6)


# --------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(90)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=T, transformer_layers=2).eval()
    gen = torch.Generator().manual_seed(91)
    return m, torch.randint(1, 49408, (B, TT), generator=gen), torch.randint(0, V, (B, N), generator=gen)


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library fails the test: the rules below come before device work."""
    from mmvid_amd import _lib

    def refuse(name, *args):
        raise AssertionError(f'{name} was called before the arguments were checked')
    monkeypatch.setattr(_lib, 'call', refuse)
    monkeypatch.setattr('mmvid_amd.ops.call', refuse)


def tokens(fill=None):
    t = torch.randint(0, V, (B, T * N), generator=torch.Generator().manual_seed(92))
    if fill is not None:
        t[1, N + 3] = fill  # frame 1 of video 1
    return t


ROW = torch.tensor([1, 1, 0, 0], dtype=torch.uint8)
BAD_GIVEN = {
    'a token-grid mask': ((torch.ones(B, T, 4, 4, dtype=torch.uint8), tokens()), 'raster-order'),
    'a pixel mask': ((torch.ones(B, T, 64, 64, dtype=torch.bool), tokens()), 'raster-order'),
    'a float mask': ((torch.ones(B, T), tokens()), 'bool or uint8'),
    'an int64 mask': ((torch.ones(B, T, dtype=torch.long), tokens()), 'bool or uint8'),
    'a mask of B + 1 rows': ((torch.ones(B + 1, T, dtype=torch.uint8), tokens()), r'\[B, T\]'),
    'a mask of T + 1 frames': ((torch.ones(T + 1, dtype=torch.uint8), tokens()), r'\[B, T\]'),
    'a token-sized mask': ((torch.ones(B, T * N, dtype=torch.uint8), tokens()), r'\[B, T\]'),
    'int32 tokens': ((ROW, tokens().int()), 'int64'),
    'tokens [B, T, n]': ((ROW, tokens().view(B, T, N)), 'int64'),
    'tokens of B + 1 rows': ((ROW, torch.cat((tokens(), tokens()[:1]))), 'int64'),
    'tokens as a list': ((ROW, tokens().tolist()), 'int64'),
    'a known id equal to num_image_tokens': ((ROW, tokens(V)), 'outside'),
    'a known negative id': ((ROW, tokens(-1)), 'outside'),
    'a mask alone': (ROW, r'\(mask, tokens\)'),
    'three things': ((ROW, tokens(), None), r'\(mask, tokens\)'),
}


@pytest.mark.parametrize('name', list(BAD_GIVEN))
@pytest.mark.parametrize('use_cache', [True, False])
def test_generate_images_refuses_a_bad_given_before_any_device_work(artv, no_device, name, use_cache):
    m, text, vis = artv
    given, match = BAD_GIVEN[name]
    with pytest.raises(ValueError, match=match):
        m.generate_images(text, visual=vis, use_cache=use_cache, given=given)


def test_ids_under_a_zero_mask_are_not_read(artv):
    from mmvid_amd.artv_sampling import check_given
    m = artv[0]
    tok = tokens(V + 7)  # frame 1 of video 1
    mask, out = check_given((torch.tensor([1, 0, 1, 0], dtype=torch.bool), tok), B, T, N, V)
    assert out is tok and mask.dtype == torch.uint8 and mask.tolist() == [[1, 0, 1, 0]] * B
    rows = torch.tensor([[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.uint8)
    assert check_given((rows, tok), B, T, N, V)[0].tolist() == rows.tolist()
    with pytest.raises(ValueError, match='1 known token ids are outside'):
        check_given((rows.roll(1, 0), tok), B, T, N, V)  # now video 1 knows its frame 1


def test_race_and_trace_need_one_mask(artv, no_device):
    m, text, vis = artv
    two = torch.tensor([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0]], dtype=torch.uint8)
    with pytest.raises(ValueError, match='2 distinct masks'):
        m.generate_images(text, visual=vis, given=(two, tokens()), _race=lambda name, shape: torch.ones(shape))
    with pytest.raises(ValueError, match='2 distinct masks'):
        m.generate_images(text, visual=vis, given=(two, tokens()), _trace=[])
    # the rules of the call without `given` still come first to last
    with pytest.raises(ValueError, match='finite'):
        m.generate_images(text, visual=vis, given=(ROW, tokens()), guidance_scale=float('nan'))
    with pytest.raises(ValueError, match='use_cache=True'):
        m.generate_images(text, visual=vis, given=(ROW, tokens()), use_cache=False, _trace=[])


def test_complete_artv_refuses_masks_finer_than_a_frame(artv, no_device):
    from mmvid_amd import completion
    m, text, vis = artv
    frames = tokens()
    for given, match in ((torch.ones(B, T, 4, 4, dtype=torch.uint8), 'raster-order'), (torch.ones(B, T, 64, 64, dtype=torch.uint8), 'raster-order'),
                         (torch.ones(B, T), 'bool or uint8'), (torch.ones(B, T + 1, dtype=torch.uint8), r'\[B, T\]')):
        with pytest.raises(ValueError, match=match):
            completion.complete_artv(m, text, frames, given, visual=vis)
    with pytest.raises(ValueError, match='token input must be int64'):
        completion.complete_artv(m, text, frames[:, :-1], ROW, visual=vis)
    with pytest.raises(ValueError, match='outside'):
        completion.complete_artv(m, text, tokens(V), ROW, visual=vis)
    doc = completion.complete_artv.__doc__
    assert 'CAUSALITY' in doc and 'only the frames that come after it' in doc


def test_everything_known_returns_the_given_tokens_without_the_device(artv, no_device):
    m, text, vis = artv
    tok = tokens()
    called = []
    _, out = m.sample_tokens(text, visual=vis, given=(torch.ones(T, dtype=torch.bool), tok), _race=lambda name, shape: called.append(name))
    assert torch.equal(out, tok) and out is not tok and not called


# ------------------------------------------------------------------------------------------------------------------- long videos
@pytest.mark.parametrize('mode', ['interp', 'interp_real'])
def test_the_interp_modes_are_refused(artv, no_device, mode):
    from mmvid_amd import long_video
    m, text, vis = artv
    with pytest.raises(ValueError, match='extrapolates only'):
        long_video.generate_long_artv(m, text, visual=vis, mode=mode, t_repeat=2)
    sample = long_video.artv_sampler(m, text, visual=vis)
    with pytest.raises(ValueError, match='extrapolates only'):
        sample(1, 0, (0, B), torch.zeros(B, T * N, dtype=torch.long), mode, 1)
    with pytest.raises(ValueError, match='expected one of'):
        long_video.generate_long_artv(m, text, visual=vis, mode='backwards')
    with pytest.raises(ValueError, match='t_overlap'):
        long_video.generate_long_artv(m, text, visual=vis, t_overlap=T)


def test_the_sampler_hands_the_last_frames_of_the_previous_clip_on(artv, monkeypatch):
    from mmvid_amd import long_video
    m, text, vis = artv
    calls = []
    monkeypatch.setattr(m, 'sample_tokens', lambda t, **kw: (calls.append((t, kw)), (t, torch.full((t.shape[0], T * N), 7)))[1])
    sample = long_video.artv_sampler(m, text, visual=vis, top_k=3, _race=lambda name, shape: name)
    prev = torch.arange(B * T * N).view(B * T, N)
    assert sample(0, 0, (0, B), None, 'long', 0).shape == (B, T * N)
    sample(2, 0, (0, B), prev, 'long', 2)
    sample(2, 1, (1, 3), prev[T:], 'long', 1)
    (t0, kw0), (t1, kw1), (t2, kw2) = calls
    assert kw0['given'] is None and t0 is text and kw0['visual'] is vis and kw0['top_k'] == 3
    mask, tok = kw1['given']
    assert mask.tolist() == [1, 1, 0, 0] and torch.equal(tok[:, :2 * N], prev.view(B, T, N)[:, 2:].reshape(B, 2 * N))
    assert kw1['_race']('tok5', (1, 1)) == 'L2c0/tok5'
    mask, tok = kw2['given']
    assert mask.tolist() == [1, 0, 0, 0] and torch.equal(tok[:, :N], prev.view(B, T, N)[1:, 3]) and torch.equal(t2, text[1:])
    assert torch.equal(kw2['visual'], vis[1:]) and kw2['_race']('tok0', (1, 1)) == 'L2c1/tok0'


# ------------------------------------------------------------------------------------------------------------ what did not move
def test_complete_and_generate_long_keep_their_signatures():
    from mmvid_amd import completion, long_video
    assert str(inspect.signature(completion.complete)) == (
        "(model, text, frames, given, *, visual=None, mask_predict_steps=0, mp_config=None, dynamic=True, erase_visual=False, vc_mode=None, "
        "face_mode=None, decode=True, paste=True, guidance_scale=None, guidance_drop=('text', 'visual'), negative_text=None, top_k=None, "
        "top_p=None, _race=None, _trace=None)")
    assert str(inspect.signature(long_video.generate_long)) == (
        "(model, text, *, visual=None, mode='long', t_repeat=10, t_overlap=1, real_frames=None, which_vae='vae', mask_predict_steps=0, "
        "mp_config=None, dynamic=True, erase_visual=False, vc_mode=None, face_mode=None, decode=True, max_rows=64, trace=None, _race=None)")
    with pytest.raises(ValueError, match='mp_config is required'):
        completion.complete(None, None, None, None)
    names = list(inspect.signature(completion.complete_artv).parameters)
    assert names[:4] == ['model', 'text', 'frames', 'given'] and {'visual', 'paste', 'top_k', 'top_p', 'guidance_scale', 'temperature'} <= set(names)


def test_no_entry_was_added_and_the_abi_number_stands():
    from mmvid_amd import _lib
    assert len(_lib.SIGNATURES) + len(_lib.OTHER) == 144
    assert _lib.ABI_VERSION == 3
