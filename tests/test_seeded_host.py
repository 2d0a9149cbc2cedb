"""Seeded sampling without a GPU: the second header and its binding, the name / shape mapping of seeded.SeededRace, the refusals of
the `seeds` keyword (all raised before any device work: the models here live on the CPU, where the first kernel call would raise
MMVIDError instead), the long-video substream id, and the block layout of the host replica (tests/variates_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import variates_ref as R
from frontend_ref import philox4x32_10
from test_host_logic import tiny_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the second header
def test_ext_header_parses_and_is_bound_from_tables_of_its_own():
    from mmvid_amd import _cdecl, _lib, build
    assert os.path.samefile(_cdecl.EXT_HEADER_PATH, os.path.join(ROOT, 'include', 'mmvid_hip_ext.h'))
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)
    assert not hdr.structs and not hdr.constants and 'mmvid_variates_fill' in hdr.functions
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    for name in hdr.functions:
        assert len(re.findall(r'\b%s\s*\(' % name, bare)) == 1, f'{name} is declared more than once'
        assert name not in _lib.SIGNATURES and name not in _lib.OTHER and name not in _lib.HEADER.functions
        assert _lib.EXT_SIGNATURES[name] == hdr.functions[name][1] and hdr.functions[name][0] is ctypes.c_int
    assert set(_lib.EXT_SIGNATURES) == set(hdr.functions) == set(_lib.EXT_HEADER.functions)
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.EXT_SIGNATURES['mmvid_variates_fill'] == [P, P, I64, I64, I64, I, I, P, I64, I64, P, P]
    assert 'variates' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'variates.hip'))


def test_library_exports_and_binds_every_ext_symbol():
    from mmvid_amd import _lib
    lib = _lib.load()
    assert not lib._mmvid_missing
    for name, args in _lib.EXT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(args) and fn.restype is ctypes.c_int, name


def test_the_build_watches_the_ext_header(monkeypatch):
    from mmvid_amd import _cdecl, build
    real = os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda p: 4e9 if os.path.abspath(p) == os.path.abspath(_cdecl.EXT_HEADER_PATH) else real(p))
    assert build._deps_mtime() == 4e9


def test_a_library_without_an_ext_symbol_is_refused(monkeypatch):
    """The package's own library must have every ext symbol; one given through MMVID_LIB (an older build for an A/B) loads, and
    calling the symbol it lacks raises."""
    from mmvid_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'EXT_SIGNATURES', dict(_lib.EXT_SIGNATURES, mmvid_no_such_entry=[ctypes.c_void_p]))
    monkeypatch.delenv('MMVID_LIB', raising=False)
    with pytest.raises(_lib.MMVIDError, match='mmvid_no_such_entry'):
        _lib.load()
    monkeypatch.setenv('MMVID_LIB', _lib.LIB_PATH)
    lib = _lib.load()
    assert lib._mmvid_missing == {'mmvid_no_such_entry'}
    with pytest.raises(_lib.MMVIDError, match='older build'):
        _lib.call('mmvid_no_such_entry', None)
    monkeypatch.setattr(_lib, '_lib', None)  # (the next user loads it afresh, with the real tables)


def test_the_entry_point_refuses_bad_arguments_without_a_launch():
    """Every refusal of the header, through _lib.call (which also shows call() serves the ext names).  The pointers are never
    dereferenced: the argument checks come first and nothing is launched."""
    from mmvid_amd import _lib
    ok = dict(seeds=ctypes.c_void_p(64), sub=None, videos=2, rpv=3, n=5, purpose=1, kind=1, ddev=None, d0=0, draws=1, out=ctypes.c_void_p(64))

    def call(**kw):
        a = dict(ok, **kw)
        _lib.call('mmvid_variates_fill', a['seeds'], a['sub'], a['videos'], a['rpv'], a['n'], a['purpose'], a['kind'], a['ddev'], a['d0'],
                  a['draws'], a['out'], None)

    for kw, word in ((dict(seeds=None), 'NULL'), (dict(out=None), 'NULL'), (dict(videos=-1), 'negative'), (dict(rpv=-1), 'negative'),
                     (dict(n=-1), 'negative'), (dict(draws=-1), 'negative'), (dict(rpv=1 << 20, n=(1 << 14) + 1), '2\\^34'),
                     (dict(purpose=0), 'purpose'), (dict(purpose=4), 'purpose'), (dict(kind=2), 'kind'), (dict(kind=-1), 'kind'),
                     (dict(ddev=ctypes.c_void_p(64), draws=2), 'one draw'), (dict(d0=-1), 'draw numbers'),
                     (dict(d0=(1 << 32) - 1, draws=2), 'draw numbers')):
        with pytest.raises(_lib.MMVIDError, match=word):
            call(**kw)
    for kw in (dict(videos=0), dict(rpv=0), dict(n=0), dict(draws=0)):  # nothing to fill: no launch, no error
        call(**kw)


# -------------------------------------------------------------------------------------------------- names, shapes, seeds
def test_names_map_to_purpose_kind_and_draw_number():
    from mmvid_amd import seeded
    assert seeded.parse_name('tok0') == (R.TOKEN_RACE, R.EXP1, 0)
    assert seeded.parse_name('tok17') == (R.TOKEN_RACE, R.EXP1, 17)
    assert seeded.parse_name('tok3_noise_u') == (R.TOKEN_NOISE, R.UNIFORM, 3)
    assert seeded.parse_name('keep9') == (R.KEEP_RACE, R.EXP1, 9)
    for bad in ('tok', 'keep', 'tok-1', 'keep2_noise_u', 'L0c0/tok1', 'score3', 'tok1 ', ''):
        with pytest.raises(ValueError, match='no stream'):
            seeded.parse_name(bad)


def test_shapes_map_to_rows_per_video():
    from mmvid_amd import seeded
    b, nb, TS, V, Bm = 3, 2, 64, 256, 2
    assert seeded.layout((b * nb * TS, V), b) == (nb * TS, V)  # the token race and its noise: nb * TS rows of V per video
    assert seeded.layout((b * 1 * TS, V), b) == (TS, V)  # step 0: one candidate
    assert seeded.layout((b, Bm, TS), b) == (Bm, TS)  # the keep race: Bm rows of TS per video
    assert seeded.layout((b, V), b) == (1, V)  # ART-V: one row of V
    for shape, videos in (((7, V), 3), ((V, ), 1), ((4, V), 0)):
        with pytest.raises(ValueError):
            seeded.layout(shape, videos)


def test_check_seeds():
    from mmvid_amd import seeded
    assert seeded.check_seeds(None, 3) is None
    assert seeded.check_seeds([0, 5, 2**63 - 1], 3) == [0, 5, 2**63 - 1]
    assert seeded.check_seeds((np.int64(4), 7), 2) == [4, 7]
    assert seeded.check_seeds(torch.tensor([1, 2], dtype=torch.int64), 2) == [1, 2]
    assert seeded.check_seeds(np.array([1, 2], np.uint32), 2) == [1, 2]
    for bad, b in (([1, 2], 3), ([1, 2, 3], 2), ([-1], 1), ([2**63], 1), ([1.0], 1), ([True], 1), (['1'], 1), (torch.tensor([1.0]), 1),
                   (torch.tensor([[1]]), 1), (torch.tensor([True]), 1), (torch.tensor([-4]), 1), (5, 1), (np.array([1.5]), 1)):
        with pytest.raises(ValueError, match='seeds'):
            seeded.check_seeds(bad, b)
    with pytest.raises(ValueError, match='_race'):
        seeded.check_seeds([1], 1, race=lambda name, shape: None)
    with pytest.raises(ValueError, match='erase_visual'):
        seeded.check_seeds([1], 1, erase_visual=True)
    assert seeded.check_seeds(None, 1, race=lambda name, shape: None, erase_visual=True) is None  # (no seeds: nothing to refuse)


# ------------------------------------------------------------------------------------------ the refusals of the keyword
T, TT = 4, 16
BAD = (([1, 2, 3], 'one per video'), ([1, -2], r'\[0, 2\^63\)'), ([1, 2.0], r'\[0, 2\^63\)'), ([True, 1], r'\[0, 2\^63\)'))


@pytest.fixture(scope='module')
def bert():
    from mmvid_amd.dalle_bert import BERT
    torch.manual_seed(1)
    return BERT(dim=768, vae=tiny_vae(), num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual', num_visuals=0,
                num_targets=T, transformer_layers=1).eval()


@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(2)
    return DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
                 num_visuals=1, num_targets=T, transformer_layers=1).eval()


def hook(name, shape):
    raise AssertionError('the hook of a refused call was asked for variates')


def test_bert_entry_points_refuse_before_any_device_work(bert):
    """On the CPU the first kernel call raises MMVIDError: a ValueError shows the refusal came first."""
    from mmvid_amd import completion, long_video
    text = torch.randint(1, 49408, (2, TT))
    n, mp = bert.image_seq_len, dict(T=3, B=2)
    control = torch.zeros(2, TT + 2, 768)
    frames = torch.zeros(2, T * n, dtype=torch.long)
    given = torch.zeros(2, T, dtype=torch.bool)
    entries = {
        'generate_images': lambda **kw: bert.generate_images(text, mask_predict_steps=3, mp_config=mp, **kw),
        'mask_predict': lambda **kw: bert.mask_predict(control, steps=3, mp_config=mp, **kw),
        'complete_seeded': lambda seeds, **kw: completion.complete_seeded(bert, text, frames, given, seeds, mp_config=mp, **kw),
        'generate_long_seeded': lambda seeds, **kw: long_video.generate_long_seeded(bert, text, seeds, mp_config=mp, t_repeat=2, **kw),
    }
    for name, entry in entries.items():
        for seeds, word in BAD:
            with pytest.raises(ValueError, match=word):
                entry(seeds=seeds)
        with pytest.raises(ValueError, match='_race'):
            entry(seeds=[1, 2], _race=hook)
        if name != 'mask_predict':  # (mask_predict takes the finished control rows: it has no erase_visual)
            with pytest.raises(ValueError, match='erase_visual'):
                entry(seeds=[1, 2], erase_visual=True)


def test_artv_entry_points_refuse_before_any_device_work(artv):
    from mmvid_amd import completion, long_video
    text = torch.randint(1, 49408, (2, TT))
    n = artv.image_seq_len
    vis = torch.zeros(2, n, dtype=torch.long)
    frames = torch.zeros(2, T * n, dtype=torch.long)
    given = torch.tensor([1, 0, 0, 0], dtype=torch.bool)
    entries = {
        'generate_images': lambda **kw: artv.generate_images(text, visual=vis, **kw),
        'sample_tokens': lambda **kw: artv.sample_tokens(text, visual=vis, **kw),
        'complete_artv': lambda **kw: completion.complete_artv(artv, text, frames, given, visual=vis, **kw),
        'generate_long_artv': lambda **kw: long_video.generate_long_artv(artv, text, visual=vis, t_repeat=2, **kw),
    }
    for name, entry in entries.items():
        for seeds, word in BAD:
            with pytest.raises(ValueError, match=word):
                entry(seeds=seeds)
        with pytest.raises(ValueError, match='_race'):
            entry(seeds=[1, 2], _race=hook)
        with pytest.raises(ValueError, match='erase_visual'):
            entry(seeds=[1, 2], erase_visual=True)


# ---------------------------------------------------------------------------------------------------- long-video substreams
def test_window_substream_is_a_function_of_the_plan_alone():
    from mmvid_amd import long_video as lv
    assert lv.window_substream(0, 0) == 0 and lv.window_substream(0, 5) == 5 and lv.window_substream(3, 2) == (3 << 16) | 2
    ids = {lv.window_substream(li, w) for li in range(6) for w in range(40)}
    assert len(ids) == 240 and max(lv.window_substream((1 << 15) - 1, (1 << 16) - 1), *ids) < 2**31  # distinct, int32
    for level, window in ((-1, 0), (0, -1), (1 << 15, 0), (0, 1 << 16)):
        with pytest.raises(ValueError):
            lv.window_substream(level, window)
    # what a (video, window) pair of a level draws from, whatever b the video sits in and however the level's rows are chunked
    seeds = [11, 22, 33, 44, 55]
    levels = lv.plan('interp', 4, 3)

    def streams(videos, max_rows):
        b, got = len(videos), {}
        for li, lev in enumerate(levels):
            rows = len(lev.windows) * b
            step = rows if not max_rows else max_rows
            for r0 in range(0, rows, step):
                sd, sub = lv.row_streams([seeds[v] for v in videos], li, (r0, min(rows, r0 + step)), b)
                for r, s, u in zip(range(r0, rows), sd, sub):
                    got[(videos[r % b], li, r // b)] = (s, u)
        return got

    whole = streams([0, 1, 2, 3, 4], None)
    assert whole[(2, 2, 3)] == (33, lv.window_substream(2, 3)) and len(whole) == 5 * (1 + 2 + 4)
    for videos, max_rows in (([0, 1, 2, 3, 4], 3), ([0, 1, 2, 3, 4], 1), ([2], None), ([4, 2], 3), ([1, 3, 0], 2)):
        part = streams(videos, max_rows)
        assert part == {k: v for k, v in whole.items() if k[0] in videos}, (videos, max_rows)


# --------------------------------------------------------------------------------------------------------- the replica
def test_replica_block_layout_with_rows_that_start_inside_a_philox_block():
    """5 rows of 3 per video: rows start at i = 0, 3, 6, 9, 12, of which only 0 and 12 are block starts.  Every element against a
    scalar call of Philox per element."""
    seeds, sub = [7, (0x9E3779B9 << 32) | 5, 2**63 - 1], [0, 4, 1 << 20]
    rpv, n, purpose, d0, draws = 5, 3, R.KEEP_RACE, 1023, 2
    got = R.block_words(seeds, sub, rpv, n, purpose, d0, draws)
    assert got.shape == (draws, 3 * rpv, n)
    for k in range(draws):
        for r in range(3 * rpv):
            v = r // rpv
            for c in range(n):
                i = (r % rpv) * n + c
                w = philox4x32_10(i >> 2, purpose, sub[v], d0 + k, seeds[v] & 0xFFFFFFFF, seeds[v] >> 32)[i & 3]
                assert int(got[k, r, c]) == int(w) >> 8, (k, r, c)
    assert [((r % rpv) * n) % 4 for r in range(rpv)] == [0, 3, 2, 1, 0]
    # a video's block does not depend on where it sits, and the mappings are what the header says
    alone = R.block_words([seeds[1]], [sub[1]], rpv, n, purpose, d0 + 1, 1)
    assert np.array_equal(alone[0], got[1, rpv:2 * rpv])
    w24 = np.array([0, 1, 2**24 - 1], np.uint64)
    assert R.uniform_of(w24).tolist() == [0.0, 2.0**-24, 1.0 - 2.0**-24] and R.uniform_of(w24).dtype == np.float32
    assert R.exp1_argument(w24).tolist() == [2.0**-24, 2.0**-23, 1.0] and R.exp1_of(w24)[2] == 0.0
    assert abs(R.exp1_of(w24)[0] - 24 * np.log(2.0)) < 1e-12
    assert R.ulp32(np.array([1.0, 1.5, 2.0, 16.6, 0.0])).tolist() == [2.0**-23, 2.0**-23, 2.0**-22, 2.0**-19, 2.0**-149]
