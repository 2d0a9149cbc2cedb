"""mmvid_amd/long_video.py without a device: the planner and the runner against the call logs of the reference's own visualize_long
(tests/golden/long_video_plan.npz, tools/make_golden.py::case_long_video), the closed forms, the rejected arguments, chunking, and the
declaration of the new entry point."""
import os
import re
from collections import Counter

import pytest
import torch

from conftest import ROOT

N_CASES = 12


class IdSampler:
    """The golden's stand-in for the sampler, on rows: one token per frame, every frame of sampler row r (window r // b in reference call
    order, rows counted across levels and chunks) gets the fresh id (r // b) * T + slot, and preserved ids are placed as
    sampling.preserved_tokens places them.  Logs (level, chunk, rows, preserve, long_mode, t_overlap) per call."""

    def __init__(self, b, T):
        self.b, self.T, self.row0, self.calls = b, T, 0, []

    def __call__(self, level, chunk, rows, preserve, long_mode, t_overlap):
        T, R = self.T, rows[1] - rows[0]
        window = (self.row0 + torch.arange(R)) // self.b
        ids = window[:, None] * T + torch.arange(T)[None, :]
        if preserve is not None:
            if long_mode == 'long':
                assert preserve.shape == (R * T, 1)
                if t_overlap:
                    ids[:, :t_overlap] = preserve.view(R, T)[:, T - t_overlap:]
            else:
                assert preserve.shape == (R, T)
                ids[:, ::2] = preserve[:, :T // 2]
        self.calls.append((level, chunk, rows, None if preserve is None else preserve.reshape(R, T).clone(), long_mode, t_overlap))
        self.row0 += R
        return ids


def run_case(meta, b=1, max_rows=None, trace=None):
    from mmvid_amd import long_video as lv
    T = meta['num_targets']
    levels = lv.plan(meta['mode'], T, meta['t_repeat'], meta['t_overlap'])
    start = None
    if meta['mode'] == 'interp_real':
        start = (900000 + torch.arange(T)).view(1, T, 1).repeat(b, 1, 1)
    s = IdSampler(b, T)
    tokens = lv.run(levels, s, b=b, num_targets=T, mask_id=-1, start=start, max_rows=max_rows, trace=trace)
    return levels, s, tokens


@pytest.mark.parametrize('case', range(N_CASES))
def test_runner_reproduces_the_reference_calls_and_timeline(golden, case):
    g = golden('long_video_plan')
    gm = g.meta
    assert len(gm['cases']) == N_CASES and gm['mask'] == -1
    meta = gm['cases'][case]
    levels, s, tokens = run_case(meta)
    ref_pres, ref_ov, ref_lm = g[f'c{case}_preserve'], g[f'c{case}_t_overlap'], meta['long_mode']
    # the reference's calls, grouped into levels: 'long' chains its calls (one per level); the interp modes pass the level as t_overlap
    key = list(range(len(ref_lm))) if meta['mode'] == 'long' else ref_ov.tolist()
    ref_levels = [[i for i, k in enumerate(key) if k == v] for v in sorted(set(key))]
    assert [len(l) for l in ref_levels] == [len(lev.windows) for lev in levels]
    assert len(s.calls) == len(levels)  # b = 1, no max_rows: one sampler call per level
    for (level, chunk, rows, pres, lm, ov), ref_calls, lev in zip(s.calls, ref_levels, levels):
        assert chunk == 0 and rows == (0, len(ref_calls))

        def as_key(row, mode):
            return (tuple(row.tolist()), mode)

        ours = Counter(as_key(pres[w] if pres is not None else torch.full((meta['num_targets'], ), gm['none']), lm)
                       for w in range(len(ref_calls)))
        theirs = Counter(as_key(ref_pres[i], ref_lm[i]) for i in ref_calls)
        assert ours == theirs, (level, ours, theirs)
        if meta['mode'] == 'long':
            assert all(int(ref_ov[i]) == ov for i in ref_calls)
    assert torch.equal(tokens.view(-1), g[f'c{case}_timeline'])
    from mmvid_amd import long_video as lv
    assert lv.frames_out(levels) == tokens.shape[1]


def test_reference_timeline_of_the_issue(golden):
    g = golden('long_video_plan')
    assert g.meta['cases'][0] == dict(mode='long', num_targets=4, t_repeat=3, t_overlap=1, long_mode=['long'] * 3)
    assert g['c0_timeline'].tolist() == [0, 1, 2, 3, 5, 6, 7, 9, 10, 11]


def test_closed_forms():
    from mmvid_amd import long_video as lv
    for T in (2, 3, 4, 8, 16):
        for r in (1, 2, 3, 5):
            for o in range(1, T):
                levels = lv.plan('long', T, r, o)
                assert lv.frames_out(levels) == T + (r - 1) * (T - o) and len(levels) == r
                assert all(len(l.windows) == 1 for l in levels)
            if T % 2 == 0:
                levels = lv.plan('interp', T, r)
                assert lv.frames_out(levels) == T * 2**(r - 1)
                assert [len(l.windows) for l in levels] == [2**t for t in range(r)]
    # interp_real: stride T/4, width T/2, the last window keeps T - 1 frames
    levels = lv.plan('interp_real', 8, 3)
    assert [len(l.windows) for l in levels] == [3, 6]
    assert [w.given for w in levels[1].windows] == [(2 * i, 2 * i + 4) for i in range(6)]
    assert [w.passes for w in levels[1].windows] == [(0, 4)] * 5 + [(0, 7)]
    assert lv.frames_out(levels) == 27


@pytest.mark.parametrize('args', [('long', 4, 3, 0), ('long', 4, 3, 4), ('long', 4, 3, -1), ('long', 1, 2, 1), ('interp', 3, 2, 1),
                                  ('interp_real', 3, 2, 1), ('interp_real', 6, 2, 1), ('interp_real', 2, 2, 1), ('interp_real', 4, 1, 1),
                                  ('interp_real', 8, 0, 1), ('extrap', 4, 2, 1)])
def test_rejected_arguments(args):
    from mmvid_amd import long_video as lv
    with pytest.raises(ValueError):
        lv.plan(*args)


@pytest.mark.parametrize('mode,T,r,o', [('interp', 4, 3, 1), ('interp_real', 8, 3, 1), ('long', 4, 3, 2)])
def test_max_rows_splits_a_level_in_row_order(mode, T, r, o):
    meta = dict(mode=mode, num_targets=T, t_repeat=r, t_overlap=o)
    b = 2
    whole_trace, split_trace = [], []
    levels, whole, tok_whole = run_case(meta, b=b, trace=whole_trace)
    _, split, tok_split = run_case(meta, b=b, max_rows=3, trace=split_trace)
    assert torch.equal(tok_whole, tok_split)
    assert tok_whole.shape == (b, sum(w.emits[1] - w.emits[0] for l in levels for w in l.windows), 1)
    assert torch.equal(tok_whole[0], tok_whole[1])  # (the stand-in gives both videos of a window the same ids)
    for li, lev in enumerate(levels):
        rows = len(lev.windows) * b
        chunks = [c for c in split.calls if c[0] == li]
        assert [c[1] for c in chunks] == list(range(len(chunks))) and len(chunks) == -(-rows // 3)
        assert [c[2] for c in chunks] == [(r0, min(rows, r0 + 3)) for r0 in range(0, rows, 3)]  # consecutive, in row order
        assert split_trace[li]['rows'] == [c[2] for c in chunks] and whole_trace[li]['rows'] == [(0, rows)]
        (one, ) = [c for c in whole.calls if c[0] == li]
        if one[3] is None:
            assert all(c[3] is None for c in chunks)
        else:
            assert torch.equal(torch.cat([c[3] for c in chunks]), one[3])  # the chunks' rows concatenate to the unchunked row list
        assert torch.equal(split_trace[li]['timeline'], whole_trace[li]['timeline'])


def test_interp_real_keeps_the_real_frames():
    _, _, tokens = run_case(dict(mode='interp_real', num_targets=4, t_repeat=3, t_overlap=1))
    assert tokens.view(-1)[::4].tolist() == [900000, 900001, 900002, 900003]


def test_entry_point_is_declared_and_bound():
    from mmvid_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    assert re.search(r'\bint\s+mmvid_frames_to_u8\s*\(const float\* img, int64_t N, int H, int W, uint8_t\* out, void\* stream\);', hdr)
    assert 'utils_html.py:157-186' in hdr
    assert len(_lib.SIGNATURES['mmvid_frames_to_u8']) == 6
    assert 'frames' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'frames.hip'))
    assert _lib.ABI_VERSION == 3


def test_frames_to_u8_refuses_host_tensors():
    from mmvid_amd import ops
    from mmvid_amd._lib import MMVIDError
    with pytest.raises(MMVIDError):
        ops.frames_to_u8(torch.zeros(1, 3, 16, 16))


def test_save_takes_bytes_only(tmp_path):
    from mmvid_amd import long_video as lv
    with pytest.raises(ValueError):
        lv.save(torch.zeros(3, 16, 16, 3), tmp_path / 'x')
    with pytest.raises(ValueError):
        lv.save(torch.zeros(3, 16, 16, 3, dtype=torch.uint8), tmp_path / 'x', video_format='avi')
