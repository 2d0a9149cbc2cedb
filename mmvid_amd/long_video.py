"""Long videos: extrapolation and interpolation on the batched sampler (utils/utils_train.py:1221-1527, `test.py --eval_mode long`).

The reference chains `generate_images` calls, one window of `num_targets` frames at a time at batch 1, and decodes every window:

    long         the last t_overlap frames of a clip are the first frames of the next clip (1337-1373)
    interp       level t doubles the frame count: window tt is given frames [tt T/2, (tt+1) T/2) of the previous level's timeline
                 in its even slots and fills the odd ones (1374-1432)
    interp_real  the same from real frames, with windows of T/2 given frames at a stride of T/4: a window passes its first T/2
                 frames on, the last window T - 1 (1433-1527)

Here `plan` restates that index arithmetic as data and touches no device, `run` walks a plan with any sampler, and `generate_long`
is the runner on a BERT: inside a level no window reads another window of that level, so a level of W windows goes through
`BERT.mask_predict` as ONE call of b * W rows (row = window * b + video) instead of W calls.  The sampler's result for a video does not
depend on its batch mates (tests/test_parity_gpu.py), so the batched level equals the chained windows token for token.  Only the final
token timeline is decoded, once, and leaves the device as bytes (csrc/frames.hip).
"""
import os
from collections import namedtuple

import torch

from . import ops, seeded

# given: (start, stop) frames of the previous level's timeline handed to the window, None = nothing; passes / emits: (start, stop)
# frames of the window's own T frames that go into the next level's timeline / into the output
Window = namedtuple('Window', 'given passes emits')
# long_mode, t_overlap: what the sampler is called with (the interp modes do not read t_overlap; the reference passes the level number)
Level = namedtuple('Level', 'windows long_mode t_overlap')

MODES = ('long', 'interp', 'interp_real')
# rows per sampler call unless the caller says otherwise: at full size the time per window still falls up to 64 rows, the largest call
# measured (8 / 16 / 32 / 64 rows: 45.1 / 29.1 / 27.0 / 26.7 ms per 8-video window, profiles/long_video_levels.log)
MAX_ROWS = 64


def plan(mode, num_targets, t_repeat, t_overlap=1):
    """-> list of Level.  The output timeline is every window's `emits`, levels and windows in order."""
    T, r = int(num_targets), int(t_repeat)
    if mode not in MODES:
        raise ValueError(f'mode={mode!r}: expected one of {MODES}')
    if T < 1 or r < 1:
        raise ValueError(f'num_targets={num_targets}, t_repeat={t_repeat}: both must be at least 1')
    none = (0, 0)
    if mode == 'long':
        o = int(t_overlap)
        if not 1 <= o <= T - 1:  # (0: the reference's preserve[:, -0:] is the whole clip; T: nothing is left to generate)
            raise ValueError(f't_overlap={t_overlap}: mode "long" needs 1 <= t_overlap <= num_targets - 1 = {T - 1}')
        # 1342-1360: every clip is handed the whole previous clip and the sampler keeps its last `o` frames
        return [Level([Window(None if k == 0 else (0, T), (0, T), (0, T) if k == 0 else (o, T))], 'long', 0 if k == 0 else o)
                for k in range(r)]
    if T % 2:
        raise ValueError(f'num_targets={T}: mode "{mode}" fills every other frame and needs an even frame count')
    levels = []
    if mode == 'interp':
        for t in range(r):  # 1376-1430
            emits = (0, T) if t == r - 1 else none
            levels.append(Level([Window(None if t == 0 else (tt * (T // 2), (tt + 1) * (T // 2)), (0, T), emits)
                                 for tt in range(2**t)], 'interp', t))
        return levels
    if T % 4:
        raise ValueError(f'num_targets={T}: mode "interp_real" strides its windows by num_targets / 4')
    if r < 2:
        raise ValueError(f't_repeat={t_repeat}: mode "interp_real" generates nothing below 2 (its loop starts at level 1)')
    curr_len = T
    for t in range(1, r):  # 1440-1524
        last_tt = (curr_len - T // 2) // (T // 4)
        curr_len = last_tt * T // 2 + T - 1
        wins = []
        for tt in range(last_tt + 1):
            keep = (0, T - 1) if tt == last_tt else (0, T // 2)
            wins.append(Window((tt * (T // 4), tt * (T // 4) + T // 2), keep, keep if t == r - 1 else none))
        levels.append(Level(wins, 'interp_real', t))
    return levels


def window_substream(level, window):
    """The substream of seeded sampling that belongs to window `window` of level `level` of a plan: (level << 16) | window, an int32.
    It is the one statement of that id.  A level's sampler rows are (window, video) pairs, row = window * b + video; under `seeds` row
    r draws from the streams of (seed of video r % b, substream of window r // b) -- a function of the plan alone, not of b, of
    `max_rows` or of the chunk a row falls into.  Level 0, window 0 is substream 0, the substream of a call outside this module: the
    first clip of a long video is the clip generate_images makes from the same seed."""
    level, window = int(level), int(window)
    if not (0 <= level < 1 << 15 and 0 <= window < 1 << 16):
        raise ValueError(f'window_substream: level {level} / window {window} outside [0, 2^15) / [0, 2^16)')
    return (level << 16) | window


def row_streams(seeds, level, rows, b):
    """(seeds, substreams) of sampler rows [rows[0], rows[1]) of a level, row = window * b + video: two host lists."""
    return ([seeds[r % b] for r in range(rows[0], rows[1])], [window_substream(level, r // b) for r in range(rows[0], rows[1])])


def frames_out(levels):
    """Length of the output timeline of a plan."""
    return sum(w.emits[1] - w.emits[0] for lev in levels for w in lev.windows)


def run(levels, sample, *, b, num_targets, mask_id, start=None, max_rows=None, trace=None):
    """Walk a plan.  `sample(level, chunk, (row0, row1), preserve, long_mode, t_overlap)` -> tokens [row1 - row0, T * n] int64 is the
    sampler of rows [row0, row1) of a level, row = window * b + video; `preserve` is None or those rows in the reference's calling
    convention: [(rows T), n] for 'long', [rows, T * n] for the interp modes with the given half first and `mask_id` behind.
    `start` [b, F0, n]: the timeline before the first level (interp_real's real tokens).  `max_rows`: rows per call of `sample`.
    `trace` (a list) receives per level dict(level, windows, rows=[(row0, row1) per chunk], timeline=[b, F, n] passed on).
    -> tokens [b, F, n]."""
    T = int(num_targets)
    prev, out = start, []
    for li, lev in enumerate(levels):
        W = len(lev.windows)
        rows = W * b
        preserve = None
        if lev.windows[0].given is not None:
            given = torch.stack([prev[:, g0:g1] for (g0, g1), _, _ in lev.windows])  # [W, b, G, n]
            n = given.shape[-1]
            if lev.long_mode == 'long':
                preserve = given.reshape(rows * T, n)
            else:
                preserve = torch.full((rows, T, n), mask_id, dtype=given.dtype, device=given.device)
                preserve[:, :T // 2] = given.reshape(rows, T // 2, n)
                preserve = preserve.view(rows, T * n)
        step = rows if not max_rows else max(1, int(max_rows))
        per = T if lev.long_mode == 'long' else 1  # rows of `preserve` per sampler row
        chunks, toks = [], []
        for ci, r0 in enumerate(range(0, rows, step)):
            r1 = min(rows, r0 + step)
            p = None if preserve is None else preserve[r0 * per:r1 * per]
            tok = sample(li, ci, (r0, r1), p, lev.long_mode, lev.t_overlap)
            toks.append(tok.reshape(r1 - r0, T, -1))
            chunks.append((r0, r1))
        tok = (toks[0] if len(toks) == 1 else torch.cat(toks)).reshape(W, b, T, -1)
        prev = torch.cat([tok[w][:, p0:p1] for w, (_, (p0, p1), _) in enumerate(lev.windows)], dim=1)
        out += [tok[w][:, e0:e1] for w, (_, _, (e0, e1)) in enumerate(lev.windows) if e1 > e0]
        if trace is not None:
            trace.append(dict(level=li, windows=W, rows=chunks, timeline=prev))
    return torch.cat(out, dim=1).contiguous()


def bert_sampler(model, text, *, visual=None, mask_predict_steps=0, mp_config=None, dynamic=True, erase_visual=False, vc_mode=None,
                 face_mode=None, seen=None, seeds=None, _race=None):
    """The `sample` of `run` on a BERT (in eval mode, under no_grad): control rows for rows [row0, row1) of a level, then ONE
    `mask_predict` call for them.  Control rows are computed once per video and repeated when nothing random enters them
    (`erase_visual` false and `vc_mode` None); otherwise per window with one forward each, as the reference's generate_images makes
    one per window (erase_codebook_face draws once per call: every window draws its own region).  `seen` (a dict) receives per level
    (rows whose control sequence was computed, control rows of the last chunk).  `seeds` (check_seeds' list, one per video): every row
    draws from its video's seed and its window's substream (row_streams)."""
    b, dev = text.shape[0], text.device
    fixed_control = not erase_visual and vc_mode is None
    ctl = dict(erase_visual=erase_visual, erase_visual_half=True, vc_mode=vc_mode, face_mode=face_mode, return_loss=False)
    base = model(text, visual=visual, **ctl) if fixed_control else None
    per_window = {}

    def sample(level, chunk, rows, preserve, long_mode, overlap):
        index = torch.arange(rows[0], rows[1], device=dev)
        if fixed_control:
            control, computed = base.index_select(0, index % b), (b if level == 0 and chunk == 0 else 0)
        else:
            w0, w1 = rows[0] // b, (rows[1] - 1) // b + 1
            for key in [k for k in per_window if k[0] != level or k[1] < w0]:  # (a window that a chunk boundary cuts is kept)
                del per_window[key]
            computed = 0
            for w in range(w0, w1):
                if (level, w) not in per_window:
                    per_window[(level, w)] = model(text, visual=visual, **ctl)
                    computed += b
            control = torch.cat([per_window[(level, w)] for w in range(w0, w1)]).index_select(0, index - w0 * b)
        if seen is not None:
            seen[level] = (seen.get(level, (0, None))[0] + computed, control)
        race = None if _race is None else (lambda name, shape: _race(f'L{level}c{chunk}/{name}', shape))
        streams = {}
        if seeds is not None:
            streams['seeds'], streams['_substream'] = row_streams(seeds, level, rows, b)
        return model.mask_predict(control, dynamic=dynamic, steps=mask_predict_steps, preserve=preserve, t_overlap=overlap,
                                  mp_config=mp_config, long_mode=long_mode, _race=race, **streams)[0]

    return sample


@torch.no_grad()
def generate_long(model, text, *, visual=None, mode='long', t_repeat=10, t_overlap=1, real_frames=None, which_vae='vae',
                  mask_predict_steps=0, mp_config=None, dynamic=True, erase_visual=False, vc_mode=None, face_mode=None, decode=True,
                  max_rows=MAX_ROWS, trace=None, _race=None):
    """`generate_long_seeded` without seeds: the variates come from torch's device generator (or from `_race`).  Its signature is pinned
    by tests/test_artv_completion_host.py, which is why the seeded call has a name of its own."""
    return generate_long_seeded(model, text, None, visual=visual, mode=mode, t_repeat=t_repeat, t_overlap=t_overlap, real_frames=real_frames,
                                which_vae=which_vae, mask_predict_steps=mask_predict_steps, mp_config=mp_config, dynamic=dynamic,
                                erase_visual=erase_visual, vc_mode=vc_mode, face_mode=face_mode, decode=decode, max_rows=max_rows,
                                trace=trace, _race=_race)


@torch.no_grad()
def generate_long_seeded(model, text, seeds, *, visual=None, mode='long', t_repeat=10, t_overlap=1, real_frames=None, which_vae='vae',
                         mask_predict_steps=0, mp_config=None, dynamic=True, erase_visual=False, vc_mode=None, face_mode=None,
                         decode=True, max_rows=MAX_ROWS, trace=None, _race=None):
    """utils_train.py:1337-1526 on a BERT -> (frames_u8 [b, F, H, W, 3] uint8 on the device, or None without `decode`;
    tokens [b, F, image_seq_len] int64).  `text`: [b, text_seq_len] ids, or [b, text_feature_dim] features with a fixed language
    model.  `real_frames` [b, T, 3, H, W] in [0, 1]: the frames mode 'interp_real' starts from.  `max_rows`: rows per sampler call
    (a level of more rows runs in consecutive chunks, in row order; None: no cap).  `_race(name, shape)` supplies the sampler's variates, names
    prefixed with 'L{level}c{chunk}/'.  `trace` (a list): per level the dict of `run` plus `control_rows`, the rows whose control
    sequence (text, visual tokens) was computed -- b per call when nothing random enters it, every row otherwise, each window then
    drawing its own erasure as the reference does by calling forward per window -- and `control`, the control rows of its last chunk.
    `seeds` (a sequence or integer tensor of b values in [0, 2^63), one per video): every window of a video draws from the video's
    seed and the window's own substream (window_substream), whatever b and max_rows are.  Refused with `_race` and erase_visual.  None:
    the unseeded call, which is `generate_long`."""
    if mp_config is None:
        raise ValueError('generate_long: mp_config is required (the schedules of mask-predict, args.mp_config of the reference)')
    seeds = seeded.check_seeds(seeds, text.shape[0], race=_race, erase_visual=erase_visual)
    T, n = model.num_targets, model.image_seq_len
    levels = plan(mode, T, t_repeat, t_overlap)
    b, dev = text.shape[0], text.device
    if isinstance(visual, (list, tuple)):  # frames [b, 3, H, W] each, as get_image_tokens takes them
        visual = torch.stack(list(visual), dim=1) if len(visual) else None
    was_training = model.training
    model.eval()
    try:
        start = None
        if mode == 'interp_real':
            if real_frames is None or tuple(real_frames.shape[:2]) != (b, T):
                raise ValueError(f'mode "interp_real" needs real_frames [b, num_targets, 3, H, W] = [{b}, {T}, ...]')
            start = model.get_image_tokens(real_frames, reshape=True, which_vae=which_vae).view(b, T, n)
        seen = {} if trace is not None else None
        sample = bert_sampler(model, text, visual=visual, mask_predict_steps=mask_predict_steps, mp_config=mp_config, dynamic=dynamic,
                              erase_visual=erase_visual, vc_mode=vc_mode, face_mode=face_mode, seen=seen, seeds=seeds, _race=_race)
        own = [] if trace is not None else None
        tokens = run(levels, sample, b=b, num_targets=T, mask_id=model.image_token_lut['[MASK]'], start=start, max_rows=max_rows,
                     trace=own)
        if trace is not None:
            for rec in own:
                rec['control_rows'], rec['control'] = seen[rec['level']]
            trace += own
        frames = None
        if decode:
            F, s = tokens.shape[1], model.image_size
            flat = tokens.view(b * F, n)
            frames = torch.empty(b * F, s, s, 3, device=dev, dtype=torch.uint8)
            step = model.vae._max_frames(s)
            for i in range(0, b * F, step):
                ops.frames_to_u8(model.vae.decode(flat[i:i + step]), frames[i:i + step])
            frames = frames.view(b, F, s, s, 3)
        return frames, tokens
    finally:
        model.train(was_training)


def artv_sampler(model, text, *, visual=None, seeds=None, _race=None, **sampling_kw):
    """The `sample` of `run` on an ART-V model (dalle_artv.DALLE, in eval mode) for mode 'long': the last `t_overlap` frames of
    `preserve` (the previous clip) are the known first frames of the next clip, which enter through the prefill
    (DALLE.sample_tokens(given=...)); the first clip is a plain call.  `sampling_kw`: the sampling keywords of generate_images.  The
    interp modes hand a window frames that lie AFTER the ones it generates, which a causal model cannot use: ValueError.  `seeds`: as
    for bert_sampler."""
    b = text.shape[0]
    T, n = model.num_targets, model.image_seq_len

    def sample(level, chunk, rows, preserve, long_mode, overlap):
        if long_mode != 'long':
            raise ValueError(f'long_mode={long_mode!r}: an ART-V model extrapolates only (mode "long"); interpolation conditions on later frames')
        index = torch.arange(rows[0], rows[1], device=text.device) % b
        whole = rows[1] - rows[0] == b and rows[0] % b == 0
        t = text if whole else text.index_select(0, index)
        v = visual if whole or visual is None else visual.index_select(0, index.to(visual.device))
        given = None
        if preserve is not None:
            o = int(overlap)
            mask = torch.tensor([1] * o + [0] * (T - o), dtype=torch.uint8)
            tokens = torch.zeros(rows[1] - rows[0], T * n, dtype=torch.long, device=preserve.device)
            tokens[:, :o * n] = preserve.reshape(rows[1] - rows[0], T, n)[:, T - o:].reshape(-1, o * n)
            given = (mask, tokens)
        race = None if _race is None else (lambda name, shape: _race(f'L{level}c{chunk}/{name}', shape))
        streams = {}
        if seeds is not None:
            streams['seeds'], streams['_substream'] = row_streams(seeds, level, rows, b)
        return model.sample_tokens(t, visual=v, given=given, _race=race, **streams, **sampling_kw)[1]

    return sample


@torch.no_grad()
def generate_long_artv(model, text, *, visual=None, mode='long', t_repeat=10, t_overlap=1, decode=True, max_rows=MAX_ROWS, trace=None,
                       seeds=None, _race=None, **sampling_kw):
    """Long extrapolation on an ART-V model -> (frames_u8 [b, F, H, W, 3] uint8 on the device, or None without `decode`; tokens
    [b, F, image_seq_len] int64): clip k + 1 continues the last `t_overlap` frames of clip k (plan / run of mode 'long', one window per
    level).  The interp modes raise ValueError: they need the future.  `sampling_kw`: the sampling keywords of generate_images;
    `_race(name, shape)` supplies the variates, names prefixed with 'L{level}c{chunk}/'.  `trace` (a list): the dicts of `run`.
    `seeds`: as for generate_long_seeded (clip k of a video draws from substream window_substream(k, 0))."""
    if mode in MODES and mode != 'long':
        raise ValueError(f'mode={mode!r}: an ART-V model extrapolates only (mode "long"); the interp modes condition a window on frames '
                         'that come after the ones it generates')
    seeds = seeded.check_seeds(seeds, text.shape[0], race=_race, erase_visual=sampling_kw.get('erase_visual', False))
    T, n = model.num_targets, model.image_seq_len
    levels = plan(mode, T, t_repeat, t_overlap)
    b, dev = text.shape[0], text.device
    if isinstance(visual, (list, tuple)):  # frames [b, 3, H, W] each, as get_image_tokens takes them
        visual = torch.stack(list(visual), dim=1) if len(visual) else None
    was_training = model.training
    model.eval()
    try:
        sample = artv_sampler(model, text, visual=visual, seeds=seeds, _race=_race, **sampling_kw)
        tokens = run(levels, sample, b=b, num_targets=T, mask_id=-1, max_rows=max_rows, trace=trace)
        frames = None
        if decode:
            F, s = tokens.shape[1], model.image_size
            flat = tokens.view(b * F, n)
            frames = torch.empty(b * F, s, s, 3, device=dev, dtype=torch.uint8)
            step = model.vae._max_frames(s)
            for i in range(0, b * F, step):
                ops.frames_to_u8(model.vae.decode(flat[i:i + step]), frames[i:i + step])
            frames = frames.view(b, F, s, s, 3)
        return frames, tokens
    finally:
        model.train(was_training)


def save(frames_u8, path, video_format='gif', fps=4):
    """One video [F, H, W, 3] uint8 (device or host; `generate_long(...)[0][i]`) -> `<path>.gif`, or `<path>.mp4` (Motion-JPEG,
    data.write_mjpeg_mp4) with video_format='mp4'.  The bytes are written as they are.  Returns the file name, as
    data.save_image_tensor does."""
    from PIL import Image

    from .data import write_mjpeg_mp4
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f'save: expected one video [F, H, W, 3] uint8, got {tuple(frames_u8.shape)} {frames_u8.dtype}')
    if video_format not in ('gif', 'mp4'):
        raise ValueError(f'video_format={video_format!r}: expected "gif" or "mp4"')
    u8 = frames_u8.detach().cpu().contiguous()
    out = f'{path}.{video_format}'
    if video_format == 'gif':
        frames = [Image.fromarray(f.numpy()) for f in u8]
        frames[0].save(out, save_all=True, append_images=frames[1:], duration=int(1000 / fps), loop=0)
    else:
        write_mjpeg_mp4(out, u8, fps=fps)
    return os.path.basename(out)
