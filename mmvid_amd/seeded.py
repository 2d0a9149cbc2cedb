"""Seeded sampling: per-video seeds for both samplers (the `seeds=` keyword of generate_images and its relatives).

The samplers ask a hook `(name, shape) -> tensor` for their random tensors -- `tok{t}` (the Exp(1) token race), `tok{t}_noise_u` (the
uniforms of the Gumbel noise) and `keep{t}` (the Exp(1) keep race of mask-predict) -- and draw them from torch's device generator when
there is none.  SeededRace is such a hook whose tensors are filled on the device by csrc/variates.hip as a pure function of (video
seed, purpose, draw number t, index within the video's block, and for long videos the window): what a video draws does not depend on
its row, on the batch size, on its batch mates or on anything drawn before in the process.  include/mmvid_hip_ext.h states the
function; INTEGRATION.md, "Seeded sampling", states what follows from it for the tokens.  torch's generator is neither read nor
advanced."""
import re

import numpy as np
import torch

from . import ops

_NAME = re.compile(r'(tok|keep)(\d+)(_noise_u)?')
SEED_BOUND = 1 << 63


def parse_name(name):
    """A sampler's tensor name -> (purpose, kind, draw number): tok{t} -> (1, Exp(1), t), tok{t}_noise_u -> (2, uniform, t), keep{t} ->
    (3, Exp(1), t).  Anything else is a ValueError."""
    m = _NAME.fullmatch(name)
    if not m or (m.group(1) == 'keep' and m.group(3)):
        raise ValueError(f'seeded sampling: no stream is defined for the tensor name {name!r} (known: tok<t>, tok<t>_noise_u, keep<t>)')
    if m.group(3):
        return ops.VARIATE_PURPOSES['noise'], 0, int(m.group(2))
    return ops.VARIATE_PURPOSES[m.group(1)], 1, int(m.group(2))


def check_seeds(seeds, b, *, race=None, erase_visual=False):
    """The argument rules of `seeds`, before any device work -> a host list of b ints, or None for the unseeded call.  Accepted: a
    sequence or an integer tensor of b values in [0, 2^63), one per video (a bool is no integer here, as for top_k).  Refused
    together with `_race` (two sources for the same tensors) and with erase_visual=True (the erasure is drawn by the front end from
    its own device state, outside what a seed determines)."""
    if seeds is None:
        return None
    if race is not None:
        raise ValueError('seeds together with _race: both supply the same variates')
    if erase_visual:
        raise ValueError("seeds with erase_visual=True: the erasure of the visual tokens is drawn from the front end's own device state, "
                         'which a seed does not determine')
    if torch.is_tensor(seeds):
        if seeds.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) or seeds.dim() != 1:
            raise ValueError(f'seeds: a tensor must be one-dimensional and of an integer type, got {seeds.dtype} {tuple(seeds.shape)}')
        vals = seeds.tolist()
    elif isinstance(seeds, np.ndarray):
        if seeds.dtype.kind not in 'iu' or seeds.ndim != 1:
            raise ValueError(f'seeds: an array must be one-dimensional and of an integer type, got {seeds.dtype} {seeds.shape}')
        vals = [int(v) for v in seeds]
    elif isinstance(seeds, (list, tuple)):
        vals = list(seeds)
    else:
        raise ValueError(f'seeds: expected a sequence or an integer tensor of {b} values, one per video, got {type(seeds).__name__}')
    if len(vals) != b:
        raise ValueError(f'seeds: one per video, {b} values, got {len(vals)}')
    for v in vals:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < SEED_BOUND:
            raise ValueError(f'seeds: expected integers in [0, 2^63), got {v!r}')
    return [int(v) for v in vals]


def layout(shape, videos):
    """The shape a sampler asks for -> (rows per video, n): the last axis holds n variates, the axes in front of it are rows, and
    every video owns the same number of consecutive rows.  (b * nb * TS, V) -> nb * TS rows of V; (b, Bm, TS) -> Bm rows of TS;
    ART-V's (B, V) -> one row of V."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2:
        raise ValueError(f'seeded sampling: a shape needs a row axis and a variate axis, got {shape}')
    rows = int(np.prod(shape[:-1]))
    if videos < 1 or rows % videos:
        raise ValueError(f'seeded sampling: {rows} rows of shape {shape} do not divide among {videos} videos')
    return rows // videos, shape[-1]


class SeededRace:
    """`race(name, shape)` for `len(seeds)` videos -> the tensor, filled by one launch.  seeds: what check_seeds returned (or a device
    int64 tensor); substream: one int per video (None: 0), see long_video.window_substream."""

    def __init__(self, seeds, device, substream=None):
        self.seeds = seeds.to(device) if torch.is_tensor(seeds) else torch.tensor(list(seeds), dtype=torch.int64, device=device)
        self.substream = None
        if substream is not None:
            self.substream = (substream.to(device) if torch.is_tensor(substream) else
                              torch.tensor(list(substream), dtype=torch.int32, device=device))
            if self.substream.shape != self.seeds.shape:
                raise ValueError(f'substream: one per video, {self.seeds.shape[0]} values, got {tuple(self.substream.shape)}')
        self.videos, self.device = self.seeds.shape[0], device

    def __call__(self, name, shape):
        purpose, kind, draw = parse_name(name)
        rpv, n = layout(shape, self.videos)
        out = torch.empty(tuple(shape), device=self.device, dtype=torch.float32)
        ops.variates_fill(out.view(-1, n), self.seeds, rpv, purpose, kind, draw_first=draw, substream=self.substream)
        return out

    def fill(self, out, purpose, kind, draw_first=0, draw_dev=None):
        """Into a caller's buffer: [R, n] (one draw: number draw_first, plus the device scalar draw_dev when given) or [draws, R, n]
        (draws draw_first ..), one launch."""
        return ops.variates_fill(out, self.seeds, out.shape[-2] // self.videos, purpose, kind, draw_first=draw_first, draw_dev=draw_dev,
                                 substream=self.substream)

    def rows(self, index):
        """The hook of a subset of the videos (index: a list of rows, or an int64 tensor on the device)."""
        index = index if torch.is_tensor(index) else torch.tensor(list(index), dtype=torch.long, device=self.device)
        return SeededRace(self.seeds.index_select(0, index), self.device,
                          None if self.substream is None else self.substream.index_select(0, index))
