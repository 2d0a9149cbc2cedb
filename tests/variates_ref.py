"""Host replica (numpy) of the seeded race variates of csrc/variates.hip, written from include/mmvid_hip_ext.h.

Variate i of the block that video seed s owns for (purpose, substream, draw) is word i & 3 of
Philox4x32-10(counter = {i >> 2, purpose, substream, draw}, key = {lo32(s), hi32(s)}); uniform = (w >> 8) * 2^-24, Exp(1) =
-log(((w >> 8) + 1) * 2^-24).  Philox itself is tests/frontend_ref.py's, pinned there to the Random123 known answers.  A plain helper:
no fixtures, no pytest settings."""
import numpy as np

from frontend_ref import philox4x32_10

U64 = np.uint64
TOKEN_RACE, TOKEN_NOISE, KEEP_RACE = 1, 2, 3
UNIFORM, EXP1 = 0, 1


def words(seed, purpose, substream, draw, count, first=0):
    """The 24-bit integers w >> 8 of variates first .. first + count - 1 of one block -> uint64 [count]."""
    i = np.arange(first, first + count, dtype=U64)
    seed = int(seed)
    r = philox4x32_10(i >> U64(2), purpose, int(substream) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    lane = i & U64(3)
    w = np.where(lane == 0, r[0], np.where(lane == 1, r[1], np.where(lane == 2, r[2], r[3])))
    return w >> U64(8)


def uniform_of(w24):
    """float32 (w >> 8) * 2^-24: exact."""
    return w24.astype(np.float32) * np.float32(2.0**-24)


def exp1_argument(w24):
    """((w >> 8) + 1) * 2^-24 in fp64: exact, and exactly the fp32 the kernel hands to logf."""
    return (w24 + U64(1)).astype(np.float64) * 2.0**-24


def exp1_of(w24):
    """-log of the argument, in fp64: what the device value is measured against."""
    return -np.log(exp1_argument(w24))


def block_words(seeds, substream, rows_per_video, n, purpose, draw_first, draws):
    """The layout of mmvid_variates_fill: w >> 8 of out[draws][videos * rows_per_video][n] -> uint64 of that shape.  Row r belongs to
    video r // rows_per_video and element (r, c) is variate (r % rows_per_video) * n + c of that video: a video's rows are ONE run of
    rows_per_video * n consecutive variates, so a row starts wherever the row before ended, inside a Philox block or not."""
    videos = len(seeds)
    substream = [0] * videos if substream is None else substream
    out = np.empty((draws, videos * rows_per_video, n), U64)
    for k in range(draws):
        for v in range(videos):
            out[k, v * rows_per_video:(v + 1) * rows_per_video] = words(seeds[v], purpose, substream[v], draw_first + k,
                                                                        rows_per_video * n).reshape(rows_per_video, n)
    return out


def ulp32(x):
    """The fp32 unit in the last place at the magnitude of the fp64 values x, as OpenCL defines it for an infinitely precise result:
    2^(floor(log2 |x|) - 23), and 2^-149 below the normal range."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0**-126)))
    return np.maximum(2.0**(e - 23), 2.0**-149)
