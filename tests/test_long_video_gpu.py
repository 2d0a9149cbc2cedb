"""Long videos on the device (mmvid_amd/long_video.py, csrc/frames.hip): the byte kernel bit for bit through guarded buffers, batched
levels against the reference's chain of per-window generate_images calls on the same variates (no tolerance), chunking, the structure
of the three modes, the frames and the files, and the visual control."""
import re

import pytest
import torch

from guarded import Guarded, call_abi, report_mismatch
from test_host_logic import tiny_vae

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, T, N_TOK = 2, 4, 16  # videos, num_targets, tokens per 64 x 64 frame


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _planted(shape, gen):
    """Uniform in [-0.25, 1.25] with the values planted at which a wrong quantisation shows: every k / 255 and its fp32 neighbours (a
    fused multiply-add, a rounding conversion or a reciprocal trick moves one of them across an integer), signed zero, +-inf, 0, 1."""
    x = torch.rand(shape, generator=gen) * 1.5 - 0.25
    k = torch.arange(256, dtype=torch.float32) / 255
    below, above = torch.nextafter(k, torch.tensor(-1.0)), torch.nextafter(k, torch.tensor(2.0))
    special = torch.tensor([-0.0, 0.0, 1.0, float('inf'), float('-inf')])
    plant = torch.cat((k, below, above, special))
    flat = x.view(-1)
    assert flat.numel() >= 2 * plant.numel()
    where = torch.randperm(flat.numel(), generator=gen)[:plant.numel()]
    flat[where] = plant
    flat[:plant.numel()] = plant  # and once as a contiguous run: all four lanes of a 16-byte load and every channel plane see them
    return x


@pytest.mark.parametrize('N,H,W', [(3, 16, 16), (2, 64, 64), (1, 16, 48)])
def test_frames_to_u8_bit_for_bit(N, H, W):
    gen = torch.Generator().manual_seed(1000 * N + H + W)
    x = _planted((N, 3, H, W), gen)
    want = (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    gin = Guarded(x.view(N * 3, H * W), role='in')
    # (a byte has no value to spare for a sentinel: the window starts as the complement of what is expected, so an element that was
    # never stored differs from it; outside the window the guards hold the sentinel as usual)
    gout = Guarded(base=(want ^ 0xFF).view(N * H, W * 3))
    call_abi('mmvid_frames_to_u8', gin.ptr, N, H, W, gout.ptr)
    gin.check('frames_to_u8 img')
    got = gout.check('frames_to_u8 out').view(N, H, W, 3)
    report_mismatch(got, want, f'frames_to_u8 {N}x{H}x{W}')
    # NaN -> 0 (torch's cast of NaN is undefined: not compared with it); the neighbours of a NaN are untouched by it
    y = x.clone()
    nan_at = torch.randperm(y.numel(), generator=gen)[:97]
    y.view(-1)[nan_at] = float('nan')
    gin = Guarded(y.view(N * 3, H * W), role='in')
    gout = Guarded(base=torch.full((N * H, W * 3), 7, dtype=torch.uint8))  # (7: a NaN that was skipped would not read 0)
    call_abi('mmvid_frames_to_u8', gin.ptr, N, H, W, gout.ptr)
    gin.check('frames_to_u8 img (NaN)')
    got = gout.check('frames_to_u8 out (NaN)').view(N, H, W, 3).permute(0, 3, 1, 2)
    isnan = torch.isnan(y)
    assert int(got[isnan].max()) == 0
    assert torch.equal(got[~isnan], want.permute(0, 3, 1, 2)[~isnan])


def test_frames_to_u8_refuses_a_plane_that_is_no_multiple_of_four():
    from mmvid_amd import _lib, ops
    x = torch.rand(2, 3, 3, 5)
    gin = Guarded(x.view(6, 15), role='in')
    gout = Guarded(role='out', shape=(6, 15), dtype=torch.uint8, partial=True)
    rc = _lib.load().mmvid_frames_to_u8(gin.ptr, 2, 3, 5, gout.ptr, ops._stream())
    torch.cuda.synchronize()
    assert rc == 1 and b'multiple of 4' in _lib.load().mmvid_last_error()  # MMVID_ERR_ARG
    gin.check('refused call, img')
    assert int((gout.check('refused call, out') != 0xA5).sum()) == 0  # nothing was launched: the window still holds the sentinel
    with pytest.raises(_lib.MMVIDError):
        ops.frames_to_u8(x.to(DEV))


# ------------------------------------------------------------------------------------------------------------------ the model
def build_model(num_visuals=0, **kw):
    from mmvid_amd.dalle_bert import BERT
    torch.manual_seed(20)
    m = BERT(dim=768, vae=tiny_vae(), num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
             num_visuals=num_visuals, num_targets=T, transformer_layers=2, **kw)
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model():
    return build_model()


@pytest.fixture(scope='module')
def inputs():
    gen = torch.Generator().manual_seed(21)
    text = torch.randint(1, 49408, (B, 16), generator=gen)
    text[0, 9:] = 0
    return text.to(DEV), torch.rand(B, T, 3, 64, 64, generator=gen).to(DEV)


class Recorder:
    """A `_race` that draws from the device generator and keeps what it drew, by name."""

    def __init__(self):
        self.drawn = {}

    def __call__(self, name, shape):
        assert name not in self.drawn
        t = torch.rand(shape, device=DEV) if name.endswith('_noise_u') else torch.empty(shape, device=DEV).exponential_()
        self.drawn[name] = t
        return t


def rows_of(drawn, name, rows, r0, r1):
    """Rows [r0, r1) of the `rows` sampler rows a recorded variate was drawn for (its leading dimension is rows x something)."""
    t = drawn[name]
    per = t.shape[0] // rows
    assert per * rows == t.shape[0]
    return t[r0 * per:r1 * per].contiguous()


CASES = {  # mode: generate_long arguments (test 2 of the issue), mp_config's B
    'interp': (dict(mode='interp', t_repeat=3), 2),
    'interp_real': (dict(mode='interp_real', t_repeat=2, dynamic=True), 1),
    'long': (dict(mode='long', t_repeat=3, t_overlap=2), 2),
}


@pytest.fixture(scope='module')
def batched(model, inputs, golden):
    """One generate_long run per mode with recorded variates, shared by the tests below (and left unchanged by them)."""
    from mmvid_amd import long_video as lv
    text, real = inputs
    out = {}
    for mode, (kw, beams) in CASES.items():
        mp = dict(golden('mask_predict').meta['mp_config'], B=beams)
        rec, trace = Recorder(), []
        torch.manual_seed(22)
        frames, tokens = lv.generate_long(model, text, real_frames=real if mode == 'interp_real' else None, mask_predict_steps=4,
                                          mp_config=mp, trace=trace, _race=rec, **kw)
        out[mode] = dict(frames=frames, tokens=tokens, drawn=rec.drawn, trace=trace, mp=mp, kw=kw)
    return out


# ------------------------------------------------------------------------------------ 2. batched levels equal chained windows
@pytest.mark.parametrize('mode', list(CASES))
def test_batched_levels_equal_chained_windows(model, inputs, batched, mode):
    """The reference's loop (utils_train.py:1337-1526) as it stands: one generate_images call per window, each on its rows of the
    variates the batched run drew (rows window * b .. window * b + b - 1)."""
    from mmvid_amd import long_video as lv
    text, real = inputs
    run = batched[mode]
    kw = run['kw']
    levels = lv.plan(mode, T, kw['t_repeat'], kw.get('t_overlap', 1))
    MASK = model.image_token_lut['[MASK]']
    prev = model.get_image_tokens(real, reshape=True).view(B, T, N_TOK) if mode == 'interp_real' else None
    out = []
    for li, lev in enumerate(levels):
        W = len(lev.windows)
        nxt = []
        for w, (given, passes, emits) in enumerate(lev.windows):
            preserve = None
            if given is not None and mode == 'long':
                preserve = prev[:, given[0]:given[1]].reshape(B * T, N_TOK)  # code_: (b t) n
            elif given is not None:
                preserve = torch.full((B, T * N_TOK), MASK, dtype=torch.long, device=DEV)
                preserve[:, :T * N_TOK // 2] = prev[:, given[0]:given[1]].reshape(B, -1)
            race = lambda name, shape, li=li, w=w, W=W: rows_of(run['drawn'], f'L{li}c0/{name}', W * B, w * B, w * B + B)  # noqa: E731
            _, _, seq = model.generate_images(text, mask_predict_steps=4, mp_config=run['mp'], dynamic=kw.get('dynamic', True),
                                              preserve=preserve, t_overlap=lev.t_overlap, long_mode=lev.long_mode, _race=race)
            seq = seq.view(B, T, N_TOK)
            nxt.append(seq[:, passes[0]:passes[1]])
            if emits[1] > emits[0]:
                out.append(seq[:, emits[0]:emits[1]])
        prev = torch.cat(nxt, dim=1)
    chained = torch.cat(out, dim=1)
    assert chained.shape == run['tokens'].shape
    assert torch.equal(chained, run['tokens']), f'{int((chained != run["tokens"]).sum())} of {chained.numel()} tokens differ'


# --------------------------------------------------------------------------------------------- 3. chunking changes nothing
def test_max_rows_changes_nothing(model, inputs, batched):
    from mmvid_amd import long_video as lv
    text, _ = inputs
    run = batched['interp']
    levels = lv.plan('interp', T, 3)

    def race(name, shape):
        li, ci, rest = re.fullmatch(r'L(\d+)c(\d+)/(.+)', name).groups()
        rows = len(levels[int(li)].windows) * B
        r0 = int(ci) * 3
        got = rows_of(run['drawn'], f'L{li}c0/{rest}', rows, r0, min(rows, r0 + 3))
        assert tuple(got.shape) == tuple(shape)
        return got

    trace = []
    _, tokens = lv.generate_long(model, text, mask_predict_steps=4, mp_config=run['mp'], max_rows=3, decode=False, trace=trace, _race=race,
                                 **run['kw'])
    assert trace[2]['rows'] == [(0, 3), (3, 6), (6, 8)]  # the 8-row last level, split unevenly
    assert torch.equal(tokens, run['tokens'])


# ------------------------------------------------------------------------------------------------- 4. structure on the device
def test_structure_of_the_three_modes(model, inputs, batched, golden):
    from mmvid_amd import long_video as lv
    text, real = inputs
    V = model.num_image_tokens
    for mode, run in batched.items():
        kw = run['kw']
        F = lv.frames_out(lv.plan(mode, T, kw['t_repeat'], kw.get('t_overlap', 1)))
        assert run['tokens'].shape == (B, F, N_TOK) and run['tokens'].dtype == torch.int64
        assert 0 <= int(run['tokens'].min()) and int(run['tokens'].max()) < V
        assert run['frames'].shape == (B, F, 64, 64, 3) and run['frames'].dtype == torch.uint8 and run['frames'].is_cuda
    # long: the first t_overlap frames of clip k are the last t_overlap frames of the timeline before it
    run, o = batched['long'], 2
    assert run['tokens'].shape[1] == T + 2 * (T - o)
    for k in range(1, 3):
        clip = run['trace'][k]['timeline']  # the whole clip k: [b, T, n]
        end = T + (k - 1) * (T - o)  # frames of the output before clip k's own
        assert torch.equal(clip[:, :o], run['tokens'][:, end - o:end])
        assert torch.equal(clip[:, o:], run['tokens'][:, end:end + T - o])
    # interp: the even frames of a level are the whole previous level
    run = batched['interp']
    lines = [r['timeline'] for r in run['trace']]
    assert [t.shape[1] for t in lines] == [T, 2 * T, 4 * T] and torch.equal(lines[-1], run['tokens'])
    for t in (1, 2):
        assert torch.equal(lines[t][:, ::2], lines[t - 1])
    # interp_real: two levels (t_repeat = 3) put three frames between two real ones
    real_tok = model.get_image_tokens(real, reshape=True).view(B, T, N_TOK)
    assert torch.equal(batched['interp_real']['tokens'][:, ::2], real_tok)
    mp = dict(golden('mask_predict').meta['mp_config'], B=1)
    _, tokens = lv.generate_long(model, text, mode='interp_real', t_repeat=3, real_frames=real, mask_predict_steps=4, mp_config=mp,
                                 decode=False)
    assert tokens.shape == (B, 13, N_TOK) and int(tokens.max()) < V
    assert torch.equal(tokens[:, ::4], real_tok)


# ------------------------------------------------------------------------------------------------------------------ 5. frames
def test_frames_and_files(model, batched, tmp_path):
    from PIL import Image

    from mmvid_amd import long_video as lv, ops
    from test_data_path import _boxes
    run = batched['interp']
    tokens, frames = run['tokens'], run['frames']
    F = tokens.shape[1]
    dec = model.vae.decode(tokens.view(-1, N_TOK))
    assert torch.equal(frames, ops.frames_to_u8(dec).view(B, F, 64, 64, 3))
    host = (dec.cpu().clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).reshape(B, F, 64, 64, 3)  # data.save_image_tensor's
    assert torch.equal(frames.cpu(), host)
    assert lv.save(frames[1], tmp_path / 'video', video_format='gif') == 'video.gif'
    assert lv.save(frames[1], tmp_path / 'video', video_format='mp4', fps=4) == 'video.mp4'
    with Image.open(tmp_path / 'video.gif') as im:
        assert im.n_frames == F and im.size == (64, 64)
    buf = (tmp_path / 'video.mp4').read_bytes()
    assert len(buf) > 0
    box = {k: (o, n) for k, o, n in _boxes(buf)}
    for name in ('moov', 'trak', 'mdia', 'minf', 'stbl'):
        box = {k: (o, n) for k, o, n in _boxes(buf, box[name][0], sum(box[name]))}
    o, _ = box['stsz']
    assert int.from_bytes(buf[o + 8:o + 12], 'big') == F


# ------------------------------------------------------------------------------------------------- 6. visual control, redraw
def test_visual_control_once_per_video_or_per_window(golden):
    """Nothing random in the control rows (no erasure, no vc_mode): the visual frames go through the VQGAN encoder once per video.
    erase_visual during generation is the reference's erase_visual_half=True (dalle_bert.py:458-466, 784-787): the lower half of
    every visual frame becomes [MASK], the same in every window, so no two windows can differ there -- the control rows are still
    computed per window, as the reference computes them.  What IS drawn per generate_images call is the region of
    erase_codebook_face (vc_mode): there the windows of one video must not all agree."""
    from mmvid_amd import long_video as lv
    m = build_model(num_visuals=1, frontend_seed=1234)
    gen = torch.Generator().manual_seed(23)
    text = torch.randint(1, 49408, (B, 16), generator=gen).to(DEV)
    visual = torch.rand(B, 1, 3, 64, 64, generator=gen).to(DEV)
    mp = dict(golden('mask_predict').meta['mp_config'], B=1)
    encoded = []
    encode = m.vae.get_codebook_indices
    m.vae.get_codebook_indices = lambda img: (encoded.append(img.shape[0]), encode(img))[1]
    common = dict(visual=visual, mode='interp', t_repeat=3, mask_predict_steps=2, mp_config=mp, decode=False)
    lo, hi = 1 + 16, 1 + 16 + N_TOK  # the visual segment of the control rows

    trace = []
    _, tokens = lv.generate_long(m, text, trace=trace, **common)
    assert tokens.shape == (B, 4 * T, N_TOK)
    assert sum(encoded) == B and [r['control_rows'] for r in trace] == [B, 0, 0]
    plain = trace[-1]['control'][:, lo:hi]
    assert all(torch.equal(plain[w * B:(w + 1) * B], plain[:B]) for w in range(4))

    encoded.clear()
    trace = []
    _, tokens = lv.generate_long(m, text, erase_visual=True, trace=trace, **common)
    assert int(tokens.max()) < m.num_image_tokens
    assert sum(encoded) == 7 * B and [r['control_rows'] for r in trace] == [B, 2 * B, 4 * B]
    half = trace[-1]['control'][:, lo:hi]
    with torch.no_grad():  # what one generate_images call of the reference assembles (dalle_bert.py:458-466)
        one = m(text, visual=visual, erase_visual=True, erase_visual_half=True, return_loss=False)[:, lo:hi]
    assert torch.equal(half, one.repeat(4, 1, 1))
    assert torch.equal(half[:, :N_TOK // 2], plain[:, :N_TOK // 2])  # upper half: the frame's own tokens
    assert not bool((half[:, N_TOK // 2:] == plain[:, N_TOK // 2:]).all(-1).any())  # lower half: [MASK] at every position

    trace = []
    lv.generate_long(m, text, vc_mode='face_8x8', trace=trace, **common)
    assert [r['control_rows'] for r in trace] == [B, 2 * B, 4 * B]
    drawn = torch.cat([r['control'][:, lo:hi].view(-1, B, N_TOK, 768) for r in trace])  # [7 windows, b, n, E]
    for v in range(B):
        assert any(not torch.equal(drawn[w, v], drawn[0, v]) for w in range(1, 7)), 'every window drew the same region'
