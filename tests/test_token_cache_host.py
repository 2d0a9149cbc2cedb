"""Token cache (mmvid_amd/token_cache.py), host side: the on-disk format, the dataset's window parity with data.TextVideoDataset,
the tokeniser check, and a numpy restatement of how a WarpParams record maps target tokens to the VID negative's tokens
(tests/test_token_step_gpu.py reuses the helpers here)."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from mmvid_amd import data, token_cache

SIZE, N_TOK = 32, 4  # frames of 32 x 32 -> a 2 x 2 token map


# ------------------------------------------------------------------------------------------------- helpers (shared with the GPU file)
def write_frame_folder(root, lengths, size=40, seed=0, captions=3):
    """`root/video/<key>/<i>.png` (noise frames: every frame distinct) + `root/txt/<key>.txt` (`captions` lines).  -> keys."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'txt'), exist_ok=True)
    keys = []
    for v, count in enumerate(lengths):
        key = f'vid{v:02d}'
        os.makedirs(os.path.join(root, 'video', key))
        for i in range(count):  # (names that only sort right in natural order: 2.png before 10.png)
            Image.fromarray(rng.randint(0, 256, (size, size, 3)).astype(np.uint8)).save(os.path.join(root, 'video', key, f'{i}.png'))
        with open(os.path.join(root, 'txt', key + '.txt'), 'w') as fh:
            fh.write('\n'.join(f'{key} caption {c}' for c in range(captions)) + '\n\n')
        keys.append(key)
    return keys


class CharTokenizer:
    """Stands in for SimpleTokenizer: one id per character, zero padded."""

    def tokenize(self, text, context_length=256, truncate_text=False):
        out = torch.zeros(1, context_length, dtype=torch.long)
        ids = [ord(c) for c in text][:context_length]
        out[0, :len(ids)] = torch.tensor(ids)
        return out


def parse_warp_params(raw, B):
    """The WarpParams records of csrc/frontend.hip (176 bytes each: mode, j1, src_b, src_t, chan, shift, th[6], perm[32])."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8)[:B * 176])
    a, f = raw.view(np.int32).reshape(B, 44), raw.view(np.float32).reshape(B, 44)
    return [dict(mode=int(a[b, 0]), j1=int(a[b, 1]), src_b=int(a[b, 2]), src_t=int(a[b, 3]), chan=int(a[b, 4]), shift=float(f[b, 5]),
                 theta=f[b, 6:12].copy(), perm=a[b, 12:44].tolist()) for b in range(B)]


def pack_warp_params(params):
    """The inverse: a list of dicts (missing fields zero / identity) -> uint8 [B * 176]."""
    a = np.zeros((len(params), 44), np.int32)
    f = a.view(np.float32)
    for b, p in enumerate(params):
        a[b, :5] = [p['mode'], p['j1'], p.get('src_b', b), p.get('src_t', p['j1']), p.get('chan', 0)]
        f[b, 5] = p.get('shift', 0.0)
        f[b, 6:12] = p.get('theta', np.zeros(6, np.float32))
        a[b, 12:44] = p.get('perm', list(range(32)))
    return a.view(np.uint8).reshape(-1).copy()


def negative_tokens(target, new_tok, params, T):
    """What the VID negative's tokens are, restated from the reference's warp() (dalle_bert.py:204-238) on frames that the VQGAN
    tokenises independently.  target [B, T*n], new_tok [B, n] (tokens of the one re-made frame per sample), params: one record per
    sample.  mode 0: frame j1 <- frame src_t of sample src_b; 1: frames permuted (out frame t = frame perm[t]); 2 (colour shift)
    and 3 (affine warp): frame j1 <- the new frame's tokens."""
    target, new_tok = np.asarray(target), np.asarray(new_tok)
    B = target.shape[0]
    tok = target.reshape(B, T, -1)
    out = tok.copy()
    for b, p in enumerate(params):
        if p['mode'] == 1:
            out[b] = tok[b, p['perm'][:T]]
        elif p['mode'] == 0:
            out[b, p['j1']] = tok[p['src_b'], p['src_t']]
        else:
            out[b, p['j1']] = new_tok[b]
    return out.reshape(B, -1)


def stub_vae(image_size=SIZE, ncode=64, seed=0):
    """The three tensor groups a token cache fingerprints (encoder, quant_conv, codebook) without a VQGAN: no GPU needed."""
    torch.manual_seed(seed)
    model = types.SimpleNamespace(encoder=nn.Sequential(nn.Conv2d(3, 4, 3), nn.Conv2d(4, 4, 3)), quant_conv=nn.Conv2d(4, 4, 1),
                                  quantize=types.SimpleNamespace(embedding=nn.Embedding(ncode, 4)))
    return types.SimpleNamespace(image_size=image_size, model=model, strict=False)


def host_cache(tmp_path, lengths=(9, 12, 20, 5), with_frames=True, vae=None):
    """A frame folder and a cache of it written without a tokeniser: the tokens of row r spell r (so a window's tokens name its rows)."""
    root = str(tmp_path / 'set')
    keys = write_frame_folder(root, lengths)
    os.makedirs(os.path.join(root, 'video', 'nocaption'))  # a video without a caption file: dropped by both datasets
    listing = data.TextVideoDataset(root, image_size=SIZE, frame_num=1, frame_step=1)
    videos, frames, first = [], [], 0
    for key in listing.keys:
        videos.append({'key': key, 'first': first, 'count': len(listing.videos[key]), 'text': os.path.join('txt', key + '.txt')})
        frames += [data._load_frame_u8(p, SIZE) for p in listing.videos[key]]
        first += len(listing.videos[key])
    rows = np.arange(first)
    tokens = np.stack([rows // 4096, (rows // 256) % 16, (rows // 16) % 16, rows % 16], 1)
    vae = vae or stub_vae()
    out = token_cache.write_token_cache(str(tmp_path / 'cache'), tokens, np.stack(frames) if with_frames else None, videos, SIZE,
                                        vae.model.quantize.embedding.weight.shape[0], 'split', token_cache.vae_fingerprint(vae), folder=root)
    return root, out, keys, vae


def rows_of(tokens):
    t = np.asarray(tokens).reshape(-1, N_TOK)
    return t[:, 0] * 4096 + t[:, 1] * 256 + t[:, 2] * 16 + t[:, 3]


# ------------------------------------------------------------------------------------------------- 1. format
def test_format_round_trip(tmp_path):
    root, out, keys, vae = host_cache(tmp_path)
    with open(os.path.join(out, 'index.json')) as fh:
        idx = json.load(fh)
    assert idx['version'] == token_cache.FORMAT_VERSION and idx['image_size'] == SIZE and idx['fmap'] == 2
    assert idx['codebook_size'] == 64 and idx['strict'] == 'split' and len(idx['fingerprint']) == 64
    # the 5-frame video is below the 8 frames every window needs and the caption-less one has no text: neither is stored
    assert [(v['key'], v['first'], v['count'], v['text']) for v in idx['videos']] == \
        [('vid00', 0, 9, 'txt/vid00.txt'), ('vid01', 9, 12, 'txt/vid01.txt'), ('vid02', 21, 20, 'txt/vid02.txt')]
    c = token_cache.TokenCache(out)
    assert isinstance(c.tokens, np.memmap) and c.tokens.dtype == np.uint16 and c.tokens.shape == (41, N_TOK)
    assert isinstance(c.frames, np.memmap) and c.frames.dtype == np.uint8 and c.frames.shape == (41, SIZE, SIZE, 3)
    assert len(c) == 41 and np.array_equal(rows_of(c.tokens), np.arange(41))
    c.check(vae)
    # natural order of the frame files: row 9 + 10 is `10.png` of vid01, not `2.png`
    assert np.array_equal(c.frames[9 + 10], data._load_frame_u8(os.path.join(root, 'video', 'vid01', '10.png'), SIZE))


def test_frames_are_optional(tmp_path):
    _, out, _, _ = host_cache(tmp_path, with_frames=False)
    c = token_cache.TokenCache(out)
    assert c.frames is None and not os.path.exists(os.path.join(out, 'frames.u8.npy'))
    ds = token_cache.TokenVideoDataset(c, tokenizer=CharTokenizer(), text_len=24, frame_num=4, deterministic=True)
    assert ds[0][2] is None


def test_codebook_beyond_uint16_is_refused(tmp_path):
    videos = [{'key': 'a', 'first': 0, 'count': 8, 'text': 'txt/a.txt'}]
    with pytest.raises(ValueError, match='70000'):
        token_cache.write_token_cache(str(tmp_path / 'c'), np.zeros((8, 4), np.int64), None, videos, SIZE, 70000, 'split', 'x' * 64)
    token_cache.write_token_cache(str(tmp_path / 'c'), np.zeros((8, 4), np.int64), None, videos, SIZE, 65535, 'split', 'x' * 64)


def test_builder_refuses_a_recipe_that_crops(tmp_path):
    """resize_ratio < 1: the tokens change with every crop; the builder must not pretend (refused before anything is loaded)."""
    with pytest.raises(ValueError, match='resize_ratio'):
        token_cache.build_token_cache(str(tmp_path), stub_vae(), str(tmp_path / 'c'), resize_ratio=0.75)


# ------------------------------------------------------------------------------------------------- 2. window parity
@pytest.mark.parametrize('deterministic', [True, False])
@pytest.mark.parametrize('frame_step', [1, 2])
def test_window_parity_with_text_video_dataset(tmp_path, deterministic, frame_step):
    """Seeded alike, TokenVideoDataset and data.TextVideoDataset (at resize_ratio 1, the cacheable recipe) pick the same caption
    and the same frames for every sample, over two epochs of one generator; frames_u8 / 255 are the pixel dataset's frames exactly."""
    root, out, keys, _ = host_cache(tmp_path)
    tk = CharTokenizer()
    kw = dict(text_len=24, frame_step=frame_step, frame_num=4, deterministic=deterministic, tokenizer=tk)
    gens = [torch.Generator().manual_seed(11) for _ in range(3)]
    pix = data.TextVideoDataset(root, image_size=SIZE, resize_ratio=1.0, generator=gens[0], **kw)
    tok = token_cache.TokenVideoDataset(out, generator=gens[1], **kw)
    row = token_cache.TokenVideoDataset(out, generator=gens[2], return_rows=True, **kw)
    assert pix.keys == tok.keys == row.keys == keys[:3] and len(tok) == 3
    cache = tok.cache
    starts = set()
    for epoch in range(2):
        for i in range(len(pix)):
            text_p, frames_p, _ = pix[i]
            text_t, target, frames_u8 = tok[i]
            text_r, rows, _ = row[i]
            assert torch.equal(text_p, text_t) and torch.equal(text_p, text_r)
            assert target.dtype == torch.int64 and target.shape == (4 * N_TOK, ) and rows.dtype == torch.int64 and rows.shape == (4, )
            assert np.array_equal(rows_of(target.numpy()), rows.numpy())
            v = cache.videos[keys[i]]
            start = int(rows[0]) - v['first']
            assert rows.tolist() == [v['first'] + start + k * frame_step for k in range(4)] and rows[-1] < v['first'] + v['count']
            assert frames_u8.dtype == torch.uint8 and frames_u8.shape == (4, SIZE, SIZE, 3)
            assert torch.equal(frames_u8.permute(0, 3, 1, 2).float() / 255, frames_p)  # (frames are distinct: equal pixels = equal indices)
            starts.add(start)
    assert starts == {0} if deterministic else len(starts) > 1


def test_skip_sample_matches(tmp_path):
    """A caption file without captions: both datasets move on to the next sample (not shuffled) the same way."""
    root, out, keys, _ = host_cache(tmp_path)
    open(os.path.join(root, 'txt', keys[1] + '.txt'), 'w').write('\n\n')
    kw = dict(text_len=24, frame_num=4, deterministic=True, tokenizer=CharTokenizer())
    pix = data.TextVideoDataset(root, image_size=SIZE, resize_ratio=1.0, **kw)
    tok = token_cache.TokenVideoDataset(out, **kw)
    assert torch.equal(pix[1][0], tok[1][0]) and torch.equal(tok[1][1], tok[2][1])
    assert torch.equal(tok[1][2].permute(0, 3, 1, 2).float() / 255, pix[1][1])


# ------------------------------------------------------------------------------------------------- 3. the tokeniser check
def test_check_raises_on_another_tokeniser(tmp_path):
    _, out, _, vae = host_cache(tmp_path)
    c = token_cache.TokenCache(out)
    c.check(vae)
    with torch.no_grad():
        vae.model.quantize.embedding.weight[3, 1] += 1e-3
        with pytest.raises(ValueError, match='fingerprint'):
            c.check(vae)
        vae.model.quantize.embedding.weight[3, 1] -= 1e-3
    c.check(stub_vae())  # (the same seed: the same weights)
    vae.image_size = 64
    with pytest.raises(ValueError, match='image_size'):
        c.check(vae)
    vae.image_size = SIZE
    with torch.no_grad():
        vae.model.encoder[1].bias[0] += 1e-3
    with pytest.raises(ValueError, match='fingerprint'):
        c.check(vae)
    with pytest.raises(ValueError, match='codebook of 64'):
        c.check(stub_vae(ncode=128))


# ------------------------------------------------------------------------------------------------- 4. WarpParams -> negative tokens
def test_negative_tokens_restatement():
    """The numpy restatement on hand-made records, one per strategy (the GPU file checks the kernels against it)."""
    B, T, n = 4, 3, 2
    target = np.arange(B * T * n).reshape(B, T * n)
    new = -1 - np.arange(B * n).reshape(B, n)
    params = [dict(mode=0, j1=1, src_b=2, src_t=0), dict(mode=1, j1=0, perm=[2, 0, 1] + list(range(3, 32))),
              dict(mode=2, j1=2, shift=0.25, chan=1), dict(mode=3, j1=0)]
    got = negative_tokens(target, new, params, T)
    assert got.tolist() == [[0, 1, 12, 13, 4, 5], [10, 11, 6, 7, 8, 9], [12, 13, 14, 15, -5, -6], [-7, -8, 20, 21, 22, 23]]
    back = parse_warp_params(pack_warp_params(params), B)
    assert [(p['mode'], p['j1']) for p in back] == [(0, 1), (1, 0), (2, 2), (3, 0)] and back[0]['src_b'] == 2 and back[1]['perm'][:3] == [2, 0, 1]
    assert back[2]['shift'] == 0.25 and back[2]['chan'] == 1 and back[3]['src_b'] == 3
