"""Training from a pre-tokenised video cache.

The VQGAN is frozen and the reference's default training transform is deterministic per frame (`RandomResizedCrop(scale=
(resize_ratio, 1), ratio=(1, 1))` with `--random_resize_crop_lower_ratio` 1 crops the whole square frame, utils/utils_args.py:52-55,
mmvid_pytorch/loader.py:369-384; the horizontal flip is commented out), so the tokens of a frame are the same in every epoch.
They are computed once, offline, in an index-exact tokeniser mode; the training step then encodes only the one warped frame per
sample of the VID negative (BERT.forward(target=tokens, target_frames=frames_u8)).

On disk, a directory:
  tokens.u16.npy   [F_total, n] uint16      the tokens of every frame of every video, videos in key order
  frames.u8.npy    [F_total, H, W, 3] uint8 the resized frames (optional: the pixel strategies of the VID negative need them)
  index.json       format version, image_size, fmap, codebook size, the `vae.strict` mode of the build, a SHA-256 fingerprint of
                   the encoder / quant_conv / codebook tensors, and per video: key, first row, frame count, caption file

Recipes that DO augment pixels (resize_ratio < 1) cannot be cached: their tokens change with every crop.  They keep the pixel path;
`build_token_cache` refuses them."""
import hashlib
import json
import os

import numpy as np
import torch

from . import data

FORMAT_VERSION = 1
MAX_CODEBOOK = 65535  # the table is uint16
TOKENS, FRAMES, INDEX = 'tokens.u16.npy', 'frames.u8.npy', 'index.json'


def strict_name(strict):
    """`vae.strict` as index.json spells it: 'bf16' | 'mixed' | 'split' | 'fp32'."""
    return {False: 'bf16', True: 'fp32'}.get(strict, strict)


def vae_fingerprint(vae):
    """SHA-256 over everything the token indices depend on: the encoder, quant_conv and the codebook (names, shapes, fp32 bytes)."""
    m = vae.model
    groups = [('encoder', m.encoder.state_dict()), ('quant_conv', m.quant_conv.state_dict()),
              ('codebook', {'weight': m.quantize.embedding.weight})]
    h = hashlib.sha256()
    for gname, sd in groups:
        for k in sorted(sd):
            t = sd[k].detach().to('cpu', torch.float32).contiguous()
            h.update(f'{gname}.{k}{tuple(t.shape)}'.encode())
            h.update(t.numpy().tobytes())
    return h.hexdigest()


def _header(image_size, n, codebook_size, mode, fingerprint, videos, folder, with_frames):
    if codebook_size > MAX_CODEBOOK:
        raise ValueError(f'a codebook of {codebook_size} entries does not fit the uint16 token table (at most {MAX_CODEBOOK})')
    fmap = int(round(n**0.5))
    assert fmap * fmap == n, f'{n} tokens per frame is not a square map'
    return {'format': 'mmvid-token-cache', 'version': FORMAT_VERSION, 'image_size': int(image_size), 'fmap': fmap,
            'tokens_per_frame': int(n), 'codebook_size': int(codebook_size), 'strict': strict_name(mode), 'fingerprint': fingerprint,
            'folder': folder, 'frames': bool(with_frames), 'videos': videos}


def write_token_cache(out_dir, tokens, frames, videos, image_size, codebook_size, mode, fingerprint, folder=None):
    """Write a cache from arrays already in memory (tokens [F, n] integer, frames [F, H, W, 3] uint8 or None; videos: list of
    {'key', 'first', 'count', 'text'}).  `build_token_cache` streams instead; both write the same files."""
    tokens = np.asarray(tokens)
    head = _header(image_size, tokens.shape[1], codebook_size, mode, fingerprint, videos, folder, frames is not None)
    assert tokens.min() >= 0 and tokens.max() < codebook_size, 'token outside the codebook'
    assert sum(v['count'] for v in videos) == tokens.shape[0]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, TOKENS), tokens.astype(np.uint16))
    if frames is not None:
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.shape == (tokens.shape[0], image_size, image_size, 3)
        np.save(os.path.join(out_dir, FRAMES), frames)
    with open(os.path.join(out_dir, INDEX), 'w') as fh:
        json.dump(head, fh, indent=1)
    return out_dir


class TokenCache:
    """Reader: the arrays stay memory-mapped (a dataset worker touches only the rows of its window)."""

    def __init__(self, path):
        self.path = str(path)
        with open(os.path.join(self.path, INDEX)) as fh:
            self.index = json.load(fh)
        if self.index.get('format') != 'mmvid-token-cache' or self.index.get('version') != FORMAT_VERSION:
            raise ValueError(f'{self.path}: not a token cache of format version {FORMAT_VERSION}')
        self.image_size, self.fmap = self.index['image_size'], self.index['fmap']
        self.codebook_size, self.strict, self.fingerprint = self.index['codebook_size'], self.index['strict'], self.index['fingerprint']
        self.videos = {v['key']: v for v in self.index['videos']}
        self.tokens = np.load(os.path.join(self.path, TOKENS), mmap_mode='r')
        fpath = os.path.join(self.path, FRAMES)
        self.frames = np.load(fpath, mmap_mode='r') if os.path.exists(fpath) else None
        total = sum(v['count'] for v in self.index['videos'])
        if self.tokens.dtype != np.uint16 or self.tokens.shape != (total, self.fmap * self.fmap):
            raise ValueError(f'{self.path}: {TOKENS} is {self.tokens.dtype} {self.tokens.shape}, the index describes '
                             f'uint16 {(total, self.fmap * self.fmap)}')
        if self.frames is not None and (self.frames.dtype != np.uint8 or self.frames.shape != (total, self.image_size, self.image_size, 3)):
            raise ValueError(f'{self.path}: {FRAMES} is {self.frames.dtype} {self.frames.shape}, the index describes '
                             f'uint8 {(total, self.image_size, self.image_size, 3)}')

    def __len__(self):
        return self.tokens.shape[0]

    def to_device(self, device):
        """The whole token table [F_total, n] uint16 on the device, for ops.token_rows_gather (Multimodal VoxCeleb: a few
        hundred MB).  The step's target input is then the B * T frame indices."""
        return torch.from_numpy(np.ascontiguousarray(self.tokens)).to(device)

    def check(self, vae):
        """Raise ValueError unless `vae` is the tokeniser this cache was built with (size, codebook size, weights)."""
        size, ncode = getattr(vae, 'image_size', None), vae.model.quantize.embedding.weight.shape[0]
        if size != self.image_size:
            raise ValueError(f'token cache {self.path}: built at image_size {self.image_size}, the VQGAN runs at {size}')
        if ncode != self.codebook_size:
            raise ValueError(f'token cache {self.path}: built for a codebook of {self.codebook_size} entries, the VQGAN has {ncode}')
        fp = vae_fingerprint(vae)
        if fp != self.fingerprint:
            raise ValueError(f'token cache {self.path}: built with other encoder / quant_conv / codebook weights '
                             f'(fingerprint {self.fingerprint[:12]}..., this VQGAN {fp[:12]}...): rebuild it')


@torch.no_grad()
def build_token_cache(folder, vae, out_dir, mode='split', with_frames=True, chunk=64, resize_ratio=1.0):
    """Tokenise every frame of `folder` (the `video/<key>/*` + `txt/<key>.txt` layout of data.TextVideoDataset) once, with
    `vae.strict = mode`, and write the cache to out_dir.  Frames are loaded as data._load_frame loads them (PIL bilinear resize to
    uint8) and become floats on the device (ops.frames_u8_to_f32: u8 / 255).  `vae.strict` is restored afterwards.
    resize_ratio: the recipe's --random_resize_crop_lower_ratio; below 1 the training transform crops at random and no cache can
    stand in for it."""
    from . import ops
    if resize_ratio < 1:
        raise ValueError(f'resize_ratio = {resize_ratio} < 1: this recipe crops every sample at random, so its tokens differ from epoch '
                         'to epoch and cannot be cached. Train it from pixels.')
    size = vae.image_size
    ncode = vae.model.quantize.embedding.weight.shape[0]
    listing = data.TextVideoDataset(folder, image_size=size, frame_num=1, frame_step=1)  # (videos with a caption and >= 8 frames)
    videos, first = [], 0
    for key in listing.keys:
        videos.append({'key': key, 'first': first, 'count': len(listing.videos[key]),
                       'text': os.path.relpath(listing.texts[key], listing.root)})
        first += len(listing.videos[key])
    paths = [p for key in listing.keys for p in listing.videos[key]]
    n = (size // 16)**2
    head = _header(size, n, ncode, mode, vae_fingerprint(vae), videos, os.path.abspath(str(folder)), with_frames)
    os.makedirs(out_dir, exist_ok=True)
    tok = np.lib.format.open_memmap(os.path.join(out_dir, TOKENS), mode='w+', dtype=np.uint16, shape=(first, n))
    frm = np.lib.format.open_memmap(os.path.join(out_dir, FRAMES), mode='w+', dtype=np.uint8, shape=(first, size, size, 3)) \
        if with_frames else None
    device = vae.model.quantize.embedding.weight.device
    previous = vae.strict
    vae.strict = mode
    try:
        for i in range(0, first, chunk):
            u8 = np.stack([data._load_frame_u8(p, size) for p in paths[i:i + chunk]])
            idx = vae.get_codebook_indices(ops.frames_u8_to_f32(torch.from_numpy(u8).to(device)))
            tok[i:i + len(u8)] = idx.cpu().numpy().astype(np.uint16)
            if frm is not None:
                frm[i:i + len(u8)] = u8
    finally:
        vae.strict = previous
    tok.flush()
    if frm is not None:
        frm.flush()
    del tok, frm
    with open(os.path.join(out_dir, INDEX), 'w') as fh:
        json.dump(head, fh, indent=1)
    return TokenCache(out_dir)


class TokenVideoDataset(torch.utils.data.Dataset):
    """data.TextVideoDataset over a token cache: the same temporal window (`frame_num` frames, `frame_step` apart), the same text
    handling, the same `skip_sample`, and the same calls on the same generators in the same order -- the crop and visual-control
    draws of the pixel dataset included, although nothing here uses their values -- so equal RNG state gives equal samples.
    -> (text ids [text_len], target tokens [frame_num * n] int64 -- or the rows [frame_num] int64 of the device table
    (`return_rows=True`, with TokenCache.to_device + ops.token_rows_gather) --, frames uint8 [frame_num, H, W, 3] or None)."""

    def __init__(self, cache, folder=None, text_len=256, truncate_captions=False, tokenizer=None, frame_step=2, frame_num=8,
                 deterministic=False, video_only=False, keys=None, generator=None, shuffle=False, return_rows=False):
        super().__init__()
        self.cache = cache if isinstance(cache, TokenCache) else TokenCache(cache)
        self.root = str(folder) if folder is not None else self.cache.index.get('folder')
        self.text_len, self.truncate_captions, self.tokenizer = text_len, truncate_captions, tokenizer
        self.frame_step, self.frame_num, self.deterministic, self.video_only = frame_step, frame_num, deterministic, video_only
        self.generator, self.shuffle, self.return_rows = generator, shuffle, return_rows
        self.min_len = max(8, (frame_num - 1) * frame_step + 1)
        self.videos = {k: v for k, v in self.cache.videos.items() if v['count'] >= self.min_len and (keys is None or k in set(keys))}
        self.keys = sorted(self.videos)
        assert len(self.keys) > 0, f'no usable videos in {self.cache.path}'

    def __len__(self):
        return len(self.keys)

    def _rand(self, n):
        return int(torch.randint(0, n, (1, ), generator=self.generator))

    def _crop_draws(self):
        """The draws of TextVideoDataset's RandomResizedCrop at resize_ratio 1 (it crops the whole frame): values unused."""
        torch.empty(1).uniform_(1.0, 1.0, generator=self.generator)
        self._rand(1), self._rand(1)

    def _rows(self, v):
        span = (self.frame_num - 1) * self.frame_step
        start = 0 if self.deterministic else self._rand(v['count'] - span)
        if not self.deterministic:
            self._crop_draws()
            self._rand(v['count'])  # (the frame TextVideoDataset._visual picks, and its crop)
            self._crop_draws()
        return v['first'] + start + np.arange(self.frame_num) * self.frame_step

    def skip_sample(self, index):
        if self.shuffle:
            return self[self._rand(len(self))]
        return self[0 if index >= len(self) - 1 else index + 1]

    def __getitem__(self, index):
        v = self.videos[self.keys[index]]
        if self.video_only:
            caption = 'dummy text'
        else:
            path = os.path.join(self.root, v['text'])
            with open(path) as fh:
                lines = [t for t in fh.read().split('\n') if len(t) > 0]
            if not lines:
                print(f"An exception occurred trying to load file {path}.")
                print(f"Skipping index {index}")
                return self.skip_sample(index)
            caption = lines[0] if self.deterministic else lines[self._rand(len(lines))]
        rows = self._rows(v)
        text = self.tokenizer.tokenize(caption, self.text_len, truncate_text=self.truncate_captions).squeeze(0)
        target = torch.from_numpy(rows.astype(np.int64)) if self.return_rows else \
            torch.from_numpy(self.cache.tokens[rows].astype(np.int64)).reshape(-1)
        frames = None if self.cache.frames is None else torch.from_numpy(self.cache.frames[rows])
        return text, target, frames
