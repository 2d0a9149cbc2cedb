"""Video completion: fill in the unknown tokens of videos whose known part differs from video to video.

The MSM strategies a BERT is trained with hide a box on every frame, its complement, a Bernoulli subset or all but some preserved
frames (dalle_bert.py:992-1031); at inference the reference reaches two fixed patterns only (`preserve` with long_mode 'long' or
'interp*'), one pattern and one keep count per call.  Here every row of the batched sampler has its own mask and its own schedule
(`sampling.mask_predict(given=...)`, one selection kernel for both forms), so one call predicts the rest of a clip from its first
frames, in-betweens key frames, regenerates a region under a new text -- or does all three in one batch.  The sampler's result for
a row does not depend on its batch mates.

A known token's value still depends on the pixels AROUND its patch through the VQGAN encoder's receptive field: fill the unknown
region of `frames` with a constant (the reference's erase_real uses ones) rather than with noise or stale content.
"""
import torch

from . import artv_sampling, ops, sampling, seeded

SHAPES = '[b, T] (whole frames), [b, T, h, w] (token grid) or [b, T, H, W] (pixels)'


def token_mask(given, T, fmap, image_size):
    """Which tokens are known -> uint8 [b, T * fmap * fmap] (1 = known), on the device of `given`.  `given` (bool, uint8 or any
    number, non-zero = known) is [b, T] (whole frames), [b, T, fmap, fmap] (the token grid) or [b, T, image_size, image_size]
    (pixels).  A token is given only if EVERY pixel of its patch is given."""
    given = torch.as_tensor(given)
    T, f, s = int(T), int(fmap), int(image_size)
    shape = tuple(given.shape)
    if len(shape) < 2 or shape[1] != T or shape[2:] not in ((), (f, f), (s, s)):
        raise ValueError(f'given: expected {SHAPES} with T = {T}, h = w = {f}, H = W = {s}; got {shape}')
    b = shape[0]
    known = given != 0
    if shape[2:] == ():
        known = known.view(b, T, 1).expand(b, T, f * f)
    elif shape[2:] == (s, s) and s != f:
        p = s // f
        known = known.view(b, T, f, p, f, p).all(dim=5).all(dim=3)
    return known.reshape(b, T * f * f).to(torch.uint8).contiguous()


def _frames_to_tokens(model, frames, b):
    """-> (tokens [b, T * n] int64, real_u8 [b * T, H, W, 3] | None)."""
    T, n, s = model.num_targets, model.image_seq_len, model.image_size
    if frames.dim() == 2 and frames.dtype == torch.int64:
        if tuple(frames.shape) != (b, T * n):
            raise ValueError(f'frames: token input must be int64 [b, T * n] = [{b}, {T * n}], got {tuple(frames.shape)}')
        return frames.contiguous(), None
    if frames.dim() == 5 and frames.dtype == torch.uint8:
        if tuple(frames.shape) != (b, T, s, s, 3):
            raise ValueError(f'frames: uint8 input must be [b, T, H, W, 3] = {(b, T, s, s, 3)}, got {tuple(frames.shape)}')
        real = frames.contiguous().view(b * T, s, s, 3)
        pixels = ops.frames_u8_to_f32(real).view(b, T, 3, s, s)
    elif frames.dim() == 5 and frames.dtype == torch.float32:
        if tuple(frames.shape) != (b, T, 3, s, s):
            raise ValueError(f'frames: fp32 input must be [b, T, 3, H, W] = {(b, T, 3, s, s)}, got {tuple(frames.shape)}')
        pixels = frames.contiguous()
        real = ops.frames_to_u8(pixels.view(b * T, 3, s, s))
    else:
        raise ValueError('frames: expected fp32 [b, T, 3, H, W] in [0, 1], uint8 [b, T, H, W, 3] or int64 tokens [b, T * n]; got '
                         f'{frames.dtype} {tuple(frames.shape)}')
    return model.get_image_tokens(pixels, reshape=True).contiguous(), real


@torch.no_grad()
def complete(model, text, frames, given, *, visual=None, mask_predict_steps=0, mp_config=None, dynamic=True, erase_visual=False,
             vc_mode=None, face_mode=None, decode=True, paste=True, guidance_scale=None, guidance_drop=('text', 'visual'),
             negative_text=None, top_k=None, top_p=None, _race=None, _trace=None):
    """`complete_seeded` without seeds: the variates come from torch's device generator (or from `_race`).  Its signature is pinned by
    tests/test_artv_completion_host.py, which is why the seeded call has a name of its own."""
    return complete_seeded(model, text, frames, given, None, visual=visual, mask_predict_steps=mask_predict_steps, mp_config=mp_config,
                           dynamic=dynamic, erase_visual=erase_visual, vc_mode=vc_mode, face_mode=face_mode, decode=decode, paste=paste,
                           guidance_scale=guidance_scale, guidance_drop=guidance_drop, negative_text=negative_text, top_k=top_k,
                           top_p=top_p, _race=_race, _trace=_trace)


@torch.no_grad()
def complete_seeded(model, text, frames, given, seeds, *, visual=None, mask_predict_steps=0, mp_config=None, dynamic=True,
                    erase_visual=False, vc_mode=None, face_mode=None, decode=True, paste=True, guidance_scale=None,
                    guidance_drop=('text', 'visual'), negative_text=None, top_k=None, top_p=None, _race=None, _trace=None):
    """Complete `b` videos of `num_targets` frames -> (frames_u8 [b, T, H, W, 3] uint8 on the device, or None without `decode`;
    tokens [b, T, n] int64).

    `frames`: the videos as fp32 [b, T, 3, H, W] in [0, 1], uint8 [b, T, H, W, 3], or int64 tokens [b, T * n]; only what `given`
    marks is read as known.  Pixels are tokenised by `model.get_image_tokens` in the VQGAN's current `strict` mode; 'split' is the
    mode whose indices are exact.  `given`: see token_mask; every video may have its own.  `text`, `visual`, `erase_visual`,
    `vc_mode`, `face_mode`, `mask_predict_steps`, `mp_config`, `dynamic`, `guidance_scale`, `guidance_drop`, `negative_text`, `top_k`, `top_p`: as for
    generate_images (guided completion: the given tokens are visible to both branches, and belong to the conditional one).  `seeds`:
    one per video, as for BERT.mask_predict (not with erase_visual); None: the unseeded call, which is `complete`.  The per-video
    `video_top_k` / `video_top_p` of BERT.mask_predict are not taken here (`complete`'s signature is pinned): call the sampler.

    One host read precedes the sampler's loop: the number of known tokens per video together with the count of given token ids
    outside [0, num_image_tokens), which raises ValueError.  `decode` decodes the result once, in slices of `vae._max_frames`;
    with `paste` and pixel `frames` the known patches show their own pixels and not their VQGAN reconstruction (csrc/frames.hip);
    with token input there are no pixels to paste and the plain byte kernel runs."""
    if mp_config is None:
        raise ValueError('complete: mp_config is required (the schedules of mask-predict, args.mp_config of the reference)')
    seeds = seeded.check_seeds(seeds, text.shape[0], race=_race, erase_visual=erase_visual)
    drop = None
    if guidance_scale is not None or negative_text is not None:
        drop = sampling.check_guidance(model.num_visuals, model.fixed_language_model is not None, guidance_scale, guidance_drop,
                                       negative_text)
    if top_k is not None or top_p is not None:
        sampling.check_truncation(top_k, top_p, mp_config['T'] if mask_predict_steps <= 0 else mask_predict_steps, model.num_image_tokens)
    T, n, s, f = model.num_targets, model.image_seq_len, model.image_size, model.image_fmap_size
    b, dev = text.shape[0], text.device
    V = model.num_image_tokens
    if isinstance(visual, (list, tuple)):  # frames [b, 3, H, W] each, as get_image_tokens takes them
        visual = torch.stack(list(visual), dim=1) if len(visual) else None
    mask = token_mask(given, T, f, s)
    if mask.shape[0] != b:
        raise ValueError(f'given: {mask.shape[0]} rows for {b} videos')
    was_training = model.training
    model.eval()
    try:
        tokens, real = _frames_to_tokens(model, frames, b)
        mask = mask.to(tokens.device)
        known = mask != 0
        outside = (known & ((tokens < 0) | (tokens >= V))).sum().view(1)
        stats = torch.cat((known.sum(1), outside)).tolist()  # the one host read: known tokens per video, ids outside the table
        if stats[-1]:
            raise ValueError(f'frames: {stats[-1]} given token ids are outside [0, num_image_tokens) = [0, {V})')
        unknown = [T * n - c for c in stats[:-1]]
        control = model(text, visual=visual, erase_visual=erase_visual, erase_visual_half=True, vc_mode=vc_mode, face_mode=face_mode,
                        return_loss=False)
        guide = {}
        if drop is not None:
            guide = dict(guidance_scale=guidance_scale, uncond_emb=model.guidance_control(
                text, drop, negative_text, visual=visual, erase_visual=erase_visual, vc_mode=vc_mode, face_mode=face_mode))
        mask, tokens = mask.to(dev), tokens.to(dev)
        seq = model.mask_predict(control, dynamic=dynamic, steps=mask_predict_steps, mp_config=mp_config, given=(mask, tokens),
                                 _given_unknown=unknown, seeds=seeds, _race=_race, _trace=_trace, top_k=top_k, top_p=top_p, **guide)[0]
        out = None
        if decode:
            flat = seq.view(b * T, n)
            out = torch.empty(b * T, s, s, 3, device=dev, dtype=torch.uint8)
            grid = mask.view(b * T, f, f)
            step = model.vae._max_frames(s)
            for i in range(0, b * T, step):
                dec = model.vae.decode(flat[i:i + step])
                if paste and real is not None:
                    ops.frames_paste_u8(dec, real[i:i + step], grid[i:i + step], out[i:i + step])
                else:
                    ops.frames_to_u8(dec, out[i:i + step])
            out = out.view(b, T, s, s, 3)
        return out, seq.view(b, T, n)
    finally:
        model.train(was_training)


@torch.no_grad()
def complete_artv(model, text, frames, given, *, visual=None, filter_thres=0.5, temperature=1., erase_visual=False, vc_mode=None,
                  face_mode=None, use_cache=True, top_k=None, top_p=None, guidance_scale=None, guidance_drop=sampling.GUIDANCE_DROPS,
                  negative_text=None, paste=True, seeds=None, video_top_k=None, video_top_p=None, video_temperature=None, _race=None,
                  _trace=None):
    """Video prediction on the autoregressive (ART-V) model -> (frames_u8 [b, T, H, W, 3] uint8 on the device, tokens [b, T * n] int64).

    `frames`: as for `complete` (fp32 [b, T, 3, H, W] in [0, 1], uint8 [b, T, H, W, 3], or int64 tokens [b, T * n]); only the frames
    `given` marks are read as known.  `given`: whole frames, [b, T] or [T], bool or uint8; every video may have its own.  A token-grid
    or pixel mask is refused: the model predicts tokens in raster order, frame after frame, and cannot take a later token of a frame
    into account.  CAUSALITY: a known frame conditions only the frames that come after it.  Frames generated in front of a known frame
    do not see it -- [0, 1, 1, 0] generates frame 0 from the text and the visual control alone, then frame 3 from frames 0-2 -- so
    in-betweening key frames is the BERT's task (`complete`), and prediction from the first frames is this one's.

    The other keywords (`seeds` and the per-video `video_top_k`, `video_top_p`, `video_temperature` among them) are those of DALLE.generate_images, which samples (`given=(mask, tokens)`).  The result is decoded once, in
    slices of `vae._max_frames`; with `paste` and pixel `frames` the known frames are the input's own bytes and not their VQGAN
    reconstruction (csrc/frames.hip); with token input there are no pixels to paste and the plain byte kernel runs."""
    T, n, s, f = model.num_targets, model.image_seq_len, model.image_size, model.image_fmap_size
    b, dev = text.shape[0], text.device
    mask = artv_sampling.check_frame_mask(given, b, T)  # (before the frames are tokenised)
    seeds = seeded.check_seeds(seeds, b, race=_race, erase_visual=erase_visual)
    sampling.check_video_params(video_top_k, video_top_p, video_temperature, b, model.num_image_tokens, None, top_k, top_p,
                                temperature)  # (before the frames are tokenised)
    if isinstance(visual, (list, tuple)):  # frames [b, 3, H, W] each, as get_image_tokens takes them
        visual = torch.stack(list(visual), dim=1) if len(visual) else None
    was_training = model.training
    model.eval()
    try:
        tokens, real = _frames_to_tokens(model, frames, b)
        _, seq = model.sample_tokens(text, visual=visual, filter_thres=filter_thres, temperature=temperature, erase_visual=erase_visual,
                                     vc_mode=vc_mode, face_mode=face_mode, use_cache=use_cache, top_k=top_k, top_p=top_p,
                                     guidance_scale=guidance_scale, guidance_drop=guidance_drop, negative_text=negative_text,
                                     given=(mask, tokens.to(dev)), seeds=seeds, video_top_k=video_top_k, video_top_p=video_top_p,
                                     video_temperature=video_temperature, _race=_race, _trace=_trace)
        flat = seq.reshape(b * T, n)
        out = torch.empty(b * T, s, s, 3, device=dev, dtype=torch.uint8)
        grid = mask.to(dev).view(b * T, 1, 1).expand(b * T, f, f).contiguous()
        step = model.vae._max_frames(s)
        for i in range(0, b * T, step):
            dec = model.vae.decode(flat[i:i + step])
            if paste and real is not None:
                ops.frames_paste_u8(dec, real[i:i + step], grid[i:i + step], out[i:i + step])
            else:
                ops.frames_to_u8(dec, out[i:i + step])
        return out.view(b, T, s, s, 3), seq.view(b, T * n)
    finally:
        model.train(was_training)
