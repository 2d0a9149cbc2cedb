"""Batched, device-resident mask-predict sampler for BERT (mmvid_pytorch/dalle_bert.py:514-714).

The reference samples one video at a time with batch-1 tower passes, `Tmax * B` of them per video, and reads a score
back to the host for every candidate.  Here every video of the call and every beam candidate of a step go through the
tower as ONE batch of `b * B` sequences; confidences, tokens, keep-masks, scores, the best-candidate choice and the
dynamic stop live on the device (csrc/sample.hip).  The only host read is one "is anyone still running" flag per step
when `dynamic` is set.

Results are a function of the Exp(1) race variates (ops.exponential_like in production; tests inject them), of the
schedule and of the model -- independent of how many videos share the call.

`given` (video completion, mmvid_amd/completion.py) tells the sampler which tokens of which video are known: a mask and
a keep-count schedule PER ROW, where `preserve` has one pattern and one count for the whole call.

Classifier-free guidance (`uncond_emb`, `guidance_scale`): every step runs the tower a second time on the same tokens under the
unconditional control, and the token race reads `lc + w * (lc - lu)` from the two logit tensors.  Scores, candidate choice, the
dynamic stop and the given tokens belong to the conditional branch alone.  The launches of a token draw (plain, truncated, guided, both)
are token_draw.draw's; the argument rules of both samplers' keywords stand here, with the rule for the unconditional prompt of a guided call.
"""
import numpy as np
import torch

from . import ops, token_draw
from .artv_sampling import k_keep


def schedule(mp_config, N):
    """Keep-count and noise schedules of dalle_bert.py:586-614: three linear / constant segments each."""
    c = mp_config
    seg_n = [N * np.linspace(c['N1_n'], c['N2_n'], c['T1_n']), np.full(c['T2_n'], max(1, int(N * c['N3_n']))),
             np.full(c['T3_n'], max(1, int(N * c['N4_n'])))]
    seg_t = [np.linspace(c['N1_t'], c['N2_t'], c['T1_t']), np.full(c['T2_t'], c['N3_t']), np.full(c['T3_t'], c['N4_t'])]
    n = [int(v) for v in np.concatenate(seg_n)]
    temp = [float(v) for v in np.concatenate(seg_t)]
    return n, temp


def preserved_tokens(model, b, preserve, t_overlap, long_mode, device):
    """Which target positions are given (dalle_bert.py:542-583) -> (N, keep_fixed uint8 [TS] | None, fixed_tok [b, TS]).
    'long': the last t_overlap frames of the previous clip become the first frames of this one;
    'interp*': the given T/2 frames fill the even frame slots."""
    TS, ISL, T = model.target_seq_len, model.image_seq_len, model.num_targets
    MASK = model.image_token_lut['[MASK]']
    fixed_tok = torch.full((b, TS), MASK, dtype=torch.long, device=device)
    frame_of = torch.arange(TS, device=device) // ISL
    interp = long_mode in ('interp', 'interp2', 'interp_real')
    if long_mode == 'long':
        if preserve is None:
            return TS, None, fixed_tok
        prev = preserve.reshape(b, T * preserve.shape[-1])
        fixed = frame_of < t_overlap
        fixed_tok[:, :ISL * t_overlap] = prev[:, TS - ISL * t_overlap:]
        return TS - ISL * t_overlap, fixed.to(torch.uint8), fixed_tok
    if interp:
        if preserve is None:
            return TS // 2, None, fixed_tok
        given = preserve.reshape(b, T, ISL)[:, :T // 2]
        fixed_tok.view(b, T, ISL)[:, ::2] = given
        return TS // 2, (frame_of % 2 == 0).to(torch.uint8), fixed_tok
    return TS, None, fixed_tok


def keep_table(mp_config, unknown, Tmax):
    """Keep counts of a call with per-row given tokens -> int32 [Tmax - 1, b] (host): entry [t - 1, i] is the k of step t for row i,
    `unknown[i] - schedule(mp_config, unknown[i])[0][t - 1]`, with `unknown[i]` the row's number of unknown positions.  `schedule` runs
    once per distinct count."""
    per_count = {N: schedule(mp_config, N)[0] for N in sorted(set(int(v) for v in unknown))}
    table = np.empty((Tmax - 1, len(unknown)), np.int32)
    for i, N in enumerate(unknown):
        table[:, i] = [int(N) - per_count[int(N)][t - 1] for t in range(1, Tmax)]
    return table


def given_tokens(model, b, given, given_unknown, device):
    """`given` = (mask [b, TS] uint8 / bool, 1 = known; tokens [b, TS] int64) -> (unknown positions per row (host list), mask uint8
    [b, TS] on the device, fixed_tok [b, TS]: the given tokens, [MASK] elsewhere).  The per-row counts are the one host read of the
    given path: a mask on the host makes it free, a mask on the device costs one sync before the loop, and a caller that already
    holds the counts passes them as `given_unknown`."""
    TS, MASK = model.target_seq_len, model.image_token_lut['[MASK]']
    if not isinstance(given, (tuple, list)) or len(given) != 2:
        raise ValueError('given: expected (mask [b, TS] uint8 or bool, tokens [b, TS] int64)')
    mask, tokens = given
    if tuple(mask.shape) != (b, TS) or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f'given: the mask must be uint8 or bool [b, TS] = [{b}, {TS}], got {mask.dtype} {tuple(mask.shape)}')
    if tuple(tokens.shape) != (b, TS) or tokens.dtype != torch.int64:
        raise ValueError(f'given: the tokens must be int64 [b, TS] = [{b}, {TS}], got {tokens.dtype} {tuple(tokens.shape)}')
    known = mask != 0
    if given_unknown is None:
        given_unknown = (TS - known.sum(1)).tolist()
    if len(given_unknown) != b:
        raise ValueError(f'given: {len(given_unknown)} row counts for {b} rows')
    known = known.to(device)
    fixed_tok = torch.where(known, tokens.to(device), torch.full((), MASK, dtype=torch.long, device=device)).contiguous()
    return [int(v) for v in given_unknown], known.to(torch.uint8).contiguous(), fixed_tok


def guidance_table(guidance_scale, Tmax, b, device=None):
    """The guidance scales of a call as ONE fp32 table [Tmax, b] (row t: the scales of step t, one per video), contiguous, on `device`.
    Accepted: a float (every step, every video); a sequence of Tmax floats (one per step, step 0 included); a tensor [b] (one per
    video); a tensor [Tmax, b]."""
    if torch.is_tensor(guidance_scale):
        g = guidance_scale.detach().to(torch.float32)
        if g.dim() == 0:
            table = g.expand(Tmax, b)
        elif tuple(g.shape) == (Tmax, b):
            table = g
        elif tuple(g.shape) == (b, ):
            table = g.view(1, b).expand(Tmax, b)
        else:
            raise ValueError(f'guidance_scale: a tensor must be [b] = [{b}] (one scale per video) or [Tmax, b] = [{Tmax}, {b}], got '
                             f'{tuple(g.shape)}')
    elif isinstance(guidance_scale, (list, tuple, np.ndarray)):
        vals = [float(v) for v in guidance_scale]
        if len(vals) != Tmax:
            raise ValueError(f'guidance_scale: a sequence holds one scale per step, step 0 included: {Tmax} values, got {len(vals)}')
        table = torch.tensor(vals, dtype=torch.float32).view(Tmax, 1).expand(Tmax, b)
    else:
        try:
            w = float(guidance_scale)
        except (TypeError, ValueError):
            raise ValueError(f'guidance_scale: expected a float, {Tmax} floats, a tensor [{b}] or a tensor [{Tmax}, {b}]; got '
                             f'{type(guidance_scale).__name__}') from None
        table = torch.full((Tmax, b), w, dtype=torch.float32)
    if not table.is_cuda and not bool(torch.isfinite(table).all()):  # (a table already on the device is not read back)
        raise ValueError('guidance_scale: every scale must be finite')
    return table.to(device if device is not None else table.device).contiguous()


GUIDANCE_DROPS = ('text', 'visual')


def check_guidance(num_visuals, fixed_language_model, guidance_scale, guidance_drop, negative_text):
    """The argument rules of generate_images' guidance keywords, before any device work -> the drop as a tuple, or None when the call
    is unguided."""
    if guidance_scale is None:
        if negative_text is not None:
            raise ValueError('negative_text without guidance_scale: a negative prompt acts only through the guided step')
        return None
    drop = (guidance_drop, ) if isinstance(guidance_drop, str) else tuple(guidance_drop)
    unknown = [d for d in drop if d not in GUIDANCE_DROPS]
    if unknown:
        raise ValueError(f'guidance_drop: {unknown} is not among {GUIDANCE_DROPS}')
    if 'visual' in drop and num_visuals == 0:
        raise ValueError("guidance_drop names 'visual' on a model without a visual control (num_visuals == 0): pass guidance_drop=('text',)")
    if not drop and negative_text is None:
        raise ValueError('an empty guidance_drop without negative_text: the unconditional control would be the conditional one')
    if 'text' in drop and fixed_language_model and negative_text is None:
        raise ValueError("guidance_drop names 'text' on a model with a fixed language model: there is no defined null sentence "
                         'feature; pass negative_text (the feature of a negative prompt) or drop only the visual control')
    return drop


def check_truncation(top_k, top_p, Tmax, V):
    """The argument rules of the samplers' truncation keywords, before any device work -> (k per step, p per step): two host lists of
    Tmax entries (None = that filter is off at that step), or None when both keywords are None.  Accepted: an int / a float (every
    step), or a sequence of Tmax of them, one per step, step 0 included, whose None entries switch the filter off for the step.  The
    values are baked into the launches: a tensor (a per-video form) is refused.  A top_k >= V keeps every class."""
    if top_k is None and top_p is None:
        return None

    def per_step(value, name, one):
        if value is None:
            return [None] * Tmax
        if torch.is_tensor(value):
            raise ValueError(f'{name}: a tensor is not accepted (the value is a launch argument; there is no per-video form)')
        if isinstance(value, (list, tuple, np.ndarray)):
            vals = list(value)
            if len(vals) != Tmax:
                raise ValueError(f'{name}: a sequence holds one value per step, step 0 included: {Tmax} values, got {len(vals)}')
            return [None if v is None else one(v) for v in vals]
        return [one(value)] * Tmax

    def one_k(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'top_k: expected an integer >= 1 (or None: off), got {v!r}')
        return int(v)

    def one_p(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) <= 1.0:
            raise ValueError(f'top_p: expected a finite float in (0, 1] (or None: off), got {v!r}')
        return float(v)

    return per_step(top_k, 'top_k', one_k), per_step(top_p, 'top_p', one_p)


def check_truncation_artv(top_k, top_p, V):
    """ART-V's scalar `top_k` / `top_p` (check_truncation at one step) -> (k | None, p | None), or None when neither can remove a class of V."""
    trunc = check_truncation(top_k, top_p, 1, V)
    k, p = (None, None) if trunc is None else (trunc[0][0], trunc[1][0])
    return (k, p) if (k is not None and k < V) or (p is not None and p < 1.0) else None


class VideoParams:
    """What check_video_params returns: host arrays, [b] for ART-V and [Tmax, b] for BERT, each None when its keyword is.  k int32 (0: off;
    a k >= V is stored as 0), p fp32 (1: off), inv_div fp32 [b] (1 / temperature as fp32 rounds it).  on(t): can a filter remove a class
    of some video at step t -- known from the host values, so a step with nothing on takes the path without the keywords."""

    def __init__(self, k, p, inv_div):
        self.k, self.p, self.inv_div = k, p, inv_div

    def on(self, t=None):
        k, p = (self.k, self.p) if t is None else (None if self.k is None else self.k[t], None if self.p is None else self.p[t])
        return bool((k is not None and (k >= 1).any()) or (p is not None and (p < 1).any()))

    def device(self, dev):
        """-> (k, p, inv_div) on `dev`, the arrays the kernel reads (built once per call)."""
        return tuple(None if a is None else torch.from_numpy(a).to(dev) for a in (self.k, self.p, self.inv_div))


def check_video_params(video_top_k, video_top_p, video_temperature, b, V, Tmax=None, top_k=None, top_p=None, temperature=1.0):
    """The argument rules of the per-video sampling keywords, before any device work -> a VideoParams, or None when all three are None.
    check_truncation keeps the scalar keywords (a tensor there is still refused); these are their per-video forms under names of their own.

    Accepted for each: a sequence or a tensor of b entries, one per video; with Tmax (the mask-predict sampler) also [Tmax, b], one row per
    step, step 0 included, as guidance_table takes it.  A None entry of a sequence, a k of 0 and a p of 1 switch the filter off for that
    video (and step); a None temperature entry is 1.  A tensor on a device is read back once: the values are checked here, never on the
    device.  ValueError: a wrong length or shape; a bool; a negative or non-integer k; a p outside (0, 1] or not finite (or one that
    rounds to 0 in fp32); a temperature that is not finite and > 0 (or whose fp32 reciprocal is not); the scalar and the per-video form of
    one quantity together (top_k with video_top_k, top_p with video_top_p, a temperature other than 1 with video_temperature);
    video_temperature with Tmax (the mask-predict sampler has no softmax temperature to set per video)."""
    if video_top_k is None and video_top_p is None and video_temperature is None:
        return None
    if video_temperature is not None and Tmax is not None:
        raise ValueError('video_temperature: not accepted by the mask-predict sampler (its `temperature` schedule scales the noise on the '
                         'confidences; there is no per-video softmax temperature)')
    for scalar, video, name in ((top_k, video_top_k, 'top_k'), (top_p, video_top_p, 'top_p')):
        if scalar is not None and video is not None:
            raise ValueError(f'{name} and video_{name}: pass the scalar or the per-video form of one quantity, not both')
    if video_temperature is not None and not (isinstance(temperature, (int, float, np.integer, np.floating)) and float(temperature) == 1.0):
        raise ValueError('temperature and video_temperature: video_temperature replaces temperature, which must stay 1')

    def one_k(v):
        if v is None:
            return 0
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f'video_top_k: expected integers >= 0 (0 or None: off), got {v!r}')
        return int(v) if v < V else 0

    def one_p(v):
        if v is None:
            return 1.0
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) <= 1.0 or \
                not float(np.float32(v)) > 0.0:
            raise ValueError(f'video_top_p: expected finite floats in (0, 1] (1 or None: off), got {v!r}')
        return float(v)

    def one_t(v):
        if v is None:
            return 1.0
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(float(v)) and float(v) > 0.0
        if ok:
            with np.errstate(all='ignore'):
                inv = np.float32(1.0) / np.float32(v)
            ok = bool(np.isfinite(inv)) and float(inv) > 0.0
        if not ok:
            raise ValueError(f'video_temperature: expected finite floats > 0 with a finite fp32 reciprocal, got {v!r}')
        return float(v)

    def as_lists(value, name, integers):
        """A tensor, an array or a (nested) sequence as (nested) lists of Python scalars; the dtype of a tensor or an array is checked here."""
        if torch.is_tensor(value) or isinstance(value, np.ndarray):
            if torch.is_tensor(value):
                kind = 'b' if value.dtype == torch.bool else ('f' if value.dtype.is_floating_point or value.dtype.is_complex else 'i')
            else:
                kind = value.dtype.kind
            if kind == 'b' or (integers and kind not in 'iuO'):
                raise ValueError(f'{name}: values of {value.dtype} are not accepted' + (' (expected integers)' if integers else ''))
            return (value.detach().cpu() if torch.is_tensor(value) else value).tolist()
        if isinstance(value, (list, tuple)):
            return [as_lists(v, name, integers) if isinstance(v, (list, tuple, np.ndarray)) or torch.is_tensor(v) else v for v in value]
        return value

    def table(value, name, one, dtype, steps):
        if value is None:
            return None
        want = f'{b} entries, one per video' + (f', or [Tmax, b] = [{steps}, {b}]' if steps is not None else '')
        vals = as_lists(value, name, one is one_k)
        if isinstance(vals, list) and len(vals) == b and not any(isinstance(v, list) for v in vals):
            row = np.array([one(v) for v in vals], dtype)
            return row if steps is None else np.ascontiguousarray(np.broadcast_to(row, (steps, b)))
        if steps is not None and isinstance(vals, list) and len(vals) == steps and all(isinstance(r, list) and len(r) == b and
                                                                                       not any(isinstance(v, list) for v in r) for r in vals):
            return np.array([[one(v) for v in r] for r in vals], dtype)
        raise ValueError(f'{name}: expected {want}, got {type(value).__name__}' + (f' {tuple(value.shape)}' if hasattr(value, 'shape') else ''))

    k = table(video_top_k, 'video_top_k', one_k, np.int32, Tmax)
    p = table(video_top_p, 'video_top_p', one_p, np.float32, Tmax)
    temp = table(video_temperature, 'video_temperature', one_t, np.float32, None)
    return VideoParams(k, p, None if temp is None else (np.float32(1.0) / temp).astype(np.float32))


def check_guidance_artv(num_visuals, text_seq_len, total_tokens, num_image_tokens, B, guidance_scale, guidance_drop, negative_text, filter_thres):
    """The ART-V sampler's guidance keywords (check_guidance and the rules of the token loop, before any device work) -> (drop, scale),
    or None for the unguided call.  scale: a float, or a tensor [B] with one scale per video."""
    drop = check_guidance(num_visuals, False, guidance_scale, guidance_drop, negative_text)
    if drop is None:
        return None
    if isinstance(guidance_scale, (list, tuple, np.ndarray)) or (torch.is_tensor(guidance_scale) and guidance_scale.dim() > 1):
        raise ValueError('guidance_scale: a per-token schedule (a sequence, or a tensor [steps, B]) is not accepted: the captured token '
                         f'step reads one scale per video; pass a float or a tensor [B] = [{B}]')
    if torch.is_tensor(guidance_scale):
        if guidance_scale.dim() == 1 and guidance_scale.shape[0] != B:
            raise ValueError(f'guidance_scale: a tensor must be [B] = [{B}] (one scale per video), got {tuple(guidance_scale.shape)}')
        scale = guidance_scale.detach().to(torch.float32).expand(B)
        finite = scale.is_cuda or bool(torch.isfinite(scale).all())  # (a tensor already on the device is not read back)
    else:
        try:
            scale = float(guidance_scale)
        except (TypeError, ValueError):
            raise ValueError(f'guidance_scale: expected a float or a tensor [{B}], got {type(guidance_scale).__name__}') from None
        finite = np.isfinite(scale)
    if not finite:
        raise ValueError('guidance_scale: every scale must be finite')
    if negative_text is not None and (not torch.is_tensor(negative_text) or negative_text.dim() != 2 or
                                      tuple(negative_text[:, :text_seq_len].shape) != (B, text_seq_len)):
        got = tuple(negative_text.shape) if torch.is_tensor(negative_text) else type(negative_text).__name__
        raise ValueError(f'negative_text: expected int64 [B, text_seq_len] = [{B}, {text_seq_len}], got {got}')
    if k_keep(filter_thres, total_tokens) < num_image_tokens:
        raise ValueError(f'guidance_scale with filter_thres = {filter_thres}, which removes image classes: the torch.topk filter has no '
                         'guided form; leave filter_thres where it keeps the block and truncate with top_k (or top_p)')
    return drop, scale


def scale_vector(scale, B, device):
    """A float or a tensor -> fp32 [B] on the device: what the guided kernels read."""
    if torch.is_tensor(scale):
        return scale.to(device=device, dtype=torch.float32).expand(B).contiguous()
    return torch.full((B, ), float(scale), dtype=torch.float32, device=device)


def unconditional_inputs(text, visual, drop, negative_text):
    """The unconditional prompt of a guided call -> (text_u, visual_u).  The text is `negative_text` when given, all pad when `drop`
    names 'text', else `text`; the visual control (frames or tokens) is None when `drop` names 'visual', else `visual`."""
    text_u = negative_text.to(text.device) if negative_text is not None else (torch.zeros_like(text) if 'text' in drop else text)
    return text_u, None if 'visual' in drop else visual


@torch.no_grad()
def mask_predict(model, control_emb, dynamic=True, debug=False, steps=10, preserve=None, t_overlap=1, mp_config=None,
                 long_mode='long', race=None, trace=None, given=None, given_unknown=None, uncond_emb=None, guidance_scale=None,
                 top_k=None, top_p=None, video_top_k=None, video_top_p=None, video_temperature=None):
    """-> (tokens [b, TS] int64, image_samples list).  `race(name, shape)` supplies the Exp(1) variates (default: the
    device generator); `trace` (a list) receives one dict of the step's tensors per step (tests).

    `given` = (mask [b, TS] uint8 / bool, tokens [b, TS] int64): the tokens of row i where mask[i] is 1 are known.  They hold their
    value from step 0 on, are visible to the tower in every candidate and are never re-masked; row i runs the schedule of its own
    N_i = TS - sum(mask[i]) unknown positions (keep count of step t: N_i - n_i[t - 1], read by the kernel from one device table built
    before the loop).  A row with nothing unknown returns its tokens, a row with nothing given is the plain sampler's.  Exclusive
    with `preserve` and the interp modes, which are the two shared patterns of this.  See given_tokens for the one host read.

    `uncond_emb` [b, csl, E] with `guidance_scale` (see guidance_table) switches classifier-free guidance on: every tower input is
    built a second time from the same tokens and mask under `uncond_emb` and goes through the tower in a pass of its own, and tokens
    and confidences come from lc + w * (lc - lu), w the scale of the step and of the row's video, read by the kernel from one device
    table built before the loop.  The unconditional branch draws nothing and scores nothing.  With both None this is the unguided
    code path, launch for launch.

    `top_k`, `top_p` (see check_truncation): at a step with a filter on, the logits (the guided value when guided) first go through
    ops.logits_truncate and the plain race then draws from what is left, so `Y` is the confidence under the truncated distribution.
    A step with both off, and a call with both None, is the code path without them.

    `video_top_k`, `video_top_p` (see check_video_params: b values, or [Tmax, b]): the per-video forms.  Two device tables [Tmax, b]
    are built once before the loop; at a step where some video has a filter on, ONE ops.logits_truncate_rows stands where
    ops.logits_truncate would, and every row reads the values of its video (rows_per_param = candidates * TS).  A scalar of the other
    quantity composes.  A step at which no video has a filter on is the step without the per-video keywords (the host values say so).
    `video_temperature` is refused here."""
    if (uncond_emb is None) != (guidance_scale is None):
        raise ValueError('mask_predict: uncond_emb and guidance_scale come together (both, or neither)')
    guided = uncond_emb is not None
    dev = control_emb.device
    b, csl, E = control_emb.shape
    TS, MASK, V = model.target_seq_len, model.image_token_lut['[MASK]'], model.num_image_tokens
    L = csl + TS
    draw = race if race is not None else (lambda name, shape: ops.exponential_like(shape, dev))
    Tmax = mp_config['T'] if steps <= 0 else steps
    Bm = mp_config['B']
    if Tmax < 2:
        raise RuntimeError('mask_predict needs at least 2 steps (the reference returns nothing for steps == 1)')
    trunc = check_truncation(top_k, top_p, Tmax, V)
    # the steps at which a filter can remove a class; at the others (k >= V, p = 1, None) the draw is the one without the keywords
    trunc_on = [False] * Tmax if trunc is None else [(k is not None and k < V) or (p is not None and p < 1.0) for k, p in zip(*trunc)]
    video = check_video_params(video_top_k, video_top_p, video_temperature, b, V, Tmax, top_k, top_p)
    rows_on = [False] * Tmax if video is None else [video.on(t) for t in range(Tmax)]
    if given is None:
        N, fixed, fixed_tok = preserved_tokens(model, b, preserve, t_overlap, long_mode, dev)
        n, temp = schedule(mp_config, N)
        keep_count = lambda t: N - n[t - 1]  # noqa: E731
    else:
        if preserve is not None or long_mode != 'long':
            raise ValueError("given: exclusive with `preserve` and with long_mode != 'long' (both are fixed patterns of given tokens)")
        unknown, fixed, fixed_tok = given_tokens(model, b, given, given_unknown, dev)
        temp = schedule(mp_config, TS)[1]  # (the temperature schedule does not depend on N)
        k_table = torch.from_numpy(keep_table(mp_config, unknown, Tmax)).to(dev)
        keep_count = lambda t: k_table[t - 1]  # noqa: E731

    if guided:
        if tuple(uncond_emb.shape) != (b, csl, E):
            raise ValueError(f'uncond_emb: expected the shape of control_emb {(b, csl, E)}, got {tuple(uncond_emb.shape)}')
        scale = guidance_table(guidance_scale, Tmax, b, dev)
    if any(rows_on):
        rows_k, rows_p, _ = video.device(dev)  # int32 / fp32 [Tmax, b]: row t is what step t reads

    control_emb = ops._chk(control_emb.contiguous().float(), torch.float32, 'control_emb')
    if guided:
        uncond_emb = ops._chk(uncond_emb.contiguous().float(), torch.float32, 'uncond_emb')
    iemb = model.image_emb.weight.detach()
    tpos = model.target_pos_emb.table().detach().contiguous()
    rel_head, vid_head = model.to_logits_rel, model.to_logits_vid

    def tower_logits(I_in, mask1, nb, control=None):
        x = ops.mp_build_input(control_emb if control is None else control, iemb, tpos, I_in, mask1, nb, MASK)
        out = model.transformer_forward(x)  # [b*nb, L, E]
        rows = out[:, csl:, :].reshape(b * nb * TS, E)
        return out, model.to_logits_rows(rows)

    truncated = {}  # what the truncated draw of the current step read: {'logits_t', 'kept'} (the trace keeps it)

    def trunc_of(t, nb):  # the `trunc` of step t's draw: per-row where a video has a filter on, else the scalar pair, else None
        if rows_on[t]:
            k, p = (trunc[0][t], trunc[1][t]) if trunc is not None else (None, None)
            return token_draw.RowParams(nb * TS, None if rows_k is None else rows_k[t], None if rows_p is None else rows_p[t], top_k=k, top_p=p)
        return (trunc[0][t], trunc[1][t]) if trunc_on[t] else None

    def draw_tokens(logits, logits_u, t, nb):  # step t, nb candidates per video -> (tokens, Y, the race variates)
        truncated.clear()
        shape = (b * nb * TS, V)
        Et = draw(f'tok{t}', shape)
        noise_u = None if temp[t] == 0.0 else (race(f'tok{t}_noise_u', shape) if race is not None else torch.rand(shape, device=dev))
        return (*token_draw.draw(logits, Et, logits_u=logits_u, scale=scale[t] if guided else None, rows_per_scale=nb * TS, noise_u=noise_u,
                                 temperature=temp[t], trunc=trunc_of(t, nb), want_y=True,
                                 record=truncated if trace is not None else None), Et)

    # ---- step 0: everything that is not given is [MASK]
    out, logits = tower_logits(fixed_tok, None, 1)
    logits_u = tower_logits(fixed_tok, None, 1, uncond_emb)[1] if guided else None
    I_new, Y, E0 = draw_tokens(logits, logits_u, 0, 1)
    Y = Y.view(b, TS)
    I_tok = I_new.view(b, TS)
    if fixed is not None:
        I_tok = torch.where(fixed.bool(), fixed_tok, I_tok)
    I_tok = I_tok.contiguous()
    if trace is not None:
        trace.append(dict(t=0, logits=logits, E_tok=E0, Y=Y.clone(), I_tok=I_tok.clone()))
        if guided:
            trace[-1].update(logits_u=logits_u, scale=scale[0])
        trace[-1].update(truncated)
    Imax = I_tok.clone()
    Smax = torch.zeros(b, device=dev)
    tmax = torch.zeros(b, dtype=torch.int32, device=dev)
    active = torch.ones(b, dtype=torch.uint8, device=dev)
    seq0 = torch.arange(b * Bm, device=dev) * L
    rel_rows, vid_rows = (seq0 + model.rel_tok_index).contiguous(), (seq0 + model.vid_tok_index).contiguous()
    frames = [[model.decode_images(I_tok[i:i + 1])] for i in range(b)] if debug else None
    stopped_at = [None] * b

    for t in range(1, Tmax):
        Ek = draw(f'keep{t}', (b, Bm, TS))
        mask1 = ops.mp_select_keep(Y, Ek, fixed, keep_count(t))
        out, logits = tower_logits(I_tok, mask1, Bm)
        logits_u = tower_logits(I_tok, mask1, Bm, uncond_emb)[1] if guided else None
        Inew, Ynew, Et = draw_tokens(logits, logits_u, t, Bm)
        out2d = out.view(b * Bm * L, E)
        z_rel = ops.head_rows_fwd(out2d, rel_rows, rel_head[0].weight, rel_head[0].bias, rel_head[1].weight.view(-1),
                                  rel_head[1].bias, rel_head[0].eps)[0]
        z_vid = ops.head_rows_fwd(out2d, vid_rows, vid_head[0].weight, vid_head[0].bias, vid_head[1].weight.view(-1),
                                  vid_head[1].bias, vid_head[0].eps)[0]
        rec = None
        if trace is not None or debug:
            rec = dict(t=t, k=keep_count(t), E_keep=Ek, mask1=mask1, logits=logits, E_tok=Et, Ynew=Ynew.view(b, Bm, TS),
                       Inew=Inew.view(b, Bm, TS), z_rel=z_rel, z_vid=z_vid, Y_before=Y.clone(), I_before=I_tok.clone(),
                       active_before=active.clone(), S=torch.empty(b, Bm, device=dev),
                       jmax=torch.empty(b, dtype=torch.int32, device=dev))
            if guided:
                rec.update(logits_u=logits_u, scale=scale[t])
            rec.update(truncated)
        ops.mp_update(mask1, Ynew, Inew, z_rel, z_vid, t, dynamic, Y, I_tok, Imax, Smax, tmax, active,
                      rec['S'] if rec else None, rec['jmax'] if rec else None)
        if rec is not None and trace is not None:
            rec.update(Y=Y.clone(), I_tok=I_tok.clone(), Imax=Imax.clone(), Smax=Smax.clone(), tmax=tmax.clone(),
                       active=active.clone())
            trace.append(rec)
        if debug:  # per video, in the reference's order: the masked previous sample, then the new one
            was, jm = rec['active_before'].cpu(), rec['jmax'].cpu()
            for i in range(b):
                if not was[i]:
                    continue
                hidden = (mask1[i, jm[i]] == 0).float().unsqueeze(0)
                frames[i].append(torch.clamp(frames[i][-1] * 0.7 + model.decode_masks(hidden) * 0.4, 0, 1))
                frames[i].append(model.decode_images(I_tok[i:i + 1]))
        if dynamic and not bool(active.any()):  # the one host read of a step
            break
    image_samples = [f for per_video in frames for f in per_video] if debug else []
    return Imax, image_samples
