"""OpenAI CLIP (mmvid_pytorch/transformers/clip_model.py:298-473: CLIP, build_model) and the scoring helpers of the reference's
drivers (utils/utils.py:62-85 clip_similarity, utils/utils_train.py:283-294 clip_encode_image) over the native kernels: patch
extraction, sequence assembly, embedding, pooling and projection in csrc/clip.hip, the patch embedding on the bf16 GEMM, both
towers on csrc/tower.hip through OpenAICLIPTransformer.  Same constructor, parameter names and state_dict keys as the reference;
inference only (the reference's callers run CLIP under no_grad).  ViT configurations only."""

import numpy as np
import torch
from torch import nn

from . import _lib, ops
from .clip_tower import OpenAICLIPTransformer, _Holder, _ln_params
from .shadow import Cached

f32, bf16 = torch.float32, torch.bfloat16
IMAGE_SLICE = 256  # frames per pass through the visual tower at 50 positions (bounds the tower's scratch: frames_per_pass; results do not depend on it)


def _param(t):
    return nn.Parameter(t)


def _tower(seq_len, which, causal, width, layers, heads):
    if width != 64 * heads:
        raise NotImplementedError(f'CLIP tower of width {width} with {heads} heads: the tower kernels need head dimension 64')
    return OpenAICLIPTransformer(seq_len, which, causal=causal, mask_type='causal', layers=layers, width=width, heads=heads)


class VisualTransformer(_Holder):
    """clip_model.py:249-296 as parameters: conv1 (no bias), class / positional embedding, ln_pre, the tower, ln_post, proj."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution = input_resolution
        self.output_dim = output_dim
        self.patch_size = patch_size
        self.conv1 = _Holder()
        self.conv1.weight = _param(torch.randn(width, 3, patch_size, patch_size) * (3 * patch_size * patch_size)**-0.5)
        scale = width**-0.5
        self.class_embedding = _param(scale * torch.randn(width))
        self.positional_embedding = _param(scale * torch.randn((input_resolution // patch_size)**2 + 1, width))
        self.ln_pre = _ln_params(width)
        tower = _tower((input_resolution // patch_size)**2 + 1, 'openai_clip_visual', False, width, layers, heads)
        self.transformer = tower.transformer  # the parameters (keys visual.transformer.resblocks.*) ...
        object.__setattr__(self, 'tower', tower)  # ... and their runner, kept out of the module tree
        self.ln_post = _ln_params(width)
        self.proj = _param(scale * torch.randn(width, output_dim))


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_heads, transformer_layers):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError('CLIP with a ModifiedResNet image tower (RN50 family) is not implemented: ViT checkpoints only')
        if vision_patch_size < 1 or image_resolution % vision_patch_size:
            raise NotImplementedError(f'patch size {vision_patch_size} / resolution {image_resolution}: the patch kernel needs a '
                                      'patch size that divides the resolution')
        self.visual = VisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers, vision_width // 64, embed_dim)
        text_tower = _tower(context_length, 'openai_clip_text', True, transformer_width, transformer_layers, transformer_heads)
        self.transformer = text_tower.transformer
        object.__setattr__(self, 'text_tower', text_tower)
        self.token_embedding = _Holder()
        self.token_embedding.weight = _param(torch.randn(vocab_size, transformer_width) * 0.02)
        self.positional_embedding = _param(torch.randn(context_length, transformer_width) * 0.01)
        self.ln_final = _ln_params(transformer_width)
        self.text_projection = _param(torch.randn(transformer_width, embed_dim) * transformer_width**-0.5)
        self.logit_scale = _param(torch.ones([]) * np.log(1 / 0.07))
        # the TorchScript archive's attributes that the reference's callers read with .item() (utils.py:63-64)
        for k, v in (('input_resolution', image_resolution), ('context_length', context_length), ('vocab_size', vocab_size)):
            self.register_buffer(k, torch.tensor(v, dtype=torch.int64), persistent=False)
        self._shape = dict(R=image_resolution, P=vision_patch_size, L=context_length, V=vocab_size, D=embed_dim)
        self._conv_bf16 = Cached(self._conv_sources, self._build_conv_weight)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    # ---- reference API -------------------------------------------------------------------------------
    def encode_image(self, image):
        """clip_model.py:396-397: image [N,3,R,R], already normalised -> [N, embed_dim] fp32."""
        self._inference_only(image)
        with torch.no_grad():
            return self._image_features(image, normalize=False, l2=False)

    def encode_text(self, text):
        """clip_model.py:399-414: ids [B, context_length] -> [B, embed_dim] fp32, pooled at text.argmax(-1)."""
        self._inference_only(text)
        with torch.no_grad():
            return self._text_features(text, l2=False)

    def encode_text_tokens(self, text):
        """utils_train.py:264-274: ln_final(transformer(token_embedding + positional_embedding)) for every position, [B, L, width]."""
        self._inference_only(text)
        with torch.no_grad():
            x, _ = self._text_tower(text, want_pool=False)
            tw = self.ln_final
            y, _, _ = ops.layernorm_fwd(x, tw.weight.detach(), tw.bias.detach(), out_dtype=f32, save_stats=False)
            return y

    def forward(self, image, text, **kwargs):
        """clip_model.py:416-432 -> (logits_per_image [N, B], logits_per_text [B, N])."""
        self._inference_only(image, text)
        with torch.no_grad():
            img = self._image_features(image, normalize=False, l2=True)
            txt = self._text_features(text, l2=True)
            s = float(self.logit_scale.detach().exp())
            return ops.gemm_f32(img, txt, alpha=s), ops.gemm_f32(txt, img, alpha=s)

    # ---- native plumbing ------------------------------------------------------------------------------
    def _inference_only(self, *inputs):
        if torch.is_grad_enabled() and (any(t.requires_grad for t in inputs if torch.is_tensor(t))
                                        or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('mmvid_amd CLIP is inference only (no backward through CLIP): call it under torch.no_grad(), or freeze '
                               'its parameters and inputs (requires_grad_(False))')

    def _conv_weight(self):
        """bf16 copy of conv1.weight as the patch GEMM's [width, Kp] operand (columns beyond 3*P*P zero: see patch_columns), rebuilt
        when the parameter changes."""
        return self._conv_bf16.get()

    def _conv_sources(self):
        return [self.visual.conv1.weight]

    def _build_conv_weight(self):
        w = self.visual.conv1.weight
        flat = ops.cast_bf16(w.detach().contiguous().view(w.shape[0], -1))
        Kp = patch_columns(self._shape['P'])
        if Kp != flat.shape[1]:
            flat, dense = torch.zeros(w.shape[0], Kp, device=w.device, dtype=bf16), flat
            flat[:, :dense.shape[1]] = dense
        return flat

    def _check_image(self, image, normalize):
        R = self._shape['R']
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != image.shape[3]:
            raise ValueError(f'CLIP image input must be square frames [N, 3, S, S], got {tuple(image.shape)}')
        if not normalize and tuple(image.shape[2:]) != (R, R):
            raise ValueError(f'encode_image takes [N, 3, {R}, {R}] normalised frames, got {tuple(image.shape)}')
        return ops._chk(image.to(f32).contiguous(), f32, 'image')

    def _image_sequence(self, image, normalize):
        """frames [n,3,S,S] fp32 -> the visual tower's input [n, G*G+1, width]: patches (resized / normalised if `normalize`),
        conv1 as the bf16 GEMM, class token, positional embedding, ln_pre."""
        R, P = self._shape['R'], self._shape['P']
        vis = self.visual
        n, E, T = image.shape[0], vis.class_embedding.shape[0], (R // P)**2 + 1
        patches = patchify(image, R, P, normalize)
        feat = ops.gemm(patches, self._conv_weight(), out_dtype=f32)  # conv1 (stride = kernel = P, no bias): [n*G*G, Kp] x [E, Kp]^T
        x = torch.empty(n, T, E, device=image.device, dtype=f32)
        _lib.call('mmvid_clip_image_assemble', ops._p(feat), ops._p(vis.class_embedding), ops._p(vis.positional_embedding),
                  ops._p(vis.ln_pre.weight), ops._p(vis.ln_pre.bias), 1e-5, n, T, E, ops._p(x), ops._stream())
        return x

    def _image_features(self, image, normalize, l2):
        """frames [N,3,S,S] -> [N, embed_dim] fp32.  normalize: frames in [0, 1] at any S (clip_similarity's resize + normalise);
        otherwise encode_image's input (normalised, S == R).  Slices of frames_per_pass frames: every kernel is row-independent."""
        image = self._check_image(image, normalize)
        N, D = image.shape[0], self._shape['D']
        vis = self.visual
        E = vis.class_embedding.shape[0]
        out = torch.empty(N, D, device=image.device, dtype=f32)
        per = frames_per_pass((self._shape['R'] // self._shape['P'])**2 + 1)
        for n0 in range(0, N, per):
            n = min(per, N - n0)
            x = self._image_sequence(image[n0:n0 + n], normalize)
            y, _ = vis.tower._run_forward(x, keep=False)
            _lib.call('mmvid_clip_pool_project', ops._p(y), n, y.shape[1], E, None, ops._p(vis.ln_post.weight), ops._p(vis.ln_post.bias),
                      1e-5, ops._p(vis.proj), D, int(l2), ops._p(out[n0:]), ops._stream())
        return out

    def _check_text(self, text):
        L = self._shape['L']
        if text.dim() != 2 or text.shape[1] != L:
            raise ValueError(f'CLIP text input must be int64 [B, {L}], got {tuple(text.shape)}')
        return ops._chk(text.to(torch.int64).contiguous(), torch.int64, 'text')

    def _text_tower(self, text, want_pool):
        text = self._check_text(text)
        B, L = text.shape
        E = self.ln_final.weight.shape[0]
        x = torch.empty(B, L, E, device=text.device, dtype=f32)
        pool = torch.empty(B, device=text.device, dtype=torch.int32) if want_pool else None
        _lib.call('mmvid_clip_text_embed', ops._p(text), B, L, ops._p(self.token_embedding.weight), self._shape['V'],
                  ops._p(self.positional_embedding), E, ops._p(x), ops._p(pool), ops._stream())
        y, _ = self.text_tower._run_forward(x, keep=False)
        return y, pool

    def _text_features(self, text, l2):
        y, pool = self._text_tower(text, want_pool=True)
        B, L, E = y.shape
        D = self._shape['D']
        out = torch.empty(B, D, device=y.device, dtype=f32)
        _lib.call('mmvid_clip_pool_project', ops._p(y), B, L, E, ops._p(pool), ops._p(self.ln_final.weight), ops._p(self.ln_final.bias),
                  1e-5, ops._p(self.text_projection), D, int(l2), ops._p(out), ops._stream())
        return out


def patch_columns(P):
    """Kp: the patch matrix's row length, 3*P*P rounded up to a multiple of 64 (3*P*P itself when P is a multiple of 8)."""
    return -(-3 * P * P // 64) * 64


def frames_per_pass(T):
    """Frames per pass through a visual tower of T = G*G + 1 positions: the rows of IMAGE_SLICE frames at ViT-B/32's T = 50, so the
    tower's scratch stays where it is at any grid (256 frames at T = 50, 49 at 257, 22 at 577)."""
    return max(1, (IMAGE_SLICE * 50) // T)


def patchify(frames, R, P, normalize):
    """frames fp32 [N,3,S,S] -> bf16 [N*(R/P)^2, Kp], columns (c, ky, kx), then zeros up to Kp = patch_columns(P).  normalize: frames
    in [0, 1], resized to R with F.interpolate's `nearest` rule and normalised with CLIP's mean / std (utils/utils.py:66-71);
    otherwise taken as they are (S == R)."""
    frames = ops._chk(frames, f32, 'frames')
    N, S = frames.shape[0], frames.shape[2]
    out = torch.empty(N * (R // P)**2, patch_columns(P), device=frames.device, dtype=bf16)
    if N:
        _lib.call('mmvid_clip_patchify', ops._p(frames), N, S, R, P, int(normalize), ops._p(out), ops._stream())
    return out


# ---- checkpoints ----------------------------------------------------------------------------------------
def build_model(state_dict):
    """clip_model.py:438-497: configuration from the keys and shapes of a CLIP state_dict; fp16 weights become fp32 master
    weights.  Returns the model in eval mode with frozen parameters (inference only)."""
    sd = {k: v for k, v in state_dict.items() if k not in ('input_resolution', 'context_length', 'vocab_size')}
    if 'visual.proj' not in sd:
        raise NotImplementedError('CLIP with a ModifiedResNet image tower (RN50 family) is not implemented: ViT checkpoints only')
    vision_width = sd['visual.conv1.weight'].shape[0]
    vision_layers = len([k for k in sd if k.startswith('visual.') and k.endswith('.attn.in_proj_weight')])
    vision_patch_size = sd['visual.conv1.weight'].shape[-1]
    grid_size = round((sd['visual.positional_embedding'].shape[0] - 1)**0.5)
    embed_dim = sd['text_projection'].shape[1]
    context_length = sd['positional_embedding'].shape[0]
    vocab_size = sd['token_embedding.weight'].shape[0]
    transformer_width = sd['ln_final.weight'].shape[0]
    transformer_layers = len(set(k.split('.')[2] for k in sd if k.startswith('transformer.resblocks')))
    model = CLIP(embed_dim, vision_patch_size * grid_size, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_width // 64, transformer_layers)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.requires_grad_(False)
    return model.eval()


def load(path, device='cuda'):
    """The ViT CLIP of an OpenAI TorchScript archive (ViT-B-32.pt, ViT-B-16.pt, ViT-L-14.pt, ViT-L-14-336px.pt) -- what the reference gets from torch.jit.load(path)
    (utils_eval.py:241) -- on `device`."""
    archive = torch.jit.load(path, map_location='cpu')
    return build_model(archive.state_dict()).to(device)


# ---- the reference's scoring helpers --------------------------------------------------------------------
def _own(model):
    if not isinstance(model, CLIP):
        raise TypeError(f'expected mmvid_amd.clip_model.CLIP (see mmvid_amd.clip_model.load), got {type(model).__name__}')


def _tokens(tokenizer, descriptions, model, device):
    if isinstance(descriptions, str):
        descriptions = [descriptions]
    return tokenizer.tokenize(list(descriptions), model._shape['L'], truncate_text=True).to(device)


def clip_similarity(model, tokenizer, image, description):
    """utils/utils.py:62-85: per-frame cosine similarity of frames [T,3,S,S] in [0, 1] with one description -> numpy [T]
    (or frame t against description t when T descriptions are given)."""
    _own(model)
    model._inference_only(image)
    with torch.no_grad():
        img = model._image_features(image, normalize=True, l2=True)
        txt = model._text_features(_tokens(tokenizer, description, model, img.device), l2=True)
        T = img.shape[0]
        if txt.shape[0] == 1:
            B, per = 1, T
        elif txt.shape[0] == T:
            B, per = T, 1
        else:
            raise ValueError(f'{txt.shape[0]} descriptions for {T} frames: give one, or one per frame')
        out = torch.empty(T, device=img.device, dtype=f32)
        if T:
            _lib.call('mmvid_clip_pair_scores', ops._p(img), ops._p(txt), B, per, img.shape[1], ops._p(out), ops._stream())
        return out.cpu().numpy()


def clip_encode_image(model, image):
    """utils/utils_train.py:283-294: frames [N,3,S,S] in [0, 1] -> L2-normalised image features [N, embed_dim] fp32."""
    _own(model)
    model._inference_only(image)
    with torch.no_grad():
        return model._image_features(image, normalize=True, l2=True)


def clip_score(model, tokenizer, videos, descriptions):
    """Batched clip_similarity: videos [B,T,3,S,S] in [0, 1], descriptions: B strings -> [B, T] fp32 per-frame scores on the
    videos' device, in one pass (evaluate_clip, utils_eval.py:318-319, reports the mean over b of scores[b].max())."""
    _own(model)
    model._inference_only(videos)
    if videos.dim() != 5:
        raise ValueError(f'videos must be [B, T, 3, S, S], got {tuple(videos.shape)}')
    B, T = videos.shape[:2]
    if isinstance(descriptions, str) or len(descriptions) != B:
        raise ValueError(f'clip_score needs one description per video ({B})')
    with torch.no_grad():
        img = model._image_features(videos.reshape(B * T, *videos.shape[2:]), normalize=True, l2=True)
        txt = model._text_features(_tokens(tokenizer, descriptions, model, img.device), l2=True)
        out = torch.empty(B, T, device=img.device, dtype=f32)
        if B * T:
            _lib.call('mmvid_clip_pair_scores', ops._p(img), ops._p(txt), B, T, img.shape[1], ops._p(out), ops._stream())
        return out
