"""Host-side mirror of mmvid_pytorch/dalle_artv.py::DALLE (103-542), the autoregressive "ART-V" baseline, over
the HIP kernels: same constructor, state_dict keys, `forward` (logits or (loss, 0, 0)) and `generate_images`
-> (images, [], None).

The reference's block-diagonal vocabulary mask (a [1, L, 51584] bool buffer, dalle_artv.py:215-227, applied with
masked_fill at 509-512) says: text positions predict text ids, visual positions visual ids, image positions image
ids; every other class gets logit -max, i.e. probability exactly 0.  Here that structure is used instead of
materialised: each of the three position segments runs `to_logits` against ITS block of the weight only (LayerNorm +
MFMA GEMM + the fused cross-entropy kernels), which is the same loss with ~14x fewer head FLOPs and no [B, L, 51584]
tensors.  Sampling keeps a per-layer key/value cache (the reference recomputes the whole prefix per token) and draws
tokens with the device sampler of csrc/sample.hip."""
import torch
import torch.nn.functional as F
from torch import nn

from . import artv_sampling, ops, sampling, seeded, token_draw
from .artv_sampling import k_keep, keep_top
from .clip_tower import OpenAICLIPTransformer, check_tower_width
from .dalle_bert import DivideMax, eval_decorator, exists, set_requires_grad
from .frontend import Frontend, check_condition_drop, face_choices
from .functional import AssembleSequence, LNLinear, LNLinearCrossEntropy
from .modules import AxialPositionalEmbedding, AxialPositionalEmbeddingList
from .shadow import Bf16Weight

NEG = -torch.finfo(torch.float32).max


def is_empty(t):
    return t.nelement() == 0


def top_k(logits, thres=0.5):
    """dalle_artv.py:61-67: keep the k = max(int((1 - thres) * n), 1) largest logits of each row, -inf elsewhere."""
    return keep_top(logits, k_keep(thres, logits.shape[-1]))


class DALLE(nn.Module):
    def __init__(self, *, dim, vae, cvae=None, num_text_tokens=10000, text_seq_len=256, loss_img_weight=7,
                 stable=False, which_transformer='none', num_visuals=1, num_targets=1, **kwargs):
        super().__init__()
        assert num_visuals > 0
        image_fmap_size = vae.image_size // (2**vae.num_layers)
        image_seq_len = image_fmap_size**2
        num_image_tokens = vae.num_tokens
        self.dim = dim
        self.target_seq_len = image_seq_len * num_targets
        self.visual_seq_len = image_seq_len * num_visuals
        self.control_seq_len = text_seq_len + self.visual_seq_len
        self.insert_sep = False
        num_text_tokens = num_text_tokens + text_seq_len
        num_visual_tokens = num_image_tokens + self.visual_seq_len
        self.text_emb = nn.Embedding(num_text_tokens, dim)
        self.image_emb = nn.Embedding(num_image_tokens, dim)
        self.text_pos_emb = nn.Embedding(text_seq_len + 1, dim)  # +1 for <bos>
        shape = (image_fmap_size, image_fmap_size) if num_targets == 1 else (num_targets, image_fmap_size, image_fmap_size)
        self.image_pos_emb = AxialPositionalEmbedding(dim, axial_shape=shape)
        self.visual_emb = nn.Embedding(num_visual_tokens, dim)
        self.visual_pos_emb = AxialPositionalEmbeddingList(dim, num_visuals, axial_shape=(image_fmap_size, image_fmap_size))
        self.num_text_tokens, self.num_image_tokens = num_text_tokens, num_image_tokens
        self.num_visual_tokens = num_visual_tokens
        self.num_control_tokens = num_text_tokens + num_visual_tokens
        self.text_seq_len, self.image_seq_len = text_seq_len, image_seq_len
        self.num_visuals, self.num_targets, self.image_fmap_size = num_visuals, num_targets, image_fmap_size
        self.image_size = vae.image_size
        self.special_token_lut = {'[REL]': 0, '[ST1]': 1, '[ST2]': 2, '[ST3]': 3}
        self.num_special_tokens, self.num_estimation_tokens = 4, 2
        self.special_emb = nn.Embedding(self.num_special_tokens, dim)        # unused in forward (as the reference)
        self.estimation_pos_emb = nn.Embedding(self.num_estimation_tokens, dim)  # unused in forward
        self.total_tokens = num_text_tokens + num_image_tokens + num_visual_tokens
        self.total_seq_len = text_seq_len + self.target_seq_len + self.visual_seq_len
        self.vae, self.cvae = vae, cvae
        set_requires_grad(self.vae, False)
        set_requires_grad(self.cvae, False)
        self.which_transformer = which_transformer
        if not which_transformer.startswith('openai_clip'):
            raise NotImplementedError
        # the tower's shape: the checkpoint's where one is given, else transformer_width (heads = width / 64), else the ViT-B/32 table;
        # in the first two cases `dim` must be that width
        tower_width = kwargs.get('transformer_width')
        if tower_width is not None:
            check_tower_width(int(tower_width), 'transformer_width')
        self.transformer = OpenAICLIPTransformer(self.total_seq_len, which_transformer,
                                                 model_path=kwargs.get('openai_clip_path'),
                                                 layers=kwargs.get('transformer_layers'),
                                                 width=None if tower_width is None else int(tower_width),
                                                 heads=None if tower_width is None else int(tower_width) // 64, model_dim=dim)
        self.stable = stable
        if stable:
            self.norm_by_max = DivideMax(dim=-1)
        self.to_logits = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, self.total_tokens))
        self.loss_vis_weight, self.loss_img_weight = 1., loss_img_weight
        self.eraser = dict(p=1.0, scale=(0.4, 0.8), ratio=(0.5, 2.0))  # RandomErasing(value=-1), dalle_artv.py:229-232
        self.frontend = Frontend(seed=kwargs.get('frontend_seed'))
        self._head_bf16 = None  # bf16_weights()
        # (artv_sampling.token_launch_loop: reads the failure flag every so many tokens; tests: hook(tokens launched so far, session) after every launch)
        self._decode_check_every, self._token_step_hook = 64, None
        seg = [0] * (text_seq_len + 1) + [1] * self.visual_seq_len + [2] * self.target_seq_len
        self.register_buffer('_seg', torch.tensor(seg, dtype=torch.int32), persistent=False)

    def half(self):
        """train.py:194-195 (`--fp16`).  The kernels always compute in bf16 on the MFMA pipe over fp32 master weights
        (what mixed precision buys is already in place); fp16 parameters would have no kernel to run on."""
        import warnings
        warnings.warn('mmvid_amd: .half() ignored -- compute is bf16 MFMA over fp32 master weights (fp16 checkpoints still '
                      'load: values are widened on copy)', UserWarning)
        return self

    # ---- the vocabulary blocks --------------------------------------------------------------------------------------
    @property
    def logits_mask(self):
        """The reference's [1, total_seq_len, total_tokens] bool buffer, materialised on demand (tests only)."""
        m = torch.block_diag(torch.ones(self.text_seq_len, self.num_text_tokens),
                             torch.ones(self.visual_seq_len, self.num_visual_tokens),
                             torch.ones(self.target_seq_len, self.num_image_tokens)) == 0
        return m.unsqueeze(0)

    def _segments(self, L):
        """[(first position, end position, first class, end class)] of the block-diagonal mask, clipped to L positions."""
        tl, cl = self.text_seq_len, self.control_seq_len
        segs = [(0, tl, 0, self.num_text_tokens), (tl, cl, self.num_text_tokens, self.num_control_tokens),
                (cl, self.total_seq_len, self.num_control_tokens, self.total_tokens)]
        return [(lo, min(hi, L), c0, c1) for lo, hi, c0, c1 in segs if lo < L]

    def _allowed_range(self, pos):
        """classes position `pos` may predict (dalle_artv.py:215-219)."""
        for lo, hi, c0, c1 in self._segments(self.total_seq_len):
            if lo <= pos < hi:
                return c0, c1
        raise IndexError(pos)

    # ---- bf16 copy of the 51,584 x 768 head ----------------------------------------------------------------------------
    def _w16(self):
        return self.bf16_weights()[0].get()

    def bf16_weights(self):
        """As BERT.bf16_weights, for the one head: its shadow.Bf16Weight, made at first use and again if its Parameter object was replaced."""
        w = self.to_logits[1].weight
        if self._head_bf16 is None or self._head_bf16.param is not w:
            self._head_bf16 = Bf16Weight(w)
        return [self._head_bf16]

    # ---- token helpers (dalle_artv.py:306-416) --------------------------------------------------------------------------
    def get_image_tokens(self, image, reshape=True, insert_sep=False, which_vae='vae'):
        vae = self.cvae if (which_vae == 'cvae' and self.cvae is not None) else self.vae
        if isinstance(image, list):
            image = torch.stack(image, dim=1)
        if len(image.shape) == 4:
            image = image.unsqueeze(1)
        if len(image.shape) == 5:
            b, t, c, h, w = image.shape
            s = vae.image_size
            assert (c, h, w) == (3, s, s), f'invalid image of dimensions {image.shape} passed in during training'
            image = vae.get_codebook_indices(image.reshape(b * t, c, h, w))
            if reshape:
                image = image.view(b, -1)
        return image

    @torch.no_grad()
    def recon_images(self, images, which_vae='vae'):
        """dalle_artv.py:344-354: frames -> tokens -> frames through the (control) VQGAN."""
        vae = self.cvae if (which_vae == 'cvae' and self.cvae is not None) else self.vae
        return vae.decode(self.get_image_tokens(images, reshape=False, which_vae=which_vae))

    def random_erase_codebook(self, image, eraser, erase_half=False):
        f = self.image_fmap_size
        image = image.contiguous()
        return self.frontend.random_erase(image, image.shape[1] // (f * f), f, -1, eraser['p'], eraser['scale'],
                                          eraser['ratio'], erase_half)

    def erase_codebook_face(self, image, vc_mode, face_mode=None):
        """dalle_artv.py:356-416; erased positions become -1 (later replaced by per-position pad ids, 473-477)."""
        f = self.image_fmap_size
        image = image.contiguous()
        if vc_mode == 'face3_8x8':
            raise NotImplementedError(vc_mode)  # BERT-only mode
        choices, frame0 = face_choices(vc_mode, face_mode)
        if vc_mode in ('mask_8x8', 'mask2_8x8') and face_mode is None:
            # the reference builds strategy 2's masked copy but never assigns it (dalle_artv.py:401-404): unchanged
            choices = [(choices[0][0] + choices[1][0], 0, (0, 0, 0, 0)), choices[2]]
        return self.frontend.erase_choice(image, image.shape[1] // (f * f), f, -1, choices, frame0)

    def _visual_tokens(self, visual, erase_visual, erase_visual_half, vc_mode, face_mode, visual_aug_mode):
        if not (exists(visual) and not is_empty(visual)):
            return None
        if visual_aug_mode == 'motion_color' and torch.is_tensor(visual) and visual.dim() == 5:
            # scripts/mmvoxceleb/image_and_video/train.sh:10; dalle_bert.py:940-943 / dalle_artv.py:460-463: colour jitter of the
            # video part (frames 1..) of the visual control, gated at 0.9 per call -- drawn on the device
            visual = self.frontend.visual_color_jitter(visual, 0.9, 1)
        tok = self.get_image_tokens(visual, which_vae='cvae')
        if erase_visual:
            tok = self.random_erase_codebook(tok, self.eraser, erase_visual_half)
        if vc_mode is not None:
            tok = self.erase_codebook_face(tok, vc_mode, face_mode)
        return tok

    # ---- sequence -> hidden states ---------------------------------------------------------------------------------------
    def _prompt_ids(self, text, vis_tok):
        """<bos> + text (0 -> per-position pad id) + visual tokens (-1 -> per-position pad id): dalle_artv.py:441-477."""
        device, B = text.device, text.shape[0]
        assert text.shape[-1] == self.text_seq_len, \
            f'the length {text.shape[-1]} of the text tokens you passed in does not have the correct length ({self.text_seq_len})'
        text_pad = torch.arange(self.text_seq_len, device=device) + (self.num_text_tokens - self.text_seq_len)
        text = F.pad(torch.where(text == 0, text_pad, text), (1, 0), value=0)
        if vis_tok is None:
            vis_tok = torch.full((B, self.visual_seq_len), -1, dtype=torch.long, device=device)
        vis_pad = torch.arange(self.visual_seq_len, device=device) + (self.num_visual_tokens - self.visual_seq_len)
        return text, torch.where(vis_tok == -1, vis_pad, vis_tok)

    def _pos_rows(self):
        return torch.cat([self.text_pos_emb.weight, self.visual_pos_emb.table(), self.image_pos_emb.table()], 0)

    def _hidden(self, text, vis_tok, image):
        text, visual = self._prompt_ids(text, vis_tok)
        parts = [text, visual]
        if exists(image) and not is_empty(image):
            image = self.get_image_tokens(image)
            parts.append(image)
        ids = torch.cat(parts, 1)
        if ids.shape[1] > self.total_seq_len:  # drop the last token when training (dalle_artv.py:496-498)
            ids = ids[:, :-1]
        L = ids.shape[1]
        x = AssembleSequence.apply(self._pos_rows()[:L], ids.contiguous(), self._seg[:L].contiguous(), self.text_emb.weight,
                                   self.visual_emb.weight, self.image_emb.weight)
        out = self.transformer(x)
        if self.stable:
            out = self.norm_by_max(out)
        return out, text, visual, image

    def _logits_rows(self, rows, cols=None):
        lin = self.to_logits[1]
        if cols is None:
            return LNLinear.apply(rows, self.to_logits[0].weight, self.to_logits[0].bias, lin.weight, lin.bias, self._w16())
        with torch.no_grad():  # one class block: inference only (training goes through LNLinearCrossEntropy)
            hn = ops.layernorm_fwd(rows.contiguous(), self.to_logits[0].weight, self.to_logits[0].bias, 1e-5, save_stats=False)[0]
            return ops.gemm(hn, self._w16()[cols[0]:cols[1]], bias=lin.bias.detach()[cols[0]:cols[1]], out_dtype=torch.float32)

    def forward(self, text, visual=None, target=None, return_loss=False, erase_visual=False, erase_visual_half=False,
                vc_mode=None, face_mode=None, visual_aug_mode=None, null_text_prob=0.0, null_visual_prob=0.0, _null=None, **kwargs):
        """`null_text_prob` / `null_visual_prob` (training for classifier-free guidance): each sample's text becomes all pad and its visual
        control all pad ids (what an empty text and visual=None give that sample) with these probabilities, drawn on the device before the
        ids are built (Frontend.cond_drop); the labels of the text and visual segments are the ids after the drop.  `_null` (uint8 [B, 2])
        injects the decisions (tests).  A forward with the drop on advances the front-end's call counter at its end, so the next step
        draws new decisions; both probabilities 0 and no `_null`: nothing is launched and the counter stays."""
        drop = check_condition_drop(null_text_prob, null_visual_prob, False, return_loss, _null is not None)
        vis_tok = self._visual_tokens(visual, erase_visual, erase_visual_half, vc_mode, face_mode, visual_aug_mode)
        if drop:
            text, vis_tok = self.frontend.cond_drop(text.contiguous(), vis_tok.contiguous() if vis_tok is not None else None, null_text_prob,
                                                    null_visual_prob, -1, _null)
        out, text, visual, image = self._hidden(text, vis_tok, target)
        B, L, E = out.shape
        if not return_loss:
            with torch.no_grad():  # the reference's dense [B, L, total_tokens] tensor, -max outside each position's block
                logits = torch.full((B, L, self.total_tokens), NEG, device=out.device, dtype=torch.float32)
                for lo, hi, c0, c1 in self._segments(L):
                    logits[:, lo:hi, c0:c1] = self._logits_rows(out[:, lo:hi].reshape(-1, E), (c0, c1)).view(B, hi - lo, c1 - c0)
            return logits
        assert exists(image), 'when training, image must be supplied'
        # labels (dalle_artv.py:519-524) relative to each segment's class block: text[1:], visual ids, image ids
        labels = (text[:, 1:], visual, image)
        lin, ln = self.to_logits[1], self.to_logits[0]
        losses = []
        for (lo, hi, c0, c1), lab in zip(self._segments(L), labels):
            rows = out[:, lo:hi].reshape(B * (hi - lo), E)
            loss, _ = LNLinearCrossEntropy.apply(rows, lab[:, :hi - lo].reshape(-1).contiguous(), None, ln.weight, ln.bias,
                                                 lin.weight, lin.bias, self._w16(), (c0, c1))
            losses.append(loss)
        loss = (losses[0] + self.loss_vis_weight * losses[1] + self.loss_img_weight * losses[2]) / \
            (self.loss_img_weight + self.loss_vis_weight + 1)
        zero = torch.tensor(0.0, device=text.device)
        if drop:
            self.frontend.advance(text.device)
        return loss, zero, zero

    # ---- sampling ---------------------------------------------------------------------------------------------------------
    def _embed_rows(self, ids, first_pos):
        """Embedding + positional rows for `ids` [B, n] occupying positions first_pos .. first_pos+n-1."""
        n = ids.shape[1]
        return ops.assemble_sequence([self.text_emb.weight, self.visual_emb.weight, self.image_emb.weight], ids.contiguous(),
                                     self._seg[first_pos:first_pos + n].contiguous(),
                                     self._pos_rows()[first_pos:first_pos + n].contiguous())

    def _guidance(self, B, guidance_scale, guidance_drop, negative_text, filter_thres):
        return sampling.check_guidance_artv(self.num_visuals, self.text_seq_len, self.total_tokens, self.num_image_tokens, B, guidance_scale,
                                            guidance_drop, negative_text, filter_thres)

    _scale_vector = staticmethod(sampling.scale_vector)

    @staticmethod
    def _video_trunc(B, V, device, top_k, top_p, temperature, video_top_k, video_top_p, video_temperature):
        """The `trunc` of a call's draws (token_draw): check_truncation_artv's scalar pair or None without the per-video keywords; with one
        of them a token_draw.RowParams over vectors [B] built here, once per call, after every value was checked on the host -- the
        captured step reads them through pointers that stay.  Such a call always runs the per-row launch, whatever the values."""
        video = sampling.check_video_params(video_top_k, video_top_p, video_temperature, B, V, None, top_k, top_p, temperature)
        pair = sampling.check_truncation_artv(top_k, top_p, V)
        if video is None:
            return pair
        k, p = pair or (None, None)
        return token_draw.RowParams(1, *video.device(device), top_k=k, top_p=p)

    def _draw(self, block_logits, filter_thres, temperature, race, name, trunc=None, logits_u=None, scale=None):
        """One token per row from the logits of the position's class block (dalle_artv.py:274-276): top_k over ALL total_tokens classes keeps
        k = int((1 - thres) * total_tokens) of them; the classes outside the block sit at -max, so the filter only ever removes block classes
        when k is smaller than the block.  logits_u (same row stride) with scale (fp32 [B] on the device): the guided draw (token_draw.draw)."""
        B, n = block_logits.shape
        if logits_u is None:
            block_logits = keep_top(block_logits, k_keep(filter_thres, self.total_tokens)).contiguous()
        E = race(name, (B, n)) if race is not None else ops.exponential_like((B, n), block_logits.device)
        return token_draw.draw(block_logits, E, logits_u=logits_u, scale=scale, rows_per_scale=1, trunc=trunc, logit_div=temperature,
                               want_y=False)[0].view(B, 1)

    def sampling_probs(self, block_logits, filter_thres=0.5, temperature=1.0, top_k=None, top_p=None, logits_u=None, guidance_scale=None,
                       video_top_k=None, video_top_p=None, video_temperature=None):
        """The probability vector `_draw` samples from (tests compare it with the reference's full-width expression); with logits_u and
        guidance_scale, of the guided, then truncated, value (both filters off: the guided value is copied through).  video_top_k,
        video_top_p, video_temperature: one value per row (_video_trunc); the value is then divided already where temperatures are given."""
        B, guide = block_logits.shape[0], {}
        trunc = self._video_trunc(B, block_logits.shape[1], block_logits.device, top_k, top_p, temperature, video_top_k, video_top_p,
                                  video_temperature)
        if (logits_u is None) != (guidance_scale is None):
            raise ValueError('sampling_probs: logits_u and guidance_scale come together')
        if logits_u is not None:
            scale = self._scale_vector(self._guidance(B, guidance_scale, sampling.GUIDANCE_DROPS, None, filter_thres)[1], B, block_logits.device)
            guide = dict(logits_u=logits_u.contiguous(), scale=scale, rows_per_scale=1)
        else:
            block_logits = keep_top(block_logits, k_keep(filter_thres, self.total_tokens))
        lg = token_draw.race_value(block_logits.contiguous(), trunc=trunc, logit_div=temperature, materialise=True, **guide)[0]
        return F.softmax(lg / token_draw.race_div(trunc, temperature), dim=-1)

    @torch.no_grad()
    @eval_decorator
    def generate_images(self, text, *, clip=None, visual=None, mask=None, filter_thres=0.5, temperature=1.,
                        erase_visual=False, vc_mode=None, face_mode=None, use_cache=True, top_k=None, top_p=None, guidance_scale=None,
                        guidance_drop=sampling.GUIDANCE_DROPS, negative_text=None, given=None, seeds=None, video_top_k=None, video_top_p=None,
                        video_temperature=None, _race=None, _trace=None, **kwargs):
        """dalle_artv.py:236-304.  use_cache=True (default): the prompt runs once and every sampled token costs one
        incremental step over the per-layer key/value cache; use_cache=False: the reference's algorithm (the whole
        transformer over the growing prefix per token).  Both draw from the same distribution: softmax over the image
        block of the last position's logits (tests/test_parity_gpu.py compares it with the reference's expression).
        `top_k` (an int) / `top_p` (a float in (0, 1]) truncate that distribution, after whatever `filter_thres` did, to its k most
        likely classes / to its nucleus of mass top_p, with defined ties (ops.logits_truncate): one more launch per token, captured
        with the step.

        `guidance_scale` (a finite float, or a tensor [B] with one scale per video; None: the unguided call) switches classifier-free
        guidance on: every token is drawn from lc + w * (lc - lu), lu the logits under an unconditional prompt that runs beside the
        conditional one as rows B..2B-1 of the same prefill, cache and decode step and receives the same drawn tokens.  That prompt
        lacks what `guidance_drop` names ('text': all pad; 'visual': every slot its pad id) and takes `negative_text` (int64
        [B, text_seq_len]) for its text when given.  top_k / top_p then truncate the guided distribution.  Not accepted with guidance: a
        per-token scale schedule, and a `filter_thres` that removes image classes.  `_trace` (a list, cached path): one dict of clones
        per token (artv_sampling.sample), through the eager loop with per-token variates.

        `given` = (mask, tokens): video prediction.  mask ([B, T] or [T], bool or uint8) names the known frames of each video, tokens
        (int64 [B, T * n]) holds them; values under a 0 mask are ignored.  Known frames come back as they are, and every generated frame
        is conditioned on the known and generated frames BEFORE it (the model is causal: a known frame says nothing to the frames in
        front of it).  Rows with the same mask run together, one pass through artv_sampling.sample_given per distinct mask; the visual
        tokens are computed once for the whole batch.  Under guidance both branches carry the same known and drawn tokens.  Known
        positions draw nothing: `_race` is asked for `tok{j}` of the generated positions j of the target sequence only, `_trace` gets
        records of those only, and both need one mask for the whole batch.

        `seeds` (a sequence or integer tensor of B values in [0, 2^63), one per video; guided: still one per video): every token race
        draws variates that are a function of the video's seed and the token's index in the target sequence (mmvid_amd/seeded.py), not of
        torch's generator, the row or the batch; several masks in one batch are fine.  Refused with `_race` and with erase_visual.

        `video_top_k`, `video_top_p`, `video_temperature` (a sequence or tensor of B entries each; sampling.check_video_params): top_k,
        top_p and temperature per video, so that requests with different settings share one batch.  0 / 1.0 / None entries switch a
        filter off for their video; video_temperature replaces `temperature` (which stays 1).  The vectors live on the device for the
        call and ONE ops.logits_truncate_rows per token reads them (it also divides by the video's temperature, and the race then
        divides by 1): the call takes the separate launches at every batch size, captured as usual.  Under `given`, every group of
        rows takes the entries of its rows.  No per-token schedule."""
        return self._decode_tokens(*self.sample_tokens(text, visual=visual, filter_thres=filter_thres, temperature=temperature,
                                                       erase_visual=erase_visual, vc_mode=vc_mode, face_mode=face_mode, use_cache=use_cache,
                                                       top_k=top_k, top_p=top_p, guidance_scale=guidance_scale, guidance_drop=guidance_drop,
                                                       negative_text=negative_text, given=given, seeds=seeds, video_top_k=video_top_k,
                                                       video_top_p=video_top_p, video_temperature=video_temperature, _race=_race,
                                                       _trace=_trace), clip)

    def _decode_tokens(self, text, tokens, clip=None):
        """The tail of generate_images: tokens [B, target_seq_len] -> (images, [], None), or (images, clip scores)."""
        images = self.vae.decode(tokens.reshape(-1, self.image_seq_len))
        if self.num_targets > 1:
            images = images.view(-1, self.num_targets, *images.shape[1:])
        if exists(clip):
            out = torch.cat((text, tokens + self.num_control_tokens), dim=-1)
            return images, clip(out[:, :self.text_seq_len], images, return_loss=False)
        return images, [], None

    @torch.no_grad()
    @eval_decorator
    def sample_tokens(self, text, *, visual=None, filter_thres=0.5, temperature=1., erase_visual=False, vc_mode=None, face_mode=None,
                      use_cache=True, top_k=None, top_p=None, guidance_scale=None, guidance_drop=sampling.GUIDANCE_DROPS, negative_text=None,
                      given=None, seeds=None, video_top_k=None, video_top_p=None, video_temperature=None, _race=None, _trace=None,
                      _substream=None):
        """The sampler of generate_images without the decode -> (text [B, text_seq_len], tokens int64 [B, target_seq_len]).
        `_substream` (one int per video, with `seeds`): the window of a long video (long_video.window_substream)."""
        tsl = self.text_seq_len
        text = text[:, :tsl]
        B = text.shape[0]
        seeds = seeded.check_seeds(seeds, B, race=_race, erase_visual=erase_visual)
        groups = None
        if given is not None:
            gmask, gtok = artv_sampling.check_given(given, B, self.num_targets, self.image_seq_len, self.num_image_tokens)
            groups = artv_sampling.group_rows(gmask)
            if len(groups) > 1 and (_race is not None or _trace is not None):
                raise ValueError(f'_race / _trace follow one pass through the token loop: {len(groups)} distinct masks in the batch')
            if not gmask.any():  # nothing known: the call without `given`
                groups = None
        guide = self._guidance(B, guidance_scale, guidance_drop, negative_text, filter_thres)
        trunc = self._video_trunc(B, self.num_image_tokens, text.device, top_k, top_p, temperature, video_top_k, video_top_p, video_temperature)
        if _trace is not None and not use_cache:
            raise ValueError('_trace records the token loop over the key/value cache: use_cache=True')
        if groups is not None and all(all(p) for p, _ in groups):  # everything known: no tower work
            return text, gtok.to(text.device).clone()
        # visual control tokens (with the erasing the reference applies on every step, dalle_artv.py:464-472) are fixed
        # during sampling: tokenise once
        vis_tok = self._visual_tokens(visual, erase_visual, True, vc_mode, face_mode, None)
        scale = None
        text_c = text
        race = seeded.SeededRace(seeds, text.device, _substream) if seeds is not None else None
        if guide is not None:  # rows B..2B-1: the unconditional prompt (both branches share the erase and the face region of vis_tok)
            drop, scale = guide[0], self._scale_vector(guide[1], B, text.device)
            text_u, vis_u = sampling.unconditional_inputs(text, vis_tok, drop, negative_text[:, :tsl] if negative_text is not None else None)
            if vis_tok is not None and vis_u is None:
                vis_u = torch.full_like(vis_tok, -1)
            text, vis_tok = torch.cat((text, text_u), 0), (torch.cat((vis_tok, vis_u), 0) if vis_tok is not None else None)
        if groups is None:
            return text_c, self._sample_rows(text, vis_tok, B, None, None, filter_thres, temperature, use_cache, trunc, scale, _race, _trace, race)
        gtok = gtok.to(text.device)
        parts = []
        for pattern, rows in groups:
            if len(groups) == 1:
                t, v, s, g = text, vis_tok, scale, gtok
            else:  # this mask's rows of the batch (guided: of both halves)
                idx = torch.tensor(rows, dtype=torch.long, device=text.device)
                sel = idx if guide is None else torch.cat((idx, idx + B))
                t, v, g = text.index_select(0, sel), (vis_tok.index_select(0, sel) if vis_tok is not None else None), gtok.index_select(0, idx)
                s = scale.index_select(0, idx).contiguous() if scale is not None else None
            tr = trunc.rows(idx) if isinstance(trunc, token_draw.RowParams) and len(groups) > 1 else trunc
            parts.append((rows, self._sample_rows(t, v, len(rows), pattern, g, filter_thres, temperature, use_cache, tr, s, _race, _trace,
                                                  race if race is None or len(groups) == 1 else race.rows(rows))))
        return text_c, artv_sampling.scatter_rows(parts, B)

    def _sample_rows(self, text, vis_tok, B, pattern, known, filter_thres, temperature, use_cache, trunc, scale, _race, _trace, seeded_race=None):
        """Tokens [B, target_seq_len] for prompts that share one frame mask `pattern` (None: nothing known).  text / vis_tok: B rows, or
        [conditional; unconditional] = 2B rows with `scale`.  seeded_race: the seeded.SeededRace of these B videos."""
        rows = text.shape[0]
        cl = self.control_seq_len
        c0, c1 = self._allowed_range(cl)
        if use_cache:
            prompt = torch.cat(self._prompt_ids(text, vis_tok), 1)  # <bos> text visual: positions 0 .. cl
            if pattern is not None:
                return artv_sampling.sample_given(self, prompt, pattern, known, filter_thres, temperature, _race, trunc, scale, _trace, seeded_race)
            cache = self.transformer.new_kv_cache(rows, self.total_seq_len, text.device)
            h = self.transformer.prefill(self._embed_rows(prompt, 0), cache)[:, -1, :].contiguous()
            return torch.cat(artv_sampling.sample(self, h, cache, prompt.shape[1], filter_thres, temperature, _race, trunc, scale, _trace,
                                                  seeded=seeded_race), dim=-1)
        if seeded_race is not None:  # (the uncached path asks its hook per token: the seeded hook answers to the same names)
            _race = seeded_race
        n = self.image_seq_len
        image = torch.empty(rows, 0, dtype=torch.long, device=text.device)
        runs = artv_sampling.segments(pattern) if pattern is not None else [(False, 0, self.num_targets)]
        for k, f0, nf in runs:
            if k:  # known frames are appended, nothing is drawn
                image = torch.cat((image, known[:, f0 * n:(f0 + nf) * n].repeat(rows // B, 1)), dim=-1)
                continue
            for step in range(f0 * n, (f0 + nf) * n):
                hidden = self._hidden(text, vis_tok, image)[0]
                logits = self._logits_rows(hidden[:, -1, :].contiguous(), (c0, c1))
                sample = self._draw(logits[:B], filter_thres, temperature, _race, f'tok{step}', trunc, logits[B:] if scale is not None else None,
                                    scale)
                image = torch.cat((image, sample if scale is None else sample.repeat(2, 1)), dim=-1)  # (both halves carry the same tokens)
        return image[:B]
