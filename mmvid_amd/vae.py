"""Host-side mirror of mmvid_pytorch/vae.py::VQGanVAE1024 (15-71) -> taming VQModel (vqgan.py:16-75) over the HIP
kernels: same constructor, attributes (`image_size` is mutated by the driver, train.py:183; `num_layers`,
`num_tokens`), methods (`get_codebook_indices`, `decode`, `decode_train`) and the same state_dict keys as
`model.encoder.* / model.decoder.* / model.quantize.embedding.weight / model.quant_conv.* / model.post_quant_conv.*`
(taming/modules/diffusionmodules/model.py:363-582), so published `vqgan.1024.model.ckpt` files load.

Execution (csrc/vqgan.hip, conv.hip, norm.hip, vq.hip): one encode / decode is an op list that vqgan_plan.py plans once per
batch shape and arithmetic mode; this module keeps the parameters, the modes, and the caches of the plans and of the frozen
weights re-laid-out into [Cout][ky][kx][Cin] (refreshed when a parameter changes)."""
import os
from math import sqrt

import torch
from torch import nn

from . import ops, vqgan_plan
from .shadow import Cached

f32 = torch.float32

# mmvid_pytorch/data/vqgan.1024.config.yml
DEFAULT_DDCONFIG = dict(double_z=False, z_channels=256, resolution=256, in_channels=3, out_ch=3, ch=128,
                        ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16, ), dropout=0.0)


class _H(nn.Module):
    """parameter holder"""


def _conv(cin, cout, k):
    h = _H()
    h.weight = nn.Parameter(torch.empty(cout, cin, k, k))
    h.bias = nn.Parameter(torch.empty(cout))
    nn.init.kaiming_uniform_(h.weight, a=sqrt(5))
    bound = 1 / sqrt(cin * k * k)
    nn.init.uniform_(h.bias, -bound, bound)
    return h


def _norm(c):
    h = _H()
    h.weight = nn.Parameter(torch.ones(c))
    h.bias = nn.Parameter(torch.zeros(c))
    return h


def _resblock(cin, cout):
    h = _H()
    h.norm1, h.conv1, h.norm2, h.conv2 = _norm(cin), _conv(cin, cout, 3), _norm(cout), _conv(cout, cout, 3)
    if cin != cout:
        h.nin_shortcut = _conv(cin, cout, 1)
    return h


def _attnblock(c):
    h = _H()
    h.norm, h.q, h.k, h.v, h.proj_out = _norm(c), _conv(c, c, 1), _conv(c, c, 1), _conv(c, c, 1), _conv(c, c, 1)
    return h


def _mid(c):
    h = _H()
    h.block_1, h.attn_1, h.block_2 = _resblock(c, c), _attnblock(c), _resblock(c, c)
    return h


class _Encoder(_H):  # model.py:363-437
    def __init__(self, *, ch, ch_mult, num_res_blocks, attn_resolutions, in_channels, resolution, z_channels,
                 double_z=False, **_):
        super().__init__()
        self.conv_in = _conv(in_channels, ch, 3)
        cur = resolution
        in_mult = (1, ) + tuple(ch_mult)
        self.down = nn.ModuleList()
        for lvl in range(len(ch_mult)):
            d = _H()
            d.block, d.attn = nn.ModuleList(), nn.ModuleList()
            bin_, bout = ch * in_mult[lvl], ch * ch_mult[lvl]
            for _b in range(num_res_blocks):
                d.block.append(_resblock(bin_, bout))
                bin_ = bout
                if cur in attn_resolutions:
                    d.attn.append(_attnblock(bin_))
            if lvl != len(ch_mult) - 1:
                d.downsample = _H()
                d.downsample.conv = _conv(bin_, bin_, 3)
                cur //= 2
            self.down.append(d)
        self.mid = _mid(bin_)
        self.norm_out = _norm(bin_)
        self.conv_out = _conv(bin_, 2 * z_channels if double_z else z_channels, 3)


class _Decoder(_H):  # model.py:469-549
    def __init__(self, *, ch, out_ch, ch_mult, num_res_blocks, attn_resolutions, resolution, z_channels, **_):
        super().__init__()
        n = len(ch_mult)
        bin_ = ch * ch_mult[n - 1]
        cur = resolution // 2**(n - 1)
        self.conv_in = _conv(z_channels, bin_, 3)
        self.mid = _mid(bin_)
        ups = []
        for lvl in reversed(range(n)):
            u = _H()
            u.block, u.attn = nn.ModuleList(), nn.ModuleList()
            bout = ch * ch_mult[lvl]
            for _b in range(num_res_blocks + 1):
                u.block.append(_resblock(bin_, bout))
                bin_ = bout
                if cur in attn_resolutions:
                    u.attn.append(_attnblock(bin_))
            if lvl != 0:
                u.upsample = _H()
                u.upsample.conv = _conv(bin_, bin_, 3)
                cur *= 2
            ups.insert(0, u)
        self.up = nn.ModuleList(ups)
        self.norm_out = _norm(bin_)
        self.conv_out = _conv(bin_, out_ch, 3)


class VQModel(_H):  # vqgan.py:16-53
    def __init__(self, ddconfig, n_embed, embed_dim, **_):
        super().__init__()
        self.ddconfig = dict(ddconfig)
        self.encoder = _Encoder(**ddconfig)
        self.decoder = _Decoder(**ddconfig)
        self.quantize = _H()
        self.quantize.embedding = nn.Embedding(n_embed, embed_dim)
        self.quantize.embedding.weight.data.uniform_(-1.0 / n_embed, 1.0 / n_embed)  # quantize.py:254
        self.quant_conv = _conv(ddconfig['z_channels'], embed_dim, 1)
        self.post_quant_conv = _conv(embed_dim, ddconfig['z_channels'], 1)


class VQGanVAE1024(nn.Module):
    def __init__(self, vae_path=None, image_size=None, ddconfig=None, n_embed=1024, embed_dim=256):
        super().__init__()
        cfg = dict(DEFAULT_DDCONFIG)
        cfg.update(ddconfig or {})
        if image_size:
            cfg['resolution'] = image_size  # vae.py:24-25
        self.model = VQModel(cfg, n_embed, embed_dim)
        if vae_path is not None:
            state = torch.load(vae_path, map_location='cpu')['state_dict']  # vae.py:28-30
            self.model.load_state_dict(state, strict=False)
        self.num_layers = 4
        self.image_size = 256
        self.num_tokens = 1024
        # Arithmetic modes of the encoder / decoder, and what each means for the token indices (measured: the flip census of 40,960 fresh
        # full-size tokens per mode, profiles/r06_flip_census.log, and 2 x 1,024 reference tokens, tests/test_round6_gpu.py):
        #   strict = False   bf16 MFMA operands (training speed): 97.7 % of the reference's tokens; every flip a near-tie of its distances
        #   strict = 'mixed' the ENCODER's 3x3 residual-block convolutions on maps of at least mixed_f16_side pixels a side (the 128x128,
        #                    64x64 and 32x32 levels: 82 % of the multiply-adds) as ONE product of fp16 operands, the rest as 'split':
        #                    99.87 % of the tokens at 1.11x the step -- NOT an exact mode (rounds 4-5 called it one on 448 golden tokens)
        #   strict = 'split' bf16-pair convolutions (3 products per convolution, fp32 accumulate; ~1e-5 of the fp32 result), fp32 residual
        #                    stream / GroupNorm / attention: the reference's tokens except ties at its OWN fp32 resolution (2 in 40,960
        #                    against the fp32 mode; the one golden flip has a top-2 gap of 17 fp32 spacings of the distance); 1.28x
        #   strict = True    fp32 operator (csrc/strict.hip: f32 MFMA, fp64 GroupNorm statistics): every token seen equal; 2.3x
        # (per-layer sensitivity behind 'mixed': tests/sweep_exact_layers.py, profiles/r05_exact_index_layer_sensitivity_sweep.log)
        self.strict = False
        self.mixed_f16_side = 32  # (the error comes from the 128x128 level: 64 -> 32 adds 3 % to max |dz|, the sweep's rows A / B)
        # default (bf16) operator only: 'bf16' = the ENCODER's residual stream between blocks is bf16 too (round 5: the fp32 stream
        # cost 0.3 ms of the training step in stores / GroupNorm reads and bought nothing the default mode promises -- its indices
        # are 97-100 % of the reference's either way); 'bf16_all' = the decoder's as well; 'f32' = fp32
        # residual streams (rounds 1-4)
        self.stream = os.environ.get('MMVID_VQGAN_STREAM', 'bf16')
        self._prep_cache = Cached(self._prep_sources, dict)

    # ---- weight preparation (cached) ----------------------------------------------------------------
    def _prep_sources(self):
        return self.model.parameters()

    def _prepared(self):
        """The dict that _cw / _cw_qkv / _ee / _plan fill: a new, empty one whenever a parameter has changed."""
        return self._prep_cache.get()

    _prep = property(_prepared)  # (the same dict under the attribute name it had before: callers clear it between plans)

    def _cw(self, holder, form='bf16'):
        """conv holder -> (w [Cout_p, taps, Cin_p], bias f32 [Cout_p], Cout), the weights laid out for the kernels of one operator:
        form = 'bf16' | 'f32' | 'pair' | 'f16' (vqgan_plan.conv_weights)."""
        prep = self._prepared()
        k = (id(holder), form)
        if k not in prep:
            prep[k] = vqgan_plan.conv_weights(holder, form)
        return prep[k]

    def _cw_qkv(self, blk):
        """q, k, v 1x1 conv holders of an AttnBlock -> (w bf16 [3C, 1, C], bias f32 [3C])."""
        prep = self._prepared()
        key = (id(blk), 'qkv')
        if key not in prep:
            ws, bs = zip(*[self._cw(hd)[:2] for hd in (blk.q, blk.k, blk.v)])
            prep[key] = (torch.cat(ws, 0).contiguous(), torch.cat(bs, 0).contiguous())
        return prep[key]

    def _ee(self):
        prep = self._prepared()
        if 'ee' not in prep:
            prep['ee'] = ops.vq_sqnorm(self.model.quantize.embedding.weight.detach().contiguous())
        return prep['ee']

    # ---- planning: the op sequence of one encode / decode for a given batch shape (vqgan_plan.py), cached ------------------------
    def _plan(self, kind, n, size_or_hw, slot=0):
        prep = self._prepared()
        mode = 'split' if self.strict in ('split', 'mixed') else bool(self.strict)
        # (the decoder keeps its fp32 stream unless 'bf16_all': it is off the training path and its pixel tolerance is pinned)
        s16 = mode is False and (self.stream == 'bf16_all' or (self.stream == 'bf16' and kind == 'enc'))
        f16_side = self.mixed_f16_side if (self.strict == 'mixed' and kind == 'enc') else 0  # (the decoder stays the pair operator)
        key = ('plan', kind, n, size_or_hw, mode, slot, s16, f16_side)  # (slot: plans that run concurrently need arenas of their own)
        if key not in prep:
            if mode == 'split':
                pl = vqgan_plan.PairPlanner(self, f16_side=f16_side)
            else:
                pl = vqgan_plan.StrictPlanner(self) if mode else vqgan_plan.Bf16Planner(self, stream16=s16)
            if kind == 'enc':
                vqgan_plan.plan_encode(pl, self.model, n, size_or_hw)
            else:
                vqgan_plan.plan_decode(pl, self.model, n, size_or_hw, from_z=kind == 'dec_z')
            prep[key] = pl.finish(next(self.model.parameters()).device)
        return prep[key]

    # ---- reference API ------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_z(self, img):
        """img [N,3,S,S] fp32 in [0,1] -> pre-quantisation z [N, h, w, embed_dim] fp32 (NHWC; a copy)."""
        step, outs = self._max_frames(img.shape[-1]), []
        for i in range(0, max(img.shape[0], 1), step):  # (z lives in the plan's arena: read it back slice by slice)
            _, plan = self._encode(img[i:i + step])
            off, shape = plan.kept['z']
            nbytes = int(torch.tensor(shape).prod()) * 4
            outs.append(plan.arena[off:off + nbytes].view(torch.float32).view(shape).clone())
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _max_frames(self, s):
        """Frames per planned call: the kernels address an operand through 32-bit byte offsets (< 2 GiB per tensor), and the largest operand
        of a plan is a pair of bf16 planes at the full resolution with `ch` channels."""
        ch = self.model.ddconfig['ch']
        return max(1, ((1 << 31) - 1) // (s * s * max(ch, 8) * 4))

    def _encode(self, img):
        img = ops._chk(img.contiguous().float(), f32, 'img')
        n, c, s, s2 = img.shape
        assert c == 3 and s == s2
        idx = torch.empty(n, (s // 16)**2, device=img.device, dtype=torch.int64)
        step = self._max_frames(s)
        plan = None
        for i in range(0, max(n, 1), step):  # (one call for every batch the drivers use; more than 255 full-size frames go in slices)
            m = min(step, n - i)
            plan = self._plan('enc', m, s)
            plan.run(ext_in={'img': img[i:i + m]}, ext_out={'idx': idx[i:i + m]})
        return idx, plan

    @torch.no_grad()
    def get_codebook_indices(self, img):
        """vae.py:38-43: [N,3,S,S] in [0,1] -> [N, (S/16)^2] int64."""
        return self._encode(img)[0]

    def decode(self, img_seq):
        """vae.py:45-56: [N, n] int64 -> [N,3,S,S] fp32 in [0,1]."""
        with torch.no_grad():
            img_seq = ops._chk(img_seq.contiguous(), torch.int64, 'img_seq')
            b, n = img_seq.shape
            hw = int(sqrt(n))
            out = torch.empty(b, 3, hw * 16, hw * 16, device=img_seq.device, dtype=f32)
            step = self._max_frames(hw * 16)
            for i in range(0, b, step):  # (slices of at most 255 full-size frames: 32-bit operand offsets)
                m = min(step, b - i)
                self._plan('dec', m, hw).run(ext_in={'idx': img_seq[i:i + m]}, ext_out={'img': out[i:i + m]})
            return out

    def decode_train(self, probs):
        """vae.py:58-68: probs [B, N, num_tokens] (soft one-hot) @ codebook -> decoder -> [B,3,S,S] in [0,1].
        The soft lookup is the exact-fp32 matrix kernel; the decoder is the planned op list of `decode`.  The VQGAN is
        frozen and no caller of the reference differentiates through it, so this is a forward-only entry point."""
        with torch.no_grad():
            probs = ops._chk(probs.contiguous().float(), f32, 'probs')
            b, n, d = probs.shape
            cb = self.model.quantize.embedding.weight.detach()
            assert d == cb.shape[0], f'probs last dim {d} != codebook size {cb.shape[0]}'
            hw = int(sqrt(n))
            z = ops.gemm_f32(probs.view(b * n, d), cb, b_kmajor=True)  # [b*n, embed_dim] = probs @ codebook
            plan = self._plan('dec_z', b, hw)
            out = torch.empty(b, 3, hw * 16, hw * 16, device=probs.device, dtype=f32)
            plan.run(ext_in={'z': z}, ext_out={'img': out})
            return out

    def forward(self, img):
        raise NotImplementedError  # as the reference (vae.py:70-71)
