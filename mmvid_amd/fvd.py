"""FVD and PRD evaluation (`test.py --eval_mode eval --eval_metric fvd_prd`, utils/utils_eval.py:32-219) over the native I3D of
csrc/i3d.hip.

The reference embeds every real and generated clip with DeepMind's I3D (RGB, Kinetics-400) as a TF-Hub graph under tensorflow.compat.v1
(frechet_video_distance.py) and scores the embeddings with tfgan's Frechet distance and precision_recall_distributions/prd_score.py.
Here the network is `InceptionI3d`, with the state_dict layout of the common converted FVD checkpoints (pytorch_i3d's InceptionI3d,
`i3d_pretrained_400.pt`); its forward runs on the kernels of csrc/i3d.hip: a fused extend / resize / rescale preprocess, every Unit3D
as an implicit-GEMM 3-D convolution with BatchNorm folded in (NDHWC bf16, fp32 accumulate), TF-SAME max pooling and an fp32 head.
The Frechet distance and PRD run on the host (400 x 400 and 20-bin histograms: not the hot path).

Inference only; nothing here downloads: checkpoints are local files or state_dicts."""
import ctypes
import os
import pickle

import numpy as np
import torch
from torch import nn

from . import _lib, ops
from . import prd_score as prd
from .shadow import Cached

bf16, f32 = torch.bfloat16, torch.float32

# Inception blocks: (name, c0, c1, c2, c3, c4, c5); each follows the layer before it
INCEPTION = [('Mixed_3b', 64, 96, 128, 16, 32, 32), ('Mixed_3c', 128, 128, 192, 32, 96, 64),
             ('Mixed_4b', 192, 96, 208, 16, 48, 64), ('Mixed_4c', 160, 112, 224, 24, 64, 64),
             ('Mixed_4d', 128, 128, 256, 24, 64, 64), ('Mixed_4e', 112, 144, 288, 32, 64, 64),
             ('Mixed_4f', 256, 160, 320, 32, 128, 128), ('Mixed_5b', 256, 160, 320, 32, 128, 128),
             ('Mixed_5c', 384, 192, 384, 48, 128, 128)]
# the max pool in front of a block (kernel, stride), pytorch_i3d's MaxPool3d_4a_3x3 / MaxPool3d_5a_2x2
POOL_BEFORE = {'Mixed_4b': ((3, 3, 3), (2, 2, 2)), 'Mixed_5b': ((2, 2, 2), (2, 2, 2))}
BN_EPS = 1e-3
MIN_FRAMES = 9  # fewer leave less than 2 time steps for the (2, 7, 7) VALID average pool


def same_pad(n, k, s):
    """TF "SAME" padding of one dimension of size n: (front, back)."""
    pad = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
    return pad // 2, pad - pad // 2


class Unit3D(nn.Module):
    """conv3d (no bias) + BatchNorm3d(eps 1e-3) + ReLU; the logits layer has a conv bias and neither BN nor ReLU."""

    def __init__(self, cin, cout, k=(1, 1, 1), bn=True):
        super().__init__()
        self.conv3d = nn.Conv3d(cin, cout, k, bias=not bn)
        self.bn = nn.BatchNorm3d(cout, eps=BN_EPS, momentum=0.01) if bn else None


class InceptionModule(nn.Module):
    def __init__(self, cin, c):
        super().__init__()
        self.b0 = Unit3D(cin, c[0])
        self.b1a = Unit3D(cin, c[1])
        self.b1b = Unit3D(c[1], c[2], (3, 3, 3))
        self.b2a = Unit3D(cin, c[3])
        self.b2b = Unit3D(c[3], c[4], (3, 3, 3))
        self.b3b = Unit3D(cin, c[5])


class InceptionI3d(nn.Module):
    """The RGB I3D of the FVD: `forward(videos)` takes preprocessed clips [B, T, 224, 224, 3] in [-1, 1] (fp32, on the device) and
    returns the 400 Kinetics logits averaged over time, [B, 400] fp32 -- `RGB/inception_i3d/Mean:0` of the TF-Hub graph.  `embed`
    takes the reference's [n, t, 3, h, w] in [0, 1] and runs the fused preprocess."""

    def __init__(self, num_classes=400, in_channels=3):
        super().__init__()
        if in_channels != 3:
            raise NotImplementedError('only the RGB stream (in_channels=3) is built; the flow stream is out of scope')
        self.num_classes = num_classes
        self.Conv3d_1a_7x7 = Unit3D(3, 64, (7, 7, 7))
        self.Conv3d_2b_1x1 = Unit3D(64, 64)
        self.Conv3d_2c_3x3 = Unit3D(64, 192, (3, 3, 3))
        cin = 192
        for name, *c in INCEPTION:
            self.add_module(name, InceptionModule(cin, c))
            cin = c[0] + c[2] + c[4] + c[5]
        self.logits = Unit3D(cin, num_classes, bn=False)
        self._shadow, self._arenas = Cached(self._shadow_sources, self._build_shadow), {}

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def fold_bn(unit):
        """(W * s, beta - mean * s) with s = gamma / sqrt(var + eps), fp32: the eval-mode BatchNorm folded into the convolution."""
        w = unit.conv3d.weight.detach().float()
        bn = unit.bn
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        return w * s.view(-1, 1, 1, 1, 1), bn.bias.detach().float() - bn.running_mean.detach().float() * s

    def _shadow_sources(self):
        return list(self.parameters()) + list(self.buffers())

    def _build_shadow(self):
        """bf16 weights [Cout][kt][kh][kw][Cin] with BatchNorm folded in and fp32 biases, built on first use (and again only when a
        parameter or buffer changes: self._shadow).  The stem's is [64][7][7][24]: (kw, c) folded into the channel axis as the preprocess
        writes it; the three 1x1x1 branches of a block that read its input (b0, b1a, b2a) are one weight [c0 + c1 + c3][Cin]."""
        def lay(w):
            return ops.cast_bf16(w.permute(0, 2, 3, 4, 1).contiguous())

        def unit(u):
            w, b = self.fold_bn(u)
            return lay(w), b.contiguous()

        sh = {}
        w, b = self.fold_bn(self.Conv3d_1a_7x7)
        ws = w.permute(0, 2, 3, 4, 1).reshape(64, 7, 7, 21)
        sh['stem'] = (ops.cast_bf16(torch.nn.functional.pad(ws, (0, 3)).contiguous()), b.contiguous())
        sh['2b'], sh['2c'] = unit(self.Conv3d_2b_1x1), unit(self.Conv3d_2c_3x3)
        for name, *_ in INCEPTION:
            m = getattr(self, name)
            f = [self.fold_bn(u) for u in (m.b0, m.b1a, m.b2a)]
            sh[name + '.a'] = (lay(torch.cat([x[0] for x in f])), torch.cat([x[1] for x in f]).contiguous())
            sh[name + '.b1b'], sh[name + '.b2b'], sh[name + '.b3b'] = unit(m.b1b), unit(m.b2b), unit(m.b3b)
        sh['logits'] = (self.logits.conv3d.weight.detach().float().reshape(self.num_classes, -1).contiguous(),
                        self.logits.conv3d.bias.detach().float().contiguous())
        return sh

    # ---- plan ------------------------------------------------------------------------------------------------------------------
    def _arena(self, B, T, dev):
        """Per (batch, frames): the layer plan and its activation buffers (allocated once)."""
        k = (B, T, str(dev))
        if k in self._arenas:
            return self._arenas[k]
        if T < MIN_FRAMES:
            raise ValueError(f'I3D needs at least {MIN_FRAMES} frames, got {T}')
        bufs, plan = {}, []

        def buf(name, shape):
            bufs[name] = torch.empty(shape, device=dev, dtype=bf16)
            return name

        def conv(src, dims, cin, wkey, k, s, segs, pads=None):
            t, h, w = dims
            if pads is None:
                pads = [same_pad(n, kk, ss) for n, kk, ss in zip(dims, k, s)]
            out = tuple((n + p0 + p1 - kk) // ss + 1 for n, (p0, p1), kk, ss in zip(dims, pads, k, s))
            plan.append(('conv', src, (t, h, w, cin), wkey, k, s, pads, segs))
            return out

        def pool(src, dims, c, k, s, dst, ldo=None, c_off=0):
            pads = [same_pad(n, kk, ss) for n, kk, ss in zip(dims, k, s)]
            out = tuple(-(-n // ss) for n, ss in zip(dims, s))
            plan.append(('pool', src, dims, c, k, s, pads, dst, ldo or c, c_off))
            return out

        d0 = (T, 224, 112)
        bufs['x'] = torch.empty(B, T, 224, 112, 24, device=dev, dtype=bf16)
        d1 = tuple(-(-n // 2) for n in (T, 224)) + (112, )
        buf('stem', (B, *d1, 64))
        conv('x', d0, 24, 'stem', (7, 7, 1), (2, 2, 1), [('stem', 64, 0, 64)],
             pads=[same_pad(T, 7, 2), same_pad(224, 7, 2), (0, 0)])
        d = (d1[0], 56, 56)
        buf('p1', (B, *d, 64))
        pool('stem', d1, 64, (1, 3, 3), (1, 2, 2), 'p1')
        buf('c2b', (B, *d, 64))
        conv('p1', d, 64, '2b', (1, 1, 1), (1, 1, 1), [('c2b', 64, 0, 64)])
        buf('c2c', (B, *d, 192))
        conv('c2b', d, 64, '2c', (3, 3, 3), (1, 1, 1), [('c2c', 192, 0, 192)])
        d2 = (d[0], 28, 28)
        buf('p2', (B, *d2, 192))
        pool('c2c', d, 192, (1, 3, 3), (1, 2, 2), 'p2')
        src, d, cin = 'p2', d2, 192
        for name, c0, c1, c2, c3, c4, c5 in INCEPTION:
            if name in POOL_BEFORE:
                k, s = POOL_BEFORE[name]
                dn = tuple(-(-n // ss) for n, ss in zip(d, s))
                pool(src, d, cin, k, s, buf(name + '.in', (B, *dn, cin)))
                src, d = name + '.in', dn
            ct = c0 + c2 + c4 + c5
            out = buf(name, (B, *d, ct))
            t1, t2, tp = buf(name + '.t1', (B, *d, c1)), buf(name + '.t2', (B, *d, c3)), buf(name + '.tp', (B, *d, cin))
            conv(src, d, cin, name + '.a', (1, 1, 1), (1, 1, 1), [(out, c0, 0, ct), (t1, c0 + c1, 0, c1), (t2, c0 + c1 + c3, 0, c3)])
            conv(t1, d, c1, name + '.b1b', (3, 3, 3), (1, 1, 1), [(out, c2, c0, ct)])
            conv(t2, d, c3, name + '.b2b', (3, 3, 3), (1, 1, 1), [(out, c4, c0 + c2, ct)])
            pool(src, d, cin, (3, 3, 3), (1, 1, 1), tp)
            conv(tp, d, cin, name + '.b3b', (1, 1, 1), (1, 1, 1), [(out, c5, c0 + c2 + c4, ct)])
            src, cin = out, ct
        if d[1:] != (7, 7) or d[0] < 2:
            raise ValueError(f'I3D head needs a [>= 2, 7, 7] map, got {d}')
        arena = dict(bufs=bufs, plan=plan, head=(src, d[0], cin), B=B, T=T)
        self._arenas[k] = arena
        return arena

    def _run(self, arena):
        self._run_plan(arena, arena['plan'])
        return self._head(arena)

    def _run_plan(self, arena, plan):
        sh = self._shadow.get()
        bufs, B, st = arena['bufs'], arena['B'], ops._stream()
        for op in plan:
            if op[0] == 'conv':
                _, src, (t, h, w, cin), wkey, k, s, pads, segs = op
                wt, bias = sh[wkey]
                cfg = _lib.Conv3dCfg()
                cfg.N, cfg.T, cfg.H, cfg.W, cfg.Cin, cfg.Cout = B, t, h, w, cin, segs[-1][1]
                cfg.kt, cfg.kh, cfg.kw = k
                cfg.st, cfg.sh, cfg.sw = s
                (cfg.pt0, cfg.pt1), (cfg.ph0, cfg.ph1), (cfg.pw0, cfg.pw1) = pads
                cfg.relu, cfg.nseg = 1, len(segs)
                for i, (dst, end, c_off, ldo) in enumerate(segs):
                    cfg.seg_end[i], cfg.c_off[i], cfg.ldo[i], cfg.out[i] = end, c_off, ldo, bufs[dst].data_ptr()
                _lib.call('mmvid_conv3d_ndhwc', ctypes.byref(cfg), ops._p(bufs[src]), ops._p(wt), ops._p(bias), st)
            else:
                _, src, (t, h, w), c, k, s, pads, dst, ldo, c_off = op
                _lib.call('mmvid_maxpool3d_ndhwc', ops._p(bufs[src]), B, t, h, w, c, *k, *s, *pads[0], *pads[1], *pads[2],
                          ops._p(bufs[dst]), ldo, c_off, st)

    def _head(self, arena):
        bufs, B, st = arena['bufs'], arena['B'], ops._stream()
        src, To, C = arena['head']
        wl, bl = self._shadow.get()['logits']
        out = torch.empty(B, self.num_classes, device=bufs[src].device, dtype=f32)
        _lib.call('mmvid_i3d_head', ops._p(bufs[src]), B, To, C, ops._p(wl), ops._p(bl), self.num_classes, ops._p(out), st)
        return out

    # ---- public ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, videos):
        """videos: preprocessed [B, T, 224, 224, 3] fp32 in [-1, 1] on the device -> [B, num_classes] fp32."""
        ops._chk(videos, f32, 'videos')
        if videos.dim() != 5 or tuple(videos.shape[2:]) != (224, 224, 3):
            raise ValueError(f'videos must be [B, T, 224, 224, 3], got {tuple(videos.shape)}')
        B, T = videos.shape[:2]
        arena = self._arena(B, T, videos.device)
        _lib.call('mmvid_i3d_fold', ops._p(videos), B, T, ops._p(arena['bufs']['x']), ops._stream())
        return self._run(arena)

    @torch.no_grad()
    def embed(self, videos01, video_length):
        """The reference's per-batch path (utils_eval.py:214-225): videos01 [n, t, 3, h, w] fp32 in [0, 1] on the device; clips shorter
        than video_length are extended (extend_video), then cut to video_length frames, resized to 224^2 and embedded."""
        ops._chk(videos01, f32, 'videos')
        if videos01.dim() != 5 or videos01.shape[2] != 3:
            raise ValueError(f'videos must be [n, t, 3, h, w], got {tuple(videos01.shape)}')
        n, t, _, h, w = videos01.shape
        if t < video_length and t < 2:
            raise ValueError(f'a clip of {t} frame cannot be extended to {video_length}')
        arena = self._arena(n, video_length, videos01.device)
        _lib.call('mmvid_i3d_preprocess', ops._p(videos01), n, t, h, w, video_length, ops._p(arena['bufs']['x']), ops._stream())
        return self._run(arena)

    def flops(self, T=16):
        """Algorithmic FLOPs of one clip of T frames (2 M Cout K per convolution, stem K = 7^3 * 3)."""
        total, t = 0, T
        t1 = -(-t // 2)
        total += 2 * t1 * 112 * 112 * 64 * 343 * 3
        hw = 56 * 56
        total += 2 * t1 * hw * 64 * 64 + 2 * t1 * hw * 192 * 27 * 64
        d, hw, cin = t1, 28 * 28, 192
        for name, c0, c1, c2, c3, c4, c5 in INCEPTION:
            if name == 'Mixed_4b':
                d, hw = -(-d // 2), 14 * 14
            if name == 'Mixed_5b':
                d, hw = -(-d // 2), 7 * 7
            m = d * hw
            total += 2 * m * (cin * (c0 + c1 + c3 + c5) + 27 * (c1 * c2 + c3 * c4))
            cin = c0 + c2 + c4 + c5
        return total + 2 * (d - 1) * cin * self.num_classes


def load_i3d(path_or_state_dict, device=None):
    """InceptionI3d from a local checkpoint file or a bare state_dict (strict: a missing, extra or mis-shaped key raises)."""
    sd = path_or_state_dict
    if isinstance(sd, (str, os.PathLike)):
        sd = torch.load(sd, map_location='cpu', weights_only=True)
    model = InceptionI3d()
    model.load_state_dict(sd, strict=True)
    model.requires_grad_(False).eval()
    return model.to(device) if device is not None else model


# ---- mirrors of the reference ----------------------------------------------------------------------------------------------------
@torch.no_grad()
def extend_video(video, num=2):
    """utils_eval.py:18-29: [n, t, ...] -> the clip, then alternately the time-flipped clip and the clip, each without its first
    frame, num pieces in all."""
    parts, flipped = [video], torch.flip(video, [1])
    for i in range(1, num):
        parts.append((video if i % 2 == 0 else flipped)[:, 1:])
    return torch.cat(parts, dim=1)


def resize_bilinear_legacy(v, size):
    """tf.image.resize_bilinear (TF1: align_corners=False, half_pixel_centers=False) of [..., h, w, c] fp32, as a host / torch
    restatement: src = dst * in / out, lo = floor(src), hi = min(lo + 1, in - 1), lerp in x then y."""
    h, w = v.shape[-3], v.shape[-2]
    oh, ow = size

    def axis(n_in, n_out):
        src = torch.arange(n_out, dtype=torch.float32) * torch.tensor(np.float32(n_in) / np.float32(n_out))
        lo = torch.floor(src)
        return lo.long(), torch.clamp(lo.long() + 1, max=n_in - 1), src - lo

    ylo, yhi, ly = axis(h, oh)
    xlo, xhi, lx = axis(w, ow)
    dev = v.device
    ylo, yhi, ly, xlo, xhi, lx = (a.to(dev) for a in (ylo, yhi, ly, xlo, xhi, lx))
    rows_lo, rows_hi = v.index_select(-3, ylo), v.index_select(-3, yhi)
    lx = lx.view(-1, 1)
    top = rows_lo.index_select(-2, xlo) + (rows_lo.index_select(-2, xhi) - rows_lo.index_select(-2, xlo)) * lx
    bot = rows_hi.index_select(-2, xlo) + (rows_hi.index_select(-2, xhi) - rows_hi.index_select(-2, xlo)) * lx
    return top + (bot - top) * ly.view(-1, 1, 1)


def preprocess(videos, target_resolution):
    """frechet_video_distance.py:34-52 restated in torch fp32: videos [b, t, h, w, c] in [0, 255] -> resized to target_resolution
    (TF1 legacy bilinear) and scaled to 2 v / 255 - 1.  The evaluation path fuses this into one kernel (InceptionI3d.embed); this form
    is the readable statement of the contract and a check on it."""
    v = resize_bilinear_legacy(videos.float(), target_resolution)
    return 2. * v / 255. - 1


def create_id3_embedding(model, videos):
    """frechet_video_distance.py:55-83: the I3D logits (before softmax) of preprocessed [B, T, 224, 224, 3] clips in [-1, 1]."""
    return model(videos)


def _sqrtm_sym(mat, eps=1e-10):
    """tfgan's _symmetric_matrix_square_root: SVD, singular values below eps left unrooted."""
    u, s, vh = np.linalg.svd(mat)
    si = np.where(s < eps, s, np.sqrt(s))
    return (u * si) @ vh


def calculate_fvd(real_activations, generated_activations):
    """frechet_video_distance.py:86-99 = tfgan.eval.frechet_classifier_distance_from_activations, restated in float64 on the host:
    |mu_r - mu_f|^2 + tr(S_r) + tr(S_f) - 2 tr(sqrt(sqrt(S_r) S_f sqrt(S_r))), unbiased covariances.  (tfgan returns the value in
    the activations' dtype: FvdPrdEvaluator writes it as float32, as the reference does.)"""
    a = np.asarray(real_activations, dtype=np.float64)
    b = np.asarray(generated_activations, dtype=np.float64)
    ma, mb = a.mean(0), b.mean(0)
    sa = (a - ma).T @ (a - ma) / (a.shape[0] - 1)
    sb = (b - mb).T @ (b - mb) / (b.shape[0] - 1)
    r = _sqrtm_sym(sa)
    tr_sqrt = np.trace(_sqrtm_sym(r @ sb @ r))
    return float(np.trace(sa) + np.trace(sb) - 2.0 * tr_sqrt + np.sum((ma - mb) ** 2))


class FvdPrdEvaluator:
    """The accumulation and scoring of utils_eval.evaluate without its TF session.  `add(real, fake)` embeds one batch of each
    ([n, t, 3, h, w] fp32 in [0, 1], on the device); `finish()` writes real_embs.npy, fake_embs.npy, fvd_score.txt, prd_data.pkl and
    prd_score.txt into output_dir in the reference's formats and returns (fvd, (f_beta, f_beta_inv)).  `seed` (optional) is passed to
    the k-means of PRD as random_state."""

    def __init__(self, i3d, video_length, output_dir, seed=None):
        self.i3d, self.video_length, self.output_dir, self.seed = i3d, video_length, str(output_dir), seed
        self.real, self.fake = [], []

    def add(self, real, fake):
        if real.shape != fake.shape:
            raise ValueError(f'real {tuple(real.shape)} and fake {tuple(fake.shape)} batches differ')
        self.real.append(self.i3d.embed(real, self.video_length))
        self.fake.append(self.i3d.embed(fake, self.video_length))

    def finish(self):
        if not self.real:
            raise ValueError('no batches were added')
        real = torch.cat(self.real).cpu().numpy().astype(np.float32)
        fake = torch.cat(self.fake).cpu().numpy().astype(np.float32)
        os.makedirs(self.output_dir, exist_ok=True)
        np.save(os.path.join(self.output_dir, 'real_embs.npy'), real)
        np.save(os.path.join(self.output_dir, 'fake_embs.npy'), fake)
        score = np.float32(calculate_fvd(real, fake))
        with open(os.path.join(self.output_dir, 'fvd_score.txt'), 'w') as f:
            f.write(f'{score}')
        prd_data = prd.compute_prd_from_embedding(real, fake, seed=self.seed)
        with open(os.path.join(self.output_dir, 'prd_data.pkl'), 'wb') as f:
            pickle.dump(prd_data, f)
        f_beta, f_beta_inv = prd.prd_to_max_f_beta_pair(prd_data[0], prd_data[1])
        with open(os.path.join(self.output_dir, 'prd_score.txt'), 'w') as f:
            f.write(f'{f_beta}, {f_beta_inv}')
        return score, (f_beta, f_beta_inv)
