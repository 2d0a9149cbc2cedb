"""An fp32 torch restatement of the I3D forward (pytorch_i3d's InceptionI3d with TF "SAME" padding, eval-mode BatchNorm), run on the
CPU as the oracle of tests/test_fvd_gpu.py, plus seeded synthetic weights whose BatchNorm statistics are calibrated on the oracle's own
activations (every Unit3D then has unit-scale outputs, so the tests see realistic magnitudes).  Independent of mmvid_amd's kernels:
it reads only the state_dict."""
import numpy as np
import torch
import torch.nn.functional as F

from mmvid_amd.fvd import INCEPTION, POOL_BEFORE, InceptionI3d, same_pad


def _pad_same(x, k, s, value=0.):
    pads = []
    for n, kk, ss in reversed(list(zip(x.shape[2:], k, s))):
        pads += list(same_pad(n, kk, ss))
    return F.pad(x, pads, value=value)


def unit3d(sd, name, x, k, s=(1, 1, 1), calib=None):
    """conv3d (TF SAME) + BatchNorm (eps 1e-3) + ReLU on NCTHW fp32.  calib = (generator, ): set the BN statistics from this batch."""
    y = F.conv3d(_pad_same(x, k, s), sd[name + '.conv3d.weight'].float(), stride=s)
    if calib is not None:
        g = calib
        sd[name + '.bn.running_mean'] = y.mean((0, 2, 3, 4)).detach().clone()
        sd[name + '.bn.running_var'] = y.var((0, 2, 3, 4), unbiased=False).detach().clone() + 1e-3
        c = y.shape[1]
        sd[name + '.bn.weight'] = 1 + 0.1 * torch.randn(c, generator=g)
        sd[name + '.bn.bias'] = 0.2 + 0.1 * torch.randn(c, generator=g)  # mostly positive: the ReLU keeps most channels alive
    y = F.batch_norm(y, sd[name + '.bn.running_mean'].float(), sd[name + '.bn.running_var'].float(), sd[name + '.bn.weight'].float(),
                     sd[name + '.bn.bias'].float(), False, 0., 1e-3)
    return F.relu(y)


def maxpool(x, k, s):
    return F.max_pool3d(_pad_same(x, k, s), k, s)


def forward(sd, videos, calib=None):
    """videos [B, T, 224, 224, 3] fp32 in [-1, 1] -> logits averaged over time [B, 400] (fp32, on the videos' device)."""
    x = videos.permute(0, 4, 1, 2, 3).float()
    x = unit3d(sd, 'Conv3d_1a_7x7', x, (7, 7, 7), (2, 2, 2), calib)
    x = maxpool(x, (1, 3, 3), (1, 2, 2))
    x = unit3d(sd, 'Conv3d_2b_1x1', x, (1, 1, 1), calib=calib)
    x = unit3d(sd, 'Conv3d_2c_3x3', x, (3, 3, 3), calib=calib)
    x = maxpool(x, (1, 3, 3), (1, 2, 2))
    for name, *_ in INCEPTION:
        if name in POOL_BEFORE:
            x = maxpool(x, *POOL_BEFORE[name])
        b0 = unit3d(sd, name + '.b0', x, (1, 1, 1), calib=calib)
        b1 = unit3d(sd, name + '.b1b', unit3d(sd, name + '.b1a', x, (1, 1, 1), calib=calib), (3, 3, 3), calib=calib)
        b2 = unit3d(sd, name + '.b2b', unit3d(sd, name + '.b2a', x, (1, 1, 1), calib=calib), (3, 3, 3), calib=calib)
        b3 = unit3d(sd, name + '.b3b', maxpool(x, (3, 3, 3), (1, 1, 1)), (1, 1, 1), calib=calib)
        x = torch.cat([b0, b1, b2, b3], 1)
    x = F.avg_pool3d(x, (2, 7, 7), 1)
    x = F.conv3d(x, sd['logits.conv3d.weight'].float(), sd['logits.conv3d.bias'].float())
    return x.squeeze(3).squeeze(3).mean(2)


def synth_state_dict(seed, calib_clip=None):
    """Seeded conv weights (He-normal), logits ~ N(0, 1/1024); BatchNorm statistics calibrated on calib_clip (preprocessed
    [1, T, 224, 224, 3]; default: a smooth seeded clip of 16 frames)."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.clone() for k, v in InceptionI3d().state_dict().items()}
    for k, v in sd.items():
        if k.endswith('conv3d.weight'):
            fan_in = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
    sd['logits.conv3d.weight'] = torch.randn(sd['logits.conv3d.weight'].shape, generator=g) * 1024**-0.5
    sd['logits.conv3d.bias'] = 0.1 * torch.randn(400, generator=g)
    if calib_clip is None:
        calib_clip = smooth_videos(1, 16, 224, 224, seed + 1) * 2 - 1
        calib_clip = calib_clip.permute(0, 1, 3, 4, 2).contiguous()
    with torch.no_grad():
        forward(sd, calib_clip, calib=g)
    return sd


def smooth_videos(n, t, h, w, seed):
    """[n, t, 3, h, w] in [0, 1]: low-frequency seeded content (bilinear upsampling of coarse noise) plus a little fine noise, so that
    resizes and convolutions see image-like statistics."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(n * t, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    v = F.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=False)
    v = v.view(n, t, 3, h, w)
    v = 0.85 * v + 0.15 * torch.rand(v.shape, generator=g)
    return v.clamp(0, 1)


def legacy_resize_np(v, oh, ow):
    """numpy fp32 statement of TF1 resize_bilinear (align_corners / half_pixel_centers off) on [..., h, w, c]."""
    v = v.astype(np.float32)
    h, w = v.shape[-3], v.shape[-2]

    def axis(n_in, n_out):
        src = np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))
        lo = np.floor(src).astype(np.int64)
        return lo, np.minimum(lo + 1, n_in - 1), (src - np.floor(src)).astype(np.float32)

    ylo, yhi, ly = axis(h, oh)
    xlo, xhi, lx = axis(w, ow)
    tl, tr = v[..., ylo, :, :][..., xlo, :], v[..., ylo, :, :][..., xhi, :]
    bl, br = v[..., yhi, :, :][..., xlo, :], v[..., yhi, :, :][..., xhi, :]
    lx = lx[:, None]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return top + (bot - top) * ly[:, None, None]


def reference_preprocess_np(videos01, video_length):
    """utils_eval.py:214-223 + frechet_video_distance.py:34-52 in numpy fp32: [n, t, 3, h, w] in [0, 1] -> [n, VL, 224, 224, 3]."""
    v = torch.as_tensor(videos01)
    t = v.shape[1]
    if t < video_length:
        num = int(np.ceil((video_length - 1) / (t - 1)))
        parts, fl = [v], torch.flip(v, [1])
        for i in range(1, num):
            parts.append((v if i % 2 == 0 else fl)[:, 1:])
        v = torch.cat(parts, 1)
    v = (v[:, :video_length] * 255).permute(0, 1, 3, 4, 2).numpy()
    r = legacy_resize_np(v, 224, 224)
    return np.float32(2.) * r / np.float32(255.) - np.float32(1.)
