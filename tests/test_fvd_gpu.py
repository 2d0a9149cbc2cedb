"""mmvid_amd.fvd on the MI355X: the kernels of csrc/i3d.hip against fp32 torch, and the whole I3D against the fp32 CPU oracle of
tests/i3d_oracle.py (synthetic seeded weights with BatchNorm statistics calibrated on the oracle's own activations).

Error model.  Every convolution rounds its two operands to bf16 (2^-9 relative each) and accumulates in fp32; its output is rounded to
bf16 again before the next layer reads it.  Against fp32 conv3d ON THE SAME bf16 OPERANDS only the summation order and the output
rounding differ: <= 1 bf16 ulp of the output + 1e-6 * sum |terms| per element (test_conv3d).  Through the 22 layers of the network the
independent per-layer roundings add up in quadrature to a few 1e-3 of a unit-scale activation; the head is fp32.  Bars for the whole
network: logits cosine >= 0.999 and relative error <= 3e-2 per clip.  Measured on the MI355X (-s prints them): conv3d worst 0.499 ulp
over every geometry; whole network cosine 0.999796 / 0.999794 and relative error 2.04e-2 at T = 15 / 16, the difference of the two clips'
logits at cosine 0.996 / 0.998; FVD of 24 + 24 clips 50.478 against the oracle's 50.235 (4.9e-3 relative)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _conv_cfg(N, T, H, W, cin, cout, k, s, pads, segs, relu=1):
    from mmvid_amd import _lib
    c = _lib.Conv3dCfg()
    c.N, c.T, c.H, c.W, c.Cin, c.Cout = N, T, H, W, cin, cout
    c.kt, c.kh, c.kw = k
    c.st, c.sh, c.sw = s
    (c.pt0, c.pt1), (c.ph0, c.ph1), (c.pw0, c.pw1) = pads
    c.relu, c.nseg = relu, len(segs)
    for i, (t, end, off, ldo) in enumerate(segs):
        c.seg_end[i], c.c_off[i], c.ldo[i], c.out[i] = end, off, ldo, t.data_ptr()
    return c


def _bf16_ulp(x):
    a = x.abs().clamp_min(2.0**-126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# every distinct (Cin, Cout, kernel, stride) of the network (stem in its folded form), plus odd ones
GEOMS = [(24, 64, (7, 7, 1), (2, 2, 1)), (64, 64, (1, 1, 1), (1, 1, 1)), (64, 192, (3, 3, 3), (1, 1, 1))]
_cin = 192
for _name, _c0, _c1, _c2, _c3, _c4, _c5 in __import__('mmvid_amd.fvd', fromlist=['INCEPTION']).INCEPTION:
    GEOMS += [(_cin, _c0 + _c1 + _c3, (1, 1, 1), (1, 1, 1)), (_c1, _c2, (3, 3, 3), (1, 1, 1)), (_c3, _c4, (3, 3, 3), (1, 1, 1)),
              (_cin, _c5, (1, 1, 1), (1, 1, 1))]
    _cin = _c0 + _c2 + _c4 + _c5
GEOMS = sorted(set(GEOMS), key=GEOMS.index) + [(8, 24, (3, 5, 2), (2, 1, 3)), (40, 136, (2, 3, 3), (2, 2, 2))]
WORST = {}


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: f'{g[0]}x{g[1]}_k{"".join(map(str, g[2]))}_s{"".join(map(str, g[3]))}')
@pytest.mark.parametrize('N,dims', [(1, (5, 9, 8)), (3, (4, 7, 11))])
def test_conv3d(geom, N, dims):
    """conv3d + bias + ReLU against fp32 F.conv3d on the bf16-rounded operands, TF-SAME pads (even and odd extents)."""
    from mmvid_amd import _lib, fvd, ops
    cin, cout, k, s = geom
    T, H, W = dims
    g = torch.Generator().manual_seed(cin * 131 + cout + N)
    x = torch.randn(N, T, H, W, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, *k, cin, generator=g) * (cin * np.prod(k))**-0.5).to(torch.bfloat16)
    b = torch.randn(cout, generator=g) * 0.3
    pads = [fvd.same_pad(n, kk, ss) for n, kk, ss in zip(dims, k, s)]
    xi = x.float().permute(0, 4, 1, 2, 3)
    wi = w.float().permute(0, 4, 1, 2, 3)
    padv = [p for pr in reversed(pads) for p in pr]
    ref = F.relu(F.conv3d(F.pad(xi, padv), wi, b, stride=s))
    terms = F.conv3d(F.pad(xi.abs(), padv), wi.abs(), b.abs(), stride=s)
    ref, terms = ref.permute(0, 2, 3, 4, 1), terms.permute(0, 2, 3, 4, 1)
    out = torch.empty(*ref.shape, device=DEV, dtype=torch.bfloat16)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    _lib.call('mmvid_conv3d_ndhwc', _conv_cfg(N, T, H, W, cin, cout, k, s, pads, [(out, cout, 0, cout)]), ops._p(xd), ops._p(wd),
              ops._p(bd), ops._stream())
    got = out.float().cpu()
    excess = ((got - ref).abs() - 1e-6 * terms) / _bf16_ulp(ref)
    WORST[geom] = max(WORST.get(geom, 0.), excess.max().item())
    print(f'conv3d {geom} N={N}: worst {excess.max().item():.3f} ulp')
    assert excess.max().item() <= 1.0
    # channel-slice store into a sentinel-filled wider tensor: the other channels stay bitwise as they were
    ldo, off = cout + 24, 16
    wide = torch.full((*ref.shape[:-1], ldo), -7.25, device=DEV, dtype=torch.bfloat16)
    _lib.call('mmvid_conv3d_ndhwc', _conv_cfg(N, T, H, W, cin, cout, k, s, pads, [(wide, cout, off, ldo)]), ops._p(xd), ops._p(wd),
              ops._p(bd), ops._stream())
    wc = wide.cpu()
    assert torch.equal(wc[..., off:off + cout], out.cpu())
    assert (wc[..., :off] == -7.25).all() and (wc[..., off + cout:] == -7.25).all()


def test_conv3d_segments():
    """One launch, three column ranges, three destinations (the b0 / b1a / b2a branches of an Inception block)."""
    from mmvid_amd import _lib, ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 5, 6, 192, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(176, 1, 1, 1, 192, generator=g) * 0.07).to(torch.bfloat16).to(DEV)
    b = torch.randn(176, generator=g).to(DEV)
    full = torch.empty(2, 3, 5, 6, 176, device=DEV, dtype=torch.bfloat16)
    _lib.call('mmvid_conv3d_ndhwc', _conv_cfg(2, 3, 5, 6, 192, 176, (1, 1, 1), (1, 1, 1), [(0, 0)] * 3, [(full, 176, 0, 176)]), ops._p(x),
              ops._p(w), ops._p(b), ops._stream())
    cat = torch.zeros(2, 3, 5, 6, 256, device=DEV, dtype=torch.bfloat16)
    t1 = torch.zeros(2, 3, 5, 6, 96, device=DEV, dtype=torch.bfloat16)
    t2 = torch.zeros(2, 3, 5, 6, 16, device=DEV, dtype=torch.bfloat16)
    segs = [(cat, 64, 0, 256), (t1, 160, 0, 96), (t2, 176, 0, 16)]
    _lib.call('mmvid_conv3d_ndhwc', _conv_cfg(2, 3, 5, 6, 192, 176, (1, 1, 1), (1, 1, 1), [(0, 0)] * 3, segs), ops._p(x), ops._p(w),
              ops._p(b), ops._stream())
    assert torch.equal(cat[..., :64], full[..., :64]) and (cat[..., 64:] == 0).all()
    assert torch.equal(t1, full[..., 64:160]) and torch.equal(t2, full[..., 160:])


@pytest.mark.parametrize('k,s,dims,C', [((1, 3, 3), (1, 2, 2), (4, 13, 12), 64), ((3, 3, 3), (1, 1, 1), (5, 7, 6), 48),
                                        ((3, 3, 3), (2, 2, 2), (5, 14, 13), 40), ((2, 2, 2), (2, 2, 2), (3, 7, 8), 16)])
def test_maxpool3d_bitwise(k, s, dims, C):
    from mmvid_amd import _lib, fvd, ops
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, *dims, C, generator=g).to(torch.bfloat16)
    pads = [fvd.same_pad(n, kk, ss) for n, kk, ss in zip(dims, k, s)]
    padv = [p for pr in reversed(pads) for p in pr]
    ref = F.max_pool3d(F.pad(x.float().permute(0, 4, 1, 2, 3), padv, value=-float('inf')), k, s).permute(0, 2, 3, 4, 1)
    ldo, off = C + 16, 8
    out = torch.full((*ref.shape[:-1], ldo), 3.5, device=DEV, dtype=torch.bfloat16)
    _lib.call('mmvid_maxpool3d_ndhwc', ops._p(x.to(DEV)), 2, *dims, C, *k, *s, *pads[0], *pads[1], *pads[2], ops._p(out), ldo, off,
              ops._stream())
    o = out.cpu()
    assert torch.equal(o[..., off:off + C].float(), ref)
    assert (o[..., :off] == 3.5).all() and (o[..., off + C:] == 3.5).all()


def _fold_np(pre):
    """[n, T, 224, 224, 3] -> the stem operand [n, T, 224, 112, 24] (channel 3 kw + c of column wo = pixel 2 wo - 2 + kw)."""
    n, T = pre.shape[:2]
    pad = np.zeros((n, T, 224, 229, 3), np.float32)
    pad[:, :, :, 2:226] = pre
    out = np.zeros((n, T, 224, 112, 24), np.float32)
    for kw in range(7):
        out[..., 3 * kw:3 * kw + 3] = pad[:, :, :, kw:kw + 224:2]
    return out


@pytest.mark.parametrize('hw', [128, 224])
@pytest.mark.parametrize('t,vl', [(8, 15), (8, 16), (15, 15), (16, 16), (20, 16)])
def test_preprocess(hw, t, vl):
    """extend_video + cut + x255 + legacy resize + 2v/255-1, against the numpy statement: within one bf16 rounding."""
    from mmvid_amd import _lib, ops
    v = O.smooth_videos(2, t, hw, hw, seed=t + hw)
    ref = torch.from_numpy(_fold_np(O.reference_preprocess_np(v, vl)))
    out = torch.empty(2, vl, 224, 112, 24, device=DEV, dtype=torch.bfloat16)
    _lib.call('mmvid_i3d_preprocess', ops._p(v.to(DEV)), 2, t, hw, hw, vl, ops._p(out), ops._stream())
    got = out.float().cpu()
    assert ((got - ref).abs() <= _bf16_ulp(ref)).all()


@pytest.fixture(scope='module')
def net():
    from mmvid_amd.fvd import load_i3d
    sd = O.synth_state_dict(seed=11)
    return sd, load_i3d(sd, device=DEV)


def _cos(a, b):
    a, b = a.double(), b.double()
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


@pytest.mark.parametrize('vl', [15, 16])
def test_network_against_oracle(net, vl):
    sd, model = net
    v = O.smooth_videos(2, 8, 96, 96, seed=vl)
    pre = torch.from_numpy(np.ascontiguousarray(O.reference_preprocess_np(v, vl)))
    with torch.no_grad():
        ref = O.forward(sd, pre)
    got = model.embed(v.to(DEV), vl).cpu()
    got2 = model(pre.to(DEV)).cpu()
    cos = _cos(got, ref)
    rel = (got - ref).norm(dim=-1) / ref.norm(dim=-1)
    dcos = _cos((got[0] - got[1])[None], (ref[0] - ref[1])[None])
    print(f'I3D T={vl}: cosine {cos.min().item():.6f}, relative error {rel.max().item():.3e}, clip-difference cosine {dcos.item():.5f}')
    assert cos.min().item() >= 0.999 and rel.max().item() <= 3e-2
    assert dcos.item() >= 0.99
    assert torch.equal(got, got2)  # the fused preprocess and fold(preprocessed) write the same stem operand


def test_batch_independence(net):
    _, model = net
    v = O.smooth_videos(5, 16, 64, 64, seed=5).to(DEV)
    allb = model.embed(v, 16)
    for i in range(5):
        assert torch.equal(model.embed(v[i:i + 1].contiguous(), 16), allb[i:i + 1])


def test_fvd_against_oracle(net):
    from mmvid_amd.fvd import calculate_fvd
    sd, model = net
    real = O.smooth_videos(24, 8, 64, 64, seed=100)
    g = torch.Generator().manual_seed(101)
    fake = (O.smooth_videos(24, 8, 64, 64, seed=102) * 0.7 + 0.3 * torch.rand(24, 8, 3, 64, 64, generator=g)).clamp(0, 1)
    er = torch.cat([model.embed(real[i:i + 8].to(DEV), 16) for i in range(0, 24, 8)]).cpu().numpy()
    ef = torch.cat([model.embed(fake[i:i + 8].to(DEV), 16) for i in range(0, 24, 8)]).cpu().numpy()
    with torch.no_grad():
        rr = O.forward(sd, torch.from_numpy(O.reference_preprocess_np(real, 16))).numpy()
        rf = O.forward(sd, torch.from_numpy(O.reference_preprocess_np(fake, 16))).numpy()
    a, b = calculate_fvd(er, ef), calculate_fvd(rr, rf)
    print(f'FVD device {a:.6g} oracle {b:.6g} ({abs(a - b) / b:.2e} relative)')
    assert b > 0 and abs(a - b) <= 0.02 * b


def test_evaluator_end_to_end(net, tmp_path):
    import pickle
    from mmvid_amd.fvd import FvdPrdEvaluator, calculate_fvd
    _, model = net
    ev = FvdPrdEvaluator(model, 15, tmp_path, seed=0)
    for i in range(2):
        real = O.smooth_videos(6, 8, 64, 64, seed=200 + i).to(DEV)
        ev.add(real, (real * 0.8 + 0.1).contiguous())
    score, (fb, fbi) = ev.finish()
    real, fake = np.load(tmp_path / 'real_embs.npy'), np.load(tmp_path / 'fake_embs.npy')
    assert real.shape == (12, 400) and fake.shape == (12, 400) and np.isfinite(real).all()
    assert open(tmp_path / 'fvd_score.txt').read() == f'{np.float32(calculate_fvd(real, fake))}' and score > 0
    with open(tmp_path / 'prd_data.pkl', 'rb') as f:
        p, r = pickle.load(f)
    assert p.shape == (1001, ) and 0 <= fb <= 1 and 0 <= fbi <= 1
    assert open(tmp_path / 'prd_score.txt').read() == f'{fb}, {fbi}'


def test_errors(net):
    from mmvid_amd import _lib
    _, model = net
    with pytest.raises(_lib.MMVIDError):
        model.embed(torch.rand(1, 16, 3, 32, 32), 16)
    with pytest.raises(_lib.MMVIDError):
        model(torch.rand(1, 16, 224, 224, 3))
    with pytest.raises(ValueError):
        model.embed(torch.rand(1, 8, 3, 32, 32, device=DEV), 8)
    with pytest.raises(ValueError):
        model(torch.rand(1, 8, 224, 224, 3, device=DEV))
    from mmvid_amd import ops
    t = torch.zeros(4096, device=DEV)
    c = _conv_cfg(1, 2, 2, 2, 12, 16, (1, 1, 1), (1, 1, 1), [(0, 0)] * 3, [(t, 16, 0, 16)])
    with pytest.raises(_lib.MMVIDError, match='multiples of 8'):
        _lib.call('mmvid_conv3d_ndhwc', c, ops._p(t), ops._p(t), ops._p(t), ops._stream())
