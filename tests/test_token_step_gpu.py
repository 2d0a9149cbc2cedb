"""Training from cached tokens on the GPU: the uint8 input kernels, the resident token table, BERT.forward / DALLE.forward on token
targets with a real VID negative, the graphed token step, and the cache builder.  Every equivalence is against this package's own
pixel path.

Host references are computed where the data path computes them: `u8.float() / 255` on the CPU is a correctly rounded division
(ToTensor, data._load_frame); the same expression on a device tensor multiplies by a rounded 1/255 and differs in the last bit for
some byte values, so it is never used as a reference here."""
import copy
import math

import numpy as np
import pytest
import torch

from test_host_logic import tiny_vae
from test_models_gpu import DEV, close
from test_token_cache_host import negative_tokens, pack_warp_params, parse_warp_params, write_frame_folder

pytestmark = pytest.mark.gpu

INT_STAGES = ('mask1', 'target', 'target_warp', 'ids', 'sel', 'tfull', 'cnt')


def unit_frames(u8):
    """uint8 [..., H, W, 3] (host) -> fp32 [..., 3, H, W] = u8 / 255, divided on the host, on the device."""
    d = u8.dim()
    return (u8.cpu().permute(*range(d - 3), d - 1, d - 3, d - 2).float() / 255).contiguous().to(DEV)


def small_bert(T, num_visuals=0):
    from mmvid_amd.dalle_bert import BERT
    torch.manual_seed(0)
    m = BERT(dim=768, vae=tiny_vae(), cvae=tiny_vae() if num_visuals else None, num_text_tokens=49408, text_seq_len=16,
             which_transformer='openai_clip_visual', num_visuals=num_visuals, num_targets=T, transformer_layers=2).to(DEV).train()
    with torch.no_grad():
        for v in (m.vae, m.cvae):
            if v is not None:
                v.model.quantize.embedding.weight.normal_(0, 0.5)
    return m


def batch(B, T, size=64, seed=3):
    gen = torch.Generator().manual_seed(seed)
    text = torch.randint(1, 49408, (B, 16), generator=gen)
    text[0, 10:] = 0
    u8 = torch.randint(0, 256, (B, T, size, size, 3), generator=gen, dtype=torch.uint8)
    return text.to(DEV), u8


def run_forward(m, seed, text, **kw):
    """One forward at front-end (seed, step 0) -> (the three losses, the stage tensors)."""
    m.frontend.seed, m.frontend.step = seed, None
    m._debug_keep = {}
    with torch.no_grad():
        losses = torch.stack([torch.as_tensor(x).detach().float().reshape(()).cpu() for x in m(text, return_loss=True, **kw)])
    keep, m._debug_keep = m._debug_keep, None
    return losses, keep


# ------------------------------------------------------------------------------------------------- 1-3: kernels
def test_frames_u8_to_f32_is_the_host_division():
    from mmvid_amd import ops
    pix = torch.arange(256).view(16, 16)
    u8 = torch.stack([torch.stack([(pix * (2 * c + 1) + 37 * n + 91 * c) % 256 for c in range(3)], -1) for n in range(3)]).to(torch.uint8)
    for c in range(3):
        assert all(len(set(u8[n, :, :, c].reshape(-1).tolist())) == 256 for n in range(3))  # all 256 byte values in every channel
    ref = u8.permute(0, 3, 1, 2).float() / 255
    assert np.array_equal(ref.numpy(), np.transpose(u8.numpy(), (0, 3, 1, 2)).astype(np.float32) / np.float32(255))
    got = ops.frames_u8_to_f32(u8.to(DEV))
    assert got.shape == (3, 3, 16, 16) and torch.equal(got.cpu(), ref)
    odd = torch.randint(0, 256, (2, 5, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))  # (H*W % 4 != 0)
    assert torch.equal(ops.frames_u8_to_f32(odd.to(DEV)).cpu(), odd.permute(0, 3, 1, 2).float() / 255)
    big = torch.randint(0, 256, (5, 128, 128, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.frames_u8_to_f32(big.to(DEV)).cpu(), big.permute(0, 3, 1, 2).float() / 255)


def test_vid_warp_new_frames_u8_injected_parameters():
    """Every strategy, the affine one also with a sampling grid that leaves the frame (reflection): bit-equal to the fp32 kernel."""
    from mmvid_amd.frontend import Frontend
    B, T, S = 6, 4, 32
    _, u8 = batch(B, T, S)
    x = unit_frames(u8)
    ang = 0.4
    rot = np.array([math.cos(ang), -math.sin(ang), 0.05, math.sin(ang), math.cos(ang), -0.08], np.float32)
    far = np.array([1.5 * math.cos(ang), -1.5 * math.sin(ang), 0.8, 1.5 * math.sin(ang), 1.5 * math.cos(ang), -0.9], np.float32)
    xn = (2 * np.arange(S) + 1) / S - 1
    gx = far[0] * xn[None, :] + far[1] * xn[:, None] + far[2]
    assert (np.abs(gx) > 1).any() and (np.abs(rot[0] * xn[None, :] + rot[1] * xn[:, None] + rot[2]) > 1).any()
    params = [dict(mode=0, j1=1, src_b=3, src_t=2), dict(mode=1, j1=2, perm=[3, 0, 1, 2] + list(range(4, 32))),
              dict(mode=2, j1=0, shift=0.31, chan=0), dict(mode=2, j1=3, shift=-0.22, chan=2), dict(mode=3, j1=1, theta=rot),
              dict(mode=3, j1=2, theta=far)]
    raw = torch.from_numpy(pack_warp_params(params)).to(DEV)
    fe = Frontend(seed=1)
    a = fe.vid_warp_new_frames(x, [0.25] * 4, torch.empty(B, 3, S, S, device=DEV), params=raw)
    b = fe.vid_warp_new_frames_u8(u8.to(DEV), [0.25] * 4, torch.empty(B, 3, S, S, device=DEV), params=raw)
    for i, p in enumerate(params):
        assert torch.equal(a[i], b[i]), f'sample {i} (mode {p["mode"]}): {(a[i] != b[i]).sum().item()} pixels differ'
        changed = not torch.equal(a[i], x[i, p['j1']])
        assert changed == (p['mode'] >= 2), f'sample {i}: mode {p["mode"]} changed={changed}'


def test_vid_warp_new_frames_u8_drawn_parameters():
    """Equal seed and step: byte-equal parameter records (also from the draw-only entry point) and bit-equal new frames."""
    from mmvid_amd.frontend import Frontend
    B, T, S = 16, 8, 32
    _, u8 = batch(B, T, S)
    x, u8d = unit_frames(u8), u8.to(DEV)
    fa, fb, fc = Frontend(seed=5), Frontend(seed=5), Frontend(seed=5)
    seen = set()
    for rep in range(4):
        a = fa.vid_warp_new_frames(x, [0.25] * 4, torch.empty(B, 3, S, S, device=DEV))
        b = fb.vid_warp_new_frames_u8(u8d, [0.25] * 4, torch.empty(B, 3, S, S, device=DEV))
        fc.vid_warp_draw(B, T, DEV, [0.25] * 4)
        assert torch.equal(fa._warp_scratch[:B * 176], fb._warp_scratch[:B * 176])
        assert torch.equal(fa._warp_scratch[:B * 176], fc._warp_scratch[:B * 176])
        assert torch.equal(a, b), f'draw {rep}: {(a != b).sum().item()} pixels differ'
        seen |= {p['mode'] for p in parse_warp_params(fa._warp_scratch.cpu().numpy(), B)}
        for f in (fa, fb, fc):
            f.advance(DEV)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize('n', [16, 64, 6])
def test_token_rows_gather(n):
    from mmvid_amd import _lib, ops
    rng = np.random.RandomState(n)
    table = rng.randint(0, 65536, (50, n)).astype(np.uint16)
    idx = rng.randint(0, 50, (3, 4)).astype(np.int64)
    idx[0, 0], idx[2, 3] = 0, 49
    dev = torch.from_numpy(table).to(DEV)
    _lib.device_faults(reset=True)
    got = ops.token_rows_gather(dev, torch.from_numpy(idx).to(DEV))
    assert got.dtype == torch.int64 and got.shape == (3, 4 * n)
    assert np.array_equal(got.cpu().numpy(), table[idx].astype(np.int64).reshape(3, -1))
    assert _lib.device_faults(reset=True) == [0, 0, 0, 0]
    bad = idx.copy()
    bad[1, 2] = 50  # one past the table: reads row 0, is counted, and the check raises
    got = ops.token_rows_gather(dev, torch.from_numpy(bad).to(DEV)).cpu().numpy().reshape(3, 4, n)
    want = table[idx].astype(np.int64)
    want[1, 2] = table[0]
    assert np.array_equal(got, want)
    assert _lib.device_faults(reset=False)[2] == 1
    with pytest.raises(_lib.MMVIDError, match='token-table row'):
        _lib.check_device_faults()
    assert _lib.device_faults() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- 4-6: BERT.forward on token targets
@pytest.mark.parametrize('rel,num_visuals,fp32_frames', [(True, 0, False), (False, 0, False), (True, 1, False), (True, 0, True)])
def test_token_forward_equals_pixel_forward(rel, num_visuals, fp32_frames):
    """forward(target=frames) against forward(target=tokens of those frames, target_frames=...) at equal front-end seed and step.
    Exactly equal: every integer stage tensor, the assembled sequence and the tower output (the same kernels saw the same inputs).
    The losses: loss_rel and loss_vid are bit-equal; loss_msm is NOT bit-reproducible on the pixel path itself (its mean over the
    selected rows accumulates in an order that varies from launch to launch), so the bound is twice the pixel path's self-difference,
    measured here: the largest difference between any two of four pixel runs, over the three seeds of the case.  Measured on an
    MI355X: self-difference of loss_msm 0 to 1.4e-6 per pair of runs (0 for loss_rel and loss_vid), token path against pixel
    path 0 to 1.4e-6.  (Two runs alone measure 0.0 in a third of the pairs and then demand a bit equality the pixel path does not
    have with itself; four runs of three seeds estimate the same quantity with fewer accidents.)"""
    B, T = 4, 4
    m = small_bert(T, num_visuals)
    text, u8 = batch(B, T)
    frames = unit_frames(u8)
    kw = dict(rel=rel, vid=True, rel_no_fully_masked=True)
    if num_visuals:
        kw['visual'] = torch.rand(B, 1, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    tokens = m.vae.get_codebook_indices(frames.view(B * T, 3, 64, 64)).view(B, -1).contiguous()
    self_diff, diffs = torch.zeros(3), []
    for seed in (21, 22, 23):
        pix = [run_forward(m, seed, text, target=frames, **kw) for _ in range(4)]
        spread = torch.stack([(a[0] - b[0]).abs() for i, a in enumerate(pix) for b in pix[:i]]).max(0).values
        self_diff = torch.maximum(self_diff, spread)
        l1, k1 = pix[0]
        lt, kt = run_forward(m, seed, text, target=tokens, target_frames=frames if fp32_frames else u8.to(DEV), **kw)
        print(f'seed {seed}: pixel losses {l1.tolist()} self-difference {spread.tolist()} token-path difference {(lt - l1).abs().tolist()}')
        assert torch.isfinite(l1).all()
        for name in INT_STAGES + ('x_seq', 'y'):
            if all(torch.equal(k1[name], k[name]) for _, k in pix[1:]):  # (every integer stage is; x_seq and y were, too)
                assert torch.equal(k1[name], kt[name]), f'seed {seed}: stage {name} differs in {(k1[name] != kt[name]).sum().item()} places'
            else:
                assert name not in INT_STAGES, f'seed {seed}: the pixel path does not reproduce its own {name}'
                print(f'seed {seed}: the pixel path does not reproduce its own {name} bit for bit: not compared')
        assert not torch.equal(kt['target_warp'], kt['target'])
        diffs.append((seed, (lt - l1).abs(), lt, l1))
    print(f'self-difference of the pixel path over the case: {self_diff.tolist()}')
    for seed, d, lt, l1 in diffs:
        assert (d <= 2 * self_diff).all(), f'seed {seed}: losses {lt.tolist()} vs {l1.tolist()} (self-difference {self_diff.tolist()})'


def test_token_targets_get_a_real_vid_negative():
    """Token targets with vid=True and target_frames: the negative differs from the positive in every sample (before this entry
    point existed it WAS the positive: loss_vid trained on identical pairs) and is what the drawn WarpParams say.
    The seeds are those whose draws (known beforehand: the generator is counter-based) hold no near-identity warp -- every colour
    shift at least 0.4, every rotation at least 10 degrees.  A warp can be too weak to move a token: at seed 31 sample 0 draws a
    shift of -0.044 on one channel, the 16 tokens of that 64 x 64 frame stay (seen on an MI355X) and the negative equals the positive;
    the pixel path assembles the same tokens (test_token_forward_equals_pixel_forward).  That is warp() itself, not the token path."""
    from mmvid_amd.frontend import Frontend
    B, T = 6, 8
    m = small_bert(T)
    text, u8 = batch(B, T)  # (noise frames: eight mutually distinct frames per sample)
    frames = unit_frames(u8)
    tokens = m.vae.get_codebook_indices(frames.view(B * T, 3, 64, 64)).view(B, -1).contiguous()
    per_frame = tokens.view(B, T, -1)
    assert all(not torch.equal(per_frame[b, i], per_frame[b, j]) for b in range(B) for i in range(T) for j in range(i))
    modes = set()
    for seed in (32, 36, 55):
        _, k = run_forward(m, seed, text, target=tokens, target_frames=u8.to(DEV), rel=True, vid=True)
        assert torch.equal(k['target'], tokens)
        differs = (k['target_warp'] != k['target']).any(1)
        raw = m.frontend._warp_scratch[:B * 176].clone()
        params = parse_warp_params(raw.cpu().numpy(), B)
        print(f'seed {seed}:', [(p['mode'], p['j1'], round(p['shift'], 3)) for p in params], 'differs', differs.tolist())
        assert differs.all(), f'seed {seed}: the negative equals the positive in samples {(~differs).nonzero().view(-1).tolist()}'
        new = Frontend(seed=0).vid_warp_new_frames_u8(u8.to(DEV), [0.25] * 4, torch.empty(B, 3, 64, 64, device=DEV), params=raw)
        want = negative_tokens(tokens.cpu().numpy(), m.vae.get_codebook_indices(new).cpu().numpy(), params, T)
        assert np.array_equal(k['target_warp'].cpu().numpy(), want)
        modes |= {p['mode'] for p in params}
    assert modes == {0, 1, 2, 3}


def test_token_targets_without_frames():
    """Strategies 0 and 1 move whole frames: no pixels needed, the same negative as the pixel path.  Any probability on the two
    pixel strategies without target_frames is an error that names the argument."""
    B, T = 4, 4
    m = small_bert(T)
    text, u8 = batch(B, T)
    frames = unit_frames(u8)
    tokens = m.vae.get_codebook_indices(frames.view(B * T, 3, 64, 64)).view(B, -1).contiguous()
    prob = [0.5, 0.5, 0, 0]
    for seed in (41, 42, 43):
        lp, kp = run_forward(m, seed, text, target=frames, rel=True, vid=True, vid_strategy_prob=prob)
        lt, kt = run_forward(m, seed, text, target=tokens, rel=True, vid=True, vid_strategy_prob=prob)
        for name in INT_STAGES:
            assert torch.equal(kp[name], kt[name]), name
        assert not torch.equal(kt['target_warp'], kt['target'])
    with pytest.raises(ValueError, match='target_frames') as e:
        run_forward(m, 41, text, target=tokens, rel=True, vid=True, vid_strategy_prob=[0.25] * 4)
    assert 'colour-shift' in str(e.value) and 'affine' in str(e.value)
    # untouched: vid=False needs nothing, and an injected negative is taken as given
    run_forward(m, 41, text, target=tokens, rel=True, vid=False)
    _, k = run_forward(m, 41, text, target=tokens, rel=True, vid=True, _target_warp=tokens.flip(0))
    assert torch.equal(k['target_warp'], tokens.flip(0))


# ------------------------------------------------------------------------------------------------- 7: the graphed token step
def test_graphed_token_step_matches_graphed_pixel_step():
    """Config 2 at full size (12 layers, L = 579, per-GPU batch 6): the token step (48 cached frames' tokens + the uint8 frames; six
    frames through the encoder inside the graph) captures and replays, and from equal initial state, seed and data it follows the
    pixel step -- loss, sampled gradients and sampled parameters after the eager warm-up step and after each replayed one, within
    the tolerances of test_parity_gpu.py::test_config2_full_size_graphed_step_matches_eager."""
    from mmvid_amd.engine import FlatTrainer, GraphedStep, backward_order
    from test_parity_gpu import _full_bert
    base = _full_bert(0)
    B, T = 6, 8
    gen = torch.Generator().manual_seed(1)
    text = torch.randint(1, 49408, (B, 64), generator=gen)
    text[0, 40:] = 0
    u8s = [torch.randint(0, 256, (B, T, 128, 128, 3), generator=gen, dtype=torch.uint8) for _ in range(2)]
    with torch.no_grad():  # (on a copy: a VQGAN that has run holds its plan, and a plan cannot be deep-copied)
        toks = [copy.deepcopy(base).vae.get_codebook_indices(unit_frames(u).view(B * T, 3, 128, 128)).view(B, -1).contiguous() for u in u8s]

    def run(token_path):
        m = copy.deepcopy(base)
        m.frontend.seed, m.frontend.step = 77, None
        tr = FlatTrainer(m, lr=1e-4, max_grad_norm=1.0, order=backward_order)
        kw = dict(return_loss=True, rel=True, vid=True, rel_no_fully_masked=True)
        if token_path:
            def fn(text, target, target_frames):
                lm, lr, lv = m(text, target=target, target_frames=target_frames, **kw)
                return 7.0 * lm + 0.5 * lr + 0.5 * lv
            inp = lambda i: dict(text=text.to(DEV), target=toks[i], target_frames=u8s[i].to(DEV))
        else:
            def fn(text, frames):
                lm, lr, lv = m(text, target=frames, **kw)
                return 7.0 * lm + 0.5 * lr + 0.5 * lv
            inp = lambda i: dict(text=text.to(DEV), frames=unit_frames(u8s[i]))
        step = GraphedStep(tr, fn, inp(0), warmup=1)
        assert step.graph is not None, step.capture_error
        trace = [(None, tr.P[::997].clone(), tr.G[::997].clone())]  # after the one eager optimiser step of the warm-up
        for i in (1, 0):
            loss = step(**inp(i)).item()
            trace.append((loss, tr.P[::997].clone(), tr.G[::997].clone()))
        return trace

    pix, tok = run(False), run(True)
    for i, ((lp, pp, gp), (lt, pt, gt)) in enumerate(zip(pix, tok)):
        if lp is not None:
            print(f'step {i}: pixel loss {lp} token loss {lt}')
            assert math.isfinite(lp) and abs(lp - lt) <= 2e-3 * max(1.0, abs(lp))
        close(gt, gp, 2e-2, f'sampled gradients after step {i}: token step vs pixel step')
        close(pt, pp, 1e-3, f'sampled parameters after step {i}: token step vs pixel step')


# ------------------------------------------------------------------------------------------------- 8: ART-V
def test_artv_trains_from_tokens():
    """DALLE.forward(target=tokens, return_loss=True): ART-V has no VID warp, so cached tokens need nothing new there.  Loss and a
    gradient slice equal the pixel-target call on the frames the tokens came from, within twice the pixel call's own run-to-run
    difference, measured here as the largest difference between any two of four pixel runs (on an MI355X: 0 to 4.8e-7 on the loss,
    whose mean accumulates in a varying order; the token-target call then differs from a pixel call by as much)."""
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(0)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).train()
    with torch.no_grad():
        m.vae.model.quantize.embedding.weight.normal_(0, 0.5)
    B, T = 2, 2
    text, u8 = batch(B, T)
    frames = unit_frames(u8)
    visual = torch.rand(B, 1, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    tokens = m.vae.get_codebook_indices(frames.view(B * T, 3, 64, 64)).view(B, -1).contiguous()

    def run(target):
        m.zero_grad(set_to_none=True)
        loss = m(text, visual=visual, target=target, return_loss=True)[0]
        loss.backward()
        return loss.detach().cpu(), m.to_logits[1].weight.grad[:64, :64].detach().cpu().clone(), m.image_emb.weight.grad[:64, :64].detach().cpu().clone()

    pix, t = [run(frames) for _ in range(4)], run(tokens)
    assert torch.isfinite(pix[0][0]) and pix[0][1].abs().max() > 0 and pix[0][2].abs().max() > 0
    for i, name in enumerate(('loss', 'to_logits grad', 'image_emb grad')):
        self_diff = max((a[i] - b[i]).abs().max().item() for k, a in enumerate(pix) for b in pix[:k])
        diff = (pix[0][i] - t[i]).abs().max().item()
        print(f'{name}: pixel self-difference {self_diff:.3e}, token-target difference {diff:.3e}')
        assert diff <= 2 * self_diff, f'{name}: {diff} > 2 x {self_diff}'


# ------------------------------------------------------------------------------------------------- 9: the builder
@pytest.mark.parametrize('mode', [False, 'mixed', 'split', True])
def test_build_token_cache(tmp_path, mode):
    from mmvid_amd import data, token_cache
    root = str(tmp_path / 'set')
    write_frame_folder(root, (9, 12), size=80)
    torch.manual_seed(0)
    vae = tiny_vae().to(DEV)
    with torch.no_grad():
        vae.model.quantize.embedding.weight.normal_(0, 0.5)
    before = 'mixed' if mode != 'mixed' else 'split'
    vae.strict = before
    a = token_cache.build_token_cache(root, vae, str(tmp_path / 'c7'), mode=mode, chunk=7)
    assert vae.strict == before
    b = token_cache.build_token_cache(root, vae, str(tmp_path / 'c64'), mode=mode, chunk=64, with_frames=False)
    listing = data.TextVideoDataset(root, image_size=64, frame_num=1, frame_step=1)
    paths = [p for k in listing.keys for p in listing.videos[k]]
    stack = torch.stack([data._load_frame(p, 64) for p in paths]).to(DEV)
    vae.strict = mode
    want = vae.get_codebook_indices(stack).cpu().numpy()
    vae.strict = before
    assert a.tokens.shape == (21, 16) and a.strict == token_cache.strict_name(mode) and b.frames is None
    assert np.array_equal(np.asarray(a.tokens), np.asarray(b.tokens)), 'chunk 7 vs chunk 64'
    assert np.array_equal(np.asarray(a.tokens).astype(np.int64), want), f'{(np.asarray(a.tokens) != want).sum()} tokens differ'
    assert torch.equal(torch.from_numpy(np.asarray(a.frames)).permute(0, 3, 1, 2).float() / 255, stack.cpu())
    assert len(set(map(tuple, np.asarray(a.tokens)))) > 1
    a.check(vae)
    table = a.to_device(DEV)
    assert table.dtype == torch.uint16 and table.shape == (21, 16)
    with torch.no_grad():
        vae.model.quant_conv.bias[0] += 1e-3
    with pytest.raises(ValueError, match='fingerprint'):
        a.check(vae)
