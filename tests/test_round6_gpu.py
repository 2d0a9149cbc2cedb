"""Round 6: the token-index contract on evidence wider than one frame, the MFMA decode layer (item 2) and the
advisor's round-5 findings.  Stated flip-rate bounds come from the census of 40,960 fresh tokens per mode
(tools/flip_census.py -> profiles/r06_flip_census.log): bf16 2.1-2.4 %, 'mixed' 0.06-0.25 %, 'split' 2 tokens in 40,960, fp32 0 of
4,096 against the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import flip_report, relerr, wide_vqgan_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# mode -> (vae.strict, flip-rate bound on >= 1,024 tokens, relative L2 bound of z against the reference).  'split' may differ from the
# reference only on ties at the reference's OWN resolution: a top-2 gap of at most TIE_ULPS fp32 spacings of the distance (the reference's
# z is not bit-reproducible across hosts either: the oracle on the GPU box's CPU differs from the container's in the last bits); fp32: none.
MODES = {'bf16': (False, 0.04, 3e-2), 'mixed': ('mixed', 0.005, 3e-3), 'split': ('split', 2 / 1024, 1e-4), 'fp32': (True, 0.0, 1e-5)}
TIE_ULPS = 32  # (the one such token of the goldens: gap 6.1e-5 at a distance of ~50 = 17 spacings, 1.2e-6 of the distance)


def _vae_of(sd):
    from mmvid_amd.vae import VQGanVAE1024
    vae = VQGanVAE1024(None, 128)
    vae.load_state_dict(sd)
    vae = vae.to(DEV)
    vae.image_size = 128
    return vae


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', ['vqgan_full16', 'vqgan_full16_refinit'])
def test_wide_golden_tokens_every_mode(golden, name, mode):
    """1,024 tokens of 16 full-size frames per case (two weight seeds; the synthetic well-separated codebook and the reference's own
    near-uniform initialisation), indices from the REFERENCE (tools/make_golden.py::_vqgan_wide).  fp32: every index equal.  'split': equal
    except ties at the reference's own fp32 resolution (gap <= 32 spacings of the distance; at most 2 per 1,024).  'mixed' / bf16: flip rate under the stated bound, and every flip explained by the measured error of that token's two
    distances (conftest.flip_report).  The reference z of all 16 frames comes from the oracle (pinned to the reference's z on the 4 stored
    frames: tests/test_oracle_golden.py::test_vqgan_wide_index_goldens)."""
    from oracle import vqgan as ov
    g = golden(name)
    sd, img = wide_vqgan_case(g)
    strict, max_rate, z_tol = MODES[mode]
    vae = _vae_of(sd)
    vae.strict = strict
    with torch.no_grad():
        zr = ov.encode_z(sd, img, 128).permute(0, 2, 3, 1).contiguous()
    assert relerr(zr[:4], g['z_e'].permute(0, 2, 3, 1)) <= 1e-5  # (bit-identical in the build container; this host's conv kernels may order sums differently)
    idx = torch.cat([vae.get_codebook_indices(img[i:i + 8].to(DEV)).cpu() for i in range(0, 16, 8)])
    z = torch.cat([vae.encode_z(img[i:i + 8].to(DEV)).cpu() for i in range(0, 16, 8)])
    zrel = ((z - zr).norm() / zr.norm()).item()
    n, rate, ratio = flip_report(idx, g['indices'], z, zr, sd['model.quantize.embedding.weight'], f'{name} {mode}')
    hist = np.histogram(ratio.numpy(), [0, 1, 8, 64, 512, 4096, 1e30])[0].tolist()
    print(f'{name}, {mode}: {n} of {idx.numel()} indices differ from the reference ({100 * (1 - rate):.2f} % equal); z relative L2 {zrel:.2e}; '
          f'reference top-2 gap / error: min {ratio.min().item():.2f} median {ratio.median().item():.0f}, histogram [0,1,8,64,512,4096): {hist}')
    assert idx.numel() >= 1024
    assert zrel <= z_tol
    assert rate <= max_rate, f'{n} flips'
    if mode == 'split':
        print(f'   split: flipped tokens have reference gaps of {[round(u, 1) for u in flip_report.last_gaps]} fp32 spacings of their distance')
        assert all(u <= TIE_ULPS for u in flip_report.last_gaps), flip_report.last_gaps


def test_flip_census_2048_fresh_tokens(golden):
    """A small instance of tools/flip_census.py inside the suite: 32 fresh frames (16 uniform noise + 16 smooth fields; none a golden)
    through every mode.  'split' against fp32: 0 flips; 'mixed' <= 0.5 %, bf16 <= 4 %; fp32 against the CPU oracle on 8 frames: 0."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from flip_census import frames_of
    from oracle import vqgan as ov
    g = golden('vqgan_full16')
    sd, _ = wide_vqgan_case(g)
    vae = _vae_of(sd)
    img = torch.cat([frames_of('noise', 16, 777), frames_of('smooth', 16, 778)])
    res = {}
    for mode, (strict, _, _) in MODES.items():
        vae.strict = strict
        res[mode] = (vae.get_codebook_indices(img.to(DEV)).cpu(), vae.encode_z(img.to(DEV)).cpu())
    i32, z32 = res['fp32']
    with torch.no_grad():
        pick = torch.cat([img[:4], img[16:20]])
        oi = ov.get_codebook_indices(sd, pick, 128)
    assert torch.equal(torch.cat([i32[:4], i32[16:20]]), oi), 'fp32 mode differs from the CPU oracle'
    for mode in ('bf16', 'mixed', 'split'):
        n, rate, ratio = flip_report(res[mode][0], i32, res[mode][1], z32, sd['model.quantize.embedding.weight'], mode)
        print(f'{mode}: {n} of {i32.numel()} flips against the fp32 mode; gap/err < 8 on {int((ratio < 8).sum())} tokens, median {ratio.median().item():.0f}')
        assert rate <= MODES[mode][1]
        if mode == 'split':
            assert all(u <= TIE_ULPS for u in flip_report.last_gaps), flip_report.last_gaps


def test_gemv_rows_mfma_form_vs_torch():
    """csrc/decode.hip::gemv16_mfma_kernel (3..16 bf16-exact rows on v_mfma_f32_16x16x32_bf16, K split over 8 waves): LayerNorm + weights
    streamed once + bias + QuickGELU + residual + output rounding, against torch on the same bf16-rounded operands.  Tower shapes of
    both widths (768 / 3,072 and 512 / 2,048), ragged row counts, one / two / four 16-row blocks per launch (19, 33, 64 rows) and 64 + 6 rows
    through two launches."""
    import torch.nn.functional as F
    from mmvid_amd import ops
    from test_models_gpu import close
    torch.manual_seed(1)
    for NB, K, N, act, ln, res in ((16, 768, 2304, 0, True, False), (16, 768, 3072, 1, True, False), (3, 768, 768, 0, False, True),
                                   (9, 768, 1024, 0, True, False), (12, 512, 1536, 0, True, True), (7, 512, 2048, 1, True, False),
                                   (19, 768, 768, 0, True, True), (33, 768, 2304, 0, True, False), (64, 768, 3072, 1, True, False),
                                   (70, 512, 512, 0, False, True)):
        x = torch.randn(NB, K, device=DEV)
        W = (torch.randn(N, K, device=DEV) * K ** -0.5).bfloat16()
        b = torch.randn(N, device=DEV) * 0.1
        lw, lb = 1 + 0.1 * torch.randn(K, device=DEV), 0.1 * torch.randn(K, device=DEV)
        r = torch.randn(NB, N, device=DEV) if res else None
        for rout in (False, True):
            y = ops.gemv_rows(x, W, b, ln=(lw, lb, 1e-5) if ln else None, act=act, residual=r, round_in=True, round_out=rout)
            h = F.layer_norm(x, (K, ), lw, lb, 1e-5) if ln else x
            ref = h.bfloat16().float() @ W.float().t() + b
            if act:
                ref = ref * torch.sigmoid(1.702 * ref)
            if res:
                ref = ref + r
            if rout:
                assert torch.equal(y, y.bfloat16().float()), 'round_out: the output must be bf16-exact'
                close(y, ref, 8e-3, f'gemv (MFMA form, rounded output) NB={NB} K={K} N={N}')
            else:
                close(y, ref, 2e-5, f'gemv (MFMA form) NB={NB} K={K} N={N}')


def test_artv_sampler_recovers_from_a_failed_persistent_launch(golden):
    """the recovery branch of the one-launch sampler (artv_sampling.py::token_launch_loop) -- restore the last verified token,
    sess.fall_back(first_pos + good_step), finish with launch_loop().  The failure flag (workspace word 1) is raised from a hook
    after 13 of 31 launches with the flag read every 8 tokens: tokens 0..7 stand, 8..31 are redone with the launch-per-layer step.
    Same seed, same variates: the tokens must equal a run that never used the one-launch step (MMVID_DECODE_TOKEN=0)."""
    import os
    from conftest import synth_model_sd
    from mmvid_amd.dalle_artv import DALLE
    from test_host_logic import tiny_vae
    g = golden('artv_tiny')
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2)
    m.load_state_dict(synth_model_sd(g, 19))
    m = m.to(DEV).eval()
    text, visual = g['text'].to(DEV), g['visual'].to(DEV)
    seen = {}

    def run(hook):
        m._token_step_hook, m._decode_check_every = hook, 8
        torch.manual_seed(5)
        imgs, _, _ = m.generate_images(text, visual=visual, filter_thres=0.0)
        return imgs  # (decoded from the sampled tokens: equal tokens <=> equal images)

    def fail_at_13(step, sess):
        seen['sess'] = sess
        if step == 13:
            sess.ws[1] = 1

    a_img = run(fail_at_13)
    sess = seen['sess']
    assert sess.fell_back == 1 and not sess.persistent, 'the hook must have driven the sampler into its recovery branch'
    assert sess.host_pos == int(sess.pos), 'the host mirror of the position follows the device through fall-back and replays'
    os.environ['MMVID_DECODE_TOKEN'] = '0'
    try:
        b_img = run(None)
    finally:
        del os.environ['MMVID_DECODE_TOKEN']
        m._token_step_hook = None
    assert torch.equal(a_img, b_img), 'recovered run differs from the launch-per-layer run on the same variates'


def test_artv_sampler_keeps_the_session_position_on_every_path(monkeypatch):
    """The host mirror of the decode session's position (DecodeSession.host_pos) against the device scalar after a whole sampling call
    on each path of artv_sampling.py: one launch per token (batch 2), the captured launches on a persistent session (batch 2,
    MMVID_DECODE_TOKEN=0), the captured five-launch step (batch 4) and the eager loop (batch 4, injected variates).  32 tokens = 31
    steps through the tower from position 33; the captured paths replay at least 28 of them, the other two none."""
    from mmvid_amd.dalle_artv import DALLE
    from test_host_logic import tiny_vae
    torch.manual_seed(71)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(72)
    text, vis = torch.randint(1, 49408, (4, 16), generator=gen).to(DEV), torch.randint(0, 256, (4, 16), generator=gen).to(DEV)
    steps, first_pos = m.target_seq_len, m.control_seq_len + 1
    assert steps == 32
    made, replays = [], []
    inner = m.transformer.decode_session
    monkeypatch.setattr(m.transformer, 'decode_session', lambda *a, **k: (made.append(inner(*a, **k)), made[-1])[1])
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), replay(self))[1])
    cases = [('one launch per token', 2, None, {}, False), ('captured launches, persistent session', 2, '0', {}, True),
             ('captured five-launch step', 4, None, {}, True),
             ('eager, injected variates', 4, None, dict(_race=lambda name, shape: torch.ones(shape, device=DEV)), False)]
    for what, B, token_env, kw, captured in cases:
        del made[:], replays[:]
        if token_env is not None:
            monkeypatch.setenv('MMVID_DECODE_TOKEN', token_env)
        m.generate_images(text[:B], visual=vis[:B], **kw)
        monkeypatch.delenv('MMVID_DECODE_TOKEN', raising=False)
        assert len(made) == 1, what
        sess = made[0]
        print(f'{what}: host_pos {sess.host_pos}, device {int(sess.pos)}, {len(replays)} replays, persistent {sess.persistent}, fell back {sess.fell_back}')
        assert sess.host_pos == int(sess.pos) == first_pos + steps - 1, what
        assert len(replays) >= steps - 4 if captured else not replays, what


@pytest.mark.parametrize('N,H', [(3, 6), (1, 128), (2, 2)])
def test_conv_in_kernel_vs_torch(N, H):

    """csrc/conv.hip::conv_in_kernel (the full-size encoder's first layer: 3(8) -> 128 channels on 128-pixel-wide frames; two image rows per
    block, weights in registers, stores straight from the accumulators): bf16 and fp32 outputs and the bf16-pair operator against an
    fp64 convolution of the same rounded operands; the GroupNorm partial sums (one block per image row) against sums of what it stored."""
    import ctypes
    import torch.nn.functional as F
    from mmvid_amd import ops
    from mmvid_amd.ops import _p, _stream, call
    from test_models_gpu import close
    torch.manual_seed(N * 131 + H)
    W, Cin, Cout = 128, 8, 128
    x32 = torch.randn(N, H, W, Cin, device=DEV)
    x32[..., 3:] = 0  # (the image has 3 channels; 8 are stored)
    w32 = torch.randn(Cout, 9, Cin, device=DEV) * 0.2
    bias = torch.randn(Cout, device=DEV) * 0.1

    def ref_conv(xx, ww):  # fp64, NCHW
        return F.conv2d(xx.double().permute(0, 3, 1, 2), ww.double().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1)

    x16, w16 = x32.bfloat16(), w32.bfloat16()
    ref = ref_conv(x16, w16)
    for dt, tol in ((torch.bfloat16, 8e-3), (torch.float32, 2e-6)):
        st = ops.gn_stats_buffer(N, H * W, Cout, DEV)
        st.fill_(float('nan'))
        y = ops.conv2d_nhwc(x16, w16, bias, 0, out_dtype=dt, gn_stats=st)
        close(y, ref, tol, f'conv_in {dt}')
        part = st[N * 2 * Cout:][:N * H * 32 * 2].view(N, H, 32, 2).double()
        v = y.double().view(N, H, W, 32, 4)
        close(part[..., 0], v.sum((2, 4)), 1e-5, 'GroupNorm partial sums')
        close(part[..., 1], (v * v).sum((2, 4)), 1e-5, 'GroupNorm partial sums of squares')
    # the pair operator: x = hi + lo, w = hi + lo, three products; partial sums on the fp32 values
    planes, w3 = ops.split_planes(x32), ops.split_weights(w32)
    st = ops.gn_stats_buffer(N, H * W, Cout, DEV)
    y = torch.empty(N, H, W, Cout, device=DEV)
    call('mmvid_conv2d_nhwc_split3', 0, _p(planes), N, H, W, Cin, _p(w3), _p(bias), Cout, None, 0, _p(y),
         ctypes.c_void_p(st.data_ptr() + N * Cout * 2 * 4), 1, None, _stream())
    xs, ws = planes[0].double() + planes[1].double(), w3[:, 0].double() + w3[:, 2].double()
    close(y, ref_conv(xs, ws), 2e-5, 'conv_in, pair operator')
    part = st[N * 2 * Cout:][:N * H * 32 * 2].view(N, H, 32, 2).double()
    close(part[..., 0], y.double().view(N, H, W, 32, 4).sum((2, 4)), 1e-5, 'GroupNorm partial sums (pair operator)')


@pytest.mark.parametrize('L,spec', [(33, None), (97, ('rows', [(70, 70), (71, 71)])), (579, ('rows', [(65, 65), (66, 66)]))])
def test_attention_backward_rows_with_hugely_negative_scores(L, spec):
    """ADVICE r5 (attn.hip, dQ kernel): a padded key of the sub-tile that straddles L has S = 0, i.e. P = 2^(-lse2); when EVERY score of a
    row is hugely negative (here q.k / 8 = -128 for all keys: lse2 ~ -180) that overflows, and 0 x inf put NaN into dQ wherever L is
    not a multiple of 32.  The straddling sub-tile now masks its padded keys.  All three kernels against fp32 torch."""
    from mmvid_amd import ops
    from test_models_gpu import close
    from test_round5_gpu import _attn_ref, _mask_tensor
    B, H = 1, 2
    E = H * 64
    torch.manual_seed(L)
    qkv = torch.empty(B * L, 3 * E, device=DEV)
    qkv[:, :E] = 4.0
    qkv[:, E:2 * E] = -4.0 + 0.25 * torch.randn(B * L, E, device=DEV).round()
    qkv[:, 2 * E:] = torch.randn(B * L, E, device=DEV) * 0.7
    qkv = qkv.bfloat16()
    dO = (torch.randn(B * L, E, device=DEV) * 0.2).bfloat16()
    qr = qkv.float().requires_grad_(True)
    ref = _attn_ref(qr, B, L, H, _mask_tensor(L, spec))
    ref.backward(dO.float())
    out, lse2 = ops.attention_fwd(qkv, B, L, H, spec)
    assert float(lse2.max()) < -128, 'the case must drive 2^(-lse2) out of the fp32 range'
    dqkv = ops.attention_bwd(qkv, out, dO, lse2, B, L, H, spec)
    assert torch.isfinite(dqkv.float()).all(), 'non-finite gradient (0 x inf on a padded key)'
    close(out, ref, 1e-2, f'fwd L={L}')
    for nm, sl in (('dQ', slice(0, E)), ('dK', slice(E, 2 * E)), ('dV', slice(2 * E, 3 * E))):
        close(dqkv[:, sl], qr.grad[:, sl], 5e-2, f'{nm} L={L}')  # (bf16 dS of rows whose 579 probabilities are all ~1/579)


def test_vqgan_more_frames_than_one_planned_call_holds():
    """The kernels address an operand through 32-bit byte offsets, so a planned VQGAN call holds at most 255 full-size frames (ART-V sampling
    at batch 32 decodes 512): encode / decode slice larger batches, and a frame's tokens / pixels do not depend on the slicing."""
    from mmvid_amd.vae import VQGanVAE1024
    torch.manual_seed(0)
    vae = VQGanVAE1024(None, 128).to(DEV)
    vae.image_size = 128
    with torch.no_grad():
        vae.model.quantize.embedding.weight.normal_(0, 0.5)
    assert vae._max_frames(128) == 255
    img = torch.rand(300, 3, 128, 128, device=DEV)
    idx = vae.get_codebook_indices(img)
    assert idx.shape == (300, 64)
    assert torch.equal(idx[250:260], vae.get_codebook_indices(img[250:260]))
    out = vae.decode(idx)
    assert out.shape == (300, 3, 128, 128) and torch.isfinite(out).all()
    assert torch.equal(out[250:260], vae.decode(idx[250:260]))
