"""The 1,024-wide tower (ViT-L/14's visual tower: 16 heads, F = 4,096) on the device: training forward and backward against the fp32
oracle, the decode-time linear layers for K = 1,024 and K = 4,096 through mmvid_gemv_rows (csrc/decode.hip: the vector form for
1-2 rows, the matrix-pipe form for 3..64; K = 4,096 is staged in two passes), and the five-launch decode step against the full causal
forward and against the GEMM-based step it replaces at this width."""
import functools

import pytest
import torch
import torch.nn.functional as F

from guarded import SENTINEL_BITS, Guarded, bits, report_mismatch
from guarded import call_abi as _call, ptr_of as _ptr, seeded as _gen
from test_integer_exact import LIMIT, exact_f32, ints, rne_bf16
from test_models_gpu import DEV, close

pytestmark = pytest.mark.gpu
E, H = 1024, 16
BF, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------ training tower
@pytest.mark.parametrize('mask_type,idx', [('mask_prev', [17, 18]), ('causal', [])])
@pytest.mark.parametrize('L', [51, 67])
def test_tower_forward_backward_width_1024(L, mask_type, idx):
    """mmvid_tower_forward / mmvid_tower_backward at E = 1024, H = 16, F = 4096, two layers, B = 2; L = 51 and 67 (a ragged tile); BERT's
    two restricted rows and the causal mask.  Output, dL/dx and EVERY parameter gradient against oracle.tower.tower in fp32 on the same
    weights, at the bars of the width-512 test (tests/test_round3_gpu.py: 2e-2 for y, 3e-2 for gradients; max error over max value)."""
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    from oracle import tower as ot
    torch.manual_seed(5)
    tw = OpenAICLIPTransformer(L, 'openai_clip_visual', causal=True, mask_type=mask_type, mask_kwargs={'index': idx}, layers=2, width=E,
                               heads=H).to(DEV)
    with torch.no_grad():
        for p in tw.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.03)
            else:
                p.add_(torch.randn_like(p) * 0.05)  # (biases are zero and gains one after the initialisation)
    x = torch.randn(2, L, E, device=DEV, requires_grad=True)
    gy = torch.randn(2, L, E, device=DEV)
    y = tw(x)
    y.backward(gy)
    sd = {k: v.detach().float().cpu().requires_grad_(True) for k, v in tw.state_dict().items()}
    xc = x.detach().cpu().requires_grad_(True)
    yr = ot.tower(sd, xc, tw.dense_attention_mask(L), 'transformer.', heads=H)
    yr.backward(gy.cpu())
    close(y, yr, 2e-2, 'width-1024 tower y')
    close(x.grad, xc.grad, 3e-2, 'width-1024 tower dx')
    grads = dict(tw.named_parameters())
    assert set(grads) == set(sd)
    for k, p in grads.items():
        close(p.grad, sd[k].grad, 3e-2, 'width-1024 tower d ' + k)
    with torch.no_grad():
        close(tw(x.detach()), y, 1e-6, 'inference == training forward')


# ---------------------------------------------------------------------------------------- decode-time linear layers, K = 1024 / 4096
PAIRS = [(1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024)]  # in_proj, out_proj, c_fc, c_proj of the 1,024-wide tower
ROWS = [1, 2, 3, 8, 16, 17, 33, 64]


@functools.lru_cache(maxsize=2)
def int_data(K, N):
    """Integer-valued bf16-exact operands for 64 rows (a case takes the first NB): every sum of |terms| stays below 2^24, so the fp32
    result is the fp64 one whatever the order of summation (tests/test_integer_exact.py)."""
    g = _gen('wide gemv', K, N)
    x, W = ints(g, (64, K), 3), ints(g, (N, K), 3)
    bias, res = ints(g, (N,), 50, F32), ints(g, (64, N), 100, F32)
    want = x @ W.t() + bias.double() + res.double()
    mag = x.abs() @ W.abs().t() + bias.double().abs() + res.double().abs()
    assert 0 < float(mag.max()) < LIMIT
    return dict(x=x.float(), W=W.to(BF), bias=bias, res=res, want=want)


@pytest.mark.parametrize('NB', ROWS)
@pytest.mark.parametrize('K,N', PAIRS)
def test_gemv_rows_integer_exact_at_width_1024(K, N, NB):
    """No LayerNorm, no activation: the product must EQUAL the fp64 one, with bias and residual and without, fp32 and bf16-rounded
    output; operands in guarded, poisoned buffers with padded leading dimensions (a staging loop that runs past K or NB reads NaN or
    stores outside the window).  NB <= 2 also without round_in: the vector form's fp32 staging."""
    d = int_data(K, N)
    for round_in, round_out, with_epilogue in [(1, 0, True), (1, 1, False)] + ([(0, 0, True)] if NB <= 2 else []):
        x, W = Guarded(d['x'][:NB], ld=K + 8), Guarded(d['W'])
        bias, res = (Guarded(d['bias']), Guarded(d['res'][:NB], ld=N + 12)) if with_epilogue else (None, None)
        out = Guarded(role='out', shape=(NB, N), dtype=F32, ld=N + 20)
        _call('mmvid_gemv_rows', x.ptr, x.ld, NB, K, None, None, 1e-5, W.ptr, _ptr(bias), N, 0, _ptr(res), N + 12, round_in, round_out,
              out.ptr, out.ld)
        for gd in (x, W, bias, res):
            if gd is not None:
                gd.check('gemv input')
        want = d['want'][:NB] if with_epilogue else d['want'][:NB] - d['bias'].double() - d['res'][:NB].double()
        want = rne_bf16(want).float() if round_out else exact_f32(want)
        report_mismatch(out.check('gemv out'), want, f'gemv_rows NB={NB} K={K} N={N} round_in={round_in} round_out={round_out} epilogue={with_epilogue}')


# (K, N, LayerNorm, QuickGELU, residual): what the tower's four layers fuse, and LayerNorm in front of K = 4,096, which exists in the
# vector form only (no layer of the tower has it): up to 8 rows
FUSED = [(1024, 3072, True, 0, False), (1024, 1024, False, 0, True), (1024, 1024, True, 0, True), (1024, 4096, True, 1, False),
         (4096, 1024, False, 0, True), (4096, 1024, False, 1, False), (4096, 1024, True, 0, True)]
FUSED_CASES = [c + (NB,) for c in FUSED for NB in ROWS if not (c[0] == 4096 and c[2] and NB > 8)]


TIE_MARGIN = 2.0 ** -20  # relative; eight fp32 spacings: more than two fp32 evaluations of a 1,024- or 4,096-term LayerNorm differ by


def near_bf16_tie(h):
    """Where an fp64 LayerNorm value lies within TIE_MARGIN of the middle between two neighbouring bf16 values."""
    ulp = 2.0 ** (torch.floor(torch.log2(h.abs().clamp_min(1e-30))) - 7)
    middle = torch.floor(h / ulp) * ulp + ulp / 2
    return (h - middle).abs() <= h.abs() * TIE_MARGIN


def rows_without_ties(NB, K, lw, lb, g):
    """NB random rows whose LayerNorm output holds no bf16 rounding tie.  The bars of this test compare fp32 sums over THE SAME
    bf16-rounded rows; the kernel and torch both evaluate the LayerNorm in fp32, in different orders, so an element within a few fp32
    spacings of the middle between two bf16 values would be rounded up by one and down by the other (about one row in three holds
    such an element at K = 1,024, and it moves an output by ten times the bar).  Such rows are drawn again, the way the integer-exact
    cases build operands that meet their own condition; the condition is asserted in fp64, without the kernel."""
    x = torch.randn(NB, K, generator=g)
    for _ in range(64):
        bad = near_bf16_tie(F.layer_norm(x.double(), (K,), lw.double(), lb.double(), 1e-5)).any(1)
        if not bool(bad.any()):
            return x
        x[bad] = torch.randn(int(bad.sum()), K, generator=g)
    raise AssertionError('no tie-free rows after 64 draws')


@pytest.mark.parametrize('K,N,ln,act,res,NB', FUSED_CASES)
def test_gemv_rows_with_layernorm_gelu_residual_at_width_1024(K, N, ln, act, res, NB):
    """LayerNorm, QuickGELU and the residual on random operands, against fp32 torch on the same bf16-rounded rows, at the bars of
    tests/test_round6_gpu.py::test_gemv_rows_mfma_form_vs_torch (2e-5; 8e-3 where the output is rounded to bf16).  With LayerNorm the
    rows are drawn so that no normalised value sits on a bf16 rounding tie (rows_without_ties)."""
    g = torch.Generator().manual_seed(1000 * K + N + NB)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, generator=g) * 0.1
    lw, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    r = torch.randn(NB, N, generator=g) if res else None
    x = rows_without_ties(NB, K, lw, lb, g) if ln else torch.randn(NB, K, generator=g)
    if ln:
        assert not bool(near_bf16_tie(F.layer_norm(x.double(), (K,), lw.double(), lb.double(), 1e-5)).any())
    h = F.layer_norm(x.to(DEV), (K,), lw.to(DEV), lb.to(DEV), 1e-5) if ln else x.to(DEV)
    ref = h.bfloat16().float() @ W.to(DEV).float().t() + b.to(DEV)
    if act:
        ref = ref * torch.sigmoid(1.702 * ref)
    if res:
        ref = ref + r.to(DEV)
    for rout in (0, 1):
        xg, Wg, bg = Guarded(x, ld=K + 8), Guarded(W), Guarded(b)
        lwg, lbg = (Guarded(lw), Guarded(lb)) if ln else (None, None)
        rg = Guarded(r, ld=N + 12) if res else None
        out = Guarded(role='out', shape=(NB, N), dtype=F32, ld=N + 20)
        _call('mmvid_gemv_rows', xg.ptr, xg.ld, NB, K, _ptr(lwg), _ptr(lbg), 1e-5, Wg.ptr, bg.ptr, N, act, _ptr(rg), N + 12, 1, rout, out.ptr, out.ld)
        for gd in (xg, Wg, bg, lwg, lbg, rg):
            if gd is not None:
                gd.check('gemv input')
        y = out.check('gemv out')
        if rout:
            assert torch.equal(y, y.bfloat16().float()), 'round_out: the output must be bf16-exact'
        close(y, ref, 8e-3 if rout else 2e-5, f'gemv NB={NB} K={K} N={N} ln={ln} act={act} res={res} round_out={rout}')


# ------------------------------------------------------------------------------------------------------------------------ decode step
CACHED_VS_FULL = 1e-2      # tests/test_round3_gpu.py::test_decode_step_on_a_long_cache
FUSED_VS_GEMM_STEP = 1e-2  # tests/test_models_gpu.py::test_artv_kv_cache_decode_matches_full_recompute


@functools.lru_cache(maxsize=1)
def wide_tower():
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    torch.manual_seed(7)
    return OpenAICLIPTransformer(seq_len=600, which_model='openai_clip_visual', causal=True, layers=2, width=E, heads=H).to(DEV).eval()


@pytest.mark.parametrize('B', [1, 2, 3, 16, 17, 64])
@pytest.mark.parametrize('Lmax,P', [(130, 127), (600, 515)])  # (the last three positions of a short cache; beyond 512 keys of a long one: both attention instances)
def test_decode_step_width_1024(Lmax, P, B):
    """Three consecutive positions from a prefilled cache through the decode session (mmvid_tower_decode_fused_slice: the vector form
    at B <= 2, the matrix-pipe form from 3 on; the second step is captured, the third replayed): the hidden state against the full causal
    forward and against mmvid_tower_decode on a cache of its own; the step stores row p of every layer and sequence and nothing else."""
    from mmvid_amd import _lib
    import ctypes
    tw = wide_tower()
    torch.manual_seed(B)
    steps = 3
    x = torch.randn(B, P + steps, E, device=DEV) * 0.5
    with torch.no_grad():
        full = tw(x)
        cache, cache_ref = tw.new_kv_cache(B, Lmax, DEV), tw.new_kv_cache(B, Lmax, DEV)
        for c in (cache, cache_ref):
            c.view(torch.int16).fill_(SENTINEL_BITS[BF])
            tw.prefill(x[:, :P].contiguous(), c)
        assert bool((bits(cache[:, :, P:]) == SENTINEL_BITS[BF]).all()), 'the prefill stores the prompt rows only'
        sess = tw.decode_session(cache, P)
        assert not sess.persistent and _lib.load().mmvid_tower_decode_persistent_supported(ctypes.byref(sess.cfg), Lmax) == 0
        for k in range(steps):
            p = P + k
            before = cache.clone()
            h = sess.step(x[:, p].contiguous()).clone()
            href = tw.decode_step(x[:, p].contiguous(), cache_ref, p)
            close(h, full[:, p], CACHED_VS_FULL, f'B={B} Lmax={Lmax}: decode step vs full forward at position {p}')
            close(h, href, FUSED_VS_GEMM_STEP, f'B={B} Lmax={Lmax}: decode step vs the GEMM-based step at position {p}')
            changed = bits(cache) != bits(before)
            assert not bool(changed[:, :, :p].any()) and not bool(changed[:, :, p + 1:].any()), 'a row other than p was stored'
            assert not bool((bits(cache[:, :, p]) == SENTINEL_BITS[BF]).any()), 'row p was not stored completely'
            close(cache[:, :, p], cache_ref[:, :, p], FUSED_VS_GEMM_STEP, f'B={B} Lmax={Lmax}: key/value row {p}')
        assert sess.graph is not None and sess.host_pos == P + steps and int(sess.pos) == P + steps
