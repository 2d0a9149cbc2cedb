"""The attention backward at three dK/dV blocks per CU: the row constants (-lse2 / scale_log2, -delta) are the initial accumulators of
the S and dP chains, so P and dS round differently from the subtract-after form -- dQ, dK and dV against fp64 torch at the training
shape for every mask mode, ragged lengths around the 32 / 64 / 128 boundaries, bitwise repeatability, and (host only) the register
budget that gives three blocks per CU."""
import os
import re
import subprocess

import pytest
import torch

from test_models_gpu import DEV, close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ('rows', [(65, 65), (66, 66)])  # BERT's "mask_prev": two query rows that may not see earlier columns


def _mask_tensor(L, spec, dtype):
    if spec is None:
        return None
    if spec == 'causal':
        return torch.full((L, L), float('-inf'), device=DEV, dtype=dtype).triu_(1)
    m = torch.zeros(L, L, device=DEV, dtype=dtype)
    for r, c in spec[1]:
        m[r, :c] = float('-inf')
    return m


def _reference(qkv, dO, B, L, H, spec, dtype):
    """softmax(QK^T / 8 + mask) V and its gradient with respect to qkv, in `dtype`, on the bf16 inputs."""
    E = H * 64
    qr = qkv.to(dtype).requires_grad_(True)
    q, k, v = [t.view(B, L, H, 64).transpose(1, 2) for t in qr.split(E, dim=1)]
    s = q @ k.transpose(-1, -2) * 0.125
    mask = _mask_tensor(L, spec, dtype)
    if mask is not None:
        s = s + mask
    out = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, E)
    out.backward(dO.to(dtype))
    return qr.grad


def _run(B, L, H, spec, seed):
    from mmvid_amd import ops
    E = H * 64
    torch.manual_seed(seed)
    qkv = (torch.randn(B * L, 3 * E, device=DEV) * 0.7).bfloat16()
    dO = (torch.randn(B * L, E, device=DEV) * 0.2).bfloat16()
    out, lse2 = ops.attention_fwd(qkv, B, L, H, spec)
    dqkv = ops.attention_bwd(qkv, out, dO, lse2, B, L, H, spec)
    torch.cuda.synchronize()
    return qkv, dO, out, lse2, dqkv


@pytest.mark.gpu
@pytest.mark.parametrize('spec', [None, 'causal', ROWS], ids=['none', 'causal', 'rows'])
def test_attention_bwd_training_shape_vs_fp64(spec):
    B, L, H = 18, 579, 12
    E = H * 64
    qkv, dO, _, _, dqkv = _run(B, L, H, spec, 7)
    assert torch.isfinite(dqkv.float()).all()
    g = _reference(qkv, dO, B, L, H, spec, torch.float64)
    for nm, sl in (('dQ', slice(0, E)), ('dK', slice(E, 2 * E)), ('dV', slice(2 * E, 3 * E))):
        close(dqkv[:, sl], g[:, sl], 2e-2, f'{nm} {spec}')


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 31, 33, 64, 65, 127, 579, 640])
@pytest.mark.parametrize('spec', [None, 'causal', 'rows'])
def test_attention_bwd_ragged_lengths(L, spec):
    if spec == 'rows':
        spec = ('rows', [(L // 2, L // 2), (L // 2 + 1, L // 2 + 1)]) if L >= 4 else None
    B, H = 2, 2
    E = H * 64
    qkv, dO, out, lse2, dqkv = _run(B, L, H, spec, 1000 + L)
    assert torch.isfinite(dqkv.float()).all()
    g = _reference(qkv, dO, B, L, H, spec, torch.float32)
    for nm, sl in (('dQ', slice(0, E)), ('dK', slice(E, 2 * E)), ('dV', slice(2 * E, 3 * E))):
        if L == 1 and nm != 'dV':
            # one key: the softmax is constant, dQ and dK are exactly zero -- what is left is the bf16 rounding of delta = rowsum(dO * O)
            assert dqkv[:, sl].float().abs().max() <= 2e-2 * g[:, 2 * E:].abs().max(), nm
            continue
        close(dqkv[:, sl], g[:, sl], 2e-2, f'{nm} L={L} {spec}')


@pytest.mark.gpu
@pytest.mark.parametrize('spec', [None, 'causal', ROWS], ids=['none', 'causal', 'rows'])
def test_attention_bwd_two_launches_bitwise(spec):
    from mmvid_amd import ops
    B, L, H = 18, 579, 12
    E = H * 64
    qkv, dO, out, lse2, first = _run(B, L, H, spec, 11)
    bias = [torch.zeros(3 * E, device=DEV) for _ in range(2)]
    again = [ops.attention_bwd(qkv, out, dO, lse2, B, L, H, spec, dbias=bias[i]) for i in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(first, again[0]) and torch.equal(again[0], again[1])
    close(bias[0], again[0].float().sum(0), 2e-2, 'in-projection bias gradient')


def _kernel_metadata(name):
    """Register / scratch / LDS use of one kernel of csrc/attn.hip, from the device assembly the build flags produce."""
    from mmvid_amd.build import FLAGS
    src = os.path.join(REPO, 'mmvid_amd', 'csrc', 'attn.hip')
    flags = [f for f in FLAGS if f != '-fPIC']
    asm = subprocess.run(['hipcc', *flags, '--cuda-device-only', '-S', src, '-o', '-'], check=True, capture_output=True, text=True).stdout
    blocks = re.split(r'\n\s*-\s+\.', asm[asm.index('amdhsa.kernels:'):])
    for blk in blocks:
        m = re.search(r'\.name:\s+(\S+)', blk)
        if m and name in m.group(1) and not m.group(1).endswith('.kd'):
            return {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s*$', blk, re.M)}
    raise AssertionError(f'{name} not found in the device assembly')


def test_dkv_kernel_fits_three_blocks_per_cu():
    md = _kernel_metadata('attn_bwd_dkv_kernel')
    print(md)
    assert md['vgpr_count'] + md.get('agpr_count', 0) <= 168, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0, md
    assert md['group_segment_fixed_size'] <= 53 * 1024, md
