"""CPU checks of the exact decode-step construction (tests/decode_exact.py): what tests/test_decode_exact_gpu.py compares the kernels
with bit for bit must itself be the only possible fp32 result, and must tell a subtly wrong kernel from a right one.

  * every fc pre-activation lies in the alphabet on which QuickGELU is exact after the bf16 rounding;
  * for every linear stage sum |terms| < 2^24 x (last bit of the smallest term): any summation order gives the same fp32 value
    (the condition of tests/test_integer_exact.py, scaled by the census fractions' quantum);
  * census counts are at most 64; for every cache length n the GPU tests use, a key dropped (denominator n or n - 1), a key counted
    twice and a key read in place of another all change the expected bf16 bits;
  * the fp64 reference equals a plain torch fp32 evaluation of the layer on the same parameters."""
import pytest
import torch

import decode_exact as dx

BF = torch.bfloat16
ALL_N = sorted({n for c in dx.ATTN_CASES.values() for n in c['n']} | {n for runs in dx.PERSISTENT_RUNS.values() for r in runs for n in r} | set(dx.LINEAR_N))


def _prepared(master, layers, B, E, mode, pos):
    cache = master.clone()
    dx.poison_from(cache, pos)
    if mode == 'spot':
        dx.light(cache, dx.spot_keys(layers, B, E // 64, pos + 1), 0.0)
    return cache


def _cases():
    out = [(name, c['E'], 1, False, c['Lmax'], c['n']) for name, c in dx.ATTN_CASES.items()]
    out += [(f'persistent{Lmax}', 768, 1, False, Lmax, tuple(n for r in runs for n in r)) for Lmax, runs in dx.PERSISTENT_RUNS.items()]
    out += [(f'linear{E}', E, 2, True, dx.LINEAR_LMAX, dx.LINEAR_N) for E in dx.LINEAR_B]
    return out


@pytest.mark.parametrize('mode', dx.MODES)
@pytest.mark.parametrize('name,E,layers,rich,Lmax,ns', _cases(), ids=[c[0] for c in _cases()])
def test_every_stage_is_exact_in_any_summation_order(name, E, layers, rich, Lmax, ns, mode):
    """From the actual tensors (two sequences of the case: the bound does not depend on the sequence beyond its hash): alphabet,
    sum |terms| bounds of the in-projection, fc and the residual chain, census counts <= 64 and denominators == n."""
    B = 2
    P = dx.tower_params(E, layers, mode, rich)
    master = dx.cache_master(layers, B, Lmax, E, mode)
    x = dx.step_input(B, E, rich)
    for n in ns:
        cache, info = _prepared(master, layers, B, E, mode, n - 1), {}
        dx.reference_step(P, cache, x, n - 1, info)
        dx.assert_exact_conditions(info, f'{name} {mode} n={n}')
        assert bool(torch.isnan(cache[:, :, n:].float()).all()) and not bool(torch.isnan(cache[:, :, :n].float()).any())
        for l, d in enumerate(info['layers']):
            if mode == 'census':
                assert bool((d['den'] == n).all())
                assert float((d['num'].reshape(B, E) - P[l]['v_new']).max()) <= 64
            else:
                assert bool((d['den'] == 1).all()), 'one key per (sequence, head) carries all the weight'


def _bits(num, den):
    return (num.float() / torch.tensor(float(den))).to(BF).view(torch.int16)


@pytest.mark.parametrize('E', [768, 512])
def test_census_tells_a_dropped_a_doubled_and_a_swapped_key(E):
    H = E // 64
    h = torch.arange(H).view(H, 1)
    for l, s in [(0, 0), (0, 1), (1, 63)]:
        v = dx.tower_params(E, 2, 'census', False)[l]['v_new'].view(H, 64)
        for n in ALL_N:
            if n < 2:
                continue
            k = torch.arange(n - 1).view(1, -1)
            dims = dx.census_dim(l, s, h, k)                                   # [H, n - 1]
            cnt = torch.zeros(H, 64, dtype=torch.float64).scatter_add_(1, dims, torch.ones(H, n - 1, dtype=torch.float64))
            assert float(cnt.max()) <= 64
            want = _bits(cnt + v, n)
            # one key less / more in a dimension, same denominator: the bits of that dimension move (a swap is one of each)
            assert bool((_bits(cnt + v - 1, n) != want)[cnt > 0].all()), (l, s, n)
            assert bool((_bits(cnt + v + 1, n) != want).all()), (l, s, n)
            # no two keys share their dimension in every head: a key read in place of another moves some head
            assert torch.unique(dims.t(), dim=0).shape[0] == n - 1
            # one key less AND the denominator n - 1 (a loop bound off by one): seen[h, d'] = dropping a key of dimension d' shows in head h
            drop = cnt.view(H, 1, 64) - torch.eye(64, dtype=torch.float64).view(1, 64, 64)
            seen = (_bits(drop + v.view(H, 1, 64), n - 1) != want.view(H, 1, 64)).any(-1)
            assert bool(seen.gather(1, dims).any(0).all()), (l, s, n)


@pytest.mark.parametrize('mode', dx.MODES)
@pytest.mark.parametrize('E,layers,rich,B,Lmax,n', [(768, 2, True, 3, 64, 33), (512, 2, True, 2, 64, 64), (768, 1, False, 2, 300, 257),
                                                    (512, 1, False, 3, 64, 1)])
def test_reference_equals_plain_torch_fp32(E, layers, rich, B, Lmax, n, mode):
    P = dx.tower_params(E, layers, mode, rich)
    cache = _prepared(dx.cache_master(layers, B, Lmax, E, mode), layers, B, E, mode, n - 1)
    x = dx.step_input(B, E, rich)
    y32, row = dx.torch_fp32_step(P, cache, x, n - 1)
    y = dx.reference_step(P, cache, x, n - 1)
    assert torch.equal(y32, y)
    assert torch.equal(cache[-1, :, n - 1].float(), row)


def test_spot_values_spell_their_key():
    """V[k] of the 'spot' cache differs between any two (layer, sequence, head, key) the tests use."""
    ar = lambda n, shape: torch.arange(n).view(shape)
    v = dx.spot_value(torch.tensor(1), ar(70, (70, 1, 1, 1)), ar(12, (1, 1, 12, 1)), ar(4096, (1, 4096, 1, 1))[:, ::37], ar(64, (1, 1, 1, 64)) + torch.zeros(70, 111, 12, 1, dtype=torch.int64))
    assert torch.unique(v.reshape(-1, 64)[:, :13], dim=0).shape[0] == 70 * 111 * 12
    assert int(v.max()) <= 3 and int(v.min()) >= 0
