"""mmvid_amd/token_draw.py on the device: for the eight forms of a draw (guided or not x truncated or not x [the mask-predict caller |
the ART-V caller]) token_draw.draw equals, bit for bit, the sequence of ops calls that the four samplers' bodies held before the module
existed, restated here once each.  Both sides run the same kernels on the same inputs: no tolerance.  No model."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
R, V, RPS = 6, 257, 3  # two scale groups (a wrong grouping changes a token); one class past the 256-thread stride of the row kernels
K, P = 5, 0.9
STEP, STEP0 = 12, 10  # the ART-V form reads block STEP - STEP0 = 2 of the pre-drawn variates


@pytest.fixture(scope='module')
def inputs():
    gen = torch.Generator().manual_seed(4711)
    t = dict(lc=3.0 * torch.randn(R, V, generator=gen), lu=3.0 * torch.randn(R, V, generator=gen),
             E=torch.empty(3, R, V).exponential_(generator=gen), noise=torch.rand(R, V, generator=gen), scale=torch.tensor([0.0, 2.5]),
             step=torch.tensor([STEP], dtype=torch.int32))
    return {k: v.to(DEV) for k, v in t.items()}


def mask_predict_body(ops, i, guided, truncated):
    """sampling.mask_predict's draw_tokens: y wanted, noise at temperature 0.5, logit_div 1, a fresh tensor for the truncated value."""
    lc, lu, E, noise = i['lc'].clone(), i['lu'].clone(), i['E'][2].contiguous(), i['noise']
    if truncated:
        guide = dict(logits_u=lu, scale=i['scale'], rows_per_scale=RPS) if guided else {}
        return ops.sample_race(ops.logits_truncate(lc, K, P, want_kept=False, **guide), E, noise, 0.5)
    if not guided:
        return ops.sample_race(lc, E, noise, 0.5)
    return ops.sample_race_guided(lc, lu, i['scale'], RPS, E, noise, 0.5)


def artv_body(ops, i, guided, truncated, E, at):
    """artv_sampling.TokenLoop.draw after keep_top: the token alone into a static buffer, logit_div = the temperature 0.8, the truncation in
    place (unguided) or into a buffer of its own (guided), the variates indexed by a device scalar."""
    lc, lu, tok = i['lc'].clone(), i['lu'].clone(), torch.full((R, ), -1, dtype=torch.int64, device=DEV)
    lg = None
    if not guided:
        lg = lc
        if truncated:
            lg = ops.logits_truncate(lg, K, P, logit_div=0.8, out=lg, want_kept=False)
    elif truncated:
        lg = ops.logits_truncate(lc, K, P, logits_u=lu, scale=i['scale'], rows_per_scale=RPS, logit_div=0.8,
                                 out=torch.empty(R, V, device=DEV), want_kept=False)
    if lg is None:
        ops.sample_race_guided_at(lc, lu, i['scale'], RPS, E, logit_div=0.8, tok_out=tok, **at)
    else:
        ops.sample_race(lg, E, None, 0.0, logit_div=0.8, want_y=False, tok_out=tok, **at)
    return tok, None


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('truncated', [False, True])
def test_the_mask_predict_form(inputs, guided, truncated):
    from mmvid_amd import ops, token_draw
    i = inputs
    want_tok, want_y = mask_predict_body(ops, i, guided, truncated)
    lc, lu = i['lc'].clone(), i['lu'].clone()
    tok, y = token_draw.draw(lc, i['E'][2].contiguous(), logits_u=lu if guided else None, scale=i['scale'] if guided else None,
                             rows_per_scale=RPS, trunc=(K, P) if truncated else None, noise_u=i['noise'], temperature=0.5, want_y=True)
    assert torch.equal(tok, want_tok) and torch.equal(bits(y), bits(want_y))
    assert torch.equal(bits(lc), bits(i['lc'])) and torch.equal(bits(lu), bits(i['lu']))  # the operands are read only
    assert 0 <= int(tok.min()) and int(tok.max()) < V and bool(torch.isfinite(y).all())


@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('truncated', [False, True])
def test_the_artv_form(inputs, guided, truncated):
    from mmvid_amd import ops, token_draw
    i = inputs
    at = dict(step_dev=i['step'], step0=STEP0)
    want_tok, _ = artv_body(ops, i, guided, truncated, i['E'], at)
    lc, lu, lt, tok_buf = i['lc'].clone(), i['lu'].clone(), torch.empty(R, V, device=DEV), torch.full((R, ), -1, dtype=torch.int64, device=DEV)
    guide = dict(logits_u=lu, scale=i['scale'], rows_per_scale=RPS) if guided else {}
    tok, y = token_draw.draw(lc, i['E'], trunc=(K, P) if truncated else None, logit_div=0.8, want_y=False, tok_out=tok_buf,
                             trunc_out=lt if guided else lc, **guide, **at)
    assert tok is tok_buf and y is None and torch.equal(tok, want_tok)
    assert 0 <= int(tok.min()) and int(tok.max()) < V
    # block 2 of the variates is the one read: the same draw on E[2] alone
    alone, _ = artv_body(ops, i, guided, truncated, i['E'][2].contiguous(), {})
    assert torch.equal(tok, alone)
    if truncated and not guided:  # in place: the input holds the truncated value, at most K finite classes per row
        kept = torch.isfinite(lc)
        assert int(kept.sum(1).max()) <= K and torch.equal(bits(lc[kept]), bits(i['lc'][kept]))
    else:
        assert torch.equal(bits(lc), bits(i['lc']))
    if truncated and guided:
        assert int(torch.isfinite(lt).sum(1).max()) <= K and int(torch.isfinite(lt).sum(1).min()) >= 1


def test_the_forms_differ(inputs):
    """The inputs can tell the forms apart: guidance changes a token of the group with scale 2.5 and none of the group with scale 0, and
    another block of the variates gives other tokens (so an equality above is not the equality of constants)."""
    from mmvid_amd import ops, token_draw
    i = inputs
    E = i['E'][2].contiguous()
    plain = token_draw.draw(i['lc'], E, want_y=False)[0]
    guided = token_draw.draw(i['lc'], E, logits_u=i['lu'], scale=i['scale'], rows_per_scale=RPS, want_y=False)[0]
    assert torch.equal(plain[:RPS], guided[:RPS]) and not torch.equal(plain[RPS:], guided[RPS:])
    swapped = token_draw.draw(i['lc'], E, logits_u=i['lu'], scale=i['scale'].flip(0).contiguous(), rows_per_scale=RPS, want_y=False)[0]
    assert not torch.equal(swapped[:RPS], guided[:RPS])
    assert not torch.equal(plain, ops.sample_race(i['lc'], i['E'][0].contiguous(), None, 0.0, want_y=False)[0])
