"""mmvid_amd/token_draw.py, the host side: for the eight forms of a draw (guided or not x truncated or not x [y with noise, or token only])
the exact sequence of operators and the arguments by which the callers differ, the one launch of a materialised guided value, and the rule
for the unconditional prompt of a guided call.  No GPU: the four operators are replaced by recorders that return CPU tensors."""
import itertools

import pytest
import torch

R, V = 6, 257


@pytest.fixture
def calls(monkeypatch):
    """ops.sample_race, sample_race_guided, sample_race_guided_at and logits_truncate replaced -> the list of (name, args, kwargs)."""
    from mmvid_amd import ops
    log = []

    def recorder(name, result):
        def op(*args, **kw):
            log.append((name, args, kw))
            return result(*args, **kw)
        monkeypatch.setattr(ops, name, op)

    def tok(kw):
        return kw['tok_out'] if kw.get('tok_out') is not None else torch.zeros(R, dtype=torch.int64)

    def truncated(logits, top_k=None, top_p=None, *, out=None, want_kept=False, **kw):
        out = out if out is not None else torch.full((R, V), 7.0)
        return (out, torch.full((R, ), 3, dtype=torch.int32)) if want_kept else out

    recorder('sample_race', lambda *a, **kw: (tok(kw), torch.zeros(R) if kw.get('want_y', True) else None))
    recorder('sample_race_guided', lambda *a, **kw: (torch.zeros(R, dtype=torch.int64), torch.zeros(R)))
    recorder('sample_race_guided_at', lambda *a, **kw: tok(kw))
    recorder('logits_truncate', truncated)
    return log


@pytest.fixture
def operands():
    gen = torch.Generator().manual_seed(11)
    return dict(lc=torch.randn(R, V, generator=gen), lu=torch.randn(R, V, generator=gen), E=torch.rand(R, V, generator=gen),
                noise=torch.rand(R, V, generator=gen), scale=torch.tensor([0.0, 2.5]), lt=torch.empty(R, V),
                tok=torch.empty(R, dtype=torch.int64), step=torch.tensor([12], dtype=torch.int32))


FORMS = list(itertools.product((False, True), (False, True), (True, False)))  # guided, truncated, [y with noise | token only]


@pytest.mark.parametrize('guided,truncated,with_y', FORMS)
@pytest.mark.parametrize('recorded', [False, True])
def test_the_launches_of_every_form(calls, operands, guided, truncated, with_y, recorded):
    from mmvid_amd import token_draw
    o = operands
    record = {} if recorded else None
    guide = dict(logits_u=o['lu'], scale=o['scale'], rows_per_scale=3) if guided else {}
    # the mask-predict caller wants y and brings noise; the ART-V caller wants the token alone, in its own buffers
    form = dict(noise_u=o['noise'], temperature=0.5, want_y=True) if with_y else \
        dict(want_y=False, tok_out=o['tok'], step_dev=o['step'], step0=10, trunc_out=o['lt'] if guided else o['lc'])
    got = token_draw.draw(o['lc'], o['E'], trunc=(5, 0.9) if truncated else None, logit_div=0.8, record=record, **guide, **form)

    race = 'sample_race' if truncated or not guided else ('sample_race_guided' if with_y else 'sample_race_guided_at')
    assert [c[0] for c in calls] == (['logits_truncate'] if truncated else []) + [race]
    lg = o['lc']
    if truncated:
        _, args, kw = calls[0]
        assert args[0] is o['lc'] and tuple(args[1:]) == (5, 0.9)
        assert kw['logit_div'] == 0.8 and kw['want_kept'] is recorded
        assert kw['out'] is (None if with_y else (o['lt'] if guided else o['lc']))  # out is trunc_out; unguided ART-V: in place
        if guided:
            assert kw['logits_u'] is o['lu'] and kw['scale'] is o['scale'] and kw['rows_per_scale'] == 3
        else:
            assert not {'logits_u', 'scale', 'rows_per_scale'} & set(kw)
        lg = kw['out'] if kw['out'] is not None else None  # (None: the recorder's own tensor, checked below by its value)
    _, args, kw = calls[-1]
    if race == 'sample_race':  # plain: after a guided truncation too, and then without logits_u
        assert len(args) == 4 and 'logits_u' not in kw and not any(a is o['lu'] for a in args)
        assert (args[0] is lg) if lg is not None else bool((args[0] == 7.0).all())
        assert args[1] is o['E'] and kw['logit_div'] == 0.8 and kw['want_y'] is with_y
        assert (args[2] is o['noise'] and args[3] == 0.5) if with_y else (args[2] is None and args[3] == 0.0)
        assert kw['tok_out'] is (None if with_y else o['tok']) and kw['step_dev'] is (None if with_y else o['step'])
        assert kw['step0'] == (0 if with_y else 10)
    elif race == 'sample_race_guided':
        assert args[0] is o['lc'] and args[1] is o['lu'] and args[2] is o['scale'] and args[3] == 3 and args[4] is o['E']
        assert args[5] is o['noise'] and args[6] == 0.5 and kw == dict(logit_div=0.8)
    else:
        assert args[0] is o['lc'] and args[1] is o['lu'] and args[2] is o['scale'] and args[3] == 3 and args[4] is o['E']
        assert kw == dict(logit_div=0.8, tok_out=o['tok'], step_dev=o['step'], step0=10)
    tok, y = got
    assert tok.shape == (R, ) and (y is not None) == with_y and (with_y or tok is o['tok'])
    if recorded and truncated:
        assert set(record) == {'logits_t', 'kept'} and record['logits_t'].shape == (R, V) and int(record['kept'][0]) == 3
    elif recorded:
        assert record == {}


def test_a_guided_draw_with_y_takes_no_token_buffer(calls, operands):
    from mmvid_amd import token_draw
    o = operands
    with pytest.raises(ValueError, match='token-only'):
        token_draw.draw(o['lc'], o['E'], logits_u=o['lu'], scale=o['scale'], rows_per_scale=3, want_y=True, tok_out=o['tok'])
    assert calls == []


def test_race_value(calls, operands):
    from mmvid_amd import token_draw
    o = operands
    guide = dict(logits_u=o['lu'], scale=o['scale'], rows_per_scale=1)
    for kw in ({}, dict(materialise=True), dict(out=o['lt'], record={})):  # unguided, no filter: the logits themselves
        lg, lu = token_draw.race_value(o['lc'], **kw)
        assert lg is o['lc'] and lu is None
    lg, lu = token_draw.race_value(o['lc'], **guide)
    assert lg is o['lc'] and lu is o['lu'] and calls == []  # nothing to remove, nothing to write out: no launch
    lg, lu = token_draw.race_value(o['lc'], logit_div=0.8, materialise=True, **guide)  # sampling_probs, guided, both filters off
    assert len(calls) == 1 and calls[0][0] == 'logits_truncate' and lu is None and bool((lg == 7.0).all())
    _, args, kw = calls[0]
    assert args[0] is o['lc'] and tuple(args[1:]) == (None, None)  # the copy-through form
    assert kw == dict(logit_div=0.8, out=None, want_kept=False, **guide)


def test_unconditional_inputs():
    """The six cases of (drop, negative_text) that BERT.guidance_control and DALLE.generate_images build."""
    from mmvid_amd.sampling import unconditional_inputs
    text, visual, negative = torch.arange(1, 9).view(2, 4), torch.arange(6).view(2, 3), torch.full((2, 4), 5)
    pad = torch.zeros_like(text)
    cases = [(('text', 'visual'), None, pad, None), (('text', ), None, pad, visual), (('visual', ), None, text, None),
             (('text', 'visual'), negative, negative, None), (('visual', ), negative, negative, None), ((), negative, negative, visual)]
    for drop, neg, want_text, want_visual in cases:
        text_u, visual_u = unconditional_inputs(text, visual, drop, neg)
        assert torch.equal(text_u, want_text) and text_u.dtype == text.dtype, (drop, neg)
        assert visual_u is want_visual, (drop, neg)
    assert unconditional_inputs(text, visual, ('visual', ), None)[0] is text  # (the text kept: no copy)
    assert unconditional_inputs(text, None, ('text', ), None)[1] is None  # a model or a call without a visual control
