"""mmvid_amd/shadow.py without a GPU: when a cached copy of a weight is rebuilt, and what an attachment promises.  `ops.cast_bf16` is
replaced by torch's cast (the kernel's rounding is pinned in test_optim_exact_gpu.py and test_abi_contract_gpu.py).  A "raw" write
stands in for the Adam kernel: it changes the storage through numpy and leaves `_version` alone."""
import pytest
import torch

from mmvid_amd import ops, shadow


@pytest.fixture(autouse=True)
def torch_cast(monkeypatch):
    monkeypatch.setattr(ops, 'cast_bf16', lambda x, out=None: x.bfloat16() if out is None else out.copy_(x))


def param(*shape, seed=0):
    return torch.nn.Parameter(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def raw_write(p, v):
    version = p._version
    p.detach().numpy()[...] = v
    assert p._version == version


def bf16(p):
    return p.detach().bfloat16()


# ---------------------------------------------------------------------------------------------------------------------- Cached
def counted(ps):
    calls = []

    def build():
        calls.append(1)
        return [bf16(p) for p in ps]

    return shadow.Cached(lambda: ps, build), calls


def test_key_of_is_version_pointer_device():
    p = param(3, 4)
    assert shadow.key_of([p, p]) == ((p._version, p.data_ptr(), p.device), ) * 2


def test_cached_builds_once_over_repeated_gets():
    ps = [param(3, 4), param(5, seed=1)]
    c, calls = counted(ps)
    first = c.get()
    assert all(c.get() is first for _ in range(3)) and len(calls) == 1


@pytest.mark.parametrize('which', [0, 1])
def test_cached_rebuilds_after_a_torch_write_to_any_source(which):
    ps = [param(3, 4), param(5, seed=1)]
    c, calls = counted(ps)
    c.get()
    with torch.no_grad():
        ps[which].mul_(2.0)
    got = c.get()
    assert len(calls) == 2 and torch.equal(got[which], bf16(ps[which]))
    c.get()
    assert len(calls) == 2


def test_cached_rebuilds_after_the_data_moved():
    ps = [param(3, 4), param(5, seed=1)]
    c, calls = counted(ps)
    c.get()
    ps[1].data = torch.full((5, ), 7.0)
    assert torch.equal(c.get()[1], torch.full((5, ), 7.0).bfloat16()) and len(calls) == 2
    c.get()
    assert len(calls) == 2


def test_cached_rebuilds_after_invalidate_and_not_otherwise():
    ps = [param(3, 4)]
    c, calls = counted(ps)
    c.get(), c.get()
    ps[0].grad = torch.ones(3, 4)  # (nothing a derived copy depends on)
    ps[0].requires_grad_(False)
    c.get()
    assert len(calls) == 1
    c.invalidate()
    assert len(calls) == 1  # (the rebuild waits for the next get())
    c.get(), c.get()
    assert len(calls) == 2


# ---------------------------------------------------------------------------------------------------------- Bf16Weight, unattached
def test_bf16_weight_is_the_cast_of_the_parameter():
    p = param(6, 8)
    w = shadow.Bf16Weight(p)
    got = w.get()
    assert got.dtype == torch.bfloat16 and torch.equal(got, bf16(p)) and w.get() is got


def test_bf16_weight_recasts_in_place_after_a_torch_write():
    p = param(6, 8)
    w = shadow.Bf16Weight(p)
    ptr = w.get().data_ptr()
    with torch.no_grad():
        p.add_(1.0)
    got = w.get()
    assert got.data_ptr() == ptr and torch.equal(got, bf16(p))
    p.data = torch.full((6, 8), 3.0)  # same shape and device elsewhere: still the same copy, cast again
    got = w.get()
    assert got.data_ptr() == ptr and torch.equal(got, bf16(p))


def test_bf16_weight_allocates_anew_for_another_shape():
    p = param(6, 8)
    w = shadow.Bf16Weight(p)
    old = w.get()
    p.data = torch.arange(40.0).view(10, 4)
    got = w.get()
    assert got is not old and got.shape == (10, 4) and torch.equal(got, bf16(p))
    assert old.shape == (6, 8)  # (whoever still holds the old copy keeps a whole tensor)


def test_bf16_weight_does_not_see_a_raw_write():
    """Why an optimiser that writes through pointers must attach: the key does not move."""
    p = param(6, 8)
    w = shadow.Bf16Weight(p)
    before = w.get().clone()
    raw_write(p, 5.0)
    assert torch.equal(w.get(), before) and not torch.equal(before, bf16(p))
    w.invalidate()
    assert torch.equal(w.get(), bf16(p))


# ------------------------------------------------------------------------------------------------------------ Bf16Weight, attached
def attached(shape=(6, 8)):
    p = param(*shape)
    view = bf16(p).clone()
    w = shadow.Bf16Weight(p)
    w.attach(view)
    return p, view, w


def test_attached_weight_returns_the_view():
    p, view, w = attached()
    assert w.get().data_ptr() == view.data_ptr() and w.get() is view


def test_attached_view_is_left_alone_after_the_owners_write():
    p, view, w = attached()
    raw_write(p, 2.5)
    view.fill_(-1.0)  # the owner's write of the view: anything get() wrote over it would show
    w.mark_fresh()
    got = w.get()
    assert got is view and bool((view == -1.0).all())


def test_mark_fresh_records_the_version_of_a_torch_write_the_owner_overwrote():
    p, view, w = attached()
    with torch.no_grad():
        p.mul_(3.0)
    view.fill_(-1.0)
    w.mark_fresh()
    assert w.get() is view and bool((view == -1.0).all())


def test_attached_view_is_recast_after_a_torch_write():
    p, view, w = attached()
    ptr = view.data_ptr()
    with torch.no_grad():
        p.mul_(3.0)
    got = w.get()
    assert got is view and got.data_ptr() == ptr and torch.equal(view, bf16(p))
    view.fill_(-1.0)  # cast once: the next get() finds the version it recorded
    assert w.get() is view and bool((view == -1.0).all())


def test_attachment_is_void_once_the_parameter_moved():
    p, view, w = attached()
    kept = view.clone()
    p.data = torch.full((6, 8), 9.0)
    got = w.get()
    assert got.data_ptr() != view.data_ptr() and torch.equal(got, bf16(p)) and torch.equal(view, kept)


def test_invalidate_detaches():
    p, view, w = attached()
    kept = view.clone()
    w.invalidate()
    with torch.no_grad():
        p.mul_(0.5)
    got = w.get()
    assert got.data_ptr() != view.data_ptr() and torch.equal(got, bf16(p)) and torch.equal(view, kept)
    w.mark_fresh()  # nothing attached: nothing to record
    assert w.get() is got


def test_mark_fresh_without_attachment_is_a_no_op():
    p = param(6, 8)
    w = shadow.Bf16Weight(p)
    w.mark_fresh()
    got = w.get()
    with torch.no_grad():
        p.mul_(2.0)
    w.mark_fresh()
    assert torch.equal(w.get(), bf16(p)) and w.get() is got


# ------------------------------------------------------------------------------------------------------- the models that hold them
def replace(holder, name):
    """What load_state_dict(assign=True) does: another Parameter object under the same name."""
    new = torch.nn.Parameter(getattr(holder, name).detach() * 2.0 + 1.0)
    setattr(holder, name, new)
    return new


def test_tower_operands_follow_a_replaced_parameter_object():
    from mmvid_amd.clip_tower import OpenAICLIPTransformer
    tw = OpenAICLIPTransformer(8, 'openai_clip_text', layers=2, width=64, heads=1)
    ps = list(tw._matrix_params())
    assert len(ps) == 8 and ps[5] is tw.transformer.resblocks[1].attn.out_proj.weight
    before = tw._sync_shadow()
    held = list(tw.bf16_weights())
    assert all(torch.equal(s, bf16(p)) for s, p in zip(before, ps)) and all(w.param is p for w, p in zip(held, ps))
    new = replace(tw.transformer.resblocks[1].attn.out_proj, 'weight')
    after = tw._sync_shadow()
    assert list(tw._matrix_params())[5] is new and torch.equal(after[5], bf16(new)) and not torch.equal(after[5], before[5])
    for i, w in enumerate(tw.bf16_weights()):  # the others keep their object and their copy
        assert (w is held[i]) == (i != 5) and (after[i].data_ptr() == before[i].data_ptr()) == (i != 5)
    tw.load_state_dict({k: v * 0.5 for k, v in tw.state_dict().items()}, assign=True)
    assert all(torch.equal(s, bf16(p)) for s, p in zip(tw._sync_shadow(), tw._matrix_params()))


def test_bert_head_operands_follow_a_replaced_parameter_object_and_refuse_a_stranger():
    from test_host_logic import tiny_bert
    m = tiny_bert(fixed_language_model='roberta-large', text_feature_dim=1024, text_emb_bottleneck=None)
    heads = m.head_shadow_targets()
    assert heads == [m.to_logits[1], m.text_feature_mapping] and [w.param for w in m.bf16_weights()] == [h.weight for h in heads]
    first = [m._w16(h) for h in heads]
    assert all(torch.equal(f, bf16(h.weight)) for f, h in zip(first, heads)) and m._w16(heads[1]) is first[1]
    new = replace(m.text_feature_mapping, 'weight')
    assert torch.equal(m._w16(m.text_feature_mapping), bf16(new)) and m._w16(heads[0]) is first[0]
    with pytest.raises(ValueError, match='head_shadow_targets'):
        m._w16(m.to_logits_rel[1])


def test_artv_head_operand_follows_a_replaced_parameter_object():
    from mmvid_amd.dalle_artv import DALLE
    from test_host_logic import tiny_vae
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=64, text_seq_len=4, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=1, transformer_layers=1)
    first = m._w16()
    assert torch.equal(first, bf16(m.to_logits[1].weight)) and m._w16() is first
    new = replace(m.to_logits[1], 'weight')
    assert torch.equal(m._w16(), bf16(new)) and m.bf16_weights()[0].param is new


def test_vqgan_prepared_dict_is_renewed_when_a_weight_changes():
    from test_host_logic import tiny_vae
    v = tiny_vae()
    d = v._prepared()
    d['x'] = 1
    assert v._prep is d and v._prepared() is d
    v._prep.clear()
    assert v._prepared() == {} and v._prepared() is d
    d['x'] = 1
    with torch.no_grad():
        v.model.quantize.embedding.weight.add_(1.0)
    assert v._prepared() == {} and v._prep is v._prepared() and v._prep is not d
