"""Per-video sampling parameters, the host side: the keyword rules of sampling.check_video_params and every refusal before any device
work (models on the CPU: the first kernel call would raise MMVIDError), the declaration and the binding of mmvid_logits_truncate_rows,
its refusals (they come before the launch, so they run without a device), the launches token_draw makes from a per-row record, and what
stays pinned: 144 entries, ABI 3, a tensor in `top_k=` refused.  No GPU: nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_host_logic import tiny_bert, tiny_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX, V, B = 4, 256, 3


# ------------------------------------------------------------------------------------------------------ the keyword rules
def check(k=None, p=None, t=None, b=B, Tmax=None, **kw):
    from mmvid_amd.sampling import check_video_params
    return check_video_params(k, p, t, b, V, Tmax, **kw)


def test_accepted_forms():
    assert check() is None
    v = check(k=[4, 0, None])  # ART-V: vectors [b]; 0 and None are off
    assert v.k.dtype == np.int32 and v.k.tolist() == [4, 0, 0] and v.p is None and v.inv_div is None and v.on()
    assert not check(k=[0, None, V]).on() and check(k=[0, None, V + 9]).k.tolist() == [0, 0, 0]  # a k >= V keeps every class: stored as off
    v = check(p=(0.5, 1.0, None), t=torch.tensor([0.5, 2.0, 1.0]))
    assert v.p.dtype == np.float32 and v.p.tolist() == [0.5, 1.0, 1.0] and v.on()
    assert v.inv_div.dtype == np.float32 and v.inv_div.tolist() == [2.0, 0.5, 1.0]
    v = check(t=[0.7, None, 3])
    want = (np.float32(1.0) / np.array([0.7, 1.0, 3.0], np.float32)).astype(np.float32)  # the fp32 quotient the C entries compute
    assert v.inv_div.tobytes() == want.tobytes() and not v.on()
    assert check(k=torch.tensor([1, 2, 3], dtype=torch.int32)).k.tolist() == [1, 2, 3]
    assert check(k=np.array([1, 2, 255])).k.tolist() == [1, 2, 255]
    assert check(k=[np.int64(7), 1, 1], p=[np.float32(0.25), 1, 0.5]).p.tolist() == [0.25, 1.0, 0.5]
    # the mask-predict sampler: [b] holds for every step, [Tmax, b] has one row per step, step 0 included
    v = check(k=[4, 0, 2], Tmax=TMAX)
    assert v.k.shape == (TMAX, B) and v.k.flags['C_CONTIGUOUS'] and all(v.k[t].tolist() == [4, 0, 2] and v.on(t) for t in range(TMAX))
    table = [[0, 0, 0], [3, 0, 0], [0, 0, 0], [0, 0, 1]]
    v = check(k=torch.tensor(table), p=[[1.0, None, 1.0]] * TMAX, Tmax=TMAX)
    assert v.k.tolist() == table and [v.on(t) for t in range(TMAX)] == [False, True, False, True]
    assert v.p.shape == (TMAX, B) and bool((v.p == 1).all())
    # a scalar of the OTHER quantity composes
    assert check(k=[1, 2, 3], top_p=0.9).on() and check(p=[0.5, 1, 1], top_k=4, Tmax=TMAX, b=B).on(0)
    assert check(t=[1, 2, 3], temperature=1.0).inv_div.tolist()[0] == 1.0
    dev = check(k=[1, 2, 3], p=[0.5, 1, 1], t=[1, 2, 4]).device('cpu')
    assert [a.dtype for a in dev] == [torch.int32, torch.float32, torch.float32] and dev[2].tolist() == [1.0, 0.5, 0.25]


nan, inf = float('nan'), float('inf')
REFUSED = [dict(k=[1, 2]), dict(k=[1, 2, 3, 4]), dict(k=3), dict(k=torch.tensor(3)), dict(k=torch.ones(2, B, dtype=torch.int64)),  # length, shape
           dict(k=[True, 1, 1]), dict(k=torch.tensor([True, False, True])), dict(p=[True, 1.0, 1.0]), dict(t=[True, 1.0, 1.0]),  # a bool
           dict(k=[-1, 1, 1]), dict(k=[1.0, 1, 1]), dict(k=[1.5, 1, 1]), dict(k=torch.tensor([1.0, 2.0, 3.0])), dict(k=['4', 1, 1]),
           dict(k=torch.tensor([-2, 1, 1])),
           dict(p=[0.0, 1, 1]), dict(p=[-0.5, 1, 1]), dict(p=[1.0001, 1, 1]), dict(p=[nan, 1, 1]), dict(p=[inf, 1, 1]), dict(p=[1e-60, 1, 1]),
           dict(p=torch.tensor([0.5, 0.0, 1.0])), dict(p=[0.5, 0.5]), dict(p=0.5),
           dict(t=[0.0, 1, 1]), dict(t=[-1.0, 1, 1]), dict(t=[nan, 1, 1]), dict(t=[inf, 1, 1]), dict(t=[1e-45, 1, 1]), dict(t=[1.0, 1.0]), dict(t=0.7),
           dict(t=torch.ones(TMAX, B)),  # no per-token schedule in ART-V
           dict(k=[1, 2, 3], top_k=4), dict(p=[0.5, 1, 1], top_p=0.9), dict(t=[1, 2, 3], temperature=0.8)]  # the conflicting pairs


@pytest.mark.parametrize('kw', REFUSED, ids=lambda kw: re.sub(r'\s+', '', repr(kw))[:50])
def test_refusals(kw):
    with pytest.raises(ValueError, match='video_|top_k|top_p|temperature'):
        check(**kw)


def test_refusals_of_the_mask_predict_forms():
    for kw in (dict(k=[[1, 2, 3]] * (TMAX - 1)), dict(k=[[1, 2]] * TMAX), dict(p=torch.ones(TMAX + 1, B)), dict(k=[[1, 2, 3], [1, 2], [1, 2, 3], [1, 2, 3]]),
               dict(k=[[1, 2, 3], 4, 5, 6]), dict(t=[1.0, 1.0, 1.0]), dict(k=[[1, -2, 3]] * TMAX), dict(p=[[0.5, 0.0, 1.0]] * TMAX)):
        with pytest.raises(ValueError, match='video_'):
            check(Tmax=TMAX, **kw)


# ------------------------------------------------------------------------------------ the public entries, on CPU models
BAD = [(dict(video_top_k=[4, 4]), 'video_top_k'), (dict(video_top_k=[4, True]), 'video_top_k'), (dict(video_top_k=[4.0, 4]), 'video_top_k'),
       (dict(video_top_k=[-4, 4]), 'video_top_k'), (dict(video_top_k=torch.tensor([4.0, 4.0])), 'video_top_k'),
       (dict(video_top_p=[0.0, 0.5]), 'video_top_p'), (dict(video_top_p=[1.5, 0.5]), 'video_top_p'), (dict(video_top_p=[nan, 0.5]), 'video_top_p'),
       (dict(video_top_p=torch.tensor([0.5, 0.5, 0.5])), 'video_top_p'), (dict(video_top_k=[4, 4], top_k=4), 'top_k and video_top_k'),
       (dict(video_top_p=[0.5, 0.5], top_p=0.5), 'top_p and video_top_p')]
BAD[0] = (dict(video_top_k=[4, 4, 4]), 'video_top_k')  # (two videos below: three entries are a wrong length)


@pytest.fixture(scope='module')
def cpu_bert():
    torch.manual_seed(3)
    return tiny_bert()


@pytest.fixture(scope='module')
def cpu_artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(4)
    return DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
                 num_visuals=1, num_targets=2, transformer_layers=2)


def test_bert_refuses_before_any_device_work(cpu_bert, golden):
    from mmvid_amd import _lib, sampling
    mp = golden('mask_predict').meta['mp_config']
    text = torch.ones(2, 16, dtype=torch.int64)
    control = torch.zeros(2, cpu_bert.control_seq_len, 768)
    bert_bad = BAD + [(dict(video_temperature=[1.0, 1.0]), 'video_temperature'), (dict(video_top_k=[[1, 2]] * 3), 'video_top_k'),
                      (dict(video_top_p=torch.full((5, 2), 0.5)), 'video_top_p')]
    for kw, match in bert_bad:
        with pytest.raises(ValueError, match=match):
            cpu_bert.generate_images(text, mask_predict_steps=4, mp_config=mp, **kw)
        with pytest.raises(ValueError, match=match):
            cpu_bert.mask_predict(control, steps=4, mp_config=mp, **kw)
        with pytest.raises(ValueError, match=match):
            sampling.mask_predict(cpu_bert, control, steps=4, mp_config=mp, **kw)
    with pytest.raises(ValueError, match='video_top_k'):  # steps <= 0: the schedule's own length counts
        cpu_bert.generate_images(text, mask_predict_steps=0, mp_config=mp, video_top_k=[[1, 2]] * (mp['T'] + 1))
    with pytest.raises(ValueError, match='top_k'):  # the old keyword keeps its refusal of a tensor
        cpu_bert.generate_images(text, mask_predict_steps=4, mp_config=mp, top_k=torch.tensor([4, 4]))
    # accepted values pass the checks and reach the first kernel call, which a CPU model cannot make
    for kw in (dict(video_top_k=[4, 0]), dict(video_top_k=torch.tensor([[4, 0]] * 4), video_top_p=[0.5, None]), dict(video_top_p=[0.5, 1.0], top_k=3)):
        with pytest.raises(_lib.MMVIDError, match='no CPU path'):
            cpu_bert.mask_predict(control, steps=4, mp_config=mp, **kw)


def test_artv_refuses_before_any_device_work(cpu_artv):
    from mmvid_amd import _lib, completion
    m = cpu_artv
    text = torch.ones(2, 16, dtype=torch.int64)
    frames = torch.zeros(2, m.target_seq_len, dtype=torch.int64)
    given = torch.tensor([1, 0], dtype=torch.uint8)
    artv_bad = BAD + [(dict(video_temperature=[0.0, 1.0]), 'video_temperature'), (dict(video_temperature=[1.0, inf]), 'video_temperature'),
                      (dict(video_temperature=[1.0]), 'video_temperature'), (dict(video_temperature=[0.5, 2.0], temperature=0.8), 'temperature'),
                      (dict(video_top_k=[[1, 2]] * 4), 'video_top_k')]  # no per-token schedule
    for kw, match in artv_bad:
        with pytest.raises(ValueError, match=match):
            m.generate_images(text, **kw)
        with pytest.raises(ValueError, match=match):
            m.sample_tokens(text, **kw)
        with pytest.raises(ValueError, match=match):
            m.sampling_probs(torch.zeros(2, 256), **kw)
        with pytest.raises(ValueError, match=match):
            completion.complete_artv(m, text, frames, given, **kw)
    with pytest.raises(ValueError, match='top_k'):  # the old keyword keeps its refusal of a tensor
        m.sampling_probs(torch.zeros(2, 256), top_k=torch.tensor([4, 4]))
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):  # accepted: the per-row launch is the next thing that happens
        m.sampling_probs(torch.zeros(2, 256), video_top_k=[0, 0])


def test_the_keywords_are_where_the_documents_say():
    from mmvid_amd import completion, long_video, sampling
    from mmvid_amd.dalle_artv import DALLE
    from mmvid_amd.dalle_bert import BERT
    three, two = {'video_top_k', 'video_top_p', 'video_temperature'}, {'video_top_k', 'video_top_p'}
    # (generate_images and sample_tokens sit behind eval_decorator, which hides their signatures: the refusal tests above call them)
    for fn in (DALLE.sampling_probs, completion.complete_artv):
        assert three <= set(inspect.signature(fn).parameters), fn
    for fn in (BERT.mask_predict, sampling.mask_predict):
        assert two <= set(inspect.signature(fn).parameters), fn
    for fn in (completion.complete, completion.complete_seeded, long_video.generate_long):  # out of scope, and said to be
        assert not three & set(inspect.signature(fn).parameters), fn
    assert 'def check_video_params(' in inspect.getsource(sampling).split('def check_truncation(')[1].split('def check_guidance_artv(')[0]  # beside it


# ----------------------------------------------------------------------------------------------------- the token draw
R_, V_ = 6, 257


@pytest.fixture
def calls(monkeypatch):
    """The operators token_draw calls, replaced by recorders that return CPU tensors -> the list of (name, args, kwargs)."""
    from mmvid_amd import ops
    log = []

    def recorder(name, result):
        def op(*args, **kw):
            log.append((name, args, kw))
            return result(*args, **kw)
        monkeypatch.setattr(ops, name, op)

    def truncated(logits, *a, out=None, want_kept=False, **kw):
        out = out if out is not None else torch.full((R_, V_), 7.0)
        return (out, torch.full((R_, ), 3, dtype=torch.int32)) if want_kept else out

    recorder('sample_race', lambda *a, **kw: (torch.zeros(R_, dtype=torch.int64), torch.zeros(R_) if kw.get('want_y', True) else None))
    recorder('sample_race_guided', lambda *a, **kw: (torch.zeros(R_, dtype=torch.int64), torch.zeros(R_)))
    recorder('sample_race_guided_at', lambda *a, **kw: torch.zeros(R_, dtype=torch.int64))
    recorder('logits_truncate', truncated)
    recorder('logits_truncate_rows', truncated)
    return log


@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('divisors', [False, True])
def test_a_per_row_record_is_one_rows_launch_and_the_plain_race(calls, guided, divisors):
    from mmvid_amd import token_draw
    gen = torch.Generator().manual_seed(12)
    lc, lu, E = torch.randn(R_, V_, generator=gen), torch.randn(R_, V_, generator=gen), torch.rand(R_, V_, generator=gen)
    scale, lt = torch.tensor([0.0, 2.5]), torch.empty(R_, V_)
    k, p = torch.tensor([1, 0, 5], dtype=torch.int32), torch.tensor([1.0, 0.5, 0.9])
    inv = torch.tensor([1.0, 2.0, 0.5]) if divisors else None
    rows = token_draw.RowParams(2, k, p, inv, top_k=None, top_p=None)
    guide = dict(logits_u=lu, scale=scale, rows_per_scale=3) if guided else {}
    record = {}
    tok, y = token_draw.draw(lc, E, trunc=rows, logit_div=1.0 if divisors else 0.8, want_y=False, trunc_out=lt, record=record, **guide)
    assert [c[0] for c in calls] == ['logits_truncate_rows', 'sample_race'] and y is None  # one launch more than the untruncated draw, as the scalar form
    _, args, kw = calls[0]
    assert len(args) == 1 and args[0] is lc
    assert kw['rows_k'] is k and kw['rows_p'] is p and kw['rows_inv_div'] is inv and kw['rows_per_param'] == 2
    assert kw['divide_out'] is divisors and kw['out'] is lt and kw['want_kept'] is True and kw['top_k'] is None and kw['top_p'] is None
    assert kw['logit_div'] == (1.0 if divisors else 0.8)
    assert ({'logits_u', 'scale', 'rows_per_scale'} <= set(kw)) == guided
    _, args, kw = calls[1]
    assert args[0] is lt and args[1] is E and kw['logit_div'] == (1.0 if divisors else 0.8)  # divided already: the race divides by 1
    assert set(record) == {'logits_t', 'kept', 'rows_k', 'rows_p', 'rows_inv_div', 'rows_per_param'}
    assert record['rows_k'] is k and record['rows_p'] is p and record['rows_inv_div'] is inv and record['rows_per_param'] == 2
    assert token_draw.race_div(rows, 0.8) == (1.0 if divisors else 0.8) and token_draw.race_div((5, 0.9), 0.8) == 0.8 and token_draw.race_div(None, 0.8) == 0.8
    sub = rows.rows(torch.tensor([2, 0]))
    assert sub.k.tolist() == [5, 1] and torch.equal(sub.p, p[[2, 0]]) and sub.rows_per_param == 2 and (sub.inv_div is None) == (inv is None)


def test_a_temperature_record_divides_with_a_scalar_race_temperature_of_one(calls):
    """video_temperature alone: the record holds divisors only; the rows launch divides (both filters off) and the race runs with 1."""
    from mmvid_amd import token_draw
    lc, E = torch.zeros(R_, V_), torch.ones(R_, V_)
    rows = token_draw.RowParams(1, None, None, torch.full((R_, ), 2.0))
    token_draw.draw(lc, E, trunc=rows, logit_div=1.0, want_y=True)
    assert [c[0] for c in calls] == ['logits_truncate_rows', 'sample_race']
    assert calls[0][2]['divide_out'] is True and calls[0][2]['rows_k'] is None and calls[1][2]['logit_div'] == 1.0


# ------------------------------------------------------------------------------------------------ declaration and binding
def test_the_entry_is_declared_in_the_ext_header_and_bound():
    from mmvid_amd import _cdecl, _lib
    text = open(_cdecl.EXT_HEADER_PATH).read()
    hdr = _cdecl.parse(text)
    name = 'mmvid_logits_truncate_rows'
    assert name in hdr.functions and hdr.functions[name][0] is ctypes.c_int
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    assert len(re.findall(r'\b%s\s*\(' % name, bare)) == 1
    P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.EXT_SIGNATURES[name] == hdr.functions[name][1] == [P, P, I64, P, I64, F, I, F, P, P, P, I64, I, I64, I, P, I64, P, P]
    assert name not in _lib.SIGNATURES and name not in _lib.OTHER and name not in _lib.HEADER.functions
    assert re.search(r'\bint\s+mmvid_logits_truncate_rows\s*\(const float\* logits, const float\* logits_u, int64_t ld, const float\* scale_dev, '
                     r'int64_t rows_per_scale,\s*float logit_div, int top_k, float top_p, const int32_t\* top_k_dev, const float\* top_p_dev,\s*'
                     r'const float\* inv_div_dev, int64_t rows_per_param, int divide_out, int64_t R, int V,\s*float\* out, int64_t ld_out, '
                     r'int32_t\* kept, void\* stream\);', text)
    comment = text[:text.index('int mmvid_logits_truncate_rows')].rsplit('/* ----', 1)[1]
    for phrase in ('dalle_artv.py', 'dalle_bert.py', 'rows_per_param', 'divide_out', 'byte for byte', 'Refused', '4-byte aligned', 'No atomics'):
        assert phrase in comment, phrase
    lib = _lib.load()
    assert name not in lib._mmvid_missing
    fn = getattr(lib, name)
    assert list(fn.argtypes) == list(_lib.EXT_SIGNATURES[name]) and fn.restype is ctypes.c_int


def test_the_pinned_counts_stand():
    from mmvid_amd import _lib
    assert len(_lib.SIGNATURES) + len(_lib.OTHER) == 144 and _lib.ABI_VERSION == 3
    assert 'mmvid_logits_truncate' in _lib.SIGNATURES  # the scalar entry is where it was


def test_the_new_kernel_uses_no_atomics_no_lds_and_shares_the_rule():
    src = open(os.path.join(ROOT, 'mmvid_amd', 'csrc', 'sample.hip')).read()
    kernel = re.search(r'void logits_truncate_rows_kernel\(.*?\n\}', src, re.S).group(0)
    assert 'atomic' not in kernel and '__shared__' not in kernel and '__syncthreads' not in kernel
    assert 'guided_logit(x[c], xu[c], w)' in kernel and len(re.findall(r'float guided_logit\(', src)) == 1
    shared = re.search(r'uint32_t truncate_keep\(.*?\n\}', src, re.S).group(0)  # the searches: one definition, called by both kernels
    assert 'atomic' not in shared and '__shared__' not in shared and '__syncthreads' not in shared
    old = re.search(r'void logits_truncate_kernel\(.*?\n\}', src, re.S).group(0)
    assert 'truncate_keep<NS>(' in kernel and 'truncate_keep<NS>(' in old and len(re.findall(r'uint32_t truncate_keep\(', src)) == 1
    assert ' / ' not in re.sub(r'//.*', '', kernel).replace('r / rows_per_param', '').replace('r / rows_per_scale', '')  # the device never divides
    entry = re.search(r'extern "C" int mmvid_logits_truncate_rows\(.*?\n\}', src, re.S).group(0)
    assert 'atomic' not in entry


def test_the_entry_refuses_before_it_launches():
    """Every refusal precedes the launch, so a host without a device sees it: a nonzero status and its text."""
    from mmvid_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    ok = dict(logits=p, lu=None, ld=8, scale=None, rps=1, div=1.0, k=2, p=0.9, rk=p, rp=p, ri=p, rpp=2, divide=0, R=4, V=8, out=p, ld_out=8)
    bad = [dict(V=0), dict(V=2049), dict(ld=7), dict(ld_out=7), dict(R=-1), dict(div=0.0), dict(p=0.0), dict(p=float('nan')), dict(lu=p), dict(scale=p),
           dict(lu=p, scale=p, rps=3), dict(logits=None), dict(out=None), dict(rpp=0), dict(rpp=-1), dict(rpp=3), dict(rk=odd), dict(rp=odd),
           dict(ri=odd), dict(divide=2), dict(divide=-1)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(_lib.MMVIDError, match=r'rc=[1-9-].*logits_truncate_rows: \S') as err:
            _lib.call('mmvid_logits_truncate_rows', a['logits'], a['lu'], a['ld'], a['scale'], a['rps'], a['div'], a['k'], a['p'], a['rk'], a['rp'],
                      a['ri'], a['rpp'], a['divide'], a['R'], a['V'], a['out'], a['ld_out'], None, None)
        assert 'launch failed' not in str(err.value), change
    assert not any(buf)
