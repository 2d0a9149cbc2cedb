"""Per-video sampling parameters on the device: mmvid_logits_truncate_rows (csrc/sample.hip) on guarded, padded and poisoned buffers
against the scalar entry launched with each row's own values -- every comparison an equality; the rule itself stays pinned to fp64
through the scalar kernel (tests/test_truncate_gpu.py) -- and the two samplers with the per-video keywords: a uniform vector against
the scalar call, a mixed batch restated from its trace and against the calls that give every video one video's values."""
import numpy as np
import pytest
import torch

import truncate_ref as T
from guarded import SENTINEL_BITS, Guarded, bits, call_abi, ptr_of, report_mismatch
from test_guidance_gpu import BEAMS, NB, STEPS, TS, build_model, composed
from test_host_logic import tiny_vae

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG_INF = float('-inf')
f32, i32 = torch.float32, torch.int32
R = 15  # rows: parameter groups of 1, 3, 5 and 15 rows straddle the kernel's 4-row blocks, and the last block is partial
VS = (1, 2, 63, 64, 65, 200, 256, 257, 1024, 1025, 2047, 2048)  # the three register-slot classes (4, 16, 32 slots) and their edges
GROUPS = (1, 3, 5, 15)  # rows_per_param


# --------------------------------------------------------------------------------------------------------------------- helpers
def palette(V):
    """(top_k, top_p, temperature) settings a row can have: off in the documented and in the undocumented ways (a k outside [1, V), a
    p >= 1), k = 1, k = V - 1, both filters, the nucleus alone."""
    return [(0, 1.0, 1.0), (1, 1.0, 0.7), (V - 1, 1.0, 2.0), (min(5, V), 0.9, 0.5), (0, 0.5, 1.3), (V, 2.0, 1.0), (-3, 0.75, 0.9), (V + 7, 1.0, 3.0)]


def inv_of(t):
    """1 / temperature as the host rounds it in fp32: what the Python layer stores, and what the C entries compute from logit_div."""
    return float(np.float32(1.0) / np.float32(t))


def case(V, guided):
    """Device operands of a case: lc (every seventh column -inf, as the samplers' excluded classes), lu and the scales when guided, E."""
    gen = torch.Generator().manual_seed(8000 + 2 * V + guided)
    lc = 3 * torch.randn(R, V, generator=gen)
    lc[:, 6::7] = NEG_INF
    lu = 3 * torch.randn(R, V, generator=gen) if guided else None
    scale = torch.tensor([0.0, 3.0, -1.0, 0.5, 1.5]) if guided else None  # rows_per_scale = 3: not the parameter groups
    E = torch.empty(R, V).exponential_(generator=gen)
    return lc, lu, scale, E


def run_rows(lc, *, k=0, p=1.0, div=1.0, rows_k=None, rows_p=None, rows_inv=None, rpp=1, divide=0, lu=None, scale=None, rps=3, pad=24,
             pad_out=8, in_place=False):
    """One call of the new entry on guarded buffers (ld = V + pad > V; in_place: out is logits) -> (out, kept) on the host."""
    n, V = lc.shape
    gl = Guarded(base=lc, ld=V + pad) if in_place else Guarded(lc, role='in', ld=V + pad)
    glu = None if lu is None else Guarded(lu, role='in', ld=V + pad)
    gs = None if scale is None else Guarded(scale, role='in')
    arrays = [None if a is None else Guarded(torch.as_tensor(a, dtype=dt), role='in') for a, dt in ((rows_k, i32), (rows_p, f32), (rows_inv, f32))]
    gout = gl if in_place else Guarded(role='out', shape=(n, V), dtype=f32, ld=V + pad_out)
    gk = Guarded(role='out', shape=(n, ), dtype=i32)
    call_abi('mmvid_logits_truncate_rows', gl.ptr, ptr_of(glu), V + pad, ptr_of(gs), rps, div, k, p, *(ptr_of(a) for a in arrays), rpp, divide,
             n, V, gout.ptr, gout.ld, gk.ptr)
    for gb in (glu, gs, *arrays) + (() if in_place else (gl, )):
        if gb is not None:
            gb.check('logits_truncate_rows: an input')
    return gout.check('logits_truncate_rows out'), gk.check('logits_truncate_rows kept')


def scalar(lc, lu, scale, k, p, temp):
    """The scalar entry (ops.logits_truncate on dense device tensors) with one setting for every row -> (out, kept) on the host."""
    from mmvid_amd import ops
    guide = {} if lu is None else dict(logits_u=lu.to(DEV), scale=scale.to(DEV), rows_per_scale=3)
    out, kept = ops.logits_truncate(lc.to(DEV), max(k, 0), p, logit_div=temp, want_kept=True, **guide)
    return out.cpu(), kept.cpu()


def same(got, want, what):
    report_mismatch(got, want, what)
    assert torch.equal(bits(got), bits(want)), f'{what}: a value changed its bits (a signed zero)'


# ----------------------------------------------------------- 1, 2. no arrays and uniform arrays: the scalar entry, byte for byte
@pytest.mark.parametrize('V', VS)
def test_null_and_uniform_arrays_are_the_scalar_entry(V):
    for guided in (False, True):
        lc, lu, scale, _ = case(V, guided)
        for k, p, temp in ((min(3, V), 1.0, 1.0), (0, 0.8, 0.7), (V - 1, 0.95, 2.0)):
            want, want_kept = scalar(lc, lu, scale, k, p, temp)
            for rpp in GROUPS:
                n = R // rpp
                for in_place in (False, True):
                    kw = dict(lu=lu, scale=scale, rpp=rpp, in_place=in_place)
                    out, kept = run_rows(lc, k=k, p=p, div=temp, **kw)
                    same(out, want, f'V={V} no arrays k={k} p={p} T={temp} rpp={rpp} in_place={in_place} guided={guided}')
                    assert torch.equal(kept, want_kept)
                    out, kept = run_rows(lc, rows_k=[k] * n, rows_p=[p] * n, rows_inv=[inv_of(temp)] * n, **kw)
                    same(out, want, f'V={V} uniform arrays k={k} p={p} T={temp} rpp={rpp} in_place={in_place} guided={guided}')
                    assert torch.equal(kept, want_kept)


# ---------------------------------------- 3. mixed arrays: every row is the scalar entry launched with that row's values; 4. divide_out
def mixed(V, rpp, shift):
    """The setting of every parameter group (a walk through the palette) -> (settings per group, palette index per row)."""
    pal = palette(V)
    idx = [(3 * g + shift) % len(pal) for g in range(R // rpp)]
    return [pal[i] for i in idx], torch.tensor(idx).repeat_interleave(rpp)


@pytest.mark.parametrize('V', VS)
def test_mixed_rows_equal_the_scalar_entry_row_by_row(V):
    from mmvid_amd import ops
    pal = palette(V)
    for guided in (False, True):
        lc, lu, scale, E = case(V, guided)
        g = lc if not guided else composed(lc.to(DEV), lu.to(DEV), scale.to(DEV).repeat_interleave(3)).cpu()
        refs = [scalar(lc, lu, scale, *s) for s in pal]  # one scalar launch per setting, shared by the cases below and left unchanged
        k_fixed = min(7, V)
        refs_k = [scalar(lc, lu, scale, k_fixed, s[1], s[2]) for s in pal]
        Ed = E.to(DEV)
        for rpp in GROUPS:
            settings, row_idx = mixed(V, rpp, rpp)
            ks, ps, invs = [s[0] for s in settings], [s[1] for s in settings], [inv_of(s[2]) for s in settings]
            want = torch.stack([refs[i][0][r] for r, i in enumerate(row_idx.tolist())])
            want_kept = torch.stack([refs[i][1][r] for r, i in enumerate(row_idx.tolist())])
            for in_place in (False, True):
                what = f'V={V} rpp={rpp} in_place={in_place} guided={guided}'
                out, kept = run_rows(lc, rows_k=ks, rows_p=ps, rows_inv=invs, rpp=rpp, lu=lu, scale=scale, in_place=in_place)
                same(out, want, 'mixed ' + what)
                assert torch.equal(kept, want_kept), what
                # a scalar of one quantity beside the array of the other
                out, kept = run_rows(lc, k=k_fixed, rows_p=ps, rows_inv=invs, rpp=rpp, lu=lu, scale=scale, in_place=in_place)
                same(out, torch.stack([refs_k[i][0][r] for r, i in enumerate(row_idx.tolist())]), 'scalar k, p per row ' + what)
                assert torch.equal(kept, torch.stack([refs_k[i][1][r] for r, i in enumerate(row_idx.tolist())])), what
                # 4. divide_out: the kept classes are g * inv_div of their row, one rounded product
                inv_rows = torch.tensor(invs, dtype=f32).repeat_interleave(rpp).view(R, 1)
                div_out, div_kept = run_rows(lc, rows_k=ks, rows_p=ps, rows_inv=invs, rpp=rpp, divide=1, lu=lu, scale=scale, in_place=in_place)
                product = g * inv_rows
                same(div_out, torch.where(torch.isfinite(want), product, want), 'divide_out ' + what)
                assert torch.equal(div_kept, torch.isfinite(div_out).sum(1).to(i32)), what
            # the race on the divided value with logit_div = 1 is the race on the undivided one with the row's temperature
            div_dev = div_out.to(DEV)
            for want_y in (True, False):  # the wave-per-row race (with y) and the token-only, block-per-row one
                tok, y = ops.sample_race(div_dev, Ed, logit_div=1.0, want_y=want_y)
                for gi, s in enumerate(settings):
                    rows = slice(gi * rpp, (gi + 1) * rpp)
                    tok_s, y_s = ops.sample_race(want[rows].to(DEV), Ed[rows].contiguous(), logit_div=s[2], want_y=want_y)
                    assert torch.equal(tok[rows], tok_s), f'race token, want_y={want_y} group {gi} ' + what
                    assert not want_y or torch.equal(bits(y[rows]), bits(y_s)), f'race y, group {gi} ' + what


@pytest.mark.parametrize('V', (65, 1025, 2048))
def test_temperature_alone_reaches_the_guided_races_through_the_divided_value(V):
    """No filter on: the rows are divided and nothing else.  The plain race on the materialised, divided guided value with logit_div = 1
    draws what both guided races draw from (lc, lu, w) with the row's temperature."""
    from mmvid_amd import ops
    lc, lu, scale, E = case(V, True)
    lcd, lud, sd, Ed = lc.to(DEV), lu.to(DEV), scale.to(DEV), E.to(DEV)
    temps = [0.7, 2.0, 1.0, 0.5, 1.3]
    out = ops.logits_truncate_rows(lcd, rows_inv_div=torch.tensor([inv_of(t) for t in temps], device=DEV), rows_per_param=3, divide_out=True,
                                   logits_u=lud, scale=sd, rows_per_scale=3)
    g = composed(lcd, lud, sd.repeat_interleave(3))
    same(out.cpu(), (g * torch.tensor([inv_of(t) for t in temps], device=DEV).repeat_interleave(3).view(R, 1)).cpu(), f'V={V}: divided copy-through')
    tok, y = ops.sample_race(out, Ed, logit_div=1.0)
    tok_at = ops.sample_race(out, Ed, logit_div=1.0, want_y=False)[0]
    for gi, t in enumerate(temps):
        rows = slice(3 * gi, 3 * gi + 3)
        tg, yg = ops.sample_race_guided(lcd[rows], lud[rows], sd[gi:gi + 1], 3, Ed[rows].contiguous(), logit_div=t)
        assert torch.equal(tok[rows], tg) and torch.equal(bits(y[rows]), bits(yg)), f'V={V} group {gi}: sample_race_guided'
        assert torch.equal(tok_at[rows], ops.sample_race_guided_at(lcd[rows], lud[rows], sd[gi:gi + 1], 3, Ed[rows].contiguous(), logit_div=t)), \
            f'V={V} group {gi}: sample_race_guided_at'


def test_tie_rows_with_a_k_per_row():
    rows = T.tie_rows()
    g = torch.from_numpy(np.stack([r[1] for r in rows]))
    ks = [r[2] for r in rows]
    out, kept = run_rows(g, rows_k=ks, rpp=1, rps=1)
    for i, (name, _, k, want) in enumerate(rows):
        assert torch.isfinite(out[i]).nonzero().view(-1).tolist() == want, name
        o, kk = scalar(g[i:i + 1], None, None, k, 1.0, 1.0)
        same(out[i:i + 1], o, name)
        assert int(kept[i]) == int(kk[0]) == len(want)


# ------------------------------------------------------------------- 5. a bad device value stays in its row; 6. the refusals
@pytest.mark.parametrize('V', (64, 1025))
def test_a_bad_device_value_spoils_its_own_row_only(V):
    lc, lu, scale, _ = case(V, True)
    nan, inf = float('nan'), float('inf')
    ks = [3] * R
    good_p, good_inv = [0.9] * R, [inv_of(0.7)] * R
    want, want_kept = run_rows(lc, rows_k=ks, rows_p=good_p, rows_inv=good_inv, lu=lu, scale=scale)
    for in_place in (False, True):
        bad_p, bad_inv = list(good_p), list(good_inv)
        bad_p[2], bad_p[5], bad_p[7] = 0.0, -1.0, nan
        bad_inv[9], bad_inv[11], bad_inv[12], bad_inv[14] = nan, inf, -1.0, 0.0
        bad_rows = [2, 5, 7, 9, 11, 12, 14]
        for divide in (0, 1):
            ref = run_rows(lc, rows_k=ks, rows_p=good_p, rows_inv=good_inv, divide=divide, lu=lu, scale=scale)
            out, kept = run_rows(lc, rows_k=ks, rows_p=bad_p, rows_inv=bad_inv, divide=divide, lu=lu, scale=scale, in_place=in_place)  # (guards checked inside)
            good = torch.tensor([r not in bad_rows for r in range(R)])
            same(out[good], ref[0][good], f'V={V} divide={divide} in_place={in_place}: rows beside the bad ones')
            assert torch.equal(kept[good], ref[1][good])
    assert torch.equal(want_kept, torch.isfinite(want).sum(1).to(i32))


def test_every_refusal_returns_nonzero_and_writes_nothing():
    from mmvid_amd import _lib
    n, V = 6, 64
    g = 3 * torch.randn(n, V, generator=torch.Generator().manual_seed(8100))
    gl, glu, gs = Guarded(g, role='in'), Guarded(g + 1, role='in'), Guarded(torch.ones(2), role='in')
    gk_in, gp_in, gi_in = (Guarded(torch.tensor([4, 0, 2], dtype=i32), role='in'), Guarded(torch.tensor([0.9, 1.0, 0.5]), role='in'),
                           Guarded(torch.tensor([1.0, 2.0, 0.5]), role='in'))
    gout = Guarded(role='out', shape=(n, V), dtype=f32, partial=True)
    gk = Guarded(role='out', shape=(n, ), dtype=i32, partial=True)
    nan = float('nan')
    off = lambda gb, nbytes: type(gb.ptr)(gb.ptr.value + nbytes)  # noqa: E731
    ok = dict(logits=gl.ptr, logits_u=None, ld=V, scale=None, rps=1, div=1.0, k=4, p=0.9, rk=gk_in.ptr, rp=gp_in.ptr, ri=gi_in.ptr, rpp=2,
              divide=0, R=n, V=V, out=gout.ptr, ld_out=V)
    bad = [dict(V=0), dict(V=2049, ld=2049, ld_out=2049), dict(div=0.0), dict(div=-1.0), dict(p=0.0), dict(p=-0.5), dict(p=nan),  # the scalar entry's
           dict(logits_u=glu.ptr, scale=gs.ptr, rps=0), dict(logits_u=glu.ptr, scale=gs.ptr, rps=4), dict(logits_u=glu.ptr), dict(scale=gs.ptr),
           dict(logits=None), dict(out=None), dict(ld=V - 1), dict(ld_out=V - 1), dict(R=-1),
           dict(rpp=0), dict(rpp=-2), dict(rpp=4),  # 6 rows are no multiple of 4
           dict(rk=off(gk_in, 2)), dict(rp=off(gp_in, 1)), dict(ri=off(gi_in, 3)), dict(divide=2), dict(divide=-1)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(_lib.MMVIDError, match=r'rc=[1-9-].*logits_truncate_rows: \S') as err:
            call_abi('mmvid_logits_truncate_rows', a['logits'], a['logits_u'], a['ld'], a['scale'], a['rps'], a['div'], a['k'], a['p'], a['rk'],
                     a['rp'], a['ri'], a['rpp'], a['divide'], a['R'], a['V'], a['out'], a['ld_out'], gk.ptr)
        assert 'launch failed' not in str(err.value), change
        for gb in (gl, glu, gs, gk_in, gp_in, gi_in, gout, gk):
            gb.check(f'refused call {change}')
        assert bool((bits(gout.window()) == SENTINEL_BITS[f32]).all()) and bool((bits(gk.window()) == SENTINEL_BITS[i32]).all()), change
    a = dict(ok, R=0)  # R == 0 is no refusal: status 0, nothing stored
    call_abi('mmvid_logits_truncate_rows', a['logits'], None, V, None, 1, 1.0, 4, 0.9, a['rk'], a['rp'], a['ri'], 2, 0, 0, V, a['out'], V, gk.ptr)
    assert bool((bits(gout.window()) == SENTINEL_BITS[f32]).all())
    call_abi('mmvid_logits_truncate_rows', gl.ptr, glu.ptr, V, gs.ptr, 3, 1.0, 4, 0.9, a['rk'], a['rp'], a['ri'], 2, 1, n, V, gout.ptr, V, gk.ptr)
    assert bool(torch.isfinite(gout.check('accepted call')).any(dim=1).all())


def test_the_operator_checks_its_arrays():
    from mmvid_amd import _lib, ops
    g = torch.randn(6, 64, device=DEV)
    k = torch.tensor([1, 2, 3], dtype=i32, device=DEV)
    assert ops.logits_truncate_rows(g[:0], rows_per_param=1).shape == (0, 64)
    with pytest.raises(_lib.MMVIDError, match='no CPU path'):
        ops.logits_truncate_rows(g, rows_k=k.cpu(), rows_per_param=2)
    with pytest.raises(TypeError, match='rows_k'):
        ops.logits_truncate_rows(g, rows_k=k.long(), rows_per_param=2)
    with pytest.raises(TypeError, match='rows_p'):
        ops.logits_truncate_rows(g, rows_p=k, rows_per_param=2)
    with pytest.raises(ValueError, match='rows_inv_div'):
        ops.logits_truncate_rows(g, rows_inv_div=torch.ones(2, device=DEV), rows_per_param=2)
    with pytest.raises(ValueError, match='no multiple'):
        ops.logits_truncate_rows(g, rows_k=k, rows_per_param=4)
    with pytest.raises(ValueError, match='come together'):
        ops.logits_truncate_rows(g, rows_k=k, rows_per_param=2, logits_u=g)
    buf = g.clone()
    got = ops.logits_truncate_rows(buf, rows_k=k, rows_per_param=2, out=buf)
    assert got is buf and torch.equal((torch.isfinite(buf).sum(1)).cpu(), torch.tensor([1, 1, 2, 2, 3, 3]))


# ------------------------------------------------------------------------------------------------------ 7. the BERT sampler
SEEDS = [1001, 2**62 + 5, 77]
VK, VP = [4, 0, 1], [1.0, 0.75, None]  # video 0: top-k alone; video 1: the nucleus alone; video 2: greedy


@pytest.fixture(scope='module')
def model():
    return build_model()


@pytest.fixture(scope='module')
def mp(golden):
    return dict(golden('mask_predict').meta['mp_config'], B=BEAMS)  # two candidates per video: rows_per_param = 2 * TS after step 0


@pytest.fixture(scope='module')
def controls(model):
    gen = torch.Generator().manual_seed(71)
    text = torch.randint(1, 49408, (NB, 16), generator=gen)
    text[0, 9:] = 0
    text = text.to(DEV)
    with torch.no_grad():
        control = model(text, return_loss=False)
        uncond = model(torch.zeros_like(text), return_loss=False)
    uncond[:, 1:17] = torch.randn(uncond[:, 1:17].shape, generator=gen).to(DEV) * 4 * float(control.std())
    return control, uncond.contiguous()


def bert_run(model, mp, controls, rows=(0, 1, 2), guided=None, **kw):
    """mask_predict on the videos `rows` with their seeds (guided: the scale of every video, or None)."""
    idx = torch.tensor(rows, device=DEV)
    if guided is not None:
        kw.update(uncond_emb=controls[1].index_select(0, idx), guidance_scale=torch.tensor([guided[i] for i in rows], device=DEV))
    return model.mask_predict(controls[0].index_select(0, idx), dynamic=False, steps=STEPS, mp_config=mp, seeds=[SEEDS[i] for i in rows], **kw)[0]


def restate_bert(trace, cfg, ks, ps, scales=None):
    """Every step of a traced per-video run from its own records: each video's rows are the scalar ops.logits_truncate of those rows with
    the video's values (bit for bit, kept included), and the step's tokens and confidences are the plain race on the recorded E."""
    from mmvid_amd import ops, sampling
    seen = 0
    for rec in trace:
        t = rec['t']
        nb = 1 if t == 0 else BEAMS
        n = nb * TS
        if 'logits_t' not in rec:
            continue
        seen += 1
        assert rec['rows_per_param'] == n
        assert (rec['rows_k'] is None) == (ks is None) and (rec['rows_p'] is None) == (ps is None)
        for i in range(NB):
            k = None if ks is None else ks[t][i]
            p = None if ps is None else ps[t][i]
            assert k is None or int(rec['rows_k'][i]) == k
            assert p is None or float(rec['rows_p'][i]) == float(np.float32(p))
            rows = slice(i * n, (i + 1) * n)
            guide = {} if scales is None else dict(logits_u=rec['logits_u'][rows], scale=torch.tensor([scales[i]], device=DEV), rows_per_scale=n)
            want, want_kept = ops.logits_truncate(rec['logits'][rows], k or None, p, want_kept=True, **guide)
            same(rec['logits_t'][rows].cpu(), want.cpu(), f'step {t} video {i}: the scalar truncation with the video\'s values')
            assert torch.equal(rec['kept'][rows], want_kept)
        temp = sampling.schedule(cfg, TS)[1][t]
        assert temp == 0.0  # (the cold schedule below: no noise tensor to restate)
        tok, y = ops.sample_race(rec['logits_t'], rec['E_tok'], None, 0.0)
        got_tok = (rec['I_tok'] if t == 0 else rec['Inew']).reshape(-1)
        got_y = (rec['Y'] if t == 0 else rec['Ynew']).reshape(-1)
        assert torch.equal(got_tok, tok) and torch.equal(bits(got_y), bits(y)), f'step {t}: not the plain race on the truncated logits'
    return seen


@pytest.fixture(scope='module')
def cold(mp):
    """The schedule without Gumbel noise: a step is restated from its logits and its race variates alone."""
    return dict(mp, N1_t=0.0, N2_t=0.0, N3_t=0.0, N4_t=0.0)


def test_bert_uniform_vectors_are_the_scalar_call(model, mp, controls):
    want = bert_run(model, mp, controls, top_k=5, top_p=0.9)
    got = bert_run(model, mp, controls, video_top_k=[5, 5, 5], video_top_p=torch.full((NB, ), 0.9))
    report_mismatch(got.cpu(), want.cpu(), 'uniform vectors against the scalars')
    got = bert_run(model, mp, controls, top_k=5, video_top_p=[[0.9] * NB] * STEPS)  # a scalar beside a [Tmax, b] table
    report_mismatch(got.cpu(), want.cpu(), 'scalar top_k with a video_top_p table against the scalars')
    guided = [2.0, 0.5, 1.0]
    want = bert_run(model, mp, controls, guided=guided, top_k=5)
    report_mismatch(bert_run(model, mp, controls, guided=guided, video_top_k=torch.tensor([5, 5, 5])).cpu(), want.cpu(), 'guided, uniform')
    assert not torch.equal(want, bert_run(model, mp, controls, guided=guided))  # (the filter did something)


@pytest.mark.parametrize('guided', [None, [2.0, 0.5, 1.0]], ids=['unguided', 'per-video guidance_scale'])
def test_bert_mixed_videos_restated_and_against_the_uniform_calls(model, cold, controls, guided):
    trace = []
    mixed = bert_run(model, cold, controls, guided=guided, video_top_k=VK, video_top_p=VP, _trace=trace)
    assert len(trace) == STEPS
    ks, ps = [[k or 0 for k in VK]] * STEPS, [[1.0 if p is None else p for p in VP]] * STEPS
    assert restate_bert(trace, cold, ks, ps, guided) == STEPS
    for i in range(NB):  # video i of the mixed batch is video i of the call in which every video has video i's values ...
        uniform = bert_run(model, cold, controls, guided=guided, top_k=VK[i] or None, top_p=VP[i])
        report_mismatch(mixed[i].cpu(), uniform[i].cpu(), f'video {i} of the mixed batch against the uniform call')
        alone = bert_run(model, cold, controls, rows=(i, ), guided=guided, video_top_k=[VK[i]], video_top_p=[VP[i]])  # ... and the video alone
        report_mismatch(mixed[i:i + 1].cpu(), alone.cpu(), f'video {i} of the mixed batch against the video alone')
    moved = bert_run(model, cold, controls, rows=(2, 0, 1), guided=guided, video_top_k=[VK[i] for i in (2, 0, 1)], video_top_p=[VP[i] for i in (2, 0, 1)])
    report_mismatch(moved.cpu(), mixed[[2, 0, 1]].cpu(), 'the batch in another order')


def launches(monkeypatch, fn):
    """fn() -> (its result, the names of the C entries it called, in order)."""
    from mmvid_amd import _lib, ops
    seen, real = [], _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)
    with monkeypatch.context() as mpatch:
        mpatch.setattr(_lib, 'call', recorder)
        mpatch.setattr(ops, 'call', recorder)  # (ops binds the function by name at import)
        out = fn()
    return out, seen


def test_bert_a_step_with_every_filter_off_is_the_unfiltered_step(model, cold, controls, monkeypatch):
    table_k = [[4, 0, 1], [3, 3, 0], [0, 0, 0], [0, 2, 0]]  # step 2: nothing on
    trace = []
    plain, log_plain = launches(monkeypatch, lambda: bert_run(model, cold, controls))
    tabled, log = launches(monkeypatch, lambda: bert_run(model, cold, controls, video_top_k=table_k))
    bert_run(model, cold, controls, video_top_k=table_k, _trace=trace)
    assert restate_bert(trace, cold, table_k, None) == 3 and 'logits_t' not in trace[2]
    assert log.count('mmvid_logits_truncate_rows') == 3 and 'mmvid_logits_truncate' not in log and 'mmvid_logits_truncate_rows' not in log_plain
    assert [n for n in log if n != 'mmvid_logits_truncate_rows'] == log_plain  # one launch more at the three steps, nothing else

    def steps(names):  # the launch list cut at the keep selection that opens every step after step 0
        cuts = [i for i, n in enumerate(names) if n.startswith('mmvid_mp_select_keep')] + [len(names)]
        return [names[:cuts[0]]] + [names[a:b] for a, b in zip(cuts, cuts[1:])]
    assert len(steps(log)) == STEPS and steps(log)[2] == steps(log_plain)[2], 'the step with every filter off is not the unfiltered step'
    # calls without the new keywords record what they recorded: the scalar call has the scalar entry where the rows entry stands
    _, log_scalar = launches(monkeypatch, lambda: bert_run(model, cold, controls, top_k=4))
    assert log_scalar.count('mmvid_logits_truncate') == STEPS and 'mmvid_logits_truncate_rows' not in log_scalar
    assert [n for n in log_scalar if n != 'mmvid_logits_truncate'] == log_plain
    assert not torch.equal(tabled, plain)


# ----------------------------------------------------------------------------------------------------- 8. the ART-V sampler
ART_SEEDS = [901, 2**62 + 9, 903, 904]
AK, AP, AT = [3, 0, 1, 0], [1.0, 0.6, None, 1.0], [0.7, 1.0, 2.0, 1.3]  # video 3: no filter, its own temperature


@pytest.fixture(scope='module')
def artv():
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(73)
    m = DALLE(dim=768, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(74)
    text = torch.randint(1, 49408, (4, 16), generator=gen).to(DEV)  # batch 4: the separate launches
    vis = torch.randint(0, 256, (4, 16), generator=gen).to(DEV)
    known = torch.randint(0, 256, (4, m.target_seq_len), generator=gen).to(DEV)
    return m, text, vis, known


def art_run(artv, videos=(0, 1, 2, 3), **kw):
    m, text, vis, _ = artv
    idx = torch.tensor(videos, device=DEV)
    return m.sample_tokens(text.index_select(0, idx), visual=vis.index_select(0, idx), seeds=[ART_SEEDS[v] for v in videos], **kw)[1]


def restate_artv(trace, ks, ps, temps, scales=None):
    """Every token of a traced run: each row's logits_t is the scalar truncation of that row with the row's values, divided by the row's
    temperature (one rounded product) where temperatures are given, and the token is the plain race on the recorded E."""
    from mmvid_amd import ops
    for j, rec in enumerate(trace):
        B = rec['E'].shape[0]
        lc = rec['logits'][:B]
        for i in range(B):
            guide = {} if scales is None else dict(logits_u=rec['logits'][B + i:B + i + 1], scale=torch.tensor([scales[i]], device=DEV), rows_per_scale=1)
            t = 1.0 if temps is None else temps[i]
            want, kept = ops.logits_truncate(lc[i:i + 1], (ks[i] or None) if ks else None, ps[i] if ps else None, logit_div=t, want_kept=True, **guide)
            if temps is not None:
                want = want * inv_of(t)
            same(rec['logits_t'][i:i + 1].cpu(), want.cpu(), f'token {j} video {i}')
            assert int(rec['kept'][i]) == int(kept[0])
            tok = ops.sample_race(want, rec['E'][i:i + 1].contiguous(), logit_div=1.0, want_y=False)[0]
            assert int(tok[0]) == int(rec['tok'][i]), f'token {j} video {i}: not the plain race on the restated value'


def test_artv_uniform_vectors_are_the_scalar_call(artv):
    want = art_run(artv, top_k=5, top_p=0.9, temperature=0.8)
    got = art_run(artv, video_top_k=[5] * 4, video_top_p=[0.9] * 4, video_temperature=torch.full((4, ), 0.8))
    report_mismatch(got.cpu(), want.cpu(), 'uniform vectors against the scalars')
    got = art_run(artv, top_k=5, video_top_p=[0.9] * 4, temperature=0.8)  # scalars of the other quantities compose
    report_mismatch(got.cpu(), want.cpu(), 'scalar top_k and temperature with video_top_p')
    assert not torch.equal(want, art_run(artv, temperature=0.8))


@pytest.mark.parametrize('guided', [None, [2.0, 0.5, 1.0, 1.5]], ids=['unguided', 'per-video guidance_scale'])
def test_artv_mixed_videos_captured_eager_restated_and_against_the_uniform_calls(artv, guided, monkeypatch):
    kw = {} if guided is None else dict(guidance_scale=torch.tensor(guided, device=DEV))
    replays = []
    inner = torch.cuda.CUDAGraph.replay
    with monkeypatch.context() as mpatch:
        mpatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), inner(self))[1])
        mixed = art_run(artv, video_top_k=AK, video_top_p=AP, video_temperature=AT, **kw)  # production: the captured [draw -> advance] step
    m = artv[0]
    assert len(replays) >= m.target_seq_len - 4, 'the per-video call did not run its captured step'
    trace = []
    eager = art_run(artv, video_top_k=AK, video_top_p=AP, video_temperature=AT, _trace=trace, **kw)
    report_mismatch(eager.cpu(), mixed.cpu(), 'the eager loop against the captured step')
    assert len(trace) == m.target_seq_len
    restate_artv(trace, AK, AP, AT, guided)
    for i in range(4):  # the same B: video i against the call in which all four videos have video i's values
        uniform = art_run(artv, top_k=AK[i] or None, top_p=AP[i], temperature=AT[i], **kw)
        report_mismatch(mixed[i].cpu(), uniform[i].cpu(), f'video {i} of the mixed batch against the uniform call')


def test_artv_temperature_alone_costs_one_launch_per_token(artv, monkeypatch):
    m = artv[0]
    mixed, log = launches(monkeypatch, lambda: art_run(artv, video_temperature=AT, _trace=[]))  # (a trace: the eager loop, every launch visible)
    _, log_scalar = launches(monkeypatch, lambda: art_run(artv, temperature=0.7, _trace=[]))
    assert log.count('mmvid_logits_truncate_rows') == m.target_seq_len and 'mmvid_logits_truncate' not in log
    assert [n for n in log if n != 'mmvid_logits_truncate_rows'] == log_scalar  # one launch per token more, otherwise the scalar call's list
    for i in range(4):
        uniform = art_run(artv, temperature=AT[i])
        report_mismatch(mixed[i].cpu(), uniform[i].cpu(), f'video {i} against the call at temperature {AT[i]}')
    report_mismatch(art_run(artv, video_temperature=AT).cpu(), mixed.cpu(), 'the captured step against the eager loop')


def test_artv_batch_2_with_a_keyword_takes_the_separate_launches(artv, monkeypatch):
    from mmvid_amd import _lib
    launched = []
    inner = _lib.DecodeToken
    with monkeypatch.context() as mpatch:
        mpatch.setattr(_lib, 'DecodeToken', lambda *a, **k: (launched.append(1), inner(*a, **k))[1])
        two = art_run(artv, videos=(1, 3), video_top_k=[0, 0])  # nothing on, and still the per-row launch
        assert not launched, 'a call with a per-video keyword set up the one-launch-per-token path'
        mpatch.setenv('MMVID_DECODE_TOKEN', '0')  # the plain call through the separate launches
        plain = art_run(artv, videos=(1, 3))
    report_mismatch(two.cpu(), plain.cpu(), 'batch 2, every filter off: the tokens of the call without the keyword')
    trace = []
    art_run(artv, videos=(1, 3), video_top_k=[0, 0], _trace=trace)
    assert all('rows_k' in rec for rec in trace)


def test_complete_artv_with_two_given_patterns(artv):
    from mmvid_amd import completion
    m, text, vis, known = artv
    given = torch.tensor([[1, 0], [0, 0], [1, 0], [0, 0]], dtype=torch.bool)  # rows 0, 2 know frame 0; rows 1, 3 know nothing
    kw = dict(visual=vis, paste=False, seeds=ART_SEEDS)
    _, mixed = completion.complete_artv(m, text, known, given, video_top_k=AK, video_top_p=AP, video_temperature=AT, **kw)
    half = m.target_seq_len // 2
    assert torch.equal(mixed[[0, 2], :half], known[[0, 2], :half])
    for rows in ([0, 2], [1, 3]):  # every group of rows takes the parameters of its rows: the group alone, with its own entries
        idx = torch.tensor(rows, device=DEV)
        pick = lambda a: [a[r] for r in rows]  # noqa: E731
        _, alone = completion.complete_artv(m, text[idx], known[idx], given[rows], visual=vis[idx], paste=False, seeds=pick(ART_SEEDS),
                                            video_top_k=pick(AK), video_top_p=pick(AP), video_temperature=pick(AT))
        report_mismatch(mixed[idx].cpu(), alone.cpu(), f'rows {rows} of the mixed call against the group alone')
    for i in range(4):
        _, uniform = completion.complete_artv(m, text, known, given, top_k=AK[i] or None, top_p=AP[i], temperature=AT[i], **kw)
        report_mismatch(mixed[i].cpu(), uniform[i].cpu(), f'video {i} against the uniform call')


def test_artv_sampling_probs_is_the_softmax_of_the_restated_value(artv):
    from mmvid_amd import ops
    m = artv[0]
    gen = torch.Generator().manual_seed(76)
    lg, lu = (3 * torch.randn(4, 256, generator=gen)).to(DEV), (3 * torch.randn(4, 256, generator=gen)).to(DEV)
    scales = [2.0, 0.5, 1.0, 1.5]
    for guide in ({}, dict(logits_u=lu, guidance_scale=torch.tensor(scales, device=DEV))):
        probs = m.sampling_probs(lg, filter_thres=0.0, video_top_k=AK, video_top_p=AP, video_temperature=AT, **guide)
        value = []
        for i in range(4):
            g = {} if not guide else dict(logits_u=lu[i:i + 1], scale=torch.tensor([scales[i]], device=DEV), rows_per_scale=1)
            value.append(ops.logits_truncate(lg[i:i + 1], AK[i] or None, AP[i], logit_div=AT[i], **g) * inv_of(AT[i]))
        same(probs.cpu(), torch.softmax(torch.cat(value), dim=-1).cpu(), f'guided={bool(guide)}')
        assert bool(((probs > 0).sum(1)[[0, 2]] == torch.tensor([3, 1], device=DEV)).all())
