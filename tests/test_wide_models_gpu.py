"""BERT and ART-V at dim 1024 (a ViT-L/14 visual tower: 16 heads, two layers here) end to end on the device: the ART-V sampler over the
key/value cache against the reference's loop, its captured step, a guided and a prediction call restated from their records, one ART-V
training step against the reference's; a BERT training step against the reference's (tests/golden/wide_models.npz,
tools/make_golden.py::case_wide_models) and a mask-predict run against the oracle's decisions.  The helpers are those of the width-768 tests."""
import pytest
import torch

from guarded import report_mismatch
from test_artv_completion_gpu import B, N, T, TT, V, known_columns, restate, row, run, stacked_race
from test_host_logic import tiny_vae
from test_models_gpu import DEV, _with_tokens, close, load_synth
from test_truncate_gpu import stored_race

pytestmark = pytest.mark.gpu
D = 1024


# ----------------------------------------------------------------------------------------------------------------------------- ART-V
@pytest.fixture(scope='module')
def artv():
    """The tiny ART-V model of tests/test_artv_completion_gpu.py at dim 1024: 2 layers, 16 text positions, one visual, 4 targets of 16
    tokens, 256 codes, seeded random weights."""
    from mmvid_amd.dalle_artv import DALLE
    torch.manual_seed(193)
    m = DALLE(dim=D, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=TT, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=T, transformer_layers=2, transformer_width=D).to(DEV).eval()
    assert (m.transformer.width, m.transformer.heads, m.to_logits[1].weight.shape[1]) == (D, 16, D)
    gen = torch.Generator().manual_seed(194)
    text = torch.randint(1, 49408, (B, TT), generator=gen)
    text[1, 11:] = 0
    vis = torch.randint(0, V, (B, N), generator=gen)
    known = torch.randint(0, V, (B, T * N), generator=gen)
    return m, text.to(DEV), vis.to(DEV), known.to(DEV)


def test_artv_cached_sampler_equals_the_reference_loop(artv):
    """generate_images over the key/value cache (the five-launch decode step at width 1024) against use_cache=False (the whole prefix
    through the training forward per token), token for token under the same `_race` variates."""
    m, text, vis, _ = artv
    race = stacked_race(B, seed=195)
    cached = run(m, text, vis, _race=race)
    recomputed = run(m, text, vis, _race=race, use_cache=False)
    assert cached.shape == (B, T * N) and 0 <= int(cached.min()) and int(cached.max()) < V
    report_mismatch(cached.cpu(), recomputed.cpu(), 'dim 1024: tokens over the key/value cache against the reference\'s loop')


def test_artv_captured_step_equals_the_eager_one(artv, monkeypatch):
    m, text, vis, _ = artv
    replays = []
    inner = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', lambda self: (replays.append(1), inner(self))[1])
    produced = run(m, text, vis, top_k=1)  # pre-drawn variates, [truncate -> draw -> embed -> advance] captured
    n_replays = len(replays)
    eager = run(m, text, vis, top_k=1, _race=stored_race())
    assert n_replays >= m.target_seq_len - 4 and len(replays) == n_replays, 'the call without _race did not run its captured step'
    report_mismatch(produced.cpu(), eager.cpu(), 'dim 1024, top_k = 1: the captured step against the eager one (both greedy)')


def test_artv_guided_call_is_its_records_restatement(artv):
    m, text, vis, _ = artv
    scale = torch.tensor([2.0, 0.0, -0.5], device=DEV)
    trace = []
    tokens = run(m, text, vis, _race=stacked_race(2 * B, seed=196), _trace=trace, guidance_scale=scale)
    assert trace[0]['logits'].shape == (2 * B, V)
    restate(m, torch.cat((text, torch.zeros_like(text))), torch.cat((vis, torch.full_like(vis, -1))), '0000', tokens, trace, scale=scale,
            what='dim 1024, guided at scales 2 / 0 / -0.5')


def test_artv_prediction_call_is_its_records_restatement(artv):
    m, text, vis, known = artv
    mask, trace = '1010', []
    tokens = run(m, text, vis, given=(row(mask), known), _race=stacked_race(B, seed=197), _trace=trace)
    cols = known_columns(mask)
    report_mismatch(tokens[:, cols].cpu(), known[:, cols].cpu(), 'the known columns of the result against the given tokens')
    restate(m, text, vis, mask, tokens, trace, what=f'dim 1024, mask {mask}')


def test_artv_training_step_vs_reference_at_dim_1024(golden):
    """DALLE.forward(return_loss=True) + backward at dim 1024 (the 49,952-way head [V, 1024] through LNLinearCrossEntropy, the assemble and
    positional-table kernels at width 1024) against the reference's step on the same weights and the reference's tokens, at the bars of
    tests/test_models_gpu.py::test_artv_logits_and_loss_vs_reference (loss 2e-2, gradients 5e-2)."""
    from conftest import synth_model_sd
    from mmvid_amd.dalle_artv import DALLE
    g = golden('wide_models')
    m = DALLE(dim=D, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
              num_visuals=1, num_targets=2, transformer_layers=2, transformer_width=D)
    sd = synth_model_sd(type('G', (), {'manifest': [(k, tuple(s_)) for k, s_ in g.json('manifest_artv')]})(), g.meta['artv_seed'])
    m.load_state_dict(sd)
    m.to(DEV).train()
    assert tuple(m.to_logits[1].weight.shape) == (m.total_tokens, D)
    loss, _, _ = m(g['artv_text'].to(DEV), visual=g['artv_visual_tok'].to(DEV), target=g['artv_target_tok'].to(DEV), return_loss=True)
    print('artv loss at dim 1024', loss.item(), 'ref', g['artv_loss'].item())
    assert abs(loss.item() - g['artv_loss'].item()) < 2e-2 * abs(g['artv_loss'].item())
    loss.backward()
    blk = m.transformer.transformer.resblocks
    close(m.to_logits[1].weight.grad[::997, ::13], g['artv_g_to_logits_w_s'], 5e-2, 'artv g to_logits')
    close(m.image_emb.weight.grad[::3, ::5], g['artv_g_image_emb_s'], 5e-2, 'artv g image_emb')
    close(blk[0].attn.in_proj_weight.grad[::61, ::29], g['artv_g_inw_s'], 5e-2, 'artv g in_proj')
    close(blk[1].mlp.c_proj.weight.grad[::61, ::29], g['artv_g_pjw_s'], 5e-2, 'artv g c_proj')
    tn = torch.sqrt(sum((p.grad.double()**2).sum() for p in m.parameters() if p.grad is not None)).item()
    assert abs(tn / g['artv_g_total_norm'].item() - 1) < 3e-2


# ------------------------------------------------------------------------------------------------------------------------------ BERT
def wide_bert(T_=2):
    from mmvid_amd.dalle_bert import BERT
    return BERT(dim=D, vae=tiny_vae(), cvae=None, num_text_tokens=49408, text_seq_len=16, which_transformer='openai_clip_visual',
                num_visuals=0, num_targets=T_, transformer_layers=2, transformer_width=D)


def test_bert_training_step_vs_reference_at_dim_1024(golden):
    """The three losses, the MSM logits and selected gradients of one training step with the reference's tokens, mask and warped frames
    injected, at the bars of tests/test_models_gpu.py::test_bert_training_forward_backward_vs_reference."""
    g = golden('wide_models')
    m = load_synth(wide_bert(), g, 17)
    m.train()
    text, frames = g['text'].to(DEV), g['frames'].to(DEV)
    with torch.no_grad():
        ctrl = _with_tokens(m, g, lambda: m(text, visual=None, return_loss=False))
    close(ctrl[:, ::2], g['control_emb'], 1e-6, 'control_emb')

    def step():
        return m(text, visual=None, target=frames, return_loss=True, rel=True, vid=True, rel_no_fully_masked=True,
                 _mask1=g['mask1'], _target_warp=g['warped_frames'])
    lm, lr, lv = _with_tokens(m, g, step)
    losses = torch.stack([lm, lr, lv]).detach().cpu()
    print('losses', losses.tolist(), 'ref', g['losses'].tolist())
    assert torch.allclose(losses, g['losses'], rtol=2e-2, atol=2e-2)
    close(m._last_logits_msm[:, ::2], g['logits_msm'], 3e-2, 'logits_msm')
    (7 * lm + 0.5 * lr + 0.5 * lv).backward()
    G = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    blk = 'transformer.transformer.resblocks.'
    close(G['image_emb.weight'][::3, ::5], g['g_image_emb'], 5e-2, 'g image_emb')
    close(G['to_logits.1.weight'][::4, ::6], g['g_to_logits_w'], 5e-2, 'g to_logits')
    close(G['special_emb.weight'], g['g_special_emb'], 5e-2, 'g special_emb')
    close(G['text_pos_emb.weight'][:, ::5], g['g_text_pos'], 5e-2, 'g text_pos')
    close(G['target_pos_emb.weights_0'].reshape(-1, D), g['g_tpos0'], 5e-2, 'g tpos0')
    close(G[blk + '0.ln_1.weight'], g['g_ln1w'], 5e-2, 'g ln1w')
    close(G[blk + '1.mlp.c_fc.bias'], g['g_fcb'], 5e-2, 'g fcb')
    close(G[blk + '0.attn.in_proj_weight'][::61, ::29], g['g_inw_s'], 5e-2, 'g in_proj')
    close(G[blk + '1.mlp.c_proj.weight'][::61, ::29], g['g_pjw_s'], 5e-2, 'g c_proj')
    close(G['to_logits_rel.1.weight'], g['g_relw'], 5e-2, 'g relw')
    close(G['to_logits_vid.1.weight'], g['g_vidw'], 5e-2, 'g vidw')
    close(G['text_emb.weight'][g['g_text_emb_row_ids'].to(DEV)][:, ::11], g['g_text_emb_rows'], 5e-2, 'g text_emb rows')
    tn = torch.sqrt(sum((v.double()**2).sum() for v in G.values())).item()
    print('total grad norm', tn, 'ref', g['g_total_norm'].item())
    assert abs(tn / g['g_total_norm'].item() - 1) < 3e-2


def test_bert_mask_predict_against_the_oracles_decisions_at_dim_1024(golden):
    """generate_images at dim 1024 under injected race variates: every sampled token, keep mask, candidate score and choice against
    oracle/sampling.py on the run's own logits (the form of tests/test_parity_gpu.py::test_mask_predict_trajectory_with_injected_randomness)."""
    from oracle.synth import synth_tokens
    from test_parity_gpu import _replay_trace
    g = golden('wide_models')
    m = load_synth(wide_bert(), g, 17).eval()
    text = synth_tokens('text', (3, 16), 49408, 17, low=1).to(DEV)
    mp = dict(golden('mask_predict').meta['mp_config'], B=2)
    gen = torch.Generator().manual_seed(5)
    trace = []
    images, _, seq = m.generate_images(text, mask_predict_steps=6, mp_config=mp, dynamic=False, _trace=trace,
                                       _race=lambda name, shape: torch.empty(shape).exponential_(generator=gen).to(DEV))
    assert images.shape == (3, 2, 3, 64, 64) and seq.shape == (6, 16) and int(seq.max()) < 256
    n = _replay_trace(trace, None, 3, 2, False)
    assert n > 0
    print(f'dim 1024 mask-predict: {len(trace)} steps, {n} (video, step) updates verified')
