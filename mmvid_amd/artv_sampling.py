"""The token loop of the ART-V sampler over the key/value cache (DALLE.generate_images, use_cache=True).

One token = [head logits of the image block -> draw -> embedding row of the drawn token -> one decode step through the tower].  The
position lives in the decode session (clip_tower.DecodeSession); the race variates come from torch's graph-safe device generator, or,
with per-video seeds (`seeded`: a seeded.SeededRace), from csrc/variates.hip: block `tok0 + step` of each video's token-race stream.
`sample` picks launch_loop (separate launches, [draw -> advance] per token: captured once and replayed in production; eager for injected
variates, a `filter_thres` that filters, `stable` and up to 4 tokens) or, at batch 1-2, token_launch_loop (the whole token is ONE
persistent launch, with a restart point from which launch_loop finishes the call when the device was shared under it).

Classifier-free guidance (`guide`: one fp32 scale per video, on the device): the cache, the session and the head rows hold 2B sequences,
rows 0..B-1 under the conditional prompt and rows B..2B-1 under the unconditional one.  One head launch gives both logit blocks, the
draw races lc + w * (lc - lu), and the embedding launch writes the drawn token's row for both halves: the launches of a guided token
are the unguided token's, and launch_loop captures them the same way.  A guided call never takes token_launch_loop.  Which launches
make a draw (plain, truncated, guided, both) is token_draw.draw's decision; TokenLoop.draw hands it the static buffers.

Video prediction (`given`: known frames per video, sample_given): a frame mask splits the target sequence into runs (segments).  A known
run enters through the prefill, the prompt and every frame so far once more from position 0; an unknown run is a TokenLoop of its own
length (`steps`) that starts at the run's first position, on a fresh decode session.  A generated token runs the launches above."""
import os

import torch

from . import _lib, ops, token_draw


TOKEN_RACE = ops.VARIATE_PURPOSES['tok']
# the pre-drawn variates of a whole loop, in floats (256 MB); above it the captured step draws per token
E_ALL_MAX = 1 << 26


def k_keep(filter_thres, total):
    return max(int((1 - filter_thres) * total), 1)


def keep_top(logits, k):
    """dalle_artv.py:61-67: each row's k largest logits, -inf elsewhere (the logits themselves when k covers the row)."""
    if k >= logits.shape[-1]:
        return logits
    val, ind = torch.topk(logits, k)
    return torch.full_like(logits, float('-inf')).scatter_(1, ind, val)


class TokenLoop:
    """The buffers of one sampling call and the two halves of a token, draw(step) and advance()."""

    def __init__(self, model, h, cache, first_pos, filter_thres, temperature, race, trunc, guide=None, trace=None, steps=None, seeded=None):
        rows, dev = h.shape[0], h.device  # the tower's rows: B, or 2B under guidance (h = [conditional; unconditional])
        B = rows // 2 if guide is not None else rows
        c0, c1 = model._allowed_range(model.control_seq_len)
        self.model, self.ln, self.first_pos, self.temperature, self.race, self.trunc = model, model.to_logits[0], first_pos, temperature, race, trunc
        self.guide, self.trace, self.seeded = guide, trace, seeded
        # steps: the tokens of this loop, a run of unknown frames (None: the whole target sequence); tok0: the run's first token as an
        # index in the target sequence, which names the injected variates
        self.V, self.steps, self.k_keep = c1 - c0, model.target_seq_len if steps is None else int(steps), k_keep(filter_thres, model.total_tokens)
        self.tok0 = first_pos - model.control_seq_len - 1
        self.w_blk, self.b_blk = model._w16()[c0:c1], model.to_logits[1].bias.detach()[c0:c1].contiguous()
        self.pos_rows, self.iemb = model._pos_rows().detach().contiguous(), model.image_emb.weight.detach()
        self.sess = model.transformer.decode_session(cache, first_pos, graph=False)
        self.out = torch.empty(B, self.steps, dtype=torch.long, device=dev)
        self.hbuf, self.logits = h.clone(), torch.empty(rows, self.V, device=dev)
        self.lc, self.lu = self.logits[:B], self.logits[B:]  # (guided: the two branches, one row stride)
        self.lt = torch.empty(B, self.V, device=dev) if guide is not None and trunc is not None else None  # the guided, truncated value
        self.tok, self.E = torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, self.V, device=dev)
        # production: the race variates of the whole loop in one draw (an exponential_ inside the captured step costs its launch and two
        # generator-state fills per replay: 7 us per token at batch 72); the draw of token n reads block n = position - first_pos.  Capped at 256 MB on top of
        # the KV cache (batch 64 at 1,024 steps x 1,024 codes) and at the 1,024 rows the indexed draw kernel takes: larger calls draw per step
        fits = race is None and trace is None and self.steps * B * self.V <= E_ALL_MAX and B <= 1024
        self.E_all = torch.empty(self.steps, B, self.V, device=dev) if fits else None
        if fits and seeded is None:
            self.E_all.exponential_()
        elif fits:  # seeded: the same block, ONE fill launch; the draw number of a token is its index in the target sequence
            seeded.fill(self.E_all, TOKEN_RACE, 1, draw_first=self.tok0)
        self.guided = dict(logits_u=self.lu, scale=guide, rows_per_scale=1) if guide is not None else {}  # (built once: draw runs per token)
        self.variates = (self.E_all, dict(step_dev=self.sess.pos, step0=first_pos)) if fits else (self.E, {})
        self.hid = self.hbuf  # the hidden state the next draw reads: the prompt's last position, then the session's output buffer

    def draw(self, step):
        """The token of `step` into self.tok.  (`step` names the injected variates only: the pre-drawn ones are indexed by the position.)"""
        src, ln, T = self.hid, self.ln, self.temperature
        rec = None
        if self.trace is not None:
            rec = {}
            self.trace.append(rec)
        if self.model.stable:
            self.hbuf.copy_(self.model.norm_by_max(src))
            src = self.hbuf
        ops.gemv_rows(src, self.w_blk, self.b_blk, ln=(ln.weight, ln.bias, ln.eps), round_in=True, out=self.logits)  # LN + head block
        if rec is not None:
            rec['logits'] = self.logits.clone()
        lg = keep_top(self.logits, self.k_keep) if self.guide is None else self.lc
        E, at = self.variates
        if self.race is not None:
            E.copy_(self.race(f'tok{self.tok0 + step}', tuple(E.shape)))
        elif self.E_all is None and self.seeded is None:
            E.exponential_()
        elif self.E_all is None:  # draw number tok0 + (pos - first_pos), the position read on the device: captured with the step
            self.seeded.fill(E, TOKEN_RACE, 1, draw_first=self.tok0 - self.first_pos, draw_dev=self.sess.pos)
        token_draw.draw(lg, E, trunc=self.trunc, logit_div=T, want_y=False, tok_out=self.tok, record=rec, **self.guided, **at,
                        trunc_out=lg if self.guide is None else self.lt)  # unguided: the truncation is in place
        if rec is not None:
            rec['E'], rec['tok'] = E.clone(), self.tok.clone()
            if self.guide is not None:
                rec['scale'] = self.guide.clone()

    def advance(self):
        """The embedding row of the drawn token (the same launch files it in `out` at column pos - first_pos), then one position through the
        tower.  Guided: the row goes to both halves of the session's input."""
        if self.guide is not None:
            ops.decode_embed_groups(self.tok, self.iemb, self.pos_rows, self.sess.pos, self.sess.x, 2, record=self.out, record_pos0=self.first_pos)
        else:
            ops.decode_embed(self.tok, self.iemb, self.pos_rows, self.sess.pos, self.sess.x, record=self.out, record_pos0=self.first_pos)
        if self.trace is not None:
            self.trace[-1]['x_in'] = self.sess.x.clone()
        self.sess.advance()
        self.hid = self.sess.y

    def token(self, step=-1):
        self.draw(step)
        self.advance()

    def decode_token(self):
        """The argument block of the one-launch token (the tensors it points to stay alive in this object and in the model)."""
        tk, ln = _lib.DecodeToken(), self.ln
        tk.tok, tk.table, tk.table_rows, tk.pos_rows, tk.pos_off = self.tok.data_ptr(), self.iemb.data_ptr(), self.iemb.shape[0], self.pos_rows.data_ptr(), 0
        tk.record, tk.record_ld, tk.record_pos0 = self.out.data_ptr(), self.out.stride(0), self.first_pos
        tk.lnf_w, tk.lnf_b, tk.lnf_eps, tk.head_w, tk.head_b, tk.V = ln.weight.data_ptr(), ln.bias.data_ptr(), ln.eps, self.w_blk.data_ptr(), self.b_blk.data_ptr(), self.V
        tk.E, tk.e_step_stride, tk.e_pos0, tk.temperature, tk.tok_offset, tk.logits_out = self.E_all.data_ptr(), self.E_all.stride(0), self.first_pos, self.temperature, 0, None
        return tk

    def finish(self):
        self.out[:, self.steps - 1].copy_(self.tok)  # (the last token is never embedded, so no launch has filed it in `out`)
        return [self.out[:, i:i + 1] for i in range(self.steps)]


def launch_loop(loop, start=0, capture=False):
    """Tokens start .. steps - 1 by separate launches: every token but the last is drawn and run through the tower, the last only drawn.
    capture: two eager tokens have warmed every kernel; [draw -> advance] is then captured once and replayed."""
    sess = loop.sess
    for step in range(start, loop.steps - 1):
        if sess.graph is not None:
            sess.replay()
            continue
        loop.token(step)
        if capture and step == 1:
            sess.capture(loop.token)
    loop.draw(loop.steps - 1)
    toks = loop.finish()
    sess.check()
    return toks


def token_launch_loop(loop):
    """One persistent launch per token.  The first token is drawn from the prompt's hidden state the usual way; every launch then embeds
    the token drawn last, files it in `out`, and draws the next one.  Restart point: the launch needs its 256 blocks resident together; if
    the device is shared while it runs, a poll times out, the launch and all later ones on the session's workspace are void, and the
    failure flag says so.  Every `_decode_check_every` tokens the flag is read (one sync per ~15 ms of work) and the token to embed next is
    kept; after a failure the loop goes back to the last verified token and finishes with launch_loop (five launches per layer, eager)."""
    sess, tok, steps, tk = loop.sess, loop.tok, loop.steps, loop.decode_token()
    check_every, hook = loop.model._decode_check_every, loop.model._token_step_hook  # (hook, tests: called after every launch)
    loop.draw(0)
    direct = os.environ.get('MMVID_DECODE_TOKEN_GRAPH', '0') == '0'  # one kernel per token: launched directly (a one-node graph replay costs more)
    good_step, good_tok = 0, tok.clone()
    for step in range(1, steps):  # step = tokens launched so far
        if sess.graph is not None:
            sess.replay()
        else:
            sess.token_step(tk)
            if step == 2 and not direct:
                sess.capture(lambda: sess.token_step(tk))
        if hook is not None:
            hook(step, sess)
        if step % check_every == 0 or step == steps - 1:
            if sess.failed():
                break
            good_step = step
            good_tok.copy_(tok)
    else:
        return loop.finish()
    # a persistent launch failed somewhere after token `good_step` (which `tok` holds again): go on from there with the separate launches
    tok.copy_(good_tok)
    sess.fall_back(loop.first_pos + good_step)
    loop.advance()
    return launch_loop(loop, good_step + 1)


def sample(model, h, cache, first_pos, filter_thres, temperature, race, trunc=None, guide=None, trace=None, steps=None, seeded=None):
    """h [B, dim]: the hidden state of the prompt's last position, `cache` filled below first_pos -> the sampled tokens, target_seq_len columns [B, 1]
    (`steps` columns for a run of that many tokens that starts at first_pos: sample_given).
    guide (fp32 [B] on the device): h and the cache hold 2B sequences, conditional then unconditional.  trace (a list): one dict of clones
    per token (logits, E, tok, x_in for every token but the last; scale when guided; logits_t and kept when truncated), eager loop.
    seeded (a seeded.SeededRace over the B videos): the variates are a function of each video's seed; every path below stays as it is."""
    loop = TokenLoop(model, h, cache, first_pos, filter_thres, temperature, race, trunc, guide, trace, steps, seeded)
    capture = race is None and trace is None and loop.k_keep >= loop.V and not model.stable and loop.steps > 4
    # (the one-launch token has no truncation and no second branch in it: a call with top_k / top_p or guidance takes the separate
    # launches; MMVID_DECODE_TOKEN=0: all do)
    if (capture and loop.sess.persistent and loop.E_all is not None and loop.V <= 2048 and trunc is None and guide is None and
            os.environ.get('MMVID_DECODE_TOKEN', '1') != '0'):
        return token_launch_loop(loop)
    return launch_loop(loop, 0, capture)


# ---- video prediction: known frames enter through the prefill ---------------------------------------------------------------------------
def segments(mask_row):
    """The runs of a frame mask (T values, non-zero = known) -> [(known, frame0, frames)], in frame order.  Pure host code."""
    row = [bool(v) for v in (mask_row.tolist() if torch.is_tensor(mask_row) else mask_row)]
    runs = []
    for t, k in enumerate(row):
        if runs and runs[-1][0] == k:
            runs[-1] = (k, runs[-1][1], runs[-1][2] + 1)
        else:
            runs.append((k, t, 1))
    return runs


def group_rows(mask):
    """Rows of a [B, T] mask with the same pattern -> [(pattern as a tuple of 0 / 1, [rows])], in order of first appearance."""
    groups = {}
    for r, row in enumerate(mask.tolist() if torch.is_tensor(mask) else mask):
        groups.setdefault(tuple(int(bool(v)) for v in row), []).append(r)
    return list(groups.items())


def scatter_rows(parts, B):
    """[(rows, tokens [len(rows), L])] of disjoint row sets that cover 0 .. B-1 -> tokens [B, L] (one part over all rows: that tensor)."""
    if len(parts) == 1 and list(parts[0][0]) == list(range(B)):
        return parts[0][1]
    first = parts[0][1]
    out = torch.empty((B, ) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
    seen = 0
    for rows, tok in parts:
        out[torch.as_tensor(list(rows), dtype=torch.long, device=first.device)] = tok
        seen += len(rows)
    if seen != B:
        raise ValueError(f'scatter_rows: {seen} rows for a batch of {B}')
    return out


def check_frame_mask(mask, B, T):
    """A mask of known frames, [B, T] or [T], bool or uint8 -> uint8 [B, T] on the host, or ValueError."""
    mask = torch.as_tensor(mask)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'given: the mask must be bool or uint8, got {mask.dtype}')
    if mask.dim() > 2:
        raise ValueError(f'given: a token-grid or pixel mask {tuple(mask.shape)} cannot be honoured by a raster-order model (a token cannot '
                         f'condition on later tokens of its frame): expected whole frames, [B, T] or [T] with T = {T}')
    if tuple(mask.shape) not in ((T, ), (B, T)):
        raise ValueError(f'given: the mask must be [B, T] = [{B}, {T}] or [T], got {tuple(mask.shape)}')
    mask = (mask != 0).to(torch.uint8).cpu()
    if mask.dim() == 1:
        mask = mask.view(1, T).expand(B, T)
    return mask.contiguous()


def check_given(given, B, T, n, V):
    """The `given` of DALLE.generate_images -> (mask [B, T] uint8 on the host, tokens int64 [B, T * n] where they were), or ValueError.
    An ART-V model predicts tokens in raster order, frame after frame: it can condition on whole known frames that come BEFORE what it
    generates and on nothing else, so a mask per token or per pixel is refused.  One host read when the tokens are on a device: the count
    of known ids outside [0, V)."""
    if not isinstance(given, (tuple, list)) or len(given) != 2:
        raise ValueError('given: expected (mask, tokens)')
    mask, tokens = given
    mask = check_frame_mask(mask, B, T)
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int64 or tuple(tokens.shape) != (B, T * n):
        got = f'{tokens.dtype} {tuple(tokens.shape)}' if torch.is_tensor(tokens) else type(tokens).__name__
        raise ValueError(f'given: the tokens must be int64 [B, T * n] = [{B}, {T * n}], got {got}')
    known = mask.bool().view(B, T, 1).expand(B, T, n).reshape(B, T * n).to(tokens.device)
    outside = int((known & ((tokens < 0) | (tokens >= V))).sum())
    if outside:
        raise ValueError(f'given: {outside} known token ids are outside [0, num_image_tokens) = [0, {V})')
    return mask, tokens


def sample_given(model, prompt, pattern, known, filter_thres, temperature, race, trunc=None, guide=None, trace=None, seeded=None):
    """One pass through the segments of a frame mask for rows that share it.  prompt [rows, 1 + control_seq_len]: <bos> text visual ids
    (rows = B, or 2B under guidance); pattern: the T mask values; known int64 [B, T * n], read under the mask -> tokens [B, T * n].

    A run of known frames draws nothing: its tokens join the prefix, and the whole prefix (prompt and every frame up to the end of the
    run) goes through the tower's prefill from position 0 once more, which rewrites those cache rows -- the known frames get their keys
    and values exactly as the prompt's tokens do -- and gives the hidden state of the last known position, from which the next token is
    drawn.  A run of unknown frames is a TokenLoop of its own length over a fresh decode session, under the rules of `sample` (capture
    above 4 tokens, the one-launch token at batch 1-2): a generated token runs the launches it runs in a call without known frames.  The
    last token of a run is never embedded by the loop; when a known run follows, the prefill embeds it.  A known run at the end costs
    nothing.  Known frames condition only what comes after them."""
    n, dev = model.image_seq_len, prompt.device
    B = known.shape[0]
    halves = prompt.shape[0] // B
    runs = segments(pattern)
    if all(k for k, _, _ in runs):
        return known.clone()
    tower = model.transformer
    cache = tower.new_kv_cache(prompt.shape[0], model.total_seq_len, dev)
    out = torch.empty(B, len(pattern) * n, dtype=torch.long, device=dev)
    ids, h = prompt, None
    for i, (k, f0, nf) in enumerate(runs):
        lo, hi = f0 * n, (f0 + nf) * n
        if k:
            out[:, lo:hi] = known[:, lo:hi]
            if i == len(runs) - 1:
                break
            ids = torch.cat((ids, out[:, lo:hi].repeat(halves, 1)), 1)
            h = tower.prefill(model._embed_rows(ids, 0), cache)[:, -1, :].contiguous()
            continue
        if h is None:  # the sequence starts with unknown frames: the prompt alone, as in a call without known frames
            h = tower.prefill(model._embed_rows(ids, 0), cache)[:, -1, :].contiguous()
        toks = sample(model, h, cache, ids.shape[1], filter_thres, temperature, race, trunc, guide, trace, steps=hi - lo, seeded=seeded)
        out[:, lo:hi] = torch.cat(toks, dim=-1)
        if i < len(runs) - 1:
            ids = torch.cat((ids, out[:, lo:hi].repeat(halves, 1)), 1)
    return out
