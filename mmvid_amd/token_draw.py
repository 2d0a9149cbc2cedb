"""The token draw of both samplers: which launches turn logits [R, V] into one token per row (the table: DESIGN.md, "The token draw").
sampling.mask_predict, artv_sampling.TokenLoop.draw, DALLE._draw and DALLE.sampling_probs come through here and differ in arguments only: a
new sampling feature belongs here and nowhere else.  The operators are looked up on `ops` at call time (a host test replaces them)."""
from . import ops


class RowParams:
    """The per-row form of `trunc`: the filter settings of a launch whose videos do not share them (sampling.check_video_params makes the
    values).  k int32, p f32, inv_div f32: each [R // rows_per_param] on the device, or None where the scalar holds (top_k, top_p: the
    scalar pair of the old keywords; the caller's logit_div).  Entry r // rows_per_param serves row r; a k of 0 and a p of 1 are off.
    inv_div holds 1 / temperature per entry: the truncation then writes the divided value and the race runs with logit_div = 1."""

    def __init__(self, rows_per_param, k=None, p=None, inv_div=None, top_k=None, top_p=None):
        self.rows_per_param, self.k, self.p, self.inv_div, self.top_k, self.top_p = int(rows_per_param), k, p, inv_div, top_k, top_p

    def rows(self, idx):
        """The record of a subset of the entries (idx: int64 on the device), as a launch over those rows alone reads it."""
        pick = lambda t: None if t is None else t.index_select(0, idx).contiguous()  # noqa: E731
        return RowParams(self.rows_per_param, pick(self.k), pick(self.p), pick(self.inv_div), self.top_k, self.top_p)


def race_value(logits, *, logits_u=None, scale=None, rows_per_scale=None, trunc=None, logit_div=1.0, out=None, record=None, materialise=False):
    """-> (lg, lu): what the race launch reads.  trunc = (k | None, p | None), a RowParams, or None when nothing can be removed: the
    operands as they are, no launch.  Else one ops.logits_truncate (guided when logits_u is given; into `out`, which may be `logits`) and lu
    is None; with a RowParams one ops.logits_truncate_rows, and lg is divided already where the record holds divisors (race_div).
    materialise: a guided value is written out even with no filter on (copy-through).  record (a dict) receives `logits_t` (a clone), `kept`,
    and with a RowParams the parameter rows used: `rows_k`, `rows_p`, `rows_inv_div` (the record's tensors), `rows_per_param`."""
    if trunc is None and not (materialise and logits_u is not None):
        return logits, logits_u
    guide = {} if logits_u is None else dict(logits_u=logits_u, scale=scale, rows_per_scale=rows_per_scale)
    if isinstance(trunc, RowParams):
        lg = ops.logits_truncate_rows(logits, top_k=trunc.top_k, top_p=trunc.top_p, rows_k=trunc.k, rows_p=trunc.p, rows_inv_div=trunc.inv_div,
                                      rows_per_param=trunc.rows_per_param, divide_out=trunc.inv_div is not None, logit_div=logit_div, out=out,
                                      want_kept=record is not None, **guide)
    else:
        lg = ops.logits_truncate(logits, *(trunc or (None, None)), logit_div=logit_div, out=out, want_kept=record is not None, **guide)
    if record is not None:
        lg, kept = lg
        record.update(logits_t=lg.clone(), kept=kept)
        if isinstance(trunc, RowParams):
            record.update(rows_k=trunc.k, rows_p=trunc.p, rows_inv_div=trunc.inv_div, rows_per_param=trunc.rows_per_param)
    return lg, None


def race_div(trunc, logit_div):
    """The logit_div of the race that follows race_value: 1 where the truncation has divided (a RowParams with divisors)."""
    return 1.0 if isinstance(trunc, RowParams) and trunc.inv_div is not None else logit_div


def draw(logits, E, *, logits_u=None, scale=None, rows_per_scale=None, trunc=None, logit_div=1.0, noise_u=None, temperature=0.0, want_y,
         tok_out=None, trunc_out=None, step_dev=None, step0=0, record=None):
    """-> (tok int64 [R], y f32 [R] | None): race_value (into trunc_out), then exactly one race launch on the Exp(1) variates E.  noise_u, temperature:
    the mask-predict noise on y.  tok_out, step_dev, step0 (token-only forms): ART-V's static token buffer and pre-drawn variates E [draws, R, V]."""
    lg, lu = race_value(logits, logits_u=logits_u, scale=scale, rows_per_scale=rows_per_scale, trunc=trunc, logit_div=logit_div, out=trunc_out,
                        record=record)
    logit_div = race_div(trunc, logit_div)
    if lu is None:
        return ops.sample_race(lg, E, noise_u, temperature, logit_div=logit_div, want_y=want_y, tok_out=tok_out, step_dev=step_dev, step0=step0)
    if not want_y and noise_u is None:
        return ops.sample_race_guided_at(lg, lu, scale, rows_per_scale, E, logit_div=logit_div, tok_out=tok_out, step_dev=step_dev, step0=step0), None
    if tok_out is not None or step_dev is not None:
        raise ValueError('token_draw.draw: tok_out and step_dev belong to the token-only guided draw (want_y False, no noise)')
    return ops.sample_race_guided(lg, lu, scale, rows_per_scale, E, noise_u, temperature, logit_div=logit_div)
