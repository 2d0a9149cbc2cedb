"""The token draw of both samplers: which launches turn logits [R, V] into one token per row (the table: DESIGN.md, "The token draw").
sampling.mask_predict, artv_sampling.TokenLoop.draw, DALLE._draw and DALLE.sampling_probs come through here and differ in arguments only: a
new sampling feature belongs here and nowhere else.  The operators are looked up on `ops` at call time (a host test replaces them)."""
from . import ops


def race_value(logits, *, logits_u=None, scale=None, rows_per_scale=None, trunc=None, logit_div=1.0, out=None, record=None, materialise=False):
    """-> (lg, lu): what the race launch reads.  trunc = (k | None, p | None), or None when nothing can be removed: the operands as they
    are, no launch.  Else one ops.logits_truncate (guided when logits_u is given; into `out`, which may be `logits`) and lu is None.
    materialise: a guided value is written out even with no filter on (copy-through).  record (a dict) receives `logits_t` (a clone), `kept`."""
    if trunc is None and not (materialise and logits_u is not None):
        return logits, logits_u
    guide = {} if logits_u is None else dict(logits_u=logits_u, scale=scale, rows_per_scale=rows_per_scale)
    lg = ops.logits_truncate(logits, *(trunc or (None, None)), logit_div=logit_div, out=out, want_kept=record is not None, **guide)
    if record is not None:
        lg, kept = lg
        record.update(logits_t=lg.clone(), kept=kept)
    return lg, None


def draw(logits, E, *, logits_u=None, scale=None, rows_per_scale=None, trunc=None, logit_div=1.0, noise_u=None, temperature=0.0, want_y,
         tok_out=None, trunc_out=None, step_dev=None, step0=0, record=None):
    """-> (tok int64 [R], y f32 [R] | None): race_value (into trunc_out), then exactly one race launch on the Exp(1) variates E.  noise_u, temperature:
    the mask-predict noise on y.  tok_out, step_dev, step0 (token-only forms): ART-V's static token buffer and pre-drawn variates E [draws, R, V]."""
    lg, lu = race_value(logits, logits_u=logits_u, scale=scale, rows_per_scale=rows_per_scale, trunc=trunc, logit_div=logit_div, out=trunc_out,
                        record=record)
    if lu is None:
        return ops.sample_race(lg, E, noise_u, temperature, logit_div=logit_div, want_y=want_y, tok_out=tok_out, step_dev=step_dev, step0=step0)
    if not want_y and noise_u is None:
        return ops.sample_race_guided_at(lg, lu, scale, rows_per_scale, E, logit_div=logit_div, tok_out=tok_out, step_dev=step_dev, step0=step0), None
    if tok_out is not None or step_dev is not None:
        raise ValueError('token_draw.draw: tok_out and step_dev belong to the token-only guided draw (want_y False, no noise)')
    return ops.sample_race_guided(lg, lu, scale, rows_per_scale, E, noise_u, temperature, logit_div=logit_div)
