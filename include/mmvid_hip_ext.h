/* mmvid_hip_ext.h -- entry points of libmmvid_hip.so added after the list of mmvid_hip.h was pinned.
 *
 * tests/test_cdecl_host.py pins mmvid_hip.h to an exact count of functions and structs, and the binding tests require the ctypes
 * tables derived from it to equal that list.  A new entry point therefore goes HERE: same library, same plain C conventions (device
 * pointers + sizes, caller-allocated outputs, `stream` a hipStream_t, 0 on success, message via mmvid_last_error()), read by the same
 * strict reader (mmvid_amd/_cdecl.py) and bound by mmvid_amd/_lib.py from tables of its own (EXT_HEADER, EXT_SIGNATURES).  Adding an
 * entry point here leaves MMVID_ABI_VERSION alone; changing one raises it, in mmvid_hip.h.
 */
#ifndef MMVID_HIP_EXT_H
#define MMVID_HIP_EXT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Seeded sampling: the race variates of the samplers as a pure function of (video seed, purpose, substream, draw, index) ------
 *
 * The function.  Philox4x32-10 is the generator of Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (the Random123
 * philox4x32 with 10 rounds: multipliers 0xD2511F53 on counter word 0 and 0xCD9E8D57 on counter word 2, key increments 0x9E3779B9 and
 * 0xBB67AE85 per round; one round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))).
 * Variate i of the block that the 64-bit video seed s owns for (purpose, substream, draw) is made from
 *     w = word (i & 3) of Philox4x32-10(counter = {i >> 2, purpose, substream, draw}, key = {s & 0xffffffff, s >> 32})
 * (counter and key words in the order c0..c3, k0..k1; substream and draw enter as their low 32 bits) as
 *     kind 0, uniform:  (float)(w >> 8) * 2^-24                       in [0, 1), a multiple of 2^-24
 *     kind 1, Exp(1):   0 - logf((float)((w >> 8) + 1) * 2^-24)       the argument is an exact fp32 in (0, 1]: the result lies in
 *                                                                     [0, 24 ln 2 = 16.64], is +0 at w >> 8 = 2^24 - 1, never inf / NaN
 * (logf: the device's fp32 natural logarithm.)  Purposes: 1 = token race, 2 = token noise, 3 = keep race -- the `tok{t}`,
 * `tok{t}_noise_u` and `keep{t}` tensors of the samplers; `draw` is t (mask-predict: the step; ART-V: the token's index in the target
 * sequence); substream is 0 but for long videos, where it names the window (mmvid_amd/long_video.py: window_substream).
 *
 * The layout.  out is fp32 [draws][videos * rows_per_video][n], contiguous.  Row r of a block belongs to video v = r / rows_per_video
 * and element (r, c) is variate i = (r % rows_per_video) * n + c of that video -- a video's rows_per_video * n variates of one draw lie
 * contiguous, in index order, wherever the video sits in the batch.  Block k has draw number draw_first + k.  With draw_dev != NULL
 * (an int32 on the device) draws must be 1 and the draw number is *draw_dev + draw_first, read on the device at execution: a captured
 * per-token step needs no host input.  seeds: int64 [videos] on the device, each in [0, 2^63) by the Python layer's rule (the kernel
 * takes all 64 bits as they are); substream: int32 [videos] on the device, or NULL for 0.
 *
 * Refused with an error (never a fault): NULL seeds or out; a negative size; rows_per_video * n > 2^34 (i >> 2 must fit counter word
 * 0); purpose outside 1..3; kind outside 0..1; draws != 1 with draw_dev; without draw_dev a draw number outside [0, 2^32).  Zero
 * rows, zero columns or zero draws: nothing is launched. */
int mmvid_variates_fill(const int64_t* seeds, const int32_t* substream, int64_t videos, int64_t rows_per_video, int64_t n,
                        int purpose, int kind, const int32_t* draw_dev, int64_t draw_first, int64_t draws,
                        float* out, void* stream);

/* ---- Weight EMA: an exponential moving average of the flat fp32 weights, updated on the device after the optimiser ----------------
 *
 * The rule (csrc/ema.hip; tests/ema_ref.py is the host replica, bit for bit).  t = *step_dev where step_dev != NULL (an fp32 on the
 * device: the count of finished optimiser steps, this one included, read at execution so that a captured step needs no host input),
 * else (float)step.  Then, every operation one correctly rounded fp32 operation,
 *     d    = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay
 *     a    = 1.f - d
 *     ema' = fmaf(a, p - ema, ema)             for each of the n elements; p - ema is an fp32 subtraction of its own
 * Where ema == p the result is p, bit for bit (but for ema = p = -0, which IEEE arithmetic turns into +0: the same number).  Denormal
 * intermediates are left unspecified.
 *
 * Lazy rows: row_flags, table_lo, table_rows, rowlen as in mmvid_adam_step_rows (a table of table_rows x rowlen elements at element
 * table_lo of both buffers, one uint8 flag per row on the device; row_flags NULL: no table).  A row whose flag is 0 is neither read nor
 * written: the caller keeps ema == p there, where the update is the identity.
 *
 * Refused with an error (never a fault, nothing launched): NULL ema or p; ema == p or overlapping ranges; n < 0; a pointer that is
 * not 16-byte aligned; decay outside [0, 1) or NaN; step < 1 without step_dev; a lazy table that does not lie inside [0, n) or whose
 * table_lo or rowlen is not a multiple of 4.  n == 0: nothing is launched. */
int mmvid_ema_update(float* ema, const float* p, int64_t n, float decay, int warmup, int step, const float* step_dev,
                     const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, void* stream);

/* ---- Non-finite guard: a training step whose gradient is not finite is skipped, by a verdict taken and obeyed on the device ------
 *
 * The rule (csrc/optim.hip; tests/guard_ref.py is the host replica).  mmvid_step_guard runs between the gradient norm and the
 * optimiser, on their stream: one launch of one thread, plain loads and stores.  With sq = *sqnorm (the sum of squares that
 * mmvid_grad_sqnorm* left) and skip = sq is inf or NaN (1 or 0):
 *     guard_i[0] = skip                           the verdict the guarded entries read
 *     guard_i[1] += skip                          steps skipped so far
 *     guard_i[2] = skip ? guard_i[2] + 1 : 0      the current run of skipped steps
 *     guard_i[3] += 1                             steps seen
 *     guard_f[0] = sqrtf(sq) * grad_scale         the gradient norm the Adam kernel clips on (two fp32 operations), NaN / inf included
 *     guard_f[1] = guard_f[0]   only if !skip     the last finite gradient norm
 *     *step_dev += 1.f          only if !skip     the count of APPLIED steps: this call stands in for the step's mmvid_counter_add
 * guard_i: int32 [4], guard_f: fp32 [2], step_dev: fp32 [1], all on the device, zeroed by the caller before the first step.
 * Refused with an error (nothing launched): a NULL pointer; a pointer that is not 4-byte aligned.
 *
 * mmvid_adam_step_guarded / mmvid_ema_update_guarded take the arguments of mmvid_adam_step_rows (mmvid_hip.h) / mmvid_ema_update plus
 * skip_dev, an int32 on the device (guard_i) read at execution: every thread of the kernel returns before its first load where
 * *skip_dev != 0 -- nothing is read, nothing is written, p, m, v, the bf16 shadow and ema keep every byte.  With skip_dev NULL or
 * *skip_dev == 0 they write the bytes of the unguarded entry (the same kernel; the unguarded entries pass NULL).  Every refusal of the
 * unguarded entry carries over; in addition a skip_dev that is not 4-byte aligned is refused.  No atomics. */
int mmvid_step_guard(const float* sqnorm, float grad_scale, float* step_dev, int32_t* guard_i, float* guard_f, void* stream);
int mmvid_adam_step_guarded(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, const float* lr_dev,
                            float beta1, float beta2, float eps, float weight_decay, int step, const float* step_dev, float max_norm,
                            const float* sqnorm, float grad_scale, const uint8_t* row_flags, int64_t table_lo, int64_t table_rows,
                            int rowlen, const int32_t* skip_dev, void* stream);
int mmvid_ema_update_guarded(float* ema, const float* p, int64_t n, float decay, int warmup, int step, const float* step_dev,
                             const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, const int32_t* skip_dev,
                             void* stream);

/* ---- Per-video sampling parameters: top-k, top-p and the softmax temperature of a row read on the device ---------------------------
 *
 * Serves the truncation of both samplers (mmvid_logits_truncate in mmvid_hip.h states the rule and which reference lines it stands
 * for: the draw of dalle_bert.py:527-534, the top_k filter of dalle_artv.py:61-67 and the division by the temperature of :274-276)
 * for a batch whose videos do not share their settings.  The contract is mmvid_logits_truncate's -- the same rule, one wave per row,
 * the row in registers, 1 <= V <= 2048, the guided form with logits_u / scale_dev / rows_per_scale, kept nullable -- and with
 * top_k_dev, top_p_dev and inv_div_dev all NULL and divide_out 0 the output is that entry's, byte for byte.
 *
 * Per-row arrays.  top_k_dev (int32), top_p_dev (fp32) and inv_div_dev (fp32) live on the device, hold R / rows_per_param entries
 * each and are read at execution, entry r / rows_per_param for row r (a captured step may change them between replays).  Each is
 * optional: NULL means the scalar argument (top_k, top_p, 1.0f / logit_div) holds for every row.  inv_div_dev holds 1 / temperature
 * as the host rounds it in fp32 -- the 1.0f / logit_div that the C entries compute; the device never divides.
 *
 * Device values.  A top_k outside [1, V) switches top-k off for its row (0 is the documented "off"); a top_p >= 1 switches the
 * nucleus off.  A top_p that is not > 0, or an inv_div that is not finite and positive, leaves the values of THAT ROW unspecified:
 * no other row, no byte outside out [R, V] and kept [R] and no trip count depends on it.  The caller checks its values on the host
 * (mmvid_amd/sampling.py: check_video_params).
 *
 * divide_out.  0: a kept class is written as g, as mmvid_logits_truncate writes it.  1: as g * inv_div of its row, one rounded fp32
 * product -- the product a race forms from g and 1.0f / logit_div -- so mmvid_sample_race* on out with logit_div = 1 draws what it
 * would draw on the undivided row with that row's logit_div: this is how a per-row temperature reaches a draw kernel that takes one
 * scalar.  A row with both filters off is copied through (divide_out 0) or divided (1).  kept counts the finite values written.
 *
 * No atomics, no LDS, no barrier; a row's stores follow all of its loads, so out may be logits.
 *
 * Refused with an error (never a fault, nothing launched, nothing written): everything mmvid_logits_truncate refuses (NULL logits
 * or out; V outside [1, 2048]; R < 0; ld or ld_out below V; logit_div or the scalar top_p not > 0; logits_u without scale_dev or the
 * reverse; in the guided form rows_per_scale <= 0 or R no multiple of it); rows_per_param <= 0 or R no multiple of it; a per-row
 * array that is not 4-byte aligned; divide_out outside {0, 1}.  R == 0: nothing is launched. */
int mmvid_logits_truncate_rows(const float* logits, const float* logits_u, int64_t ld, const float* scale_dev, int64_t rows_per_scale,
                               float logit_div, int top_k, float top_p, const int32_t* top_k_dev, const float* top_p_dev,
                               const float* inv_div_dev, int64_t rows_per_param, int divide_out, int64_t R, int V,
                               float* out, int64_t ld_out, int32_t* kept, void* stream);

/* ---- Trainer telemetry: per-parameter gradient, weight and update statistics, taken on the device after the optimiser ----------------
 *
 * The rule (csrc/telemetry.hip; tests/telemetry_ref.py is the host replica, bit for bit).  g, p, m, v are the flat fp32 buffers of
 * mmvid_adam_step_rows, n elements each, as the optimiser LEFT them; they are only read.  CHUNK = MMVID_TELEMETRY_CHUNK (mmvid_hip.h).
 *
 * Segments and chunks.  Segment s (0 <= s < segments: one parameter) is the range [seg_off[s], seg_off[s] + seg_len[s]) of the flat
 * buffers: offsets are multiples of 128 elements, lengths are >= 1, what lies between two segments belongs to none and is never read.
 * A segment of length L is cut into ceil(L / CHUNK) chunks; chunk k of it covers its elements [k CHUNK, min(L, (k + 1) CHUNK)) and has
 * the global index seg_chunk0[s] + k.  seg_chunk0 is ascending (seg_chunk0[0] = 0, seg_chunk0[s + 1] = seg_chunk0[s] + the chunks of s)
 * and `chunks` is the total.  The three tables are int64 [segments] on the device.
 *
 * Statistics of a segment.  Over the elements the optimiser touched -- all of them, but for the rows of the lazy table (below) whose
 * flag is 0 -- with "finite" meaning neither NaN nor +-inf:
 *     g_sumsq     sum of g * g over the finite g               g_absmax   max of |g| over the finite g (+0 where there is none)
 *     g_nonfinite the number of g that are NaN or +-inf        g_count    the number of g looked at, finite or not       (both int32)
 *     d_sumsq     sum of d * d, d the update this step applied to the element, recomputed from the state Adam left:
 *                     lr = lr_dev ? *lr_dev : lr ;  t = step_dev ? *step_dev : (float)step
 *                     bc1 = 1.f - powf(beta1, t) ;  bc2s = sqrtf(1.f - powf(beta2, t))     (with step_dev: the device's powf, as in the
 *                                                                                            Adam kernel; else computed by the host)
 *                     d = ((lr / bc1) * m) / (sqrtf(v) / bc2s + eps)                         every operation one rounded fp32 operation,
 *                                                                                            none contracted; lr / bc1 is formed once
 *                 (L2 weight decay sits inside m, so the formula holds with it.)  With skip_dev != NULL and *skip_dev != 0 (the verdict
 *                 of mmvid_step_guard: no update happened) d_sumsq is +0 for every segment and m, v are not read; the g statistics are
 *                 taken as ever -- they say where the non-finite values sit.
 * and over ALL elements of the segment:
 *     p_sumsq     sum of p * p
 * Lazy rows: row_flags, table_lo, table_rows, rowlen as in mmvid_adam_step_rows.  A row whose flag is 0 adds nothing to the g
 * statistics, g_count and d_sumsq (Adam did not touch it; g, m, v are not read there) and adds to p_sumsq like any other.
 *
 * Summation order: a function of a segment's length and CHUNK only -- never of the grid, the CU count or an arrival order; no
 * floating-point atomics.  Every product and sum below is one rounded fp32 operation.  A term that does not count (a non-finite g, an
 * unflagged row, a skipped step, an element past the end of the segment) is +0.
 *   Pass 1, a chunk (256 threads; thread T, trip r = 0..3, lane e = 0..3 hold element j = 1024 r + 4 T + e of the chunk):
 *     q(T, r) = (x0 x0 + x1 x1) + (x2 x2 + x3 x3)                            the four elements of a thread's trip
 *     a(T)    = (((0 + q(T, 0)) + q(T, 1)) + q(T, 2)) + q(T, 3)              a thread, its trips in order
 *     w(W)    = the halving tree over the 64 threads of wave W = T / 64:     x[i] + x[i + 32] for i < 32, then + 16, 8, 4, 2, 1
 *     chunk   = (w(0) + w(1)) + (w(2) + w(3))
 *   Pass 2, a segment of C chunks with the chunk sums c[0..C):
 *     a(T)    = ((0 + c[T]) + c[T + 256]) + c[T + 512] ...                   thread T, every 256th chunk in order (+0 where T >= C)
 *     then the wave trees and the sum of the four waves, as in pass 1.
 * Maxima and counts are order-free and exact.  The record's total is the sum of g_sumsq over the segments by the pass-2 rule with the
 * segments in the place of the chunks.
 *
 * The ring.  count = count_dev[0] counts calls (an int32 on the device, zeroed by the caller before the first call; taken as unsigned).
 * When count % every != 0 the call writes nothing but count_dev[0] = count + 1: every thread of passes 1 and 2 returns before its
 * first load on that scalar.  Otherwise the record goes to slot k = (count / every) % slots of
 *     ring_f [slots][segments][4]   g_sumsq, g_absmax, p_sumsq, d_sumsq              ring_i [slots][segments][2]   g_nonfinite, g_count
 *     head_i [slots][4]             count, (int)t, the skip verdict (0 / 1), 1       head_f [slots][2]             lr, the record's total
 * and count_dev[0] = count + 1 follows, in a last launch of one block on the stream: at most three launches and no host input, so a
 * captured step fills the ring by itself.  partials_f (fp32 [chunks][4]) and partials_i (int32 [chunks][2]) are the per-chunk results
 * between the passes, overwritten by every call that is not gated.  The caller zeroes head_i once: a slot is valid where head_i[k][3] is 1.
 *
 * Table values are data.  seg_off is read rounded down to a multiple of 4 and clipped to [0, n], seg_len clipped to [0, n - offset], a
 * chunk index formed from seg_chunk0 clipped to [0, chunks): a corrupt table gives wrong numbers for the segments it concerns and no
 * access outside the buffers.  Every store index comes from the launch geometry, segments, chunks, slots and count_dev.
 *
 * Refused with an error (never a fault, nothing launched, nothing written): a NULL g, p, m, v, table, count_dev, partials, ring or
 * head pointer; g, p, m or v not 16-byte aligned, a table not 8-byte aligned, any other pointer not 4-byte aligned; n < 0; segments
 * outside [1, MMVID_TELEMETRY_MAX_SEGMENTS]; chunks < segments or chunks > n / CHUNK + segments (no plan has more); every < 1;
 * slots < 1; step < 1 without step_dev; beta1 or beta2 outside [0, 1) or NaN; a lazy table that does not lie inside [0, n) or whose
 * table_lo or rowlen is not a multiple of 4.  n == 0: nothing is launched, count_dev included. */
int mmvid_segment_stats(const float* g, const float* p, const float* m, const float* v, int64_t n,
                        const int64_t* seg_off, const int64_t* seg_len, const int64_t* seg_chunk0, int32_t segments, int64_t chunks,
                        float lr, const float* lr_dev, float beta1, float beta2, float eps, int step, const float* step_dev,
                        const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, const int32_t* skip_dev,
                        int32_t every, int32_t slots, int32_t* count_dev, float* partials_f, int32_t* partials_i,
                        float* ring_f, int32_t* ring_i, int32_t* head_i, float* head_f, void* stream);

/* ---- AdamW and the learning-rate schedules of --lr_scheduler, on the device -------------------------------------------------------
 *
 * mmvid_adam_step_decoupled is torch.optim.AdamW (utils/utils_train.py:173-179, `--optimizer adamw`; stepped at train.py:324-325):
 * the argument list of mmvid_adam_step_guarded (skip_dev may be NULL), and with coef, bc1, bc2s, the step count and the learning rate
 * formed exactly as in every other Adam entry (csrc/optim.hip: one kernel text, this form a compile-time variant of it)
 *     gr   = g * coef                                            no decay term in the gradient
 *     m'   = b1 m + (1 - b1) gr ;  v' = b2 v + (1 - b2) gr^2
 *     keep = 1.f - lr * wd                                       one fp32 scalar per launch; lr is *lr_dev where lr_dev != NULL
 *     p'   = p * keep - (lr / bc1) * m' / (sqrtf(v') / bc2s + eps)
 * which is AdamW's order (param.mul_(1 - lr * wd) first).  tests/adamw_ref.py is the fp64 replica with its derived bound.  The bf16
 * shadow, the lazy rows and the verdict behave as in mmvid_adam_step_guarded; with weight_decay == 0 the bytes written are that
 * entry's.  Refused (nothing launched): everything mmvid_adam_step_guarded refuses -- a lazy table with weight_decay != 0 included: a
 * row that never saw a gradient still decays --, and a weight_decay that is negative or not finite.  No atomics. */
int mmvid_adam_step_decoupled(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, const float* lr_dev,
                              float beta1, float beta2, float eps, float weight_decay, int step, const float* step_dev, float max_norm,
                              const float* sqnorm, float grad_scale, const uint8_t* row_flags, int64_t table_lo, int64_t table_rows,
                              int rowlen, const int32_t* skip_dev, void* stream);

/* mmvid_lr_schedule_ext: the closed-form schedules of utils/utils_train.py:332-371 beside mmvid_lr_schedule's kinds 0 and 1, one
 * thread, *lr_out written from *step_dev (the fp32 count of finished optimiser steps).  ns = (long)*step_dev / every is the number of
 * scheduler steps taken before this iteration (train.py:373-374 steps the scheduler after every `every`-th iteration).
 *     kind 2  StepLR(step_size = a, gamma)  (utils_train.py:332-343)
 *                 lr = lr_max * powf(gamma, (float)(ns / a))                                    integer quotient
 *     kind 3  CosineAnnealingLR(T_max = a, eta_min = lr_min)  (utils_train.py:345-356)
 *                 r = ns % (2 a) ;  x = (PI * (float)r) / (float)a ;  lr = lr_min + ((lr_max - lr_min) * (1.f + cosf(x))) * 0.5f
 *                 PI the fp32 nearest to pi.  The argument is reduced in integers: the error does not grow with the step count.
 *     kind 4  deepspeed WarmupDecayLR(total = b, min = lr_min, max = lr_max, warmup = a)  (utils_train.py:358-371)
 *                 ns == 0: lr_max (the optimiser's construction rate).  Otherwise k = ns - 1, w = max(a, 2),
 *                 g = k < w ? logf((float)(k + 1)) / logf((float)w) : fmaxf(0.f, (float)(b - k) / (float)max(1, b - w))
 *                 lr = lr_min + (lr_max - lr_min) * g
 *                 The warm-up branch and the clamp w >= 2 are kind 1's.  Third-party arithmetic, restated from deepspeed's
 *                 published semantics: parity unpinned, as for kind 1.
 * Every product, sum and quotient is one rounded fp32 operation; powf, cosf and logf are the device library's.  lr_min is not read by
 * kind 2, gamma only by kind 2, b only by kind 4.  Refused (nothing launched): a NULL or misaligned pointer; kind outside 2..4 (0 and
 * 1 stay with mmvid_lr_schedule); every < 1; a < 1; b < a for kind 4; gamma outside (0, 1] or NaN for kind 2; a (kind 4: b) above
 * 2^24, where the fp32 step count stops -- below it every integer the kernel converts is exact. */
int mmvid_lr_schedule_ext(const float* step_dev, int kind, float lr_min, float lr_max, int every, int64_t a, int64_t b, float gamma,
                          float* lr_out, void* stream);

/* mmvid_lr_plateau: torch's ReduceLROnPlateau(mode='min', threshold_mode='rel') (utils/utils_train.py:315-330, fed the loss at
 * train.py:373-374) as one device thread.  state_f = {lr, best} (fp32 [2]; best starts at +inf; state_f is what the Adam entries take
 * as lr_dev), state_i = {bad epochs, cool-down left, reductions} (int32 [3]), loss_dev an fp32 on the device.  Launched AFTER the
 * optimiser, *step_dev already advanced.  Returns at once where skip_dev != NULL and *skip_dev != 0 (the step was skipped) or where
 * (long)*step_dev % every != 0.  Otherwise, in fp32, each operation rounded once, in this order:
 *     if (loss < best * (1.f - threshold)) { best = loss; bad = 0; } else bad += 1;          NaN compares false: a bad epoch
 *     if (cool > 0) { cool -= 1; bad = 0; }
 *     if (bad > patience) { nw = fmaxf(lr * factor, min_lr); if (lr - nw > eps) { lr = nw; reductions += 1; } cool = cooldown; bad = 0; }
 * Multiplies, subtractions and comparisons only: tests/sched_ref.py replays it bit for bit.  Refused (nothing launched): a NULL
 * loss_dev, step_dev, state_f or state_i; a pointer that is not 4-byte aligned; every < 1; factor outside (0, 1); patience or
 * cooldown < 0; threshold outside [0, 1); min_lr or eps negative or not finite.  No atomics. */
int mmvid_lr_plateau(const float* loss_dev, const float* step_dev, int every, float factor, int patience, int cooldown, float threshold,
                     float min_lr, float eps, float* state_f, int32_t* state_i, const int32_t* skip_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
