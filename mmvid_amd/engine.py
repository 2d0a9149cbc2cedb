"""Training engine for the data-parallel hot path (train.py:28-35, 298-325 of the reference: DDP + clip_grad_norm_
+ Adam), MI355X-first:

  * every trainable parameter, its gradient and its Adam moments are slices of FLAT fp32 buffers (plus one flat
    bf16 shadow the MFMA kernels read), so the optimiser is one HIP launch over 125 M elements and the gradient
    exchange is a handful of large RCCL collectives instead of hundreds of per-tensor ones;
  * gradients are all-reduced (SUM; the 1/world factor is folded into the Adam kernel) in buckets on a side
    stream.  Buckets follow the order in which the hand-written backward FINISHES gradients -- heads and tower
    layers first, embedding tables last -- so the exchange of the big early buckets overlaps the rest of the
    backward.  xGMI is point-to-point: few, large messages keep every link busy.

One process per GPU; `torch.distributed` backend "nccl" is RCCL on ROCm, "gloo" in the CPU tests.
"""
import os

import torch
import torch.distributed as dist

from . import _lib, ops

ALIGN = 128  # elements: keeps every slice 16-B aligned for the vector kernels (fp32 and bf16)


def _round_up(x, m):
    return (x + m - 1) // m * m


class WarmupLR:
    """The reference's default schedule (utils_train.py:373-385 -> deepspeed.runtime.lr_schedules.WarmupLR; third-party,
    restated from its published semantics: parity unpinned): lr = min + (max - min) * gamma, gamma = log(k + 1) /
    log(warmup) for scheduler step k < warmup, else 1.  train.py:373-374 steps it after every `every`-th iteration;
    before its first step the optimiser runs at its construction lr.  `lr_at(i)` is the host view; the training step
    evaluates the same closed form on the device (mmvid_lr_schedule) so that a captured step follows it."""

    def __init__(self, warmup_min_lr=1e-6, warmup_max_lr=1e-4, warmup_num_steps=5000, every=1):
        self.min_lr, self.max_lr = float(warmup_min_lr), float(warmup_max_lr)
        self.warmup = max(2, int(warmup_num_steps))
        self.every = max(1, int(every))

    def lr_at(self, iteration):
        import math
        ns = iteration // self.every
        if ns == 0:
            return self.max_lr
        k = ns - 1
        gamma = math.log(k + 1) / math.log(self.warmup) if k < self.warmup else 1.0
        return self.min_lr + (self.max_lr - self.min_lr) * gamma


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f'{name}={v!r}: an int >= 1')
    return v


def _finite(name, v, lo=0.0):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) < float('inf'):  # (NaN: False)
        raise ValueError(f'{name}={v!r}: a finite number >= {lo}')
    return float(v)


class _ClosedFormLR:
    """A schedule mmvid_lr_schedule_ext evaluates from the device step count alone: no state, so a resumed or captured step follows
    it from the restored count.  ns = iteration // every scheduler steps have happened before `iteration` (train.py:373-374).
    `lr_at(i)` is the host view in fp64; `ext_args()` the (kind, lr_min, lr_max, every, a, b, gamma) of the device call."""

    def ns(self, iteration):
        return int(iteration) // self.every


class StepLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.StepLR(step_size, gamma) as the reference builds it (utils_train.py:332-343: gamma 0.5)."""

    def __init__(self, lr, step_size, gamma=0.5, every=1):
        self.lr, self.step_size, self.every = _finite('lr', lr), _positive_int('step_size', step_size), _positive_int('every', every)
        self.gamma = _finite('gamma', gamma)
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError(f'gamma={gamma!r}: in (0, 1]')

    def lr_at(self, iteration):
        return self.lr * self.gamma**(self.ns(iteration) // self.step_size)

    def ext_args(self):
        return ops.LR_STEP, 0.0, self.lr, self.every, self.step_size, 0, self.gamma


class CosineAnnealingLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.CosineAnnealingLR(T_max, eta_min) as the reference builds it (utils_train.py:345-356: eta_min 1e-6),
    in its closed form with the argument reduced in integers: r = ns mod 2 T_max, eta_min + (lr - eta_min) (1 + cos(pi r / T_max)) / 2.
    torch steps a recursion whose value drifts from this by rounding only (tests/test_sched_host.py)."""

    def __init__(self, lr, T_max, eta_min=1e-6, every=1):
        self.lr, self.T_max, self.every = _finite('lr', lr), _positive_int('T_max', T_max), _positive_int('every', every)
        self.eta_min = _finite('eta_min', eta_min)

    def lr_at(self, iteration):
        import math
        r = self.ns(iteration) % (2 * self.T_max)
        return self.eta_min + (self.lr - self.eta_min) * (1.0 + math.cos(math.pi * r / self.T_max)) / 2.0

    def ext_args(self):
        return ops.LR_COSINE, self.eta_min, self.lr, self.every, self.T_max, 0, 1.0


class WarmupDecayLR(_ClosedFormLR):
    """deepspeed.runtime.lr_schedules.WarmupDecayLR as the reference builds it (utils_train.py:358-371; third-party, restated from
    its published semantics: parity unpinned, as for WarmupLR): WarmupLR's logarithmic warm-up, then a linear decay that reaches
    warmup_min_lr at scheduler step total_num_steps, gamma = max(0, (total - k) / max(1, total - warmup)).  Before the first
    scheduler step the optimiser runs at its construction lr, warmup_max_lr."""

    def __init__(self, total_num_steps, warmup_min_lr=1e-6, warmup_max_lr=1e-4, warmup_num_steps=1000, every=1):
        self.min_lr, self.max_lr = _finite('warmup_min_lr', warmup_min_lr), _finite('warmup_max_lr', warmup_max_lr)
        self.warmup_arg = _positive_int('warmup_num_steps', warmup_num_steps)
        self.warmup = max(2, self.warmup_arg)
        self.total, self.every = _positive_int('total_num_steps', total_num_steps), _positive_int('every', every)
        if self.total < self.warmup_arg:
            raise ValueError(f'total_num_steps={total_num_steps} is below warmup_num_steps={warmup_num_steps}')

    def lr_at(self, iteration):
        import math
        ns = self.ns(iteration)
        if ns == 0:
            return self.max_lr
        k = ns - 1
        if k < self.warmup:
            gamma = math.log(k + 1) / math.log(self.warmup)
        else:
            gamma = max(0.0, (self.total - k) / max(1, self.total - self.warmup))
        return self.min_lr + (self.max_lr - self.min_lr) * gamma

    def ext_args(self):
        return ops.LR_WARMUP_DECAY, self.min_lr, self.max_lr, self.every, self.warmup_arg, self.total, 1.0


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel') as the reference builds it (utils_train.py:315-330:
    factor 0.5, patience 2, cooldown 5, min_lr 1e-6; threshold 1e-4 and eps 1e-8 are torch's defaults), fed the loss of every
    `every`-th iteration (train.py:373-374).  The trainer keeps its state on the device (mmvid_lr_plateau) and steps it from the loss
    tensor given to `FlatTrainer.step(loss=...)`; `replay(losses)` is the host view of the same fp32 rule."""
    STATE = ('lr', 'best', 'bad', 'cooldown', 'reductions')

    def __init__(self, lr, factor=0.5, patience=2, cooldown=5, min_lr=1e-6, threshold=1e-4, eps=1e-8, every=1):
        self.lr, self.min_lr, self.eps = _finite('lr', lr), _finite('min_lr', min_lr), _finite('eps', eps)
        self.factor, self.threshold = _finite('factor', factor), _finite('threshold', threshold)
        if not 0.0 < self.factor < 1.0:
            raise ValueError(f'factor={factor!r}: in (0, 1)')
        if not self.threshold < 1.0:
            raise ValueError(f'threshold={threshold!r}: in [0, 1)')
        for name, v in (('patience', patience), ('cooldown', cooldown)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f'{name}={v!r}: an int >= 0')
        self.patience, self.cooldown, self.every = patience, cooldown, _positive_int('every', every)

    def initial_state(self):
        """(state_f, state_i) as the device holds them before the first scheduler step."""
        return [self.lr, float('inf')], [0, 0, 0]

    def replay(self, losses, state=None):
        """The learning rate after each scheduler step fed `losses` in turn, from `state` (default: initial_state()), in the fp32
        arithmetic of the device -> (list of lr, final (state_f, state_i))."""
        import numpy as np
        f = np.float32
        sf, si = state if state is not None else self.initial_state()
        lr, best = f(sf[0]), f(sf[1])
        bad, cool, reductions = (int(x) for x in si)
        keep, out = f(1) - f(self.threshold), []
        with np.errstate(invalid='ignore', over='ignore'):
            for loss in losses:
                loss = f(loss)
                if loss < best * keep:
                    best, bad = loss, 0
                else:
                    bad += 1
                if cool > 0:
                    cool, bad = cool - 1, 0
                if bad > self.patience:
                    nw = max(lr * f(self.factor), f(self.min_lr))
                    if lr - nw > f(self.eps):
                        lr, reductions = nw, reductions + 1
                    cool, bad = self.cooldown, 0
                out.append(float(lr))
        return out, ([float(lr), float(best)], [bad, cool, reductions])


def lr_scheduler_from_args(name, learning_rate, iters=None, step_size=None, warmup=None, every=1):
    """The reference's prepare_lr_scheduler (utils_train.py:314-388) with its constants: `name` is --lr_scheduler, `learning_rate`
    --learning_rate, `iters` --iters, `step_size` --lr_scheduler_step_size, `warmup` --lr_scheduler_warmup, `every`
    --lr_scheduler_every.  -> the schedule object for FlatTrainer(lr_schedule=...)."""
    if name == 'reducelronplateau':
        return ReduceLROnPlateau(learning_rate, factor=0.5, patience=2, cooldown=5, min_lr=1e-6, every=every)
    if name == 'steplr':
        return StepLR(learning_rate, step_size, gamma=0.5, every=every)
    if name == 'cosineannealinglr':
        return CosineAnnealingLR(learning_rate, step_size, eta_min=1e-6, every=every)
    if name == 'warmupdecaylr':
        return WarmupDecayLR(iters, 1e-6, learning_rate, warmup, every=every)
    if name == 'warmuplr':
        return WarmupLR(1e-6, learning_rate, warmup, every=every)
    raise NotImplementedError(f'lr_scheduler {name!r}')


def optimizer_kwargs(name, weight_decay=0.0):
    """The reference's get_optimizer (utils_train.py:167-182) as FlatTrainer keywords: 'adam' is torch.optim.Adam with its default
    betas and L2 decay, 'adamw' torch.optim.AdamW with betas (0.9, 0.95) and decoupled decay."""
    if name == 'adam':
        return dict(betas=(0.9, 0.999), weight_decay=weight_decay, decoupled_weight_decay=False)
    if name == 'adamw':
        return dict(betas=(0.9, 0.95), weight_decay=weight_decay, decoupled_weight_decay=True)
    raise NotImplementedError(f'optimizer {name!r}')


PROVEN_TOWER_WIDTH = 768  # the widest tower whose captured / deterministic trainer step is covered by passing tests


def refuse_unproven_width(model, what):
    """A captured (GraphedStep) or deterministic-mode trainer step on a tower wider than 768 is refused: the one run of that
    combination (BERT(dim=1024), two captured deterministic-mode runs) ended in a GPU memory-access fault whose cause is not known.
    The training forward and backward, sampling and decoding at width 1024 are tested and stay available."""
    width = getattr(getattr(model, 'transformer', None), 'width', 0)
    if width > PROVEN_TOWER_WIDTH:
        raise NotImplementedError(f'{what} on a tower {width} wide: refused above width {PROVEN_TOWER_WIDTH} (this combination ended in a GPU '
                                  'memory-access fault at width 1024 and its cause is not known)')


def telemetry_group(name):
    """The group a parameter's telemetry falls into under `telemetry(by='layer')`: 'layer.<i>' for everything of tower layer i
    (`transformer.transformer.resblocks.<i>.*`), 'heads' for the output heads (`to_logits*`), 'tables' for the rest -- the embedding
    and positional tables.  The same three kinds as `backward_order`."""
    if name.startswith('transformer.transformer.resblocks.'):
        return f'layer.{int(name.split(".")[3])}'
    return 'heads' if name.startswith('to_logits') else 'tables'


class FlatTrainer:
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0,
                 process_group=None, bucket_mb=64, order=None, lr_schedule=None, force_exchange=False, sparse_tables=True,
                 lazy_rows=True, exchange=None, ema_decay=None, ema_warmup=False, skip_nonfinite=False,
                 telemetry_every=None, telemetry_slots=64, decoupled_weight_decay=False):
        self.model = model
        # AdamW and the schedules of --lr_scheduler (INTEGRATION.md "Optimiser and schedule flags"): False and a WarmupLR (or None) = the
        # launches and the state_dict() of a trainer built without these keywords
        if not isinstance(decoupled_weight_decay, bool):
            raise ValueError(f'decoupled_weight_decay={decoupled_weight_decay!r}: True or False')
        if isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float)) or not 0.0 <= float(weight_decay) < float('inf'):
            raise ValueError(f'weight_decay={weight_decay!r}: a finite number >= 0 (a negative decay grows the weights)')
        if decoupled_weight_decay and weight_decay != 0 and telemetry_every is not None:
            raise ValueError('decoupled_weight_decay=True with weight_decay != 0 and telemetry_every: the telemetry restates the update '
                             'from the moments Adam left (mmvid_segment_stats) and would miss the decay term p * lr * weight_decay')
        self.decoupled = decoupled_weight_decay
        if isinstance(lr_schedule, ReduceLROnPlateau):
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
                raise ValueError('a ReduceLROnPlateau schedule in a process group of more than one rank: the reference feeds each rank its '
                                 'own loss (train.py:327, 374), so the ranks\' learning rates drift apart; that is not reproduced')
            if any(p.requires_grad and p.device.type != 'cuda' for p in model.parameters()):
                raise ValueError('a ReduceLROnPlateau schedule on a host trainer: its state lives on the device and is stepped by a kernel')
        # trainer telemetry (INTEGRATION.md "Trainer telemetry"): None = off -- no buffer, no launch, state_dict() unchanged key for key
        for key, val in (('telemetry_every', telemetry_every), ('telemetry_slots', telemetry_slots)):
            if (val is not None or key == 'telemetry_slots') and (isinstance(val, bool) or not isinstance(val, int) or val < 1):
                raise ValueError(f'{key}={val!r}: an int >= 1' + (', or None for no telemetry' if key == 'telemetry_every' else ''))
        self.telemetry_every, self.telemetry_slots = telemetry_every, telemetry_slots
        # non-finite guard (INTEGRATION.md "Non-finite guard"): False = off -- no buffer, the unguarded step's launches, state_dict() unchanged
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f'skip_nonfinite={skip_nonfinite!r}: True or False')
        self.skip_nonfinite = skip_nonfinite
        # weight EMA (INTEGRATION.md "Weight EMA"): None = off -- no buffer, no launch, state_dict() unchanged key for key
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= float(ema_decay) < 1.0:  # (NaN, inf: False)
                raise ValueError(f'ema_decay={ema_decay!r}: a number in [0, 1), or None for no EMA')
        elif ema_warmup:
            raise ValueError('ema_warmup=True needs ema_decay')
        self.ema_decay, self.ema_warmup = (None if ema_decay is None else float(ema_decay)), bool(ema_warmup)
        # how a dense gradient message is summed over the ranks: 'allreduce' (one RCCL all-reduce: a ring, bound by ONE xGMI link
        # per hop) or 'direct' (every rank sends shard j of the message straight to rank j -- all_to_all over the 7
        # point-to-point links at once --, sums the shards it received in rank order, and the summed shards are all-gathered).
        # Same sums up to fp32 summation order; MMVID_EXCHANGE overrides.
        self.exchange = os.environ.get('MMVID_EXCHANGE', exchange or 'allreduce')
        assert self.exchange in ('allreduce', 'direct'), self.exchange
        self._direct_buf = None
        # row-wise exchange of the tables model.sparse_grad_rows() names (MMVID_SPARSE_TABLES=0 forces the dense all-reduce)
        self.sparse_tables = bool(sparse_tables) and os.environ.get('MMVID_SPARSE_TABLES', '1') != '0'
        self.lr_schedule = lr_schedule
        # force_exchange: run the all-reduce path even in a group of one (exercises RCCL + graph capture on a 1-GPU box)
        self.force_exchange = bool(force_exchange) and dist.is_available() and dist.is_initialized()
        self.exchange_enabled = True
        params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if order is not None:
            params = order(params)
        self.names = [n for n, _ in params]
        self.params = [p for _, p in params]
        dev = self.params[0].device
        offs, tot = [], 0
        for p in self.params:
            offs.append(tot)
            tot += _round_up(p.numel(), ALIGN)
        self.offsets, self.numel = offs, tot
        self.P = torch.zeros(tot, device=dev, dtype=torch.float32)
        self.G = torch.zeros(tot, device=dev, dtype=torch.float32)
        self.M = torch.zeros(tot, device=dev, dtype=torch.float32)
        self.V = torch.zeros(tot, device=dev, dtype=torch.float32)
        self.S = torch.zeros(tot, device=dev, dtype=torch.bfloat16) if dev.type == 'cuda' else None
        # E: the averaged weights, fp32 in the layout of P, primed (E <- P) by the first step() or the first reader; ES: their bf16
        # shadow, allocated by the first `with ema_weights():`
        self.E = torch.zeros(tot, device=dev, dtype=torch.float32) if self.ema_decay is not None else None
        self.ES, self._ema_primed, self._ema_scope = None, False, False
        self._index = {id(p): i for i, p in enumerate(self.params)}
        for i, p in enumerate(self.params):
            self._view(self.P, i).copy_(p.detach())
            p.data, p.grad = self._view(self.P, i), self._view(self.G, i)
        self._attached = []  # the shadow.Bf16Weights that read views of S (_attach_shadows)
        if self.S is not None:
            ops.cast_bf16(self.P, self.S)
            self._attach_shadows()
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.step_count = 0
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.bucket_elems = max(ALIGN, int(bucket_mb * (1 << 20) / 4) // ALIGN * ALIGN)
        self._sq = torch.zeros(1, device=dev, dtype=torch.float32)
        self._sq_partials = torch.zeros(2048, device=dev, dtype=torch.float32) if dev.type == 'cuda' else None
        # the step count also lives on the device, advanced by a device op: a captured step (GraphedStep) replays with
        # the right Adam bias corrections and learning rate without the host passing new scalars
        self._step_dev = torch.zeros(1, device=dev, dtype=torch.float32) if dev.type == 'cuda' else None
        self._lr_dev = torch.full((1, ), float(lr), device=dev, dtype=torch.float32) if dev.type == 'cuda' else None
        # the plateau schedule's device state (mmvid_lr_plateau): plateau_f = lr, best -- element 0 is the lr_dev Adam reads --,
        # plateau_i = bad epochs, cool-down left, reductions
        self.plateau_f = self.plateau_i = None
        if isinstance(lr_schedule, ReduceLROnPlateau):
            sf, si = lr_schedule.initial_state()
            self.plateau_f = torch.tensor(sf, dtype=torch.float32).to(dev)
            self.plateau_i = torch.tensor(si, dtype=torch.int32).to(dev)
        # the guard's device state (mmvid_step_guard): guard_i = verdict, steps skipped, current run of skips, steps seen;
        # guard_f = gradient norm of the last step, last finite gradient norm.  A host trainer has no optimiser kernel to guard.
        guarded = self.skip_nonfinite and dev.type == 'cuda'
        self.guard_i = torch.zeros(4, device=dev, dtype=torch.int32) if guarded else None
        self.guard_f = torch.zeros(2, device=dev, dtype=torch.float32) if guarded else None
        self._tel = None
        if telemetry_every is not None:
            if dev.type != 'cuda':
                raise ValueError('telemetry_every on a host trainer: it has no optimiser kernel to take the statistics after')
            self._init_telemetry(dev)
        self._comm_stream = torch.cuda.Stream(device=dev) if dev.type == 'cuda' else None
        self._works = []
        self._sent_from = tot  # gradients at flat offsets >= this are already on the wire this step
        # first flat offset of each tower layer (the flat order puts layers ascending, heads after, tables before)
        self._layer_start = {}
        for n, o in zip(self.names, offs):
            if n.startswith('transformer.transformer.resblocks.'):
                i = int(n.split('.')[3])
                self._layer_start[i] = min(o, self._layer_start.get(i, tot))
        tw = getattr(model, 'transformer', None)
        # (only when there is something to exchange: a chunked backward returns to the host every few layers, and a group of one
        # would pay for that -- the weight gradients of all layers could no longer go out as one launch per kind, csrc/tower.hip)
        if tw is not None and hasattr(tw, 'on_layers_done') and self._layer_start and (self.world > 1 or self.force_exchange):
            tw.on_layers_done = self.layers_done
        self._init_lazy_rows(lazy_rows and os.environ.get('MMVID_LAZY_ROWS', '1') != '0')

    # ------------------------------------------------------------------------------------------------ telemetry
    def _init_telemetry(self, dev):
        """The segment tables (one segment per parameter, uploaded once), the counter, the per-chunk partials and the ring of
        mmvid_segment_stats.  The ring is diagnostics, not state: it is in no checkpoint and a resumed trainer starts with an empty one."""
        off, ln, c0, chunks = ops.telemetry_plan(self.offsets, [p.numel() for p in self.params])
        S, slots = len(off), self.telemetry_slots
        i32 = dict(device=dev, dtype=torch.int32)
        self._tel = {'tables': tuple(torch.tensor(t, dtype=torch.int64).to(dev) for t in (off, ln, c0)), 'chunks': chunks,
                     'count': torch.zeros(1, **i32), 'partials_f': torch.zeros(chunks * 4, device=dev), 'partials_i': torch.zeros(chunks * 2, **i32),
                     'ring_f': torch.zeros(slots * S * 4, device=dev), 'ring_i': torch.zeros(slots * S * 2, **i32),
                     'head_i': torch.zeros(slots * 4, **i32), 'head_f': torch.zeros(slots * 2, device=dev)}

    def _telemetry_read(self):
        """Every valid record of the ring, oldest first, as (head_i [4], head_f [2], ring_f [S, 4], ring_i [S, 2]) of host tensors -- one
        device read.  It touches the ring only, nothing `ema_weights()` re-points: allowed inside that scope."""
        t = self._tel
        if t is None:
            raise RuntimeError('this trainer takes no telemetry (telemetry_every=None)')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('telemetry is read inside a stream capture: it reads the device')
        S, slots = len(self.names), self.telemetry_slots
        raw = torch.cat([t['head_i'], t['head_f'].view(torch.int32), t['ring_f'].view(torch.int32), t['ring_i']]).cpu()
        hi, hf = raw[:slots * 4].view(slots, 4), raw[slots * 4:slots * 6].view(torch.float32).view(slots, 2)
        rf = raw[slots * 6:slots * 6 + slots * S * 4].view(torch.float32).view(slots, S, 4)
        ri = raw[slots * 6 + slots * S * 4:].view(slots, S, 2)
        valid = sorted((int(hi[k, 0]), k) for k in range(slots) if int(hi[k, 3]) == 1)
        return [(hi[k], hf[k], rf[k], ri[k]) for _, k in valid]

    def telemetry(self, last=None, by='param'):
        """The telemetry records the ring holds, oldest first (at most the `last` newest), in one device read (it synchronises).  A
        record: 'record' (the number of the step() call, from 0), 'step' (applied optimiser steps, that one included), 'skipped' (the
        non-finite guard's verdict), 'lr', 'grad_norm' (sqrt of the sum over the FINITE gradient elements, / world: what
        guard_stats()['grad_norm'] reports for a step it did not skip) and 'params': name -> 'grad_norm', 'grad_absmax' (both / world),
        'grad_nonfinite', 'weight_norm', 'update_norm' (0 on a skipped step) and 'update_ratio' = update_norm / weight_norm.  by='layer'
        merges the parameters by `telemetry_group` (squares summed, maxima taken, counts added).  Roots, the 1 / world scaling and the
        ratio are taken in fp64 on the host."""
        if by not in ('param', 'layer'):
            raise ValueError(f"by={by!r}: 'param' or 'layer'")
        if last is not None and (isinstance(last, bool) or not isinstance(last, int) or last < 1):
            raise ValueError(f'last={last!r}: an int >= 1, or None for every record')
        recs = self._telemetry_read()
        out = []
        for hi, hf, rf, ri in (recs if last is None else recs[-last:]):
            rf, ri = rf.double(), ri.tolist()
            merged = {}
            for s, name in enumerate(self.names):
                key = name if by == 'param' else telemetry_group(name)
                a = merged.setdefault(key, [0.0, 0.0, 0.0, 0.0, 0])
                a[0] += float(rf[s, 0]); a[1] = max(a[1], float(rf[s, 1])); a[2] += float(rf[s, 2]); a[3] += float(rf[s, 3]); a[4] += ri[s][0]
            params = {}
            for key, (gsq, gmax, psq, dsq, bad) in merged.items():
                wn, un = psq**0.5, dsq**0.5
                params[key] = {'grad_norm': gsq**0.5 / self.world, 'grad_absmax': gmax / self.world, 'grad_nonfinite': bad,
                               'weight_norm': wn, 'update_norm': un, 'update_ratio': un / wn if wn > 0 else float('nan')}
            out.append({'record': int(hi[0]), 'step': int(hi[1]), 'skipped': bool(int(hi[2])), 'lr': float(hf[0]),
                        'grad_norm': float(hf[1].double())**0.5 / self.world, 'params': params})
        return out

    def first_nonfinite(self):
        """The names of the parameters, in flat order, whose gradient held a NaN or an inf at the newest record; [] if none did (or no
        record was taken yet)."""
        recs = self._telemetry_read()
        if not recs:
            return []
        bad = recs[-1][3][:, 0].tolist()
        return [n for n, b in zip(self.names, bad) if b > 0]

    # ------------------------------------------------------------------------------------------ lazy table rows
    def _init_lazy_rows(self, enabled):
        """The table `model.sparse_grad_rows()` names (BERT: text_emb, 49,472 x 768 = 30 % of the parameters) gets a flag per row
        "has ever received a gradient".  Rows that never did have g = m = v = 0: Adam (no weight decay) and the gradient norm skip
        them exactly (csrc/optim.hip), and zero_grad() only clears the rows the last step touched.  The flags follow the ids the
        model logs per forward (and, under data parallelism, the ids every rank sent); anything the trainer cannot account for
        -- an overflowed log, a gradient accumulated outside the flat buffer, a loaded optimiser state -- raises the flags."""
        self._lazy = None
        fn = getattr(self.model, 'sparse_grad_rows', None)
        if not enabled or fn is None or self.S is None or self.wd != 0.0:
            return
        names = [n for n in fn() if n in self.names]
        if len(names) != 1:
            return
        i = self.names.index(names[0])
        p = self.params[i]
        if p.dim() != 2 or p.shape[1] % 4 != 0:
            return
        dev = p.device
        self._lazy = {'name': names[0], 'lo': self.offsets[i], 'rows': p.shape[0], 'rowlen': p.shape[1],
                      'flags': torch.zeros(p.shape[0], device=dev, dtype=torch.uint8),
                      'dirty': None, 'dirty_n': 0, 'all_dirty': True}  # rows whose gradient is non-zero right now

    def _lazy_arg(self):
        z = self._lazy
        return None if z is None else (z['flags'], z['lo'], z['rows'], z['rowlen'])

    def _lazy_mark(self, ids):
        """Rows `ids` (int64, any shape; -1 = blank) carry a gradient this step.  ids None: unknown -> every row from now on."""
        z = self._lazy
        if z is None:
            return
        if ids is None:
            z['flags'].fill_(1)
            z['all_dirty'] = True
            return
        ids = ids.reshape(-1).clamp_min(0)
        z['flags'].index_fill_(0, ids, 1)
        if z['all_dirty']:
            return
        n = ids.numel()
        if z['dirty'] is None or z['dirty_n'] + n > z['dirty'].numel():
            if z['dirty'] is not None and z['dirty_n'] > 0 or torch.cuda.is_current_stream_capturing():
                z['all_dirty'] = True  # no room (and no allocation inside a capture): the next zero_grad clears the whole table
                return
            z['dirty'] = torch.zeros(max(4 * n, 1024), device=ids.device, dtype=torch.int64)
            z['dirty_n'] = 0
        z['dirty'][z['dirty_n']:z['dirty_n'] + n].copy_(ids)
        z['dirty_n'] += n

    def _view(self, flat, i):
        """Parameter i's view, in its own shape, of a flat buffer laid out like P."""
        o, p = self.offsets[i], self.params[i]
        return flat[o:o + p.numel()].view(p.shape)

    def _shadow_view(self, p, S=None):
        return self._view(self.S if S is None else S, self._index[id(p)])

    def _attach_shadows(self, S=None):
        """Every weight the MFMA kernels read in bf16 is a shadow.Bf16Weight, listed by the `bf16_weights()` of the module that owns
        it (the tower: its matrices; BERT / ART-V: their heads).  One whose parameter lives in the flat buffer is handed its view of
        the flat bf16 shadow, which step() keeps current; every other one (frozen) is told to cast again for itself.  S: the flat bf16
        buffer the views are taken from (default self.S; `ema_weights()` passes the shadow of the averaged weights).  An attachment
        records the parameter's data_ptr, so the parameters must already point where they will be read from.  The walk is over
        `model.modules()`: a model that only holds a tower (no `bf16_weights()` of its own) is served, and so is every tower
        registered anywhere below the model, not only `model.transformer`."""
        self._attached, self._tower_shadow_attached = [], False
        for mod in self.model.modules():
            for w in getattr(mod, 'bf16_weights', list)():
                if id(w.param) in self._index:
                    w.attach(self._shadow_view(w.param, S))
                    self._attached.append(w)
                    self._tower_shadow_attached |= mod is getattr(self.model, 'transformer', None)  # (read by bench.py)
                else:
                    w.invalidate()

    def _check_bindings(self):
        """`p.data` / `p.grad` must still be the views into P / G the kernels update: `model.zero_grad()` (set_to_none),
        `load_state_dict(assign=True)` or `.to()` would silently detach them.  Re-bind gradients, refuse moved params."""
        if self._ema_scope:
            raise RuntimeError('the model reads the averaged weights (inside `with trainer.ema_weights():`): leave the scope first')
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if p.data_ptr() != self.P.data_ptr() + 4 * o:
                raise RuntimeError('a parameter no longer lives in FlatTrainer.P (moved by .to() / load_state_dict(assign=True)); '
                                   'rebuild the trainer after moving the model')
            if p.grad is None or p.grad.data_ptr() != self.G.data_ptr() + 4 * o:
                stray = p.grad
                p.grad = self._view(self.G, i)
                if stray is not None:  # gradients were accumulated into a detached tensor this step: fold them in
                    p.grad.add_(stray)
                    if self._lazy is not None and o == self._lazy['lo']:
                        self._lazy_mark(None)  # rows the id log does not know about (every flag up: the EMA sweeps the table too)

    # --------------------------------------------------------------------------------------------- checkpoint
    def state_dict(self):
        """Optimiser state in torch.optim.Adam's layout (train.py:202-203, 352, 387 save / restore `optimizer`): per
        parameter exp_avg / exp_avg_sq / step, keyed by position in `self.names` order (recorded under 'names'), plus the
        front-end's (seed, forward count) so a resumed run continues its mask / warp stream instead of replaying it.  With the
        non-finite guard the step count is first reconciled with the device (guard_stats): 'step' is the number of APPLIED steps."""
        guard = self.guard_stats() if self.guard_i is not None else None
        state = {}
        for i in range(len(self.params)):
            state[i] = {'step': torch.tensor(float(self.step_count)), 'exp_avg': self._view(self.M, i).clone(),
                        'exp_avg_sq': self._view(self.V, i).clone()}
        group = {'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.wd, 'amsgrad': False,
                 'params': list(range(len(self.params)))}
        if self.decoupled:  # (the key torch.optim.AdamW's own state_dict() carries: a reference `adamw` checkpoint has it too)
            group['decoupled_weight_decay'] = True
        out = {'state': state, 'param_groups': [group], 'names': list(self.names)}
        if self.plateau_f is not None:  # (one device read each; the closed-form schedules follow the step count and keep no state)
            out['lr_plateau'] = dict(zip(ReduceLROnPlateau.STATE, self.plateau_f.tolist() + self.plateau_i.tolist()))
        fe = getattr(self.model, 'frontend', None)
        if fe is not None and hasattr(fe, 'state_dict'):
            out['frontend'] = fe.state_dict()
        if self.E is not None:
            out['ema'] = {'decay': self.ema_decay, 'warmup': self.ema_warmup, 'weights': self.ema_state_dict()}
        if guard is not None:
            out['guard'] = {'skipped': guard['skipped'], 'seen': guard['seen']}
        return out

    def load_state_dict(self, sd):
        """Accepts this class's own state_dict and a plain torch.optim.Adam one (the reference's checkpoints,
        train.py:352): without a 'names' entry the indices are torch's -- position in the requires_grad-filtered
        `model.parameters()` order the reference hands to Adam (utils_train.py:167-172) -- and are mapped through the
        parameter names to the flat layout; every entry's shape is checked, so moments can never land on another layer."""
        saved_decoupled = bool(sd['param_groups'][0].get('decoupled_weight_decay', False))
        if saved_decoupled != self.decoupled:
            raise ValueError(f'the optimiser state was saved with decoupled_weight_decay={saved_decoupled} (AdamW: True, Adam: False) and '
                             f'this trainer was built with decoupled_weight_decay={self.decoupled}: the moments would be stepped by the other rule')
        if 'names' in sd:
            names = list(sd['names'])
        else:
            names = [n for n, p in self.model.named_parameters() if p.requires_grad]
        if sorted(names) != sorted(self.names):
            raise ValueError('optimizer state was saved for a different set of parameters: '
                             f'{sorted(set(names) ^ set(self.names))[:6]} ...')
        at = {n: i for i, n in enumerate(self.names)}
        steps, loaded = set(), []
        for j, name in enumerate(names):
            st = sd['state'].get(j, sd['state'].get(str(j)))
            if st is None:
                continue
            i = at[name]
            p, o, n = self.params[i], self.offsets[i], self.params[i].numel()
            for k in ('exp_avg', 'exp_avg_sq'):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f'optimizer state entry {j} ({name}): {k} has shape {tuple(st[k].shape)}, the parameter '
                                     f'{tuple(p.shape)}')
            loaded.append((o, n, st))
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('per-parameter step counts differ')
        ema = sd.get('ema') if self.E is not None else None  # (an 'ema' entry given to a trainer without EMA is ignored)
        if ema is not None:
            w = ema['weights']
            if sorted(w) != sorted(self.names):
                raise ValueError(f'EMA weights were saved for a different set of parameters: {sorted(set(w) ^ set(self.names))[:6]} ...')
            for name, p in zip(self.names, self.params):
                if tuple(w[name].shape) != tuple(p.shape):
                    raise ValueError(f'EMA weights entry {name}: shape {tuple(w[name].shape)}, the parameter {tuple(p.shape)}')
        for o, n, st in loaded:
            self.M[o:o + n].copy_(st['exp_avg'].reshape(-1))
            self.V[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
        if steps:
            self.step_count = steps.pop()
            if self._step_dev is not None:
                self._step_dev.fill_(float(self.step_count))
        if self.guard_i is not None:  # the two totals as saved (none saved: zero); the run of skips starts again
            saved = sd.get('guard') or {}
            self.guard_i.copy_(torch.tensor([0, int(saved.get('skipped', 0)), 0, int(saved.get('seen', 0))], dtype=torch.int32))
            self.guard_f.zero_()
        if self._tel is not None:  # the ring is diagnostics, not state: a resumed trainer starts with an empty one
            self._tel['head_i'].zero_()
            self._tel['count'].zero_()
        if self.plateau_f is not None:  # the five values as saved; none saved: the schedule starts again
            saved = sd.get('lr_plateau')
            sf, si = self.lr_schedule.initial_state()
            if saved is not None:
                sf, si = [saved['lr'], saved['best']], [saved['bad'], saved['cooldown'], saved['reductions']]
            self.plateau_f.copy_(torch.tensor(sf, dtype=torch.float32))
            self.plateau_i.copy_(torch.tensor([int(x) for x in si], dtype=torch.int32))
        g = sd['param_groups'][0]
        self.lr, self.betas, self.eps, self.wd = g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']
        fe = getattr(self.model, 'frontend', None)
        if fe is not None and 'frontend' in sd and hasattr(fe, 'load_state_dict'):
            fe.load_state_dict(sd['frontend'])
        z = getattr(self, '_lazy', None)
        if z is not None:  # rows with loaded moments must keep decaying
            lo, hi = z['lo'], z['lo'] + z['rows'] * z['rowlen']
            live = (self.M[lo:hi].view(z['rows'], -1).abs().amax(1) > 0) | (self.V[lo:hi].view(z['rows'], -1).amax(1) > 0)
            z['flags'].copy_(live.to(torch.uint8) | z['flags'])
        if ema is not None:  # the averaged weights as saved; the decay and the warm-up stay the constructor's
            for i, name in enumerate(self.names):
                self._view(self.E, i).copy_(ema['weights'][name])
            self._ema_primed = True
            self._ema_flag_rows()
        elif self.E is not None:  # a checkpoint without averaged weights: E is primed again from the weights as they stand
            self.ema_reset()

    def refresh_shadows(self):
        """Call after writing parameters behind the trainer's back (model.load_state_dict): re-cast the bf16 shadow."""
        if self._ema_scope:
            raise RuntimeError('refresh_shadows() inside `with trainer.ema_weights():`: leave the scope first')
        if self.S is not None:
            ops.cast_bf16(self.P, self.S)
            self._attach_shadows()
        self._ema_flag_rows()

    # ------------------------------------------------------------------------------------------------ weight EMA
    def ema_decay_at(self, t):
        """The decay the device applies at the t-th optimiser step (t >= 1 counts finished steps, that one included), as the fp32
        value: d = min(decay, (1 + t) / (10 + t)) with ema_warmup, else decay -- each operation one fp32 operation (csrc/ema.hip)."""
        if self.E is None:
            raise RuntimeError('this trainer keeps no EMA (ema_decay=None)')
        d = torch.tensor(self.ema_decay, dtype=torch.float32)
        if self.ema_warmup:
            t32 = torch.tensor(float(t), dtype=torch.float32)
            one, ten = torch.tensor(1.0, dtype=torch.float32), torch.tensor(10.0, dtype=torch.float32)
            d = torch.minimum(d, (one + t32) / (ten + t32))
        return float(d)

    def _ema_prime(self):
        """E <- P, once: at the first step() (before Adam) or the first reader of E, whichever comes first -- so whatever rewrote the
        weights before training started (broadcast_parameters, model.load_state_dict + refresh_shadows) is in E without a call."""
        if self.E is None:
            raise RuntimeError('this trainer keeps no EMA (ema_decay=None)')
        if not self._ema_primed:
            if self.E.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the EMA would be primed inside a stream capture; GraphedStep primes it before it captures')
            self.E.copy_(self.P)
            self._ema_primed = True

    def ema_reset(self):
        """Forget the average: the next step() (or reader) primes E from the weights as they stand then."""
        if self.E is None:
            raise RuntimeError('this trainer keeps no EMA (ema_decay=None)')
        if self._ema_scope:
            raise RuntimeError('ema_reset() inside `with trainer.ema_weights():`: leave the scope first')
        self._ema_primed = False

    def _ema_flag_rows(self):
        """The EMA kernel skips the unflagged rows of the lazy table, which is exact while E == P there, bit for bit.  After P or E
        was written outside step() (refresh_shadows, load_state_dict): raise the flag of every row that holds a difference.  A raised
        flag is always safe: Adam leaves a row without gradient and moments as it is."""
        z = self._lazy
        if self.E is None or not self._ema_primed or z is None:
            return
        lo, hi = z['lo'], z['lo'] + z['rows'] * z['rowlen']
        differ = (self.E[lo:hi].view(torch.int32) != self.P[lo:hi].view(torch.int32)).view(z['rows'], -1).any(1)
        z['flags'].copy_(differ.to(torch.uint8) | z['flags'])

    def ema_state_dict(self):
        """{name: tensor} of the trainable parameters, taken from E (clones, parameter shapes): what
        `other_model.load_state_dict(..., strict=False)` takes to run another copy of the model on the averaged weights."""
        self._ema_prime()
        return {n: self._view(self.E, i).clone() for i, n in enumerate(self.names)}

    def ema_weights(self):
        """`with trainer.ema_weights():` -- the model runs on the averaged weights inside the block (sampling, evaluation) and on the
        trained ones after it.  Entry points every flat parameter's `.data` at its view of E, casts E into its bf16 shadow ES (on
        EVERY entry: the bf16 copies can never be older than E) and hands the tower and the heads views of ES; exit puts the views
        of P and S back.  `p.grad` keeps pointing into G.  Frozen weights are not touched.  Inside the block step(), zero_grad(),
        refresh_shadows(), a GraphedStep call and a second scope raise: they would train P while the model reads E."""
        return _EmaScope(self)

    # ---------------------------------------------------------------------------------------------
    def zero_grad(self):
        if self._ema_scope:
            raise RuntimeError('zero_grad() inside `with trainer.ema_weights():`: the model reads the averaged weights; leave the scope first')
        z = self._lazy
        if z is not None:
            # Table rows a backward wrote that no step() recorded as dirty (a step skipped on a non-finite loss; a backward whose forward
            # ran before the previous zero_grad()) must not survive as stale rows behind unflagged rows: the model raises
            # `table_grad_pending` from a hook on the backward itself and step() lowers it once the rows are recorded, so a raised flag
            # here means "unaccounted rows" -> clear the whole table.  Two zero_grad() calls in a row raise nothing (no 152-MB fill).
            # A model without the flag: any zero_grad() that does not follow a step() clears the whole table.
            pending = getattr(self.model, 'table_grad_pending', None)
            if pending is None:
                pending = not getattr(self, '_stepped_since_zero', True)
            if pending or getattr(self.model, '_text_id_overflow', False):
                z['all_dirty'] = True
        self._stepped_since_zero = False
        if z is None or z['all_dirty']:
            self.G.zero_()
        else:  # everything but the lazy table, and of the table only the rows the last step left a gradient in
            lo, hi = z['lo'], z['lo'] + z['rows'] * z['rowlen']
            self.G[:lo].zero_()
            self.G[hi:].zero_()
            if z['dirty_n']:
                self.G[lo:hi].view(z['rows'], z['rowlen']).index_fill_(0, z['dirty'][:z['dirty_n']], 0.0)
        if z is not None:
            z['all_dirty'], z['dirty_n'] = False, 0
            if hasattr(self.model, 'table_grad_pending'):
                self.model.table_grad_pending = False
        reset = getattr(self.model, 'reset_sparse_grad_rows', None)
        if reset is not None:
            reset()

    def _sparse_ranges(self):
        """Flat ranges of the tables whose gradient is exchanged row-wise (see _exchange_sparse): excluded from the all-reduce."""
        fn = getattr(self.model, 'sparse_grad_rows', None)
        if not self.sparse_tables or fn is None:
            return []
        out = []
        for name, ids in fn().items():
            # ids None = the model has no (complete) list of the rows this step touched -- no forward logged yet, or its
            # log overflowed under gradient accumulation: that table goes through the dense all-reduce like any other
            if name in self.names and ids is not None:
                i = self.names.index(name)
                out.append((self.offsets[i], self.offsets[i] + _round_up(self.params[i].numel(), ALIGN)))
        return sorted(out)

    def _send(self, lo, hi):
        """All-reduce G[lo:hi] (SUM) on the side stream, in messages of at most bucket_elems."""
        if (self.world == 1 and not self.force_exchange) or hi <= lo or not self.exchange_enabled:
            return
        pieces, at = [], lo
        for a, b in self._sparse_ranges():  # cut the row-wise exchanged tables out of [lo, hi)
            if b <= at or a >= hi:
                continue
            if a > at:
                pieces.append((at, a))
            at = max(at, b)
        if at < hi:
            pieces.append((at, hi))
        if self._comm_stream is not None:
            self._comm_stream.wait_stream(torch.cuda.current_stream())
        for plo, phi in pieces:
            for s in range(plo, phi, self.bucket_elems):
                e = min(s + self.bucket_elems, phi)
                if self._comm_stream is not None:
                    with torch.cuda.stream(self._comm_stream):
                        self._reduce_message(s, e)
                else:
                    self._reduce_message(s, e)

    def _reduce_message(self, s, e):
        """G[s:e] <- sum over ranks (on the current stream)."""
        if self.exchange == 'allreduce' or self.world == 1 or (e - s) % self.world != 0:  # (a group of one has no peers to send shards to)
            self._works.append(dist.all_reduce(self.G[s:e], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
            return
        # direct reduce-scatter + all-gather: fixed buffers (capturable), every peer link busy at once
        n, w = e - s, self.world
        if self._direct_buf is None or self._direct_buf.numel() < n + n // w:
            self._direct_buf = torch.empty(self.bucket_elems + self.bucket_elems // w + w, device=self.G.device, dtype=torch.float32)
        recv = self._direct_buf[:n].view(w, n // w)
        shard = self._direct_buf[n:n + n // w]
        msg = self.G[s:e]
        nccl = dist.get_backend(self.pg) == 'nccl'
        if nccl:
            dist.all_to_all_single(recv.view(-1), msg, group=self.pg)
        else:  # gloo (CPU tests) has no all_to_all: the same exchange as point-to-point sends
            me, parts = self._rank(), msg.view(w, n // w)
            recv[me].copy_(parts[me])
            reqs = [dist.P2POp(dist.isend, parts[j].contiguous(), j, self.pg) for j in range(w) if j != me] + \
                   [dist.P2POp(dist.irecv, recv[j], j, self.pg) for j in range(w) if j != me]
            for r in dist.batch_isend_irecv(reqs):
                r.wait()
        torch.sum(recv, dim=0, out=shard)  # rank order: the same bits on every rank
        if nccl:
            dist.all_gather_into_tensor(msg, shard, group=self.pg)
        else:
            dist.all_gather(list(msg.view(w, n // w).unbind(0)), shard, group=self.pg)

    def _gather(self, t):
        """[n, ...] on every rank -> [world * n, ...] (rank-major)."""
        out = torch.empty((self.world * t.shape[0], ) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        if dist.get_backend(self.pg) == 'nccl':
            dist.all_gather_into_tensor(out, t, group=self.pg)
        else:
            dist.all_gather(list(out.chunk(self.world, 0)), t, group=self.pg)
        return out

    def _exchange_sparse(self):
        """Row-wise gradient exchange of the tables `model.sparse_grad_rows()` names (BERT: the 49,472 x 768 text embedding,
        152 MB dense, of which a step touches at most B * 64 rows).  The table is the LAST gradient of the backward, so its
        dense all-reduce cannot overlap anything: instead every rank gathers (row id, gradient row) of the rows ITS batch
        touched -- ids sorted, repeats blanked, fixed shapes, so the step stays capturable -- and adds the other ranks' rows
        to its own table gradient: the same sum, ~1 MB per rank on the wire instead of 152 MB."""
        fn = getattr(self.model, 'sparse_grad_rows', None)
        if not self.sparse_tables or fn is None or not self.exchange_enabled:
            return
        rank = self._rank()
        for name, ids in fn().items():
            if name not in self.names or ids is None:
                continue  # None: the table was not cut out of the dense all-reduce (_sparse_ranges)
            W = self.params[self.names.index(name)].grad  # [V, E] view into G
            uid, rows = self.pack_rows(W, ids)
            all_ids = self._gather(uid)
            self.merge_rows(W, all_ids, self._gather(rows), rank, uid.shape[0])
            if self._lazy is not None and self._lazy['name'] == name:
                self._lazy_mark(all_ids)  # the other ranks' rows now carry a gradient here too

    def _rank(self):
        return dist.get_rank(self.pg)

    @staticmethod
    def pack_rows(W, ids):
        """This rank's message: (ids sorted, repeats blanked to -1) and the matching gradient rows (zero where blanked)."""
        ids = ids.reshape(-1)
        if W.is_cuda and ids.numel() <= 4096 and W.dtype == torch.float32 and W.is_contiguous():  # two launches, no allocator traffic beyond the outputs
            uid = torch.empty_like(ids)
            rows = torch.empty(ids.numel(), W.shape[1], device=W.device, dtype=W.dtype)
            _lib.call('mmvid_rows_pack', ops._p(W), W.shape[0], W.shape[1], ops._p(ids.contiguous()), ids.numel(), ops._p(uid), ops._p(rows),
                      ops._stream())
            return uid, rows
        srt, _ = torch.sort(ids)
        first = torch.ones_like(srt, dtype=torch.bool)
        first[1:] = srt[1:] != srt[:-1]
        uid = torch.where(first, srt, torch.full_like(srt, -1))
        rows = W.index_select(0, srt) * first.unsqueeze(1).to(W.dtype)
        return uid, rows

    @staticmethod
    def merge_rows(W, all_ids, all_rows, rank, n):
        """Add every OTHER rank's rows (rank-major gathered messages of n rows each) to this rank's table gradient."""
        if W.is_cuda and W.dtype == torch.float32 and W.is_contiguous():  # one launch per peer, in rank order: a fixed summation order
            for r in range(all_ids.shape[0] // n):
                if r != rank:
                    _lib.call('mmvid_rows_merge', ops._p(W), W.shape[0], W.shape[1], ops._p(all_ids[r * n:(r + 1) * n]),
                              ops._p(all_rows[r * n:(r + 1) * n]), n, ops._stream())
            return
        own = torch.zeros(all_ids.shape[0], dtype=torch.bool, device=all_ids.device)
        own[rank * n:(rank + 1) * n] = True
        valid = (all_ids >= 0) & ~own
        W.index_add_(0, all_ids.clamp_min(0), all_rows * valid.unsqueeze(1).to(W.dtype))

    def layers_done(self, first_layer):
        """Tower backward callback: gradients of layers >= first_layer (and everything after them in the flat
        buffer: later layers, heads) are final -> put them on the wire while the backward continues."""
        lo = self._layer_start.get(first_layer)
        if lo is None or lo >= self._sent_from:
            return
        self._send(lo, self._sent_from)
        self._sent_from = lo

    def after_failed_capture(self):
        """A step that was being captured raised (e.g. a collective the runtime cannot capture).  The communication stream joined that
        capture through an event and HIP leaves it in capture mode when the origin's capture is torn down: every later launch on it fails
        with 'operation not permitted when stream is capturing'.  Take a fresh stream and forget the half-finished exchange."""
        if self._comm_stream is not None:
            self._comm_stream = torch.cuda.Stream(device=self.G.device)
        self._works = []
        self._sent_from = self.numel

    def allreduce_grads(self):
        """Send whatever is still local (embedding tables, or everything when no callback fired) and wait."""
        if self.world > 1 or self.force_exchange:
            self._send(0, self._sent_from)
            if self._comm_stream is not None:
                with torch.cuda.stream(self._comm_stream):  # after the dense messages, on the same stream
                    self._exchange_sparse()
            else:
                self._exchange_sparse()
            for w in self._works:
                w.wait()
            self._works = []
            if self._comm_stream is not None:
                torch.cuda.current_stream().wait_stream(self._comm_stream)
        self._sent_from = self.numel

    def step(self, loss=None):
        """clip_grad_norm_(max_norm) + Adam (train.py:324-325) on the averaged gradients.  loss: what a ReduceLROnPlateau schedule is
        stepped with (train.py:373-374) -- a one-element fp32 tensor on the trainer's device, read by the device; no other schedule
        looks at it."""
        if self._ema_scope:
            raise RuntimeError('step() inside `with trainer.ema_weights():`: the model reads the averaged weights; leave the scope first')
        if self.plateau_f is not None:
            if not (isinstance(loss, torch.Tensor) and loss.numel() == 1 and loss.dtype == torch.float32 and loss.device == self.P.device
                    and loss.is_contiguous()):
                raise ValueError('a ReduceLROnPlateau schedule needs step(loss=...): a one-element fp32 tensor on the trainer\'s device '
                                 '(the device steps the schedule from it), got '
                                 f'{(loss.dtype, loss.device, tuple(loss.shape)) if isinstance(loss, torch.Tensor) else repr(loss)}')
            loss = loss.detach()
        if _lib.is_deterministic():
            refuse_unproven_width(self.model, 'a deterministic-mode trainer step')
        self._check_bindings()
        if self.E is not None:
            self._ema_prime()  # (before Adam: the average starts from the weights this step starts from)
        self.allreduce_grads()
        if self._lazy is not None:
            ids = self.model.sparse_grad_rows().get(self._lazy['name'])
            # a multi-rank step whose table went through the DENSE all-reduce (sparse_tables off) carries the other ranks' rows
            # too, and this rank's id log does not know them: every row counts from now on
            dense_exchange = (self.world > 1 or self.force_exchange) and self.exchange_enabled and not self.sparse_tables
            self._lazy_mark(None if dense_exchange else ids)
            if hasattr(self.model, 'table_grad_pending'):
                self.model.table_grad_pending = False  # (the rows are now recorded as dirty)
        self._stepped_since_zero = True
        self.step_count += 1
        gscale = 1.0 / self.world
        # the update itself is the HIP kernel; on a host tensor ops.adam_step raises (there is no CPU path)
        self._sq.zero_()
        lr_dev = None
        if self._step_dev is not None:
            sc = self.lr_schedule
            if self.plateau_f is not None:  # the rate the last scheduler step left; this iteration's scheduler step follows Adam
                lr_dev = self.plateau_f
            elif isinstance(sc, _ClosedFormLR):
                kind, lo, hi, every, a, b, gamma = sc.ext_args()
                ops.lr_schedule_ext(self._step_dev, kind, lo, hi, every, a, b, gamma, self._lr_dev)
                lr_dev = self._lr_dev
            elif sc is not None:  # lr of THIS iteration from the count of finished steps, on the device
                ops.lr_schedule(self._step_dev, 1, sc.min_lr, sc.max_lr, sc.warmup, sc.every, self._lr_dev)
                lr_dev = self._lr_dev
            if self.guard_i is None:
                ops.counter_add(self._step_dev, 1.0)
        # what Adam and the kernels after it on the stream read alike: the device's step count, the lazy rows, the guard's verdict
        # (element 0 of guard_i; None: unguarded)
        state = dict(step_dev=self._step_dev, lazy=self._lazy_arg(), skip_dev=self.guard_i)
        ops.grad_sqnorm(self.G, self._sq, partials=self._sq_partials, lazy=state['lazy'])
        if self.guard_i is not None:
            # the verdict on the exchanged gradient, on the device: step_guard advances the step count in counter_add's place (only
            # where the step is applied) and Adam and the EMA return at once where it says skip -- no host input, so a replay obeys it
            ops.step_guard(self._sq, gscale, self._step_dev, self.guard_i, self.guard_f)
        ops.adam_step(self.P, self.G, self.M, self.V, self.S, self.step_count, self.lr, self.betas, self.eps, self.wd,
                      self.max_norm, self._sq, gscale, lr_dev=lr_dev, decoupled=self.decoupled, **state)
        if self._tel is not None:  # after Adam; it only reads
            t = self._tel
            ops.segment_stats(self.G, self.P, self.M, self.V, t['tables'], t['chunks'], self.step_count, self.lr, self.betas, self.eps,
                              self.telemetry_every, self.telemetry_slots, t['count'], t['partials_f'], t['partials_i'], t['ring_f'],
                              t['ring_i'], t['head_i'], t['head_f'], lr_dev=lr_dev, **state)
        if self.E is not None:  # after Adam; t is read from the device counter: a captured step carries it as it stands
            ops.ema_update(self.E, self.P, self.ema_decay, self.ema_warmup, self.step_count, **state)
        if self.plateau_f is not None:
            # the scheduler step of train.py:373-374, after everything that reads the learning rate of THIS step; it does nothing where
            # the guard skipped the step or the (already advanced) step count is no multiple of `every`
            sc = self.lr_schedule
            ops.lr_plateau(loss.reshape(1), self._step_dev, sc.every, sc.factor, sc.patience, sc.cooldown, sc.threshold, sc.min_lr, sc.eps,
                           self.plateau_f, self.plateau_i, skip_dev=self.guard_i)
        for w in self._attached:
            # the Adam kernel wrote the attached bf16 views (a weight that is not attached is frozen: no kernel writes it); after a
            # skipped step they still equal cast(P)
            w.mark_fresh()

    def guard_stats(self):
        """The non-finite guard's counters, in one device read (it synchronises): 'seen' steps, of which 'skipped'; 'run', the current
        run of skipped steps; 'last_skipped'; 'grad_norm' of the last step (sqrt(sum g^2) / world, before clipping; NaN or inf where it
        was skipped) and 'last_finite_grad_norm'.  Sets `step_count` to the device's count of applied steps."""
        if self.guard_i is None:
            raise RuntimeError('this trainer has no non-finite guard (skip_nonfinite=False, or a host trainer)')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('guard_stats() inside a stream capture: it reads the device')
        raw = torch.cat([self.guard_i, self.guard_f.view(torch.int32), self._step_dev.view(torch.int32)]).cpu()
        i, f = raw[:4].tolist(), raw[4:].view(torch.float32).tolist()
        self.step_count = int(f[2])
        return {'seen': i[3], 'skipped': i[1], 'run': i[2], 'last_skipped': bool(i[0]), 'grad_norm': f[0], 'last_finite_grad_norm': f[1]}

    def grad_norm(self):
        return float(self.G.norm()) / self.world


class _EmaScope:
    """FlatTrainer.ema_weights()."""

    def __init__(self, trainer):
        self.tr = trainer

    def _point(self, flat, shadow):
        tr = self.tr
        for i, p in enumerate(tr.params):
            p.data = tr._view(flat, i)
        if shadow is not None:
            tr._attach_shadows(shadow)

    def __enter__(self):
        tr = self.tr
        if tr.E is None:
            raise RuntimeError('this trainer keeps no EMA (ema_decay=None)')
        if tr._ema_scope:
            raise RuntimeError('`with trainer.ema_weights():` is already active: the scope does not nest')
        if tr.E.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('`with trainer.ema_weights():` inside a stream capture: a replay would not switch the weights')
        tr._check_bindings()
        tr._ema_prime()
        if tr.S is not None:
            if tr.ES is None:
                tr.ES = torch.empty_like(tr.S)
            ops.cast_bf16(tr.E, tr.ES)
        self._point(tr.E, tr.ES)
        tr._ema_scope = True
        return tr

    def __exit__(self, *exc):
        tr = self.tr
        self._point(tr.P, tr.S)
        tr._ema_scope = False
        return False


class GraphedStep:
    """One training step -- zero_grad, forward, backward, gradient exchange, clip + Adam -- as ONE hipGraph
    (torch.cuda.CUDAGraph).

    The step is several hundred kernel launches issued from Python and from the native layer loops; replayed as a graph
    it costs the host one call, so a slow or contended host (8 ranks sharing a 16-core quota) can no longer stall the GPU.
    `fn(**inputs)` returns the loss and must be capture-safe: device work only, fixed shapes; the stochastic front-end
    draws on the device from a device step counter, so replays need no host input at all.

    With torch.distributed the bucketed all-reduces are captured too: the tower backward returns to the host every few
    layers DURING CAPTURE, `FlatTrainer.layers_done` enqueues the finished range on the communication stream (which
    joins the capture through an event), and the replayed graph carries the same fork / join dependencies -- RCCL
    kernels overlapping the remaining backward.  If the runtime refuses to capture a collective, the step falls back to
    eager launches (`graph is None`, `capture_error` says why).

        step = GraphedStep(trainer, fn, example_inputs)      # runs `warmup` real steps, then captures
        loss = step()                                        # replay on the static inputs
        loss = step(text=..., frames=...)                    # copy new data into the static inputs, then replay
    """

    def __init__(self, trainer, fn, example_inputs, warmup=2):
        refuse_unproven_width(trainer.model, 'a captured trainer step (GraphedStep)')
        self.trainer, self.fn = trainer, fn
        self.static = {k: v.clone() for k, v in example_inputs.items()}
        self.graph, self.capture_error = None, None
        # a captured graph keeps the kernels of the mode it was captured with: recorded here, checked at every replay
        self.deterministic = _lib.is_deterministic()
        if trainer.E is not None:
            if trainer._ema_scope:
                raise RuntimeError('GraphedStep inside `with trainer.ema_weights():`: leave the scope first')
            trainer._ema_prime()  # before the warm-up: the copy E <- P is never captured
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture requires (real training steps)
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        saved = (trainer.step_count, trainer._step_dev.clone(), self._frontend_steps())
        guard = None if trainer.guard_i is None else (trainer.guard_i.clone(), trainer.guard_f.clone())
        graph = torch.cuda.CUDAGraph()
        # with a process group alive, its watchdog thread polls events while we capture: only THIS thread's calls may be
        # policed (the default "global" mode turns the watchdog's hipEventQuery into a capture violation)
        mode = 'thread_local' if (dist.is_available() and dist.is_initialized()) else 'global'
        try:
            with torch.cuda.graph(graph, capture_error_mode=mode):
                self.loss = self._step()
            self.graph = graph
        except Exception as e:  # e.g. a collective that cannot be captured: keep training, eagerly
            self.capture_error = f'{type(e).__name__}: {e}'.splitlines()[0][:200]
            try:
                torch.cuda.synchronize()
            except Exception:  # (the failed capture's own error may surface once more here)
                pass
            trainer.after_failed_capture()
        # the capture pass enqueued nothing: it was not a step
        trainer.step_count = saved[0]
        trainer._step_dev.copy_(saved[1])
        self._frontend_steps(saved[2])
        if guard is not None:
            trainer.guard_i.copy_(guard[0])
            trainer.guard_f.copy_(guard[1])

    def _frontend_steps(self, restore=None):
        fe = getattr(self.trainer.model, 'frontend', None)
        if fe is None or fe.step is None:
            return None
        if restore is not None:
            fe.step.copy_(restore)
            return None
        return fe.step.clone()

    def _step(self):
        self.trainer.zero_grad()
        loss = self.fn(**self.static)
        loss.backward()
        if isinstance(self.trainer.lr_schedule, ReduceLROnPlateau):  # the plateau schedule is stepped on the device from this step's loss
            self.trainer.step(loss=loss.detach())
        else:
            self.trainer.step()
        return loss.detach()

    def __call__(self, **inputs):
        if self.trainer._ema_scope:
            raise RuntimeError('a GraphedStep call inside `with trainer.ema_weights():`: the replay would train P while the model reads '
                               'the averaged weights; leave the scope first')
        if _lib.is_deterministic() != self.deterministic:
            raise RuntimeError(f'this GraphedStep was captured with deterministic={self.deterministic} and is called with '
                               f'deterministic={_lib.is_deterministic()}: a replay would run the other mode\'s kernels; switch back '
                               '(mmvid_amd.set_deterministic) or capture a new GraphedStep')
        for k, v in inputs.items():
            self.static[k].copy_(v, non_blocking=True)
        if self.graph is None:
            return self._step()
        self.graph.replay()
        self.trainer.step_count += 1
        return self.loss


_CAPTURABLE = {}  # (world size, device) -> the answer of collectives_capturable, once per process


def collectives_capturable(device):
    """Can this runtime capture a collective of the current backend into a hipGraph?  Asked BEFORE the training step is captured, on a
    throw-away process group: a collective that fails inside a capture leaves the group's internal streams in capture mode (HIP does not
    release the streams that joined a capture that is torn down), and every later EAGER collective on that group fails with 'operation
    not permitted when stream is capturing' -- the eager fall-back would be dead too.  gloo copies through the host: never capturable.
    All ranks return the same answer."""
    if not (dist.is_available() and dist.is_initialized()):
        return True
    if dist.get_backend() != 'nccl':
        return False
    key = (dist.get_world_size(), str(device))
    if key in _CAPTURABLE:
        return _CAPTURABLE[key]

    def vote(ok):  # every rank learns whether EVERY rank got this far (the default group: untouched by the trial)
        flag = torch.tensor([1 if ok else 0], device=device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(int(flag.item()))

    pg = None
    try:
        pg = dist.new_group(backend='nccl')
    except Exception:
        pg = None
    ok = vote(pg is not None)  # (no rank enters a collective of the trial group unless all of them have it)
    if ok:
        t = torch.zeros(64, device=device)
        try:
            dist.all_reduce(t, group=pg)  # (the communicator is built by the first, eager, collective)
            torch.cuda.synchronize()
        except Exception:
            ok = False
        ok = vote(ok)
    if ok:
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                dist.all_reduce(t, group=pg)
            g.replay()
            torch.cuda.synchronize()
        except Exception:
            ok = False
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
        ok = vote(ok)
    # (the trial group is kept: destroying a group whose collective sits in a captured graph aborts the process on this runtime; the
    #  answer is cached per process, so exactly one extra communicator exists however often steps are captured)
    _CAPTURABLE[key] = ok
    return ok


def backward_order(params):
    """Flat-buffer order = REVERSE of the order gradients become final in the backward, so that reversed buckets
    (heads + last layers first) can be sent while earlier layers are still being differentiated."""
    def key(item):
        n = item[0]
        if n.startswith('transformer.transformer.resblocks.'):
            return (1, int(n.split('.')[3]))
        if n.startswith('to_logits'):
            return (2, 0)
        return (0, 0)  # embeddings / positional tables: final only when the whole backward is done

    return sorted(params, key=key)


def broadcast_parameters(model, src=0, group=None):
    """DDP construction broadcast (train.py:32): parameters and buffers from rank 0."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, src=src, group=group)
