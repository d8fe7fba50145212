"""Fused AdamW over the towers' flat parameter buffers (reference distil_model.py:160-169,
dual_distill_model.py:194-202: AdamW over every requires_grad parameter in one group + HF cosine-with-warmup
stepped per epoch)."""
import contextlib
import math
import struct
from typing import NamedTuple

import torch

from ._lib import lib


# One materialised tower's part of a step: the stream its update runs on (None: a CPU rehearsal) and its ranges, [(p, g, m, v)] or, keeping
# an EMA, [(p, g, m, v, e)] (a sharded tower's: its owned slices, and only for the sums of a clipping step).
_Job = NamedTuple('_Job', [('tower', object), ('stream', object), ('items', list), ('sharded', bool)])
# What every update of one step is handed after its operands, in the order of the hooks' trailing arguments.  st: the raw handle of the stream
# it runs on (None: the current one); ema_weight: None, or 1 - ema_decay, the step keeps the average; gscale: None, or the clipping
# coefficient, a 1-element device tensor; record: None, or the scaler-driven step's device record.
_Control = NamedTuple('_Control', [('zero_grad', bool), ('st', object), ('ema_weight', object), ('gscale', object), ('record', object)])
# What one step() does, settled (and what it cannot do refused) before the step counter moves.  clip: max_grad_norm is set; amp: None, or
# (found_inf, grad_scale) as the loss scaler left them; ema_w: None, or 1 - ema_decay rounded once to f32; kind: the launch, 'multi' (the 24-range
# entries), 'table' (groups) or 'lamb' (trust_ratio); hyper: {id(parameter): (lr_scale, weight_decay)} of the declared groups; layouts:
# (kind, id(tower)) -> the ranges such a launch takes, cut once per step (_layout).
_Plan = NamedTuple('_Plan', [('clip', bool), ('amp', object), ('ema_w', object), ('kind', str), ('hyper', dict), ('layouts', dict)])


def cosine_with_warmup(step, warm, total):
    """transformers.get_cosine_schedule_with_warmup's lr multiplier (num_cycles = 0.5)."""
    if step < warm:
        return float(step) / float(max(1, warm))
    prog = float(step - warm) / float(max(1, total - warm))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))


class FusedAdamW:
    """AdamW over the contiguous trainable ranges of each tower's flat buffer: one multi-range launch (dclip_adamw_multi_scaled) per
    tower and 24 ranges; a range of odd length or off a 16-byte boundary gets a dclip_adamw launch of its own.  That holds for the plain
    step only: every other step has float4 kernels alone (REFUSALS, below).

    The trainable set is fixed when the optimizer is built, like the reference's AdamW(filter(requires_grad, parameters()))
    (dual_distill_model.py:195, distil_model.py:161): parameters unfrozen later (unfreeze_embed) do not enter it.

    Data-parallel runs (tower.dp set by parallel.GradSync.plan): each rank updates only its 1/W shard of every gradient bucket
    from the reduce-scattered average, keeps m / v for that shard only, and the updated parameters are all-gathered.

    max_grad_norm (None = off; a plain attribute, may change between steps): the step clips the global L2 norm of the gradients of
    exactly the parameters this optimizer was built over, like torch.nn.utils.clip_grad_norm_(params, max_grad_norm) before
    torch.optim.AdamW.step(): coef = min(1, max_grad_norm / (norm + 1e-6)) and the update uses g * coef.  Norm and coefficient
    stay on the device (no host synchronisation); last_grad_norm is a 1-element device tensor holding the norm after step(), None
    while clipping is off.  A non-finite norm is not special-cased: coef and the update become NaN, as in torch.  Not optimizer
    state: state_dict() does not carry it.

    Under a loss scaler (precision: 16) this is an optimizer torch.amp.GradScaler.step() drives directly (_step_supports_amp_scaling):
    the scaler sets the device tensors `grad_scale` (None after scaler.unscale_(opt)) and `found_inf` on the optimizer just before
    step() and deletes them after it.  One preparation kernel (dclip_amp_prepare) then turns them, and the sums of a clipping
    step, into a device record every update of the step reads (dclip_adamw_multi_amp): the update uses g * coef / grad_scale, the
    threshold is compared with the norm of the unscaled gradients (last_grad_norm shows that norm), and with found_inf set no
    parameter and no moment is written, on the device, without a host synchronisation.  A skipped step is counted on the device
    and does not advance the bias corrections (t = step_count - skipped); state_dict() writes that t.  The gradients themselves
    are consumed as they are: p.grad is not written back unscaled (torch's fused AdamW does that).  Once steps have been taken
    through a scaler, keep stepping through it: a plain step() takes its bias corrections from step_count alone.

    ema_decay (None = off; a plain attribute, may change between steps): the step also keeps an exponential moving average of the
    parameters it updates, e <- e + (1 - ema_decay) * (p' - e) with p' the parameter the step has just written, in the same kernel
    (dclip_adamw_multi_ema): one more f32 buffer per tower in the layout of m / v and one per extra parameter, allocated by the first
    step() that finds a decay set and filled from the parameters as they are before that step; no launch more per step after it, no
    host synchronisation, and a step that a loss scaler skips leaves the average where it is.  1 - ema_decay is formed in double and
    rounded once.  The usual warm-up, so that the average does not stay at the initial weights for the first 1 / (1 - d) steps, is
    host arithmetic before each step: `opt.ema_decay = min(d, (1 + t) / (10 + t))` with t = opt.step_count.  Back to None freezes the
    average and keeps it.  `with opt.ema_weights():` runs the towers on the average; ema_state_dict() exports it; state_dict() carries
    it under 'ema', next to 'state' and 'param_groups', which stay what torch.optim.AdamW loads.

    groups (None = one weight_decay and one lr for every element, the reference's behaviour and exactly today's launches): a list of
    torch-style dicts {'params': [...], 'weight_decay': x, 'lr_scale': s}, either key optional.  A group's elements are decayed by its
    weight_decay and stepped with lr * lr_scale, the product rounded once to f32; a parameter in no group keeps the optimizer's
    weight_decay and scale 1 (the default group).  Parameters are matched by identity against the trainable set; the constructor
    raises ValueError for a parameter in two groups, one that is frozen or in none of the towers / extra_params, a negative or
    non-finite value, an unknown key (betas and eps are not per group).  Every tower is then stepped by ONE table-driven launch
    (dclip_adamw_table), plain, clipped or scaler-driven, with or without the EMA: its ranges are cut where neighbouring parameters
    differ in (lr_scale, weight_decay), the table lies in device memory, is built at the tower's first step and uploaded again (pinned
    memory, asynchronously on the update's stream) only after `opt.groups[i]['weight_decay']` / `['lr_scale']` or opt.weight_decay
    changed, which takes effect at the next step; no copy and no host synchronisation in any other step.  The clipping norm stays
    global over all groups.  Extra parameters are stepped per distinct (lr_scale, weight_decay) through the 24-range entries.
    param_groups lists the declared groups and then the default group, each with lr = opt.lr * lr_scale; state_dict() writes torch's
    multi-group layout with lr_scale as an extra key per group, which torch.optim.AdamW([*groups, {'params': rest}]) loads and whose
    own dict loads back; a dict with another number of groups is a ValueError.

    trust_ratio (False = off, and then every launch and every bit is what it is without the argument), trust_clip (None = no clip),
    always_adapt: plain attributes, may change between steps.  With trust_ratio the step is LAMB's (You et al. 2020, timm's Lamb): every
    trainable parameter tensor is one UNIT, its update u = m^ / (sqrt(v^) + eps) + wd p (weight decay INSIDE the update, not AdamW's
    p (1 - lr wd)) is scaled by r = |p| / |u|, the L2 norms over the unit's old parameters and its update, and p' = p - lr lr_scale r u.
    r = 1 for a unit whose weight decay is 0 unless always_adapt, and where a norm is 0 or not finite; r <= trust_clip if that is set.
    m and v mean what they mean in AdamW, so switching between steps is well defined.  Every tower is stepped by dclip_lamb_table
    (three launches: moments and partial norms, ratios, apply) over a table cut at EVERY trainable parameter's offset (the layout's
    padding goes with the parameter before it) with the (lr_scale, weight_decay) of its group, or (1, weight_decay) without groups; the
    table is built and re-uploaded by the mechanism of `groups`, workspace and statistics are allocated once per tower.  It composes
    with max_grad_norm (the norm stays global and is formed before the ratios), a loss scaler (a skipped step changes nothing, the
    statistics included), ema_decay, groups and overlap / join=False, with no host wait.  Extra parameters are one unit each, every one
    stepped by the same entry as its own one-range layout: three tiny launches per tensor, a dozen for the four projection tensors of a
    plain CLIP student, which is accepted.  last_trust_stats: {tower index: f32 [units, 4] device tensor of (|p|, |u|, r, 0)} and
    {('extra', j): f32 [1, 4]} after a step; trust_units() lists (parameter name, begin, length) per key in the same order.
    state_dict() then carries trust_ratio / trust_clip / always_adapt as extra keys of every parameter group
    (torch.optim.AdamW.load_state_dict ignores them, like lr_scale); load_state_dict() restores them.

    REFUSALS.  What a step cannot do, step() refuses on the host, before the step counter advances and before anything is launched or
    written (_plan):
      - RuntimeError under the sharded data-parallel exchange for a step that a loss scaler drives (there p.grad holds zeros when the
        scaler looks for overflows), that keeps an EMA (every rank holds 1/W of the optimizer state), that has groups or that forms
        trust ratios (the table kernels have no sharded form; no rank holds a whole unit's norm).  DCLIP_DP_MODE=allreduce and
        DCLIP_DP_MODE=off work for all four.
      - ValueError naming the range, for every step but the plain one, if a range is no multiple of 4 elements or off a 16-byte
        boundary: a tower range or an `extra_params` tensor of a step that clips, is driven by a loss scaler or keeps an EMA; a range as
        the groups cut it; a unit of a trust-ratio step, an extra parameter included.
      - ValueError for an ema_decay outside [0, 1], a group value that has become negative or non-finite, a trust_clip that is <= 0 or
        not finite; RuntimeError inside ema_weights()."""

    _step_supports_amp_scaling = True

    def __init__(self, towers, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, extra_params=(), max_grad_norm=None, ema_decay=None,
                 groups=None, trust_ratio=False, trust_clip=None, always_adapt=False):
        """extra_params: trainable parameters that live outside the towers' flat buffers — the embedding_projection / hidden_projection
        linears of a plain CLIP encoder in the student role (reference image_encoder.py:23-25, text_encoder.py:45-47): four small tensors
        whose gradients autograd produces; they are updated together, like one more tower's ranges (after an all-reduce of each gradient
        in a data-parallel run whose exchange this package owns)."""
        self.towers = list(towers)
        self.extras = [p for p in extra_params if p.requires_grad]
        self._extra_state = {}
        self.base_lr = self.lr = lr
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.step_count = 0
        self._state = {}
        self._fixed_ranges = {}
        for tw in self.towers:
            if tw.flat is not None:
                self._fixed_ranges[id(tw)] = [list(r) for r in tw.trainable_ranges()]
        # overlap mode only: also re-cast the bf16 weight cache right after the update.  Off by default: the re-cast of the NEXT
        # forward runs under the teacher towers' forward (4 streams wide), which hides it better than the end of the step does
        self.refresh_cache_in_step = False
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self._clip_parts = self._clip_out = None
        self._amp_rec = self._skipped = None               # the scaler-driven step's device record and its count of skipped steps
        self.ema_decay = ema_decay
        self._ema = {}                                     # id(tower) -> the average, in the tower's flat layout ; id(extra parameter) -> 1-D
        self._ema_unseeded = set()                         # keys of _ema allocated by the step in flight, not yet filled from the parameters
        self._ema_in_use = False                           # inside ema_weights(): parameters and average have changed places
        self.groups = None if groups is None else self._declare_groups(groups)
        self._tables = {}                                  # id(tower) -> the device table of its ranges and what it was filled from
        self.trust_ratio, self.trust_clip, self.always_adapt = bool(trust_ratio), trust_clip, bool(always_adapt)
        self._lamb = {}                                    # id(tower or extra parameter) -> (workspace, stats) of dclip_lamb_table
        self.last_trust_stats = {}                         # tower index / ('extra', j) -> f32 [units, 4] on the device: (|p|, |u|, r, 0)
        self._trust_clip_value()

    def _ranges(self, tw):
        """contiguous [begin, end) element ranges of the parameters this optimizer was built over"""
        r = self._fixed_ranges.get(id(tw))
        if r is None:                                  # tower materialised after construction: captured at first use
            r = self._fixed_ranges[id(tw)] = [list(x) for x in tw.trainable_ranges()]
        return r

    @staticmethod
    def _placed(tw):
        """[(parameter, its offset in the tower's flat layout)]"""
        return list(zip([p for p in tw._params() if p is not None], tw._offsets))

    def _owned(self, tw):
        """_placed(tw) of the parameters this optimizer updates: the set captured by _ranges(), not the live requires_grad flags"""
        rng = self._ranges(tw)
        return [(p, off) for p, off in self._placed(tw) if any(a <= off < b for a, b in rng)]

    def _is_hip(self, hook):
        """whether `hook` (one of the nine, e.g. '_adamw') is the product's HIP launch, not a torch stand-in substituted for a rehearsal"""
        return getattr(type(self), hook) is getattr(FusedAdamW, hook + '_hip')

    # ---- parameter groups ----
    _GROUP_KEYS = ('params', 'weight_decay', 'lr_scale')

    def _candidates(self):
        """the parameters a group may name: the trainable set this optimizer is built over (a tower that is not materialised yet:
        its requires_grad parameters, which are what _ranges() will capture), tower by tower, extras last"""
        out = []
        for tw in self.towers:
            out += [p for p, _ in self._placed(tw) if p.requires_grad] if tw.flat is None else [p for p, _ in self._owned(tw)]
        return out + list(self.extras)

    @staticmethod
    def _group_value(g, i, key, default):
        x = g.get(key, default)
        if x is None and default is None:                    # (weight_decay: the optimizer's own, whatever it is at the step)
            return None
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0:
            raise ValueError(f'FusedAdamW: groups[{i}][{key!r}] must be a finite number >= 0, got {x!r}')
        return float(x)

    def _declare_groups(self, groups):
        """-> [{'params': [...], 'weight_decay': x or None (the optimizer's), 'lr_scale': s}], checked (class docstring)"""
        known = {id(p) for p in self._candidates()}
        seen, out = {}, []
        for i, g in enumerate(groups):
            if not isinstance(g, dict) or 'params' not in g:
                raise ValueError(f'FusedAdamW: groups[{i}] must be a dict with a \'params\' list')
            unknown = sorted(set(g) - set(self._GROUP_KEYS))
            if unknown:
                raise ValueError(f'FusedAdamW: groups[{i}] has unknown key(s) {unknown}; a group takes {list(self._GROUP_KEYS)} '
                                 '(betas and eps are the optimizer\'s, one lr schedule drives every group through lr_scale)')
            params = [g['params']] if isinstance(g['params'], torch.Tensor) else list(g['params'])
            for p in params:
                if id(p) in seen:
                    raise ValueError(f'FusedAdamW: a parameter of shape {tuple(p.shape)} is in groups[{seen[id(p)]}] and in groups[{i}]')
                if id(p) not in known:
                    raise ValueError(f'FusedAdamW: groups[{i}] names a parameter of shape {tuple(p.shape)} that this optimizer does not update: '
                                     'it is frozen (requires_grad False), or belongs to none of the towers and extra_params')
                seen[id(p)] = i
            out.append({'params': params, 'weight_decay': self._group_value(g, i, 'weight_decay', None), 'lr_scale': self._group_value(g, i, 'lr_scale', 1.0)})
        return out

    def _hyper_of(self):
        """{id(parameter): (lr_scale, weight_decay)} of the declared groups as they stand now (their values may change between steps)"""
        out = {}
        for i, g in enumerate(self.groups):
            key = (self._group_value(g, i, 'lr_scale', 1.0), self._group_value(g, i, 'weight_decay', None))
            out.update((id(p), (key[0], self.weight_decay if key[1] is None else key[1])) for p in g['params'])
        return out

    def _group_ranges(self, tw, hyper=None, units=False):
        """[(begin, end, lr_scale, weight_decay)] of a tower: its fixed ranges cut where neighbouring parameters differ in (lr_scale,
        weight_decay).  A parameter's segment runs to the next parameter's offset (the layout's padding goes with the parameter before it).
        units: cut at EVERY parameter's offset, equal neighbours are not merged (the trust-ratio step: one range per tensor)."""
        hyper = (self._hyper_of() if self.groups is not None else {}) if hyper is None else hyper
        default = (1.0, self.weight_decay)
        segs = sorted((off, hyper.get(id(p), default)) for p, off in self._owned(tw))
        out = []
        for a, b in self._ranges(tw):
            inside = [(off, key) for off, key in segs if a <= off < b]
            if not inside or inside[0][0] != a:
                inside.insert(0, (a, default))
            for (off, key), nxt in zip(inside, [o for o, _ in inside[1:]] + [b]):
                if not units and out and out[-1][1] == off and out[-1][2:] == key and off != a:
                    out[-1] = (out[-1][0], nxt) + key
                else:
                    out.append((off, nxt) + key)
        return out

    def _adamw_table_hip(self, tw, bufs, ranges, zero_grad, st, ema_weight, gscale, record):
        """bufs: the tower's whole flat (p, g, m, v, e or None); ranges: _group_ranges(tw).  ONE launch of dclip_adamw_table.  The device
        table is built on first use and uploaded again only when `ranges` differ from what it holds: from a fresh pinned image, with an
        asynchronous copy on the stream the update runs on (the current one), so the launches of that stream see it in order and no
        host waits.  (`_adamw_table` can be substituted by a torch version like `_adamw`.)"""
        from . import ops
        tab = self._table_of(id(tw), bufs[0], ranges)
        p, g, m, v, e = bufs
        ops.adamw_table(p, g, m, v, e, tab['dev'], len(ranges), tab['tiles'], self.lr, self.betas, self.eps, self.step_count, zero_grad,
                        0.0 if ema_weight is None else ema_weight, gscale, record, st)

    def _table_of(self, key, flat, ranges):
        """the device table of `ranges` over the flat buffer `flat`, kept under `key`: built on first use, uploaded again when `ranges` differ"""
        from . import ops
        tab = self._tables.get(key)
        if tab is None or tab['ranges'] != ranges:
            rows = [(b, e - b, s, wd) for b, e, s, wd in ranges]
            image, tiles = ops.adamw_table_image(rows, flat.numel(), torch.zeros(lib().dclip_adamw_table_bytes(len(rows)), dtype=torch.uint8).pin_memory())
            if tab is None or tab['dev'].numel() != image.numel():
                tab = self._tables[key] = {'dev': torch.empty(image.numel(), dtype=torch.uint8, device=flat.device), 'uploads': 0}
            tab['dev'].copy_(image, non_blocking=True)
            tab.update(ranges=list(ranges), tiles=tiles, uploads=tab['uploads'] + 1)
        return tab

    # ---- layer-wise trust ratios (trust_ratio) ----
    def _trust_clip_value(self):
        """None, or trust_clip as a float; ValueError unless it is finite and > 0"""
        c = self.trust_clip
        if c is None:
            return None
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0:
            raise ValueError(f'FusedAdamW: trust_clip must be None or a finite number > 0, got {c!r}')
        return float(c)

    def _lamb_table_hip(self, key, bufs, ranges, zero_grad, st, ema_weight, gscale, record):
        """bufs: a whole flat (p, g, m, v, e or None); ranges: its units, [(begin, end, lr_scale, weight_decay)].  The three launches of
        dclip_lamb_table; the table is _table_of's, workspace and statistics are allocated at the first step and again only when the
        number of units or tiles changes.  -> the statistics, f32 [units, 4] on the device.  (`_lamb_table` can be substituted by a
        torch version like `_adamw`.)"""
        from . import ops
        tab = self._table_of(key, bufs[0], ranges)
        held = self._lamb.get(key)
        if held is None or held[0] != (len(ranges), tab['tiles']):
            held = self._lamb[key] = ((len(ranges), tab['tiles']),) + ops.lamb_buffers(len(ranges), tab['tiles'], bufs[0].device)
        p, g, m, v, e = bufs
        ops.lamb_table(p, g, m, v, e, tab['dev'], len(ranges), tab['tiles'], self.lr, self.betas, self.eps, self.step_count, held[1], held[2], zero_grad,
                       0.0 if ema_weight is None else ema_weight, gscale, record, self._trust_clip_value(), self.always_adapt, st)
        return held[2]

    def trust_units(self):
        """{tower index: [(parameter name, begin, length)], ('extra', j): [(name, 0, numel)]}: the units of a trust-ratio step, in the
        order of the rows of last_trust_stats (begin and length in elements of the tower's flat buffer, the layout's padding included)"""
        out, names = {}, {}
        for i, tw in enumerate(self.towers):
            module = getattr(tw, 'module', None)
            named = {id(p): n for n, p in module.named_parameters()} if module is not None else {}
            names.update(named)
            at = {off: named.get(id(p), f'parameter {j}') for j, (p, off) in enumerate(self._placed(tw))}
            fresh = id(tw) not in self._fixed_ranges
            out[i] = [(at.get(a, f'[{a}, {b})'), a, b - a) for a, b, _, _ in self._group_ranges(tw, {}, units=True)]
            if fresh and tw.flat is None:                    # a tower that is not materialised yet: its trainable set is captured at its first step
                del self._fixed_ranges[id(tw)]
        for j, p in enumerate(self.extras):
            out[('extra', j)] = [(names.get(id(p), f'extra parameter {j}'), 0, p.numel())]
        return out

    @contextlib.contextmanager
    def _with_hyper(self, lr_scale, weight_decay):
        """inside: self.lr is lr_k = f32(lr) * f32(lr_scale) rounded once to f32, as the table kernel forms it, and self.weight_decay
        the group's: what the existing entries read when the extras of one group are stepped through them"""
        f32 = lambda x: struct.unpack('f', struct.pack('f', x))[0]
        keep = self.lr, self.weight_decay
        self.lr, self.weight_decay = f32(f32(self.lr) * f32(lr_scale)), weight_decay   # (the product of two f32 is exact in double)
        try:
            yield
        finally:
            self.lr, self.weight_decay = keep

    def _adamw_hip(self, p, g, m, v, zero_grad, st, gscale=None):
        """p, g, m, v: equally long 1-D f32 views.  (tests/test_parallel_cpu.py substitutes a torch version as `_adamw` to rehearse the
        sharded bookkeeping over gloo; the product path is the HIP kernel.)  gscale: 1-element tensor, the step uses g * gscale
        (passed only by a clipping step)."""
        if gscale is not None:
            from . import ops
            return ops.adamw_multi_scaled([(p, g, m, v)], self.lr, self.betas, self.eps, self.weight_decay, self.step_count, zero_grad, gscale, st)
        lib().dclip_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), self.lr, self.betas[0],
                          self.betas[1], self.eps, self.weight_decay, self.step_count, 1 if zero_grad else 0, st)

    def _sumsq_hip(self, views, out, st):
        """out (f32, ops.SUMSQ_PARTIALS slots per 24 views, every slot written) <- partial sums of the squares of the 1-D f32 `views`.
        (`_sumsq` and `_coef` can be substituted by torch versions like `_adamw`, for the gloo rehearsals.)"""
        from . import ops
        for i in range(0, len(views), ops.ADAMW_MAX_RANGES):
            k = i // ops.ADAMW_MAX_RANGES
            ops.sumsq_multi(views[i:i + ops.ADAMW_MAX_RANGES], out[k * ops.SUMSQ_PARTIALS:(k + 1) * ops.SUMSQ_PARTIALS], st)

    def _coef_hip(self, partials, extra, out, st):
        """out[0] <- sqrt(sum(partials) + extra[0]) (extra may be None), out[1] <- min(1, max_grad_norm / (out[0] + 1e-6))"""
        from . import ops
        ops.clip_coef(partials, self.max_grad_norm, out, extra, st)

    def _prepare_hip(self, found_inf, grad_scale, partials, extra, record, skipped, st):
        """record <- this step's control record, skipped += (found_inf != 0) (ops.amp_prepare); partials None: the step does not clip.
        (`_prepare` and `_adamw_amp` can be substituted by torch versions like `_adamw`.)"""
        from . import ops
        ops.amp_prepare(record, skipped, self.betas, self.step_count, found_inf, grad_scale, partials,
                        0.0 if partials is None else self.max_grad_norm, extra, st)

    def _adamw_amp_hip(self, p, g, m, v, zero_grad, st, record):
        from . import ops
        ops.adamw_multi_amp([(p, g, m, v)], self.lr, self.betas, self.eps, self.weight_decay, zero_grad, record, st)

    def _adamw_ema_hip(self, items, zero_grad, st, ema_weight, gscale, record):
        """items: at most ops.ADAMW_MAX_RANGES of (p, g, m, v, e).  (`_adamw_ema` and `_swap` can be substituted by torch versions like `_adamw`.)"""
        from . import ops
        ops.adamw_multi_ema(items, self.lr, self.betas, self.eps, self.weight_decay, self.step_count, zero_grad, ema_weight, gscale, record, st)

    def _swap_hip(self, pairs, st):
        from . import ops
        ops.swap_multi(pairs, st)

    # The hook seam: step() and ema_weights() launch through these nine names, which a CPU rehearsal substitutes by name with torch versions
    # (tests/test_parallel_cpu.py was the first); _is_hip() tells which checks a stand-in, which takes any range, switches off.
    _adamw, _sumsq, _coef, _prepare, _adamw_amp = _adamw_hip, _sumsq_hip, _coef_hip, _prepare_hip, _adamw_amp_hip
    _adamw_ema, _swap, _adamw_table, _lamb_table = _adamw_ema_hip, _swap_hip, _adamw_table_hip, _lamb_table_hip

    def _adamw_many(self, items, zero_grad, st, gscale=None, record=None, ema_weight=None):
        """items: [(p, g, m, v)] of equally long 1-D f32 views — ONE multi-range launch per ops.ADAMW_MAX_RANGES ranges (the sharded step
        has one owned slice per gradient bucket: nine launches per step for the two l_clip students became one per tower).  A substituted
        `_adamw`, an odd length or a misaligned pointer: one `_adamw` call per range.  record: the scaler-driven step, every range reads
        that record instead (step() has refused an odd length or a misaligned pointer before it began: _refuse_misaligned).
        ema_weight: items are [(p, g, m, v, e)] and every launch is dclip_adamw_multi_ema, whichever of the three steps it is."""
        from . import ops
        chunks = [items[i:i + ops.ADAMW_MAX_RANGES] for i in range(0, len(items), ops.ADAMW_MAX_RANGES)]
        hyper = self.lr, self.betas, self.eps, self.weight_decay
        if ema_weight is not None:                           # items: [(p, g, m, v, e)], plain, clipped or scaler-driven alike
            for chunk in chunks:
                self._adamw_ema(chunk, zero_grad, st, ema_weight, gscale, record)
        elif record is not None and self._is_hip('_adamw_amp'):
            for chunk in chunks:
                ops.adamw_multi_amp(chunk, *hyper, zero_grad, record, st)
        elif record is not None:
            for p, g, m, v in items:
                self._adamw_amp(p, g, m, v, zero_grad, st, record)
        elif self._is_hip('_adamw') and not any(p.numel() % 4 or (p.data_ptr() | g.data_ptr() | m.data_ptr() | v.data_ptr()) % 16 for p, g, m, v in items):
            for chunk in chunks:
                ops.adamw_multi_scaled(chunk, *hyper, self.step_count, zero_grad, gscale, st)
        else:
            for p, g, m, v in items:
                self._adamw(p, g, m, v, zero_grad, st, *(() if gscale is None else (gscale,)))

    def zero_grad(self, set_to_none=False):
        from .model.component._tower import autograd_params_mode
        for tw in self.towers:
            if tw.flat is not None and autograd_params_mode(tw):
                # the gradients belong to autograd (AccumulateGrad / a DDP reducer): drop them, as torch's zero_grad(set_to_none) does
                for p in tw._params():
                    if p is not None and p.requires_grad:
                        p.grad = None
            if tw.flat_grad is not None and not getattr(tw, '_grad_clean', False):
                self.join()
                tw.flat_grad.zero_()
        for p in self.extras:
            p.grad = None

    @staticmethod
    def _pack_autograd_grads(tw):
        """DCLIP_DP_MODE=off / tower.autograd_params: the backward handed the parameter gradients to autograd, so p.grad are autograd's own
        tensors (or a DistributedDataParallel reducer's bucket views) and tower.flat_grad, which the kernel below reads, was never
        written.  Copy them into the flat buffer (one multi-tensor copy); a trainable parameter without a gradient counts as zero."""
        dst, src = [], []
        for p, off in FusedAdamW._placed(tw):
            if not p.requires_grad:
                continue
            view = tw.flat_grad[off:off + p.numel()]
            g = p.grad
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr():
                if g.dtype != torch.float32 or g.device != view.device:
                    raise RuntimeError('FusedAdamW: parameter gradients must be f32 tensors on the tower\'s device')
                dst.append(view)
                src.append(g.reshape(-1))
        if dst:
            torch._foreach_copy_(dst, src)

    def _ranges_cover_everything(self, tw):
        r = self._ranges(tw)
        return len(r) == 1 and r[0][0] == 0 and r[0][1] >= tw.flat.numel()

    @staticmethod
    def _sharded(tw):
        return getattr(tw, 'dp', None) is not None and getattr(tw, 'sync', None) is not None and tw.sync.enabled

    def _moments(self, tw):
        key = id(tw)
        n = tw.dp.shard_elems if self._sharded(tw) else tw.flat.numel()
        if key in self._state and self._state[key][0].numel() != max(n, 1):
            # the layout of the moments changed under us (torch.distributed initialised, or the shard plan swapped, after state
            # was created or loaded): re-zeroing would silently drop trained / restored Adam moments
            raise RuntimeError(f'FusedAdamW: optimizer state of {self._state[key][0].numel()} elements, but the tower now needs '
                               f'{max(n, 1)} (sharded={self._sharded(tw)}): build the optimizer / load its state after '
                               'torch.distributed and the data-parallel plan are set up')
        if key not in self._state:
            self._state[key] = (torch.zeros(max(n, 1), dtype=torch.float32, device=tw.flat.device),
                                torch.zeros(max(n, 1), dtype=torch.float32, device=tw.flat.device))
        return self._state[key]

    @staticmethod
    def _shard_items(tw, m, v):
        """[(p, g, m, v)] of the trainable slices this rank owns: one per gradient bucket and trainable range inside its shard"""
        items = []
        for b in tw.dp.buckets:
            if b is None:
                continue
            b0, b1, o0, o1, off, own_tr = b
            for a, e in own_tr:
                lo, hi = off + a - o0, off + e - o0
                items.append((tw.flat[a:e], tw.gshard[lo:hi], m[lo:hi], v[lo:hi]))
        return items

    def _step_sharded(self, tw, gscale=None):
        """reduce-scattered gradient shards -> AdamW on the owned slices -> all-gather of the updated parameters, all on the
        exchange stream behind the tower's reduce-scatters (which were released from inside its backward)."""
        from .parallel import all_gather_flat
        sync = tw.sync
        m, v = self._moments(tw)
        s = sync.stream_for(tw.flat, tw)
        grp = sync.group_for(tw)
        if s is not None:
            # whatever the caller's stream holds before step() must be visible on the exchange stream — in particular the
            # zero-fill of freshly allocated m / v (first step): without this edge AdamW read uninitialised moments at world
            # size 2 (NaN weights after one step; found by tests/test_parallel_gpu.py)
            s.wait_stream(torch.cuda.current_stream())
        works = []
        with sync._On(s):
            st = s.cuda_stream if s is not None else None
            items = self._shard_items(tw, m, v)
            if items:
                self._adamw_many(items, False, st, gscale)
            for b in tw.dp.buckets:
                if b is not None:
                    b0, b1, o0, o1, off, own_tr = b
                    works.append(all_gather_flat(tw.flat[b0:b1], tw.flat[o0:o1], async_op=True, group=grp))
            for w in works:
                if w is not None:
                    w.wait()
        tw.wcache_dirty = True
        tw.grads_ready = None
        tw.dp_unstepped.clear()                     # the exchanged averages are consumed: the next backward may release again
        if s is not None:
            tw.opt_done = torch.cuda.Event()
            tw.opt_done.record(s)
        return s

    def _ema_of(self, key, like):
        """the average kept under `key`, in the layout of the f32 tensor `like`; a new one is filled by the step that asked for it"""
        e = self._ema.get(key)
        if e is None:
            e = self._ema[key] = torch.empty(like.numel(), dtype=torch.float32, device=like.device)
            self._ema_unseeded.add(key)
        return e

    def _jobs(self, overlap, main, clip, ema=False):
        """[_Job] of the materialised towers, in tower order: the stream the tower's update runs on and the [(p, g, m, v)] ranges it
        updates (a sharded tower's: only for the sums of a clipping step, _step_sharded takes its own); ema: [(p, g, m, v, e)]"""
        from .model.component._tower import autograd_params_mode
        jobs = []
        for tw in self.towers:
            if tw.flat is None:
                continue
            m, v = self._moments(tw)
            if self._sharded(tw):
                jobs.append(_Job(tw, tw.sync.stream_for(tw.flat, tw), self._shard_items(tw, m, v) if clip else [], True))
                continue
            # (gradients that went through autograd may have been written by anybody's stream — a DDP reducer's —: take them on `main`)
            stream = tw.bwd_stream if (overlap and not autograd_params_mode(tw) and getattr(tw, 'bwd_stream', None) is not None) else main
            bufs = (tw.flat, tw.flat_grad, m, v) + ((self._ema_of(id(tw), tw.flat),) if ema else ())
            jobs.append(_Job(tw, stream, [tuple(t[b:e] for t in bufs) for b, e in self._ranges(tw)], False))
        return jobs

    def _await_grads(self, job, main):
        """a tower that is not sharded: its stream waits for the caller's and for the tower's gradients, which then lie in flat_grad"""
        from .model.component._tower import autograd_params_mode
        from .parallel import GradSync
        tw, stream = job.tower, job.stream
        if stream != main:
            stream.wait_stream(main)                         # whatever the caller enqueued before step() (e.g. zero_grad of others)
        if getattr(tw, 'grads_ready', None) is not None:
            stream.wait_event(tw.grads_ready)                # this tower's gradient average (RCCL side stream), whichever stream updates
            tw.grads_ready = None
        if autograd_params_mode(tw):
            with GradSync._On(stream):
                self._pack_autograd_grads(tw)

    def _multi(self, items, ctl):
        """`items` through the 24-range entries (_adamw_many) under the step's control"""
        self._adamw_many(items, ctl.zero_grad, ctl.st, ctl.gscale, ctl.record, ctl.ema_weight)

    def _update(self, job, plan, ctl, overlap, main):
        """one tower's update by the launch the plan names, on g * ctl.gscale if given or driven by the scaler's record, and what follows
        it on the tower's stream.  Returns the stream the current one has to join, None if there is none.  A step that keeps the
        average first fills a new one from the whole flat buffer (frozen ranges too: they never change), on the same stream."""
        from .parallel import GradSync
        tw, stream = job.tower, job.stream
        if job.sharded:
            return self._step_sharded(tw, ctl.gscale)        # (its exchange stream waits for the current one: the coefficient)
        if (ctl.gscale is not None or ctl.record is not None) and stream != main:
            stream.wait_stream(main)
        with GradSync._On(stream):
            if id(tw) in self._ema_unseeded:
                self._ema[id(tw)].copy_(tw.flat)
                self._ema_unseeded.discard(id(tw))
            ctl = ctl._replace(st=stream.cuda_stream if stream is not None else None)
            if plan.kind == 'multi':
                self._multi(job.items, ctl)
            else:                                            # the whole flat buffers and a table of ranges
                bufs = (tw.flat, tw.flat_grad, *self._moments(tw), self._ema[id(tw)] if ctl.ema_weight is not None else None)
                if plan.kind == 'table':                     # ONE launch for the tower, whichever of the three steps it is
                    self._adamw_table(tw, bufs, self._layout(plan, 'table', tw), *ctl)
                else:                                        # one unit per tensor: moments and partial norms, ratios, apply
                    self.last_trust_stats[self.towers.index(tw)] = self._lamb_table(id(tw), bufs, self._layout(plan, 'lamb', tw), *ctl)
            tw.wcache_dirty = True
            tw._grad_clean = bool(ctl.zero_grad) and self._ranges_cover_everything(tw)
            if overlap and self.refresh_cache_in_step:
                tw._prepare_always = False                   # from now on this optimizer keeps the bf16 cache in step
                tw.prepare()
        if stream == main:
            return None
        tw.opt_done = torch.cuda.Event()
        tw.opt_done.record(stream)
        return stream

    def _update_extras(self, extras, plan, ctl):
        """the parameters outside the tower buffers (`extras`: _extra_items()), on the current stream: their gradients were written by
        autograd on it.  Every tensor is a one-range layout of its own, [(0, numel, lr_scale, weight_decay)]: the trust-ratio step
        launches it as that; with groups the tensors of one (lr_scale, weight_decay) go through the 24-range entries together."""
        if not extras:
            return
        if plan.kind == 'multi':
            return self._multi([it for _, it in extras], ctl)
        hyper = {j: plan.hyper.get(id(self.extras[j]), (1.0, self.weight_decay)) for j, _ in extras}
        if plan.kind == 'lamb':
            for j, it in extras:
                p = self.extras[j]
                self.last_trust_stats[('extra', j)] = self._lamb_table(id(p), it if ctl.ema_weight is not None else it + (None,),
                                                                       [(0, p.numel()) + hyper[j]], *ctl)
            return
        by_key = {}
        for j, it in extras:
            by_key.setdefault(hyper[j], []).append(it)
        for (scale, wd), its in by_key.items():
            with self._with_hyper(scale, wd):
                self._multi(its, ctl)

    def _clip_coef(self, jobs, extras, main, amp=None):
        """max_grad_norm is set: (norm, coef) as two 1-element device tensors, ordered by events only:
          1. every tower's sum of squared gradients, on the stream that tower's update runs on (behind its backward / exchange);
          2. on the current stream, after all of them: the extras' sum, the cross-rank sum, ONE clip_coef -> (norm, coef).
        The updates follow the coefficient and read it from the device.
        amp = (found_inf, grad_scale), the scaler-driven step: 2. ends in ONE amp_prepare instead, which forms the coefficient from
        the unscaled norm -> (norm, record).
        Data-parallel: a sharded tower contributes the squares of this rank's owned slices of the averaged gradient (tw.gshard), so
        those sums are added over the ranks (one all-reduce of one double); gradients every rank holds whole — the extras after
        their all-reduce, a tower that is not sharded — are identical everywhere and enter once, as clip_coef's extra_sumsq.
        Every rank computes the coefficient from the same bits in the same order: `jobs` has the sharded towers first."""
        from . import ops
        from .parallel import GradSync, all_reduce_sum
        G, R = ops.SUMSQ_PARTIALS, ops.ADAMW_MAX_RANGES
        slots = [G * ((len(j.items) + R - 1) // R) for j in jobs] + [G * ((len(extras) + R - 1) // R)]
        device = jobs[0].tower.flat.device if jobs else self.extras[0].device
        if self._clip_parts is None or self._clip_parts.numel() != max(sum(slots), 1) or self._clip_parts.device != device:
            self._clip_parts = torch.zeros(max(sum(slots), 1), dtype=torch.float32, device=device)
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=device)
        parts, out = self._clip_parts, self._clip_out
        at = 0
        for job, n in zip(jobs, slots):
            stream = job.stream
            if not job.sharded:
                self._await_grads(job, main)
            elif stream != main:
                stream.wait_stream(main)
            if job.items:
                with GradSync._On(stream):
                    self._sumsq([it[1] for it in job.items], parts[at:at + n], stream.cuda_stream if stream is not None else None)
            if stream != main:
                ev = torch.cuda.Event()
                ev.record(stream)
                main.wait_event(ev)
            at += n
        st = main.cuda_stream if main is not None else None
        if extras:
            self._sumsq([it[1] for _, it in extras], parts[at:at + slots[-1]], st)
        if amp is not None:
            return self._amp_record(*amp, parts, st)
        n_sharded = sum(n for j, n in zip(jobs, slots) if j.sharded)
        if any(j.sharded for j in jobs):                     # (the same on every rank, whatever this rank owns)
            total = parts[:n_sharded].sum(dtype=torch.float64).view(1)
            all_reduce_sum(total)
            rest = parts[n_sharded:sum(slots)]
            self._coef(total.float(), rest.sum(dtype=torch.float64).float().view(1) if rest.numel() else None, out, st)
        else:
            self._coef(parts, None, out, st)
        return out[0:1], out[1:2]

    def _amp_record(self, found_inf, grad_scale, partials, st):
        """ONE preparation launch on the current stream -> (norm or None, record).  The record of the step before may still be read by a
        tower's un-joined update, which this launch must not overtake: the current stream waits for those first."""
        from . import ops
        self.join()
        if self._amp_rec is None:
            dev = found_inf.device if found_inf is not None else grad_scale.device
            self._amp_rec = torch.zeros(ops.AMP_RECORD_FLOATS, dtype=torch.float32, device=dev)
            self._skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        one = lambda t: None if t is None else t.detach().reshape(1)
        self._prepare(one(found_inf), one(grad_scale), partials, None, self._amp_rec, self._skipped, st)
        return (None if partials is None else self._amp_rec[ops.AMP_NORM:ops.AMP_NORM + 1]), self._amp_rec

    def _norm_coef_record(self, plan, jobs, extras, main):
        """-> (norm, coef, record) of the step, device tensors or None, for {clipping or not} x {a loss scaler or not}: a clipping step
        forms the sums and from them (norm, coef), under a scaler (norm, record); a scaler alone needs no gradient for its record, so the
        updates can then go on tower by tower; the plain step has none of the three."""
        if plan.clip:
            norm, made = self._clip_coef(jobs, extras, main, plan.amp)
            return (norm, made, None) if plan.amp is None else (norm, None, made)
        if plan.amp is None:
            return None, None, None
        return None, None, self._amp_record(*plan.amp, None, main.cuda_stream if main is not None else None)[1]

    # ---- what a step cannot do: refused by _plan(), on the host, before the step counter moves and before anything is launched or written ----
    _NOT_SHARDED = {                                         # feature -> why the sharded data-parallel exchange does not carry it
        'amp': 'a loss scaler (precision: 16) cannot drive the sharded data-parallel exchange: after backward_and_sync() p.grad holds zeros, so the '
               'scaler\'s overflow check sees nothing.  The modes that work under precision: 16 are DCLIP_DP_MODE=allreduce and DCLIP_DP_MODE=off',
        'ema': 'ema_decay is not kept under the sharded data-parallel exchange: every rank updates and holds the state of 1/W of each gradient '
               'bucket only, and an average in shards would have to be gathered to be used.  The modes that keep an EMA are '
               'DCLIP_DP_MODE=allreduce and DCLIP_DP_MODE=off',
        'groups': 'parameter groups are not stepped under the sharded data-parallel exchange: every rank updates 1/W of each gradient bucket, '
                  'cut by the exchange plan and not by the groups.  The modes that take groups are DCLIP_DP_MODE=allreduce and DCLIP_DP_MODE=off',
        'trust': 'trust ratios are not formed under the sharded data-parallel exchange: every rank updates 1/W of each gradient bucket, cut by '
                 'the exchange plan and not at the tensors, so no rank holds a whole unit\'s norm.  The modes that take trust_ratio are '
                 'DCLIP_DP_MODE=allreduce and DCLIP_DP_MODE=off',
    }
    _FLOAT4_ONLY = {                                         # launch kind -> what its float4 kernels need of every range
        'multi': 'a step that clips the gradient norm, is driven by a loss scaler or keeps an EMA (ema_decay) needs every range to be a multiple '
                 'of 4 elements on a 16-byte boundary.  Only the plain step has an element-wise kernel (dclip_adamw)',
        'table': 'a step with parameter groups (dclip_adamw_table) needs every range, cut at the group boundaries, to be a multiple of 4 elements '
                 'on a 16-byte boundary',
        'lamb': 'a step with trust ratios (dclip_lamb_table) needs every unit, one per parameter tensor, to be a multiple of 4 elements on a '
                '16-byte boundary',
    }

    def _features(self, amp):
        """(feature, what this step has of it or None) of the four features the sharded exchange does not carry, in the order in which
        they refuse.  Lazily: a setting of a feature's own that cannot be stepped (raised here) comes after the refusals of those before it."""
        yield 'amp', amp
        if self._ema_in_use:
            raise RuntimeError('FusedAdamW.step: inside ema_weights() the towers hold the averaged weights; leave the context first')
        yield 'ema', self._ema_weight()
        yield 'groups', None if self.groups is None else self._hyper_of()       # (a value spoiled since construction: ValueError)
        if self.trust_ratio:
            self._trust_clip_value()
        yield 'trust', True if self.trust_ratio else None

    def _plan(self):
        """-> the _Plan of the step about to be taken.  The only place that refuses: a feature under the sharded exchange, then a range
        that a float4-only launch of this step cannot take."""
        found_inf, grad_scale = getattr(self, 'found_inf', None), getattr(self, 'grad_scale', None)
        amp = None if found_inf is None and grad_scale is None else (found_inf, grad_scale)
        sharded = any(tw.flat is not None and self._sharded(tw) for tw in self.towers)
        on = {}
        for feature, value in self._features(amp):
            if value is not None and sharded:
                raise RuntimeError(f'FusedAdamW.step: {self._NOT_SHARDED[feature]}')
            on[feature] = value
        kind = 'lamb' if on['trust'] else 'multi' if on['groups'] is None else 'table'
        plan = _Plan(self.max_grad_norm is not None, amp, on['ema'], kind, on['groups'] or {}, {})
        # Which ranges must be float4 ranges.  The table kernels have no other form: their ranges are checked unless the hook is a torch
        # stand-in, which takes any range (with groups AND trust ratios the groups' cut is still checked first, and named first).  The
        # fixed ranges and the extras go through the 24-range entries and dclip_sumsq_multi, float4 only except for the plain step; H(x): hook
        # x is the HIP launch:
        #     EMA  clip  scaler | checked if
        #      1    0     any   | H(_adamw_ema)
        #      1    1     any   | H(_adamw_ema) or H(_sumsq)
        #      0    0     0     | never: dclip_adamw takes any range
        #      0    0     1     | H(_adamw_amp)
        #      0    1     0     | H(_sumsq) or H(_adamw)
        #      0    1     1     | H(_sumsq) or H(_adamw_amp)
        H, clip, scaler = self._is_hip, plan.clip, amp is not None
        if plan.ema_w is not None:
            multi = H('_adamw_ema') or (clip and H('_sumsq'))
        else:
            multi = (clip and (H('_sumsq') or (not scaler and H('_adamw')))) or (scaler and H('_adamw_amp'))
        for check, due in (('table', on['groups'] is not None and H('_adamw_table')), ('lamb', on['trust'] and H('_lamb_table')), ('multi', multi)):
            if due:
                self._refuse_misaligned(plan, check)
        return plan

    def _layout(self, plan, kind, tw):
        """the ranges a launch of `kind` takes over tower `tw` in this step: what _plan() checks is what _update() launches, cut once"""
        if (kind, id(tw)) not in plan.layouts:
            plan.layouts[kind, id(tw)] = self._ranges(tw) if kind == 'multi' else self._group_ranges(tw, plan.hyper, units=kind == 'lamb')
        return plan.layouts[kind, id(tw)]

    def _refuse_misaligned(self, plan, kind):
        """ValueError naming the first range of a launch of `kind` (_layout; except for 'table', whose extras go through the 24-range
        entries, also an extra parameter that has a gradient) that is no multiple of 4 elements or off a 16-byte boundary.  (The moments
        and the average start on an allocation's boundary and share the parameters' offsets.)"""
        found = []
        for i, tw in enumerate(self.towers):
            if tw.flat is None or self._sharded(tw):         # (a sharded tower's owned slices are cut by the plan of parallel.GradSync)
                continue
            found += [(f'tower {i} range [{a}, {e})', e - a, tw.flat.data_ptr() + 4 * a, tw.flat_grad.data_ptr() + 4 * a, 4 * a)
                      for a, e, *_ in self._layout(plan, kind, tw)]
        if kind != 'table':
            found += [(f'extra parameter {i} ({tuple(p.shape)})', p.numel(), p.data_ptr(), p.grad.data_ptr(), 0)
                      for i, p in enumerate(self.extras) if p.grad is not None]
        for what, n, *ptrs in found:
            if n % 4 or any(x % 16 for x in ptrs):
                raise ValueError(f'FusedAdamW.step: {what} has {n} elements at {ptrs[0]:#x} (gradient at {ptrs[1]:#x}); {self._FLOAT4_ONLY[kind]}')

    @torch.no_grad()
    def step(self, zero_grad=False, overlap=False, join=True):
        """zero_grad=True: the kernel clears each gradient element once it has consumed it (saves the separate 306 MB fill that
        otherwise runs alone on the main stream); the next zero_grad() is then free.  Frozen ranges are never written by the
        backward, so a fully trainable tower stays clean until its next backward.

        overlap=True: each tower is updated on the stream its backward ran on, as soon as that backward (and, under data
        parallelism, that tower's gradient exchange) is done, followed by the re-cast of its bf16 weight cache — the shorter
        tower's update then runs under the longer tower's backward instead of alone at the end of the step.  The current stream
        is ordered after every tower's update before step() returns, unless join=False: then only the tower streams carry the
        dependency (backward -> exchange -> update -> next forward of that tower) and the next step's frozen teacher towers
        may start while the last gradient exchange and update are still running; join() orders the current stream after them
        (zero_grad() and state_dict() call it)."""
        plan = self._plan()                                  # (every refusal)
        self.step_count += 1
        # decided by where the parameters live, not by asking the runtime: a CPU step (the gloo rehearsals) leaves the GPU closed
        on_gpu = any(t.is_cuda for t in [tw.flat for tw in self.towers if tw.flat is not None] + self.extras)
        main = torch.cuda.current_stream() if on_gpu else None
        jobs = self._jobs(overlap, main, plan.clip, plan.ema_w is not None)
        extras = None
        if plan.clip:                                        # all sums before the first update: the extras are taken now, not after the towers
            jobs.sort(key=lambda j: not j.sharded)           # (stable) the sharded towers' partial sums lie first
            extras = self._extra_items(plan.ema_w is not None)
        self.last_grad_norm, coef, record = self._norm_coef_record(plan, jobs, extras, main)
        ctl = _Control(zero_grad, main.cuda_stream if main is not None else None, plan.ema_w, coef, record)
        joined = []
        for job in jobs:
            if not plan.clip and not job.sharded:            # tower by tower (a clipping step has awaited them all for its sums)
                self._await_grads(job, main)
            joined.append(self._update(job, plan, ctl, overlap, main))
        self._update_extras(self._extra_items(plan.ema_w is not None) if extras is None else extras, plan, ctl)
        if join:
            for stream in joined:
                if stream is not None:
                    main.wait_stream(stream)
            for tw in self.towers:
                tw.opt_done = None

    def _extra_moments(self, p):
        st = self._extra_state.get(id(p))
        if st is None:
            st = self._extra_state[id(p)] = (torch.zeros(p.numel(), dtype=torch.float32, device=p.device),
                                             torch.zeros(p.numel(), dtype=torch.float32, device=p.device))
        return st

    def _extra_items(self, ema=False):
        """[(j, (p, g, m, v))] of the extras[j] that have a gradient, the gradients averaged over the ranks; ema: (p, g, m, v, e), a new
        average filled from its parameter here, on the current stream, which the extras' update runs on"""
        if not self.extras:
            return []
        from .parallel import all_reduce_avg
        sync = next((tw.sync for tw in self.towers if getattr(tw, 'sync', None) is not None), None)
        items = []
        for j, p in enumerate(self.extras):
            if p.grad is None:
                continue                                  # torch.optim.AdamW skips parameters without a gradient
            if not (p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32 and p.grad.dtype == torch.float32):
                raise RuntimeError('FusedAdamW: extra parameters and their gradients must be contiguous f32 tensors')
            if sync is not None and sync.enabled:
                all_reduce_avg(p.grad)
            m, v = self._extra_moments(p)
            item = (p.data.view(-1), p.grad.view(-1), m, v)
            if ema:
                e = self._ema_of(id(p), p)
                if id(p) in self._ema_unseeded:
                    e.copy_(p.data.view(-1))
                    self._ema_unseeded.discard(id(p))
                item += (e,)
            items.append((j, item))
        return items

    def join(self):
        """order the current stream after every tower's pending (un-joined) update"""
        pending = [tw for tw in self.towers if getattr(tw, 'opt_done', None) is not None]
        if not pending:
            return
        cur = torch.cuda.current_stream()
        for tw in pending:
            cur.wait_event(tw.opt_done)
            tw.opt_done = None

    # ---- the exponential moving average of the parameters (ema_decay) ----
    def _ema_weight(self):
        """None while ema_decay is None, else 1 - ema_decay formed in double and rounded once to f32 (1.f - 0.9999f is 1.66e-4 off)"""
        if self.ema_decay is None:
            return None
        d = float(self.ema_decay)
        if not 0.0 <= d <= 1.0:                              # (a NaN fails both)
            raise ValueError(f'FusedAdamW: ema_decay must lie in [0, 1], got {self.ema_decay!r}')
        return struct.unpack('f', struct.pack('f', 1.0 - d))[0]

    def _has_ema(self):
        return any(k not in self._ema_unseeded for k in self._ema)

    def _ema_pairs(self):
        """[(tower or None, [(parameters, average)])]: the optimizer's fixed ranges of every tower that has an average, then the extras"""
        out = []
        for tw in self.towers:
            e = self._ema.get(id(tw))
            if tw.flat is not None and e is not None and id(tw) not in self._ema_unseeded:
                out.append((tw, [(tw.flat[a:b], e[a:b]) for a, b in self._ranges(tw)]))
        extras = [(p.data.view(-1), self._ema[id(p)]) for p in self.extras if id(p) in self._ema and id(p) not in self._ema_unseeded]
        return out + ([(None, extras)] if extras else [])

    def _ema_exchange(self):
        """parameters <-> average on the current stream, after every pending update: one launch per tower (per 24 ranges) and one for
        the extras; every tower touched re-casts its bf16 weight cache at its next forward"""
        from . import ops
        self.join()
        st = torch.cuda.current_stream().cuda_stream if any(a.is_cuda for _, prs in self._ema_pairs() for a, _ in prs) else None
        for tw, pairs in self._ema_pairs():
            for i in range(0, len(pairs), ops.ADAMW_MAX_RANGES):
                self._swap(pairs[i:i + ops.ADAMW_MAX_RANGES], st)
            if tw is not None:
                tw.wcache_dirty = True

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights():` the towers (and the extra parameters) hold the averaged weights: evaluate, export, score.  An
        exchange in place, bit for bit (dclip_swap_multi), of the ranges this optimizer updates — frozen ranges are not touched —, and
        the same exchange back on exit, after which every parameter is what it was.  Both mark the towers' bf16 weight caches stale.
        Runs on the current stream; enter and leave on the same one.  Inside, step(), state_dict(), load_state_dict(),
        ema_state_dict() and a second ema_weights() raise RuntimeError, and so does entering before any step has kept an average."""
        if self._ema_in_use:
            raise RuntimeError('FusedAdamW.ema_weights: already inside ema_weights()')
        if not self._has_ema():
            raise RuntimeError('FusedAdamW.ema_weights: there is no average yet: no step() has run with ema_decay set, and none was loaded')
        self._ema_exchange()
        self._ema_in_use = True
        try:
            yield self
        finally:
            self._ema_in_use = False
            self._ema_exchange()

    def _refuse_inside_ema(self, what):
        if self._ema_in_use:
            raise RuntimeError(f'FusedAdamW.{what}: inside ema_weights() parameters and average have changed places; leave the context first')

    def _ema_params(self, slots):
        """{i: the average of slot i, shaped like its parameter} for the slots that have one"""
        out = {}
        for i, (tw, off, n, shape) in enumerate(slots):
            e = self._ema.get(id(tw))
            if e is not None and id(tw) not in self._ema_unseeded:
                out[i] = (e if off is None else e[off:off + n]).view(shape).clone()
        return out

    def ema_state_dict(self, params=None):
        """{i: averaged parameter i} over _slots(params), the order of state_dict()'s 'state': what to export as the averaged student.
        A slot without an average of its own (an extra parameter that never had a gradient) carries its parameter."""
        self._refuse_inside_ema('ema_state_dict')
        if not self._has_ema():
            raise RuntimeError('FusedAdamW.ema_state_dict: there is no average yet: no step() has run with ema_decay set, and none was loaded')
        self.join()
        slots = self._slots(params)
        out = self._ema_params(slots)
        for i, (tw, off, n, shape) in enumerate(slots):
            if i not in out:
                out[i] = (tw.data if off is None else tw.flat[off:off + n]).view(shape).clone()
        return dict(sorted(out.items()))

    def _load_ema(self, ema, slots):
        """restore the average from state_dict()'s 'ema' entry; none saved: forget the one held, the next step starts from the parameters"""
        self._ema.clear()
        self._ema_unseeded.clear()
        if ema is None:
            return
        if ema.get('decay') is not None:
            self.ema_decay = ema['decay']
        for i, (tw, off, n, shape) in enumerate(slots):
            t = ema['params'].get(i, ema['params'].get(str(i)))
            if t is None:
                continue
            if tuple(t.shape) != shape:
                raise ValueError(f'FusedAdamW.load_state_dict: parameter {i} has shape {shape}, its saved average {tuple(t.shape)}')
            if off is None:
                self._ema[id(tw)] = t.detach().to(device=tw.device, dtype=torch.float32, copy=True).reshape(-1)
                continue
            if self._sharded(tw):
                raise RuntimeError('FusedAdamW.load_state_dict: the checkpoint carries an EMA, which the sharded data-parallel exchange '
                                   'does not keep (DCLIP_DP_MODE=allreduce and DCLIP_DP_MODE=off do)')
            if id(tw) not in self._ema:
                self._ema[id(tw)] = tw.flat.detach().clone()     # (frozen ranges and slots without a saved average: the parameters)
            self._ema[id(tw)][off:off + n].copy_(t.reshape(-1))

    def _full_moments(self, tw):
        """(m, v) in the flat layout of the tower; collective in a sharded data-parallel run (all-gather of the ranks' shards)"""
        m, v = self._moments(tw)
        if self._sharded(tw):
            return tw.sync.gather_full(tw, m), tw.sync.gather_full(tw, v)
        return m, v

    # ---- torch.optim.AdamW-compatible (de)serialisation: what a Lightning checkpoint stores under 'optimizer_states' ----
    def _partition(self, items, ptr_of):
        """items split like torch's param_groups: one list per declared group, in the order its 'params' were given, then the rest
        (the default group) in the order of `items`"""
        by_ptr = {ptr_of(x): x for x in items}
        parts = [[by_ptr[p.data_ptr()] for p in g['params'] if p.data_ptr() in by_ptr] for g in self.groups]
        taken = {p.data_ptr() for g in self.groups for p in g['params']}
        return parts + [[x for x in items if ptr_of(x) not in taken]]

    @staticmethod
    def _slot_ptr(slot):
        """the address of a slot's parameter"""
        return slot[0].data_ptr() if slot[1] is None else slot[0].flat.data_ptr() + 4 * slot[1]

    def _slots(self, params=None):
        """[(tower, offset, numel, shape)] of the trainable parameters, in `params` order (default: tower order).  With parameter groups:
        group by group as torch numbers them, the declared groups first, then the default group in `params` order."""
        slots = self._slots_flat(params)
        if self.groups is None:
            return slots
        return sum(self._partition(slots, self._slot_ptr), [])

    def _slots_flat(self, params=None):
        where = {}
        for tw in self.towers:
            if tw.flat is not None:
                where.update((p.data_ptr(), (tw, off, p.numel(), tuple(p.shape))) for p, off in self._owned(tw))
        for p in self.extras:
            where[p.data_ptr()] = (p, None, p.numel(), tuple(p.shape))
        if params is None:
            return list(where.values())
        out = []
        for p in params:
            if p.data_ptr() not in where and not p.requires_grad:
                continue
            if p.data_ptr() not in where:
                if any(p.data_ptr() == q.data_ptr() for tw in self.towers if tw.flat is not None for q, _ in self._placed(tw)):
                    continue                                  # unfrozen after the optimizer was built: not one of its slots
                raise ValueError('FusedAdamW.state_dict: a trainable parameter is not a view of a tower buffer')
            out.append(where[p.data_ptr()])
        return out

    def _trainable(self):
        """the parameters behind _slots(), in its order: tower by tower, extras last"""
        out = [p for tw in self.towers if tw.flat is not None for p, _ in self._owned(tw)] + list(self.extras)
        return out if self.groups is None else sum(self._partition(out, lambda p: p.data_ptr()), [])

    @property
    def param_groups(self):
        """what torch.amp.GradScaler iterates to reach the p.grad views (unscale_, its overflow check): one group over the parameters
        this optimizer was built over.  A read-only picture: the hyper-parameters are the optimizer's attributes (opt.lr is the knob).
        With parameter groups: the declared groups, then the default group with the rest, each with lr = opt.lr * lr_scale; the knobs
        are opt.lr and the dicts of opt.groups."""
        one = lambda ps, s, wd: {'params': ps, 'lr': self.lr * s, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': wd}
        if self.groups is None:
            return [one(self._trainable(), 1.0, self.weight_decay)]
        flat = self._trainable()
        parts = self._partition(flat, lambda p: p.data_ptr())
        out = []
        for g, ps in zip(self.groups + [{'lr_scale': 1.0, 'weight_decay': None}], parts):
            out.append(dict(one(ps, g['lr_scale'], self.weight_decay if g['weight_decay'] is None else g['weight_decay']), lr_scale=g['lr_scale']))
        return out

    def _steps_taken(self):
        """step_count less the steps a loss scaler had skipped (one host read of the device counter)"""
        return self.step_count - (int(self._skipped.item()) if self._skipped is not None else 0)

    def state_dict(self, params=None):
        """`params`: the iteration order torch.optim.AdamW would have been built with (reference distil_model.py:161,
        dual_distill_model.py:195: filter(requires_grad, self.parameters())); default = canonical tower order.

        COLLECTIVE in a sharded data-parallel run: every rank holds 1/W of m / v, so every rank must call this (the moments are
        all-gathered per bucket); checkpoint.save_checkpoint does that and lets rank 0 alone write the file.

        Once a step has kept an EMA (ema_decay) there is a third top-level key: 'ema': {'decay': ema_decay, 'params': {i: the average of
        parameter i, shaped like it}}, i as in 'state'.  torch.optim.AdamW.load_state_dict ignores it; load_state_dict() here restores it."""
        self._refuse_inside_ema('state_dict')
        self.join()
        slots = self._slots(params)
        state = {}
        steps = self._steps_taken()
        full = {id(tw): self._full_moments(tw) for tw in self.towers if id(tw) in self._state}
        for i, (tw, off, n, shape) in enumerate(slots):
            if off is None:                               # a parameter outside the tower buffers
                if id(tw) in self._extra_state:
                    m, v = self._extra_state[id(tw)]
                    state[i] = {'step': torch.tensor(float(steps)), 'exp_avg': m.view(shape).clone(),
                                'exp_avg_sq': v.view(shape).clone()}
                continue
            if id(tw) in full:
                m, v = full[id(tw)]
                state[i] = {'step': torch.tensor(float(steps)), 'exp_avg': m[off:off + n].view(shape).clone(),
                            'exp_avg_sq': v[off:off + n].view(shape).clone()}
        group = {'lr': self.lr, 'initial_lr': self.base_lr, 'betas': tuple(self.betas), 'eps': self.eps,
                 'weight_decay': self.weight_decay, 'amsgrad': False, 'maximize': False, 'foreach': None,
                 'capturable': False, 'differentiable': False, 'fused': None, 'params': list(range(len(slots)))}
        sd = {'state': state, 'param_groups': [group]}
        if self.groups is not None:
            # torch's multi-group layout: parameter ids count on from group to group (_slots() is in that order), lr_scale an extra key
            sd['param_groups'], at = [], 0
            sizes = [len(part) for part in self._partition(slots, self._slot_ptr)]
            for g, n in zip(self.groups + [{'lr_scale': 1.0, 'weight_decay': None}], sizes):
                s, wd = g['lr_scale'], self.weight_decay if g['weight_decay'] is None else g['weight_decay']
                sd['param_groups'].append(dict(group, lr=self.lr * s, initial_lr=self.base_lr * s, weight_decay=wd, lr_scale=s, params=list(range(at, at + n))))
                at += n
        if self.trust_ratio:                                 # extra keys of every group, like lr_scale: torch ignores them, load_state_dict() restores them
            for g in sd['param_groups']:
                g.update(trust_ratio=True, trust_clip=self._trust_clip_value(), always_adapt=self.always_adapt)
        if self._has_ema():
            sd['ema'] = {'decay': self.ema_decay, 'params': self._ema_params(slots)}
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, params=None):
        """Restores moments, step count, hyper-parameters and, if the dict carries one, the EMA.  A dict without 'ema' drops an average
        this optimizer holds: with ema_decay set, the next step() starts a new one from the parameters as they are then."""
        self._refuse_inside_ema('load_state_dict')
        slots = self._slots(params)
        saved = sd['param_groups']
        here = 1 if self.groups is None else len(self.groups) + 1
        if len(saved) != here:
            raise ValueError(f'FusedAdamW.load_state_dict: the dict has {len(saved)} parameter group(s), this optimizer {here} '
                             f'({here - 1} declared in `groups` and the default group): build it with the groups the dict was saved with')
        group = saved[-1]                                    # the default group carries the optimizer's own lr and weight_decay
        if self.groups is not None:
            sizes = [len(part) for part in self._partition(slots, self._slot_ptr)]
            for i, (g, n) in enumerate(zip(saved, sizes)):
                if len(g['params']) != n:
                    raise ValueError(f"FusedAdamW.load_state_dict: group {i} has {len(g['params'])} saved parameters, {n} here")
            for i, (mine, g) in enumerate(zip(self.groups, saved)):
                new = {'weight_decay': self._group_value(g, i, 'weight_decay', mine['weight_decay']), 'lr_scale': self._group_value(g, i, 'lr_scale', mine['lr_scale'])}
                mine.update(new)
        elif len(group['params']) != len(slots):
            raise ValueError(f"FusedAdamW.load_state_dict: {len(group['params'])} saved parameters, {len(slots)} trainable here")
        self.lr = group['lr']
        self.base_lr = group.get('initial_lr', self.base_lr)
        self.betas, self.eps, self.weight_decay = tuple(group['betas']), group['eps'], group['weight_decay']
        if 'trust_ratio' in group:                           # (a dict saved with the feature off, or torch's own, has no such key: keep what is set)
            self.trust_ratio, self.trust_clip, self.always_adapt = bool(group['trust_ratio']), group.get('trust_clip'), bool(group.get('always_adapt', False))
            self._trust_clip_value()
        steps = set()
        for i, (tw, off, n, shape) in enumerate(slots):
            st = sd['state'].get(i, sd['state'].get(str(i)))
            if st is None:
                continue
            if tuple(st['exp_avg'].shape) != shape:
                raise ValueError(f"FusedAdamW.load_state_dict: parameter {i} has shape {shape}, saved {tuple(st['exp_avg'].shape)}")
            if off is None:                               # a parameter outside the tower buffers
                m, v = self._extra_moments(tw)
                m.copy_(st['exp_avg'].reshape(-1))
                v.copy_(st['exp_avg_sq'].reshape(-1))
                steps.add(int(float(st['step'])))
                continue
            m, v = self._moments(tw)
            if self._sharded(tw):
                # keep the slices of this parameter that fall into the shards this rank owns
                for b in tw.dp.live():
                    b0, b1, o0, o1, soff, _ = b
                    lo, hi = max(off, o0), min(off + n, o1)
                    if lo < hi:
                        m[soff + lo - o0:soff + hi - o0].copy_(st['exp_avg'].reshape(-1)[lo - off:hi - off])
                        v[soff + lo - o0:soff + hi - o0].copy_(st['exp_avg_sq'].reshape(-1)[lo - off:hi - off])
            else:
                m[off:off + n].copy_(st['exp_avg'].reshape(-1))
                v[off:off + n].copy_(st['exp_avg_sq'].reshape(-1))
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('FusedAdamW.load_state_dict: parameters with different step counts (one fused step counter here)')
        self.step_count = steps.pop() if steps else 0
        if self._skipped is not None:
            self._skipped.zero_()
        self._load_ema(sd.get('ema'), slots)


class FusedLAMB(FusedAdamW):
    """FusedAdamW with trust_ratio=True: LAMB on the towers' flat buffers (the class docstring of FusedAdamW states the arithmetic)."""

    def __init__(self, towers, *args, trust_ratio=True, **kw):
        super().__init__(towers, *args, trust_ratio=trust_ratio, **kw)


def no_decay_groups(model):
    """-> [one group with weight_decay = 0] for FusedAdamW(groups=...) / model.optimizer_groups: every trainable parameter of the student
    towers (model.towers(), their extra parameters included) with dim() <= 1 — biases, LayerNorm gains and biases, the head-mixing
    vectors — plus the names each student encoder's no_weight_decay() returns (pos_embed, cls_token): what timm and open_clip leave
    undecayed by default.  The reference defines no_weight_decay() and never uses it, so this is not the default here either."""
    params, seen = [], set()
    for tw in model.towers():
        skip = set(getattr(tw.module, 'no_weight_decay', lambda: ())())
        named = {id(p): n for n, p in tw.module.named_parameters()}
        mine = [p for p in tw._params() if p is not None] + list(getattr(tw.module, 'extra_parameters', lambda: [])())
        for p in mine:
            if p.requires_grad and id(p) not in seen and (p.dim() <= 1 or named.get(id(p)) in skip):
                seen.add(id(p))
                params.append(p)
    return [{'params': params, 'weight_decay': 0.0}]


class EpochCosineSchedule:
    """lr = base_lr * cosine_with_warmup(epoch): stepped once per epoch like the reference's Lightning default."""

    def __init__(self, optimizer, warm_steps, total_steps):
        self.opt, self.warm, self.total, self.epoch = optimizer, warm_steps, total_steps, 0
        self.opt.lr = self.opt.base_lr * cosine_with_warmup(0, warm_steps, total_steps)

    def step(self):
        self.epoch += 1
        self.opt.lr = self.opt.base_lr * cosine_with_warmup(self.epoch, self.warm, self.total)

    def get_last_lr(self):
        return [self.opt.lr]

    def state_dict(self):
        """LambdaLR-shaped (what the reference's scheduler — transformers.get_cosine_schedule_with_warmup, a LambdaLR — saves
        and what its load_state_dict updates from: base_lrs, last_epoch, _step_count, _last_lr, lr_lambdas=[None] for a
        plain function), plus the two schedule constants under their own keys"""
        return {'base_lrs': [self.opt.base_lr], 'last_epoch': self.epoch, 'verbose': False, '_step_count': self.epoch + 1,
                '_get_lr_called_within_step': False, '_last_lr': [self.opt.lr], 'lr_lambdas': [None],
                'warm_steps': self.warm, 'total_steps': self.total}

    def load_state_dict(self, sd):
        self.epoch = sd['last_epoch']
        if sd.get('base_lrs'):
            self.opt.base_lr = sd['base_lrs'][0]
        self.opt.lr = self.opt.base_lr * cosine_with_warmup(self.epoch, self.warm, self.total)
