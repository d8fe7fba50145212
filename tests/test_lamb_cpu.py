"""Host side of the trust-ratio (LAMB) step: the header's wording and the exported symbols, every host refusal of dclip_lamb_workspace_bytes /
dclip_lamb_table (they return before anything touches the device), FusedAdamW(trust_ratio=True)'s refusals, unit cutting, trust_units() and
state-dict keys on stand-in towers with a torch version of the entry (as tests/test_adamw_groups_cpu.py rehearses the table step), the
cutting on the l_clip students' layouts, and tests/lamb_cases.py's float64 restatement against a per-tensor loop, an f32 emulation of the
kernels' operation order against its bounds, and two wrong forms outside them, on every case tests/test_lamb_gpu.py runs."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import adamw_cases as ac
import adamw_groups_cases as gc
import lamb_cases as lc
import test_adamw_groups_cpu as tg


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_header_states_the_arithmetic_and_the_library_exports_the_entries():
    from distillclip_amd import _lib as binding
    src = open(binding._HEADER).read()
    for pat in (r'size_t\s+dclip_lamb_workspace_bytes\s*\(', r'int\s+dclip_lamb_table\s*\(', r'weight decay INSIDE the update', r'r_k = min\(r_k, trust_clip\)',
                r'if wd_k == 0 and not always_adapt', r'Three launches on `stream`, no atomics, no host synchronisation: the same call gives the\s+\*?\s*same bits',
                r'changes no byte of p, m, v, e and of stats', r'a NaN trust_clip', r'bit for bit\s+\*?\s*as from dclip_adamw_table'):
        assert re.search(pat, src), pat
    lib = _lib()
    res, args = lib.protos['dclip_lamb_table']
    assert res is ctypes.c_int and len(args) == 23 and args[17] is ctypes.c_float and args[18] is ctypes.c_int and args[20] is ctypes.c_size_t
    assert lib.protos['dclip_lamb_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64])
    assert lib.protos['dclip_adamw_table'][1] == lib.protos['dclip_lamb_table'][1][:17] + [ctypes.c_void_p]       # the table entry's arguments, then the new ones
    for name in ('dclip_lamb_table', 'dclip_lamb_workspace_bytes', 'dclip_adamw_table'):
        assert getattr(lib._dll, name) is not None
    assert lib.dclip_version() == 6
    assert [lib.dclip_lamb_workspace_bytes(c, t) for c, t in ((0, 5), (-1, 5), (3, 2), (1, 1), (3, 5), (70, 9363), (1, 2 ** 31))] == [0, 0, 0, 16, 80, 16 * 9363, 0]


A0 = 0x10000                                                     # addresses that are never read: every call below is refused on the host


def test_every_host_refusal_of_dclip_lamb_table():
    lib = _lib()
    ok = dict(p=A0, g=2 * A0, m=3 * A0, v=4 * A0, e=5 * A0, table=6 * A0, count=3, tiles=5, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, zero_grad=0, w=0.5,
              gscale=None, record=None, clip=-1.0, adapt=0, ws=9 * A0, ws_bytes=80, stats=10 * A0, stream=None)
    cases = {
        'bases 16-byte aligned': [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(p=A0 + 4), dict(g=2 * A0 + 8), dict(m=3 * A0 + 12), dict(v=4 * A0 + 4),
                                  dict(e=5 * A0 + 4)],
        'a device table on an 8-byte boundary, count >= 1': [dict(table=None), dict(table=6 * A0 + 4), dict(count=0), dict(count=-3)],
        'tiles for 3 ranges': [dict(tiles=2), dict(tiles=0), dict(tiles=-1), dict(tiles=2 ** 31)],
        'exclude each other': [dict(gscale=7 * A0, record=8 * A0)],
        r'ema_weight .* \[0, 1\]': [dict(w=-1e-6), dict(w=1.0 + 2.0 ** -20), dict(w=float('nan')), dict(w=float('inf'))],
        'record of dclip_amp_prepare, or step >= 1': [dict(step=0), dict(step=-5), dict(record=8 * A0 + 4), dict(record=8 * A0 + 8, step=0)],
        'trust_clip is NaN': [dict(clip=float('nan'))],
        r'workspace needs 80 bytes on a 16-byte boundary': [dict(ws=None), dict(ws=9 * A0 + 8), dict(ws=9 * A0 + 4), dict(ws_bytes=79), dict(ws_bytes=0)],
        r'stats is 3 x 4 f32 on a 16-byte boundary': [dict(stats=None), dict(stats=10 * A0 + 4), dict(stats=10 * A0 + 8)],
    }
    for match, bads in cases.items():
        for bad in bads:
            a = dict(ok, **bad)
            with pytest.raises(ValueError, match='dclip_lamb_table: .*' + match):
                lib.dclip_lamb_table(*[a[k] for k in ok])


# ---- FusedAdamW on stand-in towers ---------------------------------------------------------------------------------------------------------------
def _torch_lamb(self, key, bufs, ranges, zero_grad, st, ema_weight, gscale, record):
    """dclip_lamb_table, plain or clipped, in torch float32 -> stats"""
    assert record is None
    self.lamb_calls = getattr(self, 'lamb_calls', []) + [(key, list(ranges))]
    p, g, m, v, e = bufs
    b1, b2 = self.betas
    stats = torch.zeros(len(ranges), 4)
    bc1, bc2s = 1 - b1 ** self.step_count, (1 - b2 ** self.step_count) ** 0.5
    for k, (a, b, s, wd) in enumerate(ranges):
        gs = g[a:b] if gscale is None else g[a:b] * gscale
        m[a:b].mul_(b1).add_(gs, alpha=1 - b1)
        v[a:b].mul_(b2).addcmul_(gs, gs, value=1 - b2)
        u = (m[a:b] / bc1) / (v[a:b].sqrt() / bc2s + self.eps) + wd * p[a:b]
        n_p, n_u = p[a:b].double().norm().item(), u.double().norm().item()
        r = n_p / n_u if (self.always_adapt or wd != 0) and n_p > 0 and n_u > 0 else 1.0
        r = r if self.trust_clip is None else min(r, self.trust_clip)
        stats[k] = torch.tensor([n_p, n_u, r, 0.0])
        p[a:b].sub_(u, alpha=self.lr * s * r)
        if e is not None:
            e[a:b].add_(p[a:b] - e[a:b], alpha=ema_weight)
        if zero_grad:
            g[a:b].zero_()
    return stats


def _rehearsal(base=None):
    from distillclip_amd import optim

    class Rehearsal(base or optim.FusedAdamW):
        _lamb_table, _adamw_table, _adamw = _torch_lamb, tg._torch_table, tg._torch_adamw
    return Rehearsal


def test_the_constructor_arguments_and_fused_lamb():
    from distillclip_amd.optim import FusedAdamW, FusedLAMB
    from distillclip_amd.model._distill_base import DistillBase
    tw = tg._tower()
    opt = FusedAdamW([tw])
    assert opt.trust_ratio is False and opt.trust_clip is None and opt.always_adapt is False and opt.last_trust_stats == {}
    opt = FusedAdamW([tw], trust_ratio=True, trust_clip=1.0, always_adapt=True)
    assert opt.trust_ratio is True and opt.trust_clip == 1.0 and opt.always_adapt is True
    assert issubclass(FusedLAMB, FusedAdamW) and FusedLAMB([tw]).trust_ratio is True and FusedLAMB([tw], trust_ratio=False).trust_ratio is False
    assert FusedLAMB([tw], 1e-2, trust_clip=3).lr == 1e-2
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError, match='trust_clip must be None or a finite number > 0'):
            FusedAdamW([tw], trust_clip=bad)
    assert DistillBase.trust_ratio is None and DistillBase.trust_clip is None and DistillBase.always_adapt is False


def test_unit_cutting_on_a_hand_written_layout():
    from distillclip_amd.optim import FusedAdamW
    tw = tg._tower()
    P = tw._params()
    cut = lambda groups, **kw: FusedAdamW([tw], weight_decay=0.05, groups=groups, trust_ratio=True, **kw)._group_ranges(tw, units=True)
    # one unit per trainable tensor, the padding with the tensor before it, the frozen tensor left out; equal neighbours are NOT merged
    assert cut(None) == [(0, 256, 1.0, 0.05), (256, 320, 1.0, 0.05), (448, 512, 1.0, 0.05), (512, 576, 1.0, 0.05), (576, 1216, 1.0, 0.05), (1216, 1280, 1.0, 0.05)]
    assert cut([{'params': [P[1], P[3], P[4], P[6]], 'weight_decay': 0.0}, {'params': [P[5]], 'lr_scale': 0.1}]) == \
        [(0, 256, 1.0, 0.05), (256, 320, 1.0, 0.0), (448, 512, 1.0, 0.0), (512, 576, 1.0, 0.0), (576, 1216, 0.1, 0.05), (1216, 1280, 1.0, 0.0)]
    opt = FusedAdamW([tw], weight_decay=0.05, trust_ratio=True)
    assert opt._group_ranges(tw) == [(0, 320, 1.0, 0.05), (448, 1280, 1.0, 0.05)]                     # (the merged form is untouched)
    extra = torch.nn.Parameter(torch.zeros(8, 4))
    opt = FusedAdamW([tw], extra_params=[extra], trust_ratio=True)
    assert opt.trust_units() == {0: [('parameter 0', 0, 256), ('parameter 1', 256, 64), ('parameter 3', 448, 64), ('parameter 4', 512, 64), ('parameter 5', 576, 640),
                                     ('parameter 6', 1216, 64)], ('extra', 0): [('extra parameter 0', 0, 32)]}


def test_unit_cutting_and_names_on_the_l_clip_students():
    from distillclip_amd.optim import FusedAdamW, no_decay_groups
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    towers = [RepeatVisionTransformer(img_size=224, patch_size=32, out_dim=512, embed_dim=768, depth=6, num_heads=24, qkv_bias=True,
                                      repeated_times=2, use_transform=True)._tower,
              RepeatTextTransformer(depth=4, repeated_times=2, use_transform=True)._tower]
    model = types.SimpleNamespace(towers=lambda: towers)
    for groups in (None, no_decay_groups(model)):
        opt = FusedAdamW(towers, weight_decay=0.05, groups=groups, trust_ratio=True)
        units = opt.trust_units()
        assert opt._fixed_ranges == {}                                                                # listing the units of towers without buffers captured nothing
        for i, tw in enumerate(towers):
            live = [p for p in tw._params() if p is not None]
            named = {id(p): n for n, p in tw.module.named_parameters()}
            offs = tw.param_offsets()
            cut = opt._group_ranges(tw, units=True)
            assert len(cut) == len(live) == len(units[i]) and all(p.requires_grad for p in live)
            assert [u[0] for u in units[i]] == [named[id(p)] for p in live] and [(a, b - a) for a, b, _, _ in cut] == [u[1:] for u in units[i]]
            assert [a for a, _, _, _ in cut] == tw._offsets and cut[0][0] == 0 and cut[-1][1] == offs[-1]
            assert all(x[1] == y[0] for x, y in zip(cut, cut[1:])) and all((b - a) % 4 == 0 and a % 4 == 0 and b - a >= p.numel() for (a, b, _, _), p in zip(cut, live))
            want = [(1.0, 0.0 if groups is not None and any(p is q for q in groups[0]['params']) else 0.05) for p in live]
            assert [c[2:] for c in cut] == want and (groups is None or 0 < sum(w[1] == 0 for w in want) < len(want))


def test_refusals_come_before_the_step_counter_moves():
    from distillclip_amd.optim import FusedAdamW
    tw = tg._FakeTower([(64, True), (7, True), (64, True)], 3, pad=1)                 # a layout without padding: a unit of 7 elements
    opt = FusedAdamW([tw], trust_ratio=True)                                           # the product hook: nothing is launched, the refusal comes first
    before = tw.flat.clone()
    with pytest.raises(ValueError, match=r'tower 0 range \[64, 71\) has 7 elements.*trust ratios \(dclip_lamb_table\)'):
        opt.step()
    assert opt.step_count == 0 and opt._state == {} and opt._tables == {} and opt._lamb == {} and torch.equal(tw.flat, before)
    tw = tg._FakeTower([(2, False), (64, True)], 3, pad=1)                             # a multiple of 4 elements, 8 bytes off a 16-byte boundary
    opt = FusedAdamW([tw], trust_ratio=True)
    with pytest.raises(ValueError, match=r'tower 0 range \[2, 66\) has 64 elements'):
        opt.step()
    assert opt.step_count == 0
    tw = tg._tower()
    extra = torch.nn.Parameter(torch.zeros(7))
    extra.grad = torch.zeros(7)
    opt = FusedAdamW([tw], extra_params=[extra], trust_ratio=True)
    with pytest.raises(ValueError, match=r'extra parameter 0 \(\(7,\)\) has 7 elements'):
        opt.step()
    assert opt.step_count == 0
    # a trust_clip spoiled after construction
    opt = _rehearsal()([tg._tower()], trust_ratio=True)
    for bad in (0.0, -2.0, float('nan'), float('inf')):
        opt.trust_clip = bad
        with pytest.raises(ValueError, match='trust_clip must be None or a finite number > 0'):
            opt.step()
    assert opt.step_count == 0 and opt._state == {}
    # the sharded exchange
    tw = tg._tower(4)

    def boom(*a, **k):
        raise AssertionError('the refusal must come before anything else')
    tw.dp = types.SimpleNamespace(shard_elems=8, buckets=[])
    tw.sync = types.SimpleNamespace(enabled=True, stream_for=boom, group_for=boom)
    opt = _rehearsal()([tw], trust_ratio=True)
    with pytest.raises(RuntimeError, match=r'trust ratios.*sharded.*DCLIP_DP_MODE=allreduce.*DCLIP_DP_MODE=off'):
        opt.step()
    assert opt.step_count == 0 and opt._state == {}


def _lamb(seed=1, base=None, **kw):
    tw = tg._tower(seed)
    P = tw._params()
    extra = [torch.nn.Parameter(torch.randn(8, 4, generator=torch.Generator().manual_seed(7))), torch.nn.Parameter(torch.randn(8, generator=torch.Generator().manual_seed(8)))]
    groups = [{'params': [P[6], P[1], P[3], P[4], extra[1]], 'weight_decay': 0.0}, {'params': [P[5]], 'lr_scale': 0.1}]
    return tw, extra, _rehearsal(base)([tw], lr=1e-2, weight_decay=0.05, extra_params=extra, groups=groups, **kw)


def test_a_rehearsed_step_against_the_float64_restatement():
    tw, extra, opt = _lamb(trust_ratio=True, trust_clip=2.0, ema_decay=0.75)
    frozen = tw.flat[320:448].clone()
    for step in range(2):
        g = torch.Generator().manual_seed(20 + step)
        tw.flat_grad.copy_(torch.randn(tw.flat.numel(), generator=g) * tg._mask(tw))
        for x in extra:
            x.grad = torch.randn(x.shape, generator=g)
        units = [(a, b - a, s, wd) for a, b, s, wd in opt._group_ranges(tw, units=True)]
        m, v = (opt._moments(tw) if step else (torch.zeros_like(tw.flat), torch.zeros_like(tw.flat)))
        flat = dict(p=tw.flat.numpy().copy(), g=tw.flat_grad.numpy().copy(), m=m.numpy().copy(), v=v.numpy().copy())
        h = (1e-2, 0.9, 0.999, 1e-8)
        ref = lc.reference(flat, units, h, 1 - 0.9 ** (step + 1), (1 - 0.999 ** (step + 1)) ** 0.5, None, 2.0, False)
        opt.step()
        assert np.allclose(tw.flat.numpy(), ref['p'], rtol=1e-5, atol=1e-6) and np.allclose(opt.last_trust_stats[0][:, 2].numpy(), ref['r'], rtol=1e-5)
        assert (opt.last_trust_stats[0][[1, 2, 3, 5], 2] == 1).all() and (opt.last_trust_stats[0][[0, 4], 2] != 1).all()
    assert torch.equal(tw.flat[320:448], frozen) and opt.step_count == 2
    calls = opt.lamb_calls
    assert [k for k, _ in calls] == [id(tw), id(extra[0]), id(extra[1])] * 2
    assert calls[0][1] == [(0, 256, 1.0, 0.05), (256, 320, 1.0, 0.0), (448, 512, 1.0, 0.0), (512, 576, 1.0, 0.0), (576, 1216, 0.1, 0.05), (1216, 1280, 1.0, 0.0)]
    assert calls[1][1] == [(0, 32, 1.0, 0.05)] and calls[2][1] == [(0, 8, 1.0, 0.0)]                 # every extra parameter is one unit with its group's values
    assert set(opt.last_trust_stats) == {0, ('extra', 0), ('extra', 1)} and set(opt.trust_units()) == set(opt.last_trust_stats)
    assert opt.last_trust_stats[('extra', 1)][0, 2] == 1 and opt.last_trust_stats[('extra', 0)][0, 2] != 1
    assert opt._has_ema() and not hasattr(opt, 'table_calls')                                         # the AdamW table was never called


def test_state_dict_keys_both_ways():
    from distillclip_amd.optim import FusedLAMB
    tw, extra, off = _lamb()
    tw2, extra2, on = _lamb(trust_ratio=True, trust_clip=1.5, always_adapt=True)
    plain_keys = {'lr', 'initial_lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable', 'differentiable', 'fused', 'params', 'lr_scale'}
    assert all(set(g) == plain_keys for g in off.state_dict()['param_groups']) and set(off.state_dict()) == {'state', 'param_groups'}
    sd = on.state_dict()
    assert all(set(g) == plain_keys | {'trust_ratio', 'trust_clip', 'always_adapt'} for g in sd['param_groups'])
    assert all(g['trust_ratio'] is True and g['trust_clip'] == 1.5 and g['always_adapt'] is True for g in sd['param_groups'])
    assert [set(g) for g in on.param_groups] == [set(g) for g in off.param_groups]                    # the scaler's picture is unchanged
    # torch.optim.AdamW loads the dict, keeps the extra keys, and its own dict restores them here
    cpu, ref = tg._twin(on)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]['trust_clip'] == 1.5
    tw3, extra3, fresh = _lamb()
    fresh.load_state_dict(ref.state_dict())
    assert fresh.trust_ratio is True and fresh.trust_clip == 1.5 and fresh.always_adapt is True
    # a dict saved with the feature off leaves what is set; one saved with it on and None as the clip restores None
    fresh.load_state_dict(off.state_dict())
    assert fresh.trust_ratio is True and fresh.trust_clip == 1.5
    on.trust_clip, on.always_adapt = None, False
    fresh.load_state_dict(on.state_dict())
    assert fresh.trust_ratio is True and fresh.trust_clip is None and fresh.always_adapt is False
    # without groups: the one group there has always been, plus the keys
    one = FusedLAMB([tg._tower()], trust_clip=4)
    (g,) = one.state_dict()['param_groups']
    assert g['trust_ratio'] is True and g['trust_clip'] == 4.0 and 'lr_scale' not in g
    one.trust_ratio = False
    assert set(one.state_dict()['param_groups'][0]) == plain_keys - {'lr_scale'}


# ---- the restatement, the bounds and the emulation on every case of tests/test_lamb_gpu.py ---------------------------------------------------------------
def _gpu_cases():
    """(label, flat, ranges, gs, clip, adapt, t)"""
    for count in lc.COUNTS:
        flat, _ = gc.inputs(count)
        for gs in (None, 0.3172):
            for adapt, t in ((False, 1), (True, 7)):
                yield f'count {count} gs {gs} adapt {adapt}', flat, lc.units_of(count)[0], gs, None, adapt, t
    for fam in lc.FAMILIES:
        flat, gs = gc.inputs(25, fam)
        for t in [t for t in (1, 1000) if t in ac.steps_of(fam)]:
            yield f'{fam} t {t}', flat, lc.units_of(25)[0], gs, None, t == 1000, t
    for kind, clip in (('zero_p', None), ('zero_u', None), ('clip', lc.CLIP)):
        flat, ranges, _ = lc.planted(kind)
        yield kind, flat, ranges, None, clip, True, 3


def test_the_restatement_equals_a_per_tensor_loop_on_every_gpu_case():
    n = 0
    for label, flat, ranges, gs, clip, adapt, t in _gpu_cases():
        bc1, bc2s = ac.exact_bc(ac.HYPER, t)
        ref = lc.reference(flat, ranges, lc.H4, bc1, bc2s, gs, clip, adapt)
        p2, rows = lc.brute_force(flat, ranges, lc.H4, bc1, bc2s, gs, clip, adapt)
        scale = np.maximum(np.abs(p2), 1e-30)
        assert float((np.abs(ref['p'] - p2) / scale).max()) < 1e-12, label
        got = np.stack([ref['np'], ref['nu'], ref['r']], axis=1)
        assert np.allclose(got, np.array(rows), rtol=1e-12, atol=0), label
        mask = gc.inside_mask(ranges, flat['p'].size)
        assert np.array_equal(ref['p'][~mask], np.asarray(flat['p'], dtype=np.float64)[~mask])
        n += 1
    assert n == 16 + 11 + 3


def test_the_emulated_kernels_stay_inside_the_bounds_and_wrong_forms_do_not():
    for label, flat, ranges, gs, clip, adapt, t in _gpu_cases():
        if label.startswith('count') and not label.startswith('count 25'):
            continue
        pairs = [ac.exact_bc(ac.HYPER, t)]
        p2, m2, v2, stats = lc.emulate(flat, ranges, lc.H4, *pairs[0], gs, clip, adapt)
        res = lc.judge(flat, dict(p=p2, m=m2, v=v2), stats, ranges, lc.H4, pairs, gs, clip, adapt, label=label)
        assert max(res.values()) <= 1, (label, res)
    flat, _ = gc.inputs(25)
    ranges = lc.units_of(25)[0]
    pairs = [ac.exact_bc(ac.HYPER, 7)]
    _, m2, v2, stats = lc.emulate(flat, ranges, lc.H4, *pairs[0], None, None, True)
    for form in ('decay_outside', 'grad_norm'):
        bad = lc.wrong(form, flat, ranges, lc.H4, *pairs[0]).astype(np.float32)
        with pytest.raises(AssertionError, match='no candidate pair'):
            lc.judge(flat, dict(p=bad, m=m2, v=v2), stats, ranges, lc.H4, pairs, None, None, True, label=form)
