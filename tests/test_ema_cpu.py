"""Host side of the EMA in the fused AdamW step: the two C entries' declarations and refusals (they return before anything touches the
device), FusedAdamW's refusals and bookkeeping on stand-in towers with torch versions of the two kernels (the way
tests/test_parallel_cpu.py rehearses the sharded step), and the float64 reference and bound of tests/ema_cases.py held to an f32
emulation of the kernel's arithmetic on every case tests/test_ema_gpu.py runs."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import ema_cases as ec


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_two_entries():
    from distillclip_amd import _lib as binding
    src = open(binding._HEADER).read()
    assert re.search(r'int\s+dclip_adamw_multi_ema\s*\(', src) and re.search(r'int\s+dclip_swap_multi\s*\(', src)
    lib = _lib()
    res, args = lib.protos['dclip_adamw_multi_ema']
    assert res is ctypes.c_int and len(args) == 18 and args[14] is ctypes.c_float and args[12] is ctypes.c_int64
    res, args = lib.protos['dclip_swap_multi']
    assert res is ctypes.c_int and len(args) == 5
    for name in ('dclip_adamw_multi_ema', 'dclip_swap_multi', 'dclip_adamw_multi', 'dclip_adamw_multi_scaled', 'dclip_adamw_multi_amp', 'dclip_adamw'):
        assert getattr(lib._dll, name) is not None
    assert lib.dclip_version() == 6


A0 = 0x10000                                                     # addresses that are never read: every call below is refused on the host


def _ptrs(count, base, step=0x1000):
    return (ctypes.c_void_p * max(count, 1))(*[base + k * step for k in range(count)])


def _ema_args(**kw):
    a = dict(p=_ptrs(3, A0), g=_ptrs(3, 2 * A0), m=_ptrs(3, 3 * A0), v=_ptrs(3, 4 * A0), e=_ptrs(3, 5 * A0), n=(ctypes.c_int64 * 3)(4, 8, 1028), count=3,
             lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, zero_grad=0, w=0.5, gscale=None, record=None, stream=None)
    a.update(kw)
    return [a[k] for k in ('p', 'g', 'm', 'v', 'e', 'n', 'count', 'lr', 'b1', 'b2', 'eps', 'wd', 'step', 'zero_grad', 'w', 'gscale', 'record', 'stream')]


def _with(arr, k, value):
    out = type(arr)(*list(arr))
    out[k] = value
    return out


def test_every_host_refusal_of_dclip_adamw_multi_ema():
    lib = _lib()
    e, p, n = _ptrs(3, 5 * A0), _ptrs(3, A0), (ctypes.c_int64 * 3)(4, 8, 1028)
    cases = {
        'e is NULL': dict(e=None),
        'e of range 1': dict(e=_with(e, 1, None)),
        'e of range 2': dict(e=_with(e, 2, e[2] + 4)),
        'e of range 0': dict(e=_with(e, 0, e[0] + 8)),
        r'ema_weight .* \[0, 1\]': [dict(w=-1e-6), dict(w=1.0 + 2.0 ** -20), dict(w=float('nan')), dict(w=float('inf')), dict(w=-float('inf'))],
        'exclude each other': dict(gscale=6 * A0, record=7 * A0),
        'record': dict(record=7 * A0 + 4),
        'step >= 1': dict(step=0),
        '1..24 ranges': [dict(count=0), dict(count=25), dict(p=None), dict(n=None)],
        'range 1 must be': [dict(p=_with(p, 1, None)), dict(p=_with(p, 1, p[1] + 4)), dict(n=_with(n, 1, 6)), dict(n=_with(n, 1, 0))],
    }
    for match, bads in cases.items():
        for bad in bads if isinstance(bads, list) else [bads]:
            with pytest.raises(ValueError, match='dclip_adamw_multi_ema: .*' + match):
                lib.dclip_adamw_multi_ema(*_ema_args(**bad))


def test_every_host_refusal_of_dclip_swap_multi():
    lib = _lib()
    a, b, n = _ptrs(3, A0), _ptrs(3, 2 * A0), (ctypes.c_int64 * 3)(4, 8, 1028)
    cases = {
        '1..24 ranges': [(None, b, n, 3), (a, None, n, 3), (a, b, None, 3), (a, b, n, 0), (a, b, n, 25), (a, b, n, -1)],
        'range 1 must be': [(_with(a, 1, None), b, n, 3), (a, _with(b, 1, None), n, 3), (_with(a, 1, a[1] + 4), b, n, 3), (a, _with(b, 1, b[1] + 8), n, 3),
                            (a, b, _with(n, 1, 6), 3), (a, b, _with(n, 1, 0), 3)],
        'range 2 overlap': [(a, _with(b, 2, a[2] + 16), n, 3), (_with(a, 2, b[2] + 4 * 1028 - 16), b, n, 3)],
    }
    for match, bads in cases.items():
        for bad in bads:
            with pytest.raises(ValueError, match='dclip_swap_multi: .*' + match.replace('range 2 overlap', 'range 2 overlap')):
                lib.dclip_swap_multi(*bad, None)


# ---- FusedAdamW on stand-in towers ------------------------------------------------------------------------------------------------------------
class _FakeTower:
    """flat buffers and trainable ranges of a tower, without the HIP runtime (tests/test_parallel_cpu.py's)"""

    def __init__(self, total, trainable, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat = torch.randn(total, generator=g)
        self.flat_grad = torch.randn(total, generator=g)
        self._trainable = trainable
        self.sync = self.dp = self.gshard = None
        self.wcache_dirty = False
        self.grads_ready = self.opt_done = self.bwd_stream = None
        self._grad_clean = False
        edges = sorted({0, total} | {e for r in trainable for e in r})
        self._offsets = edges[:-1]
        self._plist = [self.flat[a:b] for a, b in zip(edges[:-1], edges[1:])]

    def _params(self):
        return self._plist

    def trainable_ranges(self):
        return [list(r) for r in self._trainable]


def _torch_adamw_ema(self, items, zero_grad, st, ema_weight, gscale, record):
    """dclip_adamw_multi_ema, plain or clipped: torch.optim.AdamW, then e += w (p' - e)"""
    assert record is None and len(items) <= 24
    b1, b2 = self.betas
    for p, g, m, v, e in items:
        gs = g if gscale is None else g * gscale
        p.mul_(1.0 - self.lr * self.weight_decay)
        m.mul_(b1).add_(gs, alpha=1 - b1)
        v.mul_(b2).addcmul_(gs, gs, value=1 - b2)
        bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
        p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(self.eps), value=-self.lr / bc1)
        e.add_(p - e, alpha=ema_weight)
        if zero_grad:
            g.zero_()


def _torch_swap(self, pairs, st):
    for a, b in pairs:
        t = a.clone()
        a.copy_(b)
        b.copy_(t)


def _rehearsal():
    from distillclip_amd.optim import FusedAdamW

    class Rehearsal(FusedAdamW):
        _adamw_ema, _swap = _torch_adamw_ema, _torch_swap

        def _adamw(self, *a, **k):
            raise AssertionError('a step with ema_decay set took the path without the average')
    return Rehearsal


TOTAL, TRAINABLE = 64 * 10, [[64, 64 * 4], [64 * 5, 64 * 9]]


def _mask():
    m = torch.zeros(TOTAL, dtype=torch.bool)
    for a, b in TRAINABLE:
        m[a:b] = True
    return m


def test_the_average_follows_the_parameters_and_the_context_exchanges_them():
    tw = _FakeTower(TOTAL, TRAINABLE, 1)
    extra = torch.nn.Parameter(torch.randn(16, 8, generator=torch.Generator().manual_seed(2)))
    opt = _rehearsal()([tw], lr=1e-2, weight_decay=1e-2, extra_params=[extra], ema_decay=0.75)
    with pytest.raises(RuntimeError, match='no average'):
        with opt.ema_weights():
            pass
    with pytest.raises(RuntimeError, match='no average'):
        opt.ema_state_dict()
    assert 'ema' not in opt.state_dict()
    start, start_x = tw.flat.clone(), extra.detach().clone()
    want, want_x = start.double(), start_x.double()
    for step in range(3):
        g = torch.Generator().manual_seed(10 + step)
        tw.flat_grad.copy_(torch.randn(TOTAL, generator=g) * _mask())
        extra.grad = torch.randn(16, 8, generator=g)
        opt.step()
        want = want + 0.25 * (tw.flat.double() - want)
        want_x = want_x + 0.25 * (extra.detach().double() - want_x)
    mask = _mask()
    e = opt._ema[id(tw)]
    assert torch.allclose(e[mask].double(), want[mask], rtol=1e-6, atol=1e-7) and torch.equal(e[~mask], start[~mask]) and torch.equal(tw.flat[~mask], start[~mask])
    assert torch.allclose(opt._ema[id(extra)].view(16, 8).double(), want_x, rtol=1e-6, atol=1e-7)
    # the dicts
    esd = opt.ema_state_dict()
    slots = opt._slots()
    assert list(esd) == list(range(len(slots))) == [0, 1, 2]
    for i, (t, off, n, shape) in enumerate(slots):
        assert tuple(esd[i].shape) == shape and torch.equal(esd[i].reshape(-1), e[off:off + n] if off is not None else opt._ema[id(extra)])
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups', 'ema'} and set(sd['ema']) == {'decay', 'params'} and sd['ema']['decay'] == 0.75
    assert list(sd['ema']['params']) == [0, 1, 2] and all(torch.equal(sd['ema']['params'][i], esd[i]) for i in esd)
    assert all(sd['ema']['params'][i].shape == sd['state'][i]['exp_avg'].shape for i in esd)
    ref = [torch.nn.Parameter(torch.zeros(shape)) for _, _, _, shape in slots]
    topt = torch.optim.AdamW(ref, lr=1e-2)
    topt.load_state_dict(sd)                                      # torch ignores the extra key
    assert float(topt.state_dict()['state'][0]['step']) == 3.0
    # the context
    live, live_x, avg = tw.flat.clone(), extra.detach().clone(), e.clone()
    tw.wcache_dirty = False
    with opt.ema_weights() as inside:
        assert inside is opt and tw.wcache_dirty
        assert torch.equal(tw.flat[mask], avg[mask]) and torch.equal(tw.flat[~mask], live[~mask]) and torch.equal(e[mask], live[mask])
        assert torch.equal(extra.detach().reshape(-1), esd[2].reshape(-1))
        tw.wcache_dirty = False
        for fn, what in ((opt.step, 'step'), (opt.state_dict, 'state_dict'), (lambda: opt.load_state_dict(sd), 'load_state_dict'), (opt.ema_state_dict, 'ema_state_dict')):
            with pytest.raises(RuntimeError, match=what + ': inside ema_weights'):
                fn()
        with pytest.raises(RuntimeError, match='already inside'):
            with opt.ema_weights():
                pass
        assert opt._ema_in_use and torch.equal(tw.flat[mask], avg[mask])           # (the refused nesting exchanged nothing)
    assert tw.wcache_dirty and not opt._ema_in_use and opt.step_count == 3
    assert torch.equal(tw.flat, live) and torch.equal(e, avg) and torch.equal(extra.detach(), live_x)
    # None freezes the average and keeps it; the plain path runs again
    opt.ema_decay = None
    type(opt)._adamw = lambda self, p, g, m, v, zero_grad, st, *s: p.sub_(1e-3 * g)
    opt.step()
    assert torch.equal(e, avg) and not torch.equal(tw.flat, live) and 'ema' in opt.state_dict()
    # load: with 'ema' restored, without it dropped
    tw2 = _FakeTower(TOTAL, TRAINABLE, 1)
    extra2 = torch.nn.Parameter(extra.detach().clone())
    opt2 = _rehearsal()([tw2], lr=1e-2, weight_decay=1e-2, extra_params=[extra2])
    opt2.load_state_dict(sd)
    assert opt2.ema_decay == 0.75 and opt2.step_count == 3 and all(torch.equal(a, b) for a, b in zip(opt2.ema_state_dict().values(), esd.values()))
    assert torch.equal(opt2._ema[id(tw2)][~mask], tw2.flat[~mask])
    opt2.load_state_dict({k: v for k, v in sd.items() if k != 'ema'})
    assert not opt2._has_ema() and opt2.ema_decay == 0.75
    tw2.flat_grad.zero_()
    extra2.grad = torch.zeros(16, 8)
    before = tw2.flat.clone()
    opt2.step()
    want = before.double() + 0.25 * (tw2.flat.double() - before.double())
    assert torch.allclose(opt2._ema[id(tw2)].double(), want, rtol=1e-6, atol=1e-7)


def test_an_odd_range_is_refused_before_the_step_counter_moves():
    from distillclip_amd.optim import FusedAdamW
    tw = _FakeTower(64, [[4, 11], [16, 32]], 3)
    opt = FusedAdamW([tw], ema_decay=0.9)                         # the product hooks: nothing is launched, the refusal comes first
    before = tw.flat.clone()
    with pytest.raises(ValueError, match=r'tower 0 range \[4, 11\) has 7 elements.*EMA'):
        opt.step()
    assert opt.step_count == 0 and opt._ema == {} and opt._state == {} and torch.equal(tw.flat, before)
    tw = _FakeTower(64, [[2, 10]], 3)                             # a multiple of 4 elements, 8 bytes off a 16-byte boundary
    opt = FusedAdamW([tw], ema_decay=0.9)
    with pytest.raises(ValueError, match=r'tower 0 range \[2, 10\)'):
        opt.step()
    odd = torch.nn.Parameter(torch.zeros(2, 3))
    odd.grad = torch.ones(2, 3)
    opt = FusedAdamW([], extra_params=[odd], ema_decay=0.9)
    with pytest.raises(ValueError, match=r'extra parameter 0 \(\(2, 3\)\)'):
        opt.step()
    assert opt.step_count == 0 and opt._ema == {}
    for bad in (-0.1, 1.5, float('nan')):
        opt = _rehearsal()([_FakeTower(TOTAL, TRAINABLE, 1)], ema_decay=bad)
        with pytest.raises(ValueError, match='ema_decay'):
            opt.step()
        assert opt.step_count == 0


def test_a_sharded_tower_is_refused_before_the_step_counter_moves():
    tw = _FakeTower(TOTAL, TRAINABLE, 4)

    def boom(*a, **k):
        raise AssertionError('the refusal must come before anything else')
    tw.dp = types.SimpleNamespace(shard_elems=8, buckets=[])
    tw.sync = types.SimpleNamespace(enabled=True, stream_for=boom, group_for=boom)
    opt = _rehearsal()([tw], ema_decay=0.9)
    assert opt._sharded(tw)
    with pytest.raises(RuntimeError, match=r'ema_decay.*sharded.*DCLIP_DP_MODE=allreduce.*DCLIP_DP_MODE=off'):
        opt.step()
    assert opt.step_count == 0 and opt._ema == {} and opt._state == {}


def test_ema_weight_is_rounded_once_from_the_double_difference():
    from distillclip_amd.optim import FusedAdamW
    opt = FusedAdamW([], ema_decay=0.9999)
    w = opt._ema_weight()
    assert w == float(np.float32(1.0 - 0.9999)) == ec.weight(0.9999)
    naive = float(np.float32(1) - np.float32(0.9999))
    assert abs(naive - 1e-4) / 1e-4 > 1e-4 and abs(w - 1e-4) / 1e-4 < 2.0 ** -24
    opt.ema_decay = None
    assert opt._ema_weight() is None
    for d, want in ((0.0, 1.0), (1.0, 0.0), (0.5, 0.5)):
        opt.ema_decay = d
        assert opt._ema_weight() == want


def test_the_model_hands_its_attributes_to_the_optimizer():
    from distillclip_amd.model._distill_base import DistillBase
    assert DistillBase.ema_decay is None and DistillBase.validate_with_ema is False
    m = DistillBase()
    m.on_validation_start()                                       # no optimizer, no flag: nothing
    m.on_validation_end()
    entered = []
    opt = types.SimpleNamespace(_has_ema=lambda: True)

    class Ctx:
        def __enter__(self):
            entered.append('in')

        def __exit__(self, *a):
            entered.append('out')
    opt.ema_weights = Ctx
    m._optimizer = opt
    m.on_validation_start()
    m.on_validation_end()
    assert entered == []
    m.validate_with_ema = True
    m.on_validation_start()
    m.on_validation_start()                                       # (a second call does not enter twice)
    assert entered == ['in']
    m.on_validation_end()
    m.on_validation_end()
    assert entered == ['in', 'out']
    opt._has_ema = lambda: False
    m.on_validation_start()
    m.on_validation_end()
    assert entered == ['in', 'out']


# ---- reference and bound -------------------------------------------------------------------------------------------------------------------------
def test_the_emulated_kernel_stays_inside_the_bound_on_every_gpu_case():
    n = sum(ec.LENS5)
    worst, worst_wide = 0.0, 0.0
    for fam in ec.FAMILIES:
        e, p = ec.family(fam, n, seed=2)
        for w in ec.WEIGHTS:
            got = ec.emulate(e, p, w)
            r, i = ec.ratio(got, e, p, w)
            assert r <= 1, (fam, w, i, r)
            worst = max(worst, r)
            if w == 0.0 or fam == 'equal':
                assert np.array_equal(ec.bits(got), ec.bits(e))
            # a rounded product and a rounded sum: inside the issue's bound, u (2 |w d| + |e'|) (1 + 4 u)
            two = ec.emulate(e, p, w, fma=False).astype(np.float64)
            ref = ec.reference(e, p, w)
            wide = ec.U * (2 * np.abs(w * (p.astype(np.float64) - e)) + np.abs(ref)) * (1 + 4 * ec.U) + ec.S
            worst_wide = max(worst_wide, float((np.abs(two - ref) / wide).max()))
    print(f'worst err / bound: fused {worst:.4f}, product and sum rounded apart against the wider bound {worst_wide:.4f}')
    assert 0.9 < worst <= 1 and worst_wide <= 1                   # (the bound is not slack: the tie cases reach it)


def test_wrong_forms_fall_outside_the_bound():
    n = sum(ec.LENS5)
    e, p = ec.family('wide', n, seed=2)
    w = ec.weight(0.9999)
    f = np.float32
    naive_w = f(1) - f(0.9999)                                    # 1.66e-4 off
    forms = {'f32 1 - decay': ec.emulate(e, p, naive_w), 'decay * e + w * p with decay = 1 - w in f32': f(1 - w) * e + f(w) * p,
             'old p': e.copy(), 'w applied to p alone': e + f(w) * p}
    for name, got in forms.items():
        assert ec.ratio(got, e, p, w)[0] > 1, name


def test_the_long_range_takes_three_trips():
    lens, S, long4 = ec.lens24()
    assert len(lens) == 24 and all(n % 4 == 0 for n in lens) and sum(lens) < 800_000
    assert (long4 + S - 1) // S == 3 and long4 % S == 77
