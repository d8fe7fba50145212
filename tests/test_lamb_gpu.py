"""Layer-wise trust ratios on the device: dclip_lamb_table through the C entry on guarded buffers (sections 1-5), FusedAdamW(trust_ratio=True)
on the tiny two-tower model and the recorded backwards of tests/test_ema_gpu.py (section 6).  Cases, the float64 restatement and the derived
bounds: tests/lamb_cases.py.

Every call runs on guarded copies: NaN guard words around p, g, m, v, e, a workspace of exactly dclip_lamb_workspace_bytes in front of a
patterned guard, stats between patterned guards; guards and frozen gaps are compared bit for bit after every call.

m', v' ARE COMPARED BIT FOR BIT with dclip_adamw_table on the same inputs.  That holds by construction: both kernels call adam_moments()
(csrc/optim_elem.h) on the same g' = g * gs, and a skipped step writes neither.  They are held to the float64 bound of tests/adamw_cases.py
as well.

MEASURED on one MI355X with `pytest tests/test_lamb_gpu.py -m gpu -s` (37 passed in 6 s).  Worst err / bound per case family, as (|p|, |u|, r, p'):
by count and mode, EMA on and off: 1 range (0.05, 0.07, 0.04, 0.990), 7 (0.08, 0.10, 0.06, 0.996), 25 (0.13, 0.11, 0.12, 0.998), 70 (0.21, 0.18, 0.14, 0.997),
plain, gscale and AMP record alike; by input family over 25 ranges: normal (0.13, 0.14, 0.11, 0.998), tiny (0.18, 0.14, 0.07, 0.992), first (0.16, 0.05,
0.07, 0.978), cancel (0.16, 0.05, 0.03, 0.948), big (0.16, 0.12, 0.07, 0.995), sub (0.14, 0.15, 0.09, 0.991); m' at most 0.49, v' 0.39.  p' sits just below 1
by nature: it is ONE rounding of an fmaf whose other error terms are orders below u |p'|, so the worst of 10^5 elements lies at half an ulp just above a
power of two; the bound is sharp there, not loose elsewhere.  Section 6: worst err / tolerance 0.013 after three steps in every variant (0.008 with the
skipped step), the statistics inside their bounds."""
import numpy as np
import pytest
import torch

import adamw_cases as ac
import adamw_groups_cases as gc
import ema_cases as ec
import lamb_cases as lc
import test_ema_gpu as eg
from test_ema_gpu import recorded                        # noqa: F401  (module-scoped fixture: three recorded backwards of the tiny model)
from test_grad_clip_gpu import _tolerance

pytestmark = pytest.mark.gpu

W = ec.weight(0.9)
GS = 0.3172
PATTERN = 0x5A


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _ops():
    from distillclip_amd import ops
    assert ops.ADAMW_TABLE_TILE == gc.TILE
    return ops


def _small(words, at=4):
    host = np.full(at + len(words) + 4, gc.GUARD_BITS, dtype=np.uint32).view(np.float32)
    host[at:at + len(words)] = words
    return torch.from_numpy(host.copy()).cuda(), host, at


def _record(t, mult=1.0, skip=0.0):
    bc1, bc2s = ac.exact_bc(ac.HYPER, t)
    return [float(np.float32(mult)), skip, float(bc1), float(bc2s), np.nan, np.nan, np.nan, np.nan]


def run(flat, ranges, mode, t, zero_grad=0, ema=False, clip=None, adapt=False, gs=GS, record=None, eps=None, twice=False, adamw=False, stats_in=None):
    """one dclip_lamb_table call (adamw: one dclip_adamw_table call) over guarded copies of flat = {name: f32 [total]}
    -> ({name: the guarded buffer after the call}, stats f32 [count, 4]).  Checked here: the multiplier / record, the guard behind the
    workspace and the guards around stats are untouched; twice: a second identical call on fresh copies gives the same bits."""
    lib, ops = _lib(), _ops()
    lr, b1, b2, eps0, _ = ac.HYPER
    eps = eps0 if eps is None else eps
    names = 'pgmv' + ('e' if ema else '')
    total, count = flat['p'].size, len(ranges)
    dev = {k: torch.from_numpy(gc.guarded(flat[k]).copy()).cuda() for k in names}
    base = {k: d.data_ptr() + 4 * gc.GUARD for k, d in dev.items()}
    assert all(x % 16 == 0 for x in base.values())
    small = None
    if mode == 'scaled':
        small = _small([gs], at=5)
    elif mode == 'amp':
        small = _small(_record(t, gs) if record is None else record)
    sp = None if small is None else small[0].data_ptr() + 4 * small[2]
    gscale, rec = (sp if mode == 'scaled' else None), (sp if mode == 'amp' else None)
    st = torch.cuda.current_stream().cuda_stream
    image, tiles = ops.adamw_table_image(list(ranges), total)
    assert tiles == gc.tile0_of(ranges)[-1]
    tab = image.cuda()
    stats = None
    if adamw:
        lib.dclip_adamw_table(base['p'], base['g'], base['m'], base['v'], base.get('e'), tab.data_ptr(), count, tiles, lr, b1, b2, eps, t, zero_grad,
                              W if ema else 0.0, gscale, rec, st)
        torch.cuda.synchronize()
    else:
        need = lib.dclip_lamb_workspace_bytes(count, tiles)
        assert need == 16 * tiles
        ws = torch.full((need + 64,), PATTERN, dtype=torch.uint8).cuda()
        s_host = np.full((count + 2, 4), np.float32(-7.5), dtype=np.float32) if stats_in is None else np.concatenate([np.full((1, 4), np.float32(-7.5)), stats_in, np.full((1, 4), np.float32(-7.5))]).astype(np.float32)
        s_dev = torch.from_numpy(s_host.copy()).cuda()
        assert ws.data_ptr() % 16 == 0 and s_dev.data_ptr() % 16 == 0
        lib.dclip_lamb_table(base['p'], base['g'], base['m'], base['v'], base.get('e'), tab.data_ptr(), count, tiles, lr, b1, b2, eps, t, zero_grad,
                             W if ema else 0.0, gscale, rec, -1.0 if clip is None else clip, 1 if adapt else 0, ws.data_ptr(), need, s_dev.data_ptr() + 16, st)
        torch.cuda.synchronize()
        assert (ws[need:].cpu().numpy() == PATTERN).all(), 'written past the workspace of the queried size'
        s_got = s_dev.cpu().numpy()
        assert np.array_equal(gc.bits(s_got[[0, -1]]), gc.bits(s_host[[0, -1]])), 'written outside stats'
        stats = s_got[1:-1]
    if small is not None:
        assert np.array_equal(gc.bits(small[0].cpu().numpy()), gc.bits(small[1]))
    got = {k: d.cpu().numpy() for k, d in dev.items()}
    if twice:
        again, s2 = run(flat, ranges, mode, t, zero_grad, ema, clip, adapt, gs, record, eps, False, adamw, stats_in)
        for k in names:
            assert np.array_equal(gc.bits(got[k]), gc.bits(again[k])), f'a second call gave other bits in {k}'
        assert stats is None or np.array_equal(gc.bits(stats), gc.bits(s2)), 'a second call gave other statistics'
    return got, stats


def _untouched_outside(got, flat, ranges, what):
    """guard words and frozen gaps, bit for bit"""
    mask = np.concatenate([np.zeros(gc.GUARD, bool), gc.inside_mask(ranges, flat['p'].size), np.zeros(gc.GUARD, bool)])
    for k, buf in got.items():
        assert np.array_equal(gc.bits(buf)[~mask], gc.bits(gc.guarded(flat[k]))[~mask]), f'{what}: {k} was written outside the ranges'
    return mask


def _inner(got):
    return {k: b[gc.GUARD:-gc.GUARD] for k, b in got.items()}


def _pairs(mode, t):
    return [ac.exact_bc(ac.HYPER, t)] if mode == 'amp' else ac.candidates(ac.HYPER, t)


# ---- 1. the three modes, the average on and off, every count: float64 and the moments of dclip_adamw_table ----------------------------------------
@pytest.mark.parametrize('mode', ['plain', 'scaled', 'amp'])
@pytest.mark.parametrize('count', lc.COUNTS)
def test_1_every_mode_and_count_inside_the_float64_bounds(count, mode):
    ranges, total = lc.units_of(count)
    flat, _ = gc.inputs(count)
    gs = None if mode == 'plain' else GS
    worst = {}
    for ema in (False, True):
        for zero_grad, adapt in ((0, False), (1, True)):
            t = 7 if zero_grad else 1
            got, stats = run(flat, ranges, mode, t, zero_grad, ema, adapt=adapt, twice=True)
            mask = _untouched_outside(got, flat, ranges, (count, mode, ema, zero_grad))
            res = lc.judge(flat, _inner(got), stats, ranges, lc.H4, _pairs(mode, t), gs, None, adapt, label=f'count {count} {mode} ema {ema} t {t}')
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in res.items()}
            old, _ = run(flat, ranges, mode, t, zero_grad, ema, adamw=True)
            for k in 'mvg':                                  # shared moment code: bit for bit what the AdamW table kernel leaves
                assert np.array_equal(gc.bits(got[k]), gc.bits(old[k])), f'{k} differs from dclip_adamw_table (count {count}, {mode})'
            assert (gc.bits(got['g'])[mask] == 0).all() if zero_grad else np.array_equal(gc.bits(got['g']), gc.bits(gc.guarded(flat['g'])))
            undecayed = np.array([np.float32(r[3]) == 0 for r in ranges])
            assert np.array_equal(gc.bits(stats[:, 3]), np.zeros(count, np.uint32))
            if not adapt:
                assert (gc.bits(stats[undecayed, 2]) == gc.bits(np.float32(1))).all()      # wd_k == 0: r_k is 1, bit for bit
            assert count == 1 or adapt or undecayed.any()
            if ema:                                          # the average follows the p' the call wrote
                p2, e0 = _inner(got)['p'][mask[gc.GUARD:-gc.GUARD]], np.asarray(flat['e'])[mask[gc.GUARD:-gc.GUARD]]
                assert ec.ratio(_inner(got)['e'][mask[gc.GUARD:-gc.GUARD]], e0, p2, W)[0] <= 1
    print(f'count {count} {mode}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('fam', lc.FAMILIES)
def test_1_every_input_family_inside_the_float64_bounds(fam):
    count = 25
    ranges, total = lc.units_of(count)
    flat, gs = gc.inputs(count, fam)
    worst = {}
    for t in [t for t in (1, 1000) if t in ac.steps_of(fam)]:
        mode = 'plain' if gs is None else 'scaled'
        got, stats = run(flat, ranges, mode, t, gs=gs, adapt=(t == 1000))
        _untouched_outside(got, flat, ranges, fam)
        res = lc.judge(flat, _inner(got), stats, ranges, lc.H4, _pairs(mode, t), gs, None, t == 1000, label=f'{fam} t = {t}')
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in res.items()}
    print(f'{fam}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


# ---- 2. exact cases --------------------------------------------------------------------------------------------------------------------------------
def test_2_an_all_zero_p_unit_has_ratio_one():
    flat, ranges, total = lc.planted('zero_p')
    got, stats = run(flat, ranges, 'plain', 3, adapt=True)
    _untouched_outside(got, flat, ranges, 'zero_p')
    zero = np.arange(len(ranges)) % 3 == 0
    assert (gc.bits(stats[zero, 2]) == gc.bits(np.float32(1))).all() and (stats[zero, 0] == 0).all() and (stats[zero, 1] > 0).all()
    assert (stats[~zero, 2] != 1).all()
    lc.judge(flat, _inner(got), stats, ranges, lc.H4, _pairs('plain', 3), None, None, True, label='zero_p')


def test_2_an_all_zero_update_has_ratio_one_and_leaves_p():
    flat, ranges, total = lc.planted('zero_u')
    got, stats = run(flat, ranges, 'plain', 3, adapt=True)
    _untouched_outside(got, flat, ranges, 'zero_u')
    p_in, p_out = gc.bits(np.asarray(flat['p'])), gc.bits(_inner(got)['p'])
    for k, (b, n, s, _) in enumerate(ranges):
        if k % 3 == 0:
            assert gc.bits(stats[k, 2:3])[0] == gc.bits(np.float32(1)) and stats[k, 1] == 0 and stats[k, 0] > 0
            assert np.array_equal(p_out[b:b + n], p_in[b:b + n])
        elif s > 0:
            assert stats[k, 2] != 1 and not np.array_equal(p_out[b:b + n], p_in[b:b + n])


def test_2_trust_clip_is_met_exactly():
    flat, ranges, total = lc.planted('clip')
    h, pairs = lc.H4, _pairs('plain', 3)
    free = lc.reference(flat, ranges, h, *pairs[0], None, None, True)['rfree']
    above = np.arange(len(ranges)) % 2 == 0
    assert (free[above] > 5 * lc.CLIP).all() and (free[~above] < lc.CLIP / 5).all()      # the float64 reference decides every unit
    got, stats = run(flat, ranges, 'plain', 3, clip=lc.CLIP, adapt=True)
    _untouched_outside(got, flat, ranges, 'clip')
    assert (gc.bits(stats[above, 2]) == gc.bits(np.float32(lc.CLIP))).all() and (stats[~above, 2] < lc.CLIP / 5).all()
    lc.judge(flat, _inner(got), stats, ranges, h, pairs, None, lc.CLIP, True, label='clip')


# ---- 3. exact invariants, eps = 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', lc.KS)
def test_3_scaling_the_gradient_and_the_moments_changes_nothing(k):
    ranges, total = lc.units_of(25)
    flat, _ = gc.inputs(25)
    base, s0 = run(flat, ranges, 'plain', 3, adapt=True, eps=0.0)
    got, s1 = run(lc.scaled(flat, k, 'gmv'), ranges, 'plain', 3, adapt=True, eps=0.0)
    assert np.array_equal(gc.bits(base['p']), gc.bits(got['p'])) and np.array_equal(gc.bits(s0[:, 2]), gc.bits(s1[:, 2]))
    assert not np.array_equal(gc.bits(base['m']), gc.bits(got['m'])) and (s0[:, 2] != 1).any()


@pytest.mark.parametrize('k', lc.KS)
def test_3_scaling_p_scales_the_step_without_weight_decay(k):
    ranges, total = lc.units_of(25, 0.0)
    flat, _ = gc.inputs(25)
    base, s0 = run(flat, ranges, 'plain', 3, adapt=True, eps=0.0)
    got, s1 = run(lc.scaled(flat, k, 'p'), ranges, 'plain', 3, adapt=True, eps=0.0)
    mask = np.concatenate([np.zeros(gc.GUARD, bool), gc.inside_mask(ranges, total), np.zeros(gc.GUARD, bool)])
    assert np.array_equal(gc.bits(base['p'][mask] * np.float32(2.0 ** k)), gc.bits(got['p'][mask]))
    assert np.array_equal(gc.bits(s0[:, 2] * np.float32(2.0 ** k)), gc.bits(s1[:, 2])) and np.array_equal(gc.bits(s0[:, 1]), gc.bits(s1[:, 1]))
    live = np.concatenate([np.zeros(gc.GUARD, bool), gc.inside_mask([r for r in ranges if r[2] > 0], total), np.zeros(gc.GUARD, bool)])
    assert (gc.bits(base['p'])[live] != gc.bits(gc.guarded(flat['p']))[live]).mean() > 0.9


# ---- 4. a skipped step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_4_a_skipped_step_changes_nothing_but_g(zero_grad):
    ranges, total = lc.units_of(25)
    flat, _ = gc.inputs(25)
    before = np.random.RandomState(3).randn(25, 4).astype(np.float32)
    for g in (flat['g'], np.full_like(flat['g'], np.nan)):
        f = dict(flat, g=g)
        got, stats = run(f, ranges, 'amp', 9, zero_grad, True, adapt=True, record=[np.nan, 1.0, np.nan, np.nan, 0, 0, 0, 0], stats_in=before)
        mask = _untouched_outside(got, f, ranges, 'skipped')
        for k in 'pmve':
            assert np.array_equal(gc.bits(got[k]), gc.bits(gc.guarded(f[k]))), k
        assert np.array_equal(gc.bits(stats), gc.bits(before))
        assert (gc.bits(got['g'])[mask] == 0).all() if zero_grad else np.array_equal(gc.bits(got['g']), gc.bits(gc.guarded(g)))


# ---- 5. the wrapper --------------------------------------------------------------------------------------------------------------------------------
def test_5_ops_wrappers():
    ops = _ops()
    ranges, total = lc.units_of(7)
    flat, _ = gc.inputs(7)
    t = {k: torch.from_numpy(np.array(flat[k])).cuda() for k in gc.NAMES}
    image, tiles = ops.adamw_table_image(list(ranges), total)
    lr, b1, b2, eps, _ = ac.HYPER
    ws, stats = ops.lamb_buffers(7, tiles, 'cuda')
    assert ws.numel() == 16 * tiles and tuple(stats.shape) == (7, 4)
    ops.lamb_table(t['p'], t['g'], t['m'], t['v'], t['e'], image.cuda(), 7, tiles, lr, (b1, b2), eps, 2, ws, stats, False, W, trust_clip=lc.CLIP, always_adapt=True)
    want, s = run(flat, ranges, 'plain', 2, 0, True, clip=lc.CLIP, adapt=True)
    for k in gc.NAMES:
        assert np.array_equal(gc.bits(t[k].cpu().numpy()), gc.bits(want[k][gc.GUARD:-gc.GUARD])), k
    assert np.array_equal(gc.bits(stats.cpu().numpy()), gc.bits(s))
    with pytest.raises(ValueError, match='one length'):
        ops.lamb_table(t['p'], t['g'][:-4], t['m'], t['v'], None, image.cuda(), 7, tiles, lr, (b1, b2), eps, 2, ws, stats)
    with pytest.raises(ValueError, match='workspace needs'):
        ops.lamb_table(t['p'], t['g'], t['m'], t['v'], None, image.cuda(), 7, tiles, lr, (b1, b2), eps, 2, ws[:-16], stats)
    with pytest.raises(RuntimeError):
        ops.lamb_table(t['p'].cpu(), t['g'], t['m'], t['v'], None, image.cuda(), 7, tiles, lr, (b1, b2), eps, 2, ws, stats)


# ---- 6. the optimizer on the tiny dual model of tests/test_ema_gpu.py --------------------------------------------------------------------------------
LR, CLIP_NORM = 1e-3, 0.5


def _build(groups=None, ema_decay=None, **trust):
    from distillclip_amd.optim import FusedAdamW, no_decay_groups
    model, _ = eg._build(None)
    model.optimizer_groups, model.ema_decay = (no_decay_groups if groups else None), ema_decay
    for k, x in trust.items():
        setattr(model, k, x)
    (opt,), _ = model.configure_optimizers()
    assert isinstance(opt, FusedAdamW) and opt.trust_ratio == bool(trust.get('trust_ratio'))
    opt.lr = LR
    return model, opt


def _units(model, opt):
    """[(tower index, begin, length, lr_scale, weight_decay)] in the order of the rows of last_trust_stats"""
    return [(i, a, b - a, s, wd) for i, tw in enumerate(model.towers()) for a, b, s, wd in opt._group_ranges(tw, units=True)]


@pytest.mark.parametrize('variant', ['plain', 'groups', 'ema', 'groups_ema', 'scaler_overflow'])
def test_6_three_clipped_steps_against_the_float64_restatement(recorded, variant):
    groups, ema = variant.startswith('groups'), variant.endswith('ema')
    model, opt = _build(groups, eg.DECAY if ema else None, trust_ratio=True)
    opt.max_grad_norm = CLIP_NORM
    towers = model.towers()
    units = _units(model, opt)
    names = opt.trust_units()
    assert [len(names[i]) for i in range(len(towers))] == [sum(1 for u in units if u[0] == i) for i in range(len(towers))]
    assert all(n > 1 for n in map(len, names.values())) and (not groups or any(u[4] == 0 for u in units)) and (groups or all(u[4] == opt.weight_decay for u in units))
    b1, b2 = (float(np.float32(x)) for x in opt.betas)
    eps, lr = float(np.float32(opt.eps)), float(np.float32(LR))
    p64 = [tw.flat.double().cpu().numpy() for tw in towers]
    m64, v64 = [np.zeros_like(p) for p in p64], [np.zeros_like(p) for p in p64]
    e64 = [p.copy() for p in p64]
    scaler = torch.amp.GradScaler('cuda', init_scale=eg.SCALE) if variant == 'scaler_overflow' else None
    batches, t, worst = eg._batches(), 0, 0.0
    for i in range(3):
        overflow = variant == 'scaler_overflow' and i == 1
        mult = 1.0 if scaler is None else eg.SCALE / scaler.get_scale()
        before = [tw.flat.clone() for tw in towers] + [s.clone() for s in opt.last_trust_stats.values()]
        eg._step(model, opt, batches[i], recorded[i], scaler, overflow)
        if overflow:                                         # the skipped step moved nothing, the statistics included
            after = [tw.flat for tw in towers] + list(opt.last_trust_stats.values())
            assert len(before) == len(after) == 2 * len(towers) and all(eg._eq(a, b) for a, b in zip(before, after))
            continue
        t += 1
        g64 = [g.double().cpu().numpy() * mult for g in recorded[i]]
        inside = [np.zeros(p.size, bool) for p in p64]
        for i_tw, a, n, _, _ in units:
            inside[i_tw][a:a + n] = True
        norm = float(np.sqrt(sum(float(np.sum(g[k] ** 2)) for g, k in zip(g64, inside))))
        assert abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm                              # global, formed before the ratios
        coef = min(1.0, CLIP_NORM / (norm + 1e-6))
        bc1, bc2s = 1 - b1 ** t, float(np.sqrt(1 - b2 ** t))
        stats = {i_tw: opt.last_trust_stats[i_tw].cpu().numpy() for i_tw in range(len(towers))}
        row = {i_tw: 0 for i_tw in range(len(towers))}
        k1, k2s = (float(x) for x in ac.exact_bc(ac.hyper(LR, opt.betas, opt.eps, 0.0), t))
        own = [(before[i_tw].double().cpu().numpy(),) + tuple(x.double().cpu().numpy() for x in opt._moments(tw)) for i_tw, tw in enumerate(towers)]
        for i_tw, a, n, s, wd in units:
            sl = slice(a, a + n)
            g = g64[i_tw][sl] * coef
            m64[i_tw][sl] = b1 * m64[i_tw][sl] + (1 - b1) * g
            v64[i_tw][sl] = b2 * v64[i_tw][sl] + (1 - b2) * g * g
            wd32 = float(np.float32(wd))
            u = (m64[i_tw][sl] / bc1) / (np.sqrt(v64[i_tw][sl]) / bc2s + eps) + wd32 * p64[i_tw][sl]
            n_p, n_u = float(np.linalg.norm(p64[i_tw][sl])), float(np.linalg.norm(u))
            r = n_p / n_u if wd32 != 0 and n_p > 0 and n_u > 0 else 1.0
            # last_trust_stats against the same run: the norms of the f32 p the step read and of u formed in float64 from the m', v' it left.
            # The kernel's u is 6 roundings from those (two quotients by the bias corrections, the root, the sum with eps, the quotient,
            # the fmaf) from ITS bias corrections k1, k2s: the f32 formulas on the rounded powers (ac.exact_bc), which the host's powf meets
            # within a last bit.  (1 - b2^t cancels in f32 and lies 1e-5 from the float64 value: the float64 ones will not do here.)  Together
            # 8 U of |q| + |wd p| per element;
            # the sums of squares add 5 U to a norm (lamb_cases: G / 2), the f32 result one more; r is the rounded quotient of the double
            # norms whose roundings the two f32 norms are: 3 U, taken as 4.
            got = stats[i_tw][row[i_tw]]
            row[i_tw] += 1
            p0, m1, v1 = (x[sl] for x in own[i_tw])
            q = (m1 / k1) / (np.sqrt(v1) / k2s + eps)
            d_p, d_u = float(np.linalg.norm(p0)), float(np.linalg.norm(q + wd32 * p0))
            assert abs(got[0] - d_p) <= 8 * lc.U * d_p + lc.S and got[3] == 0, (i, i_tw, a, got, d_p)
            assert abs(got[1] - d_u) <= 8 * lc.U * float(np.linalg.norm(np.abs(q) + np.abs(wd32 * p0))) + 8 * lc.U * d_u + lc.S, (i, i_tw, a, got, d_u)
            assert got[2] == 1 if wd32 == 0 else abs(got[2] - float(got[0]) / float(got[1])) <= 4 * lc.U * got[2], (i, i_tw, a, got)
            p64[i_tw][sl] = p64[i_tw][sl] - gc.lr_of(lr, s) * r * u
            if ema:
                e64[i_tw][sl] += ec.weight(eg.DECAY) * (p64[i_tw][sl] - e64[i_tw][sl])
        for i_tw, tw in enumerate(towers):
            for name, a, n in names[i_tw]:
                ref = torch.from_numpy(p64[i_tw][a:a + n])
                err = (tw.flat[a:a + n].double().cpu() - ref).abs().max().item()
                assert _tolerance(err, ref), (variant, i, name, err)
                worst = max(worst, err / (1e-6 + 1e-5 * ref.abs().max().item()))
                if ema:
                    e_ref = torch.from_numpy(e64[i_tw][a:a + n])
                    assert _tolerance((opt._ema[id(tw)][a:a + n].double().cpu() - e_ref).abs().max().item(), e_ref), (variant, i, name)
    assert opt.step_count == 3 and all(opt._tables[id(tw)]['uploads'] == 1 for tw in towers)
    if variant == 'scaler_overflow':
        assert int(opt._skipped) == 1
    print(f'{variant}: worst err / tolerance {worst:.3f}')


def test_6_extra_parameters_are_one_unit_each():
    """parameters outside the towers' flat buffers: each its own one-range layout through the same entry, with its group's values"""
    from distillclip_amd.optim import FusedLAMB
    rs = np.random.RandomState(5)
    shapes = [(64, 128), (64,), (3, 8196)]                # exactly one tile ; less than a trip ; three tiles + 12 elements
    ps = [torch.nn.Parameter(torch.from_numpy((0.05 * rs.randn(*s)).astype(np.float32)).cuda()) for s in shapes]
    grads = [(1e-3 * rs.randn(*s)).astype(np.float32) for s in shapes]
    opt = FusedLAMB([], lr=LR, weight_decay=0.05, extra_params=ps, groups=[{'params': [ps[1]], 'weight_decay': 0.0}, {'params': [ps[2]], 'lr_scale': 0.1}])
    before = [p.detach().cpu().numpy().reshape(-1).copy() for p in ps]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).cuda()
    opt.step()
    torch.cuda.synchronize()
    h5 = ac.hyper(LR, opt.betas, opt.eps, 0.0)
    assert set(opt.last_trust_stats) == {('extra', 0), ('extra', 1), ('extra', 2)} == set(opt.trust_units())
    for j, (scale, wd) in enumerate(((1.0, 0.05), (1.0, 0.0), (0.1, 0.05))):
        n = before[j].size
        flat = dict(p=before[j], g=grads[j].reshape(-1), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
        m, v = opt._extra_state[id(ps[j])]
        got = dict(p=ps[j].detach().cpu().numpy().reshape(-1), m=m.cpu().numpy(), v=v.cpu().numpy())
        stats = opt.last_trust_stats[('extra', j)].cpu().numpy()
        lc.judge(flat, got, stats, ((0, n, scale, wd),), h5[:4], ac.candidates(h5, 1), None, None, False, label=f'extra parameter {j}')
        assert (stats[0, 2] == 1) == (wd == 0) and not np.array_equal(got['p'], before[j])


def test_6_trust_ratio_off_is_bit_equal_to_an_optimizer_built_without_it(recorded):
    from distillclip_amd.optim import FusedAdamW, FusedLAMB
    batches = eg._batches()
    m0, _ = eg._build(None)
    extras = lambda m: [p for tw in m.towers() for p in getattr(tw.module, 'extra_parameters', lambda: [])()]
    o0 = FusedAdamW(m0.towers(), lr=LR, weight_decay=m0.hparams.weight_decay, extra_params=extras(m0))             # built without the argument
    m1, o1 = _build(trust_ratio=False, trust_clip=2.0, always_adapt=True)
    for i in range(2):
        eg._step(m0, o0, batches[i], recorded[i])
        eg._step(m1, o1, batches[i], recorded[i])
    for a, b in zip(eg._state(m0, o0), eg._state(m1, o1)):
        assert eg._eq(a, b)
    assert o1._tables == {} and o1._lamb == {} and o1.last_trust_stats == {} and 'trust_ratio' not in o1.state_dict()['param_groups'][0]
    # switching on between steps is well defined, and overlap / join=False composes
    o1.trust_ratio = True
    eg._step(m1, o1, batches[2], recorded[2], overlap=True, join=False)
    m2, _ = eg._build(None)
    o2 = FusedLAMB(m2.towers(), lr=LR, weight_decay=m2.hparams.weight_decay, extra_params=extras(m2), trust_clip=2.0, always_adapt=True)
    assert o2.trust_ratio
    for i in range(2):
        o2.trust_ratio = False
        eg._step(m2, o2, batches[i], recorded[i])
    o2.trust_ratio = True
    eg._step(m2, o2, batches[2], recorded[2])
    for a, b in zip(eg._state(m1, o1), eg._state(m2, o2)):
        assert eg._eq(a, b)
    assert not all(eg._eq(a, b) for a, b in zip(eg._params(o0), eg._params(o1)))
    sd = o1.state_dict()
    assert all(g['trust_ratio'] is True and g['trust_clip'] == 2.0 and g['always_adapt'] is True for g in sd['param_groups'])
