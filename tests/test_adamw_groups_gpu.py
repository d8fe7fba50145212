"""AdamW with per-range hyper-parameters, on the device: dclip_adamw_table through the C entry (sections 1-3), FusedAdamW(groups=...) on
the tiny two-tower model of tests/test_ema_gpu.py (section 4).  Cases, layouts and the yardstick: tests/adamw_groups_cases.py.

Sections 1 and 2 know no tolerance: the table entry is compared bit for bit, guard words and frozen gaps included, with the existing
entries called range by range.  Section 3 holds it to float64 inside tests/adamw_cases.py's derived bound, each range with its own
hyper-parameters.  Section 4 compares three optimizer steps with torch.optim.AdamW on float64 CPU clones built with the same groups.
Its bound for the parameters is the one every optimizer-level comparison with torch.optim.AdamW here uses, imported from
tests/test_grad_clip_gpu.py (`_tolerance`: err <= 1e-6 + 1e-5 max |ref| per tensor; tests/test_ema_gpu.py has no bound of its own for
parameters against torch, its twins are compared bit for bit); the average is held to the float64 recurrence within the sum of the
per-step bounds of tests/ema_cases.py, as tests/test_ema_gpu.py::test_7_twins does for three steps.  Model, batches, recorded gradients
and the step helper are imported from tests/test_ema_gpu.py.

MEASURED on one MI355X with `pytest tests/test_adamw_groups_gpu.py -m gpu -s` (32 passed in 6 s).  Sections 1 and 2: every bit equal.  Section 3:
worst err / bound over the 25 ranges 0.46 (normal), 0.47 (tiny), 0.39 (first), 0.39 (cancel), 0.49 (big), 0.48 (sub).  Section 4: worst err / tolerance
0.014 after three steps in every variant (0.009 with the skipped step), the average inside the summed bounds."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_cases as ac
import adamw_groups_cases as gc
import ema_cases as ec
import test_ema_gpu as eg
from test_ema_gpu import recorded                        # noqa: F401  (module-scoped fixture: three recorded backwards of the tiny model)
from test_grad_clip_gpu import _tolerance

pytestmark = pytest.mark.gpu

W = ec.weight(0.9)
GS = 0.3172


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


def run(flat, ranges, mode, t, zero_grad, ema, table, gs=GS, record=None, twice=False):
    """one step over guarded copies of flat = {name: f32 [total]}.  table=True: ONE dclip_adamw_table launch; False: the existing entry of
    `mode` (with ema: dclip_adamw_multi_ema), one call per range with that range's lr_k and wd_k.  -> {name: the guarded buffer after the
    call}; the multiplier / the record have been checked to be untouched.  twice: a second identical call on fresh copies must give
    the same bits."""
    lib, ops = _lib(), _ops()
    lr, b1, b2, eps, _ = ac.HYPER
    names = 'pgmv' + ('e' if ema else '')
    total = flat['p'].size
    host = {k: gc.guarded(flat[k]) for k in names}
    dev = {k: torch.from_numpy(b.copy()).cuda() for k, b in host.items()}
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
    if table:
        image, tiles = ops.adamw_table_image(list(ranges), total)
        assert tiles == gc.tile0_of(ranges)[-1]
        tab = image.cuda()
        lib.dclip_adamw_table(base['p'], base['g'], base['m'], base['v'], base.get('e'), tab.data_ptr(), len(ranges), tiles, lr, b1, b2, eps, t, zero_grad,
                              W if ema else 0.0, gscale, rec, st)
    else:
        one = lambda x: (ctypes.c_void_p * 1)(x)
        for b, n, s, wd in ranges:
            a = {k: one(base[k] + 4 * b) for k in names}
            n1, lrk = (ctypes.c_int64 * 1)(n), gc.lr_of(lr, s)
            if ema:
                lib.dclip_adamw_multi_ema(a['p'], a['g'], a['m'], a['v'], a['e'], n1, 1, lrk, b1, b2, eps, wd, t, zero_grad, W, gscale, rec, st)
            elif mode == 'plain':
                lib.dclip_adamw_multi(a['p'], a['g'], a['m'], a['v'], n1, 1, lrk, b1, b2, eps, wd, t, zero_grad, st)
            elif mode == 'scaled':
                lib.dclip_adamw_multi_scaled(a['p'], a['g'], a['m'], a['v'], n1, 1, lrk, b1, b2, eps, wd, t, zero_grad, gscale, st)
            else:
                lib.dclip_adamw_multi_amp(a['p'], a['g'], a['m'], a['v'], n1, 1, lrk, b1, b2, eps, wd, zero_grad, rec, st)
    torch.cuda.synchronize()
    if small is not None:
        assert np.array_equal(gc.bits(small[0].cpu().numpy()), gc.bits(small[1]))
    got = {k: d.cpu().numpy() for k, d in dev.items()}
    if twice:
        again = run(flat, ranges, mode, t, zero_grad, ema, table, gs, record)
        for k in names:
            assert np.array_equal(gc.bits(got[k]), gc.bits(again[k])), f'a second call gave other bits in {k}'
    return got


def _untouched_outside(got, flat, ranges, what):
    """guard words and frozen gaps, bit for bit"""
    mask = np.concatenate([np.zeros(gc.GUARD, bool), gc.inside_mask(ranges, flat['p'].size), np.zeros(gc.GUARD, bool)])
    for k, buf in got.items():
        assert np.array_equal(gc.bits(buf)[~mask], gc.bits(gc.guarded(flat[k]))[~mask]), f'{what}: {k} was written outside the ranges'
    return mask


# ---- 1. bit equality with the existing kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['plain', 'scaled', 'amp'])
@pytest.mark.parametrize('count', gc.COUNTS)
def test_1_bit_equal_to_the_existing_entries_range_by_range(count, mode):
    ranges, total = gc.ranges_of(count)
    assert len(ranges) == count and (count < 25 or {r[1] for r in ranges} == set(gc.LENGTHS))
    assert count < 7 or ({r[2] for r in ranges} == set(gc.SCALES) and {r[3] for r in ranges} == set(gc.WDS))
    flat, _ = gc.inputs(count)
    for ema in (False, True):
        for zero_grad in (0, 1):
            t = 7 if zero_grad else 1
            old = run(flat, ranges, mode, t, zero_grad, ema, table=False)
            new = run(flat, ranges, mode, t, zero_grad, ema, table=True, twice=True)
            mask = _untouched_outside(new, flat, ranges, (count, mode, ema, zero_grad))
            for k in old:
                same = gc.bits(old[k]) == gc.bits(new[k])
                assert same.all(), f'{k} differs at element {int(np.argmin(same)) - gc.GUARD} (count {count}, {mode}, ema {ema}, zero_grad {zero_grad})'
            g_in = gc.bits(gc.guarded(flat['g']))
            assert (gc.bits(new['g'])[mask] == 0).all() if zero_grad else np.array_equal(gc.bits(new['g']), g_in)
            live = np.concatenate([np.zeros(gc.GUARD, bool), gc.inside_mask([r for r in ranges if r[2] > 0], total), np.zeros(gc.GUARD, bool)])
            p_in = gc.bits(gc.guarded(flat['p']))
            assert (gc.bits(new['p'])[live] != p_in[live]).mean() > 0.9              # (the step did step ...
            assert np.array_equal(gc.bits(new['p'])[mask & ~live], p_in[mask & ~live])   # ... and stood still where lr_k = 0: p (1 - 0 wd) - 0 = p)
            if ema:
                assert not np.array_equal(gc.bits(new['e'])[mask], gc.bits(gc.guarded(flat['e']))[mask])


def test_1_ema_weight_zero_and_no_average_leave_e_alone():
    ranges, total = gc.ranges_of(7)
    flat, _ = gc.inputs(7)
    lib, ops = _lib(), _ops()
    lr, b1, b2, eps, _ = ac.HYPER
    dev = {k: torch.from_numpy(gc.guarded(flat[k]).copy()).cuda() for k in gc.NAMES}
    base = {k: d.data_ptr() + 4 * gc.GUARD for k, d in dev.items()}
    image, tiles = ops.adamw_table_image(list(ranges), total)
    tab = image.cuda()
    lib.dclip_adamw_table(base['p'], base['g'], base['m'], base['v'], base['e'], tab.data_ptr(), 7, tiles, lr, b1, b2, eps, 3, 0, 0.0, None, None,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(gc.bits(dev['e'].cpu().numpy()), gc.bits(gc.guarded(flat['e'])))
    plain = run(flat, ranges, 'plain', 3, 0, False, table=True)
    assert np.array_equal(gc.bits(dev['p'].cpu().numpy()), gc.bits(plain['p']))


# ---- 2. a skipped step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_2_a_skipped_step_changes_nothing_but_g(zero_grad):
    ranges, total = gc.ranges_of(25)
    flat, _ = gc.inputs(25)
    for g in (flat['g'], np.full_like(flat['g'], np.nan)):
        f = dict(flat, g=g)
        got = run(f, ranges, 'amp', 9, zero_grad, True, table=True, record=[np.nan, 1.0, np.nan, np.nan, 0, 0, 0, 0])
        mask = _untouched_outside(got, f, ranges, 'skipped')
        for k in 'pmve':
            assert np.array_equal(gc.bits(got[k]), gc.bits(gc.guarded(f[k]))), k
        assert (gc.bits(got['g'])[mask] == 0).all() if zero_grad else np.array_equal(gc.bits(got['g']), gc.bits(gc.guarded(g)))


# ---- 3. float64 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', ac.FAMILIES)
def test_3_every_range_inside_the_float64_bound_with_its_own_hyper_parameters(fam):
    count = 25
    ranges, total = gc.ranges_of(count)
    flat, gs = gc.inputs(count, fam)
    worst = 0.0
    for t in [t for t in (1, 1000) if t in ac.steps_of(fam)]:
        got = run(flat, ranges, 'plain' if gs is None else 'scaled', t, 0, False, table=True, gs=gs)
        _untouched_outside(got, flat, ranges, fam)
        for k, (b, n, s, wd) in enumerate(ranges):
            h = gc.hyper_of(ranges[k])
            cut = lambda a: np.asarray(a[b:b + n])
            after = tuple(got[x][gc.GUARD + b:gc.GUARD + b + n] for x in 'pmv')
            res = ac.judge(tuple(cut(flat[x]) for x in 'pgmv'), after, h, ac.candidates(h, t), gs, label=f'{fam} t = {t} range {k} (lr_scale {s}, wd {wd})')
            worst = max(worst, res['p'], res['m'], res['v'])
    print(f'{fam}: worst err / bound over the ranges {worst:.3f}')


def test_ops_wrappers():
    ops = _ops()
    ranges, total = gc.ranges_of(7)
    flat, _ = gc.inputs(7)
    t = {k: torch.from_numpy(np.array(flat[k])).cuda() for k in gc.NAMES}
    image, tiles = ops.adamw_table_image(list(ranges), total)
    lr, b1, b2, eps, _ = ac.HYPER
    ops.adamw_table(t['p'], t['g'], t['m'], t['v'], t['e'], image.cuda(), 7, tiles, lr, (b1, b2), eps, 2, False, W)
    want = run(flat, ranges, 'plain', 2, 0, True, table=False)
    for k in gc.NAMES:
        assert np.array_equal(gc.bits(t[k].cpu().numpy()), gc.bits(want[k][gc.GUARD:-gc.GUARD])), k
    with pytest.raises(ValueError, match='one length'):
        ops.adamw_table(t['p'], t['g'][:-4], t['m'], t['v'], None, image.cuda(), 7, tiles, lr, (b1, b2), eps, 2)
    with pytest.raises(ValueError, match='image of 7 ranges'):
        ops.adamw_table(t['p'], t['g'], t['m'], t['v'], None, image.cuda()[:64], 7, tiles, lr, (b1, b2), eps, 2)
    with pytest.raises(RuntimeError):
        ops.adamw_table(t['p'].cpu(), t['g'], t['m'], t['v'], None, image.cuda(), 7, tiles, lr, (b1, b2), eps, 2)


# ---- 4. the optimizer on the tiny dual model of tests/test_ema_gpu.py -----------------------------------------------------------------------------
LR, SCALE_BLOCK = 1e-3, 0.1


DECAY = eg.DECAY


def recipe(model):
    """no_decay_groups + lr_scale = 0.1 on the image student's first block: the block's 1-D parameters leave the no-decay group for a
    group of their own (a parameter is in one group only)"""
    from distillclip_amd.optim import no_decay_groups
    (nd,) = no_decay_groups(model)
    tw = model.towers()[0]
    block = [p for n, p in tw.module.named_parameters() if n.startswith('blocks.0.') and p.requires_grad and any(p is q for q in tw._params())]
    assert block and any(p.dim() <= 1 for p in block) and any(p.dim() > 1 for p in block)
    ids = {id(p) for p in block}
    return [{'params': [p for p in nd['params'] if id(p) not in ids], 'weight_decay': 0.0},
            {'params': [p for p in block if p.dim() > 1], 'lr_scale': SCALE_BLOCK},
            {'params': [p for p in block if p.dim() <= 1], 'lr_scale': SCALE_BLOCK, 'weight_decay': 0.0}]


def trivial(model):
    """every group equal to the defaults"""
    (nd,) = __import__('distillclip_amd.optim', fromlist=['x']).no_decay_groups(model)
    return [{'params': nd['params'][::2], 'weight_decay': model.hparams.weight_decay, 'lr_scale': 1.0}, {'params': nd['params'][1::2]}]


def _build(groups, ema_decay=None):
    from distillclip_amd.optim import FusedAdamW
    model, _ = eg._build(None)
    model.optimizer_groups, model.ema_decay = groups, ema_decay
    (opt,), _ = model.configure_optimizers()
    assert isinstance(opt, FusedAdamW) and (opt.groups is None) == (groups is None)
    opt.lr = LR
    return model, opt


def _torch_twin(model, opt):
    """torch.optim.AdamW on float64 CPU clones, built with the same groups -> (clones in opt._trainable() order, optimizer)"""
    cpu = [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in opt._trainable()]
    groups, at = [], 0
    for g in opt.param_groups:
        n = len(g['params'])
        groups.append({'params': cpu[at:at + n], 'lr': g['lr'], 'weight_decay': g['weight_decay']})
        at += n
    assert at == len(cpu)
    return cpu, torch.optim.AdamW(groups, lr=LR, betas=opt.betas, eps=opt.eps, weight_decay=opt.weight_decay)


def _grads_of(model, opt, flats):
    index = {id(tw): k for k, tw in enumerate(model.towers())}
    return [flats[index[id(tw)]][off:off + n].double().cpu().view(shape) for tw, off, n, shape in opt._slots()]


def _close(opt, cpu, what):
    worst = 0.0
    for i, (p, c) in enumerate(zip(opt._trainable(), cpu)):
        err = (p.detach().double().cpu() - c.detach()).abs().max().item()
        assert _tolerance(err, c.detach()), (what, i, tuple(c.shape), err)
        worst = max(worst, err / (1e-6 + 1e-5 * c.detach().abs().max().item()))
    print(f'{what}: worst err / tolerance {worst:.3f}')


@pytest.mark.parametrize('variant', ['plain', 'clip', 'scaler_overflow', 'ema', 'overlap'])
def test_4_three_steps_against_torch_adamw_with_the_same_groups(recorded, variant):
    model, opt = _build(recipe, DECAY if variant == 'ema' else None)
    assert len(opt.param_groups) == 4 and all(len(opt._group_ranges(tw)) > 3 * len(opt._ranges(tw)) for tw in model.towers())
    cpu, ref = _torch_twin(model, opt)
    start = [p.detach().clone() for p in opt._trainable()]
    scaler = torch.amp.GradScaler('cuda', init_scale=eg.SCALE) if variant == 'scaler_overflow' else None
    if variant == 'clip':
        opt.max_grad_norm = 0.5
    kw = dict(overlap=True, join=False) if variant == 'overlap' else {}
    batches, after = eg._batches(), []
    for i in range(3):
        overflow = variant == 'scaler_overflow' and i == 1
        # (eg._step hands over recorded * eg.SCALE whatever the scaler's scale has become: after the overflow halved it, the step sees 2 g)
        mult = 1.0 if scaler is None else eg.SCALE / scaler.get_scale()
        eg._step(model, opt, batches[i], recorded[i], scaler, overflow, **kw)
        after.append([p.detach().clone() for p in opt._trainable()])
        if overflow:
            assert all(eg._eq(a, b) for a, b in zip(after[0], after[1]))              # the skipped step moved nothing
            continue
        for c, g in zip(cpu, _grads_of(model, opt, recorded[i])):
            c.grad = g * mult
        if variant == 'clip':
            total = torch.nn.utils.clip_grad_norm_(cpu, 0.5)
            assert abs(float(opt.last_grad_norm) - float(total)) <= 1e-5 * float(total)      # global over all groups
        ref.step()
        _close(opt, cpu, f'{variant} step {i + 1}')
    assert opt.step_count == 3 and all(opt._tables[id(tw)]['uploads'] == 1 for tw in model.towers())
    assert not all(eg._eq(a, b) for a, b in zip(start, after[2]))
    if variant == 'scaler_overflow':
        assert int(opt._skipped) == 1
    if variant == 'ema':
        w = ec.weight(DECAY)
        for k, p0 in enumerate(start):
            e = p0.double().cpu().numpy().reshape(-1)
            tol = np.zeros_like(e)
            for i in range(3):
                p2 = after[i][k].cpu().numpy().reshape(-1)
                tol += ec.bound(e, p2, w)
                e = ec.reference(e, p2, w)
            got = opt.ema_state_dict()[k].cpu().numpy().reshape(-1)
            assert float((np.abs(got - e) / tol).max()) <= 1, k


def _three(recorded, groups, **kw):
    model, opt = _build(groups)
    batches = eg._batches()
    for i in range(3):
        eg._step(model, opt, batches[i], recorded[i], **kw)
    torch.cuda.synchronize()
    return model, opt


def test_4_trivial_groups_give_the_bits_of_no_groups(recorded):
    m0, o0 = _three(recorded, None)
    m1, o1 = _three(recorded, trivial)
    assert o0._tables == {} and len(o1.param_groups) == 3 and all(len(o1._group_ranges(tw)) == len(o1._ranges(tw)) for tw in m1.towers())
    flat0 = [tw.flat for tw in m0.towers()] + [t for tw in m0.towers() for t in o0._moments(tw)]
    flat1 = [tw.flat for tw in m1.towers()] + [t for tw in m1.towers() for t in o1._moments(tw)]
    for a, b in zip(flat0, flat1):
        assert eg._eq(a, b)


def test_4_a_layernorm_gain_takes_the_undecayed_update(recorded):
    model, opt = _build(recipe)
    gain = dict(model.towers()[0].module.named_parameters())['norm.weight']
    assert gain.dim() == 1 and any(gain is p for p in opt.groups[0]['params'])
    k = next(i for i, p in enumerate(opt._trainable()) if p is gain)
    p0 = gain.detach().double().cpu()
    eg._step(model, opt, eg._batches()[0], recorded[0])
    g = _grads_of(model, opt, recorded[0])[k]
    b1, b2 = opt.betas
    upd = LR * ((1 - b1) * g / (1 - b1)) / (((1 - b2) * g * g / (1 - b2)).sqrt() + opt.eps)
    undecayed, decayed = p0 - upd, p0 * (1 - LR * opt.weight_decay) - upd
    got = gain.detach().double().cpu()
    assert (undecayed - decayed).abs().min().item() > 5e-6                           # (gains near 1: the decay would show)
    assert _tolerance((got - undecayed).abs().max().item(), undecayed)
    assert (got - decayed).abs().min().item() > 4e-6


def test_4_a_changed_weight_decay_takes_effect_at_the_next_step(recorded):
    model, opt = _build(recipe)
    cpu, ref = _torch_twin(model, opt)
    batches = eg._batches()
    for i in range(3):
        if i == 1:
            opt.groups[0]['weight_decay'] = 0.3
            ref.param_groups[0]['weight_decay'] = 0.3
        eg._step(model, opt, batches[i], recorded[i])
        for c, g in zip(cpu, _grads_of(model, opt, recorded[i])):
            c.grad = g.clone()
        ref.step()
        _close(opt, cpu, f'weight_decay changed, step {i + 1}')
        assert all(opt._tables[id(tw)]['uploads'] == (1 if i == 0 else 2) for tw in model.towers())      # uploaded again once, at the change
    assert opt.param_groups[0]['weight_decay'] == 0.3
    opt.groups[1]['lr_scale'] = float('nan')
    with pytest.raises(ValueError, match='lr_scale'):
        opt.step()
    assert opt.step_count == 3


def test_4_state_dict_round_trips_with_torch_both_ways(recorded):
    from distillclip_amd.checkpoint import trainable_parameters
    model, opt = _build(recipe)
    cpu, ref = _torch_twin(model, opt)
    batches = eg._batches()
    for i in range(2):
        eg._step(model, opt, batches[i], recorded[i])
        for c, g in zip(cpu, _grads_of(model, opt, recorded[i])):
            c.grad = g.clone()
        ref.step()
    sd = opt.state_dict()
    assert len(sd['param_groups']) == 4 and [g['lr_scale'] for g in sd['param_groups']] == [1.0, SCALE_BLOCK, SCALE_BLOCK, 1.0]
    assert sorted(i for g in sd['param_groups'] for i in g['params']) == list(range(len(cpu)))
    # into torch: a float32 twin takes the dict, steps, and its own dict loads back
    cpu32 = [torch.nn.Parameter(p.detach().cpu().clone()) for p in opt._trainable()]
    at, tgroups = 0, []
    for g in opt.param_groups:
        tgroups.append({'params': cpu32[at:at + len(g['params'])]})
        at += len(g['params'])
    topt = torch.optim.AdamW(tgroups, lr=123.0)
    topt.load_state_dict(sd)
    assert [g['lr'] for g in topt.param_groups] == [g['lr'] for g in opt.param_groups] and topt.param_groups[1]['lr_scale'] == SCALE_BLOCK
    assert [g['weight_decay'] for g in topt.param_groups] == [0.0, opt.weight_decay, 0.0, opt.weight_decay]
    back = topt.state_dict()
    model2, opt2 = _build(recipe)
    opt2.load_state_dict(back)
    assert opt2.step_count == 2 and opt2.lr == opt.lr
    for tw, tw2 in zip(model.towers(), model2.towers()):
        tw2.flat.copy_(tw.flat)
        for a, b in zip(opt._moments(tw), opt2._moments(tw2)):
            assert eg._eq(a, b)
    for m_, o_ in ((model, opt), (model2, opt2)):
        eg._step(m_, o_, batches[2], recorded[2])
    for a, b in zip(eg._state(model, opt), eg._state(model2, opt2)):
        assert eg._eq(a, b)
    for c, g in zip(cpu, _grads_of(model, opt, recorded[2])):
        c.grad = g.clone()
    ref.step()
    _close(opt2, cpu, 'the step after loading')
    # the order torch.optim.AdamW would have been built with changes only the default group's numbering
    sd_p = opt.state_dict(trainable_parameters(model))
    assert [len(g['params']) for g in sd_p['param_groups']] == [len(g['params']) for g in sd['param_groups']]
    # another number of groups: refused, both counts named
    _, plain = _build(None)
    with pytest.raises(ValueError, match=r'4 parameter group\(s\), this optimizer 1'):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match=r'1 parameter group\(s\), this optimizer 4'):
        opt.load_state_dict(plain.state_dict())


def test_4_the_model_hands_its_groups_to_the_optimizer():
    from distillclip_amd.optim import FusedAdamW
    model, opt = _build(recipe)
    direct = FusedAdamW(model.towers(), lr=LR, weight_decay=model.hparams.weight_decay, groups=recipe(model))
    assert [[id(p) for p in g['params']] for g in direct.groups] == [[id(p) for p in g['params']] for g in opt.groups]
    assert all(direct._group_ranges(tw) == opt._group_ranges(tw) for tw in model.towers())
    model.optimizer_groups = recipe(model)                                           # a list instead of a callable
    (opt3,), _ = model.configure_optimizers()
    assert all(opt3._group_ranges(tw) == opt._group_ranges(tw) for tw in model.towers())
    assert [p.data_ptr() for g in opt.param_groups for p in g['params']] == [p.data_ptr() for p in opt._trainable()]
