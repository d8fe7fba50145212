"""The EMA inside the fused AdamW step, on the device: dclip_adamw_multi_ema and dclip_swap_multi through the C entry (sections 1-6),
FusedAdamW(ema_decay=...), ema_weights(), the checkpoint round trip and the model hooks on the tiny two-tower model of
tests/test_amp_optim_gpu.py (sections 7-10).  Cases, reference and bound: tests/ema_cases.py.

Every raw call runs on guarded buffers: each range of p, g, m, v, e lies between NaN guard words, which must come back bit-equal.

MEASURED on one MI355X with `pytest tests/test_ema_gpu.py -m gpu -s` (24 passed in 6 s).  Worst err / bound of the kernel cases (sections 1
and 2): 1.000 to three digits, reached by the `ulp` family at w = 0.5, where e + ulp / 2 is a tie and the error is half an ulp of e', which the
bound's |e'| term allows and no more (0.999995 in tests/test_ema_cpu.py's emulation, to which the kernel's e' is bit-equal); up to 0.999 on the
random families.  After three optimizer steps (section 7): 0.999 of the summed per-step bounds in all five variants."""
import ctypes
import io

import numpy as np
import pytest
import torch

import adamw_cases as ac
import ema_cases as ec
from distillclip_amd import synth

pytestmark = pytest.mark.gpu

WORST = [0.0]


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _small(words, at=4):
    host = np.full(at + len(words) + 4, ec.GUARD_BITS, dtype=np.uint32).view(np.float32)
    host[at:at + len(words)] = words
    return torch.from_numpy(host.copy()).cuda(), host, at


def _record(t, mult=1.0, skip=0.0):
    bc1, bc2s = ac.exact_bc(ac.HYPER, t)
    return [float(np.float32(mult)), skip, float(bc1), float(bc2s), np.nan, np.nan, np.nan, np.nan]


def call(flat, lens, mode, t, zero_grad, w=None, h=ac.HYPER, gs=0.3172, record=None, bad=None, order=None):
    """one guarded call.  flat: {name: f32 [sum(lens)]} for p, g, m, v and, with w given, e.  w None: the existing entry of `mode`
    ('plain' dclip_adamw_multi, 'scaled' dclip_adamw_multi_scaled, 'amp' dclip_adamw_multi_amp); else dclip_adamw_multi_ema.
    order: the ranges are handed over in this order.  bad: a function that spoils the argument dict; the call must then be refused.
    -> {name: the ranges' contents after the call}; the guard words, the multiplier and the record have been checked"""
    lib = _lib()
    lr, b1, b2, eps, wd = h
    names = 'pgmv' + ('e' if w is not None else '')
    host, spans = {}, None
    for k in names:
        host[k], spans = ec.guarded(flat[k], lens)
    dev = {k: torch.from_numpy(b.copy()).cuda() for k, b in host.items()}
    count = len(lens)
    order = list(range(count)) if order is None else list(order)
    arr = lambda k: (ctypes.c_void_p * count)(*[dev[k].data_ptr() + 4 * spans[i][0] for i in order])
    a = {k: arr(k) for k in names}
    a['n'] = (ctypes.c_int64 * count)(*[lens[i] for i in order])
    a['count'] = count
    small = None
    if mode == 'scaled':
        small = _small([gs], at=5)
    elif mode == 'amp':
        small = _small(_record(t) if record is None else record)
    sp = None if small is None else small[0].data_ptr() + 4 * small[2]
    a['gscale'], a['record'] = (sp if mode == 'scaled' else None), (sp if mode == 'amp' else None)
    a['w'], a['step'] = w, t
    st = torch.cuda.current_stream().cuda_stream
    if bad is not None:
        bad(a, dev, spans)
    if w is None:
        assert bad is None
        if mode == 'plain':
            lib.dclip_adamw_multi(a['p'], a['g'], a['m'], a['v'], a['n'], count, lr, b1, b2, eps, wd, t, zero_grad, st)
        elif mode == 'scaled':
            lib.dclip_adamw_multi_scaled(a['p'], a['g'], a['m'], a['v'], a['n'], count, lr, b1, b2, eps, wd, t, zero_grad, sp, st)
        else:
            lib.dclip_adamw_multi_amp(a['p'], a['g'], a['m'], a['v'], a['n'], count, lr, b1, b2, eps, wd, zero_grad, sp, st)
    else:
        go = lambda: lib.dclip_adamw_multi_ema(a['p'], a['g'], a['m'], a['v'], a['e'], a['n'], a['count'], lr, b1, b2, eps, wd, a['step'],
                                               zero_grad, a['w'], a['gscale'], a['record'], st)
        if bad is None:
            go()
        else:
            with pytest.raises(ValueError, match='dclip_adamw_multi_ema'):
                go()
    torch.cuda.synchronize()
    if small is not None:
        assert np.array_equal(ec.bits(small[0].cpu().numpy()), ec.bits(small[1]))
    got = {k: d.cpu().numpy() for k, d in dev.items()}
    mask = np.zeros(host['p'].size, dtype=bool)
    for s, e in spans:
        mask[s:e] = True
    for k in names:
        same = ec.bits(got[k]) == ec.bits(host[k])
        assert same[~mask].all(), f'a guard word of {k} was written'
        if bad is not None:
            assert same.all(), f'a refused call wrote {k}'
    return {k: ec.inside(got[k], spans) for k in names}


def _inputs(n, seed, fam='normal', e_from=None):
    p, g, m, v, _ = ac.shared_family(fam, n, seed=seed)
    r = np.random.RandomState(seed)
    e = (p + 1e-3 * r.randn(n)).astype(np.float32) if e_from is None else e_from
    return dict(p=p, g=g, m=m, v=v, e=e)


def _same(a, b, names):
    for k in names:
        assert np.array_equal(ec.bits(a[k]), ec.bits(b[k])), k


# ---- 1. AdamW is untouched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['plain', 'scaled', 'amp'])
def test_1_p_g_m_v_are_those_of_the_existing_entry(mode):
    lens, S, long4 = ec.lens24()
    assert max(lens) == 4 * long4 and -(-long4 // S) == 3 and long4 % S != 0          # three trips, the last one ragged
    for ls, seed in ((list(ec.LENS5), 11), (lens, 12)):
        flat = _inputs(sum(ls), seed)
        for zero_grad in (0, 1):
            for t in (1, 7):
                old = call(flat, ls, mode, t, zero_grad)
                new = call(flat, ls, mode, t, zero_grad, w=ec.weight(0.9))
                _same(old, new, 'pgmv')
                assert not np.array_equal(new['p'], flat['p']) and not np.array_equal(new['e'], flat['e'])
                assert (ec.bits(new['g']) == 0).all() if zero_grad else np.array_equal(ec.bits(new['g']), ec.bits(flat['g']))
                r, i = ec.ratio(new['e'], flat['e'], new['p'], ec.weight(0.9))
                assert r <= 1, (mode, t, zero_grad, i, r)
                WORST[0] = max(WORST[0], r)


# ---- 2. the average against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', ec.FAMILIES)
def test_2_the_average_element_by_element(fam):
    """lr = 0 and weight_decay = 0: the step writes p' = p, so that the family's relation between e and p' is the one it was built with"""
    ls = list(ec.LENS5)
    n = sum(ls)
    e, p = ec.family(fam, n, seed=2)
    flat = _inputs(n, 21)
    flat.update(p=p, e=e)
    h0 = ac.hyper(lr=0.0, wd=0.0)
    for w in ec.WEIGHTS:
        got = call(flat, ls, 'plain', 3, 0, w=w, h=h0)
        assert np.array_equal(ec.bits(got['p']), ec.bits(p))
        r, i = ec.ratio(got['e'], e, got['p'], w)
        print(f'{fam} w = {w!r}: worst err / bound {r:.3f} at {i} (e {e[i]!r}, p\' {p[i]!r}, e\' {got["e"][i]!r})')
        assert r <= 1
        WORST[0] = max(WORST[0], r)
        if w == 0.0 or fam == 'equal':
            assert np.array_equal(ec.bits(got['e']), ec.bits(e))
        if w == 1.0 and fam in ('ulp', 'equal'):
            assert np.array_equal(ec.bits(got['e']), ec.bits(p))
        assert np.array_equal(ec.bits(got['e']), ec.bits(ec.emulate(e, p, w)))       # (the two roundings the header states, bit for bit)
    print(f'worst err / bound so far: {WORST[0]:.3f}')


def test_2_a_real_step_all_three_modes():
    lens, _, _ = ec.lens24()
    flat = _inputs(sum(lens), 22)
    for mode in ('plain', 'scaled', 'amp'):
        for w in (ec.weight(0.9999), 0.5):
            got = call(flat, lens, mode, 7, 1, w=w)
            r, i = ec.ratio(got['e'], flat['e'], got['p'], w)
            assert r <= 1, (mode, w, i, r)
            WORST[0] = max(WORST[0], r)
    print(f'worst err / bound so far: {WORST[0]:.3f}')


# ---- 3. exact properties --------------------------------------------------------------------------------------------------------------------
def test_3_exact_properties():
    ls = list(ec.LENS5)
    n = sum(ls)
    flat = _inputs(n, 31)
    # e == p' elementwise (lr = 0, weight_decay = 0, e = p, a -0 and a +0 among them): e' == e bit for bit
    p = flat['p'].copy()
    p[[0, 5]] = -0.0, 0.0
    same = dict(flat, p=p, e=p.copy())
    got = call(same, ls, 'plain', 2, 0, w=0.5, h=ac.hyper(lr=0.0, wd=0.0))
    assert np.array_equal(ec.bits(got['e']), ec.bits(p)) and np.array_equal(got['p'], p)
    # w = 0: e bit-unchanged whatever the step does, a NaN gradient included
    g = flat['g'].copy()
    g[7] = np.nan
    got = call(dict(flat, g=g), ls, 'scaled', 2, 1, w=0.0)
    assert np.array_equal(ec.bits(got['e']), ec.bits(flat['e'])) and np.isnan(got['p'][7]) and not np.array_equal(got['p'], flat['p'])
    # the same call twice: the same bits
    a, b = (call(flat, ls, 'amp', 7, 0, w=ec.weight(0.999)) for _ in range(2))
    _same(a, b, 'pgmve')
    # the ranges permuted: the permuted result
    order = [3, 0, 4, 2, 1]
    c = call(flat, ls, 'amp', 7, 0, w=ec.weight(0.999), order=order)
    _same(a, c, 'pgmve')


# ---- 4. skipped step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_4_a_skipped_step_reads_and_writes_nothing(zero_grad):
    lens, _, _ = ec.lens24()
    flat = _inputs(sum(lens), 41)
    for g in (flat['g'], np.full_like(flat['g'], np.nan)):
        got = call(dict(flat, g=g), lens, 'amp', 9, zero_grad, w=0.5, record=[np.nan, 1.0, np.nan, np.nan, 0, 0, 0, 0])
        _same(got, flat, 'pmve')
        assert (ec.bits(got['g']) == 0).all() if zero_grad else np.array_equal(ec.bits(got['g']), ec.bits(g))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_5_refusals_leave_everything_untouched():
    ls = list(ec.LENS5)
    flat = _inputs(sum(ls), 51)

    def shifted(name, k, by):
        def f(a, dev, spans):
            a[name][k] = a[name][k] + by
        return f

    def null(name, k=None):
        def f(a, dev, spans):
            if k is None:
                a[name] = None
            else:
                a[name][k] = None
        return f

    def setv(name, x):
        def f(a, dev, spans):
            a[name] = x
        return f

    def both(a, dev, spans):
        a['record'] = dev['m'].data_ptr()            # (16-byte aligned; never read: the call is refused)

    def short(a, dev, spans):
        a['n'][2] = 1018

    bads = [null('e'), null('e', 1), shifted('e', 2, 4), shifted('e', 0, 8), setv('w', -1e-3), setv('w', 1.0 + 2.0 ** -20), setv('w', float('nan')),
            setv('w', float('inf')), both, null('p'), null('g', 3), shifted('p', 1, 4), shifted('v', 4, 12), short, setv('count', 0), setv('count', 25),
            setv('step', 0)]
    def record_off_by_4(a, dev, spans):
        a['record'] += 4

    for bad in bads:
        call(flat, ls, 'scaled' if bad is both else 'plain', 3, 1, w=0.5, bad=bad)
    call(flat, ls, 'amp', 3, 1, w=0.5, bad=record_off_by_4)


# ---- 6. dclip_swap_multi ----------------------------------------------------------------------------------------------------------------------
def _patterns(n, seed):
    """every kind of word: NaNs with payloads (quiet, signalling, either sign), +-0, +-inf, subnormals, ordinary numbers"""
    r = np.random.RandomState(seed)
    w = r.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC0BEEF, 0xFFC12345, 0x7F800001, 0xFF80FFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32)
    w[::3] = special[r.randint(0, special.size, size=w[::3].size)]
    return w.view(np.float32)


def _swap(a_flat, b_flat, lens, selfswap=()):
    ha, spans = ec.guarded(a_flat, lens)
    hb, _ = ec.guarded(b_flat, lens)
    da, db = torch.from_numpy(ha.copy()).cuda(), torch.from_numpy(hb.copy()).cuda()
    count = len(lens)
    pa = [da.data_ptr() + 4 * s for s, _ in spans]
    pb = [(pa[k] if k in selfswap else db.data_ptr() + 4 * s) for k, (s, _) in enumerate(spans)]
    args = ((ctypes.c_void_p * count)(*pa), (ctypes.c_void_p * count)(*pb), (ctypes.c_int64 * count)(*lens), count, torch.cuda.current_stream().cuda_stream)
    return da, db, ha, hb, spans, args


def test_6_swap_is_exact_and_twice_is_the_identity():
    lib = _lib()
    lens24, _, _ = ec.lens24()
    for lens in ([4], [1028], [4, 1028], lens24):
        n = sum(lens)
        a, b = _patterns(n, 61), _patterns(n, 62)
        da, db, ha, hb, spans, args = _swap(a, b, lens)
        lib.dclip_swap_multi(*args)
        torch.cuda.synchronize()
        ga, gb = da.cpu().numpy(), db.cpu().numpy()
        mask = np.zeros(ha.size, dtype=bool)
        for s, e in spans:
            mask[s:e] = True
        assert np.array_equal(ec.bits(ga), np.where(mask, ec.bits(hb), ec.bits(ha))) and np.array_equal(ec.bits(gb), np.where(mask, ec.bits(ha), ec.bits(hb)))
        lib.dclip_swap_multi(*args)
        torch.cuda.synchronize()
        assert np.array_equal(ec.bits(da.cpu().numpy()), ec.bits(ha)) and np.array_equal(ec.bits(db.cpu().numpy()), ec.bits(hb))


def test_6_swap_with_itself_is_the_identity_and_refusals_write_nothing():
    lib = _lib()
    lens = [4, 1028, 8]
    a, b = _patterns(sum(lens), 63), _patterns(sum(lens), 64)
    da, db, ha, hb, spans, args = _swap(a, b, lens, selfswap=(1,))
    lib.dclip_swap_multi(*args)
    torch.cuda.synchronize()
    ga, gb = da.cpu().numpy(), db.cpu().numpy()
    s, e = spans[1]
    assert np.array_equal(ec.bits(ga[s:e]), ec.bits(ha[s:e])) and np.array_equal(ec.bits(gb[s:e]), ec.bits(hb[s:e]))      # a[1] == b[1]: as it was
    assert np.array_equal(ec.bits(ga[spans[0][0]:spans[0][1]]), ec.bits(hb[spans[0][0]:spans[0][1]]))
    da, db, ha, hb, spans, args = _swap(a, b, lens)
    pa, pb, n, count, st = args
    mk = lambda vals: (ctypes.c_void_p * 3)(*vals)
    for bad in ((None, pb, n, count), (pa, None, n, count), (pa, pb, None, count), (pa, pb, n, 0), (pa, pb, n, 25),
                (mk([pa[0], None, pa[2]]), pb, n, count), (mk([pa[0], pa[1] + 4, pa[2]]), pb, n, count), (pa, mk([pb[0], pb[1], pb[2] + 8]), n, count),
                (pa, pb, (ctypes.c_int64 * 3)(4, 1026, 8), count), (pa, pb, (ctypes.c_int64 * 3)(4, 0, 8), count),
                (pa, mk([pb[0], pa[1] + 16, pb[2]]), n, count)):                                                            # (overlapping, not equal)
        with pytest.raises(ValueError, match='dclip_swap_multi'):
            lib.dclip_swap_multi(*bad, st)
    torch.cuda.synchronize()
    assert np.array_equal(ec.bits(da.cpu().numpy()), ec.bits(ha)) and np.array_equal(ec.bits(db.cpu().numpy()), ec.bits(hb))


def test_ops_wrappers():
    from distillclip_amd import ops
    n = 1028
    f = _inputs(n, 71)
    t = {k: torch.from_numpy(np.array(x)).cuda() for k, x in f.items()}
    u = {k: x.clone() for k, x in t.items()}
    lr, b1, b2, eps, wd = ac.HYPER
    ops.adamw_multi_scaled([(t['p'], t['g'], t['m'], t['v'])], lr, (b1, b2), eps, wd, 2)
    ops.adamw_multi_ema([(u['p'], u['g'], u['m'], u['v'], u['e'])], lr, (b1, b2), eps, wd, 2, False, 0.5)
    assert all(torch.equal(t[k].view(torch.int32), u[k].view(torch.int32)) for k in 'pgmv')
    r, _ = ec.ratio(u['e'].cpu().numpy(), f['e'], u['p'].cpu().numpy(), 0.5)
    assert r <= 1
    ops.swap_multi([(u['p'], u['e'])])
    assert torch.equal(u['e'].view(torch.int32), t['p'].view(torch.int32))
    with pytest.raises(ValueError):
        ops.swap_multi([(u['p'], u['e'][:8])])
    with pytest.raises(RuntimeError):
        ops.swap_multi([(u['p'].cpu(), u['e'].cpu())])


# ---- 7-10. the optimizer on the tiny dual model of tests/test_amp_optim_gpu.py ------------------------------------------------------------------
S_IMG = dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4, mlp_ratio=4.0,
             qkv_bias=True, repeated_times=2, use_transform=True)
S_TXT = dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0,
             qkv_bias=False, repeated_times=2, use_transform=True)
SEED, B = 33, 4
LOSS = dict(loss_name=['out_l1', 'out_cos', 'cos_diff'], loss_scale={'cos_diff': 0.1})
SCALE = 65536.0
DECAY = 0.9


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _build(ema_decay=None, student_state=None):
    from distillclip_amd.model import DualDistillModel
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    from distillclip_amd.optim import FusedAdamW
    si, st = RepeatVisionTransformer(**S_IMG), RepeatTextTransformer(**S_TXT)
    si.load_state_dict(T(synth.student_image_state(SEED, **S_IMG)))
    st.load_state_dict(T(synth.student_text_state(SEED, **S_TXT)))
    tsd = T(synth.teacher_image_state(SEED, 128, 2, 8, 32, 64))
    tsd.update(T(synth.teacher_text_state(SEED, 128, 2, 13, 97, 64)))
    model = DualDistillModel(si, st, LOSS, 0, 10, 1e-2, 1e-3, '.', teacher_state_dict=tsd).cuda()
    if student_state is not None:
        model.student.load_state_dict(student_state)
    model.ema_decay = ema_decay
    (opt,), _ = model.configure_optimizers()
    assert isinstance(opt, FusedAdamW) and opt.ema_decay == ema_decay
    opt.lr = 1e-3
    return model, opt


def _batches():
    return [[torch.from_numpy(synth.images(SEED + i, B, 32)).cuda(), torch.from_numpy(synth.captions(SEED + i, B, 13, 97, 3, 9)).cuda()] for i in range(3)]


def _params(opt):
    return [p.detach().clone() for p in opt._trainable()]


def _state(model, opt):
    return _params(opt) + [t.clone() for tw in model.towers() for t in opt._moments(tw)]


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def recorded():
    """three backwards of the tiny dual model at its initial weights: the towers' flat gradient buffers.  The weight-gradient atomics
    differ from run to run (tests/test_grad_clip_gpu.py's `recorded`), so twins that are to be compared bit for bit step on these bits:
    every step still runs its own forward and backward on the batch, which sets the towers' streams as a real step does, and the
    recorded gradient then takes the place of the one that backward left."""
    model, opt = _build(None)
    grads = []
    for batch in _batches():
        opt.zero_grad()
        model.training_step(batch).backward()
        torch.cuda.synchronize()
        grads.append([tw.flat_grad.clone() for tw in model.towers()])
    return grads


def _step(model, opt, batch, grads, scaler=None, overflow=False, **kw):
    opt.zero_grad()
    if scaler is None:
        model.training_step(batch).backward()
    else:
        with torch.autocast('cuda', dtype=torch.float16):
            loss = model.training_step(batch)
        (scaler.scale(loss) * (float('inf') if overflow else 1.0)).backward()
    torch.cuda.synchronize()
    if not overflow:                                              # (an overflow's gradients are non-finite and the step is skipped)
        for tw, g in zip(model.towers(), grads):
            tw.flat_grad.copy_(g if scaler is None else g * SCALE)
    torch.cuda.synchronize()
    if scaler is None:
        opt.step(**kw)
    else:
        scaler.step(opt)
        scaler.update()
    opt.join()


def _run(recorded, variant, ema_decay, steps=3):
    """`steps` steps of one variant -> model, opt, [parameters after each step], [ema_state_dict after each step or None]"""
    model, opt = _build(ema_decay)
    batches = _batches()
    scaler = torch.amp.GradScaler('cuda', init_scale=SCALE) if variant.startswith('scaler') else None
    if variant == 'clip':
        opt.max_grad_norm = 0.5
    kw = dict(overlap=True, join=False) if variant == 'overlap' else {}
    after, emas = [], []
    for i in range(steps):
        _step(model, opt, batches[i], recorded[i], scaler, variant == 'scaler_overflow' and i == 1, **kw)
        after.append(_params(opt))
        emas.append(list(opt.ema_state_dict().values()) if opt._has_ema() else None)
    torch.cuda.synchronize()
    return model, opt, after, emas


@pytest.mark.parametrize('variant', ['plain', 'clip', 'overlap', 'scaler', 'scaler_overflow'])
def test_7_twins(recorded, variant):
    """a model stepped with ema_decay = 0.9 and one without, same seed, same batches, same gradient bits: parameters, m and v bit-equal
    after three steps; the average equals the float64 recurrence over the recorded parameters within the sum of the per-step bounds
    (each step's error is carried on by a factor 1 - w < 1, so the sum of the bounds covers it)"""
    model0, opt0, after0, _ = _run(recorded, variant, None)
    start = _params(_build(None)[1])
    model1, opt1, after1, emas = _run(recorded, variant, DECAY)
    assert opt0._ema == {} and opt1.step_count == 3
    for a, b in zip(_state(model0, opt0), _state(model1, opt1)):
        assert _eq(a, b)
    assert not all(_eq(a, b) for a, b in zip(start, after1[2]))              # (the weights did move)
    w = ec.weight(DECAY)
    worst = 0.0
    for k, p0 in enumerate(start):
        e = p0.double().cpu().numpy().reshape(-1)
        tol = np.zeros_like(e)
        for i in range(3):
            p2 = after1[i][k].cpu().numpy().reshape(-1)
            moved = not _eq(after1[i][k], (start if i == 0 else after1[i - 1])[k])
            if variant == 'scaler_overflow' and i == 1:
                assert not moved and _eq(emas[1][k], emas[0][k])             # across the overflow step the average does not move
                continue
            tol += ec.bound(e, p2, w)
            e = ec.reference(e, p2, w)
            got = emas[i][k].cpu().numpy().reshape(-1)
            r = float((np.abs(got - e) / tol).max())
            worst = max(worst, r)
            assert r <= 1, (variant, k, i, r)
    print(f'{variant}: worst |ema - float64 recurrence| / (sum of bounds) = {worst:.3f}')
    if variant == 'scaler_overflow':
        assert int(opt1._skipped) == 1


def _outputs(model, batch):
    with torch.no_grad():
        s, _ = model.forward(batch)
    return [s.visual_output.last_representation.clone(), s.text_output.last_representation.clone()]


def test_8_ema_weights_context():
    """the towers' bf16 weight caches are kept by the optimizer here (refresh_cache_in_step: the towers no longer re-cast on every
    forward), so outputs inside the context are right only if ema_weights() marks the caches stale"""
    from distillclip_amd.optim import FusedAdamW
    model, opt = _build(DECAY)
    with pytest.raises(RuntimeError, match='no average'):
        with opt.ema_weights():
            pass
    opt.refresh_cache_in_step = True
    batches = _batches()
    for i in range(3):
        opt.zero_grad()
        model.training_step(batches[i]).backward()
        opt.step(overlap=True)
    assert all(not tw._prepare_always and not tw.wcache_dirty for tw in model.towers())
    model.eval()
    before_p, before_out = _params(opt), _outputs(model, batches[0])
    ema = opt.ema_state_dict()
    names = [n for n, p in model.student.named_parameters() if any(p.data_ptr() == q.data_ptr() for q in opt._trainable())]
    assert len(names) == len(ema)
    sd = {k: v.clone() for k, v in model.student.state_dict().items()}
    by_ptr = {q.data_ptr(): i for i, q in enumerate(opt._trainable())}
    for n, p in model.student.named_parameters():
        if p.data_ptr() in by_ptr:
            sd[n] = ema[by_ptr[p.data_ptr()]]
    fresh, _ = _build(None, student_state=sd)
    fresh.eval()
    want = _outputs(fresh, batches[0])
    with opt.ema_weights():
        inside = _outputs(model, batches[0])
        for i, q in enumerate(opt._trainable()):
            assert _eq(q.detach(), ema[i])
        for fn in (opt.step, opt.state_dict, opt.ema_state_dict, lambda: opt.load_state_dict({})):
            with pytest.raises(RuntimeError, match='ema_weights'):
                fn()
        with pytest.raises(RuntimeError, match='already inside'):
            with opt.ema_weights():
                pass
    for a, b in zip(inside, want):
        assert _eq(a, b)
    assert not _eq(inside[0], before_out[0])
    for a, b in zip(_params(opt), before_p):
        assert _eq(a, b)
    for a, b in zip(_outputs(model, batches[0]), before_out):
        assert _eq(a, b)
    assert opt.step_count == 3


def test_9_checkpoint_round_trip(recorded):
    from distillclip_amd.checkpoint import checkpoint_dict
    model, opt, _, _ = _run(recorded, 'plain', DECAY, steps=2)
    ckpt = checkpoint_dict(model, opt)
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    ckpt = torch.load(buf, map_location='cpu', weights_only=False)
    sd = ckpt['optimizer_states'][0]
    assert set(sd) == {'state', 'param_groups', 'ema'} and sd['ema']['decay'] == DECAY
    assert list(sd['ema']['params']) == list(range(len(opt._trainable())))
    ema = opt.ema_state_dict()
    student = {k.replace('student.', '', 1): v for k, v in ckpt['state_dict'].items() if k.startswith('student.')}
    from distillclip_amd.checkpoint import trainable_parameters
    model2, opt2 = _build(DECAY, student_state=student)
    opt2.load_state_dict(sd, trainable_parameters(model2))
    ema2 = opt2.ema_state_dict()
    assert all(_eq(ema[i], ema2[i]) for i in ema) and opt2.step_count == 2
    batch = _batches()[2]
    for m_, o_ in ((model, opt), (model2, opt2)):
        _step(m_, o_, batch, recorded[2])
    for a, b in zip(_state(model, opt) + list(opt.ema_state_dict().values()), _state(model2, opt2) + list(opt2.ema_state_dict().values())):
        assert _eq(a, b)
    # torch.optim.AdamW takes the dict, the extra key and all
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in opt._trainable()]
    topt = torch.optim.AdamW(ref, lr=1e-3)
    topt.load_state_dict({k: v for k, v in opt.state_dict().items()})
    assert len(topt.state_dict()['state']) == len(ref)
    # a dict without 'ema': the average starts again from the parameters at the next step
    plain = {k: v for k, v in sd.items() if k != 'ema'}
    opt2.load_state_dict(plain, trainable_parameters(model2))
    assert not opt2._has_ema() and opt2.ema_decay == DECAY
    p_before = _params(opt2)
    opt2.zero_grad()
    model2.training_step(batch).backward()
    opt2.step()
    w = ec.weight(DECAY)
    for p0, p1, e in zip(p_before, _params(opt2), opt2.ema_state_dict().values()):
        p0, p1 = p0.cpu().numpy().reshape(-1), p1.cpu().numpy().reshape(-1)
        assert ec.ratio(e.cpu().numpy().reshape(-1), p0, p1, w)[0] <= 1


def test_10_model_hooks(recorded):
    model, opt, _, _ = _run(recorded, 'plain', DECAY, steps=2)
    model.eval()
    batch = _batches()[0]
    base_out, base_log = model.validation_step(batch)
    with opt.ema_weights():
        want_out, want_log = model.validation_step(batch)
    model.on_validation_start()                                   # the flag is off: nothing happens
    off_out, _ = model.validation_step(batch)
    model.on_validation_end()
    model.validate_with_ema = True
    before = _params(opt)
    model.on_validation_start()
    assert opt._ema_in_use
    got_out, got_log = model.validation_step(batch)
    model.on_validation_end()
    assert not opt._ema_in_use
    for k in want_out:
        assert _eq(got_out[k], want_out[k]) and _eq(off_out[k], base_out[k])
    assert not _eq(got_out['stu_image_outs'], base_out['stu_image_outs'])
    assert all(_eq(got_log[k], want_log[k]) for k in want_log)
    for a, b in zip(_params(opt), before):
        assert _eq(a, b)
    fresh, fopt = _build(None)                                    # no average: the hooks do nothing even with the flag set
    fresh.validate_with_ema = True
    fresh.on_validation_start()
    assert not fopt._ema_in_use
    fresh.on_validation_end()
