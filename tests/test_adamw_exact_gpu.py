"""The AdamW kernels element by element against float64 (csrc/optim.hip: adamw_kernel and the three modes of adamw4_multi_kernel through
dclip_adamw, dclip_adamw_multi, dclip_adamw_multi_scaled, dclip_adamw_multi_amp).  Reference, bound, families and buffer layout are in
tests/adamw_cases.py; tests/test_adamw_exact_cpu.py checks the reference and the bound themselves.

Every raw call runs on guarded buffers: each range of p, g, m, v lies between NaN guard words (at least four on either side).  After the
call the guard words are bit-equal to before, g is bit-equal to before (zero_grad = 0) or +0 in every word of a range (zero_grad = 1),
the multiplier or the record is as it was, and p', m', v' are compared on the host in float64, one step at a time.  A call of an entry
that forms its bias corrections on the host passes if ONE candidate pair (adamw_cases.candidates) holds EVERY p' of the call; the
record-driven entry gets a record written by hand and no candidates.

MEASURED on one MI355X with `pytest tests/test_adamw_exact_gpu.py -m gpu -s` (29 passed in 7 s; the lines that _report() prints after the
last raw-call test).  Worst err / bound over every call of this file:

    kernel, entry                                              p'      m'      v'
    adamw4_multi_kernel<PLAIN>, dclip_adamw_multi              0.398   0.485   0.397
    adamw4_multi_kernel<SCALED>, dclip_adamw_multi_scaled      0.418   0.487   0.397
    adamw4_multi_kernel<AMP>, dclip_adamw_multi_amp            0.418   0.487   0.397
    dclip_adamw, aligned (float4 part and tail)                0.359   0.488   0.396
    dclip_adamw, a pointer misaligned (adamw_kernel alone)     0.484   0.452   0.392

The candidate pair that held each call of a host-formed entry, measured in the same run, was at every tested t the FIRST candidate,
the pair of the correctly rounded powers (the host's powf was correctly rounded at these steps):

    t        bc1                    bc2s                    candidates   |bc2s - double| / double (f32 beta2 / the double 0.999)
    1        0.10000002384185791    0.03162257373332977     9            2.2e-8 / 6.4e-6
    2        0.19000005722045898    0.044709742069244385    9            3.3e-6 / 9.7e-6
    3        0.27100008726119995    0.05474469065666199     9            3.1e-6 / 3.3e-6
    4        0.34390008449554443    0.0631975382566452      9            3.0e-6 / 9.4e-6
    5        0.40951007604599       0.07063937932252884     9            2.4e-6 / 8.8e-6
    7        0.5217031836509705     0.08353998512029648     9            1.2e-6 / 7.6e-6
    1000     1.0                    0.7951728105545044      2            3.0e-8 / 3.8e-6
    100000   1.0                    1.0                     1            0 / 0

(the last column is host arithmetic, printed by tests/test_adamw_exact_cpu.py as well: the f32 formula loses most at t = 2, where
1 - beta2^2 = 2e-3 carries the rounding of beta2^2 to f32 at 500 times its relative size.)  No test of this file found a fault in
csrc/optim.hip; the one change the tests asked for is on the host (FusedAdamW.step, section 6)."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_cases as ac

pytestmark = pytest.mark.gpu

LENS3 = (4, 1028, 4100)                                    # tests/test_amp_optim_gpu.py's three ranges
WORST = {}                                                 # mode -> [p', m', v']: the worst err / bound so far in this module
PAIRS = {}                                                 # t -> set of (bc1, bc2s) that held a whole call


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _split(arrays, lens):
    """(p, g, m, v) of sum(lens) elements -> [(p, g, m, v)] per range"""
    at, out = 0, []
    for n in lens:
        out.append(tuple(a[at:at + n] for a in arrays))
        at += n
    return out


def _small(words, at=4):
    """a guarded device vector for a multiplier or a record: `words` f32 starting 16 bytes into NaN guard words -> tensor, host copy"""
    host = np.full(at + len(words) + 4, ac.GUARD_BITS, dtype=np.uint32).view(np.float32)
    host[at:at + len(words)] = words
    return torch.from_numpy(host.copy()).cuda(), host


def run(ranges, t, mode='plain', entry='multi', gs=None, zero_grad=0, offsets=(0, 0, 0, 0), h=ac.HYPER, record=None):
    """one guarded call.  ranges: [(p, g, m, v)] f32 arrays.  entry 'single' = dclip_adamw on the one range; 'multi' = the entry of
    `mode`: 'plain' dclip_adamw_multi, 'scaled' dclip_adamw_multi_scaled with the device multiplier gs, 'amp' dclip_adamw_multi_amp with
    `record` = (multiplier, skip flag, bc1, bc2s).  -> before (p, g, m, v), after (p', m', v'), all ranges concatenated"""
    lib = _lib()
    lr, b1, b2, eps, wd = h
    bufs, spans = ac.host_buffers(ranges, offsets)
    dev = {k: torch.from_numpy(b).cuda() for k, b in bufs.items()}
    count = len(ranges)
    ptr = lambda name, k: dev[name].data_ptr() + 4 * spans[name][k][0]
    for name, off in zip(ac.NAMES, offsets):
        assert all(ptr(name, k) % 16 == 4 * off for k in range(count))
    st = torch.cuda.current_stream().cuda_stream
    small = None
    if entry == 'single':
        assert count == 1 and mode == 'plain'
        lib.dclip_adamw(ptr('p', 0), ptr('g', 0), ptr('m', 0), ptr('v', 0), len(ranges[0][0]), lr, b1, b2, eps, wd, t, zero_grad, st)
    else:
        arr = lambda name: (ctypes.c_void_p * count)(*[ptr(name, k) for k in range(count)])
        lens = (ctypes.c_int64 * count)(*[len(r[0]) for r in ranges])
        if mode == 'plain':
            lib.dclip_adamw_multi(arr('p'), arr('g'), arr('m'), arr('v'), lens, count, lr, b1, b2, eps, wd, t, zero_grad, st)
        elif mode == 'scaled':
            small = _small([gs], at=5)                                                   # (a multiplier needs 4-byte alignment only)
            lib.dclip_adamw_multi_scaled(arr('p'), arr('g'), arr('m'), arr('v'), lens, count, lr, b1, b2, eps, wd, t, zero_grad,
                                         small[0].data_ptr() + 20, st)
        else:
            small = _small(list(record) + [np.nan] * 4)
            lib.dclip_adamw_multi_amp(arr('p'), arr('g'), arr('m'), arr('v'), lens, count, lr, b1, b2, eps, wd, zero_grad,
                                      small[0].data_ptr() + 16, st)
    torch.cuda.synchronize()
    if small is not None:
        assert np.array_equal(_bits(small[0].cpu().numpy()), _bits(small[1]))
    got = {k: d.cpu().numpy() for k, d in dev.items()}
    for name in ac.NAMES:
        inside = np.zeros(got[name].size, dtype=bool)
        for a, e in spans[name]:
            inside[a:e] = True
        same = _bits(got[name]) == _bits(bufs[name])
        assert same[~inside].all(), f'a guard word of {name} was written at {int(np.argmin(same | inside))}'
        if name == 'g':
            assert (_bits(got[name])[inside] == 0).all() if zero_grad else same.all(), 'g after the call'
    cat = lambda src, name: np.concatenate([src[name][a:e] for a, e in spans[name]])
    return tuple(cat(bufs, k) for k in ac.NAMES), tuple(cat(got, k) for k in 'pmv')


def judged(ranges, t, mode='plain', entry='multi', gs=None, h=ac.HYPER, label='', **kw):
    """run() and judge(): the host's candidates, or the record's own pair and nothing else -> the verdict, before, after"""
    record = kw.get('record')
    pairs = ac.candidates(h, t) if record is None else [(np.float32(record[2]), np.float32(record[3]))]
    mult = gs if record is None else float(np.float32(record[0]))
    before, after = run(ranges, t, mode, entry, gs, h=h, **kw)
    res = ac.judge(before, after, h, pairs, None if mult is None else float(np.float32(mult)), f'{label} {mode}/{entry} t={t}')
    key = mode if entry == 'multi' else ('single' if not any(kw.get('offsets', (0,))) else 'single, scalar kernel')
    WORST[key] = [max(a, b) for a, b in zip(WORST.get(key, [0, 0, 0]), (res['p'], res['m'], res['v']))]
    if record is None:
        PAIRS.setdefault(t, set()).add((res['pair'], res['tried']))
    return res, before, after


def _report(what):
    print(f'{what}: worst err / bound so far (p\', m\', v\'): ' + '; '.join(f'{k} {r[0]:.3f} {r[1]:.3f} {r[2]:.3f}' for k, r in sorted(WORST.items())))
    for t in sorted(PAIRS):
        d = [(pair, tried, ac.bc2s_distance(ac.HYPER, t, pair[1])) for pair, tried in sorted(PAIRS[t])]
        print(f'  t = {t}: pair(s) that held a call: ' + '; '.join(
            f'bc1 {p[0]!r} bc2s {p[1]!r} (candidate {k} of {len(ac.candidates(ac.HYPER, t))}, bc2s {dist[0]:.3e} from the double value)' for p, k, dist in d))


def _record(t, mult=1.0, skip=0.0, h=ac.HYPER):
    bc1, bc2s = ac.exact_bc(h, t)
    return (float(np.float32(mult)), skip, float(bc1), float(bc2s))


def _mode_args(mode, t, gs):
    """the multiplier the way each mode takes it (plain has none: gs must be None)"""
    if mode == 'plain':
        assert gs is None
        return {}
    if mode == 'scaled':
        return dict(gs=1.0 if gs is None else gs)
    return dict(record=_record(t, 1.0 if gs is None else gs))


# ---- 1. dclip_adamw: the float4 part plus a tail of 0..3, and the scalar kernel alone --------------------------------------------------
SINGLE_N = (1, 2, 3, 4, 5, 7, 8, 1020, 1023, 1024, 1025, 1027)


@pytest.mark.parametrize('offsets', [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 0, 0, 1)],
                         ids=['aligned', 'off1', 'off2', 'off3', 'only_v_off1'])
def test_single_range_entry(offsets):
    """aligned: adamw4_multi_kernel on n / 4 * 4 elements and adamw_kernel on the tail; any pointer off a 16-byte boundary: adamw_kernel alone"""
    for i, n in enumerate(SINGLE_N):
        name = ('normal', 'tiny', 'cancel')[i % 3]
        p, g, m, v, _ = ac.shared_family(name, n, seed=1)
        judged([(p, g, m, v)], 7 if i % 2 else 2, entry='single', zero_grad=i % 2, offsets=offsets, label=f'{name} n={n} offsets={offsets}')
    _report(f'dclip_adamw {offsets}')


# ---- 2. the grid-stride loop -------------------------------------------------------------------------------------------------------------
def _lens24():
    S = 341 * 256
    assert ac.stride4(24, 3 * S + 1) == S                                                # max(256, 8192 / 24) = 341 workgroups per range
    lens4 = [1, 255, 256, 257, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 1] + [1, 2, 3, 5, 17, 64, 100, 255, 256, 300, 511, 512, 1000]
    assert len(lens4) == 24
    order = np.random.RandomState(24).permutation(24)                                     # the long ranges are not the first or the last
    return [4 * lens4[k] for k in order], S


@pytest.mark.parametrize('mode', ['plain', 'scaled', 'amp'])
def test_24_ranges_straddling_the_loops_ends(mode):
    """lengths of 1, 255, 256, 257, S - 1, S, S + 1, 2 S - 1, 2 S, 2 S + 1, 3 S + 1 float4 around the grid-stride S = 87 296: the loop's
    first, second, third and fourth iteration, whole and partly idle, next to ranges of a single workgroup"""
    lens, S = _lens24()
    fam, gs = {'plain': ('normal', None), 'scaled': ('normal', 0.3172), 'amp': ('big', ac.GS_BIG)}[mode]
    p, g, m, v, _ = ac.shared_family(fam, sum(lens), seed=2)
    res, _, _ = judged(_split((p, g, m, v), lens), 7, mode, zero_grad=int(mode != 'scaled'), label=f'24 ranges {fam}', **_mode_args(mode, 7, gs))
    print(f'{mode}: {sum(lens)} elements in 24 ranges, stride {S} float4, longest {max(lens) // 4}: {res}')
    _report('24 ranges')


@pytest.mark.parametrize('mode', ['plain', 'scaled', 'amp'])
def test_1_and_3_ranges(mode):
    """other counts, other grids: 3 ranges -> 2730 workgroups per range, stride 698 880 float4, lengths S + 1, 257, S - 1; 1 range of 257 float4"""
    S = ac.stride4(3, 10 ** 7)
    assert S == 2730 * 256
    for lens4 in ([S + 1, 257, S - 1], [257]):
        lens = [4 * n for n in lens4]
        assert ac.stride4(len(lens4), max(lens4)) == (S if len(lens4) == 3 else 512)
        p, g, m, v, _ = ac.shared_family('normal', sum(lens), seed=3)
        gs = None if mode == 'plain' else 0.3172
        judged(_split((p, g, m, v), lens), 2, mode, zero_grad=1, label=f'{len(lens)} ranges', **_mode_args(mode, 2, gs))
    _report('1 and 3 ranges')


def test_one_range_past_a_single_range_grid():
    """dclip_adamw on 4 (8192 * 256 + 257) elements: its float4 launch has the capped grid of 8192 workgroups, of which the first two
    run a second iteration, the second partly idle"""
    n4 = 8192 * 256 + 257
    assert ac.stride4(1, n4) == 8192 * 256
    p, g, m, v, _ = ac.family('normal', 4 * n4, seed=4)                                   # (134 MB: used once, not kept)
    res, _, _ = judged([(p, g, m, v)], 7, entry='single', zero_grad=1, label='one long range')
    print(f'{4 * n4} elements: {res}')
    _report('one long range')


# ---- 3. families and steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ac.FAMILIES)
def test_families_at_every_step(name):
    """3 ranges of 4, 1028 and 4100 elements; the host-formed bias corrections (plain, or scaled where the family carries a multiplier)
    and the record-driven kernel with the two exact f32 bias corrections written by hand"""
    p, g, m, v, gs = ac.shared_family(name, sum(LENS3), seed=5)
    ranges = _split((p, g, m, v), LENS3)
    for t in ac.steps_of(name):
        host_mode = 'plain' if gs is None else 'scaled'
        a, _, _ = judged(ranges, t, host_mode, label=name, **_mode_args(host_mode, t, gs))
        b, _, _ = judged(ranges, t, 'amp', label=name, zero_grad=1, **_mode_args('amp', t, gs))
        print(f"{name} t = {t}: {host_mode} p' {a['p']:.3f} m' {a['m']:.3f} v' {a['v']:.3f}, pair {a['pair']} (candidate {a['tried']}); "
              f"amp p' {b['p']:.3f} m' {b['m']:.3f} v' {b['v']:.3f}")
    _report(name)


def test_five_consecutive_steps_from_zero_moments():
    """t = 1..5 with fresh gradients, the kernel's own p, m, v fed forward, every step checked on its own"""
    r = np.random.RandomState(55)
    n = sum(LENS3)
    p, m, v = (0.05 * r.randn(n)).astype(np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    start = p.copy()
    for t in range(1, 6):
        g = (1e-3 * r.randn(n) * (1 + 10 * (t % 2))).astype(np.float32)
        res, _, (p, m, v) = judged(_split((p, g, m, v), LENS3), t, 'plain', label='consecutive')
        print(f"t = {t}: p' {res['p']:.3f} m' {res['m']:.3f} v' {res['v']:.3f}, pair {res['pair']} (candidate {res['tried']})")
    assert float(np.abs(p - start).max()) > 5e-3 and (v > 0).all()
    _report('five steps')


# ---- 4. multipliers, the skip flag, non-finite gradients ---------------------------------------------------------------------------------
@pytest.mark.parametrize('gs', [1.0, ac.GS_BIG, 0.3172, 0.0])
def test_multipliers(gs):
    lr, b1, b2, eps, wd = ac.HYPER
    p, g, m, v, _ = ac.shared_family('big' if gs == ac.GS_BIG else 'normal', sum(LENS3), seed=6)
    ranges = _split((p, g, m, v), LENS3)
    for mode in ('scaled', 'amp'):
        res, _, (p2, m2, v2) = judged(ranges, 7, mode, label=f'gs={gs}', **_mode_args(mode, 7, gs))
        print(f"gs = {gs} {mode}: p' {res['p']:.3f} m' {res['m']:.3f} v' {res['v']:.3f}")
        if gs == 0.0:
            # g * 0 = 0: the moments only decay, one rounding each, and the reference is exact in f32
            f = np.float32
            assert np.array_equal(m2, f(b1) * m) and np.array_equal(v2, f(b2) * v)
    _report(f'multiplier {gs}')


@pytest.mark.parametrize('zero_grad', [0, 1])
def test_skip_flag(zero_grad):
    """a record with the skip flag set, NaN in its other three fields, an inf and a NaN in g: p, m, v bit-equal to before (run() checks g
    and the guard words); ranges of one workgroup and ranges long enough for the loop's second and third iteration"""
    lens, S = _lens24()
    p, g, m, v, _ = ac.shared_family('big', sum(lens), seed=7)
    g = g.copy()
    g[[0, 5, sum(lens) - 1]] = np.inf, np.nan, -np.inf
    n3 = sum(LENS3)
    for ranges, record in ((_split((p, g, m, v), lens), (np.nan, 1.0, np.nan, np.nan)),
                           (_split((p[:n3], g[:n3], m[:n3], v[:n3]), LENS3), (1.0, 2.0, 0.5, 0.5))):     # any flag but 0 skips
        before, after = run(ranges, 9, 'amp', zero_grad=zero_grad, record=record)
        for name, b, a in zip('pmv', (before[0], before[2], before[3]), after):
            assert np.array_equal(_bits(b), _bits(a)), name


def test_a_non_finite_gradient_poisons_its_own_element_only():
    """an inf and a NaN in g at the first and the last lane of a float4 and in the tail: p', m', v' are non-finite exactly where the
    float64 reference's are (judge() demands the same kind of value there) and every other element stays inside its bound"""
    n = 1027
    p, g, m, v, _ = ac.shared_family('normal', n, seed=8)
    hit = {0: np.inf, 7: np.nan, 512: np.nan, 1019: -np.inf, 1024: np.inf, 1026: np.nan}  # lanes 0 and 3; the tail of dclip_adamw
    g = g.copy()
    for i, x in hit.items():
        g[i] = x
    _, _, after = judged([(p, g, m, v)], 7, entry='single', label='non-finite')
    for a in after:
        assert sorted(np.flatnonzero(~np.isfinite(a)).tolist()) == sorted(hit)
    g4 = np.concatenate([g, g[:1]])
    p4, m4, v4 = (np.concatenate([a, a[:1]]) for a in (p, m, v))
    for mode in ('plain', 'scaled', 'amp'):
        _, _, after = judged(_split((p4, g4, m4, v4), (4, 1024)), 7, mode, label='non-finite', **_mode_args(mode, 7, None if mode == 'plain' else 0.3172))
        for a in after:
            assert sorted(np.flatnonzero(~np.isfinite(a)).tolist()) == sorted(list(hit) + [1027])
    _report('non-finite')


# ---- 5. corners --------------------------------------------------------------------------------------------------------------------------
def test_corners():
    p, g, m, v, _ = ac.shared_family('normal', sum(LENS3), seed=9)
    ranges = _split((p, g, m, v), LENS3)
    # lr = 0: p (1 - 0) - 0 * q = p, bit for bit; the moments still advance
    h = ac.hyper(lr=0.0)
    for mode in ('plain', 'amp'):
        _, before, after = judged(ranges, 7, mode, h=h, label='lr=0', **_mode_args(mode, 7, None))
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and not np.array_equal(after[1], before[2]) and not np.array_equal(after[2], before[3])
    # wd = 0: no decay
    judged(ranges, 7, 'plain', h=ac.hyper(wd=0.0), label='wd=0')
    judged([ranges[1]], 7, entry='single', offsets=(1, 1, 1, 1), h=ac.hyper(wd=0.0), label='wd=0')
    # g = m = v = 0: the moments stay 0 exactly and p' = p (1 - lr wd): c = 1 - lr wd within u, the product one rounding more
    z = np.zeros_like(p)
    lr, wd = ac.HYPER[0], ac.HYPER[4]
    for kw in (dict(mode='plain'), dict(mode='amp', record=_record(7)), dict(entry='single', offsets=(2, 2, 2, 2))):
        many = kw.get('entry') != 'single'
        _, _, after = judged(_split((p, z, z, z), LENS3) if many else [(p[:1027], z[:1027], z[:1027], z[:1027])], 7, label='zeros', **kw)
        want = p[:after[0].size].astype(np.float64) * (1 - lr * wd)
        assert (_bits(after[1]) == 0).all() and (_bits(after[2]) == 0).all()
        assert (np.abs(after[0] - want) <= 2 * ac.U * np.abs(want)).all()
    _report('corners')


# ---- 6. FusedAdamW: a range the float4 kernels refuse -------------------------------------------------------------------------------------
def _extras(which):
    """a 64-element parameter that fits and one that does not: 6 elements ('odd') or 64 elements 4 bytes off a 16-byte boundary"""
    r = np.random.RandomState(66)
    mk = lambda n: torch.from_numpy((0.05 * r.randn(n)).astype(np.float32)).cuda()
    good = torch.nn.Parameter(mk(64).view(8, 8))
    bad = torch.nn.Parameter(mk(6).view(2, 3) if which == 'odd' else mk(68)[1:65].view(8, 8))
    good.grad, bad.grad = 1e-3 * torch.randn_like(good), 1e-3 * torch.randn_like(bad)
    assert good.data_ptr() % 16 == 0 and (bad.numel() % 4 != 0 if which == 'odd' else bad.data_ptr() % 16 == 4)
    return [good, bad]


@pytest.mark.parametrize('which', ['odd', 'misaligned'])
def test_fused_adamw_refuses_a_scalar_range_before_anything_moves(which):
    from distillclip_amd.optim import FusedAdamW
    lr, (b1, b2), eps, wd = ac.LR, ac.BETAS, ac.EPS, ac.WD
    params = _extras(which)
    opt = FusedAdamW([], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, extra_params=params)
    before = [(p.detach().cpu().numpy().reshape(-1).copy(), p.grad.cpu().numpy().reshape(-1).copy()) for p in params]
    opt.step()                                                                           # the plain step takes both
    torch.cuda.synchronize()
    assert opt.step_count == 1 and opt.last_grad_norm is None
    state = lambda: [t.cpu().numpy().reshape(-1).copy() for p in params for t in (p.detach(), p.grad) + opt._extra_moments(p)]
    for (p0, g0), p in zip(before, params):
        m2, v2 = (t.cpu().numpy() for t in opt._extra_moments(p))
        z = np.zeros_like(p0)
        res = ac.judge((p0, g0, z, z), (p.detach().cpu().numpy().reshape(-1), m2, v2), ac.HYPER, ac.candidates(ac.HYPER, 1), None, f'extras {which}')
        print(f"{which}: plain step on {p0.size} elements: p' {res['p']:.3f} m' {res['m']:.3f} v' {res['v']:.3f}")
    held = state()
    assert all(np.abs(h).max() > 0 for h in held)

    def refused(**attrs):
        for k, x in attrs.items():
            setattr(opt, k, x)
        with pytest.raises(ValueError, match=r'extra parameter 1 \(\(%s\)\)' % ('2, 3' if which == 'odd' else '8, 8')):
            opt.step(zero_grad=True)
        torch.cuda.synchronize()
        assert opt.step_count == 1 and opt._amp_rec is None and opt._skipped is None and opt._clip_parts is None
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(state(), held))
    refused(max_grad_norm=1.0)                                                           # the clipping step
    refused(max_grad_norm=None, found_inf=torch.zeros(1, device='cuda'), grad_scale=torch.full((1,), 65536.0, device='cuda'))
    refused(max_grad_norm=1.0)                                                           # both
    del opt.found_inf, opt.grad_scale
    opt.max_grad_norm = None
    opt.step()                                                                           # and the plain step still works: t = 2
    assert opt.step_count == 2
    # the same optimizer over the parameter that fits alone: all three kinds of step run
    ok = FusedAdamW([], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, extra_params=params[:1], max_grad_norm=1.0)
    ok.step()
    ok.found_inf, ok.grad_scale = torch.zeros(1, device='cuda'), torch.ones(1, device='cuda')
    ok.step()
    torch.cuda.synchronize()
    assert ok.step_count == 2 and int(ok._skipped) == 0
