"""The reference and the bound of tests/adamw_cases.py, checked on their own (no GPU): the float64 reference against torch.optim.AdamW on
float64 parameters, an f32 emulation of adamw_elem's operation order inside the bound (separately rounded, and with the sums fused with
either product), and five known wrong forms of the update outside it.  Run with -s to see the worst ratios and the caught shares."""
import numpy as np
import pytest
import torch

import adamw_cases as ac

N = 4096


def test_reference_equals_torch_adamw_on_float64_for_five_steps():
    """torch.optim.AdamW(lr, betas, eps, weight_decay) with the f32-rounded hyper-parameters on float64 CPU parameters; the reference
    gets the exact double bias corrections: p within 1e-12 relative, m and v equal to exp_avg and exp_avg_sq (torch's lerp_ forms
    m + (1 - b1)(g - m): a few double roundings apart)"""
    lr, b1, b2, eps, wd = ac.HYPER
    r = np.random.RandomState(0)
    p0 = 0.05 * r.randn(N)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0, np.zeros(N), np.zeros(N)
    e = 2.0 ** -53
    for t in range(1, 6):
        g = 1e-3 * r.randn(N) * (1 + 10 * (t % 2))
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        bc1, bc2s = ac.double_bc(ac.HYPER, t)
        want_p, want_m, want_v = ac.reference(p, g, m, v, ac.HYPER, bc1, bc2s)           # one step from torch's own state
        st = opt.state[param]
        got_p, got_m, got_v = param.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()
        assert got_p.dtype == np.float64 and float(st['step']) == t
        rel = float((np.abs(got_p - want_p) / np.abs(want_p)).max())
        print(f't = {t}: max relative |p - torch| = {rel:.2e}')
        assert rel <= 1e-12
        # a handful of double roundings each way: 8 of them on the terms of m (which may cancel), 8 on v
        assert (np.abs(got_m - want_m) <= 8 * e * (np.abs(m) + np.abs(g))).all() and (np.abs(got_v - want_v) <= 8 * e * want_v).all()
        p, m, v = got_p, got_m, got_v
    assert float(np.abs(p - p0).max()) > 5e-3                                            # (the parameters moved: about lr per step)


def test_candidates_hold_the_c_librarys_powf():
    """the host's powf(beta, (float)t) is one of the three candidates at every tested step, and the first candidate is the correctly
    rounded power (exact rational arithmetic where that is cheap)"""
    import ctypes
    from fractions import Fraction
    libm = ctypes.CDLL('libm.so.6')
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    for t in ac.STEPS + (3, 4, 5):
        for beta in ac.HYPER[1:3]:
            cand = ac.power_candidates(beta, t)
            assert np.float32(libm.powf(beta, float(t))) in cand, (beta, t)
            if t <= 1000:
                exact = Fraction(beta) ** t
                assert min(cand, key=lambda y: abs(Fraction(float(y)) - exact)) == cand[0]
        pairs = ac.candidates(ac.HYPER, t)
        assert 1 <= len(pairs) <= 9 and pairs[0] == ac.exact_bc(ac.HYPER, t)
        d = ac.bc2s_distance(ac.HYPER, t, pairs[0][1])
        print(f't = {t}: {len(pairs)} candidate pairs, bc1 = {float(pairs[0][0])!r}, bc2s = {float(pairs[0][1])!r}, relative distance of '
              f'bc2s from the double value {d[0]:.3e} (beta2 = f32(0.999)), {d[1]:.3e} (beta2 = 0.999)')


def _cases():
    for name in ac.FAMILIES:
        for t in ac.steps_of(name):
            yield name, t


def test_the_f32_emulation_stays_inside_the_bound():
    """every family, every step, every candidate pair's first (the correctly rounded one), separately rounded and both contractions; the
    multiplier 2^-16 where the family carries one, 0.3172 (a rounding of its own) on the others as well"""
    worst = {}
    for name, t in _cases():
        p, g, m, v, gs = ac.shared_family(name, N)
        bc1, bc2s = ac.exact_bc(ac.HYPER, t)
        for mult in ((gs,) if gs is not None else (None, 0.3172)):
            mult = None if mult is None else float(np.float32(mult))
            p2, m2, v2 = ac.reference(p, g, m, v, ac.HYPER, bc1, bc2s, mult)
            tp, tm, tv = ac.bounds(p, g, m, v, ac.HYPER, bc1, bc2s, mult)
            assert np.isfinite(p2).all() and (tp > 0).all() and (tm > 0).all() and (tv > 0).all()
            for contract in (None, 'left', 'right'):
                e = ac.emulate(p, g, m, v, ac.HYPER, bc1, bc2s, mult, contract)
                ratios = [float((np.abs(e[k].astype(np.float64) - want) / tol).max()) for k, (want, tol) in enumerate(((p2, tp), (m2, tm), (v2, tv)))]
                key = (name, 'fused' if contract else 'separate')
                worst[key] = [max(a, b) for a, b in zip(worst.get(key, [0, 0, 0]), ratios)]
                assert max(ratios) <= 1, (name, t, mult, contract, ratios)
    for (name, how), r in worst.items():
        print(f"{name:7s} {how:9s}: worst err / bound  p' {r[0]:.3f}  m' {r[1]:.3f}  v' {r[2]:.3f}")
    print("overall: p' %.3f  m' %.3f  v' %.3f" % tuple(max(r[k] for r in worst.values()) for k in range(3)))


@pytest.mark.parametrize('form', ac.WRONG_FORMS)
def test_a_known_wrong_form_falls_outside_the_bound(form):
    """at least one (family, t) has more than half of its p' outside tp"""
    share = {}
    for name, t in _cases():
        p, g, m, v, gs = ac.shared_family(name, N)
        bc1, bc2s = ac.exact_bc(ac.HYPER, t)
        p2 = ac.reference(p, g, m, v, ac.HYPER, bc1, bc2s, gs)[0]
        tp = ac.bounds(p, g, m, v, ac.HYPER, bc1, bc2s, gs)[0]
        share[name, t] = float((np.abs(ac.wrong(form, p, g, m, v, ac.HYPER, bc1, bc2s, gs) - p2) > tp).mean())
    for (name, t), s in share.items():
        print(f'{form}: {name:7s} t = {t:6d}: {100 * s:5.1f} % outside')
    assert max(share.values()) > 0.5
    # the shares the bound was designed to keep
    if form in ('eps_in_root', 'bc2_without_root', 'old_m'):
        assert all(share['normal', t] >= 0.99 for t in (1, 2, 7, 1000))
    if form == 'eps_before_bc2s':
        assert all(share['tiny', t] >= 0.99 for t in (1, 2, 7, 1000))
    if form == 'decay_after_step':
        assert share['normal', 1000] >= 0.9 and share['normal', 100000] >= 0.9


def test_a_neighbouring_candidate_changes_little_and_a_wrong_step_changes_much():
    """what the candidates are allowed to absorb: the pair of a neighbouring power moves p' by a few bounds at most; the bias
    corrections of t + 1 at a small t move it by thousands"""
    p, g, m, v, _ = ac.shared_family('normal', N)
    for t in (2, 7):
        pairs = ac.candidates(ac.HYPER, t)
        ref = ac.reference(p, g, m, v, ac.HYPER, *pairs[0])[0]
        tp = ac.bounds(p, g, m, v, ac.HYPER, *pairs[0])[0]
        near = max(float((np.abs(ac.reference(p, g, m, v, ac.HYPER, *q)[0] - ref) / tp).max()) for q in pairs[1:])
        far = float(np.median(np.abs(ac.reference(p, g, m, v, ac.HYPER, *ac.exact_bc(ac.HYPER, t + 1))[0] - ref) / tp))
        print(f't = {t}: a neighbouring pair moves p by at most {near:.2f} bounds, the pair of t + 1 by a median of {far:.0f}')
        assert near < 100 and far > 1000


def test_layout_and_stride():
    spans, total = ac.layout([1, 5, 1024], (0, 1, 2, 3))
    for name, off in zip(ac.NAMES, (0, 1, 2, 3)):
        last = 0
        for (a, e), n in zip(spans[name], (1, 5, 1024)):
            assert e - a == n and a % 4 == off and a - last >= ac.GUARD
            last = e
        assert total[name] - last >= ac.GUARD
    bufs, spans = ac.host_buffers([tuple(np.full(3, k, dtype=np.float32) for k in range(4))])
    assert np.isnan(bufs['p'][:4]).all() and bufs['v'][4:7].tolist() == [3, 3, 3] and np.isnan(bufs['v'][7:]).all()
    assert bufs['g'].view(np.uint32)[0] == ac.GUARD_BITS
    assert ac.stride4(24, 3 * 87296 + 1) == 341 * 256 == 87296 and ac.stride4(3, 10 ** 7) == 2730 * 256 and ac.stride4(1, 257) == 2 * 256
    assert ac.stride4(1, 8192 * 256 + 257) == 8192 * 256
    # stride4 restates adamw_ranges and grid_for: the lengths of the GPU tests straddle the loop's ends only while these lines stand
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'distillclip_amd', 'csrc')
    optim, common = open(os.path.join(csrc, 'optim.hip')).read(), open(os.path.join(csrc, 'common.h')).read()
    assert 'const int per_range = 8192 / count < 256 ? 256 : 8192 / count;' in optim
    assert 'grid = dim3(grid_for(longest, 256, per_range), (unsigned)count);' in optim
    assert 'const int64_t stride = (int64_t)gridDim.x * 256;' in optim
    assert 'int64_t g = (work + per_block - 1) / per_block;' in common and 'return (int)(g < 1 ? 1 : (g > cap ? cap : g));' in common
