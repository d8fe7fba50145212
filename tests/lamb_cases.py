"""Cases, float64 restatement and derived bounds of the trust-ratio (LAMB) tests (csrc/lamb.hip: lamb_moments_kernel, lamb_ratio_kernel,
lamb_apply_kernel through dclip_lamb_table; FusedAdamW(trust_ratio=True)).  tests/test_lamb_gpu.py runs them on the device,
tests/test_lamb_cpu.py holds the host side and checks the restatement against a per-tensor loop.  Layouts, input families and guarded
buffers are those of tests/adamw_groups_cases.py (gc) and tests/adamw_cases.py (ac): the lengths 4 ... 24 580 (one lane, a tile edge, three tiles
plus four elements), 1, 7, 25 and 70 ranges with frozen gaps between them, every range with its own lr_scale (0 included) and weight decay
(0 included), NaN guard words around every buffer.

RESTATEMENT (include/dclip.h: dclip_lamb_table), in float64 from the f32 inputs; lr_k = f32(lr) * f32(lr_scale_k) rounded once, bc1, bc2s and
the multiplier gs GIVEN f32 numbers; per unit k (one range of the table):

    g' = g gs ;  m' = b1 m + (1 - b1) g' ;  v' = b2 v + (1 - b2) g'^2                    (ac.reference's lines)
    q  = (m' / bc1) / (sqrt(v') / bc2s + eps) ;  u = q + wd_k p
    r_k = |p| / |u| if (wd_k != 0 or always_adapt) and both norms are > 0 and finite, else 1 ;  r_k = min(r_k, trust_clip)
    p' = p - lr_k r_k u

BOUNDS, derived from the operations the kernels perform; U = ac.U bounds one f32 rounding, T = 2^-126 is ac's absolute floor.
  m', v'   tm, tv of ac.moment_bounds: the lines are shared with the AdamW kernels (adam_moments in csrc/optim_elem.h).
  u        den carries ac's tden (square root, quotient by bc2s, sum with eps).  q is two correctly rounded divisions, u one fmaf:
               tq = [ tm / (bc1 den) + |q| (tden / den + 3 U) ] (1 + 2^-20) + T      (two roundings, the third U is spare; the factor pays for
                                                                                     the denominator being off by tden / den < 2^-21)
               tu = tq + U (|u| + tq) + T
  sums     a lane adds at most 8 squares per component by fmaf and joins the four components by two additions: at most 10 roundings over
           non-negative terms, relative error G = (1 + U)^10 - 1 of its sum, so of the tile's and the unit's; everything above the lane
           is added in double (below 2^-40 relatively), and a square that underflows costs at most 2^-149 absolutely, n 2^-149 for the unit.
  norms    the kernel squares its OWN u, which is within tu of the reference's element by element, so |u^| lies within |tu|_2 of |u|
           (triangle inequality); p is exact.  With S the reference's sum of squares and d = |tu|_2 (0 for p):
               lo = sqrt(max(0, (max(0, sqrt S - d))^2 (1 - G - 2^-40) - n 2^-149)) (1 - 2^-50) ,  hi likewise with +
           is where the double norm lies; the f32 in stats[k] is one more rounding (1 +- U) and a subnormal's 2^-149.
  r        the quotient of the double norms, rounded once: inside [lo_p / hi_u, hi_p / lo_u] (1 -+ U).  A unit that does not adapt has
           r = 1 with no tolerance; with trust_clip, an interval wholly above the clip gives the clip with no tolerance, one wholly
           below it is unclipped, one that straddles it keeps the interval's bound (the planted cases avoid that).
  p'       l = fl(lr_k r^) is off by tl = lr_k tr + U lr_k (r + tr); p' = fmaf(-l, u^, p) is one rounding:
               tp = e + U (|p'| + e) + T ,  e = tl |u| + lr_k r tu + tl tu          (the product's error in full, no term dropped)
Nothing here is fitted to what the kernels return; tests/test_lamb_cpu.py shows that an f32 emulation of the kernels' operation order
stays inside the bounds and that two wrong forms (AdamW's decay outside the update; the norm of the gradient in place of |u|) fall outside."""
import functools

import numpy as np

import adamw_cases as ac
import adamw_groups_cases as gc

U, T, S = ac.U, ac.T, 2.0 ** -149
G = (1 + U) ** 10 - 1
COUNTS = gc.COUNTS
FAMILIES = ac.FAMILIES
CLIP = 0.5                                               # the planted trust_clip
KS = (-7, 5, 12)                                         # the powers of two of the exact invariants


def units_of(count, wd=None):
    """gc.ranges_of(count): ((begin, length, lr_scale, weight_decay), ...), total; wd: every unit's decay replaced"""
    ranges, total = gc.ranges_of(count)
    if wd is not None:
        ranges = tuple((b, n, s, wd) for b, n, s, _ in ranges)
    return ranges, total


def _seg(x, ranges):
    """sum of x over every range, in float64 -> [count]"""
    return np.array([float(np.sum(x[b:b + n], dtype=np.float64)) for b, n, _, _ in ranges])


def _per_element(ranges, total, col):
    """column `col` of the ranges, as the f32 the table holds, spread over their elements"""
    out = np.zeros(total)
    for r in ranges:
        out[r[0]:r[0] + r[1]] = float(np.float32(r[col]))
    return out


def reference(flat, ranges, h, bc1, bc2s, gs=None, clip=None, adapt=False):
    """float64, whole flat buffers at once (module docstring).  h = (lr, b1, b2, eps) f32-valued floats.
    -> dict m, v, u, p (flat; outside the ranges m, v, p are the inputs and u is 0), np, nu, rfree, r (per unit), lrk"""
    lr, b1, b2, eps = h
    p, g, m, v = (np.asarray(flat[k], dtype=np.float64) for k in 'pgmv')
    total = p.size
    mask = gc.inside_mask(ranges, total)
    wd = _per_element(ranges, total, 3)
    lrk = np.array([gc.lr_of(lr, s) for _, _, s, _ in ranges])
    with np.errstate(all='ignore'):
        if gs is not None:
            g = g * float(gs)
        m2 = np.where(mask, b1 * m + (1 - b1) * g, m)
        v2 = np.where(mask, b2 * v + (1 - b2) * g * g, v)
        den = np.sqrt(v2) / float(bc2s) + eps
        q = (m2 / float(bc1)) / den
        u = np.where(mask, q + wd * p, 0.0)
        n_p, n_u = np.sqrt(_seg(p * p, ranges)), np.sqrt(_seg(u * u, ranges))
        adapts = np.array([adapt or float(np.float32(r[3])) != 0.0 for r in ranges])
        ok = adapts & (n_p > 0) & (n_u > 0) & np.isfinite(n_p) & np.isfinite(n_u)
        rfree = np.where(ok, n_p / np.where(ok, n_u, 1.0), 1.0)
        r = rfree if clip is None else np.minimum(rfree, float(clip))
        step = np.zeros(total)
        for k, (b, n, _, _) in enumerate(ranges):
            step[b:b + n] = lrk[k] * r[k]
        p2 = np.where(mask, p - step * u, p)
    return dict(m=m2, v=v2, u=u, q=np.where(mask, q, 0.0), den=den, p=p2, np=n_p, nu=n_u, rfree=rfree, r=r, lrk=lrk, adapts=adapts, ok=ok)


def bounds(flat, ranges, h, bc1, bc2s, gs=None, clip=None, adapt=False, ref=None):
    """-> dict tm, tv, tu, tp (flat), tnp, tnu (for the f32 norms in stats), tr (per unit), exact_r (per unit: no tolerance)"""
    lr, b1, b2, eps = h
    ref = reference(flat, ranges, h, bc1, bc2s, gs, clip, adapt) if ref is None else ref
    p = np.asarray(flat['p'], dtype=np.float64)
    tm, tv = ac.moment_bounds(flat['g'], flat['m'], flat['v'], (lr, b1, b2, eps, 0.0), gs)
    with np.errstate(all='ignore'):
        v2, den, q, u = ref['v'], ref['den'], ref['q'], ref['u']
        root = np.sqrt(v2)
        dsq = np.where(tv < v2, tv / (root * (1 + np.sqrt(np.maximum(0.0, 1 - tv / v2)))), np.inf)
        dsq = np.minimum(np.sqrt(tv), dsq)
        tden = (dsq + 2 * U * root) / float(bc2s) + U * den
        mask = gc.inside_mask(ranges, p.size)
        assert float((tden[mask] / den[mask]).max()) < 2.0 ** -21, 'eps is too small for the first-order bound of the denominator'
        tq = (tm / (float(bc1) * den) + np.abs(q) * (tden / den + 3 * U)) * (1 + 2.0 ** -20) + T
        tu = np.where(mask, tq + U * (np.abs(u) + tq) + T, 0.0)
        d_u = np.sqrt(_seg(tu * tu, ranges))
        ns = np.array([r[1] for r in ranges], dtype=np.float64)

        def interval(norm, d):
            lo = np.sqrt(np.maximum(0.0, np.maximum(0.0, norm - d) ** 2 * (1 - G - 2.0 ** -40) - ns * S)) * (1 - 2.0 ** -50)
            hi = np.sqrt((norm + d) ** 2 * (1 + G + 2.0 ** -40) + ns * S) * (1 + 2.0 ** -50)
            return lo, hi
        p_lo, p_hi = interval(ref['np'], 0.0)
        u_lo, u_hi = interval(ref['nu'], d_u)
        tnp = np.maximum(p_hi * (1 + U) - ref['np'], ref['np'] - p_lo * (1 - U)) + S
        tnu = np.maximum(u_hi * (1 + U) - ref['nu'], ref['nu'] - u_lo * (1 - U)) + S
        r_lo = np.where(ref['ok'], p_lo / np.where(u_hi > 0, u_hi, 1.0) * (1 - U), 1.0)
        r_hi = np.where(ref['ok'], np.where(u_lo > 0, p_hi / np.where(u_lo > 0, u_lo, 1.0), np.inf) * (1 + U), 1.0)
        exact = ~ref['ok']
        if clip is not None:
            exact = exact | (r_lo > clip)
            r_lo, r_hi = np.minimum(r_lo, clip), np.minimum(r_hi, clip)
        tr = np.where(exact, 0.0, np.maximum(r_hi - ref['r'], ref['r'] - r_lo))
        tp = np.zeros(p.size)
        for k, (b, n, _, _) in enumerate(ranges):
            lrk, r = ref['lrk'][k], ref['r'][k]
            tl = lrk * tr[k] + U * lrk * (r + tr[k])
            e = tl * np.abs(u[b:b + n]) + lrk * r * tu[b:b + n] + tl * tu[b:b + n]
            tp[b:b + n] = e + U * (np.abs(ref['p'][b:b + n]) + e) + T
    return dict(tm=tm, tv=tv, tu=tu, tp=tp, tnp=tnp, tnu=tnu, tr=tr, exact_r=exact)


def judge(flat, got, stats, ranges, h, pairs, gs=None, clip=None, adapt=False, label=''):
    """got: {p, m, v: flat f32 after the call}, stats: f32 [count, 4].  m' and v' do not depend on the bias corrections; the norms, r and
    p' must lie inside their bounds, all of them, under ONE of `pairs` (ac.candidates: the host's powf is within 0.52 ulp).
    -> {'m', 'v', 'np', 'nu', 'r', 'p': worst err / bound}"""
    mask = gc.inside_mask(ranges, flat['p'].size)
    worst = []
    for k, (bc1, bc2s) in enumerate(pairs):
        ref = reference(flat, ranges, h, bc1, bc2s, gs, clip, adapt)
        bd = bounds(flat, ranges, h, bc1, bc2s, gs, clip, adapt, ref)
        if k == 0:
            rm, im = ac._ratio(got['m'][mask], ref['m'][mask], bd['tm'][mask], "m'", label)
            rv, iv = ac._ratio(got['v'][mask], ref['v'][mask], bd['tv'][mask], "v'", label)
            assert rm <= 1 and rv <= 1, f"{label}: m' err / bound {rm:.3f} (element {im}), v' {rv:.3f} (element {iv})"
        assert np.isfinite(bd['tr']).all() and np.isfinite(bd['tp'][mask]).all(), f'{label}: a bound is not finite'
        out = {'m': rm, 'v': rv}
        out['np'] = float((np.abs(stats[:, 0].astype(np.float64) - ref['np']) / bd['tnp']).max())
        out['nu'] = float((np.abs(stats[:, 1].astype(np.float64) - ref['nu']) / bd['tnu']).max())
        dr = np.abs(stats[:, 2].astype(np.float64) - ref['r'])
        out['r'] = float(np.where(bd['exact_r'], np.where(dr == 0, 0.0, np.inf), dr / np.where(bd['exact_r'], 1.0, bd['tr'])).max())
        out['p'] = ac._ratio(got['p'][mask], ref['p'][mask], bd['tp'][mask], "p'", label)[0]
        if max(out['np'], out['nu'], out['r'], out['p']) <= 1:
            return out
        worst.append((max(out['np'], out['nu'], out['r'], out['p']), float(bc1), float(bc2s), out))
    w = min(worst, key=lambda x: x[0])
    raise AssertionError(f'{label}: no candidate pair of bias corrections holds every bound; the best, bc1 = {w[1]!r}, bc2s = {w[2]!r}, leaves err / bound {w[3]}')


def brute_force(flat, ranges, h, bc1, bc2s, gs=None, clip=None, adapt=False):
    """the same arithmetic, tensor by tensor on slices, with numpy's own norm -> (p' flat, [(|p|, |u|, r)])"""
    lr, b1, b2, eps = h
    out, rows = np.array(flat['p'], dtype=np.float64), []
    for b, n, s, wd in ranges:
        p, g, m, v = (np.asarray(flat[k][b:b + n], dtype=np.float64) for k in 'pgmv')
        g = g if gs is None else g * float(gs)
        m2, v2 = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        u = (m2 / float(bc1)) / (np.sqrt(v2) / float(bc2s) + eps) + float(np.float32(wd)) * p
        n_p, n_u = float(np.linalg.norm(p)), float(np.linalg.norm(u))
        r = n_p / n_u if (adapt or float(np.float32(wd)) != 0.0) and n_p > 0 and n_u > 0 and np.isfinite(n_p) and np.isfinite(n_u) else 1.0
        r = r if clip is None else min(r, float(clip))
        out[b:b + n] = p - gc.lr_of(lr, s) * r * u
        rows.append((n_p, n_u, r))
    return out, rows


# ---- f32 emulation of the kernels' operation order, and two wrong forms -------------------------------------------------------------------------
def emulate(flat, ranges, h, bc1, bc2s, gs=None, clip=None, adapt=False):
    """numpy f32 with the kernels' roundings (the sums of squares in f32 per 32 elements, then double) -> p', m', v' (flat f32), stats [count, 4]"""
    f = np.float32
    lr, b1, b2, eps = (f(x) for x in h)
    bc1, bc2s, one = f(bc1), f(bc2s), f(1)
    p2, m2, v2 = (np.array(flat[k], dtype=f) for k in 'pmv')
    stats = np.zeros((len(ranges), 4), dtype=f)
    with np.errstate(all='ignore'):
        for k, (b, n, s, wd) in enumerate(ranges):
            p, g, m, v = (np.asarray(flat[x][b:b + n], dtype=f) for x in 'pgmv')
            g = g if gs is None else g * f(gs)
            m2[b:b + n] = mk = b1 * m + (one - b1) * g
            v2[b:b + n] = vk = b2 * v + ((one - b2) * g) * g
            u = ac._fma(np.full_like(p, f(wd)), p, (mk / bc1) / (np.sqrt(vk) / bc2s + eps))

            def sumsq(x):                                # four chains of eight fused multiply-adds, joined by two additions, then double
                x = np.concatenate([x, np.zeros(-len(x) % 32, dtype=f)]).reshape(-1, 8, 4)
                acc = np.zeros((len(x), 4), dtype=f)
                for j in range(8):
                    acc = ac._fma(x[:, j], x[:, j], acc)
                return float(np.sum(((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])).astype(np.float64)))
            n_p, n_u = np.sqrt(sumsq(p)), np.sqrt(sumsq(u))
            r = one
            if (adapt or f(wd) != 0) and f(n_p) > 0 and f(n_u) > 0 and np.isfinite(f(n_p)) and np.isfinite(f(n_u)):
                r = f(n_p / n_u)
            if clip is not None and r > f(clip):
                r = f(clip)
            stats[k] = (n_p, n_u, r, 0)
            step = f(f(lr) * f(s)) * r
            p2[b:b + n] = ac._fma(np.full_like(u, -step), u, p)
    return p2, m2, v2, stats


def wrong(form, flat, ranges, h, bc1, bc2s, gs=None):
    """p' of a wrong form, in float64 with always_adapt: 'decay_outside' (AdamW's p (1 - lr wd), u without wd p), 'grad_norm' (|g| for |u|)"""
    lr, b1, b2, eps = h
    out = np.array(flat['p'], dtype=np.float64)
    for b, n, s, wd in ranges:
        p, g, m, v = (np.asarray(flat[k][b:b + n], dtype=np.float64) for k in 'pgmv')
        g = g if gs is None else g * float(gs)
        m2, v2 = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        q = (m2 / float(bc1)) / (np.sqrt(v2) / float(bc2s) + eps)
        lrk, wd = gc.lr_of(lr, s), float(np.float32(wd))
        if form == 'decay_outside':
            out[b:b + n] = p * (1 - lrk * wd) - lrk * (np.linalg.norm(p) / np.linalg.norm(q)) * q
        elif form == 'grad_norm':
            u = q + wd * p
            out[b:b + n] = p - lrk * (np.linalg.norm(p) / np.linalg.norm(g)) * u
        else:
            raise KeyError(form)
    return out


# ---- planted inputs -------------------------------------------------------------------------------------------------------------------------------
H4 = ac.HYPER[:4]                                        # (lr, b1, b2, eps)


@functools.lru_cache(maxsize=None)
def planted(kind, count=25):
    """-> flat {p, g, m, v, e} (read-only), ranges, total.
    'zero_p': p of every third unit all zero; 'zero_u': g, m, v of every third unit all zero and every decay 0 (with always_adapt: u = 0);
    'clip': p of every even unit x 10^5 (u is then wd p, r = 1 / wd >= 3.3, or |p| / |q| without decay), so that its free ratio lies far above CLIP and the others' far below"""
    ranges, total = units_of(count, 0.0 if kind == 'zero_u' else None)
    base, _ = gc.inputs(count)
    flat = {k: np.array(a) for k, a in base.items()}
    for k, (b, n, _, _) in enumerate(ranges):
        if kind == 'zero_p' and k % 3 == 0:
            flat['p'][b:b + n] = 0
        elif kind == 'zero_u' and k % 3 == 0:
            for x in 'gmv':
                flat[x][b:b + n] = 0
        elif kind == 'clip' and k % 2 == 0:
            flat['p'][b:b + n] *= np.float32(1e5)
    for a in flat.values():
        a.setflags(write=False)
    return flat, ranges, total


def scaled(flat, k, what):
    """the inputs of the exact invariants: what = 'gmv': g, m x 2^k and v x 4^k; 'p': p (and e) x 2^k -- all exact in f32 for these magnitudes"""
    out = dict(flat)
    s = np.float32(2.0 ** k)
    if what == 'gmv':
        out['g'], out['m'], out['v'] = flat['g'] * s, flat['m'] * s, flat['v'] * s * s
        assert np.array_equal(out['v'].astype(np.float64), flat['v'].astype(np.float64) * 4.0 ** k)
    else:
        out['p'], out['e'] = flat['p'] * s, flat['e'] * s
    for x in 'pgmv':
        a = np.abs(out[x][out[x] != 0])
        assert a.size == 0 or (a.min() > 1e-30 and a.max() < 1e30)
    return out
