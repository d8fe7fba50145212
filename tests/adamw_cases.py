"""Reference, bound, input families and guarded buffers of the AdamW tests (csrc/optim.hip: adamw_elem in adamw_kernel and in the three
modes of adamw4_multi_kernel; entries dclip_adamw, dclip_adamw_multi, dclip_adamw_multi_scaled, dclip_adamw_multi_amp).

REFERENCE.  One step, in float64, from the f32 inputs and the f32-rounded hyper-parameters (the C ABI takes float).  bc1 and bc2s are
GIVEN f32 numbers (what the host formed, or what the record holds), g is replaced by g * gs when a multiplier is given:

    m'  = b1 m + (1 - b1) g
    v'  = b2 v + (1 - b2) g^2
    den = sqrt(v') / bc2s + eps
    p'  = p (1 - lr wd) - (lr / bc1) m' / den

which is torch.optim.AdamW (tests/test_adamw_exact_cpu.py holds it to torch on float64 for five steps).  Every step is checked on its
own, from the kernel's own f32 state, so no model of accumulated error is needed.

BOUND.  Per element, for round-to-nearest f32 arithmetic with correctly rounded division and square root (the library is built
without fast-math flags), whether or not the compiler contracts a product and a sum into one fused multiply-add (contraction only removes a
rounding).  u = 2^-24 bounds the relative error of one rounding, T = 2^-126 is the smallest normal number.  adamw_elem, operation
by operation, with 0.5 <= b1, b2 < 1 so that 1 - b1 and 1 - b2 are exact (Sterbenz), and gt = g gs:

    gt = g * gs                      1 rounding (none without a multiplier)
    m' = b1 * m + (1 - b1) * gt      term b1 m: product, sum = 2 roundings; term (1 - b1) gt: gt, product, sum = 3 roundings
         tm = 4 u am + T             am = |b1 m| + |(1 - b1) gt|; the fourth u is spare (it pays for a 1 - b1 that is not exact)
    v' = b2 * v + ((1 - b2) * gt) * gt
                                     term b2 v: 2 roundings; term (1 - b2) gt^2: gt twice, two products, sum = 5 roundings
         tv = 5 u v' + 4 T           both terms are >= 0, so the larger count times v' covers the sum
    s  = sqrtf(v')                   |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt |a - b|, and with |a - v'| <= tv:
         dsq = min( sqrt tv, tv / (sqrt v' (1 + sqrt(1 - tv / v'))) )          (the issue's tv / (2 sqrt v') to first order; this one is exact)
                                     then 1 rounding of the root itself
    den = s / bc2s + eps             1 rounding of the quotient, 1 of the sum
         tden = (dsq + 2 u sqrt v') / bc2s + u den
    c  = 1 - lr * wd                 product: u lr wd <= u / 2 absolute, as lr wd <= 1/2; difference: the result lies in [1/2, 1], where half
                                     a spacing is u / 2; together at most u absolute, at most 2 u relative to c >= 1/2
    pd = p * c                       1 rounding; with c: 3 u |p c|
    k  = lr / bc1                    1 rounding
    q  = m' / den                    1 rounding; its operands carry tm and tden
    p' = pd - k * q                  1 rounding of the product (none if contracted), 1 of the difference
         tp = 3 u |p c| + (lr / bc1) ( tm / den + |m'| / den (tden / den + 4 u) ) + u |p'| + T
                                     k, q and k q are 3 roundings; the fourth u is spare

T: under gradual underflow (the kernels keep f32 subnormals) an operation whose result is subnormal errs by at most 2^-150, so every T
above is an absolute floor far above what the arithmetic needs; it is there so that one result flushed to zero is tolerated too (an
error below T).  The four in tv are for the two products and the sum of v' and for a subnormal input v.
Second order: every line above is first order in u.  The products of first-order terms that were dropped are below 16 u times the
bound as long as tden / den < 2^-21 (asserted: it fails only if eps is so small that the floor 4 T decides the denominator), so every u
above is U = u (1 + 2^-20).  None of the issue's constants is loosened by more than that factor.

The bound is derived, not fitted: tests/test_adamw_exact_cpu.py shows that an f32 emulation of this operation order stays inside it,
contracted and not, and that five known wrong forms fall outside it.

NOT COVERED.  |g gs| >= 1e18 is tested nowhere: above about 1.8e19 g * g overflows f32, which torch's f32 AdamW computes, where the kernel's
((1 - b2) g) g overflows only above about 5.8e20; between the two the kernel is right and torch's f32 step is not, and the float64
reference leaves the f32 range.  Every bounded family keeps |g gs| < 1e18.

HOST BIAS CORRECTIONS.  dclip_adamw, _multi and _multi_scaled form bc1 = 1 - powf(b1, t) and bc2s = sqrtf(1 - powf(b2, t)) on the host;
powf is within 0.52 ulp of the correctly rounded power (the loss-scaler section).  candidates() gives the correctly rounded
f32 power and its two f32 neighbours through the f32 formulas; a call passes if ONE pair (bc1, bc2s) puts EVERY element inside the bound."""
import functools
import itertools

import numpy as np

U0, T = 2.0 ** -24, 2.0 ** -126
U = U0 * (1 + 2.0 ** -20)
LR, BETAS, EPS, WD = 3e-3, (0.9, 0.999), 1e-8, 1e-2
FAMILIES = ('normal', 'tiny', 'first', 'cancel', 'big', 'sub')
STEPS = (1, 2, 7, 1000, 100000)
GS_BIG = 2.0 ** -16
G_MAX = 1e18
GUARD_BITS = 0x7FC0BEEF                                  # a quiet NaN with a payload: an element read by mistake poisons its result
GUARD = 4


def hyper(lr=LR, betas=BETAS, eps=EPS, wd=WD):
    """-> (lr, b1, b2, eps, wd) as Python floats holding the f32 values the C ABI passes on"""
    return tuple(float(np.float32(x)) for x in (lr, betas[0], betas[1], eps, wd))


HYPER = hyper()


def reference(p, g, m, v, h, bc1, bc2s, gs=None):
    """float64 -> p', m', v' (module docstring); bc1, bc2s, gs are taken as they are given"""
    lr, b1, b2, eps, wd = h
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    with np.errstate(all='ignore'):
        if gs is not None:
            g = g * float(gs)
        m2 = b1 * m + (1 - b1) * g
        v2 = b2 * v + (1 - b2) * g * g
        den = np.sqrt(v2) / float(bc2s) + eps
        p2 = p * (1 - lr * wd) - (lr / float(bc1)) * m2 / den
    return p2, m2, v2


def moment_bounds(g, m, v, h, gs=None):
    """-> tm, tv"""
    lr, b1, b2, eps, wd = h
    assert 0.5 <= b1 < 1 and 0.5 <= b2 < 1 and lr * wd <= 0.5 and eps > 0
    g, m, v = (np.asarray(a, dtype=np.float64) for a in (g, m, v))
    with np.errstate(all='ignore'):
        if gs is not None:
            g = g * float(gs)
        tm = 4 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g)) + T
        tv = 5 * U * (b2 * v + (1 - b2) * g * g) + 4 * T
    return tm, tv


def bounds(p, g, m, v, h, bc1, bc2s, gs=None):
    """-> tp, tm, tv (module docstring), from the reference's own quantities"""
    lr, b1, b2, eps, wd = h
    p2, m2, v2 = reference(p, g, m, v, h, bc1, bc2s, gs)
    tm, tv = moment_bounds(g, m, v, h, gs)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all='ignore'):
        root = np.sqrt(v2)
        den = root / float(bc2s) + eps
        dsq = np.where(tv < v2, tv / (root * (1 + np.sqrt(np.maximum(0.0, 1 - tv / v2)))), np.inf)
        dsq = np.minimum(np.sqrt(tv), dsq)
        tden = (dsq + 2 * U * root) / float(bc2s) + U * den
        ok = np.isfinite(den)
        assert not ok.any() or float((tden[ok] / den[ok]).max()) < 2.0 ** -21, 'eps is too small for the first-order bound'
        tp = 3 * U * np.abs(p * (1 - lr * wd)) + (lr / float(bc1)) * (tm / den + np.abs(m2) / den * (tden / den + 4 * U)) + U * np.abs(p2) + T
    return tp, tm, tv


# ---- the host's bias corrections ---------------------------------------------------------------------------------------------------------
def power_candidates(beta, t):
    """the correctly rounded f32 of float64(beta)^t first, then its two f32 neighbours"""
    x = np.float32(float(np.float32(beta)) ** int(t))
    return [x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))]


def bc_of(x1, x2):
    """the f32 formulas of adamw_multi_launch on the two f32 powers -> (bc1, bc2s) as np.float32"""
    one = np.float32(1)
    return one - np.float32(x1), np.sqrt(one - np.float32(x2), dtype=np.float32)


def candidates(h, t):
    """[(bc1, bc2s)]: the pair of the correctly rounded powers first, no pair twice"""
    out = []
    for x1, x2 in itertools.product(power_candidates(h[1], t), power_candidates(h[2], t)):
        pair = bc_of(x1, x2)
        if not any(pair[0] == q[0] and pair[1] == q[1] for q in out):
            out.append(pair)
    return out


def exact_bc(h, t):
    """the pair of the correctly rounded powers: what the record of dclip_amp_prepare holds"""
    return candidates(h, t)[0]


def double_bc(h, t, b2=None):
    """(1 - b1^t, sqrt(1 - b2^t)) in float64, as torch.optim.AdamW forms them"""
    return 1 - h[1] ** t, float(np.sqrt(1 - (h[2] if b2 is None else b2) ** t))


def bc2s_distance(h, t, bc2s):
    """relative distance of an f32 bc2s from the float64 value: (with the f32-rounded beta2, with the double 0.999 it was rounded from)"""
    a, b = double_bc(h, t)[1], double_bc(h, t, BETAS[1] if h[2] == HYPER[2] else h[2])[1]
    return abs(float(bc2s) - a) / a, abs(float(bc2s) - b) / b


# ---- judging a result ----------------------------------------------------------------------------------------------------------------------
def _same_kind(got, want):
    """non-finite values of the same kind: NaN with NaN, an infinity with the same infinity"""
    return (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))


def _ratio(got, want, tol, what, label):
    """largest |got - want| / tol over the elements whose reference is finite; the others must be non-finite in the same way"""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want)
    bad = ~fin & ~_same_kind(got, want)
    assert not bad.any(), f'{label}: {what}[{int(np.argmax(bad))}] = {got[np.argmax(bad)]!r}, the reference is {want[np.argmax(bad)]!r}'
    if not fin.any():
        return 0.0, -1
    with np.errstate(all='ignore'):
        r = np.where(fin, np.abs(got - want) / tol, 0.0)
    r = np.where(np.isnan(r), np.inf, r)                 # a NaN where the reference is finite
    i = int(np.argmax(r))
    return float(r[i]), i


def judge(before, after, h, pairs, gs=None, label=''):
    """before = (p, g, m, v), after = (p', m', v') of one call, all elements of the call in one array each.  m' and v' do not depend on
    the bias corrections; p' must lie inside tp for every element under ONE of `pairs`.
    -> {'p': ratio, 'm': ratio, 'v': ratio, 'pair': (bc1, bc2s), 'tried': k}"""
    p, g, m, v = before
    tm, tv = moment_bounds(g, m, v, h, gs)
    worst = []
    for k, (bc1, bc2s) in enumerate(pairs):
        p2, m2, v2 = reference(p, g, m, v, h, bc1, bc2s, gs)
        if k == 0:
            rm, im = _ratio(after[1], m2, tm, "m'", label)
            rv, iv = _ratio(after[2], v2, tv, "v'", label)
            assert rm <= 1, f"{label}: m'[{im}] = {after[1][im]!r}, reference {m2[im]!r}, err / bound = {rm:.3f}"
            assert rv <= 1, f"{label}: v'[{iv}] = {after[2][iv]!r}, reference {v2[iv]!r}, err / bound = {rv:.3f}"
        tp = bounds(p, g, m, v, h, bc1, bc2s, gs)[0]
        rp, ip = _ratio(after[0], p2, tp, "p'", label)
        if rp <= 1:
            return {'p': rp, 'm': rm, 'v': rv, 'pair': (float(bc1), float(bc2s)), 'tried': k + 1}
        worst.append((rp, ip, float(bc1), float(bc2s), float(np.asarray(after[0])[ip]), float(p2[ip])))
    rp, ip, bc1, bc2s, got, want = min(worst)
    raise AssertionError(f"{label}: no candidate pair holds every p'; the best, bc1 = {bc1!r}, bc2s = {bc2s!r}, leaves p'[{ip}] = {got!r} "
                         f'against {want!r}, err / bound = {rp:.3f}')


# ---- input families ------------------------------------------------------------------------------------------------------------------------
def _loguniform(r, lo, hi, n):
    return np.exp(r.uniform(np.log(lo), np.log(hi), size=n))


def _signs(r, n):
    return r.randint(0, 2, size=n) * 2.0 - 1.0


def family(name, n, seed=0):
    """-> p, g, m, v (f32 [n]), gs (a float, or None: no multiplier is needed).  `first` is meant for t = 1, `big` carries loss-scaled
    gradients that want the multiplier 2^-16."""
    r = np.random.RandomState(1000 * seed + 17 * FAMILIES.index(name) + 3)
    p = 0.05 * r.randn(n)
    gs = None
    if name == 'normal':
        g, m = 1e-3 * r.randn(n), 1e-3 * r.randn(n)
        v = (g * r.uniform(0.5, 1.5, size=n)) ** 2
    elif name == 'tiny':                                  # eps = 1e-8 dominates sqrt(v') or ties with it; one magnitude per element, as
        s = _loguniform(r, 1e-11, 1e-6, n)                # a gradient and its running moments have
        g, m = s * r.randn(n), s * r.randn(n)
        v = (s * r.uniform(0.5, 1.5, size=n)) ** 2
    elif name == 'first':
        g = _signs(r, n) * _loguniform(r, 1e-10, 1.0, n)
        m, v = np.zeros(n), np.zeros(n)
    elif name == 'cancel':                                # b1 m + (1 - b1) g cancels to about 1e-6 of its terms
        g = 1e-3 * r.randn(n)
        m = -(1 - HYPER[1]) / HYPER[1] * g * (1 + 1e-6 * r.randn(n))
        v = (g * r.uniform(0.5, 1.5, size=n)) ** 2
    elif name == 'big':                                   # what a backward under a loss scale of 65536 leaves
        g = _signs(r, n) * _loguniform(r, 1.0, 2e6, n)
        m = GS_BIG * _signs(r, n) * _loguniform(r, 1.0, 2e6, n)
        v = (GS_BIG * g * r.uniform(0.5, 1.5, size=n)) ** 2
        gs = GS_BIG
    elif name == 'sub':                                   # g^2 is subnormal or zero in f32, v is too
        g, m = _signs(r, n) * _loguniform(r, 1e-24, 1e-17, n), _signs(r, n) * _loguniform(r, 1e-24, 1e-17, n)
        v = _loguniform(r, 1e-24, 1e-17, n) ** 2
    else:
        raise KeyError(name)
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (p, g, m, v))
    assert float(np.abs(out[1]).max()) * (1.0 if gs is None else gs) < G_MAX
    return out + (gs,)


@functools.lru_cache(maxsize=None)
def shared_family(name, n, seed=0):
    """family(), formed once, shared, never written to"""
    out = family(name, n, seed)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def steps_of(name):
    return (1,) if name == 'first' else STEPS


# ---- f32 emulations: the documented operation order, and five wrong forms --------------------------------------------------------------------
def _fma(a, b, c):
    """f32 fused multiply-add: the product of two f32 is exact in float64, the sum is rounded to float64 and then to f32 (the double
    rounding can move the last bit in rare cases, which an emulation may)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(p, g, m, v, h, bc1, bc2s, gs=None, contract=None):
    """adamw_elem in f32 numpy.  contract: None = every product and sum rounded; 'left' / 'right' = the sums of m' and v' fused with
    their left / right product, c and the final difference fused too"""
    f = np.float32
    lr, b1, b2, eps, wd = (f(x) for x in h)
    bc1, bc2s, one = f(bc1), f(bc2s), f(1)
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    with np.errstate(all='ignore'):
        if gs is not None:
            g = g * f(gs)
        k = lr / bc1
        if contract is None:
            pd = p * (one - lr * wd)
            m2 = b1 * m + (one - b1) * g
            v2 = b2 * v + ((one - b2) * g) * g
        else:
            pd = p * _fma(-np.asarray(lr), np.asarray(wd), np.asarray(one))
            if contract == 'left':
                m2 = _fma(np.full_like(m, b1), m, (one - b1) * g)
                v2 = _fma(np.full_like(v, b2), v, ((one - b2) * g) * g)
            else:
                m2 = _fma(np.full_like(g, one - b1), g, b1 * m)
                v2 = _fma((one - b2) * g, g, b2 * v)
        den = np.sqrt(v2) / bc2s + eps
        q = m2 / den
        p2 = pd - k * q if contract is None else _fma(np.full_like(q, -k), q, pd)
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


WRONG_FORMS = ('eps_in_root', 'eps_before_bc2s', 'bc2_without_root', 'decay_after_step', 'old_m')


def wrong(form, p, g, m, v, h, bc1, bc2s, gs=None):
    """p' of a known wrong form, in float64 so that the form is the only difference"""
    lr, b1, b2, eps, wd = h
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1, bc2s = float(bc1), float(bc2s)
    if gs is not None:
        g = g * float(gs)
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    den = np.sqrt(v2) / bc2s + eps
    k = lr / bc1
    if form == 'eps_in_root':
        return p * (1 - lr * wd) - k * m2 / (np.sqrt(v2 + eps) / bc2s)
    if form == 'eps_before_bc2s':
        return p * (1 - lr * wd) - k * m2 / ((np.sqrt(v2) + eps) / bc2s)
    if form == 'bc2_without_root':
        return p * (1 - lr * wd) - k * m2 / (np.sqrt(v2) / (bc2s * bc2s) + eps)
    if form == 'decay_after_step':
        return (p - k * m2 / den) * (1 - lr * wd)
    if form == 'old_m':
        return p * (1 - lr * wd) - k * m / den
    raise KeyError(form)


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------------------
NAMES = 'pgmv'


def layout(lens, offsets=(0, 0, 0, 0)):
    """-> {name: [(begin, end)]}, {name: words}: every range starts `offset` elements past a 16-byte boundary and has at least GUARD
    guard words before and after it"""
    spans, total = {}, {}
    for name, off in zip(NAMES, offsets):
        at, s = GUARD, []
        for n in lens:
            s.append((at + off, at + off + n))
            at = (at + off + n + 3) // 4 * 4 + GUARD
        spans[name], total[name] = s, at
    return spans, total


def host_buffers(ranges, offsets=(0, 0, 0, 0)):
    """ranges: [(p, g, m, v)] of f32 arrays -> {name: f32 buffer with the ranges between guard words}, spans"""
    spans, total = layout([len(r[0]) for r in ranges], offsets)
    bufs = {}
    for k, name in enumerate(NAMES):
        b = np.full(total[name], GUARD_BITS, dtype=np.uint32).view(np.float32)
        for (a, e), r in zip(spans[name], ranges):
            b[a:e] = r[k]
        bufs[name] = b
    return bufs, spans


def stride4(count, longest4):
    """float4 per grid-stride iteration of adamw4_multi_kernel: adamw_ranges' grid (grid_for(longest, 256, max(256, 8192 / count))) x 256"""
    cap = max(256, 8192 // count)
    return min(max((longest4 + 255) // 256, 1), cap) * 256
