"""Cases, the integer reference and the Pearson bound of the rank-correlation tests (dclip_rank_correlation, metrics.rank_correlation,
HumanCorrelation.compute(stats=...)).

Reference.  Twice-ranks R_i = 2 #{v_j < v_i} + #{v_j == v_i} + 1 come from np.searchsorted (left and right) on the sorted f32 vector; a
NaN item compares false to everything, so its R is 1.  The three sums of the centred twice-ranks are int64 (|c_i| <= n <= 2^18: at most
2^54), rho is the defining expression in float64.  Pearson is exact: every f32 is a fraction with a power-of-two denominator
(fractions.Fraction(float) is exact), the sums of fractions are carried as integers over their common denominator (what Fraction
arithmetic does, without the gcds), r^2's numerator and denominator are exact integers and mpmath takes the one square root at 60
digits.  That costs a fraction of a second at n = 262 144 as well, so the larger sizes use it too.  tests/test_rankcorr_cpu.py checks
all of it against scipy.stats.rankdata, spearmanr and pearsonr, and the integer sums against literal Fraction sums.

Pearson bound, from the kernel's summation shape (rankcorr.hip), u = 2^-53.  With G = min(ceil(n / 1024), 256) workgroups of 256
lanes, a lane adds T = ceil(n / (256 G)) <= 4 terms in item order (T roundings: the first fma onto 0 rounds as well), the wave's xor
tree adds 6 levels, the workgroup's 4 waves 3 more in order, and the workgroup that adds the G <= 256 records repeats 6 + 3: every
sum is a tree of depth K = T + 18 <= 22, whose error is at most ((1 + u)^K - 1) sum |terms|.
  means       xm^ = fl(sum^ / n): |xm^ - xm| <= ex = (K + 1) u mean|x| (1 + small)
  centred     d^_i = fl(x_i - xm^) (x_i exact in double): one rounding; sum (x_i - xm^)(y_i - ym^) = sxy + n dx dy EXACTLY because the
              true centred values sum to 0, so a wrong mean enters at second order only: sxx^ = (sxx + n dx^2)(1 + theta),
              sxy^ = sxy + n dx dy + eps with |theta| <= (K + 2) u and |eps| <= (K + 2) u sqrt(sxx' syy') by Cauchy-Schwarz
              (sxx' = sxx + n ex^2), the 2 being the roundings of d^x and d^y
  quotient    one product, one correctly rounded root (two roundings), one division: 4 u
  |r^ - r| <= [(K + 2) sqrt((1 + ax)(1 + ay)) + (K + 2) + 4] u + n ex ey / sqrt(sxx syy) + (ax + ay) / 2,   ax = n ex^2 / sxx, ay alike
with |r| <= 1 used for the relative terms and 1 % on top for the products of small terms.  Nothing in it is fitted to the kernel's output.
The bound is on the value before clipping; clipping to [-1, 1] only moves a result towards the exact one."""
import fractions
import functools
import math

import numpy as np

import kendall_cases as kc

SIZES, SEEDS, FAMILIES = kc.SIZES, kc.SEEDS, kc.FAMILIES           # the fourteen sizes, three seeds and four families of the Kendall tests
MAX_N, MAX_C = kc.MAX_N, kc.MAX_C
SUM_SLOTS = ('sxy', 'sxx', 'syy', 'nan')
RHO_TOL = 1e-14
SCIPY_R_TOL = 1e-12
# rankcorr.hip: RS_THREADS, RS_PER_BLOCK, RS_MAXGRID (test_rankcorr_cpu.py reads them from the source)
SUMS_THREADS, SUMS_PER_BLOCK, SUMS_MAXGRID = 256, 1024, 256
U = 2.0 ** -53


# ---- twice-ranks and Spearman ---------------------------------------------------------------------------------------------------------
def twice_ranks(v):
    """[n] f32 -> int64 [n]: R_i = 2 L_i + Q_i + 1"""
    v = np.asarray(v, dtype=np.float32)
    s = np.sort(v)                                                 # NaNs last; -0 and +0 compare equal
    lo, hi = np.searchsorted(s, v, side='left'), np.searchsorted(s, v, side='right')
    r = (lo + hi + 1).astype(np.int64)                             # 2 lo + (hi - lo) + 1
    r[np.isnan(v)] = 1
    return r


def rank_sums(rx, ry, x, y):
    """-> [Sxy, Sxx, Syy, nan items] as Python ints"""
    n = rx.shape[0]
    cx, cy = rx.astype(np.int64) - (n + 1), ry.astype(np.int64) - (n + 1)
    assert n <= MAX_N and max(np.abs(cx).max(), np.abs(cy).max()) <= n               # every int64 sum below stays within 2^54
    return [int((cx * cy).sum()), int((cx * cx).sum()), int((cy * cy).sum()), int((np.isnan(x) | np.isnan(y)).sum())]


def rho_from_sums(s):
    sxy, sxx, syy, nan = s
    if nan or sxx == 0 or syy == 0:
        return float('nan')
    return min(1.0, max(-1.0, float(sxy) / (math.sqrt(float(sxx)) * math.sqrt(float(syy)))))


# ---- exact Pearson --------------------------------------------------------------------------------------------------------------------
def _scaled_ints(v):
    """[n] finite f32 -> (Python ints m_i, k) with v_i == m_i / 2^k exactly"""
    ratios = [float(t).as_integer_ratio() for t in v]
    k = max(d.bit_length() - 1 for _, d in ratios)
    return [m << (k - (d.bit_length() - 1)) for m, d in ratios], k


def pearson_exact(x, y):
    """-> (r as float, float(sxx), float(syy)) from exact rational sums; NaN for a NaN, an inf or a constant vector"""
    import mpmath
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n = x.shape[0]
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return float('nan'), float('nan'), float('nan')
    (xi, kx), (yi, ky) = _scaled_ints(x), _scaled_ints(y)
    sx, sy = sum(xi), sum(yi)
    nxy = n * sum(a * b for a, b in zip(xi, yi)) - sx * sy         # n sxy 2^(kx + ky), exactly
    nxx = n * sum(a * a for a in xi) - sx * sx                     # n sxx 2^(2 kx)
    nyy = n * sum(b * b for b in yi) - sy * sy
    fxx, fyy = float(fractions.Fraction(nxx, n << (2 * kx))), float(fractions.Fraction(nyy, n << (2 * ky)))
    if nxx == 0 or nyy == 0:
        return float('nan'), fxx, fyy
    with mpmath.workdps(60):
        r = mpmath.mpf(nxy) / mpmath.sqrt(mpmath.mpf(nxx) * mpmath.mpf(nyy))
        return float(r), fxx, fyy


def sum_depth(n):
    """K of the docstring: the depth of every double sum of rank_sums_kernel and rank_finalize_kernel at n items"""
    grid = min(-(-n // SUMS_PER_BLOCK), SUMS_MAXGRID)
    per_lane = -(-n // (SUMS_THREADS * grid))
    return per_lane + 6 + 3 + 6 + 3


def pearson_bound(x, y, sxx, syy):
    """the bound of the docstring on |r^ - r|; sxx, syy: the exact centred sums as floats (pearson_exact)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, K = x.shape[0], sum_depth(x.shape[0])
    ex, ey = (K + 1) * U * np.abs(x).mean(), (K + 1) * U * np.abs(y).mean()
    ax, ay = n * ex * ex / sxx, n * ey * ey / syy
    rounding = ((K + 2) * math.sqrt((1 + ax) * (1 + ay)) + (K + 2) + 4) * U
    return 1.01 * (rounding + n * ex * ey / math.sqrt(sxx * syy) + 0.5 * (ax + ay))


# ---- the whole reference --------------------------------------------------------------------------------------------------------------
def reference(x, y):
    """x [C, n] or [n], y [n] -> dict: ranks int64 [C + 1, n] (the ratings last), sums int64 [C, 4], rho, r, bound float64 [C]"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    y = np.asarray(y, dtype=np.float32)
    ry = twice_ranks(y)
    ranks, sums, rho, r, bound = [], [], [], [], []
    for row in x:
        rx = twice_ranks(row)
        s = rank_sums(rx, ry, row, y)
        ranks.append(rx)
        sums.append(s)
        rho.append(rho_from_sums(s))
        if s[3]:
            pr, b = float('nan'), float('nan')
        else:
            pr, fxx, fyy = pearson_exact(row, y)
            b = pearson_bound(row, y, fxx, fyy) if not math.isnan(pr) else float('nan')
        r.append(pr)
        bound.append(b)
    return dict(ranks=np.array(ranks + [ry], dtype=np.int64), sums=np.array(sums, dtype=np.int64), rho=np.array(rho, dtype=np.float64),
                r=np.array(r, dtype=np.float64), bound=np.array(bound, dtype=np.float64))


def scipy_reference(x, y):
    """the second reference: (rho, r) float64 [C] from scipy.stats.spearmanr and pearsonr on the float64 copies"""
    import warnings
    from scipy.stats import pearsonr, spearmanr
    x = np.atleast_2d(np.asarray(x, dtype=np.float32)).astype(np.float64)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')                            # constant input, inf - inf
        rho = [spearmanr(row, y).statistic for row in x]
        r = [pearsonr(row, y).statistic if x.shape[1] > 1 else float('nan') for row in x]
    return np.array(rho, dtype=np.float64), np.array(r, dtype=np.float64)


def close(a, b, tol):
    """|a - b| <= tol elementwise (tol a number or an array); NaN exactly where the other is NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid='ignore'):
        ok = np.abs(a - b) <= tol
    return bool((both_nan | (ok & ~np.isnan(a) & ~np.isnan(b))).all())


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
PEARSON_FAMILY = 'offset20'
ALL_FAMILIES = FAMILIES + (PEARSON_FAMILY,)


def case(family, n, seed, C=None):
    """-> x [C, n] f32, y [n] f32.  The four Kendall families, and 'offset20': values 2^20 + k ulp with small integer k (ulp = 1/8 at
    2^20), where the mean is large against the spread: a one-pass or f32-mean Pearson loses every digit there."""
    if family != PEARSON_FAMILY:
        return kc.case(family, n, seed, C)
    C = 1 + (seed + n) % MAX_C if C is None else C
    r = np.random.RandomState(5000 * seed + n)
    level = r.randint(-4, 5, size=n)
    if n >= 2 and level.min() == level.max():
        level[0] += 1                                              # (never constant: that is a case of its own)
    k = level[None, :] * (1 + np.arange(C))[:, None] % 7 + r.randint(-3, 4, size=(C, n))
    k[:, 0] = k[:, 0] + 9                                          # (and never a constant score vector)
    x = (2.0 ** 20 + k / 8.0).astype(np.float32)
    y = (2.0 ** 20 + level / 8.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), 2.0 ** 20 + k / 8.0)
    return np.ascontiguousarray(x), y


@functools.lru_cache(maxsize=None)
def case_with_reference(family, n, seed):
    """-> x, y, reference dict; computed once, shared, never written to"""
    x, y = case(family, n, seed)
    ref = reference(x, y)
    for a in (x, y) + tuple(ref.values()):
        a.setflags(write=False)
    return x, y, ref
