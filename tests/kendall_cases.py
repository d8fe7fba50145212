"""Cases and the integer reference of the Kendall tau tests (dclip_kendall_tau, metrics.kendall_tau, HumanCorrelation).

The reference forms the sign matrices of x and y over the upper triangle i < j in row chunks, sums them in int64, counts the distinct
values with np.unique on its own, and forms both taus in float64 from the integers as scipy.stats.kendalltau defines them.  Comparisons
are IEEE f32 comparisons, as in the kernel.  tests/test_kendall_cpu.py checks this reference against SciPy; the GPU tests demand EQUALITY
of the eight integers and 1e-14 on the taus (both sides take about a dozen double roundings; one miscounted pair moves tau by at least
about 1 / n0 >= 2.9e-11 at the cap on n)."""
import functools

import numpy as np

ROW_BLOCK, TILE = 64, 128                # kendall.hip: KT_ROWS, KT_TILE (test_kendall_cpu.py reads them from the source)
MAX_N, MAX_C = 262144, 4
# 2..4099 as the issue lists them, and T - 1, T, T + 1, 2 T + 1 for T = 64 and T = 128
SIZES = (2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4099)
SEEDS = (0, 1, 2)
FAMILIES = ('ratings14', 'thirds', 'quant5', 'rep3')
SLOTS = ('con', 'dis', 'tie_x', 'tie_y', 'tie_xy', 'distinct_x', 'distinct_y', 'nan')
TAU_TOL = 1e-14


def counts(x, y, chunk=512):
    """x, y: [n] -> the 8 slots of dclip_kendall_tau as Python ints"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n = x.shape[0]
    assert x.shape == y.shape == (n,)
    con = dis = tie_x = tie_y = tie_xy = 0
    cols = np.arange(n)
    for s in range(0, n, chunk):
        xi, yi = x[s:s + chunk, None], y[s:s + chunk, None]
        upper = cols[None, s:] > cols[s:s + chunk, None]                     # j > i
        xj, yj = x[None, s:], y[None, s:]
        sx = (xi > xj).astype(np.int8) - (xi < xj).astype(np.int8)
        sy = (yi > yj).astype(np.int8) - (yi < yj).astype(np.int8)
        p = sx * sy
        ex, ey = (xi == xj) & upper, (yi == yj) & upper
        con += int(((p > 0) & upper).sum(dtype=np.int64))
        dis += int(((p < 0) & upper).sum(dtype=np.int64))
        tie_x += int(ex.sum(dtype=np.int64))
        tie_y += int(ey.sum(dtype=np.int64))
        tie_xy += int((ex & ey).sum(dtype=np.int64))
    nan = int((np.isnan(x) | np.isnan(y)).sum())
    return [con, dis, tie_x, tie_y, tie_xy, distinct(x), distinct(y), nan]


def distinct(v):
    """an element counts when no earlier element equals it: -0 and +0 are one value, every NaN is its own"""
    return int(np.unique(np.asarray(v, dtype=np.float32), equal_nan=False).size)


def taus(slots, n):
    """(tau_b, tau_c) in float64 from the integers, as scipy.stats.kendalltau: NaN for a NaN input, a constant input"""
    con, dis, tie_x, tie_y, _, dx, dy, nan = slots
    n0 = n * (n - 1) // 2
    if nan:
        return float('nan'), float('nan')
    cmd = con - dis
    tb = tc = float('nan')
    if tie_x != n0 and tie_y != n0:
        tb = min(1.0, max(-1.0, cmd / np.sqrt(float(n0 - tie_x)) / np.sqrt(float(n0 - tie_y))))
    m = min(dx, dy)
    if m > 1:
        tc = min(1.0, max(-1.0, 2 * cmd / (n ** 2 * (m - 1) / m)))
    return float(tb), float(tc)


def reference(x, y):
    """x [C, n] or [n], y [n] -> (int64 [C, 8], float64 [C, 2])"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    slots = [counts(row, y) for row in x]
    return np.array(slots, dtype=np.int64), np.array([taus(s, x.shape[1]) for s in slots], dtype=np.float64)


def scipy_taus(x, y):
    """the second reference: float64 [C, 2] from scipy.stats.kendalltau(variant='b' | 'c')"""
    from scipy.stats import kendalltau
    x = np.atleast_2d(np.asarray(x, dtype=np.float32)).astype(np.float64)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    return np.array([[kendalltau(row, y, variant=v).statistic for v in 'bc'] for row in x], dtype=np.float64)


def tau_close(a, b):
    """relative 1e-14 (absolute 1e-14 around 0); NaN exactly where the other is NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a - b)
    with np.errstate(invalid='ignore'):
        ok = (d <= TAU_TOL * np.abs(b)) | ((np.abs(b) < TAU_TOL) & (d <= TAU_TOL))
    return bool((both_nan | (ok & ~np.isnan(a) & ~np.isnan(b))).all())


def n_vectors(family, n, seed):
    """1 to 4 score vectors, every count met at every size"""
    return 1 + (FAMILIES.index(family) + seed + n) % MAX_C


def case(family, n, seed, C=None):
    """-> x [C, n] f32, y [n] f32.  Vector c follows the ratings less closely than vector c - 1."""
    C = n_vectors(family, n, seed) if C is None else C
    r = np.random.RandomState(1000 * seed + 7 * FAMILIES.index(family) + n)
    if family == 'rep3':                                                                 # every score three times: A = 3 annotators who
        group = r.randint(0, 4, size=(n + 2) // 3)                                       # rate around the level the score follows
        level = np.clip(np.repeat(group, 3)[:n] + r.randint(-1, 2, size=n), 0, 3)
        x = np.repeat(r.randn(C, group.size) * (1.0 + np.arange(C)[:, None]) + group[None, :], 3, axis=1)[:, :n]
    else:
        level = r.randint(0, 4, size=n)
        x = r.randn(C, n) * (1.0 + np.arange(C)[:, None]) + level[None, :]
    y = (level / 3.0 if family == 'thirds' else level + 1.0).astype(np.float32)          # {0, 1/3, 2/3, 1} or {1, 2, 3, 4}
    if family == 'quant5':
        x = np.clip(np.round(x), 0, 4)
    return np.ascontiguousarray(x, dtype=np.float32), y


@functools.lru_cache(maxsize=None)
def case_with_reference(family, n, seed):
    """-> x, y, slots [C, 8], taus [C, 2]; computed once, shared, never written to"""
    x, y = case(family, n, seed)
    slots, t = reference(x, y)
    for a in (x, y, slots, t):
        a.setflags(write=False)
    return x, y, slots, t


REPORT_N, REPORT_A = 5664, 3                  # Flickr8k-Expert: 5 664 scores against 3 annotators each, n = 16 992


def report_case():
    """n = 16 992, C = 3: every score three times against ratings in {1, 2, 3, 4}"""
    return case('rep3', REPORT_N * REPORT_A, 5, C=3)


def tie_counts(v):
    """pairs of equal elements, from the multiplicities of np.unique (no NaN)"""
    _, mult = np.unique(np.asarray(v, dtype=np.float32), return_counts=True)
    return int((mult.astype(np.int64) * (mult.astype(np.int64) - 1) // 2).sum())


def joint_tie_counts(x, y):
    pairs = np.stack([np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)], axis=1)
    pairs = pairs + np.float32(0)                                                        # -0 -> +0: one value
    _, mult = np.unique(pairs, axis=0, return_counts=True)
    return int((mult.astype(np.int64) * (mult.astype(np.int64) - 1) // 2).sum())
