"""Cases, float64 references and error bounds shared by tests/test_metrics_exact_cpu.py and tests/test_metrics_exact_gpu.py (the
validation-metrics kernel: include/dclip.h dclip_retrieval_metrics, csrc/metrics.hip).  Not a test module.

Bounds, derived, not measured (u = 2^-24; the inputs are f32, hence exact in float64):
  one element of a normalised row   (E / 2 + 3) u relative                                 recall_cases.py
  one logit                         b(E) = (2 E + 8) u absolute                            recall_cases.py (rc.bound)
  one planted logit                 4 u relative: the planted rows hold 0, 1 and 2 only, so a squared norm is an integer below 2^24,
                                    exact in any order of summation, and a dot product with a one-hot row is one product: all that
                                    rounds is the square root, the reciprocal and the product x * inv
  sexp_i = sum_j exp(L_ij - 1)      relative: b(E) from the logits (exp turns an absolute error of its argument into a relative one of
                                    its value), (ceil(ntile / 4) + 6) u from the additions, all of positive terms (a wave adds its
                                    ceil(ntile / 4) tiles, four shuffle steps over the 16 lanes of a row group, two additions over the
                                    four waves), and EXP_REL for __expf(S - 1) itself
  finalize                          (ceil(n / 256) + 12) u of sum |term| / n: ceil(n / 256) additions per thread, six shuffle steps, two
                                    additions over the waves, the division by n, and three for forming a term
EXP_REL is the one figure that nothing in the project yields: the relative error of __expf(S - 1.f) for S in [-1, 1], the subtraction
included.  It is MEASURED on the GPU (test_metrics_exact_gpu.py::test_expf_error_measured_on_single_rows: sexp of an n = 1 problem is
one such term, compared with float64 exp of the kernel's own diagonal, and the worst residual of sexp over all other cases after the
derived terms) and set to four times the worst value seen, rounded up to a power of two times u; four, because the cases sample only a
few thousand arguments.

Out of scope: n >= 2^24.  The entry admits n < 2^30, but the hit counts are summed in f32 and stop being exact integers there; such a
case cannot run in seconds."""
import functools
import math

import numpy as np
import torch

import recall_cases as rc

U = rc.U
# Measured on an MI355X: the worst relative error of __expf(S - 1.f) over the 2049 single-row problems is 3.283 u (at S = -0.9678; the
# mean is 0.64 u).  Over all other cases the worst residual of sexp after the derived terms is negative (planted -8.8 u, roles swapped
# -9.4 u, random -44.6 u): the derived terms are worst cases and the kernel stays well inside them, so the single rows decide.
# 4 x 3.283 u = 13.1 u, rounded up to a power of two times u:
EXP_REL = 16 * U

K_DEFAULT = (1, 3, 5, 10, 20, 50)


def k_lists(n):
    """the three cut-off lists of every planted case: the default, nk = 8 unsorted / repeated / above n, and none"""
    return [K_DEFAULT, (50, 1, 1, 1000, n, n - 1, 2, 7), ()]


def ntile(n):
    return (n + 15) // 16


def sexp_terms(n, E, logit_bound=None):
    """the derived part of sexp's relative bound (without EXP_REL): exp(b) - 1 from logits off by b, and the additions"""
    return math.expm1(rc.bound(E) if logit_bound is None else logit_bound) + (math.ceil(ntile(n) / 4) + 6) * U


def finalize_factor(n):
    return (math.ceil(n / 256) + 12) * U


def expected_acc(rank, ks):
    """out[0 .. nk) from the ranks: the kernel's own single f32 division of two exact integers"""
    rank = np.asarray(rank)
    return np.array([np.float32(int((rank < k).sum())) / np.float32(len(rank)) for k in ks], dtype=np.float32)


# ---- the workspace -----------------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) & ~255


def workspace_layout(n, E, query=None):
    """Mirror of the Bump carving in csrc/metrics.hip (dclip_retrieval_metrics): nimg f32 [n, E], ntxt f32 [n, E], rank i32 [n],
    sexp f32 [n], diag f32 [n], in this order, each piece rounded up to 256 bytes.  THIS DEPENDS ON THAT LAYOUT, which is no part of
    the C ABI: when metrics.hip carves its workspace differently, change this helper with it.  `query` is what
    dclip_retrieval_metrics_workspace(n, E) answers; a total that differs raises, and the tests that read the pieces compare every one
    with float64 and demand all-ones bits in the slack after each, so a reordered layout fails them too.
    -> ({name: (byte offset, live bytes, numpy dtype, shape)}, total bytes)"""
    pieces, off = {}, 0
    for name, dtype, shape in (('nimg', np.float32, (n, E)), ('ntxt', np.float32, (n, E)), ('rank', np.int32, (n,)),
                               ('sexp', np.float32, (n,)), ('diag', np.float32, (n,))):
        live = int(np.prod(shape)) * 4
        pieces[name] = (off, live, dtype, shape)
        off += up256(live)
    if query is not None and query != off:
        raise AssertionError(f'workspace layout of metrics.hip changed: the five pieces take {off} bytes, the query answers {query} '
                             f'(n={n}, E={E}); tests/metrics_cases.py: workspace_layout must follow csrc/metrics.hip')
    return pieces, off


# ---- 1. planted ranks ----------------------------------------------------------------------------------------------------------------
PLANTED_SIZES = [(1, 16), (15, 16), (16, 16), (17, 32), (63, 64), (64, 64), (65, 80), (130, 144), (257, 272)]      # (n, E)
LOW_RANK = 15                                  # rows of rank 1 .. LOW_RANK are the "low-rank rows" whose chosen columns visit every tile
PLANTED_LOGIT_REL = 4 * U


@functools.lru_cache(maxsize=None)
def planted_square(n, E, seed=7):
    """Columns are the one-hot rows e_j (so E >= n); row c is e_c + 2 sum of e_j over r_c chosen other j.  In float64
        L[c, j] = 2 / sqrt(1 + 4 r_c) on the chosen columns,  L[c, c] = 1 / sqrt(1 + 4 r_c),  0 elsewhere:  rank_c = r_c.
    In f32 the chosen logits are exactly twice the diagonal and the others exactly 0, whatever the roundings: the ranks are exact.
    r is a permutation of 0 .. n - 1: every rank occurs, n - 1 included (the last row has it).  The rows of rank 1 .. LOW_RANK place
    their chosen columns tile after tile, round robin, so that together they visit every column tile several times (every residue of
    the tile index mod 4 with it); the other rows choose at random.
    With the roles swapped (rows one-hot, columns planted) L[i, c] = 2 / sqrt(1 + 4 r_c) if i is chosen in c, 1 / sqrt(1 + 4 r_i) on
    the diagonal, 0 elsewhere: column c beats row i's diagonal iff i is chosen in c and 1 + 4 r_c < 4 (1 + 4 r_i), integers that are
    never equal (1 against 0 mod 4).
    -> rows f32 [n, E], cols f32 [n, E] (CPU tensors), r int64 [n], chosen bool [n, n], swapped ranks int64 [n]"""
    assert E >= n and E % 16 == 0
    rng = np.random.RandomState(1000 * seed + n)
    r = rng.permutation(n).astype(np.int64)
    last = int(np.nonzero(r == n - 1)[0][0])
    r[last], r[n - 1] = r[n - 1], n - 1                                         # the last row, alone in its panel when n % 16 == 1, sees every tile
    chosen = np.zeros((n, n), dtype=bool)
    nt, counter = ntile(n), 0
    for c in sorted(range(n), key=lambda c: r[c]):
        if 1 <= r[c] <= LOW_RANK and n > 64:
            for _ in range(r[c]):
                while True:
                    t = counter % nt
                    counter += 1
                    free = [j for j in range(16 * t, min(16 * t + 16, n)) if j != c and not chosen[c, j]]
                    if free:
                        break
                chosen[c, free[(7 * counter) % len(free)]] = True
        elif r[c]:
            others = np.array([j for j in range(n) if j != c])
            chosen[c, rng.choice(others, size=r[c], replace=False)] = True
    rows = np.zeros((n, E), dtype=np.float32)
    cols = np.zeros((n, E), dtype=np.float32)
    cols[np.arange(n), np.arange(n)] = 1.0
    rows[:, :n][chosen] = 2.0
    rows[np.arange(n), np.arange(n)] = 1.0
    swapped = np.array([sum(1 for c in range(n) if c != i and chosen[c, i] and 1 + 4 * int(r[c]) < 4 * (1 + 4 * int(r[i])))
                        for i in range(n)], dtype=np.int64)
    return torch.from_numpy(rows), torch.from_numpy(cols), r, chosen, swapped


def planted_logits(r, chosen):
    """the closed form of the planted logits in float64 -> L [n, n]"""
    inv = 1.0 / np.sqrt(1.0 + 4.0 * r.astype(np.float64))
    L = np.where(chosen, 2.0 * inv[:, None], 0.0)
    L[np.arange(len(r)), np.arange(len(r))] = inv
    return L


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------
TIE_SIZES = [(17, 32), (40, 48), (130, 144)]          # the planted case that is doubled: n = 34, 80, 260 (17 tiles)


def tied_square(n0, E):
    """The planted case twice: columns [cols; cols], rows [rows; rows], bit copies.  For row c and row n0 + c alike, the copy of its
    own diagonal column ties with the diagonal and must not count, and the copy of every column that was ahead is ahead again:
    every rank is exactly 2 r_c, where one counted tie would give 2 r_c + 1.
    -> rows, cols f32 [2 n0, E], ranks int64 [2 n0]"""
    rows, cols, r, _, _ = planted_square(n0, E)
    return torch.cat([rows, rows]), torch.cat([cols, cols]), np.concatenate([2 * r, 2 * r])


# ---- 3. random operands --------------------------------------------------------------------------------------------------------------
RANDOM_N = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 130, 257)
RANDOM_E = (16, 64, 512, 1024)
CORRS = (0.25, 0.05)                          # 0.25: most ranks 0 ; 0.05: the ranks spread
SEEDS = (0, 1, 2)
# picked so that the cap below holds (test_metrics_exact_cpu.py asserts it): at E = 64 and correlation 0.05 seeds 0 and 1 leave 3 or 4
# of 130 rows, seeds 1 and 3 leave 6 or 9 of 257 rows with a competitor inside the undecided band
OTHER_SEEDS = {(130, 64, 0.05): (2, 3, 5), (257, 64, 0.05): (0, 2, 4)}
UNDECIDED_CAP = 0.02                          # of a case's rows, at least one row; and of all rows pooled


def random_cases():
    """(n, E, corr, seed).  E >= 512 at correlation 0.05 is left out: 10 to 43 % of such rows have a competitor inside the undecided
    band, an interval test of them would assert little.  The planted cases cover high ranks at large n."""
    return [(n, E, corr, seed) for n in RANDOM_N for E in RANDOM_E for corr in CORRS if not (E >= 512 and corr < 0.1)
            for seed in OTHER_SEEDS.get((n, E, corr), SEEDS)]


def make_square(n, E, corr, seed):
    """the twin of recall_cases.make_case with one caption per image and a correlation to choose -> img, txt f32 [n, E] (CPU tensors)"""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * n + E + int(1000 * corr))
    img = torch.randn(n, E, generator=g) * (0.5 + torch.rand(n, 1, generator=g))
    txt = 3 * (corr * img + torch.randn(n, E, generator=g))
    return img, txt


def rank_intervals(L, b):
    """float64 logits [n, n] -> (lo, hi): per row the competitors decided ahead of the diagonal, and those plus the undecided ones
    (within 2 b: both sides carry up to b)"""
    n = L.shape[0]
    d = np.diagonal(L)[:, None]
    off = ~np.eye(n, dtype=bool)
    lo = ((L > d + 2 * b) & off).sum(axis=1)
    hi = lo + ((np.abs(L - d) <= 2 * b) & off).sum(axis=1)
    return lo, hi


def scores64(L):
    """float64 logits -> (sexp [n] = sum_j exp(L_ij - 1), softmax diagonal terms [n], diagonal [n])"""
    d = np.diagonal(L).copy()
    sexp = np.exp(L - 1.0).sum(axis=1)
    return sexp, np.exp(d - 1.0) / sexp, d


@functools.lru_cache(maxsize=None)
def reference(n, E, corr, seed):
    """the case, its float64 logits and rank intervals, computed once per session and left unchanged"""
    img, txt = make_square(n, E, corr, seed)
    L = rc.cos64(img, txt)
    return img, txt, L, rank_intervals(L, rc.bound(E))


def unit_rows64(x):
    x = x.double().numpy()
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---- 5. scales -------------------------------------------------------------------------------------------------------------------------
def power_of_two_scales(x, seed):
    """x f32 [n, E] -> x with every row times its own power of two in 2^-30 .. 2^30.  Powers of two commute with every rounding of the
    kernel as long as nothing leaves the normal range of f32: the squares, their sum, its root and the reciprocal only change exponent.
    That is asserted here: every non-zero element's square and every squared norm, scaled or not, lies within [2^-126, 2^127]."""
    n = x.shape[0]
    k = torch.randint(-30, 31, (n, 1), generator=torch.Generator().manual_seed(seed))
    k[0], k[-1] = 30, -30
    y = x * torch.pow(torch.tensor(2.0), k)
    for t in (x, y):
        sq = t.double() ** 2
        nz = sq[sq > 0]
        assert nz.min() >= 2.0 ** -126 and sq.sum(dim=1).max() <= 2.0 ** 127 and sq.sum(dim=1).min() >= 2.0 ** -126
    assert torch.equal(y * torch.pow(torch.tensor(2.0), -k), x)                # nothing was rounded
    return y
