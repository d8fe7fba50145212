"""Cases, the float64 reference and the checker shared by tests/test_topk_cpu.py and tests/test_topk_gpu.py (top-K search over
embeddings: include/dclip.h dclip_topk_search, dclip_group_mean_rows).  Not a test module.

The error bound of one logit is recall_cases.bound: b(E) = (2 E + 8) 2^-24 (the search uses the same normaliser
and the same tile routine as the recall kernels).  With it, against the float64 logits L of a row and their k-th best value t:
  every returned score is within b of the L of its index;
  an index with L > t + 2 b must be returned: its f32 logit is above t + b, while at most k - 1 indices have L > t, so fewer than k
    indices can have an f32 logit at or above it;
  an index with L < t - 2 b must not be returned: its f32 logit is below t - b, and the k indices with L >= t all have f32 logits above.
The order of the kernel's own output is checked exactly."""
import functools

import numpy as np
import torch

from recall_cases import U, bound, cos64          # noqa: F401  (one definition of the bound and of the float64 cosine)

SEEDS = (0, 1, 2)
# (nq, ng, k, E): every nq of {1, 15, 16, 17, 33, 70}, every ng of {1, 15, 16, 17, 63, 64, 65, 127, 257, 1000, 4099} (the 16-column
# tile edge, fewer tiles than waves, one tile per wave and one more, more tiles than list entries), every k of {1, 2, 5, 10, 16, 17, 63,
# 64}, every E of {16, 64, 512, 768}, k == ng and k > ng
CASES = [
    (1, 1, 1, 16), (1, 15, 5, 16), (15, 16, 16, 64), (16, 17, 17, 64), (17, 63, 63, 64), (33, 64, 64, 64), (70, 65, 64, 512),
    (16, 127, 10, 768), (17, 257, 2, 64), (33, 1000, 64, 64), (70, 4099, 10, 512), (15, 4099, 64, 64), (1, 1000, 17, 768),
    (16, 1, 1, 16), (33, 257, 63, 16), (70, 127, 16, 64),
    (17, 15, 16, 64), (33, 1, 5, 64), (16, 63, 64, 16), (70, 17, 64, 64), (1, 16, 17, 512),       # k > ng
]


def make_case(nq, ng, E, seed):
    """-> queries f32 [nq, E], gallery f32 [ng, E] (CPU tensors), un-normalised: rows of different lengths, the gallery loosely
    gathered around a few directions so that the best logits of a row lie close together"""
    g = torch.Generator().manual_seed(7919 * seed + 104729 * nq + 1299709 * ng + E)
    centres = torch.randn(5, E, generator=g)
    q = (centres[torch.randint(0, 5, (nq,), generator=g)] + torch.randn(nq, E, generator=g)) * (0.5 + 3 * torch.rand(nq, 1, generator=g))
    gal = (0.5 * centres[torch.randint(0, 5, (ng,), generator=g)] + torch.randn(ng, E, generator=g)) * (0.25 + torch.rand(ng, 1, generator=g))
    return q, gal


def order64(L):
    """float64 logits [nq, ng] -> every row's gallery indices in the order (L descending, index ascending)"""
    return np.argsort(-L, axis=1, kind='stable')


def brute_order(L):
    """the same by an explicit sort of (-L, index) pairs"""
    return np.array([[j for _, j in sorted((-float(v), j) for j, v in enumerate(row))] for row in L], dtype=np.int64).reshape(L.shape)


@functools.lru_cache(maxsize=None)
def reference(nq, ng, E, seed):
    """the case, its float64 logits and their order, computed once per session"""
    q, gal = make_case(nq, ng, E, seed)
    L = cos64(q, gal)
    return q, gal, L, order64(L)


def check_order(idx, score, ng):
    """exact, on the kernel's own output: scores non-increasing, equal scores with ascending indices, indices distinct and in [0, ng),
    and past the gallery's end idx -1 with score -inf"""
    nq, k = idx.shape
    m = min(k, ng)
    assert idx.dtype == np.int32 and (score is None or score.dtype == np.float32)
    assert (idx[:, m:] == -1).all(), 'entries past the gallery are idx -1'
    head = idx[:, :m]
    assert (head >= 0).all() and (head < ng).all(), 'index out of range'
    srt = np.sort(head, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), 'an index occurs twice in a row'
    if score is None:
        return
    assert np.isneginf(score[:, m:]).all(), 'entries past the gallery are score -inf'
    s = score[:, :m]
    assert np.isfinite(s).all()
    assert (s[:, 1:] <= s[:, :-1]).all(), 'scores increase'
    tie = s[:, 1:] == s[:, :-1]
    assert (head[:, 1:][tie] > head[:, :-1][tie]).all(), 'equal scores out of index order'


def check_against_float64(idx, score, L, k, E):
    """the three interval checks of every row, none left out; -> (rows whose index list differs from the float64 order's, the largest
    |score - L|) for the record"""
    nq, ng = L.shape
    b = bound(E)
    m = min(k, ng)
    check_order(idx, score, ng)
    head = idx[:, :m].astype(np.int64)
    Lh = np.take_along_axis(L, head, axis=1)
    err = np.abs(score[:, :m].astype(np.float64) - Lh)
    assert (err <= b).all(), ('score off by more than b(E)', float(err.max()), b)
    kth = np.sort(L, axis=1)[:, ng - m][:, None]                               # the float64 m-th best of every row
    present = np.zeros(L.shape, dtype=bool)
    np.put_along_axis(present, head, True, axis=1)
    missing = (L > kth + 2 * b) & ~present
    assert not missing.any(), ('an index clearly among the k best is missing', np.argwhere(missing)[:4])
    intruder = Lh < kth - 2 * b
    assert not intruder.any(), ('an index clearly outside the k best was returned', np.argwhere(intruder)[:4])
    differ = int((head != order64(L)[:, :m]).any(axis=1).sum())
    return differ, float(err.max()) if err.size else 0.0


# ---- planted logits ---------------------------------------------------------------------------------------------------------------
PLANTED_E = 64


def planted_case(nq=40, ng=300, seed=3):
    """Cosines that f32 represents and computes exactly.  A query is a signed, scaled one-hot row s 2^p e_a.  A gallery row has 0, 1, 4
    or 16 entries of +-2^p: norm 0, 2^p, 2^(p + 1) or 2^(p + 2), squared norms, roots, reciprocals and products all powers of two.
    cos = s sign(g[a]) / (1, 2 or 4), or 0: in quarters, v = 4 cos in {0, +-1, +-2, +-4}; few distinct values, so most of a row ties.
    -> queries, gallery, v int64 [nq, ng]"""
    rng = np.random.RandomState(seed)
    q = np.zeros((nq, PLANTED_E), dtype=np.float32)
    gal = np.zeros((ng, PLANTED_E), dtype=np.float32)
    a = rng.randint(0, 16, size=nq)                                            # the few-hot entries live in the same 16 columns
    sq = rng.choice([-1, 1], size=nq)
    q[np.arange(nq), a] = sq * 2.0 ** rng.randint(-3, 4, size=nq)
    sign = np.zeros((ng, PLANTED_E), dtype=np.int64)
    quarter = np.zeros(ng, dtype=np.int64)                                     # 4 / (norm / 2^p)
    for j in range(ng):
        nnz = (0, 1, 4, 16)[rng.randint(0, 4)]
        cols = rng.choice(16, size=nnz, replace=False)
        sign[j, cols] = rng.choice([-1, 1], size=nnz)
        quarter[j] = {0: 0, 1: 4, 4: 2, 16: 1}[nnz]
        gal[j] = sign[j] * 2.0 ** rng.randint(-3, 4)
    v = sq[:, None] * sign[:, a].T * quarter[None, :]
    return torch.from_numpy(q), torch.from_numpy(gal), v


def planted_answer(v, k):
    """-> idx int32 [nq, k], score f32 [nq, k] from the integers: order (v descending, index ascending), score v / 4"""
    nq, ng = v.shape
    order = np.argsort(-v, axis=1, kind='stable')[:, :k]
    idx = np.full((nq, k), -1, dtype=np.int32)
    score = np.full((nq, k), -np.inf, dtype=np.float32)
    idx[:, :order.shape[1]] = order
    score[:, :order.shape[1]] = np.take_along_axis(v, order, axis=1) / 4.0
    return idx, score


# ---- group means ------------------------------------------------------------------------------------------------------------------
def group_mean_bound(E, n):
    """|out - float64| of one element of a group of n rows, from the chain (u = 2^-24, every normalised element at most 1 in size):
      normalise: the squared norm is a sum of non-negative products, each lane's chain 4 roundings deep per 256 columns, the wave sum
        6 more: off by at most (4 ceil(E / 256) + 6) u relative; the root halves that; the correctly rounded root, the reciprocal and the
        product add one u each: (2 ceil(E / 256) + 6) u on an element;
      n adds in index order: add j rounds a partial sum of size at most j: (1 + 2 + .. + n) u before, at most (n + 1) / 2 u after the
        division by n;
      the rounded 1 / n and the product with it: 2 u;
      second-order terms: 1 u."""
    return (2 * -(-E // 256) + 6 + (n + 1) / 2 + 2 + 1) * U


def group_mean64(rows, counts):
    """float64: the mean of x / |x| per group, a zero row adding nothing, an empty group giving the zero row"""
    x = rows.double().numpy()
    norm = np.linalg.norm(x, axis=1, keepdims=True)
    xn = np.where(norm > 0, x / np.where(norm > 0, norm, 1.0), 0.0)
    offs = np.concatenate([[0], np.cumsum(counts)])
    return np.stack([xn[a:b].sum(axis=0) / max(b - a, 1) for a, b in zip(offs, offs[1:])])
