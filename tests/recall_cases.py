"""Cases and float64 references shared by tests/test_recall_cpu.py and tests/test_recall_gpu.py (Recall@K with several captions per
image: include/dclip.h dclip_retrieval_recall).  Not a test module.

Error bound of one logit, derived, not measured.  The inputs are f32, hence exact in float64; u = 2^-24.
  normalisation: the squared norm is a sum of E non-negative products, off by at most E u relative in any summation order; its square
    root halves that, the correctly rounded sqrt, the reciprocal and the product x_k * inv add one u each: every element of a normalised
    row is x_k / |x| (1 + d), |d| <= (E / 2 + 3) u;
  dot product: the MFMA is an fmaf chain of length E, off by at most E u sum_k |a_k b_k| <= E u |a| |b| (Cauchy-Schwarz), the
    normalised rows having norms 1 + O(E u);
  together |L - L64| <= (E + 6) u + E u, second-order terms (below (2 E u)^2 = 4e-9 at E = 512) covered by two more u:
      b(E) = (2 E + 8) u
which is dclip_clipscore's bound and smaller than the stand-in (3 E + 16) u the cap of 2 % undecided rows was first checked with.
A competitor is undecided when |L64[competitor] - L64[target]| <= 2 b: both sides carry up to b."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
COUNT_CYCLE = (5, 1, 7, 0, 3, 40)             # an empty group, a group longer than two tiles, groups across every tile border
SHAPES = [(1, 16), (15, 16), (16, 64), (17, 64), (33, 64), (70, 512), (130, 64), (130, 512)]      # (n_img, E)
SEEDS = (0, 1, 2)
UNDECIDED_CAP = 0.02                          # of the ranked rows of a case


def bound(E):
    return (2 * E + 8) * U


def cycle_counts(n_img):
    return [5] if n_img == 1 else [COUNT_CYCLE[i % len(COUNT_CYCLE)] for i in range(n_img)]


def owners(counts):
    return np.repeat(np.arange(len(counts)), counts)


def make_case(n_img, E, seed):
    """-> img f32 [n_img, E], txt f32 [n_txt, E] (CPU tensors), counts"""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * n_img + E)
    counts = cycle_counts(n_img)
    own = torch.from_numpy(owners(counts))
    img = torch.randn(n_img, E, generator=g) * (0.5 + torch.rand(n_img, 1, generator=g))
    txt = 3 * (0.25 * img[own] + torch.randn(len(own), E, generator=g))
    return img, txt, counts


def cos64(img, txt):
    """[n_img, n_txt] cosine in float64, 0 where a norm is 0"""
    a, b = img.double().numpy(), txt.double().numpy()
    den = np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :]
    return np.where(den > 0, (a @ b.T) / np.where(den > 0, den, 1.0), 0.0)


def intervals(L, counts, b):
    """float64 logits L [n_img, n_txt] -> (lo_i, hi_i, lo_t, hi_t): per image / per caption the number of decided-greater competitors
    and that plus the undecided ones; -1 / -1 for an image without captions.  Image -> text: the target is the float64 best own
    caption; own captions never compete."""
    n_img, n_txt = L.shape
    own = owners(counts)
    mine = own[None, :] == np.arange(n_img)[:, None]                           # [n_img, n_txt]
    has = np.asarray(counts) > 0
    target_i = np.where(mine, L, -np.inf).max(axis=1, initial=-np.inf)        # [n_img]
    t = np.where(has, target_i, 0.0)[:, None]
    lo_i = ((L > t + 2 * b) & ~mine).sum(axis=1)
    hi_i = lo_i + ((np.abs(L - t) <= 2 * b) & ~mine).sum(axis=1)
    lo_i, hi_i = np.where(has, lo_i, -1), np.where(has, hi_i, -1)
    target_t = L[own, np.arange(n_txt)][None, :]                               # [1, n_txt]
    lo_t = ((L > target_t + 2 * b) & ~mine).sum(axis=0)
    hi_t = lo_t + ((np.abs(L - target_t) <= 2 * b) & ~mine).sum(axis=0)
    return lo_i, hi_i, lo_t, hi_t


@functools.lru_cache(maxsize=None)
def reference(n_img, E, seed):
    """the case and its float64 intervals, computed once per session"""
    img, txt, counts = make_case(n_img, E, seed)
    return img, txt, counts, intervals(cos64(img, txt), counts, bound(E))


def undecided_fraction(iv):
    lo_i, hi_i, lo_t, hi_t = iv
    ranked = int((lo_i >= 0).sum()) + len(lo_t)
    return (int((hi_i > lo_i).sum()) + int((hi_t > lo_t).sum())) / ranked, ranked


def expected_out(rank_i, rank_t, ks):
    """out of dclip_retrieval_recall from its own ranks: integer hits over the ranked rows, one division in double, one cast"""
    res = []
    for r in (np.asarray(rank_i), np.asarray(rank_t)):
        r = r[r >= 0]
        res.append([np.float32(np.float64(int((r < k).sum())) / np.float64(len(r))) for k in ks])
    for r in (np.asarray(rank_i), np.asarray(rank_t)):
        r = r[r >= 0]
        res.append([np.float32(np.float64(int(r.astype(np.int64).sum())) / np.float64(len(r)))])
    return np.array([x for part in res for x in part], dtype=np.float32)


# ---- planted ranks ---------------------------------------------------------------------------------------------------------------
PLANTED_E = 64


def planted_case(n_img=40, seed=5):
    """images are one-hot e_i; caption c of image i with planned rank r_c is e_i + 2 sum of e_j over r_c chosen other images j:
    cos(img_j, c) = 2 / sqrt(1 + 4 r_c) for the chosen j, 1 / sqrt(1 + 4 r_c) for the owner, 0 elsewhere, so rank_t2i[c] = r_c.
    Image -> text: caption c' (r' = r_c') of another image beats image i's best own caption (the smallest r among its own) iff i is
    chosen in c' and 2 / sqrt(1 + 4 r') > 1 / sqrt(1 + 4 r)  <=>  1 + 4 r' < 4 (1 + 4 r): integers, never equal (1 against 0 mod 4).
    -> img, txt, counts, rank_i2t, rank_t2i (the planned integer ranks)"""
    rng = np.random.RandomState(seed)
    counts = [(2, 1, 3, 0, 4)[i % 5] for i in range(n_img)]
    own = owners(counts)
    n_txt = len(own)
    img = np.zeros((n_img, PLANTED_E), dtype=np.float32)
    img[np.arange(n_img), np.arange(n_img)] = 1.0
    txt = np.zeros((n_txt, PLANTED_E), dtype=np.float32)
    r_c = rng.randint(0, n_img, size=n_txt)                                     # 0 .. n_img - 1 other images
    r_c[::7] = 0
    chosen = np.zeros((n_txt, n_img), dtype=bool)
    for c in range(n_txt):
        others = np.array([j for j in range(n_img) if j != own[c]])
        chosen[c, rng.choice(others, size=r_c[c], replace=False)] = True
        txt[c, own[c]] = 1.0
        txt[c, :n_img][chosen[c]] = 2.0
    rank_i = np.full(n_img, -1, dtype=np.int64)
    for i in range(n_img):
        if counts[i]:
            r = int(r_c[own == i].min())
            rank_i[i] = sum(1 for c in range(n_txt) if own[c] != i and chosen[c, i] and 1 + 4 * int(r_c[c]) < 4 * (1 + 4 * r))
    return torch.from_numpy(img), torch.from_numpy(txt), counts, rank_i, r_c.astype(np.int64)
