"""The validation-metrics kernel (dclip_retrieval_metrics, metrics.retrieval_metrics), the parts that need no GPU: the conditions that
the builders of tests/metrics_cases.py state (planted ranks equal the float64 count with a gap no rounding reaches, every rank and every
column tile is covered, the ties case has the closed-form ranks, few random rows have an undecided competitor, the power-of-two scales
round nothing), the workspace layout against the query, and the entry's refusals on the host."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_cases as mc
import recall_cases as rc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. planted ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E', mc.PLANTED_SIZES)
def test_planted_square_gives_the_planned_ranks(n, E):
    rows, cols, r, chosen, swapped = mc.planted_square(n, E)
    assert rows.shape == cols.shape == (n, E) and rows.dtype == cols.dtype == torch.float32
    assert sorted(r.tolist()) == list(range(n))                              # every rank occurs, n - 1 included
    assert (chosen.sum(axis=1) == r).all() and not chosen[np.arange(n), np.arange(n)].any()
    L = rc.cos64(rows, cols)
    assert np.abs(L - mc.planted_logits(r, chosen)).max() <= 4 * np.finfo(np.float64).eps      # the closed form
    off = ~np.eye(n, dtype=bool)
    d = np.diagonal(L)[:, None]
    assert (((L > d) & off).sum(axis=1) == r).all()                          # planned ranks equal the float64 count
    gap = np.abs(L - d)[off].min() if n > 1 else np.inf
    assert gap > 2 * rc.bound(E), (gap, 2 * rc.bound(E))                     # every competitor is more than 2 b(E) from the diagonal
    lo, hi = mc.rank_intervals(L, rc.bound(E))
    assert (lo == hi).all() and (lo == r).all()
    # swapped roles: the closed form equals the float64 count, with a gap beyond the planted logits' own error of 4 u relative
    Ls = rc.cos64(cols, rows)
    ds = np.diagonal(Ls)[:, None]
    assert (((Ls > ds) & off).sum(axis=1) == swapped).all()
    if n > 1:
        assert (np.abs(Ls - ds) - 2 * mc.PLANTED_LOGIT_REL * np.maximum(np.abs(Ls), np.abs(ds)))[off].min() > 0
    if n >= 63:
        assert swapped.max() > n // 4 and (swapped == 0).any()
    # the cut-off lists: nk = 6, 8 and 0; the second holds a cut-off above n, n itself, repeats, and is unsorted
    lists = mc.k_lists(n)
    assert [len(k) for k in lists] == [6, 8, 0] and 1000 > n and lists[1].count(1) >= 2 and list(lists[1]) != sorted(lists[1])
    acc = mc.expected_acc(r, lists[1])
    assert acc.dtype == np.float32 and acc[3] == 1.0 and acc[4] == 1.0 and acc[1] == acc[2] == np.float32(1) / np.float32(n)
    if n > 1:
        assert acc[5] == np.float32(n - 1) / np.float32(n) < 1.0             # rank n - 1 misses the cut-off n - 1


@pytest.mark.parametrize('n,E', [(n, E) for n, E in mc.PLANTED_SIZES if n > 64])
def test_planted_low_rank_rows_visit_every_column_tile(n, E):
    """a column tile that any one wave skipped would change the rank of a row of rank <= LOW_RANK: together these rows have a chosen
    column in every tile, hence in every residue of the tile index mod 4; and every 16-row panel has a row with a chosen column in
    every tile (but for a last panel of one row, whose own tile holds nothing but its diagonal), so a tile skipped by one workgroup alone shows too"""
    _, _, r, chosen, _ = mc.planted_square(n, E)
    nt = mc.ntile(n)
    tile_of = np.arange(n) // 16
    low = (r >= 1) & (r <= mc.LOW_RANK)
    assert low.sum() == mc.LOW_RANK
    hit = {int(t) for t in tile_of[chosen[low].any(axis=0)]}
    assert hit == set(range(nt)) and {t % 4 for t in hit} == {0, 1, 2, 3}
    for p in range(nt):
        panel = chosen[16 * p:16 * p + 16].any(axis=0)
        alone = {p} if n - 16 * p == 1 else set()                               # a panel of one row whose tile holds its diagonal only
        assert {int(t) for t in tile_of[panel]} == set(range(nt)) - alone, p
    assert (n, nt) != (257, 17) or len(range(0, nt, 4)) == 5                  # wave 0 walks five tiles


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n0,E', mc.TIE_SIZES)
def test_tied_square_has_the_closed_form_ranks(n0, E):
    rows, cols, want = mc.tied_square(n0, E)
    n = 2 * n0
    assert rows.shape == cols.shape == (n, E) and n <= 272
    assert torch.equal(rows[:n0], rows[n0:]) and torch.equal(cols[:n0], cols[n0:])       # bit copies
    L = rc.cos64(rows, cols)
    d = np.diagonal(L)[:, None]
    off = ~np.eye(n, dtype=bool)
    assert (((L > d) & off).sum(axis=1) == want).all()                      # strictly ahead: 2 r
    assert (((L == d) & off).sum(axis=1) == 1).all()                        # and exactly one tie per row, which >= would count
    assert (want % 2 == 0).all() and want.max() == 2 * (n0 - 1) and (want == 0).sum() == 2


# ---- 3. random operands --------------------------------------------------------------------------------------------------------------
def test_random_case_list():
    cases = mc.random_cases()
    assert len(cases) == len(set(cases)) == 12 * (4 * 2 - 2) * 3
    assert {c[0] for c in cases} == {1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 130, 257} and {c[1] for c in cases} == {16, 64, 512, 1024}
    assert all(n <= 272 and E <= 1024 for n, E, _, _ in cases)
    assert not any(E >= 512 and corr == 0.05 for _, E, corr, _ in cases)
    for n, E in ((257, 16), (130, 64), (257, 1024)):
        assert sum(1 for c in cases if c[:2] == (n, E)) in (3, 6)


def test_few_rows_have_an_undecided_competitor():
    """conditions of the GPU interval test, from float64 alone: per case at most max(1, 2 % of n) rows have an undecided competitor,
    pooled over the list at most 2 %; one correlation leaves most ranks 0, the other spreads them"""
    rows = undecided = 0
    zero = {c: [0, 0] for c in mc.CORRS}
    top = 0
    for n, E, corr, seed in mc.random_cases():
        img, txt, L, (lo, hi) = mc.reference(n, E, corr, seed)
        assert img.shape == txt.shape == (n, E) and L.shape == (n, n)
        und = int((hi > lo).sum())
        assert und <= max(1, int(mc.UNDECIDED_CAP * n)), (n, E, corr, seed, und)
        assert (lo >= 0).all() and (hi <= n - 1).all()
        rows, undecided = rows + n, undecided + und
        if n >= 63:
            zero[corr][0] += int((hi == 0).sum())
            zero[corr][1] += n
        top = max(top, int(lo.max()))
    assert undecided <= mc.UNDECIDED_CAP * rows, (undecided, rows)
    assert zero[0.25][0] > 0.5 * zero[0.25][1] and zero[0.05][0] < 0.5 * zero[0.05][1], zero
    assert top > 200                                                         # high ranks occur among the random cases too


def test_power_of_two_scales_round_nothing():
    for n, E, corr, seed in ((33, 64, 0.05, 0), (130, 512, 0.25, 1)):
        img, txt, _, _ = mc.reference(n, E, corr, seed)
        a, b = mc.power_of_two_scales(img, 11), mc.power_of_two_scales(txt, 12)          # the builder asserts its own conditions
        ratio = (a / img)[:, 0].abs().log2()
        assert ratio.max() == 30 and ratio.min() == -30 and torch.equal(ratio, ratio.round())
        assert np.array_equal(rc.cos64(a, b), rc.cos64(img, txt)) or np.abs(rc.cos64(a, b) - rc.cos64(img, txt)).max() < 1e-15


# ---- 4. bounds and the workspace layout ------------------------------------------------------------------------------------------------
def test_bounds():
    assert mc.U == 2.0 ** -24 and rc.bound(512) == 1032 * mc.U
    assert mc.sexp_terms(257, 512) == np.expm1(1032 * mc.U) + (5 + 6) * mc.U and mc.sexp_terms(16, 16, 0.0) == 7 * mc.U
    assert (40 + 1 + 6) * mc.U < mc.sexp_terms(64, 16) < (40 + 1 + 6 + 0.001) * mc.U
    assert mc.finalize_factor(256) == 13 * mc.U and mc.finalize_factor(257) == 14 * mc.U
    m = mc.EXP_REL / mc.U
    assert m >= 1 and m == 2 ** round(np.log2(m))                           # a power of two times u


@pytest.mark.parametrize('n,E', [(1, 16), (15, 16), (64, 64), (65, 80), (257, 272), (257, 1024), (5000, 512)])
def test_workspace_layout_matches_the_query(n, E):
    pieces, total = mc.workspace_layout(n, E, _lib().dclip_retrieval_metrics_workspace(n, E))
    assert list(pieces) == ['nimg', 'ntxt', 'rank', 'sexp', 'diag']
    end = 0
    for off, live, _, shape in pieces.values():
        assert off % 256 == 0 and off >= end and live == 4 * int(np.prod(shape))
        end = off + live
    assert end <= total and total % 256 == 0
    with pytest.raises(AssertionError, match='layout of metrics.hip changed'):
        mc.workspace_layout(n, E, total + 256)


def test_workspace_query_of_a_refused_shape_is_zero():
    q = _lib().dclip_retrieval_metrics_workspace
    assert q(0, 64) == 0 and q(-1, 64) == 0 and q(5, 0) == 0 and q(5, -16) == 0 and q(1, 16) > 0


# ---- 5. host refusals ----------------------------------------------------------------------------------------------------------------
# dummy non-null, 16-byte aligned addresses: never dereferenced, every call below is refused before a launch
IMG, TXT, OUT, RANK, WS = 4096, 8192, 16384, 20480, 1 << 20
REFUSALS = [
    (dict(img=None), 'null'), (dict(txt=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'),
    (dict(n=0), '0 < n'), (dict(E=0), 'multiple of 16'), (dict(E=8), 'multiple of 16'), (dict(E=24), 'multiple of 16'),
    (dict(nk=-1), 'cut-offs'), (dict(nk=9), 'cut-offs'), (dict(nk=2, ks=None), 'cut-offs'),
    (dict(ws_short=1), 'workspace too small'),
    (dict(img_skew=4), '16-byte aligned'), (dict(txt_skew=4), '16-byte aligned'), (dict(ws_skew=4), '16-byte aligned'),
]
REFUSAL_IDS = ['-'.join(f'{a}={b}' for a, b in kw.items()) for kw, _ in REFUSALS]


@pytest.mark.parametrize('kw,word', REFUSALS, ids=REFUSAL_IDS)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    l = _lib()
    g = lambda name, default: kw[name] if name in kw else default
    n, E, nk = g('n', 5), g('E', 64), g('nk', 3)
    ks = (ctypes.c_int32 * 16)(*range(1, 17))
    ws_bytes = max(l.dclip_retrieval_metrics_workspace(5, 64), l.dclip_retrieval_metrics_workspace(max(n, 1), max(E, 16))) - g('ws_short', 0)
    rc_ = l._dll.dclip_retrieval_metrics(g('img', IMG + g('img_skew', 0)), g('txt', TXT + g('txt_skew', 0)), n, E, g('ks', ks), nk,
                                         g('out', OUT), RANK, g('ws', WS + g('ws_skew', 0)), ws_bytes, None)
    assert rc_ != 0 and word in l._dll.dclip_last_error_string().decode()
    assert 'dclip_retrieval_metrics' in l._dll.dclip_last_error_string().decode()
