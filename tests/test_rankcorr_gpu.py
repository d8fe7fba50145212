"""Spearman and Pearson against human ratings on the GPU (dclip_rank_correlation, metrics.rank_correlation, HumanCorrelation).  Every
twice-rank of every vector and the four integers per column are compared for EQUALITY with the integer reference of
tests/rankcorr_cases.py, rho with the reference expression and scipy.stats.spearmanr within 1e-14, r with the exact reference within
the bound derived there from the kernel's summation shape and with scipy.stats.pearsonr within 1e-12.  Invariances are exact on the
integers and bit-equal on rho; on r they are bit-equal where the arithmetic is the same (x -> 2 x, x -> -x) and within the bound under a
permutation, which changes which items share a lane: bits need not survive it.  Every raw call runs on guarded buffers: the inputs sit
16 bytes into NaN-filled buffers with ld > n, the outputs between sentinels, the workspace is exactly as large as the query says and is
followed by a patterned guard.  tests/test_rankcorr_cpu.py checks the reference itself against SciPy."""
import numpy as np
import pytest
import torch

import rankcorr_cases as rc

pytestmark = pytest.mark.gpu

PAD, SENT = 64, -777
WORST = {'ratio': 0.0}                                             # the largest |r - exact| / bound seen so far in this session


def raw(x, y, extra_ld=3, sums=True, ranks=True):
    """x [C, n], y [n] (numpy f32) -> corr float64 [C, 2], sums int64 [C, 4] or None, ranks int32 [C + 1, n] or None, from one guarded
    call of the C entry"""
    from distillclip_amd._lib import lib
    x, y = np.atleast_2d(np.asarray(x, dtype=np.float32)), np.asarray(y, dtype=np.float32)
    C, n = x.shape
    ld = n + extra_ld
    xb = np.full(4 + C * ld + 4, np.nan, dtype=np.float32)
    for c in range(C):
        xb[4 + c * ld:4 + c * ld + n] = x[c]
    yb = np.full(4 + n + 4, np.nan, dtype=np.float32)
    yb[4:4 + n] = y
    d_x, d_y = torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda()
    corr = torch.full((2 * PAD + 2 * C,), float(SENT), dtype=torch.float64, device='cuda')
    sm = torch.full((2 * PAD + 4 * C,), SENT, dtype=torch.int64, device='cuda')
    rk = torch.full((2 * PAD + (C + 1) * n,), SENT, dtype=torch.int32, device='cuda')
    need = lib().dclip_rank_correlation_workspace(n, C)
    assert need > 0 and need % 16 == 0
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device='cuda')
    lib().dclip_rank_correlation(d_x.data_ptr() + 16, ld, C, d_y.data_ptr() + 16, n, corr.data_ptr() + 8 * PAD,
                                 sm.data_ptr() + 8 * PAD if sums else None, rk.data_ptr() + 4 * PAD if ranks else None,
                                 ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    corr, sm, rk = corr.cpu().numpy(), sm.cpu().numpy(), rk.cpu().numpy()
    for buf, m in ((corr, 2 * C), (sm, 4 * C if sums else 0), (rk, (C + 1) * n if ranks else 0)):
        assert (buf[:PAD] == SENT).all() and (buf[PAD + m:] == SENT).all()               # nothing outside the outputs, nothing in an absent one
    assert (ws[need:] == 0xA5).all()                                                      # nothing past the workspace
    assert np.array_equal(d_x.cpu().numpy(), xb, equal_nan=True) and np.array_equal(d_y.cpu().numpy(), yb, equal_nan=True)
    return (corr[PAD:PAD + 2 * C].reshape(C, 2).copy(), sm[PAD:PAD + 4 * C].reshape(C, 4).copy() if sums else None,
            rk[PAD:PAD + (C + 1) * n].reshape(C + 1, n).copy() if ranks else None)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check_against(x, y, ref, what='', scipy=True):
    """the guarded call, with and without the optional outputs, against the reference -> corr, sums, ranks"""
    x = np.atleast_2d(x)
    n = x.shape[1]
    corr, sums, ranks = raw(x, y)
    assert np.array_equal(ranks, ref['ranks']), (what, np.argwhere(ranks != ref['ranks'])[:8].tolist())
    assert np.array_equal(sums, ref['sums']), (what, sums.tolist(), ref['sums'].tolist())
    clean = ~np.isnan(np.vstack([x, y[None, :]])).any(axis=1)
    assert (ranks[clean].sum(axis=1, dtype=np.int64) == n * (n + 1)).all(), what
    assert rc.close(corr[:, 0], ref['rho'], rc.RHO_TOL), (what, corr[:, 0], ref['rho'])
    err = np.abs(corr[:, 1] - ref['r'])
    finite = ~np.isnan(ref['r'])
    if finite.any():
        ratio = float((err[finite] / ref['bound'][finite]).max())
        WORST['ratio'] = max(WORST['ratio'], ratio)
        print(f'{what}: worst |r - exact| {err[finite].max():.3e}, worst error / bound {ratio:.3f} (session worst {WORST["ratio"]:.3f})')
    assert rc.close(corr[:, 1], ref['r'], np.nan_to_num(ref['bound'])), (what, corr[:, 1], ref['r'], ref['bound'])
    if scipy:
        sp_rho, sp_r = rc.scipy_reference(x, y)
        assert rc.close(corr[:, 0], sp_rho, rc.RHO_TOL), (what, corr[:, 0], sp_rho)
        assert rc.close(corr[:, 1], sp_r, rc.SCIPY_R_TOL), (what, corr[:, 1], sp_r)
    bare, no_sums, no_ranks = raw(x, y, sums=False, ranks=False)                          # the twice-ranks go through the workspace
    assert no_sums is None and no_ranks is None and same_bits(bare, corr), what
    return corr, sums, ranks


def check(x, y, what='', scipy=True):
    return check_against(x, y, rc.reference(x, y), what, scipy)


# ---- 1. the case families at every size ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', rc.SEEDS)
@pytest.mark.parametrize('n', rc.SIZES)
def test_ranks_and_sums_equal_the_integer_reference(n, seed):
    for family in rc.ALL_FAMILIES:
        x, y, ref = rc.case_with_reference(family, n, seed)
        corr, sums, ranks = check_against(x, y, ref, f'{family} n={n} seed={seed} C={x.shape[0]}')
        assert (sums[:, 2] == sums[0, 2]).all() and (sums[:, 3] == 0).all()               # Syy is the same for every column
        assert (np.abs(corr[~np.isnan(corr)]) <= 1).all()


# ---- 2. exact structure --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (65, 257, 1000))
def test_identity_reversal_and_constant_vectors(n):
    r = np.random.RandomState(n)
    v = ((r.permutation(n) - n // 2) / 8.0).astype(np.float32)                           # n distinct values
    y = r.randint(1, 5, size=n).astype(np.float32)
    S = n * (n * n - 1) // 3
    # x = y: rho exactly 1, with and without ties
    corr, sums, ranks = check(v, v, 'x = y')
    assert sums[0].tolist() == [S, S, S, 0] and corr[0, 0] == 1.0 and corr[0, 1] == 1.0
    assert np.array_equal(np.sort(ranks[0]), 2 * np.arange(1, n + 1))
    corr, sums, _ = check(y, y, 'x = y with ties')
    assert sums[0, 0] == sums[0, 1] == sums[0, 2] < S and corr[0, 0] == 1.0
    # the ratings reversed: exactly -1, and every column's rho negated
    corr, sums, _ = check(-v, v, 'x = -y')
    assert sums[0].tolist() == [-S, S, S, 0] and corr[0, 0] == -1.0
    corr, sums, _ = check(-y, y, 'x = -y with ties')
    assert -sums[0, 0] == sums[0, 1] == sums[0, 2] and corr[0, 0] == -1.0
    x = np.stack([v + y, r.randn(n).astype(np.float32)])
    fwd, fs, _ = check(x, y, 'forward')
    rev, rs, _ = check(x, -y, 'y reversed')
    assert np.array_equal(rs[:, 0], -fs[:, 0]) and np.array_equal(rs[:, 1:], fs[:, 1:]) and np.array_equal(rev, -fwd)
    # constant vectors: NaN for both coefficients where there is nothing to rank, and only there
    one = np.full(n, 2.5, dtype=np.float32)
    corr, sums, ranks = check(np.stack([one, v]), y, 'x constant')
    assert sums[0, :2].tolist() == [0, 0] and (ranks[0] == n + 1).all() and np.isnan(corr[0]).all() and not np.isnan(corr[1]).any()
    corr, sums, _ = check(np.stack([v, one]), one, 'y constant')
    assert (sums[:, 2] == 0).all() and np.isnan(corr).all()


def test_signed_zeros_and_infinities():
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1.0], dtype=np.float32)
    f = np.array([0.0, 0.0, 9.0, -9.0, 1.0], dtype=np.float32)
    t = np.arange(5, dtype=np.float32)
    cz, sz, rz = check(z, t, 'zeros and infinities')
    cf, sf, rf = check(f, t, 'the same order, finite')
    assert rz[0].tolist() == [5, 5, 10, 2, 8]                                            # -0 == +0: one value, the average rank
    assert np.array_equal(rz, rf) and np.array_equal(sz, sf) and same_bits(cz[:, 0], cf[:, 0])
    assert np.isnan(cz[0, 1]) and not np.isnan(cf[0, 1])
    r = np.random.RandomState(5)
    n = 130
    x = r.randn(3, n).astype(np.float32)
    y = r.randint(0, 4, size=n).astype(np.float32)
    y[::17] = -0.0
    clean_c, clean_s, clean_r = check(x, y, 'finite')
    big = x.copy()
    big[0][np.argsort(x[0])[-3:]] = np.inf                                                # the three largest: tied at the top
    big[0][np.argsort(x[0])[:2]] = -np.inf
    big[1, ::2], big[1, 1::2] = 0.0, -0.0                                                 # one value: a constant vector
    tied = x.copy()
    tied[0][np.argsort(x[0])[-3:]], tied[0][np.argsort(x[0])[:2]] = 100.0, -100.0
    corr, sums, ranks = check(big, y, 'many zeros and infinities')
    fin, fsums, franks = check(np.stack([tied[0], x[2]]), y, 'finite, the same order')
    assert np.array_equal(ranks[[0, 2, 3]], franks) and np.array_equal(sums[[0, 2]], fsums) and same_bits(corr[[0, 2], 0], fin[:, 0])
    assert np.isnan(corr[0, 1]) and not np.isnan(corr[0, 0])                              # inf: legal for rho, r is NaN
    assert np.isnan(corr[1]).all() and (ranks[1] == n + 1).all()                          # -0 and +0 rank as equal: constant
    assert same_bits(corr[2], clean_c[2]) and np.array_equal(sums[2], clean_s[2])
    yi = y.copy()
    yi[5] = np.inf
    corr, _, _ = check(x, yi, 'an inf rating')
    assert np.isnan(corr[:, 1]).all() and not np.isnan(corr[:, 0]).any()


@pytest.mark.parametrize('n', (65, 300))
def test_nan_in_one_column_and_in_the_ratings(n):
    x, y = rc.case('ratings14', n, 7, C=3)
    clean_c, clean_s, clean_r = check(x, y, 'clean')
    xn = x.copy()
    xn[1, n // 2] = np.nan
    corr, sums, ranks = check(xn, y, 'NaN in column 1')
    assert sums[1, 3] == 1 and np.isnan(corr[1]).all() and ranks[1, n // 2] == 1
    for c in (0, 2):                                                                     # the neighbours: bit-equal to the clean run
        assert np.array_equal(sums[c], clean_s[c]) and same_bits(corr[c], clean_c[c]) and np.array_equal(ranks[c], clean_r[c])
    assert np.array_equal(ranks[3], clean_r[3])
    yn = y.copy()
    yn[[0, n - 1]] = np.nan
    corr, sums, _ = check(x, yn, 'NaN in y')
    assert (sums[:, 3] == 2).all() and np.isnan(corr).all()
    xn[1, 0] = np.nan                                                                    # items 0 (x and y), n / 2 (x), n - 1 (y)
    corr, sums, _ = check(xn, yn, 'NaN in both')
    assert sums[:, 3].tolist() == [2, 3, 2] and np.isnan(corr).all()


# ---- 3. invariances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (129, 1000, 1500))
def test_invariances(n):
    x, y = rc.case('rep3', n, 3, C=4)
    x[3] = np.clip(np.round(x[3]), -2, 6)                                                # one quantised column: ties in x
    ref = rc.reference(x, y)
    corr, sums, ranks = check_against(x, y, ref, 'base')
    assert not np.isnan(corr).any() and (sums[:, 1] < n * (n * n - 1) // 3).all()        # ties everywhere
    again = raw(x, y)                                                                    # the same call twice: the same bits everywhere
    assert same_bits(again[0], corr) and np.array_equal(again[1], sums) and np.array_equal(again[2], ranks)
    dc, ds, dr = raw(2 * x, y)                                                           # x -> 2 x: exact in f32, order and ties kept
    assert same_bits(dc, corr) and np.array_equal(ds, sums) and np.array_equal(dr, ranks)
    nc, ns, nr = raw(-x, y)                                                              # x -> -x: rho and r exactly negated
    assert same_bits(nc, -corr) and np.array_equal(ns[:, 0], -sums[:, 0]) and np.array_equal(ns[:, 1:], sums[:, 1:])
    assert np.array_equal(nr[:4], 2 * (n + 1) - ranks[:4]) and np.array_equal(nr[4], ranks[4])
    # any strictly increasing map of the quantised values: ranks, sums and rho keep their bits (r does not: other values)
    values = np.unique(x[3])
    image = np.cumsum(np.random.RandomState(2).rand(values.size) + 0.1).astype(np.float32) - 3
    mapped = x.copy()
    mapped[3] = image[np.searchsorted(values, x[3])]
    mc, ms, mr = raw(mapped, y)
    assert same_bits(mc[:, 0], corr[:, 0]) and np.array_equal(ms, sums) and np.array_equal(mr, ranks) and same_bits(mc[:3], corr[:3])
    # a joint permutation of the items: rho and the sums keep their bits, the ranks are permuted exactly; r stays within the bound
    # of the exact value (other items share a lane, so the sums round differently: bits need not survive)
    perm = np.random.RandomState(11).permutation(n)
    pc, ps, pr = raw(x[:, perm], y[perm])
    assert same_bits(pc[:, 0], corr[:, 0]) and np.array_equal(ps, sums) and np.array_equal(pr, ranks[:, perm])
    assert rc.close(pc[:, 1], ref['r'], ref['bound']), (pc[:, 1], ref['r'])
    for ld in (0, 1, 61):                                                                # ld = n and other strides: the same answer
        lc, ls, lr = raw(x, y, extra_ld=ld)
        assert same_bits(lc, corr) and np.array_equal(ls, sums) and np.array_equal(lr, ranks)
    for C in (1, 2, 3):                                                                  # a column's answer does not depend on its neighbours
        sc, ss, sr = raw(x[4 - C:], y)
        assert same_bits(sc, corr[4 - C:]) and np.array_equal(ss, sums[4 - C:]) and np.array_equal(sr, ranks[4 - C:])


# ---- 4. the Python wrapper -----------------------------------------------------------------------------------------------------------
def test_wrapper_shapes_dtypes_and_views():
    from distillclip_amd.metrics import RANKCORR_SUMS, rank_correlation
    assert RANKCORR_SUMS == rc.SUM_SLOTS
    x, y = rc.case('quant5', 257, 1, C=3)
    ref = rc.reference(x, y)
    want, _, _ = raw(x, y, extra_ld=0)
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = rank_correlation(d_x, d_y, return_sums=True, return_ranks=True)
    assert set(res) == {'spearman', 'pearson', 'sums', 'ranks', 'human_ranks'}
    assert res['spearman'].shape == res['pearson'].shape == (3,) and res['sums'].shape == (3, 4)
    assert res['ranks'].shape == (3, 257) and res['human_ranks'].shape == (257,) and res['ranks'].dtype == torch.int32
    assert res['spearman'].dtype == torch.float64 and res['sums'].dtype == torch.int64 and res['spearman'].is_cuda
    assert res['spearman'].untyped_storage().data_ptr() == res['pearson'].untyped_storage().data_ptr()      # views of one result buffer
    got = torch.stack([res['spearman'], res['pearson']], dim=1).cpu().numpy()
    assert same_bits(got, want) and np.array_equal(res['sums'].cpu().numpy(), ref['sums'])
    assert np.array_equal(torch.cat([res['ranks'], res['human_ranks'][None]]).cpu().numpy(), ref['ranks'])
    assert set(rank_correlation(d_x, d_y)) == {'spearman', 'pearson'}
    assert set(rank_correlation(d_x, d_y, return_sums=True)) == {'spearman', 'pearson', 'sums'}
    # one vector: 0-dim results; quantised scores and ratings are whole numbers, so integer and float64 inputs give the same f32 values
    one = rank_correlation(d_x[1].long(), d_y.double(), return_sums=True, return_ranks=True)
    assert one['spearman'].shape == one['pearson'].shape == () and one['sums'].shape == (4,) and one['ranks'].shape == (257,)
    assert np.array_equal(one['sums'].cpu().numpy(), ref['sums'][1]) and np.array_equal(one['ranks'].cpu().numpy(), ref['ranks'][1])
    assert same_bits(one['spearman'].item(), got[1, 0]) and same_bits(one['pearson'].item(), got[1, 1])
    half = rank_correlation(d_x.half(), d_y.to(torch.int32), return_sums=True)
    assert np.array_equal(half['sums'].cpu().numpy(), ref['sums'])
    # non-contiguous scores: a transposed [n, C] matrix and a strided slice
    t = rank_correlation(d_x.t().contiguous().t(), d_y, return_sums=True)
    assert not d_x.t().contiguous().t().is_contiguous() and np.array_equal(t['sums'].cpu().numpy(), ref['sums'])
    wide = torch.full((3, 2 * 257), float('nan'), device='cuda')
    wide[:, ::2] = d_x
    s = rank_correlation(wide[:, ::2], d_y)
    assert torch.equal(s['spearman'], res['spearman']) and torch.equal(s['pearson'], res['pearson'])
    with pytest.raises(ValueError, match='device tensors'):
        rank_correlation(d_x, torch.from_numpy(y))


# ---- 5. reporting sizes --------------------------------------------------------------------------------------------------------------
def _check_large(x, y):
    """quantised data: ranks and the four integers against the reference (equality), rho against its expression and SciPy, r against
    the exact value within the bound"""
    ref = rc.reference(x, y)
    corr, sums, ranks = check_against(x, y, ref, f'n={x.shape[1]} C={x.shape[0]}')
    return corr, sums, ranks


def test_flickr8k_expert_size():
    x, y = rc.kc.report_case()
    x = np.round(4 * x) / 4                                                              # quantised scores, every one three times
    assert x.shape == (3, 16992)
    corr, sums, _ = _check_large(x, y)
    assert (np.abs(corr) < 1).all() and (corr > 0.1).all()
    print(f'n=16992 C=3: rho {corr[:, 0]}, r {corr[:, 1]}')


def test_the_cap_on_n():
    """n = 262 144: 4 096 workgroups of the counting kernel, 256 records of the sums, sums of squares that do not fit 53 bits"""
    n = rc.MAX_N
    r = np.random.RandomState(9)
    level = r.randint(0, 4, size=n)
    x = np.round(2 * r.randn(n) + level).astype(np.float32)
    corr, sums, ranks = _check_large(x[None, :], (level / 3.0).astype(np.float32))
    assert sums[0, 1] > 2 ** 52 and sums[0, 2] > 2 ** 52 and ranks.max() > n and 0.2 < corr[0, 0] < 0.8


# ---- 6. the evaluator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('annotators', (None, 3))
@pytest.mark.parametrize('with_refs', (False, True))
def test_evaluator_end_to_end(with_refs, annotators):
    from test_clipscore_gpu import SCOUNTS, _inputs, _students
    from distillclip_amd import HumanCorrelation
    from distillclip_amd.metrics import kendall_tau, rank_correlation
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    hc = HumanCorrelation.from_model(clip, max_batch=4)
    g = torch.Generator().manual_seed(17)
    direct, ratings = [], []
    for b in range(2):
        images, cand, refs = _inputs(40 + 2 * b)
        if not with_refs:
            cand = cand[:, b].contiguous()
        shape = tuple(cand.shape[:-1]) + (() if annotators is None else (annotators,))
        human = torch.randint(1, 5, shape, generator=g)
        human = human if b == 0 else human.float().cuda()
        args = (refs, SCOUNTS) if with_refs else ()
        out = hc.scorer(images, cand, *args)                                              # direct LCLIPScore calls
        direct.append([None if s is None else s.reshape(-1) if annotators is None else s.reshape(-1).repeat_interleave(annotators)
                       for s in out])
        ratings.append(human.reshape(-1).float().cuda())
        hc.update(images, cand, human, *args)
    names = ('clip_s', 'ref_s', 'refclip_s') if with_refs else ('clip_s',)
    scores = torch.stack([torch.cat([d[c] for d in direct]) for c in range(len(names))])
    want = rank_correlation(scores, torch.cat(ratings))
    tau = kendall_tau(scores, torch.cat(ratings), return_counts=True)
    ref = rc.reference(scores.cpu().numpy(), torch.cat(ratings).cpu().numpy())
    assert rc.close(want['spearman'].cpu().numpy(), ref['rho'], rc.RHO_TOL) and rc.close(want['pearson'].cpu().numpy(), ref['r'], ref['bound'])
    for stats in (('spearman',), ('pearson',), ('spearman', 'pearson'), ('pearson', 'kendall'), ('kendall', 'spearman', 'pearson')):
        got = hc.compute(stats=stats)
        kinds = [k for s in stats for k in (('tau_b', 'tau_c') if s == 'kendall' else (s,))]
        assert set(got) == {f'{m}_{k}' for m in names for k in kinds}, stats
        for c, m in enumerate(names):
            for k in kinds:
                src = tau if k.startswith('tau') else want
                assert torch.equal(got[f'{m}_{k}'], src[k][c]) and got[f'{m}_{k}'].dim() == 0 and got[f'{m}_{k}'].dtype == torch.float64, (m, k)
    both = hc.compute(return_counts=True, stats=('kendall', 'pearson'))
    assert set(both) == {f'{m}_{k}' for m in names for k in ('tau_b', 'tau_c', 'counts', 'pearson')}
    # the default: exactly the keys and bits of a kendall_tau call
    for kw, kinds in ((dict(), ('tau_b', 'tau_c')), (dict(return_counts=True), ('tau_b', 'tau_c', 'counts'))):
        got = hc.compute(**kw)
        assert set(got) == {f'{m}_{k}' for m in names for k in kinds}
        assert all(torch.equal(got[f'{m}_{k}'], tau[k][c]) for c, m in enumerate(names) for k in kinds)


def test_default_compute_issues_only_the_kendall_call(monkeypatch):
    from distillclip_amd import correlation
    from distillclip_amd.correlation import HumanCorrelation
    calls = []
    real_k, real_r = correlation.kendall_tau, correlation.rank_correlation
    monkeypatch.setattr(correlation, 'kendall_tau', lambda *a, **k: calls.append('kendall') or real_k(*a, **k))
    monkeypatch.setattr(correlation, 'rank_correlation', lambda *a, **k: calls.append('rank') or real_r(*a, **k))
    hc = HumanCorrelation(lambda *a: None)
    x, y = rc.case('ratings14', 129, 0, C=3)
    hc.add_scores(torch.from_numpy(y).cuda(), *[torch.from_numpy(v).cuda() for v in x])
    hc.compute()
    hc.compute(return_counts=True)
    assert calls == ['kendall', 'kendall']
    del calls[:]
    hc.compute(stats=('spearman', 'pearson'))
    assert calls == ['rank']                                                              # one call for all score kinds, no Kendall call
    del calls[:]
    hc.compute(stats=('pearson', 'kendall', 'spearman'))
    assert calls == ['kendall', 'rank']
