"""Spearman and Pearson against human ratings (dclip_rank_correlation, metrics.rank_correlation, HumanCorrelation.compute(stats=...)), the
parts that need no GPU: the header and the library carry the two entries and the header's wording holds the definitions, the C entry
refuses bad arguments on the host before any launch, the Python layers raise before a kernel runs, and the reference of the GPU tests
(tests/rankcorr_cases.py) agrees with scipy.stats.rankdata, spearmanr and pearsonr on every case the GPU tests use."""
import ctypes
import fractions
import os
import re

import numpy as np
import pytest
import torch

import rankcorr_cases as rc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI and the header's wording ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert protos['dclip_rank_correlation_workspace'] == (ctypes.c_size_t, [I, I])
    assert protos['dclip_rank_correlation'] == (ctypes.c_int, [P, I, I, P, I, P, P, P, P, ctypes.c_size_t, P])
    for name in ('dclip_rank_correlation_workspace', 'dclip_rank_correlation'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed
    # records of at most 256 workgroups and the (C + 1) n twice-ranks: 4 bytes per item and vector, not per pair
    lo, hi = l.dclip_rank_correlation_workspace(2, 1), l.dclip_rank_correlation_workspace(rc.MAX_N, rc.MAX_C)
    assert 0 < lo <= hi and (rc.MAX_C + 1) * rc.MAX_N * 4 <= hi <= (rc.MAX_C + 1) * rc.MAX_N * 4 + (1 << 17) and lo % 16 == 0 and hi % 16 == 0


def _contract():
    from distillclip_amd._lib import _HEADER
    src = open(_HEADER).read()
    block = src[:src.index('size_t dclip_rank_correlation_workspace')]
    block = block[block.rindex('/*'):]
    return re.sub(r'\s*\n \*\s*', ' ', block)


def test_header_states_the_definitions():
    text = _contract()
    for words in ('L_i = #{j : v_j < v_i}', 'Q_i = #{j : v_j == v_i} (i itself included)', 'R_i = 2 L_i + Q_i + 1', 'sum_i R_i = n (n + 1)',
                  "scipy.stats.rankdata(v, 'average')", 'cx_i = Rx_i - (n + 1)', 'all in int64',
                  '-0 == +0', 'a NaN compares false to everything',
                  # the range argument
                  '|c_i| <= n <= 2^18', 'at most 2^36', 'at most 2^54', 'int64 never overflows',
                  'rho = (double)Sxy / (sqrt((double)Sxx) sqrt((double)Syy))', 'clipped to [-1, 1]', 'No floating-point sum occurs before that line',
                  # Pearson
                  'taken to double, which is exact', 'Two passes', 'fixed shape that depends on n alone', 'No atomics',
                  # degenerate inputs
                  "A NaN in a score vector makes that vector's rho and r NaN", 'bit for bit', 'a NaN in human makes every column NaN',
                  'A constant vector (Sxx == 0 or Syy == 0; sxx == 0 or syy == 0) gives rho = r = NaN',
                  '+-inf in a vector is a legal value for rho', 'makes r NaN',
                  '2 <= n <= 262144', '1 <= C <= 4', 'ld >= n', 'nothing launched, nothing written', 'Added without a version bump'):
        assert words in text, words


def test_the_bound_uses_the_kernels_own_summation_shape():
    from distillclip_amd._lib import _HERE
    src = open(os.path.join(_HERE, 'csrc', 'rankcorr.hip')).read()
    assert int(re.search(r'RS_THREADS = (\d+),', src).group(1)) == rc.SUMS_THREADS
    assert int(re.search(r'RS_PER_BLOCK = (\d+);', src).group(1)) == rc.SUMS_PER_BLOCK
    assert int(re.search(r'RS_MAXGRID = (\d+);', src).group(1)) == rc.SUMS_MAXGRID
    assert int(re.search(r'RC_ROWS = (\d+);', src).group(1)) == rc.kc.ROW_BLOCK and int(re.search(r'RC_TILE = (\d+);', src).group(1)) == rc.kc.TILE
    assert [rc.sum_depth(n) for n in (2, 256, 257, 1024, 1025, 4099, 16992, 262144)] == [19, 19, 20, 22, 21, 22, 22, 22]
    assert max(rc.sum_depth(n) for n in range(2, 70000, 7)) == 22 and rc.SUMS_MAXGRID * rc.SUMS_PER_BLOCK == rc.MAX_N


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
# dummy non-null, aligned addresses: never dereferenced, every call below is refused before a launch
X, Y, CORR, SUMS, RANKS, WS = 4096, 8192, 12288, 16384, 20480, 1 << 20


def _call(**k):
    g = lambda name, default: k[name] if name in k else default
    n, C = g('n', 100), g('C', 3)
    ws_bytes = g('ws_bytes', max(_lib().dclip_rank_correlation_workspace(n, C), 16))
    return _lib().dclip_rank_correlation(g('x', X), g('ld', n), C, g('y', Y), n, g('corr', CORR), g('sums', SUMS), g('ranks', RANKS),
                                         g('ws', WS), ws_bytes, None)


@pytest.mark.parametrize('kw,word', [
    (dict(n=1), 'n <= 262144'), (dict(n=0), 'n <= 262144'), (dict(n=-5), 'n <= 262144'), (dict(n=rc.MAX_N + 1, ws_bytes=1 << 30), 'n <= 262144'),
    (dict(C=0), 'C <= 4'), (dict(C=5, ws_bytes=1 << 30), 'C <= 4'), (dict(C=-1), 'C <= 4'),
    (dict(ld=99), 'ld=99'), (dict(ld=0), 'ld=0'), (dict(ld=-100), 'ld=-100'),
    (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(corr=None), 'null'), (dict(ws=None), 'null'),
    (dict(x=None, sums=None, ranks=None), 'null'),
    (dict(x=X + 2), 'misaligned'), (dict(y=Y + 1), 'misaligned'), (dict(corr=CORR + 4), 'misaligned'), (dict(sums=SUMS + 4), 'misaligned'),
    (dict(ranks=RANKS + 2), 'misaligned'), (dict(ws=WS + 8), 'misaligned'), (dict(sums=None, ranks=RANKS + 1), 'misaligned'),
    (dict(ws_bytes=0), 'workspace too small'), (dict(ws_bytes=255), 'workspace too small'),
    (dict(sums=None, ranks=None, ws_bytes=1024), 'workspace too small'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word) as e:
        _call(**kw)
    assert 'dclip_rank_correlation:' in str(e.value)             # the error string names the entry


def test_workspace_query_of_a_refused_shape_is_zero():
    l = _lib()
    for n, C in ((1, 1), (0, 2), (-3, 1), (rc.MAX_N + 1, 1), (100, 0), (100, 5), (100, -1)):
        assert l.dclip_rank_correlation_workspace(n, C) == 0, (n, C)
    assert l.dclip_rank_correlation_workspace(2, 1) > 0 and l.dclip_rank_correlation_workspace(rc.MAX_N, 4) > 0
    with pytest.raises(ValueError, match='workspace too small'):
        _call(n=rc.MAX_N, ws_bytes=l.dclip_rank_correlation_workspace(rc.MAX_N, 3) - 1)


# ---- 3. the Python layers ------------------------------------------------------------------------------------------------------------
def test_rank_correlation_raises_on_the_host():
    """CPU tensors are themselves refused with a ValueError, last: every other complaint comes before it and before any launch"""
    from distillclip_amd.metrics import RANKCORR_SUMS, rank_correlation
    assert RANKCORR_SUMS == rc.SUM_SLOTS
    with pytest.raises(ValueError, match='7 scores per vector against 6 ratings'):
        rank_correlation(torch.zeros(7), torch.zeros(6))
    with pytest.raises(ValueError, match='7 scores per vector against 3 ratings'):
        rank_correlation(torch.zeros(3, 7), torch.zeros(3))
    with pytest.raises(ValueError, match='n=1'):
        rank_correlation(torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match='n=0'):
        rank_correlation(torch.zeros(2, 0), torch.zeros(0))
    with pytest.raises(ValueError, match=f'n={rc.MAX_N + 1}'):
        rank_correlation(torch.zeros(rc.MAX_N + 1), torch.zeros(rc.MAX_N + 1))
    with pytest.raises(ValueError, match='C=5'):
        rank_correlation(torch.zeros(5, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='C=0'):
        rank_correlation(torch.zeros(0, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='need scores'):
        rank_correlation(torch.zeros(2, 3, 4), torch.zeros(4))
    with pytest.raises(ValueError, match='need scores'):
        rank_correlation(torch.zeros(4), torch.zeros(4, 1))
    with pytest.raises(ValueError, match='need scores'):
        rank_correlation([1.0, 2.0], torch.zeros(2))
    with pytest.raises(ValueError, match='device tensors'):
        rank_correlation(torch.zeros(3, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='device tensors'):
        rank_correlation(torch.zeros(9, dtype=torch.int64), torch.zeros(9, dtype=torch.float64), return_sums=True, return_ranks=True)


def test_compute_refuses_bad_stats_before_a_concatenation(monkeypatch):
    from distillclip_amd import correlation
    from distillclip_amd.correlation import HumanCorrelation
    from test_kendall_cpu import _FixedScorer
    assert correlation.STATS == ('kendall', 'spearman', 'pearson')
    hc = HumanCorrelation(_FixedScorer())
    v = torch.zeros(5)
    hc._store(v, [v, None, None], False)                           # what an accepted update leaves behind
    hc._store(v, [v, None, None], False)
    cats = []
    monkeypatch.setattr(correlation.torch, 'cat', lambda *a, **k: cats.append(a))
    for bad in ((), [], ('kendal',), ('kendall', 'rho'), ('spearman', 'spearman'), ('kendall', None), 'tau', 'kendall', (1,)):              # (a string is a sequence of letters)
        with pytest.raises(ValueError, match='stats must be a non-empty subset'):
            hc.compute(stats=bad)
    for stats in (('spearman',), ('pearson',), ('pearson', 'spearman'), ['spearman']):
        with pytest.raises(ValueError, match="has no 'kendall'"):
            hc.compute(return_counts=True, stats=stats)
    assert not cats
    hc.reset()
    with pytest.raises(ValueError, match='0 rated items'):
        hc.compute(stats=('spearman', 'pearson'))
    with pytest.raises(ValueError, match='stats must be'):           # a bad stats is reported whatever is stored
        hc.compute(stats=())


# ---- 4. the reference against SciPy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', rc.SEEDS)
@pytest.mark.parametrize('n', rc.SIZES)
def test_reference_agrees_with_scipy(n, seed):
    from scipy.stats import rankdata
    seen = set()
    for family in rc.ALL_FAMILIES:
        x, y, ref = rc.case_with_reference(family, n, seed)
        C = x.shape[0]
        assert x.dtype == y.dtype == np.float32 and y.shape == (n,) and ref['ranks'].shape == (C + 1, n)
        if family != rc.PEARSON_FAMILY:
            assert C == rc.kc.n_vectors(family, n, seed)
            seen.add(C)
        for v, rk in zip(list(x) + [y], ref['ranks']):
            assert np.array_equal(rk, np.rint(2 * rankdata(v.astype(np.float64), 'average')).astype(np.int64))
            assert rk.sum() == n * (n + 1)
        sp_rho, sp_r = rc.scipy_reference(x, y)
        assert rc.close(ref['rho'], sp_rho, rc.RHO_TOL), (family, ref['rho'], sp_rho)
        assert rc.close(ref['r'], sp_r, rc.SCIPY_R_TOL), (family, ref['r'], sp_r)
        assert (ref['sums'][:, 3] == 0).all() and (ref['sums'][:, 2] == ref['sums'][0, 2]).all()
        finite = ~np.isnan(ref['r'])
        assert (ref['bound'][finite] > 0).all() and (ref['bound'][finite] < 1e-13).all(), (family, ref['bound'])
        if n >= 63:
            assert finite.all() and not np.isnan(ref['rho']).any(), family
    assert seen == {1, 2, 3, 4}


def test_exact_pearson_equals_literal_fraction_sums():
    import mpmath
    F = fractions.Fraction
    for family, n in (('thirds', 65), ('offset20', 129), ('quant5', 257), ('rep3', 64)):
        x, y = rc.case(family, n, 1, C=2)
        for row in x:
            fx, fy = [F(float(t)) for t in row], [F(float(t)) for t in y]
            mx, my = sum(fx) / n, sum(fy) / n
            sxy = sum((a - mx) * (b - my) for a, b in zip(fx, fy))
            sxx, syy = sum((a - mx) ** 2 for a in fx), sum((b - my) ** 2 for b in fy)
            with mpmath.workdps(60):
                want = float(mpmath.mpf(sxy.numerator) / sxy.denominator /
                             mpmath.sqrt(mpmath.mpf(sxx.numerator) / sxx.denominator * mpmath.mpf(syy.numerator) / syy.denominator))
            r, fxx, fyy = rc.pearson_exact(row, y)
            assert r == want and fxx == float(sxx) and fyy == float(syy), (family, r, want)


def test_reference_on_degenerate_inputs():
    r = np.random.RandomState(3)
    n = 65
    x, y = r.randn(n).astype(np.float32), r.randint(1, 5, size=n).astype(np.float32)
    one = np.ones(n, dtype=np.float32)
    for a, b in ((one, y), (x, one), (one, one)):                  # constant: NaN for both, as SciPy
        ref = rc.reference(a, b)
        sp = rc.scipy_reference(a, b)
        assert np.isnan(ref['rho']).all() and np.isnan(ref['r']).all() and np.isnan(sp[0]).all() and np.isnan(sp[1]).all()
    xn = x.copy()
    xn[7] = np.nan
    ref = rc.reference(np.stack([x, xn]), y)
    assert ref['sums'][:, 3].tolist() == [0, 1] and ref['ranks'][1, 7] == 1 and np.isnan(ref['rho'][1]) and np.isnan(ref['r'][1])
    assert not np.isnan(ref['rho'][0]) and np.isnan(rc.scipy_reference(xn, y)[0]).all()
    # -0 == +0 (one value, average rank) and +-inf rank first and last: rho as with finite values in the same order, r NaN
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1.0], dtype=np.float32)
    f = np.array([0.0, 0.0, 9.0, -9.0, 1.0], dtype=np.float32)
    t = np.arange(5, dtype=np.float32)
    rz, rf = rc.reference(z, t), rc.reference(f, t)
    assert rz['ranks'][0].tolist() == [5, 5, 10, 2, 8] and np.array_equal(rz['ranks'], rf['ranks']) and rz['rho'] == rf['rho']
    assert np.isnan(rz['r']).all() and not np.isnan(rf['r']).any()
    sp = rc.scipy_reference(z, t)
    assert rc.close(rz['rho'], sp[0], rc.RHO_TOL) and np.isnan(sp[1]).all()
    # x = y and reversed ranks: the integers say +-1 exactly
    for m in rc.SIZES:
        v = ((np.random.RandomState(m).permutation(m) - m // 2) / 8.0).astype(np.float32)
        s = rc.reference(v, v)['sums'][0]
        assert s[0] == s[1] == s[2] == m * (m * m - 1) // 3         # sum (2 k - (m + 1))^2 over k = 1 .. m
        s = rc.reference(-v, v)['sums'][0]
        assert -s[0] == s[1] == s[2]
