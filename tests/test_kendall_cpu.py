"""Kendall tau against human ratings (dclip_kendall_tau, metrics.kendall_tau, HumanCorrelation), the parts that need no GPU: the header
and the library carry the two entries, the C entry refuses bad arguments on the host before any launch, the Python layers raise before
a tower or a kernel runs, and the integer reference of the GPU tests (tests/kendall_cases.py) agrees with scipy.stats.kendalltau on every
case the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kendall_cases as kc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert protos['dclip_kendall_tau_workspace'] == (ctypes.c_size_t, [I, I])
    assert protos['dclip_kendall_tau'] == (ctypes.c_int, [P, I, I, P, I, P, P, P, ctypes.c_size_t, P])
    for name in ('dclip_kendall_tau_workspace', 'dclip_kendall_tau'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed
    # per-workgroup partial sums only: far below one byte per item pair, and growing with n
    assert 0 < l.dclip_kendall_tau_workspace(2, 1) <= l.dclip_kendall_tau_workspace(kc.MAX_N, kc.MAX_C) <= 4 << 20


def test_the_cases_use_the_kernels_own_tile_sizes():
    from distillclip_amd._lib import _HERE
    src = open(os.path.join(_HERE, 'csrc', 'kendall.hip')).read()
    assert int(re.search(r'KT_ROWS = (\d+);', src).group(1)) == kc.ROW_BLOCK
    assert int(re.search(r'KT_TILE = (\d+);', src).group(1)) == kc.TILE
    for T in (kc.ROW_BLOCK, kc.TILE):
        assert {T - 1, T, T + 1, 2 * T + 1} <= set(kc.SIZES)
    assert {2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4099} <= set(kc.SIZES)


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
# dummy non-null, aligned addresses: never dereferenced, every call below is refused before a launch
X, Y, TAU, CNT, WS = 4096, 8192, 12288, 16384, 1 << 20


def _call(**k):
    g = lambda name, default: k[name] if name in k else default
    n, C = g('n', 100), g('C', 3)
    ws_bytes = g('ws_bytes', max(_lib().dclip_kendall_tau_workspace(n, C), 16))
    return _lib().dclip_kendall_tau(g('x', X), g('ld', n), C, g('y', Y), n, g('tau', TAU), g('counts', CNT), g('ws', WS), ws_bytes, None)


@pytest.mark.parametrize('kw,word', [
    (dict(n=1), 'n <= 262144'), (dict(n=0), 'n <= 262144'), (dict(n=-5), 'n <= 262144'), (dict(n=kc.MAX_N + 1, ws_bytes=1 << 30), 'n <= 262144'),
    (dict(C=0), 'C <= 4'), (dict(C=5, ws_bytes=1 << 30), 'C <= 4'), (dict(C=-1), 'C <= 4'),
    (dict(ld=99), 'ld=99'), (dict(ld=0), 'ld=0'), (dict(ld=-100), 'ld=-100'),
    (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(tau=None), 'null'), (dict(counts=None), 'null'), (dict(ws=None), 'null'),
    (dict(x=X + 2), 'misaligned'), (dict(y=Y + 1), 'misaligned'), (dict(tau=TAU + 4), 'misaligned'), (dict(counts=CNT + 4), 'misaligned'),
    (dict(ws=WS + 8), 'misaligned'),
    (dict(ws_bytes=0), 'workspace too small'), (dict(ws_bytes=255), 'workspace too small'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word):
        _call(**kw)


def test_workspace_query_of_a_refused_shape_is_zero():
    l = _lib()
    for n, C in ((1, 1), (0, 2), (-3, 1), (kc.MAX_N + 1, 1), (100, 0), (100, 5), (100, -1)):
        assert l.dclip_kendall_tau_workspace(n, C) == 0, (n, C)
    assert l.dclip_kendall_tau_workspace(2, 1) > 0 and l.dclip_kendall_tau_workspace(kc.MAX_N, 4) > 0
    with pytest.raises(ValueError, match='workspace too small'):
        _call(n=kc.MAX_N, ws_bytes=l.dclip_kendall_tau_workspace(kc.MAX_N, 3) - 1)


# ---- 3. the Python layers ------------------------------------------------------------------------------------------------------------
def test_kendall_tau_raises_on_the_host():
    """CPU tensors are themselves refused with a ValueError, last: every other complaint comes before it and before any launch"""
    from distillclip_amd.metrics import kendall_tau
    with pytest.raises(ValueError, match='7 scores per vector against 6 ratings'):
        kendall_tau(torch.zeros(7), torch.zeros(6))
    with pytest.raises(ValueError, match='7 scores per vector against 3 ratings'):
        kendall_tau(torch.zeros(3, 7), torch.zeros(3))
    with pytest.raises(ValueError, match='n=1'):
        kendall_tau(torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match='n=0'):
        kendall_tau(torch.zeros(2, 0), torch.zeros(0))
    with pytest.raises(ValueError, match=f'n={kc.MAX_N + 1}'):
        kendall_tau(torch.zeros(kc.MAX_N + 1), torch.zeros(kc.MAX_N + 1))
    with pytest.raises(ValueError, match='C=5'):
        kendall_tau(torch.zeros(5, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='C=0'):
        kendall_tau(torch.zeros(0, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='need scores'):
        kendall_tau(torch.zeros(2, 3, 4), torch.zeros(4))
    with pytest.raises(ValueError, match='need scores'):
        kendall_tau(torch.zeros(4), torch.zeros(4, 1))
    with pytest.raises(ValueError, match='device tensors'):
        kendall_tau(torch.zeros(3, 9), torch.zeros(9))
    with pytest.raises(ValueError, match='device tensors'):
        kendall_tau(torch.zeros(9, dtype=torch.int64), torch.zeros(9, dtype=torch.float64), return_counts=True)


class _FixedScorer:
    """stands in for an LCLIPScore: fixed tensors of the right shape, and a count of its calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self, images, candidates, references=None, ref_counts=None):
        from distillclip_amd.score import ScoreOutput
        self.calls += 1
        s = torch.arange(candidates.shape[:-1].numel(), dtype=torch.float32).reshape(candidates.shape[:-1])
        return ScoreOutput(s, None if references is None else s + 1, None if references is None else s + 2)


def _stored(hc):
    return hc._n, len(hc._human), [len(v) for v in hc._scores]


def test_evaluator_is_exported_and_raises_on_the_host():
    import distillclip_amd
    from distillclip_amd.correlation import HumanCorrelation
    assert distillclip_amd.HumanCorrelation is HumanCorrelation
    sc = _FixedScorer()
    hc = HumanCorrelation(sc)
    assert hc.scorer is sc
    with pytest.raises(ValueError, match='scorer'):
        HumanCorrelation(None)
    B, K, L = 4, 3, 13
    images = torch.zeros(B, 3, 32, 32)
    one, many = torch.ones(B, L, dtype=torch.int64), torch.ones(B, K, L, dtype=torch.int64)
    # a human of the wrong shape: refused before the scorer (the towers) runs
    for cand, human in ((one, torch.zeros(B + 1)), (one, torch.zeros(B, 2, 2)), (one, torch.zeros(())), (many, torch.zeros(B)),
                        (many, torch.zeros(B, K + 1)), (many, torch.zeros(B, K, 2, 2)), (many, torch.zeros(K, B)), (one, torch.zeros(B, 0))):
        with pytest.raises(ValueError, match='human must be'):
            hc.update(images, cand, human)
    with pytest.raises(ValueError, match='need images'):
        hc.update(images[0], one, torch.zeros(B))
    with pytest.raises(ValueError, match='need images'):
        hc.update(images, one[:2], torch.zeros(2))
    assert sc.calls == 0 and _stored(hc) == (0, 0, [0, 0, 0])
    with pytest.raises(ValueError, match='0 rated items'):
        hc.compute()
    # add_scores: flat device vectors of one length, ref_s and refclip_s together
    v = torch.zeros(5)
    with pytest.raises(ValueError, match='come together'):
        hc.add_scores(v, v, ref_s=v)
    with pytest.raises(ValueError, match='flat vectors'):
        hc.add_scores(v, torch.zeros(6))
    with pytest.raises(ValueError, match='flat vectors'):
        hc.add_scores(torch.zeros(5, 1), torch.zeros(5, 1))
    with pytest.raises(ValueError, match='flat vectors'):
        hc.add_scores(torch.zeros(0), torch.zeros(0))
    with pytest.raises(ValueError, match='device tensors'):
        hc.add_scores(v, v, v, v)
    assert _stored(hc) == (0, 0, [0, 0, 0])
    # what has been stored decides what may follow: the stand-in state below is what accepted calls leave behind
    hc._store(v, [v, None, None], False)
    with pytest.raises(ValueError, match='cannot be mixed'):
        hc.update(images, one, torch.zeros(B), references=torch.ones(B, 2, L, dtype=torch.int64))
    with pytest.raises(ValueError, match='cannot be mixed'):
        hc.add_scores(v, v, v, v)
    assert sc.calls == 0 and _stored(hc) == (5, 1, [1, 1, 1])
    hc.reset()
    assert _stored(hc) == (0, 0, [0, 0, 0]) and hc._with_refs is None
    hc._store(v[:1], [v[:1], v[:1], v[:1]], True)
    with pytest.raises(ValueError, match='cannot be mixed'):
        hc.update(images, one, torch.zeros(B))
    with pytest.raises(ValueError, match='1 rated items'):
        hc.compute()                                                   # fewer than 2
    hc.reset()
    big = torch.zeros(kc.MAX_N // 2 + 1)
    hc._store(big, [big, None, None], False)
    hc._store(big, [big, None, None], False)
    with pytest.raises(ValueError, match=f'{kc.MAX_N + 2} rated items'):
        hc.compute()                                                   # more than the kernel takes: refused before any concatenation


def test_evaluator_from_model_builds_the_scorer():
    from test_host_logic_cpu import _tiny_students
    from distillclip_amd import HumanCorrelation, LCLIPScore
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _tiny_students()
    clip = CLIPModel(True, s_img, s_txt)
    hc = HumanCorrelation.from_model(clip, max_batch=64)
    assert isinstance(hc.scorer, LCLIPScore) and hc.scorer.image_encoder is s_img and hc.scorer.max_batch == 64
    with pytest.raises(ValueError, match='tower'):
        HumanCorrelation.from_model(s_img)
    images, cand = torch.zeros(4, 3, 32, 32), torch.ones(4, 13, dtype=torch.int64)
    with pytest.raises(ValueError, match='human must be'):
        hc.update(images, cand, torch.zeros(5))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hc.update(images, cand, torch.zeros(4))                        # well-formed: reaches the towers, which have no CPU path
    assert _stored(hc) == (0, 0, [0, 0, 0])
    flags = [(p.requires_grad, m.training) for m in (s_img, s_txt) for p in m.parameters()]
    assert all(r for r, _ in flags) and all(t for _, t in flags)       # building an evaluator changes no flag


# ---- 4. the integer reference against SciPy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', kc.SEEDS)
@pytest.mark.parametrize('n', kc.SIZES)
def test_reference_agrees_with_scipy(n, seed):
    n0 = n * (n - 1) // 2
    seen = set()
    for family in kc.FAMILIES:
        x, y, slots, taus = kc.case_with_reference(family, n, seed)
        assert x.shape == (kc.n_vectors(family, n, seed), n) and y.shape == (n,) and x.dtype == y.dtype == np.float32
        seen.add(x.shape[0])
        want = kc.scipy_taus(x, y)
        assert kc.tau_close(taus, want), (family, taus, want)
        assert (np.isnan(taus) == np.isnan(want)).all()
        con, dis, tie_x, tie_y, tie_xy, dx, dy, nan = slots.T
        assert (con + dis + tie_x + tie_y - tie_xy == n0).all() and (nan == 0).all()
        assert (tie_y == kc.tie_counts(y)).all() and (dy == kc.distinct(y)).all()
        for c, row in enumerate(x):
            assert tie_x[c] == kc.tie_counts(row) and tie_xy[c] == kc.joint_tie_counts(row, y)
        if family == 'rep3' and n >= 63:
            assert (tie_x >= n // 3).all() and (dx <= (n + 2) // 3).all()             # systematic ties in x
        if family == 'quant5':
            assert (dx <= 5).all()
    assert seen == {1, 2, 3, 4}


def test_reference_on_degenerate_inputs_is_nan_where_scipy_is():
    r = np.random.RandomState(3)
    n = 65
    x, y = r.randn(n).astype(np.float32), r.randint(1, 5, size=n).astype(np.float32)
    one = np.ones(n, dtype=np.float32)
    for a, b, nan_b, nan_c in ((one, y, True, True), (x, one, True, True), (one, one, True, True), (x, y, False, False),
                               (x[:2], y[:2] * 0, True, True), (np.array([1, 2], np.float32), np.array([3, 4], np.float32), False, False)):
        slots, taus = kc.reference(a, b)
        want = kc.scipy_taus(a, b)
        assert (np.isnan(taus[0]) == [nan_b, nan_c]).all() and (np.isnan(want[0]) == [nan_b, nan_c]).all(), (taus, want)
        assert kc.tau_close(taus, want)
    # a NaN anywhere: both taus NaN, as SciPy propagates it; the slot counts the items
    xn = x.copy()
    xn[7] = np.nan
    slots, taus = kc.reference(xn, y)
    assert slots[0, 7] == 1 and np.isnan(taus).all() and np.isnan(kc.scipy_taus(xn, y)).all()
    assert slots[0, 5] == kc.distinct(x)                               # continuous: the NaN is one more distinct value, 65 in all
    # -0 == +0 and +-inf order normally
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1.0], dtype=np.float32)
    slots, taus = kc.reference(z, np.arange(5, dtype=np.float32))
    assert slots[0].tolist() == [5, 4, 1, 0, 0, 4, 5, 0] and kc.tau_close(taus, kc.scipy_taus(z, np.arange(5)))
    # x = y: every pair concordant and both taus 1; SciPy's own quotient a / sqrt(a) / sqrt(a) is one ulp off 1 for many a
    for m in kc.SIZES:
        v = ((np.random.RandomState(m).permutation(m) - m // 2) / 8.0).astype(np.float32)
        slots, taus = kc.reference(v, v)
        assert slots[0].tolist() == [m * (m - 1) // 2, 0, 0, 0, 0, m, m, 0] and kc.tau_close(taus, [[1.0, 1.0]])
        assert kc.tau_close(taus, kc.scipy_taus(v, v))
