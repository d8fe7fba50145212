"""Kendall tau against human ratings on the GPU (dclip_kendall_tau, metrics.kendall_tau, HumanCorrelation).  The eight integer counts are
compared for EQUALITY with the integer reference of tests/kendall_cases.py, the taus with that reference and with scipy.stats.kendalltau
within relative 1e-14; invariances are exact on counts and bit-equal on taus.  Every raw call runs on guarded buffers: the inputs sit 16
bytes into NaN-filled buffers with ld > n, the outputs between sentinels, the workspace is exactly as large as the query says and is
followed by a patterned guard.  tests/test_kendall_cpu.py checks the reference itself against SciPy."""
import numpy as np
import pytest
import torch

import kendall_cases as kc

pytestmark = pytest.mark.gpu

PAD, SENT = 64, -777


def raw(x, y, extra_ld=3):
    """x [C, n], y [n] (numpy f32) -> counts int64 [C, 8], taus float64 [C, 2] from one guarded call of the C entry"""
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
    tau = torch.full((2 * PAD + 2 * C,), float(SENT), dtype=torch.float64, device='cuda')
    cnt = torch.full((2 * PAD + 8 * C,), SENT, dtype=torch.int64, device='cuda')
    need = lib().dclip_kendall_tau_workspace(n, C)
    assert need > 0 and need % 16 == 0
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device='cuda')
    lib().dclip_kendall_tau(d_x.data_ptr() + 16, ld, C, d_y.data_ptr() + 16, n, tau.data_ptr() + 8 * PAD, cnt.data_ptr() + 8 * PAD,
                            ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    tau, cnt = tau.cpu().numpy(), cnt.cpu().numpy()
    for buf, m in ((tau, 2 * C), (cnt, 8 * C)):
        assert (buf[:PAD] == SENT).all() and (buf[PAD + m:] == SENT).all()               # nothing outside [C][2] and [C][8]
    assert (ws[need:] == 0xA5).all()                                                      # nothing past the workspace
    assert np.array_equal(d_x.cpu().numpy(), xb, equal_nan=True) and np.array_equal(d_y.cpu().numpy(), yb, equal_nan=True)
    return cnt[PAD:PAD + 8 * C].reshape(C, 8).copy(), tau[PAD:PAD + 2 * C].reshape(C, 2).copy()


def check(x, y, what=''):
    """the guarded call against the integer reference (equality) and both tau references (1e-14) -> counts, taus"""
    want_c, want_t = kc.reference(x, y)
    return check_against(x, y, want_c, want_t, what)


def check_against(x, y, want_c, want_t, what=''):
    cnt, tau = raw(x, y)
    assert np.array_equal(cnt, want_c), (what, cnt.tolist(), want_c.tolist())
    assert kc.tau_close(tau, want_t), (what, tau, want_t)
    sp = kc.scipy_taus(x, y)
    assert kc.tau_close(tau, sp), (what, tau, sp)
    return cnt, tau


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ---- 1. the case families at every size ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', kc.SEEDS)
@pytest.mark.parametrize('n', kc.SIZES)
def test_counts_equal_the_integer_reference(n, seed):
    n0 = n * (n - 1) // 2
    for family in kc.FAMILIES:
        x, y, want_c, want_t = kc.case_with_reference(family, n, seed)
        cnt, tau = check_against(x, y, want_c, want_t, (family, n, seed))
        con, dis, tie_x, tie_y, tie_xy = cnt.T[:5]
        assert (con + dis + tie_x + tie_y - tie_xy == n0).all()
        assert (cnt[:, 3] == cnt[0, 3]).all() and (cnt[:, 6] == cnt[0, 6]).all()          # the y slots are the same for every column
        print(f'{family} n={n} seed={seed} C={x.shape[0]}: counts equal, tau_b {tau[:, 0]}, tau_c {tau[:, 1]}')


# ---- 2. special inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (65, 257, 1000))
def test_identity_reversal_and_constant_vectors(n):
    n0 = n * (n - 1) // 2
    r = np.random.RandomState(n)
    v = ((r.permutation(n) - n // 2) / 8.0).astype(np.float32)                           # n distinct values
    y = r.randint(1, 5, size=n).astype(np.float32)
    # x = y: every untied pair is concordant and tau_b is 1 exactly
    cnt, tau = check(v, v, 'x = y')
    assert cnt[0].tolist() == [n0, 0, 0, 0, 0, n, n, 0] and tau[0, 0] == 1.0 and tau[0, 1] == 1.0
    cnt, tau = check(y, y, 'x = y with ties')
    t = kc.tie_counts(y)
    assert cnt[0].tolist()[:5] == [n0 - t, 0, t, t, t] and tau[0, 0] == 1.0
    # the ratings reversed: con and dis change places
    x = np.stack([v + y, r.randn(n).astype(np.float32)])
    fwd, tf = check(x, y, 'forward')
    rev, tr = check(x, -y, 'y reversed')
    assert np.array_equal(rev[:, [1, 0]], fwd[:, [0, 1]]) and np.array_equal(rev[:, 2:], fwd[:, 2:]) and np.array_equal(tr, -tf)
    cnt, tau = check(-v, v, 'x = -y')
    assert cnt[0].tolist() == [0, n0, 0, 0, 0, n, n, 0] and tau[0, 0] == -1.0
    # all x tied, all y tied, both: NaN where there is nothing to rank, and only there
    one = np.ones(n, dtype=np.float32)
    cnt, tau = check(np.stack([one, v]), y, 'x tied')
    assert cnt[0].tolist() == [0, 0, n0, t, t, 1, cnt[1, 6], 0] and np.isnan(tau[0]).all() and not np.isnan(tau[1]).any()
    cnt, tau = check(np.stack([v, one]), one, 'y tied')
    assert cnt[0].tolist() == [0, 0, 0, n0, 0, n, 1, 0] and cnt[1].tolist() == [0, 0, n0, n0, n0, 1, 1, 0] and np.isnan(tau).all()


def test_signed_zeros_and_infinities():
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1.0], dtype=np.float32)
    cnt, _ = check(z, np.arange(5, dtype=np.float32), 'zeros and infinities')
    assert cnt[0].tolist() == [5, 4, 1, 0, 0, 4, 5, 0]                                   # -0 == +0: a tie, one value
    r = np.random.RandomState(5)
    n = 130
    x = r.randn(2, n).astype(np.float32)
    x[0, ::7], x[0, 3::11], x[1, ::2], x[1, 1::2] = np.inf, -np.inf, 0.0, -0.0
    y = r.randint(0, 4, size=n).astype(np.float32)
    y[5::13], y[::17] = -np.inf, -0.0
    cnt, tau = check(x, y, 'many zeros and infinities')
    assert cnt[1].tolist()[:2] == [0, 0] and cnt[1, 5] == 1 and np.isnan(tau[1]).all() and not np.isnan(tau[0]).any()


@pytest.mark.parametrize('n', (65, 300))
def test_nan_in_one_column_and_in_the_ratings(n):
    x, y = kc.case('ratings14', n, 7, C=3)
    clean_c, clean_t = check(x, y, 'clean')
    xn = x.copy()
    xn[1, n // 2] = np.nan
    cnt, tau = check(xn, y, 'NaN in column 1')
    assert cnt[1, 7] == 1 and np.isnan(tau[1]).all()
    for c in (0, 2):                                                                     # the neighbours: bit-equal to the clean run
        assert np.array_equal(cnt[c], clean_c[c]) and same_bits(tau[c], clean_t[c])
    yn = y.copy()
    yn[[0, n - 1]] = np.nan
    cnt, tau = check(x, yn, 'NaN in y')
    assert (cnt[:, 7] == 2).all() and np.isnan(tau).all()
    xn[1, 0] = np.nan                                                                    # items 0 (x and y), n / 2 (x), n - 1 (y)
    cnt, tau = check(xn, yn, 'NaN in both')
    assert cnt[:, 7].tolist() == [2, 3, 2] and np.isnan(tau).all()


# ---- 3. invariances: exact on counts, bit-equal on taus ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (129, 1000))
def test_invariances(n):
    x, y = kc.case('rep3', n, 3, C=4)
    x[3] = np.round(x[3])                                                                # one quantised column: ties in x and joint ties
    cnt, tau = check(x, y, 'base')
    assert (cnt[:, 2] > 0).all() and cnt[3, 4] > 0 and (cnt[:, :2] > 0).all()
    again_c, again_t = raw(x, y)                                                         # the same call twice
    assert np.array_equal(again_c, cnt) and same_bits(again_t, tau)
    perm = np.random.RandomState(11).permutation(n)                                      # a joint permutation of the items
    pc, pt = raw(x[:, perm], y[perm])
    assert np.array_equal(pc, cnt) and same_bits(pt, tau)
    dc, dt = raw(2 * x, y)                                                               # x -> 2 x: exact in f32, order and ties kept
    assert np.array_equal(dc, cnt) and same_bits(dt, tau)
    nc, nt = raw(-x, y)                                                                  # x -> -x: con and dis change places
    assert np.array_equal(nc[:, [1, 0]], cnt[:, [0, 1]]) and np.array_equal(nc[:, 2:], cnt[:, 2:]) and np.array_equal(nt, -tau)
    for ld in (0, 1, 61):                                                                # ld = n and other strides: the same answer
        lc, lt = raw(x, y, extra_ld=ld)
        assert np.array_equal(lc, cnt) and same_bits(lt, tau)
    for C in (1, 2, 3):                                                                  # a column's answer does not depend on its neighbours
        sc, st_ = raw(x[4 - C:], y)
        assert np.array_equal(sc, cnt[4 - C:]) and same_bits(st_, tau[4 - C:])


# ---- 4. the Python wrapper -----------------------------------------------------------------------------------------------------------
def test_wrapper_shapes_dtypes_and_views():
    from distillclip_amd.metrics import KENDALL_COUNTS, kendall_tau
    assert KENDALL_COUNTS == kc.SLOTS
    x, y = kc.case('quant5', 257, 1, C=3)
    want_c, want_t = kc.reference(x, y)
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = kendall_tau(d_x, d_y, return_counts=True)
    assert set(res) == {'tau_b', 'tau_c', 'counts'}
    assert res['tau_b'].shape == res['tau_c'].shape == (3,) and res['counts'].shape == (3, 8)
    assert res['tau_b'].dtype == torch.float64 and res['counts'].dtype == torch.int64 and res['tau_b'].is_cuda
    assert res['tau_b'].untyped_storage().data_ptr() == res['tau_c'].untyped_storage().data_ptr()      # views of one result buffer
    got_t = torch.stack([res['tau_b'], res['tau_c']], dim=1).cpu().numpy()
    assert np.array_equal(res['counts'].cpu().numpy(), want_c) and kc.tau_close(got_t, want_t)
    assert set(kendall_tau(d_x, d_y)) == {'tau_b', 'tau_c'}
    # one vector: 0-dim results; quantised scores and ratings are whole numbers, so integer and float64 inputs give the same f32 values
    one = kendall_tau(d_x[1].long(), d_y.double(), return_counts=True)
    assert one['tau_b'].shape == one['tau_c'].shape == () and one['counts'].shape == (8,)
    assert np.array_equal(one['counts'].cpu().numpy(), want_c[1])
    assert same_bits(one['tau_b'].item(), got_t[1, 0]) and same_bits(one['tau_c'].item(), got_t[1, 1])
    half = kendall_tau(d_x.half(), d_y.to(torch.int32), return_counts=True)
    assert np.array_equal(half['counts'].cpu().numpy(), want_c)
    # non-contiguous scores: a transposed [n, C] matrix and a strided slice
    t = kendall_tau(d_x.t().contiguous().t(), d_y, return_counts=True)
    assert not d_x.t().contiguous().t().is_contiguous() and np.array_equal(t['counts'].cpu().numpy(), want_c)
    wide = torch.full((3, 2 * 257), float('nan'), device='cuda')
    wide[:, ::2] = d_x
    s = kendall_tau(wide[:, ::2], d_y, return_counts=True)
    assert np.array_equal(s['counts'].cpu().numpy(), want_c) and torch.equal(s['tau_b'], res['tau_b']) and torch.equal(s['tau_c'], res['tau_c'])
    with pytest.raises(ValueError, match='device tensors'):
        kendall_tau(d_x, torch.from_numpy(y))


# ---- 5. reporting sizes --------------------------------------------------------------------------------------------------------------
def _check_large(x, y):
    """counts against np.unique multiplicities (slots 2 to 6) and, for con and dis, the two exact integers SciPy's tau_b pins down:
    con + dis = n0 - tie_x - tie_y + tie_xy by the identity, and con - dis = tau_b sqrt(n0 - tie_x) sqrt(n0 - tie_y), an integer that
    the double quotient determines to far better than 1/2 (|con - dis| <= 3.5e10, relative rounding 1e-15)"""
    C, n = x.shape
    n0 = n * (n - 1) // 2
    cnt, tau = raw(x, y)
    sp = kc.scipy_taus(x, y)
    assert kc.tau_close(tau, sp), (tau, sp)
    ty, dy = kc.tie_counts(y), kc.distinct(y)
    for c in range(C):
        tx, txy, dx = kc.tie_counts(x[c]), kc.joint_tie_counts(x[c], y), kc.distinct(x[c])
        assert cnt[c, 2:].tolist() == [tx, ty, txy, dx, dy, 0], c
        cmd = sp[c, 0] * np.sqrt(float(n0 - tx)) * np.sqrt(float(n0 - ty))
        assert abs(cmd - round(cmd)) < 1e-3, cmd
        total = n0 - tx - ty + txy
        assert (total + round(cmd)) % 2 == 0
        assert cnt[c, :2].tolist() == [(total + round(cmd)) // 2, (total - round(cmd)) // 2], c
    return cnt, tau


def test_flickr8k_expert_size():
    x, y = kc.report_case()
    assert x.shape == (3, 16992)
    cnt, tau = _check_large(x, y)
    assert (cnt[:, 2] >= 5664 * 3).all() and (np.abs(tau) < 1).all() and (tau[:, 0] > 0.1).all()
    print(f'n=16992 C=3: tau_b {tau[:, 0]}, tau_c {tau[:, 1]}')


def test_the_cap_on_n():
    """n = 262 144: n0 = 3.4e10 pairs does not fit 32 bits, and the 4 096 workgroups are not all resident at once"""
    n = kc.MAX_N
    r = np.random.RandomState(9)
    level = r.randint(0, 4, size=n)
    x = np.stack([r.randn(n) + level, np.round(2 * r.randn(n) + level)]).astype(np.float32)
    cnt, tau = _check_large(x, (level / 3.0).astype(np.float32))
    assert cnt[0, 0] > 2 ** 33 and cnt[0, 3] > 2 ** 32 and cnt[1, 2] > 2 ** 31


# ---- 6. the evaluator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('annotators', (None, 3))
@pytest.mark.parametrize('with_refs', (False, True))
def test_evaluator_end_to_end(with_refs, annotators):
    from test_clipscore_gpu import SB, SK, SCOUNTS, _inputs, _students
    from distillclip_amd import HumanCorrelation, LCLIPScore
    from distillclip_amd.metrics import kendall_tau
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    modules = list(clip.modules())
    before = {n: p.detach().clone() for n, p in clip.named_parameters()}
    flags = [p.requires_grad for p in clip.parameters()], [m.training for m in modules]
    hc = HumanCorrelation.from_model(clip, max_batch=4)
    assert isinstance(hc.scorer, LCLIPScore) and torch.is_grad_enabled()
    g = torch.Generator().manual_seed(17)
    batches, direct, ratings = [], [], []
    for b in range(2):
        images, cand, refs = _inputs(40 + 2 * b)
        if not with_refs:
            cand = cand[:, b].contiguous()                                                # [B, L]: one candidate per image
        shape = tuple(cand.shape[:-1]) + (() if annotators is None else (annotators,))
        human = torch.randint(1, 5, shape, generator=g)                                   # integer ratings, on the host for batch 0
        human = human if b == 0 else human.float().cuda()
        args = (refs, SCOUNTS) if with_refs else ()
        batches.append((images, cand, human) + args)
        out = hc.scorer(images, cand, *args)
        direct.append([None if s is None else s.reshape(-1) if annotators is None else s.reshape(-1).repeat_interleave(annotators)
                       for s in out])
        ratings.append(human.reshape(-1).float().cuda())
    for batch in batches:
        hc.update(*batch)
    got = hc.compute(return_counts=True)
    names = ('clip_s', 'ref_s', 'refclip_s') if with_refs else ('clip_s',)
    assert set(got) == {f'{m}_{k}' for m in names for k in ('tau_b', 'tau_c', 'counts')}
    scores = torch.stack([torch.cat([d[c] for d in direct]) for c in range(len(names))])
    n = SB * (SK if with_refs else 1) * (annotators or 1) * 2
    assert scores.shape == (len(names), n)
    want = kendall_tau(scores, torch.cat(ratings), return_counts=True)
    for c, m in enumerate(names):
        for k in ('tau_b', 'tau_c', 'counts'):
            assert torch.equal(got[f'{m}_{k}'], want[k][c]), (m, k)
        assert got[f'{m}_tau_b'].dim() == 0 and got[f'{m}_tau_b'].dtype == torch.float64 and not got[f'{m}_tau_b'].requires_grad
    ref_c, ref_t = kc.reference(scores.cpu().numpy(), torch.cat(ratings).cpu().numpy())
    assert np.array_equal(want['counts'].cpu().numpy(), ref_c)
    assert kc.tau_close(torch.stack([want['tau_b'], want['tau_c']], dim=1).cpu().numpy(), ref_t)
    if annotators:
        assert (want['counts'][0, 2] >= n // annotators * 3).item()                       # every score three times: ties in x
    assert set(hc.compute()) == {f'{m}_{k}' for m in names for k in ('tau_b', 'tau_c')}
    # flat vectors formed elsewhere give the same bits
    hc2 = HumanCorrelation(hc.scorer)
    for d, h in zip(direct, ratings):
        hc2.add_scores(h, *d) if with_refs else hc2.add_scores(h, d[0])
    also = hc2.compute(return_counts=True)
    assert set(also) == set(got) and all(torch.equal(also[k], got[k]) for k in got)
    with pytest.raises(ValueError, match='cannot be mixed'):
        hc2.add_scores(ratings[0], direct[0][0]) if with_refs else hc2.add_scores(ratings[0], direct[0][0], direct[0][0], direct[0][0])
    # reset() forgets everything
    hc.reset()
    with pytest.raises(ValueError, match='0 rated items'):
        hc.compute()
    hc.update(*batches[1])
    assert hc._n == n // 2 and set(hc.compute()) == {f'{m}_{k}' for m in names for k in ('tau_b', 'tau_c')}
    # nothing of the towers changed
    for name, p in clip.named_parameters():
        assert torch.equal(p.detach(), before[name]) and p.grad is None, name
    assert [p.requires_grad for p in clip.parameters()] == flags[0] and [m.training for m in modules] == flags[1]
