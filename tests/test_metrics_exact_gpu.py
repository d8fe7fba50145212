"""The validation-metrics kernel on the GPU (dclip_retrieval_metrics, csrc/metrics.hip; metrics.retrieval_metrics), row by row against
float64: exact ranks and accuracies on planted cases and under ties, ranks as float64 intervals on random operands, the per-row
intermediates of the workspace (normalised rows, diagonal, sum of exponentials) and the finalize step each against its own bound,
guards around every buffer, determinism, power-of-two scales, zero rows, refusals that write nothing, and the Python wrapper.
Cases, bounds and the float64 references live in tests/metrics_cases.py; tests/test_metrics_exact_cpu.py checks the cases themselves.

Every raw call goes through `Call`: each buffer starts as all-ones bits (f32 NaN, int32 -1) with PAD guard elements on both sides, the
workspace is exactly dclip_retrieval_metrics_workspace(n, E) bytes inside such a buffer, and after the call every guard, the slack after
each workspace piece and the inputs are compared bit for bit.

Out of scope: n >= 2^24 (the entry admits n < 2^30, but the hit counts are summed in f32 there); such a case cannot run in seconds."""
import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_cases as mc
import recall_cases as rc

pytestmark = pytest.mark.gpu

PAD = 64                                             # guard elements (256 bytes) before and after every buffer
U = mc.U
WORST = {}                                           # what -> worst err / bound of this process
RESIDUAL = {}                                        # what -> worst (relative error of sexp - derived terms) / u


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _note(what, err, bound):
    q = float(np.max(np.asarray(err, dtype=np.float64) / bound)) if np.size(err) else 0.0
    WORST[what] = max(WORST.get(what, 0.0), q if q == q else math.inf)
    return q


def _ones(count):
    return torch.full((count,), -1, dtype=torch.int32, device='cuda')


def _guarded(values):
    """f32 / i32 CPU tensor -> all-ones int32 device buffer with the values' bits behind PAD guard elements"""
    flat = values.contiguous().view(torch.int32).reshape(-1)
    buf = _ones(2 * PAD + flat.numel())
    buf[PAD:PAD + flat.numel()] = flat.cuda()
    return buf


class Call:
    """One raw call of dclip_retrieval_metrics.  `how` holds the overrides of the refusal tests: an argument to pass instead (n, E, nk, ks),
    None or a byte skew for a pointer (img, txt, out, ws), ws_short bytes less than the workspace.
    -> .status, .error, .out f32 [nk + 2], .out_bits, .rank i32 [n] (None without rank_out), .ws {piece: array}, .untouched"""

    def __init__(self, img, txt, ks, ranks=True, how=None):
        l = _lib()
        kw = how or {}
        g = lambda name, default: kw[name] if name in kw else default
        self.n, self.E, self.ks = img.shape[0], img.shape[1], tuple(int(k) for k in ks)
        n, E, nk = g('n', self.n), g('E', self.E), g('nk', len(self.ks))
        self.nlive = len(self.ks) + 2
        self.img_buf, self.txt_buf = _guarded(img), _guarded(txt)
        self.img_bits, self.txt_bits = self.img_buf.clone(), self.txt_buf.clone()
        self.out_buf, self.rank_buf = _ones(2 * PAD + self.nlive), _ones(2 * PAD + self.n)
        self.need = l.dclip_retrieval_metrics_workspace(self.n, self.E)
        self.pieces, total = mc.workspace_layout(self.n, self.E, self.need)
        self.ws_buf = torch.full((4 * PAD + total + 4 * PAD,), 0xFF, dtype=torch.uint8, device='cuda')
        karr = (ctypes.c_int32 * 16)(*(self.ks + (0,) * (16 - len(self.ks))))
        at = lambda t, key: None if g(key, 0) is None else t.data_ptr() + PAD * 4 + g(key, 0)
        torch.cuda.synchronize()
        self.status = l._dll.dclip_retrieval_metrics(at(self.img_buf, 'img'), at(self.txt_buf, 'txt'), n, E, g('ks', karr), nk,
                                                     at(self.out_buf, 'out'), at(self.rank_buf, 'rank') if ranks else None,
                                                     at(self.ws_buf, 'ws'), total - g('ws_short', 0), torch.cuda.current_stream().cuda_stream)
        self.error = l._dll.dclip_last_error_string().decode() if self.status else ''
        torch.cuda.synchronize()
        out, rank, ws = self.out_buf.cpu().numpy(), self.rank_buf.cpu().numpy(), self.ws_buf.cpu().numpy()
        self.untouched = bool((out == -1).all() and (rank == -1).all() and (ws == 0xFF).all())
        assert torch.equal(self.img_buf, self.img_bits) and torch.equal(self.txt_buf, self.txt_bits), 'an input was written'
        if self.status:
            return
        # guards and slack: nothing outside out[0 .. nk + 2), rank_out[0 .. n) and the live part of the five workspace pieces
        assert (out[:PAD] == -1).all() and (out[PAD + self.nlive:] == -1).all(), 'out guard'
        assert (rank[:PAD] == -1).all() and (rank[PAD + self.n:] == -1).all(), 'rank_out guard'
        assert ranks or (rank == -1).all(), 'rank_out = NULL, yet ranks were written'
        live = np.zeros(ws.size, dtype=bool)
        self.ws = {}
        for name, (off, nbytes, dtype, shape) in self.pieces.items():
            live[4 * PAD + off:4 * PAD + off + nbytes] = True
            self.ws[name] = ws[4 * PAD + off:4 * PAD + off + nbytes].view(dtype).reshape(shape).copy()
        assert (ws[~live] == 0xFF).all(), f'workspace bytes outside the five pieces: {np.nonzero((ws != 0xFF) & ~live)[0][:8] - 4 * PAD}'
        self.out_bits = out[PAD:PAD + self.nlive].copy()
        self.out = self.out_bits.view(np.float32)
        self.rank = rank[PAD:PAD + self.n].copy() if ranks else None
        assert ranks is False or np.array_equal(self.rank, self.ws['rank']), 'rank_out is no copy of the ranks'

    def same_bits(self, other):
        return np.array_equal(self.out_bits, other.out_bits) and all(
            np.array_equal(self.ws[k].view(np.int32), other.ws[k].view(np.int32)) for k in self.ws)


def check_accuracies(c):
    """out[0 .. nk) is exactly float32(hits) / float32(n) of the kernel's own ranks"""
    want = mc.expected_acc(c.ws['rank'], c.ks)
    assert np.array_equal(c.out[:len(c.ks)].view(np.int32), want.view(np.int32)), (c.out[:len(c.ks)], want)


def check_numbers(c, img, txt, L, logit_bound, what):
    """section 4 of the module docstring of metrics_cases.py: every intermediate against float64 within its derived bound"""
    n, E, nk = c.n, c.E, len(c.ks)
    # normalised rows
    norm_rel = (E / 2 + 3) * U
    for name, x in (('nimg', img), ('ntxt', txt)):
        ref = mc.unit_rows64(x)
        err = np.abs(c.ws[name].astype(np.float64) - ref)
        assert (err <= norm_rel * np.abs(ref)).all(), (what, name, float((err / np.maximum(np.abs(ref), 1e-300)).max() / U))
        nz = ref != 0
        _note('normalised rows', err[nz] / np.abs(ref[nz]), norm_rel)
    # diagonal
    sexp64, soft64, diag64 = mc.scores64(L)
    diag = c.ws['diag'].astype(np.float64)
    q = _note('diag', np.abs(diag - diag64), logit_bound)
    assert q <= 1, (what, 'diag', q)
    # sum of exponentials, relative
    sexp = c.ws['sexp'].astype(np.float64)
    rel = np.abs(sexp - sexp64) / sexp64
    derived = mc.sexp_terms(n, E, logit_bound)
    RESIDUAL[what.split(' ')[0]] = max(RESIDUAL.get(what.split(' ')[0], -math.inf), float((rel - derived).max() / U))
    q = _note('sexp', rel, derived + mc.EXP_REL)
    assert q <= 1, (what, 'sexp', q, float(rel.max() / U))
    # finalize alone: the two scores from the kernel's own per-row results
    fin = mc.finalize_factor(n)
    soft_own = np.exp(diag - 1.0) / sexp
    for idx, terms, name in ((nk, soft_own, 'softmax_mean_score'), (nk + 1, diag, 'mean_score')):
        q = _note(f'finalize {name}', abs(float(c.out[idx]) - terms.mean()), fin * np.abs(terms).mean())
        assert q <= 1, (what, 'finalize', name, q)
    check_accuracies(c)
    # end to end, the composed bounds.  A softmax term is __expf(d - 1) / sexp: the numerator carries the diagonal's logit error and
    # EXP_REL, the denominator sexp's whole bound, the division one u; the finalize step then adds its share of the (positive) terms'
    # mean.  A diagonal is off by the logit bound, and the finalize step adds its share of the mean of |diagonal|.
    num, den = math.expm1(logit_bound) + mc.EXP_REL, derived + mc.EXP_REL
    term_rel = (1 + num) * (1 + U) / (1 - den) - 1
    b_soft = soft64.mean() * term_rel * (1 + fin) + fin * soft64.mean()
    b_diag = logit_bound * (1 + fin) + fin * np.abs(diag64).mean()
    off_soft, off_diag = abs(float(c.out[nk]) - soft64.mean()), abs(float(c.out[nk + 1]) - diag64.mean())
    q1 = _note('end to end softmax_mean_score', off_soft, b_soft)
    q2 = _note('end to end mean_score', off_diag, b_diag)
    print(f'{what}: softmax_mean_score off {off_soft:.3e} (bound {b_soft:.3e}), mean_score off {off_diag:.3e} (bound {b_diag:.3e}), '
          f'sexp worst {rel.max() / U:.2f} u of {(derived + mc.EXP_REL) / U:.0f} u')
    assert q1 <= 1 and q2 <= 1, (what, 'end to end', q1, q2)


# ---- 1. planted ranks and scores, exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E', mc.PLANTED_SIZES)
def test_planted_ranks_and_accuracies_are_exact(n, E):
    rows, cols, r, chosen, swapped = mc.planted_square(n, E)
    L = mc.planted_logits(r, chosen)
    first = None
    for ks in mc.k_lists(n):
        c = Call(rows, cols, ks)
        assert c.status == 0, c.error
        assert np.array_equal(c.rank, r.astype(np.int32)), np.nonzero(c.rank != r)[0][:8]
        want = mc.expected_acc(r, ks)
        assert np.array_equal(c.out[:len(ks)].view(np.int32), want.view(np.int32)), (ks, c.out, want)
        if len(ks) == 8:
            assert c.out[3] == 1.0 and c.out[4] == 1.0                       # a cut-off above n, and n itself
        check_numbers(c, rows, cols, L, 4 * U, f'planted ({n}, {E}) nk={len(ks)}')
        # rank_out = NULL: the same bits in out and in the workspace, and no rank written anywhere (Call asserts that)
        c0 = Call(rows, cols, ks, ranks=False)
        assert c0.status == 0 and c0.rank is None and c0.same_bits(c)
        # the per-row results do not depend on the cut-offs
        first = first or c
        assert all(np.array_equal(c.ws[k].view(np.int32), first.ws[k].view(np.int32)) for k in c.ws)
        assert np.array_equal(c.out_bits[len(ks):], first.out_bits[len(first.ks):])


@pytest.mark.parametrize('n,E', mc.PLANTED_SIZES)
def test_planted_ranks_with_the_roles_swapped(n, E):
    """one-hot rows against planted columns: closed-form ranks again; the clamped rows of the last panel meet every column"""
    rows, cols, r, chosen, swapped = mc.planted_square(n, E)
    ks = mc.k_lists(n)[1]
    c = Call(cols, rows, ks)
    assert c.status == 0, c.error
    assert np.array_equal(c.rank, swapped.astype(np.int32)), np.nonzero(c.rank != swapped)[0][:8]
    assert np.array_equal(c.out[:8].view(np.int32), mc.expected_acc(swapped, ks).view(np.int32))
    check_numbers(c, cols, rows, mc.planted_logits(r, chosen).T, 4 * U, f'swapped ({n}, {E})')


# ---- 2. ties, against the truth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n0,E', mc.TIE_SIZES)
def test_ties_count_for_the_diagonal(n0, E):
    """the planted case twice (metrics_cases.tied_square): every rank is 2 r, one counted tie would give 2 r + 1.  The bit-equality of
    the dot products of bit-equal rows is the documented property of dot_tile (csrc/sim_tiles.h)."""
    rows, cols, want = mc.tied_square(n0, E)
    ks = (1, 2, 3, 2 * n0 - 2, 2 * n0 - 1)
    c = Call(rows, cols, ks)
    assert c.status == 0, c.error
    assert np.array_equal(c.rank, want.astype(np.int32)), (np.nonzero(c.rank != want)[0][:8], c.rank[:8], want[:8])
    assert np.array_equal(c.out[:5].view(np.int32), mc.expected_acc(want, ks).view(np.int32))
    assert c.out[0] == np.float32(2) / np.float32(2 * n0) and c.out[1] == c.out[0] and c.out[4] == 1.0
    # the two halves are bit copies of each other in every per-row result
    for k in ('rank', 'sexp', 'diag'):
        assert np.array_equal(c.ws[k][:n0].view(np.int32), c.ws[k][n0:].view(np.int32)), k


# ---- 3. ranks as float64 intervals on random operands ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E,corr,seed', mc.random_cases())
def test_ranks_lie_in_the_float64_intervals(n, E, corr, seed):
    img, txt, L, (lo, hi) = mc.reference(n, E, corr, seed)
    assert int((hi > lo).sum()) <= max(1, int(mc.UNDECIDED_CAP * n))         # a condition on the case, not a measurement
    c = Call(img, txt, mc.K_DEFAULT)
    assert c.status == 0, c.error
    bad = np.nonzero((c.rank < lo) | (c.rank > hi))[0]
    assert bad.size == 0, (bad[:8], c.rank[bad[:8]], lo[bad[:8]], hi[bad[:8]])
    check_numbers(c, img, txt, L, rc.bound(E), f'random ({n}, {E}) corr {corr} seed {seed}')


@pytest.mark.parametrize('n,E,corr', [(130, 64, 0.05), (257, 16, 0.05), (65, 512, 0.25)])
def test_permuting_the_pairs_permutes_the_ranks(n, E, corr):
    seed = mc.OTHER_SEEDS.get((n, E, corr), mc.SEEDS)[0]
    img, txt, _, _ = mc.reference(n, E, corr, seed)
    c = Call(img, txt, mc.K_DEFAULT)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n))
    p = Call(img[perm], txt[perm], mc.K_DEFAULT)
    assert c.status == 0 and p.status == 0
    for k in ('rank', 'diag'):                           # functions of the row and of the SET of columns (sexp adds in column order)
        assert np.array_equal(p.ws[k].view(np.int32), c.ws[k][perm.numpy()].view(np.int32)), k
    assert np.array_equal(p.out_bits[:6], c.out_bits[:6])
    assert corr > 0.1 or c.rank.max() > n // 2


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E,corr', [(257, 1024, 0.25), (130, 64, 0.05), (17, 16, 0.05)])
def test_same_call_same_bits(n, E, corr):
    seed = mc.OTHER_SEEDS.get((n, E, corr), mc.SEEDS)[0]
    img, txt, _, _ = mc.reference(n, E, corr, seed)
    a, b = Call(img, txt, mc.K_DEFAULT), Call(img, txt, mc.K_DEFAULT)        # each on a fresh all-ones workspace
    assert a.status == 0 and b.status == 0 and a.same_bits(b) and np.array_equal(a.rank, b.rank)


# ---- 5. the error of __expf, measured ------------------------------------------------------------------------------------------------------
def test_expf_error_measured_on_single_rows():
    """An n = 1 problem's sexp is the single term __expf(S - 1.f) of its diagonal S, with nothing added to it but zeros: against float64
    exp of the kernel's own f32 diagonal it shows the error of that expression alone.  2049 problems whose cosine runs from 1 to -1;
    one launch sequence each, one wait for all.  EXP_REL of metrics_cases.py is four times the worst figure printed here, rounded up
    to a power of two times u."""
    l = _lib()
    m, E = 2049, 16
    theta = torch.linspace(0, math.pi, m, dtype=torch.float64)
    img = torch.zeros(m, E)
    img[:, 0] = 1.0
    txt = torch.zeros(m, E)
    txt[:, 0], txt[:, 1] = theta.cos().float(), theta.sin().float()
    d_img, d_txt = img.cuda(), txt.cuda()
    need = l.dclip_retrieval_metrics_workspace(1, E)
    pieces, total = mc.workspace_layout(1, E, need)
    ws = torch.full((m, total), 0xFF, dtype=torch.uint8, device='cuda')
    out = _ones(2 * m).view(m, 2)
    for i in range(m):
        l.dclip_retrieval_metrics(d_img[i].data_ptr(), d_txt[i].data_ptr(), 1, E, None, 0, out[i].data_ptr(), None, ws[i].data_ptr(), total,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ws = ws.cpu().numpy()
    piece = lambda name: np.ascontiguousarray(ws[:, pieces[name][0]:pieces[name][0] + 4]).view(pieces[name][2])[:, 0]
    diag, sexp, rank = piece('diag').astype(np.float64), piece('sexp').astype(np.float64), piece('rank')
    assert (rank == 0).all() and np.isfinite(diag).all() and diag.max() == 1.0 and diag.min() <= -0.999999
    rel = np.abs(sexp - np.exp(diag - 1.0)) / np.exp(diag - 1.0)
    RESIDUAL['single rows (__expf alone)'] = float(rel.max() / U)
    print(f'__expf(S - 1) over {m} single rows: worst relative error {rel.max() / U:.3f} u at S = {diag[rel.argmax()]:.6f}, '
          f'mean {rel.mean() / U:.3f} u; EXP_REL = {mc.EXP_REL / U:.0f} u')
    assert _note('__expf(S - 1) alone', rel, mc.EXP_REL) <= 1
    # finalize on one row: softmax of a single logit is 1 up to the division, the mean is the logit
    o = out.cpu().numpy().view(np.float32)
    assert (np.abs(o[:, 0] - 1.0) <= 2 * U).all() and np.array_equal(o[:, 1], piece('diag'))


# ---- 6. scales, zero rows, refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E,corr,seed', [(33, 64, 0.05, 0), (130, 512, 0.25, 1), (257, 16, 0.05, 2)])
def test_power_of_two_row_scales_change_no_bit(n, E, corr, seed):
    img, txt, _, _ = mc.reference(n, E, corr, seed)
    base = Call(img, txt, mc.K_DEFAULT)
    scaled = Call(mc.power_of_two_scales(img, 11), mc.power_of_two_scales(txt, 12), mc.K_DEFAULT)
    assert base.status == 0 and scaled.status == 0
    assert np.array_equal(base.rank, scaled.rank) and scaled.same_bits(base)  # ranks, both scores, and the normalised rows themselves


def test_a_zero_image_row_gives_nan_scores_and_leaves_the_other_ranks():
    """include/dclip.h: rows are divided by their norm without an epsilon, so a zero row becomes NaN.  Pinned here: both scores are NaN, the
    accuracies stay finite and exact, the zero row itself has rank 0 (a NaN diagonal is beaten by nothing), every other row keeps the
    rank it has when row i is not zero (its columns are untouched)."""
    rows, cols, r, _, _ = mc.planted_square(65, 80)
    ks = mc.K_DEFAULT
    for i in (0, 37, 64):
        z = rows.clone()
        z[i] = 0
        c = Call(z, cols, ks)
        assert c.status == 0, c.error
        assert np.isnan(c.out[6]) and np.isnan(c.out[7])
        want = r.copy()
        want[i] = 0
        assert np.array_equal(c.rank, want.astype(np.int32))
        assert np.array_equal(c.out[:6].view(np.int32), mc.expected_acc(want, ks).view(np.int32))
        others = np.arange(65) != i
        assert np.isnan(c.ws['sexp'][i]) and np.isnan(c.ws['diag'][i]) and np.isnan(c.ws['nimg'][i]).all()
        assert np.isfinite(c.ws['sexp'][others]).all() and np.isfinite(c.ws['diag'][others]).all()


def test_a_zero_caption_row_gives_nan_scores_and_counts_for_no_row():
    """A zero caption row j is NaN after the normalisation, and so is column j of the logits: it is in every row's sum of exponentials, so
    both scores are NaN, and every row's sexp is NaN.  The ranks, pinned here: a NaN logit is ahead of nothing, so column j counts for no
    row (rank_c = r_c less one where j was among row c's chosen columns), and row j, whose diagonal is NaN, has rank 0."""
    rows, cols, r, chosen, _ = mc.planted_square(65, 80)
    ks = mc.K_DEFAULT
    for j in (3, 64):
        z = cols.clone()
        z[j] = 0
        c = Call(rows, z, ks)
        assert c.status == 0, c.error
        assert np.isnan(c.out[6]) and np.isnan(c.out[7])
        want = r - chosen[:, j]
        want[j] = 0
        assert chosen[:, j].sum() > 3
        assert np.array_equal(c.rank, want.astype(np.int32)), np.nonzero(c.rank != want)[0][:8]
        assert np.array_equal(c.out[:6].view(np.int32), mc.expected_acc(want, ks).view(np.int32))
        assert np.isnan(c.ws['sexp']).all() and np.isnan(c.ws['diag'][j]) and np.isfinite(np.delete(c.ws['diag'], j)).all()


REFUSALS = [
    (dict(img=None), 'null'), (dict(txt=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'),
    (dict(n=0), '0 < n'), (dict(E=0), 'multiple of 16'), (dict(E=8), 'multiple of 16'), (dict(E=24), 'multiple of 16'),
    (dict(nk=-1), 'cut-offs'), (dict(nk=9), 'cut-offs'), (dict(nk=2, ks=None), 'cut-offs'),
    (dict(ws_short=1), 'workspace too small'),
    (dict(img=4), '16-byte aligned'), (dict(txt=4), '16-byte aligned'), (dict(ws=4), '16-byte aligned'),
]


@pytest.mark.parametrize('kw,word', REFUSALS, ids=['-'.join(f'{a}={b}' for a, b in kw.items()) for kw, _ in REFUSALS])
def test_a_refused_call_writes_nothing(kw, word):
    img, txt, _, _ = mc.reference(33, 64, 0.25, 0)
    c = Call(img, txt, (1, 5, 10), how=kw)
    assert c.status != 0 and word in c.error and 'dclip_retrieval_metrics' in c.error, (c.status, c.error)
    assert c.untouched                                                       # out, rank_out and the workspace, guards included: all-ones still
    q = _lib().dclip_retrieval_metrics_workspace
    assert q(0, 64) == 0 and q(-3, 64) == 0 and q(33, 0) == 0 and q(33, -16) == 0
    good = Call(img, txt, (1, 5, 10))                                        # and the next well-formed call is served
    assert good.status == 0 and not good.untouched


# ---- 7. the Python wrapper -----------------------------------------------------------------------------------------------------------------
def _wrapped(rows, cols, ks=mc.K_DEFAULT):
    from distillclip_amd.metrics import retrieval_metrics
    res = retrieval_metrics(rows, cols, ks, return_ranks=True)
    vals = [res[f'acc_top{k}'] for k in ks] + [res['softmax_mean_score'], res['mean_score']]
    assert set(res) == {f'acc_top{k}' for k in ks} | {'softmax_mean_score', 'mean_score', 'ranks'}
    assert all(v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 for v in vals)
    assert len({v.untyped_storage().data_ptr() for v in vals}) == 1          # 0-dim views of one result vector
    assert [v.storage_offset() for v in vals] == list(range(len(ks) + 2))
    return torch.stack(vals).cpu().numpy().view(np.int32), res['ranks'].cpu().numpy()


def test_wrapper_equals_the_raw_call():
    from distillclip_amd.metrics import retrieval_metrics
    img, txt, _, _ = mc.reference(65, 64, 0.05, 0)
    raw = Call(img, txt, mc.K_DEFAULT)
    out, ranks = _wrapped(img.cuda(), txt.cuda())
    assert np.array_equal(out, raw.out_bits) and np.array_equal(ranks, raw.rank)
    res = retrieval_metrics(img.cuda(), txt.cuda())                          # the default path, rank_out = NULL: the same figures
    assert 'ranks' not in res and len(res) == 8
    assert np.array_equal(torch.stack(list(res.values())).cpu().numpy().view(np.int32), raw.out_bits)
    none = retrieval_metrics(img.cuda(), txt.cuda(), ())
    assert list(none) == ['softmax_mean_score', 'mean_score'] and none['mean_score'].item() == raw.out[7]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float64])
def test_wrapper_takes_other_dtypes_as_their_float_copies(dtype):
    img, txt, _, _ = mc.reference(65, 64, 0.05, 0)
    a, b = img.cuda().to(dtype), txt.cuda().to(dtype)
    got, want = _wrapped(a, b), _wrapped(a.float(), b.float())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    raw = Call(a.float().cpu(), b.float().cpu(), mc.K_DEFAULT)
    assert np.array_equal(got[0], raw.out_bits) and np.array_equal(got[1], raw.rank)


def test_wrapper_takes_views_as_their_contiguous_copies():
    img, txt, _, _ = mc.reference(65, 64, 0.05, 0)
    want = _wrapped(img.cuda(), txt.cuda())
    wide = torch.full((65, 200), float('nan'), device='cuda')
    wide[:, 70:134] = img.cuda()
    tall = torch.full((64, 65), float('nan'), device='cuda')
    tall.copy_(txt.cuda().t())
    a, b = wide[:, 70:134], tall.t()                                         # a column slice of a wider tensor, a transposed storage
    assert not a.is_contiguous() and not b.is_contiguous()
    got = _wrapped(a, b)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert torch.isnan(wide[:, :70]).all() and torch.isnan(wide[:, 134:]).all()


def test_wrapper_refuses_nine_cutoffs_before_any_launch():
    from distillclip_amd.metrics import retrieval_metrics
    img, txt, _, _ = mc.reference(33, 64, 0.25, 0)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='cut-offs'):
        retrieval_metrics(img.cuda(), txt.cuda(), k_list=range(1, 10))
    with pytest.raises(ValueError, match='cut-offs'):
        retrieval_metrics(img.cuda(), txt.cuda(), k_list=range(1, 10), return_ranks=True)
    torch.cuda.synchronize()                                                 # nothing was launched that could fail later
    assert _wrapped(img.cuda(), txt.cuda())[1].shape == (33,)


# ---- 8. the table ------------------------------------------------------------------------------------------------------------------------------
def test_worst_ratios_of_this_run():
    """prints what the tests above saw (run the file as a whole, with -s or -rP); every ratio is an assertion already made"""
    for k in sorted(WORST):
        print(f'worst err / bound  {k:36s} {WORST[k]:.4f}')
    for k in sorted(RESIDUAL):
        print(f'sexp: worst relative error less the derived terms, in u  {k:28s} {RESIDUAL[k]:+.3f}')
    print(f'EXP_REL = {mc.EXP_REL / U:.0f} u')
    assert all(v <= 1 for v in WORST.values()), WORST
