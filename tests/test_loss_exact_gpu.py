"""dclip_distill_loss / dclip_distill_loss_rows term by term and element by element against float64 (tests/test_loss_gpu.py compares a
mixture of 3 to 8 terms with the f32 oracle as max-error-over-max-value of the whole tensor; this file resolves one term, one row, one
element).  U24 = 2^-24.  The input builders, the float64 reference and its bounds are properties of the inputs alone: they draw with a
CPU generator (the same numbers with and without a GPU) and tests/test_loss_exact_cpu.py checks every one of them without the kernels.

The reference (`Reference`) restates the eight terms in closed form with their analytic gradients, from the definitions oracle/loss.py
cites (out_l1.py, out_cos.py, out_kl.py, out_ce.py, clip_cos_diff.py, hard_label.py, soft_label.py, logits_mse.py, clip_model.py:37-44).
a, b = student image / text rows, a^ = a / |a|, S = a^ b^T, T the same of the teacher, tw = 1/2 with two towers and 1 with one,
R_i / C_j = log-sum-exp of row i / column j.  dL/dS =: D, then G_a = D b^, G_b = D^T a^, then d a_i = (G_i - a^_i (a^_i . G_i)) / |a_i|:
  out_l1      mean |s - t|                                        d s = w tw sign(s - t) / (B E)
  out_cos     mean_i (1 - s.t / sqrt((s.s + 1e-12)(t.t + 1e-12)))  d s = -w tw (t / den - cos s / (s.s + 1e-12)) / B
  out_kl      tau^2 sum_i KL(softmax(t_i / tau) || softmax(s_i / tau))   (feature axis)      d s = w tw tau (p_s - p_t)
  out_ce      -mean_i sum_e softmax(t_i)_e log softmax(s_i)_e                                d s = w tw (p_s - p_t) / B
  cos_diff    mean_i relu(T_ii - S_ii) + mean_{i != j} relu(S_ij - T_ij)   (the same in both directions)
              D_ii = -w [T_ii > S_ii] / B,  D_ij = w [S_ij > T_ij] / (B (B - 1))
  hard_label  (mean_i (R_i - S_ii) + mean_j (C_j - S_jj)) / 2          D_ij = w (exp(S_ij - R_i) + exp(S_ij - C_j) - 2 [i = j]) / (2 B)
  soft_label  tau^2 (sum_i KL(rows of T / tau || rows of S / tau) + the same of the columns) / 2
              D_ij = w tau ((Ps^r - Pt^r) + (Ps^c - Pt^c))_ij / 2
  logits_mse  mean (S - T)^2                                        D = 2 w (S - T) / B^2

Bounds, per element, in float64: U24 times a count of roundings times the same sum with absolute values inside.
  logit       e_S = (E + 2) U24 (|a^| |b^|^T): the E-term product on the f32 MFMA and the two normalisations; e_T alike.  S / tau carries
              e_S / tau + 2 U24 |S / tau| (1 / tau and the product with it).
  exp, log    XA = 8 U24 per evaluated exp(x - lse) or log, the allowance of _loss_tol in tests/test_softmax_edges_gpu.py for __expf /
              __logf.  A log-sum-exp carries the softmax-weighted error of its inputs plus n_merge (8 + |lse|) U24: each running add,
              lane, wave and slice merge is two exps, a sum, a log (XA) and one rounding of max + log; n_merge = ceil(tiles / 4) + 15
              (the lane's running adds, its own log, 4 lane steps, 2 wave levels, at most 8 slices).
  D           e_D: e_S, e_T and the statistics' errors through the term's derivative (sum over the four probabilities p (e_x + e_lse + XA
              + U24 |x - lse|) for the softmax terms, k (e_S + e_T) for logits_mse, nothing for cos_diff but the hinge rule below).
  product     e_G = e_D |Y| + (B + 16) U24 (|D| |Y|): B accumulations of the stripe product, at most 8 slice additions, and 8 for the
              roundings of D's constants and of the normalised rows Y.
  projection  e_da = (e_G + |a^| (|a^| . e_G) + (E + 32) U24 |a^| (|a^| . |G|) + 16 U24 (|G| + |a^| |a^ . G|)) / |a|
  tower       n = E roundings of a row sum in ANY order.  (The kernel's longest chain is 4 ceil(E / 256) + 6 additions; the f32 oracle
              on the CPU runs longer ones and loses every term below half an ulp of its running sum -- 25 U24 on the softmax
              denominator of a row of E = 1024 with one dominant feature -- so the shorter count would not hold for it.)
              out_l1: 4 U24 |g| (the sign is exact).
              out_cos: the error of s.t is n U24 sum |s t|, carried through cos and the two quotients.  out_kl / out_ce: a feature logit
              (s - max) / tau carries 3 U24 of itself, its log-sum-exp the weighted error plus (n + 8) U24 + U24 |lse|; a probability
              carries 2^-126 on top (rows of norm 12 put features 200 below the row maximum at tau = 0.5: a denormal or 0 in f32).
  hinge       a pair with |S - T| <= e_S + e_T is undecided: either branch is allowed and its k |y^_j| is added to the bound of the rows
              it touches.  At most 0.5 % of a case's pairs are undecided and 90 % of each tower's rows have none (asserted on the CPU,
              the seed is redrawn until both hold).
  scalars     slot = sum of per-row values; bound = n_acc U24 sum |terms| + the rows' own errors + 4 U24 |slot|; n_acc is the longest
              chain of additions: the wave's sum, one atomic per wave into a replica, the 64 replicas (`Reference.share`).
  total       sum |weight| bound(slot) + 16 U24 sum |weight slot| against the float64 total, and against the kernel's own slots.
No constant in these bounds was measured.  tests/test_loss_exact_cpu.py asserts that oracle.LossOracle evaluated in float32 on the CPU
stays within HALF of every bound (the hinge allowance apart) at every case: the kernel has a factor 2 over an honest f32 evaluation
for its other summation order and the hardware exp / log.

Cases.  B in {1, 2, 15, 16, 17, 33, 40, 130} at E = 48 and 768, every E in {16, 48, 64, 256, 272, 512, 528, 768, 1024} at B = 17 and
130: every instantiation of loss_rows_kernel with its last float4 chunk full and partly filled, and E = 16 where three of the stripe
kernel's four waves have no slab of the gradient product.  Column slices (`loss_slices`, the host code's rule, asserted on the CPU):
B <= 16: 1 tile, 1 slice; B = 17: 2 tiles, 2 slices, ONE column in the last tile; B = 33 and 40: 3 tiles, 3 slices (last tile: 1 and 8
columns); B = 130: 9 tiles over 8 slices (the last slice has two, the last tile 2 columns), for every row block too.
Row blocks at B = 130: [0, 8), [61, 69), [61, 130), [129, 130), and [8, 61), [69, 129) to complete the partition.
Rows have their own norms over more than two decades (row scales 0.08 to 12 in every tensor with two rows or more); the columns
decay as 1 / (1 + c / 16), so the cosines are of order 0.1 at every E.

Measured on an MI355X, worst err / bound over all cases (gradient; scalar slot), also in DESIGN.md section 8:
  out_l1 0.22; 0.03   out_cos 0.12; 0.03   out_kl 0.35; 0.04   out_ce 0.33; 0.03   cos_diff 0.10; 0.05   hard_label 0.03; 0.05
  soft_label 0.01; 0.05   logits_mse 0.05; 0.05   all terms 0.06; 0.05   tower terms 0.23; 0.03   statistics 0.06   totals <= 0.05
(the scalars are accumulated atomically: their figures move in the last digit from run to run).  The f32 oracle on the CPU uses at most
0.26 of a gradient bound.  The whole file: 38 tests in 6 s.
"""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda' if torch.cuda.is_available() else 'cpu'
U24 = 2.0 ** -24
XA = 8 * U24                                        # __expf / __logf allowance (tests/test_softmax_edges_gpu.py::_loss_tol)
TINY = 2.0 ** -126                                   # below it an f32 exp is a denormal or flushed to zero: absolute, not relative
F64 = torch.float64
NAMES = ['out_l1', 'out_cos', 'out_kl', 'out_ce', 'cos_diff', 'hard_label', 'soft_label', 'logits_mse']     # cfg order
TOWER, CROSS = NAMES[:4], NAMES[4:]
SLOT = {'out_l1': 1, 'out_cos': 2, 'out_kl': 3, 'out_ce': 4, 'cos_diff': 9, 'hard_label': 10, 'soft_label': 11, 'logits_mse': 12}
B_LIST = (1, 2, 15, 16, 17, 33, 40, 130)
E_LIST = (16, 48, 64, 256, 272, 512, 528, 768, 1024)
SWEEP = sorted({(B, E) for B in (17, 130) for E in E_LIST} | {(B, E) for B in B_LIST for E in (48, 768)})
BLOCKS = ((0, 8), (61, 8), (61, 69), (129, 1))       # (row0, rows) the issue names
PARTITION = ((0, 8), (8, 53), (61, 8), (69, 60), (129, 1))
BLOCK_E = (48, 768)
W_ALL = dict(out_l1=0.5, out_cos=1.5, out_kl=0.25, out_ce=0.75, cos_diff=0.125, hard_label=2.0, soft_label=0.375, logits_mse=1.25)     # exact in f32
PAD_FRONT, PAD_BACK = 4, 64                          # floats around every tensor: 16 bytes in front, so never 256-byte aligned
WS_GUARD = 4096
NREP = 64                                            # replicated scalar accumulators of loss.hip


class Cfg:
    """weights {term: w}, temperature, one or two towers"""

    def __init__(self, weights, tau=None, two=True):
        self.w = {n: float(weights.get(n, 0.0)) for n in NAMES}
        self.tau, self.two = tau, two
        self.cross = two and any(self.w[n] != 0 for n in CROSS)
        self.key = (tuple(self.w[n] for n in NAMES), tau, two)

    @property
    def what(self):
        on = '+'.join(f'{n}*{w:g}' for n, w in self.w.items() if w)
        return f'{on} tau={self.tau} {"two" if self.two else "one"}-tower'

    def array(self):
        return (ctypes.c_float * 10)(*[self.w[n] for n in NAMES], float(self.tau or 0.0), 1.0 if self.two else 0.0)


def configs():
    """each term alone with weight 1 (temperature terms at tau 0.5 and 2), the tower terms also with one tower, all terms with unequal
    weights, and the tower terms alone with two towers (the loss_total_kernel path)"""
    out = []
    for two in (True, False):
        for n in (NAMES if two else TOWER):
            for tau in ((0.5, 2.0) if n in ('out_kl', 'soft_label') else (None,)):
                out.append(Cfg({n: 1.0}, tau, two))
    out.append(Cfg(W_ALL, 0.5, True))
    out.append(Cfg({n: W_ALL[n] for n in TOWER}, 2.0, True))
    return out


def loss_slices(B, rows):
    """column slices of the stripe kernels, as run_distill_loss picks them (the LDS rule does not bind below B = 4096)"""
    rtile, ctile = (rows + 15) // 16, (B + 15) // 16
    return min(max(256 // (2 * rtile), 1), 8, ctile)


def slice_tiles(B, rows):
    """[(first tile, end tile)] of every column slice"""
    nt, zs = (B + 15) // 16, loss_slices(B, rows)
    return [(nt * z // zs, nt * (z + 1) // zs) for z in range(zs)]


def n_sum(E):
    """roundings of an E-term row sum in any order"""
    return E


# ----------------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------------
def _draw(B, E, seed):
    g = torch.Generator().manual_seed(seed)
    col = 1.0 / (1.0 + torch.arange(E, dtype=torch.float32) / 16)      # anisotropic like trained embeddings: ~48 effective dimensions at
    r = lambda: torch.randn(B, E, generator=g, dtype=torch.float32) * col      # any E, so |S - T| ~ 0.1 and few pairs sit on the hinge
    u = r()                                           # what an image and its caption share: the diagonal of S and T stands out
    zi, zt = u + r(), u + r()
    z = dict(si=zi, st=zt, ti=0.5 * zi + 0.3 * u + 0.7 * r(), tt=0.5 * zt + 0.3 * u + 0.7 * r())      # teacher correlated with student
    e = {}
    for k in ('si', 'ti', 'st', 'tt'):
        scale = 10.0 ** (2.2 * torch.rand(B, generator=g) - 1.1)
        if B >= 2:
            p = torch.randperm(B, generator=g)
            scale[p[0]], scale[p[1]] = 0.08, 12.0     # > two decades between two rows of every tensor
        e[k] = (z[k] * scale[:, None]).contiguous()
    return e


def hinge_counts(e):
    """(undecided pairs, image rows with one, text rows with one, pairs per branch: diag on, diag off, off-diag on, off-diag off)"""
    r = Reference(e, Cfg({'cos_diff': 1.0}))
    und, eye = r.und, torch.eye(r.B, dtype=torch.bool)
    on = torch.where(eye, r.T > r.S, r.S > r.T)
    return (int(und.sum()), int(und.any(1).sum()), int(und.any(0).sum()),
            (int((on & eye).sum()), int((~on & eye).sum()), int((on & ~eye).sum()), int((~on & ~eye).sum())))


def hinge_ok(e):
    B = e['si'].shape[0]
    n, ri, rt, _ = hinge_counts(e)
    return n <= 0.005 * B * B and ri <= 0.1 * B and rt <= 0.1 * B


@functools.lru_cache(maxsize=None)
def inputs(B, E):
    """the four f32 [B, E] tensors of a case; the seed is redrawn until the hinge caps hold (module docstring)"""
    for k in range(64):
        e = _draw(B, E, 7919 * B + E + 1000003 * k)
        if hinge_ok(e):
            return e
    raise AssertionError(f'B={B} E={E}: no seed keeps the undecided hinge pairs under their caps')


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ----------------------------------------------------------------------------------------------------------------------------------
def _wlse(x, dim, w=None):
    """log sum_j w_j exp(x_j) along dim"""
    m = x.max(dim, keepdim=True).values
    ex = torch.exp(x - m)
    if w is not None:
        ex = ex * w
    return (m + torch.log(ex.sum(dim, keepdim=True))).squeeze(dim)


def _feat_softmax(x, itau, n):
    """log-softmax over the feature axis of x * itau as loss_rows_body forms it, with the error of lp and of p"""
    arg = (x - x.max(1, keepdim=True).values) * itau
    lz = torch.logsumexp(arg, 1, keepdim=True)
    lp = arg - lz
    p = lp.exp()
    e_arg = 3 * U24 * arg.abs()
    e_lz = (p * e_arg).sum(1, keepdim=True) + (n + 8) * U24 + U24 * lz.abs()
    e_lp = e_arg + e_lz + U24 * lp.abs()
    return lp, p, e_lp, p * (e_lp + XA) + TINY


WRONGS = ('cd_b2', 'cd_swap', 'hl_rowstat', 'sl_rowstat', 'kl_scalar_tau', 'kl_grad_tau2', 'sl_scalar_tau', 'sl_grad_tau2', 'ce_no_b',
          'tower_no_half', 'last_col_twice', 'tile_lost', 'slice_lost', 'no_projection', 'neighbour_inv')


class Reference:
    """Whole-batch float64 values of one (inputs, Cfg): gradients g[tower] [B, E] with bounds gb (hinge allowance gh apart), the 12 term
    slots as per-row contributions (value, sum of |terms|, own error) so that a row block's share is a sum over its rows, the six
    statistics [6, B] with bounds.  `wrong` builds one of the wrong kernels of WRONGS instead (values only: the bounds stay those of
    the right one)."""

    def __init__(self, e32, cfg, wrong=None):
        assert wrong is None or wrong in WRONGS
        e = {k: v.to(F64) for k, v in e32.items()}
        self.cfg, self.wrong = cfg, wrong
        self.B, self.E = B, E = e['si'].shape
        self.rows_of = {}                                   # slot -> (value, abs, own) per row, slot normaliser applied
        tw = 0.5 if cfg.two and wrong != 'tower_no_half' else 1.0
        self.tw = 0.5 if cfg.two else 1.0
        self.g, self.gb, self.gh = {}, {}, {}
        for tow, (sk, tk) in enumerate((('si', 'ti'), ('st', 'tt'))[:2 if cfg.two else 1]):
            self._tower(tow, e[sk], e[tk], tw)
        self.stats = self.stats_b = None
        if cfg.two:
            self._cross(e)

    # -- tower terms ---------------------------------------------------------------------------------------------------------------
    def _tower(self, tow, s, t, tw):
        cfg, w, B, E, n = self.cfg, self.cfg.w, self.B, self.E, n_sum(self.E)
        off = 4 * tow
        d = s - t
        k = w['out_l1'] * tw / (B * E)
        g = k * torch.sign(d)
        gb = 4 * U24 * g.abs()
        a = d.abs().sum(1) / (B * E)
        self.rows_of[1 + off] = (a, a, U24 * a)

        ss, tt, st, ast = (s * s).sum(1), (t * t).sum(1), (s * t).sum(1), (s * t).abs().sum(1)
        den = torch.sqrt((ss + 1e-12) * (tt + 1e-12))
        cos = st / den
        e_cos = n * U24 * ast / den + (n + 4) * U24 * cos.abs()
        k = w['out_cos'] * tw / B
        g = g - k * (t / den[:, None] - (cos / (ss + 1e-12))[:, None] * s)
        gb = gb + abs(k) * ((n + 10) * U24 * t.abs() / den[:, None]
                            + ((e_cos + (n + 8) * U24 * cos.abs()) / (ss + 1e-12))[:, None] * s.abs())
        self.rows_of[2 + off] = ((1 - cos) / B, (1 - cos).abs() / B, (e_cos + U24) / B)

        zero = torch.zeros(B, dtype=F64)
        self.rows_of[3 + off] = self.rows_of[4 + off] = (zero, zero, zero)
        if w['out_kl'] != 0:
            tau = cfg.tau
            lps, ps, e_lps, e_ps = _feat_softmax(s, 1 / tau, n)
            lpt, pt, e_lpt, e_pt = _feat_softmax(t, 1 / tau, n)
            sc = tau if self.wrong == 'kl_scalar_tau' else tau * tau
            term = pt * (lpt - lps)
            a = term.abs().sum(1)
            self.rows_of[3 + off] = (sc * term.sum(1), sc * a,
                                     sc * ((e_pt * (lpt - lps).abs() + pt * (e_lpt + e_lps)).sum(1) + 2 * U24 * a))
            k = w['out_kl'] * tw * (tau * tau if self.wrong == 'kl_grad_tau2' else tau)
            g = g + k * (ps - pt)
            gb = gb + abs(k) * (e_ps + e_pt + 4 * U24 * (ps + pt))
        if w['out_ce'] != 0:
            lps, ps, e_lps, e_ps = _feat_softmax(s, 1.0, n)
            lpt, pt, e_lpt, e_pt = _feat_softmax(t, 1.0, n)
            nb = 1.0 if self.wrong == 'ce_no_b' else 1.0 / B
            a = (pt * lps.abs()).sum(1)
            self.rows_of[4 + off] = (-nb * (pt * lps).sum(1), nb * a, nb * ((e_pt * lps.abs() + pt * e_lps).sum(1) + 2 * U24 * a))
            k = w['out_ce'] * tw * nb
            g = g + k * (ps - pt)
            gb = gb + abs(k) * (e_ps + e_pt + 4 * U24 * (ps + pt))
        self.g[tow], self.gb[tow], self.gh[tow] = g, gb, torch.zeros_like(g)

    # -- cross-modal terms ---------------------------------------------------------------------------------------------------------
    def _cross(self, e):
        cfg, w, B, E, wrong = self.cfg, self.cfg.w, self.B, self.E, self.wrong
        zero = torch.zeros(B, dtype=F64)
        for s in (9, 10, 11, 12):
            self.rows_of[s] = (zero, zero, zero)
        inv = [1 / e[k].norm(dim=1) for k in ('si', 'st')]
        ah, bh = e['si'] * inv[0][:, None], e['st'] * inv[1][:, None]
        tah, tbh = e['ti'] / e['ti'].norm(dim=1, keepdim=True), e['tt'] / e['tt'].norm(dim=1, keepdim=True)
        self.S, self.T = S, T = ah @ bh.T, tah @ tbh.T
        eS, eT = (E + 2) * U24 * (ah.abs() @ bh.abs().T), (E + 2) * U24 * (tah.abs() @ tbh.abs().T)
        eST = eS + eT
        self.und = (S - T).abs() <= eST
        if not cfg.cross:
            return
        eye = torch.eye(B, dtype=torch.bool)
        eyef = eye.to(F64)
        ntile = (B + 15) // 16
        # column weights of the wrong kernels: cw in every sum over the columns of an image row, gw in the gradient product only
        cw, gw = torch.ones(B, dtype=F64), torch.ones(B, dtype=F64)
        if wrong == 'last_col_twice':
            cw[B - 1] = gw[B - 1] = 2.0
        elif wrong == 'tile_lost':
            cw[16 * (ntile - 1):] = 0.0
            gw[16 * (ntile - 1):] = 0.0
        elif wrong == 'slice_lost':
            t0, t1 = slice_tiles(B, B)[-1]
            gw[16 * t0:16 * t1] = 0.0
        D, eD = torch.zeros(B, B, dtype=F64), torch.zeros(B, B, dtype=F64)
        n_merge = (ntile + 3) // 4 + 15

        # cos_diff and logits_mse: accumulated by every call that runs the stripes
        k_pos = w['cos_diff'] / B
        k_neg = (w['cos_diff'] / (B * B if wrong == 'cd_b2' else B * (B - 1))) if B > 1 else 0.0
        sgn = -1.0 if wrong == 'cd_swap' else 1.0
        D = D - k_pos * ((sgn * (T - S) > 0) & eye).to(F64) + k_neg * ((sgn * (S - T) > 0) & ~eye).to(F64)
        pos = torch.relu(sgn * (T - S)).diagonal()
        neg = (torch.relu(sgn * (S - T)) * (1 - eyef) * cw).sum(1)
        nn = B * B if wrong == 'cd_b2' else B * (B - 1)
        if B > 1 or w['cos_diff'] != 0:
            v = pos / B + neg / nn                          # B = 1 with the term on: 0 / 0 = NaN, as the reference
            own = (eST * (T - S + eST > 0).to(F64)).diagonal() / B + (eST * (S - T + eST > 0).to(F64) * (1 - eyef)).sum(1) / nn
        else:
            v, own = pos / B, eST.diagonal() / B
        self.rows_of[9] = (v, v, own)
        k = 2 * w['logits_mse'] / (B * B)
        D = D + k * (S - T)
        eD = eD + abs(k) * eST
        v = ((S - T) ** 2 * cw).sum(1) / (B * B)
        self.rows_of[12] = (v, v, (2 * (S - T).abs() * eST + eST ** 2).sum(1) / (B * B) + 2 * U24 * v)

        def stat(X, eX):
            """row and column log-sum-exps of X, probabilities against each, and their errors"""
            R, C = _wlse(X, 1, cw), _wlse(X, 0)
            Pr, Pc = torch.exp(X - R[:, None]), torch.exp(X - C[None, :])
            eR = (Pr * eX).sum(1) + n_merge * (8 + R.abs()) * U24
            eC = (Pc * eX).sum(0) + n_merge * (8 + C.abs()) * U24
            elr = eX + eR[:, None] + U24 * (X - R[:, None]).abs()           # error of log p (rows), then of p
            elc = eX + eC[None, :] + U24 * (X - C[None, :]).abs()
            return R, C, eR, eC, Pr, Pc, elr, elc

        ninf = torch.full((B,), -math.inf, dtype=F64)
        st, sb = [ninf] * 6, [zero] * 6
        if w['hard_label'] != 0:
            R, C, eR, eC, Pr, Pc, elr, elc = stat(S, eS)
            st[0], st[3], sb[0], sb[3] = R, C, eR, eC
            if wrong == 'hl_rowstat':
                Pc = torch.exp(S - R[None, :])
            k = 0.5 * w['hard_label'] / B
            D = D + k * (Pr + Pc - 2 * eyef)
            eD = eD + abs(k) * (Pr * (elr + XA) + Pc * (elc + XA))
            d = S.diagonal()
            self.rows_of[10] = (0.5 * (R + C - 2 * d) / B, 0.5 * (R.abs() + C.abs() + 2 * d.abs()) / B,
                                0.5 * (eR + eC + 2 * eS.diagonal()) / B)
        if w['soft_label'] != 0:
            tau = cfg.tau
            Xs, Xt = S / tau, T / tau
            eXs, eXt = eS / tau + 2 * U24 * Xs.abs(), eT / tau + 2 * U24 * Xt.abs()
            Rs, Cs, eRs, eCs, Psr, Psc, elsr, elsc = stat(Xs, eXs)
            Rt, Ct, eRt, eCt, Ptr, Ptc, eltr, eltc = stat(Xt, eXt)
            st[1], st[2], st[4], st[5], sb[1], sb[2], sb[4], sb[5] = Rs, Rt, Cs, Ct, eRs, eRt, eCs, eCt
            sc = 0.5 * (tau if wrong == 'sl_scalar_tau' else tau * tau)
            dr = (Xt - Rt[:, None]) - (Xs - Rs[:, None])                    # log p_t - log p_s, rows
            dc = (Xt - Ct[None, :]) - (Xs - Cs[None, :])
            v = (Ptr * dr * cw).sum(1) + (Ptc * dc).sum(0)
            a = (Ptr * dr.abs()).sum(1) + (Ptc * dc.abs()).sum(0)
            own = ((Ptr * (eltr + XA) * dr.abs() + Ptr * (eltr + elsr)).sum(1)
                   + (Ptc * (eltc + XA) * dc.abs() + Ptc * (eltc + elsc)).sum(0) + 2 * U24 * a)
            self.rows_of[11] = (sc * v, sc * a, sc * own)
            if wrong == 'sl_rowstat':
                Psc, Ptc = torch.exp(Xs - Rs[None, :]), torch.exp(Xt - Rt[None, :])
            k = 0.5 * w['soft_label'] * (tau * tau if wrong == 'sl_grad_tau2' else tau)
            D = D + k * ((Psr - Ptr) + (Psc - Ptc))
            eD = eD + abs(k) * (Psr * (elsr + XA) + Ptr * (eltr + XA) + Psc * (elsc + XA) + Ptc * (eltc + XA))
        self.stats, self.stats_b = torch.stack(st), torch.stack(sb)
        self.D = D

        hinge = self.und.to(F64) * (abs(k_pos) * eyef + abs(k_neg) * (1 - eyef))      # kept apart from eD: either branch is allowed there
        for tow, (Dm, Y, xh, wcol) in enumerate(((D, bh, ah, gw), (D.T, ah, bh, None))):
            G = (Dm * wcol if wcol is not None else Dm) @ Y
            eG = (eD if tow == 0 else eD.T) @ Y.abs() + (B + 16) * U24 * (Dm.abs() @ Y.abs())
            hG = (hinge if tow == 0 else hinge.T) @ Y.abs()
            iv = inv[tow].roll(-1) if wrong == 'neighbour_inv' else inv[tow]
            dot = (xh * G).sum(1, keepdim=True)
            da = (G if wrong == 'no_projection' else G - xh * dot) * iv[:, None]
            xa = xh.abs()
            proj = lambda v: v + xa * (xa * v).sum(1, keepdim=True)
            e_da = (proj(eG) + (E + 32) * U24 * xa * (xa * G.abs()).sum(1, keepdim=True)
                    + 16 * U24 * (G.abs() + xa * dot.abs())) * inv[tow][:, None]
            self.gb[tow] = self.gb[tow] + e_da + U24 * (self.g[tow].abs() + da.abs())
            self.gh[tow] = proj(hG) * inv[tow][:, None]
            self.g[tow] = self.g[tow] + da

    # -- scalars of a row block ----------------------------------------------------------------------------------------------------
    def share(self, r0=0, rows=None):
        """(value [16], bound [16]) of the scalars a call that owns rows [r0, r0 + rows) writes: its share of every slot"""
        cfg, B = self.cfg, self.B
        rows = B if rows is None else rows
        val, bnd = torch.zeros(16, dtype=F64), torch.zeros(16, dtype=F64)
        rtile, ntile = (rows + 15) // 16, (B + 15) // 16
        n_tower = n_sum(self.E) + rows + NREP + 4
        n_cross = 4 * ((ntile + 3) // 4) + 6 + 16 * rtile * loss_slices(B, rows) + NREP + 4
        tot_b = tot_a = 0.0
        for slot, (v, a, own) in self.rows_of.items():
            v, a, own = (x[r0:r0 + rows].sum() for x in (v, a, own))
            val[slot] = v
            bnd[slot] = (n_tower if slot <= 8 else n_cross) * U24 * a + own + 4 * U24 * v.abs()
            name = NAMES[(slot - 1) % 4] if slot <= 8 else CROSS[slot - 9]
            weight = cfg.w[name] * (self.tw if slot <= 8 else 1.0)
            if weight != 0:                                 # (a NaN slot of a switched-off term must not reach the total)
                val[0] += weight * v
                tot_b = tot_b + abs(weight) * bnd[slot]
                tot_a = tot_a + abs(weight * v)
        bnd[0] = tot_b + 16 * U24 * tot_a
        return val, bnd

    def grad_rows(self, tow, r0=0, rows=None):
        rows = self.B if rows is None else rows
        return tuple(x[tow][r0:r0 + rows] for x in (self.g, self.gb, self.gh))


@functools.lru_cache(maxsize=64)
def _reference(B, E, key):
    w, tau, two = key
    return Reference(inputs(B, E), Cfg(dict(zip(NAMES, w)), tau, two))


def reference(B, E, cfg):
    return _reference(B, E, cfg.key)


def leaves_bound(ref, other, r0=0, rows=None):
    """None if every value of `other` (a Reference with the same inputs) lies inside the bounds of `ref`; else what leaves them first"""
    for tow in ref.g:
        g, gb, gh = ref.grad_rows(tow, r0, rows)
        bad = ~((other.grad_rows(tow, r0, rows)[0] - g).abs() <= gb + gh)
        if bad.any():
            return f'gradient of tower {tow}: {int(bad.sum())} elements'
    (v, b), (vo, _) = ref.share(r0, rows), other.share(r0, rows)
    bad = ~((vo - v).abs() <= b) & ~(torch.isnan(v) & torch.isnan(vo))
    if bad.any():
        return f'scalar slots {torch.nonzero(bad).flatten().tolist()}'
    if ref.stats is not None and other.stats is not None:
        bad = ~((other.stats - ref.stats).abs() <= ref.stats_b) & ~(ref.stats == other.stats)
        if bad.any():
            return f'statistics: {int(bad.sum())} elements'
    return None


def insensitive(B, E, cfg, wrong):
    """None if the wrong kernel `wrong` leaves a bound of the right reference at this case; else a message: the bounds would hide it"""
    if leaves_bound(reference(B, E, cfg), Reference(inputs(B, E), cfg, wrong)) is not None:
        return None
    return f'B={B} E={E} {cfg.what}: every value of the wrong kernel "{wrong}" stays inside the bounds'


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernel under guards
# ----------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ones_bits(n):
    return torch.full((n,), -1, dtype=torch.int32, device=DEV).view(torch.float32)


class _Slot:
    """an owned [n] float range inside a larger guard-filled buffer, PAD_FRONT floats (16 bytes) after its start"""

    def __init__(self, n, data=None):
        self.n = n
        self.buf = _ones_bits(PAD_FRONT + n + PAD_BACK)               # all-ones bits: a NaN
        if data is not None:
            self.buf[PAD_FRONT:PAD_FRONT + n] = data.reshape(-1).to(DEV)
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 256 == 0 and self.ptr % 16 == 0 and self.ptr % 256 != 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD_FRONT

    def owned(self):
        return self.buf[PAD_FRONT:PAD_FRONT + self.n]

    def foreign_changed(self, owned_may_change):
        want = self.before.clone()
        if owned_may_change:
            want[PAD_FRONT:PAD_FRONT + self.n] = self.owned()
        return int((want.view(torch.int32) != self.buf.view(torch.int32)).sum())


class Workspace:
    """exactly dclip_distill_loss_workspace(B, E) bytes at a 256-byte-aligned offset of a patterned buffer, WS_GUARD bytes behind it"""

    def __init__(self, B, E):
        self.bytes = _lib().dclip_distill_loss_workspace(B, E)
        n = 512 + self.bytes + WS_GUARD
        self.buf = ((torch.arange(n, device=DEV, dtype=torch.int32) * 37 + 11) % 251).to(torch.uint8)
        self.off = (-self.buf.data_ptr()) % 256 + 256
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0

    def foreign_changed(self):
        end = self.off + self.bytes
        return int((self.buf[:self.off] != self.before[:self.off]).sum()) + int((self.buf[end:] != self.before[end:]).sum())


class Result:
    pass


def run_kernel(B, E, cfg, r0=None, rows=None, gstats=None, want_stats=False, ws=None):
    """one call with its own buffers -> Result(out [16], d [tower] [rows, E], stats [6, rows], all float64 on the CPU; `memory`: the
    failures of the guards).  r0 None: dclip_distill_loss, else dclip_distill_loss_rows."""
    e = inputs(B, E)
    n = B if rows is None else rows
    ins = {k: _Slot(B * E, e[k]) for k in (('si', 'ti', 'st', 'tt') if cfg.two else ('si', 'ti'))}
    d = [_Slot(n * E) for _ in range(2 if cfg.two else 1)]
    out = _Slot(16)
    ws = ws or Workspace(B, E)
    stats = _Slot(6 * n) if want_stats else None
    gs = _Slot(6 * B, gstats.float()) if gstats is not None else None
    p = lambda k: ins[k].ptr if k in ins else None
    cfg_arr = cfg.array()
    cfg_p = ctypes.cast(cfg_arr, ctypes.c_void_p)
    if r0 is None:
        _lib().dclip_distill_loss(p('si'), p('ti'), p('st'), p('tt'), B, E, cfg_p, out.ptr, d[0].ptr, d[1].ptr if cfg.two else None,
                                  ws.ptr, ws.bytes, _stream())
    else:
        _lib().dclip_distill_loss_rows(p('si'), p('ti'), p('st'), p('tt'), B, E, r0, n, cfg_p, out.ptr, d[0].ptr,
                                       d[1].ptr if cfg.two else None, gs.ptr if gs else None, stats.ptr if stats else None,
                                       ws.ptr, ws.bytes, _stream())
    torch.cuda.synchronize()
    stats_only = want_stats and gstats is None
    r = Result()
    r.memory = []
    for name, slot, may in ([(k, v, False) for k, v in ins.items()] + [(f'd[{i}]', v, True) for i, v in enumerate(d)]
                            + [('scalars', out, True)] + ([('stats_out', stats, True)] if stats else [])
                            + ([('gathered_stats', gs, False)] if gs else [])):
        c = slot.foreign_changed(may)
        if c:
            r.memory.append(f'{name}: {c} floats changed outside what the call owns')
    c = ws.foreign_changed()
    if c:
        r.memory.append(f'workspace: {c} guard bytes changed around its {ws.bytes} bytes')
    r.out = None if stats_only else out.owned().cpu()
    r.d = None if stats_only else [s.owned().view(n, E).cpu() for s in d]
    r.stats = stats.owned().view(6, n).cpu() if stats else None
    return r


WORST = {}                                           # what -> worst err / bound of this process


def _ratio(what, err, bound):
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=math.inf).max().item() if q.numel() else 0.0
    WORST[what] = max(WORST.get(what, 0.0), q)
    return q


def check(ref, res, label, r0=0, rows=None, fails=None):
    """every output of one call against the reference; appends to `fails`, records the worst err / bound per term"""
    cfg = ref.cfg
    fails = [] if fails is None else fails
    on = [n for n in NAMES if cfg.w[n] != 0]
    term = (on[0] if len(on) == 1 else 'all' if cfg.cross else 'towers') + ('' if cfg.two else ' (one tower)')
    fails += [f'{label}: {m}' for m in res.memory]
    for tow, got in enumerate(res.d):
        g, gb, gh = ref.grad_rows(tow, r0, rows)
        err = (got.double() - g).abs()
        bad = ~(err <= gb + gh)
        q = _ratio(f'grad {term}', err, gb + gh)
        if bad.any():
            i = tuple(torch.nonzero(bad)[0].tolist())
            fails.append(f'{label}: gradient of tower {tow}: {int(bad.sum())} of {bad.numel()} elements outside their bound; first at {i}: '
                         f'got {got[i].item()!r} ref {g[i].item()!r} bound {(gb + gh)[i].item():.3e}; worst err / bound {q:.3f}')
    val, bnd = ref.share(r0, rows)
    out = res.out.double()
    for slot in range(16):
        name = 'total' if slot == 0 else f'{term} slot {slot}'
        if math.isnan(val[slot].item()):
            if not math.isnan(out[slot].item()):
                fails.append(f'{label}: {name}: got {out[slot].item()!r}, the reference is NaN')
            continue
        if not math.isfinite(out[slot].item()):
            fails.append(f'{label}: {name}: got {out[slot].item()!r}, the reference is finite ({val[slot].item()!r})')
            continue
        if bnd[slot] == 0 and val[slot] == 0:               # a slot nobody fills, and slots 13 to 15: zero
            if out[slot].item() != 0:
                fails.append(f'{label}: {name}: got {out[slot].item()!r}, must be 0')
            continue
        err = (out[slot] - val[slot]).abs()
        q = _ratio(f'scalar {term}' if slot else f'total {term}', err.reshape(1), bnd[slot].reshape(1))
        if not err <= bnd[slot]:
            fails.append(f'{label}: {name}: got {out[slot].item()!r} ref {val[slot].item()!r} bound {bnd[slot].item():.3e}; err / bound {q:.3f}')
    if not torch.isnan(val[0]):                             # the total against the kernel's own slots
        ws = [(s, cfg.w[NAMES[(s - 1) % 4] if s <= 8 else CROSS[s - 9]] * (ref.tw if s <= 8 else 1.0)) for s in ref.rows_of]
        own = sum(wt * out[s] for s, wt in ws if wt != 0)
        mag = sum(abs(wt * out[s]) for s, wt in ws if wt != 0)
        if not abs(out[0] - own) <= 16 * U24 * mag:
            fails.append(f'{label}: total {out[0].item()!r} is not the weighted sum of the slots {float(own)!r}')
    return fails


def check_stats(ref, got, label, r0=0, rows=None, fails=None):
    """the six statistics of a statistics-only call: float64 log-sum-exps inside their bounds, -inf where no enabled term fills them"""
    fails = [] if fails is None else fails
    rows = ref.B if rows is None else rows
    want, bnd = ref.stats[:, r0:r0 + rows], ref.stats_b[:, r0:r0 + rows]
    got = got.double()
    for k in range(6):
        if torch.isinf(want[k]).all():
            if not (got[k] == -math.inf).all():
                fails.append(f'{label}: statistic {k} belongs to a disabled term and is not -inf: {got[k][:4].tolist()}')
            continue
        err = (got[k] - want[k]).abs()
        q = _ratio('statistics', err, bnd[k])
        if not (err <= bnd[k]).all():
            i = int(torch.nonzero(~(err <= bnd[k]))[0])
            fails.append(f'{label}: statistic {k} row {r0 + i}: got {got[k, i].item()!r} ref {want[k, i].item()!r} '
                         f'bound {bnd[k, i].item():.3e}; worst err / bound {q:.3f}')
    return fails


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f'worst err / bound  {k:32s} {WORST[k]:.4f}')


# ----------------------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,E', SWEEP)
def test_every_term_alone_and_together(B, E):
    """all configurations of `configs()` at one (B, E): gradients, the 16 scalars, the guards around every buffer, and a second call
    that must give bit-equal gradients"""
    fails = []
    ws = Workspace(B, E)                                    # one workspace for all calls: nothing may depend on what a call left in it
    for cfg in configs():
        ref = reference(B, E, cfg)
        label = f'B={B} E={E} {cfg.what}'
        res = run_kernel(B, E, cfg, ws=ws)
        check(ref, res, label, fails=fails)
        again = run_kernel(B, E, cfg)                       # fresh workspace, fresh outputs
        fails += [f'{label} (second call): {m}' for m in again.memory]
        for tow, (x, y) in enumerate(zip(res.d, again.d)):
            if not _bits_equal(x, y):
                fails.append(f'{label}: the gradient of tower {tow} differs between two calls in {int((x != y).sum())} elements')
    assert not fails, '\n'.join(fails[:40])


@pytest.mark.parametrize('E', BLOCK_E)
def test_row_blocks_without_statistics(E):
    """cos_diff and logits_mse over row blocks of B = 130: every block's gradient rows are the float64 rows of the whole batch, its
    scalars its share, and the shares of a partition add up to the whole-batch scalars"""
    B, fails = 130, []
    for cfg in (Cfg({'cos_diff': 1.0}), Cfg({'logits_mse': 1.0})):
        ref = reference(B, E, cfg)
        total = torch.zeros(16, dtype=F64)
        tot_b = torch.zeros(16, dtype=F64)
        for r0, rows in sorted(set(BLOCKS) | set(PARTITION)):
            label = f'B={B} E={E} rows [{r0}, {r0 + rows}) {cfg.what}'
            res = run_kernel(B, E, cfg, r0, rows)
            check(ref, res, label, r0, rows, fails)
            again = run_kernel(B, E, cfg, r0, rows)
            if not all(_bits_equal(x, y) for x, y in zip(res.d, again.d)):
                fails.append(f'{label}: gradients differ between two calls')
            if (r0, rows) in PARTITION:
                total += res.out.double()
                tot_b += ref.share(r0, rows)[1]
        whole = ref.share()[0]
        bad = ~((total - whole).abs() <= tot_b)
        if bad.any():
            fails.append(f'B={B} E={E} {cfg.what}: the shares of the partition do not add up in slots {torch.nonzero(bad).flatten().tolist()}: '
                         f'{total[bad].tolist()} against {whole[bad].tolist()}')
    assert not fails, '\n'.join(fails[:40])


@pytest.mark.parametrize('E', BLOCK_E)
def test_row_blocks_with_gathered_statistics(E):
    """hard_label and soft_label over row blocks of B = 130: statistics call per block of the partition (all six rows against float64
    log-sum-exps), a gather built here, then the gradient call per block with the gathered [6, B]"""
    B, fails = 130, []
    for cfg in (Cfg({'hard_label': 1.0}), Cfg({'soft_label': 1.0}, 0.5), Cfg({'soft_label': 1.0}, 2.0), Cfg(W_ALL, 0.5)):
        ref = reference(B, E, cfg)
        gathered = torch.empty(6, B, dtype=torch.float32)
        for r0, rows in PARTITION:
            label = f'B={B} E={E} statistics of rows [{r0}, {r0 + rows}) {cfg.what}'
            res = run_kernel(B, E, cfg, r0, rows, want_stats=True)
            fails += [f'{label}: {m}' for m in res.memory]
            check_stats(ref, res.stats, label, r0, rows, fails)
            gathered[:, r0:r0 + rows] = res.stats
        total = torch.zeros(16, dtype=F64)
        tot_b = torch.zeros(16, dtype=F64)
        for r0, rows in sorted(set(BLOCKS) | set(PARTITION)):
            label = f'B={B} E={E} rows [{r0}, {r0 + rows}) gathered {cfg.what}'
            res = run_kernel(B, E, cfg, r0, rows, gstats=gathered)
            check(ref, res, label, r0, rows, fails)
            again = run_kernel(B, E, cfg, r0, rows, gstats=gathered)
            if not all(_bits_equal(x, y) for x, y in zip(res.d, again.d)):
                fails.append(f'{label}: gradients differ between two calls')
            if (r0, rows) in PARTITION:
                total += res.out.double()
                tot_b += ref.share(r0, rows)[1]
        whole = ref.share()[0]
        bad = ~((total - whole).abs() <= tot_b)
        if bad.any():
            fails.append(f'B={B} E={E} {cfg.what}: the shares of the partition do not add up in slots {torch.nonzero(bad).flatten().tolist()}')
    assert not fails, '\n'.join(fails[:40])


@pytest.mark.parametrize('B,E', [(17, 48), (40, 768), (130, 272)])
def test_statistics_of_the_whole_batch(B, E):
    """a statistics-only call that owns every row, per enabled term: the filled rows against float64, the others -inf (include/dclip.h)"""
    fails = []
    for cfg in (Cfg({'hard_label': 1.0}), Cfg({'soft_label': 1.0}, 0.5), Cfg({'soft_label': 1.0}, 2.0), Cfg({'cos_diff': 1.0}),
                Cfg(W_ALL, 2.0)):
        label = f'B={B} E={E} statistics {cfg.what}'
        res = run_kernel(B, E, cfg, 0, B, want_stats=True)
        fails += [f'{label}: {m}' for m in res.memory]
        check_stats(reference(B, E, cfg), res.stats, label, fails=fails)
    assert not fails, '\n'.join(fails[:40])


def test_batch_of_one_total():
    """B = 1: with cos_diff off every slot and the total are finite; with it on slot 9 and the total are NaN like the reference (mean
    over no negatives) while the gradient stays finite and inside its bound"""
    fails = []
    for E in (48, 768):
        for cfg in (Cfg({n: W_ALL[n] for n in NAMES if n != 'cos_diff'}, 0.5), Cfg({'cos_diff': 1.0}), Cfg(W_ALL, 2.0)):
            ref = reference(1, E, cfg)
            res = run_kernel(1, E, cfg)
            check(ref, res, f'B=1 E={E} {cfg.what}', fails=fails)
            on = cfg.w['cos_diff'] != 0
            assert math.isnan(ref.share()[0][0].item()) == on
            if math.isnan(res.out[0].item()) != on or math.isnan(res.out[9].item()) != on:
                fails.append(f'B=1 E={E} {cfg.what}: total {res.out[0].item()!r}, slot 9 {res.out[9].item()!r}')
            if not all(torch.isfinite(d).all() for d in res.d):
                fails.append(f'B=1 E={E} {cfg.what}: gradient not finite')
    assert not fails, '\n'.join(fails)
