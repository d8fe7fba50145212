"""Inputs, float64 reference and error bounds of dclip_relation_kl (the `intra_kl` term), shared by tests/test_relkl_cpu.py and
tests/test_relkl_gpu.py.  Everything here is a property of the inputs alone: the draws come from a CPU generator (the same numbers with
and without a GPU) and no constant was fitted to what a kernel gives.  U24 = 2^-24.

The term, for one tower.  s, t = student / teacher rows, x^ = x / |x| (no epsilon), tau the temperature, every sum over j != i:
    a = s^ s^T / tau ; b = t^ t^T / tau ; lseS_i = log sum_j exp a_ij ; lseT_i the same of b ; p = exp(a - lseS) ; q = exp(b - lseT)
    KL_i = sum_j q_ij ((b_ij - lseT_i) - (a_ij - lseS_i)) ; intra_kl = tau^2 mean_i KL_i
    M = p - q ; D = w (tau / B) (M + M^T) ; G = D s^ ; d s_i = (G_i - s^_i (s^_i . G_i)) / |s_i|

Bounds, per element, built as tests/icl_cases.py builds them: U24 times a count of roundings, read off relation.hip, times the same sum
with absolute values inside.  What differs from ICL is marked (*).
  logit       e_a = (E + 2) U24 (|s^| |s^|^T) / tau + 2 U24 |a|: the E-term product on the f32 MFMA and the two normalisations, then 1 / tau
              and the product with it.  (*) two matrices: e_b the same of t^.
  lse         the softmax-weighted error of its inputs plus n_merge (8 + |lse|) U24: each running add, lane, wave and slice merge is two
              exps, a sum, a log (XA = 8 U24) and one rounding of max + log.  n_merge: a lane's running adds, one per column tile its wave
              walks, ceil(tiles of the largest slice / 4); its own log, 1; the 4 lane steps of stripe_put; the 2 wave levels of
              stripe_get; one merge per slice in rel_merge_kernel (it starts from the empty sum): ceil(slice tiles / 4) + 7 + slices.
              (*) two statistics per row, lseS and lseT, each with its own inputs' errors; the same count (the same code merges both).
  log-prob    la = a - lseS: e_la = e_a + e_lseS + U24 |la| (one subtraction); lb the same.
  prob        e_p = p (e_la + U24 |la| + XA) + 2^-126: the product with log2(e) inside __expf is a second rounding of la, then the exp (XA);
              a probability carries 2^-126 on top (at tau = 0.01 a logit sits up to 200 below its row's log-sum-exp: a denormal or 0).
  element     (*) W_ij = (p_ij - q_ij) + (p_ji - q_ji) carries four exps and the statistics of rows i AND j:
              e_M = e_p + e_q + U24 |M| ; e_W = e_M + e_M^T + U24 |W| ; e_D = |k| e_W, k = w tau / B.
  product     e_G = e_D |s^| + (B + 16) U24 (|D| |s^|): B accumulations of the stripe product, at most 8 slice additions, and 8 for the
              roundings of k (tau, tau / B, the product with w) and of the normalised rows.
  projection  e_ds = (e_G + |s^| (|s^| . e_G) + (E + 32) U24 |s^| (|s^| . |G|) + 16 U24 (|G| + |s^| |s^ . G|)) / |s|
  scalars     (*) the term of (i, j) is T_ij = q_ij r_ij, r = lb - la: e_r = e_lb + e_la + U24 |r| ; e_T = e_q |r| + q e_r + U24 |T|.
              mean_i KL_i = sum_ij T_ij / B; bound = (n_acc U24 sum |T| + sum e_T) / B + 4 U24 |mean KL|, n_acc the longest chain of
              additions of the fixed-order sum: a lane's tiles ceil(slice tiles / 4), 4 lane steps and 2 wave levels (stripe_put /
              stripe_get), 4 steps over the 16 rows of a record, the slices of a stripe in order, 6 steps of the wave sum, 2 over
              the four waves: ceil(slice tiles / 4) + 18 + slices.  intra_kl = tau^2 mean KL adds 4 U24 (tau, tau^2, the product),
              out[0] the product with w.
tests/test_relkl_cpu.py asserts that the same formulas evaluated in float32 on the CPU stay within HALF of every bound on every case.

Cases.  B in {1, 2, 3, 15, 16, 17, 33, 40, 130} at E = 48 and 768, every E in {16, 48, 64, 256, 272, 512, 528, 768, 1024} at B = 17 and
130, each at tau = 0.01, 0.07 and 2: every stripe edge and slice count (B <= 16: 1 tile, 1 slice; 17: 2, 2, ONE column in the last tile;
33 and 40: 3, 3; 130: 9 tiles over 8 slices, the last slice has two), and E = 16 where three of stripe B's four waves have no slab of the
product.  Row norms spread over more than two decades (0.08 to 12) in student and teacher independently.  The kernel has one workgroup
per (stripe, slice) where ICL has two, so it asks stripe_slices for twice the slices: B = 340 is 22 tiles over 8 slices of 2 and 3 (three
waves hold statistics), B = 512 at E = 512 is 32 tiles over 8 slices of 4 (every wave holds one tile), and B = 1040, added for this
slicing, is 65 tiles over 3 slices of 21 and 22: every wave walks five or six tiles, so its running (max, sum) is merged six times.
Four more families: near-orthogonal rows (every cosine within +-0.02) at tau = 0.01, where a maximum fixed at 1 / tau = 100 would
underflow every row; all teacher rows bit copies of one row (q uniform, KL_i = -log(B - 1) - mean_j (a_ij - lseS_i)); a duplicated
student row pair inside one tile (the excluded diagonal next to an equal off-diagonal logit); student bit-equal to teacher (zeros).
"""
import functools
import math

import torch

U24 = 2.0 ** -24
XA = 8 * U24                                        # __expf / __logf allowance (tests/test_softmax_edges_gpu.py::_loss_tol)
TINY = 2.0 ** -126                                   # below it an f32 exp is a denormal or flushed to zero: absolute, not relative
F64 = torch.float64
B_LIST = (1, 2, 3, 15, 16, 17, 33, 40, 130)
E_LIST = (16, 48, 64, 256, 272, 512, 528, 768, 1024)
SWEEP = sorted({(B, E) for B in (17, 130) for E in E_LIST} | {(B, E) for B in B_LIST for E in (48, 768)})
TAUS = (0.01, 0.07, 2.0)
MAX_B, MAX_E = 4096, 1024
KEYS = ('s', 't')                                    # the C entry's order


def slices(B):
    """column slices of the stripe kernels, as rel_slices of relation.hip picks them: stripe_slices for HALF the row stripes"""
    tiles = (B + 15) // 16
    zs = min(max(256 // (2 * ((tiles + 1) // 2)), 1), 8, tiles)
    while zs < 8 and -(-tiles // zs) * 16 > 512:
        zs += 1
    return zs


def slice_tiles(B):
    """[(first tile, end tile)] of every column slice"""
    nt, zs = (B + 15) // 16, slices(B)
    return [(nt * z // zs, nt * (z + 1) // zs) for z in range(zs)]


def _lane_tiles(B):
    return -(-max(t1 - t0 for t0, t1 in slice_tiles(B)) // 4)


def n_merge(B):
    return _lane_tiles(B) + 7 + slices(B)


def n_acc(B):
    return _lane_tiles(B) + 18 + slices(B)


# ----------------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------------
def _scales(B, g):
    scale = 10.0 ** (2.2 * torch.rand(B, generator=g) - 1.1)
    if B >= 2:
        p = torch.randperm(B, generator=g)
        scale[p[0]], scale[p[1]] = 0.08, 12.0         # > two decades between two rows of every tensor
    return scale


def _draw(B, E, seed):
    g = torch.Generator().manual_seed(seed)
    col = 1.0 / (1.0 + torch.arange(E, dtype=torch.float32) / 16)      # anisotropic like trained embeddings
    r = lambda: torch.randn(B, E, generator=g, dtype=torch.float32) * col
    c = torch.randn(max(B // 6, 1), E, generator=g, dtype=torch.float32) * col      # a few clusters: some rows are near neighbours
    zs = c[torch.randint(0, c.shape[0], (B,), generator=g)] + r()
    z = dict(s=zs, t=0.6 * zs + 0.8 * r())                              # teacher correlated with student
    return {k: (z[k] * _scales(B, g)[:, None]).contiguous() for k in KEYS}


def _orthogonal(B, E, seed):
    """rows of two mutually orthogonal orthonormal sets plus a little noise: every cosine within +-0.02"""
    g = torch.Generator().manual_seed(seed)
    assert 2 * B <= E
    qm, _ = torch.linalg.qr(torch.randn(E, 2 * B, generator=g, dtype=F64))
    e = {}
    for i, k in enumerate(KEYS):
        rows = qm[:, i * B:(i + 1) * B].T + 0.08 * torch.randn(B, E, generator=g, dtype=F64) / math.sqrt(E)
        e[k] = (rows.float() * _scales(B, g)[:, None]).contiguous()
    return e


def _teacher_copies(B, E, seed):
    """all teacher rows bit copies of one row: every b_ij is the same number, q is uniform"""
    e = _draw(B, E, seed)
    e['t'] = e['t'][:1].repeat(B, 1).contiguous()
    return e


DUP_ROWS = (3, 9)


def _dup_pair(B, E, seed):
    """student rows 3 and 9 bit copies of each other: a_39 is the diagonal's number, in the tile that holds both diagonals"""
    e = _draw(B, E, seed)
    e['s'][DUP_ROWS[1]] = e['s'][DUP_ROWS[0]]
    return e


def _equal(B, E, seed):
    """student bit-equal to teacher"""
    e = _draw(B, E, seed)
    e['s'] = e['t'].clone()
    return e


class Case:
    def __init__(self, name, B, E, tau, build):
        self.name, self.B, self.E, self.tau, self._build = name, B, E, tau, build

    @property
    def e(self):
        return _inputs(self._build, self.B, self.E)

    @property
    def ref(self):
        return _reference(self._build, self.B, self.E, self.tau)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _inputs(build, B, E):
    return build(B, E, 7907 * B + E)


@functools.lru_cache(maxsize=None)
def _reference(build, B, E, tau):
    return Reference(_inputs(build, B, E), tau)


def sweep_case(B, E, tau):
    return SWEEP_CASES[SWEEP.index((B, E)) * 3 + TAUS.index(tau)]


SWEEP_CASES = [Case(f'B{B}-E{E}-tau{tau:g}', B, E, tau, _draw) for B, E in SWEEP for tau in TAUS]
ORTHOGONAL = Case('orthogonal-B130-E768-tau0.01', 130, 768, 0.01, _orthogonal)
TEACHER_COPIES = Case('teacher-copies-B40-E48-tau0.07', 40, 48, 0.07, _teacher_copies)
DUP_PAIR = [Case(f'dup-pair-B33-E48-tau{tau:g}', 33, 48, tau, _dup_pair) for tau in (0.01, 0.07)]
EQUAL = [Case(f'equal-B{B}-E{E}-tau{tau:g}', B, E, tau, _equal) for B, E, tau in ((33, 48, 0.07), (130, 768, 0.01))]
FOUR_WAVES = [Case('four-waves-B340-E48-tau0.07', 340, 48, 0.07, _draw), Case('four-waves-B512-E512-tau0.01', 512, 512, 0.01, _draw),
              Case('four-waves-B1040-E48-tau0.07', 1040, 48, 0.07, _draw)]
CASES = SWEEP_CASES + [ORTHOGONAL, TEACHER_COPIES] + DUP_PAIR + EQUAL + FOUR_WAVES


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 reference with its bounds
# ----------------------------------------------------------------------------------------------------------------------------------
WRONGS = ('tile_lost', 'diag_kept', 'no_transpose', 'no_tau_in_grad', 'no_projection', 'slice_lost', 'wave_lost', 'teacher_stat')


class Reference:
    """float64 values of one (inputs, tau, weight): out [4] with bounds out_b, the gradient g [B, E] with bounds gb, and the logits A,
    log-sum-exps lse, probabilities P of the two matrices (index 0: student, 1: teacher), W = M + M^T, D, G.
    `wrong` builds one of the wrong kernels of WRONGS instead (values only: the bounds stay those of the right one)."""

    def __init__(self, e32, tau, weight=1.0, wrong=None):
        assert wrong is None or wrong in WRONGS
        s, t = e32['s'].to(F64), e32['t'].to(F64)
        self.B, self.E = B, E = s.shape
        self.tau, self.weight = tau, weight
        self.out, self.out_b = torch.zeros(4, dtype=F64), torch.zeros(4, dtype=F64)
        if B == 1:                                            # no column: zeros, exactly
            self.g, self.gb = torch.zeros_like(s), torch.zeros_like(s)
            return
        nm = n_merge(B)
        off = torch.ones(B, B, dtype=F64) if wrong == 'diag_kept' else 1.0 - torch.eye(B, dtype=F64)
        last = 16 * ((B + 15) // 16 - 1)
        cw = torch.ones(B, dtype=F64)                         # column weights of the statistics
        gw = torch.ones(B, dtype=F64)                         # of the product and the scalar
        if wrong == 'tile_lost' and last:
            cw[last:] = 0.0
            gw[last:] = 0.0
        if wrong == 'wave_lost':                              # the fourth wave's tiles missing from the statistics, not from the product
            for t0, t1 in slice_tiles(B):
                for jt in range(t0 + 3, t1, 4):
                    cw[16 * jt:16 * jt + 16] = 0.0
        pw = gw.clone()
        if wrong == 'slice_lost' and slices(B) > 1:           # the last slice's partial rows not added: the product only
            t0, t1 = slice_tiles(B)[-1]
            pw[16 * t0:16 * t1] = 0.0
        ns = s.norm(dim=1)
        sh, th = s / ns[:, None], t / t.norm(dim=1, keepdim=True)
        self.A, self.lse, self.P = [], [], []
        LA, eLA, eP = [], [], []
        for xh in (sh, th):
            A = xh @ xh.T / tau
            eA = (E + 2) * U24 * (xh.abs() @ xh.abs().T) / tau + 2 * U24 * A.abs()
            Am = A.masked_fill((off * cw) == 0, -math.inf)
            m = Am.max(1, keepdim=True).values
            lse = (m + torch.log(torch.exp(Am - m).sum(1, keepdim=True))).squeeze(1)
            self.A.append(A), self.lse.append(lse)
            LA.append((A, eA))
        if wrong == 'teacher_stat':
            self.lse[0] = self.lse[1]
        for (A, eA), lse in zip(LA, self.lse):
            la = (A - lse[:, None]) * off
            P = torch.exp(la) * off
            e_lse = (P * eA).sum(1) + nm * (8 + lse.abs()) * U24
            e_la = (eA + e_lse[:, None] + U24 * la.abs()) * off
            self.P.append(P)
            eLA.append((la, e_la))
            eP.append((P * (e_la + U24 * la.abs() + XA) + TINY) * off)
        (la, e_la), (lb, e_lb) = eLA
        p, q = self.P
        M, eM = p - q, eP[0] + eP[1] + U24 * (p - q).abs()
        W = (M if wrong == 'no_transpose' else M + M.T) * gw
        eW = eM + eM.T + U24 * W.abs()
        k = weight * (1.0 if wrong == 'no_tau_in_grad' else tau) / B
        D, eD = k * W, abs(weight * tau / B) * eW
        G = (D * pw) @ sh
        eG = eD @ sh.abs() + (B + 16) * U24 * (D.abs() @ sh.abs())
        dot = (sh * G).sum(1, keepdim=True)
        self.W, self.D, self.G = W, D, G
        self.g = (G if wrong == 'no_projection' else G - sh * dot) / ns[:, None]
        xa = sh.abs()
        proj = lambda v: v + xa * (xa * v).sum(1, keepdim=True)
        self.gb = (proj(eG) + (E + 32) * U24 * xa * (xa * G.abs()).sum(1, keepdim=True)
                   + 16 * U24 * (G.abs() + xa * dot.abs())) / ns[:, None]
        r = lb - la
        e_r = e_lb + e_la + U24 * r.abs()
        T = q * r * gw
        e_T = eP[1] * r.abs() + q * e_r + U24 * T.abs()
        self.kl_rows = T.sum(1)
        kl = T.sum() / B
        kl_b = (n_acc(B) * U24 * T.abs().sum() + e_T.sum()) / B + 4 * U24 * kl.abs()
        intra, intra_b = tau * tau * kl, tau * tau * kl_b + 4 * U24 * (tau * tau * kl).abs()
        self.out = torch.stack([weight * intra, intra, kl, torch.zeros((), dtype=F64)])
        self.out_b = torch.stack([abs(weight) * intra_b + 2 * U24 * (weight * intra).abs(), intra_b, kl_b, torch.zeros((), dtype=F64)])


def evaluate_f32(e32, tau, weight=1.0):
    """the formulas of the term in float32 on the CPU -> (out [4], d s), as float64"""
    s, t = e32['s'], e32['t']
    B = s.shape[0]
    if B == 1:
        return torch.zeros(4, dtype=F64), torch.zeros_like(s).to(F64)
    tau32, w32 = torch.tensor(tau, dtype=torch.float32), torch.tensor(weight, dtype=torch.float32)
    eye = torch.eye(B, dtype=torch.bool)
    inv = 1.0 / s.norm(dim=1)
    sh, th = s * inv[:, None], t / t.norm(dim=1, keepdim=True)
    lp = []
    for xh in (sh, th):
        A = ((xh @ xh.T) * (1.0 / tau32)).masked_fill(eye, -math.inf)
        lp.append((A - torch.logsumexp(A, 1, keepdim=True)).masked_fill(eye, 0.0))
    la, lb = lp
    p, q = torch.exp(la).masked_fill(eye, 0.0), torch.exp(lb).masked_fill(eye, 0.0)
    kl = (q * (lb - la)).sum() / B
    intra = (tau32 * tau32) * kl
    M = p - q
    G = ((w32 * (tau32 / B)) * (M + M.T)) @ sh
    g = (G - sh * (sh * G).sum(1, keepdim=True)) * inv[:, None]
    out = torch.stack([w32 * intra, intra, kl, torch.zeros(())])
    assert out.dtype == torch.float32 and g.dtype == torch.float32
    return out.to(F64), g.to(F64)


def torch_autograd_f64(e32, tau):
    """tau^2 times the batch mean of KL(softmax of the teacher's off-diagonal logits || the student's) by torch autograd in float64
    -> (intra_kl, mean KL, d s)"""
    F = torch.nn.functional
    s, t = e32['s'].to(F64).requires_grad_(True), e32['t'].to(F64)
    B = s.shape[0]
    if B == 1:
        return torch.zeros((), dtype=F64), torch.zeros((), dtype=F64), torch.zeros_like(s).detach()
    keep = ~torch.eye(B, dtype=torch.bool)
    rows = lambda x: (F.normalize(x, dim=1, eps=0) @ F.normalize(x, dim=1, eps=0).T / tau)[keep].view(B, B - 1)
    kl = F.kl_div(F.log_softmax(rows(s), 1), F.log_softmax(rows(t), 1), reduction='batchmean', log_target=True)
    intra = tau * tau * kl
    intra.backward()
    return intra.detach(), kl.detach(), s.grad


def ratio(err, bound):
    """worst err / bound; an exact result counts 0 whatever its bound, a NaN counts inf"""
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.nan_to_num(q, nan=math.inf).max().item() if q.numel() else 0.0
