"""Inputs, float64 reference and error bounds of dclip_interactive_loss (the `icl` term), shared by tests/test_icl_cpu.py and
tests/test_icl_gpu.py.  Everything here is a property of the inputs alone: the draws come from a CPU generator (the same numbers with
and without a GPU) and no constant was fitted to what a kernel gives.  U24 = 2^-24.

The term.  a, b = student image / text rows, p, q = teacher image / text rows, x^ = x / |x| (no epsilon), tau the temperature:
    A = a^ q^T / tau ; C = b^ p^T / tau ; L_i2t = mean_i (lse_j A_ij - A_ii) ; L_t2i the same of C ; icl = (L_i2t + L_t2i) / 2
    P = exp(A - lse) ; D = w (P - I) / (2 B tau) ; G = D q^ ; d a_i = (G_i - a^_i (a^_i . G_i)) / |a_i|   (b with C and p^)

Bounds, per element, built as the docstring of tests/test_loss_exact_gpu.py builds them: U24 times a count of roundings times the
same sum with absolute values inside.
  logit       e_A = (E + 2) U24 (|a^| |q^|^T) / tau + 2 U24 |A|: the E-term product on the f32 MFMA and the two normalisations, then 1 / tau
              and the product with it.
  exp, log    XA = 8 U24 per evaluated exp(x - lse) or log, plus U24 |x - lse| for the subtraction; a probability carries 2^-126 on top
              (at tau = 0.01 a logit sits up to 200 below its row's log-sum-exp: a denormal or 0 in f32).
  lse         the softmax-weighted error of its inputs plus n_merge (8 + |lse|) U24: each running add, lane, wave and slice merge is two
              exps, a sum, a log (XA) and one rounding of max + log.  n_merge, read off interactive.hip: a lane's running adds, one
              per column tile its wave walks, ceil(tiles of the largest slice / 4); its own log, 1; the 4 lane steps of stripe_put;
              the 2 wave levels of stripe_get; one merge per slice in icl_row_lse (it starts from the empty sum):
              n_merge = ceil(slice tiles / 4) + 7 + slices, at most 8 + 7 + 8 = 23 at B = 4096.
  D           e_D = |k| (P (e_A + e_lse + U24 |A - lse| + XA) + 2^-126), k = w / (2 B tau); the identity is exact.
  product     e_G = e_D |Y| + (B + 16) U24 (|D| |Y|): B accumulations of the stripe product, at most 8 slice additions, and 8 for the
              roundings of k and of the normalised rows Y.
  projection  e_da = (e_G + |a^| (|a^| . e_G) + (E + 32) U24 |a^| (|a^| . |G|) + 16 U24 (|G| + |a^| |a^ . G|)) / |a|
  scalars     L = sum of per-row values (lse_i - A_ii) / B; bound = n_acc U24 sum |terms| + the rows' own errors (e_lse + e_A_ii + U24 of
              the difference) + 4 U24 |L|; n_acc = 12 is the longest chain of additions of the fixed-order sum: 4 lane steps of a
              stripe's record, 6 steps of the wave sum over the records, 2 over the four waves.  icl adds the two halves and one rounding,
              out[0] the product with w.
tests/test_icl_cpu.py asserts that the same formulas evaluated in float32 on the CPU stay within HALF of every bound on every case.

Cases.  B in {1, 2, 15, 16, 17, 33, 40, 130} at E = 48 and 768, every E in {16, 48, 64, 256, 272, 512, 528, 768, 1024} at B = 17 and
130, each at tau = 0.01, 0.07 and 2: every stripe edge and every slice count `slices` gives up to nine tiles (B <= 16: 1 tile, 1
slice; 17: 2, 2, ONE column in the last tile; 33 and 40: 3, 3; 130: 9 tiles over 8 slices, the last slice has two), and E = 16 where
three of stripe B's four waves have no slab of the product.  Row norms spread over more than two decades (0.08 to 12 in every tensor
with two rows or more).  Three more families: near-orthogonal rows (every cosine within +-0.02) at tau = 0.01, where a maximum fixed
at 1 / tau = 100 would underflow every row; student rows equal to the paired teacher rows (loss near 0, the diagonal of D cancels);
all teacher text rows bit copies of one row (L_i2t = log B).  No slice of the sweep has more than two tiles, so two of the four waves of a
stripe workgroup stay idle in it: B = 340 (22 tiles over 5 slices of 4 and 5) and B = 512 at E = 512 (32 tiles over 4 slices, two tiles
per wave) give every wave statistics to merge.
"""
import functools
import math

import torch

U24 = 2.0 ** -24
XA = 8 * U24                                        # __expf / __logf allowance (tests/test_softmax_edges_gpu.py::_loss_tol)
TINY = 2.0 ** -126                                   # below it an f32 exp is a denormal or flushed to zero: absolute, not relative
F64 = torch.float64
B_LIST = (1, 2, 15, 16, 17, 33, 40, 130)
E_LIST = (16, 48, 64, 256, 272, 512, 528, 768, 1024)
SWEEP = sorted({(B, E) for B in (17, 130) for E in E_LIST} | {(B, E) for B in B_LIST for E in (48, 768)})
TAUS = (0.01, 0.07, 2.0)
MAX_B, MAX_E = 4096, 1024
N_ACC = 12                                           # longest addition chain of the scalars' fixed-order sum
KEYS = ('si', 'ti', 'st', 'tt')                      # the C entry's order: s_img, t_img, s_txt, t_txt


def slices(B):
    """column slices of the stripe kernels, as icl_slices of interactive.hip picks them"""
    tiles = (B + 15) // 16
    zs = min(max(256 // (2 * tiles), 1), 8, tiles)
    while zs < 8 and -(-tiles // zs) * 16 > 512:
        zs += 1
    return zs


def slice_tiles(B):
    """[(first tile, end tile)] of every column slice"""
    nt, zs = (B + 15) // 16, slices(B)
    return [(nt * z // zs, nt * (z + 1) // zs) for z in range(zs)]


def n_merge(B):
    return -(-max(t1 - t0 for t0, t1 in slice_tiles(B)) // 4) + 7 + slices(B)


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
    u = r()                                           # what an image and its caption share: the diagonals stand out
    zi, zt = u + r(), u + r()
    z = dict(si=zi, st=zt, ti=0.5 * zi + 0.3 * u + 0.7 * r(), tt=0.5 * zt + 0.3 * u + 0.7 * r())      # teacher correlated with student
    return {k: (z[k] * _scales(B, g)[:, None]).contiguous() for k in KEYS}


def _orthogonal(B, E, seed):
    """rows of four mutually orthogonal orthonormal sets plus a little noise: every cosine, the paired ones included, within +-0.02"""
    g = torch.Generator().manual_seed(seed)
    assert 4 * B <= E
    qm, _ = torch.linalg.qr(torch.randn(E, 4 * B, generator=g, dtype=F64))
    e = {}
    for i, k in enumerate(KEYS):
        rows = qm[:, i * B:(i + 1) * B].T + 0.08 * torch.randn(B, E, generator=g, dtype=F64) / math.sqrt(E)
        e[k] = (rows.float() * _scales(B, g)[:, None]).contiguous()
    return e


def _paired(B, E, seed):
    """student rows that are bit copies of the paired teacher rows of the OTHER modality, which they are contrasted against"""
    e = _draw(B, E, seed)
    e['si'], e['st'] = e['tt'].clone(), e['ti'].clone()
    return e


def _one_text(B, E, seed):
    """all teacher text rows bit copies of one row: every logit of a row of A is the same number, L_i2t = log B"""
    e = _draw(B, E, seed)
    e['tt'] = e['tt'][:1].repeat(B, 1).contiguous()
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
    return build(B, E, 7919 * B + E)


@functools.lru_cache(maxsize=None)
def _reference(build, B, E, tau):
    return Reference(_inputs(build, B, E), tau)


SWEEP_CASES = [Case(f'B{B}-E{E}-tau{tau:g}', B, E, tau, _draw) for B, E in SWEEP for tau in TAUS]
ORTHOGONAL = Case('orthogonal-B130-E768-tau0.01', 130, 768, 0.01, _orthogonal)
PAIRED = [Case(f'paired-B33-E48-tau{tau:g}', 33, 48, tau, _paired) for tau in (0.01, 0.07)]
ONE_TEXT = Case('one-text-row-B40-E48-tau0.07', 40, 48, 0.07, _one_text)
# slices of four tiles and more, where all four waves of a stripe workgroup hold statistics: 22 tiles over 5 slices, 32 over 4
FOUR_WAVES = [Case('four-waves-B340-E48-tau0.07', 340, 48, 0.07, _draw), Case('four-waves-B512-E512-tau0.01', 512, 512, 0.01, _draw)]
CASES = SWEEP_CASES + [ORTHOGONAL] + PAIRED + [ONE_TEXT] + FOUR_WAVES


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 reference with its bounds
# ----------------------------------------------------------------------------------------------------------------------------------
WRONGS = ('tile_lost', 'no_tau_in_grad', 'no_projection', 'slice_lost', 'neighbour_diag', 'wave_lost')


class Reference:
    """float64 values of one (inputs, tau, weight): out [4] with bounds out_b, gradients g[dir] [B, E] with bounds gb[dir], and per
    direction (0: student image against teacher text, 1: student text against teacher image) the logits X, log-sum-exps lse, P, D, G.
    `wrong` builds one of the wrong kernels of WRONGS instead (values only: the bounds stay those of the right one)."""

    def __init__(self, e32, tau, weight=1.0, wrong=None):
        assert wrong is None or wrong in WRONGS
        e = {k: v.to(F64) for k, v in e32.items()}
        self.B, self.E = B, E = e['si'].shape
        self.tau, self.weight = tau, weight
        nm = n_merge(B)
        eye = torch.eye(B, dtype=F64)
        cw = torch.ones(B, dtype=F64)                     # column weights of the wrong kernels
        if wrong == 'tile_lost':
            cw[16 * ((B + 15) // 16 - 1):] = 0.0
        gw = cw.clone()
        if wrong == 'wave_lost':                          # the fourth wave's tiles missing from the statistics, not from the product
            for t0, t1 in slice_tiles(B):
                for jt in range(t0 + 3, t1, 4):
                    cw[16 * jt:16 * jt + 16] = 0.0
        if wrong == 'slice_lost':
            t0, t1 = slice_tiles(B)[-1]
            gw[16 * t0:16 * t1] = 0.0
        self.X, self.lse, self.P, self.D, self.G, self.g, self.gb = [], [], [], [], [], [], []
        L, Lb = [], []
        for x, y in ((e['si'], e['tt']), (e['st'], e['ti'])):
            nx = x.norm(dim=1)
            xh, yh = x / nx[:, None], y / y.norm(dim=1, keepdim=True)
            X = xh @ yh.T / tau
            eX = (E + 2) * U24 * (xh.abs() @ yh.abs().T) / tau + 2 * U24 * X.abs()
            m = X.max(1, keepdim=True).values
            lse = (m + torch.log((torch.exp(X - m) * cw).sum(1, keepdim=True))).squeeze(1)
            P = torch.exp(X - lse[:, None])
            e_lse = (P * eX).sum(1) + nm * (8 + lse.abs()) * U24
            e_P = P * (eX + e_lse[:, None] + U24 * (X - lse[:, None]).abs() + XA) + TINY
            k = weight / (2 * B * (1.0 if wrong == 'no_tau_in_grad' else tau))
            D, eD = k * (P - eye), abs(weight / (2 * B * tau)) * e_P
            G = (D * gw) @ yh
            eG = eD @ yh.abs() + (B + 16) * U24 * (D.abs() @ yh.abs())
            dot = (xh * G).sum(1, keepdim=True)
            da = (G if wrong == 'no_projection' else G - xh * dot) / nx[:, None]
            xa = xh.abs()
            proj = lambda v: v + xa * (xa * v).sum(1, keepdim=True)
            e_da = (proj(eG) + (E + 32) * U24 * xa * (xa * G.abs()).sum(1, keepdim=True)
                    + 16 * U24 * (G.abs() + xa * dot.abs())) / nx[:, None]
            d = X[torch.arange(B), (torch.arange(B) + 4) % B] if wrong == 'neighbour_diag' else X.diagonal()      # the next row group's column
            rows = lse - d
            own = e_lse + eX.diagonal() + U24 * rows.abs()
            L.append(rows.sum() / B)
            Lb.append((N_ACC * U24 * rows.abs().sum() + own.sum()) / B + 4 * U24 * L[-1].abs())
            for lst, v in ((self.X, X), (self.lse, lse), (self.P, P), (self.D, D), (self.G, G), (self.g, da), (self.gb, e_da)):
                lst.append(v)
        icl = 0.5 * (L[0] + L[1])
        icl_b = 0.5 * (Lb[0] + Lb[1]) + 2 * U24 * icl.abs()
        self.out = torch.stack([weight * icl, icl, L[0], L[1]])
        self.out_b = torch.stack([abs(weight) * icl_b + 2 * U24 * (weight * icl).abs(), icl_b, Lb[0], Lb[1]])


def evaluate_f32(e32, tau, weight=1.0):
    """the formulas of the term in float32 on the CPU -> (out [4], [d a, d b]), as float64"""
    B = e32['si'].shape[0]
    L, g = [], []
    tau32 = torch.tensor(tau, dtype=torch.float32)
    k = torch.tensor(weight, dtype=torch.float32) * (0.5 / (B * tau32))
    for x, y in ((e32['si'], e32['tt']), (e32['st'], e32['ti'])):
        inv = 1.0 / x.norm(dim=1)
        xh, yh = x * inv[:, None], y / y.norm(dim=1, keepdim=True)
        X = (xh @ yh.T) * (1.0 / tau32)
        lse = torch.logsumexp(X, 1)
        L.append((lse - X.diagonal()).sum() / B)
        G = (k * (torch.exp(X - lse[:, None]) - torch.eye(B))) @ yh
        g.append(((G - xh * (xh * G).sum(1, keepdim=True)) * inv[:, None]).to(F64))
    icl = 0.5 * (L[0] + L[1])
    out = torch.stack([torch.tensor(weight, dtype=torch.float32) * icl, icl, L[0], L[1]])
    assert out.dtype == torch.float32
    return out.to(F64), g


def torch_autograd_f64(e32, tau):
    """cross_entropy on the two cross-logit matrices by torch autograd in float64 -> (icl, L_i2t, L_t2i, d a, d b)"""
    F = torch.nn.functional
    a, b = e32['si'].to(F64).requires_grad_(True), e32['st'].to(F64).requires_grad_(True)
    p, q = e32['ti'].to(F64), e32['tt'].to(F64)
    lab = torch.arange(a.shape[0])
    l0 = F.cross_entropy(F.normalize(a, dim=1, eps=0) @ F.normalize(q, dim=1, eps=0).T / tau, lab)
    l1 = F.cross_entropy(F.normalize(b, dim=1, eps=0) @ F.normalize(p, dim=1, eps=0).T / tau, lab)
    icl = 0.5 * (l0 + l1)
    icl.backward()
    return icl.detach(), l0.detach(), l1.detach(), a.grad, b.grad


def ratio(err, bound):
    """worst err / bound; an exact result counts 0 whatever its bound, a NaN counts inf"""
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.nan_to_num(q, nan=math.inf).max().item() if q.numel() else 0.0
