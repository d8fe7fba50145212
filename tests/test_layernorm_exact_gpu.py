"""LayerNorm forward and backward (csrc/layernorm.hip) element by element against float64, with an error model read off the kernels'
own operation order.  tests/test_layernorm_exact_cpu.py imports the builders, references and bounds of this file and checks, without a
GPU, the conditions they rest on (closed forms = float64 autograd, an honest f32 evaluation within half of every bound, every wrong
kernel of `WRONGS` outside some bound, the host's refusals).

Inputs.  One 64-row master matrix per (D, input type), drawn with a CPU generator; row r is of variant VARIANTS[r % 13], so every call
mixes families and a row processed with a neighbour's statistics is grossly wrong.  Rows draw their own scale in [0.5, 2]:
  plain    N(0.5, 2)                                 offset   N(0, 1) + c, |c| = 1e2, 1e3, 1e4 (fp16 at 1e4: N(0, 16), its ulp is 8 there)
  outlier  N(0, 1), one channel at +-1e3 in the first, a middle, the last 4-column group
  tiny     std 1e-4 (var << eps) and 3e-3 (var ~ eps)
  const    one value per row: small integers (D c exact in f32) and 0.1 k
  big      std 3e4 (f32 rows); fp16 rows over the whole fp16 range with +-65504, and one row of fp16 subnormals
A call takes M consecutive master rows from r0 (`SLICES`: M = 1 from every variant, M = 2..5 from three starts, 37 from two, 64).
gamma / beta: 'usual' (1 +- 0.1, +- 0.1), 'wide' (exact zeros, negatives, values around 10; beta around +-5) and, for the fp16 output,
'huge' (wide with some gamma at +-6e4, so that y leaves the fp16 range).

Forward error model (eps = 2^-24 = U24, g(n) = n eps / (1 - n eps), NV = ceil(D / 256) float4 chunks per lane):
  mu     each lane adds NV chunk sums (x + y) + (z + w): 3 adds per chunk and NV - 1 adds between chunks, the first `0 +` being exact,
         at most 4 NV - 1 roundings; 6 adds of the wave's xor tree; one correctly rounded division by D.  c_s = 4 NV + 6 and
         |dmu| <= g(c_s) mean|x|.
  var    a term is fl(fl(x - mu^)^2): 3 roundings, then the same sum and division: c_v = c_s + 3.  sum (x - mu^)^2 / D is exactly
         var + dmu^2, so |dvar| <= g(c_v) (var + dmu^2) + dmu^2.
  rstd   w = fl(var^ + eps): |dw| / (var + eps) <= T = dvar / (var + eps) (1 + U24) + U24; rsqrt moves that to (1 - T)^-1/2 - 1, and
         v_rsq_f32 is specified to 1 ulp: 2 ulp = 4 U24 are allowed.  rr = (1 + ((1 - T)^-1/2 - 1)) (1 + 4 U24) - 1 bounds |drstd| / rstd.
  y      fl(fl(fl(fl(x - mu^) rs^) gamma) + beta) (the last two may contract into one fma, which drops a rounding):
         |dy| <= [ |gamma| rstd (|dmu| + U24 |x - mu|) (1 + rr) (1 + U24)^3 + |gamma xhat| ((1 + rr) (1 + U24)^2 - 1) ] (1 + U24) + 2 U24 |y|.
         The last term is the one rounding of the sum with beta, given a FULL ulp as in the backward: where beta dominates, that rounding
         is the only error, and a correct kernel then sits at up to half an ulp, which is half of this bound.
         It grows with |mean| / std: that is f32 two-pass arithmetic, and the bound models it instead of hiding it in a flat tolerance.
  16-bit outputs are one RNE rounding of the f32-output call's result: bit equality, +-inf included.
  const rows with exact D c: mean == c and y == beta bit for bit, rstd within the rsqrt allowance of 1 / sqrt(eps).
The reference uses the f32 value of eps, which is what the kernel receives.

Backward error model, from the SAVED statistics (the f32 mu and rstd handed to the kernel enter the float64 closed form as they are, so
their rounding is not the kernel's error): X = (x - mu) rs, G = dy gamma, C1 = mean G, C2 = mean(G X), U = rs (G - C1 - X C2).
  xh has 2 roundings, g 1; C1: g(c_s + 1) mean|G|; C2: g(c_s + 4) mean|G X| (g, xh and their product, then the sum);
  inner = U24 (4 |G| + 3 |C1| + 6 |X C2|) + dC1 + |X| dC2 (the roundings of g - c1, xh c2, their difference and the product with rs);
  |d(acc - acc0)| <= rs inner (1 + 1e-6) + 2 U24 |acc|: the last term is the one rounding of the accumulated value, given a FULL ulp
  (where nothing else errs, a correct kernel is at half an ulp: half of this bound).
  dx_bf16 is RNE of the updated f32 row, bit for bit.  dgamma, dbeta, colsum: the sum-bound rule of test_glue_kernels_gpu.py,
  |got - ref| <= n 2^-23 sum|terms| with n = M + 1 (the non-zero start is a term); colsum's terms are the kernel's own updated rows.
Chained (the forward kernel's mean / rstd into the backward, against float64 autograd of F.layer_norm): the bound above, evaluated at the
kernel's statistics, plus the propagation of the forward's |dmu| and rr through xhat:
  eX = |X| rr' + rs |dmu| (1 + rr'), eC2 = mean(|G| eX), prop = rs (1 + rr') (eX |C2| + |X| eC2 + eX eC2) + rr' |U|, rr' = rr / (1 - rr)
  (X, C2, U, rs at the kernel's statistics; U(exact) - U(kernel's) expands into exactly these products); dgamma gains sum_rows |dy| eX.
  A statistic that is wrong but used consistently leaves this bound; it cannot leave the first.
Row sums across blocks leave as f32 atomics whose order is free, so the bit-for-bit comparisons of dgamma / dbeta / colsum between two
calls are made at M <= 8 (one block) only.

Measured on the MI355X, largest err / bound per checked quantity and family (this module prints the table at the end of a run; the
CPU file prints the honest-f32 ratios, which peak at mu 0.23, rstd 0.38, y 0.46, dx 0.50, dgamma 0.66 (M = 1; 0.46 from M = 2 on),
dbeta 0.31, colsum 0.33):
                        plain   offset  outlier     tiny    const      big      all
  mu                   0.1009   0.2302   0.1690   0.1310   0.0694   0.0225        -
  rstd                 0.1409   0.1475   0.1756   0.2940   0.2041   0.3278        -
  y                    0.4155   0.3016   0.4449   0.4506   0.1159   0.4618        -
  dx                   0.3550   0.3476   0.4837   0.3596   0.3032   0.4990        -
  dx chained           0.2687   0.1962   0.4698   0.2520   0.2530   0.4987        -
  dgamma                    -        -        -        -        -        -   0.6617
  dbeta                     -        -        -        -        -        -   0.3072
  colsum                    -        -        -        -        -        -   0.3383
  dgamma chained            -        -        -        -        -        -   0.2301
mu agrees with the lane-order f32 restatement of the CPU file to every digit shown.  dgamma's 0.66 is the M = 1 case, where the sum-bound
rule (4 U24) is exactly the four roundings a correct kernel makes.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
U23 = 2.0 ** -23
F64 = torch.float64
F32 = torch.float32

D_LIST = (4, 100, 128, 252, 256, 260, 516, 768, 772, 1020, 1024)
M_LIST = (1, 2, 3, 4, 5, 37, 64)
EPS_LIST = (1e-5, 1e-6)
NROWS = 64
VARIANTS = ('plain', 'offset_1e2', 'offset_1e3', 'offset_1e4', 'outlier_first', 'outlier_mid', 'outlier_last', 'tiny_1e-4', 'tiny_3e-3',
            'const_int', 'const_tenth', 'big', 'sub')
FAMILIES = ('plain', 'offset', 'outlier', 'tiny', 'const', 'big')
SLICES = tuple([(1, r0) for r0 in range(len(VARIANTS))] + [(M, r0) for M in (2, 3, 4, 5) for r0 in (0, 5, 10)] + [(37, 0), (37, 27), (64, 0)])
BIG_CASES = ((2049, 260, torch.bfloat16), (4101, 1020, torch.float32))       # the persistent grid with the hard-row mix
STRIDED_D = (100, 260)
GAP = 28
OUT_CODE = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}


def variant(r, f16):
    v = VARIANTS[r % len(VARIANTS)]
    return 'plain' if v == 'sub' and not f16 else v


def family(r, f16):
    v = variant(r, f16)
    return 'big' if v == 'sub' else v.split('_')[0]


def fam_ids(rows, f16):
    return torch.tensor([FAMILIES.index(family(int(r), f16)) for r in rows])


def g_(n):
    return n * U24 / (1 - n * U24)


def c_s(D):
    return 4 * ((D + 255) // 256) + 6


def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def outlier_col(v, D):
    return {'outlier_first': min(1, D - 1), 'outlier_mid': 4 * (D // 8) + 2, 'outlier_last': D - 1}[v]


@functools.lru_cache(maxsize=None)
def master(D, f16):
    """[64, D] rows of x (f32, or fp16), row r of variant(r); a CPU tensor that nothing modifies"""
    g = _gen(20261019 + 2 * D + int(f16))
    z = torch.randn(NROWS, D, generator=g, dtype=F64)
    s = 0.5 + 1.5 * torch.rand(NROWS, 1, generator=g, dtype=F64)
    x = torch.empty(NROWS, D, dtype=F64)
    for r in range(NROWS):
        v, k, sg = variant(r, f16), r // len(VARIANTS), (-1.0) ** r
        if v == 'plain':
            x[r] = s[r] * (2 * z[r] + 0.5)
        elif v.startswith('offset'):
            c = float(v.split('_')[1])
            x[r] = s[r] * z[r] * (16 if f16 and c == 1e4 else 1) + sg * c       # fp16 has ulp 8 at 1e4: N(0, 1) would round to a constant row
        elif v.startswith('outlier'):
            x[r] = s[r] * z[r]
            x[r, outlier_col(v, D)] = sg * 1e3
        elif v.startswith('tiny'):
            x[r] = s[r] * float(v.split('_')[1]) * z[r]
        elif v == 'const_int':
            x[r] = sg * (1 + k)
        elif v == 'const_tenth':
            x[r] = sg * 0.1 * (1 + k)
        elif v == 'big' and not f16:
            x[r] = s[r] * 3e4 * z[r]
        elif v == 'big':
            x[r] = (s[r] * 2.5e4 * z[r]).clamp(-65504, 65504)
            x[r, 0], x[r, D - 1] = 65504.0, -65504.0
        else:                                                   # 'sub': fp16 subnormals k 2^-24, |k| < 1024
            x[r] = torch.randint(-1023, 1024, (D,), generator=g).double() * 2.0 ** -24
    return x.to(torch.float16 if f16 else F32)


@functools.lru_cache(maxsize=None)
def affine(D, kind):
    """(gamma, beta) f32 [D]: 'usual', 'wide' (zeros, negatives, around 10; beta around +-5), 'huge' (wide, some gamma at +-6e4)"""
    g = _gen(77 + D)
    z, w = torch.randn(D, generator=g, dtype=F64), torch.randn(D, generator=g, dtype=F64)
    c = torch.arange(D)
    if kind == 'usual':
        return (1 + 0.1 * z).float(), (0.1 * w).float()
    gamma = torch.where(c % 3 == 0, 10 + z, torch.where(c % 3 == 1, -1 + 0.3 * z, z))
    gamma[c % 5 == 0] = 0.0
    if kind == 'huge':
        gamma[c % 7 == 3] = 6e4 * torch.where(c % 2 == 0, 1.0, -1.0)[c % 7 == 3].double()
    beta = torch.where(c % 2 == 0, 5.0, -5.0) + 0.3 * w
    return gamma.float(), beta.float()


@functools.lru_cache(maxsize=None)
def grads(D, bf16):
    """masters of the backward's other inputs: dy [64, D] (f32 or bf16, rows with their own scale), acc0 [64, D], dgamma / dbeta / colsum starts"""
    g = _gen(4242 + 2 * D + int(bf16))
    dy = torch.randn(NROWS, D, generator=g) * (0.25 + 3 * torch.rand(NROWS, 1, generator=g))
    acc0 = torch.randn(NROWS, D, generator=g)
    starts = tuple(torch.randn(D, generator=g) for _ in range(3))
    return dy.to(torch.bfloat16 if bf16 else F32), acc0, starts


def f32_eps(eps):
    return float(np.float32(eps))


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 references (device-agnostic torch; `wrong` names one of WRONGS)
# ----------------------------------------------------------------------------------------------------------------------------------
FWD_WRONGS = ('one_pass_variance', 'divisor_d_minus_1', 'eps_outside_sqrt', 'padded_divisor', 'tail_chunk_lost', 'neighbour_stats',
              'affine_4_columns_off', 'bf16_truncation')
BWD_WRONGS = ('c1_from_dy', 'projection_dropped', 'projection_sign', 'dgamma_from_g', 'colsum_of_update', 'idle_wave_stale')
WRONGS = FWD_WRONGS + BWD_WRONGS


def fwd_eval(x, gamma, beta, eps, wrong=None):
    """(mean, rstd, y) in float64 of the rows x [M, D] (the f32 / fp16 values the kernel reads), eps the f32 value; or what a kernel with
    the named mistake gives"""
    M, D = x.shape
    nv = (D + 255) // 256
    x32, x, g, b = x.float(), x.double(), gamma.double(), beta.double()
    xs, div = x, D
    if wrong == 'padded_divisor':
        div = 256 * nv
    if wrong == 'tail_chunk_lost' and D % 256:
        xs = x[:, :256 * (nv - 1)]
    mu = xs.sum(1) / div
    if wrong == 'one_pass_variance':                            # the mistake is one of precision: it is made in f32
        var = ((x32 * x32).sum(1) / D - (x32.sum(1) / D) ** 2).double()
    else:
        var = ((xs - mu[:, None]) ** 2).sum(1) / div
    if wrong == 'divisor_d_minus_1':
        var = var * D / (D - 1)
    rstd = 1 / (var.sqrt() + eps) if wrong == 'eps_outside_sqrt' else 1 / (var + eps).sqrt()
    if wrong == 'neighbour_stats':
        mu, rstd = mu.roll(1), rstd.roll(1)
    if wrong == 'affine_4_columns_off':
        g, b = g.roll(-4), b.roll(-4)
    return mu, rstd, (x - mu[:, None]) * rstd[:, None] * g + b


class FwdRef:
    """float64 forward of the whole master for one (D, input type, gamma / beta kind, eps), with the per-row / per-element bounds"""

    def __init__(self, D, f16, kind, eps):
        self.D, self.f16, self.kind, self.eps = D, f16, kind, f32_eps(eps)
        self.x = master(D, f16)
        self.gamma, self.beta = affine(D, kind)
        x, g = self.x.double(), self.gamma.double()
        self.mu, self.rstd, self.y = fwd_eval(self.x, self.gamma, self.beta, self.eps)
        self.var = ((x - self.mu[:, None]) ** 2).mean(1)
        cs = c_s(D)
        self.mu_b = g_(cs) * x.abs().mean(1)
        self.var_b = g_(cs + 3) * (self.var + self.mu_b ** 2) + self.mu_b ** 2
        self.T = self.var_b / (self.var + self.eps) * (1 + U24) + U24
        self.rr = (1 - self.T) ** -0.5 * (1 + 4 * U24) - 1
        self.rstd_b = self.rr * self.rstd
        rr, rs, dmu = self.rr[:, None], self.rstd[:, None], self.mu_b[:, None]
        cen = (x - self.mu[:, None]).abs()
        a = g.abs() * rs * (dmu + U24 * cen) * (1 + rr) * (1 + U24) ** 3
        b = (g * cen * rs).abs() * ((1 + rr) * (1 + U24) ** 2 - 1)
        self.y_b = (a + b) * (1 + U24) + 2 * U24 * self.y.abs() + 2.0 ** -149


@functools.lru_cache(maxsize=None)
def fwd_ref(D, f16, kind, eps):
    return FwdRef(D, f16, kind, eps)


class BwdRef:
    """float64 backward of the rows given, from the f32 statistics given, with bounds; `wrong` evaluates a mistaken kernel instead"""

    def __init__(self, x, gamma, mu, rs, dy, acc0, starts, wrong=None):
        M, D = x.shape
        x, g, mu, rs, d, a0 = x.double(), gamma.double(), mu.double()[:, None], rs.double()[:, None], dy.double(), acc0.double()
        dg0, db0, cs0 = (s.double() for s in starts)
        X, G = (x - mu) * rs, d * g
        C1 = (d if wrong == 'c1_from_dy' else G).mean(1, keepdim=True)
        C2 = (G * X).mean(1, keepdim=True)
        proj = {'projection_dropped': 0.0, 'projection_sign': -1.0}.get(wrong, 1.0) * X * C2
        self.U = rs * (G - C1 - proj)
        self.acc = a0 + self.U
        self.X, self.G, self.C2, self.rs, self.d = X, G, C2, rs, d
        cs = c_s(D)
        e1, e2 = g_(cs + 1) * G.abs().mean(1, keepdim=True), g_(cs + 4) * (G * X).abs().mean(1, keepdim=True)
        inner = U24 * (4 * G.abs() + 3 * C1.abs() + 6 * (X * C2).abs()) + e1 + X.abs() * e2
        self.U_b = rs * inner * (1 + 1e-6) + 2 * U24 * self.acc.abs() + 2.0 ** -149
        tg = (G if wrong == 'dgamma_from_g' else d) * X
        self.dgamma, self.dgamma_b = dg0 + tg.sum(0), (M + 1) * U23 * (dg0.abs() + tg.abs().sum(0))
        self.dbeta, self.dbeta_b = db0 + d.sum(0), (M + 1) * U23 * (db0.abs() + d.abs().sum(0))
        self.cs0 = cs0
        self.colsum, self.colsum_b = self.colsum_of(self.U if wrong == 'colsum_of_update' else self.acc)
        if wrong == 'idle_wave_stale':                          # the waves of the last block that have no row add wave 0's partials again
            idle = -M % 8
            self.dgamma, self.dbeta, self.colsum = self.dgamma + idle * tg[0], self.dbeta + idle * d[0], self.colsum + idle * self.acc[0]

    def colsum_of(self, rows):
        """colsum and its bound from updated rows: the reference's own, or (on the GPU) the kernel's f32 rows, which are its exact terms"""
        rows = rows.double()
        return self.cs0 + rows.sum(0), (rows.shape[0] + 1) * U23 * (self.cs0.abs() + rows.abs().sum(0))

    def propagation(self, fr, rows):
        """what the forward's |dmu| and rr (FwdRef `fr`, master rows `rows`) add to the bounds of U and dgamma when the kernel's own
        statistics replace the exact ones"""
        rr, dmu = fr.rr[rows][:, None].to(self.X.device), fr.mu_b[rows][:, None].to(self.X.device)
        rr = rr / (1 - rr)                                       # this reference stands at the kernel's statistics: exact rs = rs^ (1 + rho')
        eX = self.X.abs() * rr + self.rs * dmu * (1 + rr)
        eC2 = (self.G.abs() * eX).mean(1, keepdim=True)
        return (self.rs * (1 + rr) * (eX * self.C2.abs() + self.X.abs() * eC2 + eX * eC2) + rr * self.U.abs(),
                (1 + (self.X.shape[0] + 1) * U23) * (self.d.abs() * eX).sum(0))


def bwd_case(D, bf16, kind, M, r0, wrong=None, eps=1e-5):
    """the backward reference of one SLICES case from the f32 roundings of the exact statistics"""
    fr = fwd_ref(D, False, kind, eps)
    dy, acc0, starts = grads(D, bf16)
    rows = slice(r0, r0 + M)
    return BwdRef(fr.x[rows], fr.gamma, fr.mu[rows].float(), fr.rstd[rows].float(), dy[rows], acc0[rows], starts, wrong)


def outside(got, want, bound):
    """does `got` leave the bound somewhere, or hold a non-finite value"""
    got = got.double()
    return bool((~torch.isfinite(got)).any() or ((got - want).abs() > bound).any())


def fwd_leaves(fr, rows, mu, rstd, y):
    """the first forward quantity of (mu, rstd, y), given for the master rows `rows`, that leaves its bound; None if all stay inside"""
    for what, got, want, bound in (('mu', mu, fr.mu, fr.mu_b), ('rstd', rstd, fr.rstd, fr.rstd_b), ('y', y, fr.y, fr.y_b)):
        if outside(got, want[rows], bound[rows]):
            return what
    return None


def bwd_leaves(ref, other):
    for what in ('U', 'dgamma', 'dbeta', 'colsum'):
        if outside(getattr(other, what), getattr(ref, what), getattr(ref, what + '_b')):
            return what
    return None


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.view({F32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[t.dtype])


def _ones(shape, dtype):
    """a buffer of all-ones bits: a NaN in every float type, and the sentinel of the gap columns"""
    return torch.full(shape, -1, dtype=_bits(torch.empty(0, dtype=dtype)).dtype, device='cuda').view(dtype)


def _padded(t, ld, fill_nan=True):
    """t [M, D] in a [M, ld] buffer on the GPU, as the view [:, :D]; the gap holds NaN (an input) or the sentinel (an output)"""
    M, D = t.shape
    buf = torch.full((M, ld), math.nan, dtype=t.dtype, device='cuda') if fill_nan else _ones((M, ld), t.dtype)
    buf[:, :D] = t.cuda()
    return buf[:, :D]


def _gap_untouched(view, ld):
    M, D = view.shape
    whole = torch.as_strided(view, (M, ld), (ld, 1))
    return bool((_bits(whole[:, D:]) == -1).all())


def run_fwd(x, gamma, beta, eps, out_dtype, M=None, ridx=None, stats=True, ldy=None):
    """one forward call: x a GPU view [Mx, D] with any row stride; outputs pre-filled with all-ones bits.  -> (y view [M, D], mean, rstd)"""
    D = x.shape[1]
    M = M or (ridx.numel() if ridx is not None else x.shape[0])
    ybuf = _ones((M, ldy or D), out_dtype)
    mean, rstd = (_ones((M,), F32), _ones((M,), F32)) if stats else (None, None)
    fn = _lib().dclip_layernorm_fwd_f16 if x.dtype == torch.float16 else _lib().dclip_layernorm_fwd
    fn(_p(x), x.stride(0), _p(ridx), _p(gamma), _p(beta), _p(ybuf), ybuf.stride(0), OUT_CODE[out_dtype], _p(mean), _p(rstd), M, D, eps, _st())
    return ybuf[:, :D], mean, rstd


def run_bwd(dy, x, gamma, mean, rstd, acc, dxb=None, dg=None, db=None, cs=None, ridx=None):
    """one backward call on GPU views (any row strides); acc, dxb, dg, db, cs are updated in place"""
    M, D = dy.shape
    _lib().dclip_layernorm_bwd(_p(dy), dy.stride(0), 1 if dy.dtype == F32 else 0, _p(x), x.stride(0), _p(ridx), _p(gamma), _p(mean), _p(rstd),
                               _p(acc), acc.stride(0), _p(dxb), dxb.stride(0) if dxb is not None else 0, _p(dg), _p(db), _p(cs), M, D, _st())


WORST = {}                                           # (quantity, family) -> worst err / bound of this process


def within(what, got, want, bound, fams=None, label=''):
    """NaN fails: finiteness first.  Then |got - want| <= bound per element; records the worst err / bound per family (`fams`: the
    family id of each row; None for a per-column quantity)"""
    got, want, bound = got.double().cpu(), want.cpu(), bound.cpu()
    assert got.shape == want.shape == bound.shape, (what, label, got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all(), (what, label, 'non-finite values', int((~torch.isfinite(got)).sum()))
    err = (got - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if fams is None:
        WORST[(what, 'all')] = max(WORST.get((what, 'all'), 0.0), q.max().item())
    else:
        rowq = q.reshape(q.shape[0], -1).max(1).values
        for f in fams.unique().tolist():
            key = (what, FAMILIES[f])
            WORST[key] = max(WORST.get(key, 0.0), rowq[fams == f].max().item())
    bad = err > bound
    assert not bad.any(), (what, label, int(bad.sum()), 'of', bad.numel(), 'first at', torch.nonzero(bad)[0].tolist(), 'worst err / bound', q.max().item())


def exact(got, want, what=''):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got.contiguous()) != _bits(want.contiguous())
    assert not bad.any(), (what, int(bad.sum()), 'first at', torch.nonzero(bad)[0].tolist())


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    quantities = ('mu', 'rstd', 'y', 'dx', 'dx chained', 'dgamma', 'dbeta', 'colsum', 'dgamma chained')
    print('\nworst err / bound   ' + ''.join(f'{f:>9s}' for f in FAMILIES + ('all',)))
    for what in quantities:
        cells = [WORST.get((what, f)) for f in FAMILIES + ('all',)]
        if any(c is not None for c in cells):
            print(f'{what:20s}' + ''.join('        -' if c is None else f'{c:9.4f}' for c in cells))


def check_fwd(fr, rows, y, mean, rstd, label):
    """the f32 output and the statistics of one call whose output row i is master row rows[i]"""
    rows = torch.as_tensor(rows)
    fams = fam_ids(rows, fr.f16)
    within('mu', mean, fr.mu[rows], fr.mu_b[rows], fams, label)
    within('rstd', rstd, fr.rstd[rows], fr.rstd_b[rows], fams, label)
    within('y', y, fr.y[rows], fr.y_b[rows], fams, label)
    mean, rstd, y = mean.cpu(), rstd.cpu(), y.cpu()
    for i, r in enumerate(rows.tolist()):
        if variant(r, fr.f16) == 'const_int':                   # var^ = 0 and 0 + eps is exact: only the rsqrt allowance is left
            assert mean[i].item() == fr.x[r, 0].item(), (label, 'mean of a constant row', r, mean[i].item())
            assert abs(rstd[i].item() * math.sqrt(fr.eps) - 1) <= 4 * U24, (label, 'rstd of a constant row', r, rstd[i].item())
            assert torch.equal(_bits(y[i].contiguous()), _bits(fr.beta)), (label, 'y of a constant row is not beta', r)


def check_bwd(ref, fams, got_acc, acc0, dxb, dg, db, cs, label):
    """one backward call's outputs on its M rows against the saved-statistics reference `ref`; an absent output is None"""
    within('dx', got_acc.double() - acc0.double(), ref.U, ref.U_b, fams, label)
    if dxb is not None:
        exact(dxb, got_acc.bfloat16(), label + ': bf16 copy of the updated row')
    if dg is not None:
        within('dgamma', dg, ref.dgamma, ref.dgamma_b, None, label)
        within('dbeta', db, ref.dbeta, ref.dbeta_b, None, label)
    if cs is not None:
        want, bound = ref.colsum_of(got_acc)
        within('colsum', cs, want, bound, None, label)


# ----------------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('D', D_LIST)
def test_forward_statistics_and_output(D, f16):
    """mean, rstd and the f32 output of every SLICES case, both gamma / beta kinds, both eps, inside their bounds; constant rows exact"""
    xm = master(D, f16).cuda()
    for kind in ('usual', 'wide'):
        gamma, beta = (t.cuda() for t in affine(D, kind))
        for eps in EPS_LIST:
            fr = fwd_ref(D, f16, kind, eps)
            for M, r0 in SLICES:
                y, mean, rstd = run_fwd(xm[r0:r0 + M], gamma, beta, eps, F32)
                check_fwd(fr, range(r0, r0 + M), y, mean, rstd, f'D={D} {kind} eps={eps} M={M} r0={r0}')


@pytest.mark.gpu
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('D', D_LIST)
def test_forward_16_bit_outputs_and_absent_statistics(D, f16):
    """the bf16 (and, from fp16 rows, f16) output is the RNE rounding of the f32-output call's result, +-inf included ('huge' gamma on
    the big rows); mean = rstd = NULL gives the same output bits"""
    xm = master(D, f16).cuda()
    for kind in ('usual', 'wide', 'huge'):
        gamma, beta = (t.cuda() for t in affine(D, kind))
        fr = fwd_ref(D, f16, kind, 1e-5)
        for M, r0 in ((64, 0), (3, 10), (1, 11)):
            y32, mean, rstd = run_fwd(xm[r0:r0 + M], gamma, beta, 1e-5, F32)
            check_fwd(fr, range(r0, r0 + M), y32, mean, rstd, f'D={D} {kind} M={M}')
            y32n, _, _ = run_fwd(xm[r0:r0 + M], gamma, beta, 1e-5, F32, stats=False)
            exact(y32n, y32, 'f32 output without statistics')
            for dt in (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,):
                y16, m16, r16 = run_fwd(xm[r0:r0 + M], gamma, beta, 1e-5, dt)
                exact(y16, y32.to(dt), f'D={D} {kind} M={M} {dt}: one RNE rounding of the f32 output')
                exact(m16, mean, 'mean'), exact(r16, rstd, 'rstd')
                y16n, _, _ = run_fwd(xm[r0:r0 + M], gamma, beta, 1e-5, dt, stats=False)
                exact(y16n, y16, '16-bit output without statistics')
                if dt == torch.float16 and kind == 'huge' and M == 64 and D >= 100:
                    big = [r for r in range(64) if variant(r, True) == 'big']
                    assert torch.isinf(y16[big]).any() and (y16[big] == math.inf).any() and (y16[big] == -math.inf).any()


@pytest.mark.gpu
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('D', (100, 772))
def test_forward_row_index(D, f16):
    """row_index in reversed order, with a repeated index: output row i is LN(x[row_index[i]])"""
    rows = list(range(62, -1, -2)) + [7, 7, 3, 7]
    xm, ridx = master(D, f16).cuda(), torch.tensor(rows, dtype=torch.int32).cuda()
    for kind in ('usual', 'wide'):
        gamma, beta = (t.cuda() for t in affine(D, kind))
        y, mean, rstd = run_fwd(xm, gamma, beta, 1e-5, F32, ridx=ridx)
        check_fwd(fwd_ref(D, f16, kind, 1e-5), rows, y, mean, rstd, f'D={D} {kind} row_index')
        yb, _, _ = run_fwd(xm, gamma, beta, 1e-5, torch.bfloat16, ridx=ridx)
        exact(yb, y.bfloat16(), 'bf16 output with row_index')


@pytest.mark.gpu
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('D', STRIDED_D)
def test_forward_strided(D, f16):
    """ldx = ldy = D + 28: NaN in the gap columns of x must not reach the sums, the sentinel in the gap columns of y must stay"""
    ld = D + GAP
    gamma, beta = (t.cuda() for t in affine(D, 'wide'))
    fr = fwd_ref(D, f16, 'wide', 1e-5)
    for M, r0 in ((5, 9), (37, 27)):
        x = _padded(master(D, f16)[r0:r0 + M], ld)
        for dt in (F32, torch.bfloat16):
            y, mean, rstd = run_fwd(x, gamma, beta, 1e-5, dt, ldy=ld)
            assert _gap_untouched(y, ld), (D, M, dt, 'gap columns of y were written')
            if dt == F32:
                check_fwd(fr, range(r0, r0 + M), y, mean, rstd, f'D={D} M={M} strided')
                y32 = y
            else:
                exact(y.contiguous(), y32.bfloat16(), 'strided bf16 output')


# ----------------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------------
def _bwd_call(x, gamma, mean, rstd, dy, acc0, starts, absent=()):
    """a backward call from non-zero starts, dx_bf16 pre-filled with all-ones bits -> its outputs by name, None for those in `absent`"""
    out = dict(acc=acc0.clone(), dxb=_ones(tuple(acc0.shape), torch.bfloat16), dg=starts[0].clone(), db=starts[1].clone(), cs=starts[2].clone())
    for k in absent:
        out[k] = None
    run_bwd(dy, x, gamma, mean, rstd, out['acc'], out['dxb'], out['dg'], out['db'], out['cs'])
    return out


def _bwd_all_outputs(x, gamma, mean, rstd, dy, acc0, starts, label, fams):
    """a backward call with every output on, checked against the saved-statistics reference -> (reference, outputs)"""
    out = _bwd_call(x, gamma, mean, rstd, dy, acc0, starts)
    ref = BwdRef(x, gamma, mean, rstd, dy, acc0, starts)
    check_bwd(ref, fams, out['acc'], acc0, out['dxb'], out['dg'], out['db'], out['cs'], label)
    return ref, out


@pytest.mark.gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['dy_f32', 'dy_bf16'])
@pytest.mark.parametrize('D', D_LIST)
def test_backward_from_saved_statistics(D, bf16):
    """dx update, its bf16 copy, dgamma, dbeta and colsum of every SLICES case (M < 8 leaves waves without a row), both gamma kinds"""
    dym, acc0m, starts = grads(D, bf16)
    dym, acc0m, starts = dym.cuda(), acc0m.cuda(), tuple(s.cuda() for s in starts)
    xm = master(D, False).cuda()
    for kind in ('usual', 'wide'):
        fr = fwd_ref(D, False, kind, 1e-5)
        gamma, mu32, rs32 = fr.gamma.cuda(), fr.mu.float().cuda(), fr.rstd.float().cuda()
        for M, r0 in SLICES:
            s = slice(r0, r0 + M)
            _bwd_all_outputs(xm[s], gamma, mu32[s].clone(), rs32[s].clone(), dym[s], acc0m[s], starts,
                             f'D={D} {kind} M={M} r0={r0}', fam_ids(range(r0, r0 + M), False))


@pytest.mark.gpu
@pytest.mark.parametrize('M,D,dy_dtype', BIG_CASES)
def test_backward_persistent_grid_hard_rows(M, D, dy_dtype):
    """the persistent grid (waves with 2 and 3 rows) on the hard-row mix: row i is master row i % 64"""
    fr = fwd_ref(D, False, 'wide', 1e-5)
    rows = torch.arange(M) % NROWS
    g = _gen(M + D)
    dy = (torch.randn(M, D, generator=g) * (0.25 + 3 * torch.rand(M, 1, generator=g))).to(dy_dtype).cuda()
    acc0 = torch.randn(M, D, generator=g).cuda()
    starts = tuple(s.cuda() for s in grads(D, False)[2])
    _bwd_all_outputs(fr.x[rows].cuda(), fr.gamma.cuda(), fr.mu.float()[rows].cuda(), fr.rstd.float()[rows].cuda(), dy, acc0, starts,
                     f'M={M} D={D}', fam_ids(rows, False))


@pytest.mark.gpu
@pytest.mark.parametrize('D', (100, 772))
def test_backward_absent_outputs(D):
    """the combinations encoder.cpp uses: no colsum; no dgamma / dbeta; no dx_bf16.  dx_acc and dx_bf16 keep their bits; dgamma, dbeta
    and colsum keep theirs at M <= 8 (one block: no free atomic order) and stay inside their bounds at M = 37"""
    dym, acc0m, starts = grads(D, True)
    fr = fwd_ref(D, False, 'wide', 1e-5)
    xm, gamma = fr.x.cuda(), fr.gamma.cuda()
    starts = tuple(s.cuda() for s in starts)
    for M, r0 in ((3, 9), (8, 0), (37, 27)):
        s = slice(r0, r0 + M)
        x, dy, acc0, mu, rs = xm[s], dym[s].cuda(), acc0m[s].cuda(), fr.mu.float()[s].cuda(), fr.rstd.float()[s].cuda()
        fams = fam_ids(range(r0, r0 + M), False)
        ref, full = _bwd_all_outputs(x, gamma, mu, rs, dy, acc0, starts, f'D={D} M={M} all outputs', fams)
        for absent in (('cs',), ('dg', 'db'), ('dxb',)):
            out = _bwd_call(x, gamma, mu, rs, dy, acc0, starts, absent)
            check_bwd(ref, fams, out['acc'], acc0, out['dxb'], out['dg'], out['db'], out['cs'], f'D={D} M={M} without {absent}')
            for k in ('acc', 'dxb') + (('dg', 'db', 'cs') if M <= 8 else ()):
                if out[k] is not None:
                    exact(out[k], full[k], f'D={D} M={M} without {absent}: {k}')


@pytest.mark.gpu
@pytest.mark.parametrize('D', (100, 772))
def test_backward_row_index(D):
    """row_index with distinct rows: dy row i updates dx row row_index[i]; the rows outside it stay bit-unchanged in dx_acc and dx_bf16"""
    rows = [63, 0, 31, 9, 10, 40, 2, 55, 22, 21, 20]
    M, ridx = len(rows), torch.tensor(rows, dtype=torch.int32).cuda()
    dym, acc0m, starts = grads(D, True)
    fr = fwd_ref(D, False, 'wide', 1e-5)
    xm, gamma, dy, acc0 = fr.x.cuda(), fr.gamma.cuda(), dym[:M].cuda(), acc0m.cuda()
    mu, rs = fr.mu.float()[rows].cuda(), fr.rstd.float()[rows].cuda()
    acc, dxb = acc0.clone(), _ones((NROWS, D), torch.bfloat16)
    dg, db, cs = (s.cuda() for s in starts)
    starts = tuple(t.clone() for t in (dg, db, cs))
    run_bwd(dy, xm, gamma, mu, rs, acc, dxb, dg, db, cs, ridx=ridx)
    ref = BwdRef(xm[rows], gamma, mu, rs, dy, acc0[rows], starts)
    check_bwd(ref, fam_ids(rows, False), acc[rows], acc0[rows], dxb[rows], dg, db, cs, f'D={D} row_index')
    other = torch.ones(NROWS, dtype=torch.bool, device='cuda')
    other[rows] = False
    exact(acc[other], acc0[other], 'dx_acc rows outside row_index')
    assert (_bits(dxb[other]) == -1).all(), 'dx_bf16 rows outside row_index were written'


@pytest.mark.gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['dy_f32', 'dy_bf16'])
@pytest.mark.parametrize('D', STRIDED_D)
def test_backward_strided(D, bf16):
    """lddy, ldx, lddx, lddb larger than D and all different: NaN in the gaps of dy and x is not read into a sum, the sentinel in the gaps
    of dx_acc and dx_bf16 stays"""
    dym, acc0m, starts = grads(D, bf16)
    fr = fwd_ref(D, False, 'wide', 1e-5)
    starts = tuple(s.cuda() for s in starts)
    for M, r0 in ((5, 9), (37, 27)):
        s = slice(r0, r0 + M)
        dy, x = _padded(dym[s], D + GAP), _padded(fr.x[s], D + 12)
        acc, dxb = _padded(acc0m[s], D + 4, fill_nan=False), _padded(torch.zeros(M, D, dtype=torch.bfloat16), D + 20, fill_nan=False)
        _bits(dxb)[:] = -1
        dg, db, cs = (t.clone() for t in starts)
        mu, rs = fr.mu.float()[s].cuda(), fr.rstd.float()[s].cuda()
        run_bwd(dy, x, fr.gamma.cuda(), mu, rs, acc, dxb, dg, db, cs)
        assert _gap_untouched(acc, D + 4) and _gap_untouched(dxb, D + 20), (D, M, 'gap columns of an output were written')
        acc0 = acc0m[s].cuda()
        ref = BwdRef(fr.x[s].cuda(), fr.gamma.cuda(), mu, rs, dym[s].cuda(), acc0, starts)
        check_bwd(ref, fam_ids(range(r0, r0 + M), False), acc.contiguous(), acc0, dxb.contiguous(), dg, db, cs, f'D={D} M={M} strided')


@pytest.mark.gpu
@pytest.mark.parametrize('D', D_LIST)
def test_backward_chained_to_forward_against_autograd(D):
    """the forward kernel's own mean / rstd go into the backward; the result is held to float64 autograd of F.layer_norm on the same x,
    gamma and dy, within the saved-statistics bound plus the propagation of the forward's error bounds"""
    dym, acc0m, starts = grads(D, False)
    dym, acc0m, starts = dym.cuda(), acc0m.cuda(), tuple(s.cuda() for s in starts)
    xm = master(D, False).cuda()
    for kind in ('usual', 'wide'):
        fr = fwd_ref(D, False, kind, 1e-5)
        gamma, beta = fr.gamma.cuda(), fr.beta.cuda()
        for M, r0 in ((1, 0), (1, 3), (3, 9), (5, 0), (37, 27), (64, 0)):
            s = slice(r0, r0 + M)
            _, mean, rstd = run_fwd(xm[s], gamma, beta, 1e-5, torch.bfloat16)
            acc, dg, db = acc0m[s].clone(), starts[0].clone(), starts[1].clone()
            run_bwd(dym[s], xm[s], gamma, mean, rstd, acc, None, dg, db, None)
            xr, gr = xm[s].double().requires_grad_(True), gamma.double().requires_grad_(True)
            br = torch.zeros(D, dtype=F64, device='cuda', requires_grad=True)
            F.layer_norm(xr, (D,), gr, br, fr.eps).backward(dym[s].double())
            at_kernel = BwdRef(xm[s], gamma, mean, rstd, dym[s], acc0m[s], starts)
            pu, pg = at_kernel.propagation(fr, torch.arange(r0, r0 + M))
            label, fams = f'D={D} {kind} M={M} r0={r0} chained', fam_ids(range(r0, r0 + M), False)
            within('dx chained', acc.double() - acc0m[s].double(), xr.grad, at_kernel.U_b + pu, fams, label)
            within('dgamma chained', dg, starts[0].double() + gr.grad, at_kernel.dgamma_b + pg, None, label)
            within('dbeta', db, starts[1].double() + br.grad, at_kernel.dbeta_b, None, label)
