"""dclip_gemm_nt, dclip_gemm_tn_acc and dclip_colsum_acc element by element against float64 (tests/test_gemm_gpu.py is broad in shapes
but asserts max-error-over-max-value with bounds of several bf16 roundings; this file resolves one rounding, one row, one operand).

Layer 1 -- exact integer probes, no tolerance.  Operands are small integers held in bf16, side operands integer-valued, alpha in
{1, 0.5, 2}: every partial sum of every output element is an integer (or half-integer) below 2^23 in magnitude, hence exact in f32 in
ANY summation order (MFMA block order, split order, f32 atomics).  That is a condition on the inputs and is asserted on the float64
reference (`_assert_exact_inputs`: sum_k |alpha a b| + |side operands| < 2^23 per element -- one bit below the 2^24 of the integers,
for the half-integers of alpha = 0.5 -- and the same summed over rows for column sums).  The kernel output must then be bit-equal to
the float64 result rounded ONCE to the output type (round to nearest even; the inputs contain exact ties, asserted).  Outputs live in
column slices of wider NaN-filled buffers with more rows than M: one bit comparison of the whole buffer checks that every owned
element was written and no other element was touched.

Layer 2 -- real-valued operands, per-element bounds in float64, every bound derived (U23 = 2^-23, U24 = 2^-24):
  bz      |z_got - z| <= K U23 mag + U23 (|z| + |bias| + |rowadd|), mag = |alpha| |A| |B|^T: K exact products summed in any order with
          every add rounded (or truncated) to f32, plus the epilogue's own multiply-add and add.  (One-hot A: the sum has one non-zero
          term, adding zeros is exact, the first term is dropped.)
  store   f32: no rounding of its own (a residual add / a product adds U24 |y|); bf16 / f16 of a value y known to within b:
          b + half_ulp(|y| + b), half an ulp of the binade the value lies in, 2^(floor(log2 x) - p) with p = 8 for bf16 (8 significant
          bits) and 11 for f16 (f16 subnormals: 2^-25) -- ONE rounding to nearest, no extra factor: a truncating store (error up to a
          whole ulp) fails.  Relative to the value that is between 2^-9 and 2^-8 for bf16: a flat 2^-9 |y| would reject correctly rounded
          values in the lower half of every binade (1.7224 -> 1.71875 is off by 2^-8.2 of itself), a flat 2^-8 |y| is up to twice as
          loose as this.
  gelu    1.13 bz + 2e-6: |gelu'| <= 1.13 (verified below) and the project's own 2e-6 for the branch-free erf of gelu and gelu' over
          |z| <= 9 (tests/test_gemm_gpu.py::test_gelu_epilogue_accuracy_over_range); |z| <= 9 is asserted on the reference.
  quickgelu  y = z s(t), t = 1.702 z, from the instruction sequence of quick_gelu_f (common.h): t rounded once, the multiply inside
          __expf, a 1-ulp v_exp_f32, the add 1 + e, a 1-ulp v_rcp_f32 give a relative error of s of at most
          rs = ((1 - s)(2 |t| + 2) + 3) U24, and |dy| <= |y| (rs + U24) + 1.1 bz (|quickgelu'| <= 1.1, verified below); twice the first
          term is allowed.  The 1-ulp figures of the two hardware approximations are taken from the ISA description and common.h's
          comment; they have NOT been measured by this project.
          Derivative d = fma(t s, 1 - s, s): e_d6 = 2 [s rs (1 + |t|) + 3 U24 |t| s (1 - s) + U24 |d|]  (ds = s rs enters through
          dd/ds = 1 + t (1 - 2 s), |.| <= 1 + |t|; t s carries two roundings and 1 - s one; the fma rounds once; the same factor two).
  codes   saved 8-bit derivative: with c = (g'(z) - DG_LO) / DG_STEP in float64, |q - c| <= 0.5 + (|g''|max bz + e_act) / DG_STEP
          + 255 * 2^-22 per element (the last term: dg_pack4's own fma and its two f32 constants, at code magnitude <= 255), |g''| <= 0.8
          (GELU) / 0.86 (QuickGELU), both verified below.  No cap on the share of neighbouring codes: the condition says where one is
          legitimate.
  mulaux  |got - ref d| <= store(|d| bz + |ref| e_d + U24 |ref d|), d in float64 from the same codes; e_d = U23 (|DG_LO| + q DG_STEP), the
          unpack fma and its two f32 constants; dgelu the same with e_d = 2e-6 (the project's figure, above).
  colsum  |cs_got - cs| <= M U23 sum_rows |v| + sum_rows b_v (the accumulator's initial value is one of the terms); the reference sums
          the UN-rounded float64 values.  At the matrix sizes used here that bound is wider than the difference between summing before
          and after the bf16 rounding of random values, so `_before_rounding_case` uses a column of equal values that all round the
          same way, where the two differ by 3e-3 M against a bound of 1.2e-7 M^2 (M = 1300: 3.9 against 0.2).
  wgrad   |dW_got - dW| <= M U23 (|A|^T |B|) + U23 |dW|; colsum_acc the same with sum |x|.

The tile height of dclip_gemm_nt is chosen by a cost model and latched once per process, so the epilogue matrix runs in child
processes (this file run as a script) under DCLIP_GEMM256=0 (128 x 128), DCLIP_GEMM320=0 (256 rows), =2 (320 rows), =6 (192 rows).
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda' if torch.cuda.is_available() else 'cpu'
U23, U24 = 2.0 ** -23, 2.0 ** -24
BF16, F32, F16, U8 = torch.bfloat16, torch.float32, torch.float16, torch.uint8
SIG_BITS = {BF16: 8, F16: 11}
PAD = 16                                            # columns left and right of every output slice (16 keeps u8 rows 16-byte aligned)
EXTRA_ROWS = 3                                      # rows below M in every output buffer
GELU_D1, GELU_D2, QGELU_D1, QGELU_D2 = 1.13, 0.8, 1.1, 0.86
ERF_FIGURE = 2e-6                                   # test_gelu_epilogue_accuracy_over_range
HEIGHTS = {'128': {'DCLIP_GEMM256': '0'}, '256': {'DCLIP_GEMM320': '0'}, '320': {'DCLIP_GEMM320': '2'}, '192': {'DCLIP_GEMM320': '6'}}


def _ops():
    from distillclip_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _int_view(t):
    return t.view({F32: torch.int32, BF16: torch.int16, F16: torch.int16, U8: torch.uint8}[t.dtype])


def _wide(rows, cols, dtype, pad=PAD):
    """a [rows, pad + cols + pad] buffer of all-ones bits (NaN in every float type, 0xFF in u8) and its middle column slice"""
    w = torch.full((rows, cols + 2 * pad), -1 if dtype != U8 else 255, dtype=_int_view(torch.empty(0, dtype=dtype)).dtype, device=DEV).view(dtype)
    return w, w[:, pad:pad + cols]


def _sliced(x, pad=8):
    """x as a column slice of a wider buffer (leading dimension > row length), surrounded by a value that would show in any sum"""
    w = torch.full((x.shape[0], x.shape[1] + 2 * pad), 7, dtype=x.dtype, device=x.device)
    w[:, pad:pad + x.shape[1]] = x
    return w[:, pad:pad + x.shape[1]]


def _bits_fail(wide_got, wide_want, rows, cols, what, pad=PAD):
    """None, or a description of where the buffers differ bit for bit (inside / outside the owned [rows, cols] block)"""
    bad = _int_view(wide_got) != _int_view(wide_want)
    if not bad.any():
        return None
    inside = bad[:rows, pad:pad + cols]
    n_in = int(inside.sum())
    msg = f'{what}: {n_in} owned elements differ, {int(bad.sum()) - n_in} foreign elements changed'
    if n_in:
        r, c = torch.nonzero(inside)[0].tolist()
        msg += f'; first owned at ({r}, {c}): got {wide_got[r, pad + c].item()!r} want {wide_want[r, pad + c].item()!r}'
    return msg


def _bound_fail(got, ref, bound, what):
    """None, or a description of the elements with |got - ref| > bound (float64, per element; a NaN fails)"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if not bad.any():
        return None
    i = torch.nonzero(bad)[0].tolist()
    worst = torch.nan_to_num(err / bound, nan=math.inf).max().item()
    return (f'{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; first at {i}: got {got[tuple(i)].item()!r} '
            f'ref {ref[tuple(i)].item()!r} bound {bound[tuple(i)].item():.3e}; worst err / bound {worst:.3f}')


def _ties(y, dtype):
    """number of elements of y (exact in f32) that lie exactly half way between two neighbouring values of dtype"""
    r = y.float().to(dtype).double()
    other = 2 * y - r
    return int(((y != r) & (other.float().to(dtype).double() == other)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# layer 1: integer operands
# ---------------------------------------------------------------------------------------------------------------------------------
class IntOperands:
    """A [M, K], B [N, K]: sparse entries in {-2..2} (about 16 non-zero products per output element whatever K), plus a fixed number of
    'hot' rows of A / every eighth row of B with dense entries in {-32..32} over the first 64 k (M > 4096: {-128..128} and {-4..4}, and
    smaller side operands, so that the column sums of 39 424 rows still fit): their intersections give values in the thousands (real
    bf16 and f16 roundings, exact ties) while the sums over rows stay below 2^23.  Rows 0 and M - 1 and the rows
    around every tile edge (128, 192, 256, 320) are hot.  Both are column slices of wider buffers (lda, ldb > K)."""

    def __init__(self, M, N, K, seed):
        g = _gen(seed)
        p = min(1.0, math.sqrt(16.0 / K))

        ha, hb, n_bias, n_ra, n_res = (128, 4, 16, 8, 40) if M > 4096 else (32, 32, 64, 32, 300)

        def mat(rows, hot, amp):
            x = torch.randint(-2, 3, (rows, K), generator=g, device=DEV).float() * (torch.rand((rows, K), generator=g, device=DEV) < p)
            h = torch.zeros(len(hot), K, device=DEV)
            h[:, :64] = torch.randint(-amp, amp + 1, (len(hot), 64), generator=g, device=DEV).float()
            x[torch.tensor(hot, device=DEV)] = h
            return x
        hot_a = sorted({r for r in (0, 1, 127, 128, 191, 192, 255, 256, 319, 320, M // 2, M - 2, M - 1) if 0 <= r < M})
        hot_b = sorted(set(range(3, N, 8)) | {0, N - 1})
        a, b = mat(M, hot_a, ha), mat(N, hot_b, hb)
        self.M, self.N, self.K = M, N, K
        self.a, self.b = _sliced(a.to(BF16)), _sliced(b.to(BF16), 24)
        self.acc = a.double() @ b.double().t()
        self.mag = a.double().abs() @ b.double().abs().t()
        gi = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float()
        self.bias = gi(-n_bias, n_bias, (N,))
        self.rowadd = {G: gi(-n_ra, n_ra, (G, N)) for G in (50, 77)}
        self.res = gi(-n_res, n_res, (M, N))
        self.cs0 = gi(-9, 9, (N,))
        self.rows = torch.arange(M, device=DEV)


def _assert_exact_inputs(lim, cs_lim=None):
    """the condition on the INPUTS that makes every f32 summation order exact (module docstring)"""
    assert lim.max().item() < 2 ** 23, ('inputs too large for an exact probe', lim.max().item())
    if cs_lim is not None:
        assert cs_lim.max().item() < 2 ** 23, ('column sums too large for an exact probe', cs_lim.max().item())


def exact_case(d, out_dtype, flags, alpha, G=50, inplace=False, act='none'):
    """One dclip_gemm_nt launch on integer operands; flags is a subset of {bias, rowadd, aux, res, colsum}.  -> list of failure strings.
    act none: C, aux_out and the column sums bit-equal to float64; act quickgelu / gelu: aux_out and ownership only (C must be written)."""
    ops, M, N = _ops(), d.M, d.N
    what = f'[{M},{N},{d.K}] {str(out_dtype)[6:]} act={act} alpha={alpha} {"+".join(sorted(flags)) or "plain"}{" in-place" if inplace else ""}'
    res_dtype = F16 if out_dtype == F16 else F32
    z = alpha * d.acc
    lim = abs(alpha) * d.mag
    if 'bias' in flags:
        z, lim = z + d.bias.double(), lim + d.bias.double().abs()
    if 'rowadd' in flags:
        ra = d.rowadd[G].double()[d.rows % G]
        z, lim = z + ra, lim + ra.abs()
    y = z
    if 'res' in flags:
        y, lim = z + d.res.double(), lim + d.res.double().abs()
    _assert_exact_inputs(lim, d.cs0.double().abs() + lim.sum(0) if 'colsum' in flags else None)
    if out_dtype == F16:
        assert y.abs().max().item() < 65504
    fails = []
    wide, out = _wide(M + EXTRA_ROWS, N, out_dtype)
    want = wide.clone()
    residual = None
    if 'res' in flags:
        if inplace:
            out[:M] = d.res.to(res_dtype)
            want = wide.clone()
            residual = out[:M]
        else:
            residual = _sliced(d.res.to(res_dtype))
    aux_w = aux = None
    if 'aux' in flags:
        aux_w, aux = _wide(M + EXTRA_ROWS, N, BF16)
        assert aux.stride(0) == out.stride(0)
    cs = d.cs0.clone() if 'colsum' in flags else None
    ops.gemm_nt(d.a, d.b, bias=d.bias if 'bias' in flags else None, act=act, aux_out=aux, residual=residual, out=out, alpha=alpha,
                row_group=G if 'rowadd' in flags else 0, rowadd=d.rowadd[G] if 'rowadd' in flags else None, colsum=cs)
    if act == 'none':
        if out_dtype != F32:
            assert _ties(y, out_dtype) >= 1, ('the inputs produce no exact tie', what)
        want[:M, PAD:PAD + N] = y.float().to(out_dtype)
        fails.append(_bits_fail(wide, want, M, N, what + ' C'))
        if cs is not None:
            cs_want = (d.cs0.double() + y.sum(0)).float()
            if not torch.equal(cs, cs_want):
                bad = torch.nonzero(cs != cs_want)
                fails.append(f'{what} colsum: {bad.numel()} of {N} columns differ; first {bad[0].item()}: got {cs[bad[0]].item()} want {cs_want[bad[0]].item()}')
    else:
        got = wide.clone()
        if torch.isnan(got[:M, PAD:PAD + N]).any():
            fails.append(what + ' C: owned elements not written')
        got[:M, PAD:PAD + N] = want[:M, PAD:PAD + N]
        fails.append(_bits_fail(got, want, M, N, what + ' C outside'))
    if aux is not None:
        aux_want = _wide(M + EXTRA_ROWS, N, BF16)[0]
        assert _ties(z, BF16) >= 1, ('the inputs produce no exact tie', what)
        aux_want[:M, PAD:PAD + N] = z.float().to(BF16)
        fails.append(_bits_fail(aux_w, aux_want, M, N, what + ' aux_out'))
    return [f for f in fails if f]


SIDE_FLAGS = ('bias', 'rowadd', 'aux', 'res', 'colsum')


def exact_matrix(shapes, seed=100):
    """ACT none x OUT {bf16, f32, f16} x every subset of {bias, rowadd + row_group, aux_out, residual, colsum} (f32 / f16 with a residual
    both out of place and in place), alpha cycling through {1, 0.5, 2}, row_group 50 / 77 (neither divides a tile height); and the saved
    pre-activation of ACT quickgelu / gelu.  -> (number of launches, failures)"""
    fails, n = [], 0
    for si, (M, N, K) in enumerate(shapes):
        d = IntOperands(M, N, K, seed + si)
        for oi, od in enumerate((BF16, F32, F16)):
            for fi in range(32):
                flags = {f for b, f in enumerate(SIDE_FLAGS) if fi >> b & 1}
                for inplace in ((False, True) if 'res' in flags and od != BF16 else (False,)):
                    n += 1
                    fails += exact_case(d, od, flags, (1.0, 0.5, 2.0)[(fi + oi + si + inplace) % 3], (50, 77)[(fi + si) % 2], inplace)
        for ai, act in enumerate(('quickgelu', 'gelu')):
            for oi, od in enumerate((BF16, F32)):
                for flags in ({'aux'}, {'aux', 'bias', 'rowadd'}, {'aux', 'bias', 'res', 'colsum'}):
                    n += 1
                    fails += exact_case(d, od, flags, (1.0, 0.5, 2.0)[(ai + oi + si) % 3], 77, False, act)
        del d
    return n, fails


def exact_tn_case(M, P, Q, splits, seed, workspace=True, calls=2):
    """dW (a column slice of a NaN-filled buffer, integer start values) += A^T B, `calls` times, bit-equal to float64"""
    ops = _ops()
    g = _gen(seed)
    p = min(1.0, math.sqrt(16.0 / M))
    mk = lambda cols: torch.randint(-2, 3, (M, cols), generator=g, device=DEV).float() * (torch.rand((M, cols), generator=g, device=DEV) < p)
    a, b = mk(P), mk(Q)
    a[M - 1], b[M - 1] = 1, 2                                   # the last row of the contraction reaches every output element
    dw0 = torch.randint(-8, 9, (P, Q), generator=g, device=DEV).float()
    ref = a.double().t() @ b.double()
    _assert_exact_inputs(dw0.double().abs() + calls * (a.double().abs().t() @ b.double().abs()))
    wide, dw = _wide(P, Q, F32)
    dw[:] = dw0
    want = wide.clone()
    a_s, b_s = _sliced(a.to(BF16)), _sliced(b.to(BF16), 24)
    fails = []
    for c in range(1, calls + 1):
        ops.gemm_tn_acc(a_s, b_s, dw, splits, workspace=workspace)
        want[:, PAD:PAD + Q] = (dw0.double() + c * ref).float()
        fails.append(_bits_fail(wide, want, P, Q, f'gemm_tn_acc [{M},{P},{Q}] splits={splits} workspace={workspace} call {c}'))
    return [f for f in fails if f]


def exact_colsum_case(M, N, full, off, seed):
    """dclip_colsum_acc on integers in {-3..3}, the last row all non-zero, db a slice of a NaN-filled vector with integer start values"""
    ops = _ops()
    g = _gen(seed)
    xw = torch.randint(-3, 4, (M, full), generator=g, device=DEV).float()
    xw[M - 1] = 3
    x = xw.to(BF16)[:, off:off + N]
    db0 = torch.randint(-9, 10, (N,), generator=g, device=DEV).float()
    _assert_exact_inputs(db0.double().abs() + x.double().abs().sum(0))
    wide, db = _wide(1, N, F32)
    db[0] = db0
    want = wide.clone()
    ops.colsum_acc(x, db[0])
    want[0, PAD:PAD + N] = (db0.double() + x.double().sum(0)).float()
    f = _bits_fail(wide, want, 1, N, f'colsum_acc [{M},{N}] of [{M},{full}] at column {off}')
    return [f] if f else []


# ---------------------------------------------------------------------------------------------------------------------------------
# layer 2: real operands, per-element bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _phi(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def _cdf(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2)))


def gelu64(z):
    return z * _cdf(z)


def dgelu64(z):
    return _cdf(z) + z * _phi(z)


def d2gelu64(z):
    return _phi(z) * (2 - z * z)


def qgelu64(z):
    return z * torch.sigmoid(1.702 * z)


def dqgelu64(z):
    s = torch.sigmoid(1.702 * z)
    return s + 1.702 * z * s * (1 - s)


def d2qgelu64(z):
    s, t = torch.sigmoid(1.702 * z), 1.702 * z
    return 1.702 * s * (1 - s) * (2 + t * (1 - 2 * s))


def _dg64(q):
    ops = _ops()
    return ops.DG_LO + q.double() * ops.DG_STEP


def _qgelu_rs(z):
    """relative error bound of the kernel's sigmoid(1.702 z) (module docstring)"""
    t = (1.702 * z).abs()
    return ((1 - torch.sigmoid(1.702 * z)) * (2 * t + 2) + 3) * U24


def act_bounds(act, z, bz):
    """-> (y, b_y, code reference c or None, code bound or None): the activated value in float64, its bound, and for the saving
    variants the real-valued 8-bit code with its bound (module docstring: gelu, quickgelu, codes)"""
    ops = _ops()
    if act in ('gelu', 'gelu_save'):
        assert z.abs().max().item() <= 9.0, ('|z| <= 9 is the range of the erf figure', z.abs().max().item())
        y, by = gelu64(z), GELU_D1 * bz + ERF_FIGURE
        d, bd = dgelu64(z), GELU_D2 * bz + ERF_FIGURE
    elif act in ('quickgelu', 'quickgelu_save'):
        assert z.abs().max().item() <= 9.0, ('|z| <= 9 is the range the bound is derived for', z.abs().max().item())
        y = qgelu64(z)
        rs = _qgelu_rs(z)
        by = 2 * y.abs() * (rs + U24) + QGELU_D1 * bz
        s, t = torch.sigmoid(1.702 * z), (1.702 * z).abs()
        d = dqgelu64(z)
        bd = QGELU_D2 * bz + 2 * (s * rs * (1 + t) + 3 * U24 * t * s * (1 - s) + U24 * d.abs())
    else:
        return z, bz, None, None
    if not act.endswith('_save'):
        return y, by, None, None
    return y, by, (d - ops.DG_LO) / ops.DG_STEP, 0.5 + bd / ops.DG_STEP + 255 * 2.0 ** -22


def half_ulp(x, dtype):
    """half the spacing of dtype's values in the binade of x >= 0 (0 at x = 0; f16: the subnormal spacing below 2^-14)"""
    e = torch.floor(torch.log2(x))
    if dtype == F16:
        e = e.clamp(min=-14)
    return torch.exp2(e - SIG_BITS[dtype])


def store_bound(y, b, dtype):
    return b if dtype == F32 else b + half_ulp(y.abs() + b, dtype)


class RealOperands:
    """bf16 operands for the bound checks; the scale of B is chosen so that z = alpha A B^T stays within a few units whatever alpha.
    fill: 'random' N(0, 1) ; 'positive' (all terms of one sign: sum |terms| = |ref|, the bound is tight in relative terms) ;
    'cancel' (columns in pairs, A equal and B of opposite sign within a pair, except the last pair: ref is near 0, the terms are not)."""

    def __init__(self, M, N, K, alpha, fill, seed):
        g = _gen(seed)
        rn = lambda *s: torch.randn(s, generator=g, device=DEV)
        if fill == 'random':
            a, b = rn(M, K), rn(N, K) * (1.2 / (math.sqrt(K) * alpha))
        elif fill == 'positive':
            a, b = rn(M, K).abs(), rn(N, K).abs() * (3.0 / (0.6366 * K * alpha))
        else:
            a, b = rn(M, K), rn(N, K) * (4.0 / alpha)
            a[:, 1::2] = a[:, 0::2]
            b[:, 1::2] = -b[:, 0::2]
            a[:, K - 2:] = a[:, K - 2:].clamp(-3, 3)             # (a product of two normals has heavy tails: keep |z| <= 9)
            b[:, K - 2:] = rn(N, 2).clamp(-2, 2) * (0.4 / alpha)
        a, b = a.to(BF16), b.to(BF16)
        self.M, self.N, self.K, self.alpha, self.fill, self.kterms = M, N, K, alpha, fill, K
        self.a, self.b = _sliced(a), _sliced(b, 24)
        self.acc = alpha * (a.double() @ b.double().t())
        self.mag = abs(alpha) * (a.double().abs() @ b.double().abs().t())
        self.bias = rn(N) * 0.3
        self.rowadd = rn(77, N) * 0.3
        self.res = rn(M, N)
        self.aux_z = (rn(M, N) * 2).clamp(-9, 9).to(BF16)
        self.aux_q = torch.randint(0, 256, (M, N), generator=g, device=DEV, dtype=torch.int32).to(U8)
        self.cs0 = rn(N)
        self.rows = torch.arange(M, device=DEV)


def bound_case(d, act, out_dtype, flags, G=77, inplace=False):
    """One dclip_gemm_nt launch on real operands against the per-element float64 bounds; flags as in exact_case.  -> failure strings"""
    ops, M, N = _ops(), d.M, d.N
    what = (f'[{M},{N},{d.K}] {d.fill} alpha={d.alpha:.4f} {str(out_dtype)[6:]} act={act} '
            f'{"+".join(sorted(flags)) or "plain"}{" in-place" if inplace else ""}')
    res_dtype = F16 if out_dtype == F16 else F32
    z, side = d.acc, 0.0
    if 'bias' in flags:
        z, side = z + d.bias.double(), side + d.bias.double().abs()
    if 'rowadd' in flags:
        ra = d.rowadd.double()[d.rows % G]
        z, side = z + ra, side + ra.abs()
    bz = (d.kterms * U23 * d.mag if d.kterms > 1 else 0.0) + U23 * (z.abs() + side)
    fails = []
    code_ref = code_b = None
    if act == 'dgelu':
        dd = dgelu64(d.aux_z.double())
        y = z * dd
        by = dd.abs() * bz + z.abs() * ERF_FIGURE + U24 * y.abs()
    elif act == 'mulaux':
        dd = _dg64(d.aux_q)
        y = z * dd
        by = dd.abs() * bz + z.abs() * U23 * (abs(ops.DG_LO) + d.aux_q.double() * ops.DG_STEP) + U24 * y.abs()
    else:
        y, by, code_ref, code_b = act_bounds(act, z, bz)
    res = None
    if 'res' in flags:
        res = d.res.to(res_dtype)
        y = y + res.double()
        by = by + U24 * y.abs()
    wide, out = _wide(M + EXTRA_ROWS, N, out_dtype)
    residual = None
    if res is not None:
        if inplace:
            out[:M] = res
            residual = out[:M]
        else:
            residual = _sliced(res)
    untouched = wide.clone()
    aux_w = aux = None
    if 'aux' in flags:
        aux_w, aux = _wide(M + EXTRA_ROWS, N, U8 if act.endswith('_save') else BF16)
        assert aux.stride(0) == out.stride(0)
    aux_in = None
    if act in ('dgelu', 'mulaux'):                   # aux_in shares C's leading dimension (include/dclip.h)
        aux_in = _wide(M, N, BF16 if act == 'dgelu' else U8)[1]
        aux_in[:] = d.aux_z if act == 'dgelu' else d.aux_q
        assert aux_in.stride(0) == out.stride(0)
    cs = d.cs0.clone() if 'colsum' in flags else None
    kw = dict(bias=d.bias if 'bias' in flags else None, act=act, aux_in=aux_in, residual=residual, alpha=d.alpha,
              row_group=G if 'rowadd' in flags else 0, rowadd=d.rowadd if 'rowadd' in flags else None)
    ops.gemm_nt(d.a, d.b, aux_out=aux, out=out, colsum=cs, **kw)
    got = out[:M]
    fails.append(_bound_fail(got, y, store_bound(y, by, out_dtype), what + ' C'))
    chk = wide.clone()
    chk[:M, PAD:PAD + N] = untouched[:M, PAD:PAD + N]
    fails.append(_bits_fail(chk, untouched, M, N, what + ' C outside'))
    if cs is not None:
        cs_ref = d.cs0.double() + y.sum(0)
        cs_b = M * U23 * (d.cs0.double().abs() + y.abs().sum(0)) + by.sum(0)
        fails.append(_bound_fail(cs, cs_ref, cs_b, what + ' colsum'))
    if aux is not None:
        blank = _wide(M + EXTRA_ROWS, N, aux.dtype)[0]
        if aux.dtype == BF16:
            fails.append(_bound_fail(aux[:M], z, store_bound(z, bz, BF16), what + ' aux_out'))
        else:
            fails.append(_bound_fail(aux[:M], code_ref, code_b, what + ' saved derivative code'))
        chk = aux_w.clone()
        chk[:M, PAD:PAD + N] = blank[:M, PAD:PAD + N]
        fails.append(_bits_fail(chk, blank, M, N, what + ' aux_out outside'))
    if act.endswith('_save') and not inplace:
        # the activated output of a saving variant is bit-equal to the plain activation's on the same operands
        plain = ops.gemm_nt(d.a, d.b, out_dtype=out_dtype, **dict(kw, act=act[:-5]))
        if not torch.equal(_int_view(plain), _int_view(got.contiguous())):
            fails.append(what + f' C differs from act={act[:-5]} in {int((_int_view(plain) != _int_view(got.contiguous())).sum())} elements')
    if not inplace and 'colsum' not in flags:
        # plain stores, no atomics: a repeat is bit-identical
        wide2, out2 = _wide(M + EXTRA_ROWS, N, out_dtype)
        ops.gemm_nt(d.a, d.b, out=out2, **kw)
        if not torch.equal(_int_view(out2[:M].contiguous()), _int_view(got.contiguous())):
            fails.append(what + ' C: a repeated launch differs')
    return [f for f in fails if f]


# per activation: the operand set that takes the compile-time lean epilogue of the 192- / 256- / 320-row kernels, and one that does not
ACT_VARIANTS = {
    'none': [(BF16, {'bias'}), (BF16, {'bias', 'colsum'}), (BF16, {'bias', 'rowadd', 'aux', 'res', 'colsum'}),
             (F32, {'bias', 'res'}), (F32, {'bias', 'rowadd'}), (F32, {'bias', 'res', 'colsum'}),
             (F16, {'bias', 'res'}), (F16, {'rowadd'}), (F16, {'bias', 'res', 'colsum'})],
    'quickgelu': [(BF16, {'bias'}), (BF16, {'bias', 'aux', 'colsum'}), (F32, {'bias', 'aux', 'res'})],
    'gelu': [(BF16, {'bias'}), (BF16, {'bias', 'aux', 'colsum'}), (F32, {'bias', 'aux', 'res'})],
    'dgelu': [(BF16, {'colsum'}), (BF16, set()), (F32, {'res', 'colsum'})],
    'mulaux': [(BF16, {'colsum'}), (BF16, {'bias', 'res'}), (F32, {'colsum'})],
    'gelu_save': [(BF16, {'bias', 'aux'}), (BF16, {'bias', 'aux', 'colsum'}), (BF16, {'bias'}), (BF16, {'bias', 'aux', 'rowadd', 'res'}),
                  (F32, {'bias', 'aux'})],
    'quickgelu_save': [(BF16, {'bias', 'aux'}), (BF16, {'bias', 'aux', 'colsum'}), (BF16, {'bias'}), (BF16, {'bias', 'aux', 'rowadd', 'res'}),
                       (F32, {'bias', 'aux'})],
}
ALPHAS = (1.0, 0.125, 80 ** -0.5)                  # 1, a power of two, and a head dimension's hd^-0.5 that is not one


def bound_matrix(shapes, seed=300):
    """every activation code with every output type it accepts, each fill, alpha in ALPHAS.  -> (launch groups, failures)"""
    fails, n = [], 0
    for si, (M, N, K) in enumerate(shapes):
        for ai, alpha in enumerate(ALPHAS):
            for fi, fill in enumerate(('random', 'positive', 'cancel')):
                d = RealOperands(M, N, K, alpha, fill, seed + 9 * si + 3 * ai + fi)
                for act, variants in ACT_VARIANTS.items():
                    for od, flags in variants:
                        n += 1
                        fails += bound_case(d, act, od, flags, inplace=('res' in flags and od != BF16 and (n & 1) == 1))
                del d
    return n, fails


def sweep_case(n, act, out_dtype=F32):
    """identity A, so z runs over a chosen grid: every bf16 value met by 'n * n points of [-9, 9]', as test_gelu_epilogue_accuracy_over_range
    does for the erf.  quickgelu, quickgelu_save (value, code, and the MULAUX product with ones after it) and gelu_save."""
    ops = _ops()
    d = RealOperands.__new__(RealOperands)
    a = torch.eye(n, dtype=BF16, device=DEV)
    x = torch.linspace(-9, 9, n * n, device=DEV).reshape(n, n).to(BF16)
    d.M = d.N = d.K = n
    d.alpha, d.fill, d.kterms = 1.0, 'grid', 1
    d.a, d.b = _sliced(a), _sliced(x, 24)
    d.acc, d.mag = x.double().t().contiguous(), x.double().abs().t().contiguous()
    d.bias, d.rowadd, d.res, d.cs0, d.rows = None, None, None, None, None
    flags = {'aux'} if act.endswith('_save') else set()
    fails = bound_case(d, act, out_dtype, flags)
    if act.endswith('_save'):
        # the backward half of the pair: ones x I, times the codes just written = the decoded derivative itself
        _, out = _wide(n + EXTRA_ROWS, n, U8)
        ops.gemm_nt(d.a, d.b, act=act, aux_out=out, out=_wide(n + EXTRA_ROWS, n, out_dtype)[1])
        d.aux_q = out[:n].contiguous()
        d.b = _sliced(torch.ones(n, n, dtype=BF16, device=DEV), 24)
        d.acc, d.mag = torch.ones(n, n, dtype=torch.float64, device=DEV), torch.ones(n, n, dtype=torch.float64, device=DEV)
        d.fill = 'grid, codes of ' + act
        fails += bound_case(d, 'mulaux', out_dtype, set())
    return fails


def _before_rounding_case(M=1300, N=264, K=64):
    """column sums are taken BEFORE the bf16 rounding of the stored copy: one-hot A rows and B = 1 give z = 1 + bias with bias = 0.003,
    below half a bf16 ulp of 1 (2^-8): every stored value rounds down to 1.0.  The sums of the un-rounded values are 1.003 M, of the
    stored ones 1.0 M: 3.9 apart at M = 1300, against a bound of about 0.2 (module docstring: colsum)."""
    d = RealOperands.__new__(RealOperands)
    a = torch.zeros(M, K, device=DEV)
    a[torch.arange(M), torch.arange(M) % K] = 1
    b = torch.ones(N, K, device=DEV)
    d.M, d.N, d.K, d.alpha, d.fill, d.kterms = M, N, K, 1.0, 'one-hot ones', 1
    d.a, d.b = _sliced(a.to(BF16)), _sliced(b.to(BF16), 24)
    d.acc = torch.ones(M, N, dtype=torch.float64, device=DEV)
    d.mag = d.acc.clone()
    d.bias = torch.full((N,), 0.003, device=DEV)
    d.cs0 = torch.zeros(N, device=DEV)
    d.rowadd = d.res = d.rows = None
    cs_b = M * U23 * 1.003 * M
    assert 0.003 * M > 4 * cs_b, 'the case no longer separates the two sums'
    return bound_case(d, 'none', BF16, {'bias', 'colsum'})


def bound_tn_case(M, P, Q, splits, seed, workspace=True):
    ops = _ops()
    g = _gen(seed)
    a = torch.randn((M, P), generator=g, device=DEV).to(BF16)
    b = torch.randn((M, Q), generator=g, device=DEV).to(BF16)
    dw0 = torch.randn((P, Q), generator=g, device=DEV)
    wide, dw = _wide(P, Q, F32)
    dw[:] = dw0
    blank = _wide(P, Q, F32)[0]
    ops.gemm_tn_acc(_sliced(a), _sliced(b, 24), dw, splits, workspace=workspace)
    ref = dw0.double() + a.double().t() @ b.double()
    bound = M * U23 * (a.double().abs().t() @ b.double().abs()) + U23 * ref.abs() + U23 * dw0.double().abs()
    what = f'gemm_tn_acc [{M},{P},{Q}] splits={splits} workspace={workspace}'
    fails = [_bound_fail(dw, ref, bound, what)]
    chk = wide.clone()
    chk[:, PAD:PAD + Q] = blank[:, PAD:PAD + Q]
    fails.append(_bits_fail(chk, blank, P, Q, what + ' outside'))
    return [f for f in fails if f]


# ---------------------------------------------------------------------------------------------------------------------------------
# the forced-height children
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD_EXACT_SHAPES = [(1025, 264, 64), (1300, 520, 192), (1279, 256, 768), (1024, 264, 128)]
CHILD_BOUND_SHAPES = [(1300, 520, 192)]
CHILD_SWEEP_N = 1280


def child_main():
    sys.path.insert(0, ROOT)
    n1, f1 = exact_matrix(CHILD_EXACT_SHAPES)
    n2, f2 = bound_matrix(CHILD_BOUND_SHAPES)
    for act in ('quickgelu', 'quickgelu_save', 'gelu_save'):
        for od in (BF16, F32):
            n2 += 1
            f2 += sweep_case(CHILD_SWEEP_N, act, od)
    n2 += 1
    f2 += _before_rounding_case()
    torch.cuda.synchronize()
    print('RESULT ' + json.dumps({'n1': n1, 'layer1': f1, 'n2': n2, 'layer2': f2}))


_CHILD = {}


def _child(height):
    """run (once per height) this file as a script in a fresh process with the tile-height knob set; no further child is started after one
    that died (non-zero exit or timeout)"""
    if height in _CHILD:
        return _CHILD[height]
    assert not _CHILD.get('dead'), 'not started: an earlier child process died (' + str(_CHILD.get('dead')) + ')'
    env = {k: v for k, v in os.environ.items() if k not in ('DCLIP_GEMM256', 'DCLIP_GEMM320')}
    env.update(HEIGHTS[height])
    torch.cuda.synchronize()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired:
        _CHILD['dead'] = height + ': timeout'
        raise
    lines = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    if r.returncode != 0 or not lines:
        _CHILD['dead'] = f'{height}: exit {r.returncode}'
        raise AssertionError(f'child for tile height {height} exit {r.returncode}\n' + r.stdout[-2000:] + r.stderr[-3000:])
    _CHILD[height] = json.loads(lines[-1][7:])
    return _CHILD[height]


def _report(fails, n):
    assert not fails, f'{len(fails)} failures in {n} launches:\n' + '\n'.join(fails[:40])


@pytest.mark.parametrize('height', list(HEIGHTS))
def test_exact_epilogue_matrix_forced_tile_height(height):
    """layer 1 on the 128 x 128 kernel and on the 256-, 320- and 192-row kernels: exact_matrix over CHILD_EXACT_SHAPES (M, N just above and
    just below the tile edges, K = 64 .. 768), which reaches MODE 0 / 1 / 2 / 3 and the full / ragged unit test of each height"""
    r = _child(height)
    assert r['n1'] == 140 * len(CHILD_EXACT_SHAPES)         # 96 subsets x types, 32 of them also in place, 12 activated
    _report(r['layer1'], r['n1'])


@pytest.mark.parametrize('height', list(HEIGHTS))
def test_bounds_every_activation_forced_tile_height(height):
    """layer 2 on every tile height: bound_matrix (activation codes 0..6 x the output types each accepts x three fills x ALPHAS), the
    activation sweeps over [-9, 9] and the before-rounding column-sum case"""
    r = _child(height)
    assert r['n2'] >= 9 * sum(len(v) for v in ACT_VARIANTS.values())
    _report(r['layer2'], r['n2'])


# ---------------------------------------------------------------------------------------------------------------------------------
# in process: the default route on the step's shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K', [(12800, 768, 768), (25600, 2304, 128), (39424, 3072, 64), (25600, 512, 3072), (12800, 3072, 128)])
def test_exact_step_shapes_default_route(M, N, K):
    """layer 1 where the cost model sends the step's own shapes: the operand sets the towers launch, plus the general epilogue"""
    d = IntOperands(M, N, K, 7)
    fails = []
    cases = [(BF16, {'bias'}, 2.0), (BF16, {'bias', 'colsum'}, 0.5), (BF16, {'bias', 'rowadd', 'aux', 'res', 'colsum'}, 1.0),
             (F32, {'bias', 'res'}, 1.0), (F16, {'bias', 'res'}, 2.0), (F32, {'rowadd', 'colsum'}, 0.5)]
    for od, flags, alpha in cases:
        fails += exact_case(d, od, flags, alpha, 50, inplace=od != BF16 and 'res' in flags)
    fails += exact_case(d, BF16, {'aux', 'bias'}, 1.0, 50, False, 'gelu')
    _report(fails, len(cases) + 1)


@pytest.mark.parametrize('M,N,K,fill', [(12800, 768, 768, 'random'), (25600, 768, 128, 'positive'), (39424, 512, 64, 'cancel')])
def test_bounds_step_shapes_default_route(M, N, K, fill):
    d = RealOperands(M, N, K, 0.125, fill, 11)
    fails = []
    for act, (od, flags) in (('none', (BF16, {'bias', 'colsum'})), ('none', (F32, {'bias', 'res'})), ('quickgelu_save', (BF16, {'bias', 'aux'})),
                             ('gelu_save', (BF16, {'bias', 'aux'})), ('mulaux', (BF16, {'colsum'})), ('dgelu', (BF16, {'colsum'}))):
        fails += bound_case(d, act, od, flags)
    _report(fails, 6)


@pytest.mark.parametrize('n', [256, 1024])
@pytest.mark.parametrize('act', ['quickgelu', 'quickgelu_save', 'gelu_save'])
def test_activation_sweep_over_range(n, act):
    """n = 256 runs on the 128 x 128 kernel, n = 1024 on the default large-tile route"""
    fails = sweep_case(n, act, F32) + sweep_case(n, act, BF16)
    _report(fails, 2)


def test_colsum_is_summed_before_the_output_rounding():
    _report(_before_rounding_case(), 1)


def test_derivative_maxima():
    """the constants the bounds use: max |gelu'| <= 1.13, |gelu''| <= 0.8, |quickgelu'| <= 1.1, |quickgelu''| <= 0.86 (float64, a grid of
    4e6 points over [-12, 12]; outside it all four are below 1e-6 away from their limits 0 or 1)"""
    z = torch.linspace(-12, 12, 4_000_001, dtype=torch.float64, device=DEV)
    for f, lim in ((dgelu64, GELU_D1), (d2gelu64, GELU_D2), (dqgelu64, QGELU_D1), (d2qgelu64, QGELU_D2)):
        m = f(z).abs().max().item()
        assert m <= lim and m > 0.9 * lim, (f.__name__, m, lim)
    # the closed forms are the derivatives of the functions (central differences)
    z = torch.linspace(-9, 9, 20001, dtype=torch.float64, device=DEV)
    h = 1e-5
    for f, df in ((gelu64, dgelu64), (dgelu64, d2gelu64), (qgelu64, dqgelu64), (dqgelu64, d2qgelu64)):
        assert ((f(z + h) - f(z - h)) / (2 * h) - df(z)).abs().max().item() < 1e-8


# wgrad routes: gemm_tn_kernel (M % 64 != 0; P, Q = 8 mod 16; more splits than 64-row chunks), gemm_tn_glds_kernel (M % 64 == 0), both
# with ragged P, Q; the 256^2 pipeline is below
TN_CASES = [(200, 72, 200, 7), (37, 8, 24, 1), (1000, 136, 264, 4), (51, 384, 128, 3),
            (640, 72, 200, 3), (128, 8, 8, 2), (1024, 264, 136, 4), (4096, 128, 3072, 7)]


@pytest.mark.parametrize('M,P,Q,splits', TN_CASES)
def test_gemm_tn_acc_exact(M, P, Q, splits):
    """P, Q = 8 mod 16 are accepted by the entry (P % 8, Q % 8) and are exact on both small-tile kernels: include/dclip.h says % 8"""
    _report(exact_tn_case(M, P, Q, splits, 21), 2)


@pytest.mark.parametrize('M,P,Q,splits', TN_CASES[:2] + TN_CASES[4:6] + [(4096, 1024, 1024, 4)])
def test_gemm_tn_acc_bounds(M, P, Q, splits):
    _report(bound_tn_case(M, P, Q, splits, 23), 1)


@pytest.mark.parametrize('M,P,Q', [(4096, 1024, 1024), (6400, 768, 3072)])
def test_gemm_tn_256_pipeline_exact(M, P, Q):
    """the 256 x 256 wgrad pipeline: partial tiles + fixed-order sum (two accumulating calls, and bit-identical repeats), the f32-atomic
    epilogue without a workspace, and a workspace that is too small -- the fallback counter rises by exactly one each time"""
    ops = _ops()
    from distillclip_amd._lib import lib
    c0 = lib().dclip_gemm_tn_atomic_fallbacks()
    fails = exact_tn_case(M, P, Q, 4, 25)
    assert lib().dclip_gemm_tn_atomic_fallbacks() == c0, 'the partial-tile path fell back to atomics'
    fails += exact_tn_case(M, P, Q, 4, 26, workspace=False, calls=1)
    assert lib().dclip_gemm_tn_atomic_fallbacks() == c0 + 1
    # too small a workspace, through the C entry
    g = _gen(27)
    a = (torch.randint(-2, 3, (M, P), generator=g, device=DEV).float() * (torch.rand((M, P), generator=g, device=DEV) < 0.06)).to(BF16)
    b = (torch.randint(-2, 3, (M, Q), generator=g, device=DEV).float() * (torch.rand((M, Q), generator=g, device=DEV) < 0.06)).to(BF16)
    a[M - 1], b[M - 1] = 1, 2
    mag = a.double().abs().t() @ b.double().abs()
    _assert_exact_inputs(5 + mag)
    wide, dw = _wide(P, Q, F32)
    dw[:] = 5
    want = wide.clone()
    want[:, PAD:PAD + Q] = (5 + a.double().t() @ b.double()).float()
    ws = torch.empty(1 << 20, dtype=U8, device=DEV)
    lib().dclip_gemm_tn_acc(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), dw.data_ptr(), dw.stride(0), M, P, Q, 4, ws.data_ptr(),
                            ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert lib().dclip_gemm_tn_atomic_fallbacks() == c0 + 2
    f = _bits_fail(wide, want, P, Q, f'gemm_tn_acc [{M},{P},{Q}] with a 1 MiB workspace')
    fails += [f] if f else []
    # no atomics on the partial-tile path: a repeat on real operands is bit-identical
    ar, br = torch.randn((M, P), generator=g, device=DEV).to(BF16), torch.randn((M, Q), generator=g, device=DEV).to(BF16)
    d1, d2 = torch.zeros(P, Q, device=DEV), torch.zeros(P, Q, device=DEV)
    ops.gemm_tn_acc(ar, br, d1, 4)
    ops.gemm_tn_acc(ar, br, d2, 4)
    assert torch.equal(d1, d2)
    _report(fails, 4)


@pytest.mark.parametrize('M,N,full,off', [(1037, 304, 320, 8), (4099, 768, 2304, 1536), (25600, 2304, 2304, 0),      # colsum8_kernel
                                          (1037, 300, 300, 0), (1037, 304, 320, 4), (513, 8, 24, 3)])                # colsum_kernel
def test_colsum_acc_exact(M, N, full, off):
    _report(exact_colsum_case(M, N, full, off, 31), 1)


@pytest.mark.parametrize('M,N,full,off', [(4099, 768, 2304, 1536), (1037, 300, 300, 0)])
def test_colsum_acc_bounds(M, N, full, off):
    ops = _ops()
    g = _gen(33)
    x = torch.randn((M, full), generator=g, device=DEV).to(BF16)[:, off:off + N]
    db0 = torch.randn((N,), generator=g, device=DEV)
    db = db0.clone()
    ops.colsum_acc(x, db)
    ref = db0.double() + x.double().sum(0)
    bound = M * U23 * (db0.double().abs() + x.double().abs().sum(0)) + U23 * ref.abs()
    f = _bound_fail(db, ref, bound, f'colsum_acc [{M},{N}]')
    _report([f] if f else [], 1)


if __name__ == '__main__':
    assert sys.argv[1:] == ['child']
    child_main()
