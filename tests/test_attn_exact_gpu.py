"""dclip_attn_nt / _nn / _tn and dclip_attn_fused_fwd element by element against float64 (tests/test_kernels_gpu.py compares them with
torch fp32 as max-error-over-max-value of the whole tensor; this file resolves one element, one rounding, one key).  U23 = 2^-23,
U24 = 2^-24.  The input builders and the conditions they assert are properties of the float64 reference alone: they draw with a CPU
generator (the same numbers with and without a GPU) and tests/test_attn_exact_cpu.py runs every one of them without the library.

Layer 1 -- exact probes, no tolerance.
  products   Operands are integers in [-31, 31] held in bf16, alpha in {1, 0.5, 2, -1}: for every output element sum |alpha a b| < 2^23
             (asserted on the reference), so every partial sum is an integer or half-integer that f32 holds exactly in ANY order, and the
             output must be bit-equal to the float64 result rounded ONCE to the output type (f32: no rounding; bf16: nearest even).
             Every case of 256 or more output elements contains real bf16 roundings and exact ties (asserted, redrawn until it does;
             smaller cases -- N = 1 has one element per problem -- cannot, and each sweep asserts both counts over all its cases).
             Every (b, h) problem draws its own integers.  Token-major operands are column slices of wider buffers, a separate one or
             the packed [B*N, 3D] layout of the towers, the rest filled with 192 (larger than any operand: it shows in any sum); A of
             nn / tn keeps its pad columns [N, Np) zero.  Outputs are slices of all-ones-bits (NaN) buffers -- nn / tn: a column slice
             with extra rows; nt: the [B,H,N,Np] block with guard elements on both sides -- and ONE bit comparison of the whole buffer
             checks every owned element, the +0 pad columns of nt, and that nothing else was touched.  Quad-blocked A comes from
             `block_scores`, written from the index formula of include/dclip.h and checked against ops.unblock_scores; both layouts
             are compared with float64, not with each other.
  selection  (fused) q_i = 32 w_t(i), k_j = 32 w_j with distinct +-1 words w: the scaled score of key t(i) is at least
             2 * 1024 * hd^-0.5 >= 256 above every other allowed key (asserted for EVERY row: gap >= 200).  exp2 of anything below -288
             is 0 in f32, denormals included, so e = 0 at every other key.  At t(i) the kernel evaluates exp2(fma(m, c2, -(m c2)))
             with m c2 rounded once: the argument is that rounding's error, at most half an ulp of m c2 < 2^14 (asserted), 2^-11, so
             e = 1 +- 2^-11, its bf16 copy is exactly 1, the row sum is e and ctx = v[t] / e lies within 2^-10 |v| of the bf16 value
             v[t]: less than half a bf16 ulp (>= 2^-9 |v|), so ctx[i] must equal v[t(i)] BIT FOR BIT.  Without the mask t is a
             permutation with a stride per problem (every key of every tile is hit in every problem, never the diagonal for N > 1).
             Under the causal mask t(i) <= i, and the only such map onto all keys is the identity: problem 0 of every causal case
             takes it, the others take t(i) = i - o(i), o in {0, 5, .., 35}.  In the causal cases feature 0 is 512 for the queries
             i < N / 2 and 256 for the keys j >= N / 2 (masked for those queries) and 0 elsewhere: allowed scores do not change, and
             N // 2 >= N / 3 rows have their best key over ALL keys at a masked j > i (asserted), so a kernel that skips or misplaces
             the mask returns another row of v (rows of v are distinct, asserted).
  uniform    (fused) q = 0: every allowed key has e = exp2(fma(0, c2, -0)) = 1 exactly, the row sum is the integer n (N, or i + 1
             under the mask), the PV product sums integers exactly, and ctx[i] = (sum_j v[j]) / n goes through 1.f / n (the Makefile
             builds with -O3 and no fast-math flag: a correctly rounded division, half an ulp; 1 ulp = 2 U24 is allowed for a
             v_rcp_f32), one f32 product (U24) and one bf16 store: |err| <= 3 U24 |y| + half_ulp_bf16(|y|).  Asserted on the reference:
             for every row and every allowed key j, losing v[j] from the product, from product and sum, adding it once more to the
             product, to product and sum, and a sum that is one too large or one too small, each move at least one element of the row
             outside its bound (a key lost or counted twice in a tail tile, a pad key counted in the sum).

Layer 2 -- real-valued operands, per-element bounds in float64.
  nt         |err| <= hd U23 |alpha| (|A| |B|^T) + U24 |c|, and for bf16 output half an ulp of the binade of the value on top
             (`store_bound`, the rule of tests/test_gemm_exact_gpu.py: one rounding to nearest, no extra factor).  alpha = hd^-0.5,
             80^-0.5 and 1: two of them are not powers of two, where rounding before the multiplication differs from rounding after it.
  nn, tn     the same with N terms.  Standard-normal operands, and the same scaled by 2^-20 and 2^10.
  fused      the model of tests/test_softmax_edges_gpu.py::test_fused_attention_forward_under_offsets, unchanged: the reference rounds
             the unnormalised e to bf16 as the kernel does; |err| <= u |ctx| + (u + 2 dx) (e |V|) / sum e + U24, u = 2^-8,
             dx = 8 U24 |S|max log2(e) + 2^-22.  ldq > 3D, ldc > D, the output a slice of a NaN buffer compared bit for bit outside.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda' if torch.cuda.is_available() else 'cpu'
U23, U24, U_BF16 = 2.0 ** -23, 2.0 ** -24, 2.0 ** -8
BF16, F32 = torch.bfloat16, torch.float32
PAD = 16                                            # columns left and right of a token-major output slice
EXTRA_ROWS = 3                                      # rows below B * N in a token-major output buffer
GUARD = 64                                          # elements before and after nt's [B,H,N,Np] block
FILL = 192.0                                        # what surrounds an operand slice
ALPHAS = (1.0, 0.5, 2.0, -1.0)
COUNTS = ((1, 1), (1, 2), (3, 1), (1, 5), (7, 1))   # (B, H): 1, 2, 3, 5, 7 problems; a workgroup holds four
EDGE_N = sorted({1, 50, 77, 101} | {16 * t + o for t in range(1, 9) for o in (-1, 0, -15)})       # every tile count, at its edges


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _int_view(t):
    return t.view({F32: torch.int32, BF16: torch.int16}[t.dtype])


def _nan_buf(shape, dtype):
    """all-ones bits: a NaN in both float types"""
    return torch.full(shape, -1, dtype={F32: torch.int32, BF16: torch.int16}[dtype], device=DEV).view(dtype)


def _tok(x):
    """[B, H, N, hd] -> token-major [B * N, H * hd]"""
    B, H, N, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * hd)


def _bits_fail(got, want, owned, what):
    """None, or where the two buffers differ bit for bit (owned: mask of the elements the kernel has to write)"""
    bad = _int_view(got) != _int_view(want)
    if not bad.any():
        return None
    n_in = int((bad & owned).sum())
    i = tuple(torch.nonzero(bad & owned if n_in else bad)[0].tolist())
    return (f'{what}: {n_in} owned elements differ, {int(bad.sum()) - n_in} foreign elements changed; first {"owned" if n_in else "foreign"} '
            f'at {i}: got {got[i].item()!r} want {want[i].item()!r}')


def _bound_fail(got, ref, bound, what):
    """None, or the elements with |got - ref| > bound (float64, per element; a NaN fails)"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if not bad.any():
        return None
    i = tuple(torch.nonzero(bad)[0].tolist())
    worst = torch.nan_to_num(err / bound, nan=math.inf).max().item()
    return (f'{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; first at {i}: got {got[i].item()!r} '
            f'ref {ref[i].item()!r} bound {bound[i].item():.3e}; worst err / bound {worst:.3f}')


def rounding_counts(y):
    """(exact ties, real roundings) among the elements of y (float64, exact in f32) on their way to bf16"""
    r = y.float().to(BF16).double()
    other = 2 * y - r
    tie = (y != r) & (other.float().to(BF16).double() == other)
    return int(tie.sum()), int(((y != r) & ~tie).sum())


def half_ulp(x):
    """half the spacing of bf16 values in the binade of x >= 0 (0 at x = 0)"""
    return torch.exp2(torch.floor(torch.log2(x)) - 8)


def store_bound(y, b, dtype):
    return b if dtype == F32 else b + half_ulp(y.abs() + b)


def block_scores(a):
    """row-major [B,H,N,Np] -> quad-blocked [B,H,Np/4,N,4] from the formula of include/dclip.h: (i, j) at ((j >> 2) * N + i) * 4 + (j & 3)"""
    B, H, N, Np = a.shape
    i = torch.arange(N, device=a.device)[:, None]
    j = torch.arange(Np, device=a.device)[None, :]
    dst = (((j >> 2) * N + i) * 4 + (j & 3)).reshape(-1)
    out = torch.empty(B, H, N * Np, dtype=a.dtype, device=a.device)
    out[:, :, dst] = a.reshape(B, H, N * Np)
    return out.view(B, H, Np // 4, N, 4)


def _operand_slices(toks, rows, D, packed, fill):
    """{which: token-major float64 [rows, D]} -> {which: bf16 column slice of a wider buffer filled with `fill`}: one packed [rows, 3D]
    buffer (slice `which` at column which * D) or a buffer of its own each (lda != ldb)"""
    if packed:
        buf = torch.full((rows, 3 * D), fill, dtype=BF16, device=DEV)
        for w, t in toks.items():
            buf[:, w * D:(w + 1) * D] = t.to(BF16)
        return {w: buf[:, w * D:(w + 1) * D] for w in toks}
    out = {}
    for w, t in toks.items():
        left = 8 * (1 + w)
        buf = torch.full((rows, left + D + 24), fill, dtype=BF16, device=DEV)
        buf[:, left:left + D] = t.to(BF16)
        out[w] = buf[:, left:left + D]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the products: cases
# ---------------------------------------------------------------------------------------------------------------------------------
class ProductCase:
    """kind nt: C[b,h,i,j] = alpha sum_d A[(b,i),h hd+d] Bm[(b,j),h hd+d]; nn: C[(b,i),h hd+d] = alpha sum_j A[b,h,i,j] Bm[(b,j),h hd+d];
    tn: C[(b,j),h hd+d] = alpha sum_i A[b,h,i,j] Bm[(b,i),h hd+d].  scale None: integers in [-31, 31] (layer 1); else N(0, 1) * scale in
    bf16 (layer 2).  ref / mag: float64, in the layout of the output (nt [B,H,N,N]; nn, tn token-major [B*N, D])."""

    def __init__(self, kind, B, H, N, hd, alpha, seed, Np=None, packed=False, scale=None):
        self.kind, self.B, self.H, self.N, self.hd, self.alpha, self.packed, self.scale = kind, B, H, N, hd, alpha, packed, scale
        self.Np = Np or (N + 7) // 8 * 8
        self.D = H * hd
        self.terms = hd if kind == 'nt' else N
        self.what = f'{kind} B={B} H={H} N={N} Np={self.Np} hd={hd} alpha={alpha:.4g} {"packed" if packed else "separate"}' + \
            (f' scale={scale:g}' if scale else '')
        for attempt in range(64):
            g = _gen(seed * 64 + attempt)
            if scale is None:
                draw = lambda *s: torch.randint(-31, 32, s, generator=g).double().to(DEV)
            else:
                draw = lambda *s: (torch.randn(s, generator=g) * scale).to(BF16).double().to(DEV)
            x = draw(B, H, N, hd if kind == 'nt' else N)            # nt: A rows ; nn / tn: the score-like A
            b = draw(B, H, N, hd)
            if kind == 'nt':
                acc, mag = x @ b.transpose(-1, -2), x.abs() @ b.abs().transpose(-1, -2)
            else:
                xm = x if kind == 'nn' else x.transpose(-1, -2)
                acc, mag = _tok(xm @ b), _tok(xm.abs() @ b.abs())
            a32 = torch.tensor(alpha, dtype=F32).item()                # the entry takes alpha as a float
            self.x, self.b, self.ref, self.mag = x, b, a32 * acc, abs(a32) * mag
            if scale is not None:
                return
            assert self.mag.max().item() < 2 ** 23, ('inputs too large for an exact probe', self.what, self.mag.max().item())
            self.ties, self.roundings = rounding_counts(self.ref)
            if self.ref.numel() < 256 or (self.ties and self.roundings):
                return
        raise AssertionError(('no draw with both exact ties and real bf16 roundings', self.what))

    def operands(self):
        """-> (A, Bm) as the entry takes them; nt: two token-major slices; nn / tn: row-major bf16 [B,H,N,Np] with zero pad columns, and a slice"""
        fill = FILL if self.scale is None else FILL * self.scale
        rows = self.B * self.N
        if self.kind == 'nt':
            s = _operand_slices({0: _tok(self.x), 1: _tok(self.b)}, rows, self.D, self.packed, fill)
            return s[0], s[1]
        w = 2 if self.kind == 'nn' else 0
        a = torch.zeros(self.B, self.H, self.N, self.Np, dtype=BF16, device=DEV)
        a[..., :self.N] = self.x.to(BF16)
        return a, _operand_slices({w: _tok(self.b)}, rows, self.D, self.packed, fill)[w]

    def bound(self, dtype):
        return store_bound(self.ref, self.terms * U23 * self.mag + U24 * self.ref.abs(), dtype)


WIDE_NP = [(16, 24), (64, 72), (80, 88), (1, 16), (50, 64), (100, 128), (113, 128), (8, 128)]   # Np > round_up(N, 8); tn picks its instance from Np


def product_sweep(kind):
    """every N from 1 to 128 for both head sizes, problem counts, alpha and the operand layout cycling; Np beyond round_up(N, 8); one grid
    of many workgroups"""
    for hd in (32, 64):
        for N in range(1, 129):
            B, H = COUNTS[(N + hd // 32) % len(COUNTS)]
            yield ProductCase(kind, B, H, N, hd, ALPHAS[(N + hd // 64) % 4], 1000 * hd + N, packed=bool((N // 2) & 1))
        for k, (N, Np) in enumerate(WIDE_NP):
            B, H = COUNTS[k % len(COUNTS)]
            yield ProductCase(kind, B, H, N, hd, ALPHAS[k % 4], 5000 * hd + N, Np=Np, packed=bool(k & 1))
    yield ProductCase(kind, 64, 24, 50, 32, 0.5, 77, packed=True)
    yield ProductCase(kind, 33, 12, 77, 64, -1.0, 78)


SHIPPED = [(8, 24, 50, 32), (8, 12, 77, 64), (8, 24, 101, 32)]


def product_real_cases(kind):
    for si, (B, H, N, hd) in enumerate(SHIPPED):
        for ki, scale in enumerate((1.0, 2.0 ** -20, 2.0 ** 10)):
            alpha = (hd ** -0.5, 80 ** -0.5, 1.0)[(si + ki) % 3]
            yield ProductCase(kind, B, H, N, hd, alpha, 300 + 10 * si + ki, packed=bool(ki & 1), scale=scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# the products: launches
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_nt(c, a, bm, out_dtype):
    """-> (flat buffer with guards, owned mask, the [B,H,N,Np] view)"""
    n = c.B * c.H * c.N * c.Np
    flat = _nan_buf((GUARD + n + GUARD,), out_dtype)
    block = flat[GUARD:GUARD + n]
    _lib().dclip_attn_nt(a.data_ptr(), a.stride(0), bm.data_ptr(), bm.stride(0), block.data_ptr(), 1 if out_dtype == F32 else 0,
                         c.B, c.H, c.N, c.Np, c.hd, c.alpha, _stream())
    owned = torch.zeros(flat.shape, dtype=torch.bool, device=DEV)
    owned[GUARD:GUARD + n] = True
    return flat, owned, block.view(c.B, c.H, c.N, c.Np)


def _launch_tok(c, a, bm, blocked):
    """nn / tn -> (wide buffer, owned mask, the [B*N, D] slice); the output alternates between a padded buffer and the middle third of a
    packed [rows, 3D] one"""
    rows, D = c.B * c.N, c.D
    left, width = (D, 3 * D) if c.packed else (PAD, D + 2 * PAD)
    wide = _nan_buf((rows + EXTRA_ROWS, width), BF16)
    out = wide[:rows, left:left + D]
    if blocked:
        a = block_scores(a)
    fn = _lib().dclip_attn_nn if c.kind == 'nn' else _lib().dclip_attn_tn
    fn(a.data_ptr(), bm.data_ptr(), bm.stride(0), out.data_ptr(), wide.stride(0), c.B, c.H, c.N, c.Np, c.hd, c.alpha, blocked, _stream())
    owned = torch.zeros(wide.shape, dtype=torch.bool, device=DEV)
    owned[:rows, left:left + D] = True
    return wide, owned, out


def product_launches(c):
    """every variant of the case's entry: nt f32 / bf16 output ; nn, tn row-major / quad-blocked A.  -> [(label, buffer, owned, view, dtype)]"""
    a, bm = c.operands()
    if c.kind == 'nt':
        return [(f'{c.what} {str(od)[6:]}',) + _launch_nt(c, a, bm, od) + (od,) for od in (F32, BF16)]
    return [(f'{c.what} a_blocked={bl}',) + _launch_tok(c, a, bm, bl) + (BF16,) for bl in (0, 1)]


def exact_product(c):
    """layer 1 -> failure strings"""
    fails = []
    for label, buf, owned, view, od in product_launches(c):
        want = _nan_buf(tuple(buf.shape), od)
        if c.kind == 'nt':
            wv = want[GUARD:GUARD + view.numel()].view(view.shape)
            wv[:] = 0                                      # pad columns [N, Np): +0
            wv[..., :c.N] = c.ref.float().to(od)
        else:
            left = c.D if c.packed else PAD
            want[:c.B * c.N, left:left + c.D] = c.ref.float().to(od)
        fails.append(_bits_fail(buf, want, owned, label))
    return [f for f in fails if f]


def bound_product(c):
    """layer 2 -> failure strings"""
    fails = []
    for label, buf, owned, view, od in product_launches(c):
        got = view[..., :c.N] if c.kind == 'nt' else view
        fails.append(_bound_fail(got, c.ref, c.bound(od), label))
        blank = _nan_buf(tuple(buf.shape), od)
        chk = buf.clone()
        if c.kind == 'nt':
            if torch.count_nonzero(_int_view(view[..., c.N:].contiguous())):
                fails.append(label + ': pad columns are not +0')
            chk[owned] = blank[owned]
        else:
            chk[owned] = blank[owned]
        fails.append(_bits_fail(chk, blank, owned, label + ' outside'))
    return [f for f in fails if f]


def _report(fails, n):
    assert not fails, f'{len(fails)} failures in {n} cases:\n' + '\n'.join(fails[:40])


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused forward: cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _keep(N, causal):
    m = torch.ones(N, N, dtype=torch.bool, device=DEV)
    return m.tril_() if causal else m


def _stride_for(N):
    return next(s for s in (7, 11, 13, 5, 3, 9, 1) if math.gcd(s, N) == 1)


class SelectionCase:
    """module docstring, `selection`.  q, k, v: float64 [B,H,N,hd] of bf16-exact values; t: [B,H,N] the selected key of every query"""

    def __init__(self, B, H, N, hd, causal, seed):
        assert not causal or B * H >= 2, 'a causal case needs a second problem for the off-diagonal pattern'
        self.B, self.H, self.N, self.hd, self.causal = B, H, N, hd, causal
        self.what = f'selection B={B} H={H} N={N} hd={hd} causal={int(causal)}'
        P, scale = B * H, hd ** -0.5
        i = torch.arange(N)
        p = torch.arange(P)[:, None]
        if causal:
            o = ((p + 2 * i[None, :]) % 8) * 5
            t = i[None, :] - o % (i[None, :] + 1)
            t[0] = i                                                     # the only map with t(i) <= i onto every key
        else:
            t = (_stride_for(N) * i[None, :] + 3 * p + 1) % N
            ident = (t == i[None, :]).all(1)
            t[ident] = (t[ident] + 1) % N                                # (N = 2, odd p: the stride alone gives the diagonal)
        t = t.view(B, H, N).to(DEV)
        keep = _keep(N, causal)
        for attempt in range(64):
            g = _gen(seed * 64 + attempt)
            w = (torch.randint(0, 2, (B, H, N, hd), generator=g) * 2 - 1).double().to(DEV)
            v = torch.randint(-120, 121, (B, H, N, hd), generator=g).double().to(DEV)
            k = 32 * w
            q = 32 * torch.gather(w, 2, t[..., None].expand(B, H, N, hd))
            if causal:
                h = N // 2
                q[..., 0] = 0
                k[..., 0] = 0
                q[:, :, :h, 0] = 512
                k[:, :, h:, 0] = 256
            s = scale * (q @ k.transpose(-1, -2))
            target = torch.gather(s, 3, t[..., None])
            rivals = s.masked_fill(~keep, -math.inf).scatter(3, t[..., None], -math.inf)
            gap = (target - rivals.amax(-1, keepdim=True)).min().item()
            distinct = (torch.cdist(v, v) + torch.eye(N, device=DEV) > 0).all().item()
            if gap >= 200 and distinct:
                break
        self.q, self.k, self.v, self.t, self.gap = q, k, v, t, gap
        # --- the conditions, every row of every problem ---
        assert gap >= 200, (self.what, 'selection gap', gap)
        assert distinct, (self.what, 'two rows of v are equal')
        assert (t >= 0).all() and (t < N).all() and bool(torch.gather(keep.expand(B, H, N, N), 3, t[..., None]).all()), (self.what, 't not allowed')
        assert (target * 1.4426950408889634).abs().max().item() < 2 ** 14, (self.what, 'm c2 too large for e to round to 1')
        hits = torch.zeros(P, N, dtype=torch.bool, device=DEV).scatter_(1, t.view(P, N), True)
        if causal:
            assert hits.any(0).all(), (self.what, 'a key is never selected')
            off = (t.view(P, N)[1:] != torch.arange(N, device=DEV)).double().mean().item() if N >= 16 else 1.0
            assert off >= 0.5, (self.what, 'too few off-diagonal selections', off)
            if N >= 2:
                best = s.argmax(-1)
                share = (best > torch.arange(N, device=DEV)).double().mean(-1).min().item()
                assert share * 3 >= 1 - 1e-12, (self.what, 'share of rows whose best key is masked', share)
        else:
            assert hits.all(), (self.what, 'a key is never selected in some problem')
            assert N == 1 or (t != torch.arange(N, device=DEV)).any(-1).all(), (self.what, 't is the diagonal')
        self.expect = torch.gather(v, 2, t[..., None].expand(B, H, N, hd))

    def qkv(self):
        return torch.cat([_tok(self.q), _tok(self.k), _tok(self.v)], 1)


def selection_cases():
    for hd in (32, 64):
        for N in range(1, 129):
            for causal in (False, True):
                B, H = COUNTS[(N + hd // 32 + causal) % len(COUNTS)]
                if causal and B * H == 1:
                    B, H = 2, 2
                yield SelectionCase(B, H, N, hd, causal, 7 * N + hd + causal)
    yield SelectionCase(64, 12, 101, 64, False, 5)
    yield SelectionCase(64, 8, 77, 64, True, 6)


class UniformCase:
    """module docstring, `uniform`.  y: float64 [B,H,N,hd], bound: per element"""

    def __init__(self, B, H, N, hd, causal, seed):
        self.B, self.H, self.N, self.hd, self.causal = B, H, N, hd, causal
        self.what = f'uniform B={B} H={H} N={N} hd={hd} causal={int(causal)}'
        keep = _keep(N, causal).double()
        n = keep.sum(-1, keepdim=True)                                   # [N, 1]
        for attempt in range(16):
            g = _gen(seed * 16 + attempt)
            k = (torch.randint(0, 2, (B, H, N, hd), generator=g) * 64 - 32).double().to(DEV)
            v = torch.randint(-120, 121, (B, H, N, hd), generator=g).double().to(DEV)
            tot = keep @ v                                               # [B,H,N,hd]: sum over the allowed keys of row i
            y = tot / n
            bound = store_bound(y, 3 * U24 * y.abs(), BF16)
            weak = self._insensitive(v, tot, y, bound, keep, n)
            if not weak:
                break
        assert not weak, (self.what, 'a single lost / doubled key stays inside the bound', weak)
        assert tot.abs().max().item() < 2 ** 23
        self.q, self.k, self.v, self.y, self.bound = torch.zeros_like(k), k, v, y, bound

    @staticmethod
    def _insensitive(v, tot, y, bound, keep, n):
        """the first (model, problem, row, key) whose faulty value stays within the bound in every element of the row, or None.  (A row with
        ONE allowed key has no value without it, and the key counted twice in product and sum gives (v + v) / 2 = v: those three models
        apply to rows of two or more keys.)"""
        B, H, N, hd = v.shape
        T, Y, Bd = tot[:, :, :, None, :], y[:, :, :, None, :], bound[:, :, :, None, :]         # [B,H,i,1,d]
        V = v[:, :, None, :, :]                                                               # [B,H,1,j,d]
        nn = n.view(1, 1, N, 1, 1)
        allowed = keep.bool().view(1, 1, N, N)
        models = {'lost in the product': ((T - V) / nn, None), 'doubled in the product': ((T + V) / nn, None),
                  'lost in product and sum': ((T - V) / (nn - 1), 2), 'doubled in product and sum': ((T + V) / (nn + 1), 2),
                  'sum one too large': (T / (nn + 1) + 0 * V, None), 'sum one too small': (T / (nn - 1) + 0 * V, 2)}
        for name, (faulty, nmin) in models.items():
            moved = ((faulty - Y).abs() > Bd).any(-1)                                         # [B,H,i,j]
            need = allowed if nmin is None else allowed & (nn[..., 0] >= nmin)
            bad = need & ~moved
            if bad.any():
                return (name,) + tuple(torch.nonzero(bad)[0].tolist())
        return None

    def qkv(self):
        return torch.cat([_tok(self.q), _tok(self.k), _tok(self.v)], 1)


def uniform_cases():
    for hd in (32, 64):
        for ni, N in enumerate(EDGE_N):
            for causal in (False, True):
                B, H = COUNTS[(ni + causal + hd // 32) % len(COUNTS)]
                yield UniformCase(B, H, N, hd, causal, 11 * N + hd + causal)


class FusedRealCase:
    """layer 2: standard-normal bf16 q, k, v and the error model of test_fused_attention_forward_under_offsets"""

    def __init__(self, B, H, N, hd, causal, seed):
        self.B, self.H, self.N, self.hd, self.causal = B, H, N, hd, causal
        self.what = f'fused B={B} H={H} N={N} hd={hd} causal={int(causal)}'
        g = _gen(seed)
        q, k, v = ((torch.randn((B, H, N, hd), generator=g)).to(BF16).double().to(DEV) for _ in range(3))
        s = q @ k.transpose(-1, -2) * hd ** -0.5
        sm = s.masked_fill(~_keep(N, causal), -math.inf)
        e = torch.exp(sm - sm.amax(-1, keepdim=True))
        den = e.sum(-1, keepdim=True)
        self.y = (e.to(BF16).double() @ v) / den
        dx = 8 * U24 * s.abs().max().item() * 1.4427 + 2 ** -22
        self.bound = U_BF16 * self.y.abs() + (U_BF16 + 2 * dx) * (e @ v.abs()) / den + U24
        self.q, self.k, self.v = q, k, v

    def qkv(self):
        return torch.cat([_tok(self.q), _tok(self.k), _tok(self.v)], 1)


FUSED_COUNTS = ((1, 1), (3, 1), (1, 5), (7, 1))       # 1, 3, 5, 7 problems: the launch puts 4 or 2 in a workgroup
TEACHERS = [(64, 12, 50, 64, False), (64, 12, 101, 64, False), (64, 8, 77, 64, True)]


def fused_real_cases():
    n = 0
    for hd in (32, 64):
        for N in sorted({16 * t + o for t in range(1, 9) for o in (-1, 0, -15)}):
            for causal in (False, True):
                B, H = FUSED_COUNTS[n % 4]
                n += 1
                yield FusedRealCase(B, H, N, hd, causal, 900 + n)
    for i, (B, H, N, hd, causal) in enumerate(TEACHERS):
        yield FusedRealCase(B, H, N, hd, causal, 990 + i)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused forward: launches
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_fused(c, extra_ldq=16):
    """qkv [B*N, 3D + extra_ldq] (the extra columns hold FILL), ctx a column slice of a NaN buffer with rows below B*N -> (wide, owned, slice)"""
    rows, D = c.B * c.N, c.H * c.hd
    buf = torch.full((rows, 3 * D + extra_ldq), FILL, dtype=BF16, device=DEV)
    buf[:, :3 * D] = c.qkv().to(BF16)
    wide = _nan_buf((rows + EXTRA_ROWS, D + 2 * PAD), BF16)
    out = wide[:rows, PAD:PAD + D]
    _lib().dclip_attn_fused_fwd(buf.data_ptr(), buf.stride(0), out.data_ptr(), wide.stride(0), c.B, c.H, c.N, c.hd, c.hd ** -0.5,
                                1 if c.causal else 0, _stream())
    owned = torch.zeros(wide.shape, dtype=torch.bool, device=DEV)
    owned[:rows, PAD:PAD + D] = True
    return wide, owned, out


def exact_fused(c):
    wide, owned, out = launch_fused(c)
    want = _nan_buf(tuple(wide.shape), BF16)
    want[:out.shape[0], PAD:PAD + out.shape[1]] = _tok(c.expect).to(BF16)
    f = _bits_fail(wide, want, owned, c.what)
    return [f] if f else []


def bound_fused(c, extra_ldq=16):
    wide, owned, out = launch_fused(c, extra_ldq)
    fails = [_bound_fail(out, _tok(c.y), _tok(c.bound), c.what)]
    blank = _nan_buf(tuple(wide.shape), BF16)
    chk = wide.clone()
    chk[owned] = blank[owned]
    fails.append(_bits_fail(chk, blank, owned, c.what + ' outside'))
    return [f for f in fails if f]


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_block_scores_agrees_with_unblock_scores():
    from distillclip_amd import ops
    for N, Np in ((1, 8), (50, 56), (77, 80), (64, 72), (128, 128)):
        a = torch.randn((2, 3, N, Np), generator=_gen(N)).to(BF16).to(DEV)
        blk = block_scores(a)
        assert blk.shape == (2, 3, Np // 4, N, 4) and torch.equal(ops.unblock_scores(blk), a)
        i, j = N - 1, Np - 3
        assert blk.reshape(2, 3, -1)[1, 2, ((j >> 2) * N + i) * 4 + (j & 3)] == a[1, 2, i, j]


@pytest.mark.parametrize('kind', ['nt', 'nn', 'tn'])
def test_products_exact_every_n(kind):
    """layer 1 over product_sweep: N = 1..128, both head sizes, Np beyond round_up(N, 8), 1..7 problems and grids of many workgroups"""
    fails, n, ties, roundings = [], 0, 0, 0
    for c in product_sweep(kind):
        n += 1
        ties, roundings = ties + c.ties, roundings + c.roundings
        fails += exact_product(c)
    assert n == 2 * (128 + len(WIDE_NP)) + 2 and ties > 1000 and roundings > 1000, (n, ties, roundings)
    _report(fails, n)


@pytest.mark.parametrize('kind', ['nt', 'nn', 'tn'])
def test_products_bounds_shipped_shapes(kind):
    """layer 2 at the towers' shapes: standard-normal operands, and scaled by 2^-20 and 2^10"""
    fails, n = [], 0
    for c in product_real_cases(kind):
        n += 1
        fails += bound_product(c)
    assert n == 9
    _report(fails, n)


@pytest.mark.parametrize('hd', [32, 64])
def test_products_bounds_every_tile_edge(hd):
    """layer 2 at N = 16 t - 1, 16 t, 16 t - 15 (and 50, 77, 101), alpha not a power of two"""
    fails, n = [], 0
    for kind in ('nt', 'nn', 'tn'):
        for ni, N in enumerate(EDGE_N):
            B, H = COUNTS[ni % len(COUNTS)]
            n += 1
            fails += bound_product(ProductCase(kind, B, H, N, hd, (hd ** -0.5, 80 ** -0.5)[ni & 1], 400 + N, packed=bool(ni & 1), scale=1.0))
    _report(fails, n)


def test_fused_selects_one_key_exactly():
    fails, n = [], 0
    for c in selection_cases():
        n += 1
        fails += exact_fused(c)
    assert n == 2 * 128 * 2 + 2
    _report(fails, n)


def test_fused_uniform_weights():
    fails, n = [], 0
    for c in uniform_cases():
        n += 1
        fails += bound_fused(c)
    assert n == 4 * len(EDGE_N)
    _report(fails, n)


def test_fused_bounds_tile_edges_and_teacher_shapes():
    fails, n = [], 0
    for c in fused_real_cases():
        n += 1
        fails += bound_fused(c, extra_ldq=(16, 0, 40)[n % 3])
    assert n == 2 * 24 * 2 + len(TEACHERS)
    _report(fails, n)


def test_attention_entries_refuse_bad_arguments():
    """each entry returns DCLIP_EINVAL (a ValueError) before any launch: the NaN-filled output stays bit-unchanged.  (hd = 48 through
    dclip_attn_nt is asserted in tests/test_cabi_cpu.py.)"""
    l = _lib()
    B, H, N, Np, hd = 2, 2, 16, 16, 32
    D = H * hd
    tokm = torch.ones((B * N + 1, 3 * D), dtype=BF16, device=DEV)
    sc = torch.zeros((B, H, N + 8, Np + 8), dtype=BF16, device=DEV)
    out = _nan_buf((B * H * (N + 8) * (Np + 8) + 64,), F32)
    blank = out.clone()
    o, a, t, st = out.data_ptr(), sc.data_ptr(), tokm.data_ptr(), _stream()
    bad = {
        'nt': lambda **k: l.dclip_attn_nt(t, k.get('ld', 3 * D), t + 2 * D, 3 * D, o, 1, B, H, k.get('N', N), k.get('Np', Np), k.get('hd', hd), 1.0, st),
        'nn': lambda **k: l.dclip_attn_nn(a, t + k.get('boff', 0), k.get('ld', 3 * D), o + k.get('coff', 0), k.get('ldc', D), B, H, k.get('N', N),
                                          k.get('Np', Np), k.get('hd', hd), 1.0, 0, st),
        'tn': lambda **k: l.dclip_attn_tn(a, t + k.get('boff', 0), k.get('ld', 3 * D), o + k.get('coff', 0), k.get('ldc', D), B, H, k.get('N', N),
                                          k.get('Np', Np), k.get('hd', hd), 1.0, 1, st),
        'fused': lambda **k: l.dclip_attn_fused_fwd(t + k.get('boff', 0), k.get('ld', 3 * D), o + k.get('coff', 0), k.get('ldc', D), B, H,
                                                    k.get('N', N), k.get('hd', hd), 0.125, 0, st),
    }
    common = [dict(N=0), dict(N=129, Np=136), dict(ld=3 * D + 4)]
    per_entry = {
        'nt': [dict(Np=8), dict(Np=20), dict(N=128, Np=136)],
        'nn': [dict(hd=48), dict(Np=8), dict(Np=20), dict(N=128, Np=136), dict(ldc=D + 4), dict(boff=8), dict(coff=8)],
        'tn': [dict(hd=48), dict(Np=8), dict(Np=20), dict(N=128, Np=136), dict(ldc=D + 4), dict(boff=8), dict(coff=8)],
        'fused': [dict(hd=48), dict(ldc=D + 4), dict(boff=8), dict(coff=8)],
    }
    for name, call in bad.items():
        for kw in common + per_entry[name]:
            with pytest.raises(ValueError):
                call(**kw)
            torch.cuda.synchronize()
            assert torch.equal(_int_view(out), _int_view(blank)), (name, kw, 'the output changed')
