"""dclip_attn_stream_fwd (the long-sequence companion of dclip_attn_fused_fwd: frozen ViT-B/16 / ViT-L/14 teachers, 197 / 257 / 577
tokens) element by element against float64, in the two layers of tests/test_attn_exact_gpu.py, whose helpers and case builders this
file imports.  The builders below assert the premises of every probe on the float64 reference alone; tests/test_long_teacher_cpu.py
runs them without a GPU and without the library.

The kernel walks the keys in chunks of KC = 64 (attention.hip: SKC).  Per query and chunk c it takes m_c = max(m_(c-1), chunk maximum)
of the raw scores, a_c = exp2(fma(m_(c-1), c2, -(m_c c2))), e_j = exp2(fma(s_j, c2, -(m_c c2))) for the chunk's keys (c2 = scale log2 e,
m_c c2 rounded once), and updates  O <- O a_c + sum_j bf16(e_j) v_j  (f32; the sum on the matrix pipe),  l <- fma(l, a_c, sum_j e_j);
at the end ctx = bf16(O * (1.f / l)).  m_(-1) = -inf, so a_0 = exp2(-inf) = 0 meets O = l = 0.

Layer 1 -- exact probes, no tolerance.
  uniform    q = 0: every raw score is +0, so m_c = 0 from the first chunk on and nm = -(0 c2) = -0.  Every e is exp2(fma(0, c2, -0)) =
             exp2(+0) = 1 exactly, and every later rescale factor is exp2(fma(0, c2, -0)) = 1 too: the maximum never moves, O and l are
             multiplied by 1 and stay the integers sum v_j and the key count (asserted: sum |v| < 2^23, so any order of f32 additions is
             exact).  The bound of the register-resident kernel, 3 U24 |y| + half_ulp_bf16(|y|) (1.f / n within 1 ulp, one f32 product,
             one bf16 store), holds unchanged.  Asserted on the reference for every problem and key j: losing v[j] from the product, from
             product and sum, counting it twice in the product, in product and sum, each move an element of the row outside its bound; a
             sum that is one too large or too small does for N <= 256 (the move is |y| / (N +- 1), and half a bf16 ulp of |y| is at
             least |y| / 512: above N = 512 no bf16 output can show it, between 256 and 512 only elements in the upper part of their
             binade; those two models are asserted up to 256 and left out above).
  selection  SelectionCase of the imported file without the mask: q_i = 32 w_t(i), k_j = 32 w_j, distinct +-1 words, t a permutation
             with a stride per problem.  The scaled score of key t(i) is at least 200 above every other key (asserted there for every
             row), i.e. more than 288 in the exponent's base-2 units (asserted here: gap log2 e > 288).  Chunks before the one that
             holds t(i): finite O and l relative to a smaller maximum.  In that chunk the maximum moves up by more than 288 / c2, so
             a = exp2(less than -288) = 0 exactly (f32, denormals included) and everything accumulated so far is multiplied by 0; the
             chunk's other keys have e = 0 for the same reason, and e_t = exp2(fma(m, c2, -(m c2))) = 1 +- 2^-11 rounds to a bf16 1
             (|m c2| < 2^14 asserted there).  Every later chunk has e = 0 and a = exp2(fma(m, c2, -(m c2))) within 2^-11 of 1 -- but
             l = e_t a and O = v[t] a carry the SAME factor, computed once: ctx = (v[t] a ..) / (e_t a ..) with one f32 rounding per
             product, so ctx lies within 2^-10 |v| + a few U24 |v| of v[t], less than half a bf16 ulp (>= 2^-9 |v|): ctx[i] == v[t(i)]
             BIT FOR BIT.  Asserted here: in every problem every chunk holds the selected key of some query -- the first chunk, every
             middle one and the last (the stride permutation also sends the queries of one 16-query tile to different chunks).
Layer 2 -- standard-normal bf16 q, k, v; per-element bound in float64.
  The reference forms e_j = exp(s_j - m_c) against the RUNNING maximum m_c of the chunk that holds j, rounds it to bf16 there, as the
  kernel does, and carries it to the final maximum in float64: y = (sum_j bf16(e_j) g_j v_j) / (sum_j e_j g_j), g_j = exp(m_c(j) - m_last).
  (Asserted on the reference: without the bf16 rounding this is the plain softmax product to 1e-12.)  With w = (e g |V|) / sum e g,
  u = 2^-8, dx = 8 U24 |S|max log2(e) + 2^-22 (the exponent's argument error: f32 scores of hd bf16 products and one fma),
  nc = number of key chunks:
      |err| <= u |ctx|                      the bf16 store
             + (u + 2 dx) w                 bf16 rounding of e; the argument error of e in numerator and denominator
             + nc (10 U24 + 2 dx) w         per chunk: one f32 rounding of O a and one of fma(l, a, .) (2 U24); a itself is exp2 of an
                                            argument with error <= dx, within 1 ulp (2 U24): relative error dx + 2 U24 on the weight of
                                            every earlier key, in numerator and denominator (2 (dx + 2 U24)); the chunk's two 32-key
                                            MFMA steps accumulate into O in f32 (2 x 2 U24)
             + 4 U24 |ctx| + U24            1.f / l (1 ulp), the product O inv, and the absolute slack of the imported bound.
  The terms beside u are five orders of magnitude below it: the bound is, to three digits, the one of the register-resident kernel.
Every output is a column slice (ldc > D) of an all-NaN buffer with rows below B N, compared bit for bit outside the owned elements;
qkv rows carry extra columns (ldq > 3 D) filled with 192.
"""
import math

import pytest
import torch

import test_attn_exact_gpu as ax
from test_attn_exact_gpu import BF16, DEV, PAD, EXTRA_ROWS, FILL, U24, U_BF16

pytestmark = pytest.mark.gpu

KC = 64                                               # the kernel's key chunk (attention.hip: SKC)
HD = 64
LOG2E = 1.4426950408889634
ISSUE_N = (129, 144, 145, 197, 257, 577)
CHUNK_EDGE_N = tuple(KC * t + o for t in (1, 2, 3, 4, 5, 9, 10) for o in (-1, 0, 1))          # just below, at and just above chunk multiples
SMALL_N = (1, 15, 16, 17, 50)                         # the entry takes any N >= 1
ALL_N = tuple(sorted(set(ISSUE_N + CHUNK_EDGE_N + SMALL_N)))
COUNTS = ax.COUNTS                                    # (B, H): 1, 2, 3, 5, 7 problems
BIG_GRID = (16, 12, 197)                              # 16 * 12 problems x 4 query blocks = 768 workgroups


def nchunks(N):
    return (N + KC - 1) // KC


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def selection_case(B, H, N, seed):
    """ax.SelectionCase (non-causal) + the premises of the running-maximum argument"""
    c = ax.SelectionCase(B, H, N, HD, False, seed)
    assert c.gap * LOG2E > 288, (c.what, 'the rescale factor at the selected chunk is not exactly 0', c.gap)
    t = c.t.view(B * H, N)
    chunk = t // KC
    nc = nchunks(N)
    for p in range(B * H):
        assert len(set(chunk[p].tolist())) == nc, (c.what, 'a chunk never holds a selected key', p)
    return c


def selection_cases():
    for ni, N in enumerate(ALL_N):
        B, H = COUNTS[ni % len(COUNTS)]
        yield selection_case(B, H, N, 13 * N + 1)
    yield selection_case(*BIG_GRID, 5)


class UniformCase:
    """module docstring, `uniform`: q = 0, k = +-32, integer v.  Without a mask every row of a problem has the same y = sum_j v[j] / N."""

    def __init__(self, B, H, N, seed):
        self.B, self.H, self.N, self.hd, self.causal = B, H, N, HD, False
        self.what = f'uniform B={B} H={H} N={N}'
        for attempt in range(16):
            g = ax._gen(seed * 16 + attempt)
            k = (torch.randint(0, 2, (B, H, N, HD), generator=g) * 64 - 32).double().to(DEV)
            v = torch.randint(-120, 121, (B, H, N, HD), generator=g).double().to(DEV)
            tot = v.sum(2, keepdim=True)                                 # [B,H,1,hd]
            y = tot / N
            bound = ax.store_bound(y, 3 * U24 * y.abs(), BF16)
            weak = self._insensitive(v, tot, y, bound, N)
            if not weak:
                break
        assert not weak, (self.what, 'a single lost / doubled key stays inside the bound', weak)
        assert v.abs().sum(2).max().item() < 2 ** 23, (self.what, 'sums not exact in f32')
        self.q, self.k, self.v = torch.zeros_like(k), k, v
        assert (self.q @ k.transpose(-1, -2)).abs().max().item() == 0          # every score is 0: e = 1, the maximum never moves
        self.y, self.bound = y.expand(B, H, N, HD), bound.expand(B, H, N, HD)

    @staticmethod
    def _insensitive(v, tot, y, bound, N):
        """the first (model, problem, key) whose faulty value stays within the bound in every element of the row, or None"""
        models = {'lost in the product': (tot - v) / N, 'doubled in the product': (tot + v) / N,
                  'lost in product and sum': (tot - v) / max(N - 1, 1), 'doubled in product and sum': (tot + v) / (N + 1)}
        if N == 1:
            del models['lost in product and sum'], models['doubled in product and sum']       # (no value without the only key; (v + v) / 2 = v)
        if N <= 256:
            models['sum one too large'] = tot / (N + 1) + 0 * v
            if N >= 2:
                models['sum one too small'] = tot / (N - 1) + 0 * v
        for name, faulty in models.items():
            moved = ((faulty - y).abs() > bound).any(-1)                 # [B,H,j]
            if not moved.all():
                return (name,) + tuple(torch.nonzero(~moved)[0].tolist())
        return None

    def qkv(self):
        return torch.cat([ax._tok(self.q), ax._tok(self.k), ax._tok(self.v)], 1)


def uniform_cases():
    for ni, N in enumerate(ALL_N):
        B, H = COUNTS[(ni + 2) % len(COUNTS)]
        yield UniformCase(B, H, N, 17 * N + 3)


class RealCase:
    """layer 2 (module docstring): standard-normal bf16 operands, e rounded to bf16 against the running maximum of its chunk"""

    def __init__(self, B, H, N, seed):
        self.B, self.H, self.N, self.hd, self.causal = B, H, N, HD, False
        self.what = f'stream B={B} H={H} N={N}'
        g = ax._gen(seed)
        q, k, v = ((torch.randn((B, H, N, HD), generator=g)).to(BF16).double().to(DEV) for _ in range(3))
        s = q @ k.transpose(-1, -2) * HD ** -0.5
        nc = nchunks(N)
        pad = nc * KC - N
        sp = torch.nn.functional.pad(s, (0, pad), value=-math.inf).view(B, H, N, nc, KC)
        run = torch.cummax(sp.amax(-1), -1).values                       # [B,H,N,nc]: m_c
        m_of_key = run[..., None].expand(B, H, N, nc, KC).reshape(B, H, N, nc * KC)[..., :N]
        m_last = run[..., -1:]
        e = torch.exp(s - m_of_key)                                      # what the kernel rounds to bf16
        carry = torch.exp(m_of_key - m_last)
        den = (e * carry).sum(-1, keepdim=True)
        self.y = ((e.to(BF16).double() * carry) @ v) / den
        plain = torch.softmax(s, -1) @ v
        exact = ((e * carry) @ v) / den
        assert (exact - plain).abs().max().item() <= 1e-12 * max(1.0, plain.abs().max().item()), self.what
        self.moves = int((run[..., 1:] > run[..., :-1]).sum()) if nc > 1 else 0        # how often a running maximum moved
        dx = 8 * U24 * s.abs().max().item() * 1.4427 + 2 ** -22
        w = ((e * carry) @ v.abs()) / den
        self.bound = U_BF16 * self.y.abs() + (U_BF16 + 2 * dx) * w + nc * (10 * U24 + 2 * dx) * w + 4 * U24 * self.y.abs() + U24
        self.q, self.k, self.v = q, k, v

    def qkv(self):
        return torch.cat([ax._tok(self.q), ax._tok(self.k), ax._tok(self.v)], 1)


def real_cases():
    for ni, N in enumerate(ALL_N):
        B, H = COUNTS[(ni + 1) % len(COUNTS)]
        yield RealCase(B, H, N, 700 + N)
    yield RealCase(*BIG_GRID, 699)


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_stream(c, extra_ldq=16):
    """ax.launch_fused for the new entry: qkv [B*N, 3D + extra_ldq], ctx a column slice of a NaN buffer with rows below B*N"""
    rows, D = c.B * c.N, c.H * c.hd
    buf = torch.full((rows, 3 * D + extra_ldq), FILL, dtype=BF16, device=DEV)
    buf[:, :3 * D] = c.qkv().to(BF16)
    wide = ax._nan_buf((rows + EXTRA_ROWS, D + 2 * PAD), BF16)
    out = wide[:rows, PAD:PAD + D]
    ax._lib().dclip_attn_stream_fwd(buf.data_ptr(), buf.stride(0), out.data_ptr(), wide.stride(0), c.B, c.H, c.N, c.hd, c.hd ** -0.5, ax._stream())
    owned = torch.zeros(wide.shape, dtype=torch.bool, device=DEV)
    owned[:rows, PAD:PAD + D] = True
    return wide, owned, out


def exact_stream(c, extra_ldq=16):
    wide, owned, out = launch_stream(c, extra_ldq)
    want = ax._nan_buf(tuple(wide.shape), BF16)
    want[:out.shape[0], PAD:PAD + out.shape[1]] = ax._tok(c.expect).to(BF16)
    f = ax._bits_fail(wide, want, owned, c.what)
    return [f] if f else []


def bound_stream(c, extra_ldq=16):
    wide, owned, out = launch_stream(c, extra_ldq)
    fails = [ax._bound_fail(out, ax._tok(c.y), ax._tok(c.bound), c.what)]
    blank = ax._nan_buf(tuple(wide.shape), BF16)
    chk = wide.clone()
    chk[owned] = blank[owned]
    fails.append(ax._bits_fail(chk, blank, owned, c.what + ' outside'))
    return [f for f in fails if f]


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_selects_one_key_exactly():
    fails, n = [], 0
    for c in selection_cases():
        n += 1
        fails += exact_stream(c, extra_ldq=(16, 0, 40)[n % 3])
    assert n == len(ALL_N) + 1
    ax._report(fails, n)


def test_stream_uniform_weights():
    fails, n = [], 0
    for c in uniform_cases():
        n += 1
        fails += bound_stream(c, extra_ldq=(0, 16, 40)[n % 3])
    assert n == len(ALL_N)
    ax._report(fails, n)


def test_stream_bounds_real_operands():
    fails, n, moves = [], 0, 0
    for c in real_cases():
        n += 1
        moves += c.moves
        fails += bound_stream(c, extra_ldq=(40, 16, 0)[n % 3])
    assert n == len(ALL_N) + 1 and moves > 1000, (n, moves)               # the running maximum did move: the rescale path ran
    ax._report(fails, n)


def test_stream_agrees_with_the_register_resident_kernel_below_129():
    """the two kernels differ in where e is rounded, not in what they compute: at N <= 128 both satisfy their float64 bounds on the same
    operands (the towers send such N to dclip_attn_fused_fwd; the new entry takes them too)"""
    fails = []
    for N in (50, 101, 128):
        c = RealCase(3, 2, N, 40 + N)
        fails += bound_stream(c)
        f = ax.FusedRealCase(3, 2, N, HD, False, 40 + N)
        fails += ax.bound_fused(f)
    ax._report(fails, 6)


def test_stream_refuses_bad_arguments():
    """each refusal is DCLIP_EINVAL (a ValueError) before any launch: the NaN-filled output stays bit-unchanged"""
    l = ax._lib()
    B, H, N = 2, 2, 130
    D = H * HD
    qkv = torch.ones((B * N + 1, 3 * D + 8), dtype=BF16, device=DEV)
    out = ax._nan_buf((B * N + 4, D + 16), BF16)
    blank = out.clone()
    t, o, st = qkv.data_ptr(), out.data_ptr(), ax._stream()
    call = lambda **k: l.dclip_attn_stream_fwd(k.get('q', t) + k.get('boff', 0), k.get('ld', 3 * D + 8), k.get('c', o) + k.get('coff', 0), k.get('ldc', D + 16),
                                               k.get('B', B), k.get('H', H), k.get('N', N), k.get('hd', HD), 0.125, st)
    call()                                                                # (the good call runs: the refusals below are about their argument)
    torch.cuda.synchronize()
    out.copy_(blank)
    for kw in (dict(hd=48), dict(hd=32), dict(N=0), dict(N=-3), dict(B=0), dict(H=0), dict(ld=3 * D + 4), dict(ldc=D + 4), dict(ld=3 * D - 8),
               dict(ldc=D - 8), dict(boff=8), dict(coff=8), dict(q=0), dict(c=0)):
        with pytest.raises(ValueError):
            call(**kw)
        torch.cuda.synchronize()
        assert torch.equal(ax._int_view(out), ax._int_view(blank)), (kw, 'the output changed')


def test_ops_wrapper():
    from distillclip_amd import ops
    c = RealCase(2, 3, 197, 77)
    got = ops.attn_stream_fwd(c.qkv().to(BF16).contiguous(), c.B, c.N, c.H, HD)
    f = ax._bound_fail(got, ax._tok(c.y), ax._tok(c.bound), c.what)
    assert not f, f
