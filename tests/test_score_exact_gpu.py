"""The attention score stages between QK^T and PV, element by element against float64: dclip_attn_softmax_fwd / _bwd (attn_softmax.hip: the
plain, VALU-mix and MFMA-mix kernels) and the register-resident dclip_attn_mix_fwd / _bwd (attention_mix.hip + attn_mix_wave.h).
tests/test_kernels_gpu.py holds them to max-error-over-max-value of a whole tensor, tests/test_softmax_edges_gpu.py to per-element
bounds at three shapes with logits made sharp by a per-ROW constant, which never moves the running softmax reference of the register
kernel.  This file follows tests/test_attn_exact_gpu.py: CPU-generator draws, float64 references, builders that assert their own input
conditions (tests/test_score_exact_cpu.py runs every one of them without the library), outputs inside all-ones-bits (NaN) buffers with
guard elements on both sides, compared whole.  EPS = 2^-24, U_BF16 = 2^-8, U_F16 = 2^-11.

Layer 1 -- exact probes, no tolerance.
  selection  Head h of query i selects key t_h(i) by a gap so large that P is exactly one-hot; W_l is a permutation matrix pi (identity,
             rotate by 1, rotate by H/2 + 1, reversal: A_g = S_pi(g)); W_w has entries k / 64, 0 < |k| <= 128 (exact in bf16 and f16,
             every (g, h) pair non-zero).  Then R_g[i, j] = sum over {h : t_pi(h)(i) = j} of W_w[g, h]: an exact f32 sum (multiples of 1/64
             below 2^6) in ANY order, rounded once to bf16, compared BIT FOR BIT; P is the one-hot itself; pad columns are +0.
             t_h has a stride and an offset per (b, h): without the mask it is a permutation of the keys, so every key of every quad and
             tile is selected in every problem (asserted).
             unfused: S is fed directly.  The selected entry is c[b, h, i], an even integer with |c| <= 300 (bf16-exact: the split-bf16
               operands of the MFMA kernel hold it in the hi part alone) whose sign alternates over the heads, every other allowed
               entry is c - 200 (an integer: exact in f32 and in a hi + lo pair).  exp(-200) = 2^-288.5 is 0 in f32, so e is exactly
               one-hot, the row sum is 1, 1 / 1 = v_rcp_f32(1) = 1.  Causal cases (plain and VALU) take t_h(i) <= i as
               test_attn_exact_gpu does, and the rows i < N // 2 hold c + 64 at the masked keys j >= N // 2: a third of the rows or
               more have their best key over all keys at a masked j > i (asserted).
             register: q_i = 16 w_t(i), k_j = 16 w_j with +-1 words w per (b, h): raw scores are multiples of 512 up to 256 hd <= 16384,
               exact in f16 and inside its range (asserted).  The kernel's mix operand is f16(W_l * f32(scale * log2 e)): A' = that
               times the raw score of head pi(g), an 11-bit by 6-bit product that f32 holds exactly, as it does every difference of
               two of them (so `m += d` lands on the new maximum exactly).  Asserted for every row: the gap to every other key is
               >= 500 log2 units (exp2 of it is 0 in f32, so is l * exp2(-d) when the reference moves), the f32 row sum is exactly 1,
               the f16 copy of P is exactly one-hot, argmax = t_pi(g).  Rows whose key lies beyond the first quad FORCE a move of the
               running reference by hundreds of log2 units (counted, asserted > 0 for N > 4).  stats = max_j A' ln 2 within
               4 EPS (|lse| + 1) + da, da = H EPS max_j (|W_l'| |raw|) + 2^-20 (test_register_resident_mix_under_offsets).
               In half the cases qkv has ld = 3D + 8 or 3D + 64, the surplus columns filled with 192.
  uniform    S constant per (b, h, i) (register: q = 0): every allowed key has e = 1, the row sum is the integer n (N, or i + 1 under
             the mask), P = 1 / n.  W_l and W_w are permutations.  Plain and VALU divide (IEEE: -O3, no fast-math): bit-equal to
             bf16(f32(1 / n)).  MFMA takes v_rcp_f32 (1 ulp), splits P = hi + lo (hi is the saved P) and forms R = bf16(hi + lo): the
             builder asserts for every n <= 128 that the three f32 values within one ulp of 1 / n give the same bits, none is dropped.
             Register: |err| <= (U_BF16 + U_F16 + 2 da) / n + EPS, and 1 / (n +- 1) lies outside that bound for every n (asserted): a key
             lost or counted twice shows.

Layer 2 -- per-element bounds, the error models of test_softmax_edges_gpu.py term by term.
  steep      (register) q, k as _qkv_with_offsets(quantised=True) there, but the offset feature varies ALONG THE KEYS: q[i, 0] = a_i in
             {1.5, 0.25, 1, 0, 0.5, 0.25, 1.5, 0} cycling with i + h, k[j, 0] = u_{b,h,j}, an integer profile with |u| <= 280 (ascending
             ramp, descending ramp, flat -140 with a spike of +280 on the last key, five-step staircase, cycling over h, sign flipped
             with b).  Asserted: raw scores exact in f16, |raw| < 512.  A float64 replay of pass 1 of fwd_item (reference from the first
             quad, threshold 24, wave-wide trigger, every register of the wave rescaled) asserts that at least 3/4 of the (sample, tile)
             items move their reference at least once, and that registers with 0 < d <= 24 and a non-zero running sum are rescaled
             alongside: the rows where a wrong rescale is not hidden below 2^-24.  stats and R: bounds of
             test_register_resident_mix_under_offsets.  Backward (dS, dW_l, dW_w): the same test's bounds, EXCEPT that the reference P
             is the FORWARD MODEL's P (f16 W_l log2(e) scale, exact raw scores) with pf = da + 4 EPS (|lse2| + 1) for the stored
             statistic instead of the exact-graph P with pf = U_F16 |W_l| |S|: at |S| ~ 80 that term is several percent and would hide
             everything.  One term is ADDED to that test's dS bound, the one its plain-kernel bound already carries: the row sum
             delta_g = sum_k P_g[k] dP_g[k] is formed from dR rounded to bf16 (U_BF16 |W_w|^T |dR| = U_BF16 dp_abs per term) and from
             P (relative error pf), so |err delta_g| <= (U_BF16 + pf) sigma_g, sigma_g = sum_k P_g[k] dp_abs_g[k]; it enters dA_g[j] times
             P_g[j] and dS through |W_l|^T: t3 = |W_l|^T (P sigma) next to t2 = |W_l|^T (P dp_abs), with t2's factors.  Without it an
             element with dP[j] ~ delta (a small dA left by cancellation) has no allowance for the error of delta; the test prints
             the worst err / bound against the bound without t3 next to the asserted one.
             The _rows forms: R, stats and dS bit-equal to the full forms on the picked tile, the other rows left alone; their dW_l
             and dW_w within the full form's bounds, every sum restricted to the query rows of the picked tiles.
             The same cases run through dclip_attn_nt -> dclip_attn_softmax_fwd / _bwd once per kernel kind with the bounds of
             test_attention_softmax_stage_under_offsets.
  edges      ordinary random operands at every N of MIX_N: the unfused kernels (forward, backward, weight gradients accumulated over
             two calls, once per mixing kernel with bf16 scores) with the bounds of test_attention_softmax_stage_under_offsets, the
             register stage (every reachable instantiation at every N, forward, backward, two calls) with the bounds of `steep`, and one batch
             whose backward needs more than one persistent round.

Wide Np.  dclip_attn_softmax_fwd / _bwd take any multiple of 8 with N <= Np <= 128 like the product entries (64-key slots chosen from
  Np): selection and edge cases at WIDE_NP of test_attn_exact_gpu, pad columns of P, R, dS +0, guards intact; Np = 136 and Np < N are
  refused, and dclip_attn_mix_* refuse Np != round_up(N, 8), each with nothing written.
"""
import functools
import math

import pytest
import torch

from test_attn_exact_gpu import (BF16, DEV, F32, FILL, GUARD, WIDE_NP, _bits_fail, _bound_fail, _gen, _int_view, _keep, _lib,
                                 _nan_buf, _report, _stream, _tok, block_scores)

pytestmark = pytest.mark.gpu

EPS, U_BF16, U_F16 = 2.0 ** -24, 2.0 ** -8, 2.0 ** -11
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
RESCALE_THR = 24.0                                   # attn_mix_wave.h
MIX_N = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 20, 21, 31, 32, 33, 48, 49, 63, 64, 65, 100, 101, 125, 127, 128]
# MIX_DISPATCH has a ninth instance, (H, hd) = (2, 32), that no call can reach: dclip_attn_mix_supported wants H * hd % 128 == 0 (a quad of
# token rows is a whole number of 1-KiB LDS-DMA pieces).  test_score_entries_refuse_other_np holds the entries to that refusal.
REG_INST = [(2, 64), (4, 32), (4, 64), (8, 32), (8, 64), (12, 32), (12, 64), (24, 32)]
UNFUSED_MIX = [(2, False), (2, True), (4, False), (4, True), (8, False), (8, True), (12, False), (12, True), (24, True), (24, False)]
STEEP_SHAPES = [(2, 24, 50, 32), (2, 24, 101, 32), (2, 12, 77, 64), (2, 12, 16, 32), (2, 8, 77, 32), (2, 8, 128, 64), (2, 4, 128, 64),
                (2, 4, 5, 32), (2, 2, 33, 64), (2, 2, 64, 64), (1, 12, 101, 32), (2, 8, 17, 64)]
MULTI_ROUND = (150, 2, 101, 64)                      # B * ceil(N / 16) / 4 = 263 workgroups > the backward's 256 persistent ones


def mix_kind(H, mix, causal):
    """dclip_attn_softmax_fwd's dispatch"""
    return 'plain' if not mix else ('mfma' if H > 12 and not causal else 'valu')


def round8(N):
    return (N + 7) // 8 * 8


def perms(H):
    """identity, rotate by 1, rotate by H/2 + 1, reversal (index vectors pi: A_g = S_pi(g))"""
    i = torch.arange(H)
    return [i, (i + 1) % H, (i + H // 2 + 1) % H, H - 1 - i]


def perm_matrix(pi):
    H = pi.numel()
    w = torch.zeros(H, H, dtype=torch.float64)
    w[torch.arange(H), pi] = 1.0
    return w


def grid_weights(H, g):
    """entries k / 64, 0 < |k| <= 128"""
    k = torch.randint(1, 129, (H, H), generator=g) * (torch.randint(0, 2, (H, H), generator=g) * 2 - 1)
    return k.double() / 64


def select_map(B, H, N, causal, seed):
    """t[b, h, i], the key that head h of query i selects (module docstring)"""
    i = torch.arange(N)[None, :]
    p = torch.arange(B * H)[:, None]
    if causal:
        o = ((p + 2 * i) % 8) * 5
        t = i - o % (i + 1)
        t[0] = i[0]                                                  # the only map with t(i) <= i onto every key
    else:
        strides = [s for s in (1, 3, 5, 7, 9, 11, 13) if math.gcd(s, N) == 1]
        st = torch.tensor([strides[(k + seed) % len(strides)] for k in range(B * H)])[:, None]
        t = (st * i + 3 * p + seed) % N
    t = t.view(B, H, N)
    hits = torch.zeros(B * H, N, dtype=torch.bool).scatter_(1, t.view(B * H, N), True)
    assert (hits.any(0) if causal else hits).all(), ('a key is never selected', B, H, N, causal)
    assert not causal or (t <= torch.arange(N)).all()
    return t.to(DEV)


def _gap(a, keep, tsel):
    """smallest distance of the selected entry to the largest other allowed entry over all rows (inf where a row allows one key)"""
    am = a.masked_fill(~keep, -math.inf)
    target = torch.gather(am, 3, tsel[..., None])
    rivals = am.scatter(3, tsel[..., None], -math.inf)
    assert torch.equal(am.argmax(-1), tsel), 'the selected key is not the largest allowed one'
    return (target - rivals.amax(-1, keepdim=True)).min().item()


def _onehot(tsel, N):
    return torch.zeros(tsel.shape + (N,), dtype=torch.float64, device=DEV).scatter_(3, tsel[..., None], 1.0)


def _mix(w, x):
    return torch.einsum('gh,bhij->bgij', w, x)


def _mixt(w, x):
    return torch.einsum('gh,bgij->bhij', w, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def guarded(n, dtype):
    """-> (flat NaN buffer with GUARD elements on both sides, the n owned elements)"""
    flat = _nan_buf((GUARD + n + GUARD,), dtype)
    return flat, flat[GUARD:GUARD + n]


def owned_mask(n):
    m = torch.zeros(GUARD + n + GUARD, dtype=torch.bool, device=DEV)
    m[GUARD:GUARD + n] = True
    return m


def want_buf(block, dtype):
    """the whole expected buffer around `block` (float64 values exact in `dtype`, or a tensor of `dtype`)"""
    n = block.numel()
    w = _nan_buf((GUARD + n + GUARD,), dtype)
    w[GUARD:GUARD + n] = block.reshape(-1).to(dtype)
    return w


def pad_rows(x, Np):
    """float64 [B,H,N,N] -> [B,H,N,Np] with +0 pad columns"""
    out = torch.zeros(x.shape[:-1] + (Np,), dtype=x.dtype, device=x.device)
    out[..., :x.shape[-1]] = x
    return out


def guards_fail(flat, n, dtype, what):
    """None, or how the guard elements around the n owned ones changed"""
    chk = flat.clone()
    chk[GUARD:GUARD + n] = _nan_buf((n,), dtype)
    return _bits_fail(chk, _nan_buf(tuple(flat.shape), dtype), owned_mask(n), what + ' guards')


def pads_fail(block, N, what):
    """None, or a complaint when a pad column of the row-major [B,H,N,Np] block is not +0"""
    bad = int(torch.count_nonzero(_int_view(block[..., N:].contiguous())))
    return f'{what}: {bad} pad elements are not +0' if bad else None


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfused stage: exact probes
# ---------------------------------------------------------------------------------------------------------------------------------
class StageSelect:
    """module docstring, `selection`, unfused.  s: f32 [B,H,N,Np]; wl, ww: f32 [H,H] or None; p, r: float64 [B,H,N,N]"""

    def __init__(self, B, H, N, mix, causal, pi_idx, seed, Np=None):
        self.B, self.H, self.N, self.mix, self.causal, self.Np = B, H, N, mix, causal, Np or round8(N)
        self.kind = mix_kind(H, mix, causal)
        self.what = f'stage selection {self.kind} B={B} H={H} N={N} Np={self.Np} causal={int(causal)} perm={pi_idx}'
        g = _gen(seed)
        t = select_map(B, H, N, causal, seed)
        sign = torch.where(torch.arange(H) % 2 == 0, 1, -1).view(1, H, 1)
        c = (sign * 2 * torch.randint(0, 151, (B, H, N), generator=g)).double().to(DEV)
        s = (c[..., None] - 200).expand(B, H, N, N).clone().scatter_(3, t[..., None], c[..., None])
        keep = _keep(N, causal)
        if causal and N >= 2:
            h = N // 2
            s[:, :, :h, h:] = c[:, :, :h, None] + 64
            share = (s.argmax(-1) > torch.arange(N, device=DEV)).double().mean(-1).min().item()
            assert share * 3 >= 1 - 1e-12, (self.what, 'share of rows whose best key is masked', share)
        pi = perms(H)[pi_idx].to(DEV)
        a, tsel = (s[:, pi], t[:, pi]) if mix else (s, t)
        self.gap = _gap(a, keep, tsel)
        assert self.gap >= 199, (self.what, 'selection gap', self.gap)               # e^-199 = 2^-287: 0 in f32, denormals included
        assert s.abs().max().item() <= 500 and torch.equal(c, c.to(BF16).double()) and torch.equal(s, s.float().double())
        self.p = _onehot(tsel, N)
        if mix:
            self.wl, ww = perm_matrix(pi.cpu()).float().to(DEV), grid_weights(H, g).to(DEV)
            assert (ww != 0).all() and torch.equal(ww, ww.to(BF16).double()) and torch.equal(ww, ww.half().double())
            self.ww, self.r = ww.float(), _mix(ww, self.p)
            assert torch.equal(self.r, self.r.float().double())
        else:
            self.wl = self.ww = None
            self.r = self.p
        self.s = pad_rows(s, self.Np).float()
        self.tsel = tsel


def _rcp_candidates(n):
    """f32(1 / n) and its two f32 neighbours, for n a float64 tensor of integers"""
    r0 = (torch.ones_like(n).float() / n.float())
    return r0, torch.nextafter(r0, torch.zeros_like(r0)), torch.nextafter(r0, torch.full_like(r0, 2.0))


def _hi_lo_sum(r):
    """the MFMA kernel's R for P = r (f32) through a permutation W_w: bf16(hi + lo), hi = bf16(r), lo = bf16(r - hi)"""
    hi = r.to(BF16)
    lo = (r - hi.float()).to(BF16)
    return hi, (hi.float() + lo.float()).to(BF16)


@functools.lru_cache(maxsize=None)
def unstable_reciprocals(nmax=128):
    """the n <= nmax for which the three f32 values within one ulp of 1 / n do not store the same bf16 bits (P and R of the MFMA kernel)"""
    n = torch.arange(1, nmax + 1, dtype=torch.float64)
    outs = [_hi_lo_sum(r) for r in _rcp_candidates(n)]
    bad = torch.zeros(nmax, dtype=torch.bool)
    for hi, rr in outs[1:]:
        bad |= (_int_view(hi) != _int_view(outs[0][0])) | (_int_view(rr) != _int_view(outs[0][1]))
    return tuple((torch.nonzero(bad)[:, 0] + 1).tolist())


class StageUniform:
    """module docstring, `uniform`, unfused.  p_bits, r_bits: bf16 [B,H,N,N], what the kernel has to store"""

    def __init__(self, B, H, N, mix, causal, pi_idx, seed, Np=None):
        self.B, self.H, self.N, self.mix, self.causal, self.Np = B, H, N, mix, causal, Np or round8(N)
        self.kind = mix_kind(H, mix, causal)
        self.what = f'stage uniform {self.kind} B={B} H={H} N={N} Np={self.Np} causal={int(causal)} perm={pi_idx}'
        g = _gen(seed)
        sign = torch.where(torch.arange(H) % 2 == 0, 1, -1).view(1, H, 1)
        c = (sign * 2 * torch.randint(0, 151, (B, H, N), generator=g)).double()
        assert torch.equal(c, c.to(BF16).double())
        keep = _keep(N, causal)
        n = keep.double().sum(-1, keepdim=True)                                      # [N, 1]
        r0 = _rcp_candidates(n.cpu())[0].to(DEV)
        assert not unstable_reciprocals(N), (self.what, 'a reciprocal within one ulp stores other bits')
        hi, rr = _hi_lo_sum(r0)
        zero = torch.zeros((), dtype=BF16, device=DEV)
        self.p_bits = torch.where(keep, hi.expand(N, N), zero).expand(B, H, N, N)
        self.r_bits = torch.where(keep, (rr if self.kind == 'mfma' else hi).expand(N, N), zero).expand(B, H, N, N)
        self.n = n
        if mix:
            pis = perms(H)
            self.wl, self.ww = perm_matrix(pis[pi_idx]).float().to(DEV), perm_matrix(pis[(pi_idx + 1) % 4]).float().to(DEV)
        else:
            self.wl = self.ww = None
        self.s = pad_rows(c.to(DEV)[..., None].expand(B, H, N, N), self.Np).float()


def launch_stage_fwd(c):
    """-> (P flat, R flat, P block, R block), blocks as [B,H,N,Np]"""
    n = c.B * c.H * c.N * c.Np
    pf, pb = guarded(n, BF16)
    rf, rb = guarded(n, BF16)
    s = c.s.contiguous()
    _lib().dclip_attn_softmax_fwd(s.data_ptr(), c.wl.data_ptr() if c.mix else None, c.ww.data_ptr() if c.mix else None, pb.data_ptr(),
                                  rb.data_ptr(), c.B, c.H, c.N, c.Np, 1 if c.causal else 0, _stream())
    shape = (c.B, c.H, c.N, c.Np)
    return pf, rf, pb.view(shape), rb.view(shape)


def exact_stage(c, p_want, r_want):
    """p_want, r_want: [B,H,N,N] (float64 exact in bf16, or bf16) -> failure strings; one bit comparison per output buffer"""
    pf, rf, _, _ = launch_stage_fwd(c)
    n = c.B * c.H * c.N * c.Np
    fails = [_bits_fail(pf, want_buf(pad_rows(p_want, c.Np), BF16), owned_mask(n), c.what + ' P'),
             _bits_fail(rf, want_buf(pad_rows(r_want, c.Np), BF16), owned_mask(n), c.what + ' R')]
    return [f for f in fails if f]


def stage_counts(ni):
    """B cycles over 1, 2, 3"""
    return (1, 2, 3)[ni % 3]


def plain_cases(cls):
    """every N from 1 to 128, H in {1, 3, 16} and the mask cycling"""
    for N in range(1, 129):
        for causal in (False, True):
            yield cls(stage_counts(N + causal), (1, 3, 16)[(N + 2 * causal) % 3], N, False, causal, 0, 3 * N + causal)


def mix_cases(cls):
    """every mixing kernel instance at every N of MIX_N, the permutation and the batch cycling"""
    for ni, N in enumerate(MIX_N):
        for ki, (H, causal) in enumerate(UNFUSED_MIX):
            yield cls(stage_counts(ni + ki), H, N, True, causal, (ni + ki) % 4, 50 * N + ki)


def wide_cases(cls):
    """Np beyond round_up(N, 8): every kernel kind at every pair of WIDE_NP"""
    for k, (N, Np) in enumerate(WIDE_NP):
        for ki, (H, mix, causal) in enumerate([(3, False, False), (16, False, True), (4, True, False), (12, True, True), (24, True, False)]):
            yield cls(stage_counts(k + ki), H, N, mix, causal, (k + ki) % 4, 900 + 10 * k + ki, Np=Np)


# ---------------------------------------------------------------------------------------------------------------------------------
# the register-resident stage: cases
# ---------------------------------------------------------------------------------------------------------------------------------
def kernel_wl16(wl, hd):
    """f16(W_l * f32(scale * log2 e)) as fwd_load_weights packs it (f32 products), float64 [H,H]"""
    sc = torch.tensor(hd ** -0.5, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    return (wl.float().cpu() * sc).half().double().to(DEV)


def qkv_buffer(q, k, v, extra):
    """float64 [B,H,N,hd] x 3 (bf16-exact) -> bf16 [B*N, 3D + extra], the surplus columns filled with FILL"""
    rows, D = q.shape[0] * q.shape[2], q.shape[1] * q.shape[3]
    buf = torch.full((rows, 3 * D + extra), FILL, dtype=BF16, device=DEV)
    buf[:, :3 * D] = torch.cat([_tok(q), _tok(k), _tok(v)], 1).to(BF16)
    assert torch.equal(buf[:, :3 * D].double(), torch.cat([_tok(q), _tok(k), _tok(v)], 1))
    return buf


class RegCase:
    """what the register-stage launches need: B, H, N, hd, wl, ww (f32 [H,H] on DEV), q, k, v (float64 [B,H,N,hd]), extra (ld - 3D)"""

    def qkv(self):
        return qkv_buffer(self.q, self.k, self.v, self.extra)

    def model(self):
        """the forward model: raw exact, a2 = f16 mix in the log2 domain, lse2, p, r (f16 W_w), da"""
        raw = self.q @ self.k.transpose(-1, -2)
        wl16, ww16 = kernel_wl16(self.wl, self.hd), self.ww.half().double()
        a2 = _mix(wl16, raw)
        lse2 = torch.logsumexp(a2 * LN2, -1) / LN2
        p = torch.exp2(a2 - lse2[..., None])
        da = self.H * EPS * _mix(wl16.abs(), raw.abs()).amax(-1, keepdim=True) + 2 ** -20
        return raw, a2, lse2, p, _mix(ww16, p), _mix(ww16.abs(), p), da


class RegSelect(RegCase):
    """module docstring, `selection`, register"""

    def __init__(self, B, H, N, hd, pi_idx, seed, extra=0):
        self.B, self.H, self.N, self.hd, self.extra = B, H, N, hd, extra
        self.what = f'register selection B={B} H={H} N={N} hd={hd} perm={pi_idx} ld=3D+{extra}'
        t = select_map(B, H, N, False, seed)
        pi = perms(H)[pi_idx].to(DEV)
        self.wl = perm_matrix(pi.cpu()).float().to(DEV)
        wl16 = kernel_wl16(self.wl, hd)
        tsel, keep = t[:, pi], _keep(N, False)
        for attempt in range(64):
            g = _gen(seed * 64 + attempt)
            w = (torch.randint(0, 2, (B, H, N, hd), generator=g) * 2 - 1).double().to(DEV)
            k = 16 * w
            q = 16 * torch.gather(w, 2, t[..., None].expand(B, H, N, hd))
            raw = q @ k.transpose(-1, -2)
            a2 = _mix(wl16, raw)
            gap = _gap(a2, keep, tsel) if (a2.argmax(-1) == tsel).all() else 0.0
            if gap >= 500:
                break
        v = torch.randint(-120, 121, (B, H, N, hd), generator=g).double().to(DEV)
        self.q, self.k, self.v, self.gap = q, k, v, gap
        self.ww = grid_weights(H, g).float().to(DEV)
        # --- the conditions, every row of every problem ---
        assert gap >= 500, (self.what, 'selection gap (log2 units)', gap)
        assert torch.equal(raw, raw.half().double()) and raw.abs().max().item() <= 256 * hd <= 16384 and (raw % 512 == 0).all(), self.what
        assert torch.equal(a2, a2.float().double()), (self.what, 'a mixed score is not exact in f32')
        e = torch.exp2(a2 - a2.amax(-1, keepdim=True)).float()
        hot = _onehot(tsel, N)
        assert (e.sum(-1) == 1).all() and torch.equal(e.half().double(), hot), (self.what, 'P is not exactly one-hot')
        self.moved = int((tsel >= 4).sum())                                          # registers whose reference has to move
        assert N <= 4 or (self.moved > 0 and int((tsel < 4).sum()) > 0), (self.what, 'no key beyond / inside the first quad')
        self.r = _mix(self.ww.double(), hot)
        assert torch.equal(self.r, self.r.float().double()) and (self.ww != 0).all() and torch.equal(self.ww.double(), self.ww.half().double())
        self.lse = a2.amax(-1) * LN2
        da = H * EPS * _mix(wl16.abs(), raw.abs()).amax(-1) + 2 ** -20
        self.lse_bound = da + 4 * EPS * (self.lse.abs() + 1)


class RegUniform(RegCase):
    """module docstring, `uniform`, register"""

    def __init__(self, B, H, N, hd, pi_idx, seed, extra=0):
        self.B, self.H, self.N, self.hd, self.extra = B, H, N, hd, extra
        self.what = f'register uniform B={B} H={H} N={N} hd={hd} perm={pi_idx} ld=3D+{extra}'
        g = _gen(seed)
        self.k = (torch.randint(0, 2, (B, H, N, hd), generator=g) * 64 - 32).double().to(DEV)
        self.v = torch.randint(-120, 121, (B, H, N, hd), generator=g).double().to(DEV)
        self.q = torch.zeros_like(self.k)
        pis = perms(H)
        self.wl, self.ww = perm_matrix(pis[pi_idx]).float().to(DEV), perm_matrix(pis[(pi_idx + 1) % 4]).float().to(DEV)
        self.r = torch.full((B, H, N, N), 1.0 / N, dtype=torch.float64, device=DEV)
        self.bound = (U_BF16 + U_F16 + 2 * 2 ** -20) * self.r + EPS
        for other in (N - 1, N + 1):                                                 # one key lost or counted twice
            assert other == 0 or abs(1.0 / other - 1.0 / N) > self.bound.max().item(), (self.what, 'insensitive to one key', other)
        self.lse = torch.full((B, H, N), math.log(N), dtype=torch.float64, device=DEV)
        self.lse_bound = 2 ** -20 + 4 * EPS * (self.lse.abs() + 1)


def steep_profile(kind, N, flip):
    """integer key profile u_j, |u| <= 280"""
    j = torch.arange(N, dtype=torch.float64)
    if kind == 0:
        u = torch.round(-280 + 560 * j / max(N - 1, 1))
    elif kind == 1:
        u = torch.round(280 - 560 * j / max(N - 1, 1))
    elif kind == 2:
        u = torch.full((N,), -140.0, dtype=torch.float64)
        u[-1] = 280
    else:
        u = -280 + 140 * torch.floor(5 * j / N)
    return -u if flip else u


A_CYCLE = (1.5, 0.25, 1.0, 0.0, 0.5, 0.25, 1.5, 0.0)


class RegSteep(RegCase):
    """module docstring, `steep`; steep=False: ordinary quantised operands (the `edges` of the register stage)"""

    def __init__(self, B, H, N, hd, seed, extra=0, steep=True):
        self.B, self.H, self.N, self.hd, self.extra = B, H, N, hd, extra
        self.what = f'register {"steep" if steep else "edge"} B={B} H={H} N={N} hd={hd} ld=3D+{extra}'
        g = _gen(seed)
        q, k, v = (0.5 * torch.randint(-2, 3, (B, H, N, hd), generator=g).double() for _ in range(3))
        if steep:
            i, h = torch.arange(N)[None, :], torch.arange(H)[:, None]
            q[..., 0] = torch.tensor(A_CYCLE, dtype=torch.float64)[(i + h) % 8]
            for b in range(B):
                for hh in range(H):
                    k[b, hh, :, 0] = steep_profile(hh % 4, N, bool(b & 1)).to(BF16).double()      # (integers above 256: the even ones)
        self.q, self.k, self.v = q.to(DEV), k.to(DEV), v.to(DEV)
        from test_softmax_edges_gpu import _wmat
        self.wl, self.ww = _wmat(H, 5 + H, 0.15).float().to(DEV), _wmat(H, 6 + H, 0.15).float().to(DEV)
        raw = self.q @ self.k.transpose(-1, -2)
        self.raw_max = raw.abs().max().item()
        assert torch.equal(raw, raw.half().double()) and self.raw_max < 512, (self.what, 'raw scores not exact in f16 / too large', self.raw_max)
        self.d_ctx = torch.randn((B * N, H * hd), generator=g).to(BF16).double().to(DEV)


def replay_pass1(a2):
    """float64 replay of pass 1 of fwd_item on the log2-domain scores a2 [B,H,N,N]: reference m from the first quad, per quad the rise
    d = max(0, max over the quad of a - m) of every register, and when ANY register of the (sample, 16-query tile) wave has d > 24 every
    register of the wave takes m += d, l *= 2^-d.  -> (lse2 [B,H,N], moves [B, tiles], alongside: registers moved with 0 < d <= 24, l > 0)"""
    B, H, N, _ = a2.shape
    QT = (N + 15) // 16
    tile = (torch.arange(N, device=a2.device) // 16)
    m = a2[..., :min(4, N)].amax(-1)
    l = torch.zeros_like(m)
    moves = torch.zeros(B, QT, dtype=torch.long, device=a2.device)
    alongside = 0
    for j0 in range(0, N, 4):
        av = a2[..., j0:j0 + 4] - m[..., None]
        d = av.amax(-1).clamp(min=0)
        over = torch.zeros(B, H, QT * 16, dtype=torch.bool, device=a2.device)
        over[..., :N] = d > RESCALE_THR
        big = over.view(B, H, QT, 16).any(3).any(1)                                  # [B, QT]: hw::any over the wave
        moves += big
        bigr = big[:, None, :].expand(B, H, QT)[:, :, tile]                          # [B,H,N]: this register's wave moves
        alongside += int((bigr & (d > 0) & (d <= RESCALE_THR) & (l > 0)).sum())
        d = torch.where(bigr, d, torch.zeros_like(d))
        m = m + d
        l = l * torch.exp2(-d) + torch.exp2(av - d[..., None]).sum(-1)
    return m + torch.log2(l), moves, alongside


def reg_extra(k):
    return (0, 8, 0, 64)[k % 4]


def reg_select_cases(cls=RegSelect):
    """every reachable instantiation at every N of MIX_N, then one launch of more workgroups than a persistent round"""
    for ni, N in enumerate(MIX_N):
        for ki, (H, hd) in enumerate(REG_INST):
            yield cls(stage_counts(ni + ki), H, N, hd, (ni + ki) % 4, 40 * N + ki, extra=reg_extra(ni + ki))
    B, H, N, hd = MULTI_ROUND
    yield cls(B, H, N, hd, 1, 7, extra=8)


def reg_steep_cases():
    for k, (B, H, N, hd) in enumerate(STEEP_SHAPES):
        yield RegSteep(B, H, N, hd, 60 + k, extra=reg_extra(k))


def reg_edge_cases():
    for ni, N in enumerate(MIX_N):
        for ki, (H, hd) in enumerate(REG_INST):      # every instantiation at every N
            yield RegSteep(stage_counts(ni + ki), H, N, hd, 300 + 10 * ni + ki, extra=reg_extra(ni + ki), steep=False)
    B, H, N, hd = MULTI_ROUND                        # the backward's persistent waves take a second item
    yield RegSteep(B, H, N, hd, 499, extra=8, steep=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the register-resident stage: launches
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_reg_fwd(c, qkv, pick=None):
    """-> (R flat, stats flat, R block (quad-blocked, flat), stats block [B,H,N]); pick: int32 [B] -> the _rows form"""
    Np = round8(c.N)
    n, ns = c.B * c.H * c.N * Np, c.B * c.H * c.N
    (rf, rb), (sf, sb) = guarded(n, BF16), guarded(ns, F32)
    args = (qkv.data_ptr(), qkv.stride(0), c.wl.data_ptr(), c.ww.data_ptr(), rb.data_ptr(), sb.data_ptr(), c.B, c.H, c.N, Np, c.hd, c.hd ** -0.5)
    if pick is None:
        _lib().dclip_attn_mix_fwd(*args, _stream())
    else:
        _lib().dclip_attn_mix_fwd_rows(*args, pick.data_ptr(), _stream())
    return rf, sf, rb, sb.view(c.B, c.H, c.N)


def unblock(rb, c):
    """flat quad-blocked block -> row-major [B,H,N,Np]"""
    Np = round8(c.N)
    return rb.view(c.B, c.H, Np // 4, c.N, 4).permute(0, 1, 3, 2, 4).reshape(c.B, c.H, c.N, Np)


def launch_reg_bwd(c, qkv, stats, dwl, dww, pick=None):
    """-> (dS flat, dS block); d_ctx rides in a wider buffer (ldo > D) when the case has surplus columns"""
    Np, D = round8(c.N), c.H * c.hd
    n = c.B * c.H * c.N * Np
    dsf, dsb = guarded(n, BF16)
    do = torch.full((c.B * c.N, D + (8 if c.extra else 0)), FILL, dtype=BF16, device=DEV)
    do[:, :D] = c.d_ctx.to(BF16)
    ws_bytes = _lib().dclip_attn_mix_bwd_workspace_bytes(c.B, c.H, c.N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    args = (qkv.data_ptr(), qkv.stride(0), do.data_ptr(), do.stride(0), c.wl.data_ptr(), c.ww.data_ptr(), stats.data_ptr(), dsb.data_ptr(),
            dwl.data_ptr(), dww.data_ptr(), ws.data_ptr(), ws_bytes, c.B, c.H, c.N, Np, c.hd, c.hd ** -0.5)
    if pick is None:
        _lib().dclip_attn_mix_bwd(*args, _stream())
    else:
        _lib().dclip_attn_mix_bwd_rows(*args, pick.data_ptr(), _stream())
    return dsf, dsb


def exact_reg(c):
    """layer 1 -> failure strings: R bit for bit in its guarded buffer, stats within its bound, its guards intact"""
    Np = round8(c.N)
    rf, sf, rb, sb = launch_reg_fwd(c, c.qkv())
    n = c.B * c.H * c.N * Np
    want = want_buf(block_scores(pad_rows(c.r, Np)), BF16)
    fails = [_bits_fail(rf, want, owned_mask(n), c.what + ' R'), _bound_fail(sb, c.lse, c.lse_bound, c.what + ' stats'),
             guards_fail(sf, c.B * c.H * c.N, F32, c.what + ' stats')]
    return [f for f in fails if f]


WORST = {}


def _note(name, got, ref, bound):
    w = torch.nan_to_num((got.double() - ref).abs() / bound, nan=math.inf).max().item()
    WORST[name] = max(WORST.get(name, 0.0), w)


def bound_reg_fwd(c, label):
    """layer 2 forward -> (failure strings, the launch's buffers): stats and R against the forward model, pad columns +0, guards intact"""
    raw, a2, lse2, p, r, rabs, da = c.model()
    rf, sf, rb, sb = launch_reg_fwd(c, c.qkv())
    R = unblock(rb, c)
    lse_bound = da[..., 0] + 4 * EPS * (lse2.abs() + 1)
    r_bound = (U_BF16 + U_F16 + 2 * da) * rabs + EPS
    _note(f'{label} stats', sb, lse2 * LN2, lse_bound)
    _note(f'{label} R', R[..., :c.N], r, r_bound)
    fails = [_bound_fail(sb, lse2 * LN2, lse_bound, c.what + ' stats'), _bound_fail(R[..., :c.N], r, r_bound, c.what + ' R'),
             pads_fail(R, c.N, c.what + ' R'), guards_fail(rf, R.numel(), BF16, c.what + ' R'),
             guards_fail(sf, sb.numel(), F32, c.what + ' stats')]
    return [f for f in fails if f], (rf, sf, rb, sb)


def reg_bwd_model(c):
    """the backward reference (module docstring: the forward model's P, pf from the stored statistic) -> dict of float64 tensors"""
    raw, _, lse2, p, _, _, da = c.model()
    do = c.d_ctx.view(c.B, c.N, c.H, c.hd).permute(0, 2, 1, 3)
    dr = do @ c.v.transpose(-1, -2)
    wld, wwd = c.wl.double(), c.ww.double()
    dp, dp_abs = _mixt(wwd, dr), _mixt(wwd.abs(), dr.abs())
    da_ref = p * (dp - (p * dp).sum(-1, keepdim=True))
    ds_ref = _mixt(wld, da_ref)
    t1, t2 = _mixt(wld.abs(), da_ref.abs()), _mixt(wld.abs(), p * dp_abs)
    pf = da + 4 * EPS * (lse2.abs()[..., None] + 1)
    # pf and the row sum belong to the OUTPUT head g of the forward mix: they multiply P_g before the adjoint mix W_l^T carries them to head h
    sigma = (p * dp_abs).sum(-1, keepdim=True)
    t3 = _mixt(wld.abs(), p * sigma)
    ds_bound = 2 * U_BF16 * (2 * t1 + t2 + t3) + 2 * _mixt(wld.abs(), pf * p * (dp_abs + sigma)) + U_BF16 * ds_ref.abs() + EPS
    ds_bound_short = 2 * U_BF16 * (2 * t1 + t2) + 2 * _mixt(wld.abs(), pf * p * dp_abs) + U_BF16 * ds_ref.abs() + EPS     # without the row-sum term
    return dict(dr=dr, p=p, dp_abs=dp_abs, da=da_ref, s=raw * c.hd ** -0.5, pf=pf.max().item(), ds=ds_ref, ds_bound=ds_bound,
                ds_bound_short=ds_bound_short)


def reg_wgrad_model(m, mul=1.0, rows=None):
    """dW_w, dW_l and their bounds from reg_bwd_model, over all query rows or those of the bool mask rows [B, N]; mul: number of calls"""
    k = 1.0 if rows is None else rows.double()[:, None, :, None]
    u = mul * (2 * U_BF16 + 2 * m['pf'])
    dww = mul * torch.einsum('bgij,bhij->gh', m['dr'] * k, m['p'])
    dww_bound = u * torch.einsum('bgij,bhij->gh', m['dr'].abs() * k, m['p']) + EPS
    dwl = mul * torch.einsum('bgij,bhij->gh', m['da'] * k, m['s'])
    dwl_bound = u * torch.einsum('bgij,bhij->gh', (m['da'].abs() + m['p'] * m['dp_abs']) * k, m['s'].abs()) + EPS
    return dww, dww_bound, dwl, dwl_bound


def bound_reg_bwd(c, label, fwd, twice=False):
    """layer 2 backward -> (failure strings, the dS buffers)"""
    N = c.N
    m = reg_bwd_model(c)
    stats = fwd[3].contiguous()
    dwl, dww = torch.zeros(c.H, c.H, device=DEV), torch.zeros(c.H, c.H, device=DEV)
    qkv = c.qkv()
    dsf, dsb = launch_reg_bwd(c, qkv, stats, dwl, dww)
    if twice:
        launch_reg_bwd(c, qkv, stats, dwl, dww)
    dS = unblock(dsb, c)
    dww_ref, dww_bound, dwl_ref, dwl_bound = reg_wgrad_model(m, 2.0 if twice else 1.0)
    for name, got, ref, bound in (('dS', dS[..., :N], m['ds'], m['ds_bound']), ('dW_w', dww, dww_ref, dww_bound), ('dW_l', dwl, dwl_ref, dwl_bound),
                                  ('dS over the bound without the row-sum term', dS[..., :N], m['ds'], m['ds_bound_short'])):
        _note(f'{label} {name}', got, ref, bound)
    fails = [_bound_fail(dS[..., :N], m['ds'], m['ds_bound'], c.what + ' dS'), _bound_fail(dww, dww_ref, dww_bound, c.what + ' dW_w'),
             _bound_fail(dwl, dwl_ref, dwl_bound, c.what + ' dW_l'), pads_fail(dS, N, c.what + ' dS'),
             guards_fail(dsf, dS.numel(), BF16, c.what + ' dS')]
    return [f for f in fails if f], (dsf, dsb)


def rows_forms_fail(c, fwd, bwd):
    """the _rows forms on one picked row per sample: R, stats and dS bit-equal to the full forms on the rows of that row's 16-query tile,
    everything else (other rows, guards) left as it was; dW_l and dW_w within the full form's bounds with every sum restricted to the
    query rows of the picked tiles -> failure strings"""
    N, Np = c.N, round8(c.N)
    rf, sf, rb, sb = fwd
    dsf, dsb = bwd
    n_pick = torch.tensor([(5 * b + N - 1) % N for b in range(c.B)])
    pick = (torch.arange(c.B) * N + n_pick).to(torch.int32).to(DEV)
    rows = torch.zeros(c.B, N, dtype=torch.bool)
    for b in range(c.B):
        it = int(n_pick[b]) >> 4
        rows[b, 16 * it:16 * it + 16] = True
    rows = rows.to(DEV)
    qkv = c.qkv()
    rf2, sf2, rb2, sb2 = launch_reg_fwd(c, qkv, pick=pick)
    blank_r, blank_s = _nan_buf(tuple(rf.shape), BF16), _nan_buf(tuple(sf.shape), F32)
    rmask = block_scores(rows[:, None, :, None].expand(c.B, c.H, N, Np).contiguous()).reshape(-1)
    smask = rows[:, None, :].expand(c.B, c.H, N).reshape(-1)
    want_r, want_s = blank_r.clone(), blank_s.clone()
    want_r[GUARD:GUARD + rmask.numel()] = torch.where(rmask, rf[GUARD:GUARD + rmask.numel()], blank_r[GUARD:GUARD + rmask.numel()])
    want_s[GUARD:GUARD + smask.numel()] = torch.where(smask, sf[GUARD:GUARD + smask.numel()], blank_s[GUARD:GUARD + smask.numel()])
    fails = [_bits_fail(rf2, want_r, owned_mask(rmask.numel()), c.what + ' R of fwd_rows'),
             _bits_fail(sf2, want_s, owned_mask(smask.numel()), c.what + ' stats of fwd_rows')]
    dwl, dww = torch.zeros(c.H, c.H, device=DEV), torch.zeros(c.H, c.H, device=DEV)
    dsf2, _ = launch_reg_bwd(c, qkv, sb.contiguous(), dwl, dww, pick=pick)
    want_d = blank_r.clone()
    want_d[GUARD:GUARD + rmask.numel()] = torch.where(rmask, dsf[GUARD:GUARD + rmask.numel()], blank_r[GUARD:GUARD + rmask.numel()])
    fails.append(_bits_fail(dsf2, want_d, owned_mask(rmask.numel()), c.what + ' dS of bwd_rows'))
    dww_ref, dww_bound, dwl_ref, dwl_bound = reg_wgrad_model(reg_bwd_model(c), rows=rows)
    _note('register steep dW_w of bwd_rows', dww, dww_ref, dww_bound)
    _note('register steep dW_l of bwd_rows', dwl, dwl_ref, dwl_bound)
    fails += [_bound_fail(dww, dww_ref, dww_bound, c.what + ' dW_w of bwd_rows'), _bound_fail(dwl, dwl_ref, dwl_bound, c.what + ' dW_l of bwd_rows')]
    return [f for f in fails if f]


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfused stage: real-valued operands (the model of test_attention_softmax_stage_under_offsets)
# ---------------------------------------------------------------------------------------------------------------------------------
class StageReal:
    """S = 1.5 randn, W = I + 0.2 randn; s: f32 [B,H,N,Np] with zero pad columns"""

    def __init__(self, B, H, N, mix, causal, seed, Np=None):
        from test_softmax_edges_gpu import _wmat
        self.B, self.H, self.N, self.mix, self.causal, self.Np = B, H, N, mix, causal, Np or round8(N)
        self.kind = mix_kind(H, mix, causal)
        self.what = f'stage real {self.kind} B={B} H={H} N={N} Np={self.Np} causal={int(causal)}'
        g = _gen(seed)
        s = (1.5 * torch.randn((B, H, N, N), generator=g, dtype=torch.float64)).float()
        self.s = pad_rows(s.to(DEV), self.Np)
        self.wl = _wmat(H, seed + 2, 0.2).float().to(DEV) if mix else None
        self.ww = _wmat(H, seed + 3, 0.2).float().to(DEV) if mix else None
        dr = torch.randn((B, H, N, N), generator=g).to(BF16)
        self.dr = pad_rows(dr.to(DEV), self.Np)

    @classmethod
    def from_steep(cls, c, mix, seed):
        """the scaled scores of a RegSteep case as dclip_attn_nt writes them (f32, alpha = hd^-0.5), with the case's own W_l, W_w"""
        self = cls.__new__(cls)
        self.B, self.H, self.N, self.mix, self.causal, self.Np = c.B, c.H, c.N, mix, False, round8(c.N)
        self.kind = mix_kind(c.H, mix, False)
        self.what = f'stage steep {self.kind} B={c.B} H={c.H} N={c.N} hd={c.hd}'
        qkv, D = c.qkv(), c.H * c.hd
        self.s = torch.empty((c.B, c.H, c.N, self.Np), dtype=F32, device=DEV)
        _lib().dclip_attn_nt(qkv.data_ptr(), qkv.stride(0), qkv.data_ptr() + 2 * D, qkv.stride(0), self.s.data_ptr(), 1, c.B, c.H, c.N, self.Np,
                             c.hd, c.hd ** -0.5, _stream())
        self.wl, self.ww = (c.wl, c.ww) if mix else (None, None)
        self.dr = pad_rows(torch.randn((c.B, c.H, c.N, c.N), generator=_gen(seed)).to(BF16).to(DEV), self.Np)
        return self

    def forward_model(self):
        """-> (P, R, |W_w| P, dA bound) in float64: the forward reference of test_attention_softmax_stage_under_offsets"""
        from test_softmax_edges_gpu import _split
        H, N = self.H, self.N
        s64 = self.s[..., :N].double()
        keep = _keep(N, self.causal)
        if self.kind == 'plain':
            a = s64
            da = 4 * EPS * s64.abs().amax(-1, keepdim=True) + 2 ** -16
        elif self.kind == 'valu':
            a = _mix(self.wl.double(), s64)
            da = H * EPS * _mix(self.wl.double().abs(), s64.abs()).amax(-1, keepdim=True) + 2 ** -16
        else:
            (lh, ll), (sh, sl) = _split(self.wl.double().cpu()), _split(s64.cpu())
            lh, ll, sh, sl = (x.to(DEV) for x in (lh, ll, sh, sl))
            a = _mix(lh, sh) + _mix(lh, sl) + _mix(ll, sh)
            da = 3 * H * EPS * _mix(self.wl.double().abs(), s64.abs()).amax(-1, keepdim=True) + 2 ** -12
        am = a.masked_fill(~keep, -math.inf)
        if self.kind == 'mfma':
            ee = torch.exp(am - am.amax(-1, keepdim=True))
            p = ee / ee.to(BF16).double().sum(-1, keepdim=True)
        else:
            p = torch.softmax(am, -1)
        if self.mix:
            return p, _mix(self.ww.double(), p), _mix(self.ww.double().abs(), p), da
        return p, p, p, da


def bound_stage(c, label, s_bf16=False):
    """forward, backward and the weight gradients accumulated over two calls -> failure strings"""
    B, H, N, Np = c.B, c.H, c.N, c.Np
    pref, rref, rabs, da = c.forward_model()
    pf, rf, pb, rb = launch_stage_fwd(c)
    n = B * H * N * Np
    p_bound, r_bound = (U_BF16 + 2 * da) * pref + EPS, (U_BF16 + 2 * da) * rabs + EPS
    _note(f'{label} P', pb[..., :N], pref, p_bound)
    _note(f'{label} R', rb[..., :N], rref, r_bound)
    fails = [_bound_fail(pb[..., :N], pref, p_bound, c.what + ' P'), _bound_fail(rb[..., :N], rref, r_bound, c.what + ' R'),
             pads_fail(pb, N, c.what + ' P'), pads_fail(rb, N, c.what + ' R'), guards_fail(pf, n, BF16, c.what + ' P'),
             guards_fail(rf, n, BF16, c.what + ' R')]
    # backward from the kernel's own bf16 P
    dsf, dsb = guarded(n, BF16)
    dwl = torch.zeros(H, H, device=DEV) if c.mix else None
    dww = torch.zeros(H, H, device=DEV) if c.mix else None
    s_in = c.s.to(BF16).contiguous() if s_bf16 else c.s.contiguous()
    pin, dr = pb.contiguous(), c.dr.contiguous()
    for _ in range(2 if c.mix else 1):
        _lib().dclip_attn_softmax_bwd(dr.data_ptr(), pin.data_ptr(), s_in.data_ptr(), 1 if s_bf16 else 0, c.wl.data_ptr() if c.mix else None,
                                      c.ww.data_ptr() if c.mix else None, dsb.data_ptr(), dwl.data_ptr() if c.mix else None,
                                      dww.data_ptr() if c.mix else None, B, H, N, Np, _stream())
    ds = dsb.view(B, H, N, Np)
    pk, d64 = pb[..., :N].double(), c.dr[..., :N].double()
    s64 = s_in[..., :N].double()
    if c.mix:
        wld, wwd = c.wl.double(), c.ww.double()
        dp, dp_abs = _mixt(wwd, d64), _mixt(wwd.abs(), d64.abs())
    else:
        dp, dp_abs = d64, d64.abs()
    da_ref = pk * (dp - (pk * dp).sum(-1, keepdim=True))
    if c.mix:
        ds_ref = _mixt(wld, da_ref)
        t1, t2 = _mixt(wld.abs(), da_ref.abs()), _mixt(wld.abs(), pk * dp_abs)
        ds_bound = 2 * U_BF16 * (2 * t1 + t2) + U_BF16 * ds_ref.abs() + EPS
    else:
        ds_ref = da_ref
        ds_bound = 2 * U_BF16 * pk * (dp_abs + (pk * dp_abs).sum(-1, keepdim=True)) + U_BF16 * ds_ref.abs() + EPS
    _note(f'{label} dS', ds[..., :N], ds_ref, ds_bound)
    fails += [_bound_fail(ds[..., :N], ds_ref, ds_bound, c.what + ' dS'), pads_fail(ds, N, c.what + ' dS'),
              guards_fail(dsf, n, BF16, c.what + ' dS')]
    if c.mix:
        npos = B * N * N + 1                                                         # terms of one call's f32 sum, and the second call's +=
        dww_ref = 2 * torch.einsum('bgij,bhij->gh', d64, pk)
        dww_bound = 2 * npos * EPS * torch.einsum('bgij,bhij->gh', d64.abs(), pk.abs()) + EPS
        dwl_ref = 2 * torch.einsum('bgij,bhij->gh', da_ref, s64)
        dwl_bound = 2 * (2 * U_BF16 * torch.einsum('bgij,bhij->gh', da_ref.abs() + pk * dp_abs, s64.abs())) + EPS
        _note(f'{label} dW_w', dww, dww_ref, dww_bound)
        _note(f'{label} dW_l', dwl, dwl_ref, dwl_bound)
        fails += [_bound_fail(dww, dww_ref, dww_bound, c.what + ' dW_w (two calls)'), _bound_fail(dwl, dwl_ref, dwl_bound, c.what + ' dW_l (two calls)')]
    return [f for f in fails if f]


def stage_edge_cases():
    """every N of MIX_N for the plain kernel (H and the mask cycling) and for every mixing instance of UNFUSED_MIX (VALU: H in {2, 4, 8, 12}
    with and without the mask, H = 24 causal; MFMA: H = 24), each with its backward twin"""
    for ni, N in enumerate(MIX_N):
        yield StageReal(stage_counts(ni), (1, 3, 16)[ni % 3], N, False, bool(ni & 1), 500 + ni)
        for ki, (H, causal) in enumerate(UNFUSED_MIX):
            yield StageReal(stage_counts(ni + ki), H, N, True, causal, 600 + 20 * ni + ki)


def stage_wide_real_cases():
    for k, (N, Np) in enumerate(WIDE_NP):
        for ki, (H, mix, causal) in enumerate([(3, False, False), (16, False, True), (4, True, False), (12, True, True), (24, True, False)]):
            yield StageReal(stage_counts(k + ki), H, N, mix, causal, 800 + 10 * k + ki, Np=Np)


def _print_worst(prefix):
    for k in sorted(WORST):
        if k.startswith(prefix):
            print(f'worst err / bound, {k}: {WORST[k]:.3f}')


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_plain_softmax_selects_one_key_exactly():
    fails, n = [], 0
    for c in plain_cases(StageSelect):
        n += 1
        fails += exact_stage(c, c.p, c.r)
    assert n == 256
    _report(fails, n)


def test_mixing_softmax_selects_one_key_exactly():
    """VALU mix (H in {2, 4, 8, 12} with and without the mask, H = 24 causal) and MFMA mix (H = 24) at every N of MIX_N"""
    fails, n = [], 0
    for c in mix_cases(StageSelect):
        n += 1
        fails += exact_stage(c, c.p, c.r)
    assert n == len(MIX_N) * len(UNFUSED_MIX)
    _report(fails, n)


def test_softmax_uniform_rows_exact():
    fails, n = [], 0
    for cases in (plain_cases, mix_cases):
        for c in cases(StageUniform):
            n += 1
            fails += exact_stage(c, c.p_bits, c.r_bits)
    assert n == 256 + len(MIX_N) * len(UNFUSED_MIX)
    _report(fails, n)


def test_register_stage_selects_one_key_exactly():
    fails, n, moved = [], 0, 0
    for c in reg_select_cases():
        n += 1
        moved += c.moved
        fails += exact_reg(c)
    assert n == len(MIX_N) * len(REG_INST) + 1 and moved > 0, (n, moved)
    _report(fails, n)


def test_register_stage_uniform_rows():
    fails, n = [], 0
    for ni, N in enumerate(MIX_N):
        for ki, (H, hd) in enumerate(REG_INST):
            if (ni + ki) % 3:
                continue
            c = RegUniform(stage_counts(ni + ki), H, N, hd, (ni + ki) % 4, 20 * N + ki, extra=reg_extra(ni + ki))
            n += 1
            rf, sf, rb, sb = launch_reg_fwd(c, c.qkv())
            R = unblock(rb, c)
            fails += [f for f in (_bound_fail(R[..., :N], c.r, c.bound, c.what + ' R'), _bound_fail(sb, c.lse, c.lse_bound, c.what + ' stats'),
                                  pads_fail(R, N, c.what + ' R'), guards_fail(rf, R.numel(), BF16, c.what + ' R'),
                                  guards_fail(sf, sb.numel(), F32, c.what + ' stats')) if f]
    assert n == 75
    _report(fails, n)


def test_register_stage_steep_rows():
    """forward, backward and the _rows forms on rows that climb along the keys (module docstring, `steep`)"""
    fails, n = [], 0
    for c in reg_steep_cases():
        n += 1
        raw, a2, lse2, p, r, rabs, da = c.model()
        got, moves, alongside = replay_pass1(a2)
        assert (got - lse2).abs().max().item() < 1e-9, (c.what, 'the replay of pass 1 does not reproduce the log-sum-exp')
        assert (moves > 0).double().mean().item() >= 0.75 and alongside > 0, (c.what, moves.tolist(), alongside)
        f, fwd = bound_reg_fwd(c, 'register steep')
        fails += f
        f, bwd = bound_reg_bwd(c, 'register steep', fwd)
        fails += f
        fails += rows_forms_fail(c, fwd, bwd)
    _print_worst('register steep')
    assert n == len(STEEP_SHAPES)
    _report(fails, n)


def test_softmax_stage_steep_rows():
    """the steep cases through dclip_attn_nt -> dclip_attn_softmax_fwd / _bwd: VALU mix (H <= 12), MFMA mix (H = 24, one and two slots) and
    the plain kernel (one and two slots), with the bounds of test_attention_softmax_stage_under_offsets on the f32 scores nt wrote"""
    fails, n, kinds = [], 0, set()
    for k, c in enumerate(reg_steep_cases()):
        for mix in ((True, False) if k < 2 else (True,)):
            sc = StageReal.from_steep(c, mix, 70 + k)
            assert torch.isfinite(sc.s).all() and sc.s[..., :c.N].abs().max().item() > 40 and torch.count_nonzero(sc.s[..., c.N:]) == 0
            n += 1
            kinds.add((sc.kind, sc.Np > 64))
            fails += bound_stage(sc, f'steep stage {sc.kind}')
    _print_worst('steep stage')
    assert n == len(STEEP_SHAPES) + 2 and kinds == {(k, w) for k in ('plain', 'valu', 'mfma') for w in (False, True)}
    _report(fails, n)


def test_register_stage_edges():
    """ordinary operands at every N of MIX_N, every reachable instantiation, weight gradients accumulated over two calls"""
    fails, n = [], 0
    for c in reg_edge_cases():
        n += 1
        f, fwd = bound_reg_fwd(c, 'register edge')
        fails += f
        fails += bound_reg_bwd(c, 'register edge', fwd, twice=True)[0]
    _print_worst('register edge')
    assert n == len(MIX_N) * len(REG_INST) + 1
    _report(fails, n)


def test_softmax_stage_edges():
    fails, n, bf16_done = [], 0, set()
    for c in stage_edge_cases():
        n += 1
        s_bf16 = c.mix and c.N >= 16 and c.kind not in bf16_done                     # scores_bf16 = 1 once per mixing kernel
        if s_bf16:
            bf16_done.add(c.kind)
        fails += bound_stage(c, f'stage {c.kind}' + (' (bf16 scores)' if s_bf16 else ''), s_bf16)
    _print_worst('stage')
    assert n == (1 + len(UNFUSED_MIX)) * len(MIX_N) and bf16_done == {'valu', 'mfma'}
    _report(fails, n)


def test_softmax_stage_wide_np():
    """Np beyond round_up(N, 8): selection, uniform and real-valued cases, forward and backward, every kernel kind"""
    fails, n = [], 0
    for c in wide_cases(StageSelect):
        n += 1
        fails += exact_stage(c, c.p, c.r)
    for c in wide_cases(StageUniform):
        n += 1
        fails += exact_stage(c, c.p_bits, c.r_bits)
    for c in stage_wide_real_cases():
        n += 1
        fails += bound_stage(c, f'wide {c.kind}')
    _print_worst('wide')
    assert n == 3 * 5 * len(WIDE_NP)
    _report(fails, n)


def test_score_entries_refuse_other_np():
    """softmax_fwd / _bwd: Np = 136, Np < N, Np % 8 != 0; mix_fwd / _bwd: any Np but round_up(N, 8).  DCLIP_EINVAL (a ValueError) and
    nothing written"""
    l = _lib()
    B, H, hd = 2, 4, 32
    D = H * hd
    big = B * H * 136 * 136
    out, out32 = _nan_buf((big,), BF16), _nan_buf((big,), F32)
    s = torch.zeros(big, dtype=F32, device=DEV)
    z = torch.zeros(big, dtype=BF16, device=DEV)
    w = torch.eye(H, device=DEV)
    dw = torch.zeros(2, H, H, device=DEV)
    qkv = torch.ones((B * 128, 3 * D), dtype=BF16, device=DEV)
    ws = torch.empty(l.dclip_attn_mix_bwd_workspace_bytes(B, H, 128), dtype=torch.uint8, device=DEV)
    st = _stream()
    for N_, Np_ in ((128, 136), (16, 136), (16, 8), (50, 48), (16, 20)):
        for wl in (None, w.data_ptr()):
            with pytest.raises(ValueError):
                l.dclip_attn_softmax_fwd(s.data_ptr(), wl, wl, out.data_ptr(), out.data_ptr(), B, H, N_, Np_, 0, st)
            with pytest.raises(ValueError):
                l.dclip_attn_softmax_bwd(z.data_ptr(), z.data_ptr(), s.data_ptr(), 0, wl, wl, out.data_ptr(), dw[0].data_ptr() if wl else None,
                                         dw[1].data_ptr() if wl else None, B, H, N_, Np_, st)
    assert l.dclip_attn_mix_supported(H, 16, hd) == 1 and l.dclip_attn_mix_supported(2, 16, 32) == 0
    for H_, N_, Np_ in ((H, 16, 24), (H, 16, 8), (H, 50, 64), (H, 8, 128), (H, 13, 24), (2, 16, 16)):
        with pytest.raises(ValueError):
            l.dclip_attn_mix_fwd(qkv.data_ptr(), 3 * D, w.data_ptr(), w.data_ptr(), out.data_ptr(), out32.data_ptr(), B, H_, N_, Np_, hd, 0.125, st)
        with pytest.raises(ValueError):
            l.dclip_attn_mix_bwd(qkv.data_ptr(), 3 * D, qkv.data_ptr(), 3 * D, w.data_ptr(), w.data_ptr(), s.data_ptr(), out.data_ptr(),
                                 dw[0].data_ptr(), dw[1].data_ptr(), ws.data_ptr(), ws.numel(), B, H_, N_, Np_, hd, 0.125, st)
    torch.cuda.synchronize()
    assert bool((_int_view(out) == -1).all()) and bool((_int_view(out32) == -1).all()) and torch.count_nonzero(dw) == 0
