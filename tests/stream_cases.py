"""One case per stream-taking entry of include/dclip.h, for tests/test_stream_contract_cpu.py and tests/test_stream_contract_gpu.py: the
stream contract of the C ABI ("no synchronisation inside any entry point, no allocation, no global mutable state on the compute path").
Not a test module.  Everything here is host-side: the operands are CPU tensors, the device only appears as a dict of addresses.

A case declares its device buffers by role,
  value : float / bf16 / f16 / image-byte data.  The GPU checks withhold them (zeros) until the entry's own stream releases them.
  index : everything a kernel uses as an index, offset, count or descriptor.  Valid from the first moment, so that a launch that ran
          too early, on zeros, still stays inside its buffers (test_stream_contract_cpu.py checks the ranges).
  out   : written by the entry; 0xFF before the call; compared.
  work  : workspace; 0xFF before the call; only its guards are looked at.
its HOST arrays (pointer arrays over those buffers, or numbers together with `other` valid numbers to overwrite them with), and the call
as a function of (addresses, host arrays, stream handle).

Comparison is bit for bit, with two documented exceptions:
  * entries that accumulate with f32 atomics get small-integer operands (Case.int_sum: an upper bound of the sum of magnitudes behind any
    output element, asserted < 2^23 on the CPU), so that every order of additions is exact;
  * sums of f32 atomics whose addends cannot be made integers -- the loss scalars (1 - cos, KL, log-sum-exps per row), dgamma / colsum
    of the LayerNorm backward, dWl / dWw of the unfused softmax backward -- carry `noise` = K and are held to 2 K u (max|want| + 1),
    u = 2^-24.  Two orders of one f32 sum of n addends differ by at most 2 (n - 1) u sum|a_i| to first order, so K is an upper estimate
    of (n - 1) sum|a_i| / (max|want| + 1), from the operands alone:
      loss scalars : n <= 4 B (one addend per row and term, or per wave of a stripe); the addends of a term have one sign (|s - t|,
                     1 - cos, KL and CE rows, hinge and squared differences) or are cosines and log-sum-exps bounded by the result's own
                     size, so sum|a_i| <= 4 (max|want| + 1): K = 16 B;
      dgamma, colsum : n <= M row partials of dy * xhat and of the updated dx, |dy| <= 3 integers, so sum|a_i| <= 12 (max|want| + 1)
                     with room: K = 12 M;
      dWl, dWw     : every (sample, row, key) contributes one product bounded by the result's size: K = B N Np.
    A launch on the wrong stream leaves zeros or NaN (0xFF) there, far outside any of these.
The tower cases' gradients follow tower_memory_cases.grad_failures (Case.grad_rule); their forward outputs are bit-equal.
"""
import ctypes
import math

import numpy as np
import torch

from distillclip_amd._lib import lib

F32, BF16, F16, I32, I64, U8 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8
INT_LIMIT = 2 ** 23


class Buf:
    def __init__(self, name, role, data, noise=None, bound=None):
        self.name, self.role, self.data, self.noise, self.bound = name, role, data.contiguous(), noise, bound

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def bytes(self):
        return self.data.reshape(-1).view(U8)


class HostPtrs:
    """a HOST array of device pointers: entries are None, a buffer name, or (buffer name, byte offset)"""

    def __init__(self, entries):
        self.entries = [e if (e is None or isinstance(e, tuple)) else (e, 0) for e in entries]

    def make(self, ptr):
        return (ctypes.c_void_p * max(len(self.entries), 1))(*[None if e is None else ptr[e[0]] + e[1] for e in self.entries])


class HostNums:
    """a HOST array of numbers, and other valid numbers of the same count to overwrite it with once the call has returned"""

    def __init__(self, ctype, values, other):
        assert len(values) == len(other)
        self.ctype, self.values, self.other = ctype, list(values), list(other)

    def make(self, ptr=None):
        return (self.ctype * len(self.values))(*self.values)


def no_problems():
    return []


class Case:
    def __init__(self, name, entries):
        self.name, self.entries = name, tuple(entries)
        self.bufs, self.host = {}, {}
        self.call = None
        self.deterministic = True          # the entry is documented to give the same bits on every call
        self.int_sum = None                # small-integer operands: bound of the sum of magnitudes behind an output element
        self.index_problems = no_problems  # custom range checks of descriptor-like index operands
        self.grad_rule = None              # (buffer, tower): compared by tower_memory_cases.grad_failures
        self.fired = None                  # towers: the on_bucket callbacks that have fired so far
        self.n_buckets = 0
        self.keep = []                     # host objects the call needs alive

    def _add(self, name, role, data, **kw):
        assert name not in self.bufs
        self.bufs[name] = Buf(name, role, data, **kw)
        return data

    def value(self, name, data, noise=None):
        return self._add(name, 'value', data, noise=noise)

    def index(self, name, data, bound=None):
        """bound = (lo, hi): every element in [lo, hi)"""
        return self._add(name, 'index', data, bound=bound)

    def out(self, name, shape, dtype, noise=None):
        return self._add(name, 'out', torch.zeros(shape, dtype=dtype), noise=noise)

    def work(self, name, nbytes):
        return self._add(name, 'work', torch.zeros(max(int(nbytes), 16), dtype=U8))

    def make_host(self, ptr):
        return {k: h.make(ptr) for k, h in self.host.items()}

    def scramble_host(self, harr, decoy_ptr):
        """overwrite every host array of a call that has returned: pointers -> the decoy of their buffer, numbers -> `other`"""
        for k, h in self.host.items():
            if isinstance(h, HostPtrs):
                for i, e in enumerate(h.entries):
                    if e is not None:
                        harr[k][i] = decoy_ptr[e[0]] + e[1]
            else:
                for i, v in enumerate(h.other):
                    harr[k][i] = v

    def host_pointed(self):
        return sorted({e[0] for h in self.host.values() if isinstance(h, HostPtrs) for e in h.entries if e is not None})


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rnd(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def ints(g, *shape, lo=-3, hi=3, dtype=F32):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def up8(n):
    return (n + 7) // 8 * 8


TABLE = []          # (case name, entries, builder(seed) -> Case)


def case(name, *entries):
    def deco(fn):
        number = len(TABLE) + 1

        def build(seed=0):
            c = Case(name, entries)
            fn(c, _gen(1000 * number + seed))
            assert c.call is not None
            return c
        TABLE.append((name, tuple(entries), build))
        return fn
    return deco


def builders():
    return {name: b for name, _, b in TABLE}


def stream_entries():
    """the stream-taking prototypes of include/dclip.h: those whose last parameter is `void* stream`"""
    import re
    from distillclip_amd import _lib
    protos = _lib._parse_header()
    src = re.sub(r'/\*.*?\*/', '', open(_lib._HEADER).read(), flags=re.S)
    taking = set(re.findall(r'\b(dclip_\w+)\s*\([^;{]*?void\s*\*\s*stream\s*\)\s*;', src))
    assert taking <= set(protos)
    return sorted(taking), protos


# HOST arrays the header documents, by entry (check B covers exactly these)
HOST_ARRAY_ENTRIES = (
    'dclip_cast_transpose_bf16_multi', 'dclip_adamw_multi', 'dclip_adamw_multi_scaled', 'dclip_adamw_multi_amp', 'dclip_adamw_multi_ema',
    'dclip_swap_multi', 'dclip_sumsq_multi', 'dclip_distill_loss', 'dclip_distill_loss_rows', 'dclip_retrieval_metrics',
    'dclip_retrieval_recall', 'dclip_augment_normalize', 'dclip_encoder_prepare', 'dclip_encoder_forward', 'dclip_encoder_backward',
    'dclip_encoder_last_layer_output')


# ---- GEMMs ----------------------------------------------------------------------------------------------------------------------------------
@case('gemm_nt_37x64x64', 'dclip_gemm_nt')
def _(c, g):
    M, N, K = 37, 64, 64
    c.value('A', rnd(g, M, K, dtype=BF16)); c.value('B', rnd(g, N, K, dtype=BF16)); c.out('C', (M, N), BF16)
    c.call = lambda p, h, st: lib().dclip_gemm_nt(p['A'], K, p['B'], K, p['C'], N, M, N, K, 1.0, None, 0, None, None, None, 0, 0, 0, None, None, st)


@case('gemm_nt_200x192x128_bias_residual_colsum', 'dclip_gemm_nt')
def _(c, g):
    M, N, K = 200, 192, 128
    c.value('A', ints(g, M, K, lo=-2, hi=2, dtype=BF16)); c.value('B', ints(g, N, K, lo=-2, hi=2, dtype=BF16))
    c.value('bias', ints(g, N)); c.value('res', ints(g, M, N)); c.value('colsum', ints(g, N)); c.out('C', (M, N), F32)
    c.deterministic, c.int_sum = False, 3 + M * (K * 4 + 3 + 3)
    c.call = lambda p, h, st: lib().dclip_gemm_nt(p['A'], K, p['B'], K, p['C'], N, M, N, K, 1.0, p['bias'], 0, None, None, p['res'], N, 1, 0, None,
                                                  p['colsum'], st)


@case('gemm_tn_acc_splits_atomics', 'dclip_gemm_tn_acc')
def _(c, g):
    M, P, Q = 200, 72, 40
    c.value('A', ints(g, M, P, lo=-2, hi=2, dtype=BF16)); c.value('B', ints(g, M, Q, lo=-2, hi=2, dtype=BF16)); c.value('dW', ints(g, P, Q))
    c.deterministic, c.int_sum = False, 3 + M * 4
    c.call = lambda p, h, st: lib().dclip_gemm_tn_acc(p['A'], P, p['B'], Q, p['dW'], Q, M, P, Q, 3, None, 0, st)


@case('gemm_tn_acc_workspace', 'dclip_gemm_tn_acc')
def _(c, g):
    M, P, Q = 128, 256, 256
    ws = lib().dclip_gemm_tn_workspace_bytes()
    c.value('A', ints(g, M, P, lo=-2, hi=2, dtype=BF16)); c.value('B', ints(g, M, Q, lo=-2, hi=2, dtype=BF16)); c.value('dW', ints(g, P, Q))
    c.work('ws', ws)
    c.int_sum = 3 + M * 4
    c.call = lambda p, h, st: lib().dclip_gemm_tn_acc(p['A'], P, p['B'], Q, p['dW'], Q, M, P, Q, 2, p['ws'], ws, st)


@case('colsum_acc', 'dclip_colsum_acc')
def _(c, g):
    M, N = 37, 72
    c.value('X', ints(g, M, N, dtype=BF16)); c.value('db', ints(g, N))
    c.deterministic, c.int_sum = False, 3 + 3 * M
    c.call = lambda p, h, st: lib().dclip_colsum_acc(p['X'], N, p['db'], M, N, st)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
@case('layernorm_fwd_gather', 'dclip_layernorm_fwd')
def _(c, g):
    R, M, D = 37, 20, 128
    c.value('x', rnd(g, R, D)); c.value('gamma', rnd(g, D)); c.value('beta', rnd(g, D))
    c.index('rows', torch.randint(0, R, (M,), generator=g).to(I32), bound=(0, R))
    c.out('y', (M, D), BF16); c.out('mean', (M,), F32); c.out('rstd', (M,), F32)
    c.call = lambda p, h, st: lib().dclip_layernorm_fwd(p['x'], D, p['rows'], p['gamma'], p['beta'], p['y'], D, 0, p['mean'], p['rstd'], M, D, 1e-5, st)


@case('layernorm_fwd_f16', 'dclip_layernorm_fwd_f16')
def _(c, g):
    M, D = 37, 128
    c.value('x', rnd(g, M, D, dtype=F16)); c.value('gamma', rnd(g, D)); c.value('beta', rnd(g, D))
    c.out('y', (M, D), F16); c.out('mean', (M,), F32); c.out('rstd', (M,), F32)
    c.call = lambda p, h, st: lib().dclip_layernorm_fwd_f16(p['x'], D, None, p['gamma'], p['beta'], p['y'], D, 2, p['mean'], p['rstd'], M, D, 1e-5, st)


@case('layernorm_bwd', 'dclip_layernorm_bwd')
def _(c, g):
    M, D = 37, 128
    x = rnd(g, M, D)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()
    c.value('dy', ints(g, M, D, dtype=BF16)); c.value('x', x); c.value('gamma', rnd(g, D))
    c.value('mean', mean.float()); c.value('rstd', rstd.float())
    c.value('dx', ints(g, M, D)); c.out('dxb', (M, D), BF16)
    # dbeta sums the integer dy: exact in any order.  dgamma sums dy * xhat (|xhat| <= sqrt(D)), colsum the updated dx rows
    c.value('dgamma', ints(g, D), noise=M * 12); c.value('dbeta', ints(g, D)); c.value('colsum', ints(g, D), noise=M * 12)
    c.deterministic = False
    c.call = lambda p, h, st: lib().dclip_layernorm_bwd(p['dy'], D, 0, p['x'], D, None, p['gamma'], p['mean'], p['rstd'], p['dx'], D, p['dxb'], D,
                                                        p['dgamma'], p['dbeta'], p['colsum'], M, D, st)


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
ATTN = dict(a=(3, 4, 17, 32), b=(3, 2, 50, 64))      # B, H, N, hd; the mix kernels need H * hd % 128 == 0


def _scores(g, B, H, N, Np, dtype, scale=1.0):
    s = rnd(g, B, H, N, Np, scale=scale)
    s[..., N:] = 0
    return s.to(dtype)


def _pick(c, g, B, N):
    pk = torch.arange(B) * N + torch.randint(0, N, (B,), generator=g)
    c.index('pick', pk.to(I32))
    prev = c.index_problems
    c.index_problems = lambda: prev() + [f'pick[{b}] = {int(v)} outside sample {b}' for b, v in enumerate(pk) if not b * N <= int(v) < (b + 1) * N]


def _attn_cases(tag):
    B, H, N, hd = ATTN[tag]
    Np, D, M = up8(N), H * hd, B * N
    scale = hd ** -0.5

    @case(f'attn_nt_{tag}', 'dclip_attn_nt')
    def _(c, g):
        c.value('q', rnd(g, M, D, dtype=BF16)); c.value('k', rnd(g, M, D, dtype=BF16)); c.out('S', (B, H, N, Np), F32)
        c.call = lambda p, h, st: lib().dclip_attn_nt(p['q'], D, p['k'], D, p['S'], 1, B, H, N, Np, hd, scale, st)

    @case(f'attn_nn_{tag}', 'dclip_attn_nn')
    def _(c, g):
        c.value('R', _scores(g, B, H, N, Np, BF16)); c.value('v', rnd(g, M, D, dtype=BF16)); c.out('O', (M, D), BF16)
        c.call = lambda p, h, st: lib().dclip_attn_nn(p['R'], p['v'], D, p['O'], D, B, H, N, Np, hd, 1.0, 0, st)

    @case(f'attn_tn_{tag}', 'dclip_attn_tn')
    def _(c, g):
        c.value('R', _scores(g, B, H, N, Np, BF16)); c.value('dO', rnd(g, M, D, dtype=BF16)); c.out('dV', (M, D), BF16)
        c.call = lambda p, h, st: lib().dclip_attn_tn(p['R'], p['dO'], D, p['dV'], D, B, H, N, Np, hd, 1.0, 0, st)

    @case(f'attn_nn_rows_{tag}', 'dclip_attn_nn_rows')
    def _(c, g):
        c.value('R', _scores(g, B, H, N, Np, BF16)); c.value('v', rnd(g, M, D, dtype=BF16)); c.out('O', (M, D), BF16)
        _pick(c, g, B, N)
        c.call = lambda p, h, st: lib().dclip_attn_nn_rows(p['R'], p['v'], D, p['O'], D, B, H, N, Np, hd, 1.0, 0, p['pick'], 1, st)

    @case(f'attn_tn_rows_{tag}', 'dclip_attn_tn_rows')
    def _(c, g):
        c.value('R', _scores(g, B, H, N, Np, BF16)); c.value('dO', rnd(g, M, D, dtype=BF16)); c.out('dV', (M, D), BF16)
        _pick(c, g, B, N)
        c.call = lambda p, h, st: lib().dclip_attn_tn_rows(p['R'], p['dO'], D, p['dV'], D, B, H, N, Np, hd, 1.0, 0, p['pick'], st)

    causal = 1 if tag == 'a' else 0

    @case(f'attn_fused_fwd_{tag}', 'dclip_attn_fused_fwd')
    def _(c, g):
        c.value('qkv', rnd(g, M, 3 * D, dtype=BF16)); c.out('ctx', (M, D), BF16)
        c.call = lambda p, h, st: lib().dclip_attn_fused_fwd(p['qkv'], 3 * D, p['ctx'], D, B, H, N, hd, scale, causal, st)

    @case(f'attn_fused_fwd_rows_{tag}', 'dclip_attn_fused_fwd_rows')
    def _(c, g):
        c.value('qkv', rnd(g, M, 3 * D, dtype=BF16)); c.out('ctx', (M, D), BF16)
        _pick(c, g, B, N)
        c.call = lambda p, h, st: lib().dclip_attn_fused_fwd_rows(p['qkv'], 3 * D, p['ctx'], D, B, H, N, hd, scale, causal, p['pick'], st)

    @case(f'attn_softmax_fwd_{tag}', 'dclip_attn_softmax_fwd')
    def _(c, g):
        c.value('S', _scores(g, B, H, N, Np, F32)); c.value('Wl', rnd(g, H, H)); c.value('Ww', rnd(g, H, H))
        c.out('P', (B, H, N, Np), BF16); c.out('R', (B, H, N, Np), BF16)
        c.call = lambda p, h, st: lib().dclip_attn_softmax_fwd(p['S'], p['Wl'], p['Ww'], p['P'], p['R'], B, H, N, Np, causal, st)

    @case(f'attn_softmax_bwd_{tag}', 'dclip_attn_softmax_bwd')
    def _(c, g):
        P = torch.softmax(_scores(g, B, H, N, Np, F32)[..., :N], -1)
        Pp = torch.zeros(B, H, N, Np); Pp[..., :N] = P
        c.value('dR', _scores(g, B, H, N, Np, BF16)); c.value('P', Pp.to(BF16)); c.value('S', _scores(g, B, H, N, Np, F32))
        c.value('Wl', rnd(g, H, H)); c.value('Ww', rnd(g, H, H)); c.out('dS', (B, H, N, Np), BF16)
        # dWl / dWw: f32 atomics, one addend per (sample, row, wave) at most; every addend is a sum over keys of bounded products
        c.value('dWl', rnd(g, H, H), noise=B * N * Np); c.value('dWw', rnd(g, H, H), noise=B * N * Np)
        c.deterministic = False
        c.call = lambda p, h, st: lib().dclip_attn_softmax_bwd(p['dR'], p['P'], p['S'], 0, p['Wl'], p['Ww'], p['dS'], p['dWl'], p['dWw'], B, H, N, Np, st)

    def mix_fwd_operands(c, g):
        c.value('qkv', rnd(g, M, 3 * D, dtype=BF16, scale=0.5)); c.value('Wl', rnd(g, H, H, scale=0.5)); c.value('Ww', rnd(g, H, H, scale=0.5))

    @case(f'attn_mix_fwd_{tag}', 'dclip_attn_mix_fwd')
    def _(c, g):
        mix_fwd_operands(c, g)
        c.out('R', (B, H, Np // 4, N, 4), BF16); c.out('stats', (B, H, N), F32)
        c.call = lambda p, h, st: lib().dclip_attn_mix_fwd(p['qkv'], 3 * D, p['Wl'], p['Ww'], p['R'], p['stats'], B, H, N, Np, hd, scale, st)

    @case(f'attn_mix_fwd_rows_{tag}', 'dclip_attn_mix_fwd_rows')
    def _(c, g):
        mix_fwd_operands(c, g)
        c.out('R', (B, H, Np // 4, N, 4), BF16); c.out('stats', (B, H, N), F32)
        _pick(c, g, B, N)
        c.call = lambda p, h, st: lib().dclip_attn_mix_fwd_rows(p['qkv'], 3 * D, p['Wl'], p['Ww'], p['R'], p['stats'], B, H, N, Np, hd, scale,
                                                                p['pick'], st)

    def mix_bwd_operands(c, g):
        mix_fwd_operands(c, g)
        c.value('dO', rnd(g, M, D, dtype=BF16)); c.value('stats', 3.0 + rnd(g, B, H, N, scale=0.1))
        c.out('dS', (B, H, Np // 4, N, 4), BF16); c.value('dWl', rnd(g, H, H)); c.value('dWw', rnd(g, H, H))
        ws = lib().dclip_attn_mix_bwd_workspace_bytes(B, H, N)
        c.work('ws', ws)
        return ws

    @case(f'attn_mix_bwd_{tag}', 'dclip_attn_mix_bwd')
    def _(c, g):
        ws = mix_bwd_operands(c, g)
        c.call = lambda p, h, st: lib().dclip_attn_mix_bwd(p['qkv'], 3 * D, p['dO'], D, p['Wl'], p['Ww'], p['stats'], p['dS'], p['dWl'], p['dWw'],
                                                           p['ws'], ws, B, H, N, Np, hd, scale, st)

    @case(f'attn_mix_bwd_rows_{tag}', 'dclip_attn_mix_bwd_rows')
    def _(c, g):
        ws = mix_bwd_operands(c, g)
        _pick(c, g, B, N)
        c.call = lambda p, h, st: lib().dclip_attn_mix_bwd_rows(p['qkv'], 3 * D, p['dO'], D, p['Wl'], p['Ww'], p['stats'], p['dS'], p['dWl'],
                                                                p['dWw'], p['ws'], ws, B, H, N, Np, hd, scale, p['pick'], st)

    @case(f'attn_maps_fwd_{tag}', 'dclip_attn_maps_fwd')
    def _(c, g):
        c.value('qkv', rnd(g, M, 3 * D, dtype=BF16, scale=0.5)); c.value('Wl', rnd(g, H, H, scale=0.5))
        c.out('score', (B, N, N), F32); c.out('prob', (B, N, N), F32)
        c.call = lambda p, h, st: lib().dclip_attn_maps_fwd(p['qkv'], 3 * D, p['Wl'], p['score'], p['prob'], B, H, N, hd, scale, causal, st)

    @case(f'attn_maps_bwd_{tag}', 'dclip_attn_maps_bwd')
    def _(c, g):
        c.value('qkv', rnd(g, M, 3 * D, dtype=BF16, scale=0.5)); c.value('Wl', rnd(g, H, H, scale=0.5))
        c.value('d_score', rnd(g, B, N, N)); c.value('d_prob', rnd(g, B, N, N))
        c.value('dS', _scores(g, B, H, N, Np, BF16)); c.value('dWl', rnd(g, H, H))
        ws = lib().dclip_attn_maps_bwd_workspace_bytes(B, H, N)
        c.work('ws', ws)
        c.call = lambda p, h, st: lib().dclip_attn_maps_bwd(p['qkv'], 3 * D, p['Wl'], p['d_score'], p['d_prob'], p['dS'], 0, p['dWl'], p['ws'], ws,
                                                            B, H, N, Np, hd, scale, causal, st)


_attn_cases('a')
_attn_cases('b')


@case('attn_stream_fwd_N129', 'dclip_attn_stream_fwd')
def _(c, g):
    B, H, N, hd = 2, 2, 129, 64
    D, M = H * hd, B * N
    c.value('qkv', rnd(g, M, 3 * D, dtype=BF16)); c.out('ctx', (M, D), BF16)
    c.call = lambda p, h, st: lib().dclip_attn_stream_fwd(p['qkv'], 3 * D, p['ctx'], D, B, H, N, hd, hd ** -0.5, st)


# ---- embedding-side helpers -----------------------------------------------------------------------------------------------------------------
@case('cast_bf16', 'dclip_cast_bf16')
def _(c, g):
    n = 1028
    c.value('src', rnd(g, n)); c.out('dst', (n,), BF16)
    c.call = lambda p, h, st: lib().dclip_cast_bf16(p['src'], p['dst'], n, st)


@case('cast_f16_f32', 'dclip_cast_f16_f32')
def _(c, g):
    n = 1028
    c.value('src', rnd(g, n, dtype=F16)); c.out('dst', (n,), F32)
    c.call = lambda p, h, st: lib().dclip_cast_f16_f32(p['src'], p['dst'], n, st)


@case('axpy_f32_colsum', 'dclip_axpy_f32')
def _(c, g):
    M, D = 37, 64
    c.value('dst', ints(g, M * D)); c.value('src', ints(g, M * D)); c.out('dstb', (M * D,), BF16); c.value('colsum', ints(g, D))
    c.deterministic, c.int_sum = False, 3 + 3 * M
    c.call = lambda p, h, st: lib().dclip_axpy_f32(p['dst'], p['src'], p['dstb'], M * D, p['colsum'], D, st)


@case('cast_transpose_bf16_multi', 'dclip_cast_transpose_bf16_multi')
def _(c, g):
    shapes = [(40, 72), (64, 128), (72, 40)]
    for i, (r, k) in enumerate(shapes):
        c.value(f'W{i}', rnd(g, r, k))
        if i != 1:                               # job 1 asks for no Wb, job 2 for no Wt (nullable per job)
            c.out(f'Wb{i}', (r, k), BF16)
        if i != 2:
            c.out(f'Wt{i}', (k, r), BF16)
    c.host['W'] = HostPtrs(['W0', 'W1', 'W2']); c.host['Wb'] = HostPtrs(['Wb0', None, 'Wb2']); c.host['Wt'] = HostPtrs(['Wt0', 'Wt1', None])
    c.host['R'] = HostNums(ctypes.c_int64, [s[0] for s in shapes], [s[1] for s in shapes])
    c.host['C'] = HostNums(ctypes.c_int64, [s[1] for s in shapes], [s[0] for s in shapes])
    c.call = lambda p, h, st: lib().dclip_cast_transpose_bf16_multi(h['W'], h['Wb'], h['Wt'], h['R'], h['C'], 3, st)


@case('im2row', 'dclip_im2row')
def _(c, g):
    B, C, res, patch = 2, 3, 32, 8
    G = res // patch
    c.value('img', rnd(g, B, C, res, res)); c.out('rows', (B * (G * G + 1), C * patch * patch), BF16)
    c.call = lambda p, h, st: lib().dclip_im2row(p['img'], p['rows'], B, C, res, patch, 1, st)


@case('im2row_ld_patch14', 'dclip_im2row_ld')
def _(c, g):
    B, C, res, patch, ldk = 2, 3, 28, 14, 640
    G = res // patch
    c.value('img', rnd(g, B, C, res, res)); c.out('rows', (B * (G * G + 1), ldk), BF16)
    c.call = lambda p, h, st: lib().dclip_im2row_ld(p['img'], p['rows'], ldk, B, C, res, patch, 1, st)


@case('token_table', 'dclip_token_table')
def _(c, g):
    n, D = 17, 128
    c.value('pos', rnd(g, n, D)); c.value('cls', rnd(g, D)); c.value('bias', rnd(g, D)); c.out('out', (n, D), F32)
    c.call = lambda p, h, st: lib().dclip_token_table(p['pos'], p['cls'], p['bias'], p['out'], n, D, st)


@case('token_table_bwd', 'dclip_token_table_bwd')
def _(c, g):
    n, D = 17, 128
    c.value('tok', ints(g, n, D)); c.value('dpos', ints(g, n, D)); c.value('dcls', ints(g, D)); c.value('dbias', ints(g, D))
    c.int_sum = 3 + 3 * n
    c.call = lambda p, h, st: lib().dclip_token_table_bwd(p['tok'], p['dpos'], p['dcls'], p['dbias'], n, D, 1, st)


@case('batch_sum_acc', 'dclip_batch_sum_acc')
def _(c, g):
    B, N, D = 3, 17, 128
    c.value('G', ints(g, B, N, D)); c.value('out', ints(g, N, D))
    c.deterministic, c.int_sum = False, 3 + 3 * B
    c.call = lambda p, h, st: lib().dclip_batch_sum_acc(p['G'], p['out'], B, N, D, st)


def _captions(g, B, L, vocab):
    """clip.tokenize layout: SOT (vocab - 2), words, EOT (vocab - 1, the largest id), padding 0"""
    ids = torch.zeros(B, L, dtype=I64)
    for b in range(B):
        n = int(torch.randint(1, L - 2, (1,), generator=g))
        ids[b, 0] = vocab - 2
        ids[b, 1:1 + n] = torch.randint(1, vocab - 2, (n,), generator=g)
        ids[b, 1 + n] = vocab - 1
    return ids


@case('embed_gather', 'dclip_embed_gather')
def _(c, g):
    B, L, N, D, vocab = 3, 13, 11, 64, 97
    c.index('ids', _captions(g, B, L, vocab), bound=(0, vocab)); c.value('table', rnd(g, vocab, D)); c.value('pos', rnd(g, N, D))
    c.out('out', (B * N, D), BF16)
    c.call = lambda p, h, st: lib().dclip_embed_gather(p['ids'], L, p['table'], p['pos'], p['out'], 0, B * N, N, D, st)


@case('embed_scatter_add', 'dclip_embed_scatter_add')
def _(c, g):
    B, L, D, vocab = 3, 13, 64, 97
    rows = B * L
    c.index('ids', _captions(g, B, L, vocab).reshape(-1), bound=(0, vocab)); c.value('dx', ints(g, rows, D)); c.value('dtable', ints(g, vocab, D))
    c.deterministic, c.int_sum = False, 3 + 3 * rows
    c.call = lambda p, h, st: lib().dclip_embed_scatter_add(p['ids'], p['dx'], 1, p['dtable'], rows, D, vocab, st)


@case('pick_index', 'dclip_pick_index')
def _(c, g):
    B, L, vocab = 3, 13, 97
    c.index('ids', _captions(g, B, L, vocab), bound=(0, vocab)); c.out('idx', (B,), I32)
    c.call = lambda p, h, st: lib().dclip_pick_index(p['ids'], L, p['idx'], B, L, st)


# ---- optimizer ------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (4, 8, 252, 1024, 1028, 8192, 12)          # 7 ranges, in elements (multiples of 4)
HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=7)


def _flat_ranges(lengths=LENGTHS, gap=12):
    """[(begin, length)] in elements inside one flat buffer, 16-byte aligned, `gap` untouched elements between neighbours -> ranges, total"""
    out, pos = [], 8
    for n in lengths:
        out.append((pos, n))
        pos += n + gap
    return out, pos + 8


def _streams(c, g, names='pgmv'):
    ranges, total = _flat_ranges()
    for k in names:
        t = rnd(g, total)
        c.value(k, t.abs() if k == 'v' else t)
    for k in names:
        c.host[k] = HostPtrs([(k, 4 * b) for b, _ in ranges])
    c.host['n'] = HostNums(ctypes.c_int64, [n for _, n in ranges], [max(4, n // 8 * 4) for _, n in ranges])
    return ranges, total


@case('adamw', 'dclip_adamw')
def _(c, g):
    n = 1028
    for k in 'pgmv':
        t = rnd(g, n)
        c.value(k, t.abs() if k == 'v' else t)
    H = HYP
    c.call = lambda p, h, st: lib().dclip_adamw(p['p'], p['g'], p['m'], p['v'], n, H['lr'], H['b1'], H['b2'], H['eps'], H['wd'], H['step'], 1, st)


@case('adamw_multi', 'dclip_adamw_multi')
def _(c, g):
    _streams(c, g)
    H = HYP
    c.call = lambda p, h, st: lib().dclip_adamw_multi(h['p'], h['g'], h['m'], h['v'], h['n'], len(LENGTHS), H['lr'], H['b1'], H['b2'], H['eps'],
                                                      H['wd'], H['step'], 1, st)


@case('adamw_multi_scaled', 'dclip_adamw_multi_scaled')
def _(c, g):
    _streams(c, g)
    c.value('gscale', torch.tensor([0.37]))
    H = HYP
    c.call = lambda p, h, st: lib().dclip_adamw_multi_scaled(h['p'], h['g'], h['m'], h['v'], h['n'], len(LENGTHS), H['lr'], H['b1'], H['b2'],
                                                             H['eps'], H['wd'], H['step'], 0, p['gscale'], st)


def _record(skip=0.0):
    H = HYP
    return torch.tensor([1.0 / 1024, skip, 1 - H['b1'] ** H['step'], math.sqrt(1 - H['b2'] ** H['step']), 2.5, 0.4, 0.0, 0.0], dtype=F32)


@case('adamw_multi_amp', 'dclip_adamw_multi_amp')
def _(c, g):
    _streams(c, g)
    c.value('record', _record())
    H = HYP
    c.call = lambda p, h, st: lib().dclip_adamw_multi_amp(h['p'], h['g'], h['m'], h['v'], h['n'], len(LENGTHS), H['lr'], H['b1'], H['b2'], H['eps'],
                                                          H['wd'], 1, p['record'], st)


@case('adamw_multi_ema', 'dclip_adamw_multi_ema')
def _(c, g):
    _streams(c, g, 'pgmve')
    c.value('gscale', torch.tensor([0.37]))
    H = HYP
    w = float(np.float32(1.0 - 0.999))
    c.call = lambda p, h, st: lib().dclip_adamw_multi_ema(h['p'], h['g'], h['m'], h['v'], h['e'], h['n'], len(LENGTHS), H['lr'], H['b1'], H['b2'],
                                                          H['eps'], H['wd'], H['step'], 1, w, p['gscale'], None, st)


@case('swap_multi', 'dclip_swap_multi')
def _(c, g):
    _streams(c, g, 'ab')
    c.call = lambda p, h, st: lib().dclip_swap_multi(h['a'], h['b'], h['n'], len(LENGTHS), st)


@case('sumsq_multi', 'dclip_sumsq_multi')
def _(c, g):
    _streams(c, g, 'g')
    npart = 1024 + 8
    c.out('partials', (npart,), F32)
    c.call = lambda p, h, st: lib().dclip_sumsq_multi(h['g'], h['n'], len(LENGTHS), p['partials'], npart, st)


@case('clip_coef', 'dclip_clip_coef')
def _(c, g):
    c.value('partials', rnd(g, 1024).abs()); c.value('extra', torch.tensor([3.5])); c.out('out', (2,), F32)
    c.call = lambda p, h, st: lib().dclip_clip_coef(p['partials'], 1024, p['extra'], 1.0, p['out'], st)


@case('amp_prepare', 'dclip_amp_prepare')
def _(c, g):
    c.value('found_inf', torch.tensor([0.0])); c.value('scale', torch.tensor([1024.0])); c.value('partials', rnd(g, 1024).abs())
    c.value('skipped', torch.tensor([2], dtype=I64)); c.out('record', (8,), F32)
    H = HYP
    c.call = lambda p, h, st: lib().dclip_amp_prepare(p['found_inf'], p['scale'], p['partials'], 1024, None, 1.0, H['b1'], H['b2'], H['step'],
                                                      p['skipped'], p['record'], st)


def _table(c, g, names='pgmve'):
    ranges, total = _flat_ranges()
    n = len(ranges)
    col = lambda vals, ct: (ct * n)(*vals)
    nbytes = lib().dclip_adamw_table_bytes(n)
    image = torch.zeros(nbytes, dtype=U8)
    tiles = ctypes.c_int64(0)
    lr_scale = [1.0, 0.1, 1.0, 3.0, 0.0, 1.0, 0.5]
    wds = [0.0, 0.01, 0.3, 0.01, 0.0, 0.01, 0.3]
    lib().dclip_adamw_table_fill(col([b for b, _ in ranges], ctypes.c_int64), col([m for _, m in ranges], ctypes.c_int64),
                                 col(lr_scale, ctypes.c_float), col(wds, ctypes.c_float), n, total, image.data_ptr(), nbytes, ctypes.byref(tiles))
    for k in names:
        t = rnd(g, total)
        c.value(k, t.abs() if k == 'v' else t)
    c.index('table', image)

    def problems():
        rec = np.frombuffer(image.numpy().tobytes(), dtype=np.dtype([('tile0', '<i8'), ('begin', '<i8'), ('length', '<i8'), ('s', '<f4'), ('w', '<f4')]))
        bad = [f'range {k}: [{r["begin"]}, {r["begin"] + r["length"]}) outside [0, {total})' for k, r in enumerate(rec[:n])
               if not (0 <= r['begin'] and r['length'] > 0 and r['begin'] + r['length'] <= total)]
        want = 0
        for k, r in enumerate(rec[:n]):
            if r['tile0'] != want:
                bad.append(f'range {k}: tile0 {r["tile0"]}, expected {want}')
            want += (int(r['length']) + 8191) // 8192
        if rec[n]['tile0'] != tiles.value or want != tiles.value:
            bad.append(f'closing record says {rec[n]["tile0"]} tiles, the fill returned {tiles.value}, the ranges need {want}')
        return bad
    c.index_problems = problems
    return n, tiles.value


@case('adamw_table', 'dclip_adamw_table')
def _(c, g):
    n, tiles = _table(c, g)
    c.value('gscale', torch.tensor([0.37]))
    H = HYP
    w = float(np.float32(1.0 - 0.999))
    c.call = lambda p, h, st: lib().dclip_adamw_table(p['p'], p['g'], p['m'], p['v'], p['e'], p['table'], n, tiles, H['lr'], H['b1'], H['b2'], H['eps'],
                                                      H['step'], 1, w, p['gscale'], None, st)


@case('lamb_table', 'dclip_lamb_table')
def _(c, g):
    n, tiles = _table(c, g)
    c.value('record', _record())
    ws = lib().dclip_lamb_workspace_bytes(n, tiles)
    c.work('ws', ws); c.out('stats', (n, 4), F32)
    H = HYP
    w = float(np.float32(1.0 - 0.999))
    c.call = lambda p, h, st: lib().dclip_lamb_table(p['p'], p['g'], p['m'], p['v'], p['e'], p['table'], n, tiles, H['lr'], H['b1'], H['b2'], H['eps'],
                                                     H['step'], 1, w, None, p['record'], 0.5, 1, p['ws'], max(ws, 16), p['stats'], st)


# ---- losses ---------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((8, 64), (37, 64))
CFG = [0.5, 1.0, 0.3, 0.2, 1.0, 0.5, 1.0, 0.25, 0.07, 1.0]         # every term on, tau 0.07, two towers
CFG_OTHER = [1.0, 0.5, 0.0, 0.2, 0.5, 1.0, 0.5, 1.0, 0.5, 1.0]


def _four(c, g, B, E):
    for k in ('s_img', 't_img', 's_txt', 't_txt'):
        c.value(k, rnd(g, B, E))


def _loss_cases(B, E):
    @case(f'distill_loss_B{B}', 'dclip_distill_loss')
    def _(c, g):
        _four(c, g, B, E)
        ws = lib().dclip_distill_loss_workspace(B, E)
        # every scalar is a sum of f32 atomics: one addend per row and term (tower terms) or per wave of a stripe (cross-modal terms)
        c.out('scalars', (16,), F32, noise=16 * B); c.out('d_img', (B, E), F32); c.out('d_txt', (B, E), F32); c.work('ws', ws)
        c.host['cfg'] = HostNums(ctypes.c_float, CFG, CFG_OTHER)
        c.deterministic = False
        c.call = lambda p, h, st: lib().dclip_distill_loss(p['s_img'], p['t_img'], p['s_txt'], p['t_txt'], B, E, h['cfg'], p['scalars'], p['d_img'],
                                                           p['d_txt'], p['ws'], ws, st)

    @case(f'interactive_loss_B{B}', 'dclip_interactive_loss')
    def _(c, g):
        _four(c, g, B, E)
        ws = lib().dclip_interactive_loss_workspace(B, E)
        c.out('out', (4,), F32); c.out('d_img', (B, E), F32); c.out('d_txt', (B, E), F32); c.work('ws', ws)
        c.call = lambda p, h, st: lib().dclip_interactive_loss(p['s_img'], p['t_img'], p['s_txt'], p['t_txt'], B, E, 0.07, 0.5, p['out'], p['d_img'],
                                                               p['d_txt'], p['ws'], ws, st)

    @case(f'relation_kl_B{B}', 'dclip_relation_kl')
    def _(c, g):
        c.value('s', rnd(g, B, E)); c.value('t', rnd(g, B, E))
        ws = lib().dclip_relation_kl_workspace(B, E)
        c.out('out', (4,), F32); c.out('d_s', (B, E), F32); c.work('ws', ws)
        c.call = lambda p, h, st: lib().dclip_relation_kl(p['s'], p['t'], B, E, 0.07, 0.5, p['out'], p['d_s'], p['ws'], ws, st)


for _B, _E in LOSS_SHAPES:
    _loss_cases(_B, _E)


@case('distill_loss_rows', 'dclip_distill_loss_rows')
def _(c, g):
    B, E, row0, rows = 37, 64, 16, 16
    _four(c, g, B, E)
    ws = lib().dclip_distill_loss_workspace(B, E)
    cfg = [0.5, 1.0, 0.3, 0.2, 1.0, 0.0, 0.0, 0.25, 0.07, 1.0]        # no gathered statistics: hard_label and soft_label off
    c.out('scalars', (16,), F32, noise=16 * B); c.out('d_img', (rows, E), F32); c.out('d_txt', (rows, E), F32); c.work('ws', ws)
    c.host['cfg'] = HostNums(ctypes.c_float, cfg, [1.0, 0.5, 0.0, 0.2, 0.5, 0.0, 0.0, 1.0, 0.5, 1.0])
    c.deterministic = False
    c.call = lambda p, h, st: lib().dclip_distill_loss_rows(p['s_img'], p['t_img'], p['s_txt'], p['t_txt'], B, E, row0, rows, h['cfg'], p['scalars'],
                                                            p['d_img'], p['d_txt'], None, None, p['ws'], ws, st)


@case('feature_mse', 'dclip_feature_mse')
def _(c, g):
    n = 1024                                 # a power of two, with coef one too: every addend coef * partial / n is an exact scaling
    c.value('s', ints(g, n)); c.value('t', ints(g, n)); c.value('loss', torch.tensor([2.0])); c.value('ds', ints(g, n))
    c.deterministic, c.int_sum = False, 2 + 36 * n
    c.call = lambda p, h, st: lib().dclip_feature_mse(p['s'], p['t'], n, 0.5, p['loss'], p['ds'], st)


# ---- input pipeline -------------------------------------------------------------------------------------------------------------------------
@case('augment_normalize', 'dclip_augment_normalize')
def _(c, g):
    from distillclip_amd.augment import AUG_OP_DTYPE, op_record
    B, H, W = 4, 32, 48
    plans = [[('TranslateX', 5.0), ('Brightness', 0.3), ('Posterize', 4), ('Equalize', 0.0)],
             [('ShearX', 0.2), ('Contrast', -0.3), ('AutoContrast', 0.0), ('Sharpness', 0.5)],
             [('Rotate', 20.0), ('Identity', 0.0), ('TranslateY', -4.0), ('Equalize', 0.0)],
             [('ShearY', -0.2), ('Sharpness', -0.4), ('Posterize', 6), ('Brightness', -0.2)]]
    rec = np.zeros((B, 4), dtype=AUG_OP_DTYPE)
    for i, ops in enumerate(plans):
        for j, (name, mag) in enumerate(ops):
            rec[i, j] = op_record(name, mag, H, W)
    c.value('images', torch.randint(0, 256, (B, H, W, 3), generator=g).to(U8))
    c.index('ops', torch.from_numpy(rec.view(np.uint8).reshape(B, -1).copy()))
    ws = lib().dclip_augment_workspace(B, H, W)
    c.out('out', (B, 3, H, W), F32); c.out('aug', (B, H, W, 3), U8); c.work('ws', ws)
    c.host['mean'] = HostNums(ctypes.c_float, [0.48, 0.46, 0.41], [0.1, 0.2, 0.3]); c.host['std'] = HostNums(ctypes.c_float, [0.27, 0.26, 0.28], [1.0, 2.0, 3.0])

    def problems():
        # the affine op bounds-checks every source pixel (Pillow's fill), the shift op is not produced by op_record: codes and masks only
        return [f'ops[{i},{j}].op = {rec[i, j]["op"]}' for i in range(B) for j in range(4) if not 0 <= rec[i, j]['op'] <= 8] + \
               [f'ops[{i},{j}] posterize mask {rec[i, j]["c"][0]}' for i in range(B) for j in range(4) if rec[i, j]['op'] == 6 and not 0 <= rec[i, j]['c'][0] <= 255] + \
               [f'ops[{i},{j}] is the integer shift' for i in range(B) for j in range(4) if rec[i, j]['op'] == 2 and
                not (abs(rec[i, j]['c'][0]) < W and abs(rec[i, j]['c'][1]) < H)]
    c.index_problems = problems
    c.call = lambda p, h, st: lib().dclip_augment_normalize(p['images'], B, H, W, p['ops'], 4, h['mean'], h['std'], p['out'], p['aug'], p['ws'], ws, st)


@case('resize_center_crop', 'dclip_resize_center_crop')
def _(c, g):
    from distillclip_amd.augment import RESIZE_DESC_DTYPE, resample_tables
    S, sizes = 16, [(21, 33), (40, 17), (16, 16)]
    desc = np.zeros(len(sizes), dtype=RESIZE_DESC_DTYPE)
    tabs, tpos, spos, wpos, imgs = [], 0, 0, 0, []
    for i, (hh, ww) in enumerate(sizes):
        block, row0, nrows, ksh, ksv = resample_tables(hh, ww, S)
        desc[i] = (spos, tpos, wpos, hh, ww, row0, nrows, ksh, ksv)
        tabs.append(block)
        tpos += block.size
        a = torch.randint(0, 256, (hh * ww * 3,), generator=g).to(U8)
        imgs.append(torch.cat([a, torch.zeros((-a.numel()) % 16, dtype=U8)]))
        spos += imgs[-1].numel()
        wpos += (nrows * S * 3 + 15) // 16 * 16
    tables = np.concatenate(tabs).astype(np.int32)
    c.value('packed', torch.cat(imgs)); c.index('desc', torch.from_numpy(desc.view(np.uint8).copy())); c.index('tables', torch.from_numpy(tables))
    c.out('out', (len(sizes), S, S, 3), U8); c.work('ws', wpos)

    def problems():
        bad = []
        for i, d in enumerate(desc):
            hh, ww, nrows, ksh, ksv, t0 = (int(d[k]) for k in ('height', 'width', 'nrows', 'ksize_h', 'ksize_v', 'table_offset'))
            if not (0 <= d['src_offset'] and d['src_offset'] + hh * ww * 3 <= spos):
                bad.append(f'image {i}: source outside the packed bytes')
            if not (0 <= d['temp_offset'] and d['temp_offset'] + nrows * S * 3 <= max(wpos, 16)):
                bad.append(f'image {i}: scratch outside the workspace')
            if not (0 <= d['row0'] and d['row0'] + nrows <= hh):
                bad.append(f'image {i}: rows [{d["row0"]}, {d["row0"] + nrows}) outside the image')
            need = S * 2 + S * ksh + S * 2 + S * ksv
            if not (0 <= t0 and t0 + need <= tables.size):
                bad.append(f'image {i}: table block outside the tables')
                continue
            hb = tables[t0:t0 + 2 * S].reshape(S, 2)
            vb = tables[t0 + 2 * S + S * ksh:t0 + 4 * S + S * ksh].reshape(S, 2)
            if not ((hb[:, 0] >= 0).all() and (hb[:, 0] + hb[:, 1] <= ww).all() and (hb[:, 1] <= ksh).all()):
                bad.append(f'image {i}: a horizontal window outside the row')
            if not ((vb[:, 0] >= 0).all() and (vb[:, 0] + vb[:, 1] <= nrows).all() and (vb[:, 1] <= ksv).all()):
                bad.append(f'image {i}: a vertical window outside the scratch rows')
        return bad
    c.index_problems = problems
    c.call = lambda p, h, st: lib().dclip_resize_center_crop(p['packed'], p['desc'], p['tables'], len(sizes), S, p['out'], p['ws'], max(wpos, 16), st)


# ---- evaluators -----------------------------------------------------------------------------------------------------------------------------
@case('retrieval_metrics', 'dclip_retrieval_metrics')
def _(c, g):
    n, E = 37, 64
    c.value('img', rnd(g, n, E)); c.value('txt', rnd(g, n, E))
    ws = lib().dclip_retrieval_metrics_workspace(n, E)
    c.out('out', (5,), F32); c.out('rank', (n,), I32); c.work('ws', ws)
    c.host['ks'] = HostNums(ctypes.c_int32, [1, 5, 10], [2, 3, 20])
    c.call = lambda p, h, st: lib().dclip_retrieval_metrics(p['img'], p['txt'], n, E, h['ks'], 3, p['out'], p['rank'], p['ws'], ws, st)


def _offsets(counts):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=I32)


@case('retrieval_recall', 'dclip_retrieval_recall')
def _(c, g):
    counts = [5, 1, 7, 0, 3, 40] * 3
    n_img, n_txt, E = len(counts), sum(counts), 64
    c.value('img', rnd(g, n_img, E)); c.value('txt', rnd(g, n_txt, E)); c.index('offsets', _offsets(counts), bound=(0, n_txt + 1))
    ws = lib().dclip_retrieval_recall_workspace(n_img, n_txt, E)
    c.out('out', (2 * 3 + 2,), F32); c.out('rank_i2t', (n_img,), I32); c.out('rank_t2i', (n_txt,), I32); c.work('ws', ws)
    c.host['ks'] = HostNums(ctypes.c_int32, [1, 5, 10], [2, 3, 20])
    c.call = lambda p, h, st: lib().dclip_retrieval_recall(p['img'], p['txt'], p['offsets'], n_img, n_txt, E, h['ks'], 3, p['out'], p['rank_i2t'],
                                                           p['rank_t2i'], p['ws'], ws, st)


@case('topk_search', 'dclip_topk_search')
def _(c, g):
    nq, ng, E, k = 17, 50, 64, 5
    c.value('q', rnd(g, nq, E)); c.value('gal', rnd(g, ng, E))
    ws = lib().dclip_topk_search_workspace(nq, ng, E, k)
    c.out('idx', (nq, k), I32); c.out('score', (nq, k), F32); c.work('ws', ws)
    c.call = lambda p, h, st: lib().dclip_topk_search(p['q'], p['gal'], nq, ng, E, k, p['idx'], p['score'], p['ws'], ws, st)


@case('group_mean_rows', 'dclip_group_mean_rows')
def _(c, g):
    counts = [5, 1, 0, 7, 37]
    n_rows, E = sum(counts), 64
    c.value('rows', rnd(g, n_rows, E)); c.index('offsets', _offsets(counts), bound=(0, n_rows + 1)); c.out('out', (len(counts), E), F32)
    c.call = lambda p, h, st: lib().dclip_group_mean_rows(p['rows'], p['offsets'], len(counts), n_rows, E, p['out'], st)


@case('clipscore', 'dclip_clipscore')
def _(c, g):
    counts = [2, 0, 5, 1, 3]
    B, K, R, E = len(counts), 2, sum(counts), 64
    c.value('img', rnd(g, B, E)); c.value('cand', rnd(g, B * K, E)); c.value('refs', rnd(g, R, E)); c.index('offsets', _offsets(counts), bound=(0, R + 1))
    for k in ('clip_s', 'ref_s', 'refclip_s'):
        c.out(k, (B * K,), F32)
    c.call = lambda p, h, st: lib().dclip_clipscore(p['img'], E, p['cand'], E, p['refs'], E, p['offsets'], B, K, R, E, 2.5, p['clip_s'], p['ref_s'],
                                                    p['refclip_s'], st)


@case('kendall_tau', 'dclip_kendall_tau')
def _(c, g):
    n, C, ld = 129, 2, 136
    c.value('scores', ints(g, C, ld, lo=0, hi=20)); c.value('human', ints(g, n, lo=1, hi=4))
    ws = lib().dclip_kendall_tau_workspace(n, C)
    c.out('tau', (C, 2), torch.float64); c.out('counts', (C, 8), I64); c.work('ws', ws)
    c.call = lambda p, h, st: lib().dclip_kendall_tau(p['scores'], ld, C, p['human'], n, p['tau'], p['counts'], p['ws'], ws, st)


@case('rank_correlation', 'dclip_rank_correlation')
def _(c, g):
    n, C, ld = 129, 2, 136
    c.value('scores', rnd(g, C, ld)); c.value('human', ints(g, n, lo=1, hi=4))
    ws = lib().dclip_rank_correlation_workspace(n, C)
    c.out('corr', (C, 2), torch.float64); c.out('sums', (C, 4), I64); c.out('ranks', (C + 1, n), I32); c.work('ws', ws)
    c.call = lambda p, h, st: lib().dclip_rank_correlation(p['scores'], ld, C, p['human'], n, p['corr'], p['sums'], p['ranks'], p['ws'], ws, st)


# ---- towers ---------------------------------------------------------------------------------------------------------------------------------
TOWER_B = 3
_TOWERS = {}


def tower_of(tag):
    """the TINY student of tests/test_towers_gpu.py (tower_memory_cases.S_IMG / S_TXT), built on the host: its plan and its parameters"""
    if tag not in _TOWERS:
        import tower_memory_cases as tm
        from distillclip_amd import synth
        from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
        if tag == 'img':
            m = RepeatVisionTransformer(**tm.S_IMG)
            m.load_state_dict(tm._T(synth.student_image_state(11, **tm.S_IMG)))
        else:
            m = RepeatTextTransformer(**tm.S_TXT)
            m.load_state_dict(tm._T(synth.student_text_state(11, **tm.S_TXT)))
        _TOWERS[tag] = m
    return _TOWERS[tag]


def _tower_case(tag):
    entries = ('dclip_encoder_prepare', 'dclip_encoder_forward', 'dclip_encoder_last_layer_output', 'dclip_encoder_backward')

    @case(f'tower_{tag}', *entries)
    def _(c, g):
        from distillclip_amd import synth
        from distillclip_amd.model.component._tower import EncoderRun, AttnMapsDesc, _BUCKET_CB
        import tower_memory_cases as tm
        m = tower_of(tag)
        tw = m._tower
        ps = tw._params()
        offs = tw.param_offsets()
        total = offs[-1]
        flat = torch.zeros(total)
        for p_, off in zip(ps, offs):
            if p_ is not None:
                flat[off:off + p_.numel()] = p_.detach().reshape(-1).float()
        B, N, D, E, nex = TOWER_B, tw.cfg.tokens, tw.cfg.width, tw.cfg.out_dim, tw.cfg.layers * tw.cfg.repeats
        H = tw._handle
        seed = int(torch.randint(0, 1 << 30, (1,), generator=g))
        c.value('params', flat); c.value('grads', torch.zeros(total))
        if tag == 'img':
            c.value('input', torch.from_numpy(synth.images(seed, B, tm.S_IMG['img_size'])).float())
        else:
            vocab = tm.S_TXT['vocab_size']
            c.index('input', torch.from_numpy(synth.captions(seed, B, N, vocab, 3, N - 5)).to(I64), bound=(0, vocab))
        wc, ws = lib().dclip_encoder_wcache_bytes(H), lib().dclip_encoder_workspace_bytes(H, B, 1)
        sc = lib().dclip_encoder_last_layer_output_scratch_bytes(H, B, 1)
        c.out('wcache', (wc,), U8); c.work('ws', ws); c.work('scratch', sc)
        c.out('last_rep', (B, E), F32); c.out('rep0', (B * N, D), F32); c.out('emb', (B * N, D), F32); c.out('score0', (B, N, N), F32)
        c.out('all_tokens', (B * N, E), F32)
        c.value('d_last', rnd(g, B, E)); c.value('d_rep0', rnd(g, B * N, D, scale=0.1)); c.value('d_score0', rnd(g, B, N, N, scale=0.1))
        c.host['params'] = HostPtrs([None if p_ is None else ('params', 4 * off) for p_, off in zip(ps, offs)])
        c.host['grads'] = HostPtrs([None if (p_ is None or not p_.requires_grad) else ('grads', 4 * off) for p_, off in zip(ps, offs)])
        c.host['rep_out'] = HostPtrs(['rep0'] + [None] * (nex - 1))
        c.host['d_rep'] = HostPtrs(['d_rep0'] + [None] * (nex - 1))
        c.host['exec'] = HostNums(ctypes.c_int32, [0], [1])
        c.host['score'] = HostPtrs(['score0']); c.host['d_score'] = HostPtrs(['d_score0'])
        c.grad_rule = ('grads', tw)
        c.deterministic = False
        c.n_buckets = lib().dclip_encoder_num_grad_buckets(H)
        c.fired = []
        run = EncoderRun()
        fired = c.fired
        cb = _BUCKET_CB(lambda user, bucket: fired.append(int(bucket)))
        c.keep = [run, cb]
        is_img = tag == 'img'

        def call(p, h, st):
            vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
            fmaps = AttnMapsDesc(1, vp(h['exec']), vp(h['score']), None, None, None, None, 0)
            bmaps = AttnMapsDesc(1, vp(h['exec']), None, None, vp(h['d_score']), None, None, 0)
            c.keep[2:] = [fmaps, bmaps]
            L = lib()
            L.dclip_encoder_prepare(H, h['params'], p['wcache'], st)
            L.dclip_encoder_forward(H, p['input'], None, B, h['params'], p['wcache'], p['ws'], ws, ctypes.byref(run), 1, p['last_rep'], h['rep_out'],
                                    p['emb'], 0, ctypes.byref(fmaps), st)
            L.dclip_encoder_last_layer_output(H, B, h['params'], p['wcache'], p['ws'], ws, ctypes.byref(run), 1, p['scratch'], p['all_tokens'], st)
            L.dclip_encoder_backward(H, p['input'], None, B, h['params'], h['grads'], p['wcache'], p['ws'], ws, ctypes.byref(run), p['d_last'],
                                     h['d_rep'], None, ctypes.byref(bmaps), vp(cb), None, st)
        c.call = call


_tower_case('img')
_tower_case('txt')
