"""Row-tile forms of the attention kernels (include/dclip.h: dclip_attn_*_rows), which a pruned last block execution runs: each forms
only the 16-row tile that holds row pick[b] of every sample, by the instructions and operands of its full form.

Against the full kernels, at B = 3 (not a multiple of the 4 waves of a workgroup) on both shipped student shapes, with the picks in
tile 0, in the ragged last tile (N = 50: 2 valid rows, N = 77: 13) and different per sample:
  mix_fwd_rows -> nn_rows, fused_fwd_rows   ctx (and R, stats) on the picked tiles' rows bit-equal; every other row untouched
  tn_rows, nn_rows(fill_zero)               the whole output bit-equal to the full kernel fed operands zeroed outside the tiles
  mix_bwd_rows                              dS on the tiles bit-equal with dO zero outside the picked rows; dW_l / dW_w within rel-L2 1e-3
                                            (per-workgroup partials summed in another order); dQ, dK, dV of the row-tile chain bit-equal
Everything a row-tile form must not read -- the rows of R, stats, dS and of the backward's workspace (delta) outside the tiles -- is
NaN beforehand in every test, so reading any of it shows up as a non-finite or changed output."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
SHAPES = {'img': (24, 32, 50), 'txt': (12, 64, 77)}                 # H, hd, N
BF16 = torch.bfloat16


def _picks(N, kind):
    """token index of the picked row of each of the B samples"""
    last = N - 1
    return {'tile0': [0, 3, 15], 'ragged': [last, last - 1, last], 'mixed': [5, 16 + N % 16, last]}[kind]


CASES = [(s, k) for s in SHAPES for k in ('tile0', 'ragged', 'mixed')]


def _randn(shape, seed, std=1.0, dtype=torch.float32):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return (torch.randn(shape, generator=g, device='cuda') * std).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _block(a):
    """row-major [B,H,N,Np] -> quad-blocked [B,H,Np/4,N,4]"""
    b, h, n, npad = a.shape
    return a.reshape(b, h, n, npad // 4, 4).permute(0, 1, 3, 2, 4).contiguous()


class Case:
    """one shape and pick set: the operands, the tile masks and the full kernels' results (computed once, never written again)"""

    def __init__(self, shape, kind):
        from distillclip_amd import ops
        H, hd, N = SHAPES[shape]
        self.H, self.hd, self.N, self.D, self.Np = H, hd, N, H * hd, (N + 7) // 8 * 8
        D = self.D
        n = _picks(N, kind)
        assert {'tile0': all(v < 16 for v in n), 'ragged': all(v >> 4 == (N - 1) >> 4 for v in n), 'mixed': len({v >> 4 for v in n}) == 3}[kind]
        self.pick = torch.tensor([b * N + v for b, v in enumerate(n)], dtype=torch.int32, device='cuda')
        tile = torch.tensor([v >> 4 for v in n], device='cuda')
        self.in_tile = (torch.arange(N, device='cuda')[None, :] >> 4) == tile[:, None]              # [B, N]
        self.rows = self.in_tile.reshape(-1)                                                         # [B * N] token-major rows
        self.picked = torch.zeros(B * N, dtype=torch.bool, device='cuda')
        self.picked[self.pick.long()] = True
        self.scale = hd ** -0.5
        self.qkv = _randn((B * N, 3 * D), 51, 0.7, BF16)
        self.wl = torch.eye(H, device='cuda') + _randn((H, H), 52, 0.15)
        self.ww = torch.eye(H, device='cuda') + _randn((H, H), 53, 0.15)
        # dO of a pruned execution: zero outside the picked rows
        self.d_ctx = torch.where(self.picked[:, None], _randn((B * N, D), 54, 1.0, BF16), torch.zeros((), dtype=BF16, device='cuda'))
        # full forward and backward
        self.R, self.stats = ops.attn_mix_fwd(self.qkv, B, N, H, hd, self.wl, self.ww, self.scale)
        self.ctx = torch.zeros(B * N, D, dtype=BF16, device='cuda')
        ops.attn_nn(self.R, self.qkv[:, 2 * D:], 3 * D, self.ctx, D, hd)
        self.dwl, self.dww = torch.zeros(H, H, device='cuda'), torch.zeros(H, H, device='cuda')
        self.dS = ops.attn_mix_bwd(self.qkv, self.d_ctx, B, N, H, hd, self.wl, self.ww, self.stats, self.scale, self.dwl, self.dww)
        self.dqkv = torch.zeros(B * N, 3 * D, dtype=BF16, device='cuda')
        ops.attn_tn(self.R, self.d_ctx, D, self.dqkv[:, 2 * D:], 3 * D, hd)
        ops.attn_nn(self.dS, self.qkv[:, D:], 3 * D, self.dqkv, 3 * D, hd, self.scale)
        ops.attn_tn(self.dS, self.qkv, 3 * D, self.dqkv[:, D:], 3 * D, hd, self.scale)
        torch.cuda.synchronize()

    def poison_blocked(self, a):
        """copy of a quad-blocked [B,H,Np/4,N,4] tensor with every row outside the tiles NaN"""
        return torch.where(self.in_tile[:, None, None, :, None], a, torch.full((), float('nan'), dtype=a.dtype, device='cuda'))

    def poison_stats(self, s):
        return torch.where(self.in_tile[:, None, :], s, torch.full((), float('nan'), device='cuda'))

    def tile_blocked(self, a):
        return a[self.in_tile[:, None, None, :, None].expand_as(a)]

    def nan_workspace(self):
        from distillclip_amd._lib import lib
        return torch.full((lib().dclip_attn_mix_bwd_workspace_bytes(B, self.H, self.N),), 0xFF, dtype=torch.uint8, device='cuda')


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return Case(shape, kind)


SENTINEL = 7.0


@pytest.mark.parametrize('shape,kind', CASES)
def test_mix_forward_rows_match_the_full_kernels_on_the_picked_tiles(shape, kind):
    from distillclip_amd import ops
    c = _case(shape, kind)
    R = torch.full_like(c.R, float('nan'))
    stats = torch.full_like(c.stats, float('nan'))
    ops.attn_mix_fwd_rows(c.qkv, R, stats, c.wl, c.ww, c.scale, c.pick)
    assert _same(c.tile_blocked(R), c.tile_blocked(c.R))
    assert _same(stats[c.in_tile[:, None, :].expand_as(stats)], c.stats[c.in_tile[:, None, :].expand_as(stats)])
    assert torch.isnan(R[~c.in_tile[:, None, None, :, None].expand_as(R)]).all()                    # rows outside the tiles: not written
    ctx = torch.full((B * c.N, c.D), SENTINEL, dtype=BF16, device='cuda')
    ops.attn_nn_rows(R, c.qkv[:, 2 * c.D:], 3 * c.D, ctx, c.D, c.hd, c.pick)                        # R still NaN outside the tiles
    assert torch.isfinite(ctx).all()
    assert _same(ctx[c.rows], c.ctx[c.rows])
    assert (ctx[~c.rows] == SENTINEL).all()


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('shape,kind', CASES)
def test_fused_forward_rows_match_the_full_kernel_on_the_picked_tiles(shape, kind, causal):
    from distillclip_amd import ops
    c = _case(shape, kind)
    full = ops.attn_fused_fwd(c.qkv, B, c.N, c.H, c.hd, causal)
    ctx = torch.full((B * c.N, c.D), SENTINEL, dtype=BF16, device='cuda')
    ops.attn_fused_fwd_rows(c.qkv, ctx, B, c.N, c.H, c.hd, c.pick, causal)
    assert torch.isfinite(ctx).all()
    assert _same(ctx[c.rows], full[c.rows])
    assert (ctx[~c.rows] == SENTINEL).all()


@pytest.mark.parametrize('blocked', [True, False])
@pytest.mark.parametrize('shape,kind', CASES)
def test_product_rows_match_the_full_kernels_on_operands_zeroed_outside_the_tiles(shape, kind, blocked):
    """tn_rows and nn_rows(fill_zero) on NaN outside the tiles (A, and for tn the token-major operand as well) against attn_tn / attn_nn
    on zeros there: the whole output, bit for bit, for both layouts of A"""
    from distillclip_amd import ops
    c = _case(shape, kind)
    N, Np, D, hd = c.N, c.Np, c.D, c.hd
    a = _randn((B, c.H, N, Np), 61, 0.3, BF16)
    a[..., N:] = 0                                                                                  # pad columns are zero
    keep = c.in_tile[:, None, :, None]
    nan, zero = torch.full((), float('nan'), dtype=BF16, device='cuda'), torch.zeros((), dtype=BF16, device='cuda')
    lay = _block if blocked else (lambda t: t.contiguous())
    a_nan, a_zero = lay(torch.where(keep, a, nan)), lay(torch.where(keep, a, zero))
    bm = c.qkv[:, :D].contiguous()
    bm_nan, bm_zero = torch.where(c.rows[:, None], bm, nan), torch.where(c.rows[:, None], bm, zero)
    want, got = (torch.full((B * N, D), SENTINEL, dtype=BF16, device='cuda') for _ in range(2))
    ops.attn_tn(a_zero, bm_zero, D, want, D, hd, c.scale)
    ops.attn_tn_rows(a_nan, bm_nan, D, got, D, hd, c.pick, c.scale)
    assert torch.isfinite(got).all() and _same(got, want)
    want, got = (torch.full((B * N, D), SENTINEL, dtype=BF16, device='cuda') for _ in range(2))
    ops.attn_nn(a_zero, bm, D, want, D, hd, c.scale)
    ops.attn_nn_rows(a_nan, bm, D, got, D, hd, c.pick, c.scale, fill_zero=True)
    assert torch.isfinite(got).all() and _same(got, want)
    assert torch.count_nonzero(got[~c.rows]) == 0 and torch.count_nonzero(got[c.rows]) > 0


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize('shape,kind', CASES)
def test_mix_backward_rows_match_the_full_backward(shape, kind):
    """dS on the tiles bit-equal; dW_l, dW_w rel-L2 <= 1e-3 (the bound tests/test_prune_last_exec_gpu.py holds gradients to); then the
    chain a pruned execution runs (tn_rows, mix_bwd_rows, nn_rows(fill_zero), tn_rows on the row-tile forward's R and stats): dQ, dK, dV
    bit-equal to the full chain's"""
    from distillclip_amd import ops
    c = _case(shape, kind)
    D, hd = c.D, c.hd
    R, stats = c.poison_blocked(c.R), c.poison_stats(c.stats)
    dS = torch.full_like(c.dS, float('nan'))
    dwl, dww = torch.zeros_like(c.dwl), torch.zeros_like(c.dww)
    ops.attn_mix_bwd_rows(c.qkv, c.d_ctx, dS, c.wl, c.ww, stats, c.scale, dwl, dww, c.pick, ws=c.nan_workspace())
    assert _same(c.tile_blocked(dS), c.tile_blocked(c.dS))
    assert torch.isnan(dS[~c.in_tile[:, None, None, :, None].expand_as(dS)]).all()
    assert torch.isfinite(dwl).all() and torch.isfinite(dww).all()
    el, ew = _rel_l2(dwl, c.dwl), _rel_l2(dww, c.dww)
    print(f'\n{shape} {kind}: dW_l rel-L2 {el:.3e}, dW_w rel-L2 {ew:.3e}')
    assert el <= 1e-3 and ew <= 1e-3, (el, ew)
    dqkv = torch.full((B * c.N, 3 * D), SENTINEL, dtype=BF16, device='cuda')
    ops.attn_tn_rows(R, c.d_ctx, D, dqkv[:, 2 * D:], 3 * D, hd, c.pick)
    ops.attn_nn_rows(dS, c.qkv[:, D:], 3 * D, dqkv, 3 * D, hd, c.pick, c.scale, fill_zero=True)
    ops.attn_tn_rows(dS, c.qkv, 3 * D, dqkv[:, D:], 3 * D, hd, c.pick, c.scale)
    assert torch.isfinite(dqkv).all()
    assert _same(dqkv, c.dqkv)
