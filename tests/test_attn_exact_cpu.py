"""The input conditions of tests/test_attn_exact_gpu.py, checked without a GPU and without the library.  Every probe there rests on a
property of its float64 reference alone -- integer sums below 2^23, bf16 ties and real roundings present, a selection gap of 200 in
every row, a masked best key in a third of the causal rows, a bound that a single lost or doubled key breaks -- and the builders assert
them while they build.  The builders draw with a CPU generator, so the numbers here are the numbers of the GPU run."""
import pytest
import torch

import test_attn_exact_gpu as ax


@pytest.mark.parametrize('kind', ['nt', 'nn', 'tn'])
def test_product_cases_are_exact_probes(kind):
    n = ties = roundings = 0
    for c in ax.product_sweep(kind):
        n += 1
        assert c.mag.max().item() < 2 ** 23 and torch.equal(c.ref, c.ref.float().double())
        assert c.ref.numel() < 256 or (c.ties >= 1 and c.roundings >= 1), c.what
        ties, roundings = ties + c.ties, roundings + c.roundings
        a, bm = c.operands()
        if kind != 'nt':
            assert a.shape[-1] == c.Np and torch.count_nonzero(a[..., c.N:]) == 0                 # pad columns of A are zero
            assert torch.equal(a[..., :c.N].double(), c.x)
        assert bm.stride(0) > c.D and bm.stride(0) % 8 == 0 and bm.data_ptr() % 16 == 0
        assert torch.equal(bm.double(), ax._tok(c.b))                                             # bf16 holds the integers
        if c.B * c.H > 1:                                                                         # every problem has its own integers
            flat = c.b.reshape(c.B * c.H, -1)
            assert not (flat[1:] == flat[:1]).all(1).any(), c.what
    assert n == 2 * (128 + len(ax.WIDE_NP)) + 2 and ties > 1000 and roundings > 1000, (n, ties, roundings)


def test_block_scores_follows_the_header_formula():
    a = torch.arange(2 * 3 * 5 * 8, dtype=torch.float32).view(2, 3, 5, 8).to(ax.DEV)
    blk = ax.block_scores(a)
    assert blk.shape == (2, 3, 2, 5, 4)
    for i in range(5):
        for j in range(8):
            assert blk.reshape(2, 3, -1)[1, 2, ((j >> 2) * 5 + i) * 4 + (j & 3)] == a[1, 2, i, j]


def test_rounding_counts_tells_ties_from_roundings():
    y = torch.tensor([256.0, 257.0, 258.0, 513.0, 514.0, 516.0, 128.5, 0.0], dtype=torch.float64)
    assert ax.rounding_counts(y) == (3, 1)                  # ties: 257, 514, 128.5; real rounding: 513


def test_selection_cases_hold_their_conditions():
    n = 0
    for c in ax.selection_cases():                           # (the builder asserts gap, coverage, masked-best share, distinct rows)
        n += 1
        assert c.gap >= 200 and torch.equal(c.q.to(ax.BF16).double(), c.q) and torch.equal(c.k.to(ax.BF16).double(), c.k)
        assert torch.equal(c.expect.to(ax.BF16).double(), c.expect)
    assert n == 2 * 128 * 2 + 2


def test_uniform_cases_are_sensitive_to_one_key():
    n = 0
    for c in ax.uniform_cases():                             # (the builder asserts the single-key sensitivity of every row)
        n += 1
        assert (c.bound > 0).any() and c.q.abs().max().item() == 0
    assert n == 4 * len(ax.EDGE_N)


def test_uniform_sensitivity_check_can_fail():
    """the check itself: values too small for a single key to show (all v equal to 0 but one) are reported"""
    N, hd = 128, 32
    v = torch.zeros(1, 1, N, hd, dtype=torch.float64, device=ax.DEV)
    v[0, 0, 0] = 100
    keep = ax._keep(N, False).double()
    n = keep.sum(-1, keepdim=True)
    tot = keep @ v
    y = tot / n
    assert ax.UniformCase._insensitive(v, tot, y, ax.store_bound(y, 3 * ax.U24 * y.abs(), ax.BF16), keep, n) is not None
