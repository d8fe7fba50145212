"""The input conditions of tests/test_score_exact_gpu.py, checked without a GPU and without the library.  Every probe there rests on
properties of its float64 reference alone -- scores exact in f32 / f16, a selection gap that makes P exactly one-hot, every key selected,
a masked best key in a third of the causal rows, reciprocals whose stored bits do not depend on the last ulp, a bound that a lost or
doubled key breaks, steep rows that move the running reference of the register kernel -- and the builders assert them while they build.
The builders draw with a CPU generator, so the numbers here are the numbers of the GPU run."""
import torch

import test_score_exact_gpu as sx


def _exact(x, dtype):
    return torch.equal(x.to(dtype).double(), x.double())


def test_stage_selection_cases_hold_their_conditions():
    n, kinds = 0, set()
    for cases in (sx.plain_cases, sx.mix_cases, sx.wide_cases):
        for c in cases(sx.StageSelect):                   # (the builder asserts gap, argmax, coverage, masked-best share, exactness)
            n += 1
            kinds.add((c.kind, c.Np > 64))
            assert c.gap >= 199 and _exact(c.r, torch.float32) and c.s.shape[-1] == c.Np and torch.count_nonzero(c.s[..., c.N:]) == 0
            assert (c.p.sum(-1) == 1).all() and ((c.p == 0) | (c.p == 1)).all()
            if c.mix:                                      # W_l is a permutation, A_g = S_pi(g); every row of R sums the weights of its head row
                assert (c.wl.sum(0) == 1).all() and (c.wl.sum(1) == 1).all()
                assert torch.allclose(c.r.sum(-1), c.ww.double().sum(1)[None, :, None].expand(c.B, c.H, c.N), atol=0, rtol=0)
    assert n == 256 + len(sx.MIX_N) * len(sx.UNFUSED_MIX) + 5 * len(sx.WIDE_NP)
    assert kinds == {(k, w) for k in ('plain', 'valu', 'mfma') for w in (False, True)}          # every kernel kind with one and two slots


def test_stage_uniform_cases_and_stable_reciprocals():
    assert sx.unstable_reciprocals(128) == ()             # none dropped
    n = 0
    for cases in (sx.plain_cases, sx.mix_cases, sx.wide_cases):
        for c in cases(sx.StageUniform):
            n += 1
            row = c.s[..., :c.N]
            assert (row == row[..., :1]).all() and row.abs().max().item() <= 300
            want = (1.0 / c.n).expand(c.N, c.N).masked_fill(~sx._keep(c.N, c.causal), 0.0)
            assert ((c.p_bits[0, 0].double() - want).abs() <= sx.U_BF16 * want).all()             # one rounding to bf16
            assert ((c.r_bits[0, 0].double() - want).abs() <= sx.U_BF16 * want).all()
    assert n == 256 + len(sx.MIX_N) * len(sx.UNFUSED_MIX) + 5 * len(sx.WIDE_NP)


def test_reciprocal_stability_check_can_fail():
    """the check itself: bf16(x) of the three f32 values around a bf16 rounding boundary differs"""
    r = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float32)               # the tie between bf16 1.0 and 1.0078125
    lo, hi = torch.nextafter(r, torch.zeros(1)), torch.nextafter(r, torch.full((1,), 2.0))
    assert sx._hi_lo_sum(lo)[0].item() != sx._hi_lo_sum(hi)[0].item()


def test_register_selection_cases_hold_their_conditions():
    n, inst, extras = 0, set(), set()
    for c in sx.reg_select_cases():                        # (the builder asserts f16 exactness, gap >= 500, one-hot model, argmax, moves)
        n += 1
        inst.add((c.H, c.hd, c.N % 4, ((c.N + 3) // 4) & 1))
        extras.add(c.extra)
        assert c.gap >= 500 and _exact(c.q, sx.BF16) and _exact(c.k, sx.BF16) and _exact(c.r, torch.float32)
        assert c.N <= 4 or c.moved > 0
        buf = c.qkv()
        assert buf.stride(0) == 3 * c.H * c.hd + c.extra and (c.extra == 0 or (buf[:, 3 * c.H * c.hd:] == sx.FILL).all())
    assert n == len(sx.MIX_N) * len(sx.REG_INST) + 1 and extras == {0, 8, 64}
    for H, hd in sx.REG_INST:                              # every instantiation meets every residue of N mod 4 and both parities of nq
        mine = [(r, par) for h_, d_, r, par in inst if (h_, d_) == (H, hd)]
        assert {r for r, _ in mine} == {0, 1, 2, 3} and {par for _, par in mine} == {0, 1}, (H, hd)
    B, H, N, hd = sx.MULTI_ROUND
    assert B * ((N + 15) // 16) / 4 > 256


def test_register_uniform_cases_are_sensitive_to_one_key():
    for N in range(1, 129):                                # every n <= 128 (the builder asserts 1 / (n +- 1) outside the bound)
        c = sx.RegUniform(1, 4, N, 32, 0, N)
        assert c.q.abs().max().item() == 0 and c.bound.max().item() < 1.0 / (N * (N + 1))


def test_steep_cases_move_the_running_reference():
    n = 0
    for c in sx.reg_steep_cases():                         # (the builder asserts raw exact in f16, |raw| < 512)
        n += 1
        raw, a2, lse2, p, r, rabs, da = c.model()
        got, moves, alongside = sx.replay_pass1(a2)
        assert (got - lse2).abs().max().item() < 1e-9
        assert (moves > 0).double().mean().item() >= 0.75 and alongside > 0, (c.what, moves.tolist(), alongside)
        assert c.k[..., 0].abs().max().item() <= 280 and a2.abs().max().item() > 70
        buf = c.qkv()                                      # (asserts that bf16 holds every operand)
        assert buf.stride(0) == 3 * c.H * c.hd + c.extra
    assert n == len(sx.STEEP_SHAPES)


def test_ordinary_inputs_never_move_the_reference():
    """what the steep rows add: on the ordinary operands of the edge cases the replay sees no move at all"""
    moved = 0
    for c in sx.reg_edge_cases():
        moved += int(sx.replay_pass1(c.model()[1])[1].sum())
        c.qkv()
    assert moved == 0


def _n_classes(ns):
    """(residues of N mod 4, parities of the quad count nq, sides of the 64-key slot edge) met by the values ns"""
    return {n % 4 for n in ns}, {((n + 3) // 4) & 1 for n in ns}, {sx.round8(n) > 64 for n in ns}


def test_edge_case_counts_and_kernel_kinds():
    stage = list(sx.stage_edge_cases())
    assert len(stage) == (1 + len(sx.UNFUSED_MIX)) * len(sx.MIX_N)
    assert {(c.kind, c.Np > 64) for c in stage} == {(k, w) for k in ('plain', 'valu', 'mfma') for w in (False, True)}
    for H, causal in sx.UNFUSED_MIX:                       # every mixing instance (forward and backward template) meets every N of the list
        assert sorted(c.N for c in stage if c.mix and (c.H, c.causal) == (H, causal)) == sx.MIX_N, (H, causal)
    assert sorted(c.N for c in stage if not c.mix) == sx.MIX_N
    for causal in (False, True):                           # the plain kernel: both slot counts with and without the mask
        assert {c.Np > 64 for c in stage if not c.mix and c.causal == causal} == {False, True}
    wide = list(sx.stage_wide_real_cases())
    assert len(wide) == 5 * len(sx.WIDE_NP) and all(c.Np > sx.round8(c.N) and torch.count_nonzero(c.dr[..., c.N:]) == 0 for c in wide)
    reg = list(sx.reg_edge_cases())
    assert len(reg) == len(sx.MIX_N) * len(sx.REG_INST) + 1
    for H, hd in sx.REG_INST:                              # every instantiation meets every N: every residue mod 4, both parities of nq
        ns = sorted(c.N for c in reg if (c.H, c.hd) == (H, hd) and c.B <= 3)
        assert ns == sx.MIX_N and _n_classes(ns) == ({0, 1, 2, 3}, {0, 1}, {False, True}), (H, hd)
    assert [(c.B, c.H, c.N, c.hd) for c in reg if c.B > 3] == [sx.MULTI_ROUND]


def test_guard_layout_and_block_scores_agree_with_unblock_scores():
    from distillclip_amd import ops
    c = sx.RegSelect(2, 4, 13, 32, 1, 5)
    Np = sx.round8(c.N)
    blk = sx.block_scores(sx.pad_rows(c.r, Np))
    assert torch.equal(ops.unblock_scores(blk), sx.pad_rows(c.r, Np))
    want = sx.want_buf(blk, sx.BF16)
    n = blk.numel()
    assert want.numel() == n + 2 * sx.GUARD and (sx._int_view(want[:sx.GUARD]) == -1).all() and (sx._int_view(want[sx.GUARD + n:]) == -1).all()
    assert torch.equal(sx.unblock(want[sx.GUARD:sx.GUARD + n], c).double(), sx.pad_rows(c.r, Np))
    flat, block = sx.guarded(n, sx.BF16)
    assert sx.guards_fail(flat, n, sx.BF16, 'x') is None
    flat[3] = 0
    assert sx.guards_fail(flat, n, sx.BF16, 'x') is not None
