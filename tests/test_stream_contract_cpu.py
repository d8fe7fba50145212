"""The table of tests/stream_cases.py, checked without a GPU: every stream-taking prototype of include/dclip.h has a case (no exclusions),
and no case can make a kernel leave its buffers, even one that runs too early, on zeroed value operands: every index operand is valid by
itself for the shapes the call passes.  tests/test_stream_contract_gpu.py runs the cases."""
import torch

import stream_cases as sc

# the table's cases by name: a case cannot leave (or join) the table without this list saying so
CASES = """
gemm_nt_37x64x64 gemm_nt_200x192x128_bias_residual_colsum gemm_tn_acc_splits_atomics gemm_tn_acc_workspace colsum_acc
layernorm_fwd_gather layernorm_fwd_f16 layernorm_bwd
attn_nt_a attn_nn_a attn_tn_a attn_nn_rows_a attn_tn_rows_a attn_fused_fwd_a attn_fused_fwd_rows_a attn_softmax_fwd_a attn_softmax_bwd_a
attn_mix_fwd_a attn_mix_fwd_rows_a attn_mix_bwd_a attn_mix_bwd_rows_a attn_maps_fwd_a attn_maps_bwd_a
attn_nt_b attn_nn_b attn_tn_b attn_nn_rows_b attn_tn_rows_b attn_fused_fwd_b attn_fused_fwd_rows_b attn_softmax_fwd_b attn_softmax_bwd_b
attn_mix_fwd_b attn_mix_fwd_rows_b attn_mix_bwd_b attn_mix_bwd_rows_b attn_maps_fwd_b attn_maps_bwd_b attn_stream_fwd_N129
cast_bf16 cast_f16_f32 axpy_f32_colsum cast_transpose_bf16_multi im2row im2row_ld_patch14 token_table token_table_bwd batch_sum_acc
embed_gather embed_scatter_add pick_index
adamw adamw_multi adamw_multi_scaled adamw_multi_amp adamw_multi_ema swap_multi sumsq_multi clip_coef amp_prepare adamw_table lamb_table
distill_loss_B8 interactive_loss_B8 relation_kl_B8 distill_loss_B37 interactive_loss_B37 relation_kl_B37 distill_loss_rows feature_mse
augment_normalize resize_center_crop
retrieval_metrics retrieval_recall topk_search group_mean_rows clipscore kendall_tau rank_correlation
tower_img tower_txt
""".split()


def test_every_stream_taking_prototype_has_a_case():
    taking, protos = sc.stream_entries()
    assert len(taking) >= 63 and len(protos) >= 99            # what the header held when the table was written; it only grows
    covered = {e for _, entries, _ in sc.TABLE for e in entries}
    assert not set(taking) - covered, f'stream-taking entries without a case in tests/stream_cases.py: {sorted(set(taking) - covered)}'
    assert not covered - set(taking), f'cases for entries that take no stream: {sorted(covered - set(taking))}'
    # the last parameter of each is a pointer, as the regular expression of stream_entries() read it
    import ctypes
    assert all(protos[e][1][-1] is ctypes.c_void_p for e in taking)


def test_the_table_is_the_list_above():
    names = [name for name, _, _ in sc.TABLE]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(CASES), (sorted(set(CASES) - set(names)), sorted(set(names) - set(CASES)))


def test_every_entry_with_documented_host_arrays_declares_them():
    taking, _ = sc.stream_entries()
    assert set(sc.HOST_ARRAY_ENTRIES) <= set(taking)
    build = sc.builders()
    for name, entries, _ in sc.TABLE:
        if set(entries) & set(sc.HOST_ARRAY_ENTRIES):
            c = build[name](0)
            assert c.host, name
            for k, h in c.host.items():
                if isinstance(h, sc.HostPtrs):
                    assert all(e is None or (e[0] in c.bufs and 0 <= e[1] < c.bufs[e[0]].nbytes) for e in h.entries), (name, k)
                else:
                    assert h.values != h.other, (name, k)
    covered = {e for name, entries, _ in sc.TABLE for e in entries if build[name](0).host}
    assert set(sc.HOST_ARRAY_ENTRIES) <= covered


def test_index_operands_are_in_range_whatever_the_value_operands_hold():
    """an index operand either has a numeric range, checked here, or a checker of its own (descriptor tables); nothing a kernel uses as an
    index is a value operand or computed from one"""
    for name, _, build in sc.TABLE:
        c = build(0)
        assert c.bufs, name
        for b in c.bufs.values():
            if b.role == 'index':
                assert b.data.dtype in (torch.int32, torch.int64, torch.uint8), (name, b.name)
                if b.bound is not None:
                    lo, hi = b.bound
                    assert lo <= int(b.data.min()) and int(b.data.max()) < hi, (name, b.name, int(b.data.min()), int(b.data.max()), b.bound)
                else:
                    assert c.index_problems is not sc.no_problems and b.data.numel(), (name, b.name)
            elif b.role == 'value':
                assert b.data.dtype in (torch.float32, torch.bfloat16, torch.float16, torch.uint8) or b.data.numel() == 1, (name, b.name)
        assert c.index_problems() == [], (name, c.index_problems())
        # offsets ascend: a CSR table is valid as a whole, not only element by element
        for b in c.bufs.values():
            if b.name == 'offsets':
                assert bool((b.data[1:] >= b.data[:-1]).all()) and int(b.data[0]) == 0, name


def test_order_free_cases_have_integer_operands_within_f32():
    """entries that add with f32 atomics: integer operands whose sums of magnitudes stay below 2^23, so every order of additions is exact"""
    seen = 0
    for name, _, build in sc.TABLE:
        c = build(0)
        if c.int_sum is None:
            assert c.deterministic or any(b.noise for b in c.bufs.values()) or c.grad_rule, f'{name}: not deterministic, no integer operands, no bound'
            continue
        seen += 1
        assert 0 < c.int_sum < sc.INT_LIMIT, (name, c.int_sum)
        for b in c.bufs.values():
            if b.role == 'value':
                x = b.data.double()
                assert bool((x == x.round()).all()) and x.abs().max().item() <= 3, (name, b.name)
    assert seen >= 8


def test_two_seeds_give_two_instances_of_one_layout():
    for name, _, build in sc.TABLE:
        a, b = build(1), build(2)
        assert [(x.name, x.role, x.data.shape, x.data.dtype) for x in a.bufs.values()] == [(x.name, x.role, x.data.shape, x.data.dtype) for x in b.bufs.values()]
        differ = [x.name for x in a.bufs.values() if x.role in ('value', 'index') and x.data.numel() > 8 and not torch.equal(x.data, b.bufs[x.name].data)]
        assert differ, f'{name}: seeds 1 and 2 give the same operands'
