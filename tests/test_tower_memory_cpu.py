"""Host-side half of the tower memory tests (tests/tower_memory_cases.py, tests/test_tower_memory_gpu.py): what the fill patterns read as,
and that the case table reaches every layout the tower runtime distinguishes.  Needs neither the library nor a GPU."""
import numpy as np

import tower_memory_cases as tm


def _as(byte, dtype, n=4):
    return np.full(n * np.dtype(dtype).itemsize, byte, dtype=np.uint8).view(dtype)


def _bf16(byte, n=4):
    """bf16 = the upper half of an f32"""
    half = np.full(2 * n, byte, dtype=np.uint8).view(np.uint16).astype(np.uint32) << 16
    return half.view(np.float32)


def test_fill_patterns_read_as_the_docstrings_say():
    assert tm.FILLS == (0x00, 0xFF, 0x7B) and tm.GUARD_BYTE not in tm.FILLS
    # 0x00: +0 in every format
    for v in (_as(0x00, np.float32), _bf16(0x00), _as(0x00, np.float16)):
        assert (v == 0).all() and not np.signbit(v).any()
    assert (_as(0x00, np.uint8) == 0).all()
    # 0xFF: NaN as f32, bf16 and f16; the largest byte
    for v in (_as(0xFF, np.float32), _bf16(0xFF), _as(0xFF, np.float16)):
        assert np.isnan(v).all()
    assert (_as(0xFF, np.uint8) == 255).all()
    assert (_as(0xFF, np.int32) == -1).all()                     # as an index: out of range below, never a large positive offset
    # 0x7B: about 1.3e36 as f32 and as bf16: finite, and its square is not
    f32, b16, f16 = _as(0x7B, np.float32), _bf16(0x7B), _as(0x7B, np.float16)
    assert np.isfinite(f32).all() and 1.2e36 < f32[0] < 1.4e36
    assert np.isfinite(b16).all() and 1.2e36 < b16[0] < 1.4e36
    with np.errstate(over='ignore'):
        assert np.isinf(f32 * f32).all() and np.isinf(b16 * b16).all()
    # f16: finite and large (0x7B7B = 61 280, the largest finite f16 is 65 504): any product with a value >= 2 saturates
    assert np.isfinite(f16).all() and float(f16[0]) == 61280.0
    with np.errstate(over='ignore'):
        assert np.isinf(f16 * np.float16(2)).all()
    assert (_as(0x7B, np.uint8) == 123).all()
    assert (_as(0x7B, np.int32) == 0x7B7B7B7B).all()             # as an index: far outside any buffer, which is why `pick` is traced by reading


# (kind, AttnPath, last execution pruned, training) as encoder.cpp distinguishes them, written down by hand from layout(), attn_path() and
# the `prune` decision of dclip_encoder_forward; a new branch there makes this list stale:
#   kind 0 (frozen, f16 stream, one shared activation set): inference only, always Fused (<= 128 tokens: dclip_attn_fused_fwd(_rows),
#     above: dclip_attn_stream_fwd)
#   kind 1 with head mixing: Mix in both modes; Unfused in both modes under DCLIP_ATTN_MIX=0
#   kind 1 without head mixing, kind 2 (x0 / G0 / mean0 on the image tower): Unfused in training, Fused in inference
#   pruned or not: any of them (need_rep / a map of the last execution, or DCLIP_PRUNE_LAST=0, un-prune it)
LAYOUTS_DEFAULT = {
    (0, 'Fused', True, False), (0, 'Fused', False, False),
    (1, 'Mix', True, True), (1, 'Mix', False, True), (1, 'Mix', True, False), (1, 'Mix', False, False),
    (1, 'Unfused', True, True), (1, 'Unfused', False, True), (1, 'Fused', True, False), (1, 'Fused', False, False),
    (2, 'Unfused', True, True), (2, 'Unfused', False, True), (2, 'Fused', True, False), (2, 'Fused', False, False),
}
LAYOUTS_ATTN_MIX_OFF = {(1, 'Unfused', True, True), (1, 'Unfused', False, True), (1, 'Unfused', True, False), (1, 'Unfused', False, False)}
LAYOUTS_PRUNE_LAST_OFF = {(1, 'Mix', False, True), (1, 'Mix', False, False)}


def test_case_table_reaches_every_layout_the_runtime_distinguishes():
    assert tm.combos(tm.CASES) == LAYOUTS_DEFAULT
    assert tm.combos(tm.KNOB_CASES, attn_mix=False) == LAYOUTS_ATTN_MIX_OFF
    assert tm.combos(tm.KNOB_CASES, prune_last=False) == LAYOUTS_PRUNE_LAST_OFF
    # the other things layout() branches on: modality, compressed token embedding, ln_pre (CLIP image towers), more than 128 tokens,
    # padded patch rows (in_chans * patch^2 no multiple of 64), weight-shared repeats
    c = tm.CASES
    assert {(v['kind'], v['modality']) for v in c.values()} == {(k, m) for k in (0, 1, 2) for m in (0, 1)}
    assert c['s_txt_rank']['cfg']['compression_embedding'] and 'compression_embedding' not in c['s_txt_mix']['cfg']
    assert c['t_long']['tokens'] > 128 and c['t_long_p14']['tokens'] > 128
    assert (3 * c['t_long_p14']['cfg']['patch'] ** 2) % 64 != 0 and (3 * c['t_long']['cfg']['patch'] ** 2) % 64 == 0
    assert all(c[t]['cfg']['repeated_times'] == 2 for t in ('s_img_mix', 's_txt_mix', 's_txt_rank', 's_img_nomix'))
    assert c['c_txt']['causal'] and c['t_txt']['causal'] and not c['s_txt_mix']['causal']
    for tag, v in c.items():
        if v['modality'] == 0:
            assert v['tokens'] == (v['res'] // (v['cfg'].get('patch') or v['cfg'].get('patch_size'))) ** 2 + 1, tag


def test_every_sequence_runs_at_one_sample_and_on_both_sides_of_a_workgroup():
    for tag in tm.CASES:
        for seq in tm.sequences_of(tag):
            assert seq in tm.SEQUENCES
            bs = tm.batches_of(tag, seq)
            assert 1 in bs and set(bs) == {1, 3, 5}, (tag, seq)
    used = {seq for tag in tm.CASES for seq in tm.sequences_of(tag)}
    assert used == set(tm.SEQUENCES)
    assert 'infer_prefix' in tm.sequences_of('t_txt')
    # map sequences: students of at most 128 tokens only (dclip_attn_maps_fwd); the frozen towers have no backward
    for tag in tm.TEACHERS:
        assert not any(tm.SEQUENCES[s][0] for s in tm.sequences_of(tag)), tag
    for tag in tm.STUDENTS:
        assert 'train_maps' in tm.sequences_of(tag) and tm.CASES[tag]['tokens'] <= 128


def test_every_student_has_pad_columns():
    for tag in tm.STUDENTS:
        assert tm.CASES[tag]['tokens'] % 8 != 0, tag
    assert tm.CASES['t_long']['tokens'] % 8 != 0


def test_chains_change_mode_pruning_maps_and_batch_size_on_one_workspace():
    assert set(tm.CHAIN_CASES) <= set(tm.STUDENTS) and set(tm.KNOB_CASES) <= set(tm.CHAIN_CASES)
    seqs = [s for s, _ in tm.CHAIN]
    assert {'train', 'infer', 'train_full', 'train_maps', 'train_lastout'} == set(seqs)
    bs = [b for _, b in tm.CHAIN]
    assert any(a > b for a, b in zip(bs, bs[1:])) and any(a < b for a, b in zip(bs, bs[1:])) and 1 in bs
    # an unpruned step directly before a pruned one of the same B: a pruned bit or a compact slot left over would show
    assert any(not tm.SEQUENCES[s0][1] and tm.SEQUENCES[s1][1] and b0 == b1 for (s0, b0), (s1, b1) in zip(tm.CHAIN, tm.CHAIN[1:]))
    assert [b for _, b in tm.TEACHER_CHAIN] == [5, 2, 5]
    assert {s for s, _ in tm.TEACHER_CHAIN_TXT} == {'infer', 'infer_prefix'}
