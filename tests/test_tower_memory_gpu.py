"""The tower runtime's memory contract (csrc/encoder.cpp: layout(), dclip_encoder_forward / _backward / _last_layer_output), through
HipTower.forward / .backward / .last_layer_output with every caller-owned device buffer placed by the test (tests/tower_memory_cases.py):

  guards : workspace, weight cache, last_layer_output scratch, maps scratch, flat_grad and every output are exactly as large as their size
           query says and lie between 64 KiB of 0xA5 on each side; no guard byte changes, and the const operands stay bit for bit.
  poison : the workspace, the scratch buffers, the weight cache (before prepare()) and the outputs are filled with 0x00, 0xFF (NaN in every
           float format) or 0x7B (1.3e36; large and finite in f16) before a run.  Forward results are bit-equal across the fills; gradients
           follow the rule below.  A second backward on one forward, with another d_out, clears its own seeds.
  reuse  : one workspace (0xFF before the first step, never refilled) and one record through a chain of training / inference, pruned /
           full, maps / no maps and larger / smaller B; every step equals the same step alone on a zero-filled workspace of its own.

Gradient rule (tower_memory_cases.grad_failures): per flat range of grad_buckets(), finite wherever the 0x00 run is and within
2e-5 * max|want| of it (order noise of the f32 atomics in the LayerNorm, bias and table sums: the bound test_towers_gpu.py holds the same
comparison to).  Every weight gradient that is one dclip_gemm_tn_acc launch (tower_memory_cases.GEMM_WGRADS) and that two 0x00 runs
reproduce bit for bit is held bit-equal.  How many ranges two 0x00 runs reproduce as a whole is printed; tower_memory_cases.grad_classes says
why whole ranges are not held bit-equal on that evidence.

Integer and pointer-like regions of the workspace, traced by reading encoder.cpp before any poisoned run.  There is one: Work::pick, int32
[B], the row index b * N + (class token: 0; text: argmax of the ids) of each sample's picked row.  dclip_pick_index writes all B entries in
every dclip_encoder_forward, after the embedding and before the first block execution; it reads the caller's ids, nothing of the workspace.
  infer, infer_prefix : dclip_pick_index, then the readers of the pruned last execution: dclip_attn_fused_fwd_rows (frozen and unmixed
                        towers of at most 128 tokens) or dclip_attn_mix_fwd_rows + dclip_attn_nn_rows (Mix), the two dclip_rows_pick.
                        dclip_encoder_last_layer_output reads no pick: its LayerNorm runs on all rows (ridx = null), the re-run of a pruned
                        execution is un-pruned (pick = null).
  infer_full          : dclip_pick_index, then the final LayerNorm's row index (ln_stream, ridx = pick).
  train, train_lastout: forward as `infer` (Unfused: dclip_attn_nn_rows after the all-row score stage).  The backward reads the pick of that
                        forward: same workspace, same B, training layout in both, so the same offset, and nothing between them writes the
                        workspace (last_layer_output writes its scratch only): dclip_rows_expand twice, dclip_attn_tn_rows,
                        dclip_attn_mix_bwd_rows, dclip_attn_nn_rows.  A repeated backward reads the same entries again.
  train_full,         : forward as `infer_full`; the backward's first LayerNorm backward gathers by pick (un-pruned record).
  train_maps
  reuse chain         : every step starts with a forward, which rewrites pick at the offset of its own (B, mode) before any reader; the
                        wrapper refuses a backward whose B is not the last training forward's.
(Above 128 tokens the pruned execution's attention runs on all rows, dclip_attn_stream_fwd; its only readers are the two dclip_rows_pick.)
Everything else a kernel uses as an address comes from the host (plan offsets, dclip_attn_maps arrays) or from the caller (the token ids,
which are never copied into the workspace).  The saved activation derivative `z` is uint8
data, and the wgrad / mix / maps partial-tile buffers hold f32 partial sums written before their reduce launch reads them: no counters.
No sequence reads one of these stale, so every sequence runs poisoned.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import tower_memory_cases as tm

pytestmark = pytest.mark.gpu

_COUNTS = {'runs': 0, 'bit-reproducible': 0, 'order-noise': 0}


@functools.lru_cache(maxsize=None)
def _run(tag, seq, B, fill, k):
    """run k (0 or 1) of (case, sequence, B) on buffers of its own filled with `fill`"""
    _COUNTS['runs'] += 1
    try:
        return tm.run_sequence(tag, seq, B, fill)
    except (AssertionError, ValueError):             # (ValueError: the library refused an argument before any launch)
        raise
    except Exception as exc:
        # a refused call or a HIP error: after a device error every later launch of this process fails too, so the session ends here
        pytest.exit(f'tower memory run {(tag, seq, B, hex(fill), k)} raised {exc!r}', returncode=3)


@pytest.fixture(scope='module', autouse=True)
def _drop_the_cached_runs_afterwards():
    yield
    _run.cache_clear()
    tm.inputs.cache_clear()
    tm.build.cache_clear()


def _pairs():
    return [(tag, seq) for tag in tm.CASES for seq in tm.sequences_of(tag)]


def _classes(tag, seq, B):
    a, b = _run(tag, seq, B, 0x00, 0), _run(tag, seq, B, 0x00, 1)
    return tm.grad_classes(tm.build(tag)._tower, a['grad'], b['grad'])


def test_the_built_towers_are_the_cases_the_table_describes():
    from distillclip_amd._lib import lib
    for tag, c in tm.CASES.items():
        tw = tm.build(tag)._tower
        assert (tw.cfg.kind, tw.cfg.modality, tw.cfg.tokens, bool(tw.cfg.head_mix), bool(tw.cfg.causal)) == \
            (c['kind'], c['modality'], c['tokens'], c['mixing'], c['causal']), tag
        if c['mixing']:
            hd = tw.cfg.width // tw.cfg.heads
            assert lib().dclip_attn_mix_supported(tw.cfg.heads, tw.cfg.tokens, hd) != 0, tag        # path_of() takes this for granted
        assert tw.wcache.numel() == lib().dclip_encoder_wcache_bytes(tw._handle)
        for B in tm.BATCHES:
            for training in ((0, 1) if c['kind'] else (0,)):
                assert lib().dclip_encoder_workspace_bytes(tw._handle, B, training) % 256 == 0, (tag, B, training)


# ---- section 1: guards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,seq', _pairs())
def test_nothing_outside_the_declared_sizes_is_written_and_no_input_changes(tag, seq):
    bad = []
    for B in tm.batches_of(tag, seq):
        for fill, k in ((0x00, 0), (0x00, 1), (0xFF, 0), (0x7B, 0)):
            r = _run(tag, seq, B, fill, k)
            bad += [f'B={B} fill={fill:#04x}: {m}' for m in r['guards'] + r['inputs']]
    assert not bad, '\n'.join(bad[:12])


# ---- section 2: poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,seq', _pairs())
def test_no_result_depends_on_what_the_buffers_held(tag, seq):
    bad, n_repro, n_noise, n_exact = [], 0, 0, 0
    for B in tm.batches_of(tag, seq):
        zero, again = _run(tag, seq, B, 0x00, 0), _run(tag, seq, B, 0x00, 1)
        classes = None
        if zero['grad'] is not None:
            classes = _classes(tag, seq, B)
            n_repro += sum(1 for c in classes[0] if c[2])
            n_noise += sum(1 for c in classes[0] if not c[2])
            n_exact += len(classes[1])
        assert set(zero['fwd']) == set(again['fwd']) and zero['fwd']
        for fill, got in ((0x00, again), (0xFF, _run(tag, seq, B, 0xFF, 0)), (0x7B, _run(tag, seq, B, 0x7B, 0))):
            what = f'B={B} fill={fill:#04x}'
            for name, want in zero['fwd'].items():
                m = tm.bits_differ(got['fwd'][name], want, f'{what}: {name}')
                if m:
                    bad.append(m)
            if classes is not None:
                bad += tm.grad_failures(classes, got['grad'], zero['grad'], what)
    _COUNTS['bit-reproducible'] += n_repro
    _COUNTS['order-noise'] += n_noise
    print(f'{tag} {seq}: gradient ranges over B in {tm.batches_of(tag, seq)}: {n_repro} bit-reproducible between two 0x00 runs, {n_noise} '
          f'order-noise; {n_exact} weight gradients held bit-equal; so far {_COUNTS}')
    assert not bad, '\n'.join(bad[:12])


@pytest.mark.parametrize('tag', tm.STUDENTS)
def test_a_repeated_backward_clears_its_own_seeds_on_a_poisoned_workspace(tag):
    """the backward-only variants of test_towers_gpu.py::test_c_abi_backward_is_self_contained_on_a_repeated_or_foreign_call: a second
    backward on one forward with another d_out, then the first again, each the gradients of a forward + backward of its own"""
    B, bad = 3, []
    inp = tm.inputs(tag, 'train', B)
    g = torch.Generator().manual_seed(99)
    d2 = torch.randn(inp['d_out'].shape, generator=g).cuda()
    zero, again = _run(tag, 'train', B, 0x00, 0), _run(tag, 'train', B, 0x00, 1)
    classes = tm.grad_classes(tm.build(tag)._tower, zero['grad'], again['grad'])
    # the other d_out on a forward of its own, twice, on zero-filled workspaces
    want2 = tm.run_sequence(tag, 'train', B, 0x00, d_out=d2)['grad']
    classes2 = tm.grad_classes(tm.build(tag)._tower, want2, tm.run_sequence(tag, 'train', B, 0x00, d_out=d2)['grad'])
    scale = zero['grad'].abs().max().item()
    assert (want2 - zero['grad']).abs().max().item() > 1e-2 * scale          # the two d_out really give different gradients
    for fill in tm.FILLS:
        r = tm.run_sequence(tag, 'train', B, fill, second_backward=[d2, inp['d_out']])
        bad += [f'fill={fill:#04x}: {m}' for m in r['guards'] + r['inputs']]
        bad += tm.grad_failures(classes, r['grad'], zero['grad'], f'fill={fill:#04x}: first backward')
        bad += tm.grad_failures(classes2, r['more_grads'][0], want2, f'fill={fill:#04x}: second backward, other d_out')
        bad += tm.grad_failures(classes, r['more_grads'][1], zero['grad'], f'fill={fill:#04x}: third backward, first d_out again')
    assert not bad, '\n'.join(bad[:12])


# ---- section 3: reuse ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', tm.CHAIN_CASES + tm.TEACHERS)
def test_one_workspace_through_changing_modes_and_batch_sizes(tag):
    from distillclip_amd.model.component._tower import EncoderRun
    tw = tm.build(tag)._tower
    chain = tm.chain_of(tag)
    arena = tm.Arena(0xFF)
    need = max(tm.workspace_need(tw, seq, B) for seq, B in chain)
    shared = (arena.take(need, torch.uint8, 'the chain\'s workspace'), EncoderRun())
    bad = []
    for step, (seq, B) in enumerate(chain, 1):
        what = f'step {step} ({seq}, B={B})'
        alone = _run(tag, seq, B, 0x00, 0)
        got = tm.run_sequence(tag, seq, B, 0x00, shared=shared)
        assert tw.workspace is shared[0] and tw._run is shared[1], what
        bad += [f'{what}: {m}' for m in got['guards'] + got['inputs']]
        assert set(got['fwd']) == set(alone['fwd'])
        for name, want in alone['fwd'].items():
            m = tm.bits_differ(got['fwd'][name], want, f'{what}: {name}')
            if m:
                bad.append(m)
        if alone['grad'] is not None:
            bad += tm.grad_failures(_classes(tag, seq, B), got['grad'], alone['grad'], what)
    torch.cuda.synchronize()
    bad += arena.guard_failures()
    assert not bad, '\n'.join(bad[:12])


# ---- the two knobs that are read once per process ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('knob', tm.KNOBS)
def test_the_mixing_students_once_more_with_a_knob_switched_off(knob):
    """DCLIP_ATTN_MIX=0 (the head-mixing students on the Unfused score stage, in both modes) and DCLIP_PRUNE_LAST=0 (no pruned execution): all
    three sections for tm.KNOB_CASES in one fresh child process per knob; this process has no GPU work in flight meanwhile"""
    if os.environ.get('DCLIP_TEST_CHILD'):
        pytest.skip('already inside a child test process')
    torch.cuda.synchronize()
    env = dict(os.environ, DCLIP_TEST_CHILD='1')
    env[knob] = '0'
    sel = ' or '.join(tm.KNOB_CASES)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-s', '-k', sel, '-p', 'no:cacheprovider'],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout and 'skipped' not in r.stdout, r.stdout[-2000:]
