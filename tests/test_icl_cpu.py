"""The `icl` and `out_mse` loss names without a GPU: the C entry's declaration and host refusals, LossCalculator's bookkeeping with the
two names, and the float64 reference of tests/icl_cases.py against torch autograd and against an honest float32 evaluation."""
import ctypes
import re
import types

import pytest
import torch

import icl_cases as ic


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI and the header's wording ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert protos['dclip_interactive_loss_workspace'] == (ctypes.c_size_t, [I, I])
    assert protos['dclip_interactive_loss'] == (ctypes.c_int, [P, P, P, P, I, I, F, F, P, P, P, P, ctypes.c_size_t, P])
    for name in ('dclip_interactive_loss_workspace', 'dclip_interactive_loss'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed


def _contract():
    from distillclip_amd._lib import _HEADER
    src = open(_HEADER).read()
    block = src[:src.index('size_t dclip_interactive_loss_workspace')]
    block = block[block.rindex('/*'):]
    return re.sub(r'\s*\n \*\s*', ' ', block)


def test_header_states_the_contract():
    text = _contract()
    for words in ('A_ij = a^_i . q^_j / tau', 'C_ij = b^_i . p^_j / tau', 'icl = (L_i2t + L_t2i) / 2', 'no epsilon',
                  'The anchors are the student rows only', 'the teacher receives no gradient', "row's true maximum",
                  '1 <= B <= 4096', 'E % 16 == 0', '16 <= E <= 1024', 'tau finite and > 0', 'weight finite',
                  'weight * icl, icl, L_i2t, L_t2i', 'OVERWRITTEN', '0 for a refused shape', 'never reach HBM',
                  'No atomics', 'the same call gives the same bits', 'follow dclip_distill_loss', '0 * (1 / 0) = NaN',
                  'makes row i of its own gradient NaN', 'makes every logit of its column NaN',
                  'DCLIP_EINVAL, nothing launched, nothing written', 'Added without a version bump'):
        assert words in text, words


def test_the_bounds_use_the_kernels_own_shapes():
    from distillclip_amd._lib import _HERE
    import os
    src = open(os.path.join(_HERE, 'csrc', 'interactive.hip')).read()
    assert int(re.search(r'ICL_MAX_B = (\d+),', src).group(1)) == ic.MAX_B
    assert int(re.search(r'ICL_MAX_E = (\d+);', src).group(1)) == ic.MAX_E
    assert int(re.search(r'ICL_MAX_SLICES = (\d+);', src).group(1)) == 8 and int(re.search(r'ICL_LDS_COLS = (\d+);', src).group(1)) == 512
    # the slice counts the cases are chosen for, and the cap: a slice never exceeds 512 columns
    assert [ic.slices(B) for B in ic.B_LIST] == [1, 1, 1, 1, 2, 3, 3, 8]
    assert ic.slice_tiles(130)[-1] == (7, 9) and ic.slice_tiles(17) == [(0, 1), (1, 2)]
    assert [ic.slices(B) for B in (512, 1024, 2048, 4096)] == [4, 2, 4, 8]
    assert all(max(t1 - t0 for t0, t1 in ic.slice_tiles(B)) <= 32 for B in range(1, 4097, 5))
    assert [ic.n_merge(B) for B in (1, 17, 130, 4096)] == [9, 10, 16, 23]
    # the sweep never gives a wave beyond the second a tile; the four-waves cases do
    assert max(t1 - t0 for B in ic.B_LIST for t0, t1 in ic.slice_tiles(B)) == 2
    assert sorted(t1 - t0 for t0, t1 in ic.slice_tiles(340)) == [4, 4, 4, 5, 5] and [t1 - t0 for t0, t1 in ic.slice_tiles(512)] == [8] * 4


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
def _guarded(n):
    """a patterned host buffer with a 256-byte aligned address in its middle"""
    buf = (ctypes.c_uint8 * (n + 1024))(*[(37 * i + 11) % 251 for i in range(n + 1024)])
    addr = (ctypes.addressof(buf) + 511) & ~255
    return buf, addr


_ARGS = ('s_img', 't_img', 's_txt', 't_txt', 'out', 'd_s_img', 'd_s_txt', 'workspace')


def _call(**k):
    """one call on host buffers: every call here is refused before a launch, and no buffer may change"""
    B, E = k.get('B', 8), k.get('E', 32)
    bufs = {n: _guarded(4096) for n in _ARGS}
    before = {n: bytes(b[0]) for n, b in bufs.items()}
    p = {n: bufs[n][1] for n in _ARGS}
    for n in _ARGS:
        if n in k:
            p[n] = None if k[n] is None else p[n] + k[n]
    ws_bytes = k.get('ws_bytes', max(_lib().dclip_interactive_loss_workspace(B, E), 1 << 20))
    try:
        _lib().dclip_interactive_loss(p['s_img'], p['t_img'], p['s_txt'], p['t_txt'], B, E, k.get('tau', 0.07), k.get('weight', 1.0),
                                      p['out'], p['d_s_img'], p['d_s_txt'], p['workspace'], ws_bytes, None)
    finally:
        for n, b in bufs.items():
            assert bytes(b[0]) == before[n], f'{n} was written by a refused call'


@pytest.mark.parametrize('kw,word', [
    (dict(B=0), '1 <= B <= 4096'), (dict(B=-3), '1 <= B <= 4096'), (dict(B=4097), '1 <= B <= 4096'),
    (dict(E=0), 'E=0'), (dict(E=8), 'E=8'), (dict(E=40), 'E=40'), (dict(E=1040), 'E=1040'), (dict(E=-16), 'E=-16'),
    (dict(tau=0.0), 'tau'), (dict(tau=-0.07), 'tau'), (dict(tau=float('inf')), 'tau'), (dict(tau=float('nan')), 'tau'),
    (dict(weight=float('inf')), 'weight'), (dict(weight=float('-inf')), 'weight'), (dict(weight=float('nan')), 'weight'),
    *[({n: None}, 'null') for n in _ARGS],
    *[({n: 4}, 'misaligned') for n in _ARGS], (dict(workspace=128), 'misaligned'), (dict(s_txt=2), 'misaligned'),
    (dict(ws_bytes=0), 'workspace too small'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word) as e:
        _call(**kw)
    assert 'dclip_interactive_loss:' in str(e.value)             # the error string names the entry


def test_workspace_query_and_a_workspace_one_byte_short():
    l = _lib()
    for B, E in ((0, 64), (-1, 64), (4097, 64), (8, 0), (8, 8), (8, 40), (8, 1040), (8, -16)):
        assert l.dclip_interactive_loss_workspace(B, E) == 0, (B, E)
    for B, E in ((1, 16), (130, 768), (512, 512), (4096, 1024)):
        need = l.dclip_interactive_loss_workspace(B, E)
        # four normalised copies and one partial gradient per tower and slice, plus per-row and per-stripe records
        assert need % 256 == 0 and need >= (4 + 2 * ic.slices(B)) * B * E * 4
        assert need <= (4 + 2 * ic.slices(B)) * (B * E * 4 + 256) + (2 * ic.slices(B) + 4) * B * 4 + B + 6 * 256
        with pytest.raises(ValueError, match='workspace too small'):
            _call(B=B, E=E, ws_bytes=need - 1)


# ---- 3. LossCalculator ---------------------------------------------------------------------------------------------------------------
def _standin(B=4, E=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    rep = lambda: types.SimpleNamespace(last_representation=torch.randn(B, E, generator=g))
    two = lambda: types.SimpleNamespace(visual_output=rep(), text_output=rep())
    return two(), two()


def test_icl_needs_a_temperature():
    from distillclip_amd.model import LossCalculator
    stu, tea = _standin()
    lc = LossCalculator(['out_cos', 'icl'])
    with pytest.raises(AssertionError, match='You should give the temperature'):
        lc(stu, tea, 'all')
    with pytest.raises(AssertionError, match='You should give the temperature'):
        LossCalculator(['out_cos', 'soft_label'])(stu, tea, 'all')          # the same assertion, at the same point
    assert LossCalculator(['out_cos', 'icl'])._weights(False) == {'out_cos': 0.5}     # one tower: the name is ignored, no temperature needed


def test_percent_and_scale_bookkeeping_with_the_new_names():
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model._loss import IMAGE_TEXT_LOSS
    assert 'icl' in IMAGE_TEXT_LOSS and 'out_mse' not in IMAGE_TEXT_LOSS
    lc = LossCalculator(['out_l1', 'out_mse', 'icl', 'soft_label'], {'icl': 0.5}, temperature=0.07)
    assert lc.loss_scale == {'out_l1': 1, 'out_mse': 1, 'icl': 0.5, 'soft_label': 1}
    assert lc.percent == {n: 0.25 for n in lc.loss_name}
    lc = LossCalculator(['out_mse', 'icl'], percent={'icl': 0.5}, temperature=0.07)
    assert lc.percent == pytest.approx({'icl': 0.5, 'out_mse': 0.5})       # the reference's default rule: (1 - sum) / len(percent)
    lc = LossCalculator(['out_mse', 'icl'], percent={'icl': 0.25, 'out_mse': 0.75}, temperature=0.07)
    assert lc.percent == {'icl': 0.25, 'out_mse': 0.75}
    with pytest.raises(AssertionError):
        LossCalculator(['out_mse', 'icl'], percent={'icl': 0.5, 'out_mse': 0.75})
    # the fused kernel's weights never see the new names
    lc = LossCalculator(['out_l1', 'out_mse', 'icl', 'soft_label'], {'icl': 0.5}, temperature=0.07)
    assert lc._weights(True) == {'out_l1': 0.25, 'soft_label': 0.25} and lc._weights(False) == {'out_l1': 0.25}


def test_control_output_is_unchanged_by_the_new_names():
    from distillclip_amd.model import LossCalculator
    a = LossCalculator(['out_l1', 'hidden_rep_mse']).get_control_output()
    b = LossCalculator(['out_l1', 'hidden_rep_mse', 'out_mse', 'icl'], temperature=0.07).get_control_output()
    assert vars(a) == vars(b)
    c = LossCalculator(['out_mse', 'icl'], temperature=0.07).get_control_output()
    assert vars(c) == vars(LossCalculator(['out_l1']).get_control_output())


def test_global_negatives_with_icl_raises_before_anything_runs(monkeypatch):
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model import _loss
    lc = LossCalculator(['out_cos', 'icl'], temperature=0.07)
    lc.global_negatives = True
    stu, tea = _standin()

    def boom(*a, **k):
        raise AssertionError('a kernel or a collective was reached')
    monkeypatch.setattr(_loss.ops, 'distill_loss', boom)
    monkeypatch.setattr(_loss.ops, 'interactive_loss', boom)
    with pytest.raises(ValueError, match='global_negatives'):
        lc(stu, tea, 'all')


def test_a_batch_beyond_the_kernels_rows_raises(monkeypatch):
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model import _loss
    lc = LossCalculator(['out_cos', 'icl'], temperature=0.07)
    stu, tea = _standin(B=4097, E=16)
    monkeypatch.setattr(_loss.ops, 'distill_loss', lambda *a, **k: (_ for _ in ()).throw(AssertionError('launched')))
    with pytest.raises(ValueError, match='4096'):
        lc(stu, tea, 'all')


def test_unknown_and_refused_names_behave_as_before():
    from distillclip_amd.model import LossCalculator
    with pytest.raises(ValueError, match='Invalid Loss Type!'):
        LossCalculator(['out_l1', 'nope'])
    with pytest.raises(ValueError, match='Invalid Loss Type!'):
        LossCalculator(['icl', 'out_mse', 'nope'], temperature=0.07)
    for n in ('attention_probs_kl', 'last_value_map_kl', 'vit_kd', 'fine_grain', 'smd'):
        with pytest.raises(NotImplementedError):
            LossCalculator(['out_l1', 'icl', n], temperature=0.07)


def test_ops_refuses_what_the_kernel_cannot_take():
    from distillclip_amd import ops
    x = torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.interactive_loss(x, x, x, x, 0.07)


# ---- 4. the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ic.CASES, ids=repr)
def test_reference_agrees_with_torch_autograd(case):
    ref = case.ref
    icl, l0, l1, da, db = ic.torch_autograd_f64(case.e, case.tau)
    # 1e-12 of the value plus the size of the terms it is a sum of: a logit is up to 1 / tau, an element of the gradient a sum of
    # P_ij q^_j / (2 B tau |a_i|) that cancels where the loss is near 0 (both sides then hold float64 rounding only)
    want = torch.stack([icl, l0, l1])
    assert ((ref.out[1:] - want).abs() <= 1e-12 * (want.abs() + 1 / case.tau)).all()
    for got, auto, x in ((ref.g[0], da, case.e['si']), (ref.g[1], db, case.e['st'])):
        term = 1 / (2 * case.B * case.tau * x.to(ic.F64).norm(dim=1, keepdim=True))
        assert ((got - auto).abs() <= 1e-12 * (auto.abs() + term)).all()


def test_out_mse_restatement_agrees_with_torch():
    e = ic.SWEEP_CASES[5].e
    s, t = e['si'].to(ic.F64).requires_grad_(True), e['ti'].to(ic.F64)
    torch.nn.functional.mse_loss(s, t).backward()
    assert torch.allclose(s.grad, 2 * (s.detach() - t) / s.numel(), rtol=1e-12, atol=0)


@pytest.mark.parametrize('case', ic.CASES, ids=repr)
def test_float32_evaluation_stays_within_half_of_every_bound(case):
    ref = case.ref
    out, g = ic.evaluate_f32(case.e, case.tau)
    q = max(ic.ratio((out - ref.out).abs(), ref.out_b), ic.ratio((g[0] - ref.g[0]).abs(), ref.gb[0]),
            ic.ratio((g[1] - ref.g[1]).abs(), ref.gb[1]))
    assert q <= 0.5, q


def test_the_extra_families_are_what_they_claim():
    o = ic.ORTHOGONAL
    for X in o.ref.X:
        assert (X * o.tau).abs().max() <= 0.02 and (X * o.tau).abs().max() > 0.002
    for c in ic.PAIRED:
        assert c.ref.out[1] < (1e-6 if c.tau == 0.01 else 0.2) and (c.ref.X[0].diagonal() * c.tau - 1).abs().max() < 1e-12
    t = ic.ONE_TEXT
    assert abs(t.ref.out[2].item() - torch.log(torch.tensor(40.0, dtype=ic.F64)).item()) < 1e-12
    for c in ic.CASES:                                   # row norms over two decades wherever there are two rows
        if c.B >= 2:
            for k in ic.KEYS if c is not ic.ONE_TEXT else ('si', 'ti', 'st'):
                n = c.e[k].norm(dim=1)
                assert n.max() / n.min() > 100, (c, k)


def test_every_wrong_kernel_leaves_the_bounds_somewhere():
    """the deliberate breaks the reference can restate move some output beyond its bound on at least one case"""
    probes = [c for c in ic.CASES if (c.B, c.E) in ((17, 48), (130, 768), (33, 48), (340, 48))]
    for wrong in ic.WRONGS:
        worst = 0.0
        for c in probes:
            w = ic.Reference(c.e, c.tau, wrong=wrong)
            worst = max(worst, ic.ratio((w.out - c.ref.out).abs(), c.ref.out_b),
                        *(ic.ratio((w.g[d] - c.ref.g[d]).abs(), c.ref.gb[d]) for d in (0, 1)))
        assert worst > 4, (wrong, worst)
