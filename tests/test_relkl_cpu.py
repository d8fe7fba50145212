"""The `intra_kl` loss name without a GPU: the C entry's declaration and host refusals, LossCalculator's bookkeeping with the name, and
the float64 reference of tests/relkl_cases.py against torch autograd and against an honest float32 evaluation."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

import relkl_cases as rc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI and the header's wording ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert protos['dclip_relation_kl_workspace'] == (ctypes.c_size_t, [I, I])
    assert protos['dclip_relation_kl'] == (ctypes.c_int, [P, P, I, I, F, F, P, P, P, ctypes.c_size_t, P])
    for name in ('dclip_relation_kl_workspace', 'dclip_relation_kl'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed


def _contract():
    from distillclip_amd._lib import _HEADER
    src = open(_HEADER).read()
    block = src[:src.index('size_t dclip_relation_kl_workspace')]
    block = block[block.rindex('/*'):]
    return re.sub(r'\s*\n \*\s*', ' ', block)


def test_header_states_the_contract():
    text = _contract()
    for words in ('a_ij = s^_i . s^_j / tau', 'b_ij = t^_i . t^_j / tau', 'the diagonal is EXCLUDED from every sum', 'no epsilon',
                  "the row's true maximum", 'never log of a probability', 'intra_kl = tau^2 mean_i KL_i', "not soft_label's sum",
                  'The teacher receives no gradient', 'D = weight (tau / B) (M + M^T)', 'B = 1 has no column and B = 2 one',
                  '1 <= B <= 4096', 'E % 16 == 0', '16 <= E <= 1024', 'tau finite and > 0', 'weight finite', 'One tower per call',
                  'weight * intra_kl, intra_kl, mean_i KL_i, +0', 'OVERWRITTEN', '0 for a refused shape', 'never reach HBM',
                  'Five launches', 'No atomics', 'the same call gives the same bits', '0 * (1 / 0) = NaN',
                  'in EITHER matrix makes every element of d_s and out[0..2] NaN', 'With B = 1 no statistic is read',
                  'DCLIP_EINVAL, nothing launched, nothing written', 'Added without a version bump'):
        assert words in text, words


def test_the_bounds_use_the_kernels_own_shapes():
    from distillclip_amd._lib import _HERE
    src = open(os.path.join(_HERE, 'csrc', 'relation.hip')).read()
    assert int(re.search(r'REL_MAX_B = (\d+),', src).group(1)) == rc.MAX_B
    assert int(re.search(r'REL_MAX_E = (\d+);', src).group(1)) == rc.MAX_E
    assert int(re.search(r'REL_MAX_SLICES = (\d+);', src).group(1)) == 8 and int(re.search(r'REL_LDS_COLS = (\d+);', src).group(1)) == 512
    assert 'stripe_slices((stripe_tiles(B) + 1) / 2, stripe_tiles(B), REL_LDS_COLS)' in src
    # the slice counts the cases are chosen for, and the cap: a slice never exceeds 512 columns
    assert [rc.slices(B) for B in rc.B_LIST] == [1, 1, 1, 1, 1, 2, 3, 3, 8]
    assert rc.slice_tiles(130)[-1] == (7, 9) and rc.slice_tiles(17) == [(0, 1), (1, 2)]
    assert [rc.slices(B) for B in (512, 1024, 2048, 4096)] == [8, 4, 4, 8]
    assert all(max(t1 - t0 for t0, t1 in rc.slice_tiles(B)) <= 32 for B in range(1, 4097, 5))
    assert [rc.n_merge(B) for B in (1, 17, 130, 4096)] == [9, 10, 16, 23]
    assert [rc.n_acc(B) for B in (1, 17, 130, 4096)] == [20, 21, 27, 34]
    # the sweep never gives a wave beyond the second a tile; B = 340 reaches the third, B = 512 and 1040 all four
    assert max(t1 - t0 for B in rc.B_LIST for t0, t1 in rc.slice_tiles(B)) == 2
    assert sorted(t1 - t0 for t0, t1 in rc.slice_tiles(340)) == [2, 2, 3, 3, 3, 3, 3, 3]
    assert [t1 - t0 for t0, t1 in rc.slice_tiles(512)] == [4] * 8 and sorted(t1 - t0 for t0, t1 in rc.slice_tiles(1040)) == [21, 22, 22]


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
def _guarded(n):
    """a patterned host buffer with a 256-byte aligned address in its middle"""
    buf = (ctypes.c_uint8 * (n + 1024))(*[(37 * i + 11) % 251 for i in range(n + 1024)])
    addr = (ctypes.addressof(buf) + 511) & ~255
    return buf, addr


_ARGS = ('s', 't', 'out', 'd_s', 'workspace')


def _call(**k):
    """one call on host buffers: every call here is refused before a launch, and no buffer may change"""
    B, E = k.get('B', 8), k.get('E', 32)
    bufs = {n: _guarded(4096) for n in _ARGS}
    before = {n: bytes(b[0]) for n, b in bufs.items()}
    p = {n: bufs[n][1] for n in _ARGS}
    for n in _ARGS:
        if n in k:
            p[n] = None if k[n] is None else p[n] + k[n]
    ws_bytes = k.get('ws_bytes', max(_lib().dclip_relation_kl_workspace(B, E), 1 << 20))
    try:
        _lib().dclip_relation_kl(p['s'], p['t'], B, E, k.get('tau', 0.07), k.get('weight', 1.0), p['out'], p['d_s'], p['workspace'],
                                 ws_bytes, None)
    finally:
        for n, b in bufs.items():
            assert bytes(b[0]) == before[n], f'{n} was written by a refused call'


@pytest.mark.parametrize('kw,word', [
    (dict(B=0), '1 <= B <= 4096'), (dict(B=-3), '1 <= B <= 4096'), (dict(B=4097), '1 <= B <= 4096'),
    (dict(E=0), 'E=0'), (dict(E=8), 'E=8'), (dict(E=40), 'E=40'), (dict(E=1040), 'E=1040'), (dict(E=-16), 'E=-16'),
    (dict(tau=0.0), 'tau'), (dict(tau=-0.07), 'tau'), (dict(tau=float('inf')), 'tau'), (dict(tau=float('nan')), 'tau'),
    (dict(weight=float('inf')), 'weight'), (dict(weight=float('-inf')), 'weight'), (dict(weight=float('nan')), 'weight'),
    *[({n: None}, 'null') for n in _ARGS],
    *[({n: 4}, 'misaligned') for n in _ARGS], (dict(workspace=128), 'misaligned'), (dict(t=2), 'misaligned'),
    (dict(ws_bytes=0), 'workspace too small'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word) as e:
        _call(**kw)
    assert 'dclip_relation_kl:' in str(e.value)                  # the error string names the entry


def test_workspace_query_and_a_workspace_one_byte_short():
    l = _lib()
    for B, E in ((0, 64), (-1, 64), (4097, 64), (8, 0), (8, 8), (8, 40), (8, 1040), (8, -16)):
        assert l.dclip_relation_kl_workspace(B, E) == 0, (B, E)
    for B, E in ((1, 16), (130, 768), (512, 512), (4096, 1024)):
        need = l.dclip_relation_kl_workspace(B, E)
        zs = rc.slices(B)
        # two normalised copies and one partial gradient per slice, plus per-row and per-stripe records
        assert need % 256 == 0 and need >= (2 + zs) * B * E * 4
        assert need <= (2 + zs) * (B * E * 4 + 256) + (2 * zs + 3) * B * 4 + zs * B + 8 * 256
        with pytest.raises(ValueError, match='workspace too small'):
            _call(B=B, E=E, ws_bytes=need - 1)


# ---- 3. LossCalculator ---------------------------------------------------------------------------------------------------------------
def _rep(B, E, g):
    return types.SimpleNamespace(last_representation=torch.randn(B, E, generator=g))


def _standin(B=4, E=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    two = lambda: types.SimpleNamespace(visual_output=_rep(B, E, g), text_output=_rep(B, E, g))
    return two(), two()


def test_intra_kl_needs_a_temperature():
    from distillclip_amd.model import LossCalculator
    stu, tea = _standin()
    for model_type, so, to in (('all', stu, tea), ('image', stu.visual_output, tea.visual_output)):
        with pytest.raises(AssertionError, match='You should give the temperature for the kl loss'):
            LossCalculator(['out_cos', 'intra_kl'])(so, to, model_type)
    with pytest.raises(AssertionError, match='You should give the temperature for the kl loss'):
        LossCalculator(['out_cos', 'soft_label'])(stu, tea, 'all')          # the same assertion, at the same point


def test_name_registration_and_bookkeeping():
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model._loss import IMAGE_TEXT_LOSS, _TOWER_OWN
    assert 'intra_kl' in _TOWER_OWN and 'intra_kl' not in IMAGE_TEXT_LOSS
    lc = LossCalculator(['out_l1', 'intra_kl', 'soft_label'], {'intra_kl': 0.5}, temperature=0.07)
    assert lc.loss_scale == {'out_l1': 1, 'intra_kl': 0.5, 'soft_label': 1}
    assert lc.percent == pytest.approx({n: 1 / 3 for n in lc.loss_name})
    lc = LossCalculator(['out_l1', 'intra_kl'], percent={'intra_kl': 0.25, 'out_l1': 0.75}, temperature=0.07)
    assert lc.percent == {'intra_kl': 0.25, 'out_l1': 0.75}
    # the fused kernel's weights never see the name, with one tower or two
    assert lc._weights(True) == {'out_l1': 0.75} and lc._weights(False) == {'out_l1': 0.75}


def test_bookkeeping_of_both_modes_with_a_stand_in_kernel(monkeypatch):
    """res = loss_scale * intra_kl, total += res * percent; one tower: key intra_kl; two: image_ / text_ under 0.5 (image + text)"""
    from distillclip_amd.model import LossCalculator, _loss
    calls = []

    def fake_distill(s_img, t_img, s_txt=None, t_txt=None, **k):
        return torch.zeros(16), torch.zeros_like(s_img), None if s_txt is None else torch.zeros_like(s_txt)

    def fake_relation(s, t, temperature, weight=1.0):
        calls.append((s, t, temperature, weight))
        v = float(len(calls))                                     # intra_kl of call n is n
        return torch.tensor([weight * v, v, 9.0, 0.0]), torch.ones_like(s) * weight
    monkeypatch.setattr(_loss.ops, 'distill_loss', fake_distill)
    monkeypatch.setattr(_loss.ops, 'relation_kl', fake_relation)
    stu, tea = _standin()
    for o in (stu.visual_output, stu.text_output):
        o.last_representation.requires_grad_(True)
    lc = LossCalculator(['out_l1', 'intra_kl'], {'intra_kl': 3.0}, temperature=0.5, percent={'intra_kl': 0.25, 'out_l1': 0.75})
    loss, res = lc(stu, tea, 'all')
    assert set(res) == {'image_out_l1', 'text_out_l1', 'image_intra_kl', 'text_intra_kl'}
    assert res['image_intra_kl'].item() == 3.0 and res['text_intra_kl'].item() == 6.0
    assert loss.item() == pytest.approx(0.5 * (3.0 * 0.25 * 1 + 3.0 * 0.25 * 2))
    assert [c[2:] for c in calls] == [(0.5, 0.75), (0.5, 0.75)]
    assert torch.equal(calls[0][0], stu.visual_output.last_representation) and torch.equal(calls[1][1], tea.text_output.last_representation)
    loss.backward()
    assert torch.equal(stu.visual_output.last_representation.grad, torch.full((4, 16), 0.5 * 0.75))      # the kernel's gradient, halved
    calls.clear()
    s1 = _rep(4, 16, torch.Generator().manual_seed(1))
    s1.last_representation.requires_grad_(True)
    loss, res = lc(s1, tea.visual_output, 'image')
    assert set(res) == {'out_l1', 'intra_kl'} and res['intra_kl'].item() == 3.0 and loss.item() == pytest.approx(0.75)
    loss.backward()
    assert torch.equal(s1.last_representation.grad, torch.full((4, 16), 0.75))


def test_control_output_is_unchanged_by_the_new_name():
    from distillclip_amd.model import LossCalculator
    a = LossCalculator(['out_l1', 'hidden_rep_mse']).get_control_output()
    b = LossCalculator(['out_l1', 'hidden_rep_mse', 'intra_kl'], temperature=0.07).get_control_output()
    assert vars(a) == vars(b)
    assert vars(LossCalculator(['intra_kl'], temperature=0.07).get_control_output()) == vars(LossCalculator(['out_l1']).get_control_output())


@pytest.mark.parametrize('model_type', ['all', 'image'])
def test_a_batch_beyond_the_kernels_rows_raises_before_anything_launches(monkeypatch, model_type):
    from distillclip_amd.model import LossCalculator, _loss
    lc = LossCalculator(['out_cos', 'intra_kl'], temperature=0.07)
    stu, tea = _standin(B=4097, E=16)

    def boom(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(_loss.ops, 'distill_loss', boom)
    monkeypatch.setattr(_loss.ops, 'relation_kl', boom)
    with pytest.raises(ValueError, match='4096.*dclip_relation_kl'):
        lc(*((stu, tea) if model_type == 'all' else (stu.visual_output, tea.visual_output)), model_type)


def test_global_negatives_is_not_refused_and_adds_no_collective(monkeypatch):
    """a tower term over the rank's own rows in both modes: the flag reaches the fused kernel's function as before, the term's call
    sees the local rows"""
    from distillclip_amd.model import LossCalculator, _loss
    seen = []
    monkeypatch.setattr(_loss._FusedLossFn, 'apply', lambda *a: (seen.append(a[-1]), (torch.zeros(()), torch.zeros(16)))[1])
    monkeypatch.setattr(_loss.ops, 'relation_kl', lambda s, t, tau, w=1.0: (seen.append(tuple(s.shape)), (torch.zeros(4), torch.zeros_like(s)))[1])
    lc = LossCalculator(['out_cos', 'intra_kl'], temperature=0.07)
    lc.global_negatives = True
    stu, tea = _standin(B=4, E=16)
    loss, res = lc(stu, tea, 'all')
    assert seen == [True, (4, 16), (4, 16)] and set(res) == {'image_out_cos', 'text_out_cos', 'image_intra_kl', 'text_intra_kl'}


def test_unknown_and_refused_names_behave_as_before():
    from distillclip_amd.model import LossCalculator
    with pytest.raises(ValueError, match='Invalid Loss Type!'):
        LossCalculator(['out_l1', 'nope'])
    with pytest.raises(ValueError, match='Invalid Loss Type!'):
        LossCalculator(['intra_kl', 'nope'], temperature=0.07)
    for n in ('attention_probs_kl', 'last_value_map_kl', 'vit_kd', 'fine_grain', 'smd'):
        with pytest.raises(NotImplementedError):
            LossCalculator(['out_l1', 'intra_kl', n], temperature=0.07)


def test_ops_refuses_what_the_kernel_cannot_take():
    from distillclip_amd import ops
    x = torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.relation_kl(x, x, 0.07)


# ---- 4. the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', rc.CASES, ids=repr)
def test_reference_agrees_with_torch_autograd(case):
    ref = case.ref
    intra, kl, ds = rc.torch_autograd_f64(case.e, case.tau)
    # 1e-12 of the value plus the size of the terms it is a sum of: a log-probability is up to 2 / tau, an element of the gradient a sum
    # of (p + q)_ij s^_j tau / (B |s_i|) that cancels where student and teacher agree (both sides then hold float64 rounding only)
    want = torch.stack([intra, kl])
    assert ((ref.out[1:3] - want).abs() <= 1e-12 * (want.abs() + torch.tensor([case.tau, 1 / case.tau]))).all()
    term = 4 * case.tau / (case.B * case.e['s'].to(rc.F64).norm(dim=1, keepdim=True))
    assert ((ref.g - ds).abs() <= 1e-12 * (ds.abs() + term)).all()


@pytest.mark.parametrize('case', rc.CASES, ids=repr)
def test_float32_evaluation_stays_within_half_of_every_bound(case):
    ref = case.ref
    out, g = rc.evaluate_f32(case.e, case.tau)
    q = max(rc.ratio((out - ref.out).abs(), ref.out_b), rc.ratio((g - ref.g).abs(), ref.gb))
    assert q <= 0.5, q


def test_the_extra_families_are_what_they_claim():
    o = rc.ORTHOGONAL
    for A in o.ref.A:
        cos = (A * o.tau).masked_fill(torch.eye(o.B, dtype=torch.bool), 0.0)
        assert cos.abs().max() <= 0.02 and cos.abs().max() > 0.002
    c = rc.TEACHER_COPIES
    assert torch.equal(c.e['t'], c.e['t'][:1].expand_as(c.e['t']))
    la = (c.ref.A[0] - c.ref.lse[0][:, None]).masked_fill(torch.eye(c.B, dtype=torch.bool), 0.0)
    assert (c.ref.kl_rows - (-math.log(c.B - 1) - la.sum(1) / (c.B - 1))).abs().max() < 1e-12
    for c in rc.DUP_PAIR:
        i, j = rc.DUP_ROWS
        assert torch.equal(c.e['s'][i], c.e['s'][j]) and i // 16 == j // 16
        assert abs(c.ref.A[0][i, j].item() * c.tau - 1) < 1e-12
    for c in rc.EQUAL:
        assert torch.equal(c.e['s'], c.e['t']) and (c.ref.out == 0).all() and (c.ref.g == 0).all()
    for c in rc.CASES:                                   # row norms over two decades wherever there are two rows
        if c.B >= 2:
            for k in rc.KEYS if c is not rc.TEACHER_COPIES else ('s',):
                n = c.e[k].norm(dim=1)
                assert n.max() / n.min() > 100, (c, k)
    for B in (1, 2):                                     # no column / one column: zeros by construction
        for c in (rc.sweep_case(B, 48, 0.07), rc.sweep_case(B, 768, 0.01)):
            assert (c.ref.out == 0).all() and (c.ref.g == 0).all()


def test_every_wrong_kernel_leaves_the_bounds_somewhere():
    """the deliberate breaks the reference can restate move some output beyond its bound on at least one case"""
    probes = [c for c in rc.CASES if (c.B, c.E) in ((17, 48), (130, 768), (33, 48), (512, 512))]
    for wrong in rc.WRONGS:
        worst = 0.0
        for c in probes:
            w = rc.Reference(c.e, c.tau, wrong=wrong)
            worst = max(worst, rc.ratio((w.out - c.ref.out).abs(), c.ref.out_b), rc.ratio((w.g - c.ref.g).abs(), c.ref.gb))
        assert worst > 4, (wrong, worst)
