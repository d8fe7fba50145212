"""dclip_relation_kl (the `intra_kl` term) element by element against float64, its exact symmetries, its memory contract, and the new
LossCalculator name up to one training step.  Inputs, reference and bounds: tests/relkl_cases.py (its docstring derives every bound;
tests/test_relkl_cpu.py checks them without the kernel).  Every kernel call of this file runs on inputs surrounded by NaNs, with outputs
between sentinels and a workspace of exactly the queried size in front of a patterned guard.

Measured on an MI355X, worst err / bound over all 105 cases (printed by the last test of this file, also in DESIGN.md section 7.0):
gradients 0.024, scalars 0.008.  The float32 evaluation on the CPU uses at most 0.021 of a bound.  The whole file: 146 tests in 4 s."""
import math
import types

import pytest
import torch

import relkl_cases as rc

pytestmark = pytest.mark.gpu

DEV = 'cuda' if torch.cuda.is_available() else 'cpu'
PAD_FRONT, PAD_BACK = 4, 64                          # floats around every tensor: 16 bytes in front, so never 256-byte aligned
WS_GUARD = 4096
WORST = {}                                           # what -> worst err / bound of this process


def _lib():
    from distillclip_amd._lib import lib
    return lib()


class _Slot:
    """an owned [n] float range inside a larger NaN-filled buffer (all-ones bits), PAD_FRONT floats after its start"""

    def __init__(self, n, data=None):
        self.n = n
        self.buf = torch.full((PAD_FRONT + n + PAD_BACK,), -1, dtype=torch.int32, device=DEV).view(torch.float32)
        if data is not None:
            self.buf[PAD_FRONT:PAD_FRONT + n] = data.reshape(-1).to(DEV)
        self.before = self.buf.clone()
        assert self.ptr % 16 == 0 and self.ptr % 256 != 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD_FRONT

    def owned(self):
        return self.buf[PAD_FRONT:PAD_FRONT + self.n]

    def foreign_changed(self, owned_may_change):
        want = self.before.clone()
        if owned_may_change:
            want[PAD_FRONT:PAD_FRONT + self.n] = self.owned()
        return int((want.view(torch.int32) != self.buf.view(torch.int32)).sum())


class _Workspace:
    """exactly dclip_relation_kl_workspace(B, E) bytes at a 256-byte-aligned offset of a patterned buffer, WS_GUARD bytes behind"""

    def __init__(self, B, E):
        self.bytes = _lib().dclip_relation_kl_workspace(B, E)
        assert self.bytes > 0
        n = 512 + self.bytes + WS_GUARD
        self.buf = ((torch.arange(n, device=DEV, dtype=torch.int32) * 37 + 11) % 251).to(torch.uint8)
        self.off = (-self.buf.data_ptr()) % 256 + 256
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + self.off

    def foreign_changed(self):
        end = self.off + self.bytes
        return int((self.buf[:self.off] != self.before[:self.off]).sum()) + int((self.buf[end:] != self.before[end:]).sum())


def run(e, tau, weight=1.0):
    """one guarded call -> (out [4], d_s), f32 on the CPU; asserts the memory contract and that out[3] is +0"""
    B, E = e['s'].shape
    ins = [_Slot(B * E, e[k]) for k in rc.KEYS]
    d, out = _Slot(B * E), _Slot(4)
    ws = _Workspace(B, E)
    _lib().dclip_relation_kl(ins[0].ptr, ins[1].ptr, B, E, tau, weight, out.ptr, d.ptr, ws.ptr, ws.bytes,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bad = [f'input {k}: {s.foreign_changed(False)} floats changed' for k, s in zip(rc.KEYS, ins) if s.foreign_changed(False)]
    bad += [f'{n}: {s.foreign_changed(True)} floats changed outside what the call owns'
            for n, s in (('d_s', d), ('out', out)) if s.foreign_changed(True)]
    if ws.foreign_changed():
        bad.append(f'workspace: {ws.foreign_changed()} guard bytes changed around its {ws.bytes} bytes')
    assert not bad, bad
    o = out.owned().cpu()
    assert o.view(torch.int32)[3].item() == 0, f'out[3] is not +0: {o[3].item()!r}'
    return o, d.owned().view(B, E).cpu()


def _bits(*ts):
    return [t.contiguous().view(torch.int32) for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


def _worst(what, q):
    WORST[what] = max(WORST.get(what, 0.0), q)


NAMES = ('weight * intra_kl', 'intra_kl', 'mean KL')


def _check(ref, got, label, perm=None):
    """every element of the gradient and the three scalars within the bounds; -> the failures"""
    out, d = got
    want, bound = (ref.g, ref.gb) if perm is None else (ref.g[perm], ref.gb[perm])
    fails = []
    q = rc.ratio((d.to(rc.F64) - want).abs(), bound)
    _worst('gradient', q)
    if not q <= 1:
        fails.append(f'{label} d_s: err / bound = {q:.3g}')
    for i, name in enumerate(NAMES):
        q = rc.ratio((out[i].to(rc.F64) - ref.out[i]).abs().reshape(1), ref.out_b[i].reshape(1))
        _worst('scalar', q)
        if not q <= 1:
            fails.append(f'{label} {name}: {out[i].item()!r} against {ref.out[i].item()!r}, err / bound = {q:.3g}')
    return fails


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', rc.CASES, ids=repr)
def test_every_element_against_float64(case):
    fails = _check(case.ref, run(case.e, case.tau), repr(case))
    assert not fails, fails


def test_teacher_copies_give_the_closed_form():
    """q uniform: KL_i = -log(B - 1) - mean_{j != i} (a_ij - lseS_i), so mean KL follows from the student's side alone"""
    c = rc.TEACHER_COPIES
    out, _ = run(c.e, c.tau)
    la = (c.ref.A[0] - c.ref.lse[0][:, None]).masked_fill(torch.eye(c.B, dtype=torch.bool), 0.0)
    want = (-math.log(c.B - 1) - la.sum(1) / (c.B - 1)).mean()
    assert abs(out[2].item() - want.item()) <= c.ref.out_b[2].item()


def test_joint_permutation_of_the_samples_permutes_the_gradient_rows():
    """within the bound, not bit for bit: the rows change stripes and the columns change slices, so every merge order changes"""
    for c in (rc.sweep_case(130, 768, 0.01), rc.sweep_case(33, 48, 0.07)):
        perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
        e = {k: v[perm].contiguous() for k, v in c.e.items()}
        fails = _check(c.ref, run(e, c.tau), f'{c} permuted', perm)
        assert not fails, fails


# ---- 2. exact, no tolerance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('E', [16, 48, 768])
@pytest.mark.parametrize('tau', rc.TAUS)
def test_batches_of_one_and_two_are_exactly_zero(B, E, tau):
    out, d = run(rc._draw(B, E, 5), tau, weight=3.0)
    assert (out == 0).all() and (d == 0).all(), (out, d.abs().max())


@pytest.mark.parametrize('case', rc.EQUAL, ids=repr)
def test_student_bit_equal_to_teacher_is_exactly_zero(case):
    """dot_tile gives bit-equal rows bit-equal products, and both statistics go through the same merges: p and q are the same bits"""
    for w in (1.0, -2.5):
        out, d = run(case.e, case.tau, weight=w)
        assert (out == 0).all() and (d == 0).all(), (out, d.abs().max())


EXACT = rc.sweep_case(33, 48, 0.07)                  # three stripes, three slices


def test_scaling_teacher_rows_by_powers_of_two_changes_no_bit():
    c = EXACT
    base = run(c.e, c.tau)
    e = dict(c.e)
    s = torch.tensor([2.0 ** -30, 2.0 ** 7, 2.0 ** 30])[torch.randint(0, 3, (c.B,), generator=torch.Generator().manual_seed(3))]
    assert len(set(s.tolist())) == 3
    e['t'] = (c.e['t'] * s[:, None]).contiguous()
    assert _same_bits(run(e, c.tau), base)


@pytest.mark.parametrize('k', [-30, 7, 30])
def test_scaling_a_student_row_by_a_power_of_two(k):
    c, row = EXACT, 18
    base = run(c.e, c.tau)
    e = dict(c.e)
    e['s'] = c.e['s'].clone()
    e['s'][row] *= 2.0 ** k
    got = run(e, c.tau)
    assert _same_bits([got[0]], [base[0]])
    want = base[1].clone()
    want[row] *= 2.0 ** -k
    assert _same_bits([got[1]], [want])


def test_weight_two_doubles_exactly_and_a_second_call_gives_the_same_bits():
    for c in (EXACT, rc.sweep_case(130, 768, 0.01), rc.FOUR_WAVES[0]):
        one = run(c.e, c.tau)
        assert _same_bits(run(c.e, c.tau), one), c
        out, d = run(c.e, c.tau, weight=2.0)
        assert _same_bits([out[0], out[1:], d], [2 * one[0][0], one[0][1:], 2 * one[1]]), c


# ---- 3. zero and non-finite rows, as the header states them -----------------------------------------------------------------------------
def _spoil(e, key, row, how):
    e = dict(e)
    e[key] = e[key].clone()
    if how == 'zero':
        e[key][row] = 0.0
    else:
        e[key][row, 5] = math.nan if how == 'nan' else math.inf
    return e


@pytest.mark.parametrize('how', ['zero', 'nan', 'inf'])
def test_zero_and_non_finite_rows_follow_the_header(how):
    for c in (EXACT, rc.sweep_case(2, 48, 0.07), rc.sweep_case(130, 48, 2.0)):
        for key, row in (('s', c.B - 1), ('t', 0), ('s', 0), ('t', c.B // 2)):
            out, d = run(_spoil(c.e, key, row, how), c.tau)               # run() asserts out[3] is +0
            assert torch.isnan(d).all() and torch.isnan(out[:3]).all(), (c, key, row, how, out)
    # B = 1: no statistic is read.  out is zeros; a spoilt student row gives 0 * NaN in the product, a spoilt teacher row is never used
    c = rc.sweep_case(1, 48, 0.07)
    out, d = run(_spoil(c.e, 's', 0, how), c.tau)
    assert (out == 0).all() and torch.isnan(d).all()
    out, d = run(_spoil(c.e, 't', 0, how), c.tau)
    assert (out == 0).all() and (d == 0).all()


# ---- 4. the Python layer ---------------------------------------------------------------------------------------------------------------
def _rep(x, grad):
    return types.SimpleNamespace(last_representation=x.clone().to(DEV).requires_grad_(grad))


def _two(e, grad):
    return (types.SimpleNamespace(visual_output=_rep(e['si'], grad), text_output=_rep(e['st'], grad)),
            types.SimpleNamespace(visual_output=_rep(e['ti'], False), text_output=_rep(e['tt'], False)))


def _four(B, E, seed):
    a, b = rc._draw(B, E, seed), rc._draw(B, E, seed + 1)
    return dict(si=a['s'], ti=a['t'], st=b['s'], tt=b['t'])


def _intra_f64(s, t, tau):
    F = torch.nn.functional
    B = s.shape[0]
    keep = ~torch.eye(B, dtype=torch.bool)
    rows = lambda x: (F.normalize(x, dim=1, eps=0) @ F.normalize(x, dim=1, eps=0).T / tau)[keep].view(B, B - 1)
    return tau * tau * F.kl_div(F.log_softmax(rows(s), 1), F.log_softmax(rows(t), 1), reduction='batchmean', log_target=True)


def _restatement(e, names, scale, percent, tau, two):
    """float64: total, every dict entry, gradients at the student embeddings (oracle/loss.py's term functions, intra_kl by kl_div)"""
    from oracle import loss as ol
    F = torch.nn.functional
    x = {k: v.to(rc.F64) for k, v in e.items()}
    a, p = x['si'].requires_grad_(True), x['ti']
    b, q = (x['st'].requires_grad_(True), x['tt']) if two else (None, None)
    nz = lambda t: F.normalize(t, dim=1, eps=0)
    tower = dict(out_l1=ol.out_l1, out_cos=ol.out_cos, intra_kl=lambda s, t: _intra_f64(s, t, tau))
    res, total = {}, 0
    for n in names:
        if n in tower and two:
            res['image_' + n], res['text_' + n] = tower[n](a, p) * scale[n], tower[n](b, q) * scale[n]
            total = total + 0.5 * percent[n] * (res['image_' + n] + res['text_' + n])
        elif n in tower:
            res[n] = tower[n](a, p) * scale[n]
            total = total + percent[n] * res[n]
        elif n == 'soft_label':
            S, T = nz(a) @ nz(b).T, nz(p) @ nz(q).T
            res[n] = 0.5 * (ol.kl_sum(S, T, tau) + ol.kl_sum(S.T, T.T, tau)) * scale[n]
            total = total + percent[n] * res[n]
    total.backward()
    return total.detach(), {k: v.detach() for k, v in res.items()}, a.grad, b.grad if two else None


def _rel(a, b):
    return (a.cpu().to(rc.F64) - b).abs().max().item() / (b.abs().max().item() + 1e-300)


@pytest.mark.parametrize('autocast', [False, True])
@pytest.mark.parametrize('names,two', [(['out_l1', 'intra_kl'], False), (['out_cos', 'intra_kl', 'soft_label'], True), (['intra_kl'], False)],
                         ids=['one-tower', 'two-towers', 'alone'])
def test_loss_calculator_against_the_float64_restatement(names, two, autocast):
    """total, every dict entry and the gradients at the student embeddings against the float64 restatement, to the tolerances
    tests/test_loss_gpu.py holds the fused kernel's mixtures to (3e-5 of max(1, |value|); 2e-4 of the largest gradient element)"""
    from distillclip_amd import ops
    from distillclip_amd.model import LossCalculator
    tau = 0.07
    lc = LossCalculator(names, {'intra_kl': 0.5}, temperature=tau)
    e = _four(40, 64, 77)
    stu, tea = _two(e, True)
    so, to = (stu, tea) if two else (stu.visual_output, tea.visual_output)
    with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
        loss, res = lc(so, to, 'all' if two else 'image')
    loss.backward()
    total, want, ga, gb = _restatement(e, names, lc.loss_scale, lc.percent, tau, two)
    assert set(res) == set(want)
    assert ('image_intra_kl' in res and 'text_intra_kl' in res) if two else 'intra_kl' in res
    assert abs(loss.item() - total.item()) <= 3e-5 * max(1.0, abs(total.item())), (loss.item(), total.item())
    for k, v in want.items():
        assert abs(res[k].item() - v.item()) <= 3e-5 * max(1.0, abs(v.item())), (k, res[k].item(), v.item())
    assert _rel(stu.visual_output.last_representation.grad, ga) < 2e-4
    if two:
        assert _rel(stu.text_output.last_representation.grad, gb) < 2e-4
    # the term's logged value against the direct kernel call, bit for bit
    g = {k: v.to(DEV) for k, v in e.items()}
    out, _ = ops.relation_kl(g['si'], g['ti'], tau, 0.5 / len(names))
    assert _same_bits([res['image_intra_kl' if two else 'intra_kl']], [out[1] * 0.5])


def test_a_calculator_without_the_name_never_reaches_the_new_entry(monkeypatch):
    from distillclip_amd.model import LossCalculator, _loss

    def boom(*a, **k):
        raise AssertionError('ops.relation_kl was called')
    monkeypatch.setattr(_loss.ops, 'relation_kl', boom)
    e = _four(17, 48, 79)
    stu, tea = _two(e, True)
    loss, res = LossCalculator(['out_l1', 'out_cos', 'cos_diff', 'soft_label', 'out_mse', 'icl'], temperature=0.5)(stu, tea, 'all')
    loss.backward()
    assert torch.isfinite(loss) and not any('intra_kl' in k for k in res)
    loss, res = LossCalculator(['out_l1', 'out_cos', 'out_mse'])(stu.visual_output, tea.visual_output, 'image')
    assert torch.isfinite(loss) and set(res) == {'out_l1', 'out_cos', 'out_mse'}
    for args in ((stu, tea, 'all'), (stu.visual_output, tea.visual_output, 'image')):
        with pytest.raises(AssertionError, match='ops.relation_kl was called'):
            LossCalculator(['out_l1', 'intra_kl'], temperature=0.5)(*args)


def test_ops_refuses_a_shape_the_kernel_cannot_take():
    from distillclip_amd import ops
    x = torch.randn(4, 40, device=DEV)
    with pytest.raises(ValueError, match='E % 16 == 0'):
        ops.relation_kl(x, x, 0.07)
    y = torch.randn(4, 48, device=DEV)
    with pytest.raises(ValueError, match='tau'):
        ops.relation_kl(y, y, 0.0)
    with pytest.raises(ValueError, match='one shape'):
        ops.relation_kl(y, y[:3], 0.07)
    with pytest.raises(ValueError, match='contiguous f32'):
        ops.relation_kl(y.half(), y.half(), 0.07)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def _tiny_batch(B):
    from test_towers_gpu import TINY
    from distillclip_amd import synth
    image = torch.from_numpy(synth.images(TINY['seed'], B, TINY['res'])).cuda()
    text = torch.from_numpy(synth.captions(TINY['seed'], B, TINY['ctx'], TINY['vocab'], 3, 9)).cuda()
    return image, text


def _assert_grads(*modules):
    for m in modules:
        for n, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, n


def test_one_training_step_of_the_tiny_two_tower_model_with_intra_kl():
    from test_towers_gpu import _tiny_modules
    from distillclip_amd import ops
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model.component import CLIPModel
    s_img, s_txt, t_img, t_txt = _tiny_modules()
    student, teacher = CLIPModel(True, s_img, s_txt), CLIPModel(False, t_img, t_txt)
    for p in teacher.parameters():
        p.requires_grad = False
    lc = LossCalculator(['out_cos', 'intra_kl', 'soft_label'], temperature=0.07)
    image, text = _tiny_batch(4)
    so = student(text, image, lc.get_control_output())
    to = teacher(text, image, lc.get_control_output())
    loss, res = lc(so, to, 'all')
    assert torch.isfinite(loss)
    f = lambda o: o.last_representation.detach().float().contiguous()
    for key, s, t in (('image_intra_kl', so.visual_output, to.visual_output), ('text_intra_kl', so.text_output, to.text_output)):
        out, _ = ops.relation_kl(f(s), f(t), 0.07)
        assert _same_bits([res[key]], [out[1]]) and out[1].item() > 0, key
    loss.backward()
    _assert_grads(s_img, s_txt)


def test_one_training_step_of_the_tiny_one_tower_model_with_intra_kl():
    from test_towers_gpu import _tiny_modules
    from distillclip_amd import ops
    from distillclip_amd.model import LossCalculator
    s_img, _, t_img, _ = _tiny_modules()
    for p in t_img.parameters():
        p.requires_grad = False
    lc = LossCalculator(['out_l1', 'out_cos', 'intra_kl'], temperature=0.07)
    image, _ = _tiny_batch(4)
    so, to = s_img(image, lc.get_control_output()), t_img(image, lc.get_control_output())
    loss, res = lc(so, to, 'image')
    assert torch.isfinite(loss) and set(res) == {'out_l1', 'out_cos', 'intra_kl'}
    f = lambda o: o.last_representation.detach().float().contiguous()
    out, _ = ops.relation_kl(f(so), f(to), 0.07)
    assert _same_bits([res['intra_kl']], [out[1]]) and out[1].item() > 0
    loss.backward()
    _assert_grads(s_img)


# ---- last: the figures for DESIGN.md ---------------------------------------------------------------------------------------------------
def test_zz_report_worst_ratios():
    print('\nintra_kl worst err / bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
    assert all(v <= 1 for v in WORST.values()), WORST
