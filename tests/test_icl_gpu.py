"""dclip_interactive_loss (the `icl` term) element by element against float64, its exact symmetries, its memory contract, and the two
new LossCalculator names up to one training step.  Inputs, reference and bounds: tests/icl_cases.py (its docstring derives every bound;
tests/test_icl_cpu.py checks them without the kernel).  Every kernel call of this file runs on inputs surrounded by NaNs, with outputs
between sentinels and a workspace of exactly the queried size in front of a patterned guard.

Measured on an MI355X, worst err / bound over all 96 cases (printed by the last test of this file, also in DESIGN.md section 7.0):
gradients 0.039, scalars 0.038.  The float32 evaluation on the CPU uses at most 0.049 of a bound.  The whole file: 121 tests in 4 s."""
import math
import types

import pytest
import torch

import icl_cases as ic

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
    """exactly dclip_interactive_loss_workspace(B, E) bytes at a 256-byte-aligned offset of a patterned buffer, WS_GUARD bytes behind"""

    def __init__(self, B, E):
        self.bytes = _lib().dclip_interactive_loss_workspace(B, E)
        assert self.bytes > 0
        n = 512 + self.bytes + WS_GUARD
        self.buf = ((torch.arange(n, device=DEV, dtype=torch.int32) * 37 + 11) % 251).to(torch.uint8)
        self.off = (-self.buf.data_ptr()) % 256 + 256
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + self.off

    def foreign_changed(self):
        end = self.off + self.bytes
        return int((self.buf[:self.off] != self.before[:self.off]).sum()) + int((self.buf[end:] != self.before[end:]).sum())


def run(e, tau, weight=1.0, order=ic.KEYS):
    """one guarded call -> (out [4], d of the first student tensor, d of the second), f32 on the CPU; asserts the memory contract.
    `order`: the keys of e passed as (s_img, t_img, s_txt, t_txt)."""
    B, E = e['si'].shape
    ins = [_Slot(B * E, e[k]) for k in order]
    d = [_Slot(B * E), _Slot(B * E)]
    out = _Slot(4)
    ws = _Workspace(B, E)
    _lib().dclip_interactive_loss(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, B, E, tau, weight, out.ptr, d[0].ptr, d[1].ptr,
                                  ws.ptr, ws.bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bad = [f'input {k}: {s.foreign_changed(False)} floats changed' for k, s in zip(order, ins) if s.foreign_changed(False)]
    bad += [f'{n}: {s.foreign_changed(True)} floats changed outside what the call owns'
            for n, s in (('d_s_img', d[0]), ('d_s_txt', d[1]), ('out', out)) if s.foreign_changed(True)]
    if ws.foreign_changed():
        bad.append(f'workspace: {ws.foreign_changed()} guard bytes changed around its {ws.bytes} bytes')
    assert not bad, bad
    return out.owned().cpu(), d[0].owned().view(B, E).cpu(), d[1].owned().view(B, E).cpu()


def _bits(*ts):
    return [t.contiguous().view(torch.int32) for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


def _worst(what, q):
    WORST[what] = max(WORST.get(what, 0.0), q)


def _check(ref, got, label):
    """every element of both gradients and the four scalars within the bounds; -> the failures"""
    out, d0, d1 = got
    fails = []
    for name, g, want, bound in (('d_s_img', d0, ref.g[0], ref.gb[0]), ('d_s_txt', d1, ref.g[1], ref.gb[1])):
        q = ic.ratio((g.to(ic.F64) - want).abs(), bound)
        _worst('gradient', q)
        if not q <= 1:
            fails.append(f'{label} {name}: err / bound = {q:.3g}')
    for i, name in enumerate(('weight * icl', 'icl', 'L_i2t', 'L_t2i')):
        q = ic.ratio((out[i].to(ic.F64) - ref.out[i]).abs().reshape(1), ref.out_b[i].reshape(1))
        _worst('scalar', q)
        if not q <= 1:
            fails.append(f'{label} {name}: {out[i].item()!r} against {ref.out[i].item()!r}, err / bound = {q:.3g}')
    return fails


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ic.CASES, ids=repr)
def test_every_element_against_float64(case):
    fails = _check(case.ref, run(case.e, case.tau), repr(case))
    assert not fails, fails


def test_one_text_row_gives_log_b():
    c = ic.ONE_TEXT
    out, _, _ = run(c.e, c.tau)
    assert abs(out[2].item() - math.log(c.B)) <= c.ref.out_b[2].item()


def test_joint_permutation_of_the_samples_permutes_the_gradient_rows():
    """within the bound, not bit for bit: the rows change stripes and the columns change slices, so every merge order changes"""
    for c in (ic.SWEEP_CASES[ic.SWEEP.index((130, 768)) * 3], ic.SWEEP_CASES[ic.SWEEP.index((33, 48)) * 3 + 1]):
        perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
        e = {k: v[perm].contiguous() for k, v in c.e.items()}
        out, d0, d1 = run(e, c.tau)
        ref = c.ref
        fails = []
        for name, g, d in (('d_s_img', d0, 0), ('d_s_txt', d1, 1)):
            q = ic.ratio((g.to(ic.F64) - ref.g[d][perm]).abs(), ref.gb[d][perm])
            if not q <= 1:
                fails.append(f'{c} {name}: err / bound = {q:.3g}')
        q = ic.ratio((out.to(ic.F64) - ref.out).abs(), ref.out_b)
        assert not fails and q <= 1, (fails, q)


# ---- 2. exact, no tolerance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [16, 48, 768])
@pytest.mark.parametrize('tau', ic.TAUS)
def test_batch_of_one_is_exactly_zero(E, tau):
    e = ic._draw(1, E, 5)
    out, d0, d1 = run(e, tau, weight=3.0)
    assert (out == 0).all() and (d0 == 0).all() and (d1 == 0).all(), (out, d0.abs().max(), d1.abs().max())


EXACT = ic.SWEEP_CASES[ic.SWEEP.index((33, 48)) * 3 + 1]          # B = 33, E = 48, tau = 0.07: three stripes, three slices


@pytest.mark.parametrize('k', [-30, 7, 30])
def test_scaling_a_student_row_by_a_power_of_two(k):
    c, row = EXACT, 18
    base = run(c.e, c.tau)
    for key, which in (('si', 1), ('st', 2)):
        e = dict(c.e)
        e[key] = c.e[key].clone()
        e[key][row] *= 2.0 ** k
        got = run(e, c.tau)
        assert _same_bits([got[0]], [base[0]])
        want = [base[1].clone(), base[2].clone()]
        want[which - 1][row] *= 2.0 ** -k
        assert _same_bits(got[1:], want), key


def test_scaling_teacher_rows_by_powers_of_two_changes_no_bit():
    c = EXACT
    base = run(c.e, c.tau)
    e = dict(c.e)
    for key in ('ti', 'tt'):
        s = 2.0 ** torch.randint(-30, 31, (c.B,), generator=torch.Generator().manual_seed(3)).float()
        e[key] = (c.e[key] * s[:, None]).contiguous()
    assert _same_bits(run(e, c.tau), base)


def test_swapping_the_modalities_swaps_the_outputs_bit_for_bit():
    for c in (EXACT, ic.SWEEP_CASES[ic.SWEEP.index((130, 768)) * 3]):
        out, d0, d1 = run(c.e, c.tau)
        sout, s0, s1 = run(c.e, c.tau, order=('st', 'tt', 'si', 'ti'))
        assert _same_bits([sout[0], sout[1], sout[2], sout[3], s0, s1], [out[0], out[1], out[3], out[2], d1, d0]), c


def test_weight_two_doubles_exactly_and_a_second_call_gives_the_same_bits():
    for c in (EXACT, ic.SWEEP_CASES[ic.SWEEP.index((130, 768)) * 3]):
        one = run(c.e, c.tau)
        assert _same_bits(run(c.e, c.tau), one), c
        out, d0, d1 = run(c.e, c.tau, weight=2.0)
        assert _same_bits([out[0], out[1:], d0, d1], [2 * one[0][0], one[0][1:], 2 * one[1], 2 * one[2]]), c


# ---- 3. zero and non-finite rows, as the header states them -----------------------------------------------------------------------------
def test_zero_and_non_finite_rows_follow_the_header():
    c = EXACT
    fin = lambda t: torch.isfinite(t).all()
    for how in ('zero', 'nan', 'inf'):
        def spoil(key, row):
            e = dict(c.e)
            e[key] = c.e[key].clone()
            if how == 'zero':
                e[key][row] = 0.0
            else:
                e[key][row, 5] = math.nan if how == 'nan' else math.inf
            return e
        # a student image row: its own gradient row and its direction's scalars, nothing else
        out, d0, d1 = run(spoil('si', 18), c.tau)
        keep = torch.arange(c.B) != 18
        assert torch.isnan(d0[18]).all() and fin(d0[keep]) and fin(d1), how
        assert torch.isnan(out[:3]).all() and fin(out[3]), (how, out)
        # a teacher text row: every logit of its column in A, so all of d_s_img; C and d_s_txt never see it
        out, d0, d1 = run(spoil('tt', 2), c.tau)
        assert torch.isnan(d0).all() and fin(d1) and torch.isnan(out[:3]).all() and fin(out[3]), (how, out)
        # the text side
        out, d0, d1 = run(spoil('st', 32), c.tau)
        keep = torch.arange(c.B) != 32
        assert torch.isnan(d1[32]).all() and fin(d1[keep]) and fin(d0) and torch.isnan(out[[0, 1, 3]]).all() and fin(out[2]), (how, out)
        out, d0, d1 = run(spoil('ti', 0), c.tau)
        assert torch.isnan(d1).all() and fin(d0) and torch.isnan(out[[0, 1, 3]]).all() and fin(out[2]), (how, out)


# ---- 4. the Python layer ---------------------------------------------------------------------------------------------------------------
def _outputs(e, grad):
    rep = lambda x, g: types.SimpleNamespace(last_representation=x.clone().to(DEV).requires_grad_(g))
    two = lambda i, t, g: types.SimpleNamespace(visual_output=rep(e[i], g), text_output=rep(e[t], g))
    return two('si', 'st', grad), two('ti', 'tt', False)


def _restatement(e, names, scale, percent, tau):
    """float64: total, every dict entry, gradients at the two student embeddings (oracle/loss.py's term functions, ICL by cross_entropy)"""
    from oracle import loss as ol
    F = torch.nn.functional
    x = {k: v.to(ic.F64) for k, v in e.items()}
    a, b = x['si'].requires_grad_(True), x['st'].requires_grad_(True)
    p, q = x['ti'], x['tt']
    nz = lambda t: F.normalize(t, dim=1, eps=0)
    res, total = {}, 0
    tower = dict(out_l1=ol.out_l1, out_mse=ol.mse)
    for n in names:
        if n in tower:
            res['image_' + n], res['text_' + n] = tower[n](a, p) * scale[n], tower[n](b, q) * scale[n]
            total = total + 0.5 * percent[n] * (res['image_' + n] + res['text_' + n])
        elif n == 'soft_label':
            S, T = nz(a) @ nz(b).T, nz(p) @ nz(q).T
            res[n] = 0.5 * (ol.kl_sum(S, T, tau) + ol.kl_sum(S.T, T.T, tau)) * scale[n]
            total = total + percent[n] * res[n]
        elif n == 'icl':
            lab = torch.arange(a.shape[0])
            res[n] = 0.5 * (F.cross_entropy(nz(a) @ nz(q).T / tau, lab) + F.cross_entropy(nz(b) @ nz(p).T / tau, lab)) * scale[n]
            total = total + percent[n] * res[n]
    total.backward()
    return total.detach(), {k: v.detach() for k, v in res.items()}, a.grad, b.grad


def _rel(a, b):
    return (a.cpu().to(ic.F64) - b).abs().max().item() / (b.abs().max().item() + 1e-300)


@pytest.mark.parametrize('autocast', [False, True])
def test_loss_calculator_with_the_clip_kd_recipe(autocast):
    """total, every dict entry and the gradients at the student embeddings against the float64 restatement, to the tolerances
    tests/test_loss_gpu.py holds the fused kernel's mixtures to (3e-5 of max(1, |value|); 2e-4 of the largest gradient element)"""
    from distillclip_amd.model import LossCalculator
    names = ['out_l1', 'out_mse', 'icl', 'soft_label']
    lc = LossCalculator(names, {'icl': 0.5}, temperature=0.07)
    e = ic._draw(40, 64, 77)
    stu, tea = _outputs(e, True)
    with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
        loss, res = lc(stu, tea, 'all')
    loss.backward()
    total, want, ga, gb = _restatement(e, names, lc.loss_scale, lc.percent, 0.07)
    assert set(res) == set(want) == {'image_out_l1', 'text_out_l1', 'image_out_mse', 'text_out_mse', 'icl', 'soft_label'}
    assert abs(loss.item() - total.item()) <= 3e-5 * max(1.0, abs(total.item())), (loss.item(), total.item())
    for k, v in want.items():
        assert abs(res[k].item() - v.item()) <= 3e-5 * max(1.0, abs(v.item())), (k, res[k].item(), v.item())
    assert _rel(stu.visual_output.last_representation.grad, ga) < 2e-4 and _rel(stu.text_output.last_representation.grad, gb) < 2e-4
    # the term's own share against the direct kernel call: the logged value bit for bit
    from distillclip_amd import ops
    g = {k: v.to(DEV) for k, v in e.items()}
    out, _, _ = ops.interactive_loss(g['si'], g['ti'], g['st'], g['tt'], 0.07, 0.5 * 0.25)
    assert _same_bits([res['icl']], [out[1] * 0.5])


def test_out_mse_alone_in_one_tower_mode():
    from distillclip_amd.model import LossCalculator
    e = ic._draw(17, 48, 78)
    lc = LossCalculator(['out_mse', 'icl'], temperature=0.07)          # one tower: icl is ignored, out_mse keeps its percent
    s = types.SimpleNamespace(last_representation=e['si'].clone().to(DEV).requires_grad_(True))
    t = types.SimpleNamespace(last_representation=e['ti'].to(DEV))
    loss, res = lc(s, t, 'image')
    loss.backward()
    a, p = e['si'].to(ic.F64), e['ti'].to(ic.F64)
    want = ((a - p) ** 2).mean()
    assert set(res) == {'out_mse'}
    assert abs(res['out_mse'].item() - want.item()) <= 3e-5 * max(1.0, want.item())
    assert abs(loss.item() - 0.5 * want.item()) <= 3e-5 * max(1.0, want.item())
    assert _rel(s.last_representation.grad, 0.5 * 2 * (a - p) / a.numel()) < 2e-4


def test_a_calculator_without_icl_never_reaches_the_new_entry(monkeypatch):
    from distillclip_amd.model import LossCalculator, _loss

    def boom(*a, **k):
        raise AssertionError('ops.interactive_loss was called')
    monkeypatch.setattr(_loss.ops, 'interactive_loss', boom)
    e = ic._draw(17, 48, 79)
    stu, tea = _outputs(e, True)
    loss, res = LossCalculator(['out_l1', 'out_cos', 'cos_diff', 'soft_label', 'out_mse'], temperature=0.5)(stu, tea, 'all')
    loss.backward()
    assert torch.isfinite(loss) and 'icl' not in res
    with pytest.raises(AssertionError, match='ops.interactive_loss was called'):
        LossCalculator(['out_l1', 'icl'], temperature=0.5)(stu, tea, 'all')


def test_ops_refuses_a_shape_the_kernel_cannot_take():
    from distillclip_amd import ops
    x = torch.randn(4, 40, device=DEV)
    with pytest.raises(ValueError, match='E % 16 == 0'):
        ops.interactive_loss(x, x, x, x, 0.07)
    y = torch.randn(4, 48, device=DEV)
    with pytest.raises(ValueError, match='tau'):
        ops.interactive_loss(y, y, y, y, 0.0)
    with pytest.raises(ValueError, match='one shape'):
        ops.interactive_loss(y, y, y[:3], y, 0.07)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def test_one_training_step_of_the_tiny_two_tower_model_with_icl():
    from test_towers_gpu import TINY, _tiny_modules
    from distillclip_amd import ops, synth
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model.component import CLIPModel
    s_img, s_txt, t_img, t_txt = _tiny_modules()
    student, teacher = CLIPModel(True, s_img, s_txt), CLIPModel(False, t_img, t_txt)
    for p in teacher.parameters():
        p.requires_grad = False
    lc = LossCalculator(['out_cos', 'out_mse', 'icl'], temperature=0.07)
    B = 4
    image = torch.from_numpy(synth.images(TINY['seed'], B, TINY['res'])).cuda()
    text = torch.from_numpy(synth.captions(TINY['seed'], B, TINY['ctx'], TINY['vocab'], 3, 9)).cuda()
    so = student(text, image, lc.get_control_output())
    to = teacher(text, image, lc.get_control_output())
    loss, res = lc(so, to, 'all')
    assert torch.isfinite(loss)
    f = lambda o: o.last_representation.detach().float().contiguous()
    out, _, _ = ops.interactive_loss(f(so.visual_output), f(to.visual_output), f(so.text_output), f(to.text_output), 0.07)
    assert _same_bits([res['icl']], [out[1]])
    loss.backward()
    for n, p in list(s_img.named_parameters()) + list(s_txt.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, n


# ---- last: the figures for DESIGN.md ---------------------------------------------------------------------------------------------------
def test_zz_report_worst_ratios():
    print('\nicl worst err / bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
    assert all(v <= 1 for v in WORST.values()), WORST
