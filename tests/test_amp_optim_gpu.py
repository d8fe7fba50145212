"""FusedAdamW driven by torch.amp.GradScaler.step() (`precision: 16`): dclip_amp_prepare + dclip_adamw_multi_amp (csrc/optim.hip) and the
protocol on top of them (optim.py: _step_supports_amp_scaling, grad_scale / found_inf, param_groups).

Kernel level: three ranges of 4, 1028 and 4100 elements (one lane-load, a row of 1024 plus one load, four rows plus one load: the grid has
several workgroups per range and a last one that is partly idle), every range with 4 guard words before and after it in each of the four
buffers.  Bounds: bit equality wherever the arithmetic is the same arithmetic (a scale of 2^16 only moves exponents), and for the norm the
bound in the header of tests/test_grad_clip_gpu.py, 0.5 * (L + 64) * 2^-24 + 2^-24 with L = 8.

End to end: the tiny dual model of tests/test_amp_gpu.py against a twin stepped by FusedAdamW without scaler or autocast: 2e-5 max-abs per
trainable tensor after three steps at lr 1e-3 (the bound tests/test_amp_gpu.py::test_fused_adamw_consumes_gradients_that_went_through_autograd
holds two runs with the same atomic-ordering noise to) and 1e-5 relative on last_grad_norm (tests/test_grad_clip_gpu.py's)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from distillclip_amd import synth

pytestmark = pytest.mark.gpu

LENS = [4, 1028, 4100]
NORM_BOUND = 0.5 * (8 + 64) * 2.0 ** -24 + 2.0 ** -24
SCALE = 65536.0
HYPER = (3e-3, (0.9, 0.999), 1e-8, 1e-2)                       # lr, betas, eps, weight decay


def _ops():
    from distillclip_amd import ops
    assert ops.AMP_RECORD_FLOATS == 8 and ops.SUMSQ_PARTIALS == 1024
    return ops


class _Buffers:
    """p, g, m, v: one buffer each, 4 guard words | range 0 | 4 guard words | range 1 | ... | 4 guard words, random everywhere"""

    def __init__(self, seed, g_scale=1.0):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        total = 4 + sum(n + 4 for n in LENS)
        self.p, self.g, self.m = (torch.randn(total, device='cuda', generator=gen) for _ in range(3))
        self.v = torch.randn(total, device='cuda', generator=gen).abs()
        self.g *= g_scale
        self.spans, at = [], 4
        for n in LENS:
            self.spans.append((at, at + n))
            at += n + 4
        self.inside = torch.zeros(total, dtype=torch.bool, device='cuda')
        for a, b in self.spans:
            self.inside[a:b] = True

    def clone(self, g=None):
        c = object.__new__(_Buffers)
        c.spans, c.inside = self.spans, self.inside
        c.p, c.m, c.v = self.p.clone(), self.m.clone(), self.v.clone()
        c.g = (self.g if g is None else g).clone()
        return c

    def items(self):
        return [(self.p[a:b], self.g[a:b], self.m[a:b], self.v[a:b]) for a, b in self.spans]

    def grads(self):
        return [self.g[a:b] for a, b in self.spans]


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _one(x, dtype=torch.float32):
    return torch.tensor([x], dtype=dtype, device='cuda')


def _amp_step(buf, step, zero_grad, skipped, record, found_inf=None, grad_scale=None, max_norm=None):
    """the new pair on buf: [sums ->] dclip_amp_prepare -> dclip_adamw_multi_amp"""
    ops = _ops()
    parts = None
    if max_norm is not None:
        parts = torch.full((ops.SUMSQ_PARTIALS,), float('nan'), device='cuda')
        ops.sumsq_multi(buf.grads(), parts)
    ops.amp_prepare(record, skipped, HYPER[1], step, found_inf, grad_scale, parts, 0.0 if max_norm is None else max_norm)
    ops.adamw_multi_amp(buf.items(), *HYPER, zero_grad, record)


def _scaled_step(buf, step, zero_grad, max_norm=None):
    """the kernels of a step without a scaler: [sums -> dclip_clip_coef ->] dclip_adamw_multi_scaled; -> out (norm, coef) or None"""
    ops = _ops()
    out = None
    if max_norm is not None:
        parts = torch.full((ops.SUMSQ_PARTIALS,), float('nan'), device='cuda')
        out = torch.full((2,), float('nan'), device='cuda')
        ops.sumsq_multi(buf.grads(), parts)
        ops.clip_coef(parts, max_norm, out)
    ops.adamw_multi_scaled(buf.items(), *HYPER, step, zero_grad, None if out is None else out[1:2])
    return out


def _check_gradients(buf, before_g, zero_grad):
    """inside the ranges cleared or untouched, the guard words untouched"""
    want = torch.where(buf.inside, torch.zeros_like(before_g), before_g) if zero_grad else before_g
    assert _same(buf.g, want)


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('step', [1, 7])
@pytest.mark.parametrize('clip', [False, True])
def test_a_unscaling_in_the_kernel_equals_the_scaled_kernel_on_predivided_gradients(clip, step, zero_grad):
    """grad_scale = 65536: p, m, v (guard words included) bit-equal to dclip_adamw_multi_scaled on g / 65536 divided on the host, where
    the division is exact; clip: a threshold of half the norm, so that the coefficient bites"""
    ops = _ops()
    src = _Buffers(21, g_scale=SCALE)                          # gradients as a backward under the scaler leaves them
    divided = (src.g.cpu() / SCALE).cuda()
    assert _same(divided * SCALE, src.g)                       # (exact both ways)
    ref_buf, new_buf = src.clone(divided), src.clone()
    max_norm = None
    if clip:
        max_norm = 0.5 * float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in ref_buf.grads())))
    out = _scaled_step(ref_buf, step, zero_grad, max_norm)
    record, skipped = torch.full((8,), float('nan'), device='cuda'), _one(0, torch.int64)
    _amp_step(new_buf, step, zero_grad, skipped, record, _one(0.0), _one(SCALE), max_norm)
    torch.cuda.synchronize()
    for name in 'pmv':
        assert _same(getattr(new_buf, name), getattr(ref_buf, name)), name
    assert float((new_buf.p - src.p).abs().max()) > 0          # (the step was taken)
    _check_gradients(new_buf, src.g, zero_grad)
    rec = record.cpu().numpy()
    assert int(skipped) == 0 and rec[ops.AMP_SKIP] == 0.0 and rec[6] == 0.0 and rec[7] == 0.0
    if clip:
        norm, coef = out.cpu().numpy()
        print(f'norm: record {rec[ops.AMP_NORM]:.9e}, scaled path {norm:.9e}, |d| / norm = {abs(rec[ops.AMP_NORM] - norm) / norm:.3e} '
              f'(bound {NORM_BOUND:.3e}); coef {rec[ops.AMP_COEF]:.9e} / {coef:.9e}')
        assert abs(float(rec[ops.AMP_NORM]) - float(norm)) <= NORM_BOUND * float(norm)
        assert coef < 0.6 and rec[ops.AMP_MULT] == np.float32(rec[ops.AMP_COEF]) / np.float32(SCALE)
    else:
        assert rec[ops.AMP_NORM] == 0.0 and rec[ops.AMP_COEF] == 1.0 and rec[ops.AMP_MULT] == np.float32(1.0 / SCALE)


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('clip', [False, True])
def test_b_a_skipped_step_writes_nothing(clip, zero_grad):
    """found_inf = 1, the gradients holding an inf and a NaN: p, m, v and every guard word byte-identical before and after, g zero if and
    only if zero_grad is set, skipped one higher"""
    ops = _ops()
    src = _Buffers(22, g_scale=SCALE)
    src.g[src.spans[1][0] + 5] = float('inf')
    src.g[src.spans[2][1] - 1] = float('nan')
    buf = src.clone()
    record, skipped = torch.full((8,), float('nan'), device='cuda'), _one(3, torch.int64)
    _amp_step(buf, 9, zero_grad, skipped, record, _one(1.0), _one(SCALE), 1.0 if clip else None)
    torch.cuda.synchronize()
    for name in 'pmv':
        assert _same(getattr(buf, name), getattr(src, name)), name
    _check_gradients(buf, src.g, zero_grad)
    assert int(skipped) == 4 and float(record[ops.AMP_SKIP]) == 1.0


def test_c_bias_correction_does_not_advance_on_a_skip():
    """host steps 1, 2, 3 with the second skipped = dclip_adamw_multi with steps 1 and 2 on the first and the third gradients, bit for bit"""
    ops = _ops()
    src = _Buffers(23)
    gen = torch.Generator(device='cuda').manual_seed(24)
    grads = [torch.randn(src.g.numel(), device='cuda', generator=gen) for _ in range(3)]
    ref_buf, new_buf = src.clone(), src.clone()
    for step, k in ((1, 0), (2, 2)):
        ref_buf.g.copy_(grads[k])
        ops.adamw_multi_scaled(ref_buf.items(), *HYPER, step, False, None)      # (gscale None: dclip_adamw_multi itself)
    record, skipped = torch.full((8,), float('nan'), device='cuda'), _one(0, torch.int64)
    for step, k in ((1, 0), (2, 1), (3, 2)):
        new_buf.g.copy_(grads[k])
        _amp_step(new_buf, step, False, skipped, record, _one(1.0 if k == 1 else 0.0))
    torch.cuda.synchronize()
    for name in 'pmv':
        assert _same(getattr(new_buf, name), getattr(ref_buf, name)), name
    assert int(skipped) == 1 and _same(new_buf.g, grads[2])


def test_d_refusals_on_the_host_before_any_launch():
    from distillclip_amd._lib import lib
    src = _Buffers(25)
    buf = src.clone()
    record, skipped = torch.full((8,), 7.0, device='cuda'), _one(0, torch.int64)
    parts = torch.zeros(1024, device='cuda')
    n_ranges = len(LENS)
    arr = lambda k, shift=0: (ctypes.c_void_p * 25)(*([it[k].data_ptr() + shift for it in buf.items()] + [buf.items()[0][k].data_ptr()] * (25 - n_ranges)))
    lens = lambda *l: (ctypes.c_int64 * 25)(*(list(l) + [4] * (25 - len(l))))
    call = lambda count=n_ranges, rec=record.data_ptr(), g=None, n=None: lib().dclip_adamw_multi_amp(
        arr(0), arr(1) if g is None else g, arr(2), arr(3), lens(*LENS) if n is None else n, count, 3e-3, 0.9, 0.999, 1e-8, 1e-2, 1, rec, None)
    with pytest.raises(ValueError, match='record'):
        call(rec=None)                                         # null record
    with pytest.raises(ValueError, match='record'):
        call(rec=record.data_ptr() + 4)
    for count in (0, 25):
        with pytest.raises(ValueError, match='1..24'):
            call(count=count)
    with pytest.raises(ValueError, match='16-byte aligned'):
        call(g=arr(1, 8))                                      # a pointer off by 8 bytes
    with pytest.raises(ValueError, match='multiple of 4'):
        call(n=lens(4, 1026, 4100))
    prep = lambda **kw: lib().dclip_amp_prepare(*[kw.get(k, d) for k, d in (
        ('found_inf', None), ('grad_scale', None), ('partials', None), ('n_partials', 0), ('extra', None), ('max_norm', 1.0), ('b1', 0.9),
        ('b2', 0.999), ('step', 1), ('skipped', skipped.data_ptr()), ('record', record.data_ptr()), ('stream', None))])
    for bad in (dict(record=None), dict(record=record.data_ptr() + 4), dict(skipped=None), dict(step=0),
                dict(partials=parts.data_ptr()), dict(n_partials=1024), dict(extra=parts.data_ptr())):
        with pytest.raises(ValueError, match='dclip_amp_prepare'):
            prep(**bad)
    with pytest.raises(RuntimeError):
        _ops().amp_prepare(record.cpu(), skipped, (0.9, 0.999), 1)      # no CPU fallback
    torch.cuda.synchronize()
    assert record.tolist() == [7.0] * 8 and int(skipped) == 0
    for name in 'pgmv':
        assert _same(getattr(buf, name), getattr(src, name)), name


def _f32_power(beta, t):
    """beta^t for the f32 beta, rounded once to f32 (exact rational arithmetic)"""
    exact = Fraction(float(np.float32(beta))) ** t
    x = np.float32(float(exact))
    return min((np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))), key=lambda y: abs(Fraction(float(y)) - exact))


def test_the_records_bias_corrections_are_the_f32_formula_on_the_correctly_rounded_power():
    """bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) in f32 as dclip_adamw_multi's host code forms them, with beta^t rounded
    correctly (the kernel multiplies in double): t = step - skipped over small, odd, power-of-two and late steps, three beta pairs;
    and at the steps the tests above compare with the host's kernels (1, 2, 7) the power is the C library's powf, bit for bit"""
    ops = _ops()
    libm = ctypes.CDLL('libm.so.6')
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    cases = [(b, t, s) for b in ((0.9, 0.999), (0.9, 0.98), (0.95, 0.99))
             for t, s in [(t, 0) for t in (1, 2, 3, 7, 8, 31, 64, 100, 1000, 4097, 12345)] + [(5, 4), (1003, 3), (4, 3)]]
    records = torch.full((len(cases), 8), float('nan'), device='cuda')
    counters = torch.tensor([s for _, _, s in cases], dtype=torch.int64, device='cuda')
    for i, (betas, t, s) in enumerate(cases):
        ops.amp_prepare(records[i], counters[i:i + 1], betas, t)
    got = records.cpu().numpy()
    one = np.float32(1)
    for (betas, step, s), rec in zip(cases, got):
        t = step - s
        want1, want2 = one - _f32_power(betas[0], t), np.sqrt(one - _f32_power(betas[1], t))
        assert rec[ops.AMP_BC1].tobytes() == want1.tobytes() and rec[ops.AMP_BC2_SQRT].tobytes() == want2.tobytes(), (betas, step, s)
        assert rec[ops.AMP_MULT] == 1.0 and rec[ops.AMP_SKIP] == 0.0
        if betas == (0.9, 0.999) and step in (1, 2, 7):
            assert all(np.float32(libm.powf(np.float32(b), np.float32(t))) == _f32_power(b, t) for b in betas)
    assert counters.cpu().tolist() == [s for _, _, s in cases]


# ---- end to end: the tiny dual model of tests/test_amp_gpu.py ------------------------------------------------------------------------------
S_IMG = dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4, mlp_ratio=4.0,
             qkv_bias=True, repeated_times=2, use_transform=True)
S_TXT = dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0,
             qkv_bias=False, repeated_times=2, use_transform=True)
SEED, B = 33, 6
LOSS = dict(loss_name=['out_l1', 'out_cos', 'cos_diff'], loss_scale={'cos_diff': 0.1})
TENSOR_BOUND, NORM_REL = 2e-5, 1e-5


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _build():
    from distillclip_amd.model import DualDistillModel
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    from distillclip_amd.optim import FusedAdamW
    si, st = RepeatVisionTransformer(**S_IMG), RepeatTextTransformer(**S_TXT)
    si.load_state_dict(T(synth.student_image_state(SEED, **S_IMG)))
    st.load_state_dict(T(synth.student_text_state(SEED, **S_TXT)))
    tsd = T(synth.teacher_image_state(SEED, 128, 2, 8, 32, 64))
    tsd.update(T(synth.teacher_text_state(SEED, 128, 2, 13, 97, 64)))
    model = DualDistillModel(si, st, LOSS, 0, 10, 1e-2, 1e-3, '.', teacher_state_dict=tsd).cuda()
    (opt,), _ = model.configure_optimizers()
    assert isinstance(opt, FusedAdamW)
    opt.lr = 1e-3
    return model, opt


def _batch():
    return [torch.from_numpy(synth.images(SEED, B, 32)).cuda(), torch.from_numpy(synth.captions(SEED, B, 13, 97, 3, 9)).cuda()]


def _weights(model):
    return {n: p.detach().clone() for n, p in model.student.named_parameters() if p.requires_grad}


def _twin(max_grad_norm):
    """three plain FusedAdamW steps, no scaler, no autocast -> (weights after step 1, after step 3, last_grad_norm of each step)"""
    model, opt = _build()
    opt.max_grad_norm = max_grad_norm
    batch, norms, first = _batch(), [], None
    for i in range(3):
        opt.zero_grad()
        model.training_step(batch).backward()
        opt.step()
        norms.append(float(opt.last_grad_norm))
        if i == 0:
            first = _weights(model)
    torch.cuda.synchronize()
    return first, _weights(model), norms


@pytest.fixture(scope='module')
def twins():
    """{False: the twin that does not clip, True: the twin that clips at half its first-step norm}.  The one that does not clip runs with
    a threshold never reached, which is the unclipped step bit for bit (tests/test_grad_clip_gpu.py) and reports the norm."""
    off = _twin(1e30)
    return {False: off, True: _twin(0.5 * off[2][0])}


def _closest(got, want):
    worst = max(((got[n] - want[n]).abs().max().item(), n) for n in want)
    print(f'largest |difference| to the twin: {worst[0]:.3e} in {worst[1]} (bound {TENSOR_BOUND:.1e})')
    return worst


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('unscale_first', [False, True])
def test_three_steps_through_gradscaler_equal_the_twin(twins, unscale_first, clip):
    """autocast -> scaler.scale(loss).backward() -> [scaler.unscale_(opt) ->] scaler.step(opt) -> scaler.update(), opt from
    configure_optimizers()"""
    _, want, twin_norms = twins[clip]
    model, opt = _build()
    opt.max_grad_norm = 0.5 * twins[False][2][0] if clip else None
    scaler = torch.amp.GradScaler('cuda', init_scale=SCALE)
    batch, start = _batch(), _weights(model)
    for i in range(3):
        opt.zero_grad()
        with torch.autocast('cuda', dtype=torch.float16):
            loss = model.training_step(batch)
        scaler.scale(loss).backward()
        if unscale_first:
            scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        assert not hasattr(opt, 'grad_scale') and not hasattr(opt, 'found_inf')
        if clip:
            got = float(opt.last_grad_norm)
            print(f'step {i + 1}: last_grad_norm {got:.6e}, twin {twin_norms[i]:.6e}, relative {abs(got - twin_norms[i]) / twin_norms[i]:.3e}')
            assert abs(got - twin_norms[i]) <= NORM_REL * twin_norms[i]
        else:
            assert opt.last_grad_norm is None
    torch.cuda.synchronize()
    got = _weights(model)
    assert _closest(got, want)[0] <= TENSOR_BOUND
    assert max((got[n] - start[n]).abs().max().item() for n in got) > 1e-3      # (the weights did move: three steps at lr 1e-3)
    assert scaler.get_scale() == SCALE and opt.step_count == 3 and int(opt._skipped) == 0
    assert float(opt.state_dict()['state'][0]['step']) == 3.0


def test_an_overflow_skips_the_step_on_the_device_and_the_next_step_is_the_first(twins):
    first = twins[False][0]
    model, opt = _build()
    scaler = torch.amp.GradScaler('cuda', init_scale=SCALE)
    batch = _batch()
    with torch.autocast('cuda', dtype=torch.float16):
        loss = model.training_step(batch)
    (scaler.scale(loss) * float('inf')).backward()
    before = _weights(model)
    moments = [t.clone() for tw in model.towers() for t in opt._moments(tw)]
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == SCALE / 2
    for n, p in _weights(model).items():
        assert _same(p, before[n]), n
    for t, u in zip([t for tw in model.towers() for t in opt._moments(tw)], moments):
        assert _same(t, u)
    assert opt.step_count == 1 and int(opt._skipped) == 1
    opt.zero_grad()
    with torch.autocast('cuda', dtype=torch.float16):
        loss = model.training_step(batch)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == SCALE / 2
    assert _closest(_weights(model), first)[0] <= TENSOR_BOUND          # bias corrections of t = 1: those of t = 2 would move every weight by lr * 0.3
    sd = opt.state_dict()
    assert opt.step_count == 2 and all(float(st['step']) == 1.0 for st in sd['state'].values()) and len(sd['state']) > 0
