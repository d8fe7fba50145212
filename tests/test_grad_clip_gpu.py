"""Global gradient-norm clipping inside the fused AdamW step: dclip_sumsq_multi + dclip_clip_coef,
dclip_adamw_multi_scaled (csrc/optim.hip), FusedAdamW(max_grad_norm=...).  Semantics: torch.nn.utils.clip_grad_norm_(params, c)
followed by torch.optim.AdamW.step(), with norm and coefficient staying on the device.

Kernel constants the probes straddle (csrc/optim.hip): a lane loads LANE = 4 elements (one float4) at a time, the workgroup's 256 lanes
one ROW = 1024 elements per load, SUMSQ_LOADS = 8 loads make a workgroup TILE = 8192 elements, and a launch has PARTIALS = 1024 workgroups
(DCLIP_SUMSQ_PARTIALS), so a workgroup meets a second tile only past PARTIALS * TILE elements.  The kernel documents the longest serial
f32 accumulation chain as L = 8 (SUMSQ_LOADS).

Bound of the bounded probes, on the f32 norm against float64: |out[0] - ref| / ref <= 0.5 * (L + 64) * 2^-24 + 2^-24: all terms of the
sum of squares are non-negative, so a serial f32 chain of L terms and at most 64 further f32 additions lose at most L + 64 half-ulps
relative, the partial sums are added in double, the square root halves the relative error, and (float)sqrt(sum) rounds once more.

Optimizer-level tolerance: the one tests/test_checkpoint_gpu.py::test_layout_is_the_references holds FusedAdamW to torch.optim.AdamW with,
`err <= 1e-6 + 1e-5 * c.detach().abs().max().item()` per parameter tensor (err = largest absolute difference)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import real_cases as rc
from distillclip_amd import synth

pytestmark = pytest.mark.gpu

LANE, ROW, TILE, PARTIALS, L = 4, 1024, 8192, 1024, 8
NORM_BOUND = 0.5 * (L + 64) * 2.0 ** -24 + 2.0 ** -24
SIZES = [4, 8, 1020, 4100, 2 ** 20 + 12]                       # (the issue's) + the tile's own edges below
EDGES = [ROW - LANE, ROW, ROW + LANE, TILE - LANE, TILE, TILE + LANE]
T = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _ops():
    from distillclip_amd import ops
    assert ops.SUMSQ_PARTIALS == PARTIALS and ops.ADAMW_MAX_RANGES == 24
    return ops


def _carve(buf, lens):
    """views of `lens` elements each into buf, 16-byte aligned, 4 unused elements between neighbours"""
    views, at = [], 0
    for n in lens:
        views.append(buf[at:at + n])
        at += n + 4
    assert at <= buf.numel() + 4
    return views


def _norm_coef(views, max_norm=1.0, extra=None):
    """-> device tensor out[2] = (norm, coef) of one sumsq_multi + clip_coef"""
    ops = _ops()
    parts = torch.full((PARTIALS,), float('nan'), device='cuda')
    out = torch.full((2,), float('nan'), device='cuda')
    ops.sumsq_multi(views, parts)
    ops.clip_coef(parts, max_norm, out, extra)
    return out


def _range_sets():
    """[lens] with 1, 3 and 24 ranges"""
    small = SIZES[:4] + EDGES
    sets = [[n] for n in SIZES + EDGES]
    sets += [[n, 4, TILE + LANE] for n in SIZES + EDGES]
    sets += [[(small + [SIZES[4]])[(i + j) % 11] for i in range(24)] for j in (0, 5)]
    sets.append([PARTIALS * TILE + TILE + LANE])              # one range long enough that workgroups 0 and 1 take a second tile
    return sets


def test_sumsq_of_plus_minus_one_is_exactly_n():
    """(a) every element +-1: the sum of squares is n, exact in f32 below 2^24, and the norm is the f32 rounding of sqrt(n)"""
    gen = torch.Generator(device='cuda').manual_seed(1)
    outs, ns = [], []
    for lens in _range_sets():
        n = sum(lens)
        assert n < 2 ** 24
        buf = (torch.randint(0, 2, (n + 4 * len(lens),), device='cuda', generator=gen) * 2 - 1).float()
        outs.append(_norm_coef(_carve(buf, lens)))
        ns.append(n)
    got = torch.stack(outs).cpu().numpy()
    for (norm, _), n, lens in zip(got, ns, _range_sets()):
        want = np.float32(np.sqrt(np.float64(n)))
        assert norm.tobytes() == want.tobytes(), (lens[:4], len(lens), norm, want)


def test_a_single_element_is_found_wherever_it_lies():
    """(b) x = 3 at position k, zeros elsewhere: the norm is exactly 3 — a lost tail or a skipped range would give 0"""
    n = SIZES[4]
    buf = torch.zeros(n, device='cuda')
    ks = sorted({0, n - 1} | {e + d for e in (LANE, ROW, TILE, 2 * TILE, 127 * TILE, 128 * TILE) for d in (-1, 0, 1) if 0 <= e + d < n})
    outs = []
    for k in ks:
        buf[k] = 3.0
        outs.append(_norm_coef([buf]))
        buf[k] = 0.0
    lens = _range_sets()[-2]
    assert len(lens) == 24
    buf = torch.zeros(sum(lens) + 4 * 24, device='cuda')
    views = _carve(buf, lens)
    where = []
    for i, v in enumerate(views):
        for k in (0, v.numel() - 1):
            v[k] = 3.0
            outs.append(_norm_coef(views))
            v[k] = 0.0
            where.append((i, k))
    got = torch.stack(outs).cpu().numpy()
    for tag, (norm, _) in zip(ks + where, got):
        assert norm == np.float32(3.0), (tag, norm)


def test_extra_sumsq_enters_the_norm_and_the_coefficient_is_torchs():
    """(c) all-zero ranges + extra_sumsq = 16: norm 4; max_norm 2: coef = 2 / (4 + 1e-6) in f32.  (d) the same call twice: same bits."""
    buf = torch.zeros(4100 + 8 + 1020 + 12, device='cuda')
    views = _carve(buf, [4100, 8, 1020])
    extra = torch.tensor([16.0], device='cuda')
    norm, coef = _norm_coef(views, 2.0, extra).cpu().numpy()
    assert norm == np.float32(4.0)
    assert coef.tobytes() == (np.float32(2) / (np.float32(4) + np.float32(1e-6))).tobytes()
    assert _norm_coef(views, 1e30, extra).cpu().numpy()[1] == np.float32(1.0)
    g = torch.randn(2 ** 20 + 12, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    a, b = _norm_coef([g, g[:4100]], 0.25, extra), _norm_coef([g, g[:4100]], 0.25, extra)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    nan = _norm_coef([torch.full((8,), float('nan'), device='cuda')], 1.0).cpu().numpy()
    assert np.isnan(nan).all()                                 # a non-finite norm is not special-cased: NaN coefficient, as in torch


def test_buffers_the_kernels_may_and_may_not_touch():
    """(e) gradients are read-only; sumsq_multi writes partials[0 .. n_partials) — all finite, zeros past the workgroups' — and nothing after"""
    ops = _ops()
    gen = torch.Generator(device='cuda').manual_seed(3)
    buf = torch.randn(TILE + LANE + 4 + 1020 + 4 + 8, device='cuda', generator=gen)
    views = _carve(buf, [TILE + LANE, 1020, 8])
    before = buf.clone()
    parts = torch.full((PARTIALS + 37,), float('nan'), device='cuda')
    out = torch.full((2,), float('nan'), device='cuda')
    ops.sumsq_multi(views, parts[:PARTIALS + 5])
    ops.clip_coef(parts[:PARTIALS + 5], 1.0, out)
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    assert bool(torch.isfinite(parts[:PARTIALS + 5]).all()) and float(parts[PARTIALS:PARTIALS + 5].abs().max()) == 0.0
    assert bool(torch.isnan(parts[PARTIALS + 5:]).all())
    assert int((parts[:PARTIALS] != 0).sum()) == 4             # 2 + 1 + 1 tiles, one workgroup each
    ref = np.sqrt(sum(float((v.double() ** 2).sum()) for v in views))
    assert abs(float(out[0]) - ref) <= NORM_BOUND * ref


def test_refusals():
    """(f) a length that is no multiple of 4, a pointer off by 8 bytes, 0 and 25 ranges, a short partials array, a null out: ValueError
    before any launch, nothing written"""
    from distillclip_amd._lib import lib
    g = torch.ones(64, device='cuda')
    parts = torch.full((PARTIALS,), float('nan'), device='cuda')
    out = torch.full((2,), 7.0, device='cuda')
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    n1 = lambda n: (ctypes.c_int64 * 1)(n)
    with pytest.raises(ValueError, match='multiple of 4'):
        lib().dclip_sumsq_multi(one(g), n1(6), 1, parts.data_ptr(), PARTIALS, None)
    with pytest.raises(ValueError, match='16-byte aligned'):
        lib().dclip_sumsq_multi(one(g[2:]), n1(4), 1, parts.data_ptr(), PARTIALS, None)
    for count in (0, 25):
        with pytest.raises(ValueError, match='1..24'):
            lib().dclip_sumsq_multi(one(g), n1(64), count, parts.data_ptr(), PARTIALS, None)
    with pytest.raises(ValueError, match='slots'):
        lib().dclip_sumsq_multi(one(g), n1(64), 1, parts.data_ptr(), PARTIALS - 1, None)
    with pytest.raises(ValueError):
        lib().dclip_clip_coef(parts.data_ptr(), PARTIALS, None, 1.0, None, None)
    with pytest.raises(ValueError):
        lib().dclip_clip_coef(None, PARTIALS, None, 1.0, out.data_ptr(), None)
    with pytest.raises(ValueError):
        lib().dclip_clip_coef(parts.data_ptr(), 0, None, 1.0, out.data_ptr(), None)
    p = [torch.zeros(64, device='cuda') for _ in range(4)]
    with pytest.raises(ValueError, match='multiple of 4'):
        lib().dclip_adamw_multi_scaled(one(p[0]), one(p[1]), one(p[2]), one(p[3]), n1(6), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, out.data_ptr(), None)
    with pytest.raises(RuntimeError):
        _ops().sumsq_multi([torch.ones(8)], parts)             # no CPU fallback
    torch.cuda.synchronize()
    assert bool(torch.isnan(parts).all()) and out.tolist() == [7.0, 7.0] and float(sum(t.abs().sum() for t in p)) == 0.0


@pytest.mark.parametrize('scale', [1e-6, 1.0, 1e4])
def test_norm_of_normal_gradients_against_float64(scale):
    gen = torch.Generator(device='cuda').manual_seed(4)
    mixed = [[4, 8, 1020, 4100, TILE, TILE + LANE, 65540, ROW - LANE][i % 8] for i in range(24)]
    worst = 0.0
    for lens in ([1_048_588], mixed):
        buf = torch.randn(sum(lens) + 4 * len(lens), device='cuda', generator=gen) * scale
        views = _carve(buf, lens)
        got = float(_norm_coef(views)[0])
        ref = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in views)))
        err = abs(got - ref) / ref
        worst = max(worst, err)
        print(f'scale {scale:g}, {len(lens)} ranges: |norm - ref| / ref = {err:.3e} (bound {NORM_BOUND:.3e})')
        assert err <= NORM_BOUND, (scale, len(lens), got, ref)
    print(f'scale {scale:g}: worst {worst:.3e}')


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('step', [1, 7])
def test_adamw_multi_scaled_is_adamw_multi_on_the_rounded_product(step, zero_grad):
    """gscale null or 1.0: dclip_adamw_multi bit for bit; 0.5 and 0.3172: dclip_adamw_multi on the gradients multiplied beforehand in
    torch f32 — the kernel forms g * scale as one f32 product before anything else"""
    from distillclip_amd._lib import lib
    ops = _ops()
    gen = torch.Generator(device='cuda').manual_seed(5)
    lens = [4, 1020, 65_540]
    mk = lambda: [torch.randn(n, device='cuda', generator=gen) for n in lens]
    p0, g0, m0 = mk(), mk(), mk()
    v0 = [t.abs() for t in mk()]
    hyper = (3e-3, (0.9, 0.999), 1e-8, 1e-2)

    def base(gs):
        a = [[t.clone() for t in x] for x in (p0, gs, m0, v0)]
        arr = lambda k: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in a[k]])
        lib().dclip_adamw_multi(arr(0), arr(1), arr(2), arr(3), (ctypes.c_int64 * 3)(*lens), 3, hyper[0], hyper[1][0], hyper[1][1], hyper[2],
                                hyper[3], step, zero_grad, torch.cuda.current_stream().cuda_stream)
        return a

    for scale in (None, 1.0, 0.5, 0.3172):
        s = None if scale is None else torch.tensor([scale], dtype=torch.float32, device='cuda')
        want = base(g0 if scale is None else [g * torch.tensor(scale, dtype=torch.float32) for g in g0])
        a = [[t.clone() for t in x] for x in (p0, g0, m0, v0)]
        ops.adamw_multi_scaled(list(zip(*a)), *hyper, step, zero_grad, s)
        torch.cuda.synchronize()
        for k in (0, 2, 3):
            for t, u in zip(a[k], want[k]):
                assert torch.equal(t.view(torch.int32), u.view(torch.int32)), (scale, 'pgmv'[k], t.numel())
        for g, orig in zip(a[1], g0):                          # the gradient itself is consumed (cleared on request), never scaled in place
            assert torch.equal(g, torch.zeros_like(g) if zero_grad else orig)


# ---- optimizer level: the tiny dual configuration of tests/test_towers_gpu.py (TINY there), built from synth ----------------------------------
S_IMG = dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4,
             mlp_ratio=4.0, qkv_bias=True, repeated_times=2, use_transform=True)
S_TXT = dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2,
             mlp_ratio=4.0, qkv_bias=False, repeated_times=2, use_transform=True)
SEED, LR, WD = 11, 1e-3, 1e-2


def _dual(**opt_kw):
    from distillclip_amd.model import DualDistillModel
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    from distillclip_amd.optim import FusedAdamW
    s_img, s_txt = RepeatVisionTransformer(**S_IMG), RepeatTextTransformer(**S_TXT)
    s_img.load_state_dict(T(synth.student_image_state(SEED, **S_IMG)))
    s_txt.load_state_dict(T(synth.student_text_state(SEED, **S_TXT)))
    tsd = synth.teacher_image_state(SEED, 128, 2, 8, 32, 64)
    tsd.update(synth.teacher_text_state(SEED, 128, 2, 13, 97, 64))
    m = DualDistillModel(s_img, s_txt, dict(loss_name=['out_cos', 'cos_diff'], loss_scale={'cos_diff': 0.1}),
                         warm_steps=0, total_steps=10, weight_decay=WD, lr=LR, download_root='.', teacher_state_dict=T(tsd)).cuda()
    towers = m.towers()
    for tw in towers:
        tw.materialize(torch.device('cuda', torch.cuda.current_device()))
    return m, FusedAdamW(towers, lr=LR, weight_decay=WD, **opt_kw)


def _batch(i, B=3):
    return [torch.from_numpy(synth.images(100 + i, B, 32)).cuda(), torch.from_numpy(synth.captions(100 + i, B, 13, 97, 3, 9)).cuda()]


@pytest.fixture(scope='module')
def recorded():
    """two backwards of the tiny dual model at its initial weights (batches 0 and 1): the towers' flat gradient buffers, so that every
    variant below steps on the same bits (the weight-gradient atomics differ from run to run), and the float64 norm G of the first"""
    m, opt = _dual()
    grads = []
    for i in range(2):
        opt.zero_grad()
        m.backward_and_sync(m.training_step(_batch(i)))
        torch.cuda.synchronize()
        grads.append([tw.flat_grad.clone() for tw in m.towers()])
    slots = opt._slots()
    index = {id(tw): k for k, tw in enumerate(m.towers())}
    cpu_g = [[g[index[id(tw)]][off:off + n].cpu().view(shape) for tw, off, n, shape in slots] for g in grads]
    G = float(np.sqrt(sum(float((t.double() ** 2).sum()) for t in cpu_g[0])))
    return dict(grads=grads, cpu_g=cpu_g, G=G)


def _run(recorded, max_grad_norm, **step_kw):
    """a fresh model, two steps on the recorded gradients -> (flat weights, moments, the norm after the first step, CPU start weights)"""
    m, opt = _dual(max_grad_norm=max_grad_norm)
    start = [tw.flat[off:off + n].detach().cpu().view(shape).clone() for tw, off, n, shape in opt._slots()]
    norms = []
    for i in range(2):
        opt.zero_grad()
        m.backward_and_sync(m.training_step(_batch(i)), defer_wait=bool(step_kw))      # (sets the towers' streams as a real step does)
        torch.cuda.synchronize()
        for tw, g in zip(m.towers(), recorded['grads'][i]):
            tw.flat_grad.copy_(g)
        torch.cuda.synchronize()
        opt.step(**step_kw)
        if step_kw.get('join') is False:
            opt.join()
        norms.append(None if opt.last_grad_norm is None else float(opt.last_grad_norm))
    torch.cuda.synchronize()
    moments = [t.clone() for tw in m.towers() for t in opt._state[id(tw)]]
    return [tw.flat.clone() for tw in m.towers()], moments, norms, start, opt


def _tolerance(err, ref):
    """tests/test_checkpoint_gpu.py::test_layout_is_the_references: err <= 1e-6 + 1e-5 * c.detach().abs().max().item()"""
    return err <= 1e-6 + 1e-5 * ref.abs().max().item()


@pytest.fixture(scope='module')
def clipped(recorded):
    return _run(recorded, 0.5 * recorded['G'])


def test_clipped_step_equals_clip_grad_norm_then_torch_adamw(recorded, clipped):
    """(i) max_grad_norm = G / 2, two steps"""
    flats, _, norms, start, opt = clipped
    G = recorded['G']
    print(f'G = {G:.6e}, last_grad_norm after step 1 = {norms[0]:.6e}, |d| / G = {abs(norms[0] - G) / G:.3e} (bound {NORM_BOUND:.3e})')
    assert abs(norms[0] - G) <= NORM_BOUND * G
    cpu = [torch.nn.Parameter(t.clone()) for t in start]
    ref = torch.optim.AdamW(cpu, lr=LR, weight_decay=WD)
    for i in range(2):
        for c, g in zip(cpu, recorded['cpu_g'][i]):
            c.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(cpu, 0.5 * G)
        assert i or abs(float(total) - G) <= 1e-5 * G
        ref.step()
    index = {id(tw): k for k, tw in enumerate(opt.towers)}
    moved = 0.0
    for c, s, (tw, off, n, shape) in zip(cpu, start, opt._slots()):
        got = flats[index[id(tw)]][off:off + n].cpu().view(shape)
        err = (got - c.detach()).abs().max().item()
        assert _tolerance(err, c.detach()), (off, shape, err)
        moved = max(moved, (got - s).abs().max().item())
    assert moved > 1e-4                                        # (the weights did move: two steps at lr 1e-3)


def test_a_threshold_never_reached_changes_nothing(recorded):
    """(ii) max_grad_norm = 1e30: coef is exactly 1, weights and moments are those of an optimizer built without clipping, bit for bit"""
    a = _run(recorded, 1e30)
    b = _run(recorded, None)
    assert b[2] == [None, None] and abs(a[2][0] - recorded['G']) <= NORM_BOUND * recorded['G']
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_overlapped_unjoined_clipped_step_gives_the_same_bits(recorded, clipped):
    """(iii) step(overlap=True, join=False) + join(): sums on the towers' streams, one coefficient after all of them, updates after it"""
    a = _run(recorded, 0.5 * recorded['G'], overlap=True, join=False)
    assert a[2] == clipped[2]
    for x, y in zip(a[0] + a[1], clipped[0] + clipped[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_clip_student_pair_with_extra_parameters(golden_dir):
    """(iv) ImageEncoder / TextEncoder as students (the tiny case of tests/real_cases.py): their projection linears lie outside the towers'
    buffers (extra_params) and take part in the norm; the update is clip_grad_norm_ + torch.optim.AdamW's"""
    from distillclip_amd.model import LossCalculator
    from distillclip_amd.model.component import ImageEncoder, TextEncoder, CLIPModel
    from distillclip_amd.optim import FusedAdamW
    c = rc.CLIPSTU_TINY
    image, text, tsd_i, tsd_t, sd_i, sd_t = rc.clipstu_inputs(rc.load(golden_dir, 'clip_student_tiny.npz'), c)
    tw_i, tw_t = tsd_i['visual.conv1.weight'].shape[0], tsd_t['positional_embedding'].shape[1]
    t_img = ImageEncoder(False, dict(input_resolution=c['res'], patch_size=c['patch'], width=tw_i, layers=c['tea_layers'], heads=c['tea_heads'],
                                     output_dim=c['out_dim'], need_layers=c['need_layers']))
    t_txt = TextEncoder(tw_t, c['tea_layers'], c['tea_heads'], c['ctx'], c['need_layers'], c['vocab'], c['out_dim'], is_student=False)
    s_img = ImageEncoder(True, dict(input_resolution=c['res'], patch_size=c['patch'], width=c['width'], layers=c['layers'], heads=c['heads'],
                                    output_dim=c['out_dim'], need_layers=None), tea_transformer_width=tw_i)
    s_txt = TextEncoder(c['width'], c['layers'], c['heads'], c['ctx'], None, c['vocab'], c['out_dim'], tea_transformer_width=tw_t, is_student=True)
    for m, sd in ((t_img, tsd_i), (t_txt, tsd_t), (s_img, sd_i), (s_txt, sd_t)):
        m.load_state_dict(sd)
    student, teacher = CLIPModel(True, s_img.cuda(), s_txt.cuda()), CLIPModel(False, t_img.cuda(), t_txt.cuda())
    for p in teacher.parameters():
        p.requires_grad = False
    towers = [s_img._tower, s_txt._tower]
    for tw in towers:
        tw.materialize(torch.device('cuda', torch.cuda.current_device()))
    extras = s_img.extra_parameters() + s_txt.extra_parameters()
    assert len(extras) == 8                                    # four projection tensors per encoder
    lc = LossCalculator(rc.CLIPSTU_SMOOTH)
    opt = FusedAdamW(towers, lr=2e-3, weight_decay=1e-2, extra_params=extras)
    opt.zero_grad()
    loss, _ = lc(student(text.cuda(), image.cuda(), lc.get_control_output()), teacher(text.cuda(), image.cuda(), lc.get_control_output()), 'all')
    loss.backward()
    torch.cuda.synchronize()
    params = list(student.parameters())
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    for q, p in zip(cpu, params):
        q.grad = p.grad.detach().cpu().clone()
    sq = lambda ts: sum(float((t.grad.double() ** 2).sum()) for t in ts)
    G = float(np.sqrt(sq(cpu)))
    extra_ids = {id(p) for p in extras}
    G_towers = float(np.sqrt(sq([q for q, p in zip(cpu, params) if id(p) not in extra_ids])))
    assert G - G_towers > 100 * NORM_BOUND * G                 # the projections' share of the norm is far above what the bound lets pass
    opt.max_grad_norm = 0.5 * G
    opt.step()
    got = float(opt.last_grad_norm)
    print(f'G = {G:.6e} (towers alone {G_towers:.6e}), last_grad_norm = {got:.6e}, |d| / G = {abs(got - G) / G:.3e} (bound {NORM_BOUND:.3e})')
    assert abs(got - G) <= NORM_BOUND * G
    ref = torch.optim.AdamW(cpu, lr=2e-3, weight_decay=1e-2)
    torch.nn.utils.clip_grad_norm_(cpu, 0.5 * G)
    ref.step()
    for (name, p), q in zip(student.named_parameters(), cpu):
        err = (p.detach().cpu() - q.detach()).abs().max().item()
        assert _tolerance(err, q.detach()), (name, err)


_WORLD1 = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import numpy as np, torch, torch.distributed as dist
import test_grad_clip_gpu as t
from distillclip_amd.parallel import GradSync

def train(model, opt, c, steps=3):
    opt.max_grad_norm = c
    norms = []
    for i in range(steps):
        loss = model.training_step(t._batch(0, 6))
        opt.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        opt.step(zero_grad=True, overlap=True, join=False)
        norms.append(opt.last_grad_norm.clone())
    opt.join()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in model.student.named_parameters()}, [float(n) for n in norms]

m, opt = t._dual()
m.backward_and_sync(m.training_step(t._batch(0, 6)))
torch.cuda.synchronize()
G = float(np.sqrt(sum(float((tw.flat_grad[a:b].double() ** 2).sum()) for tw in m.towers() for a, b in opt._ranges(tw))))
plain, n_plain = train(*t._dual(), 0.5 * G)
os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
os.environ.setdefault('MASTER_PORT', '29543')
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
try:
    model, opt = t._dual()
    model._sync = GradSync()
    model._sync.enabled = True                      # world 1: the collectives still run (RCCL), the shard is the whole bucket
    model._ensure_sync()
    sharded, n_sharded = train(model, opt, 0.5 * G)
    assert all(tw.dp is not None for tw in model.towers())
finally:
    dist.destroy_process_group()
print('norms', G, n_plain, n_sharded)
assert abs(n_plain[0] - G) <= 1e-3 * G and all(abs(a - b) <= 1e-3 * a for a, b in zip(n_plain, n_sharded)), (G, n_plain, n_sharded)
for k in plain:
    d = (plain[k] - sharded[k]).abs()
    assert d.max() < 3e-3 and d.mean() < (1e-3 if 'qkv.bias' in k else 2e-5), (k, d.max().item(), d.mean().item())
print('WORLD1 OK')
'''


def test_clipped_sharded_path_over_rccl_world1_equals_clipped_plain_path(tmp_path):
    """(v) the exchange forced at world size 1 (bench.py's DCLIP_FORCE_DIST=1: a 1-rank RCCL group with GradSync.enabled set, as
    tests/test_checkpoint_gpu.py sets it up), in a fresh child process: the clipped data-parallel step (owned-slice sums of tw.gshard,
    the all-reduce of the sum, the scaled sharded AdamW) against the clipped plain step, within the bound of
    tests/test_checkpoint_gpu.py::test_reduce_scatter_sharded_path_over_rccl_world1_equals_plain_path:
    d.max() < 3e-3 and d.mean() < (1e-3 if 'qkv.bias' in k else 2e-5) after 3 steps at lr 1e-3"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'world1.py'
    script.write_text(_WORLD1)
    env = dict(os.environ, DCLIP_FORCE_DIST='1')
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [str(script), root], env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0 and 'WORLD1 OK' in r.stdout
