"""Host side of the gradient clipping in FusedAdamW: the Lightning hook, the launches of a step without clipping, and the sharded
bookkeeping rehearsed at world size 2 over gloo with torch substitutes for the three kernels (launcher pattern of tests/test_parallel_cpu.py)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_configure_gradient_clipping_hands_the_threshold_to_the_optimizer():
    from distillclip_amd.model._distill_base import DistillBase
    hook = DistillBase.configure_gradient_clipping
    opt = types.SimpleNamespace(max_grad_norm=None)
    hook(None, opt, 0.7, 'norm')
    assert opt.max_grad_norm == 0.7
    hook(None, opt, gradient_clip_val=0.3, gradient_clip_algorithm='norm')
    assert opt.max_grad_norm == 0.3
    hook(None, opt, 0, 0.9, 'norm')                               # older Lightning: optimizer_idx second
    assert opt.max_grad_norm == 0.9
    hook(None, opt, gradient_clip_val=0.4)
    assert opt.max_grad_norm == 0.4
    for off in (None, 0, 0.0):
        opt.max_grad_norm = 1.0
        hook(None, opt, gradient_clip_val=off, gradient_clip_algorithm=None)
        assert opt.max_grad_norm is None
    opt.max_grad_norm = 1.0
    hook(None, opt, None, None)
    assert opt.max_grad_norm is None
    for call in (lambda: hook(None, opt, 0.5, 'value'), lambda: hook(None, opt, 0, 0.5, 'value'),
                 lambda: hook(None, opt, gradient_clip_val=0.5, gradient_clip_algorithm='value')):
        with pytest.raises(ValueError, match='value'):
            call()
    assert opt.max_grad_norm is None                              # a refused call changes nothing


# ---- torch restatements of the three kernels (the CPU rehearsal; the product path is HIP) ---------------------------------------------
def _torch_adamw(self, p, g, m, v, zero_grad, st, gscale=None):
    """dclip_adamw / dclip_adamw_multi_scaled: torch.optim.AdamW on gs = g * gscale"""
    gs = g if gscale is None else g * gscale
    b1, b2 = self.betas
    p.mul_(1.0 - self.lr * self.weight_decay)
    m.mul_(b1).add_(gs, alpha=1 - b1)
    v.mul_(b2).addcmul_(gs, gs, value=1 - b2)
    bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
    p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(self.eps), value=-self.lr / bc1)
    if zero_grad:
        g.zero_()


def _torch_sumsq(self, views, out, st):
    """dclip_sumsq_multi: every slot of `out` written, their sum is the sum of squares"""
    out.zero_()
    out[0] = sum((v.double() ** 2).sum() for v in views).float()


def _torch_coef(self, partials, extra, out, st):
    """dclip_clip_coef"""
    s = partials.double().sum()
    if extra is not None:
        s = s + extra.double().sum()
    out[0] = s.sqrt().float()
    out[1] = torch.clamp(self.max_grad_norm / (out[0] + 1e-6), max=1.0)


def _rehearsal_optimizer():
    from distillclip_amd.optim import FusedAdamW

    class Rehearsal(FusedAdamW):
        _adamw, _sumsq, _coef = _torch_adamw, _torch_sumsq, _torch_coef
    return Rehearsal


def test_a_step_without_clipping_never_reaches_the_new_hooks():
    def boom(*a, **k):
        raise AssertionError('clipping hook called')

    class NoClip(_rehearsal_optimizer()):
        _sumsq = _coef = boom

        def _adamw(self, p, g, m, v, zero_grad, st, *scale):
            assert not scale                                      # the step as it was: no scale argument at all
            _torch_adamw(self, p, g, m, v, zero_grad, st)
    gen = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(16, 8, generator=gen)), torch.nn.Parameter(torch.randn(16, generator=gen))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = NoClip([], lr=1e-2, weight_decay=1e-2, extra_params=ps)
    assert opt.max_grad_norm is None and opt.last_grad_norm is None
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    for p, q in zip(ps, ref):
        p.grad = torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    opt.step()
    topt.step()
    assert opt.last_grad_norm is None
    for p, q in zip(ps, ref):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6)
    opt.max_grad_norm = 1.0                                       # ... and with a threshold it does reach them
    with pytest.raises(AssertionError, match='clipping hook called'):
        opt.step()
    sd = opt.state_dict()                                         # not optimizer state, as in torch
    assert 'max_grad_norm' not in sd['param_groups'][0] and set(sd) == {'state', 'param_groups'}


def test_clipped_step_on_extras_alone_equals_clip_grad_norm_then_adamw():
    gen = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(16, 8, generator=gen)), torch.nn.Parameter(torch.randn(16, generator=gen))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = _rehearsal_optimizer()([], lr=1e-2, weight_decay=1e-2, extra_params=ps, max_grad_norm=0.5)
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    for step in range(3):
        for p, q in zip(ps, ref):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        G = float(np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in ps)))
        opt.step()
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        topt.step()
        assert G > 0.5 and abs(float(opt.last_grad_norm) - G) <= 2.0 ** -22 * G
        for p, q in zip(ps, ref):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), step
    opt.max_grad_norm = None
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert opt.last_grad_norm is None


# ---- world size 2 over gloo (tests/test_parallel_cpu.py's launcher: FileStore rendezvous, results by value, no retry) ------------------
def _to_numpy(o):
    if isinstance(o, torch.Tensor):
        return ('__tensor__', o.detach().cpu().numpy().copy())
    if isinstance(o, (list, tuple)):
        return type(o)(_to_numpy(v) for v in o)
    return o


def _to_torch(o):
    if isinstance(o, tuple) and len(o) == 2 and isinstance(o[0], str) and o[0] == '__tensor__':
        return torch.from_numpy(o[1])
    if isinstance(o, (list, tuple)):
        return type(o)(_to_torch(v) for v in o)
    return o


class _ResultQueue:
    def __init__(self, q):
        self.q = q

    def put(self, item):
        self.q.put(_to_numpy(item))


def _run_ranks(target, world=2, timeout=120):
    import queue as _queue
    import shutil
    import tempfile
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    d = tempfile.mkdtemp(prefix='dclip_rdzv_')
    ps = [ctx.Process(target=target, args=(r, world, os.path.join(d, 'store'), _ResultQueue(q))) for r in range(world)]
    for p in ps:
        p.start()
    try:
        try:
            res = [_to_torch(q.get(timeout=timeout)) for _ in ps]
        except _queue.Empty:
            raise AssertionError(f'ranks did not report within {timeout} s (exit codes so far {[p.exitcode for p in ps]})')
        codes = []
        for p in ps:
            p.join(timeout=60)
            codes.append(p.exitcode)
        assert all(c == 0 for c in codes), f'rank exit codes {codes}'
        return res
    finally:
        for p in ps:
            if p.is_alive():
                p.terminate()
            p.join(timeout=30)
        shutil.rmtree(d, ignore_errors=True)


class _FakeTower:
    """flat buffers + bucket layout of a tower, without the HIP runtime (the bookkeeping under test is host logic)"""

    def __init__(self, total, buckets, trainable, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat = torch.randn(total, generator=g)
        self.flat_grad = torch.zeros(total)
        self._buckets, self._trainable = buckets, trainable
        self.sync = self.dp = self.gshard = None
        self.dp_released = 0
        self.wcache_dirty = False
        self.grads_ready = self.opt_done = self.bwd_stream = None
        self._grad_clean = False
        edges = sorted({0, total} | {e for r in trainable for e in r})
        self._offsets = edges[:-1]
        self._plist = [self.flat[a:b] for a, b in zip(edges[:-1], edges[1:])]

    def _params(self):
        return self._plist

    def grad_buckets(self):
        return list(self._buckets)

    def trainable_ranges(self):
        return [list(r) for r in self._trainable]


# completion order: head bucket at the END of the flat layout, two blocks, a frozen-only bucket, embedding at the start
_TOTAL = 64 * 40
_BUCKETS = [(64 * 34, 64 * 40), (64 * 20, 64 * 34), (64 * 12, 64 * 20), (64 * 8, 64 * 12), (0, 64 * 8)]
_TRAINABLE = [[64 * 2, 64 * 8], [64 * 12, 64 * 25], [64 * 26, 64 * 40]]
_MAX_NORM, _STEPS, _EXTRA_SCALE = 0.75, 3, 3.0


def _mask():
    mask = torch.zeros(_TOTAL, dtype=torch.bool)
    for a, b in _TRAINABLE:
        mask[a:b] = True
    return mask


def _extras():
    g0 = torch.Generator().manual_seed(7)
    return [torch.nn.Parameter(torch.randn(16, 8, generator=g0)), torch.nn.Parameter(torch.randn(16, generator=g0))]


def _rank_grads(step, rank, shapes):
    g = torch.Generator().manual_seed(100 * step + rank)
    return torch.randn(_TOTAL, generator=g) * _mask(), [torch.randn(s, generator=g) * _EXTRA_SCALE for s in shapes]


def _clip_worker(rank, world, rdzv, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', init_method='file://' + rdzv, rank=rank, world_size=world)
    from distillclip_amd.parallel import GradSync
    tw = _FakeTower(_TOTAL, _BUCKETS, _TRAINABLE, seed=3)
    extras = _extras()
    sync = GradSync()
    assert sync.enabled and sync.sharded
    sync.attach([tw])
    opt = _rehearsal_optimizer()([tw], lr=1e-2, weight_decay=1e-2, extra_params=extras, max_grad_norm=_MAX_NORM)
    outs = []
    for step in range(_STEPS):
        flat_g, extra_g = _rank_grads(step, rank, [p.shape for p in extras])
        tw.flat_grad.add_(flat_g)
        for i in range(len(_BUCKETS)):
            sync.bucket_ready(tw, i)
        sync.finish(tw)
        for p, g in zip(extras, extra_g):
            p.grad = g
        opt.step()
        outs.append(opt._clip_out.clone())                                 # (norm, coef)
        opt.zero_grad()
    q.put((rank, tw.flat.clone(), [p.detach().clone() for p in extras], torch.stack(outs)))
    dist.monitored_barrier()
    dist.destroy_process_group()


def test_sharded_clipped_step_world2_equals_clip_grad_norm_on_the_averaged_gradients():
    world = 2
    res = sorted(_run_ranks(_clip_worker, world, timeout=240), key=lambda r: r[0])
    # every rank ends with the same coefficient and the same parameters, bit for bit
    for r in res[1:]:
        assert torch.equal(r[3].view(torch.int32), res[0][3].view(torch.int32))
        assert torch.equal(r[1].view(torch.int32), res[0][1].view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(r[2], res[0][2]))
    # one process: clip_grad_norm_ on the averaged gradients + torch.optim.AdamW over the same parameter set
    ref = _FakeTower(_TOTAL, _BUCKETS, _TRAINABLE, seed=3)
    chunks = [torch.nn.Parameter(ref.flat[a:b].clone()) for a, b in _TRAINABLE]
    extras = _extras()
    topt = torch.optim.AdamW(chunks + extras, lr=1e-2, weight_decay=1e-2)
    for step in range(_STEPS):
        per_rank = [_rank_grads(step, r, [p.shape for p in extras]) for r in range(world)]
        avg = sum(g for g, _ in per_rank) / world
        for c, (a, b) in zip(chunks, _TRAINABLE):
            c.grad = avg[a:b].clone()
        for k, p in enumerate(extras):
            p.grad = sum(e[k] for _, e in per_rank) / world
        tower_sq = sum(float((c.grad.double() ** 2).sum()) for c in chunks)
        extra_sq = sum(float((p.grad.double() ** 2).sum()) for p in extras)
        G = np.sqrt(tower_sq + extra_sq)
        # the extras' gradients are whole on every rank: counted once.  Counted once per rank, the norm would be
        # sqrt(tower_sq + world * extra_sq), larger by the factor below — far outside what the assertion lets pass
        wrong = np.sqrt(tower_sq + world * extra_sq)
        assert wrong / G > 1.01
        norm, coef = (float(x) for x in res[0][3][step])
        assert abs(norm - G) <= 2.0 ** -22 * G, (step, norm, G, wrong)      # f32 roundings of the rehearsal's sums: a few 2^-24
        assert G > _MAX_NORM and abs(coef - _MAX_NORM / (G + 1e-6)) <= 1e-6
        torch.nn.utils.clip_grad_norm_(chunks + extras, _MAX_NORM)
        topt.step()
    want = ref.flat.clone()
    for c, (a, b) in zip(chunks, _TRAINABLE):
        want[a:b] = c.detach()
    mask = _mask()
    for rank, flat, got_extras, _ in res:
        assert torch.allclose(flat, want, rtol=1e-5, atol=1e-6), (rank, (flat - want).abs().max())     # tests/test_parallel_cpu.py's Adam-noise tolerance
        assert torch.equal(flat[~mask], ref.flat[~mask])
        for a, b in zip(got_extras, extras):
            assert torch.allclose(a, b.detach(), rtol=1e-5, atol=1e-6), rank


def test_a_tower_that_is_not_sharded_steps_unclipped_on_the_cpu_like_torch_adamw():
    """one process, no exchange, no clipping: step() takes the tower's ranges from flat_grad on the caller's (here: no) stream"""
    gen = torch.Generator().manual_seed(5)
    tw = _FakeTower(16 * 8 + 16 + 16, [(0, 16 * 8 + 16 + 16)], [[0, 16 * 8], [16 * 8 + 16, 16 * 8 + 32]], seed=4)
    before = tw.flat.clone()
    ref = [torch.nn.Parameter(tw.flat[a:b].clone()) for a, b in tw.trainable_ranges()]
    opt = _rehearsal_optimizer()([tw], lr=1e-2, weight_decay=1e-2)
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    for step in range(3):
        for q, (a, b) in zip(ref, tw.trainable_ranges()):
            q.grad = torch.randn(b - a, generator=gen)
            tw.flat_grad[a:b] = q.grad
        opt.step(zero_grad=True)
        topt.step()
        assert opt.last_grad_norm is None
        for q, (a, b) in zip(ref, tw.trainable_ranges()):
            assert torch.allclose(tw.flat[a:b], q.detach(), rtol=1e-5, atol=1e-6), step
            assert not tw.flat_grad[a:b].any()                    # consumed and cleared
    assert torch.equal(tw.flat[16 * 8:16 * 8 + 16], before[16 * 8:16 * 8 + 16])      # the frozen range
    assert tw.wcache_dirty and not tw._grad_clean                 # two ranges: not the whole buffer


# one bucket whose trainable part lies in rank 0's half: rank 1 owns no slice, and still takes part in the sum over the ranks
_HALF_TOTAL, _HALF_TRAINABLE = 64 * 4, [[0, 64 * 2]]


def _half_grad(step, rank):
    g = torch.zeros(_HALF_TOTAL)
    g[:64 * 2] = torch.randn(64 * 2, generator=torch.Generator().manual_seed(300 + 10 * step + rank))
    return g


def _half_owner_worker(rank, world, rdzv, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', init_method='file://' + rdzv, rank=rank, world_size=world)
    from distillclip_amd.parallel import GradSync
    tw = _FakeTower(_HALF_TOTAL, [(0, _HALF_TOTAL)], _HALF_TRAINABLE, seed=9)
    sync = GradSync()
    sync.attach([tw])
    opt = _rehearsal_optimizer()([tw], lr=1e-2, weight_decay=1e-2, max_grad_norm=_MAX_NORM)
    outs = []
    for step in range(2):
        tw.flat_grad.add_(_half_grad(step, rank))
        sync.bucket_ready(tw, 0)
        sync.finish(tw)
        opt.step()
        outs.append(opt._clip_out.clone())
        opt.zero_grad()
    q.put((rank, tw.flat.clone(), torch.stack(outs), len(opt._shard_items(tw, *opt._moments(tw)))))
    dist.monitored_barrier()
    dist.destroy_process_group()


def test_a_rank_that_owns_no_trainable_slice_still_gets_the_global_coefficient():
    world = 2
    res = sorted(_run_ranks(_half_owner_worker, world, timeout=120), key=lambda r: r[0])
    assert [r[3] for r in res] == [1, 0]                              # the layout does what the test is about
    assert torch.equal(res[0][2].view(torch.int32), res[1][2].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    ref = _FakeTower(_HALF_TOTAL, [(0, _HALF_TOTAL)], _HALF_TRAINABLE, seed=9)
    chunk = torch.nn.Parameter(ref.flat[:64 * 2].clone())
    topt = torch.optim.AdamW([chunk], lr=1e-2, weight_decay=1e-2)
    for step in range(2):
        chunk.grad = (sum(_half_grad(step, r) for r in range(world)) / world)[:64 * 2].clone()
        G = float(chunk.grad.double().norm())
        norm, coef = (float(x) for x in res[0][2][step])
        assert abs(norm - G) <= 2.0 ** -22 * G and G > _MAX_NORM and abs(coef - _MAX_NORM / (G + 1e-6)) <= 1e-6
        torch.nn.utils.clip_grad_norm_([chunk], _MAX_NORM)
        topt.step()
    for r in res:
        assert torch.allclose(r[1][:64 * 2], chunk.detach(), rtol=1e-5, atol=1e-6), r[0]
        assert torch.equal(r[1][64 * 2:], ref.flat[64 * 2:])
