"""Host side of AdamW with per-range hyper-parameters: the three C entries' declarations and refusals (they return before anything touches
the device; dclip_adamw_table_fill is host code altogether), FusedAdamW(groups=...)'s refusals and bookkeeping on stand-in towers with
a torch version of the table kernel (the way tests/test_ema_cpu.py rehearses the EMA), and the kernel's tile-to-range lookup emulated
at every tile edge of the cases tests/test_adamw_groups_gpu.py runs."""
import copy
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import adamw_groups_cases as gc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_header_states_the_roundings_and_the_library_exports_the_entries():
    from distillclip_amd import _lib as binding
    src = open(binding._HEADER).read()
    for pat in (r'size_t\s+dclip_adamw_table_bytes\s*\(', r'int\s+dclip_adamw_table_fill\s*\(', r'int\s+dclip_adamw_table\s*\(',
                r'#define\s+DCLIP_ADAMW_TABLE_TILE\s+8192', r'lr_k = lr \* lr_scale_k, ONE f32 product', r'bit for bit', r'No atomics: the same call gives the same',
                r'no cap of DCLIP_ADAMW_MAX_RANGES', r'A refusal writes neither the image'):
        assert re.search(pat, src), pat
    lib = _lib()
    res, args = lib.protos['dclip_adamw_table']
    assert res is ctypes.c_int and len(args) == 18 and args[6] is ctypes.c_int32 and args[7] is ctypes.c_int64 and args[14] is ctypes.c_float
    res, args = lib.protos['dclip_adamw_table_fill']
    assert res is ctypes.c_int and len(args) == 9
    assert lib.protos['dclip_adamw_table_bytes'] == (ctypes.c_size_t, [ctypes.c_int32])
    for name in ('dclip_adamw_table', 'dclip_adamw_table_fill', 'dclip_adamw_table_bytes', 'dclip_adamw_multi', 'dclip_adamw_multi_ema'):
        assert getattr(lib._dll, name) is not None
    assert lib.dclip_version() == 6
    assert [lib.dclip_adamw_table_bytes(c) for c in (-1, 0, 1, 70)] == [0, 0, 64, 71 * 32]
    from distillclip_amd import ops
    assert ops.ADAMW_TABLE_TILE == gc.TILE == 8192 and ops.ADAMW_MAX_RANGES == 24


def _fill(begin, length, scale, wd, total, count=None, image='own', nbytes=None, tiles='own'):
    """-> (image bytes after the call as uint8, tiles after the call); raises what the entry raises, after checking it wrote nothing"""
    lib = _lib()
    n = len(length if begin is None else begin) if count is None else count
    arr = lambda xs, ct: None if xs is None else (ct * max(len(xs), 1))(*xs)
    buf = np.full(32 * (max(n, 0) + 2), 0xA5, dtype=np.uint8)
    out = ctypes.c_int64(-77)
    args = (arr(begin, ctypes.c_int64), arr(length, ctypes.c_int64), arr(scale, ctypes.c_float), arr(wd, ctypes.c_float), n, total,
            buf.ctypes.data + (4 if image == 'odd' else 0) if image is not None else None, buf.size - 32 if nbytes is None else nbytes,
            ctypes.byref(out) if tiles is not None else None)
    try:
        lib.dclip_adamw_table_fill(*args)
    except ValueError:
        assert (buf == 0xA5).all() and out.value == -77, 'a refused fill wrote something'
        raise
    return buf, out.value


def test_fill_writes_the_image_the_kernel_reads():
    for count in gc.COUNTS:
        ranges, total = gc.ranges_of(count)
        buf, tiles = _fill(*zip(*ranges), total)
        rec = buf[:32 * (count + 1)].view(gc.RECORD)
        tile0 = gc.tile0_of(ranges)
        assert tiles == tile0[-1] and rec['tile0'].tolist() == tile0
        assert rec['begin'][:count].tolist() == [r[0] for r in ranges] and rec['length'][:count].tolist() == [r[1] for r in ranges]
        assert np.array_equal(rec['lr_scale'][:count], np.float32([r[2] for r in ranges])) and np.array_equal(rec['weight_decay'][:count], np.float32([r[3] for r in ranges]))
        assert rec['length'][count] == 0 and (buf[32 * (count + 1):] == 0xA5).all()                  # nothing past the closing record
    # two ranges that touch, a range that ends exactly at `total`, lr_scale = 0
    _fill([0, 8], [8, 4], [0.0, 1.0], [0.0, 0.1], 12)


def test_every_host_refusal_of_dclip_adamw_table_fill():
    ok = dict(begin=[8, 64, 4096], length=[8, 1028, 8196], scale=[1.0, 0.1, 0.0], wd=[0.0, 0.01, 0.3], total=4096 + 8196)
    _fill(**ok)
    inf, nan = float('inf'), float('nan')
    cases = {
        'bad argument': [dict(begin=None), dict(length=None), dict(scale=None), dict(wd=None), dict(image=None), dict(tiles=None), dict(count=0), dict(count=-1), dict(total=0)],
        '128 bytes on an 8-byte boundary': [dict(image='odd'), dict(nbytes=127), dict(nbytes=0)],
        'range 1 must be non-empty': [dict(length=[8, 0, 8196]), dict(length=[8, -4, 8196]), dict(length=[8, 1030, 8196]), dict(begin=[8, 66, 4096])],
        'range 0 must be non-empty': [dict(begin=[-4, 64, 4096]), dict(begin=[2, 64, 4096])],
        'range 1 begins at .* ascend and do not overlap': [dict(begin=[8, 12, 4096]), dict(begin=[8, 4, 4096]), dict(begin=[64, 8, 4096])],
        'range 2 begins at': [dict(begin=[8, 64, 64 + 1024])],
        'range 2 ends past the stated total': [dict(total=4096 + 8192), dict(total=4096)],
        'range 1 needs a finite lr_scale >= 0': [dict(scale=[1.0, -0.1, 0.0]), dict(scale=[1.0, nan, 0.0]), dict(scale=[1.0, inf, 0.0]), dict(wd=[0.0, nan, 0.3]),
                                                 dict(wd=[0.0, -inf, 0.3])],
    }
    for match, bads in cases.items():
        for bad in bads:
            with pytest.raises(ValueError, match='dclip_adamw_table_fill: .*' + match):
                _fill(**dict(ok, **bad))


A0 = 0x10000                                                     # addresses that are never read: every call below is refused on the host


def test_every_host_refusal_of_dclip_adamw_table():
    lib = _lib()
    ok = dict(p=A0, g=2 * A0, m=3 * A0, v=4 * A0, e=5 * A0, table=6 * A0, count=3, tiles=5, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, zero_grad=0, w=0.5,
              gscale=None, record=None, stream=None)
    cases = {
        'bases 16-byte aligned': [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(p=A0 + 4), dict(g=2 * A0 + 8), dict(m=3 * A0 + 12), dict(v=4 * A0 + 4),
                                  dict(e=5 * A0 + 4)],
        'a device table on an 8-byte boundary, count >= 1': [dict(table=None), dict(table=6 * A0 + 4), dict(count=0), dict(count=-3)],
        'tiles for 3 ranges': [dict(tiles=2), dict(tiles=0), dict(tiles=-1), dict(tiles=2 ** 31)],
        'exclude each other': [dict(gscale=7 * A0, record=8 * A0)],
        r'ema_weight .* \[0, 1\]': [dict(w=-1e-6), dict(w=1.0 + 2.0 ** -20), dict(w=float('nan')), dict(w=float('inf'))],
        'record of dclip_amp_prepare, or step >= 1': [dict(step=0), dict(step=-5), dict(record=8 * A0 + 4), dict(record=8 * A0 + 8, step=0)],
    }
    for match, bads in cases.items():
        for bad in bads:
            a = dict(ok, **bad)
            with pytest.raises(ValueError, match='dclip_adamw_table: .*' + match):
                lib.dclip_adamw_table(*[a[k] for k in ok])


# ---- the kernel's lookup ---------------------------------------------------------------------------------------------------------------------------
def test_the_tile_lookup_at_every_tile_edge_of_the_gpu_cases():
    """workgroup t -> (range, first element, elements): the bisection over the table's tile0 column, emulated on the very image
    dclip_adamw_table_fill writes, must cover every range exactly once, tile by tile, and nothing else"""
    for count in gc.COUNTS:
        ranges, total = gc.ranges_of(count)
        buf, tiles = _fill(*zip(*ranges), total)
        tile0 = buf[:32 * (count + 1)].view(gc.RECORD)['tile0'].tolist()
        covered = np.zeros(total, dtype=np.int32)
        edges = set()
        for k in range(count):
            edges |= {tile0[k], tile0[k + 1] - 1, max(tile0[k] - 1, 0), min(tile0[k] + 1, tiles - 1)}
        for t in range(tiles):                                    # (every tile: the longest case has 70 ranges in about 90 tiles)
            k, first, n = gc.tile_span(ranges, tile0, t)
            assert k == int(np.searchsorted(tile0, t, side='right')) - 1 and 0 <= k < count
            b, length = ranges[k][:2]
            assert b <= first and first + n <= b + length and 0 < n <= gc.TILE and n % 4 == 0 and (first - b) % gc.TILE == 0
            assert n == gc.TILE or first + n == b + length         # only a range's last tile is short
            covered[first:first + n] += 1
            edges.discard(t)
        assert not edges and np.array_equal(covered, gc.inside_mask(ranges, total).astype(np.int32))
    ranges, _ = gc.ranges_of(70)
    assert max(r[1] for r in ranges) == 24580 and gc.tile0_of([(0, 24580, 1, 0)]) == [0, 4] and gc.tile0_of([(0, 8192, 1, 0), (8192, 8196, 1, 0)]) == [0, 1, 3]


# ---- FusedAdamW on stand-in towers --------------------------------------------------------------------------------------------------------------
class _FakeTower:
    """flat buffers of a tower whose parameters are given as (numel, trainable): each starts a segment of its size rounded up to 64
    elements, as a tower's do (tests/test_ema_cpu.py's stand-in, with a parameter list that is not derived from the ranges)"""

    def __init__(self, sizes, seed, pad=64):
        offs = [0]
        for n, _ in sizes:
            offs.append(offs[-1] + (n + pad - 1) // pad * pad)
        g = torch.Generator().manual_seed(seed)
        self.flat = torch.randn(offs[-1], generator=g)
        self.flat_grad = torch.randn(offs[-1], generator=g)
        self._offsets = offs[:-1]
        self._plist = [self.flat[o:o + n] for o, (n, _) in zip(offs, sizes)]
        self._flags = [t for _, t in sizes]
        self._ends = offs[1:]
        self.sync = self.dp = self.gshard = None
        self.wcache_dirty = False
        self.grads_ready = self.opt_done = self.bwd_stream = None
        self._grad_clean = False

    def _params(self):
        return self._plist

    def trainable_ranges(self):
        out = []
        for off, end, t in zip(self._offsets, self._ends, self._flags):
            if t:
                if out and out[-1][1] == off:
                    out[-1][1] = end
                else:
                    out.append([off, end])
        return out


def _torch_table(self, tw, bufs, ranges, zero_grad, st, ema_weight, gscale, record):
    """dclip_adamw_table, plain or clipped, in torch: per range torch.optim.AdamW's step with lr * lr_scale and the range's decay"""
    assert record is None
    self.table_calls = getattr(self, 'table_calls', []) + [list(ranges)]
    p, g, m, v, e = bufs
    b1, b2 = self.betas
    for a, b, s, wd in ranges:
        gs = g[a:b] if gscale is None else g[a:b] * gscale
        p[a:b].mul_(1.0 - self.lr * s * wd)
        m[a:b].mul_(b1).add_(gs, alpha=1 - b1)
        v[a:b].mul_(b2).addcmul_(gs, gs, value=1 - b2)
        bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
        p[a:b].addcdiv_(m[a:b], (v[a:b].sqrt() / bc2 ** 0.5).add_(self.eps), value=-self.lr * s / bc1)
        if e is not None:
            e[a:b].add_(p[a:b] - e[a:b], alpha=ema_weight)
        if zero_grad:
            g[a:b].zero_()


def _torch_adamw(self, p, g, m, v, zero_grad, st, *scale):
    b1, b2 = self.betas
    p.mul_(1.0 - self.lr * self.weight_decay)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
    p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(self.eps), value=-self.lr / bc1)


def _rehearsal():
    from distillclip_amd.optim import FusedAdamW

    class Rehearsal(FusedAdamW):
        _adamw_table, _adamw = _torch_table, _torch_adamw
    return Rehearsal


# parameter:  0 w    1 b   2 w(frozen) 3 b    4 gain 5 w     6 b
SIZES = [(256, True), (64, True), (128, False), (60, True), (64, True), (640, True), (10, True)]
#  offsets:   0        256         320           448         512         576          1216   -> 1280


def _tower(seed=1):
    return _FakeTower(SIZES, seed)


def test_range_cutting_on_a_hand_written_layout():
    from distillclip_amd.optim import FusedAdamW
    tw = _tower()
    P = tw._params()
    assert tw._offsets == [0, 256, 320, 448, 512, 576, 1216] and tw.trainable_ranges() == [[0, 320], [448, 1280]]
    cut = lambda groups, **kw: FusedAdamW([tw], weight_decay=0.05, groups=groups, **kw)._group_ranges(tw)
    # no declared group at all: the fixed ranges, the frozen gap splits
    assert cut([]) == [(0, 320, 1.0, 0.05), (448, 1280, 1.0, 0.05)]
    # biases and the gain undecayed: weights and biases alternate, neighbours that are equal merge (3 b with 4 gain), padding goes with its parameter
    assert cut([{'params': [P[1], P[3], P[4], P[6]], 'weight_decay': 0.0}]) == [(0, 256, 1.0, 0.05), (256, 320, 1.0, 0.0), (448, 576, 1.0, 0.0), (576, 1216, 1.0, 0.05),
                                                                                  (1216, 1280, 1.0, 0.0)]
    # two declared groups with the same values merge with each other, and with the default group where they equal it
    assert cut([{'params': [P[0]], 'lr_scale': 0.5}, {'params': [P[1]], 'lr_scale': 0.5}, {'params': [P[5]], 'weight_decay': 0.05, 'lr_scale': 1.0}]) == \
        [(0, 320, 0.5, 0.05), (448, 1280, 1.0, 0.05)]
    # equal values on both sides of the frozen gap do not merge across it
    assert cut([{'params': [P[1], P[3]], 'lr_scale': 0.1, 'weight_decay': 0.0}]) == [(0, 256, 1.0, 0.05), (256, 320, 0.1, 0.0), (448, 512, 0.1, 0.0), (512, 1280, 1.0, 0.05)]
    # a group without 'weight_decay' follows the optimizer's
    opt = FusedAdamW([tw], weight_decay=0.05, groups=[{'params': [P[5]], 'lr_scale': 3.0}])
    opt.weight_decay = 0.2
    assert opt._group_ranges(tw) == [(0, 320, 1.0, 0.2), (448, 576, 1.0, 0.2), (576, 1216, 3.0, 0.2), (1216, 1280, 1.0, 0.2)]


def test_the_constructor_refuses():
    from distillclip_amd.optim import FusedAdamW
    tw = _tower()
    P = tw._params()
    extra = torch.nn.Parameter(torch.zeros(4, 4))
    frozen_extra = torch.nn.Parameter(torch.zeros(4), requires_grad=False)
    mk = lambda groups: FusedAdamW([tw], extra_params=[extra, frozen_extra], groups=groups)
    mk([{'params': [P[0], extra], 'weight_decay': 0, 'lr_scale': 0}, {'params': P[1]}])                      # (zeros and a bare tensor are fine)
    cases = {
        r'in groups\[0\] and in groups\[1\]': [[{'params': [P[0]]}, {'params': [P[1], P[0]]}]],
        r'in groups\[0\] and in groups\[0\]': [[{'params': [P[0], P[0]]}]],
        r'groups\[0\] names a parameter of shape \(128,\) that this optimizer does not update': [[{'params': [P[2]]}]],
        r'groups\[1\] names a parameter of shape \(4,\)': [[{'params': [P[0]]}, {'params': [frozen_extra]}]],
        r'groups\[0\] names a parameter of shape \(3,\)': [[{'params': [torch.nn.Parameter(torch.zeros(3))]}]],
        r"groups\[0\]\['weight_decay'\] must be a finite number >= 0": [[{'params': [P[0]], 'weight_decay': x}] for x in (-1e-3, float('nan'), float('inf'), 'x', True)],
        r"groups\[1\]\['lr_scale'\] must be a finite number >= 0": [[{'params': [P[0]]}, {'params': [P[1]], 'lr_scale': x}] for x in (-1.0, float('nan'), float('inf'), None)],
        r"groups\[0\] has unknown key\(s\) \['betas'\]": [[{'params': [P[0]], 'betas': (0.9, 0.99)}]],
        r"groups\[0\] has unknown key\(s\) \['lr'\]": [[{'params': [P[0]], 'lr': 1e-3}]],
        r"groups\[0\] must be a dict with a 'params' list": [[{'weight_decay': 0.0}], [[P[0]]]],
    }
    for match, bads in cases.items():
        for bad in bads:
            with pytest.raises(ValueError, match='FusedAdamW: .*' + match):
                mk(bad)
    with pytest.raises(TypeError):
        FusedAdamW([tw], group=[])


def test_an_odd_range_is_refused_before_the_step_counter_moves():
    from distillclip_amd.optim import FusedAdamW
    tw = _FakeTower([(64, True), (7, True), (64, True)], 3, pad=1)                 # a layout without padding: the cut lands on an odd range
    P = tw._params()
    opt = FusedAdamW([tw], groups=[{'params': [P[1]], 'weight_decay': 0.0}])       # the product hook: nothing is launched, the refusal comes first
    before = tw.flat.clone()
    with pytest.raises(ValueError, match=r'tower 0 range \[64, 71\) has 7 elements.*parameter groups \(dclip_adamw_table\)'):
        opt.step()
    assert opt.step_count == 0 and opt._state == {} and opt._tables == {} and torch.equal(tw.flat, before)
    tw = _FakeTower([(66, True), (64, True)], 3, pad=1)                            # a multiple of 4 elements, 8 bytes off a 16-byte boundary
    opt = FusedAdamW([tw], groups=[{'params': [tw._params()[1]], 'lr_scale': 0.1}])
    with pytest.raises(ValueError, match=r'tower 0 range \[0, 66\)'):
        opt.step()
    assert opt.step_count == 0
    # a value spoiled after construction is refused the same way
    tw = _tower()
    opt = _rehearsal()([tw], groups=[{'params': [tw._params()[0]], 'weight_decay': 0.0}])
    opt.groups[0]['weight_decay'] = -1.0
    with pytest.raises(ValueError, match=r"groups\[0\]\['weight_decay'\]"):
        opt.step()
    assert opt.step_count == 0 and opt._state == {}


def test_a_sharded_tower_is_refused_before_the_step_counter_moves():
    tw = _tower(4)

    def boom(*a, **k):
        raise AssertionError('the refusal must come before anything else')
    tw.dp = types.SimpleNamespace(shard_elems=8, buckets=[])
    tw.sync = types.SimpleNamespace(enabled=True, stream_for=boom, group_for=boom)
    opt = _rehearsal()([tw], groups=[{'params': [tw._params()[1]], 'weight_decay': 0.0}])
    assert opt._sharded(tw)
    with pytest.raises(RuntimeError, match=r'parameter groups.*sharded.*DCLIP_DP_MODE=allreduce.*DCLIP_DP_MODE=off'):
        opt.step()
    assert opt.step_count == 0 and opt._state == {} and opt._tables == {}


def _grouped(seed=1, **kw):
    tw = _tower(seed)
    P = tw._params()
    extra = [torch.nn.Parameter(torch.randn(8, 4, generator=torch.Generator().manual_seed(7))), torch.nn.Parameter(torch.randn(8, generator=torch.Generator().manual_seed(8)))]
    groups = [{'params': [P[6], P[1], P[3], P[4], extra[1]], 'weight_decay': 0.0}, {'params': [P[5]], 'lr_scale': 0.1}]
    return tw, extra, _rehearsal()([tw], lr=1e-2, weight_decay=0.05, extra_params=extra, groups=groups, **kw)


def test_the_param_groups_picture():
    from distillclip_amd.optim import EpochCosineSchedule
    tw, extra, opt = _grouped()
    P = tw._params()
    pg = opt.param_groups
    assert len(pg) == 3 and [g['lr_scale'] for g in pg] == [1.0, 0.1, 1.0] and [g['weight_decay'] for g in pg] == [0.0, 0.05, 0.05]
    assert [[id(p) for p in g['params']] for g in pg] == [[id(P[6]), id(P[1]), id(P[3]), id(P[4]), id(extra[1])], [id(P[5])], [id(P[0]), id(extra[0])]]
    ids = [id(p) for g in pg for p in g['params']]
    assert len(ids) == len(set(ids)) and ids == [id(p) for p in opt._trainable()] and id(P[2]) not in ids                 # disjoint, their union the trainable set
    assert [tuple(s[3]) for s in opt._slots()] == [tuple(p.shape) for p in opt._trainable()]
    sched = EpochCosineSchedule(opt, 2, 10)
    for _ in range(4):
        assert [g['lr'] for g in opt.param_groups] == [opt.lr, opt.lr * 0.1, opt.lr] and all(g['betas'] == (0.9, 0.999) for g in opt.param_groups)
        sched.step()
    assert 0 < opt.lr < 1e-2
    # without groups: the one group there has always been
    from distillclip_amd.optim import FusedAdamW
    plain = FusedAdamW([tw], lr=1e-2, weight_decay=0.05, extra_params=extra)
    assert plain.groups is None and len(plain.param_groups) == 1 and set(plain.param_groups[0]) == {'params', 'lr', 'betas', 'eps', 'weight_decay'}
    assert [id(p) for p in plain.param_groups[0]['params']] == [id(P[i]) for i in (0, 1, 3, 4, 5, 6)] + [id(e) for e in extra]


def _twin(opt, lr=1e-2):
    cpu = [torch.nn.Parameter(p.detach().clone()) for p in opt._trainable()]
    groups, at = [], 0
    for g in opt.param_groups:
        groups.append({'params': cpu[at:at + len(g['params'])], 'lr': g['lr'], 'weight_decay': g['weight_decay'], 'lr_scale': g['lr_scale']})
        at += len(g['params'])
    return cpu, torch.optim.AdamW(groups, lr=lr, weight_decay=0.05)


def _mask(tw):
    m = torch.zeros(tw.flat.numel(), dtype=torch.bool)
    for o, p, t in zip(tw._offsets, tw._params(), tw._flags):
        m[o:o + p.numel()] = t
    return m


def test_steps_and_the_state_dict_layout_against_torch_adamw():
    tw, extra, opt = _grouped()
    cpu, ref = _twin(opt)
    frozen = tw.flat[320:448].clone()
    for step in range(3):
        g = torch.Generator().manual_seed(20 + step)
        tw.flat_grad.copy_(torch.randn(tw.flat.numel(), generator=g) * _mask(tw))
        for x in extra:
            x.grad = torch.randn(x.shape, generator=g)
        for c, p in zip(cpu, opt._trainable()):
            c.grad = (p.grad if p.grad is not None else tw.flat_grad[(p.data_ptr() - tw.flat.data_ptr()) // 4:][:p.numel()].view(p.shape)).clone()
        if step == 2:                                             # a changed value takes effect at the next step, and only then is the table rebuilt
            opt.groups[1]['lr_scale'] = 0.5
            ref.param_groups[1]['lr'] = opt.lr * 0.5
        opt.step()
        ref.step()
        for c, p in zip(cpu, opt._trainable()):
            assert torch.allclose(p.detach(), c.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(tw.flat[320:448], frozen) and len(opt.table_calls) == 3
    assert opt.table_calls[0] == opt.table_calls[1] == [(0, 256, 1.0, 0.05), (256, 320, 1.0, 0.0), (448, 576, 1.0, 0.0), (576, 1216, 0.1, 0.05), (1216, 1280, 1.0, 0.0)]
    assert opt.table_calls[2][3] == (576, 1216, 0.5, 0.05)
    sd, tsd = opt.state_dict(), ref.state_dict()
    assert len(sd['param_groups']) == 3 and [g['params'] for g in sd['param_groups']] == [g['params'] for g in tsd['param_groups']] == [[0, 1, 2, 3, 4], [5], [6, 7]]
    for g, t in zip(sd['param_groups'], tsd['param_groups']):
        assert g['lr'] == t['lr'] and g['weight_decay'] == t['weight_decay'] and g['betas'] == t['betas'] and g['eps'] == t['eps']
    assert [g['lr_scale'] for g in sd['param_groups']] == [1.0, 0.5, 1.0] and sd['param_groups'][1]['initial_lr'] == opt.base_lr * 0.5
    assert set(sd['state']) == set(tsd['state']) == set(range(8))
    for i in range(8):
        assert float(sd['state'][i]['step']) == 3.0 and sd['state'][i]['exp_avg'].shape == tsd['state'][i]['exp_avg'].shape
        assert torch.allclose(sd['state'][i]['exp_avg'], tsd['state'][i]['exp_avg'], rtol=1e-5, atol=1e-7)
        assert torch.allclose(sd['state'][i]['exp_avg_sq'], tsd['state'][i]['exp_avg_sq'], rtol=1e-5, atol=1e-9)
    # into a fresh torch optimizer built with [*groups, {'params': rest}], and torch's own dict back into a fresh FusedAdamW
    cpu2, ref2 = _twin(opt, lr=77.0)
    ref2.load_state_dict(sd)
    assert [g['lr'] for g in ref2.param_groups] == [g['lr'] for g in sd['param_groups']] and ref2.param_groups[1]['lr_scale'] == 0.5
    back = copy.deepcopy(ref2.state_dict())
    for c in cpu2:
        c.grad = torch.zeros_like(c)
    ref2.step()                                                   # (torch steps on what it loaded)
    tw3, extra3, opt3 = _grouped()
    opt3.load_state_dict(back)
    assert opt3.step_count == 3 and opt3.lr == opt.lr and opt3.weight_decay == 0.05 and [g['lr_scale'] for g in opt3.groups] == [1.0, 0.5]
    assert [g['weight_decay'] for g in opt3.groups] == [0.0, 0.05]
    for a, b in zip(opt._moments(tw), opt3._moments(tw3)):
        assert torch.equal(a[_mask(tw)], b[_mask(tw)])
    # another number of groups is refused, both counts named
    from distillclip_amd.optim import FusedAdamW
    plain = FusedAdamW([_tower()], extra_params=extra3)
    with pytest.raises(ValueError, match=r'3 parameter group\(s\), this optimizer 1'):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match=r'1 parameter group\(s\), this optimizer 3 \(2 declared'):
        opt3.load_state_dict(plain.state_dict())
    assert opt3.step_count == 3


def test_an_ema_step_and_the_extras_per_distinct_pair():
    tw, extra, opt = _grouped(ema_decay=0.75)
    seen = []

    def spy(self, items, zero_grad, st, ema_weight, gscale, record):
        seen.append((len(items), self.lr, self.weight_decay, ema_weight))
    type(opt)._adamw_ema = spy
    for x in extra:
        x.grad = torch.ones_like(x)
    start = tw.flat.clone()
    opt.step()
    f32 = lambda x: float(np.float32(x))
    assert seen == [(1, f32(f32(1e-2) * f32(1.0)), 0.05, 0.25), (1, f32(1e-2), 0.0, 0.25)] and opt.lr == 1e-2 and opt.weight_decay == 0.05
    e = opt._ema[id(tw)]
    want = start.double() + 0.25 * (tw.flat.double() - start.double())
    assert torch.allclose(e.double(), want, rtol=1e-6, atol=1e-7) and torch.equal(e[320:448], start[320:448])


# ---- the helper and the model attribute ------------------------------------------------------------------------------------------------------------
def test_no_decay_groups_and_the_model_attribute():
    from distillclip_amd.model._distill_base import DistillBase
    from distillclip_amd.optim import no_decay_groups
    assert DistillBase.optimizer_groups is None

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_embed = torch.nn.Parameter(torch.zeros(5, 8))
            self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, 8))
            self.fc = torch.nn.Linear(8, 8)
            self.norm = torch.nn.LayerNorm(8)
            self.frozen_bias = torch.nn.Parameter(torch.zeros(8), requires_grad=False)
            self.proj = torch.nn.Linear(8, 4)

        def no_weight_decay(self):
            return {'pos_embed', 'cls_token'}

        def extra_parameters(self):
            return list(self.proj.parameters())

    enc, bare = Enc(), torch.nn.Linear(4, 4)
    tower = lambda mod, skip=(): types.SimpleNamespace(module=mod, _params=lambda: [None] + [p for n, p in mod.named_parameters() if not n.startswith('proj.')])
    model = types.SimpleNamespace(towers=lambda: [tower(enc), tower(bare)])
    (g,) = no_decay_groups(model)
    assert set(g) == {'params', 'weight_decay'} and g['weight_decay'] == 0.0
    want = [enc.pos_embed, enc.cls_token, enc.fc.bias, enc.norm.weight, enc.norm.bias, enc.proj.bias, bare.bias]
    assert [id(p) for p in g['params']] == [id(p) for p in want]
