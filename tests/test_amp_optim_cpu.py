"""FusedAdamW as an optimizer torch.amp.GradScaler.step() drives directly (optim.py; include/dclip.h: dclip_amp_prepare,
dclip_adamw_multi_amp): what can be pinned without a GPU — the protocol attributes, the library surface, the refusal under the sharded
exchange, and the step count a state dict carries after skipped steps, with the two substitution points `_prepare` / `_adamw_amp`
restated in torch as tests/test_parallel_cpu.py restates `_adamw`."""
import pytest
import torch

from distillclip_amd.optim import FusedAdamW


class _FakeTower:
    """flat buffers and parameter layout of a tower, without the HIP runtime (tests/test_parallel_cpu.py's, less the buckets)"""

    def __init__(self, total, trainable, seed):
        self.flat = torch.randn(total, generator=torch.Generator().manual_seed(seed))
        self.flat_grad = torch.zeros(total)
        self._trainable = trainable
        self.sync = self.dp = self.gshard = None
        self.wcache_dirty = False
        self.grads_ready = self.opt_done = self.bwd_stream = None
        self._grad_clean = False
        edges = sorted({0, total} | {e for r in trainable for e in r})
        self._offsets = edges[:-1]
        self._plist = [self.flat[a:b] for a, b in zip(edges[:-1], edges[1:])]      # one "parameter" per segment

    def _params(self):
        return self._plist

    def trainable_ranges(self):
        return [list(r) for r in self._trainable]


_TOTAL, _TRAINABLE = 64 * 10, [[64 * 2, 64 * 5], [64 * 6, 64 * 10]]              # frozen: [0, 128) and [320, 384)
_REC = dict(mult=0, skip=1, bc1=2, bc2_sqrt=3, norm=4, coef=5)


def _torch_prepare(self, found_inf, grad_scale, partials, extra, record, skipped, st):
    """torch restatement of dclip_amp_prepare without clipping"""
    assert partials is None and extra is None
    skip = found_inf is not None and float(found_inf) != 0.0
    skipped += int(skip)
    t = self.step_count - int(skipped)
    record.zero_()
    record[_REC['mult']] = 1.0 / (float(grad_scale) if grad_scale is not None else 1.0)
    record[_REC['skip']] = float(skip)
    record[_REC['bc1']] = 1 - self.betas[0] ** t
    record[_REC['bc2_sqrt']] = (1 - self.betas[1] ** t) ** 0.5
    record[_REC['coef']] = 1.0


def _torch_adamw_amp(self, p, g, m, v, zero_grad, st, record):
    """torch restatement of dclip_adamw_multi_amp"""
    if not float(record[_REC['skip']]):
        b1, b2 = self.betas
        gs = g * record[_REC['mult']]
        p.mul_(1.0 - self.lr * self.weight_decay)
        m.mul_(b1).add_(gs, alpha=1 - b1)
        v.mul_(b2).addcmul_(gs, gs, value=1 - b2)
        p.addcdiv_(m, (v.sqrt() / record[_REC['bc2_sqrt']]).add_(self.eps), value=-self.lr / float(record[_REC['bc1']]))
    if zero_grad:
        g.zero_()


@pytest.fixture
def torch_kernels(monkeypatch):
    monkeypatch.setattr(FusedAdamW, '_prepare', _torch_prepare)
    monkeypatch.setattr(FusedAdamW, '_adamw_amp', _torch_adamw_amp)


def _opt(**kw):
    tw = _FakeTower(_TOTAL, _TRAINABLE, seed=5)
    g0 = torch.Generator().manual_seed(6)
    extras = [torch.nn.Parameter(torch.randn(8, 4, generator=g0)), torch.nn.Parameter(torch.randn(4, generator=g0), requires_grad=False),
              torch.nn.Parameter(torch.randn(8, generator=g0))]
    return tw, extras, FusedAdamW([tw], lr=1e-2, weight_decay=1e-2, extra_params=extras, **kw)


def test_interface_attributes():
    tw, extras, opt = _opt()
    assert FusedAdamW._step_supports_amp_scaling is True and opt._step_supports_amp_scaling is True
    groups = opt.param_groups
    assert len(groups) == 1
    g = groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (1e-2, (0.9, 0.999), 1e-8, 1e-2)
    params, slots = g['params'], opt._slots()
    assert len(params) == len(slots) == 2 + 2                          # two trainable segments of the tower, then the two trainable extras
    for p, (owner, off, n, shape) in zip(params, slots):
        assert p.numel() == n and tuple(p.shape) == shape
        if off is None:
            assert p is owner
        else:
            assert owner is tw and p.data_ptr() == tw.flat[off:].data_ptr()
    assert params[2] is extras[0] and params[3] is extras[2]           # extras last, the frozen one left out
    opt.lr = 0.5                                                       # opt.lr stays the knob, the group shows it
    assert opt.param_groups[0]['lr'] == 0.5
    with pytest.raises(AttributeError):
        opt.param_groups = []
    assert not hasattr(opt, 'grad_scale') and not hasattr(opt, 'found_inf')        # the scaler's to set and to delete


def test_header_declares_and_library_exports_the_new_entries():
    from distillclip_amd._lib import _HEADER, _parse_header, lib
    protos = _parse_header(_HEADER)
    l = lib()
    for name, nargs in (('dclip_amp_prepare', 12), ('dclip_adamw_multi_amp', 14)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert getattr(l._dll, name) is not None                       # (AttributeError if the library lacks the symbol)
    assert len(protos['dclip_adamw_multi_scaled'][1]) == 15 and len(protos['dclip_clip_coef'][1]) == 6
    assert l.dclip_version() == 6                                      # additive: no existing signature changed
    from distillclip_amd import ops
    text = open(_HEADER).read()
    assert f'#define DCLIP_AMP_RECORD_FLOATS {ops.AMP_RECORD_FLOATS}\n' in text
    for name in ('MULT', 'SKIP', 'BC1', 'BC2_SQRT', 'NORM', 'COEF'):
        assert f'#define DCLIP_AMP_{name} {getattr(ops, "AMP_" + name)}\n' in text
        assert getattr(ops, 'AMP_' + name) == _REC[name.lower()]


class _Sync:
    enabled = True


def test_a_scale_under_the_sharded_exchange_is_refused_before_anything_runs(monkeypatch):
    tw, extras, opt = _opt()
    tw.sync, tw.dp = _Sync(), object()                                 # what FusedAdamW._sharded asks for
    assert opt._sharded(tw)
    ran = []
    for name in ('_jobs', '_adamw_many', '_amp_record', '_clip_coef', '_step_sharded', '_extra_items'):
        monkeypatch.setattr(FusedAdamW, name, lambda self, *a, _n=name, **k: ran.append(_n) or [])
    before = tw.flat.clone()
    for attrs in (dict(grad_scale=torch.tensor(65536.0)), dict(found_inf=torch.tensor(0.0)),
                  dict(grad_scale=torch.tensor(2.0), found_inf=torch.tensor(0.0))):
        for k, v in attrs.items():
            setattr(opt, k, v)
        with pytest.raises(RuntimeError) as e:
            opt.step()
        assert 'DCLIP_DP_MODE=allreduce' in str(e.value) and 'DCLIP_DP_MODE=off' in str(e.value) and 'precision: 16' in str(e.value)
        for k in attrs:
            delattr(opt, k)
    assert ran == [] and opt.step_count == 0 and torch.equal(tw.flat, before)
    opt.step()                                                         # no scale, no flag: the sharded step is taken as before
    assert ran and ran[0] == '_jobs' and opt.step_count == 1


def test_state_dict_carries_the_steps_taken_not_the_calls(torch_kernels):
    """five calls, the second and the fourth with found_inf set: weights and moments are those of three steps of torch.optim.AdamW on
    the three good gradients, 'step' is 3, and a loaded optimizer continues at step 4 with its skipped count at zero"""
    tw, extras, opt = _opt()
    params = opt.param_groups[0]['params']
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    scale = 1024.0
    gen = torch.Generator().manual_seed(9)
    mask = torch.zeros(_TOTAL, dtype=torch.bool)
    for a, b in _TRAINABLE:
        mask[a:b] = True

    def one_step(o, t, bad, with_ref):
        g = torch.randn(_TOTAL, generator=gen) * mask
        ge = [torch.randn(extras[0].shape, generator=gen), torch.randn(extras[2].shape, generator=gen)]
        t.flat_grad.copy_(g * scale)
        for p, x in zip((o.extras[0], o.extras[1]), ge):
            p.grad = x * scale
        if with_ref and not bad:
            for r, (owner, off, n, shape) in zip(ref, o._slots()):
                r.grad = (ge[0] if r.shape == ge[0].shape else ge[1]).clone() if off is None else g[off:off + n].clone()
            topt.step()
        o.grad_scale, o.found_inf = torch.tensor(scale), torch.tensor(float(bad))
        o.step(zero_grad=True)
        del o.grad_scale, o.found_inf
        assert float(t.flat_grad.abs().max()) == 0.0 and all(float(p.grad.abs().max()) == 0.0 for p in o.extras)

    for call in range(5):
        one_step(opt, tw, call in (1, 3), True)
    assert opt.step_count == 5 and int(opt._skipped) == 2
    for r, p in zip(ref, params):
        assert torch.allclose(p.detach(), r.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(tw.flat[~mask], _FakeTower(_TOTAL, _TRAINABLE, seed=5).flat[~mask])
    sd = opt.state_dict()
    tsd = topt.state_dict()
    assert sd['state'].keys() == tsd['state'].keys()
    for i, st in sd['state'].items():
        assert float(st['step']) == 3.0 == float(tsd['state'][i]['step'])
        assert torch.allclose(st['exp_avg'], tsd['state'][i]['exp_avg'], rtol=1e-5, atol=1e-7)
        assert torch.allclose(st['exp_avg_sq'], tsd['state'][i]['exp_avg_sq'], rtol=1e-5, atol=1e-9)
    assert 'max_grad_norm' not in sd['param_groups'][0] and 'skipped' not in sd and 'grad_scale' not in sd['param_groups'][0]

    tw2, extras2, opt2 = _opt()
    tw2.flat.copy_(tw.flat)
    for a, b in zip(extras2, extras):
        a.data.copy_(b.data)
    opt2._skipped = torch.tensor([7])                                  # (a counter left over from before the load)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3 and int(opt2._skipped) == 0
    opt.load_state_dict(sd)                                            # the same into the optimizer that wrote it
    assert opt.step_count == 3 and int(opt._skipped) == 0 and opt._steps_taken() == 3
    state = gen.get_state()
    one_step(opt, tw, False, True)                                     # step 4 in all three
    gen.set_state(state)
    extras_of_opt = opt.extras
    one_step(opt2, tw2, False, False)
    assert torch.equal(tw2.flat, tw.flat) and all(torch.equal(a.data, b.data) for a, b in zip(opt2.extras, extras_of_opt))
    for r, p in zip(ref, params):
        assert torch.allclose(p.detach(), r.detach(), rtol=1e-5, atol=1e-6)
    assert float(opt.state_dict()['state'][0]['step']) == 4.0
