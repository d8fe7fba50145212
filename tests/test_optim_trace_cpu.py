"""What FusedAdamW.step() asks of its nine hooks, call by call, and in which order it refuses: recorded once and held to the recording
(tests/golden/optim_step_trace.json).  On the CPU, without the library: every hook is a spy that writes down its name and the shape of its
arguments, on the stand-in towers of tests/test_adamw_groups_cpu.py; the refusals come from the real class, before anything is launched.
A change to optim.py that moves, adds, drops or re-orders a launch, or hands one another lr / weight_decay / step, shows here.

`python tests/test_optim_trace_cpu.py --write` records the fixture; it is written once, from the code the comparison is to be held to, and
not again afterwards."""
import itertools
import json
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_adamw_groups_cpu import SIZES, _FakeTower                # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'optim_step_trace.json')
HOOKS = ('_adamw', '_sumsq', '_coef', '_prepare', '_adamw_amp', '_adamw_ema', '_swap', '_adamw_table', '_lamb_table')
KINDS = ('plain', 'groups', 'trust', 'groups+trust')


def _describe(x):
    """a tensor as its element count, lists recursively, numbers / None / bools as they are, anything else as its class name"""
    if isinstance(x, torch.Tensor):
        return x.numel()
    if isinstance(x, (list, tuple)):
        return [_describe(y) for y in x]
    if x is None or isinstance(x, (bool, int, float)):
        return x
    return type(x).__name__


def _spy(name):
    def hook(self, *args):
        described = _describe(args)
        if name == '_lamb_table':                                  # (its first argument is id(tower or extra parameter): named, to be repeatable)
            described[0] = self.labels[args[0]]
        self.trace.append([name, described, self.lr, self.weight_decay, self.step_count])
        if name == '_lamb_table':
            return torch.zeros(len(args[2]), 4)
    return hook


def _spy_class():
    from distillclip_amd.optim import FusedAdamW
    return type('Spy', (FusedAdamW,), {name: _spy(name) for name in HOOKS})


def _trace_of(clip, amp, ema, kind, with_extras, zero_grad):
    """the hook calls of two steps of one case"""
    towers = [_FakeTower(SIZES, 1), _FakeTower(SIZES[:3], 2)]
    extras = []
    if with_extras:
        extras = [torch.nn.Parameter(torch.ones(8)), torch.nn.Parameter(torch.ones(2, 4)), torch.nn.Parameter(torch.ones(4))]
        extras[0].grad, extras[1].grad = torch.ones(8), torch.ones(2, 4)           # (the third has no gradient)
    groups = None
    if 'groups' in kind:
        P = towers[0]._params()
        groups = [{'params': [P[1], P[3]] + extras[:1], 'weight_decay': 0.0}, {'params': [P[5]], 'lr_scale': 0.5}]
    opt = _spy_class()(towers, lr=1e-3, weight_decay=0.05, extra_params=extras, max_grad_norm=1.0 if clip else None, ema_decay=0.9 if ema else None,
                       groups=groups, trust_ratio='trust' in kind)
    opt.trace = []
    opt.labels = {id(tw): f'tower {i}' for i, tw in enumerate(towers)}
    opt.labels.update((id(p), f'extra {j}') for j, p in enumerate(extras))
    for _ in range(2):
        if amp:                                                    # as torch.amp.GradScaler.step() does around the call
            opt.found_inf, opt.grad_scale = torch.zeros(1), torch.tensor(8.0)
        opt.step(zero_grad=zero_grad)
        if amp:
            del opt.found_inf, opt.grad_scale
    assert opt.step_count == 2
    return opt.trace


def _traces():
    out = {}
    for clip, amp, ema, kind, extras, zg in itertools.product((0, 1), (0, 1), (0, 1), KINDS, (0, 1), (0, 1)):
        out[f'clip{clip} amp{amp} ema{ema} {kind} extras{extras} zero_grad{zg}'] = _trace_of(clip, amp, ema, kind, extras, bool(zg))
    return out


# ---- the order of refusals: the real class, nothing substituted ------------------------------------------------------------------------------------
FEATURES = ('amp', 'clip', 'ema', 'bad ema_decay', 'groups', 'trust')


def _no_launch(*a, **k):
    raise AssertionError('a step that had to be refused reached the library')


def _refusal_of(features, sharded, monkeypatch):
    """-> [exception type, its message with every address masked] of one step of the real FusedAdamW over one tower that has a
    7-element trainable range; asserts that the step counter did not move"""
    from distillclip_amd import ops, optim
    monkeypatch.setattr(optim, 'lib', _no_launch)                  # (a safety net, not a substitution: no case here may get this far)
    monkeypatch.setattr(ops, 'lib', _no_launch)
    tw = _FakeTower([(64, True), (64, False), (7, True), (1, False), (64, True)], 3, pad=1)
    assert tw.trainable_ranges() == [[0, 64], [128, 135], [136, 200]]
    if sharded:
        tw.dp = types.SimpleNamespace(shard_elems=8, buckets=[])
        tw.sync = types.SimpleNamespace(enabled=True, stream_for=_no_launch, group_for=_no_launch)
    opt = optim.FusedAdamW([tw], max_grad_norm=1.0 if 'clip' in features else None,
                           ema_decay=1.5 if 'bad ema_decay' in features else 0.9 if 'ema' in features else None,
                           groups=[{'params': [tw._params()[2]], 'weight_decay': 0.0}] if 'groups' in features else None, trust_ratio='trust' in features)
    if 'amp' in features:
        opt.found_inf, opt.grad_scale = torch.zeros(1), torch.tensor(8.0)
    with pytest.raises((ValueError, RuntimeError)) as err:
        opt.step()
    assert opt.step_count == 0 and opt._state == {} and opt._ema == {} and opt._tables == {}
    return [err.type.__name__, re.sub(r'0x[0-9a-f]+', '0x?', str(err.value))]


def _refusal_cases():
    """every feature alone and every pair of features, on a plain and on a sharded tower (a sharded tower's ranges are the exchange
    plan's, so clipping alone refuses nothing there)"""
    for sharded in (False, True):
        for n in (1, 2):
            for features in itertools.combinations(FEATURES, n):
                if {'ema', 'bad ema_decay'} <= set(features) or (sharded and features == ('clip',)):
                    continue
                yield ('sharded: ' if sharded else '') + ' + '.join(features), features, sharded


def _refusals(monkeypatch):
    return {name: _refusal_of(features, sharded, monkeypatch) for name, features, sharded in _refusal_cases()}


# ---- the comparison -------------------------------------------------------------------------------------------------------------------------------
def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _through_json(x):
    return json.loads(json.dumps(x))


def test_every_hook_call_of_every_kind_of_step_is_the_recorded_one():
    want, got = _recorded()['trace'], _through_json(_traces())
    assert list(got) == list(want) and len(got) == 128
    for name in want:
        assert got[name] == want[name], name
    assert sum(len(t) for t in got.values()) == sum(len(t) for t in want.values())
    assert {rec[0] for t in got.values() for rec in t} == set(HOOKS) - {'_swap'}           # (step() exchanges nothing: ema_weights() does)


def test_the_refusals_come_in_the_recorded_order(monkeypatch):
    want, got = _recorded()['refusals'], _through_json(_refusals(monkeypatch))
    assert list(got) == list(want) and len(got) == 39
    for name in want:
        assert got[name] == want[name], name
    # every pair of {clip, EMA, groups, trust} is there, by the first 80 characters and by the whole text
    for pair in itertools.combinations(('clip', 'ema', 'groups', 'trust'), 2):
        assert got[' + '.join(pair)][1][:80] == want[' + '.join(pair)][1][:80]


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/test_optim_trace_cpu.py --write')
    patch = pytest.MonkeyPatch()
    try:
        recorded = {'trace': _traces(), 'refusals': _refusals(patch)}
    finally:
        patch.undo()
    with open(FIXTURE, 'w') as f:
        json.dump(recorded, f, separators=(',', ':'))
    print(f"{len(recorded['trace'])} cases, {sum(len(t) for t in recorded['trace'].values())} hook calls, {len(recorded['refusals'])} refusals, "
          f'{os.path.getsize(FIXTURE)} bytes -> {FIXTURE}')
