"""The stream contract of the C ABI (include/dclip.h: "`stream` is a hipStream_t passed as void*.  No synchronisation inside any entry
point, no allocation, no global mutable state on the compute path") and of the Python layer above it, on the cases of
tests/stream_cases.py: every stream-taking entry.

  reference : the case run eagerly on the default stream, on buffers of its own, and synchronised.  Computed once per (case, seed).
  blocker   : torch.cuda._sleep on a side stream `s`: one thread that spins, the rest of the GPU stays free.  Calibrated once per process
              with events; BLOCK_MS long.
  control   : once per module.  While `s` is held by the blocker, a plain torch copy issued on the default stream completes before the
              blocker's event does.  HIP maps streams onto a few hardware queues; two streams that share one would make every ordering
              check blind.  Up to eight torch.cuda.Stream() are tried, the first that passes is kept, and for check C the first two that are
              independent of each other as well.  Without such streams the checks skip, saying so; they never pass without the control.
  A  ordering and no host wait.  Before anything else: index operands real, value operands zero, outputs and workspace zero.  On `s`: the
     blocker, ONE device copy that brings in the real value operands and fills outputs and workspace with 0xFF, the entry, an event.  When
     the entry returns the blocker's event is still unfinished (otherwise the case FAILS as inconclusive: the entry made the host wait, or
     the blocker was too short).  After s.synchronize() every buffer but the workspace equals the reference as stream_cases.py says, and
     the 0xFF guards around every buffer are intact.  A launch issued elsewhere runs while the blocker holds `s`: a reader sees zeros, an
     initialiser is overwritten by the 0xFF fill; either way the final bits differ.
  B  HOST arrays are consumed by the call.  As A; as soon as the call returns every host array is overwritten: pointers with pointers
     to decoy buffers of the same size, numbers with other valid numbers.  The result equals the reference, the decoys are bit-unchanged,
     and every on_bucket callback of dclip_encoder_backward has fired before the call returned.
  C  two calls in flight.  Two instances of a case (two seeds, own buffers and workspace) on two side streams released together,
     alternating three times, each compared with its own serial reference; the towers on one handle with two workspaces, and the image
     and text tower at once.
  D  the Python layer.  Under `with torch.cuda.stream(s)` behind the blocker, the fused loss, LossCalculator with its backward, a student
     forward and backward through the module and FusedAdamW.step in six forms return while the blocker runs and agree with their
     default-stream run.

No test can make a kernel fault, even a misrouted one: index operands are valid from the first moment and withheld values are zeros.
No child processes, three streams at most; after a HIP error the session ends.

Blocker: BLOCK_MS = 150.  On an MI355X the longest return time of any call was 0.9 to 1.9 ms over the runs made (LossCalculator with its backward; the tower case's four
entries together 0.6 ms), so no case was inconclusive; the control held for the first two of eight side streams and nothing was skipped; the
file's 190 tests ran in 35 s, none above 0.6 s (test_zz_report prints the figures of a run; the assertions, not these numbers, validate the
blocker's length).
"""
import contextlib
import time

import pytest
import torch

import stream_cases as sc
import tower_memory_cases as tm

pytestmark = pytest.mark.gpu

GUARD = 4096                   # bytes of 0xFF on each side of every buffer
BLOCK_MS = 150.0
U8 = torch.uint8
_STATE = dict(cycles_per_ms=None, longest=(0.0, None), t0=time.perf_counter(), runs=0)
_BUILD = sc.builders()
NAMES = [name for name, _, _ in sc.TABLE]
HOST_NAMES = [name for name, entries, _ in sc.TABLE if set(entries) & set(sc.HOST_ARRAY_ENTRIES)]


# ---- blocker and control --------------------------------------------------------------------------------------------------------------------
def _cycles():
    if _STATE['cycles_per_ms'] is None:
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(20_000_000)
        e1.record()
        e1.synchronize()
        _STATE['cycles_per_ms'] = 20_000_000 / e0.elapsed_time(e1)
    return int(_STATE['cycles_per_ms'] * BLOCK_MS)


def _block(s):
    """the blocker on `s` -> the event behind it"""
    with torch.cuda.stream(s):
        torch.cuda._sleep(_cycles())
        ev = torch.cuda.Event()
        ev.record()
    return ev


def _independent(holder, other):
    """while `holder` is held by the blocker, does a plain copy on `other` (None: the default stream) complete before the blocker?"""
    src = torch.arange(4096, device='cuda', dtype=torch.float32)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    evb = _block(holder)
    with (torch.cuda.stream(other) if other is not None else contextlib.nullcontext()):
        dst.copy_(src)
        evc = torch.cuda.Event()
        evc.record()
    evc.synchronize()
    ok = not evb.query()
    torch.cuda.synchronize()
    return ok and bool(torch.equal(dst, src))


@pytest.fixture(scope='module')
def streams():
    """(s1, s2): side streams for which the control holds; s2 is None when no second one is independent of s1 as well"""
    cands = [torch.cuda.Stream() for _ in range(8)]
    good = [s for s in cands if _independent(s, None)]
    if not good:
        pytest.skip('control failed: none of eight side streams leaves the default stream free while the blocker holds it (they share a '
                    'hardware queue): the ordering checks would be blind')
    s1 = good[0]
    s2 = next((s for s in good[1:] if _independent(s1, s) and _independent(s, s1)), None)
    print(f'control: stream {cands.index(s1)} of 8 holds' + ('' if s2 is None else f', stream {cands.index(s2)} is independent of it'))
    return s1, s2


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    if _STATE.get('dead'):
        pytest.fail('not run: an earlier check ended with a HIP error')
    yield


# ---- buffers --------------------------------------------------------------------------------------------------------------------------------
def _layout(c):
    off, pos = {}, GUARD
    for b in c.bufs.values():
        off[b.name] = pos
        pos += (b.nbytes + 255) // 256 * 256 + GUARD
    return off, pos


def _images(c, off, total):
    """-> (the bytes before anything is released, the bytes the entry's own stream brings in), both with 0xFF between the buffers"""
    init = torch.full((total,), 0xFF, dtype=U8)
    go = torch.full((total,), 0xFF, dtype=U8)
    for b in c.bufs.values():
        lo, hi = off[b.name], off[b.name] + b.nbytes
        init[lo:hi] = b.bytes() if b.role == 'index' else 0
        if b.role in ('index', 'value'):
            go[lo:hi] = b.bytes()
    return init, go


class Rig:
    def __init__(self, c, decoys=False):
        self.c = c
        self.off, self.total = _layout(c)
        init, go = _images(c, self.off, self.total)
        self.arena = torch.empty(self.total, dtype=U8, device='cuda')
        assert self.arena.data_ptr() % 256 == 0
        self.arena.copy_(init)
        self.go = go.cuda()
        self.ptr = {k: self.arena.data_ptr() + v for k, v in self.off.items()}
        self.harr = c.make_host(self.ptr)
        self.decoy, self.decoy_ptr = {}, {}
        if decoys:
            for k in c.host_pointed():
                self.decoy[k] = torch.full((c.bufs[k].nbytes,), 0x5A, dtype=U8, device='cuda')
                self.decoy_ptr[k] = self.decoy[k].data_ptr()
        torch.cuda.synchronize()

    def release_and_call(self, stream_handle):
        """on the current stream: bring the operands in, fill outputs and workspace with 0xFF, call the entry -> host seconds of the call"""
        self.arena.copy_(self.go)
        t0 = time.perf_counter()
        self.c.call(self.ptr, self.harr, stream_handle)
        return time.perf_counter() - t0

    def result(self):
        return self.arena                  # (stays on the device: a tower's workspace is 100 MB)


def _guarded(fn, what):
    try:
        return fn()
    except (AssertionError, ValueError):
        raise
    except Exception as exc:           # a HIP error: every later launch of this process would fail too
        _STATE['dead'] = True
        pytest.exit(f'stream contract: {what} raised {exc!r}', returncode=3)


_REF = {}


def _reference(name, seed):
    """the case on the default stream, on buffers of its own -> (arena bytes, gradient classes of a tower case or None)"""
    key = (name, seed)
    if key not in _REF:
        def run():
            c = _BUILD[name](seed)
            rig = Rig(c)
            rig.release_and_call(None)
            torch.cuda.synchronize()
            return c, rig, rig.result()
        c, rig, a = _guarded(run, f'reference of {key}')
        for b in c.bufs.values():                   # the comparison is not vacuous: the entry wrote every output it declares
            if b.role == 'out':
                assert bool((a[rig.off[b.name]:rig.off[b.name] + b.nbytes] != 0xFF).any()), f'{name}: the reference run left `{b.name}` as it was'
        classes = None
        if c.grad_rule is not None:
            _, _, b = _guarded(run, f'second reference of {key}')
            buf, mod = c.grad_rule
            classes = tm.grad_classes(mod, _view(c, rig.off, a, buf), _view(c, rig.off, b, buf))
        _REF[key] = (a, classes)
    return _REF[key]


def _view(c, off, arena, name):
    b = c.bufs[name]
    return arena[off[name]:off[name] + b.nbytes].clone().view(b.data.dtype).view(b.data.shape)


def _compare(c, off, got, want, classes, what):
    """-> what differs between a run and the reference"""
    bad = []
    mask = torch.ones(got.numel(), dtype=torch.bool, device=got.device)
    for b in c.bufs.values():
        mask[off[b.name]:off[b.name] + b.nbytes] = False
    hit = mask & (got != 0xFF)
    if hit.any():
        bad.append(f'{what}: {int(hit.sum())} guard bytes changed, first at arena offset {int(torch.nonzero(hit)[0])} (buffers at {off})')
    for b in c.bufs.values():
        if b.role == 'work':
            continue
        g, w = _view(c, off, got, b.name), _view(c, off, want, b.name)
        if c.grad_rule is not None and b.name == c.grad_rule[0]:
            bad += tm.grad_failures(classes, g, w, f'{what}: {b.name}')
        elif b.noise is not None:
            tol = 2 * b.noise * 2.0 ** -24 * (w.abs().max().item() + 1)
            err = (g.double() - w.double()).abs()
            if not bool(torch.isfinite(g).all()) or err.max().item() > tol:
                bad.append(f'{what}: {b.name} (a sum of f32 atomics, {b.noise} addends): max |got - want| {err.max().item():.3e} > {tol:.3e}, '
                           f'or not finite: got {g.reshape(-1)[:4].tolist()} want {w.reshape(-1)[:4].tolist()}')
        else:
            m = tm.bits_differ(g, w, f'{what}: {b.name} ({b.role})')
            if m:
                bad.append(m)
    return bad


def _note(name, dt):
    _STATE['runs'] += 1
    if dt > _STATE['longest'][0]:
        _STATE['longest'] = (dt, name)


def _behind_the_blocker(name, seed, s, scramble):
    """checks A (scramble = False) and B (True) of one case -> problems"""
    want, classes = _reference(name, seed)

    def run():
        c = _BUILD[name](seed)
        rig = Rig(c, decoys=scramble)
        evb = _block(s)
        with torch.cuda.stream(s):
            dt = rig.release_and_call(s.cuda_stream)
            fired = None if c.fired is None else len(c.fired)
            if scramble:
                c.scramble_host(rig.harr, rig.decoy_ptr)
            held = not evb.query()
        s.synchronize()
        torch.cuda.synchronize()
        return c, rig, dt, fired, held
    c, rig, dt, fired, held = _guarded(run, f'case {name}')
    _note(name, dt)
    print(f'{name}: the call returned after {dt * 1e3:.2f} ms, blocker of {BLOCK_MS:.0f} ms ' + ('still running' if held else 'FINISHED'))
    bad = []
    if not held:
        bad.append(f'{name}: INCONCLUSIVE, counted as failed: the blocker had finished when the entry returned after {dt * 1e3:.2f} ms: the entry '
                   f'made the host wait, or the blocker of {BLOCK_MS:.0f} ms was too short')
    bad += _compare(c, rig.off, rig.result(), want, classes, name)
    if scramble:
        for k, d in rig.decoy.items():
            n = int((d != 0x5A).sum())
            if n:
                bad.append(f'{name}: {n} bytes of the decoy of `{k}` changed: a host pointer array was read after the call had returned')
        if c.fired is not None and fired != c.n_buckets:
            bad.append(f'{name}: {fired} of {c.n_buckets} on_bucket callbacks had fired when dclip_encoder_backward returned')
    return bad


def test_the_control_holds(streams):
    """the ordering checks below are evidence only on a run where this passes and nothing is skipped"""
    s1, s2 = streams
    assert s1 is not None
    if s2 is None:
        pytest.skip('control: no second side stream is independent of the first as well: check C cannot see two calls in flight')


@pytest.mark.parametrize('name', NAMES)
def test_a_the_entry_runs_on_its_stream_and_makes_no_host_wait(name, streams):
    bad = _behind_the_blocker(name, 0, streams[0], scramble=False)
    assert not bad, '\n'.join(bad[:12])


@pytest.mark.parametrize('name', HOST_NAMES)
def test_b_host_arrays_are_consumed_by_the_call(name, streams):
    c = _BUILD[name](0)
    assert c.host, f'{name}: the header documents HOST arrays for {c.entries}, the case declares none'
    bad = _behind_the_blocker(name, 0, streams[0], scramble=True)
    assert not bad, '\n'.join(bad[:12])


def _two_in_flight(pairs, s1, s2):
    """pairs: ((case name, seed), (case name, seed)), one per stream -> problems"""
    refs = [_reference(n, k) for n, k in pairs]

    def run():
        cs = [_BUILD[n](k) for n, k in pairs]
        rigs = [Rig(c) for c in cs]
        evb = _block(s1)
        s2.wait_event(evb)                         # both streams are released together, when the one blocker ends
        dts = [0.0, 0.0]
        for _ in range(3):
            for i, s in enumerate((s1, s2)):
                with torch.cuda.stream(s):
                    dts[i] = max(dts[i], rigs[i].release_and_call(s.cuda_stream))
        held = not evb.query()
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
        return cs, rigs, dts, held
    cs, rigs, dts, held = _guarded(run, f'cases {pairs} in flight together')
    bad = []
    if not held:
        bad.append(f'{pairs}: INCONCLUSIVE, counted as failed: the blocker had finished before both streams were issued (calls of up to '
                   f'{max(dts) * 1e3:.2f} ms): the two instances were not in flight together')
    for i, ((n, k), c, rig) in enumerate(zip(pairs, cs, rigs)):
        _note(n, dts[i])
        bad += _compare(c, rig.off, rig.result(), refs[i][0], refs[i][1], f'{n} (seed {k}, stream {i + 1} of 2)')
    return bad


@pytest.mark.parametrize('name', NAMES)
def test_c_two_calls_in_flight_share_nothing(name, streams):
    s1, s2 = streams
    if s2 is None:
        pytest.skip('control: no second side stream is independent of the first as well')
    bad = _two_in_flight(((name, 1), (name, 2)), s1, s2)
    assert not bad, '\n'.join(bad[:12])


def test_c_the_image_and_the_text_tower_in_flight_together(streams):
    s1, s2 = streams
    if s2 is None:
        pytest.skip('control: no second side stream is independent of the first as well')
    bad = _two_in_flight((('tower_img', 1), ('tower_txt', 1)), s1, s2)
    assert not bad, '\n'.join(bad[:12])


# ---- D: the Python layer --------------------------------------------------------------------------------------------------------------------
def _python_layer(s, make, what):
    """make() -> (release: [(withheld device tensor, its real values)], act: () -> {name: (tensor, noise or None)}).
    The reference releases and acts on the default stream; the check does both on `s` behind the blocker -> problems"""
    def run(stream):
        release, act = make()
        for dst, _ in release:
            with torch.no_grad():
                dst.zero_()
        torch.cuda.synchronize()
        evb = _block(stream) if stream is not None else None
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            with torch.no_grad():
                for dst, src in release:
                    dst.copy_(src)
            t0 = time.perf_counter()
            res = act()
            dt = time.perf_counter() - t0
            held = evb is None or not evb.query()
        torch.cuda.synchronize()
        return {k: (t.detach().clone(), n) for k, (t, n) in res.items()}, dt, held
    want, _, _ = _guarded(lambda: run(None), f'{what} on the default stream')
    got, dt, held = _guarded(lambda: run(s), f'{what} on a side stream')
    _note(what, dt)
    print(f'{what}: returned after {dt * 1e3:.2f} ms, blocker of {BLOCK_MS:.0f} ms ' + ('still running' if held else 'FINISHED'))
    bad = []
    if not held:
        bad.append(f'{what}: INCONCLUSIVE, counted as failed: the blocker had finished when the call returned after {dt * 1e3:.2f} ms: the Python '
                   f'layer made the host wait (an .item(), a blocking copy), or the blocker of {BLOCK_MS:.0f} ms was too short')
    assert set(got) == set(want)
    for k, (g, noise) in got.items():
        w = want[k][0]
        if callable(noise):
            bad += noise(g, w, f'{what}: {k}')
        elif noise is not None:
            tol = 2 * noise * 2.0 ** -24 * (w.abs().max().item() + 1)
            err = (g.double() - w.double()).abs().max().item()
            if not bool(torch.isfinite(g).all()) or err > tol:
                bad.append(f'{what}: {k} (a sum of f32 atomics, {noise} addends): |got - want| {err:.3e} > {tol:.3e}, or not finite')
        else:
            m = tm.bits_differ(g, w, f'{what}: {k}')
            if m:
                bad.append(m)
    return bad


LOSS_NAMES = ['out_l1', 'out_cos', 'cos_diff', 'soft_label', 'out_mse', 'icl', 'intra_kl']
D_B, D_E = 37, 64


def _embeddings(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(D_B, D_E, generator=g).cuda() for _ in range(4)]


def test_d_ops_distill_loss_keeps_the_contract(streams):
    from distillclip_amd import ops
    real = _embeddings(5)

    def make():
        live = [torch.zeros_like(t) for t in real]

        def act():
            out, d_i, d_t = ops.distill_loss(live[0], live[1], live[2], live[3], weights={'out_l1': 0.5, 'out_cos': 1.0, 'cos_diff': 1.0, 'soft_label': 1.0},
                                             temperature=0.07)
            return dict(scalars=(out, 16 * D_B), d_s_img=(d_i, None), d_s_txt=(d_t, None))
        return list(zip(live, real)), act
    bad = _python_layer(streams[0], make, 'ops.distill_loss')
    assert not bad, '\n'.join(bad[:12])


def test_d_loss_calculator_and_its_backward_keep_the_contract(streams):
    import types
    from distillclip_amd.model import LossCalculator
    lc = LossCalculator(LOSS_NAMES, {'icl': 0.5}, temperature=0.07)
    real = _embeddings(6)

    def make():
        live = [torch.zeros_like(t) for t in real]
        live[0].requires_grad_(True)
        live[2].requires_grad_(True)
        rep = lambda x: types.SimpleNamespace(last_representation=x)
        stu = types.SimpleNamespace(visual_output=rep(live[0]), text_output=rep(live[2]))
        tea = types.SimpleNamespace(visual_output=rep(live[1]), text_output=rep(live[3]))

        def act():
            loss, res = lc(stu, tea, 'all')
            loss.backward()
            out = {f'res[{k}]': (v.reshape(1), 16 * D_B) for k, v in res.items()}
            out.update(loss=(loss.reshape(1), 16 * D_B * len(LOSS_NAMES)), d_s_img=(live[0].grad, None), d_s_txt=(live[2].grad, None))
            return out
        return list(zip(live, real)), act
    bad = _python_layer(streams[0], make, 'LossCalculator')
    assert not bad, '\n'.join(bad[:12])


def _student(tag):
    from distillclip_amd import synth
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    if tag == 'img':
        m = RepeatVisionTransformer(**tm.S_IMG)
        m.load_state_dict(tm._T(synth.student_image_state(11, **tm.S_IMG)))
    else:
        m = RepeatTextTransformer(**tm.S_TXT)
        m.load_state_dict(tm._T(synth.student_text_state(11, **tm.S_TXT)))
    m = m.cuda()
    m._tower.materialize(torch.device('cuda', torch.cuda.current_device()))
    m._tower.attach_grads()
    return m


@pytest.mark.parametrize('tag', ['img', 'txt'])
def test_d_a_student_forward_and_backward_through_the_module_keep_the_contract(tag, streams):
    from distillclip_amd import synth
    from distillclip_amd.model.component import ControlOutput
    m = _student(tag)
    tw = m._tower
    B = 3
    if tag == 'img':
        x = torch.from_numpy(synth.images(77, B, tm.S_IMG['img_size'])).cuda()
    else:
        x = torch.from_numpy(synth.captions(77, B, tw.cfg.tokens, tm.S_TXT['vocab_size'], 3, tw.cfg.tokens - 5)).cuda()
    w = torch.randn(B, tw.cfg.out_dim, generator=torch.Generator().manual_seed(9)).cuda()
    grads = []

    def make():
        live_w = torch.zeros_like(w)
        live_x = torch.zeros_like(x) if tag == 'img' else x         # token ids are indices: never withheld
        release = [(live_w, w)] + ([(live_x, x)] if tag == 'img' else [])

        def act():
            tw.flat_grad.zero_()
            out = m(live_x, ControlOutput()).last_representation
            (out * live_w).sum().backward()
            return dict(last_representation=(out, None), flat_grad=(tw.flat_grad, rule))
        return release, act

    def rule(g, wnt, what):
        return tm.grad_failures(classes, g, wnt, what)
    # two default-stream runs say which weight gradients are reproducible (tower_memory_cases.grad_classes)
    for _ in range(2):
        rel, act = make()
        for dst, src in rel:
            dst.copy_(src)
        act()
        torch.cuda.synchronize()
        grads.append(tw.flat_grad.clone())
    classes = tm.grad_classes(tw, grads[0], grads[1])
    bad = _python_layer(streams[0], make, f'student {tag} forward + backward')
    assert not bad, '\n'.join(bad[:12])


OPT_FORMS = ('plain', 'clipped', 'scaler', 'groups', 'ema', 'trust')


@pytest.mark.parametrize('form', OPT_FORMS)
def test_d_fused_adamw_step_keeps_the_contract(form, streams):
    from distillclip_amd.optim import FusedAdamW
    SCALE = 1024.0
    total = _student('img')._tower.flat.numel()
    gen = torch.Generator().manual_seed(21)
    g1, g2 = (torch.randn(total, generator=gen).cuda() * 0.01 for _ in range(2))

    def make():
        m = _student('img')
        tw = m._tower
        kw = dict(lr=1e-3, weight_decay=0.01)
        if form == 'clipped':
            kw['max_grad_norm'] = 0.5
        if form == 'ema':
            kw['ema_decay'] = 0.9
        if form == 'groups':
            kw['groups'] = [{'params': [p for p in m.parameters() if p.requires_grad and p.dim() == 1], 'weight_decay': 0.0, 'lr_scale': 0.5}]
        if form == 'trust':
            kw['trust_ratio'] = True
        opt = FusedAdamW([tw], **kw)
        scaler = None
        mult = 1.0
        if form == 'scaler':
            scaler = torch.amp.GradScaler('cuda', init_scale=SCALE, growth_interval=1000)
            scaler.scale(torch.zeros(1, device='cuda'))
            mult = SCALE

        def step():
            if scaler is None:
                opt.step(zero_grad=True)
            else:
                scaler.step(opt)
                scaler.update()
        # the first step allocates the optimizer's state (moments, tables in pinned memory, the average): taken on the default stream
        tw.flat_grad.copy_(g1 * mult)
        step()
        opt.join()
        torch.cuda.synchronize()

        def act():
            step()
            res = dict(params=(tw.flat, None))
            for i, t in enumerate(opt._moments(tw)):
                res[f'moment{i}'] = (t, None)
            for k, t in opt._ema.items():
                res['ema'] = (t, None)
            for k, t in opt.last_trust_stats.items():
                res[f'trust_stats[{k}]'] = (t, None)
            if opt.last_grad_norm is not None:
                res['last_grad_norm'] = (opt.last_grad_norm, None)
            return res
        return [(tw.flat_grad, g2 * mult)], act
    bad = _python_layer(streams[0], make, f'FusedAdamW.step ({form})')
    assert not bad, '\n'.join(bad[:12])


def test_zz_report():
    """the figures the module docstring quotes: printed, not asserted (the assertions above are what validates the blocker's length)"""
    dt, name = _STATE['longest']
    print(f'stream contract: blocker {BLOCK_MS:.0f} ms; longest return time of any call {dt * 1e3:.2f} ms ({name}); {_STATE["runs"]} runs behind a blocker; '
          f'{time.perf_counter() - _STATE["t0"]:.1f} s since the module was imported')
    _REF.clear()
