"""The conditions tests/test_loss_exact_gpu.py rests on, checked without a GPU and without the library's kernels: its float64 closed form
agrees with float64 autograd of the oracle; an honest f32 evaluation (oracle.LossOracle in float32 on the CPU) stays within half of every
bound; the undecided hinge pairs stay under their caps; the bounds are tight enough that every wrong kernel of `WRONGS` leaves them
somewhere; the column slices are the ones the docstring names; and the host refuses what it must before any launch.  The builders draw
with a CPU generator, so the numbers here are the numbers of the GPU run."""
import ctypes

import pytest
import torch

import oracle
import test_loss_exact_gpu as lx

F64 = torch.float64


def _oracle(B, E, cfg, dtype):
    """oracle.LossOracle / oracle.clip_forward on the case's inputs in `dtype` -> (loss, {slot: raw term value}, [gradients])"""
    e = {k: v.to(dtype) for k, v in lx.inputs(B, E).items()}
    names = [n for n in lx.NAMES if cfg.w[n] != 0]
    lc = oracle.LossOracle(names, {n: cfg.w[n] * len(names) for n in names}, temperature=cfg.tau, percent={n: 1 / len(names) for n in names})
    si, st = e['si'].clone().requires_grad_(True), e['st'].clone().requires_grad_(True)
    if cfg.two:
        loss, res = lc(oracle.clip_forward({'last_representation': si}, {'last_representation': st}),
                       oracle.clip_forward({'last_representation': e['ti']}, {'last_representation': e['tt']}), 'all')
    else:
        loss, res = lc({'last_representation': si}, {'last_representation': e['ti']}, 'image')
    loss.backward()
    slots = {}
    for n in names:
        raw = lambda key: res[key].detach().double() / lc.loss_scale[n]
        if n in lx.CROSS:
            slots[lx.SLOT[n]] = raw(n)
        elif cfg.two:
            slots[lx.SLOT[n]], slots[lx.SLOT[n] + 4] = raw('image_' + n), raw('text_' + n)
        else:
            slots[lx.SLOT[n]] = raw(n)
    return loss.detach().double(), slots, [x.grad.double() for x in ((si, st) if cfg.two else (si,))]


@pytest.mark.parametrize('B,E', lx.SWEEP)
def test_closed_form_is_the_oracle_and_f32_stays_within_half_of_every_bound(B, E):
    worst = 0.0
    for cfg in lx.configs():
        ref = lx.reference(B, E, cfg)
        val, bnd = ref.share()
        # (a) float64 autograd of the oracle: the closed form is the same function
        loss, slots, grads = _oracle(B, E, cfg, F64)
        for tow, g in enumerate(grads):
            assert (g - ref.g[tow]).abs().max() <= 1e-9 * ref.g[tow].abs().max() + 1e-300, (cfg.what, tow)
        for slot, v in slots.items():
            assert torch.isnan(v) == torch.isnan(val[slot]) and not abs(v - val[slot]) > 1e-10 * abs(v) + 1e-300, (cfg.what, slot, v, val[slot])
        assert torch.isnan(loss) == torch.isnan(val[0]) and not abs(loss - val[0]) > 1e-10 * abs(loss), (cfg.what, loss, val[0])
        assert torch.isnan(val[0]) == (B == 1 and cfg.two and cfg.w['cos_diff'] != 0)
        # (b) the same in float32: half of every bound, the hinge allowance apart
        loss, slots, grads = _oracle(B, E, cfg, torch.float32)
        for tow, g in enumerate(grads):
            err = (g - ref.g[tow]).abs()
            assert (err <= 0.5 * ref.gb[tow] + ref.gh[tow]).all(), (cfg.what, tow, (err / (0.5 * ref.gb[tow] + ref.gh[tow])).max())
            worst = max(worst, ((err - ref.gh[tow]).clamp(min=0) / ref.gb[tow]).max().item())
        for slot, v in list(slots.items()) + [(0, loss)]:
            if not torch.isnan(val[slot]):
                assert abs(v - val[slot]) <= 0.5 * bnd[slot], (cfg.what, slot, v, val[slot], bnd[slot])
        assert (val[13:] == 0).all() and (bnd[13:] == 0).all()
    assert worst <= 0.5
    print(f'B={B} E={E}: the f32 oracle uses at most {worst:.4f} of a gradient bound')


def test_inputs_hold_their_conditions():
    for B, E in lx.SWEEP:
        e = lx.inputs(B, E)
        assert all(v.dtype == torch.float32 and v.shape == (B, E) for v in e.values())
        n, ri, rt, (d_on, d_off, o_on, o_off) = lx.hinge_counts(e)
        assert n <= 0.005 * B * B and ri <= 0.1 * B and rt <= 0.1 * B, (B, E, n, ri, rt)
        if B >= 2:
            for v in e.values():
                norm = v.double().norm(dim=1)
                assert norm.max() / norm.min() >= 100, (B, E)
        if B >= 15:                                          # both hinge branches on and off the diagonal
            assert min(d_on, d_off, o_on, o_off) >= 1, (B, E, d_on, d_off, o_on, o_off)
    assert lx.inputs(130, 1024) is lx.inputs(130, 1024)


def test_cases_reach_the_slices_the_docstring_names():
    assert [lx.slice_tiles(B, B) for B in (1, 16)] == [[(0, 1)], [(0, 1)]]
    assert lx.slice_tiles(17, 17) == [(0, 1), (1, 2)] and 17 - 16 == 1
    assert lx.slice_tiles(33, 33) == lx.slice_tiles(40, 40) == [(0, 1), (1, 2), (2, 3)]
    want = [(z, z + 1) for z in range(7)] + [(7, 9)]
    assert all(lx.slice_tiles(130, rows) == want for rows in (130, 8, 53, 60, 69, 1)) and 130 - 8 * 16 == 2
    assert {(E + 255) // 256 for _, E in lx.SWEEP} == {1, 2, 3, 4}
    assert sorted(sum(lx.PARTITION, ())[::2]) == [0, 8, 61, 69, 129] and sum(r for _, r in lx.PARTITION) == 130
    assert all(a + r == b for (a, r), (b, _) in zip(lx.PARTITION, lx.PARTITION[1:]))
    assert len(lx.SWEEP) == 30 and len(lx.configs()) == 17


ALONE = lambda n, tau=None, two=True: lx.Cfg({n: 1.0}, tau, two)
SENSITIVITY = [
    # (wrong kernel, B, E, configuration at which it must leave a bound)
    ('cd_b2', 2, 48, ALONE('cos_diff')), ('cd_b2', 17, 768, ALONE('cos_diff')), ('cd_b2', 130, 1024, ALONE('cos_diff')),
    ('cd_swap', 17, 48, ALONE('cos_diff')), ('cd_swap', 130, 768, ALONE('cos_diff')),
    ('hl_rowstat', 17, 48, ALONE('hard_label')), ('hl_rowstat', 130, 768, ALONE('hard_label')),
    ('sl_rowstat', 17, 48, ALONE('soft_label', 0.5)), ('sl_rowstat', 130, 768, ALONE('soft_label', 2.0)),
    ('kl_scalar_tau', 17, 48, ALONE('out_kl', 0.5)), ('kl_scalar_tau', 17, 768, ALONE('out_kl', 2.0, False)),
    ('kl_grad_tau2', 17, 48, ALONE('out_kl', 2.0)), ('kl_grad_tau2', 130, 768, ALONE('out_kl', 0.5, False)),
    ('sl_scalar_tau', 17, 48, ALONE('soft_label', 0.5)), ('sl_scalar_tau', 130, 768, ALONE('soft_label', 2.0)),
    ('sl_grad_tau2', 17, 48, ALONE('soft_label', 2.0)), ('sl_grad_tau2', 130, 768, ALONE('soft_label', 0.5)),
    ('ce_no_b', 2, 48, ALONE('out_ce')), ('ce_no_b', 130, 768, ALONE('out_ce', None, False)),
    ('tower_no_half', 17, 48, ALONE('out_l1')), ('tower_no_half', 17, 768, ALONE('out_cos')), ('tower_no_half', 130, 48, ALONE('out_kl', 2.0)),
    ('tower_no_half', 130, 768, ALONE('out_ce')),
    ('last_col_twice', 17, 48, ALONE('cos_diff')), ('last_col_twice', 130, 768, ALONE('logits_mse')),
    ('last_col_twice', 130, 1024, ALONE('hard_label')), ('last_col_twice', 33, 768, ALONE('soft_label', 0.5)),
    ('tile_lost', 17, 48, ALONE('logits_mse')), ('tile_lost', 130, 768, ALONE('hard_label')), ('tile_lost', 40, 768, ALONE('cos_diff')),
    ('slice_lost', 17, 48, ALONE('cos_diff')), ('slice_lost', 130, 768, ALONE('soft_label', 2.0)), ('slice_lost', 130, 1024, ALONE('logits_mse')),
    ('no_projection', 17, 48, ALONE('logits_mse')), ('no_projection', 130, 768, ALONE('hard_label')), ('no_projection', 2, 768, ALONE('cos_diff')),
    ('neighbour_inv', 2, 48, ALONE('logits_mse')), ('neighbour_inv', 130, 768, ALONE('cos_diff')), ('neighbour_inv', 17, 1024, ALONE('soft_label', 0.5)),
]


def test_every_wrong_kernel_leaves_a_bound():
    """the bounds are tight enough: each of these float64 "wrong references" has at least one value outside the right one's bound, at
    EVERY case listed for it (the issue asks for at least one)"""
    assert {w for w, *_ in SENSITIVITY} == set(lx.WRONGS)
    hidden = [m for m in (lx.insensitive(B, E, cfg, wrong) for wrong, B, E, cfg in SENSITIVITY) if m]
    assert not hidden, '\n'.join(hidden)


def test_all_terms_case_is_sensitive_too():
    """within the weighted mixture of all eight terms at B = 130 the same mistakes still leave the bounds: per-element bounds do not
    have the blind spot of a max-norm tolerance (cos_diff carries 0.125 of 8 terms here)"""
    cfg = lx.Cfg(lx.W_ALL, 0.5)
    hidden = [m for m in (lx.insensitive(130, 768, cfg, wrong) for wrong in lx.WRONGS) if m]
    assert not hidden, '\n'.join(hidden)


def test_sensitivity_check_can_fail():
    """the check itself: a mistake that changes nothing at the case (tau for tau^2 at tau = 1, a lost half in one-tower mode, the
    neighbour's norm at B = 1) is reported as hidden"""
    assert 'stays inside' in lx.insensitive(17, 48, ALONE('out_kl', 1.0), 'kl_scalar_tau')
    assert 'stays inside' in lx.insensitive(17, 48, ALONE('soft_label', 1.0), 'sl_grad_tau2')
    assert 'stays inside' in lx.insensitive(17, 48, ALONE('out_l1', None, False), 'tower_no_half')
    assert 'stays inside' in lx.insensitive(1, 48, ALONE('logits_mse'), 'neighbour_inv')


def test_leaves_bound_sees_one_element():
    """one gradient element moved by twice its bound, one statistic moved, one scalar moved: each is reported"""
    cfg = lx.Cfg(lx.W_ALL, 0.5)
    ref = lx.reference(17, 48, cfg)
    assert lx.leaves_bound(ref, ref) is None
    for what in ('grad', 'stat', 'scalar'):
        other = lx.Reference(lx.inputs(17, 48), cfg)
        if what == 'grad':
            other.g[1][16, 47] += 2 * (ref.gb[1] + ref.gh[1])[16, 47]
        elif what == 'stat':
            other.stats[5, 16] += 2 * ref.stats_b[5, 16]
        else:
            v, a, own = other.rows_of[12]
            other.rows_of[12] = (v + 2 * ref.share()[1][12] / 17, a, own)
        assert lx.leaves_bound(ref, other) is not None, what


# ----------------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks run on the host, before any launch (no GPU here)
# ----------------------------------------------------------------------------------------------------------------------------------
def _call(B=32, E=64, cfg=None, row0=None, rows=None, ws_short=0, ws_off=0, txt=True, gstats=None, stats_out=None):
    from distillclip_amd._lib import lib
    l = lib()
    cfg = cfg or lx.Cfg({'out_l1': 1.0, 'cos_diff': 1.0})
    arr = cfg.array()
    ws = l.dclip_distill_loss_workspace(B, E)
    p = 4096                                                # never dereferenced: the host refuses first
    t = p if txt else None
    if row0 is None:
        return l.dclip_distill_loss(p, p, t, t, B, E, ctypes.cast(arr, ctypes.c_void_p), p, p, t, 256 * 64 + ws_off, ws - ws_short, None)
    return l.dclip_distill_loss_rows(p, p, t, t, B, E, row0, rows, ctypes.cast(arr, ctypes.c_void_p), p, p, t, gstats, stats_out,
                                     256 * 64 + ws_off, ws - ws_short, None)


@pytest.mark.parametrize('kw,match', [
    (dict(E=24), 'E % 16'), (dict(E=1040), 'E <= 1024'), (dict(B=4097), 'B <= 4096'),
    (dict(row0=-1, rows=8), 'outside'), (dict(row0=30, rows=3), 'outside'), (dict(row0=32, rows=1), 'outside'), (dict(row0=0, rows=0), 'outside'),
    (dict(cfg=lx.Cfg({'out_kl': 1.0}, 0.0)), 'temperature'), (dict(cfg=lx.Cfg({'soft_label': 1.0}, 0.0)), 'temperature'),
    (dict(ws_short=1), 'workspace too small'), (dict(ws_off=16), '256-byte aligned'), (dict(txt=False), 'both towers'),
    (dict(row0=0, rows=16, cfg=lx.Cfg({'hard_label': 1.0})), 'statistics of every row'),
    # a statistics-only call that no kernel would answer: no cross-modal term, or one tower
    (dict(row0=0, rows=16, stats_out=4096, cfg=lx.Cfg({'out_l1': 1.0})), 'stats_out needs'),
    (dict(row0=0, rows=32, stats_out=4096, cfg=lx.Cfg({'out_l1': 1.0, 'hard_label': 1.0}, None, False), txt=False), 'stats_out needs'),
])
def test_host_refuses_before_any_launch(kw, match):
    """every other argument of `_call` is valid, and the message names the defect: the refusal is this defect's and not another's"""
    with pytest.raises(ValueError, match=match):
        _call(**kw)

