"""The conditions tests/test_layernorm_exact_gpu.py rests on, checked without a GPU and without a kernel launch: its float64 closed forms
agree with float64 autograd of F.layer_norm; an honest f32 evaluation (the forward sums in the kernel's lane and chunk order, plain torch
f32 for the rest) stays within half of every bound on every case the GPU file runs; every wrong kernel of `WRONGS` leaves a bound, or
gives a non-finite value, on one of those cases; the inputs hold what the docstring says of them; and the host refuses what it must
before any launch.  The builders draw with a CPU generator, so the numbers here are the numbers of the GPU run."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_layernorm_exact_gpu as lx

F64, F32 = torch.float64, torch.float32
KINDS = ('usual', 'wide')


# ----------------------------------------------------------------------------------------------------------------------------------
# the closed forms are the function
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', lx.D_LIST)
def test_closed_forms_are_float64_autograd_of_layer_norm(D):
    for kind, eps in itertools.product(KINDS, lx.EPS_LIST):
        fr = lx.fwd_ref(D, False, kind, eps)
        dy, acc0, starts = lx.grads(D, False)
        x = fr.x.double().requires_grad_(True)
        g, b = fr.gamma.double().requires_grad_(True), fr.beta.double().requires_grad_(True)
        y = F.layer_norm(x, (D,), g, b, fr.eps)
        assert ((y.detach() - fr.y).abs() <= 1e-9 * fr.y.abs() + 1e-12 * fr.rstd[:, None] * x.detach().abs().max(1, keepdim=True).values).all()
        y.backward(dy.double())
        ref = lx.BwdRef(fr.x, fr.gamma, fr.mu, fr.rstd, dy, acc0, starts)         # the float64 statistics themselves
        scale = ref.rs * (ref.G.abs().max(1, keepdim=True).values * (1 + ref.X.abs().max(1, keepdim=True).values ** 2))
        assert ((x.grad - ref.U).abs() <= 1e-9 * scale).all(), (kind, eps, ((x.grad - ref.U).abs() / scale).max())
        assert ((starts[0].double() + g.grad - ref.dgamma).abs() <= 1e-9 * ref.dgamma_b / lx.U23).all()
        assert ((starts[1].double() + b.grad - ref.dbeta).abs() <= 1e-9 * ref.dbeta_b / lx.U23).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# an honest f32 evaluation uses at most half of every bound
# ----------------------------------------------------------------------------------------------------------------------------------
def f32_forward(x, gamma, beta, eps):
    """the forward in torch f32 with the kernel's summation order: per lane NV chunk sums (x + y) + (z + w) added in turn, the xor tree
    over the 64 lanes, a division by D; torch rounds every operation on its own (no fma)"""
    M, D = x.shape
    nv = (D + 255) // 256
    xp = torch.zeros(M, nv * 256, dtype=F32)
    xp[:, :D] = x.float()
    v = xp.view(M, nv, 64, 4)
    valid = (torch.arange(nv * 256) < D).view(nv, 64, 4)[..., 0].float()
    lanes = torch.arange(64)

    def wave(ch):
        s = torch.zeros(M, 64, dtype=F32)
        for i in range(nv):
            s = s + ch[:, i]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, 0]

    mu = wave((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) / torch.tensor(float(D), dtype=F32)
    a = v - mu[:, None, None, None]
    q = a * a
    var = wave(((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) * valid) / torch.tensor(float(D), dtype=F32)
    rs = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    y = (x.float() - mu[:, None]) * rs[:, None] * gamma + beta
    return mu, rs, y


def _share(worst, what, fams, got, want, bound, label, limit=0.5):
    got = got.double()
    assert torch.isfinite(got).all(), (what, label)
    q = (got - want).abs() / bound
    q = torch.where(got == want, torch.zeros_like(q), q)
    assert (q <= limit).all(), (what, label, q.max().item())
    if fams is None:
        worst[(what, 'all')] = max(worst.get((what, 'all'), 0.0), q.max().item())
    else:
        rowq = q.reshape(q.shape[0], -1).max(1).values
        for f in fams.unique().tolist():
            worst[(what, lx.FAMILIES[f])] = max(worst.get((what, lx.FAMILIES[f]), 0.0), rowq[fams == f].max().item())


def _table(worst, title):
    print(f'\n{title:28s}' + ''.join(f'{f:>9s}' for f in lx.FAMILIES + ('all',)))
    for what in dict.fromkeys(k for k, _ in worst):
        cells = [worst.get((what, f)) for f in lx.FAMILIES + ('all',)]
        print(f'{what:28s}' + ''.join('        -' if c is None else f'{c:9.4f}' for c in cells))


def test_honest_f32_forward_uses_at_most_half_of_every_bound():
    """rows are independent in the forward, so the master's 64 rows are every row of every case the GPU file runs"""
    worst = {}
    for D, f16, kind, eps in itertools.product(lx.D_LIST, (False, True), KINDS + ('huge',), lx.EPS_LIST):
        fr = lx.fwd_ref(D, f16, kind, eps)
        mu, rs, y = f32_forward(fr.x, fr.gamma, fr.beta, fr.eps)
        fams, label = lx.fam_ids(range(lx.NROWS), f16), (D, f16, kind, eps)
        _share(worst, 'mu', fams, mu, fr.mu, fr.mu_b, label)
        _share(worst, 'rstd', fams, rs, fr.rstd, fr.rstd_b, label)
        _share(worst, 'y', fams, y, fr.y, fr.y_b, label)
        for r in range(lx.NROWS):                               # the exact rows are exact in honest f32 too
            if lx.variant(r, f16) == 'const_int':
                assert mu[r].item() == fr.x[r, 0].item() and torch.equal(y[r], fr.beta) and abs(rs[r].item() * fr.eps ** 0.5 - 1) <= 4 * lx.U24
    _table(worst, 'honest f32 / bound, forward')


def f32_backward(x, gamma, mu, rs, dy, acc0, starts):
    """the backward in plain torch f32"""
    D = x.shape[1]
    d, mu, rs = dy.float(), mu[:, None], rs[:, None]
    xh, g = (x - mu) * rs, d * gamma
    c1, c2 = g.sum(1, keepdim=True) / D, (g * xh).sum(1, keepdim=True) / D
    acc = acc0 + rs * (g - c1 - xh * c2)
    return acc, starts[0] + (d * xh).sum(0), starts[1] + d.sum(0), starts[2] + acc.sum(0)


@pytest.mark.parametrize('D', lx.D_LIST)
def test_honest_f32_backward_uses_at_most_half_of_every_bound(D):
    """One exception, and it is analytic: dgamma at M = 1.  The sum-bound rule allows n 2^-23 = 4 U24 of |start| + |dy xhat| there, and a
    correct f32 kernel spends exactly four roundings on that element (two in xhat, the product, the add to the start), so an honest
    evaluation can use the whole bound and not half of it (0.66 of it is reached on these inputs, 0.46 at M = 2); the rule is kept as it is
    and dgamma at M = 1 is held to the bound itself."""
    worst = {}
    for bf16, kind, (M, r0) in itertools.product((False, True), KINDS, lx.SLICES):
        fr = lx.fwd_ref(D, False, kind, 1e-5)
        dy, acc0, starts = lx.grads(D, bf16)
        s = slice(r0, r0 + M)
        mu, rs = fr.mu[s].float(), fr.rstd[s].float()
        ref = lx.BwdRef(fr.x[s], fr.gamma, mu, rs, dy[s], acc0[s], starts)
        acc, dg, db, cs = f32_backward(fr.x[s], fr.gamma, mu, rs, dy[s], acc0[s], starts)
        fams, label = lx.fam_ids(range(r0, r0 + M), False), (D, bf16, kind, M, r0)
        _share(worst, 'dx', fams, acc.double() - acc0[s].double(), ref.U, ref.U_b, label)
        _share(worst, 'dgamma' + (' at M = 1' if M == 1 else ''), None, dg, ref.dgamma, ref.dgamma_b, label, 1.0 if M == 1 else 0.5)
        _share(worst, 'dbeta', None, db, ref.dbeta, ref.dbeta_b, label)
        _share(worst, 'colsum', None, cs, *ref.colsum_of(acc), label)
        # chained: honest f32 statistics, float64 autograd as the reference
        if not bf16 and (M, r0) in ((1, 0), (1, 3), (3, 9), (5, 0), (37, 27), (64, 0)):
            m32, r32, _ = f32_forward(fr.x[s], fr.gamma, fr.beta, fr.eps)
            acc, dg, _, _ = f32_backward(fr.x[s], fr.gamma, m32, r32, dy[s], acc0[s], starts)
            at = lx.BwdRef(fr.x[s], fr.gamma, m32, r32, dy[s], acc0[s], starts)
            exact = lx.BwdRef(fr.x[s], fr.gamma, fr.mu[s], fr.rstd[s], dy[s], acc0[s], starts)
            pu, pg = at.propagation(fr, torch.arange(r0, r0 + M))
            _share(worst, 'dx chained', fams, acc.double() - acc0[s].double(), exact.U, at.U_b + pu, label)
            _share(worst, 'dgamma chained' + (' at M = 1' if M == 1 else ''), None, dg, exact.dgamma, at.dgamma_b + pg, label, 1.0 if M == 1 else 0.5)
    _table(worst, f'honest f32 / bound, D={D}')


@pytest.mark.parametrize('M,D,dy_dtype', lx.BIG_CASES)
def test_honest_f32_backward_on_the_persistent_grid_cases(M, D, dy_dtype):
    fr = lx.fwd_ref(D, False, 'wide', 1e-5)
    rows = torch.arange(M) % lx.NROWS
    g = lx._gen(M + D)
    dy = (torch.randn(M, D, generator=g) * (0.25 + 3 * torch.rand(M, 1, generator=g))).to(dy_dtype)
    acc0 = torch.randn(M, D, generator=g)
    starts = lx.grads(D, False)[2]
    mu, rs = fr.mu.float()[rows], fr.rstd.float()[rows]
    ref = lx.BwdRef(fr.x[rows], fr.gamma, mu, rs, dy, acc0, starts)
    acc, dg, db, cs = f32_backward(fr.x[rows], fr.gamma, mu, rs, dy, acc0, starts)
    worst = {}
    _share(worst, 'dx', lx.fam_ids(rows, False), acc.double() - acc0.double(), ref.U, ref.U_b, (M, D))
    _share(worst, 'dgamma', None, dg, ref.dgamma, ref.dgamma_b, (M, D))
    _share(worst, 'dbeta', None, db, ref.dbeta, ref.dbeta_b, (M, D))
    _share(worst, 'colsum', None, cs, *ref.colsum_of(acc), (M, D))
    _table(worst, f'honest f32 / bound, M={M} D={D}')


# ----------------------------------------------------------------------------------------------------------------------------------
# the inputs are what the docstring says
# ----------------------------------------------------------------------------------------------------------------------------------
def test_inputs_hold_their_conditions():
    assert {M for M, _ in lx.SLICES} == set(lx.M_LIST) and all(r0 + M <= lx.NROWS for M, r0 in lx.SLICES)
    assert {lx.variant(r0, True) for M, r0 in lx.SLICES if M == 1} == set(lx.VARIANTS)
    assert {(D + 255) // 256 for D in lx.D_LIST} == {1, 2, 3, 4} and all(D % 4 == 0 for D in lx.D_LIST)
    assert any(D % 256 and D > 256 for D in lx.D_LIST) and lx.master(100, False) is lx.master(100, False)
    for D, f16 in itertools.product(lx.D_LIST, (False, True)):
        x = lx.master(D, f16)
        assert x.dtype == (torch.float16 if f16 else F32) and torch.isfinite(x).all()
        x = x.double()
        mu, sd = x.mean(1), x.var(1, unbiased=False).sqrt()
        for r in range(lx.NROWS):
            v = lx.variant(r, f16)
            if v.startswith('offset'):
                assert abs(abs(mu[r]) / float(v.split('_')[1]) - 1) < 0.05 and sd[r] > 0.2
            elif v.startswith('outlier'):
                c = lx.outlier_col(v, D)
                assert abs(x[r, c]) == 1000 and c // 4 == {'outlier_first': 0, 'outlier_mid': D // 8, 'outlier_last': D // 4 - 1}[v]
            elif v.startswith('tiny'):
                assert sd[r] ** 2 < (1e-6 if v == 'tiny_1e-4' else 1e-4)
            elif v == 'const_int':
                assert sd[r] == 0 and x[r, 0] == x[r, 0].round() and abs(x[r, 0]) * D < 2 ** 24
            elif v == 'const_tenth':
                assert (x[r] == x[r, 0]).all() and x[r, 0] != x[r, 0].round()
            elif v == 'big':
                assert sd[r] > 1e4 and (not f16 or (x[r].max() == 65504 and x[r].min() == -65504))
            elif v == 'sub':
                assert x[r].abs().max() < 2.0 ** -14 and x[r].abs().max() > 0 and (x[r] * 2.0 ** 24 == (x[r] * 2.0 ** 24).round()).all()
        gamma, beta = lx.affine(D, 'wide')
        assert (gamma == 0).any() and (gamma < 0).any() and (gamma > 7).any() and beta.abs().min() > 3
        for kind, eps in itertools.product(KINDS + ('huge',), lx.EPS_LIST):
            assert lx.fwd_ref(D, f16, kind, eps).T.max() < 1e-3                      # (1 - T)^-1/2 is far from its pole
        if f16 and D >= 100:                                                         # the fp16 output overflows to both infinities on big rows
            big = [r for r in range(lx.NROWS) if lx.variant(r, True) == 'big']
            y = lx.fwd_ref(D, True, 'huge', 1e-5).y[big]
            assert (y > 7e4).any() and (y < -7e4).any()


# ----------------------------------------------------------------------------------------------------------------------------------
# the bounds are tight enough: every wrong kernel leaves one
# ----------------------------------------------------------------------------------------------------------------------------------
def _bf16_trunc(y32):
    return (y32.view(torch.int32) & -65536).view(F32).bfloat16()


def _first_case_that_catches(wrong):
    """the first case of the GPU file, in its order, at which the wrong kernel leaves a bound or gives a non-finite value"""
    if wrong in lx.FWD_WRONGS:
        for D, f16, kind, eps, (M, r0) in itertools.product(lx.D_LIST, (False, True), KINDS, lx.EPS_LIST, lx.SLICES):
            fr = lx.fwd_ref(D, f16, kind, eps)
            rows = torch.arange(r0, r0 + M)
            if wrong == 'bf16_truncation':                      # the 16-bit output is compared bit for bit with RNE
                y32 = fr.y[rows].float()
                what = 'y bf16 bits' if not torch.equal(_bf16_trunc(y32).view(torch.int16), y32.bfloat16().view(torch.int16)) else None
            else:
                what = lx.fwd_leaves(fr, rows, *lx.fwd_eval(fr.x[rows], fr.gamma, fr.beta, fr.eps, wrong))
            if what:
                return f'{what} at D={D} {"f16" if f16 else "f32"} rows, {kind} gamma, eps={eps}, M={M}, r0={r0} ({lx.variant(r0, f16)})'
    else:
        for D, bf16, kind, (M, r0) in itertools.product(lx.D_LIST, (False, True), KINDS, lx.SLICES):
            what = lx.bwd_leaves(lx.bwd_case(D, bf16, kind, M, r0), lx.bwd_case(D, bf16, kind, M, r0, wrong))
            if what:
                return f'{what} at D={D} dy {"bf16" if bf16 else "f32"}, {kind} gamma, M={M}, r0={r0} ({lx.variant(r0, False)})'
    return None


@pytest.mark.parametrize('wrong', lx.WRONGS)
def test_every_wrong_kernel_leaves_a_bound(wrong):
    caught = _first_case_that_catches(wrong)
    assert caught, f'{wrong} stays inside every bound on every case: the inputs or the bounds are too weak'
    print(f'{wrong:24s} caught by {caught}')


def test_wrong_kernels_are_caught_on_every_family_of_rows_that_can_show_them():
    """beyond the one case the list asks for: the statistics mistakes leave a bound on the plain rows of the widest and the narrowest D as
    well (a per-element bound has no blind spot behind a hard row), and the right kernel leaves none"""
    for D in (4, 100, 1020):
        fr = lx.fwd_ref(D, False, 'usual', 1e-5)
        rows = torch.arange(0, 1)                               # one plain row
        assert lx.fwd_leaves(fr, rows, *lx.fwd_eval(fr.x[rows], fr.gamma, fr.beta, fr.eps)) is None
        for wrong in ('divisor_d_minus_1', 'eps_outside_sqrt') + (('padded_divisor', 'tail_chunk_lost') if D % 256 else ()):
            assert lx.fwd_leaves(fr, rows, *lx.fwd_eval(fr.x[rows], fr.gamma, fr.beta, fr.eps, wrong)), (D, wrong)
        assert lx.bwd_leaves(lx.bwd_case(D, False, 'usual', 5, 0), lx.bwd_case(D, False, 'usual', 5, 0)) is None
    # a mistake that changes nothing at a case is reported as hidden there: the neighbour's statistics at M = 1, the idle waves at M = 64
    fr = lx.fwd_ref(100, False, 'usual', 1e-5)
    assert lx.fwd_leaves(fr, torch.arange(3, 4), *lx.fwd_eval(fr.x[3:4], fr.gamma, fr.beta, fr.eps, 'neighbour_stats')) is None
    assert lx.bwd_leaves(lx.bwd_case(100, False, 'usual', 64, 0), lx.bwd_case(100, False, 'usual', 64, 0, 'idle_wave_stale')) is None


# ----------------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks run on the host, before any launch (no GPU here)
# ----------------------------------------------------------------------------------------------------------------------------------
P = 4096                                                       # never dereferenced: the host refuses first


def _fwd(f16=False, x=P, ldx=64, gamma=P, beta=P, y=P, ldy=64, out=0, M=8, D=64):
    from distillclip_amd._lib import lib
    fn = lib().dclip_layernorm_fwd_f16 if f16 else lib().dclip_layernorm_fwd
    return fn(x, ldx, None, gamma, beta, y, ldy, out, None, None, M, D, 1e-5, None)


def _bwd(dy=P, lddy=64, dy_f32=0, x=P, ldx=64, gamma=P, mean=P, rstd=P, dx_acc=P, lddx=64, dx_bf16=P, lddb=64, M=8, D=64):
    from distillclip_amd._lib import lib
    return lib().dclip_layernorm_bwd(dy, lddy, dy_f32, x, ldx, None, gamma, mean, rstd, dx_acc, lddx, dx_bf16, lddb, None, None, None, M, D, None)


@pytest.mark.parametrize('kw,match', [
    (dict(D=66, ldx=68, ldy=68), 'D % 4'), (dict(D=0), '0 < D'), (dict(D=1028, ldx=1028, ldy=1028), 'D <= 1024'), (dict(M=0), 'M > 0'),
    (dict(ldx=66), 'multiples of 4'), (dict(ldy=70), 'multiples of 4'),
    (dict(x=P + 4), 'x must be 16-byte'), (dict(f16=True, x=P + 4), 'x must be 8-byte'), (dict(f16=True, x=P + 2), 'x must be 8-byte'),
    (dict(y=P + 4), 'y must be 8-byte'), (dict(y=P + 8, out=1), 'y must be 16-byte'), (dict(f16=True, y=P + 4, out=2), 'y must be 8-byte'),
    (dict(gamma=P + 4), 'gamma and beta'), (dict(beta=P + 8), 'gamma and beta'),
    (dict(out=2), 'output dtype'), (dict(out=3, f16=True), 'output dtype'), (dict(out=-1), 'output dtype'),
    (dict(x=None), 'null operand'), (dict(gamma=None), 'null operand'), (dict(beta=None), 'null operand'), (dict(y=None), 'null operand'),
])
def test_forward_host_refuses_before_any_launch(kw, match):
    """every other argument of `_fwd` is valid and the message names the defect: the refusal is this defect's and not another's"""
    with pytest.raises(ValueError, match=match):
        _fwd(**kw)


@pytest.mark.parametrize('kw,match', [
    (dict(D=66), 'D % 4'), (dict(D=0), '0 < D'), (dict(D=1028, lddy=1028, ldx=1028, lddx=1028, lddb=1028), 'D <= 1024'), (dict(M=0), 'M > 0'),
    (dict(lddy=66), 'multiples of 4'), (dict(ldx=70), 'multiples of 4'), (dict(lddx=65), 'multiples of 4'), (dict(lddb=66), 'multiples of 4'),
    (dict(dy=P + 4), 'dy must be 8-byte'), (dict(dy=P + 8, dy_f32=1), 'dy must be 16-byte'),
    (dict(x=P + 8), 'x, dx_acc and gamma'), (dict(dx_acc=P + 4), 'x, dx_acc and gamma'), (dict(gamma=P + 12), 'x, dx_acc and gamma'),
    (dict(dx_bf16=P + 4), 'dx_bf16 must be 8-byte'),
    (dict(dy=None), 'null operand'), (dict(x=None), 'null operand'), (dict(gamma=None), 'null operand'), (dict(mean=None), 'null operand'),
    (dict(rstd=None), 'null operand'), (dict(dx_acc=None), 'null operand'),
])
def test_backward_host_refuses_before_any_launch(kw, match):
    with pytest.raises(ValueError, match=match):
        _bwd(**kw)
