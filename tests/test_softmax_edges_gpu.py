"""Every hand-written softmax at sharp logits: the loss's temperature softmaxes at small tau, and the five attention score stages under
large per-(batch, head, query-row) score offsets, against float64 references built from the same rounded operands the kernels receive.

A softmax is invariant to a constant added to each of its rows, so the attention references do not move with the offsets: matching
them at every magnitude is the shift-invariance check.  A kernel that keeps a fixed or shared maximum instead of the row's own fails
here with zeros or NaN once two maxima sit more than ~87 apart (f32 exp underflows below -87.3 / -103.3).

Error model used by the tolerances (eps = 2^-24, the f32 unit roundoff; u = 2^-8, the bf16 unit roundoff: 7 stored mantissa bits):
  * a bf16 store of x costs at most u |x|; a bf16 or f16 operand the reference does not round itself costs u (2^-11 for f16) of
    its magnitude in every product it enters, so those terms are bounded through products of absolute values;
  * an f32 logit x carries an absolute error of a few eps |x|, which becomes the relative error of exp(x - m);
  * where a kernel rounds an intermediate by design (split-bf16 scores, bf16 e in the row sums, f16 mix operands), the reference
    applies exactly that rounding, and only the f32 arithmetic around it is left to the bound.
"""
import math

import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
U_BF16 = 2.0 ** -8
U_F16 = 2.0 ** -11

# ----------------------------------------------------------------------------------------------------------------------------------
# A1 / A2: the fused distillation loss at small temperatures
# ----------------------------------------------------------------------------------------------------------------------------------
NAMES = ['out_l1', 'out_cos', 'out_kl', 'out_ce', 'cos_diff', 'hard_label', 'soft_label', 'logits_mse']
TOWER = ['out_l1', 'out_cos', 'out_kl', 'out_ce']
SLOT_IMG = {'out_l1': 1, 'out_cos': 2, 'out_kl': 3, 'out_ce': 4}
SLOT_X = {'cos_diff': 9, 'hard_label': 10, 'soft_label': 11, 'logits_mse': 12}
SCALE = {'cos_diff': 0.1, 'hard_label': 2.0}
TAUS = [0.07, 0.02, 0.01, 0.005]


def _features(kind, B, E, seed):
    """si / st: student image / text, ti / tt: teacher image / text, f32 [B, E].
    random   independent N(0, 1) rows: every cosine logit is O(1 / sqrt(E)), row maxima ~0.1 (at tau = 0.01 a fixed maximum of 1 / tau
             leaves exp((0.1 - 1) / tau) = e^-90: denormal row sums)
    negative image rows around +u, text rows around -u: every cosine in [-1, -0.6], so every row's largest logit is <= -0.6
    neardup  text = image + small noise, teacher = student + small noise: diagonal cosines -> 1 (the regime a fixed maximum covered)
    sharp    the random set with every feature x30: the tower terms' feature-axis softmax (out_kl / out_ce) is sharp as well"""
    g = torch.Generator().manual_seed(seed)
    n = lambda: torch.randn(B, E, generator=g, dtype=torch.float64)
    if kind in ('random', 'sharp'):
        e = {k: n() for k in ('si', 'st', 'ti', 'tt')}
        if kind == 'sharp':
            e = {k: 30 * v for k, v in e.items()}
    elif kind == 'negative':
        u = torch.randn(E, generator=g, dtype=torch.float64)
        u = u / u.norm()
        sig = 0.25 / math.sqrt(E)                           # |noise| ~ 0.25: cosines -1 + O(0.1), well inside [-1, -0.6]
        e = {'si': u + sig * n(), 'ti': u + sig * n(), 'st': -u + sig * n(), 'tt': -u + sig * n()}
        e = {k: v * (1 + torch.rand(B, 1, generator=g, dtype=torch.float64)) for k, v in e.items()}   # norms vary
    elif kind == 'neardup':
        base = n()
        e = {'si': base + 0.05 * n(), 'st': base + 0.05 * n(), 'ti': base + 0.05 * n(), 'tt': base + 0.05 * n()}
    else:
        raise ValueError(kind)
    return {k: v.float() for k, v in e.items()}


def _oracle64(e, names, tau, two=True):
    """float64 LossOracle / clip_forward on the f32 inputs the kernel receives -> (loss, res, d si, d st)"""
    si = e['si'].double().requires_grad_(True)
    st = e['st'].double().requires_grad_(True)
    lc = oracle.LossOracle(names, SCALE, temperature=tau)
    if two:
        stu = oracle.clip_forward({'last_representation': si}, {'last_representation': st})
        tea = oracle.clip_forward({'last_representation': e['ti'].double()}, {'last_representation': e['tt'].double()})
        loss, res = lc(stu, tea, 'all')
    else:
        loss, res = lc({'last_representation': si}, {'last_representation': e['ti'].double()}, 'image')
    loss.backward()
    return lc, loss.detach(), {k: v.detach() for k, v in res.items()}, si.grad, st.grad


def _loss_tol(e, tau):
    """Relative tolerance of every loss scalar and gradient (max-norm).  Each softmax input x = logit / tau is formed in f32: a cosine
    logit comes out of an E-term dot product of normalised rows with an error of ~4 sqrt(E) eps (normalisation, products, random-walk
    accumulation), a feature-axis logit (out_kl / out_ce) carries ~2 eps |feature| (the max subtraction); dividing by tau and the f32
    product x * (1 / tau) scale that into the exponent.  Both enter exp(x - lse) twice (numerator and log-sum-exp), and the
    __expf / __logf hardware approximations add a few eps of their own.  The floors (3e-5 scalars, 2e-4 gradients) are the
    mild-temperature suite's bounds (tests/test_loss_gpu.py), where the rest of the arithmetic dominates."""
    E = e['si'].shape[1]
    feat = max(v.abs().max().item() for v in e.values())
    x_err = (4 * math.sqrt(E) + 2) * EPS / tau + 2 * EPS * feat / tau + 8 * EPS
    return 3e-5 + 4 * x_err, 2e-4 + 4 * x_err


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-30)


def _check_scalars(out, loss, res, lc, names, tol, two=True):
    out = out.double().cpu()
    assert torch.isfinite(out).all(), out
    assert abs(out[0].item() - loss.item()) <= tol * max(1.0, abs(loss.item())), ('total', out[0].item(), loss.item())
    for n in names:
        if n in SLOT_X:
            got, ref = out[SLOT_X[n]].item() * lc.loss_scale[n], res[n].item()
            assert abs(got - ref) <= tol * max(1.0, abs(ref)), (n, got, ref)
        else:
            for tow, off in ((('image_', 0), ('text_', 4)) if two else (('', 0),)):      # one tower: unprefixed names
                got, ref = out[SLOT_IMG[n] + off].item() * lc.loss_scale[n], res[tow + n].item()
                assert abs(got - ref) <= tol * max(1.0, abs(ref)), (tow + n, got, ref)


def _weights(lc):
    return {n: lc.loss_scale[n] * lc.percent[n] for n in lc.loss_name}


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('kind', ['random', 'negative', 'neardup', 'sharp'])
@pytest.mark.parametrize('B', [37, 512])
def test_loss_two_towers_at_small_temperature(B, kind, tau):
    """every term on, E = 512: total, each raw scalar slot and both gradients against the float64 oracle (tolerance: _loss_tol)"""
    from distillclip_amd import ops
    e = _features(kind, B, 512, 1000 * B + len(kind))
    lc, loss, res, gi, gt = _oracle64(e, NAMES, tau)
    assert torch.isfinite(loss) and torch.isfinite(gi).all() and torch.isfinite(gt).all()      # the inputs stay inside the oracle's range
    g = {k: v.cuda() for k, v in e.items()}
    out, di, dt = ops.distill_loss(g['si'], g['ti'], g['st'], g['tt'], weights=_weights(lc), temperature=tau)
    tol_s, tol_g = _loss_tol(e, tau)
    _check_scalars(out, loss, res, lc, NAMES, tol_s)
    assert torch.isfinite(di).all() and torch.isfinite(dt).all()
    assert _rel(di.cpu(), gi) < tol_g, ('d s_img', _rel(di.cpu(), gi), tol_g)
    assert _rel(dt.cpu(), gt) < tol_g, ('d s_txt', _rel(dt.cpu(), gt), tol_g)


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('kind', ['random', 'sharp'])
def test_loss_one_tower_at_small_temperature(kind, tau):
    """single tower, B = 100: out_kl / out_ce are softmaxes over the feature axis (x30 features: logits up to ~4e4 at tau = 0.005)"""
    from distillclip_amd import ops
    e = _features(kind, 100, 512, 77 + len(kind))
    lc, loss, res, gi, _ = _oracle64(e, TOWER, tau, two=False)
    assert torch.isfinite(loss) and torch.isfinite(gi).all()
    out, di, _ = ops.distill_loss(e['si'].cuda(), e['ti'].cuda(), weights=_weights(lc), temperature=tau)
    tol_s, tol_g = _loss_tol(e, tau)
    _check_scalars(out, loss, res, lc, TOWER, tol_s, two=False)
    assert torch.isfinite(di).all()
    assert _rel(di.cpu(), gi) < tol_g, (_rel(di.cpu(), gi), tol_g)


@pytest.mark.parametrize('kind', ['random', 'negative'])
@pytest.mark.parametrize('B,world', [(48, 3), (4096, 8)])
def test_loss_row_blocks_at_small_temperature(B, world, kind):
    """data-parallel row blocks at tau = 0.01 with every cross term on: statistics pass per block -> gather -> gradient pass per block.
    The block shares add up to the whole-batch call and the gradient rows equal its rows (same tolerance: only the order in which the
    column slices' statistics are merged differs), and both match the float64 oracle on the concatenated batch."""
    from distillclip_amd import ops
    tau = 0.01
    e = _features(kind, B, 512, 3 * B + world + len(kind))
    lc, loss, res, ogi, ogt = _oracle64(e, NAMES, tau)
    w = _weights(lc)
    g = {k: v.cuda() for k, v in e.items()}
    tol_s, tol_g = _loss_tol(e, tau)
    full, di, dt = ops.distill_loss(g['si'], g['ti'], g['st'], g['tt'], weights=w, temperature=tau)
    per = B // world
    blocks = [ops.distill_loss(g['si'], g['ti'], g['st'], g['tt'], weights=w, temperature=tau, row0=r * per, rows=per, stats_only=True)
              for r in range(world)]
    gstats = torch.stack(blocks).permute(1, 0, 2).reshape(6, B).contiguous()          # what the all-gather builds
    assert torch.isfinite(gstats).all()
    tot = torch.zeros(16, dtype=torch.float64)
    for r in range(world):
        sc, gi, gt = ops.distill_loss(g['si'], g['ti'], g['st'], g['tt'], weights=w, temperature=tau, row0=r * per, rows=per,
                                      gathered_stats=gstats)
        tot += sc.double().cpu()
        assert _rel(gi, di[r * per:(r + 1) * per]) < tol_g and _rel(gt, dt[r * per:(r + 1) * per]) < tol_g, r
    fullc = full.double().cpu()
    assert ((tot - fullc).abs() <= tol_s * fullc.abs().clamp(min=1.0)).all(), (tot, fullc)
    _check_scalars(tot, loss, res, lc, NAMES, tol_s)
    _check_scalars(full, loss, res, lc, NAMES, tol_s)
    assert _rel(di.cpu(), ogi) < tol_g and _rel(dt.cpu(), ogt) < tol_g, (_rel(di.cpu(), ogi), _rel(dt.cpu(), ogt), tol_g)


# ----------------------------------------------------------------------------------------------------------------------------------
# A3: attention score stages under per-(batch, head, query-row) offsets
# ----------------------------------------------------------------------------------------------------------------------------------
MAGS = [0, 30, 100, 300]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offsets(B, H, N, mag, seed):
    """c[b, h, i] = sign_h * mag * (1 + 0.25 xi): heads alternate in sign, so two heads' maxima sit >= 2 mag apart"""
    xi = torch.rand(B, H, N, 1, generator=_gen(seed), dtype=torch.float64)
    sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(H)], dtype=torch.float64).view(1, H, 1, 1)
    return sign * mag * (1 + 0.25 * xi)


def _bf(x):
    return x.to(torch.bfloat16).double()


def _split(x):
    """split-bf16 operand pair of the MFMA head mix: hi = bf16(x), lo = bf16(x - hi)"""
    hi = x.float().to(torch.bfloat16).float()
    lo = (x.float() - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def _mask(N, causal):
    return torch.ones(N, N, dtype=torch.bool).tril_() if causal else torch.ones(N, N, dtype=torch.bool)


def _softmax64(a, keep):
    a = a.masked_fill(~keep, float('-inf'))
    return torch.softmax(a, -1)


def _within(got, ref, tol, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert torch.isfinite(got).all(), (what, 'non-finite values', (~torch.isfinite(got)).sum().item())
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (what, bad.sum().item(), err.max().item(), (err / tol.clamp(min=1e-300)).max().item())


def _wmat(H, seed, amp):
    return torch.eye(H, dtype=torch.float64) + amp * torch.randn(H, H, generator=_gen(seed), dtype=torch.float64)


def _mix_kind(H, mix, causal):
    if not mix:
        return 'plain'
    return 'mfma' if (H > 12 and not causal) else 'valu'     # dclip_attn_softmax_fwd's dispatch


@pytest.mark.parametrize('mag', MAGS)
@pytest.mark.parametrize('B,N,H,mix,causal', [(2, 77, 8, False, False), (2, 77, 8, False, True), (2, 50, 16, False, False),
                                              (2, 101, 16, False, True), (2, 77, 12, True, False), (2, 101, 12, True, True),
                                              (2, 50, 24, True, False), (2, 101, 24, True, False), (2, 50, 24, True, True)])
def test_attention_softmax_stage_under_offsets(B, N, H, mix, causal, mag):
    """dclip_attn_softmax_fwd / _bwd fed S directly: plain kernel (no mix, H = 8 / 16), VALU mix (H = 12, and H = 24 causal), MFMA mix
    (H = 24 non-causal, N = 50: one 64-key slot, N = 101: two).  S = randn * 1.5 + c[b, h, i], |c| up to 375.

    Forward reference: A = S (plain), W_l S in float64 (VALU: f32 FMAs, bound H eps sum|W_l| |S| on A), or the MFMA mix's own split
    product W_l,hi S_hi + W_l,hi S_lo + W_l,lo S_hi; P = softmax(A).  The MFMA kernel sums bf16 copies of e = exp(A - m): the reference
    does the same.  P and R are stored as bf16: |err| <= (u + 2 dA) * (|P|, resp. |W_w| |P|) + eps, dA the exponent error bound.

    Backward, from the kernel's own bf16 P and a bf16 dR: dP = W_w^T dR, dA = P (dP - sum_j P dP), dS = W_l^T dA in float64.  The mix
    backward rounds W_w, W_l, dA to bf16 operands and stores dS as bf16: |err| <= 2 u (2 |W_l|^T |dA| + |W_l|^T (|P| |W_w|^T |dR|)) +
    u |dS| (the factor 2 covers second-order products and the f32 accumulations).  dW_w = sum dR P^T has exact bf16 products:
    f32 accumulation over the n = B N^2 positions, n eps sum |dR| |P|.  dW_l = sum dA S^T multiplies bf16 dA (itself off by u |P| |dP|)
    by bf16 S: 2 u sum (|dA| + |P| |W_w|^T |dR|) |S|, which grows with |S| while dW_l itself does not (sum_j dA = 0 cancels the
    offsets)."""
    from distillclip_amd import ops
    kind = _mix_kind(H, mix, causal)
    seed = 7 * N + H + (1 if causal else 0)
    Np = (N + 7) // 8 * 8
    s64 = 1.5 * torch.randn(B, H, N, N, generator=_gen(seed), dtype=torch.float64) + _offsets(B, H, N, mag, seed + 1)
    s = torch.zeros(B, H, N, Np)
    s[..., :N] = s64.float()
    s64 = s[..., :N].double()                                    # the f32 scores the kernel reads
    wl = _wmat(H, seed + 2, 0.2).float() if mix else None
    ww = _wmat(H, seed + 3, 0.2).float() if mix else None
    keep = _mask(N, causal)
    babs = lambda w, x: torch.einsum('gh,bhij->bgij', w.double().abs(), x.abs())
    if kind == 'plain':
        a = s64
        da = 4 * EPS * s64.abs().amax(-1, keepdim=True) + 2 ** -16
    elif kind == 'valu':
        a = torch.einsum('gh,bhij->bgij', wl.double(), s64)
        da = H * EPS * babs(wl, s64).amax(-1, keepdim=True) + 2 ** -16
    else:
        (lh, ll), (sh, sl) = _split(wl.double()), _split(s64)
        mm = lambda w, x: torch.einsum('gh,bhij->bgij', w, x)
        a = mm(lh, sh) + mm(lh, sl) + mm(ll, sh)
        da = 3 * H * EPS * babs(wl, s64).amax(-1, keepdim=True) + 2 ** -12     # + bf16 copies of e that round the other way
    if kind == 'mfma':
        am = a.masked_fill(~keep, float('-inf'))
        ee = torch.exp(am - am.amax(-1, keepdim=True))
        pref = ee / _bf(ee).sum(-1, keepdim=True)
    else:
        pref = _softmax64(a, keep)
    rref = torch.einsum('gh,bhij->bgij', ww.double(), pref) if mix else pref
    p, r = ops.attn_softmax_fwd(s.cuda(), wl.cuda() if mix else None, ww.cuda() if mix else None, causal=causal, save_p=True)
    _within(p[..., :N], pref, (U_BF16 + 2 * da) * pref + EPS, f'P ({kind}, |c| ~ {mag})')
    _within(r[..., :N], rref, (U_BF16 + 2 * da) * (babs(ww, pref) if mix else pref) + EPS, f'R ({kind}, |c| ~ {mag})')
    assert torch.count_nonzero(p[..., N:]) == 0 and torch.count_nonzero(r[..., N:]) == 0

    dr = torch.zeros(B, H, N, Np, dtype=torch.bfloat16)
    dr[..., :N] = torch.randn(B, H, N, N, generator=_gen(seed + 4)).to(torch.bfloat16)
    dwl = torch.zeros(H, H, device='cuda') if mix else None
    dww = torch.zeros(H, H, device='cuda') if mix else None
    ds = ops.attn_softmax_bwd(dr.cuda(), p, s.cuda(), wl.cuda() if mix else None, ww.cuda() if mix else None, dwl, dww)
    pk, d64 = p[..., :N].double().cpu(), dr[..., :N].double()
    if mix:
        dp = torch.einsum('gh,bgij->bhij', ww.double(), d64)
        dp_abs = torch.einsum('gh,bgij->bhij', ww.double().abs(), d64.abs())
    else:
        dp, dp_abs = d64, d64.abs()
    da_ref = pk * (dp - (pk * dp).sum(-1, keepdim=True))
    if mix:
        ds_ref = torch.einsum('gh,bgij->bhij', wl.double(), da_ref)
        t1 = torch.einsum('gh,bgij->bhij', wl.double().abs(), da_ref.abs())
        t2 = torch.einsum('gh,bgij->bhij', wl.double().abs(), pk * dp_abs)
        tol = 2 * U_BF16 * (2 * t1 + t2) + U_BF16 * ds_ref.abs() + EPS
    else:
        ds_ref = da_ref
        tol = 2 * U_BF16 * pk * (dp_abs + (pk * dp_abs).sum(-1, keepdim=True)) + U_BF16 * ds_ref.abs() + EPS
    _within(ds[..., :N], ds_ref, tol, f'dS ({kind}, |c| ~ {mag})')
    assert torch.count_nonzero(ds[..., N:]) == 0
    if mix:
        n = B * N * N
        dww_ref = torch.einsum('bgij,bhij->gh', d64, pk)
        dww_tol = n * EPS * torch.einsum('bgij,bhij->gh', d64.abs(), pk.abs()) + EPS
        _within(dww, dww_ref, dww_tol, f'dW_w ({kind}, |c| ~ {mag})')
        dwl_ref = torch.einsum('bgij,bhij->gh', da_ref, s64)
        dwl_tol = 2 * U_BF16 * torch.einsum('bgij,bhij->gh', da_ref.abs() + pk * dp_abs, s64.abs()) + EPS
        _within(dwl, dwl_ref, dwl_tol, f'dW_l ({kind}, |c| ~ {mag})')
        print(f'dW_l error growth: {kind} H={H} N={N} |c|~{mag}: max |err| {(dwl.double().cpu() - dwl_ref).abs().max().item():.3e}, '
              f'max |dW_l| {dwl_ref.abs().max().item():.3e}, bound {dwl_tol.max().item():.3e}')


def _quant(shape, seed, step):
    """values in {-2 step .. 2 step}: products of two such operands are multiples of step^2 and exact in every format used below"""
    return step * torch.randint(-2, 3, shape, generator=_gen(seed)).double()


def _qkv_with_offsets(B, N, H, hd, mag, seed, quantised):
    """q, k, v (float64 copies of the bf16 operands) and the bf16 [B*N, 3D] buffer.  The offset rides on feature 0 of every head:
    q[i, 0] = a_i in [1, 1.5], k[j, 0] = u_{b,h} for every key j, so row i of head h gains scale * a_i * u_{b,h}, a per-row
    constant of magnitude mag .. 1.5 mag and alternating sign over the heads."""
    D, scale = H * hd, hd ** -0.5
    if quantised:
        q, k, v = (_quant((B, H, N, hd), seed + t, 0.5) for t in range(3))
        a = 1 + 0.5 * torch.randint(0, 2, (B, H, N), generator=_gen(seed + 3)).double()
        u = torch.round(_offsets(B, H, 1, mag, seed + 4)[..., 0, 0] / scale * 2) / 2       # multiples of 1/2: q k products exact
    else:
        q, k, v = (torch.randn(B, H, N, hd, generator=_gen(seed + t), dtype=torch.float64) for t in range(3))
        a = 1 + 0.5 * torch.rand(B, H, N, generator=_gen(seed + 3), dtype=torch.float64)
        u = _offsets(B, H, 1, mag, seed + 4)[..., 0, 0] / scale
    q[..., 0], k[..., 0] = a, u[..., None].expand(B, H, N)
    q, k, v = _bf(q), _bf(k), _bf(v)
    tok = lambda x: x.permute(0, 2, 1, 3).reshape(B * N, D)
    qkv = torch.cat([tok(q), tok(k), tok(v)], 1).to(torch.bfloat16)
    return q, k, v, qkv


@pytest.mark.parametrize('mag', MAGS)
@pytest.mark.parametrize('N', [1, 77, 128])
@pytest.mark.parametrize('hd,causal', [(32, False), (64, False), (32, True), (64, True)])
def test_fused_attention_forward_under_offsets(hd, causal, N, mag):
    """dclip_attn_fused_fwd (the frozen teacher), H = 4: ctx = P V with P = e / sum e, e = exp(S - m) stored as bf16 for the PV product
    (the reference rounds e the same way and divides by the f32-exact sum).  The raw scores are exact f32 sums of exact bf16 products
    up to a few eps |S|; scale * log2(e) and the max enter one f32 FMA: exponent error dx = 8 eps |S|max + 2^-22.  Bound:
    |err| <= u |ctx| + (u + 2 dx) |e| |V| / sum e + eps (u for a bf16 copy of e rounding the other way, u for the bf16 store)."""
    from distillclip_amd import ops
    B, H = 2, 4
    q, k, v, qkv = _qkv_with_offsets(B, N, H, hd, mag, 100 * hd + N + int(causal), quantised=False)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    keep = _mask(N, causal)
    sm = s.masked_fill(~keep, float('-inf'))
    e = torch.exp(sm - sm.amax(-1, keepdim=True))
    den = e.sum(-1, keepdim=True)
    ctx = (_bf(e) @ v) / den
    dx = 8 * EPS * s.abs().max().item() * 1.4427 + 2 ** -22
    tol = U_BF16 * ctx.abs() + (U_BF16 + 2 * dx) * (e @ v.abs()) / den + EPS
    got = ops.attn_fused_fwd(qkv.cuda(), B, N, H, hd, causal).double().cpu().view(B, N, H, hd).permute(0, 2, 1, 3)
    _within(got, ctx, tol, f'fused ctx (hd={hd}, causal={causal}, N={N}, |c| ~ {mag})')


@pytest.mark.parametrize('mag', [0, 30])
@pytest.mark.parametrize('B,N,H,hd', [(2, 50, 24, 32), (2, 77, 12, 64), (2, 77, 8, 32)])
def test_register_resident_mix_under_offsets(B, N, H, hd, mag):
    """dclip_attn_mix_fwd / _bwd (attention_mix.hip) with the offsets on a common key component.  The forward mixes run on f16
    operands: the raw scores q k^T and log2(e) * scale * W_l enter as f16, P as f16 for the W_w mix.  q, k are drawn from multiples of
    1/2 (offset feature included), so every raw score is a multiple of 1/4 below 512 in magnitude and exact in f16: the reference then
    models the f16 path exactly (f16 W_l, f16 W_w; the f16 copy of P costs 2^-11 of |W_w| |P|), and the f16 range is what limits the
    tested offset to |c| ~ 30..45.  Log-sum-exp rows (natural log): f32 MFMA accumulation, H eps sum |W_l| |S| absolute.
    Backward against float64 autograd of the exact graph, same bounds as the softmax stage's mix backward, the operands being bf16
    there; dW_l grows with |S| as there."""
    from distillclip_amd import ops
    D, scale = H * hd, hd ** -0.5
    q, k, v, qkv = _qkv_with_offsets(B, N, H, hd, mag, 31 * N + H + hd, quantised=True)
    raw = q @ k.transpose(-1, -2)
    assert torch.equal(raw, raw.half().double())                                           # exact f16 operands
    wl, ww = _wmat(H, 5 + H, 0.15).float(), _wmat(H, 6 + H, 0.15).float()
    sc = torch.tensor(1.4426950408889634 * scale, dtype=torch.float32)
    wl16 = (wl * sc).half().double()                                  # log2(e) * scale * W_l as the kernel packs it
    ww16 = ww.half().double()
    a2 = torch.einsum('gh,bhij->bgij', wl16, raw)                     # log2-domain mixed scores
    lse2 = torch.logsumexp(a2 * math.log(2), -1) / math.log(2)
    p = torch.exp2(a2 - lse2[..., None])
    r = torch.einsum('gh,bhij->bgij', ww16, p)
    da = H * EPS * torch.einsum('gh,bhij->bgij', wl16.abs(), raw.abs()).amax(-1, keepdim=True) + 2 ** -20
    rb, lse = ops.attn_mix_fwd(qkv.cuda(), B, N, H, hd, wl.cuda(), ww.cuda(), scale)
    R = ops.unblock_scores(rb)
    tol_r = (U_BF16 + U_F16 + 2 * da) * torch.einsum('gh,bhij->bgij', ww16.abs(), p) + EPS
    _within(R[..., :N], r, tol_r, f'R (register mix, |c| ~ {mag})')
    assert torch.count_nonzero(R[..., N:]) == 0
    _within(lse, lse2 * math.log(2), da[..., 0] + 4 * EPS * (lse2.abs() + 1), f'log-sum-exp (register mix, |c| ~ {mag})')

    d_ctx = _bf(torch.randn(B * N, D, generator=_gen(H + N), dtype=torch.float64))
    do = d_ctx.view(B, N, H, hd).permute(0, 2, 1, 3)
    dr = do @ v.transpose(-1, -2)
    dwl, dww = torch.zeros(H, H, device='cuda'), torch.zeros(H, H, device='cuda')
    dsb = ops.attn_mix_bwd(qkv.cuda(), d_ctx.to(torch.bfloat16).cuda(), B, N, H, hd, wl.cuda(), ww.cuda(), lse, scale, dwl, dww)
    dS = ops.unblock_scores(dsb)[..., :N]
    s64 = raw * scale
    wld, wwd = wl.double(), ww.double()
    p64 = torch.softmax(torch.einsum('gh,bhij->bgij', wld, s64), -1)
    dp = torch.einsum('gh,bgij->bhij', wwd, dr)
    dp_abs = torch.einsum('gh,bgij->bhij', wwd.abs(), dr.abs())
    da_ref = p64 * (dp - (p64 * dp).sum(-1, keepdim=True))
    ds_ref = torch.einsum('gh,bgij->bhij', wld, da_ref)
    t1 = torch.einsum('gh,bgij->bhij', wld.abs(), da_ref.abs())
    t2 = torch.einsum('gh,bgij->bhij', wld.abs(), p64 * dp_abs)
    # + the forward's f16 path: P here is recomputed from f16 operands (exponent error ~ 2^-11 |A| beyond the exact reference)
    pf = U_F16 * torch.einsum('gh,bhij->bgij', wld.abs(), s64.abs()).amax(-1, keepdim=True)
    tol = 2 * U_BF16 * (2 * t1 + t2) + 2 * pf * t2 + U_BF16 * ds_ref.abs() + EPS
    _within(dS, ds_ref, tol, f'dS (register mix, |c| ~ {mag})')
    dww_ref = torch.einsum('bgij,bhij->gh', dr, p64)
    dww_tol = (2 * U_BF16 + 2 * pf.max().item()) * torch.einsum('bgij,bhij->gh', dr.abs(), p64) + EPS
    _within(dww, dww_ref, dww_tol, f'dW_w (register mix, |c| ~ {mag})')
    dwl_ref = torch.einsum('bgij,bhij->gh', da_ref, s64)
    dwl_tol = (2 * U_BF16 + 2 * pf.max().item()) * torch.einsum('bgij,bhij->gh', da_ref.abs() + p64 * dp_abs, s64.abs()) + EPS
    _within(dwl, dwl_ref, dwl_tol, f'dW_l (register mix, |c| ~ {mag})')
    print(f'dW_l error growth: register H={H} hd={hd} |c|~{mag}: max |err| {(dwl.double().cpu() - dwl_ref).abs().max().item():.3e}, '
          f'max |dW_l| {dwl_ref.abs().max().item():.3e}, bound {dwl_tol.max().item():.3e}')
