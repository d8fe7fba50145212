"""GPU parity of the MFMA GEMM kernels against torch fp32 on the SAME bf16-rounded operands, over many shapes.

Every comparison here is max |got - ref| over max |ref|: 1e-5 sqrt(K) for f32 outputs (bf16 products are exact in fp32, the difference is
the fp32 summation order), 6e-3 to 8e-3 -- several bf16 roundings -- for bf16 / f16 outputs, 2e-3 to 3e-3 for column sums.  That resolves
neither a single rounding nor a single row or operand: the per-element checks (float64 reference, bit equality on integer operands,
derived bounds on real ones, ownership of the output buffers, every tile height) are in tests/test_gemm_exact_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).cuda()


def _dg(aux):
    """the saved gelu' from its 8-bit fixed-point code (include/dclip.h, DCLIP_ACT_GELU_SAVE)"""
    from distillclip_amd import ops
    return aux.float() * ops.DG_STEP + ops.DG_LO


def _close(got, ref, tol):
    err = (got.float() - ref).abs().max().item()
    den = ref.abs().max().item() + 1e-6
    assert err / den < tol, (err, den)


@pytest.mark.parametrize('M,N,K', [(128, 128, 64), (200, 192, 128), (37, 64, 64), (1000, 768, 768), (256, 2304, 768),
                                   (3 * 17, 128, 192)])
def test_gemm_nt_plain(M, N, K):
    from distillclip_amd import ops
    a, b = _rand((M, K), 1), _rand((N, K), 2)
    ref = a.float() @ b.float().t()
    _close(ops.gemm_nt(a, b, out_dtype=torch.float32), ref, 1e-5 * K ** 0.5 + 1e-5)
    _close(ops.gemm_nt(a, b), ref, 6e-3)


def test_gemm_nt_asymmetric_identity():
    """A = I with an asymmetric B catches a transposed C-write (guide §3)."""
    from distillclip_amd import ops
    n = 128
    a = torch.eye(n, dtype=torch.bfloat16, device='cuda')
    b = (torch.arange(n * n, device='cuda').reshape(n, n) % 251).to(torch.bfloat16)
    out = ops.gemm_nt(a, b, out_dtype=torch.float32)
    assert torch.equal(out, b.float().t())


@pytest.mark.parametrize('act', ['none', 'quickgelu', 'gelu'])
def test_gemm_nt_epilogue(act):
    from distillclip_amd import ops
    M, N, K = 300, 256, 128
    a, b = _rand((M, K), 3), _rand((N, K), 4, 0.1)
    bias = torch.randn(N, device='cuda')
    res = torch.randn(M, N, device='cuda')
    z = a.float() @ b.float().t() * 0.5 + bias
    f = {'none': lambda t: t, 'quickgelu': lambda t: t * torch.sigmoid(1.702 * t),
         'gelu': torch.nn.functional.gelu}[act]
    aux = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
    out = ops.gemm_nt(a, b, bias=bias, act=act, aux_out=aux, residual=res, out_dtype=torch.float32, alpha=0.5)
    _close(aux, z, 6e-3)
    # the activation is applied to the fp32 value, not to the bf16-rounded aux
    _close(out, f(z) + res, 1e-4)
    # in-place residual (C aliases residual)
    x = res.clone()
    ops.gemm_nt(a, b, bias=bias, act=act, residual=x, out=x, alpha=0.5)
    _close(x, f(z) + res, 1e-4)


def test_gemm_nt_dgelu():
    from distillclip_amd import ops
    M, N, K = 130, 128, 64
    a, b = _rand((M, K), 5), _rand((N, K), 6, 0.2)
    z = _rand((M, N), 7)
    zf = z.float().requires_grad_(True)
    torch.nn.functional.gelu(zf).sum().backward()
    cs = torch.zeros(N, device='cuda')
    out = ops.gemm_nt(a, b, act='dgelu', aux_in=z, out_dtype=torch.float32, colsum=cs)
    _close(out, (a.float() @ b.float().t()) * zf.grad, 1e-4)
    _close(cs, out.sum(0), 1e-5)
    a2, b2 = _rand((2100, 128), 15), _rand((512, 128), 16, 0.2)           # 256x256 kernel path
    cs2 = torch.zeros(512, device='cuda')
    o2 = ops.gemm_nt(a2, b2, out_dtype=torch.float32, colsum=cs2)
    _close(cs2, o2.sum(0), 1e-5)


def test_gemm_nt_patch_rowmap():
    from distillclip_amd import ops
    Bn, G, N, K = 5, 9, 128, 192
    a, b = _rand((Bn * G, K), 8), _rand((N, K), 9, 0.1)
    bias = torch.randn(N, device='cuda')
    pos = torch.randn(G + 1, N, device='cuda')
    pos = pos[:G].contiguous()
    out = ops.gemm_nt(a, b, bias=bias, out_dtype=torch.float32, row_group=G, rowadd=pos)
    ref = (a.float() @ b.float().t() + bias).view(Bn, G, N) + pos
    _close(out.view(Bn, G, N), ref, 1e-4)


def test_gemm_nt_rejects_bad_k():
    from distillclip_amd import ops
    with pytest.raises(ValueError):
        ops.gemm_nt(_rand((64, 48), 1), _rand((64, 48), 2))


@pytest.mark.parametrize('M,P,Q,splits', [(64, 128, 128, 1), (200, 64, 192, 2), (1000, 768, 256, 4), (37, 16, 24, 1),
                                          (3 * 17, 384, 128, 3), (1024, 768, 256, 4), (640, 72, 200, 3), (4096, 128, 3072, 7),
                                          (128, 8, 8, 2)])
def test_gemm_tn_acc(M, P, Q, splits):
    from distillclip_amd import ops
    a, b = _rand((M, P), 11), _rand((M, Q), 12)
    dw = torch.ones(P, Q, device='cuda')
    ops.gemm_tn_acc(a, b, dw, splits)
    ops.gemm_tn_acc(a, b, dw, splits)          # accumulates (weight sharing: R uses per step)
    ref = 1 + 2 * (a.float().t() @ b.float())
    _close(dw, ref, 1e-5 * M ** 0.5 + 1e-5)


@pytest.mark.parametrize('M,P,Q', [(4096, 1024, 1024), (8192, 3072, 768), (6400, 768, 3072), (4160, 2304, 768)])
def test_gemm_tn_256_pipeline(M, P, Q):
    """wgrad shapes routed to the 256x256 staggered pipeline (P, Q % 256 == 0, >= 16 tiles, M % 64 == 0)"""
    from distillclip_amd import ops
    a, b = _rand((M, P), 31), _rand((M, Q), 32)
    dw = torch.full((P, Q), 0.5, device='cuda')
    ops.gemm_tn_acc(a, b, dw, 4)
    ref = 0.5 + a.float().t() @ b.float()
    _close(dw, ref, 1e-5 * M ** 0.5 + 1e-5)
    # a second, independent accumulation must add exactly one more product (no lost / duplicated contributions)
    ops.gemm_tn_acc(a, b, dw, 4)
    _close(dw, 2 * ref - 0.5, 1e-5 * M ** 0.5 + 1e-5)
    # partial tiles + fixed-order sum: run-to-run IDENTICAL gradients (the atomic path is only equal up to f32 summation order)
    d1, d2 = torch.zeros(P, Q, device='cuda'), torch.zeros(P, Q, device='cuda')
    ops.gemm_tn_acc(a, b, d1, 4)
    ops.gemm_tn_acc(a, b, d2, 4)
    assert torch.equal(d1, d2)
    d3 = torch.zeros(P, Q, device='cuda')
    ops.gemm_tn_acc(a, b, d3, 4, workspace=False)                  # the f32-atomic epilogue of the same kernel
    _close(d3, d1, 1e-5 * M ** 0.5 + 1e-5)


def test_gemm_tn_asymmetric():
    from distillclip_amd import ops
    M = 64
    a = torch.zeros(M, 32, device='cuda')
    a[torch.arange(32), torch.arange(32)] = 1          # A^T picks rows 0..31 of B
    b = (torch.arange(M * 48, device='cuda').reshape(M, 48) % 127).float()
    dw = torch.zeros(32, 48, device='cuda')
    ops.gemm_tn_acc(a.bfloat16(), b.bfloat16(), dw, 1)
    assert torch.equal(dw, b[:32])


def test_colsum():
    from distillclip_amd import ops
    x = _rand((1037, 300), 13)
    db = torch.zeros(300, device='cuda')
    ops.colsum_acc(x, db)
    _close(db, x.float().sum(0), 1e-5)
    # 16-byte path (N % 8 == 0): ragged rows, a column slice of a wider buffer (ld > N), the qkv-bias shape of the step
    for M, N, full in ((1037, 304, 304), (4099, 768, 2304), (51200, 2304, 2304)):
        xf = _rand((M, full), 14)
        xs = xf[:, full - N:]
        db = torch.ones(N, device='cuda')
        ops.colsum_acc(xs, db)
        _close(db, 1.0 + xs.float().sum(0), 2e-5 * max(1.0, (M / 1000) ** 0.5))


@pytest.mark.parametrize('M,N,K', [(1024, 256, 64), (1024, 256, 128), (1100, 264, 192), (2048, 768, 768), (1500, 512, 256),
                                   (4096, 2304, 768), (3000, 320, 3072)])
def test_gemm_nt_256_tile_kernel(M, N, K):
    """shapes routed to the 256x256 staggered-pipeline kernel (M >= 1024, N >= 256): edges, short K, long K"""
    from distillclip_amd import ops
    a, b = _rand((M, K), 21), _rand((N, K), 22, 0.2)
    ref = a.float() @ b.float().t()
    _close(ops.gemm_nt(a, b, out_dtype=torch.float32), ref, 1e-5 * K ** 0.5 + 1e-5)
    bias = torch.randn(N, device='cuda')
    res = torch.randn(M, N, device='cuda')
    aux = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
    out = ops.gemm_nt(a, b, bias=bias, act='gelu', aux_out=aux, residual=res, out_dtype=torch.float32)
    z = ref + bias
    _close(aux, z, 6e-3)
    _close(out, torch.nn.functional.gelu(z) + res, 1e-4)
    # repeated launches must be bit-identical (no LDS race)
    o1 = ops.gemm_nt(a, b)
    for _ in range(5):
        assert torch.equal(ops.gemm_nt(a, b), o1)


def test_gelu_epilogue_accuracy_over_range():
    """the fused exact-GELU / GELU' epilogues use a branch-free erf (A&S 7.1.26): check against torch over the whole range"""
    from distillclip_amd import ops
    n = 256
    a = torch.eye(n, dtype=torch.bfloat16, device='cuda')
    x = torch.linspace(-9, 9, n * n, device='cuda').reshape(n, n).to(torch.bfloat16)     # identity GEMM: out = act(x^T)
    ref = x.float().t()
    out = ops.gemm_nt(a, x, act='gelu', out_dtype=torch.float32)
    assert (out - torch.nn.functional.gelu(ref)).abs().max().item() < 2e-6
    z = x.t().contiguous()
    zf = z.float().requires_grad_(True)
    torch.nn.functional.gelu(zf).sum().backward()
    ones = torch.ones(n, n, dtype=torch.bfloat16, device='cuda')
    d = ops.gemm_nt(a, ones, act='dgelu', aux_in=z, out_dtype=torch.float32)               # 1 * gelu'(z)
    assert (d - zf.grad).abs().max().item() < 2e-6
    # the pair the training towers use: forward stores gelu'(z) as 8-bit fixed point, backward multiplies by it
    saved = torch.empty(n, n, dtype=torch.uint8, device='cuda')
    out2 = ops.gemm_nt(a, x, act='gelu_save', aux_out=saved, out_dtype=torch.float32)
    assert torch.equal(out2, out)
    assert (_dg(saved) - zf.grad).abs().max().item() <= 0.5 * ops.DG_STEP + 1e-6              # the nearest code of a value in [-0.13, 1.13]
    want_code = torch.clamp(torch.round((zf.grad - ops.DG_LO) / ops.DG_STEP), 0, 255)
    assert (saved.float() - want_code).abs().max().item() <= 1 and (saved.float() != want_code).float().mean().item() < 2e-3   # (ties of the f32 erf)
    d2 = ops.gemm_nt(a, ones, act='mulaux', aux_in=saved, out_dtype=torch.float32)
    _close(d2, _dg(saved), 1e-6)


@pytest.mark.parametrize('M,N,K', [(22272, 768, 128), (19800, 512, 64)])
def test_gemm_nt_row_split_between_tile_sizes(M, N, K):
    """T = 261 / 156 x 2 = 312 tiles of 256^2, ragged last row tile: every row-indexed operand (residual, aux_in / aux_out, column sums)
    of the epilogue, here in the combinations only the general (run-time tested) epilogue mode serves."""
    from distillclip_amd import ops
    a, b = _rand((M, K), 31), _rand((N, K), 32, 0.2)
    bias = torch.randn(N, device='cuda')
    ref = a.float() @ b.float().t()
    _close(ops.gemm_nt(a, b, out_dtype=torch.float32), ref, 1e-5 * K ** 0.5 + 1e-5)
    res = torch.randn(M, N, device='cuda')
    aux = torch.empty(M, N, dtype=torch.uint8, device='cuda')
    cs = torch.zeros(N, device='cuda')
    out = ops.gemm_nt(a, b, bias=bias, act='gelu_save', aux_out=aux, residual=res, out_dtype=torch.float32, colsum=cs)
    z = (ref + bias).requires_grad_(True)
    y = torch.nn.functional.gelu(z)
    y.sum().backward()
    _close(out, y.detach() + res, 1e-4)
    assert (_dg(aux) - z.grad).abs().max().item() <= 0.5 * ops.DG_STEP + 1e-5
    _close(cs, out.sum(0), 2e-4)
    d = ops.gemm_nt(a, b, act='mulaux', aux_in=aux, out_dtype=torch.bfloat16)
    _close(d, ref * _dg(aux), 6e-3)
    x = res.clone()
    ops.gemm_nt(a, b, bias=bias, residual=x, out=x)                       # in-place residual stream
    _close(x, ref + bias + res, 1e-4)


@pytest.mark.parametrize('M,N,K', [(25600, 768, 128), (25610, 768, 64), (39424, 512, 192), (20480, 1024, 64), (25600, 768, 768),
                                   (12800, 768, 768), (12810, 768, 128), (12800, 768, 3072)])
def test_gemm_nt_320_row_tile_variant(M, N, K):
    """(The M = 12 800 cases — image.yaml at B = 256 — run on the 192 x 256 tile: 201 workgroups instead of 120 of 320 rows.)
    Shapes whose 256^2 tiling leaves a nearly empty last round on 256 CUs ([25600, 768] = 300 tiles, [39424, 512] = 308) run on
    320 x 256 tiles (240 / 248 workgroups, one round): full and ragged last row tile, every epilogue the towers use with it
    (bias, f32 + residual, in-place residual, QuickGELU / GELU + saved pre-activation, positional row table, column sums), and
    bit-identical repeats (LDS-DMA races show as run-to-run differences)."""
    from distillclip_amd import ops
    a, b = _rand((M, K), 41), _rand((N, K), 42, 0.2)
    ref = a.float() @ b.float().t()
    _close(ops.gemm_nt(a, b, out_dtype=torch.float32), ref, 1e-5 * K ** 0.5 + 1e-5)
    o1 = ops.gemm_nt(a, b)
    _close(o1, ref, 6e-3)
    for _ in range(4):
        assert torch.equal(ops.gemm_nt(a, b), o1)
    bias = torch.randn(N, device='cuda')
    res = torch.randn(M, N, device='cuda')
    cs = torch.zeros(N, device='cuda')
    out = ops.gemm_nt(a, b, bias=bias, residual=res, out_dtype=torch.float32, colsum=cs)
    _close(out, ref + bias + res, 1e-4)
    _close(cs, out.sum(0), 3e-4)
    x = res.clone()
    ops.gemm_nt(a, b, bias=bias, residual=x, out=x)                       # in-place f32 residual stream (student inference towers)
    _close(x, ref + bias + res, 1e-4)
    # the frozen teacher's residual stream is fp16 (reference `precision: 16`): fp16 residual in, fp16 out, in place and out of place
    xh = res.to(torch.float16)
    want_h = (ref + bias + xh.float())
    oh = ops.gemm_nt(a, b, bias=bias, residual=xh, out_dtype=torch.float16)
    assert oh.dtype == torch.float16
    _close(oh, want_h, 1.2e-3)                                            # one fp16 rounding (2^-11) on top of the f32 accumulation
    ops.gemm_nt(a, b, bias=bias, residual=xh, out=xh)
    assert torch.equal(xh, oh)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
    z = ref + bias
    q = ops.gemm_nt(a, b, bias=bias, act='quickgelu')
    _close(q, z * torch.sigmoid(1.702 * z), 6e-3)
    g = ops.gemm_nt(a, b, bias=bias, act='gelu', aux_out=aux)
    _close(g, torch.nn.functional.gelu(z), 6e-3)
    _close(aux, z, 6e-3)
    G = 50
    if M % G == 0:
        pos = torch.randn(G, N, device='cuda')
        o = ops.gemm_nt(a, b, out_dtype=torch.float32, row_group=G, rowadd=pos)
        _close(o.view(M // G, G, N), ref.view(M // G, G, N) + pos, 1e-4)
        oh = ops.gemm_nt(a, b, out_dtype=torch.float16, row_group=G, rowadd=pos)       # the teacher's patch embedding writes fp16
        assert torch.equal(oh, o.to(torch.float16))


@pytest.mark.parametrize('M,N,K', [(4096, 3072, 768), (25600, 2312, 128), (2100, 520, 192), (39424, 3072, 64), (12800, 768, 192)])
def test_gemm_nt_register_epilogue_variants(M, N, K):
    """The 256- / 320-row kernels store straight from the accumulators (operand-swapped MFMA, permuted B staging): every epilogue
    variant with bf16 output, including the column sums reduced by lane shuffles (the dgrad GEMMs' bias gradients), on shapes that
    exercise the grouped tile raster (12 column tiles, K = 768), a ragged last column tile (N = 2312, 520), ragged rows, and the
    320-row tile with the DGELU / MULAUX / GELU-saving epilogues."""
    from distillclip_amd import ops
    a, b = _rand((M, K), 51), _rand((N, K), 52, 0.2)
    ref = a.float() @ b.float().t()
    bias = torch.randn(N, device='cuda')
    z = _rand((M, N), 53)
    tol = 8e-3
    # plain + bias, bf16, with column sums
    cs = torch.zeros(N, device='cuda')
    o = ops.gemm_nt(a, b, bias=bias, colsum=cs)
    _close(o, ref + bias, tol)
    _close(cs, o.float().sum(0), 2e-3)          # sums of the f32 values before the bf16 rounding of the stored copy
    # MULAUX (dz = (dY W) o saved gelu') and DGELU, with column sums
    zq = torch.randint(0, 256, (M, N), dtype=torch.uint8, device='cuda')
    for act, aux_in, want in (('mulaux', zq, ref * _dg(zq)),
                              ('dgelu', z, ref * torch.autograd.functional.vjp(torch.nn.functional.gelu, z.float(), torch.ones_like(ref))[1])):
        cs = torch.zeros(N, device='cuda')
        o = ops.gemm_nt(a, b, act=act, aux_in=aux_in, colsum=cs)
        _close(o, want, tol)
        _close(cs, want.sum(0), 3e-3)
    # GELU with the saved derivative (training towers' fc1)
    aux = torch.empty(M, N, dtype=torch.uint8, device='cuda')
    zz = (ref + bias).requires_grad_(True)
    g = torch.nn.functional.gelu(zz)
    g.sum().backward()
    o = ops.gemm_nt(a, b, bias=bias, act='gelu_save', aux_out=aux)
    _close(o, g.detach(), tol)
    assert (_dg(aux) - zz.grad).abs().max().item() <= 0.5 * ops.DG_STEP + 1e-5
    # f32 output with a residual read through the side-operand ring, bf16 output with an (inline) residual
    res = torch.randn(M, N, device='cuda')
    _close(ops.gemm_nt(a, b, bias=bias, residual=res, out_dtype=torch.float32), ref + bias + res, 1e-4 * max(1.0, K ** 0.5 / 8))
    _close(ops.gemm_nt(a, b, bias=bias, residual=res), ref + bias + res, tol)
    resh = res.to(torch.float16)
    _close(ops.gemm_nt(a, b, bias=bias, residual=resh, out_dtype=torch.float16), ref + bias + resh.float(), 1.5e-3 * max(1.0, K ** 0.5 / 8))
    o1 = ops.gemm_nt(a, b, bias=bias, act='quickgelu')
    for _ in range(3):
        assert torch.equal(ops.gemm_nt(a, b, bias=bias, act='quickgelu'), o1)


def test_random_shapes_gemm_attention_products_wgrad_layernorm():
    """16 random shapes through gemm_nt (every epilogue the towers use), gemm_tn_acc, the attention products (row-major and quad-blocked
    operand), the teacher's fused attention (causal and not) and LayerNorm forward, against torch fp32 on the same bf16 inputs, run-to-run
    equality included (tools/diag/kernel_fuzz.py; the fixed shape lists above cannot cover what a fuzz of the score stage found in round 3)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.cuda.synchronize()
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'diag', 'kernel_fuzz.py'), '16', '41'], capture_output=True, text=True,
                       timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
