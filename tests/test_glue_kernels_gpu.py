"""The glue kernels between a tower's GEMMs (elementwise.hip), the feature MSE (loss.hip) and the persistent-grid LayerNorm backward
(layernorm.hip), each against a plain float64 torch reference of the same operation, at the shapes, dtypes and edge paths the tower
tests cannot resolve.

Tolerance rules (each test's docstring names the one it uses):
  exact      -- the kernel moves data or rounds once: bit equality (NaN positions compared with isnan).  Outputs are pre-filled with a
                NaN pattern, so an element the kernel never writes shows up.
  sum bound  -- the kernel sums in an order it does not fix (f32 atomics, split reductions): per element
                |got - ref64| <= n 2^-23 sum|terms| (the initial accumulator value is one of the n terms), and also the 2e-5
                relative-to-max form of test_kernels_gpu.py, so neither is ever looser than what that file asserts.
Accumulator elements no term reaches (table rows whose ids never occur, rows outside the picked ones) must be bit-unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23
_POOL_N = 36_000_000


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).cuda()


_POOL = {}


def _pool(n, off=0):
    """elements [off, off + n) of one seeded N(0, 1) f32 buffer on the GPU, drawn once per process: the real-shape cases take views of it
    instead of drawing tens of millions of values each (off a multiple of 4 keeps the view 16-byte aligned)"""
    assert off % 4 == 0 and off + n <= _POOL_N
    if 'x' not in _POOL:
        _POOL['x'] = torch.randn(_POOL_N, generator=_gen(20261016)).cuda()
    return _POOL['x'][off:off + n]


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[t.dtype])


def _nan_like(shape, dtype):
    """an output buffer filled with all-ones bits (a NaN in every float type)"""
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.int32: torch.int32}[dtype]
    return torch.full(shape, -1, dtype=it, device='cuda').view(dtype)


def _exact(got, want, what=''):
    """exact rule: same NaN positions, every other element bit-equal (so -0 != +0)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, 'NaN positions differ', int((gn != wn).sum()))
    bad = _bits(got) != _bits(want)
    bad &= ~gn
    assert not bad.any(), (what, int(bad.sum()), 'first at', torch.nonzero(bad)[0].tolist())


def _close(got, ref, tol, what=''):
    err = (got.double() - ref.double()).abs().max().item()
    den = ref.double().abs().max().item() + 1e-9
    assert err / den < tol, (what, err, den)


def _sum_bound(got, ref64, nterms, abs_terms, what=''):
    """sum-bound rule: |got - ref64| <= n 2^-23 sum|terms| per element, and the 2e-5 relative-to-max form"""
    err = (got.double() - ref64).abs()
    bound = nterms * U23 * abs_terms
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), 'worst excess', (err - bound).max().item())
    _close(got, ref64, 2e-5, what)


def _raw_row_entry(name, argtypes):
    """dclip_rows_pick / dclip_rows_expand are declared in csrc/common.h only (not in the ABI header): the binding hands back the raw
    ctypes function, typed here from those prototypes"""
    fn = getattr(_lib(), name)
    fn.argtypes = argtypes
    fn.restype = ctypes.c_int
    return fn


def _rows_pick(src, dst, idx, B, row_bytes):
    f = _raw_row_entry('dclip_rows_pick', [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_void_p])
    assert f(_p(src), _p(dst), _p(idx), B, row_bytes, _st()) == 0


def _rows_expand(src, dst, idx, B, N, row_bytes):
    f = _raw_row_entry('dclip_rows_expand', [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_void_p])
    assert f(_p(src), _p(dst), _p(idx), B, N, row_bytes, _st()) == 0


def _pick(ids, id_stride, B, N):
    idx = _nan_like((B,), torch.int32)
    _lib().dclip_pick_index(_p(ids), id_stride, _p(idx), B, N, _st())
    return idx


def _captions(seed, B, N, V, lo=5, hi=40):
    from distillclip_amd import synth
    return torch.from_numpy(synth.captions(seed, B, N, V, lo, hi)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. embed_gather
# ---------------------------------------------------------------------------------------------------------------------------------
_OUT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}


def _gather_ref(ids, id_stride, table, pos, B, N, dt):
    rows = ids.reshape(B, id_stride)[:, :N].reshape(-1)
    v = table.double()[rows]
    if pos is not None:
        v = v + pos.double().repeat(B, 1)
    return v.float().to(dt)                      # the f32 sum rounded once (RNE), then the one cast of the output type


@pytest.mark.parametrize('out_dtype', [0, 1, 2])
@pytest.mark.parametrize('with_pos', [True, False])
@pytest.mark.parametrize('B,id_stride,N,D,V', [(3, 77, 20, 4, 50), (5, 13, 13, 100, 97), (2, 77, 77, 512, 300), (7, 77, 20, 100, 1000)])
def test_embed_gather(out_dtype, with_pos, B, id_stride, N, D, V):
    """dclip_embed_gather out[r] = table[ids[(r / N) * id_stride + r % N]] + pos[r % N] for bf16 / f32 / f16 outputs, with and without
    pos, id_stride > N (a caption prefix) and D of 4, 100, 512.  Rule: exact (one RNE rounding of the f32 sum)."""
    seed = out_dtype * 100 + B * 7 + D
    ids = torch.randint(0, V, (B, id_stride), generator=_gen(seed)).cuda()
    table, pos = _randn((V, D), seed + 1), (_randn((N, D), seed + 2) if with_pos else None)
    dt = _OUT[out_dtype]
    out = _nan_like((B * N, D), dt)
    _lib().dclip_embed_gather(_p(ids), id_stride, _p(table), _p(pos), _p(out), out_dtype, B * N, N, D, _st())
    _exact(out, _gather_ref(ids, id_stride, table, pos, B, N, dt), 'gather')


@pytest.mark.parametrize('out_dtype,with_pos,D', [(1, True, 512), (2, True, 512), (0, False, 256)])
def test_embed_gather_real_shapes(out_dtype, with_pos, D):
    """the text tower's gather at B = 512, N = 77, vocab 49408: the plain tower (f32 / f16 rows, pos added, D = 512) and the compressed
    one (bf16 rows, pos = NULL, D = embed_rank = 256).  Rule: exact."""
    B, N, V = 512, 77, 49408
    ids = _captions(5, B, N, V)
    table = _pool(V * D).reshape(V, D)
    pos = _pool(N * D, 30_000_000).reshape(N, D) if with_pos else None
    dt = _OUT[out_dtype]
    out = _nan_like((B * N, D), dt)
    _lib().dclip_embed_gather(_p(ids), N, _p(table), _p(pos), _p(out), out_dtype, B * N, N, D, _st())
    _exact(out, _gather_ref(ids, N, table, pos, B, N, dt), 'gather')


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. embed_scatter_add
# ---------------------------------------------------------------------------------------------------------------------------------
def _scatter_ids(layout, B, N, V, seed):
    if layout == 'clip':                    # clip.tokenize layout: SOT, words, EOT, padding 0 (hot ids 0 / V-2 / V-1)
        ids = _captions(seed, B, N, V, 3 if N < 20 else 5, 9 if N < 20 else 40).reshape(-1)
        assert (ids == 0).any() and (ids == V - 2).sum() == B and (ids == V - 1).sum() == B
    elif layout == 'cold':                  # no hot id at all: every row goes through the per-row atomics
        ids = torch.randint(1, V - 2, (B * N,), generator=_gen(seed)).cuda()
        assert not ((ids == 0) | (ids >= V - 2)).any()
    else:                                   # vocab 3: every id is hot, the per-row kernel skips every row
        assert V == 3
        ids = torch.randint(0, 3, (B * N,), generator=_gen(seed)).cuda()
    return ids


def _check_scatter(ids, dx, t0, V, D):
    rows = ids.numel()
    got = t0.clone()
    _lib().dclip_embed_scatter_add(_p(ids), _p(dx), 1 if dx.dtype == torch.float32 else 0, _p(got), rows, D, V, _st())
    ref = t0.double().index_add_(0, ids, dx.double())
    absum = t0.double().abs().index_add_(0, ids, dx.double().abs())
    cnt = torch.zeros(V, dtype=torch.float64, device='cuda').index_add_(0, ids, torch.ones(rows, dtype=torch.float64, device='cuda'))
    _sum_bound(got, ref, (cnt + 1)[:, None], absum, 'dtable')
    _close(got, ref, 1e-5, 'dtable (test_kernels_gpu form)')
    cold = cnt == 0
    assert torch.equal(_bits(got[cold]), _bits(t0[cold])), 'a table row no id points at was written'


@pytest.mark.parametrize('layout', ['clip', 'cold', 'all_hot'])
@pytest.mark.parametrize('D', [64, 100, 256, 300, 512, 768])
@pytest.mark.parametrize('dx_dtype', [torch.float32, torch.bfloat16])
def test_embed_scatter_add(layout, D, dx_dtype):
    """dclip_embed_scatter_add dtable[ids[r]] += dx[r] over 37 x 13 rows: f32 and bf16 dx; D below, at and past the 256-column chunk
    of a wave, not a multiple of 64; the clip caption layout, a batch without hot ids, and vocab 3 (every id hot).  Rule: sum bound
    (n = rows with that id + 1), also <= 1e-5 of the max like test_kernels_gpu.py; rows never hit bit-unchanged."""
    B, N = 37, 13
    V = 3 if layout == 'all_hot' else 97
    ids = _scatter_ids(layout, B, N, V, D)
    dx = _randn((B * N, D), D + 1).to(dx_dtype)
    _check_scatter(ids, dx, _randn((V, D), D + 2), V, D)


@pytest.mark.parametrize('layout,V,D,dx_dtype', [('clip', 49408, 512, torch.float32), ('clip', 49408, 512, torch.bfloat16),
                                                  ('clip', 49408, 256, torch.float32), ('cold', 4096, 768, torch.float32),
                                                  ('all_hot', 3, 300, torch.bfloat16)])
def test_embed_scatter_add_real_rows(layout, V, D, dx_dtype):
    """the same at the step's 512 x 77 = 39424 rows: the per-row kernel's grid (4096 x 4 waves) sweeps the rows more than twice.
    The plain text tower (D 512), the compressed one (D = embed_rank 256), a hot-free batch of 4096 ids (contended per-row atomics,
    D 768) and vocab 3.  Rule: sum bound, also <= 1e-5 of the max; rows never hit bit-unchanged."""
    B, N = 512, 77
    ids = _scatter_ids(layout, B, N, V, 9)
    dx = _pool(B * N * D).reshape(B * N, D).to(dx_dtype)
    t0 = _pool(V * D, 4_000_000).reshape(V, D).clone()
    _check_scatter(ids, dx, t0, V, D)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. token_table / token_table_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
# (class token, bias) of the four encoder.cpp call patterns
_TT = {'student_image': (True, True), 'clip_image': (True, False), 'compressed_text': (False, True), 'plain_text': (False, False)}


@pytest.mark.parametrize('pattern', list(_TT))
@pytest.mark.parametrize('ntok', [1, 50, 77, 101])
@pytest.mark.parametrize('D', [100, 768])
def test_token_table_and_adjoint(pattern, ntok, D):
    """dclip_token_table out[0] = pos[0] + cls, out[n] = pos[n] + bias (cls / bias NULL as encoder.cpp passes them) and
    dclip_token_table_bwd accumulating into non-zero gradients.  Rules: out, dpos, dcls exact (one rounding each); dbias sum bound
    over n >= has_cls (at ntok 1 with a class token: bit-unchanged); a float64 adjoint identity
    <table(pos, cls, bias), G> == <pos, dpos> + <cls, dcls> + <bias, dbias> within the rounding of out and of the dbias sums."""
    has_cls, has_bias = _TT[pattern]
    seed = ntok * 1000 + D
    pos = _randn((ntok, D), seed)
    cls = _randn((D,), seed + 1) if has_cls else None
    bias = _randn((D,), seed + 2) if has_bias else None
    out = _nan_like((ntok, D), torch.float32)
    _lib().dclip_token_table(_p(pos), _p(cls), _p(bias), _p(out), ntok, D, _st())
    add = torch.zeros(ntok, D, dtype=torch.float64, device='cuda')
    if has_bias:
        add[int(has_cls):] = bias.double()
    if has_cls:
        add[0] = cls.double()
    _exact(out, (pos.double() + add).float(), 'token table')

    G = _randn((ntok, D), seed + 3)
    dpos0, dcls0, dbias0 = _randn((ntok, D), seed + 4), _randn((D,), seed + 5), _randn((D,), seed + 6)
    dpos, dcls, dbias = dpos0.clone(), dcls0.clone(), dbias0.clone()
    _lib().dclip_token_table_bwd(_p(G), _p(dpos), _p(dcls) if has_cls else None, _p(dbias) if has_bias else None, ntok, D,
                                 int(has_cls), _st())
    _exact(dpos, (dpos0.double() + G.double()).float(), 'dpos')
    if has_cls:
        _exact(dcls, (dcls0.double() + G[0].double()).float(), 'dcls')
    Gb = G[int(has_cls):].double()
    if has_bias:
        if ntok == int(has_cls):
            assert torch.equal(_bits(dbias), _bits(dbias0)), 'dbias summed the class row'
        _sum_bound(dbias, dbias0.double() + Gb.sum(0), ntok - int(has_cls) + 1, dbias0.double().abs() + Gb.abs().sum(0), 'dbias')

    # adjoint identity, gradients from zero
    zp, zc, zb = torch.zeros_like(pos), torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
    _lib().dclip_token_table_bwd(_p(G), _p(zp), _p(zc) if has_cls else None, _p(zb) if has_bias else None, ntok, D, int(has_cls), _st())
    lhs = (out.double() * G.double()).sum().item()
    rhs = (pos.double() * zp.double()).sum().item()
    if has_cls:
        rhs += (cls.double() * zc.double()).sum().item()
    tol = 2.0 ** -24 * (out.double() * G.double()).abs().sum().item() + 1e-9
    if has_bias:
        rhs += (bias.double() * zb.double()).sum().item()
        tol += ntok * U23 * (bias.double().abs() * Gb.abs().sum(0)).sum().item()
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. batch_sum_acc
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 4, 5, 31, 32, 33, 100, 512])
@pytest.mark.parametrize('N', [1, 77])
@pytest.mark.parametrize('D', [4, 100, 768])
def test_batch_sum_acc(B, N, D):
    """dclip_batch_sum_acc out[n, :] += sum_b G[b, n, :]: B not a multiple of 4 (the tail loop) or of the 32-sample split (several
    z-splits adding to one non-zero out).  Rule: sum bound (n = B + 1)."""
    G = _pool(B * N * D).reshape(B, N, D)
    out0 = _randn((N, D), B * 10 + N + D)
    out = out0.clone()
    _lib().dclip_batch_sum_acc(_p(G), _p(out), B, N, D, _st())
    Gd = G.double()
    _sum_bound(out, out0.double() + Gd.sum(0), B + 1, out0.double().abs() + Gd.abs().sum(0), 'batch sum')


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pick_index
# ---------------------------------------------------------------------------------------------------------------------------------
_PREFIX = {13: 7, 64: 40, 65: 64, 77: 20, 200: 77}


def _pick_want(ids, B, N):
    """the documented contract: b * N + the first maximum over the whole id_stride (torch.argmax), else N - 1 when it lies past N"""
    am = ids.cpu().argmax(1)
    am = torch.where(am < N, am, torch.full_like(am, N - 1))
    return (torch.arange(B) * N + am).to(torch.int32)


def _hand_rows(S):
    """id rows built around the ways the wave reduction can go wrong"""
    g = _gen(S)
    base = lambda: torch.randint(-10, 1, (S,), generator=g)
    rows = [torch.full((S,), 5, dtype=torch.int64),                                  # all tied: position 0
            torch.randint(-1000, -1, (S,), generator=g),                             # all negative
            torch.full((S,), -2 ** 63, dtype=torch.int64)]                           # all the most negative id
    for a, b in [(1, 2), (S - 2, S - 1), (62, 63), (63, 64), (0, 64), (S - 65, S - 1), (3, 67), (0, 128), (64, 128), (1, 129)]:
        if 0 <= a < b < S:                                                           # a tie across lanes (b - a < 64) or in one lane
            r = base()
            r[a] = r[b] = 7
            rows.append(r)
    for p in [0, S - 1, S // 2, min(S - 1, 64)]:                                    # one unique maximum (past N for the prefix cases)
        r = base()
        r[p] = 3
        rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize('S', [13, 64, 65, 77, 200])
@pytest.mark.parametrize('prefix', [False, True])
def test_pick_index_hand_built_rows(S, prefix):
    """dclip_pick_index on hand-built rows: ties at (n, n + 1) across lanes, (63, 64) where the later lane holds the earlier position,
    (n, n + 64) / (n, n + 128) within one lane; negative ids down to -2^63; a unique maximum before and past N.  id_stride S with
    N = S and N < S.  Rule: exact against the contract (torch.argmax, first maximum; N - 1 past the prefix)."""
    ids = _hand_rows(S).cuda()
    B, N = ids.shape[0], (_PREFIX[S] if prefix else S)
    got = _pick(ids, S, B, N)
    assert torch.equal(got.cpu(), _pick_want(ids, B, N)), (got.cpu().tolist(), _pick_want(ids, B, N).tolist())


@pytest.mark.parametrize('S', [13, 64, 65, 77, 200])
@pytest.mark.parametrize('prefix', [False, True])
@pytest.mark.parametrize('B', [1, 5, 513])
def test_pick_index_random_rows(S, prefix, B):
    """random rows of ids in [-3, 3] (ties everywhere, within and across lanes), B in {1, 5, 513} (not a multiple of the 4 waves of a
    workgroup), plus ids = NULL (the class-token row b * N).  Rule: exact."""
    ids = torch.randint(-3, 4, (B, S), generator=_gen(B * 1000 + S)).cuda()
    N = _PREFIX[S] if prefix else S
    assert torch.equal(_pick(ids, S, B, N).cpu(), _pick_want(ids, B, N))
    assert torch.equal(_pick(None, S, B, N).cpu(), (torch.arange(B) * N).to(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. rows_pick / rows_expand
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['16B', 'f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 5, 512])
@pytest.mark.parametrize('N', [13, 50, 77])
def test_rows_pick_expand(kind, B, N):
    """dclip_rows_pick dst[b] = src[idx[b]] and dclip_rows_expand (every row of [B*N, .] written: the compact row at idx[b], zeros
    elsewhere) with idx from dclip_pick_index; rows of 16 bytes, 768 f32 and 768 bf16; expand(pick(x)) == x masked to the picked rows
    (at B = 512 the expand grid sweeps its chunks four times).  Rule: exact (data moves only)."""
    D = 768
    if kind == '16B':
        x = _pool(B * N * 4).reshape(B * N, 4)
    elif kind == 'f32':
        x = _pool(B * N * D).reshape(B * N, D)
    else:
        x = _pool(B * N * D).reshape(B * N, D).bfloat16()
    row_bytes = x.shape[1] * x.element_size()
    ids = torch.randint(0, 1000, (B, N), generator=_gen(B + N)).cuda()
    idx = _pick(ids, N, B, N)
    sel = idx.long()
    picked = _nan_like((B, x.shape[1]), x.dtype)
    _rows_pick(x, picked, idx, B, row_bytes)
    _exact(picked, x[sel], 'rows_pick')
    full = _nan_like(x.shape, x.dtype)
    _rows_expand(picked, full, idx, B, N, row_bytes)
    want = torch.zeros_like(x)
    want[sel] = x[sel]
    _exact(full, want, 'rows_expand(rows_pick(x))')


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. im2row
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res,patch,C', [(224, 32, 3), (336, 32, 3), (36, 8, 1), (32, 8, 3)])
@pytest.mark.parametrize('cls_rows', [0, 1])
def test_im2row(res, patch, C, cls_rows):
    """dclip_im2row: rows (b, cls + py G + px), columns (c, ky, kx) as F.unfold orders them (= the conv weight layout); res % patch
    trailing pixels dropped (336 / 32 drops 16); a zero class row first when cls_rows = 1.  Rules: exact against the unfold reference
    cast to bf16; and rows @ W^T == conv2d(bf16-rounded image, W, stride=patch) in float64 to the f64 summation order only."""
    B, G = 2, res // patch
    K, L = C * patch * patch, G * G + cls_rows
    img = _randn((B, C, res, res), res + patch + C)
    out = _nan_like((B * L, K), torch.bfloat16)
    _lib().dclip_im2row(_p(img), _p(out), B, C, res, patch, cls_rows, _st())
    cols = F.unfold(img.double(), patch, stride=patch).transpose(1, 2)             # [B, G*G, K], (c, ky, kx)
    if cls_rows:
        cols = torch.cat([torch.zeros(B, 1, K, dtype=torch.float64, device='cuda'), cols], 1)
    _exact(out, cols.reshape(B * L, K).float().bfloat16(), 'im2row')

    Dout = 16
    W = _randn((Dout, C, patch, patch), 7).double()
    got = (out.double() @ W.reshape(Dout, -1).T).reshape(B, L, Dout)
    conv = F.conv2d(img.bfloat16().double(), W, stride=patch).flatten(2).transpose(1, 2)
    scale = (out.double().abs() @ W.reshape(Dout, -1).abs().T).reshape(B, L, Dout)
    if cls_rows:
        assert torch.equal(got[:, 0], torch.zeros_like(got[:, 0]))
        got, scale = got[:, 1:], scale[:, 1:]
    assert ((got - conv).abs() <= K * 2.0 ** -52 * scale).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. casts
# ---------------------------------------------------------------------------------------------------------------------------------
_CAST_N = [1, 2, 3, 4, 5, 1023, 1025, 8192 * 1024 + 3]

# f32 bit patterns: NaNs (a payload only in the low half would truncate to inf), +-inf, +-0, the largest finite value and the bf16
# rounding edges below it, RNE ties to even / odd and their neighbours, the smallest normal
_F32_SPECIAL = [0x7FC00000, 0x7F800001, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF,
                0x7F7F8000, 0x7F7F7FFF, 0x7F7F0000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF818000, 0x00800000, 0x80800000]


def _f32_cast_source(n, seed):
    """n f32 values without subnormals: random signs / exponents / upper mantissas, low halves drawn from the rounding edges
    (0x8000 ties, 0x7FFF, 0x8001, 0) or at random, the specials at the head and at the tail"""
    g = _gen(seed)
    hi = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    e = (hi >> 7) & 0xFF
    hi = torch.where(e == 0, hi | (1 << 7), hi)
    hi = torch.where(e == 0xFF, hi & ~(1 << 7), hi)
    lo = torch.tensor([0x8000, 0x7FFF, 0x8001, 0])[torch.randint(0, 4, (n,), generator=g)]
    lo = torch.where(torch.rand(n, generator=g) < 0.5, torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64), lo)
    bits = (hi << 16) | lo
    sp = torch.tensor(_F32_SPECIAL, dtype=torch.int64)
    k = min(n, len(sp))
    bits[:k] = sp[:k]
    if n > len(sp):
        t = min(3, n - len(sp))
        bits[n - t:] = sp[:t]
    return bits.to(torch.int32)                          # wraps to the same 32 bits


@pytest.mark.parametrize('n', _CAST_N)
def test_cast_bf16(n):
    """dclip_cast_bf16 f32 -> bf16 (RNE, NaN kept NaN): tails n % 4 != 0, several grid-stride sweeps at 8 M + 3, the special values;
    source 16-byte aligned, destination only 8-byte aligned (the minimum the entry accepts); the words around the destination
    untouched.  Rule: exact against .to(torch.bfloat16), NaN positions by isnan."""
    src_cpu = _f32_cast_source(n, n).view(torch.float32)
    src = src_cpu.cuda()
    buf = _nan_like((n + 12,), torch.bfloat16)
    dst = buf[4:4 + n]
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 8
    _lib().dclip_cast_bf16(_p(src), _p(dst), n, _st())
    _exact(dst, src_cpu.to(torch.bfloat16).cuda(), 'cast_bf16')
    assert (_bits(buf[:4]) == -1).all() and (_bits(buf[4 + n:]) == -1).all(), 'cast_bf16 wrote outside [0, n)'


@pytest.mark.parametrize('n', _CAST_N)
def test_cast_f16_f32(n):
    """dclip_cast_f16_f32 f16 -> f32 over every kind of f16 (random bit patterns: subnormals, +-inf, NaN, +-0, 65504): tails, sweeps,
    source only 8-byte aligned, destination 16-byte aligned, the words after it untouched.  Rule: exact against .float()."""
    bits = torch.randint(-(1 << 15), 1 << 15, (n,), generator=_gen(n + 1), dtype=torch.int16)
    sp = torch.tensor([0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x0000, -0x8000, 0x7BFF, 0xFBFF - 0x10000, 0x0001, 0x03FF, 0x0400],
                      dtype=torch.int32).to(torch.int16)
    k = min(n, len(sp))
    bits[:k] = sp[:k]
    if n > len(sp):
        bits[-min(3, n - len(sp)):] = sp[:min(3, n - len(sp))]
    src_cpu = bits.view(torch.float16)
    sbuf = torch.zeros(n + 8, dtype=torch.float16, device='cuda')
    src = sbuf[4:4 + n]
    src.copy_(src_cpu.cuda())
    buf = _nan_like((n + 8,), torch.float32)
    dst = buf[:n]
    assert src.data_ptr() % 16 == 8 and dst.data_ptr() % 16 == 0
    _lib().dclip_cast_f16_f32(_p(src), _p(dst), n, _st())
    _exact(dst, src_cpu.float().cuda(), 'cast_f16_f32')
    assert (_bits(buf[n:]) == -1).all(), 'cast_f16_f32 wrote past n'


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. feature_mse
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 12, 1020, 2048 * 1024 * 16 + 4])
@pytest.mark.parametrize('with_ds', [False, True])
@pytest.mark.parametrize('coef', [1.0, 0.3])
def test_feature_mse(n, with_ds, coef):
    """dclip_feature_mse loss += coef mean((s - t)^2), ds += coef 2 (s - t) / n (ds NULL or a non-zero start): tiny n (one partly busy
    wave), and a grid-stride sweep past the 2048-workgroup cap.  Rules: sum bound on the loss (n + 1 terms: the start and the n
    scaled squares) and on ds (2 terms per element), each also within 2e-5 of the max."""
    s, t = _pool(n), _pool(n, 2_000_004)
    c = float(np.float32(coef))                        # the kernel's coefficient is the f32 one
    acc = torch.tensor([0.75], device='cuda')
    ds0 = _pool(n, 1_000_000).clone() * 0.01 if with_ds else None
    ds = ds0.clone() if with_ds else None
    _lib().dclip_feature_mse(_p(s), _p(t), n, coef, _p(acc), _p(ds), _st())
    d = s.double() - t.double()
    sq = (d * d).sum() * c / n
    _sum_bound(acc, 0.75 + sq, n + 1, 0.75 + sq, 'loss')
    if with_ds:
        g = c * 2.0 * d / n
        _sum_bound(ds, ds0.double() + g, 2, ds0.double().abs() + g.abs(), 'ds')


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. layernorm_bwd on the persistent grid
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_case(Mx, D, seed):
    """x rows with their own scale and offset (a row's gradient taken with another row's statistics is then grossly wrong), f32
    mean / rstd of the float64 statistics (eps 1e-5 inside the sqrt), gamma around 1"""
    g = _gen(seed)
    x = _pool(Mx * D, 8).reshape(Mx, D) * (0.5 + 1.5 * torch.rand(Mx, 1, generator=g)).cuda() + (torch.rand(Mx, 1, generator=g) * 2 - 1).cuda()
    x64 = x.double()
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-5)
    gamma = (torch.randn(D, generator=g) * 0.1 + 1).cuda()
    return x, mean, rstd, gamma


def _ln_run_and_check(x, mean, rstd, gamma, dy, ridx):
    """one dclip_layernorm_bwd call (dx_bf16, dgamma, dbeta, colsum all on) checked against F.layer_norm's float64 autograd"""
    Mx, D = x.shape
    M = dy.shape[0]
    rows = ridx.long() if ridx is not None else torch.arange(M, device='cuda')
    acc0 = _pool(Mx * D, 12).reshape(Mx, D).clone()
    acc = acc0.clone()
    dxb = _nan_like((Mx, D), torch.bfloat16)
    dg0, db0, cs0 = _randn((D,), 1), _randn((D,), 2), _randn((D,), 3)
    dg, db, cs = dg0.clone(), db0.clone(), cs0.clone()
    mean32, rstd32 = mean[rows].float(), rstd[rows].float()          # the saved statistics, indexed by the row of dy
    _lib().dclip_layernorm_bwd(_p(dy), D, 1 if dy.dtype == torch.float32 else 0, _p(x), D, _p(ridx), _p(gamma), _p(mean32), _p(rstd32),
                               _p(acc), D, _p(dxb), D, _p(dg), _p(db), _p(cs), M, D, _st())
    xr = x.double()[rows].requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = torch.zeros(D, dtype=torch.float64, device='cuda', requires_grad=True)
    y = F.layer_norm(xr, (D,), gr, br, 1e-5)
    dy64 = dy.double()
    y.backward(dy64)
    # dx: the form of test_kernels_gpu.py; the bf16 copy is the one rounding of the updated f32 row
    _close(acc[rows].double() - acc0[rows].double(), xr.grad, 2e-5, 'dx')
    _exact(dxb[rows], acc[rows].bfloat16(), 'dx bf16 copy')
    if ridx is not None:
        other = torch.ones(Mx, dtype=torch.bool, device='cuda')
        other[rows] = False
        assert torch.equal(_bits(acc[other]), _bits(acc0[other])) and (_bits(dxb[other]) == -1).all(), 'a row outside row_index was written'
    xhat = (xr.detach() - xr.detach().mean(1, keepdim=True)) * rstd[rows][:, None]
    _sum_bound(dg, dg0.double() + gr.grad, M + 1, dg0.double().abs() + (dy64 * xhat).abs().sum(0), 'dgamma')
    _close(dg.double() - dg0.double(), gr.grad, 2e-5, 'dgamma (test_kernels_gpu form)')
    _sum_bound(db, db0.double() + br.grad, M + 1, db0.double().abs() + dy64.abs().sum(0), 'dbeta')
    _close(db.double() - db0.double(), br.grad, 2e-5, 'dbeta (test_kernels_gpu form)')
    upd = acc[rows].double()
    _sum_bound(cs, cs0.double() + upd.sum(0), M + 1, cs0.double().abs() + upd.abs().sum(0), 'colsum')
    _close(cs.double() - cs0.double(), upd.sum(0), 2e-5, 'colsum (test_kernels_gpu form)')


@pytest.mark.parametrize('M,D,dy_dtype', [(2049, 100, torch.float32), (2049, 1024, torch.bfloat16), (4101, 512, torch.float32),
                                          (4101, 1024, torch.bfloat16), (25600, 768, torch.bfloat16), (25600, 768, torch.float32),
                                          (39424, 512, torch.bfloat16)])
def test_layernorm_bwd_persistent_grid(M, D, dy_dtype):
    """dclip_layernorm_bwd past M = 2048, where the 256 x 8 waves of the persistent grid each run the ping-pong row pipeline: 2049 (one
    wave gets a second row), 4101 (waves with 2 rows and with 3), the step's 25600 x 768 and 39424 x 512; bf16 and f32 dy; bf16 dx copy,
    dgamma, dbeta and colsum accumulating into non-zero starts.  Rules: dx within 2e-5 of the max (test_kernels_gpu.py form); the
    bf16 copy exact; dgamma / dbeta / colsum sum bound (n = M + 1)."""
    x, mean, rstd, gamma = _ln_case(M, D, M + D)
    dy = _pool(M * D, 15_000_000).reshape(M, D).to(dy_dtype)
    _ln_run_and_check(x, mean, rstd, gamma, dy, None)


@pytest.mark.parametrize('Mx,M,D', [(39424, 512, 512), (8202, 4101, 768)])
def test_layernorm_bwd_row_index(Mx, M, D):
    """the final-norm form: row_index = the B = 512 picked EOT rows (dclip_pick_index of a caption batch) of a 39424-row x, and 4101
    scattered rows of 8202 (row_index on the persistent grid); rows outside row_index bit-unchanged in dx and in its bf16 copy.
    Rules as for the full form."""
    x, mean, rstd, gamma = _ln_case(Mx, D, Mx + M)
    if M == 512:
        ridx = _pick(_captions(3, 512, 77, 49408), 77, 512, 77)
    else:
        ridx = torch.randperm(Mx, generator=_gen(M))[:M].to(torch.int32).cuda()
    dy = _pool(M * D, 15_000_000).reshape(M, D).to(torch.bfloat16)
    _ln_run_and_check(x, mean, rstd, gamma, dy, ridx)
