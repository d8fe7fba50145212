"""Thin torch-tensor wrappers over the C ABI (device pointers + current stream).  Plumbing only: every
function launches hand-written HIP kernels from libdistillclip_hip.so and raises if the tensors are not on a GPU."""
import torch

from ._lib import lib

ACT = {'none': 0, None: 0, 'quickgelu': 1, 'gelu': 2, 'dgelu': 3, 'mulaux': 4, 'gelu_save': 5, 'quickgelu_save': 6}
OUT_DTYPE = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}      # DCLIP_OUT_*
# 8-bit fixed-point code of the saved gelu' (include/dclip.h: DCLIP_ACT_GELU_SAVE / DCLIP_ACT_MULAUX): value = DG_LO + q * DG_STEP
DG_LO, DG_STEP = -0.13, 1.26 / 255.0


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('distillclip_amd ops need CUDA(HIP) tensors; there is no CPU fallback')


def gemm_nt(a, b, *, bias=None, act=None, aux_in=None, aux_out=None, residual=None, out=None, out_dtype=torch.bfloat16,
            alpha=1.0, row_group=0, rowadd=None, out_rows=None, colsum=None):
    """out[M,N] = epilogue(alpha * a[M,K] @ b[N,K]^T); see include/dclip.h:dclip_gemm_nt.
    act='gelu_save' / 'quickgelu_save' write, act='mulaux' reads the 8-bit derivative (uint8 [M,N]); out_dtype float16 = the teacher's fp16 residual stream
    (residual then float16 too, act none)."""
    _chk(a, b, bias, aux_in, aux_out, residual, out, rowadd)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.dim() == 2 and b.dim() == 2
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, K = a.shape
    N = b.shape[0]
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty((rows, N), dtype=out_dtype, device=a.device)
    assert out.stride(1) == 1
    ldr = residual.stride(0) if residual is not None else 0
    if act in ('gelu_save', 'quickgelu_save') and aux_out is not None:
        assert aux_out.dtype == torch.uint8 and aux_out.stride(0) == out.stride(0)
    if act == 'mulaux':
        assert aux_in.dtype == torch.uint8 and aux_in.stride(0) == out.stride(0)
    if residual is not None:
        assert residual.dtype == (torch.float16 if out.dtype == torch.float16 else torch.float32)
    lib().dclip_gemm_nt(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, float(alpha),
                        _p(bias), ACT[act], _p(aux_in), _p(aux_out), _p(residual), ldr,
                        OUT_DTYPE[out.dtype], row_group, _p(rowadd), _p(colsum), _stream())
    return out


_TN_WS = {}


def _tn_workspace(device):
    # one workspace per (device, stream): two wgrad calls enqueued on different streams must not share partial tiles
    key = (device, _stream())
    ws = _TN_WS.get(key)
    if ws is None:
        ws = _TN_WS[key] = torch.empty(lib().dclip_gemm_tn_workspace_bytes(), dtype=torch.uint8, device=device)
    return ws


def gemm_tn_acc(a, b, dw, splits=4, workspace=True):
    """dw[P,Q] (f32) += a[M,P]^T @ b[M,Q].  workspace=True: large outputs leave as per-split partial tiles + a fixed-order sum
    (no f32 atomics, run-to-run identical); False: f32 atomics."""
    _chk(a, b, dw)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and dw.dtype == torch.float32
    M, P = a.shape
    Q = b.shape[1]
    assert b.shape[0] == M and tuple(dw.shape) == (P, Q) and dw.stride(1) == 1
    ws = _tn_workspace(a.device) if workspace else None
    lib().dclip_gemm_tn_acc(_p(a), a.stride(0), _p(b), b.stride(0), _p(dw), dw.stride(0), M, P, Q, splits, _p(ws),
                            0 if ws is None else ws.numel(), _stream())
    return dw


def colsum_acc(x, db):
    _chk(x, db)
    assert x.dtype == torch.bfloat16 and db.dtype == torch.float32
    lib().dclip_colsum_acc(_p(x), x.stride(0), _p(db), x.shape[0], x.shape[1], _stream())
    return db


def layernorm_fwd(x, gamma, beta, *, row_index=None, out_dtype=torch.bfloat16, eps=1e-5, save_stats=True):
    """x f32, or f16 (the frozen teacher's residual stream: dclip_layernorm_fwd_f16, which can also return f16)"""
    _chk(x, gamma, beta, row_index)
    assert x.dtype in (torch.float32, torch.float16) and x.dim() == 2 and x.stride(1) == 1
    M = row_index.numel() if row_index is not None else x.shape[0]
    D = x.shape[1]
    y = torch.empty((M, D), dtype=out_dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    fn = lib().dclip_layernorm_fwd_f16 if x.dtype == torch.float16 else lib().dclip_layernorm_fwd
    fn(_p(x), x.stride(0), _p(row_index), _p(gamma), _p(beta), _p(y), D, OUT_DTYPE[out_dtype], _p(mean), _p(rstd), M, D, eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dx_acc, *, row_index=None, dx_bf16=None, dgamma=None, dbeta=None, colsum=None):
    _chk(dy, x, gamma, mean, rstd, dx_acc, dx_bf16, dgamma, dbeta)
    M, D = dy.shape
    lib().dclip_layernorm_bwd(_p(dy), dy.stride(0), 1 if dy.dtype == torch.float32 else 0, _p(x), x.stride(0),
                              _p(row_index), _p(gamma), _p(mean), _p(rstd), _p(dx_acc), dx_acc.stride(0), _p(dx_bf16),
                              dx_bf16.stride(0) if dx_bf16 is not None else 0, _p(dgamma), _p(dbeta), _p(colsum), M, D, _stream())


def attn_nt(a, lda, bm, ldb, B, H, N, hd, alpha=1.0, out_dtype=torch.float32):
    Np = (N + 7) // 8 * 8
    c = torch.empty((B, H, N, Np), dtype=out_dtype, device=a.device)
    lib().dclip_attn_nt(_p(a), lda, _p(bm), ldb, _p(c), 1 if out_dtype == torch.float32 else 0, B, H, N, Np, hd, alpha,
                        _stream())
    return c


def _score_dims(a):
    """row-major [B,H,N,Np] or the quad-blocked [B,H,Np/4,N,4] of the register-resident score stage -> (B, H, N, Np, blocked)"""
    if a.dim() == 5:
        B, H, nq, N, four = a.shape
        assert four == 4
        return B, H, N, nq * 4, 1
    B, H, N, Np = a.shape
    return B, H, N, Np, 0


def attn_nn(a, bm, ldb, c, ldc, hd, alpha=1.0):
    B, H, N, Np, blocked = _score_dims(a)
    lib().dclip_attn_nn(_p(a), _p(bm), ldb, _p(c), ldc, B, H, N, Np, hd, alpha, blocked, _stream())


def attn_tn(a, bm, ldb, c, ldc, hd, alpha=1.0):
    B, H, N, Np, blocked = _score_dims(a)
    lib().dclip_attn_tn(_p(a), _p(bm), ldb, _p(c), ldc, B, H, N, Np, hd, alpha, blocked, _stream())


def attn_nn_rows(a, bm, ldb, c, ldc, hd, pick, alpha=1.0, fill_zero=False):
    """attn_nn on the 16-row tile that holds row pick[b] of each sample (include/dclip.h: row-tile forms); pick: int32 [B]"""
    _chk(pick)
    B, H, N, Np, blocked = _score_dims(a)
    lib().dclip_attn_nn_rows(_p(a), _p(bm), ldb, _p(c), ldc, B, H, N, Np, hd, alpha, blocked, _p(pick), 1 if fill_zero else 0, _stream())


def attn_tn_rows(a, bm, ldb, c, ldc, hd, pick, alpha=1.0):
    """attn_tn contracted over the rows of each sample's picked tile only"""
    _chk(pick)
    B, H, N, Np, blocked = _score_dims(a)
    lib().dclip_attn_tn_rows(_p(a), _p(bm), ldb, _p(c), ldc, B, H, N, Np, hd, alpha, blocked, _p(pick), _stream())


def unblock_scores(a):
    """quad-blocked [B,H,Np/4,N,4] -> row-major [B,H,N,Np] (tests / diagnostics)"""
    B, H, nq, N, _ = a.shape
    return a.permute(0, 1, 3, 2, 4).reshape(B, H, N, nq * 4)


def attn_softmax_fwd(s, wl=None, ww=None, causal=False, save_p=False):
    B, H, N, Np = s.shape
    r = torch.empty((B, H, N, Np), dtype=torch.bfloat16, device=s.device)
    p = torch.empty_like(r) if save_p else None
    lib().dclip_attn_softmax_fwd(_p(s), _p(wl), _p(ww), _p(p), _p(r), B, H, N, Np, 1 if causal else 0, _stream())
    return p, r


def attn_softmax_bwd(dr, p, s, wl=None, ww=None, dwl=None, dww=None):
    B, H, N, Np = dr.shape
    ds = torch.empty_like(dr)
    lib().dclip_attn_softmax_bwd(_p(dr), _p(p), _p(s), 1 if (s is not None and s.dtype == torch.bfloat16) else 0, _p(wl), _p(ww), _p(ds),
                                 _p(dwl), _p(dww), B, H, N, Np, _stream())
    return ds


LOSS_SLOTS = {'out_l1': 0, 'out_cos': 1, 'out_kl': 2, 'out_ce': 3, 'cos_diff': 4, 'hard_label': 5, 'soft_label': 6,
              'logits_mse': 7}


def distill_loss(s_img, t_img, s_txt=None, t_txt=None, *, weights, temperature=None, row0=None, rows=None, gathered_stats=None,
                 stats_only=False):
    """Fused loss fwd+bwd.  weights: {term: scale*percent}.  -> (scalars[16] device tensor, d_s_img, d_s_txt).
    row0 / rows: evaluate only the row block [row0, row0 + rows) of the (gathered) batch against all columns — gradients
    [rows, E] of the owned samples, scalars = this block's share (sum over the blocks = the whole-batch values).
    hard_label / soft_label in row-block mode: first `stats_only=True` -> [6, rows] statistics of the owned rows (natural-log
    log-sum-exps of S, S / tau, T / tau over each row, then over each column); gather all blocks into [6, B] and pass them as
    `gathered_stats` to the second call.  `stats_only` needs both towers and a cross-modal term (ValueError otherwise: no kernel would
    write the statistics); a statistic of a disabled term is -inf."""
    import ctypes
    _chk(s_img, t_img, s_txt, t_txt)
    B, E = s_img.shape
    two = s_txt is not None
    cfg = [0.0] * 10
    for k, w in weights.items():
        cfg[LOSS_SLOTS[k]] = float(w)
    cfg[8] = float(temperature or 0.0)
    cfg[9] = 1.0 if two else 0.0
    cfg_arr = (ctypes.c_float * 10)(*cfg)
    ws_bytes = lib().dclip_distill_loss_workspace(B, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s_img.device)
    out = torch.empty(16, dtype=torch.float32, device=s_img.device)
    nrow = B if rows is None else int(rows)
    d_i = torch.empty((nrow, E), dtype=torch.float32, device=s_img.device)
    d_t = torch.empty((nrow, E), dtype=torch.float32, device=s_img.device) if two else None
    if rows is None:
        lib().dclip_distill_loss(_p(s_img), _p(t_img), _p(s_txt), _p(t_txt), B, E, ctypes.cast(cfg_arr, ctypes.c_void_p),
                                 _p(out), _p(d_i), _p(d_t), _p(ws), ws_bytes, _stream())
    else:
        stats = torch.empty((6, nrow), dtype=torch.float32, device=s_img.device) if stats_only else None
        if gathered_stats is not None:
            assert gathered_stats.shape == (6, B) and gathered_stats.dtype == torch.float32 and gathered_stats.is_contiguous()
        lib().dclip_distill_loss_rows(_p(s_img), _p(t_img), _p(s_txt), _p(t_txt), B, E, int(row0), nrow,
                                      ctypes.cast(cfg_arr, ctypes.c_void_p), _p(out), _p(d_i), _p(d_t), _p(gathered_stats),
                                      _p(stats), _p(ws), ws_bytes, _stream())
        if stats_only:
            return stats
    return out, d_i, d_t


def interactive_loss(s_img, t_img, s_txt, t_txt, temperature, weight=1.0):
    """Interactive contrastive distillation fwd+bwd (include/dclip.h: dclip_interactive_loss): student image rows against teacher text
    rows and student text rows against teacher image rows.  f32 [B, E] contiguous device tensors.
    -> (out[4] = weight * icl, icl, L_i2t, L_t2i ; d_s_img, d_s_txt = weight * d icl / d student rows)"""
    _chk(s_img, t_img, s_txt, t_txt)
    for t in (s_img, t_img, s_txt, t_txt):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != s_img.shape or not t.is_contiguous():
            raise ValueError(f'interactive_loss: need four contiguous f32 [B, E] tensors of one shape, got {tuple(t.shape)} {t.dtype}')
    B, E = s_img.shape
    ws_bytes = lib().dclip_interactive_loss_workspace(B, E)
    if ws_bytes == 0:
        raise ValueError(f'interactive_loss: need 1 <= B <= 4096, E % 16 == 0, 16 <= E <= 1024, got B={B} E={E}')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s_img.device)
    out = torch.empty(4, dtype=torch.float32, device=s_img.device)
    d_i, d_t = torch.empty_like(s_img), torch.empty_like(s_txt)
    lib().dclip_interactive_loss(_p(s_img), _p(t_img), _p(s_txt), _p(t_txt), B, E, float(temperature), float(weight), _p(out), _p(d_i),
                                 _p(d_t), _p(ws), ws_bytes, _stream())
    return out, d_i, d_t


def relation_kl(s, t, temperature, weight=1.0):
    """Intra-modal relational KL distillation fwd+bwd of one tower (include/dclip.h: dclip_relation_kl): the KL between the teacher's and
    the student's softmax over the same-modality in-batch similarities.  f32 [B, E] contiguous device tensors.
    -> (out[4] = weight * intra_kl, intra_kl, mean_i KL_i, +0 ; d_s = weight * d intra_kl / d student rows)"""
    _chk(s, t)
    for x in (s, t):
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape != s.shape or not x.is_contiguous():
            raise ValueError(f'relation_kl: need two contiguous f32 [B, E] tensors of one shape, got {tuple(x.shape)} {x.dtype}')
    B, E = s.shape
    ws_bytes = lib().dclip_relation_kl_workspace(B, E)
    if ws_bytes == 0:
        raise ValueError(f'relation_kl: need 1 <= B <= 4096, E % 16 == 0, 16 <= E <= 1024, got B={B} E={E}')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
    out = torch.empty(4, dtype=torch.float32, device=s.device)
    d_s = torch.empty_like(s)
    lib().dclip_relation_kl(_p(s), _p(t), B, E, float(temperature), float(weight), _p(out), _p(d_s), _p(ws), ws_bytes, _stream())
    return out, d_s


def attn_fused_fwd(qkv, B, N, H, hd, causal=False):
    """ctx = softmax(q k^T / sqrt(hd) (+ causal mask)) v for plain multi-head attention; qkv: [B*N, 3*H*hd] bf16."""
    _chk(qkv)
    D = H * hd
    ctx = torch.empty((B * N, D), dtype=torch.bfloat16, device=qkv.device)
    lib().dclip_attn_fused_fwd(_p(qkv), qkv.stride(0), _p(ctx), D, B, H, N, hd, hd ** -0.5, 1 if causal else 0, _stream())
    return ctx


def attn_fused_fwd_rows(qkv, ctx, B, N, H, hd, pick, causal=False):
    """attn_fused_fwd into the rows of each sample's picked tile of `ctx` [B*N, H*hd] bf16; the other rows are left as they are"""
    _chk(qkv, ctx, pick)
    lib().dclip_attn_fused_fwd_rows(_p(qkv), qkv.stride(0), _p(ctx), ctx.stride(0), B, H, N, hd, hd ** -0.5, 1 if causal else 0, _p(pick),
                                    _stream())
    return ctx


def attn_stream_fwd(qkv, B, N, H, hd):
    """attn_fused_fwd for sequences of any length (the frozen ViT-B/16 / ViT-L/14 teachers), non-causal, hd = 64: keys streamed in chunks
    with a running maximum and sum (include/dclip.h: dclip_attn_stream_fwd); qkv: [B*N, 3*H*hd] bf16."""
    _chk(qkv)
    D = H * hd
    ctx = torch.empty((B * N, D), dtype=torch.bfloat16, device=qkv.device)
    lib().dclip_attn_stream_fwd(_p(qkv), qkv.stride(0), _p(ctx), D, B, H, N, hd, hd ** -0.5, _stream())
    return ctx


def im2row_ld(image, patch, ldk=None, cls_rows=1):
    """image f32 [B, C, R, R] -> bf16 patch rows [B * ((R // patch)^2 + cls_rows), ldk], ldk >= C * patch^2 (default: rounded up to 64),
    pad columns zero, any even patch (include/dclip.h: dclip_im2row_ld)"""
    _chk(image)
    assert image.dtype == torch.float32 and image.dim() == 4 and image.is_contiguous() and image.shape[2] == image.shape[3]
    B, C, R, _ = image.shape
    K = C * patch * patch
    ldk = (K + 63) // 64 * 64 if ldk is None else int(ldk)
    g = R // patch
    rows = torch.empty((B * (g * g + cls_rows), ldk), dtype=torch.bfloat16, device=image.device)
    lib().dclip_im2row_ld(_p(image), _p(rows), ldk, B, C, R, patch, cls_rows, _stream())
    return rows


def embed_scatter_add(ids, dx, dtable):
    _chk(ids, dx, dtable)
    rows, D = dx.shape
    lib().dclip_embed_scatter_add(_p(ids), _p(dx), 1 if dx.dtype == torch.float32 else 0, _p(dtable), rows, D, dtable.shape[0],
                                  _stream())
    return dtable


def feature_mse(s, t, coef=1.0):
    """-> (mean((s - t)^2) * coef as a 0-d tensor, d/ds of it)"""
    _chk(s, t)
    assert s.dtype == torch.float32 and t.dtype == torch.float32 and s.numel() == t.numel() and s.numel() % 4 == 0
    val = torch.zeros(1, dtype=torch.float32, device=s.device)
    ds = torch.zeros_like(s)
    lib().dclip_feature_mse(_p(s), _p(t), s.numel(), float(coef), _p(val), _p(ds), _stream())
    return val[0], ds


def attn_mix_fwd(qkv, B, N, H, hd, wl, ww, scale):
    """register-resident head-mixed attention scores (include/dclip.h: dclip_attn_mix_fwd)
    -> (R bf16, quad-blocked [B,H,Np/4,N,4] (unblock_scores() gives [B,H,N,Np]), lse f32 [B,H,N])"""
    _chk(qkv, wl, ww)
    Np = (N + 7) // 8 * 8
    r = torch.full((B, H, Np // 4, N, 4), float('nan'), dtype=torch.bfloat16, device=qkv.device)    # the kernel writes every element
    stats = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    lib().dclip_attn_mix_fwd(_p(qkv), qkv.stride(0), _p(wl), _p(ww), _p(r), _p(stats), B, H, N, Np, hd, scale, _stream())
    return r, stats


def attn_mix_bwd(qkv, d_ctx, B, N, H, hd, wl, ww, stats, scale, dwl, dww):
    """-> dS bf16, quad-blocked [B,H,Np/4,N,4] (gradient of the scaled pre-mix scores); dwl / dww += (include/dclip.h: dclip_attn_mix_bwd)"""
    _chk(qkv, d_ctx, wl, ww, stats, dwl, dww)
    Np = (N + 7) // 8 * 8
    ds = torch.full((B, H, Np // 4, N, 4), float('nan'), dtype=torch.bfloat16, device=qkv.device)  # the kernel writes every element
    ws = torch.empty(lib().dclip_attn_mix_bwd_workspace_bytes(B, H, N), dtype=torch.uint8, device=qkv.device)
    lib().dclip_attn_mix_bwd(_p(qkv), qkv.stride(0), _p(d_ctx), d_ctx.stride(0), _p(wl), _p(ww), _p(stats), _p(ds), _p(dwl), _p(dww),
                             _p(ws), ws.numel(), B, H, N, Np, hd, scale, _stream())
    return ds


def attn_mix_fwd_rows(qkv, r, stats, wl, ww, scale, pick):
    """attn_mix_fwd into the rows of each sample's picked tile of `r` (quad-blocked [B,H,Np/4,N,4]) and `stats` [B,H,N]"""
    _chk(qkv, r, stats, wl, ww, pick)
    B, H, N, Np, _ = _score_dims(r)
    lib().dclip_attn_mix_fwd_rows(_p(qkv), qkv.stride(0), _p(wl), _p(ww), _p(r), _p(stats), B, H, N, Np, qkv.shape[1] // (3 * H), scale,
                                  _p(pick), _stream())


def attn_mix_bwd_rows(qkv, d_ctx, ds, wl, ww, stats, scale, dwl, dww, pick, ws=None):
    """attn_mix_bwd on each sample's picked tile: dS into those rows of `ds` (quad-blocked), dwl / dww +=; `ws`: the workspace to use
    (uint8, dclip_attn_mix_bwd_workspace_bytes), by default a fresh one"""
    _chk(qkv, d_ctx, ds, wl, ww, stats, dwl, dww, pick)
    B, H, N, Np, _ = _score_dims(ds)
    if ws is None:
        ws = torch.empty(lib().dclip_attn_mix_bwd_workspace_bytes(B, H, N), dtype=torch.uint8, device=qkv.device)
    lib().dclip_attn_mix_bwd_rows(_p(qkv), qkv.stride(0), _p(d_ctx), d_ctx.stride(0), _p(wl), _p(ww), _p(stats), _p(ds), _p(dwl), _p(dww),
                                  _p(ws), ws.numel(), B, H, N, Np, qkv.shape[1] // (3 * H), scale, _p(pick), _stream())


def cast_transpose_multi(ws, want_b=True, want_t=True):
    """[W f32 [R, C]] -> ([bf16 [R, C]] or None, [bf16 [C, R]] or None) in ONE launch (include/dclip.h: dclip_cast_transpose_bf16_multi)"""
    import ctypes
    _chk(*ws)
    n = len(ws)
    wb = [torch.empty_like(w, dtype=torch.bfloat16) for w in ws] if want_b else [None] * n
    wt = [torch.empty((w.shape[1], w.shape[0]), dtype=torch.bfloat16, device=w.device) for w in ws] if want_t else [None] * n
    arr = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    R = (ctypes.c_int64 * n)(*[w.shape[0] for w in ws])
    C = (ctypes.c_int64 * n)(*[w.shape[1] for w in ws])
    lib().dclip_cast_transpose_bf16_multi(arr(ws), arr(wb), arr(wt), R, C, n, _stream())
    return (wb if want_b else None), (wt if want_t else None)


SUMSQ_PARTIALS = 1024      # DCLIP_SUMSQ_PARTIALS (include/dclip.h): partial sums one dclip_sumsq_multi launch writes
ADAMW_MAX_RANGES = 24      # DCLIP_ADAMW_MAX_RANGES


def _range_arrays(items, width):
    """what a multi-range entry takes for `items`, a list of `width`-tuples of equally long 1-D tensors (all checked to be on a GPU):
    -> ([one pointer array per position], the array of their lengths, the number of ranges)"""
    import ctypes
    for it in items:
        _chk(*it)
    n = len(items)
    ptrs = [(ctypes.c_void_p * max(n, 1))(*[t[k].data_ptr() for t in items]) for k in range(width)]
    return ptrs, (ctypes.c_int64 * max(n, 1))(*[t[0].numel() for t in items]), n


def sumsq_multi(gs, partials, stream=None):
    """partials[:SUMSQ_PARTIALS] <- partial sums of g^2 over at most 24 read-only f32 ranges `gs` in ONE launch, the rest of `partials` <- 0
    (include/dclip.h: dclip_sumsq_multi); dclip_clip_coef adds them up"""
    _chk(partials)
    (ptrs,), lens, n = _range_arrays([(g,) for g in gs], 1)
    lib().dclip_sumsq_multi(ptrs, lens, n, _p(partials), partials.numel(), _stream() if stream is None else stream)
    return partials


def clip_coef(partials, max_norm, out, extra_sumsq=None, stream=None):
    """out[0] <- sqrt(sum(partials) [+ extra_sumsq[0]]), out[1] <- min(1, max_norm / (out[0] + 1e-6)) (include/dclip.h: dclip_clip_coef)"""
    _chk(partials, extra_sumsq, out)
    lib().dclip_clip_coef(_p(partials), partials.numel(), _p(extra_sumsq), float(max_norm), _p(out), _stream() if stream is None else stream)
    return out


def adamw_multi_scaled(items, lr, betas, eps, weight_decay, step, zero_grad=False, gscale=None, stream=None):
    """AdamW on at most 24 ranges [(p, g, m, v)] of equally long 1-D f32 tensors in ONE launch, on g * gscale[0] (gscale: a device tensor,
    None = unscaled; include/dclip.h: dclip_adamw_multi_scaled)"""
    ptrs, lens, n = _range_arrays(items, 4)
    _chk(gscale)
    lib().dclip_adamw_multi_scaled(*ptrs, lens, n, lr, betas[0], betas[1], eps, weight_decay, step,
                                   1 if zero_grad else 0, _p(gscale), _stream() if stream is None else stream)


AMP_RECORD_FLOATS = 8      # DCLIP_AMP_RECORD_FLOATS
AMP_MULT, AMP_SKIP, AMP_BC1, AMP_BC2_SQRT, AMP_NORM, AMP_COEF = range(6)      # DCLIP_AMP_*


def amp_prepare(record, skipped, betas, step, found_inf=None, grad_scale=None, partials=None, max_norm=0.0, extra_sumsq=None, stream=None):
    """record (8 f32) <- the control record of a step under a loss scaler, skipped (1 int64) += (found_inf != 0): multiplier coef / grad_scale,
    skip flag, the bias corrections of step - skipped, and with `partials` (of sumsq_multi) the unscaled norm and its clipping coefficient
    (include/dclip.h: dclip_amp_prepare).  found_inf, grad_scale: 1-element f32 device tensors or None."""
    _chk(record, skipped, found_inf, grad_scale, partials, extra_sumsq)
    for t in (found_inf, grad_scale):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise ValueError('amp_prepare: found_inf and grad_scale are 1-element f32 tensors')
    if record.dtype != torch.float32 or record.numel() < AMP_RECORD_FLOATS or skipped.dtype != torch.int64:
        raise ValueError('amp_prepare: record is %d f32, skipped one int64' % AMP_RECORD_FLOATS)
    lib().dclip_amp_prepare(_p(found_inf), _p(grad_scale), _p(partials), 0 if partials is None else partials.numel(), _p(extra_sumsq), float(max_norm),
                            betas[0], betas[1], step, _p(skipped), _p(record), _stream() if stream is None else stream)
    return record


def adamw_multi_amp(items, lr, betas, eps, weight_decay, zero_grad, record, stream=None):
    """adamw_multi_scaled with multiplier, skip flag and bias corrections read from `record` of amp_prepare (include/dclip.h: dclip_adamw_multi_amp)"""
    ptrs, lens, n = _range_arrays(items, 4)
    _chk(record)
    lib().dclip_adamw_multi_amp(*ptrs, lens, n, lr, betas[0], betas[1], eps, weight_decay, 1 if zero_grad else 0,
                                _p(record), _stream() if stream is None else stream)


def adamw_multi_ema(items, lr, betas, eps, weight_decay, step, zero_grad, ema_weight, gscale=None, record=None, stream=None):
    """AdamW on at most 24 ranges [(p, g, m, v, e)] in ONE launch, e <- e + ema_weight * (p' - e) on the parameters it writes
    (include/dclip.h: dclip_adamw_multi_ema).  gscale: adamw_multi_scaled's multiplier; record: adamw_multi_amp's record (`step` is then
    not read); not both.  ema_weight: float(numpy.float32(1.0 - decay)), the subtraction in double."""
    ptrs, lens, n = _range_arrays(items, 5)
    _chk(gscale, record)
    lib().dclip_adamw_multi_ema(*ptrs, lens, n, lr, betas[0], betas[1], eps, weight_decay, step,
                                1 if zero_grad else 0, ema_weight, _p(gscale), _p(record), _stream() if stream is None else stream)


ADAMW_TABLE_TILE = 8192    # DCLIP_ADAMW_TABLE_TILE: every range of a table starts a new tile of this many elements


def adamw_table_image(ranges, total, out=None):
    """The HOST image of the device table of adamw_table (include/dclip.h: dclip_adamw_table_fill), validated there.
    ranges: [(begin, length, lr_scale, weight_decay)] in elements, ascending.  total: the element count of the buffers the ranges lie in.
    out: a CPU uint8 tensor to fill (e.g. pinned), at least adamw_table_bytes long; default a new one.  -> (image, tiles)"""
    import ctypes
    n = len(ranges)
    need = lib().dclip_adamw_table_bytes(n)
    if out is None:
        out = torch.zeros(max(need, 8), dtype=torch.uint8)
    if out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError('adamw_table_image: out is a contiguous CPU uint8 tensor')
    col = lambda k, ct: (ct * max(n, 1))(*[r[k] for r in ranges])
    tiles = ctypes.c_int64(0)
    lib().dclip_adamw_table_fill(col(0, ctypes.c_int64), col(1, ctypes.c_int64), col(2, ctypes.c_float), col(3, ctypes.c_float), n, total,
                                 out.data_ptr(), out.numel(), ctypes.byref(tiles))
    return out, tiles.value


def _table_operands(what, p, g, m, v, e, table, count):
    """the operand checks adamw_table and lamb_table share"""
    if table.dtype != torch.uint8 or table.numel() < lib().dclip_adamw_table_bytes(count):
        raise ValueError('%s: table is the uint8 device copy of an image of %d ranges' % (what, count))
    if any(t.numel() != p.numel() or t.dtype != torch.float32 for t in (p, g, m, v) + (() if e is None else (e,))):
        raise ValueError('%s: p, g, m, v (and e) are f32 buffers of one length, the `total` the table was filled for' % what)


def adamw_table(p, g, m, v, e, table, count, tiles, lr, betas, eps, step, zero_grad=False, ema_weight=0.0, gscale=None, record=None, stream=None):
    """AdamW on `count` ranges of the flat f32 buffers p, g, m, v (and e, or None) in ONE launch, each range with its own lr_scale and
    weight_decay from the device `table` (the uploaded image of adamw_table_image, with its `tiles`); gscale / record as in
    adamw_multi_ema (include/dclip.h: dclip_adamw_table)"""
    _chk(p, g, m, v, e, table, gscale, record)
    _table_operands('adamw_table', p, g, m, v, e, table, count)
    lib().dclip_adamw_table(_p(p), _p(g), _p(m), _p(v), _p(e), _p(table), count, tiles, lr, betas[0], betas[1], eps, step, 1 if zero_grad else 0,
                            ema_weight, _p(gscale), _p(record), _stream() if stream is None else stream)


def lamb_buffers(count, tiles, device):
    """-> (workspace, stats) of lamb_table for a table of `count` ranges and `tiles` tiles: the tile records (uint8,
    dclip_lamb_workspace_bytes) and the f32 [count, 4] rows {|p|, |u|, r, 0}, zero until the first step"""
    return (torch.empty(max(lib().dclip_lamb_workspace_bytes(count, tiles), 16), dtype=torch.uint8, device=device),
            torch.zeros(count, 4, dtype=torch.float32, device=device))


def lamb_table(p, g, m, v, e, table, count, tiles, lr, betas, eps, step, workspace, stats, zero_grad=False, ema_weight=0.0, gscale=None, record=None,
               trust_clip=None, always_adapt=False, stream=None):
    """adamw_table's operands, stepped with a trust ratio per range (include/dclip.h: dclip_lamb_table): three launches.  workspace, stats:
    lamb_buffers(count, tiles); stats holds {|p|, |u|, r, 0} per range afterwards.  trust_clip: None = no clip."""
    _chk(p, g, m, v, e, table, gscale, record, workspace, stats)
    _table_operands('lamb_table', p, g, m, v, e, table, count)
    if workspace.dtype != torch.uint8 or stats.dtype != torch.float32 or stats.numel() < 4 * count:
        raise ValueError('lamb_table: workspace is uint8, stats f32 [%d, 4] (lamb_buffers)' % count)
    lib().dclip_lamb_table(_p(p), _p(g), _p(m), _p(v), _p(e), _p(table), count, tiles, lr, betas[0], betas[1], eps, step, 1 if zero_grad else 0,
                           ema_weight, _p(gscale), _p(record), -1.0 if trust_clip is None else float(trust_clip), 1 if always_adapt else 0,
                           _p(workspace), workspace.numel(), _p(stats), _stream() if stream is None else stream)


def swap_multi(pairs, stream=None):
    """a <-> b, bit for bit, for at most 24 pairs [(a, b)] of equally long 1-D f32 tensors in ONE launch (include/dclip.h: dclip_swap_multi)"""
    for a, b in pairs:
        _chk(a, b)
        if a.numel() != b.numel():
            raise ValueError('swap_multi: the two sides of a pair have %d and %d elements' % (a.numel(), b.numel()))
    ptrs, lens, n = _range_arrays(pairs, 2)
    lib().dclip_swap_multi(*ptrs, lens, n, _stream() if stream is None else stream)


def clipscore(img, cand, refs=None, ref_offsets=None, *, K=1, w=2.5):
    """CLIP-S / RefCLIP-S of K candidates per image in ONE launch (include/dclip.h: dclip_clipscore).  img f32 [B, E], cand f32 [B * K, E]
    (row b * K + k belongs to image b), refs f32 [R, E] with ref_offsets int32 [B + 1] on the device (CSR into refs), or neither: raw,
    un-normalised embeddings; rows may be strided.  -> (clip_s, ref_s, refclip_s), f32 [B * K] each; the last two None without references."""
    _chk(img, cand, refs, ref_offsets)
    if (refs is None) != (ref_offsets is None):
        raise ValueError('clipscore: refs and ref_offsets come together')
    for name, t in (('img', img), ('cand', cand), ('refs', refs)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1):
            raise ValueError(f'clipscore: {name} must be an f32 [rows, E] matrix with unit column stride')
    B, E = img.shape
    K = int(K)
    if K < 1 or cand.shape != (B * K, E) or (refs is not None and refs.shape[1] != E):
        raise ValueError(f'clipscore: img {tuple(img.shape)} and K={K} need cand [{B * K}, {E}] and refs [R, {E}], got {tuple(cand.shape)}'
                         + ('' if refs is None else f' and {tuple(refs.shape)}'))
    R = 0
    if refs is not None:
        if ref_offsets.dtype != torch.int32 or ref_offsets.dim() != 1 or ref_offsets.numel() != B + 1 or not ref_offsets.is_contiguous():
            raise ValueError(f'clipscore: ref_offsets must be a contiguous int32 [{B + 1}] tensor')
        R = refs.shape[0]
        if R == 0:
            refs = img.new_zeros((1, E))           # an empty tensor has no address to hand over; with R = 0 no row of this one is read
    clip_s = torch.empty(B * K, dtype=torch.float32, device=img.device)
    ref_s = torch.empty_like(clip_s) if refs is not None else None
    refclip_s = torch.empty_like(clip_s) if refs is not None else None
    lib().dclip_clipscore(_p(img), img.stride(0), _p(cand), cand.stride(0), _p(refs), 0 if refs is None else refs.stride(0),
                          _p(ref_offsets), B, K, R, E, float(w), _p(clip_s), _p(ref_s), _p(refclip_s), _stream())
    return clip_s, ref_s, refclip_s
