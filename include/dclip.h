/*
 * dclip.h — C ABI of libdistillclip_hip.so (MI355X / gfx950).
 *
 * The reference (ForJadeForest/DistillCLIP) is 100 % Python on top of PyTorch ATen; it has no FFI of its own.
 * The boundary this library replaces is therefore the implicit ATen kernel sequence behind the reference's
 * nn.Module calls.  Each entry point cites the reference call site (file:line under the reference root) whose
 * arithmetic it implements.  All pointers are raw device pointers; `stream` is a hipStream_t passed as void*.
 * No synchronisation inside any entry point, no allocation, no global mutable state on the compute path: the process-global state is
 * the opt-in profiling hooks (dclip_trace_*: launch trace, GEMM stamps / clock stamps; the wgrad fallback counter) and a handful of
 * tuning knobs read from DCLIP_* environment variables, latched once on first use and constant
 * afterwards.  The stream half of this paragraph is tested for every entry that takes a stream: launched on `stream`
 * and nowhere else, no host wait, HOST arrays consumed before the call returns, two calls in flight sharing nothing
 * (tests/stream_cases.py, tests/test_stream_contract_gpu.py; a new stream-taking prototype needs a case there).  Every function returns
 * 0 on success, DCLIP_EINVAL (-1) for a bad argument, DCLIP_ELAUNCH (-2) for a HIP launch failure, and
 * dclip_last_error_string() (thread-local) explains the last failure.
 *
 * dtypes: "bf16" = bfloat16 storage (MFMA operands), "f32" = float, "f16" = IEEE half (the frozen teacher's residual stream, the
 * 16-bit type the reference's `precision: 16` autocast keeps it in).  Row-major everywhere.
 *
 * Load order: the library links the HIP runtime (libamdhip64) the usual way.  A process that also loads PyTorch-ROCm must import torch
 * BEFORE this library is mapped, so that both resolve to the one HIP runtime torch ships (two runtimes in one process do not see each
 * other's device state: "no ROCm-capable device is detected").  dclip_runtime_check() reports that condition in words.
 */
#ifndef DCLIP_H
#define DCLIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DCLIP_OK 0
#define DCLIP_EINVAL (-1)
#define DCLIP_ELAUNCH (-2)

int dclip_version(void);                    /* ABI version, bumped on any signature change */
/* 0 when the HIP runtime this library is bound to sees a device; DCLIP_ELAUNCH otherwise, with dclip_last_error_string() naming the
 * likely cause (a second HIP runtime mapped before this one: see "Load order" above) */
int dclip_runtime_check(void);
const char* dclip_arch(void);               /* "gfx950" */
const char* dclip_last_error_string(void);  /* thread-local */

/* activation codes for dclip_gemm_nt */
#define DCLIP_ACT_NONE 0
#define DCLIP_ACT_QUICKGELU 1 /* reference model/component/_common.py:23-25 */
#define DCLIP_ACT_GELU 2      /* exact erf GELU: timm Mlp act, reference weight_share_model.py:177 */
#define DCLIP_ACT_DGELU 3     /* multiply by gelu'(aux_in): backward of DCLIP_ACT_GELU from the saved pre-activation */
#define DCLIP_ACT_MULAUX 4    /* multiply by the 8-bit gelu' in aux_in: backward of DCLIP_ACT_GELU_SAVE */
#define DCLIP_ACT_GELU_SAVE 5 /* DCLIP_ACT_GELU whose aux_out receives gelu'(pre-activation) as 8-bit fixed point (below) */
#define DCLIP_ACT_QUICKGELU_SAVE 6 /* DCLIP_ACT_QUICKGELU with its derivative saved the same way: a CLIP tower that trains (plain
                                      ImageEncoder / TextEncoder as student, reference image_encoder.py:23-25, text_encoder.py:45-47) */
/* output dtype codes of dclip_gemm_nt / dclip_embed_gather / dclip_layernorm_fwd_f16 */
#define DCLIP_OUT_BF16 0
#define DCLIP_OUT_F32 1
#define DCLIP_OUT_F16 2

/*
 * C[M,N] = epilogue(alpha * A[M,K] · B[N,K]^T)        (nn.Linear / F.linear / x @ proj / conv-as-GEMM)
 *   reference: _common.py:59,90,104-108,213 ; text_encoder.py:72 ; weight_share_model.py:90,132,177,364
 *   A, B bf16 (lda, ldb in elements; K % 64 == 0; 16-byte aligned rows).
 *   epilogue, in order: + bias[N] (f32, may be NULL) ; if aux_out: store pre-activation as bf16 [M,N] (ld = ldc) ;
 *   activation `act` (DCLIP_ACT_DGELU multiplies by gelu'(aux_in[M,N] bf16, ld = ldc); DCLIP_ACT_GELU_SAVE stores
 *   gelu'(pre-activation) in aux_out instead — ONE BYTE per element, uint8 [M,N] with ld = ldc bytes: code q = rint((g' + 0.13) * 255 / 1.26),
 *   value -0.13 + q * 1.26 / 255 (the derivative of the exact GELU lies in [-0.129, 1.129]; |error| <= 2.5e-3) — which
 *   DCLIP_ACT_MULAUX multiplies by: the training towers use that pair, the derivative being a few extra instructions in the
 *   forward epilogue and a single multiply in the backward one; DCLIP_ACT_QUICKGELU_SAVE is the same pair for QuickGELU, whose
 *   derivative s + 1.702 x s (1 - s), s = sigmoid(1.702 x), lies in [-0.1, 1.1]) ;
 *   + residual[M,N] (ld = ldr, may be NULL; f32 with bf16 / f32 output — may alias C when the output is f32 —, f16 with f16 output — may
 *   alias C) ; store C as bf16 / f32 / f16 (out_dtype = DCLIP_OUT_*; f16 needs act = DCLIP_ACT_NONE: the frozen teacher's in-place
 *   residual stream, reference _common.py:124-125 under `precision: 16`, config/final_config/l_clip.yaml:64).
 *   row_group > 0 adds `rowadd` (f32 [row_group, N]) row (r % row_group) to GEMM row r: the positional-embedding
 *   add of the token embedders (reference _common.py:196-202, text_encoder.py:65-66, weight_share_model.py:344-349,
 *   :487-489); for images the caller folds class token and conv bias into the table (see dclip_token_table).
 *   colsum_acc (f32 [N], may be NULL) += column sums of the stored values (bias gradient of the producing linear).
 */
int dclip_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                  int64_t M, int64_t N, int64_t K, float alpha, const float* bias, int act,
                  const void* aux_in, void* aux_out, const void* residual, int64_t ldr, int out_dtype,
                  int64_t row_group, const float* rowadd, float* colsum_acc, void* stream);

/*
 * dW[P,Q] (f32, ld = ldo) += sum_m A[m,P] * B[m,Q]         (weight gradient of nn.Linear: dY^T · X)
 *   autograd of the reference linears listed above (student only: weight_share_model.py:90,132,177,364).
 *   A bf16 [M,P] (lda), B bf16 [M,Q] (ldb).  P % 8 == 0, Q % 8 == 0, lda % 8 == 0, ldb % 8 == 0 (16-byte operand chunks; P, Q = 8 mod 16
 *   are exact on every kernel: tests/test_gemm_exact_gpu.py).  Accumulates with f32 atomics
 *   (weight-shared layers add R uses per step, weight_share_model.py:199-218); `splits` >= 1 partitions M.
 */
/* workspace (nullable; dclip_gemm_tn_workspace_bytes() bytes, 16-byte aligned): with it the 256 x 256 wgrad pipeline writes each
 * split's partial tile with plain stores and a second launch adds the splits to dW in a fixed order (no f32 atomics: faster,
 * and run-to-run identical); without it, or for outputs on the small-tile kernels, f32 atomics as before. */
size_t dclip_gemm_tn_workspace_bytes(void);
/* diagnostic (process-global counter): how many 256 x 256 wgrad launches so far had to fall back from the partial-tile path (run-to-run
 * identical) to f32 atomics because no / too small a workspace was passed */
int64_t dclip_gemm_tn_atomic_fallbacks(void);
int dclip_gemm_tn_acc(const void* A, int64_t lda, const void* B, int64_t ldb, float* dW, int64_t ldo,
                      int64_t M, int64_t P, int64_t Q, int splits, void* workspace, size_t ws_bytes, void* stream);

/* db[N] (f32) += column sums of X[M,N] (bf16, ld) — bias gradient of nn.Linear. */
int dclip_colsum_acc(const void* X, int64_t ld, float* db, int64_t M, int64_t N, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * LayerNorm (fp32 statistics, eps inside the sqrt).
 *   reference: model/component/_common.py:14-20 (call sites :123,:125,:208,:210 ; text_encoder.py:69) and nn.LayerNorm in
 *   weight_share_model.py:181,183,363,503.
 * fwd: y[r] = LN(x[row_index ? row_index[r] : r]) * gamma + beta ; y is bf16 (out_f32=0) or f32 ; mean/rstd (f32 [M],
 *      nullable) are saved for backward.  D % 4 == 0, D <= 1024.
 * bwd: dx_acc[src(r)] += LN'(dy[r]) (f32, in place: the residual-stream gradient) ; optional bf16 copy of the updated
 *      rows in dx_bf16 ; dgamma / dbeta (f32 [D], nullable) += batch sums ; colsum_acc (f32 [D], nullable) += column sums
 *      of the updated dx_acc rows (the bias gradient of the linear that fed this residual stream).
 */
int dclip_layernorm_fwd(const float* x, int64_t ldx, const int32_t* row_index, const float* gamma, const float* beta,
                        void* y, int64_t ldy, int out_f32, float* mean, float* rstd, int64_t M, int64_t D, float eps,
                        void* stream);
/* the same on fp16 rows (x f16 [.., ldx]; y bf16 / f32 / f16 by out_dtype = DCLIP_OUT_*): the frozen teacher's LayerNorms, whose input is
 * the fp16 residual stream and which compute in f32 and return the input's type (reference _common.py:14-20) */
int dclip_layernorm_fwd_f16(const void* x, int64_t ldx, const int32_t* row_index, const float* gamma, const float* beta,
                            void* y, int64_t ldy, int out_dtype, float* mean, float* rstd, int64_t M, int64_t D, float eps,
                            void* stream);
int dclip_layernorm_bwd(const void* dy, int64_t lddy, int dy_f32, const float* x, int64_t ldx, const int32_t* row_index,
                        const float* gamma, const float* mean, const float* rstd, float* dx_acc, int64_t lddx,
                        void* dx_bf16, int64_t lddb, float* dgamma, float* dbeta, float* colsum_acc, int64_t M, int64_t D,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Attention building blocks.  q/k/v/ctx are token-major bf16 (row = b*N + n, column = head*hd + d, row stride ld*);
 * score-like tensors are [B,H,N,Np], Np = round_up(N, 8) in the towers (the product entries and softmax_fwd / softmax_bwd take any
 * multiple of 8 with N <= Np <= 128 and refuse others with DCLIP_EINVAL, nothing launched; dclip_attn_mix_* take Np = round_up(N, 8)
 * alone), pad columns [N, Np) zero: nt and softmax_fwd / softmax_bwd write them as +0 (P, R, dS), nn / tn require them of A and
 * softmax_bwd of dR and P (the mix backward forms dA = P (dP - rs) on the pad columns inside a real 32-key tile and copies the
 * pad tiles of dR to dS).
 * hd in {32, 64}, N <= 128 (dclip_attn_stream_fwd alone takes longer sequences).
 *   reference teacher: _common.py:73-89 ; student: weight_share_model.py:101-125 (scale, QK^T, conv_l, softmax,
 *   conv_w, PV) ; causal mask: text_encoder.py:54-60.
 * nt : C[b,h,i,j] = alpha * sum_d A[(b,i),h*hd+d] * Bm[(b,j),h*hd+d]          (S = QK^T ; dR = dO V^T)
 * nn : C[(b,i),h*hd+d] = alpha * sum_j A[b,h,i,j] * Bm[(b,j),h*hd+d]          (O = R V ; dQ = dS K)
 * tn : C[(b,j),h*hd+d] = alpha * sum_i A[b,h,i,j] * Bm[(b,i),h*hd+d]          (dV = R^T dO ; dK = dS^T Q)
 * softmax_fwd : A_g = sum_h Wl[g,h] S_h ; P = softmax_j(A) (causal: j <= i) ; R_g = sum_h Ww[g,h] P_h.
 *               Wl/Ww NULL = plain multi-head softmax (CLIP towers; any head count — with mixing H must be 2, 4, 8, 12 or 24).
 *               P (nullable) is saved for backward.
 * softmax_bwd : dS from dR (+ dWl, dWw += H x H weight gradients, f32).
 */
int dclip_attn_nt(const void* A, int64_t lda, const void* Bm, int64_t ldb, void* C, int out_f32, int64_t B, int64_t H,
                  int64_t N, int64_t Np, int64_t hd, float alpha, void* stream);
/* a_blocked != 0: A is in the quad-blocked layout the register-resident score stage writes (dclip_attn_mix_fwd / _bwd):
 * [B, H, Np / 4, N, 4], element (i, j) of a (b, h) matrix at ((j >> 2) * N + i) * 4 + (j & 3); 0: row-major [B, H, N, Np]. */
int dclip_attn_nn(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N,
                  int64_t Np, int64_t hd, float alpha, int a_blocked, void* stream);
int dclip_attn_tn(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N,
                  int64_t Np, int64_t hd, float alpha, int a_blocked, void* stream);
/* fused_fwd : ctx = softmax(scale * q k^T (+ causal mask)) v for plain multi-head attention (teacher, _common.py:73-89);
 *              qkv is the fused [B*N, 3*H*hd] projection ; scores / probabilities never reach HBM. */
int dclip_attn_fused_fwd(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                         float scale, int causal, void* stream);
/* stream_fwd : the same product for sequences dclip_attn_fused_fwd does not take (the frozen ViT-B/16 / ViT-L/14 teachers: 197, 257, 577
 *              tokens): any N >= 1, non-causal, hd = 64 only.  64 queries per workgroup, keys streamed through LDS in chunks of 64 with a
 *              running maximum and sum per query; scores / probabilities never reach HBM.  ldq >= 3*H*hd and
 *              ldc >= H*hd in elements, multiples of 8; qkv and ctx 16-byte aligned.  Refused (DCLIP_EINVAL, nothing launched): a null
 *              pointer, N <= 0, hd != 64, a misaligned pointer or stride.  Added without a version bump: no existing signature changed. */
int dclip_attn_stream_fwd(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                          float scale, void* stream);
int dclip_attn_softmax_fwd(const float* S, const float* Wl, const float* Ww, void* P, void* R, int64_t B, int64_t H,
                           int64_t N, int64_t Np, int causal, void* stream);
int dclip_attn_softmax_bwd(const void* dR, const void* P, const void* S, int scores_bf16, const float* Wl, const float* Ww,
                           void* dS, float* dWl, float* dWw, int64_t B, int64_t H, int64_t N, int64_t Np, void* stream);
/*
 * Head-mixed student attention, score stage, with the score tensors kept in registers and BOTH head mixes on the matrix pipe
 * (attention_mix.hip + attn_mix_wave.h; reference weight_share_model.py:101-125).  One wave per (sample, 16 query rows):
 * S = scale q k^T comes out of block-diagonal MFMAs with lane group g holding head 4s + g, so that the packed accumulator
 * registers are the B operand of A = conv_l(S) with the mix matrix as the A operand; P = softmax(A) is a per-register exp2
 * against the log-sum-exp that enters as the initial accumulator; R = conv_w(P) contracts over the accumulator's row index
 * (no lane movement).  Only R (bf16, quad-blocked [B,H,Np/4,N,4]: element (i, j) at ((j >> 2) * N + i) * 4 + (j & 3), pad
 * columns zero -- a lane owns a query, so this is the layout in which a wave's 8-byte stores of 4 keys are contiguous over
 * the 16 queries of a tile; dclip_attn_nn / _tn read it with a_blocked = 1) and the softmax statistics (f32 [B,H,N]:
 * log-sum-exp of every row of A) are stored.  The backward recomputes S, A, P from the packed qkv rows, forms dR = dO v^T on the fly and
 * writes dS (bf16, same quad-blocked layout, gradient of the scaled pre-mix scores); dWl / dWw += [H,H] leave as one partial tile per workgroup in
 * `workspace` (dclip_attn_mix_bwd_workspace_bytes(B, H, N) bytes, 16-byte aligned; it also carries the [B,H,N] softmax-backward
 * row sums between the two launches of the backward) summed by a further launch: no atomics, run-to-run identical.  The products over keys / queries stay with dclip_attn_nn / dclip_attn_tn:
 *   forward   dclip_attn_mix_fwd -> dclip_attn_nn(R, v) ;   backward   dclip_attn_tn(R, dO) -> dV, dclip_attn_mix_bwd -> dS,
 *             dclip_attn_nn(dS, k) -> dQ, dclip_attn_tn(dS, q) -> dK.
 * Replaces dclip_attn_nt + dclip_attn_softmax_fwd and dclip_attn_nt + dclip_attn_softmax_bwd (S f32, P, dR never stored).
 * Mix operands are f16 in the forward (the precision of the reference's fp16 autocast) and bf16 on the gradient side.
 * dclip_attn_mix_supported: H in {2, 4, 8, 12} with hd in {32, 64}, or H = 24 with hd = 32; N <= 128 (other shapes use the
 * unfused kernels).
 */
int dclip_attn_mix_supported(int64_t H, int64_t N, int64_t hd);
size_t dclip_attn_mix_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N);
void dclip_attn_mix_debug_stamps(void* fwd, void* bwd_a, void* bwd_b);   /* diagnostics: per-tile cycle counts of later launches, NULL = off */
int dclip_attn_mix_fwd(const void* qkv, int64_t ld, const float* Wl, const float* Ww, void* R, float* stats, int64_t B, int64_t H,
                       int64_t N, int64_t Np, int64_t hd, float scale, void* stream);
int dclip_attn_mix_bwd(const void* qkv, int64_t ld, const void* dO, int64_t ldo, const float* Wl, const float* Ww,
                       const float* stats, void* dS, float* dWl, float* dWw, void* workspace, size_t ws_bytes, int64_t B, int64_t H,
                       int64_t N, int64_t Np, int64_t hd, float scale, void* stream);
/*
 * Row-tile forms, for a block execution of which only ONE row per sample is read afterwards (the class token / EOT row of a tower's last
 * execution).  pick: device int32 [B], pick[b] = b * N + n (dclip_pick_index).  Each works on the 16-row tile
 * it = (pick[b] - b * N) >> 4 of every sample alone, with the fragments, rings and MFMA order of its full form, so what it writes is
 * bit-equal to the full form's (weight gradients: up to the order in which per-workgroup partials are summed).
 *   nn_rows       : the tile's rows of C; the other rows are stored as zeros (fill_zero != 0) or left untouched (0).
 *   tn_rows       : contracts over the tile's rows only; rows of A and Bm outside the tile are never read.  All N rows of C are written.
 *   fused_fwd_rows: the tile's rows of ctx; other rows untouched.
 *   mix_fwd_rows  : the tile's rows of R and stats; other rows untouched.
 *   mix_bwd_rows  : reads stats and writes dS (and the delta rows of the workspace) on the tile's rows only; dWl / dWw += as the full form.
 * Rows outside the tiles of R, stats and dS therefore hold stale data after these calls: only row-tile forms may consume them.
 * The backward forms equal the full backward when dO is zero outside the picked rows.  Added without a version bump: no existing
 * signature changed.
 */
int dclip_attn_nn_rows(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t Np,
                       int64_t hd, float alpha, int a_blocked, const int32_t* pick, int fill_zero, void* stream);
int dclip_attn_tn_rows(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t Np,
                       int64_t hd, float alpha, int a_blocked, const int32_t* pick, void* stream);
int dclip_attn_fused_fwd_rows(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                              float scale, int causal, const int32_t* pick, void* stream);
int dclip_attn_mix_fwd_rows(const void* qkv, int64_t ld, const float* Wl, const float* Ww, void* R, float* stats, int64_t B, int64_t H,
                            int64_t N, int64_t Np, int64_t hd, float scale, const int32_t* pick, void* stream);
int dclip_attn_mix_bwd_rows(const void* qkv, int64_t ld, const void* dO, int64_t ldo, const float* Wl, const float* Ww,
                            const float* stats, void* dS, float* dWl, float* dWw, void* workspace, size_t ws_bytes, int64_t B, int64_t H,
                            int64_t N, int64_t Np, int64_t hd, float scale, const int32_t* pick, void* stream);
/*
 * Head-mean attention maps (attn_maps.hip; the attention_score_mse / attention_probs_mse terms, reference
 * model/loss_component/attention_score_mse.py, attention_probs_mse.py, which only ever read sum(dim=1) / H of a map).
 * maps_fwd : score_map = mean_h S_h, prob_map = mean_h softmax(conv_l(S))_h, f32 [B, N, N] each (nullable), from the packed qkv rows
 *            (ld elements, 16-byte aligned) the score stage read; S = scale q k^T.  Wl = the [H, H] conv_l weight (students,
 *            weight_share_model.py:101-121) or NULL (CLIP towers, _common.py:73-94).  causal: masked scores read 0 (text_encoder.py:81-85),
 *            masked probabilities are 0.  One workgroup per (sample, 4 query rows) with every head's S of the tile in LDS; per exported
 *            map it reads the q and k columns of qkv (2 B * N * H * hd bytes) and writes B * N * N * 4 bytes.  hd in {32, 64}, N <= 128.
 * maps_bwd : dS[h] += g_S / H + (Wl^T dA)[h],  dA[g] = P[g] o (g_P / H - rowsum(P[g] o g_P / H)), P recomputed from qkv; d_score_map /
 *            d_prob_map f32 [B, N, N] (nullable).  dS = the score stage's gradient of the scaled pre-mix scores, bf16 [B, H, N, Np], in the
 *            quad-blocked layout of dclip_attn_mix_bwd (ds_blocked = 1) or row-major (0).  dWl (nullable) += sum dA_g S_h^T, built from
 *            per-workgroup [H, H] partials in `workspace` (dclip_attn_maps_bwd_workspace_bytes(B, H, N) bytes, needed when Wl, dWl and
 *            d_prob_map are all given) and a fixed-order reduce: no atomics, run-to-run identical.  Masked entries get no gradient.
 */
int dclip_attn_maps_fwd(const void* qkv, int64_t ld, const float* Wl, float* score_map, float* prob_map, int64_t B, int64_t H, int64_t N,
                        int64_t hd, float scale, int causal, void* stream);
size_t dclip_attn_maps_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N);
int dclip_attn_maps_bwd(const void* qkv, int64_t ld, const float* Wl, const float* d_score_map, const float* d_prob_map, void* dS,
                        int ds_blocked, float* dWl, void* workspace, size_t ws_bytes, int64_t B, int64_t H, int64_t N, int64_t Np,
                        int64_t hd, float scale, int causal, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Embedding-side helpers (HBM-bound).
 * cast_bf16            : f32 -> bf16 copy (per-step weight down-cast).
 * cast_transpose_bf16_multi : per job, W f32 [R,C] -> Wb bf16 [R,C] (nullable) and Wt bf16 [C,R] (nullable; the dgrad operand).
 * im2row               : image f32 [B,C,res,res] -> bf16 rows [B*(G*G+cls_rows), C*p*p], G = res / p; the class-token row
 *                        is zero.  Conv2d(k=p,s=p) of _common.py:176,196 / timm PatchEmbed (weight_share_model.py:250).
 * im2row_ld            : im2row with rows of stride ldk >= C*p*p elements (ldk even), columns [C*p*p, ldk) zero, and any EVEN patch:
 *                        patch 14 gives C*p*p = 588, which the GEMM contraction (K % 64 == 0) takes padded to 640.
 * token_table          : out[0] = pos[0] + cls ; out[n>=1] = pos[n] + bias  (cls NULL: out[n] = pos[n] + bias)
 *                        (_common.py:199-202 ; weight_share_model.py:346-349, :489) ; token_table_bwd is its adjoint given
 *                        tok_sum[n] = sum_b G[b,n,:] from batch_sum_acc.
 * embed_gather         : out[r] = table[ids[(r / N) * id_stride + r % N]] + pos[r % N] (text_encoder.py:65-66 ;
 *                        weight_share_model.py:487-489); id_stride = tokens per caption in `ids`, N <= id_stride = tokens used.
 * embed_scatter_add    : dtable[ids[r]] += dx[r] (f32 atomics; rows with the hot ids 0 / vocab-2 / vocab-1 = padding / SOT / EOT
 *                        of the clip.tokenize layout are reduced per block first instead of contending on three table rows).
 * pick_index           : idx[b] = b*N + argmax_n ids[b, 0..id_stride) (text_encoder.py:86, weight_share_model.py:506); ids NULL: b*N.
 * adamw                : torch.optim.AdamW step on flat f32 buffers (distil_model.py:160-162, dual_distill_model.py:194-196).
 */
int dclip_cast_bf16(const float* src, void* dst, int64_t n, void* stream);
int dclip_cast_f16_f32(const void* src, float* dst, int64_t n, void* stream);   /* f16 -> f32 (teacher hidden-state export) */
/* dst += src (f32) ; optional bf16 copy of the updated dst ; optional column sums of src (row length D; then n % D == 0) */
int dclip_axpy_f32(float* dst, const float* src, void* dst_bf16, int64_t n, float* colsum_acc, int64_t D, void* stream);
/* n cast_transpose jobs in one launch (per-step refresh of a student tower's bf16 weight cache): host arrays of device pointers
 * and shapes; Wb[i] / Wt[i] nullable per job. */
int dclip_cast_transpose_bf16_multi(const float* const* W, void* const* Wb, void* const* Wt, const int64_t* R, const int64_t* C,
                                    int64_t n, void* stream);
int dclip_im2row(const float* img, void* rows, int64_t B, int64_t C, int64_t res, int64_t patch, int cls_rows, void* stream);
int dclip_im2row_ld(const float* img, void* rows, int64_t ldk, int64_t B, int64_t C, int64_t res, int64_t patch, int cls_rows,
                    void* stream);
int dclip_token_table(const float* pos, const float* cls, const float* bias, float* out, int64_t ntok, int64_t D, void* stream);
int dclip_token_table_bwd(const float* tok_sum, float* dpos, float* dcls, float* dbias, int64_t ntok, int64_t D, int has_cls,
                          void* stream);
int dclip_batch_sum_acc(const float* G, float* out, int64_t B, int64_t N, int64_t D, void* stream);
int dclip_embed_gather(const int64_t* ids, int64_t id_stride, const float* table, const float* pos, void* out, int out_dtype,
                       int64_t rows, int64_t N, int64_t D, void* stream);
int dclip_embed_scatter_add(const int64_t* ids, const void* dx, int dx_f32, float* dtable, int64_t rows, int64_t D,
                            int64_t vocab, void* stream);
int dclip_pick_index(const int64_t* ids, int64_t id_stride, int32_t* idx, int64_t B, int64_t N, void* stream);
int dclip_adamw(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int64_t step, int zero_grad, void* stream);   /* zero_grad: g := 0 once consumed */
/* the same step on `count` <= DCLIP_ADAMW_MAX_RANGES ranges in ONE launch (HOST arrays of device pointers and lengths; every range a
 * multiple of 4 elements, 16-byte aligned): the sharded data-parallel optimizer updates one owned slice per gradient bucket */
#define DCLIP_ADAMW_MAX_RANGES 24
int dclip_adamw_multi(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad, void* stream);
/* dclip_adamw_multi on gs = g * (*gscale), the product rounded to f32 before anything else uses it (gscale: DEVICE pointer to one
 * f32, read by the kernel, e.g. out + 1 of dclip_clip_coef).  gscale NULL: dclip_adamw_multi itself. */
int dclip_adamw_multi_scaled(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count,
                             float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad,
                             const float* gscale, void* stream);
/*
 * Global gradient-norm clipping, torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) (the reference reaches it through
 * Lightning's gradient_clip_val), without a host-visible norm:
 *   sumsq_multi : sum of g^2 over `count` <= DCLIP_ADAMW_MAX_RANGES read-only ranges (HOST arrays; the alignment rules of
 *                 dclip_adamw_multi) as DCLIP_SUMSQ_PARTIALS f32 partial sums, one per workgroup, partials[0 .. n_partials)
 *                 (n_partials >= DCLIP_SUMSQ_PARTIALS; the slots past the workgroups' are written as 0).  No atomics: the same
 *                 call gives the same bits.
 *   clip_coef   : sum = partials[0] + ... + partials[n_partials - 1] (in double, fixed order) + *extra_sumsq (DEVICE, may be NULL:
 *                 a sum of squares that is already complete, e.g. of gradients every rank holds whole) ;
 *                 out[0] = (float)sqrt(sum) ; out[1] = min(1, max_norm / (out[0] + 1e-6f)).  A non-finite sum is not
 *                 special-cased: NaN gives out[1] = NaN, as torch does.
 */
#define DCLIP_SUMSQ_PARTIALS 1024
int dclip_sumsq_multi(const float* const* g, const int64_t* n, int32_t count, float* partials, int64_t n_partials, void* stream);
int dclip_clip_coef(const float* partials, int64_t n_partials, const float* extra_sumsq, float max_norm, float* out, void* stream);
/*
 * The same step under a loss scaler (torch.amp.GradScaler's protocol for an optimizer with _step_supports_amp_scaling: the scaler
 * hands over its scale and its overflow flag as device tensors, the optimizer unscales in its kernel and skips on the device):
 *   amp_prepare     : one workgroup, after the sums and before the updates.  Writes the step's control record (DEVICE,
 *                     DCLIP_AMP_RECORD_FLOATS f32, 16-byte aligned) from
 *                       found_inf, grad_scale : DEVICE, one f32 each, either may be NULL (no overflow / scale 1) ;
 *                       partials, n_partials, extra_sumsq, max_norm : as dclip_clip_coef, or NULL, 0, NULL for a step that does not clip ;
 *                       skipped : DEVICE, one int64 the caller keeps across steps (8-byte aligned, 0 before the first step) ;
 *                     record[DCLIP_AMP_SKIP] = (*found_inf != 0) ; *skipped += that ;
 *                     record[DCLIP_AMP_NORM] = (float)(sqrt(sum) / *grad_scale), the norm of the unscaled gradients (0 without clipping) ;
 *                     record[DCLIP_AMP_COEF] = min(1, max_norm / (norm + 1e-6f)) (1 without clipping) ;
 *                     record[DCLIP_AMP_MULT] = coef / *grad_scale ;
 *                     record[DCLIP_AMP_BC1], [DCLIP_AMP_BC2_SQRT] = dclip_adamw_multi's bias corrections 1 - beta1^t and sqrt(1 - beta2^t)
 *                     for t = step - *skipped, bit for bit what a host step t gives.
 *   adamw_multi_amp : dclip_adamw_multi_scaled with gscale = record[DCLIP_AMP_MULT] and the record's bias corrections.  With
 *                     record[DCLIP_AMP_SKIP] set it writes no p, m or v; g is still cleared if zero_grad.  The gradient is never
 *                     written back unscaled (torch's fused AdamW does that; nothing here reads it afterwards).
 */
#define DCLIP_AMP_RECORD_FLOATS 8
#define DCLIP_AMP_MULT 0
#define DCLIP_AMP_SKIP 1
#define DCLIP_AMP_BC1 2
#define DCLIP_AMP_BC2_SQRT 3
#define DCLIP_AMP_NORM 4
#define DCLIP_AMP_COEF 5
int dclip_amp_prepare(const float* found_inf, const float* grad_scale, const float* partials, int64_t n_partials, const float* extra_sumsq,
                      float max_norm, float beta1, float beta2, int64_t step, int64_t* skipped, float* record, void* stream);
int dclip_adamw_multi_amp(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int zero_grad, const float* record, void* stream);
/*
 * The same step keeping an exponential moving average of the parameters: one more f32 range e[k] per range, in the same launch.
 *   adamw_multi_ema : gscale == NULL and record == NULL: dclip_adamw_multi ; gscale alone: dclip_adamw_multi_scaled ; record alone:
 *                     dclip_adamw_multi_amp (`step` is then not read: the record carries the bias corrections) ; both: refused.
 *                     p, g, m, v come out bit for bit as from that entry.  Per element, with p' the parameter this launch writes
 *                     and w = ema_weight:
 *                         d = p' - e (rounded to f32) ;  e <- d == 0 ? e : fmaf(w, d, e)
 *                     two roundings, the difference and the fused multiply-add: |e' - (e + w (p' - e))| <= u (|w (p' - e)| + |e'|)
 *                     to first order, u = 2^-24.  p' == e gives e back bit for bit (the sign of a zero included), so a parameter
 *                     that has stopped moving does not drift.  ema_weight == 0 runs the step alone: e is neither read nor
 *                     written.  A skipped step (record[DCLIP_AMP_SKIP] set) reads and writes no e, like p, m, v.
 *                     ema_weight: 1 - decay, in [0, 1].  Form it in double and round once, (float)(1.0 - decay): in f32,
 *                     1.f - 0.9999f is 1.66e-4 off relatively.
 *                     e[k]: 16-byte aligned, n[k] elements, disjoint from everything else.  Refused on the host, before any
 *                     launch: whatever dclip_adamw_multi refuses, a NULL or misaligned e[k], ema_weight outside [0, 1] or NaN,
 *                     gscale together with record, a misaligned record.
 *   swap_multi      : a[k][0 .. n[k]) <-> b[k][0 .. n[k]) for `count` <= DCLIP_ADAMW_MAX_RANGES pairs in ONE launch (HOST arrays; the
 *                     alignment rules of dclip_adamw_multi), moved as 128-bit integers: every bit pattern survives (NaN payloads,
 *                     -0).  a[k] == b[k] is allowed and leaves the range as it is; two sides that overlap otherwise are refused.
 *                     Ranges of different k must not overlap (not checked).
 */
int dclip_adamw_multi_ema(float* const* p, float* const* g, float* const* m, float* const* v, float* const* e, const int64_t* n, int32_t count,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad, float ema_weight,
                          const float* gscale, const float* record, void* stream);
int dclip_swap_multi(float* const* a, float* const* b, const int64_t* n, int32_t count, void* stream);
/*
 * The same step with per-range hyper-parameters (parameter groups: no decay on 1-D parameters, a smaller learning rate for the parts
 * that arrive initialised), driven by a table in DEVICE memory: ONE launch for any number of ranges, no cap of DCLIP_ADAMW_MAX_RANGES.
 * p, g, m, v and e are the BASES of five streams that share one flat layout (a tower's flat buffers); range k covers the elements
 * [begin, begin + length) of each of them.
 *   adamw_table_bytes : size of the table of `count` ranges: count + 1 records of 32 bytes, the struct below; 0 for count < 1.
 *   adamw_table_fill  : builds and validates the HOST image of the table, which the caller then copies to the device (8-byte aligned
 *                       there too).  begin, length, lr_scale, weight_decay: HOST arrays of `count` >= 1 entries.  Ranges ascend, do not
 *                       overlap and are not empty; begin and length are multiples of 4 elements (with 16-byte aligned bases every range
 *                       is then 16-byte aligned); lr_scale is finite and >= 0, weight_decay finite; every range ends inside `total`,
 *                       the element count of the buffers, which the caller states.  Record k also holds tile0, the first tile of
 *                       range k in the launch's tile list: every range starts a new tile of DCLIP_ADAMW_TABLE_TILE elements; record
 *                       `count` closes the list with the number of tiles, which *tiles returns.  A refusal writes neither the image
 *                       nor *tiles.
 *   adamw_table       : gscale == NULL and record == NULL: the step of dclip_adamw_multi ; gscale alone: of dclip_adamw_multi_scaled ;
 *                       record alone: of dclip_adamw_multi_amp (`step` is then not read) ; both: refused.  e != NULL: it keeps the
 *                       average of dclip_adamw_multi_ema with ema_weight (e == NULL, or ema_weight == 0: e is neither read nor written).
 *                       Roundings: per range lr_k = lr * lr_scale_k, ONE f32 product of the two f32 values, and wd_k = weight_decay_k as
 *                       stored; after that every element is computed exactly as by those entries called on the range alone with
 *                       lr_k and wd_k: p, g, m, v, e come out bit for bit as from them.  No atomics: the same call gives the same
 *                       bits.  A skipped step (record[DCLIP_AMP_SKIP] set) reads and writes no p, m, v, e; g is still cleared if
 *                       zero_grad.  Elements outside the ranges are neither read nor written.
 *                       table, count, tiles: the device copy of an image of adamw_table_fill, and what it was filled with / returned.
 *                       Refused on the host, before any launch: a NULL or misaligned base (e may be NULL), a NULL or misaligned
 *                       table, count < 1, tiles < count or > 2^31 - 1, step < 1 without a record, a misaligned record, gscale
 *                       together with record, ema_weight outside [0, 1] or NaN with e given.  The table itself is in device memory:
 *                       the host cannot see it, and a table that does not match count and the buffers is the caller's error.
 */
#define DCLIP_ADAMW_TABLE_TILE 8192
typedef struct dclip_adamw_range {
    int64_t tile0;            /* first tile of the range ; in record `count`: the number of tiles */
    int64_t begin, length;    /* elements, multiples of 4 */
    float lr_scale, weight_decay;
} dclip_adamw_range;
size_t dclip_adamw_table_bytes(int32_t count);
int dclip_adamw_table_fill(const int64_t* begin, const int64_t* length, const float* lr_scale, const float* weight_decay, int32_t count,
                           int64_t total, void* image, size_t image_bytes, int64_t* tiles);
int dclip_adamw_table(float* p, float* g, float* m, float* v, float* e, const void* table, int32_t count, int64_t tiles, float lr, float beta1,
                      float beta2, float eps, int64_t step, int zero_grad, float ema_weight, const float* gscale, const float* record,
                      void* stream);
/*
 * Layer-wise trust ratios (LAMB; You et al. 2020, timm's Lamb) on the same table: one range is one UNIT, normally one parameter tensor,
 * and its update is scaled by |p| / |u|, the L2 norms taken over the unit.  Per element of unit k, in f32, with g' = g, g * *gscale or
 * g * record[DCLIP_AMP_MULT] and the bias corrections bc1, bc2s of dclip_adamw_table:
 *       m'  = b1 m + (1 - b1) g' ;  v' = b2 v + (1 - b2) g' g'           (the very lines of the AdamW kernels: m', v' come out bit for bit
 *                                                                          as from dclip_adamw_table on the same inputs)
 *       u   = fmaf(wd_k, p, (m' / bc1) / (sqrtf(v') / bc2s + eps))        weight decay INSIDE the update, not the p (1 - lr wd) of AdamW
 *       r_k = 1                      if wd_k == 0 and not always_adapt
 *           = |p| / |u|              if both norms, rounded to f32, are > 0 and finite, else 1 ; the quotient of the double norms, rounded once
 *       r_k = min(r_k, trust_clip)   if trust_clip >= 0
 *       p'  = fmaf(-(lr_k * r_k), u, p)     lr_k = lr * lr_scale_k, ONE f32 product, then ONE f32 product with r_k
 *       e   <- the average of dclip_adamw_multi_ema from p' (e == NULL, or ema_weight == 0: e is neither read nor written)
 *   The norms are over the OLD p and over u.  Three launches on `stream`, no atomics, no host synchronisation: the same call gives the
 *   same bits.  Sums of squares: per tile of DCLIP_ADAMW_TABLE_TILE elements every lane adds its <= 32 squares in f32 (four chains of
 *   <= 8 fused multiply-adds and two additions: relative error <= 10 * 2^-24 of the lane's sum), everything above the lane is added in
 *   double, in a fixed order.
 *   lamb_workspace_bytes : bytes of the tile records (16 per tile) for a table of `count` ranges and `tiles` tiles; 0 for count < 1,
 *                          tiles < count or tiles > 2^31 - 1.
 *   lamb_table           : table, count, tiles: as dclip_adamw_table (an uploaded image of dclip_adamw_table_fill).  workspace: DEVICE,
 *                          16-byte aligned, ws_bytes >= lamb_workspace_bytes; contents need not survive between calls.  stats: DEVICE,
 *                          f32 [count][4], 16-byte aligned: {|p|, |u|, r_k, 0} of every range after the call.
 *                          A skipped step (record[DCLIP_AMP_SKIP] set) changes no byte of p, m, v, e and of stats; g is still cleared if
 *                          zero_grad.  Elements outside the ranges are neither read nor written.
 *                          Refused on the host, before any launch: whatever dclip_adamw_table refuses, a NULL or misaligned workspace
 *                          or stats, a workspace smaller than lamb_workspace_bytes, a NaN trust_clip (trust_clip < 0: no clip).
 */
size_t dclip_lamb_workspace_bytes(int32_t count, int64_t tiles);
int dclip_lamb_table(float* p, float* g, float* m, float* v, float* e, const void* table, int32_t count, int64_t tiles, float lr, float beta1,
                     float beta2, float eps, int64_t step, int zero_grad, float ema_weight, const float* gscale, const float* record,
                     float trust_clip, int always_adapt, void* workspace, size_t ws_bytes, float* stats, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused distillation loss, forward + backward.
 *   reference: model/_loss.py:118-202 (cal_tow_tower_loss / cal_one_tower_loss), model/component/clip_model.py:37-44,
 *   model/loss_component/{out_l1,out_cos,out_kl,out_ce,clip_cos_diff,hard_label,soft_label,logits_mse}.py.
 * s_*, t_*: student / teacher last_representation, f32 [B,E] (E % 16 == 0, E <= 1024, B <= 4096).
 * cfg (HOST pointer, 10 floats): w_out_l1, w_out_cos, w_out_kl, w_out_ce, w_cos_diff, w_hard_label, w_soft_label,
 *   w_logits_mse (each = loss_scale * percent of _loss.py:148-152,195-200; 0 disables), temperature, two_tower (0/1).
 *   two_tower = 1: loss = 0.5 * (image_tower + text_tower) + cross-modal terms ; 0: tower 0 only (s_txt etc. ignored).
 * out_scalars (device, 16 f32): [0] total ; [1..4] image out_l1, out_cos, out_kl, out_ce ; [5..8] text ; [9..12] cos_diff,
 *   hard_label, soft_label, logits_mse — raw (un-scaled) term values.
 * d_s_img / d_s_txt (f32 [B,E]): d total / d student embeddings (overwritten).  The [B,B] logits never reach HBM.
 */
size_t dclip_distill_loss_workspace(int64_t B, int64_t E);
int dclip_distill_loss(const float* s_img, const float* t_img, const float* s_txt, const float* t_txt, int64_t B, int64_t E,
                       const float* cfg, float* out_scalars, float* d_s_img, float* d_s_txt, void* workspace,
                       size_t ws_bytes, void* stream);
/*
 * Training image transform after decode / resize / crop: RandAugment -> ToTensor -> Normalize.
 *   reference: data/component/ms_coco.py:15-26 (transform chain), rand_augment.py:10-87 (_apply_op), :128-166 (op table,
 *   per-image loop), utils.py:11-12 (CLIP mean / std).  Pixel results equal Pillow's (the reference's backend) bit for bit.
 * images: uint8 [B,H,W,3] device (RGB, what np.asarray(PIL image) holds); ops: device [B, num_ops] records, applied in order:
 *   op 0 identity ; 1 nearest affine, c[0..5] = Pillow's 16.16 fixed-point coefficients (a0 a1 a2 a3 a4 a5 of Geometry.c
 *   affine_fixed) ; 2 integer shift, source = (x + c[0], y + c[1]) ; 3 brightness, 4 contrast, 5 sharpness with enhancement
 *   factor f ; 6 posterize with byte mask c[0] ; 7 autocontrast ; 8 equalize.   (distillclip_amd/augment.py builds the
 *   records from RandAugment's (op name, magnitude) draws.)
 * mean3 / std3: HOST float[3].  out: f32 [B,3,H,W] = (byte / 255 - mean) / std.  aug_out (nullable): the augmented bytes
 * [B,H,W,3].  workspace: dclip_augment_workspace(B,H,W) bytes (two byte images per sample), unused when num_ops == 0.
 */
typedef struct dclip_aug_op {
    int32_t op;
    int32_t c[6];
    float f;
} dclip_aug_op;
size_t dclip_augment_workspace(int64_t B, int64_t H, int64_t W);
int dclip_augment_normalize(const uint8_t* images, int64_t B, int64_t H, int64_t W, const dclip_aug_op* ops, int num_ops,
                            const float* mean3, const float* std3, float* out, uint8_t* aug_out, void* workspace,
                            size_t ws_bytes, void* stream);
/*
 * Resize(S) + CenterCrop(S) of a batch of decoded RGB images of mixed sizes, Pillow's antialiased
 * bilinear two-pass resample evaluated on the crop window, bit-exact.
 *   reference: data/component/ms_coco.py:16-17,23-24 (transforms.Resize(224) + transforms.CenterCrop(224) on PIL images).
 * packed: device bytes, image i = uint8 [height, width, 3] at desc[i].src_offset.  desc: device [B].  tables: device int32;
 * image i's block at tables + table_offset holds  hb[S][2] (first source column, count) , hk[S][ksize_h] (22-bit fixed-point
 * weights) , vb[S][2] (first row relative to row0, count) , vk[S][ksize_v]  for the S crop columns / rows — the values
 * Pillow's precompute_coeffs + normalize_coeffs_8bpc produce (distillclip_amd/augment.py:resample_tables builds and caches
 * them per source size).  workspace: image i's horizontal-pass scratch uint8 [nrows, S, 3] at temp_offset.
 * out: uint8 [B,S,S,3].
 */
typedef struct dclip_resize_desc {
    int64_t src_offset;
    int64_t table_offset;
    int64_t temp_offset;
    int32_t height, width;
    int32_t row0, nrows;
    int32_t ksize_h, ksize_v;
} dclip_resize_desc;
int dclip_resize_center_crop(const uint8_t* packed, const dclip_resize_desc* desc, const int32_t* tables, int64_t B, int64_t S,
                             uint8_t* out, void* workspace, size_t ws_bytes, void* stream);
/*
 * Validation retrieval metrics of one image -> caption logits matrix, without materialising it.
 *   reference: dual_distill_model.py:271-275 (norm_and_logits), :204-212 (log_diag_score), :220-224 (log_acc with
 *   torchmetrics accuracy(top_k = k) against labels arange(n)), k_list :87 ; distil_model.py:171-191, :224-231.
 * img, txt: f32 [n, E] device, un-normalised (rows are divided by their L2 norm, no epsilon, as the reference does);
 * ks: HOST array of nk <= 8 cut-offs.  out (device, nk + 2 f32): acc@ks[0..nk) (fraction of rows whose matching caption is
 * among the ks[i] highest logits of the row; strict comparison, a tie with the diagonal counts for the diagonal),
 * out[nk] = mean_i softmax(logits_i)[i], out[nk + 1] = mean_i logits_ii.  rank_out (device int32 [n], nullable) receives
 * the number of captions that beat the matching one.  Other pairings (student image x teacher text, ...) are further calls.
 * A zero row is NaN after the division, and so is every logit it enters: out[nk] and out[nk + 1] are then NaN.  A NaN logit beats
 * nothing and is beaten by nothing: a zero image row has rank 0 and leaves the other rows' ranks alone, a zero caption row counts for
 * no row (its own row has rank 0), and the accuracies stay the exact fractions of these ranks (tests/test_metrics_exact_gpu.py).
 */
size_t dclip_retrieval_metrics_workspace(int64_t n, int64_t E);
int dclip_retrieval_metrics(const float* img, const float* txt, int64_t n, int64_t E, const int32_t* ks, int nk,
                            float* out, int32_t* rank_out, void* workspace, size_t ws_bytes, void* stream);
/*
 * Recall@K retrieval with several captions per image, both directions, in one call (recall.hip): the MS-COCO protocol (5 000 images x
 * 25 010 captions on the 5k test split).  The reference's validation pairs each image with one caption (dclip_retrieval_metrics above);
 * its data set (data/component/ms_coco.py) carries the several captions ranked here.
 * Logits
 *   L[i, c] = cos(img_i, txt_c) on raw, un-normalised f32 rows [n_img, E] and [n_txt, E].
 *   The cosine is 0 when either norm is 0.  This is dclip_clipscore's convention: never NaN for finite rows.
 * Offsets
 *   txt_offsets is a DEVICE int32 [n_img + 1] table.
 *   Caption c belongs to image i iff txt_offsets[i] <= c < txt_offsets[i+1].
 *   The Python layer validates the counts on the host.
 *   The kernel clamps every offset into [0, n_txt] and reads end <= start as an empty group.  No table content makes it read or write
 *   outside its buffers.
 * Ranks
 *   rank_i2t[i] is the number of captions not owned by i with L[i, c] > max over i's own captions of L[i, c'].  It is -1 for an image
 *   without captions.
 *   rank_t2i[c] is the number of images j != owner(c) with L[j, c] > L[owner(c), c].  It is -1 for a caption no group covers, which can
 *   only happen with a malformed table.  (owner(c) is the last image i with txt_offsets[i] <= c, when c < txt_offsets[i+1].)
 *   Comparison is strict: a tie never counts against the target.
 *   Both sides of a comparison come from the same instruction sequence on the same rows.  Bit-equal rows then give bit-equal logits.
 * Outputs
 *   ks is a HOST array of nk <= 8 cut-offs.
 *   out is device f32 [2 nk + 2]:
 *     out[0..nk)   = image->text recall@ks over the images that have captions.
 *     out[nk..2nk) = text->image recall@ks over the covered captions.  A recall is the fraction with 0 <= rank < k.
 *     out[2nk] and out[2nk+1] = the two mean 0-based ranks over the same sets.
 *   Hits and rank sums are accumulated as integers.  Each output is the one-time correctly rounded quotient: divided in double, cast once
 *   (0 for an empty set, which only a malformed table produces).
 *   rank_i2t (device int32 [n_img]) and rank_t2i (device int32 [n_txt]) are nullable.
 * Determinism
 *   The [n_img, n_txt] logits never reach HBM.  No atomics.  The same call gives the same bits.
 * Limits, refused on the host with a message (DCLIP_EINVAL, nothing launched)
 *   E must be a positive multiple of 16.  1 <= n_img, n_txt < 2^24.  0 <= nk <= 8.  img, txt and workspace must be 16-byte aligned.
 *   Null operands and a workspace smaller than dclip_retrieval_recall_workspace(n_img, n_txt, E) are refused.
 * Added without a version bump: no existing signature changed.
 */
size_t dclip_retrieval_recall_workspace(int64_t n_img, int64_t n_txt, int64_t E);
int dclip_retrieval_recall(const float* img, const float* txt, const int32_t* txt_offsets, int64_t n_img, int64_t n_txt, int64_t E,
                           const int32_t* ks, int nk, float* out, int32_t* rank_i2t, int32_t* rank_t2i, void* workspace, size_t ws_bytes,
                           void* stream);
/*
 * Top-K search over embeddings (topk.hip): for every query row the k best gallery rows by cosine, with their logits.  It answers what
 * the entries above cannot: zero-shot classification over class prompts, the k best images for a caption, k-NN, hard negatives.
 * Logits
 *   L[i, j] = cos(q_i, g_j) on raw, un-normalised f32 rows [nq, E] and [ng, E].
 *   It is 0 when either row's squared norm is 0 or not a positive finite number (dclip_retrieval_recall's and dclip_clipscore's
 *   convention).  A row that holds an inf or a NaN is such a row: it is treated as the zero row.
 *   Rows are normalised once into the workspace.  Every logit comes from the tile routine of dclip_retrieval_recall, on rows from the
 *   same normaliser: bit-equal rows give bit-equal logits, and a logit here is bit for bit the one the recall kernels compare.
 * Order
 *   Row i of idx holds the first k gallery indices in the total order (L descending, index ascending).
 *   score[i, p] = L[i, idx[i, p]], exactly as the tile routine produced it (a -0 is reported as +0).
 *   -0 and +0 compare equal: a zero gallery row ties with any other 0 logit and the lower index wins.
 *   The order is total, so the result is a function of the logits alone: the same bits on every call, and the result for k1 < k2 is
 *   the prefix of the result for k2.
 *   When k > ng, the trailing k - ng entries of a row are idx = -1, score = -inf.
 * Outputs
 *   idx is device int32 [nq, k].  score is device f32 [nq, k] and may be NULL.  Both are fully overwritten, with plain stores.
 * Determinism
 *   The [nq, ng] logits never reach HBM.  No atomics.  Nothing waits for the device.
 * Limits, refused on the host with a message (DCLIP_EINVAL, nothing launched)
 *   1 <= k <= 64.  1 <= nq, ng < 2^24.  E must be a positive multiple of 16.  queries, gallery and workspace must be 16-byte aligned,
 *   idx and score 4-byte.  Null queries, gallery, idx or workspace, and a workspace smaller than
 *   dclip_topk_search_workspace(nq, ng, E, k), which is 0 for arguments the search refuses.
 * Added without a version bump: no existing signature changed.
 */
size_t dclip_topk_search_workspace(int64_t nq, int64_t ng, int64_t E, int k);
int dclip_topk_search(const float* queries, const float* gallery, int64_t nq, int64_t ng, int64_t E, int k, int32_t* idx, float* score,
                      void* workspace, size_t ws_bytes, void* stream);
/*
 * Mean of the normalised rows of each group (topk.hip): class embeddings from prompt ensembles.
 *   out[c] = (1 / n_c) sum over r in [offsets[c], offsets[c + 1]) of x_r / |x_r|, n_c the number of rows of the group.
 *   x / |x| is the normaliser of the search above: a row whose squared norm is 0 or not a positive finite number adds nothing.
 *   An empty group gives the zero row.  The mean is not normalised again: the search normalises its gallery.
 * offsets is a DEVICE int32 [n_groups + 1] table.  Every offset is clamped into [0, n_rows] by the kernel and end <= start reads as an
 * empty group, so no table content makes it read outside rows.  The Python layer validates the counts on the host.
 * rows f32 [n_rows, E], out f32 [n_groups, E], fully overwritten.  One wave per group adds its rows in index order: no atomics, the
 * same call gives the same bits.
 * Limits, refused on the host (DCLIP_EINVAL, nothing launched): 1 <= n_groups, n_rows < 2^24.  E a positive multiple of 16, at most
 * 4096.  Null operands.  rows and out 16-byte, offsets 4-byte aligned.  Added without a version bump.
 */
int dclip_group_mean_rows(const float* rows, const int32_t* offsets, int64_t n_groups, int64_t n_rows, int64_t E, float* out,
                          void* stream);
/*
 * L-CLIPScore scoring: CLIP-S and RefCLIP-S (Hessel et al. 2021) of K candidate captions per image against the image and against a
 * ragged set of reference captions, in one launch (score.hip; the metric the reference's students are trained to be — the reference
 * itself ships no scorer).
 *   cos(a, b) = a.b / (|a| |b|), 0 when either norm is 0 (never NaN for finite rows whose squared norms are finite in f32)
 *   clip_s[b K + k]    = w max(cos(img[b], cand[b K + k]), 0)                       (the paper's w = 2.5)
 *   ref_s[b K + k]     = max(0, max over r in [ref_offsets[b], ref_offsets[b + 1]) of cos(cand[b K + k], refs[r])), 0 for an empty set
 *   refclip_s[b K + k] = 2 clip_s ref_s / (clip_s + ref_s), 0 when the denominator is 0
 * img f32 [B, E], cand f32 [B K, E], refs f32 [R, E] or NULL: the towers' raw last_representation rows, un-normalised (the norms are
 * formed in the kernel); ld_* = row strides in elements, >= E and multiples of 4; the three row pointers 16-byte aligned.
 * ref_offsets: DEVICE int32 [B + 1], NULL exactly when refs is NULL.  Every offset is clamped into [0, R] by the kernel and
 * end <= start reads as an empty set, so no table content makes it read outside refs.  E % 4 == 0, 4 <= E <= 1024; B, K >= 1; R >= 0.
 * clip_s, ref_s, refclip_s: f32 [B K] each, fully overwritten; ref_s and refclip_s may be NULL and must be without refs.
 * One wave per candidate row; plain stores, no atomics, no workspace: the same call gives the same bits.  Added without a version bump:
 * no existing signature changed.
 */
int dclip_clipscore(const float* img, int64_t ld_img, const float* cand, int64_t ld_cand, const float* refs, int64_t ld_ref,
                    const int32_t* ref_offsets, int64_t B, int64_t K, int64_t R, int64_t E, float w, float* clip_s, float* ref_s,
                    float* refclip_s, void* stream);
/*
 * Kendall tau-b and tau-c of C score vectors against one vector of human ratings, in one call (kendall.hip): the rank correlation a
 * caption metric is judged by (tau-c on Flickr8k-Expert and Composite, tau-b on Flickr8k-CF).  The reference ships no such evaluation.
 * Inputs
 *   scores: C vectors of n f32, vector c at scores + c ld, ld >= n.  human: n f32 ratings.  All C vectors are correlated with human in
 *   the same pass.
 * Counts
 *   Over the n0 = n (n - 1) / 2 unordered pairs i < j, with IEEE f32 comparisons (-0 == +0, +-inf order normally, a NaN compares false).
 *   out_counts is device int64 [C][8]:
 *     0 con        (x_i - x_j) and (y_i - y_j) have the same non-zero sign
 *     1 dis        they have opposite non-zero signs
 *     2 tie_x      x_i == x_j
 *     3 tie_y      y_i == y_j
 *     4 tie_xy     both
 *     5 distinct_x the number of distinct values in x: an element counts when no earlier element equals it
 *     6 distinct_y the same for y
 *     7 nan        the number of i for which x_i or y_i is a NaN
 *   Without a NaN, con + dis + tie_x + tie_y - tie_xy == n0.  Slots 3 and 6 are the same for every c.
 * Results
 *   out_tau is device f64 [C][2], formed once in double from the integers as scipy.stats.kendalltau defines them (clipped to [-1, 1]):
 *     tau_b = (con - dis) / sqrt(n0 - tie_x) / sqrt(n0 - tie_y), NaN when either factor is 0.  It is evaluated with one root,
 *             (con - dis) / sqrt((n0 - tie_x) (n0 - tie_y)), which makes it exactly 1 for x = y and -1 for x = -y
 *     tau_c = 2 (con - dis) / (n^2 (m - 1) / m) with m = min(distinct_x, distinct_y), NaN when m == 1
 *   Both are NaN for a column whose slot 7 is non-zero.  A NaN in one score vector leaves the other columns as they are; a NaN in human
 *   makes every column NaN.
 * Determinism
 *   Integer counters only, no atomics: the same call gives the same bits.  No n makes the kernels read or write outside their buffers.
 * Limits, refused on the host with a message (DCLIP_EINVAL, nothing launched, nothing written)
 *   2 <= n <= 262144.  1 <= C <= 4.  ld >= n.  Null operands.  scores and human 4-byte, out_tau and out_counts 8-byte, workspace 16-byte
 *   aligned.  A workspace smaller than dclip_kendall_tau_workspace(n, C), which is 0 for a refused shape.
 * Added without a version bump: no existing signature changed.
 */
size_t dclip_kendall_tau_workspace(int64_t n, int64_t C);
int dclip_kendall_tau(const float* scores, int64_t ld, int64_t C, const float* human, int64_t n, double* out_tau, int64_t* out_counts,
                      void* workspace, size_t ws_bytes, void* stream);
/*
 * Spearman rho and Pearson r of C score vectors against one vector of human ratings, in one call (rankcorr.hip): the two coefficients
 * caption-metric work reports instead of, or next to, Kendall tau.  The reference ships no such evaluation.
 * Inputs
 *   As dclip_kendall_tau: scores is C vectors of n f32, vector c at scores + c ld, ld >= n; human is n f32 ratings.  Comparisons are IEEE
 *   f32 comparisons: -0 == +0, +-inf order normally, a NaN compares false to everything.
 * Twice-ranks
 *   For a vector v and item i: L_i = #{j : v_j < v_i}, Q_i = #{j : v_j == v_i} (i itself included), R_i = 2 L_i + Q_i + 1.  R_i is twice
 *   the average rank of scipy.stats.rankdata(v, 'average'), an exact integer; without a NaN, sum_i R_i = n (n + 1).  (A NaN item has
 *   L = Q = 0, so R = 1.)  out_ranks, when given, is device int32 [C + 1][n]: the C score vectors, then the ratings, which are ranked
 *   once and not once per column.
 * Spearman rho
 *   cx_i = Rx_i - (n + 1), cy_i = Ry_i - (n + 1); Sxy = sum cx_i cy_i, Sxx = sum cx_i^2, Syy = sum cy_i^2, all in int64.  Range:
 *   |c_i| <= n <= 2^18 (and |c_i| < 2^18 without a NaN), so every product is at most 2^36 and every sum of n <= 2^18 of them at most
 *   2^54: int64 never overflows and the three sums are exact.  rho = (double)Sxy / (sqrt((double)Sxx) sqrt((double)Syy)), formed once,
 *   by one thread, in double, and clipped to [-1, 1]; it is evaluated with one root, Sxy / sqrt(Sxx Syy), which makes it exactly 1 for
 *   x = y and exactly -1 for reversed ranks and differs from the two-root form in the last bits only.  No floating-point sum occurs
 *   before that line: the same call gives the same bits.  This is scipy.stats.spearmanr (average ranks on ties).
 *   out_sums, when given, is device int64 [C][4]: Sxy, Sxx, Syy, and the number of items i for which x_i or y_i is a NaN.
 * Pearson r
 *   The f32 values are taken to double, which is exact.  Two passes: the means xm = (sum x_i) / n and ym; then sxy = sum (x_i - xm)
 *   (y_i - ym), sxx = sum (x_i - xm)^2, syy = sum (y_i - ym)^2 in double, r = sxy / (sqrt(sxx) sqrt(syy)) (one root, as above), clipped
 *   to [-1, 1].  Every sum has a fixed shape that depends on n alone: per-lane partials in item order, then the wave, then the
 *   workgroup, then one finalizing workgroup.  No atomics: the same call gives the same bits.  Error bound: DESIGN.md section 7.0.
 * Results
 *   out_corr is device f64 [C][2]: rho, r.
 * Degenerate inputs, all decided on the device with nothing waiting
 *   A NaN in a score vector makes that vector's rho and r NaN and leaves the other columns bit for bit as they are without it; a NaN in
 *   human makes every column NaN.  A constant vector (Sxx == 0 or Syy == 0; sxx == 0 or syy == 0) gives rho = r = NaN.  +-inf in a
 *   vector is a legal value for rho (it ranks first or last) and makes r NaN, as SciPy's float arithmetic does.
 * Determinism
 *   Integer counters and fixed-shape sums, no atomics.  No n makes the kernels read or write outside their buffers.
 * Limits, refused on the host with a message (DCLIP_EINVAL, nothing launched, nothing written)
 *   2 <= n <= 262144.  1 <= C <= 4.  ld >= n.  Null scores, human, out_corr or workspace (out_sums and out_ranks may be null).  scores,
 *   human and out_ranks 4-byte, out_corr and out_sums 8-byte, workspace 16-byte aligned.  A workspace smaller than
 *   dclip_rank_correlation_workspace(n, C), which is 0 for a refused shape.
 * Out of scope: p-values and confidence intervals, weighted variants, n > 262144, sharing one pair walk with dclip_kendall_tau.
 * Added without a version bump: no existing signature changed.
 */
size_t dclip_rank_correlation_workspace(int64_t n, int64_t C);
int dclip_rank_correlation(const float* scores, int64_t ld, int64_t C, const float* human, int64_t n, double* out_corr, int64_t* out_sums,
                           int32_t* out_ranks, void* workspace, size_t ws_bytes, void* stream);
/*
 * Row block of the same loss for data-parallel global negatives (Collective 2): the four inputs are the GATHERED
 * [B, E] embeddings of all ranks, this call owns rows [row0, row0 + rows) — its own samples — against all B columns.
 * d_s_img / d_s_txt: [rows, E] gradients of the owned samples (d global loss / d embedding).  out_scalars: this block's share of
 * every scalar: summing the 16 values over the ranks (one small all-reduce) gives the loss of the concatenated batch.
 * hard_label / soft_label need the softmax statistics of EVERY row (both directions): call once with stats_out (f32 [6, rows]; only the
 * statistics pass runs, no gradients), all-gather the ranks' blocks into [6, B] (statistic-major, rows in rank order), and call again
 * with gathered_stats.  Statistic k of row r is a natural-log log-sum-exp over the B logits of that row (k = 0..2) or column (k = 3..5):
 * log sum_j exp(x_j) for x = S (hard_label), S / tau and T / tau (soft_label); S / T = student / teacher cosine logits, tau = cfg[8].
 * The statistics-only call (stats_out set, gathered_stats null) writes all six rows of stats_out: statistic 0 / 3 is filled when
 * hard_label is enabled, 1, 2, 4, 5 when soft_label is; a statistic of a disabled term is -inf (the empty log-sum-exp) in every
 * element.  It needs two_tower = 1 and at least one cross-modal term (otherwise the pass that writes them does not run: DCLIP_EINVAL),
 * does not write out_scalars, and leaves the owned [rows, E] of d_s_img / d_s_txt unspecified.  With gathered_stats given, stats_out
 * is ignored.
 * Both pointers null: only terms without such statistics (cos_diff, logits_mse, tower terms) may be enabled.
 * Same workspace query (with the gathered B).
 */
int dclip_distill_loss_rows(const float* s_img, const float* t_img, const float* s_txt, const float* t_txt, int64_t B, int64_t E,
                            int64_t row0, int64_t rows, const float* cfg, float* out_scalars, float* d_s_img, float* d_s_txt,
                            const float* gathered_stats, float* stats_out, void* workspace, size_t ws_bytes, void* stream);
/* feature MSE (hidden_rep_mse / embedding_mse: hidden_mse.py:9-17, embed_mse.py:9-10):
 *   loss_acc[0] += coef * mean((s - t)^2) ; ds_acc (nullable) += coef * 2 (s - t) / n */
int dclip_feature_mse(const float* s, const float* t, int64_t n, float coef, float* loss_acc, float* ds_acc, void* stream);
/*
 * Interactive contrastive distillation, forward + backward (the ICL term of CLIP-KD, Yang et al., CVPR 2024): the student's image rows
 * are contrasted against the TEACHER's text rows and the student's text rows against the teacher's image rows.
 *   a, b = rows of s_img, s_txt ; p, q = rows of t_img, t_txt ; x^ = x / |x|, no epsilon (clip_model.py:37-44, as dclip_distill_loss)
 *       A_ij = a^_i . q^_j / tau                 C_ij = b^_i . p^_j / tau
 *       L_i2t = mean_i (lse_j A_ij - A_ii)       L_t2i = mean_i (lse_j C_ij - C_ii)       icl = (L_i2t + L_t2i) / 2
 *   The anchors are the student rows only (row softmaxes, no column direction); the teacher receives no gradient:
 *       P_ij = exp(A_ij - lse_j A_ij) ;  G_i = (sum_j P_ij q^_j - q^_i) / (2 B tau) ;  d a_i = (G_i - a^_i (a^_i . G_i)) / |a_i|
 *   and the same of b with C and p^.  lse is the natural-log log-sum-exp with the row's true maximum.
 *   s_*, t_*   : DEVICE, f32 [B, E], 16-byte aligned.  Limits: 1 <= B <= 4096, E % 16 == 0, 16 <= E <= 1024, tau finite and > 0,
 *                weight finite.
 *   out        : DEVICE, 4 f32, 16-byte aligned: weight * icl, icl, L_i2t, L_t2i.
 *   d_s_img, d_s_txt : DEVICE, f32 [B, E], 16-byte aligned, OVERWRITTEN with weight * d icl / d row.
 *   workspace  : DEVICE, 256-byte aligned, ws_bytes >= dclip_interactive_loss_workspace(B, E) (0 for a refused shape); contents need
 *                not survive between calls.  The [B, B] logits never reach HBM.
 *   Four launches on `stream`.  No atomics, no allocation, no synchronisation, no global state: the same call gives the same bits.
 *   Zero and non-finite rows follow dclip_distill_loss: there is no epsilon, so a zero row normalises to 0 * (1 / 0) = NaN in every
 *   element, and so does a row that holds a NaN or an infinity.  Such a STUDENT row i makes row i of its own gradient NaN in every
 *   element and its direction's L, icl and out[0] NaN; the other rows of that gradient and the other direction stay finite.  Such a
 *   TEACHER row makes every logit of its column NaN: every element of the gradient that is contrasted against it (d_s_img for a row of
 *   t_txt, d_s_txt for a row of t_img), that direction's L, icl and out[0] become NaN; the other gradient and the other L stay finite.
 *   Refused on the host with DCLIP_EINVAL, nothing launched, nothing written: B or E outside the limits, tau not finite or <= 0, a
 *   non-finite weight, any null pointer, a misaligned pointer, a workspace smaller than the query.
 *   Added without a version bump: no existing signature changed.
 */
size_t dclip_interactive_loss_workspace(int64_t B, int64_t E);
int dclip_interactive_loss(const float* s_img, const float* t_img, const float* s_txt, const float* t_txt, int64_t B, int64_t E,
                           float tau, float weight, float* out, float* d_s_img, float* d_s_txt, void* workspace, size_t ws_bytes,
                           void* stream);
/*
 * Intra-modal relational KL distillation, forward + backward of ONE tower (the `intra_kl` term; uni-modal distance preservation as in
 * DIME-FM, Sun et al., ICCV 2023): the KL between the teacher's and the student's softmax over the same-modality in-batch similarities.
 *   s_i, t_i = rows of s, t ; x^ = x / |x|, no epsilon (as dclip_interactive_loss).  For j != i (the diagonal is EXCLUDED from every sum):
 *       a_ij = s^_i . s^_j / tau                 b_ij = t^_i . t^_j / tau
 *       lseS_i = log sum_{j != i} exp a_ij       lseT_i = log sum_{j != i} exp b_ij       (natural log, the row's true maximum)
 *       p_ij = exp(a_ij - lseS_i)                q_ij = exp(b_ij - lseT_i)
 *       KL_i = sum_{j != i} q_ij ((b_ij - lseT_i) - (a_ij - lseS_i))                      (from logits and lse, never log of a probability)
 *       intra_kl = tau^2 mean_i KL_i                                                      (batch mean and tau^2; not soft_label's sum)
 *   The teacher receives no gradient.  The student rows are anchors and columns of their symmetric Gram matrix:
 *       M = p - q (zero diagonal) ;  D = weight (tau / B) (M + M^T) ;  G = D s^ ;  d s_i = (G_i - s^_i (s^_i . G_i)) / |s_i|
 *   B = 1 has no column and B = 2 one (p = q = 1): out and d_s are zeros, by construction.
 *   s, t       : DEVICE, f32 [B, E], 16-byte aligned.  Limits: 1 <= B <= 4096, E % 16 == 0, 16 <= E <= 1024, tau finite and > 0,
 *                weight finite.  One tower per call.
 *   out        : DEVICE, 4 f32, 16-byte aligned: weight * intra_kl, intra_kl, mean_i KL_i, +0.
 *   d_s        : DEVICE, f32 [B, E], 16-byte aligned, OVERWRITTEN with weight * d intra_kl / d row.
 *   workspace  : DEVICE, 256-byte aligned, ws_bytes >= dclip_relation_kl_workspace(B, E) (0 for a refused shape); contents need not
 *                survive between calls.  The [B, B] matrices never reach HBM.
 *   Five launches on `stream` (normalise, row statistics per column slice, their merge, gradient stripes, close).  No atomics, no
 *   allocation, no synchronisation, no global state: the same call gives the same bits.
 *   Zero and non-finite rows: there is no epsilon, so a zero row normalises to 0 * (1 / 0) = NaN in every element, and a row that
 *   holds a NaN or an infinity to a row that holds a NaN: every dot product with it is NaN.  With B >= 2 such a row in EITHER matrix makes every element of d_s and out[0..2] NaN: the NaN sits
 *   in a column of every other row's sum, so every row statistic of that matrix is NaN, and every element of D reads one.  out[3] stays
 *   +0.  With B = 1 no statistic is read: out is zeros, and d_s is NaN in every element for such a row of s (0 * NaN in the product with
 *   s^) and zeros for such a row of t.
 *   Refused on the host with DCLIP_EINVAL, nothing launched, nothing written: B or E outside the limits, tau not finite or <= 0, a
 *   non-finite weight, any null pointer, a misaligned pointer, a workspace smaller than the query.
 *   Added without a version bump: no existing signature changed.
 */
size_t dclip_relation_kl_workspace(int64_t B, int64_t E);
int dclip_relation_kl(const float* s, const float* t, int64_t B, int64_t E, float tau, float weight, float* out, float* d_s,
                      void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Tower-level runtime: one call issues the whole launch sequence of an encoder tower on `stream`.
 *   teacher: reference model/component/_common.py:188-221 (VisionTransformer.forward) and
 *            model/component/text_encoder.py:62-92 (TextEncoder.encode_text) — kind 0: frozen, inference only, fp16 residual stream;
 *            kind 2: the same architecture and parameter order as a TRAINABLE tower — the plain ImageEncoder / TextEncoder in the
 *            student role (reference image_encoder.py:16-25,54-59, text_encoder.py:41-47,75-80; their embedding_projection /
 *            hidden_projection linears act on the exported hidden states and stay with the caller) — f32 residual stream, autograd of it;
 *   student: reference model/component/weight_share_model.py:336-372 / :482-512 (forward_features) and autograd of it.
 * The handle is an immutable host-side plan; params / grads / wcache / workspace are caller-owned device buffers, and what a forward
 * left in a workspace is noted in a caller-owned host record that travels with it (dclip_encoder_run below).
 * Threads: the handle is read-only after create, so any number of threads may use one handle at once.  Calls that share a workspace
 * share its record and are the caller's to serialise (they share device buffers, so they already are).
 *
 * Canonical parameter order (arrays of f32 device pointers; names are the reference's state_dict keys):
 *  teacher image : visual.conv1.weight, visual.class_embedding, visual.positional_embedding, visual.ln_pre.{weight,bias},
 *                  per layer i { ln_1.weight, ln_1.bias, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight,
 *                  attn.out_proj.bias, ln_2.weight, ln_2.bias, mlp.c_fc.weight, mlp.c_fc.bias, mlp.c_proj.weight,
 *                  mlp.c_proj.bias }, visual.ln_post.{weight,bias}, visual.proj
 *  teacher text  : token_embedding.weight, positional_embedding, per layer i { same 12 }, ln_final.{weight,bias},
 *                  text_projection
 *  student image : patch_embed.proj.weight, patch_embed.proj.bias, cls_token, pos_embed,
 *                  per block i { attn.qkv.weight, attn.qkv.bias (NULL if absent), attn.proj.weight, attn.proj.bias,
 *                  mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, per repeat r { norm1.instances.r.weight,
 *                  .bias, norm2.instances.r.weight, .bias, attn.conv_l.instances.r.weight, attn.conv_w.instances.r.weight
 *                  (NULL, NULL when head_mix = 0) } }, norm.weight, norm.bias, head.weight, head.bias
 *  student text  : patch_embed.weight, pos_embed   (embed_rank = 0)   or
 *                  patch_embed.0.weight, patch_embed.1.weight, patch_embed.1.bias, pos_embed   (embed_rank > 0),
 *                  then blocks / norm / head as above.
 * `grads` uses the same order; a NULL entry means "frozen, skip" (requires_grad = False).  Gradients ACCUMULATE (+=).
 */
typedef struct dclip_encoder_cfg {
    int32_t kind;        /* 0 teacher (CLIP residual blocks, QuickGELU; frozen), 1 student (weight-shared MiniViT blocks, erf GELU),
                          * 2 CLIP tower that trains (architecture and parameter order of kind 0, workspace / backward of kind 1) */
    int32_t modality;    /* 0 image, 1 text */
    int32_t tokens;      /* N: (resolution / patch)^2 + 1 for images, context_length for text.  1..128; a frozen (kind 0), non-causal
                          * image tower with D / H = 64 may have up to 640 (ViT-B/16: 197, ViT-L/14: 257, at 336 px: 577) */
    int32_t width;       /* D */
    int32_t heads;       /* H (D / H in {32, 64}) */
    int32_t layers;      /* distinct blocks: teacher = transformer layers, student = depth / repeated_times */
    int32_t repeats;     /* repeated_times (teacher: 1) */
    int32_t mlp_dim;     /* int(D * mlp_ratio) */
    int32_t out_dim;     /* E */
    int32_t patch, resolution, in_chans;  /* image only; resolution = height = width of the INPUT images; the patch conv floors
                                           * (grid = resolution / patch: 336 px at patch 32 reads the top-left 320 x 320).
                                           * in_chans * patch^2 must be a multiple of 64, except in a frozen (kind 0) tower, which takes
                                           * any even patch and pads the contraction to the next multiple of 64 (patch 14: 588 -> 640) */
    int32_t vocab, embed_rank;            /* text only; embed_rank = embedding_compression_dim or 0 */
    int32_t head_mix;    /* use_transform: conv_l / conv_w cross-head mixing */
    int32_t causal;      /* CLIP text towers: 1 */
} dclip_encoder_cfg;

typedef struct dclip_encoder dclip_encoder;

dclip_encoder* dclip_encoder_create(const dclip_encoder_cfg* cfg);   /* NULL + last_error_string on a bad configuration */
void dclip_encoder_destroy(dclip_encoder* enc);
int64_t dclip_encoder_num_params(const dclip_encoder* enc);
size_t dclip_encoder_wcache_bytes(const dclip_encoder* enc);
/* the size depends on the tower's attention path (training, head mixing, DCLIP_ATTN_MIX): only the score buffers it reads are reserved */
size_t dclip_encoder_workspace_bytes(const dclip_encoder* enc, int64_t B, int training);
/* refresh the bf16 GEMM-weight cache from the f32 parameters (student: every step; teacher: once) */
int dclip_encoder_prepare(const dclip_encoder* enc, const void* const* params, void* wcache, void* stream);
/* Head-mean attention maps of chosen block executions (ControlOutput.need_attn_score / need_attn_prob of the reference, exported as
 * dclip_attn_maps_fwd computes them).  All arrays are HOST arrays of n entries; every device buffer is caller-owned.
 *   exec[k]            : block-execution index (0 .. layers * repeats - 1) of map k
 *   score[k] / prob[k] : forward, f32 [B, N, N] outputs (array or entries nullable); written right after that execution's score stage
 *   d_score / d_prob   : backward, their gradients (array or entries nullable); added to that execution's dS before dQ / dK are formed.
 *                        Only maps the most recent training forward of the workspace exported (its dclip_encoder_run says which)
 *                        may receive a gradient.
 *   scratch            : backward, dclip_attn_maps_bwd_workspace_bytes(B, heads, tokens) bytes (head-mixing students with d_prob)
 * Refused (DCLIP_EINVAL, nothing launched): an index out of range or, in the forward, above 63 (one bit per execution in the record),
 * maps together with tokens_eff != 0, maps from a tower of more than 128 tokens (the limit of dclip_attn_maps_fwd), a gradient for a map
 * the forward did not export.  maps = NULL or n = 0 exports nothing;
 * workspace sizes do not depend on maps. */
typedef struct dclip_attn_maps {
    int32_t n;
    const int32_t* exec;
    float* const* score;
    float* const* prob;
    const float* const* d_score;
    const float* const* d_prob;
    void* scratch;
    size_t scratch_bytes;
} dclip_attn_maps;
/* What the most recent dclip_encoder_forward left in one workspace.  Host memory, caller-owned, one per workspace;
 * all-zero = "no forward yet".  Opaque: written by the forward, consumed by the backward, read by last_layer_output. */
typedef struct dclip_encoder_run {
    uint32_t flags;        /* bit 0: backward seeds are clear; bit 1: last block execution ran on the picked rows only */
    uint32_t reserved;
    uint64_t score_maps;   /* bit e: the training forward exported the score map of block execution e */
    uint64_t prob_maps;    /* the same for the probability maps */
} dclip_encoder_run;
/* input: image f32 [B,C,res,res] or token ids i64 [B,N].  last_representation: f32 [B,E] (class token / EOT row).
 * run: the workspace's record, written whole when the call has issued everything (an inference forward notes the pruned bit only).
 * patches (image towers only; nullable): replaces `input` with patch rows the caller has already cut, bf16 [B*N, C*patch*patch] from
 * dclip_im2row(..., cls_rows = 1), 16-byte aligned.  Teacher and student see the same image batch (reference
 * dual_distill_model.py:107-109, distil_model.py forward) and, when their patch size and resolution agree, the same conv1 /
 * PatchEmbed unfolding (_common.py:196-198, weight_share_model.py:344): one conversion then serves both towers.  input may then be
 * NULL (not both); patches are refused on text towers, together with tokens_eff != 0, and on a tower that pads its patch rows
 * (a frozen tower whose in_chans * patch^2 is not a multiple of 64: it cuts its own rows with dclip_im2row_ld).
 * training = 1 keeps every activation backward needs inside `workspace` (kinds 1 and 2).
 * rep_out (nullable array of layers*repeats nullable f32 [B*N, D] pointers) / emb_out (nullable f32 [B*N, D]) receive the hidden
 * state after each block execution and the post-positional-embedding tokens (ControlOutput.need_rep / need_emb of the
 * reference, _loss.py:100-116); d_rep / d_emb are the matching gradients, added to the residual-stream gradient in backward.
 * tokens_eff (0 = all): causal text teacher only — run the tower on the first tokens_eff positions of every caption.  The
 * caller guarantees that every caption's EOT lies inside that prefix; positions after it cannot influence the EOT row
 * (causal mask), so last_representation is unchanged.
 * maps (nullable): head-mean attention maps to export, see dclip_attn_maps. */
int dclip_encoder_forward(const dclip_encoder* enc, const void* input, const void* patches, int64_t B, const void* const* params,
                          const void* wcache, void* workspace, size_t ws_bytes, dclip_encoder_run* run, int training,
                          float* last_representation, float* const* rep_out, float* emb_out, int64_t tokens_eff,
                          const dclip_attn_maps* maps, void* stream);
/* last_layer_output (reference output.py:16-35; _common.py:210-215, text_encoder.py:69-72, weight_share_model.py:363-366,
 * :503-506): final norm + projection of EVERY token, f32 [B*N, E], computed on request from the residual stream the most
 * recent dclip_encoder_forward(enc, ..., B, training) left in `workspace` and noted in `run` (tokens_eff must have been 0).  scratch: caller-owned,
 * dclip_encoder_last_layer_output_scratch_bytes(enc, B, training) bytes, 256-byte aligned.  A forward that exported neither the
 * hidden state nor a map of the last block execution runs that execution's out_proj / LN2 / MLP on the class / EOT rows only
 * (DCLIP_PRUNE_LAST=0: on all rows); this call then runs it again on all rows in `scratch`, leaving `workspace` untouched.
 * last_representation is the class-token / EOT row of this tensor. */
size_t dclip_encoder_last_layer_output_scratch_bytes(const dclip_encoder* enc, int64_t B, int training);
int dclip_encoder_last_layer_output(const dclip_encoder* enc, int64_t B, const void* const* params, const void* wcache,
                                    void* workspace, size_t ws_bytes, const dclip_encoder_run* run, int training, void* scratch,
                                    float* out, void* stream);
/* input / patches: what the forward ran on (caller-made patch rows are the patch-embedding wgrad's operand).
 * maps (nullable): gradients of the maps the forward exported, see dclip_attn_maps.
 * on_bucket (nullable): host callback, invoked on the calling thread as soon as every launch that writes gradient bucket
 * `bucket` has been enqueued on `stream` (an event recorded on `stream` inside the callback marks the bucket complete): the
 * data-parallel exchange of that bucket may start while the rest of the backward runs (reference: Lightning DDP's bucketed
 * all-reduce from autograd hooks, config/final_config/l_clip.yaml:56 strategy ddp_find_unused_parameters_false).
 * Buckets complete in index order; see dclip_encoder_grad_bucket.
 * Seeds: the backward starts from a residual-stream gradient accumulator (and one bf16 operand slot) that must be zero.  The training
 * forward clears them at its end (beside the other towers' work) and says so in `run`; the backward consumes that note, and one that does
 * not find it — a second backward on one forward, a retry, a record no forward has written — clears them itself.
 * Either way one call = the gradients of the most recent training forward of that workspace for the given d_*; gradients ACCUMULATE (+=)
 * into `grads` as everywhere.  After a forward that ran its last block execution on the class / EOT rows only (see last_layer_output),
 * d_rep[layers * repeats - 1] and map gradients of that execution are refused (DCLIP_EINVAL). */
typedef void (*dclip_bucket_cb)(void* user, int32_t bucket);
int dclip_encoder_backward(const dclip_encoder* enc, const void* input, const void* patches, int64_t B, const void* const* params,
                           void* const* grads, const void* wcache, void* workspace, size_t ws_bytes, dclip_encoder_run* run,
                           const float* d_last_representation, const float* const* d_rep, const float* d_emb,
                           const dclip_attn_maps* maps, dclip_bucket_cb on_bucket, void* cb_user, void* stream);
/* gradient buckets in completion order: 0 = final norm + head, 1..L = blocks L-1..0, L+1 = embedding parameters; each is the
 * range [first_param, end_param) of the canonical parameter order above. */
int32_t dclip_encoder_num_grad_buckets(const dclip_encoder* enc);
int dclip_encoder_grad_bucket(const dclip_encoder* enc, int32_t bucket, int32_t* first_param, int32_t* end_param);

/* ---------------------------------------------------------------------------------------------------------------
 * Launch trace (profiling only; process-global): between begin and end every GEMM / LayerNorm-forward / loss call is
 * bracketed by HIP events on the stream it is launched on.  trace_end writes (kind, ms, algorithmic flops, algorithmic
 * bytes) per call and returns the number of calls seen.  kind: 0 gemm_nt, 1 gemm_tn_acc, 2 layernorm_fwd, 3 distill_loss,
 * 4 attention family (nt / nn / tn / fused / softmax fwd / softmax bwd), 5 layernorm_bwd. */
int dclip_trace_begin(int64_t max_records);
int64_t dclip_trace_end(int32_t* kind, float* ms, double* flops, double* bytes, int64_t cap);
/* problem sizes of the traced calls so far, 4 ints per record (GEMM: M, N, K, variant bits); call before dclip_trace_end */
int64_t dclip_trace_dims(int32_t* dims, int64_t cap);
/* profiling only (process-global): while `buf` is non-NULL every workgroup of the 256- / 320-row dclip_gemm_nt kernels writes 6
 * uint64 stamps to buf[6 * workgroup ..]: s_memtime at start / first operands landed / main loop done / epilogue done, then
 * s_memrealtime (100 MHz) at start / end (tools/diag/gemm_phases.py).  NULL switches it off. */
int dclip_trace_gemm_stamps(void* buf);
/* same for the head-mixing softmax backward: 8 uint64 per (wave, row iteration < 4): s_memtime at row start / operands in LDS /
 * row sums done / key tiles done / dW_l done (tools/diag/attn_phases.py) */
int dclip_trace_attn_stamps(void* buf);
/* measurement only (bench.py `clock_mhz_during_timed_steps`; process-global): while `buf` is non-NULL, workgroup 0 of every 256- / 320-row
 * dclip_gemm_nt launch writes 4 uint64 — s_memtime (shader cycles) and s_memrealtime (100 MHz) at its start and at its end — to
 * buf[4 * (launch % cap) ..]; shader clock held during that launch = d(memtime) / d(memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS
 * give-back).  One thread of one workgroup per launch: the timed steps are not perturbed (a resident probe wave on a stream of its own
 * cost 1.7 % of the step and was dropped).  Returns the number of launches stamped since the previous call; NULL switches it off. */
int64_t dclip_trace_gemm_clock(void* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DCLIP_H */
