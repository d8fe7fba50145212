// Tower-level runtime: one C call = the whole stream-ordered launch sequence of an encoder tower.
//
//   CLIP tower (kind 0 frozen teacher / kind 2 trainable: the plain ImageEncoder / TextEncoder in the student role, reference
//                           image_encoder.py:23-25,54-59, text_encoder.py:45-47,75-80):
//                           reference model/component/_common.py:188-221 (VisionTransformer.forward),
//                           model/component/text_encoder.py:62-92 (TextEncoder.encode_text)
//   student (weight-shared MiniViT blocks): reference model/component/weight_share_model.py:336-372, :482-512
//                           (forward_features), :199-218 (RepeatedMiniBlock), :179-185 (MiniBlock), :88-140 (MiniAttention)
//
// The handle is a read-only plan (shapes + workspace/weight-cache offsets).  Everything else is owned by the caller:
//   params / grads : arrays of f32 device pointers in the canonical order documented in include/dclip.h
//   wcache         : bf16 copies of the GEMM weights (W and, for the student, W^T for dgrad), refreshed by _prepare
//   workspace      : activations; in training mode everything backward needs stays resident between the two calls
//   run            : host record of what the last forward left in that workspace (dclip_encoder_run)
// No device allocation (the host-side std::vectors below are per-call scratch), no synchronisation, no global state: safe to call
// from the autograd thread and capturable in a hipGraph.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "common.h"

namespace {

#define CK(expr)                      \
    do {                              \
        int _rc = (expr);             \
        if (_rc != DCLIP_OK) return _rc; \
    } while (0)

// canonical parameter order (see include/dclip.h)
enum { P_PER_TBLOCK = 12, P_PER_SBLOCK = 8, P_PER_SREPEAT = 6 };

struct Plan {
    dclip_encoder_cfg c;
    int D, H, hd, N, Np, F, E, L, R;
    int K;                                     // contraction of the embedding GEMM: in_chans * patch^2 (image), embed_rank (compressed text), else 0
    int Kp;                                    // its width in memory (rows of w.patches and of the cached weight): K, or round_up(K, 64) with zero
                                               // pad columns in both operands for a frozen image tower (patch 14: 588 -> 640)
    bool student, image, compressed;           // student = the weight-shared MiniViT architecture (kind 1)
    bool mixing;                               // conv_l / conv_w cross-head mixing (head_mix; students only)
    bool train;                                // the tower has a backward (kind 1, 2): transposed weights cached, f32 residual stream
    // parameter indices (canonical order, include/dclip.h), -1 = the tower has no such parameter
    struct EmbP { int table, w, bias, cls, pos, ln_w, ln_b; } emb;    // w: the embedding GEMM's weight (patch conv / compressed-text linear);
                                                                      // ln_w / ln_b: ln_pre (CLIP image tower); table: token embedding (text)
    int p_blocks;                              // first block parameter
    struct HeadP { int norm_w, norm_b, head_w, head_b; } head;        // norm / ln_post / ln_final, head / proj / text_projection
    int n_params;
    // weight cache offsets (bf16 elements), -1 = absent
    struct BlockW { int64_t qkv, qkv_t, proj, proj_t, fc1, fc1_t, fc2, fc2_t; };
    std::vector<BlockW> bw;
    int64_t w_embed, w_embed_t, w_head, w_head_t, w_total;
};

int64_t wtake(int64_t& off, int64_t n) { int64_t o = off; off += (n + 127) & ~(int64_t)127; return o; }

bool make_plan(const dclip_encoder_cfg& c, Plan& p) {
    p.c = c;
    p.student = c.kind == 1; p.train = c.kind != 0; p.image = c.modality == 0; p.mixing = p.student && c.head_mix;
    p.D = c.width; p.H = c.heads; p.N = c.tokens; p.F = c.mlp_dim; p.E = c.out_dim; p.L = c.layers; p.R = c.repeats;
    if (c.kind < 0 || c.kind > 2 || c.modality < 0 || c.modality > 1) { dclip_set_error("encoder: bad kind/modality"); return false; }
    if (p.D <= 0 || p.H <= 0 || p.D % p.H) { dclip_set_error("encoder: width %d not divisible by heads %d", p.D, p.H); return false; }
    p.hd = p.D / p.H;
    if (p.hd != 32 && p.hd != 64) { dclip_set_error("encoder: head dim %d unsupported (32 or 64)", p.hd); return false; }
    if (p.D % 64 || p.F % 64 || p.E % 64 || p.D > 1024) { dclip_set_error("encoder: width/mlp/out dims must be multiples of 64, width <= 1024"); return false; }
    // sequences above 128 tokens run dclip_attn_stream_fwd, which exists for the frozen, non-causal, hd = 64 case only
    const bool long_ok = c.kind == 0 && p.image && !c.causal && p.hd == 64;
    if (p.N <= 0 || p.N > (long_ok ? 640 : 128)) {
        if (long_ok) dclip_set_error("encoder: tokens must be in 1..640 for a frozen image tower (got %d)", p.N);
        else if (p.N > 128 && c.kind != 0) dclip_set_error("encoder: tokens must be in 1..128 for a trainable tower (kind %d; got %d): only frozen image towers run longer sequences", c.kind, p.N);
        else if (p.N > 128 && !p.image) dclip_set_error("encoder: tokens must be in 1..128 for a text tower (got %d): only frozen image towers run longer sequences", p.N);
        else if (p.N > 128) dclip_set_error("encoder: tokens must be in 1..128 for a causal or head-dim-%d tower (got %d): longer sequences need a non-causal tower with head dim 64", p.hd, p.N);
        else dclip_set_error("encoder: tokens must be in 1..128 (got %d)", p.N);
        return false;
    }
    if (p.L <= 0 || p.R <= 0 || (!p.student && p.R != 1)) { dclip_set_error("encoder: bad layers/repeats"); return false; }
    p.Np = (p.N + 7) & ~7;
    p.compressed = !p.image && c.embed_rank > 0;
    p.K = p.Kp = 0;
    if (p.image) {
        if (c.patch <= 0 || c.resolution < c.patch || c.in_chans <= 0) { dclip_set_error("encoder: bad patch geometry"); return false; }
        const int g = c.resolution / c.patch;
        if (g * g + 1 != p.N) { dclip_set_error("encoder: tokens %d != (res/patch)^2 + 1 = %d", p.N, g * g + 1); return false; }
        p.K = c.in_chans * c.patch * c.patch;
        p.Kp = p.K;
        if (p.K % 64) {
            if (p.train) { dclip_set_error("encoder: in_chans*patch^2 = %d must be a multiple of 64 in a trainable tower", p.K); return false; }
            if (c.patch % 2) { dclip_set_error("encoder: patch %d must be even", c.patch); return false; }
            p.Kp = (p.K + 63) & ~63;
        }
    } else {
        if (c.vocab <= 0) { dclip_set_error("encoder: vocab required for text"); return false; }
        if (p.compressed && c.embed_rank % 64) { dclip_set_error("encoder: embed_rank must be a multiple of 64"); return false; }
        if (p.compressed && !p.student) { dclip_set_error("encoder: a compressed token embedding exists for the weight-shared student only (kind 1)"); return false; }
        if (p.compressed) p.K = p.Kp = c.embed_rank;
    }
    if (p.mixing && p.H != 2 && p.H != 4 && p.H != 8 && p.H != 12 && p.H != 24) {
        dclip_set_error("encoder: head count %d unsupported by the head-mixing kernels", p.H); return false;
    }
    // parameter order
    int n = 0;
    Plan::EmbP& em = p.emb;
    em = Plan::EmbP{-1, -1, -1, -1, -1, -1, -1};
    if (p.image) {
        em.w = n++;
        if (p.student) em.bias = n++;
        em.cls = n++; em.pos = n++;
        if (!p.student) { em.ln_w = n++; em.ln_b = n++; }
    } else {
        em.table = n++;
        if (p.compressed) { em.w = n++; em.bias = n++; }
        em.pos = n++;
    }
    p.p_blocks = n;
    n += p.student ? p.L * (P_PER_SBLOCK + p.R * P_PER_SREPEAT) : p.L * P_PER_TBLOCK;
    p.head.norm_w = n++; p.head.norm_b = n++; p.head.head_w = n++;
    p.head.head_b = p.student ? n++ : -1;                         // CLIP towers project without a bias
    p.n_params = n;
    // weight cache
    int64_t off = 0;
    const int64_t D = p.D, F = p.F, E = p.E;
    p.bw.resize(p.L);
    for (int l = 0; l < p.L; ++l) {
        auto& b = p.bw[l];
        b.qkv = wtake(off, 3 * D * D); b.proj = wtake(off, D * D); b.fc1 = wtake(off, F * D); b.fc2 = wtake(off, D * F);
        if (p.train) { b.qkv_t = wtake(off, 3 * D * D); b.proj_t = wtake(off, D * D); b.fc1_t = wtake(off, F * D); b.fc2_t = wtake(off, D * F); }
        else b.qkv_t = b.proj_t = b.fc1_t = b.fc2_t = -1;
    }
    p.w_embed = p.w_embed_t = -1;
    if (em.w >= 0) p.w_embed = wtake(off, D * p.Kp);
    if (p.compressed) p.w_embed_t = wtake(off, D * p.K);          // dgrad towards the token table
    p.w_head = wtake(off, E * D);                                 // [E, D] (CLIP towers: proj^T)
    p.w_head_t = p.train ? wtake(off, E * D) : -1;                // [D, E]
    p.w_total = off;
    return true;
}

// The score stage a tower's attention runs; the workspace layout and both directions' launches follow it.
//   Fused   : inference without head mixing (the frozen teacher): one kernel, no score tensors in HBM.
//   Mix     : head-mixing students whose shape has an instantiation of the register-resident score stage (attention_mix.hip:
//             both head mixes on the matrix pipe).  S, P, dR never reach HBM: the backward recomputes them from qkv and the
//             forward's softmax statistics.
//   Unfused : everything else (training without head mixing, head counts dclip_attn_mix_supported rejects, DCLIP_ATTN_MIX=0):
//             attn_nt -> softmax -> attn_nn with scores and probabilities through HBM.
enum class AttnPath { Fused, Mix, Unfused };
inline AttnPath attn_path(const Plan& p, bool training) {
    static const int mode = [] { const char* e = getenv("DCLIP_ATTN_MIX"); return e ? atoi(e) : 1; }();
    if (!training && !p.mixing) return AttnPath::Fused;
    if (p.mixing && mode != 0 && !p.c.causal && dclip_attn_mix_supported(p.H, p.N, p.hd) != 0) return AttnPath::Mix;
    return AttnPath::Unfused;
}

// ------------------------------------------------------------------------------------------------------------
// workspace layout
// ------------------------------------------------------------------------------------------------------------
struct ExecSave {          // one block execution: its own set per execution in training, one set shared by all in inference
    void* x_mid;           // residual stream after the attention branch: f32 (students), f16 (the frozen teacher)
    float* mean1; float* rstd1; float* mean2; float* rstd2;
    bf16_t *h1, *qkv, *ctx, *h2, *u;
    uint8_t* z;            // gelu'(fc1 pre-activation) as 8-bit fixed point (DCLIP_ACT_GELU_SAVE -> DCLIP_ACT_MULAUX)
    // score stage, [B, H, N, Np]; null where the tower's AttnPath does not read them
    float* S;              // Unfused: raw scores, f32
    bf16_t* P;             // Unfused: probabilities (saved for the backward)
    bf16_t* Rm;            // Mix: mixed probabilities, quad-blocked; Unfused: mixed probabilities (= P without head mixing)
    float* stats;          // Mix: [B, H, N] log-sum-exp rows
};

// score buffers are reserved only on the paths that read them; the others stay null (see ExecSave)
void take_scores(Bump& b, const Plan& p, AttnPath path, int64_t B, int64_t N, int64_t Np, ExecSave& s) {
    const int64_t SN = B * p.H * N * Np;
    const bool unfused = path == AttnPath::Unfused;
    s.S = unfused ? b.take<float>(SN) : nullptr;
    s.P = unfused ? b.take<bf16_t>(SN) : nullptr;
    s.Rm = p.mixing ? b.take<bf16_t>(SN) : s.P;
    s.stats = path == AttnPath::Mix ? b.take<float>(B * p.H * N) : nullptr;
}

// What the row-local half of one block execution (exec_mlp) reads and writes, over `rows` rows:
//   x_mid = xin + proj(ctx) ; xout = x_mid + fc2(act(fc1(LN2(x_mid)))).  The backward reads x_mid, mean2 / rstd2, z and rows of the same set.
struct RowSet {
    bf16_t* ctx;                           // attention output (out_proj operand)
    void *xin, *x_mid, *xout;              // residual in, after the attention branch, out (stream dtype)
    bf16_t *h2, *u;                        // LN2 output (fc1 operand), fc2 operand
    float *mean2, *rstd2; uint8_t* z;      // training, else null: LN2 statistics, saved gelu'
    int64_t rows;
};

struct Work {
    // persistent
    std::vector<void*> X;                  // residual stream: X[0] embedding output .. X[LR]; f32 for students, f16 for the frozen
                                           // teacher (what the reference's `precision: 16` autocast keeps there: _common.py:14-20, :124-125)
    bool h16;
    std::vector<ExecSave> ex;
    bf16_t* patches;                       // image: [M, K] ; compressed text: [M, rank]
    float* tok_table;                      // [N, D]
    int32_t* pick;                         // [B]
    float *meanf, *rstdf;                  // final LN stats [B]
    bf16_t* hf;                            // [B, D]
    // temporaries
    void* x0;                              // CLIP image tower: pre-ln_pre tokens (f16 frozen, f32 trainable)
    float *mean0, *rstd0;                  // ln_pre statistics (trainable CLIP image tower)
    float* G0;                             // gradient of the pre-ln_pre tokens (trainable CLIP image tower)
    float* G; bf16_t* Gb;                  // residual-stream gradient
    // gradients that are wgrad operands keep one slot per repeat: the R executions of a weight-shared block feed ONE
    // wgrad GEMM over R * M rows (half the launches and half the f32 atomic traffic at R = 2)
    bf16_t *gb_f2, *gb_pr;                 // [R][M, D] bf16 residual gradient as seen by fc2 / attn.proj
    bf16_t *dbig, *dh, *dqkv, *dout;       // dbig [R][M, F], dqkv [R][M, 3D]
    bf16_t* dR;                            // Unfused: [B, H, N, Np] gradient of the mixed probabilities
    bf16_t* dS;                            // [B, H, N, Np] gradient of the scaled pre-mix scores (Mix: quad-blocked)
    float* tok_sum; float* demb;           // [N, D] ; compressed: [M, rank] f32
    float* wg_dummy;                       // Mix: [2, H, H] sink for conv_l / conv_w gradients when those parameters are frozen
    float* mix_ws; size_t mix_ws_bytes;    // Mix: per-workgroup weight-gradient partials of dclip_attn_mix_bwd
    void* tn_ws; size_t tn_ws_bytes;       // partial tiles of the 256 x 256 wgrad launches (dclip_gemm_tn_acc)
    // the last block execution run on the B picked rows only (prune_last); where these live is decided in layout()
    RowSet compact;                        // its [B, .] operands: ctx and xin are gathered (dclip_rows_pick) from ctx_full and X[nex - 1]
    bf16_t* ctx_full;                      // the execution's attention output, all M rows, before its picked rows are gathered
    float* Gc;                             // training: [B, D] residual-stream gradient of the compact rows
    AttnPath path;                         // the score stage every buffer above was sized for
    size_t bytes;
};

void layout(const Plan& p, int64_t B, bool training, void* base, Work& w, int64_t N = 0) {
    Bump b(base);
    w = Work{};                            // whatever this tower and mode do not use stays null
    if (N <= 0) N = p.N;
    const int64_t Npad = (N + 7) & ~(int64_t)7;
    const int64_t M = B * N, D = p.D, F = p.F, SN = B * p.H * N * Npad;
    const int nex = p.L * p.R;
    const bool save = p.train && training;
    w.path = attn_path(p, save);
    const bool mix = w.path == AttnPath::Mix, unfused = w.path == AttnPath::Unfused;
    w.X.assign(nex + 1, nullptr);
    w.ex.assign(nex, ExecSave{});
    // teacher / inference: a single ping-pong set reused by every block
    ExecSave shared{};
    void* xs = nullptr;
    w.h16 = !p.train;
    if (!save) {
        xs = w.h16 ? (void*)b.take<_Float16>(M * D) : (void*)b.take<float>(M * D);
        shared.x_mid = xs;   // in-place residual stream
        shared.h1 = b.take<bf16_t>(M * D); shared.qkv = b.take<bf16_t>(M * 3 * D);
        take_scores(b, p, w.path, B, N, Npad, shared);
        shared.ctx = b.take<bf16_t>(M * D); shared.h2 = shared.h1; shared.u = b.take<bf16_t>(M * F);
    }
    for (int e = 0; e <= nex; ++e) w.X[e] = save ? (void*)b.take<float>(M * D) : xs;
    for (int e = 0; e < nex; ++e) {
        if (!save) { w.ex[e] = shared; continue; }
        ExecSave& s = w.ex[e];
        s.x_mid = b.take<float>(M * D);
        s.mean1 = b.take<float>(M); s.rstd1 = b.take<float>(M); s.mean2 = b.take<float>(M); s.rstd2 = b.take<float>(M);
        s.qkv = b.take<bf16_t>(M * 3 * D);
        take_scores(b, p, w.path, B, N, Npad, s);
        s.z = b.take<uint8_t>(M * F);
        if (e % p.R == 0) {
            // the wgrad operands (inputs of the four linears) of a block's R executions lie back to back: [R][M, .]
            bf16_t* h1 = b.take<bf16_t>(p.R * M * D); bf16_t* ctx = b.take<bf16_t>(p.R * M * D);
            bf16_t* h2 = b.take<bf16_t>(p.R * M * D); bf16_t* u = b.take<bf16_t>(p.R * M * F);
            for (int r = 0; r < p.R; ++r) {
                ExecSave& t = w.ex[e + r];
                t.h1 = h1 + r * M * D; t.ctx = ctx + r * M * D; t.h2 = h2 + r * M * D; t.u = u + r * M * F;
            }
        }
    }
    // Compact [B, .] operands of a pruned last execution.  This is the one place that decides where they live; both directions reach
    // them through w.compact only.
    //   training : the first B rows of that execution's own saved buffers and of X[nex].  Its ctx / h2 / u are slot R - 1 of the last
    //              block's [R][M, .] wgrad operands, so those wgrads find the compact rows at the start of that slot and contract over
    //              (R - 1) M + B rows, with no copy.  The gathered input shares X[nex] with the output: out_proj consumes it before
    //              fc2 writes.  The all-row attention output goes to the h2 slot, whose rows B.. a pruned execution does not use.
    //   inference: buffers of their own, so that the shared residual stream keeps X[nex - 1] for last_layer_output.
    {
        const ExecSave& s = w.ex[nex - 1];
        if (save) {
            w.ctx_full = s.h2;
            w.compact = RowSet{s.ctx, w.X[nex], s.x_mid, w.X[nex], s.h2, s.u, s.mean2, s.rstd2, s.z, B};
        } else {
            w.ctx_full = shared.ctx;
            bf16_t* cctx = b.take<bf16_t>(B * D);
            const size_t es = w.h16 ? 2 : 4;
            void* xr = b.take<char>(B * D * es); void* xmc = b.take<char>(B * D * es); void* xoc = b.take<char>(B * D * es);
            w.compact = RowSet{cctx, xr, xmc, xoc, shared.h1, shared.u, nullptr, nullptr, nullptr, B};
        }
        w.Gc = save ? b.take<float>(B * D) : nullptr;
    }
    w.patches = p.emb.w >= 0 ? b.take<bf16_t>(M * p.Kp) : nullptr;
    w.tok_table = b.take<float>((int64_t)N * D);
    w.pick = b.take<int32_t>(B);
    w.meanf = b.take<float>(B); w.rstdf = b.take<float>(B);
    w.hf = b.take<bf16_t>(B * D);
    const bool pre_ln = p.emb.ln_w >= 0, pre = save && pre_ln;        // CLIP image tower
    w.x0 = pre_ln ? (w.h16 ? (void*)b.take<_Float16>(M * D) : (void*)b.take<float>(M * D)) : nullptr;
    w.mean0 = pre ? b.take<float>(M) : nullptr; w.rstd0 = pre ? b.take<float>(M) : nullptr; w.G0 = pre ? b.take<float>(M * D) : nullptr;
    if (save) {
        w.G = b.take<float>(M * D); w.Gb = b.take<bf16_t>(M * D);
        w.gb_f2 = b.take<bf16_t>(p.R * M * D); w.gb_pr = b.take<bf16_t>(p.R * M * D);
        w.dbig = b.take<bf16_t>(p.R * M * F); w.dh = b.take<bf16_t>(M * D); w.dqkv = b.take<bf16_t>(p.R * M * 3 * D);
        w.dR = unfused ? b.take<bf16_t>(SN) : nullptr; w.dS = b.take<bf16_t>(SN); w.dout = b.take<bf16_t>(B * p.E);
        w.tok_sum = b.take<float>((int64_t)N * D);
        w.wg_dummy = mix ? b.take<float>(2 * p.H * p.H) : nullptr;
        w.mix_ws_bytes = mix ? dclip_attn_mix_bwd_workspace_bytes(B, p.H, N) : 0;
        w.mix_ws = w.mix_ws_bytes ? (float*)b.take<char>(w.mix_ws_bytes) : nullptr;
        w.tn_ws_bytes = dclip_gemm_tn_workspace_bytes();
        w.tn_ws = b.take<char>(w.tn_ws_bytes);
        w.demb = p.compressed ? b.take<float>(M * p.K) : nullptr;
    }
    w.bytes = b.off;
}

// the full-row set of block execution ei
inline RowSet full_rows(const Work& w, int ei, int64_t M) {
    const ExecSave& s = w.ex[ei];
    return RowSet{s.ctx, w.X[ei], s.x_mid, w.X[ei + 1], s.h2, s.u, s.mean2, s.rstd2, s.z, M};
}

// parameter i of the canonical order, null for an index the tower does not have (-1)
inline const float* PF(const void* const* params, int i) { return i < 0 ? nullptr : (const float*)params[i]; }

// split count of the wgrad contraction: minimise  rounds(tiles*s / 512 resident workgroups) * work per workgroup
//                                                   + atomic traffic (s * P*Q*4 bytes at ~1.3 TB/s, half hidden)
inline int wsplits(int64_t M, int64_t P, int64_t Q) {
    const double tiles = (double)((P + 127) / 128) * (double)((Q + 127) / 128);
    const int smax = (int)((M + 255) / 256);
    int best = 1;
    double best_t = 1e30;
    for (int s = 1; s <= smax && s <= 64; ++s) {
        const double blocks = tiles * s;
        const double rounds = ceil(blocks / 512.0);
        const double t_mm = rounds * (2.0 * 128 * 128 * ((double)M / s)) / 1.76e12;      // ~900 TF/s shared by 512 workgroups
        const double t_at = 0.5 * s * (double)P * Q * 4.0 / 1.3e12;
        const double t = t_mm + t_at + 2e-6;
        if (t < best_t) { best_t = t; best = s; }
    }
    return best;
}

inline int gemm(const void* A, int64_t lda, const void* Bw, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                const float* bias, int act, const void* aux_in, void* aux_out, const void* res, int64_t ldr, int out_dtype,
                int64_t row_group, const float* rowadd, void* st) {
    return dclip_gemm_nt(A, lda, Bw, ldb, C, ldc, M, N, K, 1.f, bias, act, aux_in, aux_out, res, ldr, out_dtype, row_group, rowadd, nullptr, st);
}

// LayerNorm over rows of the tower's residual stream (f32, or f16 for the frozen teacher)
inline int ln_stream(bool h16, const void* x, int64_t ldx, const int32_t* ridx, const float* g, const float* b, void* y, int64_t ldy, int out_dtype,
                     float* mean, float* rstd, int64_t M, int64_t D, void* st) {
    if (h16) return dclip_layernorm_fwd_f16(x, ldx, ridx, g, b, y, ldy, out_dtype, mean, rstd, M, D, 1e-5f, st);
    return dclip_layernorm_fwd((const float*)x, ldx, ridx, g, b, y, ldy, out_dtype, mean, rstd, M, D, 1e-5f, st);
}

// a [M, D] piece of the residual stream as the f32 tensor the caller asked for (hidden-state / embedding export)
inline int export_stream(bool h16, const void* src, float* dst, int64_t n, void* st) {
    if (h16) return dclip_cast_f16_f32(src, dst, n, st);
    if (hipMemcpyAsync(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)st) != hipSuccess) {
        dclip_set_error("dclip_encoder_forward: hidden-state export failed");
        return DCLIP_ELAUNCH;
    }
    return DCLIP_OK;
}

// The score stage of one block execution, on the path its workspace was laid out for: ctx = attention(qkv).
// wl / ww: the execution's conv_l / conv_w weights (head-mixing students), else null.
// pick (nullable): the execution is pruned and only row pick[b] of each sample's ctx is read afterwards.  The row-tile kernels then form
// that row's 16-query tile alone; R and stats (Mix) and ctx are valid on the tile's rows only, and only row-tile kernels may read them.
int attn_forward(AttnPath path, const Plan& p, const ExecSave& s, const float* wl, const float* ww, int64_t B, int64_t N, const int32_t* pick,
                 void* st) {
    const int64_t D = p.D, H = p.H, hd = p.hd, Np = (N + 7) & ~(int64_t)7;
    const float scale = 1.f / sqrtf((float)hd);
    if (path == AttnPath::Fused) {
        if (N <= 128 && pick) return dclip_attn_fused_fwd_rows(s.qkv, 3 * D, s.ctx, D, B, H, N, hd, scale, p.c.causal, pick, st);
        if (N <= 128) return dclip_attn_fused_fwd(s.qkv, 3 * D, s.ctx, D, B, H, N, hd, scale, p.c.causal, st);
        return dclip_attn_stream_fwd(s.qkv, 3 * D, s.ctx, D, B, H, N, hd, scale, st);      // (make_plan: frozen, non-causal, hd = 64)
    }
    const int blk = path == AttnPath::Mix ? 1 : 0;
    if (path == AttnPath::Mix) {
        if (pick) CK(dclip_attn_mix_fwd_rows(s.qkv, 3 * D, wl, ww, s.Rm, s.stats, B, H, N, Np, hd, scale, pick, st));
        else CK(dclip_attn_mix_fwd(s.qkv, 3 * D, wl, ww, s.Rm, s.stats, B, H, N, Np, hd, scale, st));
    } else {
        CK(dclip_attn_nt(s.qkv, 3 * D, s.qkv + D, 3 * D, s.S, 1, B, H, N, Np, hd, scale, st));
        CK(dclip_attn_softmax_fwd(s.S, wl, ww, wl ? s.P : nullptr, s.Rm, B, H, N, Np, p.c.causal, st));
    }
    if (pick) return dclip_attn_nn_rows(s.Rm, s.qkv + 2 * D, 3 * D, s.ctx, D, B, H, N, Np, hd, 1.f, blk, pick, 0, st);
    return dclip_attn_nn(s.Rm, s.qkv + 2 * D, 3 * D, s.ctx, D, B, H, N, Np, hd, 1.f, blk, st);
}

// Its backward (Mix or Unfused): dqkv from dctx = dO.  gl / gw: the conv_l / conv_w gradients (+=), null when frozen.
// mg: the gradients of this execution's exported head-mean maps (null when it has none), added to dS before dQ / dK are formed.
// pick (nullable): the forward formed the picked tiles only (attn_forward) and dctx is zero outside the picked rows.  Every term the
// row-tile kernels skip is then an exact zero; dQ is zero-filled outside the tiles, dK and dV are written whole.
struct MapGrad { const float* d_score; const float* d_prob; void* scratch; size_t scratch_bytes; };
int attn_backward(AttnPath path, const Plan& p, const ExecSave& s, const Work& w, const float* wl, const float* ww, float* gl, float* gw,
                  const bf16_t* dctx, bf16_t* dqkv, int64_t B, const MapGrad* mg, const int32_t* pick, void* st) {
    const int64_t D = p.D, H = p.H, hd = p.hd, N = p.N, Np = p.Np;
    const float scale = 1.f / sqrtf((float)hd);
    const int blk = path == AttnPath::Mix ? 1 : 0;                // R and dS of the register-resident score stage are quad-blocked
    if (pick) {
        CK(dclip_attn_tn_rows(s.Rm, dctx, D, dqkv + 2 * D, 3 * D, B, H, N, Np, hd, 1.f, blk, pick, st));     // dV = R^T dO
        if (path == AttnPath::Mix) {
            CK(dclip_attn_mix_bwd_rows(s.qkv, 3 * D, dctx, D, wl, ww, s.stats, w.dS, gl ? gl : w.wg_dummy, gw ? gw : w.wg_dummy + H * H,
                                       w.mix_ws, w.mix_ws_bytes, B, H, N, Np, hd, scale, pick, st));
        } else {                                                      // (all rows: these two read nothing a row-tile forward left stale)
            CK(dclip_attn_nt(dctx, D, s.qkv + 2 * D, 3 * D, w.dR, 0, B, H, N, Np, hd, 1.f, st));
            CK(dclip_attn_softmax_bwd(w.dR, s.P, s.S, 0, wl, ww, w.dS, gl, gw, B, H, N, Np, st));
        }
        CK(dclip_attn_nn_rows(w.dS, s.qkv + D, 3 * D, dqkv, 3 * D, B, H, N, Np, hd, scale, blk, pick, 1, st));   // dQ = dS K
        return dclip_attn_tn_rows(w.dS, s.qkv, 3 * D, dqkv + D, 3 * D, B, H, N, Np, hd, scale, blk, pick, st);   // dK = dS^T Q
    }
    CK(dclip_attn_tn(s.Rm, dctx, D, dqkv + 2 * D, 3 * D, B, H, N, Np, hd, 1.f, blk, st));                    // dV = R^T dO
    if (path == AttnPath::Mix) {
        CK(dclip_attn_mix_bwd(s.qkv, 3 * D, dctx, D, wl, ww, s.stats, w.dS, gl ? gl : w.wg_dummy, gw ? gw : w.wg_dummy + H * H,
                              w.mix_ws, w.mix_ws_bytes, B, H, N, Np, hd, scale, st));
    } else {
        CK(dclip_attn_nt(dctx, D, s.qkv + 2 * D, 3 * D, w.dR, 0, B, H, N, Np, hd, 1.f, st));               // dR = dO V^T
        CK(dclip_attn_softmax_bwd(w.dR, s.P, s.S, 0, wl, ww, w.dS, gl, gw, B, H, N, Np, st));
    }
    if (mg) CK(dclip_attn_maps_bwd(s.qkv, 3 * D, wl, mg->d_score, mg->d_prob, w.dS, blk, gl, mg->scratch, mg->scratch_bytes, B, H, N, Np, hd,
                                   scale, p.c.causal, st));
    CK(dclip_attn_nn(w.dS, s.qkv + D, 3 * D, dqkv, 3 * D, B, H, N, Np, hd, scale, blk, st));                 // dQ = dS K
    return dclip_attn_tn(w.dS, s.qkv, 3 * D, dqkv + D, 3 * D, B, H, N, Np, hd, scale, blk, st);              // dK = dS^T Q
}

}  // namespace

// dclip_encoder_run::flags.  The seeds are the residual-gradient accumulator and the last execution's fc2 operand slot (or, after a
// pruned forward, the compact accumulator) that a backward starts from: clear_backward_seeds.
// RUN_PRUNED_ATTN: the pruned execution's attention ran on the picked tiles only, so its backward must read those tiles only.
enum : uint32_t { RUN_SEEDS_CLEAR = 1u, RUN_PRUNED = 2u, RUN_PRUNED_ATTN = 4u };

struct dclip_encoder { Plan p; };

extern "C" dclip_encoder* dclip_encoder_create(const dclip_encoder_cfg* cfg) {
    if (!cfg) { dclip_set_error("dclip_encoder_create: null cfg"); return nullptr; }
    dclip_encoder* e = new (std::nothrow) dclip_encoder();
    if (!e) { dclip_set_error("dclip_encoder_create: out of host memory"); return nullptr; }
    if (!make_plan(*cfg, e->p)) { delete e; return nullptr; }
    return e;
}

extern "C" void dclip_encoder_destroy(dclip_encoder* e) { delete e; }
extern "C" int64_t dclip_encoder_num_params(const dclip_encoder* e) { return e ? e->p.n_params : -1; }
extern "C" size_t dclip_encoder_wcache_bytes(const dclip_encoder* e) { return e ? dclip_up256((size_t)e->p.w_total * 2) : 0; }

extern "C" size_t dclip_encoder_workspace_bytes(const dclip_encoder* e, int64_t B, int training) {
    if (!e || B <= 0) return 0;
    Work w;
    layout(e->p, B, training != 0, nullptr, w);
    return w.bytes;
}

// parameter index helpers -------------------------------------------------------------------------------------
namespace {
// one block execution's parameters under the names the backward uses, for both architectures (CLIP: ln_1/2, in_proj, out_proj, c_fc, c_proj;
// no conv_l / conv_w).  The order inside a block is the canonical one (include/dclip.h).
struct BX { int n1w, n1b, n2w, n2b, qkvw, qkvb, prw, prb, f1w, f1b, f2w, f2b, cl, cw; };
inline BX bexec(const Plan& p, int l, int r) {
    if (!p.student) {       // ln_1, attn.in_proj, attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj: weight, bias each
        const int b = p.p_blocks + l * P_PER_TBLOCK;
        return BX{b, b + 1, b + 6, b + 7, b + 2, b + 3, b + 4, b + 5, b + 8, b + 9, b + 10, b + 11, -1, -1};
    }
    // the block's shared qkv, proj, fc1, fc2 (weight, bias each), then per repeat norm1 w b, norm2 w b, conv_l, conv_w
    const int b = p.p_blocks + l * (P_PER_SBLOCK + p.R * P_PER_SREPEAT), q = b + P_PER_SBLOCK + r * P_PER_SREPEAT;
    return BX{q, q + 1, q + 2, q + 3, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, q + 4, q + 5};
}

// the parameters one block execution's forward reads
struct EP { const float *n1w, *n1b, *n2w, *n2b, *bq, *bp, *b1, *b2, *wl, *ww; };
inline EP exec_params(const Plan& p, const void* const* params, int l, int r) {
    const BX bx = bexec(p, l, r);
    EP e{PF(params, bx.n1w), PF(params, bx.n1b), PF(params, bx.n2w), PF(params, bx.n2b), PF(params, bx.qkvb), PF(params, bx.prb),
         PF(params, bx.f1b), PF(params, bx.f2b), nullptr, nullptr};
    if (p.mixing) { e.wl = PF(params, bx.cl); e.ww = PF(params, bx.cw); }
    return e;
}

// first half of a block execution, on all M rows: LN1 -> QKV -> score stage (s.qkv, s.ctx and the path's saved score tensors)
int exec_attn(const Plan& p, AttnPath path, const ExecSave& s, const bf16_t* W, int l, const EP& e, bool h16, const void* xin, int64_t B,
              int64_t N, const int32_t* pick, void* st) {
    const int64_t D = p.D, M = B * N;
    CK(ln_stream(h16, xin, D, nullptr, e.n1w, e.n1b, s.h1, D, DCLIP_OUT_BF16, s.mean1, s.rstd1, M, D, st));
    CK(gemm(s.h1, D, W + p.bw[l].qkv, D, s.qkv, 3 * D, M, 3 * D, D, e.bq, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
    return attn_forward(path, p, s, e.wl, e.ww, B, N, pick, st);
}

// second half, row-local, on the rows of `rs` (see RowSet): z, if there, receives the saved activation derivative, mean2 / rstd2 the LN2
// statistics
int exec_mlp(const Plan& p, const bf16_t* W, int l, const EP& e, bool h16, const RowSet& rs, void* st) {
    const int64_t D = p.D, F = p.F, rows = rs.rows;
    const auto& bw = p.bw[l];
    const int sdt = h16 ? DCLIP_OUT_F16 : DCLIP_OUT_F32;            // dtype of the residual stream
    const int act = p.student ? (rs.z ? DCLIP_ACT_GELU_SAVE : DCLIP_ACT_GELU) : (rs.z ? DCLIP_ACT_QUICKGELU_SAVE : DCLIP_ACT_QUICKGELU);
    CK(gemm(rs.ctx, D, W + bw.proj, D, rs.x_mid, D, rows, D, D, e.bp, 0, nullptr, nullptr, rs.xin, D, sdt, 0, nullptr, st));
    CK(ln_stream(h16, rs.x_mid, D, nullptr, e.n2w, e.n2b, rs.h2, D, DCLIP_OUT_BF16, rs.mean2, rs.rstd2, rows, D, st));
    CK(gemm(rs.h2, D, W + bw.fc1, D, rs.u, F, rows, F, D, e.b1, act, nullptr, rs.z, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
    return gemm(rs.u, F, W + bw.fc2, F, rs.xout, D, rows, D, F, e.b2, 0, nullptr, nullptr, rs.x_mid, D, sdt, 0, nullptr, st);
}

// Scratch of dclip_encoder_last_layer_output: after a pruned forward it re-runs the last execution on all rows into buffers of its
// own (a pending backward's saved activations stay untouched): t for its attention half, rs (reading the residual xin) for its
// row-local half.  h1 comes first: it is also the bf16 final-LN output, the whole scratch an unpruned forward needs.
size_t llo_scratch(const Plan& p, AttnPath path, bool h16, int64_t B, void* base, void* xin, ExecSave& t, RowSet& rs) {
    Bump b(base);
    const int64_t N = p.N, M = B * N, D = p.D, F = p.F;
    const size_t es = h16 ? 2 : 4;
    t = ExecSave{};
    t.h1 = b.take<bf16_t>(M * D); t.h2 = t.h1;
    t.qkv = b.take<bf16_t>(M * 3 * D);
    take_scores(b, p, path, B, N, p.Np, t);
    t.ctx = b.take<bf16_t>(M * D);
    t.x_mid = b.take<char>(M * D * es);
    t.u = b.take<bf16_t>(M * F);
    rs = RowSet{t.ctx, xin, t.x_mid, b.take<char>(M * D * es), t.h2, t.u, nullptr, nullptr, nullptr, M};
    return b.off;
}

// DCLIP_PRUNE_LAST=0 (read once): every forward runs its last block execution on all rows
inline bool prune_last_enabled() {
    static const int v = [] { const char* e = getenv("DCLIP_PRUNE_LAST"); return e ? atoi(e) : 1; }();
    return v != 0;
}
// DCLIP_PRUNE_ATTN=0 (read once): a pruned last execution still runs its attention on all rows
inline bool prune_attn_enabled() {
    static const int v = [] { const char* e = getenv("DCLIP_PRUNE_ATTN"); return e ? atoi(e) : 1; }();
    return v != 0;
}

// One walk of a dclip_attn_maps descriptor for both directions: its two pointer arrays (forward: the score / prob outputs; backward:
// d_score / d_prob) checked against the plan and spread to one entry per block execution.  The forward (rec = null) also notes what it
// was given as one bit per execution, for the record; the backward passes that record and is refused a gradient for a map not in it.
template <class T> struct ExecMaps { std::vector<T*> score, prob; uint64_t score_bits = 0, prob_bits = 0; };
template <class T>
int exec_maps(const Plan& p, const dclip_attn_maps* maps, T* const* score, T* const* prob, const dclip_encoder_run* rec, const char* fn,
              ExecMaps<T>& out) {
    const int nex = p.L * p.R;
    out.score.assign(nex, nullptr); out.prob.assign(nex, nullptr);
    if (!maps || !maps->n) return DCLIP_OK;
    DCLIP_REQUIRE(maps->n > 0 && maps->exec, "%s: maps need n > 0 execution indices", fn);
    for (int k = 0; k < maps->n; ++k) {
        const int ei = maps->exec[k];
        DCLIP_REQUIRE(ei >= 0 && ei < nex, "%s: map %d: block execution %d out of range 0..%d", fn, k, ei, nex - 1);
        T* sm = score ? score[k] : nullptr;
        T* pm = prob ? prob[k] : nullptr;
        if (!rec) {
            DCLIP_REQUIRE(ei < 64, "%s: map %d: block execution %d: maps are exported for executions 0..63 only", fn, k, ei);
        } else {
            const bool had_s = ei < 64 && (rec->score_maps >> ei & 1), had_p = ei < 64 && (rec->prob_maps >> ei & 1);
            DCLIP_REQUIRE((!sm || had_s) && (!pm || had_p), "%s: a gradient for the %s map of block execution %d, which the forward did not export",
                          fn, sm && !had_s ? "score" : "probability", ei);
        }
        if (sm) { out.score[ei] = sm; out.score_bits |= (uint64_t)1 << ei; }
        if (pm) { out.prob[ei] = pm; out.prob_bits |= (uint64_t)1 << ei; }
    }
    return DCLIP_OK;
}
}  // namespace

extern "C" int dclip_encoder_prepare(const dclip_encoder* e, const void* const* params, void* wcache, void* st) {
    DCLIP_REQUIRE(e && params && wcache, "dclip_encoder_prepare: null argument");
    const Plan& p = e->p;
    bf16_t* W = (bf16_t*)wcache;
    const int64_t D = p.D, F = p.F, E = p.E;
    auto at = [&](int64_t off) -> void* { return off < 0 ? nullptr : (void*)(W + off); };
    // one multi-tensor launch for the whole tower (students refresh their cache every step: 14 / 9 launches became 1)
    std::vector<const float*> src; std::vector<void*> wb, wt; std::vector<int64_t> rr, cc;
    auto job = [&](const float* w, void* b, void* t, int64_t R, int64_t C) { src.push_back(w); wb.push_back(b); wt.push_back(t); rr.push_back(R); cc.push_back(C); };
    for (int l = 0; l < p.L; ++l) {
        const auto& b = p.bw[l];
        const BX bx = bexec(p, l, 0);
        job(PF(params, bx.qkvw), at(b.qkv), at(b.qkv_t), 3 * D, D);
        job(PF(params, bx.prw), at(b.proj), at(b.proj_t), D, D);
        job(PF(params, bx.f1w), at(b.fc1), at(b.fc1_t), F, D);
        job(PF(params, bx.f2w), at(b.fc2), at(b.fc2_t), D, F);
    }
    const bool pad_embed = p.Kp != p.K;                                                       // (frozen patch-14 towers: cast apart, below)
    if (p.emb.w >= 0 && !pad_embed) job(PF(params, p.emb.w), at(p.w_embed), at(p.w_embed_t), D, p.K);       // conv weight [D, C*p*p] / compressed-text linear [D, rank]
    if (p.student) job(PF(params, p.head.head_w), at(p.w_head), at(p.w_head_t), E, D);
    else job(PF(params, p.head.head_w), at(p.w_head_t), at(p.w_head), D, E);                  // proj [D,E] -> [E,D] (+ as it is: the dgrad operand of a trainable tower)
    for (size_t i = 0; i < src.size(); ++i) DCLIP_REQUIRE(src[i], "dclip_encoder_prepare: parameter %zu missing", i);
    if (pad_embed) {
        DCLIP_REQUIRE(PF(params, p.emb.w), "dclip_encoder_prepare: the patch-embedding weight is missing");
        CK(dclip_cast_bf16_pad(PF(params, p.emb.w), at(p.w_embed), D, p.K, p.Kp, st));       // [D, Kp], columns [K, Kp) zero
    }
    return dclip_cast_transpose_bf16_multi(src.data(), wb.data(), wt.data(), rr.data(), cc.data(), (int64_t)src.size(), st);
}

// The backward starts from a residual-stream gradient that is non-zero in B of the M rows (the picked class / EOT rows): its f32
// accumulator and the fc2 operand slot of the last execution start as zeros.  After a pruned forward only the compact [B, D]
// accumulator w.Gc does: the full one is written whole from it (dclip_rows_expand) and the fc2 operand rows are the B compact ones,
// every one of which the final LayerNorm backward writes.  Those fills used to open dclip_encoder_backward, i.e. sat
// on the critical path right after the loss; issued at the end of the training forward, they run on the tower's stream while the other
// towers finish and the loss is evaluated (the buffers are not touched by the forward).  (Round 5: the bf16 copy w.Gb is no longer
// cleared — every row of it is written by the first execution's LayerNorm backward before anything reads it.)
static int clear_backward_seeds(const Plan& p, const Work& w, int64_t M, int64_t B, bool pruned, void* st) {
    const int64_t D = p.D;
    hipStream_t hs = (hipStream_t)st;
    bf16_t* gb_last = w.gb_f2 + (int64_t)(p.R - 1) * M * D;
    const bool ok = pruned ? hipMemsetAsync(w.Gc, 0, (size_t)B * D * 4, hs) == hipSuccess
                           : hipMemsetAsync(w.G, 0, (size_t)M * D * 4, hs) == hipSuccess && hipMemsetAsync(gb_last, 0, (size_t)M * D * 2, hs) == hipSuccess;
    if (!ok) { dclip_set_error("dclip_encoder: clearing the backward seeds failed"); return DCLIP_ELAUNCH; }
    return DCLIP_OK;
}

// patches: the image tower's [B*N, K] bf16 patch rows made by the caller (dclip_im2row, cls_rows = 1) — two towers that
// see the same images and cut them the same way share one conversion; null: this call converts `input` itself
extern "C" int dclip_encoder_forward(const dclip_encoder* e, const void* input, const void* patches, int64_t B, const void* const* params,
                                     const void* wcache, void* workspace, size_t ws_bytes, dclip_encoder_run* run, int training,
                                     float* last_representation, float* const* rep_out, float* emb_out, int64_t tokens_eff,
                                     const dclip_attn_maps* maps, void* st) {
    DCLIP_REQUIRE(e && (input || patches) && params && wcache && workspace && run && last_representation, "dclip_encoder_forward: null argument");
    DCLIP_REQUIRE(B > 0, "dclip_encoder_forward: empty batch");
    const Plan& p = e->p;
    const bf16_t* ext_patches = (const bf16_t*)patches;
    DCLIP_REQUIRE(!ext_patches || (p.image && ((uintptr_t)ext_patches % 16) == 0), "dclip_encoder_forward: patches: image towers only, 16-byte aligned rows");
    DCLIP_REQUIRE(!ext_patches || tokens_eff == 0, "dclip_encoder_forward: patches cannot be combined with tokens_eff");
    DCLIP_REQUIRE(!ext_patches || p.Kp == p.K, "dclip_encoder_forward: this tower pads its patch rows (%d -> %d columns) and cuts them itself: pass the images", p.K, p.Kp);
    DCLIP_REQUIRE(!training || p.train, "dclip_encoder_forward: the frozen teacher tower (kind 0) is inference-only");
    // tokens_eff: causal text teacher only.  Positions after the longest caption's EOT cannot influence any EOT row (causal
    // attention; LN / MLP are per token), so the tower may run on the first tokens_eff positions with identical output.
    DCLIP_REQUIRE(tokens_eff == 0 || (!p.train && !p.image && p.c.causal && tokens_eff > 0 && tokens_eff <= p.N && !rep_out && !emb_out),
                  "dclip_encoder_forward: tokens_eff is only valid for the causal text teacher without hidden-state export");
    // head-mean attention maps per block execution
    DCLIP_REQUIRE(!(maps && maps->n > 0 && maps->exec) || tokens_eff == 0,
                  "dclip_encoder_forward: attention maps cannot be exported from a caption prefix (tokens_eff)");
    DCLIP_REQUIRE(!(maps && maps->n > 0) || p.N <= 128,
                  "dclip_encoder_forward: attention maps cannot be exported from a tower of %d tokens (dclip_attn_maps_fwd / _bwd take N <= 128)", p.N);
    ExecMaps<float> xm;
    CK(exec_maps<float>(p, maps, maps ? maps->score : nullptr, maps ? maps->prob : nullptr, nullptr, "dclip_encoder_forward", xm));
    Work w;
    layout(p, B, training != 0, workspace, w, tokens_eff);
    DCLIP_REQUIRE(ws_bytes >= w.bytes, "dclip_encoder_forward: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    DCLIP_REQUIRE(((uintptr_t)workspace % 256) == 0 && ((uintptr_t)wcache % 256) == 0, "dclip_encoder_forward: buffers must be 256-byte aligned");
    const bf16_t* W = (const bf16_t*)wcache;
    const int64_t N = tokens_eff ? tokens_eff : p.N, D = p.D, F = p.F, E = p.E, M = B * N;
    const int nex = p.L * p.R;

    // ---- embedding -----------------------------------------------------------------------------------------
    // GEMM embeddings (image patches; compressed text): rows [M, K] x weight [D, K], plus a per-token table (pos + cls / bias) added by
    // row group.  The CLIP image tower alone normalises the result (ln_pre) on its way into the stream; plain text is a gather.
    const Plan::EmbP& em = p.emb;
    const bool pre_ln = em.ln_w >= 0;
    const int sdt = w.h16 ? DCLIP_OUT_F16 : DCLIP_OUT_F32;            // dtype of the residual stream
    if (em.w >= 0) {
        const bf16_t* rows = ext_patches ? ext_patches : w.patches;
        if (!p.image) CK(dclip_embed_gather((const int64_t*)input, p.N, PF(params, em.table), nullptr, w.patches, 0, M, N, p.K, st));
        else if (!ext_patches && p.Kp != p.K) CK(dclip_im2row_ld((const float*)input, w.patches, p.Kp, B, p.c.in_chans, p.c.resolution, p.c.patch, 1, st));
        else if (!ext_patches) CK(dclip_im2row((const float*)input, w.patches, B, p.c.in_chans, p.c.resolution, p.c.patch, 1, st));
        CK(dclip_token_table(PF(params, em.pos), PF(params, em.cls), PF(params, em.bias), w.tok_table, N, D, st));
        CK(gemm(rows, p.Kp, W + p.w_embed, p.Kp, pre_ln ? w.x0 : w.X[0], D, M, D, p.Kp, nullptr, 0, nullptr, nullptr, nullptr, 0, sdt, N, w.tok_table, st));
        if (pre_ln) CK(ln_stream(w.h16, w.x0, D, nullptr, PF(params, em.ln_w), PF(params, em.ln_b), w.X[0], D, sdt, w.mean0, w.rstd0, M, D, st));
    } else {
        CK(dclip_embed_gather((const int64_t*)input, p.N, PF(params, em.table), PF(params, em.pos), w.X[0], sdt, M, N, D, st));
    }

    // optional export of the post-positional-embedding tokens (reference ControlOutput.need_emb: _common.py:204-206 captures
    // them BEFORE ln_pre; text_encoder.py:66-67 ; weight_share_model.py:350,490)
    if (emb_out) CK(export_stream(w.h16, pre_ln ? w.x0 : w.X[0], emb_out, M * D, st));

    // ---- blocks --------------------------------------------------------------------------------------------
    // Only the picked token of each sample (class token / EOT = argmax of the ids) leaves the tower, and after the last execution's
    // attention everything is row-local: unless its hidden state or maps are exported, that execution's out_proj, LN2 and MLP run on
    // the B picked rows only, and its attention forms the picked rows' 16-query tiles only (the QKV projection stays on all M rows: the
    // picked queries attend to every key).
    CK(dclip_pick_index(p.image ? nullptr : (const int64_t*)input, p.N, w.pick, B, N, st));
    const bool prune = prune_last_enabled() && !(rep_out && rep_out[nex - 1]) && !xm.score[nex - 1] && !xm.prob[nex - 1];
    const bool prune_attn = prune && prune_attn_enabled() && N <= 128;      // (the streaming forward of longer sequences has no row-tile form)
    for (int ei = 0; ei < nex; ++ei) {
        const int l = ei / p.R, r = ei % p.R;
        const ExecSave& s = w.ex[ei];
        const EP ep = exec_params(p, params, l, r);
        const bool compact = prune && ei == nex - 1;
        ExecSave sa = s;
        if (compact) sa.ctx = w.ctx_full;
        CK(exec_attn(p, w.path, sa, W, l, ep, w.h16, w.X[ei], B, N, compact && prune_attn ? w.pick : nullptr, st));
        // before the next execution reuses the inference set's qkv
        if (xm.score[ei] || xm.prob[ei]) CK(dclip_attn_maps_fwd(s.qkv, 3 * D, ep.wl, xm.score[ei], xm.prob[ei], B, p.H, N, p.hd, 1.f / sqrtf((float)p.hd), p.c.causal, st));
        if (compact) {
            CK(dclip_rows_pick(w.ctx_full, w.compact.ctx, w.pick, B, D * 2, st));
            CK(dclip_rows_pick(w.X[ei], w.compact.xin, w.pick, B, D * (w.h16 ? 2 : 4), st));
        }
        CK(exec_mlp(p, W, l, ep, w.h16, compact ? w.compact : full_rows(w, ei, M), st));
        // optional export of this execution's hidden state (ControlOutput.need_rep: _common.py:156-158, weight_share_model.py:211)
        if (rep_out && rep_out[ei]) CK(export_stream(w.h16, w.X[ei + 1], rep_out[ei], M * D, st));
    }

    // ---- final norm + projection on the picked token only ------------------------------------------------------
    CK(ln_stream(w.h16, prune ? w.compact.xout : w.X[nex], D, prune ? nullptr : w.pick, PF(params, p.head.norm_w), PF(params, p.head.norm_b), w.hf, D,
                 DCLIP_OUT_BF16, w.meanf, w.rstdf, B, D, st));
    CK(gemm(w.hf, D, W + p.w_head, D, last_representation, E, B, E, D, PF(params, p.head.head_b), 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_F32, 0, nullptr, st));
    *run = dclip_encoder_run{(prune ? RUN_PRUNED : 0u) | (prune_attn ? RUN_PRUNED_ATTN : 0u), 0, 0, 0};
    if (training) {
        CK(clear_backward_seeds(p, w, M, B, prune, st));
        run->flags |= RUN_SEEDS_CLEAR;
        run->score_maps = xm.score_bits;
        run->prob_maps = xm.prob_bits;
    }
    return DCLIP_OK;
}

// All-token output of the final norm + projection (reference _common.py:210-215, text_encoder.py:69-72,
// weight_share_model.py:363-366 / :503-506: `last_layer_output`, of which `last_representation` is one row per sample).  The
// training path projects only the picked row; this call produces the whole [B*N, E] tensor on request from the residual
// stream the most recent forward of this tower left in `workspace`.  If that forward ran its last block execution on the picked rows
// only, the execution is run again on all rows from X[nex - 1], in `scratch`, on the same kernels: the result is the one an
// unpruned forward leaves, and nothing a pending backward reads is touched.
extern "C" size_t dclip_encoder_last_layer_output_scratch_bytes(const dclip_encoder* e, int64_t B, int training) {
    if (!e || B <= 0) return 0;
    const Plan& p = e->p;
    ExecSave t;
    RowSet rs;
    return llo_scratch(p, attn_path(p, p.train && training != 0), !p.train, B, nullptr, nullptr, t, rs);
}

extern "C" int dclip_encoder_last_layer_output(const dclip_encoder* e, int64_t B, const void* const* params, const void* wcache,
                                               void* workspace, size_t ws_bytes, const dclip_encoder_run* run, int training, void* scratch,
                                               float* out, void* st) {
    DCLIP_REQUIRE(e && params && wcache && workspace && run && scratch && out, "dclip_encoder_last_layer_output: null argument");
    DCLIP_REQUIRE(B > 0, "dclip_encoder_last_layer_output: empty batch");
    const Plan& p = e->p;
    DCLIP_REQUIRE(!training || p.train, "dclip_encoder_last_layer_output: the frozen teacher tower (kind 0) is inference-only");
    Work w;
    layout(p, B, training != 0, workspace, w);
    DCLIP_REQUIRE(ws_bytes >= w.bytes, "dclip_encoder_last_layer_output: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    const bf16_t* W = (const bf16_t*)wcache;
    const int64_t M = B * p.N, D = p.D, E = p.E;
    const int nex = p.L * p.R;
    const void* xlast = w.X[nex];
    if (run->flags & RUN_PRUNED) {
        ExecSave t;
        RowSet rs;
        const int ei = nex - 1, l = ei / p.R;
        llo_scratch(p, w.path, w.h16, B, scratch, w.X[ei], t, rs);
        const EP ep = exec_params(p, params, l, ei % p.R);
        CK(exec_attn(p, w.path, t, W, l, ep, w.h16, w.X[ei], B, p.N, nullptr, st));
        CK(exec_mlp(p, W, l, ep, w.h16, rs, st));
        xlast = rs.xout;
    }
    CK(ln_stream(w.h16, xlast, D, nullptr, PF(params, p.head.norm_w), PF(params, p.head.norm_b), scratch, D, DCLIP_OUT_BF16, nullptr, nullptr, M, D, st));
    CK(gemm(scratch, D, W + p.w_head, D, out, E, M, E, D, PF(params, p.head.head_b), 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_F32, 0, nullptr, st));
    return DCLIP_OK;
}

// patches: the rows the forward ran on, if the caller made them (they are the patch-embedding wgrad's operand)
extern "C" int dclip_encoder_backward(const dclip_encoder* e, const void* input, const void* patches, int64_t B, const void* const* params,
                                      void* const* grads, const void* wcache, void* workspace, size_t ws_bytes, dclip_encoder_run* run,
                                      const float* d_last_representation, const float* const* d_rep, const float* d_emb,
                                      const dclip_attn_maps* maps, dclip_bucket_cb on_bucket, void* cb_user, void* st) {
    DCLIP_REQUIRE(e && (input || patches) && params && grads && wcache && workspace && run && d_last_representation, "dclip_encoder_backward: null argument");
    const Plan& p = e->p;
    const bf16_t* ext_patches = (const bf16_t*)patches;
    DCLIP_REQUIRE(!ext_patches || p.image, "dclip_encoder_backward: patches: image towers only");
    DCLIP_REQUIRE(p.train, "dclip_encoder_backward: the frozen teacher tower (kind 0) has no backward");
    // gradients of exported head-mean maps, per block execution
    ExecMaps<const float> gm;
    CK(exec_maps<const float>(p, maps, maps ? maps->d_score : nullptr, maps ? maps->d_prob : nullptr, run, "dclip_encoder_backward", gm));
    if (p.mixing && gm.prob_bits) {
        const size_t need = dclip_attn_maps_bwd_workspace_bytes(B, p.H, p.N);
        DCLIP_REQUIRE(maps->scratch && maps->scratch_bytes >= need,
                      "dclip_encoder_backward: probability-map gradients of a head-mixing tower need %zu bytes of maps scratch", need);
    }
    Work w;
    layout(p, B, true, workspace, w);
    DCLIP_REQUIRE(ws_bytes >= w.bytes, "dclip_encoder_backward: workspace too small");
    const bf16_t* W = (const bf16_t*)wcache;
    const int64_t N = p.N, D = p.D, F = p.F, E = p.E, M = B * N;
    const int nex = p.L * p.R;
    // a pruned forward (its last execution on the picked rows only) keeps no hidden state of that execution and exports no map of it
    const bool pruned = (run->flags & RUN_PRUNED) != 0;
    DCLIP_REQUIRE(!pruned || !(d_rep && d_rep[nex - 1]),
                  "dclip_encoder_backward: a gradient for the hidden state of block execution %d, which the forward ran on the class / EOT "
                  "rows only (request that hidden state in the forward, or set DCLIP_PRUNE_LAST=0)", nex - 1);
    DCLIP_REQUIRE(!pruned || !(gm.score[nex - 1] || gm.prob[nex - 1]),
                  "dclip_encoder_backward: a map gradient for block execution %d, which the forward ran on the class / EOT rows only", nex - 1);
    auto GR = [&](int i) -> float* { return i < 0 ? nullptr : (float*)grads[i]; };    // null: frozen, or no such parameter (-1)
    hipStream_t hs = (hipStream_t)st;

    // the seeds were cleared at the end of the training forward of this workspace (clear_backward_seeds) unless a backward has consumed
    // them since: then they are cleared here
    if (run->flags & RUN_SEEDS_CLEAR) run->flags &= ~RUN_SEEDS_CLEAR;
    else CK(clear_backward_seeds(p, w, M, B, pruned, st));
    // ---- head + final norm -----------------------------------------------------------------------------------
    CK(dclip_cast_bf16(d_last_representation, w.dout, B * E, st));
    if (p.student) {         // head = nn.Linear: weight [E, D], bias
        if (GR(p.head.head_w)) CK(dclip_gemm_tn_acc(w.dout, E, w.hf, D, GR(p.head.head_w), D, B, E, D, 1, w.tn_ws, w.tn_ws_bytes, st));
        if (GR(p.head.head_b)) CK(dclip_colsum_acc(w.dout, E, GR(p.head.head_b), B, E, st));
    } else if (GR(p.head.head_w)) {  // x @ proj: proj [D, E], no bias (reference _common.py:213, text_encoder.py:72)
        CK(dclip_gemm_tn_acc(w.hf, D, w.dout, E, GR(p.head.head_w), E, B, D, E, 1, w.tn_ws, w.tn_ws_bytes, st));
    }
    CK(gemm(w.dout, E, W + p.w_head_t, E, w.dh, D, B, D, E, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
    // every LayerNorm backward also emits the column sums of the updated residual gradient = the bias gradient of the
    // linear that wrote into that residual stream (fc2 of the previous execution / attn.proj of this one)
    const int R = p.R;
    bf16_t* gb_last = w.gb_f2 + (int64_t)(R - 1) * M * D;            // fc2 of the last execution reads slot R - 1
    // (pruned: the compact rows of the last execution's output and of its gradient, identity pick)
    CK(dclip_layernorm_bwd(w.dh, D, 0, (const float*)(pruned ? w.compact.xout : w.X[nex]), D, pruned ? nullptr : w.pick, PF(params, p.head.norm_w), w.meanf,
                           w.rstdf, pruned ? w.Gc : w.G, D, gb_last, D, GR(p.head.norm_w), GR(p.head.norm_b), GR(bexec(p, (nex - 1) / p.R, 0).f2b), B, D, st));
    // gradient bucket 0 (final norm + head) is complete: every launch that writes it is enqueued on `st`
    if (on_bucket) on_bucket(cb_user, 0);

    // ---- blocks, last execution first --------------------------------------------------------------------------
    for (int ei = nex - 1; ei >= 0; --ei) {
        const int l = ei / p.R, r = ei % p.R;
        const auto& bw = p.bw[l];
        const ExecSave& s = w.ex[ei];
        const BX bx = bexec(p, l, r);
        const float *wl = nullptr, *ww = nullptr;
        float *gl = nullptr, *gw = nullptr;
        if (p.mixing) { wl = PF(params, bx.cl); ww = PF(params, bx.cw); gl = GR(bx.cl); gw = GR(bx.cw); }
        // this execution's slots; a block's wgrads run once, after its first execution's gradients are there (r == 0)
        bf16_t* gb_f2 = w.gb_f2 + (int64_t)r * M * D;
        bf16_t* gb_pr = w.gb_pr + (int64_t)r * M * D;
        bf16_t* dbig = w.dbig + (int64_t)r * M * F;
        bf16_t* dqkv = w.dqkv + (int64_t)r * M * 3 * D;
        const int64_t MR = (int64_t)R * M;
        const ExecSave& s0 = w.ex[ei - r];                               // execution r = 0 of this block: base of the [R][M, .] operands
        // the row-local half's saved operands: after a pruned forward the last execution's are the B compact rows, and the last block's
        // fc1 / fc2 / out_proj wgrads contract over (R - 1) M + B rows (see layout())
        const bool compact = pruned && ei == nex - 1;
        const RowSet rs = compact ? w.compact : full_rows(w, ei, M);
        const int64_t Mx = rs.rows;
        const int64_t MRw = pruned && l == p.L - 1 ? (int64_t)(R - 1) * M + B : MR;
        // gradient arriving directly at this execution's output (feature-MSE terms): G += d_rep[ei], refresh the bf16 copy
        if (d_rep && d_rep[ei]) CK(dclip_axpy_f32(w.G, d_rep[ei], gb_f2, M * D, GR(bx.f2b), D, st));
        // MLP: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
        CK(dclip_gemm_nt(gb_f2, D, W + bw.fc2_t, D, dbig, F, Mx, F, D, 1.f, nullptr, DCLIP_ACT_MULAUX, rs.z, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr,
                         GR(bx.f1b), st));                                        // dz = (G W2) o gelu'(z) ; db1 += colsum(dz)
        if (r == 0 && GR(bx.f2w)) CK(dclip_gemm_tn_acc(w.gb_f2, D, s0.u, F, GR(bx.f2w), F, MRw, D, F, wsplits(MRw, D, F), w.tn_ws, w.tn_ws_bytes, st));
        if (r == 0 && GR(bx.f1w)) CK(dclip_gemm_tn_acc(w.dbig, F, s0.h2, D, GR(bx.f1w), D, MRw, F, D, wsplits(MRw, F, D), w.tn_ws, w.tn_ws_bytes, st));
        CK(gemm(dbig, F, W + bw.fc1_t, F, w.dh, D, Mx, D, F, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
        CK(dclip_layernorm_bwd(w.dh, D, 0, (const float*)rs.x_mid, D, nullptr, PF(params, bx.n2w), rs.mean2, rs.rstd2, compact ? w.Gc : w.G, D, gb_pr, D,
                               GR(bx.n2w), GR(bx.n2b), GR(bx.prb), Mx, D, st));
        // attention: x_mid = x_in + proj(attn(LN1(x_in)))
        if (r == 0 && GR(bx.prw)) CK(dclip_gemm_tn_acc(w.gb_pr, D, s0.ctx, D, GR(bx.prw), D, MRw, D, D, wsplits(MRw, D, D), w.tn_ws, w.tn_ws_bytes, st));
        bf16_t* dctx = w.dh;
        if (!compact) {
            CK(gemm(gb_pr, D, W + bw.proj_t, D, dctx, D, M, D, D, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
        } else {
            // the compact dctx goes through this execution's dqkv slot (written by the attention backward only after it is read);
            // dctx and the residual-stream gradient are then the full-M tensors, zero outside the picked rows
            bf16_t* dctx_c = dqkv;
            CK(gemm(gb_pr, D, W + bw.proj_t, D, dctx_c, D, B, D, D, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
            CK(dclip_rows_expand(dctx_c, dctx, w.pick, B, N, D * 2, st));
            CK(dclip_rows_expand(w.Gc, w.G, w.pick, B, N, D * 4, st));
        }
        const MapGrad mg{gm.score[ei], gm.prob[ei], maps ? maps->scratch : nullptr, maps ? maps->scratch_bytes : 0};
        CK(attn_backward(w.path, p, s, w, wl, ww, gl, gw, dctx, dqkv, B, mg.d_score || mg.d_prob ? &mg : nullptr,
                         compact && (run->flags & RUN_PRUNED_ATTN) ? w.pick : nullptr, st));
        if (r == 0 && GR(bx.qkvw)) CK(dclip_gemm_tn_acc(w.dqkv, 3 * D, s0.h1, D, GR(bx.qkvw), D, MR, 3 * D, D, wsplits(MR, 3 * D, D), w.tn_ws, w.tn_ws_bytes, st));
        if (r == 0 && params[bx.qkvb] && GR(bx.qkvb)) CK(dclip_colsum_acc(w.dqkv, 3 * D, GR(bx.qkvb), MR, 3 * D, st));
        CK(gemm(dqkv, 3 * D, W + bw.qkv_t, 3 * D, w.dh, D, M, D, 3 * D, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_BF16, 0, nullptr, st));
        // the bf16 residual gradient leaving this execution is the fc2 operand of the previous one (slot of its repeat index)
        bf16_t* gb_next = ei > 0 ? w.gb_f2 + (int64_t)((ei - 1) % R) * M * D : w.Gb;
        CK(dclip_layernorm_bwd(w.dh, D, 0, (const float*)w.X[ei], D, nullptr, PF(params, bx.n1w), s.mean1, s.rstd1, w.G, D, gb_next, D, GR(bx.n1w), GR(bx.n1b),
                               ei > 0 ? GR(bexec(p, (ei - 1) / p.R, 0).f2b) : nullptr, M, D, st));
        // block l's gradients (shared weights: both repeats; its fc2 bias also collects from block l + 1's first LayerNorm
        // backward, which ran earlier) are complete after its first execution's backward: bucket 1 + (L - 1 - l)
        if (r == 0 && on_bucket) on_bucket(cb_user, 1 + (p.L - 1 - l));
    }

    // ---- embedding ---------------------------------------------------------------------------------------------
    const Plan::EmbP& em = p.emb;
    const bool pre_ln = em.ln_w >= 0;                    // CLIP image tower; its exported embedding is taken BEFORE ln_pre (_common.py:204-208)
    if (d_emb && !pre_ln) CK(dclip_axpy_f32(w.G, d_emb, w.Gb, M * D, nullptr, D, st));
    if (hipMemsetAsync(w.tok_sum, 0, (size_t)N * D * 4, hs) != hipSuccess) { dclip_set_error("dclip_encoder_backward: memset failed"); return DCLIP_ELAUNCH; }
    const float* Ge = w.G;                               // f32 gradient of the embedding's output; w.Gb is its bf16 copy
    if (pre_ln) {
        // x = ln_pre(x0), no bypass: the gradient of x0 is LN'(G) alone, accumulated into a cleared buffer
        if (hipMemsetAsync(w.G0, 0, (size_t)M * D * 4, hs) != hipSuccess) { dclip_set_error("dclip_encoder_backward: memset failed"); return DCLIP_ELAUNCH; }
        CK(dclip_layernorm_bwd(w.G, D, 1, (const float*)w.x0, D, nullptr, PF(params, em.ln_w), w.mean0, w.rstd0, w.G0, D, w.Gb, D, GR(em.ln_w), GR(em.ln_b),
                               nullptr, M, D, st));
        if (d_emb) CK(dclip_axpy_f32(w.G0, d_emb, w.Gb, M * D, nullptr, D, st));
        Ge = w.G0;
    }
    if (em.w >= 0) {         // GEMM embedding: weight, then the token table's parts (pos, cls, bias), then the compressed-text token table
        const int64_t K = p.K;
        const bf16_t* rows = ext_patches ? ext_patches : w.patches;
        if (GR(em.w)) CK(dclip_gemm_tn_acc(w.Gb, D, rows, K, GR(em.w), K, M, D, K, wsplits(M, D, K), w.tn_ws, w.tn_ws_bytes, st));
        if (GR(em.bias) || GR(em.cls) || GR(em.pos)) {
            CK(dclip_batch_sum_acc(Ge, w.tok_sum, B, N, D, st));
            CK(dclip_token_table_bwd(w.tok_sum, GR(em.pos), GR(em.cls), GR(em.bias), N, D, p.image ? 1 : 0, st));
        }
        if (GR(em.table)) {
            CK(gemm(w.Gb, D, W + p.w_embed_t, D, w.demb, K, M, K, D, nullptr, 0, nullptr, nullptr, nullptr, 0, DCLIP_OUT_F32, 0, nullptr, st));
            CK(dclip_embed_scatter_add((const int64_t*)input, w.demb, 1, GR(em.table), M, K, p.c.vocab, st));
        }
    } else {                 // plain text: token table scatter, positional sum
        if (GR(em.table)) CK(dclip_embed_scatter_add((const int64_t*)input, w.G, 1, GR(em.table), M, D, p.c.vocab, st));
        if (GR(em.pos)) {
            CK(dclip_batch_sum_acc(w.G, w.tok_sum, B, N, D, st));
            CK(dclip_token_table_bwd(w.tok_sum, GR(em.pos), nullptr, nullptr, N, D, 0, st));
        }
    }
    if (on_bucket) on_bucket(cb_user, p.L + 1);          // embedding parameters: the last bucket
    return DCLIP_OK;
}

// Gradient buckets in the order the backward completes them (data-parallel exchange, SURVEY.md section 8e Collective 1):
// bucket 0 = final norm + head, 1 .. L = blocks L-1 .. 0, L + 1 = embedding parameters.  Each is a contiguous range of the
// canonical parameter order, hence a contiguous range of a flat gradient buffer laid out in that order.
extern "C" int32_t dclip_encoder_num_grad_buckets(const dclip_encoder* e) { return e ? e->p.L + 2 : -1; }
extern "C" int dclip_encoder_grad_bucket(const dclip_encoder* e, int32_t bucket, int32_t* first_param, int32_t* end_param) {
    DCLIP_REQUIRE(e && first_param && end_param, "dclip_encoder_grad_bucket: null argument");
    const Plan& p = e->p;
    DCLIP_REQUIRE(bucket >= 0 && bucket <= p.L + 1, "dclip_encoder_grad_bucket: bucket %d out of range 0..%d", bucket, p.L + 1);
    const int per_block = p.student ? P_PER_SBLOCK + p.R * P_PER_SREPEAT : P_PER_TBLOCK;
    if (bucket == 0) { *first_param = p.head.norm_w; *end_param = p.n_params; }
    else if (bucket == p.L + 1) { *first_param = 0; *end_param = p.p_blocks; }
    else { const int l = p.L - bucket; *first_param = p.p_blocks + l * per_block; *end_param = *first_param + per_block; }
    return DCLIP_OK;
}
