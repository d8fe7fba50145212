// Attention kernels (gfx950): per-(batch, head) bf16 MFMA products and the two fused forwards built from them.
//
//   reference teacher: model/component/_common.py:73-89   (QK^T / sqrt(hd), + causal mask, softmax, PV)
//   reference student: model/component/weight_share_model.py:101-125
//                      (q *= scale ; QK^T ; conv_l over heads ; softmax ; conv_w over heads ; PV)
//
// The sequences are tiny (N = 50 / 77 / 101) so one wave owns one (b, h) problem and the whole row of scores.
// Three MFMA product shapes cover forward and backward (all v_mfma_f32_16x16x32_bf16, f32 accumulate):
//   NT  C[i,j] = a * sum_d A[i,d] B[j,d]     scores S = QK^T ; dR = dO V^T        (fragments straight from HBM/L2)
//   NN  C[i,d] = a * sum_j A[i,j] B[j,d]     O = R V ; dQ = dS K                  (B through LDS + tr16 reads)
//   TN  C[j,d] = a * sum_i A[i,j] B[i,d]     dV = R^T dO ; dK = dS^T Q            (A and B through LDS + tr16 reads)
// The softmax / head-mix stage between NT and NN is attn_softmax.hip; attn_tiles.h holds what the two files share (NMAX) and
// the output epilogue; tr_frag, shared with the wgrad GEMM too, is in common.h.  The V / B column permutation (wave_stage_perm4), the Q / K fragment load, the S^T exponent step and the P.V step
// are still written out per kernel: hipcc optimises a helper's body before it inlines it and there loses what the kernel knows about
// its arguments (non-negative indices, the lane range), and every helper form tried changed main-loop code or register counts.
//
// Score-like tensors live as [B, H, N, Np] with Np = round_up(N, 8) (16-byte rows); pad columns are zero.
// q/k/v/ctx are token-major: row = b*N + n, column = head*hd + d (+ which*D inside the fused qkv buffer).
#include <stdlib.h>
#include "attn_tiles.h"

namespace {

struct AttnMM {
    const void* A; int64_t lda;      // NT: token-major bf16 ; NN/TN: [B,H,N,Np] bf16 (lda = Np)
    const bf16_t* Bm; int64_t ldb;   // token-major bf16
    void* C; int64_t ldc;            // NT: [B,H,N,Np] (f32 or bf16, ldc = Np) ; NN/TN: token-major bf16
    int B, H, N, Np, hd;
    float alpha;
    int a_blocked;                   // NN/TN: A is quad-blocked [B,H,Np/4,N,4] (attention_mix.hip) instead of row-major [B,H,N,Np]
};

// 8 consecutive columns j0 .. j0 + 7 (j0 % 8 == 0) of row i of a score-like matrix of one (b, h): row-major rows of Np, or the
// quad-blocked layout of the register-resident score stage (element (i, j) at ((j >> 2) * N + i) * 4 + (j & 3)): two 8-byte halves
__device__ __forceinline__ u32x4 load_a8(const bf16_t* A, int64_t lda, int N, int blocked, int i, int j0) {
    if (!blocked) return *(const u32x4*)(A + (int64_t)i * lda + j0);
    const u32x2 lo = *(const u32x2*)(A + ((int64_t)(j0 >> 2) * N + i) * 4);
    const u32x2 hi = *(const u32x2*)(A + ((int64_t)((j0 >> 2) + 1) * N + i) * 4);
    return u32x4{lo[0], lo[1], hi[0], hi[1]};
}

// the 16-row tile of sample b that holds its picked row (pick[b] = b * N + n, dclip_pick_index), held inside the sample
__device__ __forceinline__ int pick_tile(const int32_t* pick, int b, int N) {
    return min(max((pick[b] - b * N) >> 4, 0), (N - 1) >> 4);
}

// ---------------------------------------------------------------------------------------------------------
// NT: one wave per (b,h).  HD = head dim (32 or 64).
// ---------------------------------------------------------------------------------------------------------
template <int HD, bool OUT_F32>
__global__ __launch_bounds__(256) void attn_nt_kernel(AttnMM p) {
    const int lane = threadIdx.x & 63;
    const int prob = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (prob >= p.B * p.H) return;
    const int b = prob / p.H, h = prob % p.H;
    const bf16_t* A = (const bf16_t*)p.A + (int64_t)b * p.N * p.lda + h * HD;
    const bf16_t* Bm = p.Bm + (int64_t)b * p.N * p.ldb + h * HD;
    const int nt = (p.N + 15) >> 4;
    const int fr = lane & 15, fk = (lane >> 4) * 8;
    constexpr int KS = HD / 32;
    constexpr int NTM = 8;                               // N <= 128
    // the B-side fragments (all key tiles) are the same for every query tile: load them once, keep them in registers
    bf16x8 bfr[NTM][KS];
#pragma unroll
    for (int jt = 0; jt < NTM; ++jt)
        if (jt < nt) {
            const int jb = min(jt * 16 + fr, p.N - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bfr[jt][ks] = *(const bf16x8*)(Bm + (int64_t)jb * p.ldb + ks * 32 + fk);
        }
    // every query-tile fragment is requested before the first store: vmcnt retires loads and stores in one in-order queue, so a
    // load issued after a store cannot be waited for without waiting for that store's acknowledgement as well
    bf16x8 afa[NTM][KS];
#pragma unroll
    for (int it = 0; it < NTM; ++it)
        if (it < nt) {
            const int ia = min(it * 16 + fr, p.N - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) afa[it][ks] = *(const bf16x8*)(A + (int64_t)ia * p.lda + ks * 32 + fk);
        }
#pragma unroll
    for (int it = 0; it < NTM; ++it) {
        if (it < nt) {
#pragma unroll
            for (int jt = 0; jt < NTM; ++jt) {
                if (jt < nt) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afa[it][ks], bfr[jt][ks], acc, 0, 0, 0);
                    const int j = jt * 16 + fr;
                    if (j < p.Np) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = it * 16 + (lane >> 4) * 4 + r;
                            if (i < p.N) {
                                const float v = j < p.N ? acc[r] * p.alpha : 0.f;
                                const int64_t o = (((int64_t)b * p.H + h) * p.N + i) * p.ldc + j;
                                if (OUT_F32) ((float*)p.C)[o] = v;
                                else ((bf16_t*)p.C)[o] = f2bf(v);
                            }
                        }
                    }
                }
            }
        }
    }
    // pad columns behind the last 16-key tile (Np > 16 ceil(N / 16), e.g. N = 16, Np = 24: never with Np = round_up(N, 8)) are zero too
    const int wpad = p.Np - nt * 16;
    for (int idx = lane; idx < p.N * wpad; idx += 64) {
        const int64_t o = (((int64_t)b * p.H + h) * p.N + idx / wpad) * p.ldc + nt * 16 + idx % wpad;
        if (OUT_F32) ((float*)p.C)[o] = 0.f;
        else ((bf16_t*)p.C)[o] = f2bf(0.f);
    }
}

// copy tile rows [row0, rows) x 16 DT bf16 columns from global (row stride ld) into a wave's LDS tile (row stride ROWB bytes), zero-
// filling rows >= rows_valid, with the columns permuted in groups of four: group q = DT * g + dt of a row lands at group 4 * dt + g.
// A transposing fragment read of column block dt then hands MFMA row 4 g + r the column (4 DT) g + 4 dt + r, so that in a product
// computed transposed (O^T = V^T P^T) lane (query c, group g) ends up with the 4 DT CONSECUTIVE output columns (4 DT) g .. + 4 DT - 1
// of its query (store_scaled): 16- / 32-byte row-contiguous stores instead of 8-byte pieces on 64 different lines per instruction.
template <int ROWB, int DT>
__device__ __forceinline__ void wave_stage_perm4(const bf16_t* __restrict__ G, int64_t ld, int rows_valid, int rows, char* tile, int lane,
                                                 int row0 = 0) {
    constexpr int cpr = DT * 2;                // 16-byte chunks per row (HD = 16 DT)
    constexpr int BATCH = 8;                   // loads in flight per lane: a load -> write loop pays one HBM round trip per chunk
    const int total = (rows - row0) * cpr;
    for (int base = 0; base < total; base += BATCH * 64) {
        u32x4 v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int idx = base + k * 64 + lane;
            const int r = row0 + idx / cpr, c = idx % cpr;
            v[k] = u32x4{0u, 0u, 0u, 0u};
            if (idx < total && r < rows_valid) v[k] = *(const u32x4*)(G + (int64_t)r * ld + c * 8);
        }
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int idx = base + k * 64 + lane;
            const int r = row0 + idx / cpr, c = idx % cpr;
            const int q0 = 2 * c, q1 = 2 * c + 1;
            const int p0 = 4 * (q0 % DT) + q0 / DT, p1 = 4 * (q1 % DT) + q1 / DT;
            if (idx < total) {
                *(u32x2*)(tile + r * ROWB + p0 * 8) = u32x2{v[k][0], v[k][1]};
                *(u32x2*)(tile + r * ROWB + p1 * 8) = u32x2{v[k][2], v[k][3]};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// NN: C[(b,i), h*HD + d] = alpha * sum_j A[b,h,i,j] * B[(b,j), h*HD + d]
// ---------------------------------------------------------------------------------------------------------
// ROWS: only the 16-row tile that holds row pick[b] of each sample is formed (same fragments, same MFMA order: those rows come out
// bit-equal); with fill_zero the other rows of C are stored as zeros, without it they are left untouched.
template <int HD, bool ROWS = false>
__global__ __launch_bounds__(256) void attn_nn_kernel(AttnMM p, const int32_t* pick, int fill_zero) {
    constexpr int ROWB = HD * 2 + 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nprob = p.B * p.H;
    const int prob = min(blockIdx.x * 4 + wave, nprob - 1);
    const bool live = blockIdx.x * 4 + wave < nprob;
    const int b = prob / p.H, h = prob % p.H;
    const int n32 = (p.N + 31) & ~31;
    char* tile = smem + wave * (n32 * ROWB);        // sized by the padded sequence, not by NMAX: N = 50 fits 6 workgroups per CU instead of 3
    wave_stage_perm4<ROWB, HD / 16>(p.Bm + (int64_t)b * p.N * p.ldb + h * HD, p.ldb, p.N, n32, tile, lane);
    __syncthreads();
    const bf16_t* A = (const bf16_t*)p.A + ((int64_t)b * p.H + h) * p.N * p.lda;
    const int nt = (p.N + 15) >> 4, nks = n32 >> 5;
    const int fr = lane & 15, fk = (lane >> 4) * 8;
    constexpr int DT = HD / 16;
    constexpr int KSM = NMAX / 32;
    bf16x8 af[KSM], afn[KSM];
    auto load_a = [&](int it, bf16x8 (&dst)[KSM]) {
        const int ia = min(it * 16 + fr, p.N - 1);
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks) {
            const int j0 = ks * 32 + fk;
            dst[ks] = (ks < nks && j0 < p.Np) ? __builtin_bit_cast(bf16x8, load_a8(A, p.lda, p.N, p.a_blocked, ia, j0)) : zero_frag();
        }
    };
    const int it0 = ROWS ? pick_tile(pick, b, p.N) : 0, it1 = ROWS ? it0 + 1 : nt;
    load_a(it0, af);
    for (int it = it0; it < it1; ++it) {
        if (it + 1 < it1) load_a(it + 1, afn);
        f32x4 acc[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks) {
            if (ks < nks) {
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    // computed transposed (C^T = B^T A^T; both fragment kinds share one lane layout, so the operands just swap)
                    const bf16x8 bf = tr_frag<ROWB>(tile, ks * 32, d * 16, lane);
                    acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af[ks], acc[d], 0, 0, 0);
                }
            }
        }
        const int i = it * 16 + fr;
        if (live && i < p.N) {
            // lane (query fr, group g) holds the 4 DT consecutive columns from (4 DT) g (wave_stage_perm4): 16-byte row-contiguous stores
            store_scaled((bf16_t*)p.C + ((int64_t)b * p.N + i) * p.ldc + h * HD + (lane >> 4) * (4 * DT), acc, p.alpha);
        }
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks) af[ks] = afn[ks];
    }
    if (ROWS && fill_zero && live) {
        // this head's HD columns of every row outside the tile, 16 bytes per lane
        constexpr int CPR = HD / 8;
        for (int idx = lane; idx < p.N * CPR; idx += 64) {
            const int i = idx / CPR, c = idx - i * CPR;
            if ((i >> 4) != it0) *(u32x4*)((bf16_t*)p.C + ((int64_t)b * p.N + i) * p.ldc + h * HD + c * 8) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Fused multi-head attention forward (no head mixing: the frozen CLIP teacher, reference _common.py:73-89):
//   ctx[(b,i), h*HD + d] = sum_j softmax_j(scale * q_i . k_j (+ causal mask)) v_j[d]
// One wave per (b, h).  Everything is computed transposed so that the query index sits on the lane:
//   S^T tile = mfma(K frag, Q frag)  -> a lane holds 4 consecutive keys of ONE query: softmax needs 2 cross-lane steps,
//   P goes to a wave-private LDS tile with 8-byte writes, O^T = V^T P^T (V through LDS + tr16 reads) -> 8-byte stores.
// Scores and probabilities never touch HBM.
// ---------------------------------------------------------------------------------------------------------
struct AttnFused {
    const bf16_t* qkv; int64_t ldq;      // [B*N, 3*H*HD] : q | k | v
    bf16_t* ctx; int64_t ldc;
    int B, H, N, causal;
    float scale;
    int split;                           // waves per (b, h) problem: 1, or 2 that share the V tile and take alternate query tiles
};

// NTM = 16-key tiles the instance holds registers for (4: N <= 64, 5: N <= 80, 7: N <= 112, 8: N <= 128); the K fragments and score tiles
// scale with it, and at NTM = 4 / 5 three waves per SIMD fit where the N = 128 sizing allowed two.
// LDS (round 5): the V and P tiles hold 16 x ceil(N / 16) key rows, not the sequence padded to 32 — an odd number of key tiles ends in
// ONE v_mfma_f32_16x16x16_bf16 step instead of a half-empty 32-key step —, and the launch (dclip_attn_fused_fwd) picks the workgroup
// shape that puts the most waves on a CU.  Evaluated for every N <= 128 and both head sizes it picks one of two shapes only: four
// problems of one wave each for N <= 16 (a single query tile cannot be split), and for every other N four waves as two problems of two
// waves, which share the problem's V tile and take alternate query tiles -- the first candidate already reaches the register cap of
// 12 / 8 waves per CU, and ties go to the split form.  At N = 101 (l_clip at 336 px), hd = 64, that workgroup needs 50 KB (two V tiles
// of 17.5 KB, four P tiles of 3.75 KB: three workgroups per CU) where four one-wave problems at the N = 128 sizing needed 99 KB and left
// ONE workgroup per CU.
// ROWS (launched with split = 1): a problem's wave forms only the query tile that holds row pick[b], as the full kernel forms it.
template <int HD, int NTM, bool ROWS = false>
__global__ __launch_bounds__(256, NTM <= 7 ? 3 : 2) void attn_fused_fwd_kernel(AttnFused p, const int32_t* pick) {
    constexpr int VROWB = HD * 2 + 32;
    constexpr int KS = HD / 32, DT = HD / 16, KSM = (NTM + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6, split = p.split, ppw = nw / split;      // ppw: problems per workgroup
    const int nprob = p.B * p.H;
    const int slot = wave / split, part = wave - slot * split;
    const int prob = min((int)blockIdx.x * ppw + slot, nprob - 1);
    const bool live = (int)blockIdx.x * ppw + slot < nprob;
    const int b = prob / p.H, h = prob % p.H;
    const int D = p.H * HD;
    constexpr bool ODD = (NTM & 1) != 0;              // odd instances serve exactly NTM key tiles: whole 32-key steps + one 16-key step
    const int nt = (p.N + 15) >> 4;
    const int nrows = ODD ? nt * 16 : ((nt + 1) & ~1) * 16, nks = ODD ? nt >> 1 : (nt + 1) >> 1;
    const int prowb = nrows * 2 + 16;
    // LDS: [problems per workgroup] V tiles, then [waves] P tiles
    char* vt = smem + slot * (nrows * VROWB);
    char* pt = smem + ppw * (nrows * VROWB) + wave * (16 * prowb);
    const bf16_t* Q = p.qkv + (int64_t)b * p.N * p.ldq + h * HD;
    const bf16_t* K = Q + D;
    const bf16_t* V = Q + 2 * D;
    const int fr = lane & 15, g = lane >> 4, fk = g * 8;
    bf16x8 kf[NTM][KS];
#pragma unroll
    for (int jt = 0; jt < NTM; ++jt)
        if (jt < nt) {
            const int jb = min(jt * 16 + fr, p.N - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[jt][ks] = *(const bf16x8*)(K + (int64_t)jb * p.ldq + ks * 32 + fk);
        }
    const int it0 = ROWS ? pick_tile(pick, b, p.N) : part, it1 = ROWS ? it0 + 1 : nt;
    bf16x8 qf[KS], qn[KS];
    {
        const int ia = min(it0 * 16 + fr, p.N - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(Q + (int64_t)ia * p.ldq + ks * 32 + fk);
    }
    // V last: its loads join the K / Q requests already in flight, and only its LDS writes wait
    {   // the waves of a problem stage disjoint row ranges of its V tile
        const int per = ((nrows / split) + 15) & ~15;
        wave_stage_perm4<VROWB, DT>(V, p.ldq, p.N, min(nrows, (part + 1) * per), vt, lane, part * per);
    }
    for (int idx = lane; idx < 16 * prowb / 4; idx += 64) ((unsigned*)pt)[idx] = 0u;
    __syncthreads();
    for (int it = it0; it < it1; it += split) {
        if (it + split < it1) {
            const int ia = min((it + split) * 16 + fr, p.N - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) qn[ks] = *(const bf16x8*)(Q + (int64_t)ia * p.ldq + ks * 32 + fk);
        }
        const int i = it * 16 + fr;                         // this lane's query
        // S^T tiles: acc[jt][r] = raw score(query i, key jt*16 + 4g + r); the scale rides in the exponent's fma (scale > 0: the maximum of
        // the raw scores is the maximum of the scaled ones), masked keys are -inf and come out of exp2 as 0, and the probabilities are
        // stored UNNORMALISED (e in [0, 1]: the same relative bf16 precision) with 1 / sum applied to the 4 DT outputs instead of to
        // every one of the N probabilities: 4.5 vector instructions per score element where the first version spent ~10
        f32x4 st[NTM];
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < NTM; ++jt) {
            st[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (jt < nt && (!p.causal || jt <= it)) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) st[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[jt][ks], qf[ks], st[jt], 0, 0, 0);
                if (jt * 16 + 16 > p.N || (p.causal && jt == it)) {        // (wave-uniform: only the last key tile / the diagonal tile mask)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = jt * 16 + g * 4 + r;
                        const bool ok = j < p.N && (!p.causal || j <= i);
                        st[jt][r] = ok ? st[jt][r] : -INFINITY;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, st[jt][r]);
            } else {
                st[jt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float c2 = p.scale * 1.4426950408889634f, nm = -m * c2;      // (key 0 is never masked: m is finite)
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NTM; ++jt)
            if (jt < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __builtin_amdgcn_exp2f(fmaf(st[jt][r], c2, nm));
                    st[jt][r] = e;
                    sum += e;
                }
                *(bf16x4*)(pt + fr * prowb + (jt * 16 + g * 4) * 2) = bf16x4{f2bf(st[jt][0]), f2bf(st[jt][1]), f2bf(st[jt][2]), f2bf(st[jt][3])};
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.f / sum;
        wave_lds_fence();           // (a workgroup-scope fence would also wait for the next tile's query fragments, requested above)
        // O^T[d, i] = sum_j V[j, d] P[i, j]
        f32x4 oc[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) oc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks)
            if (ks < nks && (!p.causal || ks * 32 <= it * 16 + 15)) {
                const bf16x8 pf = *(const bf16x8*)(pt + fr * prowb + (ks * 32 + fk) * 2);
#pragma unroll
                for (int d = 0; d < DT; ++d)
                    oc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<VROWB>(vt, ks * 32, d * 16, lane), pf, oc[d], 0, 0, 0);
            }
        if (ODD && (nt & 1) && (!p.causal || (nt - 1) * 16 <= it * 16 + 15)) {
            // the last, odd key tile: 16 keys, lane (column, g) holds k = 4 g .. 4 g + 3 of both operands
            const int r0 = (nt - 1) * 16;
            const s16x4 pf = *(const s16x4*)(pt + fr * prowb + (r0 + g * 4) * 2);
            const int q4 = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const s16x4 vf = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + (r0 + 4 * g + q4) * VROWB + (d * 16 + 4 * pp) * 2));
                oc[d] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf, pf, oc[d], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (live && i < p.N) {
            // (columns permuted when V was staged: this lane holds the 4 DT consecutive columns from (4 DT) g of query i)
            store_scaled(p.ctx + ((int64_t)b * p.N + i) * p.ldc + h * HD + g * (4 * DT), oc, inv);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Streaming form of the fused forward for sequences the register-resident kernel cannot hold (N > 128: the frozen ViT-B/16,
// ViT-L/14 teachers, 197 / 257 / 577 tokens), non-causal, HD = 64:
//   ctx[(b,i), h*HD + d] = sum_j softmax_j(scale * q_i . k_j) v_j[d]
// A workgroup of four waves owns 64 consecutive queries of one (b, h), 16 per wave, and walks the keys in chunks of SKC = 64.  The four
// waves stage each chunk's K rows (row-major) and V rows (columns permuted as in wave_stage_perm4) once, through registers, into
// one of two LDS buffers: the loads of chunk c + 1 are requested before chunk c is computed and written behind it, one barrier per chunk.
// Per chunk a wave forms S^T = mfma(K frag, Q frag) (lane = query, as in attn_fused_fwd_kernel), moves its running maximum m,
// rescales the O accumulators and its partial row sum by a = exp2((m_old - m) c2), writes the unnormalised e = exp2(fma(s, c2, -m c2))
// as bf16 to its private P tile and adds O^T += V^T P^T.  1 / sum is applied to the 4 DT outputs at the end.  Keys behind N are zero
// rows with score -inf (e = 0); whole 16-key tiles behind N are skipped.  Scores and probabilities never touch HBM.
// Registers: Q 8 + S 16 + O 16 + staging 16 + fragments ~16 VGPRs, far below the 168 of three waves per SIMD.
// LDS: 2 x (64 x 144 K + 64 x 160 V) + 4 x 16 x 144 P = 48 128 bytes: three workgroups (12 waves) per CU of 160 KB.
// ---------------------------------------------------------------------------------------------------------
constexpr int SKC = 64;                        // keys per chunk
constexpr int SQB = 64;                        // queries per workgroup

struct AttnStream {
    const bf16_t* qkv; int64_t ldq;      // [B*N, 3*H*HD] : q | k | v
    bf16_t* ctx; int64_t ldc;
    int B, H, N, nqb;                    // nqb = ceil(N / SQB) workgroups per (b, h)
    float scale;
};

template <int HD>
__global__ __launch_bounds__(256, 3) void attn_stream_fwd_kernel(AttnStream p) {
    constexpr int KROWB = HD * 2 + 16, VROWB = HD * 2 + 32, PROWB = SKC * 2 + 16;
    constexpr int KS = HD / 32, DT = HD / 16, NKT = SKC / 16;
    constexpr int CPR = HD / 8;                         // 16-byte pieces per K / V row
    constexpr int NLD = SKC * CPR / 256;                // pieces per thread and operand of one chunk
    constexpr int KBUF = SKC * KROWB, VBUF = SKC * VROWB;
    __shared__ __attribute__((aligned(16))) char smem[2 * (KBUF + VBUF) + 4 * 16 * PROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int prob = (int)blockIdx.x / p.nqb, qb = (int)blockIdx.x - prob * p.nqb;
    const int b = prob / p.H, h = prob - b * p.H;
    const int D = p.H * HD;
    const bf16_t* Q = p.qkv + (int64_t)b * p.N * p.ldq + h * HD;
    const bf16_t* K = Q + D;
    const bf16_t* V = Q + 2 * D;
    char* pt = smem + 2 * (KBUF + VBUF) + wave * (16 * PROWB);
    const int fr = lane & 15, g = lane >> 4, fk = g * 8;
    const int q0 = qb * SQB + wave * 16;                // this wave's first query
    const bool wave_live = q0 < p.N;                    // (a wave without queries still stages)
    const int i = q0 + fr;                              // this lane's query
    bf16x8 qf[KS];
    {
        const int ia = min(i, p.N - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(Q + (int64_t)ia * p.ldq + ks * 32 + fk);
    }
    u32x4 rk[NLD], rv[NLD];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = k * 256 + tid, r = idx / CPR, c = idx % CPR;
            rk[k] = rv[k] = u32x4{0u, 0u, 0u, 0u};
            if (c0 + r < p.N) {
                rk[k] = *(const u32x4*)(K + (int64_t)(c0 + r) * p.ldq + c * 8);
                rv[k] = *(const u32x4*)(V + (int64_t)(c0 + r) * p.ldq + c * 8);
            }
        }
    };
    auto store_chunk = [&](int buf) {
        char* kt = smem + buf * (KBUF + VBUF);
        char* vt = kt + KBUF;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = k * 256 + tid, r = idx / CPR, c = idx % CPR;
            *(u32x4*)(kt + r * KROWB + c * 16) = rk[k];
            const int g0 = 2 * c, g1 = 2 * c + 1;       // column groups of four, permuted as in wave_stage_perm4
            *(u32x2*)(vt + r * VROWB + (4 * (g0 % DT) + g0 / DT) * 8) = u32x2{rv[k][0], rv[k][1]};
            *(u32x2*)(vt + r * VROWB + (4 * (g1 % DT) + g1 / DT) * 8) = u32x2{rv[k][2], rv[k][3]};
        }
    };
    const int nchunk = (p.N + SKC - 1) / SKC;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const float c2 = p.scale * 1.4426950408889634f;
    float m = -INFINITY, lsum = 0.f;                    // running maximum of the raw scores; this lane's share of the row sum
    f32x4 oc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) oc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch + 1 < nchunk) load_chunk((ch + 1) * SKC);
        if (wave_live) {
            const char* kt = smem + (ch & 1) * (KBUF + VBUF);
            const char* vt = kt + KBUF;
            const int left = p.N - ch * SKC;                        // keys from this chunk's first to the end
            const int nkt = left >= SKC ? NKT : (left + 15) >> 4;   // 16-key tiles with a key in them
            f32x4 st[NKT];
            float mc = m;
#pragma unroll
            for (int jt = 0; jt < NKT; ++jt)
                if (jt < nkt) {
                    st[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    bf16x8 kf[KS];
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        kf[ks] = *(const bf16x8*)(kt + (jt * 16 + fr) * KROWB + (ks * 32 + fk) * 2);
                        st[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[ks], st[jt], 0, 0, 0);
                    }
                    if (jt * 16 + 16 > left) {                      // (wave-uniform: the tile the sequence ends in)
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[jt][r] = jt * 16 + g * 4 + r < left ? st[jt][r] : -INFINITY;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) mc = fmaxf(mc, st[jt][r]);
                    // the K fragments stay live past the VALU work on their tile: hipcc otherwise lets the accumulator share the registers of
                    // the first fragment, and the mask's select then writes a queued MFMA's SrcA registers (common.h)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) mfma_keep_alive(kf[ks]);
                }
            mc = fmaxf(mc, __shfl_xor(mc, 16));
            mc = fmaxf(mc, __shfl_xor(mc, 32));
            // (every chunk has a key: mc is finite.  First chunk: m = -inf and a = 0 meet accumulators that are still 0)
            const float nm = -mc * c2;
            const float a = __builtin_amdgcn_exp2f(fmaf(m, c2, nm));
            m = mc;
            float cs = 0.f;
#pragma unroll
            for (int jt = 0; jt < NKT; ++jt) {
                if (jt < nkt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __builtin_amdgcn_exp2f(fmaf(st[jt][r], c2, nm));
                        st[jt][r] = e;
                        cs += e;
                    }
                    *(bf16x4*)(pt + fr * PROWB + (jt * 16 + g * 4) * 2) = bf16x4{f2bf(st[jt][0]), f2bf(st[jt][1]), f2bf(st[jt][2]), f2bf(st[jt][3])};
                } else if (jt == nkt && (nkt & 1)) {                // upper half of the last 32-key step
                    *(bf16x4*)(pt + fr * PROWB + (jt * 16 + g * 4) * 2) = bf16x4{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
                }
            }
            lsum = fmaf(lsum, a, cs);
#pragma unroll
            for (int d = 0; d < DT; ++d) oc[d] *= a;
            wave_lds_fence();
#pragma unroll
            for (int ks = 0; ks < NKT / 2; ++ks)
                if (ks * 2 < nkt) {
                    const bf16x8 pf = *(const bf16x8*)(pt + fr * PROWB + (ks * 32 + fk) * 2);
#pragma unroll
                    for (int d = 0; d < DT; ++d)
                        oc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<VROWB>(vt, ks * 32, d * 16, lane), pf, oc[d], 0, 0, 0);
                }
            __builtin_amdgcn_wave_barrier();
        }
        if (ch + 1 < nchunk) store_chunk((ch + 1) & 1);
        __syncthreads();
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    const float inv = 1.f / lsum;
    if (wave_live && i < p.N) {
        // (columns permuted when V was staged: this lane holds the 4 DT consecutive columns from (4 DT) g of query i)
        store_scaled(p.ctx + ((int64_t)b * p.N + i) * p.ldc + h * HD + g * (4 * DT), oc, inv);
    }
}

// ---------------------------------------------------------------------------------------------------------
// TN: C[(b,j), h*HD + d] = alpha * sum_i A[b,h,i,j] * B[(b,i), h*HD + d]   (contraction over query rows)
// ---------------------------------------------------------------------------------------------------------

// MAXJ = output row tiles (16 rows each) the instance holds accumulators for: 4 (N <= 64), 5 (N <= 80) or 8 (N <= 128)
// ROWS: the contraction runs over the 16 rows of the tile that holds row pick[b] only: the one 32-row chunk with that tile in it, its
// other half (and rows >= N) staged as zeros for A and B alike, so nothing outside the tile is read.  Every output row is written.
template <int HD, int MAXJ, bool ROWS = false>
__global__ __launch_bounds__(256, MAXJ <= 5 ? 2 : 1) void attn_tn_kernel(AttnMM p, const int32_t* pick) {
    constexpr int BROW = HD * 2 + 32;
    constexpr int DT = HD / 16;
    constexpr int AROW = MAXJ * 32 + 32;            // LDS row of the A chunk [32 x 16 MAXJ] bf16, padded
    constexpr int ACH = 32 * (MAXJ * 2) / 64, BCH = 32 * (HD / 8) / 64;     // 16-byte chunks per lane of a 32-row chunk (A: Np <= 16 MAXJ columns)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nprob = p.B * p.H;
    const int prob = min(blockIdx.x * 4 + wave, nprob - 1);
    const bool live = blockIdx.x * 4 + wave < nprob;
    const int b = prob / p.H, h = prob % p.H;
    char* at = smem + wave * (32 * AROW + 32 * BROW);
    char* bt = at + 32 * AROW;
    const bf16_t* A = (const bf16_t*)p.A + ((int64_t)b * p.H + h) * p.N * p.lda;
    const bf16_t* Bm = p.Bm + (int64_t)b * p.N * p.ldb + h * HD;
    const int ntj = (p.N + 15) >> 4;
    const int nchunk = (p.N + 31) >> 5;
    const int acpr = p.Np >> 3;                       // A: 16-byte chunks per row
    const int itp = ROWS ? pick_tile(pick, b, p.N) : 0;
    const int ch0 = ROWS ? itp >> 1 : 0, ch1 = ROWS ? ch0 + 1 : nchunk;
    auto row_ok = [&](int i) { return i < p.N && (!ROWS || (i >> 4) == itp); };
    f32x4 acc[MAXJ][DT];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
#pragma unroll
        for (int d = 0; d < DT; ++d) acc[j][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    // register-staged pipeline (guide T14): chunk c+1 is loaded into registers before chunk c is consumed, and written to
    // the wave-private LDS tiles afterwards.  Rows >= N are zero (they must not contribute to the contraction).
    u32x4 ra[ACH], rb[BCH];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int k = 0; k < ACH; ++k) {
            // lane -> (row r, 16-byte column chunk c): columns fastest for row-major A, ROWS fastest for the quad-blocked layout, whose
            // 8-byte pieces of consecutive rows are adjacent in memory (16 lanes = 128 contiguous bytes; with the columns fastest every
            // lane of a load touched a line of its own and the texture addresser, not HBM, set the kernel's time)
            const int idx = k * 64 + lane;
            const int r = p.a_blocked ? (idx & 31) : idx / acpr, c = p.a_blocked ? (idx >> 5) : idx - r * acpr;
            ra[k] = u32x4{0u, 0u, 0u, 0u};
            if (r < 32 && c < acpr && row_ok(ch * 32 + r)) ra[k] = load_a8(A, p.lda, p.N, p.a_blocked, ch * 32 + r, c * 8);
        }
#pragma unroll
        for (int k = 0; k < BCH; ++k) {
            const int idx = k * 64 + lane, r = idx / (HD / 8), c = idx % (HD / 8);
            rb[k] = u32x4{0u, 0u, 0u, 0u};
            if (row_ok(ch * 32 + r)) rb[k] = *(const u32x4*)(Bm + (int64_t)(ch * 32 + r) * p.ldb + c * 8);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int k = 0; k < ACH; ++k) {
            const int idx = k * 64 + lane;
            const int r = p.a_blocked ? (idx & 31) : idx / acpr, c = p.a_blocked ? (idx >> 5) : idx - r * acpr;
            if (r < 32 && c < acpr) *(u32x4*)(at + r * AROW + c * 16) = ra[k];
        }
#pragma unroll
        for (int k = 0; k < BCH; ++k) {
            // columns permuted in groups of four as in wave_stage_perm4: the product is computed transposed and a lane ends up with
            // 4 DT consecutive output columns
            const int idx = k * 64 + lane, r = idx / (HD / 8), c = idx % (HD / 8);
            const int q0 = 2 * c, q1 = 2 * c + 1;
            *(u32x2*)(bt + r * BROW + (4 * (q0 % DT) + q0 / DT) * 8) = u32x2{rb[k][0], rb[k][1]};
            *(u32x2*)(bt + r * BROW + (4 * (q1 % DT) + q1 / DT) * 8) = u32x2{rb[k][2], rb[k][3]};
        }
    };
    load_chunk(ch0);
    for (int ch = ch0; ch < ch1; ++ch) {
        __builtin_amdgcn_wave_barrier();
        store_chunk();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (ch + 1 < ch1) load_chunk(ch + 1);
        bf16x8 bf[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) bf[d] = tr_frag<BROW>(bt, 0, d * 16, lane);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            if (j < ntj) {
                // columns beyond Np were never staged: they only feed output rows >= N, which are not stored
                const bf16x8 af = tr_frag<AROW>(at, 0, j * 16, lane);
#pragma unroll
                for (int d = 0; d < DT; ++d)
                    acc[j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[d], af, acc[j][d], 0, 0, 0);      // transposed: lane = output row
            }
        }
    }
    if (live) {
        bf16_t* C = (bf16_t*)p.C + (int64_t)b * p.N * p.ldc + h * HD + (lane >> 4) * (4 * DT);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < ntj) {
                const int jj = j * 16 + (lane & 15);
                if (jj < p.N) store_scaled(C + (int64_t)jj * p.ldc, acc[j], p.alpha);
            }
    }
}

int check_mm(const AttnMM& p, const char* who) {
    DCLIP_REQUIRE(p.A && p.Bm && p.C, "%s: null operand", who);
    DCLIP_REQUIRE(p.B > 0 && p.H > 0 && p.N > 0 && p.N <= NMAX, "%s: need 0 < N <= %d (N=%d)", who, NMAX, p.N);
    DCLIP_REQUIRE(p.hd == 32 || p.hd == 64, "%s: head dim must be 32 or 64 (got %d)", who, p.hd);
    // Np <= NMAX: attn_tn_kernel stages 16 MAXJ <= 128 columns of A per chunk (Np = 136 would leave rows of the chunk unstaged)
    DCLIP_REQUIRE(p.Np % 8 == 0 && p.Np >= p.N && p.Np <= NMAX, "%s: Np must be a multiple of 8, >= N and <= %d (Np=%d)", who, NMAX, p.Np);
    return DCLIP_OK;
}

}  // namespace

extern "C" int dclip_attn_nt(const void* A, int64_t lda, const void* Bm, int64_t ldb, void* C, int out_f32, int64_t B,
                             int64_t H, int64_t N, int64_t Np, int64_t hd, float alpha, void* stream) {
    AttnMM p{A, lda, (const bf16_t*)Bm, ldb, C, Np, (int)B, (int)H, (int)N, (int)Np, (int)hd, alpha, 0};
    if (int rc = check_mm(p, "dclip_attn_nt")) return rc;
    DCLIP_REQUIRE(lda % 8 == 0 && ldb % 8 == 0, "dclip_attn_nt: token-major strides must be multiples of 8");
    TraceScope tr(DCLIP_TRACE_ATTN, 2.0 * B * H * N * N * hd, 4.0 * B * H * N * hd + (out_f32 ? 4.0 : 2.0) * B * H * N * Np, stream, (int)(B * H), (int)N, (int)hd, 1);
    const dim3 grid((unsigned)((B * H + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    if (hd == 32) {
        if (out_f32) hipLaunchKernelGGL((attn_nt_kernel<32, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((attn_nt_kernel<32, false>), grid, dim3(256), 0, st, p);
    } else {
        if (out_f32) hipLaunchKernelGGL((attn_nt_kernel<64, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((attn_nt_kernel<64, false>), grid, dim3(256), 0, st, p);
    }
    return dclip_check_launch("dclip_attn_nt");
}

namespace {

// pick: null = the full product; else the row-tile form (ROWS instances) with one picked row per sample
int launch_nn(const char* who, const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t Np,
              int64_t hd, float alpha, int a_blocked, const int32_t* pick, int fill_zero, void* stream) {
    AttnMM p{A, Np, (const bf16_t*)Bm, ldb, C, ldc, (int)B, (int)H, (int)N, (int)Np, (int)hd, alpha, a_blocked};
    if (int rc = check_mm(p, who)) return rc;
    DCLIP_REQUIRE(ldc % 8 == 0 && ((uintptr_t)C % 16) == 0 && ldb % 8 == 0 && ((uintptr_t)Bm % 16) == 0, "%s: token-major operands must be 16-byte aligned", who);
    const double rows = pick ? 16.0 : (double)N;
    TraceScope tr(DCLIP_TRACE_ATTN, 2.0 * B * H * rows * N * hd, 2.0 * B * H * (N + rows) * hd + 2.0 * B * H * rows * Np, stream, (int)(B * H), (int)N, (int)hd, 2);
    const dim3 grid((unsigned)((B * H + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    const size_t n32 = ((size_t)N + 31) & ~(size_t)31;
    if (hd == 32) {
        if (pick) hipLaunchKernelGGL((attn_nn_kernel<32, true>), grid, dim3(256), 4 * n32 * (32 * 2 + 32), st, p, pick, fill_zero);
        else hipLaunchKernelGGL((attn_nn_kernel<32>), grid, dim3(256), 4 * n32 * (32 * 2 + 32), st, p, nullptr, 0);
    } else {
        if (pick) hipLaunchKernelGGL((attn_nn_kernel<64, true>), grid, dim3(256), 4 * n32 * (64 * 2 + 32), st, p, pick, fill_zero);
        else hipLaunchKernelGGL((attn_nn_kernel<64>), grid, dim3(256), 4 * n32 * (64 * 2 + 32), st, p, nullptr, 0);
    }
    return dclip_check_launch(who);
}

int launch_tn(const char* who, const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t Np,
              int64_t hd, float alpha, int a_blocked, const int32_t* pick, void* stream) {
    AttnMM p{A, Np, (const bf16_t*)Bm, ldb, C, ldc, (int)B, (int)H, (int)N, (int)Np, (int)hd, alpha, a_blocked};
    if (int rc = check_mm(p, who)) return rc;
    DCLIP_REQUIRE(ldc % 8 == 0 && ((uintptr_t)C % 16) == 0 && ldb % 8 == 0 && ((uintptr_t)Bm % 16) == 0, "%s: token-major operands must be 16-byte aligned", who);
    const double rows = pick ? 16.0 : (double)N;
    TraceScope tr(DCLIP_TRACE_ATTN, 2.0 * B * H * rows * N * hd, 2.0 * B * H * (N + rows) * hd + 2.0 * B * H * rows * Np, stream, (int)(B * H), (int)N, (int)hd, 3);
    const dim3 grid((unsigned)((B * H + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    const int ntile = ((int)Np + 15) / 16;
    const int mj = ntile <= 4 ? 4 : (ntile <= 5 ? 5 : 8);
    const size_t lds = (size_t)4 * (32 * (mj * 32 + 32) + 32 * ((int)hd * 2 + 32));
#define TN_LAUNCH(HDv, NTv)                                                                                          \
    do {                                                                                                             \
        if (pick) hipLaunchKernelGGL((attn_tn_kernel<HDv, NTv, true>), grid, dim3(256), lds, st, p, pick);           \
        else hipLaunchKernelGGL((attn_tn_kernel<HDv, NTv>), grid, dim3(256), lds, st, p, nullptr);                   \
    } while (0)
    if (hd == 32) { if (ntile <= 4) TN_LAUNCH(32, 4); else if (ntile <= 5) TN_LAUNCH(32, 5); else TN_LAUNCH(32, 8); }
    else { if (ntile <= 4) TN_LAUNCH(64, 4); else if (ntile <= 5) TN_LAUNCH(64, 5); else TN_LAUNCH(64, 8); }
#undef TN_LAUNCH
    return dclip_check_launch(who);
}

int launch_fused(const char* who, const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd, float scale,
                 int causal, const int32_t* pick, void* stream) {
    DCLIP_REQUIRE(qkv && ctx && B > 0 && H > 0 && N > 0 && N <= NMAX, "%s: bad argument (N <= %d)", who, NMAX);
    DCLIP_REQUIRE(hd == 32 || hd == 64, "%s: head dim must be 32 or 64 (got %ld)", who, (long)hd);
    DCLIP_REQUIRE(ldq % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)ctx % 16) == 0, "%s: misaligned buffers", who);
    AttnFused p{(const bf16_t*)qkv, ldq, (bf16_t*)ctx, ldc, (int)B, (int)H, (int)N, causal, scale, 1};
    const double rows = pick ? 16.0 : (double)N;
    TraceScope tr(DCLIP_TRACE_ATTN, 4.0 * B * H * rows * N * hd, 4.0 * B * H * (N + rows) * hd, stream, (int)(B * H), (int)N, (int)hd, 4);
    hipStream_t st = (hipStream_t)stream;
    const int ntile = ((int)N + 15) / 16;
    // an instance holds registers for NT key tiles; odd tile counts need an instance with the 16-key tail step (NT odd)
    const int NT = ntile <= 4 ? 4 : (ntile == 5 ? 5 : (ntile == 7 ? 7 : 8));
    const int nrows = (NT & 1) ? ntile * 16 : ((ntile + 1) & ~1) * 16;            // (even instances: whole 32-key steps, zero rows behind N)
    const size_t vtile = (size_t)nrows * (hd * 2 + 32), ptile = 16 * ((size_t)nrows * 2 + 16);
    // workgroup shape: four waves as `ppw` problems of `split` waves each.  split = 2 (two waves share a problem's V tile and take
    // alternate query tiles) wherever there is a second query tile to take.  A search for the shape that puts the most waves on a CU
    // (160 KB of LDS; registers allow 12 / 8 waves: launch bounds; ties to the split form, which also halves the dependent chain of a
    // problem) returns exactly this for every N <= 128 and both head sizes: the four-wave split form already reaches the register cap.
    // Row-tile form: one wave per problem (there is one query tile to take), in workgroups of as many waves as fit 64 KB of LDS.
    int nw = 4;
    const int split = !pick && ntile >= 2 ? 2 : 1;
    while (pick && nw > 1 && nw * (vtile + ptile) > 64 * 1024) nw >>= 1;
    p.split = split;
    const int ppw = nw / split;
    const dim3 grid((unsigned)((B * H + ppw - 1) / ppw));
    const size_t lds = ppw * vtile + (size_t)nw * ptile;
#define FUSED_LAUNCH(HDv, NTv)                                                                                               \
    do {                                                                                                                     \
        if (pick) hipLaunchKernelGGL((attn_fused_fwd_kernel<HDv, NTv, true>), grid, dim3(64 * nw), lds, st, p, pick);        \
        else hipLaunchKernelGGL((attn_fused_fwd_kernel<HDv, NTv>), grid, dim3(64 * nw), lds, st, p, nullptr);                \
    } while (0)
    if (hd == 32) { if (NT == 4) FUSED_LAUNCH(32, 4); else if (NT == 5) FUSED_LAUNCH(32, 5); else if (NT == 7) FUSED_LAUNCH(32, 7); else FUSED_LAUNCH(32, 8); }
    else { if (NT == 4) FUSED_LAUNCH(64, 4); else if (NT == 5) FUSED_LAUNCH(64, 5); else if (NT == 7) FUSED_LAUNCH(64, 7); else FUSED_LAUNCH(64, 8); }
#undef FUSED_LAUNCH
    return dclip_check_launch(who);
}

}  // namespace

extern "C" int dclip_attn_nn(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H,
                             int64_t N, int64_t Np, int64_t hd, float alpha, int a_blocked, void* stream) {
    return launch_nn("dclip_attn_nn", A, Bm, ldb, C, ldc, B, H, N, Np, hd, alpha, a_blocked, nullptr, 0, stream);
}

extern "C" int dclip_attn_tn(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H,
                             int64_t N, int64_t Np, int64_t hd, float alpha, int a_blocked, void* stream) {
    return launch_tn("dclip_attn_tn", A, Bm, ldb, C, ldc, B, H, N, Np, hd, alpha, a_blocked, nullptr, stream);
}

extern "C" int dclip_attn_fused_fwd(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                                    float scale, int causal, void* stream) {
    return launch_fused("dclip_attn_fused_fwd", qkv, ldq, ctx, ldc, B, H, N, hd, scale, causal, nullptr, stream);
}

// Row-tile forms for an execution of which only row pick[b] (= b * N + n, a device array) of each sample is read afterwards: the
// products are formed for the 16-row tile that holds that row alone, by the instructions and operands of the full kernels.
extern "C" int dclip_attn_nn_rows(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N,
                                  int64_t Np, int64_t hd, float alpha, int a_blocked, const int32_t* pick, int fill_zero, void* stream) {
    DCLIP_REQUIRE(pick, "dclip_attn_nn_rows: null pick");
    return launch_nn("dclip_attn_nn_rows", A, Bm, ldb, C, ldc, B, H, N, Np, hd, alpha, a_blocked, pick, fill_zero, stream);
}

extern "C" int dclip_attn_tn_rows(const void* A, const void* Bm, int64_t ldb, void* C, int64_t ldc, int64_t B, int64_t H, int64_t N,
                                  int64_t Np, int64_t hd, float alpha, int a_blocked, const int32_t* pick, void* stream) {
    DCLIP_REQUIRE(pick, "dclip_attn_tn_rows: null pick");
    return launch_tn("dclip_attn_tn_rows", A, Bm, ldb, C, ldc, B, H, N, Np, hd, alpha, a_blocked, pick, stream);
}

extern "C" int dclip_attn_fused_fwd_rows(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                                         float scale, int causal, const int32_t* pick, void* stream) {
    DCLIP_REQUIRE(pick, "dclip_attn_fused_fwd_rows: null pick");
    return launch_fused("dclip_attn_fused_fwd_rows", qkv, ldq, ctx, ldc, B, H, N, hd, scale, causal, pick, stream);
}

// Long-sequence companion of dclip_attn_fused_fwd (attn_stream_fwd_kernel): any N >= 1, non-causal, hd = 64.
extern "C" int dclip_attn_stream_fwd(const void* qkv, int64_t ldq, void* ctx, int64_t ldc, int64_t B, int64_t H, int64_t N, int64_t hd,
                                     float scale, void* stream) {
    DCLIP_REQUIRE(qkv && ctx, "dclip_attn_stream_fwd: null operand");
    DCLIP_REQUIRE(B > 0 && H > 0 && N > 0, "dclip_attn_stream_fwd: need B, H, N > 0 (B=%ld H=%ld N=%ld)", (long)B, (long)H, (long)N);
    DCLIP_REQUIRE(hd == 64, "dclip_attn_stream_fwd: head dim must be 64 (got %ld)", (long)hd);
    DCLIP_REQUIRE(ldq % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)ctx % 16) == 0, "dclip_attn_stream_fwd: misaligned buffers");
    DCLIP_REQUIRE(ldq >= 3 * H * hd && ldc >= H * hd, "dclip_attn_stream_fwd: row strides shorter than the rows (ldq >= 3 H hd, ldc >= H hd)");
    const int64_t nqb = (N + SQB - 1) / SQB;
    DCLIP_REQUIRE(N < (1 << 24) && B * H * nqb < (1LL << 31) && B * N < (1LL << 31), "dclip_attn_stream_fwd: problem too large for one launch");
    AttnStream p{(const bf16_t*)qkv, ldq, (bf16_t*)ctx, ldc, (int)B, (int)H, (int)N, (int)nqb, scale};
    TraceScope tr(DCLIP_TRACE_ATTN, 4.0 * B * H * N * N * hd, 8.0 * B * H * N * hd, stream, (int)(B * H), (int)N, (int)hd, 7);
    hipLaunchKernelGGL((attn_stream_fwd_kernel<64>), dim3((unsigned)(B * H * nqb)), dim3(256), 0, (hipStream_t)stream, p);
    return dclip_check_launch("dclip_attn_stream_fwd");
}
