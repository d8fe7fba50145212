// Attention softmax stage with optional cross-head mixes (gfx950): the unfused score stage between the NT product that writes the
// scores and the NN product that reads the probabilities (attention.hip).
//
//   reference teacher: model/component/_common.py:73-89   (+ causal mask, softmax)
//   reference student: model/component/weight_share_model.py:101-125   (conv_l over heads ; softmax ; conv_w over heads)
//
// fp32 VALU with one wave per (b, query row); the head mixes of wide students and the weight gradients (dW_l, dW_w: H x H, reduced
// over B*N*N positions) run on 32x32x16 MFMA from wave-private LDS tiles.
// Score-like tensors live as [B, H, N, Np] with Np = round_up(N, 8) (16-byte rows); pad columns are zero.
#include <stdlib.h>
#include "attn_tiles.h"

namespace {

// B fragment of v_mfma_f32_32x32x16_bf16 from a k-major LDS tile (rows = contraction index, 32 columns from x0,
// 16 rows from r0): lane (col = l & 31, k = 8*(l >> 5) + e).  Each 16-lane group does two ds_read_b64_tr_b16.
template <int ROWB>
__device__ __forceinline__ bf16x8 tr_frag32(const char* tile, int r0, int x0, int lane) {
    const int g4 = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const char* a0 = tile + (r0 + 8 * (g4 >> 1) + q) * ROWB + (x0 + 16 * (g4 & 1) + 4 * pp) * 2;
    union { struct { s16x4 lo, hi; } s; bf16x8 v; } u;
    u.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    u.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * ROWB));
    return u.v;
}

__device__ __forceinline__ float lane_bcast(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// ---------------------------------------------------------------------------------------------------------
// softmax with optional cross-head mixes, one wave per (b, query row i); lane <-> key j (+64 per slot)
//   A_g = sum_h Wl[g,h] S_h ; P_g = softmax_j(A_g) (causal: j <= i) ; R_g = sum_h Ww[g,h] P_h
// ---------------------------------------------------------------------------------------------------------
struct SoftmaxFwd {
    const float* S;          // [B,H,N,Np] f32
    const float* Wl;         // [H,H] or null
    const float* Ww;         // [H,H] or null
    bf16_t* P;               // [B,H,N,Np] or null (saved for backward when Ww is set)
    bf16_t* R;               // [B,H,N,Np]
    int B, N, Np, causal;
    int H;                   // (run-time copy: the kernel without head mixing takes any head count)
};

// plain multi-head softmax (no head mixing: a CLIP tower that trains), any head count: one wave per (b, query row), heads in turn
template <int NS>
__global__ __launch_bounds__(256) void attn_softmax_fwd_plain_kernel(SoftmaxFwd p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.B * p.N) return;
    const int b = row / p.N, i = row % p.N;
    const int64_t hs = (int64_t)p.N * p.Np;
    const int64_t base = ((int64_t)b * p.H * p.N + i) * p.Np;
    float nxt[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) nxt[s] = lane + 64 * s < p.N ? p.S[base + lane + 64 * s] : 0.f;
    for (int h = 0; h < p.H; ++h) {
        float a[NS];
        float m = -INFINITY;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = lane + 64 * s;
            a[s] = (j < p.N && (!p.causal || j <= i)) ? nxt[s] : -INFINITY;
            m = fmaxf(m, a[s]);
            if (h + 1 < p.H) nxt[s] = j < p.N ? p.S[base + (h + 1) * hs + j] : 0.f;       // the next head's row is in flight during this one's reductions
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            a[s] = a[s] == -INFINITY ? 0.f : __expf(a[s] - m);
            sum += a[s];
        }
        const float inv = 1.f / wave_sum(sum);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = lane + 64 * s;
            if (j < p.Np) {
                const bf16_t v = f2bf(a[s] * inv);
                if (p.P) p.P[base + h * hs + j] = v;
                p.R[base + h * hs + j] = v;
            }
        }
    }
}

template <int H, int NS>
__global__ __launch_bounds__(256) void attn_softmax_fwd_kernel(SoftmaxFwd p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.B * p.N) return;
    const int b = row / p.N, i = row % p.N;
    const int64_t hs = (int64_t)p.N * p.Np;                       // head stride
    const int64_t base = ((int64_t)b * H * p.N + i) * p.Np;
    float sv[NS][H];
    bool valid[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = lane + 64 * s;
        valid[s] = j < p.N && (!p.causal || j <= i);
#pragma unroll
        for (int h = 0; h < H; ++h) sv[s][h] = j < p.N ? p.S[base + h * hs + j] : 0.f;
    }
    float pr[NS][H];
#pragma unroll
    for (int g = 0; g < H; ++g) {
        float a[NS];
        float m = -INFINITY;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (p.Wl) {
                float t = 0.f;
#pragma unroll
                for (int h = 0; h < H; ++h) t = fmaf(p.Wl[g * H + h], sv[s][h], t);
                a[s] = t;
            } else {
                a[s] = sv[s][g];
            }
            if (!valid[s]) a[s] = -INFINITY;
            m = fmaxf(m, a[s]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            a[s] = valid[s] ? __expf(a[s] - m) : 0.f;
            sum += a[s];
        }
        const float inv = 1.f / wave_sum(sum);
#pragma unroll
        for (int s = 0; s < NS; ++s) pr[s][g] = a[s] * inv;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = lane + 64 * s;
        if (j < p.Np) {
#pragma unroll
            for (int g = 0; g < H; ++g) {
                if (p.P) p.P[base + g * hs + j] = f2bf(pr[s][g]);
                float r = pr[s][g];
                if (p.Ww) {
                    r = 0.f;
#pragma unroll
                    for (int h = 0; h < H; ++h) r = fmaf(p.Ww[g * H + h], pr[s][h], r);
                }
                p.R[base + g * hs + j] = f2bf(r);
            }
        }
    }
}

// Head-mixing softmax forward on MFMA (one wave per (b, query row), tiles [32 heads][COLS keys] in wave-private LDS):
//   A_g = sum_h Wl[g,h] S_h     3 MFMAs per step with split-bf16 operands (Wl_hi S_hi + Wl_hi S_lo + Wl_lo S_hi): ~16 mantissa
//                               bits on the pre-softmax scores instead of 8
//   e   = exp(A - m_g)          m_g = max_j A[g, j], one maximum per output head g of the query row: a maximum shared by the heads
//                               would underflow every e of a head whose scores sit ~87 below another head's (sum 0 -> P = NaN)
//   sum_g = sum_j e[g,j]        MFMA of the e tile against a ones operand -> lands in accumulator layout (row g)
//   P = e / sum (saved for backward) ; R_g = sum_h Ww[g,h] P_h (MFMA) ; P and R leave through LDS as 16-byte rows
template <int H, int NS>
__global__ __launch_bounds__(256) void attn_softmax_fwd_mix_kernel(SoftmaxFwd p) {
    constexpr int COLS = 64 * NS, ROWB = COLS * 2 + 16, NCT = COLS / 32, TILE = 32 * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* tH = smem + wave * 3 * TILE;          // S_hi, later R
    char* tL = tH + TILE;                       // S_lo
    char* tP = tL + TILE;                       // e, then P
    for (int idx = lane; idx < 3 * TILE / 16; idx += 64) ((u32x4*)tH)[idx] = u32x4{0u, 0u, 0u, 0u};
    const int hh = lane >> 5, c = lane & 31;
    bf16x8 aLh[2], aLl[2], aWh[2], aWl2[2], ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = f2bf(1.f);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int h = 16 * s + 8 * hh + e;                                   // A[g = c][k = h]
            const float wl = (h < H && c < H) ? p.Wl[c * H + h] : 0.f;
            const bf16_t hi = f2bf(wl);
            aLh[s][e] = hi;
            aLl[s][e] = f2bf(wl - bf2f(hi));
            const float ww = (h < H && c < H) ? p.Ww[c * H + h] : 0.f;
            const bf16_t whi = f2bf(ww);
            aWh[s][e] = whi;
            aWl2[s][e] = f2bf(ww - bf2f(whi));
        }
    const int64_t hs = (int64_t)p.N * p.Np;
    const int rows = p.B * p.N;
    const int nchunk = p.Np >> 3, total = H * nchunk;
    // the next row's scores are fetched into registers BEFORE this row's P / R stores are issued: vmcnt retires loads and stores
    // in one in-order queue, so loads that follow the stores could only be waited for together with the stores' acknowledgements
    constexpr int NIT = (H * (COLS / 8) + 63) / 64;
    float4 q0[NIT], q1[NIT];
    auto fetch = [&](int row) {
        const int64_t fb = ((int64_t)(row / p.N) * H * p.N + row % p.N) * p.Np;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + it * 64;
            if (idx < total) {
                const int h = idx / nchunk, ck = idx - h * nchunk;
                const int64_t src = fb + h * hs + ck * 8;
                q0[it] = *(const float4*)(p.S + src); q1[it] = *(const float4*)(p.S + src + 4);
            }
        }
    };
    const int row_first = blockIdx.x * 4 + wave, row_step = gridDim.x * 4;
    if (row_first < rows) fetch(row_first);
    for (int row = row_first; row < rows; row += row_step) {
        const int b = row / p.N, i = row % p.N;
        const int64_t base = ((int64_t)b * H * p.N + i) * p.Np;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + it * 64;
            if (idx < total) {
                const int h = idx / nchunk, ck = idx - h * nchunk;
                const float4 s0 = q0[it], s1 = q1[it];
                const float v[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                bf16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) { hi[e] = f2bf(v[e]); lo[e] = f2bf(v[e] - bf2f(hi[e])); }
                *(bf16x8*)(tH + h * ROWB + ck * 16) = hi;
                *(bf16x8*)(tL + h * ROWB + ck * 16) = lo;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        f32x16 am[NCT];
        float m[16];                            // accumulator register r holds head g(r, hh) for every key: its maximum, per register
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            am[ct] = f32x16{0};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 bh = tr_frag32<ROWB>(tH, 16 * s, 32 * ct, lane), bl = tr_frag32<ROWB>(tL, 16 * s, 32 * ct, lane);
                am[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aLh[s], bh, am[ct], 0, 0, 0);
                am[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aLh[s], bl, am[ct], 0, 0, 0);
                am[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aLl[s], bh, am[ct], 0, 0, 0);
            }
            const bool jok = 32 * ct + c < p.N;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (jok && g < H) m[r] = fmaxf(m[r], am[ct][r]);
            }
        }
        // the keys of head g(r, hh) are spread over the 32 lanes of half hh (and the column tiles, folded in above)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o));
        // e = exp(A - m_g) as bf16 rows [g][j] in LDS (pad keys / pad heads stay zero; head g's largest e is 1, so its sum is >= 1)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const bool jok = 32 * ct + c < p.N;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float e = (jok && g < H) ? __expf(am[ct][r] - m[r]) : 0.f;
                am[ct][r] = e;
                *(bf16_t*)(tP + g * ROWB + (32 * ct + c) * 2) = f2bf(e);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // row sums on the matrix pipe: sum_g = sum_j e[g, j] * 1  (accumulator layout: row g in the registers)
        f32x16 rs = {0};
#pragma unroll
        for (int ks = 0; ks < COLS / 16; ++ks)
            rs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(tP + c * ROWB + (ks * 16 + hh * 8) * 2), ones, rs, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) rs[r] = __builtin_amdgcn_rcpf(rs[r]);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float pv = g < H ? am[ct][r] * rs[r] : 0.f;
                const bf16_t phi = f2bf(pv);
                *(bf16_t*)(tP + g * ROWB + (32 * ct + c) * 2) = phi;                       // saved P (bf16) = the hi part
                *(bf16_t*)(tL + g * ROWB + (32 * ct + c) * 2) = f2bf(pv - bf2f(phi));    // lo part, over the dead S_lo tile
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // R = Ww P, written over the (dead) S_hi tile as bf16 rows
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            f32x16 rr = {0};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 ph = tr_frag32<ROWB>(tP, 16 * s, 32 * ct, lane), pl = tr_frag32<ROWB>(tL, 16 * s, 32 * ct, lane);
                rr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aWh[s], ph, rr, 0, 0, 0);
                rr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aWh[s], pl, rr, 0, 0, 0);
                rr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aWl2[s], ph, rr, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
                *(bf16_t*)(tH + g * ROWB + (32 * ct + c) * 2) = f2bf(rr[r]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (row + row_step < rows) fetch(row + row_step);
        for (int idx = lane; idx < total; idx += 64) {
            const int h = idx / nchunk, ck = idx - h * nchunk;
            const int64_t dst = base + h * hs + ck * 8;
            if (p.P) *(u32x4*)(p.P + dst) = *(const u32x4*)(tP + h * ROWB + ck * 16);
            *(u32x4*)(p.R + dst) = *(const u32x4*)(tH + h * ROWB + ck * 16);
        }
    }
}

// backward of the stage above.  dP = Ww^T dR ; dA = P o (dP - sum_j P dP) ; dS = Wl^T dA
// dWw[g,h] += sum dR_g P_h ; dWl[g,h] += sum dA_g S_h     (32x32x16 MFMA over the key axis, per-wave accumulators)
struct SoftmaxBwd {
    const bf16_t* dR;        // [B,H,N,Np]
    const bf16_t* P;         // [B,H,N,Np] (post-softmax, pre conv_w)
    const float* S;          // [B,H,N,Np] raw scores (only read when Wl is set); bf16 when s_bf16
    int s_bf16;
    const float* Wl;
    const float* Ww;
    bf16_t* dS;              // [B,H,N,Np]
    float* dWl;              // [H,H] += (may be null)
    float* dWw;
    int B, N, Np;
    unsigned long long* stamps;   // profiling only (dclip_trace_attn_stamps): 8 x u64 per (wave, row iteration < 4), else null
    int H;                        // (run-time copy: the kernel without head mixing takes any head count)
};

// Head-mixing softmax backward, everything matrix-shaped on v_mfma_f32_32x32x16_bf16 (one wave per (b, query row)):
//   Cw[g,h] = sum_j dR[g,j] P[h,j]                (this row's dW_w contribution; also gives the softmax row sums:)
//   rs[h]   = sum_j P[h,j] dP[h,j] = sum_g Ww[g,h] Cw[g,h]
//   dP = Ww^T dR ; dA = P o (dP - rs) ; dS = Wl^T dA ; dWl += dA S^T
// Tiles [32 heads][COLS keys] bf16 live in wave-private LDS; dA feeds the second mix straight from the accumulator
// registers (guide §3 "An accumulator tile as the next MFMA's operand": Wl^T is pre-permuted in k).
template <int H, int NS>
__global__ __launch_bounds__(256) void attn_softmax_bwd_mix_kernel(SoftmaxBwd p) {
    constexpr int COLS = 64 * NS, ROWB = COLS * 2 + 16, NCT = COLS / 32, TILE = 32 * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* tR = smem + wave * 4 * TILE;      // dR
    char* tP = tR + TILE;                   // P
    char* tS = tP + TILE;                   // S (bf16)
    char* tD = tS + TILE;                   // dA
    for (int idx = lane; idx < 4 * TILE / 16; idx += 64) ((u32x4*)tR)[idx] = u32x4{0u, 0u, 0u, 0u};
    const int hh = lane >> 5, c = lane & 31;
    bf16x8 aWw[2], aWl[2], aI[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int g = 16 * s + 8 * hh + e;                               // natural k order
            const int rho = 16 * s + 8 * (e >> 2) + 4 * hh + (e & 3);        // k order of an accumulator-as-operand
            aWw[s][e] = f2bf((g < H && c < H) ? p.Ww[g * H + c] : 0.f);      // A[h = c][k = g]   = Ww[g][h]
            aWl[s][e] = f2bf((rho < H && c < H) ? p.Wl[rho * H + c] : 0.f);  // A[h' = c][k = g]  = Wl[g][h']
            aI[s][e] = f2bf(g == c ? 1.f : 0.f);
        }
    float wwc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
        wwc[r] = (g < H && c < H) ? p.Ww[g * H + c] : 0.f;
    }
    f32x16 accw = {0}, accl = {0};
    const int64_t hs = (int64_t)p.N * p.Np;
    const int rows = p.B * p.N;
    const int nchunk = p.Np >> 3, total = H * nchunk;
    const int nct = (p.N + 31) >> 5;                 // key tiles that hold real keys (the rest is all padding)
    const int nks = nct * 2;
    // NS == 2 (one workgroup per CU, one wave per SIMD): the next row's operands are fetched into registers while this row is
    // being computed, otherwise every row pays the full HBM latency before its first MFMA (229 -> 200 us at H = 12, N = 77).
    // With two workgroups per CU (NS == 1) the second wave already covers that latency and the extra registers cost more.
    constexpr bool PREFETCH = NS == 2;
    constexpr int NIT = (H * (COLS / 8) + 63) / 64;
    u32x4 qR[NIT], qP[NIT];
    float4 qS0[NIT], qS1[NIT];
    auto fetch = [&](int row) {
        const int64_t base = ((int64_t)(row / p.N) * H * p.N + row % p.N) * p.Np;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + it * 64;
            if (idx < total) {
                const int h = idx / nchunk, ck = idx - h * nchunk;
                const int64_t src = base + h * hs + ck * 8;
                qR[it] = *(const u32x4*)(p.dR + src);
                qP[it] = *(const u32x4*)(p.P + src);
                if (p.s_bf16) qS0[it] = *(const float4*)((const bf16_t*)p.S + src);       // 8 bf16 scores in one 16-byte register set
                else { qS0[it] = *(const float4*)(p.S + src); qS1[it] = *(const float4*)(p.S + src + 4); }
            }
        }
    };
    const int row_first = blockIdx.x * 4 + wave, row_step = gridDim.x * 4;
    if (PREFETCH && row_first < rows) fetch(row_first);
    int iter = 0;
    auto stamp = [&](int k) {
        if (p.stamps && lane == 0 && iter < 4) {
            if (k == 1 || k == 4) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            p.stamps[(((int64_t)blockIdx.x * 4 + wave) * 4 + iter) * 8 + k] = __builtin_readcyclecounter();
        }
    };
    // dS of a row is staged in the dR tile (each key tile's columns are dead once its dP product has been read) and leaves as
    // 16-byte row segments at the START of the next iteration, after that row's loads have been issued: vmcnt retires loads and
    // stores in one in-order queue, so the 32 scattered 2-byte stores per row of the first version, issued before the next
    // row's loads, made every row wait for their acknowledgement.
    int64_t prev_base = -1;
    auto flush = [&]() {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + it * 64;
            if (idx < total) {
                const int h = idx / nchunk, ck = idx - h * nchunk;
                *(u32x4*)(p.dS + prev_base + h * hs + ck * 8) = *(const u32x4*)(tR + h * ROWB + ck * 16);
            }
        }
    };
    for (int row = row_first; row < rows; row += row_step, ++iter) {
        const int b = row / p.N, i = row % p.N;
        const int64_t base = ((int64_t)b * H * p.N + i) * p.Np;
        __builtin_amdgcn_wave_barrier();
        stamp(0);
        if (!PREFETCH) fetch(row);                       // loads first ...
        if (prev_base >= 0) flush();                     // ... then the previous row's stores
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = lane + it * 64;
                if (idx < total) {
                    const int h = idx / nchunk, ck = idx - h * nchunk;
                    *(u32x4*)(tR + h * ROWB + ck * 16) = qR[it];
                    *(u32x4*)(tP + h * ROWB + ck * 16) = qP[it];
                    const float4 s0 = qS0[it], s1 = qS1[it];
                    if (p.s_bf16) *(float4*)(tS + h * ROWB + ck * 16) = s0;
                    else *(bf16x8*)(tS + h * ROWB + ck * 16) = bf16x8{f2bf(s0.x), f2bf(s0.y), f2bf(s0.z), f2bf(s0.w),
                                                                      f2bf(s1.x), f2bf(s1.y), f2bf(s1.z), f2bf(s1.w)};
                }
            }
        }
        prev_base = base;
        if (PREFETCH && row + row_step < rows) fetch(row + row_step);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        stamp(1);
        // Cw = dR P^T  (this row's dW_w contribution) and the softmax row sums rs[h] = sum_g Ww[g,h] Cw[g,h]
        float part = 0.f;
        {
            f32x16 cw = {0};
#pragma unroll
            for (int ks = 0; ks < COLS / 16; ++ks)
                if (ks < nks) {
                    const int off = c * ROWB + (ks * 16 + hh * 8) * 2;
                    cw = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(tR + off), *(const bf16x8*)(tP + off), cw, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) part = fmaf(wwc[r], cw[r], part);
            accw += cw;
        }
        part += __shfl_xor(part, 32);                      // lanes h and h + 32 now hold rs[h]
        float rsr[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int h0 = (r & 3) + 8 * (r >> 2);
            rsr[r] = hh ? lane_bcast(part, h0 + 4) : lane_bcast(part, h0);
        }
        stamp(2);
        // one key tile at a time: dP = Ww^T dR, P in accumulator layout, dA = P o (dP - rs), dS = Wl^T dA
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            if (ct < nct) {
                f32x16 dp = {0}, pa = {0};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aWw[s], tr_frag32<ROWB>(tR, 16 * s, 32 * ct, lane), dp, 0, 0, 0);
                    pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aI[s], tr_frag32<ROWB>(tP, 16 * s, 32 * ct, lane), pa, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int h = (r & 3) + 8 * (r >> 2) + 4 * hh;
                    dp[r] = pa[r] * (dp[r] - rsr[r]);                                   // dA
                    *(bf16_t*)(tD + h * ROWB + (32 * ct + c) * 2) = f2bf(dp[r]);
                }
                f32x16 ds = {0};
                bf16x8 bf[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) bf[s][e] = f2bf(dp[8 * s + e]);
                    ds = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aWl[s], bf[s], ds, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int h = (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (h < H) *(bf16_t*)(tR + h * ROWB + (32 * ct + c) * 2) = f2bf(ds[r]);      // this key tile's dR columns are dead
                }
                mfma_keep_alive(bf);            // operands built by the VALU stay live past their (queued) MFMAs (common.h)
            }
        }
        // dW_l += dA S^T
        stamp(3);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < COLS / 16; ++ks)
            if (ks < nks) {
                const int off = c * ROWB + (ks * 16 + hh * 8) * 2;
                accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(tD + off), *(const bf16x8*)(tS + off), accl, 0, 0, 0);
            }
        stamp(4);
    }
    if (prev_base >= 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        flush();
    }
    // accumulators: element (g = (r&3) + 8*(r>>2) + 4*hh, h = c).  The 2 H^2 gradient elements live in ~36 cache lines that every
    // wave of the grid adds to: the workgroup's four waves are summed through LDS first (the tiles are dead) so that one wave
    // issues the atomics — same-line atomics serialise, and with 2 048 waves adding they were ~half of the kernel's time.
    __syncthreads();
    float* red = (float*)smem;                          // [4 waves][2][16][64]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        red[((wave * 2 + 0) * 16 + r) * 64 + lane] = accw[r];
        red[((wave * 2 + 1) * 16 + r) * 64 + lane] = accl[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int g = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (g < H && c < H) {
                float w = 0.f, l = 0.f;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    w += red[((v * 2 + 0) * 16 + r) * 64 + lane];
                    l += red[((v * 2 + 1) * 16 + r) * 64 + lane];
                }
                if (p.dWw) unsafeAtomicAdd(p.dWw + g * H + c, w);
                if (p.dWl) unsafeAtomicAdd(p.dWl + g * H + c, l);
            }
        }
    }
}

// plain multi-head softmax backward (no head mixing): dS = P o (dR - sum_j P dR), one wave per (b, query row)
template <int NS>
__global__ __launch_bounds__(256) void attn_softmax_bwd_plain_kernel(SoftmaxBwd p) {
    const int H = p.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t hs = (int64_t)p.N * p.Np;
    const int rows = p.B * p.N;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const int b = row / p.N, i = row % p.N;
        const int64_t base = ((int64_t)b * H * p.N + i) * p.Np;
        for (int h = 0; h < H; ++h) {
            float dr[NS], pv[NS], rs = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                dr[s] = j < p.N ? bf2f(p.dR[base + h * hs + j]) : 0.f;
                pv[s] = j < p.N ? bf2f(p.P[base + h * hs + j]) : 0.f;
                rs += dr[s] * pv[s];
            }
            rs = wave_sum(rs);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int j = lane + 64 * s;
                if (j < p.Np) p.dS[base + h * hs + j] = f2bf(j < p.N ? pv[s] * (dr[s] - rs) : 0.f);     // pad columns [N, Np) +0 at every Np, the towers' round_up(N, 8) included: 0 * (0 - rs) gave -0 there for rs > 0
            }
        }
    }
}

unsigned long long* g_attn_stamps = nullptr;
}  // namespace

extern "C" int dclip_trace_attn_stamps(void* buf) { g_attn_stamps = (unsigned long long*)buf; return 0; }

#define SM_DISPATCH_H(Hv, NSv, ...)                                               \
    switch (Hv) {                                                                 \
        case 2: { constexpr int HH = 2; SM_DISPATCH_NS(NSv, __VA_ARGS__); break; }   \
        case 4: { constexpr int HH = 4; SM_DISPATCH_NS(NSv, __VA_ARGS__); break; }   \
        case 8: { constexpr int HH = 8; SM_DISPATCH_NS(NSv, __VA_ARGS__); break; }   \
        case 12: { constexpr int HH = 12; SM_DISPATCH_NS(NSv, __VA_ARGS__); break; } \
        case 24: { constexpr int HH = 24; SM_DISPATCH_NS(NSv, __VA_ARGS__); break; } \
        default: dclip_set_error("attention softmax: unsupported head count %d (2/4/8/12/24)", (int)(Hv)); return DCLIP_EINVAL; \
    }
#define SM_DISPATCH_NS(NSv, ...)                              \
    if ((NSv) == 1) { constexpr int NSS = 1; __VA_ARGS__; }   \
    else { constexpr int NSS = 2; __VA_ARGS__; }

extern "C" int dclip_attn_softmax_fwd(const float* S, const float* Wl, const float* Ww, void* P, void* R, int64_t B, int64_t H,
                                      int64_t N, int64_t Np, int causal, void* stream) {
    DCLIP_REQUIRE(S && R && B > 0 && N > 0 && N <= NMAX && Np % 8 == 0 && Np >= N && Np <= NMAX, "dclip_attn_softmax_fwd: bad argument");
    DCLIP_REQUIRE((Wl == nullptr) == (Ww == nullptr), "dclip_attn_softmax_fwd: conv_l and conv_w come together");
    SoftmaxFwd p{S, Wl, Ww, (bf16_t*)P, (bf16_t*)R, (int)B, (int)N, (int)Np, causal, (int)H};
    TraceScope tr(DCLIP_TRACE_ATTN, Wl ? 4.0 * B * H * H * N * N : 0.0, (4.0 + 2.0 + (P ? 2.0 : 0.0)) * B * H * N * Np, stream, (int)(B * H), (int)N, (int)H, 5);
    const int ns = Np > 64 ? 2 : 1;      // 64-key slots of a row, pad columns included: any multiple of 8 with N <= Np <= 128
    hipStream_t st = (hipStream_t)stream;
    if (Wl && !causal && H > 12) {     // H <= 12: the 144-FMA register mix is faster than 32-row MFMA tiles (measured)
        int blocks = (int)((B * N + 3) / 4);
        if (blocks > 512) blocks = 512;              // persistent waves: constant fragments / LDS zero-fill amortised over rows
        const size_t lds = (size_t)4 * 3 * 32 * (64 * ns * 2 + 16);
        SM_DISPATCH_H(H, ns, hipLaunchKernelGGL((attn_softmax_fwd_mix_kernel<HH, NSS>), dim3(blocks), dim3(256), lds, st, p));
    } else if (!Wl) {                  // no head mixing: any head count
        const dim3 grid((unsigned)((B * N + 3) / 4));
        if (ns == 1) hipLaunchKernelGGL((attn_softmax_fwd_plain_kernel<1>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((attn_softmax_fwd_plain_kernel<2>), grid, dim3(256), 0, st, p);
    } else {
        const dim3 grid((unsigned)((B * N + 3) / 4));
        SM_DISPATCH_H(H, ns, hipLaunchKernelGGL((attn_softmax_fwd_kernel<HH, NSS>), grid, dim3(256), 0, st, p));
    }
    return dclip_check_launch("dclip_attn_softmax_fwd");
}

extern "C" int dclip_attn_softmax_bwd(const void* dR, const void* P, const void* S, int scores_bf16, const float* Wl, const float* Ww,
                                      void* dS, float* dWl, float* dWw, int64_t B, int64_t H, int64_t N, int64_t Np, void* stream) {
    DCLIP_REQUIRE(dR && P && dS && B > 0 && N > 0 && N <= NMAX && Np % 8 == 0 && Np >= N && Np <= NMAX, "dclip_attn_softmax_bwd: bad argument");
    DCLIP_REQUIRE((Wl == nullptr) == (Ww == nullptr), "dclip_attn_softmax_bwd: conv_l and conv_w come together");
    DCLIP_REQUIRE(!Wl || S, "dclip_attn_softmax_bwd: raw scores needed for dW_l");
    SoftmaxBwd p{(const bf16_t*)dR, (const bf16_t*)P, (const float*)S, scores_bf16, Wl, Ww, (bf16_t*)dS, dWl, dWw, (int)B, (int)N, (int)Np, g_attn_stamps, (int)H};
    TraceScope tr(DCLIP_TRACE_ATTN, Wl ? 8.0 * B * H * H * N * N : 0.0, (2.0 + 2.0 + 2.0 + (Wl ? (scores_bf16 ? 2.0 : 4.0) : 0.0)) * B * H * N * Np, stream, (int)(B * H), (int)N, (int)H, 6);
    int blocks = (int)((B * N + 3) / 4);
    if (blocks > 2048) blocks = 2048;
    const int ns = Np > 64 ? 2 : 1;      // 64-key slots of a row, pad columns included: any multiple of 8 with N <= Np <= 128
    hipStream_t st = (hipStream_t)stream;
    if (Wl) {
        // ~280 registers -> one resident workgroup per CU: launch one persistent workgroup per CU so the per-workgroup
        // setup (LDS zero-fill, constant Ww / Wl fragments) is amortised over all its rows
        const size_t lds = (size_t)4 * 4 * 32 * (64 * ns * 2 + 16);
        const int per_cu = lds <= 80 * 1024 ? 2 : 1;        // persistent workgroups: setup amortised over all rows
        if (blocks > 256 * per_cu) blocks = 256 * per_cu;
        SM_DISPATCH_H(H, ns, hipLaunchKernelGGL((attn_softmax_bwd_mix_kernel<HH, NSS>), dim3(blocks), dim3(256), lds, st, p));
    } else {
        if (ns == 1) hipLaunchKernelGGL((attn_softmax_bwd_plain_kernel<1>), dim3(blocks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((attn_softmax_bwd_plain_kernel<2>), dim3(blocks), dim3(256), 0, st, p);
    }
    return dclip_check_launch("dclip_attn_softmax_bwd");
}
