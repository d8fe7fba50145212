// What gemm_nt.hip (forward / dgrad) and gemm_tn.hip (wgrad) share: the forward launch descriptor and its per-unit epilogue (8 consecutive
// output columns of one row), the sub-tile swizzle, and the tile primitives of both families, each written down once.
#pragma once
#include <math.h>
#include <stdlib.h>
#include "common.h"
#include <type_traits>

namespace dgemm {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int SUB = 1024;                       // bytes of one [16 x 32] bf16 sub-tile
constexpr int HT = 16384;                       // bytes of a half-tile of the 256-row pipelines: 128 x 64 bf16, either way round

// profiling stamps of the next launches (dclip_trace_gemm_stamps sets it, both families read it): 6 x u64 per workgroup, or null
inline unsigned long long* g_gemm_stamps = nullptr;

struct GemmNT {
    const bf16_t* A; int64_t lda;
    const bf16_t* B; int64_t ldb;
    void* C; int64_t ldc;
    int M, N, K;
    float alpha;
    const float* bias;
    const void* aux_in;                             // ACT 3: bf16 pre-activation ; ACT 4: u8 fixed-point gelu' (dg_pack4)
    void* aux_out;                                  // ACT 5: u8 gelu' ; other ACT: bf16 pre-activation
    const void* residual; int64_t ldr;              // OUT 1: f32 ; OUT 2: f16 ; OUT 0: f32 (never aliases C)
    int row_group; const float* rowadd;
    float* colsum;                                  // += column sums of the epilogue output (bias gradient), may be null
    int tiles_m, tiles_n;
    unsigned long long* stamps;                     // profiling only (dclip_trace_gemm_stamps): 6 x u64 per workgroup, else null
    int group_n;                                    // 256-/320-row kernels: column tiles per raster group (>= tiles_n: plain n-fastest)
    unsigned long long* clk;                        // measurement only (dclip_trace_gemm_clock): 4 x u64 of this launch, else null
};

__device__ __forceinline__ int swz(int x) { return x ^ (((x >> 9) & 1) << 5); }

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

// side operands of one output row segment, loaded ahead of use: residual and C may alias (in-place residual stream), so the
// compiler cannot hoist these loads above the previous row's store by itself — left inside the row loop every row pays a
// full HBM round trip in sequence
struct EpiSide {
    float4 r0, r1;      // residual (f32 stream)
    f16x8 rh;           // residual (f16 stream)
    bf16x8 z;           // aux_in, ACT 3
    uint2 zq;           // aux_in, ACT 4
};

// OUT: 0 bf16, 1 f32, 2 f16 output.  (The residual travels in EpiSide only with f32 / f16 output — the in-place residual stream; with
//  bf16 output it cannot alias C and is read inline.)
template <int ACT, int OUT>
__device__ __forceinline__ void epilogue_load_side(const GemmNT& p, int64_t o, int64_t orr, EpiSide& sd) {
    if (OUT == 1 && p.residual) {
        const float* rp = (const float*)p.residual + orr;
        sd.r0 = *(const float4*)rp; sd.r1 = *(const float4*)(rp + 4);
    }
    if (OUT == 2 && p.residual) sd.rh = *(const f16x8*)((const _Float16*)p.residual + orr);
    if (ACT == 3) sd.z = *(const bf16x8*)((const bf16_t*)p.aux_in + o);
    if (ACT == 4) sd.zq = *(const uint2*)((const uint8_t*)p.aux_in + o);
}

// MODE 0: every optional operand is a run-time test (wave-uniform branches: four per 8-column unit, 80 per 320 x 256 tile and wave —
// about 40 % of the issue slots of a plain bf16 epilogue, which is issue-bound).  MODE 1 / 2: the launch has no positional table, no
// residual and no saved pre-activation (ACT 5 / 6 always save their derivative), without / with bias-gradient column sums — the
// combinations the step's bf16 GEMMs use; the tests are compiled out.
// CSUM_ALWAYS: csum takes every unit's output whatever OUT and p.colsum are (gemm_nt_kernel, which launch_nt gives every launch that wants
// column sums with f32 / f16 output, and which tests p.colsum once per tile); the 256-row kernels leave it off and sum with bf16 output only.
template <int ACT, int OUT, int MODE = 0, bool CSUM_ALWAYS = false>
__device__ __forceinline__ void epilogue_vec8(const GemmNT& p, float (&v)[8], int row, int col, int64_t o, int64_t orr,
                                              const float (&bias)[8], float (&csum)[8], const EpiSide& sd) {
    constexpr bool LEAN = MODE != 0;            // MODE 3: f32 / f16 output with the (in-place) residual, nothing else optional
    // o = row * ldc + col, orr = row * ldr + col (formed incrementally by the caller)
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] * p.alpha + bias[e];
    if (!LEAN && p.row_group > 0) {      // (patch-embedding GEMM only: the position-embedding rows, L2-resident)
        const float* ra = p.rowadd + (int64_t)(row % p.row_group) * p.N + col;
        const float4 a0 = *(const float4*)ra, a1 = *(const float4*)(ra + 4);
        v[0] += a0.x; v[1] += a0.y; v[2] += a0.z; v[3] += a0.w; v[4] += a1.x; v[5] += a1.y; v[6] += a1.z; v[7] += a1.w;
    }
    if (!LEAN && ACT != 5 && ACT != 6 && p.aux_out) {
        bf16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = f2bf(v[e]);
        *(bf16x8*)((bf16_t*)p.aux_out + o) = z;
    }
    if (ACT == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = quick_gelu_f(v[e]);
    }
    if (ACT == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_erf_f(v[e]);
    }
    if (ACT == 3) {
        const bf16x8 z = sd.z;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= dgelu_erf_f(bf2f(z[e]));
    }
    if (ACT == 4) {
        const uint2 q = sd.zq;
        v[0] *= dg_unpack(q.x, 0); v[1] *= dg_unpack(q.x, 1); v[2] *= dg_unpack(q.x, 2); v[3] *= dg_unpack(q.x, 3);
        v[4] *= dg_unpack(q.y, 0); v[5] *= dg_unpack(q.y, 1); v[6] *= dg_unpack(q.y, 2); v[7] *= dg_unpack(q.y, 3);
    }
    if (ACT == 5) {
        float dg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float g;
            gelu_erf_both_f(v[e], g, dg[e]);
            v[e] = g;
        }
        if (LEAN || p.aux_out) *(uint2*)((uint8_t*)p.aux_out + o) = uint2{dg_pack4(dg[0], dg[1], dg[2], dg[3]), dg_pack4(dg[4], dg[5], dg[6], dg[7])};
    }
    if (ACT == 6) {      // QuickGELU of a trainable CLIP tower: x s(1.702 x) and its derivative s + 1.702 x s (1 - s), in [-0.1, 1.1]
        float dg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * v[e]));
            dg[e] = fmaf(1.702f * v[e] * sg, 1.f - sg, sg);
            v[e] *= sg;
        }
        if (LEAN || p.aux_out) *(uint2*)((uint8_t*)p.aux_out + o) = uint2{dg_pack4(dg[0], dg[1], dg[2], dg[3]), dg_pack4(dg[4], dg[5], dg[6], dg[7])};
    }
    if (MODE == 3 || (!LEAN && p.residual)) {
        if (OUT == 2) {
            const f16x8 r = sd.rh;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
        } else {
            float4 r0, r1;
            if (OUT == 1) { r0 = sd.r0; r1 = sd.r1; }
            else {
                const float* rp = (const float*)p.residual + orr;
                r0 = *(const float4*)rp; r1 = *(const float4*)(rp + 4);
            }
            v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
        }
    }
    if (OUT == 1) {
        float* cp = (float*)p.C + o;
        *(float4*)cp = float4{v[0], v[1], v[2], v[3]};
        *(float4*)(cp + 4) = float4{v[4], v[5], v[6], v[7]};
    } else if (OUT == 2) {
        f16x8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = (_Float16)v[e];
        *(f16x8*)((_Float16*)p.C + o) = ov;
    } else {
        bf16x8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = f2bf(v[e]);
        *(bf16x8*)((bf16_t*)p.C + o) = ov;
    }
    if (CSUM_ALWAYS || (OUT == 0 && (MODE == 2 || (MODE == 0 && p.colsum)))) {
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[e] += v[e];
    }
}

#define WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// workgroup stamp k (off unless dclip_trace_gemm_stamps armed it): s_memtime at 0 start / 1 first operands landed / 2 main loop done /
// 3 epilogue done (stores acknowledged); slots 4 and 5 take s_memrealtime at start and end.  (Arguments by reference, as a lambda would
// capture them: by value, hipcc forms gemm_tn256_kernel's wave index and first source addresses differently.)
__device__ __forceinline__ void wg_stamp(unsigned long long* const& stamps, const int& tid, int k) {
    if (stamps && tid == 0) {
        if (k == 3) WAIT_VMCNT(0);
        stamps[6 * (int64_t)blockIdx.x + k] = __builtin_readcyclecounter();
        if (k == 0) stamps[6 * (int64_t)blockIdx.x + 4] = __builtin_amdgcn_s_memrealtime();
        if (k == 3) stamps[6 * (int64_t)blockIdx.x + 5] = __builtin_amdgcn_s_memrealtime();
    }
}

// the 128^2 kernels' wave tile: acc[i][j] += a[i] b[j]^T over one 32-wide k block, 4 x 4 tiles of 16 x 16
__device__ __forceinline__ void mfma_4x4(f32x4 (&acc)[4][4], const bf16x8 (&a)[4], const bf16x8 (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
}

// One phase of the 256-row pipelines between its two barriers: row tiles R0 .. R0 + RT - 1 of the wave x its four column tiles
// (fragments b0: columns 0, 1; b1: columns 2, 3) x both k halves, at raised priority.  SWAP: the row fragment is the MFMA's second
// operand (C^T = B A^T, gemm_nt256_kernel).  The caller has retired its own LDS reads (lgkmcnt(0)) before it.
// A macro, not a function: with the fragment and accumulator arrays handed to a function by reference (forced inline or not, a
// generic lambda too), hipcc moves 20 of a phase's 32 MFMAs behind the closing barrier, among the next phase's LDS reads — every
// instruction count stays the same, only the order shows it (tools/diag/isa_compare.py).
template <bool SWAP>
__device__ __forceinline__ f32x4 mfma_rc(bf16x8 rowf, bf16x8 colf, f32x4 c) {
    return SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(colf, rowf, c, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x32_bf16(rowf, colf, c, 0, 0, 0);
}
#define PHASE_MFMA(SWAP, acc, R0, RT, af, b0, b1)                                                                         \
    do {                                                                                                                  \
        __builtin_amdgcn_s_barrier();                                                                                     \
        __builtin_amdgcn_s_setprio(1);                                                                                    \
        _Pragma("unroll") for (int kb_ = 0; kb_ < 2; ++kb_)                                                               \
            _Pragma("unroll") for (int i_ = 0; i_ < (RT); ++i_) {                                                         \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                                          \
                    acc[(R0) + i_][j_] = mfma_rc<SWAP>(af[i_][kb_], b0[j_][kb_], acc[(R0) + i_][j_]);                     \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                                          \
                    acc[(R0) + i_][2 + j_] = mfma_rc<SWAP>(af[i_][kb_], b1[j_][kb_], acc[(R0) + i_][2 + j_]);             \
            }                                                                                                             \
        __builtin_amdgcn_s_setprio(0);                                                                                    \
        __builtin_amdgcn_s_barrier();                                                                                     \
    } while (0)

// accumulator tiles -> f32 LDS image with rows of LD floats: NI row tiles x 4 column tiles of a wave, from (row0, col0).  acc[i][j][r]
// is element (i * 16 + (lane >> 4) * 4 + r, j * 16 + (lane & 15)), so storing from registers would mean scattered 4-byte accesses.
template <int NI, int LD>
__device__ __forceinline__ void stage_acc(float* cs, const f32x4 (*acc)[4], int row0, int col0, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) cs[(row0 + i * 16 + (lane >> 4) * 4 + r) * LD + col0 + j * 16 + (lane & 15)] = acc[i][j][r];
}

}  // namespace dgemm
