// Device pieces shared by the embedding-side kernels (metrics.hip, recall.hip, topk.hip, and through loss_stripes.h loss.hip and
// interactive.hip): the 16 x 16 tile of dot products on the exact-f32 MFMA, its diagonal, the reduction of a 16-row stripe over the four
// waves of a workgroup, and the row normaliser.
#pragma once
#include "common.h"

// One 16 x 16 tile of dot products.  pa / pb: THIS LANE's row of the A / B panel (row lane & 15; the 16 rows need not be neighbours).
// Lane (r = l & 15, g = l >> 4) feeds column 16 o + 4 g + t at MFMA step t ; acc[q] = X[A row 4 g + q][B row l & 15].  Each element is the
// fmaf chain over k = 16 o + 4 g + t in the order (o, t, g): a function of the two rows only, so bit-equal rows give bit-equal dot
// products wherever they sit and whichever kernel asks.  A panel of neighbouring rows [i0, i0 + 16) clamped inside an n-row matrix is
// base + (int64_t)min(i0 + (lane & 15), n - 1) * E.
__device__ __forceinline__ f32x4 dot_tile(const float* __restrict__ pa, const float* __restrict__ pb, int E, int lane) {
    pa += (lane >> 4) * 4;
    pb += (lane >> 4) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < E; o += 16) {
        const float4 av = *(const float4*)(pa + o), bv = *(const float4*)(pb + o);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
    }
    return acc;
}

// d[q] = X[4 g + q][4 g + q]: the diagonal of a tile, handed to every lane of the row group that owns the row
__device__ __forceinline__ f32x4 tile_diag(const f32x4& S, int lane) {
    const int g = lane >> 4;
    f32x4 d;
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = __shfl(S[q], g * 16 + g * 4 + q);
    return d;
}

struct StripeSum { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct StripeMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// Reduction of a 16-row stripe whose column tiles the four waves of a workgroup split: v[q] is this lane's partial of row 4 g + q.
// stripe_put combines the 16 lanes of each row group and leaves the wave's 16 results in red[wave]; stripe_get combines the four
// waves' results of row r.  Neither holds a barrier: the caller puts ONE __syncthreads() between its puts and its gets, so several
// quantities (each with a [4][16] array of its own) share it.
template <class Op, class T>
__device__ __forceinline__ void stripe_put(T (*red)[16], const T (&v)[4], int lane, int wave, Op op) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        T x = v[q];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) x = op(x, __shfl_xor(x, o));
        if ((lane & 15) == 0) red[wave][(lane >> 4) * 4 + q] = x;
    }
}
template <class Op, class T>
__device__ __forceinline__ T stripe_get(T (*red)[16], int r, Op op) {
    return op(op(red[0][r], red[1][r]), op(red[2][r], red[3][r]));
}

// x / |x| of one row by one wave.  ZERO_SAFE = false: no epsilon and 1 / sqrt(0) on a zero row, as the reference's validation
// metrics; true: a row whose squared norm is 0 (or not a positive finite number) becomes the zero row, so every cosine with it is 0.
// Returns the scale it applied, 1 / |x| (every lane holds it).
template <bool ZERO_SAFE>
__device__ __forceinline__ float normalize_row(const float* src, float* dst, int E, int lane) {
    float s = 0.f;
    for (int c = lane * 4; c < E; c += 256) {
        const float4 v = *(const float4*)(src + c);
        s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    s = wave_sum(s);
    const float inv = (!ZERO_SAFE || (s > 0.f && s < __builtin_inff())) ? 1.f / sqrtf(s) : 0.f;
    for (int c = lane * 4; c < E; c += 256) {
        const float4 v = *(const float4*)(src + c);
        *(float4*)(dst + c) = float4{v.x * inv, v.y * inv, v.z * inv, v.w * inv};
    }
    return inv;
}
