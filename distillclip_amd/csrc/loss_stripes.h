// The stripe skeleton of the cross-modal loss kernels (loss.hip, interactive.hip), on the pieces of sim_tiles.h.  A [B, B] logit matrix is
// never stored: a workgroup owns 16 rows ("stripe") and one slice of the column tiles, and every kernel of the two files is built from
//   pass A  running log-sum-exp of every row over the slice's tiles (RunLse per lane, LogAddExp over lanes and waves through stripe_put /
//           stripe_get), one partial per slice;
//   pass B  slices_lse of the partials, dL/dlogit of the slice in LDS ([16][ldl] f32), stripe_times_rows -> one partial gradient row per slice;
//   close   stripe_close_row: the slices' rows added in slice order and the backward of x / |x|.
// What a kernel computes per element (which terms, which scalars) stays with the kernel; the geometry, the merges and the two products
// are defined here once.  Every sum here has a fixed shape: bit-equal inputs give bit-equal results.
#pragma once
#include "sim_tiles.h"
#include <math.h>

constexpr int STRIPE_MAX_SLICES = 8;
constexpr int STRIPE_MAX_E = 1024;            // stripe_close_row keeps a row in 4 float4 per lane

// running softmax statistic of one lane: maximum m and sum l of exp(x - m) over the values seen so far.  A NaN logit makes l NaN
// (fmaxf drops it from m) and lse() hands it on.
struct RunLse {
    float m = -INFINITY, l = 0.f;
    __device__ __forceinline__ void add(float x) {
        const float mn = fmaxf(m, x);
        l = l * __expf(m - mn) + __expf(x - mn);
        m = mn;
    }
    __device__ __forceinline__ float lse() const { return l == 0.f ? -INFINITY : m + __logf(l); }
};

// log(exp(a) + exp(b)); -inf stands for an empty sum, a NaN on either side gives NaN.  The merge operator of stripe_put / stripe_get.
struct LogAddExp {
    __device__ __forceinline__ float operator()(float a, float b) const {
        if (a == -INFINITY && b == -INFINITY) return a;
        const float m = fmaxf(a, b);
        return m + __logf(__expf(a - m) + __expf(b - m));
    }
};

// log-sum-exp of one row: its per-slice partials p[0], p[stride], ... merged in slice order
__device__ __forceinline__ float slices_lse(const float* p, int64_t stride, int zs) {
    float v = -INFINITY;
    for (int zz = 0; zz < zs; ++zz) v = LogAddExp{}(v, p[zz * stride]);
    return v;
}

// Column slices of a [., B] logit matrix.  Slice z of zs walks the column tiles [t0, t1); stripe B holds its columns in LDS rows of ldl
// floats (the widest slice's columns + 4: the pad keeps the 16 rows on different banks).
struct StripeSlice { int t0, t1; };
__host__ __device__ inline int stripe_tiles(int64_t n) { return (int)((n + 15) / 16); }
__host__ __device__ inline StripeSlice stripe_slice(int B, int zs, int z) {
    const int64_t nt = stripe_tiles(B);
    return {(int)(nt * z / zs), (int)(nt * (z + 1) / zs)};
}
__host__ __device__ inline int stripe_ldl(int B, int zs) { return ((stripe_tiles(B) + zs - 1) / zs) * 16 + 4; }
inline size_t stripe_lds_bytes(int B, int zs) { return (size_t)16 * stripe_ldl(B, zs) * sizeof(float); }

// slice count: enough workgroups for the chip from the owned row stripes (two directions each), at most 8, at most one per column tile,
// then as many more as keep a slice within max_cols columns (the caller's LDS budget)
inline int stripe_slices(int row_tiles, int col_tiles, int max_cols) {
    int zs = 256 / (2 * row_tiles);
    zs = zs < 1 ? 1 : (zs > STRIPE_MAX_SLICES ? STRIPE_MAX_SLICES : zs);
    zs = zs > col_tiles ? col_tiles : zs;
    while (zs < STRIPE_MAX_SLICES && ((col_tiles + zs - 1) / zs) * 16 > max_cols) ++zs;
    return zs;
}

// Partial gradient rows of one stripe and slice: G[16, E] = D[16, columns of the slice] @ Y[columns, E] on the f32 MFMA, by the four
// waves of a workgroup (16 columns of E each per trip).  dsl: the stripe's D in LDS, [16][ldl], column 0 = column 16 t0 of the matrix.
// Row i0 + r of the matrix is written to G row i0 + r - first_row if it is below row_end (plain stores, one writer each).
__device__ __forceinline__ void stripe_times_rows(const float* dsl, int ldl, const float* Y, StripeSlice s, int B, int E,
                                                  float* G, int i0, int first_row, int row_end, int lane, int wave) {
    const float* arow = dsl + (lane & 15) * ldl + (lane >> 4) * 4;
    for (int e0 = wave * 16; e0 < E; e0 += 64) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* yb = Y + e0 + (lane & 15);
        for (int o = 0; o < (s.t1 - s.t0) * 16; o += 16) {
            const float4 av = *(const float4*)(arow + o);
            const int k0 = s.t0 * 16 + o + (lane >> 4) * 4;
            // columns beyond B carry zero weights in dsl; clamp the address only
            const float b0 = yb[(int64_t)min(k0 + 0, B - 1) * E], b1 = yb[(int64_t)min(k0 + 1, B - 1) * E];
            const float b2 = yb[(int64_t)min(k0 + 2, B - 1) * E], b3 = yb[(int64_t)min(k0 + 3, B - 1) * E];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = i0 + (lane >> 4) * 4 + q;
            if (row < row_end) G[(int64_t)(row - first_row) * E + e0 + (lane & 15)] = acc[q];
        }
    }
}

// Normalisation backward of one row by one wave: x^ = x / |x|  =>  d x = (g - x^ (x^ . g)) / |x|, with g = the zs slices' partial rows
// (g, g + zstride, ...) added in slice order and kept in registers (E <= STRIPE_MAX_E).  ADD: added onto what d holds, else stored.
template <bool ADD>
__device__ __forceinline__ void stripe_close_row(const float* xh, const float* g, int64_t zstride, int zs,
                                                 float inv, float* d, int E, int lane) {
    float4 y[STRIPE_MAX_E / 256];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < STRIPE_MAX_E / 256; ++i) {
        const int c = (i * 64 + lane) * 4;
        y[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < E) {
            y[i] = *(const float4*)(g + c);
            for (int zz = 1; zz < zs; ++zz) {
                const float4 p = *(const float4*)(g + zz * zstride + c);
                y[i].x += p.x; y[i].y += p.y; y[i].z += p.z; y[i].w += p.w;
            }
            const float4 x = *(const float4*)(xh + c);
            dot += (x.x * y[i].x + x.y * y[i].y) + (x.z * y[i].z + x.w * y[i].w);
        }
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int i = 0; i < STRIPE_MAX_E / 256; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < E) {
            const float4 x = *(const float4*)(xh + c);
            float4 o;
            if constexpr (ADD) {
                o = *(const float4*)(d + c);
                o.x += (y[i].x - x.x * dot) * inv; o.y += (y[i].y - x.y * dot) * inv;
                o.z += (y[i].z - x.z * dot) * inv; o.w += (y[i].w - x.w * dot) * inv;
            } else {
                o = float4{(y[i].x - x.x * dot) * inv, (y[i].y - x.y * dot) * inv, (y[i].z - x.z * dot) * inv, (y[i].w - x.w * dot) * inv};
            }
            *(float4*)(d + c) = o;
        }
    }
}
