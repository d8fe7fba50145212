// What the attention translation units share (attention.hip, attn_softmax.hip; gfx950): the sequence bound, the LDS fragment reads
// and the output epilogue of the transposed products, each written down once with its layout constants as template parameters.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int NMAX = 128;                      // max padded sequence length handled by the register-resident attention kernels

__device__ __forceinline__ bf16x8 zero_frag() {
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
    return z;
}

// k-major LDS tile fragment (16 columns from x0, 32 rows from r0): two ds_read_b64_tr_b16
template <int ROWB>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int r0, int x0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const char* a0 = tile + (r0 + 8 * g + q) * ROWB + (x0 + 4 * pp) * 2;
    union { struct { s16x4 lo, hi; } s; bf16x8 v; } u;
    u.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    u.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * ROWB));
    return u.v;
}

// output epilogue of the transposed products: the lane's 4 DT consecutive columns (attention.hip, wave_stage_perm4), scaled by s, as bf16x8 stores at o
template <int DT>
__device__ __forceinline__ void store_scaled(bf16_t* o, const f32x4 (&acc)[DT], float s) {
#pragma unroll
    for (int d = 0; d < DT; d += 2)
        *(bf16x8*)(o + d * 4) = bf16x8{f2bf(acc[d][0] * s), f2bf(acc[d][1] * s), f2bf(acc[d][2] * s), f2bf(acc[d][3] * s),
                                        f2bf(acc[d + 1][0] * s), f2bf(acc[d + 1][1] * s), f2bf(acc[d + 1][2] * s), f2bf(acc[d + 1][3] * s)};
}

}  // namespace
