// What the attention translation units share (attention.hip, attn_softmax.hip; gfx950): the sequence bound, the zero fragment
// and the output epilogue of the transposed products, each written down once with its layout constants as template parameters.  (The
// transposed LDS fragment read, tr_frag, is shared with the wgrad GEMM and lives in common.h.)
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int NMAX = 128;                      // max padded sequence length handled by the register-resident attention kernels

__device__ __forceinline__ bf16x8 zero_frag() {
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
    return z;
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
