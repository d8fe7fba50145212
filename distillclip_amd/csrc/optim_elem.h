// Per-element arithmetic and the table lookup shared by the optimizer kernels (optim.hip: AdamW; lamb.hip: the trust-ratio step).  Every
// function is forced inline: a kernel that used to hold these lines itself compiles to the instruction stream it had.  At the end, the
// host code the entries of both files share: the step control and the table entries' operand checks.
#pragma once
#include "common.h"

#include <math.h>

// how a step learns its gradient multiplier and bias corrections: none / *gscale / the record of dclip_amp_prepare
enum AdamwMode { ADAMW_PLAIN = 0, ADAMW_SCALED = 1, ADAMW_AMP = 2 };

// the two moments of Adam from the (already scaled) gradient
__device__ __forceinline__ void adam_moments(float gi, float& mi, float& vi, float b1, float b2) {
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
}

// torch.optim.AdamW semantics (decoupled weight decay; bias-corrected), reference distil_model.py:160-162
__device__ __forceinline__ void adamw_elem(float& pi, float gi, float& mi, float& vi, float lr, float b1, float b2, float eps,
                                           float wd, float bc1, float bc2_sqrt) {
    pi = pi * (1.f - lr * wd);
    adam_moments(gi, mi, vi, b1, b2);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
}

// e <- e + w (p - e): the difference rounded once, then one fmaf, two roundings in all.  p == e gives a difference of 0 and e back as it
// is (the select keeps the sign of a zero, which 0 + (-0) would lose).
__device__ __forceinline__ void ema_elem(float& ei, float pi, float w) {
    const float d = pi - ei;
    ei = d == 0.f ? ei : fmaf(w, d, ei);
}

// One tile of a table-driven launch (include/dclip.h: dclip_adamw_table_fill): TABLE_TRIPS trips of 256 float4.
constexpr int TABLE_TRIPS = DCLIP_ADAMW_TABLE_TILE / 1024;
constexpr int TABLE_TILE4 = 256 * TABLE_TRIPS;          // float4 per tile
static_assert(sizeof(dclip_adamw_range) == 32 && DCLIP_ADAMW_TABLE_TILE % 1024 == 0, "the table's record is 32 bytes, a tile whole trips");

// the range of tile t < tab[count].tile0: the k with tab[k].tile0 <= t < tab[k + 1].tile0, by bisection (uniform: scalar loads, about
// log2(count) of them)
__device__ __forceinline__ int table_range_of(const dclip_adamw_range* __restrict__ tab, int count, int64_t t) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- host side: what the entries of optim.hip and lamb.hip share before they launch ----

// How a step's kernels learn their multiplier and bias corrections: the mode, bc1 and sqrt(bc2) of `step` (0 under a scaler, whose record
// carries those of the steps taken) and the device pointer the kernels read, the record or gscale (NULL: the plain step).
struct AdamwControl { int mode; float bc1, bc2_sqrt; const float* dev; };
inline AdamwControl adamw_control(float beta1, float beta2, int64_t step, const float* gscale, const float* record) {
    if (record) return {ADAMW_AMP, 0.f, 0.f, record};
    return {gscale ? ADAMW_SCALED : ADAMW_PLAIN, 1.f - powf(beta1, (float)step), sqrtf(1.f - powf(beta2, (float)step)), gscale};
}

// the operands dclip_adamw_table and dclip_lamb_table have in common, checked
inline int adamw_table_operands(const char* what, const float* p, const float* g, const float* m, const float* v, const float* e, const void* table, int32_t count,
                                int64_t tiles, int64_t step, float ema_weight, const float* gscale, const float* record) {
    DCLIP_REQUIRE(p && g && m && v && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)e) & 15) == 0),
                  "%s: bad argument (p, g, m, v non-NULL, all bases 16-byte aligned)", what);
    DCLIP_REQUIRE(table && ((uintptr_t)table & 7) == 0 && count >= 1, "%s: bad argument (a device table on an 8-byte boundary, count >= 1)", what);
    DCLIP_REQUIRE(tiles >= count && tiles <= INT32_MAX, "%s: %lld tiles for %d ranges: every range has at least one, a launch at most 2^31 - 1", what,
                  (long long)tiles, (int)count);
    DCLIP_REQUIRE(!(gscale && record), "%s: gscale (a clipped step) and record (a scaler-driven step) exclude each other", what);
    DCLIP_REQUIRE(!e || (ema_weight >= 0.f && ema_weight <= 1.f), "%s: ema_weight = 1 - decay must lie in [0, 1] (got %g)", what, (double)ema_weight);
    DCLIP_REQUIRE(record ? ((uintptr_t)record & 15) == 0 : step >= 1, "%s: bad argument (a 16-byte aligned record of dclip_amp_prepare, or step >= 1)", what);
    return DCLIP_OK;
}
