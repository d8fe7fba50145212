// The optimizer step's device code.  Global gradient norm for clipping (include/dclip.h: dclip_sumsq_multi, dclip_clip_coef):
// torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) with the norm and the coefficient staying on the device.  AdamW
// (dclip_adamw, dclip_adamw_multi, dclip_adamw_multi_scaled): torch.optim.AdamW on f32 ranges, optionally on g * that coefficient.
// Under a loss scaler (dclip_amp_prepare, dclip_adamw_multi_amp): the same step driven by a device record that also carries the
// scaler's 1 / scale, its overflow flag and the bias corrections of the steps that were not skipped.  An exponential moving average of the
// parameters kept by the same kernel (dclip_adamw_multi_ema), and the exchange of parameters and average in place (dclip_swap_multi).
// The table-driven form of all of these for parameter groups (dclip_adamw_table_bytes, dclip_adamw_table_fill, dclip_adamw_table): ranges
// with their own lr_scale and weight_decay as records in device memory, one launch per flat buffer.  Host side: every dclip_adamw_multi*
// entry and dclip_adamw are argument checks and one call of adamw_multi_launch; the step control (mode, bias corrections, device
// pointer) and the table entries' operand checks are optim_elem.h's, shared with lamb.hip.
#include "common.h"
#include "optim_elem.h"   // adamw_elem, ema_elem, AdamwMode, the table's tile constants and lookup, adamw_control, adamw_table_operands

#include <math.h>

#include <type_traits>

namespace {

// One workgroup tile: 256 lanes x SUMSQ_LOADS float4 (16-byte) loads, all issued before the first is used.
constexpr int SUMSQ_LOADS = 8;
constexpr int SUMSQ_TILE4 = 256 * SUMSQ_LOADS;          // float4 per tile (SUMSQ_TILE4 * 4 = 8192 elements)

struct SumsqRanges {
    const float4* g[DCLIP_ADAMW_MAX_RANGES];
    int64_t n4[DCLIP_ADAMW_MAX_RANGES];
    int64_t tile0[DCLIP_ADAMW_MAX_RANGES + 1];          // first tile of range k in the launch's tile list ; [count] = all tiles
};

// partials[b] = sum of g^2 over the tiles b, b + DCLIP_SUMSQ_PARTIALS, ... of the ranges' tile list (every range starts a new tile;
// the grid is DCLIP_SUMSQ_PARTIALS workgroups whatever the data, so each partial is the same sum in the same order on every call).
//
// Rounding: per tile a lane squares-and-adds its SUMSQ_LOADS float4 into four f32 accumulators, one per component, by fmaf (the
// square is not rounded on its own), so the longest serial f32 accumulation chain is
//     L = SUMSQ_LOADS = 8 elements,
// followed by a tree of two f32 additions.  The lane's tile sum then goes into a double, and everything after it (the lane's
// further tiles, the wave, the workgroup) is added in double; the f32 partial is one rounding of that.  HBM-bound: 4 bytes per
// element read once, 1 v_fma_f32 per element and 2 double-rate instructions per 32.
__global__ __launch_bounds__(256) void sumsq_multi_kernel(SumsqRanges r, int count, float* __restrict__ partials, int64_t n_partials) {
    __shared__ double wave_part[4];
    const int64_t tiles = r.tile0[count];
    double acc = 0.0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int k = 0;
        while (t >= r.tile0[k + 1]) ++k;                 // (uniform ; t < tile0[count] ends it inside the table)
        const float4* __restrict__ g = r.g[k];
        const int64_t n4 = r.n4[k];
        const int64_t base = (t - r.tile0[k]) * SUMSQ_TILE4 + threadIdx.x;
        float4 x[SUMSQ_LOADS];
        if ((t - r.tile0[k] + 1) * SUMSQ_TILE4 <= n4) {  // (uniform) a whole tile: eight loads back to back, no per-lane test between them
#pragma unroll
            for (int u = 0; u < SUMSQ_LOADS; ++u) x[u] = g[base + u * 256];
        } else {                                         // the range's last tile
#pragma unroll
            for (int u = 0; u < SUMSQ_LOADS; ++u) {
                const int64_t i = base + u * 256;
                x[u] = i < n4 ? g[i] : float4{0.f, 0.f, 0.f, 0.f};
            }
        }
        float4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < SUMSQ_LOADS; ++u) {
            s.x = fmaf(x[u].x, x[u].x, s.x);
            s.y = fmaf(x[u].y, x[u].y, s.y);
            s.z = fmaf(x[u].z, x[u].z, s.z);
            s.w = fmaf(x[u].w, x[u].w, s.w);
        }
        acc += (double)((s.x + s.y) + (s.z + s.w));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (float)(((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3]);
    if (blockIdx.x == 0)
        for (int64_t i = (int64_t)gridDim.x + threadIdx.x; i < n_partials; i += 256) partials[i] = 0.f;
}

// One workgroup's sum of the partials, valid in lane 0.  Lane t adds the slots t, t + 256, ... in rising index order, the 256 lane
// sums meet in a fixed tree: all in double, where the order of at most a few thousand non-negative f32 terms moves the sum by parts
// in 2^-40 — nothing the f32 results can show — and a fixed order gives every call (and every rank of a data-parallel run) the same bits.
__device__ __forceinline__ double sum_partials(const float* __restrict__ partials, int64_t n_partials, double* wave_part) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_partials; i += 256) acc += (double)partials[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

__device__ __forceinline__ float clip_coef_of(float max_norm, float norm) {
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.f ? 1.f : c;                            // (a NaN stays a NaN, like torch.clamp(max=1))
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, int64_t n_partials, const float* __restrict__ extra_sumsq,
                                                        float max_norm, float* __restrict__ out) {
    __shared__ double wave_part[4];
    double sum = sum_partials(partials, n_partials, wave_part);
    if (threadIdx.x == 0) {
        if (extra_sumsq) sum += (double)*extra_sumsq;
        const float norm = (float)sqrt(sum);
        out[0] = norm;
        out[1] = clip_coef_of(max_norm, norm);
    }
}

// beta^t for the host's powf(beta, (float)t) (adamw_control): square-and-multiply in double (a relative error below
// 2 * 24 * 2^-53 for t < 2^24, far inside the half-ulp of the f32 it is rounded to), i.e. the correctly rounded f32.  The host's powf
// is within 0.52 ulp of that: the bias corrections agree bit for bit except for a rare last bit (DESIGN.md section 7.0 counts them).
__device__ __forceinline__ float powf_int(float beta, int64_t t) {
    double b = (double)beta, r = 1.0;
    for (uint64_t e = t > 0 ? (uint64_t)(float)t : 0; e; e >>= 1) {  // ((float)t: the host's rounding of a step past 2^24)
        if (e & 1) r *= b;
        b *= b;
    }
    return (float)r;
}

// One workgroup: what the AdamW kernels of a step under a loss scaler read (include/dclip.h: dclip_amp_prepare).  clip_coef_kernel
// with the scaler's two tensors folded in: the norm is that of the unscaled gradients, the multiplier carries coefficient and
// 1 / scale in one f32, and a step that found an overflow is counted, so that the bias corrections are those of the steps taken.
__global__ __launch_bounds__(256) void amp_prepare_kernel(const float* __restrict__ found_inf, const float* __restrict__ grad_scale,
                                                          const float* __restrict__ partials, int64_t n_partials,
                                                          const float* __restrict__ extra_sumsq, float max_norm, float b1, float b2,
                                                          int64_t step, int64_t* __restrict__ skipped, float* __restrict__ rec) {
    __shared__ double wave_part[4];
    double sum = sum_partials(partials, n_partials, wave_part);      // (no clipping: n_partials = 0)
    if (threadIdx.x == 0) {
        const float gs = grad_scale ? *grad_scale : 1.f;
        const bool skip = found_inf && *found_inf != 0.f;
        float norm = 0.f, coef = 1.f;
        if (partials) {
            if (extra_sumsq) sum += (double)*extra_sumsq;
            norm = (float)(sqrt(sum) / (double)gs);
            coef = clip_coef_of(max_norm, norm);
        }
        const int64_t gone = *skipped + (skip ? 1 : 0);
        *skipped = gone;
        const int64_t t = step - gone;                               // (>= 1 on every step that is not skipped)
        rec[DCLIP_AMP_MULT] = coef / gs;
        rec[DCLIP_AMP_SKIP] = skip ? 1.f : 0.f;
        rec[DCLIP_AMP_BC1] = 1.f - powf_int(b1, t);
        rec[DCLIP_AMP_BC2_SQRT] = sqrtf(1.f - powf_int(b2, t));
        rec[DCLIP_AMP_NORM] = norm;
        rec[DCLIP_AMP_COEF] = coef;
        rec[6] = rec[7] = 0.f;
    }
}

// (adamw_elem: optim_elem.h)
// an element per thread: ranges that are misaligned, and the tail of < 4 elements of the others
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2_sqrt, int zero_grad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i];
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_elem(pi, gi, mi, vi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (zero_grad) g[i] = 0.f;                // the gradient is consumed: leave the accumulator clean for the next backward
    }
}

// float4 form, several ranges in one launch (blockIdx.y = range): the sharded data-parallel step updates one owned slice per gradient
// bucket — 9 launches of ~20 us each per step for the two l_clip students where two whole-tower launches do the same bytes.
// SCALED: on g * (*gscale), one f32 product per element before anything else uses it: the coefficient of the global-norm clipping is
// read from the device, so no host waits for the norm.
// The loads of the next grid-stride iteration are issued before the stores of the current one: vmcnt retires loads and stores in
// one in-order queue, so loads that follow stores wait for the stores' acknowledgements as well.
struct AdamwRanges { float4* p[DCLIP_ADAMW_MAX_RANGES]; float4* g[DCLIP_ADAMW_MAX_RANGES]; float4* m[DCLIP_ADAMW_MAX_RANGES]; float4* v[DCLIP_ADAMW_MAX_RANGES]; int64_t n4[DCLIP_ADAMW_MAX_RANGES]; };
// AMP: gscale points at the record of amp_prepare_kernel, whose first four floats (multiplier, skip flag, the two bias corrections:
// one 16-byte load, the same for every lane) take the place of *gscale, bc1 and bc2_sqrt.  A skipped step writes no p, m or v and
// reads nothing; the gradients, which hold an overflow, are still cleared on request.  (enum AdamwMode: optim_elem.h)
// EMA: a fifth stream e per range, the exponential moving average of the parameters, advanced with weight w = 1 - decay from the p this
// launch writes (include/dclip.h: dclip_adamw_multi_ema).  The ranges of these instantiations are a struct of their own, which also
// carries w, so that the kernel arguments of the others stay what they were.  e travels with p, m, v: loaded with the next trip's
// loads, stored with the current trip's stores, neither read nor written by a skipped step.
struct AdamwEmaRanges : AdamwRanges { float4* e[DCLIP_ADAMW_MAX_RANGES]; float w; };
// (ema_elem, e <- e + w (p - e) in two roundings: optim_elem.h)
template <int MODE, bool EMA = false>
__global__ __launch_bounds__(256) void adamw4_multi_kernel(std::conditional_t<EMA, AdamwEmaRanges, AdamwRanges> r, float lr, float b1, float b2, float eps,
                                                           float wd, float bc1, float bc2_sqrt, int zero_grad, const float* __restrict__ gscale) {
    constexpr bool SCALED = MODE != ADAMW_PLAIN;
    const int k = blockIdx.y;
    float4* __restrict__ p = r.p[k]; float4* __restrict__ g = r.g[k]; float4* __restrict__ m = r.m[k]; float4* __restrict__ v = r.v[k];
    float4* __restrict__ e = nullptr;
    float w = 0.f;
    if constexpr (EMA) { e = r.e[k]; w = r.w; }
    const int64_t n4 = r.n4[k];
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float gs = MODE == ADAMW_SCALED ? *gscale : 1.f;
    if constexpr (MODE == ADAMW_AMP) {
        const float4 c = *(const float4*)gscale;
        if (c.y != 0.f) {
            if (zero_grad)
                for (; i < n4; i += stride) g[i] = float4{0.f, 0.f, 0.f, 0.f};
            return;
        }
        gs = c.x; bc1 = c.z; bc2_sqrt = c.w;
    }
    float4 pi = p[i], gi = g[i], mi = m[i], vi = v[i];
    float4 ei = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ei = e[i];
    for (;;) {
        const int64_t nx = i + stride;
        const bool more = nx < n4;
        float4 pn = pi, gn = gi, mn = mi, vn = vi, en = ei;
        if (more) {
            pn = p[nx]; gn = g[nx]; mn = m[nx]; vn = v[nx];
            if constexpr (EMA) en = e[nx];
        }
        if (SCALED) { gi.x *= gs; gi.y *= gs; gi.z *= gs; gi.w *= gs; }
        adamw_elem(pi.x, gi.x, mi.x, vi.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.y, gi.y, mi.y, vi.y, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.z, gi.z, mi.z, vi.z, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.w, gi.w, mi.w, vi.w, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        if constexpr (EMA) { ema_elem(ei.x, pi.x, w); ema_elem(ei.y, pi.y, w); ema_elem(ei.z, pi.z, w); ema_elem(ei.w, pi.w, w); }
        p[i] = pi; m[i] = mi; v[i] = vi;
        if constexpr (EMA) e[i] = ei;
        if (zero_grad) g[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (!more) break;
        i = nx; pi = pn; gi = gn; mi = mn; vi = vn; ei = en;
    }
}

// Table-driven form (include/dclip.h: dclip_adamw_table): the ranges are records in DEVICE memory, each with its own learning-rate scale
// and weight decay, all inside one flat layout that p, g, m, v (and e) share, so one launch takes any number of them: parameter groups
// cut a student tower into several dozen ranges (weights and biases alternate), three launches and more through the 24-range entries.
// The grid is 1-D over a tile list in which every range starts a new tile, as in sumsq_multi_kernel: one workgroup per tile of
// TABLE_TRIPS trips of 256 float4.  Record k holds the first tile of its range, record `count` the number of tiles; a workgroup finds its
// range by bisection over them (uniform: scalar loads, about log2(count) of them, before the first vector load).  Inside the tile the
// loop is adamw4_multi_kernel's with a stride of one trip: the float4 loads of the next trip are issued before the stores of the current
// one, zero_grad and a skipped step are handled the same way, the arithmetic is adamw_elem / ema_elem on lr_k = lr * lr_scale_k (one
// f32 product) and wd_k.  No atomics, every element is touched by exactly one lane: the same call gives the same bits.
// (TABLE_TRIPS, TABLE_TILE4: optim_elem.h)
template <int MODE, bool EMA>
__global__ __launch_bounds__(256) void adamw4_table_kernel(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ m, float4* __restrict__ v,
                                                           float4* __restrict__ e, const dclip_adamw_range* __restrict__ tab, int count, float lr, float b1,
                                                           float b2, float eps, float bc1, float bc2_sqrt, int zero_grad, float w,
                                                           const float* __restrict__ gscale) {
    constexpr bool SCALED = MODE != ADAMW_PLAIN;
    const int64_t t = blockIdx.x;
    if (t >= tab[count].tile0) return;                   // (a grid wider than the table's tile list: nothing to do, nothing read past it)
    int lo = 0, hi = count;                              // tab[lo].tile0 <= t < tab[hi].tile0 (uniform) ; table_range_of() is these lines: calling
    while (hi - lo > 1) {                                // it here swaps the operands of one s_add_i32, so this kernel keeps its own copy
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    const int64_t first = (t - tab[lo].tile0) * TABLE_TILE4;             // float4 of the range before this tile
    const int64_t left = tab[lo].length / 4 - first;
    const int64_t n4 = left < TABLE_TILE4 ? left : TABLE_TILE4;
    const int64_t at = tab[lo].begin / 4 + first;
    lr = __fmul_rn(lr, tab[lo].lr_scale);                // (one rounding, never contracted into what follows)
    const float wd = tab[lo].weight_decay;
    p += at; g += at; m += at; v += at;
    if constexpr (EMA) e += at;
    int64_t i = threadIdx.x;
    if (i >= n4) return;
    float gs = MODE == ADAMW_SCALED ? *gscale : 1.f;
    if constexpr (MODE == ADAMW_AMP) {
        const float4 c = *(const float4*)gscale;
        if (c.y != 0.f) {
            if (zero_grad)
                for (; i < n4; i += 256) g[i] = float4{0.f, 0.f, 0.f, 0.f};
            return;
        }
        gs = c.x; bc1 = c.z; bc2_sqrt = c.w;
    }
    float4 pi = p[i], gi = g[i], mi = m[i], vi = v[i];
    float4 ei = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ei = e[i];
    for (;;) {
        const int64_t nx = i + 256;
        const bool more = nx < n4;
        float4 pn = pi, gn = gi, mn = mi, vn = vi, en = ei;
        if (more) {
            pn = p[nx]; gn = g[nx]; mn = m[nx]; vn = v[nx];
            if constexpr (EMA) en = e[nx];
        }
        if (SCALED) { gi.x *= gs; gi.y *= gs; gi.z *= gs; gi.w *= gs; }
        adamw_elem(pi.x, gi.x, mi.x, vi.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.y, gi.y, mi.y, vi.y, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.z, gi.z, mi.z, vi.z, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        adamw_elem(pi.w, gi.w, mi.w, vi.w, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        if constexpr (EMA) { ema_elem(ei.x, pi.x, w); ema_elem(ei.y, pi.y, w); ema_elem(ei.z, pi.z, w); ema_elem(ei.w, pi.w, w); }
        p[i] = pi; m[i] = mi; v[i] = vi;
        if constexpr (EMA) e[i] = ei;
        if (zero_grad) g[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (!more) break;
        i = nx; pi = pn; gi = gn; mi = mn; vi = vn; ei = en;
    }
}

template <bool EMA>
void adamw_table_launch(const AdamwControl& c, unsigned tiles, hipStream_t stream, float* p, float* g, float* m, float* v, float* e, const void* table, int count,
                        float lr, float b1, float b2, float eps, int zero_grad, float w) {
    auto kernel = c.mode == ADAMW_PLAIN ? adamw4_table_kernel<ADAMW_PLAIN, EMA> : c.mode == ADAMW_SCALED ? adamw4_table_kernel<ADAMW_SCALED, EMA> : adamw4_table_kernel<ADAMW_AMP, EMA>;
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), 0, stream, (float4*)p, (float4*)g, (float4*)m, (float4*)v, (float4*)e, (const dclip_adamw_range*)table, count,
                       lr, b1, b2, eps, c.bc1, c.bc2_sqrt, zero_grad, w, c.dev);
}

// Pairs of ranges exchanged word for word (include/dclip.h: dclip_swap_multi).  128-bit integer loads and stores and nothing between
// them: no value is ever interpreted as a float.  The grid and the order of loads and stores are those of adamw4_multi_kernel.
struct SwapRanges { uint4* a[DCLIP_ADAMW_MAX_RANGES]; uint4* b[DCLIP_ADAMW_MAX_RANGES]; int64_t n4[DCLIP_ADAMW_MAX_RANGES]; };
__global__ __launch_bounds__(256) void swap4_multi_kernel(SwapRanges r) {
    const int k = blockIdx.y;
    uint4* a = r.a[k]; uint4* b = r.b[k];                // (no __restrict__: a range may be exchanged with itself)
    const int64_t n4 = r.n4[k];
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    uint4 ai = a[i], bi = b[i];
    for (;;) {
        const int64_t nx = i + stride;
        const bool more = nx < n4;
        uint4 an = ai, bn = bi;
        if (more) { an = a[nx]; bn = b[nx]; }
        a[i] = bi; b[i] = ai;
        if (!more) break;
        i = nx; ai = an; bi = bn;
    }
}

// the ranges of a multi-range launch, checked, and its grid
int adamw_ranges(const char* what, float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count, AdamwRanges& r,
                 dim3& grid) {
    DCLIP_REQUIRE(p && g && m && v && n && count > 0 && count <= DCLIP_ADAMW_MAX_RANGES, "%s: bad argument (1..%d ranges)", what, DCLIP_ADAMW_MAX_RANGES);
    int64_t longest = 0;
    for (int k = 0; k < count; ++k) {
        DCLIP_REQUIRE(p[k] && g[k] && m[k] && v[k] && n[k] > 0 && n[k] % 4 == 0 && ((((uintptr_t)p[k] | (uintptr_t)g[k] | (uintptr_t)m[k] | (uintptr_t)v[k]) & 15) == 0),
                      "%s: range %d must be non-empty, a multiple of 4 elements and 16-byte aligned", what, k);
        r.p[k] = (float4*)p[k]; r.g[k] = (float4*)g[k]; r.m[k] = (float4*)m[k]; r.v[k] = (float4*)v[k]; r.n4[k] = n[k] / 4;
        longest = r.n4[k] > longest ? r.n4[k] : longest;
    }
    const int per_range = 8192 / count < 256 ? 256 : 8192 / count;          // (grid-stride loop: the longest range sets the width, capped)
    grid = dim3(grid_for(longest, 256, per_range), (unsigned)count);
    return DCLIP_OK;
}

// the (MODE, EMA) instantiation of adamw4_multi_kernel that `c` and the ranges' type ask for, launched
template <bool EMA, class R>
void adamw_multi_go(const AdamwControl& c, dim3 grid, hipStream_t stream, const R& r, float lr, float b1, float b2, float eps, float wd, int zero_grad) {
    auto kernel = c.mode == ADAMW_PLAIN ? adamw4_multi_kernel<ADAMW_PLAIN, EMA> : c.mode == ADAMW_SCALED ? adamw4_multi_kernel<ADAMW_SCALED, EMA> : adamw4_multi_kernel<ADAMW_AMP, EMA>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, r, lr, b1, b2, eps, wd, c.bc1, c.bc2_sqrt, zero_grad, c.dev);
}

// THE launch of adamw4_multi_kernel, behind every dclip_adamw_multi* entry and dclip_adamw: the ranges checked, and with `e` the averages;
// ema_weight == 0 (always so without e): the average stands still, the step alone, e neither read nor written.
int adamw_multi_launch(const char* what, float* const* p, float* const* g, float* const* m, float* const* v, float* const* e, const int64_t* n, int32_t count,
                       float lr, float beta1, float beta2, float eps, float weight_decay, const AdamwControl& c, int zero_grad, float ema_weight, void* stream) {
    AdamwEmaRanges r;
    dim3 grid;
    const int rc = adamw_ranges(what, p, g, m, v, n, count, r, grid);
    if (rc != DCLIP_OK) return rc;
    for (int k = 0; e && k < count; ++k) {
        DCLIP_REQUIRE(e[k] && ((uintptr_t)e[k] & 15) == 0, "%s: e of range %d must be non-NULL and 16-byte aligned", what, k);
        r.e[k] = (float4*)e[k];
    }
    r.w = ema_weight;
    if (ema_weight == 0.f)
        adamw_multi_go<false>(c, grid, (hipStream_t)stream, (const AdamwRanges&)r, lr, beta1, beta2, eps, weight_decay, zero_grad);
    else
        adamw_multi_go<true>(c, grid, (hipStream_t)stream, r, lr, beta1, beta2, eps, weight_decay, zero_grad);
    return dclip_check_launch(what);
}

}  // namespace

extern "C" int dclip_sumsq_multi(const float* const* g, const int64_t* n, int32_t count, float* partials, int64_t n_partials, void* stream) {
    DCLIP_REQUIRE(g && n && partials && count > 0 && count <= DCLIP_ADAMW_MAX_RANGES, "dclip_sumsq_multi: bad argument (1..%d ranges)", DCLIP_ADAMW_MAX_RANGES);
    DCLIP_REQUIRE(n_partials >= DCLIP_SUMSQ_PARTIALS && ((uintptr_t)partials & 3) == 0, "dclip_sumsq_multi: partials needs at least %d slots", DCLIP_SUMSQ_PARTIALS);
    SumsqRanges r;
    r.tile0[0] = 0;
    for (int k = 0; k < count; ++k) {
        DCLIP_REQUIRE(g[k] && n[k] > 0 && n[k] % 4 == 0 && ((uintptr_t)g[k] & 15) == 0,
                      "dclip_sumsq_multi: range %d must be non-empty, a multiple of 4 elements and 16-byte aligned", k);
        r.g[k] = (const float4*)g[k];
        r.n4[k] = n[k] / 4;
        r.tile0[k + 1] = r.tile0[k] + (r.n4[k] + SUMSQ_TILE4 - 1) / SUMSQ_TILE4;
    }
    for (int k = count; k < DCLIP_ADAMW_MAX_RANGES; ++k) { r.g[k] = nullptr; r.n4[k] = 0; r.tile0[k + 1] = r.tile0[count]; }
    hipLaunchKernelGGL(sumsq_multi_kernel, dim3(DCLIP_SUMSQ_PARTIALS), dim3(256), 0, (hipStream_t)stream, r, (int)count, partials, n_partials);
    return dclip_check_launch("dclip_sumsq_multi");
}

extern "C" int dclip_clip_coef(const float* partials, int64_t n_partials, const float* extra_sumsq, float max_norm, float* out, void* stream) {
    DCLIP_REQUIRE(partials && n_partials > 0 && out, "dclip_clip_coef: bad argument");
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, extra_sumsq, max_norm, out);
    return dclip_check_launch("dclip_clip_coef");
}

extern "C" int dclip_adamw_multi(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad, void* stream) {
    DCLIP_REQUIRE(step >= 1, "dclip_adamw_multi: bad argument (step >= 1)");
    return adamw_multi_launch("dclip_adamw_multi", p, g, m, v, nullptr, n, count, lr, beta1, beta2, eps, weight_decay, adamw_control(beta1, beta2, step, nullptr, nullptr),
                              zero_grad, 0.f, stream);
}

extern "C" int dclip_adamw_multi_scaled(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count,
                                        float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad,
                                        const float* gscale, void* stream) {
    DCLIP_REQUIRE(step >= 1, "dclip_adamw_multi_scaled: bad argument (step >= 1)");
    return adamw_multi_launch("dclip_adamw_multi_scaled", p, g, m, v, nullptr, n, count, lr, beta1, beta2, eps, weight_decay,
                              adamw_control(beta1, beta2, step, gscale, nullptr), zero_grad, 0.f, stream);
}

extern "C" int dclip_amp_prepare(const float* found_inf, const float* grad_scale, const float* partials, int64_t n_partials, const float* extra_sumsq,
                                 float max_norm, float beta1, float beta2, int64_t step, int64_t* skipped, float* record, void* stream) {
    DCLIP_REQUIRE(record && ((uintptr_t)record & 15) == 0 && skipped && ((uintptr_t)skipped & 7) == 0 && step >= 1,
                  "dclip_amp_prepare: bad argument (a 16-byte aligned record, an 8-byte aligned counter, step >= 1)");
    DCLIP_REQUIRE(partials ? n_partials > 0 : (n_partials == 0 && !extra_sumsq), "dclip_amp_prepare: partials and n_partials come together, extra_sumsq only with them");
    hipLaunchKernelGGL(amp_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, found_inf, grad_scale, partials, n_partials, extra_sumsq, max_norm,
                       beta1, beta2, step, skipped, record);
    return dclip_check_launch("dclip_amp_prepare");
}

extern "C" int dclip_adamw_multi_amp(float* const* p, float* const* g, float* const* m, float* const* v, const int64_t* n, int32_t count, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int zero_grad, const float* record, void* stream) {
    DCLIP_REQUIRE(record && ((uintptr_t)record & 15) == 0, "dclip_adamw_multi_amp: bad argument (a 16-byte aligned record of dclip_amp_prepare)");
    return adamw_multi_launch("dclip_adamw_multi_amp", p, g, m, v, nullptr, n, count, lr, beta1, beta2, eps, weight_decay, adamw_control(beta1, beta2, 0, nullptr, record),
                              zero_grad, 0.f, stream);
}

extern "C" int dclip_adamw_multi_ema(float* const* p, float* const* g, float* const* m, float* const* v, float* const* e, const int64_t* n, int32_t count,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, int zero_grad, float ema_weight,
                                     const float* gscale, const float* record, void* stream) {
    const char* what = "dclip_adamw_multi_ema";
    DCLIP_REQUIRE(e, "%s: bad argument (e is NULL)", what);
    DCLIP_REQUIRE(!(gscale && record), "%s: gscale (a clipped step) and record (a scaler-driven step) exclude each other", what);
    DCLIP_REQUIRE(ema_weight >= 0.f && ema_weight <= 1.f, "%s: ema_weight = 1 - decay must lie in [0, 1] (got %g)", what, (double)ema_weight);   // (a NaN fails both)
    DCLIP_REQUIRE(record ? ((uintptr_t)record & 15) == 0 : step >= 1, "%s: bad argument (a 16-byte aligned record of dclip_amp_prepare, or step >= 1)", what);
    return adamw_multi_launch(what, p, g, m, v, e, n, count, lr, beta1, beta2, eps, weight_decay, adamw_control(beta1, beta2, step, gscale, record), zero_grad,
                              ema_weight, stream);
}

extern "C" size_t dclip_adamw_table_bytes(int32_t count) { return count < 1 ? 0 : ((size_t)count + 1) * sizeof(dclip_adamw_range); }

extern "C" int dclip_adamw_table_fill(const int64_t* begin, const int64_t* length, const float* lr_scale, const float* weight_decay, int32_t count,
                                      int64_t total, void* image, size_t image_bytes, int64_t* tiles) {
    const char* what = "dclip_adamw_table_fill";
    DCLIP_REQUIRE(begin && length && lr_scale && weight_decay && image && tiles && count >= 1 && total >= 4, "%s: bad argument (count >= 1 ranges, total >= 4)", what);
    DCLIP_REQUIRE(((uintptr_t)image & 7) == 0 && image_bytes >= dclip_adamw_table_bytes(count),
                  "%s: the image needs %zu bytes on an 8-byte boundary (dclip_adamw_table_bytes)", what, dclip_adamw_table_bytes(count));
    int64_t end = 0, tile0 = 0;                              // everything is checked before the first record is written
    for (int k = 0; k < count; ++k) {
        DCLIP_REQUIRE(begin[k] >= 0 && begin[k] % 4 == 0 && length[k] > 0 && length[k] % 4 == 0,
                      "%s: range %d must be non-empty, begin and length multiples of 4 elements (begin %lld, length %lld)", what, k, (long long)begin[k], (long long)length[k]);
        DCLIP_REQUIRE(begin[k] >= end, "%s: range %d begins at %lld, inside or before range %d, which ends at %lld: ranges ascend and do not overlap", what, k,
                      (long long)begin[k], k - 1, (long long)end);
        DCLIP_REQUIRE(length[k] <= total - begin[k], "%s: range %d ends past the stated total of %lld elements", what, k, (long long)total);
        DCLIP_REQUIRE(isfinite(lr_scale[k]) && lr_scale[k] >= 0.f && isfinite(weight_decay[k]),
                      "%s: range %d needs a finite lr_scale >= 0 and a finite weight_decay (got %g, %g)", what, k, (double)lr_scale[k], (double)weight_decay[k]);
        end = begin[k] + length[k];
        tile0 += (length[k] + DCLIP_ADAMW_TABLE_TILE - 1) / DCLIP_ADAMW_TABLE_TILE;
    }
    DCLIP_REQUIRE(tile0 <= INT32_MAX, "%s: %lld tiles, more than one launch's grid", what, (long long)tile0);
    dclip_adamw_range* rec = (dclip_adamw_range*)image;
    tile0 = 0;
    for (int k = 0; k < count; ++k) {
        rec[k] = dclip_adamw_range{tile0, begin[k], length[k], lr_scale[k], weight_decay[k]};
        tile0 += (length[k] + DCLIP_ADAMW_TABLE_TILE - 1) / DCLIP_ADAMW_TABLE_TILE;
    }
    rec[count] = dclip_adamw_range{tile0, end, 0, 0.f, 0.f};
    *tiles = tile0;
    return DCLIP_OK;
}

extern "C" int dclip_adamw_table(float* p, float* g, float* m, float* v, float* e, const void* table, int32_t count, int64_t tiles, float lr, float beta1,
                                 float beta2, float eps, int64_t step, int zero_grad, float ema_weight, const float* gscale, const float* record,
                                 void* stream) {
    const char* what = "dclip_adamw_table";
    const int rc = adamw_table_operands(what, p, g, m, v, e, table, count, tiles, step, ema_weight, gscale, record);
    if (rc != DCLIP_OK) return rc;
    const AdamwControl c = adamw_control(beta1, beta2, step, gscale, record);
    if (!e || ema_weight == 0.f)                             // no average, or one that stands still: e neither read nor written
        adamw_table_launch<false>(c, (unsigned)tiles, (hipStream_t)stream, p, g, m, v, nullptr, table, count, lr, beta1, beta2, eps, zero_grad, 0.f);
    else
        adamw_table_launch<true>(c, (unsigned)tiles, (hipStream_t)stream, p, g, m, v, e, table, count, lr, beta1, beta2, eps, zero_grad, ema_weight);
    return dclip_check_launch(what);
}

extern "C" int dclip_swap_multi(float* const* a, float* const* b, const int64_t* n, int32_t count, void* stream) {
    DCLIP_REQUIRE(a && b && n && count > 0 && count <= DCLIP_ADAMW_MAX_RANGES, "dclip_swap_multi: bad argument (1..%d ranges)", DCLIP_ADAMW_MAX_RANGES);
    SwapRanges r;
    int64_t longest = 0;
    for (int k = 0; k < count; ++k) {
        DCLIP_REQUIRE(a[k] && b[k] && n[k] > 0 && n[k] % 4 == 0 && ((((uintptr_t)a[k] | (uintptr_t)b[k]) & 15) == 0),
                      "dclip_swap_multi: range %d must be non-empty, a multiple of 4 elements and 16-byte aligned", k);
        const uintptr_t lo = (uintptr_t)a[k] < (uintptr_t)b[k] ? (uintptr_t)a[k] : (uintptr_t)b[k], hi = (uintptr_t)a[k] ^ (uintptr_t)b[k] ^ lo;
        DCLIP_REQUIRE(lo == hi || hi - lo >= (uintptr_t)n[k] * sizeof(float), "dclip_swap_multi: the two sides of range %d overlap without being the same range", k);
        r.a[k] = (uint4*)a[k]; r.b[k] = (uint4*)b[k]; r.n4[k] = n[k] / 4;
        longest = r.n4[k] > longest ? r.n4[k] : longest;
    }
    const int per_pair = 8192 / count < 256 ? 256 : 8192 / count;            // (adamw_ranges' grid)
    hipLaunchKernelGGL(swap4_multi_kernel, dim3(grid_for(longest, 256, per_pair), (unsigned)count), dim3(256), 0, (hipStream_t)stream, r);
    return dclip_check_launch("dclip_swap_multi");
}

extern "C" int dclip_adamw(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int64_t step, int zero_grad, void* stream) {
    DCLIP_REQUIRE(p && g && m && v && n > 0 && step >= 1, "dclip_adamw: bad argument");
    // 16-byte aligned buffers (the flat parameter layout guarantees it; odd slices fall back): the float4 kernel, one range, for the
    // multiple-of-4 part, the scalar kernel for a tail of < 4 elements
    const AdamwControl c = adamw_control(beta1, beta2, step, nullptr, nullptr);
    int64_t done = 0;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) done = n / 4 * 4;
    if (done > 0) {
        const int rc = adamw_multi_launch("dclip_adamw", &p, &g, &m, &v, nullptr, &done, 1, lr, beta1, beta2, eps, weight_decay, c, zero_grad, 0.f, stream);
        if (rc != DCLIP_OK) return rc;
    }
    if (done < n)
        hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n - done)), dim3(256), 0, (hipStream_t)stream, p + done, g + done, m + done,
                           v + done, n - done, lr, beta1, beta2, eps, weight_decay, c.bc1, c.bc2_sqrt, zero_grad);
    return dclip_check_launch("dclip_adamw");
}
