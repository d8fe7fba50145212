// Layer-wise trust ratios (LAMB) on the table-driven layout of optim.hip (include/dclip.h: dclip_lamb_table).  One range of the table
// is one unit, normally one parameter tensor; its update u = m^ / (sqrt(v^) + eps) + wd p is scaled by r = |p| / |u|, the two L2 norms
// taken over the unit.  The norms need every element of the unit before the first parameter may move, so the step is three launches
// on one stream, with no atomics and nothing the host waits for:
//   1. lamb_moments_kernel  one workgroup per tile of the table's tile list: m', v' (adam_moments, the lines adamw_elem runs), u, and the
//                           tile's sums of p^2 and u^2 as one 16-byte record of a workspace;
//   2. lamb_ratio_kernel    one workgroup per range: the range's records added in double, the norms, r, written to stats[k];
//   3. lamb_apply_kernel    the tile list again: u once more from p, m', v' through the same lamb_update, p' = p - (lr_k r_k) u, and the EMA.
// The moments are stored by pass 1 and read back by pass 3 (8 bytes per element more than one fused pass would move): keeping u
// instead would cost the same bytes, and m', v' have to be written anyway.
#include "common.h"
#include "optim_elem.h"

#include <math.h>

namespace {

// u of one element.  The only sum that a compiler could contract is written as the fused multiply-add it would become, so pass 1 and
// pass 3 form the same bits whatever surrounds the call: a correctly rounded square root, three correctly rounded divisions-and-sum,
// one fmaf.
__device__ __forceinline__ float lamb_update(float pi, float mi, float vi, float eps, float wd, float bc1, float bc2_sqrt) {
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return fmaf(wd, pi, (mi / bc1) / denom);
}

struct LambTile { double p2, u2; };                      // one tile's sums, 16 bytes: written and read as one vector
constexpr int RATIO_LOADS = 4;                           // records a lane of lamb_ratio_kernel loads before it adds them
static_assert(sizeof(LambTile) == 16, "a tile's record is one 16-byte vector");

// the step's multiplier and bias corrections (uniform).  -> false: the loss scaler skips this step
__device__ __forceinline__ bool lamb_control(int mode, const float* __restrict__ dev, float& gs, float& bc1, float& bc2_sqrt) {
    gs = 1.f;
    if (mode == ADAMW_SCALED) gs = *dev;
    if (mode == ADAMW_AMP) {
        const float4 c = *(const float4*)dev;
        if (c.y != 0.f) return false;
        gs = c.x; bc1 = c.z; bc2_sqrt = c.w;
    }
    return true;
}

// where tile t lies: the range k, and its first float4 and float4 count inside the flat layout
struct LambSpan { int k; int64_t at, n4; };
__device__ __forceinline__ LambSpan lamb_span(const dclip_adamw_range* __restrict__ tab, int count, int64_t t) {
    const int k = table_range_of(tab, count, t);
    const int64_t first = (t - tab[k].tile0) * TABLE_TILE4;
    const int64_t left = tab[k].length / 4 - first;
    return LambSpan{k, tab[k].begin / 4 + first, left < TABLE_TILE4 ? left : TABLE_TILE4};
}

// Pass 1.  The loop is adamw4_table_kernel's: the float4 loads of the next trip are issued before the stores of the current one (vmcnt
// retires loads and stores in one in-order queue).  Rounding of the sums: a lane squares-and-adds its at most TABLE_TRIPS = 8 float4 into four f32
// accumulators per sum, one per component, by fmaf (the square is not rounded on its own), then a tree of two f32 additions; the lane's
// sum goes into a double, and the wave (xor butterfly) and the workgroup (four waves, fixed order, one barrier) add in double.
// A lane without an element in a short tile adds zeros and still meets the barrier.  A skipped step leaves the whole workgroup early
// (the flag is uniform), having written no m, v and no record.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ m,
                                                           float4* __restrict__ v, const dclip_adamw_range* __restrict__ tab, int count, float b1,
                                                           float b2, float eps, float bc1, float bc2_sqrt, int zero_grad, int mode,
                                                           const float* __restrict__ dev, LambTile* __restrict__ ws) {
    __shared__ double part[2][4];
    const int64_t t = blockIdx.x;
    if (t >= tab[count].tile0) return;                   // (a grid wider than the table's tile list)
    const LambSpan s = lamb_span(tab, count, t);
    const float wd = tab[s.k].weight_decay;
    p += s.at; g += s.at; m += s.at; v += s.at;
    const int64_t n4 = s.n4;
    int64_t i = threadIdx.x;
    float gs;
    if (!lamb_control(mode, dev, gs, bc1, bc2_sqrt)) {
        if (zero_grad)
            for (; i < n4; i += 256) g[i] = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    float4 sp = {0.f, 0.f, 0.f, 0.f}, su = {0.f, 0.f, 0.f, 0.f};
    if (i < n4) {
        float4 pi = p[i], gi = g[i], mi = m[i], vi = v[i];
        for (;;) {
            const int64_t nx = i + 256;
            const bool more = nx < n4;
            float4 pn = pi, gn = gi, mn = mi, vn = vi;
            if (more) { pn = p[nx]; gn = g[nx]; mn = m[nx]; vn = v[nx]; }
            gi.x *= gs; gi.y *= gs; gi.z *= gs; gi.w *= gs;          // (gs = 1 without a multiplier: exact)
            adam_moments(gi.x, mi.x, vi.x, b1, b2);
            adam_moments(gi.y, mi.y, vi.y, b1, b2);
            adam_moments(gi.z, mi.z, vi.z, b1, b2);
            adam_moments(gi.w, mi.w, vi.w, b1, b2);
            const float ux = lamb_update(pi.x, mi.x, vi.x, eps, wd, bc1, bc2_sqrt), uy = lamb_update(pi.y, mi.y, vi.y, eps, wd, bc1, bc2_sqrt);
            const float uz = lamb_update(pi.z, mi.z, vi.z, eps, wd, bc1, bc2_sqrt), uw = lamb_update(pi.w, mi.w, vi.w, eps, wd, bc1, bc2_sqrt);
            sp.x = fmaf(pi.x, pi.x, sp.x); sp.y = fmaf(pi.y, pi.y, sp.y); sp.z = fmaf(pi.z, pi.z, sp.z); sp.w = fmaf(pi.w, pi.w, sp.w);
            su.x = fmaf(ux, ux, su.x); su.y = fmaf(uy, uy, su.y); su.z = fmaf(uz, uz, su.z); su.w = fmaf(uw, uw, su.w);
            m[i] = mi; v[i] = vi;
            if (zero_grad) g[i] = float4{0.f, 0.f, 0.f, 0.f};
            if (!more) break;
            i = nx; pi = pn; gi = gn; mi = mn; vi = vn;
        }
    }
    double a = (double)((sp.x + sp.y) + (sp.z + sp.w)), b = (double)((su.x + su.y) + (su.z + su.w));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0)
        ws[t] = LambTile{((part[0][0] + part[0][1]) + part[0][2]) + part[0][3], ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3]};
}

// Pass 2, one workgroup per range.  Lane l adds the records tile0_k + l, + 256, ... of its range in rising order, RATIO_LOADS independent
// loads in flight per round (one wave with one load in flight took 31 us for the token table's 4626 records, measured), the lane sums meet
// in the xor butterfly and the four waves in LDS: a fixed order, all in double, where the order of a few thousand non-negative terms moves
// the sum by parts in 2^-40.
// stats[k] = {|p|, |u|, r, 0} as f32; r is the quotient of the two double norms rounded once.  r = 1 for a unit that is not decayed
// (unless always_adapt) and for a norm that is zero or not finite as f32.  A skipped step writes nothing.
__global__ __launch_bounds__(256) void lamb_ratio_kernel(const dclip_adamw_range* __restrict__ tab, int count, int64_t tiles, const LambTile* __restrict__ ws,
                                                         float trust_clip, int always_adapt, int mode, const float* __restrict__ dev,
                                                         float4* __restrict__ stats) {
    __shared__ double part[2][4];
    const int k = blockIdx.x;
    if (k >= count) return;
    if (mode == ADAMW_AMP && dev[DCLIP_AMP_SKIP] != 0.f) return;
    const int64_t t0 = tab[k].tile0;
    int64_t t1 = tab[k + 1].tile0;
    t1 = t1 < tiles ? t1 : tiles;                        // (never past the workspace, whatever the table says)
    double a = 0.0, b = 0.0;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += 256 * RATIO_LOADS) {
        LambTile r[RATIO_LOADS];                         // all loads of a round first, every one from a valid address, then the sums in rising order
#pragma unroll
        for (int j = 0; j < RATIO_LOADS; ++j) r[j] = ws[t + 256 * j < t1 ? t + 256 * j : t];
#pragma unroll
        for (int j = 0; j < RATIO_LOADS; ++j) {
            const bool in = t + 256 * j < t1;
            a += in ? r[j].p2 : 0.0; b += in ? r[j].u2 : 0.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    b = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    const double np = sqrt(a), nu = sqrt(b);
    const float npf = (float)np, nuf = (float)nu;
    float r = 1.f;
    if ((always_adapt || tab[k].weight_decay != 0.f) && npf > 0.f && nuf > 0.f && isfinite(npf) && isfinite(nuf)) r = (float)(np / nu);
    if (trust_clip >= 0.f && r > trust_clip) r = trust_clip;
    stats[k] = float4{npf, nuf, r, 0.f};
}

// Pass 3.  Reads p, m', v' (and e), forms u as pass 1 did, p' = fmaf(-(lr_k r_k), u, p) with lr_k = lr * lr_scale_k and lr_k r_k one f32
// product each.  A skipped step reads and writes nothing.
template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float4* __restrict__ p, const float4* __restrict__ m, const float4* __restrict__ v,
                                                         float4* __restrict__ e, const dclip_adamw_range* __restrict__ tab, int count, float lr,
                                                         float eps, float bc1, float bc2_sqrt, float w, int mode, const float* __restrict__ dev,
                                                         const float4* __restrict__ stats) {
    const int64_t t = blockIdx.x;
    if (t >= tab[count].tile0) return;
    const LambSpan s = lamb_span(tab, count, t);
    const int64_t n4 = s.n4;
    int64_t i = threadIdx.x;
    if (i >= n4) return;
    float gs;
    if (!lamb_control(mode, dev, gs, bc1, bc2_sqrt)) return;
    const float wd = tab[s.k].weight_decay;
    const float step = -__fmul_rn(__fmul_rn(lr, tab[s.k].lr_scale), stats[s.k].z);
    p += s.at; m += s.at; v += s.at;
    if constexpr (EMA) e += s.at;
    float4 pi = p[i], mi = m[i], vi = v[i];
    float4 ei = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ei = e[i];
    for (;;) {
        const int64_t nx = i + 256;
        const bool more = nx < n4;
        float4 pn = pi, mn = mi, vn = vi, en = ei;
        if (more) {
            pn = p[nx]; mn = m[nx]; vn = v[nx];
            if constexpr (EMA) en = e[nx];
        }
        pi.x = fmaf(step, lamb_update(pi.x, mi.x, vi.x, eps, wd, bc1, bc2_sqrt), pi.x);
        pi.y = fmaf(step, lamb_update(pi.y, mi.y, vi.y, eps, wd, bc1, bc2_sqrt), pi.y);
        pi.z = fmaf(step, lamb_update(pi.z, mi.z, vi.z, eps, wd, bc1, bc2_sqrt), pi.z);
        pi.w = fmaf(step, lamb_update(pi.w, mi.w, vi.w, eps, wd, bc1, bc2_sqrt), pi.w);
        if constexpr (EMA) { ema_elem(ei.x, pi.x, w); ema_elem(ei.y, pi.y, w); ema_elem(ei.z, pi.z, w); ema_elem(ei.w, pi.w, w); }
        p[i] = pi;
        if constexpr (EMA) e[i] = ei;
        if (!more) break;
        i = nx; pi = pn; mi = mn; vi = vn; ei = en;
    }
}

}  // namespace

extern "C" size_t dclip_lamb_workspace_bytes(int32_t count, int64_t tiles) {
    return count < 1 || tiles < count || tiles > INT32_MAX ? 0 : (size_t)tiles * sizeof(LambTile);
}

extern "C" int dclip_lamb_table(float* p, float* g, float* m, float* v, float* e, const void* table, int32_t count, int64_t tiles, float lr, float beta1,
                                float beta2, float eps, int64_t step, int zero_grad, float ema_weight, const float* gscale, const float* record,
                                float trust_clip, int always_adapt, void* workspace, size_t ws_bytes, float* stats, void* stream) {
    const char* what = "dclip_lamb_table";
    const int rc = adamw_table_operands(what, p, g, m, v, e, table, count, tiles, step, ema_weight, gscale, record);
    if (rc != DCLIP_OK) return rc;
    DCLIP_REQUIRE(trust_clip == trust_clip, "%s: trust_clip is NaN (a negative value switches the clip off)", what);
    DCLIP_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && ws_bytes >= dclip_lamb_workspace_bytes(count, tiles),
                  "%s: the workspace needs %zu bytes on a 16-byte boundary (dclip_lamb_workspace_bytes), got %zu", what, dclip_lamb_workspace_bytes(count, tiles), ws_bytes);
    DCLIP_REQUIRE(stats && ((uintptr_t)stats & 15) == 0, "%s: stats is %d x 4 f32 on a 16-byte boundary", what, (int)count);
    const AdamwControl c = adamw_control(beta1, beta2, step, gscale, record);
    const dclip_adamw_range* tab = (const dclip_adamw_range*)table;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const float4*)p, (float4*)g, (float4*)m, (float4*)v, tab, (int)count, beta1,
                       beta2, eps, c.bc1, c.bc2_sqrt, zero_grad, c.mode, c.dev, (LambTile*)workspace);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)count), dim3(256), 0, st, tab, (int)count, tiles, (const LambTile*)workspace, trust_clip, always_adapt,
                       c.mode, c.dev, (float4*)stats);
    if (!e || ema_weight == 0.f)                             // no average, or one that stands still: e neither read nor written
        hipLaunchKernelGGL(lamb_apply_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, (float4*)p, (const float4*)m, (const float4*)v, (float4*)nullptr, tab,
                           (int)count, lr, eps, c.bc1, c.bc2_sqrt, 0.f, c.mode, c.dev, (const float4*)stats);
    else
        hipLaunchKernelGGL(lamb_apply_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, (float4*)p, (const float4*)m, (const float4*)v, (float4*)e, tab,
                           (int)count, lr, eps, c.bc1, c.bc2_sqrt, ema_weight, c.mode, c.dev, (const float4*)stats);
    return dclip_check_launch(what);
}
