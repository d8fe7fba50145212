// Kendall tau-b and tau-c of C score vectors against one vector of human ratings (gfx950): the number a caption metric is judged by
// (CLIPScore and its successors report tau-c on Flickr8k-Expert and Composite, tau-b on Flickr8k-CF).  One pass over the n (n - 1) / 2
// unordered pairs with integer counters; no floating-point sum anywhere, so the counts are exact and the same call gives the same bits.
//
//   per pair j < i and column c (IEEE f32 comparisons: -0 == +0, +-inf order, a NaN compares false to everything):
//     con    (x_i - x_j) and (y_i - y_j) have the same non-zero sign          tie_x   x_i == x_j
//     dis    opposite non-zero signs                                          tie_y   y_i == y_j         tie_xy  both
//   per element i: dup_x / dup_y = some earlier element equals it (distinct = n - dup), nan = x_i or y_i is a NaN
//
// Two kernels on one stream, no atomics, plain vector stores:
//   kendall_pairs_kernel     one workgroup per block of 64 rows i, heaviest block first.  Lane l of EVERY wave holds row i0 + l (y_i and the
//                            C x_i in registers); the 16 waves split the 128-column tiles of j in [0, i0 + 64), each wave streaming its
//                            tiles of y and of the C score vectors through a wave-private LDS tile (the next tile's global loads are in
//                            flight while the current one is compared).  Every lane reads the same LDS address: a broadcast, conflict
//                            free, 4 columns per ds_read_b128.  Tiles wholly below the row block need no test; the tiles that reach
//                            the diagonal count a pair only when j < i, which also keeps every padded column (j >= n > i) out.
//                            Per-lane counters are 32-bit: a lane sees one row, so at most n - 1 < 2^18 pairs.  Everything summed across
//                            lanes is 64-bit.  A row has an earlier equal element exactly when its tie count, summed over the
//                            waves, is non-zero: the distinct counts cost no extra comparison.
//   kendall_finalize_kernel  one workgroup: adds the per-workgroup records, then one thread per column forms tau-b and tau-c in double
//                            from the integers, once, as scipy.stats.kendalltau defines them.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int KT_ROWS = 64;                   // rows per workgroup, one per lane
constexpr int KT_TILE = 128;                  // columns per wave-private LDS tile
constexpr int KT_WAVES = 16;                  // waves per workgroup: they split the column tiles of the row block
constexpr int KT_MAXC = 4;
constexpr int KT_MAXN = 1 << 18;
// one record of KT_REC int64 per workgroup: column c at 6 c + {con, dis, tie_x, tie_xy, dup_x, nan}; tie_y and dup_y after the columns
constexpr int KT_REC = 32;
constexpr int KT_TIE_Y = 6 * KT_MAXC, KT_DUP_Y = 6 * KT_MAXC + 1;

struct KendallArgs {
    const float* x; const float* y;           // C score vectors (vector c at x + c ld) and the ratings, n floats each
    int64_t ld;
    int n, nblk;
    long long* part;                          // [nblk][KT_REC] (workspace)
    double* tau;                              // [C][2]
    long long* counts;                        // [C][8]
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int C>
struct PairCounters {
    int both[C], dis[C], tx[C], txy[C], ty;
};

// 128 columns from j0 against this lane's row: t = the wave's LDS tile, y in row 0, x_c in row 1 + c.  DIAG: count column j only when
// j < lim (lim = the lane's row index, 0 for a row past n).
template <int C, bool DIAG>
__device__ __forceinline__ void walk_tile(const float (*t)[KT_TILE], const float (&xi)[C], float yi, int j0, int lim, PairCounters<C>& k) {
#pragma unroll 2
    for (int jj = 0; jj < KT_TILE; jj += 4) {
        const f32x4 yj = *(const f32x4*)&t[0][jj];
        f32x4 xj[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xj[c] = *(const f32x4*)&t[1 + c][jj];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = !DIAG || j0 + jj + u < lim;
            // ny / nx: ordered and different.  Among the pairs with both, the signs agree exactly when (y_i > y_j) == (x_i > x_j), so
            // `both` and `dis` are counted and con = both - dis is formed once at the end
            const bool gy = yi > yj[u], ny = ok && (yi < yj[u] || yi > yj[u]), ey = ok && yi == yj[u];
            k.ty += ey ? 1 : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool gx = xi[c] > xj[c][u], nx = xi[c] < xj[c][u] || xi[c] > xj[c][u], ex = ok && xi[c] == xj[c][u];
                const bool both = nx && ny;
                k.both[c] += both ? 1 : 0;
                k.dis[c] += (both && (gx != gy)) ? 1 : 0;
                k.tx[c] += ex ? 1 : 0;
                k.txy[c] += (ex && ey) ? 1 : 0;
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(64 * KT_WAVES) void kendall_pairs_kernel(KendallArgs a) {
    __shared__ __attribute__((aligned(16))) float s_tile[KT_WAVES][C + 1][KT_TILE];
    __shared__ int s_ties[KT_WAVES][C + 1][KT_ROWS];
    __shared__ long long s_sum[KT_WAVES][KT_REC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n;
    const int rb = a.nblk - 1 - (int)blockIdx.x;                   // the last row block has the most columns: it starts first
    const int i0 = rb * KT_ROWS, i = i0 + lane;
    const bool valid = i < n;
    const int ic = min(i, n - 1);
    float xi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xi[c] = a.x[c * a.ld + ic];
    const float yi = a.y[ic];

    PairCounters<C> k;
#pragma unroll
    for (int c = 0; c < C; ++c) k.both[c] = k.dis[c] = k.tx[c] = k.txy[c] = 0;
    k.ty = 0;

    // columns [0, i0 + 64) in tiles of 128, tile t to wave t % KT_WAVES; a column index is clamped for the load and kept out by j < i
    const int ntile = (i0 + KT_ROWS + KT_TILE - 1) / KT_TILE;
    float (*tile)[KT_TILE] = s_tile[wave];
    float nxt[C + 1][2];
    auto fetch = [&](int t) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = min(t * KT_TILE + h * 64 + lane, n - 1);
            nxt[0][h] = a.y[j];
#pragma unroll
            for (int c = 0; c < C; ++c) nxt[1 + c][h] = a.x[c * a.ld + j];
        }
    };
    if (wave < ntile) fetch(wave);
    for (int t = wave; t < ntile; t += KT_WAVES) {                        // wave-uniform
        wave_lds_fence();                                          // the reads of the previous tile are issued before it is overwritten
#pragma unroll
        for (int r = 0; r < C + 1; ++r) {
            tile[r][lane] = nxt[r][0];
            tile[r][64 + lane] = nxt[r][1];
        }
        wave_lds_fence();
        if (t + KT_WAVES < ntile) fetch(t + KT_WAVES);
        const int j0 = t * KT_TILE;
        if (j0 + KT_TILE <= i0) walk_tile<C, false>(tile, xi, yi, j0, 0, k);
        else walk_tile<C, true>(tile, xi, yi, j0, valid ? i : 0, k);
    }
    if (!valid) {                                                  // a row past n met real columns in the tiles below the diagonal
#pragma unroll
        for (int c = 0; c < C; ++c) k.both[c] = k.dis[c] = k.tx[c] = k.txy[c] = 0;
        k.ty = 0;
    }

    // per row: its ties over the waves (an earlier equal element exists iff the sum is non-zero)
#pragma unroll
    for (int c = 0; c < C; ++c) s_ties[wave][1 + c][lane] = k.tx[c];
    s_ties[wave][0][lane] = k.ty;
    if (threadIdx.x < KT_REC) {
#pragma unroll
        for (int w = 0; w < KT_WAVES; ++w) s_sum[w][threadIdx.x] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const long long con = wave_sum_i64(k.both[c] - k.dis[c]), dis = wave_sum_i64(k.dis[c]), txy = wave_sum_i64(k.txy[c]);
        if (lane == 0) { s_sum[wave][6 * c + 0] = con; s_sum[wave][6 * c + 1] = dis; s_sum[wave][6 * c + 3] = txy; }
    }
    if (wave == 0) {
        const bool ynan = yi != yi;
#pragma unroll
        for (int r = 0; r < C + 1; ++r) {
            int row = 0;
#pragma unroll
            for (int w = 0; w < KT_WAVES; ++w) row += s_ties[w][r][lane];
            const long long tie = wave_sum_i64(row), dup = wave_sum_i64(row > 0 ? 1 : 0);
            if (lane == 0) {
                if (r == 0) { s_sum[0][KT_TIE_Y] = tie; s_sum[0][KT_DUP_Y] = dup; }
                else { s_sum[0][6 * (r - 1) + 2] = tie; s_sum[0][6 * (r - 1) + 4] = dup; }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long long nan = wave_sum_i64((valid && (ynan || xi[c] != xi[c])) ? 1 : 0);
            if (lane == 0) s_sum[0][6 * c + 5] = nan;
        }
    }
    __syncthreads();
    if (threadIdx.x < KT_REC) {
        const int s = threadIdx.x;
        long long v = 0;
#pragma unroll
        for (int w = 0; w < KT_WAVES; ++w) v += s_sum[w][s];
        a.part[(int64_t)blockIdx.x * KT_REC + s] = v;
    }
}

// sqrt(v) rounded to nearest, v >= 1: one residual step on the library's result.  tau_b divides by sqrt((n0 - tie_x) (n0 - tie_y)), one
// root of the product: for x = y that is sqrt(fl(a a)), which a correctly rounded root returns as a itself, so tau_b is exactly 1 there
// (a / sqrt(a) / sqrt(a) is one ulp off 1 for many a); elsewhere the two forms differ in the last bits only.
__device__ __forceinline__ double sqrt_rn(double v) {
    const double s = sqrt(v);
    return s + fma(-s, s, v) / (2.0 * s);
}

__device__ __forceinline__ double clip1(double t) { return fmin(fmax(t, -1.0), 1.0); }     // (a NaN stays a NaN: neither branch of either is taken)

template <int C>
__global__ __launch_bounds__(256) void kendall_finalize_kernel(KendallArgs a) {
    __shared__ long long red[8][KT_REC];
    __shared__ long long tot[KT_REC];
    const int s = threadIdx.x & (KT_REC - 1), g = threadIdx.x / KT_REC;
    long long v = 0;
    for (int b = g; b < a.nblk; b += 8) v += a.part[(int64_t)b * KT_REC + s];
    red[g][s] = v;
    __syncthreads();
    if (threadIdx.x < KT_REC) {
        long long t = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[q][s];
        tot[s] = t;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= C) return;
    const long long n = a.n, n0 = n * (n - 1) / 2;
    const long long con = tot[6 * c], dis = tot[6 * c + 1], tx = tot[6 * c + 2], txy = tot[6 * c + 3], nan = tot[6 * c + 5];
    const long long ty = tot[KT_TIE_Y], dx = n - tot[6 * c + 4], dy = n - tot[KT_DUP_Y];
    long long* o = a.counts + 8 * c;
    o[0] = con; o[1] = dis; o[2] = tx; o[3] = ty; o[4] = txy; o[5] = dx; o[6] = dy; o[7] = nan;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double cmd = (double)(con - dis);
    const long long m = min(dx, dy);
    double tb = qnan, tc = qnan;
    if (nan == 0 && tx != n0 && ty != n0) tb = clip1(cmd / sqrt_rn((double)(n0 - tx) * (double)(n0 - ty)));
    if (nan == 0 && m > 1) tc = clip1(2.0 * cmd / ((double)(n * n * (m - 1)) / (double)m));
    a.tau[2 * c] = tb;
    a.tau[2 * c + 1] = tc;
}

inline bool shape_ok(int64_t n, int64_t C) { return n >= 2 && n <= KT_MAXN && C >= 1 && C <= KT_MAXC; }
inline int64_t row_blocks(int64_t n) { return (n + KT_ROWS - 1) / KT_ROWS; }

template <int C>
void launch(const KendallArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(kendall_pairs_kernel<C>, dim3((unsigned)a.nblk), dim3(64 * KT_WAVES), 0, st, a);
    hipLaunchKernelGGL(kendall_finalize_kernel<C>, dim3(1), dim3(256), 0, st, a);
}

}  // namespace

extern "C" size_t dclip_kendall_tau_workspace(int64_t n, int64_t C) {
    if (!shape_ok(n, C)) return 0;
    return dclip_up256((size_t)row_blocks(n) * KT_REC * sizeof(long long));
}

extern "C" int dclip_kendall_tau(const float* scores, int64_t ld, int64_t C, const float* human, int64_t n, double* out_tau, int64_t* out_counts,
                                 void* ws, size_t ws_bytes, void* stream) {
    DCLIP_REQUIRE(scores && human && out_tau && out_counts && ws,
                  "dclip_kendall_tau: null operand (scores, human, out_tau, out_counts and workspace are required)");
    DCLIP_REQUIRE(n >= 2 && n <= KT_MAXN, "dclip_kendall_tau: need 2 <= n <= %d items (n=%ld)", KT_MAXN, (long)n);
    DCLIP_REQUIRE(C >= 1 && C <= KT_MAXC, "dclip_kendall_tau: need 1 <= C <= %d score vectors (C=%ld)", KT_MAXC, (long)C);
    DCLIP_REQUIRE(ld >= n, "dclip_kendall_tau: ld=%ld is below n=%ld", (long)ld, (long)n);
    DCLIP_REQUIRE(ws_bytes >= dclip_kendall_tau_workspace(n, C), "dclip_kendall_tau: workspace too small (%zu < %zu)", ws_bytes,
                  dclip_kendall_tau_workspace(n, C));
    DCLIP_REQUIRE(((uintptr_t)scores % 4) == 0 && ((uintptr_t)human % 4) == 0 && ((uintptr_t)out_tau % 8) == 0 &&
                  ((uintptr_t)out_counts % 8) == 0 && dclip_aligned16(ws),
                  "dclip_kendall_tau: misaligned pointer (scores and human 4-byte, out_tau and out_counts 8-byte, workspace 16-byte aligned)");
    KendallArgs a;
    a.x = scores; a.y = human; a.ld = ld; a.n = (int)n; a.nblk = (int)row_blocks(n);
    a.part = (long long*)ws; a.tau = out_tau; a.counts = (long long*)out_counts;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: launch<1>(a, st); break;
        case 2: launch<2>(a, st); break;
        case 3: launch<3>(a, st); break;
        default: launch<4>(a, st); break;
    }
    return dclip_check_launch("dclip_kendall_tau");
}
