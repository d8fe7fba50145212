// Spearman rho and Pearson r of C score vectors against one vector of human ratings (gfx950): the two coefficients caption-metric work
// reports next to Kendall tau (kendall.hip).  Contract in include/dclip.h (dclip_rank_correlation).
//
//   twice-ranks   R_i = 2 L_i + Q_i + 1 with L_i = #{j : v_j < v_i}, Q_i = #{j : v_j == v_i} (i included): twice the average rank, an
//                 exact integer.  IEEE f32 comparisons: -0 == +0, +-inf order, a NaN compares false to everything (its R is 1).
//   Spearman      c_i = R_i - (n + 1); Sxy, Sxx, Syy = sums of cx cy, cx^2, cy^2 in int64 (|c_i| <= n <= 2^18, so every sum stays within
//                 2^54); rho is formed once from the three integers.  No floating-point sum before that.
//   Pearson       two passes in double over the exactly converted f32 values: the means, then the centred sums.  Every sum has a fixed
//                 shape that depends on n alone (lane partials in item order, wave tree, the workgroup's waves in order, one workgroup
//                 over the records), so the same call gives the same bits.
//
// Four launches on one stream, no atomics, plain vector stores:
//   rank_count_kernel     the O(n^2 (C + 1)) part, laid out as kendall_pairs_kernel but over the full square.  One workgroup per block of
//                         64 items: lane l of EVERY wave holds item i0 + l (the C x_i and y_i in registers); the 16 waves split the
//                         128-column tiles of j in [0, n), each wave streaming its tiles of all C + 1 vectors through a wave-private LDS
//                         tile read as broadcasts, 4 columns per ds_read_b128, the next tile's global loads in flight meanwhile.  A column
//                         j >= n of the last tile is staged as a NaN, which no comparison counts: the mask costs the walk nothing.
//                         Two comparisons per column and vector, 32-bit per-lane counters (an item meets n <= 2^18 columns).  The waves'
//                         counters are added through LDS after one barrier and R_i is stored as int32.  The ratings are one of the C + 1
//                         vectors of the walk: ranked once.
//   rank_sums_kernel<0>   min(ceil(n / 1024), 256) workgroups, one record each: the sum of every vector in double and the NaN items per column
//   rank_sums_kernel<1>   every workgroup first adds the records of <0> (the same fixed shape in each: the same means everywhere), then
//                         writes one record of the three int64 rank sums and the three centred double sums per column
//   rank_finalize_kernel  one workgroup adds the records; one thread per column forms rho and r in double, once.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int RC_ROWS = 64;                   // items per workgroup, one per lane
constexpr int RC_TILE = 128;                  // columns per wave-private LDS tile
constexpr int RC_WAVES = 16;                  // waves per workgroup: they split the column tiles
constexpr int RC_MAXC = 4;
constexpr int RC_MAXN = 1 << 18;
constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64;
constexpr int RS_PER_BLOCK = 1024;            // items per sums workgroup until the grid is capped: at most 4 items per lane at any n
constexpr int RS_MAXGRID = 256;               // one record per lane of the workgroup that adds them
// records, 8-byte slots.  <0>: sum of vector v at v (double), NaN items of column c at 5 + c (int64).
// <1>: column c at 4 c + {Sxy, Sxx (int64), sxy, sxx (double)}, Syy (int64) and syy (double) after the columns
constexpr int RS_REC0 = 16, RS_NAN = RC_MAXC + 1;
constexpr int RS_REC1 = 32, RS_SYY = 4 * RC_MAXC, RS_FYY = 4 * RC_MAXC + 1;

struct RankArgs {
    const float* x; const float* y;           // C score vectors (vector c at x + c ld) and the ratings, n floats each
    int64_t ld;
    int n, grid;                              // grid: workgroups of rank_sums_kernel
    int* ranks;                               // [C + 1][n] twice-ranks, the ratings last (out_ranks or workspace)
    long long* rec0;                          // [grid][RS_REC0] (workspace)
    long long* rec1;                          // [grid][RS_REC1] (workspace)
    double* corr;                             // [C][2]
    long long* sums;                          // [C][4] or null
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// 128 columns against this lane's item: t = the wave's LDS tile, vector v in row v
template <int V>
__device__ __forceinline__ void walk_tile(const float (*t)[RC_TILE], const float (&vi)[V], int (&lt)[V], int (&eq)[V]) {
#pragma unroll 2
    for (int jj = 0; jj < RC_TILE; jj += 4) {
        f32x4 vj[V];
#pragma unroll
        for (int v = 0; v < V; ++v) vj[v] = *(const f32x4*)&t[v][jj];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                lt[v] += vj[v][u] < vi[v] ? 1 : 0;
                eq[v] += vj[v][u] == vi[v] ? 1 : 0;
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(64 * RC_WAVES) void rank_count_kernel(RankArgs a) {
    constexpr int V = C + 1;
    __shared__ __attribute__((aligned(16))) float s_tile[RC_WAVES][V][RC_TILE];
    __shared__ int s_cnt[RC_WAVES][V][RC_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n;
    const int i = (int)blockIdx.x * RC_ROWS + lane;
    const int ic = min(i, n - 1);
    float vi[V];
#pragma unroll
    for (int c = 0; c < C; ++c) vi[c] = a.x[c * a.ld + ic];
    vi[C] = a.y[ic];
    int lt[V], eq[V];
#pragma unroll
    for (int v = 0; v < V; ++v) lt[v] = eq[v] = 0;

    // columns [0, n) in tiles of 128, tile t to wave t % RC_WAVES; a column index is clamped for the load and a column past n becomes a NaN
    const int ntile = (n + RC_TILE - 1) / RC_TILE;
    float (*tile)[RC_TILE] = s_tile[wave];
    float nxt[V][2];
    auto fetch = [&](int t) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = t * RC_TILE + h * 64 + lane, jc = min(j, n - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) nxt[c][h] = a.x[c * a.ld + jc];
            nxt[C][h] = a.y[jc];
            if (j >= n) {
#pragma unroll
                for (int v = 0; v < V; ++v) nxt[v][h] = __int_as_float(0x7fc00000);
            }
        }
    };
    if (wave < ntile) fetch(wave);
    for (int t = wave; t < ntile; t += RC_WAVES) {                 // wave-uniform
        wave_lds_fence();                                          // the reads of the previous tile are issued before it is overwritten
#pragma unroll
        for (int v = 0; v < V; ++v) {
            tile[v][lane] = nxt[v][0];
            tile[v][64 + lane] = nxt[v][1];
        }
        wave_lds_fence();
        if (t + RC_WAVES < ntile) fetch(t + RC_WAVES);
        walk_tile<V>(tile, vi, lt, eq);
    }

    // R_i - 1 = 2 L_i + Q_i is a sum over the columns, so each wave hands over its share of it: one int per vector
#pragma unroll
    for (int v = 0; v < V; ++v) s_cnt[wave][v][lane] = 2 * lt[v] + eq[v];
    __syncthreads();
    if (wave < V && i < n) {                                       // wave v adds vector v's shares over the waves
        int R = 1;
#pragma unroll
        for (int w = 0; w < RC_WAVES; ++w) R += s_cnt[w][wave][lane];
        a.ranks[(int64_t)wave * n + i] = R;
    }
}

// adds 8-byte slots over the workgroup: lanes by the xor tree, then the waves in order.  red: [RS_WAVES][NS].  Every thread returns
// with the totals readable in red[0] after the closing barrier.
template <int NK, int NF>
__device__ __forceinline__ void block_add(const long long* k, const double* f, long long (*red)[NK + NF]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const long long t = wave_sum_i64(k[s]);
        if (lane == 0) red[wave][s] = t;
    }
#pragma unroll
    for (int s = 0; s < NF; ++s) {
        const double t = wave_sum_f64(f[s]);
        if (lane == 0) red[wave][NK + s] = __double_as_longlong(t);
    }
    __syncthreads();
    if (threadIdx.x < NK) {
        long long t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < RS_WAVES; ++w) t += red[w][threadIdx.x];
        red[0][threadIdx.x] = t;
    } else if (threadIdx.x < NK + NF) {
        double t = __longlong_as_double(red[0][threadIdx.x]);
#pragma unroll
        for (int w = 1; w < RS_WAVES; ++w) t += __longlong_as_double(red[w][threadIdx.x]);
        red[0][threadIdx.x] = __double_as_longlong(t);
    }
    __syncthreads();
}

template <int C, int PASS>
__global__ __launch_bounds__(RS_THREADS) void rank_sums_kernel(RankArgs a) {
    constexpr int V = C + 1;
    constexpr int NK = PASS == 0 ? C : 2 * C + 1, NF = PASS == 0 ? V : 2 * C + 1;   // <0>: NaN items; sums.  <1>: Sxy, Sxx, .., Syy; sxy, sxx, .., syy
    __shared__ long long red[RS_WAVES][NK + NF];
    __shared__ long long red0[RS_WAVES][V];
    const int n = a.n, G = a.grid;
    long long k[NK];
    double f[NF];
#pragma unroll
    for (int s = 0; s < NK; ++s) k[s] = 0;
#pragma unroll
    for (int s = 0; s < NF; ++s) f[s] = 0.0;
    double mean[V];
    if (PASS == 1) {                                               // the means: record t of <0> to lane t, the same adds in every workgroup
        double part[V];
#pragma unroll
        for (int v = 0; v < V; ++v) part[v] = (int)threadIdx.x < G ? __longlong_as_double(a.rec0[(int64_t)threadIdx.x * RS_REC0 + v]) : 0.0;
        block_add<0, V>(nullptr, part, red0);
#pragma unroll
        for (int v = 0; v < V; ++v) mean[v] = __longlong_as_double(red0[0][v]) / (double)n;
    }
    for (int i = (int)blockIdx.x * RS_THREADS + (int)threadIdx.x; i < n; i += G * RS_THREADS) {
        const float yf = a.y[i];
        if (PASS == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float xf = a.x[c * a.ld + i];
                f[c] += (double)xf;
                k[c] += (xf != xf || yf != yf) ? 1 : 0;
            }
            f[C] += (double)yf;
        } else {
            const long long cy = a.ranks[(int64_t)C * n + i] - (n + 1);
            const double dy = (double)yf - mean[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const long long cx = a.ranks[(int64_t)c * n + i] - (n + 1);
                const double dx = (double)a.x[c * a.ld + i] - mean[c];
                k[2 * c] += cx * cy;
                k[2 * c + 1] += cx * cx;
                f[2 * c] = fma(dx, dy, f[2 * c]);
                f[2 * c + 1] = fma(dx, dx, f[2 * c + 1]);
            }
            k[2 * C] += cy * cy;
            f[2 * C] = fma(dy, dy, f[2 * C]);
        }
    }
    block_add<NK, NF>(k, f, red);
    if (PASS == 0) {
        long long* o = a.rec0 + (int64_t)blockIdx.x * RS_REC0;
        if (threadIdx.x < V) o[threadIdx.x] = red[0][NK + threadIdx.x];
        else if (threadIdx.x < V + C) o[RS_NAN + threadIdx.x - V] = red[0][threadIdx.x - V];
    } else {
        long long* o = a.rec1 + (int64_t)blockIdx.x * RS_REC1;
        const int c = threadIdx.x >> 2, q = threadIdx.x & 3;       // q: Sxy, Sxx, sxy, sxx
        if (c < C) o[4 * c + q] = red[0][q < 2 ? 2 * c + q : NK + 2 * c + q - 2];
        else if (threadIdx.x == 4 * C) o[RS_SYY] = red[0][2 * C];
        else if (threadIdx.x == 4 * C + 1) o[RS_FYY] = red[0][NK + 2 * C];
    }
}

// sqrt(v) rounded to nearest, v > 0: one residual step on the library's result (as in kendall.hip).  Both coefficients divide by ONE
// root of the product, a / sqrt(b c): for x = y that is a / sqrt(fl(a a)), which a correctly rounded root returns as a itself, so the
// coefficient is exactly 1 there (a / (sqrt(a) sqrt(a)) is one ulp off 1 for many a); elsewhere the two forms differ in the last bits.
__device__ __forceinline__ double sqrt_rn(double v) {
    const double s = sqrt(v);
    return s + fma(-s, s, v) / (2.0 * s);
}

__device__ __forceinline__ double clip1(double t) { return fmin(fmax(t, -1.0), 1.0); }

template <int C>
__global__ __launch_bounds__(RS_THREADS) void rank_finalize_kernel(RankArgs a) {
    constexpr int NK = 3 * C + 1, NF = 2 * C + 1;                  // Sxy, Sxx, NaN items per column, Syy; sxy, sxx per column, syy
    __shared__ long long red[RS_WAVES][NK + NF];
    const bool has = (int)threadIdx.x < a.grid;
    const long long* r0 = a.rec0 + (int64_t)threadIdx.x * RS_REC0;
    const long long* r1 = a.rec1 + (int64_t)threadIdx.x * RS_REC1;
    long long k[NK];
    double f[NF];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        k[3 * c] = has ? r1[4 * c] : 0;
        k[3 * c + 1] = has ? r1[4 * c + 1] : 0;
        k[3 * c + 2] = has ? r0[RS_NAN + c] : 0;
        f[2 * c] = has ? __longlong_as_double(r1[4 * c + 2]) : 0.0;
        f[2 * c + 1] = has ? __longlong_as_double(r1[4 * c + 3]) : 0.0;
    }
    k[3 * C] = has ? r1[RS_SYY] : 0;
    f[2 * C] = has ? __longlong_as_double(r1[RS_FYY]) : 0.0;
    block_add<NK, NF>(k, f, red);
    const int c = threadIdx.x;
    if (c >= C) return;
    const long long Sxy = red[0][3 * c], Sxx = red[0][3 * c + 1], nan = red[0][3 * c + 2], Syy = red[0][3 * C];
    const double sxy = __longlong_as_double(red[0][NK + 2 * c]), sxx = __longlong_as_double(red[0][NK + 2 * c + 1]);
    const double syy = __longlong_as_double(red[0][NK + 2 * C]);
    if (a.sums) {
        long long* o = a.sums + 4 * c;
        o[0] = Sxy; o[1] = Sxx; o[2] = Syy; o[3] = nan;
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __longlong_as_double(0x7ff0000000000000LL);
    double rho = qnan, r = qnan;
    if (nan == 0 && Sxx != 0 && Syy != 0) rho = clip1((double)Sxy / sqrt_rn((double)Sxx * (double)Syy));
    if (nan == 0 && sxx > 0.0 && syy > 0.0 && sxx < inf && syy < inf) r = clip1(sxy / sqrt_rn(sxx * syy));   // (an inf item: sxx is a NaN)
    a.corr[2 * c] = rho;
    a.corr[2 * c + 1] = r;
}

inline bool shape_ok(int64_t n, int64_t C) { return n >= 2 && n <= RC_MAXN && C >= 1 && C <= RC_MAXC; }
inline int sums_grid(int64_t n) {              // workgroups of rank_sums_kernel: a function of n alone
    const int64_t g = (n + RS_PER_BLOCK - 1) / RS_PER_BLOCK;
    return (int)(g < RS_MAXGRID ? g : RS_MAXGRID);
}

// workspace: the records of both sums passes, then the twice-ranks (used when the caller does not take them)
struct Carve {
    long long *rec0, *rec1; int* ranks; size_t bytes;
    Carve(void* ws, int64_t n, int64_t C) {
        Bump b(ws);
        rec0 = b.take<long long>((size_t)sums_grid(n) * RS_REC0);
        rec1 = b.take<long long>((size_t)sums_grid(n) * RS_REC1);
        ranks = b.take<int>((size_t)(C + 1) * n);
        bytes = b.off;
    }
};

template <int C>
void launch(const RankArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rank_count_kernel<C>, dim3((unsigned)((a.n + RC_ROWS - 1) / RC_ROWS)), dim3(64 * RC_WAVES), 0, st, a);
    hipLaunchKernelGGL((rank_sums_kernel<C, 0>), dim3((unsigned)a.grid), dim3(RS_THREADS), 0, st, a);
    hipLaunchKernelGGL((rank_sums_kernel<C, 1>), dim3((unsigned)a.grid), dim3(RS_THREADS), 0, st, a);
    hipLaunchKernelGGL(rank_finalize_kernel<C>, dim3(1), dim3(RS_THREADS), 0, st, a);
}

}  // namespace

extern "C" size_t dclip_rank_correlation_workspace(int64_t n, int64_t C) {
    if (!shape_ok(n, C)) return 0;
    return Carve(nullptr, n, C).bytes;
}

extern "C" int dclip_rank_correlation(const float* scores, int64_t ld, int64_t C, const float* human, int64_t n, double* out_corr,
                                      int64_t* out_sums, int32_t* out_ranks, void* ws, size_t ws_bytes, void* stream) {
    DCLIP_REQUIRE(scores && human && out_corr && ws,
                  "dclip_rank_correlation: null operand (scores, human, out_corr and workspace are required; out_sums and out_ranks may be null)");
    DCLIP_REQUIRE(n >= 2 && n <= RC_MAXN, "dclip_rank_correlation: need 2 <= n <= %d items (n=%ld)", RC_MAXN, (long)n);
    DCLIP_REQUIRE(C >= 1 && C <= RC_MAXC, "dclip_rank_correlation: need 1 <= C <= %d score vectors (C=%ld)", RC_MAXC, (long)C);
    DCLIP_REQUIRE(ld >= n, "dclip_rank_correlation: ld=%ld is below n=%ld", (long)ld, (long)n);
    DCLIP_REQUIRE(ws_bytes >= dclip_rank_correlation_workspace(n, C), "dclip_rank_correlation: workspace too small (%zu < %zu)", ws_bytes,
                  dclip_rank_correlation_workspace(n, C));
    DCLIP_REQUIRE(((uintptr_t)scores % 4) == 0 && ((uintptr_t)human % 4) == 0 && ((uintptr_t)out_corr % 8) == 0 &&
                  ((uintptr_t)out_sums % 8) == 0 && ((uintptr_t)out_ranks % 4) == 0 && dclip_aligned16(ws),
                  "dclip_rank_correlation: misaligned pointer (scores, human and out_ranks 4-byte, out_corr and out_sums 8-byte, workspace "
                  "16-byte aligned)");
    const Carve w(ws, n, C);
    RankArgs a;
    a.x = scores; a.y = human; a.ld = ld; a.n = (int)n; a.grid = sums_grid(n);
    a.ranks = out_ranks ? (int*)out_ranks : w.ranks;
    a.rec0 = w.rec0; a.rec1 = w.rec1; a.corr = out_corr; a.sums = (long long*)out_sums;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: launch<1>(a, st); break;
        case 2: launch<2>(a, st); break;
        case 3: launch<3>(a, st); break;
        default: launch<4>(a, st); break;
    }
    return dclip_check_launch("dclip_rank_correlation");
}
