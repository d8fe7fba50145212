// Intra-modal relational KL distillation (`intra_kl`), forward + backward of ONE tower (gfx950): the KL between the teacher's and the
// student's softmax over the same-modality in-batch similarities, as the uni-modal distance-preserving regulariser of DIME-FM (Sun et al.,
// ICCV 2023) and the similarity-distribution terms of relational KD.
//
//   a_ij = s^_i . s^_j / tau ; b_ij = t^_i . t^_j / tau  (j != i: the diagonal is in no sum) ; lseS_i, lseT_i their row log-sum-exps
//   p = exp(a - lseS) ; q = exp(b - lseT) ; KL_i = sum_{j != i} q_ij ((b_ij - lseT_i) - (a_ij - lseS_i)) ; intra_kl = tau^2 mean_i KL_i
//   M = p - q ; D = weight (tau / B) (M + M^T) ; G = D s^ ; d s_i = (G_i - s^_i (s^_i . G_i)) / |s_i| ; the teacher has no gradient
//
// The stripe skeleton of loss_stripes.h with TWO dot_tiles per tile (student against student, teacher against teacher: the same rows on
// both sides of the panel) and no atomics: five launches on the caller's stream,
//   normalise  one wave per row of the two matrices: x / |x| (no epsilon), 1 / |s_i| kept
//   stripe A   (16 rows, column slice): running (max, sum) of both logit rows with row == col skipped, merged over lanes and waves
//              (stripe_put / stripe_get): one lseS and one lseT partial per row and slice
//   merge      slices_lse of every row's partials into [2][B], once: stripe B needs the statistics of its 16 rows AND of every column
//   stripe B   recomputes the tiles.  The Gram matrices are symmetric, a_ji is the number a_ij, so the element of M + M^T is
//              (p_ij - q_ij) + (p_ji - q_ji) from the statistics of row i and of row j: no transposed pass.  D of the slice goes to LDS
//              ([16][columns of the slice + 4] f32, at most 33 024 bytes) and is multiplied with the student rows (stripe_times_rows):
//              one partial gradient row per slice, plain stores.  The same pass adds up q_ij (...) of its rows: one record per
//              (stripe, slice)
//   close      stripe_close_row (the slices' partial rows in slice order, the normalisation backward); one extra workgroup adds the
//              records (slices in order, then a fixed tree) and writes the four scalars
// Every store has one writer and every sum a fixed shape: the same call gives the same bits.
#include "loss_stripes.h"

namespace {

constexpr int REL_MAX_B = 4096, REL_MAX_E = 1024;
constexpr int REL_MAX_SLICES = 8;
constexpr int REL_LDS_COLS = 512;             // columns of a slice that stripe B holds in LDS: 16 x (512 + 4) f32 = 33 024 bytes
constexpr int REL_MAX_STRIPES = REL_MAX_B / 16;   // = the threads of the workgroup that adds the records
static_assert(REL_MAX_SLICES == STRIPE_MAX_SLICES && REL_MAX_E == STRIPE_MAX_E && REL_MAX_STRIPES == 256, "the shared skeleton's limits");

struct RelArgs {
    const float* src[2];                      // s, t
    float* nrm[2];                            // their normalised rows [B, E]
    float* inv;                               // 1 / |s_i|  [B]
    float* stats;                             // [zs][2][B]: lseS, lseT of a row over the columns of one slice
    float* rowst;                             // [2][B]: the slices' partials merged
    float* rec;                               // [zs][stripes]: sum over a stripe's rows of q (...) over the slice's columns
    float* dsh;                               // [zs][B, E]: the slices' partial rows of G
    float* ds;                                // d_s
    float* out;                               // 4 scalars
    int B, E, zs;
    float itau, k, tau2, weight;              // 1 / tau ; weight tau / B ; tau^2
};

// dot product / tau, rounded HERE, the fence of icl_logit (interactive.hip): without it the compiler contracts the product into the
// subtraction that follows it (x - max in stripe A, x - lse in stripe B) and the two passes would see different logits
__device__ __forceinline__ float rel_logit(float s, float itau) {
    float x = s * itau;
    asm volatile("" : "+v"(x));
    return x;
}

// x / |x| of one row per wave, no epsilon: a zero row becomes 0 * (1 / 0) = NaN in every element
__global__ __launch_bounds__(256) void rel_normalize_kernel(RelArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), mat = blockIdx.y;
    if (b >= a.B) return;
    const float inv = normalize_row<false>(a.src[mat] + (int64_t)b * a.E, a.nrm[mat] + (int64_t)b * a.E, a.E, lane);
    if (mat == 0 && lane == 0) a.inv[b] = inv;
}

// grid = (ceil(B / 16), 1, column slices)
__global__ __launch_bounds__(256) void rel_stripe_a_kernel(RelArgs a) {
    __shared__ float red[2][4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = a.B, E = a.E;
    const int i0 = blockIdx.x * 16;
    const int64_t ia = (int64_t)min(i0 + (lane & 15), B - 1) * E;  // this lane's row of the panel, clamped inside the matrix
    RunLse run[2][4];
    const int z = blockIdx.z;
    const StripeSlice sl = stripe_slice(B, a.zs, z);
    for (int jt = sl.t0 + wave; jt < sl.t1; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const int64_t jb = (int64_t)min(col, B - 1) * E;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f32x4 S = dot_tile(a.nrm[m] + ia, a.nrm[m] + jb, E, lane);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = i0 + (lane >> 4) * 4 + q;
                if (row < B && col < B && row != col) run[m][q].add(rel_logit(S[q], a.itau));
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = run[m][q].lse();
        stripe_put(red[m], v, lane, wave, LogAddExp{});
    }
    __syncthreads();
    if (threadIdx.x < 32 && i0 + (threadIdx.x & 15) < B) {
        const int m = threadIdx.x >> 4, r = threadIdx.x & 15;
        a.stats[((int64_t)z * 2 + m) * B + i0 + r] = stripe_get(red[m], r, LogAddExp{});
    }
}

// one thread per (matrix, row): the row's log-sum-exp over all columns, the slices' partials in slice order
__global__ __launch_bounds__(256) void rel_merge_kernel(RelArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * a.B) a.rowst[i] = slices_lse(a.stats + i, (int64_t)2 * a.B, a.zs);
}

__global__ __launch_bounds__(256) void rel_stripe_b_kernel(RelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dsl[];   // [16][ldl]
    __shared__ float redk[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = a.B, E = a.E;
    const int ldl = stripe_ldl(B, a.zs);                          // the LDS stripe holds this slice's columns only
    const int i0 = blockIdx.x * 16;
    const float* sh = a.nrm[0], *th = a.nrm[1];
    const int64_t ia = (int64_t)min(i0 + (lane & 15), B - 1) * E;
    float rs[4], rt[4], kl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = min(i0 + (lane >> 4) * 4 + q, B - 1);
        rs[q] = a.rowst[row]; rt[q] = a.rowst[B + row];
        kl[q] = 0.f;
    }
    const int z = blockIdx.z;
    const StripeSlice sl = stripe_slice(B, a.zs, z);
    for (int jt = sl.t0 + wave; jt < sl.t1; jt += 4) {
        const int col = jt * 16 + (lane & 15), cc = min(col, B - 1);
        const int64_t jb = (int64_t)cc * E;
        const float cs = a.rowst[cc], ct = a.rowst[B + cc];       // the statistics of row `col`: the transposed half
        const f32x4 S = dot_tile(sh + ia, sh + jb, E, lane);
        const f32x4 T = dot_tile(th + ia, th + jb, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rl = (lane >> 4) * 4 + q, row = i0 + rl;
            float d = 0.f;
            if (row < B && col < B && row != col) {
                const float x = rel_logit(S[q], a.itau), y = rel_logit(T[q], a.itau);
                const float la = x - rs[q], lb = y - rt[q];       // log p_ij, log q_ij
                const float qij = __expf(lb);
                d = a.k * ((__expf(la) - qij) + (__expf(x - cs) - __expf(y - ct)));
                kl[q] += qij * (lb - la);
            }
            dsl[rl * ldl + col - sl.t0 * 16] = d;
        }
    }
    stripe_put(redk, kl, lane, wave, StripeSum{});
    __syncthreads();
    // the record of this stripe and slice: its 16 rows' sums over the four waves, then a fixed tree over 16 lanes
    if (wave == 0 && lane < 16) {
        float v = i0 + lane < B ? stripe_get(redk, lane, StripeSum{}) : 0.f;
        v += __shfl_xor(v, 1, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 8, 16);
        if (lane == 0) a.rec[z * gridDim.x + blockIdx.x] = v;
    }
    // partial gradient rows of the slice against Y = the normalised student rows
    stripe_times_rows(dsl, ldl, sh, sl, B, E, a.dsh + (int64_t)z * B * E, i0, 0, B, lane, wave);
}

// grid = ceil(B / 4) + 1: one wave per row; the extra last workgroup adds the records (thread t holds stripe t: its slices in order, then
// a tree over the wave and over the four waves) and writes the scalars
__global__ __launch_bounds__(256) void rel_close_kernel(RelArgs a) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        const int stripes = (a.B + 15) / 16;                       // <= REL_MAX_STRIPES = blockDim.x
        float v = 0.f;
        if ((int)threadIdx.x < stripes)
            for (int z = 0; z < a.zs; ++z) v += a.rec[z * stripes + threadIdx.x];
        v = wave_sum(v);
        if (lane == 0) part[wave] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float kl = ((part[0] + part[1]) + (part[2] + part[3])) / (float)a.B;
            const float intra = a.tau2 * kl;
            a.out[0] = a.weight * intra; a.out[1] = intra; a.out[2] = kl; a.out[3] = 0.f;
        }
        return;
    }
    const int b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;
    const int64_t row = (int64_t)b * a.E;
    stripe_close_row<false>(a.nrm[0] + row, a.dsh + row, (int64_t)a.B * a.E, a.zs, a.inv[b], a.ds + row, a.E, lane);
}

bool rel_shape_ok(int64_t B, int64_t E) { return B >= 1 && B <= REL_MAX_B && E >= 16 && E <= REL_MAX_E && E % 16 == 0; }

// column slices: stripe_slices counts two workgroups (directions) per row stripe and slice, this term has one, so it is asked for half
// the row stripes; a slice stays within REL_LDS_COLS columns
int rel_slices(int64_t B) { return stripe_slices((stripe_tiles(B) + 1) / 2, stripe_tiles(B), REL_LDS_COLS); }

// carves the workspace (a null base only counts)
size_t rel_carve(RelArgs& a, void* base, int64_t B, int64_t E) {
    Bump w(base);
    const int zs = rel_slices(B);
    const size_t stripes = (size_t)stripe_tiles(B);
    for (int i = 0; i < 2; ++i) a.nrm[i] = w.take<float>((size_t)B * E);
    a.dsh = w.take<float>((size_t)zs * B * E);
    a.inv = w.take<float>((size_t)B);
    a.stats = w.take<float>((size_t)zs * 2 * B);
    a.rowst = w.take<float>((size_t)2 * B);
    a.rec = w.take<float>((size_t)zs * stripes);
    a.zs = zs;
    return w.off;
}

}  // namespace

extern "C" size_t dclip_relation_kl_workspace(int64_t B, int64_t E) {
    if (!rel_shape_ok(B, E)) return 0;
    RelArgs a;
    return rel_carve(a, nullptr, B, E);
}

extern "C" int dclip_relation_kl(const float* s, const float* t, int64_t B, int64_t E, float tau, float weight, float* out, float* d_s,
                                 void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "dclip_relation_kl";
    DCLIP_REQUIRE(B >= 1 && B <= REL_MAX_B, "%s: need 1 <= B <= 4096, got B=%ld", who, (long)B);
    DCLIP_REQUIRE(E >= 16 && E <= REL_MAX_E && E % 16 == 0, "%s: need E %% 16 == 0, 16 <= E <= 1024, got E=%ld", who, (long)E);
    DCLIP_REQUIRE(tau > 0.f && tau < INFINITY, "%s: tau must be finite and positive, got %g", who, (double)tau);
    DCLIP_REQUIRE(weight - weight == 0.f, "%s: weight must be finite, got %g", who, (double)weight);
    DCLIP_REQUIRE(s && t && out && d_s && workspace, "%s: null argument", who);
    DCLIP_REQUIRE(dclip_aligned16(s) && dclip_aligned16(t) && dclip_aligned16(out) && dclip_aligned16(d_s),
                  "%s: misaligned pointer (the embeddings, the gradient and out must be 16-byte aligned)", who);
    DCLIP_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: misaligned workspace (256 bytes)", who);
    DCLIP_REQUIRE(ws_bytes >= dclip_relation_kl_workspace(B, E), "%s: workspace too small", who);
    RelArgs a;
    rel_carve(a, workspace, B, E);
    a.src[0] = s; a.src[1] = t;
    a.ds = d_s; a.out = out;
    a.B = (int)B; a.E = (int)E;
    a.itau = 1.f / tau;
    a.k = weight * (tau / (float)B);
    a.tau2 = tau * tau;
    a.weight = weight;
    hipStream_t st = (hipStream_t)stream;
    // algorithmic HBM bytes: read 2 B E 4, write B E 4; the logits contribute none
    TraceScope tr(DCLIP_TRACE_LOSS, 0.0, 3.0 * (double)B * E * 4.0, stream);
    const unsigned stripes = (unsigned)stripe_tiles(B);
    const size_t lds = stripe_lds_bytes(a.B, a.zs);
    hipLaunchKernelGGL(rel_normalize_kernel, dim3((unsigned)((B + 3) / 4), 2), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rel_stripe_a_kernel, dim3(stripes, 1, (unsigned)a.zs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rel_merge_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rel_stripe_b_kernel, dim3(stripes, 1, (unsigned)a.zs), dim3(256), lds, st, a);
    hipLaunchKernelGGL(rel_close_kernel, dim3((unsigned)((B + 3) / 4) + 1), dim3(256), 0, st, a);
    return dclip_check_launch(who);
}
