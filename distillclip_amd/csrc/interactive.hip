// Interactive contrastive distillation (ICL of CLIP-KD, Yang et al., CVPR 2024), forward + backward (gfx950).
//
//   A = a^ q^T / tau (student image rows against teacher text rows), C = b^ p^T / tau (student text against teacher image)
//   icl = (mean_i (lse_j A_ij - A_ii) + mean_i (lse_j C_ij - C_ii)) / 2 ; anchors are the student rows, the teacher has no gradient
//   D = weight (softmax_rows(A) - I) / (2 B tau) ; G = D q^ ; d a_i = (G_i - a^_i (a^_i . G_i)) / |a_i|        (the same of b with C, p^)
//
// The stripe skeleton of loss_stripes.h (shared with loss.hip's cross-modal passes), with ONE dot_tile per tile (there is no second
// logit matrix) and no atomics: four launches on the caller's stream,
//   normalise  one wave per row of the four matrices: x / |x| (no epsilon), 1 / |x| of the student rows kept
//   stripe A   (16 rows, direction, column slice): running (max, sum) of every row with the row's TRUE maximum, merged over lanes,
//              waves (stripe_put / stripe_get) and written as one log-sum-exp per slice; the diagonal logit of every row
//   stripe B   recomputes the tiles, forms D of the slice in LDS ([16][columns of the slice + 4] f32, at most 33 024 bytes) and
//              multiplies it with the teacher rows (stripe_times_rows): one partial gradient row per slice, plain stores.  Slice 0
//              leaves one record per stripe: sum over its rows of (lse - diagonal)
//   close      stripe_close_row (the slices' partial rows in slice order, the normalisation backward); one extra workgroup adds the
//              stripe records in a fixed tree and writes the four scalars
// Every store has one writer and every sum a fixed shape: the same call gives the same bits.
#include "loss_stripes.h"

namespace {

constexpr int ICL_MAX_B = 4096, ICL_MAX_E = 1024;
constexpr int ICL_MAX_SLICES = 8;
constexpr int ICL_LDS_COLS = 512;             // columns of a slice that stripe B holds in LDS: 16 x (512 + 4) f32 = 33 024 bytes
constexpr int ICL_MAX_STRIPES = ICL_MAX_B / 16;   // = the threads of the workgroup that adds the stripe records
static_assert(ICL_MAX_SLICES == STRIPE_MAX_SLICES && ICL_MAX_E == STRIPE_MAX_E, "the shared skeleton's limits");

struct IclArgs {
    const float* src[4];                      // s_img, s_txt, t_img, t_txt
    float* nrm[4];                            // their normalised rows [B, E]
    float* inv[2];                            // 1 / |row| of s_img, s_txt  [B]
    float* stats;                             // [zs][2][B]: log-sum-exp of a row over the columns of one slice
    float* diag;                              // [2][B]: A_ii, C_ii
    float* rec;                               // [2][stripes]: sum over a stripe's rows of (lse - diagonal)
    float* dsh[2];                            // [zs][B, E]: the slices' partial rows of G
    float* ds[2];                             // d_s_img, d_s_txt
    float* out;                               // 4 scalars
    int B, E, zs;
    float itau, k, weight;                    // 1 / tau ; weight / (2 B tau)
};

// dot product / tau, rounded HERE: without the barrier the compiler contracts the product into the subtraction that follows it
// (x - max in stripe A, x - lse in stripe B), and the two passes would see different logits (B = 1 would not give P = 1 exactly)
__device__ __forceinline__ float icl_logit(float s, float itau) {
    float x = s * itau;
    asm volatile("" : "+v"(x));
    return x;
}

// x / |x| of one row per wave, no epsilon: a zero row becomes 0 * (1 / 0) = NaN in every element
__global__ __launch_bounds__(256) void icl_normalize_kernel(IclArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), mat = blockIdx.y;
    if (b >= a.B) return;
    const float inv = normalize_row<false>(a.src[mat] + (int64_t)b * a.E, a.nrm[mat] + (int64_t)b * a.E, a.E, lane);
    if (mat < 2 && lane == 0) a.inv[mat][b] = inv;
}

// grid = (ceil(B / 16), 2 directions, column slices)
__global__ __launch_bounds__(256) void icl_stripe_a_kernel(IclArgs a) {
    __shared__ float red[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dir = blockIdx.y;
    const int B = a.B, E = a.E;
    const int i0 = blockIdx.x * 16;
    const float* sa = a.nrm[dir], *tb = a.nrm[3 - dir];            // student rows / teacher columns of the other modality
    const int64_t ia = (int64_t)min(i0 + (lane & 15), B - 1) * E;  // this lane's row of the panel, clamped inside the matrix
    RunLse run[4];
    const int z = blockIdx.z;
    const StripeSlice sl = stripe_slice(B, a.zs, z);
    for (int jt = sl.t0 + wave; jt < sl.t1; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const int64_t jb = (int64_t)min(col, B - 1) * E;
        const f32x4 S = dot_tile(sa + ia, tb + jb, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = i0 + (lane >> 4) * 4 + q;
            if (row < B && col < B) {
                const float x = icl_logit(S[q], a.itau);
                run[q].add(x);
                if (row == col) a.diag[dir * B + row] = x;          // one lane of one workgroup per row
            }
        }
    }
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = run[q].lse();
    stripe_put(red, v, lane, wave, LogAddExp{});
    __syncthreads();
    if (threadIdx.x < 16 && i0 + threadIdx.x < B)
        a.stats[((int64_t)z * 2 + dir) * B + i0 + threadIdx.x] = stripe_get(red, threadIdx.x, LogAddExp{});
}

// log-sum-exp of row `row` of direction `dir`
__device__ __forceinline__ float icl_row_lse(const IclArgs& a, int dir, int row) {
    return slices_lse(a.stats + (int64_t)dir * a.B + row, (int64_t)2 * a.B, a.zs);
}

__global__ __launch_bounds__(256) void icl_stripe_b_kernel(IclArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dsl[];   // [16][ldl]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dir = blockIdx.y;
    const int B = a.B, E = a.E;
    const int ldl = stripe_ldl(B, a.zs);                          // the LDS stripe holds this slice's columns only
    const int i0 = blockIdx.x * 16;
    const float* sa = a.nrm[dir], *tb = a.nrm[3 - dir];
    const int64_t ia = (int64_t)min(i0 + (lane & 15), B - 1) * E;
    float rr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rr[q] = icl_row_lse(a, dir, min(i0 + (lane >> 4) * 4 + q, B - 1));
    const int z = blockIdx.z;
    const StripeSlice sl = stripe_slice(B, a.zs, z);
    for (int jt = sl.t0 + wave; jt < sl.t1; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const int64_t jb = (int64_t)min(col, B - 1) * E;
        const f32x4 S = dot_tile(sa + ia, tb + jb, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rl = (lane >> 4) * 4 + q, row = i0 + rl;
            float d = 0.f;
            if (row < B && col < B) d = a.k * (__expf(icl_logit(S[q], a.itau) - rr[q]) - (row == col ? 1.f : 0.f));
            dsl[rl * ldl + col - sl.t0 * 16] = d;
        }
    }
    // the stripe's record of the scalar: sum over its rows of (lse - diagonal), a fixed tree over 16 lanes
    if (z == 0 && wave == 0 && lane < 16) {
        const int row = i0 + lane;
        float v = row < B ? icl_row_lse(a, dir, row) - a.diag[dir * B + row] : 0.f;
        v += __shfl_xor(v, 1, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 8, 16);
        if (lane == 0) a.rec[dir * gridDim.x + blockIdx.x] = v;
    }
    __syncthreads();
    // partial gradient rows of the slice against Y = the normalised teacher rows
    stripe_times_rows(dsl, ldl, tb, sl, B, E, a.dsh[dir] + (int64_t)z * B * E, i0, 0, B, lane, wave);
}

// grid = ceil(B / 4) + 1: one wave per row, both towers; the extra last workgroup adds the stripe records (thread t holds record t,
// then a tree over the wave and over the four waves) and writes the scalars
__global__ __launch_bounds__(256) void icl_close_kernel(IclArgs a) {
    __shared__ float part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        const int stripes = (a.B + 15) / 16;                       // <= ICL_MAX_STRIPES = blockDim.x
        float v0 = (int)threadIdx.x < stripes ? a.rec[threadIdx.x] : 0.f;
        float v1 = (int)threadIdx.x < stripes ? a.rec[stripes + threadIdx.x] : 0.f;
        v0 = wave_sum(v0); v1 = wave_sum(v1);
        if (lane == 0) { part[0][wave] = v0; part[1][wave] = v1; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float l0 = ((part[0][0] + part[0][1]) + (part[0][2] + part[0][3])) / (float)a.B;
            const float l1 = ((part[1][0] + part[1][1]) + (part[1][2] + part[1][3])) / (float)a.B;
            const float icl = 0.5f * (l0 + l1);
            a.out[0] = a.weight * icl; a.out[1] = icl; a.out[2] = l0; a.out[3] = l1;
        }
        return;
    }
    const int b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;
    const int64_t row = (int64_t)b * a.E, zstride = (int64_t)a.B * a.E;
#pragma unroll
    for (int tow = 0; tow < 2; ++tow)
        stripe_close_row<false>(a.nrm[tow] + row, a.dsh[tow] + row, zstride, a.zs, a.inv[tow][b], a.ds[tow] + row, a.E, lane);
}

bool icl_shape_ok(int64_t B, int64_t E) { return B >= 1 && B <= ICL_MAX_B && E >= 16 && E <= ICL_MAX_E && E % 16 == 0; }

// column slices: every call owns all rows, and a slice stays within ICL_LDS_COLS columns
int icl_slices(int64_t B) { return stripe_slices(stripe_tiles(B), stripe_tiles(B), ICL_LDS_COLS); }

// carves the workspace (a null base only counts)
size_t icl_carve(IclArgs& a, void* base, int64_t B, int64_t E) {
    Bump w(base);
    const int zs = icl_slices(B);
    const size_t stripes = (size_t)stripe_tiles(B);
    for (int i = 0; i < 4; ++i) a.nrm[i] = w.take<float>((size_t)B * E);
    for (int i = 0; i < 2; ++i) a.dsh[i] = w.take<float>((size_t)zs * B * E);
    a.inv[0] = w.take<float>((size_t)B); a.inv[1] = w.take<float>((size_t)B);
    a.stats = w.take<float>((size_t)zs * 2 * B);
    a.diag = w.take<float>((size_t)2 * B);
    a.rec = w.take<float>(2 * stripes);
    a.zs = zs;
    return w.off;
}

}  // namespace

extern "C" size_t dclip_interactive_loss_workspace(int64_t B, int64_t E) {
    if (!icl_shape_ok(B, E)) return 0;
    IclArgs a;
    return icl_carve(a, nullptr, B, E);
}

extern "C" int dclip_interactive_loss(const float* s_img, const float* t_img, const float* s_txt, const float* t_txt, int64_t B,
                                      int64_t E, float tau, float weight, float* out, float* d_s_img, float* d_s_txt,
                                      void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "dclip_interactive_loss";
    DCLIP_REQUIRE(B >= 1 && B <= ICL_MAX_B, "%s: need 1 <= B <= 4096, got B=%ld", who, (long)B);
    DCLIP_REQUIRE(E >= 16 && E <= ICL_MAX_E && E % 16 == 0, "%s: need E %% 16 == 0, 16 <= E <= 1024, got E=%ld", who, (long)E);
    DCLIP_REQUIRE(tau > 0.f && tau < INFINITY, "%s: tau must be finite and positive, got %g", who, (double)tau);
    DCLIP_REQUIRE(weight - weight == 0.f, "%s: weight must be finite, got %g", who, (double)weight);
    DCLIP_REQUIRE(s_img && t_img && s_txt && t_txt && out && d_s_img && d_s_txt && workspace, "%s: null argument", who);
    DCLIP_REQUIRE(dclip_aligned16(s_img) && dclip_aligned16(t_img) && dclip_aligned16(s_txt) && dclip_aligned16(t_txt) &&
                  dclip_aligned16(out) && dclip_aligned16(d_s_img) && dclip_aligned16(d_s_txt),
                  "%s: misaligned pointer (the embeddings, the gradients and out must be 16-byte aligned)", who);
    DCLIP_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: misaligned workspace (256 bytes)", who);
    DCLIP_REQUIRE(ws_bytes >= dclip_interactive_loss_workspace(B, E), "%s: workspace too small", who);
    IclArgs a;
    icl_carve(a, workspace, B, E);
    a.src[0] = s_img; a.src[1] = s_txt; a.src[2] = t_img; a.src[3] = t_txt;
    a.ds[0] = d_s_img; a.ds[1] = d_s_txt; a.out = out;
    a.B = (int)B; a.E = (int)E;
    a.itau = 1.f / tau;
    a.k = weight * (0.5f / ((float)B * tau));
    a.weight = weight;
    hipStream_t st = (hipStream_t)stream;
    // algorithmic HBM bytes: read 4 B E 4, write 2 B E 4; the logits contribute none
    TraceScope tr(DCLIP_TRACE_LOSS, 0.0, 6.0 * (double)B * E * 4.0, stream);
    const unsigned stripes = (unsigned)stripe_tiles(B);
    const size_t lds = stripe_lds_bytes(a.B, a.zs);
    hipLaunchKernelGGL(icl_normalize_kernel, dim3((unsigned)((B + 3) / 4), 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(icl_stripe_a_kernel, dim3(stripes, 2, (unsigned)a.zs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(icl_stripe_b_kernel, dim3(stripes, 2, (unsigned)a.zs), dim3(256), lds, st, a);
    hipLaunchKernelGGL(icl_close_kernel, dim3((unsigned)((B + 3) / 4) + 1), dim3(256), 0, st, a);
    return dclip_check_launch(who);
}
