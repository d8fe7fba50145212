// Interactive contrastive distillation (ICL of CLIP-KD, Yang et al., CVPR 2024), forward + backward (gfx950).
//
//   A = a^ q^T / tau (student image rows against teacher text rows), C = b^ p^T / tau (student text against teacher image)
//   icl = (mean_i (lse_j A_ij - A_ii) + mean_i (lse_j C_ij - C_ii)) / 2 ; anchors are the student rows, the teacher has no gradient
//   D = weight (softmax_rows(A) - I) / (2 B tau) ; G = D q^ ; d a_i = (G_i - a^_i (a^_i . G_i)) / |a_i|        (the same of b with C, p^)
//
// The structure is that of loss.hip's cross-modal passes on the pieces of sim_tiles.h, with ONE dot_tile per tile (there is no second
// logit matrix) and no atomics: four launches on the caller's stream,
//   normalise  one wave per row of the four matrices: x / |x| (no epsilon), 1 / |x| of the student rows kept
//   stripe A   (16 rows, direction, column slice): running (max, sum) of every row with the row's TRUE maximum, merged over lanes,
//              waves (stripe_put / stripe_get) and written as one log-sum-exp per slice; the diagonal logit of every row
//   stripe B   recomputes the tiles, forms D of the slice in LDS ([16][columns of the slice + 4] f32, at most 33 024 bytes) and
//              multiplies it with the teacher rows on the f32 MFMA: one partial gradient row per slice, plain stores.  Slice 0 leaves
//              one record per stripe: sum over its rows of (lse - diagonal)
//   close      adds the slices' partial rows in slice order, does the normalisation backward; one extra workgroup adds the stripe
//              records in a fixed tree and writes the four scalars
// Every store has one writer and every sum a fixed shape: the same call gives the same bits.
#include "sim_tiles.h"
#include <math.h>

namespace {

constexpr int ICL_MAX_B = 4096, ICL_MAX_E = 1024;
constexpr int ICL_MAX_SLICES = 8;
constexpr int ICL_LDS_COLS = 512;             // columns of a slice that stripe B holds in LDS: 16 x (512 + 4) f32 = 33 024 bytes
constexpr int ICL_MAX_STRIPES = ICL_MAX_B / 16;   // = the threads of the workgroup that adds the stripe records

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

// running softmax statistic of one lane: maximum m and sum l of exp(x - m) over the values seen so far.  A NaN logit makes l NaN
// (fmaxf drops it from m) and lse() hands it on.
struct IclRun {
    float m = -INFINITY, l = 0.f;
    __device__ __forceinline__ void add(float x) {
        const float mn = fmaxf(m, x);
        l = l * __expf(m - mn) + __expf(x - mn);
        m = mn;
    }
    __device__ __forceinline__ float lse() const { return l == 0.f ? -INFINITY : m + __logf(l); }
};

// log(exp(a) + exp(b)); -inf stands for an empty sum, a NaN on either side gives NaN
struct IclLogAddExp {
    __device__ __forceinline__ float operator()(float a, float b) const {
        if (a == -INFINITY && b == -INFINITY) return a;
        const float m = fmaxf(a, b);
        return m + __logf(__expf(a - m) + __expf(b - m));
    }
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
    const int E = a.E;
    const float* src = a.src[mat] + (int64_t)b * E;
    float* dst = a.nrm[mat] + (int64_t)b * E;
    float s = 0.f;
    for (int c = lane * 4; c < E; c += 256) {
        const float4 v = *(const float4*)(src + c);
        s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    s = wave_sum(s);
    const float inv = 1.f / sqrtf(s);
    for (int c = lane * 4; c < E; c += 256) {
        const float4 v = *(const float4*)(src + c);
        *(float4*)(dst + c) = float4{v.x * inv, v.y * inv, v.z * inv, v.w * inv};
    }
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
    IclRun run[4];
    const int ntile = (B + 15) / 16;
    const int z = blockIdx.z, t0 = (int)((int64_t)ntile * z / a.zs), t1 = (int)((int64_t)ntile * (z + 1) / a.zs);
    for (int jt = t0 + wave; jt < t1; jt += 4) {
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
    stripe_put(red, v, lane, wave, IclLogAddExp{});
    __syncthreads();
    if (threadIdx.x < 16 && i0 + threadIdx.x < B)
        a.stats[((int64_t)z * 2 + dir) * B + i0 + threadIdx.x] = stripe_get(red, threadIdx.x, IclLogAddExp{});
}

// log-sum-exp of row `row` of direction `dir`: the slices' partials merged in slice order
__device__ __forceinline__ float icl_row_lse(const IclArgs& a, int dir, int row) {
    float v = -INFINITY;
    for (int zz = 0; zz < a.zs; ++zz) v = IclLogAddExp{}(v, a.stats[((int64_t)zz * 2 + dir) * a.B + row]);
    return v;
}

__global__ __launch_bounds__(256) void icl_stripe_b_kernel(IclArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dsl[];   // [16][ldl]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dir = blockIdx.y;
    const int B = a.B, E = a.E;
    const int ntile = (B + 15) / 16;
    const int ldl = ((ntile + a.zs - 1) / a.zs) * 16 + 4;         // the LDS stripe holds this slice's columns only
    const int i0 = blockIdx.x * 16;
    const float* sa = a.nrm[dir], *tb = a.nrm[3 - dir];
    const int64_t ia = (int64_t)min(i0 + (lane & 15), B - 1) * E;
    float rr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rr[q] = icl_row_lse(a, dir, min(i0 + (lane >> 4) * 4 + q, B - 1));
    const int z = blockIdx.z, t0 = (int)((int64_t)ntile * z / a.zs), t1 = (int)((int64_t)ntile * (z + 1) / a.zs);
    for (int jt = t0 + wave; jt < t1; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const int64_t jb = (int64_t)min(col, B - 1) * E;
        const f32x4 S = dot_tile(sa + ia, tb + jb, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rl = (lane >> 4) * 4 + q, row = i0 + rl;
            float d = 0.f;
            if (row < B && col < B) d = a.k * (__expf(icl_logit(S[q], a.itau) - rr[q]) - (row == col ? 1.f : 0.f));
            dsl[rl * ldl + col - t0 * 16] = d;
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
    // partial gradient rows: G[16, E] = D_stripe[16, columns of the slice] @ Y[columns, E],  Y = normalised teacher rows
    const float* Y = tb;
    float* G = a.dsh[dir] + (int64_t)z * B * E;
    const float* arow = dsl + (lane & 15) * ldl + (lane >> 4) * 4;
    for (int e0 = wave * 16; e0 < E; e0 += 64) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* yb = Y + e0 + (lane & 15);
        for (int o = 0; o < (t1 - t0) * 16; o += 16) {
            const float4 av = *(const float4*)(arow + o);
            const int k0 = t0 * 16 + o + (lane >> 4) * 4;
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
            if (row < B) G[(int64_t)row * E + e0 + (lane & 15)] = acc[q];
        }
    }
}

// normalisation backward of row b of tower `tow` by one wave: g = the slices' partial rows added in slice order,
// d x = (g - x^ (x^ . g)) / |x|
__device__ __forceinline__ void icl_close_row(const IclArgs& a, int tow, int b, int lane) {
    const int E = a.E;
    const float* xh = a.nrm[tow] + (int64_t)b * E;
    const float* g = a.dsh[tow] + (int64_t)b * E;
    float* d = a.ds[tow] + (int64_t)b * E;
    const int64_t zstride = (int64_t)a.B * E;
    float4 y[ICL_MAX_E / 256];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < ICL_MAX_E / 256; ++i) {
        const int c = (i * 64 + lane) * 4;
        y[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < E) {
            y[i] = *(const float4*)(g + c);
            for (int zz = 1; zz < a.zs; ++zz) {
                const float4 p = *(const float4*)(g + zz * zstride + c);
                y[i].x += p.x; y[i].y += p.y; y[i].z += p.z; y[i].w += p.w;
            }
            const float4 x = *(const float4*)(xh + c);
            dot += (x.x * y[i].x + x.y * y[i].y) + (x.z * y[i].z + x.w * y[i].w);
        }
    }
    dot = wave_sum(dot);
    const float inv = a.inv[tow][b];
#pragma unroll
    for (int i = 0; i < ICL_MAX_E / 256; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < E) {
            const float4 x = *(const float4*)(xh + c);
            *(float4*)(d + c) = float4{(y[i].x - x.x * dot) * inv, (y[i].y - x.y * dot) * inv,
                                       (y[i].z - x.z * dot) * inv, (y[i].w - x.w * dot) * inv};
        }
    }
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
    icl_close_row(a, 0, b, lane);
    icl_close_row(a, 1, b, lane);
}

bool icl_shape_ok(int64_t B, int64_t E) { return B >= 1 && B <= ICL_MAX_B && E >= 16 && E <= ICL_MAX_E && E % 16 == 0; }

// column slices: loss.hip's rule (enough workgroups for the chip from the row stripes, at most 8, at most one per column tile), then
// as many more as keep a slice within ICL_LDS_COLS columns
int icl_slices(int64_t B) {
    const int tiles = (int)((B + 15) / 16);
    int zs = 256 / (2 * tiles);
    zs = zs < 1 ? 1 : (zs > ICL_MAX_SLICES ? ICL_MAX_SLICES : zs);
    zs = zs > tiles ? tiles : zs;
    while (zs < ICL_MAX_SLICES && ((tiles + zs - 1) / zs) * 16 > ICL_LDS_COLS) ++zs;
    return zs;
}

// carves the workspace (a null base only counts)
size_t icl_carve(IclArgs& a, void* base, int64_t B, int64_t E) {
    Bump w(base);
    const int zs = icl_slices(B);
    const size_t stripes = (size_t)((B + 15) / 16);
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
    const unsigned stripes = (unsigned)((B + 15) / 16);
    const int cols = (((int)stripes + a.zs - 1) / a.zs) * 16;
    const size_t lds = (size_t)16 * (cols + 4) * sizeof(float);
    hipLaunchKernelGGL(icl_normalize_kernel, dim3((unsigned)((B + 3) / 4), 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(icl_stripe_a_kernel, dim3(stripes, 2, (unsigned)a.zs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(icl_stripe_b_kernel, dim3(stripes, 2, (unsigned)a.zs), dim3(256), lds, st, a);
    hipLaunchKernelGGL(icl_close_kernel, dim3((unsigned)((B + 3) / 4) + 1), dim3(256), 0, st, a);
    return dclip_check_launch(who);
}
