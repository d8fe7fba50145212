// Head-mean attention maps for the attention_score_mse / attention_probs_mse distillation terms (reference
// model/loss_component/attention_score_mse.py, attention_probs_mse.py: both reduce every exported map to sum(dim=1) / H before the MSE).
//   student (weight_share_model.py:101-121): S = (q scale) k^T before conv_l ; P = softmax(conv_l(S)) before conv_w
//   CLIP    (_common.py:73-94, text_encoder.py:81-85): S = q k^T / sqrt(hd) + mask, masked scores read as 0 ; P = softmax(S + mask)
// Only the head means leave the chip: one f32 [B, N, N] map per exported layer and kind.  Separate kernels from the score stage itself
// (attention.hip / attention_mix.hip): they recompute S from the packed qkv rows the score stage read, so the default step is unchanged
// when no map is asked for.
//
// Layout: one workgroup per (sample, TQ = 4 query rows), one wave per row.  Per head, K_h (f32, rows padded to hd + 4) and the tile's Q rows go to
// LDS and S_h of the tile is formed there; every head's S stays in LDS, because conv_l mixes all heads of a (query, key) element.  A wave
// then owns its row: lane l holds keys l and l + 64 (N <= 128).  No atomics: the dW_l partials of the backward are one [H, H] tile per
// workgroup, summed in a fixed order by a second launch.
#include <math.h>
#include "common.h"

namespace {

constexpr int TQ = 4;            // query rows per workgroup (one wave each)
constexpr int MAPS_NMAX = 128;
constexpr size_t MAPS_LDS_MAX = 160 * 1024;

struct MapsArgs {
    const bf16_t* qkv; int64_t ld;
    const float* Wl;             // [H, H] conv_l weight or null
    float* score; float* prob;   // forward: [B, N, N] head means (nullable)
    const float* gS; const float* gP;   // backward: their gradients (nullable)
    bf16_t* dS; int blocked;     // backward: gradient of the scaled pre-mix scores, quad-blocked or row-major [B, H, N, Np]
    float* part;                 // backward: [workgroups, H, H] dW_l partials (null = no dW_l)
    int B, H, N, Np, hd, causal;
    float scale;
};

__host__ __device__ inline size_t maps_lds_floats(int H, int N, int hd, bool wl, bool two) {
    return (size_t)N * (hd + 4) + (size_t)TQ * hd + (two ? 2 : 1) * (size_t)H * TQ * N + (wl ? (size_t)H * H : 0);
}

// S[h][i][j] (f32, LDS, [H][TQ][N]) = scale * q_h(i0 + i) . k_h(j); rows past N are zero.  Ends with a barrier.
__device__ void tile_scores(const MapsArgs& a, int b, int i0, float* Ks, float* Qs, float* S) {
    const int N = a.N, hd = a.hd, D = a.H * hd, tid = threadIdx.x, kst = hd + 4, v8 = hd / 8;      // K rows padded, 16-byte aligned
    for (int h = 0; h < a.H; ++h) {
        __syncthreads();                                           // the previous head's K / Q reads are done
        for (int v = tid; v < N * v8; v += 256) {
            const int j = v / v8, d0 = (v % v8) * 8;
            const bf16x8 x = *(const bf16x8*)(a.qkv + (int64_t)(b * N + j) * a.ld + D + h * hd + d0);
            *(f32x4*)(Ks + j * kst + d0) = f32x4{(float)x[0], (float)x[1], (float)x[2], (float)x[3]};
            *(f32x4*)(Ks + j * kst + d0 + 4) = f32x4{(float)x[4], (float)x[5], (float)x[6], (float)x[7]};
        }
        for (int v = tid; v < TQ * v8; v += 256) {
            const int i = v / v8, d0 = (v % v8) * 8;
            if (i0 + i < N) {
                const bf16x8 x = *(const bf16x8*)(a.qkv + (int64_t)(b * N + i0 + i) * a.ld + h * hd + d0);
#pragma unroll
                for (int u = 0; u < 8; ++u) Qs[i * hd + d0 + u] = (float)x[u];
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) Qs[i * hd + d0 + u] = 0.f;
            }
        }
        __syncthreads();
        for (int e = tid; e < TQ * N; e += 256) {
            const int i = e / N, j = e - i * N;
            const f32x4* q = (const f32x4*)(Qs + i * hd);
            const f32x4* k = (const f32x4*)(Ks + j * kst);
            float acc = 0.f;
            for (int d = 0; d < hd / 4; ++d) {
                const f32x4 x = q[d], y = k[d];
                acc = fmaf(x[0], y[0], acc);
                acc = fmaf(x[1], y[1], acc);
                acc = fmaf(x[2], y[2], acc);
                acc = fmaf(x[3], y[3], acc);
            }
            S[(h * TQ + i) * N + j] = acc * a.scale;
        }
    }
    __syncthreads();
}

// row softmax of head g's mixed scores over the lane's two keys: p[] (0 where masked / past N)
__device__ inline void row_probs(const MapsArgs& a, const float* S, const float* W, int g, int w, int i, int lane, float p[2]) {
    const int H = a.H, N = a.N;
    float x[2];
    bool ok[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int j = lane + 64 * jj;
        ok[jj] = j < N && !(a.causal && j > i);
        float v = -INFINITY;
        if (ok[jj]) {
            if (W) {
                v = 0.f;
                for (int h = 0; h < H; ++h) v = fmaf(W[g * H + h], S[(h * TQ + w) * N + j], v);
            } else {
                v = S[(g * TQ + w) * N + j];
            }
        }
        x[jj] = v;
    }
    const float m = wave_max(fmaxf(x[0], x[1]));
    const float e0 = ok[0] ? __expf(x[0] - m) : 0.f, e1 = ok[1] ? __expf(x[1] - m) : 0.f;
    const float r = 1.f / wave_sum(e0 + e1);
    p[0] = e0 * r;
    p[1] = e1 * r;
}

__device__ inline int64_t ds_index(const MapsArgs& a, int b, int h, int i, int j) {
    const int64_t base = ((int64_t)b * a.H + h) * a.N * a.Np;
    return a.blocked ? base + ((int64_t)(j >> 2) * a.N + i) * 4 + (j & 3) : base + (int64_t)i * a.Np + j;
}

__global__ __launch_bounds__(256) void attn_maps_fwd_kernel(MapsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, i0 = blockIdx.x * TQ, H = a.H, N = a.N, tid = threadIdx.x;
    float* Ks = lds;
    float* Qs = Ks + N * (a.hd + 4);
    float* S = Qs + TQ * a.hd;
    float* W = a.Wl ? S + H * TQ * N : nullptr;
    if (W)
        for (int t = tid; t < H * H; t += 256) W[t] = a.Wl[t];
    tile_scores(a, b, i0, Ks, Qs, S);
    const int w = tid >> 6, lane = tid & 63, i = i0 + w;
    if (i >= N) return;                                            // no barrier below
    const float invH = 1.f / (float)H;
    const int64_t row = ((int64_t)b * N + i) * N;
    if (a.score) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = lane + 64 * jj;
            if (j >= N) continue;
            float s = 0.f;
            for (int h = 0; h < H; ++h) s += S[(h * TQ + w) * N + j];
            a.score[row + j] = (a.causal && j > i) ? 0.f : s * invH;
        }
    }
    if (a.prob) {
        float acc[2] = {0.f, 0.f};
        for (int g = 0; g < H; ++g) {
            float p[2];
            row_probs(a, S, W, g, w, i, lane, p);
            acc[0] += p[0];
            acc[1] += p[1];
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = lane + 64 * jj;
            if (j < N) a.prob[row + j] = acc[jj] * invH;
        }
    }
}

// dS[h] += gS / H + (Wl^T dA)[h],  dA[g] = P[g] o (gP / H - rowsum(P[g] o gP / H))   (no Wl: the identity mix)
__global__ __launch_bounds__(256) void attn_maps_bwd_kernel(MapsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, i0 = blockIdx.x * TQ, H = a.H, N = a.N, tid = threadIdx.x;
    const bool mixed = a.Wl && a.gP;
    float* Ks = lds;
    float* Qs = Ks + N * (a.hd + 4);
    float* S = Qs + TQ * a.hd;
    float* dA = mixed ? S + H * TQ * N : nullptr;
    float* W = mixed ? dA + H * TQ * N : nullptr;
    if (W)
        for (int t = tid; t < H * H; t += 256) W[t] = a.Wl[t];
    if (a.gP) tile_scores(a, b, i0, Ks, Qs, S);
    const int w = tid >> 6, lane = tid & 63, i = i0 + w;
    const float invH = 1.f / (float)H;
    const int64_t row = ((int64_t)b * N + i) * N;
    float gs[2] = {0.f, 0.f}, gp[2] = {0.f, 0.f};
    if (i < N) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = lane + 64 * jj;
            if (j < N && !(a.causal && j > i)) {           // masked entries get no gradient
                if (a.gS) gs[jj] = a.gS[row + j] * invH;
                if (a.gP) gp[jj] = a.gP[row + j] * invH;
            }
        }
    }
    auto add_ds = [&](int h, int jj, float v) {
        const int j = lane + 64 * jj;
        if (j >= N) return;
        bf16_t* d = a.dS + ds_index(a, b, h, i, j);
        *d = f2bf(bf2f(*d) + v);
    };
    if (a.gP) {
        for (int g = 0; g < H; ++g) {
            float da[2] = {0.f, 0.f};
            if (i < N) {                                   // wave-uniform
                float p[2];
                row_probs(a, S, W, g, w, i, lane, p);
                const float r = wave_sum(p[0] * gp[0] + p[1] * gp[1]);
                da[0] = p[0] * (gp[0] - r);
                da[1] = p[1] * (gp[1] - r);
            }
            if (mixed) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = lane + 64 * jj;
                    if (j < N) dA[(g * TQ + w) * N + j] = da[jj];
                }
            } else if (i < N) {
                add_ds(g, 0, da[0] + gs[0]);
                add_ds(g, 1, da[1] + gs[1]);
            }
        }
    } else if (i < N) {
        for (int h = 0; h < H; ++h) {
            add_ds(h, 0, gs[0]);
            add_ds(h, 1, gs[1]);
        }
    }
    if (!mixed) return;
    __syncthreads();
    if (i < N) {
        for (int h = 0; h < H; ++h) {
            float v[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = lane + 64 * jj;
                float s = gs[jj];
                if (j < N)
                    for (int g = 0; g < H; ++g) s = fmaf(W[g * H + h], dA[(g * TQ + w) * N + j], s);
                v[jj] = s;
            }
            add_ds(h, 0, v[0]);
            add_ds(h, 1, v[1]);
        }
    }
    if (a.part) {                                          // dW_l[g, h] partial = sum over the tile of dA_g S_h (rows past N: dA = 0)
        const int rows = min(TQ, N - i0), ne = rows * N;
        float* out = a.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * H * H;
        for (int gh = tid; gh < H * H; gh += 256) {
            const float* x = dA + (gh / H) * TQ * N;
            const float* y = S + (gh % H) * TQ * N;
            float acc = 0.f;
            for (int e = 0; e < ne; ++e) acc = fmaf(x[e], y[e], acc);
            out[gh] = acc;
        }
    }
}

// dWl[gh] += sum over workgroups of part[wg][gh], in a fixed order
__global__ __launch_bounds__(256) void attn_maps_dwl_reduce_kernel(const float* part, float* dWl, int nwg, int HH) {
    __shared__ float red[256];
    const int gh = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int k = tid; k < nwg; k += 256) s += part[(int64_t)k * HH + gh];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dWl[gh] += red[0];
}

int check_common(const char* who, const void* qkv, int64_t ld, int64_t B, int64_t H, int64_t N, int64_t hd, size_t lds) {
    DCLIP_REQUIRE(qkv && B > 0 && H > 0 && N > 0 && N <= MAPS_NMAX, "%s: bad argument (N <= %d)", who, MAPS_NMAX);
    DCLIP_REQUIRE(hd == 32 || hd == 64, "%s: head dim must be 32 or 64 (got %ld)", who, (long)hd);
    DCLIP_REQUIRE(ld >= 3 * H * hd && ld % 8 == 0 && ((uintptr_t)qkv % 16) == 0, "%s: qkv rows must hold 3 * H * hd elements, 16-byte aligned", who);
    DCLIP_REQUIRE(B * N <= INT32_MAX / 2, "%s: batch too large", who);
    DCLIP_REQUIRE(lds <= MAPS_LDS_MAX, "%s: H = %ld, N = %ld, hd = %ld needs %zu bytes of LDS (max %zu)", who, (long)H, (long)N, (long)hd,
                  lds, MAPS_LDS_MAX);
    return DCLIP_OK;
}

}  // namespace

extern "C" int dclip_attn_maps_fwd(const void* qkv, int64_t ld, const float* Wl, float* score_map, float* prob_map, int64_t B, int64_t H,
                                   int64_t N, int64_t hd, float scale, int causal, void* stream) {
    const size_t lds = maps_lds_floats((int)H, (int)N, (int)hd, Wl && prob_map, false) * 4;
    const int rc = check_common("dclip_attn_maps_fwd", qkv, ld, B, H, N, hd, lds);
    if (rc != DCLIP_OK) return rc;
    if (!score_map && !prob_map) return DCLIP_OK;
    MapsArgs a{(const bf16_t*)qkv, ld, prob_map ? Wl : nullptr, score_map, prob_map, nullptr, nullptr, nullptr, 0, nullptr,
               (int)B, (int)H, (int)N, 0, (int)hd, causal ? 1 : 0, scale};
    TraceScope tr(DCLIP_TRACE_ATTN, 2.0 * B * H * N * N * hd, 2.0 * B * N * 3 * H * hd + 4.0 * B * N * N * ((score_map ? 1 : 0) + (prob_map ? 1 : 0)),
                  stream, (int)(B * H), (int)N, (int)H, 7);
    hipLaunchKernelGGL(attn_maps_fwd_kernel, dim3((unsigned)((N + TQ - 1) / TQ), (unsigned)B), dim3(256), lds, (hipStream_t)stream, a);
    return dclip_check_launch("dclip_attn_maps_fwd");
}

extern "C" size_t dclip_attn_maps_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N) {
    if (B <= 0 || H <= 0 || N <= 0) return 0;
    return (((size_t)B * ((N + TQ - 1) / TQ) * H * H * 4) + 255) & ~(size_t)255;
}

extern "C" int dclip_attn_maps_bwd(const void* qkv, int64_t ld, const float* Wl, const float* d_score_map, const float* d_prob_map, void* dS,
                                   int ds_blocked, float* dWl, void* workspace, size_t ws_bytes, int64_t B, int64_t H, int64_t N, int64_t Np,
                                   int64_t hd, float scale, int causal, void* stream) {
    const bool mixed = Wl && d_prob_map;
    const size_t lds = maps_lds_floats((int)H, (int)N, (int)hd, mixed, mixed) * 4;
    const int rc = check_common("dclip_attn_maps_bwd", qkv, ld, B, H, N, hd, lds);
    if (rc != DCLIP_OK) return rc;
    DCLIP_REQUIRE(dS && Np >= N && Np % 8 == 0, "dclip_attn_maps_bwd: dS [B, H, N, Np] with Np = round_up(N, 8) required");
    const bool want_dwl = mixed && dWl;
    DCLIP_REQUIRE(!want_dwl || (workspace && ws_bytes >= dclip_attn_maps_bwd_workspace_bytes(B, H, N) && ((uintptr_t)workspace % 16) == 0),
                  "dclip_attn_maps_bwd: dW_l needs dclip_attn_maps_bwd_workspace_bytes(B, H, N) = %zu bytes of workspace (got %zu)",
                  dclip_attn_maps_bwd_workspace_bytes(B, H, N), workspace ? ws_bytes : (size_t)0);
    if (!d_score_map && !d_prob_map) return DCLIP_OK;
    MapsArgs a{(const bf16_t*)qkv, ld, mixed ? Wl : nullptr, nullptr, nullptr, d_score_map, d_prob_map, (bf16_t*)dS, ds_blocked ? 1 : 0,
               want_dwl ? (float*)workspace : nullptr, (int)B, (int)H, (int)N, (int)Np, (int)hd, causal ? 1 : 0, scale};
    TraceScope tr(DCLIP_TRACE_ATTN, d_prob_map ? 2.0 * B * H * N * N * hd : 0.0,
                  (d_prob_map ? 2.0 * B * N * 2 * H * hd : 0.0) + 4.0 * B * N * N * ((d_score_map ? 1 : 0) + (d_prob_map ? 1 : 0)) + 4.0 * B * H * N * N,
                  stream, (int)(B * H), (int)N, (int)H, 8);
    const dim3 grid((unsigned)((N + TQ - 1) / TQ), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_maps_bwd_kernel, grid, dim3(256), lds, st, a);
    if (want_dwl) {
        const int rc2 = dclip_check_launch("dclip_attn_maps_bwd");
        if (rc2 != DCLIP_OK) return rc2;
        hipLaunchKernelGGL(attn_maps_dwl_reduce_kernel, dim3((unsigned)(H * H)), dim3(256), 0, st, (const float*)workspace, dWl,
                           (int)(grid.x * grid.y), (int)(H * H));
    }
    return dclip_check_launch("dclip_attn_maps_bwd");
}
