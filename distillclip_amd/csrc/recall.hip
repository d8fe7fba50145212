// Recall@K retrieval with several captions per image, both directions (gfx950): the MS-COCO protocol every CLIP-distillation result is
// compared by (5 000 images x 25 010 captions on the 5k test split).  The reference validates with one caption per image
// (model/dual_distill_model.py:220-224, torchmetrics accuracy against labels arange(n)); its data set (data/component/ms_coco.py)
// carries the several captions this protocol ranks.
//
//   L[i, c]     = cos(img_i, txt_c), 0 when either norm is 0 (dclip_clipscore's convention)
//   rank_i2t[i] = #{ c not owned by i : L[i, c] > max over i's own captions of L[i, c'] }        (-1 without captions)
//   rank_t2i[c] = #{ j != owner(c)    : L[j, c] > L[owner(c), c] }                                (-1 when no group covers c)
//
// Four kernels on one stream, no atomics, plain vector stores; the [n_img, n_txt] logits are never written:
//   recall_norm_kernel    one wave per row: x / |x| (a zero row stays zero) into the workspace
//   recall_owner_kernel   one thread per caption: its owner by bisection of the clamped offset table
//   recall_i2t_kernel     16 images per workgroup: the best own caption first, then every caption tile
//   recall_t2i_kernel     16 captions per workgroup: the target tile (rows = the captions, columns = their owners, diagonal read) first,
//                         then every image tile; the logits are computed a second time
//   recall_finalize_kernel  one workgroup: integer hits and rank sums, each output one double division cast once
// Every logit comes from dot_tile() of sim_tiles.h, the tile routine of the loss and of metrics.hip: v_mfma_f32_16x16x4_f32 is bit for bit
// an fmaf chain in k order, the order there depends on the row pair only, so bit-equal rows give bit-equal logits wherever they sit, and a
// tie never counts against the target.
#include <hip/hip_runtime.h>

#include "sim_tiles.h"

namespace {

constexpr int MAXK = 8;

struct RecallArgs {
    const float* img; const float* txt;       // raw embeddings [n_img, E], [n_txt, E]
    const int32_t* off;                       // device [n_img + 1]
    float* nimg; float* ntxt;                 // normalised copies (workspace)
    int* owner;                               // [n_txt] (workspace)
    int* rank_i; int* rank_t;                 // [n_img], [n_txt] (workspace)
    int n_img, n_txt, E, nk;
    int ks[MAXK];
    float* out;                               // [2 nk + 2]
    int* rank_i2t; int* rank_t2i;             // optional copies of the ranks
};

// whatever the table holds, an offset names a caption boundary in [0, n_txt]
__device__ __forceinline__ int clamped_off(const RecallArgs& a, int i) { return min(max(a.off[i], 0), a.n_txt); }

// one wave per row of img then txt: x / |x|; a row whose squared norm is 0 (or not a positive finite number) becomes the zero row,
// so every cosine with it is 0
__global__ __launch_bounds__(256) void recall_norm_kernel(RecallArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)a.n_img + a.n_txt) return;                  // wave-uniform
    const float* src = row < a.n_img ? a.img + row * a.E : a.txt + (row - a.n_img) * a.E;
    float* dst = row < a.n_img ? a.nimg + row * a.E : a.ntxt + (row - a.n_img) * a.E;
    normalize_row<true>(src, dst, a.E, lane);
}

// owner[c] = the last image i with off[i] <= c, when c < off[i + 1]; -1 otherwise.  On a well-formed table that is the one group that
// holds c (empty groups are skipped: they share their start with a later one); on any other table the bisection still ends inside
// [0, n_img) and the answer depends on the table alone.
__global__ __launch_bounds__(256) void recall_owner_kernel(RecallArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n_txt) return;
    int lo = 0, hi = a.n_img - 1;                                   // invariant: the answer, if any, is in [lo, hi]
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (clamped_off(a, mid) <= c) lo = mid; else hi = mid - 1;
    }
    a.owner[c] = (clamped_off(a, lo) <= c && c < clamped_off(a, lo + 1)) ? lo : -1;
}

// grid = ceil(n_img / 16) ; the four waves split the caption tiles
__global__ __launch_bounds__(256) void recall_i2t_kernel(RecallArgs a) {
    __shared__ int s_start[16], s_end[16];
    __shared__ float red_b[4][16];
    __shared__ int red_c[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int n_img = a.n_img, n_txt = a.n_txt, E = a.E;
    const int i0 = blockIdx.x * 16;
    if (threadIdx.x < 16) {
        const int i = i0 + threadIdx.x;
        int s = 0, e = 0;                                          // rows past n_img: an empty group
        if (i < n_img) { s = clamped_off(a, i); e = clamped_off(a, i + 1); }
        s_start[threadIdx.x] = s;
        s_end[threadIdx.x] = e;
    }
    __syncthreads();
    int st[4], en[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { st[q] = s_start[4 * g + q]; en[q] = s_end[4 * g + q]; }
    int cmin = n_txt, cmax = 0;                                    // the captions some image of this panel owns lie in [cmin, cmax)
    for (int r = 0; r < 16; ++r)
        if (s_start[r] < s_end[r]) { cmin = min(cmin, s_start[r]); cmax = max(cmax, s_end[r]); }
    const float* pa = a.nimg + (int64_t)min(i0 + (lane & 15), n_img - 1) * E;
    // the best own caption first: every later logit is compared with values the very same routine produced
    float best[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) best[q] = -__builtin_inff();
    for (int jt = cmin / 16 + wave; jt * 16 < cmax; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const f32x4 S = dot_tile(pa, a.ntxt + (int64_t)min(col, n_txt - 1) * E, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (col >= st[q] && col < en[q]) best[q] = fmaxf(best[q], S[q]);      // (en <= n_txt: a clamped column is never inside)
    }
    stripe_put(red_b, best, lane, wave, StripeMax());
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) best[q] = stripe_get(red_b, 4 * g + q, StripeMax());
    int cnt[4] = {0, 0, 0, 0};
    const int ntile = (n_txt + 15) / 16;
    for (int jt = wave; jt < ntile; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const f32x4 S = dot_tile(pa, a.ntxt + (int64_t)min(col, n_txt - 1) * E, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool own = col >= st[q] && col < en[q];
            cnt[q] += (col < n_txt && !own && S[q] > best[q]) ? 1 : 0;
        }
    }
    stripe_put(red_c, cnt, lane, wave, StripeSum());
    __syncthreads();
    if (threadIdx.x < 16 && i0 + threadIdx.x < n_img) {
        const int r = threadIdx.x;
        a.rank_i[i0 + r] = s_start[r] < s_end[r] ? stripe_get(red_c, r, StripeSum()) : -1;
    }
}

// grid = ceil(n_txt / 16) ; rows of a tile = captions, columns = images ; the four waves split the image tiles
__global__ __launch_bounds__(256) void recall_t2i_kernel(RecallArgs a) {
    __shared__ int s_owner[16];
    __shared__ int red_c[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int n_img = a.n_img, n_txt = a.n_txt, E = a.E;
    const int c0 = blockIdx.x * 16;
    if (threadIdx.x < 16) s_owner[threadIdx.x] = c0 + threadIdx.x < n_txt ? a.owner[c0 + threadIdx.x] : -1;
    __syncthreads();
    int own[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) own[q] = s_owner[4 * g + q];
    const float* pa = a.ntxt + (int64_t)min(c0 + (lane & 15), n_txt - 1) * E;
    // the target tile: column r is the owner of caption r, the diagonal holds L[owner(c), c] (an unowned caption borrows image 0; its
    // rank is not kept)
    // (this kernel keeps its own spelling of tile_diag() and of the stripe reduction: written with the shared helpers it compiled to
    // two more VGPRs and measured 1.5 % slower at 5 000 x 25 010 x 512, the k-loop being instruction for instruction the same)
    float d[4];
    {
        const f32x4 S = dot_tile(pa, a.nimg + (int64_t)max(s_owner[lane & 15], 0) * E, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = __shfl(S[q], g * 16 + g * 4 + q);
    }
    int cnt[4] = {0, 0, 0, 0};
    const int ntile = (n_img + 15) / 16;
    for (int jt = wave; jt < ntile; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const f32x4 S = dot_tile(pa, a.nimg + (int64_t)min(col, n_img - 1) * E, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt[q] += (col < n_img && col != own[q] && S[q] > d[q]) ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int c = cnt[q];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o);
        if ((lane & 15) == 0) red_c[wave][4 * g + q] = c;
    }
    __syncthreads();
    if (threadIdx.x < 16 && c0 + threadIdx.x < n_txt) {
        const int r = threadIdx.x;
        const int c = (red_c[0][r] + red_c[1][r]) + (red_c[2][r] + red_c[3][r]);
        a.rank_t[c0 + r] = s_owner[r] >= 0 ? c : -1;
    }
}

// one workgroup: integer hits, rank sums and denominators of both directions; slot layout of the reduction:
//   [0, 8) i2t hits, [8, 16) t2i hits, 16 / 17 rank sums, 18 / 19 denominators
constexpr int NSLOT = 2 * MAXK + 4;

__global__ __launch_bounds__(256) void recall_finalize_kernel(RecallArgs a) {
    __shared__ long long red[256];
    __shared__ long long tot[NSLOT];
    long long v[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) v[s] = 0;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir ? a.n_txt : a.n_img;
        const int* rank = dir ? a.rank_t : a.rank_i;
        int* copy = dir ? a.rank_t2i : a.rank_i2t;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int r = rank[i];
            if (copy) copy[i] = r;
            if (r < 0) continue;
#pragma unroll
            for (int k = 0; k < MAXK; ++k) v[dir * MAXK + k] += (k < a.nk && r < a.ks[k]) ? 1 : 0;
            v[2 * MAXK + dir] += r;
            v[2 * MAXK + 2 + dir] += 1;
        }
    }
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        red[threadIdx.x] = v[s];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) tot[s] = red[0];
        __syncthreads();
    }
    // out[0, nk) i2t recall, [nk, 2 nk) t2i recall, then the two mean ranks; an empty set (only a malformed table has one) gives 0
    const int t = threadIdx.x;
    if (t < 2 * a.nk + 2) {
        const int dir = t < 2 * a.nk ? t / a.nk : t - 2 * a.nk;
        const long long num = t < 2 * a.nk ? tot[dir * MAXK + t % a.nk] : tot[2 * MAXK + dir];
        const long long den = tot[2 * MAXK + 2 + dir];
        a.out[t] = den > 0 ? (float)((double)num / (double)den) : 0.f;
    }
}

inline bool size_ok(int64_t n_img, int64_t n_txt, int64_t E) {
    return n_img >= 1 && n_txt >= 1 && n_img < (1LL << 24) && n_txt < (1LL << 24) && E > 0 && E % 16 == 0 && E < (1LL << 24);
}

}  // namespace

extern "C" size_t dclip_retrieval_recall_workspace(int64_t n_img, int64_t n_txt, int64_t E) {
    if (!size_ok(n_img, n_txt, E)) return 0;
    return dclip_up256((size_t)n_img * E * 4) + dclip_up256((size_t)n_txt * E * 4) + dclip_up256((size_t)n_img * 4) +
           2 * dclip_up256((size_t)n_txt * 4);
}

extern "C" int dclip_retrieval_recall(const float* img, const float* txt, const int32_t* txt_offsets, int64_t n_img, int64_t n_txt, int64_t E,
                                      const int32_t* ks, int nk, float* out, int32_t* rank_i2t, int32_t* rank_t2i, void* ws, size_t ws_bytes,
                                      void* stream) {
    DCLIP_REQUIRE(img && txt && txt_offsets && out && ws, "dclip_retrieval_recall: null operand (img, txt, txt_offsets, out and workspace are required)");
    DCLIP_REQUIRE(n_img >= 1 && n_img < (1LL << 24) && n_txt >= 1 && n_txt < (1LL << 24),
                  "dclip_retrieval_recall: need 1 <= n_img, n_txt < 2^24 (n_img=%ld n_txt=%ld)", (long)n_img, (long)n_txt);
    DCLIP_REQUIRE(E > 0 && E % 16 == 0 && E < (1LL << 24), "dclip_retrieval_recall: E=%ld must be a positive multiple of 16 (below 2^24)", (long)E);
    DCLIP_REQUIRE(nk >= 0 && nk <= MAXK && (nk == 0 || ks), "dclip_retrieval_recall: 0 <= nk <= %d cut-offs in a host array (nk=%d)", MAXK, nk);
    DCLIP_REQUIRE(ws_bytes >= dclip_retrieval_recall_workspace(n_img, n_txt, E), "dclip_retrieval_recall: workspace too small (%zu < %zu)",
                  ws_bytes, dclip_retrieval_recall_workspace(n_img, n_txt, E));
    DCLIP_REQUIRE(dclip_aligned16(img) && dclip_aligned16(txt) && dclip_aligned16(ws) && ((uintptr_t)txt_offsets % 4) == 0 &&
                  ((uintptr_t)out % 4) == 0 && ((uintptr_t)rank_i2t % 4) == 0 && ((uintptr_t)rank_t2i % 4) == 0,
                  "dclip_retrieval_recall: img, txt and workspace must be 16-byte aligned (offsets, out and ranks 4-byte)");
    RecallArgs a;
    a.img = img; a.txt = txt; a.off = txt_offsets;
    a.n_img = (int)n_img; a.n_txt = (int)n_txt; a.E = (int)E; a.nk = nk;
    for (int k = 0; k < MAXK; ++k) a.ks[k] = k < nk ? ks[k] : 0;
    Bump w(ws);
    a.nimg = w.take<float>(n_img * E); a.ntxt = w.take<float>(n_txt * E);
    a.rank_i = w.take<int>(n_img); a.rank_t = w.take<int>(n_txt); a.owner = w.take<int>(n_txt);
    a.out = out; a.rank_i2t = rank_i2t; a.rank_t2i = rank_t2i;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(recall_norm_kernel, dim3((unsigned)((n_img + n_txt + 3) / 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(recall_owner_kernel, dim3((unsigned)((n_txt + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(recall_i2t_kernel, dim3((unsigned)((n_img + 15) / 16)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(recall_t2i_kernel, dim3((unsigned)((n_txt + 15) / 16)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(recall_finalize_kernel, dim3(1), dim3(256), 0, st, a);
    return dclip_check_launch("dclip_retrieval_recall");
}
