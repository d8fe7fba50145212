// Top-K search over embeddings and the group mean of normalised rows (gfx950): which gallery rows are a query's best (zero-shot
// classification over class prompts, "the K best images for a caption", k-NN), the question recall.hip cannot answer.
//
//   L[i, j]   = cos(q_i, g_j), 0 when either row's squared norm is 0 or not a positive finite number
//   idx[i, :] = the first k gallery indices in the total order (L descending, index ascending); score[i, p] = L[i, idx[i, p]]
//
// Two or three kernels on one stream, no atomics, plain vector stores; the [nq, ng] logits are never written:
//   topk_norm_kernel     one wave per row: x / |x| into the workspace (recall_norm_kernel's routine); an invalid row becomes the zero row
//   topk_search_kernel   16 queries per workgroup, the four waves split the gallery's 16-column tiles (recall_i2t_kernel's stripe pass).
//                        A wave keeps, per query row, the sorted list of its best keys, entry t in lane t; the four lists of a row are
//                        merged through LDS by rank.  Few query panels and a long gallery: the gallery is cut into up to 8 slices
//                        (blockIdx.y), each workgroup leaves its k best keys in the workspace, and
//   topk_merge_kernel    one wave per query merges the slices' lists by the same rank rule
// Every logit comes from dot_tile() of sim_tiles.h, so bit-equal rows give bit-equal logits here as in recall.hip, loss.hip and
// metrics.hip.  A candidate is one 64-bit key, the orderable bits of its logit above ~index: "better" is one unsigned compare, the
// order is total, and the answer is a function of the logits alone, however the waves split the gallery.
//
//   group_mean_kernel    one wave per group: out[c] = (1 / n_c) sum over the group's rows of x / |x|, rows added in index order
#include <hip/hip_runtime.h>

#include "sim_tiles.h"

namespace {

typedef unsigned long long u64;

constexpr int MAXK = 64;                                  // one list entry per lane
// the key of "no entry": the logit -inf with index -1.  Every real key is above it (a cosine is finite), and it decodes to what the
// trailing k - ng outputs hold
constexpr u64 EMPTY_KEY = (u64)0x007FFFFFu << 32;

struct TopkArgs {
    const float* q; const float* g;                       // raw rows [nq, E], [ng, E]
    float* qn; float* gn;                                 // normalised copies (workspace)
    int nq, ng, E, k;
    int slices;                                           // gallery slices; 1: the search kernel writes idx / score itself
    u64* part;                                            // [nq, slices, k] keys (workspace), slices > 1
    int32_t* idx; float* score;                           // [nq, k]; score may be null
};

// (logit, column) -> key.  -0 and +0 compare equal, so both become +0 first (a NaN, which no finite normalised row produces, too).
// f32 bits order as unsigned once the sign bit of a non-negative value is set and a negative value is complemented; ~col puts the
// lower index ahead among equal logits.
__device__ __forceinline__ u64 make_key(float s, int col) {
    s = (s < 0.f || s > 0.f) ? s : 0.f;
    unsigned b = __float_as_uint(s);
    b ^= (b >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((u64)b << 32) | (unsigned)~col;
}
__device__ __forceinline__ float key_score(u64 key) {
    unsigned b = (unsigned)(key >> 32);
    b ^= (b >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(b);
}
__device__ __forceinline__ int key_index(u64 key) { return (int)~(unsigned)key; }

// the value lane `src` (wave-uniform) holds
__device__ __forceinline__ u64 read_lane(u64 v, int src) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, src), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// one wave per row of q then g: normalize_row<true>, then an invalid row is made the zero row.  A row whose squared norm is a
// positive finite number has finite elements and a finite scale, so its copy holds no NaN; of the others, a zero or overflowing
// finite row is already 0 x = (+-)0 everywhere, and one that holds an inf or a NaN has 0 x = NaN in its copy: "holds a NaN" is
// exactly "was invalid and is not yet zero".  Each lane reads back what it wrote itself.
__global__ __launch_bounds__(256) void topk_norm_kernel(TopkArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)a.nq + a.ng) return;                        // wave-uniform
    const float* src = row < a.nq ? a.q + row * a.E : a.g + (row - a.nq) * a.E;
    float* dst = row < a.nq ? a.qn + row * a.E : a.gn + (row - a.nq) * a.E;
    normalize_row<true>(src, dst, a.E, lane);
    bool bad = false;
    for (int c = lane * 4; c < a.E; c += 256) {
        const float4 v = *(const float4*)(dst + c);
        bad |= v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;
    }
    if (__ballot(bad) == 0) return;                                 // wave-uniform
    for (int c = lane * 4; c < a.E; c += 256) *(float4*)(dst + c) = float4{0.f, 0.f, 0.f, 0.f};
}

// list: this wave's sorted keys of one query row, descending, entry t in lane t (all 64 lanes, whatever k is; the k-th is lane k - 1).
// Puts `key` (wave-uniform) where it belongs: the entries above it stay, the others move up one lane, the last falls off.
__device__ __forceinline__ void list_insert(u64& list, u64 key, int lane) {
    const int pos = __popcll(__ballot(list > key));
    const u64 below = __shfl_up(list, 1);
    list = lane < pos ? list : (lane == pos ? key : below);
}

// the number of entries of the descending list[0, k) that come before `key` in the merge: those above it, and with `ties` those equal
__device__ __forceinline__ int count_before(const u64* list, int k, u64 key, bool ties) {
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u64 v = list[mid];
        if (v > key || (ties && v == key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Merge by rank of n descending lists of k keys, list w at lists + w stride, by the lanes t < k of one wave: lane t takes the t-th
// entry of every list.  An entry's place in the merged order is its place in its own list plus the entries of the other lists that
// come before it; equal keys (only EMPTY_KEY occurs twice: the lists hold different columns) go by list number, so every place below
// n k is taken exactly once and put(place, key) is called exactly once for every place below k.
template <class Put>
__device__ __forceinline__ void merge_lists(const u64* lists, int stride, int n, int k, int lane, Put put) {
    if (lane >= k) return;
    for (int w = 0; w < n; ++w) {
        const u64 key = lists[w * stride + lane];
        int place = lane;
        for (int w2 = 0; w2 < n; ++w2)
            if (w2 != w) place += count_before(lists + w2 * stride, k, key, w2 < w);
        if (place < k) put(place, key);
    }
}

__device__ __forceinline__ void put_result(const TopkArgs& a, int64_t row, int place, u64 key) {
    const int64_t o = row * a.k + place;
    a.idx[o] = key_index(key);
    if (a.score) a.score[o] = key_score(key);
}

// grid = (ceil(nq / 16), slices) ; slice s owns the gallery tiles [s ntile / slices, (s + 1) ntile / slices), its four waves split them
__global__ __launch_bounds__(256) void topk_search_kernel(TopkArgs a) {
    __shared__ u64 s_list[4][16][MAXK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int nq = a.nq, ng = a.ng, E = a.E, k = a.k;
    const int i0 = blockIdx.x * 16;
    u64 list[16];                                                   // row r's list; only ever indexed by unrolled constants
#pragma unroll
    for (int r = 0; r < 16; ++r) list[r] = EMPTY_KEY;
    u64 kth[4];                                                     // the k-th key of row 4 g + q: what a candidate has to beat
#pragma unroll
    for (int q = 0; q < 4; ++q) kth[q] = EMPTY_KEY;
    const float* pa = a.qn + (int64_t)min(i0 + (lane & 15), nq - 1) * E;
    const int ntile = (ng + 15) / 16;
    const int t0 = (int)((int64_t)blockIdx.y * ntile / a.slices), t1 = (int)((int64_t)(blockIdx.y + 1) * ntile / a.slices);
    for (int jt = t0 + wave; jt < t1; jt += 4) {
        const int col = jt * 16 + (lane & 15);
        const f32x4 S = dot_tile(pa, a.gn + (int64_t)min(col, ng - 1) * E, E, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u64 cand = col < ng ? make_key(S[q], col) : 0;    // a column past the gallery: below EMPTY_KEY, never ahead
            const u64 ahead = __ballot(cand > kth[q]);
            if (ahead == 0) continue;                               // wave-uniform; the common case after the first few tiles
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {                        // the candidates of row 4 gg + q sit in lanes [16 gg, 16 gg + 16)
                unsigned m = (unsigned)(ahead >> (16 * gg)) & 0xFFFFu;
                if (m == 0) continue;
                u64 bar = read_lane(list[4 * gg + q], k - 1);
                while (m) {
                    const int src = 16 * gg + __builtin_ctz(m);
                    m &= m - 1;
                    const u64 key = read_lane(cand, src);
                    if (key > bar) {                                // (an earlier insertion of this tile may have raised the bar)
                        list_insert(list[4 * gg + q], key, lane);
                        bar = read_lane(list[4 * gg + q], k - 1);
                    }
                }
                if (g == gg) kth[q] = bar;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_list[wave][r][lane] = list[r];
    __syncthreads();
    // wave w merges the four lists of rows [4 w, 4 w + 4): into idx / score, or with a sliced gallery into this slice's list of the row
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const int64_t row = i0 + r;
        if (row >= nq) continue;                                    // wave-uniform
        if (a.slices == 1) {
            merge_lists(&s_list[0][r][0], 16 * MAXK, 4, k, lane, [&](int place, u64 key) { put_result(a, row, place, key); });
        } else {
            u64* dst = a.part + (row * a.slices + blockIdx.y) * k;
            merge_lists(&s_list[0][r][0], 16 * MAXK, 4, k, lane, [&](int place, u64 key) { dst[place] = key; });
        }
    }
}

// one wave per query: the slices' lists [slices, k] of the row, each descending, into idx / score
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.nq) return;                                        // wave-uniform
    merge_lists(a.part + row * a.slices * a.k, a.k, a.slices, a.k, lane, [&](int place, u64 key) { put_result(a, row, place, key); });
}

constexpr int GM_CHUNKS = 16;                             // float4 accumulators per lane: E <= 4096

struct GroupMeanArgs {
    const float* rows; const int32_t* off; float* out;
    int n_groups, n_rows, E;
};

// one wave per group.  The scale of a row is normalize_row<true>'s, sum for sum: 1 / sqrt of the squared norm, 0 when that is 0 or
// not a positive finite number (such a row adds nothing).
__global__ __launch_bounds__(256) void group_mean_kernel(GroupMeanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.n_groups) return;                                    // wave-uniform
    const int E = a.E;
    const int start = min(max(a.off[c], 0), a.n_rows), end = min(max(a.off[c + 1], 0), a.n_rows);
    float4 acc[GM_CHUNKS];
#pragma unroll
    for (int j = 0; j < GM_CHUNKS; ++j) acc[j] = float4{0.f, 0.f, 0.f, 0.f};
    for (int r = start; r < end; ++r) {
        const float* src = a.rows + (int64_t)r * E;
        float s = 0.f;
        for (int col = lane * 4; col < E; col += 256) {
            const float4 v = *(const float4*)(src + col);
            s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
        s = wave_sum(s);
        if (!(s > 0.f && s < __builtin_inff())) continue;           // wave-uniform
        const float inv = 1.f / sqrtf(s);
#pragma unroll
        for (int j = 0; j < GM_CHUNKS; ++j) {
            const int col = lane * 4 + 256 * j;
            if (col < E) {
                const float4 v = *(const float4*)(src + col);
                acc[j].x += v.x * inv; acc[j].y += v.y * inv; acc[j].z += v.z * inv; acc[j].w += v.w * inv;
            }
        }
    }
    const float w = end > start ? 1.f / (float)(end - start) : 0.f;
    float* dst = a.out + c * E;
#pragma unroll
    for (int j = 0; j < GM_CHUNKS; ++j) {
        const int col = lane * 4 + 256 * j;
        if (col < E) *(float4*)(dst + col) = float4{acc[j].x * w, acc[j].y * w, acc[j].z * w, acc[j].w * w};
    }
}

inline bool size_ok(int64_t nq, int64_t ng, int64_t E, int k) {
    return nq >= 1 && ng >= 1 && nq < (1LL << 24) && ng < (1LL << 24) && E >= 16 && E % 16 == 0 && E < (1LL << 24) && k >= 1 && k <= MAXK;
}

// Gallery slices: a panel of 16 queries is one workgroup, and a wave's tile is one dependent MFMA chain, so few panels leave the card
// idle.  Enough slices for about 1 536 workgroups (six waves per SIMD on 256 CUs, where the per-element time levels off), at most 8,
// each at least 8 tiles long.  A function of the sizes alone: the workspace query and the call agree, and so do two calls.
inline int slices_for(int64_t nq, int64_t ng) {
    const int64_t panels = (nq + 15) / 16, ntile = (ng + 15) / 16;
    int64_t s = (1536 + panels - 1) / panels;
    s = s < 8 ? s : 8;
    s = s < ntile / 8 ? s : ntile / 8;
    return (int)(s < 1 ? 1 : s);
}

}  // namespace

extern "C" size_t dclip_topk_search_workspace(int64_t nq, int64_t ng, int64_t E, int k) {
    if (!size_ok(nq, ng, E, k)) return 0;
    const int slices = slices_for(nq, ng);
    return dclip_up256((size_t)nq * E * 4) + dclip_up256((size_t)ng * E * 4) + (slices > 1 ? dclip_up256((size_t)nq * slices * k * 8) : 0);
}

extern "C" int dclip_topk_search(const float* queries, const float* gallery, int64_t nq, int64_t ng, int64_t E, int k, int32_t* idx,
                                 float* score, void* ws, size_t ws_bytes, void* stream) {
    DCLIP_REQUIRE(queries && gallery && idx && ws, "dclip_topk_search: null operand (queries, gallery, idx and workspace are required)");
    DCLIP_REQUIRE(k >= 1 && k <= MAXK, "dclip_topk_search: need 1 <= k <= %d (k=%d)", MAXK, k);
    DCLIP_REQUIRE(nq >= 1 && nq < (1LL << 24) && ng >= 1 && ng < (1LL << 24), "dclip_topk_search: need 1 <= nq, ng < 2^24 (nq=%ld ng=%ld)",
                  (long)nq, (long)ng);
    DCLIP_REQUIRE(E >= 16 && E % 16 == 0 && E < (1LL << 24), "dclip_topk_search: E=%ld must be a positive multiple of 16 (below 2^24)", (long)E);
    DCLIP_REQUIRE(ws_bytes >= dclip_topk_search_workspace(nq, ng, E, k), "dclip_topk_search: workspace too small (%zu < %zu)", ws_bytes,
                  dclip_topk_search_workspace(nq, ng, E, k));
    DCLIP_REQUIRE(dclip_aligned16(queries) && dclip_aligned16(gallery) && dclip_aligned16(ws) && ((uintptr_t)idx % 4) == 0 &&
                  ((uintptr_t)score % 4) == 0,
                  "dclip_topk_search: queries, gallery and workspace must be 16-byte aligned (idx and score 4-byte)");
    TopkArgs a;
    a.q = queries; a.g = gallery;
    a.nq = (int)nq; a.ng = (int)ng; a.E = (int)E; a.k = k;
    Bump w(ws);
    a.qn = w.take<float>(nq * E); a.gn = w.take<float>(ng * E);
    a.slices = slices_for(nq, ng);
    a.part = a.slices > 1 ? w.take<u64>((size_t)nq * a.slices * k) : nullptr;
    a.idx = idx; a.score = score;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(topk_norm_kernel, dim3((unsigned)((nq + ng + 3) / 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(topk_search_kernel, dim3((unsigned)((nq + 15) / 16), (unsigned)a.slices), dim3(256), 0, st, a);
    if (a.slices > 1) hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, a);
    return dclip_check_launch("dclip_topk_search");
}

extern "C" int dclip_group_mean_rows(const float* rows, const int32_t* offsets, int64_t n_groups, int64_t n_rows, int64_t E, float* out,
                                     void* stream) {
    DCLIP_REQUIRE(rows && offsets && out, "dclip_group_mean_rows: null operand (rows, offsets and out are required)");
    DCLIP_REQUIRE(n_groups >= 1 && n_groups < (1LL << 24) && n_rows >= 1 && n_rows < (1LL << 24),
                  "dclip_group_mean_rows: need 1 <= n_groups, n_rows < 2^24 (n_groups=%ld n_rows=%ld)", (long)n_groups, (long)n_rows);
    DCLIP_REQUIRE(E >= 16 && E % 16 == 0 && E <= 256 * GM_CHUNKS, "dclip_group_mean_rows: E=%ld must be a positive multiple of 16, at most %d",
                  (long)E, 256 * GM_CHUNKS);
    DCLIP_REQUIRE(dclip_aligned16(rows) && dclip_aligned16(out) && ((uintptr_t)offsets % 4) == 0,
                  "dclip_group_mean_rows: rows and out must be 16-byte aligned (offsets 4-byte)");
    GroupMeanArgs a;
    a.rows = rows; a.off = offsets; a.out = out;
    a.n_groups = (int)n_groups; a.n_rows = (int)n_rows; a.E = (int)E;
    hipLaunchKernelGGL(group_mean_kernel, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return dclip_check_launch("dclip_group_mean_rows");
}
