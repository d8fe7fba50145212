// L-CLIPScore scoring (gfx950): CLIP-S and RefCLIP-S of Hessel et al. 2021 ("CLIPScore: A Reference-free Evaluation Metric for Image
// Captioning") from the towers' raw last_representation rows.  The reference trains the students of this metric and has no scorer of its
// own: the three formulas below are the paper's.
//
//   cos(a, b)  = a.b / (|a| |b|), 0 when either norm is 0 (never NaN for finite rows)
//   clip_s     = w max(cos(v_b, c), 0)                        v_b: image b, c: its k-th candidate (row b K + k of cand)
//   ref_s      = max(0, max_{r in R_b} cos(c, r))             R_b: rows [off[b], off[b + 1]) of refs; 0 for an empty set
//   refclip_s  = 2 clip_s ref_s / (clip_s + ref_s)            0 when the denominator is 0
//
// One wave per candidate row, four waves per workgroup, nothing shared between waves.  The candidate row stays in registers (at most
// four float4 per lane: E <= 1024); the image row and then every reference row of the wave's image are read once, 16 bytes per lane,
// the next reference row in flight while the current one is reduced.  The K waves of one image read the same reference rows: they sit in
// neighbouring workgroups, so all but the first read come from L2.  The dense [B K, R] similarity matrix of a matmul formulation, of
// which only the block diagonal is wanted, is never formed.  Plain stores, no atomics, no workspace: the same call gives the same bits.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int SCORE_VEC = 4;                    // float4 per lane: 64 lanes x 4 x 4 floats = 1024 = the largest E

struct ScoreArgs {
    const float* img; const float* cand; const float* refs;
    const int32_t* off;                         // [B + 1] CSR into refs (null without references)
    int64_t ld_img, ld_cand, ld_ref;
    int64_t rows;                               // B K
    int K, R, E;
    float w;
    float* clip_s; float* ref_s; float* refclip_s;
};

struct Row { float4 v[SCORE_VEC]; };

// the lane's columns 4 lane + 256 i .. + 3 of a row; columns past E read as 0 (E % 4 == 0: a float4 is inside or outside as a whole)
__device__ __forceinline__ Row load_row(const float* __restrict__ p, int E, int lane) {
    Row r;
#pragma unroll
    for (int i = 0; i < SCORE_VEC; ++i) {
        const int c = lane * 4 + i * 256;
        r.v[i] = c < E ? *(const float4*)(p + c) : float4{0.f, 0.f, 0.f, 0.f};
    }
    return r;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// a.b and b.b over the whole row, in every lane
__device__ __forceinline__ void dot_and_norm(const Row& a, const Row& b, float& ab, float& bb) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < SCORE_VEC; ++i) { s += dot4(a.v[i], b.v[i]); q += dot4(b.v[i], b.v[i]); }
    ab = wave_sum(s);
    bb = wave_sum(q);
}

__device__ __forceinline__ float cosine(float ab, float aa, float bb) {
    return (aa > 0.f && bb > 0.f) ? ab * (1.f / sqrtf(aa)) * (1.f / sqrtf(bb)) : 0.f;
}

__global__ __launch_bounds__(256) void clipscore_kernel(ScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;                                      // wave-uniform
    const int64_t b = row / a.K;
    const int E = a.E;
    const Row c = load_row(a.cand + row * a.ld_cand, E, lane);
    const Row v = load_row(a.img + b * a.ld_img, E, lane);
    float cc = 0.f;
#pragma unroll
    for (int i = 0; i < SCORE_VEC; ++i) cc += dot4(c.v[i], c.v[i]);
    cc = wave_sum(cc);
    float cv, vv;
    dot_and_norm(c, v, cv, vv);
    const float clip = a.w * fmaxf(cosine(cv, cc, vv), 0.f);
    float best = 0.f;                                               // max(0, .) over the set; an empty set leaves 0
    if (a.refs && (a.ref_s || a.refclip_s)) {
        // whatever the table holds, only rows [0, R) of refs are read: both ends are clamped, and end <= start is an empty set
        const int start = min(max(a.off[b], 0), a.R), end = min(max(a.off[b + 1], 0), a.R);
        if (start < end) {
            Row cur = load_row(a.refs + (int64_t)start * a.ld_ref, E, lane);
            for (int r = start; r < end; ++r) {
                const Row nxt = load_row(a.refs + (int64_t)min(r + 1, end - 1) * a.ld_ref, E, lane);   // (the last round re-reads its own row)
                float cr, rr;
                dot_and_norm(c, cur, cr, rr);
                best = fmaxf(best, cosine(cr, cc, rr));
                cur = nxt;
            }
        }
    }
    if (lane == 0) {
        a.clip_s[row] = clip;
        if (a.ref_s) a.ref_s[row] = best;
        if (a.refclip_s) {
            const float den = clip + best;
            a.refclip_s[row] = den > 0.f ? 2.f * clip * best / den : 0.f;
        }
    }
}

}  // namespace

extern "C" int dclip_clipscore(const float* img, int64_t ld_img, const float* cand, int64_t ld_cand, const float* refs, int64_t ld_ref,
                               const int32_t* ref_offsets, int64_t B, int64_t K, int64_t R, int64_t E, float w, float* clip_s, float* ref_s,
                               float* refclip_s, void* stream) {
    DCLIP_REQUIRE(img && cand && clip_s, "dclip_clipscore: null operand (img, cand and clip_s are required)");
    DCLIP_REQUIRE(B >= 1 && K >= 1 && R >= 0, "dclip_clipscore: need B >= 1, K >= 1, R >= 0 (B=%ld K=%ld R=%ld)", (long)B, (long)K, (long)R);
    DCLIP_REQUIRE(B < (1LL << 30) && K < (1LL << 30) && B * K < (1LL << 30) && R < (1LL << 31),
                  "dclip_clipscore: B K must stay below 2^30 and R below 2^31 (B=%ld K=%ld R=%ld)", (long)B, (long)K, (long)R);
    DCLIP_REQUIRE(E >= 4 && E % 4 == 0 && E <= 256 * SCORE_VEC, "dclip_clipscore: E=%ld must be a multiple of 4 in 4..%d", (long)E, 256 * SCORE_VEC);
    DCLIP_REQUIRE((refs != nullptr) == (ref_offsets != nullptr), "dclip_clipscore: refs and ref_offsets come together (one of them is null)");
    DCLIP_REQUIRE(refs || (!ref_s && !refclip_s), "dclip_clipscore: ref_s / refclip_s requested without refs");
    DCLIP_REQUIRE(ld_img >= E && ld_img % 4 == 0 && ld_cand >= E && ld_cand % 4 == 0 && (!refs || (ld_ref >= E && ld_ref % 4 == 0)),
                  "dclip_clipscore: row stride below E=%ld or not a multiple of 4 (ld_img=%ld ld_cand=%ld ld_ref=%ld)", (long)E, (long)ld_img,
                  (long)ld_cand, (long)ld_ref);
    DCLIP_REQUIRE(dclip_aligned16(img) && dclip_aligned16(cand) && dclip_aligned16(refs) && ((uintptr_t)ref_offsets % 4) == 0 &&
                  ((uintptr_t)clip_s % 4) == 0 && ((uintptr_t)ref_s % 4) == 0 && ((uintptr_t)refclip_s % 4) == 0,
                  "dclip_clipscore: misaligned pointer (img, cand and refs rows are read 16 bytes at a time)");
    ScoreArgs a;
    a.img = img; a.cand = cand; a.refs = refs; a.off = ref_offsets;
    a.ld_img = ld_img; a.ld_cand = ld_cand; a.ld_ref = ld_ref;
    a.rows = B * K; a.K = (int)K; a.R = (int)R; a.E = (int)E; a.w = w;
    a.clip_s = clip_s; a.ref_s = ref_s; a.refclip_s = refclip_s;
    hipLaunchKernelGGL(clipscore_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return dclip_check_launch("dclip_clipscore");
}
