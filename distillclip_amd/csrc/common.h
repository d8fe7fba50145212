// Common device/host helpers for the distill-step kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#include "dclip.h"   // DCLIP_OK / DCLIP_EINVAL (bad shape, dtype, alignment -> ValueError in Python) / DCLIP_ELAUNCH (-> RuntimeError)

// thread-local last-error string (include/dclip.h: dclip_last_error_string)
void dclip_set_error(const char* fmt, ...);

#define DCLIP_REQUIRE(cond, ...)                 \
    do {                                          \
        if (!(cond)) {                            \
            dclip_set_error(__VA_ARGS__);         \
            return DCLIP_EINVAL;                  \
        }                                         \
    } while (0)

// row moves of the last block execution run on the picked class / EOT rows only (elementwise.hip; used by encoder.cpp, not C ABI):
//   rows_pick   : dst[b] = src[idx[b]]                                       (compact [B, .] from [B*N, .])
//   rows_expand : dst[r] = r == idx[r / N] ? src[r / N] : 0 for every r < B*N (full [B*N, .] from compact [B, .])
// idx[b] lies in sample b's rows (dclip_pick_index); row_bytes a multiple of 16, buffers 16-byte aligned.
extern "C" int dclip_rows_pick(const void* src, void* dst, const int32_t* idx, int64_t B, int64_t row_bytes, void* stream);
extern "C" int dclip_rows_expand(const void* src, void* dst, const int32_t* idx, int64_t B, int64_t N, int64_t row_bytes, void* stream);

// dst bf16 [R, ldd] = src f32 [R, C], columns [C, ldd) zero (elementwise.hip; the frozen patch-14 towers' conv1 weight, whose contraction
// width is padded to a multiple of 64; used by encoder.cpp, not C ABI)
extern "C" int dclip_cast_bf16_pad(const float* src, void* dst, int64_t R, int64_t C, int64_t ldd, void* stream);

// launch trace (capi.cpp): open() returns false unless dclip_trace_begin() enabled tracing
bool dclip_trace_open(int kind, double flops, double bytes, void* stream, int* slot, int d0 = 0, int d1 = 0, int d2 = 0, int d3 = 0);
void dclip_trace_close(int slot, void* stream);
struct TraceScope {
    int slot = -1; void* st;
    TraceScope(int kind, double flops, double bytes, void* stream, int d0 = 0, int d1 = 0, int d2 = 0, int d3 = 0) : st(stream) {
        if (!dclip_trace_open(kind, flops, bytes, stream, &slot, d0, d1, d2, d3)) slot = -1;
    }
    ~TraceScope() { if (slot >= 0) dclip_trace_close(slot, st); }
};
#define DCLIP_TRACE_GEMM_NT 0
#define DCLIP_TRACE_GEMM_TN 1
#define DCLIP_TRACE_LAYERNORM 2
#define DCLIP_TRACE_LOSS 3
#define DCLIP_TRACE_ATTN 4
#define DCLIP_TRACE_LN_BWD 5

// a failed launch, in words (capi.cpp): names a second HIP runtime in the process or an invisible device where that is the cause
void dclip_explain_hip_error(const char* what, int hip_error, const char* hip_text);
static inline int dclip_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dclip_explain_hip_error(what, (int)e, hipGetErrorString(e));
        return DCLIP_ELAUNCH;
    }
    return DCLIP_OK;
}

// workgroups of a grid-stride launch: ceil(work / per_block), at least 1, at most cap
static inline int grid_for(int64_t work, int per_block = 256, int cap = 2048 * 4) {
    int64_t g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// workspaces: every piece starts on a 256-byte boundary; rows read 16 bytes per lane need 16-byte aligned operands
static inline size_t dclip_up256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline bool dclip_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
// carves a workspace front to back: take<T>(n) is the next piece of n elements, off the bytes handed out so far.  A null base
// only counts (the workspace-size queries).
struct Bump {
    char* base; size_t off;
    explicit Bump(void* b) : base((char*)b), off(0) {}
    template <class T> T* take(size_t n) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += dclip_up256(n * sizeof(T));
        return p;
    }
};

__device__ __forceinline__ float bf2f(bf16_t x) { return (float)x; }
__device__ __forceinline__ bf16_t f2bf(float x) { return (bf16_t)x; }   // v_cvt_pk_bf16_f32: RNE, NaN-preserving

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// LDS traffic of ONE wave (wave-private tiles).  The DS queue of a wave is in order, so a ds_read issued after a ds_write sees the
// data of every lane; all that is needed is that the compiler keeps the program order.  (A workgroup-scope release fence would also
// emit s_waitcnt vmcnt(0): the full latency of whatever global loads / LDS-DMA requests are in flight for the next tile.)
__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_wave_barrier(); asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

// MFMA source registers must outlive the MFMA's issue by ~10 issue slots.  The matrix pipe accepts MFMAs faster than it starts
// them: an MFMA that queues behind two or three others reads its A / B registers only when its turn comes, and neither the hardware
// nor hipcc's hazard recogniser keeps a VALU instruction from overwriting them meanwhile (asynchronous LDS / memory returns arrive
// late enough).  Found with H = 8, hd = 32: the compiler reused the packed dA operand of the LAST of four back-to-back mix MFMAs
// three instructions after it — wrong dS for the fourth key of every quad but the (peeled) first, deterministically, with no
// tool complaining (tools/diag/mix_fuzz.py; tools/asm/mfma_hazard.py now looks for it).  mfma_keep_alive() pins operands (one
// fragment, or a group of 2 or 4) until a point well past their MFMAs, at no cost in instructions.
template <class T> __device__ __forceinline__ void mfma_keep_alive(const T& f) { asm volatile("" :: "v"(f)); }
template <class T> __device__ __forceinline__ void mfma_keep_alive(const T (&f)[2]) { asm volatile("" :: "v"(f[0]), "v"(f[1])); }
template <class T> __device__ __forceinline__ void mfma_keep_alive(const T (&f)[4]) { asm volatile("" :: "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3])); }

__device__ __forceinline__ float quick_gelu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * x)); }   // v_rcp_f32: 1 ulp
// exact-GELU pieces with a branch-free erf (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7, i.e. at the f32 rounding level of
// libdevice's erff but ~4x fewer instructions; the activations are stored as bf16 anyway).  phi = exp(-x^2/2) is shared
// between erf(x / sqrt2) and the density term of the derivative.
__device__ __forceinline__ float erf_tail(float ax_over_sqrt2, float phi) {      // 1 - erf(|x|/sqrt2), phi = exp(-x^2/2)
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax_over_sqrt2, 1.f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    return p * t * phi;
}
__device__ __forceinline__ float gelu_erf_f(float x) {
    const float phi = __expf(-0.5f * x * x);
    const float tail = erf_tail(fabsf(x) * 0.70710678118654752f, phi);
    const float cdf = x >= 0.f ? 1.f - 0.5f * tail : 0.5f * tail;                // 0.5 (1 + erf(x / sqrt2))
    return x * cdf;
}
__device__ __forceinline__ float dgelu_erf_f(float x) {
    // d/dx [x Phi(x)] = Phi(x) + x phi(x) / sqrt(2 pi)
    const float phi = __expf(-0.5f * x * x);
    const float tail = erf_tail(fabsf(x) * 0.70710678118654752f, phi);
    const float cdf = x >= 0.f ? 1.f - 0.5f * tail : 0.5f * tail;
    return fmaf(x * phi, 0.3989422804014327f, cdf);
}

// gelu(x) and gelu'(x) together: the derivative costs two more instructions once the pieces of gelu are there, so the forward
// epilogue can hand the backward its factor instead of the pre-activation (DCLIP_ACT_GELU_SAVE / DCLIP_ACT_MULAUX).
__device__ __forceinline__ void gelu_erf_both_f(float x, float& g, float& dg) {
    const float phi = __expf(-0.5f * x * x);
    const float tail = erf_tail(fabsf(x) * 0.70710678118654752f, phi);
    const float cdf = x >= 0.f ? 1.f - 0.5f * tail : 0.5f * tail;
    g = x * cdf;
    dg = fmaf(x * phi, 0.3989422804014327f, cdf);
}

// gelu'(x) saved for the backward as 8-bit fixed point (DCLIP_ACT_GELU_SAVE writes it, DCLIP_ACT_MULAUX multiplies by it): the
// derivative of the exact GELU lies in [-0.1289, 1.1289]; code q = rint((g' - DG_LO) / DG_STEP) in 0..255, value DG_LO + q DG_STEP.
// |error| <= DG_STEP / 2 = 2.5e-3: on dz = dy g'(z) the same relative L2 error as a bf16 g' (DESIGN.md section 7), at half the bytes.
#define DCLIP_DG_LO (-0.13f)
#define DCLIP_DG_STEP (1.26f / 255.f)
__device__ __forceinline__ unsigned dg_pack4(float a, float b, float c, float d) {
    const float inv = 255.f / 1.26f, off = 0.13f * (255.f / 1.26f);
    unsigned r = 0;
    r = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(fmaf(a, inv, off)), 0, r);
    r = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(fmaf(b, inv, off)), 1, r);
    r = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(fmaf(c, inv, off)), 2, r);
    r = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(fmaf(d, inv, off)), 3, r);
    return r;
}
__device__ __forceinline__ float dg_unpack(unsigned w, int byte) {      // byte: compile-time constant 0..3
    return fmaf((float)((w >> (8 * byte)) & 0xffu), DCLIP_DG_STEP, DCLIP_DG_LO);
}

// bf16x8 MFMA fragment from its two 4-element halves (the two ds_read_b64_tr_b16 of a transposed read)
__device__ __forceinline__ bf16x8 frag_halves(s16x4 lo, s16x4 hi) {
    union { struct { s16x4 lo, hi; } s; bf16x8 v; } u;
    u.s.lo = lo; u.s.hi = hi;
    return u.v;
}

// k-major LDS tile fragment (16 columns from x0, 32 rows from r0; rows of ROWB bytes): two ds_read_b64_tr_b16.
// Lane l gets column x0 + (l & 15), contraction rows r0 + 8 (l >> 4) + (0..7).
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
template <int ROWB>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int r0, int x0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const char* a0 = tile + (r0 + 8 * g + q) * ROWB + (x0 + 4 * pp) * 2;
    return frag_halves(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0), __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * ROWB)));
}

// XCD-aware, bijective remap of a linear workgroup id: blocks that share an XCD (same id % 8 under the
// observed round-robin placement) get a contiguous chunk of the tile space, so neighbouring tiles share an L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
