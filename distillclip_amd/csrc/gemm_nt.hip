// Forward / dgrad bf16 MFMA GEMMs of the distill step (gfx950):
//
//   gemm_nt      C[M,N] = epi(alpha * A[M,K] · B[N,K]^T)      forward linears, dgrad (with pre-transposed W)
//
// Two kernels.  gemm_nt_kernel: 128x128x64 tile, 4 waves (2x2), each wave 64x64 = 4x4 tiles of v_mfma_f32_16x16x32_bf16; it serves the
// small problems and every launch the large kernel does not instantiate.  gemm_nt256_kernel: 192- / 256- / 320-row x 256-column tiles on
// the staggered two-phase pipeline below.  In both, operands go HBM -> LDS with global_load_lds (16 B/lane, no VGPR staging).  The LDS
// image is made of 1 KiB [16 rows x 32 k] sub-tiles (one per wave-instruction) with the st_16x32 XOR swizzle
// (byte ^= ((byte >> 9) & 1) << 5) applied on the SOURCE address and again on the ds_read_b128 address.
// The wgrad family (contraction over tokens) is gemm_tn.hip; what both share is gemm_common.h.

#include "gemm_common.h"
#include <atomic>

using namespace dgemm;

namespace {

constexpr int TILE_BYTES = (BM / 16) * (BK / 32) * SUB;   // 16 KiB per operand per stage
constexpr int CLD = BN + 4;                     // f32 row stride of the C tile staged through LDS in the epilogue
constexpr int NT_LDS = (4 * TILE_BYTES > BM * CLD * 4) ? 4 * TILE_BYTES : BM * CLD * 4;


// one wave stages 4 of the 16 sub-tiles of an operand tile
__device__ __forceinline__ void stage_operand(const bf16_t* __restrict__ G, int64_t ld, int row0, int rows_max,
                                              int k0, char* lds_tile, int wave, int lane) {
    const int L = lane * 16;
    const int X = swz(L);
    const int r = X >> 6, c = (X >> 4) & 3;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int sub = wave * 4 + s;          // sub = rb * 2 + kb
        const int rb = sub >> 1, kb = sub & 1;
        int row = row0 + rb * 16 + r;
        row = row < rows_max ? row : rows_max - 1;
        const bf16_t* src = G + (int64_t)row * ld + (k0 + kb * 32 + c * 8);
        __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(lds_tile + sub * SUB), 16, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------------
// gemm_nt_kernel: one 128x128 tile per workgroup, operands double buffered, one barrier per K-tile (the barrier's fence drains
// vmcnt, so tile kt has landed and every wave has left buffer (kt + 1) & 1 when the next tile is requested into it).
// Epilogue: the accumulators are staged through LDS (the operand buffers are dead by then) and the shared per-unit epilogue runs on
// row-contiguous 8-element vectors, 16-byte loads and stores.  This is the one kernel that keeps column sums with f32 / f16 output.
// ------------------------------------------------------------------------------------------------------
template <int ACT, int OUT>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmNT p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    const int nwg = p.tiles_m * p.tiles_n;
    const int t = xcd_remap(blockIdx.x, nwg);
    const int tm = t / p.tiles_n, tn = t % p.tiles_n;     // n fastest: the A row-panel stays in this XCD's L2
    const int m0 = tm * BM, n0 = tn * BN;

    char* As = smem;
    char* Bs = smem + 2 * TILE_BYTES;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / BK;
    stage_operand(p.A, p.lda, m0, p.M, 0, As, wave, lane);
    stage_operand(p.B, p.ldb, n0, p.N, 0, Bs, wave, lane);

    const int fragoff = swz((lane & 15) * 64 + (lane >> 4) * 16);

    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        if (kt + 1 < nk) {
            const int nb = (kt + 1) & 1;
            stage_operand(p.A, p.lda, m0, p.M, (kt + 1) * BK, As + nb * TILE_BYTES, wave, lane);
            stage_operand(p.B, p.ldb, n0, p.N, (kt + 1) * BK, Bs + nb * TILE_BYTES, wave, lane);
        }
        const char* a_t = As + (kt & 1) * TILE_BYTES;
        const char* b_t = Bs + (kt & 1) * TILE_BYTES;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                af[i] = *(const bf16x8*)(a_t + ((wm * 4 + i) * 2 + kb) * SUB + fragoff);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bfr[j] = *(const bf16x8*)(b_t + ((wn * 4 + j) * 2 + kb) * SUB + fragoff);
            mfma_4x4(acc, af, bfr);
        }
    }

    __syncthreads();
    float* cs = (float*)smem;
    stage_acc<4, CLD>(cs, acc, wm * 64, wn * 64, lane);
    __syncthreads();
    const int cc = (tid & 15) * 8;
    const int col = n0 + cc;
    const bool col_ok = col < p.N;
    float bias[8], csum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { bias[e] = 0.f; csum[e] = 0.f; }
    if (p.bias && col_ok) {
        const float4 b0 = *(const float4*)(p.bias + col), b1 = *(const float4*)(p.bias + col + 4);
        bias[0] = b0.x; bias[1] = b0.y; bias[2] = b0.z; bias[3] = b0.w; bias[4] = b1.x; bias[5] = b1.y; bias[6] = b1.z; bias[7] = b1.w;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int rl = (tid >> 4) + it * 16;
        const int row = m0 + rl;
        if (row >= p.M || !col_ok) break;
        const float4 c0 = *(const float4*)(cs + rl * CLD + cc), c1 = *(const float4*)(cs + rl * CLD + cc + 4);
        float v[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const int64_t o = (int64_t)row * p.ldc + col, orr = (int64_t)row * p.ldr + col;
        EpiSide sd;
        epilogue_load_side<ACT, OUT>(p, o, orr, sd);
        epilogue_vec8<ACT, OUT, 0, true>(p, v, row, col, o, orr, bias, csum, sd);     // every optional operand a run-time test, csum always kept
    }
    if (p.colsum) {
        // reduce the 16 row-groups through LDS so that each atomic wave-instruction covers 256 contiguous bytes
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) cs[(tid >> 4) * CLD + cc + e] = csum[e];
        __syncthreads();
        if (tid < BN && n0 + tid < p.N) {
            float x = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) x += cs[r * CLD + tid];
            unsafeAtomicAdd(p.colsum + n0 + tid, x);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// gemm_nt256_kernel: (32 MI) x 256 x 64 tile, MI = 6, 8 or 10 sixteen-row MFMA tiles per wave along M (192, 256 or 320 rows; the heights
// exist for wave quantisation, launch_nt picks one per problem).  8 waves (2 x 4, wave tile 16 MI x 64 = MI x 4 MFMA tiles, 16 MI
// accumulator registers), one workgroup per CU.
//   * LDS = [2 parities][B_lo, B_hi, A region of wave group 0, A region of wave group 1]; B halves are 128 rows x 64 k (16 KiB, the
//     swizzled [16 x 32] sub-tile image of the 128^2 kernel), an A region holds the group's MI row tiles.  The load stream moves
//     "half-tiles" staged by all 8 waves (2-3 global_load_lds per wave): B_lo, B_hi, A_up (the upper MI/2 row tiles of BOTH groups),
//     A_dn (the lower ones).
//   * a K-tile is 2 phases of 2 MI MFMAs x 2 (k halves): phase A = upper row tiles x all four column tiles (fragments: 8 B + MI A),
//     phase B = lower row tiles (MI A fragments, the B fragments stay in registers).  4 barriers per K-tile.
//   * load stream: B_lo, B_hi, A_up of tile kt + 2 are requested in phase B of tile kt, A_dn(kt + 1) in phase A of tile kt, so every
//     half-tile has two full phases to land — what the loop needs when all 256 CUs pull operands at once.
//   * vmcnt counting rule: vmcnt retires in issue order, so "half-tile X has landed" = s_waitcnt vmcnt(N) with N = the LDS-DMA
//     instructions this wave issued after X (B half 2, A row-half 2 at MI = 6 / 8 and 3 at MI = 10, the same for every wave).  Never 0
//     inside the loop except on the last tiles.
//   * WAR: a wave retires its own LDS reads (lgkmcnt(0)) BEFORE the phase's first barrier, so after any barrier every read issued
//     before it has completed and the regions refilled by the next phase's loads are idle.
//   * the two wave groups (wr = 0 / 1, one wave of each per SIMD) run one barrier apart: while one group issues its MFMAs the other
//     issues its ds_reads / LDS-DMA, so the matrix pipe of every SIMD stays fed.
//   * MFMA operands are swapped (C^T = B A^T) and the B rows permuted on the global side of the LDS-DMA (stage_half_perm), so a lane
//     ends up with 8 consecutive output columns and the epilogue stores straight from registers.
//   * no idle slots separate the last MFMA cluster from the epilogue: no VALU instruction of the epilogue writes a fragment register
//     within 12 slots of the MFMAs that read it, which tests/test_mfma_hazard_cpu.py checks on the shipped object.
// ------------------------------------------------------------------------------------------------------

// LDS bytes of both parities at tile height 32 mi: per parity two B halves and the two wave groups' A regions of 16 mi rows
constexpr int nt256_lds(int mi) { return 2 * (2 * HT + 2 * (mi * 16 * BK * 2)); }

// B half-tile: the sub-tile layout of the 128^2 kernel, but LDS row rho of sub-tile s (strip = s >> 2, j = s & 3) holds the operand row
// strip * 64 + (j >> 1) * 32 + (rho >> 2) * 8 + (j & 1) * 4 + (rho & 3).  With the MFMA operands swapped (C^T = B A^T) lane
// (g = lane >> 4, c = lane & 15) then owns, for output row c of row tile i, the accumulators acc[i][2 jp][0..3], acc[i][2 jp + 1][0..3]
// = 8 CONSECUTIVE output columns jp * 32 + g * 8 + (0..7) of the wave's 64-column strip: the epilogue stores straight from registers,
// 16 B (bf16) / 32 B (f32) per lane, 64 / 128 contiguous bytes per row, with no staging through LDS and no barrier.  The permutation
// is applied on the global-memory side of the LDS-DMA: free.
__device__ __forceinline__ void stage_half_perm(const bf16_t* __restrict__ G, int64_t ld, int row0, int rows_max, int k0,
                                                char* buf, int wave, int lane) {
    const int L = lane * 16;
    const int X = swz(L);
    const int r = X >> 6, c = (X >> 4) & 3;
    const int j = wave & 3;
    int row = row0 + (wave >> 2) * 64 + (j >> 1) * 32 + (r >> 2) * 8 + (j & 1) * 4 + (r & 3);
    row = row < rows_max ? row : rows_max - 1;
    const bf16_t* src = G + (int64_t)row * ld + k0 + c * 8;
    __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(buf + (wave * 2 + 0) * SUB), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void*)(src + 32), (lds_void*)(buf + (wave * 2 + 1) * SUB), 16, 0, 0);
}

// A "row-half": the upper (dn = 0) or lower (dn = 1) RH row tiles of BOTH wave groups, written to the LDS addresses the fragment
// reads expect (group g's region at g * HTA, row tile i at sub-tiles 2 i, 2 i + 1).  Every wave issues the same number of LDS-DMA
// instructions, so the counted vmcnt waits stay wave-independent: with RH = 3 the six row blocks go to eight waves and waves 6, 7
// repeat blocks 0, 1 (same bytes to the same LDS address); with RH = 5 row blocks 0-7 go by wave and the remaining two are split in
// four [16 x 32] pieces over waves 0-3, which waves 4-7 repeat.
template <int RH>
__device__ __forceinline__ void stage_rowhalf(const bf16_t* __restrict__ G, int64_t ld, int m0, int rows_max, int k0,
                                              char* abase, int hta, int dn, int wave, int lane) {
    const int L = lane * 16;
    const int X = swz(L);
    const int r = X >> 6, c = (X >> 4) & 3;
    constexpr int AROWS = RH * 32;
    {
        const int wv = RH == 3 ? wave % 6 : wave;
        const int g = wv / RH, i = wv % RH + dn * RH;              // row block `wv` of 2 RH
        int row = m0 + g * AROWS + i * 16 + r;
        row = row < rows_max ? row : rows_max - 1;
        const bf16_t* src = G + (int64_t)row * ld + k0 + c * 8;
        char* dst = abase + g * hta + (i * 2) * SUB;
        __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void*)(src + 32), (lds_void*)(dst + SUB), 16, 0, 0);
    }
    if (RH == 5) {
        const int e = wave & 3, rbk = 8 + (e >> 1), kb = e & 1;
        const int g = rbk / RH, i = rbk % RH + dn * RH;
        int row = m0 + g * AROWS + i * 16 + r;
        row = row < rows_max ? row : rows_max - 1;
        const bf16_t* src = G + (int64_t)row * ld + k0 + kb * 32 + c * 8;
        __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(abase + g * hta + (i * 2 + kb) * SUB), 16, 0, 0);
    }
}

// sum over the 16 lanes of a DPP row (= the 16 rows a lane group holds of one output column), in every lane of the row: quad swaps,
// then the half-row and row mirrors.  VALU only: no LDS round trip per step and no lane index kept alive through the tile loop.
__device__ __forceinline__ float row16_sum(float x) {
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, false));
    };
    x += dpp(x, std::integral_constant<int, 0xB1>{});     // quad_perm [1, 0, 3, 2]
    x += dpp(x, std::integral_constant<int, 0x4E>{});     // quad_perm [2, 3, 0, 1]
    x += dpp(x, std::integral_constant<int, 0x141>{});    // row_half_mirror
    x += dpp(x, std::integral_constant<int, 0x140>{});    // row_mirror
    return x;
}

template <int ACT, int OUT, int MI>
__global__ __launch_bounds__(512) void gemm_nt256_kernel(GemmNT p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RH = MI / 2;                      // row tiles per phase
    constexpr int AROWS = MI * 16;                  // rows of an A half-tile (one wave group's rows)
    constexpr int HTA = AROWS * BK * 2;             // bytes of an A half-tile
    constexpr int PAR = nt256_lds(MI) / 2;          // one parity: B_lo, B_hi, A_lo, A_hi
    constexpr int BMT = 2 * AROWS;                  // tile rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    // Tile raster inside an XCD's chunk: groups of group_n column tiles, rows fastest-but-one.  With n fastest over ALL column
    // tiles the 32 concurrent tiles of an XCD span every B panel (N = 3072, K = 768: 4.7 MB, more than the 4 MB L2), so B is
    // re-streamed from beyond L2 once per round; with a group whose B panels stay L2-resident an XCD streams its A rows once
    // per group and reads B once (host-side choice and traffic model: raster_group_n).
    const int nwg = p.tiles_m * p.tiles_n;
    const int nk = p.K / BK;
    const int nload = 4 * nk;
    int m0, n0;
    auto locate = [&](int tl) {
        const int t = xcd_remap(tl, nwg);
        int tm, tn;
        if (p.group_n >= p.tiles_n) { tm = t / p.tiles_n; tn = t % p.tiles_n; }
        else {
            const int per = p.tiles_m * p.group_n;
            const int gi = t / per, rem = t - gi * per;
            const int left = p.tiles_n - gi * p.group_n;
            const int gw = left < p.group_n ? left : p.group_n;
            tm = rem / gw; tn = gi * p.group_n + rem % gw;
        }
        m0 = tm * BMT; n0 = tn * 256;
    };
    locate(blockIdx.x);

    f32x4 acc[MI][4];

    // half-tile l = 4*tile + w ; w: 0 B_lo, 1 B_hi, 2 A_up (upper row tiles of both wave groups), 3 A_dn (lower row tiles)
    auto issue = [&](int l) {
        const int tile = l >> 2, w = l & 3;
        char* par = smem + (tile & 1) * PAR;
        if (w < 2) stage_half_perm(p.B, p.ldb, n0 + w * 128, p.N, tile * BK, par + w * HT, wave, lane);
        else stage_rowhalf<RH>(p.A, p.lda, m0, p.M, tile * BK, par + 2 * HT, HTA, w - 2, wave, lane);
    };
    wg_stamp(p.stamps, tid, 0);
    if (p.clk && blockIdx.x == 0 && tid == 0) { p.clk[0] = __builtin_amdgcn_s_memtime(); p.clk[1] = __builtin_amdgcn_s_memrealtime(); }
    // the counted wait of the header's rule, per tile height: n10 at MI = 10 (3 LDS-DMA instructions per A row-half), n8 otherwise (2)
#define WAIT_VM2(n8, n10) do { if (MI == 10) WAIT_VMCNT(n10); else WAIT_VMCNT(n8); } while (0)
    const int npro = nload < 7 ? nload : 7;                // tile 0 entirely, tile 1: B_lo, B_hi, A_up
    for (int l = 0; l < npro; ++l) issue(l);
    const int a_off = 2 * HT + wr * HTA;                     // this wave's A half
    const int b_off = (wc >> 1) * HT + (wc & 1) * 8 * SUB;   // this wave's B half, its 4 column blocks start at (wc&1)*4
    const int fragoff = swz((lane & 15) * 64 + (lane >> 4) * 16);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B_lo, B_hi, A_up of K-tile 0 landed (younger: A_dn(0), B, B, A_up(1))
    if (nload > 4) WAIT_VM2(8, 10); else WAIT_VMCNT(0);
    __builtin_amdgcn_s_barrier();
    wg_stamp(p.stamps, tid, 1);
    if (wr == 1) __builtin_amdgcn_s_barrier();            // stagger: the wr = 1 group runs one barrier behind

    bf16x8 af[RH][2], b0[2][2], b1[2][2];

    for (int kt = 0; kt < nk; ++kt) {
        const char* base = smem + (kt & 1) * PAR;
        const char* ap = base + a_off + fragoff;
        const char* bp = base + b_off + fragoff;
        // ---------------- phase A : upper row tiles ----------------
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                b0[j][kb] = *(const bf16x8*)(bp + (j * 2 + kb) * SUB);
                b1[j][kb] = *(const bf16x8*)(bp + ((2 + j) * 2 + kb) * SUB);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < RH; ++i)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) af[i][kb] = *(const bf16x8*)(ap + (i * 2 + kb) * SUB);
        if (kt + 1 < nk) { issue(4 * (kt + 1) + 3); WAIT_VM2(8, 10); }  // request A_dn(kt + 1); A_dn(kt) landed (younger: B, B, A_up, A_dn(kt + 1))
        else WAIT_VMCNT(0);
        WAIT_LGKM0();
        PHASE_MFMA(true, acc, 0, RH, af, b0, b1);
        // ---------------- phase B : lower row tiles ----------------
#pragma unroll
        for (int i = 0; i < RH; ++i)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) af[i][kb] = *(const bf16x8*)(ap + ((RH + i) * 2 + kb) * SUB);
        // request B_lo, B_hi, A_up(kt + 2); B_lo, B_hi, A_up(kt + 1) landed (younger: A_dn(kt + 1) and the three just issued)
        if (kt + 2 < nk) { issue(4 * (kt + 2)); issue(4 * (kt + 2) + 1); issue(4 * (kt + 2) + 2); WAIT_VM2(8, 10); }
        else if (kt + 1 < nk) WAIT_VM2(2, 3);
        else WAIT_VMCNT(0);
        WAIT_LGKM0();
        PHASE_MFMA(true, acc, RH, RH, af, b0, b1);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();            // re-align the two groups
    wg_stamp(p.stamps, tid, 2);
    const int g = lane >> 4, rl = lane & 15;

    // epilogue, straight from registers (see stage_half_perm): lane (g, c) owns row c of every row tile i and, per column pair
    // jp, 8 consecutive columns.  No LDS, no barrier: a wave starts storing as soon as its own accumulators are final.  Side
    // operands (the f32 residual, which may alias C in place, and the aux rows of the DGELU / MULAUX variants) of row tile
    // i + 1 are requested before the stores of row tile i are issued, so that their in-order vmcnt wait never includes a store.
    const int colb = n0 + wc * 64 + g * 8;
    float bias[2][8], csum[2][8];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { bias[jp][e] = 0.f; csum[jp][e] = 0.f; }
        const int col = colb + jp * 32;
        if (p.bias && col < p.N) {
            const float4 q0 = *(const float4*)(p.bias + col), q1 = *(const float4*)(p.bias + col + 4);
            bias[jp][0] = q0.x; bias[jp][1] = q0.y; bias[jp][2] = q0.z; bias[jp][3] = q0.w;
            bias[jp][4] = q1.x; bias[jp][5] = q1.y; bias[jp][6] = q1.z; bias[jp][7] = q1.w;
        }
    }
    // units u = 2 i + jp, processed in batches of BU: a batch's side operands are all requested before its first store.  vmcnt
    // retires loads and stores in ONE in-order queue, so a load issued after a store cannot be waited for without also waiting
    // for that store's acknowledgement; with batches the wave pays that once per batch boundary, and not at all where the side
    // operands of the whole tile fit the registers the dead fragments free.
    constexpr bool OUT_F32 = OUT == 1;               // (f32 units are 32 B per lane: smaller side-operand batches)
    constexpr bool SIDE = OUT != 0 || ACT == 3 || ACT == 4;
    constexpr int NU = 2 * MI;
    constexpr int BU = !SIDE ? NU : (OUT_F32 ? ((ACT == 3 || ACT == 4) ? 4 : (MI == 8 ? 8 : (MI == 6 ? 6 : 5))) : (MI == 10 ? 10 : NU));
    static_assert(NU % BU == 0, "batch size must divide the unit count");
    EpiSide side[SIDE ? BU : 1];
    const int row0 = m0 + wr * AROWS + rl;
    const int64_t o0 = (int64_t)row0 * p.ldc + colb, r0off = (int64_t)row0 * p.ldr + colb;
    const int64_t ostep = 16 * p.ldc, rstep = 16 * p.ldr;
    // full: the tile lies inside the matrix (all but the last row / column of tiles) — the per-unit bounds test is then one scalar
    // branch instead of two vector compares and an exec-mask update.  (Compiled out entirely, the 2 MI units become one basic block
    // whose addresses and conversions are all hoisted to the top: 100-240 spilled registers.)
    const bool full = m0 + BMT <= p.M && n0 + 256 <= p.N;
    auto run_units = [&](auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
#pragma unroll
        for (int ub = 0; ub < NU; ub += BU) {
            if (SIDE) {
#pragma unroll
                for (int u = ub; u < ub + BU; ++u) {
                    const int i = u >> 1, jp = u & 1;
                    if (full || (row0 + i * 16 < p.M && colb + jp * 32 < p.N))
                        epilogue_load_side<ACT, OUT>(p, o0 + i * ostep + jp * 32, r0off + i * rstep + jp * 32, side[u - ub]);
                }
            }
#pragma unroll
            for (int u = ub; u < ub + BU; ++u) {
                const int i = u >> 1, jp = u & 1;
                const int row = row0 + i * 16, col = colb + jp * 32;
                if (full || (row < p.M && col < p.N)) {
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { v[r] = acc[i][2 * jp][r]; v[4 + r] = acc[i][2 * jp + 1][r]; }
                    epilogue_vec8<ACT, OUT, MODE>(p, v, row, col, o0 + i * ostep + jp * 32, r0off + i * rstep + jp * 32, bias[jp], csum[jp],
                                                      side[SIDE ? u - ub : 0]);
                }
            }
        }
    };
    // (kernel arguments: the tests below are scalar, the whole workgroup takes one path)
    const bool lean = p.row_group == 0 && ((ACT == 5 || ACT == 6) ? p.aux_out != nullptr : p.aux_out == nullptr) && (OUT != 0 ? p.residual != nullptr : p.residual == nullptr);
    if constexpr (OUT != 0) {
        if (lean) run_units(std::integral_constant<int, 3>{});
        else run_units(std::integral_constant<int, 0>{});
    } else if constexpr (ACT == 3 || ACT == 4) {      // (the dgrad epilogues always come with bias-gradient column sums in the step)
        if (lean && p.colsum) run_units(std::integral_constant<int, 2>{});
        else run_units(std::integral_constant<int, 0>{});
    } else {
        if (lean && !p.colsum) run_units(std::integral_constant<int, 1>{});
        else if (lean) run_units(std::integral_constant<int, 2>{});
        else run_units(std::integral_constant<int, 0>{});
    }
    if (OUT == 0 && p.colsum) {     // (f32 / f16 output + column sums: launch_nt routes that combination to the 128^2 kernel)
        // 16-lane shuffle reduce, then the 8 waves combine through LDS (idle since the main loop's last barrier) so that the
        // workgroup issues 4 atomic wave-instructions for its 256 columns: the chip retires about one atomic wave-instruction per
        // 50 ns and CU whatever its width
        float* cs = (float*)smem;                   // [2 wave groups][256 columns]
#pragma unroll
        for (int jp = 0; jp < 2; ++jp)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = row16_sum(csum[jp][e]);
                if (rl == 0) cs[wr * 256 + wc * 64 + jp * 32 + g * 8 + e] = x;
            }
        WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
        const int tc = wave * 64 + lane;            // (= tid, from the scalar wave index: spelled tid, hipcc forms the addresses of the unit loop differently)
        if (tc < 256 && n0 + tc < p.N) unsafeAtomicAdd(p.colsum + n0 + tc, cs[tc] + cs[256 + tc]);
    }
    wg_stamp(p.stamps, tid, 3);
    if (p.clk && blockIdx.x == 0 && tid == 0) { p.clk[2] = __builtin_amdgcn_s_memtime(); p.clk[3] = __builtin_amdgcn_s_memrealtime(); }
}

// DCLIP_GEMM256=0: every shape on the 128^2 kernel (the one fallback of this stage); default: the 256- / 320- / 192-row kernel for
// every shape it tiles — with the towers on four streams, other kernels fill its tail rounds
bool use_256(const GemmNT& p) {
    static const int mode = [] { const char* e = getenv("DCLIP_GEMM256"); return e ? atoi(e) : 1; }();
    return mode != 0 && p.M >= 1024 && p.N >= 256;
}

// clock probe (dclip_trace_gemm_clock): slot of the next 256- / 320- / 192-row launch, null when the probe is off
std::atomic<unsigned long long*> g_clock_buf{nullptr};
std::atomic<long long> g_clock_cap{0};
std::atomic<long long> g_clock_count{0};
inline unsigned long long* next_clock_slot() {
    unsigned long long* buf = g_clock_buf.load(std::memory_order_acquire);
    const long long cap = g_clock_cap.load(std::memory_order_relaxed);
    if (!buf || cap <= 0) return nullptr;
    return buf + 4 * (g_clock_count.fetch_add(1, std::memory_order_relaxed) % cap);
}

// Tile height of the large kernel: 192, 256 or 320 rows (MI = 6, 8, 10), whichever needs the fewest rounds x cycles per tile on 256 CUs;
// a tie keeps the 256-row tile, whose loads carry no duplicates.  DCLIP_GEMM320=0 keeps 256 rows, =2 forces 320, =6 forces 192.
// The taller tile exists for wave quantisation: a [25600, 768] output is 300 tiles of 256^2 (two rounds on 256 CUs, the second 17 %
// full) but 240 tiles of 320 x 256 (one round); the 192-row tile serves M = 12 800 problems, where 320 x 256 tiles leave half the CUs
// idle at N = 768.  Every epilogue variant fits the 160 accumulator registers of the 320-row tile without spilling (tools/diag/regs.py).
// Cycle figures: in-kernel stamps (tools/diag/gemm_phases.py) of the four-phase schedule this kernel had when the model was fitted —
// prologue 3.3 k, main loop 2 750 (256 rows) / 3 200 (320 rows) cycles per K-tile, the 192-row tile priced at 0.78 x the 256-row one,
// and an epilogue that scales with the rows (bf16 ~9.5 k, f32 + residual ~40 k when the whole chip stores).  The two-phase schedule
// above runs 2 465 / 2 995; the model was not refitted, since the ratios decide and they moved by < 5 %.
int tile_height_mi(const GemmNT& p, int act, int out) {
    static const int mode320 = [] { const char* e = getenv("DCLIP_GEMM320"); return e ? atoi(e) : 1; }();
    if (!mode320) return 8;
    if (mode320 == 2) return 10;
    if (mode320 == 6) return 6;
    const int tn = (p.N + 255) / 256;
    const double nkt = (double)(p.K / BK), e8 = out == 1 ? 40000.0 : out == 2 ? 24000.0 : (act == 0 || act == 4 ? 9500.0 : 14000.0);
    auto cost = [&](int rows, double per_kt, double escale) {
        const int tmx = (p.M + rows - 1) / rows;
        return (double)((tmx * tn + 255) / 256) * (3300.0 + nkt * per_kt + escale * e8);
    };
    const double c8 = cost(256, 2750.0, 1.0), c10 = cost(320, 3200.0, 1.25), c6 = cost(192, 2150.0, 0.75);
    int mi = 8;
    if (c10 < c8) mi = 10;
    if (c6 < (mi == 10 ? c10 : c8) * 0.97) mi = 6;
    return mi;
}

// Raster group width (column tiles per group, p.tiles_m / p.tiles_n set): minimise the modelled operand bytes from beyond L2 — A once
// per group, B once per XCD while a group's B panels (256 x K bf16 each) fit ~2.5 MB of the XCD's 4 MB L2, else once per round of 32
// tiles per XCD
int raster_group_n(const GemmNT& p) {
    const int tn = p.tiles_n, ntiles = p.tiles_m * p.tiles_n;
    const double panel = 512.0 * (double)p.K, a_bytes = 2.0 * (double)p.M * (double)p.K;
    double best = 0.0; int best_g = tn;
    for (int g = 1; g <= tn; ++g) {
        const int ngroups = (tn + g - 1) / g;
        const double b_term = (g * panel <= 2.5e6) ? 8.0 * g * panel * (ngroups > 8 ? ngroups / 8.0 : 1.0)
                                                   : (double)ntiles / 32.0 * g * panel;
        const double cost = a_bytes * ngroups + b_term;
        if (g == 1 || cost < best * 0.999) { best = cost; best_g = g; }
    }
    return best_g;
}

// the large kernel instantiates an activation with the bf16 store only, and f32 / f16 output for the plain epilogue only (launch_nt)
template <int ACT, int MI>
void launch_nt256(const GemmNT& p, int out, hipStream_t st) {
    const dim3 grid(p.tiles_m * p.tiles_n), block(512);
    constexpr size_t lds = nt256_lds(MI) + 16;
    if (out == 1) { if constexpr (ACT == 0) hipLaunchKernelGGL((gemm_nt256_kernel<0, 1, MI>), grid, block, lds, st, p); }
    else if (out == 2) { if constexpr (ACT == 0) hipLaunchKernelGGL((gemm_nt256_kernel<0, 2, MI>), grid, block, lds, st, p); }
    else hipLaunchKernelGGL((gemm_nt256_kernel<ACT, 0, MI>), grid, block, lds, st, p);
}

template <int ACT>
int launch_nt(GemmNT p, int out, hipStream_t st) {
    // OUT = 2 (f16 output + f16 in-place residual: the frozen teacher's residual stream) exists for the plain epilogue only
    if constexpr (ACT != 0) { if (out == 2) { dclip_set_error("dclip_gemm_nt: f16 output needs act = DCLIP_ACT_NONE"); return DCLIP_EINVAL; } }
    // (the 256- / 320-row kernels keep column sums only with bf16 output, and an activation only with bf16 output: the step's activated
    //  GEMMs all store bf16 — an f32 store after an activation is served by the 128^2 kernel, 15 instantiations less in the library)
    if (use_256(p) && !(out != 0 && p.colsum) && (ACT == 0 || out == 0)) {
        const int mi = tile_height_mi(p, ACT, out);
        p.tiles_m = (p.M + mi * 32 - 1) / (mi * 32); p.tiles_n = (p.N + 255) / 256;
        p.clk = next_clock_slot();
        p.group_n = raster_group_n(p);
        if (mi == 10) launch_nt256<ACT, 10>(p, out, st);
        else if (mi == 6) launch_nt256<ACT, 6>(p, out, st);
        else launch_nt256<ACT, 8>(p, out, st);
        return dclip_check_launch("dclip_gemm_nt");
    }
    const int grid = p.tiles_m * p.tiles_n;
    const size_t lds = NT_LDS;
    if (out == 1) hipLaunchKernelGGL((gemm_nt_kernel<ACT, 1>), dim3(grid), dim3(256), lds, st, p);
    else if (out == 2) { if constexpr (ACT == 0) hipLaunchKernelGGL((gemm_nt_kernel<0, 2>), dim3(grid), dim3(256), lds, st, p); }
    else hipLaunchKernelGGL((gemm_nt_kernel<ACT, 0>), dim3(grid), dim3(256), lds, st, p);
    return dclip_check_launch("dclip_gemm_nt");
}

}  // namespace

extern "C" int dclip_trace_gemm_stamps(void* buf) { g_gemm_stamps = (unsigned long long*)buf; return 0; }
extern "C" int64_t dclip_trace_gemm_clock(void* buf, int64_t cap) {
    const long long n = g_clock_count.exchange(0, std::memory_order_relaxed);
    g_clock_cap.store(buf ? (long long)cap : 0, std::memory_order_relaxed);
    g_clock_buf.store((unsigned long long*)buf, std::memory_order_release);
    return (int64_t)n;
}

extern "C" int dclip_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, float alpha, const float* bias, int act,
                             const void* aux_in, void* aux_out, const void* residual, int64_t ldr, int out_dtype,
                             int64_t row_group, const float* rowadd, float* colsum_acc, void* stream) {
    DCLIP_REQUIRE(A && B && C, "dclip_gemm_nt: null operand");
    DCLIP_REQUIRE(M > 0 && N > 0 && K > 0, "dclip_gemm_nt: empty problem M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
    DCLIP_REQUIRE(K % BK == 0, "dclip_gemm_nt: K=%ld must be a multiple of %d", (long)K, BK);
    DCLIP_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0,
                  "dclip_gemm_nt: operand rows must be 16-byte aligned (lda=%ld ldb=%ld)", (long)lda, (long)ldb);
    DCLIP_REQUIRE(N % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)C % 16) == 0, "dclip_gemm_nt: N and ldc must be multiples of 8 and C 16-byte aligned (N=%ld ldc=%ld)", (long)N, (long)ldc);
    DCLIP_REQUIRE(out_dtype >= 0 && out_dtype <= 2, "dclip_gemm_nt: bad output dtype %d (0 bf16, 1 f32, 2 f16)", out_dtype);
    DCLIP_REQUIRE(!residual || (ldr % (out_dtype == 2 ? 8 : 4) == 0 && ((uintptr_t)residual % 16) == 0), "dclip_gemm_nt: residual rows must be 16-byte aligned");
    DCLIP_REQUIRE(act >= 0 && act <= 6, "dclip_gemm_nt: bad activation code %d", act);
    DCLIP_REQUIRE(out_dtype != 2 || act == 0, "dclip_gemm_nt: f16 output needs act = DCLIP_ACT_NONE");
    DCLIP_REQUIRE((act != DCLIP_ACT_DGELU && act != DCLIP_ACT_MULAUX) || aux_in, "dclip_gemm_nt: DGELU / MULAUX need aux_in");
    DCLIP_REQUIRE(!aux_in || ((uintptr_t)aux_in % 16) == 0, "dclip_gemm_nt: aux_in must be 16-byte aligned");
    DCLIP_REQUIRE(!aux_out || ((uintptr_t)aux_out % 16) == 0, "dclip_gemm_nt: aux_out must be 16-byte aligned");
    DCLIP_REQUIRE(row_group == 0 || rowadd, "dclip_gemm_nt: row_group needs rowadd");
    DCLIP_REQUIRE(M < (1LL << 31) && N < (1LL << 31), "dclip_gemm_nt: dimension overflow");
    GemmNT p;
    p.A = (const bf16_t*)A; p.lda = lda; p.B = (const bf16_t*)B; p.ldb = ldb; p.C = C; p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.alpha = alpha; p.bias = bias;
    p.aux_in = aux_in; p.aux_out = aux_out; p.residual = residual; p.ldr = ldr;
    p.row_group = (int)row_group; p.rowadd = rowadd; p.colsum = colsum_acc;
    p.tiles_m = (int)((M + BM - 1) / BM); p.tiles_n = (int)((N + BN - 1) / BN);
    p.stamps = g_gemm_stamps;
    p.group_n = 1 << 30;
    p.clk = nullptr;
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes of the call: both operands once, the output once, plus what the fused epilogue consumes / produces — the f32 residual
    // it adds (read), the saved pre-activation / derivative it multiplies by (aux_in) or stores (aux_out)
    const int out_f32 = out_dtype == 1;
    const double aux_b = (act == DCLIP_ACT_MULAUX || act == DCLIP_ACT_GELU_SAVE || act == DCLIP_ACT_QUICKGELU_SAVE) ? 1.0 : 2.0;      // the saved gelu' is one byte per element
    TraceScope tr(DCLIP_TRACE_GEMM_NT, 2.0 * (double)M * (double)N * (double)K,
                  2.0 * ((double)M * K + (double)N * K) + ((out_f32 ? 4.0 : 2.0) + (residual ? (out_dtype == 2 ? 2.0 : 4.0) : 0.0) + (aux_in ? aux_b : 0.0) + (aux_out ? aux_b : 0.0)) * (double)M * N,
                  stream, (int)M, (int)N, (int)K,
                  act + 8 * (out_f32 != 0) + 16 * (residual != nullptr) + 32 * (colsum_acc != nullptr) + 64 * (out_dtype == 2));
    switch (act) {
        case 0: return launch_nt<0>(p, out_dtype, st);
        case 1: return launch_nt<1>(p, out_dtype, st);
        case 2: return launch_nt<2>(p, out_dtype, st);
        case 3: return launch_nt<3>(p, out_dtype, st);
        case 4: return launch_nt<4>(p, out_dtype, st);
        case 5: return launch_nt<5>(p, out_dtype, st);
        default: return launch_nt<6>(p, out_dtype, st);
    }
}
