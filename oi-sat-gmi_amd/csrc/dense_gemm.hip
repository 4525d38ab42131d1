// The fp32 GEMMs of the dense solver,  C[MxN] (-)= A[MxK] * B[NxK]^T  on v_mfma_f32_32x32x2_f32: gemm_nt_big (one tile per workgroup,
// K >= 2048), gemm_nt (persistent, C prefetched across tiles), gemm_nt_small and gemm_nt_rows64 (64-row tiles for launches that
// cannot fill the chip), each single and batched, with launch_gemm / launch_gemm_batched and the batched launches' tile tables.
// The tile, the LDS image and the software pipeline are described at the top of dense_chol.hip, whose schedules are the callers;
// dense_post.hip's row solves call launch_gemm too.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"

// ---- batched launches -------------------------------------------------------------------------
// Many independent factorizations (the tiles of a localised analysis, the months of a batch) advance in LOCK-STEP:
// one launch applies the same node of the recursion to every matrix -- blockIdx.y picks the matrix from a device
// table, blockIdx.x its tile -- so that a step which is a 1-workgroup kernel or a 40-tile GEMM for one 6,000-
// observation tile becomes one launch that fills the chip, and the chain of dependent launches is paid once per batch
// instead of once per tile.  The table is sorted by block count (largest first): the matrices a node applies to are a
// prefix of it.  Operands are derived in the kernel from (table entry, node), so nothing is uploaded per launch.
// (BatchArgs, one such launch: dense_internal.h -- the factorization schedules fill it in)

// operands of matrix `which` for this node, in units of `unit` rows/columns (128 or 64); false: the node does not apply
__device__ __forceinline__ bool batch_operands(const BatchArgs& ba, int which, int unit, float*& C, int64_t& ldc, const float*& A,
                                               int64_t& lda, const float*& B, int64_t& ldb, int& ntm, int& ntn) {
    const BatchMat m = ba.mats[which];
    const int per = NB / unit;
    if (ba.kind == 0) {                                     // S[mid:, mid:b1] -= L[mid:, b0:mid] * L[mid:b1, b0:mid]^T
        const int rows = m.mpb - ba.mid, cols = (ba.b1 < m.mpb ? ba.b1 : m.mpb) - ba.mid;
        if (rows <= 0 || cols <= 0) return false;
        ntm = rows * per;
        ntn = cols * per;
        C = m.S + (int64_t)ba.mid * NB * m.ld + (int64_t)ba.mid * NB;
        A = m.S + (int64_t)ba.mid * NB * m.ld + (int64_t)ba.b0 * NB;
        B = A;
        ldc = lda = ldb = m.ld;
    } else {                                                // P <- P * T_b0^T, P = S[(b0+1)*128:, b0*128 : (b0+1)*128], in place
        const int rows = m.mpb - ba.b0 - 1;
        if (rows <= 0) return false;
        ntm = rows * per;
        ntn = per;
        float* P = m.S + (int64_t)(ba.b0 + 1) * NB * m.ld + (int64_t)ba.b0 * NB;
        C = P;
        A = P;
        ldc = lda = m.ld;
        B = m.tinv + (int64_t)ba.b0 * NB * NB;
        ldb = NB;
    }
    return true;
}

// Virtual id -> work item for launches whose ids are NOT all equally loaded (batched launches: the ids past a smaller
// matrix's tile count are empty).  Workgroups go to the 8 XCDs round-robin in dispatch order; giving each XCD one
// contiguous eighth of the whole range (as gemm_nt_big does for a single matrix) would hand some XCDs mostly empty ids.
// Instead every run of 512 ids is dealt out in 64-id chunks: id 512g + 8s + x (XCD x, its s-th workgroup of the run)
// -> 512g + 64x + s, so an XCD still works on 64 consecutive items (an 8x8 patch of tiles in row-band order) and all
// XCDs sweep the range together.  The ragged tail of the range keeps its ids.
__device__ __forceinline__ int64_t xcd_chunk_remap(int64_t v, int64_t total) {
    const int64_t g = v >> 9;
    if (((g + 1) << 9) > total) return v;
    const int64_t x = v & 7, sidx = (v >> 3) & 63;
    return (g << 9) + (x << 6) + sidx;
}

// ---- gemm_nt_big: one tile per workgroup, for K >= 2048 --------------------------------------------------------------
// The kernel the headline factorization spends 95 % of its time in (round 1's gemm_nt, unchanged): with 64+ K-steps per
// tile the 22 us of per-tile overhead are < 10 %, and this instruction schedule of the K-loop sustains 140 TFLOP/s at
// 8192^3 where the pipelined-across-tiles kernel below, with 64 more live registers for the prefetched C tile, reaches
// 135 (measured: K = 1024: 913 vs 870 us for 3240 tiles, K = 2048: 1683 vs 1684, K = 5120: 4054 vs 4250).
template <bool BATCH>
__global__ __launch_bounds__(256, 2) void gemm_nt_big_kernel(float* C, int64_t ldc, const float* A,
                                                          int64_t lda, const float* __restrict__ B, int64_t ldb, int ntm,
                                                          int ntn, int K, int mode, int lower, int ntiles_total, BatchArgs ba) {
    if (BATCH) group_prio(ba.prio);
    __shared__ __attribute__((aligned(16))) float lds[2][2][NB * BK];        // [buf][A|B][row*32 + 4*(chunk ^ (row&7))] = 65,536 B
    int wg;
    if (BATCH) {
        const float* Bb = nullptr;
        // Workgroups go to the 8 XCDs round-robin in dispatch order (x fastest, then y): chunked remap over the 2-D grid
        // (xcd_chunk_remap), so that neighbouring tiles of the same matrix share an L2 and no XCD is left with the
        // empty ids of the smaller matrices.
        const int64_t total = (int64_t)gridDim.x * gridDim.y, orig = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t lin = xcd_chunk_remap(orig, total);
        const int which = (int)(lin / gridDim.x);
        if (!batch_operands(ba, which, NB, C, ldc, A, lda, Bb, ldb, ntm, ntn)) return;
        B = Bb;
        wg = (int)(lin - (int64_t)which * gridDim.x);
    } else {
        // XCD-aware, bijective remap: blocks b, b+8, b+16.. share an XCD -> give each XCD a contiguous strip
        const int nwg = gridDim.x;
        const int orig = blockIdx.x;
        const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    // wg -> tile in ROW-BAND order: bands of 8 tile rows, inside a band column by column.  64 consecutive
    // workgroups (what one XCD runs at once: 32 CUs x 2) are then an 8x8 patch of tiles: per K-step they
    // pull 8 A + 8 B tiles through the XCD's L2 instead of 64 + 1 for a column strip.  In `lower` mode only
    // tiles with ti >= tj are enumerated (the last columns of a band are partial).  The band search is a
    // short wave-uniform loop (<= ntm/8 iterations of scalar arithmetic).
    int ti = 0, tj = 0;
    {
        int rem = wg;
        bool found = false;
        for (int R0 = 0; R0 < ntm; R0 += 8) {
            const int R1 = (R0 + 7 < ntm ? R0 + 7 : ntm - 1), nr = R1 - R0 + 1;
            const int cmax = lower ? (R1 < ntn - 1 ? R1 : ntn - 1) : ntn - 1;       // last column of this band
            const int cfull = lower ? (R0 < cmax ? R0 : cmax) : cmax;               // columns 0..cfull hold all nr rows
            const int tri = cmax - cfull;                                           // partial columns cfull+1..cmax
            const int count = nr * (cfull + 1) + tri * (R1 - cfull + 1) - tri * (tri + 1) / 2;   // + sum_{c} (R1 - c + 1)
            if (rem < count) {
                if (rem < nr * (cfull + 1)) {
                    tj = rem / nr;
                    ti = R0 + rem - tj * nr;
                } else {
                    rem -= nr * (cfull + 1);
                    int c = cfull + 1;
                    while (rem >= R1 - c + 1) { rem -= R1 - c + 1; ++c; }
                    tj = c;
                    ti = c + rem;
                }
                found = true;
                break;
            }
            rem -= count;
        }
        if (BATCH && !found) return;                        // this matrix has fewer tiles than the largest of the batch
    }
    (void)ntiles_total;
    const int t = threadIdx.x;
    const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const float* Ag = A + (int64_t)ti * NB * lda;
    const float* Bg = B + (int64_t)tj * NB * ldb;
    // LDS-DMA (global_load_lds_dwordx4): wave `wid` brings rows wid*32 + 8i .. +7 (i = 0..3) of each operand, one KiB
    // per instruction, straight into LDS -- no staging registers, no ds_write, and the wave only waits for its pieces
    // right before the barrier.  A DMA instruction fills LDS linearly (lane l -> 16 bytes at 16 l), so the image cannot
    // be padded; it is XOR-swizzled instead: lane l lands at physical chunk (l&7) of row (l>>3) and therefore fetches
    // the LOGICAL chunk (l&7) ^ (row&7) of that row from global memory (still one 128-byte segment per row).
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int rl = lane >> 3, lc = (lane & 7) ^ rl;
    const float* Ad = Ag + (int64_t)(wid * 32 + rl) * lda + 4 * lc;
    const float* Bd = Bg + (int64_t)(wid * 32 + rl) * ldb + 4 * lc;
#define OISAT_DMA(buf, k0)                                                                                         \
    do {                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                            \
            __builtin_amdgcn_global_load_lds((gptr_t)(Ad + (int64_t)(8 * i) * lda + (k0)),                         \
                                             (lptr_t)&lds[buf][0][(wid * 32 + 8 * i) * BK], 16, 0, 0);             \
            __builtin_amdgcn_global_load_lds((gptr_t)(Bd + (int64_t)(8 * i) * ldb + (k0)),                         \
                                             (lptr_t)&lds[buf][1][(wid * 32 + 8 * i) * BK], 16, 0, 0);             \
        }                                                                                                          \
    } while (0)
    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};

    const int nkt = K / BK;
    OISAT_DMA(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int frow = lane & 31, fh = lane >> 5;
    // a lane's fragment of K-group s is logical chunk 2s+fh of its row: physical chunk (2s+fh) ^ (row&7).  Any 8 consecutive
    // rows hold one logical chunk in 8 different physical chunks = all 32 banks once: conflict-free ds_read_b128.
    const int sw = frow & 7;
    const int arow = (wr * 64 + frow) * BK, brow = (wc * 64 + frow) * BK;
    // fragment registers, two sets: the operands of MFMA group s+1 are read from LDS while group s runs
    float4 fa0, fa1, fb0, fb1, ga0, ga1, gb0, gb1;
#define OISAT_FRAG(A0, A1, B0, B1, buf, s)                                                      \
    do {                                                                                        \
        A0 = *reinterpret_cast<const float4*>(&lds[buf][0][arow + 4 * ((2 * (s) + fh) ^ sw)]);            \
        A1 = *reinterpret_cast<const float4*>(&lds[buf][0][arow + 32 * BK + 4 * ((2 * (s) + fh) ^ sw)]);  \
        B0 = *reinterpret_cast<const float4*>(&lds[buf][1][brow + 4 * ((2 * (s) + fh) ^ sw)]);            \
        B1 = *reinterpret_cast<const float4*>(&lds[buf][1][brow + 32 * BK + 4 * ((2 * (s) + fh) ^ sw)]);  \
    } while (0)
#define OISAT_MFMA4(A0, A1, B0, B1, c)                                                          \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B0.c, acc00, 0, 0, 0);                   \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B1.c, acc01, 0, 0, 0);                   \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B0.c, acc10, 0, 0, 0);                   \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B1.c, acc11, 0, 0, 0);
#define OISAT_MFMA16(A0, A1, B0, B1)                                                            \
    OISAT_MFMA4(A0, A1, B0, B1, x) OISAT_MFMA4(A0, A1, B0, B1, y) OISAT_MFMA4(A0, A1, B0, B1, z) OISAT_MFMA4(A0, A1, B0, B1, w)
    OISAT_FRAG(fa0, fa1, fb0, fb1, 0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) OISAT_DMA(cur ^ 1, (kt + 1) * BK);            // the other buffer is free since the last barrier
        OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 1);
        OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 0
        OISAT_FRAG(fa0, fa1, fb0, fb1, cur, 2);
        OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 1
        OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 3);
        OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA pieces of tile kt+1 have landed ...
        __syncthreads();                                        // ... and so have everyone else's; every read of tile kt has been issued
        if (more) OISAT_FRAG(fa0, fa1, fb0, fb1, cur ^ 1, 0);   // first operands of the next tile, behind the last MFMA group
        OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 3
    }
    // epilogue: C/D layout col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
    float* Cg = C + ((int64_t)ti * NB + wr * 64) * ldc + (int64_t)tj * NB + wc * 64;
#define OISAT_EPI(ACC, i, j)                                                         \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                 \
        const int row = (i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;                  \
        float* p = Cg + (int64_t)row * ldc + (j) * 32 + frow;                        \
        if (mode == 0) *p = *p - ACC[e];                                             \
        else *p = ACC[e];                                                            \
    }
    OISAT_EPI(acc00, 0, 0)
    OISAT_EPI(acc01, 0, 1)
    OISAT_EPI(acc10, 1, 0)
    OISAT_EPI(acc11, 1, 1)
}
#undef OISAT_DMA
#undef OISAT_FRAG
#undef OISAT_MFMA4
#undef OISAT_MFMA16
#undef OISAT_EPI

// ---- gemm_nt ---------------------------------------------------------------------------------
// mode 0: C -= A*B^T      mode 1: C = A*B^T (C may alias A when N == K == 128: TRSM-as-GEMM)
// lower != 0: the C region is anchored on the diagonal; tiles strictly above it are skipped.
//
// PERSISTENT workgroups: the grid is min(tiles, 2 per CU) and workgroup b walks the tiles b, b + G, b + 2G, ...  A
// tile's fixed costs -- the first operand load in front of an idle MFMA pipe, the read-modify-write of C behind it --
// measured 22 us per tile (the time of six K-steps; 37 us per tile at K = 128, 81 us at K = 512 against 15 / 62 us of
// MFMA work), which is what the tall-and-thin updates deep in the recursion and every update of a 4,000-18,000-
// observation tile are made of.  Here the pipeline runs ACROSS tiles: the first K-step of the next tile is fetched (LDS-
// DMA into the free buffer) during the last K-step of the current one, and the C tile is prefetched into registers at
// the start of that last K-step, so the epilogue is 64 stores and the next tile's MFMAs start right behind it.
// Bit-identical to the one-tile-per-workgroup form (same accumulation order, C - sum rounded once).
template <bool BATCH>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(float* C0, int64_t ldc0, const float* A0, int64_t lda0,
                                                          const float* __restrict__ B0, int64_t ldb0, int ntm0, int ntn0, int K,
                                                          int mode, int lower, int ntiles_total, BatchArgs ba, int* dyn) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][NB * BK];        // [buf][A|B][row*32 + 4*(chunk ^ (row&7))] = 65,536 B
    // DYNAMIC tile walk (dyn != nullptr): a workgroup's first tile is its blockIdx, every further one a ticket drawn
    // from its XCD's counter (ids x, x + 8, x + 16, ... keep the XCD and the 64-id chunks of xcd_chunk_remap), other XCDs'
    // counters once its own is exhausted.  With the static walk b, b + G, ... a workgroup that starts late -- another
    // stream's kernel held its slot -- still has its whole share of tiles in front of it and the launch ends that much
    // later; with tickets the workgroups that did get a slot take the work.  dyn[0..7]: tickets per XCD, dyn[8]: workgroups
    // that have left; the last one to leave zeroes the block again (the next launch on the stream finds it clean).
    __shared__ int s_tkt[2];
    if (BATCH) group_prio(ba.prio);
    const int t = threadIdx.x;
    const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    // virtual tile ids: plain launch: the tiles of C;  batched launch: (ntm0 = tiles of the largest matrix) x (ntn0 = matrices)
    const bool compact = BATCH && ba.cum != nullptr;
    const int64_t VT = compact ? (int64_t)ba.total : (BATCH ? (int64_t)ntm0 * ntn0 : (int64_t)ntiles_total);
    int cw = 0;                                             // compact enumeration: member of the last id located (ids only grow)
    const int64_t G = gridDim.x;                            // a multiple of 8 whenever a workgroup gets more than one tile
    // LDS-DMA (global_load_lds_dwordx4): wave `wid` brings rows wid*32 + 8i .. +7 (i = 0..3) of each operand, one KiB
    // per instruction, straight into LDS -- no staging registers, no ds_write, and the wave only waits for its pieces
    // right before the barrier.  A DMA instruction fills LDS linearly (lane l -> 16 bytes at 16 l), so the image cannot
    // be padded; it is XOR-swizzled instead: lane l lands at physical chunk (l&7) of row (l>>3) and therefore fetches
    // the LOGICAL chunk (l&7) ^ (row&7) of that row from global memory (still one 128-byte segment per row).
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int rl = lane >> 3, lc = (lane & 7) ^ rl;
    const int frow = lane & 31, fh = lane >> 5;

    // virtual id -> tile.  Workgroups go to the 8 XCDs round-robin in dispatch order, and v = b + iG keeps b's XCD (G is
    // a multiple of 512 / 8): xcd_chunk_remap hands each XCD (private 4 MiB L2) 64 consecutive ids at a time, which the
    // row-band order below turns into 8x8 patches of tiles that share operand panels (in a batched launch: neighbouring
    // tiles of the same matrix).
    // Row-band order: bands of 8 tile rows, inside a band column by column; in `lower` mode only tiles with ti >= tj
    // are enumerated (the last columns of a band are partial).  The band search is a short wave-uniform loop.
    const bool dynamic = dyn != nullptr && G < VT;         // (host: G is a multiple of 8 then, and every id is a real tile)
    const int xcd = (int)(blockIdx.x & 7);
    const int64_t G8 = G >> 3;
    auto leave = [&]() {                                    // thread 0, once per workgroup
        if (dyn != nullptr && t == 0) {
            const int gone = __hip_atomic_fetch_add(&dyn[8], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gone == (int)G - 1) {
#pragma unroll
                for (int x = 0; x < 9; ++x) __hip_atomic_store(&dyn[x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    auto ticket_to_id = [&](int x, int tk) -> int64_t { return (int64_t)x + 8 * (G8 + (int64_t)tk); };
    auto steal = [&]() -> int {                             // thread 0: own counter exhausted, try the other XCDs' (end of launch only)
        for (int k = 1; k < 8; ++k) {
            const int x = (xcd + k) & 7;
            const int tk = __hip_atomic_fetch_add(&dyn[x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t vv = ticket_to_id(x, tk);
            if (vv < VT) return (int)vv;
        }
        return (int)VT;
    };
    auto locate = [&](int64_t v, const float*& oAd, const float*& oBd, float*& oCg, int64_t& olda, int64_t& oldb,
                      int64_t& oldc) -> int64_t {
        for (; v < VT; v += (dynamic ? VT : G)) {
            const int64_t lin = xcd_chunk_remap(v, VT);
            float* C = C0;
            const float* A = A0;
            const float* B = B0;
            int64_t lda = lda0, ldb = ldb0, ldc = ldc0;
            int ntm = ntm0, ntn = ntn0, wg = (int)lin;
            if (BATCH) {
                int which;
                if (compact) {                              // ids of a workgroup (almost) only grow: gallop forward from the last
                    int lo = cw, step = 1;                  // member, then bisect (wave-uniform: scalar loads); a ticket stolen
                    if ((int)lin < ba.cum[lo]) lo = 0;      // from another XCD's counter may lie behind it
                    while (lo + step < ba.cnt && ba.cum[lo + step] <= (int)lin) { lo += step; step <<= 1; }
                    int hi = lo + step < ba.cnt ? lo + step : ba.cnt;
                    while (hi - lo > 1) {
                        const int md = (lo + hi) >> 1;
                        if (ba.cum[md] <= (int)lin) lo = md; else hi = md;
                    }
                    cw = which = lo;
                    wg = (int)lin - ba.cum[lo];
                } else {
                    which = (int)(lin / ntm0);
                    wg = (int)(lin - (int64_t)which * ntm0);
                }
                if (!batch_operands(ba, which, NB, C, ldc, A, lda, B, ldb, ntm, ntn)) continue;
            }
            int ti = 0, tj = 0, rem = wg;
            bool found = false;
            for (int R0 = 0; R0 < ntm; R0 += 8) {
                const int R1 = (R0 + 7 < ntm ? R0 + 7 : ntm - 1), nr = R1 - R0 + 1;
                const int cmax = lower ? (R1 < ntn - 1 ? R1 : ntn - 1) : ntn - 1;       // last column of this band
                const int cfull = lower ? (R0 < cmax ? R0 : cmax) : cmax;               // columns 0..cfull hold all nr rows
                const int tri = cmax - cfull;                                           // partial columns cfull+1..cmax
                const int count = nr * (cfull + 1) + tri * (R1 - cfull + 1) - tri * (tri + 1) / 2;   // + sum_{c} (R1 - c + 1)
                if (rem < count) {
                    if (rem < nr * (cfull + 1)) {
                        tj = rem / nr;
                        ti = R0 + rem - tj * nr;
                    } else {
                        rem -= nr * (cfull + 1);
                        int c = cfull + 1;
                        while (rem >= R1 - c + 1) { rem -= R1 - c + 1; ++c; }
                        tj = c;
                        ti = c + rem;
                    }
                    found = true;
                    break;
                }
                rem -= count;
            }
            if (!found) continue;                           // batched: this matrix has fewer tiles than the largest one
            oAd = A + ((int64_t)ti * NB + wid * 32 + rl) * lda + 4 * lc;
            oBd = B + ((int64_t)tj * NB + wid * 32 + rl) * ldb + 4 * lc;
            oCg = C + ((int64_t)ti * NB + wr * 64) * ldc + (int64_t)tj * NB + wc * 64;
            olda = lda;
            oldb = ldb;
            oldc = ldc;
            return v;
        }
        return -1;
    };
#define OISAT_DMA(buf, PA, PB, LA, LB, k0)                                                                         \
    do {                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                            \
            __builtin_amdgcn_global_load_lds((gptr_t)((PA) + (int64_t)(8 * i) * (LA) + (k0)),                      \
                                             (lptr_t)&lds[buf][0][(wid * 32 + 8 * i) * BK], 16, 0, 0);             \
            __builtin_amdgcn_global_load_lds((gptr_t)((PB) + (int64_t)(8 * i) * (LB) + (k0)),                      \
                                             (lptr_t)&lds[buf][1][(wid * 32 + 8 * i) * BK], 16, 0, 0);             \
        }                                                                                                          \
    } while (0)
    const float *Ad = nullptr, *Bd = nullptr, *nAd = nullptr, *nBd = nullptr;
    float *Cg = nullptr, *nCg = nullptr;
    int64_t lda = 0, ldb = 0, ldc = 0, nlda = 0, nldb = 0, nldc = 0;
    int64_t v = locate(blockIdx.x, Ad, Bd, Cg, lda, ldb, ldc);
    if (v < 0) {
        leave();
        return;
    }
    if (dynamic && t == 0) {                                // ticket of this workgroup's SECOND tile
        const int tk = __hip_atomic_fetch_add(&dyn[xcd], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int64_t vv = ticket_to_id(xcd, tk);
        s_tkt[0] = vv < VT ? (int)vv : steal();
    }

    const int nkt = K / BK;
    OISAT_DMA(0, Ad, Bd, lda, ldb, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // a lane's fragment of K-group s is logical chunk 2s+fh of its row: physical chunk (2s+fh) ^ (row&7).  Any 8 consecutive
    // rows hold one logical chunk in 8 different physical chunks = all 32 banks once: conflict-free ds_read_b128.
    const int sw = frow & 7;
    const int arow = (wr * 64 + frow) * BK, brow = (wc * 64 + frow) * BK;
    // fragment registers, two sets: the operands of MFMA group s+1 are read from LDS while group s runs
    float4 fa0, fa1, fb0, fb1, ga0, ga1, gb0, gb1;
#define OISAT_FRAG(A0, A1, B0, B1, buf, s)                                                      \
    do {                                                                                        \
        A0 = *reinterpret_cast<const float4*>(&lds[buf][0][arow + 4 * ((2 * (s) + fh) ^ sw)]);            \
        A1 = *reinterpret_cast<const float4*>(&lds[buf][0][arow + 32 * BK + 4 * ((2 * (s) + fh) ^ sw)]);  \
        B0 = *reinterpret_cast<const float4*>(&lds[buf][1][brow + 4 * ((2 * (s) + fh) ^ sw)]);            \
        B1 = *reinterpret_cast<const float4*>(&lds[buf][1][brow + 32 * BK + 4 * ((2 * (s) + fh) ^ sw)]);  \
    } while (0)
#define OISAT_MFMA4(A0, A1, B0, B1, c)                                                          \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B0.c, acc00, 0, 0, 0);                   \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B1.c, acc01, 0, 0, 0);                   \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B0.c, acc10, 0, 0, 0);                   \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B1.c, acc11, 0, 0, 0);
#define OISAT_MFMA16(A0, A1, B0, B1)                                                            \
    OISAT_MFMA4(A0, A1, B0, B1, x) OISAT_MFMA4(A0, A1, B0, B1, y) OISAT_MFMA4(A0, A1, B0, B1, z) OISAT_MFMA4(A0, A1, B0, B1, w)
    // C/D layout: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5).  The 64 elements a lane owns are addressed through
    // a buffer descriptor on the wave's 64x64 quadrant: ONE per-lane offset register (row 4*fh, column frow) and a
    // wave-uniform scalar offset per element -- 64 separate 64-bit addresses would not fit next to 64 prefetched values.
#define OISAT_CRSRC()                                                                                   \
    __builtin_amdgcn_make_buffer_rsrc((void*)Cg, (short)0, (int)(64 * ldc * 4), 0x00020000)
#define OISAT_CSOFF(i, j, e) (int)((((i) * 32 + ((e) & 3) + 8 * ((e) >> 2)) * ldc + (j) * 32) * 4)
#define OISAT_CPRE(DST, i, j)                                                                           \
    _Pragma("unroll") for (int e = 0; e < 16; ++e)                                                      \
        DST[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(crs, cvoff, OISAT_CSOFF(i, j, e), 0));
#define OISAT_EPI(ACC, PRE, i, j)                                                                       \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                    \
        const float o = (mode == 0) ? PRE[e] - ACC[e] : ACC[e];                                         \
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), crs, cvoff, OISAT_CSOFF(i, j, e), 0); \
    }
    int base = 0;                                           // LDS buffer that holds K-step 0 of the current tile
    int nth = 0;                                            // tiles this workgroup has started
    OISAT_FRAG(fa0, fa1, fb0, fb1, 0, 0);
    while (true) {
        // next tile: static v + G, or the ticket parked in LDS one tile ago (barriers in between); thread 0 then draws the
        // ticket of the tile after that -- the atomic's round trip hides behind this tile's K-loop, its value is parked
        // right before the tile's last barrier
        const int64_t nvid = dynamic ? (int64_t)s_tkt[nth & 1] : v + G;
        int pend = 0;
        if (dynamic && t == 0 && nvid < VT)
            pend = __hip_atomic_fetch_add(&dyn[xcd], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int64_t nv = nvid < VT ? locate(nvid, nAd, nBd, nCg, nlda, nldb, nldc) : -1;
        const bool has_next = nv >= 0;
        f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
        f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
        const __amdgpu_buffer_rsrc_t crs = OISAT_CRSRC();
        const int cvoff = (int)(((4 * fh) * ldc + frow) * 4);
        // steady state: the loop of the one-tile kernel, branch-free (one scheduling region)
        for (int kt = 0; kt + 1 < nkt; ++kt) {
            const int cur = (kt + base) & 1;
            OISAT_DMA(cur ^ 1, Ad, Bd, lda, ldb, (kt + 1) * BK);   // the other buffer is free since the last barrier
            OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 1);
            OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 0
            OISAT_FRAG(fa0, fa1, fb0, fb1, cur, 2);
            OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 1
            OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 3);
            OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 2
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA pieces of K-step kt+1 have landed ...
            __syncthreads();                                        // ... and so have everyone else's; every read of K-step kt has been issued
            OISAT_FRAG(fa0, fa1, fb0, fb1, cur ^ 1, 0);             // first operands of the next K-step, behind the last MFMA group
            OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 3
        }
        {   // last K-step of this tile: K-step 0 of the NEXT tile goes to the free buffer, the C tile to registers
            const int cur = (nkt - 1 + base) & 1;
            if (has_next) OISAT_DMA(cur ^ 1, nAd, nBd, nlda, nldb, 0);
            if (mode == 0) {
                OISAT_CPRE(c00, 0, 0)
                OISAT_CPRE(c01, 0, 1)
                OISAT_CPRE(c10, 1, 0)
                OISAT_CPRE(c11, 1, 1)
            }
            OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 1);
            OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 0
            OISAT_FRAG(fa0, fa1, fb0, fb1, cur, 2);
            OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 1
            OISAT_FRAG(ga0, ga1, gb0, gb1, cur, 3);
            OISAT_MFMA16(fa0, fa1, fb0, fb1)                       // s = 2
            if (dynamic && t == 0) {
                int64_t vv = VT;
                if (nvid < VT) {
                    vv = ticket_to_id(xcd, pend);
                    if (vv >= VT) vv = steal();
                }
                s_tkt[(nth + 1) & 1] = (int)vv;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (has_next) OISAT_FRAG(fa0, fa1, fb0, fb1, cur ^ 1, 0);
            OISAT_MFMA16(ga0, ga1, gb0, gb1)                       // s = 3
        }
        OISAT_EPI(acc00, c00, 0, 0)
        OISAT_EPI(acc01, c01, 0, 1)
        OISAT_EPI(acc10, c10, 1, 0)
        OISAT_EPI(acc11, c11, 1, 1)
        if (!has_next) break;
        base = (base + nkt) & 1;
        ++nth;
        v = nv;
        Ad = nAd; Bd = nBd; Cg = nCg;
        lda = nlda; ldb = nldb; ldc = nldc;
    }
    leave();
}

// ---- gemm_nt for launches that cannot fill the chip with 128x128 tiles ------------------------------
// Deep in the recursion the updates are tall and thin (e.g. 71 x 2 blocks, K = 3 blocks): 141 tiles of 128x128 on
// 512 workgroup slots, every workgroup alone on its CU for 12 K-tiles of ~2.3 us plus load/epilogue latency.  The
// same launch cut into 64x64 tiles is 564 workgroups of a quarter of the work each, four per CU: ~2x faster.
// 4 waves as 2x2, one 32x32 MFMA tile per wave, BK = 32, same LDS image rows (36-float stride), same k permutation
// and per-element accumulation order as gemm_nt_kernel (bit-identical results).
// NBUF: LDS images per operand.  2 = double-buffered (36,864 B).  1 = single image, one more barrier per K-step (18,432 B):
// the batched instantiation -- its launches are the dependent chain of one group of systems while ANOTHER group's
// 128x128 GEMMs hold two 64-KB workgroups on every CU, which leaves 32 KB of the 160: a 36-KB workgroup then waits for
// one of them to retire (hundreds of microseconds with the persistent kernel), an 18-KB one moves in next to them.
template <bool BATCH, int NBUF>
__global__ __launch_bounds__(256) void gemm_nt_small_kernel(float* C, int64_t ldc, const float* A, int64_t lda,
                                                             const float* __restrict__ B, int64_t ldb, int ntm, int ntn, int K,
                                                             int mode, int lower, BatchArgs ba) {
    __shared__ __attribute__((aligned(16))) float lds[NBUF][2][SB * LDSW];    // 36,864 B / 18,432 B
    if (BATCH) group_prio(ba.prio);
    if (BATCH) {
        const float* Bb = nullptr;
        if (!batch_operands(ba, blockIdx.y, SB, C, ldc, A, lda, Bb, ldb, ntm, ntn)) return;
        B = Bb;
    }
    // tile decode: column-major; in `lower` mode column c holds rows c .. ntm-1 (units of 64)
    int ti, tj;
    {
        int rem = blockIdx.x;
        if (!lower) {
            tj = rem / ntm;
            ti = rem - tj * ntm;
            if (BATCH && tj >= ntn) return;
        } else {
            int c = 0;
            while (c < ntn && rem >= ntm - c) { rem -= ntm - c; ++c; }
            if (BATCH && c >= ntn) return;
            tj = c;
            ti = c + rem;
        }
    }
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const float* Ag = A + (int64_t)ti * SB * lda;
    const float* Bg = B + (int64_t)tj * SB * ldb;
    const int srow = t >> 3, sk = (t & 7) * 4;           // rows srow and srow+32, 16 bytes at k = sk
    const float* Ap = Ag + (int64_t)srow * lda + sk;
    const float* Bp = Bg + (int64_t)srow * ldb + sk;
    float4 ra0, ra1, rb0, rb1;
#define OISAT_SGLOAD(k0)                                                             \
    do {                                                                             \
        ra0 = *reinterpret_cast<const float4*>(Ap + (k0));                           \
        ra1 = *reinterpret_cast<const float4*>(Ap + 32 * lda + (k0));                \
        rb0 = *reinterpret_cast<const float4*>(Bp + (k0));                           \
        rb1 = *reinterpret_cast<const float4*>(Bp + 32 * ldb + (k0));                \
    } while (0)
#define OISAT_SLSTORE(buf)                                                           \
    do {                                                                             \
        *reinterpret_cast<float4*>(&lds[buf][0][srow * LDSW + sk]) = ra0;            \
        *reinterpret_cast<float4*>(&lds[buf][0][(srow + 32) * LDSW + sk]) = ra1;     \
        *reinterpret_cast<float4*>(&lds[buf][1][srow * LDSW + sk]) = rb0;            \
        *reinterpret_cast<float4*>(&lds[buf][1][(srow + 32) * LDSW + sk]) = rb1;     \
    } while (0)
    f32x16 acc = {0};
    const int nkt = K / BK;
    OISAT_SGLOAD(0);
    OISAT_SLSTORE(0);
    __syncthreads();
    const int frow = lane & 31, fh = lane >> 5;
    const int aoff = (wr * 32 + frow) * LDSW + 4 * fh, boff = (wc * 32 + frow) * LDSW + 4 * fh;
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = NBUF == 2 ? (kt & 1) : 0;
        const bool more = kt + 1 < nkt;
        if (more) OISAT_SGLOAD((kt + 1) * BK);
        float4 fa[4], fb[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            fa[s4] = *reinterpret_cast<const float4*>(&lds[cur][0][aoff + 8 * s4]);
            fb[s4] = *reinterpret_cast<const float4*>(&lds[cur][1][boff + 8 * s4]);
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s4].x, fb[s4].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s4].y, fb[s4].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s4].z, fb[s4].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s4].w, fb[s4].w, acc, 0, 0, 0);
        }
        if (NBUF == 1 && more) __syncthreads();                  // every wave has read this image
        if (more) OISAT_SLSTORE(NBUF == 2 ? (cur ^ 1) : 0);
        __syncthreads();
    }
    float* Cg = C + ((int64_t)ti * SB + wr * 32) * ldc + (int64_t)tj * SB + wc * 32;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * fh;
        float* p = Cg + (int64_t)row * ldc + frow;
        if (mode == 0) *p = *p - acc[e];
        else *p = acc[e];
    }
}

// The in-place TRSM-as-GEMM (C aliases A, N == K == 128) cannot use 64-wide tiles: a tile would overwrite panel columns
// its row neighbour still reads.  64 rows x all 128 columns per workgroup instead (each wave 32 x 64 = two MFMA tiles):
// a workgroup owns whole rows and has read every K-tile of them before its epilogue writes.
template <bool BATCH, int NBUF>
__global__ __launch_bounds__(256) void gemm_nt_rows64_kernel(float* C, int64_t ldc, const float* A, int64_t lda,
                                                              const float* __restrict__ B, int64_t ldb, int K, int mode, BatchArgs ba) {
    __shared__ __attribute__((aligned(16))) float ldsA[NBUF][SB * LDSW];     // 18,432 B / 9,216 B
    __shared__ __attribute__((aligned(16))) float ldsB[NBUF][NB * LDSW];     // 36,864 B / 18,432 B  (NBUF = 1: 27,648 B in all)
    if (BATCH) group_prio(ba.prio);
    if (BATCH) {
        int ntm, ntn;
        const float* Bb = nullptr;
        if (!batch_operands(ba, blockIdx.y, SB, C, ldc, A, lda, Bb, ldb, ntm, ntn) || (int)blockIdx.x >= ntm) return;
        B = Bb;
    }
    const int ti = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int srow = t >> 3, sk = (t & 7) * 4;
    const float* Ap = A + ((int64_t)ti * SB + srow) * lda + sk;
    const float* Bp = B + (int64_t)srow * ldb + sk;
    float4 ra0, ra1, rb0, rb1, rb2, rb3;
#define OISAT_RGLOAD(k0)                                                             \
    do {                                                                             \
        ra0 = *reinterpret_cast<const float4*>(Ap + (k0));                           \
        ra1 = *reinterpret_cast<const float4*>(Ap + 32 * lda + (k0));                \
        rb0 = *reinterpret_cast<const float4*>(Bp + (k0));                           \
        rb1 = *reinterpret_cast<const float4*>(Bp + 32 * ldb + (k0));                \
        rb2 = *reinterpret_cast<const float4*>(Bp + 64 * ldb + (k0));                \
        rb3 = *reinterpret_cast<const float4*>(Bp + 96 * ldb + (k0));                \
    } while (0)
#define OISAT_RLSTORE(buf)                                                           \
    do {                                                                             \
        *reinterpret_cast<float4*>(&ldsA[buf][srow * LDSW + sk]) = ra0;              \
        *reinterpret_cast<float4*>(&ldsA[buf][(srow + 32) * LDSW + sk]) = ra1;       \
        *reinterpret_cast<float4*>(&ldsB[buf][srow * LDSW + sk]) = rb0;              \
        *reinterpret_cast<float4*>(&ldsB[buf][(srow + 32) * LDSW + sk]) = rb1;       \
        *reinterpret_cast<float4*>(&ldsB[buf][(srow + 64) * LDSW + sk]) = rb2;       \
        *reinterpret_cast<float4*>(&ldsB[buf][(srow + 96) * LDSW + sk]) = rb3;       \
    } while (0)
    f32x16 acc0 = {0}, acc1 = {0};
    const int nkt = K / BK;
    OISAT_RGLOAD(0);
    OISAT_RLSTORE(0);
    __syncthreads();
    const int frow = lane & 31, fh = lane >> 5;
    const int aoff = (wr * 32 + frow) * LDSW + 4 * fh, boff = (wc * 64 + frow) * LDSW + 4 * fh;
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = NBUF == 2 ? (kt & 1) : 0;
        const bool more = kt + 1 < nkt;
        if (more) OISAT_RGLOAD((kt + 1) * BK);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const float4 a = *reinterpret_cast<const float4*>(&ldsA[cur][aoff + 8 * s4]);
            const float4 b0 = *reinterpret_cast<const float4*>(&ldsB[cur][boff + 8 * s4]);
            const float4 b1 = *reinterpret_cast<const float4*>(&ldsB[cur][boff + 32 * LDSW + 8 * s4]);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
        }
        if (NBUF == 1 && more) __syncthreads();
        if (more) OISAT_RLSTORE(NBUF == 2 ? (cur ^ 1) : 0);
        __syncthreads();
    }
    float* Cg = C + ((int64_t)ti * SB + wr * 32) * ldc + wc * 64;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * fh;
        float* p = Cg + (int64_t)row * ldc + frow;
        if (mode == 0) { p[0] = p[0] - acc0[e]; p[32] = p[32] - acc1[e]; }
        else { p[0] = acc0[e]; p[32] = acc1[e]; }
    }
}

static const int kBigK = 2048;                           // K from which gemm_nt_big_kernel is used (below it the persistent kernel with the C prefetch wins)

// grid of the persistent gemm_nt_kernel: every tile its own workgroup while they all fit (2 per CU), else 2 per CU
// (a multiple of 8, so that workgroup b keeps its XCD for all of its tiles)
static inline unsigned persistent_grid(const oisat_ctx* h, int64_t virtual_tiles) {
    const int per_cu = h->gemm_wg_per_cu > 0 ? h->gemm_wg_per_cu : 2;
    const int64_t slots = ((int64_t)(h->cu_count > 0 ? h->cu_count : 256) * per_cu) / 8 * 8;
    return (unsigned)(virtual_tiles <= slots || per_cu <= 0 ? virtual_tiles : slots);
}

// ticket block of the dynamic tile walk (gemm_nt_kernel): 9 ints per stream of the handle (main | look-ahead aux), zero
// when a launch starts -- zeroed here when first allocated, by the last workgroup of every launch from then on
static int* dyn_tickets(oisat_ctx* h) {
    const bool fresh = h->ws[8] == nullptr;
    char* base = (char*)oisat_ws(h, 8, 256);
    if (!base) return nullptr;
    if (fresh && hipMemsetAsync(base, 0, 256, h->stream) != hipSuccess) return nullptr;
    return (int*)(base + (h->aux_stream != nullptr && h->stream == h->aux_stream ? 128 : 0));
}

static inline int64_t tiles_lower(int64_t ntm, int64_t ntn) { return ntn * ntm - ntn * (ntn - 1) / 2; }

// node key of the compact-enumeration tables: kind 0 (b0, mid, b1) / kind 1 (b0)
static inline long long cum_key_of(int kind, int b0, int mid, int b1) {
    return ((long long)kind << 60) | ((long long)b0 << 40) | ((long long)mid << 20) | (long long)b1;
}

static inline void attach_cum(const ChBatch& bt, BatchArgs& ba) {
    if (!bt.cum_dev) return;
    const long long key = cum_key_of(ba.kind, ba.b0, ba.kind == 0 ? ba.mid : 0, ba.kind == 0 ? ba.b1 : 0);
    auto it = std::lower_bound(bt.cum_key.begin(), bt.cum_key.end(), key);
    if (it == bt.cum_key.end() || *it != key) return;
    const size_t s = it - bt.cum_key.begin();
    ba.cum = bt.cum_dev + bt.cum_off[s];
    ba.cnt = bt.cum_cnt[s];
    ba.total = bt.cum_total[s];
}

}  // namespace

namespace oisat_dense {

int launch_gemm(oisat_ctx* h, const char* name, float* C, int64_t ldc, const float* A, int64_t lda, const float* B, int64_t ldb,
                int64_t M, int64_t N, int K, int mode, int lower) {
    const int ntm = (int)(M / NB), ntn = (int)(N / NB);
    const int64_t ntiles = lower ? (int64_t)ntn * ntm - (int64_t)ntn * (ntn - 1) / 2 : (int64_t)ntm * ntn;
    if (ntiles <= 0) return OISAT_OK;
    char dname[64];
    if (prof_detail() && h->prof) {                         // profiling aid: one record per launch shape
        snprintf(dname, sizeof(dname), "%s K%d t%lld n1", name, K, (long long)ntiles);
        name = dname;
    }
    // too few 128x128 tiles for the 512 workgroup slots: 64x64 tiles, four workgroups per CU; the in-place TRSM form
    // (C aliases A, N == K == 128) takes 64 x 128 tiles (gemm_nt_rows64_kernel).
    constexpr int small_max = 700;
    if (ntiles <= small_max && h->small_tiles && C != A) {
        const int sm = (int)(M / SB), sn = (int)(N / SB);
        const int64_t st = lower ? (int64_t)sn * sm - (int64_t)sn * (sn - 1) / 2 : (int64_t)sm * sn;
        OISAT_LAUNCH(h, name, (gemm_nt_small_kernel<false, 2>), dim3((unsigned)st), dim3(256), 0, C, ldc, A, lda, B, ldb, sm, sn, K, mode, lower,
                     BatchArgs{});
        return OISAT_OK;
    }
    if (ntiles <= small_max && h->small_tiles && C == A && N == NB && !lower) {     // in-place TRSM-as-GEMM
        OISAT_LAUNCH(h, name, (gemm_nt_rows64_kernel<false, 2>), dim3((unsigned)(M / SB)), dim3(256), 0, C, ldc, A, lda, B, ldb, K, mode,
                     BatchArgs{});
        return OISAT_OK;
    }
    if (ntiles >= (int64_t)INT32_MAX) {
        oisat_set_error("gemm grid too large");
        return OISAT_EINVAL;
    }
    if (K >= kBigK) {
        OISAT_LAUNCH(h, name, gemm_nt_big_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, C, ldc, A, lda, B, ldb, ntm, ntn, K, mode,
                     lower, (int)ntiles, BatchArgs{});
        return OISAT_OK;
    }
    OISAT_LAUNCH(h, name, gemm_nt_kernel<false>, dim3(persistent_grid(h, ntiles)), dim3(256), 0, C, ldc, A, lda, B, ldb, ntm, ntn, K, mode,
                 lower, (int)ntiles, BatchArgs{}, dyn_tickets(h));
    return OISAT_OK;
}

// prefix sums of the members' 128x128 tile counts for every node of the recursion tree (the tree of potrf_rec_batched)
void build_cum_tables(ChBatch* bt, std::vector<int>& host) {
    std::vector<std::pair<long long, int>> keys;            // (key, slot)
    auto add = [&](int kind, int b0, int mid, int b1) {
        const int off = (int)host.size();
        int acc = 0, cnt = 0;
        host.push_back(0);
        for (const BatchMat& m : bt->table) {
            int64_t rows, cols;
            if (kind == 0) { rows = m.mpb - mid; cols = (b1 < m.mpb ? b1 : m.mpb) - mid; }
            else { rows = m.mpb - b0 - 1; cols = 1; }
            if (rows <= 0 || cols <= 0) break;
            acc += (int)(kind == 0 ? cols * rows - cols * (cols - 1) / 2 : rows);
            host.push_back(acc);
            ++cnt;
        }
        if (cnt == 0) { host.resize(off); return; }
        keys.emplace_back(cum_key_of(kind, b0, mid, b1), (int)bt->cum_off.size());
        bt->cum_off.push_back(off);
        bt->cum_cnt.push_back(cnt);
        bt->cum_total.push_back(acc);
    };
    struct Rec {
        static void go(int b0, int b1, const decltype(add)& add, bool pairs) {
            if (b1 - b0 == 1) { add(1, b0, 0, 0); return; }
            if (b1 - b0 == 2 && pairs) return;                  // a leaf pair: its kernels enumerate their own workgroups
            const int mid = (int)split_mid(b0, b1, pairs);
            go(b0, mid, add, pairs);
            add(0, b0, mid, b1);
            go(mid, b1, add, pairs);
        }
    };
    Rec::go(0, bt->max_mpb, add, bt->pairs);
    std::sort(keys.begin(), keys.end());
    std::vector<int> off, cnt, tot;
    for (auto& kv : keys) {
        bt->cum_key.push_back(kv.first);
        off.push_back(bt->cum_off[kv.second]); cnt.push_back(bt->cum_cnt[kv.second]); tot.push_back(bt->cum_total[kv.second]);
    }
    bt->cum_off = off; bt->cum_cnt = cnt; bt->cum_total = tot;
}

int launch_gemm_batched(oisat_ctx* h, const char* name, const ChBatch& bt, BatchArgs ba, int K, int mode, int lower) {
    ba.prio = h->wave_prio;
    // participants and tile counts (units of 128) from the host copy of the table
    int cnt = 0;
    int64_t sum = 0, mx = 0;
    for (const BatchMat& m : bt.table) {
        int64_t rows, cols;
        if (ba.kind == 0) { rows = m.mpb - ba.mid; cols = (ba.b1 < m.mpb ? ba.b1 : m.mpb) - ba.mid; }
        else { rows = m.mpb - ba.b0 - 1; cols = 1; }
        if (rows <= 0 || cols <= 0) break;                  // sorted: nobody further down reaches this node either
        const int64_t t = lower ? tiles_lower(rows, cols) : rows * cols;
        sum += t;
        if (t > mx) mx = t;
        ++cnt;
    }
    if (cnt == 0) return OISAT_OK;
    constexpr int small_max = 700;
    // OISAT_PROF_DETAIL=1 (profiling aid): one profile record per launch shape -- "name K tiles members" -- instead of per name
    char dname[64];
    if (prof_detail() && h->prof) {
        snprintf(dname, sizeof(dname), "%s K%d t%lld n%d", name, K, (long long)sum, cnt);
        name = dname;
    }
    const BatchMat& big = bt.table[0];
    if (ba.kind == 1) {                                     // in-place TRSM: whole rows per workgroup
        const int64_t rows = big.mpb - ba.b0 - 1;
        if (sum <= small_max) {
            OISAT_LAUNCH(h, name, (gemm_nt_rows64_kernel<true, 1>), dim3((unsigned)(rows * 2), (unsigned)cnt), dim3(256), 0, (float*)nullptr,
                         (int64_t)0, (const float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, K, mode, ba);
        } else {
            attach_cum(bt, ba);
            OISAT_LAUNCH(h, name, gemm_nt_kernel<true>, dim3(persistent_grid(h, ba.cum ? ba.total : rows * cnt)), dim3(256), 0,
                         (float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, (int)rows, cnt, K,
                         mode, 0, 0, ba, ba.cum ? dyn_tickets(h) : nullptr);       // tickets only over the compact ids (all real tiles)
        }
        return OISAT_OK;
    }
    const int64_t rows = big.mpb - ba.mid, cols = (ba.b1 < big.mpb ? ba.b1 : big.mpb) - ba.mid;
    if (sum <= small_max) {
        const int64_t st = lower ? tiles_lower(rows * 2, cols * 2) : rows * cols * 4;
        OISAT_LAUNCH(h, name, (gemm_nt_small_kernel<true, 1>), dim3((unsigned)st, (unsigned)cnt), dim3(256), 0, (float*)nullptr, (int64_t)0,
                     (const float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, 0, 0, K, mode, lower, ba);
    } else if (K >= kBigK) {
        OISAT_LAUNCH(h, name, gemm_nt_big_kernel<true>, dim3((unsigned)mx, (unsigned)cnt), dim3(256), 0, (float*)nullptr, (int64_t)0,
                     (const float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, 0, 0, K, mode, lower, 0, ba);
    } else {
        if (lower) attach_cum(bt, ba);                          // (the tables hold the lower-triangle tile counts)
        OISAT_LAUNCH(h, name, gemm_nt_kernel<true>, dim3(persistent_grid(h, ba.cum ? ba.total : mx * cnt)), dim3(256), 0, (float*)nullptr,
                     (int64_t)0, (const float*)nullptr, (int64_t)0, (const float*)nullptr, (int64_t)0, (int)mx, cnt, K, mode, lower, 0, ba,
                     ba.cum ? dyn_tickets(h) : nullptr);
    }
    return OISAT_OK;
}

}  // namespace oisat_dense

extern "C" int oisat_set_share(oisat_ctx* h, int wave_prio, int gemm_wg_per_cu) {
    ARG_CHECK(h != nullptr && wave_prio >= 0 && wave_prio <= 3 && gemm_wg_per_cu >= 0 && gemm_wg_per_cu <= 2);
    h->wave_prio = wave_prio;
    h->gemm_wg_per_cu = gemm_wg_per_cu;
    return OISAT_OK;
}

extern "C" int oisat_gemm_nt(oisat_ctx* h, float* C, int64_t ldc, const float* A, int64_t lda, const float* B, int64_t ldb,
                             int64_t M, int64_t N, int64_t K, int mode, int lower) {
    ARG_CHECK(h && C && A && B && M > 0 && N > 0 && K > 0);
    ARG_CHECK(M % NB == 0 && N % NB == 0 && K % BK == 0 && K < (int64_t)INT32_MAX);
    ARG_CHECK(ldc % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldc >= N && lda >= K && ldb >= K);
    ARG_CHECK(((uintptr_t)C % 16) == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0);
    ARG_CHECK((mode == 0 || mode == 1) && (!lower || M >= N));
    return launch_gemm(h, "gemm_nt", C, ldc, A, lda, B, ldb, M, N, (int)K, mode, lower);
}
