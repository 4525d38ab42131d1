// Kalman-gain solve: in-place blocked Cholesky of S = H B H^T + R (fp32, lower) on the MI355X
// matrix cores, plus the triangular solves and the double-residual refinement around it.
// (North-star extension; the reference's `(Sa*reg+So)**(-1)` is element-wise,
//  optimal_interpolation.py:27.)
//
// Data layout in HBM: S is row-major float, leading dimension ld >= mp = roundup(m,128); rows
// m..mp are identity padding so no kernel needs a bounds check.  L overwrites the lower triangle.
//
// Algorithm: recursive (cache-oblivious) blocked Cholesky.  All O(m^3) work is in ONE kernel,
//     gemm_nt:  C[MxN] (-)= A[MxK] * B[NxK]^T      (both operands K-contiguous, "NT")
// built on v_mfma_f32_32x32x2_f32 (exact fp32, 256 flop/clk/CU = 157 TFLOP/s peak):
//   * 128x128 block tile, 4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles (64 accumulator VGPRs)
//   * K in steps of 32 through a double-buffered LDS image [128][32] floats per operand, filled by LDS-DMA
//     (global_load_lds_dwordx4: no staging registers, no ds_write) and XOR-swizzled at 16-byte granularity --
//     chunk c of row r lives at chunk c ^ (r & 7) -- so that every ds_read_b128 fragment read is conflict-free
//     without padding (a DMA instruction fills LDS linearly, padding is not expressible)
//   * a lane reads k = 8s+4h..+3 as one ds_read_b128 and feeds 4 consecutive MFMAs; A and B use
//     the same k permutation, so the product is unchanged
//   * software pipeline, skewed across the barrier: the fragments of MFMA group s+1 are read from
//     LDS while group s runs (two fragment register sets); the one barrier per K-tile sits before
//     the LAST group, so the first fragments of tile t+1 are fetched behind 16 MFMAs instead of in
//     front of an idle pipe (measured +7 %: 129 -> 138 TFLOP/s at 8192^3)
//   * the DMA of tile t+1 is issued at the top of tile t into the other buffer; each wave waits for its own
//     pieces (vmcnt) only right before the barrier: three MFMA groups of cover
//   * blockIdx -> tile map keeps each XCD (private 4 MiB L2) on a contiguous strip of tiles that
//     share B rows
// The 128x128 diagonal blocks are factored and inverted by one workgroup in LDS; the panel below
// a diagonal block is then a GEMM with the inverse (TRSM as GEMM, the MAGMA trick), so it also
// runs on MFMA.  The inverses are kept: the triangular solves reuse them.
//
// This unit: the leaf-pair and padding kernels, the three factorization schedules -- the recursion (potrf_rec, potrf_rec_batched),
// the two-stream look-ahead, the task graph -- and oisat_potrf*.  gemm_nt is dense_gemm.hip, the diagonal-block kernel and the
// task-graph kernel dense_dag.hip, sweeps, gain solve and the batch API dense_solve.hip, the diagnostics dense_post.hip.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"

// ---- leaf PAIRS: two block columns (b, b+1) per leaf of the recursion ---------------------------------------------------
// With one block per leaf the rows below a pair of diagonal blocks are swept three times at K = 128 -- TRSM with T_b, the
// rank-128 update of column b+1, TRSM with T_b+1 -- each pass reading and writing a 64-KB tile per 4.2 MFLOP (16 flop/B:
// HBM-bound; in a month of 48 tiles these launches are 40 % of the factorization time for 10 % of its flops).  The pair
// form makes ONE pass:  P1 = X1 T_b^T;  X2 -= P1 L21^T;  P2 = X2 T_b+1^T  per 64 rows, with P1 and X2 handed from one
// product to the next through an LDS image (pair_panel_kernel), after a one-workgroup step has produced
// L21 = S[b+1,b] T_b^T and S[b+1,b+1] -= L21 L21^T between the two diagonal factorizations (pair_mid_kernel).
// Same products, same k order and the same single rounding of C - sum as the three launches they replace.
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int LDP = NB + 4;                // row stride of a full-K LDS operand image (floats)

// whole B operand [128 x 128] of one product into registers: 16 float4 per thread (chunk kt = rb[4 kt .. 4 kt + 3]), all
// loads in flight at once -- these kernels are latency-bound when few workgroups run (a polar cap, a single system)
__device__ __forceinline__ void b_load_all(v4f (&rb)[16], const float* __restrict__ g, int64_t ldg, int t) {
    const float* p = g + (int64_t)(t >> 3) * ldg + (t & 7) * 4;
#define OISAT_BL(kt, q) rb[4 * (kt) + (q)] = *reinterpret_cast<const v4f*>(p + (int64_t)(32 * (q)) * ldg + (kt) * BK);
    OISAT_BL(0, 0) OISAT_BL(0, 1) OISAT_BL(0, 2) OISAT_BL(0, 3) OISAT_BL(1, 0) OISAT_BL(1, 1) OISAT_BL(1, 2) OISAT_BL(1, 3)
    OISAT_BL(2, 0) OISAT_BL(2, 1) OISAT_BL(2, 2) OISAT_BL(2, 3) OISAT_BL(3, 0) OISAT_BL(3, 1) OISAT_BL(3, 2) OISAT_BL(3, 3)
#undef OISAT_BL
}

// acc0 | acc1 (a wave's 32 x 64 piece: rows wr*32.., columns wc*64.. and +32) += A[64 x 128] B[128 x 128]^T, A from a full-K
// LDS image (stride LDP), B from registers (b_load_all) through the one-chunk LDS image `ldsB`.  next != nullptr: as soon
// as chunk kt has gone to LDS its registers are refilled with chunk kt of the NEXT product's B operand, so that product
// finds its operand in registers -- one register set, and only the first product of a kernel waits for memory.
template <int KT, bool NEXT>
__device__ __forceinline__ void rows64_chunk(f32x16& acc0, f32x16& acc1, const float* __restrict__ imgA, v4f (&rb)[16],
                                             float* __restrict__ ldsB, int t, const float* __restrict__ next, int64_t ldnext) {
    const int lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int frow = lane & 31, fh = lane >> 5;
    const int aoff = (wr * 32 + frow) * LDP + 4 * fh, boff = (wc * 64 + frow) * LDSW + 4 * fh;
    const int srow = t >> 3, sk = (t & 7) * 4;
    __syncthreads();                                                    // the previous chunk (or the image's writers) are done
    *reinterpret_cast<v4f*>(&ldsB[(srow + 0) * LDSW + sk]) = rb[4 * KT + 0];
    *reinterpret_cast<v4f*>(&ldsB[(srow + 32) * LDSW + sk]) = rb[4 * KT + 1];
    *reinterpret_cast<v4f*>(&ldsB[(srow + 64) * LDSW + sk]) = rb[4 * KT + 2];
    *reinterpret_cast<v4f*>(&ldsB[(srow + 96) * LDSW + sk]) = rb[4 * KT + 3];
    if (NEXT) {
        const float* g = next + (int64_t)srow * ldnext + KT * BK + sk;
        rb[4 * KT + 0] = *reinterpret_cast<const v4f*>(g);
        rb[4 * KT + 1] = *reinterpret_cast<const v4f*>(g + 32 * ldnext);
        rb[4 * KT + 2] = *reinterpret_cast<const v4f*>(g + 64 * ldnext);
        rb[4 * KT + 3] = *reinterpret_cast<const v4f*>(g + 96 * ldnext);
    }
    __syncthreads();
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const float4 a = *reinterpret_cast<const float4*>(&imgA[aoff + KT * BK + 8 * s4]);
        const float4 b0 = *reinterpret_cast<const float4*>(&ldsB[boff + 8 * s4]);
        const float4 b1 = *reinterpret_cast<const float4*>(&ldsB[boff + 32 * LDSW + 8 * s4]);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
    }
}

template <bool NEXT>
__device__ __forceinline__ void rows64_product(f32x16& acc0, f32x16& acc1, const float* __restrict__ imgA, v4f (&rb)[16],
                                               float* __restrict__ ldsB, int t, const float* __restrict__ next, int64_t ldnext) {
    rows64_chunk<0, NEXT>(acc0, acc1, imgA, rb, ldsB, t, next, ldnext);
    rows64_chunk<1, NEXT>(acc0, acc1, imgA, rb, ldsB, t, next, ldnext);
    rows64_chunk<2, NEXT>(acc0, acc1, imgA, rb, ldsB, t, next, ldnext);
    rows64_chunk<3, NEXT>(acc0, acc1, imgA, rb, ldsB, t, next, ldnext);
}

// element (e, half) of a wave's accumulator pair -> (row, column) inside the 64 x 128 piece of the workgroup
#define OISAT_PIECE_ROW(e) (wr * 32 + ((e) & 3) + 8 * ((e) >> 2) + 4 * fh)
#define OISAT_PIECE_COL(half) (wc * 64 + 32 * (half) + frow)

// rows of 64 below a leaf pair (b, b+1): one pass over S[rows, b*128 : (b+2)*128].  Every global load is issued as early
// as registers allow: X1 and T_b at once, L21 while the first product runs, T_b+1 and X2 while the second one does.
template <bool BATCH>
__global__ __launch_bounds__(256) void pair_panel_kernel(float* __restrict__ S, int64_t ld, int mpb, const float* __restrict__ tinv,
                                                          int b, const BatchMat* __restrict__ mats, int prio) {
    __shared__ __attribute__((aligned(16))) float img[SB * LDP];         // 33,792 B: X1 -> P1 -> X2'
    __shared__ __attribute__((aligned(16))) float ldsB[NB * LDSW];       // 18,432 B
    group_prio(prio);
    if (BATCH) {
        const BatchMat* bm = mats + blockIdx.y;
        S = bm->S;
        ld = bm->ld;
        mpb = bm->mpb;
        tinv = bm->tinv;
    }
    if ((int)blockIdx.x >= (mpb - b - 2) * 2) return;                   // this matrix has fewer rows below the pair (or none)
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1, frow = lane & 31, fh = lane >> 5;
    float* X1 = S + ((int64_t)(b + 2) * NB + (int64_t)blockIdx.x * SB) * ld + (int64_t)b * NB;      // my 64 rows, column block b
    float* X2 = X1 + NB;                                                                            // ... column block b+1
    const float* Tb = tinv + (int64_t)b * NB * NB;
    const float* Tb1 = Tb + NB * NB;
    const float* L21 = S + (int64_t)(b + 1) * NB * ld + (int64_t)b * NB;
    v4f rb[16];
    {
        v4f xr[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) xr[q] = *reinterpret_cast<const v4f*>(X1 + (int64_t)((t >> 5) + 8 * q) * ld + (t & 31) * 4);
        b_load_all(rb, Tb, NB, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) *reinterpret_cast<v4f*>(&img[((t >> 5) + 8 * q) * LDP + (t & 31) * 4]) = xr[q];
    }
    f32x16 acc0 = {0}, acc1 = {0};
    rows64_product<true>(acc0, acc1, img, rb, ldsB, t, L21, ld);              // P1 = X1 T_b^T            (rb <- L21 on the way)
    __syncthreads();                                                    // every wave has read X1 from the image
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        X1[(int64_t)r * ld + OISAT_PIECE_COL(0)] = acc0[e];
        X1[(int64_t)r * ld + OISAT_PIECE_COL(1)] = acc1[e];
        img[r * LDP + OISAT_PIECE_COL(0)] = acc0[e];
        img[r * LDP + OISAT_PIECE_COL(1)] = acc1[e];
    }
    f32x16 x2a, x2b;                                                    // my elements of X2, in accumulator layout
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        x2a[e] = X2[(int64_t)r * ld + OISAT_PIECE_COL(0)];
        x2b[e] = X2[(int64_t)r * ld + OISAT_PIECE_COL(1)];
    }
    acc0 = f32x16{0};
    acc1 = f32x16{0};
    rows64_product<true>(acc0, acc1, img, rb, ldsB, t, Tb1, NB);              // Q = P1 L21^T             (rb <- T_b+1 on the way)
    __syncthreads();                                                    // every wave has read P1 from the image
#pragma unroll
    for (int e = 0; e < 16; ++e) {                                      // X2' = X2 - Q, rounded once, as the rank-128 update does
        const int r = OISAT_PIECE_ROW(e);
        img[r * LDP + OISAT_PIECE_COL(0)] = x2a[e] - acc0[e];
        img[r * LDP + OISAT_PIECE_COL(1)] = x2b[e] - acc1[e];
    }
    acc0 = f32x16{0};
    acc1 = f32x16{0};
    rows64_product<false>(acc0, acc1, img, rb, ldsB, t, (const float*)nullptr, 0);      // P2 = X2' T_b+1^T
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        X2[(int64_t)r * ld + OISAT_PIECE_COL(0)] = acc0[e];
        X2[(int64_t)r * ld + OISAT_PIECE_COL(1)] = acc1[e];
    }
}

// one 64-row half of pair_mid's second product: D_half -= L21_half L21^T (B = L21 from registers)
__device__ __forceinline__ void pair_mid_update(float* __restrict__ Dh, int64_t ld, const float* __restrict__ imgA, v4f (&rb)[16],
                                                float* __restrict__ ldsB, int t, bool keep_b) {
    const int lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1, frow = lane & 31, fh = lane >> 5;
    f32x16 d0, d1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        d0[e] = Dh[(int64_t)r * ld + OISAT_PIECE_COL(0)];
        d1[e] = Dh[(int64_t)r * ld + OISAT_PIECE_COL(1)];
    }
    f32x16 a0 = {0}, a1 = {0};
    (void)keep_b;
    rows64_product<false>(a0, a1, imgA, rb, ldsB, t, (const float*)nullptr, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        Dh[(int64_t)r * ld + OISAT_PIECE_COL(0)] = d0[e] - a0[e];
        Dh[(int64_t)r * ld + OISAT_PIECE_COL(1)] = d1[e] - a1[e];
    }
}

// between the two diagonal factorizations of a pair: L21 = S[b+1,b] T_b^T (in place), S[b+1,b+1] -= L21 L21^T.  One
// workgroup per matrix, on the dependent chain: X and T_b are requested at once, L21 is handed from the first product to
// the second through LDS (as A image and, chunk by chunk, as B), 64 rows at a time.
template <bool BATCH>
__global__ __launch_bounds__(256) void pair_mid_kernel(float* __restrict__ S, int64_t ld, int mpb, const float* __restrict__ tinv, int b,
                                                        const BatchMat* __restrict__ mats, int prio) {
    __shared__ __attribute__((aligned(16))) float img0[SB * LDP], img1[SB * LDP];      // the two 64-row halves of X, then of L21
    __shared__ __attribute__((aligned(16))) float ldsB[NB * LDSW];                     // 67,584 + 18,432 B
    group_prio(prio);
    if (BATCH) {
        const BatchMat* bm = mats + blockIdx.x;
        S = bm->S;
        ld = bm->ld;
        mpb = bm->mpb;
        tinv = bm->tinv;
    }
    if (b + 1 >= mpb) return;                                           // the pair's second block does not exist in this matrix
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1, frow = lane & 31, fh = lane >> 5;
    float* X = S + (int64_t)(b + 1) * NB * ld + (int64_t)b * NB;          // S[b+1, b]
    float* D = X + NB;                                                    // S[b+1, b+1]
    v4f rb[16];
    {
        v4f xr[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const v4f*>(X + (int64_t)((t >> 5) + 8 * q) * ld + (t & 31) * 4);
        b_load_all(rb, tinv + (int64_t)b * NB * NB, NB, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            *reinterpret_cast<v4f*>(&img0[((t >> 5) + 8 * q) * LDP + (t & 31) * 4]) = xr[q];
            *reinterpret_cast<v4f*>(&img1[((t >> 5) + 8 * q) * LDP + (t & 31) * 4]) = xr[8 + q];
        }
    }
    // L21 = X T_b^T: both halves need the same B, so its registers are refilled with T_b itself for the second half
    f32x16 la0 = {0}, la1 = {0}, lb0 = {0}, lb1 = {0};
    rows64_product<true>(la0, la1, img0, rb, ldsB, t, tinv + (int64_t)b * NB * NB, NB);
    rows64_product<false>(lb0, lb1, img1, rb, ldsB, t, (const float*)nullptr, 0);
    __syncthreads();                                                    // every wave has read X from the images
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = OISAT_PIECE_ROW(e);
        X[(int64_t)r * ld + OISAT_PIECE_COL(0)] = la0[e];
        X[(int64_t)r * ld + OISAT_PIECE_COL(1)] = la1[e];
        X[(int64_t)(SB + r) * ld + OISAT_PIECE_COL(0)] = lb0[e];
        X[(int64_t)(SB + r) * ld + OISAT_PIECE_COL(1)] = lb1[e];
        img0[r * LDP + OISAT_PIECE_COL(0)] = la0[e];
        img0[r * LDP + OISAT_PIECE_COL(1)] = la1[e];
        img1[r * LDP + OISAT_PIECE_COL(0)] = lb0[e];
        img1[r * LDP + OISAT_PIECE_COL(1)] = lb1[e];
    }
    __syncthreads();
    // B operand of the second product = L21 itself: its K-chunks come from the images (row r of L21, the chunk's columns)
    const int srow = t >> 3, sk = (t & 7) * 4;
#define OISAT_LOAD_L21()                                                                                        \
    do {                                                                                                        \
        rb[0] = *reinterpret_cast<const v4f*>(&img0[srow * LDP + 0 * BK + sk]);                              \
        rb[1] = *reinterpret_cast<const v4f*>(&img0[(srow + 32) * LDP + 0 * BK + sk]);                       \
        rb[2] = *reinterpret_cast<const v4f*>(&img1[srow * LDP + 0 * BK + sk]);                              \
        rb[3] = *reinterpret_cast<const v4f*>(&img1[(srow + 32) * LDP + 0 * BK + sk]);                       \
        rb[4] = *reinterpret_cast<const v4f*>(&img0[srow * LDP + 1 * BK + sk]);                              \
        rb[5] = *reinterpret_cast<const v4f*>(&img0[(srow + 32) * LDP + 1 * BK + sk]);                       \
        rb[6] = *reinterpret_cast<const v4f*>(&img1[srow * LDP + 1 * BK + sk]);                              \
        rb[7] = *reinterpret_cast<const v4f*>(&img1[(srow + 32) * LDP + 1 * BK + sk]);                       \
        rb[8] = *reinterpret_cast<const v4f*>(&img0[srow * LDP + 2 * BK + sk]);                              \
        rb[9] = *reinterpret_cast<const v4f*>(&img0[(srow + 32) * LDP + 2 * BK + sk]);                       \
        rb[10] = *reinterpret_cast<const v4f*>(&img1[srow * LDP + 2 * BK + sk]);                             \
        rb[11] = *reinterpret_cast<const v4f*>(&img1[(srow + 32) * LDP + 2 * BK + sk]);                      \
        rb[12] = *reinterpret_cast<const v4f*>(&img0[srow * LDP + 3 * BK + sk]);                             \
        rb[13] = *reinterpret_cast<const v4f*>(&img0[(srow + 32) * LDP + 3 * BK + sk]);                      \
        rb[14] = *reinterpret_cast<const v4f*>(&img1[srow * LDP + 3 * BK + sk]);                             \
        rb[15] = *reinterpret_cast<const v4f*>(&img1[(srow + 32) * LDP + 3 * BK + sk]);                      \
    } while (0)
    OISAT_LOAD_L21();
    pair_mid_update(D, ld, img0, rb, ldsB, t, true);
    OISAT_LOAD_L21();
    pair_mid_update(D + (int64_t)SB * ld, ld, img1, rb, ldsB, t, false);
#undef OISAT_LOAD_L21
}
#undef OISAT_PIECE_ROW
#undef OISAT_PIECE_COL

// identity padding of rows m..mp (columns 0..mp)
__global__ __launch_bounds__(256) void pad_identity_kernel(float* __restrict__ S, int64_t ld, int64_t m, int64_t mp) {
    const int64_t total = (mp - m) * mp;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int64_t r = m + p / mp, c = p % mp;
        S[r * ld + c] = r == c ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void pad_identity_batched_kernel(const BatchMat* __restrict__ mats) {
    const BatchMat m = mats[blockIdx.y];
    const int64_t mp = (int64_t)m.mpb * NB;
    const int64_t total = (mp - m.m) * mp;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int64_t r = m.m + p / mp, c = p % mp;
        m.S[r * m.ld + c] = r == c ? 1.f : 0.f;
    }
}

// factor block columns [b0, b1) (units of NB) given that everything to their left is applied
int potrf_rec(oisat_ctx* h, float* S, int64_t ld, int64_t mpb, int64_t b0, int64_t b1, float* tinv, int* info_dev) {
    if (b1 - b0 == 1) {
        const int64_t k0 = b0 * NB;
        if (int rc = launch_potrf_diag(h, 1, S, ld, k0, tinv, info_dev, (int)b0, nullptr, 0)) return rc;
        const int64_t rows = (mpb - b0 - 1) * NB;
        if (rows > 0) {
            float* P = S + (k0 + NB) * ld + k0;                  // panel below the diagonal block
            const int rc = launch_gemm(h, "trsm_gemm", P, ld, P, ld, tinv + b0 * NB * NB, NB, rows, NB, NB, 1, 0);
            if (rc) return rc;
        }
        return OISAT_OK;
    }
    if (b1 - b0 == 2 && kSinglePairs) {                     // leaf pair (b0, b0 + 1): OISAT_LEAF_PAIRS_SINGLE=1 (experiments)
        if (int rc = launch_potrf_diag(h, 1, S, ld, b0 * NB, tinv, info_dev, (int)b0, nullptr, 0)) return rc;
        OISAT_LAUNCH(h, "pair_mid", pair_mid_kernel<false>, dim3(1), dim3(256), 0, S, ld, (int)mpb, (const float*)tinv, (int)b0,
                     (const BatchMat*)nullptr, 0);
        if (int rc = launch_potrf_diag(h, 1, S, ld, (b0 + 1) * NB, tinv, info_dev, (int)(b0 + 1), nullptr, 0)) return rc;
        const int64_t rows = mpb - b0 - 2;
        if (rows > 0) {
            OISAT_LAUNCH(h, "pair_panel", pair_panel_kernel<false>, dim3((unsigned)(rows * 2)), dim3(256), 0, S, ld, (int)mpb,
                         (const float*)tinv, (int)b0, (const BatchMat*)nullptr, 0);
        }
        return OISAT_OK;
    }
    const int64_t mid = split_mid(b0, b1, kSinglePairs);
    int rc = potrf_rec(h, S, ld, mpb, b0, mid, tinv, info_dev);
    if (rc) return rc;
    // S[mid:, mid:b1] -= L[mid:, b0:mid] * L[mid:b1, b0:mid]^T   (region anchored on the diagonal)
    {
        float* Cc = S + mid * NB * ld + mid * NB;
        const float* Aa = S + mid * NB * ld + b0 * NB;
        rc = launch_gemm(h, "syrk_gemm", Cc, ld, Aa, ld, Aa, ld, (mpb - mid) * NB, (b1 - mid) * NB, (int)((mid - b0) * NB), 0, 1);
        if (rc) return rc;
    }
    return potrf_rec(h, S, ld, mpb, mid, b1, tinv, info_dev);
}

// ---- right-looking Cholesky with look-ahead on two streams (small and mid-size matrices) --------------
// The recursive schedule above is one dependent chain: while the panel work of a column runs (one CU for the
// diagonal block, <= mp/128 tiles for the TRSM) the other 250 CUs idle, and for m ~ 1e4 that chain IS the run
// time.  Here panel j's trailing update is split three ways:
//     A(j):  the columns of panel j+1   -> main stream, right behind panel j (the next panel needs them at once)
//     B1(j): the columns of panel j+2   -> aux stream
//     B2(j): everything further right   -> aux stream (the bulk of the trailing update)
// so the chain  panel(j) -> A(j) -> panel(j+1) ...  only ever waits for B1 of two panels back, and the bulk
// updates fill the idle CUs.  Tiles are never touched by two in-flight launches: the columns of panel c receive
// panel c-1 through A (main), panel c-2 through B1 and panels <= c-3 through B2 (aux, in order), and the main
// stream waits for B1(c-2) before it touches them.  A panel is `pw` diagonal blocks wide: rank-128 updates
// (pw = 1) stream the whole trailing matrix through HBM for 32 flop/B and lose to the chain they were meant to
// hide; pw = 2..4 gives 64..128 flop/B.  Large matrices use the recursive schedule (K = half the matrix).
int potrf_lookahead(oisat_ctx* h, float* S, int64_t ld, int64_t nb, float* tinv, int* info_dev, int64_t pw) {
    // panels of `pw` diagonal blocks: panel q covers block columns [q*pw, min((q+1)*pw, nb)); a panel is factored
    // (all rows below included) by the recursive routine on the main stream, its trailing update has K = pw*128
    const int64_t np = cdiv(nb, pw);
    if (!h->aux_stream) {
        // lowest priority: the bulk updates must not sit in front of the panel chain when a CU slot frees up
        int prio_low = 0, prio_high = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        const int prio = prio_low;
        // (round 1 also tried keeping CUs off limits for the bulk updates -- a CU-masked stream -- so that the panel chain's
        // one-workgroup kernels always find a home: every masked GEMM loses >= 12 %, profiles/EXPERIMENTS.md)
        HIP_TRY(hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, prio));
    }
    while ((int64_t)h->sync_events.size() < 2 * np + 2) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        h->sync_events.push_back(ev);
    }
    hipStream_t s1 = h->stream, s2 = h->aux_stream;
    auto E1 = [&](int64_t q) { return h->sync_events[2 * q]; };          // panel q ready (main)
    auto E2 = [&](int64_t q) { return h->sync_events[2 * q + 1]; };      // B1(q) done (aux)
    hipEvent_t ev_edge = h->sync_events[2 * np];
    HIP_TRY(hipEventRecord(ev_edge, s1));
    HIP_TRY(hipStreamWaitEvent(s2, ev_edge, 0));                          // S is built before the aux stream touches it
    auto c0 = [&](int64_t q) { return (q * pw < nb ? q * pw : nb); };     // first block column of panel q
    int rc = OISAT_OK;
    // C[r0.., cb0..cb1) -= L[r0.., kb0..kb1) * L[cb0..cb1, kb0..kb1)^T  with r0 == cb0 (anchored on the diagonal)
    auto update = [&](int64_t cb0, int64_t cb1, int64_t kb0, int64_t kb1) {
        if (cb1 <= cb0) return (int)OISAT_OK;
        float* Cc = S + cb0 * NB * ld + cb0 * NB;
        const float* Aa = S + cb0 * NB * ld + kb0 * NB;
        return launch_gemm(h, "syrk_gemm", Cc, ld, Aa, ld, Aa, ld, (nb - cb0) * NB, (cb1 - cb0) * NB, (int)((kb1 - kb0) * NB), 0, 1);
    };
    for (int64_t q = 0; q < np && rc == OISAT_OK; ++q) {
        if (q >= 2) HIP_TRY(hipStreamWaitEvent(s1, E2(q - 2), 0));       // panel q's columns hold panel q-2 (and all earlier)
        rc = potrf_rec(h, S, ld, nb, c0(q), c0(q + 1), tinv, info_dev);  // diag blocks, TRSMs, in-panel updates
        if (rc || q + 1 == np) break;
        HIP_TRY(hipEventRecord(E1(q), s1));
        if (q >= 1) HIP_TRY(hipStreamWaitEvent(s1, E2(q - 1), 0));       // B1(q-1) wrote the same columns
        rc = update(c0(q + 1), c0(q + 2), c0(q), c0(q + 1));              // A(q): the next panel's columns, main stream
        if (rc) break;
        if (q + 2 < np) {
            HIP_TRY(hipStreamWaitEvent(s2, E1(q), 0));
            h->stream = s2;                                               // launches (and their profiling events) go to aux
            rc = update(c0(q + 2), c0(q + 3), c0(q), c0(q + 1));          // B1(q): panel q+2's columns
            if (rc == OISAT_OK && hipEventRecord(E2(q), s2) != hipSuccess) rc = OISAT_EHIP;
            if (rc == OISAT_OK) rc = update(c0(q + 3), nb, c0(q), c0(q + 1));   // B2(q): everything to the right
            h->stream = s1;
        }
    }
    h->stream = s1;
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev_edge, s2));
    HIP_TRY(hipStreamWaitEvent(s1, ev_edge, 0));                          // join: nothing of the factorization is left in flight
    return OISAT_OK;
}

}  // namespace

namespace oisat_dense {

// ---- batched recursion: the same tree as potrf_rec over the block range of the LARGEST matrix; a node applies to the
// matrices that reach it (a prefix of the table), every launch covers all of them ------------------------------------------
int potrf_rec_batched(oisat_ctx* h, const ChBatch& bt, int b0, int b1, int* info_dev) {
    if (b1 - b0 == 1) {
        int cnt = 0;
        for (const BatchMat& m : bt.table) {
            if (m.mpb <= b0) break;
            ++cnt;
        }
        if (cnt == 0) return OISAT_OK;
        if (int rc = launch_potrf_diag(h, (unsigned)cnt, nullptr, 0, (int64_t)b0 * NB, nullptr, info_dev, b0, (const BatchMat*)bt.table_dev, h->wave_prio))
            return rc;
        return launch_gemm_batched(h, "trsm_gemm", bt, BatchArgs{bt.table_dev, 1, b0, 0, 0}, NB, 1, 0);
    }
    if (b1 - b0 == 2 && bt.pairs) {                         // leaf pair (b0, b0 + 1)
        int cnt = 0, maxrows = 0;
        for (const BatchMat& m : bt.table) {
            if (m.mpb <= b0) break;
            ++cnt;
            if (m.mpb - b0 - 2 > maxrows) maxrows = m.mpb - b0 - 2;
        }
        if (cnt == 0) return OISAT_OK;
        const BatchMat* tb = (const BatchMat*)bt.table_dev;
        if (int rc = launch_potrf_diag(h, (unsigned)cnt, nullptr, 0, (int64_t)b0 * NB, nullptr, info_dev, b0, tb, h->wave_prio)) return rc;
        OISAT_LAUNCH(h, "pair_mid", pair_mid_kernel<true>, dim3((unsigned)cnt), dim3(256), 0, (float*)nullptr, (int64_t)0, 0,
                     (const float*)nullptr, b0, tb, h->wave_prio);
        if (int rc = launch_potrf_diag(h, (unsigned)cnt, nullptr, 0, (int64_t)(b0 + 1) * NB, nullptr, info_dev, b0 + 1, tb, h->wave_prio)) return rc;
        if (maxrows > 0) {
            OISAT_LAUNCH(h, "pair_panel", pair_panel_kernel<true>, dim3((unsigned)(maxrows * 2), (unsigned)cnt), dim3(256), 0,
                         (float*)nullptr, (int64_t)0, 0, (const float*)nullptr, b0, tb, h->wave_prio);
        }
        return OISAT_OK;
    }
    const int mid = (int)split_mid(b0, b1, bt.pairs);
    int rc = potrf_rec_batched(h, bt, b0, mid, info_dev);
    if (rc) return rc;
    rc = launch_gemm_batched(h, "syrk_gemm", bt, BatchArgs{bt.table_dev, 0, b0, mid, b1}, (mid - b0) * NB, 0, 1);
    if (rc) return rc;
    return potrf_rec_batched(h, bt, mid, b1, info_dev);
}

// pad_identity_batched_kernel over the whole table, for the batch API (dense_solve.hip)
int pad_identity_batched(oisat_ctx* h, const ChBatch& bt) {
    OISAT_LAUNCH(h, "pad_identity", pad_identity_batched_kernel, dim3(32, (unsigned)bt.table.size()), dim3(256), 0,
                 (const BatchMat*)bt.table_dev);
    return OISAT_OK;
}

}  // namespace oisat_dense

extern "C" int oisat_set_task_graph(oisat_ctx* h, int mode) {
    ARG_CHECK(h != nullptr && mode >= -1 && mode <= 1);
    h->dag_mode = mode;
    return OISAT_OK;
}

struct PotrfEnv {                // the envelope of S and its stretches; all null: dense
    const int32_t* first = nullptr;     // host first[mpb] ...
    const int32_t* env_dev = nullptr;   // ... and device first[mpb] | last[mpb] (oisat_envelope)
    const int32_t* far = nullptr;       // host int32[mpb], with first, or null: the far stretch of every block row (oisat_factor_far), bf16 K-blocks in the task graph
    const int32_t* mid = nullptr;       // likewise: the middle stretch behind it (oisat_factor_mid), split bf16 K-blocks
    const int32_t* near = nullptr;      // likewise: the near stretch behind that (oisat_factor_near), three-way split bf16 K-blocks
};
// fwd_d (device double[m]) or nullptr: the right-hand side whose first forward sweep rides in the task-graph launch
// (oisat_potrf_env_fwd).  schedule_out (optional): OISAT_SCHEDULE_* of what ran.
static int potrf_impl(oisat_ctx* h, float* S, int64_t m, int64_t ld, int* info_host, const PotrfEnv& env, const double* fwd_d = nullptr,
                      int* schedule_out = nullptr) {
    ARG_CHECK(h && S && m > 0);
    const int32_t* const first = env.first;
    const int32_t* const env_dev = env.env_dev;
    h->factor.fwd_d = nullptr;                                  // whatever comes of this call, the last factor's forward vector is history
    h->shadow_last = nullptr;                                   // ... and so is its shadow
    if (schedule_out) *schedule_out = OISAT_SCHEDULE_OTHER;
    const int64_t mp = cdiv(m, NB) * NB;
    ARG_CHECK(ld >= mp && (ld % 4) == 0 && ((uintptr_t)S % 16) == 0);
    const int64_t mpb = mp / NB;
    float* tinv = (float*)oisat_ws(h, 3, sizeof(float) * mpb * NB * NB);
    int* info_dev = nullptr;
    if (!tinv) return OISAT_ENOMEM;
    if (int rc = status_ws(h, &info_dev, nullptr)) return rc;
    HIP_TRY(dense_kernel_attributes());
    HIP_TRY(hipMemsetAsync(info_dev, 0, sizeof(int), h->stream));      // info[0] only: the sticky words survive
    if (mp > m) {
        OISAT_LAUNCH(h, "pad_identity", pad_identity_kernel, dim3(stream_grid((mp - m) * mp, 256)), dim3(256), 0, S, ld, m, mp);
    }
    // schedule: recursive by default.  The two-stream look-ahead schedule (OISAT_POTRF=lookahead[:panel blocks]) is
    // kept selectable: at m = 1e4 it ties the recursive one in every round (round 1: 12.7 ms per analysis either way,
    // the 137 KB diagonal kernel waiting 300-350 us for an empty CU under the bulk updates; round 2 with the 26 KB
    // register-resident kernel: 7.75-7.80 ms at panel widths 6..20 against 7.84 ms) -- its rank-256..1024 bulk updates
    // cost 5.4-6.3 ms where the recursion's GEMMs cost 4.1.  See DESIGN.md section 4.
    bool lookahead = false;
    int64_t pw = 4;
    const bool schedule_forced = potrf_schedule(&lookahead, &pw);
    lookahead = lookahead && mpb >= 2;
    int rc;
    // (an enveloped ticket has ten bits for a block column: larger systems take the recursion, which reads the build's zeros)
    if (!lookahead && !schedule_forced && dag_wanted(h, mpb, 1) && dag_fits(1, dag_slots(h)) && (!first || mpb <= kDagEnvMaxBlocks)) {
        // the plan of this (S, tinv, ld, block rows, enveloped or not) -- a handle keeps the last few (a lane that factors its
        // tiles one after the other in ONE shared buffer meets the same few sizes month after month).  An enveloped plan's
        // ticket list belongs to ONE envelope: the table itself is compared, and another envelope refills the plan's buffers.
        const bool ride = fwd_d != nullptr && !fwd_in_launch_off();
        DagSingle* hit = nullptr;
        for (DagSingle& c : h->dag_cache)
            if (c.plan && c.S == S && c.tinv == tinv && c.ld == ld && c.mpb == mpb && c.enveloped == (first != nullptr) && c.fwd == ride) hit = &c;
        if (hit && first && !hit->plan->bands.equals((size_t)mpb, first, env.far, env.mid, env.near))
            if (int rf = dag_plan_refill(*hit->plan, DagBands((int)mpb, first, env.far, env.mid, env.near), h->stream)) return rf;
        if (!hit) {
            DagSingle* slot = nullptr;
            for (DagSingle& c : h->dag_cache)
                if (!c.plan) { slot = &c; break; }
            if (!slot) {                                         // evict the least recently used
                slot = &h->dag_cache[0];
                for (DagSingle& c : h->dag_cache)
                    if (c.stamp < slot->stamp) slot = &c;
                HIP_TRY(hipStreamSynchronize(h->stream));        // (a plan is never freed under a running launch)
                oisat_dag_plan_release(slot->plan);
                slot->plan = nullptr;
            }
            DagSolveShape shape;
            if (ride) {                                         // the plan's shape: its ready queue holds the block rows of one forward sweep
                shape.refine = 0;
                shape.fwd_only = true;
            }
            slot->plan = dag_plan_create(std::vector<BatchMat>{BatchMat{S, tinv, ld, m, (int)mpb, 0}}, h->stream, shape,
                                         first ? DagBands((int)mpb, first, env.far, env.mid, env.near) : DagBands());
            if (!slot->plan) return OISAT_ENOMEM;
            slot->S = S; slot->tinv = tinv; slot->ld = ld; slot->mpb = mpb; slot->enveloped = first != nullptr; slot->fwd = ride;
            hit = slot;
        }
        hit->stamp = ++h->dag_clock;
        DagPlan& pl = *hit->plan;
        // The shadow: only where a far or middle block exists (the plan's tables are this call's), in workspace slot 10 -- grow-only,
        // one per handle, whose factorizations follow each other on its stream.  No room for it (or more than
        // oisat_set_factor_shadow_cap allows): the launch converts in its K-loops as before, the same bits; that is not an error.
        char* shadow = nullptr;
        int shadow_use = 0;
        if (first && (env.far || env.mid)) {
            const int mode = factor_shadow_mode();
            ARG_CHECK(mode >= 0 && "OISAT_FACTOR_SHADOW is 0, 1, far or mid");
            bool any = false;
            for (int64_t b = 0; b < mpb; ++b) any = any || pl.bands.mid[b] > pl.bands.first[b];
            const size_t bytes = (size_t)pl.sh_tiles * (size_t)kShTile;
            if (mode > 0 && any && (h->shadow_cap < 0 || bytes <= (size_t)h->shadow_cap)) {
                shadow = (char*)oisat_ws(h, 10, bytes);
                if (!shadow) (void)hipGetLastError();          // (the refused allocation is not this launch's error)
                shadow_use = shadow ? mode : 0;
            }
        }
        HIP_TRY(dag_plan_shadow(pl, shadow, shadow_use, h->stream));
        if (ride) {
            // what oisat_gain_solve does in front of its first solve: the padded right-hand side, the forward vector "not yet
            // published", the solve state reset -- then the launch, whose chain pushes row j of the sweep behind diagonal block j
            double* w = (double*)oisat_ws(h, 5, sizeof(double) * (2 + 8) * mp);
            SolveState* st = solve_state(h);
            char* base = nullptr;
            if (!w || !st) return OISAT_ENOMEM;
            if (int rs = status_ws(h, nullptr, &base)) return rs;
            if (int rp = solve_prep(h, fwd_d, m, mp, w, w + mp, st)) return rp;
            DagSolve sv{};
            sv.queue = pl.queue_dev;
            sv.qcap = (int)pl.qcap;
            sv.qcap0 = (int)pl.qcap0;
            sv.nsys = 1;
            sv.trsv_timeouts = (unsigned*)base;
            sv.fwd_rhs = w;
            sv.fwd_sol = w + mp;
            sv.env = first ? env_dev : nullptr;
            rc = dag_launch(h, pl, info_dev, (unsigned*)(info_dev + kInfoDagTimeouts), &sv);
            if (rc == OISAT_OK) h->factor.fwd_d = fwd_d;
        } else {
            rc = dag_launch(h, pl, info_dev, (unsigned*)(info_dev + kInfoDagTimeouts));
        }
        if (schedule_out) *schedule_out = !first ? OISAT_SCHEDULE_OTHER : ride ? OISAT_SCHEDULE_ENV_DAG_FWD : OISAT_SCHEDULE_ENV_DAG;
        if (rc == OISAT_OK && shadow) {                         // what oisat_factor_shadow_tile reads back
            h->shadow_last = shadow;
            h->shadow_first = pl.bands.first;
            h->shadow_shrow = pl.shrow;
        }
    } else {
        rc = lookahead ? potrf_lookahead(h, S, ld, mpb, tinv, info_dev, pw) : potrf_rec(h, S, ld, mpb, 0, mpb, tinv, info_dev);
    }
    if (rc) {
        h->factor.fwd_d = nullptr;
        return rc;
    }
    h->factor.S = S;
    h->factor.m = m;
    h->factor.mp = mp;
    h->factor.ld = ld;
    h->factor.tinv = tinv;
    h->factor.env = env_dev;
    h->factor.band = 0;
    h->factor.first.clear();
    if (first && env_dev) {
        for (int64_t b = 0; b < mpb; ++b) h->factor.band = std::max(h->factor.band, (int)(b - first[b]) + 1);
        h->factor.first.assign(first, first + mpb);
    }
    if (info_host) {
        int* pin = (int*)oisat_pinned(h, 64);
        if (!pin) return OISAT_ENOMEM;
        HIP_TRY(hipMemcpyAsync(pin, info_dev, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        *info_host = *pin;
        if (pin[kInfoDagTimeouts] != 0) {                       // reported here, not again by oisat_solve_status
            HIP_TRY(hipMemsetAsync(info_dev + kInfoDagTimeouts, 0, sizeof(int), h->stream));
            oisat_set_error("potrf: the task-graph factorization timed out (a workgroup gave up waiting): the factor is incomplete");
            return OISAT_EHIP;
        }
        if (*pin != 0) {
            // reported to the caller right here: do not report it a second time through oisat_solve_status
            HIP_TRY(hipMemsetAsync(info_dev + 1, 0, 2 * sizeof(int), h->stream));
            oisat_set_error("potrf: matrix not positive definite at column %d", *pin);
            return OISAT_ENOTPD;
        }
    }
    return OISAT_OK;
}

extern "C" int oisat_potrf(oisat_ctx* h, float* S, int64_t m, int64_t ld, int* info_host) {
    return potrf_impl(h, S, m, ld, info_host, PotrfEnv{});
}

extern "C" int oisat_factor_shadow_layout(int nb, const int32_t* first, int64_t* rowoff_out, int64_t* ntiles_out) {
    ARG_CHECK(nb >= 1 && nb <= kDagEnvMaxBlocks && first && rowoff_out && ntiles_out);
    ARG_CHECK(envelope_table_ok(first, nb));
    *ntiles_out = dag_shadow_layout(first, nb, rowoff_out);
    return OISAT_OK;
}

extern "C" int oisat_set_factor_shadow_cap(oisat_ctx* h, int64_t bytes) {
    ARG_CHECK(h != nullptr && bytes >= -1);
    h->shadow_cap = bytes;
    return OISAT_OK;
}

extern "C" int oisat_factor_shadow_tile(oisat_ctx* h, int r, int k, uint16_t* hi_out, uint16_t* lo_out) {
    ARG_CHECK(h != nullptr && hi_out && lo_out);
    ARG_CHECK(h->shadow_last != nullptr && "the last factorization on this handle filled a shadow");
    ARG_CHECK(r >= 1 && r < (int)h->shadow_first.size() && k >= h->shadow_first[r] && k < r);
    std::vector<uint16_t> raw((size_t)kShTile / 2);
    HIP_TRY(hipMemcpyAsync(raw.data(), h->shadow_last + (h->shadow_shrow[r] + k) * kShTile, (size_t)kShTile, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int plane = 0; plane < 2; ++plane)                     // plane [group][row][16 columns] -> row-major 128 x 128
        for (int g = 0; g < NB / 16; ++g)
            for (int row = 0; row < NB; ++row)
                memcpy((plane ? lo_out : hi_out) + row * NB + g * 16, raw.data() + (plane * kShPlane + g * kShGroup + row * 32) / 2, 32);
    return OISAT_OK;
}

// the two enveloped entry points: fwd = oisat_potrf_env_fwd, whose d is required
static int potrf_env_entry(oisat_ctx* h, float* S, int64_t m, int64_t ld, const int32_t* first, const int32_t* env_dev, bool fwd, const double* d,
                           int* info_host, int* schedule_out) {
    ARG_CHECK(h != nullptr);
    std::vector<int32_t> far, mid, near;
    far.swap(h->factor_far);                                    // one-shot, whatever this call's outcome
    mid.swap(h->factor_mid);                                    // likewise
    near.swap(h->factor_near);                                  // likewise
    ARG_CHECK(first && env_dev && (!fwd || d) && m > 0);
    ARG_CHECK(envelope_table_ok(first, cdiv(m, NB)) && far_table_ok(far, first, cdiv(m, NB)) &&
              mid_table_ok(mid, far, first, cdiv(m, NB)) && near_table_ok(near, mid, far, first, cdiv(m, NB)));
    PotrfEnv env;
    if (!oisat_envelope_off()) env = PotrfEnv{first, env_dev, far.empty() ? nullptr : far.data(), mid.empty() ? nullptr : mid.data(),
                                                  near.empty() ? nullptr : near.data()};
    return potrf_impl(h, S, m, ld, info_host, env, d, schedule_out);
}

extern "C" int oisat_potrf_env(oisat_ctx* h, float* S, int64_t m, int64_t ld, const int32_t* first, const int32_t* env_dev,
                               int* info_host) {
    return potrf_env_entry(h, S, m, ld, first, env_dev, false, nullptr, info_host, nullptr);
}

extern "C" int oisat_potrf_env_fwd(oisat_ctx* h, float* S, int64_t m, int64_t ld, const int32_t* first, const int32_t* env_dev,
                                   const double* d, int* info_host, int* schedule_out) {
    return potrf_env_entry(h, S, m, ld, first, env_dev, true, d, info_host, schedule_out);
}

extern "C" int oisat_factor_adopt(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* tinv) {
    ARG_CHECK(h && L && tinv && m > 0);
    const int64_t mp = cdiv(m, NB) * NB;
    ARG_CHECK(ld >= mp && (ld % 4) == 0 && ((uintptr_t)L % 16) == 0 && ((uintptr_t)tinv % 16) == 0);
    if (int rc = status_ws(h, nullptr, nullptr)) return rc;
    HIP_TRY(dense_kernel_attributes());
    h->factor.S = L;
    h->factor.m = m;
    h->factor.mp = mp;
    h->factor.ld = ld;
    h->factor.tinv = tinv;
    h->factor.env = nullptr;                                // (adopted without an envelope: swept densely)
    h->factor.band = 0;
    h->factor.first.clear();
    h->factor.fwd_d = nullptr;
    return OISAT_OK;
}
