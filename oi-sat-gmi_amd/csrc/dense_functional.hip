// Linear functionals of the analysis: for K weight vectors W (K x n, a regional mean per row) the
// analysis error covariance is
//     A_W = W B W^T - G^T S^-1 G,    G = H B W^T (m x K),    S = H B H^T + R,
// K refined gain solves through the factor a run left behind and two PAIR SUMS: G, the weights gathered at the observations,
// and T = B W^T, the weights gathered at their own support.  The pair sum is the transpose of the increment -- many sources
// (cells), summed at each target -- and A_W is a difference of two nearly equal numbers wherever a region is well observed, so
// everything here is float64: |p - q|^2 from the double coordinates, corr_f64, double fused multiply-adds.  No fp32 tier, no far
// tier.  oisat_rows_dot forms the K x K products (W T^T, G^T Y, R^T Y) on the device in a fixed order, so that nothing K x m or
// K x n travels to the host.  (No reference counterpart: the element-wise OI has no error correlations between cells.)
#include "oisat_common.h"
#include "dense_switches.h"

namespace {

#include "dense_solve_dev.inc"

// ---- out[k][p] = psig_p sum_j C(p, j) ssig_j W[k][j] for a group of G functionals at once (oisat_functional_gather) ---------
// probe_spread_kernel (dense_spread.inc) with the roles named anew and double sums: thread = one target, 256 consecutive targets
// per workgroup, the latitude window of the block's span and the bounding-sphere cull (block_sphere<1>), the surviving sources
// staged in LDS as double coordinates + index in candidate order.  Per group of G functionals the staged sources pass in
// sub-chunks of 64 whose weights ssig_j W[k][j] are gathered into an LDS image ([64][G] doubles, read back as wave-uniform
// 16-byte words), so that one evaluation of the correlation serves G fused multiply-adds into G double sums.  The group loop
// is the outer one: the sums of one group live in registers across the whole candidate range, and a pair's correlation is
// evaluated ceil(nfun / G) times.  A functional k >= nfun of the last group has weight 0 in the image; no row of W beyond
// nfun - 1 is read.  Fixed order everywhere: candidate order, then k.
// G = 16: 32 VGPRs of sums, one evaluation per pair up to 16 regions; the image is 64 x 18 doubles (9 216 bytes) beside the
// 14 336 bytes of the stage.
constexpr int kFunStage = 512;                                 // staged sources: processed once 256 have gathered
constexpr int kFunSub = 64;                                    // sources per weight image
constexpr int kFunGroup = 16;                                  // functionals per group
template <int KIND, int G>
__global__ __launch_bounds__(256) void functional_gather_kernel(const double* __restrict__ pxyz, const double* __restrict__ psig,
                                                                 const double* __restrict__ plat, int64_t npts,
                                                                 const double* __restrict__ sxyz, const double* __restrict__ ssig,
                                                                 const double* __restrict__ slat, int64_t nsrc,
                                                                 const double* __restrict__ W, int nfun, int64_t ldw, double a,
                                                                 double win_deg, double cut_chord, double* __restrict__ out,
                                                                 int64_t ldo) {
    constexpr int GS = G + 2;                                   // row stride of the weight image (16-byte aligned rows)
    __shared__ double sx[kFunStage], sy[kFunStage], sz[kFunStage];
    __shared__ int sidx[kFunStage];
    __shared__ __attribute__((aligned(16))) double sw[kFunSub * GS];
    __shared__ double red[16], s_lo[4], s_hi[4];
    __shared__ int64_t s_j[2];
    __shared__ int wcnt[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t pt = (int64_t)blockIdx.x * 256 + t;
    const bool live = pt < npts;
    const double px[1] = {live ? pxyz[pt] : 0.0}, py[1] = {live ? pxyz[npts + pt] : 0.0}, pz[1] = {live ? pxyz[2 * npts + pt] : 0.0};
    const bool lv[1] = {live};
    int64_t j0 = 0, j1 = nsrc;
    const bool windowed = plat && slat;
    if (windowed) {                                             // latitude span of this block's targets -> source index range
        double lo = live ? plat[pt] : 1e9, hi = live ? plat[pt] : -1e9;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
        if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
        __syncthreads();
        if (t == 0) {
            lo = fmin(fmin(s_lo[0], s_lo[1]), fmin(s_lo[2], s_lo[3]));
            hi = fmax(fmax(s_hi[0], s_hi[1]), fmax(s_hi[2], s_hi[3]));
            s_j[0] = lower_bound_lat(slat, nsrc, lo - win_deg);
            s_j[1] = lower_bound_lat(slat, nsrc, hi + win_deg + 1e-9);
        }
        __syncthreads();
        j0 = s_j[0];
        j1 = s_j[1];
    }
    const BlockSphere bs = block_sphere<1>(px, py, pz, lv, windowed ? cut_chord : 1e30, (double)INFINITY, red);
    const double sg = live ? psig[pt] : 0.0;
    for (int k0 = 0; k0 < nfun; k0 += G) {
        double acc[G];
#pragma unroll
        for (int kk = 0; kk < G; ++kk) acc[kk] = 0.0;
        int fill = 0;
        for (int64_t c0 = j0; c0 < j1; c0 += 256) {
            {   // one pass of 256 candidates: the survivors of the cull go to the stage in candidate order
                const int64_t c = c0 + t;
                double x = 0.0, y = 0.0, zz = 0.0;
                bool keep = false;
                if (c < j1) {
                    x = sxyz[c]; y = sxyz[nsrc + c]; zz = sxyz[2 * nsrc + c];
                    const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
                    keep = dx * dx + dy * dy + dz * dz <= bs.r2cull;
                }
                const unsigned long long mask = __ballot(keep);
                if (lane == 0) wcnt[w] = __popcll(mask);
                __syncthreads();
                const int c0w = wcnt[0], c1w = wcnt[1], c2w = wcnt[2], c3w = wcnt[3];
                if (keep) {
                    const int pos = fill + (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0) + __popcll(mask & ((1ull << lane) - 1ull));
                    sx[pos] = x; sy[pos] = y; sz[pos] = zz;
                    sidx[pos] = (int)c;
                }
                __syncthreads();
                fill += c0w + c1w + c2w + c3w;
            }
            if (fill < 256 && c0 + 256 < j1) continue;          // (block-uniform) at most 255 + 256 entries ever wait
            for (int s0 = 0; s0 < fill; s0 += kFunSub) {
                const int cnt = fill - s0 < kFunSub ? fill - s0 : kFunSub;
                if (lane < cnt) {                               // weights: wave w takes the functionals w, w + 4, ..; a lane one source
                    const int j = sidx[s0 + lane];
                    const double so = ssig[j];
                    for (int kk = w; kk < G; kk += 4) sw[lane * GS + kk] = k0 + kk < nfun ? so * W[(int64_t)(k0 + kk) * ldw + j] : 0.0;
                }
                __syncthreads();
                for (int o = 0; o < cnt; ++o) {
                    const double dx = px[0] - sx[s0 + o], dy = py[0] - sy[s0 + o], dz = pz[0] - sz[s0 + o];
                    const double c = corr_f64<KIND>(a, dx * dx + dy * dy + dz * dz);
#pragma unroll
                    for (int kk = 0; kk < G; kk += 2) {
                        const double2 wv = *reinterpret_cast<const double2*>(&sw[o * GS + kk]);
                        acc[kk] = __builtin_fma(c, wv.x, acc[kk]);
                        acc[kk + 1] = __builtin_fma(c, wv.y, acc[kk + 1]);
                    }
                }
                __syncthreads();
            }
            fill = 0;
        }
        if (live) {
#pragma unroll
            for (int kk = 0; kk < G; ++kk)
                if (k0 + kk < nfun) out[(int64_t)(k0 + kk) * ldo + pt] = sg * acc[kk];
        }
    }
}

// ---- out[k][l] = sum_p A[k][p] B[l][p] (oisat_rows_dot) ---------------------------------------------------------------------
// One workgroup per (row k of A, group of kDotGroup rows of B) walks the whole length: thread t adds the products at p = t,
// t + 256, .. in that order, the 64 lanes of a wave are joined by the butterfly, the four waves as (w0 + w1) + (w2 + w3).  The
// tree depends on len alone -- not on the grid, which is na x ceil(nb / kDotGroup) whatever the device, and not on timing.
constexpr int kDotGroup = 8;
__global__ __launch_bounds__(256) void rows_dot_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                       int nb, int64_t len, double* __restrict__ out) {
    __shared__ double red[4][kDotGroup];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int k = blockIdx.x, l0 = blockIdx.y * kDotGroup;
    const double* __restrict__ ar = A + (int64_t)k * lda;
    double acc[kDotGroup];
#pragma unroll
    for (int q = 0; q < kDotGroup; ++q) acc[q] = 0.0;
    for (int64_t p = t; p < len; p += 256) {
        const double av = ar[p];
#pragma unroll
        for (int q = 0; q < kDotGroup; ++q) {
            const double bv = l0 + q < nb ? B[(int64_t)(l0 + q) * ldb + p] : 0.0;       // (block-uniform test)
            acc[q] = __builtin_fma(av, bv, acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < kDotGroup; ++q) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[q] += __shfl_xor(acc[q], o, kWave);
        if (lane == 0) red[w][q] = acc[q];
    }
    __syncthreads();
    if (t < kDotGroup && l0 + t < nb) out[(int64_t)k * nb + l0 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

}  // namespace

extern "C" int oisat_functional_gather(oisat_ctx* h, const double* pxyz, const double* psig, const double* plat, int64_t npts,
                                       const double* sxyz, const double* ssig, const double* slat_sorted, int64_t nsrc, const double* W,
                                       int64_t nfun, int64_t ldw, double g, double* out, int64_t ldo) {
    ARG_CHECK(h && pxyz && psig && sxyz && ssig && W && out);
    ARG_CHECK(nfun >= 1 && nfun <= 64 && npts >= 1 && nsrc >= 1 && nsrc < (int64_t)INT32_MAX && ldw >= nsrc && ldo >= npts && g >= 0.0);
    const double win = lat_window_deg(h->corr, g);
    if (!(win < 180.0) || !plat || !slat_sorted) { plat = nullptr; slat_sorted = nullptr; }
    const int64_t gx = cdiv(npts, 256);
    ARG_CHECK(gx < (int64_t)INT32_MAX);
    OISAT_LAUNCH_CORR(h, "functional_gather", functional_gather_kernel, kFunGroup, dim3((unsigned)gx), dim3(256), 0, pxyz, psig, plat, npts,
                      sxyz, ssig, slat_sorted, nsrc, W, (int)nfun, ldw, corr_scale(h->corr, g), win, cut_chord_of(h->corr, g), out, ldo);
    return OISAT_OK;
}

extern "C" int oisat_rows_dot(oisat_ctx* h, const double* A, int64_t lda, int64_t na, const double* B, int64_t ldb, int64_t nb, int64_t len,
                              double* out) {
    ARG_CHECK(h && A && B && out);
    ARG_CHECK(na >= 1 && na <= 64 && nb >= 1 && nb <= 64 && len >= 1 && lda >= len && ldb >= len);
    OISAT_LAUNCH(h, "rows_dot", rows_dot_kernel, dim3((unsigned)na, (unsigned)cdiv(nb, kDotGroup)), dim3(256), 0, A, lda, B, ldb, (int)nb, len,
                 out);
    return OISAT_OK;
}
