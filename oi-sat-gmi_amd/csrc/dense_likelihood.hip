// The likelihood of the innovations under the dense analysis' own model:
//     -2 ln p(d) = m ln 2 pi + log det S + d^T S^-1 d,    S = H B H^T + R = L L^T,
// so log det S = 2 sum_a log L_aa is one reduction over the diagonal of the factor an analysis leaves in HBM, and chi^2 = d^T z
// is oisat_rows_dot of the innovation with the refined solution.  This unit holds the reduction, oisat_factor_logdet.  The sum of
// m logarithms is compared between error scales whose log-determinants differ by O(1) out of O(m), so everything is float64: the
// logarithm of the widened float, then a fixed tree.  (No reference counterpart: the element-wise OI has no likelihood.)
#include "oisat_common.h"

namespace {

// One workgroup of 1024 threads.  Thread t reads the diagonal entries a = t, t + 1024, .. < m -- never one at or beyond m: those
// are the identity padding of the last block and whatever lies in a gutter -- four at a time into four partial sums (entry
// number i of the thread goes to sum i mod 4), joined as (0 + 1) + (2 + 3); the 64 lanes of a wave by the butterfly; the 16
// waves pairwise, ((0 + 1) + (2 + 3)) + .. .  The tree depends on m alone: one workgroup, no atomics, nothing that the CU count
// or timing could reorder.  A lane without an entry adds an exact zero.  The minimum takes the same route (fmin is exact).
constexpr int kLogdetThreads = 1024;
__global__ __launch_bounds__(kLogdetThreads) void factor_logdet_kernel(const float* __restrict__ L, int64_t m, int64_t ld,
                                                                        double* __restrict__ out) {
    __shared__ double red_s[kLogdetThreads / kWave], red_m[kLogdetThreads / kWave];
    __shared__ int red_b[kLogdetThreads / kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double lo = (double)INFINITY;
    int bad = 0;
    for (int64_t a0 = t; a0 < m; a0 += 4 * kLogdetThreads) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                           // the four loads first: one cache line each
            const int64_t a = a0 + (int64_t)q * kLogdetThreads;
            v[q] = a < m ? L[a * ld + a] : 1.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (a0 + (int64_t)q * kLogdetThreads < m) {
                const double x = (double)v[q];
                bad |= !(x > 0.0 && x < (double)INFINITY);      // zero, negative, infinite or NaN
                lo = fmin(lo, x);
                acc[q] += 2.0 * log(x);
            }
        }
    }
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        lo = fmin(lo, __shfl_xor(lo, o, kWave));
        bad |= __shfl_xor(bad, o, kWave);
    }
    if (lane == 0) { red_s[w] = s; red_m[w] = lo; red_b[w] = bad; }
    __syncthreads();
    if (t == 0) {
        constexpr int W = kLogdetThreads / kWave;
        for (int width = W / 2; width >= 1; width >>= 1)        // (0 + 1), (2 + 3), ..: neighbours first
            for (int i = 0; i < width; ++i) {
                red_s[i] = red_s[2 * i] + red_s[2 * i + 1];
                red_m[i] = fmin(red_m[2 * i], red_m[2 * i + 1]);
                red_b[i] = red_b[2 * i] | red_b[2 * i + 1];
            }
        out[0] = red_b[0] ? nan_of<double>() : red_s[0];
        out[1] = red_m[0];
    }
}

}  // namespace

extern "C" int oisat_factor_logdet(oisat_ctx* h, const float* L, int64_t m, int64_t ld, double* out) {
    ARG_CHECK(h && L && out);
    ARG_CHECK(m >= 1 && ld >= cdiv(m, 128) * 128);
    OISAT_LAUNCH(h, "factor_logdet", factor_logdet_kernel, dim3(1), dim3(kLogdetThreads), 0, L, m, ld, out);
    return OISAT_OK;
}
