// Buddy sums of the normalised innovations (quality control ahead of the dense analyses): for every
// used observation a, over the used b != a in ascending b whose correlation c = C(|p_a - p_b|^2; g) is at least cmin,
//     n_a += 1, W_a += c, t = c u_b, P_a += t, Q_a += t u_b.
// The reference has no counterpart (its analysis is element-wise: a bad retrieval stays in its cell).  The pass has the shape of
// the covariogram's (variogram.hip): 256 rows per workgroup, one per lane, columns through LDS in chunks of 256, the latitude
// window of the float64 residual in front -- but it visits both halves of the pair matrix and its sums belong to the rows.
//
// DETERMINISM: a row's four accumulators live in ONE lane's registers and that lane takes the columns in ascending order, from
// the window's start to its end; the rows are not split over workgroups.  A column that is skipped -- by the window, by the
// test of the squared chord, or because c < cmin -- adds nothing, so the order of the additions that do happen is the
// ascending order of the contributing b whatever the window and the chunking: the same bits on every run, with and without
// olat_sorted.  No atomics, no workspace.  Built with the exact flags (-ffp-contract=off): d2 = dx dx + dy dy + dz dz, left to
// right, and c by corr_f64<KIND>, the function behind oisat_corr_eval.
#include "oisat_common.h"
#include "dense_switches.h"                                     // for dense_solve_dev.inc, which sits inside the namespace below

namespace {

#include "dense_solve_dev.inc"

constexpr int kBdRows = 256;                     // rows of a workgroup, one per lane; also the columns of a chunk
constexpr int64_t kBdMaxObs = (int64_t)1 << 20;

// blockIdx.x = block of 256 rows.  a = corr_scale(KIND, g).  lim2: a pair with d2 > lim2 has c < cmin for certain (the host's
// margin, oisat_buddy_sums).  olat (ascending, or nullptr): the columns are [first latitude >= olat[r0] - win_deg, first
// latitude >= olat[r1] + win_deg), r0 / r1 the block's first / last row, 1e-9 deg of slack on either side.
template <int KIND>
__global__ __launch_bounds__(256) void buddy_sums_kernel(const double* __restrict__ oxyz, const double* __restrict__ u, int64_t m,
                                                          double a, double cmin, double lim2, const double* __restrict__ olat,
                                                          double win_deg, int32_t* __restrict__ n_out, double* __restrict__ sums_out) {
    __shared__ double4 s_col[kBdRows];                       // x, y, z, u of the staged columns
    __shared__ int64_t s_j[2];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBdRows, row = r0 + t;
    if (t == 0) {
        int64_t j0 = 0, j1 = m;
        if (olat != nullptr) {
            const int64_t r1 = r0 + kBdRows - 1 < m - 1 ? r0 + kBdRows - 1 : m - 1;
            j0 = lower_bound_lat(olat, m, olat[r0] - win_deg - 1e-9);
            j1 = lower_bound_lat(olat, m, olat[r1] + win_deg + 1e-9);
        }
        s_j[0] = j0;
        s_j[1] = j1;
    }
    double xa = 0.0, ya = 0.0, za = 0.0, ua = nan_of<double>();
    if (row < m) {
        xa = oxyz[row];
        ya = oxyz[m + row];
        za = oxyz[2 * m + row];
        ua = u[row];
    }
    const bool used = fabs(ua) <= 1.7976931348623157e308;   // finite (false for NaN)
    int32_t n = 0;
    double W = 0.0, P = 0.0, Q = 0.0;
    __syncthreads();
    const int64_t j0 = s_j[0], j1 = s_j[1];
    for (int64_t c0 = j0; c0 < j1; c0 += kBdRows) {
        const int64_t c = c0 + t;
        double4 col = make_double4(0.0, 0.0, 0.0, nan_of<double>());
        if (c < j1) col = make_double4(oxyz[c], oxyz[m + c], oxyz[2 * m + c], u[c]);
        if (!(fabs(col.w) <= 1.7976931348623157e308)) col.w = nan_of<double>();
        s_col[t] = col;
        __syncthreads();
        if (used) {
            const int ncol = (int)(j1 - c0 < kBdRows ? j1 - c0 : kBdRows);
            for (int jj = 0; jj < ncol; ++jj) {
                const double4 b = s_col[jj];                  // (one address per wave: a broadcast)
                if (c0 + jj == row || !(b.w == b.w)) continue;
                const double dx = xa - b.x, dy = ya - b.y, dz = za - b.z;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 <= lim2)) continue;
                const double cc = corr_f64<KIND>(a, d2);
                if (cc >= cmin) {
                    const double tt = cc * b.w;
                    n += 1;
                    W += cc;
                    P += tt;
                    Q += tt * b.w;
                }
            }
        }
        __syncthreads();
    }
    if (row < m) {
        n_out[row] = n;
        sums_out[row] = W;
        sums_out[m + row] = P;
        sums_out[2 * m + row] = Q;
    }
}

}  // namespace

extern "C" int oisat_buddy_sums(oisat_ctx* h, const double* oxyz, const double* u, int64_t m, double g, double cmin,
                                const double* olat_sorted, int32_t* n_out, double* sums_out) {
    ARG_CHECK(h != nullptr);
    ARG_CHECK(m >= 0 && m <= kBdMaxObs);
    ARG_CHECK(g > 0.0 && std::isfinite(g));
    ARG_CHECK(cmin >= 9.5367431640625e-07 && cmin < 1.0);    // 2^-20 <= cmin < 1 (false for NaN)
    ARG_CHECK(m == 0 || (oxyz && u && n_out && sums_out));
    if (m == 0) return OISAT_OK;
    const int kind = h->corr;
    // The chord at which C has fallen to cmin, the upper end of its bracket (cut_chord), and the margin of the kernel's test of
    // the squared chord: 1e-9 relative moves g d2 by 1e-9 |ln cmin|, the absolute term by 1e-15 where cmin is so near 1 that
    // this is less -- either way more than the rounding of c (a few 2^-53 (1 + |ln cmin|)), so a pair beyond lim2 has c < cmin
    // as the device rounds it.  The window's angle is that of sqrt(lim2): it skips nothing the test would not.
    const double chord = cut_chord(kind, g, -log2(cmin));
    const double lim2 = chord * chord * (1.0 + 1e-9) + 1e-15 / g;
    const double lim = sqrt(lim2);
    const double win = lim >= 2.0 ? 1e9 : 2.0 * asin(0.5 * lim) * 57.29577951308232;
    const double* olat = win < 180.0 ? olat_sorted : (const double*)nullptr;
    const dim3 grid((unsigned)cdiv(m, kBdRows)), block(256);
    const double a = corr_scale(kind, g);
    if (kind == OISAT_CORR_GASPARI_COHN) {
        OISAT_LAUNCH(h, "buddy_sums", buddy_sums_kernel<OISAT_CORR_GASPARI_COHN>, grid, block, 0, oxyz, u, m, a, cmin, lim2, olat, win,
                     n_out, sums_out);
    } else if (kind == OISAT_CORR_SOAR) {
        OISAT_LAUNCH(h, "buddy_sums", buddy_sums_kernel<OISAT_CORR_SOAR>, grid, block, 0, oxyz, u, m, a, cmin, lim2, olat, win, n_out,
                     sums_out);
    } else {
        OISAT_LAUNCH(h, "buddy_sums", buddy_sums_kernel<OISAT_CORR_GAUSSIAN>, grid, block, 0, oxyz, u, m, a, cmin, lim2, olat, win, n_out,
                     sums_out);
    }
    return OISAT_OK;
}
