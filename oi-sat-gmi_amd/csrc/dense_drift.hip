// A drift of the innovations: universal kriging, d = F beta + e, e ~ N(0, S), beta with a flat prior.
//     beta = M^-1 F^T S^-1 d,   M = F^T S^-1 F,   z' = S^-1 (d - F beta),   x_a = x_b + B H^T z' + f(x)^T beta,
// and the unknown beta adds q^T M^-1 q to the analysis error variance of a cell, q = f(x) - F^T S^-1 H B e_x.  F: p = (degree + 1)^2
// real harmonics up to `degree` as polynomials of the unit vector.  Everything but beta lives in the factor a run left behind;
// this unit adds the basis (oisat_drift_basis, and the same expressions inside oisat_drift_apply and oisat_drift_quadform), the
// float64 residual of a BLOCK of right-hand sides in one pass over the pairs (oisat_cov_residual_multi: one evaluation of the
// correlation serves every column) and the refined solve of such a block (oisat_gain_solve_multi: the sweeps are the row sweeps
// of dense_post.hip on an fp32 panel, i.e. GEMMs).  The host part (the p x p system, z', chi^2) is oisatgmi/dense.py.
// (No reference counterpart: the element-wise OI corrects offsets and slopes ahead of the analysis, per instrument.)
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_solve_dev.inc"

constexpr int kDriftMaxP = 16;                                 // (3 + 1)^2
constexpr int kMultiMaxRhs = 17;                               // the innovation and 16 basis columns
constexpr int kPanelRows = 128;                                // rows of the fp32 panel (oisat_trsm_rows: a multiple of 128)
constexpr int kMultiWs = 13;                                   // the handle's workspace slot: state | fp32 panel | residual block

// ---- the basis ---------------------------------------------------------------------------------------------------------------
// Real harmonics up to degree 3 as polynomials of (x, y, z), unnormalised, in the order of include/oisat.h.  One rounding per
// operation, in exactly the order written: every product that feeds a sum -- inside an expression, or as a value f[j] that a caller
// adds to or subtracts from (drift_quadform_kernel's f_j - Q_j) -- passes through rounded(), which hides it from the optimiser, so
// that the unit's -ffp-contract=fast (a back-end rule: a pragma does not reach it) cannot fuse it into the sum.  The
// same inputs give the same bits here, in a NumPy restatement and in each of the three kernels that call it.  f[j],
// j >= (degree + 1)^2, are not written.
__device__ __forceinline__ double rounded(double v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ void drift_basis_at(double x, double y, double z, int degree, double* __restrict__ f) {
    f[0] = 1.0;
    if (degree < 1) return;
    f[1] = x;
    f[2] = y;
    f[3] = z;
    if (degree < 2) return;
    const double xx = rounded(x * x), yy = rounded(y * y), zz = rounded(z * z), xy = rounded(x * y);
    f[4] = xy;
    f[5] = rounded(y * z);
    f[6] = rounded(z * x);
    f[7] = xx - yy;
    f[8] = rounded(3.0 * zz) - 1.0;
    if (degree < 3) return;
    const double t = rounded(5.0 * zz);
    f[9] = rounded(z * (t - 3.0));
    f[10] = rounded(x * (t - 1.0));
    f[11] = rounded(y * (t - 1.0));
    f[12] = rounded(z * (xx - yy));
    f[13] = rounded(xy * z);
    f[14] = rounded(x * (xx - rounded(3.0 * yy)));
    f[15] = rounded(y * (rounded(3.0 * xx) - yy));
}

// out[j][i] = f_j(p_i), i < npts; 0 for npts <= i < ld.  One thread per column i of out.
__global__ __launch_bounds__(256) void drift_basis_kernel(const double* __restrict__ pxyz, int64_t npts, int degree, double* __restrict__ out,
                                                           int64_t ld) {
    const int p = (degree + 1) * (degree + 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += stride) {
        double f[kDriftMaxP];
#pragma unroll
        for (int j = 0; j < kDriftMaxP; ++j) f[j] = 0.0;
        if (i < npts) drift_basis_at(pxyz[i], pxyz[npts + i], pxyz[2 * npts + i], degree, f);
#pragma unroll
        for (int j = 0; j < kDriftMaxP; ++j)
            if (j < p) out[(int64_t)j * ld + i] = f[j];
    }
}

// x_i, inc_i += sum_j beta_j f_j(x_i): the sum in double (fused multiply-adds in the order of j, from 0), added to the widened
// field value in double and rounded once to T
template <typename T>
__global__ __launch_bounds__(256) void drift_apply_kernel(const double* __restrict__ gxyz, int64_t n, int degree, const double* __restrict__ beta,
                                                           T* __restrict__ x, T* __restrict__ inc) {
    __shared__ double sb[kDriftMaxP];
    const int p = (degree + 1) * (degree + 1);
    if ((int)threadIdx.x < kDriftMaxP) sb[threadIdx.x] = (int)threadIdx.x < p ? beta[threadIdx.x] : 0.0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double f[kDriftMaxP];
#pragma unroll
        for (int j = 0; j < kDriftMaxP; ++j) f[j] = 0.0;
        drift_basis_at(gxyz[i], gxyz[n + i], gxyz[2 * n + i], degree, f);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kDriftMaxP; ++j) s = __builtin_fma(sb[j], f[j], s);
        if (x != nullptr) x[i] = (T)((double)x[i] + s);
        if (inc != nullptr) inc[i] = (T)((double)inc[i] + s);
    }
}

// var[i] = q^T Minv q, q_j = f_j(x_i) - Q[j][i]: t_j = sum_k Minv[j][k] q_k (k ascending), var = sum_j q_j t_j (j ascending), fused
// multiply-adds in double.  Minv sits in LDS and is read at wave-uniform addresses.
__global__ __launch_bounds__(256) void drift_quadform_kernel(const double* __restrict__ gxyz, int64_t n, int degree, const double* __restrict__ Q,
                                                              int64_t ldq, const double* __restrict__ Minv, double* __restrict__ var) {
    __shared__ double sm[kDriftMaxP * kDriftMaxP];
    const int p = (degree + 1) * (degree + 1);
    {                                                           // Minv, padded with zeros to 16 x 16
        const int j = threadIdx.x >> 4, k = threadIdx.x & 15;
        sm[threadIdx.x] = j < p && k < p ? Minv[j * p + k] : 0.0;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one cell per thread: Minv is read as it is used
    if (i >= n) return;
    double q[kDriftMaxP];
#pragma unroll
    for (int j = 0; j < kDriftMaxP; ++j) q[j] = 0.0;
    drift_basis_at(gxyz[i], gxyz[n + i], gxyz[2 * n + i], degree, q);
#pragma unroll
    for (int j = 0; j < kDriftMaxP; ++j) q[j] = j < p ? q[j] - Q[(int64_t)j * ldq + i] : 0.0;
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < kDriftMaxP; ++j) {
        double tj = 0.0;
#pragma unroll
        for (int k = 0; k < kDriftMaxP; ++k) tj = __builtin_fma(sm[j * kDriftMaxP + k], q[k], tj);
        v = __builtin_fma(q[j], tj, v);
    }
    var[i] = v;
}

// ---- R[k] = D[k] - (C o sig sig^T + diag(var)) Z[k], k < nrhs, in one pass over the pairs ------------------------------------
// A workgroup = 64 rows x 4 column phases, as in the single residual (dense_solve_dev.inc): the rows are 64 consecutive entries
// of the latitude order or, with a block list, of `perm` (neighbours in space), whose latitude span gives the candidate range
// and, with a list, whose bounding sphere culls the candidates at the library's 2^-52 chord while they are staged in LDS (double
// coordinates + index, in candidate order: wave ballots).  The staged candidates pass in sub-chunks of 64 whose weights
// sig_j Z[k][j] are gathered into an LDS image, [64][G] doubles; phase ph takes the entries ph, ph + 4, .. of a sub-chunk, and
// ONE evaluation of the correlation (15 of the pair's 24 instructions) serves G fused multiply-adds into G
// double sums.  The image is read at wave-uniform addresses, 16 bytes a time (a broadcast: no bank conflict, LDS traffic of
// 8 G bytes per pair and WAVE, not per lane), so a thread carrying all columns costs registers, not LDS: G = 18 is 36 VGPRs of
// sums, and the kernel stays under 128 (four waves per SIMD; LDS 26 KB: six workgroups per CU).  Two instantiations: G = 6 (up
// to degree 1 plus the innovation) and G = 18; a column k >= nrhs has weight 0 in the image and no row of D, Z or R beyond
// nrhs - 1 is touched.  Fixed order everywhere: candidates in latitude order, the phases joined as ((0 + 1) + 2) + 3.
constexpr int kMrStage = 512;                                  // staged candidates: processed once 256 have gathered
constexpr int kMrSub = 64;                                     // candidates per weight image
template <int KIND, int G>
__global__ __launch_bounds__(256) void cov_residual_multi_kernel(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                                  const double* __restrict__ ovar, int64_t m, double a,
                                                                  const double* __restrict__ D, const double* __restrict__ Z,
                                                                  double* __restrict__ R, int nrhs, int64_t ld,
                                                                  const double* __restrict__ olat, double win_deg,
                                                                  const int* __restrict__ perm, double cut_chord) {
    static_assert(G % 2 == 0, "the image rows are read as 16-byte words");
    __shared__ double sx[kMrStage], sy[kMrStage], sz[kMrStage];
    __shared__ int sidx[kMrStage];
    __shared__ __attribute__((aligned(16))) double sw[kMrSub * G];
    __shared__ double part[4][64];
    __shared__ double red[16], s_lo, s_hi;
    __shared__ int wcnt[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;      // w = the column phase, lane = the row of the block
    const int64_t pos = (int64_t)blockIdx.x * 64 + lane;
    const bool live = pos < m;
    const int64_t row = live ? (perm ? (int64_t)perm[pos] : pos) : 0;
    const double ax = live ? oxyz[row] : 0.0, ay = live ? oxyz[m + row] : 0.0, az = live ? oxyz[2 * m + row] : 0.0;
    int64_t j0 = 0, j1 = m;
    if (olat != nullptr) {                                      // latitude span of the block's rows -> candidate range
        if (w == 0) {
            double lo = live ? olat[row] : 1e9, hi = live ? olat[row] : -1e9;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
            if (lane == 0) { s_lo = lo; s_hi = hi; }
        }
        __syncthreads();
        j0 = lower_bound_lat(olat, m, s_lo - win_deg);
        j1 = lower_bound_lat(olat, m, s_hi + win_deg + 1e-9);
    }
    const double px[1] = {ax}, py[1] = {ay}, pz[1] = {az};
    const bool lv[1] = {live && w == 0};
    const BlockSphere bs = block_sphere<1>(px, py, pz, lv, perm != nullptr ? cut_chord : 1e30, (double)INFINITY, red);
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
                x = oxyz[c]; y = oxyz[m + c]; zz = oxyz[2 * m + c];
                const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
                keep = dx * dx + dy * dy + dz * dz <= bs.r2cull;
            }
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) wcnt[w] = __popcll(mask);
            __syncthreads();
            const int c0w = wcnt[0], c1w = wcnt[1], c2w = wcnt[2], c3w = wcnt[3];
            if (keep) {
                const int q = fill + (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0) + __popcll(mask & ((1ull << lane) - 1ull));
                sx[q] = x; sy[q] = y; sz[q] = zz;
                sidx[q] = (int)c;
            }
            __syncthreads();
            fill += c0w + c1w + c2w + c3w;                      // (at most 255 + 256 entries ever wait: kMrStage)
        }
        if (fill < 256 && c0 + 256 < j1) continue;              // (block-uniform)
        for (int s0 = 0; s0 < fill; s0 += kMrSub) {
            const int cnt = fill - s0 < kMrSub ? fill - s0 : kMrSub;
            if (lane < cnt) {                                   // weights: wave w takes the columns w, w + 4, ..; a lane one candidate
                const int j = sidx[s0 + lane];
                const double so = osig[j];
                for (int kk = w; kk < G; kk += 4) sw[lane * G + kk] = kk < nrhs ? so * Z[(int64_t)kk * ld + j] : 0.0;
            }
            __syncthreads();
            for (int o = w; o < cnt; o += 4) {
                const double dx = ax - sx[s0 + o], dy = ay - sy[s0 + o], dz = az - sz[s0 + o];
                const double c = corr_f64<KIND>(a, dx * dx + dy * dy + dz * dz);
#pragma unroll
                for (int kk = 0; kk < G; kk += 2) {
                    const double2 wv = *reinterpret_cast<const double2*>(&sw[o * G + kk]);
                    acc[kk] = __builtin_fma(c, wv.x, acc[kk]);
                    acc[kk + 1] = __builtin_fma(c, wv.y, acc[kk + 1]);
                }
            }
            __syncthreads();
        }
        fill = 0;
    }
    const double sg = live ? osig[row] : 0.0, vr = live ? ovar[row] : 0.0;
#pragma unroll
    for (int kk = 0; kk < G; ++kk) {
        if (kk < nrhs) {                                        // (block-uniform: every thread meets every barrier)
            part[w][lane] = acc[kk];
            __syncthreads();
            if (w == 0 && live) {
                const double s = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
                const int64_t e = (int64_t)kk * ld + row;
                R[e] = D[e] - (sg * s + vr * Z[e]);
            }
            __syncthreads();
        }
    }
}

// ---- the refined solve of a block of right-hand sides ------------------------------------------------------------------------
// state of one oisat_gain_solve_multi on the device (head of workspace slot kMultiWs)
struct MultiState {
    double dd[kMultiMaxRhs];                                   // |d_k|^2
    double norm[9][kMultiMaxRhs];                              // |r_k|^2 of evaluation it = 0 .. refine <= 8
    int conv[kMultiMaxRhs];                                    // set when |r_k| <= tol |d_k|: the column takes zero corrections from then on
    int computed[kMultiMaxRhs];                                // norms stored for column k
    int nconv;                                                 // columns that have converged
};
constexpr size_t kMultiStateBytes = 4096;
static_assert(sizeof(MultiState) <= kMultiStateBytes, "MultiState outgrew its slot");

// sum of v[i]^2, i < m, by one workgroup of 1024 threads in the fixed order of resid_check_kernel (dense_solve.hip)
__device__ __forceinline__ double multi_sumsq(const double* __restrict__ v, int64_t m, double* __restrict__ sh /*[1024] shared*/) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 1024) s += v[i] * v[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int q = 512; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) sh[threadIdx.x] += sh[threadIdx.x + q];
        __syncthreads();
    }
    return sh[0];
}

// blockIdx.x = column k: |d_k|^2, and the column's state reset (block 0 resets the count)
__global__ __launch_bounds__(1024) void multi_prep_kernel(const double* __restrict__ D, int64_t m, int64_t ld, MultiState* __restrict__ st) {
    __shared__ double sh[1024];
    const int k = blockIdx.x;
    const double dd = multi_sumsq(D + (int64_t)k * ld, m, sh);
    if (threadIdx.x == 0) {
        st->dd[k] = dd;
        st->conv[k] = 0;
        st->computed[k] = 0;
        if (k == 0) st->nconv = 0;
    }
}

// X[k][j] = (float)(src[k][j] / |d_k|) for j < m (0 for a converged column, and where |d_k| = 0), 0 for m <= j < ldx; the rows
// nrhs <= k < rows are zeros.  rows = 128 in front of the first sweeps, nrhs later: a zero row stays zero through the sweeps.
__global__ __launch_bounds__(256) void multi_narrow_kernel(const double* __restrict__ src, int64_t m, int64_t ld, int nrhs, int rows,
                                                            const MultiState* __restrict__ st, float* __restrict__ X, int64_t ldx) {
    const int k = blockIdx.y;
    if (k >= rows) return;
    double inv = 0.0;
    if (k < nrhs && st->conv[k] == 0 && st->dd[k] > 0.0) inv = 1.0 / sqrt(st->dd[k]);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ldx; j += stride)
        X[(int64_t)k * ldx + j] = inv != 0.0 && j < m ? (float)(src[(int64_t)k * ld + j] * inv) : 0.0f;
}

// Z[k][j] (+)= |d_k| (double)X[k][j], j < m
__global__ __launch_bounds__(256) void multi_accum_kernel(const float* __restrict__ X, int64_t ldx, int64_t m, int64_t ld, int accumulate,
                                                           const MultiState* __restrict__ st, double* __restrict__ Z) {
    const int k = blockIdx.y;
    const double nrm = sqrt(st->dd[k]);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const double dz = nrm * (double)X[(int64_t)k * ldx + j];
        Z[(int64_t)k * ld + j] = accumulate ? Z[(int64_t)k * ld + j] + dz : dz;
    }
}

// blockIdx.x = column k: |r_k|^2 of evaluation `it`, the convergence flag, and -- final: behind the last allowed correction --
// the handle's status word for a column that is still above its tolerance (tol2 = 0, "run every round", never counts)
__global__ __launch_bounds__(1024) void multi_check_kernel(const double* __restrict__ R, int64_t m, int64_t ld, int it, double tol2,
                                                            MultiState* __restrict__ st, int final, int* __restrict__ info) {
    __shared__ double sh[1024];
    const int k = blockIdx.x;
    if (st->conv[k] != 0) return;                               // (block-uniform)
    const double rr = multi_sumsq(R + (int64_t)k * ld, m, sh);
    if (threadIdx.x == 0) {
        st->norm[it][k] = rr;
        st->computed[k] = it + 1;
        if (rr <= tol2 * st->dd[k]) {
            st->conv[k] = 1;
            atomicAdd(&st->nconv, 1);
        } else if (final && tol2 > 0.0) {
            atomicAdd(&info[kInfoUnconverged], 1);
        }
    }
}

int residual_multi_launch(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g, const double* D,
                          const double* Z, double* R, int64_t nrhs, int64_t ld, const double* olat_sorted, const int* perm) {
    ARG_CHECK(h && oxyz && osig && ovar && D && Z && R);
    ARG_CHECK(m >= 1 && m < (int64_t)INT32_MAX && nrhs >= 1 && nrhs <= kMultiMaxRhs && ld >= m && g >= 0.0);
    {   // R_out must not overlap D or Z
        const char *r0 = (const char*)R, *r1 = r0 + sizeof(double) * ((nrhs - 1) * ld + m);
        const char *d0 = (const char*)D, *z0 = (const char*)Z;
        const size_t span = sizeof(double) * ((nrhs - 1) * ld + m);
        ARG_CHECK((d0 + span <= r0 || r1 <= d0) && (z0 + span <= r0 || r1 <= z0));
    }
    const int kind = h->corr;
    const double win = lat_window_deg(kind, g);
    if (!(win < 180.0)) olat_sorted = nullptr;
    if (!olat_sorted || !residual_blocks_pay(kind, g)) perm = nullptr;      // the single residual's rule for the block list
    const dim3 grid((unsigned)cdiv(m, 64));
    if (nrhs <= 6) {
        OISAT_LAUNCH_CORR(h, "cov_residual_multi", cov_residual_multi_kernel, 6, grid, dim3(256), 0, oxyz, osig, ovar, m, corr_scale(kind, g), D, Z,
                          R, (int)nrhs, ld, olat_sorted, win, perm, cut_chord_of(kind, g));
    } else {
        OISAT_LAUNCH_CORR(h, "cov_residual_multi", cov_residual_multi_kernel, 18, grid, dim3(256), 0, oxyz, osig, ovar, m, corr_scale(kind, g), D,
                          Z, R, (int)nrhs, ld, olat_sorted, win, perm, cut_chord_of(kind, g));
    }
    return OISAT_OK;
}

}  // namespace

extern "C" int oisat_drift_basis(oisat_ctx* h, const double* pxyz, int64_t npts, int degree, double* out, int64_t ld) {
    ARG_CHECK(h && pxyz && out);
    ARG_CHECK(degree >= 0 && degree <= 3 && npts >= 1 && ld >= npts);
    OISAT_LAUNCH(h, "drift_basis", drift_basis_kernel, dim3(stream_grid(ld, 256)), dim3(256), 0, pxyz, npts, degree, out, ld);
    return OISAT_OK;
}

extern "C" int oisat_drift_apply(oisat_ctx* h, int dtype, const double* gxyz, int64_t n, int degree, const double* beta, void* x_inout,
                                 void* inc_inout) {
    ARG_CHECK(h && gxyz && beta && (x_inout || inc_inout));
    ARG_CHECK(degree >= 0 && degree <= 3 && n >= 1);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    const dim3 grid(stream_grid(n, 256));
    if (dtype == OISAT_F32) {
        OISAT_LAUNCH(h, "drift_apply", drift_apply_kernel<float>, grid, dim3(256), 0, gxyz, n, degree, beta, (float*)x_inout, (float*)inc_inout);
    } else {
        OISAT_LAUNCH(h, "drift_apply", drift_apply_kernel<double>, grid, dim3(256), 0, gxyz, n, degree, beta, (double*)x_inout, (double*)inc_inout);
    }
    return OISAT_OK;
}

extern "C" int oisat_drift_quadform(oisat_ctx* h, const double* gxyz, int64_t n, int degree, const double* Q, int64_t ldq, const double* Minv,
                                    double* var_out) {
    ARG_CHECK(h && gxyz && Q && Minv && var_out);
    ARG_CHECK(degree >= 0 && degree <= 3 && n >= 1 && ldq >= n && cdiv(n, 256) < (int64_t)INT32_MAX);
    OISAT_LAUNCH(h, "drift_quadform", drift_quadform_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, gxyz, n, degree, Q, ldq, Minv, var_out);
    return OISAT_OK;
}

extern "C" int oisat_cov_residual_multi(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                        const double* D, const double* Z, double* R_out, int64_t nrhs, int64_t ld, const double* olat_sorted) {
    ARG_CHECK(h != nullptr);
    const int* perm = oisat_take_obs_perm(h, m);                // one-shot, whatever this call's outcome
    return residual_multi_launch(h, oxyz, osig, ovar, m, g, D, Z, R_out, nrhs, ld, olat_sorted, perm);
}

extern "C" int oisat_gain_solve_multi(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                                      int64_t ldl, double g, const double* D, int64_t nrhs, int64_t ld, int refine, double* Z_out,
                                      double* resid_host, const double* olat_sorted) {
    ARG_CHECK(h != nullptr);
    const int* perm = oisat_take_obs_perm(h, m);                // one-shot, whatever this call's outcome
    h->factor.fwd_d = nullptr;                                  // (a forward vector left by the factorization launch is not used here)
    ARG_CHECK(L && oxyz && osig && ovar && D && Z_out && m > 0 && refine >= 0 && refine <= 8);
    ARG_CHECK(nrhs >= 1 && nrhs <= kMultiMaxRhs && ld >= m && m < (int64_t)INT32_MAX && g >= 0.0);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ldl);
    {   // Z_out must not overlap D
        const size_t span = sizeof(double) * ((nrhs - 1) * ld + m);
        const char *d0 = (const char*)D, *z0 = (const char*)Z_out;
        ARG_CHECK(d0 + span <= z0 || z0 + span <= d0);
    }
    const double tol = h->refine_tol;
    const int64_t mp = h->factor.mp, ldx = mp;
    const size_t panel_bytes = sizeof(float) * kPanelRows * ldx, resid_bytes = sizeof(double) * nrhs * ld;
    char* ws = (char*)oisat_ws(h, kMultiWs, kMultiStateBytes + panel_bytes + resid_bytes);
    if (!ws) return OISAT_ENOMEM;
    MultiState* st = (MultiState*)ws;
    float* X = (float*)(ws + kMultiStateBytes);
    double* R = (double*)(ws + kMultiStateBytes + panel_bytes);
    int* info_dev = nullptr;
    if (int rs = status_ws(h, &info_dev, nullptr)) return rs;
    char* pin = nullptr;
    if (resid_host) {
        pin = (char*)oisat_pinned(h, kMultiStateBytes + 256);
        if (!pin) return OISAT_ENOMEM;
    }
    const unsigned gx = (unsigned)stream_grid(ldx, 256);
    OISAT_LAUNCH(h, "multi_prep", multi_prep_kernel, dim3((unsigned)nrhs), dim3(1024), 0, D, m, ld, st);
    OISAT_LAUNCH(h, "multi_narrow", multi_narrow_kernel, dim3(gx, kPanelRows), dim3(256), 0, D, m, ld, (int)nrhs, kPanelRows,
                 (const MultiState*)st, X, ldx);
    int rc = oisat_trsm_rows(h, L, m, ldl, X, kPanelRows, ldx);
    if (rc) return rc;
    rc = oisat_trsm_rows_bwd(h, L, m, ldl, X, kPanelRows, ldx);
    if (rc) return rc;
    OISAT_LAUNCH(h, "multi_accum", multi_accum_kernel, dim3(gx, (unsigned)nrhs), dim3(256), 0, (const float*)X, ldx, m, ld, 0, (const MultiState*)st,
                 Z_out);
    // (refine = 0 asks for the plain solve: no residual is formed -- unless the caller wants it reported -- and nothing is flagged)
    for (int it = 0; it <= refine && (refine > 0 || resid_host); ++it) {
        rc = residual_multi_launch(h, oxyz, osig, ovar, m, g, D, Z_out, R, nrhs, ld, olat_sorted, perm);
        if (rc) return rc;
        OISAT_LAUNCH(h, "multi_check", multi_check_kernel, dim3((unsigned)nrhs), dim3(1024), 0, (const double*)R, m, ld, it, tol * tol, st,
                     it == refine && refine > 0 ? 1 : 0, info_dev);
        if (it == refine) break;
        if (resid_host) {                                       // this call synchronises anyway: rounds behind the last column's convergence are not enqueued
            HIP_TRY(hipMemcpyAsync(pin, st, sizeof(MultiState), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            if (((const MultiState*)pin)->nconv >= (int)nrhs) break;
        }
        OISAT_LAUNCH(h, "multi_narrow", multi_narrow_kernel, dim3(gx, (unsigned)nrhs), dim3(256), 0, (const double*)R, m, ld, (int)nrhs, (int)nrhs,
                     (const MultiState*)st, X, ldx);
        rc = oisat_trsm_rows(h, L, m, ldl, X, kPanelRows, ldx);
        if (rc) return rc;
        rc = oisat_trsm_rows_bwd(h, L, m, ldl, X, kPanelRows, ldx);
        if (rc) return rc;
        OISAT_LAUNCH(h, "multi_accum", multi_accum_kernel, dim3(gx, (unsigned)nrhs), dim3(256), 0, (const float*)X, ldx, m, ld, 1,
                     (const MultiState*)st, Z_out);
    }
    if (resid_host) {
        HIP_TRY(hipMemcpyAsync(pin, st, sizeof(MultiState), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const MultiState* hs = (const MultiState*)pin;
        for (int64_t k = 0; k < nrhs; ++k) {
            const double dn = hs->dd[k] > 0.0 ? sqrt(hs->dd[k]) : 1.0;
            for (int it = 0; it <= refine; ++it) {              // rounds that were skipped after convergence repeat the last residual
                const int q = it < hs->computed[k] ? it : hs->computed[k] - 1;
                resid_host[(int64_t)it * nrhs + k] = q >= 0 ? sqrt(hs->norm[q][k]) / dn : 0.0;
            }
        }
    }
    return OISAT_OK;
}
