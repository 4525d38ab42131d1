// Dense background-error covariance pieces of the north-star analysis
//     x_a = x_b + B H^T (H B H^T + R)^-1 (y - H x_b),   B = D^1/2 C D^1/2,
//     C(p,q) = exp(-g |p-q|^2),  g = R_earth^2 / (2 L^2),  p,q unit vectors on the sphere (the default model), or the
//     compactly supported Gaspari-Cohn function or the SOAR (Matern 3/2) function of the same g (oisat_set_correlation;
//     dense_solve_dev.inc: corr_f32 / corr_f64).
// The reference has no counterpart (its OI is the L->0, H=I limit: optimal_interpolation.py:27,
// :49-50).  Chord distance keeps C positive definite on the sphere; |p-q|^2 is formed from
// coordinate DIFFERENCES (not 2-2p.q) so that fp32 keeps ~1e-7 relative accuracy at small range.
//
// Nothing n x m is ever materialised: B H^T (415 GB at n=1,036,800, m=1e5) is generated tile by
// tile in registers from 3 floats per point, so these kernels are VALU/transcendental-bound
// (v_exp_f32 is quarter rate), not HBM-bound -- except cov_build, which writes S once (4 m^2 B).
#include "oisat_common.h"
#include "dense_switches.h"

#include <algorithm>

namespace {

#include "dense_solve_dev.inc"

// ---- S = sig sig^T .* C + diag(var), lower 64x64 tiles (diagonal tiles complete) ----------------
// ENV: first[mp/128] (device) is the block envelope of a latitude-sorted system (oisat_envelope).  A tile left of its row's
// envelope holds correlations below the library's cut-off only: it is not evaluated but filled with exact zeros, so that every
// reader of S or of its factor that does not know the envelope finds zeros there (never what an earlier system left).
// BAND (oisat_cov_build_env_zeroed): the grid is tile rows x the widest row's tiles instead of the whole triangle.  Row ti
// starts at the 128-column block from = min(first, zero_first) of its block row (zero_first = nullptr: 0): tiles in
// [from, first) are zero-filled, tiles from first on evaluated, and the caller vouches for the zeros left of `from`.
template <int KIND, bool ENV, bool BAND>
__global__ __launch_bounds__(256) void cov_build_kernel(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                         const double* __restrict__ ovar, int64_t m, int64_t mp, float g2,
                                                         float* __restrict__ S, int64_t ld, int ntile, const int* __restrict__ first,
                                                         const int* __restrict__ zero_first) {
    int ti, tj;
    if (BAND) {
        ti = (int)blockIdx.y;
        int from = first[ti >> 1];
        if (zero_first != nullptr) {
            const int zf = zero_first[ti >> 1];
            from = zf < from ? (zf < 0 ? 0 : zf) : from;
        } else {
            from = 0;
        }
        from = from < 0 ? 0 : from;
        tj = 2 * from + (int)blockIdx.x;
        if (tj > ti) return;                     // (block-uniform; tj >= 0: no table content moves a store out of the lower triangle)
    } else {
        // triangular tile index -> (ti >= tj)
        const int64_t b = blockIdx.x;
        ti = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
        while ((int64_t)ti * (ti + 1) / 2 > b) --ti;
        while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
        tj = (int)(b - (int64_t)ti * (ti + 1) / 2);
    }
    __shared__ float4 pa[64], pb[64];            // x, y, z, sig
    const int t = threadIdx.x;
    if (ENV && (tj >> 1) < first[ti >> 1]) {     // (block-uniform)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t grow = (int64_t)ti * 64 + (t >> 4) + rr * 16;
            if (grow < mp) *reinterpret_cast<float4*>(&S[grow * ld + (int64_t)tj * 64 + (t & 15) * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    if (t < 128) {
        const int64_t row = (t < 64 ? (int64_t)ti * 64 + t : (int64_t)tj * 64 + (t - 64));
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < m) v = make_float4((float)oxyz[row], (float)oxyz[m + row], (float)oxyz[2 * m + row], (float)osig[row]);
        if (t < 64) pa[t] = v; else pb[t - 64] = v;
    }
    __syncthreads();
    const int cx = (t & 15) * 4;                 // 4 consecutive columns -> one 16-byte store
    const int ry = t >> 4;                       // rows ry, ry+16, ry+32, ry+48
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = ry + rr * 16;
        const int64_t grow = (int64_t)ti * 64 + r;
        if (grow >= mp) continue;
        const float4 a = pa[r];
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 q = pb[cx + c];
            const int64_t gcol = (int64_t)tj * 64 + cx + c;
            const float dx = a.x - q.x, dy = a.y - q.y, dz = a.z - q.z;
            const float d2 = dx * dx + dy * dy + dz * dz;
            float v = a.w * q.w * corr_f32<KIND>(g2, d2);
            if (grow == gcol) v = grow < m ? (float)(osig[grow] * osig[grow] + ovar[grow]) : 1.0f;     // padding: identity
            else if (grow >= m || gcol >= m) v = 0.0f;
            o[c] = v;
        }
        *reinterpret_cast<float4*>(&S[grow * ld + (int64_t)tj * 64 + cx]) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void innovation_kernel(const T* __restrict__ xb, const int64_t* __restrict__ cell,
                                                          const double* __restrict__ y, int64_t m, double* __restrict__ d) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) d[a] = y[a] - (double)xb[cell[a]];
}

// LDS of the solve-phase kernels below: one carve-out per workgroup (dense_solve_dev.inc)
#define SOLVE_LDS(W)                                                                    \
    __shared__ __attribute__((aligned(16))) char solve_lds_raw[kSolveLdsBytes];         \
    const SolveLds W = solve_lds_carve(solve_lds_raw)

// ---- r = d - S z in double (dense_solve_dev.inc: resid_rows_block); blockIdx.x = block of 64 rows ---------------------
template <int KIND, bool BATCH>
__global__ __launch_bounds__(256) void cov_residual_kernel(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                            const double* __restrict__ ovar, int64_t m, double g,
                                                            const double* __restrict__ d, const double* __restrict__ z,
                                                            double* __restrict__ r, const double* __restrict__ olat, double win_deg,
                                                            const int* __restrict__ converged, const SolveMember* __restrict__ mem,
                                                            double* __restrict__ partial, int nsplit) {
    // partial != nullptr (single system with fewer than two blocks of rows per CU): blockIdx.y = one of nsplit slices of the
    // column range; the slice's sums go to partial[y][row] and resid_combine_kernel adds them in slice order
    if (BATCH) {                                                // batched: blockIdx.y = member, r = its padded right-hand side
        const SolveMember* mb = mem + blockIdx.y;
        m = mb->m;
        if ((int64_t)blockIdx.x * 64 >= m) return;
        oxyz = mb->oxyz;
        osig = mb->osig;
        ovar = mb->ovar;
        d = mb->d;
        z = mb->z;
        r = mb->rhs;
        if (olat != nullptr) olat = mb->olat;                   // (olat non-null = "use the latitude window")
        converged = &mb->st->conv;
    }
    SOLVE_LDS(W);
    if (converged != nullptr && *converged != 0) return;       // the refinement has met its tolerance: nothing left to evaluate
    resid_rows_block<KIND, false>(oxyz, osig, ovar, m, g, d, z, r, olat, win_deg, BATCH ? (double*)nullptr : partial, nsplit, (int)blockIdx.y,
                            (int64_t)blockIdx.x, W);
}

// r = d - (sig * sum of the column slices' sums, in slice order, + var * z): second half of the sliced residual
__global__ __launch_bounds__(256) void resid_combine_kernel(const double* __restrict__ partial, int nsplit, int64_t m,
                                                             const double* __restrict__ osig, const double* __restrict__ ovar,
                                                             const double* __restrict__ d, const double* __restrict__ z,
                                                             double* __restrict__ r, const int* __restrict__ converged) {
    if (converged != nullptr && *converged != 0) return;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= m) return;
    double s = 0.0;
    for (int y = 0; y < nsplit; ++y) s += partial[(int64_t)y * m + row];
    r[row] = d[row] - (osig[row] * s + ovar[row] * z[row]);
}

// ---- the same residual on COMPACT blocks of rows (dense_solve_dev.inc: resid_compact_block) ------------------------------
template <int KIND, bool BATCH>
__global__ __launch_bounds__(256) void cov_residual_blocks_kernel(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                                   const double* __restrict__ ovar, int64_t m, double g,
                                                                   const double* __restrict__ d, const double* __restrict__ z,
                                                                   double* __restrict__ r, const double* __restrict__ olat, double win_deg,
                                                                   const int* __restrict__ converged, const SolveMember* __restrict__ mem,
                                                                   const int* __restrict__ perm, double cut_chord, double far_chord) {
    if (BATCH) {                                                // batched: blockIdx.y = member, r = its padded right-hand side
        const SolveMember* mb = mem + blockIdx.y;
        m = mb->m;
        if ((int64_t)blockIdx.x * 64 >= m) return;
        oxyz = mb->oxyz;
        osig = mb->osig;
        ovar = mb->ovar;
        d = mb->d;
        z = mb->z;
        r = mb->rhs;
        olat = mb->olat;
        perm = mb->perm;
        converged = &mb->st->conv;
    }
    SOLVE_LDS(W);
    if (converged != nullptr && *converged != 0) return;       // the refinement has met its tolerance: nothing left to evaluate
    resid_compact_block<KIND, false>(oxyz, osig, ovar, m, g, d, z, r, olat, win_deg, perm, cut_chord, far_chord, (int64_t)blockIdx.x, W);
}

// ---- out = r_prev - S dz on the same compact blocks, S dz in packed fp32 (dense_solve_dev.inc: resid_update_block) ---------
__global__ __launch_bounds__(256) void cov_residual_update_kernel(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                                   const double* __restrict__ ovar, int64_t m, double g,
                                                                   const double* __restrict__ r_prev, const double* __restrict__ dz,
                                                                   double* __restrict__ out, const double* __restrict__ olat, double win_deg,
                                                                   const int* __restrict__ converged, const int* __restrict__ perm,
                                                                   double cut_chord) {
    SOLVE_LDS(W);
    if (converged != nullptr && *converged != 0) return;       // the refinement has met its tolerance: nothing left to evaluate
    resid_update_block(oxyz, osig, ovar, m, g, r_prev, dz, out, olat, win_deg, perm, cut_chord, (int64_t)blockIdx.x, W);
}

// ---- inc_i = sig_i * sum_a C(i,a) w_a ; xa = xb + inc (dense_solve_dev.inc: increment_patch); blockIdx.x = patch / run ----
template <int KIND, typename T, int CELLS, bool BATCH>
__global__ __launch_bounds__(256) void apply_increment_kernel(const double* __restrict__ gxyz, const double* __restrict__ gsig,
                                                               int64_t n, const double* __restrict__ oxyz,
                                                               const double* __restrict__ osig, const double* __restrict__ z,
                                                               int64_t m, double g2,
                                                               const T* __restrict__ xb, T* __restrict__ xa, T* __restrict__ inc,
                                                               const double* __restrict__ glat, const double* __restrict__ olat,
                                                               double win_deg, const SolveMember* __restrict__ mem, int nx,
                                                               double cut_chord, double far_chord) {
    if (BATCH) {                                                // batched: blockIdx.y = member
        const SolveMember* mb = mem + blockIdx.y;
        n = mb->n;
        if (nx >= 0) nx = mb->nx;                                // (nx < 0: patches switched off)
        gxyz = mb->gxyz;
        gsig = mb->gsig;
        oxyz = mb->oxyz;
        osig = mb->osig;
        z = mb->z;
        m = mb->m;
        xb = (const T*)mb->xb;
        xa = (T*)mb->xa;
        inc = (T*)mb->inc;
        if (glat != nullptr) { glat = mb->glat; olat = mb->olat; }      // (non-null = "use the latitude window")
    }
    SOLVE_LDS(W);
    increment_patch<KIND, T, CELLS>(gxyz, gsig, n, oxyz, osig, z, m, g2, xb, xa, inc, glat, olat, win_deg, nx, cut_chord, far_chord, (int64_t)blockIdx.x, W);
}

// ---- the increment behind a correction as an update of the first solve's (dense_inc_update.inc; oisat_gain_solve_fields) --------
#include "dense_inc_update.inc"

// The guard of the update form, on the device: it applies where the first residual is small against the innovation, |r_0| <= t |d|
// (t2 = t^2; SolveState of the solve that has just run).  A NaN norm fails it.  Of the two launches behind a solve -- the update
// and the float64 increment of the final z -- exactly one does work and the other returns at once, in the manner of st->conv.
__device__ __forceinline__ bool inc_update_applies(const SolveState* __restrict__ st, double t2) { return st->norm[0] <= t2 * st->dd; }

template <typename T, int CELLS>
__global__ __launch_bounds__(256) void increment_update_kernel(const double* __restrict__ gxyz, const double* __restrict__ gsig, int64_t n,
                                                                const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                                const double* __restrict__ z, const double* __restrict__ z0, int64_t m,
                                                                double g2, const T* __restrict__ xb, T* __restrict__ xa, T* __restrict__ inc,
                                                                const double* __restrict__ inc0, const double* __restrict__ glat,
                                                                const double* __restrict__ olat, double win_deg, int nx, double cut_chord,
                                                                const SolveState* __restrict__ st, double t2) {
    SOLVE_LDS(W);
    if (st != nullptr && !inc_update_applies(st, t2)) return;  // the float64 increment of the final z writes the fields (block-uniform)
    const bool skip = st != nullptr && st->conv != 0 && st->computed == 1;      // converged at r_0: z = z0
    increment_update_patch<T, CELLS>(gxyz, gsig, n, oxyz, osig, z, z0, m, g2, xb, xa, inc, inc0, glat, olat, win_deg, nx, cut_chord, skip,
                                     (int64_t)blockIdx.x, W);
}

// the parent's float64 increment (Gaussian), for the solves the guard keeps off the update form
template <typename T, int CELLS>
__global__ __launch_bounds__(256) void apply_increment_guarded_kernel(const double* __restrict__ gxyz, const double* __restrict__ gsig,
                                                                       int64_t n, const double* __restrict__ oxyz,
                                                                       const double* __restrict__ osig, const double* __restrict__ z,
                                                                       int64_t m, double g2, const T* __restrict__ xb, T* __restrict__ xa,
                                                                       T* __restrict__ inc, const double* __restrict__ glat,
                                                                       const double* __restrict__ olat, double win_deg, int nx,
                                                                       double cut_chord, double far_chord,
                                                                       const SolveState* __restrict__ st, double t2) {
    SOLVE_LDS(W);
    if (inc_update_applies(st, t2)) return;                    // the update has written the fields (block-uniform)
    increment_patch<OISAT_CORR_GAUSSIAN, T, CELLS>(gxyz, gsig, n, oxyz, osig, z, m, g2, xb, xa, inc, glat, olat, win_deg, nx, cut_chord,
                                                   far_chord, (int64_t)blockIdx.x, W);
}

// ---- probe spread (oisat_probe_spread): the kernel is dense_spread.inc, shared with the ensemble's oisat_member_spread --------
#include "dense_spread.inc"

}  // namespace

extern "C" int oisat_set_correlation(oisat_ctx* h, int kind) {
    ARG_CHECK(h != nullptr && corr_kind_ok(kind));
    h->corr = kind;
    return OISAT_OK;
}

extern "C" int oisat_corr_eval(int kind, double g, const double* d2, int64_t n, double* out) {
    ARG_CHECK(corr_kind_ok(kind) && g >= 0.0 && n >= 0 && ((d2 && out) || n == 0));
    const double a = corr_scale(kind, g);
    if (kind == OISAT_CORR_GASPARI_COHN)
        for (int64_t i = 0; i < n; ++i) out[i] = corr_f64<OISAT_CORR_GASPARI_COHN>(a, d2[i]);
    else if (kind == OISAT_CORR_SOAR)
        for (int64_t i = 0; i < n; ++i) out[i] = corr_f64<OISAT_CORR_SOAR>(a, d2[i]);
    else
        for (int64_t i = 0; i < n; ++i) out[i] = corr_f64<OISAT_CORR_GAUSSIAN>(a, d2[i]);
    return OISAT_OK;
}

extern "C" int oisat_corr_cut_chord(int kind, double g, double bits, double* chord_out) {
    ARG_CHECK(corr_kind_ok(kind) && g > 0.0 && bits >= 1.0 && chord_out);
    *chord_out = cut_chord(kind, g, bits);
    return OISAT_OK;
}

// Host restatement of block_sphere + stage_near<true> for ONE block of points (an increment patch's cells, a compact residual
// block's rows): how many observations the block stages into its near and into its far list.  pts_xyz = x[npts] | y[npts] |
// z[npts], obs_xyz likewise with m; olat (ascending, or NULL: no window, hence no cull and no far tier) and the block's latitude
// span [lat_lo, lat_hi] give the candidate range as in the kernels.  bits: the far tier's (0 = off, < 0 = the library's
// setting).  The centre is summed point by point here and by a tree on the device: a count can differ by an observation that
// sits on a radius to the last bit.
extern "C" int oisat_solve_tier_counts(int kind, double g, double bits, const double* pts_xyz, int64_t npts, const double* obs_xyz, int64_t m,
                                       const double* olat, double lat_lo, double lat_hi, int64_t* near_out, int64_t* far_out) {
    ARG_CHECK(corr_kind_ok(kind) && g > 0.0 && pts_xyz && npts > 0 && obs_xyz && m > 0);
    ARG_CHECK(bits <= kCutBits && lat_lo <= lat_hi);
    double far_chord;
    ARG_CHECK(far_chord_of(kind, g, &far_chord, bits));
    const double win = lat_window_deg(kind, g);
    const bool windowed = olat != nullptr && win < 180.0;
    int64_t j0 = 0, j1 = m;
    if (windowed) {
        j0 = std::lower_bound(olat, olat + m, lat_lo - win) - olat;
        j1 = std::lower_bound(olat, olat + m, lat_hi + win + 1e-9) - olat;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t i = 0; i < npts; ++i) { sx += pts_xyz[i]; sy += pts_xyz[npts + i]; sz += pts_xyz[2 * npts + i]; }
    const double nrm = sqrt(sx * sx + sy * sy + sz * sz);
    double r2cull = 1e30, r2far = (double)INFINITY, cx = 0.0, cy = 0.0, cz = 0.0;
    if (nrm > 1e-9 && windowed) {
        cx = sx / nrm; cy = sy / nrm; cz = sz / nrm;
        double r2 = 0.0;
        for (int64_t i = 0; i < npts; ++i) {
            const double dx = pts_xyz[i] - cx, dy = pts_xyz[npts + i] - cy, dz = pts_xyz[2 * npts + i] - cz;
            r2 = std::max(r2, dx * dx + dy * dy + dz * dz);
        }
        const double rho = sqrt(r2) * (1.0 + 1e-12) + 1e-12;
        const double rr = cut_chord_of(kind, g) + rho, rf = far_chord + rho;
        r2cull = rr * rr;
        if (far_chord < 1e9) r2far = rf * rf;
    }
    int64_t nnear = 0, nfar = 0;
    for (int64_t c = j0; c < j1; ++c) {
        const double dx = obs_xyz[c] - cx, dy = obs_xyz[m + c] - cy, dz = obs_xyz[2 * m + c] - cz;
        const double q2 = dx * dx + dy * dy + dz * dz;
        if (!(q2 <= r2cull)) continue;
        if (q2 >= r2far) ++nfar; else ++nnear;
    }
    if (near_out) *near_out = nnear;
    if (far_out) *far_out = nfar;
    return OISAT_OK;
}

extern "C" int oisat_cov_build(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                               float* S, int64_t ld) {
    ARG_CHECK(h && oxyz && osig && ovar && S && m > 0 && g >= 0.0);
    const int64_t mp = cdiv(m, 128) * 128;
    ARG_CHECK(ld >= mp && (ld % 4) == 0 && ((uintptr_t)S % 16) == 0);
    const int ntile = (int)(mp / 64);
    const int64_t nblk = (int64_t)ntile * (ntile + 1) / 2;
    ARG_CHECK(nblk < (int64_t)INT32_MAX);
    OISAT_LAUNCH_CORR(h, "cov_build", cov_build_kernel, OISAT_TARGS(false, false), dim3((unsigned)nblk), dim3(256), 0, oxyz, osig, ovar, m, mp,
                      (float)corr_scale2(h->corr, g), S, ld, ntile, (const int*)nullptr, (const int*)nullptr);
    return OISAT_OK;
}

extern "C" int oisat_cov_build_env(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                   float* S, int64_t ld, const int32_t* env_dev) {
    ARG_CHECK(env_dev != nullptr);
    if (oisat_envelope_off()) return oisat_cov_build(h, oxyz, osig, ovar, m, g, S, ld);
    ARG_CHECK(h && oxyz && osig && ovar && S && m > 0 && g >= 0.0);
    const int64_t mp = cdiv(m, 128) * 128;
    ARG_CHECK(ld >= mp && (ld % 4) == 0 && ((uintptr_t)S % 16) == 0);
    const int ntile = (int)(mp / 64);
    const int64_t nblk = (int64_t)ntile * (ntile + 1) / 2;
    ARG_CHECK(nblk < (int64_t)INT32_MAX);
    OISAT_LAUNCH_CORR(h, "cov_build", cov_build_kernel, OISAT_TARGS(true, false), dim3((unsigned)nblk), dim3(256), 0, oxyz, osig, ovar, m, mp,
                      (float)corr_scale2(h->corr, g), S, ld, ntile, (const int*)env_dev, (const int*)nullptr);
    return OISAT_OK;
}

// Which tiles the banded build touches (host only: the launch below sizes its grid with it, tests restate it).  Block row i
// is zero-filled in [from[i], first[i]) and evaluated in [first[i], i], from[i] = min(first[i], max(zero_first[i], 0)) or 0
// without a claim; width = the most 64 x 64 tiles any tile row touches (row 2 i + 1: 2 (i - from[i]) + 2).
extern "C" int oisat_cov_build_cover(const int32_t* first, const int32_t* zero_first, int64_t nb, int32_t* from_out,
                                     int64_t* width_out, int64_t* zero_tiles_out) {
    ARG_CHECK(first && nb > 0);
    int64_t width = 0, zeros = 0;
    for (int64_t i = 0; i < nb; ++i) {
        ARG_CHECK(first[i] >= 0 && first[i] <= i);
        const int32_t zf = zero_first ? (zero_first[i] < 0 ? 0 : zero_first[i]) : 0;
        const int32_t from = zf < first[i] ? zf : first[i];
        if (from_out) from_out[i] = from;
        width = std::max<int64_t>(width, 2 * (i - from) + 2);
        zeros += first[i] - from;
    }
    if (width_out) *width_out = width;
    if (zero_tiles_out) *zero_tiles_out = zeros;               // (128 x 128 tiles)
    return OISAT_OK;
}

extern "C" int oisat_cov_build_env_zeroed(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                          float* S, int64_t ld, const int32_t* first, const int32_t* env_dev,
                                          const int32_t* zero_first, const int32_t* zero_first_dev, int* enveloped_out) {
    ARG_CHECK(first != nullptr && env_dev != nullptr && (zero_first == nullptr) == (zero_first_dev == nullptr));
    if (enveloped_out) *enveloped_out = 0;
    if (oisat_envelope_off()) return oisat_cov_build(h, oxyz, osig, ovar, m, g, S, ld);       // dense: the caller drops its claim
    ARG_CHECK(h && oxyz && osig && ovar && S && m > 0 && g >= 0.0);
    const int64_t mp = cdiv(m, 128) * 128;
    ARG_CHECK(ld >= mp && (ld % 4) == 0 && ((uintptr_t)S % 16) == 0);
    const int ntile = (int)(mp / 64);
    int64_t width = 0;
    if (int rc = oisat_cov_build_cover(first, zero_first, mp / 128, nullptr, &width, nullptr)) return rc;
    ARG_CHECK(width <= ntile);
    if (ntile > 65535) {                                        // (beyond a grid's second dimension: the triangular launch, which fills every tile)
        if (int rc = oisat_cov_build_env(h, oxyz, osig, ovar, m, g, S, ld, env_dev)) return rc;
        if (enveloped_out) *enveloped_out = 1;
        return OISAT_OK;
    }
    OISAT_LAUNCH_CORR(h, "cov_build", cov_build_kernel, OISAT_TARGS(true, true), dim3((unsigned)width, (unsigned)ntile), dim3(256), 0, oxyz, osig,
                      ovar, m, mp, (float)corr_scale2(h->corr, g), S, ld, ntile, (const int*)env_dev, (const int*)zero_first_dev);
    if (enveloped_out) *enveloped_out = 1;
    return OISAT_OK;
}

extern "C" int oisat_innovation(oisat_ctx* h, int dtype, const void* xb, const int64_t* cell, const double* y, int64_t m,
                                double* d_out) {
    ARG_CHECK(h && xb && cell && y && d_out && m > 0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    const int grid = stream_grid(m, 256);
    if (dtype == OISAT_F32) {
        OISAT_LAUNCH(h, "innovation", (innovation_kernel<float>), dim3(grid), dim3(256), 0, (const float*)xb, cell, y, m, d_out);
    } else {
        OISAT_LAUNCH(h, "innovation", (innovation_kernel<double>), dim3(grid), dim3(256), 0, (const double*)xb, cell, y, m, d_out);
    }
    return OISAT_OK;
}

// The permutation handed over by oisat_set_obs_blocks is ONE-SHOT: the next gain solve / residual on the handle takes it
// and the handle forgets it, so a buffer the caller frees or re-targets afterwards is never read again (a stale
// pointer matched by m alone was an out-of-bounds gather waiting to happen).
const int* oisat_take_obs_perm(oisat_ctx* h, int64_t m) {
    const int* perm = h->obs_perm_m == m ? h->obs_perm : nullptr;
    h->obs_perm = nullptr;
    h->obs_perm_m = 0;
    return perm;
}

// perm (optional, device): the observations along a space-filling curve (oisat_take_obs_perm) -> compact blocks of rows
int oisat_cov_residual_if(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                          const double* d, const double* z, double* r_out, const double* olat_sorted, const int* converged_dev,
                          const int* perm) {
    ARG_CHECK(h && oxyz && osig && ovar && d && z && r_out && m > 0);
    const int kind = h->corr;
    const double win = lat_window_deg(kind, g);
    const double gk = corr_scale(kind, g);                  // what the kernels take: g | kz2
    if (perm && olat_sorted && residual_blocks_pay(kind, g)) {
        double far_chord;
        ARG_CHECK(far_chord_of(kind, g, &far_chord, -1.0, false));
        OISAT_LAUNCH_CORR(h, "cov_residual", cov_residual_blocks_kernel, false, dim3((unsigned)cdiv(m, 64)), dim3(256), 0, oxyz, osig, ovar, m,
                          gk, d, z, r_out, olat_sorted, win, converged_dev, (const SolveMember*)nullptr, perm, cut_chord_of(kind, g), far_chord);
        return OISAT_OK;
    }
    // fewer than two blocks of 64 rows per CU (m < 32,768 on 256 CUs): the column range is cut into slices, a workgroup per
    // (block of rows, slice), and a second launch adds the slices' sums in order -- 157 workgroups of a 10,000-observation
    // system left 40 % of the CUs empty and the others with one workgroup each: 0.21 -> 0.09 ms per evaluation
    const int64_t blocks = cdiv(m, 64), cus = h->cu_count > 0 ? h->cu_count : 256;
    int nsplit = blocks < 2 * cus ? (int)std::min<int64_t>(8, cdiv(2 * cus, blocks)) : 1;
    double* partial = nullptr;
    if (nsplit > 1) {                                       // behind the solve's two work vectors (oisat_dense_reserve sizes the slot)
        const int64_t mp = cdiv(m, 128) * 128;
        double* w = (double*)oisat_ws(h, 5, sizeof(double) * (2 + 8) * mp);
        if (!w) return OISAT_ENOMEM;
        partial = w + 2 * mp;
    }
    OISAT_LAUNCH_CORR(h, "cov_residual", cov_residual_kernel, false, dim3((unsigned)blocks, (unsigned)nsplit), dim3(256), 0, oxyz, osig, ovar, m,
                      gk, d, z, r_out, win < 180.0 ? olat_sorted : (const double*)nullptr, win, converged_dev, (const SolveMember*)nullptr,
                      partial, nsplit);
    if (nsplit > 1) {
        OISAT_LAUNCH(h, "cov_residual", resid_combine_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, (const double*)partial, nsplit, m,
                     osig, ovar, d, z, r_out, converged_dev);
    }
    return OISAT_OK;
}

extern "C" int oisat_set_obs_blocks(oisat_ctx* h, const int32_t* perm, int64_t m) {
    ARG_CHECK(h != nullptr && m >= 0 && (perm != nullptr || m == 0));
    h->obs_perm = perm;
    h->obs_perm_m = perm ? m : 0;
    return OISAT_OK;
}

extern "C" int oisat_cov_residual(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                  const double* d, const double* z, double* r_out, const double* olat_sorted) {
    ARG_CHECK(h != nullptr);
    return oisat_cov_residual_if(h, oxyz, osig, ovar, m, g, d, z, r_out, olat_sorted, nullptr, oisat_take_obs_perm(h, m));
}

// The update form of the residual behind a correction (resid_update_block): where it applies -- the Gaussian on compact blocks
bool oisat_resid_update_applies(const oisat_ctx* h, double g, const double* olat_sorted, const int* perm) {
    return h->corr == OISAT_CORR_GAUSSIAN && perm != nullptr && olat_sorted != nullptr && residual_blocks_pay(h->corr, g);
}

double oisat_resid_update_c() { return kResidUpdateC; }

int oisat_cov_residual_update_if(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                 const double* r_prev, const double* dz, double* out, const double* olat_sorted, const int* converged_dev,
                                 const int* perm) {
    ARG_CHECK(h && oxyz && osig && ovar && r_prev && dz && out && olat_sorted && m > 0 && g >= 0.0);
    ARG_CHECK(out != r_prev && out != dz);
    ARG_CHECK(h->corr == OISAT_CORR_GAUSSIAN && residual_blocks_pay(h->corr, g));
    ARG_CHECK(cdiv(m, 64) < (int64_t)INT32_MAX);
    OISAT_LAUNCH(h, "cov_residual_update", cov_residual_update_kernel, dim3((unsigned)cdiv(m, 64)), dim3(256), 0, oxyz, osig, ovar, m, g, r_prev,
                 dz, out, olat_sorted, lat_window_deg(h->corr, g), converged_dev, perm, cut_chord_of(h->corr, g));
    return OISAT_OK;
}

extern "C" int oisat_cov_residual_update(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                         const double* r_prev, const double* dz, double* out, const double* olat_sorted) {
    ARG_CHECK(h != nullptr);
    return oisat_cov_residual_update_if(h, oxyz, osig, ovar, m, g, r_prev, dz, out, olat_sorted, nullptr, oisat_take_obs_perm(h, m));
}

template <typename T, int CELLS, bool BATCH>
static int increment_launch(oisat_ctx* h, unsigned gx, unsigned gy, const double* gxyz, const double* gsig, int64_t n, int nx, const double* oxyz,
                            const double* osig, const double* z, int64_t m, double g, const void* xb, void* xa, void* inc,
                            const double* glat, const double* olat, double win, const SolveMember* mem) {
    double far_chord;
    ARG_CHECK(far_chord_of(h->corr, g, &far_chord));
    OISAT_LAUNCH_CORR(h, "apply_increment", apply_increment_kernel, OISAT_TARGS(T, CELLS, BATCH), dim3(gx, gy), dim3(256), 0, gxyz, gsig, n, oxyz,
                      osig, z, m, corr_scale2_f64(h->corr, g), (const T*)xb, (T*)xa, (T*)inc, glat, olat, win, mem, nx, cut_chord_of(h->corr, g),
                      far_chord);
    return OISAT_OK;
}

// nx > 0: the n cells are a (n / nx) x nx grid, row-major (oisat_apply_increment_grid); 0: no known shape
static int apply_increment_impl(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t n, int64_t nx, const double* oxyz,
                                const double* osig, const double* z, int64_t m, double g, const void* xb, void* xa, void* inc,
                                const double* glat, const double* olat_sorted) {
    ARG_CHECK(h && gxyz && gsig && oxyz && osig && z && n > 0 && m > 0 && (xa || inc));
    ARG_CHECK(!xa || xb);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    ARG_CHECK(nx >= 0 && nx < (int64_t)INT32_MAX && (nx == 0 || n % nx == 0));
    const double win = lat_window_deg(h->corr, g);
    if (!(win < 180.0) || !glat || !olat_sorted) { glat = nullptr; olat_sorted = nullptr; }
    const int cells = increment_cells(h->cu_count, n, 1);
    const int64_t gx = increment_blocks(n, nx, cells);
    ARG_CHECK(gx < (int64_t)INT32_MAX);
    const unsigned ux = (unsigned)gx;
    if (dtype == OISAT_F32)
        return cells == 1 ? increment_launch<float, 1, false>(h, ux, 1, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, win, nullptr)
                          : increment_launch<float, 2, false>(h, ux, 1, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, win, nullptr);
    return cells == 1 ? increment_launch<double, 1, false>(h, ux, 1, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, win, nullptr)
                      : increment_launch<double, 2, false>(h, ux, 1, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, win, nullptr);
}

extern "C" int oisat_apply_increment(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t n,
                                     const double* oxyz, const double* osig, const double* z, int64_t m, double g,
                                     const void* xb, void* xa, void* inc, const double* glat, const double* olat_sorted) {
    return apply_increment_impl(h, dtype, gxyz, gsig, n, 0, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted);
}

extern "C" int oisat_apply_increment_grid(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx,
                                          const double* oxyz, const double* osig, const double* z, int64_t m, double g,
                                          const void* xb, void* xa, void* inc, const double* glat, const double* olat_sorted) {
    ARG_CHECK(ny > 0 && nx > 0);
    return apply_increment_impl(h, dtype, gxyz, gsig, ny * nx, nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted);
}

// ---- the three launches of oisat_gain_solve_fields (dense_solve.hip) behind its sweeps ------------------------------------------
// inc0 = the float64 increment of z0 into a double scratch field: apply_increment_kernel<double> with neither xb nor xa
int oisat_increment_scratch(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                            const double* osig, const double* z0, int64_t m, double g, double* inc0, const double* glat,
                            const double* olat_sorted) {
    return apply_increment_impl(h, OISAT_F64, gxyz, gsig, ny * nx, nx, oxyz, osig, z0, m, g, nullptr, nullptr, inc0, glat, olat_sorted);
}

template <typename T, int CELLS>
static int increment_update_launch(oisat_ctx* h, unsigned gx, const double* gxyz, const double* gsig, int64_t n, int nx, const double* oxyz,
                                   const double* osig, const double* z, const double* z0, int64_t m, double g, const void* xb, void* xa,
                                   void* inc, const double* inc0, const double* glat, const double* olat, const SolveState* st, double t) {
    OISAT_LAUNCH(h, "increment_update", (increment_update_kernel<T, CELLS>), dim3(gx), dim3(256), 0, gxyz, gsig, n, oxyz, osig, z, z0, m,
                 corr_scale2_f64(OISAT_CORR_GAUSSIAN, g), (const T*)xb, (T*)xa, (T*)inc, inc0, glat, olat,
                 lat_window_deg(OISAT_CORR_GAUSSIAN, g, kIncUpdateCutBits), nx, cut_chord(OISAT_CORR_GAUSSIAN, g, kIncUpdateCutBits), st, t * t);
    return OISAT_OK;
}

template <typename T, int CELLS>
static int increment_guarded_launch(oisat_ctx* h, unsigned gx, const double* gxyz, const double* gsig, int64_t n, int nx, const double* oxyz,
                                    const double* osig, const double* z, int64_t m, double g, const void* xb, void* xa, void* inc,
                                    const double* glat, const double* olat, const SolveState* st, double t) {
    double far_chord;
    ARG_CHECK(far_chord_of(OISAT_CORR_GAUSSIAN, g, &far_chord));
    OISAT_LAUNCH(h, "apply_increment", (apply_increment_guarded_kernel<T, CELLS>), dim3(gx), dim3(256), 0, gxyz, gsig, n, oxyz, osig, z, m,
                 corr_scale2_f64(OISAT_CORR_GAUSSIAN, g), (const T*)xb, (T*)xa, (T*)inc, glat, olat, lat_window_deg(OISAT_CORR_GAUSSIAN, g), nx,
                 cut_chord_of(OISAT_CORR_GAUSSIAN, g), far_chord, st, t * t);
    return OISAT_OK;
}

double oisat_inc_update_t() { return kIncUpdateT; }

// fields = T(inc0 + delta) (increment_update_kernel) where the guard lets the update form apply, and the float64 increment of the
// final z (apply_increment_guarded_kernel: the arithmetic of oisat_apply_increment_grid) where it does not; st = nullptr: the
// update alone, unguarded (oisat_increment_update: the kernel at the ABI).  Patches and cells per thread: apply_increment_impl's.
int oisat_increment_update_if(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                              const double* osig, const double* z, const double* z0, int64_t m, double g, const void* xb, void* xa,
                              void* inc, const double* inc0, const double* glat, const double* olat_sorted, const SolveState* st, double t) {
    ARG_CHECK(h && gxyz && gsig && oxyz && osig && z && z0 && inc0 && ny > 0 && nx > 0 && m > 0 && (xa || inc) && g >= 0.0);
    ARG_CHECK(!xa || xb);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    ARG_CHECK(h->corr == OISAT_CORR_GAUSSIAN && nx < (int64_t)INT32_MAX);
    const int64_t n = ny * nx;
    const double win = lat_window_deg(OISAT_CORR_GAUSSIAN, g);
    if (!(win < 180.0) || !glat || !olat_sorted) { glat = nullptr; olat_sorted = nullptr; }       // (the rule of apply_increment_impl)
    const int cells = increment_cells(h->cu_count, n, 1);
    const int64_t gx = increment_blocks(n, nx, cells);
    ARG_CHECK(gx < (int64_t)INT32_MAX);
    const unsigned ux = (unsigned)gx;
    int rc;
    if (dtype == OISAT_F32)
        rc = cells == 1 ? increment_update_launch<float, 1>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, z0, m, g, xb, xa, inc, inc0, glat, olat_sorted, st, t)
                        : increment_update_launch<float, 2>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, z0, m, g, xb, xa, inc, inc0, glat, olat_sorted, st, t);
    else
        rc = cells == 1 ? increment_update_launch<double, 1>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, z0, m, g, xb, xa, inc, inc0, glat, olat_sorted, st, t)
                        : increment_update_launch<double, 2>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, z0, m, g, xb, xa, inc, inc0, glat, olat_sorted, st, t);
    if (rc || st == nullptr) return rc;
    if (dtype == OISAT_F32)
        return cells == 1 ? increment_guarded_launch<float, 1>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, st, t)
                          : increment_guarded_launch<float, 2>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, st, t);
    return cells == 1 ? increment_guarded_launch<double, 1>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, st, t)
                      : increment_guarded_launch<double, 2>(h, ux, gxyz, gsig, n, (int)nx, oxyz, osig, z, m, g, xb, xa, inc, glat, olat_sorted, st, t);
}

extern "C" int oisat_increment_update(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx,
                                      const double* oxyz, const double* osig, const double* z, const double* z0, int64_t m, double g,
                                      const void* xb, void* xa, void* inc, const double* inc0, const double* glat,
                                      const double* olat_sorted) {
    return oisat_increment_update_if(h, dtype, gxyz, gsig, ny, nx, oxyz, osig, z, z0, m, g, xb, xa, inc, inc0, glat, olat_sorted, nullptr, 0.0);
}

extern "C" int oisat_probe_spread(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                                  const double* osig, const float* U, int64_t nprobe, int64_t ldu, int64_t m, double g, const double* glat,
                                  const double* olat_sorted, int accumulate, double* sum2_out, double* sum4_out) {
    return spread_launch<false>(h, "probe_spread", gxyz, gsig, ny, nx, oxyz, osig, U, nprobe, ldu, m, g, glat, olat_sorted, accumulate, sum2_out,
                                sum4_out, nullptr, 0);
}

// ---- batched forms (oisat_batch_solve, dense_solve.hip): blockIdx.y = member of the device table --------------------------
int oisat_cov_residual_batched(oisat_ctx* h, const SolveMember* mem_dev, const std::vector<SolveMember>& mem_host, int64_t max_m, double g) {
    const int kind = h->corr;
    const double win = lat_window_deg(kind, g);
    const double gk = corr_scale(kind, g);
    const int nmem = (int)mem_host.size();
    bool blocks = residual_blocks_pay(kind, g);
    for (const SolveMember& sm : mem_host) blocks = blocks && sm.perm != nullptr;
    if (blocks) {
        double far_chord;
        ARG_CHECK(far_chord_of(kind, g, &far_chord, -1.0, false));
        OISAT_LAUNCH_CORR(h, "cov_residual", cov_residual_blocks_kernel, true, dim3((unsigned)cdiv(max_m, 64), (unsigned)nmem), dim3(256), 0,
                          (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (int64_t)0, gk, (const double*)nullptr,
                          (const double*)nullptr, (double*)nullptr, (const double*)nullptr, win, (const int*)nullptr, mem_dev, (const int*)nullptr,
                          cut_chord_of(kind, g), far_chord);
        return OISAT_OK;
    }
    static const double dummy = 0.0;                        // non-null marker: "use each member's latitude window"
    OISAT_LAUNCH_CORR(h, "cov_residual", cov_residual_kernel, true, dim3((unsigned)cdiv(max_m, 64), (unsigned)nmem), dim3(256), 0,
                 (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (int64_t)0, gk, (const double*)nullptr,
                 (const double*)nullptr, (double*)nullptr, win < 180.0 ? &dummy : (const double*)nullptr, win, (const int*)nullptr,
                 mem_dev, (double*)nullptr, 1);
    return OISAT_OK;
}

int oisat_apply_increment_batched(oisat_ctx* h, int dtype, const SolveMember* mem_dev, const std::vector<SolveMember>& mem_host, int64_t max_n,
                                  double g) {
    const double win = lat_window_deg(h->corr, g);
    static const double dummy = 0.0;
    const double* use = win < 180.0 ? &dummy : (const double*)nullptr;
    const int nmem = (int)mem_host.size();
    const int cells = increment_cells(h->cu_count, max_n, nmem);
    int64_t gx = 0;                                         // workgroups of the member that needs the most
    for (const SolveMember& sm : mem_host) gx = std::max(gx, increment_blocks(sm.n, sm.nx, cells));
    ARG_CHECK(gx > 0 && gx < (int64_t)INT32_MAX);
    const unsigned ux = (unsigned)gx, gy = (unsigned)nmem;
    if (dtype == OISAT_F32)
        return cells == 1 ? increment_launch<float, 1, true>(h, ux, gy, nullptr, nullptr, max_n, 0, nullptr, nullptr, nullptr, 0, g, nullptr, nullptr, nullptr, use, use, win, mem_dev)
                          : increment_launch<float, 2, true>(h, ux, gy, nullptr, nullptr, max_n, 0, nullptr, nullptr, nullptr, 0, g, nullptr, nullptr, nullptr, use, use, win, mem_dev);
    return cells == 1 ? increment_launch<double, 1, true>(h, ux, gy, nullptr, nullptr, max_n, 0, nullptr, nullptr, nullptr, 0, g, nullptr, nullptr, nullptr, use, use, win, mem_dev)
                      : increment_launch<double, 2, true>(h, ux, gy, nullptr, nullptr, max_n, 0, nullptr, nullptr, nullptr, 0, g, nullptr, nullptr, nullptr, use, use, win, mem_dev);
}
