// Posterior ensembles of the dense analysis by Matheron's rule: a member is a draw from N(x_a, A),
//     delta_k = xi_k - B H^T S^-1 (H xi_k + eps_k),    xi_k ~ N(0, B),  eps_k ~ N(0, R),    A = B - B H^T S^-1 H B.
// The solve is the factor's own row sweeps (oisat_trsm_rows, oisat_trsm_rows_bwd); what this unit adds is the prior draw
// and the last step.  The correlations are functions of the chord between unit vectors in R^3, so xi is a random-feature
// field, xi(p) = sqrt(2 / F) sum_f cos 2 pi (omega_f . p + phi_f) with omega_f from the correlation's spectral measure and
// phi_f uniform: E[xi(p) xi(q)] = C(|p - q|) for any F when the frequencies are fresh per member.  The library holds no
// random numbers: frequencies, phases and noise arrive as arrays (oisatgmi/dense.py: ensemble_draws), which is what makes
// both entry points testable to rounding.  (No reference counterpart: the element-wise OI has no error correlations.)
#include "oisat_common.h"
#include "dense_switches.h"

namespace {

#include "dense_solve_dev.inc"
#include "dense_spread.inc"

// ---- out[k][p] = scale_p sqrt(2 / F) sum_f cos 2 pi (omega_kf . p + phi_kf) + sqrt(nscale_p) noise[k][p] (oisat_field_sample) --
// Thread = one point, 256 consecutive points per workgroup, blockIdx.y = member.  A member's features pass through LDS in
// chunks of kFeatChunk (x, y, z, phase: 32 bytes a feature, read back wave-uniformly as two 16-byte words).  Per (point,
// feature): the phase in turns in DOUBLE, fma(oz, pz, fma(oy, py, fma(ox, px, phi))); minus its nearest integer, still in
// double -- SOAR's heavy-tailed frequencies give phases of 1e3 .. 1e5 turns, of which a float would keep no fraction --; the
// remainder in [-1/2, 1/2] narrowed to float; cospif(2 r), whose argument scaling is exact; added to an fp32 sum in feature
// order.  The end is one double expression rounded once: scale sqrt(2 / F) sum + sqrt(nscale) noise.  A point in npts .. ld
// gets an exact zero.  No workgroup waits for another; the bits depend on the inputs alone.
constexpr int kFeatChunk = 128;
struct __attribute__((aligned(32))) Feature { double x, y, z, phi; };
__global__ __launch_bounds__(256) void field_sample_kernel(const double* __restrict__ pxyz, int64_t npts, const double* __restrict__ scale,
                                                            const double* __restrict__ omega, const double* __restrict__ phase, int nfeature,
                                                            const float* __restrict__ noise, const double* __restrict__ nscale,
                                                            float* __restrict__ out, int64_t ld) {
    __shared__ Feature sf[kFeatChunk];
    const int t = threadIdx.x;
    const int64_t k = blockIdx.y, p = (int64_t)blockIdx.x * 256 + t;
    const bool live = p < npts;
    const double px = live ? pxyz[p] : 0.0, py = live ? pxyz[npts + p] : 0.0, pz = live ? pxyz[2 * npts + p] : 0.0;
    const double* __restrict__ om = omega + k * 3 * (int64_t)nfeature;
    const double* __restrict__ ph = phase + k * (int64_t)nfeature;
    float acc = 0.f;
    for (int f0 = 0; f0 < nfeature; f0 += kFeatChunk) {
        const int cnt = nfeature - f0 < kFeatChunk ? nfeature - f0 : kFeatChunk;
        if (t < cnt) {
            Feature ft;
            ft.x = om[f0 + t];
            ft.y = om[nfeature + f0 + t];
            ft.z = om[2 * (int64_t)nfeature + f0 + t];
            ft.phi = ph[f0 + t];
            sf[t] = ft;
        }
        __syncthreads();
        for (int f = 0; f < cnt; ++f) {
            const Feature ft = sf[f];
            const double turns = __builtin_fma(ft.z, pz, __builtin_fma(ft.y, py, __builtin_fma(ft.x, px, ft.phi)));
            const float r = (float)(turns - rint(turns));
            acc += cospif(2.0f * r);
        }
        __syncthreads();
    }
    if (p >= ld) return;
    float v = 0.f;
    if (live) {
        double d = (scale ? scale[p] : 1.0) * sqrt(2.0 / (double)nfeature) * (double)acc;
        if (noise) d += sqrt(nscale[p]) * (double)noise[k * ld + p];
        v = (float)d;
    }
    out[k * ld + p] = v;
}

}  // namespace

extern "C" int oisat_field_sample(oisat_ctx* h, const double* pxyz, int64_t npts, const double* scale, const double* omega, const double* phase,
                                  int64_t nfeature, int64_t nmember, const float* noise, const double* nscale, float* out, int64_t ld) {
    ARG_CHECK(h && pxyz && omega && phase && out && npts >= 1 && ld >= npts);
    ARG_CHECK(nfeature >= 1 && nfeature < (int64_t)INT32_MAX && nmember >= 1 && nmember <= 65535);
    ARG_CHECK((noise == nullptr) == (nscale == nullptr));
    const int64_t gx = cdiv(ld, 256);
    ARG_CHECK(gx < (int64_t)INT32_MAX);
    OISAT_LAUNCH(h, "field_sample", field_sample_kernel, dim3((unsigned)gx, (unsigned)nmember), dim3(256), 0, pxyz, npts, scale, omega, phase,
                 (int)nfeature, noise, nscale, out, ld);
    return OISAT_OK;
}

extern "C" int oisat_member_spread(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                                   const double* osig, const float* U, int64_t nmember, int64_t ldu, int64_t m, double g, const double* glat,
                                   const double* olat_sorted, float* P, int64_t ldp, int accumulate, double* sum2_out, double* sum4_out) {
    return spread_launch<true>(h, "member_spread", gxyz, gsig, ny, nx, oxyz, osig, U, nmember, ldu, m, g, glat, olat_sorted, accumulate, sum2_out,
                               sum4_out, P, ldp);
}
