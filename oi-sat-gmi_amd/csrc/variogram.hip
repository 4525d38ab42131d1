// Covariogram of the normalised innovations (Hollingsworth-Loennberg): for every pair a < b of observations within max_chord,
//     count[k] += 1, sum_prod[k] += u_a u_b, sum_chord[k] += chord_ab,  k = (int64)(chord_ab * nbins / max_chord).
// The reference has no counterpart (its analysis has no correlation length).  This is an all-pairs pass -- 5e9 pairs at the
// headline's 99,898 observations -- cut down by the latitude window of the float64 residual (dense_cov.hip) and, inside the
// window, by a test of the squared chord that keeps the square root for the pairs that can land in a bin.
//
// The sums are EXACT INTEGERS: every term is rounded once to a multiple of a power-of-two quantum (covariogram_quanta) and
// added as int64, in LDS (ds_add_u64) and across workgroups (one 64-bit global atomic per touched bin and workgroup).  Integer
// addition is associative, so the result does not depend on the order the atomics arrive in, the launch shape, the window or
// the order of the observations.  Built with the exact flags (-ffp-contract=off): d2 = dx dx + dy dy + dz dz, left to right.
#include "oisat_common.h"

namespace {

constexpr int kCvRows = 256;                     // rows of a workgroup, one per lane
constexpr int kCvSlots = 1024;                   // LDS histogram words per array: four per-wave copies while 4 nbins fit, else one
constexpr int kCvMaxBins = 1024;
constexpr int64_t kCvMaxObs = (int64_t)1 << 20;
constexpr int kCvWs = 11;                        // the handle's workspace slot: head | accumulators | u
constexpr size_t kCvHead = 64;                   // head: [0] bits of max |u| over the finite u (uint64), [1] their number

// The two quanta (include/oisat.h).  P = m (m - 1) / 2 pairs at most: |term| <= umax^2 < 2^e / P, so a bin's integer stays
// below 2^62 + P / 2; a chord is at most 2 (1 + a few ulp).  The exponent is kept at or above the smallest normal's.
__host__ __device__ inline double cv_pow2(int e) { return ldexp(1.0, e < -1022 ? -1022 : e); }

__host__ __device__ inline void covariogram_quanta(double umax, int64_t m, double* q_prod, double* q_chord) {
    const int64_t P = m * (m - 1) / 2;
    const double prod = umax * umax * (double)P;
    int e = 0, ec = 0;
    (void)frexp(prod, &e);
    *q_prod = prod == 0.0 ? 1.0 : cv_pow2(e - 62);
    (void)frexp(2.0 * (double)(P > 1 ? P : 1), &ec);
    *q_chord = cv_pow2(ec - 62);
}

// u = d * w (w == nullptr: d); a u that is not finite becomes NaN, the kernels' mark of "takes part in nothing".  head[0]
// <- max of the bits of |u| (non-negative doubles order like their bit patterns), head[1] += number of finite u.
__global__ __launch_bounds__(256) void covariogram_prepare_kernel(const double* __restrict__ d, const double* __restrict__ w, int64_t m,
                                                                   double* __restrict__ u, unsigned long long* __restrict__ head) {
    __shared__ unsigned long long s_max[256];
    __shared__ unsigned s_cnt[256];
    const int t = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    unsigned cnt = 0;
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + t; a < m; a += stride) {
        double v = w != nullptr ? d[a] * w[a] : d[a];
        if (fabs(v) <= 1.7976931348623157e308) {             // finite (false for NaN)
            const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(v));
            mx = b > mx ? b : mx;
            ++cnt;
        } else {
            v = nan_of<double>();
        }
        u[a] = v;
    }
    s_max[t] = mx;
    s_cnt[t] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            s_max[t] = s_max[t + s] > s_max[t] ? s_max[t + s] : s_max[t];
            s_cnt[t] += s_cnt[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        atomicMax(&head[0], s_max[0]);
        atomicAdd(&head[1], (unsigned long long)s_cnt[0]);
    }
}

// blockIdx.x = block of 256 rows (a row per lane, in registers); the columns come through LDS in chunks of 256, the chunks
// from the block's own (the diagonal one: pairs a < b only) upwards dealt to blockIdx.y in turn.  olat (ascending, or nullptr):
// the columns end at the first latitude beyond the block's last row's + win_deg.  acc = count | sum_prod | sum_chord, int64[nbins]
// each, zeroed by the caller.
__global__ __launch_bounds__(256) void covariogram_kernel(const double* __restrict__ oxyz, const double* __restrict__ u, int64_t m,
                                                           double bin_scale, double lim2, int nbins, const double* __restrict__ olat,
                                                           double win_deg, const unsigned long long* __restrict__ head,
                                                           unsigned long long* __restrict__ acc) {
    __shared__ double4 s_col[kCvRows];                       // x, y, z, u of the staged columns
    __shared__ unsigned long long s_prod[kCvSlots], s_chord[kCvSlots];
    __shared__ unsigned s_cnt[kCvSlots];                     // (a workgroup sees at most 256 m <= 2^28 pairs)
    __shared__ int64_t s_j1;
    const int t = threadIdx.x;
    const int copies = 4 * nbins <= kCvSlots ? 4 : 1;
    const int base = copies == 4 ? (t >> 6) * nbins : 0;
    for (int i = t; i < kCvSlots; i += 256) {
        s_prod[i] = 0;
        s_chord[i] = 0;
        s_cnt[i] = 0;
    }
    const int64_t r0 = (int64_t)blockIdx.x * kCvRows, row = r0 + t;
    if (t == 0) {
        int64_t j1 = m;
        if (olat != nullptr) {
            const int64_t r1 = r0 + kCvRows - 1 < m - 1 ? r0 + kCvRows - 1 : m - 1;
            const double v = olat[r1] + win_deg + 1e-9;
            int64_t lo = r1, hi = m;                          // first index with olat >= v
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (olat[mid] < v) lo = mid + 1; else hi = mid;
            }
            j1 = lo;
        }
        s_j1 = j1;
    }
    double xa = 0.0, ya = 0.0, za = 0.0, ua = nan_of<double>();
    if (row < m) {
        xa = oxyz[row];
        ya = oxyz[m + row];
        za = oxyz[2 * m + row];
        ua = u[row];
    }
    double q_prod, q_chord;
    covariogram_quanta(__longlong_as_double((long long)head[0]), m, &q_prod, &q_chord);
    const double iq_prod = 1.0 / q_prod, iq_chord = 1.0 / q_chord;       // powers of two: the products below are exact divisions
    __syncthreads();
    const int64_t j1 = s_j1;
    for (int64_t kc = (int64_t)blockIdx.x + blockIdx.y; kc * kCvRows < j1; kc += gridDim.y) {
        const int64_t c0 = kc * kCvRows, c = c0 + t;
        double4 col = make_double4(0.0, 0.0, 0.0, nan_of<double>());
        if (c < j1) col = make_double4(oxyz[c], oxyz[m + c], oxyz[2 * m + c], u[c]);
        s_col[t] = col;
        __syncthreads();
        if (ua == ua) {
            const int ncol = (int)(j1 - c0 < kCvRows ? j1 - c0 : kCvRows);
            for (int jj = 0; jj < ncol; ++jj) {
                const double4 b = s_col[jj];                  // (one address per wave: a broadcast)
                if (!(c0 + jj > row) || !(b.w == b.w)) continue;
                const double dx = xa - b.x, dy = ya - b.y, dz = za - b.z;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 <= lim2)) continue;                  // lim2 = max_chord^2 (1 + 1e-9): beyond it k >= nbins for certain
                const double chord = sqrt(d2);
                const long long k = (long long)(chord * bin_scale);
                if (k < 0 || k >= nbins) continue;
                const long long ip = llrint(ua * b.w * iq_prod), ic = llrint(chord * iq_chord);
                atomicAdd(&s_prod[base + k], (unsigned long long)ip);
                atomicAdd(&s_chord[base + k], (unsigned long long)ic);
                atomicAdd(&s_cnt[base + k], 1u);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int k = t; k < nbins; k += 256) {
        unsigned long long cn = 0, sp = 0, sc = 0;
        for (int w = 0; w < copies; ++w) {
            cn += s_cnt[w * nbins + k];
            sp += s_prod[w * nbins + k];
            sc += s_chord[w * nbins + k];
        }
        if (cn != 0) {
            atomicAdd(&acc[k], cn);
            atomicAdd(&acc[nbins + k], sp);
            atomicAdd(&acc[2 * nbins + k], sc);
        }
    }
}

}  // namespace

extern "C" int oisat_covariogram_quantum(double umax, int64_t m, double* q_prod_out, double* q_chord_out) {
    ARG_CHECK(m >= 0 && m <= kCvMaxObs && umax >= 0.0 && q_prod_out && q_chord_out);
    ARG_CHECK(std::isfinite(umax * umax * (double)(m * (m - 1) / 2)));
    covariogram_quanta(umax, m, q_prod_out, q_chord_out);
    return OISAT_OK;
}

extern "C" int oisat_covariogram(oisat_ctx* h, const double* oxyz, const double* d, const double* w, int64_t m, double max_chord,
                                 int nbins, const double* olat_sorted, int64_t* count_out, double* sum_prod_out, double* sum_chord_out,
                                 int64_t* nobs_used_out) {
    ARG_CHECK(h && count_out && sum_prod_out && sum_chord_out);
    ARG_CHECK(m >= 0 && m <= kCvMaxObs && (m == 0 || (oxyz && d)));
    ARG_CHECK(nbins >= 1 && nbins <= kCvMaxBins);
    ARG_CHECK(max_chord > 0.0 && std::isfinite(max_chord));
    if (m == 0) {
        for (int k = 0; k < nbins; ++k) { count_out[k] = 0; sum_prod_out[k] = 0.0; sum_chord_out[k] = 0.0; }
        if (nobs_used_out) *nobs_used_out = 0;
        return OISAT_OK;
    }
    // grow-only, allocated on first use (oisat_dense_reserve does not cover it): head | count, sum_prod, sum_chord | u[m]
    const size_t acc_bytes = sizeof(int64_t) * 3 * (size_t)nbins;
    char* ws = (char*)oisat_ws(h, kCvWs, kCvHead + sizeof(int64_t) * 3 * kCvMaxBins + sizeof(double) * (size_t)m);
    if (!ws) return OISAT_ENOMEM;
    char* pin = (char*)oisat_pinned(h, kCvHead + sizeof(int64_t) * 3 * kCvMaxBins);
    if (!pin) return OISAT_ENOMEM;
    unsigned long long* head = (unsigned long long*)ws;
    unsigned long long* acc = (unsigned long long*)(ws + kCvHead);
    double* u = (double*)(ws + kCvHead + sizeof(int64_t) * 3 * kCvMaxBins);
    HIP_TRY(hipMemsetAsync(ws, 0, kCvHead + acc_bytes, h->stream));
    OISAT_LAUNCH(h, "covariogram_prepare", covariogram_prepare_kernel, dim3(stream_grid(m, 256)), dim3(256), 0, d, w, m, u, head);
    if (m >= 2) {
        const double chord = max_chord < 2.0 ? max_chord : 2.0;
        const double win = chord >= 2.0 ? 1e9 : 2.0 * asin(0.5 * chord) * 57.29577951308232;
        const int64_t blocks = cdiv(m, kCvRows);
        const unsigned gy = (unsigned)(blocks < 8 ? blocks : 8);
        OISAT_LAUNCH(h, "covariogram", covariogram_kernel, dim3((unsigned)blocks, gy), dim3(256), 0, oxyz, (const double*)u, m,
                     (double)nbins / max_chord, max_chord * max_chord * (1.0 + 1e-9), nbins,
                     win < 180.0 ? olat_sorted : (const double*)nullptr, win, (const unsigned long long*)head, acc);
    }
    HIP_TRY(hipMemcpyAsync(pin, ws, kCvHead + acc_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    unsigned long long hd[2];
    memcpy(hd, pin, sizeof(hd));
    double umax, q_prod, q_chord;
    memcpy(&umax, &hd[0], sizeof(double));
    covariogram_quanta(umax, m, &q_prod, &q_chord);
    const int64_t* a = (const int64_t*)(pin + kCvHead);
    for (int k = 0; k < nbins; ++k) {
        count_out[k] = a[k];
        sum_prod_out[k] = (double)a[nbins + k] * q_prod;
        sum_chord_out[k] = (double)a[2 * nbins + k] * q_chord;
    }
    if (nobs_used_out) *nobs_used_out = (int64_t)hd[1];
    return OISAT_OK;
}
