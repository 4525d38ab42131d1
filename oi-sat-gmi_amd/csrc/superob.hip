// Superobservations: every observation is put into a box of a reduced latitude-longitude grid (bands of box_deg, in band j
// n_j = max(1, llrint(360 cos(mid_j) / box_deg)) longitude boxes: roughly equal area) and per box
//     count, W = sum w, Q = sum sqrt(w), D = sum w d, V = sum w d d, G = sum w sigma_b, P = sum w (x, y, z),   w = 1 / var
// are formed, from which the host makes one observation per non-empty box (oisatgmi/dense.py: superob).  The reference has no
// counterpart.  The table (n_j, offset_j) is made on the host in float64 (oisat_superob_boxes) and handed to the device, which
// never evaluates a cosine; the box rule is written out operation by operation in include/oisat.h.
//
// The sums are EXACT INTEGERS by the covariogram's rule (variogram.hip): every term is rounded once to a multiple of a
// power-of-two quantum (superob_quanta, from the device-reduced maxima of w, |d| and |sigma_b|) and added as int64 -- first in
// LDS over each run of consecutive lanes of a wave that share a box (a gridded month: the cells of one box along a row), then
// with one 64-bit global atomic per run and quantity.  The accumulators are quantity-major, acc[quantity][box], so the run
// heads of a wave, which are neighbouring boxes, add to neighbouring addresses.  Integer addition is associative: the result
// depends neither on the order of the observations nor on the launch shape nor on the run.  Built with the exact flags
// (-ffp-contract=off): one rounding per operation.
#include "oisat_common.h"

namespace {

constexpr int64_t kSoMaxObs = (int64_t)1 << 20;
constexpr int64_t kSoMaxBox = (int64_t)1 << 23;  // boxes the workspace is allowed to hold (box_deg >= 0.071 degrees)
constexpr int kSoSums = 8;                       // W, Q, D, V, G, Px, Py, Pz (include/oisat.h: OISAT_SUPEROB_*)
constexpr int kSoQuanta = 6;                     // W, Q, D, V, G, P: the three components of P share one
constexpr int kSoWs = 12;                        // the handle's workspace slot: head | band table | accumulators
constexpr size_t kSoHead = 64;                   // head: bits of wmax, max |d|, max |sigma_b| (uint64 each), [3] observations used
constexpr double kSoDblMax = 1.7976931348623157e308;

__host__ __device__ inline double so_pow2(int e) { return ldexp(1.0, e < -1022 ? -1022 : e); }

// quantum of a sum of at most m terms of magnitude <= bound: bound * m < 2^e, so the integer stays below 2^62 + m / 2
__host__ __device__ inline double so_quantum(double bound, int64_t m) {
    const double prod = bound * (double)(m > 1 ? m : 1);
    int e = 0;
    (void)frexp(prod, &e);
    return prod == 0.0 ? 1.0 : so_pow2(e - 62);
}

// The six quanta (include/oisat.h).  The bound of sqrt(w) is the power of two 2^ceil(e_w / 2), e_w the frexp exponent of wmax
// (w < 2^e_w): no square root enters a quantum.  Products left to right, as the terms themselves are formed, so that rounding
// keeps every term at or below its bound.
__host__ __device__ inline void superob_quanta(double wmax, double dmax, double smax, int64_t m, double* q) {
    int ew = 0;
    (void)frexp(wmax, &ew);
    const int eh = ew >= 0 ? (ew + 1) / 2 : -((-ew) / 2);
    q[0] = so_quantum(wmax, m);
    q[1] = so_quantum(wmax == 0.0 ? 0.0 : ldexp(1.0, eh), m);
    q[2] = so_quantum(wmax * dmax, m);
    q[3] = so_quantum(wmax * dmax * dmax, m);
    q[4] = so_quantum(wmax * smax, m);
    q[5] = so_quantum(2.0 * wmax, m);
}

__host__ __device__ inline bool so_finite(double v) { return fabs(v) <= kSoDblMax; }     // (false for NaN)

// does observation (lat, lon, d, sigma_b, var) take part?  *w = 1 / var if so
__device__ inline bool so_take(double lat, double lon, double d, double s, double var, double* w) {
    if (!(so_finite(lat) && so_finite(lon) && so_finite(d) && so_finite(s) && so_finite(var))) return false;
    if (!(fabs(lat) <= 90.0) || !(var > 0.0)) return false;
    const double iv = 1.0 / var;
    if (!so_finite(iv)) return false;
    *w = iv;
    return true;
}

// head[0..2] <- max of the bits of w, |d|, |sigma_b| over the observations that take part (non-negative doubles order like
// their bit patterns), head[3] += their number
__global__ __launch_bounds__(256) void superob_max_kernel(const double* __restrict__ olat, const double* __restrict__ olon,
                                                           const double* __restrict__ d, const double* __restrict__ sig,
                                                           const double* __restrict__ var, int64_t m, unsigned long long* __restrict__ head) {
    __shared__ unsigned long long s_max[3][256];
    __shared__ unsigned s_cnt[256];
    const int t = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mw = 0, md = 0, ms = 0;
    unsigned cnt = 0;
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + t; a < m; a += stride) {
        double w;
        const double da = d[a], sa = sig[a];
        if (!so_take(olat[a], olon[a], da, sa, var[a], &w)) continue;
        const unsigned long long bw = (unsigned long long)__double_as_longlong(w);
        const unsigned long long bd = (unsigned long long)__double_as_longlong(fabs(da));
        const unsigned long long bs = (unsigned long long)__double_as_longlong(fabs(sa));
        mw = bw > mw ? bw : mw;
        md = bd > md ? bd : md;
        ms = bs > ms ? bs : ms;
        ++cnt;
    }
    s_max[0][t] = mw;
    s_max[1][t] = md;
    s_max[2][t] = ms;
    s_cnt[t] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            for (int k = 0; k < 3; ++k) s_max[k][t] = s_max[k][t + s] > s_max[k][t] ? s_max[k][t + s] : s_max[k][t];
            s_cnt[t] += s_cnt[t + s];
        }
        __syncthreads();
    }
    if (t == 0 && s_cnt[0] != 0) {
        atomicMax(&head[0], s_max[0][0]);
        atomicMax(&head[1], s_max[1][0]);
        atomicMax(&head[2], s_max[2][0]);
        atomicAdd(&head[3], (unsigned long long)s_cnt[0]);
    }
}

// One observation per lane, 256 per workgroup and step (every workgroup takes the same number of steps: the barriers are
// uniform).  box_out[a] = the observation's box or -1.  acc = count | W | Q | D | V | G | Px | Py | Pz, int64[nbox] each,
// zeroed by the caller; with_sums = 0: box_out and count only (oxyz is then not read).
__global__ __launch_bounds__(256) void superob_accumulate_kernel(const double* __restrict__ olat, const double* __restrict__ olon,
                                                                  const double* __restrict__ oxyz, const double* __restrict__ d,
                                                                  const double* __restrict__ sig, const double* __restrict__ var, int64_t m,
                                                                  double box_deg, const int32_t* __restrict__ box_n,
                                                                  const int64_t* __restrict__ box_off, int64_t nbands, int64_t nbox,
                                                                  const unsigned long long* __restrict__ head,
                                                                  int32_t* __restrict__ box_out, unsigned long long* __restrict__ acc,
                                                                  int with_sums) {
    __shared__ unsigned long long s_acc[kSoSums][256];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave0 = t - lane;
    double iq[kSoQuanta] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
    if (with_sums) {
        double q[kSoQuanta];
        superob_quanta(__longlong_as_double((long long)head[0]), __longlong_as_double((long long)head[1]),
                       __longlong_as_double((long long)head[2]), m, q);
        for (int k = 0; k < kSoQuanta; ++k) iq[k] = 1.0 / q[k];        // powers of two: the products below are exact divisions
    }
    const unsigned long long below = lane == kWave - 1 ? ~0ull : (2ull << lane) - 1;     // lanes 0 .. lane
    for (int64_t base = (int64_t)blockIdx.x * 256; base < m; base += (int64_t)gridDim.x * 256) {
        const int64_t a = base + t;
        int box = -1;
        double w = 0.0, da = 0.0, sa = 0.0;
        if (a < m) {
            const double lat = olat[a], lon = olon[a];
            da = d[a];
            sa = sig[a];
            if (so_take(lat, lon, da, sa, var[a], &w)) {
                const double fj = floor((lat + 90.0) / box_deg);
                int64_t j = (int64_t)fj;
                j = j < nbands - 1 ? j : nbands - 1;
                const double r = lon / 360.0;
                const double tt = r - floor(r);
                const int64_t nj = box_n[j];
                int64_t k = (int64_t)(tt * (double)nj);
                k = k < nj - 1 ? k : nj - 1;
                const int64_t b = box_off[j] + k;
                box = b >= 0 && b < nbox ? (int)b : -1;       // (always inside for a table that passed the host's check)
            }
            box_out[a] = box;
        }
        // runs of equal boxes among the consecutive lanes of this wave: the first lane of a run is its head and owns a slot
        const int prev = __shfl_up(box, 1);
        const bool is_head = lane == 0 || prev != box;
        const unsigned long long heads = __ballot(is_head);
        const int mine = 63 - __clzll((long long)(heads & below));         // (bit 0 is always set)
        const unsigned long long later = heads & ~below;
        const int len = (later ? __ffsll((long long)later) - 1 : kWave) - lane;   // a head's run length
        if (with_sums) {
            for (int k = 0; k < kSoSums; ++k) s_acc[k][t] = 0;
            __syncthreads();
            if (box >= 0) {
                const int slot = wave0 + mine;
                const double wd = w * da;
                atomicAdd(&s_acc[0][slot], (unsigned long long)llrint(w * iq[0]));
                atomicAdd(&s_acc[1][slot], (unsigned long long)llrint(sqrt(w) * iq[1]));
                atomicAdd(&s_acc[2][slot], (unsigned long long)llrint(wd * iq[2]));
                atomicAdd(&s_acc[3][slot], (unsigned long long)llrint(wd * da * iq[3]));
                atomicAdd(&s_acc[4][slot], (unsigned long long)llrint(w * sa * iq[4]));
                atomicAdd(&s_acc[5][slot], (unsigned long long)llrint(w * oxyz[a] * iq[5]));
                atomicAdd(&s_acc[6][slot], (unsigned long long)llrint(w * oxyz[m + a] * iq[5]));
                atomicAdd(&s_acc[7][slot], (unsigned long long)llrint(w * oxyz[2 * m + a] * iq[5]));
            }
            __syncthreads();
            if (is_head && box >= 0)
                for (int k = 0; k < kSoSums; ++k) atomicAdd(&acc[(int64_t)(1 + k) * nbox + box], s_acc[k][t]);
        }
        if (is_head && box >= 0) atomicAdd(&acc[box], (unsigned long long)len);
    }
}

// ceil(180 / box_deg) by the rule of the header: the first j with -90 + (j + 1) box_deg >= 90 ends the bands
int64_t so_nbands(double box_deg) {
    int64_t nb = (int64_t)ceil(180.0 / box_deg);
    if (nb < 1) nb = 1;
    return nb;
}

}  // namespace

extern "C" int oisat_superob_boxes(double box_deg, int64_t cap, int32_t* n_out, int64_t* offset_out, int64_t* nbands_out,
                                   int64_t* nbox_out) {
    ARG_CHECK(std::isfinite(box_deg) && box_deg > 0.0 && box_deg <= 180.0);
    ARG_CHECK(cap >= 0 && (cap == 0 || (n_out && offset_out)));
    ARG_CHECK(180.0 / box_deg <= (double)kSoMaxBox);                     // (every band holds a box: nbox >= nbands)
    const int64_t nbands = so_nbands(box_deg);
    ARG_CHECK(cap == 0 || cap >= nbands);
    int64_t off = 0;
    for (int64_t j = 0; j < nbands; ++j) {
        const double lo = -90.0 + (double)j * box_deg;
        double hi = -90.0 + (double)(j + 1) * box_deg;
        if (hi > 90.0) hi = 90.0;
        const double mid = 0.5 * (lo + hi);
        long long n = llrint(360.0 * cos(mid * (3.14159265358979323846 / 180.0)) / box_deg);
        if (n < 1) n = 1;
        if (cap) {
            n_out[j] = (int32_t)n;
            offset_out[j] = off;
        }
        off += n;
    }
    if (nbands_out) *nbands_out = nbands;
    if (nbox_out) *nbox_out = off;
    return OISAT_OK;
}

extern "C" int oisat_superob_quanta(double wmax, double dmax, double smax, int64_t m, double* q_out) {
    ARG_CHECK(q_out && m >= 0 && m <= kSoMaxObs && wmax >= 0.0 && dmax >= 0.0 && smax >= 0.0);
    const double mm = (double)(m > 1 ? m : 1);
    ARG_CHECK(std::isfinite(2.0 * wmax * mm) && std::isfinite(wmax * dmax * dmax * mm) && std::isfinite(wmax * smax * mm));
    superob_quanta(wmax, dmax, smax, m, q_out);
    return OISAT_OK;
}

extern "C" int oisat_superob(oisat_ctx* h, const double* olat, const double* olon, const double* oxyz, const double* d,
                             const double* sigma_b, const double* var, int64_t m, double box_deg, const int32_t* box_n,
                             const int64_t* box_offset, int64_t nbands, int64_t nbox, int32_t* box_out, int64_t* count_out,
                             double* sums_out, int64_t* nused_out) {
    ARG_CHECK(h && box_n && box_offset && count_out);
    ARG_CHECK(std::isfinite(box_deg) && box_deg > 0.0 && box_deg <= 180.0);
    ARG_CHECK(m >= 0 && m <= kSoMaxObs);
    ARG_CHECK(m == 0 || (olat && olon && d && sigma_b && var && box_out && (oxyz || !sums_out)));
    // the table must be one this box_deg can have: the device indexes the accumulators with it
    ARG_CHECK(nbox >= 1 && nbox <= kSoMaxBox && 180.0 / box_deg <= (double)kSoMaxBox && nbands == so_nbands(box_deg));
    int64_t off = 0;
    for (int64_t j = 0; j < nbands; ++j) {
        ARG_CHECK(box_n[j] >= 1 && box_offset[j] == off);
        off += box_n[j];
        ARG_CHECK(off <= nbox);
    }
    ARG_CHECK(off == nbox);
    const int nq = sums_out ? 1 + kSoSums : 1;
    if (m == 0) {
        memset(count_out, 0, sizeof(int64_t) * (size_t)nbox);
        if (sums_out) memset(sums_out, 0, sizeof(double) * kSoSums * (size_t)nbox);     // (+0.0)
        if (nused_out) *nused_out = 0;
        return OISAT_OK;
    }
    // grow-only, allocated on first use (oisat_dense_reserve does not cover it): head | n_j, offset_j | accumulators
    const size_t table_bytes = ((sizeof(int32_t) + sizeof(int64_t)) * (size_t)nbands + 63) / 64 * 64;
    const size_t off_bytes = sizeof(int64_t) * (size_t)nbands;
    const size_t acc_bytes = sizeof(int64_t) * (size_t)nq * (size_t)nbox;
    char* ws = (char*)oisat_ws(h, kSoWs, kSoHead + table_bytes + acc_bytes);
    if (!ws) return OISAT_ENOMEM;
    unsigned long long* head = (unsigned long long*)ws;
    int64_t* off_dev = (int64_t*)(ws + kSoHead);
    int32_t* n_dev = (int32_t*)(ws + kSoHead + off_bytes);
    unsigned long long* acc = (unsigned long long*)(ws + kSoHead + table_bytes);
    HIP_TRY(hipMemsetAsync(ws, 0, kSoHead, h->stream));
    HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, h->stream));
    HIP_TRY(hipMemcpyAsync(off_dev, box_offset, off_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(n_dev, box_n, sizeof(int32_t) * (size_t)nbands, hipMemcpyHostToDevice, h->stream));
    OISAT_LAUNCH(h, "superob_max", superob_max_kernel, dim3(stream_grid(m, 256)), dim3(256), 0, olat, olon, d, sigma_b, var, m, head);
    OISAT_LAUNCH(h, "superob_accumulate", superob_accumulate_kernel, dim3(stream_grid(m, 256)), dim3(256), 0, olat, olon, oxyz, d,
                 sigma_b, var, m, box_deg, (const int32_t*)n_dev, (const int64_t*)off_dev, nbands, nbox,
                 (const unsigned long long*)head, box_out, acc, sums_out ? 1 : 0);
    unsigned long long hd[4];
    HIP_TRY(hipMemcpyAsync(hd, head, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double mx[3], q[kSoQuanta];
    memcpy(mx, hd, sizeof(mx));
    if (sums_out) {
        const double mm = (double)(m > 1 ? m : 1);
        if (!(std::isfinite(2.0 * mx[0] * mm) && std::isfinite(mx[0] * mx[1] * mx[1] * mm) && std::isfinite(mx[0] * mx[2] * mm))) {
            oisat_set_error("oisat_superob: the largest w, w d d or w sigma_b times m is not finite");
            return OISAT_EINVAL;
        }
        superob_quanta(mx[0], mx[1], mx[2], m, q);
    }
    // the integers come back into the caller's arrays and are scaled in place
    HIP_TRY(hipMemcpy(count_out, acc, sizeof(int64_t) * (size_t)nbox, hipMemcpyDeviceToHost));
    if (sums_out) {
        HIP_TRY(hipMemcpy(sums_out, acc + nbox, sizeof(int64_t) * kSoSums * (size_t)nbox, hipMemcpyDeviceToHost));
        static const int which[kSoSums] = {0, 1, 2, 3, 4, 5, 5, 5};
        for (int k = 0; k < kSoSums; ++k) {
            double* s = sums_out + (size_t)k * (size_t)nbox;
            const double qk = q[which[k]];
            for (int64_t b = 0; b < nbox; ++b) {
                int64_t v;
                memcpy(&v, &s[b], sizeof(v));
                s[b] = (double)v * qk;
            }
        }
    }
    if (nused_out) *nused_out = (int64_t)hd[3];
    return OISAT_OK;
}
