// Monthly averaging and error propagation: averaging.py:11-24 (error_averager) and :97-108 (the
// np.nanmean(axis=0) reductions) of the reference.
//
// HBM layout: a stack of k regridded granules, k*n contiguous elements of T (granule-major), read
// exactly once; one n-element field out.  Thread per cell (x VEC cells), k-loop innermost: for
// every k the wave reads 64*VEC consecutive cells -> fully coalesced 16-byte-per-lane loads.
// The sum runs over k in order, exactly the order NumPy's axis-0 reduction uses, so float64
// results are bit-identical to np.nanmean for finite data.
#include "oisat_common.h"

namespace {

template <typename T>
struct Vec;
template <>
struct Vec<float> {
    using type = float4;
    static constexpr int N = 4;
};
template <>
struct Vec<double> {
    using type = double2;
    static constexpr int N = 2;
};

template <typename T>
__device__ __forceinline__ bool is_inf(T v) { return v == __builtin_inf() || v == -__builtin_inf(); }

template <typename T, bool ERR>
__device__ __forceinline__ void accum(T v, bool flagA, T& sum, unsigned& cnt) {
    // ERR:  flagA = square_input;  drop NaN and inf (averaging.py:19-20)
    // mean: flagA = inf_to_nan;    drop NaN, and inf too when flagged (averaging.py:92)
    if (ERR) {
        if (flagA) v = v * v;
        if (v == v && !is_inf(v)) { sum += v; ++cnt; }
    } else {
        if (v == v && !(flagA && is_inf(v))) { sum += v; ++cnt; }
    }
}

template <typename T, bool ERR>
__device__ __forceinline__ T finish(T sum, unsigned cnt) {
    if (ERR) {
        const T c = (T)cnt;
        return sqrt(sum / (c * c));        // sqrt(sum/size**2); 0/0 -> NaN
    }
    return sum / (T)cnt;                   // nanmean: 0/0 -> NaN
}

template <typename T, bool ERR>
__global__ __launch_bounds__(256) void stack_reduce_kernel(const T* __restrict__ stack, int k, int64_t n, bool flagA,
                                                            bool aligned, T* __restrict__ out) {
    using V = typename Vec<T>::type;
    constexpr int N = Vec<T>::N;
    const int64_t nvec = n / N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (aligned) {
        for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
            T sum[N];
            unsigned cnt[N];
#pragma unroll
            for (int j = 0; j < N; ++j) { sum[j] = T(0); cnt[j] = 0; }
            const V* p = reinterpret_cast<const V*>(stack) + v;
            for (int g = 0; g < k; ++g) {
                const V x = p[(int64_t)g * nvec];
                const T* xs = reinterpret_cast<const T*>(&x);
#pragma unroll
                for (int j = 0; j < N; ++j) accum<T, ERR>(xs[j], flagA, sum[j], cnt[j]);
            }
            V r;
            T* rs = reinterpret_cast<T*>(&r);
#pragma unroll
            for (int j = 0; j < N; ++j) rs[j] = finish<T, ERR>(sum[j], cnt[j]);
            reinterpret_cast<V*>(out)[v] = r;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            T sum = T(0);
            unsigned cnt = 0;
            for (int g = 0; g < k; ++g) accum<T, ERR>(stack[(int64_t)g * n + i], flagA, sum, cnt);
            out[i] = finish<T, ERR>(sum, cnt);
        }
    }
}

template <typename T, bool ERR>
int launch(oisat_ctx* h, const char* name, const void* stack, int k, int64_t n, int flag, void* out) {
    // vector path: every granule row (and the output) must start 16-byte aligned
    const bool aligned = (n % Vec<T>::N) == 0 && ((uintptr_t)stack % 16) == 0 && ((uintptr_t)out % 16) == 0;
    const int64_t items = aligned ? n / Vec<T>::N : n;
    const int grid = stream_grid(items, 256);
    OISAT_LAUNCH(h, name, (stack_reduce_kernel<T, ERR>), dim3(grid), dim3(256), 0, (const T*)stack, k, n, flag != 0,
                 aligned, (T*)out);
    return OISAT_OK;
}

}  // namespace

extern "C" int oisat_nanmean_stack(oisat_ctx* h, int dtype, const void* stack, int k, int64_t n, int inf_to_nan, void* out) {
    ARG_CHECK(h && stack && out && k > 0 && n > 0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    if (dtype == OISAT_F32) return launch<float, false>(h, "nanmean_stack", stack, k, n, inf_to_nan, out);
    return launch<double, false>(h, "nanmean_stack", stack, k, n, inf_to_nan, out);
}

extern "C" int oisat_error_average(oisat_ctx* h, int dtype, const void* stack, int k, int64_t n, int square_input, void* out) {
    ARG_CHECK(h && stack && out && k > 0 && n > 0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    if (dtype == OISAT_F32) return launch<float, true>(h, "error_average", stack, k, n, square_input, out);
    return launch<double, true>(h, "error_average", stack, k, n, square_input, out);
}

// ---- device-resident month (oisatgmi/month.py) ------------------------------------------------------------------------
// The same reductions as above, but granule by granule: a running per-cell (sum, count) of the accumulator type T for each
// of the five averaged fields, updated in granule order with accum<T, ERR> and closed with finish<T, ERR>.  Starting from
// T(0) and adding the granules in the order the stack above would hold them gives the bits of stack_reduce_kernel.
// Accumulator block: sums [5][n] of T, then counts [5][n] of uint32.  Field f uses the flag averaging() uses for it:
// 0 vcd (mean, inf -> NaN), 1 uncertainty (error kind, squared), 2 ctm_vcd, 3 new_amf, 4 old_amf (plain mean).
namespace {

constexpr int kMonthFields = 5;

struct MonthIn {
    const void* p[kMonthFields];
};

template <typename T>
__device__ __forceinline__ T load_as(const void* p, bool f32, int64_t i) {
    return f32 ? (T)(static_cast<const float*>(p)[i]) : (T)(static_cast<const double*>(p)[i]);
}

// four consecutive elements (index 4v .. 4v+3) of a float32 or float64 field, converted to T: one 16-byte load for
// float32, two for float64 (the caller guarantees 16-byte aligned pointers)
template <typename T>
__device__ __forceinline__ void load4_as(const void* p, bool f32, int64_t v, T out[4]) {
    if (f32) {
        const float4 x = static_cast<const float4*>(p)[v];
        out[0] = (T)x.x; out[1] = (T)x.y; out[2] = (T)x.z; out[3] = (T)x.w;
    } else {
        const double2 a = static_cast<const double2*>(p)[2 * v];
        const double2 b = static_cast<const double2*>(p)[2 * v + 1];
        out[0] = (T)a.x; out[1] = (T)a.y; out[2] = (T)b.x; out[3] = (T)b.y;
    }
}

template <typename T, int F>
__device__ __forceinline__ void accum_field(T v, T& sum, unsigned& cnt) {
    if (F == 1) accum<T, true>(v, true, sum, cnt);
    else accum<T, false>(v, F == 0, sum, cnt);
}

template <typename T, int F>
__device__ __forceinline__ void month_field_vec(const MonthIn& in, int f32_mask, int64_t n, int64_t v, T* __restrict__ sums,
                                                unsigned* __restrict__ cnts) {
    using V = typename Vec<T>::type;
    T x[4];
    load4_as<T>(in.p[F], (f32_mask >> F) & 1, v, x);
    constexpr int VN = Vec<T>::N;                       // 4 floats or 2 doubles per 16-byte access
    V* sv = reinterpret_cast<V*>(sums + (int64_t)F * n) + (4 / VN) * v;
    V sl[4 / VN];
#pragma unroll
    for (int j = 0; j < 4 / VN; ++j) sl[j] = sv[j];
    T* s = reinterpret_cast<T*>(sl);
    uint4* cv = reinterpret_cast<uint4*>(cnts + (int64_t)F * n) + v;
    const uint4 c = *cv;
    unsigned cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) accum_field<T, F>(x[j], s[j], cc[j]);
#pragma unroll
    for (int j = 0; j < 4 / VN; ++j) sv[j] = sl[j];
    *cv = make_uint4(cc[0], cc[1], cc[2], cc[3]);
}

template <typename T, int F>
__device__ __forceinline__ void month_field(const MonthIn& in, int f32_mask, int64_t n, int64_t i, T* __restrict__ sums,
                                            unsigned* __restrict__ cnts) {
    T s = sums[(int64_t)F * n + i];
    unsigned c = cnts[(int64_t)F * n + i];
    accum_field<T, F>(load_as<T>(in.p[F], (f32_mask >> F) & 1, i), s, c);
    sums[(int64_t)F * n + i] = s;
    cnts[(int64_t)F * n + i] = c;
}

template <typename T>
__global__ __launch_bounds__(256) void month_accumulate_kernel(MonthIn in, int f32_mask, int64_t n, const int32_t* __restrict__ kept,
                                                               bool aligned, T* __restrict__ sums, unsigned* __restrict__ cnts) {
    if (*kept == 0) return;                             // skipped granule (all-NaN vcd): the launch is a no-op
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (aligned) {
        for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n / 4; v += stride) {
            month_field_vec<T, 0>(in, f32_mask, n, v, sums, cnts);
            month_field_vec<T, 1>(in, f32_mask, n, v, sums, cnts);
            month_field_vec<T, 2>(in, f32_mask, n, v, sums, cnts);
            month_field_vec<T, 3>(in, f32_mask, n, v, sums, cnts);
            month_field_vec<T, 4>(in, f32_mask, n, v, sums, cnts);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            month_field<T, 0>(in, f32_mask, n, i, sums, cnts);
            month_field<T, 1>(in, f32_mask, n, i, sums, cnts);
            month_field<T, 2>(in, f32_mask, n, i, sums, cnts);
            month_field<T, 3>(in, f32_mask, n, i, sums, cnts);
            month_field<T, 4>(in, f32_mask, n, i, sums, cnts);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void month_finish_kernel(const T* __restrict__ sums, const unsigned* __restrict__ cnts, int64_t n,
                                                           T* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
#pragma unroll
        for (int f = 0; f < kMonthFields; ++f) {
            const int64_t k = (int64_t)f * n + i;
            out[k] = f == 1 ? finish<T, true>(sums[k], cnts[k]) : finish<T, false>(sums[k], cnts[k]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void any_not_nan_kernel(const T* __restrict__ x, int64_t n, int32_t* __restrict__ kept) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) any |= (x[i] == x[i]);
    if (any) *kept = 1;                                 // every writer writes the same 1: no ordering needed
}

__global__ __launch_bounds__(256) void widen_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (double)x[i];
}

}  // namespace

extern "C" int oisat_month_accumulate(oisat_ctx* h, int acc_dtype, const void* vcd, const void* uncertainty, const void* ctm_vcd,
                                      const void* new_amf, const void* old_amf, int f32_mask, int64_t n, const int32_t* kept, void* acc) {
    ARG_CHECK(h && vcd && uncertainty && ctm_vcd && new_amf && old_amf && kept && acc && n > 0);
    ARG_CHECK(acc_dtype == OISAT_F32 || acc_dtype == OISAT_F64);
    ARG_CHECK(f32_mask >= 0 && f32_mask < (1 << kMonthFields));
    const MonthIn in = {{vcd, uncertainty, ctm_vcd, new_amf, old_amf}};
    bool aligned = (n % 4) == 0 && ((uintptr_t)acc % 16) == 0;
    for (int f = 0; f < kMonthFields; ++f) aligned = aligned && ((uintptr_t)in.p[f] % 16) == 0;
    const int grid = stream_grid(aligned ? n / 4 : n, 256);
    if (acc_dtype == OISAT_F32) {
        float* sums = (float*)acc;
        OISAT_LAUNCH(h, "month_accumulate", (month_accumulate_kernel<float>), dim3(grid), dim3(256), 0, in, f32_mask, n, kept,
                     aligned, sums, (unsigned*)(sums + kMonthFields * n));
    } else {
        double* sums = (double*)acc;
        OISAT_LAUNCH(h, "month_accumulate", (month_accumulate_kernel<double>), dim3(grid), dim3(256), 0, in, f32_mask, n, kept,
                     aligned, sums, (unsigned*)(sums + kMonthFields * n));
    }
    return OISAT_OK;
}

extern "C" int oisat_month_finish(oisat_ctx* h, int acc_dtype, const void* acc, int64_t n, void* out) {
    ARG_CHECK(h && acc && out && n > 0);
    ARG_CHECK(acc_dtype == OISAT_F32 || acc_dtype == OISAT_F64);
    const int grid = stream_grid(n, 256);
    if (acc_dtype == OISAT_F32) {
        const float* sums = (const float*)acc;
        OISAT_LAUNCH(h, "month_finish", (month_finish_kernel<float>), dim3(grid), dim3(256), 0, sums,
                     (const unsigned*)(sums + kMonthFields * n), n, (float*)out);
    } else {
        const double* sums = (const double*)acc;
        OISAT_LAUNCH(h, "month_finish", (month_finish_kernel<double>), dim3(grid), dim3(256), 0, sums,
                     (const unsigned*)(sums + kMonthFields * n), n, (double*)out);
    }
    return OISAT_OK;
}

extern "C" int oisat_all_nan(oisat_ctx* h, int dtype, const void* x, int64_t n, int32_t* kept) {
    ARG_CHECK(h && x && kept && n > 0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    HIP_TRY(hipMemsetAsync(kept, 0, sizeof(int32_t), h->stream));
    const int grid = stream_grid(n, 256);
    if (dtype == OISAT_F32) {
        OISAT_LAUNCH(h, "all_nan", (any_not_nan_kernel<float>), dim3(grid), dim3(256), 0, (const float*)x, n, kept);
    } else {
        OISAT_LAUNCH(h, "all_nan", (any_not_nan_kernel<double>), dim3(grid), dim3(256), 0, (const double*)x, n, kept);
    }
    return OISAT_OK;
}

extern "C" int oisat_widen(oisat_ctx* h, const float* x, int64_t n, double* out) {
    ARG_CHECK(h && x && out && n > 0);
    OISAT_LAUNCH(h, "widen", widen_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, x, n, out);
    return OISAT_OK;
}
