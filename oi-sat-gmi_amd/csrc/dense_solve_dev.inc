// Device code shared by the solve-phase kernels (dense_cov.hip) and the task-graph launch (dense_dag.inc, which runs a
// system's residuals and increment as tasks of the same persistent launch that factors it): the latitude window, the
// bounding-sphere cull, and the bodies of the float64 residual and of the increment as functions of a block index and a
// carve-out of the caller's LDS.  Included inside the anonymous namespace of dense_cov.hip, dense_dag.hip, dense_solve.hip and dense_tables.hip
// (host rules), dense_functional.hip (window, cull, corr_f64), dense_post.hip and buddy.hip (correlation functions); expects dense_switches.h at file scope before it; no kernels here.
// (No reference counterpart: the dense analysis is the north-star extension, SURVEY.md section 8 a-ext.)
#ifndef OISAT_DENSE_SWITCHES_H
#error "include dense_switches.h at file scope before dense_solve_dev.inc: this file is included inside a namespace and cannot"
#endif

constexpr float kLog2e = 1.4426950408889634f;                   // (a FLOAT: cut-off chords and fp32 scales only; the float64 increment takes kLog2eD)
// A pair of points whose correlation is below 2^-kCutBits is left out of the float64 sums (residual, increment): 2^-52 is the
// last bit of a term of correlation 1, and a sum's terms cancel to ~1/500 of their absolute sum at swath densities, so what
// is dropped stays below 1e-12 of the result (rounds 1-3 used 2^-64: 19 % more pairs for nothing measurable).
constexpr double kCutBits = 52.0;
// The far tier of the Gaussian's float64 sums (increment, compact-block residual): an observation whose correlation with EVERY
// point of a workgroup's block is below 2^-kSolveFarBits is evaluated in fp32 -- coordinates, |p - q|^2, v_exp_f32, product --
// into an fp32 partial sum per flush of the staging buffer, which is then added to the double accumulator.  Such a term is at
// most 2^-bits of a near one, so its fp32 relative error (~2e-5: the coordinates' rounding through the argument, v_exp_f32's
// ulp) is 2^-bits 2e-5 of a near term.  Gaspari-Cohn has no far tier.  On by default in the increment; the residual has it
// behind the variable only (far_chord_of).  OISAT_SOLVE_FAR_BITS=<b> (read at every call): 0 = off, every pair in float64, the
// bits of the code before the tier; up to 52 = the tier at 2^-b in both kernels (at 52 the far radius is the cull's own or just
// beyond it: the tier's code runs and its list stays empty).  The value is a measurement, by the protocol of kFactorFarBits
// (profiles/EXPERIMENTS.md, "The solve phase's far tier"): on four months 16 bits is the smallest value that leaves the refinement's residuals (three digits) and the fp32
// fields (one ulp of the largest entry, fewer elements than the factor's two schedules move) where they were; but the FLOAT64
// fields of oisat_apply_increment are held to 1e-13 of their largest entry against the sum over every pair
// (tests/test_gpu_parity.py: test_latitude_window_equals_the_full_sum), which 20 bits miss by a factor 3 and 24 bits meet:
// 24 is the smallest admissible value, kept with 4 bits of headroom.
constexpr double kSolveFarBits = 28.0;

// ---- the correlation model ------------------------------------------------------------------------------------------
// KIND = OISAT_CORR_GAUSSIAN (0): C = exp(-g d^2), d = |p - q| the chord.  KIND = OISAT_CORR_GASPARI_COHN (1): the compactly
// supported fifth-order piecewise rational of Gaspari and Cohn (1999, eq. 4.10) in z = d / c, half-support c = L sqrt(10/3)
// (the Gaussian's curvature at d = 0), i.e. z^2 = 0.6 g d^2; exactly 0 from z = 2 on.  Positive definite in R^3, hence on the
// sphere with chord distance (dense_cov.hip, head).  Every kernel that evaluates a correlation is a template on KIND and takes
// ONE scale next to d^2: what its Gaussian form has always taken (g, or g2 = g log2 e where it uses exp2) or kz2 = 0.6 g.
constexpr double kGcZ2PerG = 0.6;
// KIND = OISAT_CORR_SOAR (3): the second-order autoregressive function, the Matern function of nu = 3/2, C = (1 + s) exp(-s) with
// s = d sqrt(2 g) = distance / L (the Gaussian's curvature at d = 0: C ~ 1 - g d^2).  Positive definite in R^3, hence on the sphere
// with chord distance; once mean-square differentiable, exponential tails: 2^-52 at s = 39.75 where the Gaussian is there at
// 8.49 L.  Its scale is s^2 / d^2 = 2 g, or 2 g (log2 e)^2 where the kernel uses exp2: then s' = sqrt(a d^2) = s log2 e and
// C = fma(s', ln 2, 1) 2^-s'.  No far tier, no parameter besides g.
constexpr double kLog2eD = 1.4426950408889634;
constexpr double kLn2D = 0.6931471805599453;
// what a kernel of model `kind` takes in the place of the Gaussian's g2 = g log2 e / of the Gaussian's g
static inline double corr_scale2(int kind, double g) {
    if (kind == OISAT_CORR_SOAR) return 2.0 * g * (kLog2eD * kLog2eD);
    return kind == OISAT_CORR_GASPARI_COHN ? kGcZ2PerG * g : g * (double)kLog2e;
}
// ... and what the FLOAT64 increment takes: the Gaussian's g2 with log2 e in double.  (The scale above serves the fp32 kernels --
// the build of S, the probes -- which round it to float; the increment took it too, and the float constant put its exponent
// 1.3e-8 off: the increment of a correlation length 7e-9 longer.  The fp32 kernels keep theirs, so S keeps its bits.)
static inline double corr_scale2_f64(int kind, double g) {
    return kind == OISAT_CORR_GAUSSIAN ? g * kLog2eD : corr_scale2(kind, g);
}
static inline double corr_scale(int kind, double g) {
    if (kind == OISAT_CORR_SOAR) return 2.0 * g;
    return kind == OISAT_CORR_GASPARI_COHN ? kGcZ2PerG * g : g;
}

// Both branches in Horner form and a select: a wave's 64 pairs straddle all three ranges.  (z = 0: the far branch is -inf /
// NaN and not selected.)  Rounding noise below 0 next to z = 2 is clamped.
__device__ __forceinline__ float gc_f32(float kz2, float d2) {
    const float z2 = kz2 * d2;
    const float z = __builtin_amdgcn_sqrtf(z2);                             // one v_sqrt_f32 ...
    const float rz = __builtin_amdgcn_rcpf(z);                              // ... and one v_rcp_f32 (the 2 / (3 z) term)
    const float nearv = ((((-0.25f * z + 0.5f) * z + 0.625f) * z - 1.6666666666666667f) * z2) + 1.0f;
    const float farv = (((((0.083333333333333333f * z - 0.5f) * z + 0.625f) * z + 1.6666666666666667f) * z - 5.0f) * z + 4.0f) - 0.66666666666666667f * rz;
    const float c = z <= 1.0f ? nearv : farv;
    return z < 2.0f ? fmaxf(c, 0.0f) : 0.0f;
}
__host__ __device__ inline double gc_f64(double kz2, double d2) {
    const double z2 = kz2 * d2;
    const double z = sqrt(z2);
#if defined(__HIP_DEVICE_COMPILE__)
    double rz = __builtin_amdgcn_rcp(z);                                    // v_rcp_f64 and two Newton steps: full precision,
    rz = __builtin_fma(__builtin_fma(-z, rz, 1.0), rz, rz);                 // cheaper than the division's scale / fix-up
    rz = __builtin_fma(__builtin_fma(-z, rz, 1.0), rz, rz);
#else
    const double rz = 1.0 / z;
#endif
    const double nearv = ((((-0.25 * z + 0.5) * z + 0.625) * z - 1.6666666666666667) * z2) + 1.0;
    const double farv = (((((0.083333333333333333 * z - 0.5) * z + 0.625) * z + 1.6666666666666667) * z - 5.0) * z + 4.0) - 0.66666666666666667 * rz;
    const double c = z <= 1.0 ? nearv : farv;
    return z < 2.0 ? (c > 0.0 ? c : 0.0) : 0.0;
}

// the models the library knows (include/oisat.h: 2 is unassigned)
static inline bool corr_kind_ok(int kind) { return kind == OISAT_CORR_GAUSSIAN || kind == OISAT_CORR_GASPARI_COHN || kind == OISAT_CORR_SOAR; }

// SOAR in fp32: one v_sqrt_f32, one v_exp_f32, one fma, one multiply; no division, no branch (d2 = 0: sqrt 0, 2^-0, exactly 1)
__device__ __forceinline__ float soar_f32(float a, float d2) {
    const float sp = __builtin_amdgcn_sqrtf(a * d2);                         // s log2 e
    return __builtin_fmaf(sp, (float)kLn2D, 1.0f) * __builtin_amdgcn_exp2f(-sp);
}

template <bool FULL> __device__ __forceinline__ double exp2_neg(double x);
// fp32 (the build of S, the rows of H B): a = g2 | kz2 | 2 g (log2 e)^2
template <int KIND>
__device__ __forceinline__ float corr_f32(float a, float d2) {
    if (KIND == OISAT_CORR_GASPARI_COHN) return gc_f32(a, d2);
    if (KIND == OISAT_CORR_SOAR) return soar_f32(a, d2);
    return __builtin_amdgcn_exp2f(-a * d2);
}
// float64 (the residual): a = g | kz2 | 2 g
template <int KIND>
__host__ __device__ inline double corr_f64(double a, double d2) {
    if (KIND == OISAT_CORR_GASPARI_COHN) return gc_f64(a, d2);
    if (KIND == OISAT_CORR_SOAR) {
        const double s = sqrt(a * d2);
        return (1.0 + s) * exp(-s);
    }
    return exp(-a * d2);
}
// float64 (the increment): a = g2 | kz2 | 2 g (log2 e)^2
template <int KIND>
__device__ __forceinline__ double corr_f64_exp2(double a, double d2) {
    if (KIND == OISAT_CORR_GASPARI_COHN) return gc_f64(a, d2);
    if (KIND == OISAT_CORR_SOAR) {
        const double sp = sqrt(a * d2);
        return __builtin_fma(sp, kLn2D, 1.0) * exp2_neg<true>(-sp);
    }
    return exp2_neg<false>(-a * d2);                                        // (the Gaussian: its far tier's share sets the precision)
}

// ---- host: the chord at which the correlation has fallen to 2^-bits -------------------------------------------------------
// Gaussian: sqrt(bits / g2).  Gaspari-Cohn: by bisection on z in [0, 2] (C falls monotonically there), the upper end of the
// last bracket, never beyond the support chord 2 / sqrt(0.6 g); from kCutBits on it IS the support chord: the float64 sums
// then leave out nothing.  SOAR: by bisection on s for (1 + s) exp(-s) = 2^-bits (C falls monotonically; the root lies below
// bits ln 2 + ln(1 + s) < 2 bits + 2), the upper end of the last bracket too; NOT clamped to the sphere's diameter: from
// L ~ 321 km on the 2^-52 chord is 2 or more and lat_window_deg windows nothing.  Every window, envelope and cull of the library
// derives its chord here.
static inline double cut_chord(int kind, double g, double bits) {
    if (kind == OISAT_CORR_SOAR) {
        const double lt = -bits * kLn2D;                                    // ln of the target: log1p(s) - s <= lt beyond the root
        double lo = 0.0, hi = 2.0 * bits + 2.0;
        for (int it = 0; it < 100; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (log1p(mid) - mid > lt) lo = mid; else hi = mid;
        }
        return hi / sqrt(2.0 * g);
    }
    if (kind != OISAT_CORR_GASPARI_COHN) return sqrt(bits / (g * (double)kLog2e));
    double hi = 2.0;
    if (bits < kCutBits) {
        const double target = exp2(-bits);
        double lo = 0.0;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (gc_f64(1.0, mid * mid) > target) lo = mid; else hi = mid;
        }
    }
    return hi / sqrt(kGcZ2PerG * g);
}

// ---- latitude window ----------------------------------------------------------------------------------
// The correlation is below 2^-kCutBits once the chord d exceeds cut_chord(): such a pair changes a double sum by less than its
// last bit times the cancellation factor (Gaspari-Cohn: by nothing), and two points whose latitudes differ by more than the
// matching angle are at least that far apart.  With the observations sorted by latitude the pairs worth evaluating for a block
// of rows / cells are therefore one contiguous index range, found by two binary searches.  (3.6x fewer pairs at L = 300 km.)
static inline double lat_window_deg(int kind, double g, double bits = kCutBits) {
    const double chord = cut_chord(kind, g, bits);
    return chord >= 2.0 ? 1e9 : 2.0 * asin(0.5 * chord) * 57.29577951308232;
}

__device__ __forceinline__ int64_t lower_bound_lat(const double* __restrict__ a, int64_t n, double v) {   // first i with a[i] >= v
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- culling by distance (round 3) -------------------------------------------------------------------------------------
// The latitude window keeps one contiguous range of the (latitude-ordered) observations per block of cells, but in
// longitude it keeps everything: at L = 300 km and 0.25 deg most of the pairs it leaves are still further apart than the
// chord at which 2^x < 2^-kCutBits (a polar cap's cells see every observation of the cap's band, all around the pole).  The
// increment kernel therefore gives its block of cells -- a compact PATCH of the grid -- a bounding sphere: centre c (normalised
// mean of its points), radius rho (largest chord to c), and, while it stages the candidates of the window into LDS, keeps only
// the observations with |q - c| <= cut + rho (|p - q| >= |q - c| - |p - c|: nothing closer than the cut-off is dropped).  A
// test per (block, observation) instead of an exponential per (cell, observation); no latitudes, longitudes, poles or date
// line in it.  The survivors are compacted in candidate order (wave ballots), so the sums keep a fixed order.
// (The residual kernel's blocks are 64 consecutive observations in LATITUDE order -- all around the globe in longitude -- so a
// sphere around them culls nothing; it keeps the plain window.)
// a block-uniform double, moved to scalar registers (the far tier's radius beside the four words every thread already holds)
__device__ __forceinline__ double uniform_f64(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// r2far: the far tier's squared radius, (chord(kSolveFarBits) + rho)^2 with the cull's safety margins: an observation at least
// that far from c is at least chord(bits) from every point of the block.  +inf (nothing is far) where there is no cull (no
// centre, no window), where the tier is off (far_chord = +inf: far_chord_of) and for every model but the Gaussian.
struct BlockSphere { double cx, cy, cz, r2cull, r2far; };

// centre and cull radius of the block's live points (px, py, pz per thread and slot; every thread calls this)
template <int SLOTS>
__device__ __forceinline__ BlockSphere block_sphere(const double (&px)[SLOTS], const double (&py)[SLOTS], const double (&pz)[SLOTS],
                                                    const bool (&live)[SLOTS], double cut_chord, double far_chord,
                                                    double* __restrict__ red /*[16] shared*/) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q)
        if (live[q]) { sx += px[q]; sy += py[q]; sz += pz[q]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sx += __shfl_xor(sx, o, kWave);
        sy += __shfl_xor(sy, o, kWave);
        sz += __shfl_xor(sz, o, kWave);
    }
    __syncthreads();
    if (lane == 0) { red[w] = sx; red[4 + w] = sy; red[8 + w] = sz; }
    __syncthreads();
    sx = (red[0] + red[1]) + (red[2] + red[3]);
    sy = (red[4] + red[5]) + (red[6] + red[7]);
    sz = (red[8] + red[9]) + (red[10] + red[11]);
    const double nrm = sqrt(sx * sx + sy * sy + sz * sz);
    BlockSphere b;
    if (!(nrm > 1e-9)) {                                        // points all around the sphere (or none): keep everything
        b.cx = b.cy = b.cz = 0.0;
        b.r2cull = 1e30;
        b.r2far = __builtin_inf();
        return b;
    }
    b.cx = sx / nrm; b.cy = sy / nrm; b.cz = sz / nrm;
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q)
        if (live[q]) {
            const double dx = px[q] - b.cx, dy = py[q] - b.cy, dz = pz[q] - b.cz;
            r2 = fmax(r2, dx * dx + dy * dy + dz * dz);
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) r2 = fmax(r2, __shfl_xor(r2, o, kWave));
    __syncthreads();
    if (lane == 0) red[12 + w] = r2;
    __syncthreads();
    r2 = fmax(fmax(red[12], red[13]), fmax(red[14], red[15]));
    const double rr = cut_chord + sqrt(r2) * (1.0 + 1e-12) + 1e-12;
    b.r2cull = cut_chord < 1e9 ? rr * rr : 1e30;
    const double rf = far_chord + sqrt(r2) * (1.0 + 1e-12) + 1e-12;
    b.r2far = uniform_f64(cut_chord < 1e9 && far_chord < 1e9 ? rf * rf : __builtin_inf());
    return b;
}

constexpr int kStage = 768;                                     // staged observations: processed once 512 have gathered

// one pass of 256 candidates [c0, c0 + 256) /\ [.., j1): the near ones go to buf[fill ..) in candidate order; returns the new fill.
// FAR (the Gaussian's far tier): the survivors at least sqrt(bs.r2far) from the centre go to a second list instead, float4
// {x, y, z, sig * z_solve}, in candidate order too and by the same ballots and prefix sums (a wave's two counts share one word
// of wcnt: near in the low half, far in the high half; neither passes 64, no sum of them 256).  The far list grows from the BACK
// of the same buffer, in the slots the near list has not reached: entry k is the 16 bytes of bzw[kStage - 1 - k / 2] (k even) or
// bxy[kStage - 1 - k / 2] (k odd) -- far_entry().  A near entry takes one slot of either array, two far entries take one of
// either, so the lists fit while 2 near + far <= 2 kStage = 1536; a pass adds at most 256 survivors, i.e. at most 512 to that
// weight, hence the callers' flush rule: process both lists once 2 near + far >= 1024 (with an empty far list: near >= 512,
// the rule before the tier), or behind the last pass.  A rule of the counts alone: the sums' order does not depend on timing.
template <bool FAR>
__device__ __forceinline__ int stage_near(const double* __restrict__ oxyz, const double* __restrict__ osig, const double* __restrict__ z,
                                          int64_t m, int64_t c0, int64_t j1, const BlockSphere& bs, double2* __restrict__ bxy,
                                          double2* __restrict__ bzw, int fill, int& ffill, int* __restrict__ wcnt /*[4] shared*/) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t c = c0 + t;
    double x = 0.0, y = 0.0, zz = 0.0;
    bool near = false, far = false;
    if (c < j1) {
        x = oxyz[c]; y = oxyz[m + c]; zz = oxyz[2 * m + c];
        const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
        const double q2 = dx * dx + dy * dy + dz * dz;
        near = q2 <= bs.r2cull;
        if (FAR) {
            far = near && q2 >= bs.r2far;
            near = near && !far;
        }
    }
    const unsigned long long mask = __ballot(near);
    const unsigned long long fmask = FAR ? __ballot(far) : 0ull;
    if (lane == 0) wcnt[w] = FAR ? (__popcll(mask) | (__popcll(fmask) << 16)) : __popcll(mask);
    __syncthreads();
    const int c0w = wcnt[0], c1w = wcnt[1], c2w = wcnt[2], c3w = wcnt[3];
    const int before = (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0);
    const int base = fill + (FAR ? (before & 0xffff) : before);
    if (near) {
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        bxy[pos] = make_double2(x, y);
        bzw[pos] = make_double2(zz, osig[c] * z[c]);
    }
    if (FAR && far) {
        const int k = ffill + (before >> 16) + __popcll(fmask & ((1ull << lane) - 1ull));
        reinterpret_cast<float4*>((k & 1) ? bxy : bzw)[kStage - 1 - (k >> 1)] = make_float4((float)x, (float)y, (float)zz, (float)(osig[c] * z[c]));
    }
    __syncthreads();
    const int all = c0w + c1w + c2w + c3w;
    if (FAR) {
        ffill += all >> 16;
        return fill + (all & 0xffff);
    }
    return fill + all;
}
// the two lists are due: see stage_near
template <bool FAR>
__device__ __forceinline__ bool stage_full(int fill, int ffill) { return FAR ? 2 * fill + ffill >= 1024 : fill >= 512; }
// far entry k of the staging buffer (stage_near)
__device__ __forceinline__ float4 far_entry(const double2* __restrict__ bxy, const double2* __restrict__ bzw, int k) {
    return reinterpret_cast<const float4*>((k & 1) ? bxy : bzw)[kStage - 1 - (k >> 1)];
}

// Two far pairs in packed fp32 (v_pk_add / v_pk_mul / v_pk_fma_f32, two v_exp_f32): sum + 2^(-g2 |p - q|^2) w per lane.  The lanes
// are the thread's two cells against one observation (increment, CELLS = 2) or one point against two observations.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 far_pairs(f32x2 dx, f32x2 dy, f32x2 dz, float g2, f32x2 w, f32x2 sum) {
    const f32x2 x = (dx * dx + dy * dy + dz * dz) * -g2;
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(x.x);
    e.y = __builtin_amdgcn_exp2f(x.y);
    return e * w + sum;
}
// one point (ax, ay, az) against far entries o0 and o1
__device__ __forceinline__ f32x2 far_pairs_of(float ax, float ay, float az, const float4& o0, const float4& o1, float g2, f32x2 sum) {
    const f32x2 dx = {ax - o0.x, ax - o1.x}, dy = {ay - o0.y, ay - o1.y}, dz = {az - o0.z, az - o1.z}, w = {o0.w, o1.w};
    return far_pairs(dx, dy, dz, g2, w, sum);
}
// v, opaque to the optimiser: what a far loop derives from it (fp32 copies of the coordinates, LDS addresses) is formed where the
// loop runs, once per flush, and does not sit in registers across the float64 loop, whose occupancy the far tier must not cost.
// Nothing but the compiler's register allocation depends on these: a compiler that hoists across them anyway costs waves, not
// bits.  If `make asm` shows the Gaussian apply_increment_kernel above 96 VGPRs (two cells) / 80 (one) or
// cov_residual_blocks_kernel above 80 -- occupancy 5 / 6 / 6, recorded in profiles/EXPERIMENTS.md -- look here and at
// uniform_f64 first: the values to keep out of the float64 loops' live ranges are fx, fy, fz, g2 and the far list's addresses.
__device__ __forceinline__ double far_local(double v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ int far_local(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ int far_local_uniform(int v) { asm volatile("" : "+s"(v)); return v; }

// 2^x for x <= 0 in double: x = n + f, |f| <= 1/2, 2^f = 1 + f q(f) with q a polynomial in f (the Chebyshev interpolant of
// (2^f - 1) / f on that range -- FULL: of 2^f itself, whose constant term rounds to 1 -- with ln 2 in its coefficients; exactly 1 at
// f = 0), 2^n by ldexp.
// FULL: q of degree 10, 2e-17 from 2^f with these rounded coefficients -- what is left is the rounding of the last Horner steps, one
// unit in the last place.  SOAR takes it: nothing else in its increment is coarser than float64.
// !FULL: q of degree 8, 3.7e-14 of a term at the most.  The Gaussian takes it: its far tier (kSolveFarBits) already allows a term
// 2^-28 x 2e-5 = 7.5e-14 of a term of correlation 1, a far observation has the one error and a near one the other, and three more
// fused multiply-adds per pair cost the benchmark's increment 0.6 ms of 5 (profiles/EXPERIMENTS.md, "Batched solve at the ABI").
// (Up to the tests of the batched calls at the ABI both took the degree-8 Taylor polynomial of e^t in t = f ln 2, 2e-10 of a term:
// 1e2 .. 4e4 times the float64 bound those tests hold the increment to.)
// The far tier's share is the DEFAULT tier's: with OISAT_SOLVE_FAR_BITS = 0 (no tier) or a tighter one the near terms keep their 3.7e-14
// and that argument no longer covers them -- the increment is then good to 3.7e-14 of a term, not to float64 rounding.
// No clamp of x (there was one at -1100).  n is converted by v_cvt_i32_f64 itself, which SATURATES (the instruction's definition;
// a C++ cast of an out-of-range double would be undefined): |x| = g2 |p - q|^2 passes 2^31 in the L -> 0 limit that the
// element-wise parity tests drive the dense analysis to, n then becomes INT_MIN, and ldexp gives 0 for every n below -1075 -- far
// pairs outside any window: 2^x = 0.  A NaN x (a NaN coordinate) gives NaN; under the clamp it gave 0.
__device__ __forceinline__ int cvt_i32_saturating(double v) {
    int i;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(i) : "v"(v));
    return i;
}
template <bool FULL>
__device__ __forceinline__ double exp2_neg(double x) {
    const double n = __builtin_rint(x);
    const double f = x - n;                                                 // |f| <= 1/2, exact
    double p;
    if (FULL) {
        p = 4.4558179124523303e-10;
        p = __builtin_fma(p, f, 7.07419430501114e-09);
        p = __builtin_fma(p, f, 1.0178057087710788e-07);
        p = __builtin_fma(p, f, 1.3215432535868937e-06);
        p = __builtin_fma(p, f, 1.5252733841556817e-05);
        p = __builtin_fma(p, f, 0.0001540353046372444);
        p = __builtin_fma(p, f, 0.001333355814640647);
        p = __builtin_fma(p, f, 0.009618129107587256);
        p = __builtin_fma(p, f, 0.055504108664821625);
        p = __builtin_fma(p, f, 0.24022650695910158);
        p = __builtin_fma(p, f, 0.6931471805599453);
    } else {
        p = 1.0203121073417321e-07;
        p = __builtin_fma(p, f, 1.3255224894585756e-06);
        p = __builtin_fma(p, f, 1.5252686846230125e-05);
        p = __builtin_fma(p, f, 0.00015403455852394153);
        p = __builtin_fma(p, f, 0.001333355817904315);
        p = __builtin_fma(p, f, 0.009618129159402621);
        p = __builtin_fma(p, f, 0.055504108664760424);
        p = __builtin_fma(p, f, 0.2402265069581299);
        p = __builtin_fma(p, f, 0.6931471805599453);
    }
    p = __builtin_fma(p, f, 1.0);
    return __builtin_ldexp(p, cvt_i32_saturating(n));
}


// ---- host: which form of the residual / increment a solve takes (the same rule for the kernels of dense_cov.hip and for the
// tasks of the task-graph launch, so that the two paths do the same arithmetic) ------------------------------------------------
// chord beyond which the correlation is below 2^-kCutBits (the same cut-off as the latitude window's)
static inline double cut_chord_of(int kind, double g) { return cut_chord(kind, g, kCutBits); }
// chord from which a pair belongs to the far tier (kSolveFarBits), passed beside cut_chord_of by every launch of the increment
// and of the compact-block residual; +inf = no far tier: another model than the Gaussian, or bits = 0.  bits < 0: the library's setting, kSolveFarBits or OISAT_SOLVE_FAR_BITS.  false: the variable
// holds something else than a number in [0, 52].  default_on = false (the compact-block residual, whose tier did not earn its
// place at kSolveFarBits -- profiles/EXPERIMENTS.md): a tier only where the variable asks for one.  The chord is rounded UP to
// a float (the correlation there is no larger than 2^-bits): the task-graph launch carries it as one, in the padding of its argument block (DagSolve), and every path takes the
// same value.
static inline bool far_chord_of(int kind, double g, double* chord_out, double bits = -1.0, bool default_on = true) {
    if (bits < 0.0) {
        bits = default_on ? kSolveFarBits : 0.0;
        const int set = oisat_dense::solve_far_bits(&bits);     // (dense_switches.h)
        if (set < 0 || (set > 0 && !(bits >= 0.0 && bits <= kCutBits))) return false;
    }
    const bool on = kind == OISAT_CORR_GAUSSIAN && bits > 0.0 && bits <= kCutBits;
    *chord_out = (double)INFINITY;
    if (on) {
        const double chord = cut_chord(kind, g, bits);
        const float f = (float)chord;
        *chord_out = (double)f >= chord ? (double)f : (double)nextafterf(f, INFINITY);
    }
    return true;
}
// The compact-block residual pays where the covariance's reach is small against the domain: measured at 720x1440 / 1e5
// observations, L = 300 km (reach 2 800 km): 6.6 -> 4.6 ms; a month's 50 tiles: 1.69 -> 1.59 ms; at 360x720 / 1e4 observations,
// L = 500 km (reach 4 700 km) the staging costs more than the cull saves: 0.21 -> 0.26 ms.
// (The rule is about the reach: the Gaussian's 2^-64 chord, as measured -- the 64 below is that measurement's and did not follow
// the sums' cut-off when kCutBits went from 64 to 52; include/oisat.h says the same of oisat_cov_residual_update.  Gaspari-Cohn: the same 0.5 applied to its support
// chord; SOAR: to its 2^-52 chord (L <= 80 km) -- both reasoned from the Gaussian's figures, not measured.)
static inline bool residual_blocks_pay(int kind, double g) {
    if (kind != OISAT_CORR_GAUSSIAN) return cut_chord(kind, g, kCutBits) <= 0.5;
    return sqrt(64.0 / (g * (double)kLog2e)) <= 0.5;           // chord on the unit sphere: 3 200 km (L <= 340 km)
}
// two cells per thread share every observation fetched from LDS; with too few cells to fill the GPU that way (a polar cap:
// 338 workgroups) one cell per thread doubles the waves in flight instead
static inline int increment_cells(int cu_count, int64_t n, int nmem) {
    const int64_t wgs2 = cdiv(n, 512) * nmem;
    return wgs2 < 4 * (int64_t)(cu_count > 0 ? cu_count : 256) ? 1 : 2;
}
// workgroups of one system: patches of 32 x (8 CELLS) cells of its ny x nx grid (nx > 0) or runs of 256 CELLS cells
static inline int64_t increment_blocks(int64_t n, int64_t nx, int cells) {
    if (nx > 0) return cdiv(nx, 32) * cdiv(n / nx, 8 * cells);
    return cdiv(n, 256 * cells);
}

// ---- LDS of one workgroup running a residual block or an increment patch ------------------------------------------------
struct SolveLds {
    double2* bxy;                // [kStage] staged near observations: (x, y)            | residual by rows: sx[256], sy[256]
    double2* bzw;                // [kStage]                           (z, sig * z_solve) |                   sz[256], sw[256]
    double* part;                // [4][64] column-phase sums of the residual
    double* red;                 // [16]
    double* s_lo;                // [4]
    double* s_hi;                // [4]
    int64_t* s_j;                // [2]
    int* wcnt;                   // [4]
};
constexpr size_t kSolveLdsBytes = 2 * sizeof(double2) * kStage + sizeof(double) * (256 + 16 + 4 + 4) + sizeof(int64_t) * 2 + sizeof(int) * 4;
__device__ __forceinline__ SolveLds solve_lds_carve(void* base /* 16-byte aligned, kSolveLdsBytes */) {
    SolveLds L;
    char* p = (char*)base;
    L.bxy = (double2*)p; p += sizeof(double2) * kStage;
    L.bzw = (double2*)p; p += sizeof(double2) * kStage;
    L.part = (double*)p; p += sizeof(double) * 256;
    L.red = (double*)p; p += sizeof(double) * 16;
    L.s_lo = (double*)p; p += sizeof(double) * 4;
    L.s_hi = (double*)p; p += sizeof(double) * 4;
    L.s_j = (int64_t*)p; p += sizeof(int64_t) * 2;
    L.wcnt = (int*)p;
    return L;
}

// r[row] <- v: plain inside a kernel of its own (the next kernel reads it), write-through agent-scope store when another
// workgroup of the SAME launch reads it (task graph: cdna_hip_programming.md Guideline 16, R1 -- the caller drains and signals)
template <bool AGENT>
__device__ __forceinline__ void solve_store(double* p, double v) {
    if (AGENT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// ---- r = d - S z in double, S regenerated on the fly (iterative refinement) ----------------------
// Block `blk` = 64 rows; 256 threads = 64 rows x 4 column phases; fixed-order combine (deterministic).
// olat (optional): latitudes of the observations in degrees, ASCENDING -- the block's rows then span
// [olat[row0], olat[row_last]] and only columns inside that span +/- the window are visited.
// partial != nullptr (single system with fewer than two blocks of rows per CU): `slice` = one of nsplit slices of the
// column range; the slice's sums go to partial[slice][row] and resid_combine_kernel adds them in slice order
template <int KIND, bool AGENT>
__device__ __forceinline__ void resid_rows_block(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                 const double* __restrict__ ovar, int64_t m, double g, const double* __restrict__ d,
                                                 const double* __restrict__ z, double* __restrict__ r, const double* __restrict__ olat,
                                                 double win_deg, double* __restrict__ partial, int nsplit, int slice, int64_t blk,
                                                 const SolveLds& W) {
    double* sx = (double*)W.bxy;                               // chunk of 256 columns: coords and sig*z
    double* sy = sx + 256;
    double* sz = (double*)W.bzw;
    double* sw = sz + 256;
    double (*part)[64] = (double (*)[64])W.part;
    const int t = threadIdx.x;
    const int lr = t & 63, ph = t >> 6;
    const int64_t row = blk * 64 + lr;
    const bool live = row < m;
    const double ax = live ? oxyz[row] : 0.0, ay = live ? oxyz[m + row] : 0.0, az = live ? oxyz[2 * m + row] : 0.0;
    int64_t j0 = 0, j1 = m;
    if (olat) {                                                 // block-uniform: every thread runs the same two searches
        const int64_t r0 = blk * 64, r1 = (r0 + 63 < m - 1) ? r0 + 63 : m - 1;
        j0 = lower_bound_lat(olat, m, olat[r0] - win_deg);
        j1 = lower_bound_lat(olat, m, olat[r1] + win_deg + 1e-9);
        j0 &= ~(int64_t)255;                                    // keep the chunking aligned: same summation order per row
    }
    if (partial != nullptr) {                                   // this slice of [j0, j1), in whole chunks of 256 columns
        const int64_t chunks = (j1 - j0 + 255) >> 8, per = (chunks + nsplit - 1) / nsplit;
        const int64_t a = j0 + (int64_t)slice * per * 256, b = a + per * 256;
        j0 = a < j1 ? a : j1;
        j1 = b < j1 ? b : j1;
    }
    double acc = 0.0;
    for (int64_t c0 = j0; c0 < j1; c0 += 256) {
        const int64_t c = c0 + t;
        __syncthreads();
        if (c < m) {
            sx[t] = oxyz[c]; sy[t] = oxyz[m + c]; sz[t] = oxyz[2 * m + c];
            sw[t] = osig[c] * z[c];
        } else {
            sx[t] = 0.0; sy[t] = 0.0; sz[t] = 0.0; sw[t] = 0.0;
        }
        __syncthreads();
        for (int j = ph * 64; j < ph * 64 + 64; ++j) {
            const double dx = ax - sx[j], dy = ay - sy[j], dz = az - sz[j];
            acc += corr_f64<KIND>(g, dx * dx + dy * dy + dz * dz) * sw[j];
        }
    }
    part[ph][lr] = acc;
    __syncthreads();
    if (ph == 0 && live) {
        const double s = ((part[0][lr] + part[1][lr]) + part[2][lr]) + part[3][lr];
        if (partial != nullptr) partial[(int64_t)slice * m + row] = s;
        else solve_store<AGENT>(&r[row], d[row] - (osig[row] * s + ovar[row] * z[row]));
    }
}

// ---- the same residual on COMPACT blocks of rows (round 3) ------------------------------------------------------------
// The form above takes 64 consecutive observations of the latitude order per block: one latitude, every longitude -- its
// window keeps all observations of a latitude band around the globe.  Here `perm` lists the observations along a space-
// filling curve (the host's Morton order of latitude x longitude), so the 64 rows of a block are neighbours in space: the
// block reduces its latitude span (the candidates are still one contiguous range of the latitude order), gets a bounding
// sphere and keeps, while staging the candidates into LDS, only the observations within the covariance's reach of it -- the
// increment's cull (block_sphere / stage_near).  Per row: the same terms in the same (latitude) order, four column phases
// combined in a fixed order; terms below 2^-kCutBits of a term left out.
// Gaussian: the staged observations that are far from the whole block (stage_near<true>) are evaluated in packed fp32, every
// fourth entry of the far list per column phase like the near list, two entries per step in the two lanes of a partial sum
// that joins the phase's double sum behind each flush (lane 0, then lane 1).  far_chord = +inf: no such entry, the same bits
// as without the tier.
template <int KIND, bool AGENT>
__device__ __forceinline__ void resid_compact_block(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                    const double* __restrict__ ovar, int64_t m, double g, const double* __restrict__ d,
                                                    const double* __restrict__ z, double* __restrict__ r, const double* __restrict__ olat,
                                                    double win_deg, const int* __restrict__ perm, double cut_chord, double far_chord,
                                                    int64_t blk, const SolveLds& W) {
    constexpr bool FAR = KIND == OISAT_CORR_GAUSSIAN;
    double (*part)[64] = (double (*)[64])W.part;
    const int t = threadIdx.x;
    const int lr = t & 63, ph = t >> 6;
    const int64_t pos = blk * 64 + lr;
    const bool live = pos < m;
    const int64_t row = live ? (perm ? (int64_t)perm[pos] : pos) : 0;
    const double ax = live ? oxyz[row] : 0.0, ay = live ? oxyz[m + row] : 0.0, az = live ? oxyz[2 * m + row] : 0.0;
    if (ph == 0) {                                              // latitude span of the block's rows (wave 0 holds each row once)
        double lo = live ? olat[row] : 1e9, hi = live ? olat[row] : -1e9;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
        if (lr == 0) { W.s_lo[0] = lo; W.s_hi[0] = hi; }
    }
    __syncthreads();
    const int64_t j0 = lower_bound_lat(olat, m, W.s_lo[0] - win_deg);
    const int64_t j1 = lower_bound_lat(olat, m, W.s_hi[0] + win_deg + 1e-9);
    const double sx1[1] = {ax}, sy1[1] = {ay}, sz1[1] = {az};
    const bool lv1[1] = {live && ph == 0};
    const BlockSphere bs = block_sphere<1>(sx1, sy1, sz1, lv1, cut_chord, FAR ? far_chord : (double)INFINITY, W.red);
    double acc = 0.0;
    int fill = 0, ffill = 0;
    for (int64_t c0 = j0; c0 < j1 || fill > 0 || ffill > 0; c0 += 256) {
        if (c0 < j1) fill = stage_near<FAR>(oxyz, osig, z, m, c0, j1, bs, W.bxy, W.bzw, fill, ffill, W.wcnt);
        if (stage_full<FAR>(fill, ffill) || c0 + 256 >= j1) {  // block-uniform
            for (int j = ph; j < fill; j += 4) {                // column phase ph takes every fourth staged observation
                const double2 oxy = W.bxy[j];
                const double2 ozw = W.bzw[j];
                const double dx = ax - oxy.x, dy = ay - oxy.y, dz = az - ozw.x;
                acc += corr_f64<KIND>(g, dx * dx + dy * dy + dz * dz) * ozw.y;
            }
            if (FAR && ffill > 0) {                             // block-uniform; g is the Gaussian's: the far terms are 2^(-g2 d^2) w
                const float fx = (float)far_local(ax), fy = (float)far_local(ay), fz = (float)far_local(az);
                const float g2 = (float)(far_local(g) * (double)kLog2e);
                f32x2 fs = {0.0f, 0.0f};
                int k = far_local(ph);
                for (; k + 4 < ffill; k += 8) fs = far_pairs_of(fx, fy, fz, far_entry(W.bxy, W.bzw, k), far_entry(W.bxy, W.bzw, k + 4), g2, fs);
                if (k < ffill) {                                // an odd entry: its twin with weight 0
                    const float4 o = far_entry(W.bxy, W.bzw, k);
                    fs = far_pairs_of(fx, fy, fz, o, make_float4(o.x, o.y, o.z, 0.0f), g2, fs);
                }
                acc += (double)fs.x;
                acc += (double)fs.y;
            }
            fill = 0;
            ffill = 0;
            __syncthreads();
        }
    }
    part[ph][lr] = acc;
    __syncthreads();
    if (ph == 0 && live) {
        const double s = ((part[0][lr] + part[1][lr]) + part[2][lr]) + part[3][lr];
        solve_store<AGENT>(&r[row], d[row] - (osig[row] * s + ovar[row] * z[row]));
    }
}

// ---- the residual behind a correction as an UPDATE of the last one: out = r_prev - S dz, S dz in packed fp32 ---------------
// Behind a correction z <- z + dz the float64 residual is r_prev - S dz, and |S dz| ~ |r_prev|: a relative error e in S dz
// moves the new residual by e |r_prev|, a few 1e-5 of a vector that is itself 1e-5 |d| -- far below what the refinement's
// stopping test can see.  So every pair is evaluated the way the far tier above evaluates its own: fp32 coordinates,
// v_pk_* / v_exp_f32, fp32 partial sums per flush joined into the phase's double sum.  Gaussian only.  Geometry, latitude span,
// bounding sphere, the 2^-kCutBits cull and the candidate order are resid_compact_block's.  The survivors are staged as four
// float arrays x[], y[], z[], w[] (w = sig dz) in the bytes of bxy | bzw: kUpdStage = 1536 entries, twice the float64 lists'.
// A pass adds at most 256, hence the flush rule: evaluate once another pass might not fit (fill + 256 > kUpdStage), or behind
// the last pass -- a rule of the counts alone.  The list is padded with weight-0 entries to a multiple of 16; column phase ph
// takes the quads ph, ph + 4, ..: one 16-byte broadcast read per array, entries (0, 1) and (2, 3) of the quad in the two lanes
// of two partial sums, joined in that order.  The diagonal term and the subtraction from r_prev stay double.  Deterministic.
constexpr int kUpdStage = (int)(2 * sizeof(double2) * kStage / (4 * sizeof(float)));
// the reported residual may be this form: it is within kResidUpdateC |r_prev| of the float64 one (8x the largest error measured
// on the protocol's months and the tests' geometries, rounded up to a power of two: profiles/EXPERIMENTS.md, "The verification
// residual as an update"); the stopping test charges that bound (resid_update_check_kernel, dense_solve.hip)
constexpr double kResidUpdateC = OISAT_RESID_UPDATE_C;         // (include/oisat.h documents it to callers)
// The same argument for the INCREMENT behind a correction (dense_inc_update.inc; oisat_gain_solve_fields): delta = B H^T (z - z0) in
// packed fp32 is e |delta| (max-norm) from its float64 value, and |delta| <= |r_0| / |d| of the field's scale (|K| <= 1), so the
// fields move by e t of their largest value where |r_0| <= t |d|.  kIncUpdateT is the largest power of two t with e t <= 2^-27, a
// quarter ulp of the largest fp32 field value, for the largest e measured on the protocol's four months (profiles/EXPERIMENTS.md,
// "The increment under the correction's sweeps": e = 1.69e-4 on NO2 seed 3003, so t = 2^-15 = 3.05e-5 against first residuals of
// 3.1e-6 .. 2.6e-5); a solve whose first residual is above it takes the float64 increment of its final z.
constexpr double kIncUpdateT = OISAT_INC_UPDATE_T;             // (include/oisat.h documents it to callers)
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void resid_update_block(const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                   const double* __restrict__ ovar, int64_t m, double g,
                                                   const double* __restrict__ r_prev, const double* __restrict__ dzv,
                                                   double* __restrict__ out, const double* __restrict__ olat, double win_deg,
                                                   const int* __restrict__ perm, double cut_chord, int64_t blk, const SolveLds& W) {
    static_assert(kUpdStage % 16 == 0 && kUpdStage >= 512, "the padded list must fit");
    float* const lx = (float*)W.bxy;                            // bxy and bzw are adjacent (solve_lds_carve)
    float* const ly = lx + kUpdStage;
    float* const lz = ly + kUpdStage;
    float* const lw = lz + kUpdStage;
    double (*part)[64] = (double (*)[64])W.part;
    const int t = threadIdx.x;
    const int lr = t & 63, ph = t >> 6;
    const int64_t pos = blk * 64 + lr;
    const bool live = pos < m;
    const int64_t row = live ? (perm ? (int64_t)perm[pos] : pos) : 0;
    const double ax = live ? oxyz[row] : 0.0, ay = live ? oxyz[m + row] : 0.0, az = live ? oxyz[2 * m + row] : 0.0;
    if (ph == 0) {                                              // latitude span of the block's rows (wave 0 holds each row once)
        double lo = live ? olat[row] : 1e9, hi = live ? olat[row] : -1e9;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
        if (lr == 0) { W.s_lo[0] = lo; W.s_hi[0] = hi; }
    }
    __syncthreads();
    const int64_t j0 = lower_bound_lat(olat, m, W.s_lo[0] - win_deg);
    const int64_t j1 = lower_bound_lat(olat, m, W.s_hi[0] + win_deg + 1e-9);
    const double sx1[1] = {ax}, sy1[1] = {ay}, sz1[1] = {az};
    const bool lv1[1] = {live && ph == 0};
    const BlockSphere bs = block_sphere<1>(sx1, sy1, sz1, lv1, cut_chord, (double)INFINITY, W.red);
    const f32x2 fx = {(float)ax, (float)ax}, fy = {(float)ay, (float)ay}, fz = {(float)az, (float)az};
    const float g2 = (float)(g * (double)kLog2e);
    double acc = 0.0;
    int fill = 0;
    for (int64_t c0 = j0; c0 < j1; c0 += 256) {
        {                                                       // one pass of 256 candidates: the survivors, in candidate order
            const int lane = t & 63, w = t >> 6;
            const int64_t c = c0 + t;
            double x = 0.0, y = 0.0, zz = 0.0;
            bool near = false;
            if (c < j1) {
                x = oxyz[c]; y = oxyz[m + c]; zz = oxyz[2 * m + c];
                const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
                near = dx * dx + dy * dy + dz * dz <= bs.r2cull;
            }
            const unsigned long long mask = __ballot(near);
            if (lane == 0) W.wcnt[w] = __popcll(mask);
            __syncthreads();
            const int c0w = W.wcnt[0], c1w = W.wcnt[1], c2w = W.wcnt[2], c3w = W.wcnt[3];
            if (near) {
                const int p = fill + (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0) + __popcll(mask & ((1ull << lane) - 1ull));
                lx[p] = (float)x; ly[p] = (float)y; lz[p] = (float)zz;
                lw[p] = (float)(osig[c] * dzv[c]);
            }
            fill += c0w + c1w + c2w + c3w;                      // <= kUpdStage: a pass starts at fill <= kUpdStage - 256
            if (t < 16 && fill + t < ((fill + 15) & ~15)) {     // the padding behind the list (the next pass writes over it)
                lx[fill + t] = 0.0f; ly[fill + t] = 0.0f; lz[fill + t] = 0.0f; lw[fill + t] = 0.0f;
            }
            __syncthreads();
        }
        if (fill + 256 > kUpdStage || c0 + 256 >= j1) {        // block-uniform
            f32x2 s0 = {0.0f, 0.0f}, s1 = {0.0f, 0.0f};
#pragma unroll 2
            for (int j = 4 * ph; j < fill; j += 16) {           // this phase's quads; wave-uniform addresses: broadcast reads
                const f32x4 ox = *reinterpret_cast<const f32x4*>(lx + j), oy = *reinterpret_cast<const f32x4*>(ly + j);
                const f32x4 oz = *reinterpret_cast<const f32x4*>(lz + j), ow = *reinterpret_cast<const f32x4*>(lw + j);
                s0 = far_pairs(fx - ox.xy, fy - oy.xy, fz - oz.xy, g2, ow.xy, s0);
                s1 = far_pairs(fx - ox.zw, fy - oy.zw, fz - oz.zw, g2, ow.zw, s1);
            }
            acc += (double)s0.x;
            acc += (double)s0.y;
            acc += (double)s1.x;
            acc += (double)s1.y;
            fill = 0;
            __syncthreads();
        }
    }
    part[ph][lr] = acc;
    __syncthreads();
    if (ph == 0 && live) {
        const double s = ((part[0][lr] + part[1][lr]) + part[2][lr]) + part[3][lr];
        out[row] = r_prev[row] - (osig[row] * s + ovar[row] * dzv[row]);
    }
}

// ---- inc_i = sig_i * sum_a C(i,a) w_a, w = osig.*z ; xa = xb + inc --------------------------------------------
// Thread = CELLS grid cells, block = 256 threads; observations stream through LDS in chunks and
// are read as wave-uniform (broadcast) 16-byte words.  |p-q|^2 is formed in double: with float
// coordinates the rounding of the inputs alone (3e-8 each) moves the exponent by g*2|p-q|*3e-8 ~ 1e-6
// at the ranges that matter, and the increment -- a sum of ~1e3 such terms of both signs -- was off by
// 1.3e-5 of the field scale at 720x1440 / 1e5 obs.  v_fma_f64 issues at the unpacked fp32 rate on
// CDNA4, so this costs a few extra issue slots per pair, not a factor.  The product with sig*z and the
// running sum are double, because the terms cancel: sum|term| reaches several hundred times the field
// scale at swath densities, so fp32 partial sums alone cost ~1e-5.
// Cells of block `blk`: a 32-wide patch of the (ny x nx) grid (nx > 0: CELLS * 8 rows x 32 columns -- a compact patch has a
// small bounding sphere, 512 consecutive cells of a 1440-wide row span 128 degrees), or CELLS * 256 consecutive cells (nx <= 0).
template <int KIND, typename T, int CELLS>
__device__ __forceinline__ void increment_patch(const double* __restrict__ gxyz, const double* __restrict__ gsig, int64_t n,
                                                const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                const double* __restrict__ z, int64_t m, double g2, const T* __restrict__ xb,
                                                T* __restrict__ xa, T* __restrict__ inc, const double* __restrict__ glat,
                                                const double* __restrict__ olat, double win_deg, int nx, double cut_chord, double far_chord,
                                                int64_t blk, const SolveLds& W) {
    constexpr bool FAR = KIND == OISAT_CORR_GAUSSIAN;
    constexpr int PW = 32, PH = CELLS * 8;
    const int t = threadIdx.x;
    int64_t cell[CELLS];
    bool live[CELLS];
    if (nx > 0) {                                               // patch `blk` of the ny x nx grid
        const int64_t ny = n / nx;
        const int64_t ppr = (nx + PW - 1) / PW;                 // patches per row of patches
        if (blk >= ppr * ((ny + PH - 1) / PH)) return;          // block-uniform
        const int64_t py0 = (blk / ppr) * PH, px0 = (blk % ppr) * PW;
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            const int64_t yy = py0 + q * 8 + (t >> 5), xx = px0 + (t & 31);
            live[q] = yy < ny && xx < nx;
            cell[q] = yy * nx + xx;
        }
    } else {
        if (blk * CELLS * 256 >= n) return;
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            cell[q] = (blk * CELLS + q) * 256 + t;
            live[q] = cell[q] < n;
        }
    }
    double px[CELLS], py[CELLS], pz[CELLS];
    double acc[CELLS];
#pragma unroll
    for (int q = 0; q < CELLS; ++q) {
        px[q] = live[q] ? gxyz[cell[q]] : 0.0;
        py[q] = live[q] ? gxyz[n + cell[q]] : 0.0;
        pz[q] = live[q] ? gxyz[2 * n + cell[q]] : 0.0;
        acc[q] = 0.0;
    }
    int64_t j0 = 0, j1 = m;
    const bool windowed = glat && olat;
    if (windowed) {                                             // latitude span of this block's cells -> observation index range
        double lo = 1e9, hi = -1e9;
#pragma unroll
        for (int q = 0; q < CELLS; ++q)
            if (live[q]) { const double la = glat[cell[q]]; lo = fmin(lo, la); hi = fmax(hi, la); }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
        if ((t & 63) == 0) { W.s_lo[t >> 6] = lo; W.s_hi[t >> 6] = hi; }
        __syncthreads();
        if (t == 0) {
            lo = fmin(fmin(W.s_lo[0], W.s_lo[1]), fmin(W.s_lo[2], W.s_lo[3]));
            hi = fmax(fmax(W.s_hi[0], W.s_hi[1]), fmax(W.s_hi[2], W.s_hi[3]));
            W.s_j[0] = lower_bound_lat(olat, m, lo - win_deg);
            W.s_j[1] = lower_bound_lat(olat, m, hi + win_deg + 1e-9);
        }
        __syncthreads();
        j0 = W.s_j[0];
        j1 = W.s_j[1];
    }
    BlockSphere bs = block_sphere<CELLS>(px, py, pz, live, windowed ? cut_chord : 1e30, FAR ? far_chord : (double)INFINITY, W.red);
    if (FAR) {                                                  // (the same values: registers for the far loop, at the old occupancy)
        bs.cx = uniform_f64(bs.cx); bs.cy = uniform_f64(bs.cy); bs.cz = uniform_f64(bs.cz);
        bs.r2cull = uniform_f64(bs.r2cull);
    }
    int fill = 0, ffill = 0;
    for (int64_t c0 = j0; c0 < j1 || fill > 0 || ffill > 0; c0 += 256) {
        if (c0 < j1) fill = stage_near<FAR>(oxyz, osig, z, m, c0, j1, bs, W.bxy, W.bzw, fill, ffill, W.wcnt);
        if (stage_full<FAR>(fill, ffill) || c0 + 256 >= j1) {  // block-uniform
#pragma unroll 4
            for (int j = 0; j < fill; ++j) {
                const double2 oxy = W.bxy[j];
                const double2 ozw = W.bzw[j];
#pragma unroll
                for (int q = 0; q < CELLS; ++q) {
                    const double dx = px[q] - oxy.x, dy = py[q] - oxy.y, dz = pz[q] - ozw.x;
                    // C = 2^x, x = -g2 |p - q|^2, in DOUBLE (exp2_neg, 3.7e-14).  Rounds 1-2 used v_exp_f32: good to 1 ulp = 1.2e-7 of
                    // the term, but the terms cancel (sum|term| is several hundred times the field at swath densities, more at
                    // larger L) and that alone put the fields 2.5e-6 of their scale off at 720x1440 / 1e5 obs, L = 300 km, and
                    // 1.3e-5 -- outside the 1e-5 bar -- at 360x720 / 1e4 gridded obs, L = 500 km; with this: 4e-8.  Twice the
                    // instructions per pair (taking only the pairs with C > 2^-8 in double diverges inside the waves and is
                    // slower still at L = 500 km); the bounding-sphere cull above pays for it.
                    acc[q] += corr_f64_exp2<KIND>(g2, dx * dx + dy * dy + dz * dz) * ozw.y;
                }
            }
            // The far list (stage_near<true>; Gaussian only): every correlation between such an observation and a cell of this
            // patch is below 2^-kSolveFarBits, so the term's fp32 error (coordinates, argument, v_exp_f32: ~1e-5 of it) is that
            // much below the near terms' own.  Packed fp32, an fp32 partial sum per cell and flush, in list order; two cells =
            // the two lanes, one cell = two consecutive entries per step (lane 0 the even ones), joined lane 0 first.
            if (FAR && ffill > 0) {                             // block-uniform
                const float fg2 = (float)far_local(g2);
                if (CELLS == 2) {
                    const f32x2 fx = {(float)far_local(px[0]), (float)far_local(px[CELLS - 1])},
                                fy = {(float)far_local(py[0]), (float)far_local(py[CELLS - 1])},
                                fz = {(float)far_local(pz[0]), (float)far_local(pz[CELLS - 1])};
                    f32x2 fs = {0.0f, 0.0f};
#pragma unroll 4
                    for (int k = far_local_uniform(0); k < ffill; ++k) {
                        const float4 o = far_entry(W.bxy, W.bzw, k);
                        const f32x2 w = {o.w, o.w};
                        fs = far_pairs(fx - o.x, fy - o.y, fz - o.z, fg2, w, fs);
                    }
                    acc[0] += (double)fs.x;
                    acc[CELLS - 1] += (double)fs.y;
                } else {
                    const float fx = (float)far_local(px[0]), fy = (float)far_local(py[0]), fz = (float)far_local(pz[0]);
                    f32x2 fs = {0.0f, 0.0f};
                    int k = far_local_uniform(0);
#pragma unroll 2
                    for (; k + 1 < ffill; k += 2) fs = far_pairs_of(fx, fy, fz, far_entry(W.bxy, W.bzw, k), far_entry(W.bxy, W.bzw, k + 1), fg2, fs);
                    if (k < ffill) {                            // an odd entry: its twin with weight 0
                        const float4 o = far_entry(W.bxy, W.bzw, k);
                        fs = far_pairs_of(fx, fy, fz, o, make_float4(o.x, o.y, o.z, 0.0f), fg2, fs);
                    }
                    acc[0] += (double)fs.x;
                    acc[0] += (double)fs.y;
                }
            }
            fill = 0;
            ffill = 0;
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < CELLS; ++q) {
        if (live[q]) {
            const double v = gsig[cell[q]] * acc[q];
            if (inc) inc[cell[q]] = (T)v;
            if (xa) xa[cell[q]] = (T)((double)xb[cell[q]] + v);
        }
    }
}
