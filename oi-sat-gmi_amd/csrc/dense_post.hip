// The posterior diagnostics of the dense solver: rows of X <- X L^-T (as GEMMs: launch_gemm, dense_gemm.hip) and X <- X L^-1 (the
// backward row sweep), the posterior error and diag(K H) from their row norms, and the Rademacher probes.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"
#include "dense_solve_dev.inc"                                  // (the correlation functions)

// ---- posterior diagnostics: rows of X <- X L^-T, then row norms -----------------------------------
// rows [i0, i0+nrows) of (H B)^T: X[r][a] = sig_{i0+r} * osig_a * C(i0+r, a), zero in the padding columns
template <int KIND>
__global__ __launch_bounds__(256) void cross_cov_rows_kernel(const double* __restrict__ gxyz, const double* __restrict__ gsig,
                                                              int64_t n, int64_t i0, int64_t nrows, const double* __restrict__ oxyz,
                                                              const double* __restrict__ osig, int64_t m, int64_t mp, float g2,
                                                              float* __restrict__ X, int64_t ldx) {
    // block = 64 rows x 64 columns tile (like cov_build): blockIdx.x = column tile, blockIdx.y = row tile
    __shared__ float4 pr[64], pc[64];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    if (t < 64) {
        const int64_t cell = i0 + r0 + t;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + t < nrows && cell < n) v = make_float4((float)gxyz[cell], (float)gxyz[n + cell], (float)gxyz[2 * n + cell], (float)gsig[cell]);
        pr[t] = v;
    } else if (t < 128) {
        const int64_t a = c0 + (t - 64);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a < m) v = make_float4((float)oxyz[a], (float)oxyz[m + a], (float)oxyz[2 * m + a], (float)osig[a]);
        pc[t - 64] = v;
    }
    __syncthreads();
    const int cx = (t & 15) * 4, ry = t >> 4;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = ry + rr * 16;
        if (r0 + r >= nrows) continue;
        const float4 a = pr[r];
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 q = pc[cx + c];
            const float dx = a.x - q.x, dy = a.y - q.y, dz = a.z - q.z;
            o[c] = (c0 + cx + c < m) ? a.w * q.w * corr_f32<KIND>(g2, dx * dx + dy * dy + dz * dz) : 0.f;
        }
        *reinterpret_cast<float4*>(&X[(r0 + r) * ldx + c0 + cx]) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// X = rows [a0, a0+nrows) of the identity (padded to mp columns)
__global__ __launch_bounds__(256) void identity_rows_kernel(float* __restrict__ X, int64_t ldx, int64_t a0, int64_t nrows, int64_t mp) {
    const int64_t total = nrows * mp;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int64_t r = p / mp, c = p % mp;
        X[r * ldx + c] = (c == a0 + r) ? 1.f : 0.f;
    }
}

// out[r] = sum_c X[r][c]^2 in double; one wave per row, fixed shuffle tree
__global__ __launch_bounds__(256) void row_sumsq_kernel(const float* __restrict__ X, int64_t nrows, int64_t ncols, int64_t ldx,
                                                         double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (row >= nrows) return;
    const float* x = X + row * ldx;
    double s = 0.0;
    for (int64_t c = lane * 4; c < ncols; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + c);
        s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, kWave);
    if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(256) void post_err_kernel(const double* __restrict__ gsig, int64_t i0, int64_t nrows, int64_t n,
                                                        const double* __restrict__ ss, float* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows || i0 + r >= n) return;
    const double v = gsig[i0 + r] * gsig[i0 + r] - ss[r];
    err[r] = (float)sqrt(v > 0.0 ? v : 0.0);
}

__global__ __launch_bounds__(256) void gain_diag_kernel(const double* __restrict__ ovar, int64_t a0, int64_t nrows, int64_t m,
                                                         const double* __restrict__ ss, double* __restrict__ ak) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows || a0 + r >= m) return;
    ak[a0 + r] = 1.0 - ovar[a0 + r] * ss[r];         // diag(K H) at the observation: 1 - R_aa (S^-1)_aa
}

// X[nrows x mp] <- X L^-T  by block forward substitution over column blocks [b0, b1)
int trsm_rows_rec(oisat_ctx* h, const ChFactor& f, float* X, int64_t nrows, int64_t ldx, int64_t b0, int64_t b1) {
    if (b1 - b0 == 1) {
        float* Xb = X + b0 * NB;
        return launch_gemm(h, "trsm_rows_diag", Xb, ldx, Xb, ldx, f.tinv + b0 * NB * NB, NB, nrows, NB, NB, 1, 0);
    }
    const int64_t mid = b0 + (b1 - b0 + 1) / 2;
    int rc = trsm_rows_rec(h, f, X, nrows, ldx, b0, mid);
    if (rc) return rc;
    // X[:, mid:b1] -= X[:, b0:mid] * L[mid:b1, b0:mid]^T
    rc = launch_gemm(h, "trsm_rows_gemm", X + mid * NB, ldx, X + b0 * NB, ldx, f.S + mid * NB * f.ld + b0 * NB, f.ld, nrows,
                     (b1 - mid) * NB, (int)((mid - b0) * NB), 0, 0);
    if (rc) return rc;
    return trsm_rows_rec(h, f, X, nrows, ldx, mid, b1);
}

// ---- X <- X L^-1: the backward row sweep (oisat_trsm_rows_bwd) ---------------------------------------------------------
// Y L = X, block column by block column from the right: Y_j = (X_j - sum_{i > j} Y_i L_ij) T_j, T_j = L_jj^-1 (tinv).  One
// launch per block column j = nb-1 .. 1: blockIdx.x = k - k0 for the block columns k0 <= k < j of block row j inside the
// envelope (k0 = first[j], or 0 for a dense factor), blockIdx.y = panel of 128 rows of X.  Workgroup k applies
// X_k -= X_j L_jk, an NN product: L_jk is read row-major as it lies.  X_j is final when launch j starts (stream order, nothing
// else): the workgroup of k = j-1 has applied the last update X_{j-1} will ever get (first[j] <= j-1) and multiplies by
// T_{j-1} before it stores.  Exactly one workgroup writes a tile of X in a launch and none reads a tile another one writes.
// 4 waves as 2x2, each 64x64 = 2x2 MFMA tiles; K in slices of 32 through one LDS image per operand (A [128][36], B [32][132]),
// the next slice prefetched into registers; a lane feeds k = 8s+4h..+3 to four consecutive MFMAs, A and B alike.
constexpr int BWD_LDB = 132;      // LDS row stride of the B slice (4 rows apart = 16 banks apart: the two half-waves do not collide)

struct BwdTile { f32x16 a[2][2]; };

// acc += A[128 x 32 slice in As] * B[32 x 128 slice in Bs] for this wave's 64x64 quadrant
__device__ __forceinline__ void bwd_slice_mfma(const float* __restrict__ As, const float* __restrict__ Bs, int wr, int wc, int frow, int fh,
                                               BwdTile& acc) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        float4 fa[2];
        float fb[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4*>(&As[(wr * 64 + i * 32 + frow) * LDSW + 8 * s4 + 4 * fh]);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int c = 0; c < 4; ++c) fb[jj][c] = Bs[(8 * s4 + 4 * fh + c) * BWD_LDB + wc * 64 + jj * 32 + frow];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                acc.a[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[jj][0], acc.a[i][jj], 0, 0, 0);
                acc.a[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[jj][1], acc.a[i][jj], 0, 0, 0);
                acc.a[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[jj][2], acc.a[i][jj], 0, 0, 0);
                acc.a[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[jj][3], acc.a[i][jj], 0, 0, 0);
            }
    }
}

// a slice of an operand on its way to LDS: 4 x 16 bytes per thread
struct BwdRegs { float4 q0, q1, q2, q3; };
// the B slice of rows [kk, kk + 32) of a row-major 128-wide block: rows brow + 8 q
__device__ __forceinline__ BwdRegs bwd_load_b(const float* __restrict__ B, int64_t ldb, int kk, int t) {
    const float* p = B + (int64_t)(kk + (t >> 5)) * ldb + (t & 31) * 4;
    BwdRegs r;
    r.q0 = *reinterpret_cast<const float4*>(p);
    r.q1 = *reinterpret_cast<const float4*>(p + 8 * ldb);
    r.q2 = *reinterpret_cast<const float4*>(p + 16 * ldb);
    r.q3 = *reinterpret_cast<const float4*>(p + 24 * ldb);
    return r;
}
__device__ __forceinline__ void bwd_store_b(float* __restrict__ Bs, int t, const BwdRegs& r) {
    float* p = Bs + (t >> 5) * BWD_LDB + (t & 31) * 4;
    *reinterpret_cast<float4*>(p) = r.q0;
    *reinterpret_cast<float4*>(p + 8 * BWD_LDB) = r.q1;
    *reinterpret_cast<float4*>(p + 16 * BWD_LDB) = r.q2;
    *reinterpret_cast<float4*>(p + 24 * BWD_LDB) = r.q3;
}
// the A slice of columns [kk, kk + 32) of 128 rows: rows srow + 32 q
__device__ __forceinline__ BwdRegs bwd_load_a(const float* __restrict__ A, int64_t lda, int kk, int t) {
    const float* p = A + (int64_t)(t >> 3) * lda + kk + (t & 7) * 4;
    BwdRegs r;
    r.q0 = *reinterpret_cast<const float4*>(p);
    r.q1 = *reinterpret_cast<const float4*>(p + 32 * lda);
    r.q2 = *reinterpret_cast<const float4*>(p + 64 * lda);
    r.q3 = *reinterpret_cast<const float4*>(p + 96 * lda);
    return r;
}
__device__ __forceinline__ void bwd_store_a(float* __restrict__ As, int t, const BwdRegs& r) {
    float* p = As + (t >> 3) * LDSW + (t & 7) * 4;
    *reinterpret_cast<float4*>(p) = r.q0;
    *reinterpret_cast<float4*>(p + 32 * LDSW) = r.q1;
    *reinterpret_cast<float4*>(p + 64 * LDSW) = r.q2;
    *reinterpret_cast<float4*>(p + 96 * LDSW) = r.q3;
}

// out = V * T for a 128 x 128 tile V held in MFMA C layout (col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) per 32 x 32
// tile), T row-major [128][128]: slice s of V's columns is tile column s & 1 of the waves with wc == s >> 1, which park it in As
__device__ __forceinline__ void bwd_times_tinv(const BwdTile& v, const float* __restrict__ T, float* __restrict__ As, float* __restrict__ Bs,
                                               int t, int wr, int wc, int frow, int fh, BwdTile& out) {
    BwdRegs rb = bwd_load_b(T, NB, 0, t);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (wc == (s >> 1)) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    As[(wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh) * LDSW + frow] = v.a[i][s & 1][e];
        }
        bwd_store_b(Bs, t, rb);
        __syncthreads();
        if (s < 3) rb = bwd_load_b(T, NB, (s + 1) * BK, t);
        bwd_slice_mfma(As, Bs, wr, wc, frow, fh, out);
        __syncthreads();
    }
}

// FIRST: the one launch in front of the sweep, X_j <- X_j T_j for the last block column (grid.x = 1)
template <bool FIRST>
__global__ __launch_bounds__(256) void trsm_rows_bwd_kernel(const float* __restrict__ L, int64_t ld, const float* __restrict__ tinv,
                                                             float* __restrict__ X, int64_t ldx, int j, int k0) {
    __shared__ __attribute__((aligned(16))) float As[NB * LDSW];          // 18,432 B
    __shared__ __attribute__((aligned(16))) float Bs[BK * BWD_LDB];       // 16,896 B
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wr = wid >> 1, wc = wid & 1, frow = lane & 31, fh = lane >> 5;
    const int k = FIRST ? j : k0 + (int)blockIdx.x;                        // the block column this workgroup writes
    float* Xr = X + (int64_t)blockIdx.y * NB * ldx;                        // this panel of rows
    float* Ck = Xr + (int64_t)k * NB + (int64_t)(wr * 64) * ldx + wc * 64; // this wave's quadrant of X_k
    BwdTile acc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc.a[i][jj][e] = 0.f;
    if (!FIRST) {
        const float* Aj = Xr + (int64_t)j * NB;                            // X_j, rows of this panel
        const float* Bjk = L + (int64_t)j * NB * ld + (int64_t)k * NB;     // L_jk
        BwdRegs ra = bwd_load_a(Aj, ldx, 0, t), rb = bwd_load_b(Bjk, ld, 0, t);
        for (int kt = 0; kt < NB / BK; ++kt) {
            bwd_store_a(As, t, ra);
            bwd_store_b(Bs, t, rb);
            __syncthreads();
            if (kt + 1 < NB / BK) {
                ra = bwd_load_a(Aj, ldx, (kt + 1) * BK, t);
                rb = bwd_load_b(Bjk, ld, (kt + 1) * BK, t);
            }
            bwd_slice_mfma(As, Bs, wr, wc, frow, fh, acc);
            __syncthreads();
        }
    }
    // acc <- X_k - acc (FIRST: X_j itself), in C layout
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                acc.a[i][jj][e] = Ck[(int64_t)row * ldx + jj * 32 + frow] - acc.a[i][jj][e];
            }
    if (FIRST || k == j - 1) {                                             // (block-uniform) the column is complete: times T_k
        BwdTile fin;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int e = 0; e < 16; ++e) fin.a[i][jj][e] = 0.f;
        bwd_times_tinv(acc, tinv + (int64_t)k * NB * NB, As, Bs, t, wr, wc, frow, fh, fin);
        acc = fin;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                Ck[(int64_t)row * ldx + jj * 32 + frow] = acc.a[i][jj][e];
            }
}

int trsm_rows_bwd(oisat_ctx* h, const ChFactor& f, float* X, int64_t nrows, int64_t ldx) {
    const int nb = (int)(f.mp / NB);
    const unsigned panels = (unsigned)(nrows / NB);
    const bool env = f.env != nullptr && (int64_t)f.first.size() == nb;
    OISAT_LAUNCH(h, "trsm_rows_bwd_diag", trsm_rows_bwd_kernel<true>, dim3(1, panels), dim3(256), 0, f.S, f.ld, (const float*)f.tinv, X, ldx,
                 nb - 1, 0);
    for (int j = nb - 1; j >= 1; --j) {
        int k0 = env ? f.first[j] : 0;
        if (k0 < 0 || k0 > j - 1) k0 = 0;                               // (never: the table was checked when it was recorded)
        OISAT_LAUNCH(h, "trsm_rows_bwd", trsm_rows_bwd_kernel<false>, dim3((unsigned)(j - k0), panels), dim3(256), 0, f.S, f.ld,
                     (const float*)f.tinv, X, ldx, j, k0);
    }
    return OISAT_OK;
}

// ---- Rademacher probes (oisat_probe_sign / _fill / _diag) ---------------------------------------------------------------
// A counter-based sign: splitmix64's finaliser over (seed, probe, column), the same function on host and device.
__host__ __device__ inline uint64_t probe_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ inline float probe_sign(uint64_t seed_mixed, uint64_t probe, uint64_t column) {
    return (probe_mix(probe_mix(seed_mixed ^ probe) ^ column) >> 63) ? -1.0f : 1.0f;
}

__global__ __launch_bounds__(256) void probe_fill_kernel(uint64_t seed_mixed, int64_t first_probe, float* __restrict__ X, int64_t nrows,
                                                          int64_t ldx, int64_t m) {
    const int64_t total = nrows * ldx;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int64_t r = p / ldx, c = p - r * ldx;
        X[p] = c < m ? probe_sign(seed_mixed, (uint64_t)(first_probe + r), (uint64_t)c) : 0.0f;
    }
}

// per column a < m: the sums of U[k][a]^2 and U[k][a]^4 over the probes, in double, in the order of k
__global__ __launch_bounds__(256) void probe_diag_kernel(const float* __restrict__ U, int64_t nprobe, int64_t ldu, int64_t m, int accumulate,
                                                          double* __restrict__ sum2, double* __restrict__ sum4) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m) return;
    double s2 = 0.0, s4 = 0.0;
    for (int64_t k = 0; k < nprobe; ++k) {
        const double u = (double)U[k * ldu + a], q = u * u;
        s2 += q;
        s4 += q * q;
    }
    sum2[a] = accumulate ? sum2[a] + s2 : s2;
    sum4[a] = accumulate ? sum4[a] + s4 : s4;
}

}  // namespace

extern "C" int oisat_trsm_rows(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* X, int64_t nrows, int64_t ldx) {
    ARG_CHECK(h && L && X && m > 0 && nrows > 0);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);     // must follow oisat_potrf of this matrix
    ARG_CHECK(nrows % NB == 0 && ldx >= h->factor.mp && ldx % 4 == 0 && ((uintptr_t)X % 16) == 0);
    return trsm_rows_rec(h, h->factor, X, nrows, ldx, 0, h->factor.mp / NB);
}

extern "C" int oisat_trsm_rows_bwd(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* X, int64_t nrows, int64_t ldx) {
    ARG_CHECK(h && L && X && m > 0 && nrows > 0);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);     // must follow a factorization of this matrix
    ARG_CHECK(nrows % NB == 0 && nrows / NB <= 65535 && ldx >= h->factor.mp && ldx % 4 == 0 && ((uintptr_t)X % 16) == 0);
    return trsm_rows_bwd(h, h->factor, X, nrows, ldx);
}

extern "C" int oisat_probe_sign(uint64_t seed, int64_t probe, int64_t column, float* sign_out) {
    ARG_CHECK(sign_out != nullptr && probe >= 0 && column >= 0);
    *sign_out = probe_sign(probe_mix(seed), (uint64_t)probe, (uint64_t)column);
    return OISAT_OK;
}

extern "C" int oisat_probe_fill(oisat_ctx* h, uint64_t seed, int64_t first_probe, float* X, int64_t nrows, int64_t ldx, int64_t m) {
    ARG_CHECK(h && X && m > 0 && nrows > 0 && first_probe >= 0);
    ARG_CHECK(ldx >= cdiv(m, NB) * NB);
    OISAT_LAUNCH(h, "probe_fill", probe_fill_kernel, dim3(stream_grid(nrows * ldx, 256)), dim3(256), 0, probe_mix(seed), first_probe, X, nrows,
                 ldx, m);
    return OISAT_OK;
}

extern "C" int oisat_probe_diag(oisat_ctx* h, const float* U, int64_t nprobe, int64_t ldu, int64_t m, int accumulate, double* sum2_out,
                                double* sum4_out) {
    ARG_CHECK(h && U && sum2_out && sum4_out && m > 0 && nprobe > 0 && ldu >= m);
    ARG_CHECK(cdiv(m, 256) < (int64_t)INT32_MAX);
    OISAT_LAUNCH(h, "probe_diag", probe_diag_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, U, nprobe, ldu, m, accumulate, sum2_out,
                 sum4_out);
    return OISAT_OK;
}

extern "C" int oisat_posterior_error(oisat_ctx* h, const float* L, int64_t m, int64_t ld, const double* gxyz, const double* gsig,
                                     int64_t n, int64_t i0, int64_t i1, const double* oxyz, const double* osig, double g,
                                     int64_t chunk_rows, float* err) {
    ARG_CHECK(h && L && gxyz && gsig && oxyz && osig && err && m > 0 && n > 0 && 0 <= i0 && i0 < i1 && i1 <= n);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);
    const int64_t mp = h->factor.mp;
    if (chunk_rows <= 0) chunk_rows = 4096;
    chunk_rows = cdiv(chunk_rows, NB) * NB;
    float* X = (float*)oisat_ws(h, 6, sizeof(float) * chunk_rows * mp + sizeof(double) * chunk_rows);
    if (!X) return OISAT_ENOMEM;
    double* ss = (double*)(X + chunk_rows * mp);
    const float g2 = h->corr == OISAT_CORR_SOAR           ? (float)corr_scale2(OISAT_CORR_SOAR, g)
                     : h->corr == OISAT_CORR_GASPARI_COHN ? (float)(kGcZ2PerG * g)
                                                          : (float)(g * 1.4426950408889634);      // g2 | kz2 | 2 g (log2 e)^2
    for (int64_t c0 = i0; c0 < i1; c0 += chunk_rows) {
        const int64_t live = (i1 - c0 < chunk_rows) ? i1 - c0 : chunk_rows;
        const int64_t nrows = cdiv(live, NB) * NB;                 // rows live..nrows are zero rows
        if (h->corr == OISAT_CORR_GASPARI_COHN) {
            OISAT_LAUNCH(h, "cross_cov_rows", cross_cov_rows_kernel<OISAT_CORR_GASPARI_COHN>, dim3((unsigned)(mp / 64), (unsigned)(nrows / 64)),
                         dim3(256), 0, gxyz, gsig, n, c0, live, oxyz, osig, m, mp, g2, X, mp);
        } else if (h->corr == OISAT_CORR_SOAR) {
            OISAT_LAUNCH(h, "cross_cov_rows", cross_cov_rows_kernel<OISAT_CORR_SOAR>, dim3((unsigned)(mp / 64), (unsigned)(nrows / 64)),
                         dim3(256), 0, gxyz, gsig, n, c0, live, oxyz, osig, m, mp, g2, X, mp);
        } else {
            OISAT_LAUNCH(h, "cross_cov_rows", cross_cov_rows_kernel<OISAT_CORR_GAUSSIAN>, dim3((unsigned)(mp / 64), (unsigned)(nrows / 64)),
                         dim3(256), 0, gxyz, gsig, n, c0, live, oxyz, osig, m, mp, g2, X, mp);
        }
        if (nrows > live) HIP_TRY(hipMemsetAsync(X + live * mp, 0, sizeof(float) * (nrows - live) * mp, h->stream));
        const int rc = trsm_rows_rec(h, h->factor, X, nrows, mp, 0, mp / NB);
        if (rc) return rc;
        OISAT_LAUNCH(h, "row_sumsq", row_sumsq_kernel, dim3((unsigned)cdiv(nrows * 64, 256)), dim3(256), 0, (const float*)X, nrows, mp,
                     mp, ss);
        OISAT_LAUNCH(h, "post_err", post_err_kernel, dim3((unsigned)cdiv(live, 256)), dim3(256), 0, gsig, c0, live, n,
                     (const double*)ss, err + (c0 - i0));
    }
    return OISAT_OK;
}

extern "C" int oisat_gain_diag(oisat_ctx* h, const float* L, int64_t m, int64_t ld, const double* ovar, int64_t chunk_rows,
                               double* ak_out) {
    ARG_CHECK(h && L && ovar && ak_out && m > 0);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);
    const int64_t mp = h->factor.mp;
    if (chunk_rows <= 0) chunk_rows = 4096;
    chunk_rows = cdiv(chunk_rows, NB) * NB;
    float* X = (float*)oisat_ws(h, 6, sizeof(float) * chunk_rows * mp + sizeof(double) * chunk_rows);
    if (!X) return OISAT_ENOMEM;
    double* ss = (double*)(X + chunk_rows * mp);
    for (int64_t a0 = 0; a0 < m; a0 += chunk_rows) {
        const int64_t live = (m - a0 < chunk_rows) ? m - a0 : chunk_rows;
        const int64_t nrows = cdiv(live, NB) * NB;
        OISAT_LAUNCH(h, "identity_rows", identity_rows_kernel, dim3(stream_grid(nrows * mp, 256)), dim3(256), 0, X, mp, a0, nrows, mp);
        const int rc = trsm_rows_rec(h, h->factor, X, nrows, mp, 0, mp / NB);
        if (rc) return rc;
        OISAT_LAUNCH(h, "row_sumsq", row_sumsq_kernel, dim3((unsigned)cdiv(nrows * 64, 256)), dim3(256), 0, (const float*)X, nrows, mp,
                     mp, ss);
        OISAT_LAUNCH(h, "gain_diag", gain_diag_kernel, dim3((unsigned)cdiv(live, 256)), dim3(256), 0, ovar, a0, live, m,
                     (const double*)ss, ak_out);
    }
    return OISAT_OK;
}
