// The solve unit of the dense solver: the triangular sweeps (trsv_pipe_kernel, and trsv_batched_kernel over many systems; their
// rows are dense_trsv.inc), the gain solve with its float64 refinement (oisat_gain_solve; the residual itself is dense_cov.hip's) and
// the same solve with the fields written underneath and behind it (oisat_gain_solve_fields; the increment kernels are dense_cov.hip's),
// oisat_potrs, the handle's status words, and the oisat_batch_* API, whose solve phase launches the same sweep kernels.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"
#include "dense_trsv.inc"
#include "dense_solve_dev.inc"                                  // (host: the rules oisat_batch_analyse hands its launch)

template <int TRANSPOSE>
__global__ __launch_bounds__(256) void trsv_pipe_kernel(const float* __restrict__ L, int64_t ld, const float* __restrict__ tinv, int nb,
                                                         double* __restrict__ rhs, double* __restrict__ sol,
                                                         TrsvCtl* __restrict__ ctl, unsigned* __restrict__ err_total, int two_tiles,
                                                         const SolveState* __restrict__ st, double* __restrict__ zout, int64_t m,
                                                         int accumulate, const int* __restrict__ env) {
    // env (or nullptr): first[nb] | last[nb] of an enveloped factor -- forward, row b's producers start at first[b]; backward,
    // column b's at last[b] = max{ j : first[j] <= b }.  Clamped into [0, tk]: no table content can move a read out of L.
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [128][TLD]  (+ a second one for T_b if two_tiles)
    __shared__ double vec[NB], part[NB];
    __shared__ unsigned s_ticket, s_ok;
    const int tid = threadIdx.x;
    if (st != nullptr && st->conv != 0) return;          // refinement already converged: this sweep is not needed (block-uniform)
    while (true) {
        __syncthreads();                                 // the previous row's LDS (vec, part, tiles, ticket) is no longer read
        if (tid == 0) {
            s_ticket = atomicAdd(&ctl->ticket, 1u);
            s_ok = 1u;
        }
        __syncthreads();
        const int tk = (int)s_ticket;                    // 0 .. nb-1 in claim order
        if (tk >= nb) break;
        int step0 = 0;
        if (env != nullptr) {
            step0 = TRANSPOSE ? nb - 1 - env[nb + (nb - 1 - tk)] : env[tk];
            step0 = step0 < 0 ? 0 : (step0 > tk ? tk : step0);
        }
        if (!trsv_row<TRANSPOSE, false>(L, ld, tinv, nb, tk, step0, rhs, sol, ctl, err_total, two_tiles, zout, m, accumulate, tile, vec, part, &s_ok))
            break;
    }
    if (tid == 0) trsv_leave(ctl);
}

// The sweeps of MANY systems in one launch (oisat_batch_solve): tickets run over the list `ord` of (member, step) pairs,
// steps ascending -- step k of every system before step k+1 of any -- so a row still waits for lower tickets only, and the
// launch streams the factors of all systems level by level instead of one latency-bound chain per system and lane.
// A member whose refinement has converged is skipped row by row (nobody waits for its rows).
template <int TRANSPOSE>
__global__ __launch_bounds__(256) void trsv_batched_kernel(const SolveMember* __restrict__ mem, const int* __restrict__ ord, int total,
                                                            TrsvCtl* __restrict__ ctl, unsigned* __restrict__ err_total,
                                                            int first_solve, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [128][TLD]
    __shared__ double vec[NB], part[NB];
    __shared__ unsigned s_ticket, s_ok;
    const int tid = threadIdx.x;
    while (true) {
        __syncthreads();
        if (tid == 0) {
            s_ticket = atomicAdd(&ctl->ticket, 1u);
            s_ok = 1u;
        }
        __syncthreads();
        const unsigned t = s_ticket;
        if (t >= (unsigned)total) break;
        const int e = ord[t];
        const SolveMember* mb = mem + (e >> 12);
        const int tk = e & 4095;
        if (!first_solve && mb->st->conv != 0) continue;             // this system needs no further correction
        double* in = TRANSPOSE ? mb->fwd : mb->rhs;
        double* out = TRANSPOSE ? mb->rhs : mb->fwd;
        if (!trsv_row<TRANSPOSE, false>(mb->S, mb->ld, mb->tinv, mb->mpb, tk, 0, in, out, ctl, err_total, 0, TRANSPOSE ? mb->z : (double*)nullptr,
                                 mb->m, accumulate, tile, vec, part, &s_ok))
            break;
    }
    if (tid == 0) trsv_leave(ctl);
}

// rhs <- src padded with zeros to mp, fwd <- the "not yet published" pattern; resets the solve's convergence state
__global__ __launch_bounds__(256) void solve_prep_kernel(const double* __restrict__ src, int64_t m, int64_t mp, double* __restrict__ rhs,
                                                          double* __restrict__ fwd, SolveState* __restrict__ st) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = g0; i < mp; i += stride) {
        rhs[i] = i < m ? src[i] : 0.0;
        reinterpret_cast<unsigned long long*>(fwd)[i] = kTrsvEmpty;
    }
    if (st != nullptr && g0 == 0) {
        st->conv = 0;
        st->computed = 0;
    }
}

// |r_k|^2 (and |d|^2 at k = 0) in one block, fixed order; sets the convergence flag when |r_k| <= tol |d|
// final: this is the check behind the LAST allowed correction -- a solve that is still above its tolerance here is counted in
// the handle's status words (info[4], info[5]); tol2 = 0 ("run every round") never counts
// keep (or nullptr): takes a copy of r -- the forward sweep that follows consumes r, and the update form of the next round's
// residual (cov_residual_update) starts from the last fully evaluated one
__global__ __launch_bounds__(1024) void resid_check_kernel(const double* __restrict__ r, const double* __restrict__ d, int64_t m, int k,
                                                            double tol2, SolveState* __restrict__ st, int final, int* __restrict__ info,
                                                            double* __restrict__ keep) {
    __shared__ double sr[1024], sd[1024];
    if (st->conv != 0) return;
    // one workgroup on the critical path: its waves go first where they share a SIMD with another stream's (the side stream's
    // increment of oisat_gain_solve_fields held this kernel for 0.72 ms instead of 0.06)
    __builtin_amdgcn_s_setprio(3);
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 1024) {
        if (keep != nullptr) keep[i] = r[i];
        a += r[i] * r[i];
        if (k == 0) b += d[i] * d[i];
    }
    sr[threadIdx.x] = a;
    sd[threadIdx.x] = b;
    __syncthreads();
    for (int q = 512; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) {
            sr[threadIdx.x] += sr[threadIdx.x + q];
            sd[threadIdx.x] += sd[threadIdx.x + q];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (k == 0) st->dd = sd[0];
        st->norm[k] = sr[0];
        st->computed = k + 1;
        if (sr[0] <= tol2 * st->dd) st->conv = 1;
        else if (final && tol2 > 0.0) atomicAdd(&info[kInfoUnconverged], 1);
    }
}

// The check behind the UPDATE form of round k's residual (t = r_{k-1} - S dz, S dz in fp32: cov_residual_update): |t|^2 in the
// order of resid_check_kernel.  t is within c |r_{k-1}| of the float64 residual, so |t| + c |r_{k-1}| <= tol |d| proves that
// the float64 test would pass: then, and only then, this round's norm is |t|^2 and the solve is converged -- the full residual,
// its check and the later sweeps return at once.  Otherwise nothing is written and the float64 residual decides as before.
__global__ __launch_bounds__(1024) void resid_update_check_kernel(const double* __restrict__ t, int64_t m, int k, double tol, double c,
                                                                   SolveState* __restrict__ st) {
    __shared__ double sr[1024];
    if (st->conv != 0) return;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 1024) a += t[i] * t[i];
    sr[threadIdx.x] = a;
    __syncthreads();
    for (int q = 512; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) sr[threadIdx.x] += sr[threadIdx.x + q];
        __syncthreads();
    }
    if (threadIdx.x == 0 && tol > 0.0 && k >= 1 && sqrt(sr[0]) + c * sqrt(st->norm[k - 1]) <= tol * sqrt(st->dd)) {
        st->norm[k] = sr[0];
        st->computed = k + 1;
        st->conv = 1;
    }
}


__global__ __launch_bounds__(256) void solve_prep_batched_kernel(const SolveMember* __restrict__ mem) {
    const SolveMember* mb = mem + blockIdx.y;
    const int64_t m = mb->m, mp = (int64_t)mb->mpb * NB;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double* src = mb->d;
    double* rhs = mb->rhs;
    unsigned long long* fwd = reinterpret_cast<unsigned long long*>(mb->fwd);
    for (int64_t i = g0; i < mp; i += stride) {
        rhs[i] = i < m ? src[i] : 0.0;
        fwd[i] = kTrsvEmpty;
    }
    if (g0 == 0) {
        mb->st->conv = 0;
        mb->st->computed = 0;
    }
}

__global__ __launch_bounds__(1024) void resid_check_batched_kernel(const SolveMember* __restrict__ mem, int k, double tol2, int final,
                                                                    int* __restrict__ info) {
    __shared__ double sr[1024], sd[1024];
    const SolveMember* mb = mem + blockIdx.x;
    SolveState* st = mb->st;
    if (st->conv != 0) return;
    const double* r = mb->rhs;
    const double* d = mb->d;
    const int64_t m = mb->m;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 1024) {
        a += r[i] * r[i];
        if (k == 0) b += d[i] * d[i];
    }
    sr[threadIdx.x] = a;
    sd[threadIdx.x] = b;
    __syncthreads();
    for (int q = 512; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) {
            sr[threadIdx.x] += sr[threadIdx.x + q];
            sd[threadIdx.x] += sd[threadIdx.x + q];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (k == 0) st->dd = sd[0];
        st->norm[k] = sr[0];
        st->computed = k + 1;
        if (sr[0] <= tol2 * st->dd) st->conv = 1;
        else if (final && tol2 > 0.0) {
            atomicAdd(&info[kInfoUnconverged], 1);
            note_unconverged_member(&info[kInfoUnconvergedMember], mb->which);
        }
    }
}

constexpr size_t kCtlBytes = ((sizeof(TrsvCtl) + 15) / 16) * 16;

}  // namespace

namespace oisat_dense {

// Status words of the dense solve, zeroed when first allocated and from then on only by oisat_solve_status(clear):
//   slot 4: int info[8]   = { first non-positive pivot column of the CURRENT factorization (reset by oisat_potrf),
//                             first such column since the last clear, number of failing diagonal blocks since then,
//                             1 + table index of the batch member that met the current one,
//                             [4] gain solves that used every refinement round and still ended above the tolerance,
//                             [5] 1 + member index of the first of them (0: a single-system solve, or none),
//                             [6] task-graph launches that ended on a time-out (their factor is incomplete), - }
//   slot 7: [unsigned err_total (16 B): triangular-solve workgroups that gave up waiting, since the last clear
//            | control block of sweep 0 | control block of sweep 1]
int status_ws(oisat_ctx* h, int** info_dev, char** trsv_base) {
    const bool fresh4 = h->ws[4] == nullptr, fresh7 = h->ws[7] == nullptr;
    int* info = (int*)oisat_ws(h, 4, 256);
    char* base = (char*)oisat_ws(h, 7, 16 + 2 * kCtlBytes);
    if (!info || !base) return OISAT_ENOMEM;
    if (fresh4) HIP_TRY(hipMemsetAsync(info, 0, 256, h->stream));
    if (fresh7) HIP_TRY(hipMemsetAsync(base, 0, 16 + 2 * kCtlBytes, h->stream));
    if (info_dev) *info_dev = info;
    if (trsv_base) *trsv_base = base;
    return OISAT_OK;
}

SolveState* solve_state(oisat_ctx* h) {
    const bool fresh = h->ws[9] == nullptr;
    SolveState* st = (SolveState*)oisat_ws(h, 9, 256);
    if (st && fresh && hipMemsetAsync(st, 0, 256, h->stream) != hipSuccess) return nullptr;
    return st;
}

// per-function attributes, set once per process (handles may be driven from different host threads)
hipError_t dense_kernel_attributes() {
    static const hipError_t attr_rc = []() {
        hipError_t e = hipFuncSetAttribute((const void*)trsv_pipe_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * NB * TLD * 2));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)trsv_pipe_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * NB * TLD * 2));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)trsv_batched_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * NB * TLD));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)trsv_batched_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * NB * TLD));
        return e;
    }();
    return attr_rc;
}

// solve_prep_kernel for a caller in another unit: the factorization launch that carries the first forward sweep (dense_chol.hip)
int solve_prep(oisat_ctx* h, const double* src, int64_t m, int64_t mp, double* rhs, double* fwd, SolveState* st) {
    OISAT_LAUNCH(h, "copy_pad", solve_prep_kernel, dim3(stream_grid(mp, 256)), dim3(256), 0, src, m, mp, rhs, fwd, st);
    return OISAT_OK;
}

}  // namespace oisat_dense

namespace {

// L L^T x = rhs: forward sweep rhs -> fwd, backward sweep fwd -> rhs (the solution, padded).  On entry `fwd` must hold the
// "not yet published" pattern (solve_prep_kernel, or the previous solve's backward sweep, which leaves it behind); each
// sweep re-arms the vector it has consumed for the sweep that follows, and the last workgroup of a sweep zeroes its
// control block, so a solve is exactly two launches.  st: skip both when the refinement has converged.  zout (m entries):
// where the solution is to be written (accumulate = 0) or added (1) besides rhs.  fwd_done: the forward sweep of this right-
// hand side ran inside the factorization launch (oisat_potrf_env_fwd) and left both vectors as trsv_fwd would: backward only.
// The launch shape of the sweeps (host only, include/oisat.h).  A second LDS tile per workgroup (132 KB: one workgroup per CU)
// takes T_b off the critical path of every hand-over; it is given
//  - when every block row gets its own CU at once (nb <= cu_count), or
//  - when the factor is ENVELOPED and its band is at most half the CUs: only the `band` rows behind the front can make
//    progress, so one workgroup per CU serves them with as many again staging ahead, each workgroup claiming row after row
//    by ticket.  The workgroups beyond cu_count would only draw a ticket >= nb and leave: grid = min(nb, cu_count).
// Everything else -- a large dense system, bound by streaming L -- keeps one tile, a workgroup per row and two per CU in flight.
extern "C" int oisat_trsv_plan(int64_t nb, int band, int cu_count, int32_t* two_tiles_out, int32_t* grid_out) {
    ARG_CHECK(nb >= 1 && nb <= INT32_MAX && band >= 0 && cu_count >= 0);
    const bool two = nb <= cu_count || (band > 0 && band <= cu_count / 2);
    if (two_tiles_out) *two_tiles_out = two ? 1 : 0;
    if (grid_out) *grid_out = (int32_t)(two ? std::min<int64_t>(nb, cu_count) : nb);
    return OISAT_OK;
}

// The sweeps' shape while another stream's increment shares the GPU with them (oisat_gain_solve_fields; host only).  A two-tile
// sweep workgroup holds 2 * 128 * TLD floats of LDS (134 160 B with the kernel's static words) of a CU's 160 KiB: beside it exactly
// ONE increment workgroup fits (kSolveLdsBytes = 26 848 B), against five on a CU without one.  The sweeps are bound by their
// hand-overs, not by CUs: a grid of kIncOverlapSweepWgs = 128 was measured as no slower for a band of at most 128 block rows
// (profiles/EXPERIMENTS.md, "T_b ahead of the hand-over": the band's rows are all that can make progress), so such a sweep is
// capped there and the increment gets the other CUs at full occupancy.  One tile per workgroup (a dense system, 67 KB) or a wider
// band: the shape of oisat_trsv_plan, unchanged.
constexpr int kIncOverlapSweepWgs = 128;
extern "C" int oisat_trsv_plan_overlap(int64_t nb, int band, int cu_count, int32_t* two_tiles_out, int32_t* grid_out) {
    int32_t two = 0, grid = 0;
    if (int rc = oisat_trsv_plan(nb, band, cu_count, &two, &grid)) return rc;
    if (two && band > 0 && band <= kIncOverlapSweepWgs && grid > kIncOverlapSweepWgs) grid = kIncOverlapSweepWgs;
    if (two_tiles_out) *two_tiles_out = two;
    if (grid_out) *grid_out = grid;
    return OISAT_OK;
}

// Where DenseAnalysis.run takes oisat_gain_solve_fields instead of oisat_gain_solve + oisat_apply_increment_grid (host only).
// Legal: one system, the Gaussian (the update is its packed-fp32 form), at least one refinement round (the guard reads the first
// residual), fields wanted, no drift (its increment is another vector's).  Worth it: the update costs 0.7 ms at the headline's grid
// and nothing is hidden but the two sweeps of the first correction, 2 x 3.3 us per block row -- so at least kIncOverlapMinRows = 256
// block rows (1.7 ms of sweeps; the headline has 782, BASELINE's config 2 has 79 and keeps the two calls).  The bound is reasoned;
// measured is the headline alone: 1.0 ms of 63 (profiles/EXPERIMENTS.md, "The increment under the correction's sweeps").
// OISAT_INC_OVERLAP=0: nowhere; 1: wherever it is legal, whatever the size (tests); unset: kIncOverlapDefault decides whether the
// rule is in force at all.
constexpr int kIncOverlapMinRows = 256;
constexpr bool kIncOverlapDefault = true;
extern "C" int oisat_inc_overlap_plan(int64_t nb, int nsys, int corr_kind, int refine, int fields, int drift, int32_t* use_out) {
    ARG_CHECK(nb >= 1 && nsys >= 1 && refine >= 0 && use_out != nullptr);
    const int mode = inc_overlap_mode();
    ARG_CHECK(mode != -2 && "OISAT_INC_OVERLAP is 0 or 1");
    const bool legal = nsys == 1 && corr_kind == OISAT_CORR_GAUSSIAN && refine > 0 && fields != 0 && drift == 0;
    *use_out = legal && mode != 0 && (mode == 1 || (kIncOverlapDefault && nb >= kIncOverlapMinRows)) ? 1 : 0;
    return OISAT_OK;
}

// OISAT_TRSV_TWO_TILES=0|1 forces the choice of oisat_trsv_plan, OISAT_TRSV_MAX_WGS=<n >= 1> caps the sweeps' grid (A/B runs,
// tests: a few workgroups serving many rows each at a small size); read at every call, like OISAT_ENVELOPE.  Forcing two tiles
// is always legal: a row waits only for lower tickets, and every claimed ticket is held by a running workgroup.
static int trsv_launch_shape(const oisat_ctx* h, const ChFactor& f, int nb, int* two_out, int* grid_out) {
    int32_t two = 0, grid = 0;
    if (int rc = oisat_trsv_plan(nb, f.env != nullptr ? f.band : 0, h->cu_count, &two, &grid)) return rc;
    const int forced = trsv_two_tiles_forced();
    ARG_CHECK(forced != -2 && "OISAT_TRSV_TWO_TILES is 0 or 1");
    if (forced >= 0) {
        two = forced;
        grid = two && h->cu_count > 0 ? std::min(nb, h->cu_count) : nb;
    }
    // while the side stream's increment is in flight (oisat_gain_solve_fields) the two-tile sweeps leave it half the CUs
    if (h->inc_in_flight && forced < 0)
        if (int rc = oisat_trsv_plan_overlap(nb, f.env != nullptr ? f.band : 0, h->cu_count, &two, &grid)) return rc;
    long cap = 0;
    const int capped = trsv_max_wgs(&cap);
    ARG_CHECK(capped >= 0 && "OISAT_TRSV_MAX_WGS is an integer >= 1");
    if (capped && cap < grid) grid = (int32_t)cap;
    *two_out = two;
    *grid_out = grid;
    return OISAT_OK;
}

int trsv_solve(oisat_ctx* h, const ChFactor& f, double* rhs_pad, double* fwd, const SolveState* st, double* zout, int accumulate,
               bool fwd_done = false) {
    const int nb = (int)(f.mp / NB);
    const size_t ctl_bytes = kCtlBytes;
    char* base = nullptr;
    if (int rc = status_ws(h, nullptr, &base)) return rc;
    unsigned* err_total = (unsigned*)base;
    char* ctl = base + 16;
    // (rows per workgroup are not fixed: a workgroup claims rows by ticket until none is left.  A dense system on a quarter of
    // the workgroups: 0.54 vs 0.25 ms per sweep at 1e4 observations -- there every row has work from the start.)
    int two = 0, grid = 0;
    if (int rc = trsv_launch_shape(h, f, nb, &two, &grid)) return rc;
    const size_t shm = sizeof(float) * NB * TLD * (two ? 2 : 1);
    if (!fwd_done) {
        OISAT_LAUNCH(h, "trsv_fwd", (trsv_pipe_kernel<0>), dim3(grid), dim3(256), shm, f.S, f.ld, (const float*)f.tinv, nb, rhs_pad, fwd,
                     (TrsvCtl*)ctl, err_total, two, st, (double*)nullptr, (int64_t)0, 0, f.env);
    }
    OISAT_LAUNCH(h, "trsv_bwd", (trsv_pipe_kernel<1>), dim3(grid), dim3(256), shm, f.S, f.ld, (const float*)f.tinv, nb, fwd, rhs_pad,
                 (TrsvCtl*)(ctl + ctl_bytes), err_total, two, st, zout, f.m, accumulate, f.env);
    return OISAT_OK;
}

}  // namespace

extern "C" int oisat_set_refine_tol(oisat_ctx* h, double tol) {
    ARG_CHECK(h != nullptr && tol >= 0.0 && tol < 1.0);
    h->refine_tol = tol;
    return OISAT_OK;
}

// ---- oisat_potrs' correction against the factor itself ----------------------------------------------------------------------------
// The sweeps multiply by the inverted diagonal blocks T_b, which are float32 products (a few 2^-24 from the exact inverses):
// one solve is as far from L^-T L^-1 d as a float32 substitution.  oisat_potrs therefore corrects once against L L^T in
// double: x1 = M^-1 d, r = d - L (L^T x1), x = x1 + M^-1 r, after which T_b's error enters squared.  Only the lower triangle
// is read (the diagonal tiles' upper halves are not part of the factor), and of an enveloped factor only the blocks inside
// the envelope: env = first[nb] | last[nb] as in the sweeps, clamped.  Plain kernels: oisat_potrs is no hot path.
// t[c] = sum_{r >= c} L[r][c] x[r], one thread per column, rows in ascending order (coalesced across the columns)
static __global__ __launch_bounds__(256) void potrs_lt_kernel(const float* __restrict__ L, int64_t ld, int64_t mp, const double* __restrict__ x,
                                                               const int* __restrict__ env, double* __restrict__ t) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= mp) return;
    const int64_t nb = mp / NB, cb = c / NB;
    int64_t lastb = nb - 1;
    if (env != nullptr) {
        lastb = env[nb + cb];
        lastb = lastb < cb ? cb : (lastb > nb - 1 ? nb - 1 : lastb);
    }
    double s = 0.0;
    for (int64_t r = c; r < (lastb + 1) * NB; ++r) s += (double)L[r * ld + c] * x[r];
    t[c] = s;
}

// out[r] = d[r] - sum_{c <= r} L[r][c] t[c] for r < m, 0 in the padding; one wave per row, fixed shuffle tree
static __global__ __launch_bounds__(256) void potrs_resid_kernel(const float* __restrict__ L, int64_t ld, int64_t m, int64_t mp,
                                                                  const double* __restrict__ t, const double* __restrict__ d,
                                                                  const int* __restrict__ env, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= mp) return;
    if (r >= m) {
        if (lane == 0) out[r] = 0.0;
        return;
    }
    const int64_t rb = r / NB;
    int64_t firstb = 0;
    if (env != nullptr) {
        firstb = env[rb];
        firstb = firstb < 0 ? 0 : (firstb > rb ? rb : firstb);
    }
    const float* row = L + r * ld;
    double s = 0.0;
    for (int64_t c = firstb * NB + lane; c <= r; c += 64) s += (double)row[c] * t[c];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, kWave);
    if (lane == 0) out[r] = d[r] - s;
}

extern "C" int oisat_potrs(oisat_ctx* h, const float* L, int64_t m, int64_t ld, double* z_inout) {
    ARG_CHECK(h && L && z_inout && m > 0);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);     // must follow oisat_potrf of this matrix
    h->factor.fwd_d = nullptr;                                  // (the work vectors are about to be reused)
    const int64_t mp = h->factor.mp;                           // (mp / 4 workgroups at the most below: far from 2^31 for any factor that exists)
    double* w = (double*)oisat_ws(h, 5, sizeof(double) * (2 + 8) * mp);
    if (!w) return OISAT_ENOMEM;
    double* rhs = w;
    double* fwd = w + mp;
    double* lt = w + 2 * mp;                                    // L^T x1
    double* d = w + 3 * mp;                                     // the right-hand side: z_inout is about to take x1
    HIP_TRY(hipMemcpyAsync(d, z_inout, sizeof(double) * m, hipMemcpyDeviceToDevice, h->stream));
    OISAT_LAUNCH(h, "copy_pad", solve_prep_kernel, dim3(stream_grid(mp, 256)), dim3(256), 0, (const double*)z_inout, m, mp, rhs, fwd,
                 (SolveState*)nullptr);
    if (int rc = trsv_solve(h, h->factor, rhs, fwd, nullptr, z_inout, 0)) return rc;          // rhs <- x1 (padded), fwd re-armed
    OISAT_LAUNCH(h, "potrs_lt", potrs_lt_kernel, dim3((unsigned)cdiv(mp, 256)), dim3(256), 0, h->factor.S, ld, mp, (const double*)rhs,
                 (const int*)h->factor.env, lt);
    OISAT_LAUNCH(h, "potrs_resid", potrs_resid_kernel, dim3((unsigned)cdiv(mp * 64, 256)), dim3(256), 0, h->factor.S, ld, m, mp,
                 (const double*)lt, (const double*)d, (const int*)h->factor.env, rhs);
    return trsv_solve(h, h->factor, rhs, fwd, nullptr, z_inout, 1);                             // z_inout += M^-1 r
}

// z = S^-1 d through the fp32 factor as a preconditioner:  z <- M^-1 d;  repeat { r = d - S z (float64, S regenerated from
// coordinates);  stop if |r| <= tol |d|;  z <- z + M^-1 r }  at most `refine` times.  tol = 1e-6 (oisat_set_refine_tol; env OISAT_REFINE_TOL at init): the
// analysis increment is K r away from the exact one and |K| <= 1, so the fields are then 1e-6 |d| from the float64 answer,
// ten times inside the 1e-5 bar; a factor that is a good preconditioner (|r_0| / |d| = 2e-6 .. 2e-5 on the BASELINE
// workloads, 1e-9 .. 1e-10 after one correction) stops after one correction, a poor one gets all `refine` of them.  The
// test runs on the device: resid_check_kernel sets a flag and the launches of the rounds that follow return at once, so
// nothing waits for the host.  Launches: prep, 2 sweeps, then per round residual (written straight into the padded right-
// hand side), check, 2 sweeps (the backward one adds its solution to z): no fills, no copies.
// fo (or nullptr: oisat_gain_solve): the fields of oisat_gain_solve_fields, below, which the same body writes
namespace {
struct IncFields {                                              // the grid and the fields of oisat_gain_solve_fields
    int dtype;
    const double *gxyz, *gsig;
    int64_t ny, nx;
    const void* xb;
    void *xa, *inc;
    const double* glat;
};
// the side stream's launch is joined on every way out of the solve: the main stream waits for its event, so the handle's buffers
// stay ordered behind the owning stream whatever the call returns
struct IncSideJoin {
    oisat_ctx* h;
    bool forked = false;
    int join() {
        h->inc_in_flight = false;
        if (!forked) return OISAT_OK;
        forked = false;
        HIP_TRY(hipStreamWaitEvent(h->stream, h->inc_join, 0));
        return OISAT_OK;
    }
    ~IncSideJoin() { (void)join(); }
};
}  // namespace

static int gain_solve_impl(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                           int64_t ld, double g, const double* d, int refine, double* z_out, double* resid_host,
                           const double* olat_sorted, const IncFields* fo) {
    ARG_CHECK(h != nullptr);
    const int* perm = oisat_take_obs_perm(h, m);               // one-shot, whatever this call's outcome
    // the forward vector of this very d, left by oisat_potrf_env_fwd's launch: consumed once, whatever this call's outcome
    const bool fwd_done = h->factor.fwd_d != nullptr && h->factor.fwd_d == d;
    h->factor.fwd_d = nullptr;
    ARG_CHECK(L && oxyz && osig && ovar && d && z_out && m > 0 && refine >= 0 && refine <= 8);
    ARG_CHECK(h->factor.S == L && h->factor.m == m && h->factor.ld == ld);
    const int upd_mode = resid_update_mode();
    ARG_CHECK(upd_mode >= 0 && "OISAT_RESID_UPDATE is 0 or 1");
    const double tol = h->refine_tol;
    const int64_t mp = h->factor.mp;
    double* w = (double*)oisat_ws(h, 5, sizeof(double) * (2 + 8) * mp);
    SolveState* st = solve_state(h);
    if (!w || !st) return OISAT_ENOMEM;
    double* rhs = w;
    double* fwd = w + mp;
    if (!fwd_done) {
        OISAT_LAUNCH(h, "copy_pad", solve_prep_kernel, dim3(stream_grid(mp, 256)), dim3(256), 0, d, m, mp, rhs, fwd, st);
    }
    int rc = trsv_solve(h, h->factor, rhs, fwd, nullptr, z_out, 0, fwd_done);
    if (rc) return rc;
    // The fields of the first solve's z0, underneath what follows (oisat_gain_solve_fields): z0 is snapshot on the main stream -- the
    // backward sweeps of the corrections add into z_out while the side stream reads -- and the side stream, behind an event, runs
    // the float64 increment of the snapshot into a double scratch field.  Profiling (HIP events on the launch stream cannot time
    // another stream's kernel): the same launch on the main stream, serial, same bits.
    IncSideJoin side{h};
    double *inc0 = nullptr, *z0 = nullptr;
    if (fo != nullptr) {
        const int64_t n = fo->ny * fo->nx;
        inc0 = (double*)oisat_ws(h, 14, sizeof(double) * (size_t)(n + m + 2));
        if (!inc0) return OISAT_ENOMEM;
        z0 = inc0 + ((n + 1) & ~(int64_t)1);
        HIP_TRY(hipMemcpyAsync(z0, z_out, sizeof(double) * m, hipMemcpyDeviceToDevice, h->stream));
        if (!h->prof) {
            if (!h->inc_stream) {
                int prio_low = 0, prio_high = 0;
                HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
                HIP_TRY(hipStreamCreateWithPriority(&h->inc_stream, hipStreamNonBlocking, prio_low));   // the sweeps come first
                HIP_TRY(hipEventCreateWithFlags(&h->inc_fork, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&h->inc_join, hipEventDisableTiming));
            }
            hipStream_t main_stream = h->stream;
            HIP_TRY(hipEventRecord(h->inc_fork, main_stream));
            HIP_TRY(hipStreamWaitEvent(h->inc_stream, h->inc_fork, 0));
            h->stream = h->inc_stream;                           // (the launch goes to the side stream)
            rc = oisat_increment_scratch(h, fo->gxyz, fo->gsig, fo->ny, fo->nx, oxyz, osig, z0, m, g, inc0, fo->glat, olat_sorted);
            const hipError_t er = rc == OISAT_OK ? hipEventRecord(h->inc_join, h->inc_stream) : hipSuccess;
            h->stream = main_stream;
            if (rc) return rc;
            HIP_TRY(er);
            side.forked = true;
            h->inc_in_flight = true;                             // the sweeps launched from here to the join leave it CUs
        } else {
            rc = oisat_increment_scratch(h, fo->gxyz, fo->gsig, fo->ny, fo->nx, oxyz, osig, z0, m, g, inc0, fo->glat, olat_sorted);
            if (rc) return rc;
        }
    }
    // the residual is evaluated once more behind the last allowed correction: a converged solve skips it (no-op launches), one
    // that is still above the tolerance there is recorded in the handle's status (oisat_solve_status_ex)
    int* info_dev = nullptr;
    if (int rs = status_ws(h, &info_dev, nullptr)) return rs;
    // (refine = 0 asks for the plain solve: no residual is formed -- unless the caller wants it reported -- and nothing is flagged)
    // Behind a correction (it >= 1) the residual is first formed as an update of the last fully evaluated one, r_keep - S dz with
    // S dz in packed fp32 (dz: what the backward sweep left in the padded right-hand side).  If that already proves the
    // tolerance met (resid_update_check_kernel) the solve is converged and everything below returns at once; if not, nothing
    // has changed and the float64 residual decides.  Gaussian on compact blocks with a tolerance only; vectors 2 and 3 of the
    // slot (free here: the sliced residual's partial sums belong to the latitude-row form, oisat_potrs is another call).
    const bool upd =upd_mode == 1 && refine > 0 && tol > 0.0 && oisat_resid_update_applies(h, g, olat_sorted, perm);
    double* r_keep = upd ? w + 2 * mp : nullptr;
    double* r_upd = w + 3 * mp;
    for (int it = 0; it <= refine && (refine > 0 || resid_host); ++it) {
        if (upd && it >= 1) {
            rc = oisat_cov_residual_update_if(h, oxyz, osig, ovar, m, g, r_keep, rhs, r_upd, olat_sorted, &st->conv, perm);
            if (rc) return rc;
            OISAT_LAUNCH(h, "resid_update_check", resid_update_check_kernel, dim3(1), dim3(1024), 0, (const double*)r_upd, m, it, tol,
                         oisat_resid_update_c(), st);
        }
        rc = oisat_cov_residual_if(h, oxyz, osig, ovar, m, g, d, z_out, rhs, olat_sorted, &st->conv, perm);
        if (rc) return rc;
        OISAT_LAUNCH(h, "resid_check", resid_check_kernel, dim3(1), dim3(1024), 0, (const double*)rhs, d, m, it, tol * tol, st,
                     it == refine && refine > 0 ? 1 : 0, info_dev, it < refine ? r_keep : (double*)nullptr);
        if (it == refine) break;
        rc = trsv_solve(h, h->factor, rhs, fwd, st, z_out, 1);
        if (rc) return rc;
    }
    if (fo != nullptr) {
        // join, then the fields: T(inc0 + B H^T (z - z0)) where the guard lets the fp32 update apply, the float64 increment of the
        // final z where it does not -- one of the two launches returns at once
        if (int rj = side.join()) return rj;
        rc = oisat_increment_update_if(h, fo->dtype, fo->gxyz, fo->gsig, fo->ny, fo->nx, oxyz, osig, z_out, z0, m, g, fo->xb, fo->xa, fo->inc,
                                       inc0, fo->glat, olat_sorted, st, oisat_inc_update_t());
        if (rc) return rc;
    }
    if (resid_host) {
        char* pin = (char*)oisat_pinned(h, 512);
        if (!pin) return OISAT_ENOMEM;
        HIP_TRY(hipMemcpyAsync(pin, st, sizeof(SolveState), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(pin + 256, h->ws[7], sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const SolveState* hs = (const SolveState*)pin;
        const double dn = hs->dd > 0.0 ? sqrt(hs->dd) : 1.0;
        for (int it = 0; it <= refine; ++it) {                  // rounds that were skipped after convergence repeat the last residual
            const int k = it < hs->computed ? it : hs->computed - 1;
            resid_host[it] = k >= 0 ? sqrt(hs->norm[k]) / dn : 0.0;
        }
        const unsigned gave_up = *(const unsigned*)(pin + 256);
        if (gave_up != 0) {
            HIP_TRY(hipMemsetAsync(h->ws[7], 0, 16, h->stream));          // reported here, not again by oisat_solve_status
            oisat_set_error("triangular solve: %u workgroup(s) gave up waiting for a predecessor (bounded spin)", gave_up);
            return OISAT_EHIP;
        }
    }
    return OISAT_OK;
}

extern "C" int oisat_gain_solve(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                                int64_t ld, double g, const double* d, int refine, double* z_out, double* resid_host,
                                const double* olat_sorted) {
    return gain_solve_impl(h, L, oxyz, osig, ovar, m, ld, g, d, refine, z_out, resid_host, olat_sorted, nullptr);
}

// oisat_gain_solve followed by oisat_apply_increment_grid, with the increment of the FIRST solve's z0 on the handle's side stream
// underneath the correction's residual and sweeps, and what the correction adds to it as a packed-fp32 update behind them
// (dense_inc_update.inc).  Gaussian, refine >= 1.  All ordering is by events; the call returns with the side stream joined.
extern "C" int oisat_gain_solve_fields(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                                       int64_t ld, double g, const double* d, int refine, double* z_out, double* resid_host,
                                       const double* olat_sorted, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx,
                                       const void* xb, void* xa, void* inc, const double* glat) {
    ARG_CHECK(h != nullptr);
    if (!(h->corr == OISAT_CORR_GAUSSIAN && refine >= 1 && refine <= 8 && gxyz && gsig && ny > 0 && nx > 0 && nx < (int64_t)INT32_MAX &&
          (xa || inc) && (!xa || xb) && (dtype == OISAT_F32 || dtype == OISAT_F64) && z_out && m > 0)) {
        (void)oisat_take_obs_perm(h, m);                        // one-shot, whatever this call's outcome
        h->factor.fwd_d = nullptr;
        oisat_set_error("oisat_gain_solve_fields: Gaussian correlation, 1 <= refine <= 8, a grid and its fields are required");
        return OISAT_EINVAL;
    }
    const IncFields fo{dtype, gxyz, gsig, ny, nx, xb, xa, inc, glat};
    return gain_solve_impl(h, L, oxyz, osig, ovar, m, ld, g, d, refine, z_out, resid_host, olat_sorted, &fo);
}

// words of oisat_solve_status_ex (include/oisat.h: OISAT_STATUS_*)
extern "C" int oisat_solve_status_ex(oisat_ctx* h, int32_t* out, int nwords, int clear) {
    ARG_CHECK(h != nullptr && (out != nullptr || nwords == 0) && nwords >= 0 && nwords <= OISAT_STATUS_WORDS);
    int* info = nullptr;
    char* base = nullptr;
    if (int rc = status_ws(h, &info, &base)) return rc;
    int* pin = (int*)oisat_pinned(h, 256);
    if (!pin) return OISAT_ENOMEM;
    HIP_TRY(hipMemcpyAsync(pin, info, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(pin + 8, base, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (clear) {
        HIP_TRY(hipMemsetAsync(info + 1, 0, 2 * sizeof(int), h->stream));
        HIP_TRY(hipMemsetAsync(info + kInfoUnconverged, 0, 3 * sizeof(int), h->stream));
        HIP_TRY(hipMemsetAsync(base, 0, 16, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int32_t words[OISAT_STATUS_WORDS] = {pin[1], pin[2], pin[8], pin[kInfoUnconverged], pin[kInfoUnconvergedMember] - 1,
                                               pin[kInfoDagTimeouts]};
    for (int i = 0; i < nwords; ++i) out[i] = words[i];
    return OISAT_OK;
}

extern "C" int oisat_solve_status(oisat_ctx* h, int* first_notpd_col, int* n_notpd_blocks, int* trsv_timeouts, int clear) {
    int32_t w[OISAT_STATUS_WORDS];
    // (kept for callers of the round-2 ABI: the three words it knows; a clear resets all six, so such a caller folds the
    // others into the time-out count rather than lose them)
    if (int rc = oisat_solve_status_ex(h, w, OISAT_STATUS_WORDS, clear)) return rc;
    if (first_notpd_col) *first_notpd_col = w[OISAT_STATUS_NOTPD_COL];
    if (n_notpd_blocks) *n_notpd_blocks = w[OISAT_STATUS_NOTPD_BLOCKS];
    if (trsv_timeouts) *trsv_timeouts = w[OISAT_STATUS_TRSV_TIMEOUTS] + w[OISAT_STATUS_DAG_TIMEOUTS] + w[OISAT_STATUS_UNCONVERGED];
    return OISAT_OK;
}

extern "C" int oisat_dense_reserve(oisat_ctx* h, int64_t max_obs, int64_t diag_chunk_rows) {
    ARG_CHECK(h != nullptr && max_obs > 0 && diag_chunk_rows >= 0);
    const int64_t mp = cdiv(max_obs, NB) * NB;
    if (!oisat_ws(h, 3, sizeof(float) * mp * NB)) return OISAT_ENOMEM;                  // inverted diagonal blocks
    if (int rc = status_ws(h, nullptr, nullptr)) return rc;                              // slots 4 and 7
    if (!oisat_ws(h, 5, sizeof(double) * (2 + 8) * mp)) return OISAT_ENOMEM;                   // padded rhs + forward solution
    if (!solve_state(h)) return OISAT_ENOMEM;                                            // slot 9: convergence state of the gain solve
    size_t s6 = sizeof(double) * (max_obs + 16);                                         // refinement residual
    if (diag_chunk_rows > 0) {
        const int64_t ch = cdiv(diag_chunk_rows, NB) * NB;
        const size_t x = sizeof(float) * ch * mp + sizeof(double) * ch;                 // posterior-error / gain-diag rows
        if (x > s6) s6 = x;
    }
    if (!oisat_ws(h, 6, s6)) return OISAT_ENOMEM;
    if (!oisat_pinned(h, 4096)) return OISAT_ENOMEM;
    return OISAT_OK;
}

// ---- batched factorization ---------------------------------------------------------------------------------------
extern "C" int oisat_batch_create(oisat_ctx* h, int nmat, float* const* S, const int64_t* m, const int64_t* ld, float* const* tinv,
                                  int* batch_id_out) {
    ARG_CHECK(h && S && m && ld && tinv && batch_id_out && nmat > 0 && nmat <= 65535);
    ChBatch* bt = new ChBatch();
    bt->order.resize(nmat);
    for (int i = 0; i < nmat; ++i) bt->order[i] = i;
    for (int i = 0; i < nmat; ++i) {
        const int64_t mp = cdiv(m[i], NB) * NB;
        if (!(S[i] && tinv[i] && m[i] > 0 && ld[i] >= mp && (ld[i] % 4) == 0 && ((uintptr_t)S[i] % 16) == 0 && ((uintptr_t)tinv[i] % 16) == 0 &&
              mp / NB < (int64_t)INT32_MAX)) {
            delete bt;
            oisat_set_error("oisat_batch_create: matrix %d: bad pointer, size or leading dimension", i);
            return OISAT_EINVAL;
        }
    }
    // largest first (stable): the matrices a node of the recursion applies to are then a prefix of the table
    std::stable_sort(bt->order.begin(), bt->order.end(), [&](int a, int b) { return cdiv(m[a], NB) > cdiv(m[b], NB); });
    bt->table.resize(nmat);
    for (int i = 0; i < nmat; ++i) {
        const int k = bt->order[i];
        bt->table[i] = BatchMat{S[k], tinv[k], ld[k], m[k], (int)cdiv(m[k], NB), 0};
    }
    bt->max_mpb = bt->table[0].mpb;
    bt->pairs = kLeafPairsMin > 0 && nmat >= kLeafPairsMin;
    if (hipMalloc(&bt->table_dev, sizeof(BatchMat) * nmat) != hipSuccess) {
        delete bt;
        oisat_set_error("oisat_batch_create: hipMalloc of the table failed");
        return OISAT_ENOMEM;
    }
    if (hipMemcpy(bt->table_dev, bt->table.data(), sizeof(BatchMat) * nmat, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(bt->table_dev);
        delete bt;
        oisat_set_error("oisat_batch_create: upload of the table failed");
        return OISAT_EHIP;
    }
    {
        std::vector<int> host;
        build_cum_tables(bt, host);
        if (hipMalloc(&bt->cum_dev, sizeof(int) * host.size()) != hipSuccess ||
            hipMemcpy(bt->cum_dev, host.data(), sizeof(int) * host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            if (bt->cum_dev) (void)hipFree(bt->cum_dev);
            (void)hipFree(bt->table_dev);
            delete bt;
            oisat_set_error("oisat_batch_create: tile-enumeration tables failed");
            return OISAT_ENOMEM;
        }
    }
    bool want_dag = dag_wanted(h, bt->max_mpb, nmat);
    if (want_dag) {                                          // would its chains crowd out the tasks they wait for?  (host-only check)
        std::vector<int> nb_of(nmat);
        for (int i = 0; i < nmat; ++i) nb_of[i] = bt->table[i].mpb;
        DagOrder probe;
        dag_task_order(nb_of, 0, probe);
        want_dag = dag_fits(probe.max_wave_chains, dag_slots(h));        // no: the batch keeps the lock-step recursion
    }
    if (want_dag) {
        bt->dag = dag_plan_create(bt->table, h->stream);
        if (bt->dag && hipStreamSynchronize(h->stream) != hipSuccess) {       // (the plan's words are zero before any stream can launch it)
            oisat_dag_plan_release(bt->dag);
            bt->dag = nullptr;
        }
        if (!bt->dag) {
            (void)hipFree(bt->cum_dev);
            (void)hipFree(bt->table_dev);
            delete bt;
            return OISAT_ENOMEM;
        }
    }
    int id = -1;
    for (size_t i = 0; i < h->batches.size(); ++i)
        if (!h->batches[i]) { id = (int)i; break; }
    if (id < 0) { h->batches.push_back(nullptr); id = (int)h->batches.size() - 1; }
    h->batches[id] = bt;
    *batch_id_out = id;
    return OISAT_OK;
}

extern "C" int oisat_batch_destroy(oisat_ctx* h, int batch_id) {
    ARG_CHECK(h && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    HIP_TRY(hipStreamSynchronize(h->stream));
    ChBatch* bt = h->batches[batch_id];
    if (bt->table_dev) HIP_TRY(hipFree(bt->table_dev));
    if (bt->cum_dev) HIP_TRY(hipFree(bt->cum_dev));
    if (bt->solve_dev) HIP_TRY(hipFree(bt->solve_dev));
    if (bt->ord_dev) HIP_TRY(hipFree(bt->ord_dev));
    if (bt->ctl_dev) HIP_TRY(hipFree(bt->ctl_dev));
    oisat_dag_plan_release(bt->dag);
    oisat_dag_plan_release(bt->dag_solve);
    delete bt;
    h->batches[batch_id] = nullptr;
    return OISAT_OK;
}

extern "C" int oisat_batch_set_solve(oisat_ctx* h, int batch_id, int nmat, const double* const* oxyz, const double* const* osig,
                                     const double* const* ovar, const double* const* d, const double* const* olat, double* const* z,
                                     double* const* work, void* const* state, const double* const* gxyz, const double* const* gsig,
                                     const double* const* glat, const int64_t* n, const void* const* xb, void* const* xa,
                                     void* const* inc) {
    ARG_CHECK(h && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    ChBatch* bt = h->batches[batch_id];
    ARG_CHECK(nmat == (int)bt->table.size());
    ARG_CHECK(oxyz && osig && ovar && d && olat && z && work && state && gxyz && gsig && glat && n && xb && xa && inc);
    std::vector<SolveMember> mem(nmat);
    std::vector<int> ord;
    int64_t max_m = 0, max_n = 0, max_mp = 0;               // (committed behind the checks: a refused call leaves the batch as it was)
    for (int i = 0; i < nmat; ++i) {                         // table order (largest first); order[i] = the caller's index
        const int c = bt->order[i];
        const BatchMat& bm = bt->table[i];
        ARG_CHECK(oxyz[c] && osig[c] && ovar[c] && d[c] && olat[c] && z[c] && work[c] && state[c] && gxyz[c] && gsig[c] && glat[c]);
        ARG_CHECK(n[c] > 0 && xb[c] && (xa[c] || inc[c]) && bm.mpb < 4096);
        SolveMember& sm = mem[i];
        sm.S = bm.S; sm.tinv = bm.tinv; sm.ld = bm.ld; sm.m = bm.m; sm.mpb = bm.mpb; sm.nx = 0;
        sm.oxyz = oxyz[c]; sm.osig = osig[c]; sm.ovar = ovar[c]; sm.d = d[c]; sm.olat = olat[c];
        sm.z = z[c]; sm.rhs = work[c]; sm.fwd = work[c] + (int64_t)bm.mpb * NB; sm.st = (SolveState*)state[c];
        sm.gxyz = gxyz[c]; sm.gsig = gsig[c]; sm.glat = glat[c]; sm.n = n[c]; sm.xb = xb[c]; sm.xa = xa[c]; sm.inc = inc[c];
        sm.perm = nullptr;
        sm.which = c;
        if (bm.m > max_m) max_m = bm.m;
        if (n[c] > max_n) max_n = n[c];
        if ((int64_t)bm.mpb * NB > max_mp) max_mp = (int64_t)bm.mpb * NB;
    }
    bt->max_m = max_m; bt->max_n = max_n; bt->max_mp = max_mp;
    // ticket -> (member, step): steps ascending, members in table order inside a step (a prefix: sorted by block count)
    for (int k = 0; k < bt->max_mpb; ++k)
        for (int i = 0; i < nmat && bt->table[i].mpb > k; ++i) ord.push_back((i << 12) | k);
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (bt->solve_dev) HIP_TRY(hipFree(bt->solve_dev));
    if (bt->ord_dev) HIP_TRY(hipFree(bt->ord_dev));
    if (bt->ctl_dev) HIP_TRY(hipFree(bt->ctl_dev));
    bt->solve_dev = nullptr; bt->ord_dev = nullptr; bt->ctl_dev = nullptr;
    HIP_TRY(hipMalloc((void**)&bt->solve_dev, sizeof(SolveMember) * nmat));
    HIP_TRY(hipMalloc((void**)&bt->ord_dev, sizeof(int) * ord.size()));
    HIP_TRY(hipMalloc(&bt->ctl_dev, 2 * kCtlBytes));
    bt->solve_host = mem;
    bt->max_patches = 0;
    HIP_TRY(hipMemcpy(bt->solve_dev, mem.data(), sizeof(SolveMember) * nmat, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bt->ord_dev, ord.data(), sizeof(int) * ord.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(bt->ctl_dev, 0, 2 * kCtlBytes));
    bt->ord_total = (int)ord.size();
    oisat_dag_plan_release(bt->dag_solve);
    bt->dag_solve = nullptr;
    return OISAT_OK;
}

// Width of every member's cell grid (its n cells are ny x nx, row-major), in the caller's member order; 0 = unknown.  The
// increment then works on compact patches of cells and skips the observations beyond the covariance's reach of a patch.
// perm (optional; entries may be NULL): member i's observations along a space-filling curve (dev int32[m_i], a permutation
// of its latitude order): the float64 residual then works on compact blocks of rows with the same cull.
extern "C" int oisat_batch_set_grid(oisat_ctx* h, int batch_id, int nmat, const int64_t* nx, const int32_t* const* perm) {
    ARG_CHECK(h && nx && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    ChBatch* bt = h->batches[batch_id];
    ARG_CHECK(nmat == (int)bt->table.size() && bt->solve_dev != nullptr && (int)bt->solve_host.size() == nmat);
    for (int i = 0; i < nmat; ++i) {                         // (every check before the first change: a refused call leaves the batch as it was)
        const int64_t w = nx[bt->order[i]];
        ARG_CHECK(w >= 0 && w < (int64_t)INT32_MAX && (w == 0 || bt->solve_host[i].n % w == 0));
    }
    for (int i = 0; i < nmat; ++i) {
        const int64_t w = nx[bt->order[i]];
        SolveMember& sm = bt->solve_host[i];
        sm.nx = (int)w;
        sm.perm = perm ? perm[bt->order[i]] : nullptr;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(bt->solve_dev, bt->solve_host.data(), sizeof(SolveMember) * nmat, hipMemcpyHostToDevice));
    oisat_dag_plan_release(bt->dag_solve);                  // (its increment patches depend on the grids' shapes)
    bt->dag_solve = nullptr;
    return OISAT_OK;
}

// the gain solve + increment of every member, each launch covering all of them (per member the arithmetic and the bits of
// oisat_gain_solve + oisat_apply_increment(_grid), except that the single call slices its latitude-row residual and this one does
// not -- include/oisat.h; same stopping rule, per member)
extern "C" int oisat_batch_solve(oisat_ctx* h, int batch_id, int dtype, double g, int refine) {
    ARG_CHECK(h && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    ChBatch& bt = *h->batches[batch_id];
    ARG_CHECK(bt.solve_dev != nullptr && bt.ord_total > 0 && refine >= 0 && refine <= 8 && g >= 0.0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    char* base = nullptr;
    if (int rc = status_ws(h, nullptr, &base)) return rc;
    HIP_TRY(dense_kernel_attributes());
    unsigned* err_total = (unsigned*)base;
    const int nmem = (int)bt.table.size();
    const SolveMember* mem = bt.solve_dev;
    TrsvCtl* ctl_f = (TrsvCtl*)bt.ctl_dev;
    TrsvCtl* ctl_b = (TrsvCtl*)((char*)bt.ctl_dev + kCtlBytes);
    const size_t shm = sizeof(float) * NB * TLD;
    // persistent workgroups: two per CU (66 KB of LDS each) or one per row if there are fewer rows
    const int slots = 2 * (h->cu_count > 0 ? h->cu_count : 256);
    const int grid = bt.ord_total < slots ? bt.ord_total : slots;
    const double tol = h->refine_tol;
    OISAT_LAUNCH(h, "copy_pad", solve_prep_batched_kernel, dim3((unsigned)stream_grid(bt.max_mp, 256) > 64u ? 64u : (unsigned)stream_grid(bt.max_mp, 256), (unsigned)nmem),
                 dim3(256), 0, mem);
    auto sweeps = [&](int first, int accumulate) -> int {
        OISAT_LAUNCH(h, "trsv_fwd", (trsv_batched_kernel<0>), dim3(grid), dim3(256), shm, mem, (const int*)bt.ord_dev, bt.ord_total, ctl_f,
                     err_total, first, 0);
        OISAT_LAUNCH(h, "trsv_bwd", (trsv_batched_kernel<1>), dim3(grid), dim3(256), shm, mem, (const int*)bt.ord_dev, bt.ord_total, ctl_b,
                     err_total, first, accumulate);
        return OISAT_OK;
    };
    int rc = sweeps(1, 0);
    if (rc) return rc;
    int* info_dev = nullptr;
    if (int rs = status_ws(h, &info_dev, nullptr)) return rs;
    for (int it = 0; it <= refine && refine > 0; ++it) {    // (the last evaluation only runs for members that are still above the tolerance)
        rc = oisat_cov_residual_batched(h, mem, bt.solve_host, bt.max_m, g);
        if (rc) return rc;
        OISAT_LAUNCH(h, "resid_check", resid_check_batched_kernel, dim3((unsigned)nmem), dim3(1024), 0, mem, it, tol * tol,
                     it == refine ? 1 : 0, info_dev);
        if (it == refine) break;
        rc = sweeps(0, 1);
        if (rc) return rc;
    }
    return oisat_apply_increment_batched(h, dtype, mem, bt.solve_host, bt.max_n, g);
}

extern "C" int oisat_batch_is_task_graph(oisat_ctx* h, int batch_id, int* yes_out) {
    ARG_CHECK(h && yes_out && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    *yes_out = h->batches[batch_id]->dag != nullptr ? 1 : 0;
    return OISAT_OK;
}

// Factorization AND solve phase of every member as ONE task-graph launch (dense_dag.inc "The solve phase as tasks"): what
// oisat_batch_potrf + oisat_batch_solve do in 2 + 3 (refine + 2) launches with the solve phase exposed behind the
// factorization.  Same arithmetic per member.  Needs a batch whose factorization runs as a task graph (OISAT_ENOTSUP_DAG
// otherwise: the caller keeps the two calls).
extern "C" int oisat_batch_analyse(oisat_ctx* h, int batch_id, int dtype, double g, int refine, int* info_host) {
    ARG_CHECK(h && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    ChBatch& bt = *h->batches[batch_id];
    ARG_CHECK(bt.solve_dev != nullptr && bt.ord_total > 0 && refine >= 0 && refine <= DAG_MAX_REFINE && g >= 0.0);
    ARG_CHECK(dtype == OISAT_F32 || dtype == OISAT_F64);
    if (h->corr != OISAT_CORR_GAUSSIAN) {
        oisat_set_error("oisat_batch_analyse: the one-launch analysis is Gaussian only (oisat_set_correlation); use oisat_batch_potrf + oisat_batch_solve");
        return OISAT_EINVAL;
    }
    if (!bt.dag) {
        oisat_set_error("oisat_batch_analyse: this batch's factorization does not run as a task graph (oisat_set_task_graph / size)");
        return OISAT_EINVAL;
    }
    int* info_dev = nullptr;
    char* base = nullptr;
    if (int rc = status_ws(h, &info_dev, &base)) return rc;
    HIP_TRY(dense_kernel_attributes());
    const int nmem = (int)bt.table.size();
    const double g2 = corr_scale2_f64(OISAT_CORR_GAUSSIAN, g);  // (what oisat_apply_increment_batched hands its kernel)
    DagSolve sv{};
    sv.mem = bt.solve_dev;
    sv.g = g;
    sv.g2 = g2;
    sv.win_deg = lat_window_deg(OISAT_CORR_GAUSSIAN, g);
    sv.cut_chord = cut_chord_of(OISAT_CORR_GAUSSIAN, g);
    double far_chord;
    ARG_CHECK(far_chord_of(OISAT_CORR_GAUSSIAN, g, &far_chord));
    sv.far_chord = (float)far_chord;
    double far_chord_resid;                                 // the residual's: the same chord, or none (far_chord_of)
    ARG_CHECK(far_chord_of(OISAT_CORR_GAUSSIAN, g, &far_chord_resid, -1.0, false));
    sv.tol2 = h->refine_tol * h->refine_tol;
    sv.refine = refine;
    sv.dtype = dtype;
    sv.cells = increment_cells(h->cu_count, bt.max_n, nmem);
    sv.blocks = residual_blocks_pay(OISAT_CORR_GAUSSIAN, g) ? 1 : 0;
    for (const SolveMember& sm : bt.solve_host) sv.blocks = sv.blocks && sm.perm != nullptr;
    if (sv.blocks && far_chord_resid < 1e9) sv.blocks |= 2;
    sv.trsv_timeouts = (unsigned*)base;
    sv.nsys = nmem;
    if (!bt.dag_solve || bt.dag_solve_refine != refine || bt.dag_solve_cells != sv.cells) {
        HIP_TRY(hipStreamSynchronize(h->stream));            // (a plan is never freed under a running launch)
        oisat_dag_plan_release(bt.dag_solve);
        bt.dag_solve = nullptr;
        DagSolveShape shape;
        shape.refine = refine;
        for (const SolveMember& sm : bt.solve_host) {
            shape.nres.push_back((int)cdiv(sm.m, 64));
            shape.ninc.push_back((int)increment_blocks(sm.n, sm.nx, sv.cells));
        }
        bt.dag_solve = dag_plan_create(bt.table, h->stream, shape);
        if (!bt.dag_solve) return OISAT_ENOMEM;
        HIP_TRY(hipStreamSynchronize(h->stream));            // (the plan's words are zero before any stream can launch it)
        bt.dag_solve_refine = refine;
        bt.dag_solve_cells = sv.cells;
    }
    sv.queue = bt.dag_solve->queue_dev;
    sv.qcap = (int)bt.dag_solve->qcap;
    sv.qcap0 = (int)bt.dag_solve->qcap0;
    HIP_TRY(hipMemsetAsync(info_dev, 0, sizeof(int), h->stream));
    HIP_TRY(hipMemsetAsync(info_dev + 3, 0, sizeof(int), h->stream));
    if (int rc = pad_identity_batched(h, bt)) return rc;
    OISAT_LAUNCH(h, "copy_pad", solve_prep_batched_kernel, dim3((unsigned)stream_grid(bt.max_mp, 256) > 64u ? 64u : (unsigned)stream_grid(bt.max_mp, 256), (unsigned)nmem),
                 dim3(256), 0, (const SolveMember*)bt.solve_dev);
    if (int rc = dag_launch(h, *bt.dag_solve, info_dev, (unsigned*)(info_dev + kInfoDagTimeouts), &sv)) return rc;
    if (info_host) {
        int* pin = (int*)oisat_pinned(h, 64);
        if (!pin) return OISAT_ENOMEM;
        HIP_TRY(hipMemcpyAsync(pin, info_dev, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        info_host[0] = pin[0];
        info_host[1] = pin[0] ? bt.order[pin[3] - 1] : -1;          // the caller's matrix index
        if (pin[kInfoDagTimeouts] != 0) {
            HIP_TRY(hipMemsetAsync(info_dev + kInfoDagTimeouts, 0, sizeof(int), h->stream));
            oisat_set_error("batched analysis: the task-graph launch timed out (a workgroup gave up waiting): factors and fields are incomplete");
            return OISAT_EHIP;
        }
        if (pin[0] != 0) {
            HIP_TRY(hipMemsetAsync(info_dev + 1, 0, 2 * sizeof(int), h->stream));
            oisat_set_error("batched potrf: matrix %d not positive definite at column %d", info_host[1], pin[0]);
            return OISAT_ENOTPD;
        }
    }
    return OISAT_OK;
}

extern "C" int oisat_batch_potrf(oisat_ctx* h, int batch_id, int* info_host) {
    ARG_CHECK(h && batch_id >= 0 && batch_id < (int)h->batches.size() && h->batches[batch_id]);
    const ChBatch& bt = *h->batches[batch_id];
    int* info_dev = nullptr;
    if (int rc = status_ws(h, &info_dev, nullptr)) return rc;
    HIP_TRY(dense_kernel_attributes());
    HIP_TRY(hipMemsetAsync(info_dev, 0, sizeof(int), h->stream));
    HIP_TRY(hipMemsetAsync(info_dev + 3, 0, sizeof(int), h->stream));
    if (int rp = pad_identity_batched(h, bt)) return rp;
    int rc;
    if (bt.dag) {
        rc = dag_launch(h, *bt.dag, info_dev, (unsigned*)(info_dev + kInfoDagTimeouts));
    } else {
        rc = potrf_rec_batched(h, bt, 0, bt.max_mpb, info_dev);
    }
    if (rc) return rc;
    if (info_host) {
        int* pin = (int*)oisat_pinned(h, 64);
        if (!pin) return OISAT_ENOMEM;
        HIP_TRY(hipMemcpyAsync(pin, info_dev, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        info_host[0] = pin[0];
        info_host[1] = pin[0] ? bt.order[pin[3] - 1] : -1;          // the caller's matrix index
        if (pin[kInfoDagTimeouts] != 0) {
            HIP_TRY(hipMemsetAsync(info_dev + kInfoDagTimeouts, 0, sizeof(int), h->stream));
            oisat_set_error("batched potrf: the task-graph factorization timed out (a workgroup gave up waiting): the factors are incomplete");
            return OISAT_EHIP;
        }
        if (pin[0] != 0) {
            HIP_TRY(hipMemsetAsync(info_dev + 1, 0, 2 * sizeof(int), h->stream));
            oisat_set_error("batched potrf: matrix %d not positive definite at column %d", info_host[1], pin[0]);
            return OISAT_ENOTPD;
        }
    }
    return OISAT_OK;
}
