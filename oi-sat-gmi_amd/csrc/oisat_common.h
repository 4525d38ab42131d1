// Internal to liboisat_hip.so -- not installed.  gfx950 only; 64-wide wavefronts are assumed.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/oisat.h"

constexpr int kWave = 64;

void oisat_set_error(const char* fmt, ...);

struct ProfRec {
    char name[64];
    double total_ms = 0.0;
    int64_t launches = 0;
};

struct ProfPending {
    int rec;
    hipEvent_t a, b;
};

namespace oisat_dense {
struct DagPlan;                  // a task-graph plan (dense_internal.h), opaque outside the dense_*.hip units
}

struct ChFactor {                // what the triangular solves need besides L: the inverted diagonal blocks
    const float* S = nullptr;
    int64_t m = 0, mp = 0, ld = 0;
    float* tinv = nullptr;       // [mp/128][128][128]: inverted diagonal blocks, row-major
    const int* env = nullptr;    // device, first[mp/128] | last[mp/128]: the factor's block envelope (oisat_potrf_env), or nullptr = dense
    int band = 0;                // enveloped: max over b of (b - first[b]) + 1 block rows, from the host table; 0 = dense / adopted
                                 // (the sweeps' launch rule, oisat_trsv_plan)
    std::vector<int32_t> first;  // enveloped: host copy of first[mp/128] (oisat_trsm_rows_bwd sizes its launches with it); empty = dense
    // oisat_potrf_env_fwd: the right-hand side whose forward vector the factorization launch left in workspace 5 (with the
    // right-hand side re-armed and the solve state reset), or nullptr.  oisat_gain_solve of the same d takes it, once.
    const double* fwd_d = nullptr;
};

struct BatchMat {                // one matrix of a batched factorization (device table entry)
    float* S;
    float* tinv;                 // [mpb][128][128]
    int64_t ld;
    int64_t m;
    int mpb;                     // roundup(m, 128) / 128
    int pad;
};

// state of one gain solve on the device: squared norms for the convergence test and the flag that turns the remaining
// refinement launches into no-ops (workspace slot 9 of a handle, or one 256-byte block per member of a batched solve)
struct SolveState {
    double dd;                   // |d|^2
    double norm[12];             // |r_k|^2, k = 0 .. refine
    int conv;                    // set when |r_k| <= tol |d|: every later residual / sweep launch of this solve returns at once
    int computed;                // number of residual norms stored
};

struct SolveMember {             // one system of a batched solve phase (device table, oisat_batch_set_solve)
    const float* S;              // its factor (after oisat_batch_potrf) and inverted diagonal blocks
    const float* tinv;
    int64_t ld, m;
    int mpb, nx;                 // block rows; width of the system's (ny x nx, row-major) cell grid, 0 = unknown (oisat_batch_set_grid)
    const double *oxyz, *osig, *ovar, *d, *olat;       // observations (ascending latitude), innovation
    double *z, *rhs, *fwd;       // solution; padded right-hand side and forward solution [mpb * 128] each
    SolveState* st;
    const double *gxyz, *gsig, *glat;                   // the system's grid cells
    int64_t n;
    const void* xb;              // background, analysis, increment (dtype of the batch)
    void* xa;
    void* inc;
    const int* perm;             // its observations along a space-filling curve (compact residual blocks) or nullptr
    int which;                   // the caller's index of this member (oisat_batch_set_solve order), reported by the status words
};

struct ChBatch {                 // matrices factored in lock-step by oisat_batch_potrf (sorted by block count, largest first)
    BatchMat* table_dev = nullptr;
    // compact tile enumeration of the persistent GEMM launches: for every node of the recursion tree the prefix sums of
    // the members' tile counts (cum[0] = 0 .. cum[cnt] = total), built once by oisat_batch_create
    int* cum_dev = nullptr;
    std::vector<int> cum_off, cum_cnt, cum_total;      // per node slot (see ChBatch::slot)
    std::vector<long long> cum_key;                     // node key -> slot (sorted, binary search)
    std::vector<BatchMat> table;
    std::vector<int> order;      // table[i] is the caller's matrix order[i]
    int max_mpb = 0;
    // batched solve phase (oisat_batch_set_solve): member table in the order of `table`, the sweep's ticket -> (member, step)
    // list (steps ascending, so that a row only waits for lower tickets) and two control blocks (forward | backward)
    SolveMember* solve_dev = nullptr;
    std::vector<SolveMember> solve_host;
    int64_t max_patches = 0;
    int* ord_dev = nullptr;
    void* ctl_dev = nullptr;
    int ord_total = 0;
    int64_t max_m = 0, max_n = 0, max_mp = 0;
    bool pairs = false;          // leaves of its recursion are pairs of block columns (many members: the leaf launches are HBM-bound)
    oisat_dense::DagPlan* dag = nullptr;         // task-graph plan of the batch, owned
    oisat_dense::DagPlan* dag_solve = nullptr;   // ... of the batch's factorization + solve phase in one launch (oisat_batch_analyse), made on first use
    int dag_solve_refine = -1, dag_solve_cells = 0;             // what that plan was made for
};

struct DagSingle {               // a cached single-system task-graph plan (oisat_potrf)
    oisat_dense::DagPlan* plan = nullptr;
    const float* S = nullptr;
    const float* tinv = nullptr;
    int64_t ld = 0, mpb = 0;
    bool enveloped = false;      // its ticket list follows an envelope (the plan keeps the table it was made for)
    bool fwd = false;            // its launch also runs the first forward sweep (a ready queue of mpb rows)
    uint64_t stamp = 0;
};

struct oisat_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int cu_count = 0;
    size_t hbm_bytes = 0;
    char name[128] = {0};
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<ProfPending> pending;
    std::vector<hipEvent_t> free_events;
    // grow-only device workspaces (never freed/reallocated inside a timed region once warm)
    void* ws[15] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t ws_bytes[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // last scaling sweep uploaded into workspace slot 0 (oi_diag.hip)
    double scales_host[OISAT_MAX_SCALES] = {0};
    int scales_n = 0;
    const void* scales_dev = nullptr;
    // the factor left by the last oisat_potrf on this handle (dense_chol.hip; its readers: dense_solve.hip, dense_post.hip)
    ChFactor factor;
    bool small_tiles = true;            // gemm_nt: 64x64 tiles for launches of <= 700 128x128 tiles (latency-bound ones)
    double refine_tol = 1e-6;           // oisat_set_refine_tol: relative residual at which the gain solve stops refining
    int corr = 0;                       // oisat_set_correlation: the correlation model of every later call (OISAT_CORR_*)
    int wave_prio = 0;                  // oisat_set_share: s_setprio of this handle's batched factorization kernels (0..3)
    int gemm_wg_per_cu = 0;             // oisat_set_share: workgroups per CU of its persistent GEMM launches (0 = default, 2)
    hipStream_t own_stream = nullptr;   // created by oisat_stream_create, destroyed at shutdown
    hipStream_t aux_stream = nullptr;   // look-ahead Cholesky: trailing updates run here, the panel chain on `stream`
    std::vector<hipEvent_t> sync_events;
    // oisat_gain_solve_fields: the increment of the first solve runs here underneath the correction's sweeps (lowest priority,
    // created on first use); fork = z0 and its snapshot are out (main), join = the scratch field is written (side)
    hipStream_t inc_stream = nullptr;
    hipEvent_t inc_fork = nullptr, inc_join = nullptr;
    bool inc_in_flight = false;         // ... a side launch is in flight: the sweeps launched meanwhile leave it CUs (trsv_launch_shape)
    void* comm = nullptr;               // RCCL communicator (oisat_comm_init), opaque here
    int comm_rank = 0, comm_size = 1;
    hipEvent_t signal_event = nullptr;  // oisat_wait_for: recorded on this handle's stream, waited on by another handle's
    std::vector<ChBatch*> batches;      // oisat_batch_create
    // task-graph plans of the last single-system factorizations on this handle (dense_dag_plan.hip), keyed by what a plan depends on
    const int* obs_perm = nullptr;      // oisat_set_obs_blocks: space-filling order of the observations of the next gain solves
    int64_t obs_perm_m = 0;
    std::vector<int32_t> factor_far;    // oisat_set_factor_far: the far stretch of the NEXT enveloped factorization (one-shot)
    std::vector<int32_t> factor_mid;    // oisat_set_factor_mid: ... and its middle stretch (one-shot)
    std::vector<int32_t> factor_near;   // oisat_set_factor_near: ... and its near stretch (one-shot)
    // the factor's shadow (dense_dag.inc "Shadow": bf16 images of the final tiles, workspace slot 10)
    int64_t shadow_cap = -1;            // oisat_set_factor_shadow_cap: most bytes it may take, -1 = no limit
    const char* shadow_last = nullptr;  // the shadow the last factorization on this handle filled (nullptr: it had none) ...
    std::vector<int32_t> shadow_first;  // ... its envelope ...
    std::vector<int64_t> shadow_shrow;  // ... and its row table, rowoff[r] - first[r] (oisat_factor_shadow_tile)
    int dag_mode = -1;                  // oisat_set_task_graph: -1 = by size (and OISAT_DAG), 0 = recursion only, 1 = task graph wherever it applies
    DagSingle dag_cache[8];
    uint64_t dag_clock = 0;
    // pinned host scratch for small synchronous read-backs
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    hipStream_t xfer_streams[4] = {nullptr, nullptr, nullptr, nullptr};   // oisat_d2h: slices of a large read-back, one host thread each
};

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            oisat_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return OISAT_EHIP;                                                                 \
        }                                                                                      \
    } while (0)

#define ARG_CHECK(cond)                                                                        \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            oisat_set_error("invalid argument: %s (%s:%d)", #cond, __FILE__, __LINE__);        \
            return OISAT_EINVAL;                                                               \
        }                                                                                      \
    } while (0)

// workspace slot `slot` of at least `bytes` (grow-only); returns nullptr + error on failure
void* oisat_ws(oisat_ctx* h, int slot, size_t bytes);
void* oisat_pinned(oisat_ctx* h, size_t bytes);
void oisat_dag_plan_release(void* plan);                // dense_dag_plan.hip: frees a task-graph plan (nullptr allowed; void*: oisat_core.hip calls it too)
// dense_cov.hip, for dense_solve.hip: the residual and increment forms of the gain solve and of the batch API
const int* oisat_take_obs_perm(oisat_ctx* h, int64_t m);
int oisat_cov_residual_if(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                          const double* d, const double* z, double* r_out, const double* olat_sorted, const int* converged_dev,
                          const int* perm);
int oisat_cov_residual_update_if(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                                 const double* r_prev, const double* dz, double* out, const double* olat_sorted, const int* converged_dev,
                                 const int* perm);
bool oisat_resid_update_applies(const oisat_ctx* h, double g, const double* olat_sorted, const int* perm);
double oisat_resid_update_c();
int oisat_cov_residual_batched(oisat_ctx* h, const SolveMember* mem_dev, const std::vector<SolveMember>& mem_host, int64_t max_m, double g);
int oisat_apply_increment_batched(oisat_ctx* h, int dtype, const SolveMember* mem_dev, const std::vector<SolveMember>& mem_host, int64_t max_n,
                                  double g);
// ... and the launches of oisat_gain_solve_fields behind its sweeps: the float64 increment of z0 into a double scratch field, and
// the update of it (guarded by st; the float64 increment of the final z where the guard fails)
int oisat_increment_scratch(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                            const double* osig, const double* z0, int64_t m, double g, double* inc0, const double* glat,
                            const double* olat_sorted);
int oisat_increment_update_if(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                              const double* osig, const double* z, const double* z0, int64_t m, double g, const void* xb, void* xa,
                              void* inc, const double* inc0, const double* glat, const double* olat_sorted, const SolveState* st, double t);
double oisat_inc_update_t();

int oisat_prof_begin(oisat_ctx* h, const char* name);   // returns pending index or -1
void oisat_prof_end(oisat_ctx* h, int pending);

// Launch with optional per-kernel event timing on the handle's stream, then check the launch.
#define OISAT_LAUNCH(h, NAME, kernel, grid, block, shmem, ...)                                 \
    do {                                                                                       \
        int _p = (h)->prof ? oisat_prof_begin((h), NAME) : -1;                                 \
        hipLaunchKernelGGL(kernel, grid, block, shmem, (h)->stream, __VA_ARGS__);              \
        if (_p >= 0) oisat_prof_end((h), _p);                                                  \
        hipError_t _le = hipGetLastError();                                                    \
        if (_le != hipSuccess) {                                                               \
            oisat_set_error("launch of %s failed: %s", NAME, hipGetErrorString(_le));          \
            return OISAT_EHIP;                                                                 \
        }                                                                                      \
    } while (0)

// launch KERNEL<KIND, ...> for the handle's correlation model (h->corr, oisat_set_correlation): one instantiation per model,
// no test of the model inside a kernel
#define OISAT_LAUNCH_CORR(h, NAME, KERNEL, TARGS, grid, block, shmem, ...)                                         \
    do {                                                                                                           \
        if ((h)->corr == OISAT_CORR_GASPARI_COHN) {                                                                \
            OISAT_LAUNCH(h, NAME, (KERNEL<OISAT_CORR_GASPARI_COHN, TARGS>), grid, block, shmem, __VA_ARGS__);      \
        } else if ((h)->corr == OISAT_CORR_SOAR) {                                                                 \
            OISAT_LAUNCH(h, NAME, (KERNEL<OISAT_CORR_SOAR, TARGS>), grid, block, shmem, __VA_ARGS__);              \
        } else {                                                                                                   \
            OISAT_LAUNCH(h, NAME, (KERNEL<OISAT_CORR_GAUSSIAN, TARGS>), grid, block, shmem, __VA_ARGS__);          \
        }                                                                                                          \
    } while (0)
#define OISAT_TARGS(...) __VA_ARGS__

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// memory-bound grid sizing: enough blocks to fill 256 CUs x 8, grid-stride the rest
static inline int stream_grid(int64_t work_items, int per_block) {
    int64_t g = cdiv(work_items, per_block);
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return (int)g;
}

template <typename T>
__device__ __forceinline__ T nan_of();
template <>
__device__ __forceinline__ float nan_of<float>() { return __builtin_nanf(""); }
template <>
__device__ __forceinline__ double nan_of<double>() { return __builtin_nan(""); }
