// Internal to the dense solver (the dense_*.hip units of liboisat_hip.so): what crosses a file is declared here, once, in
// namespace oisat_dense, so that the library exports no bare C++ names.  Only host functions cross: a kernel is launched by the unit
// that holds it, and device code that two units need is a *.inc both take textually.  The run-time switches are in
// dense_switches.h; what dense_cov.hip offers dense_solve.hip is in oisat_common.h.
// The units: dense_gemm.hip (the four fp32 GEMMs), dense_dag.hip (the task-graph kernel of dense_dag.inc, the diagonal-block kernel
// and their launches; the only unit with test hooks), dense_chol.hip (leaf pairs and the factorization schedules), dense_solve.hip
// (sweeps, gain solve, status words, the oisat_batch_* API), dense_post.hip (posterior diagnostics, probes), dense_cov.hip, and the
// host-only dense_tables.hip and dense_dag_plan.hip.
#pragma once

#include "oisat_common.h"
#include "dense_switches.h"

#include <algorithm>

namespace oisat_dense __attribute__((visibility("hidden"))) {

// ---- the task-graph launch (dense_dag.inc: the kernel; dense_dag_plan.hip: its plan) -------------------------------------
// kinds of the tickets
constexpr int DAG_CHAIN = 0, DAG_TILE = 1, DAG_SUB = 2, DAG_PRE = 3;
// ... and, in the launch that also SOLVES (oisat_batch_analyse), the gain solve and the increment of every system as tasks too
// (dense_dag.inc, "The solve phase as tasks"): a row of a triangular sweep, a block of the float64 residual, a patch of the increment --
// (kind, system, index, round).  They are not in the ticket list: a task is put into the launch's READY QUEUE by the task
// that completes what it waits for.
constexpr int DAG_FWD = 5, DAG_BWD = 6, DAG_RES = 7, DAG_INC = 8;
constexpr int DAG_STATE_HDR = 64;                       // state[0] = diagdone; rowfin at [64 + r], pre at [64 + nb + j], sub at [64 + 2 nb + j]
// header words 1 .. of a system's state, solve phase (counters of finished tasks per refinement round r = 0 .. refine <= 8):
constexpr int DAG_ST_FWD = 2;                           // [2 + r]   rows of round r's forward sweep that are through
constexpr int DAG_ST_BWD = 11;                          // [11 + r]  ... backward sweep
constexpr int DAG_ST_RES = 20;                          // [20 + e]  blocks of residual evaluation e that are through
constexpr int DAG_ST_INC = 29;                          // [29 + g]  increment patches of generation g that are through, + DAG_INC_DECIDED once generation g is known to be the final one
constexpr int DAG_INC_DECIDED = 1 << 20;
constexpr int DAG_MAX_REFINE = 8;
constexpr unsigned kDagSpinMax = 1u << 24;              // >= 15 s of polling (the largest systems factor for seconds)
constexpr int DAG_CU_KEYS = 16 * 256;                   // (XCC id, SE / SH / CU id) -> words of the CU census

struct DagSys {                  // one system of a task-graph launch (device table)
    float* S;
    float* tinv;
    int64_t ld;
    int* state;                  // zero when a launch starts (zeroed at allocation, then by the last workgroup of every launch)
    int nb;                      // block rows
    int which;                   // index reported through info[3] (the batch table's index)
    const int* mid;              // int32[nb]: first block column of each block row that is not "middle" (DagPlan::mid_dev), or null: no middle stretch
    // The shadow (dense_dag.inc, "Shadow"): the bf16 images of every final strictly-lower tile inside the envelope, or null: none, the
    // far and middle stretches convert in their K-loops.  Tile (r, k) starts at shadow + (shrow[r] + k) * kShTile bytes.
    char* shadow;
    const int64_t* shrow;        // int64[nb]: rowoff[r] - first[r] (DagPlan::shrow_dev; rowoff: oisat_factor_shadow_layout)
    int shuse;                   // who READS it: 1 = the far stretch, 2 = the middle stretch (OISAT_FACTOR_SHADOW); the writers always store
    const int* near;             // int32[nb]: first block column of each block row that is not "near" (DagPlan::near_dev), or null: no near stretch
};
constexpr int64_t kShTile = 65536;                              // bytes of a shadow tile
constexpr int kShPlane = 32768, kShGroup = 4096;                // ... of a plane, of a 16-column group of a plane

struct DagCtl {                  // zero when a launch starts
    int ticket, error, gone, pad;
    int sys_done, pad2[3];                         // systems whose increment is complete
    struct { int head, tail, avail, pad; } q[2];   // the ready queues of the solve tasks (0: sweep rows, 1: residual blocks and increment patches):
                                                   // entries handed out | reserved | written and not yet claimed
    int cu_arrivals[DAG_CU_KEYS];        // workgroups that have started on each CU
    int cu_role[DAG_CU_KEYS];            // what the FIRST workgroup of a CU drew: 1 = bulk task, 2 = a chain that wants its CU alone
};

struct DagSolve {                // the solve phase of a launch (dense_dag.inc, "The solve phase as tasks")
    const SolveMember* mem;      // table order (the order of DagSys)
    unsigned long long* queue;   // [qcap][2]: (kind | system << 32), (index | round << 32); zero = not written yet
    double g, g2, win_deg, cut_chord, tol2;
    int refine, dtype, cells, blocks;       // blocks: residual on compact blocks of rows (every member has its permutation);
                                            // | 2: with the far tier at far_chord (off unless OISAT_SOLVE_FAR_BITS asks for it)
    int nsys, qcap, qcap0;                  // entries [0, qcap0) belong to queue 0 (sweep rows), [qcap0, qcap) to queue 1
    float far_chord;                        // far_chord_of() beside cut_chord: a float by construction, in what was padding (the
                                            // launches without solve tasks keep their argument block byte for byte)
    unsigned* trsv_timeouts;                // status slot 7
    // the launch that factors ONE system and runs its first forward sweep (DAG_SOLVE_FWD, oisat_potrf_env_fwd): the padded
    // right-hand side, the forward vector ("not yet published") and the factor's envelope first[nb] | last[nb] (or nullptr)
    double* fwd_rhs;
    double* fwd_sol;
    const int* env;
};

// ---- host: the plan of a task-graph launch ---------------------------------------------------------------------------
// The envelope an enveloped single-system plan was made for and its stretches, normalised: no far stretch (oisat_factor_far) is
// far = first, no middle stretch (oisat_factor_mid) is mid = far, no near stretch (oisat_factor_near) is near = mid.  Empty: a dense plan.
struct DagBands {
    std::vector<int> first, far, mid, near;
    DagBands() {}
    DagBands(int nb, const int* first_, const int* far_, const int* mid_, const int* near_)
        : first(first_, first_ + nb), far(far_ ? std::vector<int>(far_, far_ + nb) : first), mid(mid_ ? std::vector<int>(mid_, mid_ + nb) : far),
          near(near_ ? std::vector<int>(near_, near_ + nb) : mid) {}
    bool operator==(const DagBands& o) const { return first == o.first && far == o.far && mid == o.mid && near == o.near; }
    // ... against a caller's raw tables of nb rows, normalised the same way, without building one
    bool equals(size_t nb, const int* first_, const int* far_, const int* mid_, const int* near_) const {
        far_ = far_ ? far_ : first_;
        mid_ = mid_ ? mid_ : far_;
        near_ = near_ ? near_ : mid_;
        return first.size() == nb && std::equal(first.begin(), first.end(), first_) && std::equal(far.begin(), far.end(), far_) &&
               std::equal(mid.begin(), mid.end(), mid_) && std::equal(near.begin(), near.end(), near_);
    }
};

struct DagPlan {
    DagSys* sys_dev = nullptr;
    int4* tasks_dev = nullptr;
    int* state_dev = nullptr;
    DagCtl* ctl_dev = nullptr;
    int ntasks = 0, nsys = 0, state_words = 0, chain_rows = 0;
    int reserve_chains = 0;                                     // leading chain tickets that get a CU to themselves
    int max_wave_chains = 0;                                    // most chain tickets of ONE wave: each holds a workgroup until its system is through
    int solve_refine = -1;                                      // >= 0: the launch also solves (ready queue), at most that many refinement rounds
    bool fwd_only = false;                                      // ... only the first forward sweep of its one system (DAG_SOLVE_FWD)
    int64_t qcap = 0, qcap0 = 0;                                // entries of its ready queues (all | the sweep rows' share)
    unsigned long long* queue_dev = nullptr;
    std::vector<DagSys> sys_host;
    std::vector<int4> tasks_host;
    DagBands bands;                                             // what this plan's ticket list was made for
    int* mid_dev = nullptr;                                     // the device copy of bands.mid (an enveloped plan's int32[nb]); DagSys::mid points here while a stretch exists
    int* near_dev = nullptr;                                    // likewise bands.near; DagSys::near points here while a row has a near block
    std::vector<int64_t> shrow;                                 // the shadow's row table of `first`: rowoff[r] - first[r] (dag_shadow_layout), and its device copy
    int64_t* shrow_dev = nullptr;
    int64_t sh_tiles = 0;                                       // tiles of that shadow: sum of r - first[r]
    size_t tasks_cap = 0;                                       // tickets tasks_dev holds (an enveloped plan: the dense list's, so a new envelope refills it)
    long long* trace_dev = nullptr;                             // OISAT_DAG_TRACE: [ntasks][4] + [chain_rows][8] stamps of the last launch
};

// the ticket list of a launch over systems of nb_of[s] block rows (table order: largest first) -- host only, no device call:
// oisat_dag_task_order hands it to tests
struct DagOrder {
    std::vector<int4> tasks;
    int chain_rows = 0, reserve_chains = 0, max_wave_chains = 0;
};
// entries the ready queue of a solving launch needs: every solve task of every system, every round taken
struct DagSolveShape {                                          // refine < 0: a factorization-only launch
    int refine = -1;
    std::vector<int> nres, ninc;                                // per system: residual blocks (m / 64), increment patches
    bool fwd_only = false;                                      // DAG_SOLVE_FWD: the rows of the first forward sweep and nothing else (refine = 0)
};

// A launch drains only if, next to the chains that can be resident at one time, workgroups are left to draw the bulk tasks
// those chains wait for: chains <= a quarter of the resident workgroups.
static inline bool dag_fits(int max_wave_chains, int slots) { return 4 * max_wave_chains <= slots; }
static inline int dag_slots(const oisat_ctx* h) { return 2 * (h->cu_count > 0 ? h->cu_count : 256); }

// Which factorizations run as a task graph: every system / batch of at least three block rows (below that there is nothing to
// overlap), unless the handle says otherwise (oisat_set_task_graph) or the environment does (OISAT_DAG=0 | 1: the parity tests
// compare the two schedules inside one process, so it is read at every call).  Measured against the recursion
// (factorization alone, TFLOP/s): 10,000 observations 91.9 vs 53.9, 20,000: 126 vs 94, 30,000: 135 vs 115, 50,000: 138 vs
// 128, 100,000: 140.8 vs 137.4 -- the task graph wins at every size.  A batch of more than 1024 systems keeps the lock-step
// recursion, and so does any launch whose chains would not leave room for the tasks they wait for (dag_fits).
static inline bool dag_wanted(const oisat_ctx* h, int64_t max_blocks, int nsys) {
    const int mode = h->dag_mode >= 0 ? h->dag_mode : dag_env_mode();
    if (mode == 0 || nsys > 1024) return false;
    return max_blocks >= (mode == 1 ? 2 : 3);
}

constexpr double kDagEnvLeadFar = 0.3;                          // the ticket lead of a list with a far stretch (dag_task_order, dense_dag_plan.hip)
constexpr int kDagEnvMaxBlocks = 1024;                          // an enveloped ticket has ten bits for a block column (dag_task_order)

// dense_dag_plan.hip
void dag_plan_free(DagPlan* p);
void dag_task_order(const std::vector<int>& nb_of, int wave_arg, DagOrder& out, const int* first = nullptr, const int* far = nullptr,
                    double lead_far = kDagEnvLeadFar);
int64_t dag_shadow_layout(const int* first, int64_t nb, int64_t* rowoff);
hipError_t dag_plan_shadow(DagPlan& p, char* shadow, int use, hipStream_t stream);
DagPlan* dag_plan_create(const std::vector<BatchMat>& table, hipStream_t stream, const DagSolveShape& shape = DagSolveShape(),
                         const DagBands& bands_arg = DagBands());
int dag_plan_refill(DagPlan& p, const DagBands& bands, hipStream_t stream);
// dense_tables.hip (host only): a caller's envelope table, and the far, middle and near tables it set for a factorization (empty:
// none), checked against each other
bool envelope_table_ok(const int32_t* first, int64_t nb);
bool far_table_ok(const std::vector<int32_t>& far, const int32_t* first, int64_t nb);
bool mid_table_ok(const std::vector<int32_t>& mid, const std::vector<int32_t>& far, const int32_t* first, int64_t nb);
bool near_table_ok(const std::vector<int32_t>& near, const std::vector<int32_t>& mid, const std::vector<int32_t>& far, const int32_t* first,
                   int64_t nb);

// ---- the recursion's tree, the GEMM launches, the status words -----------------------------------------------------------
// One launch of a batched GEMM kernel (dense_gemm.hip: batch_operands derives a member's operands from its table entry and the node)
struct BatchArgs {
    const BatchMat* mats;        // nullptr: not a batched launch
    int kind;                    // 0: trailing update of node (b0, mid, b1);  1: TRSM of the panel below diagonal block b0
    int b0, mid, b1;
    const int* cum = nullptr;    // persistent kernel: prefix sums of the members' tile counts at this node (cum[cnt] = total):
    int cnt = 0, total = 0;      // virtual ids 0 .. total-1 are exactly the real tiles, member = the w with cum[w] <= id < cum[w+1]
    int prio = 0;                // wave priority of this group's kernels (oisat_set_share): where the waves of two groups share a
};                               // SIMD the arbiter serves the higher one first -- the group with the longest dependent chain

// Leaves of the recursion are PAIRS of block columns (pair_mid_kernel / pair_panel_kernel) where the leaf-level launches
// are bound by HBM traffic, i.e. in lock-step batches of many systems (>= OISAT_LEAF_PAIRS_MIN members, default 8; 0 = never):
// a month's 48 tiles factor in 23.6 ms instead of 25.6.  For one system or a couple of polar caps the same launches are
// latency-bound and the extra one-workgroup step between the two diagonal blocks costs more than the saved pass
// (10,000 observations: 8.6 ms per analysis against 8.0), so those keep single-block leaves.
static const int kLeafPairsMin = 8;                     // lock-step batches of at least this many systems take leaf PAIRS (fewer: 8.6 vs 8.0 ms at 1e4 observations)
static const bool kSinglePairs = false;                  // (single systems keep single-block leaves)
// split point of the node [b0, b1): the left part gets ceil(half), rounded up to an even number of blocks when leaves are
// pairs (so that the tree ends in pairs wherever it can); the one rule of potrf_rec, potrf_rec_batched and the tile tables
static inline int64_t split_mid(int64_t b0, int64_t b1, bool pairs) {
    const int64_t n = b1 - b0;
    int64_t left = (n + 1) / 2;
    if (pairs && n > 2 && (left & 1)) ++left;
    if (left >= n) left = n - 1;
    return b0 + left;
}

constexpr int kInfoUnconverged = 4, kInfoUnconvergedMember = 5, kInfoDagTimeouts = 6;     // status words (status_ws, dense_solve.hip)

// dense_gemm.hip
int launch_gemm(oisat_ctx* h, const char* name, float* C, int64_t ldc, const float* A, int64_t lda, const float* B, int64_t ldb,
                int64_t M, int64_t N, int K, int mode, int lower);
int launch_gemm_batched(oisat_ctx* h, const char* name, const ChBatch& bt, BatchArgs ba, int K, int mode, int lower);
void build_cum_tables(ChBatch* bt, std::vector<int>& host);
// dense_dag.hip: the task-graph launch, and the diagonal-block kernel for the other schedules (nsys workgroups: one system, or the
// first nsys of the table `mats`)
int dag_launch(oisat_ctx* h, DagPlan& p, int* info_dev, unsigned* dag_timeouts, const DagSolve* solve = nullptr);
int launch_potrf_diag(oisat_ctx* h, unsigned nsys, float* S, int64_t ld, int64_t k0, float* tinv, int* info_dev, int block_index,
                      const BatchMat* mats, int prio);
// dense_chol.hip, for the batch API
int potrf_rec_batched(oisat_ctx* h, const ChBatch& bt, int b0, int b1, int* info_dev);
int pad_identity_batched(oisat_ctx* h, const ChBatch& bt);
// dense_solve.hip: the handle's status words and solve state, the sweep kernels' attributes, the "copy_pad" launch in front of a solve
int status_ws(oisat_ctx* h, int** info_dev, char** trsv_base);
SolveState* solve_state(oisat_ctx* h);
hipError_t dense_kernel_attributes();
int solve_prep(oisat_ctx* h, const double* src, int64_t m, int64_t mp, double* rhs, double* fwd, SolveState* st);

}  // namespace oisat_dense
