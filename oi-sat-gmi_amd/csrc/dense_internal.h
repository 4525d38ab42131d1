// Internal to the dense solver (the dense_*.hip units of liboisat_hip.so): what crosses a file is declared here, once, in
// namespace oisat_dense, so that the library exports no bare C++ names.  The run-time switches are in dense_switches.h; what
// dense_cov.hip offers dense_chol.hip is in oisat_common.h.
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
};

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
// far = first, no middle stretch (oisat_factor_mid) is mid = far.  Empty: a dense plan.
struct DagBands {
    std::vector<int> first, far, mid;
    DagBands() {}
    DagBands(int nb, const int* first_, const int* far_, const int* mid_)
        : first(first_, first_ + nb), far(far_ ? std::vector<int>(far_, far_ + nb) : first), mid(mid_ ? std::vector<int>(mid_, mid_ + nb) : far) {}
    bool operator==(const DagBands& o) const { return first == o.first && far == o.far && mid == o.mid; }
    // ... against a caller's raw tables of nb rows, normalised the same way, without building one
    bool equals(size_t nb, const int* first_, const int* far_, const int* mid_) const {
        far_ = far_ ? far_ : first_;
        mid_ = mid_ ? mid_ : far_;
        return first.size() == nb && std::equal(first.begin(), first.end(), first_) && std::equal(far.begin(), far.end(), far_) &&
               std::equal(mid.begin(), mid.end(), mid_);
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
// dense_tables.hip (host only): a caller's envelope table, and the far and middle tables it set for a factorization (empty:
// none), checked against each other
bool envelope_table_ok(const int32_t* first, int64_t nb);
bool far_table_ok(const std::vector<int32_t>& far, const int32_t* first, int64_t nb);
bool mid_table_ok(const std::vector<int32_t>& mid, const std::vector<int32_t>& far, const int32_t* first, int64_t nb);

}  // namespace oisat_dense
