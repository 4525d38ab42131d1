// The dense solver: the plan of a task-graph launch -- host code only, no kernel.  The ticket order of a launch
// (dag_task_order: waves of systems, column-major lists, the enveloped system's lead), the plan that owns the launch's device
// buffers (dag_plan_create / _refill / _shadow / _free; DagPlan itself: dense_internal.h), and the two queries that hand the
// order to the tests (oisat_dag_task_order, oisat_dag_task_order_env).  The kernel that draws the tickets: dense_dag.inc.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"

constexpr int kDagWave = 8;                                     // systems per wave of small systems (12, 16, 24 and 48 measure the same to 0.2 ms of a month's 48.7)
constexpr double kDagEnvLead = 0.15;                            // enveloped systems: columns a task is drawn early per block of its K-loop (below)
// kDagEnvLeadFar = 0.3 (dense_internal.h): ... where part of the K-loops is a far stretch on the bf16 pipe (below).
// (0.3: the minimum of a sweep 0.15 .. 0.5 that ran on the 4 | 3 ring, whose far / middle K-blocks are cheaper than those of the 2 | 1 ring
// that ships; on 2 | 1 only 0.2 against 0.3 is measured: 67.5 - 67.7 -> 66.2 - 66.4 ms.  profiles/EXPERIMENTS.md, "A ring of four stages":
// the sweep is still to be repeated on 2 | 1.)
constexpr int kDagWave0Max = 64;                                // wave 0 holds at most this many chains
static inline void dag_queue_entries(const std::vector<int>& nb_of, const DagSolveShape& sh, int64_t* sweep_rows, int64_t* valu_tasks) {
    *sweep_rows = *valu_tasks = 0;
    for (size_t s = 0; s < nb_of.size(); ++s) {
        if (sh.fwd_only) {
            *sweep_rows += nb_of[s];
            continue;
        }
        *sweep_rows += (int64_t)(sh.refine + 1) * 2 * nb_of[s];
        *valu_tasks += (int64_t)(sh.refine + 1) * ((sh.refine > 0 ? sh.nres[s] : 0) + sh.ninc[s]);
    }
}

// What changes in DagSys[0] of a single-system plan after its creation -- the middle table's pointer, this call's shadow (null:
// none), its row table and its readers (DagSys::shuse) --, uploaded on `stream` when the host copy differs.  wait: launches that
// read the system's words as they are may be in flight, and a change waits for them.
static hipError_t dag_plan_sys0(DagPlan& p, const int* mid, const int* near, char* shadow, const int64_t* shrow, int shuse, bool wait,
                                hipStream_t stream) {
    DagSys& sy = p.sys_host[0];
    if (sy.mid == mid && sy.near == near && sy.shadow == shadow && sy.shrow == shrow && sy.shuse == shuse) return hipSuccess;
    if (wait)
        if (hipError_t e = hipStreamSynchronize(stream)) return e;
    sy.mid = mid;
    sy.near = near;
    sy.shadow = shadow;
    sy.shrow = shrow;
    sy.shuse = shuse;
    return hipMemcpyAsync(p.sys_dev, p.sys_host.data(), sizeof(DagSys), hipMemcpyHostToDevice, stream);
}

// An order and the tables it was made for into the plan (the ticket list's upload is the caller's) and, on `stream`, an enveloped
// plan's tables into its device buffers: the middle table, and the system's pointer to it -- null while no row has a middle block (the ticket ORDER does not depend
// on it) --; the shadow's row table of `first`, rowoff[r] - first[r] (whether a launch HAS a shadow is decided per call).  The
// plan's host vectors are the sources of the copies, so the caller has synchronised with whatever copy of them was in flight.
static hipError_t dag_plan_install(DagPlan& p, DagOrder& order, const DagBands& bands, hipStream_t stream) {
    p.tasks_host.swap(order.tasks);
    p.ntasks = (int)p.tasks_host.size();
    p.bands = bands;
    p.max_wave_chains = order.max_wave_chains;
    p.chain_rows = order.chain_rows;
    p.reserve_chains = order.reserve_chains;
    const size_t nb = bands.first.size();
    if (nb == 0) return hipSuccess;
    bool any = false;
    for (size_t i = 0; i < nb; ++i) any = any || bands.mid[i] > bands.far[i];
    if (any)
        if (hipError_t e = hipMemcpyAsync(p.mid_dev, p.bands.mid.data(), sizeof(int) * nb, hipMemcpyHostToDevice, stream)) return e;
    bool any_near = false;                                      // ... and the near table and its pointer, by the same rule
    for (size_t i = 0; i < nb; ++i) any_near = any_near || bands.near[i] > bands.mid[i];
    if (any_near)
        if (hipError_t e = hipMemcpyAsync(p.near_dev, p.bands.near.data(), sizeof(int) * nb, hipMemcpyHostToDevice, stream)) return e;
    const DagSys& sy = p.sys_host[0];
    if (hipError_t e = dag_plan_sys0(p, any ? p.mid_dev : nullptr, any_near ? p.near_dev : nullptr, sy.shadow, sy.shrow, sy.shuse, false, stream))
        return e;
    p.shrow.resize(nb);
    p.sh_tiles = dag_shadow_layout(p.bands.first.data(), (int64_t)nb, p.shrow.data());
    for (size_t r = 0; r < nb; ++r) p.shrow[r] -= p.bands.first[r];
    return hipMemcpyAsync(p.shrow_dev, p.shrow.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, stream);
}

}  // namespace

namespace oisat_dense {

void dag_plan_free(DagPlan* p) {
    if (!p) return;
    if (p->sys_dev) (void)hipFree(p->sys_dev);
    if (p->tasks_dev) (void)hipFree(p->tasks_dev);
    if (p->state_dev) (void)hipFree(p->state_dev);
    if (p->ctl_dev) (void)hipFree(p->ctl_dev);
    if (p->queue_dev) (void)hipFree(p->queue_dev);
    if (p->mid_dev) (void)hipFree(p->mid_dev);
    if (p->near_dev) (void)hipFree(p->near_dev);
    if (p->shrow_dev) (void)hipFree(p->shrow_dev);
    if (p->trace_dev) (void)hipFree(p->trace_dev);
    delete p;
}

// Envelope (first != nullptr: ONE system whose rows are in an order that makes it a band, first[i] = first block column of
// block row i that can be non-zero, non-decreasing, first[i] <= max(i - 1, 0)).  A Cholesky factor has no fill left of its
// matrix's envelope, so T(i, j) exists only for first[i] <= j and every K-loop of row i starts at k0 = first[i] (>= first[j]
// of the other operand row, j < i), which rides in the ticket's first word (kind | k0 << 8).  rowfin[i] keeps its meaning:
// the row's first task publishes first[i] + 1 and every wait is for rowfin >= k + 1 with k >= k0.  PRE(j) and SUB(j) are
// always emitted (the sub-diagonal tile is inside every envelope), so the chain is unchanged; the order -- column-major with the
// deep tasks drawn early, "Enveloped" below -- stays topological.
// Far stretch (far != nullptr, with first: far[i] = first block column of block row i that is NOT far, first[i] <= far[i] <= i,
// oisat_factor_far).  A bulk task's first word carries kfar = far[i] clamped into [k0, kend] next to k0: kind | k0 << 8 |
// kfar << 18, ten bits each (kDagEnvMaxBlocks block rows); its K-blocks k0 .. kfar - 1 run on the bf16 pipe (dag_tile_task).
// All three bulk kinds; the chain's own panel product and rank-128 update stay fp32.  The dense list and far == nullptr emit
// kfar = k0: an empty stretch.
// Middle stretch (oisat_factor_mid: mid[i] = first block column of block row i that is NOT middle, far[i] <= mid[i] <= i): the
// K-blocks kfar .. kmid - 1 of a bulk task run as split bf16 products (dag_seg_bf16x2).  Ten more bits do not fit the ticket's
// first word, and the words stay what they are: the table itself goes to the device (DagPlan::mid_dev, uploaded with the ticket
// list by dag_plan_install) and a task clamps kmid = mid[i] into [kfar, kend] with one scalar load.  The ticket ORDER does not
// depend on it.
// Near stretch (oisat_factor_near: near[i] = first block column of block row i that is NOT near, mid[i] <= near[i] <= i): the
// K-blocks kmid .. knear - 1 run as three-way split bf16 products from the fp32 tiles (dag_seg_bf16x3), the rest in fp32.  The
// middle table's path throughout: DagPlan::near_dev, one scalar load per task, knear = near[i] clamped into [kmid, kend]; the
// ticket words and their order do not know about it.
// (kDagEnvMaxBlocks = 1024 and kDagEnvLeadFar: dense_internal.h)
// lead_far: kDagEnvLeadFar for every launch; the query oisat_dag_task_order_env alone may be given another (its comment).
void dag_task_order(const std::vector<int>& nb_of, int wave_arg, DagOrder& out, const int* first, const int* far, double lead_far) {
    const int nsys = (int)nb_of.size();
    // Ticket order.  Systems are taken in WAVES.  The BIG systems -- those with at least half the block rows of the largest
    // (a month's polar caps; at most 64) -- go two at a time, the others (table order, largest first) eight at a time.  A
    // wave's tickets: its chains (a workgroup per system), then the column-major lists of its systems (PRE(j), SUB(j),
    // T(j+2.., j)) merged by the fraction j / nb of each system's columns -- the systems of a wave advance together, the next
    // wave's tasks are drawn as the slots free up.  Few systems in flight means many tasks per system in flight (512 slots /
    // 8 systems instead of / 50: the chain of a system is then rarely what its tasks wait for), operand panels shared in L2,
    // and only a wave's chains holding slots -- all 50 systems of a month interleaved: 108 TFLOP/s, in waves: 115.
    // Where the big ones go (round 4).  A pair opens the launch -- its abundant tile tasks fill the chip while nothing is
    // factored yet, and its solve, a latency chain of 3 x 137 sweep hops of ~10 us, is hidden under the small waves that
    // follow -- and the other pairs are spread evenly through the small waves (twelve months in one launch: pair, six waves,
    // pair, six waves, ...).  Why spread: a solve task is VALU / HBM work that runs beside a tile task on the other slot of its
    // CU, and a tile task beside such a partner is 1.5 x faster than beside another tile task (traced: 10.6 vs 16.2 us per
    // 128-deep K-block) -- but solve work only exists once systems are factored.  With all 24 polar caps of twelve months
    // first, the first 350 ms had no partner work and the rest was bound by it.  Measured and rejected for one month: the
    // caps in the middle (72 ms: the tickets are drawn in order, so the small waves behind the caps start when the caps'
    // tickets are gone and the caps' solve ends up exposed, 14 ms) and last (69 ms: exposed 9 ms); first: 62-63 ms.
    // Without small systems the big ones are one wave, as before.
    // Topological for the whole graph: a task's inputs come from its own system's lower columns and from its chain, whose
    // ticket precedes the system's first task.  (The solve tasks of oisat_batch_analyse are not tickets: ready queue.)
    const int wave = wave_arg > 0 ? wave_arg : kDagWave;
    int nbig = 0;
    while (nbig < nsys && nbig < kDagWave0Max && 2 * nb_of[nbig] >= nb_of[0]) ++nbig;
    std::vector<std::pair<int, int>> waves;                     // [first, last) system of each wave, in launch order
    if (nbig == nsys) {
        waves.push_back({0, nsys});
    } else {
        std::vector<std::pair<int, int>> small_waves, big_pairs;
        for (int w0 = nbig; w0 < nsys; w0 += wave) small_waves.push_back({w0, w0 + wave < nsys ? w0 + wave : nsys});
        for (int b0 = 0; b0 < nbig; b0 += 2) big_pairs.push_back({b0, b0 + 2 < nbig ? b0 + 2 : nbig});
        const int k = (int)small_waves.size(), G = (int)big_pairs.size();
        int g = 0;
        for (int w = 0; w <= k; ++w) {
            // pair g goes in front of small wave round(g k / G): the first pair opens the launch
            while (g < G) {
                int at = (int)((double)g * (double)k / (double)G + 0.5);
                if (at != w) break;
                waves.push_back(big_pairs[g++]);
            }
            if (w < k) waves.push_back(small_waves[w]);
        }
    }
    std::vector<int4>& tasks = out.tasks;
    tasks.clear();
    bool any_far = false;
    for (int i = 0; first && far && i < nb_of[0]; ++i) any_far = any_far || far[i] > first[i];
    const double env_lead = any_far ? lead_far : kDagEnvLead;
    int chain_rows = 0;                                         // (.z of a chain task: first row of its stamps in the trace)
    int max_wave_chains = 0, second = 0;
    struct Item { double key; int4 task; };
    std::vector<Item> items;
    for (const std::pair<int, int>& wv : waves) {
        const int w0 = wv.first, w1 = wv.second;
        for (int s = w0; s < w1; ++s) {
            tasks.push_back(int4{DAG_CHAIN, s, chain_rows, 0});
            chain_rows += nb_of[s];
        }
        if (w1 - w0 > max_wave_chains) { second = max_wave_chains; max_wave_chains = w1 - w0; }
        else if (w1 - w0 > second) second = w1 - w0;
        items.clear();
        for (int s = w0; s < w1; ++s) {
            const int nb = nb_of[s];
            for (int j = 0; j < nb; ++j) {
                const double key = (double)j / (double)nb;
                // Enveloped: the K-depth of a task, d = j - first[i], varies within a column from 0 (the band's far edge) to the
                // band's width (SUB(j), PRE(j) and the rows next to the diagonal: 110 blocks = 1.4 ms of K-loop in the headline
                // system), while a column passes in ~0.2 ms: drawn column by column, the deep tasks -- the chain's own inputs
                // first of all -- start far too late (traced: the chain waited 354 us of every step for sub(j), tile tasks
                // polled 37 % of the time they held a slot) and the shallow ones hold slots polling.  So a task is drawn
                // kDagEnvLead x d columns early.  Still topological: a task's inputs have a smaller column AND no larger first[],
                // hence a smaller key for any lead < 1; and no tile of a later column gets in front of SUB(j) / PRE(j + 1), which
                // is what the drain condition needs.  Headline step: lead 0 / 0.05 / 0.1 / 0.2 / 0.4 = 217.9 / 186.7 / 180.3 / 180.9 / 184.3 ms.
                // That sweep was at the 2^-52 band.  With the factor's own band (2^-28, oisat_factor_envelope: deepest K-loop 80 blocks,
                // tasks of 41 blocks on average) 0.1 leaves tile tasks polling 130 us of the 700 they hold a slot, 413 of 512 workgroups
                // computing: lead 0.05 / 0.1 / 0.15 / 0.2 / 0.25 / 0.3 = 128.8 / 116.2 / 111.0 / 110.7 / 111.3 / 111.3 ms per step (0.15 .. 0.3
                // within the spread between calls); 0.15 is kept, the smallest of the flat stretch -- at the 2^-52 band (override
                // only) it costs 0.4 % (181.1 -> 181.9 ms).
                // With a far stretch (kFactorFarBits = 18: 35 % of the headline's K-blocks at a third of their fp32 time) the tasks are
                // shorter and a column passes faster: lead 0.1 / 0.15 / 0.2 / 0.25 / 0.3 = 91.8 / 85.2, 85.1 / 84.4 / 84.6 / 84.4 ms per step;
                // 0.2 is kept there, the smallest of the flat stretch again.  Without a stretch the list is the one above, ticket for ticket.
                // With the middle stretch behind it (kFactorMidBits = 8: another 35 % of the K-blocks at ~0.6 of their fp32 time) the sweep
                // was repeated: lead 0.15 / 0.2 / 0.25 / 0.3 / 0.4 = 75.4, 75.5 / 74.4 / 74.2 / 74.4 / 74.8 ms per step.  0.2 .. 0.3 are level
                // within 0.2 ms: 0.2 stays, no third constant, and the order does not read the middle table.
                // With the shadow and its segments' reads no longer draining their DMA (far 2.83, middle 5.01 us per K-block on the 4 | 3
                // ring): lead 0.15 / 0.2 / 0.25 / 0.3 / 0.4 / 0.5 = 70.2 / 67.8, 67.7 / 67.1 / 66.5 / 66.9 / 67.7 ms per step; no flat stretch,
                // 0.3 is kept (the note at kDagEnvLeadFar: swept on 4 | 3; on the 2 | 1 ring that ships 0.2 -> 0.3 is 67.6 -> 66.3 ms).
                auto ekey = [&](int i, int jj) { return ((double)jj - env_lead * (double)(jj - first[i])) / (double)nb; };
                // PRE(j) reads row j up to column j - 2 only (the chain adds column j - 1 itself), so it is drawn ONE COLUMN EARLY,
                // in front of column j - 1's tasks: drawn with column j it was what a small system's chain waited for at every
                // step (58 us of a 141-us step; the tile tasks of column j then polled for T_j: 37 -> 16 us per task).  The
                // wait moves to SUB(j), which cannot start its last block before column j - 1 is out; a month: 48.9 -> 48.5 ms.
                auto word = [&](int kind, int i, int kend) {      // kind | k0 << 8 | kfar << 18
                    if (!first) return kind;
                    const int k0 = first[i];
                    int kfar = far ? far[i] : k0;
                    kfar = kfar < k0 ? k0 : kfar;
                    kfar = kfar > kend ? (kend > k0 ? kend : k0) : kfar;
                    return kind | k0 << 8 | kfar << 18;
                };
                if (j >= 2) items.push_back(Item{(first ? ekey(j, j - 1) : (double)(j - 1) / (double)nb) - 1e-9, int4{word(DAG_PRE, j, j - 1), s, j, j}});
                if (j >= 1 && j + 1 < nb) items.push_back(Item{first ? ekey(j + 1, j) : key, int4{word(DAG_SUB, j + 1, j), s, j + 1, j}});
                for (int i = j + 2; i < nb && (!first || first[i] <= j); ++i)
                    items.push_back(Item{first ? ekey(i, j) : key, int4{word(DAG_TILE, i, j), s, i, j}});
            }
        }
        std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key < b.key; });
        for (const Item& it : items) tasks.push_back(it.task);
    }
    out.chain_rows = chain_rows;
    // chains of consecutive waves overlap in time (a wave's chains are still walking their last columns when the next
    // wave's chain tickets are drawn): budget the two largest waves' worth
    out.max_wave_chains = max_wave_chains + (waves.size() > 1 ? (second > 0 ? second : max_wave_chains) : 0);
    {   // a CU to itself for the chains of the FIRST wave (the first tickets): at most four.  Each costs one of the 512 workgroup slots.
        int n = 0;
        const int first_w0 = waves[0].first, first_w1 = waves[0].second;
        while (first_w0 + n < first_w1 && n < 4 && nb_of[first_w0 + n] >= 8) ++n;
        out.reserve_chains = n;
    }
}

// The shadow's addressing (oisat_factor_shadow_layout): the strictly-lower tiles (r, k), first[r] <= k < r, row after row;
// rowoff[r] = tiles of the rows above r, tile (r, k) is number rowoff[r] + (k - first[r]).  Returns the number of tiles.
int64_t dag_shadow_layout(const int* first, int64_t nb, int64_t* rowoff) {
    int64_t n = 0;
    for (int64_t r = 0; r < nb; ++r) {
        rowoff[r] = n;
        n += r - first[r];
    }
    return n;
}

// This call's shadow (null: none) and its readers (DagSys::shuse) into the plan's system; a change waits for the launches
// that read the system's words as they are.
hipError_t dag_plan_shadow(DagPlan& p, char* shadow, int use, hipStream_t stream) {
    return dag_plan_sys0(p, p.sys_host[0].mid, p.sys_host[0].near, shadow, shadow ? p.shrow_dev : nullptr, use, true, stream);
}

// systems in table order (largest first)
// The progress words and the control block are zeroed ON `stream` (the stream the plan's launches go to): a plain hipMemset is
// ordered in the NULL stream only, which the handles' non-blocking streams do not wait for -- a launch could start on
// uninitialised words (wrong tickets, flags that read "ready").
// bands (single system only): its envelope and stretches; the ticket buffer is then sized for the dense list of these block rows
DagPlan* dag_plan_create(const std::vector<BatchMat>& table, hipStream_t stream, const DagSolveShape& shape, const DagBands& bands_arg) {
    DagPlan* p = new DagPlan();
    const int nsys = (int)table.size();
    const DagBands bands = nsys == 1 ? bands_arg : DagBands();
    const bool env = !bands.first.empty();
    p->nsys = nsys;
    p->sys_host.resize(nsys);
    std::vector<int> state_off(nsys);
    int words = 0;
    for (int s = 0; s < nsys; ++s) {
        state_off[s] = words;
        words += DAG_STATE_HDR + 3 * table[s].mpb;
        words = (words + 31) / 32 * 32;                          // every system's words on lines of their own
    }
    p->state_words = words;
    DagOrder order;
    {
        std::vector<int> nb_of(nsys);
        for (int s = 0; s < nsys; ++s) nb_of[s] = table[s].mpb;
        dag_task_order(nb_of, 0, order, env ? bands.first.data() : nullptr, env ? bands.far.data() : nullptr);
        if (shape.refine >= 0) {
            int64_t rows = 0, valu = 0;
            dag_queue_entries(nb_of, shape, &rows, &valu);
            p->qcap0 = rows;
            p->qcap = rows + valu;
        }
    }
    p->solve_refine = shape.refine;
    p->fwd_only = shape.fwd_only;
    p->tasks_cap = order.tasks.size();
    if (env) {                                                  // chain + PRE + SUB + every lower tile two or more below the diagonal
        const size_t nb = (size_t)table[0].mpb;
        p->tasks_cap = 1 + 2 * nb + nb * (nb + 1) / 2;
    }
    bool ok = hipMalloc((void**)&p->sys_dev, sizeof(DagSys) * nsys) == hipSuccess &&
              hipMalloc((void**)&p->tasks_dev, sizeof(int4) * p->tasks_cap) == hipSuccess &&
              hipMalloc((void**)&p->state_dev, sizeof(int) * words) == hipSuccess &&
              hipMalloc((void**)&p->ctl_dev, sizeof(DagCtl)) == hipSuccess &&
              (!env || hipMalloc((void**)&p->mid_dev, sizeof(int) * bands.first.size()) == hipSuccess) &&
              (!env || hipMalloc((void**)&p->near_dev, sizeof(int) * bands.first.size()) == hipSuccess) &&
              (!env || hipMalloc((void**)&p->shrow_dev, sizeof(int64_t) * bands.first.size()) == hipSuccess) &&
              (p->qcap == 0 || (p->qcap < (int64_t)INT32_MAX / 4 && hipMalloc((void**)&p->queue_dev, 16 * (size_t)p->qcap) == hipSuccess));
    if (ok && p->qcap > 0) ok = hipMemsetAsync(p->queue_dev, 0, 16 * (size_t)p->qcap, stream) == hipSuccess;
    if (ok) {
        for (int s = 0; s < nsys; ++s)
            p->sys_host[s] = DagSys{table[s].S, table[s].tinv, table[s].ld, p->state_dev + state_off[s], table[s].mpb, s};
        ok = hipMemcpy(p->sys_dev, p->sys_host.data(), sizeof(DagSys) * nsys, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(p->tasks_dev, order.tasks.data(), sizeof(int4) * order.tasks.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemsetAsync(p->state_dev, 0, sizeof(int) * words, stream) == hipSuccess &&
             hipMemsetAsync(p->ctl_dev, 0, sizeof(DagCtl), stream) == hipSuccess && dag_plan_install(*p, order, bands, stream) == hipSuccess;
    }
    if (!ok) {
        dag_plan_free(p);
        oisat_set_error("task-graph factorization: allocation or upload of the plan failed");
        return nullptr;
    }
    return p;
}

// A cached enveloped plan meets another envelope (same matrix, same block rows): new ticket list into the SAME buffers.  The
// copy is enqueued on `stream`, behind the launches that still read the old list.
int dag_plan_refill(DagPlan& p, const DagBands& bands, hipStream_t stream) {
    DagOrder order;
    dag_task_order(std::vector<int>{p.sys_host[0].nb}, 0, order, bands.first.data(), bands.far.data());
    if (order.tasks.size() > p.tasks_cap) {
        oisat_set_error("task-graph factorization: %zu tickets do not fit the plan's %zu", order.tasks.size(), p.tasks_cap);
        return OISAT_EINVAL;
    }
    HIP_TRY(hipStreamSynchronize(stream));                      // (the host list is the source of a copy that may still be in flight)
    if (p.trace_dev) { (void)hipFree(p.trace_dev); p.trace_dev = nullptr; }      // (profiling aid: sized by the ticket count)
    HIP_TRY(dag_plan_install(p, order, bands, stream));
    HIP_TRY(hipMemcpyAsync(p.tasks_dev, p.tasks_host.data(), sizeof(int4) * p.tasks_host.size(), hipMemcpyHostToDevice, stream));
    return OISAT_OK;
}

}  // namespace oisat_dense

void oisat_dag_plan_release(void* plan) { dag_plan_free((DagPlan*)plan); }

extern "C" int oisat_dag_task_order(int nsys, const int32_t* block_rows, int wave, int32_t* tasks_out, int64_t capacity,
                                    int64_t* ntasks_out, int32_t* reserve_out, int32_t* max_wave_chains_out) {
    ARG_CHECK(nsys > 0 && block_rows && ntasks_out && (tasks_out || capacity == 0));
    std::vector<int> nb_of(block_rows, block_rows + nsys);
    for (int s = 0; s < nsys; ++s) ARG_CHECK(nb_of[s] >= 1 && (s == 0 || nb_of[s] <= nb_of[s - 1]));
    DagOrder order;
    dag_task_order(nb_of, wave, order);
    *ntasks_out = (int64_t)order.tasks.size();
    if (reserve_out) *reserve_out = order.reserve_chains;
    if (max_wave_chains_out) *max_wave_chains_out = order.max_wave_chains;
    if ((int64_t)order.tasks.size() > capacity) return capacity == 0 ? OISAT_OK : OISAT_EINVAL;
    memcpy(tasks_out, order.tasks.data(), sizeof(int4) * order.tasks.size());
    return OISAT_OK;
}

extern "C" int oisat_dag_task_order_env(int nb, const int32_t* first, const int32_t* far, int32_t* tasks_out, int64_t capacity,
                                        int64_t* ntasks_out) {
    ARG_CHECK(nb >= 1 && nb <= kDagEnvMaxBlocks && first && ntasks_out && (tasks_out || capacity == 0));
    ARG_CHECK(envelope_table_ok(first, nb));
    if (far)
        for (int i = 0; i < nb; ++i) ARG_CHECK(far[i] >= first[i] && far[i] <= i);
    // Profiling aid, this query only (no launch reads it): OISAT_DAG_ORDER_LEAD_FAR = the order a far list would have at
    // another ticket lead, 0 <= lead < 1 -- tools/dag_sched_model.py sets a traced launch's lead beside that launch's costs.
    double lead_far = kDagEnvLeadFar;
    if (const int set = dag_order_lead_far(&lead_far))
        ARG_CHECK(set > 0 && lead_far >= 0.0 && lead_far < 1.0 && "OISAT_DAG_ORDER_LEAD_FAR is a number in [0, 1)");
    DagOrder order;
    dag_task_order(std::vector<int>{nb}, 0, order, first, far, lead_far);
    *ntasks_out = (int64_t)order.tasks.size();
    if ((int64_t)order.tasks.size() > capacity) return capacity == 0 ? OISAT_OK : OISAT_EINVAL;
    memcpy(tasks_out, order.tasks.data(), sizeof(int4) * order.tasks.size());
    return OISAT_OK;
}
