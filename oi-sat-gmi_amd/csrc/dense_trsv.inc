// The triangular sweeps' device functions: one block row of a sweep (trsv_row) with its hand-off (wait_payload, trsv_leave), the
// control block and the tile macros.  Included by dense_solve.hip (trsv_pipe_kernel, trsv_batched_kernel) and by dense_dag.hip (the
// sweep rows as tasks of the task-graph launch), inside their anonymous namespaces; no kernels here.  Expects dense_tile.inc (NB)
// before it.

// ---- triangular solves (vector right-hand side, double accumulation) --------------------------
// ONE launch per sweep.  Workgroup with ticket b owns block row b (forward) / block column b
// (backward).  It streams its 128x128 blocks of L through LDS (prefetching the next block into
// registers while it waits), applies each update as soon as the producing workgroup has published
// that piece of the solution, then multiplies by the inverted diagonal block and publishes its own
// piece.  Tickets are drawn from an atomic counter, so a workgroup only ever waits on workgroups
// that started before it: no assumption on dispatch order or residency.
// Hand-off: the PAYLOAD IS THE FLAG.  The solution vector is pre-filled with a NaN bit pattern no
// computation produces; the producer publishes its 128 doubles with agent-scope relaxed atomic
// stores (each 8-byte store is self-contained, so no fence, no vmcnt drain, no separate flag), the
// consumer's lanes each poll their own element with agent-scope atomic loads until it differs from
// the pattern.  Agent-scope traffic bypasses the per-XCD L2s, ~2 us a round trip: this form costs
// two of them per block step on the critical path, the flag-after-payload form it replaces cost
// five (store, drain, flag store | flag poll, payload load) -- 11.5 -> 6 us per step.  Spins are bounded.
constexpr int TLD = NB + 1;              // LDS tile row stride (odd: row- and column-walks are conflict-free)
constexpr unsigned long long kTrsvEmpty = 0x7ff80bad7ff80badull;      // a quiet NaN with that payload, both halves equal

// OISAT_STATUS_UNCONVERGED_MEMBER: the LOWEST caller index among the batch members that ended unconverged since the last clear,
// kept as index + 1 with 0 = none -- a minimum, so the word does not depend on which workgroup reports first.
__device__ __forceinline__ void note_unconverged_member(int* word, int which) {
    const int v = which + 1;
    int old = atomicCAS(word, 0, v);
    while (old != 0 && old > v) {
        const int seen = atomicCAS(word, old, v);
        if (seen == old) break;
        old = seen;
    }
}

// trsv_row and wait_payload may touch `error` ONLY: the task-graph launch hands them its own control block (DagCtl, whose
// `error` sits at the same offset -- asserted at the cast, dense_dag.inc: dag_sweep_task); ticket and done are the kernels'.
struct TrsvCtl {                         // zero when a sweep starts: zeroed at allocation, then by the last workgroup of every sweep
    unsigned ticket;
    unsigned error;
    unsigned done;
    unsigned pad;
};


// 256 threads: thread t moves 16 B at row (t>>5)+8p, column (t&31)*4 -> every row is one 512-B segment.
// Macros, not functions: the 16 x float4 staging registers must stay in VGPRs (arrays passed by
// reference ended up in scratch).
#define TILE_PREFETCH(src, ldsrc)                                                                              \
    _Pragma("unroll") for (int p = 0; p < 16; ++p)                                                             \
        reg[p] = *reinterpret_cast<const float4*>((src) + (int64_t)((tid >> 5) + 8 * p) * (ldsrc) + (tid & 31) * 4);
#define TILE_STORE()                                                                                           \
    _Pragma("unroll") for (int p = 0; p < 16; ++p) {                                                           \
        float* q = tile + ((tid >> 5) + 8 * p) * TLD + (tid & 31) * 4;                                         \
        q[0] = reg[p].x; q[1] = reg[p].y; q[2] = reg[p].z; q[3] = reg[p].w;                                    \
    }

// threads 0..127 fetch one published double each into vec[]; returns false if a producer never showed up
__device__ __forceinline__ bool wait_payload(const double* src, double* vec, TrsvCtl* ctl, unsigned* err_total, int tid,
                                             unsigned* lds_ok) {
    if (tid < NB) {
        const unsigned long long* p = reinterpret_cast<const unsigned long long*>(src) + tid;
        unsigned long long bits;
        unsigned spins = 0;
        while ((bits = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kTrsvEmpty) {
            __builtin_amdgcn_s_sleep(1);
            ++spins;
            if ((spins & 1023u) == 0u &&
                (spins > (1u << 22) || __hip_atomic_load(&ctl->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
                if (__hip_atomic_exchange(&ctl->error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                    atomicAdd(err_total, 1u);             // survives the per-sweep memset: read by checked solves
                *lds_ok = 0u;
                break;
            }
        }
        vec[tid] = __builtin_bit_cast(double, bits);
    }
    __syncthreads();
    return *lds_ok != 0u;
}

// forward: L y = r.  transpose == 0.   backward: L^T z = y.  transpose == 1 (block index runs downwards).
// sol must arrive filled with kTrsvEmpty.
// A workgroup claims block rows by ticket until none is left (round 3).  A row waits only for rows with lower tickets, and
// every claimed row is in the hands of a running workgroup, so the sweep drains with ANY number of resident workgroups.
// The grid is oisat_trsv_plan's (trsv_solve): a workgroup per row for a dense factor -- with fewer, a row's producers are
// fetched one agent-scope round trip after the other instead of while waiting for its turn (measured at 4 rows per
// workgroup: 0.54 vs 0.25 ms per sweep at 10,000 observations, a localised month 73.3 vs 69.6 ms) --, one workgroup per CU
// with two LDS tiles for a narrow-banded enveloped factor, where only the rows within a band width of the front have
// anything to do and each workgroup serves several rows one after the other.
// one block row of a sweep: claim order tk (0 .. nb-1) of ITS system; false = a producer never showed up (bounded spin)
// DAG: the row is a task of the task-graph launch (dense_dag.inc) -- the vectors are then shared with workgroups of the SAME
// launch across sweeps, so every store to them is an agent-scope (write-through) store and every load of a word another
// workgroup wrote an agent-scope load (cdna_hip_programming.md Guideline 16); between launches plain accesses do.
// step0: the first producer step that is walked (0 <= step0 <= tk).  Above 0 only for an ENVELOPED factor (oisat_potrf_env):
// the blocks of the skipped producers are exact zeros, whose products would add 0.0 to the double accumulator.
template <int TRANSPOSE, bool DAG>
__device__ __forceinline__ bool trsv_row(const float* __restrict__ L, int64_t ld, const float* __restrict__ tinv, int nb, int tk, int step0,
                                         double* __restrict__ rhs, double* __restrict__ sol, TrsvCtl* __restrict__ ctl,
                                         unsigned* __restrict__ err_total, int two_tiles, double* __restrict__ zout, int64_t m,
                                         int accumulate, float* __restrict__ tile, double* __restrict__ vec, double* __restrict__ part,
                                         unsigned* __restrict__ s_ok) {
    int tid = threadIdx.x;
    // (a task of the persistent launch: everything this row derives from its lane number is THIS call's value -- left to itself
    // the compiler forms the staging addresses in front of the launch's task loop and keeps them live across the K-loops)
    if (DAG) asm volatile("" : "+v"(tid));
    const int row = tid & (NB - 1), hf = tid >> 7;       // two threads per row: columns [64*hf, 64*hf+64)
    float* const tileT = tile + NB * TLD;
    const int b = TRANSPOSE ? nb - 1 - tk : tk;             // my block row (fwd) / block column (bwd)
    double acc = 0.0;
    if (hf == 0) {
        // my block of the right-hand side is read by nobody else: take it and leave the "not yet published" pattern
        // behind, so that the NEXT sweep (which publishes its solution into this vector) finds it prepared
        if (DAG) {
            acc = __hip_atomic_load(&rhs[(int64_t)b * NB + row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(rhs) + (int64_t)b * NB + row, kTrsvEmpty, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        } else {
            acc = rhs[(int64_t)b * NB + row];
            reinterpret_cast<unsigned long long*>(rhs)[(int64_t)b * NB + row] = kTrsvEmpty;
        }
    }
    float4 reg[16];
    const int nsteps = tk;                                  // producers: claim orders 0 .. tk-1
    // step-th producer j = step (fwd) / nb-1-step (bwd); its block is L[b, j] (fwd, j < b) or L[j, b] (bwd, j > b)
    const float* Tb = tinv + (int64_t)b * NB * NB;
    const float* base = TRANSPOSE ? L + (int64_t)(nb - 1) * NB * ld + (int64_t)b * NB : L + (int64_t)b * NB * ld;
    const int64_t hop = TRANSPOSE ? -(int64_t)NB * ld : (int64_t)NB;      // pointer step from one producer's block to the next
    // two_tiles: T_b goes to a second LDS tile right away -- it depends on nobody -- so that the last pass finds it there
    // instead of loading and staging it behind the last producer's hand-over.  A workgroup that serves several rows restages
    // it per row: the claim loop's top barrier stands between the previous row's last read of tileT and this store, and a
    // barrier (wait_payload's, or the last pass's) between this store and the read -- also for a row without producers.
    if (two_tiles) {
        TILE_PREFETCH(Tb, NB)
        float* tile = tileT;                                // TILE_STORE writes to the `tile` in scope
        TILE_STORE()
    }
    if (nsteps > step0) { const float* b0 = base + (int64_t)step0 * hop; TILE_PREFETCH(b0, ld) } else if (!two_tiles) { TILE_PREFETCH(Tb, NB) }
    for (int step = step0; step <= nsteps; ++step) {
        const bool last = step == nsteps;                   // last pass: multiply by the inverted diagonal block
        if (!(last && two_tiles)) TILE_STORE()              // this step's block: in LDS before the wait, off the critical path
        if (!last) {
            const int j = TRANSPOSE ? nb - 1 - step : step;
            if (!wait_payload(sol + (int64_t)j * NB, vec, ctl, err_total, tid, s_ok)) return false;
            if (step + 1 < nsteps) { const float* nx = base + (int64_t)(step + 1) * hop; TILE_PREFETCH(nx, ld) }
            else if (!two_tiles) { TILE_PREFETCH(Tb, NB) }
        } else {
            if (hf == 0) vec[row] = acc;
            __syncthreads();
        }
        double u = 0.0;
        const int c0 = hf * 64;
        const float* blk = (last && two_tiles) ? tileT : tile;
        if (!TRANSPOSE) {
#pragma unroll 8
            for (int c = c0; c < c0 + 64; ++c) u += (double)blk[row * TLD + c] * vec[c];       // row of the block
        } else {
#pragma unroll 8
            for (int c = c0; c < c0 + 64; ++c) u += (double)blk[c * TLD + row] * vec[c];       // column of the block
        }
        if (hf == 1) part[row] = u;
        __syncthreads();
        if (hf == 0) {
            if (!last) acc -= u + part[row];
            else acc = u + part[row];
        }
    }
    if (hf == 0) {
        const int64_t i = (int64_t)b * NB + row;
        __hip_atomic_store(&sol[i], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (zout != nullptr && i < m) {                     // the solve's result where the caller wants it
            if (DAG) {
                const double zi = accumulate ? __hip_atomic_load(&zout[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + acc : acc;
                __hip_atomic_store(&zout[i], zi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                zout[i] = accumulate ? zout[i] + acc : acc;
            }
        }
    }
    return true;
}

__device__ __forceinline__ void trsv_leave(TrsvCtl* __restrict__ ctl) {        // thread 0: the last workgroup to leave hands
    const unsigned gone = __hip_atomic_fetch_add(&ctl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // the block back clean
    if (gone == gridDim.x - 1u) {
        __hip_atomic_store(&ctl->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl->error, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
