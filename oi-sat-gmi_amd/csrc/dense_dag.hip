// The task-graph unit of the dense solver: the persistent kernel that factors (and, in oisat_batch_analyse, solves) whole systems
// as one launch -- dense_dag.inc, the device half -- with dag_launch, and the register-resident diagonal-block kernel that the
// other factorization schedules launch through launch_potrf_diag.  The two kernels run the same diagonal-block waves
// (dense_diag.inc) and stay in one translation unit: profiles/EXPERIMENTS.md, "the rest of the split".
// The only unit with test hooks: liboisat_hip_testhooks.so is the library with this file compiled under -DOISAT_TEST_HOOKS.
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"
#include "dense_kloop.inc"                                      // (dag_seg: the K-loop of gemm_nt_big_kernel as a function)
#include "dense_diag.inc"

__global__ __launch_bounds__(D3_THREADS, 4) void potrf_diag3_kernel(float* __restrict__ S, int64_t ld, int64_t k0, float* __restrict__ tinv,
                                                                    int* __restrict__ info, int block_index, const BatchMat* __restrict__ mats,
                                                                    int prio) {
    __shared__ __attribute__((aligned(16))) float Pp[2 * D3_PBUF], Xr[7 * D3_TILE], dinvb[2 * D3_TILE], stage[16 * D3_SLD];
    group_prio(prio);
    if (mats) {                            // batched: workgroup = matrix blockIdx.x of the table (largest first)
        const BatchMat bm = mats[blockIdx.x];
        if (block_index >= bm.mpb) return;
        S = bm.S;
        ld = bm.ld;
        tinv = bm.tinv;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    gfloat* Sb = (gfloat*)(S + k0 * ld + k0);
    gfloat* Tg = (gfloat*)(tinv + (int64_t)block_index * NB * NB);
    if (w == 0) d3_diagonal_wave<false>(Sb, ld, Pp, dinvb, stage, info, (int)k0, lane, lr, lg, (int)blockIdx.x);
    else if (w == 1) d3_worker_wave<1, false>(Sb, ld, Tg, Pp, Xr, dinvb, stage, lr, lg);
    else if (w == 2) d3_worker_wave<2, false>(Sb, ld, Tg, Pp, Xr, dinvb, stage, lr, lg);
    else d3_worker_wave<3, false>(Sb, ld, Tg, Pp, Xr, dinvb, stage, lr, lg);
}

#include "dense_trsv.inc"                                       // (the sweep rows as tasks)
#include "dense_solve_dev.inc"                                  // (the correlation functions; the solve-phase bodies)
#include "dense_dag.inc"

}  // namespace

namespace oisat_dense {

int launch_potrf_diag(oisat_ctx* h, unsigned nsys, float* S, int64_t ld, int64_t k0, float* tinv, int* info_dev, int block_index,
                      const BatchMat* mats, int prio) {
    OISAT_LAUNCH(h, "potrf_diag", potrf_diag3_kernel, dim3(nsys), dim3(D3_THREADS), 0, S, ld, k0, tinv, info_dev, block_index, mats, prio);
    return OISAT_OK;
}

// ---- host: the launch (its plan: dense_dag_plan.hip) ---------------------------------------------------------------------
// OISAT_DAG_TRACE=file (profiling aid): the launch is followed by a synchronisation and its stamps are written to `file`:
// int32 ntasks, chain_rows; int32[ntasks][4] tasks; int64[ntasks][4] ticket stamps; int64[chain_rows][8] chain stamps (100 MHz)
// dag_timeouts: the handle's task-graph time-out word (status slot 4, word 6)
int dag_launch(oisat_ctx* h, DagPlan& p, int* info_dev, unsigned* dag_timeouts, const DagSolve* solve) {
    const int slots = dag_slots(h);
    if (!dag_fits(p.max_wave_chains, slots)) {                  // (callers check dag_fits before they make a plan; a handle's stream may have changed since)
        oisat_set_error("task-graph factorization: %d chains of one wave on %d resident workgroups would not drain", p.max_wave_chains, slots);
        return OISAT_EINVAL;
    }
    if ((solve != nullptr) != (p.solve_refine >= 0) || (solve && solve->refine != p.solve_refine)) {
        oisat_set_error("task-graph launch: plan and solve arguments do not belong together");
        return OISAT_EINVAL;
    }
    const int grid = p.ntasks < slots ? p.ntasks : slots;
    const char* trace_file = dag_trace_file();
    const size_t trace_words = 4 * ((size_t)p.ntasks + (size_t)p.qcap) + 8 * (size_t)p.chain_rows + 8 * (size_t)grid;
    if (trace_file && !p.trace_dev) HIP_TRY(hipMalloc((void**)&p.trace_dev, sizeof(long long) * trace_words));       // (grid is a plan's constant)
    if (trace_file) HIP_TRY(hipMemsetAsync(p.trace_dev, 0, sizeof(long long) * trace_words, h->stream));
    int flags = 0;
#ifdef OISAT_TEST_HOOKS
    flags = dag_test_flags();
#endif
    if (p.fwd_only && (p.nsys != 1 || !solve || !solve->fwd_rhs || !solve->fwd_sol || solve->nsys != 1)) {
        oisat_set_error("task-graph launch: the forward-sweep plan takes one system and its two work vectors");
        return OISAT_EINVAL;
    }
    if (solve) {
        if (solve->queue != p.queue_dev || solve->qcap != (int)p.qcap || solve->qcap0 != (int)p.qcap0) {
            oisat_set_error("task-graph launch: the solve arguments carry another plan's ready queue");
            return OISAT_EINVAL;
        }
        if (p.fwd_only) {
            OISAT_LAUNCH(h, "potrf_dag", potrf_dag_kernel<DAG_SOLVE_FWD>, dim3((unsigned)grid), dim3(256), 0, (const DagSys*)p.sys_dev,
                         (const int4*)p.tasks_dev, p.ntasks, p.ctl_dev, info_dev, dag_timeouts, p.state_dev, p.state_words, p.reserve_chains, flags,
                         trace_file ? p.trace_dev : (long long*)nullptr, p.chain_rows, *solve);
        } else {
            OISAT_LAUNCH(h, "analyse_dag", potrf_dag_kernel<DAG_SOLVE_ALL>, dim3((unsigned)grid), dim3(256), 0, (const DagSys*)p.sys_dev,
                         (const int4*)p.tasks_dev, p.ntasks, p.ctl_dev, info_dev, dag_timeouts, p.state_dev, p.state_words, p.reserve_chains, flags,
                         trace_file ? p.trace_dev : (long long*)nullptr, p.chain_rows, *solve);
        }
    } else {
        OISAT_LAUNCH(h, "potrf_dag", potrf_dag_kernel<DAG_SOLVE_NONE>, dim3((unsigned)grid), dim3(256), 0, (const DagSys*)p.sys_dev,
                     (const int4*)p.tasks_dev, p.ntasks, p.ctl_dev, info_dev, dag_timeouts, p.state_dev, p.state_words, p.reserve_chains, flags,
                     trace_file ? p.trace_dev : (long long*)nullptr, p.chain_rows, DagSolve{});
    }
    if (trace_file) {
        std::vector<long long> host(trace_words);
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(host.data(), p.trace_dev, sizeof(long long) * trace_words, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(trace_file, "wb")) {
            const int hdr[2] = {p.ntasks + (int)p.qcap, p.chain_rows + grid};  // (rows ntasks .. are the ready tasks' stamps: their task is in word 3; behind the chains' rows one row per workgroup)
            fwrite(hdr, sizeof(int), 2, f);
            fwrite(p.tasks_host.data(), sizeof(int4), p.tasks_host.size(), f);
            {
                const std::vector<int4> pad((size_t)p.qcap, int4{-1, 0, 0, 0});
                fwrite(pad.data(), sizeof(int4), pad.size(), f);
            }
            fwrite(host.data(), sizeof(long long), host.size(), f);
            fclose(f);
        }
    }
    return OISAT_OK;
}

}  // namespace oisat_dense
