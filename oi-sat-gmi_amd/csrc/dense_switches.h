// The run-time switches of the dense solver: every environment variable that the dense_*.hip units and their .inc
// files read, each behind one function.  They are A/B and test aids; no caller of the library needs one.  Every switch is read
// at every call -- the tests flip them inside one process -- except OISAT_PROF_DETAIL, read once.  A function only parses: what
// a value means is its reader's comment.  The table lists every switch; its last column names tests that flip the switch, not
// all of them (grep tests/ for the name).
//
//   variable                   values                               reader                                        tests, among others
//   OISAT_DAG                  0 | 1 (atoi)                         dag_wanted (dense_internal.h)                 test_gpu_readers_abi
//   OISAT_POTRF                recursive | lookahead[:<blocks>]     potrf_impl (dense_chol.hip)                   test_gpu_parity, test_gpu_far_band
//   OISAT_FWD_IN_LAUNCH        0 = off (atoi)                       potrf_impl (dense_chol.hip)                   test_gpu_fwd_in_launch
//   OISAT_FACTOR_SHADOW        0 | 1 | far | mid                    potrf_impl (dense_chol.hip)                   test_gpu_factor_shadow, test_gpu_seg_pipeline
//   OISAT_DAG_TRACE            <file>                               dag_launch (dense_dag.hip)                    - (tools/dag_trace.py)
//   OISAT_DAG_FLAGS            <int> (atoi), hooks build only       dag_launch (dense_dag.hip)                    test_gpu_dag
//   OISAT_DAG_ORDER_LEAD_FAR   <number in [0, 1)>                   oisat_dag_task_order_env (dense_dag_plan.hip) test_dag_sched_model_cpu
//   OISAT_ENVELOPE             0 = off (atoi)                       the enveloped entry points (dense_chol.hip,   test_gpu_envelope, test_far_band_cpu
//                                                                   dense_cov.hip), stretch_table (dense_tables.hip)
//   OISAT_FACTOR_CUT_BITS      <number in [1, 52]>                  oisat_factor_envelope_corr (dense_tables.hip) test_factor_envelope_cpu
//   OISAT_FACTOR_FAR_BITS      0 | <number in [1, 52]>              oisat_factor_far_corr (dense_tables.hip)      test_far_band_cpu
//   OISAT_FACTOR_MID_BITS      0 | <number in [1, 52]>              oisat_factor_mid_corr (dense_tables.hip)      test_mid_band_cpu
//   OISAT_FACTOR_NEAR_BITS     0 | <number in [1, 52]> | all        oisat_factor_near_corr (dense_tables.hip)     test_near_band_cpu
//   OISAT_TRSV_TWO_TILES       0 | 1                                trsv_launch_shape (dense_solve.hip)           test_gpu_sweep_tiles
//   OISAT_TRSV_MAX_WGS         <integer >= 1>                       trsv_launch_shape (dense_solve.hip)           test_gpu_sweep_tiles
//   OISAT_RESID_UPDATE         0 | 1                                oisat_gain_solve (dense_solve.hip)            test_gpu_resid_update
//   OISAT_INC_OVERLAP          0 | 1                                oisat_inc_overlap_plan (dense_solve.hip)      test_inc_overlap_cpu, test_gpu_inc_overlap
//   OISAT_SOLVE_FAR_BITS       <number in [0, 52]>                  far_chord_of (dense_solve_dev.inc)            test_solve_tiers_cpu, test_gpu_solve_tiers
//   OISAT_PROF_DETAIL          0 | 1 (atoi), read once              launch_gemm(_batched) (dense_gemm.hip)        - (profiling aid)
#pragma once
#define OISAT_DENSE_SWITCHES_H                                  // (dense_solve_dev.inc, included inside a namespace, checks for it)

#include <cstdint>
#include <cstdlib>
#include <cstring>

// OISAT_ENVELOPE=0: the enveloped entry points behave as their dense counterparts (A/B timing, tests)
inline bool oisat_envelope_off() {
    const char* e = getenv("OISAT_ENVELOPE");
    return e != nullptr && atoi(e) == 0;
}

namespace oisat_dense __attribute__((visibility("hidden"))) {    // (inline functions: nothing of this in the library's symbol table)

// OISAT_PROF_DETAIL=1 (profiling aid): one profile record per launch shape of the GEMM instead of per name
inline bool prof_detail() {
    static const bool detail = getenv("OISAT_PROF_DETAIL") && atoi(getenv("OISAT_PROF_DETAIL")) != 0;
    return detail;
}

// OISAT_DAG=0 | 1: the task graph nowhere | wherever it applies; -1: unset, by size
inline int dag_env_mode() { return getenv("OISAT_DAG") ? atoi(getenv("OISAT_DAG")) : -1; }

// OISAT_POTRF=recursive | lookahead[:panel blocks].  false: unset.  *lookahead: the look-ahead schedule is asked for;
// *pw: its panel width where one is given (> 0), else untouched.  Any value, even one that names no schedule, rules out the task graph.
inline bool potrf_schedule(bool* lookahead, int64_t* pw) {
    const char* env = getenv("OISAT_POTRF");
    *lookahead = false;
    if (!env) return false;
    if (strncmp(env, "lookahead", 9) == 0) {
        *lookahead = true;
        if (env[9] == ':' && atoi(env + 10) > 0) *pw = atoi(env + 10);      // OISAT_POTRF=lookahead:4
    }
    return true;
}

// OISAT_FWD_IN_LAUNCH=0: oisat_potrf_env_fwd factors as oisat_potrf_env and leaves the whole first solve to oisat_gain_solve
inline bool fwd_in_launch_off() {
    const char* e = getenv("OISAT_FWD_IN_LAUNCH");
    return e != nullptr && atoi(e) == 0;
}

// OISAT_FACTOR_SHADOW: who reads the factor's shadow (dense_dag.inc "Shadow") -- unset or 1: the far and the middle stretch (3);
// 0: there is none, both convert in their K-loops; far / mid: only that stretch reads it (1 / 2; the writers store all the
// same, so that each half can be judged alone).  Anything else: -1.
inline int factor_shadow_mode() {
    const char* e = getenv("OISAT_FACTOR_SHADOW");
    if (!e || !*e || strcmp(e, "1") == 0) return 3;
    if (strcmp(e, "0") == 0) return 0;
    if (strcmp(e, "far") == 0) return 1;
    if (strcmp(e, "mid") == 0) return 2;
    return -1;
}

// OISAT_DAG_TRACE=file (profiling aid): where a task-graph launch writes its stamps, or nullptr
inline const char* dag_trace_file() { return getenv("OISAT_DAG_TRACE"); }

#ifdef OISAT_TEST_HOOKS
// OISAT_DAG_FLAGS (liboisat_hip_testhooks.so only): DagLane::flags of the next task-graph launches
inline int dag_test_flags() { return getenv("OISAT_DAG_FLAGS") ? atoi(getenv("OISAT_DAG_FLAGS")) : 0; }
#endif

// A switch that holds a number.  0: unset (or, with empty_is_unset, empty) and *out stays; 1: *out = the number; -1: not a number.
inline int number_switch(const char* name, bool empty_is_unset, double* out) {
    const char* e = getenv(name);
    if (!e || (empty_is_unset && !*e)) return 0;
    char* end = nullptr;
    *out = strtod(e, &end);
    return end != e && *end == '\0' ? 1 : -1;
}
// OISAT_DAG_ORDER_LEAD_FAR (oisat_dag_task_order_env only); OISAT_FACTOR_CUT_BITS, OISAT_FACTOR_FAR_BITS, OISAT_FACTOR_MID_BITS,
// OISAT_FACTOR_NEAR_BITS;
// OISAT_SOLVE_FAR_BITS: the readers check the range
inline int dag_order_lead_far(double* out) { return number_switch("OISAT_DAG_ORDER_LEAD_FAR", false, out); }
inline int factor_bits_switch(const char* name, double* out) { return number_switch(name, true, out); }
inline int solve_far_bits(double* out) { return number_switch("OISAT_SOLVE_FAR_BITS", true, out); }
// OISAT_FACTOR_NEAR_BITS=all: the one spelling of that switch that is not a number
inline bool factor_near_all() {
    const char* e = getenv("OISAT_FACTOR_NEAR_BITS");
    return e && strcmp(e, "all") == 0;
}
// a forced OISAT_FACTOR_CUT_BITS switches the stretches' default rule off, whatever it holds
inline bool factor_cut_bits_set() {
    const char* c = getenv("OISAT_FACTOR_CUT_BITS");
    return c && *c;
}

// OISAT_TRSV_TWO_TILES=0 | 1 forces the choice of oisat_trsv_plan.  -1: unset or empty; -2: anything else
inline int trsv_two_tiles_forced() {
    const char* e = getenv("OISAT_TRSV_TWO_TILES");
    if (!e || !*e) return -1;
    return ((e[0] == '0' || e[0] == '1') && e[1] == '\0') ? e[0] - '0' : -2;
}

// OISAT_TRSV_MAX_WGS=<n >= 1> caps the sweeps' grid.  0: unset or empty; 1: *cap = n; -1: not such an integer
inline int trsv_max_wgs(long* cap) {
    const char* e = getenv("OISAT_TRSV_MAX_WGS");
    if (!e || !*e) return 0;
    char* end = nullptr;
    *cap = strtol(e, &end, 10);
    return end != e && *end == '\0' && *cap >= 1 ? 1 : -1;
}

// OISAT_RESID_UPDATE=0: oisat_gain_solve forms every residual in float64, the launches and bits of the code before the update
// form.  Unset or empty: 1; anything but 0 or 1: -1.
inline int resid_update_mode() {
    const char* e = getenv("OISAT_RESID_UPDATE");
    if (!e || !*e) return 1;
    return ((e[0] == '0' || e[0] == '1') && e[1] == '\0') ? e[0] - '0' : -1;
}

// OISAT_INC_OVERLAP=0: DenseAnalysis.run keeps oisat_gain_solve + oisat_apply_increment_grid, the launches and bits of the code
// before oisat_gain_solve_fields; 1: the new entry wherever it is legal, whatever the system's size (tests).  Unset or empty: -1,
// the rule of oisat_inc_overlap_plan decides; anything else: -2.
inline int inc_overlap_mode() {
    const char* e = getenv("OISAT_INC_OVERLAP");
    if (!e || !*e) return -1;
    return ((e[0] == '0' || e[0] == '1') && e[1] == '\0') ? e[0] - '0' : -2;
}

}  // namespace oisat_dense
