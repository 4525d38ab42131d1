"""Measurement (not a gate): what a posterior ensemble costs next to the analysis it belongs to and next to the randomized error
``posterior_error_mc(256)``, all in one run.  Per-kernel HIP-event times (``oisat_prof_*``) of ``posterior_ensemble`` at K members
of F features on a workload of bench.py (default: the headline synthetic month), medians over the repetitions behind one
warm-up, clocks as found; the wall time includes the host draws, the uploads and the read-back of the K fields.  Also the
median ``err_se / err`` of the ensemble beside that of the randomized estimate: the number the ensemble is there for.

    python tools/ensemble_timing.py [--workload config3_720x1440_1e5obs] [--members 32 128] [--features 256] [--reps 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oi-sat-gmi_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
from oisatgmi import _hip  # noqa: E402


def timed(ctx, fn, reps):
    """Medians over ``reps`` profiled calls of ``fn`` -> (wall seconds, per-kernel dict, the last result)."""
    walls, kernels, res = [], [], None
    for _ in range(reps):
        ctx.prof_reset()
        ctx.prof_enable(True)
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
        kernels.append(ctx.prof_collect())
        ctx.prof_enable(False)
    per_kernel = {k: {"launches": kernels[0][k]["launches"], "median_ms": float(np.median([r[k]["total_ms"] for r in kernels]))}
                  for k in sorted(kernels[0])}
    return float(np.median(walls)), per_kernel, res


def rel_se(est):
    err = est["err"].astype(np.float64)
    return float(np.nanmedian(np.where(err > 0, est["err_se"] / np.where(err > 0, err, 1.0), np.nan)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=bench.DEFAULT, choices=sorted(bench.WORKLOADS))
    ap.add_argument("--members", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.context()
    ny, nx, nobs, L, swaths, refine = bench.WORKLOADS[args.workload]
    plan = bench.make_plan(ctx, args.workload, 4000)
    plan.run(L, refine=refine, check_pd=True)
    plan.check()
    t0 = time.perf_counter()
    plan.run(L, refine=refine)
    plan.check()
    analysis_s = time.perf_counter() - t0
    plan.posterior_error_mc(nprobe=128)                                        # warm-ups: buffers, code objects
    plan.posterior_ensemble(nmember=max(args.members), nfeature=args.features, keep=False)
    mc_wall, mc_kernels, mc = timed(ctx, lambda: plan.posterior_error_mc(nprobe=256, seed=1), args.reps)
    out = {"workload": args.workload, "cells": plan.n, "observations": plan.m, "features": args.features, "reps": args.reps,
           "device": ctx.device_info()["name"], "analysis_wall_s": analysis_s,
           "mc256_wall_s_median_profiled": mc_wall, "mc256_kernels": mc_kernels, "mc256_median_err_se_over_err": rel_se(mc),
           "ensembles": {}}
    for K in args.members:
        wall, kernels, ens = timed(ctx, lambda: plan.posterior_ensemble(nmember=K, nfeature=args.features, seed=1), args.reps)
        t0 = time.perf_counter()
        plan.posterior_ensemble(nmember=K, nfeature=args.features, seed=1, keep=False)
        t1 = time.perf_counter()
        t_draw = time.perf_counter()
        from oisatgmi import dense
        dense.ensemble_draws("gaussian", L, range(min(K, 128)), args.features, plan.m, 1)
        t_draw = time.perf_counter() - t_draw
        out["ensembles"][str(K)] = {"wall_s_median_profiled_with_readback": wall, "wall_s_unprofiled_keep_false": t1 - t0,
                                    "host_draws_s_per_panel": t_draw, "kernels": kernels,
                                    "median_err_se_over_err": rel_se(ens), "sqrt_1_over_2K": float(np.sqrt(0.5 / K))}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
