"""Measurement (not a gate): what the randomized analysis error costs next to the analysis it belongs to, and next to the exact
``oisat_posterior_error`` it replaces.  Per-kernel HIP-event times (``oisat_prof_*``) of ``posterior_error_mc`` at K probes on
a workload of bench.py (default: the headline synthetic month), medians over the repetitions behind one warm-up, clocks as
found; the exact error is timed on a slab of 4 096 cells of the same factor and scaled by n / 4 096.

    python tools/mc_error_timing.py [--workload config3_720x1440_1e5obs] [--nprobe 256] [--reps 3] [--out FILE.json]
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

SLAB = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=bench.DEFAULT, choices=sorted(bench.WORKLOADS))
    ap.add_argument("--nprobe", type=int, default=256)
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
    plan.posterior_error_mc(nprobe=128)                                        # warm-up: buffers, code objects
    walls, kernels = [], []
    for _ in range(args.reps):
        ctx.prof_reset()
        ctx.prof_enable(True)
        t0 = time.perf_counter()
        est = plan.posterior_error_mc(nprobe=args.nprobe, seed=1)
        walls.append(time.perf_counter() - t0)
        kernels.append(ctx.prof_collect())
        ctx.prof_enable(False)
    names = sorted(kernels[0])
    per_kernel = {k: {"launches": kernels[0][k]["launches"], "median_ms": float(np.median([r[k]["total_ms"] for r in kernels]))}
                  for k in names}
    t0 = time.perf_counter()
    plan.posterior_error_mc(nprobe=args.nprobe, seed=1)
    wall_mc_unprofiled = time.perf_counter() - t0
    # the exact error of the same factor on one slab of cells (the middle of the grid), scaled to every cell
    c, slab = ctx, min(SLAB, plan.n)
    i0 = (plan.n - slab) // 2
    err = c.alloc(slab * 4)
    exact = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        c.check(c.lib.oisat_posterior_error(c.h, plan.S.ptr, plan.m, plan.mp, plan.gxyz.ptr, plan.gsig.ptr, plan.n, i0, i0 + slab,
                                            plan.oxyz.ptr, plan.osig.ptr, plan._g, slab, err.ptr))
        c.sync()
        exact.append(time.perf_counter() - t0)
    exact_slab = float(np.median(exact[1:]))
    # ... and, while it is there, the estimate against it on that slab in units of its own standard error (float32 reference:
    # 2^-23 sig^2 of rounding in its square; fp32 solves on both sides: 2^-16 of q)
    sig2 = np.asarray(plan._gsig_host, dtype=np.float64)[i0:i0 + slab] ** 2
    q_exact = sig2 - c.download(err.ptr, (slab,), np.float32).astype(np.float64) ** 2
    q_hat, q_se = np.ravel(est["q"])[i0:i0 + slab], np.ravel(est["q_se"])[i0:i0 + slab]
    dev = np.maximum(np.abs(q_hat - q_exact) - 2.0 ** -23 * sig2 - 2.0 ** -16 * q_hat, 0.0)
    zscore = np.where(q_se > 0, dev / np.where(q_se > 0, q_se, 1.0), np.where(dev > 0, np.inf, 0.0))
    se_rel = np.sqrt(2.0 / args.nprobe)
    err64 = est["err"].astype(np.float64)
    rel = np.where(err64 > 0, est["err_se"] / np.where(err64 > 0, err64, 1.0), np.nan)       # (clipped cells report no error)
    out = {"workload": args.workload, "cells": plan.n, "observations": plan.m, "nprobe": args.nprobe, "reps": args.reps,
           "device": ctx.device_info()["name"], "analysis_wall_s": analysis_s,
           "mc_wall_s_median_profiled": float(np.median(walls)), "mc_wall_s_unprofiled": wall_mc_unprofiled, "mc_kernels": per_kernel,
           "exact_slab_cells": slab, "exact_slab_wall_s_median": exact_slab, "exact_scaled_to_all_cells_s": exact_slab * plan.n / slab,
           "noise_bound_relative_to_reduction": float(se_rel), "median_err_se_over_err": float(np.nanmedian(rel)),
           "slab_worst_deviation_in_se": float(zscore.max()), "slab_fraction_beyond_3_se": float((zscore > 3).mean()),
           "slab_median_q_over_sig2": float(np.median(q_exact / np.where(sig2 > 0, sig2, 1.0)))}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
