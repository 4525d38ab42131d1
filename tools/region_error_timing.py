"""Measurement (not a gate): what the exact analysis error of regional means costs behind the analysis it belongs to
(``DenseAnalysis.functional_covariance``), on a workload of bench.py (default: the headline synthetic
month).  Two sets of functionals: sixteen 45 x 90 degree boxes, and the single global mean.  Per set, medians over the
repetitions behind one warm-up, clocks as found, each phase enqueued alone and waited for: the gather of G = H B W^T, the gather
of T = B W^T, the K refined solves with their residual evaluations, and the whole method call.  The yardstick for the new
kernel: the same G formed by K calls of ``oisat_apply_increment`` with the roles swapped (float64 fields, the observations as
its "cells", the support as its "observations").

    python tools/region_error_timing.py [--workload config3_720x1440_1e5obs] [--reps 3] [--out FILE.json]
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
from oisatgmi import _hip, dense  # noqa: E402


def box_labels(lat, lon):
    """Sixteen boxes of 45 degrees of latitude by 90 of longitude, labels 1 .. 16."""
    iy = np.clip(np.floor((lat + 90.0) / 45.0).astype(np.int64), 0, 3)
    ix = np.clip(np.floor((np.mod(lon + 180.0, 360.0)) / 90.0).astype(np.int64), 0, 3)
    return iy * 4 + ix + 1


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def phases(plan, W, refine, tol):
    """The method's device phases one by one (the same calls in the same order), each waited for; seconds."""
    c, lib, h = plan.ctx, plan.ctx.lib, plan.ctx.h
    W, sup = plan._functional_support(W)
    K, ns, m, mp, g = W.shape[0], int(sup.size), plan.m, plan.mp, plan._g
    sx, ss, sl, sw = plan._functional_upload(W, sup)
    T = plan._functional_buffer("T", K * ns * 8)
    gyr = plan._functional_buffer("GYR", 3 * K * plan.mp_max * 8)
    G, Y, R = gyr.at(0), gyr.at(K * mp * 8), gyr.at(2 * K * mp * 8)
    c.check(lib.oisat_set_correlation(h, plan._kind))
    out = {"support": ns}
    out["gather_G_s"] = timed(c, lambda: c.check(lib.oisat_functional_gather(
        h, plan.oxyz.ptr, plan.osig.ptr, plan.olat.ptr, m, sx.ptr, ss.ptr, sl.ptr, ns, sw.ptr, K, ns, g, G, mp)))
    out["gather_T_s"] = timed(c, lambda: c.check(lib.oisat_functional_gather(
        h, sx.ptr, ss.ptr, sl.ptr, ns, sx.ptr, ss.ptr, sl.ptr, ns, sw.ptr, K, ns, g, T.ptr, ns)))

    def solves():
        for k in range(K):
            gk, yk, rk = G + k * mp * 8, Y + k * mp * 8, R + k * mp * 8
            c.check(lib.oisat_set_refine_tol(h, tol))
            c.check(lib.oisat_set_obs_blocks(h, plan.perm.ptr, m))
            c.check(lib.oisat_gain_solve(h, plan.S.ptr, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, mp, g, gk, refine, yk, None,
                                         plan.olat.ptr))
            c.check(lib.oisat_cov_residual(h, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, g, gk, yk, rk, plan.olat.ptr))
    out["solves_and_residuals_s"] = timed(c, solves)

    # the yardstick: G by K swapped calls of the increment (float64: inc = "sigma_cell sum C sigma_obs z")
    def swapped():
        for k in range(K):
            c.check(lib.oisat_apply_increment(h, _hip.F64, plan.oxyz.ptr, plan.osig.ptr, m, sx.ptr, ss.ptr, sw.at(k * ns * 8), ns, g, None,
                                              None, Y + k * mp * 8, plan.olat.ptr, sl.ptr))
    out["gather_G_by_swapped_increments_s"] = timed(c, swapped)
    got = c.download(Y, (K, mp), np.float64)[:, :m]
    want = c.download(G, (K, mp), np.float64)[:, :m]
    out["swapped_vs_gather_max_rel"] = float(np.abs(got - want).max() / np.abs(want).max())
    plan.check()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=bench.DEFAULT, choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--refine", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.context()
    ny, nx, nobs, L, swaths, refine = bench.WORKLOADS[args.workload]
    plan = bench.make_plan(ctx, args.workload, 4000)
    plan.run(L, refine=refine, check_pd=True)
    plan.check()
    analysis_s = timed(ctx, lambda: (plan.run(L, refine=refine), plan.check()))
    lat = plan._glat_host.reshape(plan.shape)
    lon = plan._glon_host.reshape(plan.shape)
    sets = {"boxes16": dense.region_weights(box_labels(lat, lon), lat)[1],
            "global1": dense.region_weights(np.ones(lat.shape, dtype=np.int64), lat)[1]}
    out = {"workload": args.workload, "cells": plan.n, "observations": plan.m, "L_km": L, "reps": args.reps, "refine": args.refine,
           "tol": dense.REFINE_TOL, "device": ctx.device_info()["name"], "analysis_wall_s": analysis_s, "sets": {}}
    for name, W in sets.items():
        res = plan.functional_covariance(W, refine=args.refine)                # warm-up: buffers, code objects
        runs, walls = [], []
        for _ in range(args.reps):
            walls.append(timed(ctx, lambda: plan.functional_covariance(W, refine=args.refine)))
            runs.append(phases(plan, W, args.refine, dense.REFINE_TOL))
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        med["support"] = int(med["support"])
        out["sets"][name] = {"K": int(W.shape[0]), "total_wall_s_median": float(np.median(walls)), **med,
                             "resid_max": float(res["resid"].max()),
                             "posterior_sd_over_prior_sd": (np.sqrt(np.diag(res["posterior"]) / np.diag(res["prior"]))).round(4).tolist()}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
