"""Measurement (not a gate): what the drift of the innovations costs and what it is for (``DenseAnalysis.run(drift=...)``,
DESIGN.md section 4.2k), on the headline month of bench.py.  Clocks as found; every timed call is enqueued alone and waited for,
after a warm-up, and the figure is the median of ``--reps`` runs; the two routes of the block solve are timed by turns.

  * ``solve``: ``oisat_gain_solve_multi`` on [d | F] (degree 3: 17 columns) against 17 consecutive ``oisat_gain_solve`` calls on
    the same factor -- the looped route is made of the parent's own entry points -- with the largest difference between the two
    solutions, and the block residual alone against 17 single residuals.
  * ``variance``: ``drift_variance()`` behind ``run(drift=3)``; ``run()`` with and without ``drift=1`` / ``drift=3``.
  * ``bias``: the month's innovations plus a degree-1 pattern of the size of the background error: chi2 / m and the scale
    ``fit_error_scales`` fits, without the bias, with it, and with it under ``drift=1`` (for the fit behind a drift F beta is
    subtracted from the innovations by hand: the two are not combined).

    python tools/drift_timing.py [--workload config3_720x1440_1e5obs] [--reps 5] [--skip-bias] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oi-sat-gmi_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
from oisatgmi import _hip, dense  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def by_turns(ctx, fns, reps):
    """Median wall time of each of ``fns``, one warm-up each, then ``reps`` rounds that run them one after the other."""
    for fn in fns:
        fn()
    ctx.sync()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(timed(ctx, fn))
    return [float(np.median(x)) for x in t], [[float(v) for v in x] for x in t]


def solve_part(ctx, plan, L, refine, reps):
    lib, h = ctx.lib, ctx.h
    nr = 17
    plan.run(L, refine=refine)                                     # the factor every solve below reads
    plan.check()
    m, ld, g = plan.m, plan.mp, plan._g
    blk = ctx.alloc((3 * nr * ld) * 8)
    D, Z, Z1 = blk.at(0), blk.at(nr * ld * 8), blk.at(2 * nr * ld * 8)
    f64 = _hip.dtype_code(np.dtype(np.float64))
    ctx.check(lib.oisat_affine(h, f64, plan.d.ptr, m, 0.0, 1.0, D))
    ctx.check(lib.oisat_drift_basis(h, plan.oxyz.ptr, m, 3, D + ld * 8, ld))
    ctx.check(lib.oisat_set_correlation(h, plan._kind))
    ctx.check(lib.oisat_set_refine_tol(h, dense.REFINE_TOL))
    resid = (C.c_double * ((refine + 1) * nr))()

    def multi(report):
        ctx.check(lib.oisat_set_obs_blocks(h, plan.perm.ptr, m))
        ctx.check(lib.oisat_gain_solve_multi(h, plan.S.ptr, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, ld, g, D, nr, ld, refine, Z,
                                             resid if report else None, plan.olat.ptr))

    def looped():
        for k in range(nr):
            ctx.check(lib.oisat_set_obs_blocks(h, plan.perm.ptr, m))
            ctx.check(lib.oisat_gain_solve(h, plan.S.ptr, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, ld, g, D + k * ld * 8, refine,
                                           Z1 + k * ld * 8, None, plan.olat.ptr))

    def resid_multi():
        ctx.check(lib.oisat_set_obs_blocks(h, plan.perm.ptr, m))
        ctx.check(lib.oisat_cov_residual_multi(h, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, g, D, Z, Z1, nr, ld, plan.olat.ptr))

    def resid_looped():
        for k in range(nr):
            ctx.check(lib.oisat_set_obs_blocks(h, plan.perm.ptr, m))
            ctx.check(lib.oisat_cov_residual(h, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, g, D + k * ld * 8, Z + k * ld * 8,
                                             Z1 + k * ld * 8, plan.olat.ptr))

    say("solve: the block solve against 17 single solves ...")
    (t_multi, t_poll, t_loop), raw = by_turns(ctx, [lambda: multi(False), lambda: multi(True), looped], reps)
    multi(True)
    res = np.array(resid).reshape(refine + 1, nr)
    looped()
    plan.check()
    zm = ctx.download(Z, (nr, ld), np.float64)[:, :m]
    zl = ctx.download(Z1, (nr, ld), np.float64)[:, :m]
    rel = [float(np.linalg.norm(zm[k] - zl[k]) / np.linalg.norm(zl[k])) for k in range(nr)]
    say("solve: the block residual against 17 single residuals ...")
    (t_rm, t_rl), raw_r = by_turns(ctx, [resid_multi, resid_looped], reps)
    ctx.prof_reset()
    ctx.prof_enable(True)
    multi(True)
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    return {"columns": nr, "refine": refine, "gain_solve_multi_enqueue_all_s": t_multi, "gain_solve_multi_polling_s": t_poll,
            "gain_solve_looped_s": t_loop, "raw_s": raw, "relative_residuals_per_round": res.tolist(),
            "largest_relative_difference_multi_vs_looped": max(rel), "cov_residual_multi_s": t_rm, "cov_residual_looped_s": t_rl,
            "raw_residual_s": raw_r,
            "kernels_ms_of_one_polling_solve": {k: round(v["total_ms"], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])}}


def variance_part(ctx, plan, L, refine, reps):
    out = {}
    say("variance: run() with and without a drift ...")
    (out["run_s"], out["run_drift1_s"], out["run_drift3_s"]), _ = by_turns(
        ctx, [lambda: (plan.run(L, refine=refine), plan.check()), lambda: (plan.run(L, refine=refine, drift=1), plan.check()),
              lambda: (plan.run(L, refine=refine, drift=3), plan.check())], reps)
    plan.run(L, refine=refine, drift=3)
    plan.check()
    est = plan.drift_estimate()
    out["drift3"] = {"cond": est["cond"], "resid_max": float(est["resid"].max()), "beta": est["beta"].tolist(), "beta_se": est["beta_se"].tolist()}
    say("variance: drift_variance() ...")
    (out["drift_variance_degree3_s"],), _ = by_turns(ctx, [plan.drift_variance], reps)
    var = plan.drift_variance()
    out["drift_variance_degree3_max_over_prior_variance"] = float(np.nanmax(var.ravel() / np.where(plan._gsig_host > 0, plan._gsig_host ** 2, np.nan)))
    return out


def bias_part(ctx, plan, L, refine):
    """chi2 / m and the fitted background scale: the month as it is, with a degree-1 bias, and with the bias under drift=1."""
    m = plan.m
    lat = plan._lat_sorted.copy()
    oxyz = ctx.download(plan.oxyz.ptr, (3, m), np.float64)
    lon = np.degrees(np.arctan2(oxyz[1], oxyz[0]))
    plan.run(L, refine=refine)
    plan.check()
    d0 = ctx.download(plan.d.ptr, (m,), np.float64)
    sig, var = plan._osig0.copy(), plan._ovar0.copy()
    amp = float(np.median(sig))
    beta_true = amp * np.array([1.0, 0.0, 0.0, 1.0])               # low everywhere, twice as low at the north pole, right at the south
    F = np.array([np.ones(m), oxyz[0], oxyz[1], oxyz[2]]).T
    out = {"bias_beta": beta_true.tolist(), "median_sigma_b": amp}

    def analyse(d, drift):
        plan.load_obs_direct(lat, lon, sig, var, d)
        plan.run(L, refine=refine, check_pd=True, exact_factor=True, drift=drift)
        lik = plan.log_likelihood()
        rec = {"chi2_per_obs": lik["chi2_per_obs"]}
        if drift is not None:
            est = plan.drift_estimate()
            rec.update(beta=est["beta"].tolist(), beta_se=est["beta_se"].tolist(), cond=est["cond"])
            plan.load_obs_direct(lat, lon, sig, var, d - F[:, :est["beta"].size] @ est["beta"])       # by hand: drift and fit are not combined
        fit = plan.fit_error_scales(L, refine=refine, want_se=False, fields=False)
        rec.update(fitted_scale_b=fit["scale_b"], fit_found=fit["found"], fit_nevals=fit["nevals"],
                   chi2_per_obs_at_the_fit=fit["likelihood"]["chi2_per_obs"])
        return rec

    say("bias: the month as it is ...")
    out["as_it_is"] = analyse(d0, None)
    say("bias: with the degree-1 bias ...")
    out["biased"] = analyse(d0 + F @ beta_true, None)
    say("bias: with the bias, drift=1 ...")
    out["biased_drift1"] = analyse(d0 + F @ beta_true, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=bench.DEFAULT)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-bias", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.context()
    ny, nx, nobs, L, swaths, refine = bench.WORKLOADS[args.workload]
    plan = bench.make_plan(ctx, args.workload, 4000)
    out = {"device": ctx.device_info()["name"], "workload": args.workload, "cells": plan.n, "observations": plan.m, "L_km": L,
           "tol": dense.REFINE_TOL, "reps": args.reps, "clocks": "as found"}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1, allow_nan=False)
                f.write("\n")

    out["solve"] = solve_part(ctx, plan, L, refine, args.reps)
    say(json.dumps({k: v for k, v in out["solve"].items() if not k.startswith("raw")}))
    save()
    out["variance"] = variance_part(ctx, plan, L, refine, args.reps)
    say(json.dumps(out["variance"]))
    save()
    if not args.skip_bias:
        out["bias"] = bias_part(ctx, plan, L, refine)
        save()
    print(json.dumps(out, indent=1, allow_nan=False))


if __name__ == "__main__":
    main()
