"""Measurement (not a gate): what the innovations' likelihood and the maximum-likelihood error scales cost, and how far the fp32
factor's log-determinant is from float64 (``DenseAnalysis.log_likelihood`` / ``fit_error_scales``), on
the workloads of bench.py.  Clocks as found, every phase enqueued alone and waited for.

  * ``--accuracy`` (default: config 2, 360 x 720 / 10^4 observations): |logdet_dev - logdet_64| with logdet_64 from a float64
    SciPy Cholesky of the same S on the host, once.
  * ``--timing`` (default: the headline month, config 3): ``run()`` as every analysis runs it; ``run(exact_factor=True)`` (what
    the 2^-52 envelope costs against the factor's own cut); one evaluation of the search, ``run(fields=False,
    exact_factor=True, check_pd=True)`` + ``log_likelihood()``; the kernel time of ``oisat_factor_logdet`` beside the
    factorization launch of the same run (HIP events); a whole ``fit_error_scales``; and the same fit on the month's
    superobservations over ``--box`` degrees.

    python tools/likelihood_timing.py [--accuracy config2_360x720_1e4obs] [--timing config3_720x1440_1e5obs] [--box 1.0] [--out FILE.json]
    (an empty string skips a part)
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


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def accuracy(ctx, workload):
    """The device's log-determinant against a float64 Cholesky of the same S (the plan's own sigma_b and variances)."""
    import scipy.linalg as sla
    ny, nx, nobs, L, swaths, refine = bench.WORKLOADS[workload]
    plan = bench.make_plan(ctx, workload, 4000)
    resid = plan.run(L, refine=refine, check_pd=True, want_resid=True, exact_factor=True)
    lik = plan.log_likelihood()
    m = plan.m
    oxyz = ctx.download(plan.oxyz.ptr, (3, m), np.float64)
    S = np.zeros((m, m))
    for k in range(3):
        S += (oxyz[k][:, None] - oxyz[k][None, :]) ** 2
    S *= -dense.decay_constant(L)
    np.exp(S, out=S)
    S *= plan._osig0[:, None]
    S *= plan._osig0[None, :]
    S[np.diag_indices_from(S)] += plan._ovar0
    d = ctx.download(plan.d.ptr, (m,), np.float64)
    say(f"accuracy: float64 Cholesky of {m} x {m} on the host ...")
    cho = sla.cho_factor(S, lower=True, overwrite_a=True, check_finite=False)
    logdet64 = 2.0 * float(np.log(np.diag(cho[0])).sum())
    chi2_64 = float(d @ sla.cho_solve(cho, d, check_finite=False))
    return {"workload": workload, "observations": m, "L_km": L, "logdet_dev": lik["logdet"], "logdet_64": logdet64,
            "abs_logdet_error": abs(lik["logdet"] - logdet64), "chi2_dev": lik["chi2"], "chi2_64": chi2_64,
            "abs_chi2_error": abs(lik["chi2"] - chi2_64), "resid": resid[-1], "min_pivot": lik["min_pivot"]}


def fit_timed(ctx, plan, L, refine):
    ctx.sync()
    t0 = time.perf_counter()
    fit = plan.fit_error_scales(L, refine=refine)
    ctx.sync()
    return {"observations": plan.m, "fit_wall_s": time.perf_counter() - t0, "nevals": fit["nevals"], "scale_b": fit["scale_b"],
            "se_ln": fit["se_ln"], "found": fit["found"], "at_bound": fit["at_bound"],
            "failed_evaluations": sum(1 for _, J in fit["evaluations"] if not np.isfinite(J)),
            # (strict JSON has no Infinity / NaN: a failed evaluation is written as null)
            "evaluations": [[x, J if np.isfinite(J) else None] for x, J in fit["evaluations"]],
            "residuals": [r if np.isfinite(r) else None for r in fit["residuals"]], "likelihood": fit["likelihood"]}


def timing(ctx, workload, box, reps):
    ny, nx, nobs, L, swaths, refine = bench.WORKLOADS[workload]
    p, cell, lat2, lon2 = bench.build_case(workload, 4000)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = dense.DenseAnalysis(lat2, lon2, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    out = {"workload": workload, "cells": plan.n, "observations": plan.m, "L_km": L, "refine": refine, "reps": reps}

    def median(fn):
        fn()                                                       # warm-up: tables, plans, code objects
        return float(np.median([timed(ctx, fn) for _ in range(reps)]))

    say("timing: run() ...")
    out["run_default_s"] = median(lambda: (plan.run(L, refine=refine), plan.check()))
    say("timing: run(exact_factor=True) ...")
    out["run_exact_factor_s"] = median(lambda: (plan.run(L, refine=refine, exact_factor=True), plan.check()))
    say("timing: one evaluation ...")
    out["evaluation_s"] = median(lambda: (plan.run(L, refine=refine, check_pd=True, fields=False, exact_factor=True), plan.log_likelihood()))
    ctx.prof_reset()
    ctx.prof_enable(True)
    plan.run(L, refine=refine, check_pd=True, fields=False, exact_factor=True)
    out["likelihood_at_scale_1"] = plan.log_likelihood()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    out["kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])}
    say("timing: the whole fit ...")
    out["fit"] = fit_timed(ctx, plan, L, refine)
    del plan
    if box:
        say(f"timing: the fit on the superobservations over {box} degrees ...")
        xb = np.ravel(p.Xa).astype(np.float32).astype(np.float64)
        so = dense.superob(p.obs_lat, p.obs_lon, np.asarray(y, dtype=np.float64) - xb[cell],
                           np.sqrt(np.ravel(np.asarray(p.Sa, dtype=np.float64)))[cell], p.obs_var, box, ctx=ctx)
        plan = dense.DenseAnalysis(lat2, lon2, max_obs=int(so["nobs"]), dtype=np.float32, ctx=ctx)
        plan.load_background(p.Xa, p.Sa)
        plan.load_obs_direct(so["lat"], so["lon"], so["sigma_b"], so["var"], so["d"])
        plan.run(L, refine=refine, check_pd=True, exact_factor=True)
        plan.check()
        out["fit_superob"] = {"box_deg": box, **fit_timed(ctx, plan, L, refine)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", default=bench.SECONDARY)
    ap.add_argument("--timing", default=bench.DEFAULT)
    ap.add_argument("--box", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.context()
    out = {"device": ctx.device_info()["name"], "tol": dense.REFINE_TOL}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1, allow_nan=False)
                f.write("\n")

    if args.accuracy:
        out["accuracy"] = accuracy(ctx, args.accuracy)
        say(json.dumps(out["accuracy"]))
        save()
    if args.timing:
        out["timing"] = timing(ctx, args.timing, args.box, args.reps)
    save()
    print(json.dumps(out, indent=1, allow_nan=False))


if __name__ == "__main__":
    main()
