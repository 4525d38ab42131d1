"""Measurement (not a gate): superobservations of a FULLY OBSERVED synthetic 720 x 1440 month (1 036 800 observations) at
``--box`` degrees (default 1).  Per repetition behind one warm-up, clocks as found, medians:
  * ``oisat_superob`` on observations already in HBM: the two kernels' own HIP-event times (``oisat_prof_*``) and the wall
    time of the call (it synchronises, copies the sums back and scales them);
  * ``dense.superob``: the same from host arrays (uploads, unit vectors and the merge formulas included);
  * a NumPy restatement of the same reduction on the host (the box rule, then ``np.bincount`` per sum, in floating point);
  * ``dense.OI_dense(superob=box)`` end to end, without the posterior error.
``--plain`` instead runs ``dense.OI_dense`` on the same month WITHOUT superobservations, once, and reports how it ends.

    python tools/superob_timing.py [--box 1.0] [--reps 3] [--plain] [--out FILE.json]
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

from oisatgmi import _hip, dense, synthetic as syn  # noqa: E402

L_KM = 300.0


def month(ny=720, nx=1440, seed=2028):
    rng = np.random.default_rng(seed)
    lat, lon = syn.global_grid(ny, nx)
    xa = syn.background_field(rng, lat, lon)
    err = rng.uniform(0.05, 0.3, xa.shape) * xa
    y = np.maximum(xa * (1.0 + 0.3 * syn._smooth_unit_field(rng, lat, lon)) + err * rng.normal(size=xa.shape), 0.0)
    return lat, lon, xa, y, (0.5 * xa) ** 2, err ** 2


def numpy_reduction(lat, lon, xyz, d, sig, var, table):
    """The box rule and the eight sums in floating point (no fixed point: the fastest honest host form)."""
    n, offset, nbox = table["n"], table["offset"], table["nbox"]
    j = np.minimum(np.floor((lat + 90.0) / table["box_deg"]).astype(np.int64), n.size - 1)
    r = lon / 360.0
    nj = n[j].astype(np.int64)
    box = offset[j] + np.minimum(((r - np.floor(r)) * nj).astype(np.int64), nj - 1)
    w = 1.0 / var
    wd = w * d
    count = np.bincount(box, minlength=nbox)
    sums = [np.bincount(box, weights=t, minlength=nbox) for t in (w, np.sqrt(w), wd, wd * d, w * sig, w * xyz[0], w * xyz[1], w * xyz[2])]
    return count, sums


def timed(fn, reps):
    fn()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append(time.perf_counter() - t0)
    return {"wall_ms_median": 1e3 * float(np.median(walls)), "wall_ms_all": [1e3 * w for w in walls]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c = _hip.context()
    lat2, lon2, xa, y, Sa, So = month()
    lat, lon = lat2.ravel(), lon2.ravel()
    d, sig, var = (y - xa).ravel(), np.sqrt(Sa).ravel(), So.ravel()
    m = int(d.size)
    out = {"grid": list(xa.shape), "observations": m, "box_deg": args.box, "L_km": L_KM, "reps": args.reps,
           "device": c.device_info()["name"]}
    if args.plain:
        t0 = time.perf_counter()
        try:
            dense.OI_dense(xa, y.copy(), Sa, So, lat2, lon2, L_KM, dtype=np.float32)
            out["plain"] = "finished"
        except Exception as e:                                  # noqa: BLE001  (the point is to record how it ends)
            out["plain"] = f"{type(e).__name__}: {e}"
        out["plain_wall_s"] = time.perf_counter() - t0
        out["plain_S_bytes"] = 4 * (-(-m // dense.NB) * dense.NB) ** 2
    else:
        table = dense.superob_boxes(args.box)
        xyz = dense.unit_vectors(lat, lon)
        bufs = [c.upload(a) for a in (lat, lon, xyz, d, sig, var)] + [c.alloc(4 * m)]
        count, sums, used = np.zeros(table["nbox"], dtype=np.int64), np.zeros((8, table["nbox"])), C.c_int64(0)

        def call(with_sums=True):
            c.check(c.lib.oisat_superob(c.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, m,
                                        table["box_deg"], table["n"].ctypes.data, table["offset"].ctypes.data, table["nbands"],
                                        table["nbox"], bufs[6].ptr, count.ctypes.data, sums.ctypes.data if with_sums else None,
                                        C.byref(used)))

        call()
        kernels, walls = [], []
        for _ in range(args.reps):
            c.prof_reset()
            c.prof_enable(True)
            t0 = time.perf_counter()
            call()
            walls.append(time.perf_counter() - t0)
            kernels.append(c.prof_collect())
            c.prof_enable(False)
        out["oisat_superob"] = {"wall_ms_median": 1e3 * float(np.median(walls)), "wall_ms_all": [1e3 * w for w in walls],
                                "kernel_ms_median": {k: float(np.median([r[k]["total_ms"] for r in kernels])) for k in sorted(kernels[0])}}
        out["oisat_superob_counts_only"] = timed(lambda: call(False), args.reps)
        out["superobservations"], out["observations_used"] = int(np.count_nonzero(count)), int(used.value)
        for b in bufs:
            b.free()
        out["dense_superob"] = timed(lambda: dense.superob(lat, lon, d, sig, var, args.box, ctx=c), args.reps)
        out["numpy_reduction"] = timed(lambda: numpy_reduction(lat, lon, xyz, d, sig, var, table), args.reps)
        rc, rs = numpy_reduction(lat, lon, xyz, d, sig, var, table)
        assert np.array_equal(rc, count)
        out["numpy_vs_device_max_rel"] = float(max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(rs, sums)))
        res = {}

        def analyse():
            res["out"] = dense.OI_dense(xa, y.copy(), Sa, So, lat2, lon2, L_KM, dtype=np.float32, superob=args.box)

        out["OI_dense_superob"] = timed(analyse, max(1, args.reps - 1))
        info = res["out"][2]
        out["OI_dense_superob"].update(nobs=info["superob"]["nobs"], residuals=info["residuals"],
                                       increment_finite=bool(np.isfinite(res["out"][1]).all()))
        out["superob_share_of_analysis"] = out["dense_superob"]["wall_ms_median"] / out["OI_dense_superob"]["wall_ms_median"]
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
