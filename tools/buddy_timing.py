"""Measurement (not a gate): one ``oisat_buddy_sums`` call on the observations of a workload of bench.py (default: the headline
synthetic month, L = 300 km) at the default cut ``dense.BUDDY_CMIN``, next to ``oisat_covariogram`` on the same observations
with ``max_km`` = the buddy radius (the chord at which the correlation has fallen to the cut) -- existing code of the same shape,
the yardstick.  The observations are uploaded once, in ascending latitude; per call the host wall time to the end of a stream
synchronise and the kernel's own HIP-event time (``oisat_prof_*``), medians over the repetitions behind one warm-up, clocks as
found.  Also counted on the device's results: pairs that contribute (sum of n), for the time per pair.

    python tools/buddy_timing.py [--workload config3_720x1440_1e5obs] [--corr gaussian] [--reps 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oi-sat-gmi_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
from oisatgmi import _hip, dense  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=bench.DEFAULT, choices=sorted(bench.WORKLOADS))
    ap.add_argument("--corr", default="gaussian", choices=sorted(dense.CORRELATIONS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c = _hip.context()
    L = bench.WORKLOADS[args.workload][3]
    p, cell, _, _ = bench.build_case(args.workload, 4000)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    u = (y - np.ravel(p.Xa)[cell]) / np.sqrt(np.ravel(p.Sa)[cell] + p.obs_var)
    m = int(u.size)
    kind, g, cmin = dense.corr_kind(args.corr), dense.decay_constant(L), dense.BUDDY_CMIN
    chord = C.c_double(0.0)
    c.check(c.lib.oisat_corr_cut_chord(kind, g, -math.log2(cmin), C.byref(chord)))
    o = dense.latitude_order(p.obs_lat)
    oxyz, du, olat = c.upload(dense.unit_vectors(p.obs_lat[o], p.obs_lon[o])), c.upload(u[o]), c.upload(p.obs_lat[o])
    n_dev, s_dev = c.alloc(4 * m), c.alloc(24 * m)
    nbins = 64
    count, sp, sc = np.zeros(nbins, dtype=np.int64), np.zeros(nbins), np.zeros(nbins)
    used = C.c_int64(0)

    def buddy():
        c.check(c.lib.oisat_buddy_sums(c.h, oxyz.ptr, du.ptr, m, g, cmin, olat.ptr, n_dev.ptr, s_dev.ptr))
        c.sync()

    def covariogram():
        c.check(c.lib.oisat_covariogram(c.h, oxyz.ptr, du.ptr, None, m, chord.value, nbins, olat.ptr, count.ctypes.data,
                                        sp.ctypes.data, sc.ctypes.data, C.byref(used)))

    c.check(c.lib.oisat_set_correlation(c.h, kind))
    out = {"workload": args.workload, "observations": m, "L_km": L, "corr": args.corr, "cmin": cmin,
           "buddy_radius_km": chord.value * dense.EARTH_RADIUS_KM, "reps": args.reps, "device": c.device_info()["name"]}
    try:
        for name, fn in (("buddy_sums", buddy), ("covariogram", covariogram)):
            fn()                                                # warm-up: code objects, the covariogram's workspace
            walls, kernels = [], []
            for _ in range(args.reps):
                c.prof_reset()
                c.prof_enable(True)
                t0 = time.perf_counter()
                fn()
                walls.append(time.perf_counter() - t0)
                kernels.append(c.prof_collect())
                c.prof_enable(False)
            out[name] = {"wall_ms_median": 1e3 * float(np.median(walls)), "wall_ms_all": [1e3 * w for w in walls],
                         "kernel_ms_median": {k: float(np.median([r[k]["total_ms"] for r in kernels])) for k in sorted(kernels[0])}}
    finally:
        c.check(c.lib.oisat_set_correlation(c.h, dense.CORRELATIONS["gaussian"]))
    n = c.download(n_dev.ptr, (m,), np.int32)
    out["buddy_pairs_contributing"] = int(n.astype(np.int64).sum())
    out["buddies_per_observation_mean"] = float(n.mean())
    out["covariogram_pairs_binned"] = int(count.sum())
    out["wall_ratio_buddy_over_covariogram"] = out["buddy_sums"]["wall_ms_median"] / out["covariogram"]["wall_ms_median"]
    for b in (oxyz, du, olat, n_dev, s_dev):
        b.free()
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
