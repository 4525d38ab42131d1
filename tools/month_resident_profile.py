"""A month of 32 OMI-like granules (98,640 pixels, 35 scattering-weight + 35 pressure levels, tropopause) onto the 0.25
degree global grid: the composed default chain (interpolator_many -> amf_recal -> averaging) against the device-resident
month_average, types 4 and 1.

    python tools/month_resident_profile.py [--types 4,1] [--reps 2] [--only resident] [--out FILE.json]

Reports seconds per month for both paths (timed alternately, device synchronised before every clock read), host->device
and device->host bytes per granule (the context's upload / upload_into / download wrapped), the tracemalloc peak of each
path, the process's peak RSS, and whether the five grids and avg_datetime are bitwise equal.  ``--only resident`` runs
the resident path once per type and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import contextlib
import copy
import io
import json
import os
import resource
import sys
import time
import tracemalloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oi-sat-gmi_amd"))

import numpy as np  # noqa: E402

from oisatgmi import _hip, synthetic as syn  # noqa: E402
from oisatgmi.amf_recal import amf_recal  # noqa: E402
from oisatgmi.averaging import averaging  # noqa: E402
from oisatgmi.interpolator import interpolator_many  # noqa: E402
from oisatgmi.month import month_average  # noqa: E402

NZ = 35
NGRAN = 32


class _Reader:
    pass


def make_inputs():
    base = syn.swath_granule(7007, nscan=1644, npix=60, lat0=-70.0, lat1=70.0, lon_c=0.0, width_deg=24.0)
    rng = np.random.default_rng(5)
    shape = base.vcd.shape
    base.scattering_weights = rng.uniform(0.1, 2.0, size=(NZ,) + shape).astype(np.float32)
    base.pressure_mid = (np.linspace(1000.0, 60.0, NZ)[:, None, None] * rng.uniform(0.98, 1.02, size=(NZ,) + shape)).astype(np.float32)
    base.tropopause = rng.uniform(90.0, 250.0, size=shape)
    granules = []
    for k in range(NGRAN):
        g = copy.copy(base)
        g.longitude_center = base.longitude_center + (-170.0 + 340.0 * k / NGRAN)
        g.time = base.time.replace(day=1 + k % 28, hour=(3 * k) % 24, minute=k)
        granules.append(g)
    # the model on the same 0.25 degree global grid, float32 as the readers hand it over: one day of 8 slots
    ctm = syn.ctm_days(720, 1440, 10, 1, 11, averaged=False, dtype=np.float32, lat0=-89.875, lat1=89.875, lon0=-179.875,
                       lon1=179.875, year=base.time.year, month=base.time.month)
    coord = {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}
    return granules, ctm, coord


class Traffic:
    """Counts the bytes through the process-wide context's copy entry points."""

    def __init__(self, ctx):
        self.h2d = self.d2h = 0
        up, upi, down = ctx.upload, ctx.upload_into, ctx.download

        def upload(arr, dtype=None):
            self.h2d += np.asarray(arr).size * np.dtype(dtype if dtype is not None else np.asarray(arr).dtype).itemsize
            return up(arr, dtype)

        def upload_into(ptr, arr, dtype=None):
            n = upi(ptr, arr, dtype)
            self.h2d += n
            return n

        def download(ptr, shape, dtype):
            out = down(ptr, shape, dtype)
            self.d2h += out.nbytes
            return out
        ctx.upload, ctx.upload_into, ctx.download = upload, upload_into, download

    def reset(self):
        self.h2d = self.d2h = 0


def default_chain(itype, granules, ctm, coord):
    sat = interpolator_many(itype, 0.25, granules, coord, 0.75)
    sat = amf_recal(ctm, sat)
    r = _Reader()
    r.sat_data, r.ctm_data = sat, ctm
    return averaging("2019-06-01", "2019-07-01", r)


def resident(itype, granules, ctm, coord):
    return month_average("2019-06-01", "2019-07-01", granules, ctm, coord, interpolator_type=itype, grid_size=0.25)


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def timed(ctx, fn, *a):
    ctx.sync()
    t0 = time.perf_counter()
    out = quiet(fn, *a)
    ctx.sync()
    return time.perf_counter() - t0, out


def equal(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="4,1")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", choices=["resident"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.context()
    granules, ctm, coord = make_inputs()
    report = {"granules": NGRAN, "pixels": int(granules[0].vcd.size), "levels": NZ, "grid": list(ctm[0].latitude.shape),
              "device": ctx.device_info()["name"], "types": {}}
    if args.only == "resident":
        for itype in (int(t) for t in args.types.split(",")):
            s, _ = timed(ctx, resident, itype, granules, ctm, coord)
            report["types"][str(itype)] = {"resident_s": s}
            print(json.dumps(report["types"][str(itype)]), flush=True)
        return
    traffic = Traffic(ctx)
    for itype in (int(t) for t in args.types.split(",")):
        rec = {}
        traffic.reset()
        s, res = timed(ctx, resident, itype, granules, ctm, coord)        # warm-up (plans, workers) and traffic
        rec["resident_h2d_bytes_per_granule"] = traffic.h2d / NGRAN
        rec["resident_d2h_bytes_per_granule"] = traffic.d2h / NGRAN
        rss_after_resident = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
        traffic.reset()
        s, ref = timed(ctx, default_chain, itype, granules, ctm, coord)
        rec["default_h2d_bytes_per_granule"] = traffic.h2d / NGRAN
        rec["default_d2h_bytes_per_granule"] = traffic.d2h / NGRAN
        rec["equal"] = bool(equal(res, ref))
        t_def, t_res = [], []
        for _ in range(args.reps):
            t_def.append(timed(ctx, default_chain, itype, granules, ctm, coord)[0])
            t_res.append(timed(ctx, resident, itype, granules, ctm, coord)[0])
        rec["default_s_per_month"] = t_def
        rec["resident_s_per_month"] = t_res
        rec["speedup_median"] = float(np.median(t_def) / np.median(t_res))
        for name, fn in (("resident", resident), ("default", default_chain)):
            tracemalloc.start()
            quiet(fn, itype, granules, ctm, coord)
            rec[f"{name}_tracemalloc_peak_bytes"] = tracemalloc.get_traced_memory()[1]
            tracemalloc.stop()
        rec["peak_rss_bytes_after_first_resident"] = rss_after_resident
        rec["peak_rss_bytes"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
        report["types"][str(itype)] = rec
        print(json.dumps({itype: rec}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
