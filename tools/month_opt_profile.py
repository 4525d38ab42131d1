"""A month of MOPITT-like or GOSAT-like granules (satellite_opt records) onto the 1.0 degree global grid: the composed
default chain (interpolator_many -> ak_conv, what conv_ak runs -> averaging) against the device-resident month_average.

    python tools/month_opt_profile.py --sensor MOPITT|GOSAT [--types 4,1] [--models 1.0,0.5] [--reps 3] [--out FILE.json]

Synthetic sizes: 16 granules a month, one a day; a granule is a swath of NSCAN x NPIX pixels from 70 S to 70 N, 30 degrees
wide (MOPITT-like: 1500 x 40 = 60,000 pixels, 10 levels, 11 averaging-kernel rows; GOSAT-like: 1000 x 12 = 12,000
pixels, 20 levels with pressure weights).  The model is one float32 ECCOH-style monthly record with 35 levels on a global
grid of ``--models`` degrees: 1.0 is the output grid itself, 0.5 is finer than the 1.0 degree grid, so the regrid stays
on the 1.0 degree grid and the model is upscaled onto it (``ctm_upscaled_needed``).

Reports, per (model, type), seconds per month for both paths (timed alternately, device synchronised before every clock
read), host->device and device->host bytes per granule, the tracemalloc peak of each path and whether the five grids and
avg_datetime are bitwise equal (month_resident_profile.py's counters and timers)."""
import argparse
import copy
import json
import os
import sys
import tracemalloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oi-sat-gmi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import month_resident_profile as mrp  # noqa: E402
from oisatgmi import _ak_conv, _hip, synthetic as syn  # noqa: E402
from oisatgmi.averaging import averaging  # noqa: E402
from oisatgmi.interpolator import interpolator_many  # noqa: E402
from oisatgmi.month import month_average  # noqa: E402

NGRAN = 16
GRID = 1.0
SIZES = {"MOPITT": dict(nscan=1500, npix=40, nz=10), "GOSAT": dict(nscan=1000, npix=12, nz=20)}
MODEL_LEVELS = 35
WINDOW = ("2019-06-01", "2019-07-01")


def make_granules(sensor):
    sz = SIZES[sensor]
    base = syn.swath_level_granule(7100, sensor, nz=sz["nz"], nscan=sz["nscan"], npix=sz["npix"], lat0=-70.0, lat1=70.0,
                                   lon_c=0.0, width_deg=30.0)
    granules = []
    for k in range(NGRAN):
        g = copy.copy(base)
        g.longitude_center = base.longitude_center + (-170.0 + 340.0 * k / NGRAN)
        g.time = base.time.replace(day=1 + k, hour=(3 * k) % 24, minute=k)
        granules.append(g)
    return granules


def make_model(step):
    h = step / 2.0
    ny, nx = int(round(180 / step)), int(round(360 / step))
    ctm = syn.ctm_monthly(ny, nx, MODEL_LEVELS, 1, 11, ctmtype="ECCOH", dtype=np.float32, lat0=-90.0 + h, lat1=90.0 - h,
                          lon0=-180.0 + h, lon1=180.0 - h, year=2019, month0=6)
    return ctm, {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sensor", choices=sorted(SIZES), required=True)
    ap.add_argument("--types", default="4,1")
    ap.add_argument("--models", default="1.0,0.5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sensor = args.sensor
    ctx = _hip.context()
    granules = make_granules(sensor)
    report = {"sensor": sensor, "granules": NGRAN, "pixels": int(granules[0].vcd.size), "levels": SIZES[sensor]["nz"],
              "model_levels": MODEL_LEVELS, "grid_deg": GRID, "device": ctx.device_info()["name"], "legs": {}}

    for step in (float(s) for s in args.models.split(",")):
        ctm, coord = make_model(step)

        def default_chain(itype):
            sat = interpolator_many(itype, GRID, granules, coord, 0.75)
            sat = _ak_conv.ak_conv(ctm, sat, sensor)
            r = mrp._Reader()
            r.sat_data, r.ctm_data = sat, ctm
            return averaging(*WINDOW, r)

        def resident(itype):
            return month_average(*WINDOW, granules, ctm, coord, interpolator_type=itype, grid_size=GRID)

        traffic = mrp.Traffic(ctx)
        for itype in (int(t) for t in args.types.split(",")):
            rec = {"model_deg": step, "model_grid": list(ctm[0].latitude.shape), "type": itype}
            traffic.reset()
            _, res = mrp.timed(ctx, resident, itype)            # warm-up (plans, workers) and traffic
            rec["resident_h2d_bytes_per_granule"] = traffic.h2d / NGRAN
            rec["resident_d2h_bytes_per_granule"] = traffic.d2h / NGRAN
            traffic.reset()
            _, ref = mrp.timed(ctx, default_chain, itype)
            rec["default_h2d_bytes_per_granule"] = traffic.h2d / NGRAN
            rec["default_d2h_bytes_per_granule"] = traffic.d2h / NGRAN
            rec["upscaled"] = bool(step < GRID)
            rec["equal"] = bool(mrp.equal(res, ref))
            t_def, t_res = [], []
            for _ in range(args.reps):
                t_def.append(mrp.timed(ctx, default_chain, itype)[0])
                t_res.append(mrp.timed(ctx, resident, itype)[0])
            rec["default_s_per_month"] = t_def
            rec["resident_s_per_month"] = t_res
            rec["speedup_median"] = float(np.median(t_def) / np.median(t_res))
            for name, fn in (("resident", resident), ("default", default_chain)):
                tracemalloc.start()
                mrp.quiet(fn, itype)
                rec[f"{name}_tracemalloc_peak_bytes"] = tracemalloc.get_traced_memory()[1]
                tracemalloc.stop()
            report["legs"][f"model{step}_type{itype}"] = rec
            print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
