"""A month of raw L2 granules to monthly means without leaving HBM.

``month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, ...)`` returns what

    sat = interpolator_many(interpolator_type, grid_size, granules, ctm_models_coordinate, flag_thresh)
    sat = amf_recal(ctm_data, sat)                 # satellite_amf records
    sat = _ak_conv.ak_conv(ctm_data, sat, S)       # satellite_opt records of sensor S: what conv_ak(S) runs
    reader.sat_data, reader.ctm_data = sat, ctm_data
    averaging(startdate, enddate, reader)

returns, bit for bit, but every granule's regridded fields stay on the device: the regrid output feeds the AMF
recalculation (``oisat_amf_recal``) or the averaging-kernel convolution (``oisat_ak_conv_mopitt`` / ``_gosat``) in
place, and the averaged fields are folded into running per-cell (sum, count) accumulators (``oisat_month_accumulate``)
in the order ``averaging()`` would stack them.  The read-backs are the finished monthly
grids and one int32 "kept" word per granule (``oisat_all_nan``: the device form of the interpolator's all-NaN skip
test), read once per month.  Host memory no longer grows with the number of granules.

Why the bits agree: the regrid and the AMF kernels are the same launches on the same device data; the square root of
the regridded variance is ``oisat_sqrt`` (correctly rounded, as ``np.sqrt``); float32 -> float64 widening is exact and
float64 -> float32 narrowing rounds to nearest-even on both sides; the accumulators add granule by granule in the
stack order from zero, as ``stack_reduce_kernel`` does, and close with the same ``finish``.

Covered, interpolator types 1-4: ``satellite_amf`` granules with scattering weights (averaged fields vcd, uncertainty,
ctm_vcd, new_amf, old_amf) and ``satellite_opt`` granules of one sensor, MOPITT or GOSAT (vcd, uncertainty, ctm_vcd, x_col,
ctm_xcol; GOSAT's ctm_vcd is all NaN).  Anything else is refused with ``NotImplementedError`` before the device is touched
(lists that mix the two record types or the two sensors; SSMIS has its own pre-gridder; without scattering weights the
default chain averages an ``np.empty((1))`` placeholder).
"""
from __future__ import annotations

import datetime

import numpy as np

from . import _hip
from . import _ak_conv
from .amf_recal import (_closest_slot, _model_slot, _model_times, _partial_column_device, _partial_column_dtype,
                        _recal_granule, _sat_grid_upscale_plan)
from .averaging import _window
from .config import satellite_amf, satellite_opt, satellite_ssmis
from .interpolator import _GranuleRegridder, _opt_check, _opt_fields, _regrid_dtype, _with_triangulations

_NFIELDS = 5                 # vcd, uncertainty, ctm_vcd, aux1, aux2 (csrc/averaging.hip, oisat_month_accumulate)


def _refuse(granules):
    """NotImplementedError for every input the resident path does not reproduce (before any device work).  -> the record
    type of the list (``satellite_amf`` or ``satellite_opt``; ``None`` when every entry is ``None``) and, for
    ``satellite_opt``, its sensor (``None`` when no record names MOPITT or GOSAT: the default chain refuses those granule
    by granule)."""
    family, sensors = None, set()
    for k, g in enumerate(granules):
        if g is None:
            continue
        if isinstance(g, satellite_ssmis):
            raise NotImplementedError(f"granule {k}: SSMIS records are pre-gridded by their own reader; "
                                      "use the composed default path")
        if not isinstance(g, (satellite_amf, satellite_opt)):
            raise NotImplementedError(f"granule {k}: {type(g).__name__} is not a satellite_amf or satellite_opt record")
        if family is not None and not isinstance(g, family):
            raise NotImplementedError(f"granule {k}: the list mixes satellite_amf and satellite_opt records, which go "
                                      "through the AMF recalculation and conv_ak respectively; average them separately")
        family = type(g)
        if isinstance(g, satellite_opt):
            if g.sensor in ("MOPITT", "GOSAT"):
                sensors.add(g.sensor)
            if len(sensors) > 1:
                raise NotImplementedError(f"granule {k}: the list mixes MOPITT and GOSAT records; conv_ak convolves a "
                                          "month with one sensor's formula, average them separately")
        elif np.size(g.scattering_weights) == 1:
            raise NotImplementedError(f"granule {k}: no scattering weights; the default path averages an np.empty((1)) "
                                      "placeholder for new_amf / old_amf, which has no defined value to reproduce")
    return family, (sensors.pop() if sensors else None)


def _amf_fields(g):
    """The mean-kernel fields of a satellite_amf granule in the interpolator's order: vcd, amf, [tropopause],
    scattering-weight levels, pressure levels.  -> (fields, has_trop, nz)"""
    fields = [g.vcd, g.amf]
    has_trop = np.size(g.tropopause) != 1
    if has_trop:
        fields.append(g.tropopause)
    nz = int(np.shape(g.pressure_mid)[0])
    fields += [np.squeeze(np.asarray(g.scattering_weights)[z]) for z in range(nz)]
    fields += [np.squeeze(np.asarray(g.pressure_mid)[z]) for z in range(nz)]
    return fields, has_trop, nz


class _ModelSlots:
    """The model partial column and pressure cube of one (day, hour) slot on the granules' grid, in HBM, made once and
    reused by every granule matched to that slot (amf_recal.py:39-83)."""

    def __init__(self, ctx, ctm_data):
        self.ctx, self.ctm_data = ctx, ctm_data
        self.cache = {}

    def get(self, day, hour, upscale, sat_lon, sat_lat):
        """-> (pressure pointer, partial-column pointer, cube dtype, levels)"""
        key = (day, hour)
        hit = self.cache.get(key)
        if hit is None:
            hit = self.cache[key] = self._make(day, hour, upscale, sat_lon, sat_lat)
        return hit[1:]

    def _make(self, day, hour, upscale, sat_lon, sat_lat):
        ctx = self.ctx
        pmid, prof, delp = _model_slot(self.ctm_data, day, hour)
        nzc = int(np.shape(pmid)[0])
        nc = int(np.size(delp))
        if not upscale:
            pc_buf, pc_dt = _partial_column_device(ctx, delp, prof)
            cdt = np.dtype(np.float32) if np.result_type(pmid, pc_dt) == np.float32 else np.dtype(np.float64)
            buf = ctx.alloc(nc * cdt.itemsize + (nc * 8 if cdt != pc_dt else 0))
            ctx.upload_into(buf.at(0), np.ravel(pmid), dtype=cdt)
            if cdt == pc_dt:
                p_pc = pc_buf.at(2 * nc * pc_dt.itemsize)
            else:                                            # float32 partial column next to float64 pressures: widen
                p_pc = buf.at(nc * cdt.itemsize)
                ctx.check(ctx.lib.oisat_widen(ctx.h, pc_buf.at(2 * nc * 4), nc, p_pc))
            return (buf, pc_buf), buf.at(0), p_pc, cdt, nzc
        # the regrid grid is the coarser one: the model comes onto it through one plan for both cubes (_upscale_cube)
        plan = _sat_grid_upscale_plan(self.ctm_data, sat_lon, sat_lat)
        rd = _regrid_dtype()
        stack = ctx.alloc(2 * nc * rd.itemsize)
        ctx.upload_into(stack.at(0), np.ravel(pmid), dtype=rd)
        pc_dt = _partial_column_dtype(delp, prof)
        if pc_dt == rd:
            pc_buf, _ = _partial_column_device(ctx, delp, prof, out_ptr=stack.at(nc * rd.itemsize))
        elif pc_dt == np.float32 and rd == np.float64:
            pc_buf, _ = _partial_column_device(ctx, delp, prof)
            ctx.check(ctx.lib.oisat_widen(ctx.h, pc_buf.at(2 * nc * 4), nc, stack.at(nc * rd.itemsize)))
        else:
            raise NotImplementedError(f"model partial column in {pc_dt} with a {rd} regrid: not a combination the default "
                                      "path produces")
        out = plan.run(stack, 2 * nzc, rd, False)
        T = int(plan.T)
        return (stack, pc_buf, out), out.at(0), out.at(nzc * T * rd.itemsize), rd, nzc


class _ModelRecords:
    """The model side of the averaging-kernel convolution for one model record on the granules' grid, in HBM
    (``_ak_conv._model_record``), made once and reused by every granule matched to that record (ak_conv_mopitt.py:47-116
    rebuilds it for every granule)."""

    def __init__(self, ctx, ctm_data):
        self.ctx, self.ctm_data = ctx, ctm_data
        self.cache = {}

    def get(self, closest, upscale, sat_lon, sat_lat) -> "_ak_conv.ModelRecord":
        hit = self.cache.get(closest)
        if hit is None:
            hit = self.cache[closest] = _ak_conv._model_record(self.ctx, self.ctm_data, closest,
                                                               (sat_lon, sat_lat) if upscale else None)
        return hit


def _slim_record(g, X, Y, need, fields, ctm_time):
    e = np.empty((0,))
    if isinstance(g, satellite_opt):
        vcd, unc, ctm_vcd, x_col, ctm_xcol = fields
        return satellite_opt(vcd, g.time, [], e, Y, X, [], [], unc, [], e, e, need, ctm_vcd, ctm_xcol, ctm_time, e, e, e, e,
                             x_col, e, g.sensor)
    vcd, unc, ctm_vcd, new_amf, old_amf = fields
    return satellite_amf(vcd, old_amf, g.time, e, Y, X, [], [], unc, [], e, e, need, ctm_vcd, ctm_time, old_amf, new_amf)


def month_average(startdate: str, enddate: str, granules, ctm_data, ctm_models_coordinate: dict, interpolator_type=1,
                  grid_size=0.25, flag_thresh=0.75, workers=None, keep_daily=False):
    """The monthly means of raw ``satellite_amf`` or ``satellite_opt`` granules between ``startdate`` and ``enddate``
    (``'YYYY-mm-dd'``, end exclusive), regridded with ``interpolator_type`` onto ``grid_size`` degrees over
    ``ctm_models_coordinate``, AMFs recalculated (``satellite_amf``) or the model convolved with the averaging kernels
    (``satellite_opt``, MOPITT or GOSAT) against ``ctm_data``.  Returns the ``averaging()`` tuple ``(sat_vcd, sat_err,
    ctm_vcd, aux1, aux2, avg_datetime)``; with ``keep_daily=True``, ``(that tuple, daily)`` where ``daily`` holds one slim
    record of the input's type per input granule (vcd, uncertainty, ctm_vcd, new_amf and old_amf or x_col and ctm_xcol,
    grid, time; empty level cubes) and ``None`` for a granule that was skipped or lies outside the averaged month.
    ``workers``: qhull processes for type 1 (``interpolator_many``).  Raises ``NotImplementedError`` for inputs it does not
    cover, ``ValueError`` when no granule of the averaged month survives the regrid, and the default chain's errors where
    it meets them (a model record index out of range, an unknown model type, missing a-priori singles)."""
    result, daily, _ = _month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, interpolator_type,
                                      grid_size, flag_thresh, workers, keep_daily)
    return (result, daily) if keep_daily else result


def _month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, interpolator_type, grid_size, flag_thresh,
                   workers, keep_daily):
    """month_average -> (averaging tuple, daily records or None, (lon, lat) of the output grid)"""
    if interpolator_type not in (1, 2, 3, 4):
        raise Exception("other type of interpolation methods has not been implemented yet")
    granules = list(granules)
    family, sensor = _refuse(granules)
    opt = family is satellite_opt
    times = [None if g is None else g.time for g in granules]
    nm, nyr, slots, time_idx = _window(startdate, enddate, times)
    slot_of = {i: yi for _, yi, idx in slots for i in idx}
    # granules outside the averaged slots are never regridded: the default chain regrids and then drops them
    wanted = [g if k in slot_of else None for k, g in enumerate(granules)]

    ctx = _hip.context()
    rd = _regrid_dtype()
    # amf_recal's vcd / ctm_vcd and ak_conv's ctm_vcd / ctm_xcol are float64; GOSAT's all-NaN ctm_vcd is in the regrid dtype,
    # which is float32 only under OISAT_DTYPE=f32, where every group is float32 anyway
    acc_dt = _hip.compute_dtype(np.empty(0, dtype=np.float64))
    ng = len(granules)
    kept = ctx.alloc(4 * max(ng, 1))
    ctx.check(ctx.lib.oisat_memset(ctx.h, kept.ptr, 0, kept.nbytes))
    if opt:
        time_ctm, _ = _ak_conv._model_times(ctm_data)
        model = _ModelRecords(ctx, ctm_data)
        # vcd, uncertainty and x_col come in the regrid dtype
        f32_mask = (1 << 0 | 1 << 1 | 1 << 3) if rd == np.float32 else 0
    else:
        time_ctm, time_ctm_h, _ = _model_times(ctm_data)
        model = _ModelSlots(ctx, ctm_data)
        f32_mask = (1 << 1 | 1 << 4) if rd == np.float32 else 0   # uncertainty and old_amf come in the regrid dtype
    acc = {}
    grid = None
    daily = [None] * ng
    deferred = []                   # (granule, model-side error): ak_conv meets them after the month is regridded
    nan_row = None                  # GOSAT's ctm_vcd: zeros_like(vcd) * nan

    it = _with_triangulations(interpolator_type, wanted, workers)
    try:
        for k, (g, tri) in enumerate(it):
            if g is None:
                continue
            rg = _GranuleRegridder(g, grid_size, ctm_models_coordinate, flag_thresh, interpolator_type, tri)
            if not rg.ok:               # qhull failed: the default chain skips the granule; its word stays 0
                continue
            if opt:
                names, fields, levels = _opt_fields(g)
            else:
                fields, has_trop, nzs = _amf_fields(g)
            X, Y, (Z, shape), need = rg.regrid(fields, device=True)
            T, nf, it_rd = int(np.prod(shape)), len(fields), rd.itemsize
            grid = (X, Y, shape, need)
            p_kept = kept.at(4 * k)
            ctx.check(ctx.lib.oisat_all_nan(ctx.h, _hip.dtype_code(rd), Z.ptr, T, p_kept))
            if opt:
                try:
                    _opt_check(g, levels)
                except NameError:       # raised by the default chain only for a granule that is not all NaN
                    if ctx.download(p_kept, (1,), np.int32)[0]:
                        raise
                    continue
            _, _, (E, _), _ = rg.regrid([g.uncertainty], error=True, device=True)      # variance kernel, :185-187
            unc = ctx.alloc(T * it_rd)
            ctx.check(ctx.lib.oisat_sqrt(ctx.h, _hip.dtype_code(rd), E.ptr, T, unc.ptr))  # :188
            if rd == np.float64:
                Zf = Z
            else:                       # the default path's astype(float64) of the float32 regrid output
                Zf = ctx.alloc(nf * T * 8)
                ctx.check(ctx.lib.oisat_widen(ctx.h, Z.ptr, nf * T, Zf.ptr))

            if opt:
                # ---- averaging-kernel convolution on the regridded cubes (ak_conv_mopitt.py / ak_conv_gosat.py:42-146)
                closest = _ak_conv._closest_record(ctm_data, time_ctm, g.time)
                try:
                    mrec = model.get(closest, need, X, Y)
                except (IndexError, NameError, ValueError) as e:
                    deferred.append((k, e))
                    continue
                sat = {f: Zf.at(levels[f][0] * T * 8) for f in
                       ("pressure_mid", "averaging_kernels", "apriori_profile", "aprior_column", "apriori_surface", "vcd",
                        "pressure_weight", "x_col") if f in levels}
                out = ctx.alloc(2 * T * 8)                  # ctm_vcd (MOPITT), ctm_xcol
                _ak_conv._conv_granule(ctx, sensor, mrec, levels["pressure_mid"][1], levels["averaging_kernels"][1], sat, T,
                                       out.at(0), out.at(T * 8))
                if sensor == "GOSAT":
                    if nan_row is None or nan_row.nbytes < T * 8:
                        nan_row = ctx.alloc(T * 8)
                        ctx.check(ctx.lib.oisat_memset(ctx.h, nan_row.ptr, 0xFF, nan_row.nbytes))   # all-ones: NaN
                    p_ctm = nan_row.ptr
                else:
                    p_ctm = out.at(0)
                # vcd, uncertainty, ctm_vcd, aux1 = x_col, aux2 = ctm_xcol (averaging.py:82-90)
                ptrs = (Z.at(0), unc.ptr, p_ctm, Z.at(levels["x_col"][0] * T * it_rd), out.at(T * 8))
                ctm_time = time_ctm[closest]
            else:
                # ---- AMF recalculation on the regridded cubes (amf_recal.py:93-182), satellite side in float64
                closest, day, hour = _closest_slot(ctm_data, time_ctm, time_ctm_h, g.time)
                p_cp, p_pc, cdt, nzc = model.get(day, hour, need, X, Y)
                first_sw = 3 if has_trop else 2
                out = ctx.alloc(3 * T * 8)                      # new_amf, vcd, ctm_vcd
                _recal_granule(ctx, Zf.at((first_sw + nzs) * T * 8), Zf.at(first_sw * T * 8), nzs, cdt, p_cp, p_pc, nzc,
                               Zf.at(2 * T * 8) if has_trop else None, Zf.at(0), Zf.at(T * 8), T,
                               out.at(0), out.at(T * 8), out.at(2 * T * 8))
                # vcd, uncertainty, ctm_vcd, aux1 = new_amf, aux2 = old_amf
                ptrs = (out.at(T * 8), unc.ptr, out.at(2 * T * 8), out.at(0), Z.at(T * it_rd))
                ctm_time = time_ctm[closest]

            # ---- fold into the month (averaging.py:82-108)
            yi = slot_of[k]
            if yi not in acc:
                acc[yi] = ctx.alloc(_NFIELDS * T * (acc_dt.itemsize + 4))
                ctx.check(ctx.lib.oisat_memset(ctx.h, acc[yi].ptr, 0, acc[yi].nbytes))
            ctx.check(ctx.lib.oisat_month_accumulate(ctx.h, _hip.dtype_code(acc_dt), *ptrs, f32_mask, T, p_kept, acc[yi].ptr))
            if keep_daily:
                dts = [np.float32 if f32_mask >> f & 1 else np.float64 for f in range(_NFIELDS)]
                vals = [ctx.download(p, shape, dt) for p, dt in zip(ptrs, dts)]
                if opt and sensor == "GOSAT":
                    vals[2] = np.zeros_like(vals[0]) * np.nan
                daily[k] = (X, Y, need, tuple(vals), ctm_time)
    finally:
        it.close()

    flags = ctx.download(kept.ptr, (ng,), np.int32) if ng else np.zeros(0, np.int32)     # the one per-granule read-back
    for k, e in deferred:           # the model side of a granule the default chain keeps: ak_conv raises, in granule order
        if flags[k]:
            raise e
    chosen_times = [granules[i].time for i in time_idx if flags[i]]
    if grid is None or not chosen_times:
        raise ValueError(f"month_average({startdate!r}, {enddate!r}): no granule of the averaged month survives the regrid "
                         "(averaging() would raise StopIteration or ZeroDivisionError here)")
    X, Y, shape, _ = grid
    ny, nx = shape
    outs = [np.zeros((ny, nx, nm, nyr))] + [np.full((ny, nx, nm, nyr), np.nan) for _ in range(4)]
    T = ny * nx
    for mi, yi, idx in slots:
        if not any(flags[i] for i in idx):
            continue                    # no granule in this slot: zeros / NaN as averaging() leaves them
        fin = ctx.alloc(_NFIELDS * T * acc_dt.itemsize)
        ctx.check(ctx.lib.oisat_month_finish(ctx.h, _hip.dtype_code(acc_dt), acc[yi].ptr, T, fin.ptr))
        res = ctx.download(fin.ptr, (_NFIELDS, ny, nx), acc_dt)
        for f in range(_NFIELDS):
            outs[f][:, :, mi, yi] = res[f]
    # averaging()'s output order: vcd, error, ctm_vcd, aux1, aux2
    result = tuple(o.squeeze() for o in outs)
    timestamps = [t.timestamp() for t in chosen_times]
    avg_datetime = datetime.datetime.fromtimestamp(sum(timestamps) / len(timestamps))
    result = result + (avg_datetime,)
    slim = None
    if keep_daily:
        slim = [None if d is None or not flags[k] else _slim_record(granules[k], *d[:3], d[3], d[4]) for k, d in enumerate(daily)]
    return result, slim, (X, Y)

