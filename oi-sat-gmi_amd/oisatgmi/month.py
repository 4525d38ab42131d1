"""A month of raw L2 granules to monthly means without leaving HBM.

``month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, ...)`` returns what

    sat = interpolator_many(interpolator_type, grid_size, granules, ctm_models_coordinate, flag_thresh)
    sat = amf_recal(ctm_data, sat)
    reader.sat_data, reader.ctm_data = sat, ctm_data
    averaging(startdate, enddate, reader)

returns, bit for bit, but every granule's regridded fields stay on the device: the regrid output feeds the AMF
recalculation (``oisat_amf_recal``) and the averaged fields are folded into running per-cell (sum, count) accumulators
(``oisat_month_accumulate``) in the order ``averaging()`` would stack them.  The read-backs are the finished monthly
grids and one int32 "kept" word per granule (``oisat_all_nan``: the device form of the interpolator's all-NaN skip
test), read once per month.  Host memory no longer grows with the number of granules.

Why the bits agree: the regrid and the AMF kernels are the same launches on the same device data; the square root of
the regridded variance is ``oisat_sqrt`` (correctly rounded, as ``np.sqrt``); float32 -> float64 widening is exact and
float64 -> float32 narrowing rounds to nearest-even on both sides; the accumulators add granule by granule in the
stack order from zero, as ``stack_reduce_kernel`` does, and close with the same ``finish``.

Covered: ``satellite_amf`` granules with scattering weights, interpolator types 1-4.  Anything else is refused with
``NotImplementedError`` before the device is touched (``satellite_opt`` goes through ``conv_ak``; SSMIS has its own
pre-gridder; without scattering weights the default chain averages an ``np.empty((1))`` placeholder).
"""
from __future__ import annotations

import datetime

import numpy as np

from . import _hip
from .amf_recal import (_closest_slot, _model_slot, _model_times, _partial_column_device, _partial_column_dtype,
                        _recal_granule, _sat_grid_upscale_plan)
from .averaging import _window
from .config import satellite_amf, satellite_opt, satellite_ssmis
from .interpolator import _GranuleRegridder, _regrid_dtype, _with_triangulations

_NFIELDS = 5                 # vcd, uncertainty, ctm_vcd, new_amf, old_amf (csrc/averaging.hip, oisat_month_accumulate)


def _refuse(granules):
    """NotImplementedError for every input the resident path does not reproduce (before any device work)."""
    for k, g in enumerate(granules):
        if g is None:
            continue
        if isinstance(g, satellite_opt):
            raise NotImplementedError(f"granule {k}: satellite_opt records (MOPITT / GOSAT) go through conv_ak, "
                                      "not the AMF recalculation; use the composed default path")
        if isinstance(g, satellite_ssmis):
            raise NotImplementedError(f"granule {k}: SSMIS records are pre-gridded by their own reader; "
                                      "use the composed default path")
        if not isinstance(g, satellite_amf):
            raise NotImplementedError(f"granule {k}: {type(g).__name__} is not a satellite_amf record")
        if np.size(g.scattering_weights) == 1:
            raise NotImplementedError(f"granule {k}: no scattering weights; the default path averages an np.empty((1)) "
                                      "placeholder for new_amf / old_amf, which has no defined value to reproduce")


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


def _slim_record(g, X, Y, need, fields, ctm_time):
    vcd, unc, ctm_vcd, new_amf, old_amf = fields
    return satellite_amf(vcd, old_amf, g.time, np.empty((0,)), Y, X, [], [], unc, [], np.empty((0,)), np.empty((0,)), need,
                         ctm_vcd, ctm_time, old_amf, new_amf)


def month_average(startdate: str, enddate: str, granules, ctm_data, ctm_models_coordinate: dict, interpolator_type=1,
                  grid_size=0.25, flag_thresh=0.75, workers=None, keep_daily=False):
    """The monthly means of raw ``satellite_amf`` granules between ``startdate`` and ``enddate`` (``'YYYY-mm-dd'``, end
    exclusive), regridded with ``interpolator_type`` onto ``grid_size`` degrees over ``ctm_models_coordinate``, AMFs
    recalculated against ``ctm_data``.  Returns the ``averaging()`` tuple ``(sat_vcd, sat_err, ctm_vcd, aux1, aux2,
    avg_datetime)``; with ``keep_daily=True``, ``(that tuple, daily)`` where ``daily`` holds one slim ``satellite_amf``
    per input granule (vcd, uncertainty, ctm_vcd, new_amf, old_amf, grid, time; empty level cubes) and ``None`` for a
    granule that was skipped or lies outside the averaged month.  ``workers``: qhull processes for type 1
    (``interpolator_many``).  Raises ``NotImplementedError`` for inputs it does not cover and ``ValueError`` when no
    granule of the averaged month survives the regrid."""
    result, daily, _ = _month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, interpolator_type,
                                      grid_size, flag_thresh, workers, keep_daily)
    return (result, daily) if keep_daily else result


def _month_average(startdate, enddate, granules, ctm_data, ctm_models_coordinate, interpolator_type, grid_size, flag_thresh,
                   workers, keep_daily):
    """month_average -> (averaging tuple, daily records or None, (lon, lat) of the output grid)"""
    if interpolator_type not in (1, 2, 3, 4):
        raise Exception("other type of interpolation methods has not been implemented yet")
    granules = list(granules)
    _refuse(granules)
    times = [None if g is None else g.time for g in granules]
    nm, nyr, slots, time_idx = _window(startdate, enddate, times)
    slot_of = {i: yi for _, yi, idx in slots for i in idx}
    # granules outside the averaged slots are never regridded: the default chain regrids and then drops them
    wanted = [g if k in slot_of else None for k, g in enumerate(granules)]

    ctx = _hip.context()
    rd = _regrid_dtype()
    acc_dt = _hip.compute_dtype(np.empty(0, dtype=np.float64))      # amf_recal's vcd / ctm_vcd are float64
    ng = len(granules)
    kept = ctx.alloc(4 * max(ng, 1))
    ctx.check(ctx.lib.oisat_memset(ctx.h, kept.ptr, 0, kept.nbytes))
    time_ctm, time_ctm_h, _ = _model_times(ctm_data)
    model = _ModelSlots(ctx, ctm_data)
    acc = {}
    grid = None
    daily = [None] * ng
    f32_mask = (1 << 1 | 1 << 4) if rd == np.float32 else 0       # uncertainty and old_amf come in the regrid dtype

    it = _with_triangulations(interpolator_type, wanted, workers)
    try:
        for k, (g, tri) in enumerate(it):
            if g is None:
                continue
            rg = _GranuleRegridder(g, grid_size, ctm_models_coordinate, flag_thresh, interpolator_type, tri)
            if not rg.ok:               # qhull failed: the default chain skips the granule; its word stays 0
                continue
            fields, has_trop, nzs = _amf_fields(g)
            X, Y, (Z, shape), need = rg.regrid(fields, device=True)
            T, nf, it_rd = int(np.prod(shape)), len(fields), rd.itemsize
            grid = (X, Y, shape, need)
            p_kept = kept.at(4 * k)
            ctx.check(ctx.lib.oisat_all_nan(ctx.h, _hip.dtype_code(rd), Z.ptr, T, p_kept))
            _, _, (E, _), _ = rg.regrid([g.uncertainty], error=True, device=True)      # variance kernel, :185-187
            unc = ctx.alloc(T * it_rd)
            ctx.check(ctx.lib.oisat_sqrt(ctx.h, _hip.dtype_code(rd), E.ptr, T, unc.ptr))  # :188

            # ---- AMF recalculation on the regridded cubes (amf_recal.py:93-182), satellite side in float64
            closest, day, hour = _closest_slot(ctm_data, time_ctm, time_ctm_h, g.time)
            p_cp, p_pc, cdt, nzc = model.get(day, hour, need, X, Y)
            if rd == np.float64:
                Zf = Z
            else:                       # the default path's astype(float64) of the float32 regrid output
                Zf = ctx.alloc(nf * T * 8)
                ctx.check(ctx.lib.oisat_widen(ctx.h, Z.ptr, nf * T, Zf.ptr))
            first_sw = 3 if has_trop else 2
            out = ctx.alloc(3 * T * 8)                      # new_amf, vcd, ctm_vcd
            _recal_granule(ctx, Zf.at((first_sw + nzs) * T * 8), Zf.at(first_sw * T * 8), nzs, cdt, p_cp, p_pc, nzc,
                           Zf.at(2 * T * 8) if has_trop else None, Zf.at(0), Zf.at(T * 8), T,
                           out.at(0), out.at(T * 8), out.at(2 * T * 8))

            # ---- fold into the month (averaging.py:82-108): vcd, uncertainty, ctm_vcd, new_amf, old_amf
            yi = slot_of[k]
            if yi not in acc:
                acc[yi] = ctx.alloc(_NFIELDS * T * (acc_dt.itemsize + 4))
                ctx.check(ctx.lib.oisat_memset(ctx.h, acc[yi].ptr, 0, acc[yi].nbytes))
            ctx.check(ctx.lib.oisat_month_accumulate(ctx.h, _hip.dtype_code(acc_dt), out.at(T * 8), unc.ptr, out.at(2 * T * 8),
                                                     out.at(0), Z.at(T * it_rd), f32_mask, T, p_kept, acc[yi].ptr))
            if keep_daily:
                res = ctx.download(out.ptr, (3,) + tuple(shape), np.float64)
                daily[k] = (X, Y, need, (res[1], ctx.download(unc.ptr, shape, rd), res[2], res[0],
                                         ctx.download(Z.at(T * it_rd), shape, rd)), time_ctm[closest])
    finally:
        it.close()

    flags = ctx.download(kept.ptr, (ng,), np.int32) if ng else np.zeros(0, np.int32)     # the one per-granule read-back
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
    # averaging()'s output order: vcd, error, ctm_vcd, aux1 = new_amf, aux2 = old_amf
    result = tuple(o.squeeze() for o in outs)
    timestamps = [t.timestamp() for t in chosen_times]
    avg_datetime = datetime.datetime.fromtimestamp(sum(timestamps) / len(timestamps))
    result = result + (avg_datetime,)
    slim = None
    if keep_daily:
        slim = [None if d is None or not flags[k] else _slim_record(granules[k], *d[:3], d[3], d[4]) for k, d in enumerate(daily)]
    return result, slim, (X, Y)

