"""Averaging-kernel convolution on the MI355X -- what ``oisatgmi.conv_ak`` runs for optimal-estimation products.

Shared body of the drop-ins for ``oisatgmi/ak_conv_mopitt.py`` and ``oisatgmi/ak_conv_gosat.py`` of the
reference (the two files are identical up to the per-pixel formula).  Time matching and record bookkeeping stay
on the host; the model columns (:60-77), the optional model upscaling (:79-116, one regridding plan instead of
4*nz ``_upscaler`` calls) and the per-pixel log-pressure interpolation + averaging kernels (:118-138, a Python
double loop with one scipy ``interp1d`` per pixel in the reference) run on the device (``csrc/amf.hip``).

The model record (``_model_record``) and the per-granule convolution (``_conv_granule``) work on device pointers, so
that ``oisatgmi.month`` can feed them the regrid output in place and reuse one model record for many granules.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _hip
from .amf_recal import _flatten_time, _sat_grid_upscale_plan
from .interpolator import _regrid_dtype

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)

#: one model record in HBM: pressure, profile and air partial column, level-major (nzc, n) cubes of ``dtype``
ModelRecord = collections.namedtuple("ModelRecord", "p_pmid p_prof p_air dtype nzc n bufs")


def _own_dtype(a) -> np.dtype:
    """The dtype NumPy keeps through the reference's arithmetic on a model cube: float32 stays, anything else is float64."""
    return _F32 if np.asarray(a).dtype == _F32 else _F64


def _time_mean(ctx, cube):
    """``np.nanmean(cube, axis=0)`` of a (nt, nz, ny, nx) model cube in its own dtype (ak_conv_mopitt.py:70-75)."""
    cube = np.asarray(cube)
    dt = _own_dtype(cube)
    k = int(cube.shape[0])
    n = int(cube[0].size)
    buf = ctx.upload(cube, dtype=dt)
    out = ctx.alloc(n * dt.itemsize)
    ctx.check(ctx.lib.oisat_nanmean_stack(ctx.h, _hip.dtype_code(dt), buf.ptr, k, n, 0, out.ptr))
    return ctx.download(out.ptr, cube.shape[1:], dt).squeeze()


def _model_times(ctm_data):
    """-> (flattened model times, one time list per record) as ak_conv_mopitt.py:30-38 builds them."""
    return np.array([_flatten_time(t) for rec in ctm_data for t in rec.time]), [rec.time for rec in ctm_data]


def _closest_record(ctm_data, time_ctm, t):
    """The model record a granule observed at ``t`` is convolved with (:42-49): day resolution only, and the index of the
    closest time SLOT is used as a RECORD index (the caller's ``ctm_data[closest]`` raises IndexError past the end)."""
    t_sat = t.year * 10000 + t.month * 100 + t.day
    return int(np.argmin(np.abs(t_sat - time_ctm))) if not ctm_data[0].averaged else 0


def _model_record(ctx, ctm_data, closest, sat_grid=None) -> ModelRecord:
    """The model side of record ``closest`` (:60-116) in HBM: pressure and profile (GMI: nan-averaged over time in their
    own dtype; ECCOH / FREE: squeezed) and the air partial column of delta_p, each in the dtype the reference keeps, then
    in the cube dtype ``result_type(pmid, prof, air)``.  ``sat_grid = (lon, lat)``: the granule grid is the coarser one
    (``ctm_upscaled_needed``) and the three cubes come onto it through one upscale plan, in the regrid dtype."""
    rec = ctm_data[closest]
    kind = ctm_data[0].ctmtype
    if kind in ("ECCOH", "FREE"):
        pieces = [rec.pressure_mid.squeeze(), rec.gas_profile.squeeze(), rec.delta_p.squeeze()]
        dts = [np.asarray(pieces[0]).dtype, np.asarray(pieces[1]).dtype, _own_dtype(pieces[2])]
        shape = np.shape(pieces[0])
    elif kind == "GMI":
        pieces = [rec.pressure_mid, rec.gas_profile, rec.delta_p]
        dts = [_own_dtype(p) for p in pieces]
        shape = np.shape(np.asarray(pieces[0])[0].squeeze())
    else:                                   # the reference leaves the names unbound for any other model (:60-77)
        raise NameError(f"name 'ctm_mid_pressure' is not defined (ctmtype {kind!r} is not handled by the AK convolution)")
    nzc = int(shape[0])
    nc = int(np.prod(shape))                # every level
    bufs = []
    if sat_grid is None:
        cdt = _F32 if np.result_type(*dts) == _F32 else _F64
    else:
        plan = _sat_grid_upscale_plan(ctm_data, *sat_grid)
        cdt = _regrid_dtype()
    stack = ctx.alloc(3 * nc * cdt.itemsize)
    bufs.append(stack)
    slots = [stack.at(i * nc * cdt.itemsize) for i in range(3)]

    def produce(dt, dst, make):
        """``make(ptr)`` writes nc values of ``dt`` at ptr; they land in ``dst`` as ``cdt`` (the host path's astype)."""
        if dt == cdt:
            make(dst)
            return
        tmp = ctx.alloc(nc * dt.itemsize)
        bufs.append(tmp)
        make(tmp.ptr)
        if dt == _F32:                      # float32 -> float64: exact
            ctx.check(ctx.lib.oisat_widen(ctx.h, tmp.ptr, nc, dst))
        else:                               # float64 model with a float32 regrid: NumPy's rounding, once per record
            ctx.upload_into(dst, ctx.download(tmp.ptr, (nc,), dt), dtype=cdt)

    def time_mean(cube, dt):
        def make(ptr):                      # np.nanmean(cube, axis=0) in the cube's own dtype (:70-75)
            buf = ctx.upload(np.asarray(cube), dtype=dt)
            bufs.append(buf)
            ctx.check(ctx.lib.oisat_nanmean_stack(ctx.h, _hip.dtype_code(dt), buf.ptr, int(np.shape(cube)[0]), nc, 0, ptr))
        return make

    for i in (0, 1):
        if kind == "GMI":
            produce(dts[i], slots[i], time_mean(pieces[i], dts[i]))
        else:
            ctx.upload_into(slots[i], np.ravel(pieces[i]), dtype=cdt)
    adt = dts[2]
    dp = ctx.alloc(nc * adt.itemsize)
    bufs.append(dp)
    if kind == "GMI":
        time_mean(pieces[2], adt)(dp.ptr)
    else:
        ctx.upload_into(dp.ptr, np.ravel(pieces[2]), dtype=adt)
    # deltap/g/Mair*N_A*1e-4*1e-15*100 in delta_p's own dtype (:66)
    produce(adt, slots[2], lambda ptr: ctx.check(ctx.lib.oisat_partial_column(ctx.h, _hip.dtype_code(adt), dp.ptr, None, nc,
                                                                                ptr)))
    if sat_grid is None:
        return ModelRecord(slots[0], slots[1], slots[2], cdt, nzc, nc // nzc, bufs)
    out = plan.run(stack, 3 * nzc, cdt, False)
    bufs.append(out)
    T = int(plan.T)
    return ModelRecord(out.at(0), out.at(nzc * T * cdt.itemsize), out.at(2 * nzc * T * cdt.itemsize), cdt, nzc, T, bufs)


def _conv_granule(ctx, sensor, model: ModelRecord, nzs, nak, sat, n, p_ctm_vcd, p_ctm_xcol):
    """The per-pixel convolution (:118-146) of one granule of ``n`` pixels on device pointers.  ``sat`` maps satellite_opt
    field names to float64 device rows: ``pressure_mid``, ``averaging_kernels`` (``nak`` rows), ``apriori_profile`` (level-
    major, ``nzs`` rows) and ``aprior_column``, ``apriori_surface``, ``vcd`` (MOPITT) or ``pressure_weight`` (``nzs`` rows),
    ``x_col`` (GOSAT).  Writes float64 ctm_vcd (MOPITT only) and ctm_xcol, n each."""
    if model.n != n:
        raise ValueError(f"the model record holds {model.n} cells per level, the granule {n}")
    code = _hip.dtype_code(model.dtype)
    if sensor == "MOPITT":
        if nak != nzs + 1:
            raise ValueError("MOPITT averaging kernels must hold one surface row plus one row per profile level")
        ctx.check(ctx.lib.oisat_ak_conv_mopitt(ctx.h, code, model.p_pmid, model.p_prof, model.p_air, model.nzc,
                                               sat["pressure_mid"], sat["averaging_kernels"], sat["apriori_profile"], nzs,
                                               sat["aprior_column"], sat["apriori_surface"], sat["vcd"], n, p_ctm_vcd,
                                               p_ctm_xcol))
    else:
        ctx.check(ctx.lib.oisat_ak_conv_gosat(ctx.h, code, model.p_pmid, model.p_prof, model.nzc, sat["pressure_mid"],
                                              sat["averaging_kernels"], sat["apriori_profile"], sat["pressure_weight"], nzs,
                                              sat["x_col"], n, p_ctm_xcol))


def ak_conv(ctm_data: list, sat_data: list, sensor: str):
    print('Averaging Kernel Conv begins...')
    ctx = _hip.context()
    time_ctm, time_ctm_datetype = _model_times(ctm_data)
    for L2 in sat_data:
        if L2 is None:
            continue
        closest = _closest_record(ctm_data, time_ctm, L2.time)
        # the reference uses the time-slot index as the record index (:47-49,:61): same IndexError when it is out of range
        print("The closest GMI file used for the L2 at " + str(L2.time) + " is at " + str(time_ctm_datetype[closest]))
        upscale = L2.ctm_upscaled_needed == True                                    # noqa: E712   :79
        model = _model_record(ctx, ctm_data, closest, (L2.longitude_center, L2.latitude_center) if upscale else None)
        nzs = int(np.shape(L2.pressure_mid)[0])
        shape = np.shape(L2.vcd)
        n = int(np.size(L2.vcd))
        names = ["pressure_mid", "averaging_kernels", "apriori_profile"]
        names += ["aprior_column", "apriori_surface", "vcd"] if sensor == "MOPITT" else ["pressure_weight", "x_col"]
        total = sum(int(np.size(getattr(L2, nm))) * 8 + 16 for nm in names) + 2 * n * 8 + 64
        cube = ctx.alloc(total)
        off = 0
        sat = {}
        for nm in names:
            off = -(-off // 16) * 16
            sat[nm] = cube.at(off)
            off += ctx.upload_into(sat[nm], np.ravel(getattr(L2, nm)), dtype=np.float64)
        off = -(-off // 16) * 16
        p_out = cube.at(off)
        _conv_granule(ctx, sensor, model, nzs, int(np.shape(L2.averaging_kernels)[0]), sat, n, p_out, cube.at(off + n * 8))
        if sensor == "MOPITT":
            res = ctx.download(p_out, (2,) + tuple(shape), np.float64)
            L2.ctm_vcd, L2.ctm_xcol = res[0], res[1]
        else:
            L2.ctm_vcd = np.zeros_like(L2.vcd) * np.nan            # NaN for GOSAT: only XCH4 is used (:138)
            L2.ctm_xcol = ctx.download(cube.at(off + n * 8), shape, np.float64)
        L2.ctm_time_at_sat = time_ctm[closest]
        cube.free()
        for b in model.bufs:
            b.free()
    return sat_data
