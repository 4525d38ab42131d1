"""The device-resident month for optimal-estimation granules (MOPITT CO, GOSAT XCH4: ``satellite_opt`` records) against
the composed default path it replaces -- interpolator_many -> _ak_conv.ak_conv (what conv_ak runs) -> averaging -- bit
for bit, on small regional grids.  Needs a real MI355X: run with  -m gpu."""
import copy
import datetime

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oisatgmi import _ak_conv, _hip, synthetic as syn
from oisatgmi.averaging import averaging
from oisatgmi.config import ctm_model
from oisatgmi.driver import oisatgmi
from oisatgmi.interpolator import interpolator_many
from oisatgmi.month import month_average


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    return c


class _Reader:
    pass


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
NZS = 6
JUNE = datetime.datetime(2019, 6, 1, 10, 30)


def _granule(sensor, seed, when, lon_c=0.0, lat0=-12.0, lat1=12.0):
    g = syn.swath_level_granule(seed, sensor, nz=NZS, nscan=80, npix=32, lat0=lat0, lat1=lat1, lon_c=lon_c, width_deg=14.0)
    g.time = when
    return g


def _june(sensor, k, **kw):
    return _granule(sensor, 9000 + k, JUNE.replace(day=2 + k % 3, minute=7 * k), lon_c=-8.0 + 4.0 * (k % 5), **kw)


def _collinear(sensor, seed, when):
    """qhull cannot triangulate it: every pixel on one line (type 1 skips the granule)."""
    g = _granule(sensor, seed, when)
    g.latitude_center = 0.5 * np.asarray(g.longitude_center)
    return g


def _ctm(kind="ECCOH", dtype=np.float32, averaged=False, nmonths=2, step=1.0):
    """Model records on a regional grid covering the granules (ctm_monthly: one record a month from May 2019, GMI with 8
    time slots)."""
    ny, nx = int(round(30 / step)) + 1, int(round(40 / step)) + 1
    ctm = syn.ctm_monthly(ny, nx, 10, nmonths, 7300, ctmtype="GMI" if kind == "GMI" else "ECCOH", dtype=dtype,
                          lat0=-15.0, lat1=15.0, lon0=-20.0, lon1=20.0)
    return [ctm_model(c.latitude, c.longitude, c.time, c.gas_profile, c.pressure_mid, c.tempeature_mid, c.delta_p, kind,
                      averaged) for c in ctm]


def _coord(ctm):
    return {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}


def _composed(itype, grid_size, raw, ctm, sensor, flag=0.75):
    sat = interpolator_many(itype, grid_size, copy.deepcopy(raw), _coord(ctm), flag)
    return _ak_conv.ak_conv(ctm, sat, sensor)


def _default_chain(itype, grid_size, raw, ctm, sensor, start, end, flag=0.75):
    r = _Reader()
    r.sat_data, r.ctm_data = _composed(itype, grid_size, raw, ctm, sensor, flag), ctm
    return averaging(start, end, r)


def _assert_same(got, want):
    assert len(got) == len(want) == 6
    for f, (a, b) in enumerate(zip(got[:5], want[:5])):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=True), (f, np.nanmax(np.abs(a - b)))
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
    assert got[5] == want[5]


MONTH = ("2019-06-01", "2019-07-01")

CASES = {
    # name: (interpolator type, grid_size, flag_thresh, ctm kwargs, granules(sensor), window)
    "type1_eccoh_f32": (1, 0.25, 0.75, {}, lambda s: [_june(s, k) for k in range(3)], MONTH),
    "type2_free_f64": (2, 0.25, 0.75, dict(kind="FREE", dtype=np.float64), lambda s: [_june(s, k) for k in range(3)], MONTH),
    "type3_gmi_averaged": (3, 0.25, 0.75, dict(kind="GMI", averaged=True), lambda s: [_june(s, k) for k in range(2)], MONTH),
    "type4_eccoh_averaged_f64": (4, 0.25, 0.75, dict(averaged=True, dtype=np.float64),
                                 lambda s: [_june(s, k) for k in range(4)], MONTH),
    # GMI, not averaged: the closest time SLOT is used as the record index -- slot 7 of 8 records here
    "type4_gmi_slot_as_record": (4, 0.25, 0.75, dict(kind="GMI", nmonths=8),
                                 lambda s: [_granule(s, 9100 + k, datetime.datetime(2019, 5, 2 + k, 9)) for k in range(2)],
                                 ("2019-05-01", "2019-06-01")),
    # the model is finer than the grid: ctm_upscaled_needed, one upscale plan for pressure, profile and air column
    "type4_upscale_eccoh": (4, 1.5, 0.75, {}, lambda s: [_june(s, k) for k in range(3)], MONTH),
    "type1_upscale_gmi_f64": (1, 1.5, 0.75, dict(kind="GMI", averaged=True, dtype=np.float64),
                              lambda s: [_june(s, k) for k in range(2)], MONTH),
    "type2_coarse_model": (2, 0.25, 0.75, dict(step=2.0), lambda s: [_june(s, k) for k in range(2)], MONTH),
    # out-of-window neighbours, a granule outside the model region (all NaN), a collinear one (no triangulation), None
    "type1_window": (1, 0.25, 0.75, {},
                     lambda s: [_june(s, 0), _granule(s, 9200, JUNE, lon_c=150.0), _collinear(s, 9201, JUNE), None,
                                _granule(s, 9202, JUNE.replace(month=7, day=2)), _june(s, 3),
                                _granule(s, 9203, JUNE.replace(month=5, day=30))], MONTH),
    # MOP03 level-3 lattice records as the MOPITT reader hands them over (type 1 / 4, 1.0 degree, flag 0.0)
    "type4_lattice": (4, 1.0, 0.0, {}, lambda s: [syn.lattice_l3_granule(9300 + k, s, nz=NZS) for k in range(2)], MONTH),
    "type1_lattice": (1, 1.0, 0.0, {}, lambda s: [syn.lattice_l3_granule(9310 + k, s, nz=NZS) for k in range(2)], MONTH),
}


def _env(monkeypatch, env):
    if env:
        monkeypatch.setenv("OISAT_DTYPE", env)
    else:
        monkeypatch.delenv("OISAT_DTYPE", raising=False)


@pytest.mark.parametrize("env", [None, "f32"])
@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_month_average_opt_is_bitwise_the_default_chain(ctx, monkeypatch, name, sensor, env):
    _env(monkeypatch, env)
    itype, gs, flag, ctm_kw, make, (start, end) = CASES[name]
    ctm = _ctm(**ctm_kw)
    raw = make(sensor)
    want = _default_chain(itype, gs, raw, ctm, sensor, start, end, flag)
    got = month_average(start, end, raw, ctm, _coord(ctm), interpolator_type=itype, grid_size=gs, flag_thresh=flag)
    _assert_same(got, want)
    assert np.isfinite(np.asarray(got[0])).sum() > 20
    assert np.isfinite(np.asarray(got[4])).sum() > 20                       # ctm_xcol
    if sensor == "GOSAT":
        assert np.isnan(np.asarray(got[2])).all()                            # ctm_vcd is NaN for GOSAT
    else:
        assert np.isfinite(np.asarray(got[2])).sum() > 20


# ------------------------------------------------------------------------------------------------------------------------
# the default chain's errors, in the same cases
# ------------------------------------------------------------------------------------------------------------------------
def _both_raise(itype, raw, ctm, sensor, start="2019-06-01", end="2019-07-01"):
    with pytest.raises(Exception) as want:
        _default_chain(itype, 0.25, raw, ctm, sensor, start, end)
    with pytest.raises(want.type) as got:
        month_average(start, end, raw, ctm, _coord(ctm), interpolator_type=itype)
    return want.value, got.value


@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
def test_model_errors(ctx, sensor):
    # GMI, not averaged, two records: a June granule's closest slot (15) is no record index
    w, g = _both_raise(4, [_june(sensor, 0), _june(sensor, 1)], _ctm(kind="GMI"), sensor)
    assert isinstance(g, IndexError)
    # a model type the convolution does not handle
    w, g = _both_raise(4, [_june(sensor, 0)], _ctm(kind="GEOS"), sensor)
    assert isinstance(g, NameError) and str(g) == str(w)


@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
def test_missing_singles_and_unknown_sensor(ctx, sensor):
    ctm = _ctm()
    for field in ("aprior_column", "surface_pressure", "apriori_surface"):
        bad = _june(sensor, 1)
        setattr(bad, field, np.zeros_like(getattr(bad, field)))
        w, g = _both_raise(4, [_june(sensor, 0), bad], ctm, sensor)
        assert isinstance(g, NameError) and str(g) == str(w)
        # the same record outside the model region is all NaN: both paths skip it without a word
        away = _granule(sensor, 9400, JUNE, lon_c=150.0)
        setattr(away, field, np.zeros_like(getattr(away, field)))
        raw = [_june(sensor, 0), away, _june(sensor, 2)]
        _assert_same(month_average(*MONTH, raw, ctm, _coord(ctm), interpolator_type=4),
                     _default_chain(4, 0.25, raw, ctm, sensor, *MONTH))
    other = _june(sensor, 1)
    other.sensor = "IASI"
    w, g = _both_raise(4, [_june(sensor, 0), other], ctm, sensor)
    assert isinstance(g, NameError) and str(g) == str(w)


def test_mopitt_averaging_kernel_rows(ctx):
    """A MOPITT record whose averaging kernels lack the surface row: both paths stop at the same error."""
    ctm = _ctm()
    bad = _june("MOPITT", 1)
    bad.averaging_kernels = np.asarray(bad.averaging_kernels)[1:]
    _both_raise(4, [_june("MOPITT", 0), bad], ctm, "MOPITT")
    # ak_conv itself still refuses a record with the wrong number of rows
    sat = _composed(4, 0.25, [_june("MOPITT", 0)], ctm, "MOPITT")
    sat[0].averaging_kernels = sat[0].averaging_kernels[1:]
    with pytest.raises(ValueError, match="surface row"):
        _ak_conv.ak_conv(ctm, sat, "MOPITT")


def test_empty_window_raises(ctx):
    ctm = _ctm()
    raw = [_granule("GOSAT", 9500, JUNE.replace(month=7, day=3)), _granule("GOSAT", 9501, JUNE, lon_c=150.0)]
    with pytest.raises((ZeroDivisionError, StopIteration)):
        _default_chain(4, 0.25, raw, ctm, "GOSAT", *MONTH)
    with pytest.raises(ValueError, match="no granule"):
        month_average(*MONTH, raw, ctm, _coord(ctm), interpolator_type=4)


# ------------------------------------------------------------------------------------------------------------------------
# daily records, traffic, facade
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, "f32"])
@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
def test_keep_daily_records(ctx, monkeypatch, sensor, env):
    _env(monkeypatch, env)
    ctm = _ctm()
    raw = [_june(sensor, 0), _granule(sensor, 9600, JUNE, lon_c=150.0), None, _june(sensor, 1),
           _granule(sensor, 9601, JUNE.replace(month=7, day=2))]
    sat = _composed(4, 0.25, raw, ctm, sensor)
    res, daily = month_average(*MONTH, raw, ctm, _coord(ctm), interpolator_type=4, keep_daily=True)
    assert len(daily) == len(raw)
    assert [d is None for d in daily] == [True if k in (1, 2, 4) else False for k in range(len(raw))]
    for d, s in zip(daily, sat):
        if d is None:
            continue
        assert type(d).__name__ == "satellite_opt" and d.sensor == sensor and d.time == s.time
        for f in ("vcd", "uncertainty", "ctm_vcd", "x_col", "ctm_xcol", "latitude_center", "longitude_center"):
            a, b = np.asarray(getattr(d, f)), np.asarray(getattr(s, f))
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), f
        assert d.ctm_time_at_sat == s.ctm_time_at_sat and d.ctm_upscaled_needed == s.ctm_upscaled_needed


def _count_downloads(monkeypatch, ctx):
    seen = {"bytes": 0, "calls": 0}
    orig = ctx.download

    def download(ptr, shape, dtype):
        out = orig(ptr, shape, dtype)
        seen["bytes"] += out.nbytes
        seen["calls"] += 1
        return out
    monkeypatch.setattr(ctx, "download", download)
    return seen


@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
@pytest.mark.parametrize("gs", [0.25, 1.5])
def test_month_average_opt_reads_back_only_the_grids(ctx, monkeypatch, sensor, gs):
    ctm = _ctm(kind="GMI", averaged=True)
    raw = [_june(sensor, k) for k in range(5)]
    want = _default_chain(4, gs, raw, ctm, sensor, *MONTH)                 # warm the plans
    seen = _count_downloads(monkeypatch, ctx)
    got = month_average(*MONTH, raw, ctm, _coord(ctm), interpolator_type=4, grid_size=gs)
    resident = seen["bytes"]
    _assert_same(got, want)
    grids = 5 * np.asarray(got[0]).size * 8
    assert resident <= grids + 64 * len(raw), (resident, grids)
    seen["bytes"] = 0
    _default_chain(4, gs, raw, ctm, sensor, *MONTH)
    assert seen["bytes"] > 10 * grids, (seen["bytes"], grids)
    # keep_daily reads back the five fields of each granule, nothing more
    seen["bytes"] = 0
    month_average(*MONTH, raw, ctm, _coord(ctm), interpolator_type=4, grid_size=gs, keep_daily=True)
    assert seen["bytes"] <= grids + 64 * len(raw) + len(raw) * grids, (seen["bytes"], grids)


@pytest.mark.parametrize("sensor", ["MOPITT", "GOSAT"])
def test_average_granules_facade(ctx, sensor):
    ctm = _ctm()
    raw = [_june(sensor, k) for k in range(4)]
    ref = oisatgmi()
    ref.reader_obj = _Reader()
    ref.reader_obj.ctm_data = ctm
    ref.reader_obj.sat_data = interpolator_many(4, 0.25, copy.deepcopy(raw), _coord(ctm), 0.75)
    ref.conv_ak(sensor)
    ref.average(*MONTH)
    ref.oi(sensor, error_ctm=50.0)
    o = oisatgmi()
    o.reader_obj = _Reader()
    o.reader_obj.ctm_data = ctm
    o.average_granules(*MONTH, raw, 4, 0.25)
    o.oi(sensor, error_ctm=50.0)
    for att in ("sat_averaged_vcd", "sat_averaged_error", "ctm_averaged_vcd", "aux1", "aux2", "ctm_averaged_vcd_corrected",
                "ak_OI", "increment_OI", "error_OI"):
        assert np.array_equal(getattr(o, att), getattr(ref, att), equal_nan=True), att
    assert o.avg_time == ref.avg_time
    assert np.isfinite(o.ctm_averaged_vcd_corrected).sum() > 20
