"""The device-resident month (oisatgmi.month.month_average, csrc/averaging.hip oisat_month_*) against the composed
default path it replaces -- interpolator_many -> amf_recal -> averaging -- bit for bit, on small regional grids.
Needs a real MI355X: run with  -m gpu."""
import copy
import datetime
import os
import tracemalloc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oisatgmi import _hip, synthetic as syn
from oisatgmi.amf_recal import amf_recal
from oisatgmi.averaging import averaging
from oisatgmi.config import ctm_model
from oisatgmi.driver import oisatgmi, O3_DIVISOR
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
NZS = 5


def _granule(seed, when, lon_c=0.0, lat0=-12.0, lat1=12.0, dtype=np.float64, trop=True, inf=False, nscan=90, npix=36):
    g = syn.swath_level_granule(seed, "amf", nz=NZS, nscan=nscan, npix=npix, lat0=lat0, lat1=lat1, lon_c=lon_c,
                                width_deg=14.0)
    g.time = when
    if dtype != np.float64:
        g.vcd, g.amf, g.uncertainty = (np.asarray(a, dtype=dtype) for a in (g.vcd, g.amf, g.uncertainty))
    if not trop:
        g.tropopause = np.empty((1))
    if inf:
        g.vcd = np.array(g.vcd)
        g.vcd[5, 3:9] = np.inf
        g.vcd[40, 10:14] = -np.inf
    return g


def _collinear(seed, when):
    """qhull cannot triangulate it: every pixel on one line (type 1 skips the granule)."""
    g = _granule(seed, when)
    g.latitude_center = 0.5 * np.asarray(g.longitude_center)
    return g


def _ctm(dtype=np.float64, averaged=False, free=False, year=2019, month=6, step=1.0):
    ny, nx = int(round(30 / step)) + 1, int(round(40 / step)) + 1
    ctm = syn.ctm_days(ny, nx, 8, 2, 7100, averaged=averaged, dtype=dtype, lat0=-15.0, lat1=15.0, lon0=-20.0, lon1=20.0,
                       year=year, month=month)
    if free:    # one profile per day, no hour axis (amf_recal.py:39-43)
        ctm = [ctm_model(c.latitude, c.longitude, c.time, c.gas_profile[3], c.pressure_mid[3], c.tempeature_mid[3],
                         c.delta_p[3], "FREE", c.averaged) for c in ctm]
    return ctm


def _coord(ctm):
    return {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}


def _default_chain(itype, grid_size, raw, ctm, start, end, flag=0.75):
    sat = interpolator_many(itype, grid_size, copy.deepcopy(raw), _coord(ctm), flag)
    sat = amf_recal(ctm, sat)
    r = _Reader()
    r.sat_data, r.ctm_data = sat, ctm
    return averaging(start, end, r)


def _assert_same(got, want):
    assert len(got) == len(want) == 6
    for f, (a, b) in enumerate(zip(got[:5], want[:5])):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=True), (f, np.nanmax(np.abs(a - b)))
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
    assert got[5] == want[5]


JUNE = datetime.datetime(2019, 6, 1, 13, 20)


def _june(k, **kw):
    return _granule(8000 + k, JUNE.replace(day=1 + k % 2, minute=5 * k), lon_c=-8.0 + 4.0 * (k % 5), **kw)


CASES = {
    # name: (interpolator type, grid_size, ctm kwargs, granules, window)
    "type4_f64": (4, 0.25, {}, lambda: [_june(k) for k in range(4)], ("2019-06-01", "2019-07-01")),
    "type1_f32ctm_averaged": (1, 0.25, dict(dtype=np.float32, averaged=True), lambda: [_june(k) for k in range(3)],
                              ("2019-06-01", "2019-07-01")),
    "type3_free": (3, 0.25, dict(free=True), lambda: [_june(k) for k in range(3)], ("2019-06-01", "2019-07-01")),
    "type4_no_trop_f32ctm": (4, 0.25, dict(dtype=np.float32), lambda: [_june(k, trop=False) for k in range(3)],
                             ("2019-06-01", "2019-07-01")),
    "type4_raw_f16_f32": (4, 0.25, {}, lambda: [_june(0, dtype=np.float16), _june(1, dtype=np.float32), _june(2)],
                          ("2019-06-01", "2019-07-01")),
    "type1_inf_outside_collinear": (1, 0.25, {}, lambda: [_june(0, inf=True), _granule(8100, JUNE, lon_c=150.0),
                                                          _collinear(8101, JUNE), None, _june(3)],
                                    ("2019-06-01", "2019-07-01")),
    "type4_neighbour_months": (4, 0.25, {}, lambda: [_june(0), _granule(8200, JUNE.replace(month=7, day=2)), _june(1),
                                                     _granule(8201, JUNE.replace(month=5, day=30))],
                               ("2019-06-01", "2019-07-01")),
    "type4_two_month_window": (4, 0.25, {}, lambda: [_granule(8300, JUNE.replace(month=5, day=20)), _june(0), _june(1)],
                               ("2019-05-15", "2019-07-01")),
    "type4_dec_jan_window": (4, 0.25, dict(year=2019, month=12),
                             lambda: [_granule(8400, datetime.datetime(2019, 12, 1, 12)),
                                      _granule(8401, datetime.datetime(2020, 1, 2, 12)),
                                      _granule(8402, datetime.datetime(2020, 12, 1, 13), lon_c=4.0),
                                      _granule(8403, datetime.datetime(2019, 12, 2, 14), lon_c=-4.0)],
                             ("2019-12-01", "2020-02-01")),
    "type4_model_finer_than_grid": (4, 1.5, {}, lambda: [_june(k) for k in range(3)], ("2019-06-01", "2019-07-01")),
    "type1_model_finer_f32ctm": (1, 1.5, dict(dtype=np.float32), lambda: [_june(k) for k in range(3)],
                                 ("2019-06-01", "2019-07-01")),
    "type3_coarse_model": (3, 0.25, dict(step=2.0), lambda: [_june(k) for k in range(2)], ("2019-06-01", "2019-07-01")),
}


@pytest.mark.parametrize("env", [None, "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_month_average_is_bitwise_the_default_chain(ctx, monkeypatch, name, env):
    if env:
        monkeypatch.setenv("OISAT_DTYPE", env)
    else:
        monkeypatch.delenv("OISAT_DTYPE", raising=False)
    itype, gs, ctm_kw, make, (start, end) = CASES[name]
    ctm = _ctm(**ctm_kw)
    raw = make()
    want = _default_chain(itype, gs, raw, ctm, start, end)
    got = month_average(start, end, raw, ctm, _coord(ctm), interpolator_type=itype, grid_size=gs)
    _assert_same(got, want)
    assert np.isfinite(np.asarray(got[0])).sum() > 50


def test_empty_window_raises(ctx):
    """Dec -> Jan: only the December of the window's last year is dated; with no granule there both paths raise."""
    ctm = _ctm(year=2019, month=12)
    raw = [_granule(8500, datetime.datetime(2019, 12, 1, 12)), _granule(8501, datetime.datetime(2020, 1, 2, 12))]
    with pytest.raises((ZeroDivisionError, StopIteration)):
        _default_chain(4, 0.25, raw, ctm, "2019-12-01", "2020-02-01")
    with pytest.raises(ValueError, match="no granule"):
        month_average("2019-12-01", "2020-02-01", raw, ctm, _coord(ctm), interpolator_type=4)
    with pytest.raises(ValueError, match="no granule"):          # everything outside the model region
        month_average("2019-06-01", "2019-07-01", [_granule(8502, JUNE, lon_c=150.0)], _ctm(), _coord(_ctm()),
                      interpolator_type=4)


# ------------------------------------------------------------------------------------------------------------------------
# the accumulator kernels against the stack kernels
# ------------------------------------------------------------------------------------------------------------------------
def _stack_reference(ctx, stacks, acc_dt):
    """oisat_nanmean_stack / oisat_error_average of the five (k, n) stacks (already in acc_dt)."""
    out = []
    for f, st in enumerate(stacks):
        k, n = st.shape
        b = ctx.upload(st, dtype=acc_dt)
        o = ctx.alloc(n * acc_dt.itemsize)
        if f == 1:
            ctx.check(ctx.lib.oisat_error_average(ctx.h, _hip.dtype_code(acc_dt), b.ptr, k, n, 1, o.ptr))
        else:
            ctx.check(ctx.lib.oisat_nanmean_stack(ctx.h, _hip.dtype_code(acc_dt), b.ptr, k, n, 1 if f == 0 else 0, o.ptr))
        out.append(ctx.download(o.ptr, (n,), acc_dt))
    return np.stack(out)


@pytest.mark.parametrize("acc", ["f32", "f64"])
@pytest.mark.parametrize("in_dt", ["f32", "f64", "mixed"])
@pytest.mark.parametrize("n,misalign", [(4096, 0), (1001, 0), (4096, 1)])
def test_month_accumulate_matches_stack_kernels(ctx, acc, in_dt, n, misalign):
    rng = np.random.default_rng(n + 7 * misalign + len(in_dt))
    acc_dt = np.dtype(np.float32 if acc == "f32" else np.float64)
    k = 7
    dts = {"f32": [np.float32] * 5, "f64": [np.float64] * 5, "mixed": [np.float64, np.float32, np.float64, np.float64, np.float32]}[in_dt]
    stacks = []
    for f in range(5):
        a = rng.lognormal(0.0, 1.0, size=(k, n)) * rng.choice([-1.0, 1.0], size=(k, n))
        a[rng.uniform(size=(k, n)) < 0.15] = np.nan
        a[rng.uniform(size=(k, n)) < 0.03] = np.inf
        a[rng.uniform(size=(k, n)) < 0.03] = -np.inf
        a[:, :5] = np.nan                               # cells with no valid granule
        stacks.append(a.astype(dts[f]))
    want = _stack_reference(ctx, [s.astype(acc_dt) for s in stacks], acc_dt)

    item = acc_dt.itemsize
    accb = ctx.alloc(5 * n * (item + 4) + 64)
    acc_ptr = accb.at(misalign * item)
    ctx.check(ctx.lib.oisat_memset(ctx.h, accb.ptr, 0, accb.nbytes))
    mask = sum(1 << f for f in range(5) if dts[f] == np.float32)
    kept = ctx.upload(np.array([1, 0], dtype=np.int32))
    junk = [ctx.upload(np.full(n + 4, 1e30, dtype=dts[f])) for f in range(5)]
    for g in range(k):
        bufs = []
        for f in range(5):
            b = ctx.alloc((n + 4) * np.dtype(dts[f]).itemsize)
            ctx.upload_into(b.at(misalign * np.dtype(dts[f]).itemsize), stacks[f][g])
            bufs.append(b)
        ptrs = [b.at(misalign * np.dtype(dts[f]).itemsize) for f, b in enumerate(bufs)]
        ctx.check(ctx.lib.oisat_month_accumulate(ctx.h, _hip.dtype_code(acc_dt), *ptrs, mask, n, kept.ptr, acc_ptr))
        # a granule whose word is 0 changes nothing
        ctx.check(ctx.lib.oisat_month_accumulate(ctx.h, _hip.dtype_code(acc_dt), *[j.ptr for j in junk], mask, n,
                                                 kept.at(4), acc_ptr))
    out = ctx.alloc(5 * n * item)
    ctx.check(ctx.lib.oisat_month_finish(ctx.h, _hip.dtype_code(acc_dt), acc_ptr, n, out.ptr))
    got = ctx.download(out.ptr, (5, n), acc_dt)
    for f in range(5):
        assert np.array_equal(got[f], want[f], equal_nan=True), f
    assert np.isnan(got[:, :5]).all()


def test_all_nan_word_and_sqrt(ctx):
    for dt in (np.float32, np.float64):
        x = np.full(3001, np.nan, dtype=dt)
        b = ctx.upload(x)
        w = ctx.upload(np.array([7], dtype=np.int32))
        ctx.check(ctx.lib.oisat_all_nan(ctx.h, _hip.dtype_code(dt), b.ptr, x.size, w.ptr))
        assert ctx.download(w.ptr, (1,), np.int32)[0] == 0
        x[2999] = np.inf
        b = ctx.upload(x)
        ctx.check(ctx.lib.oisat_all_nan(ctx.h, _hip.dtype_code(dt), b.ptr, x.size, w.ptr))
        assert ctx.download(w.ptr, (1,), np.int32)[0] == 1
    # oisat_sqrt replaces the host np.sqrt of the regridded variance: correctly rounded in both dtypes
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        x = np.concatenate([rng.lognormal(0.0, 6.0, 200000), rng.uniform(0, 1, 1000) * np.finfo(dt).tiny,
                            [0.0, -0.0, np.inf, np.nan, -1.0]]).astype(dt)
        b = ctx.upload(x)
        o = ctx.alloc(x.nbytes)
        ctx.check(ctx.lib.oisat_sqrt(ctx.h, _hip.dtype_code(dt), b.ptr, x.size, o.ptr))
        with np.errstate(invalid="ignore"):
            want = np.sqrt(x)
        got = ctx.download(o.ptr, x.shape, dt)
        assert np.array_equal(got.view(np.uint32 if dt == np.float32 else np.uint64)[:-1],
                              want.view(np.uint32 if dt == np.float32 else np.uint64)[:-1])
        assert np.isnan(got[-1])


def test_widen(ctx):
    x = np.random.default_rng(1).normal(size=1003).astype(np.float32)
    x[:3] = (np.nan, np.inf, -np.inf)
    b = ctx.upload(x)
    o = ctx.alloc(x.size * 8)
    ctx.check(ctx.lib.oisat_widen(ctx.h, b.ptr, x.size, o.ptr))
    assert np.array_equal(ctx.download(o.ptr, x.shape, np.float64), x.astype(np.float64), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------
# traffic and host memory
# ------------------------------------------------------------------------------------------------------------------------
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


def test_month_average_reads_back_only_the_grids(ctx, monkeypatch):
    ctm = _ctm()
    raw = [_june(k) for k in range(5)]
    want = _default_chain(4, 0.25, raw, ctm, "2019-06-01", "2019-07-01")        # warm the plans
    seen = _count_downloads(monkeypatch, ctx)
    got = month_average("2019-06-01", "2019-07-01", raw, ctm, _coord(ctm), interpolator_type=4)
    resident = seen["bytes"]
    _assert_same(got, want)
    grids = 5 * np.asarray(got[0]).size * 8
    assert resident <= grids + 64 * len(raw), (resident, grids)
    seen["bytes"] = 0
    _default_chain(4, 0.25, raw, ctm, "2019-06-01", "2019-07-01")
    assert seen["bytes"] > 20 * grids, (seen["bytes"], grids)


def test_month_average_host_memory_does_not_grow_with_granules(ctx):
    ctm = _ctm()
    raws = {k: [_june(i) for i in range(k)] for k in (6, 12)}
    month_average("2019-06-01", "2019-07-01", raws[6], ctm, _coord(ctm), interpolator_type=4)        # warm caches
    peaks = {}
    for k in (6, 12):
        tracemalloc.start()
        month_average("2019-06-01", "2019-07-01", raws[k], ctm, _coord(ctm), interpolator_type=4)
        peaks[k] = tracemalloc.get_traced_memory()[1]
        tracemalloc.stop()
    assert peaks[12] <= 1.1 * peaks[6], peaks


# ------------------------------------------------------------------------------------------------------------------------
# facade
# ------------------------------------------------------------------------------------------------------------------------
def test_average_granules_facade(ctx, tmp_path):
    from scipy.io import loadmat
    ctm = _ctm()
    raw = [_june(k) for k in range(4)]
    # default: regrid, recal, average on the reader
    ref = oisatgmi()
    ref.reader_obj = _Reader()
    ref.reader_obj.ctm_data = ctm
    sat = amf_recal(ctm, interpolator_many(4, 0.25, copy.deepcopy(raw), _coord(ctm), 0.75))
    ref.reader_obj.sat_data = sat
    ref.average("2019-06-01", "2019-07-01", gasname="NO2")
    ref.bias_correct("OMI", "NO2")
    ref.oi("OMI", error_ctm=50.0)
    # resident
    o = oisatgmi()
    o.reader_obj = _Reader()
    o.reader_obj.ctm_data = ctm
    o.average_granules("2019-06-01", "2019-07-01", raw, 4, 0.25, gasname="NO2", keep_daily=True)
    o.bias_correct("OMI", "NO2")
    o.oi("OMI", error_ctm=50.0)
    for att in ("sat_averaged_vcd", "sat_averaged_error", "ctm_averaged_vcd", "aux1", "aux2", "ctm_averaged_vcd_corrected",
                "ak_OI", "increment_OI", "error_OI"):
        assert np.array_equal(getattr(o, att), getattr(ref, att), equal_nan=True), att
    assert o.avg_time == ref.avg_time
    fo, fr = o.output_fields(), ref.output_fields()
    for k in fr:
        assert np.array_equal(fo[k], fr[k], equal_nan=True), k
    assert os.path.getsize(o.write_to_nc("NO2_201906", str(tmp_path / "nc"))) > 0
    # daily dumps: same files, same 2-D variables
    o.savedaily(str(tmp_path / "res"), "NO2", "201906")
    ref.savedaily(str(tmp_path / "def"), "NO2", "201906")
    names = sorted(os.listdir(tmp_path / "def"))
    assert names == sorted(os.listdir(tmp_path / "res")) and len(names) == 4
    for nm in names:
        a, b = loadmat(str(tmp_path / "res" / nm)), loadmat(str(tmp_path / "def" / nm))
        for v in ("vcd_sat", "vcd_ctm", "vcd_err", "time_sat", "lat", "lon"):
            assert np.array_equal(a[v], b[v], equal_nan=True), (nm, v)
    # without keep_daily the grid still reaches the output file
    o2 = oisatgmi()
    o2.reader_obj = _Reader()
    o2.reader_obj.ctm_data = ctm
    o2.average_granules("2019-06-01", "2019-07-01", raw, 4, 0.25, gasname="O3")
    assert np.array_equal(o2.ctm_averaged_vcd, o.ctm_averaged_vcd / O3_DIVISOR, equal_nan=True)
    o2.oi("OMI", error_ctm=50.0)
    assert np.array_equal(o2.output_fields()["lat"], fr["lat"])
