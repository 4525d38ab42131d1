"""CPU-side checks of the device-resident month (oisatgmi.month): what it refuses, before touching the device, and the
date-window selection it shares with averaging(), against a restatement of the reference's loop (averaging.py:64-108)."""
import datetime

import numpy as np
import pytest

from oisatgmi import _hip, synthetic as syn
from oisatgmi.averaging import _window
from oisatgmi.config import satellite_ssmis
from oisatgmi.month import month_average


@pytest.fixture
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the device context was touched")
    monkeypatch.setattr(_hip, "context", refuse)


def _ctm():
    return syn.ctm_days(11, 13, 4, 1, 1, lat0=-5.0, lat1=5.0, lon0=-6.0, lon1=6.0)


def _coord(ctm):
    return {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}


def _amf():
    return syn.swath_level_granule(1, "amf", nz=3, nscan=20, npix=10)


@pytest.mark.parametrize("kind", ["MOPITT", "GOSAT"])
def test_refuses_satellite_opt(no_device, kind):
    ctm = _ctm()
    raw = [_amf(), syn.swath_level_granule(2, kind, nz=3, nscan=20, npix=10)]
    with pytest.raises(NotImplementedError, match="satellite_opt"):
        month_average("2019-06-01", "2019-07-01", raw, ctm, _coord(ctm), interpolator_type=4)


def test_refuses_ssmis(no_device):
    ctm = _ctm()
    g = _amf()
    s = satellite_ssmis(g.vcd, g.uncertainty, g.time, g.latitude_center, g.longitude_center, False, [], "SSMIS")
    with pytest.raises(NotImplementedError, match="SSMIS"):
        month_average("2019-06-01", "2019-07-01", [None, s], ctm, _coord(ctm), interpolator_type=2)


def test_refuses_granules_without_scattering_weights(no_device):
    ctm = _ctm()
    g = syn.swath_granule(3, nscan=20, npix=10)                 # satellite_amf, scattering_weights = np.empty((1))
    with pytest.raises(NotImplementedError, match="scattering weights"):
        month_average("2019-06-01", "2019-07-01", [_amf(), g], ctm, _coord(ctm), interpolator_type=1)


# ------------------------------------------------------------------------------------------------------------------------
def _reference_selection(startdate, enddate, times):
    """averaging.py:40-108 restated on the granule times: the (mi, yi) output slot each reduced list goes to, the indices
    in it, the indices whose times make avg_datetime, and the output's (nm, nyr)."""
    def daterange(a, b):
        for n in range(int((b - a).days)):
            yield a + datetime.timedelta(n)
    a = datetime.date(int(startdate[0:4]), int(startdate[5:7]), int(startdate[8:10]))
    b = datetime.date(int(enddate[0:4]), int(enddate[5:7]), int(enddate[8:10]))
    months = np.array([d.month for d in daterange(a, b)])
    years = np.array([d.year for d in daterange(a, b)])
    reduced = []
    time_chosen = []
    for year in range(np.min(years), np.max(years) + 1):
        for month in range(np.min(months), np.max(months) + 1):
            chosen = []
            time_chosen = []
            for i, t in enumerate(times):
                if t is None:
                    continue
                if t.year == year and t.month == month:
                    time_chosen.append(i)
                    chosen.append(i)
        reduced.append((month - np.min(months), year - np.min(years), chosen))
    nm = np.max(months) - np.min(months) + 1
    nyr = np.max(years) - np.min(years) + 1
    return nm, nyr, reduced, time_chosen


@pytest.mark.parametrize("seed", range(40))
def test_window_selection_matches_the_reference_loop(seed):
    rng = np.random.default_rng(seed)
    y0 = int(rng.integers(2018, 2021))
    start = datetime.date(y0, int(rng.integers(1, 13)), int(rng.integers(1, 29)))
    end = start + datetime.timedelta(int(rng.integers(1, 500)))
    times = []
    for _ in range(int(rng.integers(0, 60))):
        if rng.uniform() < 0.15:
            times.append(None)
            continue
        d = start + datetime.timedelta(int(rng.integers(-40, (end - start).days + 40)))
        times.append(datetime.datetime(d.year, d.month, d.day, int(rng.integers(0, 24)), int(rng.integers(0, 60))))
    s, e = start.isoformat(), end.isoformat()
    want = _reference_selection(s, e, times)
    nm, nyr, slots, time_idx = _window(s, e, times)
    assert (nm, nyr) == (want[0], want[1])
    assert [(int(mi), int(yi), list(idx)) for mi, yi, idx in slots] == [(int(a), int(b), c) for a, b, c in want[2]]
    assert list(time_idx) == want[3]


def test_window_selection_edge_windows():
    t = lambda *a: datetime.datetime(*a)                    # noqa: E731
    times = [t(2019, 12, 3), None, t(2020, 1, 5), t(2020, 12, 9), t(2019, 11, 30), t(2019, 12, 31, 23)]
    # December -> January: December of both years is averaged (slots (11, 0) and (11, 1)), January never
    nm, nyr, slots, time_idx = _window("2019-12-01", "2020-02-01", times)
    assert (nm, nyr) == (12, 2)
    assert slots == [(11, 0, [0, 5]), (11, 1, [3])]
    assert time_idx == [3]
    # a two-month window averages its last month only
    nm, nyr, slots, time_idx = _window("2019-11-15", "2020-01-01", times)
    assert (nm, nyr, slots, time_idx) == (2, 1, [(1, 0, [0, 5])], [0, 5])
