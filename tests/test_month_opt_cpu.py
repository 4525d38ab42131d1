"""CPU-side checks of the device-resident month for satellite_opt records (oisatgmi.month): the lists it refuses before
touching the device, and the field list it regrids, which must be the one interpolator() regrids (interpolator.py:191-283)."""
import numpy as np
import pytest

from oisatgmi import _hip, interpolator as itp, synthetic as syn
from oisatgmi.config import satellite_ssmis
from oisatgmi.month import _refuse, month_average


@pytest.fixture
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the device context was touched")
    monkeypatch.setattr(_hip, "context", refuse)


def _ctm():
    return syn.ctm_monthly(11, 13, 4, 1, 1, lat0=-5.0, lat1=5.0, lon0=-6.0, lon1=6.0)


def _coord(ctm):
    return {"Latitude": ctm[0].latitude, "Longitude": ctm[0].longitude}


def _opt(kind, seed=2):
    return syn.swath_level_granule(seed, kind, nz=3, nscan=20, npix=10)


def _ssmis():
    g = _opt("GOSAT")
    return satellite_ssmis(g.vcd, g.uncertainty, g.time, g.latitude_center, g.longitude_center, False, [], "SSMIS")


@pytest.mark.parametrize("raw,match", [
    (lambda: [_opt("MOPITT"), None, _opt("GOSAT", 3)], "MOPITT and GOSAT"),
    (lambda: [_opt("GOSAT"), _opt("MOPITT", 3)], "MOPITT and GOSAT"),
    (lambda: [_opt("GOSAT"), syn.swath_level_granule(1, "amf", nz=3, nscan=20, npix=10)], "satellite_opt"),
    (lambda: [_opt("MOPITT"), _ssmis()], "SSMIS"),
    (lambda: [_opt("MOPITT"), syn.swath_granule(3, nscan=20, npix=10)], "satellite_opt"),
])
def test_refusals_before_the_device(no_device, raw, match):
    ctm = _ctm()
    with pytest.raises(NotImplementedError, match=match):
        month_average("2019-06-01", "2019-07-01", raw(), ctm, _coord(ctm), interpolator_type=4)


def test_refuse_names_the_family_and_sensor():
    assert _refuse([None, _opt("MOPITT"), _opt("MOPITT", 3)])[1] == "MOPITT"
    assert _refuse([_opt("GOSAT")])[1] == "GOSAT"
    other = _opt("GOSAT")
    other.sensor = "IASI"                  # the default chain refuses it granule by granule (NameError), not here
    assert _refuse([other, _opt("GOSAT", 3)])[1] == "GOSAT"
    assert _refuse([other])[1] is None
    assert _refuse([None, None]) == (None, None)


def _expected_names(g, nz):
    """interpolator.py:191-283: vcd, [tropopause], the a-priori singles that are not all zero, x_col, then the cubes."""
    names = ["vcd"] + (["tropopause"] if np.size(g.tropopause) != 1 else [])
    names += [nm for nm in ("aprior_column", "surface_pressure", "apriori_surface") if getattr(g, nm).any()]
    names.append("x_col")
    cubes = {"MOPITT": [("averaging_kernels", nz + 1)],
             "GOSAT": [("averaging_kernels", nz), ("pressure_weight", nz)]}.get(g.sensor, [])
    cubes += [("pressure_mid", nz), ("apriori_profile", nz)]
    return names + [f"{c}[{z}]" for c, n in cubes for z in range(n)]


class _Recorder:
    """Stands in for the device regridder: records the fields interpolator() hands over, returns an all-NaN granule."""
    seen = None

    def __init__(self, sat_data, *a):
        self.ok = True

    def regrid(self, fields, error=False, device=False):
        _Recorder.seen = list(fields)
        return None, None, np.full((len(fields), 2, 2), np.nan), False


@pytest.mark.parametrize("case", ["MOPITT", "GOSAT", "MOPITT_trop_zero_column", "GOSAT_zero_surface", "IASI", "lattice"])
def test_opt_field_list_is_the_interpolator_order(no_device, monkeypatch, case):
    nz = 3
    g = syn.lattice_l3_granule(4, "MOPITT", nz=nz) if case == "lattice" else _opt(case.split("_")[0] if case != "IASI"
                                                                                  else "GOSAT")
    if case == "IASI":
        g.sensor = "IASI"
    if case == "MOPITT_trop_zero_column":
        g.tropopause = np.full(np.shape(g.vcd), 150.0)
        g.aprior_column = np.zeros_like(g.aprior_column)
    if case == "GOSAT_zero_surface":
        g.apriori_surface = np.zeros_like(g.apriori_surface)
    names, fields, levels = itp._opt_fields(g)
    assert names == _expected_names(g, nz)
    for name, (first, count) in levels.items():
        if count:
            assert names[first:first + count] == [f"{name}[{z}]" for z in range(count)]
        else:
            assert names[first] == name
    # and it is what interpolator() regrids, field for field
    monkeypatch.setattr(itp, "_GranuleRegridder", _Recorder)
    assert itp.interpolator(4, 1.0, g, _coord(_ctm()), 0.75) is None             # all NaN: skipped
    assert len(_Recorder.seen) == len(fields)
    for a, b in zip(_Recorder.seen, fields):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
