"""Host side of the correlation-length estimate (no GPU): the fixed-point quanta of ``oisat_covariogram`` against a Python
restatement, ``fit_correlation`` on covariograms whose answer is known, the driver's ``corr_length_km = "auto"`` with the device
functions replaced, and what the fixed-point rounding can do to a fitted length."""
import ctypes as C
import itertools

import numpy as np
import pytest

import covariogram_cases as cc
from oisatgmi import _hip, dense

MODELS = ("gaussian", "gaspari_cohn", "soar")


# ---- 1. the quanta -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("umax,m", list(itertools.product((0.0, 1e-30, 1.0, 3.7, 1e12), (0, 1, 2, 257, 99898, 1 << 20))))
def test_quantum_rule(umax, m):
    lib = _hip.load_library()
    qp, qc = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.oisat_covariogram_quantum(umax, m, C.byref(qp), C.byref(qc)) == 0
    assert (qp.value, qc.value) == cc.quanta_ref(umax, m)
    assert dense.covariogram_quantum(umax, m) == (qp.value, qc.value)
    # what the rule is for: P terms of at most umax^2 / q_prod (2 / q_chord) plus their roundings stay below 2^63
    P = m * (m - 1) // 2
    assert P * (umax * umax / qp.value + 0.5) < 2.0 ** 63 and P * (2.0 * (1 + 2.0 ** -50) / qc.value + 0.5) < 2.0 ** 63


def test_quantum_rejects_what_the_kernel_rejects():
    lib = _hip.load_library()
    qp, qc = C.c_double(-1.0), C.c_double(-1.0)
    for umax, m in ((1.0, (1 << 20) + 1), (1.0, -1), (-1.0, 10), (float("nan"), 10), (1e200, 10)):
        assert lib.oisat_covariogram_quantum(umax, m, C.byref(qp), C.byref(qc)) == -1        # OISAT_EINVAL
        assert (qp.value, qc.value) == (-1.0, -1.0)
    with pytest.raises(_hip.OisatError):
        dense.covariogram_quantum(1.0, (1 << 20) + 1)


# ---- 2. the fit ----------------------------------------------------------------------------------------------------------------
def model_covariogram(corr, L0, scale=0.6, nbins=64, max_km=2000.0, count=1000):
    r = (np.arange(nbins) + 0.5) * (max_km / nbins)
    chord = r / dense.EARTH_RADIUS_KM
    cov = scale * dense._corr_at(dense.corr_kind(corr), L0, np.ascontiguousarray(chord ** 2))
    return {"chord": chord, "r_km": r, "cov": cov, "count": np.full(nbins, count, dtype=np.int64), "max_km": max_km, "nbins": nbins}


@pytest.mark.parametrize("corr", MODELS)
@pytest.mark.parametrize("L0", [150.0, 300.0, 800.0])
def test_fit_recovers_a_noise_free_model(corr, L0):
    """1e-6 relative: three orders above the 1e-9 bracket of the golden-section search, which covers the flatness of J at its
    minimum (measured: 9e-11 at worst over the nine cases)."""
    f = dense.fit_correlation(model_covariogram(corr, L0), corr)
    print(f"{corr} L0 {L0}: L {f['L_km'] / L0 - 1:+.2e}, scale {f['scale'] / 0.6 - 1:+.2e}, rms {f['rms']:.2e}")
    assert f["found"] and not f["at_bound"] and f["corr"] == corr and f["nbins_used"] == 64
    assert abs(f["L_km"] / L0 - 1) <= 1e-6 and abs(f["scale"] / 0.6 - 1) <= 1e-6


def test_fit_flat_and_rising():
    cg = model_covariogram("gaussian", 300.0)
    cg["cov"] = np.zeros(64)
    f = dense.fit_correlation(cg)
    assert f["found"] is False and f["scale"] == 0.0
    cg["cov"] = 0.1 + 0.1 * cg["r_km"] / 2000.0                  # still rising at max_km: the flattest model on offer
    f = dense.fit_correlation(cg)
    assert f["at_bound"] is True and f["found"] is True and abs(f["L_km"] / 2000.0 - 1) < 1e-9
    f = dense.fit_correlation(cg, L_bounds=(50.0, 500.0))
    assert f["at_bound"] is True and abs(f["L_km"] / 500.0 - 1) < 1e-9


def test_fit_needs_three_bins():
    cg = model_covariogram("gaussian", 300.0)
    cg["count"] = np.where(np.arange(64) < 2, 1000, 29)
    f = dense.fit_correlation(cg)
    assert f["found"] is False and f["nbins_used"] == 2
    cg["count"][2] = 30
    f = dense.fit_correlation(cg)
    assert f["nbins_used"] == 3 and f["found"] is True
    cg["cov"][5] = np.nan                                         # an empty bin's NaN is never read
    cg["count"][5] = 0
    assert dense.fit_correlation(cg)["found"] is True


@pytest.mark.parametrize("corr", MODELS)
def test_fit_picks_the_generating_model(corr):
    f = dense.fit_correlation(model_covariogram(corr, 300.0), list(MODELS))
    assert f["corr"] == corr and sorted(f["all"]) == sorted(MODELS)
    assert all(f["rms"] <= g["rms"] for g in f["all"].values())
    assert abs(f["L_km"] / 300.0 - 1) <= 1e-6
    with pytest.raises(ValueError):
        dense.fit_correlation(model_covariogram(corr, 300.0), "banana")


# ---- 3. the driver's setting ----------------------------------------------------------------------------------------------------
@pytest.fixture
def facade(monkeypatch):
    """A facade on a 4 x 8 grid whose device functions are replaced: records what ``OI_dense`` / ``OI_tiled`` were given."""
    from oisatgmi import optimal_interpolation as oi_mod
    from oisatgmi.driver import oisatgmi
    for v in ("OISAT_OI_MODE", "OISAT_CORRELATION", "OISAT_CORR_LENGTH_KM", "OISAT_UNOBSERVED", "OISAT_OI_ERROR"):
        monkeypatch.delenv(v, raising=False)
    calls = {"L": [], "fit": []}
    state = {"found": True}

    def fake_analysis(xa, y, Sa, So, lat, lon, L, **kw):
        calls["L"].append(L)
        return np.array(xa), np.zeros(np.shape(xa)), {"nobs": 3}

    def fake_estimate(Xa, Y, Sa, So, lat, lon, scale=1.0, corr="gaussian", **kw):
        calls["fit"].append((scale, corr))
        return {"L_km": 432.1 if state["found"] else float("nan"), "scale": 0.5, "rms": 0.01, "corr": corr, "found": state["found"],
                "at_bound": False, "nbins_used": 40, "covariogram": {"count": np.zeros(64)}}

    monkeypatch.setattr(oi_mod, "regularization_pick", lambda Sa, So, reg_index: (7, 0.25, None, True))
    monkeypatch.setattr(dense, "OI_dense", fake_analysis)
    monkeypatch.setattr(dense, "OI_tiled", fake_analysis)
    monkeypatch.setattr(dense, "estimate_corr_length", fake_estimate)
    o = oisatgmi()
    rng = np.random.default_rng(5)
    o.ctm_averaged_vcd, o.sat_averaged_vcd = rng.uniform(1, 2, (4, 8)), rng.uniform(1, 2, (4, 8))
    o.sat_averaged_error = np.full((4, 8), 0.3)
    o.grid_lat, o.grid_lon = np.meshgrid(np.linspace(-60, 60, 4), np.linspace(-150, 150, 8), indexing="ij")
    o.oi_want_error = "0"
    return o, calls, state


@pytest.mark.parametrize("mode", ["dense", "tiled"])
def test_driver_auto(facade, monkeypatch, capsys, mode):
    o, calls, state = facade
    o.oi_mode, o.corr_length_km, o.oi_correlation = mode, "auto", "soar"
    o.oi("OMI")
    assert calls["L"] == [432.1] and calls["fit"] == [(0.25, "soar")]
    assert o.oi_info["corr_length_km"] == 432.1 and o.oi_info["corr_fit"]["found"] is True
    assert "covariogram" not in o.oi_info["corr_fit"] and o.oi_info["corr_fit"]["nbins_used"] == 40
    o.corr_length_km = None                                      # the environment, any case
    monkeypatch.setenv("OISAT_CORR_LENGTH_KM", "AUTO")
    o.oi("OMI")
    assert calls["L"] == [432.1, 432.1]
    state["found"] = False                                       # no fit: 300 km, one printed line, found False in the info
    capsys.readouterr()
    o.oi("OMI")
    assert calls["L"][-1] == 300.0 and o.oi_info["corr_length_km"] == 300.0 and o.oi_info["corr_fit"]["found"] is False
    assert capsys.readouterr().out.count("No correlation length could be fitted") == 1


def test_driver_numbers_and_nonsense_are_as_before(facade, monkeypatch):
    o, calls, state = facade
    o.oi_mode = "dense"
    for v, want in (("450", 450.0), (275.5, 275.5), (None, 300.0)):
        o.corr_length_km = v
        o.oi("OMI")
        assert calls["L"][-1] == want and type(calls["L"][-1]) is float and "corr_fit" not in o.oi_info
    monkeypatch.setenv("OISAT_CORR_LENGTH_KM", "620")
    o.oi("OMI")
    assert calls["L"][-1] == 620.0 and calls["fit"] == []
    for bad in ("banana", "automatic", "auto km"):
        o.corr_length_km = bad
        with pytest.raises(ValueError):
            o.oi("OMI")


# ---- 4. what the fixed-point rounding can do to the fitted length -----------------------------------------------------------------
def test_rounding_cannot_move_the_fit():
    """The end-to-end draw (1500 global points, Gaussian, 400 km): sum_prod of every bin moved by +-count q_prod / 2 -- the bound of
    the device's rounding, all terms of a bin erring the same way -- random signs, 20 draws.  Largest relative shift of the fitted
    L measured: 1.7e-8 (of the scale: 1.7e-8), which is the resolution of the golden-section search on a J that does not reach
    zero (sqrt of the double's epsilon), not the perturbation (q_prod = 2^-38 = 3.6e-12 here, against mean products of 1e-2 ..
    5e-1).  Asserted below 1e-7; the basis of the 1e-6 of the GPU end-to-end test."""
    lat, lon, u, count, sp, sc = cc.end_to_end_case()
    c = cc.END_TO_END
    q_prod, q_chord = cc.quanta_ref(np.abs(u).max(), c["m"])
    var0 = float(np.mean(u * u))
    base = dense.fit_correlation(cc.covariogram_dict(count, sp, sc, c["max_km"], c["m"], var0, q_prod, q_chord))
    assert base["found"] and not base["at_bound"] and base["nbins_used"] >= 60
    print(f"reference fit: L {base['L_km']:.3f} km, scale {base['scale']:.4f}, q_prod {q_prod:.3e}")
    rng = np.random.default_rng(99)
    worst_L = worst_s = 0.0
    for _ in range(20):
        sign = rng.choice([-1.0, 1.0], size=count.size)
        f = dense.fit_correlation(cc.covariogram_dict(count, sp + sign * count * (q_prod / 2), sc, c["max_km"], c["m"], var0,
                                                      q_prod, q_chord))
        worst_L = max(worst_L, abs(f["L_km"] / base["L_km"] - 1))
        worst_s = max(worst_s, abs(f["scale"] / base["scale"] - 1))
    print(f"largest relative shift over 20 draws: L {worst_L:.3e}, scale {worst_s:.3e}")
    assert worst_L < 1e-7 and worst_s < 1e-7
