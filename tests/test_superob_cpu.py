"""Superobservations without a GPU: the host-only entry points (``oisat_superob_boxes``, ``oisat_superob_quanta``) against the
NumPy restatement of tests/superob_cases.py, the two pieces of algebra the merge rests on, and the driver's setting."""
import ctypes as C
import math

import numpy as np
import pytest

import superob_cases as sc
from oisatgmi import _hip, dense
from oisatgmi.driver import oisatgmi

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


# ---- 1. the box table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_deg", [0.1, 0.5, 1.0, 7.0, 180.0])
def test_box_table_against_the_restatement(box_deg):
    """7 does not divide 180: the last band is short.  At 180 the rule as written -- nbands = ceil(180 / 180) -- gives ONE
    band, whose centre is the equator, with n = llrint(360 / 180) = 2 boxes."""
    t = dense.superob_boxes(box_deg)
    n, offset, nbox = sc.box_table(box_deg)
    assert t["nbands"] == n.size == math.ceil(180.0 / box_deg)
    assert t["nbox"] == nbox == int(t["n"].astype(np.int64).sum())
    np.testing.assert_array_equal(t["n"], n)
    np.testing.assert_array_equal(t["offset"], offset)
    assert (t["n"] >= 1).all() and t["offset"][0] == 0
    assert (np.diff(t["offset"]) == t["n"][:-1]).all() and (np.diff(t["offset"]) >= 1).all()
    assert t["offset"][-1] + t["n"][-1] == t["nbox"]
    if box_deg == 7.0:
        assert t["nbands"] == 26 and -90.0 + 25 * 7.0 < 90.0 < -90.0 + 26 * 7.0
        # the short band's centre is the middle of [85, 90), not of [85, 92)
        assert t["n"][-1] == max(1, int(np.rint(360.0 * math.cos(math.radians(87.5)) / 7.0)))
    if box_deg == 180.0:
        assert t["nbands"] == 1 and t["n"].tolist() == [2] and t["nbox"] == 2
    if box_deg == 1.0:
        assert t["n"][89] == t["n"][90] == 360 and (t["n"] == t["n"][::-1]).all()


def test_box_table_rejects_what_the_header_says(lib):
    nb, nx = C.c_int64(-7), C.c_int64(-7)
    n, off = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int64)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 180.0000001, 1e-9):
        assert lib.oisat_superob_boxes(bad, 0, None, None, C.byref(nb), C.byref(nx)) == EINVAL
    assert lib.oisat_superob_boxes(7.0, 4, n.ctypes.data, off.ctypes.data, C.byref(nb), C.byref(nx)) == EINVAL   # 26 bands
    assert lib.oisat_superob_boxes(7.0, 26, None, None, C.byref(nb), C.byref(nx)) == EINVAL
    assert nb.value == -7 and nx.value == -7 and (n == -7).all() and (off == -7).all()


# ---- 2. the quanta ------------------------------------------------------------------------------------------------------------------
QUANTA_CASES = [(4.0, 2.0, 1.0, 1000), (1.0, 1.0, 1.0, 1), (0.0, 0.0, 0.0, 0), (1e12, 1e-3, 5.0, 1 << 20), (3e-9, 1e6, 1e-4, 4099),
                (2.0 ** -40, 2.0 ** 20, 2.0 ** 3, 256), (2.0 ** 41, 0.0, 0.0, 257), (7.3, 0.0, 2.0, 17), (1e-300, 1e-10, 1e-10, 5),
                (1e300, 1.0, 1e4, 100)]


@pytest.mark.parametrize("wmax,dmax,smax,m", QUANTA_CASES)
def test_quanta_against_the_restatement(wmax, dmax, smax, m):
    want = sc.quanta(wmax, dmax, smax, m)
    assert want is not None
    got = dense.superob_quanta(wmax, dmax, smax, m)
    assert got.tobytes() == want.tobytes()
    for q in got:                                               # powers of two, and m terms at the bound stay below 2^63
        assert math.frexp(q)[0] == 0.5
    mm = max(m, 1)
    for q, bound in zip(got, (wmax, math.sqrt(wmax), wmax * dmax, wmax * dmax * dmax, wmax * smax, wmax)):
        assert bound * mm / q + mm / 2 < 2.0 ** 63


def test_quanta_einval(lib):
    q = np.full(6, -7.0)
    for args in ((-1.0, 1.0, 1.0, 10), (1.0, -1.0, 1.0, 10), (1.0, 1.0, -1.0, 10), (float("nan"), 1.0, 1.0, 10),
                 (1.0, float("nan"), 1.0, 10), (1.0, 1.0, 1.0, -1), (1.0, 1.0, 1.0, (1 << 20) + 1), (1e300, 1e10, 1.0, 10),
                 (1e308, 1.0, 1.0, 100), (1e200, 1.0, 1e200, 2), (float("inf"), 0.0, 0.0, 1)):
        assert sc.quanta(*args) is None
        assert lib.oisat_superob_quanta(*[C.c_double(a) for a in args[:3]], args[3], q.ctypes.data) == EINVAL
    assert lib.oisat_superob_quanta(1.0, 1.0, 1.0, 10, None) == EINVAL
    assert (q == -7.0).all()
    with pytest.raises(_hip.OisatError):
        dense.superob_quanta(-1.0, 1.0, 1.0, 10)


# ---- 3. merging co-located observations is exact -----------------------------------------------------------------------------
def test_merging_colocated_observations_is_exact():
    """k = 5 observations at one point with different variances and innovations among 200 others, every one of those alone in
    its 0.25 degree box (asserted).  The analysis of all 205 and that of the 201 restated superobservations (rho = 0) are the
    same analysis: with H the 205 x 201 selection, R^-1-weighted means are sufficient statistics.  Both are solved by a float64
    SciPy Cholesky, which is backward stable: each z is the exact solution of a system perturbed by about n eps relatively, so
    its relative error is at most about n eps cond(S); the increments, C_go sig z with non-negative weights, inherit it.  Bound:
    n eps (cond(S_full) + cond(S_super)) max|increment|, with both condition numbers computed here."""
    rng = np.random.default_rng(4242)
    box, L, k = 0.25, 300.0, 5
    la, lo = np.meshgrid(20.0 + 0.6 * np.arange(10) + 0.11, 40.0 + 0.7 * np.arange(20) + 0.13, indexing="ij")
    lat = np.concatenate([la.ravel(), np.full(k, 23.3712)])
    lon = np.concatenate([lo.ravel(), np.full(k, 47.0193)])
    m = lat.size
    sig = np.concatenate([rng.uniform(0.5, 2.0, 200), np.full(k, 1.3)])
    var = rng.uniform(0.05, 1.0, m)
    d = rng.normal(size=m)
    xyz = sc.unit_vectors(lat, lon)
    ref = sc.ref_superob(lat, lon, xyz, d, sig, var, box)
    assert ref["nused"] == m and sorted(ref["count"].tolist()) == [1] * 200 + [k]
    s = sc.merge(ref)
    glat, glon = np.meshgrid(np.linspace(19.0, 27.0, 17), np.linspace(39.0, 55.0, 33), indexing="ij")
    gxyz, gsig = sc.unit_vectors(glat.ravel(), glon.ravel()), np.full(glat.size, 1.1)
    corr = sc.gaussian(L)
    _, inc_full, S_full = sc.analysis(corr, gxyz, gsig, xyz, sig, var, d)
    _, inc_so, S_so = sc.analysis(corr, gxyz, gsig, sc.unit_vectors(s["lat"], s["lon"]), s["sigma_b"], s["var"], s["d"])
    cond_full, cond_so = np.linalg.cond(S_full), np.linalg.cond(S_so)
    bound = m * np.finfo(np.float64).eps * (cond_full + cond_so) * np.abs(inc_full).max()
    err = np.abs(inc_so - inc_full).max()
    print(f"cond {cond_full:.3e} / {cond_so:.3e}; increments differ by {err:.3e}, bound {bound:.3e}, max |inc| {np.abs(inc_full).max():.3e}")
    assert err <= bound
    assert bound <= 1e-9 * np.abs(inc_full).max()               # (the bound itself says "round-off")


# ---- 4. the variance under a shared correlation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.3, 0.9])
def test_rho_formula_is_the_quadratic_form(rho):
    """var = ((1 - rho) W + rho Q^2) / W^2 is w^T R w / W^2 for R = D^1/2 ((1 - rho) I + rho 1 1^T) D^1/2, D = diag(var),
    w = 1 / var: the variance of the weighted mean under a uniform error correlation rho."""
    rng = np.random.default_rng(77)
    var = rng.uniform(0.01, 3.0, 9)
    sd = np.sqrt(var)
    R = sd[:, None] * ((1.0 - rho) * np.eye(9) + rho * np.ones((9, 9))) * sd[None, :]
    w = 1.0 / var
    W, Q = w.sum(), np.sqrt(w).sum()
    formula = ((1.0 - rho) * W + rho * Q * Q) / (W * W)
    np.testing.assert_allclose(formula, w @ R @ w / (W * W), rtol=1e-13)
    if rho == 0.0:
        np.testing.assert_allclose(formula, 1.0 / W, rtol=1e-15)
    else:
        assert formula > 1.0 / W
    # ... and it is what ``merge`` (the formulas of dense.superob) makes of the sums
    sums = np.zeros((8, 1))
    sums[0], sums[1], sums[5] = W, Q, 1.0
    got = sc.merge({"sums": sums, "count": np.array([9])}, rho)["var"][0]
    np.testing.assert_allclose(got, formula, rtol=1e-15)


# ---- 5. the setting -----------------------------------------------------------------------------------------------------------------
def test_driver_setting_parser():
    f = oisatgmi._superob_setting
    assert f("off") is None and f(" OFF ") is None
    assert f("1") == 1.0 and f("0.75") == 0.75 and f(2) == 2.0 and f(0.5) == 0.5 and f("180") == 180.0
    assert f("auto") == "auto:100000" and f("AUTO") == "auto:100000"
    assert f("auto:3000") == "auto:3000" and f(" auto:1 ") == "auto:1"
    for bad in ("", "on", "0", "-1", "nan", "inf", "181", "1deg", "auto:", "auto:0", "auto:-5", "auto:1.5", "auto:x", "auto3000",
                "buddy", 0, -2.0, float("nan"), True):
        with pytest.raises(ValueError, match="OISAT_OI_SUPEROB"):
            f(bad)
    assert dense.superob_setting(None) == (None, 0) and dense.superob_setting("auto:7") == ("auto", 7)
    assert dense.superob_setting(1.5) == (1.5, 0)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            dense._superob_rho(bad)


def test_tiled_mode_refuses_superobservations(monkeypatch):
    for var in ("OISAT_OI_MODE", "OISAT_OI_SUPEROB", "OISAT_OI_QC", "OISAT_OI_ERROR", "OISAT_CORR_LENGTH_KM", "OISAT_CORRELATION",
                "OISAT_UNOBSERVED"):
        monkeypatch.delenv(var, raising=False)
    o = oisatgmi()
    o.ctm_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.oi_mode, o.oi_superob = "tiled", "1"
    with pytest.raises(ValueError, match="OISAT_OI_SUPEROB.*dense"):
        o.oi("TROPOMI")
    o.oi_superob = None
    monkeypatch.setenv("OISAT_OI_SUPEROB", "auto")
    with pytest.raises(ValueError, match="OISAT_OI_SUPEROB.*dense"):
        o.oi("TROPOMI")
    monkeypatch.setenv("OISAT_OI_SUPEROB", "sometimes")
    o.oi_mode = "dense"
    with pytest.raises(ValueError, match="OISAT_OI_SUPEROB"):
        o.oi("TROPOMI")


def test_ladder_choice_on_counts_handed_in():
    assert dense.SUPEROB_LADDER == (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    counts = dict(zip(dense.SUPEROB_LADDER, (165000, 73000, 41000, 18300, 10300, 4580, 2580, 1150)))
    assert dense.superob_ladder_pick(counts, 100000) == 0.75
    assert dense.superob_ladder_pick(counts, 165000) == 0.5            # "at most": equality fits
    assert dense.superob_ladder_pick(counts, 164999) == 0.75
    assert dense.superob_ladder_pick(counts, 3000) == 4.0
    assert dense.superob_ladder_pick(counts, 1150) == 6.0
    asked = []
    assert dense.superob_ladder_pick(lambda b: asked.append(b) or counts[b], 41000) == 1.0
    assert asked == [0.5, 0.75, 1.0]                                    # (a callable is asked no further than the first fit)
    with pytest.raises(ValueError, match=r"1149.*0\.5: 165000.*6: 1150"):
        dense.superob_ladder_pick(counts, 1149)
