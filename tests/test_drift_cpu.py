"""The drift of the innovations, host side (no GPU): the float64 reference of tests/drift_cases.py held against what it must
satisfy (it recovers a known truth, it does not depend on the scale of a basis column, degree 0 is the closed form), the
geometry of the cases (the cap is not identifiable, the global ones are, with room), the ABI surface, the host's p x p system
and every refusal that needs no device."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import drift_cases as dc
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oisat_drift_basis", "oisat_cov_residual_multi", "oisat_gain_solve_multi", "oisat_drift_apply", "oisat_drift_quadform")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.library_path()):
        import __graft_entry__ as g
        g.build()
    return _hip.load_library()


@pytest.fixture
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the device context was touched")
    monkeypatch.setattr(_hip, "context", refuse)


def test_the_five_symbols_are_exported_and_declared(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oisat.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/oisat.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not exported"
        assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_entry_points_refuse_bad_arguments_before_the_handle_is_looked_into(lib):
    fake = np.zeros(1 << 16, dtype=np.uint8)                       # (never dereferenced: every call below is refused first)
    h, a, b = fake.ctypes.data, np.zeros(64).ctypes.data, np.zeros(64).ctypes.data
    for args in ((None, a, 4, 1, b, 4), (h, None, 4, 1, b, 4), (h, a, 4, 1, None, 4), (h, a, 4, 4, b, 4), (h, a, 4, -1, b, 4), (h, a, 0, 1, b, 4),
                 (h, a, 4, 1, b, 3)):
        assert lib.oisat_drift_basis(*args) == EINVAL, args
    for args in ((h, 1, a, 4, 4, a, b, None), (h, 1, a, 0, 1, a, b, None), (h, 7, a, 4, 1, a, b, None), (h, 1, a, 4, 1, a, None, None),
                 (h, 1, a, 4, 1, None, b, None), (None, 1, a, 4, 1, a, b, None)):
        assert lib.oisat_drift_apply(*args) == EINVAL, args
    for args in ((h, a, 4, 4, a, 4, a, b), (h, a, 4, 1, a, 3, a, b), (h, a, 0, 1, a, 4, a, b), (h, a, 4, 1, None, 4, a, b), (h, a, 4, 1, a, 4, None, b),
                 (h, a, 4, 1, a, 4, a, None)):
        assert lib.oisat_drift_quadform(*args) == EINVAL, args
    assert not fake.any()


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_the_basis_is_the_harmonics_it_claims_to_be():
    """Every function of degree l is an eigenfunction of the sphere's Laplacian: orthogonal to every function of another degree
    under the uniform measure -- and here to every other function of its own degree as well.  Checked by a Gauss-Legendre x
    uniform quadrature that is exact for polynomials of degree 6."""
    mu, w = np.polynomial.legendre.leggauss(8)
    lon = 2.0 * np.pi * np.arange(16) / 16
    st = np.sqrt(1.0 - mu ** 2)
    xyz = np.array([np.outer(st, np.cos(lon)).ravel(), np.outer(st, np.sin(lon)).ravel(), np.outer(mu, np.ones(16)).ravel()])
    F = dc.basis(xyz, 3)
    assert F.shape == (16, 128)
    G = (F * np.repeat(w, 16)) @ F.T
    off = G - np.diag(np.diag(G))
    assert np.abs(off).max() <= 1e-13 * np.diag(G).max() and (np.diag(G) > 0.1).all()
    for deg, p in ((0, 1), (1, 4), (2, 9)):
        assert np.array_equal(dc.basis(xyz, deg), F[:p])


@pytest.mark.parametrize("model", dc.MODELS)
@pytest.mark.parametrize("m", dc.SIZES)
@pytest.mark.parametrize("degree", dc.DEGREES)
def test_reference_recovers_the_truth_and_ignores_a_columns_scale(m, model, degree):
    d, bt = dc.innovations(m, model, degree)
    ref = dc.gls(m, model, degree, d)
    assert (np.abs(ref["beta"] - bt) <= 4.0 * ref["beta_se"]).all(), (ref["beta"] - bt) / ref["beta_se"]
    # the residual the weights belong to carries no drift: F^T z' = 0
    F = dc.basis(dc.case(m).oxyz, degree).T
    assert np.abs(F.T @ ref["z"]).max() <= 1e-9 * np.abs(F.T @ ref["z_d"]).max()
    # a rescaled column: its coefficient scales back, everything else stays
    k = F.shape[1] - 1
    F2 = F.copy()
    F2[:, k] *= 37.5
    ref2 = dc.gls(m, model, degree, d, F=F2)
    b2 = ref2["beta"].copy()
    b2[k] *= 37.5
    np.testing.assert_allclose(b2, ref["beta"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(ref2["z"], ref["z"], rtol=0, atol=1e-9 * np.abs(ref["z"]).max())
    assert abs(ref2["cond"] - ref["cond"]) <= 1e-6 * ref["cond"]                  # the unit-diagonal scaling removes it
    assert abs(ref2["chi2"] - ref["chi2"]) <= 1e-9 * ref["chi2"]


@pytest.mark.parametrize("model", dc.MODELS)
def test_degree_zero_is_the_closed_form(model):
    m = 333
    d, _ = dc.innovations(m, model, 0)
    ref = dc.gls(m, model, 0, d)
    one = np.ones(m)
    want = (one @ dc.solve64(m, model, d)) / (one @ dc.solve64(m, model, one))
    assert abs(ref["beta"][0] - want) <= 1e-12 * abs(want)
    assert abs(ref["beta_cov"][0, 0] - 1.0 / (one @ dc.solve64(m, model, one))) <= 1e-12 * ref["beta_cov"][0, 0]


@pytest.mark.parametrize("model", dc.MODELS)
def test_the_cap_is_not_identifiable_and_the_global_cases_are_with_room(model):
    """The scaled cond(M) of the reference: beyond 1 / tol for degree 3 in the 20-degree cap, at least a factor 100 inside it for
    every global case."""
    d, _ = dc.innovations(333, model, 3, cap=True)
    cap = dc.gls(333, model, 3, d, cap=True)["cond"]
    print(f"{model}: cap cond {cap:.3g}")
    assert cap > 1.0 / dc.TOL
    for m in dc.SIZES:
        for degree in dc.DEGREES:
            d, _ = dc.innovations(m, model, degree)
            cond = dc.gls(m, model, degree, d)["cond"]
            print(f"{model}: m = {m}, degree {degree}: cond {cond:.3g}")
            assert cond * 100.0 < 1.0 / dc.TOL


# ---- the host's p x p system ---------------------------------------------------------------------------------------------------------
def test_drift_coefficients_match_the_reference_and_refuse_what_the_tolerance_cannot_carry():
    d, _ = dc.innovations(333, "gaussian", 3)
    ref = dc.gls(333, "gaussian", 3, d)
    F = dc.basis(dc.case(333).oxyz, 3).T
    est = dense.drift_coefficients(ref["M"], F.T @ ref["z_d"], dc.TOL)
    np.testing.assert_allclose(est["beta"], ref["beta"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(est["beta_cov"], ref["beta_cov"], rtol=1e-9, atol=1e-14)
    assert abs(est["cond"] - ref["cond"]) <= 1e-9 * ref["cond"] and abs(est["logdet_M"] - ref["logdet_M"]) <= 1e-10 * abs(ref["logdet_M"])
    dcap, _ = dc.innovations(333, "gaussian", 3, cap=True)
    cap = dc.gls(333, "gaussian", 3, dcap, cap=True)
    with pytest.raises(ValueError, match="drift not identifiable"):
        dense.drift_coefficients(cap["M"], np.ones(16), dc.TOL)
    with pytest.raises(ValueError, match="drift not identifiable"):       # not positive definite: the Cholesky (or the spectrum) says so
        dense.drift_coefficients(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2), dc.TOL)
    with pytest.raises(ValueError, match="drift not identifiable"):
        dense.drift_coefficients(np.array([[1.0, 0.0], [0.0, 0.0]]), np.ones(2), dc.TOL)


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------
def test_bad_degrees_are_refused():
    assert dense.drift_degree(None) is None and dense.drift_degree(0) == 0 and dense.drift_degree(np.int64(3)) == 3
    for bad in (-1, 4, 1.0, "1", True, [1]):
        with pytest.raises(ValueError, match="drift is None or a degree"):
            dense.drift_degree(bad)


def test_run_refuses_before_the_device():
    p = dense.DenseAnalysis.__new__(dense.DenseAnalysis)               # (no context: touching the device is an AttributeError)
    p.m, p._g, p._kind, p._drift = 3, None, 0, None
    with pytest.raises(ValueError, match="drift is None or a degree"):
        p.run(300.0, drift=4)
    with pytest.raises(ValueError, match="drift not identifiable: 3 observations for 4 coefficients"):
        p.run(300.0, drift=1)
    for call in (p.drift_estimate, p.drift_variance):
        with pytest.raises(ValueError, match="must follow run"):
            call()


def test_oi_dense_refuses_before_the_device(no_device):
    c = syn.diag_case(4, 8, 10, 1)
    args = (c.Xa.copy(), c.Y.copy(), c.Sa, c.So, c.lat, c.lon, 300.0)
    for bad in (-1, 4, 2.0, "2", True):
        with pytest.raises(ValueError, match="drift is None or a degree"):
            dense.OI_dense(*args, drift=bad)
    with pytest.raises(ValueError, match="drift cannot be combined with fit_scale"):
        dense.OI_dense(*args, drift=1, fit_scale="background")
    with pytest.raises(ValueError, match="drift cannot be combined with ensemble"):
        dense.OI_dense(*args, drift=1, ensemble=32)
    with pytest.raises(ValueError, match="drift cannot be combined with regions"):
        dense.OI_dense(*args, drift=1, regions=np.ones((4, 8), dtype=int))


def test_driver_setting_for_the_drift(no_device, monkeypatch):
    f = oisatgmi._drift_setting
    assert f("off") is None and f(" OFF ") is None and f("0") == 0 and f(3) == 3 and f(" 2 ") == 2
    for junk in ("", "4", "-1", "1.5", "on", "1:2"):
        with pytest.raises(ValueError, match="OISAT_OI_DRIFT"):
            f(junk)
    o = oisatgmi()
    o.ctm_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.grid_lat, o.grid_lon = syn.global_grid(4, 8)
    monkeypatch.setenv("OISAT_OI_DRIFT", "1")
    for mode in ("tiled", "diag"):
        o.oi_mode = mode
        with pytest.raises(ValueError, match="dense mode"):
            o.oi("OMI")
    o.oi_mode = "dense"
    monkeypatch.setenv("OISAT_OI_DRIFT", "5")
    with pytest.raises(ValueError, match="a degree 0..3"):
        o.oi("OMI")
    monkeypatch.setenv("OISAT_OI_DRIFT", "1")                      # the combinations are refused with the other option checks
    monkeypatch.setenv("OISAT_OI_SCALE", "ml")
    with pytest.raises(ValueError, match="oi_drift cannot be combined with OISAT_OI_SCALE"):
        o.oi("OMI")
    monkeypatch.delenv("OISAT_OI_SCALE")
    monkeypatch.setenv("OISAT_OI_ENSEMBLE", "32")
    with pytest.raises(ValueError, match="oi_drift cannot be combined with OISAT_OI_ENSEMBLE"):
        o.oi("OMI")
    monkeypatch.delenv("OISAT_OI_ENSEMBLE")
    o.oi_regions = np.ones((4, 8), dtype=int)
    with pytest.raises(ValueError, match="oi_drift cannot be combined with OISAT_OI_REGIONS"):
        o.oi("OMI")


def test_the_neighbours_are_untouched():
    """``drift`` is a trailing keyword with the default None wherever it was added, and the draws of the ensembles do not know it."""
    for fn in (dense.DenseAnalysis.run, dense.OI_dense):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "drift" and params[-1].default is None
    assert "drift" not in inspect.signature(dense.ensemble_draws).parameters
    a = dense.ensemble_draws("gaussian", 400.0, range(4), 8, 5, 3)
    dense.drift_coefficients(np.eye(2), np.ones(2), 1e-6)
    b = dense.ensemble_draws("gaussian", 400.0, range(4), 8, 5, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
