"""The posterior ensemble, host side (no GPU): the ABI surface, the draws and their spectral measures, every refusal that needs
no device, and the float64 restatement of Matheron's rule held against the exact analysis error variance -- which guards the
restatement that tests/test_gpu_ensemble.py compares the device with, not the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import ensemble_cases as ec
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oisat_field_sample", "oisat_member_spread")
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


def test_the_two_symbols_are_exported_and_declared(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oisat.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/oisat.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not exported"
        assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_entry_points_refuse_bad_arguments_before_the_handle_is_looked_into(lib):
    fake = np.zeros(1 << 16, dtype=np.uint8)                       # (never dereferenced: every call below is refused first)
    h, a = fake.ctypes.data, np.zeros(8).ctypes.data
    good = dict(h=h, pxyz=a, npts=2, scale=None, omega=a, phase=a, F=1, K=1, noise=None, nscale=None, out=a, ld=2)
    for change in (dict(h=None), dict(pxyz=None), dict(omega=None), dict(phase=None), dict(out=None), dict(npts=0), dict(ld=1), dict(F=0),
                   dict(K=0), dict(K=65536), dict(noise=a), dict(nscale=a)):
        v = {**good, **change}
        rc = lib.oisat_field_sample(v["h"], v["pxyz"], v["npts"], v["scale"], v["omega"], v["phase"], v["F"], v["K"], v["noise"], v["nscale"],
                                    v["out"], v["ld"])
        assert rc == EINVAL, change
    good = dict(h=h, ny=2, nx=2, U=a, K=32, ldu=4, m=4, P=a, ldp=4, s2=a)
    for change in (dict(h=None), dict(U=None), dict(P=None), dict(s2=None), dict(K=48), dict(K=0), dict(K=4128), dict(ldu=3), dict(ldp=3),
                   dict(m=0), dict(ny=0)):
        v = {**good, **change}
        rc = lib.oisat_member_spread(v["h"], a, a, v["ny"], v["nx"], a, a, v["U"], v["K"], v["ldu"], v["m"], 1.0, None, None, v["P"], v["ldp"],
                                     0, v["s2"], a)
        assert rc == EINVAL, change
    assert not fake.any()


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_draws_have_their_shapes_and_member_k_is_member_k(corr):
    omega, phase, eps = dense.ensemble_draws(corr, 400.0, range(64), 48, 37, 5)
    assert omega.shape == (64, 48, 3) and phase.shape == (64, 48) and eps.shape == (64, 37)
    assert omega.dtype == phase.dtype == eps.dtype == np.float64
    assert (phase >= 0).all() and (phase < 1).all() and np.isfinite(omega).all()
    for k in (0, 17, 63):                                            # the same member alone, and in another list
        o1, p1, e1 = dense.ensemble_draws(corr, 400.0, [k], 48, 37, 5)
        assert np.array_equal(o1[0], omega[k]) and np.array_equal(p1[0], phase[k]) and np.array_equal(e1[0], eps[k])
    o2, p2, e2 = dense.ensemble_draws(corr, 400.0, [63, 3], 48, 37, 5)
    assert np.array_equal(o2[1], omega[3]) and np.array_equal(e2[0], eps[63])
    o3, p3, e3 = dense.ensemble_draws(corr, 400.0, range(4), 48, 37, 6)                # another seed: other numbers
    assert not np.array_equal(o3, omega[:4]) and not np.array_equal(p3, phase[:4]) and not np.array_equal(e3, eps[:4])
    assert not np.array_equal(omega[0], omega[1]) and not np.array_equal(eps[0], eps[1])
    # turns per unit chord: the angular frequency scales with R_earth / L
    o4 = dense.ensemble_draws(corr, 800.0, [0], 48, 37, 5)[0]
    np.testing.assert_allclose(o4[0], omega[0] / 2.0, rtol=1e-14)
    assert dense.ensemble_draws(corr, 400.0, [], 4, 0, 0)[0].shape == (0, 4, 3)


def test_gaspari_cohn_and_junk_are_refused():
    with pytest.raises(ValueError, match="no closed-form sampler.*gaussian and soar"):
        dense.ensemble_draws("gaspari_cohn", 400.0, range(2), 8, 5, 0)
    with pytest.raises(ValueError, match="corr must be"):
        dense.ensemble_draws("matern", 400.0, range(2), 8, 5, 0)
    with pytest.raises(ValueError):
        dense.ensemble_draws("gaussian", 400.0, range(2), 0, 5, 0)
    with pytest.raises(ValueError):
        dense.ensemble_draws("gaussian", 400.0, [-1], 8, 5, 0)


@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_the_frequencies_have_the_correlations_spectral_measure(lib, corr):
    """L = 400 km, 2e5 frequencies: the mean of cos 2 pi (omega . Delta) is within 5 of its own standard errors of the correlation
    ``oisat_corr_eval`` gives at the chords 0.01, 0.05, 0.1 and 0.3 (in three directions)."""
    L, N = 400.0, 200_000
    omega = dense.ensemble_draws(corr, L, [0], N, 0, 11)[0][0]                          # (N, 3)
    g = dense.decay_constant(L)
    for chord in (0.01, 0.05, 0.1, 0.3):
        for u in (np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, -0.8]), np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)):
            c = np.cos(2.0 * np.pi * (omega @ (chord * u)))
            want = np.empty(1)
            assert lib.oisat_corr_eval(ec.KINDS[corr], g, np.array([chord ** 2]).ctypes.data, 1, want.ctypes.data) == 0
            se = c.std(ddof=1) / np.sqrt(N)
            print(f"{corr}, chord {chord}: mean {c.mean():.5f}, C {want[0]:.5f}, {abs(c.mean() - want[0]) / se:.2f} se")
            assert abs(c.mean() - want[0]) <= 5.0 * se


# ---- the restatement against the exact analysis error ----------------------------------------------------------------------------
@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_float64_restatement_of_matherons_rule_meets_the_exact_error_variance(lib, corr):
    """8 x 16 cells, 40 observations, L = 1500 km, K = 4096, F = 128: the ensemble variance against the exact A on every cell
    under the two conditions, and at most 2 % of the cells beyond 3 se.  Floor: float64 rounding through a 40 x 40 solve."""
    K, F = 4096, 128
    sysm = ec.System(syn.point_obs_case(8, 16, 40, 3), 1500.0, corr, lib)
    assert np.all(sysm.A > 0) and np.all(sysm.A <= sysm.gsig ** 2)
    A_hat, A_var = sysm.ensemble_variance(K, F, ec.SEED)
    ec.check_conditions(A_hat, np.sqrt(A_var), sysm.A, K, 1e-10 * sysm.gsig ** 2, f"A (cells), {corr}")
    share = ec.beyond_three(A_hat, np.sqrt(A_var), sysm.A)
    print(f"{corr}: {100 * share:.2f} % of the cells beyond 3 se (bound 2 %); median se / A = {np.median(np.sqrt(A_var) / A_hat):.4f}")
    assert share <= 0.02


def test_the_restatement_passes_the_gpu_tests_statistical_case(lib):
    """The case of the GPU's statistical test -- 16 x 32 cells, 150 observations, K = 1024, F = 256, its seed -- in float64: the
    seed is shown to pass here before the device is held to it."""
    for corr in ("gaussian", "soar"):
        sysm = ec.System(ec.stat_case(), ec.STAT_L, corr, lib)
        A_hat, A_var = sysm.ensemble_variance(ec.STAT_K, ec.STAT_F, ec.SEED)
        ec.check_conditions(A_hat, np.sqrt(A_var), sysm.A, ec.STAT_K, 1e-10 * sysm.gsig ** 2, f"A (cells), {corr}")
        assert ec.beyond_three(A_hat, np.sqrt(A_var), sysm.A) <= 0.02
        # ... and the three regional means of the cross-check
        W = dense.region_weights(ec.stat_regions(), ec.stat_case().lat)[1].reshape(3, -1)
        import scipy.linalg as sla
        GW = W @ sysm.G
        Bw = ec.corr64(lib, sysm.kind, sysm.g, sysm.pg, sysm.pg) * sysm.gsig[:, None] * sysm.gsig[None, :]
        exact = np.diag(W @ Bw @ W.T - GW @ sla.cho_solve(sla.cho_factor(sysm.S, lower=True), GW.T))
        f = np.concatenate([sysm.deviations(range(k0, k0 + 512), ec.STAT_F, ec.SEED) @ W.T for k0 in range(0, ec.STAT_K, 512)])
        v, vv = ec.mean_var((f ** 2).sum(axis=0), (f ** 4).sum(axis=0), ec.STAT_K)
        ec.check_conditions(v, np.sqrt(vv), exact, ec.STAT_K, 1e-10 * exact, f"regional means, {corr}")


# ---- refusals that need no device --------------------------------------------------------------------------------------------------
def _bare_plan(m=5, g=1.0, kind=0):
    p = dense.DenseAnalysis.__new__(dense.DenseAnalysis)               # (no context: touching the device is an AttributeError)
    p.m, p._g, p._kind = m, g, kind
    return p


def test_posterior_ensemble_refuses_before_the_device():
    with pytest.raises(ValueError, match="must follow run"):
        _bare_plan(m=0).posterior_ensemble()
    with pytest.raises(ValueError, match="must follow run"):
        _bare_plan(g=None).posterior_ensemble()
    for bad in (0, 16, 48, -32, 32.5, "many"):
        with pytest.raises(ValueError, match="nmember"):
            _bare_plan().posterior_ensemble(nmember=bad)
    with pytest.raises(ValueError, match="nfeature"):
        _bare_plan().posterior_ensemble(nfeature=0)
    with pytest.raises(ValueError, match="gaspari_cohn"):
        _bare_plan(kind=dense.CORRELATIONS["gaspari_cohn"]).posterior_ensemble()
    with pytest.raises(ValueError, match="nmember"):
        _bare_plan().prior_ensemble(300.0, nmember=40)


def test_oi_dense_refuses_before_the_device(no_device):
    c = syn.diag_case(4, 8, 10, 1)
    args = (c.Xa.copy(), c.Y.copy(), c.Sa, c.So, c.lat, c.lon, 300.0)
    with pytest.raises(ValueError, match="nmember"):
        dense.OI_dense(*args, ensemble=48)
    with pytest.raises(ValueError, match="nfeature"):
        dense.OI_dense(*args, ensemble=32, ensemble_features=0)
    with pytest.raises(ValueError, match="gaspari_cohn"):
        dense.OI_dense(*args, ensemble=32, corr="gaspari_cohn")


def test_driver_setting_for_the_ensemble(no_device, monkeypatch):
    f = oisatgmi._ensemble_setting
    assert f("off") is None and f(" OFF ") is None
    assert f("32") == (32, 256) and f(64) == (64, 256) and f("128:64") == (128, 64) and f(" 96:1 ") == (96, 1)
    for junk in ("", "0", "48", "-32", "32:", "32:0", ":64", "32:64:2", "many", "32.5", "1e2", "on"):
        with pytest.raises(ValueError, match="OISAT_OI_ENSEMBLE"):
            f(junk)
    o = oisatgmi()
    o.ctm_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.grid_lat, o.grid_lon = syn.global_grid(4, 8)
    monkeypatch.setenv("OISAT_OI_ENSEMBLE", "32")
    for mode in ("tiled", "diag"):
        o.oi_mode = mode
        with pytest.raises(ValueError, match="dense mode"):
            o.oi("OMI")
    o.oi_mode = "dense"
    monkeypatch.setenv("OISAT_OI_ENSEMBLE", "32:junk")
    with pytest.raises(ValueError, match="<members>:<features>"):
        o.oi("OMI")
    monkeypatch.delenv("OISAT_OI_ENSEMBLE")
    o.oi_ensemble = 40
    with pytest.raises(ValueError, match="multiple of 32"):
        o.oi("OMI")
