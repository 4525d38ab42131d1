"""The randomized analysis error and averaging kernel, host side (no GPU): the ABI surface, the probe sign, the combination
of the two estimates, the driver's setting, and a float64 restatement of the whole estimator that shows -- without the code
under test -- that the seed and sizes of the GPU end-to-end test stay inside its two statistical conditions."""
import os
import re
import subprocess

import numpy as np
import pytest

import mc_error_cases as mc
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oisat_probe_sign", "oisat_probe_fill", "oisat_trsm_rows_bwd", "oisat_probe_spread", "oisat_probe_diag")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.library_path()):
        import __graft_entry__ as g
        g.build()
    return _hip.load_library()


def test_the_five_symbols_are_exported_and_declared(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oisat.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/oisat.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not exported"
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    table = open(os.path.join(ROOT, "include", "oisat.h")).read()
    assert re.search(r"oisat_gain_solve, oisat_potrs, oisat_trsm_rows_bwd\s+walk the envelope only", table)


def test_probe_sign_is_a_fair_deterministic_counter_hash(lib):
    N = 1 << 16
    seed = 7
    cols = np.arange(N)
    a = mc.np_probe_sign(seed, 3, cols)
    b = mc.np_probe_sign(seed, 4, cols)
    # the C function is the NumPy restatement, entry for entry (a sample of it: every 13th column, and odd corners)
    for c in list(range(0, N, 13)) + [N - 1]:
        assert mc.c_probe_sign(lib, seed, 3, c) == a[c]
    for s, p, c in [(0, 0, 0), (2 ** 64 - 1, 2 ** 40, 2 ** 33 + 5), (12345, 4095, 99999)]:
        v = mc.c_probe_sign(lib, s, p, c)
        assert v in (-1.0, 1.0) and v == mc.np_probe_sign(s, p, c) == mc.c_probe_sign(lib, s, p, c)
    assert set(np.unique(a)) == {-1.0, 1.0}
    assert abs(a.mean()) <= 4 / np.sqrt(N) and abs(b.mean()) <= 4 / np.sqrt(N)
    assert abs((a * b).mean()) <= 4 / np.sqrt(N)                                         # two probes are uncorrelated
    assert abs((a[:-1] * a[1:]).mean()) <= 4 / np.sqrt(N)                                # and so are neighbouring columns
    assert not np.array_equal(a, b)                                                      # differs across probes,
    assert not np.array_equal(a, mc.np_probe_sign(seed + 1, 3, cols))                    # seeds
    assert not np.array_equal(a[:-1], a[1:])                                             # and columns
    out = np.zeros(1, dtype=np.float32)
    assert lib.oisat_probe_sign(1, -1, 0, out.ctypes.data_as(_hip.C.POINTER(_hip.C.c_float))) == -1      # OISAT_EINVAL
    assert lib.oisat_probe_sign(1, 0, 0, None) == -1


def test_combine_error_estimates_on_hand_made_numbers():
    sig2 = np.array([4.0, 4.0, 4.0, 4.0, 4.0, 1.0])
    q = np.array([1.0, 3.0, 5.0, -0.5, 1.0, 0.5])
    q_var = np.array([0.04, 0.09, 0.01, 0.01, 0.04, 0.04])
    # observations: a0 alone on cell 0 (its estimate is the better one), a1 alone on cell 1 (worse), a2 and a3 share cell 4,
    # a4 alone on cell 5 with R below both estimates
    obs_cell = np.array([0, 1, 4, 4, 5])
    R = np.array([2.0, 2.0, 1.0, 1.0, 0.25])
    s = np.array([0.25, 0.25, 0.1, 0.1, -1.0])
    s_var = np.array([0.04 / 16 / 4, 0.09 / 16 * 4, 1e-9, 1e-9, 1e-9])
    A, var = dense.combine_error_estimates(sig2, q, q_var, obs_cell, R, s, s_var)
    np.testing.assert_allclose(A[0], 2.0 * (1 - 2.0 * 0.25))          # selected: R (1 - R s) = 1, variance R^4 s_var = 0.01
    np.testing.assert_allclose(var[0], 0.01)
    np.testing.assert_allclose([A[1], var[1]], [1.0, 0.09])           # not selected: R^4 s_var = 0.36 > 0.09 -> sig2 - q
    np.testing.assert_allclose([A[2], var[2]], [0.0, 0.01])           # sig2 - q = -1 clipped to 0
    np.testing.assert_allclose([A[3], var[3]], [4.0, 0.01])           # sig2 - q = 4.5 clipped to sig2
    np.testing.assert_allclose([A[4], var[4]], [3.0, 0.04])           # two observations on the cell: the first estimate
    np.testing.assert_allclose([A[5], var[5]], [0.25, 0.25 ** 4 * 1e-9])   # R (1 - R s) = 0.3125 clipped to min(sig2, R) = R
    # no observation table: the first estimate everywhere
    A0, var0 = dense.combine_error_estimates(sig2, q, q_var, None, R, s, s_var)
    np.testing.assert_allclose(A0, np.clip(sig2 - q, 0, sig2))
    np.testing.assert_allclose(var0, q_var)
    mean, v = dense._mean_and_var(np.array([8.0]), np.array([40.0]), 4)          # samples 1, 1, 3, 3: mean 2, var of mean 1/3
    np.testing.assert_allclose([mean[0], v[0]], [2.0, (10.0 - 4.0) / 3.0])


def test_driver_setting_for_the_randomized_error(monkeypatch):
    f = oisatgmi._error_setting
    assert f("mc") == ("mc", 256) and f("MC:512") == ("mc", 512) and f(" mc:128 ") == ("mc", 128)
    assert f("1") == (True, 0) and f("yes") == (True, 0) and f(True) == (True, 0)          # what they meant before
    assert f("0") == (False, 0) and f("off") == (False, 0) and f(False) == (False, 0)
    for junk in ("mc:", "mc:abc", "mc:100", "mc:0", "mc:-128", "mcx", "mc512", "mc:1e3"):
        with pytest.raises(ValueError, match="OISAT_OI_ERROR"):
            f(junk)
    o = oisatgmi()
    o.ctm_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.grid_lat, o.grid_lon = syn.global_grid(4, 8)
    o.oi_mode = "tiled"
    monkeypatch.setenv("OISAT_OI_ERROR", "mc:256")
    with pytest.raises(ValueError, match="dense mode"):                  # refused before anything touches the GPU
        o.oi("OMI")
    o.oi_mode = "dense"
    monkeypatch.setenv("OISAT_OI_ERROR", "mc:junk")
    with pytest.raises(ValueError, match="mc or mc:<probes>"):
        o.oi("OMI")


def test_float64_restatement_meets_the_end_to_end_conditions(lib):
    """12 x 24 cells, 300 observations, K = 1024, the seed of the GPU test: exact q and s against their estimates.  The floor
    is float64 rounding through a 300 x 300 solve (1e-10 relative), for the entries that have no sampling noise."""
    case = syn.point_obs_case(12, 24, 300, 11)
    r = mc.restatement(case, 300.0, mc.K_E2E, mc.SEED, lib)
    assert np.all(r["q"] > -1e-12) and np.all(r["q"] <= r["sig2"] * (1 + 1e-12))
    mc.check_conditions(r["q_hat"], np.sqrt(r["q_var"]), r["q"], mc.K_E2E, 1e-10 * r["sig2"], "q (cells)")
    mc.check_conditions(r["s_hat"], np.sqrt(r["s_var"]), r["s"], mc.K_E2E, 1e-10 * r["s"], "s (observations)")
    # the last observation of the latitude order is the entry without noise the floor is there for
    assert r["s_var"][-1] <= 1e-20 * r["s"][-1] ** 2
    # and the combination keeps A inside [0, sig2] within 6 se of the exact error variance
    A, A_var = dense.combine_error_estimates(r["sig2"], r["q_hat"], r["q_var"], None, r["R"], r["s_hat"], r["s_var"])
    assert np.all(np.abs(A - (r["sig2"] - r["q"])) <= 6 * np.sqrt(A_var) + 1e-10 * r["sig2"])
