"""Host side of the buddy check (no GPU): ``dense.buddy_decide`` on hand-built sums, the driver's ``oi_qc`` setting, and the
planted-outlier recipe through the NumPy restatement of the sums (tests/buddy_cases.py) -- the check that the reference alone
meets the conditions tests/test_gpu_buddy.py puts to the device."""
import numpy as np
import pytest

import buddy_cases as bc
from oisatgmi import dense, driver


def decide(u, n, mean, var, **kw):
    """buddy_decide on sums built from a wanted mean and spread: W = 2, P = W mean, Q = W (var + mean^2)."""
    u, n, mean, var = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (u, n, mean, var))
    W = np.full(u.size, 2.0)
    return dense.buddy_decide(u, n.astype(np.int32), W, W * mean, W * (var + mean * mean), **kw)


# ---- 1. the decision ----------------------------------------------------------------------------------------------------------
def test_each_reason():
    #          kept   background  buddy   not finite  not finite
    u = [0.5, 5.5, 3.5, np.nan, np.inf]
    r = decide(u, [5] * 5, [0.0] * 5, [0.0] * 5)
    assert r.dtype == np.uint8 and r.tolist() == [0, 1, 2, 3, 3]
    assert (dense.QC_KEPT, dense.QC_BACKGROUND, dense.QC_BUDDY, dense.QC_NOT_FINITE) == (0, 1, 2, 3)


def test_order_of_precedence():
    # |u| beyond both thresholds: the background check names it; a u that is not finite is 3 whatever the sums say
    assert decide([9.0], [5], [0.0], [0.0]).tolist() == [1]
    assert decide([-np.inf], [5], [0.0], [0.0]).tolist() == [3]
    r = dense.buddy_decide(np.array([np.nan]), np.array([5]), np.array([np.nan]), np.array([np.nan]), np.array([np.nan]))
    assert r.tolist() == [3]


def test_thresholds_are_strict_and_settable():
    # mean 1, var 3: the threshold is 3 sqrt(1 + 3) = 6 about 1
    assert decide([7.0, 7.0 + 1e-9, -5.0, -5.0 - 1e-9], [3] * 4, [1.0] * 4, [3.0] * 4, k_background=np.inf).tolist() == [0, 2, 0, 2]
    assert decide([5.0, 5.0 + 1e-12, -5.0 - 1e-12], [0] * 3, [0.0] * 3, [0.0] * 3).tolist() == [0, 1, 1]
    assert decide([2.5], [3], [0.0], [0.0], k_buddy=2.0).tolist() == [2]
    assert decide([2.5], [3], [0.0], [0.0], k_background=2.0, k_buddy=9.0).tolist() == [1]


def test_too_few_buddies_fall_back_to_the_background_check():
    assert decide([4.5, 4.5, 5.5], [2, 3, 2], [0.0] * 3, [0.0] * 3).tolist() == [0, 2, 1]
    assert decide([4.5], [4], [0.0], [0.0], min_buddies=5).tolist() == [0]


def test_rows_without_weight():
    u = np.array([4.5, 5.5, np.nan])
    z = np.zeros(3)
    assert dense.buddy_decide(u, np.zeros(3, dtype=np.int32), z, z, z).tolist() == [0, 1, 3]
    # (not what the kernel produces, but a caller's sums may say so: n >= min_buddies with W = 0 has no mean to compare with)
    assert dense.buddy_decide(u, np.full(3, 7, dtype=np.int32), z, z, z).tolist() == [0, 1, 3]


def test_variance_is_clamped_at_zero():
    # Q / W - mean^2 = -1e-3 by rounding of the caller's sums: the spread is 0, not NaN, and the threshold k_buddy
    W, mean = np.full(2, 2.0), np.full(2, 10.0)
    Q = W * (mean * mean - 1e-3)
    r = dense.buddy_decide(np.array([12.9, 13.1]), np.array([4, 4]), W, W * mean, Q, k_background=np.inf)
    assert r.tolist() == [0, 2]
    m, v = dense.buddy_stats(W, W * mean, Q)
    assert v.tolist() == [0.0, 0.0] and m.tolist() == [10.0, 10.0]


# ---- 2. the driver's setting -----------------------------------------------------------------------------------------------------
def test_qc_setting_parser():
    p = driver.oisatgmi._qc_setting
    assert p("off") is None and p(" OFF ") is None
    assert p("buddy") == {"k_buddy": 3.0} and p("Buddy") == {"k_buddy": 3.0}
    assert p("buddy:2.5") == {"k_buddy": 2.5} and p("buddy:4") == {"k_buddy": 4.0} and p("buddy:1e1") == {"k_buddy": 10.0}
    for bad in ("", "on", "1", "0", "buddy:", "buddy:0", "buddy:-1", "buddy:nan", "buddy:inf", "buddy:x", "buddy 3", "buddies", "mc"):
        with pytest.raises(ValueError, match="OISAT_OI_QC"):
            p(bad)


def make_driver(mode, qc=None):
    o = driver.oisatgmi()
    o.ctm_averaged_vcd, o.sat_averaged_vcd = np.ones((4, 8)), np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.grid_lat, o.grid_lon = np.zeros((4, 8)), np.zeros((4, 8))
    o.oi_mode = mode
    if qc is not None:
        o.oi_qc = qc
    return o


@pytest.mark.parametrize("mode", ["dense", "tiled"])
def test_a_bad_setting_is_a_value_error_before_any_device_call(mode, monkeypatch):
    for v in ("OISAT_OI_MODE", "OISAT_CORRELATION", "OISAT_CORR_LENGTH_KM", "OISAT_UNOBSERVED", "OISAT_OI_ERROR", "OISAT_OI_QC"):
        monkeypatch.delenv(v, raising=False)

    def no_device(*a, **k):
        raise AssertionError("the analysis was reached")
    monkeypatch.setattr(driver.oisatgmi, "_oi_spatial", staticmethod(no_device))
    with pytest.raises(ValueError, match="OISAT_OI_QC"):
        make_driver(mode, "bogus").oi("OMI")
    monkeypatch.setenv("OISAT_OI_QC", "buddy:zero")             # the environment variable, read where the attribute is not set
    with pytest.raises(ValueError, match="OISAT_OI_QC"):
        make_driver(mode).oi("OMI")


def test_the_setting_reaches_the_analysis(monkeypatch):
    for v in ("OISAT_OI_MODE", "OISAT_CORRELATION", "OISAT_CORR_LENGTH_KM", "OISAT_UNOBSERVED", "OISAT_OI_ERROR", "OISAT_OI_QC"):
        monkeypatch.delenv(v, raising=False)
    seen = []

    def spy(mode, xa, *a, **k):
        seen.append(k.get("qc", "absent"))
        return tuple(np.zeros(xa.shape) for _ in range(4)), {"mode": mode}
    monkeypatch.setattr(driver.oisatgmi, "_oi_spatial", staticmethod(spy))
    make_driver("dense").oi("OMI")
    make_driver("dense", "buddy:2").oi("OMI")
    monkeypatch.setenv("OISAT_OI_QC", "buddy")
    make_driver("tiled").oi("OMI")
    make_driver("tiled", "off").oi("OMI")                        # the attribute wins over the environment
    assert seen == [None, {"k_buddy": 2.0}, {"k_buddy": 3.0}, None]


def test_diag_mode_ignores_the_setting(monkeypatch):
    monkeypatch.delenv("OISAT_OI_MODE", raising=False)
    monkeypatch.setenv("OISAT_OI_QC", "bogus")
    calls = []

    def fake_oi(xa, y, Sa, So, **k):
        calls.append(k)
        return xa, xa, xa, xa
    monkeypatch.setattr(driver, "OI", fake_oi)
    o = make_driver("diag", "also bogus")
    o.oi("OMI")
    assert len(calls) == 1 and not hasattr(o, "oi_info")


# ---- 3. the planted-outlier recipe on the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_outliers_are_what_the_reference_rejects(seed):
    """Defaults but k_background = inf: only the buddy rule can reject.  All 15 planted observations are rejected, nothing
    else is, the loop ends on a pass that rejects nothing within max_passes = 4, and the clean field rejects nothing."""
    xyz, clean, u, bad = bc.planted_case(seed)
    g = bc.decay(bc.PLANTED["L0"])
    rej, reason, passes, margin = bc.ref_buddy_check(xyz, u, 0, g, k_background=np.inf)
    print(f"seed {seed}: passes {passes}, nearest decision {margin:.2e} from its threshold")
    assert np.flatnonzero(rej).tolist() == bad.tolist() and set(reason[bad].tolist()) == {2}
    assert passes[-1] == 0 and len(passes) <= 4 and sum(passes) == 15
    rej0, _, passes0, _ = bc.ref_buddy_check(xyz, clean, 0, g, k_background=np.inf)
    assert not rej0.any() and passes0 == [0]
