"""``oisat_covariogram`` at the C ABI against the NumPy restatement of its pair rule (tests/covariogram_cases.py: pairs from
``np.triu_indices``, counts by ``np.bincount``, sums by ``math.fsum``), then the estimate through ``dense`` and the driver.

Bounds per bin, all derived from the fixed-point rule (include/oisat.h), with the test's own quanta (``oisat_covariogram_quantum``):
count equal; |sum_prod - ref| <= count q_prod / 2 + 2^-52 |ref| (one rounding of at most half a quantum per term, the last bit of
the output); |sum_chord - ref| <= count (q_chord / 2 + 2^-51) + 2^-52 |ref| (the same, plus the device's square root: a chord is
at most 2, an ulp of it at most 2^-51).  Every parity case first asserts that no pair sits within 1e-9 of a bin edge."""
import ctypes as C

import numpy as np
import pytest

import covariogram_cases as cc
from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def device_covariogram(ctx, xyz, d, w, max_chord, nbins, olat=None, m=None):
    """-> (rc, count, sum_prod, sum_chord, nobs_used); the outputs start as SENTINEL."""
    m = int(np.size(d)) if m is None else m
    n = max(int(nbins), 1)
    count = np.full(min(n, 2048), int(SENTINEL), dtype=np.int64)
    sp, sc = np.full(count.size, SENTINEL), np.full(count.size, SENTINEL)
    used = C.c_int64(int(SENTINEL))
    bufs = {k: ctx.upload(np.ascontiguousarray(v, dtype=np.float64)) for k, v in (("xyz", xyz), ("d", d), ("w", w), ("olat", olat))
            if v is not None and np.size(v)}
    ptr = {k: (bufs[k].ptr if k in bufs else None) for k in ("xyz", "d", "w", "olat")}
    try:
        rc = ctx.lib.oisat_covariogram(ctx.h, ptr["xyz"], ptr["d"], ptr["w"], m, float(max_chord), int(nbins), ptr["olat"],
                                       count.ctypes.data, sp.ctypes.data, sc.ctypes.data, C.byref(used))
    finally:
        for b in bufs.values():
            b.free()
    return rc, count, sp, sc, int(used.value)


def quanta(ctx, u, m):
    fin = np.isfinite(u)
    qp, qc = C.c_double(0.0), C.c_double(0.0)
    assert ctx.lib.oisat_covariogram_quantum(float(np.abs(u[fin]).max()) if fin.any() else 0.0, m, C.byref(qp), C.byref(qc)) == 0
    return qp.value, qc.value


def check_against_numpy(ctx, xyz, d, w, max_chord, nbins, got, what):
    with np.errstate(invalid="ignore", over="ignore"):
        u = d if w is None else d * w
    m = int(u.size)
    rc, count, sp, sc, used = got
    assert rc == 0
    rcount, rsp, rsc = cc.ref_covariogram(xyz, u, max_chord, nbins)
    q_prod, q_chord = quanta(ctx, u, m)
    assert used == int(np.isfinite(u).sum())
    np.testing.assert_array_equal(count, rcount)
    tol_p = rcount * (q_prod / 2) + 2.0 ** -52 * np.abs(rsp)
    tol_c = rcount * (q_chord / 2 + 2.0 ** -51) + 2.0 ** -52 * np.abs(rsc)
    ep, ec = np.abs(sp - rsp), np.abs(sc - rsc)
    print(f"{what}: pairs binned {int(rcount.sum())}, q_prod {q_prod:.3e}, q_chord {q_chord:.3e}; worst sum_prod error / bound "
          f"{np.max(ep / np.maximum(tol_p, 1e-300)):.3f}, sum_chord {np.max(ec / np.maximum(tol_c, 1e-300)):.3f}")
    assert np.all(ep <= tol_p) and np.all(ec <= tol_c)
    return rcount, rsp, rsc


# ---- 1. sizes around the block edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_w", [True, False])
@pytest.mark.parametrize("max_chord", [0.3, 2.5])
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 700])
def test_sizes_around_the_block_edges(ctx, m, max_chord, with_w):
    rng = np.random.default_rng(1000 + m)
    xyz = cc.cap_points(rng, m, 20.0)
    d = rng.normal(size=m)
    w = rng.uniform(0.5, 2.0, m) if with_w else None
    got = device_covariogram(ctx, xyz, d, w, max_chord, 64)
    rcount, _, _ = check_against_numpy(ctx, xyz, d, w, max_chord, 64, got, f"m {m}, max_chord {max_chord}")
    if max_chord == 2.5:
        assert rcount.sum() == m * (m - 1) // 2                 # every pair is inside
    elif m >= 255:
        assert 0 < rcount.sum() < m * (m - 1) // 2


# ---- 2. the latitude window ------------------------------------------------------------------------------------------------------
def test_window_changes_no_bit(ctx):
    rng = np.random.default_rng(2025)
    lat, lon = cc.global_points(rng, 1300)
    xyz = cc.unit_vectors(lat, lon)
    d, w = rng.normal(size=1300), rng.uniform(0.5, 2.0, 1300)
    a = device_covariogram(ctx, xyz, d, w, 0.157, 64, olat=lat)
    b = device_covariogram(ctx, xyz, d, w, 0.157, 64)
    for x, y in zip(a[1:4], b[1:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4] == 1300
    check_against_numpy(ctx, xyz, d, w, 0.157, 64, a, "1300 global points, windowed")


# ---- 3. order independence -----------------------------------------------------------------------------------------------------
def test_order_and_repetition_change_no_bit(ctx):
    rng = np.random.default_rng(1700)
    xyz = cc.cap_points(rng, 700, 20.0)
    d, w = rng.normal(size=700), rng.uniform(0.5, 2.0, 700)
    a = device_covariogram(ctx, xyz, d, w, 0.3, 64)
    b = device_covariogram(ctx, xyz, d, w, 0.3, 64)
    p = rng.permutation(700)
    c = device_covariogram(ctx, xyz[:, p], d[p], w[p], 0.3, 64)
    assert a[0] == 0 and a[1].sum() > 0
    for other in (b, c):
        for x, y in zip(a[1:4], other[1:4]):
            assert x.tobytes() == y.tobytes()


# ---- 4. skipped observations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["d", "w"])
def test_non_finite_observations_take_part_in_nothing(ctx, where):
    m = 300
    rng = np.random.default_rng(4300)
    xyz = cc.cap_points(rng, m, 20.0)
    d, w = rng.normal(size=m), rng.uniform(0.5, 2.0, m)
    if where == "d":
        d[0], d[m // 2], d[m - 1] = np.nan, np.inf, -np.inf
    else:
        w[0] = w[m // 2] = w[m - 1] = np.nan
    got = device_covariogram(ctx, xyz, d, w, 0.3, 64)
    assert got[4] == m - 3
    check_against_numpy(ctx, xyz, d, w, 0.3, 64, got, f"non-finite {where} at 0, {m // 2}, {m - 1}")
    keep = np.ones(m, dtype=bool)
    keep[[0, m // 2, m - 1]] = False                            # ... which is the result on the remaining observations
    rc, rsp, rsc = cc.ref_covariogram(xyz[:, keep], (d * w)[keep], 0.3, 64)
    np.testing.assert_array_equal(got[1], rc)


# ---- 5. contention and degeneracy -----------------------------------------------------------------------------------------------------
def test_one_bin_takes_every_pair(ctx):
    rng = np.random.default_rng(5600)
    xyz = cc.cap_points(rng, 600, 0.01)
    d = rng.normal(size=600)
    got = device_covariogram(ctx, xyz, d, None, 0.3, 1)
    rcount, _, _ = check_against_numpy(ctx, xyz, d, None, 0.3, 1, got, "600 points in a 0.01 deg cap, one bin")
    assert rcount[0] == 600 * 599 // 2


def test_duplicated_points(ctx):
    rng = np.random.default_rng(5300)
    xyz = np.repeat(cc.cap_points(rng, 300, 20.0), 2, axis=1)
    d = rng.normal(size=600)
    got = device_covariogram(ctx, xyz, d, None, 0.3, 64)
    rcount, _, _ = check_against_numpy(ctx, xyz, d, None, 0.3, 64, got, "300 points, each twice")
    assert rcount[0] >= 300


def test_all_zero_innovations(ctx):
    rng = np.random.default_rng(5000)
    xyz = cc.cap_points(rng, 400, 20.0)
    d = np.zeros(400)
    rc, count, sp, sc, used = device_covariogram(ctx, xyz, d, None, 0.3, 64)
    assert rc == 0 and used == 400 and quanta(ctx, d, 400)[0] == 1.0
    assert np.all(sp == 0.0) and not np.signbit(sp).any()
    check_against_numpy(ctx, xyz, d, None, 0.3, 64, (rc, count, sp, sc, used), "u = 0")


# ---- 6. dynamic range ------------------------------------------------------------------------------------------------------------
def test_one_large_innovation(ctx):
    rng = np.random.default_rng(6100)
    xyz = cc.cap_points(rng, 500, 20.0)
    d = rng.normal(size=500)
    d[123] *= 1e6
    got = device_covariogram(ctx, xyz, d, None, 0.3, 64)
    check_against_numpy(ctx, xyz, d, None, 0.3, 64, got, "one innovation 1e6 times the rest")


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins,max_chord", [(0, 0.3), (1025, 0.3), (64, 0.0), (64, -0.3), (64, float("nan")), (64, float("inf"))])
def test_bad_arguments_leave_the_outputs_alone(ctx, nbins, max_chord):
    rng = np.random.default_rng(7)
    xyz = cc.cap_points(rng, 50, 20.0)
    rc, count, sp, sc, used = device_covariogram(ctx, xyz, rng.normal(size=50), None, max_chord, nbins)
    assert rc == EINVAL and used == int(SENTINEL)
    assert np.all(count == int(SENTINEL)) and np.all(sp == SENTINEL) and np.all(sc == SENTINEL)


def test_bad_sizes(ctx):
    rc, count, sp, sc, used = device_covariogram(ctx, None, np.empty(0), None, 0.3, 64, m=0)
    assert rc == 0 and used == 0 and not count.any() and not sp.any() and not sc.any()
    for m in (-1, (1 << 20) + 1):
        rc, count, sp, sc, used = device_covariogram(ctx, np.ones((3, 4)), np.ones(4), None, 0.3, 64, m=m)
        assert rc == EINVAL and np.all(count == int(SENTINEL)) and np.all(sp == SENTINEL)


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
def test_fit_through_the_device_covariogram(ctx):
    """A Gaussian field at L0 = 400 km, 1500 global points: the fit through the device covariogram against the same fit through
    the NumPy covariogram, 1e-6 relative in L and scale (tests/test_covariogram_cpu.py: the rounding bound moves the fit by
    1.7e-8 at most).  How close either comes to 400 km and 0.6 is sampling noise: printed."""
    lat, lon, u, rcount, rsp, rsc = cc.end_to_end_case()
    c = cc.END_TO_END
    cg = dense.innovation_covariogram(lat, lon, u, max_km=c["max_km"], nbins=c["nbins"], ctx=ctx)
    q_prod, q_chord = cc.quanta_ref(np.abs(u).max(), c["m"])
    assert (cg["q_prod"], cg["q_chord"], cg["nobs"]) == (q_prod, q_chord, c["m"]) and cg["var0"] == pytest.approx(float(np.mean(u * u)), rel=1e-14)
    np.testing.assert_array_equal(cg["count"], rcount)
    ref = cc.covariogram_dict(rcount, rsp, rsc, c["max_km"], c["m"], cg["var0"], q_prod, q_chord)
    np.testing.assert_allclose(cg["r_km"], cc.R_EARTH * cg["chord"], rtol=0, atol=0)
    fd, fr = dense.fit_correlation(cg), dense.fit_correlation(ref)
    print(f"device fit L {fd['L_km']:.4f} km scale {fd['scale']:.5f}; NumPy fit L {fr['L_km']:.4f} km scale {fr['scale']:.5f} "
          f"(drawn at 400 km, 0.6); relative difference L {abs(fd['L_km'] / fr['L_km'] - 1):.2e}, scale {abs(fd['scale'] / fr['scale'] - 1):.2e}")
    assert fd["found"] and fr["found"]
    assert abs(fd["L_km"] / fr["L_km"] - 1) <= 1e-6 and abs(fd["scale"] / fr["scale"] - 1) <= 1e-6
    both = dense.fit_correlation(cg, ["gaussian", "gaspari_cohn", "soar"])
    print("models by rms:", {k: round(v["rms"], 5) for k, v in both["all"].items()})


def test_estimate_keeps_the_callers_arrays(ctx):
    c = syn.diag_case(36, 72, 900, 41)
    Y0, So0 = c.Y.copy(), c.So.copy()
    assert np.nanmin(Y0) < 0                                     # (the clamp has something to do)
    f = dense.estimate_corr_length(c.Xa, c.Y, c.Sa, c.So, c.lat, c.lon, scale=0.5, corr=["gaussian", "soar"], nbins=32, ctx=ctx)
    np.testing.assert_array_equal(c.Y, Y0)
    np.testing.assert_array_equal(c.So, So0)
    assert f["covariogram"]["nobs"] == 900 and f["covariogram"]["count"].size == 32 and sorted(f["all"]) == ["gaussian", "soar"]


# ---- 9. the driver -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "tiled"])
def test_driver_auto_is_the_analysis_at_the_fitted_length(ctx, mode, monkeypatch):
    from oisatgmi.driver import oisatgmi
    for v in ("OISAT_OI_MODE", "OISAT_CORRELATION", "OISAT_CORR_LENGTH_KM", "OISAT_UNOBSERVED", "OISAT_OI_ERROR"):
        monkeypatch.delenv(v, raising=False)
    c = syn.diag_case(36, 72, 1200, 77)
    lat, lon = syn.global_grid(36, 72)

    def run(L):
        o = oisatgmi()
        o.ctm_averaged_vcd, o.sat_averaged_vcd = c.Xa.copy(), c.Y.copy()
        o.sat_averaged_error = np.sqrt(c.So)
        o.grid_lat, o.grid_lon = lat, lon
        o.oi_mode, o.corr_length_km = mode, L
        o.oi("OMI", error_ctm=50.0)
        return o

    a = run("auto")
    fit = a.oi_info["corr_fit"]
    print(f"{mode}: fitted {fit}")
    assert "covariogram" not in fit and a.oi_info["corr_length_km"] == (fit["L_km"] if fit["found"] else 300.0)
    b = run(a.oi_info["corr_length_km"])
    assert "corr_fit" not in b.oi_info and b.oi_info["corr_length_km"] == a.oi_info["corr_length_km"]
    for name in ("ctm_averaged_vcd_corrected", "ak_OI", "increment_OI", "error_OI"):
        assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes()
    assert np.isfinite(a.increment_OI).any()
