"""Superobservations through ``dense.OI_dense`` and ``oisatgmi.oi()``: the analysis of the merged system against float64 host
solves of the RESTATED superobservations (tests/superob_cases.py), at the tolerances of the dense-versus-host tests
(tests/test_gpu_soar.py: z 2e-5, fields 1e-5 of the largest background value)."""
import functools

import numpy as np
import pytest

import superob_cases as sc
from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def library_corr(name, L_km):
    """C(chord^2) in float64 by the library's host-only function."""
    lib, g = _hip.load_library(), sc.decay(L_km)

    def corr(d2):
        d2 = np.ascontiguousarray(d2, dtype=np.float64)
        out = np.empty_like(d2)
        assert lib.oisat_corr_eval(KINDS[name], g, d2.ctypes.data, d2.size, out.ctypes.data) == 0
        return out
    return corr


# ---- 1. one member per box: superobbing changes nothing --------------------------------------------------------------------------
def test_one_member_per_box_is_the_plain_analysis(ctx):
    """400 points on a 10 degree cap, 0.9 degrees apart with a jitter of 0.2: no two share a 0.25 degree box (asserted on the
    restatement).  Each analysis is within REFINE_TOL |d| of the exact fields (include/oisat.h, oisat_gain_solve), so the two
    are within twice that of each other; the merge itself moves d, sigma_b and the position by rounding errors only.
    Measured on the MI355X: increments and analyses differ by 1.7e-11 at most (the bound is 3.4e-5), z by 7.9e-13 relative."""
    rng = np.random.default_rng(9)
    p = syn.point_obs_case(72, 144, 400, 11)
    la, lo = np.meshgrid(31.0 + 0.9 * np.arange(20), 5.0 + 0.9 * np.arange(20), indexing="ij")
    olat, olon = la.ravel() + rng.uniform(-0.2, 0.2, 400), lo.ravel() + rng.uniform(-0.2, 0.2, 400)
    cell = dense.regular_grid_cell(p.lat, p.lon, olat, olon)
    var = rng.uniform(0.05, 0.3, 400) ** 2
    y = p.Xa.ravel()[cell] * (1.0 + 0.2 * rng.normal(size=400)) + np.sqrt(var) * rng.normal(size=400)
    y = np.where(y < 0, 0.0, y)
    d = y - p.Xa.ravel()[cell]
    sig = np.sqrt(p.Sa.ravel()[cell])
    ref = sc.ref_superob(olat, olon, sc.unit_vectors(olat, olon), d, sig, var, 0.25)
    assert ref["nused"] == 400 and ref["count"].max() <= 1 and ref["ids"].size == 400
    obs = dict(lat=olat, lon=olon, y=y, var=var)
    xb0, inc0, info0 = dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, 600.0, obs=obs)
    xb1, inc1, info1 = dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, 600.0, obs=obs, superob=0.25)
    assert info1["superob"]["nobs"] == 400 and info1["superob"]["nobs_raw"] == 400 and (info1["superob"]["count"] == 1).all()
    assert "superob" not in info0
    bound = 2.0 * dense.REFINE_TOL * np.linalg.norm(d)
    e_inc, e_xb = np.abs(inc1 - inc0).max(), np.abs(xb1 - xb0).max()
    zs = info1["z"][info1["superob"]["index"]]                  # per superobservation -> per observation
    e_z = np.abs(zs - info0["z"]).max() / np.abs(info0["z"]).max()
    print(f"one member per box: increments differ by {e_inc:.3e}, analyses by {e_xb:.3e} (bound {bound:.3e}), z by {e_z:.3e} relative")
    assert e_inc <= bound and e_xb <= bound


# ---- 2. real merging against a float64 solve of the restated superobservations -----------------------------------------------
@functools.lru_cache(maxsize=None)
def patch_fields():
    """The 48 x 48 patch as ``OI_dense`` wants it: a background of 5 (exact in float32) under the recipe's zero-mean truth, so
    that no observation is clamped at 0."""
    p = sc.patch_case(300.0)
    Xa = np.full(p["lat2"].shape, 5.0)
    Sa = np.full(p["lat2"].shape, sc.PATCH["sigma_b"] ** 2)
    Y, So = np.full(Xa.size, np.nan), np.full(Xa.size, np.nan)
    Y[p["cell"]] = 5.0 + p["d"]
    So[p["cell"]] = p["var"]
    assert np.nanmin(Y) > 0
    d = Y[p["cell"]] - 5.0
    ref = sc.ref_superob(p["obs_lat"], p["obs_lon"], sc.unit_vectors(p["obs_lat"], p["obs_lon"]), d, p["sig"], p["var"], 1.0)
    return p, Xa, Y.reshape(Xa.shape), Sa, So.reshape(Xa.shape), ref


@pytest.mark.parametrize("rho", [0.0, 0.3])
@pytest.mark.parametrize("corr", ["gaussian", "gaspari_cohn", "soar"])
def test_merged_analysis_against_float64_host_solve(ctx, corr, rho):
    p, Xa, Y, Sa, So, ref = patch_fields()
    assert ref["ids"].size < ref["nused"] / 10 and ref["count"].max() >= 12      # real merging: 1 degree boxes of 0.25 degree cells
    s = sc.merge(ref, rho)
    gsig = np.full(Xa.size, sc.PATCH["sigma_b"])
    z_ref, inc_ref, _ = sc.analysis(library_corr(corr, 300.0), p["gxyz"], gsig, sc.unit_vectors(s["lat"], s["lon"]), s["sigma_b"],
                                    s["var"], s["d"])
    xb, inc, info = dense.OI_dense(Xa, Y.copy(), Sa, So, p["lat2"], p["lon2"], 300.0, corr=corr, superob=1.0, superob_rho=rho)
    so = info["superob"]
    assert so["nobs"] == ref["ids"].size and so["nobs_raw"] == ref["nused"] == info["nobs"] and so["rho"] == rho
    np.testing.assert_array_equal(so["count"], ref["count"])
    np.testing.assert_array_equal(info["cells"], p["cell"])
    np.testing.assert_array_equal(so["index"], ref["slot"])
    assert so["spread"].tobytes() == s["spread"].tobytes()
    scale = np.abs(Xa).max()
    ez = np.abs(info["z"] - z_ref).max() / np.abs(z_ref).max()
    ei = np.abs(inc.ravel().astype(np.float64) - inc_ref).max() / scale
    ex = np.abs(xb.ravel().astype(np.float64) - (Xa.ravel() + inc_ref)).max() / scale      # (OI_dense's first field is the analysis)
    print(f"{corr} rho {rho}: {so['nobs_raw']} -> {so['nobs']} observations; residuals {info['residuals']}, z {ez:.3e}, inc {ei:.3e}, "
          f"xa {ex:.3e} against the host solve")
    assert info["residuals"][-1] <= dense.REFINE_TOL
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5


# ---- 3. error and averaging kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_error", [True, "mc"])
def test_error_and_averaging_kernel_with_superobservations(ctx, want_error):
    p, Xa, Y, Sa, So, ref = patch_fields()
    xb, inc, info = dense.OI_dense(Xa, Y.copy(), Sa, So, p["lat2"], p["lon2"], 300.0, superob=1.0, want_error=want_error, nprobe=256)
    ns = ref["ids"].size
    assert info["ak_obs"].shape == (ns,) and info["z"].shape == (ns,)
    assert info["ak"].shape == Xa.shape and info["err"].shape == Xa.shape
    if want_error == "mc":
        assert info["ak_obs_se"].shape == (ns,) and info["err_se"].shape == Xa.shape and info["error_method"] == "mc"
    ak = info["ak"].ravel()
    observed = np.zeros(Xa.size, dtype=bool)
    observed[p["cell"]] = True
    assert np.isfinite(ak[observed]).all() and np.isnan(ak[~observed]).all()     # every observed cell has a value
    total, dfs = np.nansum(ak), info["ak_obs"].sum()
    print(f"want_error={want_error!r}: nansum(ak) {total!r}, sum(ak_obs) {dfs!r}")
    assert abs(total - dfs) <= 1e-12 * abs(dfs)                                  # the share rule: w_a / W_s sums to 1 per box
    # ... and the shares are the weights
    w = 1.0 / p["var"]
    np.testing.assert_allclose(ak[p["cell"]], info["ak_obs"][ref["slot"]] * w / ref["sums"][0][ref["slot"]], rtol=1e-13)
    sig_b = np.sqrt(Sa)
    err = np.asarray(info["err"], dtype=np.float64)
    assert (err >= 0).all() and (err <= sig_b).all()
    assert err[observed.reshape(Xa.shape)].mean() < 0.8 * sig_b.mean()           # (the observations do constrain the patch)


# ---- 4. through oisatgmi.oi() -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def month_case():
    """A fully observed 72 x 144 month: 10 368 observations."""
    rng = np.random.default_rng(2027)
    lat, lon = syn.global_grid(72, 144)
    xa = syn.background_field(rng, lat, lon)
    err = rng.uniform(0.05, 0.3, xa.shape) * xa
    y = np.maximum(xa * (1.0 + 0.3 * syn._smooth_unit_field(rng, lat, lon)) + err * rng.normal(size=xa.shape), 0.0)
    return lat, lon, xa, y, err


def run_oi(monkeypatch, setting, error="1"):
    from oisatgmi.driver import oisatgmi
    lat, lon, xa, y, err = month_case()
    for var in ("OISAT_OI_QC", "OISAT_CORR_LENGTH_KM", "OISAT_CORRELATION", "OISAT_UNOBSERVED", "OISAT_OI_SUPEROB"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OISAT_OI_MODE", "dense")
    monkeypatch.setenv("OISAT_OI_ERROR", error)
    if setting is not None:
        monkeypatch.setenv("OISAT_OI_SUPEROB", setting)
    o = oisatgmi()
    o.ctm_averaged_vcd, o.sat_averaged_vcd, o.sat_averaged_error = xa.copy(), y.copy(), err.copy()
    o.grid_lat, o.grid_lon = lat, lon
    o.oi("TROPOMI")
    return o


def test_through_the_driver(ctx, monkeypatch, capsys):
    lat, lon, xa, y, err = month_case()
    assert np.isfinite(y).all() and y.size == 10368
    o = run_oi(monkeypatch, "5")
    out = capsys.readouterr().out
    assert "wider than half the correlation length" in out                       # 5 degrees = 556 km against L = 300 km
    for a in (o.ctm_averaged_vcd_corrected, o.ak_OI, o.increment_OI, o.error_OI):
        assert a.shape == xa.shape and np.isfinite(a).all()
    so = o.oi_info["superob"]
    d = y - xa
    sig = np.sqrt(o.oi_info["scale"] * (0.5 * xa) ** 2)
    ref = sc.ref_superob(lat.ravel(), lon.ravel(), sc.unit_vectors(lat.ravel(), lon.ravel()), d.ravel(), sig.ravel(), (err ** 2).ravel(), 5.0)
    assert so["box_deg"] == 5.0 and so["rho"] == 0.0 and so["nobs_raw"] == 10368 == o.oi_info["nobs"]
    assert so["nobs"] == ref["ids"].size == so["count"].size == so["spread"].size and int(so["count"].sum()) == so["nobs_raw"]
    np.testing.assert_array_equal(so["count"], ref["count"])
    assert so["index"].shape == (10368,) and so["index"].min() == 0 and so["index"].max() == so["nobs"] - 1
    assert (o.error_OI <= np.sqrt(o.oi_info["scale"]) * 0.5 * xa * (1 + 1e-6)).all()


def test_off_unset_and_a_roomy_auto_are_the_same_bits(ctx, monkeypatch):
    """(The posterior error is switched off for these three full-size analyses: it does not depend on the setting and costs more
    than the analyses themselves.)"""
    runs = [run_oi(monkeypatch, s, error="0") for s in (None, "off", "auto:20000")]
    for o in runs:
        assert "superob" not in o.oi_info
    for o in runs[1:]:
        for name in ("ctm_averaged_vcd_corrected", "increment_OI", "ak_OI", "error_OI"):
            assert getattr(o, name).tobytes() == getattr(runs[0], name).tobytes(), name
    assert np.isfinite(runs[0].increment_OI).all()


def test_auto_picks_the_first_ladder_box_that_fits(ctx, monkeypatch):
    lat, lon, xa, y, err = month_case()
    counts = {}
    used = np.ones(lat.size, dtype=bool)
    for box in dense.SUPEROB_LADDER:
        counts[box] = int(np.unique(sc.box_of(lat.ravel(), lon.ravel(), used, box)).size)
    want = next(b for b in dense.SUPEROB_LADDER if counts[b] <= 3000)
    assert want > dense.SUPEROB_LADDER[0] and counts[dense.SUPEROB_LADDER[0]] > 3000
    o = run_oi(monkeypatch, "auto:3000", error="0")
    so = o.oi_info["superob"]
    print(f"auto:3000 on 10 368 observations: ladder counts {counts}, picked {so['box_deg']}")
    assert so["box_deg"] == want and so["nobs"] == counts[want] <= 3000 and so["nobs_raw"] == 10368
    assert np.isfinite(o.increment_OI).all() and np.isfinite(o.ctm_averaged_vcd_corrected).all()
    with pytest.raises(ValueError, match="no box of the ladder"):
        run_oi(monkeypatch, "auto:100", error="0")
