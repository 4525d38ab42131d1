"""GPU tests of the posterior ensemble: the random-feature sampler and the member spread at the C ABI
against their float64 restatements (tests/ensemble_cases.py), Matheron's rule end to end with the same draws, the ensemble's
variance against the exact ``posterior_error()`` and against ``functional_covariance`` under the two statistical conditions of
tests/mc_error_cases.py, and the driver's setting.  The deterministic tolerances are four times the largest error measured on an
MI355X (recorded beside each and in DESIGN.md section 4.2j); nothing here waits, polls or can hang."""
import numpy as np
import pytest

import ensemble_cases as ec
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

pytestmark = pytest.mark.gpu
EINVAL = -1

EPS32 = 2.0 ** -24                # half an ulp of a float in [1, 2)
SAMPLER_DEFECT = 1e-4             # a sampler error above this, of the unit variance, is a defect whatever the tolerance
# Every deterministic tolerance below is 4 x the largest error measured on an MI355X (DESIGN.md section 4.2j has the figures).
# Sampler, max |out - float64| in units of the field's standard deviation over the four combinations of scale and noise:
# F = 1: 1.662e-7, F = 96: 9.867e-7, F = 257: 1.358e-6 (the expectation was sqrt(2 F) 1e-7 = 2.3e-6 at F = 257).
TOL_SAMPLER = {1: 4 * 1.662e-7, 96: 4 * 9.867e-7, 257: 4 * 1.358e-6}
# Member spread, relative to the largest entry, over the three models, K = 32 / 64 / 96, both layouts, window or not:
# P 9.1e-8 - 4.89e-7 (largest: Gaspari-Cohn), sum2 6.5e-8 - 1.99e-7, sum4 9.2e-8 - 7.04e-7 (largest: SOAR).
TOL_SPREAD_P, TOL_SPREAD_SUM2, TOL_SPREAD_SUM4 = 4 * 4.89e-7, 4 * 1.99e-7, 4 * 7.04e-7
# End to end, |deviation - float64| / max sigma; the restatement solves the float64 S exactly, so this includes the fp32
# factor's own cut: gaussian 2.017e-6, soar 1.943e-6.
TOL_E2E = {"gaussian": 4 * 2.017e-6, "soar": 4 * 1.943e-6}


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


# ---- 1. the sampler at the C ABI ---------------------------------------------------------------------------------------------------
def _sampler_points():
    """300 points: both poles, the date line from both sides, the rest area-uniform."""
    rng = np.random.default_rng(5)
    lat = np.rad2deg(np.arcsin(rng.uniform(-1, 1, 300)))
    lon = rng.uniform(-180, 180, 300)
    lat[:6] = [-90.0, 90.0, 0.0, 0.0, 45.0, -45.0]
    lon[:6] = [0.0, 77.0, 180.0, -180.0, 180.0, -180.0]
    return dense.unit_vectors(lat, lon)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("F", [1, 96, 257])
def test_field_sample_against_float64(ctx, F, with_scale, with_noise):
    """300 points (not a multiple of 256), 3 members, ld = 384, SOAR frequencies at L = 400 km with one of them scaled by 1e3
    (phases of hundreds to thousands of turns: the double range reduction), F across the 128-feature chunks of the LDS staging.
    The tolerance is ``TOL_SAMPLER``'s; independently, an error above 1e-4 of the unit variance is a defect."""
    npts, K, ld = 300, 3, 384
    pxyz = _sampler_points()
    omega, phase, eps = dense.ensemble_draws("soar", 400.0, range(K), F, npts, 9)
    omega[1, F // 2] *= 1e3
    rng = np.random.default_rng(F)
    scale = rng.uniform(0.5, 2.0, npts) if with_scale else None
    nscale = rng.uniform(0.1, 1.0, npts) if with_noise else None
    noise = np.zeros((K, ld), dtype=np.float32)
    noise[:, :npts] = eps
    d_p, d_om, d_ph = ctx.upload(pxyz), ctx.upload(np.ascontiguousarray(omega.transpose(0, 2, 1))), ctx.upload(phase)
    d_sc = ctx.upload(scale) if with_scale else None
    d_no, d_ns = (ctx.upload(noise), ctx.upload(nscale)) if with_noise else (None, None)
    out = ctx.alloc(K * ld * 4)
    ctx.check(ctx.lib.oisat_memset(ctx.h, out.ptr, 0x55, K * ld * 4))
    ctx.check(ctx.lib.oisat_field_sample(ctx.h, d_p.ptr, npts, d_sc.ptr if d_sc else None, d_om.ptr, d_ph.ptr, F, K,
                                         d_no.ptr if d_no else None, d_ns.ptr if d_ns else None, out.ptr, ld))
    got = ctx.download(out.ptr, (K, ld), np.float32)
    assert np.array_equal(got[:, npts:].view(np.uint32), np.zeros((K, ld - npts), dtype=np.uint32))        # exact +0
    want = ec.field_sample64(pxyz, scale, omega, phase, noise[:, :npts].astype(np.float64) if with_noise else None, nscale)
    assert np.abs(omega[1, F // 2] @ pxyz).max() > 300.0                                                # the reduction is exercised
    unit = 2.0 if with_scale else 1.0
    err, tol = np.abs(got[:, :npts] - want).max() / unit, TOL_SAMPLER[F]
    print(f"field_sample F = {F}, scale {with_scale}, noise {with_noise}: max error {err:.3e} of the unit standard deviation "
          f"(tolerance {tol:.1e}, defect bar {SAMPLER_DEFECT:.0e})")
    assert err <= SAMPLER_DEFECT and err <= tol
    assert np.abs(want).max() > 0.5


# ---- 2. the member spread at the C ABI -------------------------------------------------------------------------------------------
_spread_cache = {}


def _spread_setup(ctx, corr):
    """20 x 45 cells (a multiple of neither 8 nor 32), 300 observations, L = 300 km; 96 random vectors at the observations and 96
    random rows on the grid; the float64 G = B H^T is computed once per model and shared."""
    if corr not in _spread_cache:
        p = syn.point_obs_case(20, 45, 300, 78)
        plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=300, dtype=np.float32, ctx=ctx)
        plan.load_background(p.Xa, p.Sa)
        plan.load_obs(p.obs_lat, p.obs_lon, dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon), p.obs_y, p.obs_var)
        sysm = ec.System(p, 300.0, corr, ctx.lib)
        rng = np.random.default_rng(12)
        U = np.zeros((96, plan.mp), dtype=np.float32)
        U[:, :plan.m] = rng.standard_normal((96, plan.m))
        P0 = (rng.standard_normal((96, plan.n)) * sysm.gsig[None, :]).astype(np.float32)
        _spread_cache[corr] = (plan, sysm, ctx.upload(U), U, P0, ctx.alloc(96 * plan.n * 4), ctx.alloc(2 * plan.n * 8))
    return _spread_cache[corr]


@pytest.mark.parametrize("K", [32, 64, 96])
@pytest.mark.parametrize("corr", list(ec.KINDS))
def test_member_spread_against_float64(ctx, corr, K):
    """Both cell layouts (nx > 0: patches; nx = 0: runs of 256), with and without the latitude window, accumulate 0 then 1; K = 64
    takes the groups of 64, K = 32 and 96 those of 32.  P and both sums against the float64 restatement, relative to the largest
    entry (``TOL_SPREAD_*``); 48 members: ``OISAT_EINVAL``."""
    plan, sysm, dU, U, P0, dP, dS = _spread_setup(ctx, corr)
    n, m, mp, lib = plan.n, plan.m, plan.mp, ctx.lib
    wantP, want2, want4 = ec.spread64(sysm.G, U[:K, :m], P0[:K])
    ctx.check(lib.oisat_set_correlation(ctx.h, ec.KINDS[corr]))
    for grid in (True, False):
        for windowed in (True, False):
            ny, nx = (plan._ny, plan._nx) if grid else (n, 0)
            res = []
            for acc in (0, 1):
                ctx.upload_into(dP.ptr, P0[:K])
                if acc == 0:
                    ctx.check(lib.oisat_memset(ctx.h, dS.ptr, 0x7f, 2 * n * 8))      # (accumulate = 0 overwrites whatever is there)
                ctx.check(lib.oisat_member_spread(ctx.h, plan.gxyz.ptr, plan.gsig.ptr, ny, nx, plan.oxyz.ptr, plan.osig.ptr, dU.ptr, K, mp, m,
                                                  sysm.g, plan.glat.ptr if windowed else None, plan.olat.ptr if windowed else None, dP.ptr, n,
                                                  acc, dS.at(0), dS.at(n * 8)))
                res.append((ctx.download(dP.ptr, (K, n), np.float32), ctx.download(dS.ptr, (2, n), np.float64)))
            (gotP, s), (gotP1, s1) = res
            eP = np.abs(gotP - wantP).max() / np.abs(wantP).max()
            e2, e4 = np.abs(s[0] - want2).max() / want2.max(), np.abs(s[1] - want4).max() / want4.max()
            print(f"member_spread {corr}, K = {K}, {'grid' if grid else 'runs'}, {'windowed' if windowed else 'every pair'}: P error {eP:.2e} "
                  f"(tolerance {TOL_SPREAD_P:.1e}), sum2 {e2:.2e}, sum4 {e4:.2e} (tolerances {TOL_SPREAD_SUM2:.1e}, {TOL_SPREAD_SUM4:.1e}) of the largest entry")
            assert eP <= TOL_SPREAD_P and e2 <= TOL_SPREAD_SUM2 and e4 <= TOL_SPREAD_SUM4
            # the sums are those of the stored floats, in double; accumulate = 1 adds the same numbers to them
            g64 = gotP.astype(np.float64) ** 2
            np.testing.assert_allclose(s[0], g64.sum(axis=0), rtol=1e-13)
            np.testing.assert_allclose(s[1], (g64 * g64).sum(axis=0), rtol=1e-13)
            assert np.array_equal(gotP1, gotP) and np.array_equal(s1, s + s)
    ctx.upload_into(dP.ptr, P0[:K])
    rc = lib.oisat_member_spread(ctx.h, plan.gxyz.ptr, plan.gsig.ptr, plan._ny, plan._nx, plan.oxyz.ptr, plan.osig.ptr, dU.ptr, 48, mp, m,
                                 sysm.g, None, None, dP.ptr, n, 0, dS.at(0), dS.at(n * 8))
    assert rc == EINVAL
    assert np.array_equal(ctx.download(dP.ptr, (K, n), np.float32), P0[:K])             # nothing was launched


# ---- 3. end to end, deterministic ------------------------------------------------------------------------------------------------------
E2E_L = {"gaussian": 300.0, "soar": 150.0}        # lengths at which the factor's envelope of the 400 observations is not dense


@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_members_equal_the_float64_rule_with_the_same_draws(ctx, corr):
    """24 x 48 cells, 400 scattered observations (mp = 512: four block rows, an envelope that is not dense), K = 160: one full and
    one padded panel.  The restatement solves the float64 S exactly, so the difference includes the fp32 factor's own cut
    (``TOL_E2E``).  One cell has sigma = 0: its deviations are 0."""
    K, F, seed, L = 160, 64, 77, E2E_L[corr]
    p = syn.point_obs_case(24, 48, 400, 41)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    Sa = np.array(p.Sa, dtype=np.float64)
    dead = int(np.setdiff1d(np.arange(Sa.size), cell)[100])                       # an unobserved cell without background error
    Sa.flat[dead] = 0.0
    p.Sa = Sa
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=400, dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, p.obs_y, p.obs_var)
    plan.run(L, check_pd=True, corr=corr)
    plan.check()
    assert plan.mp == 512 and (plan._env_host[:4] > 0).any(), plan._env_host
    ens = plan.posterior_ensemble(nmember=K, nfeature=F, seed=seed)
    dev = ens["deviations"]
    assert dev.shape == (K, 24, 48) and dev.dtype == np.float32 and ens["err"].shape == (24, 48) and ens["err"].dtype == np.float32
    assert (ens["nmember"], ens["nfeature"], ens["seed"]) == (K, F, seed) and ens["err_se"].shape == (24, 48)
    sysm = ec.System(p, L, corr, ctx.lib)
    want = sysm.deviations(range(K), F, seed).reshape(K, 24, 48)
    e = np.abs(dev - want).max() / sysm.gsig.max()
    print(f"{corr}: max |deviation - float64| = {e:.3e} of the largest sigma (tolerance {TOL_E2E[corr]:.1e}); "
          f"full panel {np.abs(dev[:128] - want[:128]).max() / sysm.gsig.max():.3e}, padded panel {np.abs(dev[128:] - want[128:]).max() / sysm.gsig.max():.3e}")
    assert e <= TOL_E2E[corr]
    assert not dev.reshape(K, -1)[:, dead].any() and ens["err"].flat[dead] == 0 and ens["err_se"].flat[dead] == 0
    # err is the root of the members' mean square, err_se from their fourth moments
    A, A_var = ec.mean_var((dev.astype(np.float64) ** 2).sum(axis=0), (dev.astype(np.float64) ** 4).sum(axis=0), K)
    np.testing.assert_allclose(ens["err"], np.sqrt(A), rtol=1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(ens["err_se"], np.where(A > 0, np.sqrt(A_var) / (2 * np.sqrt(A)), 0.0), rtol=1e-10)
    # same seed, same bits; member k is member k whatever the ensemble's size; keep=False returns the same errors
    again = plan.posterior_ensemble(nmember=K, nfeature=F, seed=seed, keep=False)
    assert again["deviations"] is None and np.array_equal(again["err"], ens["err"]) and np.array_equal(again["err_se"], ens["err_se"])
    small = plan.posterior_ensemble(nmember=32, nfeature=F, seed=seed)
    assert np.array_equal(small["deviations"], dev[:32])
    other = plan.posterior_ensemble(nmember=32, nfeature=F, seed=seed + 1)
    assert not np.array_equal(other["deviations"], dev[:32])
    # the error scales are honoured: the ensemble of the scaled system
    plan.set_error_scales(2.0, 0.5)
    plan.run(L, check_pd=True, corr=corr)
    scaled = plan.posterior_ensemble(nmember=32, nfeature=F, seed=seed)["deviations"]
    want_s = ec.System(p, L, corr, ctx.lib, scale_b=2.0, scale_o=0.5).deviations(range(32), F, seed).reshape(32, 24, 48)
    es = np.abs(scaled - want_s).max() / (np.sqrt(2.0) * sysm.gsig.max())
    print(f"{corr}, error scales (2, 0.5): max |deviation - float64| = {es:.3e} of the largest sigma (tolerance {TOL_E2E[corr]:.1e})")
    assert es <= TOL_E2E[corr]


def test_posterior_ensemble_wants_a_run_first(ctx):
    p = syn.point_obs_case(12, 24, 50, 2)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=50, dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    with pytest.raises(ValueError, match="must follow run"):
        plan.posterior_ensemble()


# ---- 4. and 5. statistical: against the exact error and against the regional means --------------------------------------------------
_stat_cache = {}


def _stat(ctx, corr):
    if corr not in _stat_cache:
        p = ec.stat_case()
        plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=150, dtype=np.float32, ctx=ctx, diag_chunk_rows=4096)
        plan.load_background(p.Xa, p.Sa)
        plan.load_obs(p.obs_lat, p.obs_lon, dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon), p.obs_y, p.obs_var)
        plan.run(ec.STAT_L, check_pd=True, corr=corr)
        _stat_cache[corr] = (p, plan, plan.posterior_ensemble(nmember=ec.STAT_K, nfeature=ec.STAT_F, seed=ec.SEED))
        _stat_cache[corr][1].check()
    return _stat_cache[corr]


@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_ensemble_variance_meets_the_exact_posterior_error(ctx, corr):
    """16 x 32 cells, 150 observations, L = 1000 km, K = 1024, F = 256: err^2 against ``posterior_error()``^2 under conditions (a)
    and (b) of tests/mc_error_cases.py, at most 2 % of the cells beyond 3 se (tests/test_ensemble_cpu.py shows that the float64
    restatement with this seed meets the same).  Floors: the exact error is a float32 (2^-23 of sig^2 in its square) and both
    sides come from fp32 triangular solves with the same factor (2^-16 of the reduction sig^2 - A)."""
    p, plan, ens = _stat(ctx, corr)
    K = ec.STAT_K
    plan.run(ec.STAT_L, check_pd=True, corr=corr)                      # (the handle knows one factor: other tests factor in between)
    A_exact = plan.posterior_error().astype(np.float64) ** 2
    sig2 = np.asarray(p.Sa, dtype=np.float64)
    A = ens["err"].astype(np.float64) ** 2
    se = 2.0 * ens["err"] * ens["err_se"]
    ec.check_conditions(A, se, A_exact, K, 2.0 ** -23 * sig2 + 2.0 ** -16 * (sig2 - A_exact), f"A (cells), {corr}")
    share = ec.beyond_three(A, se, A_exact)
    print(f"{corr}: {100 * share:.2f} % of the cells beyond 3 se (bound 2 %); median err_se / err = {np.median(ens['err_se'] / ens['err']):.4f}")
    assert share <= 0.02


@pytest.mark.parametrize("corr", ["gaussian", "soar"])
def test_regional_means_of_the_members_meet_the_exact_functional_covariance(ctx, corr):
    """Two independent paths: the sample variance of W . delta_k over the members of the case above, with the standard error from
    its fourth moments, against the diagonal of ``functional_covariance(W)["posterior"]`` for three regions."""
    p, plan, ens = _stat(ctx, corr)
    K = ec.STAT_K
    W = dense.region_weights(ec.stat_regions(), p.lat)[1]
    plan.run(ec.STAT_L, check_pd=True, corr=corr)
    exact = np.diag(plan.functional_covariance(W)["posterior"])
    f = ens["deviations"].reshape(K, -1).astype(np.float64) @ W.reshape(3, -1).T
    v, vv = ec.mean_var((f ** 2).sum(axis=0), (f ** 4).sum(axis=0), K)
    ec.check_conditions(v, np.sqrt(vv), exact, K, 2.0 ** -16 * np.diag(plan.functional_prior(W)), f"regional means, {corr}")


# ---- 6. OI_dense and the driver -----------------------------------------------------------------------------------------------------
def test_oi_dense_carries_the_ensemble_and_prior_draws_without_observations(ctx):
    c = syn.diag_case(24, 48, 300, 23)
    Xa = c.Xa.copy()
    unobs = np.flatnonzero(~np.isfinite(c.Y.ravel()))[:5]
    Xa.flat[unobs] = np.nan                                             # (unobserved cells: the system stays the same)
    xb0, inc0, info0 = dense.OI_dense(Xa.copy(), c.Y.copy(), c.Sa, c.So, c.lat, c.lon, 300.0)
    xb, inc, info = dense.OI_dense(Xa.copy(), c.Y.copy(), c.Sa, c.So, c.lat, c.lon, 300.0, ensemble=32, ensemble_features=64, seed=4)
    assert np.array_equal(xb0, xb, equal_nan=True) and np.array_equal(inc0, inc) and "ensemble" not in info0
    ens = info["ensemble"]
    assert ens["deviations"].shape == (32, 24, 48) and (ens["nmember"], ens["nfeature"], ens["seed"]) == (32, 64, 4)
    bad = ~np.isfinite(Xa)
    assert np.isnan(ens["deviations"][:, bad]).all() and np.isfinite(ens["deviations"][:, ~bad]).all()
    assert (ens["err"][~bad] > 0).all() and (ens["err"][~bad] < 3 * np.sqrt(c.Sa[~bad])).all()
    # scattered observations and superobservations: the ensemble of whatever system the plan solved
    p = syn.point_obs_case(24, 48, 300, 8)
    obs = dict(lat=p.obs_lat, lon=p.obs_lon, y=p.obs_y, var=p.obs_var)
    for kw in (dict(), dict(superob=4.0), dict(fit_scale="background")):
        e = dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, 600.0, obs=obs, ensemble=32, ensemble_features=32, corr="soar", **kw)[2]["ensemble"]
        assert e["deviations"].shape == (32, 24, 48) and np.isfinite(e["deviations"]).all() and (e["err"] > 0).all(), kw
    # no observation at all: prior draws, err = sqrt(scale Sa)
    Y = np.full(Xa.shape, np.nan)
    pr = dense.OI_dense(Xa.copy(), Y, c.Sa, Y.copy(), c.lat, c.lon, 300.0, scale=2.0, ensemble=64, ensemble_features=64, seed=4)[2]["ensemble"]
    sig = np.sqrt(2.0 * c.Sa)
    np.testing.assert_allclose(pr["err"], sig, rtol=1e-6)
    want = ec.field_sample64(dense.unit_vectors(c.lat, c.lon), sig.ravel(), *dense.ensemble_draws("gaussian", 300.0, range(64), 64, 0, 4)[:2])
    got = pr["deviations"].reshape(64, -1)
    assert np.isnan(got[:, bad.ravel()]).all()
    assert np.abs(got - want)[:, ~bad.ravel()].max() <= (TOL_SAMPLER[96] + 4 * EPS32) * sig.max()      # (F = 64: the bar of F = 96, and one float rounding of a value up to 4 sigma)
    assert pr["err_se"].shape == (24, 48) and (pr["err_se"][~bad] > 0).all() and (pr["err_se"][~bad] < 0.5 * sig[~bad]).all()


def test_the_driver_fills_the_ensemble_in_dense_mode_and_refuses_tiled(ctx, monkeypatch):
    c = syn.diag_case(24, 48, 500, 21)
    Xa = c.Xa.copy()
    Xa.flat[np.flatnonzero(~np.isfinite(c.Y.ravel()))[:4]] = np.nan
    for var in ("OISAT_OI_QC", "OISAT_CORR_LENGTH_KM", "OISAT_CORRELATION", "OISAT_UNOBSERVED", "OISAT_OI_SUPEROB", "OISAT_OI_REGIONS",
                "OISAT_OI_ERROR", "OISAT_OI_SCALE", "OISAT_OI_ENSEMBLE"):
        monkeypatch.delenv(var, raising=False)

    def drive(mode="dense"):
        o = oisatgmi()
        o.ctm_averaged_vcd, o.sat_averaged_vcd, o.sat_averaged_error = Xa.copy(), c.Y.copy(), c.sat_err.copy()
        o.grid_lat, o.grid_lon, o.oi_mode, o.oi_reg_index = c.lat, c.lon, mode, 40
        o.oi("OMI")
        return o

    a = drive()
    monkeypatch.setenv("OISAT_OI_ENSEMBLE", "32")
    b = drive()
    assert "ensemble" not in a.oi_info
    ens = b.oi_info["ensemble"]
    assert ens["deviations"].shape == (32, 24, 48) and ens["err"].shape == (24, 48) and ens["err_se"].shape == (24, 48)
    assert (ens["nmember"], ens["nfeature"]) == (32, 256)
    assert np.array_equal(np.isnan(ens["deviations"][0]), ~np.isfinite(Xa)) and np.isnan(ens["deviations"][:, ~np.isfinite(Xa)]).all()
    for fa, fb in ((a.error_OI, b.error_OI), (a.ak_OI, b.ak_OI), (a.ctm_averaged_vcd_corrected, b.ctm_averaged_vcd_corrected)):
        assert fa.tobytes() == fb.tobytes()                           # the analysis and its exact error are untouched, to the bit
    monkeypatch.setenv("OISAT_OI_ENSEMBLE", "64:32")
    assert drive().oi_info["ensemble"]["deviations"].shape == (64, 24, 48)
    with pytest.raises(ValueError, match="belongs to the dense mode"):
        drive("tiled")
