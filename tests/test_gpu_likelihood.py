"""The innovations' likelihood and the maximum-likelihood error scales on the device.

``oisat_factor_logdet`` alone at the C ABI against 2 sum log of the float64 copy of the DOWNLOADED factor (so the factorization's
own error is out of the picture); ``DenseAnalysis.log_likelihood`` against slogdet and a solve of the float64 S;
``fit_error_scales`` against ``profile_search`` driven by the float64 objective (tests/likelihood_cases.py); then ``OI_dense`` and
the driver.  Every system is one of tests/readers_cases.py (m <= 700) or a 36 x 72 grid.

Measured on an MI355X: in the docstrings below."""
import ctypes as C
import math

import numpy as np
import pytest

import likelihood_cases as lc
import readers_cases as rc
from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
NB = rc.NB
EINVAL = -1
POISON = 0x55
F32_POISON = np.frombuffer(bytes([POISON] * 4), dtype=np.float32)[0]
F64_POISON = np.frombuffer(bytes([POISON] * 8), dtype=np.float64)[0]
LOGDET_BAR = 0.05              # the consumer's requirement: Delta J = 1 is one standard error of the estimate; a twentieth of it


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


# ---- 5. the reader alone ------------------------------------------------------------------------------------------------------------
class Factor:
    """A case factored at the C ABI into a poisoned buffer of mp rows of ld = mp + W floats: "potrf" = oisat_cov_build +
    oisat_potrf, "env" = oisat_cov_build_env + oisat_potrf_env inside the case's 2^-52 envelope."""

    def __init__(self, ctx, name, how="potrf", W=0):
        c = self.c = rc.case(name)
        self.ctx, self.ld = ctx, c.mp + W
        lib = ctx.lib
        oxyz, osig, ovar = ctx.upload(c.oxyz), ctx.upload(c.osig), ctx.upload(c.ovar)
        self.S = ctx.alloc(c.mp * self.ld * 4)
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
        ctx.check(lib.oisat_memset(ctx.h, self.S.ptr, POISON, c.mp * self.ld * 4))
        info = C.c_int(-1)
        if how == "potrf":
            ctx.check(lib.oisat_cov_build(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, c.m, c.g, self.S.ptr, self.ld))
            ctx.check(lib.oisat_potrf(ctx.h, self.S.ptr, c.m, self.ld, C.byref(info)))
        else:
            env = rc.envelope(c)
            first, env_dev = env[:c.nb].copy(), ctx.upload(env)
            ctx.check(lib.oisat_cov_build_env(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, c.m, c.g, self.S.ptr, self.ld, env_dev.ptr))
            ctx.check(lib.oisat_potrf_env(ctx.h, self.S.ptr, c.m, self.ld, first.ctypes.data, env_dev.ptr, C.byref(info)))
        assert info.value == 0
        self.full = ctx.download(self.S.ptr, (c.mp, self.ld), np.float32)
        assert (self.full[:, c.mp:].view(np.uint32) == F32_POISON.view(np.uint32)).all(), "the gutter [mp, ld) was written"
        self.diag = self.full[np.arange(c.m), np.arange(c.m)].astype(np.float64)

    def poke(self, a, value):
        """L[a][a] = value on the device."""
        self.ctx.upload_into(self.S.at((a * self.ld + a) * 4), np.array([value], dtype=np.float32))

    def logdet(self, m=None, ld=None):
        """oisat_factor_logdet into the first two of four poisoned doubles; the other two must stay as they are."""
        ctx = self.ctx
        out = ctx.alloc(32)
        ctx.check(ctx.lib.oisat_memset(ctx.h, out.ptr, POISON, 32))
        ctx.check(ctx.lib.oisat_factor_logdet(ctx.h, self.S.ptr, self.c.m if m is None else m, self.ld if ld is None else ld, out.ptr))
        got = ctx.download(out.ptr, (4,), np.float64)
        assert (got[2:].view(np.uint64) == F64_POISON.view(np.uint64)).all(), "out[2:] was written"
        return got[:2].copy()


@pytest.mark.parametrize("name,how", [("A", "potrf"), ("B", "potrf"), ("C", "potrf"), ("B", "env")])
def test_factor_logdet_against_the_downloaded_factor(ctx, name, how):
    """Measured on an MI355X: see DESIGN.md section 4.2i (the error stays below one unit of the bar's 2 + ceil(log2 m))."""
    f = Factor(ctx, name, how)
    c = f.c
    terms = [2.0 * math.log(v) for v in f.diag]
    ref = math.fsum(terms)
    bar = (2 + math.ceil(math.log2(c.m))) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
    got = f.logdet()
    print(f"case {name} ({how}): logdet {got[0]:.12g}, |error| {abs(got[0] - ref):.3g}, bar {bar:.3g}; smallest pivot {got[1]:.6g}")
    assert abs(got[0] - ref) <= bar
    assert got[1] == f.diag.min()
    assert bits(f.logdet()) == bits(got)                           # same inputs, same bits
    # a wide leading dimension with a poisoned gutter: the same bits
    wide = Factor(ctx, name, how, W=128)
    assert np.array_equal(wide.full[:, :c.mp], f.full)
    assert bits(wide.logdet()) == bits(got)


def test_factor_logdet_never_reads_the_padding(ctx):
    """A (m = 385, mp = 512): NaN on the padding's diagonal, 385..511, behind the factorization.  A kernel that walks to mp
    would return NaN."""
    f = Factor(ctx, "A")
    c = f.c
    want = f.logdet()
    full = f.full.copy()
    pad = np.arange(c.m, c.mp)
    assert (full[pad, pad] == 1.0).all()                           # the identity padding
    full[pad, pad] = np.nan
    ctx.upload_into(f.S.ptr, full)
    assert bits(f.logdet()) == bits(want) and np.isfinite(want).all()


@pytest.mark.parametrize("name", ["A", "C"])
def test_factor_logdet_reports_a_bad_pivot_as_nan_and_leaves_the_status_alone(ctx, name):
    f = Factor(ctx, name)
    c = f.c
    ctx.sync()
    before = ctx.solve_status(clear=False)
    assert before.clean
    rest = np.delete(f.diag, c.m - 1).min()
    for planted in (0.0, -0.25, float("nan"), float("inf")):
        f.poke(c.m - 1, planted)
        got = f.logdet()
        assert np.isnan(got[0]), planted
        if planted <= 0.0:
            assert got[1] == planted
        else:                                                      # (NaN, inf: the smallest entry that is a number)
            assert got[1] == rest
    f.poke(c.m - 1, f.diag[c.m - 1])
    assert np.isfinite(f.logdet()).all()
    assert ctx.solve_status(clear=False) == before


def test_factor_logdet_refusals_write_nothing(ctx):
    f = Factor(ctx, "C")
    c = f.c
    out = ctx.alloc(32)
    ctx.check(ctx.lib.oisat_memset(ctx.h, out.ptr, POISON, 32))
    good = dict(h=ctx.h, L=f.S.ptr, m=c.m, ld=c.mp, out=out.ptr)
    for change in (dict(h=None), dict(L=None), dict(out=None), dict(m=0), dict(m=-1), dict(ld=c.mp - 1), dict(ld=0), dict(m=c.mp + 1)):
        a = {**good, **change}
        assert ctx.lib.oisat_factor_logdet(a["h"], a["L"], a["m"], a["ld"], a["out"]) == EINVAL, change
    ctx.sync()
    assert (ctx.download(out.ptr, (4,), np.uint64) == F64_POISON.view(np.uint64)).all()
    assert ctx.lib.oisat_factor_logdet(*good.values()) == 0


# ---- plans on the cases -----------------------------------------------------------------------------------------------------------------
_GRID = {}


def grid36():
    if not _GRID:
        _GRID["p"] = syn.point_obs_case(rc.GRID[0], rc.GRID[1], 8, 36)
    return _GRID["p"]


def plan_for(name, d):
    """A fresh plan that holds the case's observations (its sigma_b, its variances) with the innovations d."""
    c, p = rc.case(name), grid36()
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=c.m, dtype=np.float64)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs_direct(c.lat, c.lon, c.osig, c.ovar, d)
    return plan


def chi2_bar(name, d, resid):
    """|d^T z - d^T S^-1 d| = |d^T S^-1 r| <= |d| |r| / lambda_min(S) <= resid |d|^2 / min(R)."""
    return resid * float(d @ d) / float(rc.case(name).ovar.min())


# ---- 6. log_likelihood() against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,scale_b", [("A", "gaussian", 1.0), ("B", "gaussian", 1.0), ("C", "gaussian", 1.0),
                                                ("B600", "gaussian", 1.0), ("B600", "soar", 1.0), ("B600", "gaspari_cohn", 1.0),
                                                ("A", "gaussian", 100.0)])
def test_log_likelihood_against_float64(ctx, name, model, scale_b):
    """Measured on an MI355X: see DESIGN.md section 4.2i."""
    c = rc.case(name)
    d = lc.draw(name, model, 1.0, 1.0, 2)
    plan = plan_for(name, d)
    plan.set_error_scales(scale_b, 1.0)
    resid = plan.run(c.L_km, check_pd=True, want_resid=True, corr=model, exact_factor=True)
    got = plan.log_likelihood()
    ref = lc.loglik64(name, model, d, scale_b=scale_b)
    bar = chi2_bar(name, d, resid[-1])
    print(f"case {name} {model} scale_b {scale_b:g}: |logdet - ref| {abs(got['logdet'] - ref['logdet']):.3g} of {ref['logdet']:.6g}; "
          f"|chi2 - ref| {abs(got['chi2'] - ref['chi2']):.3g} of {ref['chi2']:.6g}, bar {bar:.3g} (resid {resid[-1]:.3g}); "
          f"min pivot {got['min_pivot']:.4g}")
    assert got["m"] == c.m and got["min_pivot"] > 0.0
    assert abs(got["logdet"] - ref["logdet"]) <= LOGDET_BAR
    assert abs(got["chi2"] - ref["chi2"]) <= bar
    assert got["dd"] == pytest.approx(ref["dd"], rel=1e-14)
    assert got["chi2_per_obs"] == got["chi2"] / c.m
    assert got["neg2_log_likelihood"] == c.m * math.log(2.0 * math.pi) + got["logdet"] + got["chi2"]


def test_log_likelihood_wants_the_exact_factor_and_the_pivot_check(ctx):
    c = rc.case("C")
    plan = plan_for("C", lc.draw("C", "gaussian", 1.0, 1.0, 2))
    with pytest.raises(ValueError, match="exact_factor"):
        plan.log_likelihood()
    for kw in ({}, dict(check_pd=True), dict(exact_factor=True)):
        plan.run(c.L_km, **kw)
        with pytest.raises(ValueError, match="exact_factor"):
            plan.log_likelihood()
    plan.run(c.L_km, check_pd=True, exact_factor=True)
    first = plan.log_likelihood()
    assert plan.log_likelihood() == first
    plan.set_error_scales(2.0, 1.0)                                # new scales: the factor in HBM is no longer theirs
    with pytest.raises(ValueError, match="exact_factor"):
        plan.log_likelihood()
    # fields=False leaves the fields alone; the default writes them, and exact_factor changes nothing the analysis' bar could see
    plan.set_error_scales(1.0, 1.0)
    plan.run(c.L_km, check_pd=True)
    xa0, inc0 = plan.download()
    plan.run(2.0 * c.L_km, check_pd=True, exact_factor=True, fields=False)
    xa1, inc1 = plan.download()
    assert xa1.tobytes() == xa0.tobytes() and inc1.tobytes() == inc0.tobytes()


# ---- 7. the fit end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B600"])
@pytest.mark.parametrize("mode,truth", [("background", (4.0, 1.0)), ("both", (4.0, 0.5))])
@pytest.mark.parametrize("seed", lc.SEEDS)
def test_fit_error_scales_against_the_float64_search(ctx, name, mode, truth, seed):
    """Measured on an MI355X: see DESIGN.md section 4.2i."""
    c = rc.case(name)
    d = lc.draw(name, "gaussian", truth[0], truth[1], seed)
    prof = lc.Profile(name, "gaussian", d)
    J64 = prof.J(mode)
    plan = plan_for(name, d)
    fit = plan.fit_error_scales(c.L_km, mode=mode)
    ref = dense.profile_search(J64)
    assert fit["found"] and not fit["at_bound"] and fit["mode"] == mode and fit["nevals"] == len(fit["evaluations"]) <= 27
    assert fit["ratio"] == pytest.approx(fit["scale_b"] / fit["scale_o"], rel=1e-15)
    ev = [(x, J) for x, J in fit["evaluations"] if np.isfinite(J)]
    assert len(ev) == len(fit["evaluations"])                      # nothing failed on these cases
    assert len(fit["residuals"]) == len(ev) and all(0.0 <= r <= dense.REFINE_TOL for r in fit["residuals"])
    # per evaluation: 0.05 for the log-determinant plus the chi2 bar of the likelihood test at the residual THAT solve reported, b.
    # J_b holds chi2 itself; J_r holds m ln chi2, and |m ln(chi2 + e) - m ln chi2| <= m b / (chi2 - b) for |e| <= b < chi2
    off, bars = [], []
    for (x, J), resid in zip(ev, fit["residuals"]):
        b = chi2_bar(name, d, resid)
        if mode == "both":
            chi2_64 = float(prof.parts(x)[1])
            assert b < chi2_64
            b = c.m * b / (chi2_64 - b)
        off.append(abs(J - float(J64(x))))
        bars.append(LOGDET_BAR + b)
    worst = int(np.argmax(np.array(off) / np.array(bars)))
    delta, bar = max(off), bars[worst]
    assert all(o <= b for o, b in zip(off, bars)), (off[worst], bars[worst])
    x_dev = math.log(fit["ratio"])
    gap = float(J64(x_dev)) - ref["J"]
    lik = fit["likelihood"]
    print(f"case {name} {mode} seed {seed}: scale_b {fit['scale_b']:.4f} scale_o {fit['scale_o']:.4f} se_ln {fit['se_ln']:.3f} "
          f"nevals {fit['nevals']}; delta {delta:.3g}, worst |J_dev - J_64| / bar {off[worst] / bar:.3g} (bar there {bar:.3g}, largest "
          f"residual {max(fit['residuals']):.3g}); J64(x_dev) - J64(x_64) {gap:.3g} (bar {2 * delta + 0.02:.3g}); "
          f"x_dev - x_64 {x_dev - ref['x']:+.3g}; chi2/m at the result {lik['chi2_per_obs']:.9f}")
    assert gap <= 2.0 * delta + 0.02
    assert abs(x_dev - math.log(truth[0] / truth[1])) <= 3.0 * fit["se_ln"]
    if mode == "both":
        assert fit["scale_o"] != 1.0 and abs(lik["chi2_per_obs"] - 1.0) <= 1e-6
    else:
        assert fit["scale_o"] == 1.0 and fit["scale_b"] == fit["ratio"]
    # the plan is left at the result: its fields are those of a fresh plan run there
    assert plan._scales == (fit["scale_b"], fit["scale_o"])
    xa, inc = plan.download()
    fresh = plan_for(name, d)
    fresh.set_error_scales(fit["scale_b"], fit["scale_o"])
    fresh.run(c.L_km, check_pd=True, exact_factor=True)
    xa2, inc2 = fresh.download()
    assert xa.tobytes() == xa2.tobytes() and inc.tobytes() == inc2.tobytes() and np.abs(inc).max() > 0
    assert fresh.log_likelihood() == lik
    # ... and a new load puts the scales back
    plan.load_obs_direct(c.lat, c.lon, c.osig, c.ovar, d)
    assert plan._scales == (1.0, 1.0)
    assert ctx.download(plan.gsig.ptr, (plan.n,), np.float64).tobytes() == plan._gsig0.tobytes()
    assert ctx.download(plan.ovar.ptr, (c.m,), np.float64).tobytes() == c.ovar.tobytes()


def test_too_few_observations_make_no_fit(ctx):
    c, p = rc.case("C"), grid36()
    d = lc.draw("C", "gaussian", 4.0, 1.0, 2)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=31, dtype=np.float64)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs_direct(c.lat[:31], c.lon[:31], c.osig[:31], c.ovar[:31], d[:31])
    fit = plan.fit_error_scales(c.L_km)
    assert not fit["found"] and fit["scale_b"] == fit["scale_o"] == 1.0 and fit["nevals"] == 0 and fit["evaluations"] == []
    assert fit["likelihood"]["m"] == 31 and np.abs(plan.download()[1]).max() > 0       # the analysis proceeds as it does today


# ---- 8. OI_dense ------------------------------------------------------------------------------------------------------------------------
DEFAULT_KEYS = {"nobs", "residuals", "cells", "z"}


def test_oi_dense_fits_on_the_superobservations_and_reports_at_the_fitted_scale(ctx):
    c = syn.diag_case(36, 72, 600, 4711)
    labels = np.zeros(c.lat.shape, dtype=np.int64)
    labels[(c.lat > 20.0) & (c.lat < 50.0)] = 1
    labels[(c.lat < -30.0) & (c.lon > 100.0)] = 2
    L, scale = 600.0, 0.5
    kw = dict(superob=10.0, regions=labels, want_error="mc", nprobe=128, dtype=np.float64)
    xb, inc, info = dense.OI_dense(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, scale=scale, fit_scale="background", **kw)
    fit = info["scale_fit"]
    m = info["superob"]["nobs"]
    print(f"{info['nobs']} observations in {m} superobservations: scale_b {fit['scale_b']:.4f}, se_ln {fit['se_ln']:.3f}, "
          f"nevals {fit['nevals']}, chi2/m {info['likelihood']['chi2_per_obs']:.4f}")
    assert fit["found"] and fit["mode"] == "background" and fit["scale_o"] == 1.0 and fit["scale_b"] != 1.0
    assert 32 <= m < info["nobs"] == 600 and fit["likelihood"]["m"] == info["likelihood"]["m"] == m     # the fit is the superobbed system's
    xb2, inc2, info2 = dense.OI_dense(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, scale=scale * fit["scale_b"], likelihood=True, **kw)
    assert xb.tobytes() == xb2.tobytes() and inc.tobytes() == inc2.tobytes()
    assert info["err"].tobytes() == info2["err"].tobytes() and info["ak_obs"].tobytes() == info2["ak_obs"].tobytes()
    for key in ("posterior_cov", "prior_cov", "posterior_sd", "prior_sd", "analysis_mean"):
        assert info["regions"][key].tobytes() == info2["regions"][key].tobytes(), key
    assert info["likelihood"] == info2["likelihood"] and "scale_fit" not in info2
    # the search's own closing run had the same optimum in front of it: the same likelihood within the solves' tolerance
    assert info["likelihood"]["neg2_log_likelihood"] == pytest.approx(fit["likelihood"]["neg2_log_likelihood"], abs=1e-3)
    assert set(info) == set(info2) | {"scale_fit"}
    # default calls return the keys they always did
    _, _, plain = dense.OI_dense(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, scale=scale, dtype=np.float64)
    assert set(plain) == DEFAULT_KEYS
    _, _, lk = dense.OI_dense(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, scale=scale, dtype=np.float64, likelihood=True)
    assert set(lk) == DEFAULT_KEYS | {"likelihood"} and lk["likelihood"]["m"] == 600
    # no observation at all: nothing to fit
    Y = np.full(c.Y.shape, np.nan)
    _, inc0, none = dense.OI_dense(c.Xa, Y, c.Sa, Y.copy(), c.lat, c.lon, L, fit_scale="both", dtype=np.float64)
    assert not inc0.any() and none["likelihood"] is None
    assert none["scale_fit"]["found"] is False and none["scale_fit"]["scale_b"] == none["scale_fit"]["scale_o"] == 1.0


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------------------
OI_INFO_KEYS = {"mode", "corr_length_km", "correlation", "scale", "reg_index", "knee_found", "nobs", "unobserved", "want_error"}


def test_the_driver_fits_the_scale_in_dense_mode_only(ctx, monkeypatch, capsys):
    from oisatgmi.driver import oisatgmi
    c = syn.diag_case(24, 48, 300, 4703)
    for var in ("OISAT_OI_QC", "OISAT_CORRELATION", "OISAT_UNOBSERVED", "OISAT_OI_SUPEROB", "OISAT_OI_REGIONS", "OISAT_OI_SCALE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OISAT_OI_ERROR", "0")
    monkeypatch.setenv("OISAT_CORR_LENGTH_KM", "500")

    def facade(mode, **attrs):
        o = oisatgmi()
        o.ctm_averaged_vcd, o.sat_averaged_vcd, o.sat_averaged_error = c.Xa.copy(), c.Y.copy(), c.sat_err.copy()
        o.grid_lat, o.grid_lon, o.oi_mode = c.lat, c.lon, mode
        for k, v in attrs.items():
            setattr(o, k, v)
        return o

    plain = facade("dense")
    plain.oi("TROPOMI")
    assert set(plain.oi_info) == OI_INFO_KEYS
    capsys.readouterr()
    o = facade("dense", oi_scale="ml")
    o.oi("TROPOMI")
    said = capsys.readouterr().out
    info = o.oi_info
    fit = info["scale_fit"]
    assert set(info) == OI_INFO_KEYS | {"scale_knee", "scale_fit", "likelihood"}
    assert "The maximum-likelihood error scales are" in said and "The regularization factor is" in said
    assert fit["found"] and fit["mode"] == "background" and info["scale_knee"] == plain.oi_info["scale"]
    assert info["scale"] == info["scale_knee"] * fit["scale_b"] and info["likelihood"]["m"] == info["nobs"]
    # ... which is the analysis a forced scale of that size makes
    assert not np.array_equal(o.ctm_averaged_vcd_corrected, plain.ctm_averaged_vcd_corrected)
    monkeypatch.setenv("OISAT_OI_SCALE", "ml:both")                # the variable; both scales
    o2 = facade("dense")
    o2.oi("TROPOMI")
    fit2 = o2.oi_info["scale_fit"]
    assert fit2["mode"] == "both" and fit2["scale_o"] != 1.0 and abs(o2.oi_info["likelihood"]["chi2_per_obs"] - 1.0) <= 1e-3
    for mode in ("tiled", "diag"):
        with pytest.raises(ValueError, match="belongs to the dense mode"):
            facade(mode).oi("TROPOMI")
    monkeypatch.delenv("OISAT_OI_SCALE")
    again = facade("dense")                                        # unset: nothing changes, nothing is added
    again.oi("TROPOMI")
    assert set(again.oi_info) == OI_INFO_KEYS
    assert again.ctm_averaged_vcd_corrected.tobytes() == plain.ctm_averaged_vcd_corrected.tobytes()
