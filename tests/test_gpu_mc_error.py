"""GPU tests of the randomized analysis error and averaging kernel: the probe fill, the backward row sweep ``X L^-1`` on
dense and enveloped factors, the probe spread under the three correlation models, and the estimate end to end against the
exact ``posterior_error()`` / ``gain_diag()`` under the two statistical conditions of tests/mc_error_cases.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import mc_error_cases as mc
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

pytestmark = pytest.mark.gpu
NB = 128
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def test_probe_fill_is_the_host_function_bit_for_bit(ctx):
    m, ldx, nrows, seed, first = 300, 384, 128, 99, 256
    X = ctx.alloc(nrows * ldx * 4)
    ctx.check(ctx.lib.oisat_memset(ctx.h, X.ptr, 0x55, nrows * ldx * 4))
    ctx.check(ctx.lib.oisat_probe_fill(ctx.h, seed, first, X.ptr, nrows, ldx, m))
    got = ctx.download(X.ptr, (nrows, ldx), np.float32)
    want = np.array([[mc.c_probe_sign(ctx.lib, seed, first + r, a) for a in range(m)] for r in range(nrows)], dtype=np.float32)
    assert np.array_equal(got[:, :m].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, m:].view(np.uint32), np.zeros((nrows, ldx - m), dtype=np.uint32))      # exact +0
    assert np.array_equal(want, mc.np_probe_sign(seed, first + np.arange(nrows)[:, None], np.arange(m)[None, :]))
    assert ctx.lib.oisat_probe_fill(ctx.h, seed, 0, X.ptr, nrows, 383, m) == EINVAL                      # ldx < roundup(m, 128)
    assert ctx.lib.oisat_probe_fill(ctx.h, seed, -1, X.ptr, nrows, ldx, m) == EINVAL


class Factor:
    """A factor on the context's handle: ``how`` = "potrf" (dense) or "env" (``oisat_cov_build_env`` + ``oisat_potrf_env``)."""

    def __init__(self, ctx, m, L_km, how, seed):
        lib = ctx.lib
        p = syn.point_obs_case(72, 144, m, seed)
        o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
        lat, lon = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64), np.ravel(p.obs_lon)[o]
        cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
        g = dense.decay_constant(L_km)
        self.m, self.mp = m, -(-m // NB) * NB
        self.nb = self.mp // NB
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
        self.bufs = [ctx.upload(dense.unit_vectors(lat, lon)), ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64),
                     ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)]
        self.S = ctx.alloc(self.mp * self.mp * 4)
        self.how, self.g = how, g
        self.first = np.zeros(self.nb, dtype=np.int32)
        if how == "env":
            env = np.empty(2 * self.nb, dtype=np.int32)
            assert lib.oisat_envelope(lat.ctypes.data, m, C.c_double(g), env.ctypes.data) == 0
            self.first = env[:self.nb].copy()
            self.env_dev = ctx.upload(env)
        self.refactor(ctx)
        self.host = ctx.download(self.S.ptr, (self.mp, self.mp), np.float32)
        self.L = np.tril(self.host.astype(np.float64))                # the lower triangle as it lies in HBM, padding included

    def refactor(self, ctx):
        """Build and factor again: the handle knows ONE factor (and keeps its inverted diagonal blocks), and other tests
        factor on the same handle in between.  Same bits every time."""
        lib, (oxyz, osig, ovar), m, mp = ctx.lib, self.bufs, self.m, self.mp
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
        ctx.check(lib.oisat_memset(ctx.h, self.S.ptr, 0x55, mp * mp * 4))
        info = C.c_int(-1)
        if self.how == "env":
            ctx.check(lib.oisat_cov_build_env(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, self.g, self.S.ptr, mp, self.env_dev.ptr))
            ctx.check(lib.oisat_potrf_env(ctx.h, self.S.ptr, m, mp, self.first.ctypes.data, self.env_dev.ptr, C.byref(info)))
        else:
            ctx.check(lib.oisat_cov_build(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, self.g, self.S.ptr, mp))
            ctx.check(lib.oisat_potrf(ctx.h, self.S.ptr, m, mp, C.byref(info)))
        assert info.value == 0

    def probes(self, ctx, nrows, seed=5):
        X = ctx.alloc(nrows * self.mp * 4)
        ctx.check(ctx.lib.oisat_probe_fill(ctx.h, seed, 0, X.ptr, nrows, self.mp, self.m))
        return X

    def bwd(self, ctx, X, nrows):
        ctx.check(ctx.lib.oisat_trsm_rows_bwd(ctx.h, self.S.ptr, self.m, self.mp, X.ptr, nrows, self.mp))
        return ctx.download(X.ptr, (nrows, self.mp), np.float32)


@pytest.fixture(scope="module")
def six_blocks(ctx):
    f = Factor(ctx, 700, 100.0, "env", 4700)
    assert f.nb == 6 and (f.first > 0).any(), f.first          # the envelope is really exercised
    return f


def _sweep_errors(ctx, f, nrows):
    """(backward error, forward error): max |result - float64 reference| / max |reference| of ``oisat_trsm_rows_bwd`` and of
    ``oisat_trsm_rows`` on the same factor and the same probes."""
    X = f.probes(ctx, nrows)
    x0 = ctx.download(X.ptr, (nrows, f.mp), np.float32).astype(np.float64)
    got_b = f.bwd(ctx, X, nrows).astype(np.float64)
    ref_b = sla.solve_triangular(f.L, x0.T, lower=True, trans="T").T            # Y L = X
    X2 = f.probes(ctx, nrows)
    ctx.check(ctx.lib.oisat_trsm_rows(ctx.h, f.S.ptr, f.m, f.mp, X2.ptr, nrows, f.mp))
    got_f = ctx.download(X2.ptr, (nrows, f.mp), np.float32).astype(np.float64)
    ref_f = sla.solve_triangular(f.L, x0.T, lower=True).T                       # Z L^T = X
    assert np.isfinite(got_b).all()
    return np.abs(got_b - ref_b).max() / np.abs(ref_b).max(), np.abs(got_f - ref_f).max() / np.abs(ref_f).max()


@pytest.mark.parametrize("m,L_km,how,nrows", [(100, 300.0, "potrf", 128), (250, 300.0, "potrf", 128), (700, 100.0, "env", 128),
                                              (700, 100.0, "env", 256)])
def test_backward_sweep_against_float64(ctx, six_blocks, m, L_km, how, nrows):
    """``X L^-1`` against scipy's float64 triangular solve on the downloaded factor.  The yardstick is measured in the same
    run: the existing forward sweep ``X L^-T`` on the same factor and probes against ITS float64 reference; the backward
    sweep -- the same arithmetic in the other direction -- must stay within 4 x that."""
    f = six_blocks if how == "env" else Factor(ctx, m, L_km, how, 4000 + m)
    f.refactor(ctx)
    eb, ef = _sweep_errors(ctx, f, nrows)
    print(f"m = {m} ({how}, {nrows} rows, first = {f.first}): backward {eb:.3e}, forward {ef:.3e}, ratio {eb / ef:.2f}")
    assert eb <= 4.0 * ef


def test_backward_sweep_is_repeatable_and_walks_the_envelope_only(ctx, six_blocks):
    f, lib = six_blocks, ctx.lib
    f.refactor(ctx)
    assert np.array_equal(ctx.download(f.S.ptr, (f.mp, f.mp), np.float32).view(np.uint32), f.host.view(np.uint32))
    nrows = 128
    a = f.bwd(ctx, f.probes(ctx, nrows), nrows)
    b = f.bwd(ctx, f.probes(ctx, nrows), nrows)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # every lower tile outside the envelope becomes NaN: nothing of it is read
    poisoned = f.host.copy()
    n_poisoned = 0
    for i in range(f.nb):
        for k in range(int(f.first[i])):
            poisoned[i * NB:(i + 1) * NB, k * NB:(k + 1) * NB] = np.nan
            n_poisoned += 1
    assert n_poisoned > 0
    ctx.upload_into(f.S.ptr, poisoned, dtype=np.float32)
    try:
        c = f.bwd(ctx, f.probes(ctx, nrows), nrows)
    finally:
        ctx.upload_into(f.S.ptr, f.host, dtype=np.float32)
    assert np.isfinite(c).all() and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    # values in the padding columns m..mp pass through unchanged and leak nowhere
    X = f.probes(ctx, nrows)
    x0 = ctx.download(X.ptr, (nrows, f.mp), np.float32)
    x0[:, f.m:] = np.random.default_rng(3).uniform(-4, 4, size=(nrows, f.mp - f.m)).astype(np.float32)
    ctx.upload_into(X.ptr, x0, dtype=np.float32)
    d = f.bwd(ctx, X, nrows)
    assert np.array_equal(d[:, f.m:].view(np.uint32), x0[:, f.m:].view(np.uint32))
    assert np.array_equal(d[:, :f.m].view(np.uint32), a[:, :f.m].view(np.uint32))
    # argument errors: OISAT_EINVAL, nothing written
    ctx.upload_into(X.ptr, x0, dtype=np.float32)
    other = ctx.alloc(64)
    for args in [(f.S.ptr, f.m, f.mp, X.ptr, 100, f.mp), (f.S.ptr, f.m, f.mp, X.ptr, nrows, f.mp - 4),
                 (other.ptr, f.m, f.mp, X.ptr, nrows, f.mp), (f.S.ptr, f.m - 1, f.mp, X.ptr, nrows, f.mp),
                 (f.S.ptr, f.m, f.mp, X.ptr + 4, nrows, f.mp), (f.S.ptr, f.m, f.mp, None, nrows, f.mp), (f.S.ptr, f.m, f.mp, X.ptr, 0, f.mp)]:
        assert lib.oisat_trsm_rows_bwd(ctx.h, *args) == EINVAL, args
    assert np.array_equal(ctx.download(X.ptr, (nrows, f.mp), np.float32).view(np.uint32), x0.view(np.uint32))


# ---- probe spread ------------------------------------------------------------------------------------------------------
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}
_spread_cache = {}


def _spread_setup(ctx, corr):
    """21 x 45 cells, 500 observations, the factor of a real run under ``corr`` and one panel of swept probes; the float64
    reference products t_ik (all 128 probes) are computed once per model and shared."""
    if corr not in _spread_cache:
        p = syn.point_obs_case(21, 45, 500, 77)
        plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=500, dtype=np.float32, ctx=ctx)
        plan.load_background(p.Xa, p.Sa)
        cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
        plan.load_obs(p.obs_lat, p.obs_lon, cell, p.obs_y, p.obs_var)
        plan.run(300.0, check_pd=True, corr=corr)
        plan.check()
        U = ctx.alloc(NB * plan.mp * 4)
        ctx.check(ctx.lib.oisat_probe_fill(ctx.h, 11, 0, U.ptr, NB, plan.mp, plan.m))
        ctx.check(ctx.lib.oisat_trsm_rows_bwd(ctx.h, plan.S.ptr, plan.m, plan.mp, U.ptr, NB, plan.mp))
        u = ctx.download(U.ptr, (NB, plan.mp), np.float32).astype(np.float64)[:, :plan.m]
        assert np.isfinite(u).all() and np.abs(u).max() > 0
        o = plan._order
        pg = dense.unit_vectors(np.ravel(p.lat), np.ravel(p.lon))
        po = dense.unit_vectors(np.ravel(p.obs_lat)[o], np.ravel(p.obs_lon)[o])
        d2 = np.ascontiguousarray(((pg[:, :, None] - po[:, None, :]) ** 2).sum(axis=0))
        cm = np.empty_like(d2)
        assert ctx.lib.oisat_corr_eval(KINDS[corr], plan._g, d2.ctypes.data, d2.size, cm.ctypes.data) == 0
        sig = np.sqrt(np.ravel(p.Sa).astype(np.float64))
        T = (cm * sig[:, None] * sig[cell[o]][None, :]) @ u.T                      # t_ik, float64
        out = ctx.alloc(2 * plan.n * 8)
        _spread_cache[corr] = (plan, U, T, out)
    return _spread_cache[corr]


def _spread(ctx, plan, U, out, K, windowed, grid=True, accumulate=0):
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, plan._kind))
    ny, nx = (plan._ny, plan._nx) if grid else (plan.n, 0)
    ctx.check(ctx.lib.oisat_probe_spread(ctx.h, plan.gxyz.ptr, plan.gsig.ptr, ny, nx, plan.oxyz.ptr, plan.osig.ptr, U.ptr, K, plan.mp,
                                         plan.m, plan._g, plan.glat.ptr if windowed else None, plan.olat.ptr if windowed else None,
                                         accumulate, out.at(0), out.at(plan.n * 8)))
    got = ctx.download(out.ptr, (2, plan.n), np.float64)
    return got[0], got[1]


def _spread_check(got2, got4, want2, want4, what):
    """|difference| <= 1e-3 x the largest reference entry, sum2 and sum4 each against its own: the deterministic error has to
    stay below 1/40 of the smallest statistical standard error the interface allows, sqrt(2 / 4096) = 0.022."""
    e2, e4 = np.abs(got2 - want2).max() / want2.max(), np.abs(got4 - want4).max() / want4.max()
    print(f"{what}: sum2 error {e2:.2e}, sum4 error {e4:.2e} of the largest entry (bound 1e-3)")
    assert e2 <= 1e-3 and e4 <= 1e-3


@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("corr", list(KINDS))
def test_probe_spread_against_float64(ctx, corr, K, windowed):
    plan, U, T, out = _spread_setup(ctx, corr)
    want2, want4 = (T[:, :K] ** 2).sum(axis=1), (T[:, :K] ** 4).sum(axis=1)
    ctx.check(ctx.lib.oisat_memset(ctx.h, out.ptr, 0x7f, 2 * plan.n * 8))      # (accumulate = 0 overwrites whatever is there)
    got2, got4 = _spread(ctx, plan, U, out, K, windowed)
    _spread_check(got2, got4, want2, want4, f"{corr}, K = {K}, {'windowed' if windowed else 'every pair'}")


@pytest.mark.parametrize("corr", list(KINDS))
def test_probe_spread_consecutive_cells_accumulate_and_arguments(ctx, corr):
    plan, U, T, out = _spread_setup(ctx, corr)
    K = 64
    want2, want4 = (T[:, :K] ** 2).sum(axis=1), (T[:, :K] ** 4).sum(axis=1)
    g2, g4 = _spread(ctx, plan, U, out, K, True, grid=False)                   # nx = 0: ny consecutive cells
    _spread_check(g2, g4, want2, want4, f"{corr}, consecutive cells")
    a2, a4 = _spread(ctx, plan, U, out, K, True, grid=False, accumulate=1)     # ... added to what is there
    assert np.array_equal(a2, g2 + g2) and np.array_equal(a4, g4 + g4)
    b2, b4 = _spread(ctx, plan, U, out, K, True, grid=True)                    # repeatable, and the patches overwrite
    c2, c4 = _spread(ctx, plan, U, out, K, True, grid=True)
    assert np.array_equal(b2, c2) and np.array_equal(b4, c4)
    for bad in (0, 16, 48, 4096 + 32, 8192):
        rc = ctx.lib.oisat_probe_spread(ctx.h, plan.gxyz.ptr, plan.gsig.ptr, plan._ny, plan._nx, plan.oxyz.ptr, plan.osig.ptr, U.ptr, bad,
                                        plan.mp, plan.m, plan._g, None, None, 0, out.at(0), out.at(plan.n * 8))
        assert rc == EINVAL, bad
    assert np.array_equal(ctx.download(out.ptr, (2, plan.n), np.float64)[0], c2)
    # probe_diag: the per-observation sums of the same panel
    u = ctx.download(U.ptr, (NB, plan.mp), np.float32).astype(np.float64)[:K, :plan.m]
    od = ctx.alloc(2 * plan.m * 8)
    for acc in (0, 1):
        ctx.check(ctx.lib.oisat_probe_diag(ctx.h, U.ptr, K, plan.mp, plan.m, acc, od.at(0), od.at(plan.m * 8)))
    d = ctx.download(od.ptr, (2, plan.m), np.float64)
    np.testing.assert_allclose(d[0], 2 * (u ** 2).sum(axis=0), rtol=1e-13)
    np.testing.assert_allclose(d[1], 2 * (u ** 4).sum(axis=0), rtol=1e-13)


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_estimate_meets_the_exact_diagnostics_within_its_own_standard_errors(ctx):
    """24 x 48 cells, 600 observations, L = 300 km, K = 1024: conditions (a) and (b) of tests/mc_error_cases.py against the
    exact ``posterior_error()`` and ``gain_diag()``, in the variables the estimator samples (q = sig^2 - err^2 and
    R s = 1 - ak; clipping A to [0, sig^2] only moves it towards the exact value).  Floors, for the entries without sampling
    noise: the exact error is a float32 (2^-23 of sig^2 in its square) and both sides come from fp32 triangular solves with the
    same factor (2^-16 of the estimated quantity, the order of an fp32 factorization's own residual)."""
    K = mc.K_E2E
    p = syn.point_obs_case(24, 48, 600, 11)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=600, dtype=np.float32, ctx=ctx, diag_chunk_rows=4096)
    plan.load_background(p.Xa, p.Sa)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, p.obs_y, p.obs_var)
    plan.run(300.0, check_pd=True)
    err_exact = plan.posterior_error().astype(np.float64)
    ak_exact = plan.gain_diag()
    est = plan.posterior_error_mc(nprobe=K, seed=mc.SEED)
    assert est["nprobe"] == K and est["err"].shape == p.lat.shape and est["err"].dtype == np.float32
    assert est["ak_obs"].shape == (600,) and est["err_se"].shape == p.lat.shape and est["ak_obs_se"].shape == (600,)
    sig2 = np.asarray(p.Sa, dtype=np.float64)
    R = np.asarray(p.obs_var, dtype=np.float64)
    mc.check_conditions(est["q"], est["q_se"], sig2 - err_exact ** 2, K, 2.0 ** -23 * sig2 + 2.0 ** -16 * est["q"], "q (cells)")
    mc.check_conditions(R * est["s"], R * est["s_se"], 1.0 - ak_exact, K, 2.0 ** -16 * R * est["s"], "R s = 1 - ak (observations)")
    # what the caller sees is those estimates: err^2 = clip(sig^2 - q), ak = 1 - R s, and their standard errors
    A = np.clip(sig2 - est["q"], 0.0, sig2)
    np.testing.assert_allclose(est["err"], np.sqrt(A), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(est["ak_obs"], 1.0 - R * est["s"])
    np.testing.assert_array_equal(est["ak_obs_se"], R * est["s_se"])
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(est["err_se"], np.where(A > 0, est["q_se"] / (2 * np.sqrt(A)), 0.0), rtol=1e-12)
    # same seed, same bits; another seed, other fields
    again = plan.posterior_error_mc(nprobe=K, seed=mc.SEED)
    for k in ("err", "err_se", "ak_obs", "ak_obs_se", "q", "s"):
        assert np.array_equal(est[k], again[k]), k
    other = plan.posterior_error_mc(nprobe=K, seed=mc.SEED + 1)
    assert not np.array_equal(est["q"], other["q"]) and not np.array_equal(est["s"], other["s"])


def test_oi_dense_and_the_driver_fill_the_same_fields_as_the_exact_mode(ctx, monkeypatch):
    c = syn.diag_case(24, 48, 500, 21)
    lat, lon = c.lat, c.lon
    xb0, inc0, exact = dense.OI_dense(c.Xa.copy(), c.Y.copy(), c.Sa, c.So, lat, lon, 300.0, want_error=True)
    xb1, inc1, est = dense.OI_dense(c.Xa.copy(), c.Y.copy(), c.Sa, c.So, lat, lon, 300.0, want_error="mc", nprobe=256, seed=3)
    assert np.array_equal(xb0, xb1) and np.array_equal(inc0, inc1)                   # the analysis itself is untouched
    assert est["error_method"] == "mc" and est["nprobe"] == 256 and "error_method" not in exact
    for k in ("err", "ak", "ak_obs"):
        assert est[k].shape == exact[k].shape and est[k].dtype == exact[k].dtype, k
        assert np.array_equal(np.isnan(est[k]), np.isnan(exact[k])), k
        assert np.isfinite(est[k][~np.isnan(exact[k])]).all(), k
    assert est["err_se"].shape == est["err"].shape and est["ak_obs_se"].shape == est["ak_obs"].shape
    assert np.isfinite(est["err_se"]).all() and np.isfinite(est["ak_obs_se"]).all()
    # gridded observations: the singly observed cells may take the second estimate; the combination stays within six of its own
    # standard errors of the exact error variance (floor: fp32 arithmetic on both sides, 2^-16 of sig^2)
    sig2 = np.asarray(c.Sa, dtype=np.float64)
    A, A_exact = est["err"].astype(np.float64) ** 2, exact["err"].astype(np.float64) ** 2
    A_se = 2.0 * est["err"] * est["err_se"]
    pos = A > 0                                                 # (a clipped cell reports no standard error: err_se = 0 where err = 0)
    z = (np.abs(A - A_exact) - 2.0 ** -16 * sig2)[pos] / np.maximum(A_se[pos], 1e-300)
    print(f"OI_dense mc: worst (|A - A_exact| - floor) / se = {z.max():.2f} (bound 6) over {int(pos.sum())} of {A.size} cells")
    assert np.all((np.abs(A - A_exact) <= 6.0 * A_se + 2.0 ** -16 * sig2)[pos])
    with pytest.raises(ValueError, match="want_error"):
        dense.OI_dense(c.Xa.copy(), c.Y.copy(), c.Sa, c.So, lat, lon, 300.0, want_error="exactish")

    def drive(setting):
        o = oisatgmi()
        o.ctm_averaged_vcd, o.sat_averaged_vcd = c.Xa.copy(), c.Y.copy()
        o.sat_averaged_error = c.sat_err.copy()
        o.grid_lat, o.grid_lon, o.oi_mode, o.oi_reg_index = lat, lon, "dense", 40
        monkeypatch.setenv("OISAT_OI_ERROR", setting)
        o.oi("OMI")
        return o
    a, b = drive("1"), drive("mc:256")
    assert b.oi_info["error_method"] == "mc" and b.oi_info["nprobe"] == 256 and b.oi_info["want_error"] == "mc"
    assert a.oi_info["want_error"] is True and "error_method" not in a.oi_info
    np.testing.assert_array_equal(a.ctm_averaged_vcd_corrected, b.ctm_averaged_vcd_corrected)
    for fa, fb in ((a.ak_OI, b.ak_OI), (a.error_OI, b.error_OI)):
        assert fa.shape == fb.shape and fa.dtype == fb.dtype
        assert np.array_equal(np.isnan(fa), np.isnan(fb)) and np.isfinite(fb[~np.isnan(fa)]).all()
    assert np.array_equal(a.ak_OI == 0, b.ak_OI == 0)
    assert b.oi_info["err_se"].shape == lat.shape
