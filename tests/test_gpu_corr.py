"""The Gaspari-Cohn correlation on the device (``corr="gaspari_cohn"``, ``oisat_set_correlation``): S as built, the dense
analysis against a float64 host solve of the Gaspari-Cohn system, the Gaussian's bits next to it, the batched / tiled paths
and the diagnostics.  The references are float64 NumPy / SciPy written here and in tests/readers_cases.py (the oracle has the Gaussian only)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oisatgmi import _hip, dense, synthetic as syn
from readers_cases import chord2, corr_ref as _corr_ref, gc_ref          # the float64 restatements of the formulas in oisat.h

pytestmark = pytest.mark.gpu
NB = 128
GC = "gaspari_cohn"


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def corr_ref(pa, pb, L, model=GC):
    return _corr_ref(pa, pb, L, model)


def host_analysis(p, cell, y, L, sel, model=GC):
    """float64: z = S^-1 d by Cholesky, the increment on the cells ``sel``."""
    sb = np.sqrt(p.Sa.ravel())
    po = dense.unit_vectors(p.obs_lat, p.obs_lon)
    S = corr_ref(po, po, L, model)
    S *= sb[cell][:, None]
    S *= sb[cell][None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    z = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    pg = dense.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc = np.empty(sel.size)
    for i0 in range(0, sel.size, 4096):
        inc[i0:i0 + 4096] = sb[sel[i0:i0 + 4096]] * (corr_ref(pg[:, i0:i0 + 4096], po, L, model) @ (sb[cell] * z))
    return z, inc


# ---- 1. S as built ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [500.0, 3000.0])
def test_covariance_as_built(ctx, L, monkeypatch):
    """|S - S_ref| <= 3e-5 sig_a sig_b + 2^-23 |S_ref| off the diagonal of the lower triangle (fp32 Horner: terms <= 10, fewer
    than 20 roundings of 6e-8), sig^2 + var on it, identity padding, exact zeros beyond the support and outside the table."""
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    lib = ctx.lib
    p = syn.point_obs_case(72, 144, 385, 6385)
    m = int(p.obs_y.size)
    mp = -(-m // NB) * NB
    nb = mp // NB
    o = np.argsort(p.obs_lat, kind="stable")
    lat, lon = np.ascontiguousarray(p.obs_lat[o]), p.obs_lon[o]
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    sig, var = np.sqrt(p.Sa.ravel()[cell]), np.ascontiguousarray(p.obs_var[o])
    xyz = dense.unit_vectors(lat, lon)
    g = dense.decay_constant(L)
    zref = np.sqrt(0.6 * g * chord2(xyz, xyz))
    if L == 500.0:
        assert (zref < 1).any() and ((zref > 1) & (zref < 2)).any() and (zref > 2).any()
    ref = np.eye(mp)
    ref[:m, :m] = gc_ref(zref) * sig[:, None] * sig[None, :]
    ref[np.arange(m), np.arange(m)] = sig ** 2 + var
    ss = np.zeros((mp, mp))
    ss[:m, :m] = sig[:, None] * sig[None, :]
    env = np.empty(2 * nb, dtype=np.int32)
    assert lib.oisat_envelope_corr(1, lat.ctypes.data, m, C.c_double(g), env.ctypes.data) == 0
    first = env[:nb]
    if L == 3000.0:
        assert not first.any()
    else:
        assert first.any()
    d_xyz, d_sig, d_var, d_env = ctx.upload(xyz), ctx.upload(sig), ctx.upload(var), ctx.upload(env)
    S = ctx.alloc(mp * mp * 4)
    low = np.tril(np.ones((mp, mp), dtype=bool), -1)
    far = np.zeros((mp, mp), dtype=bool)
    far[:m, :m] = zref >= 2.0 * (1.0 + 1e-6)
    outside = np.zeros((mp, mp), dtype=bool)
    for i in range(nb):
        outside[i * NB:(i + 1) * NB, :first[i] * NB] = True
    ctx.check(lib.oisat_set_correlation(ctx.h, 1))
    try:
        for name in ("oisat_cov_build", "oisat_cov_build_env"):
            ctx.check(lib.oisat_memset(ctx.h, S.ptr, 0x55, mp * mp * 4))
            if name == "oisat_cov_build":
                ctx.check(lib.oisat_cov_build(ctx.h, d_xyz.ptr, d_sig.ptr, d_var.ptr, m, g, S.ptr, mp))
            else:
                ctx.check(lib.oisat_cov_build_env(ctx.h, d_xyz.ptr, d_sig.ptr, d_var.ptr, m, g, S.ptr, mp, d_env.ptr))
            got = ctx.download(S.ptr, (mp, mp), np.float32)
            err = np.abs(got.astype(np.float64) - ref)
            bound = 3e-5 * ss + 2.0 ** -23 * np.abs(ref)
            print(f"L = {L:g} {name}: max |S - S_ref| / (sig_a sig_b) off the diagonal = "
                  f"{(err[:m, :m][low[:m, :m]] / ss[:m, :m][low[:m, :m]]).max():.3e}")
            assert (err[low] <= bound[low]).all()
            dg = np.arange(mp)
            assert (err[dg, dg] <= 2.0 ** -23 * ref[dg, dg]).all()
            assert (got[m:, :][low[m:, :]] == 0.0).all() and (got[dg[m:], dg[m:]] == 1.0).all()
            assert (got[far & low] == 0.0).all()
            if name == "oisat_cov_build_env":
                assert (got[outside & low] == 0.0).all()
    finally:
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))


# ---- 2. the analysis against a float64 host solve ----------------------------------------------------------------------------
CASES = {"72x144_L300": (72, 144, 1000, 7000, False, 300.0), "72x144_L500": (72, 144, 1000, 7000, False, 500.0),
         "360x720_swaths_L300": (360, 720, 3000, 9000, True, 300.0)}


@functools.lru_cache(maxsize=None)
def _case(name):
    ny, nx, nobs, seed, swaths, L = CASES[name]
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    if ny == 72:
        sel = np.arange(ny * nx)
    else:                                                      # 4 000 random cells and the two rows next to each pole
        sel = np.unique(np.concatenate([np.random.default_rng(3).choice(ny * nx, 4000, replace=False), np.arange(2 * nx),
                                        np.arange((ny - 2) * nx, ny * nx)]))
    z, inc = host_analysis(p, cell, y, L, sel)
    zg, incg = host_analysis(p, cell, y, L, sel, model="gaussian")
    for a in (z, inc, zg, incg, sel):
        a.setflags(write=False)
    return p, cell, y, L, sel, z, inc, zg, incg


@pytest.mark.parametrize("envelope", ["1", "0"])
@pytest.mark.parametrize("name", list(CASES))
def test_analysis_against_float64_host_solve(ctx, monkeypatch, name, envelope):
    """The tolerances of test_enveloped_analysis_against_oracle_and_dense_path; the Gaussian's float64 answer lies more than
    100 x these tolerances away, so the wrong model cannot pass."""
    p, cell, y, L, sel, zr, inc_ref, zg, incg = _case(name)
    if name.startswith("360"):
        assert y.size == 2972
    scale = np.abs(p.Xa).max()
    assert np.abs(zg - zr).max() / np.abs(zr).max() > 100 * 2e-5 and np.abs(incg - inc_ref).max() / scale > 100 * 1e-5
    monkeypatch.setenv("OISAT_ENVELOPE", envelope)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    try:
        resid = plan.run(L, corr=GC, refine=2, check_pd=True, want_resid=True)
        xa, inc = plan.download()
        z = plan.download_z()
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    ez = np.abs(z - zr).max() / np.abs(zr).max()
    ei = np.abs(inc.ravel()[sel].astype(np.float64) - inc_ref).max() / scale
    ex = np.abs(xa.ravel()[sel].astype(np.float64) - (p.Xa.ravel()[sel] + inc_ref)).max() / scale
    print(f"{name} envelope={envelope}: residuals {resid}, z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e} against the host solve")
    assert resid[-1] <= dense.REFINE_TOL, resid
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5


# ---- 3. the Gaussian keeps its bits, no state leaks ----------------------------------------------------------------------------
def test_gaussian_bits_survive_a_gaspari_cohn_run(ctx, monkeypatch):
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    p, cell, y, _, _, _, _, _, _ = _case("72x144_L300")
    L = 300.0

    def make():
        plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
        plan.load_background(p.Xa, p.Sa)
        plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
        return plan

    def run(plan, corr):
        plan.run(L, refine=2, check_pd=True, corr=corr)
        xa, inc = plan.download()
        return xa.copy(), inc.copy(), plan.download_z().copy(), plan._envelope(plan._g, plan._kind)[: plan.mp // NB].copy()

    plan = make()
    try:
        first = run(plan, "gaussian")
        gc = run(plan, GC)
        again = run(plan, "gaussian")
        fresh = run(make(), "gaussian")
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    assert not np.array_equal(first[3], gc[3])                 # (a narrower table in between: the zero-claim is exercised)
    assert not np.array_equal(first[1], gc[1])
    for a, b, c in zip(first[:3], again[:3], fresh[:3]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


# ---- 4. batched and tiled ------------------------------------------------------------------------------------------------------
def test_tiled_and_batched(ctx, monkeypatch):
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    monkeypatch.delenv("OISAT_DAG_SOLVE", raising=False)
    ny, nx, L, tile = 72, 144, 300.0, 60.0
    c = syn.diag_case(ny, nx, 2000, 4242)
    halo = dense.GC_SUPPORT_PER_L * L
    assert halo == pytest.approx(3.6515 * L, rel=1e-4)
    try:
        xa1, inc1, info = dense.OI_tiled(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, tile_deg=tile, dtype=np.float32, corr=GC)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))          # (lane 0 of a pool is the process-wide handle)
    # every tile against a host float64 solve of its own system
    Y = np.where(c.Y < 0, 0.0, c.Y)
    cells = info["cells"]
    olat, olon = c.lat.ravel()[cells], c.lon.ravel()[cells]
    sb = np.sqrt(c.Sa.ravel())
    d = Y.ravel()[cells] - c.Xa.ravel()[cells]
    tiles = dense.tile_partition(c.lat, c.lon, olat, olon, tile, halo)
    assert len(tiles) == info["tiles"]
    inc_ref = np.zeros((ny, nx))
    for t in tiles:
        (y0, y1), (x0, x1) = t["rows"], t["cols"]
        o = t["obs"]
        po = dense.unit_vectors(olat[o], olon[o])
        so = sb[cells[o]]
        S = corr_ref(po, po, L) * so[:, None] * so[None, :]
        S[np.diag_indices_from(S)] += c.So.ravel()[cells[o]]
        z = sla.cho_solve(sla.cho_factor(S, lower=True), d[o])
        pg = dense.unit_vectors(c.lat[y0:y1, x0:x1], c.lon[y0:y1, x0:x1])
        inc_ref[y0:y1, x0:x1] = (np.sqrt(c.Sa[y0:y1, x0:x1]).ravel() * (corr_ref(pg, po, L) @ (so * z))).reshape(y1 - y0, x1 - x0)
    scale = np.abs(c.Xa).max()
    ei = np.abs(inc1 - inc_ref).max() / scale
    ex = np.abs(xa1 - (c.Xa + inc_ref)).max() / scale
    print(f"tiled Gaspari-Cohn: inc {ei:.3e}, xa {ex:.3e} against the per-tile host solves")
    assert ei <= 1e-5 and ex <= 1e-5
    # the one-launch analysis is Gaussian only: asked for, the batch takes the two calls -- the same bits
    monkeypatch.setenv("OISAT_DAG_SOLVE", "1")
    try:
        xa2, inc2, _ = dense.OI_tiled(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, tile_deg=tile, dtype=np.float32, corr=GC)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    monkeypatch.delenv("OISAT_DAG_SOLVE")
    assert np.array_equal(xa1, xa2) and np.array_equal(inc1, inc2)
    # batched=False: every lane runs its tiles' whole pipelines
    xa_f = np.where(np.isfinite(c.Xa), c.Xa, 0.0)
    for batched in (False, True):
        ta = dense.TiledAnalysis(c.lat, c.lon, tile_deg=tile, halo_km=halo, dtype=np.float32, batched=batched)
        try:
            ta.load(xa_f, c.Sa, olat, olon, c.Y.ravel()[cells], c.So.ravel()[cells])
            ta.run(L, refine=2, check_pd=True, corr=GC)
            xa3, inc3 = ta.download()
            if batched:                                        # a direct call of the one-launch analysis under Gaspari-Cohn
                bctx, bid = ta.factor.ctxs[0], ta.factor.ids[0]
                bctx.check(bctx.lib.oisat_set_correlation(bctx.h, 1))
                rc = bctx.lib.oisat_batch_analyse(bctx.h, bid, _hip.F32, dense.decay_constant(L), 2, None)
                assert rc == -1 and b"Gaussian only" in bctx.lib.oisat_last_error()       # OISAT_EINVAL
                bctx.check(bctx.lib.oisat_set_correlation(bctx.h, 0))
        finally:
            ta.close()
            ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))      # (lane 0 of a pool is the process-wide handle)
        e = max(np.abs(inc3 - inc1).max(), np.abs(xa3 - xa1).max()) / scale
        print(f"batched={batched} against OI_tiled: {e:.3e}")
        assert e <= 1e-5
        assert np.abs(inc3 - inc_ref).max() / scale <= 1e-5


# ---- 5. diagnostics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx,m,L", [(36, 72, 300, 800.0), (45, 90, 1100, 500.0)])
def test_posterior_error_and_gain_diag(ctx, ny, nx, m, L):
    """The tolerances of test_dense_posterior_error_and_gain_diag (tests/test_gpu_parity.py) against the float64 formulas."""
    p = syn.point_obs_case(ny, nx, m, 900 + m)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    sb = np.sqrt(p.Sa.ravel())
    po, pg = dense.unit_vectors(p.obs_lat, p.obs_lon), dense.unit_vectors(p.lat, p.lon)
    so = sb[cell]
    S = corr_ref(po, po, L) * so[:, None] * so[None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    Lf = sla.cholesky(S, lower=True)
    V = sla.solve_triangular(Lf, (corr_ref(pg, po, L) * sb[:, None] * so[None, :]).T, lower=True)
    err_ref = np.sqrt(np.maximum(sb ** 2 - (V * V).sum(axis=0), 0.0))
    Linv = sla.solve_triangular(Lf, np.eye(m), lower=True)
    ak_ref = 1.0 - p.obs_var * (Linv * Linv).sum(axis=0)
    try:
        xb, inc, info = dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, L, refine=2, dtype=np.float32, want_error=True,
                                       obs=dict(lat=p.obs_lat, lon=p.obs_lon, y=p.obs_y, var=p.obs_var), corr=GC)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    sig = np.sqrt(p.Sa).max()
    e = np.abs(info["err"].ravel() - err_ref).max() / sig
    print(f"{ny}x{nx} m={m}: err {e:.3e} of sig, ak_obs {np.abs(info['ak_obs'] - ak_ref).max():.3e}")
    assert e <= 2e-3
    np.testing.assert_allclose(info["ak_obs"], ak_ref, atol=2e-5, rtol=0)
    assert (info["err"] <= np.sqrt(p.Sa) * (1 + 1e-6)).all()
