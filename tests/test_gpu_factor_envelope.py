"""GPU tests of the fp32 factor's own cut-off (``oisat_factor_envelope``, kFactorCutBits = 28): the refined analysis with
the narrow factor forced at chain-bound sizes against the float64 oracle, the factor's bits inside the narrow table, the
default path at chain-bound sizes (unchanged), the readers of the factor that do not refine, and the headline month on
the default path."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

pytestmark = pytest.mark.gpu
NB = 128
FACTOR_CUT_BITS = 28               # kFactorCutBits (csrc/dense_tables.hip)
OVERRIDE = "OISAT_FACTOR_CUT_BITS"


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_task_graph(c.h, -1))


def _factor_envelope(lat_sorted, g):
    lib = _hip.load_library()
    nb = -(-lat_sorted.size // NB)
    env = np.empty(2 * nb, dtype=np.int32)
    assert lib.oisat_factor_envelope(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data) == 0
    return env


def _tiles(first):
    return int(np.sum(np.arange(first.size) - first + 1))


def _plan(ctx, p, y, cell):
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    return plan


def _run(plan, p, y, cell, L, bits, monkeypatch):
    """One analysis with the factor's cut-off forced to 2^-bits (None: the default rule).  The observations are loaded
    again: a plan keeps its table per (observations, L)."""
    if bits is None:
        monkeypatch.delenv(OVERRIDE, raising=False)
    else:
        monkeypatch.setenv(OVERRIDE, str(bits))
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    resid = plan.run(L, refine=2, check_pd=True, want_resid=True)
    xa, inc = plan.download()
    return resid, xa.astype(np.float64), inc.astype(np.float64), plan.download_z()


@pytest.mark.parametrize("name,ny,nx,nobs,seed,L,swaths", [("config2", 360, 720, 10000, 4000, 500.0, False),
                                                          ("swath_20k", 360, 720, 20000, 4001, 300.0, True)])
def test_forced_narrow_analysis_against_oracle(ctx, monkeypatch, name, ny, nx, nobs, seed, L, swaths):
    """The narrow factor forced where the default keeps 2^-52: the refinement converges, z / inc / xa meet the oracle bars
    of test_enveloped_analysis_against_oracle_and_dense_path (2e-5, 1e-5, 1e-5), and the narrow run's z is at most twice as
    far from the float64 oracle as the 2^-52 run's (both are draws around the oracle at the rounding floor).  Measured on
    MI355X, 2^-28 | 2^-52: config 2 z 8.814e-7 | 8.793e-7, residuals 5.017e-6, 1.53e-10 | 4.989e-6, 1.48e-10; swath case z
    5.310e-7 | 5.307e-7, residuals 5.373e-6, 1.60e-10 | 5.346e-6, 1.78e-10 (the distance is the fp32 innovation's)."""
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = _plan(ctx, p, y, cell)
    narrow = _run(plan, p, y, cell, L, FACTOR_CUT_BITS, monkeypatch)
    wide = _run(plan, p, y, cell, L, 52, monkeypatch)
    import scipy.linalg as sla
    sb = np.sqrt(p.Sa.ravel())
    po = orc.unit_vectors(p.obs_lat, p.obs_lon)
    S = orc.gaussian_corr(po, po, L)
    S *= sb[cell][:, None]
    S *= sb[cell][None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    zr = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    del S
    sel = np.random.default_rng(3).choice(p.Xa.size, 4000, replace=False)
    pg = orc.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc_ref = sb[sel] * (orc.gaussian_corr(pg, po, L) @ (sb[cell] * zr))
    scale = np.abs(p.Xa).max()
    ez = {}
    for label, (resid, xa, inc, z) in ((FACTOR_CUT_BITS, narrow), (52, wide)):
        ez[label] = np.abs(z - zr).max() / np.abs(zr).max()
        ei = np.abs(inc.ravel()[sel] - inc_ref).max() / scale
        ex = np.abs(xa.ravel()[sel] - (p.Xa.ravel()[sel] + inc_ref)).max() / scale
        print(f"{name} 2^-{label}: residuals {resid}, z {ez[label]:.3e}, inc {ei:.3e}, xa {ex:.3e} against the oracle")
        assert resid[-1] <= dense.REFINE_TOL, resid
        assert ez[label] <= 2e-5 and ei <= 1e-5 and ex <= 1e-5
    assert ez[FACTOR_CUT_BITS] <= 2.0 * ez[52], ez


def _inside_mask(first, mp):
    nb = mp // NB
    blk = np.arange(nb)[None, :] >= first[:nb, None]
    return np.kron(blk, np.ones((NB, NB), dtype=bool)) & np.tril(np.ones((mp, mp), dtype=bool))


@pytest.mark.parametrize("m", [3000, 10000])
def test_narrow_factor_has_the_dense_factor_s_bits(ctx, monkeypatch, m):
    """Inside the narrow table the factor equals, bit for bit, the dense task-graph factor of the same zero-filled matrix,
    and is exactly zero outside (the method of tests/test_gpu_envelope.py; L = 300 km, table forced)."""
    lib = ctx.lib
    L_km = 300.0
    p = syn.point_obs_case(72, 144, m, 6000 + m)
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat, lon = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64), np.ravel(p.obs_lon)[o]
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    g = dense.decay_constant(L_km)
    monkeypatch.setenv(OVERRIDE, "52")
    wide = _factor_envelope(lat, g)
    monkeypatch.setenv(OVERRIDE, str(FACTOR_CUT_BITS))
    env = _factor_envelope(lat, g)
    mp = -(-m // NB) * NB
    nb = mp // NB
    first = env[:nb]
    print(f"m = {m}: tiles inside {_tiles(first)} (2^-52: {_tiles(wide[:nb])}) of {nb * (nb + 1) // 2}")
    assert _tiles(first) < _tiles(wide[:nb])
    oxyz = ctx.upload(dense.unit_vectors(lat, lon))
    osig = ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64)
    ovar = ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)
    env_dev = ctx.upload(env)
    S = ctx.alloc(mp * mp * 4)
    inside = _inside_mask(first, mp)
    low = np.tril(np.ones((mp, mp), dtype=bool))
    ctx.check(lib.oisat_set_task_graph(ctx.h, 1))
    try:
        runs = []
        for which in ("env", "dense"):
            ctx.check(lib.oisat_memset(ctx.h, S.ptr, 0x55, mp * mp * 4))
            ctx.check(lib.oisat_cov_build_env(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, g, S.ptr, mp, env_dev.ptr))
            info = C.c_int(-1)
            if which == "env":
                ctx.check(lib.oisat_potrf_env(ctx.h, S.ptr, m, mp, first.ctypes.data, env_dev.ptr, C.byref(info)))
            else:
                ctx.check(lib.oisat_potrf(ctx.h, S.ptr, m, mp, C.byref(info)))
            assert info.value == 0
            runs.append(ctx.download(S.ptr, (mp, mp), np.float32))
    finally:
        ctx.check(lib.oisat_set_task_graph(ctx.h, -1))
    a, b = runs
    assert np.isfinite(a[low]).all()
    assert np.array_equal(a[inside], b[inside])
    assert np.array_equal(a[low & ~inside], np.zeros(int((low & ~inside).sum()), dtype=np.float32))
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_default_path_unchanged_at_chain_bound_size(ctx, monkeypatch):
    """Config 2 is its chain: the default rule keeps the 2^-52 table, so xa, inc and z have the bits of the override at 52."""
    p = syn.point_obs_case(360, 720, 10000, 4000)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = _plan(ctx, p, y, cell)
    default = _run(plan, p, y, cell, 500.0, None, monkeypatch)
    forced = _run(plan, p, y, cell, 500.0, 52, monkeypatch)
    assert default[0] == forced[0]
    for u, v in zip(default[1:], forced[1:]):
        assert np.array_equal(u, v)


def test_readers_that_do_not_refine(ctx, monkeypatch):
    """``posterior_error`` and ``gain_diag`` read the factor ``run()`` left behind, without refinement.  3 000 observations,
    L = 300 km: forced narrow against 52, max-norm relative to the largest entry, is no larger than what the two schedules
    of the factorization (task graph / recursion) differ by at 52.  Measured on MI355X: posterior_error 0 against 1.2e-6,
    gain_diag 4.2e-11 against 3.1e-6."""
    p = syn.point_obs_case(72, 144, 3000, 9000)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = _plan(ctx, p, y, cell)

    def readers(bits, mode):
        ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, mode))
        _run(plan, p, y, cell, 300.0, bits, monkeypatch)
        first = plan._envelope(plan._g)[: plan.mp // NB].astype(np.int64)
        return plan.posterior_error().astype(np.float64), plan.gain_diag(), _tiles(first)

    try:
        pe_n, gd_n, tiles_n = readers(FACTOR_CUT_BITS, 1)
        pe_w, gd_w, tiles_w = readers(52, 1)
        pe_r, gd_r, _ = readers(52, 0)
    finally:
        ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, -1))
    assert tiles_n < tiles_w

    def dist(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())
    print(f"posterior_error: narrow to 52 {dist(pe_n, pe_w):.3e}, task graph to recursion {dist(pe_r, pe_w):.3e}; "
          f"gain_diag: {dist(gd_n, gd_w):.3e}, {dist(gd_r, gd_w):.3e}; tiles {tiles_n} / {tiles_w}")
    assert np.isfinite(pe_n).all() and np.isfinite(gd_n).all()
    assert dist(pe_n, pe_w) <= dist(pe_r, pe_w)
    assert dist(gd_n, gd_w) <= dist(gd_r, gd_w)


def test_headline_month_on_the_default_path(ctx, monkeypatch):
    """The benchmark's month (seed 4000) with the default rule: the narrow table is the one in use, the refinement ends below
    1e-7, and the float64 residual re-derived on the host for 96 random rows from the oracle's covariance formula is at
    rounding level (the checks of test_dense_config3_full_size_properties)."""
    monkeypatch.delenv(OVERRIDE, raising=False)
    p = syn.point_obs_case(720, 1440, 100000, 4000, swaths=True)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    L = 300.0
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    m = int(y.size)
    plan = _plan(ctx, p, y, cell)
    resid = plan.run(L, refine=2, check_pd=True, want_resid=True)
    first = plan._envelope(plan._g)[: plan.mp // NB].astype(np.int64)
    print(f"headline: tiles {_tiles(first)}, residuals {resid}")
    assert _tiles(first) == 62021
    assert resid[-1] < 1e-7 and resid[-1] < resid[0], resid
    z = plan.download_z()
    del plan
    assert np.isfinite(z).all()
    sb = np.sqrt(p.Sa.ravel())
    po = orc.unit_vectors(p.obs_lat, p.obs_lon)
    d = y - p.Xa.astype(np.float32).ravel()[cell].astype(np.float64)       # the innovation the float32 plan saw
    rows = np.random.default_rng(9).choice(m, 96, replace=False)
    Srows = orc.gaussian_corr(po[rows], po, L) * sb[cell][rows][:, None] * sb[cell][None, :]
    r = d[rows] - (Srows @ z + p.obs_var[rows] * z[rows])
    assert np.abs(r).max() <= 1e-6 * np.abs(d).max(), np.abs(r).max() / np.abs(d).max()
