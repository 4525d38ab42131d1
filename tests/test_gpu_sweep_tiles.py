"""GPU tests of the triangular sweeps' launch shapes (``oisat_trsv_plan``, ``OISAT_TRSV_TWO_TILES``, ``OISAT_TRSV_MAX_WGS``):
one or two LDS tiles per workgroup, a workgroup per block row or a few workgroups that claim row after row.  The shape
changes no floating-point operation and no order of one, so everything here is bit for bit: z, xa, inc and the residual list
of ``DenseAnalysis.run()``, and the solution of ``oisat_potrs``; and no workgroup may give up waiting."""
import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
NB = 128
TWO = "OISAT_TRSV_TWO_TILES"
WGS = "OISAT_TRSV_MAX_WGS"
CUT = "OISAT_FACTOR_CUT_BITS"
ENV = "OISAT_ENVELOPE"


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c


def _case(ny, nx, nobs, seed):
    p = syn.point_obs_case(ny, nx, nobs, seed)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    return p, cell, y


@pytest.fixture(scope="module")
def narrow_3k():
    return _case(72, 144, 3000, 9000)


def _plan(ctx, p, max_obs):
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(max_obs), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    return plan


def _run(plan, p, cell, y, L):
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    resid = plan.run(L, refine=2, check_pd=True, want_resid=True)
    xa, inc = plan.download()
    return resid, xa.copy(), inc.copy(), plan.download_z()


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


def _three_shapes(ctx, monkeypatch, case, L, wgs):
    """run() with two tiles forced, one tile forced and the default choice, the grid capped at `wgs` workgroups (or not)."""
    p, cell, y = case
    plan = _plan(ctx, p, y.size)
    _set(monkeypatch, WGS, wgs)
    runs = {}
    for two in ("1", "0", None):
        _set(monkeypatch, TWO, two)
        runs[two] = _run(plan, p, cell, y, L)
        assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0), f"two tiles {two}, {wgs} workgroups"
    print(f"residuals {runs['1'][0]}")
    assert runs["1"][0][-1] <= dense.REFINE_TOL
    _same(runs["1"], runs["0"])
    _same(runs["1"], runs[None])
    return runs["1"]


@pytest.mark.parametrize("wgs", [4, 1])
def test_few_workgroups_serve_many_rows_of_a_narrow_band(ctx, monkeypatch, narrow_3k, wgs):
    """3 000 observations cut at 2^-28: 24 block rows with a narrow band on 4 workgroups -- the headline's regime at the
    smallest size that has it -- and on ONE workgroup, which serves every row in ticket order.  The capped launches also
    give the bits of the uncapped one."""
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.setenv(CUT, "28")
    p, cell, y = narrow_3k
    plan = _plan(ctx, p, y.size)
    nb = -(-y.size // NB)
    capped = _three_shapes(ctx, monkeypatch, narrow_3k, 300.0, wgs)
    monkeypatch.delenv(WGS, raising=False)
    monkeypatch.delenv(TWO, raising=False)
    free = _run(plan, p, cell, y, 300.0)
    first = plan._envelope(plan._g)[:nb]
    band = int(np.max(np.arange(nb) - first) + 1)
    print(f"{nb} block rows, band {band}, {wgs} workgroups")
    assert nb == 24 and band < nb // 2
    _same(capped, free)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_dense_factor_on_three_workgroups(ctx, monkeypatch, narrow_3k):
    """The same month with the envelope off (a dense factor: every row walks every producer), two tiles forced on 3
    workgroups, against one tile and against the default."""
    monkeypatch.setenv(ENV, "0")
    monkeypatch.setenv(CUT, "28")
    _three_shapes(ctx, monkeypatch, narrow_3k, 300.0, 3)


def test_four_block_rows_with_a_padded_last_block(ctx, monkeypatch):
    """385 observations: 4 block rows, the last one a single observation and 127 rows of padding, row 0 of either sweep
    without a producer (T_b comes from the second tile, staged in front of a loop that never waits) -- on 2 workgroups,
    through run() and through oisat_potrs with a random right-hand side, enveloped and dense."""
    monkeypatch.delenv(CUT, raising=False)
    monkeypatch.delenv(ENV, raising=False)
    case = _case(72, 144, 385, 9385)
    _three_shapes(ctx, monkeypatch, case, 300.0, 2)

    lib = ctx.lib
    p = case[0]
    m = 385
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat, lon = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64), np.ravel(p.obs_lon)[o]
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    g = dense.decay_constant(300.0)
    mp = -(-m // NB) * NB
    nb = mp // NB
    env = np.empty(2 * nb, dtype=np.int32)
    assert lib.oisat_envelope(lat.ctypes.data, m, _hip.C.c_double(g), env.ctypes.data) == 0
    first = env[:nb]
    print("first =", first)
    oxyz = ctx.upload(dense.unit_vectors(lat, lon))
    osig = ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64)
    ovar = ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)
    env_dev = ctx.upload(env)
    S = ctx.alloc(mp * mp * 4)
    rhs = np.random.default_rng(385).normal(size=m)
    monkeypatch.setenv(WGS, "2")
    for enveloped in (True, False):
        ctx.check(lib.oisat_cov_build_env(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, g, S.ptr, mp, env_dev.ptr))
        if enveloped:
            ctx.check(lib.oisat_potrf_env(ctx.h, S.ptr, m, mp, first.ctypes.data, env_dev.ptr, None))
        else:
            ctx.check(lib.oisat_potrf(ctx.h, S.ptr, m, mp, None))
        z = {}
        for two in ("1", "0", None):
            _set(monkeypatch, TWO, two)
            zb = ctx.upload(rhs)
            ctx.check(lib.oisat_potrs(ctx.h, S.ptr, m, mp, zb.ptr))
            z[two] = ctx.download(zb.ptr, (m,), np.float64)
            assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
        assert np.isfinite(z["1"]).all() and np.abs(z["1"]).max() > 0
        assert np.array_equal(z["1"], z["0"])
        assert np.array_equal(z["1"], z[None])


def test_config2_keeps_its_bits(ctx, monkeypatch):
    """Config 2 (360 x 720, 1e4 observations, L = 500 km: 79 block rows, a CU per row): the default switches, which give
    it two tiles as before, against one tile forced."""
    for name in (CUT, ENV, WGS, TWO):
        monkeypatch.delenv(name, raising=False)
    p, cell, y = _case(360, 720, 10000, 4000)
    plan = _plan(ctx, p, y.size)
    default = _run(plan, p, cell, y, 500.0)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    monkeypatch.setenv(TWO, "0")
    one = _run(plan, p, cell, y, 500.0)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    print(f"residuals {default[0]}")
    assert default[0][-1] <= dense.REFINE_TOL
    _same(default, one)


def test_a_switch_that_is_no_switch_is_refused(ctx, monkeypatch, narrow_3k):
    """Anything but 0 | 1 and n >= 1 is an invalid argument, not a silent default."""
    p, cell, y = narrow_3k
    plan = _plan(ctx, p, y.size)
    for name, value in ((TWO, "2"), (TWO, "yes"), (WGS, "0"), (WGS, "-3"), (WGS, "4x")):
        monkeypatch.delenv(TWO, raising=False)
        monkeypatch.delenv(WGS, raising=False)
        monkeypatch.setenv(name, value)
        with pytest.raises(_hip.OisatError):
            _run(plan, p, cell, y, 300.0)
    monkeypatch.delenv(TWO, raising=False)
    monkeypatch.delenv(WGS, raising=False)
    ctx.sync()
    ctx.solve_status(clear=True)
