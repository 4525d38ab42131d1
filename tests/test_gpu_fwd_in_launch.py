"""GPU tests of ``DenseAnalysis.run()`` with the first forward sweep inside the factorization launch
(``oisat_potrf_env_fwd``) and the build that zero-fills only what the last envelope left outside the new one
(``oisat_cov_build_env_zeroed``).  Neither changes a floating-point operation, so everything here is bit for bit: the fields
with and without the sweep in the launch, the factor and the zeros around it on a plan that keeps its S over changing
tables against a fresh plan's, and a second month on the same plan against a fresh plan's."""
import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
NB = 128
SWITCH = "OISAT_FWD_IN_LAUNCH"
CUT = "OISAT_FACTOR_CUT_BITS"


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_task_graph(c.h, -1))


def _case(ny, nx, nobs, seed, swaths=False):
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    return p, cell, y


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


@pytest.mark.parametrize("name,ny,nx,nobs,seed,L,swaths,bits", [("config2", 360, 720, 10000, 4000, 500.0, False, None),
                                                               ("swath_20k", 360, 720, 20000, 4001, 300.0, True, None),
                                                               ("narrow_3k", 72, 144, 3000, 9000, 300.0, False, 28)])
def test_run_has_the_same_bits_with_and_without_the_sweep_in_the_launch(ctx, monkeypatch, name, ny, nx, nobs, seed, L, swaths, bits):
    """z, xa, inc and the residual list of ``run()``: the default (the sweep rides, schedule 2) against ``OISAT_FWD_IN_LAUNCH=0``
    (schedule 1), and the same pair with the task graph off, where both take the fallback (schedule 0)."""
    if bits is None:
        monkeypatch.delenv(CUT, raising=False)
    else:
        monkeypatch.setenv(CUT, str(bits))
    p, cell, y = _case(ny, nx, nobs, seed, swaths)
    plan = _plan(ctx, p, y.size)
    try:
        for mode, want in ((-1, (dense.SCHEDULE_ENV_DAG_FWD, dense.SCHEDULE_ENV_DAG)), (0, (0, 0))):
            ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, mode))
            monkeypatch.delenv(SWITCH, raising=False)
            rides = _run(plan, p, cell, y, L)
            assert plan.last_schedule == want[0]
            again = _run(plan, p, cell, y, L)               # (second run of the plan: the build trusts the first one's zeros)
            monkeypatch.setenv(SWITCH, "0")
            plain = _run(plan, p, cell, y, L)
            assert plan.last_schedule == want[1]
            print(f"{name}, task graph {mode}: residuals {rides[0]}")
            assert rides[0][-1] <= dense.REFINE_TOL
            _same(rides, plain)
            _same(again, plain)
            assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    finally:
        ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, -1))


def _inside_mask(first, mp):
    nb = mp // NB
    blk = np.arange(nb)[None, :] >= first[:nb, None]
    return np.kron(blk, np.ones((NB, NB), dtype=bool)) & np.tril(np.ones((mp, mp), dtype=bool))


def test_zero_claim_over_changing_tables(ctx, monkeypatch):
    """A plan that owns its S, poisoned before the first run, then 2^-28 -> 2^-52 -> recursion -> 2^-52 -> 2^-28: after every
    run every lower tile outside that run's envelope is exactly zero and the factor inside equals a fresh plan's bit for bit;
    the readers of the last factor agree with the fresh plan's."""
    monkeypatch.delenv(SWITCH, raising=False)
    p, cell, y = _case(72, 144, 3000, 9000)
    L = 300.0
    plan = _plan(ctx, p, y.size)
    mp = plan.mp_max
    low = np.tril(np.ones((mp, mp), dtype=bool))
    ctx.check(ctx.lib.oisat_memset(ctx.h, plan.S.ptr, 0x55, mp * mp * 4))
    tiles = []
    try:
        for step, (bits, mode) in enumerate(((28, -1), (52, -1), (28, 0), (52, -1), (28, -1))):
            monkeypatch.setenv(CUT, str(bits))
            ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, mode))
            kept = _run(plan, p, cell, y, L)
            assert plan.last_schedule == (dense.SCHEDULE_ENV_DAG_FWD if mode == -1 else 0)
            assert (plan._zero_claim is not None) == (mode == -1)
            first = plan._envelope(plan._g)[: mp // NB].copy()
            tiles.append(int(np.sum(np.arange(first.size) - first + 1)))
            S_kept = ctx.download(plan.S.ptr, (mp, mp), np.float32)
            last = step == 4
            if last:
                pe_kept, gd_kept = plan.posterior_error().copy(), plan.gain_diag().copy()
            fresh = _plan(ctx, p, y.size)
            new = _run(fresh, p, cell, y, L)
            S_new = ctx.download(fresh.S.ptr, (mp, mp), np.float32)
            inside = _inside_mask(first, mp)
            outside = low & ~inside
            assert np.isfinite(S_kept[low]).all()
            assert not S_kept[outside].any(), f"step {step}: {int(np.count_nonzero(S_kept[outside]))} non-zeros outside the envelope"
            assert np.array_equal(S_kept[inside], S_new[inside]), f"step {step}"
            _same(kept, new)
            if last:
                assert np.array_equal(pe_kept, fresh.posterior_error())
                assert np.array_equal(gd_kept, fresh.gain_diag())
            del fresh, S_new, S_kept
    finally:
        ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, -1))
    print("tiles inside the tables:", tiles)
    assert tiles[0] < tiles[1]                              # (the two tables differ: the claim had something to do)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_envelope_change_between_months(ctx, monkeypatch):
    """Other observations on the same plan -- another envelope with the same leading dimension, then a smaller month with
    another leading dimension (the claim does not carry over) -- give the fields of a fresh plan, bit for bit."""
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setenv(CUT, "28")
    L = 300.0
    months = [_case(72, 144, 3000, 9000), _case(72, 144, 3000, 9107), _case(72, 144, 2500, 9211), _case(72, 144, 3000, 9000)]
    plan = _plan(ctx, months[0][0], 3000)
    tables = []
    for p, cell, y in months:
        kept = _run(plan, p, cell, y, L)
        assert plan.last_schedule == dense.SCHEDULE_ENV_DAG_FWD
        tables.append(plan._envelope(plan._g)[: plan.mp // NB].copy())
        fresh = _plan(ctx, p, 3000)
        new = _run(fresh, p, cell, y, L)
        _same(kept, new)
        del fresh
    assert tables[0].size == tables[1].size and not np.array_equal(tables[0], tables[1])
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
