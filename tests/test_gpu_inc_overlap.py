"""GPU tests of the increment under the correction's sweeps (``oisat_gain_solve_fields``, ``oisat_increment_update``;
csrc/dense_inc_update.inc, csrc/dense_solve.hip): the update kernel at the C ABI against a NumPy float64 sum, the converged-at-r_0
case, full runs with ``OISAT_INC_OVERLAP`` on against off and against the float64 oracle, two corrections, the guard, determinism
(the z0 snapshot and the event ordering) and the profiling mode.  Small systems: the switch forces the entry where the size rule
(``oisat_inc_overlap_plan``: 256 block rows) keeps it off."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

pytestmark = pytest.mark.gpu
NB = 128
SWITCH = "OISAT_INC_OVERLAP"
F32, F64 = 0, 1
# e = max|delta_fp32 - delta_f64| / max|delta_f64| of the update, the largest of the four months of profiles/EXPERIMENTS.md
# ("The increment under the correction's sweeps"), and the guard's threshold made from it (include/oisat.h: OISAT_INC_UPDATE_T)
E_MEASURED = 1.69e-4                                            # (NO2 seed 3003; the other three: 1.33e-4, 1.08e-4, 6.98e-5)
T_GUARD = 1.0 / 32768.0                                         # the largest power of two t with e t <= 2^-27
L_KM = 600.0


@contextlib.contextmanager
def _environ(**kw):
    """The library reads its switches at every call: set (None: unset) for the block, restored behind it."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.prof_enable(False)


def _case(seed=4000):
    """A 72 x 144 swath month of about 3 950 observations (31 block rows, the last one padded; not a multiple of 16), four of them
    moved: onto a cell centre of the 37 x 70 grid of the ABI test, next to both poles, and onto the date line."""
    p = syn.point_obs_case(72, 144, 4000, seed, swaths=True)
    lat, lon = np.array(p.obs_lat, dtype=np.float64), np.array(p.obs_lon, dtype=np.float64)
    lat[:4] = (-35.0, 89.9, -89.9, 12.3)
    lon[:4] = (-180.0 + 7 * 360.0 / 70, 10.0, -170.0, 179.999)
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    return p, lat, lon, cell, y


def _plan(ctx, case, dtype=np.float32):
    p, lat, lon, cell, y = case
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=dtype, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(lat, lon, cell, y, p.obs_var)
    return plan


def _run(plan, overlap, refine=2, tol=None, reload=None, **switches):
    """One ``DenseAnalysis.run`` under the switch: residuals, z (device order), xa and inc as stored."""
    with _environ(**dict(switches, **{SWITCH: overlap})):
        if reload is not None:                                  # (a plan keeps its factor tables per (observations, L))
            p, lat, lon, cell, y = reload
            plan.load_obs(lat, lon, cell, y, p.obs_var)
        resid = plan.run(L_KM, refine=refine, check_pd=True, want_resid=True, tol=tol)
        assert plan.last_inc_overlap == (str(overlap) == "1")
        xa, inc = plan.download()
        z = plan.ctx.download(plan.z.ptr, (plan.m,), np.float64)
    return dict(resid=resid, z=z, xa=xa.copy(), inc=inc.copy())


@pytest.fixture(scope="module")
def case():
    return _case()


@pytest.fixture(scope="module")
def plan32(ctx, case):
    return _plan(ctx, case, np.float32)


@pytest.fixture(scope="module")
def runs32(plan32):
    """The float32 plan with the switch off and on (tol: the default; refine 2), once."""
    return {"off": _run(plan32, 0), "on": _run(plan32, 1)}


@pytest.fixture(scope="module")
def oracle(case):
    p, lat, lon, cell, y = case
    want = orc.dense_oi(p.lat, p.lon, p.Xa, p.Sa, lat, lon, cell, y, p.obs_var, L_KM)
    return dict(xa=want["xa"], inc=want["inc"], z=want["z"], scale=np.abs(p.Xa).max())


def _against_oracle(plan, run, oracle):
    """z, inc, xa against the float64 oracle: the bars of tests/test_gpu_near_band.py (2e-5, 1e-5, 1e-5)."""
    z = plan._unsort(run["z"])
    ez = np.abs(z - oracle["z"]).max() / np.abs(oracle["z"]).max()
    ei = np.abs(run["inc"].astype(np.float64).ravel() - oracle["inc"]).max() / oracle["scale"]
    ex = np.abs(run["xa"].astype(np.float64).ravel() - oracle["xa"]).max() / oracle["scale"]
    print(f"against the oracle: z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e}")
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5


def _ulp_of_largest(field):
    return float(np.spacing(np.abs(field).max()))


# ---- the update kernel at the C ABI -----------------------------------------------------------------------------------------
class _Grid:
    """A regular grid with both poles and the date line among its cell centres, on the device."""

    def __init__(self, ctx, ny, nx, sig_scale, seed):
        rng = np.random.default_rng(seed)
        self.ny, self.nx, self.n = ny, nx, ny * nx
        lat = np.linspace(-90.0, 90.0, ny)
        lon = -180.0 + 360.0 / nx * np.arange(nx)
        self.lat2, self.lon2 = (a.ravel() for a in np.meshgrid(lat, lon, indexing="ij"))
        self.sig = sig_scale * rng.uniform(0.5, 1.5, self.n)
        self.gxyz = ctx.upload(dense.unit_vectors(self.lat2, self.lon2))
        self.gsig = ctx.upload(self.sig, dtype=np.float64)
        self.glat = ctx.upload(self.lat2, dtype=np.float64)


@pytest.fixture(scope="module")
def solved(ctx, case):
    """z0 (the first solve's: a run that stops at r_0) and z (one correction) of the case, in the device's order, with the
    observations as the device holds them -- a real dz, not noise."""
    plan = _plan(ctx, case, np.float64)
    first = _run(plan, 0, tol=0.9)
    assert first["resid"][1] == first["resid"][0]               # no correction was taken
    final = _run(plan, 0)
    assert final["resid"][1] < first["resid"][0] * 1e-2
    m = plan.m
    assert m % 16 != 0 and m % NB != 0
    oxyz = ctx.download(plan.oxyz.ptr, (3, m), np.float64)
    osig = ctx.download(plan.osig.ptr, (m,), np.float64)
    return dict(plan=plan, m=m, z0=first["z"], z=final["z"], oxyz=oxyz, osig=osig, z0_dev=ctx.upload(first["z"], dtype=np.float64),
                z_dev=ctx.upload(final["z"], dtype=np.float64), sig_scale=float(np.median(np.sqrt(case[0].Sa))))


@pytest.fixture(scope="module", params=[(37, 70), (513, 1025)], ids=["37x70_one_cell_per_thread", "513x1025_two_cells_per_thread"])
def abi(request, ctx, solved):
    """The grid (partial patches in both directions; the larger one is the smallest whose launch takes two cells per thread:
    increment_cells, 512 x 1024 cells), the NumPy float64 delta on a sample of its cells (all of the small grid's), and the
    float64 launch's fields."""
    ny, nx = request.param
    g = _Grid(ctx, ny, nx, solved["sig_scale"], 11)
    rng = np.random.default_rng(5)
    if g.n <= 4000:
        sel = np.arange(g.n)
    else:                                                       # corners, poles, the date line's column, the last partial patch + a sample
        must = np.array([0, nx - 1, g.n - nx, g.n - 1, (ny // 2) * nx, (ny // 2) * nx + nx - 1, 16 * nx + 32, (ny - 1) * nx + nx // 2])
        sel = np.unique(np.concatenate([must, rng.choice(g.n, 3000, replace=False)]))
    pg = orc.unit_vectors(g.lat2[sel], g.lon2[sel])
    w = solved["osig"] * (solved["z"] - solved["z0"])
    po = np.ascontiguousarray(solved["oxyz"].T)
    delta = g.sig[sel] * np.concatenate([orc.gaussian_corr(pg[i:i + 512], po, L_KM) @ w for i in range(0, sel.size, 512)])
    dmax = np.abs(delta).max()
    inc0 = rng.normal(size=g.n) * dmax * 1e4                    # the increment is 1e4 .. 1e5 times what a correction adds to it
    xb = rng.uniform(1.0, 2.0, g.n) * dmax * 1e5
    out = dict(grid=g, sel=sel, delta=delta, dmax=dmax, inc0=inc0, xb=xb, inc0_dev=ctx.upload(inc0, dtype=np.float64))
    out["f64"] = _update(ctx, solved, out, np.float64, inc0, xb)
    return out


def _update(ctx, solved, abi, dt, inc0, xb):
    g, plan = abi["grid"], solved["plan"]
    code = F32 if dt == np.float32 else F64
    item = np.dtype(dt).itemsize
    inc0_dev = abi["inc0_dev"] if inc0 is abi["inc0"] else ctx.upload(inc0, dtype=np.float64)
    xb_dev = ctx.upload(xb, dtype=dt)
    xa_dev, inc_dev = ctx.alloc(g.n * item), ctx.alloc(g.n * item)
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    ctx.check(ctx.lib.oisat_increment_update(ctx.h, code, g.gxyz.ptr, g.gsig.ptr, g.ny, g.nx, plan.oxyz.ptr, plan.osig.ptr,
                                             solved["z_dev"].ptr, solved["z0_dev"].ptr, solved["m"], dense.decay_constant(L_KM),
                                             xb_dev.ptr, xa_dev.ptr, inc_dev.ptr, inc0_dev.ptr, g.glat.ptr, plan.olat.ptr))
    return dict(xa=ctx.download(xa_dev.ptr, (g.n,), dt), inc=ctx.download(inc_dev.ptr, (g.n,), dt), xb=ctx.download(xb_dev.ptr, (g.n,), dt))


def test_update_kernel_float64(abi):
    """inc - inc0 against the NumPy float64 sum over EVERY observation: within 2 e max|delta| (e as measured on the protocol's
    months, a factor 2 of room), on every sampled cell -- poles, date line, partial patches -- and xa = xb + inc with one rounding."""
    r, sel = abi["f64"], abi["sel"]
    got = r["inc"][sel] - abi["inc0"][sel]                      # (exact to 1e-12 of delta: inc0 is 1e4 of it)
    err = np.abs(got - abi["delta"]).max() / abi["dmax"]
    print(f"{abi['grid'].ny} x {abi['grid'].nx}: max|delta_dev - delta_ref| / max|delta_ref| = {err:.3e} (e = {E_MEASURED:.1e})")
    assert np.isfinite(r["inc"]).all() and np.isfinite(r["xa"]).all()
    assert err <= 2.0 * E_MEASURED
    assert np.array_equal(r["xa"], r["xb"] + r["inc"])


def test_update_kernel_float32(ctx, solved, abi):
    """T = float32.  From inc0 = 0 and xb = 0 the field IS delta: the same bound.  With the float64 launch's inc0 and xb: its
    fields rounded ONCE -- float32(inc0 + delta), float32(xb + inc0 + delta) -- bit for bit."""
    sel = abi["sel"]
    zero = np.zeros(abi["grid"].n)
    r0 = _update(ctx, solved, abi, np.float32, zero, zero)
    err = np.abs(r0["inc"][sel].astype(np.float64) - abi["delta"]).max() / abi["dmax"]
    print(f"{abi['grid'].ny} x {abi['grid'].nx}, float32: {err:.3e} of max|delta|")
    assert err <= 2.0 * E_MEASURED
    assert np.array_equal(r0["xa"], r0["inc"])
    r = _update(ctx, solved, abi, np.float32, abi["inc0"], abi["xb"])
    v = abi["f64"]["inc"]                                       # inc0 + delta in double, as the float64 launch stored it
    assert np.array_equal(r["inc"], v.astype(np.float32))
    assert np.array_equal(r["xa"], (r["xb"].astype(np.float64) + v).astype(np.float32))


def test_update_kernel_refuses(ctx, solved, abi):
    g, plan, lib = abi["grid"], solved["plan"], ctx.lib
    out = ctx.alloc(g.n * 8)
    args = [ctx.h, F64, g.gxyz.ptr, g.gsig.ptr, g.ny, g.nx, plan.oxyz.ptr, plan.osig.ptr, solved["z_dev"].ptr, solved["z0_dev"].ptr,
            solved["m"], dense.decay_constant(L_KM), None, None, out.ptr, abi["inc0_dev"].ptr, g.glat.ptr, plan.olat.ptr]
    ctx.check(lib.oisat_set_correlation(ctx.h, 1))              # Gaspari-Cohn: the update is the Gaussian's
    try:
        assert lib.oisat_increment_update(*args) != 0
    finally:
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
    bad = list(args)
    bad[13] = bad[14] = None                                    # neither xa nor inc
    assert lib.oisat_increment_update(*bad) != 0
    bad = list(args)
    bad[15] = None                                              # no inc0
    assert lib.oisat_increment_update(*bad) != 0


# ---- full runs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_converged_at_the_first_residual(ctx, case, dtype):
    """A tolerance the first solve already meets: z = z0, nothing is summed, and the fields are those of
    oisat_apply_increment_grid of z0 (the switch-off run's), bit for bit."""
    plan = _plan(ctx, case, dtype)
    off, on = _run(plan, 0, tol=0.9), _run(plan, 1, tol=0.9)
    assert on["resid"][0] <= 0.9 and on["resid"][1] == on["resid"][0] and on["resid"] == off["resid"]
    assert np.array_equal(on["z"], off["z"])
    assert np.array_equal(on["inc"], off["inc"]) and np.array_equal(on["xa"], off["xa"])
    assert np.abs(on["inc"]).max() > 0


def test_switch_on_against_off(plan32, runs32, oracle, ctx):
    """The same z, byte for byte; the guard lets the update apply (first residual below its threshold); fields within one ulp of
    the field's largest value of the switch-off run's; fields inside the oracle's bars."""
    off, on = runs32["off"], runs32["on"]
    assert on["resid"] == off["resid"] and on["resid"][0] <= T_GUARD and on["resid"][1] <= dense.REFINE_TOL
    assert on["z"].tobytes() == off["z"].tobytes()
    for k in ("xa", "inc"):
        diff = np.abs(on[k].astype(np.float64) - off[k].astype(np.float64))
        print(f"{k}: {int((diff > 0).sum())} of {diff.size} elements differ, the largest by {diff.max() / _ulp_of_largest(off[k]):.3f} ulp of the largest value")
        assert diff.max() <= _ulp_of_largest(off[k])
    _against_oracle(plan32, on, oracle)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_two_corrections(plan32, oracle):
    """tol = 0, refine = 2: every round runs, z - z0 is two corrections' worth.  The same bounds."""
    off, on = _run(plan32, 0, tol=0.0), _run(plan32, 1, tol=0.0)
    assert on["resid"] == off["resid"] and on["resid"][2] < on["resid"][1] < on["resid"][0]
    assert on["z"].tobytes() == off["z"].tobytes()
    for k in ("xa", "inc"):
        assert np.abs(on[k].astype(np.float64) - off[k].astype(np.float64)).max() <= _ulp_of_largest(off[k])
    _against_oracle(plan32, on, oracle)


def test_guard_tripped(ctx, case):
    """A factor coarse enough (a far stretch in bf16 from OISAT_FACTOR_FAR_BITS on) that the first residual is above the guard's
    threshold: the float64 increment of the final z writes the fields -- the switch-off run's bytes."""
    plan = _plan(ctx, case, np.float32)
    for bits in (8, 6, 4, 3, 2):                                # the first (finest) far stretch that trips it
        coarse = dict(OISAT_FACTOR_CUT_BITS=28, OISAT_FACTOR_FAR_BITS=bits, OISAT_FACTOR_MID_BITS=0, OISAT_FACTOR_NEAR_BITS=0)
        off = _run(plan, 0, reload=case, **coarse)
        print(f"far stretch from 2^-{bits}: first residual {off['resid'][0]:.3e} (guard {T_GUARD:.3e})")
        if off["resid"][0] > T_GUARD:
            break
    assert off["resid"][0] > T_GUARD
    on = _run(plan, 1, reload=case, **coarse)
    assert on["resid"] == off["resid"]
    assert on["z"].tobytes() == off["z"].tobytes()
    assert on["xa"].tobytes() == off["xa"].tobytes() and on["inc"].tobytes() == off["inc"].tobytes()
    ctx.solve_status(clear=True)


def test_determinism(ctx, case, plan32, runs32):
    """Two runs on one plan, and two plans that share the handle run back to back without a synchronisation between them (the
    second one's first solve is enqueued while the first one's side launch may still be in flight): the same bits."""
    again = _run(plan32, 1)
    for k in ("z", "xa", "inc"):
        assert again[k].tobytes() == runs32["on"][k].tobytes()
    other = _case(4001)
    a, b = _plan(ctx, case), _plan(ctx, other)
    solo_b = _run(b, 1)
    with _environ(**{SWITCH: 1}):
        a.run(L_KM, refine=2)
        b.run(L_KM, refine=2)
        a.run(L_KM, refine=2)
        xa_a, inc_a = a.download()
        xa_b, inc_b = b.download()
    assert a.last_inc_overlap and b.last_inc_overlap
    assert xa_a.tobytes() == runs32["on"]["xa"].tobytes() and inc_a.tobytes() == runs32["on"]["inc"].tobytes()
    assert xa_b.tobytes() == solo_b["xa"].tobytes() and inc_b.tobytes() == solo_b["inc"].tobytes()


def test_profiling_mode(ctx, plan32, runs32):
    """With profiling on the side launch runs on the handle's stream: the same bits, and both kernels are in the records."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        r = _run(plan32, 1)
        recs = ctx.prof_collect()
    finally:
        ctx.prof_enable(False)
    for k in ("z", "xa", "inc"):
        assert r[k].tobytes() == runs32["on"][k].tobytes()
    assert recs["apply_increment"]["launches"] == 2 and recs["increment_update"]["launches"] == 1      # inc0 and the guarded one
    assert recs["apply_increment"]["total_ms"] > 0 and recs["increment_update"]["total_ms"] > 0
