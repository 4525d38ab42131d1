"""GPU tests of the far stretch of the factor's K-loops (``oisat_factor_far``; csrc/dense_dag.inc: dag_seg_bf16): small
systems with ``OISAT_FACTOR_FAR_BITS`` forced where the default rule keeps the stretch off.  The factor against the NumPy
emulation of the same rule (tests/far_band_emul.py), the switch, both launches, determinism, and the refined analysis
against the float64 oracle.  Measured on MI355X: 3 946 observations, 2^-16: factor to its emulation 9.95e-6, task graph to
recursion 8.97e-6 (x 1.11 of a bar of x 4); 2 551 observations, 2^-27: 2.47e-6 and 1.19e-6 (x 2.08); residuals with the stretch
2.832e-6, 9.60e-11, without 2.838e-6, 9.76e-11; z 8.8e-7, inc 5.3e-8, xa 8.2e-8 from the oracle."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

import far_band_emul as emu

pytestmark = pytest.mark.gpu
NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
FWD = "OISAT_FWD_IN_LAUNCH"
POTRF = "OISAT_POTRF"


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
    c.check(c.lib.oisat_set_task_graph(c.h, -1))


class Case:
    """A swath month in latitude order with its device inputs; ``factor()`` builds S inside the 2^-28 table and factors it."""

    def __init__(self, ctx, nobs, seed, L, far_bits):
        self.ctx, self.L, self.far_bits = ctx, L, far_bits
        self.p = p = syn.point_obs_case(360, 720, nobs, seed, swaths=True)
        o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
        self.lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
        self.lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
        self.m = m = self.lat.size
        self.mp = -(-m // NB) * NB
        self.nb = self.mp // NB
        self.g = dense.decay_constant(L)
        cell = dense.regular_grid_cell(p.lat, p.lon, self.lat, self.lon)
        with _environ(**{CUT: 28, FAR: far_bits}):
            self.env, self.far = emu.tables(self.lat, self.g)
        self.first = self.env[:self.nb]
        self.oxyz = ctx.upload(dense.unit_vectors(self.lat, self.lon))
        self.osig = ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64)
        self.ovar = ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)
        self.env_dev = ctx.upload(self.env)
        self.S = ctx.alloc(self.mp * self.mp * 4)
        self.built = None

    def factor(self, far, **switches):
        """Lower triangle of the factor; far = the table handed to the factorization (None: none)."""
        ctx, lib, m, mp = self.ctx, self.ctx.lib, self.m, self.mp
        with _environ(**switches):
            ctx.check(lib.oisat_memset(ctx.h, self.S.ptr, 0, mp * mp * 4))
            ctx.check(lib.oisat_cov_build_env(ctx.h, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, self.g, self.S.ptr, mp, self.env_dev.ptr))
            if self.built is None:                              # what the launch factors: the emulation's input
                b = ctx.download(self.S.ptr, (mp, mp), np.float32)
                b[m:, :] = 0.0
                b[np.arange(m, mp), np.arange(m, mp)] = 1.0
                self.built = b
            info = C.c_int(-1)
            if far is not None:
                ctx.check(lib.oisat_set_factor_far(ctx.h, far.ctypes.data, far.size))
            ctx.check(lib.oisat_potrf_env(ctx.h, self.S.ptr, m, mp, self.first.ctypes.data, self.env_dev.ptr, C.byref(info)))
            assert info.value == 0
            return np.tril(ctx.download(self.S.ptr, (mp, mp), np.float32))

    def inside(self):
        blk = np.arange(self.nb)[None, :] >= self.first[:, None]
        return np.kron(blk, np.ones((NB, NB), dtype=bool)) & np.tril(np.ones((self.mp, self.mp), dtype=bool))


@pytest.fixture(scope="module")
def main_case(ctx):
    """3 946 swath observations, L = 600 km, stretch at 2^-16: 31 block rows, the last one padded."""
    return Case(ctx, 4000, 4000, 600.0, 16)


@pytest.fixture(scope="module")
def edge_case(ctx):
    """2 551 swath observations, L = 300 km, stretch at 2^-27: at most one far block, none in most rows."""
    return Case(ctx, 2600, 4000, 300.0, 27)


def _check_factor(case):
    """The factor with the stretch against the emulation, with the distance between the two fp32 schedules as the yardstick."""
    inside, low = case.inside(), np.tril(np.ones((case.mp, case.mp), dtype=bool))
    f_far = case.factor(case.far)
    f_off = case.factor(None)
    f_rec = case.factor(None, **{POTRF: "recursive"})
    e_far = emu.factor(case.built, case.first, case.far)
    e_off = emu.factor(case.built, case.first)
    yard = float(np.abs(f_off - f_rec)[inside].max())
    dist = float(np.abs(f_far - e_far)[inside].max())
    print(f"m = {case.m}: far to its emulation {dist:.3e}, task graph to recursion {yard:.3e} (x {dist / yard:.2f}); "
          f"fp32 task graph to the fp32 emulation {float(np.abs(f_off - e_off)[inside].max()):.3e}, "
          f"far to fp32 {float(np.abs(f_far - f_off)[inside].max()):.3e} (emulated: {float(np.abs(e_far - e_off)[inside].max()):.3e})")
    assert np.isfinite(f_far[low]).all()
    assert not np.array_equal(f_far[inside], f_off[inside])     # the stretch did run ...
    assert not f_far[low & ~inside].any()                       # ... and nothing outside the envelope was touched
    assert dist <= 4.0 * yard
    assert tuple(case.ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    return f_far


def test_shape_of_the_main_case(main_case):
    c = main_case
    assert c.nb == 31 and c.m % NB != 0
    assert int((np.arange(c.nb) - c.first).max()) in (8, 9)
    width = c.far - c.first
    assert 2 <= width.max() <= 3
    t = emu.tickets(c.first, c.far)
    kind, k0, kfar = t[:, 0] & 255, (t[:, 0] >> 8) & 1023, t[:, 0] >> 18
    bulk = kind != 0
    kend = np.where(kind[bulk] == 3, t[bulk, 3] - 1, t[bulk, 3])
    assert np.any(kfar[bulk] == k0[bulk]) and np.any(kfar[bulk] == kend) and np.any((kfar[bulk] > k0[bulk]) & (kfar[bulk] < kend))


def test_factor_against_the_emulation(main_case):
    """Max-norm distance of the downloaded factor to the emulation of the same rule: at most 4 x what the two fp32 schedules
    (task graph, recursion) differ by on the same matrix -- summation order, and the bf16 products are summed in a third."""
    f = _check_factor(main_case)
    again = main_case.factor(main_case.far)
    assert np.array_equal(f, again)                             # two runs, the same bits


def test_stretch_boundary_at_both_ends(edge_case):
    """The boundary coincides with k0 (no far block) and with kend (the whole K-loop is far) in the same launch."""
    c = edge_case
    width = c.far - c.first
    assert width.max() == 1 and (width == 0).sum() > c.nb // 2
    t = emu.tickets(c.first, c.far)
    kind, k0, kfar = t[:, 0] & 255, (t[:, 0] >> 8) & 1023, t[:, 0] >> 18
    bulk = kind != 0
    kend = np.where(kind[bulk] == 3, t[bulk, 3] - 1, t[bulk, 3])
    assert np.any((kfar[bulk] == k0[bulk]) & (kend > k0[bulk])) and np.any((kfar[bulk] == kend) & (kend > k0[bulk]))
    _check_factor(c)


def test_off_switch_at_factor_level(main_case):
    """No table, a table equal to first, and the table the library makes under OISAT_FACTOR_FAR_BITS=0: one factor."""
    c = main_case
    with _environ(**{CUT: 28, FAR: 0}):
        far0 = emu.tables(c.lat, c.g)[1]
    assert np.array_equal(far0, c.first)
    a = c.factor(None)
    assert np.array_equal(a, c.factor(c.first.copy()))
    assert np.array_equal(a, c.factor(far0))


def _plan(ctx, p, y, cell):
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    return plan


@pytest.fixture(scope="module")
def analysis(ctx, main_case):
    """``DenseAnalysis.run()`` of the main case under the switches, and the float64 oracle, once for the tests below."""
    p = main_case.p
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = _plan(ctx, p, y, cell)
    L = main_case.L

    def run(**switches):
        with _environ(**switches):
            plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)         # (a plan keeps its tables per (observations, L))
            resid = plan.run(L, refine=2, check_pd=True, want_resid=True)
            xa, inc = plan.download()
            fac = np.tril(ctx.download(plan.S.ptr, (plan.mp, plan.mp), np.float32))
            return dict(resid=resid, xa=xa.astype(np.float64), inc=inc.astype(np.float64), z=plan.download_z(), factor=fac,
                        schedule=plan.last_schedule)

    runs = {
        "far": run(**{CUT: 28, FAR: 16, FWD: None}),
        "far_again": run(**{CUT: 28, FAR: 16, FWD: None}),
        "far_nofwd": run(**{CUT: 28, FAR: 16, FWD: 0}),
        "off": run(**{CUT: 28, FAR: 0, FWD: None}),
        "default": run(**{CUT: None, FAR: None, FWD: None}),
        "default_off": run(**{CUT: None, FAR: 0, FWD: None}),
    }
    import scipy.linalg as sla
    sb = np.sqrt(p.Sa.ravel())
    po = orc.unit_vectors(p.obs_lat, p.obs_lon)
    S = emu.covariance(po, sb[cell], np.ravel(p.obs_var).astype(np.float64), main_case.g, dtype=np.float64)[:y.size, :y.size]
    zr = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    sel = np.random.default_rng(3).choice(p.Xa.size, 4000, replace=False)
    pg = orc.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc_ref = sb[sel] * (orc.gaussian_corr(pg, po, L) @ (sb[cell] * zr))
    return dict(runs=runs, zr=zr, sel=sel, inc_ref=inc_ref, xa_ref=p.Xa.ravel()[sel] + inc_ref, scale=np.abs(p.Xa).max())


def test_same_factor_in_both_launches_and_twice(analysis, main_case):
    """The launch that carries the first forward sweep and the one that does not (OISAT_FWD_IN_LAUNCH=0) are two
    instantiations of the kernel: the same factor bits with the stretch on -- and the same as the factor-level call's."""
    r = analysis["runs"]
    assert r["far"]["schedule"] == dense.SCHEDULE_ENV_DAG_FWD and r["far_nofwd"]["schedule"] == dense.SCHEDULE_ENV_DAG
    assert np.array_equal(r["far"]["factor"], r["far_nofwd"]["factor"])
    assert np.array_equal(r["far"]["factor"], r["far_again"]["factor"])
    assert not np.array_equal(r["far"]["factor"], r["off"]["factor"])
    assert np.array_equal(r["far"]["factor"][main_case.inside()], main_case.factor(main_case.far)[main_case.inside()])
    for k in ("xa", "inc", "z"):
        assert np.array_equal(r["far"][k], r["far_again"][k]) and np.array_equal(r["far"][k], r["far_nofwd"][k])


def test_off_switch_is_the_default_at_this_size(analysis):
    """Chain-bound: the default rule has no stretch, and OISAT_FACTOR_FAR_BITS=0 changes nothing, bit for bit."""
    a, b = analysis["runs"]["default"], analysis["runs"]["default_off"]
    assert a["resid"] == b["resid"]
    for k in ("xa", "inc", "z", "factor"):
        assert np.array_equal(a[k], b[k])


def test_analysis_with_the_stretch(analysis):
    """First residual at most 1.05 x the run without the stretch, one correction; z, inc and xa inside the bars of
    test_forced_narrow_analysis_against_oracle (2e-5, 1e-5, 1e-5)."""
    far, off = analysis["runs"]["far"], analysis["runs"]["off"]
    zr, sel, scale = analysis["zr"], analysis["sel"], analysis["scale"]
    ez = np.abs(far["z"] - zr).max() / np.abs(zr).max()
    ei = np.abs(far["inc"].ravel()[sel] - analysis["inc_ref"]).max() / scale
    ex = np.abs(far["xa"].ravel()[sel] - analysis["xa_ref"]).max() / scale
    print(f"residuals with the stretch {far['resid']}, without {off['resid']}; z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e} against the oracle")
    assert far["resid"][0] <= 1.05 * off["resid"][0]
    assert far["resid"][1] <= dense.REFINE_TOL and far["resid"][2] == far["resid"][1]      # one correction, then skipped rounds
    assert off["resid"][1] <= dense.REFINE_TOL
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5
