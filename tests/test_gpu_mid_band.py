"""GPU tests of the middle stretch of the factor's K-loops (``oisat_factor_mid``; csrc/dense_dag.inc: dag_seg_bf16x2): small
systems with ``OISAT_FACTOR_FAR_BITS`` / ``OISAT_FACTOR_MID_BITS`` forced where the default rule keeps both stretches off.
The factor against the NumPy emulation of the same rule (tests/mid_band_emul.py), the switches, both launches, determinism,
and the refined analysis against the float64 oracle."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

import mid_band_emul as emu

pytestmark = pytest.mark.gpu
NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
MID = "OISAT_FACTOR_MID_BITS"
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

    def __init__(self, ctx, nobs, seed, L, far_bits, mid_bits):
        self.ctx, self.L = ctx, L
        self.p = p = syn.point_obs_case(360, 720, nobs, seed, swaths=True)
        o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
        self.lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
        self.lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
        self.m = m = self.lat.size
        self.mp = -(-m // NB) * NB
        self.nb = self.mp // NB
        self.g = dense.decay_constant(L)
        cell = dense.regular_grid_cell(p.lat, p.lon, self.lat, self.lon)
        with _environ(**{CUT: 28, FAR: far_bits, MID: mid_bits}):
            self.env, self.far, self.mid = emu.tables(self.lat, self.g)
        self.first = self.env[:self.nb]
        self.oxyz = ctx.upload(dense.unit_vectors(self.lat, self.lon))
        self.osig = ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64)
        self.ovar = ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)
        self.env_dev = ctx.upload(self.env)
        self.S = ctx.alloc(self.mp * self.mp * 4)
        self.built = None
        self.cache = {}

    def factor(self, far, mid, **switches):
        """Lower triangle of the factor; far / mid = the tables handed to the factorization (None: none)."""
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
            if mid is not None:
                ctx.check(lib.oisat_set_factor_mid(ctx.h, mid.ctypes.data, mid.size))
            ctx.check(lib.oisat_potrf_env(ctx.h, self.S.ptr, m, mp, self.first.ctypes.data, self.env_dev.ptr, C.byref(info)))
            assert info.value == 0
            return np.tril(ctx.download(self.S.ptr, (mp, mp), np.float32))

    def inside(self):
        blk = np.arange(self.nb)[None, :] >= self.first[:, None]
        return np.kron(blk, np.ones((NB, NB), dtype=bool)) & np.tril(np.ones((self.mp, self.mp), dtype=bool))

    def ranges(self):
        r = emu.task_ranges(self.first, self.far, self.mid)
        return r[:, 4] - r[:, 3], r[:, 5] - r[:, 4], np.maximum(r[:, 6] - r[:, 5], 0)      # far, middle, fp32 K-blocks per bulk task


@pytest.fixture(scope="module")
def main_case(ctx):
    """3 946 swath observations, L = 600 km, far at 2^-16, middle at 2^-8: 31 block rows, the last one padded."""
    return Case(ctx, 4000, 4000, 600.0, 16, 8)


@pytest.fixture(scope="module")
def edge_case(ctx):
    """2 551 swath observations, L = 300 km, far at 2^-27, middle at 2^-26: at most one middle block per row."""
    return Case(ctx, 2600, 4000, 300.0, 27, 26)


@pytest.fixture(scope="module")
def nofar_case(ctx):
    """The main case without a far stretch: the middle one starts at first[i]."""
    return Case(ctx, 4000, 4000, 600.0, 0, 8)


def _check_factor(case, discriminates):
    """The factor with the middle stretch against its emulation.  Yardstick, by the parent's code path: the far-only factor
    against the far-only emulation, and the fp32 task graph against the recursion; the bar is 2 x the larger.  Why 2: on the main
    case an emulation with the a_lo b_hi^T term left out lies 2.6e-5 from the full one, with the a_hi b_lo^T term left out
    5.4e-5, with both 5.4e-5, so a kernel that loses a term is at least 2.6 x the yardstick; accumulation order alone, as in
    the far stretch, stays near 1 x (measured: 9.95e-6, x 1.00).  And the factor is at least twice as close to the split emulation as to the
    single-bf16 emulation of the same stretch -- wherever those two emulations are two references at all, that is more than
    2 x the yardstick apart (discriminates = True: the case is expected to be such a one, and is checked to be).  Where the
    stretch holds single blocks of correlations below 2^-26 (the edge case) the two emulations are 1e-11 apart, far below the
    fp32 rounding of the tiles themselves, and no factor can be twice as close to one as to the other."""
    inside, low = case.inside(), np.tril(np.ones((case.mp, case.mp), dtype=bool))
    f_mid = case.factor(case.far, case.mid)
    f_far = case.factor(case.far, None)
    f_off = case.factor(None, None)
    f_rec = case.factor(None, None, **{POTRF: "recursive"})
    e_mid = emu.factor(case.built, case.first, case.far, case.mid)
    e_single = emu.factor(case.built, case.first, case.far, case.mid, middle="single")
    e_far = emu.factor(case.built, case.first, case.far)

    def d(a, b):
        return float(np.abs(a - b)[inside].max())

    y_far, y_rec = d(f_far, e_far), d(f_off, f_rec)
    yard = max(y_far, y_rec)
    dist, dist_single = d(f_mid, e_mid), d(f_mid, e_single)
    print(f"m = {case.m}: middle to its emulation {dist:.3e} (x {dist / yard:.2f} of the yardstick), to the single-bf16 emulation "
          f"{dist_single:.3e}; far-only to its emulation {y_far:.3e}, task graph to recursion {y_rec:.3e}; middle to far-only "
          f"{d(f_mid, f_far):.3e} (emulated: {d(e_mid, e_far):.3e}); a_lo b_hi^T dropped {d(e_mid, emu.factor(case.built, case.first, case.far, case.mid, middle='hi_lo')):.3e}, "
          f"a_hi b_lo^T dropped {d(e_mid, emu.factor(case.built, case.first, case.far, case.mid, middle='lo_hi')):.3e}, "
          f"both {d(e_mid, emu.factor(case.built, case.first, case.far, case.mid, middle='hi_only')):.3e} from the full emulation")
    assert np.isfinite(f_mid[low]).all()
    assert not np.array_equal(f_mid[inside], f_far[inside])     # the stretch did run ...
    assert not f_mid[low & ~inside].any()                       # ... and nothing outside the envelope was touched
    assert dist <= 2.0 * yard
    two_references = d(e_mid, e_single) > 2.0 * yard
    assert two_references == discriminates
    if two_references:
        assert 2.0 * dist <= dist_single
    assert tuple(case.ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    return f_mid


def test_shape_of_the_cases(main_case, edge_case, nofar_case):
    """Every path of dag_tile_task's three ranges occurs in the main case; the edge case has single middle blocks; without a
    far table kfar = k0 everywhere."""
    c = main_case
    assert c.nb == 31 and c.m % NB != 0
    nf, nm, n32 = c.ranges()
    counts = (int(((nf > 0) & (nm > 0) & (n32 > 0)).sum()), int(((nm > 0) & (nf == 0)).sum()), int((nm == 0).sum()), int((nm == 1).sum()))
    print("main case: bulk tasks with all three kinds of block, with a middle stretch and no far one, without a middle block, with exactly one:", counts)
    assert all(n > 0 for n in counts)
    assert np.all(c.far <= c.mid) and np.all(c.mid <= np.arange(c.nb))
    e = edge_case
    width = e.mid - e.far
    assert width.max() == 1 and (width == 0).sum() > e.nb // 2
    n = nofar_case
    assert np.array_equal(n.far, n.first) and np.any(n.mid > n.far)
    assert not n.ranges()[0].any() and n.ranges()[1].any()


def test_factor_against_the_emulation(main_case):
    f = _check_factor(main_case, True)
    again = main_case.factor(main_case.far, main_case.mid)
    assert np.array_equal(f, again)                             # two runs, the same bits


def test_single_middle_blocks(edge_case):
    _check_factor(edge_case, False)


def test_middle_without_far(nofar_case):
    _check_factor(nofar_case, True)


def test_off_switches_at_factor_level(main_case):
    """No middle table, a table equal to far, and the table the library makes under OISAT_FACTOR_MID_BITS=0: the far-only factor,
    bit for bit; a table that does not fit its far table is refused."""
    c = main_case
    with _environ(**{CUT: 28, FAR: 16, MID: 0}):
        mid0 = emu.tables(c.lat, c.g)[2]
    assert np.array_equal(mid0, c.far)
    a = c.factor(c.far, None)
    assert np.array_equal(a, c.factor(c.far, c.far.copy()))
    assert np.array_equal(a, c.factor(c.far, mid0))
    assert not np.array_equal(a, c.factor(c.far, c.mid))
    lib, h = c.ctx.lib, c.ctx.h
    c.ctx.check(lib.oisat_set_factor_far(h, c.far.ctypes.data, c.far.size))
    c.ctx.check(lib.oisat_set_factor_mid(h, c.first.ctypes.data, c.first.size))        # below far in some row
    assert np.any(c.first < c.far)
    assert lib.oisat_potrf_env(h, c.S.ptr, c.m, c.mp, c.first.ctypes.data, c.env_dev.ptr, None) != 0
    assert np.array_equal(a, c.factor(c.far, None))             # ... and both tables were consumed by the refused call


def _plan(ctx, p, y, cell):
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    return plan


def _runner(ctx, p, L):
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    plan = _plan(ctx, p, y, cell)

    def run(**switches):
        with _environ(**switches):
            plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)         # (a plan keeps its tables per (observations, L))
            resid = plan.run(L, refine=2, check_pd=True, want_resid=True)
            xa, inc = plan.download()
            fac = np.tril(ctx.download(plan.S.ptr, (plan.mp, plan.mp), np.float32))
            return dict(resid=resid, xa=xa.astype(np.float64), inc=inc.astype(np.float64), z=plan.download_z(), factor=fac,
                        schedule=plan.last_schedule, mid=plan._mid_host.copy(), far=plan._far_host.copy())

    return run, cell, y


@pytest.fixture(scope="module")
def analysis(ctx, main_case):
    """``DenseAnalysis.run()`` of the main case under the switches, and the float64 oracle, once for the tests below."""
    p, L = main_case.p, main_case.L
    run, cell, y = _runner(ctx, p, L)
    runs = {
        "mid": run(**{CUT: 28, FAR: 16, MID: 8, FWD: None}),
        "mid_again": run(**{CUT: 28, FAR: 16, MID: 8, FWD: None}),
        "mid_nofwd": run(**{CUT: 28, FAR: 16, MID: 8, FWD: 0}),
        "far": run(**{CUT: 28, FAR: 16, MID: 0, FWD: None}),
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
    instantiations of the kernel: the same factor bits with the stretch on -- and the same as the factor-level call's; the
    carried forward sweep gives the z, increment and analysis of the separate one."""
    r = analysis["runs"]
    assert r["mid"]["schedule"] == dense.SCHEDULE_ENV_DAG_FWD and r["mid_nofwd"]["schedule"] == dense.SCHEDULE_ENV_DAG
    assert np.array_equal(r["mid"]["mid"], main_case.mid) and np.array_equal(r["mid"]["far"], main_case.far)
    assert np.array_equal(r["far"]["mid"], r["far"]["far"])
    assert np.array_equal(r["mid"]["factor"], r["mid_nofwd"]["factor"])
    assert np.array_equal(r["mid"]["factor"], r["mid_again"]["factor"])
    assert not np.array_equal(r["mid"]["factor"], r["far"]["factor"])
    assert np.array_equal(r["mid"]["factor"][main_case.inside()], main_case.factor(main_case.far, main_case.mid)[main_case.inside()])
    for k in ("xa", "inc", "z"):
        assert np.array_equal(r["mid"][k], r["mid_again"][k]) and np.array_equal(r["mid"][k], r["mid_nofwd"][k])


def test_analysis_with_the_stretch(analysis, ctx):
    """First residual at most 1.05 x the run without the middle stretch, one correction; z, inc and xa inside the bars
    tests/test_gpu_far_band.py uses for the same case (2e-5, 1e-5, 1e-5)."""
    mid, far = analysis["runs"]["mid"], analysis["runs"]["far"]
    zr, sel, scale = analysis["zr"], analysis["sel"], analysis["scale"]
    ez = np.abs(mid["z"] - zr).max() / np.abs(zr).max()
    ei = np.abs(mid["inc"].ravel()[sel] - analysis["inc_ref"]).max() / scale
    ex = np.abs(mid["xa"].ravel()[sel] - analysis["xa_ref"]).max() / scale
    print(f"residuals with the middle stretch {mid['resid']}, without {far['resid']}; z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e} against the oracle")
    assert mid["resid"][0] <= 1.05 * far["resid"][0]
    assert mid["resid"][1] <= dense.REFINE_TOL and mid["resid"][2] == mid["resid"][1]      # one correction, then skipped rounds
    assert far["resid"][1] <= dense.REFINE_TOL
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_chain_bound_config_2_has_no_stretch(ctx):
    """Config 2 (10 000 scattered observations, L = 500 km) is chain-bound: the default rule gives no middle stretch, and
    OISAT_FACTOR_MID_BITS=0 changes nothing, bit for bit."""
    p = syn.point_obs_case(360, 720, 10000, 4000)
    run, _, _ = _runner(ctx, p, 500.0)
    a = run(**{CUT: None, FAR: None, MID: None, FWD: None})
    b = run(**{CUT: None, FAR: None, MID: 0, FWD: None})
    assert np.array_equal(a["mid"], a["far"]) and np.array_equal(b["mid"], b["far"])
    assert a["resid"] == b["resid"]
    for k in ("xa", "inc", "z", "factor"):
        assert np.array_equal(a[k], b[k])
