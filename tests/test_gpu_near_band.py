"""GPU tests of the near stretch of the factor's K-loops (``oisat_factor_near``; csrc/dense_dag.inc: dag_seg_bf16x3): small
systems with ``OISAT_FACTOR_FAR_BITS`` / ``OISAT_FACTOR_MID_BITS`` / ``OISAT_FACTOR_NEAR_BITS`` forced where the default rule keeps
all three stretches off.  The factor against the NumPy emulation of the same rule (tests/near_band_emul.py) and against
emulations that lose a term, the switches, both launches, determinism, and the refined analysis against the float64 oracle."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

import near_band_emul as emu

pytestmark = pytest.mark.gpu
NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
MID = "OISAT_FACTOR_MID_BITS"
NEAR = "OISAT_FACTOR_NEAR_BITS"
FWD = "OISAT_FWD_IN_LAUNCH"
POTRF = "OISAT_POTRF"
VARIANTS = ("hi_lo", "lo_hi", "mid_mid")


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
    c.check(c.lib.oisat_set_factor_near(c.h, None, 0))


class Case:
    """A swath month in latitude order with its device inputs; ``factor()`` builds S inside the 2^-28 table and factors it."""

    def __init__(self, ctx, nobs, seed, L, far_bits, mid_bits, near_bits):
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
        self.switches = {CUT: 28, FAR: far_bits, MID: mid_bits, NEAR: near_bits}
        with _environ(**self.switches):
            self.env, self.far, self.mid, self.near = emu.tables(self.lat, self.g)
        self.first = self.env[:self.nb]
        self.oxyz = ctx.upload(dense.unit_vectors(self.lat, self.lon))
        self.osig = ctx.upload(np.sqrt(p.Sa.ravel())[cell], dtype=np.float64)
        self.ovar = ctx.upload(np.ravel(p.obs_var)[o], dtype=np.float64)
        self.env_dev = ctx.upload(self.env)
        self.S = ctx.alloc(self.mp * self.mp * 4)
        self.built = None

    def factor(self, far, mid, near, entry="potrf_env", **switches):
        """Lower triangle of the factor; far / mid / near = the tables handed to the factorization (None: none)."""
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
            for setter, table in ((lib.oisat_set_factor_far, far), (lib.oisat_set_factor_mid, mid), (lib.oisat_set_factor_near, near)):
                if table is not None:
                    ctx.check(setter(ctx.h, table.ctypes.data, table.size))
            if entry == "potrf_env":
                ctx.check(lib.oisat_potrf_env(ctx.h, self.S.ptr, m, mp, self.first.ctypes.data, self.env_dev.ptr, C.byref(info)))
            else:                                               # the launch that carries the first forward sweep
                d = ctx.upload(np.linspace(-1.0, 1.0, m), dtype=np.float64)
                sched = C.c_int(0)
                ctx.check(lib.oisat_potrf_env_fwd(ctx.h, self.S.ptr, m, mp, self.first.ctypes.data, self.env_dev.ptr, d.ptr, C.byref(info),
                                                  C.byref(sched)))
                assert sched.value == (dense.SCHEDULE_ENV_DAG if str(switches.get(FWD)) == "0" else dense.SCHEDULE_ENV_DAG_FWD)
            assert info.value == 0
            return np.tril(ctx.download(self.S.ptr, (mp, mp), np.float32))

    def inside(self):
        blk = np.arange(self.nb)[None, :] >= self.first[:, None]
        return np.kron(blk, np.ones((NB, NB), dtype=bool)) & np.tril(np.ones((self.mp, self.mp), dtype=bool))

    def ranges(self):
        """far, middle, near, fp32 K-blocks per bulk task"""
        r = emu.task_ranges(self.first, self.far, self.mid, self.near)
        return r[:, 4] - r[:, 3], r[:, 5] - r[:, 4], r[:, 6] - r[:, 5], np.maximum(r[:, 7] - r[:, 6], 0)


@pytest.fixture(scope="module")
def main_case(ctx):
    """3 946 swath observations, L = 600 km, far at 2^-16, middle at 2^-8, near `all`: 31 block rows, the last one padded."""
    return Case(ctx, 4000, 4000, 600.0, 16, 8, "all")


@pytest.fixture(scope="module")
def only_case(ctx):
    """The main case without a far and without a middle stretch: the whole K-loop of every bulk task is the near segment."""
    return Case(ctx, 4000, 4000, 600.0, 0, 0, "all")


@pytest.fixture(scope="module")
def edge_case(ctx):
    """2 551 swath observations, L = 300 km, far at 2^-27, middle at 2^-26, near at 2^-23 (chosen on the host from the tables of
    23 .. 27 bits: the widest stretch that still has at most one block per row): at most one near block per row."""
    return Case(ctx, 2600, 4000, 300.0, 27, 26, 23)


def _check_factor(case):
    """The factor with the near stretch against its emulation: at most 2 x the yardstick.  The yardstick is measured here, on the
    code paths the stretch does not touch: the fp32 task graph against the recursion, and the factor without the near stretch
    (far and middle as the case has them) against ITS emulation; the larger of the two.
    And the factor tells a lost product: it is at least twice as close to the full emulation as to each emulation with one of
    the three small terms left out -- wherever that emulation is a second reference at all, i.e. lies more than 2 x the yardstick
    from the full one.  Measured on the host while writing this (the emulations against each other, largest entry inside the
    envelope; the yardstick of the main case is 1.0e-5 in tests/test_gpu_mid_band.py; the kernel's eight products, one of the six
    larger ones left out): main case hi_lo 4.2e-5, lo_hi 2.6e-5, mid_mid 1.6e-4 on the host's build of S (on the device's:
    3.6e-5, 2.7e-5, 1.6e-4); near-only case 3.5e-5, 2.9e-5, 1.6e-4 on the device's build.  On the edge case (single blocks of
    correlations below 2^-23) the variants are 1e-12 .. 7e-12 from the full emulation: none is a second reference, none is
    asserted.  Returns (the factor, how many variants were second references)."""
    inside, low = case.inside(), np.tril(np.ones((case.mp, case.mp), dtype=bool))
    f_near = case.factor(case.far, case.mid, case.near)
    f_mid = case.factor(case.far, case.mid, None)
    f_off = case.factor(None, None, None)
    f_rec = case.factor(None, None, None, **{POTRF: "recursive"})
    e_near = emu.factor(case.built, case.first, case.far, case.mid, case.near)
    e_mid = emu.factor(case.built, case.first, case.far, case.mid)

    def d(a, b):
        return float(np.abs(a - b)[inside].max())

    y_mid, y_rec = d(f_mid, e_mid), d(f_off, f_rec)
    yard = max(y_mid, y_rec)
    dist = d(f_near, e_near)
    print(f"m = {case.m}: near to its emulation {dist:.3e} (x {dist / yard:.2f} of the yardstick); without the stretch to its emulation "
          f"{y_mid:.3e}, task graph to recursion {y_rec:.3e}; near to without {d(f_near, f_mid):.3e} (emulated: {d(e_near, e_mid):.3e})")
    assert np.isfinite(f_near[low]).all()
    assert not np.array_equal(f_near[inside], f_mid[inside])    # the stretch did run ...
    assert not f_near[low & ~inside].any()                      # ... and nothing outside the envelope was touched
    assert dist <= 2.0 * yard
    second = 0
    for v in VARIANTS:
        e_v = emu.factor(case.built, case.first, case.far, case.mid, case.near, variant=v)
        apart, dist_v = d(e_near, e_v), d(f_near, e_v)
        print(f"    {v} left out: {apart:.3e} from the full emulation (x {apart / yard:.2f} of the yardstick), the factor {dist_v:.3e} from it")
        if apart > 2.0 * yard:
            second += 1
            assert 2.0 * dist <= dist_v, v
    assert tuple(case.ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    return f_near, second


def test_shape_of_the_cases(main_case, only_case, edge_case):
    """Every combination of dag_tile_task's four ranges occurs in the main case (asserted from the host tables); the near-only
    case runs nothing else; the edge case has single near blocks."""
    c = main_case
    assert c.nb == 31 and c.m == 3946
    nf, nm, nn, n32 = c.ranges()
    assert not n32.any()                                        # near = all: nothing is left for the fp32 segment of a bulk task
    combos = {(bool(a), bool(b), bool(e)) for a, b, e in zip(nf > 0, nm > 0, nn > 0)}
    print("main case: (far, middle, near) combinations among the bulk tasks:", sorted(combos), "; single near blocks:", int((nn == 1).sum()))
    # all eight but one: far and near blocks without a middle one between them would take a row whose middle stretch is empty
    # behind a far one, which these tables do not have (the edge case has the fp32 segment behind a near one)
    assert combos == {(f, m, n) for f in (False, True) for m in (False, True) for n in (False, True)} - {(True, False, True)}
    assert (nn == 1).any() and (nn > 1).any()
    assert np.all(c.mid <= c.near) and np.array_equal(c.near, np.arange(c.nb))
    o = only_case
    of, om, on, o32 = o.ranges()
    assert np.array_equal(o.far, o.first) and np.array_equal(o.mid, o.first) and np.array_equal(o.near, np.arange(o.nb))
    assert not of.any() and not om.any() and not o32.any() and on.any()
    e = edge_case
    width = e.near - e.mid
    assert width.max() == 1 and (width == 1).sum() >= 3
    ef, em, en, e32 = e.ranges()
    assert en.max() == 1 and e32.any()                          # ... and the fp32 segment follows the near one in the same task


def test_factor_against_the_emulation(main_case):
    f, second = _check_factor(main_case)
    assert second == 3                                          # every lost term would have shown
    assert np.array_equal(f, main_case.factor(main_case.far, main_case.mid, main_case.near))      # two runs, the same bits


def test_near_only(only_case):
    f, second = _check_factor(only_case)
    assert second >= 2                                          # (lo_hi is the closest of the three: 2.9 x the yardstick)
    assert np.array_equal(f, only_case.factor(None, None, only_case.near))


def test_single_near_blocks(edge_case):
    _check_factor(edge_case)


def test_off_switches_at_factor_level(main_case):
    """No near table, a table equal to mid, and the table the library makes under OISAT_FACTOR_NEAR_BITS=0: the factor without
    the stretch, bit for bit; a table that does not fit the middle table is refused and consumed."""
    c = main_case
    with _environ(**dict(c.switches, **{NEAR: 0})):
        near0 = emu.tables(c.lat, c.g)[3]
    assert np.array_equal(near0, c.mid)
    a = c.factor(c.far, c.mid, None)
    assert np.array_equal(a, c.factor(c.far, c.mid, c.mid.copy()))
    assert np.array_equal(a, c.factor(c.far, c.mid, near0))
    assert not np.array_equal(a, c.factor(c.far, c.mid, c.near))
    lib, h = c.ctx.lib, c.ctx.h
    for bad in (c.first, np.arange(c.nb, dtype=np.int32) + 1, c.near[:-1].copy()):     # below mid in some row | above i | wrong length
        c.ctx.check(lib.oisat_set_factor_far(h, c.far.ctypes.data, c.far.size))
        c.ctx.check(lib.oisat_set_factor_mid(h, c.mid.ctypes.data, c.mid.size))
        c.ctx.check(lib.oisat_set_factor_near(h, bad.ctypes.data, bad.size))
        assert lib.oisat_potrf_env(h, c.S.ptr, c.m, c.mp, c.first.ctypes.data, c.env_dev.ptr, None) != 0
    assert np.any(c.first < c.mid)
    assert np.array_equal(a, c.factor(c.far, c.mid, None))      # ... and all three tables were consumed by the refused call


def test_both_launches_agree(main_case, only_case):
    """oisat_potrf_env and oisat_potrf_env_fwd are two instantiations of the kernel: the same factor bits with the stretch on."""
    for c in (main_case, only_case):
        a = c.factor(c.far, c.mid, c.near)
        b = c.factor(c.far, c.mid, c.near, entry="potrf_env_fwd")
        assert np.array_equal(a[c.inside()], b[c.inside()])
        assert np.array_equal(a[c.inside()], c.factor(c.far, c.mid, c.near, entry="potrf_env_fwd", **{FWD: 0})[c.inside()])


def test_the_launch_that_also_solves_ignores_it(ctx, main_case):
    """oisat_batch_analyse factors in the kernel's third instantiation, which has no stretches: with a near table pending on the
    handle and OISAT_FACTOR_NEAR_BITS=all in the environment its results are those without, bit for bit -- and the pending table
    is still the next enveloped factorization's."""
    import batch_cases as bc
    from test_gpu_batch_abi import assert_same_results, batch
    c = main_case
    with batch(ctx, bc.two_cells(), 300.0, "gaussian", "f32") as bt:
        with _environ(**{NEAR: 0}):
            plain, st0 = bt.run(2, how="analyse")
        ctx.check(ctx.lib.oisat_set_factor_near(ctx.h, c.near.ctypes.data, c.near.size))
        with _environ(**{NEAR: "all"}):
            with_table, st1 = bt.run(2, how="analyse")
        assert bt.is_task_graph() == 1
    assert st0.clean and st1.clean
    assert_same_results(plain, with_table, "oisat_batch_analyse with a near table pending")
    ctx.check(ctx.lib.oisat_set_factor_far(ctx.h, c.far.ctypes.data, c.far.size))
    ctx.check(ctx.lib.oisat_set_factor_mid(ctx.h, c.mid.ctypes.data, c.mid.size))
    assert np.array_equal(c.factor(None, None, None), c.factor(c.far, c.mid, c.near))         # (the first call consumed the pending three)


def _plan(ctx, p, y, cell):
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    return plan


@pytest.fixture(scope="module")
def analysis(ctx, main_case):
    """``DenseAnalysis.run()`` of the main case with and without the near stretch, and the float64 oracle, once."""
    p, L = main_case.p, main_case.L
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
                        schedule=plan.last_schedule, near=plan._near_host.copy(), mid=plan._mid_host.copy())

    on = dict(main_case.switches, **{FWD: None})
    runs = {"near": run(**on), "near_nofwd": run(**dict(on, **{FWD: 0})), "off": run(**dict(on, **{NEAR: 0}))}
    import scipy.linalg as sla
    sb = np.sqrt(p.Sa.ravel())
    po = orc.unit_vectors(p.obs_lat, p.obs_lon)
    S = emu.covariance(po, sb[cell], np.ravel(p.obs_var).astype(np.float64), main_case.g, dtype=np.float64)[:y.size, :y.size]
    zr = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    sel = np.random.default_rng(3).choice(p.Xa.size, 4000, replace=False)
    pg = orc.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc_ref = sb[sel] * (orc.gaussian_corr(pg, po, L) @ (sb[cell] * zr))
    return dict(runs=runs, zr=zr, sel=sel, inc_ref=inc_ref, xa_ref=p.Xa.ravel()[sel] + inc_ref, scale=np.abs(p.Xa).max())


def test_analysis_with_the_stretch(analysis, ctx, main_case):
    """Through DenseAnalysis: the plan makes and hands over the near table; both launches give the factor-level call's bits;
    first residual at most 1.05 x the run without the near stretch, one correction; z, inc and xa against the float64 oracle
    inside the bars tests/test_gpu_mid_band.py uses for the same case (2e-5, 1e-5, 1e-5)."""
    r = analysis["runs"]
    near, off = r["near"], r["off"]
    assert near["schedule"] == dense.SCHEDULE_ENV_DAG_FWD and r["near_nofwd"]["schedule"] == dense.SCHEDULE_ENV_DAG
    assert np.array_equal(near["near"], main_case.near) and np.array_equal(off["near"], off["mid"])
    assert np.array_equal(near["factor"], r["near_nofwd"]["factor"])
    assert not np.array_equal(near["factor"], off["factor"])
    ins = main_case.inside()
    assert np.array_equal(near["factor"][ins], main_case.factor(main_case.far, main_case.mid, main_case.near)[ins])
    assert np.array_equal(off["factor"][ins], main_case.factor(main_case.far, main_case.mid, None)[ins])
    for k in ("xa", "inc", "z"):
        assert np.array_equal(near[k], r["near_nofwd"][k])
    zr, sel, scale = analysis["zr"], analysis["sel"], analysis["scale"]
    ez = np.abs(near["z"] - zr).max() / np.abs(zr).max()
    ei = np.abs(near["inc"].ravel()[sel] - analysis["inc_ref"]).max() / scale
    ex = np.abs(near["xa"].ravel()[sel] - analysis["xa_ref"]).max() / scale
    print(f"residuals with the near stretch {near['resid']}, without {off['resid']}; z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e} against the oracle")
    assert near["resid"][0] <= 1.05 * off["resid"][0]
    assert near["resid"][1] <= dense.REFINE_TOL and near["resid"][2] == near["resid"][1]      # one correction, then skipped rounds
    assert off["resid"][1] <= dense.REFINE_TOL
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
