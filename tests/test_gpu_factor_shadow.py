"""GPU tests of the factor's shadow (csrc/dense_dag.inc "Shadow"): the bf16 images of every final tile, stored once by the task
that makes the tile final and read by the far and middle stretches instead of converting in every K-loop.  The factor must
not change by a bit: everything here is ``np.array_equal`` against ``OISAT_FACTOR_SHADOW=0``, on the shapes of
tests/test_gpu_mid_band.py (the smallest at which far, middle and fp32 K-blocks all occur)."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import dense

from test_gpu_mid_band import CUT, FAR, FWD, MID, NB, Case, _environ, _runner, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
SHADOW = "OISAT_FACTOR_SHADOW"
MODES = (None, "far", "mid")                                    # both stretches read the shadow | only one of them


@pytest.fixture(scope="module")
def cases(ctx):
    """3 946 observations, L = 600 km, far 2^-16, middle 2^-8 (31 block rows, the last one padded; tasks with a middle stretch and
    no far one, tasks with exactly one middle block) | 2 551 observations, L = 300 km, far 2^-27, middle 2^-26 (single far and
    middle blocks) | the first with the far stretch off."""
    out = {"main": Case(ctx, 4000, 4000, 600.0, 16, 8), "edge": Case(ctx, 2600, 4000, 300.0, 27, 26), "nofar": Case(ctx, 4000, 4000, 600.0, 0, 8)}
    rng = np.random.default_rng(11)
    for c in out.values():
        c.d = ctx.upload(rng.standard_normal(c.m), dtype=np.float64)
        c.z = ctx.alloc(c.m * 8)
        c.olat = ctx.upload(c.lat, dtype=np.float64)
    return out


def _factor_fwd(case, **switches):
    """The factor through oisat_potrf_env_fwd, and what its carried forward sweep leads to: z of the gain solve without
    refinement, which takes the launch's forward vector and runs the backward sweep alone -- with an identical factor, z is
    identical exactly when the forward vector is."""
    ctx, lib, m, mp = case.ctx, case.ctx.lib, case.m, case.mp
    with _environ(**switches):
        ctx.check(lib.oisat_memset(ctx.h, case.S.ptr, 0, mp * mp * 4))
        ctx.check(lib.oisat_cov_build_env(ctx.h, case.oxyz.ptr, case.osig.ptr, case.ovar.ptr, m, case.g, case.S.ptr, mp, case.env_dev.ptr))
        ctx.check(lib.oisat_set_factor_far(ctx.h, case.far.ctypes.data, case.far.size))
        ctx.check(lib.oisat_set_factor_mid(ctx.h, case.mid.ctypes.data, case.mid.size))
        info, schedule = C.c_int(-1), C.c_int(-1)
        ctx.check(lib.oisat_potrf_env_fwd(ctx.h, case.S.ptr, m, mp, case.first.ctypes.data, case.env_dev.ptr, case.d.ptr, C.byref(info), C.byref(schedule)))
        assert info.value == 0 and schedule.value == dense.SCHEDULE_ENV_DAG_FWD
        ctx.check(lib.oisat_set_obs_blocks(ctx.h, None, 0))     # per solve: handles are shared
        ctx.check(lib.oisat_gain_solve(ctx.h, case.S.ptr, case.oxyz.ptr, case.osig.ptr, case.ovar.ptr, m, mp, case.g, case.d.ptr, 0, case.z.ptr,
                                       None, case.olat.ptr))
        return np.tril(ctx.download(case.S.ptr, (mp, mp), np.float32)), ctx.download(case.z.ptr, (m,), np.float64)


def _has_shadow(case):
    """Did the last factorization on the handle fill a shadow?  (Its sub-diagonal tile (1, 0) can then be read back.)"""
    buf = np.empty((2, NB, NB), dtype=np.uint16)
    return case.ctx.lib.oisat_factor_shadow_tile(case.ctx.h, 1, 0, buf[0].ctypes.data, buf[1].ctypes.data) == 0


@pytest.mark.parametrize("name", ["main", "edge", "nofar"])
def test_factor_bits_do_not_depend_on_the_shadow(cases, name):
    c = cases[name]
    want = c.factor(c.far, c.mid, **{SHADOW: 0})
    assert not _has_shadow(c)
    assert np.isfinite(want).all()
    for mode in MODES:
        got = c.factor(c.far, c.mid, **{SHADOW: mode})
        assert _has_shadow(c)
        assert np.array_equal(got, want), f"{name}: OISAT_FACTOR_SHADOW={mode}"
    assert tuple(c.ctx.solve_status(clear=True))[:3] == (0, 0, 0)


@pytest.mark.parametrize("name", ["main", "edge", "nofar"])
def test_factor_and_forward_sweep_in_the_launch_that_carries_it(cases, name):
    c = cases[name]
    want_f, want_z = _factor_fwd(c, **{SHADOW: 0, FWD: None})
    assert not _has_shadow(c)
    assert np.array_equal(want_f, c.factor(c.far, c.mid, **{SHADOW: 0}))        # (the two launches agree to begin with)
    for mode in MODES:
        f, z = _factor_fwd(c, **{SHADOW: mode, FWD: None})
        assert _has_shadow(c)
        assert np.array_equal(f, want_f) and np.array_equal(z, want_z), f"{name}: OISAT_FACTOR_SHADOW={mode}"
    assert np.isfinite(want_z).all() and np.abs(want_z).max() > 0
    assert tuple(c.ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_a_stale_shadow_is_never_read(cases):
    """One handle, one S buffer, one set of tables -- one plan and one shadow buffer: a second matrix (another obs_var) over the
    shadow the first left, then the first again over the second's."""
    c = cases["main"]
    ctx = c.ctx
    first_a = c.factor(c.far, c.mid, **{SHADOW: None})
    ovar_a = c.ovar
    try:
        c.ovar = ctx.upload(3.0 * np.ravel(c.p.obs_var)[np.argsort(np.ravel(c.p.obs_lat).astype(np.float64), kind="stable")] + 0.05, dtype=np.float64)
        b = c.factor(c.far, c.mid, **{SHADOW: None})
        b_off = c.factor(c.far, c.mid, **{SHADOW: 0})
    finally:
        c.ovar = ovar_a
    assert not np.array_equal(b, first_a)
    assert np.array_equal(b, b_off)
    c.factor(c.far, c.mid, **{SHADOW: None})                    # (the shadow holds matrix a's images again ...)
    try:
        c.ovar = ctx.upload(3.0 * np.ravel(c.p.obs_var)[np.argsort(np.ravel(c.p.obs_lat).astype(np.float64), kind="stable")] + 0.05, dtype=np.float64)
        assert np.array_equal(c.factor(c.far, c.mid, **{SHADOW: None}), b_off)
    finally:
        c.ovar = ovar_a
    again_a = c.factor(c.far, c.mid, **{SHADOW: None})           # ... and now b's: a over them
    assert np.array_equal(again_a, first_a)
    assert np.array_equal(again_a, c.factor(c.far, c.mid, **{SHADOW: 0}))


def _bf16(a):
    """float32 -> bf16 bit patterns, round to nearest even (finite input)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def test_shadow_contents(cases):
    """hi = bf16(tile), lo = bf16(tile - hi) as bit patterns: a sub-diagonal tile (the chain writes it), ordinary tiles (a tile
    task does) at both ends of a row, a tile of the padded last block row -- and a tile outside the envelope is refused."""
    c = cases["main"]
    ctx, lib = c.ctx, c.ctx.lib
    f = c.factor(c.far, c.mid, **{SHADOW: None})
    nb, first = c.nb, c.first
    r = nb // 2
    assert r - first[r] >= 3 and (nb - 1) - first[nb - 1] >= 2 and c.m % NB != 0
    tiles = [(r, r - 1), (1, 0), (r, int(first[r])), (r, r - 2), (nb - 1, int(first[nb - 1])), (nb - 1, nb - 2)]
    hi, lo = np.empty((NB, NB), dtype=np.uint16), np.empty((NB, NB), dtype=np.uint16)
    for (i, k) in tiles:
        ctx.check(lib.oisat_factor_shadow_tile(ctx.h, i, k, hi.ctypes.data, lo.ctypes.data))
        tile = f[i * NB:(i + 1) * NB, k * NB:(k + 1) * NB]
        want_hi = _bf16(tile)
        want_lo = _bf16(tile - _bf16_value(want_hi))            # (exact in float32)
        assert np.abs(tile).max() > 0
        assert np.array_equal(hi, want_hi), (i, k)
        assert np.array_equal(lo, want_lo), (i, k)
    assert lo.any() and hi.any()
    assert lib.oisat_factor_shadow_tile(ctx.h, r, r, hi.ctypes.data, lo.ctypes.data) != 0          # the diagonal has no shadow
    if first[nb - 1] > 0:
        assert lib.oisat_factor_shadow_tile(ctx.h, nb - 1, int(first[nb - 1]) - 1, hi.ctypes.data, lo.ctypes.data) != 0
    assert lib.oisat_factor_shadow_tile(ctx.h, nb, 0, hi.ctypes.data, lo.ctypes.data) != 0
    assert lib.oisat_factor_shadow_tile(ctx.h, r, r - 1, None, lo.ctypes.data) != 0


def test_no_room_for_a_shadow_is_not_an_error(cases):
    """A cap of 0 bytes: the call succeeds, converts in its K-loops and gives the same bits; a cap one tile short likewise;
    without the cap the shadow is back."""
    c = cases["main"]
    ctx, lib = c.ctx, c.ctx.lib
    want = c.factor(c.far, c.mid, **{SHADOW: 0})
    ntiles = int((np.arange(c.nb) - c.first).sum())
    try:
        for cap in (0, (ntiles - 1) * 65536):
            ctx.check(lib.oisat_set_factor_shadow_cap(ctx.h, cap))
            assert np.array_equal(c.factor(c.far, c.mid, **{SHADOW: None}), want)
            assert not _has_shadow(c)
        ctx.check(lib.oisat_set_factor_shadow_cap(ctx.h, ntiles * 65536))
        assert np.array_equal(c.factor(c.far, c.mid, **{SHADOW: None}), want)
        assert _has_shadow(c)
    finally:
        ctx.check(lib.oisat_set_factor_shadow_cap(ctx.h, -1))
    assert lib.oisat_set_factor_shadow_cap(ctx.h, -2) != 0
    assert np.array_equal(c.factor(c.far, c.mid, **{SHADOW: None}), want) and _has_shadow(c)


def test_no_stretch_no_shadow_and_bad_switch(cases):
    """Without a far or a middle block no shadow is made; a malformed OISAT_FACTOR_SHADOW is refused where it would be read."""
    c = cases["main"]
    c.factor(c.first.copy(), c.first.copy(), **{SHADOW: None})
    assert not _has_shadow(c)
    c.factor(None, None, **{SHADOW: None})
    assert not _has_shadow(c)
    ctx, lib = c.ctx, c.ctx.lib
    with _environ(**{SHADOW: "both"}):
        ctx.check(lib.oisat_set_factor_far(ctx.h, c.far.ctypes.data, c.far.size))
        ctx.check(lib.oisat_set_factor_mid(ctx.h, c.mid.ctypes.data, c.mid.size))
        assert lib.oisat_potrf_env(ctx.h, c.S.ptr, c.m, c.mp, c.first.ctypes.data, c.env_dev.ptr, None) != 0
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_analysis_is_the_same_with_and_without(cases):
    """``DenseAnalysis.run()`` of the main case (the mid-band test's runner and its arguments): identical xa, inc, z, factor and
    residual lists."""
    c = cases["main"]
    run, _, _ = _runner(c.ctx, c.p, c.L)
    on = run(**{CUT: 28, FAR: 16, MID: 8, FWD: None, SHADOW: None})
    off = run(**{CUT: 28, FAR: 16, MID: 8, FWD: None, SHADOW: 0})
    assert on["schedule"] == off["schedule"] == dense.SCHEDULE_ENV_DAG_FWD
    assert np.array_equal(on["mid"], c.mid) and np.array_equal(on["far"], c.far)
    assert on["resid"] == off["resid"]
    for k in ("xa", "inc", "z", "factor"):
        assert np.array_equal(on[k], off[k]), k
    for mode in ("far", "mid"):
        half = run(**{CUT: 28, FAR: 16, MID: 8, FWD: None, SHADOW: mode})
        assert half["resid"] == off["resid"]
        for k in ("xa", "inc", "z"):
            assert np.array_equal(half[k], off[k]), (mode, k)
    assert tuple(c.ctx.solve_status(clear=True))[:3] == (0, 0, 0)
