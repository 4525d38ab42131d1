"""The far tier of the float64 sums on the device (csrc/dense_solve_dev.inc: ``kSolveFarBits``, ``OISAT_SOLVE_FAR_BITS``): the
increment and the compact-block residual evaluate the staged observations that are far from a whole block in packed fp32.
Checked here: the near list is untouched by the second list (0 bits against 52 bits, where nothing is far), the default
against a float64 host solve and against the run without the tier, a 4-bit tier that must show and stay inside its bound,
blocks whose two lists straddle a flush (direct calls, one and two cells per thread, runs of cells), the three tiled paths,
and the Gaspari-Cohn model, which has no tier."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc

pytestmark = pytest.mark.gpu
VAR = "OISAT_SOLVE_FAR_BITS"
L_KM = 300.0
LOG2E = float(np.float32(1.4426950408889634))
KEPT_BITS = 28.0                                                # kSolveFarBits (csrc/dense_solve_dev.inc): test_the_constant


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def test_the_constant(monkeypatch):
    """KEPT_BITS is the library's constant: the host query at the library's setting counts what it counts at KEPT_BITS, and
    differently one bit to either side."""
    monkeypatch.delenv(VAR, raising=False)
    g, _, _, _, olat, olon, _, _, _ = _straddle("far")
    rng = np.random.default_rng(9)
    extra = _disc(rng, 30.0, 20.0, 4000, 0.0, 0.5)                               # a dense disc: every bit moves some observation
    la, lo = np.concatenate([olat, extra[0]]), np.concatenate([olon, extra[1]])
    o = np.argsort(la, kind="stable")
    la, obs = np.ascontiguousarray(la[o]), np.ascontiguousarray(dense.unit_vectors(la[o], lo[o]))
    pts = dense.unit_vectors(np.array([29.0, 31.0]), np.array([19.0, 21.0]))
    at = {b: tier_counts(g, b, pts, obs, la, 29.0, 31.0) for b in (-1.0, KEPT_BITS - 1.0, KEPT_BITS, KEPT_BITS + 1.0)}
    assert at[-1.0] == at[KEPT_BITS] and at[KEPT_BITS - 1.0][1] > at[KEPT_BITS][1] > at[KEPT_BITS + 1.0][1] > 0


def set_bits(monkeypatch, bits):
    if bits is None:
        monkeypatch.delenv(VAR, raising=False)
    else:
        monkeypatch.setenv(VAR, str(bits))


def tier_counts(g, bits, pts, obs, olat, lo, hi):
    lib = _hip.load_library()
    pts, obs = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(obs, dtype=np.float64)
    near, far = C.c_int64(-1), C.c_int64(-1)
    assert lib.oisat_solve_tier_counts(0, C.c_double(g), C.c_double(bits), pts.ctypes.data, pts.shape[1], obs.ctypes.data, obs.shape[1],
                                       olat.ctypes.data, C.c_double(lo), C.c_double(hi), C.byref(near), C.byref(far)) == 0
    return int(near.value), int(far.value)


# ---- the analysis: 360x720 swaths, 72x144 (polar patches), 720x1440 (two cells per thread) ----------------------------------
# (increment_cells takes two cells per thread from 1024 workgroups of 512 cells on: 720x1440.  The two smaller grids run one.)
CASES = {"360x720_swaths": (360, 720, 3000, 9000, True), "72x144": (72, 144, 1000, 7000, False),
         "720x1440_swaths": (720, 1440, 3000, 9100, True)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case, and its float64 host solve (the oracle's formulas) on a selection of cells."""
    ny, nx, nobs, seed, swaths = CASES[name]
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    if ny == 72:
        sel = np.arange(ny * nx)
    else:                                                      # 4 000 random cells and the two rows next to each pole
        sel = np.unique(np.concatenate([np.random.default_rng(3).choice(ny * nx, 4000, replace=False), np.arange(2 * nx),
                                        np.arange((ny - 2) * nx, ny * nx)]))
    sb = np.sqrt(p.Sa.ravel())
    po = orc.unit_vectors(p.obs_lat, p.obs_lon)
    S = orc.gaussian_corr(po, po, L_KM) * sb[cell][:, None] * sb[cell][None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    z = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    pg = orc.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc = np.empty(sel.size)
    for i0 in range(0, sel.size, 2048):
        inc[i0:i0 + 2048] = sb[sel[i0:i0 + 2048]] * (orc.gaussian_corr(pg[i0:i0 + 2048], po, L_KM) @ (sb[cell] * z))
    for a in (sel, z, inc):
        a.setflags(write=False)
    return p, cell, y, sel, z, inc


_RUNS = {}


def run_dense(ctx, monkeypatch, name, bits, corr="gaussian"):
    """xa, inc, the float64 residual vector of the final z (a direct call, compact blocks) under these bits -- bits = None:
    under an explicit KEPT_BITS, the residual's tier being off unless the variable asks for it --, d, sig w, the refinement's
    residuals, and the residual vector of the SAME z without the tier; once per (case, bits)."""
    key = (name, bits, corr)
    if key in _RUNS:
        return _RUNS[key]
    p, cell, y, _, _, _ = _case(name)
    set_bits(monkeypatch, bits)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    try:
        resid = plan.run(L_KM, refine=2, check_pd=True, want_resid=True, corr=corr)
        xa, inc = plan.download()
        m, lib = plan.m, ctx.lib
        r = ctx.alloc(m * 8)
        rvs = []
        for b in (int(KEPT_BITS) if bits is None else bits, 0):
            set_bits(monkeypatch, b)
            ctx.check(lib.oisat_set_obs_blocks(ctx.h, plan.perm.ptr, m))
            ctx.check(lib.oisat_cov_residual(ctx.h, plan.oxyz.ptr, plan.osig.ptr, plan.ovar.ptr, m, plan._g, plan.d.ptr, plan.z.ptr, r.ptr,
                                             plan.olat.ptr))
            rvs.append(ctx.download(r.ptr, (m,), np.float64))
        rv, rv0 = rvs
        d = ctx.download(plan.d.ptr, (m,), np.float64)
        w = np.sqrt(p.Sa.ravel())[cell] * plan.download_z()
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)
    out = (xa.copy(), inc.copy(), rv, d, w, resid, rv0)
    for a in out[:5] + out[6:]:
        a.setflags(write=False)
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_far_tier_is_not_empty(name):
    """Host query: some patch of the grid stages far observations at the default and at 4 bits (the cases below test something),
    none at 52 bits, where the far radius is the cull's."""
    p, _, _, _, _, _ = _case(name)
    ny, nx = p.lat.shape
    g = dense.decay_constant(L_KM)
    o = np.argsort(p.obs_lat, kind="stable")
    olat = np.ascontiguousarray(p.obs_lat[o])
    obs = np.ascontiguousarray(dense.unit_vectors(olat, p.obs_lon[o]))
    rows = 16 if name.startswith("720") else 8
    far_def = far_4 = far_52 = 0
    for y0 in range(0, ny, max(rows, ny // 6)):
        for x0 in range(0, nx, max(32, nx // 6)):
            la, lo = p.lat[y0:y0 + rows, x0:x0 + 32], p.lon[y0:y0 + rows, x0:x0 + 32]
            pts = dense.unit_vectors(la.ravel(), lo.ravel())
            far_def += tier_counts(g, -1.0, pts, obs, olat, float(la.min()), float(la.max()))[1]
            far_4 += tier_counts(g, 4.0, pts, obs, olat, float(la.min()), float(la.max()))[1]
            far_52 += tier_counts(g, 52.0, pts, obs, olat, float(la.min()), float(la.max()))[1]
    print(f"{name}: far observations over the sampled patches: {far_def} at the default, {far_4} at 4 bits")
    assert 0 < far_def < far_4 and far_52 == 0


@pytest.mark.parametrize("name", list(CASES))
def test_near_list_untouched_by_the_second_list(ctx, monkeypatch, name):
    """0 bits (no tier: the far radius is +inf) and 52 bits (both kernels classify every survivor against a finite far radius,
    the cull's own, and keep two lists of which the second stays empty): identical xa, inc and residual vector."""
    a = run_dense(ctx, monkeypatch, name, 0)
    b = run_dense(ctx, monkeypatch, name, 52)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[5] == b[5]


@pytest.mark.parametrize("name", list(CASES))
def test_default_against_the_float64_solve_and_the_run_without_tier(ctx, monkeypatch, name):
    """inc and xa no further from the float64 host solve than the run without the tier is, + 1e-9 of the field's scale; the
    residual vector of the run's z under the tier at KEPT_BITS within 1e-12 |d| of the same z's without the tier, and not
    identical to it (the residual's tier is live when asked for)."""
    p, _, _, sel, _, inc_ref = _case(name)
    scale = np.abs(p.Xa).max()
    off = run_dense(ctx, monkeypatch, name, 0)
    on = run_dense(ctx, monkeypatch, name, None)
    xa_ref = p.Xa.ravel()[sel] + inc_ref

    def errs(run):
        return (np.abs(run[1].ravel()[sel].astype(np.float64) - inc_ref).max() / scale,
                np.abs(run[0].ravel()[sel].astype(np.float64) - xa_ref).max() / scale)

    e0, e1 = errs(off), errs(on)
    dr = np.abs(on[2] - on[6]).max() / np.linalg.norm(on[3])
    assert np.array_equal(off[2], off[6])
    moved = int((on[1] != off[1]).sum())
    print(f"{name}: inc / xa against the host solve: without tier {e0[0]:.3e} / {e0[1]:.3e}, default {e1[0]:.3e} / {e1[1]:.3e}; "
          f"inc elements that differ {moved} of {on[1].size}, max {np.abs(on[1] - off[1]).max() / scale:.3e}; "
          f"residual vector max |r - r0| / |d| = {dr:.3e}; residuals {on[5]} | {off[5]}")
    assert e0[0] <= 1e-5 and e0[1] <= 1e-5
    assert e1[0] <= e0[0] + 1e-9 and e1[1] <= e0[1] + 1e-9
    assert dr <= 1e-12
    assert not np.array_equal(on[2], on[6])


@pytest.mark.parametrize("name", list(CASES))
def test_four_bits_show_and_stay_bounded(ctx, monkeypatch, name):
    """A tier at 2^-4: inc differs from the run without by more than 1e-9 of the field's scale (the tier is live) and per cell
    by less than sig 2^-4 2e-5 sum|w| (a far term is at most 2^-4 |w|, its fp32 error at most 2e-5 of it)."""
    p, _, _, _, _, _ = _case(name)
    scale = np.abs(p.Xa).max()
    off = run_dense(ctx, monkeypatch, name, 0)
    on = run_dense(ctx, monkeypatch, name, 4)
    diff = np.abs(on[1].astype(np.float64) - off[1].astype(np.float64)).ravel()
    bound = np.sqrt(p.Sa.ravel()) * 2.0 ** -4 * 2e-5 * np.abs(off[4]).sum()
    print(f"{name}: 4 bits against no tier: max |inc - inc0| / scale = {diff.max() / scale:.3e}, largest diff / bound = "
          f"{(diff / bound).max():.3e}")
    assert diff.max() / scale > 1e-9
    assert (diff < bound).all()


def test_gaspari_cohn_ignores_the_variable(ctx, monkeypatch):
    a = run_dense(ctx, monkeypatch, "72x144", None, corr="gaspari_cohn")
    b = run_dense(ctx, monkeypatch, "72x144", 8, corr="gaspari_cohn")
    g = run_dense(ctx, monkeypatch, "72x144", None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[1], g[1])


# ---- blocks whose lists straddle a flush: direct calls of the increment on runs of cells (nx <= 0) and of the residual -------
def _disc(rng, centre_lat, centre_lon, count, r_lo, r_hi):
    """count points at chord distance r_lo .. r_hi from (centre_lat, centre_lon), uniform in area."""
    c = dense.unit_vectors(np.array([centre_lat]), np.array([centre_lon]))[:, 0]
    e1 = np.cross(c, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(c, e1)
    chord = np.sqrt(rng.uniform(r_lo ** 2, r_hi ** 2, count))
    ang = 2.0 * np.arcsin(0.5 * chord)
    az = rng.uniform(0.0, 2.0 * np.pi, count)
    q = np.cos(ang) * c[:, None] + np.sin(ang) * (np.cos(az) * e1[:, None] + np.sin(az) * e2[:, None])
    return np.degrees(np.arcsin(np.clip(q[2], -1, 1))), np.degrees(np.arctan2(q[1], q[0]))


@functools.lru_cache(maxsize=None)
def _straddle(kind):
    """512 cells in a 4 x 4 degree box at (30 N, 20 E) and observations on a disc around it: "far" = 300 close and 900 in the far
    ring, "near" = 700 close and 200 in the ring (chords: close < the tier's chord - rho, ring beyond the tier's chord + rho).
    The first 64 of the close ones sit within a chord of 0.004 of the centre: one compact block of rows for the residual (their
    positions in the latitude order are returned last)."""
    rng = np.random.default_rng(77 if kind == "far" else 78)
    g = dense.decay_constant(L_KM)
    clat, clon = 28.0 + 4.0 * rng.uniform(size=512), 18.0 + 4.0 * rng.uniform(size=512)
    c_far, c52 = np.sqrt(KEPT_BITS / (g * LOG2E)), np.sqrt(52.0 / (g * LOG2E))
    n_close, n_ring = (300, 900) if kind == "far" else (700, 200)
    la0, lo0 = _disc(rng, 30.0, 20.0, 64, 0.0, 0.004)
    la1, lo1 = _disc(rng, 30.0, 20.0, n_close - 64, 0.0, c_far - 0.07)
    la2, lo2 = _disc(rng, 30.0, 20.0, n_ring, c_far + 0.07, c52 - 0.01)
    olat, olon = np.concatenate([la0, la1, la2]), np.concatenate([lo0, lo1, lo2])
    o = np.argsort(olat, kind="stable")
    olat, olon = np.ascontiguousarray(olat[o]), olon[o]
    m = olat.size
    osig, z, gsig = rng.uniform(0.5, 1.5, m), rng.standard_normal(m), rng.uniform(0.5, 1.5, 512)
    return g, clat, clon, gsig, olat, olon, osig, z, np.flatnonzero(o < 64)


@pytest.mark.parametrize("kind", ["far", "near"])
@pytest.mark.parametrize("cells", [1, 2])
def test_increment_lists_straddle_a_flush(ctx, monkeypatch, kind, cells):
    """oisat_apply_increment (runs of cells).  cells = 2: 1024 x 512 cells, so that increment_cells takes two per thread; block 0
    is the box, every other cell lies at 75 S, out of every observation's reach.  cells = 1: the box alone, two blocks."""
    g, clat, clon, gsig, olat, olon, osig, z, _ = _straddle(kind)
    n = 512 if cells == 1 else 512 * 1024
    assert dense_cells(ctx, n) == cells
    glat, glon, gs = np.full(n, -75.0), np.linspace(-180.0, 180.0, n, endpoint=False), np.ones(n)
    glat[:512], glon[:512], gs[:512] = clat, clon, gsig
    obs = np.ascontiguousarray(dense.unit_vectors(olat, olon))
    per = 512 // (3 - cells)                                    # cells per block: 256 or 512
    for b0 in range(0, 512, per):
        sl = slice(b0, b0 + per)
        near, far = tier_counts(g, -1.0, dense.unit_vectors(clat[sl], clon[sl]), obs, olat, float(clat[sl].min()), float(clat[sl].max()))
        print(f"{kind}, {cells} cell(s) per thread, block at {b0}: near {near}, far {far}")
        assert 2 * near + far >= 1024 + 256                     # a flush before the last pass, and entries behind it
        assert (far > 512 and near < 512) if kind == "far" else (near > 512 and far < 512)
    d_g, d_gs, d_glat = ctx.upload(dense.unit_vectors(glat, glon)), ctx.upload(gs), ctx.upload(glat)
    d_o, d_os, d_z, d_olat = ctx.upload(obs), ctx.upload(osig), ctx.upload(z), ctx.upload(olat)
    out = ctx.alloc(n * 8)
    got = {}
    for bits in (0, 52, None, 4):
        set_bits(monkeypatch, bits)
        ctx.check(ctx.lib.oisat_memset(ctx.h, out.ptr, 0xff, n * 8))
        ctx.check(ctx.lib.oisat_apply_increment(ctx.h, _hip.F64, d_g.ptr, d_gs.ptr, n, d_o.ptr, d_os.ptr, d_z.ptr, olat.size, C.c_double(g),
                                                None, None, out.ptr, d_glat.ptr, d_olat.ptr))
        got[bits] = ctx.download(out.ptr, (n,), np.float64)
    w = osig * z
    pg = orc.unit_vectors(clat, clon)
    ref = gsig * (orc.gaussian_corr(pg, orc.unit_vectors(olat, olon), L_KM) @ w)
    sw = np.abs(w).sum()
    assert np.array_equal(got[0], got[52])
    assert (got[0][512:] == 0.0).all() and (got[None][512:] == 0.0).all()
    e0, e1 = np.abs(got[0][:512] - ref).max(), np.abs(got[None][:512] - ref).max()
    d_kept, d4 = np.abs(got[None][:512] - got[0][:512]), np.abs(got[4][:512] - got[0][:512])
    print(f"  against float64 NumPy: no tier {e0 / sw:.3e}, default {e1 / sw:.3e} of sum|w|; default - no tier {d_kept.max() / sw:.3e}, "
          f"4 bits - no tier {d4.max() / sw:.3e}")
    assert e0 <= 1e-9 * sw                                      # exp2_neg: 2e-10 of a term; the 2^-52 cull
    assert d_kept.max() > 0.0 and (d_kept <= gsig * 2.0 ** -KEPT_BITS * 2e-5 * sw).all() and e1 <= e0 + 1e-9 * sw
    assert d4.max() > 1e-9 * np.abs(ref).max() and (d4 < gsig * 2.0 ** -4 * 2e-5 * sw).all()


def dense_cells(ctx, n):
    """increment_cells (csrc/dense_solve_dev.inc) for one system of n cells on this device."""
    cus = int(ctx.device_info().get("cu_count", 256))
    return 1 if -(-n // 512) < 4 * cus else 2


@pytest.mark.parametrize("kind", ["far", "near"])
def test_residual_lists_straddle_a_flush(ctx, monkeypatch, kind):
    """oisat_cov_residual on compact blocks of rows, the tier asked for at KEPT_BITS (it is off otherwise).  The observations of
    the straddling case are the rows too; the permutation puts the 64 clustered ones first, so block 0 stages exactly the case's
    two lists -- 300 near / 900 far, or 700 / 200 -- in four column phases per row, with a flush before the last pass; the other
    blocks (the rest in latitude order, wide spheres) stage whatever they stage.  Every row against float64 NumPy."""
    g, _, _, _, olat, olon, osig, z, cluster = _straddle(kind)
    m = olat.size
    rng = np.random.default_rng(5)
    ovar, d = rng.uniform(0.1, 0.2, m), rng.standard_normal(m)
    obs = np.ascontiguousarray(dense.unit_vectors(olat, olon))
    perm = np.concatenate([cluster, np.setdiff1d(np.arange(m), cluster)]).astype(np.int32)
    assert cluster.size == 64 and np.array_equal(np.sort(perm), np.arange(m))
    counts = {}
    for bits in (KEPT_BITS, 4.0):
        counts[bits] = [tier_counts(g, bits, obs[:, perm[b0:b0 + 64]], obs, olat, float(olat[perm[b0:b0 + 64]].min()),
                                    float(olat[perm[b0:b0 + 64]].max())) for b0 in range(0, m, 64)]
        print(f"{kind}: (near, far) of the residual's blocks at {bits:g} bits: {counts[bits]}")
    near, far = counts[KEPT_BITS][0]
    assert (near, far) == ((300, 900) if kind == "far" else (700, 200))
    assert (far > 512 and near < 512) if kind == "far" else (near > 512 and far < 512)
    assert 2 * near + far >= 1024 + 256                         # a flush before the last pass, and entries behind it
    assert counts[4.0][0][1] > 0
    d_o, d_os, d_ov, d_d, d_z, d_olat, d_perm = (ctx.upload(a) for a in (obs, osig, ovar, d, z, olat, perm))
    out = ctx.alloc(m * 8)
    got = {}
    for bits in (0, 52, None, int(KEPT_BITS), 4):
        set_bits(monkeypatch, bits)
        ctx.check(ctx.lib.oisat_set_obs_blocks(ctx.h, d_perm.ptr, m))
        ctx.check(ctx.lib.oisat_cov_residual(ctx.h, d_o.ptr, d_os.ptr, d_ov.ptr, m, C.c_double(g), d_d.ptr, d_z.ptr, out.ptr, d_olat.ptr))
        got[bits] = ctx.download(out.ptr, (m,), np.float64)
    po = orc.unit_vectors(olat, olon)
    w = osig * z
    ref = d - (osig * (orc.gaussian_corr(po, po, L_KM) @ w) + ovar * z)
    sw = np.abs(w).sum()
    kept = got[int(KEPT_BITS)]
    e0, e1 = np.abs(got[0] - ref).max(), np.abs(kept - ref).max()
    d_kept, d4 = np.abs(kept - got[0]), np.abs(got[4] - got[0])
    print(f"  against float64 NumPy: no tier {e0 / sw:.3e}, {KEPT_BITS:g} bits {e1 / sw:.3e} of sum|w|; {KEPT_BITS:g} bits - no tier "
          f"{d_kept.max() / sw:.3e} (block 0: {d_kept[cluster].max() / sw:.3e}), / |d| {d_kept.max() / np.linalg.norm(d):.3e}; "
          f"4 bits - no tier {d4.max() / sw:.3e}")
    assert np.array_equal(got[0], got[52]) and np.array_equal(got[0], got[None])    # unset: the residual has no tier
    assert e0 <= 1e-12 * sw                                     # libm exp in double; the 2^-52 cull
    assert d_kept[cluster].max() > 0.0                          # the tier is live in the block whose lists were counted
    assert (d_kept <= osig * 2.0 ** -KEPT_BITS * 2e-5 * sw).all() and d_kept.max() <= 1e-12 * np.linalg.norm(d)
    assert d4.max() > 1e-9 * np.abs(ref).max() and (d4 < osig * 2.0 ** -4 * 2e-5 * sw).all()


# ---- the tiled paths -------------------------------------------------------------------------------------------------------
def test_tiled_paths_agree_with_the_tier_on(ctx, monkeypatch):
    """TiledAnalysis at 72 x 144 / 2 000 gridded observations / 60 degree tiles (the tiled case of tests/test_gpu_corr.py): each
    lane's own pipeline (batched=False), the lock-step batch and the one-launch task graph give identical fields with the tier
    on, at the default and at 4 bits -- where the tier moves the batch's fields, so the comparison is about something."""
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    ny, nx, tile = 72, 144, 60.0
    c = syn.diag_case(ny, nx, 2000, 4242)
    Y = np.where(c.Y < 0, 0.0, c.Y)                            # (OI_tiled's clamp and selection of the observed cells)
    cells = np.flatnonzero(np.isfinite(Y.ravel()) & np.isfinite(c.So.ravel()) & np.isfinite(c.Xa.ravel()) & np.isfinite(c.Sa.ravel()))
    xa_f, sa_f = np.where(np.isfinite(c.Xa), c.Xa, 0.0), np.where(np.isfinite(c.Sa), c.Sa, 0.0)
    olat, olon = c.lat.ravel()[cells], c.lon.ravel()[cells]
    out = {}
    for bits, modes in ((None, ("lanes", "batch", "one_launch")), (4, ("lanes", "batch", "one_launch")), (0, ("batch",))):
        set_bits(monkeypatch, bits)
        for mode in modes:
            monkeypatch.setenv("OISAT_DAG_SOLVE", "1" if mode == "one_launch" else "0")
            ta = dense.TiledAnalysis(c.lat, c.lon, tile_deg=tile, halo_km=3 * L_KM, dtype=np.float32, batched=mode != "lanes")
            try:
                ta.load(xa_f, sa_f, olat, olon, Y.ravel()[cells], c.So.ravel()[cells])
                if mode != "lanes":
                    assert ta.factor.one_launch == (mode == "one_launch")
                ta.run(L_KM, refine=2, check_pd=True)
                out[bits, mode] = tuple(a.copy() for a in ta.download())
            finally:
                ta.close()
    scale = np.abs(xa_f).max()
    print(f"4 bits against no tier, batch: max |inc - inc0| / scale = {np.abs(out[4, 'batch'][1] - out[0, 'batch'][1]).max() / scale:.3e}")
    assert not np.array_equal(out[4, "batch"][1], out[0, "batch"][1])               # the tier is live in the batch
    for bits in (None, 4):
        for mode in ("lanes", "one_launch"):
            for a, b in zip(out[bits, mode], out[bits, "batch"]):
                assert np.array_equal(a, b), (bits, mode)
