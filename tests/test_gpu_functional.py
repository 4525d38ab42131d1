"""The exact analysis error of regional means on the MI355X: the float64 pair sum ``oisat_functional_gather`` and the reduction
``oisat_rows_dot`` at the C ABI against NumPy, ``DenseAnalysis.functional_covariance`` end to end against the dense float64
reference of tests/functional_cases.py (whose docstring derives the bound), and the way in through ``OI_dense`` and the driver."""
import ctypes as C
import functools

import numpy as np
import pytest

import functional_cases as fc
from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
EINVAL = -1
FILL = 0x55


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


# ---- 1. the gather against the float64 reference ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_inputs():
    """Targets: the 300 observations of case a in ascending latitude (two runs of 256, the second partial); sources: all 1 152
    cells (more than one stage of 512), in ascending latitude; 64 rows of weights."""
    p = fc.case("a")
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    o = dense.latitude_order(p.obs_lat)
    sig = np.sqrt(np.ravel(p.Sa))
    s = dense.latitude_order(np.ravel(p.lat))
    out = {"pxyz": dense.unit_vectors(p.obs_lat[o], p.obs_lon[o]), "psig": sig[cell[o]], "plat": np.ascontiguousarray(p.obs_lat[o]),
           "sxyz": dense.unit_vectors(np.ravel(p.lat)[s], np.ravel(p.lon)[s]), "ssig": sig[s], "slat": np.ascontiguousarray(np.ravel(p.lat)[s]),
           "W": np.random.default_rng(77).normal(size=(64, sig.size))}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gather_reference(corr, L_km):
    """(out, sum of |terms|, sum of psig ssig |W|), each (64, npts), float64 NumPy with the library's correlation function."""
    q = gather_inputs()
    Cm = fc.corr_eval(fc.KINDS[corr], dense.decay_constant(L_km), fc.chord2(q["pxyz"], q["sxyz"]))
    P = q["psig"][:, None] * Cm * q["ssig"][None, :]                 # (npts, nsrc)
    full = q["psig"][:, None] * q["ssig"][None, :]
    return q["W"] @ P.T, np.abs(q["W"]) @ np.abs(P).T, np.abs(q["W"]) @ full.T


def excluded_pairs(lib, corr, L_km):
    """(block, source) pairs that the latitude window and the bounding-sphere cull leave out, restated on the host with the
    library's own 2^-52 chord."""
    q = gather_inputs()
    chord = C.c_double(0)
    assert lib.oisat_corr_cut_chord(fc.KINDS[corr], dense.decay_constant(L_km), 52.0, C.byref(chord)) == 0
    if chord.value >= 2.0:
        return 0
    win = 2.0 * np.degrees(np.arcsin(0.5 * chord.value))
    nsrc, gone = q["slat"].size, 0
    for b0 in range(0, q["plat"].size, 256):
        lat, pts = q["plat"][b0:b0 + 256], q["pxyz"][:, b0:b0 + 256]
        j0, j1 = np.searchsorted(q["slat"], lat.min() - win, "left"), np.searchsorted(q["slat"], lat.max() + win + 1e-9, "left")
        c = pts.sum(axis=1)
        keep = j1 - j0
        if np.linalg.norm(c) > 1e-9:
            c /= np.linalg.norm(c)
            rho = np.sqrt(((pts - c[:, None]) ** 2).sum(axis=0).max()) * (1 + 1e-12) + 1e-12
            keep = int((((q["sxyz"][:, j0:j1] - c[:, None]) ** 2).sum(axis=0) <= (chord.value + rho) ** 2).sum())
        gone += nsrc - keep
    return gone


def run_gather(ctx, q, W, L_km, corr, windowed, nfun=None, ldo=None, rows_out=None):
    """One call on fresh buffers with the first ``nfun`` rows of ``W`` (default: all); returns the whole out buffer
    (rows_out x ldo), which was filled with 0x55 bytes before the call."""
    c, lib = ctx, ctx.lib
    npts, nsrc = q["psig"].size, q["ssig"].size
    nfun = W.shape[0] if nfun is None else nfun
    ldo = npts if ldo is None else ldo
    rows_out = nfun if rows_out is None else rows_out
    bufs = [c.upload(q[k], dtype=np.float64) for k in ("pxyz", "psig", "plat", "sxyz", "ssig", "slat")]
    Wd = c.upload(W, dtype=np.float64)
    out = c.alloc(rows_out * ldo * 8)
    c.check(lib.oisat_memset(c.h, out.ptr, FILL, rows_out * ldo * 8))
    c.check(lib.oisat_set_correlation(c.h, fc.KINDS[corr]))
    c.check(lib.oisat_functional_gather(c.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if windowed else None, npts, bufs[3].ptr, bufs[4].ptr,
                                        bufs[5].ptr if windowed else None, nsrc, Wd.ptr, nfun, W.shape[1], dense.decay_constant(L_km),
                                        out.ptr, ldo))
    c.sync()
    return c.download(out.ptr, (rows_out, ldo), np.float64)


@pytest.mark.parametrize("corr,L_km,culls", [("gaussian", 300.0, True), ("gaspari_cohn", 300.0, True), ("soar", 300.0, False),
                                             ("soar", 60.0, True)])
def test_gather_matches_the_float64_sum(ctx, corr, L_km, culls):
    """Bound per entry, windowed and unwindowed alike: 64 nsrc 2^-53 sum |term| -- the rounding of a double sum of nsrc terms,
    each a few ulp from the exponential.  Windowed against unwindowed: 2^-52 sum psig ssig |W|, what the terms left out can
    amount to.  nfun 1, 5, 8, 13 stay inside one group of 16 functionals (the tail group); 17, 33 and 64 run the kernel's group
    loop two, three and four times, with a tail of 1, a tail of 1 behind two full groups, and no tail.  (SOAR at 300 km reaches
    11 900 km at 2^-52: its window is on and leaves nothing out on this grid, so it is also run at 60 km.)"""
    q = gather_inputs()
    gone = excluded_pairs(ctx.lib, corr, L_km)
    print(f"{corr} L = {L_km:g} km: the window and the cull leave out {gone} of {2 * q['ssig'].size} (block, source) pairs")
    assert (gone >= 1) == culls                                       # the culled path really runs
    ref, ref_abs, full = gather_reference(corr, L_km)
    nsrc = q["ssig"].size
    for nfun in (1, 5, 8, 13, 17, 33, 64):
        W = np.full((80, nsrc), np.nan)                              # rows nfun .. 79 are NaN: never to be read
        W[:nfun] = q["W"][:nfun]
        outs = {}
        for windowed in (False, True):
            got = run_gather(ctx, q, W, L_km, corr, windowed, nfun=nfun, rows_out=80)
            assert np.isfinite(got[:nfun]).all()
            assert (got[nfun:].view(np.uint8) == FILL).all()         # rows beyond nfun: not written
            err = np.abs(got[:nfun] - ref[:nfun])
            bound = 64.0 * nsrc * 2.0 ** -53 * ref_abs[:nfun]
            print(f"  nfun {nfun:2d} windowed {windowed!s:5}: worst error / bound = {np.max(err / bound):.3g}")
            assert (err <= bound).all()
            outs[windowed] = got[:nfun]
        assert (np.abs(outs[True] - outs[False]) <= 2.0 ** -52 * full[:nfun]).all()


def test_gather_edge_cases(ctx):
    q = dict(gather_inputs())
    L_km, g = 300.0, dense.decay_constant(300.0)
    # one target, one source, coincident: C = 1 exactly under every model
    one = {"pxyz": q["sxyz"][:, 5:6], "psig": np.array([1.5]), "plat": q["slat"][5:6], "sxyz": q["sxyz"][:, 5:6],
           "ssig": np.array([0.75]), "slat": q["slat"][5:6]}
    for corr in fc.KINDS:
        for windowed in (False, True):
            got = run_gather(ctx, one, np.array([[2.0], [-3.0]]), L_km, corr, windowed)
            assert got.tolist() == [[1.5 * 0.75 * 2.0], [1.5 * 0.75 * -3.0]], (corr, windowed)
    # the targets are the first 300 SOURCES: every target coincides with a source; ldo > npts leaves the padding alone
    co = dict(q, pxyz=np.ascontiguousarray(q["sxyz"][:, :300]), psig=q["ssig"][:300], plat=q["slat"][:300])
    W = q["W"][:5]
    a = run_gather(ctx, co, W, L_km, "gaussian", True, ldo=307)
    b = run_gather(ctx, co, W, L_km, "gaussian", True, ldo=307)
    assert a.tobytes() == b.tobytes()                                # same inputs, same bits
    assert (np.ascontiguousarray(a[:, 300:]).view(np.uint8) == FILL).all()
    Cm = fc.corr_eval(0, g, fc.chord2(co["pxyz"], q["sxyz"]))
    assert (np.diag(Cm[:, :300]) == 1.0).all()
    P = co["psig"][:, None] * Cm * q["ssig"][None, :]
    err = np.abs(a[:, :300] - W @ P.T)
    assert (err <= 64.0 * 1152 * 2.0 ** -53 * (np.abs(W) @ np.abs(P).T)).all()
    # one target over every source, and every target over one source
    ref, ref_abs, _ = gather_reference("gaussian", L_km)
    t, j = 17, 700
    single = dict(q, pxyz=np.ascontiguousarray(q["pxyz"][:, t:t + 1]), psig=q["psig"][t:t + 1], plat=q["plat"][t:t + 1])
    lone = dict(q, sxyz=np.ascontiguousarray(q["sxyz"][:, j:j + 1]), ssig=q["ssig"][j:j + 1], slat=q["slat"][j:j + 1])
    Wj = np.ascontiguousarray(W[:, j:j + 1])
    c1 = fc.corr_eval(0, g, fc.chord2(q["pxyz"], lone["sxyz"]))[:, 0]
    want = Wj * (q["psig"] * c1 * q["ssig"][j])[None, :]
    full = np.abs(Wj) * (q["psig"] * q["ssig"][j])[None, :]
    for windowed in (False, True):
        got = run_gather(ctx, single, W, L_km, "gaussian", windowed)
        assert got.shape == (5, 1) and (np.abs(got[:, 0] - ref[:5, t]) <= 64.0 * 1152 * 2.0 ** -53 * ref_abs[:5, t]).all()
    plain, culled = (run_gather(ctx, lone, Wj, L_km, "gaussian", windowed) for windowed in (False, True))
    # a single term: what bounds it is the rounding of the exponential's ARGUMENT x = g d^2, formed on either side from products
    # and sums that each round to 2^-53 relative (up to x = 900 here), a relative 16 x 2^-53 of the term beside the few ulp of the
    # function itself; below the normal range (x > 708) only the absolute spacing is left
    x = g * fc.chord2(q["pxyz"], lone["sxyz"])[:, 0]
    assert plain.shape == (5, 300) and (np.abs(plain - want) <= (64.0 + 16.0 * x)[None, :] * 2.0 ** -53 * np.abs(want) + 2.0 ** -1022 * full).all()
    assert (np.abs(culled - plain) <= 2.0 ** -52 * full).all() and (culled == 0).any() and (culled == plain).any()


def test_gather_refuses_bad_arguments_and_launches_nothing(ctx):
    c, lib = ctx, ctx.lib
    q = gather_inputs()
    npts, nsrc = 300, 1152
    bufs = [c.upload(q[k], dtype=np.float64) for k in ("pxyz", "psig", "plat", "sxyz", "ssig", "slat")]
    Wd = c.upload(q["W"], dtype=np.float64)
    out = c.alloc(13 * npts * 8)
    c.check(lib.oisat_memset(c.h, out.ptr, FILL, 13 * npts * 8))
    good = dict(h=c.h, pxyz=bufs[0].ptr, psig=bufs[1].ptr, plat=bufs[2].ptr, npts=npts, sxyz=bufs[3].ptr, ssig=bufs[4].ptr, slat=bufs[5].ptr,
                nsrc=nsrc, W=Wd.ptr, nfun=13, ldw=nsrc, g=dense.decay_constant(300.0), out=out.ptr, ldo=npts)
    bad = [dict(nfun=0), dict(nfun=65), dict(nfun=-1), dict(npts=0), dict(nsrc=0), dict(ldw=nsrc - 1), dict(ldo=npts - 1), dict(h=None),
           dict(pxyz=None), dict(psig=None), dict(sxyz=None), dict(ssig=None), dict(W=None), dict(out=None), dict(nsrc=2 ** 31, ldw=2 ** 31), dict(nsrc=2 ** 31 - 1, ldw=2 ** 31 - 1), dict(g=-1.0), dict(g=float("nan"))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.oisat_functional_gather(*(a[k] for k in good))
        assert rc == EINVAL, change
    c.sync()
    assert (c.download(out.ptr, (13 * npts,), np.float64).view(np.uint8) == FILL).all()
    assert lib.oisat_functional_gather(*good.values()) == 0          # ... and the good call goes through
    c.sync()
    assert np.isfinite(c.download(out.ptr, (13 * npts,), np.float64)).all()


# ---- 2. oisat_rows_dot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 255, 1000])
def test_rows_dot_against_numpy(ctx, length):
    """na = 3 against nb = 13 (two groups of rows of B, the second partial), leading dimensions wider than the length.  Bound:
    len 2^-52 sum |a b|."""
    c, lib = ctx, ctx.lib
    rng = np.random.default_rng(length)
    lda, ldb = length + 3, length + 8
    A, B = rng.normal(size=(3, lda)), rng.normal(size=(13, ldb))
    Ad, Bd = c.upload(A), c.upload(B)
    outs = []
    for _ in range(2):
        out = c.alloc(3 * 13 * 8)
        c.check(lib.oisat_memset(c.h, out.ptr, FILL, 3 * 13 * 8))
        c.check(lib.oisat_rows_dot(c.h, Ad.ptr, lda, 3, Bd.ptr, ldb, 13, length, out.ptr))
        c.sync()
        outs.append(c.download(out.ptr, (3, 13), np.float64))
    assert outs[0].tobytes() == outs[1].tobytes()
    a, b = A[:, :length], B[:, :length]
    err, bound = np.abs(outs[0] - a @ b.T), length * 2.0 ** -52 * (np.abs(a) @ np.abs(b).T)
    print(f"len {length}: worst error / bound = {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    # the transposed roles (13 x 3) give the transposed result to the bit: the tree depends on len alone
    out = c.alloc(13 * 3 * 8)
    c.check(lib.oisat_rows_dot(c.h, Bd.ptr, ldb, 13, Ad.ptr, lda, 3, length, out.ptr))
    c.sync()
    assert c.download(out.ptr, (13, 3), np.float64).T.tobytes() == outs[0].tobytes()


def test_rows_dot_refuses_bad_arguments(ctx):
    c, lib = ctx, ctx.lib
    Ad = c.upload(np.ones((4, 16)))
    out = c.alloc(64 * 64 * 8)
    good = dict(h=c.h, A=Ad.ptr, lda=16, na=4, B=Ad.ptr, ldb=16, nb=4, len=16, out=out.ptr)
    for change in (dict(h=None), dict(A=None), dict(B=None), dict(out=None), dict(na=0), dict(na=65), dict(nb=0), dict(nb=65), dict(len=0),
                   dict(lda=15), dict(ldb=15)):
        a = dict(good, **change)
        assert lib.oisat_rows_dot(*(a[k] for k in good)) == EINVAL, change
    assert lib.oisat_rows_dot(*good.values()) == 0
    c.sync()
    assert (c.download(out.ptr, (4, 4), np.float64) == 16.0).all()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------
# the reference's own cross term between the box and the far region is below the bound in these cases; at L = 1 000 km (case b)
# it is not -- the observations couple the two regions across 7 000 km at 1.3e-7 of the prior's scale, 120 times the bound --
# and there the device's term is held to the reference's like every other entry
CROSS_FREE = ("a", "c")


def analysed_plan(name):
    p = fc.case(name)
    L = fc.CASES[name][3]
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=p.obs_y.size, dtype=np.float64, diag_chunk_rows=4096)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, np.where(p.obs_y < 0, 0.0, p.obs_y), p.obs_var)
    plan.run(L, refine=fc.REFINE, check_pd=True, tol=fc.TOL)
    plan.check()
    return plan


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_functional_covariance_against_the_float64_reference(ctx, name):
    ref = fc.reference(name)
    bound = fc.bound(ref)
    W, hot = fc.functionals(name)
    k, l = fc.I_BOX, fc.I_FAR
    if name in CROSS_FREE:
        assert abs(ref["posterior"][k, l]) <= bound[k, l]            # on the host first
    plan = analysed_plan(name)
    with pytest.raises(ValueError):
        plan.functional_covariance(np.ones((65, plan.n)))
    with pytest.raises(ValueError):
        plan.functional_covariance(np.ones((2, plan.n + 1)))
    out = plan.functional_covariance(W, refine=fc.REFINE, tol=fc.TOL)
    post, prior = out["posterior"], out["prior"]
    assert post.shape == prior.shape == out["reduction"].shape == (6, 6) and out["resid"].shape == (6,)
    for a in (post, prior, out["reduction"]):
        assert a.dtype == np.float64 and np.array_equal(a, a.T)
    assert np.array_equal(post, prior - out["reduction"])
    assert out["support"] == int(((W.reshape(6, -1) != 0).any(axis=0) & (ref["sig"] > 0)).sum())
    scale = np.where(bound > 0, bound, 1.0)
    e_post, e_prior = np.abs(post - ref["posterior"]), np.abs(prior - ref["prior"])
    print(f"case {name}: cond(S) {ref['cond']:.1f}; worst |posterior - reference| / bound {np.max(e_post / scale):.3g}, prior "
          f"{np.max(e_prior / scale):.3g}; resid {out['resid']}; posterior / prior {np.diag(post)[:5] / np.diag(prior)[:5]}; "
          f"box-far cross term {post[k, l]:.3g} (reference {ref['posterior'][k, l]:.3g}, bound {bound[k, l]:.3g})")
    assert (e_post <= bound).all()
    assert (e_prior <= bound).all()
    assert (out["resid"] <= fc.TOL).all() and out["resid"][fc.I_ZERO] == 0.0 and (out["resid"][:5] > 0).all()
    assert (np.diag(post) <= np.diag(prior)).all()
    assert np.linalg.eigvalsh(post).min() >= -bound.max()
    for a in (post, prior, out["reduction"]):
        assert (a[fc.I_ZERO] == 0).all() and (a[:, fc.I_ZERO] == 0).all()
    if name in CROSS_FREE:
        assert abs(post[k, l]) <= bound[k, l]
    # the one-hot functional is the refined exact error of one cell: the fp32 route's figure at that cell, at that route's bar
    err = plan.posterior_error().ravel()[hot]
    print(f"case {name}: error at cell {hot}: functional {np.sqrt(post[fc.I_ONEHOT, fc.I_ONEHOT]):.9g}, posterior_error() {err:.9g}, "
          f"reference {np.sqrt(ref['posterior'][fc.I_ONEHOT, fc.I_ONEHOT]):.9g}")
    np.testing.assert_allclose(np.sqrt(post[fc.I_ONEHOT, fc.I_ONEHOT]), err, rtol=2e-3, atol=1e-4 * ref["sig"][hot])
    # twenty functionals -- two groups of the gather, the second a tail of four: mixtures M W of the six, whose covariances are
    # M A M^T exactly; the same bound, from the mixtures' own priors
    M = np.random.default_rng(20).normal(size=(20, 6))
    out20 = plan.functional_covariance(M @ W.reshape(6, -1), refine=fc.REFINE, tol=fc.TOL)
    want_prior, want_post = M @ ref["prior"] @ M.T, M @ ref["posterior"] @ M.T
    d20 = np.sqrt(np.diag(want_prior))
    bound20 = (2.0 * fc.TOL ** 2 * ref["cond"] + 1e-11) * d20[:, None] * d20[None, :]
    e20, p20 = np.abs(out20["posterior"] - want_post), np.abs(out20["prior"] - want_prior)
    print(f"case {name}: twenty mixtures: worst |posterior - reference| / bound {np.max(e20 / bound20):.3g}, prior {np.max(p20 / bound20):.3g}; "
          f"resid max {out20['resid'].max():.3g}")
    assert out20["posterior"].shape == (20, 20) and (e20 <= bound20).all() and (p20 <= bound20).all()
    assert (out20["resid"] <= fc.TOL).all() and (out20["resid"] > 0).all()
    # empty support altogether: zeros, no solve
    none = plan.functional_covariance(np.zeros((2, plan.n)))
    assert none["support"] == 0 and not none["posterior"].any() and not none["resid"].any()


def test_functional_covariance_wants_a_run_first(ctx):
    p = fc.case("a")
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=300, dtype=np.float64)
    plan.load_background(p.Xa, p.Sa)
    with pytest.raises(ValueError, match="must follow run"):
        plan.functional_covariance(fc.functionals("a")[0])


def region_labels(name):
    """1 = the box, 2 = the far region, 3 = the rest of the band 20-50 N; some cells of the box have no background."""
    p = fc.case(name)
    labels = np.zeros(p.lat.shape, dtype=np.int64)
    labels[(p.lat > 20.0) & (p.lat < 50.0)] = 3
    labels[(p.lat > 25.0) & (p.lat < 45.0) & (p.lon > 0.0) & (p.lon < 60.0)] = 1
    labels[(p.lat < -30.0) & (p.lon > 100.0)] = 2
    Xa = np.array(p.Xa, dtype=np.float64)
    obs_cells = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    free = np.setdiff1d(np.flatnonzero(labels.ravel() == 1), obs_cells)[:3]
    Xa.flat[free] = np.nan                                           # (unobserved cells, so that the system stays the same)
    return labels, Xa, free


@pytest.mark.parametrize("superob", [None, 0.25])
def test_oi_dense_reports_the_regions(ctx, superob):
    name = "a"
    p, L = fc.case(name), fc.CASES[name][3]
    labels, Xa, free = region_labels(name)
    Sa = np.where(np.isfinite(Xa), p.Sa, np.nan)
    obs = dict(lat=p.obs_lat, lon=p.obs_lon, y=p.obs_y, var=p.obs_var)
    xb, inc, info = dense.OI_dense(Xa, None, Sa, None, p.lat, p.lon, L, refine=fc.REFINE, tol=fc.TOL, obs=obs, regions=labels,
                                   superob=superob, dtype=np.float64)
    if superob is not None:
        assert (info["superob"]["count"] == 1).all() and info["superob"]["nobs"] == 300      # one member per box: the same system
    reg = info["regions"]
    ids, W = dense.region_weights(labels, p.lat, valid=np.isfinite(Xa))
    assert reg["ids"].tolist() == ids.tolist() == [1, 2, 3] and (W[0].flat[free] == 0).all()
    # the same numbers as the method on a plan prepared the same way
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=300, dtype=np.float64)
    plan.load_background(np.where(np.isfinite(Xa), Xa, 0.0), np.where(np.isfinite(Sa), Sa, 0.0))
    plan.load_obs(p.obs_lat, p.obs_lon, cell, np.where(p.obs_y < 0, 0.0, p.obs_y), p.obs_var)
    plan.run(L, refine=fc.REFINE, check_pd=True, tol=fc.TOL)
    want = plan.functional_covariance(W, refine=fc.REFINE, tol=fc.TOL)
    d = np.sqrt(np.diag(want["prior"]))
    bound = (2.0 * fc.TOL ** 2 * fc.reference(name)["cond"] + 1e-11) * d[:, None] * d[None, :]
    if superob is None:
        assert np.array_equal(reg["posterior_cov"], want["posterior"]) and np.array_equal(reg["prior_cov"], want["prior"])
    print(f"superob {superob}: worst |posterior_cov - plan's| / bound = {np.max(np.abs(reg['posterior_cov'] - want['posterior']) / bound):.3g}")
    assert (np.abs(reg["posterior_cov"] - want["posterior"]) <= 2.0 * bound).all()       # (either within the bound of the exact one)
    assert (np.abs(reg["prior_cov"] - want["prior"]) <= bound).all()
    np.testing.assert_array_equal(reg["prior_sd"], np.sqrt(np.diag(reg["prior_cov"])))
    np.testing.assert_array_equal(reg["posterior_sd"], np.sqrt(np.diag(reg["posterior_cov"])))
    assert (reg["posterior_sd"] < reg["prior_sd"]).all() and (reg["resid"] <= fc.TOL).all()
    # the means: W x in float64 over the cells with a background
    ok = np.isfinite(Xa)
    assert np.isnan(xb[~ok]).all()
    Wf = W.reshape(3, -1)
    np.testing.assert_allclose(reg["background_mean"], Wf[:, ok.ravel()] @ Xa[ok], rtol=1e-13)
    np.testing.assert_allclose(reg["analysis_mean"], Wf[:, ok.ravel()] @ np.asarray(xb, dtype=np.float64)[ok], rtol=1e-13)
    assert np.isfinite(reg["analysis_mean"]).all() and not np.array_equal(reg["analysis_mean"], reg["background_mean"])


def test_oi_dense_without_observations_keeps_the_prior(ctx):
    p, L = fc.case("a"), fc.CASES["a"][3]
    labels, Xa, _ = region_labels("a")
    Y = np.full(Xa.shape, np.nan)
    xb, inc, info = dense.OI_dense(Xa, Y, p.Sa, Y.copy(), p.lat, p.lon, L, regions=labels, dtype=np.float64)
    reg = info["regions"]
    assert info["nobs"] == 0 and not inc.any()
    assert np.array_equal(reg["posterior_cov"], reg["prior_cov"]) and np.array_equal(reg["posterior_sd"], reg["prior_sd"])
    assert np.array_equal(reg["analysis_mean"], reg["background_mean"]) and not reg["resid"].any()
    # ... and that prior is W B W^T
    ids, W = dense.region_weights(labels, p.lat, valid=np.isfinite(Xa))
    ref = fc.reference("a")
    sig = np.where(np.isfinite(Xa.ravel()), ref["sig"], 0.0)
    B = fc.corr_eval(0, ref["g"], fc.chord2(ref["pg"], ref["pg"])) * sig[:, None] * sig[None, :]
    Wf = W.reshape(3, -1)
    want = Wf @ B @ Wf.T
    d = np.sqrt(np.diag(want))
    assert (np.abs(reg["prior_cov"] - want) <= 1e-11 * d[:, None] * d[None, :]).all()


# ---- 4. the driver --------------------------------------------------------------------------------------------------------------------------
def test_the_driver_fills_region_oi_in_dense_mode_and_refuses_tiled(ctx, monkeypatch, tmp_path):
    from oisatgmi.driver import oisatgmi
    c = syn.diag_case(24, 48, 300, 4703)
    labels = region_labels("a")[0]
    path = tmp_path / "regions.npy"
    np.save(path, labels)
    for var in ("OISAT_OI_QC", "OISAT_CORR_LENGTH_KM", "OISAT_CORRELATION", "OISAT_UNOBSERVED", "OISAT_OI_SUPEROB", "OISAT_OI_REGIONS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OISAT_OI_ERROR", "0")
    monkeypatch.setenv("OISAT_CORR_LENGTH_KM", "500")

    def facade(mode):
        o = oisatgmi()
        o.ctm_averaged_vcd, o.sat_averaged_vcd, o.sat_averaged_error = c.Xa.copy(), c.Y.copy(), c.sat_err.copy()
        o.grid_lat, o.grid_lon, o.oi_mode = c.lat, c.lon, mode
        return o

    o = facade("dense")
    o.oi_regions = labels
    o.oi("TROPOMI")
    reg = o.region_OI
    assert reg is o.oi_info["regions"] and reg["ids"].tolist() == [1, 2, 3]
    assert (reg["posterior_sd"] < reg["prior_sd"]).all() and (reg["posterior_sd"] > 0).all() and (reg["resid"] <= dense.REFINE_TOL).all()
    assert reg["prior_cov"].shape == reg["posterior_cov"].shape == (3, 3)
    o2 = facade("dense")                                             # the variable: a path; the same numbers
    monkeypatch.setenv("OISAT_OI_REGIONS", str(path))
    o2.oi("TROPOMI")
    assert np.array_equal(o2.region_OI["posterior_cov"], reg["posterior_cov"])
    assert o2.ctm_averaged_vcd_corrected.tobytes() == o.ctm_averaged_vcd_corrected.tobytes()
    with pytest.raises(ValueError, match="belongs to the dense mode"):
        facade("tiled").oi("TROPOMI")
    monkeypatch.delenv("OISAT_OI_REGIONS")
    o3 = facade("dense")                                             # unset: nothing changes, nothing is added
    o3.oi("TROPOMI")
    assert not hasattr(o3, "region_OI") and "regions" not in o3.oi_info
    assert o3.ctm_averaged_vcd_corrected.tobytes() == o.ctm_averaged_vcd_corrected.tobytes()
