"""The SOAR (Matern nu = 3/2) correlation on the device (``corr="soar"``, ``oisat_set_correlation(h, 3)``): S as built, the dense
analysis against a float64 host solve of the SOAR system, the other models' bits next to it, the float64 sums with and without
the latitude window, the batched / tiled paths, the diagnostics and the driver.  The references are float64 NumPy / SciPy
written here and in tests/readers_cases.py (the oracle has the Gaussian only)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oisatgmi import _hip, dense, synthetic as syn
from readers_cases import chord2, corr_ref as _corr_ref, gc_ref          # the float64 restatements of the formulas in oisat.h

pytestmark = pytest.mark.gpu
NB = 128
SOAR, GC, GAUSSIAN = "soar", "gaspari_cohn", "gaussian"
KIND = 3


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def corr_ref(pa, pb, L, model=SOAR):
    return _corr_ref(pa, pb, L, model)


def host_analysis(p, cell, y, L, sel, model=SOAR):
    """float64: z = S^-1 d by Cholesky, the increment on the cells ``sel``."""
    sb = np.sqrt(p.Sa.ravel())
    po = dense.unit_vectors(p.obs_lat, p.obs_lon)
    S = corr_ref(po, po, L, model)
    S *= sb[cell][:, None]
    S *= sb[cell][None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    z = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), y - p.Xa.ravel()[cell])
    pg = dense.unit_vectors(p.lat.ravel()[sel], p.lon.ravel()[sel])
    inc = np.empty(sel.size)
    for i0 in range(0, sel.size, 4096):
        inc[i0:i0 + 4096] = sb[sel[i0:i0 + 4096]] * (corr_ref(pg[:, i0:i0 + 4096], po, L, model) @ (sb[cell] * z))
    return z, inc


# ---- 1. S as built ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [100.0, 500.0])
def test_covariance_as_built(ctx, L, monkeypatch):
    """|S - S_ref| <= 3e-5 sig_a sig_b + 2^-23 |S_ref| off the diagonal of the lower triangle (the bound of the Gaspari-Cohn
    test; SOAR's fp32 form has fewer roundings: v_sqrt_f32, v_exp_f32, one fma, two products), sig^2 + var on it, identity
    padding, exact zeros in the lower tiles outside the table."""
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    lib = ctx.lib
    p = syn.point_obs_case(72, 144, 385, 6385)
    m = int(p.obs_y.size)
    mp = -(-m // NB) * NB
    nb = mp // NB
    o = np.argsort(p.obs_lat, kind="stable")
    lat, lon = np.ascontiguousarray(p.obs_lat[o]), p.obs_lon[o]
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    sig, var = np.sqrt(p.Sa.ravel()[cell]), np.ascontiguousarray(p.obs_var[o])
    xyz = dense.unit_vectors(lat, lon)
    g = dense.decay_constant(L)
    ref = np.eye(mp)
    ref[:m, :m] = corr_ref(xyz, xyz, L) * sig[:, None] * sig[None, :]
    ref[np.arange(m), np.arange(m)] = sig ** 2 + var
    ss = np.zeros((mp, mp))
    ss[:m, :m] = sig[:, None] * sig[None, :]
    env = np.empty(2 * nb, dtype=np.int32)
    assert lib.oisat_envelope_corr(KIND, lat.ctypes.data, m, C.c_double(g), env.ctypes.data) == 0
    first = env[:nb]
    if L == 100.0:
        assert first.any()
    else:
        assert not first.any()
    d_xyz, d_sig, d_var, d_env = ctx.upload(xyz), ctx.upload(sig), ctx.upload(var), ctx.upload(env)
    S = ctx.alloc(mp * mp * 4)
    low = np.tril(np.ones((mp, mp), dtype=bool), -1)
    outside = np.zeros((mp, mp), dtype=bool)
    for i in range(nb):
        outside[i * NB:(i + 1) * NB, :first[i] * NB] = True
    ctx.check(lib.oisat_set_correlation(ctx.h, KIND))
    try:
        for name in ("oisat_cov_build", "oisat_cov_build_env"):
            ctx.check(lib.oisat_memset(ctx.h, S.ptr, 0x55, mp * mp * 4))
            if name == "oisat_cov_build":
                ctx.check(lib.oisat_cov_build(ctx.h, d_xyz.ptr, d_sig.ptr, d_var.ptr, m, g, S.ptr, mp))
            else:
                ctx.check(lib.oisat_cov_build_env(ctx.h, d_xyz.ptr, d_sig.ptr, d_var.ptr, m, g, S.ptr, mp, d_env.ptr))
            got = ctx.download(S.ptr, (mp, mp), np.float32)
            err = np.abs(got.astype(np.float64) - ref)
            bound = 3e-5 * ss + 2.0 ** -23 * np.abs(ref)
            print(f"L = {L:g} {name}: max |S - S_ref| / (sig_a sig_b) off the diagonal = "
                  f"{(err[:m, :m][low[:m, :m]] / ss[:m, :m][low[:m, :m]]).max():.3e}")
            assert (err[low] <= bound[low]).all()
            dg = np.arange(mp)
            assert (err[dg, dg] <= 2.0 ** -23 * ref[dg, dg]).all()
            assert (got[m:, :][low[m:, :]] == 0.0).all() and (got[dg[m:], dg[m:]] == 1.0).all()
            if name == "oisat_cov_build_env":                   # (what is dropped there is below 2^-52 sig_a sig_b)
                assert (got[outside & low] == 0.0).all()
    finally:
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))


# ---- 2. the analysis against a float64 host solve ----------------------------------------------------------------------------
CASES = {"72x144_L300": (72, 144, 1000, 7000, False, 300.0), "72x144_L500": (72, 144, 1000, 7000, False, 500.0),
         "360x720_swaths_L300": (360, 720, 3000, 9000, True, 300.0)}


@functools.lru_cache(maxsize=None)
def _case(name):
    ny, nx, nobs, seed, swaths, L = CASES[name]
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    if ny == 72:
        sel = np.arange(ny * nx)
    else:                                                      # 4 000 random cells and the two rows next to each pole
        sel = np.unique(np.concatenate([np.random.default_rng(3).choice(ny * nx, 4000, replace=False), np.arange(2 * nx),
                                        np.arange((ny - 2) * nx, ny * nx)]))
    z, inc = host_analysis(p, cell, y, L, sel)
    others = [host_analysis(p, cell, y, L, sel, model=mdl) for mdl in (GAUSSIAN, GC)]
    for a in (z, inc, sel, *[b for pair in others for b in pair]):
        a.setflags(write=False)
    return p, cell, y, L, sel, z, inc, others


@pytest.mark.parametrize("envelope", ["1", "0"])
@pytest.mark.parametrize("name", list(CASES))
def test_analysis_against_float64_host_solve(ctx, monkeypatch, name, envelope):
    """The project's dense tolerances; the Gaussian's and Gaspari-Cohn's float64 answers lie more than 100 x these tolerances
    away, so a kernel that evaluates the wrong model cannot pass."""
    p, cell, y, L, sel, zr, inc_ref, others = _case(name)
    if name.startswith("360"):
        assert y.size == 2972
    scale = np.abs(p.Xa).max()
    for zo, inco in others:
        assert np.abs(zo - zr).max() / np.abs(zr).max() > 100 * 2e-5 and np.abs(inco - inc_ref).max() / scale > 100 * 1e-5
    monkeypatch.setenv("OISAT_ENVELOPE", envelope)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    try:
        resid = plan.run(L, corr=SOAR, refine=2, check_pd=True, want_resid=True)
        xa, inc = plan.download()
        z = plan.download_z()
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    ez = np.abs(z - zr).max() / np.abs(zr).max()
    ei = np.abs(inc.ravel()[sel].astype(np.float64) - inc_ref).max() / scale
    ex = np.abs(xa.ravel()[sel].astype(np.float64) - (p.Xa.ravel()[sel] + inc_ref)).max() / scale
    print(f"{name} envelope={envelope}: residuals {resid}, z {ez:.3e}, inc {ei:.3e}, xa {ex:.3e} against the host solve")
    assert resid[-1] <= dense.REFINE_TOL, resid
    assert ez <= 2e-5 and ei <= 1e-5 and ex <= 1e-5


# ---- 3. no state leaks -----------------------------------------------------------------------------------------------------------
def test_no_state_leaks_between_models(ctx, monkeypatch):
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    p, cell, y, _, _, _, _, _ = _case("72x144_L300")
    L = 300.0

    def make():
        plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
        plan.load_background(p.Xa, p.Sa)
        plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
        return plan

    def run(plan, corr):
        plan.run(L, refine=2, check_pd=True, corr=corr)
        xa, inc = plan.download()
        return xa.copy(), inc.copy(), plan.download_z().copy()

    plan = make()
    try:
        first = run(plan, GAUSSIAN)
        soar = run(plan, SOAR)
        gc = run(plan, GC)
        again = run(plan, GAUSSIAN)
        fresh = run(make(), GAUSSIAN)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    assert not np.array_equal(soar[1], first[1]) and not np.array_equal(soar[1], gc[1])
    for a, b, c in zip(first, again, fresh):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert tuple(ctx.solve_status(clear=True))[:3] == (0, 0, 0)


# ---- 4. the float64 sums: latitude window against the full sum -------------------------------------------------------------------
@pytest.mark.parametrize("L", [100.0, 500.0])
def test_latitude_window_equals_the_full_sum(ctx, L):
    """The inputs of tests/test_gpu_parity.py's test of the same name under SOAR.  Dropping every pair beyond the 2^-52 chord
    changes these sums by 6e-16 of the largest entry (host): 1e-13 has more than 100-fold room.  Against NumPy: exp2_neg is good
    to 2e-10 per term and max sum|term| / max|inc| over the field is at most 10 (asserted on the host; 4.9 and 9.6 here)."""
    lib = ctx.lib
    rng = np.random.default_rng(31)
    lat2, lon2 = syn.global_grid(90, 180)
    n = lat2.size
    m = 3000
    olat = np.concatenate([rng.uniform(-90, 90, m - 40), np.full(10, 89.9), np.full(10, -89.9), rng.uniform(-5, 5, 20)])
    olon = np.concatenate([rng.uniform(-180, 180, m - 20), np.tile([179.99, -179.99], 10)])
    order = np.argsort(olat, kind="stable")
    olat, olon = olat[order], olon[order]
    g = dense.decay_constant(L)
    h_gsig, h_osig, h_ovar = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m), rng.uniform(0.1, 1.0, m)
    h_z, h_d = rng.normal(size=m), rng.normal(size=m)
    po = dense.unit_vectors(olat, olon)
    gxyz, gsig, glat = ctx.upload(dense.unit_vectors(lat2, lon2)), ctx.upload(h_gsig), ctx.upload(lat2.ravel())
    oxyz, osig, ovar = ctx.upload(po), ctx.upload(h_osig), ctx.upload(h_ovar)
    z, d, olat_b = ctx.upload(h_z), ctx.upload(h_d), ctx.upload(olat)
    xb = ctx.upload(rng.uniform(1, 5, n))
    chord = C.c_double(0.0)
    assert lib.oisat_corr_cut_chord(KIND, C.c_double(g), C.c_double(52.0), C.byref(chord)) == 0
    d2oo = chord2(po, po)
    beyond = (d2oo > chord.value ** 2).mean()
    print(f"L = {L:g}: {100 * beyond:.0f} % of the observation pairs lie beyond the 2^-52 chord {chord.value:.3f}")
    if L == 100.0:
        assert beyond > 0.0                                     # (something is really dropped)
    outs = []
    ctx.check(lib.oisat_set_correlation(ctx.h, KIND))
    try:
        for win in (False, True):
            inc = ctx.alloc(n * 8)
            r = ctx.alloc(m * 8)
            ctx.check(lib.oisat_apply_increment(ctx.h, _hip.F64, gxyz.ptr, gsig.ptr, n, oxyz.ptr, osig.ptr, z.ptr, m, g, xb.ptr, None,
                                                inc.ptr, glat.ptr if win else None, olat_b.ptr if win else None))
            ctx.check(lib.oisat_cov_residual(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, g, d.ptr, z.ptr, r.ptr, olat_b.ptr if win else None))
            outs.append((ctx.download(inc.ptr, (n,), np.float64), ctx.download(r.ptr, (m,), np.float64)))
    finally:
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
    (inc0, r0), (inc1, r1) = outs
    assert np.abs(inc0).max() > 0
    e_inc, e_r = np.abs(inc1 - inc0).max() / np.abs(inc0).max(), np.abs(r1 - r0).max() / np.abs(r0).max()
    print(f"L = {L:g}: window against full sum: increment {e_inc:.3e}, residual {e_r:.3e} of the largest entry")
    assert e_inc <= 1e-13 and e_r <= 1e-13
    # against float64 NumPy contractions of every pair
    pg = dense.unit_vectors(lat2, lon2)
    full, absum = np.empty(n), np.empty(n)
    for i0 in range(0, n, 2048):                                # every cell on the host: the sum and the sum of |term|
        terms = h_gsig[i0:i0 + 2048, None] * corr_ref(pg[:, i0:i0 + 2048], po, L) * (h_osig * h_z)[None, :]
        full[i0:i0 + 2048], absum[i0:i0 + 2048] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    want = full[::37]
    cancel = absum.max() / np.abs(full).max()
    e_np = np.abs(inc1[::37] - want).max() / np.abs(want).max()
    s = np.sqrt(2.0 * g * d2oo)
    r_ref = h_d - (h_osig * ((((1.0 + s) * np.exp(-s)) * h_osig[None, :]) @ h_z) + h_ovar * h_z)
    e_rnp = np.abs(r1 - r_ref).max() / np.abs(r_ref).max()
    print(f"L = {L:g}: against NumPy: increment {e_np:.3e} (max sum|term| / max|inc| = {cancel:.2f}), residual {e_rnp:.3e}")
    assert cancel <= 10.0
    assert e_np <= 1e-8
    assert e_rnp <= 1e-11                                       # (the bound of the residual tests of tests/test_gpu_dag.py)


# ---- 5. batched and tiled ------------------------------------------------------------------------------------------------------
def test_tiled_and_batched(ctx, monkeypatch):
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    monkeypatch.delenv("OISAT_DAG_SOLVE", raising=False)
    ny, nx, L, tile = 72, 144, 300.0, 60.0
    c = syn.diag_case(ny, nx, 2000, 4242)
    halo = dense.SOAR_HALO_PER_L * L
    assert halo == pytest.approx(6.5172 * L, rel=1e-4)
    halos = []
    real_partition = dense.tile_partition

    def recording(lat2, lon2, olat, olon, tile_deg=30.0, halo_km=900.0, merge_polar=True):
        halos.append(halo_km)
        return real_partition(lat2, lon2, olat, olon, tile_deg, halo_km, merge_polar)

    monkeypatch.setattr(dense, "tile_partition", recording)
    try:
        xa1, inc1, info = dense.OI_tiled(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, tile_deg=tile, dtype=np.float32, corr=SOAR)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))          # (lane 0 of a pool is the process-wide handle)
    monkeypatch.setattr(dense, "tile_partition", real_partition)
    assert halos == [halo]
    # every tile against a host float64 solve of its own system
    Y = np.where(c.Y < 0, 0.0, c.Y)
    cells = info["cells"]
    olat, olon = c.lat.ravel()[cells], c.lon.ravel()[cells]
    sb = np.sqrt(c.Sa.ravel())
    d = Y.ravel()[cells] - c.Xa.ravel()[cells]
    tiles = dense.tile_partition(c.lat, c.lon, olat, olon, tile, halo)
    assert len(tiles) == info["tiles"]
    inc_ref = np.zeros((ny, nx))
    for t in tiles:
        (y0, y1), (x0, x1) = t["rows"], t["cols"]
        o = t["obs"]
        po = dense.unit_vectors(olat[o], olon[o])
        so = sb[cells[o]]
        S = corr_ref(po, po, L) * so[:, None] * so[None, :]
        S[np.diag_indices_from(S)] += c.So.ravel()[cells[o]]
        z = sla.cho_solve(sla.cho_factor(S, lower=True), d[o])
        pg = dense.unit_vectors(c.lat[y0:y1, x0:x1], c.lon[y0:y1, x0:x1])
        inc_ref[y0:y1, x0:x1] = (np.sqrt(c.Sa[y0:y1, x0:x1]).ravel() * (corr_ref(pg, po, L) @ (so * z))).reshape(y1 - y0, x1 - x0)
    scale = np.abs(c.Xa).max()
    ei = np.abs(inc1 - inc_ref).max() / scale
    ex = np.abs(xa1 - (c.Xa + inc_ref)).max() / scale
    print(f"tiled SOAR: {len(tiles)} tiles, inc {ei:.3e}, xa {ex:.3e} against the per-tile host solves")
    assert ei <= 1e-5 and ex <= 1e-5
    # the one-launch analysis is Gaussian only: asked for, the batch takes the two calls -- the same bits
    monkeypatch.setenv("OISAT_DAG_SOLVE", "1")
    try:
        xa2, inc2, _ = dense.OI_tiled(c.Xa, c.Y.copy(), c.Sa, c.So, c.lat, c.lon, L, tile_deg=tile, dtype=np.float32, corr=SOAR)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    monkeypatch.delenv("OISAT_DAG_SOLVE")
    assert np.array_equal(xa1, xa2) and np.array_equal(inc1, inc2)
    xa_f = np.where(np.isfinite(c.Xa), c.Xa, 0.0)
    for batched in (False, True):
        ta = dense.TiledAnalysis(c.lat, c.lon, tile_deg=tile, halo_km=halo, dtype=np.float32, batched=batched)
        try:
            ta.load(xa_f, c.Sa, olat, olon, c.Y.ravel()[cells], c.So.ravel()[cells])
            ta.run(L, refine=2, check_pd=True, corr=SOAR)
            xa3, inc3 = ta.download()
            if batched:                                        # a direct call of the one-launch analysis under SOAR
                bctx, bid = ta.factor.ctxs[0], ta.factor.ids[0]
                bctx.check(bctx.lib.oisat_set_correlation(bctx.h, KIND))
                rc = bctx.lib.oisat_batch_analyse(bctx.h, bid, _hip.F32, dense.decay_constant(L), 2, None)
                assert rc == -1 and b"Gaussian only" in bctx.lib.oisat_last_error()       # OISAT_EINVAL
                bctx.check(bctx.lib.oisat_set_correlation(bctx.h, 0))
        finally:
            ta.close()
            ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))      # (lane 0 of a pool is the process-wide handle)
        e = max(np.abs(inc3 - inc_ref).max(), np.abs(xa3 - (c.Xa + inc_ref)).max()) / scale
        print(f"batched={batched} against the per-tile host solves: {e:.3e}")
        assert e <= 1e-5


# ---- 6. diagnostics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx,m,L", [(36, 72, 300, 800.0), (45, 90, 1100, 500.0)])
def test_posterior_error_and_gain_diag(ctx, ny, nx, m, L):
    """The tolerances of test_dense_posterior_error_and_gain_diag (tests/test_gpu_parity.py) against the float64 formulas."""
    p = syn.point_obs_case(ny, nx, m, 900 + m)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    sb = np.sqrt(p.Sa.ravel())
    po, pg = dense.unit_vectors(p.obs_lat, p.obs_lon), dense.unit_vectors(p.lat, p.lon)
    so = sb[cell]
    S = corr_ref(po, po, L) * so[:, None] * so[None, :]
    S[np.diag_indices_from(S)] += p.obs_var
    Lf = sla.cholesky(S, lower=True)
    V = sla.solve_triangular(Lf, (corr_ref(pg, po, L) * sb[:, None] * so[None, :]).T, lower=True)
    err_ref = np.sqrt(np.maximum(sb ** 2 - (V * V).sum(axis=0), 0.0))
    Linv = sla.solve_triangular(Lf, np.eye(m), lower=True)
    ak_ref = 1.0 - p.obs_var * (Linv * Linv).sum(axis=0)
    try:
        xb, inc, info = dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, L, refine=2, dtype=np.float32, want_error=True,
                                       obs=dict(lat=p.obs_lat, lon=p.obs_lon, y=p.obs_y, var=p.obs_var), corr=SOAR)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    sig = np.sqrt(p.Sa).max()
    e = np.abs(info["err"].ravel() - err_ref).max() / sig
    print(f"{ny}x{nx} m={m}: err {e:.3e} of sig, ak_obs {np.abs(info['ak_obs'] - ak_ref).max():.3e}")
    assert e <= 2e-3
    np.testing.assert_allclose(info["ak_obs"], ak_ref, atol=2e-5, rtol=0)
    assert (info["err"] <= np.sqrt(p.Sa) * (1 + 1e-6)).all()


# ---- 7. the driver -------------------------------------------------------------------------------------------------------------
def test_driver_takes_the_model(ctx, monkeypatch):
    """``oi_correlation = "soar"`` through the facade: the four attributes are what ``OI_dense(corr="soar")`` gives at the
    knee-picked scale under the reference's mask (NaN where unobserved), and the analysis is SOAR's (float64 host solve)."""
    from oisatgmi.driver import oisatgmi
    for v in ("OISAT_OI_MODE", "OISAT_CORRELATION", "OISAT_CORR_LENGTH_KM", "OISAT_UNOBSERVED", "OISAT_OI_ERROR"):
        monkeypatch.delenv(v, raising=False)
    L = 600.0
    c = syn.diag_case(36, 72, 400, 77)
    lat, lon = syn.global_grid(36, 72)
    o = oisatgmi()
    o.ctm_averaged_vcd, o.sat_averaged_vcd = c.Xa.copy(), c.Y.copy()
    o.sat_averaged_error = np.sqrt(c.So)
    o.grid_lat, o.grid_lon = lat, lon
    o.oi_mode, o.corr_length_km, o.oi_correlation = "dense", L, "soar"
    try:
        o.oi("OMI", error_ctm=50.0)
        assert o.oi_info["correlation"] == "soar" and o.oi_info["mode"] == "dense"
        s = o.oi_info["scale"]
        Sa, So = (c.Xa * 50.0 / 100.0) ** 2, np.sqrt(c.So) ** 2
        xb, inc, info = dense.OI_dense(c.Xa.copy(), c.Y.copy(), Sa, So, lat, lon, L, scale=s, want_error=True, corr=SOAR)
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    Y = np.where(c.Y < 0, 0.0, c.Y)
    observed = np.isfinite(Y) & ~np.isnan(So) & np.isfinite(c.Xa) & np.isfinite(Sa)
    assert observed.any() and not observed.all()
    want = [np.array(a, dtype=np.float64) for a in (xb, info["ak"], inc, info["err"])]
    want[1][observed & np.isinf(So)] = 0.0
    want[1][observed & (Sa * s == 0)] = np.nan
    for a in want:
        a[~observed] = np.nan
    for got, w in zip((o.ctm_averaged_vcd_corrected, o.ak_OI, o.increment_OI, o.error_OI), want):
        np.testing.assert_array_equal(got, w)
    cell = np.flatnonzero(observed.ravel())
    sb = np.sqrt(s * Sa.ravel())
    po = dense.unit_vectors(lat.ravel()[cell], lon.ravel()[cell])
    S = corr_ref(po, po, L) * sb[cell][:, None] * sb[cell][None, :]
    S[np.diag_indices_from(S)] += So.ravel()[cell]
    z = sla.cho_solve(sla.cho_factor(S, lower=True), Y.ravel()[cell] - c.Xa.ravel()[cell])
    inc_ref = sb[cell] * (corr_ref(po, po, L) @ (sb[cell] * z))
    e = np.abs(o.increment_OI.ravel()[cell] - inc_ref).max() / np.abs(c.Xa).max()
    print(f"driver, SOAR: increment at the observed cells {e:.3e} of max |Xa| against the host solve")
    assert e <= 1e-5


# ---- 8. the residual on compact blocks of rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", ["box", "globe"])
def test_residual_on_compact_blocks(ctx, region):
    """``oisat_cov_residual`` behind ``oisat_set_obs_blocks`` under SOAR at L = 60 km, where the compact blocks pay (2^-52 chord
    0.374 <= 0.5): against the plain form and against the float64 contraction, with the tolerances of the Gaussian's test
    (tests/test_gpu_dag.py): the same terms per row up to terms below 2^-52 of a term."""
    lib = ctx.lib
    m, L = 3000, 60.0
    rng = np.random.default_rng(m)
    if region == "box":
        lat, lon = rng.uniform(-28.0, 33.0, m), rng.uniform(92.0, 168.0, m)
    else:
        lat, lon = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, m))), rng.uniform(-180.0, 180.0, m)
    o = np.argsort(lat, kind="stable")
    lat, lon = lat[o], lon[o]
    po = dense.unit_vectors(lat, lon)
    sig, var = rng.uniform(0.5, 1.5, m), rng.uniform(0.1, 0.3, m)
    zz, dd = rng.normal(size=m), rng.normal(size=m)
    oxyz, osig, ovar, z, d = ctx.upload(po), ctx.upload(sig), ctx.upload(var), ctx.upload(zz), ctx.upload(dd)
    olat = ctx.upload(lat.astype(np.float64))
    perm = ctx.upload(dense.morton_order(lat, lon))
    g = dense.decay_constant(L)
    chord = C.c_double(0.0)
    assert lib.oisat_corr_cut_chord(KIND, C.c_double(g), C.c_double(52.0), C.byref(chord)) == 0 and chord.value <= 0.5
    outs = []
    ctx.check(lib.oisat_set_correlation(ctx.h, KIND))
    try:
        for blocks in (False, True):
            r = ctx.alloc(m * 8)
            ctx.check(lib.oisat_set_obs_blocks(ctx.h, perm.ptr if blocks else None, m if blocks else 0))
            ctx.check(lib.oisat_cov_residual(ctx.h, oxyz.ptr, osig.ptr, ovar.ptr, m, g, d.ptr, z.ptr, r.ptr, olat.ptr))
            outs.append(ctx.download(r.ptr, (m,), np.float64))
    finally:
        ctx.check(lib.oisat_set_obs_blocks(ctx.h, None, 0))
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
    ref = dd - (sig * ((corr_ref(po, po, L) * sig[None, :]) @ zz) + var * zz)
    scale = np.abs(ref).max()
    e_b, e_r = np.abs(outs[1] - outs[0]).max() / scale, np.abs(outs[1] - ref).max() / scale
    print(f"{region}: compact blocks against plain rows {e_b:.3e}, against NumPy {e_r:.3e}")
    assert not np.array_equal(outs[1], outs[0])                 # (another order of the sums: the compact form really ran)
    assert e_b <= 1e-12 and e_r <= 1e-11
