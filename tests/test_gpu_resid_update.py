"""The refinement's verification residual as an fp32 update of the last one (``oisat_cov_residual_update``, and the path of
``oisat_gain_solve`` that accepts it): the entry point against a float64 host evaluation of r_prev - S dz, the whole analysis
with the path on against ``OISAT_RESID_UPDATE=0``, the rounds where the update does not prove the tolerance (the float64
residual decides: every bit as without the path), and the models / forms it does not apply to.

The bound everywhere is c = ``dense.RESID_UPDATE_C`` = 2^-10 (OISAT_RESID_UPDATE_C, include/oisat.h) times the 2-norm of the
previous residual: 8 x the largest |t - r| / |r_prev| measured on the MI355X over the protocol's four months and the geometries
below, rounded up to a power of two (profiles/resid_update.json)."""
import functools

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
C_UPD = dense.RESID_UPDATE_C
L300 = 300.0


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))
    c.prof_enable(False)


# ---- 1. the entry point ----------------------------------------------------------------------------------------------------
def _points(name):
    """(lat, lon) of a geometry, unsorted."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("m"):                                   # ragged blocks: a 20 x 30 degree box, L = 2.7 degrees
        m = int(name[1:])
        return rng.uniform(20.0, 40.0, m), rng.uniform(0.0, 30.0, m)
    if name == "disc":                                         # 1 700 observations within 1 degree: every block's list holds them
        r, a = 1.0 * np.sqrt(rng.uniform(0.0, 1.0, 1700)), rng.uniform(0.0, 2 * np.pi, 1700)      # all: 1 700 > 1 280, a flush
        return 10.0 + r * np.sin(a), 50.0 + r * np.cos(a)
    if name == "polar":                                        # the window (23 degrees at L = 300 km) runs past the pole
        return 90.0 - 6.0 * np.sqrt(rng.uniform(0.0, 1.0, 500)), rng.uniform(-180.0, 180.0, 500)
    raise KeyError(name)


GEOMETRIES = ["m1", "m63", "m64", "m65", "m257", "disc", "polar"]


@functools.lru_cache(maxsize=None)
def _abi_case(name):
    """Inputs in ascending-latitude order and the float64 reference r_prev - (sig_i sum_j C_ij sig_j dz_j + var_i dz_i) over
    EVERY pair.  dz: standard normal (both signs); r_prev: standard normal scaled to |S dz|, the relation a correction of the
    refinement leaves (|S dz| ~ |r_prev|) and the one the bound c |r_prev| is stated for."""
    lat, lon = _points(name)
    o = dense.latitude_order(lat)
    lat, lon = np.ascontiguousarray(lat[o]), np.ascontiguousarray(lon[o])
    m = lat.size
    rng = np.random.default_rng(77 + m)
    xyz = dense.unit_vectors(lat, lon)
    sig, var = rng.uniform(0.5, 1.5, m), rng.uniform(0.1, 1.0, m)
    dz = rng.standard_normal(m)
    g = dense.decay_constant(L300)
    d2 = np.zeros((m, m))
    for k in range(3):
        d2 += (xyz[k][:, None] - xyz[k][None, :]) ** 2
    sdz = sig * (np.exp(-g * d2) @ (sig * dz)) + var * dz
    r_prev = rng.standard_normal(m)
    r_prev *= np.linalg.norm(sdz) / np.linalg.norm(r_prev)
    want = r_prev - sdz
    perm = dense.morton_order(lat, lon)
    out = dict(lat=lat, xyz=xyz, sig=sig, var=var, dz=dz, r_prev=r_prev, want=want, perm=perm, g=g, m=m)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _update(ctx, c, dev, with_perm=True):
    lib = ctx.lib
    out = ctx.alloc(c["m"] * 8)
    ctx.check(lib.oisat_memset(ctx.h, out.ptr, 0xFF, c["m"] * 8))
    if with_perm:
        ctx.check(lib.oisat_set_obs_blocks(ctx.h, dev["perm"].ptr, c["m"]))
    ctx.check(lib.oisat_cov_residual_update(ctx.h, dev["xyz"].ptr, dev["sig"].ptr, dev["var"].ptr, c["m"], c["g"], dev["r_prev"].ptr,
                                            dev["dz"].ptr, out.ptr, dev["lat"].ptr))
    ctx.sync()
    return ctx.download(out.ptr, (c["m"],), np.float64)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_entry_point_against_float64_host_evaluation(ctx, name):
    """max |t - (r_prev - S dz)| <= c |r_prev|_2, not zero (the fp32 path is live), and two calls give the same bits."""
    c = _abi_case(name)
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    dev = {k: ctx.upload(c[k]) for k in ("lat", "xyz", "sig", "var", "dz", "r_prev", "perm")}
    got = _update(ctx, c, dev)
    again = _update(ctx, c, dev)
    err = np.abs(got - c["want"]).max()
    rn = np.linalg.norm(c["r_prev"])
    print(f"{name}: m = {c['m']}, max |t - r| / |r_prev| = {err / rn:.3e}, |t - r|_2 / |r_prev| = "
          f"{np.linalg.norm(got - c['want']) / rn:.3e} (c = {C_UPD:.3e})")
    assert np.isfinite(got).all()
    assert err <= C_UPD * rn
    assert err > 0.0
    assert np.array_equal(got, again)
    if name == "m257":                                         # without a list: 64 consecutive latitudes per block, the same sums
        plain = _update(ctx, c, dev, with_perm=False)
        assert np.abs(plain - c["want"]).max() <= C_UPD * rn


def test_entry_point_refuses_what_it_does_not_cover(ctx):
    """Another model, or a covariance whose reach is too long for compact blocks (L = 500 km): an error, nothing launched."""
    c = _abi_case("m65")
    dev = {k: ctx.upload(c[k]) for k in ("lat", "xyz", "sig", "var", "dz", "r_prev", "perm")}
    out = ctx.alloc(c["m"] * 8)
    lib = ctx.lib

    def call(g):
        return lib.oisat_cov_residual_update(ctx.h, dev["xyz"].ptr, dev["sig"].ptr, dev["var"].ptr, c["m"], g, dev["r_prev"].ptr,
                                             dev["dz"].ptr, out.ptr, dev["lat"].ptr)
    try:
        for kind in (dense.corr_kind("gaspari_cohn"), dense.corr_kind("soar")):
            ctx.check(lib.oisat_set_correlation(ctx.h, kind))
            assert call(c["g"]) != 0
    finally:
        ctx.check(lib.oisat_set_correlation(ctx.h, 0))
    assert call(dense.decay_constant(500.0)) != 0
    assert call(c["g"]) == 0
    ctx.sync()


# ---- 2. the whole analysis ------------------------------------------------------------------------------------------------
CASES = {"360x720_swaths": (360, 720, 3000, 9000, True), "72x144": (72, 144, 1000, 7000, False),
         "round4": (72, 144, 1500, 9401, False)}


@functools.lru_cache(maxsize=None)
def _case(name):
    ny, nx, nobs, seed, swaths = CASES[name]
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    y = np.where(p.obs_y < 0, 0, p.obs_y)
    return p, cell, y


def _analysis(ctx, monkeypatch, name, L, switch, **kw):
    """One run with the launch profile: (residuals, z, xa, inc, status, profile)."""
    p, cell, y = _case(name)
    if switch is None:
        monkeypatch.delenv("OISAT_RESID_UPDATE", raising=False)
    else:
        monkeypatch.setenv("OISAT_RESID_UPDATE", switch)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    ctx.solve_status(clear=True)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        resid = plan.run(L, want_resid=True, **kw)
        ctx.sync()
        prof = ctx.prof_collect()
    finally:
        ctx.prof_enable(False)
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    st = ctx.solve_status(clear=True)
    xa, inc = plan.download()
    return resid, plan.download_z(), xa, inc, st, prof


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("tol", [None, 1e-8])
@pytest.mark.parametrize("name", ["360x720_swaths", "72x144"])
def test_analysis_with_the_update_against_the_switch_off(ctx, monkeypatch, name, tol):
    """refine = 2 at L = 300 km.  z and the fields do not depend on the update; the first residual is the float64 one, bit for
    bit; the last ones meet the tolerance and differ by at most c times the first.
    tol = None, the default 1e-6: both systems meet it with their FIRST residual (9.7e-7 and 3.4e-7 on the MI355X), no correction
    is made and every update launch returns at once -- the residual lists are identical.  tol = 1e-8 makes the same two systems
    take one correction, whose residual (6e-12, 6e-13) is then accepted in its update form: c |r_0| < 1e-9 leaves the proof an
    order of magnitude of room.  Launches there (a converged round's are no-ops of microseconds, so the TIME tells the real
    ones): the update is launched in rounds 1 and 2 (round 2 returns at once), cov_residual as often as without the path, but
    only ONE of them evaluates where the off run has two -- its total falls below 0.8 of the off run's (0.5 plus the no-ops is
    expected)."""
    on = _analysis(ctx, monkeypatch, name, L300, None, refine=2, tol=tol)
    off = _analysis(ctx, monkeypatch, name, L300, "0", refine=2, tol=tol)
    print(f"{name} tol {tol}: residuals on {on[0]}, off {off[0]}")
    print(f"{name} tol {tol}: profile on  { {k: v for k, v in on[5].items() if 'resid' in k} }")
    print(f"{name} tol {tol}: profile off { {k: v for k, v in off[5].items() if 'resid' in k} }")
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert on[4] == off[4] and on[4].clean
    assert _same_bits(on[0][0], off[0][0])
    assert on[0][-1] <= dense.REFINE_TOL and off[0][-1] <= dense.REFINE_TOL
    assert abs(on[0][-1] - off[0][-1]) <= C_UPD * on[0][0]
    assert "cov_residual_update" not in off[5] and "resid_update_check" not in off[5]
    assert on[5]["cov_residual_update"]["launches"] == 2 and on[5]["resid_update_check"]["launches"] == 2
    assert on[5]["cov_residual"]["launches"] == off[5]["cov_residual"]["launches"] == 3
    if tol is None:
        assert on[0][0] <= dense.REFINE_TOL and _same_bits(on[0], off[0])
        return
    assert on[0][0] > tol >= on[0][-1] and off[0][-1] <= tol
    assert on[0][1] != off[0][1]                               # (the accepted update's norm, not the float64 one: the path ran)
    assert on[5]["cov_residual"]["total_ms"] < 0.8 * off[5]["cov_residual"]["total_ms"]


# ---- 3. not accepted: the float64 residual decides -------------------------------------------------------------------------
@pytest.mark.parametrize("L,kw", [(500.0, dict(refine=4, tol=1e-12)), (500.0, dict(refine=1, tol=0.0)),
                                  (L300, dict(refine=1, tol=1e-12)), (L300, dict(refine=1, tol=0.0)),
                                  (L300, dict(refine=2, tol=0.0))])
def test_rounds_the_update_does_not_accept_keep_every_bit(ctx, monkeypatch, L, kw):
    """The system of test_gpu_round4.py's status test, at its L = 500 km and at 300 km.  tol = 1e-12 with one correction: the
    update cannot accept, because c times the first residual alone is above the tolerance (asserted); tol = 0 never accepts --
    it has no tolerance to prove, and the update is not even launched.  z, the residual list and the status words are those of
    the off run, bit for bit."""
    on = _analysis(ctx, monkeypatch, "round4", L, None, **kw)
    off = _analysis(ctx, monkeypatch, "round4", L, "0", **kw)
    print(f"L = {L:g} {kw}: residuals {on[0]}, status {on[4]}, update launches "
          f"{on[5].get('cov_residual_update', {}).get('launches', 0)}")
    if kw["tol"] > 0.0 and kw["refine"] == 1:
        assert C_UPD * on[0][0] > kw["tol"]
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert _same_bits(on[0], off[0])
    assert on[4] == off[4]
    if kw["tol"] == 0.0 or L == 500.0:
        assert "cov_residual_update" not in on[5]
    else:
        assert on[5]["cov_residual_update"]["launches"] == kw["refine"]
    assert on[5]["cov_residual"]["launches"] == off[5]["cov_residual"]["launches"]


def test_a_tight_tolerance_over_many_rounds_keeps_z(ctx, monkeypatch):
    """refine = 4, tol = 1e-12 at L = 300 km: whichever round the update proves the tolerance in, the float64 test would have
    passed there too -- z is the off run's, and each reported residual is within c times the one before it of the off run's."""
    on = _analysis(ctx, monkeypatch, "round4", L300, None, refine=4, tol=1e-12)
    off = _analysis(ctx, monkeypatch, "round4", L300, "0", refine=4, tol=1e-12)
    print(f"residuals on {on[0]}, off {off[0]}")
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert on[4] == off[4]
    assert _same_bits(on[0][0], off[0][0])
    for k in range(1, 5):
        assert abs(on[0][k] - off[0][k]) <= C_UPD * off[0][k - 1]


# ---- 4. not applicable ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,corr", [(500.0, "gaussian"), (L300, "gaspari_cohn"), (L300, "soar")])
def test_forms_and_models_the_update_does_not_apply_to(ctx, monkeypatch, L, corr):
    """The latitude-row form (L = 500 km) and the other two models: no cov_residual_update launch, every bit as with the
    switch off."""
    on = _analysis(ctx, monkeypatch, "72x144", L, None, refine=2, corr=corr)
    off = _analysis(ctx, monkeypatch, "72x144", L, "0", refine=2, corr=corr)
    assert "cov_residual_update" not in on[5] and "resid_update_check" not in on[5]
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert _same_bits(on[0], off[0]) and on[4] == off[4]
    assert {k: v["launches"] for k, v in on[5].items()} == {k: v["launches"] for k, v in off[5].items()}


def test_the_switch_takes_0_or_1_only(ctx, monkeypatch):
    p, cell, y = _case("72x144")
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=int(y.size), dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, y, p.obs_var)
    monkeypatch.setenv("OISAT_RESID_UPDATE", "yes")
    with pytest.raises(_hip.OisatError, match="OISAT_RESID_UPDATE"):
        plan.run(L300, refine=2)
    ctx.sync()
    ctx.solve_status(clear=True)
    monkeypatch.setenv("OISAT_RESID_UPDATE", "1")
    plan.run(L300, refine=2)
    plan.check()
