"""``oisat_buddy_sums`` at the C ABI against the NumPy restatement of its pair rule (tests/buddy_cases.py: a dense m x m pass,
the correlation from the host-only ``oisat_corr_eval``, sums by ``math.fsum``), then the check through ``dense`` and the driver.

Bounds per row, derived, not measured.  n equal.  |W - ref| <= (n 2^-53 + E) W: n additions in the row's own order, each
rounded once, plus E for the device's correlation against the host's on identical d2; the same for P and Q with
sum |c u_b| and sum |c u_b^2| in W's place (their products are rounded too: counted in E).
  Gaussian, SOAR: E = (8 + 2 |ln cmin|) 2^-52 -- one ulp each for exp, sqrt and the products, and the rounding of the
                  exponential's argument magnified by |argument| <= |ln cmin| (SOAR: s <= 3.4 |ln cmin| at these cuts, but its
                  argument's error is half the Gaussian's: the square root halves it).
  Gaspari-Cohn:   E = 64 2^-52 / cmin -- the cancellation of a fifth-degree polynomial whose terms are at most 32, relative
                  to a value of at least cmin.
Every parity case first asserts (ref_sums) that no used pair has its correlation within 1e-9 relative of cmin."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import buddy_cases as bc
import covariogram_cases as cc
from oisatgmi import _hip, dense, synthetic as syn

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7
MODELS = ("gaussian", "gaspari_cohn", "soar")


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))


def device_sums(ctx, xyz, u, g, cmin, olat=None, m=None, kind=0, null=(), handle=True):
    """-> (rc, n, sums (3, m)); the device outputs start as SENTINEL.  ``null``: names of pointers passed as NULL."""
    m_true = int(np.size(u))
    m = m_true if m is None else m
    rows = max(m_true, 1)
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, kind))
    bufs = {"n": ctx.upload(np.full(rows, SENTINEL, dtype=np.int32)), "sums": ctx.upload(np.full((3, rows), float(SENTINEL)))}
    for k, v in (("xyz", xyz), ("u", u), ("olat", olat)):
        if v is not None and np.size(v):
            bufs[k] = ctx.upload(np.ascontiguousarray(v, dtype=np.float64))
    ptr = {k: (bufs[k].ptr if k in bufs and k not in null else None) for k in ("xyz", "u", "olat", "n", "sums")}
    try:
        rc = ctx.lib.oisat_buddy_sums(ctx.h if handle else None, ptr["xyz"], ptr["u"], m, float(g), float(cmin), ptr["olat"],
                                      ptr["n"], ptr["sums"])
        ctx.sync()
        n = ctx.download(bufs["n"].ptr, (rows,), np.int32)
        sums = ctx.download(bufs["sums"].ptr, (3, rows), np.float64)
    finally:
        for b in bufs.values():
            b.free()
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    return rc, n, sums


def model_budget(corr, cmin):
    if corr == "gaspari_cohn":
        return 64.0 * 2.0 ** -52 / cmin
    return (8.0 + 2.0 * abs(math.log(cmin))) * 2.0 ** -52


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
def polar_cap(rng, m, cap_deg):
    """Unit vectors uniform on a cap of half-angle ``cap_deg`` about the NORTH POLE, ascending z."""
    cz = rng.uniform(np.cos(np.deg2rad(cap_deg)), 1.0, m)
    ph = rng.uniform(0.0, 2.0 * np.pi, m)
    s = np.sqrt(1.0 - cz * cz)
    return bc.by_ascending_z(np.stack([s * np.cos(ph), s * np.sin(ph), cz]))


@functools.lru_cache(maxsize=None)
def geometry(name):
    """-> (xyz in ascending latitude, latitudes in degrees, L_km), read-only."""
    if name.startswith("cap"):
        m = int(name[3:])
        xyz, L = bc.by_ascending_z(cc.cap_points(np.random.default_rng(3000 + m), m, 20.0)), 400.0
    elif name == "twins":                                       # two identical points: d2 = 0, c = 1
        p = cc.cap_points(np.random.default_rng(3002), 1, 20.0)
        xyz, L = np.ascontiguousarray(np.repeat(p, 2, axis=1)), 400.0
    elif name == "global1500":                                  # both poles' neighbourhoods and the date line are inside
        lat, lon = cc.global_points(np.random.default_rng(3003), 1500)
        xyz, L = cc.unit_vectors(lat, lon), 300.0
    elif name == "pole600":
        xyz, L = polar_cap(np.random.default_rng(3004), 600, 3.0), 100.0
    else:
        raise KeyError(name)
    lat = bc.lat_lon_of(xyz)[0]
    assert np.all(np.diff(lat) >= 0)
    xyz.setflags(write=False)
    lat.setflags(write=False)
    return xyz, lat, L


def innovations(m):
    u = np.random.default_rng(4000 + m).normal(size=m)
    if m >= 255:                                                # a few observations that take part in nothing
        u[0], u[m // 2], u[m - 1], u[7] = np.nan, np.inf, -np.inf, np.nan
    return u


@pytest.mark.parametrize("cmin", [bc.CMIN, 0.01], ids=["cmin_e-2", "cmin_0.01"])
@pytest.mark.parametrize("corr", MODELS)
@pytest.mark.parametrize("name", ["twins", "cap255", "cap256", "cap257", "cap513", "cap1500", "global1500", "pole600"])
def test_parity_with_the_numpy_pair_rule(ctx, name, corr, cmin):
    xyz, lat, L = geometry(name)
    m = xyz.shape[1]
    u = innovations(m)
    kind, g = bc.KINDS[corr], bc.decay(L)
    ref = bc.ref_sums(xyz, u, kind, g, cmin)
    rc, n, sums = device_sums(ctx, xyz, u, g, cmin, olat=lat, kind=kind)
    assert rc == 0
    np.testing.assert_array_equal(n, ref["n"])
    E = model_budget(corr, cmin)
    worst = {}
    for k, (got, want, scale) in {"W": (sums[0], ref["W"], ref["W"]), "P": (sums[1], ref["P"], ref["absP"]),
                                  "Q": (sums[2], ref["Q"], ref["absQ"])}.items():
        bound = (ref["n"] * 2.0 ** -53 + E) * scale
        err = np.abs(got - want)
        worst[k] = float(np.max(err / np.where(bound > 0, bound, 1.0)))
        assert np.all(err <= bound), (k, worst[k])
    used = np.isfinite(u)
    print(f"{name} {corr} cmin {cmin:.4f}: buddies per used observation {ref['n'][used].mean():.1f} (max {ref['n'].max()}), "
          f"worst error / bound W {worst['W']:.3f} P {worst['P']:.3f} Q {worst['Q']:.3f}")
    assert not n[~used].any() and not sums[:, ~used].any()      # an unused observation's own outputs are zeros
    if name == "twins":
        assert n.tolist() == [1, 1] and sums[0].tolist() == [1.0, 1.0]
        assert sums[1].tolist() == [u[1], u[0]] and sums[2].tolist() == [u[1] * u[1], u[0] * u[0]]
    elif name == "global1500":
        assert 0 < ref["n"].max() < m // 10                     # the cut does cut, and leaves buddies


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", MODELS)
def test_repetition_and_the_window_change_no_bit(ctx, corr):
    xyz, lat, L = geometry("global1500")
    u = innovations(1500)
    kind, g = bc.KINDS[corr], bc.decay(L)
    chord = C.c_double(0.0)
    assert ctx.lib.oisat_corr_cut_chord(kind, g, -math.log2(bc.CMIN), C.byref(chord)) == 0
    assert chord.value < 1.0                                    # (the window does window: its angle is far below 180 degrees)
    a = device_sums(ctx, xyz, u, g, bc.CMIN, olat=lat, kind=kind)
    b = device_sums(ctx, xyz, u, g, bc.CMIN, olat=lat, kind=kind)
    c = device_sums(ctx, xyz, u, g, bc.CMIN, olat=None, kind=kind)
    assert a[0] == b[0] == c[0] == 0 and a[1].sum() > 0
    for other in (b, c):
        assert a[1].tobytes() == other[1].tobytes() and a[2].tobytes() == other[2].tobytes()


# ---- 3. arguments ------------------------------------------------------------------------------------------------------------------
def untouched(n, sums):
    return bool(np.all(n == SENTINEL) and np.all(sums == float(SENTINEL)))


@pytest.mark.parametrize("g,cmin", [(100.0, 0.0), (100.0, 1.0), (100.0, 2.0 ** -21), (100.0, float("nan")), (100.0, -0.1),
                                    (0.0, 0.1), (-1.0, 0.1), (float("inf"), 0.1), (float("nan"), 0.1)])
def test_bad_values_leave_the_outputs_alone(ctx, g, cmin):
    xyz, lat, _ = geometry("cap255")
    rc, n, sums = device_sums(ctx, xyz, np.ones(255), g, cmin, olat=lat)
    assert rc == EINVAL and untouched(n, sums)


def test_bad_sizes_and_null_pointers(ctx):
    xyz, lat, _ = geometry("cap255")
    u = np.ones(255)
    for m in (-1, (1 << 20) + 1):
        rc, n, sums = device_sums(ctx, xyz, u, 100.0, 0.1, olat=lat, m=m)
        assert rc == EINVAL and untouched(n, sums)
    for null in ("xyz", "u", "n", "sums"):
        rc, n, sums = device_sums(ctx, xyz, u, 100.0, 0.1, olat=lat, null=(null,))
        assert rc == EINVAL and untouched(n, sums), null
    rc, n, sums = device_sums(ctx, xyz, u, 100.0, 0.1, olat=lat, handle=False)
    assert rc == EINVAL and untouched(n, sums)
    rc, n, sums = device_sums(ctx, None, np.empty(0), 100.0, 0.1, m=0)          # m = 0: a no-op, NULL pointers allowed
    assert rc == 0 and untouched(n, sums)
    rc, n, sums = device_sums(ctx, xyz[:, :1], np.array([2.0]), 100.0, 0.1, olat=lat[:1])   # m = 1: zeros
    assert rc == 0 and n.tolist() == [0] and not sums.any()
    rc, n, sums = device_sums(ctx, xyz, u, 100.0, 2.0 ** -20, olat=lat)         # the smallest cmin is allowed
    assert rc == 0 and n.min() >= 0


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------
def test_buddy_check_is_the_numpy_loop(ctx):
    """The planted-outlier recipe, seed 1, through dense.buddy_check against the same loop on the NumPy sums: equal decisions
    and equal passes, after asserting that no decision of the reference lies within 1e-9 relative of its threshold."""
    p, _, u, bad = bc.planted_case(1)
    lat, lon = bc.lat_lon_of(p)
    xyz = cc.unit_vectors(lat, lon)                             # what buddy_check makes of (lat, lon)
    L = bc.PLANTED["L0"]
    rej, reason, passes, margin = bc.ref_buddy_check(xyz, u, 0, bc.decay(L), k_background=np.inf)
    assert margin > 1e-9, "a decision sits on its threshold: choose another seed"
    out = dense.buddy_check(lat, lon, u, L, k_background=np.inf, ctx=ctx)
    print(f"passes {out['passes']}, rejected {int(out['rejected'].sum())}, nearest reference decision {margin:.2e} from its threshold")
    np.testing.assert_array_equal(out["rejected"], rej)
    np.testing.assert_array_equal(out["reason"], reason)
    assert out["passes"] == passes and np.flatnonzero(out["rejected"]).tolist() == bad.tolist()
    assert out["n"].dtype == np.int32 and np.isnan(out["mean"][out["n"] == 0]).all() and out["cmin"] == dense.BUDDY_CMIN
    again = dense.buddy_check(lat, lon, u, L, k_background=np.inf, ctx=ctx)
    assert again["mean"].tobytes() == out["mean"].tobytes() and again["spread"].tobytes() == out["spread"].tobytes()


def driver_case():
    """36 x 72 grid, a fully observed block of 20 x 20 cells with innovations of 0.5 standard deviations, five of them planted at
    10; the prior-error scaling is forced (reg_index) so that the standard deviations are known."""
    from oisatgmi import optimal_interpolation as oi_mod
    reg_index = 9                                               # (scale 1.0 to rounding)
    scale = float(oi_mod.scaling_factors(True)[reg_index])
    rng = np.random.default_rng(515)
    lat, lon = syn.global_grid(36, 72)
    xa = syn.background_field(rng, lat, lon)
    Sa = (0.5 * xa) ** 2
    So = np.full(xa.shape, np.nan)
    y = np.full(xa.shape, np.nan)
    blk = (slice(8, 28), slice(20, 40))
    So[blk] = rng.uniform(0.05, 0.2, (20, 20)) ** 2
    sd = np.sqrt(Sa * scale + So)
    y[blk] = (xa + 0.5 * sd * rng.normal(size=xa.shape))[blk]
    planted = [(10, 23), (14, 31), (19, 26), (23, 36), (25, 22)]
    for i, j in planted:
        y[i, j] = xa[i, j] + 10.0 * sd[i, j]
    y[y < 0] = 0.0                                              # the driver's clamp, done by oi() before _oi_spatial
    return lat, lon, xa, y, Sa, So, reg_index, planted


def test_driver_qc(ctx):
    from oisatgmi.driver import oisatgmi
    lat, lon, xa, y, Sa, So, reg_index, planted = driver_case()
    assert int(np.isfinite(y).sum()) == 400
    y0 = y.copy()

    def run(**kw):
        return oisatgmi._oi_spatial("dense", xa, y, Sa, So, lat, lon, 500.0, 30.0, "nan", reg_index, False, corr="gaussian", **kw)

    plain, plain_info = run()
    off, off_info = run(qc=None)
    qc, qc_info = run(qc={"k_buddy": 3.0})
    np.testing.assert_array_equal(y, y0)                        # the caller's y: nothing beyond the clamp (already applied)
    assert sorted(off_info) == sorted(plain_info) and "qc" not in off_info and "qc_rejected" not in off_info
    for a, b in zip(plain, off):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    mask, info = qc_info["qc_rejected"], qc_info["qc"]
    print("driver qc:", info)
    assert mask.shape == xa.shape and mask.dtype == bool and all(mask[i, j] for i, j in planted)
    assert not mask[~np.isfinite(y)].any()
    assert sorted(info) == sorted(["method", "nrejected", "n_background", "n_buddy", "passes", "k_background", "k_buddy",
                                   "min_buddies", "cmin", "L_km"])
    assert info["method"] == "buddy" and info["nrejected"] == int(mask.sum()) == info["n_background"] + info["n_buddy"]
    assert info["L_km"] == 500.0 and info["k_buddy"] == 3.0 and sum(info["passes"]) == info["nrejected"]
    inc_off, inc_qc = off[2], qc[2]
    for i, j in planted:
        assert np.isnan(inc_qc[i, j]) and np.isfinite(inc_off[i, j])            # unobserved under "nan": NaN in the outputs
        nb = [(i + di, j + dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di or dj) and not mask[i + di, j + dj]]
        assert nb and all(np.isfinite(inc_qc[c]) and inc_qc[c] != inc_off[c] for c in nb)
