"""``oisat_superob`` at the C ABI against the NumPy restatement of tests/superob_cases.py: box ids, counts and every sum must be
the SAME BITS (the sums are exact integers scaled by a power of two; the restatement adds the same integers in int64), for
any order of the observations and any run.  Apart from the deliberate points on band edges and longitude seams, every recipe
keeps its observations at least 1e-9 degrees from a box edge, asserted on the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import superob_cases as sc
from oisatgmi import _hip, dense

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    return c


def device_superob(ctx, o, box_deg, with_sums=True, m=None, table=None, null=()):
    """-> (rc, box int32[m], count int64[nbox], sums float64[8][nbox] or None, nused); every output starts as SENTINEL."""
    n, offset, nbox = table if table is not None else sc.box_table(box_deg)
    n, offset = np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(offset, dtype=np.int64)
    mm = int(np.size(o["d"])) if m is None else int(m)
    have = max(int(np.size(o["d"])), 1)
    xyz = sc.unit_vectors(o["lat"], o["lon"]) if np.size(o["d"]) else np.zeros((3, 1))
    bufs = {k: ctx.upload(np.ascontiguousarray(v, dtype=np.float64) if np.size(v) else np.zeros(1))
            for k, v in (("lat", o["lat"]), ("lon", o["lon"]), ("xyz", xyz), ("d", o["d"]), ("sig", o["sig"]), ("var", o["var"]))}
    bufs["box"] = ctx.upload(np.full(have, SENTINEL, dtype=np.int32))
    ptr = {k: (None if k in null else b.ptr) for k, b in bufs.items()}
    count = np.full(max(nbox, 1), SENTINEL, dtype=np.int64)
    sums = np.full((8, max(nbox, 1)), float(SENTINEL)) if with_sums else None
    used = C.c_int64(SENTINEL)
    try:
        rc = ctx.lib.oisat_superob(ctx.h, ptr["lat"], ptr["lon"], ptr["xyz"], ptr["d"], ptr["sig"], ptr["var"], mm, float(box_deg),
                                   None if "n" in null else n.ctypes.data, None if "offset" in null else offset.ctypes.data,
                                   n.size, nbox, ptr["box"], None if "count" in null else count.ctypes.data,
                                   sums.ctypes.data if with_sums else None, C.byref(used))
        box = ctx.download(bufs["box"].ptr, (have,), np.int32)[:int(np.size(o["d"]))]
    finally:
        for b in bufs.values():
            b.free()
    return rc, box, count, sums, int(used.value)


def check_bits(got, o, box_deg, what):
    """Box ids, counts and every sum against the restatement, bit for bit.  -> the restatement."""
    rc, box, count, sums, used = got
    assert rc == 0
    ref = sc.ref_superob(o["lat"], o["lon"], sc.unit_vectors(o["lat"], o["lon"]), o["d"], o["sig"], o["var"], box_deg)
    np.testing.assert_array_equal(box, ref["box"])
    assert used == ref["nused"]
    want_count = np.zeros(count.size, dtype=np.int64)
    want_count[ref["ids"]] = ref["count"]
    np.testing.assert_array_equal(count, want_count)
    if sums is not None:
        want = np.zeros(sums.shape)
        want[:, ref["ids"]] = ref["sums"]
        for k, name in enumerate(sc.NAMES):
            assert sums[k].tobytes() == want[k].tobytes(), f"{what}: sum {name} differs in {int((sums[k] != want[k]).sum())} boxes"
    print(f"{what}: {ref['nused']} of {np.size(o['d'])} observations in {ref['ids'].size} boxes, largest {int(ref['count'].max(initial=0))}")
    return ref


def with_points(o, lat, lon, seed):
    """``o`` with deliberate positions appended (random d, sigma_b, var)."""
    rng = np.random.default_rng(seed)
    k = len(lat)
    return {"lat": np.concatenate([o["lat"], lat]), "lon": np.concatenate([o["lon"], lon]), "d": np.concatenate([o["d"], rng.normal(size=k)]),
            "sig": np.concatenate([o["sig"], rng.uniform(0.5, 2.0, k)]), "var": np.concatenate([o["var"], rng.uniform(0.05, 1.0, k)])}


# ---- 1. bit equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 4099])
@pytest.mark.parametrize("box_deg", [1.0, 7.0])
def test_sizes_around_the_block_edges(ctx, m, box_deg):
    o = sc.random_obs(100 + m, m, box_deg)
    if m:
        assert sc.edge_distance_deg(o["lat"], o["lon"], box_deg) >= 1e-9
    ref = check_bits(device_superob(ctx, o, box_deg), o, box_deg, f"m {m}, box {box_deg}")
    got = device_superob(ctx, o, box_deg, with_sums=False)                      # the count-only form: same ids, same counts
    check_bits(got, o, box_deg, f"m {m}, box {box_deg}, counts only")
    assert ref["nused"] == m


@pytest.mark.parametrize("box_deg", [0.5, 1.0, 7.0, 0.1])
def test_band_edges_poles_and_longitude_seams(ctx, box_deg):
    """Latitude +-90 and exactly on band edges (0.5 and 1 are binary-exact), longitude -180, 180, 0, 360, -1e-17 (t rounds to
    1: the last box of the band) and the double below 360, crossed with each other, among 600 random observations."""
    o = sc.random_obs(31, 600, box_deg)
    assert sc.edge_distance_deg(o["lat"], o["lon"], box_deg) >= 1e-9
    lats = [-90.0, 90.0, -90.0 + box_deg, 0.0, 3 * box_deg, -5 * box_deg, 90.0 - box_deg, math.nextafter(90.0, 0.0), 89.99, 12.3]
    lons = [-180.0, 180.0, 0.0, 360.0, -1e-17, math.nextafter(360.0, 0.0), -0.0, 720.0, -360.0, 33.3]
    la, lo = np.meshgrid(lats, lons, indexing="ij")
    o = with_points(o, la.ravel(), lo.ravel(), 32)
    ref = check_bits(device_superob(ctx, o, box_deg), o, box_deg, f"edges, box {box_deg}")
    n, offset, nbox = sc.box_table(box_deg)
    tail = ref["box"][600:].reshape(len(lats), len(lons))
    assert ref["nused"] == o["d"].size
    assert (tail[1] >= offset[-1]).all() and (tail[0] < n[0]).all()             # the poles: the last and the first band
    assert (tail[:, 4] == tail[:, 5]).all()                                     # -1e-17 and the double below 360: the band's last box
    assert (tail[:, 2] == tail[:, 3]).all() and (tail[:, 2] == tail[:, 6]).all()  # 0, 360, -0: its first
    assert (tail[:, 0] == tail[:, 1]).all()                                     # -180 and 180 are one meridian
    j_edge = int(round((0.0 + 90.0) / box_deg))
    if box_deg in (0.5, 1.0):
        assert (tail[3] >= offset[j_edge]).all() and (tail[3] < offset[j_edge] + n[j_edge]).all()   # an edge belongs to the band above


def test_all_in_one_box_and_each_in_its_own(ctx):
    rng = np.random.default_rng(5)
    m = 4099
    one = {"lat": rng.uniform(10.2, 10.8, m), "lon": rng.uniform(20.5, 21.2, m), "d": rng.normal(size=m),
           "sig": rng.uniform(0.5, 2.0, m), "var": rng.uniform(0.05, 1.0, m)}
    assert sc.edge_distance_deg(one["lat"], one["lon"], 1.0) >= 1e-9
    ref = check_bits(device_superob(ctx, one, 1.0), one, 1.0, "all in one box")
    assert ref["ids"].size == 1 and ref["count"][0] == m                        # the worst contention
    la, lo = np.meshgrid(-44.75 + 1.5 * np.arange(60), 0.7 + 5.0 * np.arange(69), indexing="ij")
    own = {"lat": la.ravel()[:m], "lon": lo.ravel()[:m], "d": rng.normal(size=m), "sig": rng.uniform(0.5, 2.0, m),
           "var": rng.uniform(0.05, 1.0, m)}
    assert sc.edge_distance_deg(own["lat"], own["lon"], 1.0) >= 1e-9
    ref = check_bits(device_superob(ctx, own, 1.0), own, 1.0, "each in its own box")
    assert ref["ids"].size == m and (ref["count"] == 1).all()


def test_gridded_rows_share_boxes_along_a_row(ctx):
    """The case the on-chip sums are for: 0.25 degree cells in row-major order, four consecutive lanes per 1 degree box at the
    equator, runs that cross wave and workgroup boundaries."""
    rng = np.random.default_rng(6)
    la, lo = np.meshgrid(-7.875 + 0.25 * np.arange(64), 0.125 + 0.25 * np.arange(65), indexing="ij")
    m = la.size
    o = {"lat": la.ravel(), "lon": lo.ravel(), "d": rng.normal(size=m), "sig": rng.uniform(0.5, 2.0, m), "var": rng.uniform(0.05, 1.0, m)}
    assert sc.edge_distance_deg(o["lat"], o["lon"], 1.0) >= 1e-9
    ref = check_bits(device_superob(ctx, o, 1.0), o, 1.0, "gridded rows")
    assert ref["count"].max() >= 16


# ---- 2. unused observations ----------------------------------------------------------------------------------------------------
def test_unused_observations_add_nothing(ctx):
    o = sc.random_obs(41, 700, 1.0)
    base = device_superob(ctx, o, 1.0)
    check_bits(base, o, 1.0, "700 used")
    rng = np.random.default_rng(42)
    bad = {"lat": rng.uniform(-80, 80, 9), "lon": rng.uniform(0, 360, 9), "d": rng.normal(size=9), "sig": np.ones(9), "var": np.full(9, 0.3)}
    bad["d"][0] = np.nan
    bad["var"][1] = np.inf
    bad["var"][2] = 0.0
    bad["var"][3] = -0.4
    bad["lat"][4] = np.nan
    bad["lat"][5] = 90.0000001
    bad["lat"][6] = -123.0
    bad["sig"][7] = np.inf
    bad["var"][8] = 5e-324                                      # 1 / var is not finite
    pos = rng.permutation(709)
    mixed = {k: np.concatenate([o[k], bad[k]])[pos] for k in o}
    got = device_superob(ctx, mixed, 1.0)
    with np.errstate(all="ignore"):
        ref = check_bits(got, mixed, 1.0, "700 used + 9 unused")
    rc, box, count, sums, used = got
    assert used == 700 and (box[np.argsort(pos)[700:]] == -1).all() and (box[np.argsort(pos)[:700]] >= 0).all()
    assert count.tobytes() == base[2].tobytes() and sums.tobytes() == base[3].tobytes()
    # the wrapper refuses var <= 0 on an otherwise usable observation instead of dropping it
    with pytest.raises(ValueError, match="variance <= 0"):
        dense.superob(mixed["lat"], mixed["lon"], mixed["d"], mixed["sig"], mixed["var"], 1.0, ctx=ctx)


# ---- 3. order and repetition; the error bound ---------------------------------------------------------------------------------------
def bound_check(ref, sums, what):
    """|sum - exact| <= count q / 2 + the last bit, the exact sum of the float64 terms by ``math.fsum``."""
    worst = 0.0
    for k in range(8):
        q = ref["q"][sc.QUANTUM_OF[k]]
        for i, b in enumerate(ref["ids"]):
            exact = math.fsum(ref["terms"][k][ref["slot"] == i])
            tol = ref["count"][i] * q / 2 + 2.0 ** -52 * abs(exact)
            err = abs(sums[k][b] - exact)
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
            assert err <= tol, (what, sc.NAMES[k], int(b), err, tol)
    print(f"{what}: worst error / bound {worst:.3f}; quanta {ref['q']}")


def test_order_and_repetition_change_no_bit(ctx):
    o = sc.random_obs(51, 1500, 7.0)
    assert sc.edge_distance_deg(o["lat"], o["lon"], 7.0) >= 1e-9
    a = device_superob(ctx, o, 7.0)
    b = device_superob(ctx, o, 7.0)
    perm = np.random.default_rng(52).permutation(1500)
    c = device_superob(ctx, {k: v[perm] for k, v in o.items()}, 7.0)
    for other in (b, c):
        assert other[2].tobytes() == a[2].tobytes() and other[3].tobytes() == a[3].tobytes() and other[4] == a[4]
    np.testing.assert_array_equal(c[1], a[1][perm])
    ref = check_bits(a, o, 7.0, "1500 observations, 7 degree boxes")
    bound_check(ref, a[3], "1500 observations, 7 degree boxes")


def test_dynamic_range(ctx):
    """Weights over twelve decades and one innovation 1e6 times the rest: the quanta grow with the maxima (as the
    covariogram's do), the bound count q / 2 still holds, and the bits still match."""
    rng = np.random.default_rng(61)
    m = 900
    o = sc.random_obs(62, m, 7.0, lat_range=(-30.0, 30.0), lon_range=(0.0, 90.0))
    o["var"] = 10.0 ** rng.uniform(-6.0, 6.0, m)
    plain = sc.ref_superob(o["lat"], o["lon"], sc.unit_vectors(o["lat"], o["lon"]), o["d"], o["sig"], o["var"], 7.0)
    o["d"][417] *= 1e6
    got = device_superob(ctx, o, 7.0)
    ref = check_bits(got, o, 7.0, "twelve decades of weights")
    assert ref["q"][2] > plain["q"][2] and ref["q"][3] > plain["q"][3] and ref["q"][0] == plain["q"][0]
    bound_check(ref, got[3], "twelve decades of weights")


# ---- 4. through the wrapper ------------------------------------------------------------------------------------------------------
def test_wrapper_matches_the_restated_merge(ctx):
    o = sc.random_obs(71, 2000, 1.0, lat_range=(20.0, 30.0), lon_range=(0.0, 12.0))
    ref = sc.ref_superob(o["lat"], o["lon"], sc.unit_vectors(o["lat"], o["lon"]), o["d"], o["sig"], o["var"], 1.0)
    for rho in (0.0, 0.3):
        want = sc.merge(ref, rho)
        s = dense.superob(o["lat"], o["lon"], o["d"], o["sig"], o["var"], 1.0, rho=rho, ctx=ctx)
        assert s["nobs"] == ref["ids"].size and s["nobs_raw"] == 2000 and s["rho"] == rho
        np.testing.assert_array_equal(s["box_id"], ref["ids"])
        np.testing.assert_array_equal(s["box"], ref["box"])
        np.testing.assert_array_equal(s["box_id"][s["index"]], ref["box"])
        for k in ("lat", "lon", "d", "sigma_b", "var", "spread", "count", "W"):
            assert np.asarray(s[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert dense.superob_count(o["lat"], o["lon"], o["d"], o["sig"], o["var"], 1.0, ctx=ctx) == ref["ids"].size


# ---- 5. OISAT_EINVAL -------------------------------------------------------------------------------------------------------------
def test_einval_leaves_the_outputs_untouched(ctx):
    o = sc.random_obs(81, 300, 1.0)
    good = sc.box_table(1.0)

    def untouched(got):
        rc, box, count, sums, used = got
        assert rc == EINVAL
        assert (box == SENTINEL).all() and (count == SENTINEL).all() and (sums == SENTINEL).all() and used == SENTINEL

    for bad in (0.0, -1.0, float("nan"), 180.5, float("inf")):
        untouched(device_superob(ctx, o, bad, table=good))
    untouched(device_superob(ctx, o, 1.0, m=(1 << 20) + 1))
    untouched(device_superob(ctx, o, 1.0, m=-1))
    for null in ("lat", "lon", "xyz", "d", "sig", "var", "box", "n", "offset"):
        untouched(device_superob(ctx, o, 1.0, null=(null,)))
    rc, box, _, sums, used = device_superob(ctx, o, 1.0, null=("count",))
    assert rc == EINVAL and (box == SENTINEL).all() and (sums == SENTINEL).all() and used == SENTINEL
    # a table that does not belong to box_deg: another box size's, a wrong offset, a wrong total, an empty band
    untouched(device_superob(ctx, o, 1.0, table=sc.box_table(0.5)))
    n, offset, nbox = good
    shifted = offset.copy()
    shifted[100] += 1
    untouched(device_superob(ctx, o, 1.0, table=(n, shifted, nbox)))
    untouched(device_superob(ctx, o, 1.0, table=(n, offset, nbox - 1)))
    untouched(device_superob(ctx, o, 1.0, table=(n, offset, nbox + 1)))
    zero = n.copy()
    zero[7] = 0
    untouched(device_superob(ctx, o, 1.0, table=(zero, offset, nbox)))
    # the count-only form does not need the unit vectors
    rc, box, count, _, used = device_superob(ctx, o, 1.0, with_sums=False, null=("xyz",))
    assert rc == 0 and used == 300 and count.sum() == 300 and (box >= 0).all()
