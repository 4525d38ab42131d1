"""Keeps tests/test_gpu_horizontal_abi.py honest without a GPU: every category the catalogues promise is present and means
what its tag says, the brute-force references agree with scipy's own trees / interpolators where those have a definite
answer, and the NumPy emulation of the UNPADDED 3 x 3 hash search misses every ``border_ulp`` target (if it ever finds
one, the catalogue has gone blunt) while the padded one agrees with brute force everywhere."""
from collections import Counter

import numpy as np
import pytest
from scipy.interpolate import LinearNDInterpolator, RBFInterpolator
from scipy.spatial import KDTree, cKDTree

import horizontal_cases as hc

NN_NAMES = hc.nn_scene_names()


# ---- A ---------------------------------------------------------------------------------------------------------------
def test_nn_catalogue_has_every_category():
    tags = Counter(t for n in NN_NAMES for t in hc.nn_scene(n).tags)
    for tag in ("border_ulp", "at_radius_kept", "at_radius_masked", "on_point", "dup_points", "tie2", "tie4", "near_tie", "nan_point",
                "nan_target", "outside_box", "one_point", "collinear", "all_nan_points", "coarsened", "coarsened_1000", "tiles2", "generic"):
        assert tags[tag] >= 16, (tag, tags[tag])
    assert all(hc.nn_scene(n).P <= 3000 and hc.nn_scene(n).T <= 300 for n in NN_NAMES)


@pytest.mark.parametrize("name", NN_NAMES)
def test_nn_reference_agrees_with_ckdtree_and_the_padded_search(name):
    sc = hc.nn_scene(name)
    ref = hc.brute_nn(sc)
    new = hc.emulate_search(sc)
    np.testing.assert_array_equal(new["idx"], ref["idx"])
    np.testing.assert_array_equal(new["dist"], ref["dist"])
    np.testing.assert_array_equal(new["ties"], ref["ties"])
    fin = np.flatnonzero(~(np.isnan(sc.px) | np.isnan(sc.py)))
    if fin.size == 0:
        assert (ref["idx"] == -1).all() and np.isposinf(ref["dist"]).all()
        return
    tfin = ~(np.isnan(sc.tx) | np.isnan(sc.ty))
    untied = tfin.copy()
    with np.errstate(invalid="ignore"):
        untied &= ~(ref["second"] - ref["best"] <= ref["best"] * hc.TIE_REL)         # tied whether kept or not
    d, i = cKDTree(np.column_stack([sc.px[fin], sc.py[fin]])).query(np.column_stack([sc.tx[untied], sc.ty[untied]]))
    masked = d > sc.max_dist
    np.testing.assert_array_equal(ref["idx"][untied] == -1, masked)
    np.testing.assert_array_equal(ref["idx"][untied][~masked], fin[i][~masked])
    np.testing.assert_array_equal(ref["dist"][untied][~masked], d[~masked])
    assert (ref["idx"][~tfin] == -1).all() and np.isposinf(ref["dist"][~tfin]).all()


def test_unpadded_search_misses_every_border_case():
    signs, near_both = set(), 0
    for name in NN_NAMES:
        sc = hc.nn_scene(name)
        ref, old = hc.brute_nn(sc), hc.emulate_search(sc, pad=0.0)
        b = sc.where("border_ulp")
        if not name.startswith("border_ulp"):
            np.testing.assert_array_equal(old["idx"], ref["idx"])           # ordinary inputs never showed it
            assert b.size == 0
            continue
        assert b.size == sc.T == 8
        assert (ref["idx"][b] >= 2).all() and (old["idx"][b] == -1).all(), name           # found by brute force, never looked at
        assert (ref["dist"][b] < sc.max_dist).all()
        gap = old["cell_gap"][:, b, ref["idx"][b]]                           # [2, n]: cells between the point and its target
        assert (np.abs(gap).max(axis=0) == 2).all(), gap
        signs |= set(np.sign(gap[np.abs(gap) == 2]))
        g = hc.hash_grid(sc.px, sc.py, sc.max_dist)
        for v, v0 in ((sc.tx[b], g["x0"]), (sc.ty[b], g["y0"])):             # 0-3 ulp from a border on the axis that matters
            q = (v - v0) * g["inv_h"]
            edge = v0 + np.rint(q) * g["cell"]
            close = np.abs(v - edge) <= 4 * np.spacing(np.abs(edge))
            near_both += int(close.sum())
        d = np.sqrt(hc._d2_matrix(sc)[b])
        assert ((d < 3 * sc.max_dist).sum(axis=1) == 1).all()                # the only point within reach
    assert signs == {-1.0, 1.0}
    assert near_both > 100                                                    # 80 targets, each near one border, half near two
    used = {n.split("-", 2)[1:][0] + n.split("-", 2)[2] for n in NN_NAMES if n.startswith("border_ulp")}
    assert len(used) == len(hc.MAX_DISTS) * len(hc.ORIGINS) - len(hc.BORDER_EXACT)


def test_no_border_case_exists_where_the_arithmetic_is_exact():
    rng = np.random.default_rng(5)
    for hi, origin in hc.BORDER_EXACT:
        for v0, span in ((float(origin), 300.0), (float(origin) + 90.0, 140.0)):
            assert hc._border_hits(rng, v0, span, hc.MAX_DISTS[hi], n=400000)[0].size == 0


def test_nn_tags_mean_what_they_say():
    sc = hc.nn_scene("main")
    ref = hc.brute_nn(sc)
    ties = set(ref["ties"].tolist())
    d2 = hc._d2_matrix(sc)
    mult = (d2 == ref["best"][:, None]).sum(axis=1)
    for tag, m in (("tie2", 2), ("tie4", 4), ("dup_points", 2)):
        w = sc.where(tag)
        assert set(w.tolist()) <= ties and (mult[w] >= m).all() and (mult[w] == m).sum() >= 16, tag   # (a duplicated node adds one)
    assert (ref["dist"][sc.where("dup_points")] == 0).all() and (ref["dist"][sc.where("on_point")] == 0).all()
    assert not set(sc.where("on_point").tolist()) & ties
    w = sc.where("near_tie")
    assert ((ref["second"][w] - ref["best"][w]) / ref["best"][w] >= 1e-9).all() and not set(w.tolist()) & ties
    assert ((ref["second"][w] - ref["best"][w]) / ref["best"][w] < 1e-5).all()
    nan_pts = np.flatnonzero(np.isnan(sc.px) | np.isnan(sc.py))
    assert nan_pts.size == hc.REPS and not np.isin(ref["idx"], nan_pts).any()
    assert (ref["idx"][sc.where("nan_point")] >= 0).all()
    assert (ref["idx"][sc.where("nan_target")] == -1).all()
    w = sc.where("outside_box")
    fin = ~np.isnan(sc.px + sc.py)
    box = (sc.px[fin].min(), sc.px[fin].max(), sc.py[fin].min(), sc.py[fin].max())
    sides = [sc.tx[w] < box[0], sc.tx[w] > box[1], sc.ty[w] < box[2], sc.ty[w] > box[3]]
    for s in sides:
        assert (ref["idx"][w][s] >= 0).sum() >= 3 and (ref["idx"][w][s] == -1).sum() >= 3
    assert np.logical_or.reduce(sides).all()
    for i in range(len(hc.MAX_DISTS)):
        sc = hc.nn_scene(f"at_radius-{i}")
        ref = hc.brute_nn(sc)
        k, m = sc.where("at_radius_kept"), sc.where("at_radius_masked")
        assert (ref["dist"][k] == sc.max_dist).all() and (ref["idx"][k] >= 0).all()
        assert (ref["dist_unmasked"][m] == np.nextafter(sc.max_dist, np.inf)).all() and (ref["idx"][m] == -1).all()
        assert ((sc.px != sc.tx) & (sc.py != sc.ty)).sum() == 1                       # one pair off the axes
    sc = hc.nn_scene("collinear")
    assert np.ptp(sc.py) == 0 and hc.hash_grid(sc.px, sc.py, sc.max_dist)["nby"] == 1
    for name in ("one_point", "collinear"):
        ref = hc.brute_nn(hc.nn_scene(name))
        assert 6 <= (ref["idx"] >= 0).sum() <= 18
    assert hc.nn_scene("one_point").P == 1


def test_nn_hash_shapes():
    def grid(name):
        sc = hc.nn_scene(name)
        return hc.hash_grid(sc.px, sc.py, sc.max_dist * (1 + hc.PAD))

    g = grid("coarsened")                       # 360 x 180 degrees against 1e-3: seven doublings, 967 tiles of 4096 counters
    assert g["cell"] == 1e-3 * (1 + hc.PAD) * 128 and g["ncell"] <= hc.MAX_CELLS and g["ntile"] > 900
    g = grid("coarsened_1000")                  # 9.75e-4 instead: the same doublings land just under the cap, 1017 tiles
    assert g["ncell"] <= hc.MAX_CELLS and g["ntile"] > 1000
    assert 4096 < grid("tiles2-4096")["ncell"] <= 4096 + 128 and 8192 < grid("tiles2-8192")["ncell"] <= 8192 + 128
    for name in ("coarsened", "coarsened_1000", "tiles2-4096", "tiles2-8192"):
        ref = hc.brute_nn(hc.nn_scene(name))
        assert (ref["idx"] >= 0).sum() >= 12 and (ref["idx"] == -1).sum() >= 12


def test_catalogues_are_deterministic():
    a = hc.nn_scene("border_ulp-2-random")
    hc.nn_scene.cache_clear()
    b = hc.nn_scene("border_ulp-2-random")
    assert a is not b
    for nm in ("px", "py", "tx", "ty"):
        np.testing.assert_array_equal(getattr(a, nm), getattr(b, nm))
    a = hc.rbf_scene("lattice", 5)
    hc.rbf_scene.cache_clear()
    hc.rbf_reference.cache_clear()
    b = hc.rbf_scene("lattice", 5)
    assert a is not b and a.tags == b.tags
    np.testing.assert_array_equal(a.tx, b.tx)
    a = hc.linear_scene("scatter30")
    hc.linear_scene.cache_clear()
    b = hc.linear_scene("scatter30")
    np.testing.assert_array_equal(a.tx, b.tx)
    np.testing.assert_array_equal(a.tri.simplices, b.tri.simplices)


# ---- B ---------------------------------------------------------------------------------------------------------------
def test_box_windows_cover_every_live_dispatch_path():
    w = hc.BOX_WINDOWS
    assert any(kx <= 64 and ky * kx >= 3 for ky, kx in w)                    # the row-wise kernel ...
    assert {kx for ky, kx in w if kx <= 64 and ky * kx >= 3} >= {3, 4, 5, 7, 21, 32, 33, 64}      # ... 64 / kx = 21 .. 1 targets a wave
    assert any(ky > 8 for ky, kx in w if kx <= 64) and any(ky % 8 for ky, kx in w)                # more than one batch of 8 rows
    assert sum(kx > 64 for ky, kx in w) == 2 and sum(ky * kx < 3 for ky, kx in w) == 3            # G = 64, G = 1
    assert hc.pick_tns(21) == [1, 2, 4, 257] and hc.pick_tns(64) == [1, 2, 257] and hc.pick_tns(70) == [1, 2, 257]
    Ny, Nx, ky, kx, nf, Tn = hc.BOX_WRAP
    assert -(-Tn // (64 // kx)) * nf > 8192 * 4
    for Ny, Nx, ky, kx in hc.BOX_NARROW:
        assert Ny < ky // 2 or Nx < kx // 2                                    # reflected more than once


@pytest.mark.parametrize("shape", [(13, 17, 4, 4), (13, 17, 3, 3), (7, 9, 1, 2), (7, 9, 2, 5)] + list(hc.BOX_NARROW))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_box_reference_is_the_window_sum(shape, dtype):
    Ny, Nx, ky, kx = shape
    Z = hc.box_fields(Ny, Nx, dtype, specials=(Ny, Nx, ky, kx) not in hc.BOX_NARROW)
    for f in range(3):
        for variance in (0, 1):
            ref, bar = hc.box_reference(Z[f], ky, kx, variance)
            kk = float(ky * kx)
            direct = hc.box_direct(Z[f], ky, kx, 1 / (kk * kk) if variance else 1 / kk)
            bad, ratio = hc.compare_bar(direct, ref, (ky * kx + 2) * 2.0 ** -53 * bar / ((ky * kx + 2) * hc.UNIT[np.dtype(dtype)]))
            assert not bad, (f, variance, bad[:5], ratio)
            if f == 1 and (Ny, Nx, ky, kx) not in hc.BOX_NARROW:
                assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isfinite(ref).any()


def test_box_fields_hold_the_special_windows():
    for ky, kx in hc.BOX_WINDOWS:
        Ny, Nx = hc.box_shape(ky, kx)
        Z = hc.box_fields(Ny, Nx, np.float32)
        ref, _ = hc.box_reference(Z[1], ky, kx, 0)
        assert np.isnan(ref[1, 1]) and np.isposinf(ref[1, Nx - 2]) and (kx < 2 or np.isnan(ref[Ny - 2, 1:3]).any())  # NaN; +inf; +inf and -inf
        assert np.isfinite(ref).mean() > 0.2, (ky, kx)
        idx = hc.pick_idx(Ny, Nx, hc.PRIME_TN)
        assert (idx == -1).sum() >= 2 and len(set(idx.tolist())) < idx.size and {0, Nx - 1, (Ny - 1) * Nx, Ny * Nx - 1} <= set(idx.tolist())
        assert idx.min() >= -1 and idx.max() < Ny * Nx


def test_compare_bar_notices_each_kind_of_difference():
    ref = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, 2.0])
    bar = np.array([1e-12, 0.0, 0.0, 0.0, 0.0, 4e-12])
    assert hc.compare_bar(ref.copy(), ref, bar)[0] == []
    for i, v in ((0, np.nan), (1, 0.0), (2, -np.inf), (3, np.inf), (4, 1e-300), (0, 1.0 + 1e-11), (5, 2.0 + 1e-11), (2, 1e308)):
        got = ref.copy()
        got[i] = v
        assert hc.compare_bar(got, ref, bar)[0] == [i], (i, v)
    got = ref.copy()
    got[5] = 2.0 + 2e-12
    assert hc.compare_bar(got, ref, bar)[0] == []


# ---- C ---------------------------------------------------------------------------------------------------------------
RBF_CASES = [(kind, K) for kind in hc.RBF_KINDS for K in hc.RBF_KS]


@pytest.mark.parametrize("kind,K", RBF_CASES, ids=[f"{k}-K{K}" for k, K in RBF_CASES])
def test_rbf_catalogue(kind, K):
    sc, r = hc.rbf_scene(kind, K), hc.rbf_reference(kind, K)
    assert sc.P <= 64 and sc.T <= 150
    judged = r["ok"] & ~r["singular"]
    # every target is one the references can judge: well conditioned, or singular because its neighbours share a row / column
    assert (r["singular"] == r["collinear"]).all()
    assert (r["cond"][~r["singular"]] <= hc.COND_MAX).all()
    if not kind.startswith("lattice"):
        assert not r["tie"].any()
    # A against B, in the measure of the bar, on the two finite value fields
    v = sc.values(np.float64)
    assert np.array_equal(v[:sc.P], np.eye(sc.P)) and np.isnan(v[sc.P + 2]).sum() == 1
    ea, sa = hc.rbf_expected(r["Wa"], r["nbr"], r["ok"], r["singular"], v[sc.P:])
    eb, _ = hc.rbf_expected(r["Wb"], r["nbr"], r["ok"], r["singular"], v[sc.P:])
    np.testing.assert_array_equal(np.isnan(ea), np.isnan(eb))
    fin = np.isfinite(ea)
    assert fin[:2].all(axis=0)[judged].all() and not fin[:, ~judged].any()
    dist = float((np.abs(ea - eb)[fin] / sa[fin]).max()) if fin.any() else 0.0
    print(f"{sc.name}: A-B {dist:.3e}")
    assert dist <= 2 * hc.RBF_AB_CPU                 # (LAPACK's kernels differ by CPU: a factor 2 of room, the bar itself is 8 x)
    # A against scipy's RBFInterpolator on the untied, evaluated targets
    u = np.flatnonzero(judged & ~r["tie"])
    if u.size:
        want = RBFInterpolator(np.column_stack([sc.px, sc.py]), v[sc.P:sc.P + 2].T, neighbors=K, kernel="thin_plate_spline")(
            np.column_stack([sc.tx[u], sc.ty[u]])).T
        assert (np.abs(want - ea[:2, u]) <= hc.RBF_TOL * sa[:2, u]).all(), float((np.abs(want - ea[:2, u]) / sa[:2, u]).max())
    # the tie flag is KDTree's ambiguity: where it is not set, scipy's tree names the same neighbours
    if sc.P > K:
        _, ids = KDTree(np.column_stack([sc.px, sc.py])).query(np.column_stack([sc.tx, sc.ty]), K)
        same = np.array([set(a) == set(b) for a, b in zip(ids, r["ids"])])
        assert same[~r["tie"]].all()


def test_rbf_bar_is_eight_times_the_cpu_distance_and_holds_the_device_distance():
    assert hc.RBF_TOL == max(8 * hc.RBF_AB_CPU, 1e-12) and hc.RBF_DEVICE_MEASURED <= hc.RBF_TOL


def test_rbf_catalogue_has_every_category():
    for K in hc.RBF_KS:
        tags = Counter(t for kind in hc.RBF_KINDS for t in hc.rbf_scene(kind, K).tags)
        for tag in ("generic", "outside_left", "outside_right", "outside_below", "outside_above", "on_point", "far_target", "nan_value",
                    "nn_minus1", "masked_far", "node", "edge_mid", "centre", "masked_beyond", "row", "p_equals_k"):
            assert tags[tag] >= 3, (K, tag)
        sc, r = hc.rbf_scene("generic", K), hc.rbf_reference("generic", K)
        hit = r["nbr"][:, sc.P // 3]
        assert hit[sc.where("nan_value")].all() and not hit.all()             # the NaN value is in those neighbourhoods, not in all
        assert (sc.nn_idx[sc.where("nn_minus1")] == -1).all() and (sc.nn_idx[sc.where("on_point")] >= 0).all()
        lat = hc.rbf_reference("lattice", K)
        wide = hc.rbf_reference("lattice_wide", K)
        assert lat["tie"].sum() >= 20 and (wide["tie"] & wide["singular"] & wide["ok"]).sum() >= 3           # zero pivots that are ties'
        masked = ~lat["ok"]
        assert (lat["singular"] & masked).sum() >= 3 and (~lat["singular"] & masked).sum() >= 3
        row = hc.rbf_reference("row", K)
        assert row["singular"].all() and row["ok"].all() and hc.rbf_scene("row", K).P == 5
        assert hc.rbf_scene("p_equals_k", K).P == K
        assert hc.rbf_scene("cluster", K).nn_idx.min() >= 0


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.LINEAR_SCENES)
def test_linear_catalogue(name):
    sc = hc.linear_scene(name)
    tri = sc.tri
    assert 30 <= sc.P <= 300 and sc.T <= 300
    xy = np.column_stack([sc.tx, sc.ty])
    v = sc.values(np.float64)
    want = LinearNDInterpolator(tri, v.T)(xy).T
    s = tri.find_simplex(xy)
    got, scale = hc.linear_in_simplex(tri, s, sc.tx, sc.ty, v)
    # generic targets: unambiguous by construction, and the restated interpolant is scipy's
    g = sc.where("generic")
    assert g.size == 2 * hc.REPS and (s[g] >= 0).all()
    c = hc.barycentric(tri, s[g], sc.tx[g], sc.ty[g])
    assert (c > 0.049).all()
    assert all(hc.accepting_simplices(tri, sc.tx[i], sc.ty[i]).size == 1 for i in g)
    bad, _ = hc.compare_bar(got[:, g], want[:, g], hc.RT64 * scale[:, g])
    assert not bad
    assert np.isnan(want[2, g]).any() and np.isfinite(want[2, g]).any() and np.isfinite(want[:2, g]).all()
    assert np.isnan(want[:, sc.where("outside")]).all() and (s[sc.where("outside")] == -1).all()
    for tag in ("on_vertex", "on_edge"):
        w = sc.where(tag)
        assert w.size >= 12 and all(hc.accepting_simplices(tri, sc.tx[i], sc.ty[i]).size >= 2 for i in w), tag
    assert (sc.nn_idx[sc.where("nn_minus1")] == -1).all() and (np.delete(sc.nn_idx, sc.where("nn_minus1")) >= 0).all()
    if name == "swath_grid":
        assert np.isnan(tri.transform[:, 0, 0]).sum() >= 3                   # collinear triples: scipy marks their transforms NaN
        assert sc.where("hull_row").size >= 50


def test_restated_walk_agrees_with_scipy_where_scipy_is_definite():
    """horizontal_cases.walk_reference (what include/oisat.h documents) against LinearNDInterpolator: everywhere on the
    scattered sets; on the swath grid everywhere but on targets that graze the hull, of which there is at least one"""
    for name in hc.LINEAR_SCENES:
        sc = hc.linear_scene(name)
        v = sc.values(np.float64)[:2]
        got, scale, amb = hc.walk_reference(sc, v, bounds=sc.arrays()["bounds"])
        want = LinearNDInterpolator(sc.tri, v.T)(np.column_stack([sc.tx, sc.ty])).T
        want[:, sc.nn_idx < 0] = np.nan
        differs = np.flatnonzero((np.isnan(got) != np.isnan(want)).any(axis=0))
        assert (differs.size > 0) == (name == "swath_grid"), (name, differs)
        assert all(hc.grazes_hull(sc.tri, sc.tx[i], sc.ty[i]) and sc.tags[i] == "hull_row" for i in differs)
        assert set(sc.where("on_vertex")) | set(sc.where("on_edge")) <= set(amb.tolist())
        g = sc.where("generic")
        bad, _ = hc.compare_bar(got[:, g], want[:, g], hc.RT64 * scale[:, g])
        assert not bad
        same = hc.walk_reference(sc, v, forced=np.full(sc.T, -2))[0]
        np.testing.assert_array_equal(same, got)
