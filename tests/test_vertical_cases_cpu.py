"""Keeps tests/test_gpu_vertical_abi.py honest without a GPU: every category of adversarial column is present in every
catalogue it launches, the catalogues are well conditioned (so the device's last bit of `log` cannot decide a verdict),
and the oracle's per-pixel functions run on all of them under the scipy installed here."""
import numpy as np
import pytest

from oracle import oi_oracle as orc
import vertical_cases as vc

PIXELS = {"amf": orc.amf_pixel, "mopitt": orc.mopitt_pixel, "gosat": orc.gosat_pixel}
CASES = [(op, nzs, nzc) for op in vc.OPS for nzs, nzc in vc.PAIRS[op]]
# what the issue lists, by the tags of vertical_cases (an absent tropopause is a launch mode, not a column)
LISTED = {
    "all": ["order_asc", "order_desc", "order_shuffled", "dup_pair_first", "dup_pair_mid", "dup_pair_last", "dup_all",
            "on_node_first", "on_node_last", "query_below_first", "query_above_last", "nan_node_p", "nan_query_p",
            "y_nan_first", "y_nan_last", "y_pinf_first", "y_pinf_last", "y_ninf_first", "y_ninf_last", "p_zero_node",
            "p_zero_query", "p_neg_node", "p_neg_query", "on_node_beside_nan", "on_node_beside_inf"],
    "three_nodes": ["dup_run3", "on_node_mid", "y_nan_mid", "y_pinf_mid", "y_ninf_mid"],
    "amf": ["trop_below_all", "trop_equal_level", "trop_above_all", "trop_nan", "sw_all_zero", "vcd_nan", "vcd_pinf", "vcd_ninf",
            "partial_column_nonfinite"],
    "mopitt": ["prof_negative", "prof_zero", "apriori_zero", "ak_zero_against_inf", "air_all_nan", "air_sum_zero",
               "surface_level0_shuffled", "vcd_nan", "vcd_pinf", "vcd_ninf"],
    "gosat": ["term_negative", "term_pzero", "term_nzero", "all_terms_dropped", "xcol_nan", "xcol_pinf", "xcol_ninf"],
}


def test_pairs_cover_the_level_counts_and_limits():
    assert {a for op in vc.OPS for a, _ in vc.PAIRS[op]} == {1, 2, 7, 8, 9, 35, 64}
    assert {b for op in vc.OPS for _, b in vc.PAIRS[op]} == {1, 2, 7, 8, 9, 16, 17, 72, 127, 128}
    assert all(a >= 2 for a, _ in vc.PAIRS["amf"]) and all(b >= 2 for op in ("mopitt", "gosat") for _, b in vc.PAIRS[op])
    assert any(a == 1 for a, _ in vc.PAIRS["mopitt"]) and any(a == 1 for a, _ in vc.PAIRS["gosat"])
    assert any(b == 1 for _, b in vc.PAIRS["amf"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("op,nzs,nzc", CASES, ids=[f"{op}-nzs{a}-nzc{b}" for op, a, b in CASES])
def test_catalogue(op, nzs, nzc, dtype):
    cat = vc.catalogue(op, nzs, nzc, dtype)
    present = set(cat.tags)
    n_nodes = nzs if op == "amf" else nzc

    # every category, by tag
    want = LISTED["all"] + LISTED[op] + (LISTED["three_nodes"] if n_nodes >= 3 else [])
    assert not [t for t in want if t not in present], (op, nzs, nzc)
    assert present == set(vc.required_tags(op, nzs, nzc))
    assert 700 <= cat.n <= 1100 and cat.n > 129
    assert cat.ctm_p.dtype == np.dtype(dtype) and cat.ctm_y.dtype == np.dtype(dtype) and cat.sat_p.dtype == np.float64
    assert cat.ctm_p.shape == (nzc, cat.n) and cat.sat_p.shape == (nzs, cat.n)
    assert cat.pattern_only().mean() <= 0.03
    assert cat.pattern_only().any() == (op == "mopitt" and dtype == np.float64)

    # the tags mean what they say: exact copies, exact ties, and 1 % between distinct levels
    node_p, query_p = (cat.sat_p, cat.ctm_p) if op == "amf" else (cat.ctm_p, cat.sat_p)
    with np.errstate(all="ignore"):
        node_x = np.log(node_p.astype(np.float64)).astype(node_p.dtype).astype(np.float64)
        query_x = np.log(query_p.astype(np.float64)).astype(query_p.dtype).astype(np.float64)
    for i, t in enumerate(cat.tags):
        assert vc.spacing_ok(cat.sat_p[:, i]) and vc.spacing_ok(cat.ctm_p[:, i]), (i, t)
        p = node_p[:, i]
        copies = p.size - np.unique(p).size
        if t in vc.DUP_TAGS:
            assert copies == {"dup_run3": 2, "dup_all": p.size - 1}.get(t, 1), (i, t, p)
        else:
            assert copies == 0, (i, t, p)
        if t.startswith("on_node") or t == "prof_zero":
            assert np.isin(query_x[:, i], node_x[:, i]).any(), (i, t)
        if t == "nan_node_p":
            assert np.isnan(p).sum() == 1
        if t == "surface_level0_shuffled":
            assert np.argmax(cat.ctm_p[:, i]) != 0         # model level 0 is not the surface: sorting moves it
    kinds = {t: {tuple(np.argsort(cat.sat_p[:, i])) for i, tt in enumerate(cat.tags) if tt == t} for t in
             ("order_asc", "order_desc", "order_shuffled")}
    if nzs > 2:
        up = tuple(range(nzs))
        assert kinds["order_asc"] == {up} and kinds["order_desc"] == {up[::-1]} and not kinds["order_shuffled"] & {up, up[::-1]}

    # well conditioned: one ulp on every logarithm moves no verdict by more than half the bar
    assert vc.well_conditioned(cat).all()

    # the oracle's own pixel functions run on every column, and the log-pinned twins are the same arithmetic
    ref = vc.reference(cat, PIXELS[op])
    if dtype == np.float64:
        twin = vc.reference(cat)
        for nm in ref:
            np.testing.assert_array_equal(ref[nm][0], twin[nm][0])
    for nm, (r, s) in ref.items():
        fin = np.isfinite(r)
        assert fin.mean() > 0.2, (nm, fin.mean())                   # a catalogue of NaNs would test nothing
        assert (np.nan_to_num(s[fin], nan=0.0) >= 0).all()
    if op == "amf":
        vc.reference(cat, PIXELS[op], use_trop=False)


def test_catalogue_is_deterministic():
    vc.catalogue.cache_clear()
    a = vc.catalogue("mopitt", 7, 7, np.float32)
    vc.catalogue.cache_clear()
    b = vc.catalogue("mopitt", 7, 7, np.float32)
    assert a.tags == b.tags and a is not b
    for nm in ("sat_p", "ctm_p", "ctm_y", "air", "ak", "ap_prof", "vcd", "ap_col", "ap_surf"):
        np.testing.assert_array_equal(getattr(a, nm), getattr(b, nm))


def test_compare_notices_each_kind_of_difference():
    ref = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, 2.0])
    scale = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 4.0])
    assert vc.compare(ref.copy(), ref, scale, 1e-12) == ([], 0.0)
    for i, v in ((0, np.nan), (1, 0.0), (2, -np.inf), (3, np.inf), (4, 1e-300), (0, 1.0 + 1e-11), (5, 2.0 + 1e-11)):
        got = ref.copy()
        got[i] = v
        assert vc.compare(got, ref, scale, 1e-12)[0] == [i], (i, v)
    got = ref.copy()
    got[5] = 2.0 + 2e-12                   # within 1e-12 of the scale 4, though not of |ref|
    assert vc.compare(got, ref, scale, 1e-12)[0] == []
    got[0] = 5.0                           # values are not judged where check_values says so; patterns always are
    only = np.array([False, True, True, True, True, True])
    assert vc.compare(got, ref, scale, 1e-12, check_values=only)[0] == []
    got[0] = np.nan
    assert vc.compare(got, ref, scale, 1e-12, check_values=only)[0] == [0]
