"""Keeps tests/test_gpu_elementwise_abi.py honest without a GPU: every family of tests/elementwise_cases.py has its members
and reproduces from its seed, the special values are where the scenes promise them, the knee scenes spread over the sweep and
the two host implementations of the pick agree on them, references (a) and (b) of the sweep agree within the derived bars (so
the bars are not vacuous), and each deliberately wrong restatement of a kernel is rejected by the catalogue's own comparison
on at least one scene (so the catalogues are sharp).  Two pins on the host knee twin say what it does on tables that are not
ascending: the library refuses those where the walk would leave its arrays."""
import math
from fractions import Fraction

import numpy as np
import pytest

import elementwise_cases as ec
from oisatgmi._kneedle import knee_index
from oracle import oi_oracle as orc

F64_MAIN = [n for n in ec.sweep_scene_names("main") if n.startswith("f64")]
F64_SPECIALS = [n for n in ec.sweep_scene_names("specials") if n.startswith("f64")]


# ---- A. the sweep ------------------------------------------------------------------------------------------------------
def test_sweep_family_has_every_member():
    pairs = ec.sweep_pairs()
    assert len(pairs) == len(set(pairs)) == 79
    for n in ec.SWEEP_NS:
        assert {s for m, s in pairs if m == n} >= {1, 33, 97, 99, 128}
    for s in ec.SWEEP_SCALES:
        assert {n for n, t in pairs if t == s} >= {1, 65, ec.STRIPE + 1}
    assert ec.SWEEP_NS == (1, 2, 63, 64, 65, 127, 129, 262143, 262144, 262145, 262144 + 65)
    assert ec.SWEEP_SCALES == (1, 2, 3, 31, 32, 33, 64, 95, 96, 97, 99, 127, 128) and max(ec.SWEEP_SCALES) == ec.MAX_SCALES
    names = ec.sweep_scene_names()
    assert len(names) == len(set(names)) == 2 * (79 + len(ec.SWEEP_SPECIALS))
    assert ec.sweep_depth(ec.STRIPE) == 64 and ec.sweep_depth(ec.STRIPE + 1) == 96 and ec.sweep_depth(1) == 64


@pytest.mark.parametrize("name", ["f64-n65-s99", "f32-n262145-s33"] + ec.sweep_scene_names("specials"))
def test_sweep_scenes_reproduce_and_hold_what_they_promise(name):
    a = ec.sweep_scene(name)
    ec.sweep_scene.cache_clear()
    b = ec.sweep_scene(name)
    assert a is not b and a.dtype == b.dtype == np.dtype(np.float64 if name.startswith("f64") else np.float32)
    for x, y in ((a.Sa, b.Sa), (a.So, b.So), (a.table, b.table)):
        np.testing.assert_array_equal(x, y)
    assert np.unique(a.table).size == a.nscales
    if a.specials:
        sp = ec.SPECIALS.astype(a.dtype)                                  # (float32: 1e-300 and 5e-324 are 0, 1e300 is inf)
        for arr in (a.Sa, a.So):
            assert np.isnan(arr).any()
            for v in sp[~np.isnan(sp)]:
                assert ((arr == v) & (np.signbit(arr) == np.signbit(v))).any(), v
        return
    i = np.arange(a.n)
    assert np.isnan(a.So[i % 7 == 3]).all() and (a.Sa[i % 11 == 5] == 0).all() and not np.isnan(a.Sa).any()
    pairs = np.stack([a.Sa, a.So])[:, ~np.isnan(a.So) & (a.Sa > 1e-30)]
    assert np.unique(pairs, axis=1).shape[1] == pairs.shape[1]            # the ordinary cells are all distinct
    if a.n >= 65:
        tiny = a.Sa[(i % 53 == 2) & (i % 11 != 5)]
        assert tiny.size and (tiny > 0).all() and (tiny < 1e-37).all()


def test_sweep_counts_depend_on_the_cell_and_on_the_scaling():
    for name in ("f64-n65-s99", "f32-n65-s99", "f64-n262145-s99", "f64-n262145-s33"):
        sc, ref = ec.sweep_scene(name), ec.sweep_reference(name)
        c = np.array(ref.count)
        steps = 3 if sc.nscales == 99 else 2                              # (the 33-point table ends at 0.17)
        assert 0 < c.max() < sc.n and np.unique(c[c > 0]).size >= steps, (name, np.unique(c))   # the tiny cells join in one by one
        assert (np.diff(c[c > 0]) >= 0).all()
    sc, ref = ec.sweep_scene("f64-n65-s33"), ec.sweep_reference("f64-n65-s33")
    at = ec.ZERO_SCALE_AT[1]
    assert sc.table[at] == 0.0 and ref.count[at] == 0 and ref.kind[at] == "nan" and ref.kind.count("nan") == 1
    kinds = {k for n in ec.sweep_scene_names("specials") for k in ec.sweep_reference(n).kind}
    assert kinds >= {"finite", "+inf"}, kinds                             # (t + So = 5e-324 + ..: 1/denormal overflows)


def test_exact_sum_is_exact():
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 1, 20000) * 10.0 ** rng.uniform(-300, 300, 20000)
    v[:6] = [5e-324, -5e-324, 0.0, -0.0, 1e-320, 1.7e308]
    assert float(ec.exact_sum(v)) == math.fsum(v.tolist())
    assert ec.exact_sum(np.array([1.0, 2.0 ** -80, -1.0])) == Fraction(1, 2 ** 80)
    assert ec.exact_sum(np.array([5e-324, 5e-324])) == Fraction(1, 2 ** 1073)
    assert ec.exact_sum(np.zeros(0)) == 0


@pytest.mark.parametrize("name", F64_MAIN + F64_SPECIALS)
def test_sweep_references_a_and_b_agree_within_the_bars(name):
    """(b) is oracle.oi_curve: np.nanmean's pairwise sum is inside the summation term, the 1 - Sb/t form inside 1.5 2^-52.  On the
    specials scenes K is not confined to [0, 1] (negative variances): there only the counts and the kinds are compared."""
    sc, ref = ec.sweep_scene(name), ec.sweep_reference(name)
    b = orc.oi_curve(sc.Sa, sc.So, sc.table)
    with np.errstate(all="ignore"):
        cb = np.array([np.count_nonzero(~np.isnan(ec.sweep_ak(sc, s, "ref"))) for s in sc.table])
    if not sc.nonnegative:
        assert cb.tolist() == ref.count
        kind = ["nan" if np.isnan(m) else "finite" if np.isfinite(m) else "+inf" if m > 0 else "-inf" for m in b]
        assert kind == ref.kind
        return
    bad, worst = ec.sweep_compare(ref, b, cb, ec.REF_FORM_ABS)
    assert not bad, (bad[:5], worst)
    # and the bar notices a curve that is off by a part in 1e12
    fin = np.flatnonzero(np.isfinite(b) & (b > 1e-2))
    if fin.size:
        off = b.copy()
        off[fin[0]] *= 1 + 1e-12
        assert ec.sweep_compare(ref, off, cb, ec.REF_FORM_ABS)[0] == [fin[0]]
    wrong = cb.copy()
    wrong[-1] += 1
    assert ec.sweep_compare(ref, b, wrong, ec.REF_FORM_ABS)[0] == [sc.nscales - 1]


def _rejected(name, mutate):
    ref = ec.sweep_reference(name)
    m = ec.sweep_reference_of(ec.sweep_scene(name), mutate=mutate)
    return ec.sweep_compare(ref, m.mean_float(), np.array(m.count))[0]


def test_sweep_mutants_are_rejected():
    assert ec.sweep_compare(ec.sweep_reference("f64-n65-s99"), ec.sweep_reference("f64-n65-s99").mean_float(),
                            np.array(ec.sweep_reference("f64-n65-s99").count))[0] == []
    # the last cell of an odd tail (the dead half of the two-at-a-time walk)
    for name in ("f64-n1-s1", "f64-n65-s99", "f32-n129-s128", "f64-n262145-s97"):
        assert _rejected(name, "drop_odd_tail"), name
    assert _rejected("f64-n64-s99", "drop_odd_tail") == []               # (nothing to drop: the mutant is the reference)
    # scalings 96 and 97 exchanged (the xor-tree lanes)
    for name in ("f64-n65-s99", "f32-n1-s128", "f64-n262145-s127"):
        assert _rejected(name, "swap_96_97") == [96, 97], name
    # the stripe loop's second pass
    for name in ("f64-n262145-s1", "f32-n262209-s99"):
        assert len(_rejected(name, "skip_second_stripe")) == ec.sweep_scene(name).nscales, name
    assert _rejected("f64-n262144-s99", "skip_second_stripe") == []


# ---- B. the knee -------------------------------------------------------------------------------------------------------
def test_knee_scenes_spread_and_the_twins_agree():
    tables = ec.knee_tables()
    assert len(tables) == 14 and len(ec.KNEE_RATIOS) == 9
    assert [t.size for t in tables.values()] == [99, 128, 33, 3, 4, 8, 9, 10, 16, 17, 18, 96, 97, 64]
    for t in tables.values():
        assert (np.diff(t) > 0).all()
    assert np.ptp(np.diff(tables["jittered64"])) > 0.05 and np.ptp(np.diff(tables["uniform96"])) < 1e-12
    picks = {}
    for name in ec.knee_scene_names():
        sc = ec.knee_scene(name)
        curve = ec.knee_curve(sc)
        picks[name] = ec.host_knee(sc.table, curve)
        assert picks[name] == ec.oracle_knee(sc.table, curve), name
        assert knee_index(sc.table, curve) != 0                           # (index 0 always means "none" here)
    none = sum(v == 0 for v in picks.values())
    print(f"{len(picks)} knee scenes: {none} without a knee, {len(set(picks.values()))} distinct indices")
    assert len(picks) == 126 and 3 * none <= len(picks) and len(set(picks.values())) >= 25


def test_degenerate_knee_scenes_give_index_zero():
    assert ec.knee_scene_names("degenerate") == list(ec.KNEE_DEGENERATE)
    for name in ec.KNEE_DEGENERATE:
        sc = ec.knee_scene(name)
        curve = ec.knee_curve(sc)
        assert ec.host_knee(sc.table, curve) == 0, name
        if name != "equal_adjacent":                                      # (scipy's interp1d has its own view of a repeated node)
            assert ec.oracle_knee(sc.table, curve) == 0, name
    assert (ec.knee_curve(ec.knee_scene("flat")) == 1.0).all()
    assert np.isnan(ec.knee_curve(ec.knee_scene("all_nan"))).all()
    c = ec.knee_curve(ec.knee_scene("nan_mean"))
    assert np.isnan(c).sum() == 1 and np.isnan(c[9])
    t = ec.knee_scene("equal_adjacent").table
    assert t[6] == t[7] and t[-1] == t.max()
    assert ec.knee_scene("one_scale").nscales == 1 and ec.knee_scene("two_scales").nscales == 2


def test_small_k_scene_shows_the_divergence():
    """Sa/So ~ 1e-10: the reference's 1 - Sb/t curve is the K curve plus rounding noise of 1e-16 absolute, a visible share of
    means of 1e-11 .. 1e-9; Kneedle finds a knee in the noise.  The K-form curve (what the sweep kernel computes) is smooth and
    has none.  Both host implementations of the pick say so."""
    for name in ec.SMALL_K:
        sc = ec.knee_scene(name)
        assert sc.n == 4096 and np.array_equal(sc.table, np.arange(0.1, 10, 0.1))
        ck, cr = ec.knee_curve(sc, "K"), ec.knee_curve(sc, "ref")
        assert np.abs(ck - cr).max() <= ec.REF_FORM_ABS
        got = (ec.host_knee(sc.table, ck), ec.host_knee(sc.table, cr))
        assert got == (ec.oracle_knee(sc.table, ck), ec.oracle_knee(sc.table, cr)) == ec.SMALL_K_INDICES[name], (name, got)
    k, r = ec.SMALL_K_INDICES["small_k-1e-10"]
    assert k == 0 and r != 0


def test_host_knee_twin_on_tables_that_do_not_ascend():
    """knee_index takes any table.  It answers on one whose LAST point is its largest (the walk ends there, xn == 1), and on
    a descending one (the walk ends at its first point); it raises IndexError exactly where the walk reaches the last point
    of a table whose last entry is not its maximum -- the tables oisat_oi_fused refuses."""
    x = ec.UNIFORM99
    desc = x[::-1].copy()
    assert knee_index(desc, desc / (1 + desc)) == 74
    shuffled = x.copy()
    shuffled[[10, 40]] = shuffled[[40, 10]]                               # not ascending, the last still the maximum
    assert knee_index(shuffled, shuffled / (1 + shuffled)) == 10
    # the maximum in front, the difference curve rising to its only peak at the last point: the walk starts there, finds
    # xn != 1 and looks one element further
    bad = np.array([5.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    y = bad.copy()
    y[0] = 0.05
    with pytest.raises(IndexError):
        knee_index(bad, y)
    with pytest.raises(IndexError):
        orc.kneedle_knee(bad, y)
    # the same points with the maximum at the end: an answer
    good, yg = np.roll(bad, -1), np.roll(y, -1)
    assert knee_index(good, yg) == orc.kneedle_knee(good, yg)[1] == 5


# ---- C. apply and variances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ec.DTYPES, ids=ec.dt_name)
def test_apply_inputs_and_reference(dtype):
    assert ec.APPLY_NS == (1, 3, 255, 257, 2048 * 256 + 1)
    for n in (255, 257):
        arrs = ec.apply_inputs(n, dtype)
        sp = ec.SPECIALS.astype(dtype)
        for a in arrs:
            assert a.dtype == np.dtype(dtype) and a.size == n and np.isnan(a).any()
            for v in sp[~np.isnan(sp)]:
                assert ((a == v) & (np.signbit(a) == np.signbit(v))).any(), v
        Xa, Y, Sa, So = arrs
        T = np.dtype(dtype).type
        for scale in ec.APPLY_SCALES:
            Yc, xb, ak, inc, err = ec.apply_reference(Xa, Y, Sa, So, scale)
            # the clamp: -inf and negatives become 0, -0.0 and NaN stay
            neg = Y < 0
            assert neg.any() and (Yc[neg] == 0).all() and not np.signbit(Yc[neg]).any()
            assert ec.same_bits(Yc[~neg], Y[~neg]) and np.signbit(Yc[(Y == 0) & np.signbit(Y)]).all()
            # oracle.oi_fields in the dtype is the kernel's expression, one rounding per operation: (t + So) ** -1 is 1 / (t + So)
            with np.errstate(all="ignore"):
                t = Sa * T(scale)
                k = t * (T(1) / (t + So))
                sb = (T(1) - k) * t
                d = k * (Yc - Xa)
                mine = (Xa + d, T(1) - sb / t, d, np.sqrt(sb))
            for a, b in zip(mine, (xb, ak, inc, err)):
                assert ec.same_bits(a, b)
            assert np.isnan(ak).any() and (err == 0).any() and np.isfinite(xb).any()
    a, b = ec.apply_inputs(257, dtype), ec.apply_inputs(257, dtype)
    assert a is b                                                         # computed once, shared, read-only
    with pytest.raises(ValueError):
        a[0][0] = 1.0


def test_variances_reference():
    Xa = np.array([2.0, -3.0, np.nan, np.inf, 1e300, 5e-324, 0.1], dtype=np.float32)
    sa, so = ec.variances_reference(Xa, Xa, 50.0)
    assert sa.dtype == so.dtype == np.float32
    with np.errstate(all="ignore"):
        assert ec.same_bits(sa, ((Xa * np.float32(50)) / np.float32(100)) * ((Xa * np.float32(50)) / np.float32(100)))
        assert ec.same_bits(so, Xa * Xa)
    assert sa[0] == 1.0 and sa[1] == 2.25 and ec.VARIANCE_PCTS == (50.0, 0.1, 1e3)


# ---- D. stacks and months ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ec.DTYPES, ids=ec.dt_name)
def test_stack_family(dtype):
    cases = ec.stack_cases(dtype)
    assert len(cases) == 33 and {k for k, n in cases} == {1, 2, 31, 450}
    assert {n for k, n in cases if k == 31} == {1, 2, 3, 4, 5, 1023, 1024, 1025}
    big = ec.stack_big_n(dtype)
    N = 4 if np.dtype(dtype) == np.float32 else 2
    assert cases[-1] == (2, big) and big % N == 0 and big // N == 2048 * 256 + 1       # one vector beyond a full grid pass
    assert 2 * big * np.dtype(dtype).itemsize <= 16 * 2 ** 20 + 64                      # the largest buffer: 16 MB
    a = ec.stack_scene(31, 1025, dtype)
    ec.stack_scene.cache_clear()
    b = ec.stack_scene(31, 1025, dtype)
    assert a is not b and ec.same_bits(a, b) and a.dtype == np.dtype(dtype) and not a.flags.writeable
    assert np.isnan(a[:, :5]).all() and (~np.isnan(a[:, 5])).sum() == 1
    assert 0.10 < np.isnan(a[:, 6:]).mean() < 0.20 and np.isposinf(a).mean() > 0.015 and np.isneginf(a).mean() > 0.015
    for n in (1, 2, 3, 4, 5):
        s = ec.stack_scene(31, n, dtype)
        assert (~np.isnan(s)).any() and np.isnan(s[:, :n // 2]).all()
    if np.dtype(dtype) == np.float32:
        with np.errstate(all="ignore"):
            sq = a * a
        assert (np.isinf(sq) & np.isfinite(a)).sum() > 100 and np.abs(a[np.isfinite(a)]).max() > 1e24


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=ec.dt_name)
def test_stack_reference_and_its_mutants(dtype):
    """where every granule is finite the loop is np.mean's axis-0 order; each wrong restatement changes at least one bit"""
    rng = np.random.default_rng(3)
    clean = rng.uniform(0.1, 2.0, size=(31, 40)).astype(dtype)
    assert ec.same_bits(ec.stack_reference(clean, "mean", True), np.add.reduce(clean, axis=0) / np.dtype(dtype).type(31))
    st = ec.stack_scene(31, 1025, dtype)
    for kind, flag in (("mean", False), ("mean", True), ("err", False), ("err", True)):
        ref = ec.stack_reference(st, kind, flag)
        assert ref.dtype == st.dtype and np.isnan(ref[:5]).all() and np.isfinite(ref).sum() > (50 if kind == "mean" and not flag else 500)
        assert not ec.same_bits(ec.stack_reference(st, kind, flag, mutate="reverse_k"), ref), (kind, flag)
    assert not ec.same_bits(ec.stack_reference(st, "mean", False), ec.stack_reference(st, "mean", True))    # inf_to_nan matters
    lone = ec.stack_reference(st, "mean", True)[5]
    assert lone == np.dtype(dtype).type(0.75) and ec.stack_reference(st, "err", True)[5] == np.dtype(dtype).type(0.75)
    for flag in (False, True):
        ref = ec.stack_reference(st, "err", flag)
        assert not ec.same_bits(ec.stack_reference(st, "err", flag, mutate="count_inf"), ref)
    if np.dtype(dtype) == np.float32:                                     # squares that overflow: dropped only if tested after squaring
        ref = ec.stack_reference(st, "err", True)
        assert not ec.same_bits(ec.stack_reference(st, "err", True, mutate="square_after_test"), ref)


def test_month_scene_and_reference():
    fields, kept = ec.month_scene(1025)
    assert [f.dtype == np.float32 for f in fields] == [True, False, True, True, False] and ec.MONTH_F32_MASK == 13
    assert kept.dtype == np.int32 and kept.sum() == ec.MONTH_K - 2 and kept[0] == 0 and kept[15] == 0
    assert not ec.same_bits(fields[2], fields[3])
    for acc in ec.DTYPES:
        s, c, out = ec.month_reference(fields, kept, acc)
        assert s.dtype == out.dtype == np.dtype(acc) and c.dtype == np.uint32 and out.shape == (5, 1025)
        # the month is the stack of its kept granules, converted first
        for f, (kind, flag) in enumerate(ec.MONTH_FIELDS):
            with np.errstate(all="ignore"):
                st = fields[f][kept == 1].astype(acc)
            assert ec.same_bits(out[f], ec.stack_reference(st, kind, flag)), (acc, f)
        s1, c1, _ = ec.month_reference(fields, kept, acc, upto=1)
        assert not s1.any() and not c1.any()                              # granule 0 is skipped
        s15, c15, _ = ec.month_reference(fields, kept, acc, upto=15)
        s16, c16, _ = ec.month_reference(fields, kept, acc, upto=16)
        assert ec.same_bits(s15, s16) and np.array_equal(c15, c16) and c15.any()


def test_all_nan_and_widen_cases():
    assert ec.ALL_NAN_NS == (1, 255, 256, 257, 2048 * 256 + 1)
    for case in ec.ALL_NAN_CASES:
        for n in (1, 257):
            x, kept = ec.all_nan_case(case, n, np.float32)
            assert x.size == n and kept == int(case != "all_nan") and (~np.isnan(x)).sum() == kept
    x, _ = ec.all_nan_case("minus_zero", 257, np.float64)
    assert np.signbit(x[~np.isnan(x)]).all() and (x[~np.isnan(x)] == 0).all()
    w = ec.widen_input(2048 * 256 + 1)
    assert w.dtype == np.float32 and np.isnan(w).any() and np.isinf(w).any()
    tiny = np.abs(w[(w != 0) & ~np.isnan(w)]).min()
    assert tiny == np.float32(1.4e-45) and np.signbit(w[1]) and w[1] == 0
    assert ec.same_bits(ec.widen_input(100), ec.widen_input(100))


def test_every_family_reproduces_from_its_seed():
    a = [ec.knee_scene(n) for n in ("jittered64-r0.3", "small_k-1e-10", "equal_adjacent")]
    x = ec.apply_inputs(257, np.float32)
    ec.knee_scene.cache_clear()
    ec.apply_inputs.cache_clear()
    for old, name in zip(a, ("jittered64-r0.3", "small_k-1e-10", "equal_adjacent")):
        new = ec.knee_scene(name)
        assert new is not old
        for p, q in ((old.Sa, new.Sa), (old.So, new.So), (old.table, new.table)):
            np.testing.assert_array_equal(p, q)
    for p, q in zip(x, ec.apply_inputs(257, np.float32)):
        assert p is not q and ec.same_bits(p, q)
    f1, k1 = ec.month_scene(5)
    ec.stack_scene.cache_clear()
    f2, k2 = ec.month_scene(5)
    assert all(ec.same_bits(p, q) for p, q in zip(f1, f2)) and np.array_equal(k1, k2)
