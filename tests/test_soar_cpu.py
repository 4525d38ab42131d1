"""The SOAR (Matern nu = 3/2) correlation's host entry points (no GPU): ``oisat_corr_eval`` against (1 + s) exp(-s) in extended
precision, the cut chords, the ``_corr`` tables (the 2^-52 envelope, nothing above 2^-52 outside; far == first and mid == far
unless a variable forces a cut-off), the ``corr`` keyword, the tiled halo and the solve tiers (no far tier)."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

NB = 128
GAUSSIAN, GC, SOAR = 0, 1, 3
UNKNOWN = (2, 5, -1)
SIZES = [(385, 6385), (1000, 7000), (3000, 9000)]           # (observations, seed) on the 72 x 144 grid, as test_corr_cpu.py
LENGTHS = [100.0, 300.0, 3000.0]
CUT_S = {18: 15.265708, 28: 22.568011, 52: 39.751137}        # s = chord R / L at which (1 + s) exp(-s) = 2^-bits
FORCING = ("OISAT_FACTOR_CUT_BITS", "OISAT_FACTOR_FAR_BITS", "OISAT_FACTOR_MID_BITS")


def soar_ref(s):
    """(1 + s) exp(-s) in the platform's long double (64-bit mantissa on x86), rounded to float64."""
    s = np.asarray(s, dtype=np.longdouble)
    return ((1 + s) * np.exp(-s)).astype(np.float64)


def corr_eval(kind, g, d2):
    lib = _hip.load_library()
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    out = np.full(d2.size, np.nan)
    rc = lib.oisat_corr_eval(kind, C.c_double(g), d2.ctypes.data, d2.size, out.ctypes.data)
    assert rc == 0, lib.oisat_last_error()
    return out


def cut_chord(kind, g, bits):
    lib = _hip.load_library()
    out = C.c_double(-1.0)
    rc = lib.oisat_corr_cut_chord(kind, C.c_double(g), C.c_double(bits), C.byref(out))
    assert rc == 0, lib.oisat_last_error()
    return out.value


def table(name, kind, lat_sorted, g, *lower):
    """env (first | last) of the envelope functions; one table of nb words for the far (first) and mid (first, far) ones."""
    lib = _hip.load_library()
    nb = -(-lat_sorted.size // NB)
    out = np.full(nb if lower else 2 * nb, -7, dtype=np.int32)
    keep = [np.ascontiguousarray(t, dtype=np.int32) for t in lower]
    rc = getattr(lib, name)(kind, lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), *[t.ctypes.data for t in keep], out.ctypes.data)
    assert rc == 0, lib.oisat_last_error()
    return out


def sorted_obs(m, seed):
    p = syn.point_obs_case(72, 144, m, seed)
    o = np.argsort(p.obs_lat, kind="stable")
    return np.ascontiguousarray(p.obs_lat[o]), np.ascontiguousarray(p.obs_lon[o])


def forced_table(kind, lat, g, bits):
    """The searchsorted form of the table of cut-off 2^-bits (tests/test_corr_cpu.py)."""
    m, nb = lat.size, -(-lat.size // NB)
    ang = np.rad2deg(2.0 * np.arcsin(min(1.0, 0.5 * cut_chord(kind, g, bits))))
    ends = np.array([lat[min((k + 1) * NB, m) - 1] for k in range(nb)])
    return np.array([min(max(i - 1, 0), int(np.searchsorted(ends, lat[i * NB] - ang))) for i in range(nb)])


def test_soar_eval_against_the_formula():
    """Relative error <= (4 + 2 s) 2^-52 where the reference is above 1e-300: the sqrt and the product cost about 2 ulp, and
    exp turns a relative error in s into s times that."""
    s = np.linspace(0.0, 60.0, 100000)
    edge = [0.0, np.nextafter(0.0, 1.0), float(np.nextafter(np.float32(0), np.float32(1)))]
    s = np.concatenate([s, edge])
    worst = 0.0
    for L in LENGTHS:
        g = dense.decay_constant(L)
        d = s / np.sqrt(2.0 * g)
        d2 = d * d
        ss = np.sqrt(np.asarray(2.0 * g * d2, dtype=np.longdouble))     # the s the library is handed (d2 is its argument)
        got, ref = corr_eval(SOAR, g, d2), soar_ref(ss)
        ok = ref > 1e-300
        assert ok.sum() > s.size // 2
        rel = np.abs(got[ok] - ref[ok]) / ref[ok]
        bound = (4.0 + 2.0 * ss[ok].astype(np.float64)) * 2.0 ** -52
        worst = max(worst, float((rel / bound).max()))
        print(f"L = {L:g}: max relative error {rel.max():.3e}, at most {float((rel / bound).max()):.3f} of the bound")
        assert np.all(rel <= bound)
        assert np.all(np.abs(got[~ok] - ref[~ok]) <= 1e-300)
        o = np.argsort(d2, kind="stable")
        assert np.all(np.diff(got[o]) <= 0.0)                   # monotone non-increasing in s
        assert np.all((got >= 0.0) & (got <= 1.0))
        assert corr_eval(SOAR, g, [0.0])[0] == 1.0
    assert worst > 0.0                                           # (something was compared)


def test_soar_curvature_is_the_gaussian_s():
    g = dense.decay_constant(300.0)
    d2 = np.array([1e-8, 1e-7])
    assert np.allclose(1.0 - corr_eval(SOAR, g, d2), g * d2, rtol=2e-2)


def test_cut_chords():
    for L in LENGTHS:
        g = dense.decay_constant(L)
        for bits, want in CUT_S.items():
            chord = cut_chord(SOAR, g, bits)
            s = chord * np.sqrt(2.0 * g)
            assert abs(s - want) <= 1e-6, (bits, s)
            assert corr_eval(SOAR, g, [chord * chord])[0] <= 2.0 ** -bits * (1.0 + 1e-12)      # the upper end of the bracket
            assert corr_eval(SOAR, g, [(chord * (1.0 - 1e-9)) ** 2])[0] > 2.0 ** -bits           # ... and a tight one
        # the Gaussian's and Gaspari-Cohn's chords are what they were
        per_z = 1.0 / np.sqrt(0.6 * g)
        for bits, z in ((18, 1.940624), (28, 1.989543)):
            assert abs(cut_chord(GC, g, bits) / per_z - z) <= 1e-6
        assert cut_chord(GC, g, 52) == 2.0 * per_z
        for bits in (18, 28, 52):
            assert cut_chord(GAUSSIAN, g, bits) == pytest.approx(np.sqrt(bits / (g * np.log2(np.e))), rel=1e-7)
    # not clamped to the sphere's diameter: L = 3000 km reaches 2^-52 at a chord of 18.7
    assert cut_chord(SOAR, dense.decay_constant(3000.0), 52) == pytest.approx(39.751137 * 3000.0 / dense.EARTH_RADIUS_KM, rel=1e-7)
    assert cut_chord(SOAR, dense.decay_constant(300.0), 52) == pytest.approx(1.8718, abs=1e-4)


def test_unknown_kinds_are_still_errors():
    lib = _hip.load_library()
    lat = np.array([0.0, 1.0])
    first = np.zeros(1, dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)
    d2, c = np.zeros(1), np.zeros(1)
    chord = C.c_double(0.0)
    g = C.c_double(1.0)
    pts = np.ascontiguousarray(dense.unit_vectors([0.0], [0.0]))
    for kind in UNKNOWN:
        assert lib.oisat_corr_eval(kind, g, d2.ctypes.data, 1, c.ctypes.data) != 0
        assert lib.oisat_corr_cut_chord(kind, g, C.c_double(28.0), C.byref(chord)) != 0
        assert lib.oisat_envelope_corr(kind, lat.ctypes.data, 2, g, out.ctypes.data) != 0
        assert lib.oisat_factor_envelope_corr(kind, lat.ctypes.data, 2, g, out.ctypes.data) != 0
        assert lib.oisat_factor_far_corr(kind, lat.ctypes.data, 2, g, first.ctypes.data, out.ctypes.data) != 0
        assert lib.oisat_factor_mid_corr(kind, lat.ctypes.data, 2, g, first.ctypes.data, first.ctypes.data, out.ctypes.data) != 0
        assert lib.oisat_solve_tier_counts(kind, g, C.c_double(0.0), pts.ctypes.data, 1, pts.ctypes.data, 1, None, C.c_double(0.0),
                                           C.c_double(0.0), None, None) != 0
    for kind in (GAUSSIAN, GC, SOAR):                           # (the same calls are fine for a model)
        assert lib.oisat_envelope_corr(kind, lat.ctypes.data, 2, g, out.ctypes.data) == 0
        assert lib.oisat_factor_mid_corr(kind, lat.ctypes.data, 2, g, first.ctypes.data, first.ctypes.data, out.ctypes.data) == 0


@pytest.mark.parametrize("m,seed", SIZES)
@pytest.mark.parametrize("L", LENGTHS)
def test_soar_tables_hold_every_pair_above_the_cut(m, seed, L, monkeypatch):
    for v in FORCING:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.delenv("OISAT_ENVELOPE", raising=False)
    lat, lon = sorted_obs(m, seed)
    g = dense.decay_constant(L)
    nb = -(-m // NB)
    env = table("oisat_envelope_corr", SOAR, lat, g)
    first, last = env[:nb].astype(np.int64), env[nb:].astype(np.int64)
    assert np.all(np.diff(first) >= 0) and np.all(first >= 0) and np.all(first <= np.maximum(np.arange(nb) - 1, 0))
    for b in range(nb):
        assert last[b] == np.flatnonzero(first <= b).max()
    xyz = dense.unit_vectors(lat, lon)
    d2 = ((xyz[:, :, None] - xyz[:, None, :]) ** 2).sum(axis=0)
    s = np.sqrt(2.0 * g * d2)
    above = (1.0 + s) * np.exp(-s) > 2.0 ** -52
    for i in range(nb):                                        # brute force over the 128-blocks left of the table
        assert not above[i * NB:(i + 1) * NB, :first[i] * NB].any(), (i, first[i])
    if L == 3000.0:
        assert not first.any()                                  # the chord is beyond the diameter: nothing is windowed
    if (m, L) == (385, 100.0):
        assert first.tolist() == [0, 0, 0, 2]                   # (the GPU test's envelope case really drops a tile)
    # by default: the factor's envelope is this table, no far stretch, no middle stretch
    assert np.array_equal(table("oisat_factor_envelope_corr", SOAR, lat, g), env)
    far = table("oisat_factor_far_corr", SOAR, lat, g, first)
    assert np.array_equal(far, first)
    assert np.array_equal(table("oisat_factor_mid_corr", SOAR, lat, g, first, far), far)
    assert np.array_equal(first, forced_table(SOAR, lat, g, 52))
    # the three variables still force their rules, through the model's own cut chord
    monkeypatch.setenv("OISAT_FACTOR_CUT_BITS", "18")
    forced = table("oisat_factor_envelope_corr", SOAR, lat, g)[:nb]
    assert np.all(forced >= first)
    assert np.array_equal(forced, forced_table(SOAR, lat, g, 18))
    monkeypatch.delenv("OISAT_FACTOR_CUT_BITS")
    monkeypatch.setenv("OISAT_FACTOR_FAR_BITS", "18")
    far = table("oisat_factor_far_corr", SOAR, lat, g, first)
    assert np.array_equal(far, np.minimum(np.maximum(forced, first), np.arange(nb)))
    monkeypatch.setenv("OISAT_FACTOR_MID_BITS", "8")
    mid = table("oisat_factor_mid_corr", SOAR, lat, g, first, far)
    assert np.array_equal(mid, np.minimum(np.maximum(forced_table(SOAR, lat, g, 8), far), np.arange(nb)))
    if L == 100.0 and m >= 1000:
        assert (far > first).any() and (mid > far).any()        # (the forced tables are not the default ones)


def test_python_names_and_the_tiled_halo():
    assert dense.corr_kind("soar") == 3 and dense.CORRELATIONS["soar"] == 3
    assert dense.corr_kind("gaussian") == 0 and dense.corr_kind("gaspari_cohn") == 1
    with pytest.raises(ValueError, match="corr"):
        dense.corr_kind("matern")
    h = dense.SOAR_HALO_PER_L
    assert h == pytest.approx(6.5172, rel=1e-4)
    assert (1.0 + h) * np.exp(-h) == pytest.approx(np.exp(-4.5), rel=1e-12)        # the Gaussian's value at its 3 L halo


@pytest.mark.parametrize("L", [100.0, 300.0])
def test_solve_tiers_have_no_far_tier(L):
    """near_out = the observations of the latitude window within the 2^-52 chord of the block's bounding sphere (centre: the
    normalised mean, radius: the largest chord to it, with the margins of tests/test_solve_tiers_cpu.py); far_out = 0."""
    rng = np.random.default_rng(52)
    m = 20000
    olat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, m)))
    lon = rng.uniform(-180.0, 180.0, m)
    o = np.argsort(olat, kind="stable")
    olat = np.ascontiguousarray(olat[o])
    obs = np.ascontiguousarray(dense.unit_vectors(olat, lon[o]))
    g = dense.decay_constant(L)
    cut = cut_chord(SOAR, g, 52)
    assert cut < 2.0
    win = 2.0 * np.arcsin(0.5 * cut) * 57.29577951308232
    lib = _hip.load_library()
    for lat0 in (-2.0, 58.0, 84.0):
        la, lo = lat0 + 0.25 * np.arange(16), 10.0 + 0.25 * np.arange(32)
        lat2, lon2 = np.meshgrid(la, lo, indexing="ij")
        pts = np.ascontiguousarray(dense.unit_vectors(lat2.ravel(), lon2.ravel()))
        c = np.array([np.cumsum(pts[k])[-1] for k in range(3)])
        c /= np.sqrt((c * c).sum())
        rho = np.sqrt(((pts - c[:, None]) ** 2).sum(axis=0).max()) * (1.0 + 1e-12) + 1e-12
        inwin = (olat >= la.min() - win) & (olat < la.max() + win + 1e-9)
        want = int((inwin & (((obs - c[:, None]) ** 2).sum(axis=0) <= (cut + rho) ** 2)).sum())
        for bits in (-1.0, 0.0, 16.0, 28.0):
            near, far = C.c_int64(-1), C.c_int64(-1)
            rc = lib.oisat_solve_tier_counts(SOAR, C.c_double(g), C.c_double(bits), pts.ctypes.data, pts.shape[1], obs.ctypes.data, m,
                                             olat.ctypes.data, C.c_double(la.min()), C.c_double(la.max()), C.byref(near), C.byref(far))
            assert rc == 0, lib.oisat_last_error()
            assert far.value == 0
            assert near.value == want
        print(f"L = {L:g}, lat0 = {lat0:g}: near = {want} of {m}")
        assert 0 < want
        if L == 100.0:
            assert want < m // 2                                # (the cull really culls)
