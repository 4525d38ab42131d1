"""The correlation model's host entry points (no GPU): ``oisat_corr_eval`` against the float64 formula of Gaspari and Cohn
(1999, eq. 4.10), the cut chords, the ``_corr`` tables (kind 0 = the existing tables word for word; kind 1 = the support
envelope, nothing with C > 0 outside) and the ``corr`` keyword's validation."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

NB = 128
GAUSSIAN, GC = 0, 1
SIZES = [(385, 6385), (1000, 7000), (3000, 9000)]           # (observations, seed) on the 72 x 144 grid
LENGTHS = [300.0, 500.0, 3000.0]


def gc_ref(z):
    """Gaspari-Cohn (1999), eq. 4.10, in z = distance / c, float64, the formula as printed."""
    z = np.asarray(z, dtype=np.float64)
    near = -z ** 5 / 4 + z ** 4 / 2 + 5 * z ** 3 / 8 - 5 * z ** 2 / 3 + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        far = z ** 5 / 12 - z ** 4 / 2 + 5 * z ** 3 / 8 + 5 * z ** 2 / 3 - 5 * z + 4 - 2 / (3 * z)
    return np.where(z <= 1, near, np.where(z < 2, np.maximum(far, 0.0), 0.0))


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


def table(name, kind, lat_sorted, g, first=None):
    lib = _hip.load_library()
    nb = -(-lat_sorted.size // NB)
    out = np.full(nb if first is not None else 2 * nb, -7, dtype=np.int32)
    fn = getattr(lib, name)
    args = [lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g)]
    if first is not None:
        args.append(np.ascontiguousarray(first, dtype=np.int32).ctypes.data)
    rc = fn(*(([kind] if kind is not None else []) + args + [out.ctypes.data]))
    assert rc == 0, lib.oisat_last_error()
    return out


def sorted_obs(m, seed):
    p = syn.point_obs_case(72, 144, m, seed)
    o = np.argsort(p.obs_lat, kind="stable")
    return np.ascontiguousarray(p.obs_lat[o]), np.ascontiguousarray(p.obs_lon[o])


def test_gaspari_cohn_eval_against_the_formula():
    """|C - C_ref| <= 1e-13: terms <= 10, fewer than 20 roundings of 1.1e-16 bound the error by 2.2e-14 (4x headroom)."""
    z = np.linspace(0.0, 2.5, 100000)
    edge = []
    for v in (0.0, 1.0, 2.0):
        edge += [v, np.nextafter(v, -1.0), np.nextafter(v, 3.0), np.float64(np.nextafter(np.float32(v), np.float32(-1))),
                 np.float64(np.nextafter(np.float32(v), np.float32(3)))]
    z = np.concatenate([z, np.abs(np.array(edge))])
    for g in (dense.decay_constant(300.0), dense.decay_constant(3000.0), 1.0 / 0.6):
        d = z / np.sqrt(0.6 * g)
        d2 = d * d
        zz = np.sqrt(0.6 * g * d2)                             # the z the library is handed (d2 is its argument)
        got = corr_eval(GC, g, d2)
        ref = gc_ref(zz)
        err = np.abs(got - ref).max()
        print(f"g = {g:.4g}: max |C - C_ref| = {err:.3e}")
        assert err <= 1e-13
        assert np.all(got >= 0.0)
        assert np.all(got[zz >= 2.0] == 0.0)
    assert corr_eval(GC, 1.0 / 0.6, [0.0])[0] == 1.0


def test_gaussian_eval_is_exp():
    g = dense.decay_constant(500.0)
    d2 = np.linspace(0.0, 4.0, 100001)
    got, ref = corr_eval(GAUSSIAN, g, d2), np.exp(-g * d2)
    ok = ref > 1e-300
    assert np.all(np.abs(got[ok] - ref[ok]) <= 4 * np.spacing(ref[ok]))
    assert np.all(np.abs(got[~ok] - ref[~ok]) <= 1e-300)


def test_cut_chords():
    for L in LENGTHS:
        g = dense.decay_constant(L)
        per_z = 1.0 / np.sqrt(0.6 * g)
        for bits, z in ((18, 1.940624), (28, 1.989543)):
            got = cut_chord(GC, g, bits) / per_z
            assert abs(got - z) <= 1e-6, (bits, got)
            assert gc_ref(got) <= 2.0 ** -bits + 1e-13          # the upper end of the bracket (to the evaluation's rounding)
        assert cut_chord(GC, g, 52) == 2.0 * per_z              # the support chord itself: nothing is left out
        assert cut_chord(GC, g, 40) < 2.0 * per_z
        for bits in (18, 28, 52):
            # (the library holds log2 e as a float: 2^-24 relative in g2, half of it in the chord)
            assert cut_chord(GAUSSIAN, g, bits) == pytest.approx(np.sqrt(bits / (g * np.log2(np.e))), rel=1e-7)
    lib = _hip.load_library()
    out = C.c_double(0.0)
    assert lib.oisat_corr_cut_chord(2, C.c_double(1.0), C.c_double(28.0), C.byref(out)) != 0        # unknown kind
    assert lib.oisat_corr_eval(-1, C.c_double(1.0), None, 0, None) != 0


@pytest.mark.parametrize("m,seed", SIZES)
@pytest.mark.parametrize("L", LENGTHS)
def test_gaussian_tables_are_the_existing_ones(m, seed, L, monkeypatch):
    monkeypatch.delenv("OISAT_FACTOR_CUT_BITS", raising=False)
    monkeypatch.delenv("OISAT_FACTOR_FAR_BITS", raising=False)
    lat, _ = sorted_obs(m, seed)
    g = dense.decay_constant(L)
    for old, new in (("oisat_envelope", "oisat_envelope_corr"), ("oisat_factor_envelope", "oisat_factor_envelope_corr")):
        assert np.array_equal(table(old, None, lat, g), table(new, GAUSSIAN, lat, g))
    nb = -(-m // NB)
    first = table("oisat_factor_envelope", None, lat, g)[:nb]
    assert np.array_equal(table("oisat_factor_far", None, lat, g, first), table("oisat_factor_far_corr", GAUSSIAN, lat, g, first))
    monkeypatch.setenv("OISAT_FACTOR_CUT_BITS", "28")          # ... and under the overrides
    monkeypatch.setenv("OISAT_FACTOR_FAR_BITS", "18")
    forced = table("oisat_factor_envelope", None, lat, g)
    assert np.array_equal(forced, table("oisat_factor_envelope_corr", GAUSSIAN, lat, g))
    assert np.array_equal(table("oisat_factor_far", None, lat, g, forced[:nb]),
                          table("oisat_factor_far_corr", GAUSSIAN, lat, g, forced[:nb]))


@pytest.mark.parametrize("m,seed", SIZES)
@pytest.mark.parametrize("L", LENGTHS)
def test_gaspari_cohn_tables_hold_every_nonzero_pair(m, seed, L, monkeypatch):
    monkeypatch.delenv("OISAT_FACTOR_CUT_BITS", raising=False)
    monkeypatch.delenv("OISAT_FACTOR_FAR_BITS", raising=False)
    lat, lon = sorted_obs(m, seed)
    g = dense.decay_constant(L)
    nb = -(-m // NB)
    env = table("oisat_envelope_corr", GC, lat, g)
    first, last = env[:nb].astype(np.int64), env[nb:].astype(np.int64)
    assert np.all(np.diff(first) >= 0) and np.all(first >= 0) and np.all(first <= np.maximum(np.arange(nb) - 1, 0))
    for b in range(nb):
        assert last[b] == np.flatnonzero(first <= b).max()
    xyz = dense.unit_vectors(lat, lon)
    d2 = ((xyz[:, :, None] - xyz[:, None, :]) ** 2).sum(axis=0)
    nonzero = gc_ref(np.sqrt(0.6 * g * d2)) > 0.0
    for i in range(nb):                                        # brute force over the 128-blocks left of the table
        assert not nonzero[i * NB:(i + 1) * NB, :first[i] * NB].any(), (i, first[i])
    assert np.array_equal(table("oisat_factor_envelope_corr", GC, lat, g), env)
    assert np.array_equal(table("oisat_factor_far_corr", GC, lat, g, first), first)
    # the Gaussian's float64 table reaches further (8.49 L against 3.65 L)
    assert np.all(table("oisat_envelope_corr", GAUSSIAN, lat, g)[:nb] <= first)
    # the overrides still force their rules, through the model's own cut chord
    monkeypatch.setenv("OISAT_FACTOR_CUT_BITS", "18")
    forced = table("oisat_factor_envelope_corr", GC, lat, g)[:nb]
    assert np.all(forced >= first)
    ang = np.rad2deg(2.0 * np.arcsin(min(1.0, 0.5 * cut_chord(GC, g, 18))))
    want = [min(max(i - 1, 0), int(np.searchsorted(np.array([lat[min((k + 1) * NB, m) - 1] for k in range(nb)]), lat[i * NB] - ang)))
            for i in range(nb)]
    assert np.array_equal(forced, want)
    monkeypatch.delenv("OISAT_FACTOR_CUT_BITS")
    monkeypatch.setenv("OISAT_FACTOR_FAR_BITS", "18")
    far = table("oisat_factor_far_corr", GC, lat, g, first)
    assert np.array_equal(far, np.minimum(np.maximum(forced, first), np.arange(nb)))


def test_unknown_model_is_a_value_error():
    p = syn.point_obs_case(18, 36, 40, 5)
    obs = {"lat": p.obs_lat, "lon": p.obs_lon, "y": p.obs_y, "var": p.obs_var}
    with pytest.raises(ValueError, match="corr"):
        dense.OI_dense(p.Xa, None, p.Sa, None, p.lat, p.lon, 500.0, obs=obs, corr="bogus")
    Y = np.full(p.Xa.shape, np.nan)
    with pytest.raises(ValueError, match="corr"):
        dense.OI_tiled(p.Xa, Y, p.Sa, Y.copy(), p.lat, p.lon, 500.0, corr="bogus")
    assert dense.corr_kind("gaussian") == 0 and dense.corr_kind("gaspari_cohn") == 1
    lib = _hip.load_library()
    lat = np.array([0.0, 1.0])
    out = np.zeros(2, dtype=np.int32)
    assert lib.oisat_envelope_corr(5, lat.ctypes.data, 2, C.c_double(1.0), out.ctypes.data) != 0
