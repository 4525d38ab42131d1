"""The far tier of the float64 sums, host side (``oisat_solve_tier_counts``, no device call): the query that restates the
kernels' bounding sphere and two-list staging (csrc/dense_solve_dev.inc: ``block_sphere``, ``stage_near``) against a NumPy
restatement written here, and a NumPy emulation of what the tier does to a patch's sums -- far pairs wholly in float32 --
at the library's constant and at a constant that is plainly too small."""
import ctypes as C
import functools

import numpy as np
import pytest

from oisatgmi import _hip, dense

L_KM = 300.0
CUT_BITS = 52.0
LOG2E = float(np.float32(1.4426950408889634))                  # the library's constant is a float
KEPT_BITS = 28.0                                                # kSolveFarBits (csrc/dense_solve_dev.inc)


def chord_of(g, bits):
    return np.sqrt(bits / (g * LOG2E))


def far_chord_of(g, bits):
    """chord(bits) rounded UP to a float; +inf where the tier is off (0 bits)."""
    if not (0.0 < bits <= CUT_BITS):
        return np.inf
    chord = chord_of(g, bits)
    f = np.float32(chord)
    if float(f) < chord:
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


def tiers_ref(g, bits, pts, obs, olat, lat_lo, lat_hi):
    """(near, far, staged mask, far mask) of one block of points; pts (3, npts), obs (3, m)."""
    m = obs.shape[1]
    cut = chord_of(g, CUT_BITS)
    win = 1e9 if cut >= 2.0 else 2.0 * np.arcsin(0.5 * cut) * 57.29577951308232
    windowed = olat is not None and win < 180.0
    j0, j1 = 0, m
    if windowed:
        j0 = int(np.searchsorted(olat, lat_lo - win, side="left"))
        j1 = int(np.searchsorted(olat, lat_hi + win + 1e-9, side="left"))
    s = np.array([np.cumsum(pts[k])[-1] for k in range(3)])    # point by point, as the host query sums
    nrm = np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    r2cull, r2far, c = 1e30, np.inf, np.zeros(3)
    if nrm > 1e-9 and windowed:
        c = s / nrm
        dx, dy, dz = pts[0] - c[0], pts[1] - c[1], pts[2] - c[2]
        rho = np.sqrt((dx * dx + dy * dy + dz * dz).max()) * (1.0 + 1e-12) + 1e-12
        r2cull = (cut + rho) ** 2
        fc = far_chord_of(g, bits)
        if fc < 1e9:
            r2far = (fc + rho) ** 2
    dx, dy, dz = obs[0] - c[0], obs[1] - c[1], obs[2] - c[2]
    q2 = dx * dx + dy * dy + dz * dz
    inwin = np.zeros(m, dtype=bool)
    inwin[j0:j1] = True
    staged = inwin & (q2 <= r2cull)
    far = staged & (q2 >= r2far)
    return int((staged & ~far).sum()), int(far.sum()), staged, far


def tiers_lib(g, bits, pts, obs, olat, lat_lo, lat_hi, kind=0):
    lib = _hip.load_library()
    pts, obs = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(obs, dtype=np.float64)
    near, far = C.c_int64(-1), C.c_int64(-1)
    rc = lib.oisat_solve_tier_counts(kind, C.c_double(g), C.c_double(bits), pts.ctypes.data, pts.shape[1], obs.ctypes.data, obs.shape[1],
                                     olat.ctypes.data if olat is not None else None, C.c_double(lat_lo), C.c_double(lat_hi),
                                     C.byref(near), C.byref(far))
    assert rc == 0, lib.oisat_last_error()
    return int(near.value), int(far.value)


@functools.lru_cache(maxsize=None)
def observations(m=100_000, seed=52):
    """m observations uniform on the sphere, in ascending latitude; weights N(0, 1)."""
    rng = np.random.default_rng(seed)
    lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, m)))
    lon = rng.uniform(-180.0, 180.0, m)
    o = np.argsort(lat, kind="stable")
    lat, lon = np.ascontiguousarray(lat[o]), lon[o]
    xyz = np.ascontiguousarray(dense.unit_vectors(lat, lon))
    w = rng.standard_normal(m)
    for a in (lat, xyz, w):
        a.setflags(write=False)
    return lat, xyz, w


def patch(lat0, lon0=10.0, rows=16, cols=32, step=0.25):
    """rows x cols cells of the 0.25 degree grid whose south-west cell centre is (lat0, lon0)."""
    la = lat0 + step * np.arange(rows)
    lo = lon0 + step * np.arange(cols)
    lat2, lon2 = np.meshgrid(la, lo, indexing="ij")
    return np.ascontiguousarray(dense.unit_vectors(lat2.ravel(), lon2.ravel())), float(la.min()), float(la.max())


def polar_ring():
    """The last 16 rows below the pole, 32 columns all around it: the centre IS the pole (well defined), the sphere a cap."""
    la = 86.125 + 0.25 * np.arange(16)
    lo = -180.0 + 11.25 * np.arange(32)
    lat2, lon2 = np.meshgrid(la, lo, indexing="ij")
    return np.ascontiguousarray(dense.unit_vectors(lat2.ravel(), lon2.ravel())), 86.125, 89.875


BLOCKS = {
    "equator": lambda: patch(-2.0),
    "60N": lambda: patch(58.0),
    "polar_cap": polar_ring,
    # a ring around the equator: the points' mean vanishes, there is no centre, hence no cull and nothing far
    "no_centre": lambda: (np.ascontiguousarray(dense.unit_vectors(np.zeros(32), -180.0 + 11.25 * np.arange(32))), 0.0, 0.0),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_counts_equal_the_numpy_restatement(name):
    olat, obs, _ = observations()
    g = dense.decay_constant(L_KM)
    pts, lo, hi = BLOCKS[name]()
    kept = None
    last_far = None
    for bits in (0.0, 4.0, 8.0, 12.0, 16.0, 20.0, 24.0, KEPT_BITS, 40.0, 52.0):
        want = tiers_ref(g, bits, pts, obs, olat, lo, hi)[:2]
        got = tiers_lib(g, bits, pts, obs, olat, lo, hi)
        print(f"{name} bits={bits:g}: near, far = {got}")
        assert got == want
        if kept is None:
            kept = sum(got)
            assert bits == 0.0 and got[1] == 0                  # the tier switched off: every staged pair is near
        assert sum(got) == kept                                 # near + far = what the 2^-52 cull keeps, whatever the bits
        if bits > 0.0:
            assert last_far is None or got[1] <= last_far       # a larger far chord: fewer far pairs
            last_far = got[1]
    if name == "no_centre":
        win = 2.0 * np.degrees(np.arcsin(0.5 * chord_of(g, CUT_BITS)))
        assert last_far == 0 and kept == int(((olat >= lo - win) & (olat < hi + win + 1e-9)).sum())
        assert tiers_lib(g, 16.0, pts, obs, olat, lo, hi) == (kept, 0)
    else:
        assert tiers_lib(g, 16.0, pts, obs, olat, lo, hi)[1] > 0 and tiers_lib(g, 52.0, pts, obs, olat, lo, hi)[1] == 0
        assert 0 < kept < olat.size


def test_an_empty_far_ring_no_window_and_the_other_model():
    olat, obs, _ = observations()
    g = dense.decay_constant(L_KM)
    pts, lo, hi = patch(-2.0)
    c = pts.mean(axis=1)
    c /= np.linalg.norm(c)
    close = ((obs - c[:, None]) ** 2).sum(axis=0) < chord_of(g, 8.0) ** 2           # everything within the 2^-8 chord of the centre
    assert close.sum() > 50
    sub, sublat = np.ascontiguousarray(obs[:, close]), np.ascontiguousarray(olat[close])
    for bits in (12.0, 16.0, KEPT_BITS):
        assert tiers_lib(g, bits, pts, sub, sublat, lo, hi) == (int(close.sum()), 0) == tiers_ref(g, bits, pts, sub, sublat, lo, hi)[:2]
    # no latitudes: no window, no cull, nothing far
    assert tiers_lib(g, 16.0, pts, obs, None, lo, hi) == (olat.size, 0)
    # Gaspari-Cohn has no far tier; its cull is its own
    n_gc, f_gc = tiers_lib(g, 16.0, pts, obs, olat, lo, hi, kind=1)
    assert f_gc == 0 and 0 < n_gc < sum(tiers_lib(g, 16.0, pts, obs, olat, lo, hi))
    # bits < 0: the library's setting -- the constant, unless the environment says otherwise
    assert tiers_lib(g, -1.0, pts, obs, olat, lo, hi) == tiers_lib(g, KEPT_BITS, pts, obs, olat, lo, hi)


def test_the_environment_sets_the_tier(monkeypatch):
    olat, obs, _ = observations()
    g = dense.decay_constant(L_KM)
    pts, lo, hi = patch(58.0)
    monkeypatch.setenv("OISAT_SOLVE_FAR_BITS", "0")
    assert tiers_lib(g, -1.0, pts, obs, olat, lo, hi)[1] == 0
    monkeypatch.setenv("OISAT_SOLVE_FAR_BITS", "12")
    assert tiers_lib(g, -1.0, pts, obs, olat, lo, hi) == tiers_lib(g, 12.0, pts, obs, olat, lo, hi)
    lib = _hip.load_library()
    for bad in ("-1", "53", "x", "12x"):
        monkeypatch.setenv("OISAT_SOLVE_FAR_BITS", bad)
        assert lib.oisat_solve_tier_counts(0, C.c_double(g), C.c_double(-1.0), pts.ctypes.data, pts.shape[1], obs.ctypes.data,
                                           obs.shape[1], olat.ctypes.data, C.c_double(lo), C.c_double(hi), None, None) != 0
    monkeypatch.delenv("OISAT_SOLVE_FAR_BITS")
    assert lib.oisat_solve_tier_counts(0, C.c_double(g), C.c_double(16.0), pts.ctypes.data, pts.shape[1], obs.ctypes.data,
                                       obs.shape[1], olat.ctypes.data, C.c_double(lo), C.c_double(hi), None, None) == 0


def emulate(g, bits, pts, obs, w, staged, far):
    """Per cell: near pairs in float64, far pairs wholly in float32 (coordinates, |p - q|^2, exp2, product, one fp32 partial
    sum in list order) added to the float64 sum; and the all-float64 sum over the same staged pairs."""
    g2 = g * LOG2E

    def terms64(sel):
        d2 = np.zeros((pts.shape[1], int(sel.sum())))
        for k in range(3):
            d2 += (pts[k][:, None] - obs[k][sel][None, :]) ** 2
        return np.exp2(-g2 * d2) * w[sel][None, :]

    full = terms64(staged).sum(axis=1)
    near = terms64(staged & ~far).sum(axis=1)
    p32, o32, w32 = pts.astype(np.float32), obs[:, far].astype(np.float32), w[far].astype(np.float32)
    d2 = np.zeros((pts.shape[1], o32.shape[1]), dtype=np.float32)
    for k in range(3):
        d = p32[k][:, None] - o32[k][None, :]
        d2 += d * d
    t32 = np.exp2(np.float32(-g2) * d2) * w32[None, :]
    assert t32.dtype == np.float32
    part = np.cumsum(t32, axis=1, dtype=np.float32)[:, -1] if t32.shape[1] else np.zeros(pts.shape[1], dtype=np.float32)
    return near + part.astype(np.float64), full


def test_emulated_sums_at_the_kept_constant_and_at_four_bits():
    """The deviation of a cell's sum from the all-float64 sum, as a fraction of the largest sum: at most 1e-9 at the kept
    constant (two orders below an fp32 ulp of the field even at swath densities, where sum|term| / |sum| is ~30 x larger
    than here), and at least 100 x that figure at 4 bits: a tier placed that badly is seen."""
    olat, obs, w = observations()
    g = dense.decay_constant(L_KM)
    pts, lo, hi = patch(-2.0)
    dev = {}
    for bits in (KEPT_BITS, 4.0):
        _, nfar, staged, far = tiers_ref(g, bits, pts, obs, olat, lo, hi)
        assert nfar > 0
        tiered, full = emulate(g, bits, pts, obs, w, staged, far)
        dev[bits] = np.abs(tiered - full).max() / np.abs(full).max()
        print(f"bits={bits:g}: far share {nfar / staged.sum():.3f}, deviation {dev[bits]:.2e}")
    assert dev[KEPT_BITS] <= 1e-9
    assert dev[4.0] >= 100.0 * dev[KEPT_BITS]
