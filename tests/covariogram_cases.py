"""What the covariogram tests share: the NumPy restatement of ``oisat_covariogram``'s pair rule (never the library), the Python
restatement of its quanta, point sets, and the correlated field of the end-to-end cases.  Everything is float64 on the host."""
import functools
import math

import numpy as np

R_EARTH = 6371.0


def quanta_ref(umax, m):
    """include/oisat.h: q_prod = 2^(e - 62), e = frexp exponent of umax * umax * (double)P (1 if that is 0); q_chord likewise of
    2.0 * max(P, 1)."""
    P = m * (m - 1) // 2
    prod = float(umax) * float(umax) * float(P)
    q_prod = 1.0 if prod == 0.0 else math.ldexp(1.0, math.frexp(prod)[1] - 62)
    q_chord = math.ldexp(1.0, math.frexp(2.0 * float(max(P, 1)))[1] - 62)
    return q_prod, q_chord


def unit_vectors(lat, lon):
    la, lo = np.deg2rad(lat), np.deg2rad(lon)
    return np.ascontiguousarray(np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)]))


def cap_points(rng, m, cap_deg):
    """(3, m) unit vectors, uniform on a cap of half-angle ``cap_deg`` about an axis that is no coordinate axis."""
    cz = rng.uniform(np.cos(np.deg2rad(cap_deg)), 1.0, m)
    ph = rng.uniform(0.0, 2.0 * np.pi, m)
    s = np.sqrt(1.0 - cz * cz)
    p = np.stack([s * np.cos(ph), s * np.sin(ph), cz])
    a, b = np.deg2rad(37.0), np.deg2rad(-61.0)                  # rotate about x, then about z
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return np.ascontiguousarray(rz @ rx @ p)


def global_points(rng, m):
    """(lat, lon) in degrees, uniform on the sphere, ascending latitude."""
    lat = np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0, m)))
    lon = rng.uniform(-180.0, 180.0, m)
    o = np.argsort(lat, kind="stable")
    return lat[o], lon[o]


def pairs(xyz, u, max_chord, nbins):
    """The pair rule on ``np.triu_indices`` pairs of the used observations, same operation order: (k, chord, u_a u_b, t, d2)."""
    idx = np.flatnonzero(np.isfinite(u))
    ia, ib = np.triu_indices(idx.size, 1)
    a, b = idx[ia], idx[ib]
    dx, dy, dz = xyz[0][a] - xyz[0][b], xyz[1][a] - xyz[1][b], xyz[2][a] - xyz[2][b]
    d2 = dx * dx + dy * dy + dz * dz
    chord = np.sqrt(d2)
    t = chord * (nbins / max_chord)
    return t.astype(np.int64), chord, u[a] * u[b], t, d2


def assert_no_pair_on_an_edge(t, d2, nbins):
    """No used pair within 1e-9 of a bin edge or of the last one: a last-bit difference in the device's sqrt cannot then move a
    pair across an edge.  (A pair of identical points has d2 = 0 and chord = 0 exactly on either side: sqrt(0) has no last bit.)"""
    tt = t[d2 > 0.0]
    if tt.size:
        assert np.abs(tt - np.rint(tt)).min() >= 1e-9, "a pair sits on a bin edge: choose another seed"
        assert np.abs(tt - nbins).min() >= 1e-9, "a pair sits on max_chord: choose another seed"


def ref_covariogram(xyz, u, max_chord, nbins):
    """-> (count int64[nbins], sum_prod, sum_chord) with counts by ``np.bincount`` and sums by ``math.fsum`` per bin; asserts the
    edge condition first."""
    k, chord, prod, t, d2 = pairs(xyz, u, max_chord, nbins)
    assert_no_pair_on_an_edge(t, d2, nbins)
    keep = k < nbins
    k, chord, prod = k[keep], chord[keep], prod[keep]
    count = np.bincount(k, minlength=nbins).astype(np.int64)
    o = np.argsort(k, kind="stable")
    cuts = np.cumsum(count)[:-1]
    sp = np.array([math.fsum(x) for x in np.split(prod[o], cuts)])
    sc = np.array([math.fsum(x) for x in np.split(chord[o], cuts)])
    return count, sp, sc


def covariogram_dict(count, sp, sc, max_km, nobs, var0, q_prod, q_chord):
    """The dict of ``dense.innovation_covariogram`` from host sums."""
    with np.errstate(invalid="ignore", divide="ignore"):
        chord = np.where(count > 0, sc / np.maximum(count, 1), np.nan)
        cov = np.where(count > 0, sp / np.maximum(count, 1), np.nan)
    return {"chord": chord, "r_km": R_EARTH * chord, "cov": cov, "count": count, "nobs": nobs, "var0": var0, "q_prod": q_prod,
            "q_chord": q_chord, "max_km": float(max_km), "nbins": int(count.size)}


END_TO_END = dict(m=1500, L0=400.0, seed=20261, max_km=2000.0, nbins=64)


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    """A field drawn from the Gaussian model at L0 = 400 km at 1500 random global points: u = chol(0.6 C + 0.4 I) xi, float64.
    -> (lat, lon, u, reference count / sum_prod / sum_chord), computed once and shared (read-only)."""
    c = END_TO_END
    rng = np.random.default_rng(c["seed"])
    lat, lon = global_points(rng, c["m"])
    p = unit_vectors(lat, lon)
    d2 = np.zeros((c["m"], c["m"]))
    for k in range(3):
        d2 += (p[k][:, None] - p[k][None, :]) ** 2
    S = 0.6 * np.exp(-0.5 * (R_EARTH / c["L0"]) ** 2 * d2) + 0.4 * np.eye(c["m"])
    u = np.linalg.cholesky(S) @ rng.normal(size=c["m"])
    count, sp, sc = ref_covariogram(p, u, c["max_km"] / R_EARTH, c["nbins"])
    for a in (lat, lon, u, count, sp, sc):
        a.setflags(write=False)
    return lat, lon, u, count, sp, sc
