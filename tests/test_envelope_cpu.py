"""The covariance's latitude envelope (``oisat_envelope``, host only): shape of the table, nothing above the cut-off is
left outside it, and the tile / K-step counts of the benchmark's headline system."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

NB = 128
# (name, ny, nx, nobs, seed, L_km, swaths): the three benchmark workloads (bench.py WORKLOADS, seed 4000) and a swath case
CASES = [
    ("config3", 720, 1440, 100000, 4000, 300.0, True),
    ("config2", 360, 720, 10000, 4000, 500.0, False),
    ("config1", 72, 144, 1000, 4000, 500.0, False),
    ("swath_20k", 180, 360, 20000, 11, 300.0, True),
]


def envelope(lat_sorted, g):
    lib = _hip.load_library()
    nb = -(-lat_sorted.size // NB)
    env = np.full(2 * nb, -1, dtype=np.int32)
    rc = lib.oisat_envelope(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data)
    assert rc == 0, lib.oisat_last_error()
    return env[:nb].astype(np.int64), env[nb:].astype(np.int64)


def counts(first):
    """Counting rule of the issue: tiles = sum_i (i - first[i] + 1); K-steps = sum_i sum_{j = first[i] .. i} (j - max(first[i], first[j]))."""
    nt = first.size
    tiles = int(np.sum(np.arange(nt) - first + 1))
    ksteps = 0
    for i in range(nt):
        j = np.arange(first[i], i + 1)
        ksteps += int(np.sum(j - np.maximum(first[i], first[j])))
    return tiles, ksteps


def sorted_obs(case):
    _, ny, nx, nobs, seed, L, swaths = case
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    lat = np.ravel(np.asarray(p.obs_lat, dtype=np.float64))
    o = np.argsort(lat, kind="stable")
    return np.ascontiguousarray(lat[o]), np.ravel(p.obs_lon)[o], dense.decay_constant(L)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_envelope_shape_and_cut_off(case):
    lat, lon, g = sorted_obs(case)
    first, last = envelope(lat, g)
    nt = first.size
    assert nt == -(-lat.size // NB)
    assert np.all(np.diff(first) >= 0)
    assert np.all(first >= 0) and np.all(first <= np.maximum(np.arange(nt) - 1, 0))
    for b in range(nt):                                       # last[b] = max{ j : first[j] <= b }
        assert last[b] == np.flatnonzero(first <= b).max()
    # every pair outside the envelope: float64 correlation below 2^-52 (by chunks: tile row i against all rows left of it)
    xyz = dense.unit_vectors(lat, lon)                         # [3][m]
    worst = 0.0
    for i in range(nt):
        ncol = int(first[i]) * NB
        if ncol == 0:
            continue
        a = xyz[:, i * NB:(i + 1) * NB]
        d2min = np.inf
        for c0 in range(0, ncol, 16384):
            b = xyz[:, c0:min(c0 + 16384, ncol)]
            d2 = ((a[:, :, None] - b[:, None, :]) ** 2).sum(axis=0)
            d2min = min(d2min, float(d2.min()))
        worst = max(worst, float(np.exp(-g * d2min)))
    print(f"{case[0]}: {nt} tile rows, largest correlation outside the envelope {worst:.3e}")
    assert worst < 2.0 ** -52


def test_headline_counts():
    """config 3: 82 651 of 305 371 tiles and 4 549 882 of 79 396 460 K-loop steps (the issue's table), or fewer."""
    lat, _, g = sorted_obs(CASES[0])
    first, _ = envelope(lat, g)
    tiles, ksteps = counts(first)
    dense_tiles, dense_k = counts(np.zeros_like(first))
    print(f"config3: tiles {tiles} / {dense_tiles}, K-steps {ksteps} / {dense_k}")
    assert (dense_tiles, dense_k) == (305371, 79396460)
    assert tiles <= 82651 and ksteps <= 4549882


def test_envelope_rejects_unsorted_latitudes():
    lib = _hip.load_library()
    lat = np.array([0.0, 1.0, 0.5])
    env = np.zeros(2, dtype=np.int32)
    assert lib.oisat_envelope(lat.ctypes.data, 3, C.c_double(1.0), env.ctypes.data) != 0
