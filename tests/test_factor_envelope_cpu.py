"""The fp32 factor's own envelope (``oisat_factor_envelope``, host only): the override at 52 reproduces ``oisat_envelope``,
the chosen cut-off leaves nothing above 2^-28 outside, only systems bound by tile work get the narrow table, and a host
emulation of the refined solve (fp32 LAPACK factor of the zero-filled fp32 S as preconditioner, float64 sweeps and residual
of the full S) shows the refinement does not see the cut-off."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn
from oracle import oi_oracle as orc
from test_envelope_cpu import CASES, NB, counts, envelope, sorted_obs

FACTOR_CUT_BITS = 28               # kFactorCutBits (csrc/dense_tables.hip)
HEADLINE_KSTEPS = 2520648          # config 3 at 2^-28, counted with the rule of test_envelope_cpu.counts (4 549 882 at 2^-52)
OVERRIDE = "OISAT_FACTOR_CUT_BITS"


def factor_envelope(lat_sorted, g):
    lib = _hip.load_library()
    nb = -(-lat_sorted.size // NB)
    env = np.full(2 * nb, -1, dtype=np.int32)
    rc = lib.oisat_factor_envelope(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data)
    assert rc == 0, lib.oisat_last_error()
    return env[:nb].astype(np.int64), env[nb:].astype(np.int64)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_override_at_52_is_the_float64_table(case, monkeypatch):
    lat, _, g = sorted_obs(case)
    monkeypatch.setenv(OVERRIDE, "52")
    first, last = factor_envelope(lat, g)
    first52, last52 = envelope(lat, g)
    assert np.array_equal(first, first52) and np.array_equal(last, last52)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forced_narrow_table_shape_and_cut_off(case, monkeypatch):
    lat, lon, g = sorted_obs(case)
    monkeypatch.setenv(OVERRIDE, str(FACTOR_CUT_BITS))
    first, last = factor_envelope(lat, g)
    first52, _ = envelope(lat, g)
    nt = first.size
    assert nt == -(-lat.size // NB)
    assert np.all(np.diff(first) >= 0)
    assert np.all(first >= 0) and np.all(first <= np.maximum(np.arange(nt) - 1, 0))
    for b in range(nt):                                       # last[b] = max{ j : first[j] <= b }
        assert last[b] == np.flatnonzero(first <= b).max()
    assert np.all(first >= first52)
    # every pair outside the table: float64 correlation below 2^-28 (by chunks: tile row i against all rows left of it)
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
    print(f"{case[0]}: {nt} tile rows, largest correlation outside the factor's table {worst:.3e}")
    assert worst < 2.0 ** -FACTOR_CUT_BITS


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_narrow_only_where_tile_work_outlasts_the_chain(case, monkeypatch):
    """Without the override: config 3 (5 826 K-steps per block row at 2^-52, 3 227 at 2^-28, threshold 1 500) gets the narrow
    table with the count of the issue's table; config 1, config 2 (228) and the 2e4-observation swath case (251) keep 2^-52."""
    lat, _, g = sorted_obs(case)
    monkeypatch.delenv(OVERRIDE, raising=False)
    first, last = factor_envelope(lat, g)
    first52, last52 = envelope(lat, g)
    if case[0] == "config3":
        monkeypatch.setenv(OVERRIDE, str(FACTOR_CUT_BITS))
        forced, forced_last = factor_envelope(lat, g)
        assert np.array_equal(first, forced) and np.array_equal(last, forced_last)
        tiles, ksteps = counts(first)
        print(f"config3: tiles {tiles}, K-steps {ksteps} ({ksteps / first.size:.0f} per block row)")
        assert (tiles, ksteps) == (62021, HEADLINE_KSTEPS)
    else:
        assert np.array_equal(first, first52) and np.array_equal(last, last52)


def test_override_is_checked(monkeypatch):
    lib = _hip.load_library()
    lat = np.array([0.0, 0.5, 1.0])
    env = np.zeros(2, dtype=np.int32)
    for bad in ("53", "0", "abc", "28x"):
        monkeypatch.setenv(OVERRIDE, bad)
        assert lib.oisat_factor_envelope(lat.ctypes.data, 3, C.c_double(1.0), env.ctypes.data) != 0, bad
    monkeypatch.setenv(OVERRIDE, "28")
    assert lib.oisat_factor_envelope(lat.ctypes.data, 3, C.c_double(1.0), env.ctypes.data) == 0
    lat = np.array([0.0, 1.0, 0.5])
    assert lib.oisat_factor_envelope(lat.ctypes.data, 3, C.c_double(1.0), env.ctypes.data) != 0


@pytest.mark.parametrize("name,ny,nx,nobs,seed,L,swaths", [("config2", 360, 720, 10000, 4000, 500.0, False),
                                                          ("swath_10k", 180, 360, 10000, 11, 300.0, True)])
def test_refinement_does_not_see_the_factor_cut_off(monkeypatch, name, ny, nx, nobs, seed, L, swaths):
    """z <- M^-1 d; r = d - S z in float64 with the full S; stop at |r| <= 1e-6 |d| (2-norms), at most two corrections --
    M the fp32 LAPACK Cholesky factor of fp32(S) zeroed outside the table.  At 2^-28 against 2^-52: first residual within
    5 %, the same number of solves, z within 2e-5 of the float64 oracle (the bar of tests/test_gpu_envelope.py).  Measured,
    2^-28 | 2^-52: config 2 2.632e-6 | 2.580e-6 (two solves), swath case 1.114e-6 | 1.089e-6 (two solves); z 7e-9 | 1.2e-8 and
    1.8e-9 | 1.1e-9.  (The swath case's host factorizations run among denormals: most of this test's time.)"""
    import scipy.linalg as sla
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat, lon = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64), np.ravel(p.obs_lon)[o]
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    sb = np.sqrt(p.Sa.ravel())[cell]
    po = orc.unit_vectors(lat, lon)
    S = orc.gaussian_corr(po, po, L)
    S *= sb[:, None]
    S *= sb[None, :]
    S[np.diag_indices_from(S)] += np.ravel(p.obs_var)[o]
    d = np.where(p.obs_y < 0, 0, p.obs_y).ravel()[o] - p.Xa.ravel()[cell]
    zr = sla.cho_solve(sla.cho_factor(S, lower=True), d)
    g = dense.decay_constant(L)
    runs = {}
    for bits in (52, FACTOR_CUT_BITS):
        monkeypatch.setenv(OVERRIDE, str(bits))
        first, _ = factor_envelope(lat, g)
        S32 = S.astype(np.float32)
        for i in range(first.size):
            c = int(first[i]) * NB
            if c:
                S32[i * NB:(i + 1) * NB, :c] = 0
                S32[:c, i * NB:(i + 1) * NB] = 0
        F = sla.cholesky(S32, lower=True, overwrite_a=True, check_finite=False)
        assert F.dtype == np.float32
        F = F.astype(np.float64)
        del S32

        def precondition(r):
            t = sla.solve_triangular(F, r, lower=True, check_finite=False)
            return sla.solve_triangular(F, t, lower=True, trans="T", check_finite=False)

        z, resid = precondition(d), []
        for k in range(3):
            r = d - S @ z
            resid.append(float(np.linalg.norm(r) / np.linalg.norm(d)))
            if resid[-1] <= dense.REFINE_TOL or k == 2:
                break
            z = z + precondition(r)
        ez = float(np.abs(z - zr).max() / np.abs(zr).max())
        print(f"{name} 2^-{bits}: tiles {counts(first)[0]}, residuals {resid}, z {ez:.3e} against the oracle")
        runs[bits] = (resid, ez)
    wide, narrow = runs[52], runs[FACTOR_CUT_BITS]
    assert narrow[0][0] <= 1.05 * wide[0][0]
    assert len(narrow[0]) == len(wide[0]) and narrow[0][-1] <= dense.REFINE_TOL
    assert narrow[1] <= 2e-5 and wide[1] <= 2e-5
