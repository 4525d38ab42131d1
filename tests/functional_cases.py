"""What the tests of the regional analysis error share (tests/test_functional_cpu.py, tests/test_gpu_functional.py): the three
cases, their six functionals and the dense float64 reference

    A_W = W B W^T - G^T S^-1 G,    G = H B W^T,    S = H B H^T + R

in NumPy, with every correlation from the library's host-only ``oisat_corr_eval`` (so any of the three models can be asked for),
B and H B from the cell centres and the observation coordinates, ``np.linalg.solve`` for the solves.  Each reference is computed
once per (case, model) and shared; nobody writes to it.

The bound of the end-to-end test is derived, not tuned: the residual-corrected reduction G^T Y + R^T Y differs from
G^T S^-1 G by R^T S^-1 R, at most |r_k| |r_l| / lambda_min(S) <= tol^2 |g_k| |g_l| / lambda_min(S), and |g_k|^2 / lambda_max(S) <=
g_k^T S^-1 g_k <= prior_kk: tol^2 cond(S) sqrt(prior_kk prior_ll).  The factor 2 and the 1e-11 cover the float64 rounding of the pair
sums and of the K x K products (a few thousand terms of 1e-16 each).
"""
import functools

import numpy as np

from oisatgmi import _hip, dense, synthetic as syn

KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}
TOL = 1e-6                     # the end-to-end tests' refinement tolerance
REFINE = 4
# (ny, nx, observations, L in km, seed) and cond(S) in float64 on the CPU, rounded: test_functional_cpu.py holds each below 1e3
CASES = {"a": (24, 48, 300, 500.0, 4700), "b": (24, 48, 300, 1000.0, 4701), "c": (36, 72, 700, 300.0, 4702)}
COND = {"a": 148, "b": 537, "c": 521}
NAMES = ("global", "band", "box", "onehot", "far", "zero")
I_GLOBAL, I_BAND, I_BOX, I_ONEHOT, I_FAR, I_ZERO = range(6)


def library():
    """The library, built first where a clean checkout has none yet (dlopen only: no device call)."""
    import os
    if not os.path.exists(_hip.library_path()):
        import __graft_entry__ as g
        g.build()
    return _hip.load_library()


def corr_eval(kind, g, d2):
    """C(chord^2) in float64 by the library's host-only function."""
    lib = library()
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    out = np.empty_like(d2)
    assert lib.oisat_corr_eval(int(kind), float(g), d2.ctypes.data, d2.size, out.ctypes.data) == 0
    return out


def chord2(pa, pb):
    """|p - q|^2 of every pair from (3, na) and (3, nb) unit vectors, by coordinate differences as the kernels form it."""
    return ((pa[:, :, None] - pb[:, None, :]) ** 2).sum(axis=0)


@functools.lru_cache(maxsize=None)
def case(name):
    ny, nx, nobs, L, seed = CASES[name]
    return syn.point_obs_case(ny, nx, nobs, seed)


@functools.lru_cache(maxsize=None)
def functionals(name):
    """(6, ny, nx) float64 and the cell of the one-hot functional: the global area mean, the band 20-50 N, a box inside it (so
    the two overlap), one cell that carries an observation, a region far from the box (lat < -30, lon > 100) and a zero row."""
    p = case(name)
    lat, lon = p.lat, p.lon
    w = np.cos(np.deg2rad(lat))
    cell = dense.regular_grid_cell(lat, lon, p.obs_lat, p.obs_lon)
    inbox = (p.obs_lat > 25.0) & (p.obs_lat < 45.0) & (p.obs_lon > 0.0) & (p.obs_lon < 60.0)
    hot = int(cell[np.flatnonzero(inbox)[0]])                        # an observed cell, inside the box
    masks = [np.ones(lat.shape, dtype=bool), (lat > 20.0) & (lat < 50.0),
             (lat > 25.0) & (lat < 45.0) & (lon > 0.0) & (lon < 60.0), None, (lat < -30.0) & (lon > 100.0), None]
    W = np.zeros((6,) + lat.shape)
    for k, mk in enumerate(masks):
        if mk is not None:
            assert mk.any()
            W[k] = np.where(mk, w, 0.0) / w[mk].sum()
    W[I_ONEHOT].flat[hot] = 1.0
    W.setflags(write=False)
    return W, hot


@functools.lru_cache(maxsize=None)
def reference(name, corr="gaussian"):
    """The dense float64 reference of case ``name`` under model ``corr``: a dict with ``prior``, ``reduction``, ``posterior``
    (6 x 6), ``cond`` = cond(S), and the pieces ``S``, ``G`` (m x 6, H B W^T, observations in the CALLER's order), ``T`` (n x 6,
    B W^T), ``sig`` (n,), ``osig``, ``R`` (m,), ``po`` / ``pg`` (unit vectors), ``cell``."""
    p = case(name)
    L = CASES[name][3]
    W, _ = functionals(name)
    Wf = W.reshape(6, -1)
    g, kind = dense.decay_constant(L), KINDS[corr]
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    sig = np.sqrt(np.ravel(np.asarray(p.Sa, dtype=np.float64)))
    osig, R = sig[cell], np.asarray(p.obs_var, dtype=np.float64)
    pg, po = dense.unit_vectors(np.ravel(p.lat), np.ravel(p.lon)), dense.unit_vectors(p.obs_lat, p.obs_lon)
    B = corr_eval(kind, g, chord2(pg, pg)) * sig[:, None] * sig[None, :]
    HB = corr_eval(kind, g, chord2(po, pg)) * osig[:, None] * sig[None, :]
    S = corr_eval(kind, g, chord2(po, po)) * osig[:, None] * osig[None, :] + np.diag(R)
    T = B @ Wf.T
    G = HB @ Wf.T
    prior = Wf @ T
    red = G.T @ np.linalg.solve(S, G)
    prior, red = 0.5 * (prior + prior.T), 0.5 * (red + red.T)
    out = {"prior": prior, "reduction": red, "posterior": prior - red, "cond": float(np.linalg.cond(S)), "S": S, "G": G, "T": T,
           "sig": sig, "osig": osig, "R": R, "po": po, "pg": pg, "cell": cell, "g": g, "kind": kind}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def bound(ref, tol=TOL):
    """(2 tol^2 cond(S) + 1e-11) sqrt(prior_kk prior_ll), (6, 6): the end-to-end bound of the module docstring."""
    d = np.sqrt(np.maximum(np.diag(ref["prior"]), 0.0))
    return (2.0 * tol * tol * ref["cond"] + 1e-11) * d[:, None] * d[None, :]
