"""Float64 references for the drift of the innovations (universal kriging), NumPy only.

A case is m scattered observations over a global 24 x 48 grid (both poles are rows of it) at L = 1500 km: unit vectors, sigma_b,
observation variances, and the dense S = sig sig^T .* C + diag(var) from the coordinates by the formulas of
tests/readers_cases.py (``corr_ref``: the ones tests/test_corr_cpu.py holds against include/oisat.h).  Sizes: m = 333 (no multiple
of 64 or 128) and m = 700 (six 128-row blocks); ``cap=True`` draws the observations inside a 20-degree cap, where a degree-3 drift
is not identifiable.  Innovations with a known truth: d = F beta_true + chol(S) eps, eps from Philox(seed).

``basis`` restates ``oisat_drift_basis`` operation for operation (NumPy rounds once per operation, as the kernel does), ``gls`` is
the textbook estimate through a float64 Cholesky of S, ``analysis``, ``drift_variance`` and the restricted likelihood follow
from it.  Observations are kept in ascending latitude, the order the plans store them in."""
import functools

import numpy as np

import readers_cases as rc
from oisatgmi import dense

GRID = (24, 48)
L_KM = 1500.0
MODELS = ("gaussian", "gaspari_cohn", "soar")
DEGREES = (0, 1, 3)
SIZES = (333, 700)
TOL = 1e-6                                                      # the solves' relative tolerance (dense.REFINE_TOL)
LN2PI = float(np.log(2.0 * np.pi))
CAP_DEG, CAP_CENTRE = 20.0, (35.0, 20.0)                        # the concentrated case: angular radius, (lat, lon) of the centre
BETA_TRUE = np.array([1.5, -1.0, 0.8, 1.2, 0.6, -0.7, 0.5, 0.4, -0.3, 0.5, -0.4, 0.3, 0.6, -0.5, 0.2, -0.3])


def basis(xyz, degree):
    """(p, npts) float64: the real harmonics up to ``degree`` at unit vectors ``xyz`` (3, npts), p = (degree + 1)^2, in the order
    and by the expressions of include/oisat.h (``oisat_drift_basis``), one rounding per operation."""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in xyz)
    f = [np.ones_like(x)]
    if degree >= 1:
        f += [x, y, z]
    if degree >= 2:
        xx, yy, zz, xy = x * x, y * y, z * z, x * y
        f += [xy, y * z, z * x, xx - yy, 3.0 * zz - 1.0]
    if degree >= 3:
        t = 5.0 * zz
        f += [z * (t - 3.0), x * (t - 1.0), y * (t - 1.0), z * (xx - yy), xy * z, x * (xx - 3.0 * yy), y * (3.0 * xx - yy)]
    return np.array(f)


class Grid:
    def __init__(self):
        ny, nx = GRID
        lat1 = np.linspace(-90.0, 90.0, ny)                     # the poles are rows
        lon1 = -180.0 + 360.0 * np.arange(nx) / nx
        self.lat, self.lon = np.meshgrid(lat1, lon1, indexing="ij")
        self.n = ny * nx
        self.gxyz = dense.unit_vectors(self.lat, self.lon)     # (3, n)
        la, lo = np.radians(self.lat), np.radians(self.lon)
        self.Xa = 10.0 + 2.0 * np.sin(2.0 * la) * np.cos(lo) + np.cos(la) * np.sin(2.0 * lo)
        self.Sa = (0.1 * self.Xa) ** 2
        self.gsig = np.sqrt(self.Sa.ravel())


@functools.lru_cache(maxsize=None)
def grid():
    return Grid()


class Case:
    """m observations in ascending latitude; ``L_km`` may leave the default (tests/test_gpu_drift.py takes L = 300 km for the
    residual's windowed and culled paths) and ``var_scale`` multiplies the observation variances.  (The ill-conditioned system
    of DESIGN.md section 5 is ``IllCase``, not one of these.)"""

    def __init__(self, m, cap=False, L_km=L_KM, var_scale=1.0, seed=7100):
        rng = np.random.Generator(np.random.Philox(seed + m + (1 if cap else 0)))
        if cap:                                                 # uniform in the cap around CAP_CENTRE
            cosr = 1.0 - rng.uniform(size=m) * (1.0 - np.cos(np.radians(CAP_DEG)))
            az = rng.uniform(0.0, 2.0 * np.pi, size=m)
            sinr = np.sqrt(1.0 - cosr * cosr)
            la0, lo0 = np.radians(CAP_CENTRE)
            c = np.array([np.cos(la0) * np.cos(lo0), np.cos(la0) * np.sin(lo0), np.sin(la0)])
            e = np.array([-np.sin(lo0), np.cos(lo0), 0.0])
            nrt = np.cross(c, e)
            v = cosr * c[:, None] + sinr * (np.cos(az) * e[:, None] + np.sin(az) * nrt[:, None])
        else:                                                   # uniform on the sphere
            v = rng.standard_normal((3, m))
            v /= np.linalg.norm(v, axis=0)
        lat = np.degrees(np.arcsin(np.clip(v[2], -1.0, 1.0)))
        lon = np.degrees(np.arctan2(v[1], v[0]))
        o = np.argsort(lat, kind="stable")
        self.m, self.cap, self.L_km = m, cap, L_km
        self.lat, self.lon = np.ascontiguousarray(lat[o]), np.ascontiguousarray(lon[o])
        self.oxyz = dense.unit_vectors(self.lat, self.lon)     # (3, m)
        self.osig = 0.8 + 0.4 * rng.uniform(size=m)
        self.ovar = (0.3 + 0.3 * rng.uniform(size=m)) ** 2 * var_scale
        self.eps = rng.standard_normal(m)
        self.g = dense.decay_constant(L_km)
        self.mp = -(-m // rc.NB) * rc.NB


@functools.lru_cache(maxsize=None)
def case(m, cap=False, L_km=L_KM, var_scale=1.0):
    return Case(m, cap, L_km, var_scale)


class IllCase:
    """The ill-conditioned system of DESIGN.md section 5 at m = 333: the observations of ``syn.point_obs_case(72, 144, m, 9403)``
    (tests/test_gpu_round4.py), sigma_b from its ``Sa`` at the cell, its observation variances x 0.03, L = 3 000 km; ascending
    latitude, the attributes of ``Case``."""

    def __init__(self, m=333, L_km=3000.0, var_scale=0.03):
        from oisatgmi import synthetic as syn
        p = syn.point_obs_case(72, 144, m, 9403)
        o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
        self.m, self.cap, self.L_km = m, False, L_km
        self.lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
        self.lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
        self.oxyz = dense.unit_vectors(self.lat, self.lon)
        self.osig = np.sqrt(p.Sa.ravel().astype(np.float64))[dense.regular_grid_cell(p.lat, p.lon, self.lat, self.lon)]
        self.ovar = np.ascontiguousarray(np.ravel(p.obs_var)[o], dtype=np.float64) * var_scale
        self.g = dense.decay_constant(L_km)
        self.mp = -(-m // rc.NB) * rc.NB


@functools.lru_cache(maxsize=None)
def ill_case():
    return IllCase()


@functools.lru_cache(maxsize=None)
def system64(m, model="gaussian", cap=False, L_km=L_KM, var_scale=1.0):
    """S = sig sig^T .* C + diag(var), float64, m x m, read-only."""
    S = rc.system64(case(m, cap, L_km, var_scale), model)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def chol64(m, model="gaussian", cap=False):
    Lc = np.linalg.cholesky(system64(m, model, cap))
    Lc.setflags(write=False)
    return Lc


def innovations(m, model, degree, cap=False):
    """d = F beta_true + chol(S) eps, and beta_true ((degree + 1)^2,)."""
    c = case(m, cap)
    bt = BETA_TRUE[:(degree + 1) ** 2].copy()
    return basis(c.oxyz, degree).T @ bt + chol64(m, model, cap) @ c.eps, bt


def solve64(m, model, rhs, cap=False):
    """S^-1 rhs through the float64 Cholesky factor (rhs (m,) or (m, k))."""
    import scipy.linalg as sla
    Lc = chol64(m, model, cap)
    return sla.solve_triangular(Lc, sla.solve_triangular(Lc, rhs, lower=True), lower=True, trans="T")


def scaled_cond(M):
    """2-norm condition number of M scaled to unit diagonal (what ``dense.drift_coefficients`` tests against 1 / tol)."""
    s = 1.0 / np.sqrt(np.diag(M))
    ev = np.linalg.eigvalsh(0.5 * (M + M.T) * s[:, None] * s[None, :])
    return float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")


def gls(m, model, degree, d, cap=False, F=None):
    """The generalised-least-squares drift and the kriging weights, float64: beta = M^-1 F^T S^-1 d, M = F^T S^-1 F,
    z' = S^-1 (d - F beta).  ``F`` (m, p) defaults to the basis at the case's observations."""
    c = case(m, cap)
    F = basis(c.oxyz, degree).T if F is None else F
    Y, zd = solve64(m, model, F, cap), solve64(m, model, d, cap)
    M = F.T @ Y
    M = 0.5 * (M + M.T)
    cov = np.linalg.inv(M)
    beta = np.linalg.solve(M, F.T @ zd)
    zp = zd - Y @ beta
    sign, logdet_M = np.linalg.slogdet(M)
    logdet_S = 2.0 * float(np.log(np.diag(chol64(m, model, cap))).sum())
    chi2 = float((d - F @ beta) @ zp)
    p = F.shape[1]
    return {"beta": beta, "beta_cov": cov, "beta_se": np.sqrt(np.diag(cov)), "cond": scaled_cond(M), "M": M, "Y": Y, "z_d": zd, "z": zp,
            "chi2": chi2, "logdet_M": float(logdet_M), "logdet": logdet_S, "p": p,
            "neg2_restricted_log_likelihood": (m - p) * LN2PI + logdet_S + float(logdet_M) + chi2}


def cross64(m, model, cap=False):
    """B H^T, (n, m) float64: gsig_i C(i, a) osig_a."""
    c, gr = case(m, cap), grid()
    return rc.corr_ref(gr.gxyz, c.oxyz, c.L_km, model) * gr.gsig[:, None] * c.osig[None, :]


def analysis(m, model, degree, ref, cap=False):
    """The increment of the analysis with drift, (n,): B H^T z' + f(x)^T beta."""
    return cross64(m, model, cap) @ ref["z"] + basis(grid().gxyz, degree).T @ ref["beta"]


def drift_variance(m, model, degree, ref, cap=False):
    """q_i^T M^-1 q_i, q_i = f(x_i) - (B H^T Y_F)_i, (n,)."""
    q = basis(grid().gxyz, degree).T - cross64(m, model, cap) @ ref["Y"]
    return np.einsum("ij,jk,ik->i", q, ref["beta_cov"], q)
