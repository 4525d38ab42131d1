"""Float64 references for the innovations' likelihood and the maximum-likelihood error scales, NumPy only.

The systems are those of tests/readers_cases.py (A, B, C, B600): P = sig sig^T .* C at the case's own sigma_b, R = diag(var),
S(scale_b, scale_o) = scale_b P + scale_o R.  Innovations for the recovery tests are drawn as d = chol(S_true) w with
w = default_rng(seed).standard_normal(m), seeds 2 and 3.

``Profile`` evaluates -2 ln p(d) along s -> s P + R through ONE symmetric eigen-decomposition R^-1/2 P R^-1/2 = V diag(lam) V^T:
log det = sum log(s lam + 1) + sum log R and chi^2 = sum (V^T R^-1/2 d)^2 / (s lam + 1), so that a 2001-point grid costs
nothing; tests/test_likelihood_cpu.py holds it against ``loglik64`` (slogdet and a solve of S itself)."""
import functools

import numpy as np

import readers_cases as rc

SEEDS = (2, 3)
BOUNDS = (1e-2, 1e2)
LN2PI = float(np.log(2.0 * np.pi))


@functools.lru_cache(maxsize=None)
def prior64(name, model="gaussian"):
    """P = H D^1/2 C D^1/2 H^T of the case, float64, m x m (no R)."""
    c = rc.case(name)
    P = rc.corr_ref(c.oxyz, c.oxyz, c.L_km, model) * c.osig[:, None] * c.osig[None, :]
    P.setflags(write=False)
    return P


def system64(name, model="gaussian", scale_b=1.0, scale_o=1.0):
    S = scale_b * prior64(name, model)
    S[np.diag_indices_from(S)] += scale_o * rc.case(name).ovar
    return S


@functools.lru_cache(maxsize=None)
def draw(name, model="gaussian", scale_b=1.0, scale_o=1.0, seed=2):
    """d = chol(S_true) w, float64 (m,), in the case's (ascending-latitude) order."""
    w = np.random.default_rng(seed).standard_normal(rc.case(name).m)
    d = np.linalg.cholesky(system64(name, model, scale_b, scale_o)) @ w
    d.setflags(write=False)
    return d


def loglik64(name, model, d, scale_b=1.0, scale_o=1.0):
    """The reference of ``DenseAnalysis.log_likelihood``: slogdet and a solve of the float64 S."""
    S = system64(name, model, scale_b, scale_o)
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    chi2 = float(d @ np.linalg.solve(S, d))
    m = d.size
    return {"m": m, "chi2": chi2, "chi2_per_obs": chi2 / m, "logdet": float(logdet), "neg2_log_likelihood": m * LN2PI + float(logdet) + chi2,
            "dd": float(d @ d)}


class Profile:
    """J_b(x) = log det(s P + R) + d^T (s P + R)^-1 d and J_r(x) = m ln(chi2 / m) + log det + m at s = exp(x)."""

    def __init__(self, name, model, d):
        c = rc.case(name)
        r = 1.0 / np.sqrt(c.ovar)
        lam, V = np.linalg.eigh(prior64(name, model) * r[:, None] * r[None, :])
        self.lam, self.q2, self.logR, self.m = lam, (V.T @ (r * d)) ** 2, float(np.log(c.ovar).sum()), c.m

    def parts(self, x):
        """(log det, chi2) at ln s = x; x may be an array."""
        den = np.exp(np.asarray(x, dtype=np.float64))[..., None] * self.lam + 1.0
        return np.log(den).sum(axis=-1) + self.logR, (self.q2 / den).sum(axis=-1)

    def J_background(self, x):
        logdet, chi2 = self.parts(x)
        return logdet + chi2

    def J_both(self, x):
        logdet, chi2 = self.parts(x)
        return self.m * np.log(chi2 / self.m) + logdet + self.m

    def J(self, mode):
        return self.J_both if mode == "both" else self.J_background


def fine_grid(npts=2001):
    return np.linspace(np.log(BOUNDS[0]), np.log(BOUNDS[1]), npts)
