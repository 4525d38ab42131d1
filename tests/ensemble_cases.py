"""What the tests of the posterior ensemble share (tests/test_ensemble_cpu.py, tests/test_gpu_ensemble.py): float64 NumPy /
SciPy restatements of the random-feature sampler, of the member spread and of the whole of Matheron's rule

    delta_k = xi_k - B H^T S^-1 (H xi_k + eps_k),   xi_k ~ N(0, B),  eps_k ~ N(0, R),

with the correlations from ``oisat_corr_eval`` (as ``mc_error_cases.restatement`` takes them) and an exact ``scipy.linalg`` solve
of the float64 S.  The statistical conditions are those of tests/mc_error_cases.py, reused as they stand
(``mc_error_cases.check_conditions``): |x_hat - x| <= 6 se + floor and se <= 1.5 sqrt(2 / K) x_hat.
"""
import numpy as np

from mc_error_cases import check_conditions, mean_var  # noqa: F401  (the two conditions: re-exported for the tests)

SEED = 20250314          # the seed of the statistical tests, CPU restatement and GPU alike
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}

# the statistical case of the GPU tests, restated on the CPU with the same seed (tests/test_ensemble_cpu.py)
STAT_K, STAT_F, STAT_L = 1024, 256, 1000.0


def stat_case():
    from oisatgmi import synthetic as syn
    return syn.point_obs_case(16, 32, 150, 29)


def stat_regions():
    """Three regions of the 16 x 32 grid: a tropical box, a northern band, a southern patch."""
    lab = np.zeros((16, 32), dtype=np.int64)
    lab[6:10, 4:14] = 1
    lab[11:14, :] = 2
    lab[2:5, 18:30] = 3
    return lab


def field_sample64(pxyz, scale, omega, phase, noise=None, nscale=None):
    """include/oisat.h: oisat_field_sample in float64.  ``pxyz`` (3, n); ``omega`` (K, F, 3) and ``phase`` (K, F) as
    ``dense.ensemble_draws`` returns them (turns); ``scale`` (n,) or None; ``noise`` (K, n) with ``nscale`` (n,), or None.
    -> (K, n).  The phase is reduced by its nearest integer before the cosine, like the device's."""
    pxyz = np.asarray(pxyz, dtype=np.float64)
    K, F = phase.shape
    out = np.empty((K, pxyz.shape[1]))
    for k in range(K):
        turns = omega[k] @ pxyz + phase[k][:, None]                     # (F, n)
        out[k] = np.sqrt(2.0 / F) * np.cos(2.0 * np.pi * (turns - np.rint(turns))).sum(axis=0)
    if scale is not None:
        out *= np.asarray(scale, dtype=np.float64)[None, :]
    if noise is not None:
        out += np.sqrt(np.asarray(nscale, dtype=np.float64))[None, :] * np.asarray(noise, dtype=np.float64)
    return out


def corr64(lib, kind, g, pa, pb):
    """C(|pa_i - pb_j|) from ``oisat_corr_eval``: pa (3, na), pb (3, nb) -> (na, nb)."""
    d2 = np.ascontiguousarray(((pa[:, :, None] - pb[:, None, :]) ** 2).sum(axis=0))
    out = np.empty_like(d2)
    assert lib.oisat_corr_eval(kind, g, d2.ctypes.data, d2.size, out.ctypes.data) == 0
    return out


def spread64(G, U, P):
    """include/oisat.h: oisat_member_spread in float64.  ``G`` (n, m) = gsig_i C(i,a) osig_a, ``U`` (K, m), ``P`` (K, n) ->
    the updated P, its sums of squares and of fourth powers over k."""
    out = np.asarray(P, dtype=np.float64) - np.asarray(U, dtype=np.float64) @ G.T
    return out, (out ** 2).sum(axis=0), (out ** 4).sum(axis=0)


class System:
    """The float64 system of a ``synthetic.PointObsCase`` at correlation length ``L_km`` under model ``corr``: the
    observations in ascending latitude (the device's column order), S = H B H^T + R, G = B H^T and the exact analysis error
    variance A_ii = sig_i^2 - g_i^T S^-1 g_i.  ``scale_b`` / ``scale_o`` multiply the variances as ``set_error_scales`` does."""

    def __init__(self, case, L_km, corr, lib, scale_b=1.0, scale_o=1.0):
        from oisatgmi import dense
        self.corr, self.kind, self.L_km = corr, KINDS[corr], float(L_km)
        self.g = dense.decay_constant(L_km)
        cell = dense.regular_grid_cell(case.lat, case.lon, case.obs_lat, case.obs_lon)
        self.order = o = dense.latitude_order(np.asarray(case.obs_lat, dtype=np.float64))
        self.R = np.asarray(case.obs_var, dtype=np.float64)[o] * scale_o
        self.gsig = np.sqrt(scale_b * np.ravel(np.asarray(case.Sa, dtype=np.float64)))
        self.osig = self.gsig[cell[o]]
        self.pg = dense.unit_vectors(np.ravel(case.lat), np.ravel(case.lon))
        self.po = dense.unit_vectors(np.asarray(case.obs_lat)[o], np.asarray(case.obs_lon)[o])
        self.n, self.m = self.gsig.size, self.R.size
        self.S = corr64(lib, self.kind, self.g, self.po, self.po) * self.osig[:, None] * self.osig[None, :] + np.diag(self.R)
        self.G = corr64(lib, self.kind, self.g, self.pg, self.po) * self.gsig[:, None] * self.osig[None, :]
        self._A = None

    @property
    def A(self):
        if self._A is None:
            import scipy.linalg as sla
            cf = sla.cho_factor(self.S, lower=True)
            self._A = self.gsig ** 2 - np.einsum("ia,ai->i", self.G, sla.cho_solve(cf, self.G.T))
        return self._A

    def draws(self, members, F, seed, noise32=True):
        """``dense.ensemble_draws`` for this system, at the length ``posterior_ensemble`` derives from the plan's decay
        constant; ``noise32``: the noise narrowed to float32 and widened again, as the device receives it."""
        from oisatgmi import dense
        omega, phase, eps = dense.ensemble_draws(self.corr, dense.corr_length_of(self.g), members, F, self.m, seed)
        return omega, phase, eps.astype(np.float32).astype(np.float64) if noise32 else eps

    def deviations(self, members, F, seed):
        """Matheron's rule in float64 with the device's draws -> delta (K, n)."""
        import scipy.linalg as sla
        omega, phase, eps = self.draws(members, F, seed)
        xi_g = field_sample64(self.pg, self.gsig, omega, phase)
        r = field_sample64(self.po, self.osig, omega, phase, eps, self.R)             # H xi + eps, rows
        X = sla.cho_solve(sla.cho_factor(self.S, lower=True), r.T).T                # rows (S^-1 r_k)^T
        return spread64(self.G, X, xi_g)[0]

    def ensemble_variance(self, K, F, seed, chunk=512):
        """(A_hat, var of A_hat) over members 0 .. K-1: the mean is known to be zero, K degrees of freedom."""
        s2, s4 = np.zeros(self.n), np.zeros(self.n)
        for k0 in range(0, K, chunk):
            d2 = self.deviations(range(k0, min(K, k0 + chunk)), F, seed) ** 2
            s2 += d2.sum(axis=0)
            s4 += (d2 * d2).sum(axis=0)
        return mean_var(s2, s4, K)


def beyond_three(est, se, exact):
    """Share of the entries that lie beyond three of their own standard errors."""
    est, se, exact = (np.ravel(np.asarray(v, dtype=np.float64)) for v in (est, se, exact))
    return float(np.mean(np.abs(est - exact) > 3.0 * se))
