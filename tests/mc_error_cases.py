"""What the tests of the randomized analysis error share (tests/test_mc_error_cpu.py, tests/test_gpu_mc_error.py): the probe
sign restated in NumPy, a float64 restatement of the whole estimator, and the two statistical conditions both are held to.

The conditions, for an estimate x_hat of x with reported standard error se:
  (a) |x_hat - x| <= 6 se + floor      (b) se <= 1.5 sqrt(2 / K) x_hat        (entries with x_hat = 0 exempt from (b))
``floor`` is not statistical slack.  Some entries have NO sampling noise at all -- the last observation of the latitude
order has u_a = w_a / L_aa, so u_a^2 is the same number in every probe and se = 0 exactly -- and there the two sides differ
by the rounding of the arithmetic that produced them, nothing else.  The floor is that rounding, stated by the caller for
the number formats involved; it is 3 to 4 orders of magnitude below 6 se wherever there is sampling noise to speak of.
"""
import ctypes as C

import numpy as np

SEED = 20240611          # the seed of the end-to-end tests, CPU restatement and GPU alike
K_E2E = 1024

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(x):
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def np_probe_sign(seed, probe, column):
    """include/oisat.h: oisat_probe_sign, vectorised (broadcasts probe against column); float32 +-1."""
    s = _mix(np.array(int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    h = _mix(_mix(s ^ np.asarray(probe, dtype=np.uint64)) ^ np.asarray(column, dtype=np.uint64))
    return np.where(h >> np.uint64(63), -1.0, 1.0).astype(np.float32)


def c_probe_sign(lib, seed, probe, column):
    out = C.c_float(0)
    assert lib.oisat_probe_sign(int(seed), int(probe), int(column), C.byref(out)) == 0
    return out.value


def mean_var(sum2, sum4, K):
    mean = sum2 / K
    return mean, np.maximum(sum4 / K - mean * mean, 0.0) / (K - 1)


def restatement(case, L_km, K, seed, lib, kind=0):
    """The estimator in float64 NumPy / SciPy on a ``synthetic.PointObsCase``: observations in ascending latitude (the device's
    column order, so probe k meets the same observation here and there), signs from the sign function, u = L^-T w by a
    triangular solve.  Returns the exact q_i = g_i^T S^-1 g_i and s_a = (S^-1)_aa beside their estimates and variances."""
    import scipy.linalg as sla
    from oisatgmi import dense
    lat, lon = np.ravel(case.lat), np.ravel(case.lon)
    cell = dense.regular_grid_cell(case.lat, case.lon, case.obs_lat, case.obs_lon)
    o = dense.latitude_order(np.asarray(case.obs_lat, dtype=np.float64))
    olat, olon, cell, R = case.obs_lat[o], case.obs_lon[o], cell[o], np.asarray(case.obs_var, dtype=np.float64)[o]
    sig = np.sqrt(np.ravel(np.asarray(case.Sa, dtype=np.float64)))
    osig = sig[cell]
    pg, po = dense.unit_vectors(lat, lon), dense.unit_vectors(olat, olon)
    g = dense.decay_constant(L_km)

    def corr(pa, pb):
        d2 = np.ascontiguousarray(((pa[:, :, None] - pb[:, None, :]) ** 2).sum(axis=0))
        out = np.empty_like(d2)
        assert lib.oisat_corr_eval(kind, g, d2.ctypes.data, d2.size, out.ctypes.data) == 0
        return out

    S = corr(po, po) * osig[:, None] * osig[None, :] + np.diag(R)
    G = corr(pg, po) * sig[:, None] * osig[None, :]                     # rows g_i of B H^T
    Lf = np.linalg.cholesky(S)
    m = R.size
    W = np_probe_sign(seed, np.arange(K)[:, None], np.arange(m)[None, :]).astype(np.float64)
    U = sla.solve_triangular(Lf, W.T, lower=True, trans="T").T          # rows u_k = (L^-T w_k)^T
    T = G @ U.T                                                         # t_ik
    q_hat, q_var = mean_var((T ** 2).sum(axis=1), (T ** 4).sum(axis=1), K)
    s_hat, s_var = mean_var((U ** 2).sum(axis=0), (U ** 4).sum(axis=0), K)
    Sinv = np.linalg.inv(S)
    return {"q": np.einsum("ia,ab,ib->i", G, Sinv, G), "s": np.diag(Sinv).copy(), "q_hat": q_hat, "q_var": q_var,
            "s_hat": s_hat, "s_var": s_var, "sig2": sig ** 2, "R": R, "order": o, "U": U}


def check_conditions(est, se, exact, K, floor, what):
    """Conditions (a) and (b) of the module docstring on every entry; prints the worst figures before it asserts."""
    est, se, exact = (np.ravel(np.asarray(v, dtype=np.float64)) for v in (est, se, exact))
    floor = np.broadcast_to(np.ravel(np.asarray(floor, dtype=np.float64)), est.shape)
    dev = np.abs(est - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0, (dev - floor) / se, np.where(dev <= floor, 0.0, np.inf))
        rel = np.where(est > 0, se / est, 0.0)
    print(f"{what}: worst (|est - exact| - floor) / se = {z.max():.2f} (bound 6), worst se / est = {rel.max():.4f} "
          f"(bound {1.5 * np.sqrt(2.0 / K):.4f}), entries {est.size}")
    assert np.all(dev <= 6.0 * se + floor), f"{what}: condition (a) fails at {np.flatnonzero(dev > 6.0 * se + floor)[:8]}"
    assert np.all(rel <= 1.5 * np.sqrt(2.0 / K)), f"{what}: condition (b) fails at {np.flatnonzero(rel > 1.5 * np.sqrt(2.0 / K))[:8]}"
