"""Host-side cases, float64 references and float32 yardsticks for the readers of the Cholesky factor that do not refine:
``oisat_trsm_rows``, ``oisat_posterior_error``, ``oisat_gain_diag`` and ``oisat_potrs`` (NumPy / SciPy only, no device).

Every reference takes a lower-triangular factor ``Lh``: the float64 copy of an fp32 factor, identity padding included.  On the
GPU that is the factor downloaded from the device, so the factorization's own error is out of the picture and what is measured
is the reader.  Every bar is a multiple of ``e32``: the max-norm distance, relative to the reference's largest entry, between
that reference and the SAME operation evaluated plainly in float32 on the CPU (coordinates cast to float32, squared chord and
correlation in float32, SciPy's float32 triangular solve, squares summed in float64).

``blocked_sweep_f32`` restates the library's scheme (diagonal blocks inverted in float64 and rounded to float32, block forward
substitution with float32 products); tests/test_readers_cases_cpu.py holds it to 2 x e32 and shows that leaving out any one
block of the factor puts it beyond 4 x e32, the bar of tests/test_gpu_readers_abi.py."""
import functools

import numpy as np
import scipy.linalg as sla

from oisatgmi import dense, synthetic as syn

NB = 128
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}
GRID = (36, 72)                                                 # the cells of the posterior-error cases: n = 2592
#        m, L (km), seed of syn.point_obs_case(72, 144, m, seed)
# (A's seed: block row 3 has ONE live row, the northernmost observation, and its block (3, 0) reaches 1e-3 of the factor's
# norm in one seed of 1500 -- best of the others: 0.97e-3.  The CPU test asserts the property, not the seed.)
CASES = {"A": (385, 3000.0, 341),                               # 4 block rows, padded last block; every block of L is large
         "B": (700, 100.0, 4700),                               # 6 block rows, a real envelope
         "C": (100, 300.0, 4100),                               # one block: the factor under three block rows
         # B's observations at L = 600 km.  B itself has first[i] = i - 1: its tiles have no K-loop at all and so no far or
         # middle stretch to force; here 8 far and 6 middle K-blocks of 14 at 2^-16 / 2^-8 (asserted where it is used).
         "B600": (700, 600.0, 4700)}
# (i0, i1, chunk_rows) of oisat_posterior_error on the n = 2592 cells
N_CELLS = GRID[0] * GRID[1]
ERR_RANGES = [(0, N_CELLS, 0), (0, N_CELLS, 128), (5, 133, 128), (1000, 1300, 100), (N_CELLS - 1, N_CELLS, 4096), (0, 1, 1)]


class Case:
    """Observations in ascending latitude, ``osig`` from ``Sa`` at the cell, ``ovar`` = the case's ``obs_var``."""

    def __init__(self, name):
        self.name = name
        self.m, self.L_km, seed = CASES[name]
        p = syn.point_obs_case(72, 144, self.m, seed)
        o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
        self.lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
        self.lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
        cell = dense.regular_grid_cell(p.lat, p.lon, self.lat, self.lon)
        self.oxyz = dense.unit_vectors(self.lat, self.lon)     # (3, m)
        self.osig = np.sqrt(p.Sa.ravel().astype(np.float64))[cell]
        self.ovar = np.ascontiguousarray(np.ravel(p.obs_var)[o], dtype=np.float64)
        self.g = dense.decay_constant(self.L_km)
        self.mp = -(-self.m // NB) * NB
        self.nb = self.mp // NB


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


class Grid:
    def __init__(self):
        p = syn.point_obs_case(GRID[0], GRID[1], 8, 36)
        self.n = p.lat.size
        self.gxyz = dense.unit_vectors(p.lat, p.lon)           # (3, n)
        self.gsig = np.sqrt(p.Sa.ravel().astype(np.float64))


@functools.lru_cache(maxsize=None)
def grid():
    return Grid()


# ---- the three correlation functions in float64, as printed in include/oisat.h (tests/test_gpu_corr.py and test_gpu_soar.py import
# them from here) ------------------------------------------------------------------------------------------------------------
def gc_ref(z):
    """Gaspari-Cohn (1999), eq. 4.10, in z = distance / c, float64, the formula as printed."""
    z = np.asarray(z, dtype=np.float64)
    near = -z ** 5 / 4 + z ** 4 / 2 + 5 * z ** 3 / 8 - 5 * z ** 2 / 3 + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        far = z ** 5 / 12 - z ** 4 / 2 + 5 * z ** 3 / 8 + 5 * z ** 2 / 3 - 5 * z + 4 - 2 / (3 * z)
    return np.where(z <= 1, near, np.where(z < 2, np.maximum(far, 0.0), 0.0))


def chord2(pa, pb):
    """|p - q|^2 from coordinate differences, pa (3, na), pb (3, nb) -> (na, nb)."""
    out = np.zeros((pa.shape[1], pb.shape[1]))
    for k in range(3):
        out += (pa[k][:, None] - pb[k][None, :]) ** 2
    return out


def corr_ref(pa, pb, L, model):
    """C between unit vectors pa (3, na) and pb (3, nb) at correlation length L (km): "soar", "gaspari_cohn" or "gaussian"."""
    g = dense.decay_constant(L)
    d2 = chord2(pa, pb)
    if model == "soar":
        s = np.sqrt(2.0 * g * d2)                               # = chord R_earth / L
        return (1.0 + s) * np.exp(-s)
    return gc_ref(np.sqrt(0.6 * g * d2)) if model == "gaspari_cohn" else np.exp(-g * d2)


# ---- the correlation in float32, plainly --------------------------------------------------------------------------------
def corr_f32(pa, pb, g, model):
    """The formulas of include/oisat.h evaluated in float32 throughout: coordinates cast to float32, the squared chord from
    their differences, the function of it."""
    f = np.float32
    a, b = pa.astype(f), pb.astype(f)
    d2 = np.zeros((a.shape[1], b.shape[1]), dtype=f)
    for k in range(3):
        d = a[k][:, None] - b[k][None, :]
        d2 += d * d
    if model == "gaussian":
        return np.exp(-f(g) * d2)
    if model == "soar":
        s = np.sqrt(f(2.0 * g) * d2)
        return (f(1) + s) * np.exp(-s)
    z = np.sqrt(f(0.6 * g) * d2)
    z2, z3 = z * z, z * z * z
    near = -z3 * z2 / f(4) + z2 * z2 / f(2) + f(5) * z3 / f(8) - f(5) * z2 / f(3) + f(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        far = z3 * z2 / f(12) - z2 * z2 / f(2) + f(5) * z3 / f(8) + f(5) * z2 / f(3) - f(5) * z + f(4) - f(2) / (f(3) * z)
    out = np.where(z <= 1, near, np.where(z < 2, np.maximum(far, f(0)), f(0))).astype(f)
    assert out.dtype == f
    return out


# ---- the system and stand-ins for the device's factor ------------------------------------------------------------------
def system64(c, model="gaussian"):
    """S = sig sig^T .* C + diag(var), float64, m x m."""
    S = corr_ref(c.oxyz, c.oxyz, c.L_km, model) * c.osig[:, None] * c.osig[None, :]
    S[np.diag_indices_from(S)] += c.ovar
    return S


def pad_factor(L, mp):
    """The m x m factor inside the identity padding of the library's mp x mp one."""
    out = np.eye(mp, dtype=L.dtype)
    out[:L.shape[0], :L.shape[0]] = L
    return out


def exact_factor64(c, model="gaussian"):
    return pad_factor(np.linalg.cholesky(system64(c, model)), c.mp)


def fp32_factor(c, model="gaussian"):
    """A host stand-in for the factor the device leaves: the float64 Cholesky factor rounded to float32 (the CPU tests need AN
    fp32 factor of the case, not the device's bits)."""
    return exact_factor64(c, model).astype(np.float32)


# ---- rows ---------------------------------------------------------------------------------------------------------------
def cross_rows64(c, gr, i0, i1, model="gaussian"):
    """g_i, i0 <= i < i1: rows of B H^T in float64, zero in the padding columns."""
    G = np.zeros((i1 - i0, c.mp))
    G[:, :c.m] = corr_ref(gr.gxyz[:, i0:i1], c.oxyz, c.L_km, model) * gr.gsig[i0:i1, None] * c.osig[None, :]
    return G


def cross_rows32(c, gr, i0, i1, model="gaussian"):
    G = np.zeros((i1 - i0, c.mp), dtype=np.float32)
    G[:, :c.m] = gr.gsig[i0:i1].astype(np.float32)[:, None] * c.osig.astype(np.float32)[None, :] * \
        corr_f32(gr.gxyz[:, i0:i1], c.oxyz, c.g, model)
    return G


def identity_rows(c, a0=0, a1=None, dtype=np.float64):
    a1 = c.m if a1 is None else a1
    E = np.zeros((a1 - a0, c.mp), dtype=dtype)
    E[np.arange(a1 - a0), np.arange(a0, a1)] = 1
    return E


def probe_rows(c, nrows, seed=5):
    """+-1 rows, exact zeros in the padding columns (on the GPU ``oisat_probe_fill`` makes them; any +-1 pattern serves the
    host tests)."""
    X = np.zeros((nrows, c.mp), dtype=np.float32)
    X[:, :c.m] = np.where(np.random.default_rng(seed).integers(0, 2, size=(nrows, c.m)) > 0, 1.0, -1.0)
    return X


# ---- float64 references on a given factor -------------------------------------------------------------------------------
def xlt_ref(Lh, X):
    """X L^-T: the rows z with z L^T = x."""
    return sla.solve_triangular(Lh, np.asarray(X, dtype=np.float64).T, lower=True).T


def q_ref(Lh, G):
    """q_i = ||L^-1 g_i||^2."""
    return (xlt_ref(Lh, G) ** 2).sum(axis=1)


def sinv_diag_ref(Lh, c, a0=0, a1=None):
    """(S^-1)_aa from identity rows: ||e_a^T L^-T||^2."""
    return (xlt_ref(Lh, identity_rows(c, a0, a1)) ** 2).sum(axis=1)


def potrs_ref(Lh, z):
    """L^-T L^-1 z on the padded factor (z of m entries)."""
    zp = np.zeros(Lh.shape[0])
    zp[:z.size] = z
    y = sla.solve_triangular(Lh, zp, lower=True)
    return sla.solve_triangular(Lh, y, lower=True, trans="T")[:z.size]


# ---- the same operations plainly in float32 -----------------------------------------------------------------------------
def xlt_f32(L32, X32):
    assert L32.dtype == np.float32 and X32.dtype == np.float32
    out = sla.solve_triangular(L32, X32.T, lower=True, check_finite=False).T
    assert out.dtype == np.float32
    return out


def sumsq64(Y):
    return (Y.astype(np.float64) ** 2).sum(axis=1)


def potrs_f32(L32, z):
    zp = np.zeros(L32.shape[0], dtype=np.float32)
    zp[:z.size] = z.astype(np.float32)
    y = sla.solve_triangular(L32, zp, lower=True, check_finite=False)
    out = sla.solve_triangular(L32, y, lower=True, trans="T", check_finite=False)
    assert out.dtype == np.float32
    return out[:z.size]


def rel_err(got, ref):
    """Max-norm distance relative to the reference's largest entry."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


# ---- the library's scheme, restated -------------------------------------------------------------------------------------
def inverted_diagonal_blocks(L32):
    """T_b = (L_bb)^-1 in float64, rounded to float32."""
    nb = L32.shape[0] // NB
    return [sla.solve_triangular(L32[b * NB:(b + 1) * NB, b * NB:(b + 1) * NB].astype(np.float64), np.eye(NB), lower=True).astype(np.float32)
            for b in range(nb)]


def blocked_sweep_f32(L32, X32, skip=None, tinv=None):
    """X L^-T by block forward substitution: Y_b = (X_b - sum_{k < b} Y_k L_bk^T) T_b^T, every product in float32.  ``skip`` =
    (b, k): that block of the factor is left out, as a sweep that lost it would."""
    assert L32.dtype == np.float32 and X32.dtype == np.float32
    nb = L32.shape[0] // NB
    tinv = inverted_diagonal_blocks(L32) if tinv is None else tinv
    Y = X32.copy()
    for b in range(nb):
        acc = Y[:, b * NB:(b + 1) * NB].copy()
        for k in range(b):
            if skip == (b, k):
                continue
            acc -= Y[:, k * NB:(k + 1) * NB] @ L32[b * NB:(b + 1) * NB, k * NB:(k + 1) * NB].T
        Y[:, b * NB:(b + 1) * NB] = acc @ tinv[b].T
    assert Y.dtype == np.float32
    return Y


def two_sweep_f64(L32, tinv, z):
    """The library's vector sweeps restated: L^-T L^-1 z with the fp32 factor's off-diagonal blocks, the diagonal solves as
    products with the given inverted blocks ``tinv`` (nb, 128, 128) taken whole, everything accumulated in float64."""
    mp = L32.shape[0]
    nb = mp // NB
    L, T = L32.astype(np.float64), np.asarray(tinv, dtype=np.float64)
    blk = lambda b: slice(b * NB, (b + 1) * NB)                # noqa: E731
    rhs = np.zeros(mp)
    rhs[:z.size] = z
    y, x = np.zeros(mp), np.zeros(mp)
    for b in range(nb):
        acc = rhs[blk(b)].copy()
        for k in range(b):
            acc -= L[blk(b), blk(k)] @ y[blk(k)]
        y[blk(b)] = T[b] @ acc
    for b in range(nb - 1, -1, -1):
        acc = y[blk(b)].copy()
        for k in range(nb - 1, b, -1):
            acc -= L[blk(k), blk(b)].T @ x[blk(k)]
        x[blk(b)] = T[b].T @ acc
    return x[:z.size]


def potrs_emul_f64(L32, tinv, z):
    """``oisat_potrs`` restated: one pass of ``two_sweep_f64``, the residual against the factor itself, r = z - L (L^T x1) over the
    lower triangle in float64, and a second pass added."""
    m = z.size
    L = np.tril(L32.astype(np.float64))
    x1 = two_sweep_f64(L32, tinv, z)
    xp = np.zeros(L.shape[0])
    xp[:m] = x1
    r = z - (L @ (L.T @ xp))[:m]
    return x1 + two_sweep_f64(L32, tinv, r)


def lower_blocks(L32):
    """[(b, k, Frobenius norm of block (b, k) / Frobenius norm of the factor)] for the strictly-lower 128-blocks."""
    nb = L32.shape[0] // NB
    tot = np.linalg.norm(np.tril(L32).astype(np.float64))
    return [(b, k, float(np.linalg.norm(L32[b * NB:(b + 1) * NB, k * NB:(k + 1) * NB].astype(np.float64)) / tot))
            for b in range(nb) for k in range(b)]


def envelope(c, model="gaussian"):
    """first[] | last[] of ``oisat_envelope_corr`` (host only, no device call) for the case's latitudes; under the Gaussian that
    is ``oisat_envelope``'s table word for word."""
    import ctypes as C
    from oisatgmi import _hip
    env = np.empty(2 * c.nb, dtype=np.int32)
    assert _hip.load_library().oisat_envelope_corr(KINDS[model], c.lat.ctypes.data, c.m, C.c_double(c.g), env.ctypes.data) == 0
    return env
