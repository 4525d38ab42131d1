"""Dense Gaussian-B optimal interpolation on the MI355X (north-star extension).

    x_a = x_b + B H^T (H B H^T + R)^-1 (y - H x_b)
    B = s D^1/2 C D^1/2,  D = diag(Sa),  C_ij = exp(-chord_ij^2 R_earth^2 / (2 L^2)),  R = diag(So)
    H = selection of the grid cell that contains each observation

``corr="gaspari_cohn"`` replaces the Gaussian C by the compactly supported function of Gaspari and Cohn (1999, eq. 4.10) of the
same L (half-support c = L sqrt(10/3), exactly zero beyond 2 c = 3.65 L); ``corr="soar"`` by the second-order autoregressive
function of classical optimal interpolation, the Matern function of nu = 3/2, C = (1 + r/L) exp(-r/L) with r the chord in km
(once differentiable, exponential tails: 2^-52 only at 39.75 L); ``corr="gaussian"`` is the default everywhere.

The reference's ``OI`` (optimal_interpolation.py:6-52) is the L -> 0 limit of this with one
observation per cell: there C = I and K_ii = s Sa_i / (s Sa_i + So_i) (:27).  There is NO
reference implementation of the dense form, so its parity is pinned only in that limit; away from
it the check is the float64 restatement in ``oracle/`` ("parity unpinned").

Pipeline (all in HBM; csrc/dense_cov.hip, dense_chol.hip with dense_gemm.hip and dense_dag.hip (factorization), dense_solve.hip,
dense_post.hip; host tables and plans: dense_tables.hip, dense_dag_plan.hip):
``oisat_innovation`` -> ``oisat_cov_build`` (S, fp32) -> ``oisat_potrf`` (MFMA fp32 Cholesky) ->
``oisat_gain_solve`` (triangular solves + float64-residual refinement) -> ``oisat_apply_increment``
(B H^T z generated on the fly, never stored).  ``DenseAnalysis.run()`` owns the latitude sort of its observations and
therefore builds and factors only the covariance's latitude envelope (``oisat_factor_envelope`` ->
``oisat_cov_build_env_zeroed`` -> ``oisat_potrf_env_fwd``; DESIGN.md section 4.2a: the fp32 factor, a preconditioner, has a
cut-off of its own; the build does not re-zero what is zero, the factorization launch carries the first forward sweep).
``OI_dense(..., superob=box_deg)`` first merges the observations of one box into a superobservation (``superob``,
csrc/superob.hip: ``oisat_superob``), so that a month denser than HBM allows still has a dense analysis.
``OI_dense(..., regions=labels)`` / ``DenseAnalysis.functional_covariance`` report the exact analysis error of regional means, error
correlations between cells included (csrc/dense_functional.hip: ``oisat_functional_gather``, ``oisat_rows_dot``).
``OI_dense(..., likelihood=True)`` / ``DenseAnalysis.log_likelihood`` report how consistent the innovations are with S itself: chi^2 =
d^T S^-1 d, log det S from the factor's diagonal (csrc/dense_likelihood.hip: ``oisat_factor_logdet``) and -2 ln p(d);
``OI_dense(..., fit_scale=)`` / ``DenseAnalysis.fit_error_scales`` estimate the amplitude of B -- and, on request, a common inflation of
R -- by maximum likelihood (``set_error_scales``, ``profile_search``).
``OI_dense(..., ensemble=K)`` / ``DenseAnalysis.posterior_ensemble`` draw K members from the analysis' own error distribution
N(x_a, A) by Matheron's rule, with random-feature prior draws (``ensemble_draws``; csrc/dense_ensemble.hip: ``oisat_field_sample``,
``oisat_member_spread``).
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _hip

EARTH_RADIUS_KM = 6371.0
NB = 128                      # Cholesky block edge (csrc/dense_tile.inc)
SCHEDULE_ENV_DAG, SCHEDULE_ENV_DAG_FWD = 1, 2      # oisat_potrf_env_fwd's schedule_out: the enveloped task graph factored (include/oisat.h)
# relative float64 residual |d - S z| / |d| at which the gain solve stops refining (oisat_gain_solve): the increment is K r
# away from the exact one and |K| <= 1, so the fields are then within 1e-6 |d| -- a tenth of the 1e-5 bar
REFINE_TOL = float(os.environ.get("OISAT_REFINE_TOL", "1e-6"))
# OISAT_RESID_UPDATE_C (include/oisat.h): a residual reported behind a correction may be the update form r_prev - S dz with
# S dz in fp32, within this fraction of |r_prev| of the float64 value
RESID_UPDATE_C = 2.0 ** -10
PROBE_PANEL = 128             # probes per pass of the randomized error estimate (one row panel of oisat_trsm_rows_bwd)


def _mean_and_var(sum2, sum4, K):
    """Mean of K samples x_k^2 and the sample variance of that mean, from sum x_k^2 and sum x_k^4."""
    mean = np.asarray(sum2, dtype=np.float64) / K
    var = np.maximum(np.asarray(sum4, dtype=np.float64) / K - mean * mean, 0.0) / (K - 1)
    return mean, var


def combine_error_estimates(sig2, q, q_var, obs_cell, R, s, s_var):
    """Analysis error variance per cell from the two randomized estimates, pure NumPy.

    ``sig2`` (n,): background variance; ``q``, ``q_var`` (n,): estimate of g_i^T S^-1 g_i and the variance of that estimate;
    ``obs_cell`` (m,) or None: the cell each observation sits on; ``R``, ``s``, ``s_var`` (m,): observation variance, estimate
    of (S^-1)_aa and its variance.  Every cell gets A = sig2 - q with variance q_var.  A cell that carries EXACTLY ONE
    observation a also has A = R_a (1 - R_a s_a), variance R_a^4 s_var_a, which is taken where that variance is the smaller
    one.  A is clipped to [0, sig2], on the singly observed cells to [0, min(sig2, R_a)] (A <= R there: the analysis is no
    worse than the observation).  Returns ``(A, A_var)``."""
    sig2 = np.ravel(np.asarray(sig2, dtype=np.float64))
    A = sig2 - np.ravel(np.asarray(q, dtype=np.float64))
    A_var = np.array(np.ravel(q_var), dtype=np.float64)
    hi = sig2.copy()
    if obs_cell is not None and np.size(obs_cell):
        cell = np.ravel(np.asarray(obs_cell, dtype=np.int64))
        R = np.ravel(np.asarray(R, dtype=np.float64))
        single = np.flatnonzero(np.bincount(cell, minlength=sig2.size)[cell] == 1)     # observations alone on their cell
        ci = cell[single]
        A2 = R[single] * (1.0 - R[single] * np.ravel(s)[single])
        v2 = R[single] ** 4 * np.ravel(s_var)[single]
        take = v2 < A_var[ci]
        A[ci[take]] = A2[take]
        A_var[ci[take]] = v2[take]
        hi[ci] = np.minimum(hi[ci], R[single])
    return np.clip(A, 0.0, hi), A_var


def _ensemble_sizes(nmember, nfeature):
    """``(K, F)`` of a posterior ensemble as ints: K a positive multiple of 32 (the member spread's groups), F >= 1;
    anything else is a ``ValueError``."""
    try:
        K, F = int(nmember), int(nfeature)
        if K != nmember or F != nfeature:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"nmember and nfeature must be integers, not {nmember!r}, {nfeature!r}") from None
    if K < 32 or K % 32:
        raise ValueError(f"nmember must be a positive multiple of 32, got {nmember}")
    if F < 1:
        raise ValueError(f"nfeature must be at least 1, got {nfeature}")
    return K, F


def ensemble_draws(corr, L_km, members, nfeature, m, seed):
    """The random numbers of the posterior ensemble, pure NumPy: for every member number k of
    ``members`` (a range or a list) the ``nfeature`` frequencies and phases of its random-feature prior draw and the ``m``
    unit normals of its observation noise -> ``omega`` (K, F, 3), ``phase`` (K, F), ``eps`` (K, m), all float64.

    Member k draws from ``np.random.Generator(np.random.Philox(key=[seed, k]))`` in the fixed order omega, phase, eps, so it is
    the same member whatever the ensemble's size and whichever panel it lands in.  ``omega`` is in TURNS per unit chord
    (angular frequency / 2 pi), from the spectral measure of the correlation in R^3 with a = R_earth / L and n ~ N(0, I_3):
    ``gaussian`` a n; ``soar`` a n / sqrt(w . w) with an independent w ~ N(0, I_3) -- the trivariate Student t of 3 degrees of
    freedom, the spectral measure of (1 + r/L) exp(-r/L).  ``phase`` is uniform on [0, 1), in turns; ``eps`` belongs to the
    observations in the device's order (ascending latitude).  ``gaspari_cohn`` is a ``ValueError``."""
    kind = corr_kind(corr)
    if kind == CORRELATIONS["gaspari_cohn"]:
        raise ValueError("the spectral measure of gaspari_cohn has no closed-form sampler: the posterior ensemble supports "
                         "gaussian and soar")
    F, m = int(nfeature), int(m)
    if F < 1 or m < 0:
        raise ValueError(f"nfeature must be at least 1 and m non-negative, got {nfeature}, {m}")
    members = [int(k) for k in members]
    if any(k < 0 for k in members):
        raise ValueError("member numbers are non-negative")
    a = EARTH_RADIUS_KM / float(L_km) / (2.0 * np.pi)
    omega = np.empty((len(members), F, 3))
    phase = np.empty((len(members), F))
    eps = np.empty((len(members), m))
    for i, k in enumerate(members):
        rng = np.random.Generator(np.random.Philox(key=[int(seed) & (2 ** 64 - 1), k]))
        n = rng.standard_normal((F, 3))
        if kind == CORRELATIONS["soar"]:
            w = rng.standard_normal((F, 3))
            n /= np.sqrt((w * w).sum(axis=1))[:, None]
        omega[i] = a * n
        phase[i] = rng.random(F)
        eps[i] = rng.standard_normal(m)
    return omega, phase, eps


def unit_vectors(lat_deg, lon_deg) -> np.ndarray:
    """(3, n) float64 unit vectors, SoA as the kernels want them."""
    la = np.deg2rad(np.ravel(np.asarray(lat_deg, dtype=np.float64)))
    lo = np.deg2rad(np.ravel(np.asarray(lon_deg, dtype=np.float64)))
    return np.ascontiguousarray(np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)]))


def morton_order(lat_deg, lon_deg) -> np.ndarray:
    """int32 permutation that lists points along the Z-order curve of (latitude, longitude), 16 bits each: consecutive
    entries are neighbours in space (what ``oisat_set_obs_blocks`` wants)."""
    def spread(v):                                               # 16 bits -> every other bit of 32
        v = v.astype(np.uint32)
        v = (v | (v << 8)) & np.uint32(0x00FF00FF)
        v = (v | (v << 4)) & np.uint32(0x0F0F0F0F)
        v = (v | (v << 2)) & np.uint32(0x33333333)
        v = (v | (v << 1)) & np.uint32(0x55555555)
        return v
    la = np.clip((np.asarray(lat_deg, dtype=np.float64) + 90.0) / 180.0 * 65535.0, 0, 65535)
    lo = np.clip((np.mod(np.asarray(lon_deg, dtype=np.float64) + 180.0, 360.0)) / 360.0 * 65535.0, 0, 65535)
    code = (spread(la.astype(np.uint32)) << np.uint32(1)) | spread(lo.astype(np.uint32))
    return np.argsort(code, kind="stable").astype(np.int32)


# correlation models (include/oisat.h: OISAT_CORR_*)
CORRELATIONS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}     # (3 = 2 nu of the Matern family; 2 is no model)
GC_SUPPORT_PER_L = 2.0 * (10.0 / 3.0) ** 0.5        # Gaspari-Cohn: C = 0 beyond 2 c = 3.6515 L


def _soar_halo_per_l() -> float:
    """s = r / L at which SOAR, (1 + s) exp(-s), has fallen to the Gaussian's value at its 3 L halo, exp(-4.5): the root of
    log1p(s) - s + 4.5 by bisection (the function falls monotonically from 4.5 at s = 0)."""
    lo, hi = 0.0, 16.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if np.log1p(mid) - mid + 4.5 > 0.0:
            lo = mid
        else:
            hi = mid
    return hi


SOAR_HALO_PER_L = _soar_halo_per_l()                # 6.5172: the ``OI_tiled`` halo under ``corr="soar"``, in units of L


def corr_kind(corr) -> int:
    """``"gaussian"`` | ``"gaspari_cohn"`` | ``"soar"`` -> the library's code; anything else is a ``ValueError`` (no device call made)."""
    try:
        return CORRELATIONS[corr]
    except (KeyError, TypeError):
        raise ValueError(f"corr must be one of {sorted(CORRELATIONS)}, not {corr!r}") from None


DRIFT_MAX_DEGREE = 3                                          # include/oisat.h: oisat_drift_basis


def drift_degree(drift):
    """``drift`` of ``DenseAnalysis.run`` / ``OI_dense``: None (no drift) or the degree 0..3 of the harmonics whose
    coefficients are estimated with the analysis; anything else is a ``ValueError``."""
    if drift is None:
        return None
    if isinstance(drift, (bool, np.bool_)) or not isinstance(drift, (int, np.integer)) or not 0 <= int(drift) <= DRIFT_MAX_DEGREE:
        raise ValueError(f"drift is None or a degree 0..{DRIFT_MAX_DEGREE}, not {drift!r}")
    return int(drift)


def drift_coefficients(M, b, tol):
    """The p x p system of universal kriging on the host, float64: ``M`` (symmetrised here) is scaled to unit diagonal,
    factored by Cholesky, and ``beta = M^-1 b``, ``cov beta = M^-1``.  ``ValueError("drift not identifiable ...")`` when the
    Cholesky fails or the 2-norm condition number of the scaled ``M`` exceeds ``1 / tol``: the solves behind ``M`` and ``b`` carry
    a relative error of ``tol``, so beyond that ``beta`` has no correct digit.  Returns ``beta``, ``beta_cov``, ``beta_se``,
    ``cond`` and ``logdet_M``."""
    M = np.asarray(M, dtype=np.float64)
    M = 0.5 * (M + M.T)
    b = np.asarray(b, dtype=np.float64)
    dg = np.diag(M)
    if not (np.all(np.isfinite(M)) and np.all(np.isfinite(b)) and np.all(dg > 0.0)):
        raise ValueError("drift not identifiable: F^T S^-1 F has a non-positive or non-finite diagonal")
    s = 1.0 / np.sqrt(dg)
    Ms = M * s[:, None] * s[None, :]
    ev = np.linalg.eigvalsh(Ms)
    cond = float(ev[-1] / ev[0]) if ev[0] > 0.0 else float("inf")
    limit = 1.0 / max(float(tol), np.finfo(np.float64).eps)
    try:
        if not cond <= limit:
            raise np.linalg.LinAlgError
        Lc = np.linalg.cholesky(Ms)
    except np.linalg.LinAlgError:
        raise ValueError(f"drift not identifiable: the scaled F^T S^-1 F has condition number {cond:.3g}, the solves' tolerance "
                         f"allows {limit:.3g}; lower the degree") from None
    Li = np.linalg.inv(Lc)
    Msi = Li.T @ Li
    beta = s * (Msi @ (s * b))
    cov = Msi * s[:, None] * s[None, :]
    logdet = 2.0 * float(np.sum(np.log(np.diag(Lc)))) - 2.0 * float(np.sum(np.log(s)))
    return {"beta": beta, "beta_cov": cov, "beta_se": np.sqrt(np.diag(cov)), "cond": cond, "logdet_M": logdet}


def latitude_order(lat_deg) -> np.ndarray:
    """The permutation into ascending latitude (stable) that every latitude window of the library assumes."""
    return np.argsort(np.ravel(np.asarray(lat_deg, dtype=np.float64)), kind="stable")


def decay_constant(L_km: float) -> float:
    """g in C = exp(-g * chord^2) for a correlation length L (km)."""
    return 0.5 * (EARTH_RADIUS_KM / float(L_km)) ** 2


def corr_length_of(g: float) -> float:
    """The correlation length (km) of a decay constant: the inverse of ``decay_constant``."""
    return EARTH_RADIUS_KM / float(np.sqrt(2.0 * float(g)))


def regular_grid_cell(lat2, lon2, obs_lat, obs_lon):
    """Flat index of the grid cell containing each observation, for a regular cell-centred grid."""
    lat2 = np.asarray(lat2)
    lon2 = np.asarray(lon2)
    ny, nx = lat2.shape
    dlat = (lat2[-1, 0] - lat2[0, 0]) / max(ny - 1, 1)
    dlon = (lon2[0, -1] - lon2[0, 0]) / max(nx - 1, 1)
    iy = np.clip(np.rint((np.asarray(obs_lat) - lat2[0, 0]) / dlat).astype(np.int64), 0, ny - 1)
    ix = np.clip(np.rint((np.asarray(obs_lon) - lon2[0, 0]) / dlon).astype(np.int64), 0, nx - 1)
    return iy * nx + ix


class DenseAnalysis:
    """Device-resident dense analysis for one grid: upload the grid once, then ``load_obs`` /
    ``run`` per month.  Buffers are sized at ``max_obs`` so nothing is allocated per analysis."""

    def __init__(self, grid_lat, grid_lon, max_obs: int, dtype=np.float32, ctx=None, shared_S=None, out_ptr=None,
                 diag_chunk_rows: int = 0, batched: bool = False):
        """``shared_S``: a factor buffer (``SharedFactor`` or device buffer) shared with other analyses that run one
        after another on the same handle.  ``out_ptr``: device address of 2 n elements where ``xa | inc`` are to be
        written (e.g. a slice of one slab that is gathered over RCCL); by default the plan owns them."""
        self.ctx = ctx or _hip.context()
        self.dt = np.dtype(dtype)
        self.code = _hip.dtype_code(self.dt)
        self.shape = np.shape(grid_lat)
        self._ny, self._nx = (self.shape if len(self.shape) == 2 else (1, int(np.size(grid_lat))))   # cells as a ny x nx grid
        self.n = int(np.size(grid_lat))
        self.max_obs = int(max_obs)
        self.mp_max = -(-self.max_obs // NB) * NB
        c = self.ctx
        self.gxyz = c.upload(unit_vectors(grid_lat, grid_lon))
        self.glat = c.upload(np.ravel(grid_lat), dtype=np.float64)       # latitude window of apply_increment
        # (functional_covariance: the support of a set of functionals is cut out of these on the host)
        self._glat_host = np.ravel(np.asarray(grid_lat, dtype=np.float64))
        self._glon_host = np.ravel(np.asarray(grid_lon, dtype=np.float64))
        item = self.dt.itemsize
        if out_ptr is None:
            # xb | xa | inc; read by torch's RCCL stream when the fields are gathered (parallel.FieldGather)
            self.fields = c.alloc(3 * self.n * item).shared_with_other_streams()
            self.xb_ptr, self.out_ptr = self.fields.at(0), self.fields.at(self.n * item)
        else:
            self.fields = c.alloc(self.n * item)            # xb; xa | inc live in the caller's slab
            self.xb_ptr, self.out_ptr = self.fields.at(0), int(out_ptr)
        self.gsig = c.alloc(self.n * 8)
        m = self.max_obs
        self.oxyz = c.alloc(3 * m * 8)
        self.osig = c.alloc(m * 8)
        self.ovar = c.alloc(m * 8)
        self.ocell = c.alloc(m * 8)
        self.olat = c.alloc(m * 8)
        self.oy = c.alloc(m * 8)
        self.d = c.alloc(m * 8)
        self.z = c.alloc(m * 8)
        # the factor workspace can be shared by analyses that run one after another on the stream (tiles)
        # (a batched plan's S and inverted diagonal blocks are worked on by the BatchedFactor group streams)
        self.S = shared_S if shared_S is not None else c.alloc(self.mp_max * self.mp_max * 4)
        if shared_S is None and batched:
            self.S.shared_with_other_streams()
        if self.S.nbytes < self.mp_max * self.mp_max * 4:
            raise ValueError("shared_S is too small for max_obs")
        # batched factorization (BatchedFactor): the inverted diagonal blocks live in a buffer of this plan, not in the
        # handle's workspace, because many plans of one handle are factored at the same time
        self.tinv = c.alloc(self.mp_max * NB * 4).shared_with_other_streams() if batched else None
        # ... and so do the work vectors and the convergence state of its gain solve (oisat_batch_solve runs on the group's stream)
        self.work = c.alloc(2 * self.mp_max * 8).shared_with_other_streams() if batched else None
        self.state = None
        if batched:
            self.state = c.alloc(256).shared_with_other_streams()
            c.check(c.lib.oisat_memset(c.h, self.state.ptr, 0, 256))
        # the observations along a space-filling curve (compact blocks of rows for the float64 residual)
        self.perm = c.alloc(self.max_obs * 4)
        if batched:
            self.perm.shared_with_other_streams()
        # the block envelope of the latitude-sorted system (``oisat_factor_envelope``): first | last, 2 x mp_max / 128 words
        self.env = c.alloc(2 * (self.mp_max // NB) * 4)
        self._env_host, self._env_key, self._far_host, self._mid_host, self._near_host = None, None, None, None, None
        self._kind = 0                                         # the correlation model of the last run / run_build
        self._g = None                                         # ... and its decay constant: None until a run has happened
        self._fun_bufs = {}                                    # functional_covariance: grow-only device buffers by name
        # What this plan knows about its S between runs (``oisat_cov_build_env_zeroed``): after a build and an enveloped
        # task-graph factorization with table T nothing outside T has been written, so every lower tile left of T is still the
        # exact zero of the fill.  Kept only by a plan that owns its S (a shared or batched buffer is written by others), as
        # (leading dimension, host table, device copy); dropped by anything that writes S any other way.
        self._owns_S = shared_S is None and not batched
        self._zero_claim = None
        self._zero_dev = c.alloc((self.mp_max // NB) * 4) if self._owns_S else None
        self.m = 0
        self._direct_innovation = False
        # the error scales (set_error_scales): host copies of the background sigma and of the sorted
        # observations' sigma_b and variance AS LOADED, which the scaled ones on the device are made from
        self._scales = (1.0, 1.0)
        self._gsig0 = self._osig0 = self._ovar0 = None
        self._lik_ready = False                                # the last run() was one that log_likelihood() may read
        self._drift = None                                     # what the last run(drift=...) estimated (drift_estimate())
        self.last_inc_overlap = False                          # the last run() took oisat_gain_solve_fields
        # every internal workspace of the solve is sized here, so that run() never allocates (include/oisat.h)
        c.check(c.lib.oisat_dense_reserve(c.h, self.max_obs, int(diag_chunk_rows)))

    # ---- inputs
    def load_background(self, Xa, Sa, scale=1.0):
        c = self.ctx
        self._reset_scales()
        c.upload_into(self.xb_ptr, np.ravel(Xa), dtype=self.dt)
        sig = np.sqrt(float(scale) * np.ravel(np.asarray(Sa, dtype=np.float64)))
        self._gsig0 = self._gsig_host = sig
        c.upload_into(self.gsig.ptr, sig, dtype=np.float64)

    # ---- error scales
    def set_error_scales(self, scale_b=1.0, scale_o=1.0):
        """Analyse with ``scale_b`` times the background error variance and ``scale_o`` times the observation error variance
        that were loaded: uploads ``gsig sqrt(scale_b)``, ``osig sqrt(scale_b)`` and ``ovar scale_o`` made from the host
        copies of the loaded ones, and ``_gsig_host`` follows, so that ``posterior_error_mc`` and ``functional_covariance``
        see the scaled variances.  The scales are absolute, not cumulative; every ``load_*`` resets them to 1.  Non-positive
        or non-finite scales are a ``ValueError`` with nothing uploaded."""
        try:
            sb, so = float(scale_b), float(scale_o)
        except (TypeError, ValueError):
            raise ValueError(f"the error scales must be positive finite numbers, not {scale_b!r}, {scale_o!r}") from None
        if not (0.0 < sb < np.inf and 0.0 < so < np.inf):
            raise ValueError(f"the error scales must be positive finite numbers, not {scale_b!r}, {scale_o!r}")
        c, rb = self.ctx, np.sqrt(sb)
        if self._gsig0 is not None:
            self._gsig_host = self._gsig0 * rb
            c.upload_into(self.gsig.ptr, self._gsig_host, dtype=np.float64)
        if self._osig0 is not None:
            c.upload_into(self.osig.ptr, self._osig0 * rb, dtype=np.float64)
            c.upload_into(self.ovar.ptr, self._ovar0 * so, dtype=np.float64)
        self._scales = (sb, so)
        self._lik_ready = False

    def _reset_scales(self, obs=True):
        """Back to the scales 1 ahead of a load; ``obs=False``: the observations are about to be replaced, only the
        background's sigma is put back."""
        if not obs:
            self._osig0 = self._ovar0 = None
        if self._scales != (1.0, 1.0):
            self.set_error_scales(1.0, 1.0)
        self._lik_ready = False
        self._drift = None

    def load_obs_direct(self, obs_lat, obs_lon, obs_sigma_b, obs_var, innovation):
        """Observations whose background value lives outside this plan's grid (tile halos): the caller
        supplies sigma_b at the observation and the innovation d = y - H x_b itself."""
        m = int(np.size(innovation))
        if m < 1 or m > self.max_obs:
            raise ValueError(f"{m} observations; this plan was sized for 1..{self.max_obs}")
        c = self.ctx
        self._reset_scales(obs=False)
        self.m = m
        self.mp = -(-m // NB) * NB
        o = self._sort_by_latitude(obs_lat, obs_lon)
        c.upload_into(self.oxyz.ptr, unit_vectors(np.ravel(obs_lat)[o], np.ravel(obs_lon)[o]))
        self._osig0 = np.ascontiguousarray(np.ravel(obs_sigma_b)[o], dtype=np.float64)
        self._ovar0 = np.ascontiguousarray(np.ravel(obs_var)[o], dtype=np.float64)
        c.upload_into(self.osig.ptr, self._osig0)
        c.upload_into(self.ovar.ptr, self._ovar0)
        c.upload_into(self.d.ptr, np.ravel(innovation)[o], dtype=np.float64)
        self._direct_innovation = True

    def _sort_by_latitude(self, obs_lat, obs_lon):
        """Observations live on the device in ascending-latitude order: the pairs (cell, observation) and
        (observation, observation) whose correlation is above 2^-52 are then contiguous index ranges, which is what the
        latitude windows of ``oisat_apply_increment`` / ``oisat_cov_residual`` skip by.  Per-observation results
        (``download_z``, ``gain_diag``) are handed back in the caller's order."""
        lat = np.ravel(np.asarray(obs_lat, dtype=np.float64))
        self._order = latitude_order(lat)
        self._lat_sorted = np.ascontiguousarray(lat[self._order])
        self._env_host = None                                  # (belongs to these observations, one L and one model: made by run())
        self.ctx.upload_into(self.olat.ptr, self._lat_sorted, dtype=np.float64)
        # ... and the float64 residual takes its blocks of 64 rows along a space-filling curve through them (Morton order of
        # latitude x longitude, as a permutation of the latitude order): neighbours in space, a small bounding sphere
        # (``oisat_set_obs_blocks``)
        lon = np.ravel(np.asarray(obs_lon, dtype=np.float64))[self._order]
        self.ctx.upload_into(self.perm.ptr, morton_order(lat[self._order], lon))
        return self._order

    def _envelope(self, g, kind=0, exact=False):
        """Host table ``first`` of this plan's observations at decay constant ``g`` under correlation model ``kind`` (the
        library's rule and the fp32 factor's cut-off: ``oisat_factor_envelope_corr``); its device copy ``first | last`` is in
        ``self.env``.  With it the far stretch of the factor's K-loops (``oisat_factor_far_corr``: the block columns of every
        row that run on the bf16 pipe), host only, in ``self._far_host``, and the middle stretch behind it (``oisat_factor_mid_corr``:
        split bf16 products) in ``self._mid_host``.  All made once per (observations, L, model, ``exact``).  ``exact``: the table is
        ``oisat_envelope_corr``'s, cut at 2^-52 -- the factor is then that of S itself, not of a truncated matrix, which is what a
        log-determinant needs; the stretches are derived from it all the same."""
        exact = bool(exact)
        if self._env_host is None or self._env_key != (g, kind, exact):
            nb = self.mp // NB
            env = np.empty(2 * nb, dtype=np.int32)
            far = np.empty(nb, dtype=np.int32)
            mid = np.empty(nb, dtype=np.int32)
            table = self.ctx.lib.oisat_envelope_corr if exact else self.ctx.lib.oisat_factor_envelope_corr
            self.ctx.check(table(kind, self._lat_sorted.ctypes.data, self.m, g, env.ctypes.data))
            self.ctx.check(self.ctx.lib.oisat_factor_far_corr(kind, self._lat_sorted.ctypes.data, self.m, g, env.ctypes.data,
                                                              far.ctypes.data))
            self.ctx.check(self.ctx.lib.oisat_factor_mid_corr(kind, self._lat_sorted.ctypes.data, self.m, g, env.ctypes.data,
                                                              far.ctypes.data, mid.ctypes.data))
            near = np.empty(nb, dtype=np.int32)
            self.ctx.check(self.ctx.lib.oisat_factor_near_corr(kind, self._lat_sorted.ctypes.data, self.m, g, env.ctypes.data,
                                                               mid.ctypes.data, near.ctypes.data))
            self.ctx.upload_into(self.env.ptr, env)
            self._env_host, self._env_key, self._far_host, self._mid_host, self._near_host = env, (g, kind, exact), far, mid, near
        return self._env_host

    def _unsort(self, per_obs):
        out = np.empty_like(per_obs)
        out[self._order] = per_obs
        return out

    def load_obs(self, obs_lat, obs_lon, obs_cell, obs_y, obs_var):
        self._direct_innovation = False
        m = int(np.size(obs_y))
        if m < 1 or m > self.max_obs:
            raise ValueError(f"{m} observations; this plan was sized for 1..{self.max_obs}")
        c = self.ctx
        self._reset_scales(obs=False)
        self.m = m
        self.mp = -(-m // NB) * NB
        o = self._sort_by_latitude(obs_lat, obs_lon)
        cell = np.ascontiguousarray(np.ravel(obs_cell)[o], dtype=np.int64)
        self._cell_sorted = cell                               # (posterior_error_mc: which cells carry exactly one observation)
        c.upload_into(self.oxyz.ptr, unit_vectors(np.ravel(obs_lat)[o], np.ravel(obs_lon)[o]))
        self._osig0 = np.ascontiguousarray(self._gsig_host[cell], dtype=np.float64)
        self._ovar0 = np.ascontiguousarray(np.ravel(obs_var)[o], dtype=np.float64)
        c.upload_into(self.osig.ptr, self._osig0)
        c.upload_into(self.ovar.ptr, self._ovar0)
        c.upload_into(self.ocell.ptr, cell)
        c.upload_into(self.oy.ptr, np.ravel(obs_y)[o], dtype=np.float64)

    # ---- the hot path: everything below runs on the device, enqueued on the handle's stream
    def run(self, L_km: float, refine: int = 2, check_pd: bool = False, want_resid: bool = False, tol=None, corr="gaussian",
            fields: bool = True, exact_factor: bool = False, drift=None):
        """``refine``: the most refinement rounds the gain solve may take; it stops earlier once the float64 residual is
        below ``tol`` |d| (default: the handle's, 1e-6 -- ``oisat_set_refine_tol``; 0 runs every round).  ``corr``: the
        correlation model, ``"gaussian"``, ``"gaspari_cohn"`` or ``"soar"`` (same L; module docstring).  ``fields=False``: stop
        behind the gain solve, the increment is not spread (``z`` and the factor are all a likelihood needs).
        ``exact_factor=True``: build and factor inside the 2^-52 envelope instead of the fp32 factor's own, narrower one, so that
        the factor's log-determinant is that of S (``log_likelihood``).
        ``drift``: None (default: the path and the bits of a run without it) or a degree 0..3: the innovations are modelled as
        d = F beta + e with F the (degree + 1)^2 real harmonics up to that degree at the observations and beta unknown with a flat
        prior (universal kriging).  One block solve S [z_d, Y_F] = [d, F] (``oisat_gain_solve_multi``),
        beta = M^-1 b from M = F^T Y_F and b = F^T z_d on the host (``drift_coefficients``), z' = z_d - Y_F beta -- what
        ``download_z()`` then returns -- and the increment is B H^T z' plus the drift itself (``oisat_drift_apply``);
        ``drift_estimate()``, ``drift_variance()`` and ``log_likelihood()`` describe the result.  ``ValueError("drift not
        identifiable ...")`` with fewer observations than coefficients, or where M cannot be inverted to the solves' tolerance.
        This one synchronises (the p x p system is solved on the host); ``want_resid`` then reports the innovation's column."""
        deg = drift_degree(drift)
        if deg is not None and self.m < (deg + 1) ** 2:
            raise ValueError(f"drift not identifiable: {self.m} observations for {(deg + 1) ** 2} coefficients")
        kind = self._kind = corr_kind(corr)
        self._lik_ready = False
        self._drift = None
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        c.check(lib.oisat_set_refine_tol(h, REFINE_TOL if tol is None else float(tol)))      # per run: handles are shared
        c.check(lib.oisat_set_correlation(h, kind))                                          # ... and so is the model
        m, ld = self.m, self.mp
        g = self._g = decay_constant(L_km)
        item = self.dt.itemsize
        xb, xa, inc = self.xb_ptr, self.out_ptr, self.out_ptr + self.n * item
        if not self._direct_innovation:
            c.check(lib.oisat_innovation(h, self.code, xb, self.ocell.ptr, self.oy.ptr, m, self.d.ptr))
        # this plan owns the latitude sort, so it may use the covariance's envelope: only the tiles inside it are evaluated
        # and factored, the sweeps of the gain solve walk inside it (OISAT_ENVELOPE=0: the dense path, in the library)
        first = self._envelope(g, kind, exact_factor)
        # the build fills with zeros only what the last run's envelope left outside this one's (equal tables: nothing), the
        # factorization launch carries the first forward sweep of the gain solve (OISAT_FWD_IN_LAUNCH=0: it does not)
        claim, self._zero_claim = self._zero_claim, None       # (an exception below leaves no claim behind)
        if claim is not None and claim[0] != ld:
            claim = None
        enveloped, schedule = C.c_int(0), C.c_int(0)
        c.check(lib.oisat_cov_build_env_zeroed(h, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, g, self.S.ptr, ld, first.ctypes.data,
                                               self.env.ptr, claim[1].ctypes.data if claim else None,
                                               self._zero_dev.ptr if claim else None, C.byref(enveloped)))
        info = C.c_int(0)
        c.check(lib.oisat_set_factor_far(h, self._far_host.ctypes.data, self._far_host.size))        # per run: handles are shared
        c.check(lib.oisat_set_factor_mid(h, self._mid_host.ctypes.data, self._mid_host.size))
        c.check(lib.oisat_set_factor_near(h, self._near_host.ctypes.data, self._near_host.size))
        c.check(lib.oisat_potrf_env_fwd(h, self.S.ptr, m, ld, first.ctypes.data, self.env.ptr, self.d.ptr,
                                        C.byref(info) if check_pd else None, C.byref(schedule)))
        self.last_schedule = schedule.value                    # (SCHEDULE_*: which factorization ran, for tests and profiles)
        resid = (C.c_double * (refine + 1))() if want_resid else None
        c.check(lib.oisat_set_obs_blocks(h, self.perm.ptr, m))                                  # per run: handles are shared
        # the solve and the fields as ONE call where the library's rule allows (oisat_inc_overlap_plan; OISAT_INC_OVERLAP): the
        # increment of the first solve then runs underneath the correction's sweeps (include/oisat.h: oisat_gain_solve_fields)
        overlap = C.c_int32(0)
        c.check(lib.oisat_inc_overlap_plan(self.mp // NB, 1, kind, int(refine), int(bool(fields)), int(deg is not None),
                                           C.byref(overlap)))
        self.last_inc_overlap = bool(overlap.value)            # (for tests and profiles)
        if overlap.value:
            c.check(lib.oisat_gain_solve_fields(h, self.S.ptr, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, ld, g, self.d.ptr,
                                                int(refine), self.z.ptr, resid, self.olat.ptr, self.code, self.gxyz.ptr,
                                                self.gsig.ptr, self._ny, self._nx, xb, xa, inc, self.glat.ptr))
        elif deg is None:
            c.check(lib.oisat_gain_solve(h, self.S.ptr, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, ld, g, self.d.ptr,
                                         int(refine), self.z.ptr, resid, self.olat.ptr))
        else:
            col0 = self._drift_solve(deg, int(refine), REFINE_TOL if tol is None else float(tol))
            if want_resid:
                resid = col0
        if fields and not overlap.value:
            c.check(lib.oisat_apply_increment_grid(h, self.code, self.gxyz.ptr, self.gsig.ptr, self._ny, self._nx, self.oxyz.ptr,
                                                   self.osig.ptr, self.z.ptr, m, g, xb, xa, inc, self.glat.ptr, self.olat.ptr))
            if deg is not None:
                c.check(lib.oisat_drift_apply(h, self.code, self.gxyz.ptr, self.n, deg, self._functional_buffer("drift_beta", 16 * 8).ptr,
                                              xa, inc))
        self._lik_ready = bool(check_pd) and bool(exact_factor)
        if self._owns_S and enveloped.value == 1 and schedule.value in (SCHEDULE_ENV_DAG, SCHEDULE_ENV_DAG_FWD):
            nb = self.mp // NB
            if claim is None or not np.array_equal(claim[1], first[:nb]):
                table = np.ascontiguousarray(first[:nb])
                c.upload_into(self._zero_dev.ptr, table)
                claim = (ld, table)
            self._zero_claim = claim
        return list(resid) if want_resid else None

    # ---- the same pipeline in two halves, for lock-step (batched) factorization of many plans: build | factor | solve
    def run_build(self, L_km: float, corr="gaussian"):
        kind = self._kind = corr_kind(corr)
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        c.check(lib.oisat_set_correlation(h, kind))             # per run: handles are shared
        g = self._g = decay_constant(L_km)
        self._zero_claim = None                                 # (a dense build: S holds correlations everywhere)
        if not self._direct_innovation:
            c.check(lib.oisat_innovation(h, self.code, self.xb_ptr, self.ocell.ptr, self.oy.ptr, self.m, self.d.ptr))
        c.check(lib.oisat_cov_build(h, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, self.m, g, self.S.ptr, self.mp))

    def run_solve(self, refine: int = 2, tol=None):
        if self.tinv is None:
            raise ValueError("run_build / run_solve belong to plans created with batched=True (they own their inverted "
                             "diagonal blocks); use run() for a plan that factors on its own handle")
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        m, ld, g = self.m, self.mp, self._g
        item = self.dt.itemsize
        xb, xa, inc = self.xb_ptr, self.out_ptr, self.out_ptr + self.n * item
        c.check(lib.oisat_set_refine_tol(h, REFINE_TOL if tol is None else float(tol)))
        c.check(lib.oisat_set_correlation(h, self._kind))       # (the model of this plan's run_build)
        c.check(lib.oisat_factor_adopt(h, self.S.ptr, m, ld, self.tinv.ptr))
        c.check(lib.oisat_set_obs_blocks(h, self.perm.ptr, m))
        c.check(lib.oisat_gain_solve(h, self.S.ptr, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, ld, g, self.d.ptr,
                                     int(refine), self.z.ptr, None, self.olat.ptr))
        c.check(lib.oisat_apply_increment_grid(h, self.code, self.gxyz.ptr, self.gsig.ptr, self._ny, self._nx, self.oxyz.ptr,
                                               self.osig.ptr, self.z.ptr, m, g, xb, xa, inc, self.glat.ptr, self.olat.ptr))

    # ---- posterior diagnostics (after run(); they reuse the factor that run() left in HBM)
    def posterior_error(self, chunk_rows: int = 4096):
        """sqrt(diag(B - B H^T S^-1 H B)) on every grid cell, float32 (n m^2 flop: regional / tiled sizes)."""
        c = self.ctx
        if not hasattr(self, "_err"):
            self._err = c.alloc(self.n * 4)
        g = self._g
        c.check(c.lib.oisat_set_correlation(c.h, self._kind))   # (the model of the run that left the factor)
        c.check(c.lib.oisat_posterior_error(c.h, self.S.ptr, self.m, self.mp, self.gxyz.ptr, self.gsig.ptr, self.n, 0, self.n,
                                            self.oxyz.ptr, self.osig.ptr, g, int(chunk_rows), self._err.ptr))
        return c.download(self._err.ptr, self.shape, np.float32)

    def gain_diag(self, chunk_rows: int = 4096):
        """diag(K H) at the observations (the averaging kernel of the dense analysis), float64 (m,)."""
        c = self.ctx
        if not hasattr(self, "_ak"):
            self._ak = c.alloc(self.max_obs * 8)
        c.check(c.lib.oisat_gain_diag(c.h, self.S.ptr, self.m, self.mp, self.ovar.ptr, int(chunk_rows), self._ak.ptr))
        return self._unsort(c.download(self._ak.ptr, (self.m,), np.float64))

    def posterior_error_mc(self, nprobe: int = 256, seed: int = 0, gridded: bool = False):
        """Randomized estimate of ``posterior_error()`` and ``gain_diag()`` from ``nprobe`` Rademacher probes pushed through
        the factor that ``run()`` left in HBM: u = L^-T w has E[u u^T] = S^-1, so the error
        variance is sig_i^2 - E[(g_i^T u)^2] and diag(K H) at observation a is 1 - R_aa E[u_a^2].  Panels of 128 probes:
        fill, backward row sweep, then the per-observation and per-cell sums of squares and fourth powers (accumulating).
        ``gridded``: every observation sits on its cell's centre (``OI_dense`` without ``obs``); a cell that carries exactly
        one observation then has the second estimate R_aa ak_a (``combine_error_estimates``).
        Returns ``err`` (grid shape, float32), ``err_se``, ``ak_obs`` (m, caller order), ``ak_obs_se``, ``nprobe`` and the
        raw estimates ``q`` / ``q_se`` (cells) and ``s`` / ``s_se`` (observations, caller order).  Every standard error is the
        sample's own, from its fourth moments; same seed, same bits."""
        K = int(nprobe)
        if K < PROBE_PANEL or K % PROBE_PANEL:
            raise ValueError(f"nprobe must be a positive multiple of {PROBE_PANEL}, got {nprobe}")
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        m, mp, n = self.m, self.mp, self.n
        if not hasattr(self, "_probe"):
            self._probe = c.alloc(PROBE_PANEL * self.mp_max * 4)        # one panel of probes, allocated once
            self._mc_sums = c.alloc(2 * (self.n + self.max_obs) * 8)    # sum2 | sum4 of the cells, then of the observations
        cell2, cell4 = self._mc_sums.at(0), self._mc_sums.at(n * 8)
        obs2, obs4 = self._mc_sums.at(2 * n * 8), self._mc_sums.at((2 * n + self.max_obs) * 8)
        c.check(lib.oisat_set_correlation(h, self._kind))               # (the model of the run that left the factor)
        ny, nx = self._ny, self._nx
        for p in range(K // PROBE_PANEL):
            acc = 1 if p else 0
            c.check(lib.oisat_probe_fill(h, int(seed) & (2 ** 64 - 1), p * PROBE_PANEL, self._probe.ptr, PROBE_PANEL, mp, m))
            c.check(lib.oisat_trsm_rows_bwd(h, self.S.ptr, m, mp, self._probe.ptr, PROBE_PANEL, mp))
            c.check(lib.oisat_probe_diag(h, self._probe.ptr, PROBE_PANEL, mp, m, acc, obs2, obs4))
            c.check(lib.oisat_probe_spread(h, self.gxyz.ptr, self.gsig.ptr, ny, nx, self.oxyz.ptr, self.osig.ptr, self._probe.ptr,
                                           PROBE_PANEL, mp, m, self._g, self.glat.ptr, self.olat.ptr, acc, cell2, cell4))
        self.check()
        cs = c.download(cell2, (2, n), np.float64)
        q, q_var = _mean_and_var(cs[0], cs[1], K)
        s, s_var = _mean_and_var(c.download(obs2, (m,), np.float64), c.download(obs4, (m,), np.float64), K)
        R = c.download(self.ovar.ptr, (m,), np.float64)
        sig2 = np.asarray(self._gsig_host, dtype=np.float64) ** 2
        obs_cell = getattr(self, "_cell_sorted", None) if gridded and not self._direct_innovation else None
        A, A_var = combine_error_estimates(sig2, q, q_var, obs_cell, R, s, s_var)
        err = np.sqrt(A)
        with np.errstate(divide="ignore", invalid="ignore"):
            err_se = np.where(err > 0, np.sqrt(A_var) / (2.0 * err), 0.0)
        return {"err": err.reshape(self.shape).astype(np.float32), "err_se": err_se.reshape(self.shape),
                "ak_obs": self._unsort(1.0 - R * s), "ak_obs_se": self._unsort(R * np.sqrt(s_var)), "nprobe": K,
                "q": q.reshape(self.shape), "q_se": np.sqrt(q_var).reshape(self.shape),
                "s": self._unsort(s), "s_se": self._unsort(np.sqrt(s_var))}

    # ---- posterior ensembles by Matheron's rule
    def _ensemble_panels(self, K, F, seed, keep, L_km, corr, solve):
        """The panel loop of ``posterior_ensemble`` (``solve``: the whole rule) and ``prior_ensemble`` (step 4 alone) ->
        ``(sum2, sum4, deviations or None)`` with the per-cell sums of squares and fourth powers over the K members in float64."""
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        n, ny, nx = self.n, self._ny, self._nx
        m, mp = (self.m, self.mp) if solve else (0, 0)
        rows_max = min(K, PROBE_PANEL)
        P = self._functional_buffer("ens_P", rows_max * n * 4)                 # one panel of members on the grid
        feat = self._functional_buffer("ens_feat", rows_max * 4 * F * 8)       # omega [rows][3][F] | phase [rows][F]
        sums = self._functional_buffer("ens_sums", 2 * n * 8)
        if solve:
            X = self._functional_buffer("ens_X", PROBE_PANEL * self.mp_max * 4)    # the panel at the observations
            noise = self._functional_buffer("ens_noise", PROBE_PANEL * self.mp_max * 4)
            c.check(lib.oisat_set_correlation(h, self._kind))                  # (the model of the run that left the factor)
        dev = np.empty((K, n), dtype=np.float32) if keep else None
        s2, s4 = np.zeros(n), np.zeros(n)
        for p0 in range(0, K, PROBE_PANEL):
            rows = min(PROBE_PANEL, K - p0)                                    # live rows: a multiple of 32
            omega, phase, eps = ensemble_draws(corr, L_km, range(p0, p0 + rows), F, m, seed)
            c.upload_into(feat.ptr, np.ascontiguousarray(omega.transpose(0, 2, 1)), dtype=np.float64)
            c.upload_into(feat.at(rows * 3 * F * 8), phase, dtype=np.float64)
            om, ph = feat.ptr, feat.at(rows * 3 * F * 8)
            c.check(lib.oisat_field_sample(h, self.gxyz.ptr, n, self.gsig.ptr, om, ph, F, rows, None, None, P.ptr, n))
            if not solve:
                got = c.download(P.ptr, (rows, n), np.float32)
                d64 = got.astype(np.float64) ** 2
                s2 += d64.sum(axis=0)
                s4 += (d64 * d64).sum(axis=0)
            else:
                # the sweeps want 128 rows.  oisat_field_sample writes every one of the mp columns of the live rows (zeros from m
                # on), so only a short panel needs the memset: it makes the rows behind the live ones zero rows
                if rows < PROBE_PANEL:
                    c.check(lib.oisat_memset(h, X.ptr, 0, PROBE_PANEL * mp * 4))
                e32 = np.zeros((rows, mp), dtype=np.float32)
                e32[:, :m] = eps
                c.upload_into(noise.ptr, e32, dtype=np.float32)
                c.check(lib.oisat_field_sample(h, self.oxyz.ptr, m, self.osig.ptr, om, ph, F, rows, noise.ptr, self.ovar.ptr, X.ptr, mp))
                c.check(lib.oisat_trsm_rows(h, self.S.ptr, m, mp, X.ptr, PROBE_PANEL, mp))
                c.check(lib.oisat_trsm_rows_bwd(h, self.S.ptr, m, mp, X.ptr, PROBE_PANEL, mp))
                c.check(lib.oisat_member_spread(h, self.gxyz.ptr, self.gsig.ptr, ny, nx, self.oxyz.ptr, self.osig.ptr, X.ptr, rows, mp, m,
                                                self._g, self.glat.ptr, self.olat.ptr, P.ptr, n, 1 if p0 else 0, sums.at(0), sums.at(n * 8)))
                if keep:
                    got = c.download(P.ptr, (rows, n), np.float32)
            if keep:
                dev[p0:p0 + rows] = got
        if solve:
            self.check()
            s2, s4 = c.download(sums.ptr, (2, n), np.float64)
        return s2, s4, dev

    def _ensemble_result(self, A, A_var, dev, K, F, seed):
        err = np.sqrt(A)
        with np.errstate(divide="ignore", invalid="ignore"):
            err_se = np.where(err > 0, np.sqrt(A_var) / (2.0 * err), 0.0)
        return {"err": err.reshape(self.shape).astype(np.float32), "err_se": err_se.reshape(self.shape),
                "deviations": None if dev is None else dev.reshape((K,) + tuple(self.shape)), "nmember": K, "nfeature": F,
                "seed": int(seed)}

    def posterior_ensemble(self, nmember: int = 32, nfeature: int = 256, seed: int = 0, keep: bool = True):
        """``nmember`` draws from N(x_a, A), A = B - B H^T S^-1 H B, by Matheron's rule through the factor that ``run()`` left in
        HBM: delta_k = xi_k - B H^T S^-1 (H xi_k + eps_k) with xi_k ~ N(0, B) a random-feature field
        of ``nfeature`` frequencies (``ensemble_draws``; ``gaussian`` and ``soar``, ``gaspari_cohn`` is a ``ValueError``) and
        eps_k ~ N(0, R).  Panels of 128 members (the last one padded with zero rows): the draws are made on the host and
        uploaded, ``oisat_field_sample`` at the observations with the noise added, ``oisat_trsm_rows`` and
        ``oisat_trsm_rows_bwd``, ``oisat_field_sample`` on the grid with the same frequencies, ``oisat_member_spread``.  The
        solve is the fp32 factor's, UNREFINED -- the grade of solve ``posterior_error_mc`` uses -- so a member carries the
        factor's own cut (its envelope, fp32 rounding) beside its sampling noise.  The device copies of the sigmas and
        variances are used, so ``set_error_scales`` is honoured.
        Returns ``err`` (grid shape, float32: the root of the members' mean square -- the mean is known to be zero, K degrees
        of freedom), ``err_se`` (from the fourth moments; 0 where err is 0), ``deviations`` ((K, ny, nx) float32, add x_a for
        members of the analysis; None with ``keep=False``), ``nmember``, ``nfeature``, ``seed``.  The relative standard error
        of err^2 is sqrt(2 / K) of ITSELF, however well a cell is observed.  A cell whose background sigma is 0 has deviation
        0.  Member k is the same for every ``nmember``; same seed, same bits."""
        if not self.m or self._g is None:
            raise ValueError("posterior_ensemble() must follow run(): it reads the factor that run() leaves behind")
        K, F = _ensemble_sizes(nmember, nfeature)
        corr = {v: k for k, v in CORRELATIONS.items()}[self._kind]
        L_km = corr_length_of(self._g)
        ensemble_draws(corr, L_km, [], F, 0, seed)              # (gaspari_cohn: ValueError before any device call)
        s2, s4, dev = self._ensemble_panels(K, F, seed, keep, L_km, corr, solve=True)
        A, A_var = _mean_and_var(s2, s4, K)
        return self._ensemble_result(A, A_var, dev, K, F, seed)

    def prior_ensemble(self, L_km, corr="gaussian", nmember: int = 32, nfeature: int = 256, seed: int = 0, keep: bool = True):
        """The ensemble where nothing was observed: ``nmember`` draws from N(0, B) -- ``oisat_field_sample`` on the grid alone
        -- in the dictionary of ``posterior_ensemble``.  Needs the background only.  Unlike ``posterior_ensemble``, whose ``err`` is
        the members' own root mean square, ``err`` here is NOT a sample statistic: it is the background sigma that was loaded,
        which is known exactly.  Only ``err_se`` comes from the sample (the variance of its squares, summed on the host from the
        fields as they are read back, over 2 err): it says how far a sample of this size would scatter about that value."""
        K, F = _ensemble_sizes(nmember, nfeature)
        ensemble_draws(corr, L_km, [], F, 0, seed)              # (ValueError before any device call)
        if getattr(self, "_gsig_host", None) is None:
            raise ValueError("load_background() first: the prior draws are scaled by the background error")
        s2, s4, dev = self._ensemble_panels(K, F, seed, keep, float(L_km), corr, solve=False)
        _, A_var = _mean_and_var(s2, s4, K)
        return self._ensemble_result(np.asarray(self._gsig_host, dtype=np.float64) ** 2, A_var, dev, K, F, seed)

    # ---- analysis error of linear functionals: regional means
    def _functional_buffer(self, name, nbytes):
        """Grow-only device buffer ``name`` of this plan."""
        bufs = self._fun_bufs
        if name not in bufs or bufs[name].nbytes < nbytes:
            bufs[name] = self.ctx.alloc(int(nbytes))
        return bufs[name]

    def _functional_support(self, W):
        """``W`` as (K, n) float64 and the support of its rows: the cells where any row is non-zero and the background sigma
        is finite and positive, in ascending latitude (stable).  Pure host work; every bad argument is a ``ValueError``."""
        W = np.asarray(W, dtype=np.float64)
        if W.ndim == 3 and W.shape[1:] == tuple(self.shape):
            W = W.reshape(W.shape[0], -1)
        if W.ndim != 2 or W.shape[1] != self.n:
            raise ValueError(f"W must be (K, {self.n}) or (K,) + {tuple(self.shape)}, not {W.shape}")
        if not 1 <= W.shape[0] <= 64:
            raise ValueError(f"1 to 64 functionals per call, not {W.shape[0]}")
        sig = getattr(self, "_gsig_host", None)
        if sig is None:
            raise ValueError("load_background() first: the functionals are weighted by the background error")
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(sig) & (sig > 0.0)
        sup = np.flatnonzero((W != 0.0).any(axis=0) & ok)
        sup = sup[latitude_order(self._glat_host[sup])]
        return W, sup

    def _functional_upload(self, W, sup):
        """Unit vectors, sigma, latitudes and the K x nsrc weight block of the support -> device (grow-only buffers)."""
        c = self.ctx
        K, ns = W.shape[0], sup.size
        sx = self._functional_buffer("sxyz", 3 * ns * 8)
        ss = self._functional_buffer("ssig", ns * 8)
        sl = self._functional_buffer("slat", ns * 8)
        sw = self._functional_buffer("W", K * ns * 8)
        c.upload_into(sx.ptr, unit_vectors(self._glat_host[sup], self._glon_host[sup]))
        c.upload_into(ss.ptr, self._gsig_host[sup], dtype=np.float64)
        c.upload_into(sl.ptr, self._glat_host[sup], dtype=np.float64)
        c.upload_into(sw.ptr, W[:, sup], dtype=np.float64)
        return sx, ss, sl, sw

    def functional_prior(self, W, L_km=None, corr=None):
        """``W B W^T`` alone, (K, K) float64, symmetric: the error covariance of the functionals before any observation.
        Needs the background only; ``L_km`` / ``corr`` default to those of the last ``run()``."""
        if L_km is None and self._g is None:
            raise ValueError("functional_prior() without L_km must follow run()")
        W, sup = self._functional_support(W)
        K, ns = W.shape[0], int(sup.size)
        if ns == 0:
            return np.zeros((K, K))
        g = self._g if L_km is None else decay_constant(L_km)
        kind = self._kind if corr is None else corr_kind(corr)
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        sx, ss, sl, sw = self._functional_upload(W, sup)
        T = self._functional_buffer("T", K * ns * 8)
        small = self._functional_buffer("small", (3 * 64 + 2) * 64 * 8)
        c.check(lib.oisat_set_correlation(h, kind))
        c.check(lib.oisat_functional_gather(h, sx.ptr, ss.ptr, sl.ptr, ns, sx.ptr, ss.ptr, sl.ptr, ns, sw.ptr, K, ns, g, T.ptr, ns))
        c.check(lib.oisat_rows_dot(h, sw.ptr, ns, K, T.ptr, ns, K, ns, small.ptr))
        prior = c.download(small.ptr, (K, K), np.float64)
        return 0.5 * (prior + prior.T)

    def functional_covariance(self, W, refine: int = 2, tol=None):
        """Exact analysis error covariance of K linear functionals ``W`` ((K, ny, nx) or (K, n); a row = weights over cells,
        e.g. ``region_weights``): A_W = W B W^T - G^T S^-1 G with G = H B W^T, through the factor that ``run()`` left in HBM.
        Two float64 pair sums (``oisat_functional_gather``: G at the observations, T = B W^T at the support), one refined
        gain solve S y_k = g_k per functional, its float64 residual r_k = g_k - S y_k, and the residual-corrected reduction
        G^T Y + R^T Y = G^T S^-1 G - R^T S^-1 R, whose error is second order in the residual and never understates a
        variance.  Returns ``prior``, ``reduction``, ``posterior`` ((K, K) float64, symmetric), ``resid`` ((K,), |r_k| / |g_k|)
        and ``support`` (cells that carry weight).  A functional with empty support gives zero rows and columns."""
        if not self.m or self._g is None:
            raise ValueError("functional_covariance() must follow run(): it reads the factor that run() leaves behind")
        W, sup = self._functional_support(W)
        K, ns, m, mp = W.shape[0], int(sup.size), self.m, self.mp
        zero = np.zeros((K, K))
        if ns == 0:
            return {"prior": zero, "reduction": zero.copy(), "posterior": zero.copy(), "resid": np.zeros(K), "support": 0}
        live = np.flatnonzero((W[:, sup] != 0.0).any(axis=1))
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        g, kind = self._g, self._kind
        sx, ss, sl, sw = self._functional_upload(W, sup)
        T = self._functional_buffer("T", K * ns * 8)
        gyr = self._functional_buffer("GYR", 3 * K * self.mp_max * 8)       # G | Y | R, rows of mp doubles (g_k is a right-hand side)
        small = self._functional_buffer("small", (3 * 64 + 2) * 64 * 8)   # W T^T | G^T Y | R^T Y | |g_k|^2 | |r_k|^2
        G, Y, R = gyr.at(0), gyr.at(K * mp * 8), gyr.at(2 * K * mp * 8)
        c.check(lib.oisat_memset(h, gyr.ptr, 0, 3 * K * mp * 8))
        c.check(lib.oisat_memset(h, small.ptr, 0, (3 * K + 2) * K * 8))
        c.check(lib.oisat_set_correlation(h, kind))
        c.check(lib.oisat_functional_gather(h, self.oxyz.ptr, self.osig.ptr, self.olat.ptr, m, sx.ptr, ss.ptr, sl.ptr, ns, sw.ptr, K,
                                            ns, g, G, mp))
        c.check(lib.oisat_functional_gather(h, sx.ptr, ss.ptr, sl.ptr, ns, sx.ptr, ss.ptr, sl.ptr, ns, sw.ptr, K, ns, g, T.ptr, ns))
        KK = K * K * 8
        c.check(lib.oisat_rows_dot(h, sw.ptr, ns, K, T.ptr, ns, K, ns, small.at(0)))
        for k in map(int, live):
            gk, yk, rk = G + k * mp * 8, Y + k * mp * 8, R + k * mp * 8
            c.check(lib.oisat_set_refine_tol(h, REFINE_TOL if tol is None else float(tol)))      # per call: handles are shared
            c.check(lib.oisat_set_correlation(h, kind))
            c.check(lib.oisat_set_obs_blocks(h, self.perm.ptr, m))                               # (one-shot: the solve takes it)
            c.check(lib.oisat_gain_solve(h, self.S.ptr, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, mp, g, gk, int(refine), yk,
                                         None, self.olat.ptr))
            c.check(lib.oisat_cov_residual(h, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, g, gk, yk, rk, self.olat.ptr))
            c.check(lib.oisat_rows_dot(h, gk, mp, 1, gk, mp, 1, m, small.at(3 * KK + k * 8)))     # |g_k|^2, |r_k|^2
            c.check(lib.oisat_rows_dot(h, rk, mp, 1, rk, mp, 1, m, small.at(3 * KK + (K + k) * 8)))
        c.check(lib.oisat_rows_dot(h, G, mp, K, Y, mp, K, m, small.at(KK)))
        c.check(lib.oisat_rows_dot(h, R, mp, K, Y, mp, K, m, small.at(2 * KK)))
        self.check()
        out = c.download(small.ptr, ((3 * K + 2) * K,), np.float64)
        prior, gy, ry = out[:3 * K * K].reshape(3, K, K)
        return assemble_functional_covariance(prior, gy, ry, out[3 * K * K:3 * K * K + K], out[3 * K * K + K:], ns)

    # ---- a drift of the innovations
    def _drift_solve(self, deg, refine, tol):
        """Behind the factorization of ``run(drift=deg)``: the basis at the observations in their stored order, the block solve,
        the p x p system on the host and z' -> ``self.z``; beta -> the device buffer ``drift_beta``.  Returns the innovation
        column's relative residuals (refine + 1)."""
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        m, ld, g = self.m, self.mp, self._g
        p = (deg + 1) ** 2
        nr = p + 1
        blk = self._functional_buffer("drift", (2 * nr * self.mp_max + nr * nr) * 8)      # [d | F] | [z_d | Y_F] | their products
        D, Z, small = blk.at(0), blk.at(nr * ld * 8), blk.at(2 * nr * ld * 8)
        c.check(lib.oisat_affine(h, _hip.dtype_code(np.dtype(np.float64)), self.d.ptr, m, 0.0, 1.0, D))      # a copy of d: (d - 0) / 1
        c.check(lib.oisat_drift_basis(h, self.oxyz.ptr, m, deg, D + ld * 8, ld))
        resid = (C.c_double * ((refine + 1) * nr))()
        c.check(lib.oisat_gain_solve_multi(h, self.S.ptr, self.oxyz.ptr, self.osig.ptr, self.ovar.ptr, m, ld, g, D, nr, ld, refine, Z,
                                           resid, self.olat.ptr))
        c.check(lib.oisat_rows_dot(h, D, ld, nr, Z, ld, nr, m, small))                      # [d | F]^T [z_d | Y_F]
        G = c.download(small, (nr, nr), np.float64)
        est = drift_coefficients(G[1:, 1:], G[1:, 0], tol)
        beta = est["beta"]
        Dh = c.download(D, (nr, ld), np.float64)[:, :m]
        Zh = c.download(Z, (nr, ld), np.float64)[:, :m]
        zp = Zh[0] - beta @ Zh[1:]
        c.upload_into(self.z.ptr, zp, dtype=np.float64)
        c.upload_into(self._functional_buffer("drift_beta", 16 * 8).ptr, beta, dtype=np.float64)
        res = np.array(resid, dtype=np.float64).reshape(refine + 1, nr)
        self._drift = {"degree": deg, "beta": beta, "beta_cov": est["beta_cov"], "beta_se": est["beta_se"], "cond": est["cond"],
                       "resid": res[-1].copy(), "chi2": float((Dh[0] - beta @ Dh[1:]) @ zp), "logdet_M": est["logdet_M"]}
        return [float(v) for v in res[:, 0]]

    def drift_estimate(self):
        """What the last ``run(drift=degree)`` estimated: ``degree``, ``beta`` ((degree + 1)^2 coefficients in the order of
        ``oisat_drift_basis``), ``beta_cov`` = (F^T S^-1 F)^-1, ``beta_se``, ``cond`` (of the unit-diagonal F^T S^-1 F), ``resid``
        (relative residual of each column of the block solve, the innovation first) and ``chi2`` = (d - F beta)^T z'."""
        if self._drift is None:
            raise ValueError("drift_estimate() must follow run(drift=degree)")
        self.check()
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self._drift.items() if k != "logdet_M"}

    def drift_variance(self):
        """(ny, nx) float64: the variance that the unknown drift adds to the analysis error of every cell, q^T M^-1 q with
        q = f(x) - Q(x), Q[j] = B H^T Y_F[:, j] -- p float64 increments (``oisat_apply_increment_grid``) and one
        ``oisat_drift_quadform``.  Needs the block solve of the last ``run(drift=degree)``."""
        if self._drift is None:
            raise ValueError("drift_variance() must follow run(drift=degree)")
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        m, ld, g, n, deg = self.m, self.mp, self._g, self.n, self._drift["degree"]
        p = (deg + 1) ** 2
        Y = self._functional_buffer("drift", 0).at((p + 1) * ld * 8 + ld * 8)             # Y_F: behind z_d in the solution block
        Q = self._functional_buffer("drift_Q", (p + 1) * n * 8)                            # Q | the variance
        Mi = self._functional_buffer("drift_Minv", 16 * 16 * 8)
        c.upload_into(Mi.ptr, np.ascontiguousarray(self._drift["beta_cov"]), dtype=np.float64)
        c.check(lib.oisat_set_correlation(h, self._kind))       # (the model of the run that left the factor)
        f64 = _hip.dtype_code(np.dtype(np.float64))
        for j in range(p):
            c.check(lib.oisat_apply_increment_grid(h, f64, self.gxyz.ptr, self.gsig.ptr, self._ny, self._nx, self.oxyz.ptr, self.osig.ptr,
                                                   Y + j * ld * 8, m, g, None, None, Q.at(j * n * 8), self.glat.ptr, self.olat.ptr))
        c.check(lib.oisat_drift_quadform(h, self.gxyz.ptr, n, deg, Q.ptr, n, Mi.ptr, Q.at(p * n * 8)))
        self.check()
        return c.download(Q.at(p * n * 8), tuple(self.shape), np.float64)

    # ---- the innovations' likelihood and the error scales it supports
    def log_likelihood(self):
        """-2 ln p(d) of the innovations under S = H B H^T + R as the last ``run(check_pd=True, exact_factor=True)`` analysed them
        (anything else is a ``ValueError``: the narrower envelope's factor has the log-determinant of a truncated matrix).  One
        diagonal reduction over the factor (``oisat_factor_logdet``) and two dot products (``oisat_rows_dot``).  Returns ``m``,
        ``chi2`` (d^T S^-1 d from the refined z), ``chi2_per_obs``, ``logdet``, ``min_pivot`` (the factor's smallest diagonal
        entry), ``neg2_log_likelihood`` (m ln 2 pi + logdet + chi2) and ``dd`` (|d|^2).  The mean of the innovations is not
        estimated: a bias shows as chi2_per_obs > 1 -- unless the run was one with ``drift=degree``: ``chi2`` is then
        (d - F beta)^T z', the value with the drift removed, and three entries are added: ``p``, ``logdet_M`` = log det F^T S^-1 F
        and ``neg2_restricted_log_likelihood`` = (m - p) ln 2 pi + logdet + logdet_M + chi2.
        ``neg2_log_likelihood`` keeps its formula, m ln 2 pi + logdet + chi2, and is then the likelihood of d AT beta-hat (the
        profile over beta: the drift-removed chi2 under the unrestricted normalisation), not the restricted one."""
        if not self._lik_ready:
            raise ValueError("log_likelihood() must follow run(check_pd=True, exact_factor=True)")
        self.check()
        c, lib, h, m = self.ctx, self.ctx.lib, self.ctx.h, self.m
        out = self._functional_buffer("lik", 4 * 8)             # logdet | smallest pivot | d^T z | d^T d
        c.check(lib.oisat_factor_logdet(h, self.S.ptr, m, self.mp, out.at(0)))
        c.check(lib.oisat_rows_dot(h, self.d.ptr, m, 1, self.z.ptr, m, 1, m, out.at(16)))
        c.check(lib.oisat_rows_dot(h, self.d.ptr, m, 1, self.d.ptr, m, 1, m, out.at(24)))
        logdet, piv, chi2, dd = (float(v) for v in c.download(out.ptr, (4,), np.float64))
        if self._drift is not None:
            chi2 = self._drift["chi2"]
        lik = {"m": m, "chi2": chi2, "chi2_per_obs": chi2 / m, "logdet": logdet, "min_pivot": piv,
               "neg2_log_likelihood": m * float(np.log(2.0 * np.pi)) + logdet + chi2, "dd": dd}
        if self._drift is not None:
            p, ldm = int(self._drift["beta"].size), self._drift["logdet_M"]
            lik.update(p=p, logdet_M=ldm, neg2_restricted_log_likelihood=(m - p) * float(np.log(2.0 * np.pi)) + logdet + ldm + chi2)
        return lik

    def _likelihood_at(self, scale_b, scale_o, L_km, corr, refine, tol):
        """One evaluation of the search: the likelihood dict at these scales with the solve's reported relative residual
        beside it (``resid``), or None where the factorization met a non-positive pivot (``OISAT_ENOTPD``, or the status
        words') or the solve ended above its tolerance -- a worse scale, not an error.  The status words are read and cleared
        either way.  A time-out of the task graph or of a sweep says nothing about the scale: it raises ``OisatError``."""
        c = self.ctx
        self.set_error_scales(scale_b, scale_o)
        try:
            resid = self.run(L_km, refine=refine, check_pd=True, want_resid=True, tol=tol, corr=corr, fields=False, exact_factor=True)
        except _hip.OisatError as e:
            if e.code != _hip.ENOTPD:
                raise
            c.solve_status(clear=True)
            return None
        st = c.solve_status(clear=True)
        if st.dag_timeouts or st.trsv_timeouts:
            raise _hip.OisatError(f"fit_error_scales: {st.dag_timeouts} task-graph and {st.trsv_timeouts} triangular-solve time-out(s) "
                                  f"at scale_b = {scale_b:g}, scale_o = {scale_o:g}")
        if not st.clean:
            return None
        lik = self.log_likelihood()
        lik["resid"] = float(resid[-1])
        return lik if np.isfinite(lik["logdet"]) and np.isfinite(lik["chi2"]) and lik["chi2"] > 0.0 else None

    def fit_error_scales(self, L_km, corr="gaussian", mode="background", bounds=(1e-2, 1e2), npts=9, wtol=0.01, refine=2, tol=None,
                         want_se=True, fields=True):
        """Maximum-likelihood scales of the loaded error variances.  With P = H B H^T at the loaded
        scale and R = diag(So): ``mode="background"`` trusts R and minimises J_b(ln s) = log det(s P + R) + d^T (s P + R)^-1 d
        -> ``scale_b`` = s, ``scale_o`` = 1; ``mode="both"`` takes S = a (rho P + R), where a = chi2(rho) / m in closed form, and
        minimises the profile J_r(ln rho) = m ln(chi2(rho) / m) + log det(rho P + R) + m -> ``scale_o`` = a, ``scale_b`` = a rho
        (the gain depends on rho alone; a scales the reported errors).  ``profile_search`` over ``bounds`` (``npts``, ``wtol``);
        an evaluation is ``set_error_scales`` -> ``run(fields=False, exact_factor=True, check_pd=True)`` -> ``log_likelihood()``,
        a failed one counts as +inf.  ``want_se``: two more evaluations for ``se_ln = sqrt(2 / J'')`` (``profile_se``; in "both"
        mode that of ln rho).  Fewer than 32 observations, or no finite evaluation: ``found`` False, scales 1.  The call ends with
        ``set_error_scales`` at the result and a run there (``fields``: with the increment spread), so that ``download()``, the
        diagnostics and ``functional_covariance`` describe the ML analysis.  Returns ``mode``, ``scale_b``, ``scale_o``, ``ratio``
        (scale_b / scale_o), ``se_ln``, ``found``, ``at_bound``, ``nevals``, ``evaluations`` ((ln s, J) in order, those of the
        standard error included), ``residuals`` (per evaluation: the solve's reported relative residual, NaN where it failed) and
        ``likelihood`` (``log_likelihood()`` at the result)."""
        if mode not in FIT_SCALE_MODES:
            raise ValueError(f"mode must be one of {FIT_SCALE_MODES}, not {mode!r}")
        corr_kind(corr)
        m, both = self.m, mode == "both"
        out = {"mode": mode, "scale_b": 1.0, "scale_o": 1.0, "ratio": 1.0, "se_ln": float("inf"), "found": False, "at_bound": False,
               "nevals": 0, "evaluations": [], "residuals": []}
        liks, evals = {}, out["evaluations"]
        self.check()                                           # (an earlier unchecked run's failure is not this search's)

        def objective(x):
            lik = liks[x] = self._likelihood_at(float(np.exp(x)), 1.0, L_km, corr, refine, tol)
            J = float("inf")
            if lik is not None:
                J = m * float(np.log(lik["chi2"] / m)) + lik["logdet"] + m if both else lik["logdet"] + lik["chi2"]
            evals.append((float(x), J))
            out["residuals"].append(lik["resid"] if lik is not None else float("nan"))
            return J

        if m >= FIT_SCALE_MIN_OBS:
            res = profile_search(objective, bounds=bounds, npts=npts, wtol=wtol)
            if np.isfinite(res["J"]):
                x = res["x"]
                rho = float(np.exp(x))
                a = liks[x]["chi2"] / m if both else 1.0
                out.update(scale_b=a * rho, scale_o=a, ratio=rho, found=True, at_bound=res["at_bound"])
                if want_se:
                    out["se_ln"] = profile_se(objective, x, res["J"])
            out["nevals"] = len(evals)
        # the analysis at the result, checked as any other: a failure here raises
        self.set_error_scales(out["scale_b"], out["scale_o"])
        self.run(L_km, refine=refine, check_pd=True, tol=tol, corr=corr, fields=fields, exact_factor=True)
        out["likelihood"] = self.log_likelihood()
        return out

    # ---- outputs
    def check(self):
        """Wait for this handle's stream and raise ``OisatError`` if any solve enqueued on it since the last check met a
        non-positive pivot or a triangular-solve time-out (``run`` is asynchronous and unchecked by default)."""
        self.ctx.check_solves()

    def download(self):
        self.check()
        out = self.ctx.download(self.out_ptr, (2,) + tuple(self.shape), self.dt)
        return out[0], out[1]

    def download_z(self):
        self.check()
        return self._unsort(self.ctx.download(self.z.ptr, (self.m,), np.float64))

    def download_S(self):
        """S (after ``run``: its Cholesky factor), rows/columns in the device's ascending-latitude order (``self._order``)."""
        return self.ctx.download(self.S.ptr, (self.mp, self.mp), np.float32)

    @staticmethod
    def flops(m: int) -> float:
        """Algorithmic flops of the gain solve as BASELINE.md counts them: m^3/3 + 2 m^2."""
        return m ** 3 / 3.0 + 2.0 * m ** 2


def assemble_functional_covariance(prior, gy, ry, gg_diag, rr_diag, support=0):
    """The result of ``DenseAnalysis.functional_covariance`` from its (K, K) products, pure NumPy: ``prior`` = W T^T, ``gy`` =
    G^T Y, ``ry`` = R^T Y with y_k the computed solve of S y = g_k and r_k = g_k - S y_k, ``gg_diag`` / ``rr_diag`` = |g_k|^2 /
    |r_k|^2.  With y = S^-1 (g - r): G^T Y + R^T Y = G^T S^-1 G - R^T S^-1 R -- the reduction's error is second order in the
    residual, bounded by tol^2 cond(S) of the prior, and it can only make the reduction smaller, the variance larger.  (The plain
    G^T Y is G^T S^-1 G - G^T S^-1 R: first order, either sign.)  Everything is symmetrised."""
    prior, gy, ry = (np.asarray(a, dtype=np.float64) for a in (prior, gy, ry))
    prior = 0.5 * (prior + prior.T)
    red = gy + ry
    red = 0.5 * (red + red.T)
    gg, rr = np.asarray(gg_diag, dtype=np.float64), np.asarray(rr_diag, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        resid = np.where(gg > 0.0, np.sqrt(rr / gg), 0.0)
    return {"prior": prior, "reduction": red, "posterior": prior - red, "resid": resid, "support": int(support)}


def region_weights(labels, lat, valid=None, area_weighted=True):
    """Regional-mean functionals from a label map, pure NumPy.  ``labels``: (ny, nx) integers, values <= 0 = no region;
    ``lat``: (ny, nx) cell-centre latitudes in degrees; ``valid``: (ny, nx) bool, the cells that may carry weight (default:
    all).  Returns ``(ids, W)``: the sorted distinct positive labels and W (K, ny, nx) float64 with W[k] = cos(lat) over the
    valid cells of region ids[k] (1 with ``area_weighted=False``), normalised to sum 1.  More than 64 regions, or a region
    without a valid cell, is a ``ValueError`` that names the label."""
    labels = np.asarray(labels)
    lat = np.asarray(lat, dtype=np.float64)
    if labels.ndim != 2 or labels.shape != lat.shape:
        raise ValueError(f"labels must be a (ny, nx) map on the grid {lat.shape}, not {labels.shape}")
    if not np.issubdtype(labels.dtype, np.integer):
        if not np.all(np.isfinite(labels)) or np.any(labels != np.rint(labels)):
            raise ValueError("labels must hold integers")
        labels = labels.astype(np.int64)
    valid = np.ones(labels.shape, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    if valid.shape != labels.shape:
        raise ValueError(f"valid must have the labels' shape {labels.shape}, not {valid.shape}")
    ids = np.unique(labels[labels > 0])
    if ids.size > 64:
        raise ValueError(f"{ids.size} regions; at most 64 per call (label {int(ids[64])} is the 65th)")
    w = np.cos(np.deg2rad(lat)) if area_weighted else np.ones(lat.shape)
    W = np.zeros((ids.size,) + labels.shape)
    for k, r in enumerate(ids):
        wk = np.where((labels == r) & valid, w, 0.0)
        tot = wk.sum()
        if not tot > 0.0:
            raise ValueError(f"region {int(r)} has no valid cell")
        W[k] = wk / tot
    return ids, W


def _region_info(ids, W, Xa, xa_an, fc):
    """``info["regions"]`` of ``OI_dense`` from the functionals' covariances and the two fields."""
    Wf = W.reshape(W.shape[0], -1)
    xb64 = np.ravel(np.asarray(Xa, dtype=np.float64))
    ok = np.isfinite(xb64)
    xa64 = np.ravel(np.asarray(xa_an, dtype=np.float64))
    return {"ids": ids, "background_mean": Wf[:, ok] @ xb64[ok], "analysis_mean": Wf[:, ok] @ xa64[ok],
            "prior_sd": np.sqrt(np.maximum(np.diag(fc["prior"]), 0.0)), "posterior_sd": np.sqrt(np.maximum(np.diag(fc["posterior"]), 0.0)),
            "prior_cov": fc["prior"], "posterior_cov": fc["posterior"], "resid": fc["resid"]}


def tile_partition(lat2, lon2, obs_lat, obs_lon, tile_deg=30.0, halo_km=900.0, merge_polar=True):
    """Localised block-B (BASELINE config 3): cut a regular lat/lon grid into tile_deg x tile_deg tiles;
    a tile is analysed with every observation inside the tile or within ``halo_km`` of it (3 L is the
    usual choice: exp(-9/2) = 1 % correlation left).  Returns a list of dicts with the tile's grid
    slices and the indices of its observations.  Longitude wraps; bands whose halo reaches a pole take
    every longitude -- all tiles of such a band then share ONE observation set, i.e. one and the same system
    (H B H^T + R) z = d, so with ``merge_polar`` (default) the band is kept as a single polar-cap tile (all
    longitudes) and that system is built, factored and solved once instead of once per 30 deg of longitude
    (12 times at tile_deg = 30: 87 % of the factorization flops of a 720x1440 / 1e5-observation month)."""
    lat2 = np.asarray(lat2)
    lon2 = np.asarray(lon2)
    ny, nx = lat2.shape
    latc, lonc = lat2[:, 0], lon2[0, :]
    dlat, dlon = abs(latc[1] - latc[0]), abs(lonc[1] - lonc[0])
    ty, tx = max(1, int(round(tile_deg / dlat))), max(1, int(round(tile_deg / dlon)))
    h_lat = np.rad2deg(halo_km / EARTH_RADIUS_KM)
    olat, olon = np.ravel(obs_lat), np.ravel(obs_lon)
    tiles = []
    for y0 in range(0, ny, ty):
        y1 = min(y0 + ty, ny)
        la0, la1 = latc[y0] - dlat / 2, latc[y1 - 1] + dlat / 2
        in_lat = (olat >= la0 - h_lat) & (olat <= la1 + h_lat)
        worst = max(abs(la0 - h_lat), abs(la1 + h_lat))
        polar = worst >= 89.0
        h_lon = 360.0 if polar else h_lat / np.cos(np.deg2rad(worst))
        if polar and merge_polar:
            tiles.append({"rows": (y0, y1), "cols": (0, nx), "obs": np.flatnonzero(in_lat)})
            continue
        for x0 in range(0, nx, tx):
            x1 = min(x0 + tx, nx)
            lo0, lo1 = lonc[x0] - dlon / 2, lonc[x1 - 1] + dlon / 2
            mid, half = 0.5 * (lo0 + lo1), 0.5 * (lo1 - lo0) + h_lon
            dl = np.abs((olon - mid + 180.0) % 360.0 - 180.0)
            sel = np.flatnonzero(in_lat & (dl <= half))
            tiles.append({"rows": (y0, y1), "cols": (x0, x1), "obs": sel})
    return tiles


class BatchedFactor:
    """Lock-step factorization of many plans (``oisat_batch_potrf``): the plans are sorted by size and cut into groups of
    comparable block count (a group's smallest matrix has at least ``ratio`` of the blocks of its largest) -- in a
    720x1440 month: the 48 mid-latitude tiles (31-48 blocks) and the two polar caps (137 blocks).  The groups run side
    by side, one stream each, and each group's solves start when it is factored (``OISAT_BATCH_SCHEDULE``)."""

    def __init__(self, device: int, plans, ratio: float = 0.5):
        groups = []
        order = sorted((p for p in plans if p is not None), key=lambda p: -p.m)
        every = list(order)
        # Task-graph factorization (csrc/dense_dag.inc; OISAT_DAG=0 turns it off): ONE persistent launch factors systems of
        # any mix of sizes -- tiles and polar caps together, the systems entering the launch in waves, every system's chain on
        # a workgroup of its own, the tile tasks drawn from one list -- so a batch of up to 1024 systems is ONE group (larger
        # ones keep the lock-step recursion, and so does a batch whose chains would crowd the handle's CUs: the library
        # decides, oisat_batch_is_task_graph tells).  Measured against the two lock-step groups
        # of the recursion: a month's 50 systems 62 vs 66 ms, a rank's 75 / 150 / 300 units of config 4 0.091 / 0.177 / 0.352 vs
        # 0.103 / 0.185 / 0.357 s, all 600 units 0.700 vs 0.706 s (what the one launch gains its fully exposed solve phase
        # costs).  Several launches side by side are what must be avoided: every launch's chains are resident and its tile
        # tasks starve (seven launches of 96: 1.03 s).
        self.dag = os.environ.get("OISAT_DAG", "-1") != "0" and bool(order) and len(order) <= 1024
        if self.dag:
            groups = [order]
            order = []
        cur = []
        for p in order:
            if cur and p.mp < ratio * cur[0].mp:
                groups.append(cur)
                cur = []
            cur.append(p)
        if cur:
            groups.append(cur)
        # the lock-step recursion (OISAT_DAG=0, or more than 1024 systems) enqueues the group with the longest dependent chain
        # first: in a 720x1440 month the two polar caps (137 diagonal blocks each) are the critical path.  Whatever the order, a
        # group's solves are released when THAT group is factored.  The gain solves and increments of a group run in lock-step on
        # the group's stream right behind its factorization (oisat_batch_solve) when every plan owns its work vectors
        self.batched_solve = all(p.work is not None for p in every)
        # ... or, with the task graph, as tasks of the factorization's own launch (oisat_batch_analyse, OISAT_DAG_SOLVE=1): the
        # same bits in one launch instead of ~15.  Not the default: it ties for one month (61.5-63 vs 62.6 ms) and loses for
        # twelve (0.73 vs 0.71 s) -- the launch is bound by workgroup-slot time, and fp64 VALU work does not overlap with the
        # MFMA K-loop on this chip (csrc/dense_dag.inc "WHAT IT BOUGHT").  The tests run both and compare them bit for bit.
        self.one_launch = self.dag and self.batched_solve and os.environ.get("OISAT_DAG_SOLVE", "0") == "1"
        self.groups = groups
        # schedule (OISAT_BATCH_SCHEDULE): "overlap" (default) -- one stream per group, all groups side by side;
        # "sequential" -- the groups one after the other (each one's dependent chain then runs at its isolated speed and
        # its solves go underneath the next group's factorization).  Same fields either way (tested).
        self.schedule = os.environ.get("OISAT_BATCH_SCHEDULE", "overlap")
        self.ctxs = [_hip.Context(device).own_stream() for _ in self.groups]
        # sharing (oisat_set_share): the group with the longest chain is the critical path of the whole batch -- its waves
        # get priority on the SIMDs they share with the other groups' GEMMs (measured: profiles/EXPERIMENTS.md, round 3)
        if len(self.groups) > 1:
            major = max(range(len(self.groups)), key=lambda gi: self.groups[gi][0].mp)
            for gi, ctx in enumerate(self.ctxs):
                ctx.check(ctx.lib.oisat_set_share(ctx.h, 3 if gi == major else 0, 2))
        self.ids = []
        for g, ctx in zip(self.groups, self.ctxs):
            n = len(g)
            ctx.check(ctx.lib.oisat_set_task_graph(ctx.h, -1 if self.dag else 0))
            Sp = (C.c_void_p * n)(*[p.S.ptr for p in g])
            Tp = (C.c_void_p * n)(*[p.tinv.ptr for p in g])
            mm = (C.c_int64 * n)(*[p.m for p in g])
            ld = (C.c_int64 * n)(*[p.mp for p in g])
            bid = C.c_int(-1)
            ctx.check(ctx.lib.oisat_batch_create(ctx.h, n, Sp, mm, ld, Tp, C.byref(bid)))
            self.ids.append(bid.value)
            yes = C.c_int(0)
            ctx.check(ctx.lib.oisat_batch_is_task_graph(ctx.h, bid.value, C.byref(yes)))
            self.one_launch = self.one_launch and bool(yes.value)      # (the library may have kept the recursion: too many chains for the CUs)
            if self.batched_solve:                          # the solve phase in lock-step too: tell the batch where everything lives
                item = g[0].dt.itemsize
                arr = lambda vals: (C.c_void_p * n)(*vals)      # noqa: E731
                ctx.check(ctx.lib.oisat_batch_set_solve(
                    ctx.h, bid.value, n, arr([p.oxyz.ptr for p in g]), arr([p.osig.ptr for p in g]), arr([p.ovar.ptr for p in g]),
                    arr([p.d.ptr for p in g]), arr([p.olat.ptr for p in g]), arr([p.z.ptr for p in g]),
                    arr([p.work.ptr for p in g]), arr([p.state.ptr for p in g]), arr([p.gxyz.ptr for p in g]),
                    arr([p.gsig.ptr for p in g]), arr([p.glat.ptr for p in g]), (C.c_int64 * n)(*[p.n for p in g]),
                    arr([p.xb_ptr for p in g]), arr([p.out_ptr for p in g]), arr([p.out_ptr + p.n * item for p in g])))
                ctx.check(ctx.lib.oisat_batch_set_grid(ctx.h, bid.value, n, (C.c_int64 * n)(*[p._nx for p in g]),
                                                       arr([p.perm.ptr for p in g])))
        self.group_of = {id(p): gi for gi, g in enumerate(self.groups) for p in g}
        self._threads = None
        # measured, one box (1 month of 720x1440 / 1e5 obs; a rank's eighth of 12 months; all 12 months):
        # overlap 73.6 / 112 / 745 ms, sequential 77.0 / 119 / 746 ms

    def run(self, pool, per_lane_plans, refine, check_pd=False):
        """``per_lane_plans[li]``: the plans of lane li in run order, already BUILT (their S enqueued on the lane).

        Every group's factorization is enqueued at once; the HOST then waits for the groups in completion order
        and enqueues each group's solves on the lanes as it finishes -- it returns when the last group is factored and its
        solves are enqueued.  (A device-side wait would park a barrier packet at the head of every lane's hardware queue for
        the whole factorization, and the command processor polls parked queues at the expense of the running one:
        with 12 parked lanes every kernel of the dependent chain took 40-60 us longer in the rocprofv3 trace --
        potrf_diag 27 -> 64, the panel TRSM 17 -> 80 us -- a third of a polar cap's factorization time.)"""
        sequential = self.schedule == "sequential"

        def enqueue_group(gi):
            g, ctx, bid = self.groups[gi], self.ctxs[gi], self.ids[gi]
            ctx.bind_thread()
            for lane in {id(p.ctx): p.ctx for p in g}.values():
                ctx.wait_for(lane)                          # short: the builds are a few ms
            if sequential and gi > 0:
                ctx.wait_for(self.ctxs[gi - 1])             # one parked queue
            info = (C.c_int * 2)(0, -1)
            kind = g[0]._kind                               # (every plan was built by the same run: one model)
            ctx.check(ctx.lib.oisat_set_correlation(ctx.h, kind))
            if self.one_launch and kind == 0:               # (the one-launch analysis is Gaussian only: the two calls otherwise)
                # factorization, gain solves and increments of the whole group as tasks of ONE persistent launch: the solves of
                # the systems factored first run underneath the factorization of the others (csrc/dense_dag.inc)
                ctx.check(ctx.lib.oisat_set_refine_tol(ctx.h, REFINE_TOL))
                ctx.check(ctx.lib.oisat_batch_analyse(ctx.h, bid, g[0].code, g[0]._g, int(refine), info if check_pd else None))
                return
            ctx.check(ctx.lib.oisat_batch_potrf(ctx.h, bid, info if check_pd else None))
            if self.batched_solve:
                ctx.check(ctx.lib.oisat_set_refine_tol(ctx.h, REFINE_TOL))
                ctx.check(ctx.lib.oisat_batch_solve(ctx.h, bid, g[0].code, g[0]._g, int(refine)))

        # One enqueueing host thread per group: a polar-cap factorization is ~700 launches = 20-25 ms of host time inside
        # ONE library call, and a single thread enqueued the groups one after the other -- whichever group came second
        # started that much later (round 2: the caps at 10 ms behind the tiles; caps first: the tiles at 25 ms).
        if len(self.groups) > 1 and not sequential and not check_pd:
            if self._threads is None:
                from concurrent.futures import ThreadPoolExecutor
                self._threads = ThreadPoolExecutor(max_workers=len(self.groups), thread_name_prefix="oisat-group")
            futures = [self._threads.submit(enqueue_group, gi) for gi in range(len(self.groups))]
        else:
            futures = []
            for gi in range(len(self.groups)):
                enqueue_group(gi)
        if self.batched_solve:                              # nothing left for the lanes: wait for the enqueueing threads only
            for f in futures:
                f.exception()
            for f in futures:
                if f.exception() is not None:
                    raise f.exception()
            return
        # release each group's solves as soon as it is factored, in COMPLETION order: poll the group streams
        pending = list(range(len(self.ctxs)))
        while pending:
            done = [gi for gi in pending if (not futures or futures[gi].done()) and not self.ctxs[gi].busy()]
            if not done:
                time.sleep(2e-5)
                continue
            for gi in done:
                if futures and futures[gi].exception() is not None:
                    for f in futures:
                        f.exception()                       # let every enqueueing thread finish before raising
                    raise futures[gi].exception()
                pending.remove(gi)
                pool.enqueue([[(lambda p=p: p.run_solve(refine)) for p in plans if self.group_of[id(p)] == gi]
                              for plans in per_lane_plans])

    def fence(self, pool):
        """Order every lane behind whatever the group streams still have in flight (the lock-step solves of a previous,
        unchecked run read the buffers the next run's builds write).  Device-side, and free when the groups are idle."""
        for lane in pool.lanes:
            for ctx in self.ctxs:
                lane.wait_for(ctx)

    def check(self, what="batched factorization"):
        errors = []
        for ctx in self.ctxs:
            try:
                ctx.check_solves(what)
            except _hip.OisatError as e:
                errors.append(str(e))
        if errors:
            raise _hip.OisatError("; ".join(errors))

    def close(self):
        if self._threads is not None:
            self._threads.shutdown(wait=True)
            self._threads = None
        for ctx, bid in zip(self.ctxs, self.ids):
            if ctx.h is not None:
                ctx.lib.oisat_batch_destroy(ctx.h, bid)
                ctx.close()
        self.ctxs, self.ids = [], []


class SharedFactor:
    """The factor workspace of one lane: analyses that run back to back on a handle share it.  Grow-only; it may be
    re-allocated between (never during) runs, which is why plans hold this object and read ``.ptr`` at run time."""

    def __init__(self, lane):
        self.lane = lane
        self.buf = None
        self.nbytes = 0

    def reserve(self, max_obs: int):
        mp = -(-max(int(max_obs), 1) // NB) * NB
        need = mp * mp * 4
        if need > self.nbytes:
            if self.buf is not None:
                self.lane.sync()
                self.buf.free()
            self.buf = self.lane.alloc(need)
            self.nbytes = need
        return self

    @property
    def ptr(self):
        return self.buf.ptr


class LanePool:
    """Several handles on ONE device, each with its own stream, workspaces and shared factor buffer.  Tiles and
    months are independent, and a 4,000-8,000-observation solve leaves most of the 256 CUs idle on its own."""

    def __init__(self, ctx=None, streams: int = 12):
        self.ctx = ctx or _hip.context()
        self.lanes = [self.ctx] + [_hip.Context(self.ctx.device).own_stream() for _ in range(max(0, int(streams) - 1))]
        self.factors = [SharedFactor(lane) for lane in self.lanes]
        self._threads = None

    @classmethod
    def from_lanes(cls, lanes):
        """A pool over handles the caller already has (each with its own stream); ``close`` leaves them open."""
        self = cls.__new__(cls)
        self.ctx, self.lanes = lanes[0], list(lanes)
        self.factors = [SharedFactor(lane) for lane in self.lanes]
        self._threads = None
        self._borrowed = True
        return self

    def __len__(self):
        return len(self.lanes)

    def assign(self, weights):
        """Longest-processing-time-first: heaviest unit to the least loaded lane.  -> (lane of each unit, run order)."""
        order = sorted(range(len(weights)), key=lambda i: (-float(weights[i]), i))
        load = [0.0] * len(self.lanes)
        lane_of = [0] * len(weights)
        for i in order:
            li = min(range(len(load)), key=load.__getitem__)
            lane_of[i] = li
            load[li] += float(weights[i])
        return lane_of, order

    def sync(self):
        for lane in self.lanes:
            lane.sync()

    def enqueue(self, per_lane):
        """``per_lane[li]``: the callables (each enqueues one unit's kernels) of lane li, in run order.  One host thread
        per lane: a 6,000-observation tile is ~150 kernel launches and a month ~8,000, so a single enqueueing thread --
        ~10 us per launch -- is slower than the GPU (91 ms of launching for 30 ms of work at 720x1440 / 1e5 obs);
        ctypes releases the GIL inside the library calls, and each handle is driven by exactly one thread."""
        work = [(li, fns) for li, fns in enumerate(per_lane) if fns]
        if len(work) <= 1:
            for _, fns in work:
                for fn in fns:
                    fn()
            return
        if self._threads is None:
            from concurrent.futures import ThreadPoolExecutor
            self._threads = ThreadPoolExecutor(max_workers=len(self.lanes), thread_name_prefix="oisat-lane")

        def drive(li, fns):
            self.lanes[li].bind_thread()
            for fn in fns:
                fn()
        futures = [self._threads.submit(drive, li, fns) for li, fns in work]
        errors = [f.exception() for f in futures]        # waits for EVERY lane before anything is raised
        for e in errors:
            if e is not None:
                raise e

    def check(self, what="tiled analysis"):
        """Wait for every lane and read (and clear) every lane's solve status before raising, so that one failed unit
        is reported once and does not poison the next run."""
        errors = []
        for li, lane in enumerate(self.lanes):
            try:
                lane.check_solves(f"{what}, lane {li}")
            except _hip.OisatError as e:
                errors.append(str(e))
        if errors:
            raise _hip.OisatError("; ".join(errors))

    def close(self):
        if self._threads is not None:
            self._threads.shutdown(wait=True)
            self._threads = None
        for f in self.factors:
            if f.buf is not None:
                f.buf.free()
        if getattr(self, "_borrowed", False):
            return
        for lane in self.lanes[1:]:
            lane.close()


def _check_all(what, *checkers):
    """Run every status check (each waits for its streams and clears what it reports), then raise once."""
    errors = []
    for c in checkers:
        if c is None:
            continue
        try:
            c.check(what)
        except _hip.OisatError as e:
            errors.append(str(e))
    if errors:
        raise _hip.OisatError("; ".join(errors))


class TiledAnalysis:
    """Localised block-B analysis: one small dense analysis per tile (its own S = H B H^T + R over the
    tile's observations + halo).  Tiles are independent work units: inside one GPU they are dealt to the lanes of a
    ``LanePool`` (heaviest first, each lane one stream with ONE shared factor workspace); across GPUs
    ``parallel.shard_units`` spreads (month x tile) units -- ``only`` restricts this object to the tiles a rank owns."""

    def __init__(self, grid_lat, grid_lon, tile_deg=30.0, halo_km=900.0, dtype=np.float32, ctx=None, streams=12, pool=None,
                 merge_polar=True, batched=True):
        """``batched`` (default): every tile keeps its own S and all tiles are factored in lock-step by
        ``oisat_batch_potrf`` (one launch per recursion node for all tiles) between a per-lane build phase and a per-lane
        solve phase; ``batched=False``: each lane runs its tiles' whole pipelines back to back with one shared factor
        buffer (less memory: one S per lane instead of one per tile)."""
        self.merge_polar = bool(merge_polar)
        self.batched = bool(batched)
        self.factor = None
        self._own_pool = pool is None
        self.pool = pool or LanePool(ctx, streams)
        self.ctx = self.pool.ctx
        self.lanes = self.pool.lanes
        self.lat2, self.lon2 = np.asarray(grid_lat), np.asarray(grid_lon)
        self.tile_deg, self.halo_km = float(tile_deg), float(halo_km)
        self.dt = np.dtype(dtype)
        self.plans = []

    def prepare(self, Xa, Sa, obs_lat, obs_lon, obs_y, obs_var, scale=1.0, only=None):
        """Host side: cut the month into tiles, innovation against the GLOBAL background.  ``only``: the tile indices
        this object analyses (default all).  -> the live tile indices and their observation counts."""
        Xa = np.asarray(Xa, dtype=np.float64)
        sig = np.sqrt(float(scale) * np.asarray(Sa, dtype=np.float64))
        olat, olon = np.ravel(obs_lat), np.ravel(obs_lon)
        cell = regular_grid_cell(self.lat2, self.lon2, olat, olon)
        y = np.where(np.ravel(obs_y) < 0, 0.0, np.ravel(obs_y))
        self._host = dict(Xa=Xa, Sa=np.asarray(Sa), scale=float(scale), olat=olat, olon=olon, ovar=np.ravel(obs_var),
                          d=y - Xa.ravel()[cell], s=sig.ravel()[cell])
        self.tiles = tile_partition(self.lat2, self.lon2, olat, olon, self.tile_deg, self.halo_km, self.merge_polar)
        nx = self.lat2.shape[1]
        self._cell, self._Sa, self._scale = cell, np.asarray(Sa), float(scale)
        self._inside = [None] * len(self.tiles)
        for ti, t in enumerate(self.tiles):
            (y0, y1), (x0, x1) = t["rows"], t["cols"]
            c = cell[t["obs"]]
            self._inside[ti] = (c // nx >= y0) & (c // nx < y1) & (c % nx >= x0) & (c % nx < x1)
        keep = set(range(len(self.tiles))) if only is None else set(int(t) for t in only)
        self.live = [ti for ti, t in enumerate(self.tiles) if ti in keep and t["obs"].size]
        self._Xa = Xa
        self.n = int(Xa.size)
        self.flops = sum(DenseAnalysis.flops(int(self.tiles[ti]["obs"].size)) for ti in self.live)
        return self.live, [int(self.tiles[ti]["obs"].size) for ti in self.live]

    def build(self, lane_of=None, order=None, out_ptrs=None, group=True):
        """Device side: one plan per live tile on its lane.  ``lane_of`` / ``order``: per live tile (default: LPT by
        obs^3 over this object's tiles alone); ``out_ptrs``: per live tile, where its ``xa | inc`` go; ``group``: form
        this object's own ``BatchedFactor`` (False when a ``MonthTileBatch`` groups the plans of several months)."""
        h = self._host
        sizes = [int(self.tiles[ti]["obs"].size) for ti in self.live]
        if lane_of is None:
            # batched: the factorization is not a lane's job, what is left per tile grows like m^2 (solves) + n m
            lane_of, order = self.pool.assign([float(m) ** (2 if self.batched else 3) for m in sizes])
        if not self.batched:
            for k, m in enumerate(sizes):
                self.pool.factors[lane_of[k]].reserve(m)
        if self.factor is not None:                      # its group streams may still be working on the OLD plans' factors
            self.factor.close()
            self.factor = None
        self.plans = [None] * len(self.tiles)
        for k, ti in enumerate(self.live):
            t = self.tiles[ti]
            (y0, y1), (x0, x1) = t["rows"], t["cols"]
            li = lane_of[k]
            p = DenseAnalysis(self.lat2[y0:y1, x0:x1], self.lon2[y0:y1, x0:x1], max_obs=sizes[k], dtype=self.dt,
                              ctx=self.lanes[li], shared_S=None if self.batched else self.pool.factors[li],
                              out_ptr=None if out_ptrs is None else out_ptrs[k], batched=self.batched)
            p.load_background(h["Xa"][y0:y1, x0:x1], h["Sa"][y0:y1, x0:x1], scale=h["scale"])
            o = t["obs"]
            p.load_obs_direct(h["olat"][o], h["olon"][o], h["s"][o], h["ovar"][o], h["d"][o])
            self.plans[ti] = p
        self._order = [self.live[k] for k in (order if order is not None else range(len(self.live)))]
        self._lane_of = {ti: lane_of[k] for k, ti in enumerate(self.live)}
        self._host = None
        if self.batched and group and self.live:
            self.factor = BatchedFactor(self.ctx.device, [self.plans[ti] for ti in self.live])

    def load(self, Xa, Sa, obs_lat, obs_lon, obs_y, obs_var, scale=1.0, only=None):
        self.prepare(Xa, Sa, obs_lat, obs_lon, obs_y, obs_var, scale=scale, only=only)
        self.build()

    def _per_lane(self, fn):
        per_lane = [[] for _ in self.lanes]
        for ti in self._order:                           # run order (heaviest first) is kept inside every lane
            per_lane[self._lane_of[ti]].append(lambda p=self.plans[ti]: fn(p))
        return per_lane

    def enqueue(self, L_km, refine=2, check_pd=False, corr="gaussian"):
        corr_kind(corr)
        if not self._order:                              # not a single observation in any owned tile: x_a = x_b
            return
        if not self.batched:
            self.pool.enqueue(self._per_lane(lambda p: p.run(L_km, refine=refine, check_pd=check_pd, corr=corr)))
            return
        self.factor.fence(self.pool)
        self.pool.enqueue(self._per_lane(lambda p: p.run_build(L_km, corr=corr)))      # innovation, S = H B H^T + R
        plans = [[] for _ in self.lanes]
        for ti in self._order:
            plans[self._lane_of[ti]].append(self.plans[ti])
        self.factor.run(self.pool, plans, refine, check_pd=check_pd)            # lock-step factor | gain solve, increment

    def run(self, L_km, refine=2, check_pd=False, corr="gaussian"):
        """Enqueue every tile on its lane's stream (largest first), wait for all lanes and check their solve status:
        a non-positive pivot or a triangular-solve time-out in ANY tile raises ``OisatError``."""
        corr_kind(corr)
        self.ctx.sync()                                 # inputs uploaded on the default stream are complete
        self._L, self._refine, self._corr = float(L_km), int(refine), corr
        self.enqueue(L_km, refine=refine, check_pd=check_pd, corr=corr)
        _check_all("tiled analysis", self.pool, self.factor)

    def close(self):
        """Release the batch streams / tables and the lane pool (if this object made it)."""
        if self.factor is not None:
            self.factor.close()
            self.factor = None
        self.plans = []
        if self._own_pool:
            self.pool.close()

    def download(self):
        """(xa, inc) on the full grid; cells of tiles this object does not own keep the background / zero."""
        xa = self._Xa.astype(self.dt).copy()
        inc = np.zeros_like(xa)
        for t, p in zip(self.tiles, self.plans):
            if p is None:
                continue
            (y0, y1), (x0, x1) = t["rows"], t["cols"]
            a, b = p.download()
            xa[y0:y1, x0:x1] = a
            inc[y0:y1, x0:x1] = b
        return xa, inc

    def download_error(self, chunk_rows: int = 4096):
        """Posterior error sqrt(diag(B - B H^T S^-1 H B)) on the full grid and diag(K H) per cell (sum over the
        observations inside the cell; 0 where none), tile by tile from each tile's own factor.  A lane shares one
        factor buffer between its tiles, so every tile is re-run (check_pd) right before its diagnostics."""
        err = np.sqrt(self._scale * np.asarray(self._Sa, dtype=np.float64)).astype(np.float32)
        ak = np.zeros(self._Xa.size)
        for ti in self._order:
            t, p = self.tiles[ti], self.plans[ti]
            (y0, y1), (x0, x1) = t["rows"], t["cols"]
            if self.batched:                             # every tile still holds its own factor: adopt, do not redo
                p.ctx.check(p.ctx.lib.oisat_factor_adopt(p.ctx.h, p.S.ptr, p.m, p.mp, p.tinv.ptr))
            else:
                p.run(self._L, refine=self._refine, check_pd=True, corr=self._corr)
            err[y0:y1, x0:x1] = p.posterior_error(chunk_rows)
            a = p.gain_diag(chunk_rows)
            inside = self._inside[ti]                    # halo observations belong to another tile's cells
            np.add.at(ak, self._cell[t["obs"]][inside], a[inside])
        return err, ak.reshape(self._Xa.shape)


class MonthTileBatch:
    """BASELINE configs[3] -- several monthly analyses cut into (month x tile) work units -- as ONE GPU sees it: the
    units this rank owns, of whatever months, dealt to the lanes of one pool by a single LPT pass and run without any
    host synchronisation in between; every unit writes its ``xa | inc`` tile into one contiguous slab, which is what
    ``parallel`` gathers to rank 0 in a single message.  (Reference: one scheduler job per month,
    run/job_submitter_sbatch.py:45-68; months alone cap 8 GPUs at 12/2 = 6x, hence the finer unit.)"""

    def __init__(self, grid_lat, grid_lon, tile_deg=30.0, halo_km=900.0, dtype=np.float32, ctx=None, streams=12, batched=True):
        self.pool = LanePool(ctx, streams)
        self.batched = bool(batched)
        self.factor = None
        self.ctx = self.pool.ctx
        self.lat2, self.lon2 = np.asarray(grid_lat), np.asarray(grid_lon)
        self.tile_deg, self.halo_km, self.dt = float(tile_deg), float(halo_km), np.dtype(dtype)
        self.months = {}                                # key -> TiledAnalysis restricted to the owned tiles
        self.units = []                                 # (month key, tile index, nobs) in insertion order

    def add_month(self, key, Xa, Sa, obs_lat, obs_lon, obs_y, obs_var, scale=1.0, only=None):
        ta = TiledAnalysis(self.lat2, self.lon2, self.tile_deg, self.halo_km, self.dt, pool=self.pool, batched=self.batched)
        live, sizes = ta.prepare(Xa, Sa, obs_lat, obs_lon, obs_y, obs_var, scale=scale, only=only)
        self.months[key] = ta
        self.units += [(key, ti, m) for ti, m in zip(live, sizes)]

    def build(self, min_slab_elems: int = 0):
        item = self.dt.itemsize
        lane_of, order = self.pool.assign([float(m) ** (2 if self.batched else 3) for (_, _, m) in self.units])
        if not self.batched:
            for li, (_, _, m) in zip(lane_of, self.units):
                self.pool.factors[li].reserve(m)
        self.offsets, total = [], 0                      # element offset of each unit's xa|inc inside the slab
        for key, ti, _ in self.units:
            (y0, y1), (x0, x1) = self.months[key].tiles[ti]["rows"], self.months[key].tiles[ti]["cols"]
            self.offsets.append(total)
            total += 2 * (y1 - y0) * (x1 - x0)
        self.slab_elems = total
        self.slab = self.ctx.alloc(max(total, int(min_slab_elems), 1) * item).shared_with_other_streams()   # lanes write, RCCL reads
        self.ctx.check(self.ctx.lib.oisat_memset(self.ctx.h, self.slab.ptr, 0, self.slab.nbytes))
        k0 = 0
        for key, ta in self.months.items():              # units of one month are contiguous in self.units
            nk = len(ta.live)
            ta.build(lane_of=lane_of[k0:k0 + nk], order=None,
                     out_ptrs=[self.slab.at(self.offsets[k] * item) for k in range(k0, k0 + nk)], group=False)
            k0 += nk
        if self.batched and self.units:                  # one lock-step factorization over the units of ALL months
            self.factor = BatchedFactor(self.ctx.device, [self.months[key].plans[ti] for key, ti, _ in self.units])
        self._run_order = [self.units[i][:2] for i in order]
        self.flops = sum(ta.flops for ta in self.months.values())

    def run(self, L_km, refine=2, check_pd=False, wait=True, corr="gaussian"):
        corr_kind(corr)
        self.ctx.sync()
        def per_lane(fn):
            out = [[] for _ in self.pool.lanes]
            for key, ti in self._run_order:              # heaviest unit first, across months
                ta = self.months[key]
                out[ta._lane_of[ti]].append(lambda p=ta.plans[ti]: fn(p))
            return out
        if not self._run_order:                          # this rank owns no unit with observations
            pass
        elif self.batched:
            self.factor.fence(self.pool)
            self.pool.enqueue(per_lane(lambda p: p.run_build(L_km, corr=corr)))
            plans = [[] for _ in self.pool.lanes]
            for key, ti in self._run_order:
                ta = self.months[key]
                plans[ta._lane_of[ti]].append(ta.plans[ti])
            self.factor.run(self.pool, plans, refine, check_pd=check_pd)
        else:
            self.pool.enqueue(per_lane(lambda p: p.run(L_km, refine=refine, check_pd=check_pd, corr=corr)))
        if wait:
            self.check()

    def check(self):
        _check_all("month x tile batch", self.pool, self.factor)

    def unit_shape(self, k):
        key, ti, _ = self.units[k]
        (y0, y1), (x0, x1) = self.months[key].tiles[ti]["rows"], self.months[key].tiles[ti]["cols"]
        return (2, y1 - y0, x1 - x0)

    def download_slab(self):
        return self.ctx.download(self.slab.ptr, (self.slab_elems,), self.dt)

    def close(self):
        if self.factor is not None:
            self.factor.close()
            self.factor = None
        for ta in self.months.values():
            ta.plans = []
        self.pool.close()


def _ensemble_mask(ens, Xa):
    """``info["ensemble"]``: the deviations are NaN where the background is not finite, as ``xb`` is."""
    bad = ~np.isfinite(np.asarray(Xa))
    if bad.any() and ens["deviations"] is not None:
        ens["deviations"][:, bad] = np.nan
    return ens


def OI_dense(Xa, Y, Sa, So, lat, lon, L_km, scale=1.0, refine=2, obs=None, dtype=None, want_error=False, tol=None,
             corr="gaussian", nprobe=256, seed=0, superob=None, superob_rho=0.0, regions=None, likelihood=False, fit_scale=None,
             ensemble=None, ensemble_features=256, drift=None):
    """Dense-covariance analysis with the reference's gridded argument convention.

    ``Xa, Sa``: (ny, nx) background and its variance; ``Y, So``: (ny, nx) observations and their
    variance, NaN where unobserved (as ``oisatgmi.oi`` passes them, driver.py:110-111);
    ``lat, lon``: (ny, nx) cell centres; ``L_km``: correlation length.  ``obs`` (optional) replaces
    ``Y, So`` by scattered observations: dict(lat, lon, y, var).  ``corr``: ``"gaussian"`` (default), ``"gaspari_cohn"`` or ``"soar"``.
    Returns ``(Xb, increment, info)``; unlike the element-wise ``OI`` every cell is analysed
    (unobserved cells get the spread increment instead of NaN).
    ``want_error``: True = the exact ``err`` / ``ak`` / ``ak_obs`` (n m^2 flop); ``"mc"`` = their randomized estimates from
    ``nprobe`` probes (``DenseAnalysis.posterior_error_mc``) with ``err_se`` / ``ak_obs_se`` beside them and
    ``info["error_method"] = "mc"``.
    ``superob``: None (default) = every observation is a row of the system; a number = the observations are first merged into
    superobservations over boxes of that many degrees (``superob``) and the system has one row per
    non-empty box; ``"auto"`` / ``"auto:<max_obs>"`` = nothing is done while the observations number at most ``max_obs``
    (default 100 000), otherwise the smallest box of ``SUPEROB_LADDER`` that leaves at most ``max_obs``.  ``superob_rho``: the
    correlation the errors of one box's members share.  With superobservations ``info["cells"]`` and ``info["nobs"]`` stay the raw ones,
    ``info["z"]`` / ``["ak_obs"]`` / ``["ak_obs_se"]`` are per superobservation, ``info["superob"]`` tells what was merged and
    ``info["ak"]`` gives member cell a of superobservation s the share ``ak_obs[s] w_a / W_s``.
    ``regions``: an (ny, nx) integer label map (values <= 0: no region, at most 64 regions).  ``info["regions"]`` then holds, per
    region in the order of ``ids``, the area-weighted ``background_mean`` and ``analysis_mean`` over the cells with a finite
    background and the EXACT error of that mean before and after the analysis, ``prior_sd`` / ``posterior_sd``, with the full
    ``prior_cov`` / ``posterior_cov`` between the regions and the solves' ``resid`` (``DenseAnalysis.functional_covariance``;
    DESIGN.md section 4.2h).  The functionals are taken on whatever system the plan solved: ``obs=`` and ``superob=`` alike.
    ``likelihood=True``: the analysis factors inside the 2^-52 envelope (``run(exact_factor=True)``) and ``info["likelihood"]``
    holds ``DenseAnalysis.log_likelihood()``: chi2, chi2_per_obs, logdet, neg2_log_likelihood of the innovations under the
    analysis' own S.  ``fit_scale``: None (default) | ``"background"`` | ``"both"``: the error scales are
    first estimated by maximum likelihood on whatever system the plan holds -- with ``superob=`` the superobservations --
    (``DenseAnalysis.fit_error_scales`` -> ``info["scale_fit"]``), and the analysis, ``want_error`` and ``regions`` are then those
    of ``scale * scale_b`` and ``So * scale_o``: the very call ``OI_dense(..., scale=scale * scale_b, likelihood=True)`` (with
    ``So * scale_o`` under ``"both"``) would make, with ``info["likelihood"]`` at the optimum.  Without a usable observation
    ``scale_fit`` is ``{"found": False, "scale_b": 1.0, "scale_o": 1.0, ...}`` and ``likelihood`` is None.
    ``ensemble``: None (default) | K, a positive multiple of 32: ``info["ensemble"]`` holds K draws from the analysis' own error
    distribution N(0, A) as ``deviations`` (K, ny, nx), NaN where the background is not finite, with the ``err`` / ``err_se``
    they imply, from ``ensemble_features`` random features per member and the seed ``seed``
    (``DenseAnalysis.posterior_ensemble``; ``gaussian`` and ``soar`` only).  The ensemble is that of
    whatever system the plan solved -- ``obs=``, ``superob=`` and ``fit_scale=`` alike; without a usable observation the
    members are prior draws (``DenseAnalysis.prior_ensemble``).
    ``drift``: None (default) | a degree 0..3: a large-scale mean of the innovations -- the (degree + 1)^2 real harmonics up to
    that degree -- is estimated together with the analysis (universal kriging, ``DenseAnalysis.run(drift=...)``; DESIGN.md
    section 4.2k).  ``xb`` and ``inc`` then include the drift, ``info["drift"]`` is ``DenseAnalysis.drift_estimate()`` with
    ``found`` True, and with ``want_error`` ``info["drift"]["var"]`` is ``DenseAnalysis.drift_variance()`` and ``info["err"]`` is
    sqrt(err^2 + var).  The basis is evaluated where the plan's rows are: ``obs=`` and ``superob=`` alike (a superobservation is
    a point at its centroid).  Without a usable observation ``info["drift"]`` is ``{"degree": ..., "found": False}`` and the
    fields are untouched.  ``drift`` with ``fit_scale``, ``ensemble`` or ``regions`` is a ``ValueError`` (not combined yet).
    """
    corr_kind(corr)                                           # (ValueError before anything is touched)
    drift = drift_degree(drift)
    if drift is not None:
        for name, v in (("fit_scale", fit_scale), ("ensemble", ensemble), ("regions", regions)):
            if v is not None:
                raise ValueError(f"drift cannot be combined with {name} yet")
    if ensemble is not None:
        ens_K, ens_F = _ensemble_sizes(ensemble, ensemble_features)
        ensemble_draws(corr, L_km, [], ens_F, 0, seed)        # (gaspari_cohn: ValueError)
    if fit_scale is not None and fit_scale not in FIT_SCALE_MODES:
        raise ValueError(f"fit_scale is None, 'background' or 'both', got {fit_scale!r}")
    want_lik = bool(likelihood) or fit_scale is not None
    if regions is not None:                                   # (and so are a bad label map's)
        reg_ids, reg_W = region_weights(regions, lat, valid=np.isfinite(np.asarray(Xa)))
    mc = isinstance(want_error, str)
    if mc and want_error != "mc":
        raise ValueError(f"want_error is False, True or 'mc', got {want_error!r}")
    so_box, so_max = superob_setting(superob)
    superob_rho = _superob_rho(superob_rho)
    Xa = np.asarray(Xa)
    if obs is None:
        Y[Y < 0] = 0.0                                        # same clamp as optimal_interpolation.py:14
        ok = np.isfinite(np.ravel(Y)) & np.isfinite(np.ravel(So)) & np.isfinite(np.ravel(Xa)) & np.isfinite(np.ravel(Sa))
        cell = np.flatnonzero(ok)
        olat, olon = np.ravel(lat)[cell], np.ravel(lon)[cell]
        oy, ovar = np.ravel(Y)[cell], np.ravel(So)[cell]
    else:
        olat, olon = np.ravel(obs["lat"]), np.ravel(obs["lon"])
        oy = np.where(np.ravel(obs["y"]) < 0, 0.0, np.ravel(obs["y"]))
        ovar = np.ravel(obs["var"])
        cell = regular_grid_cell(lat, lon, olat, olon)
    dt = np.dtype(dtype) if dtype is not None else _hip.compute_dtype(Xa)
    xa_f = np.where(np.isfinite(Xa), Xa, 0.0)
    sa_f = np.where(np.isfinite(Sa), Sa, 0.0)
    so = None

    def merge(scale, ovar):
        """The superobservations at this scale and these observation variances, and what ``info["superob"]`` says of them."""
        # innovations as the plain path forms them (oisat_innovation: y - x_b[cell] with x_b in the field dtype) and sigma_b
        # as load_obs takes it (sqrt(scale Sa) of the cell)
        nonlocal so_box
        d_raw = np.asarray(oy, dtype=np.float64) - np.ravel(xa_f).astype(dt).astype(np.float64)[cell]
        sig_raw = np.sqrt(float(scale) * np.ravel(np.asarray(sa_f, dtype=np.float64)))[cell]
        if so_box == "auto":
            so_box = superob_auto_box(olat, olon, d_raw, sig_raw, ovar, so_max)
        so = _superob_fn(olat, olon, d_raw, sig_raw, ovar, so_box, rho=superob_rho)
        return so, {"box_deg": so["box_deg"], "rho": so["rho"], "nobs_raw": so["nobs_raw"], "nobs": so["nobs"],
                    "count": so["count"], "spread": so["spread"], "index": so["index"]}

    if so_box is not None and not (so_box == "auto" and cell.size <= so_max):
        so, so_info = merge(scale, ovar)
    if cell.size == 0 or (so is not None and so["nobs"] == 0):
        # a month without a single usable observation: nothing to spread, x_a = x_b
        _hip.context()                 # (still no CPU path: fail here if the library or the GPU is missing)
        extra = {}
        if want_error:
            extra = {"ak": np.full(np.shape(Xa), np.nan), "err": np.sqrt(np.asarray(Sa, dtype=np.float64) * scale),
                     "ak_obs": np.empty(0)}
            if mc:
                extra.update(err=extra["err"].astype(np.float32), err_se=np.zeros(np.shape(Xa)), ak_obs_se=np.empty(0),
                             error_method="mc", nprobe=int(nprobe))
        if so is not None:
            extra["superob"] = so_info
        if want_lik:
            extra["likelihood"] = None
        if drift is not None:
            extra["drift"] = {"degree": drift, "found": False}
        if fit_scale is not None:
            extra["scale_fit"] = {"mode": fit_scale, "scale_b": 1.0, "scale_o": 1.0, "ratio": 1.0, "se_ln": float("inf"), "found": False,
                                  "at_bound": False, "nevals": 0, "evaluations": [], "residuals": [], "likelihood": None}
        if regions is not None:        # nothing observed: the error of a regional mean stays the background's
            plan = DenseAnalysis(lat, lon, max_obs=1, dtype=dt)
            plan.load_background(xa_f, sa_f, scale=scale)
            prior = plan.functional_prior(reg_W, L_km=L_km, corr=corr)
            fc = {"prior": prior, "posterior": prior.copy(), "resid": np.zeros(len(reg_ids))}
            extra["regions"] = _region_info(reg_ids, reg_W, Xa, xa_f, fc)
        if ensemble is not None:       # nothing observed: the members are prior draws
            plan = DenseAnalysis(lat, lon, max_obs=1, dtype=dt)
            plan.load_background(xa_f, sa_f, scale=scale)
            extra["ensemble"] = _ensemble_mask(plan.prior_ensemble(L_km, corr=corr, nmember=ens_K, nfeature=ens_F, seed=seed), Xa)
        return (np.array(Xa, dtype=dt), np.zeros(np.shape(Xa), dtype=dt),
                {"nobs": 0, "residuals": [], "cells": cell, "z": np.empty(0), **extra})
    plan = DenseAnalysis(lat, lon, max_obs=int(cell.size if so is None else so["nobs"]), dtype=dt,
                         diag_chunk_rows=4096 if want_error and not mc else 0)

    def load():
        plan.load_background(xa_f, sa_f, scale=scale)
        if so is None:
            plan.load_obs(olat, olon, cell, oy, ovar)
        else:                          # one row per superobservation: a point observation at the members' weighted centroid
            plan.load_obs_direct(so["lat"], so["lon"], so["sigma_b"], so["var"], so["d"])

    load()
    extra = {}
    if fit_scale is not None:
        # the search runs on the plan as loaded; the analysis at its result is then loaded the way a caller who passes
        # scale * scale_b (and So * scale_o) would load it, so that the two agree to the bit
        fit = extra["scale_fit"] = plan.fit_error_scales(L_km, corr=corr, mode=fit_scale, refine=refine, tol=tol, fields=False)
        if fit["found"]:
            scale = float(scale) * fit["scale_b"]
            if fit["scale_o"] != 1.0:
                ovar = np.asarray(ovar, dtype=np.float64) * fit["scale_o"]
            if so is not None:
                so, so_info = merge(scale, ovar)
                if so["nobs"] != plan.m:
                    raise RuntimeError("the superobservations changed with the error scales")
            load()
    if drift is None:
        resid = plan.run(L_km, refine=refine, check_pd=True, want_resid=True, tol=tol, corr=corr, exact_factor=want_lik)
    else:
        resid = plan.run(L_km, refine=refine, check_pd=True, want_resid=True, tol=tol, corr=corr, exact_factor=want_lik, drift=drift)
        extra["drift"] = {**plan.drift_estimate(), "found": True}
    xb, inc = plan.download()
    if want_lik:
        extra["likelihood"] = plan.log_likelihood()
    if want_error:                     # the other two members of OI's 4-tuple: averaging kernel and sqrt(Sb)
        # diag(K H) at a cell = sum over the observations INSIDE that cell of diag(H K) at the observation
        # ((B H^T S^-1)[cell(a), a] = (H B H^T S^-1)[a, a]); with one observation per cell -- the reference's
        # case -- this is AK of optimal_interpolation.py:31.  np.add.at: deterministic for repeated cells.
        est = plan.posterior_error_mc(nprobe=nprobe, seed=seed, gridded=obs is None and so is None) if mc else None
        ak_obs = est["ak_obs"] if mc else plan.gain_diag()
        ak_sum = np.zeros(Xa.size)
        if so is None:
            np.add.at(ak_sum, cell, ak_obs)
        else:                          # the share rule: member a of superobservation s carries ak_obs[s] w_a / W_s
            mem = so["index"] >= 0
            si = so["index"][mem]
            np.add.at(ak_sum, cell[mem], ak_obs[si] * (1.0 / np.asarray(ovar, dtype=np.float64)[mem]) / so["W"][si])
        ak = np.full(Xa.size, np.nan)
        ak[cell] = ak_sum[cell]
        extra.update(ak=ak.reshape(np.shape(Xa)), err=est["err"] if mc else plan.posterior_error(), ak_obs=ak_obs)
        if mc:
            extra.update(err_se=est["err_se"], ak_obs_se=est["ak_obs_se"], error_method="mc", nprobe=est["nprobe"])
        if drift is not None:          # the unknown drift's share of the analysis error
            var = extra["drift"]["var"] = plan.drift_variance()
            err = np.asarray(extra["err"])
            extra["err"] = np.sqrt(err.astype(np.float64) ** 2 + var).astype(err.dtype)
    if regions is not None:
        extra["regions"] = _region_info(reg_ids, reg_W, Xa, xb, plan.functional_covariance(reg_W, refine=refine, tol=tol))
    if ensemble is not None:
        extra["ensemble"] = _ensemble_mask(plan.posterior_ensemble(nmember=ens_K, nfeature=ens_F, seed=seed), Xa)
    bad = ~np.isfinite(Xa)
    if bad.any():
        xb = xb.copy()
        xb[bad] = np.nan
    if so is not None:
        extra["superob"] = so_info
    return xb, inc, {"nobs": int(cell.size), "residuals": resid, "cells": cell, "z": plan.download_z(), **extra}


def OI_tiled(Xa, Y, Sa, So, lat, lon, L_km, tile_deg=30.0, halo_km=None, scale=1.0, refine=2, dtype=None, want_error=False,
             streams=12, corr="gaussian"):
    """Localised block-B analysis with the reference's gridded argument convention (see ``OI_dense``): the grid is cut
    into ``tile_deg`` tiles, each analysed with the observations inside it or within ``halo_km`` (default: 3 L for the
    Gaussian; the support 2 c = 3.6515 L for ``corr="gaspari_cohn"``, where the halo is then a true boundary; 6.5172 L for
    ``corr="soar"``: ``SOAR_HALO_PER_L``, where SOAR has the Gaussian's value at 3 L).
    Returns ``(Xb, increment, info)``; ``info`` carries ``ak`` / ``err`` when ``want_error``."""
    kind = corr_kind(corr)                                    # (ValueError before anything is touched)
    Xa = np.asarray(Xa)
    Y[Y < 0] = 0.0                                            # same clamp as optimal_interpolation.py:14
    ok = np.isfinite(np.ravel(Y)) & np.isfinite(np.ravel(So)) & np.isfinite(np.ravel(Xa)) & np.isfinite(np.ravel(Sa))
    cell = np.flatnonzero(ok)
    dt = np.dtype(dtype) if dtype is not None else _hip.compute_dtype(Xa)
    if cell.size == 0:
        return OI_dense(Xa, Y, Sa, So, lat, lon, L_km, scale=scale, dtype=dt, want_error=want_error, corr=corr)
    xa_f = np.where(np.isfinite(Xa), Xa, 0.0)
    sa_f = np.where(np.isfinite(Sa), Sa, 0.0)
    if halo_km is None:
        halo_km = {CORRELATIONS["gaspari_cohn"]: GC_SUPPORT_PER_L, CORRELATIONS["soar"]: SOAR_HALO_PER_L}.get(kind, 3.0) * float(L_km)
    ta = TiledAnalysis(lat, lon, tile_deg=tile_deg, halo_km=halo_km, dtype=dt, streams=streams)
    try:
        ta.load(xa_f, sa_f, np.ravel(lat)[cell], np.ravel(lon)[cell], np.ravel(Y)[cell], np.ravel(So)[cell], scale=scale)
        ta.run(L_km, refine=refine, check_pd=True, corr=corr)
        xb, inc = ta.download()
        extra = {}
        if want_error:
            err, ak = ta.download_error()
            akf = np.full(Xa.size, np.nan)
            akf[cell] = ak.ravel()[cell]
            extra = {"ak": akf.reshape(np.shape(Xa)), "err": err}
    finally:
        ta.close()
    bad = ~np.isfinite(Xa)
    if bad.any():
        xb = xb.copy()
        xb[bad] = np.nan
    return xb, inc, {"nobs": int(cell.size), "cells": cell, "tiles": len(ta.tiles), **extra}


# ---- the correlation length from the data: the innovations' covariogram (Hollingsworth-Loennberg) ----
COVARIOGRAM_MAX_OBS = 1 << 20                        # include/oisat.h: oisat_covariogram


def covariogram_quantum(umax: float, m: int):
    """``(q_prod, q_chord)``: the fixed-point quanta of ``oisat_covariogram`` for ``m`` observations whose largest finite
    ``|u|`` is ``umax`` (host only; ``OisatError`` outside the library's range)."""
    lib = _hip.load_library()
    qp, qc = C.c_double(0.0), C.c_double(0.0)
    rc = lib.oisat_covariogram_quantum(float(umax), int(m), C.byref(qp), C.byref(qc))
    if rc != 0:
        raise _hip.OisatError(f"liboisat_hip error {rc}: {lib.oisat_last_error().decode()}")
    return qp.value, qc.value


def innovation_covariogram(obs_lat, obs_lon, innovation, sigma=None, max_km=2000.0, nbins=64, ctx=None):
    """Binned products of normalised innovations ``u = innovation / sigma`` (``sigma=None``: ``u = innovation``) over all pairs of
    observations up to ``max_km`` apart, ``nbins`` equal bins of the CHORD ``r / R_earth`` (the distance the library's ``g`` is
    defined on), on the device (``oisat_covariogram``: exact integer sums, bitwise repeatable).  An observation whose ``u`` is
    not finite takes part in nothing.  -> dict: ``chord`` (per-bin mean chord, NaN where ``count == 0``), ``r_km`` (``R_earth``
    times it), ``cov`` (mean of ``u_a u_b``), ``count``, ``nobs`` (observations used), ``var0`` (mean of ``u^2`` over them),
    ``q_prod`` / ``q_chord`` (the quanta: ``|sum - exact| <= count q / 2``), ``max_km``, ``nbins``."""
    c = ctx or _hip.context()
    lat = np.ravel(np.asarray(obs_lat, dtype=np.float64))
    lon = np.ravel(np.asarray(obs_lon, dtype=np.float64))
    d = np.ravel(np.asarray(innovation, dtype=np.float64))
    m, nbins = int(d.size), int(nbins)
    if lat.size != m or lon.size != m:
        raise ValueError("obs_lat, obs_lon and innovation must have the same size")
    with np.errstate(divide="ignore"):                        # (sigma = 0: w = inf, u not finite, the observation is dropped)
        w = None if sigma is None else 1.0 / np.broadcast_to(np.asarray(sigma, dtype=np.float64), np.shape(innovation)).ravel()
    o = latitude_order(lat)
    count = np.zeros(max(nbins, 0), dtype=np.int64)
    sp, sc = np.zeros(max(nbins, 0)), np.zeros(max(nbins, 0))
    used = C.c_int64(0)
    bufs = []
    if m:
        bufs = [c.upload(unit_vectors(lat[o], lon[o])), c.upload(d[o]), c.upload(lat[o])] + ([c.upload(w[o])] if w is not None else [])
    ptr = [b.ptr for b in bufs] + [None] * 4
    try:
        c.check(c.lib.oisat_covariogram(c.h, ptr[0], ptr[1], ptr[3], m, float(max_km) / EARTH_RADIUS_KM, nbins, ptr[2],
                                        count.ctypes.data, sp.ctypes.data, sc.ctypes.data, C.byref(used)))
    finally:
        for b in bufs:
            b.free()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = d if w is None else d * w
        fin = np.isfinite(u)
        umax = float(np.abs(u[fin]).max()) if fin.any() else 0.0
        var0 = float(np.mean(u[fin] ** 2)) if fin.any() else float("nan")
        chord = np.where(count > 0, sc / np.maximum(count, 1), np.nan)
        cov = np.where(count > 0, sp / np.maximum(count, 1), np.nan)
    q_prod, q_chord = covariogram_quantum(umax, m)
    return {"chord": chord, "r_km": EARTH_RADIUS_KM * chord, "cov": cov, "count": count, "nobs": int(used.value), "var0": var0,
            "q_prod": q_prod, "q_chord": q_chord, "max_km": float(max_km), "nbins": nbins}


def _corr_at(kind: int, L_km: float, chord2: np.ndarray) -> np.ndarray:
    """C(chord; g(L)) by the library's float64 function (``oisat_corr_eval``, host only)."""
    lib = _hip.load_library()
    out = np.empty_like(chord2)
    rc = lib.oisat_corr_eval(kind, decay_constant(L_km), chord2.ctypes.data, chord2.size, out.ctypes.data)
    if rc != 0:
        raise _hip.OisatError(f"liboisat_hip error {rc}: {lib.oisat_last_error().decode()}")
    return out


def fit_correlation(cg, corr="gaussian", L_bounds=None, min_count=30):
    """Least-squares fit of ``s C(r; L)`` to a covariogram ``cg`` (``innovation_covariogram``), host only.  Over the bins with
    ``count >= min_count``: J(L) = sum n_k (cov_k - s(L) C(chord_k; g(L)))^2 with s(L) = sum n C cov / sum n C^2 in closed form,
    clamped at 0; 64 log-spaced L in ``L_bounds`` (default: one bin width .. ``max_km``), then a golden-section search on log L
    between the best point's neighbours until the bracket is below 1e-9.  -> dict ``L_km``, ``scale`` (s: the share of the
    innovations' normalised variance that is spatially correlated, i.e. the background's if the observation errors are not),
    ``rms`` (sqrt(J / sum n)), ``corr``, ``found`` (False: fewer than three usable bins, or s = 0 at the minimum), ``at_bound``
    (the minimum sits on an end of ``L_bounds``), ``nbins_used``.  ``corr`` may be a list of models: the dict of the one with the
    smallest ``rms`` among those found is returned, all of them under ``"all"``."""
    if not isinstance(corr, str):
        fits = {name: fit_correlation(cg, name, L_bounds, min_count) for name in corr}
        if not fits:
            raise ValueError("corr is an empty list")
        best = min(fits, key=lambda name: (not fits[name]["found"], fits[name]["rms"] if fits[name]["found"] else 0.0))
        return {**fits[best], "all": fits}
    kind = corr_kind(corr)
    count = np.asarray(cg["count"], dtype=np.float64)
    chord_all, cov_all = np.asarray(cg["chord"], dtype=np.float64), np.asarray(cg["cov"], dtype=np.float64)
    use = (count >= min_count) & np.isfinite(chord_all) & np.isfinite(cov_all)
    n, cov = count[use], cov_all[use]
    chord2 = np.ascontiguousarray(chord_all[use] ** 2)
    if L_bounds is None:
        max_km = float(cg["max_km"]) if "max_km" in cg else float(np.nanmax(cg["r_km"]))
        L_bounds = (max_km / max(int(np.size(count)), 1), max_km)
    lo, hi = float(L_bounds[0]), float(L_bounds[1])
    if not (0.0 < lo < hi and np.isfinite(hi)):
        raise ValueError(f"L_bounds must be 0 < low < high, not {L_bounds!r}")
    out = {"L_km": float("nan"), "scale": 0.0, "rms": float("nan"), "corr": corr, "found": False, "at_bound": False,
           "nbins_used": int(n.size)}
    if n.size < 3:
        return out

    def s_and_J(logL):
        Cm = _corr_at(kind, float(np.exp(logL)), chord2)
        den = float(np.sum(n * Cm * Cm))
        s = max(float(np.sum(n * Cm * cov)) / den, 0.0) if den > 0.0 else 0.0
        r = cov - s * Cm
        return s, float(np.sum(n * r * r))

    grid = np.linspace(np.log(lo), np.log(hi), 64)
    Jg = [s_and_J(x)[1] for x in grid]
    i = int(np.argmin(Jg))
    a, b = grid[max(i - 1, 0)], grid[min(i + 1, 63)]
    inv_phi = 0.5 * (5.0 ** 0.5 - 1.0)
    x1, x2 = b - inv_phi * (b - a), a + inv_phi * (b - a)
    J1, J2 = s_and_J(x1)[1], s_and_J(x2)[1]
    while b - a > 1e-9:                                       # (on log L: 1e-9 relative in L)
        if J1 <= J2:
            b, x2, J2 = x2, x1, J1
            x1 = b - inv_phi * (b - a)
            J1 = s_and_J(x1)[1]
        else:
            a, x1, J1 = x1, x2, J2
            x2 = a + inv_phi * (b - a)
            J2 = s_and_J(x2)[1]
    x = 0.5 * (a + b)
    s, J = s_and_J(x)
    for xe in (grid[0], grid[-1]):                            # an end of the bounds that is no worse: the minimum is there
        se, Je = s_and_J(xe)
        if Je <= J:
            x, s, J = xe, se, Je
    L = float(np.exp(x))
    out.update(L_km=L, scale=s, rms=float(np.sqrt(J / np.sum(n))), found=bool(s > 0.0),
               at_bound=bool(abs(x - grid[0]) <= 1e-6 or abs(x - grid[-1]) <= 1e-6))
    return out


# ---- maximum-likelihood error scales: the one-dimensional search -----------------------------------
FIT_SCALE_MODES = ("background", "both")
FIT_SCALE_MIN_OBS = 32                               # fewer observations: no fit is made
PROFILE_SE_STEP = 0.25                               # the second difference of the profile is taken at ln s +- this


def profile_search(objective, bounds=(1e-2, 1e2), npts=9, wtol=0.01, max_evals=32):
    """Minimise ``objective(ln s)`` over ``bounds`` on s, host only: ``npts`` log-spaced points, then a golden-section search on
    ln s between the best point's neighbours until the bracket is below ``wtol`` (the scheme of ``fit_correlation``) or
    ``max_evals`` evaluations are spent.  An objective of +inf (a factorization that met a non-positive pivot, a solve that did
    not converge) is simply worse than any finite one.  -> dict ``x`` (ln of the minimiser: the best point EVALUATED, NaN if none
    was finite), ``J`` (the objective there), ``evaluations`` (every (ln s, J) in order), ``nevals`` and ``at_bound`` (the minimum
    is within ``wtol`` of an end of ``bounds``).  With the defaults: 21 to 23 evaluations."""
    lo, hi = float(bounds[0]), float(bounds[1])
    if not (0.0 < lo < hi and np.isfinite(hi)):
        raise ValueError(f"bounds must be 0 < low < high, not {bounds!r}")
    npts, max_evals = int(npts), int(max_evals)
    if npts < 3 or max_evals < npts + 2 or not wtol > 0.0:
        raise ValueError(f"profile_search needs npts >= 3, max_evals >= npts + 2 and wtol > 0, not {npts}, {max_evals}, {wtol!r}")
    evals = []

    def J_at(x):
        J = float(objective(float(x)))
        evals.append((float(x), J if J == J else float("inf")))         # (a NaN counts as a failed evaluation)
        return evals[-1][1]

    grid = np.linspace(np.log(lo), np.log(hi), npts)
    Jg = [J_at(x) for x in grid]
    i = int(np.argmin(Jg))
    a, b = float(grid[max(i - 1, 0)]), float(grid[min(i + 1, npts - 1)])
    inv_phi = 0.5 * (5.0 ** 0.5 - 1.0)
    x1, x2 = b - inv_phi * (b - a), a + inv_phi * (b - a)
    J1, J2 = J_at(x1), J_at(x2)
    while b - a > wtol and len(evals) < max_evals:
        if J1 <= J2:
            b, x2, J2 = x2, x1, J1
            x1 = b - inv_phi * (b - a)
            J1 = J_at(x1)
        else:
            a, x1, J1 = x1, x2, J2
            x2 = a + inv_phi * (b - a)
            J2 = J_at(x2)
    x, J = min(evals, key=lambda e: e[1])
    if not np.isfinite(J):
        x = float("nan")
    return {"x": x, "J": J, "evaluations": evals, "nevals": len(evals),
            "at_bound": bool(abs(x - grid[0]) <= wtol or abs(x - grid[-1]) <= wtol)}


def profile_se(objective, x, Jx, h=PROFILE_SE_STEP):
    """Standard error of the minimiser ``x`` of a -2 ln likelihood profile: sqrt(2 / J'') with J'' the central second
    difference (J(x + h) - 2 J(x) + J(x - h)) / h^2, two more evaluations.  J'' <= 0, or a failed evaluation: +inf."""
    d2 = (float(objective(x + h)) - 2.0 * float(Jx) + float(objective(x - h))) / (h * h)
    return float(np.sqrt(2.0 / d2)) if np.isfinite(d2) and d2 > 0.0 else float("inf")


def estimate_corr_length(Xa, Y, Sa, So, lat, lon, scale=1.0, corr="gaussian", **kw):
    """The correlation length the month's own innovations support, with the gridded convention of ``OI_dense`` (same ``ok``
    mask, same clamp of ``Y`` -- on a copy: the caller's arrays are not altered): u = (Y - Xa) / sqrt(Sa scale) at the observed
    cells (cells with ``Sa scale == 0`` dropped) -> ``innovation_covariogram`` (``max_km``, ``nbins``, ``ctx`` from ``kw``) ->
    ``fit_correlation`` (``L_bounds``, ``min_count`` from ``kw``).  -> the fit dict with the covariogram under ``"covariogram"``."""
    cg_kw = {k: kw.pop(k) for k in ("max_km", "nbins", "ctx") if k in kw}
    fit_kw = {k: kw.pop(k) for k in ("L_bounds", "min_count") if k in kw}
    if kw:
        raise TypeError(f"estimate_corr_length: unexpected arguments {sorted(kw)}")
    for name in ([corr] if isinstance(corr, str) else corr):
        corr_kind(name)                                       # (ValueError before anything is touched)
    Xa, Sa, So = np.asarray(Xa, dtype=np.float64), np.asarray(Sa, dtype=np.float64), np.asarray(So, dtype=np.float64)
    Y = np.array(Y, dtype=np.float64)
    Y[Y < 0] = 0.0
    var = np.ravel(Sa) * float(scale)
    ok = np.isfinite(np.ravel(Y)) & np.isfinite(np.ravel(So)) & np.isfinite(np.ravel(Xa)) & np.isfinite(np.ravel(Sa)) & (var != 0)
    cell = np.flatnonzero(ok)
    cg = innovation_covariogram(np.ravel(lat)[cell], np.ravel(lon)[cell], (np.ravel(Y) - np.ravel(Xa))[cell],
                                sigma=np.sqrt(var[cell]), **cg_kw)
    return {**fit_correlation(cg, corr, **fit_kw), "covariogram": cg}


# ---- quality control of the innovations: background check and buddy check ----------------------------
BUDDY_CMIN = float(np.exp(-2.0))                     # buddies are the observations with C >= exp(-2): within 2 L for the Gaussian
QC_KEPT, QC_BACKGROUND, QC_BUDDY, QC_NOT_FINITE = 0, 1, 2, 3


def buddy_sums(obs_lat, obs_lon, u, L_km, corr="gaussian", cmin=BUDDY_CMIN, ctx=None):
    """The buddy sums of the normalised innovations ``u`` on the device (``oisat_buddy_sums``; the pair rule is written out in
    include/oisat.h): per observation, over the other observations with a finite ``u`` whose correlation ``c`` with it (model
    ``corr`` at length ``L_km``) is at least ``cmin``: ``n`` their number, ``W = sum c``, ``P = sum c u_b``, ``Q = sum c u_b^2``.
    An observation whose own ``u`` is not finite gets zeros.  Sorted by latitude for the kernel's window, returned in the
    caller's order; bitwise repeatable.  -> dict ``n`` (int32), ``W``, ``P``, ``Q`` (float64)."""
    kind = corr_kind(corr)
    lat = np.ravel(np.asarray(obs_lat, dtype=np.float64))
    lon = np.ravel(np.asarray(obs_lon, dtype=np.float64))
    uu = np.ravel(np.asarray(u, dtype=np.float64))
    m = int(uu.size)
    if lat.size != m or lon.size != m:
        raise ValueError("obs_lat, obs_lon and u must have the same size")
    c = ctx or _hip.context()
    n, sums = np.zeros(m, dtype=np.int32), np.zeros((3, m))
    if m == 0:
        return {"n": n, "W": sums[0], "P": sums[1], "Q": sums[2]}
    o = latitude_order(lat)
    bufs = [c.upload(unit_vectors(lat[o], lon[o])), c.upload(uu[o]), c.upload(lat[o]), c.alloc(4 * m), c.alloc(24 * m)]
    try:
        c.check(c.lib.oisat_set_correlation(c.h, kind))
        try:
            c.check(c.lib.oisat_buddy_sums(c.h, bufs[0].ptr, bufs[1].ptr, m, decay_constant(L_km), float(cmin), bufs[2].ptr,
                                           bufs[3].ptr, bufs[4].ptr))
            ns = c.download(bufs[3].ptr, (m,), np.int32)
            ss = c.download(bufs[4].ptr, (3, m), np.float64)
        finally:
            c.check(c.lib.oisat_set_correlation(c.h, CORRELATIONS["gaussian"]))
    finally:
        for b in bufs:
            b.free()
    n[o] = ns
    sums[:, o] = ss
    return {"n": n, "W": sums[0], "P": sums[1], "Q": sums[2]}


def buddy_stats(W, P, Q):
    """``(mean, var)`` of the buddies' innovations from their sums: ``mean = P / W``, ``var = max(Q / W - mean^2, 0)``; NaN where
    ``W`` is not positive."""
    W, P, Q = (np.asarray(a, dtype=np.float64) for a in (W, P, Q))
    has = W > 0
    Ws = np.where(has, W, 1.0)
    mean = np.where(has, P / Ws, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        var = np.where(has, np.maximum(Q / Ws - mean * mean, 0.0), np.nan)
    return mean, var


def buddy_decide(u, n, W, P, Q, k_background=5.0, k_buddy=3.0, min_buddies=3):
    """The decision of one pass, host only.  -> ``reason``, uint8 per observation, tested in this order: 3 = ``u`` is not finite;
    1 = ``|u| > k_background`` (background check); 2 = ``n >= min_buddies`` and ``|u - mean| > k_buddy sqrt(1 + var)`` with
    ``mean = P / W``, ``var = max(Q / W - mean^2, 0)`` (buddy check); 0 = kept.  ``u`` has unit variance under the model and
    ``var`` is the buddies' own weighted spread: an outlier among the buddies widens its neighbours' thresholds instead of
    getting them rejected, and the next pass judges them without it.  Fewer than ``min_buddies`` buddies, or ``W = 0``: the
    background check alone."""
    u = np.ravel(np.asarray(u, dtype=np.float64))
    n = np.ravel(np.asarray(n))
    mean, var = buddy_stats(np.ravel(W), np.ravel(P), np.ravel(Q))
    fin = np.isfinite(u)
    reason = np.zeros(u.size, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        judged = fin & (n >= min_buddies) & np.isfinite(mean) & np.isfinite(var)
        dev = np.abs(np.where(judged, u - np.where(judged, mean, 0.0), 0.0))
        buddy = judged & (dev > float(k_buddy) * np.sqrt(1.0 + np.where(judged, var, 0.0)))
        reason[buddy] = QC_BUDDY
        reason[fin & (np.abs(u) > float(k_background))] = QC_BACKGROUND
    reason[~fin] = QC_NOT_FINITE
    return reason


def buddy_check(obs_lat, obs_lon, u, L_km, corr="gaussian", cmin=BUDDY_CMIN, k_background=5.0, k_buddy=3.0, min_buddies=3,
                max_passes=4, ctx=None):
    """Background check plus iterated buddy check of the normalised innovations ``u``.  Each pass computes the buddy sums over
    the observations still in use (``buddy_sums``) and decides (``buddy_decide``); the newly rejected observations get
    ``u = NaN`` on a copy, so that a rejected observation stops vouching for others; it ends when a pass rejects nothing or after
    ``max_passes``.  An observation whose ``u`` is not finite to begin with is rejected in the first pass (reason 3).
    -> dict ``rejected`` (bool), ``reason`` (uint8: the reason at the pass that rejected it, 0 = kept), ``passes`` (rejections
    per pass), ``n`` / ``mean`` / ``spread`` (buddies, their weighted mean and standard deviation at the last pass; NaN without
    buddies) and the settings."""
    corr_kind(corr)
    if int(max_passes) < 1:
        raise ValueError(f"max_passes must be at least 1, not {max_passes!r}")
    work = np.array(np.ravel(np.asarray(u, dtype=np.float64)))
    m = int(work.size)
    reason = np.zeros(m, dtype=np.uint8)
    passes = []
    s = {"n": np.zeros(m, dtype=np.int32), "W": np.zeros(m), "P": np.zeros(m), "Q": np.zeros(m)}
    for _ in range(int(max_passes)):
        s = buddy_sums(obs_lat, obs_lon, work, L_km, corr=corr, cmin=cmin, ctx=ctx)
        r = buddy_decide(work, s["n"], s["W"], s["P"], s["Q"], k_background, k_buddy, min_buddies)
        new = (r != 0) & (reason == 0)
        reason[new] = r[new]
        work[new] = np.nan
        passes.append(int(new.sum()))
        if not new.any():
            break
    mean, var = buddy_stats(s["W"], s["P"], s["Q"])
    return {"rejected": reason != 0, "reason": reason, "passes": passes, "n": s["n"], "mean": mean, "spread": np.sqrt(var),
            "L_km": float(L_km), "corr": corr, "cmin": float(cmin), "k_background": float(k_background), "k_buddy": float(k_buddy),
            "min_buddies": int(min_buddies), "max_passes": int(max_passes)}


def qc_innovations(Xa, Y, Sa, So, lat, lon, L_km, scale=1.0, corr="gaussian", **kw):
    """``buddy_check`` with the gridded convention of ``OI_dense`` / ``estimate_corr_length`` (same ``ok`` mask, same clamp of
    ``Y`` -- on a copy: the caller's arrays are not altered): u = (Y - Xa) / sqrt(Sa scale + So), the innovation over its
    standard deviation under the model, at the observed cells; a cell where that variance is 0 or not finite is dropped and
    never flagged.  ``kw``: the settings of ``buddy_check``.  -> its dict (per checked observation, ``"cells"`` their flat
    indices) plus ``"rejected_cells"``, bool (ny, nx)."""
    corr_kind(corr)                                           # (ValueError before anything is touched)
    Xa, Sa, So = np.asarray(Xa, dtype=np.float64), np.asarray(Sa, dtype=np.float64), np.asarray(So, dtype=np.float64)
    Y = np.array(Y, dtype=np.float64)
    Y[Y < 0] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        var = np.ravel(Sa) * float(scale) + np.ravel(So)
    ok = (np.isfinite(np.ravel(Y)) & np.isfinite(np.ravel(So)) & np.isfinite(np.ravel(Xa)) & np.isfinite(np.ravel(Sa))
          & np.isfinite(var) & (var > 0))
    cell = np.flatnonzero(ok)
    u = (np.ravel(Y) - np.ravel(Xa))[cell] / np.sqrt(var[cell])
    out = buddy_check(np.ravel(lat)[cell], np.ravel(lon)[cell], u, L_km, corr=corr, **kw)
    mask = np.zeros(Xa.size, dtype=bool)
    mask[cell[out["rejected"]]] = True
    return {**out, "cells": cell, "rejected_cells": mask.reshape(np.shape(Xa))}


# ---- superobservations: the observations of one box merged into one ---------------------------------
SUPEROB_MAX_OBS = 1 << 20                            # include/oisat.h: oisat_superob
SUPEROB_LADDER = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)     # box sizes "auto" tries, degrees, smallest first
SUPEROB_AUTO_MAX_OBS = 100_000                       # "auto": the size the headline is measured at
KM_PER_DEG = 111.19                                  # a degree of latitude on the sphere of EARTH_RADIUS_KM
_SO_W, _SO_Q, _SO_D, _SO_V, _SO_G, _SO_PX = 0, 1, 2, 3, 4, 5   # rows of oisat_superob's sums_out (then Py, Pz)


def _lib_check(lib, rc):
    if rc != 0:
        raise _hip.OisatError(f"liboisat_hip error {rc}: {lib.oisat_last_error().decode()}")


def _superob_rho(rho) -> float:
    rho = float(rho)
    if not (0.0 <= rho < 1.0):
        raise ValueError(f"superob_rho must be in [0, 1), not {rho!r}")
    return rho


def superob_setting(v):
    """``None`` / ``"off"`` -> ``(None, 0)``; a positive number (or its string) -> ``(box_deg, 0)``; ``"auto"`` /
    ``"auto:<max_obs>"`` -> ``("auto", max_obs)`` (default ``SUPEROB_AUTO_MAX_OBS``; a positive integer).  Anything else is a
    ``ValueError``."""
    if v is None:
        return None, 0
    bad = ValueError(f"superob: expected off, <degrees> in (0, 180], auto or auto:<max_obs> (a positive integer), not {v!r}")
    if isinstance(v, str):
        t = v.strip().lower()
        if t == "off":
            return None, 0
        if t == "auto":
            return "auto", SUPEROB_AUTO_MAX_OBS
        if t.startswith("auto:"):
            try:
                n = int(t[5:])
            except ValueError:
                raise bad from None
            if n < 1:
                raise bad
            return "auto", n
        try:
            v = float(t)
        except ValueError:
            raise bad from None
    if isinstance(v, bool):
        raise bad
    try:
        deg = float(v)
    except (TypeError, ValueError):
        raise bad from None
    if not (0.0 < deg <= 180.0):
        raise bad
    return deg, 0


def superob_boxes(box_deg):
    """The box table of ``oisat_superob`` for boxes of ``box_deg`` degrees (host only, float64; the rule is in include/oisat.h):
    -> dict ``box_deg``, ``nbands``, ``nbox``, ``n`` (int32 per latitude band: its longitude boxes), ``offset`` (int64: the id of
    the band's first box)."""
    lib = _hip.load_library()
    box_deg = float(box_deg)
    nbands, nbox = C.c_int64(0), C.c_int64(0)
    _lib_check(lib, lib.oisat_superob_boxes(box_deg, 0, None, None, C.byref(nbands), C.byref(nbox)))
    n, off = np.zeros(nbands.value, dtype=np.int32), np.zeros(nbands.value, dtype=np.int64)
    _lib_check(lib, lib.oisat_superob_boxes(box_deg, n.size, n.ctypes.data, off.ctypes.data, C.byref(nbands), C.byref(nbox)))
    return {"box_deg": box_deg, "nbands": int(nbands.value), "nbox": int(nbox.value), "n": n, "offset": off}


def superob_quanta(wmax: float, dmax: float, smax: float, m: int) -> np.ndarray:
    """The six quanta ``q_W, q_Q, q_D, q_V, q_G, q_P`` of ``oisat_superob`` (host only; ``OisatError`` outside its range)."""
    lib = _hip.load_library()
    q = np.zeros(6)
    _lib_check(lib, lib.oisat_superob_quanta(float(wmax), float(dmax), float(smax), int(m), q.ctypes.data))
    return q


def _superob_inputs(obs_lat, obs_lon, innovation, sigma_b, obs_var):
    d = np.ravel(np.asarray(innovation, dtype=np.float64))
    arrs = [np.ravel(np.asarray(a, dtype=np.float64)) for a in (obs_lat, obs_lon)] + [d]
    arrs += [np.ravel(np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(innovation))) for a in (sigma_b, obs_var)]
    if any(a.size != d.size for a in arrs):
        raise ValueError("obs_lat, obs_lon, innovation, sigma_b and obs_var must have the same size")
    if d.size > SUPEROB_MAX_OBS:
        raise ValueError(f"{d.size} observations; superobservations take at most {SUPEROB_MAX_OBS}")
    return arrs


def _superob_device(c, lat, lon, d, sig, var, table, with_sums):
    """``oisat_superob`` on host arrays -> (box int32[m], count int64[nbox], sums float64[8][nbox] or None, nused)."""
    m, nbox = int(d.size), table["nbox"]
    count = np.zeros(nbox, dtype=np.int64)
    sums = np.zeros((8, nbox)) if with_sums else None
    used = C.c_int64(0)
    if m == 0:
        return np.zeros(0, dtype=np.int32), count, sums, 0
    bufs = [c.upload(a) for a in (lat, lon, d, sig, var)] + [c.alloc(4 * m)]
    if with_sums:
        bufs.append(c.upload(unit_vectors(lat, lon)))
    try:
        c.check(c.lib.oisat_superob(c.h, bufs[0].ptr, bufs[1].ptr, bufs[6].ptr if with_sums else None, bufs[2].ptr, bufs[3].ptr,
                                    bufs[4].ptr, m, table["box_deg"], table["n"].ctypes.data, table["offset"].ctypes.data,
                                    table["nbands"], nbox, bufs[5].ptr, count.ctypes.data,
                                    sums.ctypes.data if with_sums else None, C.byref(used)))
        box = c.download(bufs[5].ptr, (m,), np.int32)
    finally:
        for b in bufs:
            b.free()
    return box, count, sums, int(used.value)


def superob_count(obs_lat, obs_lon, innovation, sigma_b, obs_var, box_deg, ctx=None) -> int:
    """The number of non-empty boxes of ``box_deg`` degrees, i.e. of superobservations ``superob`` would return (the kernel's
    count-only form: no sums are formed)."""
    lat, lon, d, sig, var = _superob_inputs(obs_lat, obs_lon, innovation, sigma_b, obs_var)
    _, count, _, _ = _superob_device(ctx or _hip.context(), lat, lon, d, sig, var, superob_boxes(box_deg), False)
    return int(np.count_nonzero(count))


def superob_ladder_pick(counts, max_obs: int) -> float:
    """The smallest box of ``SUPEROB_LADDER`` whose number of non-empty boxes is at most ``max_obs``.  ``counts``: a mapping
    ``box_deg -> count`` or a callable giving it (called for the boxes in ascending order, up to the first that fits).  None
    fits: a ``ValueError`` that names the counts."""
    get = counts if callable(counts) else counts.__getitem__
    seen = []
    for box in SUPEROB_LADDER:
        n = int(get(box))
        seen.append((box, n))
        if n <= int(max_obs):
            return box
    raise ValueError(f"superob auto: no box of the ladder leaves at most {int(max_obs)} superobservations (box_deg: count = "
                     + ", ".join(f"{b:g}: {n}" for b, n in seen) + ")")


def superob_auto_box(obs_lat, obs_lon, innovation, sigma_b, obs_var, max_obs, ctx=None) -> float:
    """``superob_ladder_pick`` with the counts from ``superob_count``."""
    return superob_ladder_pick(lambda box: superob_count(obs_lat, obs_lon, innovation, sigma_b, obs_var, box, ctx=ctx), max_obs)


def superob(obs_lat, obs_lon, innovation, sigma_b, obs_var, box_deg, rho=0.0, ctx=None):
    """Superobservations: the observations inside one box of a roughly equal-area grid of ``box_deg`` degrees merged into one,
    the inverse-variance-weighted mean.  The per-box sums are formed on the device (``oisat_superob``: exact integer sums,
    bitwise repeatable and independent of the order of the observations); with w = 1 / var and, per box, W = sum w,
    Q = sum sqrt(w), D = sum w d, V = sum w d^2, G = sum w sigma_b, P = sum w (x, y, z):
    position = P normalised; ``d = D / W``; ``sigma_b = G / W``; ``var = ((1 - rho) W + rho Q^2) / W^2``, the variance of that
    mean when the members' errors share a uniform correlation ``rho`` (0 <= rho < 1; 0: 1 / W); ``spread = max(V / W - d^2, 0)``,
    the members' weighted scatter (a diagnostic, not fed back).  An observation takes part iff its five numbers are finite,
    |lat| <= 90 and 1 / var is finite; one that would but for ``var <= 0`` is a ``ValueError``.
    -> dict, the superobservations of the non-empty boxes in ascending box id: ``lat``, ``lon``, ``d``, ``sigma_b``, ``var``,
    ``spread``, ``count``, ``W``, ``box_id``; per observation ``box`` (int32, -1: takes no part) and ``index`` (its
    superobservation, -1 likewise); ``nobs`` (superobservations), ``nobs_raw`` (observations that take part), ``box_deg``, ``rho``."""
    rho = _superob_rho(rho)
    lat, lon, d, sig, var = _superob_inputs(obs_lat, obs_lon, innovation, sigma_b, obs_var)
    with np.errstate(invalid="ignore"):
        wrong = np.isfinite(lat) & np.isfinite(lon) & np.isfinite(d) & np.isfinite(sig) & np.isfinite(var) & (np.abs(lat) <= 90) & (var <= 0)
    if wrong.any():
        raise ValueError(f"{int(wrong.sum())} observation(s) with an error variance <= 0 cannot be merged (first: index "
                         f"{int(np.flatnonzero(wrong)[0])})")
    table = superob_boxes(box_deg)
    box, count, sums, nused = _superob_device(ctx or _hip.context(), lat, lon, d, sig, var, table, True)
    ids = np.flatnonzero(count)
    W, Q, D, V, G = (sums[k][ids] for k in (_SO_W, _SO_Q, _SO_D, _SO_V, _SO_G))
    P = sums[_SO_PX:_SO_PX + 3][:, ids]
    norm = np.sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2])
    if ids.size and not (norm > 0).all():
        raise ValueError(f"superob: the members of a {table['box_deg']:g} degree box cancel each other's position; use smaller boxes")
    dm = D / W
    index = np.full(box.size, -1, dtype=np.int64)
    lookup = np.full(table["nbox"], -1, dtype=np.int64)
    lookup[ids] = np.arange(ids.size)
    index[box >= 0] = lookup[box[box >= 0]]
    return {"lat": np.rad2deg(np.arcsin(np.clip(P[2] / norm, -1.0, 1.0))), "lon": np.rad2deg(np.arctan2(P[1], P[0])),
            "d": dm, "sigma_b": G / W, "var": ((1.0 - rho) * W + rho * Q * Q) / (W * W),
            "spread": np.maximum(V / W - dm * dm, 0.0), "count": count[ids], "W": W, "box_id": ids, "box": box, "index": index,
            "nobs": int(ids.size), "nobs_raw": int(nused), "box_deg": table["box_deg"], "rho": rho}


_superob_fn = superob                                # (``OI_dense`` has an argument of that name)
