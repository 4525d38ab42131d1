"""Batches for the batched gain solve and increment (``oisat_batch_set_solve`` / ``_set_grid`` / ``_solve`` / ``_analyse``) and
their float64 references (NumPy / SciPy only, no device).

A batch is a list of members in CALLER order.  Per member and (correlation length, model): ``S64`` = sig sig^T .* C + diag(var)
with the correlation formulas of include/oisat.h written out below and NO cut-off, ``z_ref = cho_solve(S64, d)``, and
``inc_of(z)`` = gsig_i sum_a C(i, a) osig_a z_a in float64 -- a function of z, so that the increment kernel is judged on the
device's own z.  The bars of tests/test_gpu_batch_abi.py (``delta``, ``inc_bar``) and the restatements that
tests/test_batch_cases_cpu.py mutates live here too, so that both files judge by the same numbers."""
import functools

import numpy as np
import scipy.linalg as sla

from oisatgmi import dense

NB = 128
R_KM = 6371.0
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}
MODELS = ("gaussian", "gaspari_cohn", "soar")
LENGTHS = (300.0, 800.0, 5000.0)                                # compact blocks | latitude rows, windowed | no window (Gaussian)
TOL = 1e-6                                                      # the library's default (oisat_set_refine_tol)
CUT_BITS, FAR_BITS, FAR_REL = 52.0, 28.0, 2e-5                  # kCutBits, kSolveFarBits, the fp32 tier's relative error
COND_MAX, EIG_MIN = 1e4, 1e-3


def decay(L_km):
    return 0.5 * (R_KM / L_km) ** 2


# ---- the correlation, float64, as printed in include/oisat.h -----------------------------------------------------------------
def chord2(pa, pb):
    out = np.zeros((pa.shape[1], pb.shape[1]))
    for k in range(3):
        out += (pa[k][:, None] - pb[k][None, :]) ** 2
    return out


def corr(d2, L_km, model):
    g = decay(L_km)
    if model == "gaussian":
        return np.exp(-g * d2)
    if model == "soar":
        s = np.sqrt(2.0 * g * d2)
        return (1.0 + s) * np.exp(-s)
    z = np.sqrt(0.6 * g * d2)
    near = -z ** 5 / 4 + z ** 4 / 2 + 5 * z ** 3 / 8 - 5 * z ** 2 / 3 + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        far = z ** 5 / 12 - z ** 4 / 2 + 5 * z ** 3 / 8 + 5 * z ** 2 / 3 - 5 * z + 4 - 2 / (3 * z)
    return np.where(z <= 1, near, np.where(z < 2, np.maximum(far, 0.0), 0.0))


# ---- the library's host rules, restated (csrc/dense_solve_dev.inc) ----------------------------------------------------------
LOG2E_F = float(np.float32(1.4426950408889634))                 # kLog2e is a float


def cut_chord(model, g, bits=CUT_BITS):
    if model == "soar":
        lt, lo, hi = -bits * np.log(2.0), 0.0, 2.0 * bits + 2.0
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            if np.log1p(mid) - mid > lt:
                lo = mid
            else:
                hi = mid
        return hi / np.sqrt(2.0 * g)
    if model == "gaussian":
        return np.sqrt(bits / (g * LOG2E_F))
    return 2.0 / np.sqrt(0.6 * g)                               # (bits >= kCutBits: the support chord)


def lat_window_deg(model, g):
    c = cut_chord(model, g)
    return 1e9 if c >= 2.0 else 2.0 * np.arcsin(0.5 * c) * 57.29577951308232


def residual_blocks_pay(model, g):
    if model != "gaussian":
        return cut_chord(model, g) <= 0.5
    return np.sqrt(64.0 / (g * LOG2E_F)) <= 0.5


def regime(model, L_km, all_perm=True):
    """"blocks" (compact residual blocks), "rows" (latitude rows, windowed) or "full" (no window)."""
    g = decay(L_km)
    if lat_window_deg(model, g) >= 180.0:
        return "full"
    return "blocks" if (residual_blocks_pay(model, g) and all_perm) else "rows"


def increment_cells(cu_count, max_n, nmem):
    return 1 if -(-max_n // 512) * nmem < 4 * (cu_count if cu_count > 0 else 256) else 2


def increment_blocks(n, nx, cells):
    return -(-nx // 32) * -(-(n // nx) // (8 * cells)) if nx > 0 else -(-n // (256 * cells))


# ---- members -------------------------------------------------------------------------------------------------------------------
class Member:
    """Observations in ascending latitude; cells; everything the ABI takes, float64."""

    def __init__(self, name, olat, olon, glat, glon, nx, seed, perm_kind="morton"):
        rng = np.random.default_rng(seed)
        o = np.argsort(olat, kind="stable")
        self.name = name
        self.olat, self.olon = np.ascontiguousarray(olat[o], dtype=np.float64), np.ascontiguousarray(olon[o], dtype=np.float64)
        self.m = m = self.olat.size
        self.mp = -(-m // NB) * NB
        self.oxyz = dense.unit_vectors(self.olat, self.olon)
        self.osig = rng.uniform(0.8, 1.2, m)
        self.ovar = rng.uniform(0.3, 1.0, m)
        self.d = rng.standard_normal(m)
        self.glat, self.glon = np.ascontiguousarray(np.ravel(glat), dtype=np.float64), np.ascontiguousarray(np.ravel(glon), dtype=np.float64)
        self.n, self.nx = self.glat.size, int(nx)
        self.gxyz = dense.unit_vectors(self.glat, self.glon)
        self.gsig = rng.uniform(0.8, 1.2, self.n)
        self.xb = rng.standard_normal(self.n) * 3.0
        self.perm_kind = perm_kind
        self._cache = {}

    def clone(self, **kw):
        c = object.__new__(Member)
        c.__dict__.update(self.__dict__)
        c._cache = {}
        c.__dict__.update(kw)
        return c

    def perm(self):
        """int32[m] or None (the member hands the library no permutation)."""
        if self.perm_kind is None:
            return None
        if self.perm_kind == "identity":
            return np.arange(self.m, dtype=np.int32)
        if self.perm_kind == "reverse":
            return np.arange(self.m, dtype=np.int32)[::-1].copy()
        return dense.morton_order(self.olat, self.olon)

    def S64(self, L_km, model):
        k = ("S", L_km, model)
        if k not in self._cache:
            S = corr(chord2(self.oxyz, self.oxyz), L_km, model) * self.osig[:, None] * self.osig[None, :]
            S[np.diag_indices_from(S)] += self.ovar
            self._cache[k] = S
        return self._cache[k]

    def z_ref(self, L_km, model):
        k = ("z", L_km, model)
        if k not in self._cache:
            self._cache[k] = sla.cho_solve(sla.cho_factor(self.S64(L_km, model), lower=True), self.d)
        return self._cache[k]

    def cross(self, L_km, model):
        """C(i, a), n x m (cached for the small grids only)."""
        k = ("G", L_km, model)
        if k in self._cache:
            return self._cache[k]
        G = corr(chord2(self.gxyz, self.oxyz), L_km, model)
        if self.n * self.m <= 2_000_000:
            self._cache[k] = G
        return G

    def inc_of(self, z, L_km, model):
        return self.gsig * (self.cross(L_km, model) @ (self.osig * z))

    def z_f32(self, L_km, model):
        """The yardstick e32 of the plain solve, by the rule of tests/readers_cases.py: the SAME operation evaluated plainly in
        float32 on the CPU -- coordinates cast to float32, squared chord, correlation, sig sig^T .* C + var in float32 -- and a
        float32 LAPACK factor-and-solve of that matrix."""
        f = np.float32
        p = self.oxyz.astype(f)
        d2 = np.zeros((self.m, self.m), dtype=f)
        for k in range(3):
            dk = p[k][:, None] - p[k][None, :]
            d2 += dk * dk
        g = decay(L_km)
        if model == "gaussian":
            Cf = np.exp(-f(g) * d2)
        elif model == "soar":
            s = np.sqrt(f(2.0 * g) * d2)
            Cf = (f(1) + s) * np.exp(-s)
        else:
            z = np.sqrt(f(0.6 * g) * d2)
            z2, z3 = z * z, z * z * z
            near = -z3 * z2 / f(4) + z2 * z2 / f(2) + f(5) * z3 / f(8) - f(5) * z2 / f(3) + f(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                far = z3 * z2 / f(12) - z2 * z2 / f(2) + f(5) * z3 / f(8) + f(5) * z2 / f(3) - f(5) * z + f(4) - f(2) / (f(3) * z)
            Cf = np.where(z <= 1, near, np.where(z < 2, np.maximum(far, f(0)), f(0))).astype(f)
        sg = self.osig.astype(f)
        S32 = (Cf * sg[:, None] * sg[None, :]).astype(f)
        S32[np.diag_indices_from(S32)] += self.ovar.astype(f)
        assert S32.dtype == f
        return sla.cho_solve(sla.cho_factor(S32, lower=True), self.d.astype(f)).astype(np.float64)

    def delta(self, L_km, model, tol=TOL):
        """What separates |d - S64 z| from the library's own float64 residual, relative to tol |d|.  The library leaves out
        terms below 2^-52 of a term of correlation 1 and rounds its exponential (1 ulp, 2^-52): each entry of its S is within
        2^-51 max(diag S) of S64's, so |dS z| <= m 2^-51 max(diag) |z| and |z| <= |d| / lambda_min; its two norms are sums of m
        squares in float64 (m 2^-52 relative).  m = 700, max(diag) / lambda_min ~ 5: 1.5e-6 at tol = 1e-6."""
        S = self.S64(L_km, model)
        lam = np.linalg.eigvalsh(S)[0]
        return self.m * 2.0 ** -51 * S.diagonal().max() / lam / tol + self.m * 2.0 ** -52

    def inc_bar(self, z, model, f32=False, ref=None, xa_ref=None):
        """Per cell: gsig_i sum_a |osig_a z_a| (far + cut + acc).  far = 2^-kSolveFarBits x 2e-5: an observation of the fp32 tier has
        a correlation below 2^-28 with every cell of the patch and carries fp32's relative error (Gaussian only: no tier
        otherwise); cut = 2^-52: a term left out is below that; acc = 4 m 2^-53: the rounding of the squared chord, of the
        product and of m additions in float64.  float32 fields: inc is rounded once on its store (2^-24 |inc|); xa is formed as
        (double) xb + inc in DOUBLE and rounded once (2^-24 |xa|) -- returned as a pair then."""
        far = 2.0 ** -FAR_BITS * FAR_REL if model == "gaussian" else 0.0
        bar = self.gsig * np.abs(self.osig * z).sum() * (far + 2.0 ** -CUT_BITS + 4.0 * self.m * 2.0 ** -53)
        if not f32:
            return bar, bar
        return bar + 2.0 ** -24 * np.abs(ref), bar + 2.0 ** -24 * np.abs(xa_ref)


def _box(rng, m, lat0, lat1, lon0, lon1):
    return rng.uniform(lat0, lat1, m), rng.uniform(lon0, lon1, m)


def _grid(ny, nx, lat0, lat1, lon0, lon1):
    la, lo = np.meshgrid(np.linspace(lat0, lat1, ny), np.linspace(lon0, lon1, nx), indexing="ij")
    return la, lo


def _wrap(lon):
    return (np.asarray(lon) + 180.0) % 360.0 - 180.0


# caller order of ``mixed``: no member's caller index equals its index in the library's table (largest block count first,
# stable), and the largest is not first (tests/test_batch_cases_cpu.py asserts both)
MIXED_M = (128, 257, 1, 700, 300, 64, 127, 385, 129)


@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(20240611)
    mem = []
    # c0, m = 128: a random box; a run of 300 cells with no shape
    la, lo = _box(rng, 128, -20.0, 8.0, 40.0, 70.0)
    mem.append(Member("box128", la, lo, rng.uniform(-20.0, 8.0, 300), rng.uniform(40.0, 70.0, 300), 0, 1))
    # c1, m = 257: its 257 cells (no shape) ARE the observation positions: chord 0
    la, lo = _box(rng, 257, 30.0, 58.0, -30.0, 5.0)
    o = np.argsort(la, kind="stable")
    mem.append(Member("coincide257", la, lo, la[o][::-1].copy(), lo[o][::-1].copy(), 0, 2))
    # c2, m = 1: one observation, one cell
    mem.append(Member("one", np.array([12.5]), np.array([100.0]), np.array([[13.0]]), np.array([[101.0]]), 1, 3))
    # c3, m = 700: a box across the date line, 37 x 50 cells
    la, lo = _box(rng, 700, 10.0, 40.0, 165.0, 195.0)
    gla, glo = _grid(37, 50, 10.0, 40.0, 165.0, 195.0)
    mem.append(Member("dateline700", la, _wrap(lo), gla, _wrap(glo), 50, 4))
    assert (mem[-1].olon > 170).any() and (mem[-1].olon < -170).any() and (mem[-1].glon > 170).any() and (mem[-1].glon < -170).any()
    # c4, m = 300: every observation on one latitude (window-edge ties), 16 x 48 cells
    gla, glo = _grid(16, 48, 8.0, 32.0, 0.0, 30.0)
    mem.append(Member("onelat300", np.full(300, 20.0), rng.uniform(0.0, 30.0, 300), gla, glo, 48, 5))
    # c5, m = 64: a random box, 16 x 48 cells
    la, lo = _box(rng, 64, -50.0, -25.0, -80.0, -50.0)
    gla, glo = _grid(16, 48, -50.0, -25.0, -80.0, -50.0)
    mem.append(Member("box64", la, lo, gla, glo, 48, 6))
    # c6, m = 127: a random box, 8 x 32 cells
    la, lo = _box(rng, 127, 0.0, 25.0, -120.0, -95.0)
    gla, glo = _grid(8, 32, 0.0, 25.0, -120.0, -95.0)
    mem.append(Member("box127", la, lo, gla, glo, 32, 7))
    # c7, m = 385: a cap that contains the pole, one observation AT it; 33 x 65 cells on a plane through the pole, both sides
    la, lo = 90.0 - 15.0 * np.sqrt(rng.uniform(0.0, 1.0, 385)), rng.uniform(-180.0, 180.0, 385)
    la[0], lo[0] = 90.0, 0.0
    yy, xx = np.meshgrid(np.linspace(-12.0, 12.0, 33), np.linspace(-12.0, 12.0, 65), indexing="ij")
    mem.append(Member("cap385", la, lo, 90.0 - np.hypot(xx, yy), np.degrees(np.arctan2(yy, xx)), 65, 8))
    assert mem[-1].olat[-1] == 90.0
    # c8, m = 129: two observations at one position with different variances, 16 x 48 cells
    la, lo = _box(rng, 129, -10.0, 18.0, 10.0, 40.0)
    la[1], lo[1] = la[0], lo[0]
    gla, glo = _grid(16, 48, -10.0, 18.0, 10.0, 40.0)
    mb = Member("twin129", la, lo, gla, glo, 48, 9)
    k = int(np.flatnonzero((mb.olat[1:] == mb.olat[:-1]) & (mb.olon[1:] == mb.olon[:-1]))[0])
    mb.ovar[k], mb.ovar[k + 1] = 0.35, 0.9
    mem.append(mb)
    assert tuple(x.m for x in mem) == MIXED_M
    return tuple(mem)


NO_PERM_MEMBER = 5                                              # mixed_no_perm: this member hands over no permutation


@functools.lru_cache(maxsize=None)
def mixed_no_perm():
    return tuple(x.clone(perm_kind=None) if i == NO_PERM_MEMBER else x for i, x in enumerate(mixed()))


@functools.lru_cache(maxsize=None)
def mixed_perm(kind):
    """``mixed`` with every member's perm of one kind: "identity", "reverse" or "morton"."""
    return tuple(x.clone(perm_kind=kind) for x in mixed())


def table_order(ms):
    """The library's table: largest block count first, stable (oisat_batch_create); returns caller indices in table order."""
    return sorted(range(len(ms)), key=lambda i: -(-(-ms[i] // NB)))


# ---- two_cells -----------------------------------------------------------------------------------------------------------------
TWO_CELLS_L = 800.0


@functools.lru_cache(maxsize=None)
def two_cells():
    """64 members, max_n = 8192: cdiv(8192, 512) * 64 = 1024 = 4 * 256, the smallest batch on the two-cell side at 256 CUs."""
    rng = np.random.default_rng(77)
    mem = []
    for i in range(64):
        m = int(rng.integers(130, 301))
        lat0, lon0 = rng.uniform(-60.0, 35.0), rng.uniform(-170.0, 140.0)
        la, lo = _box(rng, m, lat0, lat0 + 25.0, lon0, lon0 + 30.0)
        if i == 3:                                              # a run of 8191 cells with no shape
            mem.append(Member(f"run{i}", la, lo, rng.uniform(lat0, lat0 + 25.0, 8191), rng.uniform(lon0, lon0 + 30.0, 8191), 0, 100 + i))
            continue
        if i == 40:                                             # one cell
            mem.append(Member(f"cell{i}", la, lo, np.array([lat0 + 3.0]), np.array([lon0 + 4.0]), 1, 100 + i))
            continue
        ny, nx = ((64, 128), (37, 221), (37, 221), (16, 48), (33, 65))[0 if i == 10 else 1 + i % 4]
        gla, glo = _grid(ny, nx, lat0, lat0 + 25.0, lon0, lon0 + 30.0)
        mem.append(Member(f"grid{i}", la, lo, gla, glo, nx, 100 + i))
    return tuple(mem)


# ---- one_hard / two_hard: the refinement's bookkeeping -------------------------------------------------------------------------
HARD_L, HARD_MODEL = 800.0, "gaussian"
HARD_MEMBER, HARD_MEMBER_2 = 4, 7                               # caller indices (m = 300 and m = 385; table indices 3 and 1)
HARD_SCALE, HARD_TOL = 1e-3, 1e-7                               # chosen by emulate(): tests/test_batch_cases_cpu.py asserts the clearance


@functools.lru_cache(maxsize=None)
def hard(which=(HARD_MEMBER,)):
    return tuple(x.clone(ovar=x.ovar * HARD_SCALE) if i in which else x for i, x in enumerate(mixed()))


def one_hard():
    return hard((HARD_MEMBER,))


def two_hard():
    return hard((HARD_MEMBER, HARD_MEMBER_2))


def emulate(mb, L_km, model, tol, refine):
    """The library's refinement with a float32 LAPACK Cholesky of S64 as the preconditioner and float64 residuals: the plain
    solve, then at most ``refine`` corrections, each behind a residual that is above tol |d|; a last residual behind the last
    correction.  Returns (z, [|r_k| / |d|], converged)."""
    S = mb.S64(L_km, model)
    F = sla.cho_factor(S.astype(np.float32), lower=True)
    solve = lambda r: sla.cho_solve(F, r.astype(np.float32)).astype(np.float64)       # noqa: E731
    dn = np.linalg.norm(mb.d)
    z = solve(mb.d)
    norms = []
    if refine == 0:
        return z, norms, True
    for k in range(refine + 1):
        r = mb.d - S @ z
        norms.append(np.linalg.norm(r) / dn)
        if norms[-1] <= tol:
            return z, norms, True
        if k == refine:
            break
        z = z + solve(r)
    return z, norms, tol == 0.0


def changed_d(mb):
    """The other innovation of check (d): tests/test_gpu_batch_abi.py hands it to one member and asserts the others' bits."""
    return -2.0 * mb.d[::-1].copy() + 0.25


# ---- restatements that tests/test_batch_cases_cpu.py mutates -------------------------------------------------------------------
def window(mb, lat_lo, lat_hi, win_deg):
    """[j0, j1) of the latitude window of a block whose points span [lat_lo, lat_hi] (lower_bound_lat twice)."""
    return int(np.searchsorted(mb.olat, lat_lo - win_deg, side="left")), int(np.searchsorted(mb.olat, lat_hi + win_deg + 1e-9, side="left"))


def blocks_of(mb, cells=1):
    """The cells of every increment workgroup of a member (increment_patch): patches of 32 x 8 cells, or runs of 256."""
    if mb.nx > 0:
        ny, nx = mb.n // mb.nx, mb.nx
        idx = np.arange(mb.n).reshape(ny, nx)
        return [idx[y:y + 8 * cells, x:x + 32].ravel() for y in range(0, ny, 8 * cells) for x in range(0, nx, 32)]
    return [np.arange(a, min(a + 256 * cells, mb.n)) for a in range(0, mb.n, 256 * cells)]


def inc_windowed(mb, z, L_km, model, drop=None, narrow=None):
    """The increment as the kernel forms it: per workgroup the observations of its latitude window, float64.  ``drop`` =
    (cell, observation): that term is left out; ``narrow`` = the block whose window loses its last observation, or "all"."""
    win = lat_window_deg(model, decay(L_km))
    G, w = mb.cross(L_km, model), mb.osig * z
    out = np.empty(mb.n)
    for b, cells in enumerate(blocks_of(mb)):
        j0, j1 = (0, mb.m) if win >= 180.0 else window(mb, mb.glat[cells].min(), mb.glat[cells].max(), win)
        if narrow == b or narrow == "all":
            j1 -= 1
        out[cells] = mb.gsig[cells] * (G[cells, j0:j1] @ w[j0:j1])
    if drop is not None:
        i, a = drop
        out[i] -= mb.gsig[i] * G[i, a] * w[a]
    return out
