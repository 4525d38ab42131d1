"""Seeded catalogues of adversarial point sets, grids and triangulations for the horizontal regridding operators of
csrc/regrid.hip, and the CPU references they are judged by (tests/test_gpu_horizontal_abi.py on the device,
tests/test_horizontal_cases_cpu.py here).  Nothing in this file touches the GPU.

A. nearest neighbour -- ``nn_scene(name)``: one scene = one point set, one target list, one mask radius = one launch.  The
   reference is brute force in float64 with the kernel's own expression (d2 = dx*dx + dy*dy, dx = p - t, lowest index among
   equal d2, kept iff not sqrt(d2) > max_dist), so indices must be equal and distances bit-equal.  ``emulate_search`` restates
   build_hash / nn_count_kernel / nn_query_kernel in NumPy with the hash cell padded (the library) or not (the parent
   commit: it misses every ``border_ulp`` target, which is how the catalogue is known to be sharp).
B. box filter -- ``box_fields``: fields with NaN / +inf / (+inf, -inf) in one window; reference scipy's convolve2d in float64;
   the bar (win + 2) u sum|Z w| is the summation bound for any order (one rounding for the weight, one per product, win - 1
   additions), u = 2^-53 or 2^-24.
C. local thin-plate-spline RBF -- ``rbf_scene(kind, K)``: at most 64 points so that one-hot fields expose every evaluation
   weight; reference A np.linalg.solve on the documented system, reference B the kernel's elimination written out.
D. Delaunay linear interpolation -- ``linear_scene(name)``: scipy's own Delaunay arrays, LinearNDInterpolator as the reference.

A case the reference cannot judge is drawn again in the generator, never dropped at run time.
"""
import functools

import numpy as np
from scipy.signal import convolve2d
from scipy.spatial import Delaunay

SEED = 20261019
REPS = 24                                  # targets per category, about

# ---------------------------------------------------------------------------------------------------------------------
# A. nearest neighbour
# ---------------------------------------------------------------------------------------------------------------------
PAD = 2.0 ** -26                           # nn_query_impl: hash cell = max_dist * (1 + PAD)
MAX_CELLS = 4 * 1024 * 1024                # build_hash
SCAN_TILE = 4096                           # nn_scan_lookback_kernel
TIE_REL = 1.8e-15                          # nn_query_kernel: second - best <= best * TIE_REL
MAX_DISTS = (0.7, 1.5, 0.25 * np.sqrt(2.0), 2.0 * np.hypot(0.25, 0.3125))
ORIGINS = ("-180", "-179.875", "random")
# max_dist 1.5 against a dyadic origin: x - x0 and the cell borders are exact, no pair two cells apart exists (the CPU test
# searches 400,000 draws per axis and finds none), so there is no border_ulp scene to build there
BORDER_EXACT = ((1, "-180"), (1, "-179.875"))


class NNScene:
    def __init__(self, name, px, py, tx, ty, max_dist, tags):
        self.name, self.max_dist, self.tags = name, float(max_dist), list(tags)
        self.px, self.py = (np.ascontiguousarray(a, dtype=np.float64) for a in (px, py))
        self.tx, self.ty = (np.ascontiguousarray(a, dtype=np.float64) for a in (tx, ty))
        assert self.px.shape == self.py.shape and self.tx.shape == self.ty.shape == (len(self.tags),)

    @property
    def P(self):
        return self.px.size

    @property
    def T(self):
        return self.tx.size

    def where(self, tag):
        return np.array([i for i, t in enumerate(self.tags) if t == tag], dtype=np.int64)


def _d2_matrix(sc):
    """[T, P] squared distances as the kernel forms them; +inf for a NaN point or a NaN target"""
    with np.errstate(invalid="ignore"):
        dx = sc.px[None, :] - sc.tx[:, None]
        dy = sc.py[None, :] - sc.ty[:, None]
        d2 = dx * dx + dy * dy
    d2[np.isnan(d2)] = np.inf
    return d2


def _select(d2, max_dist):
    """nn_query_kernel's choice among the candidates that d2 leaves finite"""
    T, P = d2.shape
    bi = np.argmin(d2, axis=1)                                       # first minimum = lowest index
    best = d2[np.arange(T), bi]
    second = np.partition(d2, 1, axis=1)[:, 1] if P > 1 else np.full(T, np.inf)
    found = np.isfinite(best)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(best)
        keep = found & ~(d > max_dist)
        tie = keep & (second - best <= best * TIE_REL)
    return {"idx": np.where(keep, bi, -1).astype(np.int32), "dist": np.where(keep, d, np.inf),
            "ties": np.flatnonzero(tie).astype(np.int32), "dist_unmasked": d, "best": best, "second": second}


def brute_nn(sc):
    """the reference: every finite point looked at (kept on the scene: computed once, shared, never changed)"""
    if not hasattr(sc, "_brute"):
        sc._brute = _select(_d2_matrix(sc), sc.max_dist)
    return sc._brute


def hash_grid(px, py, cell):
    """build_hash: origin, 1 / cell and cell counts, the cell doubled until at most MAX_CELLS cells"""
    fin = ~(np.isnan(px) | np.isnan(py))
    if fin.any():
        x0, x1, y0, y1 = px[fin].min(), px[fin].max(), py[fin].min(), py[fin].max()
    else:
        x0 = x1 = y0 = y1 = 0.0
    spanx, spany = x1 - x0, y1 - y0
    while (np.floor(spanx / cell) + 1.0) * (np.floor(spany / cell) + 1.0) > MAX_CELLS:
        cell *= 2.0
    nbx, nby = int(np.floor(spanx / cell)) + 1, int(np.floor(spany / cell)) + 1
    return {"x0": x0, "y0": y0, "inv_h": 1.0 / cell, "nbx": nbx, "nby": nby, "ncell": nbx * nby, "cell": cell,
            "ntile": -(-nbx * nby // SCAN_TILE)}


def emulate_search(sc, pad=PAD):
    """The 3 x 3 hash search in NumPy.  pad = 0: the parent commit (cell edge = max_dist, targets past the box's edge skip
    what lies outside it); pad > 0: the library (padded cell, a target in cell nb + 1 looks from cell nb)."""
    g = hash_grid(sc.px, sc.py, sc.max_dist * (1.0 + pad) if pad else sc.max_dist)
    with np.errstate(invalid="ignore"):
        cpx = np.clip(np.floor((sc.px - g["x0"]) * g["inv_h"]), 0, g["nbx"] - 1)
        cpy = np.clip(np.floor((sc.py - g["y0"]) * g["inv_h"]), 0, g["nby"] - 1)
        ctx = np.floor((sc.tx - g["x0"]) * g["inv_h"])
        cty = np.floor((sc.ty - g["y0"]) * g["inv_h"])
    if pad:
        ctx = np.where(ctx == g["nbx"] + 1, g["nbx"], ctx)
        cty = np.where(cty == g["nby"] + 1, g["nby"], cty)
    with np.errstate(invalid="ignore"):
        seen = (np.abs(cpx[None, :] - ctx[:, None]) <= 1) & (np.abs(cpy[None, :] - cty[:, None]) <= 1)
    d2 = _d2_matrix(sc)
    d2[~seen] = np.inf
    out = _select(d2, sc.max_dist)
    out["cell_gap"] = np.stack([cpx[None, :] - ctx[:, None], cpy[None, :] - cty[:, None]])
    return out


def _ulps(v, j):
    return v + j * np.spacing(np.abs(v))


def _border_hits(rng, v0, span, h, n=60000):
    """1-D search: a target within 3 ulp of a cell border and a point less than h away that the unpadded hash puts two
    cells off.  Returns (t, p, direction) arrays of the hits, direction = sign of p - t."""
    inv_h = 1.0 / h
    nb = int(np.floor(span / h))
    k = rng.integers(3, nb - 3, size=n)
    t = _ulps(v0 + k * h, rng.integers(-3, 4, size=n))
    sgn = rng.choice([-1.0, 1.0], size=n)
    p = t + sgn * (h * (1.0 - rng.uniform(0.0, 1.0, size=n) * 6e-16 * k))
    dx = p - t
    near = np.sqrt(dx * dx + 0.0 * 0.0) < h
    gap = np.floor((p - v0) * inv_h) - np.floor((t - v0) * inv_h)
    hit = near & (np.abs(gap) == 2) & (p > v0) & (p < v0 + span)
    return t[hit], p[hit], sgn[hit]


def _border_scene(h, origin, attempt=0):
    hi, oi = MAX_DISTS.index(h), ORIGINS.index(origin)
    rng = np.random.default_rng([SEED, 1, hi, oi, attempt])
    sx, sy = 300.0, 140.0
    if origin == "random":
        x0, y0 = rng.uniform(-175.0, -120.0), rng.uniform(-88.0, -60.0)
    else:
        x0, y0 = float(origin), float(origin) + 90.0
    assert hash_grid(np.array([x0, x0 + sx]), np.array([y0, y0 + sy]), h)["cell"] == h
    hits = {"x": _border_hits(rng, x0, sx, h, n=400000), "y": _border_hits(rng, y0, sy, h, n=400000)}
    if hits["x"][0].size + hits["y"][0].size < 4:                     # (1.5 against a dyadic origin: every product is exact)
        assert origin == "random", (h, origin)
        return _border_scene(h, origin, attempt + 1)
    px, py, tx, ty, tags = [x0, x0 + sx], [y0, y0 + sy], [], [], []
    nb = {"x": int(sx / h), "y": int(sy / h)}
    org = {"x": x0, "y": y0}
    for c in range(8):                                                # x / y alternating; 4 with the point above, 4 below;
        axis = "x" if (c % 2 == 0 and hits["x"][0].size) or not hits["y"][0].size else "y"     # every other pair near both borders
        other = "y" if axis == "x" else "x"
        t, p, s = hits[axis]
        want = np.flatnonzero(s == (1.0 if c < 4 else -1.0))          # (where the rounding of 1 / h allows that direction)
        i = rng.choice(want if want.size else np.arange(s.size))
        if c % 4 < 2:
            o = org[other] + (rng.integers(3, nb[other] - 3) + rng.uniform(0.3, 0.7)) * h
        else:
            o = _ulps(org[other] + rng.integers(3, nb[other] - 3) * h, rng.integers(-3, 4))
        tc, pc = ((t[i], o), (p[i], o)) if axis == "x" else ((o, t[i]), (o, p[i]))
        tx.append(tc[0]); ty.append(tc[1]); px.append(pc[0]); py.append(pc[1])
        tags.append("border_ulp")
    sc = NNScene(f"border_ulp-{hi}-{origin}", px, py, tx, ty, h, tags)
    # the only point within reach, less than max_dist away, two cells off: else draw again
    d = np.sqrt(_d2_matrix(sc))
    old = emulate_search(sc, pad=0.0)
    ok = ((d < 3.0 * h).sum(axis=1) == 1).all() and (d.min(axis=1) < h).all() and (old["idx"] == -1).all()
    return sc if ok else _border_scene(h, origin, attempt + 1)


def _diagonal_offset(rng, want):
    """(a, b), both non-zero, with sqrt(a*a + b*b) bit-equal to `want`: found by search"""
    while True:
        b = rng.uniform(0.1, 0.9) * want
        a0 = np.sqrt(want * want - b * b)
        for j in range(-6, 7):
            a = _ulps(a0, j)
            if np.sqrt(a * a + b * b) == want:
                return a * rng.choice([-1.0, 1.0]), b * rng.choice([-1.0, 1.0])


def _at_radius_scene(hi):
    """The only point in reach exactly max_dist away (kept) or one ulp further (masked).  Axis-aligned pairs share their other
    coordinate, so p - t is exact anywhere; the diagonal pair has its target at the origin for the same reason."""
    h = MAX_DISTS[hi]
    rng = np.random.default_rng([SEED, 2, hi])
    above = np.nextafter(h, np.inf)
    px, py, tx, ty, tags = [], [], [], [], []
    for i, (want, tag) in enumerate(((h, "at_radius_kept"), (above, "at_radius_masked"))):
        for j, sgn in enumerate((1.0, -1.0)):
            c = 16.0 * (1 + 2 * i + j)
            tx.append(0.0); ty.append(c); px.append(sgn * want); py.append(c)          # along x, in row c
            tx.append(c); ty.append(0.0); px.append(c); py.append(sgn * want)          # along y, in column c
            tags += [tag, tag]
    want, tag = ((h, "at_radius_kept"), (above, "at_radius_masked"))[hi % 2]
    a, b = _diagonal_offset(rng, want)
    tx.append(0.0); ty.append(0.0); px.append(a); py.append(b); tags.append(tag)
    return NNScene(f"at_radius-{hi}", px, py, tx, ty, h, tags)


def _main_scene():
    rng = np.random.default_rng([SEED, 3])
    nx, ny, lon0, lat0, h = 40, 30, -20.0, 10.0, 1.5
    LON, LAT = np.meshgrid(lon0 + np.arange(nx), lat0 + np.arange(ny))
    px, py = list(LON.ravel()), list(LAT.ravel())
    iso = [(100.0 + 7.0 * i, -50.0 + 7.0 * j) for i in range(8) for j in range(6)]           # isolated points, 7 apart
    px += [p[0] for p in iso]; py += [p[1] for p in iso]
    nodes = rng.permutation(nx * ny)
    dup, single = nodes[:REPS], nodes[REPS:2 * REPS]
    px += [px[i] for i in dup]; py += [py[i] for i in dup]                                    # second copies: higher index
    nan_xy = []
    for i in range(REPS):                                                                     # points with a NaN coordinate
        x, y = lon0 + rng.uniform(1, nx - 2), lat0 + rng.uniform(1, ny - 2)
        nan_xy.append((x, y))
        px.append(np.nan if i % 3 != 1 else x); py.append(np.nan if i % 3 != 0 else y)
    tx, ty, tags = [], [], []

    def add(tag, x, y):
        tx.append(x); ty.append(y); tags.append(tag)

    for i in single:
        add("on_point", px[i], py[i])
    for i in dup:
        add("dup_points", px[i], py[i])
    for i in range(REPS):
        ix, iy = rng.integers(0, nx - 1), rng.integers(0, ny - 1)
        if i % 2:
            add("tie2", lon0 + ix + 0.5, lat0 + iy)
        else:
            add("tie2", lon0 + ix, lat0 + iy + 0.5)
        add("tie4", lon0 + rng.integers(0, nx - 1) + 0.5, lat0 + rng.integers(0, ny - 1) + 0.5)
        delta = (2e-10, 1e-9, 1e-8, 1e-6)[i % 4] * (1 if i % 8 < 4 else -1)
        add("near_tie", lon0 + rng.integers(0, nx - 1) + 0.5 + delta, lat0 + rng.integers(0, ny))
        add("nan_point", *nan_xy[i])
        add("nan_target", np.nan if i % 3 != 1 else 3.3, np.nan if i % 3 != 0 else 17.7)
        add("generic", rng.uniform(-24.0, 24.0), rng.uniform(6.0, 43.0))
    xmin, xmax, ymin, ymax = -20.0, 149.0, -50.0, 39.0                                        # the box of the finite points
    for i in range(6):
        off = (0.3, 0.9, 1.4, 2.0, 40.0, 1000.0)[i]                                           # three within reach, three beyond
        add("outside_box", xmin - off, lat0 + 5.0 + 0.3 * i)
        add("outside_box", xmax + off, -50.0 + 7.0 * (i % 6) + 0.2)
        add("outside_box", 100.0 + 7.0 * i + 0.2, ymin - off)
        add("outside_box", lon0 + 3.0 * i + 0.2, ymax + off)
    return NNScene("main", px, py, tx, ty, h, tags)


def _small_scene(name):
    rng = np.random.default_rng([SEED, 4, ("one_point", "collinear", "all_nan_points").index(name)])
    h = 0.7
    ang = rng.uniform(0, 2 * np.pi, size=REPS)
    rad = np.where(np.arange(REPS) % 2 == 0, rng.uniform(0.0, 0.69, size=REPS), rng.uniform(0.71, 5.0, size=REPS))
    if name == "one_point":
        px, py = [12.5], [-33.25]
        tx, ty = px[0] + rad * np.cos(ang), py[0] + rad * np.sin(ang)
        tx[0], ty[0] = px[0], py[0]
    elif name == "collinear":
        px = -10.0 + 0.4 * np.arange(50) + rng.uniform(-0.1, 0.1, size=50)
        py = np.full(50, 21.0)
        tx = rng.uniform(-12.0, 11.0, size=REPS)
        ty = 21.0 + rad * np.where(np.arange(REPS) % 4 < 2, 1.0, -1.0)
        ty[:2] = 21.0
    else:
        px, py = [np.nan] * 5, [np.nan, 1.0, np.nan, 2.0, np.nan]
        px[1] = np.nan
        tx, ty = rng.uniform(-5, 5, size=REPS), rng.uniform(-5, 5, size=REPS)
        tx[0], ty[0] = 0.0, 0.0
    return NNScene(name, px, py, tx, ty, h, [name] * REPS)


def _coarsened_scene(name):
    """a whole globe of points against a radius of a thousandth of a degree: the cell doubles seven times and the counters
    fill about a thousand scan tiles"""
    h = {"coarsened": 1e-3, "coarsened_1000": 9.75e-4}[name]
    rng = np.random.default_rng([SEED, 5, int(name != "coarsened")])
    n = 1500
    px = np.concatenate([[-180.0, 180.0], rng.uniform(-180.0, 180.0, size=n)])
    py = np.concatenate([[-90.0, 90.0], rng.uniform(-90.0, 90.0, size=n)])
    near = rng.choice(n, size=2 * REPS, replace=False) + 2
    ang = rng.uniform(0, 2 * np.pi, size=2 * REPS)
    rad = np.where(np.arange(2 * REPS) % 2 == 0, rng.uniform(0.05, 0.95, size=2 * REPS), rng.uniform(1.05, 3.0, size=2 * REPS)) * h
    tx = np.concatenate([px[near] + rad * np.cos(ang), [-180.0, 180.0, 0.0]])
    ty = np.concatenate([py[near] + rad * np.sin(ang), [-90.0, 90.0, 0.0]])
    return NNScene(name, px, py, tx, ty, h, [name] * tx.size)


def _tiles_scene(name):
    """ncell just above one and just above two scan tiles"""
    sx, sy = {"tiles2-4096": (64.5, 63.5), "tiles2-8192": (90.5, 90.5)}[name]
    rng = np.random.default_rng([SEED, 6, int(sx)])
    n = 1500
    px = np.concatenate([[3.0, 3.0 + sx], 3.0 + rng.uniform(0, sx, size=n)])
    py = np.concatenate([[-7.0, -7.0 + sy], -7.0 + rng.uniform(0, sy, size=n)])
    tx = np.concatenate([3.0 + rng.uniform(-1.5, sx + 1.5, size=2 * REPS - 4), [3.0 + sx - 0.01, 3.0 + sx + 0.3, 3.0, 3.0 + sx - 0.2]])
    ty = np.concatenate([-7.0 + rng.uniform(-1.5, sy + 1.5, size=2 * REPS - 4), [-7.0 + sy - 0.01, -7.0 + sy + 0.3, -7.0, -7.0 + sy + 0.8]])
    return NNScene(name, px, py, tx, ty, 1.0, ["tiles2"] * tx.size)


@functools.lru_cache(maxsize=None)
def nn_scene_names():
    return tuple(["main", "one_point", "collinear", "all_nan_points", "coarsened", "coarsened_1000", "tiles2-4096", "tiles2-8192"]
                 + [f"at_radius-{i}" for i in range(len(MAX_DISTS))]
                 + [f"border_ulp-{i}-{o}" for i in range(len(MAX_DISTS)) for o in ORIGINS if (i, o) not in BORDER_EXACT])


@functools.lru_cache(maxsize=None)
def nn_scene(name):
    if name == "main":
        return _main_scene()
    if name in ("one_point", "collinear", "all_nan_points"):
        return _small_scene(name)
    if name.startswith("coarsened"):
        return _coarsened_scene(name)
    if name.startswith("tiles2"):
        return _tiles_scene(name)
    if name.startswith("at_radius"):
        return _at_radius_scene(int(name.split("-")[1]))
    _, hi, origin = name.split("-", 2)
    return _border_scene(MAX_DISTS[int(hi)], origin)


# ---------------------------------------------------------------------------------------------------------------------
# B. box filter, pick, element-wise
# ---------------------------------------------------------------------------------------------------------------------
BOX_WINDOWS = ((1, 1), (1, 2), (2, 1), (1, 3), (3, 3), (4, 4), (2, 5), (9, 7), (16, 21), (17, 32), (3, 33), (1, 64), (8, 64),
               (1, 65), (2, 70))
# (Ny, Nx, ky, kx): grids narrower than the window -- the reflection is applied more than once
BOX_NARROW = ((2, 9, 7, 3), (5, 3, 2, 64))
BOX_WRAP = (40, 50, 1, 64, 3, 12000)       # Ny, Nx, ky, kx, nfields, Tn: 36,000 waves against a grid of 32,768
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
PRIME_TN = 257


def box_shape(ky, kx):
    return max(13, 3 * ky + 1), max(17, 3 * kx + 5)


@functools.lru_cache(maxsize=None)
def box_fields(Ny, Nx, dtype, specials=True):
    """three fields [3, Ny, Nx]: plain; the same with NaN, +inf and a (+inf, -inf) pair in three corners; six decades of
    magnitude and both signs"""
    rng = np.random.default_rng([SEED, 10, Ny, Nx])
    Z = np.empty((3, Ny, Nx), dtype=np.float64)
    Z[0] = rng.normal(size=(Ny, Nx)) + 0.3
    Z[1] = Z[0]
    Z[2] = rng.normal(size=(Ny, Nx)) * 10.0 ** rng.uniform(-3, 3, size=(Ny, Nx))
    if specials:
        Z[1, 1, 1] = np.nan
        Z[1, 1, Nx - 2] = np.inf
        Z[1, Ny - 2, 1], Z[1, Ny - 2, 2] = np.inf, -np.inf
    Z = Z.astype(dtype)
    Z.setflags(write=False)
    return Z


def box_reference(Z2, ky, kx, variance):
    """(ref, bar): convolve2d in float64 on the values as stored, and (win + 2) u sum|Z w| over each window"""
    Z64 = np.asarray(Z2, dtype=np.float64)
    kk = float(kx) * float(ky)
    w = 1.0 / (kk * kk) if variance else 1.0 / kk
    ker = np.full((ky, kx), w)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = convolve2d(Z64, ker, boundary="symm", mode="same")
        mag = convolve2d(np.where(np.isfinite(Z64), np.abs(Z64), 0.0), ker, boundary="symm", mode="same")
    return ref, (ky * kx + 2) * UNIT[np.dtype(Z2.dtype)] * mag


def box_direct(Z2, ky, kx, w):
    """the window sum written out (repeated reflection), for the CPU test of the reference's alignment"""
    Ny, Nx = Z2.shape

    def refl(i, n):
        while i < 0 or i >= n:
            i = -i - 1 if i < 0 else 2 * n - 1 - i
        return i

    out = np.zeros((Ny, Nx))
    with np.errstate(invalid="ignore"):
        for i in range(Ny):
            for j in range(Nx):
                out[i, j] = sum(float(Z2[refl(i - ky // 2 + a, Ny), refl(j - kx // 2 + b, Nx)]) * w for a in range(ky) for b in range(kx))
    return out


def pick_tns(kx):
    """target counts around the row-wise kernel's targets-per-wave, plus one and a prime"""
    tpw = 64 // kx if kx <= 64 else 1
    return sorted({t for t in (1, tpw - 1, tpw + 1, PRIME_TN) if t > 0})


def pick_idx(Ny, Nx, Tn):
    """corner and edge nodes, -1 entries, repeated nodes, then random ones"""
    rng = np.random.default_rng([SEED, 11, Ny, Nx, Tn])
    n = Ny * Nx
    head = [n - 1, -1, 0, Nx - 1, (Ny - 1) * Nx, Nx // 2, (Ny // 2) * Nx, n - 1, -1, (Ny // 2) * Nx + Nx - 1, n - Nx // 2 - 1, 0]
    idx = np.concatenate([head, rng.integers(-1, n, size=max(Tn - len(head), 0))])[:Tn]
    return idx.astype(np.int32)


def compare_bar(got, ref, bar):
    """NaN pattern, inf pattern with sign, |got - ref| <= bar on the rest.  Returns (failing indices, largest ratio)."""
    got, ref, bar = (np.asarray(a, dtype=np.float64).ravel() for a in (got, ref, np.broadcast_to(bar, np.shape(ref))))
    nan, inf = np.isnan(ref), np.isinf(ref)
    fin = ~(nan | inf)
    bad = (np.isnan(got) != nan) | (np.isinf(got) != inf)
    bad[inf] |= got[inf] != ref[inf]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        ok = fin & ~bad
        bad[ok] |= err[ok] > bar[ok]
        ratio = np.where(ok & (bar > 0), err / np.where(bar > 0, bar, 1.0), 0.0)
        ratio[ok & (bar == 0) & (err > 0)] = np.inf
    return [int(i) for i in np.flatnonzero(bad)], float(ratio.max()) if ratio.size else 0.0


def elementwise_inputs(n, dtype, seed):
    """two arrays of dtype with NaN, +-inf, +-0, tiny, huge and negative values sprinkled in"""
    rng = np.random.default_rng([SEED, 12, seed, n])
    fi = np.finfo(dtype)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny, -fi.tiny, fi.max, -fi.max, 1e-30, -4.0, 9.0], dtype=dtype)
    out = []
    for lo, hi in ((-2.0, 9.0e3), (-1.0, 4.0e2)):
        a = rng.uniform(lo, hi, size=n).astype(dtype)
        hit = rng.uniform(size=n) < 0.25
        a[hit] = specials[rng.integers(0, specials.size, size=int(hit.sum()))]
        out.append(a)
    k = min(n, specials.size)
    out[0][:k], out[1][:k] = specials[:k], specials[:k]              # 0/0, inf/inf, nan/nan, x/x ...
    if n > 2 * specials.size:
        out[0][k:2 * k], out[1][k:2 * k] = np.dtype(dtype).type(3.5), specials[:k]  # x/0, x/inf, x/nan ...
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. thin-plate-spline RBF on K neighbours
# ---------------------------------------------------------------------------------------------------------------------
RBF_KS = (3, 4, 5)
COND_MAX = 1e6
# Largest |A - B| / sum|w_q v_q| over every scene, K and value field (reference A: np.linalg.solve; reference B: the kernel's
# elimination in NumPy), measured on the CPU by tests/test_horizontal_cases_cpu.py (5.16e-13, the far target of the clustered
# scene with K = 5; every other scene stays below 3e-14), which asserts it again.
RBF_AB_CPU = 5.2e-13
# The bar of the issue: 8 times that (the order of the back-substitution sums), never below 1e-12.
RBF_TOL = max(8.0 * RBF_AB_CPU, 1e-12)
# Largest |device - A| / sum|w_q v_q| measured on an MI355X over the same catalogue (float64 fields): the same target, and
# the same figure as reference B to three digits; every other scene stayed below 4e-14.
RBF_DEVICE_MEASURED = 5.159e-13


class RBFScene:
    def __init__(self, name, K, px, py, tx, ty, nn_idx, cell, tags):
        self.name, self.K, self.cell, self.tags = name, K, float(cell), list(tags)
        self.px, self.py, self.tx, self.ty = (np.ascontiguousarray(a, dtype=np.float64) for a in (px, py, tx, ty))
        self.nn_idx = np.ascontiguousarray(nn_idx, dtype=np.int32)
        assert self.P <= 64 and self.tx.shape == self.ty.shape == self.nn_idx.shape == (len(self.tags),)

    @property
    def P(self):
        return self.px.size

    @property
    def T(self):
        return self.tx.size

    def where(self, tag):
        return np.array([i for i, t in enumerate(self.tags) if t == tag], dtype=np.int64)

    def values(self, dtype):
        """[P + 3, P]: P one-hot fields (out[f][t] = the weight of point f), two random fields, one with a NaN"""
        rng = np.random.default_rng([SEED, 20, self.P])
        v = np.concatenate([np.eye(self.P), rng.normal(size=(3, self.P)) * np.array([[1.0], [300.0], [1.0]])])
        v[self.P + 2, self.P // 3] = np.nan
        return np.ascontiguousarray(v.astype(dtype))


def _tps(r2):
    r = np.sqrt(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r == 0.0, 0.0, (r * r) * np.log(r))


def knn_brute(px, py, x, y, K):
    """(ids of the K nearest by (d2, index), is the K-th tied with the runner-up)"""
    dx, dy = px - x, py - y
    d2 = dx * dx + dy * dy
    order = np.lexsort((np.arange(px.size), d2))
    tie = px.size > K and d2[order[K]] == d2[order[K - 1]]
    return order[:K], bool(tie)


def rbf_system(px, py, ids, x, y):
    """the (K+3) x (K+3) matrix and the evaluation vector as csrc/regrid.hip documents them; ids ascending"""
    ids = np.sort(np.asarray(ids))
    K = ids.size
    yx, yy = px[ids], py[ids]
    shx, shy = (yx.max() + yx.min()) / 2, (yy.max() + yy.min()) / 2
    scx, scy = (yx.max() - yx.min()) / 2, (yy.max() - yy.min()) / 2
    scx, scy = (scx if scx != 0.0 else 1.0), (scy if scy != 0.0 else 1.0)
    A = np.zeros((K + 3, K + 3))
    ddx, ddy = yx[:, None] - yx[None, :], yy[:, None] - yy[None, :]
    A[:K, :K] = _tps(ddx * ddx + ddy * ddy)
    A[np.arange(K), np.arange(K)] = 0.0
    A[:K, K], A[:K, K + 1], A[:K, K + 2] = 1.0, (yx - shx) / scx, (yy - shy) / scy
    A[K:, :K] = A[:K, K:].T
    tdx, tdy = x - yx, y - yy
    vec = np.concatenate([_tps(tdx * tdx + tdy * tdy), [1.0, (x - shx) / scx, (y - shy) / scy]])
    return A, vec, ids


def solve_b(A, vec):
    """reference B: rbf_factor's elimination -- partial pivoting on the first largest |.|, multipliers as products with the
    pivot's reciprocal, the right-hand side carried along, back substitution left to right.  Returns (w, zero pivot met)."""
    N = vec.size
    a = np.concatenate([A, vec[:, None]], axis=1)
    singular = False
    with np.errstate(all="ignore"):
        for k in range(N):
            p = k + int(np.argmax(np.abs(a[k:, k])))
            if not np.abs(a[p, k]) > 0.0:
                singular = True
                p = k
            if p != k:
                a[[k, p]] = a[[p, k]]
            inv = 1.0 / a[k, k]
            for i in range(k + 1, N):
                a[i, k + 1:] -= (a[i, k] * inv) * a[k, k + 1:]
        w = np.zeros(N)
        for i in range(N - 1, -1, -1):
            s = a[i, N]
            for j in range(i + 1, N):
                s -= a[i, j] * w[j]
            w[i] = s / a[i, i]
    return w, singular


def axis_collinear(px, py, ids):
    """all neighbours on one row or one column: a column of the polynomial block is exactly zero, so is a pivot"""
    return np.ptp(px[ids]) == 0.0 or np.ptp(py[ids]) == 0.0


def rbf_target(px, py, x, y, K, ids=None):
    """everything the references say about one target: neighbours, tie, zero pivot, weights A and B, condition number"""
    tie = False
    if ids is None:
        ids, tie = knn_brute(px, py, x, y, K)
    A, vec, ids = rbf_system(px, py, ids, x, y)
    wb, singular = solve_b(A, vec)
    with np.errstate(all="ignore"):
        cond = np.inf if singular else np.linalg.cond(A, 1)
    wa = None
    if not singular:
        wa = np.linalg.solve(A, vec)
    return {"ids": ids, "tie": tie, "singular": singular, "wa": None if wa is None else wa[:K], "wb": wb[:K], "cond": cond,
            "collinear": axis_collinear(px, py, ids)}


def _judgeable(px, py, x, y, K, allow_tie=False, allow_row=False):
    """a target the references can judge: untied (unless allowed), and either well conditioned or singular for a reason that
    does not depend on rounding (a row or a column of points)"""
    r = rbf_target(px, py, x, y, K)
    if r["tie"] and not allow_tie:
        return False
    if r["collinear"]:
        return allow_row and r["singular"]
    return not r["singular"] and r["cond"] <= COND_MAX


def _nn_of(px, py, tx, ty, cell, mask=True):
    d2 = (px[None, :] - np.asarray(tx)[:, None]) ** 2 + (py[None, :] - np.asarray(ty)[:, None]) ** 2
    nn = np.argmin(d2, axis=1)
    if mask:
        nn = np.where(np.sqrt(d2.min(axis=1)) > cell, -1, nn)
    return nn.astype(np.int32)


def _draw(rng, n, gen, ok):
    out = []
    while len(out) < n:
        c = gen(rng)
        if ok(*c):
            out.append(c)
    return out


def _rbf_generic(K):
    rng = np.random.default_rng([SEED, 21, K])
    P, cell = 48, 2.0
    px, py = rng.uniform(0.0, 10.0, size=P), rng.uniform(0.0, 8.0, size=P)
    ok = lambda x, y: _judgeable(px, py, x, y, K)
    cats = [("generic", REPS, lambda r: (r.uniform(0.5, 9.5), r.uniform(0.5, 7.5))),
            ("outside_left", 6, lambda r: (px.min() - r.uniform(0.1, 1.2), r.uniform(1.0, 7.0))),
            ("outside_right", 6, lambda r: (px.max() + r.uniform(0.1, 1.2), r.uniform(1.0, 7.0))),
            ("outside_below", 6, lambda r: (r.uniform(1.0, 9.0), py.min() - r.uniform(0.1, 1.2))),
            ("outside_above", 6, lambda r: (r.uniform(1.0, 9.0), py.max() + r.uniform(0.1, 1.2))),
            ("masked_far", 12, lambda r: (r.choice([-1.0, 1.0]) * r.uniform(14.0, 60.0), r.choice([-1.0, 1.0]) * r.uniform(12.0, 60.0))),
            ("nn_minus1", 12, lambda r: (r.uniform(0.5, 9.5), r.uniform(0.5, 7.5)))]
    tx, ty, tags = [], [], []
    for tag, n, gen in cats:
        for x, y in _draw(rng, n, gen, ok):
            tx.append(x); ty.append(y); tags.append(tag)
    for i in rng.choice(P, size=12, replace=False):
        if ok(px[i], py[i]):
            tx.append(px[i]); ty.append(py[i]); tags.append("on_point")
    nan_at = P // 3                                                        # RBFScene.values puts the NaN there
    for x, y in _draw(rng, 12, lambda r: (px[nan_at] + r.uniform(-0.6, 0.6), py[nan_at] + r.uniform(-0.6, 0.6)), ok):
        tx.append(x); ty.append(y); tags.append("nan_value")
    nn = _nn_of(px, py, tx, ty, cell)
    nn[[i for i, t in enumerate(tags) if t == "nn_minus1"]] = -1
    assert (nn[[i for i, t in enumerate(tags) if t == "masked_far"]] == -1).all()
    return RBFScene(f"generic-K{K}", K, px, py, tx, ty, nn, cell, tags)


def _rbf_cluster(K):
    """30 points in a unit square, 6 more thirty units away, cells of 0.05: the far target's rings are empty for hundreds
    of rounds"""
    rng = np.random.default_rng([SEED, 22, K])
    while True:
        px = np.concatenate([rng.uniform(0.0, 1.0, size=30), rng.uniform(30.0, 31.0, size=6)])
        py = np.concatenate([rng.uniform(0.0, 1.0, size=30), rng.uniform(30.0, 31.0, size=6)])
        far = [(15.3, 14.1), (-9.0, 0.4), (31.5, -7.0)]
        if all(_judgeable(px, py, x, y, K) for x, y in far):
            break
    near = _draw(rng, 12, lambda r: (r.uniform(0.05, 0.95), r.uniform(0.05, 0.95)), lambda x, y: _judgeable(px, py, x, y, K))
    tx, ty = [p[0] for p in far + near], [p[1] for p in far + near]
    return RBFScene(f"cluster-K{K}", K, px, py, tx, ty, _nn_of(px, py, tx, ty, 0.05, mask=False), 0.05, ["far_target"] * 3 + ["cluster"] * 12)


def _rbf_p_equals_k(K):
    rng = np.random.default_rng([SEED, 23, K])
    px, py = rng.uniform(0.0, 3.0, size=K), rng.uniform(0.0, 3.0, size=K)
    t = _draw(rng, 12, lambda r: (r.uniform(-0.5, 3.5), r.uniform(-0.5, 3.5)), lambda x, y: _judgeable(px, py, x, y, K))
    tx, ty = [p[0] for p in t], [p[1] for p in t]
    return RBFScene(f"p_equals_k-K{K}", K, px, py, tx, ty, _nn_of(px, py, tx, ty, 1.0, mask=False), 1.0, ["p_equals_k"] * 12)


def _rbf_lattice(K, dy=1.0, name="lattice"):
    """a 6 x 6 lattice: targets on nodes, edge midpoints and cell centres tie wholesale; targets beyond the edge are masked
    and some of their neighbourhoods are one row or one column of the lattice.  With rows three units apart (lattice_wide) the
    nearest five of a target near a row are that row's, the fifth tied: zero pivots that are ties' and not to be counted."""
    rng = np.random.default_rng([SEED, 24, K, int(dy)])
    n, cell = 6, 1.5
    LX, LY = np.meshgrid(np.arange(float(n)), dy * np.arange(float(n)))
    px, py = LX.ravel(), LY.ravel()
    ok = lambda x, y: _judgeable(px, py, x, y, K, allow_tie=True, allow_row=True)
    cand = {"node": [(float(i), float(j)) for i in range(n) for j in range(n)],
            "edge_mid": [(i + 0.5, float(j)) for i in range(n - 1) for j in range(n)] + [(float(i), j + 0.5) for i in range(n) for j in range(n - 1)],
            "centre": [(i + 0.5, j + 0.5) for i in range(n - 1) for j in range(n - 1)],
            "lattice_generic": [(rng.uniform(-0.9, n - 0.1), rng.uniform(-0.9, n - 0.1)) for _ in range(60)],
            "masked_beyond": [(-3.0, 2.0), (-3.0, 2.5), (8.5, 3.0), (2.0, -4.0), (3.5, 9.0), (-2.5, 1.0), (9.0, 0.0), (0.0, 8.0), (5.0, -3.0)]
                             + [(rng.uniform(-6.0, -2.0), rng.uniform(0.0, 5.0)) for _ in range(8)]
                             + [(rng.uniform(0.0, 5.0), rng.uniform(7.0, 11.0)) for _ in range(8)]
                             + [(rng.uniform(-4.0, -1.2), rng.uniform(-4.0, -1.2)) for _ in range(8)]          # off a corner: no row
                             + [(rng.uniform(6.2, 9.0), rng.uniform(6.2, 9.0)) for _ in range(8)]}
    cand["near_row"] = [(i + 0.5, j + rng.uniform(-0.2, 0.2)) for i in range(-1, n) for j in range(n)]
    tx, ty, tags = [], [], []
    for tag, pts in cand.items():
        pts = [(pts[i][0], pts[i][1] * (1.0 if tag == "masked_beyond" else dy)) for i in rng.permutation(len(pts))]
        if tag == "masked_beyond":
            pts = [p for p in pts if _nn_of(px, py, [p[0]], [p[1]], cell)[0] == -1]
        for x, y in [p for p in pts if ok(*p)][:REPS]:
            tx.append(x); ty.append(y); tags.append(tag)
    nn = _nn_of(px, py, tx, ty, cell)
    return RBFScene(f"{name}-K{K}", K, px, py, tx, ty, nn, cell, tags)


def _rbf_row(K):
    """five points on one lattice row: the y column of every system is exactly zero"""
    rng = np.random.default_rng([SEED, 25, K])
    px, py = np.arange(5.0), np.full(5, 2.0)
    t = _draw(rng, 12, lambda r: (r.uniform(-0.4, 4.4), 2.0 + r.choice([0.0, 1.0]) * r.uniform(-1.0, 1.0)),
              lambda x, y: not knn_brute(px, py, x, y, K)[1])
    tx, ty = [p[0] for p in t], [p[1] for p in t]
    return RBFScene(f"row-K{K}", K, px, py, tx, ty, _nn_of(px, py, tx, ty, 1.5), 1.5, ["row"] * 12)


RBF_KINDS = {"generic": _rbf_generic, "cluster": _rbf_cluster, "p_equals_k": _rbf_p_equals_k, "lattice": _rbf_lattice,
             "lattice_wide": lambda K: _rbf_lattice(K, 3.0, "lattice_wide"), "row": _rbf_row}


@functools.lru_cache(maxsize=None)
def rbf_scene(kind, K):
    return RBF_KINDS[kind](K)


@functools.lru_cache(maxsize=None)
def rbf_reference(kind, K):
    """per target: ok (evaluated at all), ids, tie, singular (reference B's zero pivot), W_a / W_b [T, P] evaluation weights
    scattered to the points (0 elsewhere), cond"""
    sc = rbf_scene(kind, K)
    T, P = sc.T, sc.P
    out = {"ok": sc.nn_idx >= 0, "tie": np.zeros(T, bool), "singular": np.zeros(T, bool), "collinear": np.zeros(T, bool),
           "cond": np.zeros(T), "ids": np.zeros((T, K), np.int64), "Wa": np.zeros((T, P)), "Wb": np.zeros((T, P)),
           "nbr": np.zeros((T, P), bool)}
    for t in range(T):
        r = rbf_target(sc.px, sc.py, sc.tx[t], sc.ty[t], K)
        out["tie"][t], out["singular"][t], out["cond"][t], out["ids"][t], out["collinear"][t] = r["tie"], r["singular"], r["cond"], r["ids"], r["collinear"]
        out["nbr"][t, r["ids"]] = True
        out["Wb"][t, r["ids"]] = r["wb"]
        out["Wa"][t, r["ids"]] = r["wa"] if r["wa"] is not None else np.nan
    return out


def rbf_expected(W, nbr, ok, singular, values):
    """(out [nf, T], scale [nf, T]) in float64 from evaluation weights: NaN for targets not evaluated or singular; a NaN
    value poisons exactly the neighbourhoods that hold it"""
    v = np.asarray(values, dtype=np.float64)
    nf, T = v.shape[0], W.shape[0]
    out, scale = np.full((nf, T), np.nan), np.zeros((nf, T))
    with np.errstate(invalid="ignore"):
        for t in np.flatnonzero(ok & ~singular):
            q = np.flatnonzero(nbr[t])
            terms = W[t, q][None, :] * v[:, q]
            out[:, t] = terms.sum(axis=1)
            scale[:, t] = np.abs(terms).sum(axis=1)
    return out, scale


# ---------------------------------------------------------------------------------------------------------------------
# D. Delaunay linear interpolation
# ---------------------------------------------------------------------------------------------------------------------
RT64 = 1e-12                               # the project's float64 bar (tests/test_gpu_parity.py)
EPS = 100.0 * np.finfo(np.float64).eps     # scipy's point-location tolerance


class LinScene:
    def __init__(self, name, pts, tx, ty, tags):
        self.name, self.tags = name, list(tags)
        self.pts = np.ascontiguousarray(pts, dtype=np.float64)
        self.tri = Delaunay(self.pts)
        self.tx, self.ty = (np.ascontiguousarray(a, dtype=np.float64) for a in (tx, ty))
        d2 = (self.pts[None, :, 0] - self.tx[:, None]) ** 2 + (self.pts[None, :, 1] - self.ty[:, None]) ** 2
        self.nn_idx = np.argmin(d2, axis=1).astype(np.int32)
        self.nn_idx[self.where("nn_minus1")] = -1
        assert self.tx.shape == self.ty.shape == (len(self.tags),)

    P = property(lambda self: self.pts.shape[0])
    T = property(lambda self: self.tx.size)
    ns = property(lambda self: self.tri.nsimplex)

    def where(self, tag):
        return np.array([i for i, t in enumerate(self.tags) if t == tag], dtype=np.int64)

    def arrays(self):
        """what the C ABI takes: simplices, neighbors, transform [ns][6], vertex_to_simplex, bounds"""
        t = self.tri
        return {"simplices": np.ascontiguousarray(t.simplices, dtype=np.int32), "neighbors": np.ascontiguousarray(t.neighbors, dtype=np.int32),
                "transform": np.ascontiguousarray(t.transform.reshape(self.ns, 6)), "v2s": np.ascontiguousarray(t.vertex_to_simplex, dtype=np.int32),
                "bounds": np.array([t.min_bound[0], t.max_bound[0], t.min_bound[1], t.max_bound[1]])}

    def values(self, dtype):
        """[3, P]: smooth, rough with six decades, and the smooth one with a NaN at vertex `nan_vertex`"""
        rng = np.random.default_rng([SEED, 30, self.P])
        v = np.stack([1.0 + np.sin(self.pts[:, 0]) * np.cos(self.pts[:, 1] / 3.0),
                      rng.normal(size=self.P) * 10.0 ** rng.uniform(-3, 3, size=self.P), np.zeros(self.P)])
        v[2] = v[0]
        v[2, self.nan_vertex] = np.nan
        return np.ascontiguousarray(v.astype(dtype))

    @property
    def nan_vertex(self):
        g = self.where("generic")
        s = self.tri.find_simplex(np.column_stack([self.tx[g], self.ty[g]]))
        return int(self.tri.simplices[s[0], 0])


def barycentric(tri, s, x, y):
    """scipy's coordinates of (x, y) in simplex s, same order of operations as the kernel: c0, c1, 1 - c0 - c1"""
    tr = tri.transform[s]
    dx, dy = x - tr[:, 2, 0], y - tr[:, 2, 1]
    c0 = tr[:, 0, 0] * dx + tr[:, 0, 1] * dy
    c1 = tr[:, 1, 0] * dx + tr[:, 1, 1] * dy
    return np.stack([c0, c1, 1.0 - c0 - c1], axis=1)


def linear_in_simplex(tri, s, x, y, values):
    """(value [nf, n], scale [nf, n]) of the linear interpolant of simplex s, evaluated wherever (x, y) lies; NaN for s
    outside [0, nsimplex)"""
    s = np.asarray(s)
    v = np.asarray(values, dtype=np.float64)
    good = (s >= 0) & (s < tri.nsimplex)
    sg = np.where(good, s, 0)
    c = barycentric(tri, sg, np.asarray(x), np.asarray(y))
    vv = v[:, tri.simplices[sg]]                                          # [nf, n, 3]
    with np.errstate(invalid="ignore"):
        terms = c[None, :, :] * vv
        out = terms[:, :, 0] + terms[:, :, 1] + terms[:, :, 2]
        scale = np.abs(terms).sum(axis=2)
    out[:, ~good] = np.nan
    return out, scale


def accepting_simplices(tri, x, y):
    """every simplex with a valid transform that holds (x, y) to within scipy's eps"""
    ns = tri.nsimplex
    c = barycentric(tri, np.arange(ns), np.full(ns, x), np.full(ns, y))
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(((c >= -EPS) & (c <= 1.0 + EPS)).all(axis=1))


def _interior_targets(rng, tri, n):
    """barycentric combinations with every weight >= 0.05 of simplices with a valid transform"""
    good = np.flatnonzero(~np.isnan(tri.transform[:, 0, 0]))
    pts = tri.points
    out = []
    for s in rng.choice(good, size=n):
        w = 0.05 + 0.85 * rng.dirichlet(np.ones(3))
        out.append(w @ pts[tri.simplices[s]])
    return out


def _lin_targets(rng, pts, with_facets=True):
    tri = Delaunay(pts)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    tx, ty, tags = [], [], []

    def add(tag, p):
        tx.append(float(p[0])); ty.append(float(p[1])); tags.append(tag)

    for p in _interior_targets(rng, tri, 2 * REPS):
        add("generic", p)
    for p in _interior_targets(rng, tri, 12):
        add("nn_minus1", p)
    for i in range(REPS):                                                  # outside the hull: beyond the box on each side ...
        side, off = i % 4, rng.uniform(0.02, 3.0)
        u = lo + rng.uniform(0.1, 0.9, size=2) * (hi - lo)
        add("outside", [(lo[0] - off, u[1]), (hi[0] + off, u[1]), (u[0], lo[1] - off), (u[0], hi[1] + off)][side])
    if with_facets:                                                        # ... and just beyond a hull facet, inside the box or not
        hull = np.argwhere(tri.neighbors == -1)
        for s, k in hull[rng.choice(len(hull), size=min(12, len(hull)), replace=False)]:
            a, b = pts[np.delete(tri.simplices[s], k)]
            opp = pts[tri.simplices[s, k]]
            mid = (a + b) / 2
            add("outside", mid + 0.05 * (mid - opp) / np.linalg.norm(mid - opp))
    on_hull = np.unique(tri.convex_hull)
    inner = np.setdiff1d(np.arange(len(pts)), on_hull)
    for v in rng.choice(inner, size=min(REPS, len(inner)), replace=False):
        add("on_vertex", pts[v])
    pairs = np.argwhere(tri.neighbors >= 0)                                # facet k of simplex s is shared with a neighbour
    done = 0
    for s, k in pairs[rng.permutation(len(pairs))]:
        nb = tri.neighbors[s, k]
        if np.isnan(tri.transform[s, 0, 0]) or np.isnan(tri.transform[nb, 0, 0]):
            continue
        a, b = pts[np.delete(tri.simplices[s], k)]
        add("on_edge", (a + b) / 2)
        done += 1
        if done == REPS:
            break
    return tx, ty, tags


@functools.lru_cache(maxsize=None)
def linear_scene(name):
    if name.startswith("scatter"):
        P = int(name[7:])
        rng = np.random.default_rng([SEED, 31, P])
        pts = np.column_stack([rng.uniform(0.0, 10.0, size=P), rng.uniform(-4.0, 4.0, size=P)])
        return LinScene(name, pts, *_lin_targets(rng, pts))
    assert name == "swath_grid"
    # an exactly regular pixel lattice whose latitudes carry 1e-13 deg of noise: qhull closes the hull with zero-area slivers,
    # whose transforms scipy marks NaN
    rng = np.random.default_rng([SEED, 32])
    LON, LAT = np.meshgrid(np.arange(0.0, 4.0, 0.25), np.arange(10.0, 13.0, 0.25))
    pts = np.column_stack([LON.ravel(), LAT.ravel() + 1e-13 * rng.normal(size=LON.size)])
    tx, ty, tags = _lin_targets(rng, pts, with_facets=False)
    for x in np.arange(0.0, 3.76, 0.125):                                  # along the hull's straight edges and the pixel rows
        for y, tag in ((10.0, "hull_row"), (12.75, "hull_row"), (11.0, "pixel_row")):
            tx.append(float(x)); ty.append(y); tags.append(tag)
    for y in np.arange(10.0, 12.76, 0.125):
        for x in (0.0, 3.75):
            tx.append(x); ty.append(float(y)); tags.append("hull_row")
    return LinScene(name, pts, tx, ty, tags)


LINEAR_SCENES = ("scatter30", "scatter150", "scatter300", "swath_grid")


@functools.lru_cache(maxsize=None)
def rbf_forced_case(K):
    """The lattice's tied targets whose neighbourhood as scipy's own tree names it can be judged (not singular, condition
    number within COND_MAX): (target ids, neighbour ids [n, K], evaluation weights [n, P])."""
    from scipy.spatial import KDTree
    sc, r = rbf_scene("lattice", K), rbf_reference("lattice", K)
    cand = np.flatnonzero(r["ok"] & r["tie"])
    _, ids = KDTree(np.column_stack([sc.px, sc.py])).query(np.column_stack([sc.tx[cand], sc.ty[cand]]), K)
    keep, W = [], []
    for n, t in enumerate(cand):
        q = rbf_target(sc.px, sc.py, sc.tx[t], sc.ty[t], K, ids=ids[n])
        if not q["singular"] and q["cond"] <= COND_MAX:
            w = np.zeros(sc.P)
            w[q["ids"]] = q["wa"]
            keep.append(n); W.append(w)
    return cand[keep].astype(np.int32), ids[keep].astype(np.int32), np.array(W)


# The documented point location of oisat_linear_interp, restated: scipy's directed walk started at a simplex incident to the
# target's nearest point, the brute-force scan as its fall-back, and the report of targets a second simplex accepts too.
# For a target within rounding of the hull of a triangulation that is not a partition there (zero-area slivers along a
# straight swath edge) scipy's own answer depends on the simplex its previous target ended in; this one does not.
EPS_BROAD = 1.4901161193847656e-08


def _scan_locate(tri, x, y, bounds):
    """qhull._find_simplex_bruteforce"""
    tr, nb = tri.transform.reshape(-1, 6), tri.neighbors
    if bounds is not None and (x < bounds[0] - EPS or x > bounds[1] + EPS or y < bounds[2] - EPS or y > bounds[3] + EPS):
        return -1, (0.0, 0.0, 0.0)
    for s in range(tri.nsimplex):
        t = tr[s]
        if t[0] == t[0]:
            dx, dy = x - t[4], y - t[5]
            c0 = t[0] * dx + t[1] * dy
            if not -EPS <= c0 <= 1 + EPS:
                continue
            c1 = t[2] * dx + t[3] * dy
            if not -EPS <= c1 <= 1 + EPS:
                continue
            c2 = 1.0 - c0 - c1
            if not -EPS <= c2 <= 1 + EPS:
                continue
            return s, (c0, c1, c2)
        for k in range(3):
            n = nb[s, k]
            if n == -1 or tr[n][0] != tr[n][0]:
                continue
            dx, dy = x - tr[n][4], y - tr[n][5]
            b0, b1 = tr[n][0] * dx + tr[n][1] * dy, tr[n][2] * dx + tr[n][3] * dy
            b = (b0, b1, 1.0 - b0 - b1)
            if all((-EPS_BROAD if nb[n, m] == s else -EPS) <= b[m] <= 1 + EPS for m in range(3)):
                return n, b
    return -1, (0.0, 0.0, 0.0)


def walk_locate(sc, t, v2s=None, bounds=None, forced=None):
    """(simplex or -1, barycentric coordinates, reported as ambiguous) of target t"""
    tri = sc.tri
    tr, nb, ns = tri.transform.reshape(-1, 6), tri.neighbors, tri.nsimplex
    x, y, nn = sc.tx[t], sc.ty[t], sc.nn_idx[t]
    f = -2 if forced is None else int(forced[t])
    if nn < 0:
        return -1, None, False
    if f >= -1:
        if not 0 <= f < ns:
            return -1, None, False
        dx, dy = x - tr[f][4], y - tr[f][5]
        c0, c1 = tr[f][0] * dx + tr[f][1] * dy, tr[f][2] * dx + tr[f][3] * dy
        return f, (c0, c1, 1.0 - c0 - c1), False
    s = int((tri.vertex_to_simplex if v2s is None else v2s)[nn])
    if not 0 <= s < ns:
        s = 0
    amb, found, c = False, False, (0.0, 0.0, 0.0)
    for _ in range(1 + ns // 4):
        dx, dy = x - tr[s][4], y - tr[s][5]
        go, c1, c2 = -2, c[1], c[2]
        c0 = tr[s][0] * dx + tr[s][1] * dy
        if c0 < -EPS:
            go = nb[s, 0]
        else:
            if not c0 <= 1 + EPS:
                go = -3
            c1 = tr[s][2] * dx + tr[s][3] * dy
            if c1 < -EPS:
                go = nb[s, 1]
            else:
                if not c1 <= 1 + EPS:
                    go = -3
                c2 = 1.0 - c0 - c1
                if c2 < -EPS:
                    go = nb[s, 2]
                elif not c2 <= 1 + EPS:
                    go = -3
        c = (c0, c1, c2)
        if go in (-2, -1, -3):
            found = True
            if go == -1:
                s = -1
            elif go == -3:
                (s, c), amb = _scan_locate(tri, x, y, bounds), True
            break
        s = int(go)
    if not found:
        (s, c), amb = _scan_locate(tri, x, y, bounds), True
    if s >= 0 and not amb:
        for k in range(3):
            n = nb[s, k]
            if c[k] <= 1e-6 and n >= 0:
                q = tr[n]
                if q[0] != q[0]:
                    amb = True
                    continue
                dx, dy = x - q[4], y - q[5]
                b0, b1 = q[0] * dx + q[1] * dy, q[2] * dx + q[3] * dy
                if all(-EPS <= b <= 1 + EPS for b in (b0, b1, 1.0 - b0 - b1)):
                    amb = True
    return int(s), c, amb


def walk_reference(sc, values, v2s=None, bounds=None, forced=None):
    """(out [nf, T] in values' dtype, scale [nf, T], reported target ids) of the restated walk"""
    v = np.asarray(values)
    nf = v.shape[0]
    out, scale, amb = np.full((nf, sc.T), np.nan), np.zeros((nf, sc.T)), []
    with np.errstate(invalid="ignore"):
        for t in range(sc.T):
            s, c, a = walk_locate(sc, t, v2s, bounds, forced)
            if a:
                amb.append(t)
            if s >= 0:
                vs = v[:, sc.tri.simplices[s]].astype(np.float64)
                out[:, t] = (c[0] * vs[:, 0] + c[1] * vs[:, 1]) + c[2] * vs[:, 2]
                scale[:, t] = np.abs(c[0] * vs[:, 0]) + np.abs(c[1] * vs[:, 1]) + np.abs(c[2] * vs[:, 2])
    return out.astype(v.dtype), scale, np.array(amb, dtype=np.int32)


def grazes_hull(tri, x, y, tol=1e-12):
    """within tol (barycentric) of a hull facet of some simplex that otherwise holds the point to tol"""
    ns = tri.nsimplex
    c = barycentric(tri, np.arange(ns), np.full(ns, x), np.full(ns, y))
    with np.errstate(invalid="ignore"):
        holds = ((c >= -tol) & (c <= 1.0 + tol)).all(axis=1)
        on = (np.abs(c) <= tol) & (tri.neighbors == -1)
    return bool((holds & on.any(axis=1)).any())
