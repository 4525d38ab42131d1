"""What the superobservation tests share: the float64 NumPy restatement of ``oisat_superob`` (box table, box rule, quanta and the
fixed-point sums in int64, so the integer sums are reproduced exactly; never the library's kernel), the float64 analyses the
merged system is compared with, and the recipes, each with its seed.  Everything is float64 on the host.

``python tests/superob_cases.py`` prints the method-cost table of DESIGN.md section 4.2g / profiles/EXPERIMENTS.md."""
import functools
import math

import numpy as np

R_EARTH = 6371.0
MAX_OBS = 1 << 20
NAMES = ("W", "Q", "D", "V", "G", "Px", "Py", "Pz")
QUANTUM_OF = (0, 1, 2, 3, 4, 5, 5, 5)                  # which of the six quanta a row of the sums uses


def unit_vectors(lat, lon):
    la, lo = np.deg2rad(np.asarray(lat, dtype=np.float64)), np.deg2rad(np.asarray(lon, dtype=np.float64))
    return np.ascontiguousarray(np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)]))


# ---- the box table and the box rule (include/oisat.h) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_table(box_deg):
    """-> (n int32[nbands], offset int64[nbands], nbox), read-only."""
    box_deg = float(box_deg)
    nbands = max(int(math.ceil(180.0 / box_deg)), 1)
    n = np.empty(nbands, dtype=np.int32)
    for j in range(nbands):
        lo = -90.0 + float(j) * box_deg
        hi = min(-90.0 + float(j + 1) * box_deg, 90.0)
        mid = 0.5 * (lo + hi)
        n[j] = max(1, int(np.rint(360.0 * math.cos(mid * (math.pi / 180.0)) / box_deg)))
    offset = np.concatenate([[0], np.cumsum(n.astype(np.int64))[:-1]]).astype(np.int64)
    n.setflags(write=False)
    offset.setflags(write=False)
    return n, offset, int(n.astype(np.int64).sum())


def takes_part(lat, lon, d, sig, var):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(lat) & np.isfinite(lon) & np.isfinite(d) & np.isfinite(sig) & np.isfinite(var)
        ok &= (np.abs(lat) <= 90.0) & (var > 0.0)
        ok &= np.isfinite(1.0 / np.where(ok, var, 1.0))
    return ok


def box_of(lat, lon, used, box_deg):
    """The box of every observation, -1 where ``used`` is False; one NumPy operation per operation of the rule."""
    n, offset, _ = box_table(box_deg)
    la, lo = np.where(used, lat, 0.0), np.where(used, lon, 0.0)
    j = np.minimum(np.floor((la + 90.0) / float(box_deg)).astype(np.int64), n.size - 1)
    r = lo / 360.0
    t = r - np.floor(r)
    nj = n[j].astype(np.int64)
    k = np.minimum((t * nj.astype(np.float64)).astype(np.int64), nj - 1)
    return np.where(used, offset[j] + k, -1).astype(np.int64)


def edge_distance_deg(lat, lon, box_deg):
    """The smallest distance, in degrees of latitude or longitude, of any point to an edge between two boxes."""
    n, _, _ = box_table(box_deg)
    f = (np.asarray(lat) + 90.0) / float(box_deg)
    j = np.minimum(np.floor(f).astype(np.int64), n.size - 1)
    inner = (np.rint(f) > 0) & (np.rint(f) < n.size)               # (the two poles are no edges)
    dlat = np.where(inner, np.abs(f - np.rint(f)) * float(box_deg), np.inf)
    nj = n[j].astype(np.float64)
    r = np.asarray(lon) / 360.0
    s = (r - np.floor(r)) * nj
    dlon = np.where(nj > 1, np.abs(s - np.rint(s)) * 360.0 / nj, np.inf)
    return float(min(dlat.min(initial=np.inf), dlon.min(initial=np.inf)))


# ---- the quanta -----------------------------------------------------------------------------------------------------------------
def _pow2(e):
    return math.ldexp(1.0, max(e, -1022))


def _quantum(bound, m):
    prod = bound * float(max(int(m), 1))
    return 1.0 if prod == 0.0 else _pow2(math.frexp(prod)[1] - 62)


def quanta(wmax, dmax, smax, m):
    """q_W, q_Q, q_D, q_V, q_G, q_P; None where the library answers OISAT_EINVAL."""
    mm = float(max(int(m), 1))
    if not (0 <= m <= MAX_OBS and wmax >= 0 and dmax >= 0 and smax >= 0):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        prods = np.array([np.float64(2.0) * wmax * mm, np.float64(wmax) * dmax * dmax * mm, np.float64(wmax) * smax * mm])
    if not np.isfinite(prods).all():
        return None
    ew = math.frexp(wmax)[1]
    eh = (ew + 1) // 2 if ew >= 0 else -((-ew) // 2)
    return np.array([_quantum(wmax, m), _quantum(0.0 if wmax == 0.0 else math.ldexp(1.0, eh), m), _quantum(wmax * dmax, m),
                     _quantum(wmax * dmax * dmax, m), _quantum(wmax * smax, m), _quantum(2.0 * wmax, m)])


# ---- the sums -----------------------------------------------------------------------------------------------------------------------
def ref_superob(lat, lon, xyz, d, sig, var, box_deg):
    """-> dict: ``box`` (int64[m], -1 unused), ``nused``, ``ids`` (ascending non-empty boxes), ``count`` (per id), ``q`` (the six
    quanta), ``terms`` (8, nused: the float64 terms as the kernel forms them), ``isum`` (8, ids: the int64 sums), ``sums``
    (8, ids: (double)isum q), ``used``, ``slot`` (per used observation, its position in ids)."""
    lat, lon, d, sig, var = (np.asarray(a, dtype=np.float64) for a in (lat, lon, d, sig, var))
    m = int(d.size)
    used = takes_part(lat, lon, d, sig, var) if m else np.zeros(0, dtype=bool)
    box = box_of(lat, lon, used, box_deg) if m else np.zeros(0, dtype=np.int64)
    u = np.flatnonzero(used)
    w = 1.0 / var[u]
    du, su = d[u], sig[u]
    wd = w * du
    terms = np.stack([w, np.sqrt(w), wd, wd * du, w * su, w * xyz[0][u], w * xyz[1][u], w * xyz[2][u]]) if u.size else np.zeros((8, 0))
    q = quanta(w.max(), np.abs(du).max(), np.abs(su).max(), m) if u.size else quanta(0.0, 0.0, 0.0, m)
    assert q is not None
    ids, slot = np.unique(box[u], return_inverse=True)
    count = np.bincount(slot, minlength=ids.size).astype(np.int64)
    isum = np.zeros((8, ids.size), dtype=np.int64)
    for k in range(8):
        it = np.rint(terms[k] / q[QUANTUM_OF[k]]).astype(np.int64)          # (an exact division; nearest even, like llrint)
        np.add.at(isum[k], slot, it)
    sums = isum.astype(np.float64) * q[list(QUANTUM_OF)][:, None]
    return {"box": box, "nused": int(u.size), "ids": ids, "count": count, "q": q, "terms": terms, "isum": isum, "sums": sums,
            "used": used, "slot": slot}


def merge(ref, rho=0.0):
    """The superobservations of ``ref_superob``'s sums, by the formulas of ``dense.superob``."""
    W, Q, D, V, G, Px, Py, Pz = ref["sums"]
    norm = np.sqrt(Px * Px + Py * Py + Pz * Pz)
    dm = D / W
    return {"lat": np.rad2deg(np.arcsin(np.clip(Pz / norm, -1.0, 1.0))), "lon": np.rad2deg(np.arctan2(Py, Px)), "d": dm,
            "sigma_b": G / W, "var": ((1.0 - rho) * W + rho * Q * Q) / (W * W), "spread": np.maximum(V / W - dm * dm, 0.0),
            "count": ref["count"], "W": W}


# ---- float64 analyses ----------------------------------------------------------------------------------------------------------------
def decay(L_km):
    return 0.5 * (R_EARTH / float(L_km)) ** 2


def chord2(pa, pb):
    dx, dy, dz = (pa[k][:, None] - pb[k][None, :] for k in range(3))
    return dx * dx + dy * dy + dz * dz


def gaussian(L_km):
    g = decay(L_km)
    return lambda d2: np.exp(-g * d2)


def analysis(corr, grid_xyz, grid_sig, obs_xyz, obs_sig, obs_var, d):
    """z = (sig C sig + R)^-1 d by a SciPy Cholesky, the increment sig_g C_go sig_o z on the grid points, and cond(S)."""
    from scipy.linalg import cho_factor, cho_solve
    S = obs_sig[:, None] * corr(chord2(obs_xyz, obs_xyz)) * obs_sig[None, :] + np.diag(obs_var)
    z = cho_solve(cho_factor(S, lower=True), d)
    inc = grid_sig * ((corr(chord2(grid_xyz, obs_xyz)) * obs_sig[None, :]) @ z)
    return z, inc, S


# ---- recipes --------------------------------------------------------------------------------------------------------------------------
def random_obs(seed, m, box_deg, lat_range=(-89.0, 89.0), lon_range=(-180.0, 360.0), clear_deg=1e-9):
    """m observations with random positions, each at least ``clear_deg`` from every box edge (the few that are not are drawn
    again), random d, sigma_b and var.  -> dict lat, lon, d, sig, var."""
    rng = np.random.default_rng(seed)
    lat, lon = rng.uniform(*lat_range, m), rng.uniform(*lon_range, m)
    for _ in range(100):
        close = _close(lat, lon, box_deg, 10 * clear_deg)
        if not close.any():
            break
        lat[close], lon[close] = rng.uniform(*lat_range, int(close.sum())), rng.uniform(*lon_range, int(close.sum()))
    return {"lat": lat, "lon": lon, "d": rng.normal(size=m), "sig": rng.uniform(0.5, 2.0, m), "var": rng.uniform(0.05, 1.0, m)}


def _close(lat, lon, box_deg, eps):
    n, _, _ = box_table(box_deg)
    f = (lat + 90.0) / float(box_deg)
    j = np.minimum(np.floor(f).astype(np.int64), n.size - 1)
    nj = n[j].astype(np.float64)
    r = lon / 360.0
    s = (r - np.floor(r)) * nj
    return (np.abs(f - np.rint(f)) * float(box_deg) < eps) | ((nj > 1) & (np.abs(s - np.rint(s)) * 360.0 / nj < eps))


PATCH = dict(ny=48, nx=48, cell_deg=0.25, lat0=30.0, lon0=10.0, observed=0.9, sigma_b=1.0, var_lo=0.1, var_hi=0.4, seed=20261)


@functools.lru_cache(maxsize=None)
def patch_case(L_km, seed=PATCH["seed"]):
    """The method-cost recipe: a 48 x 48 patch of 0.25 degree cells (south-west corner 30 N 10 E), 90 % of them observed at the
    cell centre, the truth drawn from a Gaussian B of length ``L_km`` with sigma_b = 1 around a zero background, every
    observation the truth plus an independent error of variance uniform in [0.1, 0.4].  -> dict, read-only arrays."""
    c = PATCH
    rng = np.random.default_rng(seed)
    la = c["lat0"] + (np.arange(c["ny"]) + 0.5) * c["cell_deg"]
    lo = c["lon0"] + (np.arange(c["nx"]) + 0.5) * c["cell_deg"]
    lat2, lon2 = np.meshgrid(la, lo, indexing="ij")
    gxyz = unit_vectors(lat2.ravel(), lon2.ravel())
    n = lat2.size
    B = c["sigma_b"] ** 2 * gaussian(L_km)(chord2(gxyz, gxyz))
    ev, evec = np.linalg.eigh(B)
    truth = evec @ (np.sqrt(np.maximum(ev, 0.0)) * rng.normal(size=n))
    cell = np.sort(rng.choice(n, int(round(c["observed"] * n)), replace=False))
    var = rng.uniform(c["var_lo"], c["var_hi"], cell.size)
    y = truth[cell] + np.sqrt(var) * rng.normal(size=cell.size)
    out = {"lat2": lat2, "lon2": lon2, "gxyz": gxyz, "truth": truth, "cell": cell, "obs_lat": lat2.ravel()[cell],
           "obs_lon": lon2.ravel()[cell], "var": var, "d": y, "sig": np.full(cell.size, c["sigma_b"]), "L_km": float(L_km)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def method_cost(L_km, box_deg, rho=0.0):
    """The superobbed analysis of ``patch_case(L_km)`` against the full one, both float64 on the host, on all patch cells.
    -> dict nobs, nsuper, diff (rms of the two increments' difference over the rms of the full increment), err_full / err_super
    (rms of increment - truth)."""
    p = patch_case(L_km)
    corr = gaussian(L_km)
    gsig = np.full(p["truth"].size, PATCH["sigma_b"])
    oxyz = unit_vectors(p["obs_lat"], p["obs_lon"])
    _, inc_full, _ = analysis(corr, p["gxyz"], gsig, oxyz, p["sig"], p["var"], p["d"])
    s = merge(ref_superob(p["obs_lat"], p["obs_lon"], oxyz, p["d"], p["sig"], p["var"], box_deg), rho)
    _, inc_so, _ = analysis(corr, p["gxyz"], gsig, unit_vectors(s["lat"], s["lon"]), s["sigma_b"], s["var"], s["d"])
    rms = lambda a: float(np.sqrt(np.mean(a * a)))      # noqa: E731
    return {"nobs": int(p["d"].size), "nsuper": int(s["d"].size), "diff": rms(inc_so - inc_full) / rms(inc_full),
            "err_full": rms(inc_full - p["truth"]), "err_super": rms(inc_so - p["truth"])}


if __name__ == "__main__":
    print("L_km  box_deg  nobs  nsuper  rms(inc_super - inc_full)/rms(inc_full)  rms error full  rms error super")
    for L in (300.0, 150.0):
        for box in (0.5, 1.0, 2.0):
            r = method_cost(L, box)
            print(f"{L:5.0f}  {box:7.2f}  {r['nobs']:4d}  {r['nsuper']:6d}  {r['diff']:39.4f}  {r['err_full']:14.4f}  {r['err_super']:15.4f}")
