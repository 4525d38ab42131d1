"""What the buddy-check tests share: the NumPy restatement of ``oisat_buddy_sums``' pair rule (never the library's kernel: the
correlation comes from ``oisat_corr_eval``, a host-only function), the reference loop of the iterated check, and the
planted-outlier recipe.  Everything is float64 on the host."""
import functools
import math

import numpy as np

import covariogram_cases as cc
from oisatgmi import _hip, dense

R_EARTH = cc.R_EARTH
KINDS = {"gaussian": 0, "gaspari_cohn": 1, "soar": 3}
CMIN = math.exp(-2.0)


def decay(L_km):
    return 0.5 * (R_EARTH / float(L_km)) ** 2


def corr_eval(kind, g, d2):
    lib = _hip.load_library()
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    out = np.empty_like(d2)
    assert lib.oisat_corr_eval(int(kind), float(g), d2.ctypes.data, d2.size, out.ctypes.data) == 0
    return out


def squared_chords(xyz):
    """Dense m x m: dx = xa - xb, d2 = dx dx + dy dy + dz dz, left to right."""
    dx, dy, dz = (xyz[k][:, None] - xyz[k][None, :] for k in range(3))
    return dx * dx + dy * dy + dz * dz


def ref_sums(xyz, u, kind, g, cmin):
    """-> dict n (int32), W, P, Q and, for the bounds, absP = sum |c u_b|, absQ = sum |c u_b^2| per row; the sums by
    ``math.fsum`` over the used b != a with c >= cmin, zeros for a row whose own u is not finite.  Asserts first that no used
    pair has |c - cmin| <= 1e-9 cmin: a last-bit difference in the device's exp cannot then move a pair across the cut."""
    u = np.asarray(u, dtype=np.float64)
    m = int(u.size)
    used = np.isfinite(u)
    c = corr_eval(kind, g, squared_chords(xyz)).reshape(m, m)
    pair = used[:, None] & used[None, :] & ~np.eye(m, dtype=bool)
    if pair.any():
        assert np.abs(c[pair] - cmin).min() > 1e-9 * cmin, "a pair sits on the cut: choose another seed"
    take = pair & (c >= cmin)
    ub = np.where(used, u, 0.0)
    t = c * ub[None, :]
    q = t * ub[None, :]
    out = {k: np.zeros(m) for k in ("W", "P", "Q", "absP", "absQ")}
    out["n"] = take.sum(axis=1).astype(np.int32)
    for a in np.flatnonzero(out["n"]):
        sel = take[a]
        out["W"][a] = math.fsum(c[a, sel])
        out["P"][a] = math.fsum(t[a, sel])
        out["Q"][a] = math.fsum(q[a, sel])
        out["absP"][a] = math.fsum(np.abs(t[a, sel]))
        out["absQ"][a] = math.fsum(np.abs(q[a, sel]))
    return out


def ref_buddy_check(xyz, u, kind, g, cmin=CMIN, k_background=5.0, k_buddy=3.0, min_buddies=3, max_passes=4):
    """The iterated check on ``ref_sums`` + ``dense.buddy_decide`` (pure NumPy).  -> (rejected, reason, passes, margin): margin =
    the smallest | |u - mean| / (k_buddy sqrt(1 + var)) - 1 | over every judged observation of every pass, i.e. how far the
    nearest decision was from its threshold."""
    work = np.array(u, dtype=np.float64)
    reason = np.zeros(work.size, dtype=np.uint8)
    passes, margin = [], np.inf
    for _ in range(max_passes):
        s = ref_sums(xyz, work, kind, g, cmin)
        judged = np.isfinite(work) & (s["n"] >= min_buddies) & (s["W"] > 0)
        if judged.any():
            mean = s["P"][judged] / s["W"][judged]
            var = np.maximum(s["Q"][judged] / s["W"][judged] - mean * mean, 0.0)
            margin = min(margin, float(np.abs(np.abs(work[judged] - mean) / (k_buddy * np.sqrt(1.0 + var)) - 1.0).min()))
        r = dense.buddy_decide(work, s["n"], s["W"], s["P"], s["Q"], k_background, k_buddy, min_buddies)
        new = (r != 0) & (reason == 0)
        reason[new] = r[new]
        work[new] = np.nan
        passes.append(int(new.sum()))
        if not new.any():
            break
    return reason != 0, reason, passes, margin


def lat_lon_of(xyz):
    """(lat, lon) in degrees of unit vectors."""
    return np.rad2deg(np.arcsin(np.clip(xyz[2], -1.0, 1.0))), np.rad2deg(np.arctan2(xyz[1], xyz[0]))


def by_ascending_z(xyz):
    return np.ascontiguousarray(xyz[:, np.argsort(xyz[2], kind="stable")])


PLANTED = dict(m=1500, cap_deg=20.0, L0=400.0, nbad=15, jump=8.0)


@functools.lru_cache(maxsize=None)
def planted_case(seed):
    """1500 points on a 20 degree cap in ascending z, a field drawn from 0.6 C + 0.4 I (Gaussian, L0 = 400 km), and 15 of its
    values moved by +-8.  -> (xyz, clean u, planted u, sorted indices of the planted ones), read-only."""
    c = PLANTED
    rng = np.random.default_rng(seed)
    p = by_ascending_z(cc.cap_points(rng, c["m"], c["cap_deg"]))
    S = 0.6 * np.exp(-decay(c["L0"]) * squared_chords(p)) + 0.4 * np.eye(c["m"])
    clean = np.linalg.cholesky(S) @ rng.normal(size=c["m"])
    bad = rng.choice(c["m"], c["nbad"], replace=False)
    u = clean.copy()
    u[bad] += c["jump"] * rng.choice([-1, 1], c["nbad"])
    bad = np.sort(bad)
    for a in (p, clean, u, bad):
        a.setflags(write=False)
    return p, clean, u, bad
