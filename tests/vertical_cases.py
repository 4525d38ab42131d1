"""Seeded catalogues of adversarial columns for the per-pixel vertical operators of csrc/amf.hip, and the scipy
references they are judged by (tests/test_gpu_vertical_abi.py on the device, tests/test_vertical_cases_cpu.py here).

Every pixel of these operators is an independent column, so a catalogue is one launch: column i of every array is
case i, tagged ``tags[i]``.  ``catalogue(op, nzs, nzc, dtype)`` is deterministic; a column whose result moves by more
than half the bar when every logarithm moves by one ulp is drawn again (never dropped), so what the device is compared
with does not hinge on the last bit of its ``log``.

Roles: the AMF recalculation interpolates the SATELLITE column (nodes) at the MODEL levels (queries); the
averaging-kernel convolutions interpolate the MODEL column (nodes) at the SATELLITE levels (queries).  "first" / "last"
below mean the node of lowest / highest pressure, whatever the storage order.

Float32 cubes: the model arrays hold float32 values, ``np.log`` / ``np.log10`` of them is the double logarithm rounded
once to float32 (what the kernels document), and interp1d receives float32 x / y so that scipy's own dtype path decides
the arithmetic (_call_linear: slope in float32, the rest in float64).  A query "exactly on a node" then needs a double
pressure whose double log IS the node's float32 log: such ties are put at pressure 1 (``_Col.tie``).
"""
import functools
import zlib

import numpy as np
from scipy.interpolate import interp1d

OPS = ("amf", "mopitt", "gosat")
# (nzs, nzc): together nzs in {1 (AK only), 2, 7, 8, 9, 35, 64} and nzc in {1 (AMF only), 2, 7, 8, 9, 16, 17, 72, 127, 128}
PAIRS = {
    "amf": ((2, 1), (2, 2), (7, 7), (8, 8), (9, 9), (35, 16), (64, 17), (35, 72), (9, 127), (64, 128)),
    "mopitt": ((1, 2), (2, 2), (7, 7), (8, 8), (9, 9), (35, 16), (64, 17), (35, 72), (9, 127), (64, 128)),
    "gosat": ((1, 2), (2, 2), (7, 7), (8, 8), (9, 9), (35, 16), (64, 17), (35, 72), (9, 127), (64, 128)),
}
RT64 = 1e-12                    # the bar of the float64 golden tests (tests/test_gpu_parity.py)
MIN_RATIO = 1.01                # distinct levels of one column are at least 1 % apart in pressure
REPS = 24                       # columns per category (12 for the NaN-node ones): about 1 000 columns per catalogue
NAN_NODE_TAGS = ("nan_node_p", "p_neg_node")
DUP_TAGS = ("dup_pair_first", "dup_pair_mid", "dup_pair_last", "dup_run3", "dup_all")
# categories whose point is the jump at an exact tie (equal bits, so equal logarithms on any device): no ulp test
# (on the first / last node MOPITT's NaN fill begins, and nansum absorbs it without a trace in the pattern; at any node
# _call_linear's float32 slope makes the two segments meet only to float32 precision)
TIE_JUMP_TAGS = DUP_TAGS + ("on_node_beside_nan", "on_node_beside_inf", "on_node_first", "on_node_mid", "on_node_last")


class _Retry(Exception):
    pass


def _levels(rng, nz, lo, hi):
    """nz pressures, descending, one in the central half of each of nz log-spaced cells: neighbours >= 3.5 % apart"""
    e = np.linspace(np.log(hi), np.log(lo), nz + 1)
    w = e[:-1] - e[1:]
    return np.exp(e[:-1] - w * (0.25 + 0.5 * rng.uniform(size=nz)))


def _smooth(rng, nz, lo=0.6, hi=1.6):
    """positive values whose neighbours differ by less than a factor 1.3: a log's ulp cannot be amplified past the bar"""
    v = np.cumsum(rng.uniform(-0.25, 0.25, size=nz))
    return rng.uniform(lo, hi) * np.exp(v - v.mean() * 0.5)


class _Col:
    """one column; ``node_*`` / ``query_p`` map onto the satellite or the model side by the operator's roles"""

    def __init__(self, op, rng, nzs, nzc, T):
        self.op, self.T, self.nzs, self.nzc = op, T, nzs, nzc
        self.sat_p = _levels(rng, nzs, 0.8, 900.0)
        self.ctm_p = _levels(rng, nzc, 0.05, 1050.0).astype(T)
        if op == "amf":
            self.sat_y = _smooth(rng, nzs)                                   # scattering weights
            self.ctm_y = (_smooth(rng, nzc) * 0.3).astype(T)                 # partial columns
            self.trop = float(np.sort(self.ctm_p)[nzc // 3]) * 0.98          # masks the upper third of the model levels
            self.vcd, self.amf = float(rng.uniform(1.0, 9.0)), float(rng.uniform(0.5, 3.0))
        else:
            self.ctm_y = (_smooth(rng, nzc) * 80.0).astype(T)                # mixing ratio
            self.ap_prof = _smooth(rng, nzs) * 70.0
            self.vcd = float(rng.uniform(1.0, 9.0))                          # MOPITT vcd / GOSAT x_col
            if op == "mopitt":
                self.air = (_smooth(rng, nzc) * 5.0e3).astype(T)
                self.ak = rng.uniform(0.02, 0.4, size=nzs + 1)
                self.ap_col, self.ap_surf = float(rng.uniform(1.0, 3.0)), float(rng.uniform(50.0, 120.0))
            else:
                self.ak = rng.uniform(0.2, 1.2, size=nzs)
                self.pw = rng.dirichlet(np.ones(nzs) * 4.0) if nzs > 1 else np.ones(1)

    # -- roles
    @property
    def nodes_are_sat(self):
        return self.op == "amf"

    @property
    def node_p(self):
        return self.sat_p if self.nodes_are_sat else self.ctm_p

    @property
    def node_y(self):
        return self.sat_y if self.nodes_are_sat else self.ctm_y

    @property
    def query_p(self):
        return self.ctm_p if self.nodes_are_sat else self.sat_p

    def reorder(self, rng, how):
        for side, names in (("sat", ("sat_p", "sat_y", "ap_prof", "pw")), ("ctm", ("ctm_p", "ctm_y", "air"))):
            n = self.nzs if side == "sat" else self.nzc
            perm = {"desc": np.arange(n), "asc": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[how]
            if how == "shuffled" and n > 1 and perm[0] == int(np.argmax(getattr(self, side + "_p"))):
                perm = np.roll(perm, 1)                  # the highest pressure (the surface) is never stored first
            for nm in names:
                if hasattr(self, nm):
                    setattr(self, nm, getattr(self, nm)[perm].copy())

    def sorted_nodes(self):
        return np.argsort(self.node_p, kind="stable")    # ascending pressure

    def tie(self, nodes, iq):
        """put query iq exactly on the node(s) `nodes` (which share one pressure).  float64 cubes: equal bits, so equal
        logarithms whatever the log function.  float32 cubes: the column is rescaled so that the tie sits at pressure 1,
        whose logarithm is 0 in both precisions and in every implementation."""
        nodes = np.atleast_1d(nodes)
        if self.T == np.float64:
            self.query_p[iq] = self.node_p[nodes[0]]
            self.node_p[nodes] = self.node_p[nodes[0]]
        else:
            f = 1.0 / float(self.node_p[nodes[0]])
            self.sat_p *= f
            self.ctm_p[:] = (self.ctm_p.astype(np.float64) * f).astype(self.T)
            if hasattr(self, "trop"):
                self.trop *= f
            self.node_p[nodes] = 1.0
            self.query_p[iq] = 1.0

    def queries(self, rng, k):
        """k distinct query indices (fewer when the column has fewer queries)"""
        n = self.query_p.size
        return list(rng.permutation(n)[:min(k, n)])

    def query_outside(self, iq, below):
        allp = np.concatenate([self.sat_p, self.ctm_p.astype(np.float64)])
        allp = allp[np.isfinite(allp) & (allp > 0)]
        self.query_p[iq] = allp.min() * 0.5 if below else allp.max() * 2.0


def _place(c, rng, rep, on=None):
    """a query on the node(s) `on` (if any), one below the first node and one above the last; with a single query the
    repetition index decides which of the three this column gets"""
    want = ([("on", on)] if on is not None else []) + [("below", None), ("above", None)]
    qs = c.queries(rng, len(want))
    if len(qs) < len(want):
        want = [want[(rep + i) % len(want)] for i in range(len(qs))]
    for iq, (what, arg) in zip(qs, want):
        if what == "on":
            c.tie(arg, iq)
        else:
            c.query_outside(iq, below=(what == "below"))


def _dup(c, rng, rep, where):
    s = c.sorted_nodes()
    n = s.size
    if where == "all":
        grp = s
    elif where == "run3":
        a = int(rng.integers(0, n - 2))
        grp = s[a:a + 3]
    else:
        a = {"first": 0, "last": n - 2, "mid": (n - 2) // 2 if n < 4 else int(rng.integers(1, n - 2))}[where]
        grp = s[a:a + 2]
    c.node_p[grp] = c.node_p[grp[0]]
    _place(c, rng, rep, on=grp)


def _node_at(c, rng, where):
    s = c.sorted_nodes()
    if where == "first":
        return int(s[0])
    if where == "last":
        return int(s[-1])
    return int(s[rng.integers(1, s.size - 1)])


def rep_safe(rng, n):
    return int(rng.integers(0, n))


def _set_y(c, rng, rep, where, value):
    c.node_y[_node_at(c, rng, where)] = value


def _beside(c, rng, rep, value):
    """a non-finite node value next to a query that lies exactly on the neighbouring node (either side)"""
    s = c.sorted_nodes()
    i = int(rng.integers(0, s.size - 1))
    on, bad = (s[i], s[i + 1]) if rep % 2 == 0 else (s[i + 1], s[i])
    c.node_y[bad] = value
    c.tie(on, c.queries(rng, 1)[0])


def _generic():
    """tag -> (mutator(c, rng, rep), minimum number of nodes); applies to all three operators through the roles"""
    g = {
        "order_desc": (lambda c, rng, rep: None, 1),
        "order_asc": (lambda c, rng, rep: c.reorder(rng, "asc"), 1),
        "order_shuffled": (lambda c, rng, rep: c.reorder(rng, "shuffled"), 1),
        "dup_pair_first": (lambda c, rng, rep: _dup(c, rng, rep, "first"), 2),
        "dup_pair_mid": (lambda c, rng, rep: _dup(c, rng, rep, "mid"), 2),
        "dup_pair_last": (lambda c, rng, rep: _dup(c, rng, rep, "last"), 2),
        "dup_run3": (lambda c, rng, rep: _dup(c, rng, rep, "run3"), 3),
        "dup_all": (lambda c, rng, rep: _dup(c, rng, rep, "all"), 2),
        "on_node_mid": (lambda c, rng, rep: c.tie(_node_at(c, rng, "mid"), c.queries(rng, 1)[0]), 3),
        "on_node_first": (lambda c, rng, rep: c.tie(_node_at(c, rng, "first"), c.queries(rng, 1)[0]), 2),
        "on_node_last": (lambda c, rng, rep: c.tie(_node_at(c, rng, "last"), c.queries(rng, 1)[0]), 2),
        "query_below_first": (lambda c, rng, rep: c.query_outside(c.queries(rng, 1)[0], True), 2),
        "query_above_last": (lambda c, rng, rep: c.query_outside(c.queries(rng, 1)[0], False), 2),
        "nan_node_p": (lambda c, rng, rep: c.node_p.__setitem__(rep_safe(rng, c.node_p.size), np.nan), 2),
        "nan_query_p": (lambda c, rng, rep: c.query_p.__setitem__(c.queries(rng, 1)[0], np.nan), 2),
        "p_zero_node": (lambda c, rng, rep: c.node_p.__setitem__(rep_safe(rng, c.node_p.size), 0.0), 2),
        "p_zero_query": (lambda c, rng, rep: c.query_p.__setitem__(c.queries(rng, 1)[0], 0.0), 2),
        "p_neg_node": (lambda c, rng, rep: c.node_p.__setitem__(rep_safe(rng, c.node_p.size), -3.5), 2),
        "p_neg_query": (lambda c, rng, rep: c.query_p.__setitem__(c.queries(rng, 1)[0], -3.5), 2),
        "on_node_beside_nan": (lambda c, rng, rep: _beside(c, rng, rep, np.nan), 2),
        "on_node_beside_inf": (lambda c, rng, rep: _beside(c, rng, rep, np.inf if rep % 4 < 2 else -np.inf), 2),
    }
    for vn, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for where in ("mid", "first", "last"):
            g[f"y_{vn}_{where}"] = (functools.partial(_set_y, where=where, value=v), 3 if where == "mid" else 2)
    return g


def _amf_specific():
    def trop_equal(c, rng, rep):
        c.trop = float(c.ctm_p[rep_safe(rng, c.nzc)])

    def sw_zero(c, rng, rep):
        c.sat_y[:] = 0.0

    def pc_bad(c, rng, rep):
        c.ctm_y[rep_safe(rng, c.nzc)] = (np.nan, np.inf, -np.inf)[rep % 3]

    return {
        "trop_below_all": (lambda c, rng, rep: setattr(c, "trop", 0.01), 2),
        "trop_equal_level": (trop_equal, 2),
        "trop_above_all": (lambda c, rng, rep: setattr(c, "trop", 5000.0), 2),
        "trop_nan": (lambda c, rng, rep: setattr(c, "trop", np.nan), 2),
        "sw_all_zero": (sw_zero, 2),
        "partial_column_nonfinite": (pc_bad, 2),
        "vcd_nan": (lambda c, rng, rep: setattr(c, "vcd", np.nan), 2),
        "vcd_pinf": (lambda c, rng, rep: setattr(c, "vcd", np.inf), 2),
        "vcd_ninf": (lambda c, rng, rep: setattr(c, "vcd", -np.inf), 2),
    }


def _block(c, rng, value):
    """`value` on a run of three neighbouring nodes (two when there are only two): the segments between them are flat"""
    s = c.sorted_nodes()
    k = min(3, s.size)
    a = int(rng.integers(0, s.size - k + 1))
    c.node_y[s[a:a + k]] = value
    return s[a:a + k]


def _mopitt_specific():
    def prof_negative(c, rng, rep):
        _block(c, rng, -7.0)

    def prof_zero(c, rng, rep):
        grp = _block(c, rng, 0.0)                      # a query on the block's middle node: both segments beside it are flat
        c.tie(grp[1], c.queries(rng, 1)[0])

    def ap_zero(c, rng, rep):
        c.ap_prof[rep_safe(rng, c.nzs)] = 0.0

    def ak_zero_inf(c, rng, rep):
        k = rep_safe(rng, c.nzs)
        c.ap_prof[k] = 0.0
        c.ak[k + 1] = 0.0

    def air_nan(c, rng, rep):
        c.air[:] = np.nan

    def air_zero(c, rng, rep):
        a = c.air[0]
        c.air[:] = 0.0
        c.air[0], c.air[1] = a, -a

    def surface(c, rng, rep):
        c.reorder(rng, "shuffled")
        c.ctm_y[0] = c.T(c.ctm_y[0] * 3.75)

    return {
        "prof_negative": (prof_negative, 2), "prof_zero": (prof_zero, 2), "apriori_zero": (ap_zero, 2),
        "ak_zero_against_inf": (ak_zero_inf, 2), "air_all_nan": (air_nan, 2), "air_sum_zero": (air_zero, 2),
        "surface_level0_shuffled": (surface, 2),
        "vcd_nan": (lambda c, rng, rep: setattr(c, "vcd", np.nan), 2),
        "vcd_pinf": (lambda c, rng, rep: setattr(c, "vcd", np.inf), 2),
        "vcd_ninf": (lambda c, rng, rep: setattr(c, "vcd", -np.inf), 2),
    }


def _gosat_specific():
    def term(c, rng, rep, value):
        c.pw[rep_safe(rng, c.nzs)] = value

    def all_dropped(c, rng, rep):
        c.pw[:] = -np.abs(c.pw) - 0.01

    return {
        "term_negative": (functools.partial(term, value=-0.2), 2),
        "term_pzero": (functools.partial(term, value=0.0), 2),
        "term_nzero": (functools.partial(term, value=-0.0), 2),
        "all_terms_dropped": (all_dropped, 2),
        "xcol_nan": (lambda c, rng, rep: setattr(c, "vcd", np.nan), 2),
        "xcol_pinf": (lambda c, rng, rep: setattr(c, "vcd", np.inf), 2),
        "xcol_ninf": (lambda c, rng, rep: setattr(c, "vcd", -np.inf), 2),
    }


def categories(op):
    g = _generic()
    g.update({"amf": _amf_specific, "mopitt": _mopitt_specific, "gosat": _gosat_specific}[op]())
    return g


def required_tags(op, nzs, nzc):
    """the categories a catalogue of this shape must hold: all of them, but for those that need more nodes than it has
    (an interior node or a run of three needs three)"""
    n_nodes = nzs if op == "amf" else nzc
    return sorted(t for t, (_, need) in categories(op).items() if n_nodes >= need)


def spacing_ok(p):
    """distinct, finite, positive levels of one side at least 1 % apart"""
    p = np.unique(np.asarray(p, dtype=np.float64))
    p = p[np.isfinite(p) & (p > 0)]
    return p.size < 2 or bool((p[1:] / p[:-1]).min() >= MIN_RATIO)


# ---------------------------------------------------------------------------------------------------------------
# references: scipy decides
# ---------------------------------------------------------------------------------------------------------------
def _lg(p, fn=np.log, shift=0):
    """fn(p) in p's dtype: for float32 the double logarithm rounded once; `shift` moves the DOUBLE logarithm by that many
    ulps first (the conditioning check)"""
    p = np.asarray(p)
    with np.errstate(all="ignore"):
        x = fn(p.astype(np.float64))
        if shift:
            x = np.where(np.isfinite(x), np.nextafter(x, np.float64(np.inf if shift > 0 else -np.inf)), x)
    return x.astype(p.dtype) if p.dtype == np.float32 else x


def amf_pixel(sat_p, sat_sw, ctm_p, ctm_pc, trop, shift=(0, 0)):
    """orc.amf_pixel with the float32 logarithm pinned -> (new_amf, model_vcd, sum |sw * pc|, sum |pc|)"""
    f = interp1d(_lg(sat_p, shift=shift[0]), sat_sw, fill_value="extrapolate")
    with np.errstate(all="ignore"):
        sw = f(_lg(ctm_p, shift=shift[1]))
        sw[np.isinf(sw)] = 0.0
        pc = np.array(ctm_pc, copy=True)
        if trop is not None:
            m = ctm_p < trop
            sw[m] = np.nan
            pc[m] = np.nan
        t = sw * pc
        scd, vcd = np.nansum(t), np.nansum(pc)
        return (scd / vcd if vcd != 0 else np.nan), vcd, np.nansum(np.abs(t)), np.nansum(np.abs(pc.astype(np.float64)))


def mopitt_pixel(ctm_p, ctm_prof, ctm_air, sat_p, ak, ap_prof, ap_col, ap_surf, shift=(0, 0)):
    """orc.mopitt_pixel with the float32 logarithms pinned -> (model_vcd, model_xcol, scale of model_vcd, |air sum|)"""
    f = interp1d(_lg(ctm_p, shift=shift[0]), ctm_prof, fill_value=np.nan, bounds_error=False)
    with np.errstate(all="ignore"):
        xi = f(_lg(sat_p, shift=shift[1]))
        t = ak[1:] * (_lg(xi, np.log10, shift[1]) - np.log10(ap_prof))
        prof_part = ap_col + np.nansum(t)
        surf_part = ak[0] * (_lg(ctm_prof[0], np.log10, shift[0]) - np.log10(ap_surf))
        v = prof_part + surf_part
        air = np.nansum(ctm_air)
        return v, 1e6 * v / air, np.abs(ap_col) + np.nansum(np.abs(t)) + np.abs(surf_part), np.abs(np.float64(air))


def gosat_pixel(ctm_p, ctm_prof, sat_p, ak, ap_prof, pw, shift=(0, 0)):
    """orc.gosat_pixel with the float32 logarithm pinned -> (model_xcol, sum |terms|)"""
    f = interp1d(_lg(ctm_p, shift=shift[0]), ctm_prof, fill_value="extrapolate")
    with np.errstate(all="ignore"):
        xi = f(_lg(sat_p, shift=shift[1]))
        t = (ap_prof + (xi - ap_prof) * ak) * pw
        t[t <= 0] = np.nan
        return np.nansum(t), np.nansum(np.abs(t))


class Catalogue:
    """arrays are level-major [nz][n] like the C ABI's cubes; `tags[i]` names column i's category"""

    def __init__(self, op, nzs, nzc, dtype, cols, tags):
        self.op, self.nzs, self.nzc, self.dtype, self.tags, self.n = op, nzs, nzc, np.dtype(dtype), list(tags), len(cols)
        names = {"amf": ("sat_p", "sat_y", "ctm_p", "ctm_y"), "mopitt": ("sat_p", "ctm_p", "ctm_y", "air", "ak", "ap_prof"),
                 "gosat": ("sat_p", "ctm_p", "ctm_y", "ak", "ap_prof", "pw")}[op]
        for nm in names:
            setattr(self, nm, np.ascontiguousarray(np.stack([getattr(c, nm) for c in cols], axis=1)))
        scal = {"amf": ("trop", "vcd", "amf"), "mopitt": ("vcd", "ap_col", "ap_surf"), "gosat": ("vcd",)}[op]
        for nm in scal:
            setattr(self, nm, np.array([getattr(c, nm) for c in cols], dtype=np.float64))

    def head(self, n):
        """the first n columns as a catalogue of their own"""
        out = object.__new__(Catalogue)
        out.__dict__.update(self.__dict__)
        out.n, out.tags = n, self.tags[:n]
        for k, v in self.__dict__.items():
            if isinstance(v, np.ndarray):
                setattr(out, k, np.ascontiguousarray(v[..., :n]))
        return out

    def pattern_only(self):
        """columns judged by NaN / inf pattern alone: a NaN among the nodes of np.interp (float64 cubes, MOPITT)"""
        on = self.op == "mopitt" and self.dtype == np.float64
        return np.array([on and t in NAN_NODE_TAGS for t in self.tags])


def reference(cat, pixels=None, use_trop=True, shift=(0, 0)):
    """name -> (reference array, scale array) for every output of the operator, with the pixel-skip rules and post-masks of
    amf_recal.py / ak_conv_*.py around the per-pixel function.  `pixels`: the function whose VALUES are used (the oracle's,
    for float64 cubes); the scales always come from the functions above."""
    n, nan = cat.n, np.nan
    out = {}
    with np.errstate(all="ignore"):
        if cat.op == "amf":
            new_amf, mv, s_amf, s_mv = (np.full(n, nan) for _ in range(4))
            for i in range(n):
                if np.isnan(cat.vcd[i]):
                    continue
                args = (cat.sat_p[:, i], cat.sat_y[:, i], cat.ctm_p[:, i], cat.ctm_y[:, i], cat.trop[i] if use_trop else None)
                a, v, s1, s2 = amf_pixel(*args, shift=shift)
                if pixels is not None:
                    a, v = pixels(*args)
                new_amf[i], mv[i], s_mv[i] = a, v, s2
                s_amf[i] = s1 / np.abs(np.float64(v)) if v != 0 else nan
            vcd_out = (cat.amf * cat.vcd) / new_amf
            mv[np.isnan(vcd_out) | np.isinf(vcd_out)] = nan
            out["new_amf"] = (new_amf, s_amf)
            out["vcd_out"] = (vcd_out, np.abs(vcd_out) * s_amf / np.abs(new_amf))
            out["ctm_vcd"] = (mv, s_mv)
        elif cat.op == "mopitt":
            mv, mx, s_v, s_x = (np.full(n, nan) for _ in range(4))
            for i in range(n):
                if np.isnan(cat.vcd[i]):
                    continue
                args = (cat.ctm_p[:, i], cat.ctm_y[:, i], cat.air[:, i], cat.sat_p[:, i], cat.ak[:, i], cat.ap_prof[:, i],
                        cat.ap_col[i], cat.ap_surf[i])
                v, x, s, a = mopitt_pixel(*args, shift=shift)
                if pixels is not None:
                    v, x = pixels(*args)
                mv[i], mx[i], s_v[i], s_x[i] = v, x, s, 1e6 * s / a
            mv[np.isinf(cat.vcd)] = nan
            out["model_vcd"], out["model_xcol"] = (mv, s_v), (mx, s_x)
        else:
            mx, s_x = np.full(n, nan), np.full(n, nan)
            for i in range(n):
                if np.isnan(cat.vcd[i]):
                    continue
                args = (cat.ctm_p[:, i], cat.ctm_y[:, i], cat.sat_p[:, i], cat.ak[:, i], cat.ap_prof[:, i], cat.pw[:, i])
                x, s = gosat_pixel(*args, shift=shift)
                if pixels is not None:
                    x = pixels(*args)
                mx[i], s_x[i] = x, s
            mx[np.isinf(cat.vcd)] = nan
            out["model_xcol"] = (mx, s_x)
    return out


def compare(got, ref, scale, tol, check_values=None):
    """The three assertions of the suite on one output array -> (list of failing columns, largest |got-ref|/scale).
    NaN pattern equal, inf pattern equal with its sign, |got - ref| <= tol * max(scale, |ref|) where both are finite;
    `check_values` (bool per column) switches the third one off for the pattern-only columns."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = set(np.flatnonzero(np.isnan(got) != np.isnan(ref)))
    bad |= set(np.flatnonzero((np.isposinf(got) != np.isposinf(ref)) | (np.isneginf(got) != np.isneginf(ref))))
    fin = np.isfinite(got) & np.isfinite(ref)
    if check_values is not None:
        fin &= check_values
    with np.errstate(all="ignore"):
        sc = np.fmax(np.where(np.isfinite(scale), scale, 0.0), np.abs(ref))
        dist = np.where(fin & (sc > 0), np.abs(got - ref) / np.where(sc > 0, sc, 1.0), 0.0)
        dist = np.where(fin & (sc == 0) & (got != ref), np.inf, dist)
    bad |= set(np.flatnonzero(dist > tol))
    return sorted(int(b) for b in bad), float(dist.max()) if dist.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# building
# ---------------------------------------------------------------------------------------------------------------
SHIFTS = ((1, -1), (-1, 1))      # (nodes, queries): opposite directions, so that the two ulps add up instead of cancelling


def well_conditioned(cat, bar=RT64):
    """bool per column: with every logarithm moved by one ulp (nodes one way, queries the other, both ways round) each
    output either changes its NaN / inf pattern -- a query exactly on a node -- or stays within half the bar"""
    base = reference(cat)
    ok = np.ones(cat.n, dtype=bool)
    exempt = np.array([t in TIE_JUMP_TAGS for t in cat.tags])     # discontinuous at the tie on purpose
    for sh in SHIFTS:
        moved = reference(cat, shift=sh)
        for nm, (r, s) in base.items():
            m = moved[nm][0]
            same = (np.isnan(r) == np.isnan(m)) & (np.isposinf(r) == np.isposinf(m)) & (np.isneginf(r) == np.isneginf(m))
            failing, _ = compare(m, r, s, 0.5 * bar, check_values=same & ~exempt)
            ok[[f for f in failing if same[f]]] = False
    return ok


def _make_column(op, nzs, nzc, T, tag, rep, seed):
    fn = categories(op)[tag][0]
    for attempt in range(60):
        rng = np.random.default_rng([seed, OPS.index(op), nzs, nzc, np.dtype(T).itemsize, rep, attempt, zlib.crc32(tag.encode())])
        c = _Col(op, rng, nzs, nzc, T)
        if not tag.startswith("order"):
            c.reorder(rng, ("desc", "asc", "shuffled")[rep % 3])
        try:
            fn(c, rng, rep)
        except _Retry:
            continue
        if not (spacing_ok(c.sat_p) and spacing_ok(c.ctm_p)):
            continue
        if well_conditioned(Catalogue(op, nzs, nzc, T, [c], [tag]))[0]:
            return c
    raise RuntimeError(f"no well-conditioned column for {op} {tag} nzs={nzs} nzc={nzc} {np.dtype(T).name}")


@functools.lru_cache(maxsize=None)
def catalogue(op, nzs, nzc, dtype, seed=20261018, reps=REPS):
    T = np.dtype(dtype).type
    cols, tags = [], []
    for tag in required_tags(op, nzs, nzc):
        for rep in range(reps // 2 if tag in NAN_NODE_TAGS else reps):
            cols.append(_make_column(op, nzs, nzc, T, tag, rep, seed))
            tags.append(tag)
    order = np.random.default_rng(seed).permutation(len(cols))       # so that the first 127..129 columns mix the categories
    return Catalogue(op, nzs, nzc, T, [cols[i] for i in order], [tags[i] for i in order])
