"""Seeded catalogues for the element-wise OI entry points of csrc/oi_diag.hip (oisat_oi_curve / _apply / _fused / _variances)
and the averaging entry points of csrc/averaging.hip (oisat_nanmean_stack / _error_average / _month_accumulate / _month_finish /
_all_nan / _widen), and the plain references they are judged by (tests/test_gpu_elementwise_abi.py on the device,
tests/test_elementwise_cases_cpu.py here).  NumPy only; nothing in this file touches the GPU.

A. sweep -- ``sweep_scene(name)`` = (dtype, n, scale table, Sa, So).  Reference (a) ``sweep_reference`` is the kernel's own form
   in the scene's dtype (t = Sa*s, k = t*(1/(t+So)), dropped where t == 0 or k is NaN), summed EXACTLY (``exact_sum``) and divided
   by the exact count: a Fraction per scaling.  Reference (b) is oracle.oi_curve, the reference's 1 - Sb/t form (float64).
   Bars (``sweep_compare``), derived not measured: the device adds at most D = 32 ceil(n / 262144) + 32 doubles in sequence per
   mean (32 cells per lane and stripe pass, eight LDS rows, four block partials per thread, an eight-level tree; the xor tree
   of scalings >= 96 is shorter), so |got - mean| <= D 2^-53 sum|ak| / count + 2^-53 |got| (the division's rounding).  Against
   (b), on scenes with Sa, So >= 0 where 0 <= K <= 1: 1.5 2^-52 absolute on top -- fl(1 - K) errs by at most 2^-54, the product
   with t and the division by t are two relative roundings of a value <= 1 (2^-52), the last subtraction 2^-54.  Counts are
   exact; NaN and +-inf means agree in kind.
B. knee -- ``knee_scene(name)``: 14 tables x 9 variance ratios, the degenerate curves that must give index 0, and the small-K
   scenes where the reference-form curve's own rounding noise has a knee the K-form curve has not.
C. apply / variances -- ``apply_inputs``; reference oracle.oi_fields on arrays of the scene's dtype: same bits.
D. stack / month -- ``stack_scene`` and ``month_scene``; reference an explicit loop over the granules in the dtype
   (``stack_reference``, ``month_reference``): the ORDER is the contract, so np.nanmean is not the yardstick.  Same bits.

Every reference takes ``mutate=``: a deliberately wrong restatement (a dropped tail cell, two scalings exchanged, a skipped
stripe, inf counted as valid, the granules summed backwards, the square taken after the validity test).  The CPU test checks
that the catalogue's own comparison rejects each of them: that is how the catalogues are known to be sharp.
"""
import functools
from fractions import Fraction

import numpy as np

from oracle import oi_oracle as orc
from oisatgmi._kneedle import knee_index

SEED = 5
DTYPES = (np.float64, np.float32)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1e-300, 1e300, 5e-324])   # test_oi_special_values_against_oracle
MAX_SCALES = 128
MAIN_SCALES = 96                            # oi_curve_kernel: three scalings per lane and half-wave; the rest lane == cell
STRIPE = 1024 * 256                         # kCurveBlocks * kCurveThreads cells per pass of the sweep's stripe loop
STREAM_PASS = 2048 * 256                    # stream_grid(n, 256): elements (or vectors) per pass of a grid-stride loop
U64 = Fraction(1, 2 ** 53)


def dt_name(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _dt(name):
    return np.dtype(np.float64 if name.startswith("f64") else np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# A. the sweep
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_NS = (1, 2, 63, 64, 65, 127, 129, STRIPE - 1, STRIPE, STRIPE + 1, STRIPE + 65)
SWEEP_SCALES = (1, 2, 3, 31, 32, 33, 64, 95, 96, 97, 99, 127, 128)
SWEEP_EVERY_N = (1, 33, 97, 99, 128)        # every n meets these scale counts ...
SWEEP_EVERY_S = (1, 65, STRIPE + 1)         # ... and every scale count these n
SWEEP_SPECIALS = ((1031, 99), (4099, 128), (129, 3))
ZERO_SCALE_AT = (33, 5)                     # the 33-point table carries an exact 0.0 here: count 0, mean NaN
TINY64 = (1e-320, 5e-324, 1.5e-323)         # float64 Sa on a few cells: t = Sa*s underflows to 0 for the small scalings only
TINY32 = (1e-42, 1.4e-45, 4.2e-45)          # the same in float32 (denormals)


def sweep_pairs():
    pairs = [(n, s) for n in SWEEP_NS for s in SWEEP_EVERY_N]
    pairs += [(n, s) for s in SWEEP_SCALES for n in SWEEP_EVERY_S if (n, s) not in pairs]
    return pairs


def sweep_scene_names(family="all"):
    names = []
    for dt in DTYPES:
        if family in ("all", "main"):
            names += [f"{dt_name(dt)}-n{n}-s{s}" for n, s in sweep_pairs()]
        if family in ("all", "specials"):
            names += [f"{dt_name(dt)}-specials-n{n}-s{s}" for n, s in SWEEP_SPECIALS]
    return names


def geometric_table(nscales):
    """non-uniform, all distinct: a swapped scaling moves its mean"""
    return 0.02 * 1.07 ** np.arange(nscales)


class SweepScene:
    def __init__(self, name, dtype, table, Sa, So, specials):
        self.name, self.dtype, self.specials = name, np.dtype(dtype), specials
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        self.Sa, self.So = np.ascontiguousarray(Sa, dtype=dtype), np.ascontiguousarray(So, dtype=dtype)

    @property
    def n(self):
        return self.Sa.size

    @property
    def nscales(self):
        return self.table.size

    @property
    def nonnegative(self):
        """0 <= K <= 1 wherever it counts: the scenes reference (b)'s bar is derived for"""
        return not self.specials


@functools.lru_cache(maxsize=8)
def sweep_scene(name):
    parts = name.split("-")
    dtype, specials = _dt(parts[0]), parts[1] == "specials"
    n, ns = int(parts[-2][1:]), int(parts[-1][1:])
    rng = np.random.default_rng([SEED, 1, n, ns, int(specials), dtype.itemsize])
    table = geometric_table(ns)
    if specials:
        Sa, So = rng.uniform(0.01, 25.0, size=n), rng.uniform(0.01, 1.0, size=n)
        for a in (Sa, So):
            hit = np.flatnonzero(rng.uniform(size=n) < 0.15)
            a[hit] = SPECIALS[np.arange(hit.size) % SPECIALS.size][rng.permutation(hit.size)]   # every special, n >= 129
        return SweepScene(name, dtype, table, Sa, So, True)
    if ns == ZERO_SCALE_AT[0]:
        table[ZERO_SCALE_AT[1]] = 0.0
    Sa = rng.uniform(0.5, 2.0, size=n) * 10.0 ** rng.uniform(-1.0, 1.0, size=n)
    So = rng.uniform(0.5, 2.0, size=n)
    Sa, So = Sa.astype(dtype), So.astype(dtype)
    i = np.arange(n)
    tiny = TINY64 if dtype == np.float64 else TINY32                     # counts depend on the scaling ...
    for j, v in enumerate(tiny):
        Sa[i % 53 == 2 + 9 * j] = dtype.type(v)
    So[i % 7 == 3] = np.nan                                              # ... and on the cell
    Sa[i % 11 == 5] = 0
    return SweepScene(name, dtype, table, Sa, So, False)


def exact_sum(v):
    """the exact sum of finite float64 values, a Fraction: mantissas as integers, binned by exponent"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.size == 0:
        return Fraction(0)
    assert np.isfinite(v).all() and v.size < 2 ** 26
    b = v.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    mi = (b & np.uint64(0xFFFFFFFFFFFFF)).astype(np.int64)
    mi |= (e > 0).astype(np.int64) << 52                                 # the implicit bit of a normal number
    np.maximum(e, 1, out=e)                                              # v = +-mi 2^(e - 1075), denormals included
    mi = np.where(b >> np.uint64(63), -mi, mi)
    hi, lo = mi >> 26, mi & 0x3FFFFFF                                    # mi = hi 2^26 + lo with lo >= 0
    H = np.bincount(e, weights=hi.astype(np.float64))                   # |hi| < 2^27 and fewer than 2^26 terms: exact in float64
    L = np.bincount(e, weights=lo.astype(np.float64))
    total = 0
    for j in np.flatnonzero((H != 0) | (L != 0)):
        total += ((int(H[j]) << 26) + int(L[j])) << int(j)
    return Fraction(total) * Fraction(2) ** -1075


def sweep_ak(sc, s, form="K"):
    """the averaging kernel of every cell for one scaling, in the scene's dtype: the kernel's form (ak_of) or the reference's"""
    T = sc.dtype.type
    with np.errstate(all="ignore"):
        t = sc.Sa * T(s)
        k = t * (T(1) / (t + sc.So))
        if form == "K":
            return np.where(t == 0, T(np.nan), k)
        sb = (T(1) - k) * t
        return T(1) - sb / t


class SweepRef:
    """per scaling: the exact count, the kind of the mean (finite / nan / +inf / -inf), the exact mean and sum|ak| (finite kind)"""

    def __init__(self, n):
        self.n, self.count, self.kind, self.mean, self.abs_sum = n, [], [], [], []

    def add(self, vals):
        vals = np.asarray(vals, dtype=np.float64)
        self.count.append(int(vals.size))
        pos, neg = bool(np.isposinf(vals).any()), bool(np.isneginf(vals).any())
        if vals.size == 0 or (pos and neg):
            kind = "nan"
        elif pos or neg:
            kind = "+inf" if pos else "-inf"
        else:
            kind = "finite"
        self.kind.append(kind)
        total = exact_sum(vals) if kind == "finite" else None
        self.mean.append(total / vals.size if kind == "finite" else None)
        self.abs_sum.append((total if (vals >= 0).all() else exact_sum(np.abs(vals))) if kind == "finite" else None)

    def mean_float(self):
        special = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
        return np.array([float(m) if k == "finite" else special[k] for m, k in zip(self.mean, self.kind)])


def sweep_reference_of(sc, form="K", mutate=None):
    ref = SweepRef(sc.n)
    table = sc.table.copy()
    if mutate == "swap_96_97":
        table[[96, 97]] = table[[97, 96]]
    keep = np.ones(sc.n, bool)
    if mutate == "drop_odd_tail" and sc.n % 2:
        keep[-1] = False
    if mutate == "skip_second_stripe":
        keep[STRIPE:2 * STRIPE] = False
    for s in table:
        ak = sweep_ak(sc, s, form)
        ak = ak if mutate is None else ak[keep]
        ref.add(ak[~np.isnan(ak)])
    return ref


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """reference (a) of a scene (cached: the references are computed once and left unchanged)"""
    return sweep_reference_of(sweep_scene(name))


def sweep_depth(n):
    return 32 * -(-n // STRIPE) + 32


def sweep_compare(ref, mean, count, extra_abs=0.0):
    """(indices that miss, largest |mean - ref| / bar over the finite means) of a float64 curve and its counts against a
    SweepRef; extra_abs = 1.5 2^-52 for the reference-form curve"""
    mean, count = np.asarray(mean, dtype=np.float64), np.asarray(count)
    assert mean.shape == count.shape == (len(ref.count),)
    D = sweep_depth(ref.n)
    bad, worst = [], 0.0
    for i, (c, kind, m, a) in enumerate(zip(ref.count, ref.kind, ref.mean, ref.abs_sum)):
        if int(count[i]) != c:
            bad.append(i)
        elif kind != "finite":
            ok = np.isnan(mean[i]) if kind == "nan" else mean[i] == (np.inf if kind == "+inf" else -np.inf)
            if not ok:
                bad.append(i)
        elif not np.isfinite(mean[i]):
            bad.append(i)
        else:
            got = Fraction(float(mean[i]))
            bar = D * U64 * a / c + U64 * abs(got) + Fraction(extra_abs)
            dist = abs(got - m)
            if dist > bar:
                bad.append(i)
            if bar > 0:
                worst = max(worst, float(dist / bar))
    return bad, worst


REF_FORM_ABS = 1.5 * 2.0 ** -52


def sweep_bars(ref, mean, extra_abs=0.0):
    """the bar of sweep_compare around `mean` as floats (NaN where the reference mean is not finite): for judging a curve
    against another float64 curve, oracle.oi_curve"""
    D = sweep_depth(ref.n)
    term = [float(D * U64 * a / c) if k == "finite" else np.nan for c, k, a in zip(ref.count, ref.kind, ref.abs_sum)]
    return np.array(term) + 2.0 ** -53 * np.abs(np.asarray(mean, dtype=np.float64)) + extra_abs


# ---------------------------------------------------------------------------------------------------------------------
# B. the knee
# ---------------------------------------------------------------------------------------------------------------------
KNEE_RATIOS = (1e-3, 1e-2, 0.1, 0.3, 1.0, 3.0, 10.0, 100.0, 1e3)
KNEE_CELLS = 1000
UNIFORM99 = np.arange(0.1, 10, 0.1)         # optimal_interpolation.py:15-20


def knee_tables():
    t = {"uniform99": UNIFORM99, "geometric128": geometric_table(128), "geometric33": geometric_table(33)}
    for k in (3, 4, 8, 9, 10, 16, 17, 18):  # numpy_sum_small changes shape at n - 1 = 7, 8, 9, 15, 16, 17
        t[f"linspace{k}"] = np.linspace(0.1, 10, k)
    t["uniform96"], t["uniform97"] = np.linspace(0.1, 10, 96), np.linspace(0.1, 10, 97)
    rng = np.random.default_rng([SEED, 2])
    t["jittered64"] = np.sort(np.linspace(0.1, 10, 64) + rng.uniform(-0.07, 0.07, size=64))
    return t


KNEE_DEGENERATE = ("equal_adjacent", "flat", "all_nan", "nan_mean", "one_scale", "two_scales")
SMALL_K = ("small_k-1e-10", "small_k-1e-12")
SMALL_K_CELLS = 4096
# knee_index(table, curve) of the two curve forms on the small-K scenes, None as 0: (K form = the device's, reference form).
# For Sa/So ~ 1e-10 the reference's 1 - Sb/t carries 1e-16 of rounding noise on means of 1e-10 .. 1e-8: the noise has a knee,
# the smooth K-form curve has none.
SMALL_K_INDICES = {"small_k-1e-10": (0, 20), "small_k-1e-12": (0, 77)}


def knee_scene_names(family="main"):
    if family == "main":
        return [f"{t}-r{r:g}" for t in knee_tables() for r in KNEE_RATIOS]
    return list(KNEE_DEGENERATE if family == "degenerate" else SMALL_K)


@functools.lru_cache(maxsize=None)
def knee_scene(name):
    """float64 scenes (SweepScene) for oisat_oi_fused"""
    pw = 2.0 ** (np.arange(KNEE_CELLS) % 8 - 4)
    rng = np.random.default_rng([SEED, 3])
    if name in KNEE_DEGENERATE:
        Sa, So = rng.uniform(0.5, 2.0, size=KNEE_CELLS), rng.uniform(0.5, 2.0, size=KNEE_CELLS)
        table = np.linspace(0.1, 10, 20)
        if name == "equal_adjacent":
            table[7] = table[6]
        elif name == "flat":                                             # t a power of two: t (1/t) = 1 exactly, every mean 1.0
            Sa, So, table = pw, np.zeros(KNEE_CELLS), 2.0 ** np.arange(-3, 4)
        elif name == "all_nan":
            Sa = np.zeros(KNEE_CELLS)
        elif name == "nan_mean":
            table[9] = 0.0
        elif name == "one_scale":
            table = table[3:4]
        elif name == "two_scales":
            table = table[3:5]
        return SweepScene(name, np.float64, table, Sa, So, False)
    if name in SMALL_K:
        r = float(name.split("-", 1)[1])
        rng = np.random.default_rng([SEED, 4])
        So = rng.uniform(0.5, 2.0, size=SMALL_K_CELLS)
        return SweepScene(name, np.float64, UNIFORM99, rng.uniform(0.5, 2.0, size=SMALL_K_CELLS) * r, So, False)
    tname, r = name.rsplit("-r", 1)
    tables = knee_tables()
    rng = np.random.default_rng([SEED, 5, list(tables).index(tname), KNEE_RATIOS.index(float(r))])
    Sa = rng.uniform(0.5, 2.0, size=KNEE_CELLS) * float(r)
    return SweepScene(name, np.float64, tables[tname], Sa, rng.uniform(0.5, 2.0, size=KNEE_CELLS), False)


def knee_curve(sc, form="K"):
    """the float64 curve of a knee scene on the CPU (np.nanmean: the device's differs in the last bits, the test on the device
    judges the device's pick on the device's own curve)"""
    out = []
    for s in sc.table:
        ak = sweep_ak(sc, s, form)
        ak = ak[~np.isnan(ak)]
        out.append(np.mean(ak) if ak.size else np.nan)
    return np.array(out)


def host_knee(table, curve):
    """the product's host pick, None as index 0 (optimal_interpolation.py:39-41)"""
    k = knee_index(table, curve)
    return 0 if k is None else int(k)


def oracle_knee(table, curve):
    if len(table) < 3:
        return 0
    k = orc.kneedle_knee(np.asarray(table), np.asarray(curve))[1]
    return 0 if k is None else int(k)


# ---------------------------------------------------------------------------------------------------------------------
# C. apply and variances
# ---------------------------------------------------------------------------------------------------------------------
APPLY_NS = (1, 3, 255, 257, STREAM_PASS + 1)
APPLY_SCALES = (1.0, 0.1, 3.7)
VARIANCE_PCTS = (50.0, 0.1, 1e3)


@functools.lru_cache(maxsize=4)
def apply_inputs(n, dtype):
    """Xa, Y, Sa, So of the scene's dtype with the nine specials in all four at 15 %"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([SEED, 6, n, dtype.itemsize])
    out = []
    for lo, hi in ((0.2, 10.0), (-1.0, 10.0), (0.01, 25.0), (0.01, 1.0)):
        a = rng.uniform(lo, hi, size=n)
        hit = np.flatnonzero(rng.uniform(size=n) < 0.15)
        a[hit] = rng.choice(SPECIALS, size=hit.size)
        if n >= 255:
            a[rng.choice(n, size=SPECIALS.size, replace=False)] = SPECIALS         # every special, whatever the draw
        a = a.astype(dtype)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def apply_reference(Xa, Y, Sa, So, scale):
    """(Y clamped in place as optimal_interpolation.py:14 does, Xb, AK, inc, err) by oracle.oi_fields in the arrays' dtype"""
    T = Xa.dtype.type
    Yc = Y.copy()
    with np.errstate(all="ignore"):
        Yc[Yc < 0] = 0
        xb, ak, inc, err = orc.oi_fields(Xa, Yc, Sa, So, T(scale))
    assert all(a.dtype == Xa.dtype for a in (xb, ak, inc, err))
    return Yc, xb, ak, inc, err


def variances_reference(Xa, e, pct):
    T = Xa.dtype.type
    with np.errstate(all="ignore"):
        return ((Xa * T(pct)) / T(100)) ** 2, e * e


# ---------------------------------------------------------------------------------------------------------------------
# D. stacks and months
# ---------------------------------------------------------------------------------------------------------------------
STACK_KS = (1, 2, 31, 450)
STACK_NS = (1, 2, 3, 4, 5, 1023, 1024, 1025)


def stack_big_n(dtype):
    """one vector beyond a full grid pass of the vector path (k = 2 only)"""
    return 4 * STREAM_PASS + 4 if np.dtype(dtype) == np.float32 else 2 * STREAM_PASS + 2


def stack_cases(dtype):
    return [(k, n) for k in STACK_KS for n in STACK_NS] + [(2, stack_big_n(dtype))]


@functools.lru_cache(maxsize=4)
def stack_scene(k, n, dtype, field=0):
    """[k, n] of dtype: 15 % NaN, 3 % +inf, 3 % -inf; the first cells NaN in every granule; one cell with a single valid
    granule; float32: some values up to 1e25, whose squares overflow and must be dropped"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([SEED, 7, k, n, dtype.itemsize, field])
    a = rng.uniform(-0.5, 2.0, size=(k, n))
    if dtype == np.float32:
        big = rng.uniform(size=(k, n)) < 0.06
        a[big] *= 10.0 ** rng.uniform(15.0, 25.0, size=int(big.sum()))
    u = rng.uniform(size=(k, n))
    a[u < 0.15] = np.nan
    a[(u >= 0.15) & (u < 0.18)] = np.inf
    a[(u >= 0.18) & (u < 0.21)] = -np.inf
    a[:, :min(5, n // 2)] = np.nan
    lone = min(5, n - 1)
    a[:, lone] = np.nan
    a[k // 2, lone] = 0.75
    a = a.astype(dtype)
    a.setflags(write=False)
    return a


def _accumulate(s, c, v, kind, flag, mutate=None):
    """one granule into the running (sum, count), as accum<T, ERR> does: kind 'err': flag = square_input, NaN and inf dropped;
    kind 'mean': flag = inf_to_nan, NaN dropped, inf too when flagged"""
    with np.errstate(all="ignore"):
        if kind == "err":
            sq = v * v if flag else v
            if mutate == "square_after_test":
                ok = ~np.isnan(v) & ~np.isinf(v)
            elif mutate == "count_inf":
                ok = ~np.isnan(sq)
            else:
                ok = ~np.isnan(sq) & ~np.isinf(sq)
            v = sq
        else:
            ok = ~np.isnan(v) & ~(np.isinf(v) if flag else np.zeros(v.shape, bool))
        s[ok] = (s + v)[ok]
        c[ok] += 1


def _finish(s, c, kind):
    cT = c.astype(s.dtype)
    with np.errstate(all="ignore"):
        return np.sqrt(s / (cT * cT)) if kind == "err" else s / cT


def stack_reference(stack, kind, flag, mutate=None):
    """sum += v over the granules IN ORDER where valid, cnt += 1; then sum / cnt, or sqrt(sum / (cnt cnt)), cnt cast to the dtype"""
    k, n = stack.shape
    s, c = np.zeros(n, stack.dtype), np.zeros(n, np.uint32)
    for g in (range(k - 1, -1, -1) if mutate == "reverse_k" else range(k)):
        _accumulate(s, c, stack[g], kind, flag, mutate)
    return _finish(s, c, kind)


def same_bits(got, ref):
    """NaN in the same places, the same bits elsewhere (-0.0 is not 0.0)"""
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    u = np.uint32 if ref.dtype == np.float32 else np.uint64
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], ref.view(u)[~nan]))


MONTH_K = 31
MONTH_FIELDS = (("mean", True), ("err", True), ("mean", False), ("mean", False), ("mean", False))   # kind, flag of field f
MONTH_F32_MASK = 0b01101                    # vcd, ctm_vcd, new_amf float32; uncertainty, old_amf float64
MONTH_SKIPPED = (0, 15)                     # granules whose kept word is 0


def month_scene(n):
    """five [MONTH_K, n] stacks of mixed dtypes (bit f of MONTH_F32_MASK: float32) and the kept words"""
    fields = [stack_scene(MONTH_K, n, np.float32 if (MONTH_F32_MASK >> f) & 1 else np.float64, field=f) for f in range(5)]
    kept = np.ones(MONTH_K, np.int32)
    kept[list(MONTH_SKIPPED)] = 0
    return fields, kept


def month_reference(fields, kept, acc_dtype, upto=None):
    """(sums [5, n] of acc_dtype, counts [5, n] uint32, finished [5, n]) after the first `upto` granules (all by default): the
    same loop as stack_reference, granule by granule, each value converted to acc_dtype first; skipped granules do nothing"""
    k, n = fields[0].shape
    s, c = np.zeros((5, n), acc_dtype), np.zeros((5, n), np.uint32)
    for g in range(k if upto is None else upto):
        if kept[g]:
            for f, (kind, flag) in enumerate(MONTH_FIELDS):
                with np.errstate(all="ignore"):
                    v = fields[f][g].astype(acc_dtype)
                _accumulate(s[f], c[f], v, kind, flag)
    return s, c, np.stack([_finish(s[f], c[f], MONTH_FIELDS[f][0]) for f in range(5)])


ALL_NAN_NS = (1, 255, 256, 257, STREAM_PASS + 1)
ALL_NAN_CASES = ("all_nan", "last", "minus_zero", "plus_inf", "minus_inf")


def all_nan_case(case, n, dtype):
    """(x, expected kept word): all NaN, or one non-NaN value -- the last element, or a -0.0 / +-inf somewhere"""
    x = np.full(n, np.nan, dtype=dtype)
    if case == "all_nan":
        return x, 0
    at = n - 1 if case == "last" else (n * 2) // 3
    x[at] = {"last": 1.5, "minus_zero": -0.0, "plus_inf": np.inf, "minus_inf": -np.inf}[case]
    return x, 1


def widen_input(n):
    """float32 bit patterns: denormals, +-0, +-inf, NaNs, the largest and smallest normals, then random bits"""
    rng = np.random.default_rng([SEED, 8, n])
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00400000], dtype=np.uint32)
    m = min(n, edge.size)
    bits[:m] = edge[:m]
    if n > 2 * edge.size:
        bits[-edge.size:] = edge
    return bits.view(np.float32)
