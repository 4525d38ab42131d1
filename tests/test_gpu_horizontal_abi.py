"""The horizontal regridding operators of csrc/regrid.hip (and the two element-wise calls of csrc/oi_diag.hip that share their
stage), called at the C ABI on the seeded catalogues of tests/horizontal_cases.py and judged by plain references: brute
force for the neighbour search, scipy's convolve2d for the box filter, np.linalg.solve / RBFInterpolator for the local
thin-plate splines, LinearNDInterpolator / Delaunay.find_simplex for the triangulated interpolation, NumPy in the same dtype
for the element-wise kernels.  Every output buffer is followed by 64 sentinels that must survive; one launch carries a whole
scene; nothing is skipped at run time.

Bars.  Neighbour search: indices equal, distances bit-equal.  Box filter: (win + 2) u sum|Z w| (horizontal_cases: the
summation bound for any order).  RBF: RBF_TOL sum|w_q v_q| = 8 x the distance between the two CPU references, plus one
float32 rounding of the result for float32 fields.  Linear: 1e-12 sum|c_k v_k| (the project's float64 bar), plus one float32
rounding for float32 fields.  Element-wise: same bits.

Planned exclusion: a target that lies on a shared facet or vertex (the kernel reports it in amb_list) takes its value from
whichever simplex the walk meets; where one of those simplices has a NaN vertex the NaN pattern depends on that choice
(include/oisat.h says so), and the NaN-vertex field is judged there only if no accepting simplex holds the NaN.  The value
of such a target agrees between the simplices only to scipy's own eps: its bar carries 6 eps max|v| on top (derived in
test_linear_interp_catalogue).  Generic targets keep the plain bar.

What the catalogues found, and what became of it:
  * oisat_nn_query / _ties: with the hash cell equal to the mask radius, a target a few ulp from a cell border and a point
    0.99999.. max_dist further on are hashed two cells apart and the point is never looked at: -1 where brute force keeps
    the target.  All 80 ``border_ulp`` targets (10 scenes) came back -1 on the parent commit's library on an MI355X, as the
    NumPy emulation of the unpadded search predicts; every other scene passed there.  Fixed: the cell is the radius padded
    by 2^-26 (nn_query_impl derives the pad from the largest cell coordinate the 4 Mi-cell cap allows) and a target one cell
    past the far edge looks from the edge's neighbour, where clamped points live.  include/oisat.h now states the mask
    (`not dist > max_dist`) and what NaN coordinates do.
  * pick_impl: the G = 16 and G = 4 branches could not be reached (kx <= 64 with three or more nodes goes to the row-wise
    kernel): deleted.  The live paths (row-wise, G = 64 for kx > 64, G = 1 for one or two nodes) are all in BOX_WINDOWS.
  * oisat_linear_interp on the swath grid (a regular lattice whose latitudes carry 1e-13 of noise: 9 NaN transforms): two
    targets ON the hull's straight edge are inside for LinearNDInterpolator and outside for the library, or the reverse, and
    neither is reported by oisat_linear_locate.  Not a kernel fault: the hull there is closed by zero-area slivers, the
    triangulation is not a partition to rounding, and scipy's own two searches disagree on one of the two; the walk takes
    the first hull facet it crosses as "outside" from wherever it starts.  Pinned as the documented behaviour
    (include/oisat.h; test_linear_hull_grazing_targets_follow_the_walk_from_the_nearest_point): on every target the library
    answers as the NumPy restatement of its walk does.  Generic targets there still match scipy; two of them are reported
    because their walk starts in a NaN-transform simplex and falls back to the scan, as the header says.
  * Targets on a shared facet or vertex agree with scipy only to scipy's eps times the largest vertex value (a field with six
    decades of magnitude shows 1e-12 of the scale): that is the interpolant's own ambiguity, the bar for reported targets
    carries it.
  * RBF, box filter, pick, gather, mask and the element-wise calls: no divergence.  RBF float64 within 5.2e-13 of
    np.linalg.solve in the bar's measure (RBF_DEVICE_MEASURED; the bar is 4.2e-12), box filter within 0.47 of its bar.
  * The issue's ``coarsened`` scene (360 x 180 degrees against 1e-3) fills 967 scan tiles, not "more than 1 000";
    ``coarsened_1000`` (9.75e-4) fills 1 017.  Both pass.
  * max_dist = 1.5 against the dyadic origins -180 / -179.875 has no border_ulp case at all (every product is exact; the CPU
    test searches and finds none), so those two of the twelve (max_dist, origin) pairs have no scene.
"""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.interpolate import LinearNDInterpolator, RBFInterpolator

pytestmark = pytest.mark.gpu

from oisatgmi import _hip
import horizontal_cases as hc

PAD, SENTINEL = 64, 12345.678
DTYPES = (np.float64, np.float32)
DT_IDS = ["f64", "f32"]
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    return c


class _Out:
    """an output array of n elements followed by PAD sentinels: the grid's tail must not write past n"""

    def __init__(self, ctx, n, dtype=np.float64):
        self.ctx, self.n, self.dtype = ctx, int(n), np.dtype(dtype)
        self.buf = ctx.upload(np.full(self.n + PAD, SENTINEL, dtype=self.dtype))
        self.ptr = self.buf.ptr
        self.fill = self.dtype.type(SENTINEL)

    def get(self):
        self.ctx.sync()
        a = self.ctx.download(self.ptr, (self.n + PAD,), self.dtype)
        assert (a[self.n:] == self.fill).all(), "wrote past the last element"
        return a[:self.n]


def _up(ctx, a, dtype=np.float64):
    return ctx.upload(np.ascontiguousarray(a, dtype=dtype))


def _same_bits(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    u = np.uint32 if ref.dtype == np.float32 else np.uint64
    diff = np.flatnonzero(got.view(u)[~nan] != ref.view(u)[~nan])
    assert diff.size == 0, (diff[:5], got[~nan][diff[:5]], ref[~nan][diff[:5]])


def _list(out, count, limit):
    """a device list of `count` entries in a sentinel-filled buffer: the entries, sorted; nothing written behind them"""
    raw = out.get()
    assert 0 <= count <= limit, count
    assert (raw[count:] == out.fill).all(), "entries behind the reported count"
    ids = np.sort(raw[:count])
    assert np.unique(ids).size == ids.size, "an id listed twice"
    return ids


# ---- A. nearest neighbour ----------------------------------------------------------------------------------------------
def run_nn(ctx, sc, ties, want_dist=True):
    b = [_up(ctx, a) for a in (sc.px, sc.py, sc.tx, sc.ty)]
    idx = _Out(ctx, sc.T, np.int32)
    dist = _Out(ctx, sc.T) if want_dist else None
    dptr = dist.ptr if want_dist else None
    tie = None
    if ties:
        tl, n = _Out(ctx, sc.T, np.int32), C.c_int64(-7)
        ctx.check(ctx.lib.oisat_nn_query_ties(ctx.h, b[0].ptr, b[1].ptr, sc.P, b[2].ptr, b[3].ptr, sc.T, sc.max_dist, idx.ptr, dptr,
                                              tl.ptr, C.byref(n)))
        tie = _list(tl, n.value, sc.T)
    else:
        ctx.check(ctx.lib.oisat_nn_query(ctx.h, b[0].ptr, b[1].ptr, sc.P, b[2].ptr, b[3].ptr, sc.T, sc.max_dist, idx.ptr, dptr))
    return idx.get(), (dist.get() if want_dist else None), tie


def judge_nn(sc, ref, idx, dist, tie, what):
    msgs = []
    for t in np.flatnonzero(idx != ref["idx"])[:8]:
        msgs.append(f"idx[{t}] {sc.tags[t]}: got {idx[t]} ref {ref['idx'][t]} (target {sc.tx[t]!r}, {sc.ty[t]!r}; unmasked distance "
                    f"{ref['dist_unmasked'][t]!r}, max_dist {sc.max_dist!r})")
    n_bad = int((idx != ref["idx"]).sum())
    if dist is not None:
        wrong = np.flatnonzero(dist.view(np.uint64) != ref["dist"].view(np.uint64))
        n_bad += wrong.size
        for t in wrong[:8]:
            msgs.append(f"dist[{t}] {sc.tags[t]}: got {dist[t]!r} ref {ref['dist'][t]!r}")
    if tie is not None and not np.array_equal(tie, ref["ties"]):
        n_bad += 1
        msgs.append(f"tie list: got {tie.tolist()} ref {ref['ties'].tolist()}")
    print(f"{what}: P={sc.P} T={sc.T} kept {int((ref['idx'] >= 0).sum())} ties {ref['ties'].size}: {n_bad} wrong")
    assert not msgs, f"{what}: {n_bad} wrong\n" + "\n".join(msgs)


@pytest.mark.parametrize("name", hc.nn_scene_names())
def test_nn_query_ties_catalogue(ctx, name):
    sc = hc.nn_scene(name)
    ref = hc.brute_nn(sc)
    judge_nn(sc, ref, *run_nn(ctx, sc, ties=True), f"nn_query_ties {name}")
    idx, _, tie = run_nn(ctx, sc, ties=True, want_dist=False)                       # dist_out = NULL is accepted
    judge_nn(sc, ref, idx, None, tie, f"nn_query_ties {name} (no dist_out)")


@pytest.mark.parametrize("name", hc.nn_scene_names())
def test_nn_query_catalogue(ctx, name):
    sc = hc.nn_scene(name)
    ref = hc.brute_nn(sc)
    judge_nn(sc, ref, *run_nn(ctx, sc, ties=False), f"nn_query {name}")
    idx, _, _ = run_nn(ctx, sc, ties=False, want_dist=False)
    judge_nn(sc, ref, idx, None, None, f"nn_query {name} (no dist_out)")


def test_nn_query_nan_coordinates_as_the_header_says(ctx):
    """include/oisat.h: a point with a NaN coordinate is never returned and never a tie; a NaN target is -1 / +inf; with no
    finite point every target is"""
    sc = hc.nn_scene("main")
    idx, dist, tie = run_nn(ctx, sc, ties=True)
    nan_pts = np.flatnonzero(np.isnan(sc.px) | np.isnan(sc.py))
    assert nan_pts.size and not np.isin(idx, nan_pts).any()
    w = sc.where("nan_target")
    assert (idx[w] == -1).all() and np.isposinf(dist[w]).all() and not np.isin(w, tie).any()
    w = sc.where("nan_point")
    assert (idx[w] >= 0).all() and not np.isin(w, tie).any()
    idx, dist, tie = run_nn(ctx, hc.nn_scene("all_nan_points"), ties=True)
    assert (idx == -1).all() and np.isposinf(dist).all() and tie.size == 0


# ---- B. box filter, pick, gather, mask, element-wise -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _box_refs(Ny, Nx, ky, kx, dtype, variance, specials):
    Z = hc.box_fields(Ny, Nx, dtype, specials)
    return [hc.box_reference(Z[f], ky, kx, variance) for f in range(3)]


def run_symm(ctx, Z2, ky, kx, variance):
    Ny, Nx = Z2.shape
    zb, out = _up(ctx, Z2, Z2.dtype), _Out(ctx, Ny * Nx, Z2.dtype)
    ctx.check(ctx.lib.oisat_boxfilter_symm(ctx.h, _hip.dtype_code(Z2.dtype), zb.ptr, Ny, Nx, ky, kx, variance, out.ptr))
    return out.get()


def run_pick(ctx, Z3, ky, kx, variance, idx):
    nf, Ny, Nx = Z3.shape
    zb, ib, out = _up(ctx, Z3, Z3.dtype), _up(ctx, idx, np.int32), _Out(ctx, nf * idx.size, Z3.dtype)
    ctx.check(ctx.lib.oisat_boxfilter_pick(ctx.h, _hip.dtype_code(Z3.dtype), zb.ptr, Ny, Nx, nf, ky, kx, variance, ib.ptr, idx.size,
                                           out.ptr))
    return out.get().reshape(nf, idx.size)


def _picked(a, idx):
    return np.where(idx >= 0, np.asarray(a, dtype=np.float64).ravel()[np.maximum(idx, 0)], np.nan)


def check_box(ctx, Ny, Nx, ky, kx, dtype, specials, cases):
    """cases: (nfields, Tn) pairs for the pick; symm runs on all three fields first"""
    Z = hc.box_fields(Ny, Nx, dtype, specials)
    msgs, worst = [], 0.0
    for variance in (0, 1):
        refs = _box_refs(Ny, Nx, ky, kx, dtype, variance, specials)
        symm = []
        for f in range(3):
            got = run_symm(ctx, Z[f], ky, kx, variance)
            assert got.dtype == np.dtype(dtype)
            symm.append(got)
            bad, ratio = hc.compare_bar(got, refs[f][0], refs[f][1])
            worst = max(worst, ratio)
            msgs += [f"symm var={variance} field {f} node {i}: got {got[i]!r} ref {refs[f][0].ravel()[i]!r} bar {refs[f][1].ravel()[i]!r}" for i in bad[:4]]
        for nf, Tn in cases:
            idx = hc.pick_idx(Ny, Nx, Tn)
            fields = [1] if nf == 1 else [0, 1, 2]
            got = run_pick(ctx, Z[fields], ky, kx, variance, idx)
            for k, f in enumerate(fields):
                bar = np.nan_to_num(_picked(refs[f][1], idx), nan=0.0)
                for other, name in ((_picked(refs[f][0], idx), "ref"), (_picked(symm[f], idx), "symm")):
                    bad, ratio = hc.compare_bar(got[k], other, bar)
                    worst = max(worst, ratio)
                    msgs += [f"pick var={variance} nf={nf} Tn={Tn} field {f} target {i} (node {idx[i]}): got {got[k][i]!r} {name} {other[i]!r} "
                             f"bar {bar[i]!r}" for i in bad[:4]]
    print(f"box {Ny}x{Nx} window {ky}x{kx} {np.dtype(dtype).name}: largest |got - ref| / bar = {worst:.3f}")
    assert not msgs, "\n".join(msgs[:24])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ky,kx", hc.BOX_WINDOWS, ids=[f"{a}x{b}" for a, b in hc.BOX_WINDOWS])
def test_boxfilter_symm_and_pick_catalogue(ctx, ky, kx, dtype):
    Ny, Nx = hc.box_shape(ky, kx)
    check_box(ctx, Ny, Nx, ky, kx, dtype, True, [(nf, Tn) for nf in (1, 3) for Tn in hc.pick_tns(kx)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Ny,Nx,ky,kx", hc.BOX_NARROW, ids=[f"{a}x{b}-win{c}x{d}" for a, b, c, d in hc.BOX_NARROW])
def test_boxfilter_grid_narrower_than_the_window(ctx, Ny, Nx, ky, kx, dtype):
    check_box(ctx, Ny, Nx, ky, kx, dtype, False, [(nf, Tn) for nf in (1, 3) for Tn in hc.pick_tns(kx)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_boxfilter_pick_rows_kernel_wraps_its_grid(ctx, dtype):
    Ny, Nx, ky, kx, nf, Tn = hc.BOX_WRAP
    check_box(ctx, Ny, Nx, ky, kx, dtype, True, [(nf, Tn)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_gather_flag_sqrt_affine_scaling_bit_for_bit(ctx, n, dtype):
    """each against the same expression in NumPy, in the same dtype: one rounding per operation, so the same bits"""
    T = np.dtype(dtype).type
    code = _hip.dtype_code(dtype)
    x, y = hc.elementwise_inputs(n, dtype, 3)
    xb, yb = _up(ctx, x, dtype), _up(ctx, y, dtype)
    lib = ctx.lib

    def call(fn, *args, size=n):
        out = _Out(ctx, size, dtype)
        ctx.check(fn(ctx.h, code, *args, out.ptr))
        return out.get()

    with np.errstate(all="ignore"):
        # gather_mask: nfields 1 and 3, idx -1
        rng = np.random.default_rng([n, 9])
        for nf in (1, 3):
            vals = np.stack([x, y, x * T(0.5)])[:nf]
            for Tn in {1, 257, max(n // 3, 1)}:
                idx = rng.integers(-1, n, size=Tn).astype(np.int32)
                idx[0] = -1 if Tn > 1 else n - 1
                vb, ib = _up(ctx, vals, dtype), _up(ctx, idx, np.int32)
                ref = np.where(idx >= 0, vals[:, np.maximum(idx, 0)], T(np.nan)).astype(dtype)
                _same_bits(call(lib.oisat_gather_mask, vb.ptr, n, nf, ib.ptr, Tn, size=nf * Tn).reshape(nf, Tn), ref)
        # flag_mask: flag equal to the threshold (not kept: `>`), NaN flag, square, x = inf
        thresh = 3.5
        flag = y.copy()
        flag[::5] = T(thresh)
        fb = _up(ctx, flag, dtype)
        mask = np.where(flag > T(thresh), T(1), T(np.nan)).astype(dtype)
        assert np.isnan(mask[::5]).all() and (n < 50 or (np.isinf(x).any() and np.isnan(flag).any()))
        _same_bits(call(lib.oisat_flag_mask, xb.ptr, fb.ptr, n, thresh, 0), x * mask)
        _same_bits(call(lib.oisat_flag_mask, xb.ptr, fb.ptr, n, thresh, 1), (x * x) * mask)
        # sqrt: negative inputs and NaN
        assert n < 50 or ((x < 0).any() and np.isnan(x).any())
        _same_bits(call(lib.oisat_sqrt, xb.ptr, n), np.sqrt(x))
        # affine: (x - offset) / slope, offset and slope rounded to the dtype
        for off, slope in ((273.15, 1.8), (0.0, 2.69e16), (-4.0, -0.3)):
            _same_bits(call(lib.oisat_affine, xb.ptr, n, off, slope), (x - T(off)) / T(slope))
        # scaling_factor: 0/0, x/0, inf/inf -> 1
        r = x / y
        ref = np.where(np.isnan(r) | np.isinf(r) | (r == 0), T(1), r).astype(dtype)
        assert n < 50 or (np.isnan(r).any() and np.isinf(r).any() and (r == 0).any())
        _same_bits(call(lib.oisat_scaling_factor, xb.ptr, yb.ptr, n), ref)


# ---- C. thin-plate-spline RBF --------------------------------------------------------------------------------------------
def run_rbf(ctx, sc, dtype, ties):
    v = sc.values(dtype)
    nf = v.shape[0]
    b = [_up(ctx, a) for a in (sc.px, sc.py, sc.tx, sc.ty)]
    nn, vb = _up(ctx, sc.nn_idx, np.int32), _up(ctx, v, dtype)
    out, nsing = _Out(ctx, nf * sc.T, dtype), C.c_int64(-7)
    args = (ctx.h, _hip.dtype_code(dtype), b[0].ptr, b[1].ptr, sc.P, b[2].ptr, b[3].ptr, sc.T, nn.ptr, sc.cell, sc.K, vb.ptr, nf, out.ptr,
            C.byref(nsing))
    tie = None
    if ties:
        tl, nt = _Out(ctx, sc.T, np.int32), C.c_int64(-7)
        ctx.check(ctx.lib.oisat_rbf_interp_ties(*args, tl.ptr, C.byref(nt)))
        tie = _list(tl, nt.value, sc.T)
    else:
        ctx.check(ctx.lib.oisat_rbf_interp(*args))
    return out.get().reshape(nf, sc.T), nsing.value, tie


RBF_CASES = [(kind, K) for kind in hc.RBF_KINDS for K in hc.RBF_KS]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,K", RBF_CASES, ids=[f"{k}-K{K}" for k, K in RBF_CASES])
def test_rbf_interp_catalogue(ctx, kind, K, dtype):
    sc, r = hc.rbf_scene(kind, K), hc.rbf_reference(kind, K)
    P, T = sc.P, sc.T
    v = sc.values(dtype)
    got, nsing, tie = run_rbf(ctx, sc, dtype, ties=True)
    plain, nsing_plain, _ = run_rbf(ctx, sc, dtype, ties=False)
    _same_bits(plain, got)
    ok, sing = r["ok"], r["singular"]
    # ties: the K-th and the (K+1)-th nearest at bit-equal d2, among the evaluated targets; their zero pivots are not counted
    np.testing.assert_array_equal(tie, np.flatnonzero(ok & r["tie"]))
    assert nsing == int((ok & sing & ~r["tie"]).sum()), (nsing, int((ok & sing & ~r["tie"]).sum()))
    assert nsing_plain == int((ok & sing).sum())                                    # without a tie list every zero pivot counts
    # not evaluated (nn_idx = -1) or singular: NaN in every field
    assert np.isnan(got[:, ~ok | sing]).all()
    # neighbourhoods are exact: a non-zero weight only on the brute-force K nearest by (d2, index)
    ev = ok & ~sing
    W = got[:P].T.astype(np.float64)
    assert np.isfinite(W[ev]).all()
    stray = (W != 0) & ~r["nbr"] & ev[:, None]
    assert not stray.any(), [(int(t), sc.tags[t], np.flatnonzero(stray[t]).tolist(), r["ids"][t].tolist()) for t in np.flatnonzero(stray.any(axis=1))[:6]]
    # values: reference A (np.linalg.solve on the documented system) on the value fields as stored
    exp, scale = hc.rbf_expected(r["Wa"], r["nbr"], ok, sing, v[P:])
    bar = hc.RBF_TOL * scale + (U32 * np.abs(np.nan_to_num(exp)) if np.dtype(dtype) == np.float32 else 0.0)
    bad, _ = hc.compare_bar(got[P:], exp, bar)
    fin = np.isfinite(exp) & (scale > 0)
    dist = float((np.abs(got[P:].astype(np.float64) - exp)[fin] / scale[fin]).max()) if fin.any() else 0.0
    print(f"rbf {sc.name} {np.dtype(dtype).name}: T={T} evaluated {int(ev.sum())} ties {tie.size} singular {nsing}; "
          f"max |got - A| / sum|w v| = {dist:.3e} (tol {hc.RBF_TOL:.1e})")
    assert not bad, [(i // T, i % T, sc.tags[i % T], got[P:].ravel()[i], exp.ravel()[i], scale.ravel()[i]) for i in bad[:6]]
    # one NaN value: its neighbourhoods go NaN, no other target does
    holds = r["nbr"][:, np.flatnonzero(np.isnan(v[P + 2]))[0]]
    np.testing.assert_array_equal(np.isnan(got[P + 2]), ~ev | holds)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", hc.RBF_KS)
def test_rbf_interp_forced_on_the_lattice_ties(ctx, K, dtype):
    """the lattice's tied targets with the neighbours scipy's tree names must match RBFInterpolator(neighbors=K); an id
    outside [0, P) leaves its target's sentinel in place, and so does every target that is not listed; a forced row of the
    lattice is a zero pivot: counted, NaN written"""
    sc = hc.rbf_scene("lattice", K)
    tg, ids, W = hc.rbf_forced_case(K)
    assert tg.size >= 8
    P, T, n = sc.P, sc.T, tg.size
    v = sc.values(dtype)[P:P + 2]
    ids = ids.copy()
    ids[0, K - 1], ids[1, 0] = P, -1                                                # two listed targets with an id out of range
    ids[2] = np.arange(K)                                                           # (0,0), (1,0) ..: one row
    b = [_up(ctx, a) for a in (sc.px, sc.py, sc.tx, sc.ty)]
    tb, ib, vb = _up(ctx, tg, np.int32), _up(ctx, ids, np.int32), _up(ctx, v, dtype)
    out, nsing = _Out(ctx, 2 * T, dtype), C.c_int64(-7)
    ctx.check(ctx.lib.oisat_rbf_interp_forced(ctx.h, _hip.dtype_code(dtype), b[0].ptr, b[1].ptr, P, b[2].ptr, b[3].ptr, T, tb.ptr, ib.ptr, n,
                                              K, vb.ptr, 2, out.ptr, C.byref(nsing)))
    got = out.get().reshape(2, T)
    untouched = np.ones(T, bool)
    untouched[tg[2:]] = False
    assert (got[:, untouched] == out.fill).all() and nsing.value == 1 and np.isnan(got[:, tg[2]]).all()
    want = RBFInterpolator(np.column_stack([sc.px, sc.py]), v.astype(np.float64).T, neighbors=K, kernel="thin_plate_spline")(
        np.column_stack([sc.tx[tg[3:]], sc.ty[tg[3:]]])).T
    scale = np.abs(W[3:][None, :, :] * v.astype(np.float64)[:, None, :]).sum(axis=2)
    bar = hc.RBF_TOL * scale + (U32 * np.abs(want) if np.dtype(dtype) == np.float32 else 0.0)
    bad, ratio = hc.compare_bar(got[:, tg[3:]], want, bar)
    print(f"rbf forced K={K} {np.dtype(dtype).name}: {n - 3} tied targets, largest |got - scipy| / bar = {ratio:.3f}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("K", hc.RBF_KS)
@pytest.mark.parametrize("kind", ["generic", "lattice", "lattice_wide"])
def test_rbf_check_masked_counts_the_rows(ctx, kind, K):
    sc, r = hc.rbf_scene(kind, K), hc.rbf_reference(kind, K)
    b = [_up(ctx, a) for a in (sc.px, sc.py, sc.tx, sc.ty)]
    nn, n = _up(ctx, sc.nn_idx, np.int32), C.c_int64(-7)
    ctx.check(ctx.lib.oisat_rbf_check_masked(ctx.h, b[0].ptr, b[1].ptr, sc.P, b[2].ptr, b[3].ptr, sc.T, nn.ptr, sc.cell, K, C.byref(n)))
    want = int((~r["ok"] & r["singular"]).sum())
    print(f"rbf_check_masked {sc.name}: {int((~r['ok']).sum())} masked targets, {want} rows")
    assert n.value == want and (want == 0) == (kind == "generic")


# ---- D. Delaunay linear interpolation ------------------------------------------------------------------------------------
class _Tri:
    def __init__(self, ctx, sc):
        a = sc.arrays()
        self.ns, self.bounds = sc.ns, (C.c_double * 4)(*a["bounds"])
        self.simp, self.neigh = _up(ctx, a["simplices"], np.int32), _up(ctx, a["neighbors"], np.int32)
        self.trans, self.v2s = _up(ctx, a["transform"]), _up(ctx, a["v2s"], np.int32)
        bad = np.where(np.arange(sc.P) % 2 == 0, sc.ns + 3, -5)
        self.v2s_bad = _up(ctx, bad, np.int32)
        self.tx, self.ty, self.nn = _up(ctx, sc.tx), _up(ctx, sc.ty), _up(ctx, sc.nn_idx, np.int32)


def run_linear(ctx, sc, tri, v, bounds=True, bad_v2s=False, forced=None):
    nf, T = v.shape[0], sc.T
    vb, out = _up(ctx, v, v.dtype), _Out(ctx, nf * T, v.dtype)
    args = (ctx.h, _hip.dtype_code(v.dtype), tri.tx.ptr, tri.ty.ptr, T, tri.nn.ptr, (tri.v2s_bad if bad_v2s else tri.v2s).ptr, tri.simp.ptr,
            tri.neigh.ptr, tri.trans.ptr, tri.ns, vb.ptr, sc.P, nf, out.ptr, tri.bounds if bounds else None)
    if forced is None:
        ctx.check(ctx.lib.oisat_linear_interp(*args))
    else:
        fb = _up(ctx, forced, np.int32)
        ctx.check(ctx.lib.oisat_linear_interp_forced(*args, fb.ptr))
    return out.get().reshape(nf, T)


def run_locate(ctx, sc, tri, bounds=True):
    al, n = _Out(ctx, sc.T, np.int32), C.c_int64(-7)
    ctx.check(ctx.lib.oisat_linear_locate(ctx.h, tri.tx.ptr, tri.ty.ptr, sc.T, tri.nn.ptr, tri.v2s.ptr, tri.simp.ptr, tri.neigh.ptr,
                                          tri.trans.ptr, tri.ns, sc.P, tri.bounds if bounds else None, al.ptr, C.byref(n)))
    return _list(al, n.value, sc.T)


def _lin_bar(scale, ref, dtype):
    return hc.RT64 * scale + (U32 * np.abs(np.nan_to_num(ref, posinf=0.0, neginf=0.0)) if np.dtype(dtype) == np.float32 else 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", hc.LINEAR_SCENES)
def test_linear_interp_catalogue(ctx, name, dtype):
    sc = hc.linear_scene(name)
    t, T = sc.tri, sc.T
    tri = _Tri(ctx, sc)
    v = sc.values(dtype)
    v64 = v.astype(np.float64)
    xy = np.column_stack([sc.tx, sc.ty])
    want = LinearNDInterpolator(t, v64.T)(xy).T                                      # scipy, sequential walk
    want[:, sc.nn_idx < 0] = np.nan                                                  # the mask
    s_walk = t.find_simplex(xy)
    _, scale = hc.linear_in_simplex(t, s_walk, sc.tx, sc.ty, v64)
    s_brute = t.find_simplex(xy, bruteforce=True)
    brute, scale_b = hc.linear_in_simplex(t, s_brute, sc.tx, sc.ty, v64)
    brute[:, sc.nn_idx < 0] = np.nan

    amb = run_locate(ctx, sc, tri)
    np.testing.assert_array_equal(run_locate(ctx, sc, tri, bounds=False), amb)
    is_amb = np.zeros(T, bool)
    is_amb[amb] = True
    for tag in ("on_vertex", "on_edge"):
        assert is_amb[sc.where(tag)].all(), (tag, sc.where(tag)[~is_amb[sc.where(tag)]])
    degenerate = bool(np.isnan(t.transform[:, 0, 0]).any())
    generic = np.zeros(T, bool)
    generic[sc.where("generic")] = True
    # generic targets are not reported -- unless their walk meets a simplex with a NaN transform and falls back to the scan
    assert not is_amb[sc.nn_idx < 0].any() and (degenerate or not is_amb[generic].any())
    assert is_amb[generic].sum() <= 4
    # A reported target may sit in more than one simplex.  The interpolants of simplices that share a facet agree ON it; the
    # target is within scipy's eps of it in barycentric units, so each differs from the facet's value by at most
    # eps (|v_off| + |v_a| + |v_b|): between two of them 6 eps max|v| over the vertices of the accepting simplices.  The
    # NaN-vertex field is judged there only if none of those simplices holds the NaN.
    acc = [hc.accepting_simplices(t, sc.tx[i], sc.ty[i]) if is_amb[i] else np.zeros(0, np.int64) for i in range(T)]
    nan_free = np.array([not np.isin(t.simplices[a], sc.nan_vertex).any() for a in acc]) | generic
    slack = np.zeros((3, T))
    for i in np.flatnonzero(is_amb & ~generic):
        if acc[i].size:
            slack[:, i] = 6.0 * hc.EPS * np.nan_to_num(np.abs(v64[:, np.unique(t.simplices[acc[i]])])).max(axis=1)

    got = run_linear(ctx, sc, tri, v)
    msgs = []
    # the documented walk restated in NumPy (horizontal_cases.walk_reference): the same report, the same pattern, the same values
    emu, emu_scale, emu_amb = hc.walk_reference(sc, v, bounds=sc.arrays()["bounds"])
    np.testing.assert_array_equal(amb, emu_amb)
    bad, _ = hc.compare_bar(got, emu, _lin_bar(emu_scale, emu, dtype))
    msgs += [f"field {i // T} target {i % T} {sc.tags[i % T]}: got {got.ravel()[i]!r} restated walk {emu.ravel()[i]!r}" for i in bad[:6]]
    # scipy has no definite answer for a target within rounding of a hull that zero-area slivers close (its walk, ours and its
    # scan leave or enter there depending on where they start): include/oisat.h documents ours, the test below pins it
    grazes = np.array([degenerate and not generic[i] and hc.grazes_hull(t, sc.tx[i], sc.ty[i]) for i in range(T)])
    for f in range(3):
        judged = (nan_free if f == 2 else np.ones(T, bool)) & ~grazes
        strict, rep = judged & (~is_amb | generic), judged & is_amb & ~generic
        for sel, ref, sc_, whom in ((strict, want[f], scale[f], "LinearNDInterpolator"), (rep, brute[f], scale_b[f], "find_simplex(bruteforce)"),
                                    # where scipy's own two searches agree the value is scipy's, reported or not
                                    (rep & ((s_walk >= 0) == (s_brute >= 0)), want[f], scale[f], "LinearNDInterpolator (reported)")):
            w = np.flatnonzero(sel)
            bad, _ = hc.compare_bar(got[f, w], ref[w], _lin_bar(sc_[w], ref[w], dtype) + slack[f, w])
            msgs += [f"field {f} target {w[i]} {sc.tags[w[i]]}: got {got[f, w[i]]!r} {whom} {ref[w[i]]!r} scale {sc_[w[i]]!r} slack {slack[f, w[i]]!r}"
                     for i in bad[:4]]
    print(f"linear {name} {np.dtype(dtype).name}: P={sc.P} ns={sc.ns} T={T} reported {amb.size} ({int(is_amb[generic].sum())} generic; "
          f"NaN transforms {int(np.isnan(t.transform[:, 0, 0]).sum())}, scipy's searches differ on {int(((s_walk >= 0) != (s_brute >= 0)).sum())})")
    assert not msgs, "\n".join(msgs[:24])
    assert np.isnan(got[:, sc.where("outside")]).all() and np.isnan(got[:, sc.where("nn_minus1")]).all()
    g = sc.where("generic")
    assert np.isnan(got[2, g]).any() and np.isfinite(got[:2, g]).all()              # a NaN value at one vertex
    # nfields = 1, bounds_host = NULL, vertex_to_simplex out of range (the walk starts at simplex 0): the same answer --
    # the same bits wherever the location is unique, the same value to the bar where it is not
    uniq, shared = (~is_amb | generic) & ~grazes, is_amb & ~generic & ~grazes       # (a hull-grazing target's answer depends on the start)
    for other in (run_linear(ctx, sc, tri, v, bounds=False), run_linear(ctx, sc, tri, v, bad_v2s=True),
                  np.concatenate([run_linear(ctx, sc, tri, v[f:f + 1]) for f in range(3)])):
        _same_bits(other[:, uniq], got[:, uniq])
        for f in range(2):
            two = 2.0 * U32 * np.abs(np.nan_to_num(got[f, shared].astype(np.float64))) if np.dtype(dtype) == np.float32 else 0.0    # two roundings
            bad, _ = hc.compare_bar(other[f, shared], got[f, shared], hc.RT64 * scale_b[f, shared] + slack[f, shared] + two)
            assert not bad, (f, bad[:4])


def test_linear_hull_grazing_targets_follow_the_walk_from_the_nearest_point(ctx):
    """Pins what include/oisat.h documents for oisat_linear_interp.  Along the straight edges of the swath grid qhull closes the
    hull with zero-area slivers, and a target on such an edge is inside or outside by 1e-13.  The library walks from a simplex
    at the target's nearest point and, like scipy's directed walk, takes the first hull facet it crosses as "outside" without a
    second look; scipy's answer for the same target depends on where its previous target ended, and its brute-force scan can
    say the opposite.  So there the library answers as its own restated walk does (every target, both patterns and values),
    it differs from LinearNDInterpolator on at least one target, and only on targets that graze the hull."""
    sc = hc.linear_scene("swath_grid")
    t, T = sc.tri, sc.T
    v = sc.values(np.float64)[:2]
    got = run_linear(ctx, sc, _Tri(ctx, sc), v)
    emu, scale, _ = hc.walk_reference(sc, v, bounds=sc.arrays()["bounds"])
    bad, _ = hc.compare_bar(got, emu, hc.RT64 * scale)
    assert not bad, [(i // T, i % T, sc.tags[i % T]) for i in bad[:8]]
    want = LinearNDInterpolator(t, v.T)(np.column_stack([sc.tx, sc.ty])).T
    want[:, sc.nn_idx < 0] = np.nan
    differs = np.flatnonzero((np.isnan(got) != np.isnan(want)).any(axis=0))
    print(f"hull-grazing targets where the library and LinearNDInterpolator disagree on inside / outside: {differs.tolist()} "
          f"({[sc.tags[i] for i in differs]})")
    assert differs.size >= 1 and all(hc.grazes_hull(t, sc.tx[i], sc.ty[i]) for i in differs)
    assert all(sc.tags[i] == "hull_row" for i in differs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", hc.LINEAR_SCENES)
def test_linear_interp_forced(ctx, name, dtype):
    """-2 walks (same bits as unforced), -1 is NaN, s evaluates in simplex s wherever the target lies, s >= nsimplex is NaN,
    and a masked target (nn_idx = -1) is NaN whatever is forced"""
    sc = hc.linear_scene(name)
    t, T = sc.tri, sc.T
    tri = _Tri(ctx, sc)
    v = sc.values(dtype)
    v64 = v.astype(np.float64)
    got = run_linear(ctx, sc, tri, v)
    _same_bits(run_linear(ctx, sc, tri, v, forced=np.full(T, -2)), got)
    rng = np.random.default_rng([hc.SEED, 40, T])
    valid = np.flatnonzero(~np.isnan(t.transform[:, 0, 0]))
    forced = rng.choice(valid, size=T)                                               # some simplex, almost never the target's own
    kind = np.arange(T) % 4
    forced[kind == 1] = -1
    forced[kind == 2] = sc.ns + np.arange((kind == 2).sum())                         # s = nsimplex, nsimplex + 1, ...
    forced[kind == 3] = -2
    out = run_linear(ctx, sc, tri, v, forced=forced)
    ref, scale = hc.linear_in_simplex(t, forced, sc.tx, sc.ty, v64)
    ref[:, sc.nn_idx < 0] = np.nan
    walk = kind == 3
    _same_bits(out[:, walk], got[:, walk])
    assert np.isnan(out[:, (kind == 1) | (kind == 2)]).all()
    own = t.find_simplex(np.column_stack([sc.tx, sc.ty]))
    assert ((kind == 0) & (forced != own)).sum() > T // 8                            # evaluated outside the forced simplex
    bad, ratio = hc.compare_bar(out[:, ~walk], ref[:, ~walk], _lin_bar(scale[:, ~walk], ref[:, ~walk], dtype))
    print(f"linear forced {name} {np.dtype(dtype).name}: largest |got - ref| / bar = {ratio:.3f}")
    assert not bad, bad[:8]
