"""The per-pixel vertical operators of csrc/amf.hip, called at the C ABI on catalogues of adversarial columns
(tests/vertical_cases.py) and judged by scipy itself: the oracle's per-pixel functions (interp1d verbatim) for float64
cubes, their float32-log-pinned twins for float32 cubes, wrapped in the pixel-skip rules and post-masks of
amf_recal.py / ak_conv_*.py.  One launch carries a whole catalogue; nothing is skipped at run time.

Per output array: (1) the NaN pattern equals the reference's, (2) so does the inf pattern with its sign, (3) on finite
values |got - ref| <= tol * scale, scale = sum of |terms| the reference summed for the pixel, floored at |ref|.
tol = 1e-12 (RT64) for float64 cubes.  Float32 cubes: TOL32 below, from the distance measured on an MI355X to the
reference whose float32 logarithms are the correctly rounded ones.

Planned exclusion: columns with a NaN among the NODES of the float64 non-extrapolating (MOPITT) path are judged by
pattern only -- np.interp wants increasing xp and its answer beside a NaN node depends on its search's starting guess.
They are 2.6 % of a MOPITT catalogue (2.9 % for two model levels); the test asserts <= 3 %.

What the catalogue found, and what became of it:
  * float64 cubes, MOPITT: interp1d hands float64 x / y with a non-extrapolating fill to np.interp (_call_linear_np),
    not to _call_linear.  The kernel used _call_linear's arithmetic: on a duplicated model level it returned the first
    duplicate's value where np.interp returns the last one's, and beside a NaN / inf profile value a query exactly on a
    node gave NaN where np.interp returns the node's value (or retries from the right-hand node).  Fixed:
    ModelColumn<double>::at_interp follows NumPy's arr_interp; float32 cubes and the extrapolating calls stay on
    _call_linear.
  * float32 cubes, both AK convolutions: log / log10 of the model pressure and of the surface mixing ratio were taken by
    the single-precision device functions, not "in double, rounded once" as the AMF kernel does and documents.  Fixed:
    the logarithm is taken in double and rounded to float32.
Measured on an MI355X (all catalogues, all outputs): before the fixes the float64 MOPITT outputs were up to 0.17 of the
scale away (duplicate levels) and the float32 AK convolutions up to 2.8e-6 (single-precision logarithms); 20 MOPITT and 10
float32 GOSAT catalogue tests failed.  After them: float64 cubes within 6.3e-16, float32 cubes within 2.2e-15 of the
reference with correctly rounded float32 logarithms (MEASURED_F32), and no pixel whose float32 logarithm differs.  The
AMF recalculation, column_sum, pwv_sum and the element-wise kernels showed no divergence.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oi_oracle as orc                       # the checker (tests only)
from oisatgmi import _hip
import vertical_cases as vc

RT64 = vc.RT64
# Largest |got - ref| / scale over every float32 catalogue below, every output, on an MI355X, against the reference with
# correctly rounded float32 logarithms: see MEASURED_F32.  It is within 1e-12, so that is the bar; no pixel's float32
# logarithm differs from the correctly rounded one (one that did would move its pixel by about 1e-7).
MEASURED_F32 = 2.184e-15
TOL32 = 1e-12
PAD, SENTINEL = 64, 12345.678
PIXELS = {"amf": orc.amf_pixel, "mopitt": orc.mopitt_pixel, "gosat": orc.gosat_pixel}
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    return c


def _tol(dtype):
    return RT64 if np.dtype(dtype) == np.float64 else TOL32


class _Out:
    """an output array of n elements followed by PAD sentinels: the grid's tail must not write past n"""

    def __init__(self, ctx, n, dtype=np.float64):
        self.ctx, self.n, self.dtype = ctx, n, np.dtype(dtype)
        self.buf = ctx.upload(np.full(n + PAD, SENTINEL, dtype=self.dtype))
        self.ptr = self.buf.ptr

    def get(self):
        self.ctx.sync()
        a = self.ctx.download(self.ptr, (self.n + PAD,), self.dtype)
        assert (a[self.n:] == self.dtype.type(SENTINEL)).all(), "wrote past the last pixel"
        return a[:self.n]

    def untouched(self):
        self.ctx.sync()
        return bool((self.ctx.download(self.ptr, (self.n + PAD,), self.dtype) == self.dtype.type(SENTINEL)).all())


def _up(ctx, a, dtype=np.float64):
    return ctx.upload(np.ascontiguousarray(a, dtype=dtype))


def run_amf(ctx, cat, use_trop=True):
    n = cat.n
    ins = [_up(ctx, cat.sat_p), _up(ctx, cat.sat_y), _up(ctx, cat.ctm_p, cat.dtype), _up(ctx, cat.ctm_y, cat.dtype),
           _up(ctx, cat.trop), _up(ctx, cat.vcd), _up(ctx, cat.amf)]
    outs = [_Out(ctx, n) for _ in range(3)]
    ctx.check(ctx.lib.oisat_amf_recal(ctx.h, ins[0].ptr, ins[1].ptr, cat.nzs, _hip.dtype_code(cat.dtype), ins[2].ptr, ins[3].ptr,
                                      cat.nzc, ins[4].ptr if use_trop else None, ins[5].ptr, ins[6].ptr, n, outs[0].ptr,
                                      outs[1].ptr, outs[2].ptr))
    return dict(zip(("new_amf", "vcd_out", "ctm_vcd"), (o.get() for o in outs)))


def run_mopitt(ctx, cat):
    n = cat.n
    ins = [_up(ctx, cat.ctm_p, cat.dtype), _up(ctx, cat.ctm_y, cat.dtype), _up(ctx, cat.air, cat.dtype), _up(ctx, cat.sat_p),
           _up(ctx, cat.ak), _up(ctx, cat.ap_prof), _up(ctx, cat.ap_col), _up(ctx, cat.ap_surf), _up(ctx, cat.vcd)]
    outs = [_Out(ctx, n) for _ in range(2)]
    ctx.check(ctx.lib.oisat_ak_conv_mopitt(ctx.h, _hip.dtype_code(cat.dtype), ins[0].ptr, ins[1].ptr, ins[2].ptr, cat.nzc, ins[3].ptr,
                                           ins[4].ptr, ins[5].ptr, cat.nzs, ins[6].ptr, ins[7].ptr, ins[8].ptr, n, outs[0].ptr,
                                           outs[1].ptr))
    return dict(zip(("model_vcd", "model_xcol"), (o.get() for o in outs)))


def run_gosat(ctx, cat):
    n = cat.n
    ins = [_up(ctx, cat.ctm_p, cat.dtype), _up(ctx, cat.ctm_y, cat.dtype), _up(ctx, cat.sat_p), _up(ctx, cat.ak),
           _up(ctx, cat.ap_prof), _up(ctx, cat.pw), _up(ctx, cat.vcd)]
    out = _Out(ctx, n)
    ctx.check(ctx.lib.oisat_ak_conv_gosat(ctx.h, _hip.dtype_code(cat.dtype), ins[0].ptr, ins[1].ptr, cat.nzc, ins[2].ptr, ins[3].ptr,
                                          ins[4].ptr, ins[5].ptr, cat.nzs, ins[6].ptr, n, out.ptr))
    return {"model_xcol": out.get()}


def run_column_sum(ctx, cat, use_trop=True):
    ins = [_up(ctx, cat.ctm_p, cat.dtype), _up(ctx, cat.ctm_y, cat.dtype), _up(ctx, cat.trop), _up(ctx, cat.vcd)]
    out = _Out(ctx, cat.n, cat.dtype)
    ctx.check(ctx.lib.oisat_column_sum(ctx.h, _hip.dtype_code(cat.dtype), ins[0].ptr, ins[1].ptr, cat.nzc,
                                       ins[2].ptr if use_trop else None, ins[3].ptr, cat.n, out.ptr))
    return {"ctm_vcd": out.get()}


def ref_column_sum(cat, use_trop=True):
    """amf_recal.py:160-171 as orc.amf_recal restates it: mask, np.nansum(axis=0) level after level in the cube's dtype"""
    pc = np.array(cat.ctm_y, copy=True)
    if use_trop:
        with np.errstate(invalid="ignore"):
            for z in range(pc.shape[0]):
                pc[z][cat.ctm_p[z] < cat.trop] = np.nan
    with np.errstate(all="ignore"):
        mv = np.nansum(pc, axis=0)
        scale = np.nansum(np.abs(pc.astype(np.float64)), axis=0)
    mv[np.isnan(cat.vcd)] = np.nan
    return {"ctm_vcd": (mv, scale)}


def run_pwv_sum(ctx, cat):
    ins = [_up(ctx, cat.ctm_y, cat.dtype), _up(ctx, cat.vcd)]
    out = _Out(ctx, cat.n, cat.dtype)
    ctx.check(ctx.lib.oisat_pwv_sum(ctx.h, _hip.dtype_code(cat.dtype), ins[0].ptr, cat.nzc, ins[1].ptr, cat.n, out.ptr))
    return {"pwv": out.get()}


def ref_pwv_sum(cat):
    """pwv_cal.py:96-98 as orc.pwv_calculator restates it"""
    with np.errstate(all="ignore"):
        pwv = np.nansum(cat.ctm_y / 1000.0, axis=0)
        scale = np.nansum(np.abs((cat.ctm_y / 1000.0).astype(np.float64)), axis=0)
    pwv[np.isnan(cat.vcd)] = np.nan
    pwv[np.isinf(cat.vcd)] = np.nan
    return {"pwv": (pwv, scale)}


def judge(cat, got, ref, what):
    assert cat.n == len(cat.tags)
    only = cat.pattern_only()
    assert only.mean() <= 0.03, f"{what}: {only.mean():.3%} pattern-only columns"
    tol, msgs = _tol(cat.dtype), []
    for nm, (r, scale) in ref.items():
        assert got[nm].shape == r.shape and got[nm].dtype == r.dtype, (nm, got[nm].dtype, r.dtype)
        bad, dist = vc.compare(got[nm], r, scale, tol, check_values=~only)
        print(f"{what} {nm}: n={cat.n} max |got-ref|/scale = {dist:.3e} (tol {tol:.0e}), {len(bad)} failing")
        for i in bad[:8]:
            msgs.append(f"{nm}[{i}] {cat.tags[i]}: got {got[nm][i]!r} ref {r[i]!r} scale {scale[i]!r}")
        if len(bad) > 8:
            msgs.append(f"{nm}: {len(bad)} failing columns, tags {sorted({cat.tags[i] for i in bad})}")
    assert not msgs, f"{what}:\n" + "\n".join(msgs)


def _pixels(op, dtype):
    return PIXELS[op] if np.dtype(dtype) == np.float64 else None      # float32: the log-pinned twins of vertical_cases


def _ids(op):
    return [f"nzs{a}-nzc{b}" for a, b in vc.PAIRS[op]]


@pytest.mark.parametrize("use_trop", [True, False], ids=["trop", "notrop"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nzs,nzc", vc.PAIRS["amf"], ids=_ids("amf"))
def test_amf_recal_catalogue(ctx, nzs, nzc, dtype, use_trop):
    cat = vc.catalogue("amf", nzs, nzc, dtype)
    judge(cat, run_amf(ctx, cat, use_trop), vc.reference(cat, _pixels("amf", dtype), use_trop=use_trop),
          f"amf_recal nzs={nzs} nzc={nzc} {np.dtype(dtype).name} trop={use_trop}")


@pytest.mark.parametrize("use_trop", [True, False], ids=["trop", "notrop"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nzs,nzc", vc.PAIRS["amf"], ids=_ids("amf"))
def test_column_sum_and_pwv_sum_catalogue(ctx, nzs, nzc, dtype, use_trop):
    cat = vc.catalogue("amf", nzs, nzc, dtype)
    what = f"nzc={nzc} {np.dtype(dtype).name} trop={use_trop}"
    judge(cat, run_column_sum(ctx, cat, use_trop), ref_column_sum(cat, use_trop), "column_sum " + what)
    if use_trop:
        judge(cat, run_pwv_sum(ctx, cat), ref_pwv_sum(cat), "pwv_sum " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nzs,nzc", vc.PAIRS["mopitt"], ids=_ids("mopitt"))
def test_ak_conv_mopitt_catalogue(ctx, nzs, nzc, dtype):
    cat = vc.catalogue("mopitt", nzs, nzc, dtype)
    judge(cat, run_mopitt(ctx, cat), vc.reference(cat, _pixels("mopitt", dtype)),
          f"ak_conv_mopitt nzs={nzs} nzc={nzc} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nzs,nzc", vc.PAIRS["gosat"], ids=_ids("gosat"))
def test_ak_conv_gosat_catalogue(ctx, nzs, nzc, dtype):
    cat = vc.catalogue("gosat", nzs, nzc, dtype)
    judge(cat, run_gosat(ctx, cat), vc.reference(cat, _pixels("gosat", dtype)),
          f"ak_conv_gosat nzs={nzs} nzc={nzc} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_grid_tail(ctx, n, dtype):
    """one pixel, one short of a block, a full block, one pixel in a second block: every operator, outputs padded"""
    what = f"n={n} {np.dtype(dtype).name} "
    cat = vc.catalogue("amf", 9, 9, dtype).head(n)
    judge(cat, run_amf(ctx, cat), vc.reference(cat, _pixels("amf", dtype)), what + "amf_recal")
    judge(cat, run_column_sum(ctx, cat), ref_column_sum(cat), what + "column_sum")
    judge(cat, run_pwv_sum(ctx, cat), ref_pwv_sum(cat), what + "pwv_sum")
    cat = vc.catalogue("mopitt", 9, 9, dtype).head(n)
    judge(cat, run_mopitt(ctx, cat), vc.reference(cat, _pixels("mopitt", dtype)), what + "ak_conv_mopitt")
    cat = vc.catalogue("gosat", 9, 9, dtype).head(n)
    judge(cat, run_gosat(ctx, cat), vc.reference(cat, _pixels("gosat", dtype)), what + "ak_conv_gosat")


def test_level_limits_are_rejected_before_any_launch(ctx):
    """nzs = 65, nzc = 129, one satellite level for the AMF, one model level for the AK convolution: OISAT_EINVAL, and
    the outputs keep their sentinels.  (The buffers are sized for the rejected shapes all the same.)"""
    n, lib, EINVAL = 4, ctx.lib, -1
    big = _up(ctx, np.ones((130, n)))
    big32 = _up(ctx, np.ones((130, n)), np.float32)
    vec = _up(ctx, np.ones(n))
    outs = [_Out(ctx, n) for _ in range(3)]
    for code, cube in ((_hip.F64, big), (_hip.F32, big32)):
        for nzs, nzc in ((65, 8), (8, 129), (1, 8), (0, 8), (8, 0)):
            assert lib.oisat_amf_recal(ctx.h, big.ptr, big.ptr, nzs, code, cube.ptr, cube.ptr, nzc, vec.ptr, vec.ptr, vec.ptr, n,
                                       outs[0].ptr, outs[1].ptr, outs[2].ptr) == EINVAL, ("amf", nzs, nzc)
        for nzs, nzc in ((65, 8), (8, 129), (8, 1), (0, 8)):
            assert lib.oisat_ak_conv_mopitt(ctx.h, code, cube.ptr, cube.ptr, cube.ptr, nzc, big.ptr, big.ptr, big.ptr, nzs, vec.ptr,
                                            vec.ptr, vec.ptr, n, outs[0].ptr, outs[1].ptr) == EINVAL, ("mopitt", nzs, nzc)
            assert lib.oisat_ak_conv_gosat(ctx.h, code, cube.ptr, cube.ptr, nzc, big.ptr, big.ptr, big.ptr, big.ptr, nzs, vec.ptr, n,
                                           outs[0].ptr) == EINVAL, ("gosat", nzs, nzc)
    assert b"invalid argument" in lib.oisat_last_error()
    assert all(o.untouched() for o in outs)


def _elementwise_inputs(n, dtype, seed):
    rng = np.random.default_rng([seed, n])
    T = np.dtype(dtype).type
    tiny = np.finfo(dtype).tiny
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny / 4, -tiny / 8, tiny, np.finfo(dtype).max, 1e-30], dtype=dtype)
    out = []
    for lo, hi in ((1.0, 9.0e3), (1e-3, 4.0e2)):
        a = rng.uniform(lo, hi, size=n).astype(dtype)
        hit = rng.uniform(size=n) < 0.15
        a[hit] = specials[rng.integers(0, specials.size, size=int(hit.sum()))]
        a[:: max(n // 7, 1)] *= T(1e-36 if dtype == np.float32 else 1e-300)     # products that end subnormal
        out.append(a)
    return out


def _same_bits(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    u = np.uint32 if ref.dtype == np.float32 else np.uint64
    diff = np.flatnonzero(got.view(u)[~nan] != ref.view(u)[~nan])
    assert diff.size == 0, (diff[:5], got[~nan][diff[:5]], ref[~nan][diff[:5]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_elementwise_kernels_bit_for_bit(ctx, n, dtype):
    """oisat_partial_column (with and without profile) and oisat_water_column against the oracle's left-to-right
    expressions evaluated in the same dtype: one rounding per operation, so every non-NaN result has the same bits."""
    delp, prof = _elementwise_inputs(n, dtype, 77)
    code, db, pb = _hip.dtype_code(dtype), _up(ctx, delp, dtype), _up(ctx, prof, dtype)
    with np.errstate(all="ignore"):
        refs = (orc.partial_column(delp, prof), orc.air_partial_column(delp), delp * prof / 9.80665 / 10000.0)
    calls = (lambda o: ctx.lib.oisat_partial_column(ctx.h, code, db.ptr, pb.ptr, n, o),
             lambda o: ctx.lib.oisat_partial_column(ctx.h, code, db.ptr, None, n, o),
             lambda o: ctx.lib.oisat_water_column(ctx.h, code, db.ptr, pb.ptr, n, o))
    for call, ref in zip(calls, refs):
        out = _Out(ctx, n, dtype)
        ctx.check(call(out.ptr))
        _same_bits(out.get(), ref)
