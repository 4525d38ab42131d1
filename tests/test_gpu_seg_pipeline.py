"""GPU tests of the ring of LDS-DMA stages in the factor's shadow K-segments (csrc/dense_dag.inc: dag_seg_sh, kShRing) and of
the shadow layout behind it.  Nothing may change by a bit: every factor here is ``np.array_equal`` to the factor that reads no
shadow (``OISAT_FACTOR_SHADOW=0``: the in-loop conversions, which the ring does not touch), through both launches; a race
in the ring -- a stage read before it landed, or refilled before its last read -- shows as a rare mismatch, so one system is
factored twenty times; and the images are read back through the ABI against NumPy's bf16 rounding."""
import numpy as np
import pytest

from test_gpu_factor_shadow import MODES, SHADOW, _bf16, _bf16_value, _factor_fwd, _has_shadow
from test_gpu_mid_band import FWD, NB, Case, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

# name -> (observations asked for, correlation length in km, far bits, middle bits)
SHAPES = {
    "main": (4000, 600.0, 16, 8),       # 3 946 observations: tests/test_gpu_mid_band.py's main case
    "edge": (2600, 300.0, 27, 26),      # 2 551 observations: single far and middle blocks
    "long": (5200, 1200.0, 12, 4),      # 5 094 observations, 40 block rows: segments of 1, 2, 3 and >= 5 K-blocks of either kind (test_shape_of_the_long_case)
}


@pytest.fixture(scope="module")
def cases(ctx):
    out = {}
    rng = np.random.default_rng(17)
    for name, (nobs, L, far_bits, mid_bits) in SHAPES.items():
        c = out[name] = Case(ctx, nobs, 4000, L, far_bits, mid_bits)
        c.d = ctx.upload(rng.standard_normal(c.m), dtype=np.float64)
        c.z = ctx.alloc(c.m * 8)
        c.olat = ctx.upload(c.lat, dtype=np.float64)
    return out


@pytest.fixture(scope="module")
def plain(cases):
    """The factor of every case with no shadow read or written, once."""
    out = {}
    for name, c in cases.items():
        out[name] = c.factor(c.far, c.mid, **{SHADOW: 0})
        assert not _has_shadow(c) and np.isfinite(out[name]).all()
    return out


def test_shape_of_the_long_case(cases):
    """The host tables hold what the ring has to get right: far and middle stretches of exactly 1, 2 and 3 K-blocks (the ring
    turns 1, 2, 3 / 2, 4, 6 times: prologue and drain meet) and of 5 and more, tasks that run far -> middle -> fp32 back to
    back, and tasks whose first segment is a middle one."""
    c = cases["long"]
    nf, nm, n32 = c.ranges()
    n = {}
    for kind, blocks in (("far", nf), ("middle", nm)):
        for k in (1, 2, 3):
            n[f"{kind} == {k}"] = int((blocks == k).sum())
        n[f"{kind} >= 5"] = int((blocks >= 5).sum())
    n["far, middle and fp32"] = int(((nf > 0) & (nm > 0) & (n32 > 0)).sum())
    n["middle and no far"] = int(((nm > 0) & (nf == 0)).sum())
    print("long case:", c.m, "observations,", c.nb, "block rows; bulk tasks with", n)
    assert all(v > 0 for v in n.values()), n
    assert c.m % NB != 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_factor_bits(cases, plain, name):
    """OISAT_FACTOR_SHADOW = 0 | unset | far | mid, through potrf_dag_kernel<0> (oisat_potrf_env) and <2> (oisat_potrf_env_fwd)."""
    c, want = cases[name], plain[name]
    want_f, want_z = _factor_fwd(c, **{SHADOW: 0, FWD: None})
    assert np.array_equal(want_f, want)
    for mode in MODES:
        got = c.factor(c.far, c.mid, **{SHADOW: mode})
        assert _has_shadow(c)
        assert np.array_equal(got, want), f"{name}: OISAT_FACTOR_SHADOW={mode}, the launch that only factors"
        f, z = _factor_fwd(c, **{SHADOW: mode, FWD: None})
        assert _has_shadow(c)
        assert np.array_equal(f, want) and np.array_equal(z, want_z), f"{name}: OISAT_FACTOR_SHADOW={mode}, the launch that carries the sweep"
    assert tuple(c.ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_twenty_runs_one_factor(cases, plain):
    c = cases["long"]
    first = c.factor(c.far, c.mid, **{SHADOW: None})
    assert _has_shadow(c)
    assert np.array_equal(first, plain["long"])
    for run in range(1, 20):
        assert np.array_equal(c.factor(c.far, c.mid, **{SHADOW: None}), first), f"run {run}"
    assert tuple(c.ctx.solve_status(clear=True))[:3] == (0, 0, 0)


def test_shadow_contents(cases):
    """hi = bf16(tile), lo = bf16(tile - hi) as bit patterns through oisat_factor_shadow_tile: a sub-diagonal tile (the chain
    writes it), ordinary tiles at both ends of a row, tiles of the padded last block row."""
    c = cases["main"]
    ctx, lib = c.ctx, c.ctx.lib
    f = c.factor(c.far, c.mid, **{SHADOW: None})
    nb, first = c.nb, c.first
    r = nb // 2
    assert r - first[r] >= 3 and (nb - 1) - first[nb - 1] >= 2 and c.m % NB != 0
    hi, lo = np.empty((NB, NB), dtype=np.uint16), np.empty((NB, NB), dtype=np.uint16)
    for (i, k) in [(r, r - 1), (1, 0), (r, int(first[r])), (r, r - 2), (nb - 1, int(first[nb - 1])), (nb - 1, nb - 2)]:
        ctx.check(lib.oisat_factor_shadow_tile(ctx.h, i, k, hi.ctypes.data, lo.ctypes.data))
        tile = f[i * NB:(i + 1) * NB, k * NB:(k + 1) * NB]
        want_hi = _bf16(tile)
        want_lo = _bf16(tile - _bf16_value(want_hi))            # (exact in float32)
        assert np.abs(tile).max() > 0
        assert np.array_equal(hi, want_hi), (i, k)
        assert np.array_equal(lo, want_lo), (i, k)
    assert lo.any() and hi.any()
