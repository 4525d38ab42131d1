"""The innovations' likelihood and the maximum-likelihood error scales, host side (no GPU): the new entry point's declaration and
refusals, ``dense.profile_search`` / ``profile_se`` against the float64 objective of tests/likelihood_cases.py (does the search
find the minimum, in how many evaluations, and is the truth within three standard errors), what ``"both"`` can and cannot
identify, and the bookkeeping of ``set_error_scales``, ``OI_dense`` and the driver's setting that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import likelihood_cases as lc
import readers_cases as rc
from oisatgmi import _hip, dense
from oisatgmi.driver import oisatgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


# ---- 1. the entry point ---------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oisat.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True, check=True).stdout
    name = "oisat_factor_logdet"
    assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/oisat.h"
    assert re.search(rf"\bT {name}\b", out), f"{name} is not exported"
    assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_every_refusal_that_needs_no_device(lib):
    """The arguments are tested before the handle is looked into: a NULL handle, and -- behind a block of zeros that stands in for
    one -- every other refusal.  ``out`` keeps its poison."""
    fake = np.zeros(1 << 16, dtype=np.uint8)                       # (never dereferenced: every call below is refused first)
    h = fake.ctypes.data
    L = np.ones(4, dtype=np.float32)
    out = np.full(2, 7.5)
    good = dict(h=h, L=L.ctypes.data, m=100, ld=128, out=out.ctypes.data)
    bad = [dict(h=None), dict(L=None), dict(out=None), dict(m=0), dict(m=-5), dict(ld=127), dict(ld=0), dict(m=129, ld=128),
           dict(m=385, ld=384), dict(h=None, L=None, out=None, m=0, ld=0)]
    for change in bad:
        a = {**good, **change}
        assert lib.oisat_factor_logdet(a["h"], a["L"], a["m"], a["ld"], a["out"]) == EINVAL, change
        assert b"invalid argument" in lib.oisat_last_error()
    assert (out == 7.5).all() and not fake.any()


def test_an_error_carries_its_return_code(lib):
    """``fit_error_scales`` tells a non-positive pivot from every other failure by the code, not by the message."""
    header = open(os.path.join(ROOT, "include", "oisat.h")).read()
    assert int(re.search(r"#define OISAT_ENOTPD \((-?\d+)\)", header).group(1)) == _hip.ENOTPD
    c = _hip.Context.__new__(_hip.Context)
    c.lib = lib
    c.check(0)
    for rc_ in (_hip.ENOTPD, -1):
        with pytest.raises(_hip.OisatError) as e:
            c.check(rc_)
        assert e.value.code == rc_
    assert _hip.OisatError("x").code is None


# ---- 2. the search against the float64 objective ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return lc.fine_grid(2001)


def test_the_profile_is_the_likelihood_of_the_system_itself():
    """``Profile`` (one eigen-decomposition) against slogdet and a solve of S(s) = s P + R."""
    for name, model, s in (("C", "gaussian", 0.3), ("B600", "soar", 7.0), ("A", "gaussian", 100.0)):
        d = lc.draw(name, model, 4.0, 1.0, 2)
        ref = lc.loglik64(name, model, d, scale_b=s)
        logdet, chi2 = lc.Profile(name, model, d).parts(np.log(s))
        assert abs(logdet - ref["logdet"]) <= 1e-8 * abs(ref["logdet"]) + 1e-8
        assert abs(chi2 - ref["chi2"]) <= 1e-8 * ref["chi2"]


@pytest.mark.parametrize("name", ["A", "B600", "C"])
@pytest.mark.parametrize("s_true", [0.25, 4.0])
@pytest.mark.parametrize("seed", lc.SEEDS)
def test_profile_search_finds_the_minimum_and_the_truth(name, s_true, seed, grid):
    prof = lc.Profile(name, "gaussian", lc.draw(name, "gaussian", s_true, 1.0, seed))
    res = dense.profile_search(prof.J_background)
    excess = res["J"] - float(prof.J_background(grid).min())
    se = dense.profile_se(prof.J_background, res["x"], res["J"])
    z = (res["x"] - np.log(s_true)) / se
    print(f"{name} s_true {s_true} seed {seed}: excess {excess:.2e}, nevals {res['nevals']}, se_ln {se:.3f}, z {z:+.2f}")
    assert excess <= 0.02
    assert res["nevals"] <= 25 and res["nevals"] == len(res["evaluations"])
    assert res["J"] == prof.J_background(res["x"]) and (res["x"], res["J"]) in res["evaluations"]
    assert abs(z) <= 3.0
    assert not res["at_bound"]


def test_a_truth_outside_the_bounds_sets_at_bound():
    for s_true, end in ((1e4, 1), (1e-4, 0)):
        prof = lc.Profile("A", "gaussian", lc.draw("A", "gaussian", s_true, 1.0, 2))
        res = dense.profile_search(prof.J_background)
        assert res["at_bound"] and abs(res["x"] - np.log(lc.BOUNDS[end])) <= 0.01, (s_true, res["x"])


def test_an_objective_that_is_inf_on_part_of_the_range_still_gives_the_finite_minimum(grid):
    prof = lc.Profile("C", "gaussian", lc.draw("C", "gaussian", 4.0, 1.0, 2))
    wall = np.log(0.5)                                             # below it the "factorization fails"; the grid's 4 lowest points

    def J(x):
        return float("inf") if x < wall else float(prof.J_background(x))

    res = dense.profile_search(J)
    assert np.isfinite(res["J"]) and res["J"] - float(prof.J_background(grid).min()) <= 0.02
    assert sum(1 for _, Jx in res["evaluations"] if Jx == float("inf")) >= 4
    # ... nothing finite anywhere: no minimiser, and no standard error
    res = dense.profile_search(lambda x: float("inf"))
    assert np.isnan(res["x"]) and res["J"] == float("inf") and not res["at_bound"] and res["nevals"] <= 32
    assert dense.profile_se(lambda x: float("inf"), 0.0, 1.0) == float("inf")
    assert dense.profile_se(lambda x: -x * x, 0.0, 0.0) == float("inf")          # (J'' <= 0)
    assert dense.profile_se(lambda x: 4.0 * x * x, 0.0, 0.0) == pytest.approx(0.5)
    for kw in (dict(bounds=(0.0, 1.0)), dict(bounds=(2.0, 1.0)), dict(npts=2), dict(wtol=0.0), dict(max_evals=5)):
        with pytest.raises(ValueError):
            dense.profile_search(lambda x: x * x, **kw)


# ---- 3. both scales: what is identified and what is not --------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("A", "gaussian"), ("B600", "gaussian"), ("B600", "soar"), ("B600", "gaspari_cohn")])
@pytest.mark.parametrize("seed", lc.SEEDS)
def test_both_recovers_the_ratio(name, model, seed):
    prof = lc.Profile(name, model, lc.draw(name, model, 4.0, 0.5, seed))
    res = dense.profile_search(prof.J_both)
    se = dense.profile_se(prof.J_both, res["x"], res["J"])
    z = (res["x"] - np.log(8.0)) / se
    a = float(prof.parts(res["x"])[1]) / prof.m
    print(f"{name} {model} seed {seed}: rho {np.exp(res['x']):.3f}, a {a:.3f}, se_ln {se:.3f}, z {z:+.2f}, nevals {res['nevals']}")
    assert abs(z) <= 3.0 and res["nevals"] <= 25


@pytest.mark.parametrize("seed", lc.SEEDS)
def test_both_cannot_tell_the_two_apart_when_P_is_nearly_diagonal(seed):
    """Case B (L = 100 km, observations mostly further apart than that): s P + R is nearly diagonal whatever s, and only the sum
    of the two variances is seen.  The standard error of ln rho says so: above 1, i.e. rho is not known within a factor e."""
    prof = lc.Profile("B", "gaussian", lc.draw("B", "gaussian", 4.0, 0.5, seed))
    res = dense.profile_search(prof.J_both)
    se = dense.profile_se(prof.J_both, res["x"], res["J"])
    print(f"B seed {seed}: rho {np.exp(res['x']):.3f}, se_ln {se:.3f}")
    assert se > 1.0


# ---- 4. bookkeeping that needs no device -------------------------------------------------------------------------------------------
class _Ctx:
    """Stands in for a handle: remembers what was uploaded where."""

    def __init__(self):
        self.mem = {}

    def upload_into(self, ptr, arr, dtype=None):
        self.mem[ptr] = np.array(arr, dtype=dtype)


class _Buf:
    def __init__(self, ptr):
        self.ptr = ptr


def _plan():
    p = dense.DenseAnalysis.__new__(dense.DenseAnalysis)
    p.ctx, p.gsig, p.osig, p.ovar = _Ctx(), _Buf(1), _Buf(2), _Buf(3)
    p._scales, p._lik_ready = (1.0, 1.0), True
    p._gsig0 = p._gsig_host = np.array([1.0, 2.0, 3.0])
    p._osig0, p._ovar0 = np.array([2.0, 3.0]), np.array([0.5, 0.25])
    return p


def test_set_error_scales_uploads_scaled_copies_of_what_was_loaded():
    p = _plan()
    p.set_error_scales(4.0, 3.0)
    assert p._scales == (4.0, 3.0) and not p._lik_ready
    assert p.ctx.mem[1].tolist() == [2.0, 4.0, 6.0] and p._gsig_host.tolist() == [2.0, 4.0, 6.0]
    assert p.ctx.mem[2].tolist() == [4.0, 6.0] and p.ctx.mem[3].tolist() == [1.5, 0.75]
    p.set_error_scales(scale_o=2.0)                                # absolute, not cumulative
    assert p._scales == (1.0, 2.0) and p.ctx.mem[1].tolist() == [1.0, 2.0, 3.0] and p.ctx.mem[3].tolist() == [1.0, 0.5]
    assert p._gsig0.tolist() == [1.0, 2.0, 3.0] and p._ovar0.tolist() == [0.5, 0.25]
    # a load puts the scales back: with the observations (load_background) or, ahead of new ones, the background only
    p.ctx.mem.clear()
    p._reset_scales()
    assert p._scales == (1.0, 1.0) and p.ctx.mem[3].tolist() == [0.5, 0.25] and p.ctx.mem[1].tolist() == [1.0, 2.0, 3.0]
    p.ctx.mem.clear()
    p._reset_scales()                                              # at 1 already: nothing travels
    assert not p.ctx.mem
    p.set_error_scales(9.0, 9.0)
    p.ctx.mem.clear()
    p._reset_scales(obs=False)
    assert sorted(p.ctx.mem) == [1] and p._osig0 is None and p._gsig_host.tolist() == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("bad", [(0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf")),
                                 ("x", 1.0), (None, 1.0)])
def test_set_error_scales_refuses_bad_scales_with_nothing_uploaded(bad):
    p = _plan()
    with pytest.raises(ValueError):
        p.set_error_scales(*bad)
    assert not p.ctx.mem and p._scales == (1.0, 1.0) and p._lik_ready


def test_log_likelihood_and_the_fit_refuse_before_a_device_is_touched():
    p = _plan()
    p._lik_ready = False
    with pytest.raises(ValueError, match="exact_factor"):
        p.log_likelihood()
    with pytest.raises(ValueError, match="mode"):
        p.fit_error_scales(300.0, mode="observations")
    with pytest.raises(ValueError):
        p.fit_error_scales(300.0, corr="cubic")
    assert not p.ctx.mem


def test_oi_dense_refuses_an_unknown_fit_scale_before_anything_is_touched():
    Y = np.full((2, 2), -1.0)
    for bad in ("ml", "Background", True, 1):
        with pytest.raises(ValueError, match="fit_scale"):
            dense.OI_dense(None, Y, None, None, None, None, 300.0, fit_scale=bad)
    assert (Y == -1.0).all()                                       # (not even the clamp of Y has happened)


def test_scale_setting():
    f = oisatgmi._scale_setting
    assert f("knee") is None and f(" KNEE ") is None
    assert f("ml") == "background" and f("ML") == "background" and f("ml:both") == "both" and f(" Ml:Both") == "both"
    for bad in ("", "ml:", "ml:background", "both", "0", "off", "ml:both:x", None, 1.0):
        with pytest.raises(ValueError, match="OISAT_OI_SCALE"):
            f(bad)


@pytest.mark.parametrize("mode", ["diag", "tiled"])
def test_the_driver_refuses_ml_outside_the_dense_mode(mode, monkeypatch):
    monkeypatch.delenv("OISAT_OI_SCALE", raising=False)
    o = oisatgmi()
    o.ctm_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_vcd = np.ones((4, 8))
    o.sat_averaged_error = np.ones((4, 8))
    o.oi_mode, o.oi_scale = mode, "ml"
    with pytest.raises(ValueError, match="OISAT_OI_SCALE"):
        o.oi("TROPOMI")
    o.oi_scale = None
    monkeypatch.setenv("OISAT_OI_SCALE", "ml:both")
    with pytest.raises(ValueError, match="dense mode"):
        o.oi("TROPOMI")
    monkeypatch.setenv("OISAT_OI_SCALE", "maximum")
    with pytest.raises(ValueError, match="expected knee, ml or ml:both"):
        o.oi("TROPOMI")
