"""The exact analysis error of regional means, host side (no GPU): ``dense.region_weights``, the NumPy assembly of the
residual-corrected reduction (and why it is that form and not the plain G^T Y), the argument checks of the two new entry points
that need no device, the settings, and the condition numbers that the GPU test's bound is derived from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import functional_cases as fc
from oisatgmi import _hip, dense, synthetic as syn
from oisatgmi.driver import oisatgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oisat_functional_gather", "oisat_rows_dot")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return fc.library()


def test_the_two_symbols_are_exported_and_declared(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oisat.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/oisat.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not exported"
        assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_a_null_handle_is_einval_before_anything_is_touched(lib):
    """Both entry points test the handle and the sizes before they look at the device: no GPU is needed to see it."""
    a = np.zeros(8)
    p = a.ctypes.data
    assert lib.oisat_functional_gather(None, p, p, None, 1, p, p, None, 1, p, 1, 1, 1.0, p, 1) == EINVAL
    assert b"invalid argument" in lib.oisat_last_error()
    assert lib.oisat_rows_dot(None, p, 1, 1, p, 1, 1, 1, p) == EINVAL
    assert b"invalid argument" in lib.oisat_last_error()
    # (bad sizes beside it change nothing: still OISAT_EINVAL, still no crash)
    assert lib.oisat_functional_gather(None, p, p, None, 0, p, p, None, 0, p, 65, 0, 1.0, p, 0) == EINVAL
    assert lib.oisat_rows_dot(None, p, 0, 65, p, 0, 0, 0, p) == EINVAL


# ---- region_weights ---------------------------------------------------------------------------------------------------------------
def _labels():
    lat, lon = syn.global_grid(12, 24)
    labels = np.zeros(lat.shape, dtype=np.int64)
    labels[(lat > 0) & (lon < 0)] = 7
    labels[(lat > 0) & (lon > 0)] = 3
    labels[lat < -60] = -2                                            # (not a region)
    return lat, lon, labels


def test_region_weights_ids_sums_and_area_weighting():
    lat, lon, labels = _labels()
    ids, W = dense.region_weights(labels, lat)
    assert ids.tolist() == [3, 7] and W.shape == (2, 12, 24) and W.dtype == np.float64
    np.testing.assert_allclose(W.sum(axis=(1, 2)), 1.0, rtol=0, atol=4e-16)
    for k, r in enumerate(ids):
        mk = labels == r
        assert (W[k][~mk] == 0).all() and (W[k][mk] > 0).all()
        np.testing.assert_allclose(W[k][mk], np.cos(np.deg2rad(lat[mk])) / np.cos(np.deg2rad(lat[mk])).sum(), rtol=1e-15)
    _, U = dense.region_weights(labels, lat, area_weighted=False)
    for k, r in enumerate(ids):
        mk = labels == r
        np.testing.assert_allclose(U[k][mk], 1.0 / mk.sum(), rtol=1e-15)
    # a float map that holds integers is taken; anything else is not
    ids2, W2 = dense.region_weights(labels.astype(np.float64), lat)
    assert ids2.tolist() == [3, 7] and np.array_equal(W2, W)
    with pytest.raises(ValueError):
        dense.region_weights(labels + 0.5, lat)
    with pytest.raises(ValueError):
        dense.region_weights(labels[:-1], lat)


def test_region_weights_leaves_out_cells_without_a_background():
    lat, lon, labels = _labels()
    valid = np.ones(lat.shape, dtype=bool)
    gone = np.flatnonzero(labels.ravel() == 3)[:5]
    valid.flat[gone] = False
    ids, W = dense.region_weights(labels, lat, valid=valid)
    assert (W[0].flat[gone] == 0).all()
    np.testing.assert_allclose(W.sum(axis=(1, 2)), 1.0, rtol=0, atol=4e-16)
    keep = (labels == 3) & valid
    np.testing.assert_allclose(W[0][keep], np.cos(np.deg2rad(lat[keep])) / np.cos(np.deg2rad(lat[keep])).sum(), rtol=1e-15)


def test_region_weights_names_the_label_it_refuses():
    lat, lon, labels = _labels()
    valid = labels != 7
    with pytest.raises(ValueError, match=r"region 7\b"):
        dense.region_weights(labels, lat, valid=valid)
    many = (np.arange(lat.size).reshape(lat.shape) % 65) + 1          # 65 regions
    with pytest.raises(ValueError, match=r"65 regions.*label 65\b"):
        dense.region_weights(many, lat)
    ids, _ = dense.region_weights(np.minimum(many, 64), lat)          # 64 are fine
    assert ids.size == 64


# ---- the assembly -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_condition_numbers_are_what_the_bound_assumes(name):
    ref = fc.reference(name)
    print(f"case {name}: cond(S) = {ref['cond']:.2f}")
    assert ref["cond"] < 1e3
    assert round(ref["cond"]) == fc.COND[name]
    ratio = np.diag(ref["posterior"])[:5] / np.diag(ref["prior"])[:5]
    print(f"case {name}: posterior / prior = {np.round(ratio, 3)}")
    assert (ratio > 0.03).all() and (ratio < 0.7).all()             # neither trivial nor cancelling
    assert (ref["prior"][fc.I_ZERO] == 0).all() and (ref["posterior"][:, fc.I_ZERO] == 0).all()


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_the_corrected_reduction_is_second_order_and_the_plain_one_is_not(name):
    """A residual of 1e-6 |g_k| is planted in every solve: y_k = S^-1 (g_k - r_k).  The assembly from (prior, G^T Y, R^T Y)
    must land within tol^2 cond(S) sqrt(prior_kk prior_ll) of the reference; G^T Y alone must not -- this is what pins the form."""
    ref = fc.reference(name)
    tol = 1e-6
    rng = np.random.default_rng(5)
    G = ref["G"]
    Rm = rng.normal(size=G.shape)
    gn = np.linalg.norm(G, axis=0)
    Rm *= tol * gn / np.linalg.norm(Rm, axis=0)                     # (the zero functional: r = 0)
    Y = np.linalg.solve(ref["S"], G - Rm)
    assert np.allclose(np.linalg.norm(G - ref["S"] @ Y, axis=0)[gn > 0] / gn[gn > 0], tol, rtol=1e-6)
    out = dense.assemble_functional_covariance(ref["prior"], G.T @ Y, Rm.T @ Y, gn ** 2, (Rm ** 2).sum(axis=0), support=11)
    d = np.sqrt(np.diag(ref["prior"]))
    bound = tol * tol * ref["cond"] * d[:, None] * d[None, :]
    scale = np.where(bound > 0, bound, 1.0)
    e2 = np.abs(out["posterior"] - ref["posterior"])
    plain = 0.5 * (G.T @ Y + (G.T @ Y).T)
    e1 = np.abs((ref["prior"] - plain) - ref["posterior"])
    live = gn > 0
    print(f"case {name}: corrected {np.max(e2 / scale):.3g} of the bound, plain G^T Y {np.max(e1 / scale):.3g} of it; of the prior: "
          f"{np.max((e2 / (d[:, None] * d[None, :] + 1e-300))[np.ix_(live, live)]):.3g} and "
          f"{np.max((e1 / (d[:, None] * d[None, :] + 1e-300))[np.ix_(live, live)]):.3g}")
    assert (e2 <= bound).all()
    assert (e1 > bound).any() and np.max(e1 / scale) > 10.0
    # the correction only ever takes away from the reduction: no variance is understated
    assert (np.diag(out["reduction"]) <= np.diag(ref["reduction"]) * (1 + 1e-13)).all()
    assert np.array_equal(out["posterior"], out["posterior"].T) and np.array_equal(out["prior"], out["prior"].T)
    np.testing.assert_allclose(out["resid"][live], tol, rtol=1e-9)
    assert (out["resid"][~live] == 0).all() and out["support"] == 11
    assert (out["posterior"][fc.I_ZERO] == 0).all() and (out["posterior"][:, fc.I_ZERO] == 0).all()


# ---- what raises before any device call -----------------------------------------------------------------------------------------------
def test_the_driver_refuses_regions_outside_the_dense_mode(monkeypatch, tmp_path):
    lat, lon = syn.global_grid(6, 12)
    labels = np.ones(lat.shape, dtype=np.int64)
    path = tmp_path / "labels.npy"
    np.save(path, labels)
    for var in ("OISAT_OI_MODE", "OISAT_OI_REGIONS"):
        monkeypatch.delenv(var, raising=False)
    for mode in ("diag", "tiled"):
        o = oisatgmi()
        o.ctm_averaged_vcd = o.sat_averaged_vcd = o.sat_averaged_error = np.ones(lat.shape)
        o.grid_lat, o.grid_lon = lat, lon
        o.oi_mode, o.oi_regions = mode, labels
        with pytest.raises(ValueError, match="oi_regions belongs to the dense mode"):
            o.oi("TROPOMI")
        o.oi_regions = None
        monkeypatch.setenv("OISAT_OI_REGIONS", str(path))
        with pytest.raises(ValueError, match="oi_regions belongs to the dense mode"):
            o.oi("TROPOMI")
        monkeypatch.delenv("OISAT_OI_REGIONS")
    o = oisatgmi()
    o.oi_regions = str(tmp_path / "missing.npy")
    with pytest.raises(ValueError, match="cannot read"):
        o._regions_setting()
    o.oi_regions = str(path)
    assert np.array_equal(o._regions_setting(), labels)
    o.oi_regions = None
    assert o._regions_setting() is None
