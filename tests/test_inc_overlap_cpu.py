"""Host logic of the increment under the correction's sweeps (``oisat_gain_solve_fields``; no device call): where
``DenseAnalysis.run`` takes the new entry (``oisat_inc_overlap_plan``, with ``OISAT_INC_OVERLAP``) and the shape the correction's
sweeps take while the side stream's increment is in flight (``oisat_trsv_plan_overlap``)."""
import contextlib
import ctypes as C
import os

import pytest

from oisatgmi import _hip

SWITCH = "OISAT_INC_OVERLAP"
GAUSSIAN, GASPARI_COHN, SOAR = 0, 1, 3
MIN_ROWS = 256                                                  # kIncOverlapMinRows (csrc/dense_solve.hip)
SWEEP_WGS = 128                                                 # kIncOverlapSweepWgs


@contextlib.contextmanager
def switch(value):
    old = os.environ.get(SWITCH)
    try:
        if value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = value
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


def use(nb, nsys=1, kind=GAUSSIAN, refine=2, fields=1, drift=0):
    lib = _hip.load_library()
    out = C.c_int32(-1)
    rc = lib.oisat_inc_overlap_plan(nb, nsys, kind, refine, fields, drift, C.byref(out))
    assert rc == 0, lib.oisat_last_error()
    return int(out.value)


def sweep(fn, nb, band, cu):
    two, grid = C.c_int32(-1), C.c_int32(-1)
    assert fn(nb, band, cu, C.byref(two), C.byref(grid)) == 0
    return int(two.value), int(grid.value)


def test_rule_by_size():
    """Unset: the headline (782 block rows) takes the new entry, BASELINE's config 2 (79) and everything below the bound keep the
    two calls; the bound itself is in."""
    with switch(None):
        assert use(782) == 1
        assert use(79) == 0
        assert use(MIN_ROWS - 1) == 0 and use(MIN_ROWS) == 1
        assert use(1) == 0


@pytest.mark.parametrize("kw", [dict(nsys=2), dict(kind=GASPARI_COHN), dict(kind=SOAR), dict(refine=0), dict(fields=0), dict(drift=1)])
def test_what_is_not_legal_is_never_taken(kw):
    """More than one system, another model than the Gaussian, no refinement round, no fields, a drift: the old path, whatever
    the size and whatever the switch."""
    for value in (None, "1", "0"):
        with switch(value):
            assert use(782, **kw) == 0


def test_switch():
    """0: nowhere; 1: wherever it is legal, whatever the size; empty = unset; anything else is refused."""
    with switch("0"):
        assert use(782) == 0 and use(79) == 0
    with switch("1"):
        assert use(782) == 1 and use(79) == 1 and use(1) == 1
        assert use(79, refine=1) == 1
    with switch(""):
        assert use(782) == 1 and use(79) == 0
    lib = _hip.load_library()
    out = C.c_int32(-1)
    for bad in ("2", "on", "01", " 1"):
        with switch(bad):
            assert lib.oisat_inc_overlap_plan(782, 1, GAUSSIAN, 2, 1, 0, C.byref(out)) != 0
    with switch(None):
        for args in ((0, 1, GAUSSIAN, 2, 1, 0), (782, 0, GAUSSIAN, 2, 1, 0), (782, 1, GAUSSIAN, -1, 1, 0)):
            assert lib.oisat_inc_overlap_plan(*args, C.byref(out)) != 0
        assert lib.oisat_inc_overlap_plan(782, 1, GAUSSIAN, 2, 1, 0, None) != 0


@pytest.mark.parametrize("nb,band,cu,want", [(782, 81, 256, (1, SWEEP_WGS)),      # the headline at 2^-28: half the CUs
                                             (782, 111, 256, (1, SWEEP_WGS)),     # ... at 2^-52
                                             (782, 128, 256, (1, SWEEP_WGS)),     # the bound itself
                                             (782, 129, 256, (0, 782)),           # one past it: one tile, a workgroup per row
                                             (782, 0, 256, (0, 782)),             # a dense factor
                                             (79, 0, 256, (1, 79)),               # config 2: a CU per row, no band to bound the sweep
                                             (100, 40, 256, (1, 100)),            # fewer workgroups than the cap already
                                             (300, 40, 64, (0, 300))])            # band above half the CUs: one tile
def test_sweep_shape_while_overlapped(nb, band, cu, want):
    lib = _hip.load_library()
    assert sweep(lib.oisat_trsv_plan_overlap, nb, band, cu) == want


@pytest.mark.parametrize("nb", [1, 2, 79, 129, 300, 782, 5000])
@pytest.mark.parametrize("band", [0, 1, 64, 128, 129, 400])
@pytest.mark.parametrize("cu", [0, 1, 64, 256, 304])
def test_the_cap_only_narrows_a_two_tile_sweep(nb, band, cu):
    """Against oisat_trsv_plan over every combination: the same number of tiles, never more workgroups, never an empty grid, and
    a different grid only for two tiles over a band of 1 .. 128 block rows -- then exactly the cap."""
    lib = _hip.load_library()
    two0, grid0 = sweep(lib.oisat_trsv_plan, nb, band, cu)
    two1, grid1 = sweep(lib.oisat_trsv_plan_overlap, nb, band, cu)
    assert two1 == two0 and 1 <= grid1 <= grid0
    if grid1 != grid0:
        assert two0 == 1 and 0 < band <= SWEEP_WGS and grid0 > SWEEP_WGS and grid1 == SWEEP_WGS
    else:
        assert not (two0 == 1 and 0 < band <= SWEEP_WGS and grid0 > SWEEP_WGS)


def test_sweep_shape_arguments():
    lib = _hip.load_library()
    assert lib.oisat_trsv_plan_overlap(782, 81, 256, None, None) == 0
    for bad in ((0, 0, 256), (782, -1, 256), (782, 81, -1)):
        assert lib.oisat_trsv_plan_overlap(*bad, None, None) != 0
