"""Host logic of the triangular sweeps' launch rule (``oisat_trsv_plan``, the function ``trsv_solve`` takes its grid and
its number of LDS tiles from; no device call): two tiles when every block row gets its own CU or when an enveloped factor's
band is at most half the CUs, then one workgroup per CU at the most; one tile and a workgroup per row otherwise."""
import ctypes as C

import pytest

from oisatgmi import _hip


def plan(nb, band, cu_count):
    lib = _hip.load_library()
    two, grid = C.c_int32(-1), C.c_int32(-1)
    rc = lib.oisat_trsv_plan(nb, band, cu_count, C.byref(two), C.byref(grid))
    assert rc == 0, lib.oisat_last_error()
    return int(two.value), int(grid.value)


@pytest.mark.parametrize("nb,band,cu,want", [(79, 0, 256, (1, 79)),         # config 2: a CU per row, today's rule
                                             (781, 0, 256, (0, 781)),       # a large dense factor: bound by streaming L
                                             (781, 81, 256, (1, 256)),      # the headline at 2^-28
                                             (781, 111, 256, (1, 256)),     # the headline at 2^-52
                                             (781, 128, 256, (1, 256)),     # the bound itself
                                             (781, 129, 256, (0, 781)),     # one past it
                                             (300, 40, 256, (1, 256)),
                                             (256, 0, 256, (1, 256)),
                                             (257, 0, 256, (0, 257))])
def test_the_rule(nb, band, cu, want):
    assert plan(nb, band, cu) == want


@pytest.mark.parametrize("nb", [1, 2, 79, 781])
@pytest.mark.parametrize("band", [0, 1, 2, 81, 781])
@pytest.mark.parametrize("cu", [0, 1, 2, 3, 256])
def test_a_grid_is_never_empty(nb, band, cu):
    """Every combination, cu_count = 0 (an unknown device) and nb = 1 among them: no division by zero, 1 <= grid <= nb, two
    tiles never on more workgroups than CUs, and two tiles exactly where the rule says."""
    two, grid = plan(nb, band, cu)
    assert 1 <= grid <= nb
    assert two == int(nb <= cu or 0 < band <= cu // 2)
    assert grid == (min(nb, cu) if two else nb)


def test_out_pointers_are_optional_and_arguments_checked():
    lib = _hip.load_library()
    assert lib.oisat_trsv_plan(781, 81, 256, None, None) == 0
    grid = C.c_int32(-1)
    assert lib.oisat_trsv_plan(781, 81, 256, None, C.byref(grid)) == 0 and grid.value == 256
    for bad in ((0, 0, 256), (-1, 0, 256), (781, -1, 256), (781, 81, -1)):
        assert lib.oisat_trsv_plan(*bad, None, None) != 0
