"""Host-only tests of the addressing of the factor's shadow (``oisat_factor_shadow_layout``; csrc/dense_dag.inc "Shadow"):
the strictly-lower tiles (r, k), first[r] <= k < r, row after row."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip


def _layout(first):
    first = np.ascontiguousarray(first, dtype=np.int32)
    rowoff = np.full(max(first.size, 1), -7, dtype=np.int64)
    ntiles = C.c_int64(-7)
    rc = _hip.load_library().oisat_factor_shadow_layout(int(first.size), first.ctypes.data, rowoff.ctypes.data, C.byref(ntiles))
    return rc, rowoff[:first.size], ntiles.value


def _numpy_layout(first):
    width = np.arange(first.size, dtype=np.int64) - np.asarray(first, dtype=np.int64)       # tiles of each block row
    return np.concatenate(([0], np.cumsum(width)[:-1])), int(width.sum())


def _enveloped(nb, band, seed):
    """A non-decreasing table with first[i] <= max(i - 1, 0) and rows of at most `band` tiles, with plateaus and jumps."""
    rng = np.random.default_rng(seed)
    first = np.zeros(nb, dtype=np.int32)
    for i in range(1, nb):
        lo = max(int(first[i - 1]), i - band)
        first[i] = rng.integers(lo, i) if rng.random() < 0.6 else lo      # (high end exclusive: at most i - 1)
    return first


TABLES = {
    "dense": np.zeros(37, dtype=np.int32),
    "narrowest": np.maximum(np.arange(29, dtype=np.int32) - 1, 0),
    "enveloped": _enveloped(61, 9, 1),
    "enveloped_wide": _enveloped(1024, 81, 2),
    "two_rows": np.zeros(2, dtype=np.int32),
    "single_row": np.zeros(1, dtype=np.int32),
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_layout_against_numpy(name):
    first = TABLES[name]
    rc, rowoff, ntiles = _layout(first)
    assert rc == 0
    want_off, want_n = _numpy_layout(first)
    assert np.array_equal(rowoff, want_off)
    assert ntiles == want_n == int((np.arange(first.size) - first).sum())
    # every block row below the first holds at least its sub-diagonal tile: the offsets increase strictly from row 1 on,
    # row 0 has no tile, and tile (r, k) -> rowoff[r] + (k - first[r]) numbers the tiles 0 .. ntiles - 1 once each
    assert rowoff[0] == 0 and np.all(np.diff(rowoff[1:]) > 0)
    if first.size > 1:
        assert rowoff[1] == 0
    ids = np.concatenate([rowoff[r] + np.arange(r - first[r]) for r in range(first.size)] + [np.empty(0, dtype=np.int64)])
    assert np.array_equal(ids, np.arange(ntiles))


def test_single_row_has_no_tile():
    rc, rowoff, ntiles = _layout(TABLES["single_row"])
    assert rc == 0 and ntiles == 0 and rowoff.tolist() == [0]


@pytest.mark.parametrize("bad", [
    [0, 1, 1],            # first[1] > 0: the sub-diagonal tile is inside every envelope
    [0, 0, 2],            # first[2] > 1
    [0, 0, 1, 0],         # decreasing
    [-1, 0, 0],           # negative
    [1],                  # first[0] must be 0
])
def test_bad_tables_are_rejected(bad):
    rc, _, ntiles = _layout(np.array(bad, dtype=np.int32))
    assert rc != 0 and ntiles == -7


def test_bad_arguments_are_rejected():
    lib = _hip.load_library()
    first = np.zeros(4, dtype=np.int32)
    rowoff = np.zeros(4, dtype=np.int64)
    n = C.c_int64(0)
    assert lib.oisat_factor_shadow_layout(0, first.ctypes.data, rowoff.ctypes.data, C.byref(n)) != 0
    assert lib.oisat_factor_shadow_layout(4, None, rowoff.ctypes.data, C.byref(n)) != 0
    assert lib.oisat_factor_shadow_layout(4, first.ctypes.data, None, C.byref(n)) != 0
    assert lib.oisat_factor_shadow_layout(4, first.ctypes.data, rowoff.ctypes.data, None) != 0
    too_many = np.zeros(1025, dtype=np.int32)                   # an enveloped ticket has ten bits for a block column
    assert lib.oisat_factor_shadow_layout(1025, too_many.ctypes.data, np.zeros(1025, dtype=np.int64).ctypes.data, C.byref(n)) != 0
    assert lib.oisat_factor_shadow_layout(4, first.ctypes.data, rowoff.ctypes.data, C.byref(n)) == 0 and n.value == 6
