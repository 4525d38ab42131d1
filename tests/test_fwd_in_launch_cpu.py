"""Host logic of the build that zero-fills only what the last envelope left outside the new one
(``oisat_cov_build_cover``, the function ``oisat_cov_build_env_zeroed`` sizes its launch with; no device call): for pairs of
tables -- narrow to wide, wide to narrow, equal, no claim -- every lower tile outside the new envelope ends up zero-filled or
covered by the claim, every tile inside it is evaluated, and nothing else is touched."""
import ctypes as C

import numpy as np
import pytest

from oisatgmi import _hip


def cover(first, zero_first):
    lib = _hip.load_library()
    nb = first.size
    frm = np.full(nb, -7, dtype=np.int32)
    width, zeros = C.c_int64(-1), C.c_int64(-1)
    rc = lib.oisat_cov_build_cover(first.ctypes.data, None if zero_first is None else zero_first.ctypes.data, nb, frm.ctypes.data,
                                   C.byref(width), C.byref(zeros))
    assert rc == 0, lib.oisat_last_error()
    return frm, int(width.value), int(zeros.value)


def band(nb, width, shift=0):
    """A valid table: non-decreasing, first[i] <= max(i - 1, 0)."""
    first = np.maximum(np.arange(nb) - width + shift, 0)
    return np.minimum(first, np.maximum(np.arange(nb) - 1, 0)).astype(np.int32)


def random_table(rng, nb):
    first = np.zeros(nb, dtype=np.int32)
    for i in range(1, nb):
        first[i] = rng.integers(first[i - 1], max(i - 1, first[i - 1]) + 1)
    return first


def emulate(first, claim):
    """Tile states of block rows after the build: the buffer starts as the last run left it -- an old factor inside the
    claim's table, zeros left of it (the claim), or unknown everywhere without a claim."""
    nb = first.size
    frm, width, zeros = cover(first, claim)
    state = np.full((nb, nb), "?", dtype="<U1")
    for i in range(nb):
        if claim is not None:
            state[i, : max(int(claim[i]), 0)] = "0"
        assert 0 <= frm[i] <= first[i]
        state[i, frm[i]: first[i]] = "0"                    # zero-filled
        state[i, first[i]: i + 1] = "S"                     # evaluated
    return state, frm, width, zeros


def check(first, claim):
    nb = first.size
    state, frm, width, zeros = emulate(first, claim)
    for i in range(nb):
        assert (state[i, : first[i]] == "0").all(), (i, first[i], None if claim is None else claim[i])
        assert (state[i, first[i]: i + 1] == "S").all()
    # the launch: tile row 2 i + 1 needs 2 (i - from) + 2 tiles of 64 columns, and the widest row sets the grid
    need = 2 * (np.arange(nb) - frm) + 2
    assert width == need.max()
    assert zeros == int((first - frm).sum())
    return frm, width, zeros


def test_no_claim_fills_everything_outside():
    first = band(40, 6)
    frm, width, zeros = check(first, None)
    assert (frm == 0).all() and zeros == int(first.sum()) and width == 2 * 40


def test_equal_tables_fill_nothing():
    first = band(40, 6)
    frm, width, zeros = check(first, first.copy())
    assert zeros == 0 and (frm == first).all() and width == 2 * 6 + 2


def test_wide_to_narrow_fills_the_difference():
    wide, narrow = band(40, 11), band(40, 5)
    frm, width, zeros = check(narrow, wide)
    assert (frm == wide).all() and zeros == int((narrow - wide).sum()) > 0


def test_narrow_to_wide_fills_nothing():
    wide, narrow = band(40, 11), band(40, 5)
    frm, width, zeros = check(wide, narrow)
    assert zeros == 0 and (frm == wide).all()


def test_crossing_and_random_tables():
    rng = np.random.default_rng(12)
    a, b = band(64, 9, shift=3), band(64, 4)
    check(a, b)
    check(b, a)
    for _ in range(200):
        nb = int(rng.integers(1, 48))
        check(random_table(rng, nb), random_table(rng, nb) if rng.random() < 0.8 else None)


def test_claim_entries_are_clamped_and_first_is_checked():
    first = band(12, 3)
    claim = first.copy()
    claim[5] = -4                                           # a negative claim is "nothing claimed"
    claim[7] = 100                                          # beyond the envelope: the envelope's own start
    frm, _, _ = check(first, np.minimum(claim, first))      # (the emulation takes the claim at its word up to the envelope)
    frm2, _, _ = cover(first, claim)
    assert frm2[5] == 0 and frm2[7] == first[7]
    lib = _hip.load_library()
    bad = first.copy()
    bad[4] = 5                                              # first[i] > i
    assert lib.oisat_cov_build_cover(bad.ctypes.data, None, bad.size, None, None, None) != 0
    assert lib.oisat_cov_build_cover(first.ctypes.data, None, first.size, None, None, None) == 0
