"""The batches of tests/batch_cases.py and their float64 references, without a device: every condition that makes the
references trustworthy, the regimes the three correlation lengths are meant to select, the ``CELLS`` rule, the clearance of the
``one_hard`` / ``two_hard`` cases under emulation, and four mutations of a NumPy restatement, each of which puts the quantity that
tests/test_gpu_batch_abi.py tests at least a factor 10 beyond its bar on every member of ``mixed`` (three against checks a and c;
the residual block taken from a neighbour against check d's bit equality, as its docstring explains)."""
import numpy as np
import pytest
import scipy.linalg as sla

import batch_cases as bc

GAUSS = "gaussian"


# ---- the cases are what the GPU test takes them for ----------------------------------------------------------------------------
def test_mixed_order_sizes_grids_and_geometries():
    mem = bc.mixed()
    ms = [x.m for x in mem]
    assert sorted(ms, reverse=True) == [700, 385, 300, 257, 129, 128, 127, 64, 1]
    order = bc.table_order(ms)                                  # caller index of every table entry
    assert all(order[t] != t for t in range(len(ms))) and ms[0] != max(ms)
    assert [-(-ms[c] // bc.NB) for c in order] == sorted((-(-m // bc.NB) for m in ms), reverse=True)
    shapes = sorted((x.n // x.nx if x.nx else x.n, x.nx) for x in mem)
    assert shapes == sorted([(37, 50), (33, 65), (8, 32), (1, 1), (300, 0), (257, 0), (16, 48), (16, 48), (16, 48)])
    for x in mem:
        assert (np.diff(x.olat) >= 0).all() and np.allclose((x.oxyz ** 2).sum(0), 1.0, atol=1e-15)
        assert x.nx == 0 or x.n % x.nx == 0
    by = {x.name: x for x in mem}
    cap = by["cap385"]                                          # the pole: an observation at 90 exactly, cells on both sides
    assert cap.olat[-1] == 90.0 and (cap.glat == 90.0).any()
    row = cap.glon.reshape(33, 65)[16]
    assert (np.abs(row) < 1.0).any() and (np.abs(np.abs(row) - 180.0) < 1.0).any()
    dl = by["dateline700"]
    assert (dl.olon > 170).any() and (dl.olon < -170).any() and (np.abs(dl.olon) <= 180).all()
    assert (by["onelat300"].olat == by["onelat300"].olat[0]).all()
    tw = by["twin129"]
    k = np.flatnonzero((tw.olat[1:] == tw.olat[:-1]) & (tw.olon[1:] == tw.olon[:-1]))
    assert k.size == 1 and tw.ovar[k[0]] != tw.ovar[k[0] + 1]
    co = by["coincide257"]
    assert co.nx == 0 and (bc.chord2(co.gxyz, co.oxyz).min(axis=1) == 0.0).all()
    # the variants
    assert [x.perm_kind for x in bc.mixed_no_perm()].count(None) == 1
    for kind in ("identity", "reverse", "morton"):
        for x in bc.mixed_perm(kind):
            assert sorted(x.perm()) == list(range(x.m))
    assert (bc.mixed_perm("reverse")[3].perm()[:2] == [699, 698]).all()


def test_the_three_lengths_select_the_three_regimes():
    """Gaussian: 300 km compact blocks with a window, 800 km latitude rows with a window below 180 degrees, 5000 km no window;
    one member without a perm moves the batch to rows.  The other models shift the borders (recorded, and asserted as they
    are, so that a change of the library's rules shows here)."""
    assert [bc.regime(GAUSS, L) for L in bc.LENGTHS] == ["blocks", "rows", "full"]
    assert bc.regime(GAUSS, 300.0, all_perm=False) == "rows"
    assert bc.lat_window_deg(GAUSS, bc.decay(300.0)) < 30.0 and 30.0 < bc.lat_window_deg(GAUSS, bc.decay(800.0)) < 180.0
    assert [bc.regime("gaspari_cohn", L) for L in bc.LENGTHS] == ["blocks", "blocks", "full"]
    assert [bc.regime("soar", L) for L in bc.LENGTHS] == ["rows", "full", "full"]
    # the window really cuts something at 300 km (both windows active) and nothing in a member's box at 800 km
    win = bc.lat_window_deg(GAUSS, bc.decay(300.0))
    dl = bc.mixed()[3]
    j0, j1 = bc.window(dl, dl.glat[:50].min(), dl.glat[:50].max(), win)
    assert j0 == 0 and j1 < dl.m
    # Gaspari-Cohn: pairs inside and outside the support in every member of two observations or more, at 300 and 800 km
    for L in (300.0, 800.0):
        for x in bc.mixed():
            if x.m > 1:
                C = bc.corr(bc.chord2(x.oxyz, x.oxyz), L, "gaspari_cohn")
                assert (C == 0.0).any() and ((C > 0.0) & (C < 1.0)).any(), (x.name, L)


def test_cells_rule():
    """increment_cells as written in csrc/dense_solve_dev.inc: two cells per thread from cdiv(max_n, 512) nmem >= 4 CUs on."""
    tc = bc.two_cells()
    assert len(tc) == 64 and max(x.n for x in tc) == 8192 and all(130 <= x.m <= 300 for x in tc)
    assert any((x.n // x.nx, x.nx) == (37, 221) for x in tc if x.nx) and any(x.nx == 0 and x.n == 8191 for x in tc) and any(x.n == 1 for x in tc)
    assert bc.increment_cells(256, 8192, 64) == 2 and bc.increment_cells(256, 8192, 63) == 1 and bc.increment_cells(256, 8191 - 511, 64) == 1
    assert bc.increment_cells(0, 8192, 64) == 2 and bc.increment_cells(304, 8192, 64) == 1
    assert bc.increment_cells(256, max(x.n for x in bc.mixed()), 9) == 1
    assert bc.increment_blocks(37 * 221, 221, 2) == 7 * 3 and bc.increment_blocks(37 * 221, 221, 1) == 7 * 5
    assert bc.increment_blocks(8191, 0, 2) == 16 and bc.increment_blocks(1, 1, 2) == 1


@pytest.mark.parametrize("model", bc.MODELS)
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_conditions_on_mixed(L, model):
    for x in bc.mixed():
        S = x.S64(L, model)
        ev = np.linalg.eigvalsh(S)
        assert ev[0] >= bc.EIG_MIN * S.diagonal().max() and ev[-1] / ev[0] <= bc.COND_MAX, (x.name, ev[0], ev[-1])
        z = x.z_ref(L, model)
        assert np.linalg.norm(x.d - S @ z) <= 1e-12 * np.linalg.norm(x.d)
        assert x.delta(L, model) < 1e-5                         # of the order of 1e-6


def test_conditions_on_two_cells():
    for x in bc.two_cells():
        S = x.S64(bc.TWO_CELLS_L, GAUSS)
        ev = np.linalg.eigvalsh(S)
        assert ev[0] >= bc.EIG_MIN * S.diagonal().max() and ev[-1] / ev[0] <= bc.COND_MAX
        assert np.linalg.norm(x.d - S @ x.z_ref(bc.TWO_CELLS_L, GAUSS)) <= 1e-12 * np.linalg.norm(x.d)


def test_one_hard_and_two_hard_clearance():
    """Emulated (float32 LAPACK Cholesky as the preconditioner, float64 residuals, the library's stopping rule): behind the ONE
    correction of refine = 1 the hard members sit at least 100 x tol above, every other member -- its correction forced, the
    plain solve of the one-observation member is within tol already -- at most tol / 100; eight corrections bring the hard
    ones in.  Emulated |r_1| / |d|: 4.8e-5 (member 4), 1.6e-5 (member 7); the others at most 3.5e-11; tol = 1e-7."""
    L, model, tol = bc.HARD_L, bc.HARD_MODEL, bc.HARD_TOL
    two = bc.two_hard()
    order = bc.table_order([x.m for x in two])
    for h in (bc.HARD_MEMBER, bc.HARD_MEMBER_2):
        assert order.index(h) != h
    assert bc.HARD_MEMBER < bc.HARD_MEMBER_2 and order.index(bc.HARD_MEMBER) > order.index(bc.HARD_MEMBER_2)   # table order is the other way round
    assert 256 < two[bc.HARD_MEMBER].m < 400
    for i, x in enumerate(two):
        S = x.S64(L, model)
        ev = np.linalg.eigvalsh(S)
        assert ev[0] > 0
        sla.cho_factor(S.astype(np.float32), lower=True)        # positive definite in float32 LAPACK as well
        # (a hard member's z_ref is no reference: |z| ~ 1e4 |d| / |S|, so the float64 rounding of z alone leaves 1e-16 |S| |z| ~ 4e-11 |d|.
        # No GPU check uses it: the hard members are judged by the residual against S64.)
        hard = i in (bc.HARD_MEMBER, bc.HARD_MEMBER_2)
        assert np.linalg.norm(x.d - S @ x.z_ref(L, model)) <= (2.0 ** -52 * ev[-1] / ev[0] if hard else 1e-12) * np.linalg.norm(x.d)
        _, forced, _ = bc.emulate(x, L, model, 0.0, 1)
        _, n1, conv1 = bc.emulate(x, L, model, tol, 1)
        _, n8, conv8 = bc.emulate(x, L, model, tol, 8)
        print(f"member {i} (m = {x.m}): |r_k| / |d| at refine = 1: {n1}, at refine = 8: {n8}")
        if i in (bc.HARD_MEMBER, bc.HARD_MEMBER_2):
            assert not conv1 and n1[-1] >= 100 * tol and conv8 and len(n8) <= 8
        else:
            assert conv1 and forced[1] <= tol / 100 and ev[-1] / ev[0] <= bc.COND_MAX
    one = bc.one_hard()
    assert [i for i, x in enumerate(one) if not bc.emulate(x, L, model, tol, 1)[2]] == [bc.HARD_MEMBER]


# ---- the mutations -------------------------------------------------------------------------------------------------------------
def _resid_ratio(x, z, L, model, tol=bc.TOL):
    """check (a): |d - S64 z| over its bar tol |d| (1 + delta)."""
    return np.linalg.norm(x.d - x.S64(L, model) @ z) / (tol * np.linalg.norm(x.d) * (1.0 + x.delta(L, model, tol)))


def _refined(x, L, model, refine=2, tol=bc.TOL):
    return bc.emulate(x, L, model, tol, refine)[0]


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_unmutated_restatements_meet_the_bars(L):
    """The emulated solve meets check (a), the windowed increment of the restatement meets check (c): the mutations below
    are what moves them."""
    for x in bc.mixed():
        z = _refined(x, L, GAUSS)
        assert _resid_ratio(x, z, L, GAUSS) <= 1.0
        bar, _ = x.inc_bar(z, GAUSS)
        assert (np.abs(bc.inc_windowed(x, z, L, GAUSS) - x.inc_of(z, L, GAUSS)) <= bar).all()


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_mutation_two_members_z_swapped(L):
    """Every member handed the z of its neighbour in the library's table (cut or zero-filled to its size): check (a)."""
    mem = bc.mixed()
    order = bc.table_order([x.m for x in mem])
    for t, c in enumerate(order):
        x, y = mem[c], mem[order[t - 1]]
        z = np.zeros(x.m)
        q = min(x.m, y.m)
        z[:q] = _refined(y, L, GAUSS)[:q]
        r = _resid_ratio(x, z, L, GAUSS)
        print(f"L {L:g}: member {c} with the z of member {order[t - 1]}: {r:.3g} x bar")
        assert r >= 10.0


def _near_term(x, z, L, model, i):
    """An observation of the float64 tier of cell i (C >= 2^-28) whose term is the median of that tier's."""
    C = x.cross(L, model)[i]
    near = np.flatnonzero(C >= 2.0 ** -bc.FAR_BITS)
    t = np.abs(C[near] * x.osig[near] * z[near])
    return int(near[np.argsort(t)[t.size // 2]])


@pytest.mark.parametrize("model", bc.MODELS)
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_mutation_one_observation_dropped_from_one_cell(L, model):
    """check (c): one cell of every member without one in-window observation of its float64 tier (the median term)."""
    for c, x in enumerate(bc.mixed()):
        z = _refined(x, L, model)
        i = int(np.argmax((x.cross(L, model) >= 2.0 ** -bc.FAR_BITS).sum(axis=1)))        # the cell with the most such observations
        a = _near_term(x, z, L, model, i)
        bar, _ = x.inc_bar(z, model)
        err = np.abs(bc.inc_windowed(x, z, L, model, drop=(i, a)) - x.inc_of(z, L, model))
        print(f"L {L:g} {model}: member {c}, cell {i} without observation {a}: {err[i] / bar[i]:.3g} x bar")
        assert err[i] >= 10.0 * bar[i] and (np.delete(err, i) <= np.delete(bar, i)).all()


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_mutation_window_narrowed_at_an_edge_tie(L):
    """check (c): every workgroup's window ends one observation early (``<`` for ``<=`` at the upper edge: the last of the
    observations that tie with it goes).  Where a window is cut short of the member the lost term is below 2^-52 and nothing
    shows; where it reaches the member's northern end -- every block at 800 km and up, the northern blocks at 300 km -- the
    member's northernmost observation goes; on the one-latitude member every observation ties with that edge.  Judged on
    the member's worst cell."""
    for c, x in enumerate(bc.mixed()):
        z = _refined(x, L, GAUSS)
        bar, _ = x.inc_bar(z, GAUSS)
        err = np.abs(bc.inc_windowed(x, z, L, GAUSS, narrow="all") - x.inc_of(z, L, GAUSS))
        print(f"L {L:g}: member {c}: {(err / bar).max():.3g} x bar")
        assert (err / bar).max() >= 10.0


def _mutated_solve(x, L, model, neighbour_r, refine=2, tol=bc.TOL):
    """bc.emulate with the first block of 64 rows of every residual taken from the neighbour's (as many rows as both have)."""
    S = x.S64(L, model)
    F = sla.cho_factor(S.astype(np.float32), lower=True)
    solve = lambda r: sla.cho_solve(F, r.astype(np.float32)).astype(np.float64)       # noqa: E731
    dn = np.linalg.norm(x.d)
    z = solve(x.d)
    for k in range(refine + 1):
        r = x.d - S @ z
        rn = neighbour_r[min(k, len(neighbour_r) - 1)]
        q = min(64, x.m, rn.size)
        r[:q] = rn[:q]
        if np.linalg.norm(r) <= tol * dn or k == refine:
            break
        z = z + solve(r)
    return z


def _residuals(x, L, model, d=None, refine=2, tol=bc.TOL):
    y = x if d is None else x.clone(d=d)
    S = y.S64(L, model)
    F = sla.cho_factor(S.astype(np.float32), lower=True)
    solve = lambda r: sla.cho_solve(F, r.astype(np.float32)).astype(np.float64)       # noqa: E731
    z, out = solve(y.d), []
    for k in range(refine + 1):
        out.append(y.d - S @ z)
        if np.linalg.norm(out[-1]) <= tol * np.linalg.norm(y.d) or k == refine:
            break
        z = z + solve(out[-1])
    return out


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_mutation_a_residual_block_from_the_neighbouring_member(L):
    """What catches this one is check (d), not the residual's norm: the rows a member takes from its neighbour are themselves
    residuals, ~1e-6 |d|, and leave |d - S z| at 0.05 .. 4 times the bar of check (a) at the default tolerance -- printed --
    which is no detection.  But the member's z then depends on the NEIGHBOUR's innovation, and check (d) changes one member's d
    and asserts the others' bits: its bar is 0.  Asserted here, at the tolerance check (d) runs at (HARD_TOL, so that every
    member of two observations or more takes a correction and so reads its residual at all): with the neighbour's d changed
    as the GPU test changes it (every member in turn), the mutated z moves by at least 10 units of 2^-52 max |z| -- 2e9 and more
    on every member, the one-observation member included: the one row it takes is above tol |d|."""
    mem = bc.mixed()
    order = bc.table_order([x.m for x in mem])
    tol = bc.HARD_TOL
    for t, c in enumerate(order):
        x, y = mem[c], mem[order[t - 1]]
        assert x.m == 1 or len(bc.emulate(x, L, GAUSS, tol, 2)[1]) >= 2          # unmutated: at least one correction
        z1 = _mutated_solve(x, L, GAUSS, _residuals(y, L, GAUSS, tol=tol), tol=tol)
        z2 = _mutated_solve(x, L, GAUSS, _residuals(y, L, GAUSS, d=bc.changed_d(y), tol=tol), tol=tol)
        moved = np.abs(z1 - z2).max() / (2.0 ** -52 * np.abs(z1).max())
        z0 = _mutated_solve(x, L, GAUSS, _residuals(y, L, GAUSS))
        print(f"L {L:g}: member {c} <- member {order[t - 1]}: check (a) at the default tolerance {_resid_ratio(x, z0, L, GAUSS):.2f} x bar; "
              f"z moves by {moved:.3g} x 2^-52 max |z|")
        assert moved >= 10.0
