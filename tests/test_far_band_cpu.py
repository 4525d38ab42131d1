"""The far stretch of the factor's K-loops on the host (``oisat_factor_far``, ``oisat_dag_task_order_env``; no GPU): the
table's properties and where the rule switches it on, the tickets' ``k0 <= kfar <= kend``, and the NumPy emulation of the
launch's arithmetic (tests/far_band_emul.py): with the far K-blocks' operands rounded to bf16 at 2^-16 the refinement of the
gain solve sees the same preconditioner."""
import numpy as np
import pytest

from oisatgmi import dense, synthetic as syn

import far_band_emul as emu

NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
ENV = "OISAT_ENVELOPE"


def _sorted_case(ny, nx, nobs, seed, **kw):
    p = syn.point_obs_case(ny, nx, nobs, seed, **kw)
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
    lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
    return p, o, lat, lon


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (CUT, FAR, ENV):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("bits", [16, 22])
def test_forced_table_properties(monkeypatch, bits):
    """3 000 swath observations, cut-off forced to 2^-28 and the stretch to 2^-bits: first <= far <= i, the stretch is not
    empty, and no observation of block row i has a correlation of 2^-bits or more with one of a block column k < far[i]."""
    L = 300.0
    g = dense.decay_constant(L)
    p, o, lat, lon = _sorted_case(360, 720, 3000, 4100, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, str(bits))
    env, far = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    assert np.all(first <= far) and np.all(far <= np.arange(nb))
    assert np.any(far > first)
    po = dense.unit_vectors(lat, lon).T
    for i in range(nb):
        if far[i] == 0:
            continue
        rows = po[i * NB:(i + 1) * NB]
        corr = np.exp(-g * np.maximum(2.0 - 2.0 * (rows @ po[:far[i] * NB].T), 0.0))
        assert corr.max() < 2.0 ** -bits, (i, corr.max())
    # a stretch cut at or above the table's own cut-off leaves nothing far
    monkeypatch.setenv(FAR, "28")
    assert np.array_equal(emu.tables(lat, g)[1], first)


def test_where_the_stretch_is_off(monkeypatch):
    """far == first at a chain-bound size by default (the rule keeps the 2^-52 table there), under a forced cut-off without a
    forced stretch, with the override at 0 and with OISAT_ENVELOPE=0; a bad override is refused."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 3000, 4100, swaths=True)
    env, far = emu.tables(lat, g)
    nb = far.size
    assert np.array_equal(far, env[:nb])
    monkeypatch.setenv(CUT, "28")
    env28, far28 = emu.tables(lat, g)
    assert np.array_equal(far28, env28[:nb])
    monkeypatch.setenv(FAR, "0")
    assert np.array_equal(emu.tables(lat, g)[1], env28[:nb])
    monkeypatch.setenv(FAR, "16")
    on = emu.tables(lat, g)[1]
    assert np.any(on > env28[:nb])
    monkeypatch.setenv(ENV, "0")
    assert np.array_equal(emu.tables(lat, g)[1], env28[:nb])
    monkeypatch.delenv(ENV)
    from oisatgmi import _hip
    lib = _hip.load_library()
    for bad in ("-1", "53", "0.5", "x"):
        monkeypatch.setenv(FAR, bad)
        out = np.empty(nb, dtype=np.int32)
        assert lib.oisat_factor_far(lat.ctypes.data, lat.size, _hip.C.c_double(g), env28.ctypes.data, out.ctypes.data) != 0, bad


def test_default_rule_at_the_headline_size(monkeypatch):
    """The benchmark's month is tile-work-bound: the default rule has the narrow table and with it the stretch; 0 switches it
    off.  Prints the far share of K-blocks."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(720, 1440, 100000, 4000, swaths=True)
    env, far = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    assert np.all(first <= far) and np.all(far <= np.arange(nb)) and np.any(far > first)
    n_far, n_all = emu.far_share(first, far)
    print(f"headline: {n_far} of {n_all} K-blocks are far: share {n_far / n_all:.3f}")
    assert 0 < n_far < n_all
    monkeypatch.setenv(FAR, "0")
    assert np.array_equal(emu.tables(lat, g)[1], first)


@pytest.mark.parametrize("bits", [None, 16])
def test_tickets_carry_the_stretch(monkeypatch, bits):
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 3000, 4100, swaths=True)
    monkeypatch.setenv(CUT, "28")
    if bits is not None:
        monkeypatch.setenv(FAR, str(bits))
    env, far = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    t = emu.tickets(first, far if bits is not None else None)
    kind, k0, kfar = t[:, 0] & 255, (t[:, 0] >> 8) & 1023, t[:, 0] >> 18
    bulk = kind != 0
    assert bulk.sum() == t.shape[0] - 1
    i, j = t[bulk, 2], t[bulk, 3]
    kend = np.where(kind[bulk] == 3, j - 1, j)
    assert np.array_equal(k0[bulk], first[i])
    assert np.all(k0[bulk] <= kfar[bulk]) and np.all(kfar[bulk] <= kend)
    assert np.array_equal(kfar[bulk], np.clip(far[i] if bits is not None else first[i], k0[bulk], kend))
    for kd in (1, 2, 3):
        assert np.any(kind == kd)
    if bits is not None:                                        # all three positions of the boundary occur
        assert np.any(kfar[bulk] == k0[bulk]) and np.any(kfar[bulk] == kend) and np.any((kfar[bulk] > k0[bulk]) & (kfar[bulk] < kend))
        assert np.any((kind[bulk] != 1) & (kfar[bulk] > k0[bulk]))
    else:
        assert np.array_equal(kfar[bulk], k0[bulk])


@pytest.mark.parametrize("nobs,seed,L", [(6000, 4000, 300.0), (4000, 4000, 600.0)])
def test_emulated_factor_preconditions_as_well(monkeypatch, nobs, seed, L):
    """Swath months of 5 938 observations at L = 300 km and 3 946 at 600 km, f = 16: the first residual of the far-rounded
    factor is at most 1.05 x the all-fp32 emulation's, the second at most 2 x; both factors are positive definite."""
    g = dense.decay_constant(L)
    p, o, lat, lon = _sorted_case(360, 720, nobs, seed, swaths=True)
    m = lat.size
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    sig = np.sqrt(p.Sa.ravel())[cell]
    var = np.ravel(p.obs_var)[o].astype(np.float64)
    y = np.ravel(np.where(p.obs_y < 0, 0, p.obs_y))[o]
    d = y - p.Xa.ravel()[cell]
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, "16")
    env, far = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    n_far, n_all = emu.far_share(first, far)
    po = dense.unit_vectors(lat, lon).T
    S64 = emu.covariance(po, sig, var, g, dtype=np.float64)[:m, :m]
    S32 = emu.covariance(po, sig, var, g, first=first)
    res_fp32 = emu.refine(emu.factor(S32, first), S64, d)       # (numpy.linalg.cholesky raises if a diagonal block is not PD)
    res_far = emu.refine(emu.factor(S32, first, far), S64, d)
    print(f"m = {m}, band {int((np.arange(nb) - first).max())}, far share {n_far / n_all:.3f}: fp32 {res_fp32}, far {res_far}")
    assert n_far > 0
    assert res_far[0] <= 1.05 * res_fp32[0]
    assert res_far[1] <= 2.0 * res_fp32[1]
