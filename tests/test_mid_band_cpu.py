"""The middle stretch of the factor's K-loops on the host (``oisat_factor_mid``, ``oisat_dag_task_order_env``; no GPU): the
table's properties and where the rule switches it on, ticket words that do not know about it, and the NumPy emulation of the
launch's arithmetic (tests/mid_band_emul.py): with the middle K-blocks as split bf16 products at 2^-8 the refinement of the gain
solve sees the same preconditioner, where single bf16 over the same stretch does not."""
import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

import mid_band_emul as emu

NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
MID = "OISAT_FACTOR_MID_BITS"
ENV = "OISAT_ENVELOPE"
GC = 1


def _sorted_case(ny, nx, nobs, seed, **kw):
    p = syn.point_obs_case(ny, nx, nobs, seed, **kw)
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
    lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
    return p, o, lat, lon


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (CUT, FAR, MID, ENV):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("far_bits,bits", [(18, 8), (22, 12), (0, 8)])
def test_forced_table_properties(monkeypatch, far_bits, bits):
    """5 938 swath observations, cut-off forced to 2^-28, the far stretch to 2^-far_bits (0: off) and the middle one to 2^-bits:
    far <= mid <= i, non-decreasing, not empty, and no observation of block row i has a correlation of 2^-bits or more with
    one of a block column k < mid[i]; at or above the far bits, and at 0, mid == far."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 6000, 4000, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, str(far_bits))
    monkeypatch.setenv(MID, str(bits))
    env, far, mid = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    assert np.all(far <= mid) and np.all(mid <= np.arange(nb)) and np.all(np.diff(mid) >= 0)
    assert np.any(mid > far)
    if far_bits == 0:
        assert np.array_equal(far, first)                       # independent switches: the middle stretch starts at first[i]
    po = dense.unit_vectors(lat, lon).T
    for i in range(nb):
        if mid[i] == 0:
            continue
        rows = po[i * NB:(i + 1) * NB]
        corr = np.exp(-g * np.maximum(2.0 - 2.0 * (rows @ po[:mid[i] * NB].T), 0.0))
        assert corr.max() < 2.0 ** -bits, (i, corr.max())
    for n in ([far_bits, far_bits + 3] if far_bits else []) + [0]:
        monkeypatch.setenv(MID, str(n))
        assert np.array_equal(emu.tables(lat, g)[2], far), n


def test_malformed_values_and_tables_are_refused(monkeypatch):
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 3000, 4100, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, "16")
    env, far, mid = emu.tables(lat, g)
    nb = far.size
    lib = _hip.load_library()
    out = np.empty(nb, dtype=np.int32)

    def call(far_table):
        return lib.oisat_factor_mid(lat.ctypes.data, lat.size, _hip.C.c_double(g), env.ctypes.data, far_table.ctypes.data, out.ctypes.data)

    for bad in ("-1", "53", "0.5", "x", "8x"):
        monkeypatch.setenv(MID, bad)
        assert call(far) != 0, bad
    monkeypatch.setenv(MID, "8")
    assert call(far) == 0
    assert call(far + 1) != 0                                   # far[0] > 0: outside first <= far <= i
    below = far.copy()
    below[-1] = env[nb - 1] - 1
    assert call(below) != 0
    assert lib.oisat_factor_mid(lat.ctypes.data, lat.size, _hip.C.c_double(g), env.ctypes.data, None, out.ctypes.data) != 0
    assert lib.oisat_factor_mid(lat[::-1].copy().ctypes.data, lat.size, _hip.C.c_double(g), env.ctypes.data, far.ctypes.data, out.ctypes.data) != 0


@pytest.mark.parametrize("name,ny,nx,nobs,seed,L,swaths", [("config2", 360, 720, 10000, 4000, 500.0, False),
                                                          ("swath_20k", 360, 720, 20000, 4001, 300.0, True)])
def test_default_rule_off_where_the_chain_binds(name, ny, nx, nobs, seed, L, swaths):
    g = dense.decay_constant(L)
    p, o, lat, lon = _sorted_case(ny, nx, nobs, seed, swaths=swaths)
    env, far, mid = emu.tables(lat, g)
    assert np.array_equal(far, env[:far.size]) and np.array_equal(mid, far)


def test_default_rule_at_the_headline_size(monkeypatch):
    """The benchmark's month is tile-work-bound: the default rule has the far stretch and with it the middle one; 0 switches it
    off, OISAT_ENVELOPE=0 and a forced cut-off without a forced stretch too, and Gaspari-Cohn has none unless forced.  Prints the
    shares of K-blocks."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(720, 1440, 100000, 4000, swaths=True)
    env, far, mid = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    assert np.all(first <= far) and np.all(far <= mid) and np.all(mid <= np.arange(nb))
    assert np.any(far > first) and np.any(mid > far)
    n_far, n_mid, n_all = emu.mid_share(first, far, mid)
    print(f"headline: {n_far} far and {n_mid} middle of {n_all} K-blocks: shares {n_far / n_all:.3f}, {n_mid / n_all:.3f}")
    assert (n_far, n_all) == emu.far_emu.far_share(first, far)
    assert 0 < n_mid < n_all - n_far
    monkeypatch.setenv(MID, "0")
    assert np.array_equal(emu.tables(lat, g)[2], far)
    monkeypatch.delenv(MID)
    monkeypatch.setenv(ENV, "0")
    assert np.array_equal(emu.tables(lat, g)[2], first)
    monkeypatch.delenv(ENV)
    monkeypatch.setenv(CUT, "28")
    env28, far28, mid28 = emu.tables(lat, g)
    assert np.array_equal(far28, env28[:nb]) and np.array_equal(mid28, far28)
    monkeypatch.delenv(CUT)
    lib = _hip.load_library()
    env_gc, far_gc, mid_gc = (np.empty(2 * nb, dtype=np.int32), np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32))
    gd = _hip.C.c_double(g)
    assert lib.oisat_factor_envelope_corr(GC, lat.ctypes.data, lat.size, gd, env_gc.ctypes.data) == 0
    assert lib.oisat_factor_far_corr(GC, lat.ctypes.data, lat.size, gd, env_gc.ctypes.data, far_gc.ctypes.data) == 0
    assert lib.oisat_factor_mid_corr(GC, lat.ctypes.data, lat.size, gd, env_gc.ctypes.data, far_gc.ctypes.data, mid_gc.ctypes.data) == 0
    assert np.array_equal(mid_gc, far_gc) and np.array_equal(far_gc, env_gc[:nb])
    monkeypatch.setenv(MID, "8")
    assert lib.oisat_factor_mid_corr(GC, lat.ctypes.data, lat.size, gd, env_gc.ctypes.data, far_gc.ctypes.data, mid_gc.ctypes.data) == 0
    assert np.any(mid_gc > far_gc)


def test_ticket_words_do_not_change(monkeypatch):
    """oisat_dag_task_order_env takes no middle table: its list is a function of (first, far), and the middle table only
    splits each task's kfar .. kend, clamped as the kernel clamps it."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 6000, 4000, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, "18")
    monkeypatch.setenv(MID, "0")
    env, far, mid0 = emu.tables(lat, g)
    before = emu.tickets(env[:far.size], far)
    monkeypatch.setenv(MID, "8")
    env8, far8, mid = emu.tables(lat, g)
    assert np.array_equal(env8, env) and np.array_equal(far8, far) and np.any(mid > far)
    assert np.array_equal(emu.tickets(env[:far.size], far), before)
    r = emu.task_ranges(env[:far.size], far, mid)
    k0, kfar, kmid, kend = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    assert np.array_equal(kfar, before[(before[:, 0] & 255) != 0][:, 0] >> 18)
    assert np.all(k0 <= kfar) and np.all(kfar <= kmid) and np.all(kmid <= np.maximum(kend, kfar))
    assert np.any(kmid == kfar) and np.any((kmid == kend) & (kmid > kfar)) and np.any((kmid > kfar) & (kmid < kend))


@pytest.mark.parametrize("nobs,seed,L,far_bits", [(6000, 4000, 300.0, 18), (4000, 4000, 600.0, 16)])
def test_emulated_factor_preconditions_as_well(monkeypatch, nobs, seed, L, far_bits):
    """Swath months of 5 938 observations at L = 300 km (far 18) and 3 946 at 600 km (far 16), middle 8: the first residual of
    the factor with the split stretch is at most 1.05 x the all-fp32 emulation's, the second at most 2 x (seen: x 1.014 / x 1.05
    and x 0.959 / x 0.78); single bf16 over the same stretch raises the first residual at least 2 x
    (seen: 4.15 and 5.82)."""
    g = dense.decay_constant(L)
    p, o, lat, lon = _sorted_case(360, 720, nobs, seed, swaths=True)
    m = lat.size
    cell = dense.regular_grid_cell(p.lat, p.lon, lat, lon)
    sig = np.sqrt(p.Sa.ravel())[cell]
    var = np.ravel(p.obs_var)[o].astype(np.float64)
    y = np.ravel(np.where(p.obs_y < 0, 0, p.obs_y))[o]
    d = y - p.Xa.ravel()[cell]
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, str(far_bits))
    monkeypatch.setenv(MID, "8")
    env, far, mid = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    n_far, n_mid, n_all = emu.mid_share(first, far, mid)
    po = dense.unit_vectors(lat, lon).T
    S64 = emu.covariance(po, sig, var, g, dtype=np.float64)[:m, :m]
    S32 = emu.covariance(po, sig, var, g, first=first)
    res_fp32 = emu.refine(emu.factor(S32, first), S64, d)       # (numpy.linalg.cholesky raises if a diagonal block is not PD)
    res_mid = emu.refine(emu.factor(S32, first, far, mid), S64, d)
    res_single = emu.refine(emu.factor(S32, first, far, mid, middle="single"), S64, d)
    print(f"m = {m}, band {int((np.arange(nb) - first).max())}, far share {n_far / n_all:.3f}, middle share {n_mid / n_all:.3f}: "
          f"fp32 {res_fp32}, split {res_mid} (x {res_mid[0] / res_fp32[0]:.3f} / x {res_mid[1] / res_fp32[1]:.2f}), "
          f"single bf16 {res_single} (x {res_single[0] / res_fp32[0]:.2f})")
    assert n_mid > 0
    assert res_mid[0] <= 1.05 * res_fp32[0]
    assert res_mid[1] <= 2.0 * res_fp32[1]
    assert res_single[0] >= 2.0 * res_fp32[0]
