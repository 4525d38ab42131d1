"""The near stretch of the factor's K-loops on the host (``oisat_factor_near``; no GPU): the table against the emulation's own,
its clamps, the spellings of ``OISAT_FACTOR_NEAR_BITS``, where the rule switches it on, the refusals of ``near_table_ok``'s
callers' arguments, and the arithmetic of the three-way bf16 split (tests/near_band_emul.py) against its bounds."""
import numpy as np
import pytest

from oisatgmi import _hip, dense, synthetic as syn

import near_band_emul as emu

NB = 128
CUT = "OISAT_FACTOR_CUT_BITS"
FAR = "OISAT_FACTOR_FAR_BITS"
MID = "OISAT_FACTOR_MID_BITS"
NEAR = "OISAT_FACTOR_NEAR_BITS"
ENV = "OISAT_ENVELOPE"
GC, SOAR = 1, 3
OISAT_EINVAL = -1


def _sorted_case(ny, nx, nobs, seed, **kw):
    p = syn.point_obs_case(ny, nx, nobs, seed, **kw)
    o = np.argsort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    lat = np.ascontiguousarray(np.ravel(p.obs_lat)[o], dtype=np.float64)
    lon = np.ascontiguousarray(np.ravel(p.obs_lon)[o], dtype=np.float64)
    return p, o, lat, lon


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (CUT, FAR, MID, NEAR, ENV):
        monkeypatch.delenv(k, raising=False)


def _reference_table(lat, lon, g, bits, lower):
    """near[i] by the rule itself: the largest k <= i, k >= lower[i], such that the latitude window of 2^-bits keeps every block
    column below k out of block row i -- the library's table is a latitude bound, so the reference is one too: block column k is
    out when its largest latitude lies more than the cut-off's angle below the row's smallest."""
    nb = lower.size
    m = lat.size
    chord = _hip.C.c_double(0.0)
    assert _hip.load_library().oisat_corr_cut_chord(0, _hip.C.c_double(g), _hip.C.c_double(bits), _hip.C.byref(chord)) == 0
    angle = 1e9 if chord.value >= 2.0 else 2.0 * np.arcsin(0.5 * chord.value) * 57.29577951308232
    out = np.empty(nb, dtype=np.int32)
    for i in range(nb):
        lo = lat[i * NB] - angle
        k = 0
        while k < i and lat[min((k + 1) * NB, m) - 1] < lo:
            k += 1
        out[i] = min(max(k, lower[i]), i)
    return out


@pytest.mark.parametrize("far_bits,mid_bits,bits", [(18, 8, 4), (22, 12, 2), (0, 0, 6), (18, 8, 1)])
def test_forced_table_against_the_rule(monkeypatch, far_bits, mid_bits, bits):
    """5 938 swath observations, cut-off forced to 2^-28: the near table at 2^-bits is the rule's (a latitude window) clamped
    into mid <= near <= i, non-decreasing; no observation of block row i has a correlation of 2^-bits or more with one of a block
    column k < near[i] that is not already below mid[i]; at 0 near == mid; `all` is near[i] = i."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 6000, 4000, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, str(far_bits))
    monkeypatch.setenv(MID, str(mid_bits))
    monkeypatch.setenv(NEAR, str(bits))
    env, far, mid, near = emu.tables(lat, g)
    nb = far.size
    assert np.all(mid <= near) and np.all(near <= np.arange(nb)) and np.all(np.diff(near) >= 0)
    assert np.any(near > mid)
    assert np.array_equal(near, _reference_table(lat, lon, g, bits, mid))
    po = dense.unit_vectors(lat, lon).T
    for i in range(nb):
        if near[i] == mid[i]:
            continue
        rows = po[i * NB:(i + 1) * NB]
        corr = np.exp(-g * np.maximum(2.0 - 2.0 * (rows @ po[:near[i] * NB].T), 0.0))
        assert corr.max() < 2.0 ** -bits, (i, corr.max())
    monkeypatch.setenv(NEAR, "0")
    assert np.array_equal(emu.tables(lat, g)[3], mid)
    monkeypatch.setenv(NEAR, "all")
    assert np.array_equal(emu.tables(lat, g)[3], np.arange(nb))
    monkeypatch.setenv(NEAR, "52")                              # at or above the cut-offs below it: clamped to mid
    assert np.array_equal(emu.tables(lat, g)[3], mid)


def test_values_and_tables_that_are_refused(monkeypatch):
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 3000, 4100, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, "16")
    monkeypatch.setenv(MID, "8")
    env, far, mid, near = emu.tables(lat, g)
    nb = far.size
    lib = _hip.load_library()
    out = np.empty(nb, dtype=np.int32)
    gd = _hip.C.c_double(g)

    def call(mid_table, lat_=lat):
        return lib.oisat_factor_near(lat_.ctypes.data, lat_.size, gd, env.ctypes.data, None if mid_table is None else mid_table.ctypes.data,
                                     out.ctypes.data)

    for bad in ("-1", "53", "0.5", "x", "8x", "ALL", "all ", "al"):
        monkeypatch.setenv(NEAR, bad)
        assert call(mid) == OISAT_EINVAL, bad
    for good in ("0", "all", "1", "52", "4"):
        monkeypatch.setenv(NEAR, good)
        assert call(mid) == 0, good
    assert call(mid + 1) != 0                                   # mid[0] > 0: outside first <= mid <= i
    below = mid.copy()
    below[-1] = env[nb - 1] - 1
    assert call(below) != 0
    assert call(None) != 0
    assert call(mid, lat[::-1].copy()) != 0


@pytest.mark.parametrize("name,ny,nx,nobs,seed,L,swaths", [("config2", 360, 720, 10000, 4000, 500.0, False),
                                                          ("swath_20k", 360, 720, 20000, 4001, 300.0, True)])
def test_default_rule_off_where_the_chain_binds(name, ny, nx, nobs, seed, L, swaths):
    g = dense.decay_constant(L)
    p, o, lat, lon = _sorted_case(ny, nx, nobs, seed, swaths=swaths)
    env, far, mid, near = emu.tables(lat, g)
    assert np.array_equal(far, env[:far.size]) and np.array_equal(mid, far) and np.array_equal(near, mid)


def test_default_rule_at_the_headline_size(monkeypatch):
    """The benchmark's month is tile-work-bound: the default rule is whatever kFactorNearBits says there (printed, with the shares
    of K-blocks; `all` makes near[i] = i) and obeys the clamps; 0 switches it off, OISAT_ENVELOPE=0 and a forced cut-off without a
    forced stretch too, and Gaspari-Cohn and SOAR have none unless forced."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(720, 1440, 100000, 4000, swaths=True)
    env, far, mid, near = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    assert np.all(mid <= near) and np.all(near <= np.arange(nb))
    monkeypatch.setenv(NEAR, "all")
    near_all = emu.tables(lat, g)[3]
    assert np.array_equal(near_all, np.arange(nb))
    n_far, n_mid, n_near, n_all = emu.near_share(first, far, mid, near_all)
    n_def = emu.near_share(first, far, mid, near)[2]
    print(f"headline: {n_far} far, {n_mid} middle and {n_near} near (`all`; by default {n_def}) of {n_all} K-blocks: shares "
          f"{n_far / n_all:.3f}, {n_mid / n_all:.3f}, {n_near / n_all:.3f}")
    assert n_far + n_mid + n_near == n_all and n_near > 0       # `all` leaves the fp32 pipe nothing of the bulk K-loops
    assert (n_far, n_mid, n_all) == emu.mid_emu.mid_share(first, far, mid)
    monkeypatch.setenv(NEAR, "0")
    assert np.array_equal(emu.tables(lat, g)[3], mid)
    monkeypatch.setenv(NEAR, "4")
    near4 = emu.tables(lat, g)[3]
    assert np.all(mid <= near4) and np.all(near4 <= near_all) and np.any(near4 > mid) and np.any(near4 < near_all)
    monkeypatch.delenv(NEAR)
    monkeypatch.setenv(ENV, "0")
    assert np.array_equal(emu.tables(lat, g)[3], first)
    monkeypatch.delenv(ENV)
    monkeypatch.setenv(CUT, "28")
    env28, far28, mid28, near28 = emu.tables(lat, g)
    assert np.array_equal(far28, env28[:nb]) and np.array_equal(mid28, far28) and np.array_equal(near28, mid28)
    monkeypatch.delenv(CUT)
    lib = _hip.load_library()
    gd = _hip.C.c_double(g)
    for kind in (GC, SOAR):
        env_k, far_k, mid_k, near_k = (np.empty(2 * nb, dtype=np.int32), np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32),
                                       np.empty(nb, dtype=np.int32))
        assert lib.oisat_factor_envelope_corr(kind, lat.ctypes.data, lat.size, gd, env_k.ctypes.data) == 0
        assert lib.oisat_factor_far_corr(kind, lat.ctypes.data, lat.size, gd, env_k.ctypes.data, far_k.ctypes.data) == 0
        assert lib.oisat_factor_mid_corr(kind, lat.ctypes.data, lat.size, gd, env_k.ctypes.data, far_k.ctypes.data, mid_k.ctypes.data) == 0
        assert lib.oisat_factor_near_corr(kind, lat.ctypes.data, lat.size, gd, env_k.ctypes.data, mid_k.ctypes.data, near_k.ctypes.data) == 0
        assert np.array_equal(near_k, mid_k) and np.array_equal(mid_k, env_k[:nb])
        monkeypatch.setenv(NEAR, "all")
        assert lib.oisat_factor_near_corr(kind, lat.ctypes.data, lat.size, gd, env_k.ctypes.data, mid_k.ctypes.data, near_k.ctypes.data) == 0
        assert np.array_equal(near_k, np.arange(nb))
        monkeypatch.delenv(NEAR)


def test_ranges_are_clamped_as_the_kernel_clamps_them(monkeypatch):
    """The ticket words do not know about the table; every bulk task's ranges are ordered k0 <= kfar <= kmid <= knear <= max(kend, .)
    and with `all` the near range ends at kend."""
    g = dense.decay_constant(300.0)
    p, o, lat, lon = _sorted_case(360, 720, 6000, 4000, swaths=True)
    monkeypatch.setenv(CUT, "28")
    monkeypatch.setenv(FAR, "18")
    monkeypatch.setenv(MID, "8")
    monkeypatch.setenv(NEAR, "0")
    env, far, mid, near0 = emu.tables(lat, g)
    before = emu.tickets(env[:far.size], far)
    monkeypatch.setenv(NEAR, "all")
    env1, far1, mid1, near = emu.tables(lat, g)
    assert np.array_equal(env1, env) and np.array_equal(far1, far) and np.array_equal(mid1, mid)
    assert np.array_equal(emu.tickets(env[:far.size], far), before)
    r = emu.task_ranges(env[:far.size], far, mid, near)
    k0, kfar, kmid, knear, kend = r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7]
    assert np.all(k0 <= kfar) and np.all(kfar <= kmid) and np.all(kmid <= knear) and np.all(knear == np.maximum(kend, kmid))
    r0 = emu.task_ranges(env[:far.size], far, mid, near0)
    assert np.array_equal(r0[:, 6], r0[:, 5])


def _random_fp32():
    """1e5 fp32 values with random bits -- every exponent, both signs --, with +-0 and 2 000 denormals put in; no inf, no NaN."""
    rng = np.random.default_rng(27)
    bits = rng.integers(0, 2 ** 32, size=100000, dtype=np.uint64).astype(np.uint32)
    a = bits.view(np.float32).copy()
    a[~np.isfinite(a)] = 1.0
    a[:4] = np.array([0.0, -0.0, np.float32(1e-45), np.float32(-1e-40)], dtype=np.float32)
    a[4:2004] = (rng.standard_normal(2000) * 1e-41).astype(np.float32)
    return a


def _terms(a, b):
    """(a b in float64, the sum of the kernel's products of the parts in float64, the parts of a and of b)"""
    pa = dict(zip(("hi", "mid", "lo"), (v.astype(np.float64) for v in emu.split3(a))))
    pb = dict(zip(("hi", "mid", "lo"), (v.astype(np.float64) for v in emu.split3(b))))
    return a.astype(np.float64) * b.astype(np.float64), sum(pa[x] * pb[y] for x, y in emu.TERMS), pa, pb


def test_three_way_split_reproduces_its_operand():
    """hi + mid + lo against a, within 2^-27 |a|; each part is a bf16; zeros stay zeros.
    Measured: over the 87 717 values of 2^-100 <= |a| < 3.38e38 the remainder is EXACTLY zero -- three parts of eight
    significant bits each hold fp32's 24.  Below 2^-100 (12 279 values) the parts run into bf16's denormal range (smallest
    2^-133) and the remainder is bounded absolutely, by 2^-134 = 4.59e-41 -- half of the smallest bf16 denormal, reached --, not
    relatively: only that is asserted there.  Within half a bf16 ulp of FLT_MAX hi rounds to infinity, as v_cvt_pk_bf16_f32 does: left out."""
    a = _random_fp32()
    hi, mid, lo = emu.split3(a)
    for part in (hi, mid, lo):
        assert np.all((part.view(np.uint32) & np.uint32(0xFFFF)) == 0)
    a64 = a.astype(np.float64)
    rem = np.abs(a64 - hi.astype(np.float64) - mid.astype(np.float64) - lo.astype(np.float64))
    fin = np.isfinite(hi) & np.isfinite(mid) & np.isfinite(lo)
    assert fin[np.abs(a64) < 3.38e38].all()
    big = (np.abs(a64) >= 2.0 ** -100) & fin
    small = (np.abs(a64) < 2.0 ** -100) & (a64 != 0.0)
    rel = rem[big] / np.abs(a64[big])
    print(f"three-way split: max |a - hi - mid - lo| / |a| = {rel.max():.3e} over {int(big.sum())} values >= 2^-100; "
          f"below that ({int(small.sum())} values) the absolute remainder is at most {rem[small].max():.3e}")
    assert rel.max() <= 2.0 ** -27
    assert rem[small].max() <= 2.0 ** -134
    for part in (hi, mid, lo):
        assert np.all(part[a == 0.0] == 0.0)


def test_six_term_product_per_term_bound():
    """|a b - (the kernel's products)| <= 2^-25 |a||b| against float64, the bound the stretch was specified with, on the same values.
    The SIX products it was specified with (hi lo, lo hi, mid mid, hi mid, mid hi, hi hi) miss it: 2^-24.23 (5.09e-8) over
    78 512 pairs -- the bound was derived with |a - hi| <= 2^-9 |a|, but bf16 carries 8 significant bits and round-to-nearest
    leaves 2^-8 |a| at the bottom of a binade, so the dropped mid lo^T + lo mid^T is bounded by 2^-23 |a||b|.  The kernel
    therefore issues EIGHT, those two included
    (near_band_emul.TERMS); only lo lo^T is left out, 2^-32, and the bound holds with room: the six are measured and printed here,
    the eight asserted.  What a LOST term does is asserted too: each of hi lo, lo hi, mid mid left out leaves more than 2^-21."""
    a = _random_fp32()
    b = np.roll(a, 1)
    exact, six, pa, pb = _terms(a, b)
    ok = np.ones(a.size, dtype=bool)
    for v in (a, b):
        ok &= (np.abs(v.astype(np.float64)) >= 2.0 ** -100) & (np.abs(v.astype(np.float64)) < 3.38e38)
    err = np.abs(exact - six)[ok] / np.abs(exact)[ok]
    err6 = np.abs(exact - (six - pa["mid"] * pb["lo"] - pa["lo"] * pb["mid"]))[ok] / np.abs(exact)[ok]
    print(f"products of the split: max relative error of the eight 2^{np.log2(err.max()):.2f} ({err.max():.3e}), of the six without "
          f"mid lo and lo mid 2^{np.log2(err6.max()):.2f} ({err6.max():.3e}), over {int(ok.sum())} pairs")
    assert len(emu.TERMS) == 8
    for x, y in (("hi", "lo"), ("lo", "hi"), ("mid", "mid")):
        e5 = np.abs(exact - (six - pa[x] * pb[y]))[ok] / np.abs(exact)[ok]
        assert e5.max() > 2.0 ** -21, (x, y)
    assert err.max() <= 2.0 ** -25


@pytest.mark.parametrize("nobs,seed,L,far_bits", [(4000, 4000, 600.0, 16)])
def test_emulated_factor_is_the_fp32_factor_to_rounding(monkeypatch, nobs, seed, L, far_bits):
    """3 946 swath observations at L = 600 km, far 16, middle 8, near `all`: the first residual of the factor with the near stretch
    is at most 1.05 x that of the same factor without it, the second at most 2 x; and near `all` alone (no far, no middle) gives
    the all-fp32 emulation's residuals by the same bars at this size (at the headline size `all` does not: kFactorNearBits,
    csrc/dense_tables.hip).  An emulation that loses a term
    differs from the full one by more than the full one differs from the factor without the stretch."""
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
    monkeypatch.setenv(NEAR, "all")
    env, far, mid, near = emu.tables(lat, g)
    nb = far.size
    first = env[:nb]
    po = dense.unit_vectors(lat, lon).T
    S64 = emu.covariance(po, sig, var, g, dtype=np.float64)[:m, :m]
    S32 = emu.covariance(po, sig, var, g, first=first)
    f_fp32 = emu.factor(S32, first)
    f_mid = emu.factor(S32, first, far, mid)
    f_near = emu.factor(S32, first, far, mid, near)
    f_only = emu.factor(S32, first, None, None, near)
    res = {k: emu.refine(f, S64, d) for k, f in (("fp32", f_fp32), ("mid", f_mid), ("near", f_near), ("only", f_only))}
    d_full = float(np.abs(f_only - f_fp32).max())
    d_drop = {v: float(np.abs(emu.factor(S32, first, None, None, near, variant=v) - f_only).max()) for v in ("hi_lo", "lo_hi", "mid_mid")}
    print(f"m = {m}: residuals fp32 {res['fp32']}, far + middle {res['mid']}, + near {res['near']}, near alone {res['only']}; near alone to "
          f"fp32 {d_full:.3e}, a dropped term to the full emulation {d_drop}")
    assert res["near"][0] <= 1.05 * res["mid"][0] and res["near"][1] <= 2.0 * res["mid"][1]
    assert res["only"][0] <= 1.05 * res["fp32"][0] and res["only"][1] <= 2.0 * res["fp32"][1]
    assert all(v > d_full for v in d_drop.values())
