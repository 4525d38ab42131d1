"""Host checks that make the bars of tests/test_gpu_readers_abi.py meaningful: the float64 references of
tests/readers_cases.py against the oracle, the library's blocked scheme against the plain float32 yardstick, and the sharpness
of the 4 x e32 bar -- a sweep that leaves out any one block of the factor lands far beyond it."""
import types

import numpy as np
import pytest

import readers_cases as rc
from oisatgmi import dense, synthetic as syn
from oracle import oi_oracle as orc

NB = rc.NB
BLOCK_FLOOR = 1e-3            # a block counts when its Frobenius norm is at least this fraction of the factor's


def test_references_reproduce_the_oracle_on_an_exact_factor():
    """err and ak_obs of ``oracle.dense_oi(..., want_error=True)`` from q_ref and sinv_diag_ref on the float64 Cholesky factor."""
    L_km = 600.0
    p = syn.point_obs_case(36, 72, 300, 8)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    want = orc.dense_oi(p.lat, p.lon, p.Xa, p.Sa, p.obs_lat, p.obs_lon, cell, p.obs_y, p.obs_var, L_km, want_error=True)
    sig = np.sqrt(p.Sa.ravel().astype(np.float64))
    c = types.SimpleNamespace(m=300, mp=384, nb=3, L_km=L_km, g=dense.decay_constant(L_km), oxyz=dense.unit_vectors(p.obs_lat, p.obs_lon),
                              osig=sig[cell], ovar=np.ravel(p.obs_var).astype(np.float64))
    gr = types.SimpleNamespace(n=sig.size, gxyz=dense.unit_vectors(p.lat, p.lon), gsig=sig)
    Lh = rc.exact_factor64(c)
    assert np.array_equal(Lh[300:, 300:], np.eye(84)) and not Lh[300:, :300].any()
    q = rc.q_ref(Lh, rc.cross_rows64(c, gr, 0, gr.n))
    err = np.sqrt(np.maximum(sig ** 2 - q, 0.0))
    ak = 1.0 - c.ovar * rc.sinv_diag_ref(Lh, c)
    assert np.abs(err - want["err"]).max() <= 1e-10 * np.abs(want["err"]).max()
    assert np.abs(ak - want["ak_obs"]).max() <= 1e-10 * np.abs(want["ak_obs"]).max()
    # a subrange of cells / observations is the same numbers
    assert np.array_equal(rc.q_ref(Lh, rc.cross_rows64(c, gr, 1000, 1300)), q[1000:1300])
    np.testing.assert_allclose(rc.sinv_diag_ref(Lh, c, 128, 300), rc.sinv_diag_ref(Lh, c)[128:], rtol=1e-13)
    # the two-sweep reference solves S x = z
    z = np.random.default_rng(0).standard_normal(300)
    np.testing.assert_allclose(rc.system64(c) @ rc.potrs_ref(Lh, z), z, atol=1e-9 * np.abs(z).max())


def test_float32_correlation_is_the_float64_one_to_float32_rounding():
    c, gr = rc.case("C"), rc.grid()
    for model in rc.KINDS:
        c64 = rc.corr_ref(gr.gxyz[:, 500:700], c.oxyz, c.L_km, model)
        c32 = rc.corr_f32(gr.gxyz[:, 500:700], c.oxyz, c.g, model)
        assert c32.dtype == np.float32
        # the squared chord of float32 coordinates is 2^-23 ABSOLUTE (coordinates of size 1), times |dC / d(d2)| <= g
        assert np.abs(c32 - c64).max() <= 4 * 2.0 ** -23 * max(1.0, c.g * 4.0), model


@pytest.fixture(scope="module")
def work():
    """Per case: the fp32 stand-in factor, the three kinds of rows, their float64 references and e32 (computed once)."""
    out = {}
    gr = rc.grid()
    for name in ("A", "B"):
        c = rc.case(name)
        L32 = rc.fp32_factor(c)
        Lh = L32.astype(np.float64)
        w = types.SimpleNamespace(c=c, L32=L32, Lh=Lh, tinv=rc.inverted_diagonal_blocks(L32))
        w.X = rc.probe_rows(c, 128)
        w.G32 = rc.cross_rows32(c, gr, 0, gr.n)
        w.E = rc.identity_rows(c, dtype=np.float32)
        w.ref = {"probe": rc.xlt_ref(Lh, w.X), "q": rc.q_ref(Lh, rc.cross_rows64(c, gr, 0, gr.n)), "sinv": rc.sinv_diag_ref(Lh, c)}
        w.e32 = {"probe": rc.rel_err(rc.xlt_f32(L32, w.X), w.ref["probe"]),
                 "q": rc.rel_err(rc.sumsq64(rc.xlt_f32(L32, w.G32)), w.ref["q"]),
                 "sinv": rc.rel_err(rc.sumsq64(rc.xlt_f32(L32, w.E)), w.ref["sinv"])}
        out[name] = w
    return out


def _blocked(w, skip=None):
    """The three readers' results through ``blocked_sweep_f32``, as multiples of e32."""
    got = {"probe": rc.blocked_sweep_f32(w.L32, w.X, skip, w.tinv),
           "q": rc.sumsq64(rc.blocked_sweep_f32(w.L32, w.G32, skip, w.tinv)),
           "sinv": rc.sumsq64(rc.blocked_sweep_f32(w.L32, w.E, skip, w.tinv))}
    return {k: rc.rel_err(got[k], w.ref[k]) / w.e32[k] for k in got}


@pytest.mark.parametrize("name", ["A", "B"])
def test_blocked_scheme_stays_within_twice_the_float32_yardstick(work, name):
    w = work[name]
    ratios = _blocked(w)
    print(f"case {name}: e32 = " + ", ".join(f"{k} {v:.2e}" for k, v in w.e32.items()) + "; blocked / e32 = " +
          ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    for k, v in w.e32.items():
        assert 1e-8 < v < 1e-5, (k, v)                  # float32 rounding, neither exact nor broken
    for k, r in ratios.items():
        assert r <= 2.0, (k, r)


def test_case_shapes(work):
    a, b, c = rc.case("A"), rc.case("B"), rc.case("C")
    assert (a.nb, a.mp - a.m) == (4, 127) and b.nb == 6 and c.nb == 1
    first = rc.envelope(b)[:b.nb]
    assert (first > 0).any(), first                     # B: a real envelope
    assert not rc.envelope(a)[:a.nb].any()              # A: none at 3000 km
    for i in range(b.nb):                               # ... outside of which the factor is zero (no fill outside the envelope)
        assert not work["B"].L32[i * NB:(i + 1) * NB, :int(first[i]) * NB].any()
    for name in "ABC":                                  # an fp32 Cholesky of the case exists
        assert np.isfinite(np.linalg.cholesky(rc.system64(rc.case(name)).astype(np.float32))).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_sweep_that_skips_one_block_cannot_pass(work, name):
    """Case A: every strictly-lower block is at least 1e-3 of the factor.  Case B: every block inside the envelope that is.
    Leaving any one of them out of the emulation puts all three readers beyond the 4 x e32 bar of the GPU tests."""
    w = work[name]
    first = rc.envelope(w.c)[:w.c.nb]
    tested = 0
    for b, k, frac in rc.lower_blocks(w.L32):
        if name == "A":
            assert frac >= BLOCK_FLOOR, (b, k, frac)
        elif k < first[b] or frac < BLOCK_FLOOR:
            continue
        ratios = _blocked(w, skip=(b, k))
        print(f"case {name}: without block ({b}, {k}) ({frac:.1e} of the factor): " + ", ".join(f"{q} {r:.3g} x e32" for q, r in ratios.items()))
        for q, r in ratios.items():
            assert r > 4.0, (b, k, q, r)
        tested += 1
    assert tested == (6 if name == "A" else 4)


@pytest.mark.parametrize("name,model", [("A", "gaussian"), ("B", "gaussian"), ("A", "gaspari_cohn"), ("B", "gaspari_cohn"),
                                        ("A", "soar"), ("B", "soar")])
def test_clamp_is_never_in_play_at_the_tested_cells(name, model):
    """q_ref < (1 - 1e-4) sig_i^2 on every cell of the grid (the Gaussian cases run all of them; the other two models one
    subrange each, inside it), so ``v > 0 ? v : 0`` of the error kernel decides nothing in the GPU tests."""
    c, gr = rc.case(name), rc.grid()
    Lh = rc.fp32_factor(c, model).astype(np.float64)
    q = rc.q_ref(Lh, rc.cross_rows64(c, gr, 0, gr.n, model))
    worst = (q / gr.gsig ** 2).max()
    print(f"case {name}, {model}: max q / sig^2 = {worst:.6f}")
    assert worst < 1.0 - 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_one_correction_against_the_factor_removes_the_inverted_blocks_error(work, name):
    """``potrs_emul_f64`` (what oisat_potrs does) against the float64 two-sweep on the factor: a single pass through float32
    inverted blocks is a float32 result, the corrected one carries that error squared."""
    w = work[name]
    z = np.random.default_rng(1).standard_normal(w.c.m)
    ref = rc.potrs_ref(w.Lh, z)
    e32 = rc.rel_err(rc.potrs_f32(w.L32, z), ref)
    one = rc.rel_err(rc.two_sweep_f64(w.L32, np.stack(w.tinv), z), ref)
    two = rc.rel_err(rc.potrs_emul_f64(w.L32, np.stack(w.tinv), z), ref)
    print(f"case {name}: single pass {one / e32:.2f} x e32, corrected {two / e32:.2g} x e32 (e32 {e32:.2e})")
    assert 1e-9 < one < 1e-5 and two <= 1e-3 * e32
