"""The readers of the Cholesky factor that do not refine, and a wide leading dimension, at the C ABI.

``oisat_trsm_rows``, ``oisat_posterior_error``, ``oisat_gain_diag`` and ``oisat_potrs`` against float64 references evaluated ON
THE FP32 FACTOR DOWNLOADED FROM THE DEVICE (tests/readers_cases.py), so the factorization's own error is out of the picture.
All comparisons are max-norm, relative to the reference's largest entry; the bar is 4 x e32, e32 being the distance of a plain
float32 evaluation of the same operation on the CPU, computed in the test.  tests/test_readers_cases_cpu.py shows that the
library's scheme stays within 2 x e32 and that a sweep which leaves out one block of the factor is at least 50 x e32 off, 13
times the bar.  Then every entry point that takes ``ld`` or ``ldx`` with a leading dimension wider than the matrix: the same bits, and
the gutter untouched.

Measured on an MI355X (x e32; see profiles/EXPERIMENTS.md, "Readers of the factor"): in the docstrings below."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import mid_band_emul as emu
import readers_cases as rc
from oisatgmi import _hip

pytestmark = pytest.mark.gpu
NB = rc.NB
EINVAL = -1
POISON = 0x55
F32_POISON = np.frombuffer(bytes([POISON] * 4), dtype=np.float32)[0]
F64_POISON = np.frombuffer(bytes([POISON] * 8), dtype=np.float64)[0]
FAR, MID, DAG = "OISAT_FACTOR_FAR_BITS", "OISAT_FACTOR_MID_BITS", "OISAT_DAG"
BAR = 4.0


@contextlib.contextmanager
def _environ(**kw):
    """The library reads its switches at every call: set (None: unset) for the block, restored behind it."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _hip.context()
    assert "gfx950" in c.device_info()["name"]
    yield c
    c.check(c.lib.oisat_set_correlation(c.h, 0))
    _dev.clear()


_dev = {}


class Dev:
    """A case's observations on a handle."""

    def __init__(self, cx, c):
        self.c = c
        self.oxyz, self.osig, self.ovar, self.olat = cx.upload(c.oxyz), cx.upload(c.osig), cx.upload(c.ovar), cx.upload(c.lat)
        self.envs = {}
        self.cx = cx

    def env(self, model="gaussian"):
        if model not in self.envs:
            e = rc.envelope(self.c, model)
            self.envs[model] = (e, e[:self.c.nb].copy(), self.cx.upload(e))
        return self.envs[model]


def dev(ctx, name):
    if name not in _dev:
        _dev[name] = Dev(ctx, rc.case(name))
    return _dev[name]


def grid_dev(ctx):
    if "grid" not in _dev:
        gr = rc.grid()
        _dev["grid"] = (ctx.upload(gr.gxyz), ctx.upload(gr.gsig))
    return _dev["grid"]


class Fac:
    """A buffer of mp rows of ld = mp + W floats, poisoned, and a factorization of a case in it on the context's handle.
    how: "potrf" (oisat_cov_build + oisat_potrf, the default schedule), "rec" / "dag" (the same under OISAT_DAG=0 / 1),
    "env" (oisat_cov_build_env + oisat_potrf_env; far / mid = the tables handed to it), "env_fwd"
    (oisat_cov_build_env_zeroed without a claim + oisat_potrf_env_fwd of ``d``)."""

    def __init__(self, ctx, name, how, W=0, model="gaussian", d=None, far=None, mid=None, env=None):
        self.ctx, self.dv, self.c = ctx, dev(ctx, name), rc.case(name)
        self.how, self.model, self.d, self.far, self.mid = how, model, d, far, mid
        self.ld = self.c.mp + W
        self.S = ctx.alloc(self.c.mp * self.ld * 4)
        if env is not None:
            self.envt = (env, env[:self.c.nb].copy(), ctx.upload(env))
        else:
            self.envt = self.dv.env(model) if how in ("env", "env_fwd") else None
        self.first = self.envt[1] if self.envt else np.zeros(self.c.nb, dtype=np.int32)
        self.refactor()

    def refactor(self):
        """Build and factor (again): the handle knows ONE factor.  Same bits every time."""
        ctx, lib, c, dv, S, ld = self.ctx, self.ctx.lib, self.c, self.dv, self.S, self.ld
        ctx.check(lib.oisat_set_correlation(ctx.h, rc.KINDS[self.model]))
        ctx.check(lib.oisat_memset(ctx.h, S.ptr, POISON, c.mp * ld * 4))
        info, sched = C.c_int(-1), C.c_int(-1)
        if self.how in ("potrf", "rec", "dag"):
            with _environ(**{DAG: {"potrf": None, "rec": "0", "dag": "1"}[self.how]}):
                ctx.check(lib.oisat_cov_build(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, c.m, c.g, S.ptr, ld))
                ctx.check(lib.oisat_potrf(ctx.h, S.ptr, c.m, ld, C.byref(info)))
        elif self.how == "env":
            _, first, env_dev = self.envt
            ctx.check(lib.oisat_cov_build_env(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, c.m, c.g, S.ptr, ld, env_dev.ptr))
            if self.far is not None:
                ctx.check(lib.oisat_set_factor_far(ctx.h, self.far.ctypes.data, self.far.size))
            if self.mid is not None:
                ctx.check(lib.oisat_set_factor_mid(ctx.h, self.mid.ctypes.data, self.mid.size))
            ctx.check(lib.oisat_potrf_env(ctx.h, S.ptr, c.m, ld, first.ctypes.data, env_dev.ptr, C.byref(info)))
        else:
            _, first, env_dev = self.envt
            built = C.c_int(-1)
            ctx.check(lib.oisat_cov_build_env_zeroed(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, c.m, c.g, S.ptr, ld, first.ctypes.data,
                                                     env_dev.ptr, None, None, C.byref(built)))
            ctx.check(lib.oisat_potrf_env_fwd(ctx.h, S.ptr, c.m, ld, first.ctypes.data, env_dev.ptr, self.d.ptr, C.byref(info), C.byref(sched)))
            assert built.value == 1 and sched.value == 2              # OISAT_SCHEDULE_ENV_DAG_FWD: the sweep rode in the launch
        assert info.value == 0

    def download(self):
        """The whole buffer, gutter included; the gutter must still hold the poison."""
        full = self.ctx.download(self.S.ptr, (self.c.mp, self.ld), np.float32)
        assert (full[:, self.c.mp:].view(np.uint32) == F32_POISON.view(np.uint32)).all(), "the gutter [mp, ld) was written"
        return full

    def lower32(self):
        return np.tril(self.download()[:, :self.c.mp])


# ---- the readers, each on an arbitrary (factor pointer, m, ld) ----------------------------------------------------------------
def rows_for(ctx, c, nrows, seed=5):
    """``oisat_probe_fill`` rows; rows 1, 2, 3 hold a single 1: first column, last live column, first padding column."""
    X = ctx.alloc(nrows * c.mp * 4)
    ctx.check(ctx.lib.oisat_probe_fill(ctx.h, seed, 0, X.ptr, nrows, c.mp, c.m))
    x0 = ctx.download(X.ptr, (nrows, c.mp), np.float32)
    assert set(np.unique(x0[:, :c.m])) == {-1.0, 1.0} and not x0[:, c.m:].any()
    for r, col in ((1, 0), (2, c.m - 1), (3, c.m)):
        x0[r] = 0.0
        x0[r, col] = 1.0
    return x0


def sweep(ctx, S_ptr, c, ld, x0, ldx=None, bwd=False):
    """oisat_trsm_rows / _bwd of the rows x0 held with leading dimension ldx in a poisoned buffer; the gutter stays poison."""
    nrows = x0.shape[0]
    ldx = c.mp if ldx is None else ldx
    host = np.full((nrows, ldx), F32_POISON, dtype=np.float32)
    host[:, :c.mp] = x0
    X = ctx.upload(host)
    fn = ctx.lib.oisat_trsm_rows_bwd if bwd else ctx.lib.oisat_trsm_rows
    ctx.check(fn(ctx.h, S_ptr, c.m, ld, X.ptr, nrows, ldx))
    got = ctx.download(X.ptr, (nrows, ldx), np.float32)
    assert (got[:, c.mp:].view(np.uint32) == F32_POISON.view(np.uint32)).all(), "the gutter of X was written"
    return got[:, :c.mp].copy()


def post_err(ctx, S_ptr, c, ld, dv, i0, i1, chunk):
    """oisat_posterior_error into a float[i1 - i0] with 64 poisoned floats on either side, which must stay as they are."""
    gr = rc.grid()
    gxyz, gsig = grid_dev(ctx)
    k = i1 - i0
    buf = ctx.alloc((k + 128) * 4)
    ctx.check(ctx.lib.oisat_memset(ctx.h, buf.ptr, POISON, (k + 128) * 4))
    ctx.check(ctx.lib.oisat_posterior_error(ctx.h, S_ptr, c.m, ld, gxyz.ptr, gsig.ptr, gr.n, i0, i1, dv.oxyz.ptr, dv.osig.ptr, c.g, chunk,
                                            buf.at(256)))
    out = ctx.download(buf.ptr, (k + 128,), np.float32)
    assert (out[:64].view(np.uint32) == F32_POISON.view(np.uint32)).all() and (out[64 + k:].view(np.uint32) == F32_POISON.view(np.uint32)).all()
    assert np.isfinite(out[64:64 + k]).all()
    return out[64:64 + k].copy()


def gain_diag(ctx, S_ptr, c, ld, dv, chunk):
    """oisat_gain_diag into a double[m] with a poisoned tail of 64."""
    buf = ctx.alloc((c.m + 64) * 8)
    ctx.check(ctx.lib.oisat_memset(ctx.h, buf.ptr, POISON, (c.m + 64) * 8))
    ctx.check(ctx.lib.oisat_gain_diag(ctx.h, S_ptr, c.m, ld, dv.ovar.ptr, chunk, buf.ptr))
    out = ctx.download(buf.ptr, (c.m + 64,), np.float64)
    assert (out[c.m:].view(np.uint64) == F64_POISON.view(np.uint64)).all(), "ak_out[m:] was written"
    return out[:c.m].copy()


def potrs(ctx, S_ptr, c, ld, z):
    zb = ctx.upload(z)
    ctx.check(ctx.lib.oisat_potrs(ctx.h, S_ptr, c.m, ld, zb.ptr))
    return ctx.download(zb.ptr, (c.m,), np.float64)


def gain_solve(ctx, S_ptr, c, ld, dv, d_buf, refine=2):
    zb = ctx.alloc(c.m * 8)
    ctx.check(ctx.lib.oisat_memset(ctx.h, zb.ptr, POISON, c.m * 8))
    ctx.check(ctx.lib.oisat_gain_solve(ctx.h, S_ptr, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, c.m, ld, c.g, d_buf.ptr, refine, zb.ptr, None,
                                       dv.olat.ptr))
    return ctx.download(zb.ptr, (c.m,), np.float64)


def rhs(c, seed=1):
    return np.random.default_rng(seed).standard_normal(c.m)


# ---- 1. oisat_trsm_rows ----------------------------------------------------------------------------------------------------------
def _check_rows(ctx, S_ptr, c, ld, L32, nrows, what):
    x0 = rows_for(ctx, c, nrows)
    got = sweep(ctx, S_ptr, c, ld, x0)
    ref = rc.xlt_ref(L32.astype(np.float64), x0)
    e32 = rc.rel_err(rc.xlt_f32(L32, x0), ref)
    e = rc.rel_err(got, ref)
    print(f"trsm_rows {what}, {nrows} rows: error {e:.3e}, e32 {e32:.3e}, ratio {e / e32:.2f} (bar {BAR:g})")
    assert np.isfinite(got).all() and e <= BAR * e32
    assert np.array_equal(got[:, c.m:].view(np.uint32), x0[:, c.m:].view(np.uint32))     # padding columns pass through unchanged
    assert got[3, c.m] == 1.0 and not got[3, :c.m].any()          # ... and the row that lives there touches nothing else
    return x0, got, ref, e32


@pytest.mark.parametrize("nrows", [128, 384])
@pytest.mark.parametrize("name,how", [("A", "potrf"), ("B", "env"), ("C", "potrf")])
def test_trsm_rows_against_float64_on_the_downloaded_factor(ctx, name, how, nrows):
    """Measured (error / e32) at 128 / 384 rows: A 1.08 / 1.03, B 1.39 / 1.39, C 1.33 / 1.33; B's enveloped result against the
    dense factor's reference and the dense result against the enveloped factor's reference 1.39 both."""
    f = Fac(ctx, name, how)
    c = f.c
    if name == "B":
        assert (f.first > 0).any(), f.first
    L32 = f.lower32()
    x0, got, ref, e32 = _check_rows(ctx, f.S.ptr, c, f.ld, L32, nrows, f"case {name} ({how})")
    if name == "B":
        # the same rows on a dense factor of the same matrix: the enveloped read finds the build's zeros
        fd = Fac(ctx, name, "potrf")
        Ld = fd.lower32()
        for i in range(c.nb):
            assert not L32[i * NB:(i + 1) * NB, :int(f.first[i]) * NB].any()
        gd = sweep(ctx, fd.S.ptr, c, fd.ld, x0)
        refd = rc.xlt_ref(Ld.astype(np.float64), x0)
        e32d = rc.rel_err(rc.xlt_f32(Ld, x0), refd)
        a, b = rc.rel_err(got, refd), rc.rel_err(gd, ref)
        print(f"   enveloped result vs dense reference {a / e32d:.2f} x e32, dense result vs enveloped reference {b / e32:.2f} x e32")
        assert a <= BAR * e32d and b <= BAR * e32


# ---- 2. oisat_posterior_error ---------------------------------------------------------------------------------------------------
_q_cache = {}


def _q_yardstick(name, model, L32):
    """q_ref and the plain float32 q on all n cells for this downloaded factor (computed once per factor)."""
    key = (name, model, hash(L32.tobytes()))
    if key not in _q_cache:
        c, gr = rc.case(name), rc.grid()
        q = rc.q_ref(L32.astype(np.float64), rc.cross_rows64(c, gr, 0, gr.n, model))
        q32 = rc.sumsq64(rc.xlt_f32(L32, rc.cross_rows32(c, gr, 0, gr.n, model)))
        assert (q < (1.0 - 1e-4) * gr.gsig ** 2).all()              # the clamp is never in play
        _q_cache[key] = (q, q32)
    return _q_cache[key]


def _check_post_err(ctx, f, i0, i1, chunk, what):
    """q = sig^2 - err^2 against q_ref; bar 4 e32 max(q_ref) + 2^-22 sig_i^2 (the float32 rounding of err: a relative 2^-24
    of err is 2^-23 of err^2 <= sig^2, and as much again for the rounding of the square root's argument and result).  e32 and
    max(q_ref) are taken over the tested cells; a range shorter than the 128 rows the kernel sweeps at the least has no
    sample to take a max-norm from, and takes both over all n cells."""
    c, gr = f.c, rc.grid()
    q_all, q32_all = _q_yardstick(c.name, f.model, f.lower32())
    err = post_err(ctx, f.S.ptr, c, f.ld, f.dv, i0, i1, chunk).astype(np.float64)
    sel = slice(i0, i1) if i1 - i0 >= NB else slice(0, gr.n)
    qmax = q_all[sel].max()
    e32 = np.abs(q32_all[sel] - q_all[sel]).max() / qmax
    sig2 = gr.gsig[i0:i1] ** 2
    diff = np.abs((sig2 - err ** 2) - q_all[i0:i1])
    ratio = (np.maximum(diff - 2.0 ** -22 * sig2, 0.0)).max() / (e32 * qmax)
    print(f"posterior_error {what} [{i0}, {i1}) chunk {chunk}: max |q - q_ref| / max q_ref = {diff.max() / qmax:.3e}, e32 {e32:.3e}, "
          f"(error - 2^-22 sig^2) / (e32 max q_ref) = {ratio:.2f} (bar {BAR:g})")
    assert (diff <= BAR * e32 * qmax + 2.0 ** -22 * sig2).all()


@pytest.mark.parametrize("i0,i1,chunk", rc.ERR_RANGES)
@pytest.mark.parametrize("name,how", [("A", "potrf"), ("B", "env")])
def test_posterior_error_ranges_and_chunks(ctx, name, how, i0, i1, chunk):
    """Measured ((error - 2^-22 sig^2) / (e32 max q_ref)), in the order of readers_cases.ERR_RANGES: A 0.56, 0.56, 0.99, 0.56,
    0.00, 0.00; B 0.64, 0.64, 0.00, 0.64, 0.00, 0.00 (max |q - q_ref| / max q_ref itself: 0.79 .. 1.68 x e32 on the ranges of 128
    cells and more)."""
    _check_post_err(ctx, Fac(ctx, name, how), i0, i1, chunk, f"case {name} ({how})")


@pytest.mark.parametrize("name,how,model,i0,i1,chunk", [("A", "potrf", "gaspari_cohn", 1000, 1300, 100), ("B", "env", "gaspari_cohn", 5, 133, 128),
                                                        ("A", "potrf", "soar", 5, 133, 128), ("B", "env", "soar", 1000, 1300, 100)])
def test_posterior_error_under_the_other_correlation_models(ctx, name, how, model, i0, i1, chunk):
    """Built, factored and read under that model.  Measured: Gaspari-Cohn A 0.34, B 0.00; SOAR A 0.39, B 0.72."""
    try:
        _check_post_err(ctx, Fac(ctx, name, how, model=model), i0, i1, chunk, f"case {name} ({how}, {model})")
    finally:
        ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))


# ---- 3. oisat_gain_diag ---------------------------------------------------------------------------------------------------------
def _check_gain_diag(ctx, S_ptr, c, ld, dv, L32, chunk, what):
    """(1 - ak_a) / ovar_a against (S^-1)_aa; the second term of the bar is the float64 rounding of ak = 1 - R s itself."""
    ak = gain_diag(ctx, S_ptr, c, ld, dv, chunk)
    ref = rc.sinv_diag_ref(L32.astype(np.float64), c)
    e32 = rc.rel_err(rc.sumsq64(rc.xlt_f32(L32, rc.identity_rows(c, dtype=np.float32))), ref)
    diff = np.abs((1.0 - ak) / c.ovar - ref)
    print(f"gain_diag {what} chunk {chunk}: error {diff.max() / ref.max():.3e}, e32 {e32:.3e}, ratio {diff.max() / ref.max() / e32:.2f} (bar {BAR:g})")
    assert (diff <= BAR * e32 * ref.max() + 2.0 ** -52 / c.ovar).all()


@pytest.mark.parametrize("chunk", [0, 128, 200])
@pytest.mark.parametrize("name,how", [("A", "potrf"), ("B", "env")])
def test_gain_diag_chunks(ctx, name, how, chunk):
    """chunk_rows 128 and 200 (rounded up to 256) put a0 > 0 on a correlated S.  Measured: A 1.72, B 3.64 x e32, the same bits at
    every chunk size.  (With correctly rounded inverted blocks the scheme gives 0.63 and 1.00, tests/test_readers_cases_cpu.py:
    the distance is the inverted blocks' own error, see test_potrs_against_the_float64_two_sweep.)"""
    f = Fac(ctx, name, how)
    _check_gain_diag(ctx, f.S.ptr, f.c, f.ld, f.dv, f.lower32(), chunk, f"case {name} ({how})")


# ---- 4. oisat_potrs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how", [("A", "potrf"), ("B", "env")])
def test_potrs_against_the_float64_two_sweep(ctx, name, how):
    """oisat_potrs corrects once against the factor itself and sits far below the fp32 two-sweep's e32.  Measured: A 6.2e-6, B 1.5e-6
    x e32 (errors 4.0e-12 and 1.1e-13).  (A single pass of the sweeps does not: it multiplies by the inverted diagonal blocks T_b, which are float32 and lie
    1.2 .. 2.6 (A: 1.1 .. 4.4) x 2^-24 of their largest entry from the exact inverses, and measured 0.42 (A) and 4.40 (B) x e32 --
    B beyond this bar -- before oisat_potrs had the correction; test_adopted_batch_members restates both passes.)"""
    f = Fac(ctx, name, how)
    L32, z = f.lower32(), rhs(f.c)
    got = potrs(ctx, f.S.ptr, f.c, f.ld, z)
    ref = rc.potrs_ref(L32.astype(np.float64), z)
    e32 = rc.rel_err(rc.potrs_f32(L32, z), ref)
    e = rc.rel_err(got, ref)
    print(f"potrs case {name} ({how}): error {e:.3e}, e32 {e32:.3e}, ratio {e / e32:.2g} (bar {BAR:g})")
    assert e <= BAR * e32


# ---- 5. an adopted factor ---------------------------------------------------------------------------------------------------------
class Batch:
    """Cases A and B factored by ``oisat_batch_potrf`` on a second handle with caller-owned inverted blocks, leading
    dimensions ``lds``; ``adopt(i)`` hands member i to the test's handle behind ``oisat_wait_for``."""

    def __init__(self, ctx, lds):
        self.ctx, lib = ctx, ctx.lib
        self.c2 = c2 = _hip.Context(ctx.device).own_stream()
        self.cases = [rc.case("A"), rc.case("B")]
        self.lds = lds
        self.devs = [Dev(c2, c) for c in self.cases]
        self.S = [c2.alloc(c.mp * ld * 4).shared_with_other_streams() for c, ld in zip(self.cases, lds)]
        self.T = [c2.alloc(c.mp * NB * 4).shared_with_other_streams() for c in self.cases]
        for c, dv, S, ld in zip(self.cases, self.devs, self.S, lds):
            c2.check(lib.oisat_memset(c2.h, S.ptr, POISON, c.mp * ld * 4))
            c2.check(lib.oisat_cov_build(c2.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, c.m, c.g, S.ptr, ld))
        bid = C.c_int(-1)
        c2.check(lib.oisat_batch_create(c2.h, 2, (C.c_void_p * 2)(*[s.ptr for s in self.S]), (C.c_int64 * 2)(*[c.m for c in self.cases]),
                                        (C.c_int64 * 2)(*lds), (C.c_void_p * 2)(*[t.ptr for t in self.T]), C.byref(bid)))
        self.bid = bid.value
        info2 = (C.c_int * 2)(-1, -1)
        c2.check(lib.oisat_batch_potrf(c2.h, self.bid, info2))
        assert list(info2) == [0, -1]
        ctx.wait_for(c2)

    def adopt(self, i):
        c = self.cases[i]
        self.ctx.check(self.ctx.lib.oisat_factor_adopt(self.ctx.h, self.S[i].ptr, c.m, self.lds[i], self.T[i].ptr))

    def lower32(self, i):
        c = self.cases[i]
        full = self.ctx.download(self.S[i].ptr, (c.mp, self.lds[i]), np.float32)
        assert (full[:, c.mp:].view(np.uint32) == F32_POISON.view(np.uint32)).all(), "the gutter [mp, ld) was written"
        return np.tril(full[:, :c.mp])

    def close(self):
        self.ctx.sync()
        self.c2.check(self.ctx.lib.oisat_batch_destroy(self.c2.h, self.bid))
        for b in self.S + self.T:
            b.free()
        for dv in self.devs:
            for b in (dv.oxyz, dv.osig, dv.ovar, dv.olat):
                b.free()
        self.c2.close()


def test_adopted_batch_members(ctx):
    """Items 1 and 3 on each member of a batch of (385, 700) adopted by the test's handle, and oisat_potrs against its float64
    restatement through the batch's own inverted blocks.  Measured: trsm_rows 1.08 (A), 1.39 (B); gain_diag 1.72 (A), 3.64 (B)
    x e32 -- the figures of oisat_potrf's and oisat_potrf_env's factors."""
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    bt = Batch(ctx, [rc.case("A").mp, rc.case("B").mp])
    try:
        for i, c in enumerate(bt.cases):
            bt.adopt(i)
            L32 = bt.lower32(i)
            _check_rows(ctx, bt.S[i].ptr, c, bt.lds[i], L32, 128, f"adopted member {c.name}")
            _check_gain_diag(ctx, bt.S[i].ptr, c, bt.lds[i], dev(ctx, c.name), L32, 128, f"adopted member {c.name}")
            _check_potrs_through_the_inverted_blocks(ctx, bt.S[i].ptr, c, bt.lds[i], L32, ctx.download(bt.T[i].ptr, (c.nb, NB, NB), np.float32))
    finally:
        bt.close()


def _check_potrs_through_the_inverted_blocks(ctx, S_ptr, c, ld, L32, T):
    """With caller-owned inverted blocks ``oisat_potrs`` can be restated exactly (readers_cases.potrs_emul_f64): a float64
    two-sweep through THE DEVICE'S T_b, the residual against L L^T, a second two-sweep added.  Bar: the forward error of
    substitutions of mp terms in float64, mp 2^-53 cond_2(L L^T), three orders of magnitude below e32.  Printed beside it: what
    a single pass gives (x e32) through the device's T_b and through correctly rounded inverses, and the distance of the
    device's T_b from the exact inverses in units of 2^-24 of the inverse's largest entry."""
    z = rhs(c)
    got = potrs(ctx, S_ptr, c, ld, z)
    Lh = L32.astype(np.float64)
    bar = c.mp * 2.0 ** -53 * np.linalg.cond(Lh) ** 2
    e = rc.rel_err(got, rc.potrs_emul_f64(L32, T, z))
    ref = rc.potrs_ref(Lh, z)
    e32 = rc.rel_err(rc.potrs_f32(L32, z), ref)
    ideal = np.stack(rc.inverted_diagonal_blocks(L32))
    ulps = [float(np.abs(T[b].astype(np.float64) - np.linalg.inv(Lh[b * NB:(b + 1) * NB, b * NB:(b + 1) * NB])).max() /
                  np.abs(ideal[b]).max() * 2.0 ** 24) for b in range(c.nb)]
    print(f"potrs adopted member {c.name}: {e:.2e} from its float64 restatement through the device's T (bar {bar:.1e}), "
          f"{rc.rel_err(got, ref) / e32:.2g} x e32 from the reference on the factor; a single pass: {rc.rel_err(rc.two_sweep_f64(L32, T, z), ref) / e32:.2f} "
          f"x e32 with the device's T, {rc.rel_err(rc.two_sweep_f64(L32, ideal, z), ref) / e32:.2f} x e32 with the correctly rounded inverse; "
          f"max |T - L_bb^-1| per block = " + ", ".join(f"{u:.1f}" for u in ulps) + " x 2^-24 of max |L_bb^-1|")
    assert not np.triu(T, 1).any()                              # the sweeps multiply by the whole tile
    assert e <= bar and rc.rel_err(got, ref) <= BAR * e32


# ---- 6. a leading dimension wider than the matrix --------------------------------------------------------------------------------
def _reader_bits(ctx, S_ptr, c, ld, dv, W, d_buf, d_host):
    """Every reader once, X with ldx = mp + W.  The gain solve goes first: behind oisat_potrf_env_fwd it takes the forward
    vector the launch left, once."""
    out = {"gain_solve": gain_solve(ctx, S_ptr, c, ld, dv, d_buf, refine=2), "potrs": potrs(ctx, S_ptr, c, ld, d_host)}
    x0 = rows_for(ctx, c, 128)
    out["trsm_rows"] = sweep(ctx, S_ptr, c, ld, x0, ldx=c.mp + W)
    out["trsm_rows_bwd"] = sweep(ctx, S_ptr, c, ld, x0, ldx=c.mp + W, bwd=True)
    out["posterior_error"] = post_err(ctx, S_ptr, c, ld, dv, 1000, 1300, 100)
    out["gain_diag"] = gain_diag(ctx, S_ptr, c, ld, dv, 128)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


def _same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs between ld = mp and ld = mp + W"


def _forced_tables(name):
    """The factor's envelope and its far / middle tables with the stretches forced at 2^-16 / 2^-8, as tests/test_gpu_mid_band.py
    forces them."""
    c = rc.case(name)
    with _environ(**{FAR: 16, MID: 8}):
        env, far, mid = emu.tables(c.lat, c.g)
    return env, far, mid, emu.mid_share(env[:c.nb], far, mid)


SCHEDULES = ["A-rec", "A-dag", "B-env_fwd", "B-forced", "B600-forced"]
_narrow = {}


def _run_schedule(ctx, sched, W):
    name, how = sched.split("-")
    c = rc.case(name)
    d_host = rhs(c, 7)
    d_buf = ctx.upload(d_host)
    kw = {}
    if how == "forced":
        env, far, mid, share = _forced_tables(name)
        if name == "B600":
            assert share[0] > 0 and share[1] > 0, share            # K-blocks in both stretches
        else:
            assert share == (0, 0, 0)                               # (B's tiles have no K-loop: nothing to force, see readers_cases.CASES)
        kw = dict(env=env, far=far, mid=mid)
        how = "env"
    f = Fac(ctx, name, how, W=W, d=d_buf, **kw)
    if sched == "B600-forced":                                     # the shadow was made: the stretches read the images, not S
        r = int(np.argmax(np.arange(c.nb) - f.first >= 2))
        hi, lo = np.empty((NB, NB), dtype=np.uint16), np.empty((NB, NB), dtype=np.uint16)
        ctx.check(ctx.lib.oisat_factor_shadow_tile(ctx.h, r, int(f.first[r]), hi.ctypes.data, lo.ctypes.data))
    low = f.lower32()                                               # (checks the gutter)
    bits = _reader_bits(ctx, f.S.ptr, c, f.ld, f.dv, W, d_buf, d_host)
    f.download()                                                    # ... and again behind every reader
    bits["factor"] = low
    return bits


@pytest.mark.parametrize("W", [4, "mp"])
@pytest.mark.parametrize("sched", SCHEDULES)
def test_wide_leading_dimension_same_bits_and_gutter_untouched(ctx, sched, W):
    """ld = mp + 4 (the smallest legal width: no 32-, 64- or 128-float pitch survives it) and ld = 2 mp (a matrix embedded in a
    larger array): the lower triangle, z of oisat_gain_solve (refine = 2) and oisat_potrs, both row sweeps with ldx = ld, the
    posterior error and the gain diagonal have the bits of the ld = mp run of the same schedule; the gutters of S and X keep
    their poison."""
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    c = rc.case(sched.split("-")[0])
    if sched not in _narrow:
        _narrow[sched] = _run_schedule(ctx, sched, 0)
    _same_bits(_narrow[sched], _run_schedule(ctx, sched, c.mp if W == "mp" else W), sched)


@pytest.mark.parametrize("W", [4, "mp"])
def test_wide_leading_dimension_in_a_batch(ctx, W):
    """The batch of item 5 with member A wide and member B not: both members' factors and, once adopted, their readers have
    the bits of the batch with ld = mp throughout."""
    ctx.check(ctx.lib.oisat_set_correlation(ctx.h, 0))
    a, b = rc.case("A"), rc.case("B")
    res = []
    for lds in ([a.mp, b.mp], [a.mp + (a.mp if W == "mp" else W), b.mp]):
        bt = Batch(ctx, lds)
        try:
            per = []
            for i, c in enumerate(bt.cases):
                d_host = rhs(c, 7)
                d_buf = ctx.upload(d_host)
                bt.adopt(i)
                bits = _reader_bits(ctx, bt.S[i].ptr, c, lds[i], dev(ctx, c.name), lds[i] - c.mp, d_buf, d_host)
                bits["factor"] = bt.lower32(i)
                per.append(bits)
            res.append(per)
        finally:
            bt.close()
    for i in range(2):
        _same_bits(res[0][i], res[1][i], f"batch member {i}")


# ---- 7. argument checks -----------------------------------------------------------------------------------------------------------
def test_bad_leading_dimensions_and_ranges_are_refused_and_write_nothing(ctx):
    lib = ctx.lib
    ctx.check(lib.oisat_set_correlation(ctx.h, 0))
    c, dv = rc.case("B"), dev(ctx, "B")
    m, mp = c.m, c.mp
    env, first, env_dev = dv.env()
    # -- the build, the factorizations, the batch and the adoption: ld < mp, ld % 4 != 0, a base 4 bytes off
    S = ctx.alloc(mp * (mp + 8) * 4)
    T = ctx.alloc(mp * NB * 4)
    ctx.check(lib.oisat_memset(ctx.h, S.ptr, POISON, mp * (mp + 8) * 4))
    ctx.check(lib.oisat_memset(ctx.h, T.ptr, POISON, mp * NB * 4))
    info, d_buf = C.c_int(-7), ctx.upload(rhs(c))
    for ptr, ld in ((S.ptr, mp - 4), (S.ptr, mp + 2), (S.ptr, mp + 1), (S.ptr + 4, mp), (S.ptr + 4, mp + 4)):
        assert lib.oisat_cov_build(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, m, c.g, ptr, ld) == EINVAL, (ptr - S.ptr, ld)
        assert lib.oisat_cov_build_env(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, m, c.g, ptr, ld, env_dev.ptr) == EINVAL
        assert lib.oisat_cov_build_env_zeroed(ctx.h, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, m, c.g, ptr, ld, first.ctypes.data, env_dev.ptr,
                                              None, None, None) == EINVAL
        assert lib.oisat_potrf(ctx.h, ptr, m, ld, C.byref(info)) == EINVAL
        assert lib.oisat_potrf_env(ctx.h, ptr, m, ld, first.ctypes.data, env_dev.ptr, C.byref(info)) == EINVAL
        assert lib.oisat_potrf_env_fwd(ctx.h, ptr, m, ld, first.ctypes.data, env_dev.ptr, d_buf.ptr, C.byref(info), None) == EINVAL
        assert lib.oisat_factor_adopt(ctx.h, ptr, m, ld, T.ptr) == EINVAL
        bid = C.c_int(-7)
        assert lib.oisat_batch_create(ctx.h, 1, (C.c_void_p * 1)(ptr), (C.c_int64 * 1)(m), (C.c_int64 * 1)(ld), (C.c_void_p * 1)(T.ptr),
                                      C.byref(bid)) == EINVAL and bid.value == -7
    assert lib.oisat_factor_adopt(ctx.h, S.ptr, m, mp, T.ptr + 4) == EINVAL
    assert info.value == -7
    for buf, count in ((S, mp * (mp + 8)), (T, mp * NB)):
        assert (ctx.download(buf.ptr, (count,), np.uint32) == F32_POISON.view(np.uint32)).all()
    # -- the readers: another ld than the factor's, bad ranges, bad row counts
    f = Fac(ctx, "B", "env")
    gr = rc.grid()
    gxyz, gsig = grid_dev(ctx)
    nrows = 128
    x0 = np.full((nrows, mp + 4), F32_POISON, dtype=np.float32)
    X = ctx.upload(x0)
    out = ctx.alloc(4096 * 8)
    ctx.check(lib.oisat_memset(ctx.h, out.ptr, POISON, 4096 * 8))
    Sp = f.S.ptr
    for ld in (mp + 4, mp - 4, 2 * mp):
        assert lib.oisat_potrs(ctx.h, Sp, m, ld, out.ptr) == EINVAL
        assert lib.oisat_gain_solve(ctx.h, Sp, dv.oxyz.ptr, dv.osig.ptr, dv.ovar.ptr, m, ld, c.g, d_buf.ptr, 2, out.ptr, None, None) == EINVAL
        assert lib.oisat_trsm_rows(ctx.h, Sp, m, ld, X.ptr, nrows, mp + 4) == EINVAL
        assert lib.oisat_trsm_rows_bwd(ctx.h, Sp, m, ld, X.ptr, nrows, mp + 4) == EINVAL
        assert lib.oisat_posterior_error(ctx.h, Sp, m, ld, gxyz.ptr, gsig.ptr, gr.n, 0, 128, dv.oxyz.ptr, dv.osig.ptr, c.g, 128, out.ptr) == EINVAL
        assert lib.oisat_gain_diag(ctx.h, Sp, m, ld, dv.ovar.ptr, 128, out.ptr) == EINVAL
    for i0, i1 in ((5, 5), (6, 5), (-1, 5), (0, gr.n + 1), (gr.n, gr.n + 1)):
        assert lib.oisat_posterior_error(ctx.h, Sp, m, mp, gxyz.ptr, gsig.ptr, gr.n, i0, i1, dv.oxyz.ptr, dv.osig.ptr, c.g, 128,
                                         out.ptr) == EINVAL, (i0, i1)
    for fn in (lib.oisat_trsm_rows, lib.oisat_trsm_rows_bwd):
        for rows, ldx, xp in ((100, mp + 4, X.ptr), (0, mp + 4, X.ptr), (nrows, mp - 4, X.ptr), (nrows, mp + 2, X.ptr), (nrows, mp + 4, X.ptr + 4)):
            assert fn(ctx.h, Sp, m, mp, xp, rows, ldx) == EINVAL, (rows, ldx, xp - X.ptr)
    assert (ctx.download(out.ptr, (4096 * 2,), np.uint32) == F32_POISON.view(np.uint32)).all()
    assert np.array_equal(ctx.download(X.ptr, (nrows, mp + 4), np.float32).view(np.uint32), x0.view(np.uint32))
    # ... and the factor is still the handle's: the legal call goes through
    ctx.check(lib.oisat_gain_diag(ctx.h, Sp, m, mp, dv.ovar.ptr, 128, out.ptr))
