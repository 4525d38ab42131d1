"""NumPy emulation of the enveloped task-graph factorization with a far, a middle AND a near stretch, shared by
tests/test_near_band_cpu.py and tests/test_gpu_near_band.py: tests/mid_band_emul.py's blocked left-looking Cholesky (fp32 tiles,
fp32 accumulation, diagonal blocks in float64) in which the K-blocks kmid <= k < knear of a tile of block row i are three-way
split bf16 products.  Beside every final fp32 tile L it keeps hi = bf16_round(L), mid = bf16_round(L - hi) and
lo = bf16_round(L - hi - mid) -- the kernel's roundings: nearest even, by integer arithmetic on the float32 bits
(far_band_emul.bf16_round); both differences are exact in float32 -- and a near K-block adds, in the kernel's order,
mid lo^T, lo mid^T, hi lo^T, lo hi^T, mid mid^T, hi mid^T, mid hi^T, hi hi^T.  knear = near[i] clamped into [kmid, kend] as the kernel clamps it."""
import ctypes as C

import numpy as np

from mid_band_emul import NB, bf16_round, covariance, refine, tickets      # noqa: F401  (shared pieces, re-exported)
import mid_band_emul as mid_emu

# the eight terms, (A's part, B's part), in the order the kernel issues them (only lo lo^T is left out)
TERMS = (("mid", "lo"), ("lo", "mid"), ("hi", "lo"), ("lo", "hi"), ("mid", "mid"), ("hi", "mid"), ("mid", "hi"), ("hi", "hi"))
# variants that lose one term: what a kernel that drops a product would compute
DROPS = {"full": None, "hi_lo": ("hi", "lo"), "lo_hi": ("lo", "hi"), "mid_mid": ("mid", "mid")}


def split3(a):
    """float32 a -> (hi, mid, lo), each a bf16 value held as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = bf16_round(a)
    r = a - hi
    mid = bf16_round(r)
    lo = bf16_round(r - mid)
    return hi, mid, lo


def tables(lat_sorted, g):
    """(first | last, far, mid, near) of the library for these latitudes under the current environment."""
    from oisatgmi import _hip
    lib = _hip.load_library()
    lat_sorted = np.ascontiguousarray(lat_sorted, dtype=np.float64)
    env, far, mid = mid_emu.tables(lat_sorted, g)
    near = np.empty(far.size, dtype=np.int32)
    assert lib.oisat_factor_near(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data, mid.ctypes.data, near.ctypes.data) == 0
    return env, far, mid, near


def task_ranges(first, far, mid, near):
    """Per bulk task of the ticket list: (kind, i, j, k0, kfar, kmid, knear, kend) as an (n, 8) array: mid_band_emul.task_ranges'
    rows with knear put in front of kend."""
    r = mid_emu.task_ranges(first, far, mid)
    i, kmid, kend = r[:, 1], r[:, 5], r[:, 6]
    knear = np.minimum(np.maximum(near[i], kmid), np.maximum(kend, kmid))
    return np.concatenate([r[:, :6], knear[:, None], kend[:, None]], axis=1)


def near_share(first, far, mid, near):
    """(far, middle, near, all) K-blocks of the factorization's bulk K-loops."""
    r = task_ranges(first, far, mid, near)
    k0, kfar, kmid, knear, kend = r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7]
    return int((kfar - k0).sum()), int((kmid - kfar).sum()), int((knear - kmid).sum()), int(np.maximum(kend - k0, 0).sum())


def factor(S, first, far=None, mid=None, near=None, variant="full"):
    """The emulated factor (lower, float32, zeros outside the envelope).  variant: "full" (the kernel's rule) or one of
    "hi_lo" / "lo_hi" / "mid_mid": the near K-blocks with the a_hi b_lo^T / a_lo b_hi^T / a_mid b_mid^T term left out."""
    drop = DROPS[variant]
    mp = S.shape[0]
    nb = mp // NB
    far = first if far is None else far
    mid = far if mid is None else mid
    near = mid if near is None else near
    Lf = np.zeros((mp, mp), dtype=np.float32)
    P = {p: np.zeros((mp, mp), dtype=np.float32) for p in ("hi", "mid", "lo")}      # the three bf16 parts of the final tiles

    def blk(A, i, k):
        return A[i * NB:(i + 1) * NB, k * NB:(k + 1) * NB]

    for j in range(nb):
        Tj = None
        for i in range(j, nb):
            if first[i] > j:
                continue
            k0 = int(first[i])
            kend = j - 1 if i == j else j
            kfar = min(max(int(far[i]), k0), max(kend, k0))
            kmid = min(max(int(mid[i]), kfar), max(kend, kfar))
            knear = min(max(int(near[i]), kmid), max(kend, kmid))
            acc = np.zeros((NB, NB), dtype=np.float32)
            for k in range(k0, j):
                if k < kfar:
                    acc += blk(P["hi"], i, k) @ blk(P["hi"], j, k).T
                elif k < kmid:                                  # (the middle stretch's lo is the three-way split's mid)
                    acc += blk(P["mid"], i, k) @ blk(P["hi"], j, k).T
                    acc += blk(P["hi"], i, k) @ blk(P["mid"], j, k).T
                    acc += blk(P["hi"], i, k) @ blk(P["hi"], j, k).T
                elif k < knear:
                    for a, b in TERMS:
                        if (a, b) != drop:
                            acc += blk(P[a], i, k) @ blk(P[b], j, k).T
                else:
                    acc += blk(Lf, i, k) @ blk(Lf, j, k).T
            X = blk(S, i, j).astype(np.float32) - acc
            if i == j:
                Ljj = np.linalg.cholesky(np.tril(X).astype(np.float64) + np.tril(X, -1).astype(np.float64).T)
                Tj = np.linalg.inv(Ljj)
                out = Ljj.astype(np.float32)
            else:
                out = (X.astype(np.float64) @ Tj.T).astype(np.float32)
            blk(Lf, i, j)[:] = out
            for p, v in zip(("hi", "mid", "lo"), split3(out)):
                blk(P[p], i, j)[:] = v
    return Lf
