"""NumPy emulation of the enveloped task-graph factorization with a far AND a middle stretch, shared by
tests/test_mid_band_cpu.py and tests/test_gpu_mid_band.py: tests/far_band_emul.py's blocked left-looking Cholesky (fp32 tiles,
fp32 accumulation, diagonal blocks in float64) in which the K-blocks kfar <= k < kmid of a tile of block row i are split bf16
products: beside every final fp32 tile it keeps hi = bf16_round(L) and lo = bf16_round(L - hi), and a middle K-block adds
lo hi^T, hi lo^T and hi hi^T, in that order.  kfar and kmid are clamped as the kernel clamps them: kfar = far[i] into
[k0, kend], kmid = mid[i] into [kfar, kend], kend = j (the diagonal tile: j - 1, its last block is the chain's fp32 update)."""
import ctypes as C

import numpy as np

from far_band_emul import NB, bf16_round, covariance, refine, tickets      # noqa: F401  (shared pieces, re-exported)
import far_band_emul as far_emu


def tables(lat_sorted, g):
    """(first | last, far, mid) of the library for these latitudes under the current environment."""
    from oisatgmi import _hip
    lib = _hip.load_library()
    lat_sorted = np.ascontiguousarray(lat_sorted, dtype=np.float64)
    env, far = far_emu.tables(lat_sorted, g)
    mid = np.empty(far.size, dtype=np.int32)
    assert lib.oisat_factor_mid(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data, far.ctypes.data, mid.ctypes.data) == 0
    return env, far, mid


def task_ranges(first, far, mid):
    """Per bulk task of the ticket list: (kind, i, j, k0, kfar, kmid, kend) as an (n, 7) array, kfar from the ticket word."""
    t = tickets(first, far)
    t = t[(t[:, 0] & 255) != 0]
    kind, k0, kfar = t[:, 0] & 255, (t[:, 0] >> 8) & 1023, t[:, 0] >> 18
    i, j = t[:, 2], t[:, 3]
    kend = np.where(kind == 3, j - 1, j)
    kmid = np.minimum(np.maximum(mid[i], kfar), np.maximum(kend, kfar))
    return np.stack([kind, i, j, k0, kfar, kmid, kend], axis=1)


def mid_share(first, far, mid):
    """(far, middle, all) K-blocks of the factorization's bulk K-loops."""
    r = task_ranges(first, far, mid)
    k0, kfar, kmid, kend = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    return int((kfar - k0).sum()), int((kmid - kfar).sum()), int(np.maximum(kend - k0, 0).sum())


def factor(S, first, far=None, mid=None, middle="split"):
    """The emulated factor (lower, float32, zeros outside the envelope).  middle: how the K-blocks kfar <= k < kmid are formed --
    "split" (the kernel's rule), "single" (rounded to bf16 like the far ones), or "lo_hi" / "hi_lo" / "hi_only" (the split with
    the a_hi b_lo^T term / the a_lo b_hi^T term / both cross terms left out: what a kernel that loses a term would compute)."""
    mp = S.shape[0]
    nb = mp // NB
    far = first if far is None else far
    mid = far if mid is None else mid
    Lf = np.zeros((mp, mp), dtype=np.float32)
    Lh = np.zeros((mp, mp), dtype=np.float32)                  # bf16 copies of the final tiles ...
    Ll = np.zeros((mp, mp), dtype=np.float32)                  # ... and of what they leave

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
            acc = np.zeros((NB, NB), dtype=np.float32)
            for k in range(k0, j):
                if k < kfar or (k < kmid and middle == "single"):
                    acc += blk(Lh, i, k) @ blk(Lh, j, k).T
                elif k < kmid:
                    if middle in ("split", "lo_hi"):
                        acc += blk(Ll, i, k) @ blk(Lh, j, k).T
                    if middle in ("split", "hi_lo"):
                        acc += blk(Lh, i, k) @ blk(Ll, j, k).T
                    acc += blk(Lh, i, k) @ blk(Lh, j, k).T
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
            hi = bf16_round(out)
            blk(Lh, i, j)[:] = hi
            blk(Ll, i, j)[:] = bf16_round(out - hi)
    return Lf
