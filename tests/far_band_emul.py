"""NumPy emulation of the enveloped task-graph factorization with a far stretch, shared by tests/test_far_band_cpu.py and
tests/test_gpu_far_band.py: blocked left-looking Cholesky with 128 x 128 tiles inside the envelope ``first``, fp32 tiles and
fp32 accumulation, diagonal blocks in float64; the K-blocks k < far[i] of a tile of block row i take round-to-nearest-even
bf16 copies of BOTH operands (the tile (j, j) up to block column j - 2 only: the last block is the chain's fp32 update)."""
import ctypes as C

import numpy as np

NB = 128


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def tables(lat_sorted, g):
    """(first, far) of the library for these latitudes under the current environment."""
    from oisatgmi import _hip
    lib = _hip.load_library()
    lat_sorted = np.ascontiguousarray(lat_sorted, dtype=np.float64)
    nb = -(-lat_sorted.size // NB)
    env = np.empty(2 * nb, dtype=np.int32)
    far = np.empty(nb, dtype=np.int32)
    assert lib.oisat_factor_envelope(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data) == 0
    assert lib.oisat_factor_far(lat_sorted.ctypes.data, lat_sorted.size, C.c_double(g), env.ctypes.data, far.ctypes.data) == 0
    return env, far


def tickets(first, far):
    """The enveloped ticket list as (n, 4) int32: (kind | k0 << 8 | kfar << 18, system, i, j)."""
    from oisatgmi import _hip
    lib = _hip.load_library()
    first = np.ascontiguousarray(first, dtype=np.int32)
    far_p = None if far is None else np.ascontiguousarray(far, dtype=np.int32)
    n = C.c_int64(0)
    assert lib.oisat_dag_task_order_env(first.size, first.ctypes.data, None if far is None else far_p.ctypes.data, None, 0, C.byref(n)) == 0
    out = np.empty((n.value, 4), dtype=np.int32)
    assert lib.oisat_dag_task_order_env(first.size, first.ctypes.data, None if far is None else far_p.ctypes.data, out.ctypes.data,
                                        n.value, C.byref(n)) == 0
    return out


def far_share(first, far):
    """(far K-blocks, all K-blocks) of the factorization's bulk K-loops: tile (i, j) runs k = first[i] .. kend - 1, kend = j (the
    diagonal tile: j - 1), the blocks below far[i] of it on the bf16 pipe."""
    nb = first.size
    n_far = n_all = 0
    for i in range(nb):
        j = np.arange(first[i], i + 1)
        kend = np.where(j == i, j - 1, j)
        n_all += int(np.maximum(kend - first[i], 0).sum())
        n_far += int(np.maximum(np.minimum(kend, far[i]) - first[i], 0).sum())
    return n_far, n_all


def covariance(po, sig, var, g, first=None, dtype=np.float32):
    """S = sig_i sig_j exp(-g chord^2) + diag(var), padded to full blocks with the identity; ``first``: zero left of the envelope."""
    m = po.shape[0]
    mp = -(-m // NB) * NB
    S = np.zeros((mp, mp), dtype=dtype)
    d2 = np.maximum(2.0 - 2.0 * (po @ po.T), 0.0)
    S[:m, :m] = (np.exp(-g * d2) * sig[:, None] * sig[None, :]).astype(dtype)
    S[np.arange(m), np.arange(m)] = (sig * sig + var).astype(dtype)
    S[np.arange(m, mp), np.arange(m, mp)] = 1.0
    if first is not None:
        for i in range(mp // NB):
            S[i * NB:(i + 1) * NB, :first[i] * NB] = 0.0
            S[:first[i] * NB, i * NB:(i + 1) * NB] = 0.0
    return S


def factor(S, first, far=None):
    """The emulated factor (lower, float32, zeros outside the envelope); raises numpy.linalg.LinAlgError if not positive definite."""
    mp = S.shape[0]
    nb = mp // NB
    far = first if far is None else far
    Lf = np.zeros((mp, mp), dtype=np.float32)
    Lb = np.zeros((mp, mp), dtype=np.float32)                  # bf16 copies of the final tiles

    def blk(A, i, k):
        return A[i * NB:(i + 1) * NB, k * NB:(k + 1) * NB]

    for j in range(nb):
        Tj = None
        for i in range(j, nb):
            if first[i] > j:
                continue
            k0 = int(first[i])
            kend = j - 1 if i == j else j                       # (far purposes only: PRE(j) stops at j - 1)
            kfar = min(max(int(far[i]), k0), max(kend, k0))
            acc = np.zeros((NB, NB), dtype=np.float32)
            for k in range(k0, j):
                src = Lb if k < kfar else Lf
                acc += blk(src, i, k) @ blk(src, j, k).T
            X = blk(S, i, j).astype(np.float32) - acc
            if i == j:
                Ljj = np.linalg.cholesky(np.tril(X).astype(np.float64) + np.tril(X, -1).astype(np.float64).T)
                Tj = np.linalg.inv(Ljj)
                out = Ljj.astype(np.float32)
            else:
                out = (X.astype(np.float64) @ Tj.T).astype(np.float32)
            blk(Lf, i, j)[:] = out
            blk(Lb, i, j)[:] = bf16_round(out)
    return Lf


def refine(Lf, S64, d, rounds=1):
    """Relative float64 residuals |d - S z| / |d| of z = M^-1 d and of ``rounds`` corrections, M = L L^T (float64 sweeps)."""
    import scipy.linalg as sla
    m = d.size
    L64 = Lf[:m, :m].astype(np.float64)

    def minv(r):
        return sla.solve_triangular(L64, sla.solve_triangular(L64, r, lower=True), lower=True, trans="T")

    z = minv(d)
    out = []
    for it in range(rounds + 1):
        r = d - S64 @ z
        out.append(float(np.linalg.norm(r) / np.linalg.norm(d)))
        if it < rounds:
            z = z + minv(r)
    return out
