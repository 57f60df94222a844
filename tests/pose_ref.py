"""The rule of DESIGN 8.14 (GPU part transforms) in numpy, bit for bit.

Host part, float64, in the stated order (derive): per part a 3 x 4 matrix -> (a, D, N) with
    q = left-to-right sum of the nine squares of A (row-major), g = sqrt(q / 3),
    C = the signed cofactors of A, det = (A00 C00 + A01 C01) + A02 C02,
    D = float32(A / g), N = float32(C / (g g));
a part is refused when an input is not finite, det == 0 or an entry of D / N is not finite.
Device part, float32, an fma exactly where one is written (fma32 of tests/exposure_ref.py: exact, round-to-odd in float64):
    vertex   p'_c = fma(a_c2, z, fma(a_c1, y, fma(a_c0, x, t_c)))
    t, bt    d'_c = fma(D_c2, z, fma(D_c1, y, D_c0 * x))
    n        the same with N        (frame vector j of a triangle's nine: j % 3 == 0 is the normal)
Nothing is normalised."""
import numpy as np

from exposure_ref import fma32

F = np.float32


class Rejected(ValueError):
    def __init__(self, part, why):
        super().__init__(f"part {part}: {why}")
        self.part = part


def derive(xf):
    """xf [n_parts, 12] float32 -> (a [n, 3, 4], D [n, 3, 3], N [n, 3, 3]) float32; raises Rejected(part)"""
    xf = np.asarray(xf, F).reshape(-1, 3, 4)
    D = np.zeros((xf.shape[0], 3, 3), F)
    N = np.zeros((xf.shape[0], 3, 3), F)
    for p, m in enumerate(xf):
        if not np.isfinite(m).all():
            raise Rejected(p, "an entry is not finite")
        A = m[:, :3].astype(np.float64)
        q = np.float64(0.0)
        for i in range(3):
            for j in range(3):
                q = q + A[i, j] * A[i, j]
        g = np.sqrt(q / np.float64(3.0))
        C = np.zeros((3, 3), np.float64)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                C[i, j] = A[i1, j1] * A[i2, j2] - A[i1, j2] * A[i2, j1]
        det = (A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1]) + A[0, 2] * C[0, 2]
        if det == 0.0:
            raise Rejected(p, "the matrix is singular")
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            D[p] = (A / g).astype(F)
            N[p] = (C / (g * g)).astype(F)
        if not (np.isfinite(D[p]).all() and np.isfinite(N[p]).all()):
            raise Rejected(p, "a derived matrix is not finite")
    return xf.copy(), D, N


def _affine(rows, v, t=None):
    """rows [n, 3, 3] (per vector), v [n, 3], t [n, 3] or None -> [n, 3] float32"""
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (rows[:, :, 0] * x).astype(F) if t is None else fma32(rows[:, :, 0], x, t)
        acc = fma32(rows[:, :, 1], y, acc)
        return fma32(rows[:, :, 2], z, acc)


def pose(part, tri, norm, xf):
    """part [T] ids, rest tri [T, 9] / norm [T, 27] (or None), xf [n_parts, 12] -> (tri' [T, 9], norm' [T, 27] or None),
    float32, what k_pose_transform writes"""
    a, D, N = derive(xf)
    part = np.asarray(part, np.int64).reshape(-1)
    T = part.size
    v = np.asarray(tri, F).reshape(T * 3, 3)
    pv = np.repeat(part, 3)
    out_t = _affine(a[pv][:, :, :3], v, a[pv][:, :, 3]).reshape(T, 9)
    if norm is None:
        return out_t, None
    f = np.asarray(norm, F).reshape(T * 9, 3)
    pf = np.repeat(part, 9)
    is_n = (np.arange(T * 9) % 9) % 3 == 0
    rows = np.where(is_n[:, None, None], N[pf], D[pf])
    return out_t, _affine(rows, f).reshape(T, 27)
