"""Independent float64 closest hit: brute-force Moller-Trumbore over every triangle of the scene, with no BVH, for
checking intersectScene (tracer.fs:366-404) in the oracle and in every HIP traversal.

The kernels and the oracle walk the same tree with the same float32 arithmetic, so their bit-equality cannot reveal an
error they share (a box one ulp too small, a culled box, a dropped leaf triangle).  This can.  It applies
rayTriangleIntersect's rule (tracer.fs:300-315: |det| >= EPSILON, 0 <= u, 0 <= v, u + v <= 1, dist > EPSILON) and
intersectScene's `res < result.t` with result.t starting at MAX_T (so dist < MAX_T), twice: eroded (every comparison
made harder by a first-order bound on the float32 rounding error) and dilated (made easier by the same bound).

  P = |d| |e2|   bounds |p| = |d x e2| and scales its rounding error
  Q = |t| |e1|   bounds |q| = |t x e1| (t = o - v1) and scales its rounding error
  tau   = max(1e-4, 64 u (|t| P + |d| Q + |e1| P) / |det|)           barycentrics (u = 2^-24)
  tau_t = 64 u (|e2| Q + |dist| |e1| P) / |det| + 4 u |dist|           distance
  tau_d = 64 u |e1| P                                                 det (|det| near EPSILON never decided by rounding)

The rounding error of a float32 cross product is bounded by the product of its operands' norms, not by the norm of
the result: with a sliver triangle or an origin on the triangle's plane, q = t x e1 cancels to a few ulps of |t| |e1|
and a bound written with |q| (or |p|) would call float32's answer wrong when it is only rounded.  The |e1| P terms
carry det's relative error into u, v and dist.

A triangle whose |det| is within 10 % (or tau_d) of EPSILON, whose dist is within a factor 2 (or tau_t) of EPSILON,
or whose dist is within tau_t of MAX_T passes the dilated test only.

Per ray:
  decisive hit   the closest eroded hit has no dilated hit closer than its tie band (tau_t of either); expected: an
                 index from the tie band (duplicated / coincident triangles: the reference's traversal order picks
                 one) and |t32 - t64[index]| <= tau_t[index].
  decisive miss  no dilated hit; expected: index -1, t == MAX_T.
  otherwise      not asserted.

Rays in a box's face plane along a zero direction component: the slab test computes 0 * inf = NaN and the
minNum/maxNum rule (DESIGN.md fspt-math) culls the box (tracer.fs:317-326 leaves NaN to the GPU).  Such a ray can only
meet that box's triangles on their boundary (every vertex lies on one side of the plane), so it is non-decisive by the
barycentric rule above and needs no special case.
"""
import numpy as np

EPSILON = float(np.float32(1e-6))     # tracer.fs:8
MAX_T = float(np.float32(100000.0))   # tracer.fs:7
U32 = 2.0 ** -24
K = 64.0                               # first-order error multiplier (dot + cross + divide chains, with margin)
TAU_MIN = 1e-4


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def classify(arrays, rays, chunk=None):
    """rays float32 [n, 6] -> Classification: kind [n] (1 decisive hit, 0 decisive miss, -1 not decisive), t64 [n]
    (the closest eroded hit, MAX_T if none) and, per decisive hit, its tie band (indices, float64 dist, tau_t)."""
    tri = arrays.tri.reshape(-1, 3, 3).astype(np.float64)
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    n, T = rays.shape[0], tri.shape[0]
    v1 = tri[:, 0]
    e1 = tri[:, 1] - v1
    e2 = tri[:, 2] - v1
    ne1, ne2 = _norm(e1), _norm(e2)
    chunk = chunk or max(1, (1 << 20) // max(T, 1))
    kind = np.full(n, -1, np.int8)
    t_best = np.full(n, MAX_T)
    tie_sets = [None] * n     # decisive hits: (indices, t64, tau_t) of the tie band
    for s in range(0, n, chunk):
        o = rays[s:s + chunk, :3].astype(np.float64)[:, None, :]
        d = rays[s:s + chunk, 3:].astype(np.float64)[:, None, :]
        p = np.cross(d, e2[None])
        det = (e1[None] * p).sum(-1)
        tv = o - v1[None]
        q = np.cross(tv, e1[None])
        adet = np.abs(det)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u = (tv * p).sum(-1) * inv
            v = (d * q).sum(-1) * inv
            dist = (e2[None] * q).sum(-1) * inv
            nt, nd = _norm(tv), _norm(d)
            P = nd * ne2[None]
            Q = nt * ne1[None]
            tau = np.maximum(TAU_MIN, K * U32 * (nt * P + nd * Q + ne1[None] * P) / adet)
            tau_t = K * U32 * (ne2[None] * Q + np.abs(dist) * ne1[None] * P) / adet + 4 * U32 * np.abs(dist)
        tau_d = K * U32 * ne1[None] * P
        finite = adet > 0
        det_lo = np.maximum(0.9 * EPSILON - tau_d, 0.0)
        det_hi = 1.1 * EPSILON + tau_d
        eps_lo = np.minimum(0.5 * EPSILON, EPSILON - tau_t)
        eps_hi = np.maximum(2.0 * EPSILON, EPSILON + tau_t)
        with np.errstate(invalid="ignore"):  # (NaN where det == 0: never a hit)
            dil = (finite & (adet >= det_lo) & (u >= -tau) & (v >= -tau) & (u + v <= 1 + tau)
                   & (dist > eps_lo) & (dist < MAX_T + tau_t))
            ero = (finite & (adet >= det_hi) & (u >= tau) & (v >= tau) & (u + v <= 1 - tau)
                   & (dist > eps_hi) & (dist < MAX_T - tau_t))
        dist_d = np.where(dil, dist, np.inf)
        dist_e = np.where(ero, dist, np.inf)
        tt_d = np.where(dil, tau_t, 0.0)
        any_d = dil.any(1)
        j = dist_e.argmin(1)
        r = np.arange(len(j))
        tj, ttj = dist_e[r, j], tt_d[r, j]
        has_e = np.isfinite(tj)
        # dilated hits strictly closer than the tie band of the eroded closest hit -> not decisive
        closer = (dist_d < (tj[:, None] - ttj[:, None] - tt_d)).any(1)
        with np.errstate(invalid="ignore"):  # (inf - inf for rays without an eroded hit: not used)
            band = dil & (np.abs(dist_d - tj[:, None]) <= ttj[:, None] + tt_d)
        dec_hit = has_e & ~closer
        for i in np.flatnonzero(dec_hit):
            b = np.flatnonzero(band[i])
            tie_sets[s + i] = (b, dist[i, b], tau_t[i, b])
        kind[s:s + chunk] = np.where(dec_hit, 1, np.where(~any_d, 0, -1))
        t_best[s:s + chunk] = np.where(has_e, tj, MAX_T)
    return Classification(kind, t_best, tie_sets)


class Classification:
    def __init__(self, kind, t64, ties):
        self.kind, self.t64, self.ties = kind, t64, ties

    def fraction(self):
        return float((self.kind >= 0).mean())

    def mismatches(self, t32, idx32):
        """Indices of decisive rays whose (t32, idx32) contradict the float64 reference."""
        t32 = np.asarray(t32, np.float32); idx32 = np.asarray(idx32)
        bad = []
        miss = np.flatnonzero(self.kind == 0)
        bad += miss[(idx32[miss] != -1) | (t32[miss] != np.float32(MAX_T))].tolist()
        for i in np.flatnonzero(self.kind == 1):
            b, tb, tt = self.ties[i]
            m = np.flatnonzero(b == idx32[i])
            if len(m) != 1 or not abs(float(t32[i]) - tb[m[0]]) <= tt[m[0]]:
                bad.append(int(i))
        return sorted(bad)

    def describe(self, i, t32, idx32):
        k = self.kind[i]
        if k == 0:
            return f"ray {i}: float64 says miss, got index {idx32[i]} t {t32[i]!r}"
        b, tb, tt = self.ties[i]
        return f"ray {i}: float64 says hit {b.tolist()} t {tb.tolist()} (+-{tt.tolist()}), got index {idx32[i]} t {t32[i]!r}"
