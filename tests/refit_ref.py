"""The box rule of fspt_scene_update_geometry, restated in numpy on reference-layout arrays.

A leaf owns the triangles [triStart, the next larger triStart among the leaves, or n_tris); its box is the min / max over
their nine-float vertices; an interior node's box is the union of its children's; a leaf that owns no triangle keeps its
box.  Min and max are taken on order-preserving integer keys (-0 < +0), so the result does not depend on any order.
`sah_cost` is the float64 arithmetic of fspt_scene_sah_cost on such arrays."""
import numpy as np


def keys(f):
    """float32 -> uint32 keys with the order of the floats (and -0 < +0)"""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def ownership(bvh, n_tris):
    """(node indices of the leaves, first triangle, triangles owned) by the rule above"""
    w = np.asarray(bvh, dtype=np.float32).reshape(-1, 9)[:, :3].view(np.int32)
    leaf = np.nonzero(w[:, 2] > -1)[0]
    first = w[leaf, 2].astype(np.int64)
    srt = np.argsort(first, kind="stable")
    nxt = np.concatenate([first[srt][1:], [n_tris]])
    cnt = np.zeros(leaf.size, np.int64)
    cnt[srt] = nxt - first[srt]
    return leaf, first, cnt


def refittable(bvh, n_tris):
    _, first, _ = ownership(bvh, n_tris)
    return first.size > 0 and np.unique(first).size == first.size and first.min() == 0


def refit(bvh, tri):
    """bvh (9 words per node, pre-order), tri (9 floats per triangle, leaf order) -> bvh with every box recomputed"""
    out = np.array(bvh, dtype=np.float32).reshape(-1, 9).copy()
    w = out[:, :3].view(np.int32)
    v = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    T = v.shape[0]
    k = keys(v.reshape(-1)).reshape(T, 3, 3)
    tmin, tmax = k.min(1), k.max(1)  # per triangle, per axis
    lo = keys(out[:, 3:6].reshape(-1)).reshape(-1, 3)
    hi = keys(out[:, 6:9].reshape(-1)).reshape(-1, 3)
    leaf, first, cnt = ownership(out, T)
    for i, a, n in zip(leaf, first, cnt):
        if n > 0:
            lo[i] = tmin[a:a + n].min(0)
            hi[i] = tmax[a:a + n].max(0)
    for i in range(out.shape[0] - 1, -1, -1):  # pre-order: children after their parent
        if w[i, 2] > -1:
            continue
        l, r = w[i, 0], w[i, 1]
        lo[i] = np.minimum(lo[l], lo[r])
        hi[i] = np.maximum(hi[l], hi[r])
    out[:, 3:6] = unkeys(lo.reshape(-1)).reshape(-1, 3)
    out[:, 6:9] = unkeys(hi.reshape(-1)).reshape(-1, 3)
    return out.reshape(-1)


def sah_cost(bvh, n_tris):
    """sum over leaves of SA / SA(root) x triangles owned + sum over interior nodes of SA / SA(root), float64"""
    b = np.asarray(bvh, dtype=np.float32).reshape(-1, 9)
    e = b[:, 6:9].astype(np.float64) - b[:, 3:6].astype(np.float64)
    sa = (e[:, 0] * e[:, 1] + e[:, 0] * e[:, 2] + e[:, 1] * e[:, 2]) * 2
    leaf, _, cnt = ownership(b, n_tris)
    interior = np.ones(b.shape[0], bool)
    interior[leaf] = False
    return float((sa[interior].sum() + (sa[leaf] * cnt).sum()) / sa[0])
