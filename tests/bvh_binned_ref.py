"""numpy restatement of the binned-SAH BVH build of fspt_builder_build_gpu (fspt_amd/csrc/fspt_bvh_build.hip),
written from the algorithm's specification.  One level of the tree per step, every node of the level at once.

    build(verts, leaf_size) -> Tree: the reference-layout `bvh` array (9 words per node, pre-order), the triangle order
    of the leaves, the depth, and per node its range, children and box

Floats are compared through order-preserving integer keys (-0 < +0), so every min / max is exact and independent of
order; counts are integers; the SAH cost is float64 on the float32 boxes."""
import os
import re
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one definition of K: the kernel's
K = int(re.search(r"#define FSPT_BVH_BINS (\d+)",
                  open(os.path.join(ROOT, "fspt_amd", "csrc", "fspt_bvh_build.hip")).read()).group(1))
# deepest node depth fspt_scene_create accepts: min(64, wf_max_stack_entries()) - 1; the stack holds 112 entries with the
# present LDS budget, so the 64 of the reference's int[64] stack decides
MAX_DEPTH = 63


def key(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def levels_below(n, leaf_size):
    """ceil(log2(ceil(n / leaf_size))), elementwise on integers"""
    x = (np.asarray(n, np.int64) + leaf_size - 1) // leaf_size - 1
    lv = np.zeros_like(x)
    while (x > 0).any():
        lv += x > 0
        x = x >> 1
    return lv


def bin_of(c, cmin, scl):
    """min(K-1, (uint32)((c - cmin) * (K / e))) in float32; NaN -> 0 and +inf -> K-1"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = (c - cmin) * scl
        safe = np.where(f > 0, np.minimum(f, np.float32(K)), np.float32(0))
        return np.where(f >= np.float32(K), K - 1, safe.astype(np.int64)).astype(np.int64)


def surface_area(lo_keys, hi_keys):
    """Box::surface_area on float32 boxes, in float64: (xl*yl + xl*zl + yl*zl) * 2"""
    lo = unkey(lo_keys).astype(np.float64)
    hi = unkey(hi_keys).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        xl, yl, zl = (hi[..., k] - lo[..., k] for k in range(3))
        return (xl * yl + xl * zl + yl * zl) * 2


@dataclass
class Tree:
    bvh: np.ndarray        # float32 [n_nodes*9]: left, right, first tri (int bits), box min.xyz, max.xyz
    order: np.ndarray      # uint32 [n]: triangle of leaf slot k
    depth: int
    lo: np.ndarray         # per node (pre-order): range [lo, lo + cnt) of `order`
    cnt: np.ndarray
    left: np.ndarray       # children (-1 on leaves)
    right: np.ndarray
    node_depth: np.ndarray
    box_keys: np.ndarray   # [n_nodes, 6]
    sah_split: np.ndarray  # bool: interior node split by SAH (False: floor(n/2))


def prims(verts):
    """triangle box keys [n, 6] and centroids [n, 3] (float32)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3, 3)
    k = key(v)
    bk = np.concatenate([k.min(1), k.max(1)], 1)
    with np.errstate(over="ignore"):  # min + max beyond float32's range is +-inf, as on the device
        c = (unkey(bk[:, :3]) + unkey(bk[:, 3:])) * np.float32(0.5)
    return bk, c.astype(np.float32)


def build(verts, leaf_size, max_depth=MAX_DEPTH):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
    if not np.isfinite(verts).all():
        raise ValueError("non-finite vertex")
    if not 1 <= leaf_size <= 64:
        raise ValueError("leaf_size must be 1..64")
    n = verts.shape[0]
    bk, cent = prims(verts)
    ck = key(cent)
    order = np.arange(n, dtype=np.int64)
    # nodes in creation order
    n_lo, n_cnt, n_dep, n_left, n_right, n_box, n_sah = [0], [n], [0], [-1], [-1], [None], [False]
    active = np.array([0], np.int64)
    while active.size:
        lo = np.array([n_lo[i] for i in active], np.int64)
        cnt = np.array([n_cnt[i] for i in active], np.int64)
        dep = np.array([n_dep[i] for i in active], np.int64)
        S = active.size
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        seg = np.repeat(np.arange(S), cnt)
        rel = np.arange(seg.size) - starts[seg]         # position inside the node
        pos = lo[seg] + rel
        tri = order[pos]
        # bounds
        box = np.concatenate([np.minimum.reduceat(bk[tri, :3], starts), np.maximum.reduceat(bk[tri, 3:], starts)], 1)
        cmin_k = np.minimum.reduceat(ck[tri], starts)
        cmax_k = np.maximum.reduceat(ck[tri], starts)
        for s in range(S):
            n_box[active[s]] = box[s]
        inner = cnt > leaf_size
        if not inner.any():
            break
        cmin = unkey(cmin_k)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ext = unkey(cmax_k) - cmin
            ok = ext > 0
            scl = np.float32(K) / ext
        # bins per (node, axis, bin): count, box keys
        cnts = np.zeros((S, 3, K), np.int64)
        bmin = np.full((S, 3, K, 3), 0xFFFFFFFF, np.uint32)
        bmax = np.zeros((S, 3, K, 3), np.uint32)
        bins = np.empty((seg.size, 3), np.int64)
        for a in range(3):
            b = bin_of(cent[tri, a], cmin[seg, a], scl[seg, a])
            bins[:, a] = b
            flat = seg * K + b
            srt = np.argsort(flat, kind="stable")
            fs = flat[srt]
            first = np.flatnonzero(np.concatenate([[True], fs[1:] != fs[:-1]]))
            u = fs[first]
            cnts[u // K, a, u % K] = np.diff(np.concatenate([first, [fs.size]]))
            bmin[u // K, a, u % K] = np.minimum.reduceat(bk[tri[srt], :3], first)
            bmax[u // K, a, u % K] = np.maximum.reduceat(bk[tri[srt], 3:], first)
        # candidates j = 1..K-1: left = bins < j, right = bins >= j
        nl = np.cumsum(cnts, 2)[:, :, :-1]
        nr = cnt[:, None, None] - nl
        lmin = np.minimum.accumulate(bmin, 2)[:, :, :-1]
        lmax = np.maximum.accumulate(bmax, 2)[:, :, :-1]
        rmin = np.minimum.accumulate(bmin[:, :, ::-1], 2)[:, :, ::-1][:, :, 1:]
        rmax = np.maximum.accumulate(bmax[:, :, ::-1], 2)[:, :, ::-1][:, :, 1:]
        sp = surface_area(box[:, :3], box[:, 3:])[:, None, None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            cost = surface_area(lmin, lmax) / sp * nl.astype(np.float64) + surface_area(rmin, rmax) / sp * nr.astype(np.float64)
        valid = (nl > 0) & (nr > 0) & ~np.isnan(cost) & ok[:, :, None]
        cost = np.where(valid, cost, np.inf).reshape(S, -1)
        best = np.argmin(cost, 1)                       # first occurrence: axis 0..2, then j ascending
        has = valid.reshape(S, -1)[np.arange(S), best]
        ax, j = best // (K - 1), best % (K - 1) + 1
        nl_s = nl.reshape(S, -1)[np.arange(S), best]
        guard = (dep + 1 + levels_below(nl_s, leaf_size) <= max_depth) & \
                (dep + 1 + levels_below(cnt - nl_s, leaf_size) <= max_depth)
        sah = inner & has & guard
        nl_n = np.where(sah, nl_s, cnt // 2)
        # stable partition of every interior node
        go_left = np.where(sah[seg], bins[np.arange(seg.size), ax[seg]] < j[seg], rel < nl_n[seg])
        keep = inner[seg]
        lcum = np.cumsum(go_left) - go_left
        lrank = lcum - lcum[starts][seg]               # lefts before this element inside its node
        dst = lo[seg] + np.where(go_left, lrank, nl_n[seg] + rel - lrank)
        order[dst[keep]] = tri[keep]
        nxt = []
        for s in np.flatnonzero(inner):
            i = int(active[s])
            c = len(n_lo)
            n_left[i], n_right[i], n_sah[i] = c, c + 1, bool(sah[s])
            for lo_c, cnt_c in ((lo[s], nl_n[s]), (lo[s] + nl_n[s], cnt[s] - nl_n[s])):
                n_lo.append(int(lo_c)); n_cnt.append(int(cnt_c)); n_dep.append(int(dep[s]) + 1)
                n_left.append(-1); n_right.append(-1); n_box.append(None); n_sah.append(False)
            nxt += [c, c + 1]
        active = np.array(nxt, np.int64)
    # pre-order numbering
    pre, stack = [], [0]
    while stack:
        i = stack.pop()
        pre.append(i)
        if n_left[i] >= 0:
            stack += [n_right[i], n_left[i]]
    N = len(pre)
    num = np.empty(len(n_lo), np.int64)
    num[pre] = np.arange(N)
    P = np.array(pre)
    left = np.array([num[n_left[i]] if n_left[i] >= 0 else -1 for i in pre], np.int64)
    right = np.array([num[n_right[i]] if n_right[i] >= 0 else -1 for i in pre], np.int64)
    lo_p = np.array(n_lo, np.int64)[P]
    words = np.zeros((N, 3), np.int32)
    leaf = left < 0
    words[:, 0] = np.where(leaf, 0, left)
    words[:, 1] = np.where(leaf, 0, right)
    words[:, 2] = np.where(leaf, lo_p, -1)
    box_keys = np.stack([n_box[i] for i in pre]).astype(np.uint32)
    bvh = np.zeros((N, 9), np.float32)
    bvh[:, :3] = words.view(np.float32)
    bvh[:, 3:] = unkey(box_keys)
    dep_p = np.array(n_dep, np.int64)[P]
    return Tree(bvh=bvh.reshape(-1), order=order.astype(np.uint32), depth=int(dep_p.max()), lo=lo_p,
                cnt=np.array(n_cnt, np.int64)[P], left=left, right=right, node_depth=dep_p, box_keys=box_keys,
                sah_split=np.array(n_sah, bool)[P])


def geometry_order(arrays):
    """The per-triangle arrays of a scene built with keep_order=True, back in the order the OBJs added the triangles:
    dict(tri, mat, norm, uv) of shape [n, 9 / 12 / 27 / 6]."""
    order = arrays.meta["tri_order"]
    out = {}
    for name, w in (("tri", 9), ("mat", 12), ("norm", 27), ("uv", 6)):
        a = getattr(arrays, name).reshape(-1, w)
        g = np.empty_like(a)
        g[order] = a
        out[name] = g
    return out


def expected_arrays(arrays, leaf_size=None):
    """What fspt_builder_build_gpu must produce for the scene `arrays` (built with keep_order=True by either builder):
    (Tree, dict(bvh, tri, mat, norm, uv) flat float32)."""
    g = geometry_order(arrays)
    t = build(g["tri"], leaf_size or arrays.leaf_size)
    out = {"bvh": t.bvh}
    for name in ("tri", "mat", "norm", "uv"):
        out[name] = g[name][t.order].reshape(-1)
    return t, out



def rebuild(make, *args, **overrides):
    """Run make(*args), which builds its scene with one scene.build_scene call, and build the same inputs again with
    `overrides` (bvh=..., keep_order=...) - for scene makers (tests/rays.py fuzz_scene, ...) that take no builder option."""
    from fspt_amd import scene as S
    calls = []
    orig = S.build_scene

    def spy(*a, **kw):
        calls.append((a, kw))
        return orig(*a, **kw)

    S.build_scene = spy
    try:
        make(*args)
    finally:
        S.build_scene = orig
    a, kw = calls[0]
    return orig(*a, **dict(kw, **overrides))


def check_tree(bvh, tri, leaf_size, depth):
    """A reference-layout tree (flat bvh / tri arrays): pre-order numbering, leaves of 1..leaf_size triangles packed in
    pre-order, the given depth within the guard, every box exactly the min / max of its triangles' vertices."""
    b = np.asarray(bvh, np.float32).reshape(-1, 9)
    w = b[:, :3].view(np.int32)
    N = b.shape[0]
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    T = t.shape[0]
    leaf = w[:, 2] > -1
    tk = key(t)
    tbox = np.concatenate([tk.min(1), tk.max(1)], 1)
    visit, stack, dep = [], [(0, 0)], np.zeros(N, np.int64)
    while stack:
        i, d = stack.pop()
        visit.append(i)
        dep[i] = d
        if not leaf[i]:
            assert w[i, 0] == i + 1 and w[i, 1] > i + 1 and w[i, 1] < N
            stack += [(int(w[i, 1]), d + 1), (int(w[i, 0]), d + 1)]
    assert visit == list(range(N))
    first = w[leaf, 2]
    assert first[0] == 0 and np.all(np.diff(first) > 0) and first[-1] < T
    cnt = np.diff(np.concatenate([first, [T]]))
    assert cnt.min() >= 1 and cnt.max() <= leaf_size
    assert dep.max() == depth <= MAX_DEPTH
    keys = np.zeros((N, 6), np.uint32)
    lidx = np.flatnonzero(leaf)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    keys[lidx, :3] = np.minimum.reduceat(tbox[:, :3], starts)
    keys[lidx, 3:] = np.maximum.reduceat(tbox[:, 3:], starts)
    for i in np.flatnonzero(~leaf)[::-1]:
        l, r = w[i, 0], w[i, 1]
        keys[i, :3] = np.minimum(keys[l, :3], keys[r, :3])
        keys[i, 3:] = np.maximum(keys[l, 3:], keys[r, 3:])
    assert np.array_equal(key(b[:, 3:]), keys)
