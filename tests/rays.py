"""Labelled families of edge-case rays for the traversal tests, built from a scene's own data, and the fuzz-scene
generator the CPU and GPU traversal tests share.

conftest.random_rays shoots rays from a shell around the scene at Gaussian targets; it never produces the inputs where
a slab test or Moller-Trumbore is hardest to get right: zero direction components (1/d = +-inf, and 0 * inf = NaN when
the origin lies on a box plane), rays through shared edges and vertices, rays in a triangle's plane, origins on a
surface, far origins, denormal components.  Every family here is deterministic in (scene, seed), returns float32
[n, 6] rays (origin, direction) and its label, and keeps every value finite (the reference never makes NaN / Inf rays).

chain_scene builds the deepest tree the reference can walk (a chain: depth n_leaves - 1) for the parity and feature tests.
"""
import numpy as np

TINY = (1e-38, 1e-40, 1.4e-45)   # smallest normal scale, a denormal, the smallest denormal


def _tris(arrays):
    return arrays.tri.reshape(-1, 3, 3)


def _bounds(arrays):
    v = _tris(arrays).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)


def _nodes(arrays):
    """(n_nodes, 9) view: words 0-2 are int32 (left, right, first triangle or -1), then bmin[3], bmax[3]."""
    b = arrays.bvh.reshape(-1, 9)
    return b[:, :3].view(np.int32), b[:, 3:6], b[:, 6:9]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _targets(arrays, rng, n):
    """Points on the scene's triangles (random barycentrics), float64."""
    tri = _tris(arrays).astype(np.float64)
    k = rng.integers(0, len(tri), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return np.einsum("nk,nkj->nj", w, tri[k])


def _pack(o, d):
    r = np.concatenate([np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)], 1)
    assert np.isfinite(r).all()
    return np.ascontiguousarray(r)


def _signed_zero(rng, shape):
    return np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def axis(arrays, seed, n=1024):
    """Directions exactly +-e_x, +-e_y, +-e_z with the zero components +0 or -0; origins on a grid over the root box
    grown by 10 %, and origins whose coordinates along the zero axes are node-box bmin / bmax values (0 * inf)."""
    rng = np.random.default_rng(seed)
    lo, hi, _, _ = _bounds(arrays)
    ext = hi - lo
    glo, ghi = lo - 0.1 * ext - 1e-3, hi + 0.1 * ext + 1e-3
    _, bmin, bmax = _nodes(arrays)
    planes = np.concatenate([bmin, bmax], 0)                 # float32 node-box coordinates, [2 * n_nodes, 3]
    k = rng.integers(0, 3, n)                                # the direction's axis
    sgn = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    d = _signed_zero(rng, (n, 3))
    d[np.arange(n), k] = sgn
    g = int(np.ceil(np.sqrt(n / 2)))
    ij = rng.integers(0, g + 1, (n, 3)) / g                  # grid cells
    o = (glo + ij * (ghi - glo)).astype(np.float32)
    on_box = rng.random(n) < 0.5                             # the zero axes take actual box planes
    pick = planes[rng.integers(0, len(planes), (n, 3)), np.arange(3)[None, :]]
    for a in range(3):
        m = on_box & (k != a)
        o[m, a] = pick[m, a]
    # start outside the grown box along the direction, shooting in (and some from inside)
    start = np.where(sgn > 0, glo[k], ghi[k]).astype(np.float32)
    outside = rng.random(n) < 0.7
    o[outside, k[outside]] = start[outside]
    return _pack(o, d), "axis"


def plane(arrays, seed, n=1024):
    """One exactly-zero component (+0 or -0), two nonzero: normalised in float64, rounded to float32, re-zeroed.
    Aimed at points on the triangles; half the origins put the zero axis on a node-box plane."""
    rng = np.random.default_rng(seed)
    _, _, _, r = _bounds(arrays)
    _, bmin, bmax = _nodes(arrays)
    planes = np.concatenate([bmin, bmax], 0)
    k = rng.integers(0, 3, n)
    d = rng.normal(size=(n, 3))
    d[np.arange(n), k] = 0.0
    d = _unit(d).astype(np.float32)
    d[np.arange(n), k] = _signed_zero(rng, n)
    tgt = _targets(arrays, rng, n)
    o = (tgt - d.astype(np.float64) * r * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32)
    on_box = rng.random(n) < 0.5
    o[on_box, k[on_box]] = planes[rng.integers(0, len(planes), on_box.sum()), k[on_box]]
    return _pack(o, d), "plane"


def _shared_edges(tri):
    """Midpoints (float64) of edges that two or more triangles share (exact float32 vertex equality)."""
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    ka, kb = a.view(np.uint32), b.view(np.uint32)
    first = np.array([tuple(x) <= tuple(y) for x, y in zip(ka.tolist(), kb.tolist())])
    key = np.where(first[:, None], np.concatenate([ka, kb], 1), np.concatenate([kb, ka], 1))
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    shared = cnt[inv.ravel()] >= 2
    return (a[shared].astype(np.float64) + b[shared].astype(np.float64)) / 2


def vertex_edge(arrays, seed, n=1024):
    """From origins on a shell around the scene, aimed at exact float32 vertices, at midpoints of edges shared by two
    triangles, and at centroids."""
    rng = np.random.default_rng(seed)
    tri = _tris(arrays)
    _, _, c, r = _bounds(arrays)
    verts = tri.reshape(-1, 3).astype(np.float64)
    mids = _shared_edges(tri)
    cents = tri.astype(np.float64).mean(1)
    pools = [verts, cents] + ([mids] if len(mids) else [])
    which = rng.integers(0, len(pools), n)
    tgt = np.stack([pools[w][rng.integers(0, len(pools[w]))] for w in which])
    o = (c + _sphere(rng, n) * r * rng.uniform(1.05, 2.0, (n, 1))).astype(np.float32)
    d = _unit(tgt - o.astype(np.float64))
    return _pack(o, d), "vertex_edge"


def _normals(tri64):
    return np.cross(tri64[:, 1] - tri64[:, 0], tri64[:, 2] - tri64[:, 0])


def grazing(arrays, seed, n=1024):
    """Directions in a triangle's plane (float64 cross product with its normal) passing within a small offset of its
    centroid."""
    rng = np.random.default_rng(seed)
    tri = _tris(arrays).astype(np.float64)
    nrm = _normals(tri)
    ok = np.flatnonzero(np.linalg.norm(nrm, axis=1) > 0)
    k = ok[rng.integers(0, len(ok), n)]
    nk = _unit(nrm[k])
    d = _unit(np.cross(nk, rng.normal(size=(n, 3))))
    size = np.linalg.norm(tri[k, 1] - tri[k, 0], axis=1, keepdims=True)
    cen = tri[k].mean(1)
    off = nk * size * rng.choice([0.0, 1e-7, -1e-7, 1e-4, -1e-4], (n, 1))
    o = cen + off - d * size * rng.uniform(1.5, 4.0, (n, 1))
    return _pack(o, d), "grazing"


def on_surface(arrays, seed, n=1024):
    """Origin at a triangle's float32 centroid; directions +-normal and random hemisphere directions (the
    `dist > EPSILON` test of tracer.fs:314 decided near its threshold)."""
    rng = np.random.default_rng(seed)
    tri = _tris(arrays)
    nrm = _normals(tri.astype(np.float64))
    ok = np.flatnonzero(np.linalg.norm(nrm, axis=1) > 0)
    k = ok[rng.integers(0, len(ok), n)]
    o = tri[k].mean(1, dtype=np.float32)
    nk = _unit(nrm[k]) * np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0)
    h = _sphere(rng, n)
    h = np.where((h * nk).sum(1, keepdims=True) < 0, -h, h)
    d = np.where(rng.random((n, 1)) < 0.4, nk, h)
    return _pack(o, _unit(d)), "on_surface"


def far(arrays, seed, n=1024):
    """Unit directions from origins 1e2 - 1e6 scene radii away, aimed at the scene (or near it): includes hits beyond
    MAX_T = 1e5 (tracer.fs:7)."""
    rng = np.random.default_rng(seed)
    _, _, c, r = _bounds(arrays)
    o = c + _sphere(rng, n) * r * 10 ** rng.uniform(2, 6, (n, 1))
    tgt = np.where(rng.random((n, 1)) < 0.7, _targets(arrays, rng, n), c + rng.normal(size=(n, 3)) * r)
    o = o.astype(np.float32)
    d = _unit(tgt - o.astype(np.float64))
    return _pack(o, d), "far"


def tiny(arrays, seed, n=1024):
    """One or two direction components set to +-1e-38, +-1e-40 (denormal) or +-1.4e-45, the rest renormalised."""
    rng = np.random.default_rng(seed)
    _, _, c, r = _bounds(arrays)
    o = c + _sphere(rng, n) * r * rng.uniform(0.3, 2.0, (n, 1))
    d = _unit(_targets(arrays, rng, n) - o)
    n_tiny = rng.integers(1, 3, n)
    order = np.argsort(rng.random((n, 3)), 1)
    val = np.float64(np.array(TINY, np.float32))[rng.integers(0, 3, (n, 3))] * np.where(rng.random((n, 3)) < 0.5, 1, -1)
    is_tiny = np.zeros((n, 3), bool)
    is_tiny[np.arange(n), order[:, 0]] = True
    is_tiny[np.arange(n)[n_tiny == 2], order[n_tiny == 2, 1]] = True
    rest = np.where(is_tiny, 0.0, d)
    rest = rest / np.linalg.norm(rest, axis=1, keepdims=True)
    d32 = np.where(is_tiny, val, rest).astype(np.float32)
    return _pack(o, d32), "tiny"


def inside(arrays, seed, n=1024):
    """Origins inside the root box and inside leaf boxes, random unit directions."""
    rng = np.random.default_rng(seed)
    w, bmin, bmax = _nodes(arrays)
    leaves = np.flatnonzero(w[:, 2] > -1)
    box = np.where(rng.random(n) < 0.3, 0, leaves[rng.integers(0, len(leaves), n)])
    lo, hi = bmin[box].astype(np.float64), bmax[box].astype(np.float64)
    o = lo + rng.random((n, 3)) * (hi - lo)
    return _pack(o, _sphere(rng, n)), "inside"


def scaled(arrays, seed, n=1024):
    """Non-unit directions, |d| = 1e-3 and 1e3 (intersection only: camera.fs and the bounce loop make unit
    directions)."""
    rng = np.random.default_rng(seed)
    _, _, c, r = _bounds(arrays)
    o = c + _sphere(rng, n) * r * rng.uniform(0.3, 2.0, (n, 1))
    d = _unit(_targets(arrays, rng, n) + rng.normal(size=(n, 3)) * r * 0.1 - o)
    d *= np.where(rng.random((n, 1)) < 0.5, 1e-3, 1e3)
    return _pack(o, d), "scaled"


UNIT_FAMILIES = (axis, plane, vertex_edge, grazing, on_surface, far, tiny, inside)
FAMILIES = UNIT_FAMILIES + (scaled,)


def all_families(arrays, seed, n=1024, families=FAMILIES):
    return [f(arrays, seed * 131 + i, n) for i, f in enumerate(families)]


def fuzz_scene(seed):
    """Random triangle soup with awkward members (degenerate, sliver, huge, duplicated and coplanar triangles,
    shared edges), random per-group MTL materials (dielectric, metallic, rough, emissive), random leaf size,
    random small RGBE environment or none."""
    from fspt_amd import scene as S
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 120))
    lines, faces = [], []
    for k in range(n):
        c = rng.normal(size=3) * 1.5
        kind = rng.integers(0, 10)
        if kind == 0:      # degenerate: two equal vertices -> NaN normals (obj_loader.js:40-44)
            a = c + rng.normal(size=3) * 0.3
            tri = [c, a, a]
        elif kind == 1:    # sliver
            a = c + rng.normal(size=3)
            tri = [c, a, a + rng.normal(size=3) * 1e-5]
        elif kind == 2:    # huge
            tri = [c * 50, c * 50 + rng.normal(size=3) * 40, c * 50 + rng.normal(size=3) * 40]
        else:
            tri = [c, c + rng.normal(size=3) * 0.8, c + rng.normal(size=3) * 0.8]
        base = len(lines) // 1
        for v in tri:
            lines.append("v %.9g %.9g %.9g" % tuple(v))
        faces.append((k, "f %d %d %d" % (3 * k + 1, 3 * k + 2, 3 * k + 3)))
        if kind == 3:      # duplicate of the same triangle (equal t: first-visited wins)
            faces.append((k, "f %d %d %d" % (3 * k + 1, 3 * k + 2, 3 * k + 3)))
    mats = ["m%d" % i for i in range(int(rng.integers(1, 5)))]
    obj = ["mtllib lib.mtl"] + lines
    for k, f in faces:
        obj += ["usemtl " + mats[k % len(mats)], f]
    mtl = []
    for m in mats:
        mtl += ["newmtl " + m, "Kd %.3f %.3f %.3f" % tuple(rng.uniform(0.05, 1, 3)),
                "Pmr %.3f %.3f 0" % (float(rng.choice([0, 0, 1, 0.5])), float(rng.uniform(0.02, 1)))]
        if rng.random() < 0.3:
            mtl += ["dielectric %.3f" % rng.uniform(0.1, 2), "ior %.3f" % rng.uniform(1.05, 2.2)]
        if rng.random() < 0.4:
            mtl += ["Kem %.3f %.3f %.3f" % tuple(rng.uniform(0, 1, 3))]
    prop = {"path": "f/soup.obj", "scale": float(rng.uniform(0.3, 1.5)), "rotate": [{"angle": float(rng.uniform(0, 6)), "axis": [0, 1, 0]}],
            "translate": [float(x) for x in rng.normal(size=3) * 0.2], "emittance": [0, 0, 0],
            "normals": str(rng.choice(["flat", "smooth"]))}
    floor = {"path": "q.obj", "scale": 8, "rotate": [], "translate": [0, -2.0, 0], "emittance": [0, 0, 0], "normals": "flat",
             "diffuse": [0.6, 0.6, 0.6]}
    env = None
    ew = eh = 0
    if rng.random() < 0.7:
        ew, eh = int(rng.integers(2, 40)), int(rng.integers(2, 24))
        env = rng.integers(0, 256, size=(eh, ew, 4), dtype=np.uint8)
        env[..., 3] = rng.integers(118, 134, size=(eh, ew))  # exponents around 2^0
    arrays = S.build_scene([prop, floor], {"f/soup.obj": "\n".join(obj) + "\n", "q.obj": S.QUAD_OBJ}, env=env, env_w=ew, env_h=eh,
                           leaf_size=int(rng.choice([1, 2, 4, 4, 5])), mtl_texts={"f/lib.mtl": "\n".join(mtl) + "\n"})
    cam = dict(P=[float(x) for x in rng.normal(size=3) * 2 + [0, 0.5, 3]], I=[float(x) for x in (rng.normal(size=3) * 0.3 + [0, -0.1, -1])],
               fov_scale=float(rng.uniform(0.2, 1.2)), env_theta=float(rng.uniform(0, 6)),
               lens=[float(rng.uniform(-0.5, 0.9)), float(rng.choice([0.0, 0.02, 0.3]))])
    return arrays, cam, int(rng.integers(1, 7)), (int(rng.integers(1, 90)), int(rng.integers(1, 60))), int(rng.integers(1, 2 ** 31))


def chain_scene(n_leaves, env_from):
    """A chain-shaped BVH of depth n_leaves - 1 in the reference layout (pre-order; interior i: left = a one-triangle
    leaf, right = the next interior), small randomly placed triangles along +x, flat normals, a grey diffuse material
    and the environment (incl. importance bins) of `env_from`."""
    from fspt_amd import scene as S
    rng = np.random.default_rng(n_leaves)
    tri = np.zeros((n_leaves, 3, 3), np.float32)
    for k in range(n_leaves):
        c = np.array([k, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
        tri[k] = c + rng.uniform(-0.9, 0.9, (3, 3)) * [0.3, 1, 1]  # boxes overlap the chain's axis: rays along it visit every level
    lo = tri.min(1); hi = tri.max(1)
    n_nodes = 2 * n_leaves - 1
    bvh = np.zeros((n_nodes, 9), np.float32)
    iv = bvh.view(np.int32)
    idx = 0
    for i in range(n_leaves - 1):  # interior i (covers leaves i..), then its left child: leaf i
        iv[idx, 0] = idx + 1; iv[idx, 1] = idx + 2; iv[idx, 2] = -1
        bvh[idx, 3:6] = lo[i:].min(0); bvh[idx, 6:9] = hi[i:].max(0)
        idx += 1
        iv[idx, 0] = 0; iv[idx, 1] = 0; iv[idx, 2] = i
        bvh[idx, 3:6] = lo[i]; bvh[idx, 6:9] = hi[i]
        idx += 1
    iv[idx, 0] = 0; iv[idx, 1] = 0; iv[idx, 2] = n_leaves - 1
    bvh[idx, 3:6] = lo[-1]; bvh[idx, 6:9] = hi[-1]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = tri[:, 1] - tri[:, 0]
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    bit = np.cross(nrm, tan)
    norm = np.zeros((n_leaves, 3, 3, 3), np.float32)  # per vertex: n, t, bt
    norm[:, :, 0] = nrm[:, None]; norm[:, :, 1] = tan[:, None]; norm[:, :, 2] = bit[:, None]
    mat = np.zeros((n_leaves, 12), np.float32)
    mat[:, 0:4] = [0, 1, 2, 3]   # diffuse / emissive / normal / metallic-roughness layers
    mat[:, 9:11] = [1.4, -1.0]   # ior, dielectric
    atlas = np.array([[200, 190, 180, 255], [0, 0, 0, 255], [128, 128, 255, 255], [0, 140, 0, 255]], np.uint8)
    return S.SceneArrays(bvh=bvh.reshape(-1), tri=tri.reshape(-1), mat=mat.reshape(-1), norm=norm.reshape(-1),
                         uv=np.zeros(n_leaves * 6, np.float32), atlas=atlas.reshape(-1), atlas_res=1, atlas_layers=4,
                         env=env_from.env, env_w=env_from.env_w, env_h=env_from.env_h, bins=env_from.bins)
