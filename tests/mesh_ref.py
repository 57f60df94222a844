"""numpy float64 restatement of the vertex-position update (fspt_scene_update_vertices): obj_loader.js's normal
rules - getNormal, averageNormals, calcTangents with its isNaN quirk - as scene_build.cpp states them, operation by operation
in the reference's order, one float64 -> float32 conversion per output.  The summation order of a vertex normal is explicit:
round k adds the k'th incident face (ascending rank) of every vertex that has one; nothing here uses np.add.at.  The quirk
is NOT the kernel's closed form: triangles whose test fires are replayed with Python lists, push and assign as the JS does."""
import numpy as np

STATIC = 0xFFFFFFFF
EPS = 2.220446049250313e-16  # Number.EPSILON


def _sub(a, b):
    return a - b


def _scale(a, s):
    return a * np.asarray(s)[..., None]


def _cross(a, b):  # vector.js:112-117 (note the sign form of y)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]),
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(v):  # vector.js:6-13
    m = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return _scale(v, 1.0 / m)


def uv_constants(uv):
    """(du1[1], du0[1], r) per triangle from the raw vt values [T, 6] float64 (scene_build.cpp's calcTangents)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2).copy()
    for i in range(3):
        uv[:, i, :] = uv[:, i, :] + EPS * (i + 1)
    du0 = uv[:, 1] - uv[:, 0]
    du1 = uv[:, 2] - uv[:, 0]
    with np.errstate(all="ignore"):
        r = 1.0 / ((du0[:, 0] * du1[:, 1]) - (du0[:, 1] * du1[:, 0]))
    return du1[:, 1], du0[:, 1], r


def vertex_rows(vertex, rank):
    """CSR rows vertex -> face ids, one entry per incident corner, ascending rank of the face: (offsets [nv + 1], faces)"""
    vertex = np.asarray(vertex, np.int64).reshape(-1, 3)
    T = vertex.shape[0]
    rank = np.arange(T, dtype=np.int64) if rank is None else np.asarray(rank, np.int64).reshape(-1)
    face = np.repeat(np.arange(T, dtype=np.int64), 3)
    v = vertex.reshape(-1)
    live = v != STATIC
    v, face = v[live], face[live]
    order = np.lexsort((rank[face], v))  # by vertex, then by rank; a face naming a vertex twice stays twice
    return v[order], face[order]


def mesh_ref(vertex, uv, pos, smooth=None, rank=None, rest_tri=None, rest_norm=None):
    """(tri [T, 9], norm [T, 27]) float32 for pos [n_vertices, 3] float32.  A triangle whose three indices are STATIC takes
    rest_tri / rest_norm."""
    vertex = np.asarray(vertex, np.int64).reshape(-1, 3)
    T = vertex.shape[0]
    pos32 = np.asarray(pos, np.float32).reshape(-1, 3)
    nv = pos32.shape[0]
    static = (vertex == STATIC).all(axis=1)
    assert not ((vertex == STATIC).any(axis=1) & ~static).any()
    smooth = np.zeros(T, bool) if smooth is None else np.asarray(smooth).reshape(-1).astype(bool)
    vi = np.where(vertex == STATIC, 0, vertex)
    P = pos32.astype(np.float64)[vi]  # [T, 3, 3], promoted exactly
    k0, k1, r = uv_constants(np.where(static[:, None], 0.0, np.asarray(uv, np.float64).reshape(-1, 6)))
    with np.errstate(all="ignore"):
        e1, e2 = _sub(P[:, 1], P[:, 0]), _sub(P[:, 2], P[:, 0])
        fn = _normalize(_cross(e1, e2))
        # vertex normals: total = (0,0,0) + the incident face normals in ascending rank, then total * (1 / count)
        n = np.repeat(fn[:, None, :], 3, axis=1).copy()
        if smooth.any():
            row_v, row_f = vertex_rows(vertex, rank)
            count = np.bincount(row_v, minlength=nv)
            start = np.concatenate([[0], np.cumsum(count)])[:-1]
            total = np.zeros((nv, 3), np.float64)
            for k in range(int(count.max()) if count.size else 0):
                has = np.nonzero(count > k)[0]
                total[has] = total[has] + fn[row_f[start[has] + k]]
            vn = _scale(total, 1.0 / count.astype(np.float64))
            n[smooth] = vn[vi[smooth]]
        pre = _normalize(_scale(_sub(_scale(e1, k0), _scale(e2, k1)), r))
        pt = np.repeat(pre[:, None, :], 3, axis=1)
        pre_bt = _normalize(_cross(n, pt))
        tg = _normalize(_cross(pre_bt, n))
        bt = _normalize(_cross(n, tg))
        fired = np.isnan(_dot(tg, bt))
        up = np.broadcast_to(np.array([0.0, 1.0, 0.0]), n.shape)
        ftg = _cross(n, up)
        fbt = _cross(ftg, n)
    out_t, out_b = tg.copy(), bt.copy()
    for t in np.nonzero(fired.any(axis=1) & ~static)[0]:  # obj_loader.js:87-100, literally
        tangents, bitangents = [], []

        def assign(arr, i, v):
            while len(arr) <= i:
                arr.append(np.full(3, np.nan))
            arr[i] = v

        for i in range(3):
            if fired[t, i]:
                assign(tangents, i, ftg[t, i])
                assign(bitangents, i, fbt[t, i])
            tangents.append(tg[t, i])
            bitangents.append(bt[t, i])
        for i in range(3):
            out_t[t, i], out_b[t, i] = tangents[i], bitangents[i]
    with np.errstate(all="ignore"):
        norm = np.concatenate([n, out_t, out_b], axis=2).astype(np.float32).reshape(T, 27)
    tri = pos32[vi].reshape(T, 9).copy()
    if static.any():
        tri[static] = np.asarray(rest_tri, np.float32).reshape(-1, 9)[static]
        norm[static] = np.asarray(rest_norm, np.float32).reshape(-1, 27)[static]
    return tri, norm


def same_bits_nan_by_position(a, b):
    """finite values (and infinities) bit for bit; NaNs by position only - their payloads differ between hosts and the GPU"""
    a = np.asarray(a, np.float32).reshape(-1)
    b = np.asarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- the meshes the tests share ------------------------------------------------------------------------------------
def f32repr(x):
    return repr(float(np.float32(x)))


def obj_text(positions, faces, vts=None, face_vt=None):
    """OBJ text with float32-exact `v` lines; faces = 0-based index triples; vts [m, 2] and face_vt (0-based triples) optional"""
    lines = ["v " + " ".join(f32repr(c) for c in p) for p in np.asarray(positions, np.float32)]
    if vts is not None:
        lines += ["vt %r %r" % (float(a), float(b)) for a, b in vts]
    for k, f in enumerate(faces):
        if vts is None:
            lines.append("f " + " ".join(str(i + 1) for i in f))
        else:
            lines.append("f " + " ".join("%d/%d" % (i + 1, j + 1) for i, j in zip(f, face_vt[k])))
    return "\n".join(lines) + "\n"


def hashed(n, seed):
    """n float32 values in [-1, 1) from an integer hash: the same on every host"""
    x = np.arange(n, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(33); x *= np.uint64(0xFF51AFD7ED558CCD); x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53); x ^= x >> np.uint64(33)
    return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def grid_mesh(nx, ny, seed=1, textured=True):
    """(positions, faces, vts, face_vt): an nx x ny vertex grid, jittered in z, two triangles per cell, per-vertex uvs"""
    ys, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    pos = np.stack([xs.reshape(-1) / max(nx - 1, 1), ys.reshape(-1) / max(ny - 1, 1), 0.25 * hashed(nx * ny, seed)], axis=1).astype(np.float32)
    faces = []
    for y in range(ny - 1):
        for x in range(nx - 1):
            a, b, c, d = y * nx + x, y * nx + x + 1, (y + 1) * nx + x, (y + 1) * nx + x + 1
            faces += [(a, b, d), (a, d, c)]
    vts = np.stack([pos[:, 0] * 0.75 + 0.125, pos[:, 1] * 0.5 + 0.25], axis=1).astype(np.float64) if textured else np.array([[0.5, 0.5]])
    face_vt = faces if textured else [(0, 0, 0)] * len(faces)
    return pos, faces, vts, face_vt


def fan_mesh(valence, seed=2):
    """a centre vertex (index 0) with `valence` triangles round it, on a jittered cone"""
    ang = np.arange(valence + 1) * (2.0 * np.pi / valence) * 0.97
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * hashed(valence + 1, seed).astype(np.float64)], axis=1)
    pos = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32)
    faces = [(0, 1 + k, 2 + k) for k in range(valence)]
    vts = np.stack([pos[:, 0] * 0.4 + 0.5, pos[:, 1] * 0.4 + 0.5], axis=1).astype(np.float64)
    return pos, faces, vts, faces


def strip_mesh(T, seed=3):
    """T triangles in a strip over T + 2 jittered vertices"""
    k = np.arange(T + 2)
    pos = np.stack([k * 0.5, (k % 2).astype(np.float64), 0.3 * hashed(T + 2, seed).astype(np.float64)], axis=1).astype(np.float32)
    faces = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(T)]
    vts = np.stack([pos[:, 0] * 0.01 + 0.1, pos[:, 1] * 0.5 + 0.2], axis=1).astype(np.float64)
    return pos, faces, vts, faces


def folded_pair(shared):
    """Two triangles folded flat onto each other along a shared edge, with opposite windings in space, so the face normals
    are n and -n and the mean at the shared vertices is exactly 0 (a NaN frame there); `shared` = the corner places of the
    shared edge in BOTH triangles: (1, 2) -> NaN pattern {1,2}, ends finite; (0, 1) -> pattern {0,1}, a NaN stays in the
    record.  The two free vertices coincide in space but are different vertices."""
    a, b = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    c = np.array([0.25, 1.0, 0.0])
    pos = np.array([a, b, c, c], np.float32)  # vertices 0, 1 shared; 2 and 3 the free ones
    free = ({0, 1, 2} - set(shared)).pop()
    f0, f1 = [0, 0, 0], [0, 0, 0]
    f0[shared[0]], f0[shared[1]], f0[free] = 0, 1, 2
    f1[shared[0]], f1[shared[1]], f1[free] = 1, 0, 3   # the edge run the other way: the opposite normal
    faces = [tuple(f0), tuple(f1)]
    vts = np.array([[0.1, 0.1], [0.9, 0.15], [0.3, 0.8], [0.35, 0.85]], np.float64)
    return pos, faces, vts, faces
