"""Adversarial triangle soups for the binned-SAH builder (fspt_bvh_build.hip) and the way the tests feed them.

Every generator is deterministic, returns finite float32 vertices [n, 9] and aims at one path of the builder that a
regular mesh never takes: nodes above SMALL = 1024 triangles (the level-synchronous kernels) that split at the median,
chunk edges (CHUNK = 4096), the depth guard at 63 on the device, and extents that are zero, denormal or infinite.
tests/test_bvh_soups_cpu.py asserts on the numpy restatement that each soup does reach the path it is named for.

    obj_text(verts)       one OBJ, vertices printed with %.9g (float32 round-trips), three per face
    feed(verts)           a builder handle holding that OBJ with scale 1 and no normalisation (caller destroys it)
    geometry(b)           the builder's own float32 triangles [n, 9], in the order they were added
    built(b)              after a build: (bvh, tri, mat, norm, uv, order, depth)
    scene_arrays(...)     SceneArrays of a built tree with one grey diffuse material and no environment
"""
import ctypes as C

import numpy as np

SMALL, CHUNK = 1024, 4096  # fspt_bvh_build.hip
ONE = np.array([0.1, 0.2, 0.3, 0.4, 0.25, 0.3, 0.2, 0.6, 0.35], np.float32)
# (n, leaf_size) of the random clouds: a lone triangle, the leaf threshold, the block size (256), the largest finisher node
# and the first level-synchronous one, one chunk against two, and three chunks with a one-triangle tail
EDGE_CASES = sorted({(n, ls) for ls in (1, 4, 64)
                     for n in (1, 2, ls, ls + 1, 255, 256, 257, SMALL - 1, SMALL, SMALL + 1, 2 * SMALL + 1, CHUNK - 1, CHUNK,
                               CHUNK + 1, 2 * CHUNK + 1)})


def cloud(n, seed=0):
    """n ordinary triangles: Gaussian centres (sigma 1.5), Gaussian edges (sigma 0.3)"""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3)) * 1.5
    return (c + rng.normal(size=(n, 3, 3)) * 0.3).astype(np.float32).reshape(n, 9)


def coincident(n):
    """n copies of one triangle: every centroid extent is zero"""
    return np.tile(ONE, (n, 1))


def point(n):
    """n zero-area triangles at one point: every box has surface area zero as well"""
    return np.tile(np.array([0.1, 0.2, 0.3] * 3, np.float32), (n, 1))


def concentric(n, seed=0):
    """n triangles whose boxes differ but share one centre: box k = (1, 2, 3) +- (hx, hy, hz) with half-sizes that are
    multiples of 2^-10, so (min + max) * 0.5f is exactly (1, 2, 3) for each; shuffled"""
    k = np.arange(n)
    h = np.stack([(k + 1) / 1024.0, (k % 17 + 1) / 64.0, (k % 5 + 1) / 8.0], 1)
    sg = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float64)  # every axis reaches -h and +h
    v = np.array([1.0, 2.0, 3.0]) + sg[None] * h[:, None, :]
    v = v[np.random.default_rng(seed).permutation(n)]
    return v.astype(np.float32).reshape(n, 9)


def mixed(n):
    """tests/test_bvh_build_cpu.py's soup("mixed"): copies of one triangle, every 7th random, zero-area members, signed zeros"""
    rng = np.random.default_rng(1)
    v = np.tile(ONE, (n, 1))
    v[::7] = rng.normal(size=(v[::7].shape[0], 9)).astype(np.float32)
    v[1::5, 3:] = np.tile(v[1::5, :3], (1, 2))
    v[2::11] = -0.0
    return v


def nested(n=215):
    """n right triangles nested at the origin of the plane z = 0, legs 2^100 * 0.5^k: the SAH peels the largest few per
    level, a chain deeper than 63 that the guard has to cut (inside one finisher block for n <= SMALL)"""
    s = (2.0 ** 100 * 0.5 ** np.arange(n, dtype=np.float64)).astype(np.float32)
    v = np.zeros((n, 9), np.float32)
    v[:, 3] = s
    v[:, 7] = s
    return v


def guard_chain(n_cluster=9000, n_chain=57, seed=0):
    """A chain the SAH must follow one triangle per level, with a cluster of n_cluster triangles at its small end.

    Chain member m sits on axis m % 3 at 2^20 * 2^(-1.8 m): along one axis successive members shrink by 2^-5.4 < 1/32, so in
    every node the largest member is alone in the last bin of its axis and everything else shares bin 0.  Peeling that
    member is the only valid candidate.  With leaf size 1 the guard d + 1 + lv(n - 1) <= 63 refuses it at depth 49
    (lv(9000) = 14) while the node still holds the whole cluster: a node of more than two chunks with distinct centroids
    splits at the median."""
    rng = np.random.default_rng(seed)
    pos = 2.0 ** (20 - 1.8 * np.arange(n_chain))
    eps = pos[-1] * 2.0 ** -12
    chain = np.zeros((n_chain, 3, 3))
    chain[np.arange(n_chain), :, np.arange(n_chain) % 3] = pos[:, None]
    chain += rng.random((n_chain, 3, 3)) * eps
    cl = rng.random((n_cluster, 3, 3)) * eps
    v = np.concatenate([chain, cl]).reshape(-1, 9)
    return v[rng.permutation(v.shape[0])].astype(np.float32)


def scaled_cloud(log2_scale, n=3000, seed=2):
    """cloud(n) times 2^log2_scale, rounded to float32: -140 and -128 leave denormal coordinates and extents (K / e
    overflows to +inf), 120 puts box areas far above float32's range"""
    return (cloud(n, seed).astype(np.float64) * 2.0 ** log2_scale).astype(np.float32)


def halves(n=3000, seed=3):
    """two halves near x = -3e38 and x = +3e38 (jitter 1e36), ordinary in y and z: min + max overflows for every triangle,
    so the x centroids are -inf / +inf, the extent is +inf, K / e is 0 and every triangle lands in bin 0 of that axis"""
    rng = np.random.default_rng(seed)
    v = cloud(n, seed).astype(np.float64).reshape(n, 3, 3)
    side = np.where(np.arange(n) % 2 == 0, -3e38, 3e38)
    v[:, :, 0] = side[:, None] + rng.uniform(-1e36, 1e36, (n, 3))
    return v.astype(np.float32).reshape(n, 9)


def planar(n=3000, seed=4):
    """cloud(n) flattened into the plane x = 0, the zeros signed at random (-0 < +0 as keys, but the extent is 0)"""
    rng = np.random.default_rng(seed)
    v = cloud(n, seed).reshape(n, 3, 3)
    v[:, :, 0] = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0))
    return v.reshape(n, 9)


def collinear(n=3000, seed=5):
    """every vertex on the x axis (y and z are +-0): two axes without extent, every box without area, so every SAH cost
    is 0 / 0 = NaN although the centroids differ"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random((n, 3, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    v[:, :, 0] = (rng.normal(size=(n, 1)) * 1.5 + rng.normal(size=(n, 3)) * 0.3).astype(np.float32)
    return v.reshape(n, 9)


def fit(v, n):
    """v padded (cyclically) or trimmed to n triangles"""
    return np.ascontiguousarray(np.resize(v, (n, 9)))


# ---- feeding ---------------------------------------------------------------------------------------------------------
def obj_text(verts):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    n = v.shape[0] // 3
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    lines += ["f %d %d %d" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(n)]
    return "\n".join(lines) + "\n"


def feed(verts):
    from fspt_amd import _lib as L
    lib = L.lib()
    b = C.c_void_p()
    L.check(lib.fspt_builder_create(C.byref(b)))
    try:
        pd = L.PropDesc()
        pd.scale = 1.0
        text = obj_text(verts).encode()
        L.check(lib.fspt_builder_add_obj(b, text, len(text), C.byref(pd)))
    except Exception:
        lib.fspt_builder_destroy(b)
        raise
    return b


def geometry(b):
    from fspt_amd import _lib as L
    lib = L.lib()
    nt = C.c_uint32()
    L.check(lib.fspt_builder_geometry(b, C.byref(nt), None, None, None, None))
    tri = np.zeros(nt.value * 9, np.float32)
    L.check(lib.fspt_builder_geometry(b, None, L.fptr(tri), None, None, None))
    return tri.reshape(-1, 9)


def built(b):
    from fspt_amd import _lib as L
    lib = L.lib()
    nn, nt, dp = C.c_uint32(), C.c_uint32(), C.c_uint32()
    L.check(lib.fspt_builder_counts(b, C.byref(nn), C.byref(nt), C.byref(dp)))
    bvh = np.zeros(nn.value * 9, np.float32)
    tri, mat = np.zeros(nt.value * 9, np.float32), np.zeros(nt.value * 12, np.float32)
    norm, uv = np.zeros(nt.value * 27, np.float32), np.zeros(nt.value * 6, np.float32)
    L.check(lib.fspt_builder_get(b, L.fptr(bvh), L.fptr(tri), L.fptr(mat), L.fptr(norm), L.fptr(uv)))
    order = np.zeros(nt.value, np.uint32)
    L.check(lib.fspt_builder_tri_order(b, L.u32ptr(order)))
    return bvh, tri, mat, norm, uv, order, int(dp.value)


def scene_arrays(bvh, tri, norm, leaf_size, depth):
    """reference-layout arrays around a tree: one grey diffuse material (tests/rays.py chain_scene's), no environment"""
    from fspt_amd import scene as S
    n = tri.size // 9
    mat = np.zeros((n, 12), np.float32)
    mat[:, 0:4] = [0, 1, 2, 3]
    mat[:, 9:11] = [1.4, -1.0]
    atlas = np.array([[200, 190, 180, 255], [0, 0, 0, 255], [128, 128, 255, 255], [0, 140, 0, 255]], np.uint8)
    return S.SceneArrays(bvh=bvh, tri=tri, mat=mat.reshape(-1), norm=norm, uv=np.zeros(n * 6, np.float32), atlas=atlas.reshape(-1),
                         atlas_res=1, atlas_layers=4, env=None, env_w=0, env_h=0, bins=np.array([0, 0, 1, 2048], np.uint32),
                         leaf_size=leaf_size, depth=depth)
