"""fspt_builder_build_gpu and fspt_scene_rebuild_geometry on the soups of tests/bvh_soups.py: the paths of
fspt_bvh_build.hip that a regular mesh never takes.  Nodes above 1024 triangles that split at the median (no valid SAH
candidate, or the depth guard refusing one) across chunk edges; the guard at 63 on the device, in the finisher and in the
level-synchronous kernels; the sizes at which the schedule changes (leaf size, block, SMALL, CHUNK); denormal, infinite and
zero extents.  No tolerance: the tree is the numpy restatement's (tests/bvh_binned_ref.py) word for word, over the
builder's own float32 triangles, and it intersects bit-equal to the oracle and consistently with the float64 closest hit.
tests/test_bvh_soups_cpu.py asserts that every soup reaches the path it is here for."""
import functools

import numpy as np
import pytest

import bvh_binned_ref as BR
import bvh_soups as SP
import hitref as HR
import oracle as O
import rays as R
from fspt_amd import Scene, _lib as L

pytestmark = pytest.mark.gpu

SOUPS = {
    "coincident": lambda: SP.coincident(9000), "point": lambda: SP.point(9000), "concentric": lambda: SP.concentric(9000),
    "mixed5000": lambda: SP.mixed(5000), "mixed9000": lambda: SP.mixed(9000),
    "nested": SP.nested, "guard_chain": SP.guard_chain,
    "scaled-140": lambda: SP.scaled_cloud(-140), "scaled-128": lambda: SP.scaled_cloud(-128), "scaled120": lambda: SP.scaled_cloud(120),
    "halves": SP.halves, "planar": SP.planar, "collinear": SP.collinear, "collinear9000": lambda: SP.collinear(9000),
}
SOUP_CASES = ([(k, ls) for k in ("coincident", "point", "concentric") for ls in (1, 4)]
              + [("mixed5000", 4), ("mixed9000", 4), ("mixed9000", 64), ("nested", 1), ("guard_chain", 1), ("guard_chain", 4)]
              + [(k, ls) for k in ("scaled-140", "scaled-128", "scaled120") for ls in (1, 4)]
              + [("halves", 4), ("planar", 4), ("collinear", 4), ("collinear9000", 4), ("collinear9000", 1)])
GEOM = (("tri", 9), ("mat", 12), ("norm", 27), ("uv", 6))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_build(verts, leaf_size):
    """verts through one OBJ into a fresh builder, fspt_builder_build_gpu -> dict: geom (the builder's float32 triangles as
    added), geom_all (tri / mat / norm / uv as added), bvh, tri, mat, norm, uv, order, depth"""
    lib = L.lib()
    b = SP.feed(verts)
    try:
        nt = verts.shape[0]
        ga = {k: np.zeros(nt * w, np.float32) for k, w in GEOM}
        L.check(lib.fspt_builder_geometry(b, None, *(L.fptr(ga[k]) for k, _ in GEOM)))
        L.check(lib.fspt_builder_build_gpu(b, leaf_size, 0))
        bvh, tri, mat, norm, uv, order, depth = SP.built(b)
    finally:
        lib.fspt_builder_destroy(b)
    return dict(geom=ga["tri"].reshape(-1, 9), geom_all=ga, bvh=bvh, tri=tri, mat=mat, norm=norm, uv=uv, order=order, depth=depth)


@functools.lru_cache(maxsize=None)
def soup_build(name, leaf_size):
    """(the soup, its GPU build, the restatement's tree over the builder's triangles), made once per module"""
    v = SOUPS[name]()
    v.setflags(write=False)
    g = gpu_build(v, leaf_size)
    return v, g, BR.build(g["geom"], leaf_size)


def assert_is_restatement(v, g, t, leaf_size):
    assert g["geom"].shape == v.shape and np.array_equal(g["geom"], v)  # nothing flushed or rounded on the way in
    assert g["bvh"].shape == t.bvh.shape and np.array_equal(words(g["bvh"]), words(t.bvh))
    assert np.array_equal(g["order"], t.order)
    assert g["depth"] == t.depth
    o = t.order.astype(np.int64)
    for k, w in GEOM:
        assert np.array_equal(words(g[k]), words(g["geom_all"][k].reshape(-1, w)[o]).reshape(-1)), k
    BR.check_tree(g["bvh"], g["tri"], leaf_size, g["depth"])


# ---- 1: random clouds at the sizes where the schedule changes --------------------------------------------------------
@pytest.mark.parametrize("n,leaf_size", SP.EDGE_CASES)
def test_size_edges_byte_equal_to_restatement(n, leaf_size):
    v = SP.cloud(n, seed=n * 131 + leaf_size)
    g = gpu_build(v, leaf_size)
    t = BR.build(g["geom"], leaf_size)
    assert_is_restatement(v, g, t, leaf_size)
    assert (t.cnt[0] > SP.SMALL) == (n > SP.SMALL)


# ---- 2-6: the adversarial soups --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,leaf_size", SOUP_CASES)
def test_soups_byte_equal_to_restatement(name, leaf_size):
    v, g, t = soup_build(name, leaf_size)
    assert_is_restatement(v, g, t, leaf_size)
    inner = t.left >= 0
    big = inner & (t.cnt > SP.SMALL)
    print(f"\n{name} leaf {leaf_size}: {v.shape[0]} triangles, {t.cnt.size} nodes, depth {g['depth']}, SAH splits "
          f"{int(t.sah_split[inner].sum())} / {int(inner.sum())}, median splits in nodes above {SP.SMALL}: "
          f"{int((big & ~t.sah_split).sum())} / {int(big.sum())}")


def soup_arrays(name, leaf_size):
    _, g, _ = soup_build(name, leaf_size)
    return SP.scene_arrays(g["bvh"], g["tri"], g["norm"], leaf_size, g["depth"])


def ray_families(arrays, n):
    # grazing and on_surface start from a triangle that has a normal: the point and collinear soups have none
    tri = arrays.tri.reshape(-1, 3, 3).astype(np.float64)
    flat = not np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).any()
    return R.all_families(arrays, 3, n, tuple(f for f in R.FAMILIES if not (flat and f in (R.grazing, R.on_surface))))


@pytest.mark.parametrize("name,leaf_size", [("coincident", 4), ("point", 4), ("concentric", 4), ("concentric", 1), ("nested", 1),
                                            ("guard_chain", 1), ("scaled-140", 4), ("scaled-128", 1)])
def test_intersect_on_soup_trees(name, leaf_size):
    """the tree is traversable, not merely as specified: a 63-deep one is what the traversal stack was sized for"""
    arrays = soup_arrays(name, leaf_size)
    sc = Scene(arrays)  # fspt_scene_create accepts the depth
    try:
        assert sc.depth == arrays.depth
        if name in ("nested", "guard_chain", "scaled-140", "scaled-128"):
            assert sc.depth == BR.MAX_DEPTH
        walked = 0
        for rays, fam in ray_families(arrays, 200):
            rt, ridx, rsteps, rleaves = O.intersect(arrays, rays)
            t, idx, steps, leaves = sc.intersect(rays)
            assert np.array_equal(idx, ridx) and np.array_equal(words(t), words(rt)), fam
            assert np.array_equal(steps, rsteps) and np.array_equal(leaves, rleaves), fam
            ref = HR.classify(arrays, rays)
            bad = ref.mismatches(t, idx)
            assert not bad, f"{fam}: " + "; ".join(ref.describe(i, t, idx) for i in bad[:3])
            walked = max(walked, int(steps.max()))
        assert walked > arrays.n_nodes // 4  # some ray did go down the tree
    finally:
        sc.close()


# ---- repeatability: node ids come from an atomic counter, only the pre-order renumbering hides that -------------------
@pytest.mark.parametrize("name,leaf_size", [("coincident", 1), ("point", 4), ("concentric", 4), ("mixed5000", 4), ("mixed9000", 4),
                                            ("guard_chain", 1)])
def test_second_build_in_the_process_is_identical(name, leaf_size):
    v, g1, _ = soup_build(name, leaf_size)
    g2 = gpu_build(v, leaf_size)
    for k in ("bvh", "tri", "mat", "norm", "uv", "order"):
        assert np.array_equal(words(g1[k]), words(g2[k])), k
    assert g1["depth"] == g2["depth"]


# ---- rebuild in place ------------------------------------------------------------------------------------------------
REBUILD_SOUPS = {
    "coincident": SP.coincident, "point": SP.point, "concentric": SP.concentric, "mixed": SP.mixed,
    "nested": lambda n: SP.fit(SP.nested(), n), "guard_chain": lambda n: SP.guard_chain(n - 57),
    "scaled-140": lambda n: SP.fit(SP.scaled_cloud(-140), n), "collinear": SP.collinear,
}


@functools.lru_cache(maxsize=None)
def base_arrays(n):
    """a scene of n ordinary triangles, leaf size 4, from the GPU builder"""
    g = gpu_build(SP.cloud(n, seed=n), 4)
    return SP.scene_arrays(g["bvh"], g["tri"], g["norm"], 4, g["depth"])


def assert_same_scene(A, B, families):
    assert A.depth == B.depth
    assert A.two_level_nodes() == B.two_level_nodes()
    assert np.array_equal(words(np.float64([A.sah_cost()])), words(np.float64([B.sah_cost()])))  # (NaN on a soup without area)
    for rays, fam in families:
        ha, hb = A.intersect(rays), B.intersect(rays)
        for k, what in enumerate(("t", "index", "steps", "leaves")):
            assert np.array_equal(words(ha[k]), words(hb[k])), (fam, what)


@pytest.mark.parametrize("n", [5000, 9000])
@pytest.mark.parametrize("name", sorted(REBUILD_SOUPS))
def test_rebuild_with_soups_equals_fresh_build(name, n):
    """rebuild_geometry, host-pointer and device form, of an n-triangle scene with a soup fitted to n: the order it returns
    and the scene it leaves are those of a fresh build of the same triangles.  The raw arrays keep their -0 vertices (the
    OBJ parser does not), so the restatement states the fresh tree; where the soup has no -0 the GPU builder is asked too."""
    import torch
    base = base_arrays(n)
    tri = REBUILD_SOUPS[name](n)
    assert tri.shape == (n, 9)
    t = BR.build(tri, 4)
    o = t.order.astype(np.int64)
    fresh = SP.scene_arrays(t.bvh, np.ascontiguousarray(tri[o]).reshape(-1),
                            np.ascontiguousarray(base.norm.reshape(-1, 27)[o]).reshape(-1), 4, t.depth)
    if not (words(tri) == 0x80000000).any():
        g = gpu_build(tri, 4)
        assert np.array_equal(words(g["bvh"]), words(t.bvh)) and np.array_equal(g["order"], t.order) and g["depth"] == t.depth
        assert np.array_equal(words(g["tri"]), words(fresh.tri))
    families = ray_families(fresh, 64)
    flat = np.ascontiguousarray(tri).reshape(-1)
    A, D, B = Scene(base), Scene(base), Scene(fresh)
    try:
        oa = A.rebuild_geometry(flat)
        assert oa.dtype == np.uint32 and np.array_equal(oa, t.order)
        od = D.rebuild_geometry(torch.from_numpy(flat).to("cuda:0"))
        assert od.is_cuda and np.array_equal(od.cpu().numpy(), o)
        assert_same_scene(A, B, families)
        assert_same_scene(D, B, families)
    finally:
        A.close(); D.close(); B.close()
