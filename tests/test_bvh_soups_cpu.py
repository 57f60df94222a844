"""CPU checks of tests/bvh_soups.py on the numpy restatement alone: every soup reaches the path of the builder it is named
for.  tests/test_bvh_build_edges_gpu.py builds the same soups on the device; these keep a later change to a generator from
silently emptying one of its cases."""
import numpy as np
import pytest

import bvh_binned_ref as BR
import bvh_soups as SP
import oracle as O
from fspt_amd import _lib as L
from test_bvh_build_cpu import soup

FLT_MIN = np.float32(1.1754944e-38)  # the smallest normal float32


def tree(v, leaf_size, **kw):
    t = BR.build(v, leaf_size, **kw)
    BR.check_tree(t.bvh, v[t.order], leaf_size, t.depth)
    return t


def centroid_extents(v, t):
    """float32 [n_nodes, 3]: the centroid extent the split of every node saw (cmax - cmin, as the builder forms it)"""
    _, cent = BR.prims(v)
    ck = BR.key(cent)[t.order.astype(np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([BR.unkey(ck[lo:lo + n].max(0)) - BR.unkey(ck[lo:lo + n].min(0)) for lo, n in zip(t.lo, t.cnt)])


GENERATORS = {"cloud": lambda: SP.cloud(300, 7), "coincident": lambda: SP.coincident(300), "point": lambda: SP.point(300),
              "concentric": lambda: SP.concentric(300), "mixed": lambda: SP.mixed(300), "nested": SP.nested,
              "guard_chain": lambda: SP.guard_chain(300), "scaled-140": lambda: SP.scaled_cloud(-140, 300),
              "scaled120": lambda: SP.scaled_cloud(120, 300), "halves": lambda: SP.halves(300), "planar": lambda: SP.planar(300),
              "collinear": lambda: SP.collinear(300)}


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_generators_are_finite_and_seeded(name):
    v, w = GENERATORS[name](), GENERATORS[name]()
    assert v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 9 and v.flags.c_contiguous
    assert np.isfinite(v).all()
    assert np.array_equal(v.view(np.uint32), w.view(np.uint32))


def test_mixed_is_the_existing_recipe():
    for n in (20, 1000):
        assert np.array_equal(SP.mixed(n).view(np.uint32), soup("mixed", n).view(np.uint32))
    assert np.array_equal(SP.coincident(10), soup("coincident", 10)) and np.array_equal(SP.point(10), soup("point", 10))


def test_fit_pads_and_trims():
    v = SP.nested()
    assert np.array_equal(SP.fit(v, 100), v[:100])
    p = SP.fit(v, 500)
    assert p.shape == (500, 9) and np.array_equal(p[:215], v) and np.array_equal(p[215:430], v) and np.array_equal(p[430:], v[:70])


@pytest.mark.parametrize("name", ["mixed", "scaled-140", "halves", "planar", "nested"])
def test_obj_round_trip_keeps_the_values(name):
    """%.9g through the builder's OBJ parser with scale 1: every float32 comes back as it went in (denormals and 3e38
    included); only the sign of a zero is lost, so -0 keys reach the device through rebuild_geometry alone"""
    v = GENERATORS[name]()
    b = SP.feed(v)
    try:
        g = SP.geometry(b)
    finally:
        L.lib().fspt_builder_destroy(b)
    assert g.shape == v.shape and np.array_equal(g, v)
    nz = v != 0
    assert np.array_equal(g.view(np.uint32)[nz], v.view(np.uint32)[nz])


# ---- case 2: large nodes without any SAH split -----------------------------------------------------------------------
@pytest.mark.parametrize("leaf_size", [1, 4])
@pytest.mark.parametrize("kind", ["coincident", "point", "concentric"])
def test_large_degenerate_soups_split_at_the_median_only(kind, leaf_size):
    v = getattr(SP, kind)(9000)
    t = tree(v, leaf_size)
    assert not t.sah_split.any()
    assert t.depth == BR.levels_below(9000, leaf_size) == (14 if leaf_size == 1 else 12)
    # the root's 4500 / 4500 cut lies inside the second of three chunks
    assert t.cnt[t.left[0]] == 4500 and SP.CHUNK < 4500 < 2 * SP.CHUNK < 9000 <= 3 * SP.CHUNK
    big = (t.left >= 0) & (t.cnt > SP.SMALL)
    assert big.sum() == 15
    assert not centroid_extents(v, t).any()
    if kind == "concentric":
        bk, _ = BR.prims(v)
        assert np.unique(bk, axis=0).shape[0] == 9000  # the boxes do differ


# ---- case 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5000, 9000])
def test_mixed_large_soup_has_both_kinds_of_split_in_large_nodes(n):
    v = SP.mixed(n)
    t = tree(v, 4)
    big = (t.left >= 0) & (t.cnt > SP.SMALL)
    assert (big & t.sah_split).any() and (big & ~t.sah_split).any()
    assert (v.view(np.uint32) == 0x80000000).any()                    # -0 keys
    assert (v[1::5, :3] == v[1::5, 3:6]).all() and t.cnt.min() >= 1   # zero-area members; no empty leaf


# ---- case 4: the guard inside one finisher block ---------------------------------------------------------------------
def test_nested_chain_is_cut_by_the_guard_at_63():
    v = SP.nested()
    assert v.shape[0] == 215 <= SP.SMALL
    free = BR.build(v, 1, max_depth=10 ** 6)
    assert free.depth > BR.MAX_DEPTH and free.sah_split[free.left >= 0].all()
    t = tree(v, 1)
    assert t.depth == BR.MAX_DEPTH == 63
    assert (~t.sah_split[t.left >= 0]).sum() >= 1
    # some ray walks the whole tree, the 63-deep part included: traversing it means something
    a = SP.scene_arrays(t.bvh, np.ascontiguousarray(v[t.order]).reshape(-1), np.zeros(v.shape[0] * 27, np.float32), 1, t.depth)
    import rays as R
    steps = np.concatenate([O.intersect(a, rays)[2] for rays, _ in R.all_families(a, 3, 200)])
    assert steps.max() == a.n_nodes


# ---- case 5: the guard refuses the split of a multi-chunk node whose centroids differ ---------------------------------
@pytest.mark.parametrize("leaf_size", [1, 4])
def test_guard_chain_falls_back_in_a_large_node_with_distinct_centroids(leaf_size):
    v = SP.guard_chain()
    t = tree(v, leaf_size)
    ext = centroid_extents(v, t)
    hit = (t.left >= 0) & (t.cnt > SP.SMALL) & ~t.sah_split & (ext != 0).any(1)
    assert hit.any()
    assert t.depth == BR.MAX_DEPTH
    assert BR.build(v, leaf_size, max_depth=10 ** 6).depth > BR.MAX_DEPTH  # it is the guard that refuses, not the SAH
    # the first refusal is deep in the level-synchronous part and spans more than two chunks
    first = np.flatnonzero(hit)[0]
    assert t.node_depth[first] >= 45 and t.cnt[first] > 2 * SP.CHUNK
    # and above it every level peels exactly one triangle
    above = np.flatnonzero((t.left >= 0) & (t.node_depth < t.node_depth[first]) & (t.cnt > SP.SMALL))
    assert t.sah_split[above].all() and (np.minimum(t.cnt[t.left[above]], t.cnt[t.right[above]]) == 1).all()


def test_collinear_soup_has_no_finite_cost_anywhere():
    """the other way into the same branch: centroids differ, but every box area is 0, so every cost is 0 / 0"""
    v = SP.collinear(9000)
    t = tree(v, 4)
    ext = centroid_extents(v, t)
    assert not t.sah_split.any()
    big = (t.left >= 0) & (t.cnt > SP.SMALL)
    assert big.sum() == 15 and (ext[big, 0] > 0).all() and not ext[:, 1:].any()


# ---- case 6 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_scale", [-140, -128])
@pytest.mark.parametrize("leaf_size", [1, 4])
def test_tiny_soups_have_denormal_extents_and_reach_the_guard(log2_scale, leaf_size):
    v = SP.scaled_cloud(log2_scale)
    assert (np.abs(v[v != 0]) < FLT_MIN).any()
    t = tree(v, leaf_size)
    ext = centroid_extents(v, t)
    inner = t.left >= 0
    den = inner[:, None] & (ext > 0) & (ext < FLT_MIN)
    assert den.any()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(BR.K) / ext[den]).all()  # K / e overflows
    assert t.depth == BR.MAX_DEPTH and not t.sah_split[inner].all()
    if log2_scale == -140:
        assert den[0].all()  # at the root already, on every axis


def test_huge_soup_is_split_by_the_sah_everywhere():
    for leaf_size, depth in ((1, 16), (4, 14)):
        v = SP.scaled_cloud(120)
        t = tree(v, leaf_size)
        assert t.sah_split[t.left >= 0].all() and t.depth == depth
        # the same tree as the unscaled soup's: scaling by a power of two changes no decision
        u = BR.build(SP.scaled_cloud(0), leaf_size)
        assert np.array_equal(t.order, u.order) and np.array_equal(t.left, u.left)


def test_halves_soup_has_an_infinite_root_extent():
    v = SP.halves()
    t = tree(v, 4)
    ext = centroid_extents(v, t)
    assert ext[0, 0] == np.inf and np.isfinite(ext[0, 1:]).all()
    _, cent = BR.prims(v)
    assert np.isinf(cent[:, 0]).all() and (cent[:, 0] > 0).sum() == 1500
    # bin 0 for every triangle on that axis: the root can only be split on y or z
    with np.errstate(invalid="ignore"):
        assert not BR.bin_of(cent[:, 0], np.float32(-np.inf), np.float32(BR.K) / ext[0, 0]).any()
    assert t.sah_split[0] and t.sah_split[t.left >= 0].all()


def test_planar_and_collinear_soups_have_axes_without_extent():
    v = SP.planar()
    assert (v.reshape(-1, 3)[:, 0] == 0).all() and {0, 0x80000000} == set(np.unique(v.reshape(-1, 3)[:, 0].view(np.uint32)).tolist())
    t = tree(v, 4)
    ext = centroid_extents(v, t)
    assert not ext[:, 0].any() and (ext[0, 1:] > 0).all() and t.sah_split[t.left >= 0].all()
    v = SP.collinear()
    ext = centroid_extents(v, tree(v, 4))
    assert not ext[:, 1:].any() and ext[0, 0] > 0


# ---- case 1: the sizes at which the schedule changes -----------------------------------------------------------------
def test_size_edges_cover_the_schedule():
    for ls in (1, 4, 64):
        sizes = {n for n, l in SP.EDGE_CASES if l == ls}
        assert {1, 2, ls, ls + 1, 255, 256, 257, SP.SMALL - 1, SP.SMALL, SP.SMALL + 1, 2049, SP.CHUNK - 1, SP.CHUNK, SP.CHUNK + 1,
                2 * SP.CHUNK + 1} <= sizes
