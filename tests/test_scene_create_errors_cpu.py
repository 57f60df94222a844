"""Every host-side refusal of fspt_scene_create: the code AND the full text of fspt_last_error, one rule broken at a time on a
hand-made description (three nodes, two triangles, leaf_size 4, one 2 x 2 atlas layer, one bin, no environment) - plus calls
that break two rules, which must report the one checked first - and that *out stayed NULL.  None of them needs a device: a
malformed description is FSPT_E_INVALID on a machine without a GPU too, and only the intact one gets as far as asking for one.
(texset_classify's refusal is left out: it takes single-layer images beyond 2^32 tiles.)

EXPECT is a literal table.  It was filled from a library built from the commit BEFORE fspt_scene_create moved to
fspt_scene.cpp and became named steps (tools/build_ab.sh, FSPT_LIB), never from the code under test: the order of the checks
and each text are part of its behaviour."""
import ctypes as C

import numpy as np
import pytest

from fspt_amd import _lib as L

DEEP = 65  # interior nodes of the left-leaning chain: its deepest node sits at depth 65


def tree(words):
    """(n, 9) float32 node records from (left, right, triStart) words; every box is the unit cube"""
    bvh = np.zeros((len(words), 9), np.float32)
    bvh[:, 6:9] = 1.0
    bvh.view(np.int32)[:, 0:3] = np.asarray(words, np.int32)
    return bvh


def chain(k):
    """k interior nodes 0 .. k - 1, each with the next one as its left child and a leaf as its right; leaves k .. 2k"""
    words = [(i + 1, k + i, -1) for i in range(k - 1)] + [(2 * k, 2 * k - 1, -1)] + [(-1, -1, 0)] * (k + 1)
    return tree(words)


def intact():
    return {
        "bvh": tree([(1, 2, -1), (-1, -1, 0), (-1, -1, 1)]),
        "tri": np.arange(18, dtype=np.float32).reshape(2, 9),
        "mat": np.zeros((2, 12), np.float32),
        "norm": np.zeros((2, 27), np.float32),
        "uv": np.zeros((2, 6), np.float32),
        "atlas": np.arange(16, dtype=np.uint8), "atlas_res": 2, "atlas_layers": 1,
        "env": None, "env_w": 0, "env_h": 0,
        "bins": np.array([0, 0, 1, 1], np.uint32), "n_bins": 1,
        "leaf_size": 4,
    }


def words_edit(node, word, value):
    def f(a):
        a["bvh"].view(np.int32)[node, word] = value
    return f


def put(**kw):
    return lambda a: a.update(kw)


ENV = np.zeros(8 * 4 * 4, np.uint8)
# case -> what it does to the intact description's fields (n_nodes / n_tris follow the arrays unless given)
CASES = {
    **{f"null_{k}": put(**{k: None}) for k in ("bvh", "tri", "mat", "norm", "uv")},
    "n_nodes_0": put(n_nodes=0),
    "n_tris_0": put(n_tris=0),
    "null_atlas": put(atlas=None),
    "atlas_res_0": put(atlas_res=0),
    "atlas_layers_0": put(atlas_layers=0),
    "null_bins": put(bins=None),
    "n_bins_0": put(n_bins=0),
    "env_w_0": put(env=ENV, env_w=0, env_h=4),
    "leaf_size_0": put(leaf_size=0),
    "leaf_size_65": put(leaf_size=65),
    "tri_start": words_edit(2, 2, 3),       # n_tris + 1
    "child_not_above": words_edit(0, 0, 0),
    "child_n_nodes": words_edit(0, 1, 3),
    "too_deep": put(bvh=chain(DEEP)),
    # two rules broken: the one checked first is reported
    "atlas_and_leaf_size": put(atlas_layers=0, leaf_size=0),
    "child_and_too_deep": lambda a: (a.update(bvh=chain(DEEP)), words_edit(0, 0, 0)(a)),
    "bins_and_env": put(bins=None, env=ENV, env_w=0, env_h=4),
}

# case -> (code, text).  -1 FSPT_E_INVALID, -2 FSPT_E_NO_DEVICE.
EXPECT_NULL = "fspt_scene_create: NULL argument"
# (between the brackets stands the HIP runtime's own reason, in its words)
EXPECT_NO_DEVICE = ("no HIP device available (", "); libfspt has no CPU fallback")
EXPECT = {
    "null_bvh": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "null_tri": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "null_mat": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "null_norm": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "null_uv": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "n_nodes_0": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "n_tris_0": (-1, "fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"),
    "null_atlas": (-1, "fspt_scene_create: atlas must have at least one layer"),
    "atlas_res_0": (-1, "fspt_scene_create: atlas must have at least one layer"),
    "atlas_layers_0": (-1, "fspt_scene_create: atlas must have at least one layer"),
    "null_bins": (-1, "fspt_scene_create: radianceBins must hold at least one bin (main.js:292)"),
    "n_bins_0": (-1, "fspt_scene_create: radianceBins must hold at least one bin (main.js:292)"),
    "env_w_0": (-1, "fspt_scene_create: env given with zero size"),
    "leaf_size_0": (-1, "fspt_scene_create: leaf_size 0 out of range [1,64]"),
    "leaf_size_65": (-1, "fspt_scene_create: leaf_size 65 out of range [1,64]"),
    "tri_start": (-1, "node 2: triStart 3 > n_tris 2"),
    "child_not_above": (-1, "node 0: child indices (0,2) violate pre-order / range [1,3)"),
    "child_n_nodes": (-1, "node 0: child indices (1,3) violate pre-order / range [1,3)"),
    "too_deep": (-1, "BVH depth 65 exceeds the traversal stack (64)"),
    "atlas_and_leaf_size": (-1, "fspt_scene_create: atlas must have at least one layer"),  # the atlas is checked before leaf_size
    "child_and_too_deep": (-1, "node 0: child indices (0,65) violate pre-order / range [1,131)"),  # tree_topology's refusals come before the depth's
    "bins_and_env": (-1, "fspt_scene_create: radianceBins must hold at least one bin (main.js:292)"),  # bins are checked before the environment's size
}


def create(a, null_out=False):
    """fspt_scene_create on the fields `a` -> (code, text, *out)"""
    lib = L.lib()
    d = L.SceneDesc()
    for k in ("bvh", "tri", "mat", "norm", "uv"):
        setattr(d, k, None if a[k] is None else L.fptr(a[k]))
    d.n_nodes = a.get("n_nodes", 0 if a["bvh"] is None else len(a["bvh"]))
    d.n_tris = a.get("n_tris", 0 if a["tri"] is None else len(a["tri"]))
    d.atlas = None if a["atlas"] is None else L.u8ptr(a["atlas"])
    d.env = None if a["env"] is None else L.u8ptr(a["env"])
    d.bins = None if a["bins"] is None else L.u32ptr(a["bins"])
    for k in ("atlas_res", "atlas_layers", "env_w", "env_h", "n_bins", "leaf_size"):
        setattr(d, k, a[k])
    out = C.c_void_p(0xDEAD)  # (a refusal must reset it)
    rc = lib.fspt_scene_create(C.byref(d), 0, None if null_out else C.byref(out))
    return rc, lib.fspt_last_error().decode(), out.value


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case):
    a = intact()
    CASES[case](a)
    rc, text, out = create(a)
    print(case, (rc, text))
    assert (rc, text) == EXPECT[case]
    assert out is None


def test_null_arguments():
    lib = L.lib()
    out = C.c_void_p(0xDEAD)
    assert lib.fspt_scene_create(None, 0, C.byref(out)) == -1
    assert lib.fspt_last_error().decode() == EXPECT_NULL
    rc, text, _ = create(intact(), null_out=True)
    assert (rc, text) == (-1, EXPECT_NULL)


def test_intact_description():
    """... is FSPT_E_NO_DEVICE with its text where there is no device, and a scene where there is one"""
    lib = L.lib()
    rc, text, out = create(intact())
    print((rc, text))
    if lib.fspt_device_count() > 0:
        assert rc == 0 and out
        assert lib.fspt_scene_destroy(C.c_void_p(out)) == 0
    else:
        assert rc == -2 and text.startswith(EXPECT_NO_DEVICE[0]) and text.endswith(EXPECT_NO_DEVICE[1])
        assert out is None
