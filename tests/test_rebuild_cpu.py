"""In-place BVH rebuild (fspt_scene_rebuild_geometry), the part that needs no GPU: the entry points exist and
check their arguments, the restatement the GPU tests compare against (tests/rebuild_ref.py on tests/bvh_binned_ref.py) is
idempotent and yields refittable trees, the parse-order map survives a rebuild, and the Node host forwards the call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bvh_binned_ref as B
import lights_ref as LR
import rebuild_ref as RB
import refit_ref as R
from refit_moves import rotated, sine
from fspt_amd import _lib as L
from fspt_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fspt_scene_rebuild_geometry", "fspt_scene_rebuild_geometry_device")


@pytest.fixture(scope="module")
def scenes(small_scene, medium_scene):
    """the GPU tests' scenes; "gpu" stands for a tree the binned builder made: here from the restatement itself"""
    sm = small_scene
    return {"small": sm, "medium": medium_scene, "textured": S.textured_test_scene(), "lights": LR.scene_e1(),
            "gpu": RB.expected(sm, sm.tri)[1]}


def test_entry_points_exist_and_check_their_arguments(small_scene):
    hdr = open(os.path.join(ROOT, "include", "fspt.h")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/fspt.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    for name in ("fspt_multi_rebuild_geometry", "fspt_scene_last_rebuild_ms"):
        assert name in L.SIGNATURES and hasattr(raw, name), name
    lib = L.lib()
    tri = np.ascontiguousarray(small_scene.tri)
    order = np.zeros(small_scene.n_tris, np.uint32)
    assert lib.fspt_scene_rebuild_geometry(None, L.fptr(tri), None, L.u32ptr(order)) == -1
    assert lib.fspt_scene_rebuild_geometry_device(None, None, None, None) == -1
    assert lib.fspt_multi_rebuild_geometry(None, L.fptr(tri), None, None) == -1
    assert lib.fspt_scene_last_rebuild_ms(None, None, None, None, None, None) == -1
    assert b"NULL" in lib.fspt_last_error()


@pytest.mark.parametrize("name", ("small", "medium", "textured", "lights", "gpu"))
def test_restatement_is_idempotent(scenes, name):
    """Consequence (a) of the rule: building again over triangles that already stand in a binned tree's leaf order is the
    identity - every stable partition finds its input partitioned - so order = arange and the same bvh words and boxes."""
    a = scenes[name]
    t1 = B.build(a.tri, a.leaf_size)
    tri1 = a.tri.reshape(-1, 9)[t1.order.astype(np.int64)]
    t2 = B.build(tri1, a.leaf_size)
    assert np.array_equal(t2.order, np.arange(a.n_tris, dtype=np.uint32))
    assert t2.bvh.tobytes() == t1.bvh.tobytes() and t2.depth == t1.depth


@pytest.mark.parametrize("move", ("rotate", "sine10"))
@pytest.mark.parametrize("name", ("small", "textured", "lights"))
def test_expected_arrays_are_a_refittable_binned_tree(scenes, name, move):
    a = scenes[name]
    tri, norm = rotated(a.tri, a.norm) if move == "rotate" else (sine(a.tri, 0.1), None)
    order, fresh = RB.expected(a, tri, norm)
    assert np.array_equal(np.sort(order), np.arange(a.n_tris))
    B.check_tree(fresh.bvh, fresh.tri, a.leaf_size, fresh.depth)
    assert R.refittable(fresh.bvh, a.n_tris)
    # the refit rule reproduces the builder's boxes byte for byte: the rebuild needs no box from the builder
    assert R.refit(fresh.bvh, fresh.tri).tobytes() == fresh.bvh.tobytes()
    o = order.astype(np.int64)
    assert np.array_equal(fresh.tri.reshape(-1, 9), tri.reshape(-1, 9)[o])
    assert np.array_equal(fresh.mat.reshape(-1, 12), a.mat.reshape(-1, 12)[o])
    assert np.array_equal(fresh.uv.reshape(-1, 6), a.uv.reshape(-1, 6)[o])
    assert np.array_equal(fresh.norm.reshape(-1, 27), (a.norm if norm is None else norm).reshape(-1, 27)[o])
    # and applying it twice composes
    order2, fresh2 = RB.expected(fresh, fresh.tri)
    assert np.array_equal(order2, np.arange(a.n_tris)) and fresh2.bvh.tobytes() == fresh.bvh.tobytes()


def test_compose_order_round_trip():
    """parse order -> leaf order -> rebuilt leaf order: the composed map fetches the right triangles"""
    texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ}
    env, ew, eh = S.synthetic_env(64, 32)
    a = S.build_scene(S.bunny_props(), texts, env=env, env_w=ew, env_h=eh, keep_order=True)
    base = a.meta["tri_order"]
    parse_tri = np.zeros_like(a.tri).reshape(-1, 9); parse_tri[base] = a.tri.reshape(-1, 9)
    moved = sine(parse_tri.reshape(-1), 0.1)                      # what a host holds: parse order
    leaf_tri, _ = S.geometry_in_leaf_order(a, moved)
    order, fresh = RB.expected(a, leaf_tri)
    assert not np.array_equal(order, np.arange(a.n_tris))
    comp = S.compose_order(base, order)
    got, none = S.geometry_in_leaf_order(comp, moved)
    assert none is None and np.array_equal(got, fresh.tri)
    # a second rebuild composes on top of the first
    moved2 = rotated(moved, a.norm)[0]
    order2, fresh2 = RB.expected(fresh, S.geometry_in_leaf_order(comp, moved2)[0])
    assert np.array_equal(S.geometry_in_leaf_order(S.compose_order(comp, order2), moved2)[0], fresh2.tri)
    with pytest.raises(ValueError):
        S.compose_order(base, order[:-1])


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("rebuild_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "rebuild_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "rebuild_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_rebuild_geometry_handles(js_report):
    """The Node host's rebuildGeometry on the mock library: the calls reach the library (with and without normals) and the
    order comes back as a Uint32Array, bad arrays are refused before it, the scene handle is guarded while a renderAsync
    runs on its target, and wrong or destroyed handles are refused."""
    r = js_report
    assert (r["cost0"], r["cost1"], r["cost2"]) == (100, 110, 140)
    assert r["order"] == [1, 0] and r["order_type"] == "Uint32Array"
    assert r["short_tri"] == "RangeError: rebuildGeometry: tri must be a Float32Array of 2 x 9 floats"
    assert r["f64_tri"] == r["short_tri"]
    assert r["short_norm"] == "RangeError: rebuildGeometry: norm must be a Float32Array of 2 x 27 floats"
    assert r["cost_after_refused"] == 140
    assert r["addon_len"].startswith("RangeError: fspt_napi: rebuildGeometry needs 9 floats")
    assert r["addon_type"].startswith("TypeError: fspt_napi: expected a TypedArray")
    assert "handle" in r["target_as_scene"]
    assert r["during"] == "Error: render in flight"
    assert r["after"] is None
    assert "destroyed" in r["closed"]
