"""In-place geometry update (fspt_scene_update_geometry), the part that needs no GPU: the numpy restatement
of the box rule (tests/refit_ref.py) is pinned to the reference's own trees, the refitted boxes are tight and nested, the
test data renders the same under the oracle whatever slack its boxes have, and the entry points exist and refuse to
compute without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import refit_ref as R
from refit_moves import rotated, sine
from fspt_amd import _lib as L
from fspt_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY_POINTS = ("fspt_scene_update_geometry", "fspt_scene_update_geometry_device", "fspt_scene_sah_cost")


def test_restated_rule_reproduces_the_reference_trees(small_scene):
    """The premise: on UNCHANGED arrays the rule gives back the boxes bvh.js (goldens) and the native builder wrote, byte
    for byte - float32 of a float64 min is the min of the float32s."""
    cases = [(n, np.load(os.path.join(GOLDEN, n + ".npz"))) for n in ("js_scene_small", "js_scene_variant", "js_scene_mtl")]
    cases = [(n, d["bvh"], d["tri"]) for n, d in cases] + [("bunny8", small_scene.bvh, small_scene.tri)]
    for name, bvh, tri in cases:
        assert R.refittable(bvh, tri.size // 9), name
        got = R.refit(bvh, tri)
        assert got.tobytes() == np.asarray(bvh, np.float32).tobytes(), name


@pytest.mark.parametrize("move", ["rotate", "sine1", "sine10"])
def test_refitted_boxes_are_tight_and_nested(small_scene, move):
    a = small_scene
    tri = {"rotate": lambda: rotated(a.tri, a.norm)[0], "sine1": lambda: sine(a.tri, 0.01), "sine10": lambda: sine(a.tri, 0.1)}[move]()
    b = R.refit(a.bvh, tri).reshape(-1, 9)
    w = b[:, :3].view(np.int32)
    v = tri.reshape(-1, 3, 3)
    leaf, first, cnt = R.ownership(b, a.n_tris)
    assert cnt.sum() == a.n_tris
    for i, f, n in zip(leaf, first, cnt):
        p = v[f:f + n].reshape(-1, 3)
        # contains every vertex, and every plane touches one (it cannot move inward)
        assert np.array_equal(b[i, 3:6], p.min(0)) and np.array_equal(b[i, 6:9], p.max(0))
    for i in np.nonzero(w[:, 2] <= -1)[0]:
        l, r = w[i, 0], w[i, 1]
        assert np.array_equal(b[i, 3:6], np.minimum(b[l, 3:6], b[r, 3:6]))
        assert np.array_equal(b[i, 6:9], np.maximum(b[l, 6:9], b[r, 6:9]))


def test_leaf_order_identity_and_oracle_ignores_box_slack(camera):
    """geometry_in_leaf_order undoes the builder's reordering; and the refitted arrays render under the oracle exactly as
    the same arrays with every box enlarged (closest hits do not depend on slack: this guards the test data)."""
    texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ}
    env, ew, eh = S.synthetic_env(64, 32)
    a = S.build_scene(S.bunny_props(), texts, env=env, env_w=ew, env_h=eh, keep_order=True)
    order = a.meta["tri_order"]
    parse_tri = np.zeros_like(a.tri).reshape(-1, 9); parse_tri[order] = a.tri.reshape(-1, 9)
    parse_norm = np.zeros_like(a.norm).reshape(-1, 27); parse_norm[order] = a.norm.reshape(-1, 27)
    tri, norm = S.geometry_in_leaf_order(a, parse_tri, parse_norm)
    assert np.array_equal(tri, a.tri) and np.array_equal(norm, a.norm)
    assert S.geometry_in_leaf_order(order, parse_tri)[1] is None
    with pytest.raises(ValueError):
        S.geometry_in_leaf_order(a, parse_tri[:-1])

    import dataclasses
    W, H = 64, 48
    moved, mnorm = rotated(a.tri, a.norm)
    tight = dataclasses.replace(a, tri=moved, norm=mnorm, bvh=R.refit(a.bvh, moved))
    slack_bvh = tight.bvh.copy().reshape(-1, 9)
    slack_bvh[:, 3:6] -= 0.125
    slack_bvh[:, 6:9] += 0.125
    slack = dataclasses.replace(tight, bvh=slack_bvh.reshape(-1))
    frames = []
    for arr in (tight, slack):
        out = np.zeros((H, W, 4), np.float32)
        O.render(arr, W, H, camera["P"], camera["I"], camera["fov_scale"], camera["lens"], camera["env_theta"], 4, 0, 4, 1, out)
        frames.append(out)
    assert np.array_equal(frames[0], frames[1])
    assert frames[0][..., :3].max() > 0


def test_sah_cost_restatement_matches_the_scene_helper(small_scene):
    assert R.sah_cost(small_scene.bvh, small_scene.n_tris) == pytest.approx(S.sah_cost(small_scene), rel=1e-15)


def test_entry_points_exist_and_refuse_without_a_device(small_scene):
    """Fails on any library without the feature: the symbols are declared, exported and bound."""
    hdr = open(os.path.join(ROOT, "include", "fspt.h")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/fspt.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert "fspt_multi_update_geometry" in L.SIGNATURES and hasattr(raw, "fspt_multi_update_geometry")
    lib = L.lib()
    tri = np.ascontiguousarray(small_scene.tri)
    cost = C.c_double()
    # argument checks come first, with or without a device
    assert lib.fspt_scene_update_geometry(None, L.fptr(tri), None) == -1
    assert lib.fspt_scene_update_geometry_device(None, None, None) == -1
    assert lib.fspt_scene_sah_cost(None, C.byref(cost)) == -1
    assert lib.fspt_multi_update_geometry(None, L.fptr(tri), None) == -1
    if lib.fspt_device_count() == 0:
        h = C.c_void_p()
        d = small_scene.desc()
        assert lib.fspt_scene_create(C.byref(d), 0, C.byref(h)) == -2  # no scene to update: no CPU fallback


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("refit_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "refit_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "refit_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_update_geometry_handles(js_report):
    """The Node host's updateGeometry / sahCost on the mock library: the calls reach the library (with and without normals),
    bad arrays are refused before it, the scene handle is guarded while a renderAsync runs on its target, and wrong or
    destroyed handles are refused."""
    r = js_report
    assert (r["cost0"], r["cost1"], r["cost2"]) == (100, 101, 104)
    assert r["short_tri"] == "RangeError: updateGeometry: tri must be a Float32Array of 2 x 9 floats"
    assert r["f64_tri"] == r["short_tri"]
    assert r["short_norm"] == "RangeError: updateGeometry: norm must be a Float32Array of 2 x 27 floats"
    assert r["cost_after_refused"] == 104
    assert r["addon_len"].startswith("RangeError: fspt_napi: updateGeometry needs 9 floats")
    assert r["addon_type"].startswith("TypeError: fspt_napi: expected a TypedArray")
    assert all(m and "handle" in m for m in r["target_as_scene"]), r["target_as_scene"]
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["after"] == [None, None]
    assert all(m and "destroyed" in m for m in r["closed"]), r["closed"]
