"""GPU part transforms in the Node host: setPose / updateTransforms on the mock library (no GPU), and against
the Python host's frame on the device."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("pose_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "pose_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "pose_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_pose_calls_reach_the_library(js_report):
    r = js_report
    assert "FSPT_E_STATE" in r["no_pose"] or "-6" in r["no_pose"] or r["no_pose"].startswith("Error")
    assert r["cost_pose"] == 3100           # max(part) + 1 = 3 parts, rest normals
    assert r["cost_updates"] == 3102        # two updates reached the library
    assert r["wrong_parts"] is not None     # 2 matrices for 3 parts: the library refuses
    assert r["cost_five"] == 5002           # nParts given, no rest normals
    assert r["cost_dropped"] == 2           # setPose(null)


def test_js_pose_argument_checks(js_report):
    r = js_report
    assert r["short_part"] == "RangeError: setPose: part must be a Uint32Array of 2 ids" == r["i32_part"]
    assert r["short_tri"] == "RangeError: setPose: tri must be a Float32Array of 2 x 9 floats" == r["no_tri"]
    assert r["short_norm"] == "RangeError: setPose: norm must be a Float32Array of 2 x 27 floats"
    assert r["few_parts"] == "RangeError: setPose: nParts must be an integer >= max(part) + 1"
    assert r["xf_len"] == "RangeError: updateTransforms: xf must be a Float32Array of n_parts x 12 floats" == r["xf_type"]
    assert r["cost_after_refused"] == r["cost_dropped"]  # nothing refused reached the library
    assert r["addon_len"].startswith("RangeError: fspt_napi: setPose needs")
    assert r["addon_xf"] == "RangeError: fspt_napi: updateTransforms needs 12 floats per part"
    assert all(e is not None and "Error" in e for e in r["target_as_scene"])


def test_js_pose_guarded_while_rendering(js_report):
    r = js_report
    assert all(e is not None and "render in flight" in e for e in r["during"])
    assert r["after"] == [None, None]
    assert all(e is not None for e in r["closed"])


@pytest.mark.gpu
def test_node_update_transforms_matches_python(tmp_path):
    import lights_ref as LR
    import pose_ref as PR
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, CAM = 64, 48, S.BUNNY_CAMERA
    e1 = LR.scene_e1()  # (no environment map: the job files stay small)
    part = (np.arange(e1.n_tris, dtype=np.uint32) * 7 // 5) % 3
    rot = S._rotation_matrix([0.0, 1.0, 0.0], 0.4)
    xf = np.stack([np.concatenate([rot * s, [[0.02 * k], [0.0], [-0.01 * k]]], 1) for k, s in enumerate((1.0, 0.8, 1.1))]).astype(np.float32)
    sc = Scene(e1)
    sc.set_pose(part, n_parts=3)
    sc.update_transforms(xf)
    got_t, got_n = sc.read_pose()
    want_t, want_n = PR.pose(part, e1.tri.reshape(-1, 9), e1.norm.reshape(-1, 27), xf)
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM); pt.seed(7); pt.render(6)
    want = pt.readRadiance()
    pt.close(); sc.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    part.tofile(os.path.join(d, "part.bin")); xf.tofile(os.path.join(d, "xf.bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=6, cam=CAM, nParts=3,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "pose_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got, want)
    assert got[..., :3].max() > 0
