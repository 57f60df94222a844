"""GPU skinning in the Node host: setSkin / updateSkin on the mock library (no GPU), and against the Python
host's frame on the device."""
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
    d = str(tmp_path_factory.mktemp("skin_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "skin_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "skin_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_skin_calls_reach_the_library(js_report):
    r = js_report
    assert r["no_skin"] is not None and r["no_skin"].startswith("Error")
    assert r["cost_skin"] == 30100            # max(joints) + 1 = 3 joints, rest normals
    assert r["cost_updates"] == 30102         # two updates reached the library
    assert r["wrong_joints"] is not None      # 2 matrices for 3 joints: the library refuses
    assert r["wrong_morph"] is not None       # 2 morph weights for no targets
    assert r["cost_morph"] == 3002152         # nJoints given, two targets with frames
    assert r["cost_morph_update"] == 3002153
    assert r["missing_weights"] is not None   # a skin with targets needs their weights
    assert r["cost_no_norm"] == 32003
    assert r["cost_dropped"] == 3             # setSkin(null)


def test_js_skin_argument_checks(js_report):
    r = js_report
    assert r["short_joints"] == "RangeError: setSkin: joints must be a Uint16Array of 2 x 12 ids" == r["u32_joints"]
    assert r["short_weights"] == "RangeError: setSkin: weights must be a Float32Array of 2 x 12 floats" == r["no_weights"]
    assert r["short_tri"] == "RangeError: setSkin: tri must be a Float32Array of 2 x 9 floats" == r["no_tri"]
    assert r["short_norm"] == "RangeError: setSkin: norm must be a Float32Array of 2 x 27 floats"
    assert r["odd_morph"] == "RangeError: setSkin: morph must be a Float32Array of nMorph x 2 x 9 floats"
    assert r["many_morph"] == "RangeError: setSkin: at most 64 morph targets, got 65"
    assert r["short_morph_norm"] == "RangeError: setSkin: morphNorm must be a Float32Array of 2 x 2 x 27 floats"
    assert r["morph_norm_alone"] == "RangeError: setSkin: morphNorm must be a Float32Array of 0 x 2 x 27 floats"
    assert r["morph_norm_no_norm"] == "RangeError: setSkin: morphNorm needs norm"
    assert r["few_joints"] == "RangeError: setSkin: nJoints must be an integer in [max(joints) + 1, 65535]" == r["many_joints"]
    assert r["xf_len"] == "RangeError: updateSkin: xf must be a Float32Array of n_joints x 12 floats" == r["xf_type"]
    assert r["mw_type"] == "RangeError: updateSkin: morphWeights must be a Float32Array of n_morph floats"
    assert r["cost_after_refused"] == r["cost_dropped"]  # nothing refused reached the library
    assert r["addon_len"].startswith("RangeError: fspt_napi: setSkin needs 12 ids")
    assert r["addon_morph"].startswith("RangeError: fspt_napi: setSkin needs 9 floats (morph)") and r["addon_morph_norm"] == r["addon_morph"]
    assert r["addon_xf"] == "RangeError: fspt_napi: updateSkin needs 12 floats per joint"
    assert all(e is not None and "Error" in e for e in r["target_as_scene"])


def test_js_skin_guarded_while_rendering(js_report):
    r = js_report
    assert all(e is not None and "render in flight" in e for e in r["during"])
    assert r["after"] == [None, None]
    assert all(e is not None for e in r["closed"])


@pytest.mark.gpu
def test_node_update_skin_matches_python(tmp_path):
    import lights_ref as LR
    import skin_ref as SR
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, CAM = 64, 48, S.BUNNY_CAMERA
    e1 = LR.scene_e1()  # (no environment map: the job files stay small)
    T = e1.n_tris
    rng = np.random.default_rng(4)
    joints = rng.integers(0, 3, (T, 3, 4)).astype(np.uint16)
    weights = rng.dirichlet(np.ones(4), (T, 3)).astype(np.float32)
    morph = rng.normal(0, 0.02, (2, T, 9)).astype(np.float32)
    mnorm = rng.normal(0, 0.05, (2, T, 27)).astype(np.float32)
    mw = np.float32([0.3, 1.0])
    rot = S._rotation_matrix([0.0, 1.0, 0.0], 0.4)
    xf = np.stack([np.concatenate([rot * s, [[0.02 * k], [0.0], [-0.01 * k]]], 1) for k, s in enumerate((1.0, 0.8, 1.1, 1.0))]).astype(np.float32)
    sc = Scene(e1)
    sc.set_skin(joints, weights, morph=morph, morph_norm=mnorm, n_joints=4)
    sc.update_skin(xf, mw)
    got_t, got_n = sc.read_skin()
    want_t, want_n = SR.skin(joints, weights, e1.tri, e1.norm, xf, morph, mnorm, mw)
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM); pt.seed(7); pt.render(6)
    want = pt.readRadiance()
    pt.close(); sc.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    for name, a in (("joints", joints), ("weights", weights), ("morph", morph), ("morph_norm", mnorm), ("mw", mw), ("xf", xf)):
        a.tofile(os.path.join(d, name + ".bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=6, cam=CAM, nJoints=4,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "skin_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got, want)
    assert got[..., :3].max() > 0
