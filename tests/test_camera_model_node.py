"""The camera models in the Node host against the Python host's frame on the device (the Node host's
argument checks on the mock library: tests/test_camera_model_cpu.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("model", [{"model": "equirect"}, {"model": "stereo", "ipd": 0.1}])
def test_node_set_camera_model_matches_python(tmp_path, model):
    import lights_ref as LR
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, CAM = 64, 48, S.BUNNY_CAMERA
    e1 = LR.scene_e1()  # (no environment map: the job files stay small)
    sc = Scene(e1)
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM); pt.seed(7)
    pt.set_camera_model(**model)
    pt.render(6)
    want = pt.readRadiance()
    pt.set_camera_model(None); pt.clear(); pt.seed(7); pt.render(6)
    pinhole = pt.readRadiance()
    pt.close(); sc.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=6, cam=CAM, model=model,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "camera_model_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, pinhole) and got[..., :3].max() > 0
    assert json.load(open(os.path.join(d, "model.json")))["model"] == model["model"]
