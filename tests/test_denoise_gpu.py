"""The guided denoiser on the MI355X: the feature pass equals the oracle's first-hit records bit for bit, the a-trous
kernel equals its float64 reference (tests/atrous_ref.py), fspt_draw_denoised equals the oracle's draw.fs, the filter
earns its place on a real frame, and nothing it does touches the existing results."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import atrous_ref as R
from fspt_amd import PathTracer, _lib as L, scene as S
from fspt_amd.tracer import DENOISE_DEFAULTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNGUIDED = dict(sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf)


def make_pt(arrays, W, H, cam, aperture=None):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"],
                  cam["aperture"] if aperture is None else aperture)
    return pt


def oracle_first_hits(arrays, W, H, pt, rand_base):
    pos, d = O.camera(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, rand_base)
    acc = np.zeros((H, W, 4), np.float32)
    return O.trace(arrays, W, H, pos, d, 0, 0.5, pt.envTheta, 4, acc, first_hits=True).reshape(H, W)


def feature_record(fh):
    """One sample's features from an oracle first-hit record (the miss values where index < 0)."""
    hit = fh["index"] >= 0
    f = np.zeros(fh.shape + (8,), np.float32)
    f[..., 0:3] = np.where(hit[..., None], fh["diffuse"], np.float32(1.0))
    f[..., 3] = np.where(hit, fh["t"], np.float32(100000.0))
    f[..., 4:7] = np.where(hit[..., None], fh["macro_normal"], np.float32(0.0))
    f[..., 7] = hit
    return f


def scenes(small):
    return {"small": small, "textured": S.textured_test_scene()}


@pytest.mark.parametrize("aperture", [None, 0.0])
@pytest.mark.parametrize("name", ["small", "textured"])
def test_features_one_sample_bitwise(small_scene, camera, name, aperture):
    arrays = scenes(small_scene)[name]
    W, H, seed = 96, 64, 11
    pt = make_pt(arrays, W, H, camera, aperture)
    pt.features(1, seed)
    got = pt.readFeatures()
    fh = oracle_first_hits(arrays, W, H, pt, O.rand_base_stream(seed, 1)[0])
    hit = fh["index"] >= 0
    assert 0 < hit.sum() < W * H  # hits and misses both present
    assert np.array_equal(got[..., 0:3][hit], fh["diffuse"][hit])
    assert np.array_equal(got[..., 4:7][hit], fh["macro_normal"][hit])
    assert np.array_equal(got[..., 3][hit], fh["t"][hit])
    assert np.array_equal(got[..., 7], hit.astype(np.float32))
    assert (got[~hit] == np.array([1, 1, 1, 100000, 0, 0, 0, 0], np.float32)).all()


@pytest.mark.parametrize("name", ["small", "textured"])
def test_features_eight_samples(small_scene, camera, name):
    """The float32 sums in sample order / 8 of the oracle's records: bit-exact (IEEE division, correctly rounded on
    both sides)."""
    arrays = scenes(small_scene)[name]
    W, H, seed, n = 80, 56, 5, 8
    pt = make_pt(arrays, W, H, camera)
    pt.features(n, seed)
    got = pt.readFeatures()
    acc = np.zeros((H, W, 8), np.float32)
    for rb in O.rand_base_stream(seed, n):
        acc = acc + feature_record(oracle_first_hits(arrays, W, H, pt, rb))
    want = acc / np.float32(n)
    assert np.array_equal(got, want)
    assert ((got[..., 7] > 0) & (got[..., 7] < 1)).any()  # some pixels have hit and missed samples (DoF, silhouettes)


def check_close(got, ref):
    big = np.abs(ref) > 1e-3
    rel = np.abs(got[big] - ref[big]) / np.abs(ref[big])
    assert rel.max() <= 1e-4, rel.max()
    assert np.abs(got[~big] - ref[~big]).max(initial=0.0) <= 1e-6


SETTINGS = [dict(), dict(iterations=1), dict(iterations=3), dict(iterations=5), dict(iterations=5, **UNGUIDED),
            dict(iterations=0)]


def test_filter_matches_reference(small_scene, camera):
    W, H = 120, 80
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(3)
    pt.render(16)
    pt.features(8, 9)
    acc, feat = pt.readRadiance(), pt.readFeatures()
    for kw in SETTINGS:
        got = pt.denoise(**kw)
        ref = R.atrous(acc, feat, **{**DENOISE_DEFAULTS, **kw})
        check_close(got, ref)
    assert np.array_equal(pt.denoise(iterations=0), acc)


def test_filter_on_bound_accumulator(small_scene, camera):
    import torch
    W, H = 100, 70
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt = make_pt(small_scene, W, H, camera)
    pt.bind_accumulator(t.data_ptr(), keep=t)
    pt.seed(4)
    pt.render(16)  # recorded into the tensor; fspt_denoise flushes first
    pt.features(8, 2)
    got = pt.denoise()
    acc = t.cpu().numpy()
    check_close(got, R.atrous(acc, pt.readFeatures(), **DENOISE_DEFAULTS))
    assert acc[..., :3].max() > 0


def test_draw_denoised_is_draw_of_the_denoised_frame(small_scene, camera):
    W, H = 96, 64
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(2)
    pt.render(8)
    pt.features(4, 3)
    den = pt.denoise(iterations=3)
    for ex, sat in ((1.0, 1.0), (2.5, 0.7)):
        assert np.array_equal(pt.drawDenoised(ex, sat), O.draw(den, ex, sat))


def test_existing_results_untouched_and_call_order(small_scene, camera):
    W, H = 96, 64
    pt = make_pt(small_scene, W, H, camera)
    # call order first: no features, no denoised frame yet
    lib = L.lib()
    buf = np.zeros((H, W, 8), np.float32)
    assert lib.fspt_read_features(pt._t, L.fptr(buf)) == -6
    assert lib.fspt_denoise(pt._t, None, None) == -6
    assert lib.fspt_draw_denoised(pt._t, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -6
    cp = L.CameraParams()
    assert lib.fspt_features(pt._t, C.byref(cp), 0, 1) == -1  # samples >= 1
    pt.seed(5)
    pt.render(6)
    before, drawn = pt.readRadiance(), pt.draw(1.3, 0.9, True, 2.0)
    pt.features(2, 7)
    for bad in (L.DenoiseParams(17, 1, 128, 0.1), L.DenoiseParams(5, -1, 128, 0.1), L.DenoiseParams(5, 1, -1, 0.1),
                L.DenoiseParams(5, 1, 128, 0.0), L.DenoiseParams(5, 1, np.inf, 0.1)):
        assert lib.fspt_denoise(pt._t, C.byref(bad), None) == -1
    assert lib.fspt_draw_denoised(pt._t, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -6
    assert lib.fspt_denoise(pt._t, None, None) == 0  # result kept on the device
    pt.drawDenoised()
    pt.denoise()
    assert pt.readRadiance().tobytes() == before.tobytes()
    assert pt.draw(1.3, 0.9, True, 2.0).tobytes() == drawn.tobytes()


# ---- quality -------------------------------------------------------------------------------------------------------
def rel_mse(x, gt, mask=None):
    e = (x[..., :3].astype(np.float64) - gt[..., :3]) ** 2 / (gt[..., :3].astype(np.float64) ** 2 + 1e-2)
    return float(e[mask].mean() if mask is not None else e.mean())


def silhouettes(depth):
    """Pixels whose 3x3 neighbourhood has a relative depth jump > 10 %."""
    H, W = depth.shape
    z = np.pad(depth, 1, mode="edge")
    jump = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q = z[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            jump |= np.abs(q - depth) > 0.1 * depth
    return jump


def quality(arrays, cam, params, W=320, H=240, gt_spp=4096, spp=16, feature_samples=8):
    pt = make_pt(arrays, W, H, cam)
    pt.seed(101)
    pt.render(gt_spp)
    gt = pt.readRadiance()
    pt.features(feature_samples, 1)
    mask = silhouettes(pt.readFeatures()[..., 3])
    pt.clear()
    pt.seed(7)
    pt.render(spp)
    raw = pt.readRadiance()
    out = {"raw": rel_mse(raw, gt), "edge_pixels": int(mask.sum())}
    for name, kw in params.items():
        den = pt.denoise(**kw)
        out[name] = rel_mse(den, gt)
        out[name + "_edge"] = rel_mse(den, gt, mask)
    pt.close()
    return out


def test_quality(medium_scene, camera):
    """320 x 240 of the medium scene, 16 spp against 4096 spp, relative MSE (error^2 / (reference^2 + 0.01)).  Measured on
    the MI355X with the shipped defaults (K 4, sigma_color 4, sigma_normal 32, sigma_depth 0.05): denoised / raw = 0.0077
    (raw 0.147); on the 965 silhouette pixels guided / unguided blur (K 4) = 0.060.  The thresholds keep a margin of 3-6x."""
    q = quality(medium_scene, camera, {"guided": dict(), "unguided": dict(iterations=4, **UNGUIDED)})
    print("quality", q)
    assert q["edge_pixels"] > 100
    assert q["guided"] <= 0.05 * q["raw"], q
    assert q["guided_edge"] <= 0.2 * q["unguided_edge"], q


# ---- the Node host ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")),
                    reason="node or the built addon is missing")
def test_node_host_matches_python_host(small_scene, camera, tmp_path):
    """fspt.js features / denoise / drawDenoised give the Python host's bytes; while a renderAsync job is in flight the
    three throw Error('render in flight')."""
    import base64
    import json
    W, H, seed, ticks, samples, fseed = 96, 64, 13, 6, 4, 3
    env, ew, eh = S.synthetic_env(64, 32)
    job = {"props": S.bunny_props(), "objs": {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ},
           "env": {"rgbe_b64": base64.b64encode(env.tobytes()).decode(), "width": ew, "height": eh},
           "W": W, "H": H, "bounces": 4, "seed": seed, "ticks": ticks, "samples": samples, "feature_seed": fseed,
           "cam": dict(P=camera["P"], I=camera["I"], fov_scale=camera["fov_scale"], env_theta=camera["env_theta"], lens=camera["lens"])}
    jp, op = tmp_path / "job.json", tmp_path / "out.json"
    jp.write_text(json.dumps(job))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "denoise_node_check.js"), str(jp), str(op)], timeout=300)
    out = json.loads(op.read_text())
    dec = lambda k: base64.b64decode(out[k])
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(seed)
    pt.render(ticks)
    pt.features(samples, fseed)
    assert dec("denoised") == pt.denoise().tobytes()
    assert dec("denoised_k2") == pt.denoise(iterations=2, sigma_color=2.0).tobytes()
    assert dec("drawn") == pt.drawDenoised(1.5, 0.8).tobytes()
    assert out["during"] == {"features": "render in flight", "denoise": "render in flight", "drawDenoised": "render in flight"}
    assert out["after"] is None
