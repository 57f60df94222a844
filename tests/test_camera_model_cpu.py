"""The opt-in camera models without a device: the GEOMETRY of the numpy restatement (tests/camera_model_ref.py)
in float64 against closed forms, to 1e-5 on unit vectors - a handful of float32 roundings of the inputs and constants
(pi as 3.14159265f, 0.707f) plus the trigonometric reduction -; the Python binding's argument checks and the library's
contract on a mock stub (tests/camera_model_mock_stub.c); the Node host's checks on the same stub; the CLI flag."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import camera_model_ref as R
from fspt_amd import _lib as L
from fspt_amd import render
from fspt_amd.tracer import CAMERA_MODELS, camera_model_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
P = np.array([0.3, -0.2, 2.0])
I = np.array([0.4, -0.3, -1.0])
FOV = 0.5
NO_LENS = [0.5, 0.0]
ZERO = (0.0, 0.0, 0.0, 0.0)


def basis():
    """camera.fs's basis in float64, from its definition"""
    f32 = lambda v: np.asarray(np.float32(v), np.float64)
    Iv = f32(I)
    bx = np.cross(Iv, [0.0, 1.0, 0.0]); bx /= np.linalg.norm(bx)
    by = np.cross(bx, Iv); by /= np.linalg.norm(by)
    return bx, by, Iv / np.linalg.norm(Iv)


def rays64(model, W, H, u=ZERO, lens=NO_LENS, **kw):
    pos, d = R.rays(model, W, H, P, I, FOV, lens, A=R.F64, u=u, **kw)
    assert pos.dtype == np.float64 and np.isfinite(pos).all() and np.isfinite(d).all()
    return pos[..., :3], d[..., :3]


def up_jitter(H=1):
    """draws that move the sample from the centre of the top row's pixel to the frame's top edge: theta = pi / 2, r = 0.5"""
    return (0.25, (0.5 / float(np.float32(0.707))) ** 2, 0.0, 0.0)


def test_equirect_centre_side_and_top():
    bx, by, F = basis()
    _, d = rays64("equirect", 33, 17)
    assert np.abs(d[8, 16] - F).max() < TOL           # the frame centre looks along I
    _, d = rays64("equirect", 2, 1)                   # pixel 1 of 2: u = 0.5
    assert np.abs(d[0, 1] - bx).max() < TOL and d[0, 1] @ bx > 0  # a quarter turn towards basisX: not mirrored
    assert d[0, 0] @ bx < 0
    _, d = rays64("equirect", 1, 1, u=up_jitter())    # v = 1
    assert np.abs(d[0, 0] - by).max() < TOL
    _, d = rays64("equirect", 64, 32)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < TOL


def test_fisheye_edge_and_centre():
    bx, by, F = basis()
    _, d = rays64("fisheye", 1, 1, u=up_jitter(), angle=np.pi)  # top centre: rho = 1, phi = angle / 2
    assert abs(d[0, 0] @ F) < TOL and np.abs(d[0, 0] - by).max() < TOL
    _, d = rays64("fisheye", 1, 1, angle=np.pi)                 # rho == 0
    assert np.array_equal(d[0, 0], F)
    pos, d = rays64("fisheye", 33, 17, angle=2.0)
    assert np.abs(d[8, 16] - F).max() < TOL and np.array_equal(pos[3, 5], np.float32(P).astype(np.float64))
    # equidistant: the angle from F grows linearly with the distance from the centre, angle / 2 per half height
    v = (np.arange(17) + 0.5) / 17 * 2 - 1
    ang = np.arccos(np.clip(d[:, 16] @ F, -1, 1))
    assert np.abs(ang - np.abs(v) * 1.0).max() < TOL
    # beyond phi = pi the backward direction repeats (documented, not special-cased)
    _, d = rays64("fisheye", 64, 8, angle=2 * np.pi)
    assert np.abs(d[4, 0] + F).max() < 1e-3 and np.abs(d[4, 1] + F).max() < 1e-3


def test_ortho_parallel_rays_on_a_grid():
    bx, by, F = basis()
    W, H = 12, 8
    pos, d = rays64("ortho", W, H)
    assert np.abs(d - F).max() == 0
    step = 2 * float(np.float32(FOV)) / H
    assert np.abs((pos[1:] - pos[:-1]) - by * step).max() < TOL
    assert np.abs((pos[:, 1:] - pos[:, :-1]) - bx * step).max() < TOL  # (aspect x 2 fov / W = 2 fov / H: square pixels)
    centre = pos.reshape(-1, 3).mean(0)
    assert np.abs(centre - np.float32(P)).max() < TOL


def test_stereo_eyes():
    bx, by, F = basis()
    W, H, ipd = 16, 8, 0.5
    pos, d = rays64("stereo", W, H, ipd=ipd)
    off = pos - np.float32(P).astype(np.float64)
    assert np.abs(np.linalg.norm(off, axis=-1) - ipd / 2).max() < TOL
    dh = d - (d @ by)[..., None] * by                  # d's horizontal part
    assert np.abs((off * dh).sum(-1)).max() < TOL      # the eye sits beside the ray, not ahead of it
    right = np.cross(dh, by)                           # (basisX = cross(I, up) is the viewer's right)
    side = (off * right).sum(-1)
    assert (side[H // 2:] < 0).all() and (side[:H // 2] > 0).all()  # upper half of the picture: the left eye
    # each half is the equirect picture of its own height
    _, de = rays64("equirect", W, H // 2)
    assert np.abs(d[:H // 2] - de).max() < TOL and np.abs(d[H // 2:] - de).max() < TOL
    with pytest.raises(ValueError):
        R.rays("stereo", 4, 3, P, I, FOV, NO_LENS, A=R.F64, u=ZERO)
    pos, _ = rays64("stereo", 1, 2, ipd=0.0)           # H = 2, no offset
    assert np.abs(pos - np.float32(P)).max() == 0


@pytest.mark.parametrize("model", ["ortho", "fisheye", "equirect", "stereo"])
def test_lens(model):
    W, H = 6, 4
    rng = np.random.default_rng(3)
    u = (rng.random((H, W)), rng.random((H, W)), rng.random((H, W)), rng.random((H, W)))
    o0, d0 = rays64(model, W, H, u=u, lens=[0.5, 0.0])
    o1, d1 = rays64(model, W, H, u=u, lens=[1.0, 0.05])  # lens[0] >= 1: no focal distance
    assert np.array_equal(o0, o1) and np.array_equal(d0, d1)
    a32 = R.rays(model, W, H, P, I, FOV, [0.5, 0.0], u=u)  # ... and exactly so in float32
    b32 = R.rays(model, W, H, P, I, FOV, [1.5, 0.05], u=u)
    assert a32[0].dtype == np.float32 and np.array_equal(a32[0], b32[0]) and np.array_equal(a32[1], b32[1])
    focal, aperture = 3.0, 0.05
    o, d = rays64(model, W, H, u=u, lens=[1 - 1 / focal, aperture])
    focus = o0 + float(1 / (1 - np.float64(np.float32(1 - 1 / focal)))) * d0
    miss = np.linalg.norm(np.cross(focus - o, d), axis=-1)  # distance of the focus point from the lensed ray
    assert miss.max() < TOL
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-12
    bx, by, F = basis()
    assert np.abs((o - o0) @ np.cross(bx, by)).max() < TOL  # the aperture disc lies in the basisX / basisY plane
    assert 0 < np.linalg.norm(o - o0, axis=-1).max() <= aperture + TOL


def test_float32_draws_are_the_samplers():
    """draws(): both samplers give values in [0, 1), the Sobol ones change with the tick and the seed, the reference ones
    with rand_base."""
    a = R.draws(5, 3, 10.0, "reference")
    b = R.draws(5, 3, 11.0, "reference")
    s0 = R.draws(5, 3, 10.0, "sobol", seed=1, tick=0)
    s1 = R.draws(5, 3, 99.0, "sobol", seed=1, tick=1)
    s0b = R.draws(5, 3, 99.0, "sobol", seed=1, tick=0)
    for u in a + s0:
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(s0[0], s1[0]) and np.array_equal(s0[2], s0b[2])


# ---- the Python binding's checks ----------------------------------------------------------------------------------------
def test_python_argument_checks():
    p = camera_model_params()
    assert (p.model, p.angle, p.ipd) == (0, float(np.float32(np.pi)), float(np.float32(0.064)))
    assert camera_model_params(None).model == 0
    assert [camera_model_params(m).model for m in ("pinhole", "ortho", "fisheye", "equirect", "stereo")] == [0, 1, 2, 3, 4]
    assert CAMERA_MODELS == {"pinhole": 0, "ortho": 1, "fisheye": 2, "equirect": 3, "stereo": 4}
    assert camera_model_params("fisheye", angle=2.5).angle == 2.5
    assert camera_model_params("fisheye", angle=2 * np.pi).angle == float(np.float32(2 * np.pi))
    assert camera_model_params("stereo", ipd=0).ipd == 0.0
    for bad in (dict(model="cube"), dict(model=3), dict(model="fisheye", angle=0.0), dict(model="fisheye", angle=6.3),
                dict(model="fisheye", angle=float("nan")), dict(model="fisheye", angle=float("inf")), dict(model="stereo", ipd=-1e-3),
                dict(model="stereo", ipd=float("inf")), dict(model="stereo", ipd=float("nan")), dict(model="ortho", angle=1.0),
                dict(model="equirect", ipd=0.1), dict(model="stereo", angle=1.0)):
        with pytest.raises(ValueError):
            camera_model_params(**bad)
    for bad in (dict(model="fisheye", angle="2"), dict(model="fisheye", angle=True), dict(model="stereo", ipd=[0.1])):
        with pytest.raises(TypeError):
            camera_model_params(**bad)
    for name in ("fspt_target_set_camera_model", "fspt_target_get_camera_model", "fspt_set_rays_device"):
        assert name in L.SIGNATURES
    header = open(os.path.join(ROOT, "include", "fspt.h")).read()
    for name, code in CAMERA_MODELS.items():
        assert "FSPT_CAMERA_%s = %d" % (name.upper(), code) in header


@pytest.fixture(scope="module")
def mock_dir(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler for the mock library")
    d = str(tmp_path_factory.mktemp("camera_model_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "camera_model_mock_stub.c")])
    return d


def test_python_struct_reaches_a_library(mock_dir):
    """The ctypes struct the binding passes is the header's: the mock stub (compiled from include/fspt.h) reads what was set,
    refuses what the library refuses and leaves the model as it was."""
    m = C.CDLL(os.path.join(mock_dir, "libfspt.so"))
    s, t, odd = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert m.fspt_scene_create(None, 0, C.byref(s)) == 0
    assert m.fspt_target_create(s, 6, 4, C.byref(t)) == 0 and m.fspt_target_create(s, 6, 5, C.byref(odd)) == 0
    setter, getter = m.fspt_target_set_camera_model, m.fspt_target_get_camera_model
    setter.argtypes, getter.argtypes = L.SIGNATURES["fspt_target_set_camera_model"][1], L.SIGNATURES["fspt_target_get_camera_model"][1]
    got = L.CameraModelParams()

    def get():
        assert getter(t, C.byref(got)) == 0
        return got.model, got.angle, round(got.ipd % 1000.0, 3)

    assert setter(t, camera_model_params("fisheye", angle=2.5)) == 0 and get() == (2, 2.5, 0.064)
    assert setter(t, camera_model_params("stereo", ipd=0.25)) == 0 and get() == (4, float(np.float32(np.pi)), 0.25)
    for bad in ((9, 1.0, 0.1), (2, 0.0, 0.1), (2, 7.0, 0.1), (2, float("nan"), 0.1), (4, 1.0, -0.5), (4, 1.0, float("inf"))):
        assert setter(t, L.CameraModelParams(*bad)) == -1 and get() == (4, float(np.float32(np.pi)), 0.25)
    assert setter(odd, camera_model_params("stereo")) == -1
    assert setter(t, None) == 0 and get()[0] == 0
    for h in (t, odd):
        m.fspt_target_destroy(h)
    m.fspt_scene_destroy(s)


# ---- the Node host's checks -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(mock_dir):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = mock_dir
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + os.path.join(ROOT, "include"),
                           "-DNODE_GYP_MODULE_NAME=fspt_napi", "-o", os.path.join(d, "fspt_napi.node"),
                           os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"), "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "camera_model_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_calls_reach_the_library(js_report):
    r = js_report
    assert r["initial"] == "pinhole"
    assert r["fisheye"] == ["fisheye", 2.5, 1]
    assert r["stereo"] == ["stereo", 0.25, 2]
    assert r["back"] == ["pinhole", 4]
    assert r["odd_height"] is not None and "-1" in r["odd_height"]  # the library's refusal comes through


def test_js_argument_checks(js_report):
    r = js_report
    assert r["unknown"].startswith("RangeError: setCameraModel: model must be one of")
    assert r["not_object"].startswith("TypeError: setCameraModel")
    for k in ("angle_zero", "angle_big", "angle_nan", "angle_string"):
        assert r[k] == "RangeError: setCameraModel: angle must be a number in (0, 2 pi] radians", k
    for k in ("ipd_neg", "ipd_inf"):
        assert r[k] == "RangeError: setCameraModel: ipd must be a finite number >= 0", k
    assert r["angle_stray"] == "RangeError: setCameraModel: angle only goes with 'fisheye'"
    assert r["ipd_stray"] == "RangeError: setCameraModel: ipd only goes with 'stereo'"
    assert r["calls_after_refused"] == 4  # nothing refused reached the library
    assert r["addon_model"] == "RangeError: fspt_napi: setCameraModel: unknown model"
    assert r["addon_angle"] == "RangeError: fspt_napi: setCameraModel: angle must lie in (0, 2 pi]"
    assert r["addon_ipd"] == "RangeError: fspt_napi: setCameraModel: ipd must be finite and >= 0"
    assert r["scene_as_target"] is not None and "Error" in r["scene_as_target"]
    assert r["calls_after_addon"] == 4  # the addon's own checks come before the library too


def test_js_guarded_while_rendering(js_report):
    r = js_report
    assert all(e is not None and "render in flight" in e for e in r["during"])
    assert r["after"] is None
    assert r["closed"] is not None


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_flag_parsing():
    assert render.parse_camera("pinhole") == {"model": "pinhole"}
    assert render.parse_camera("ortho") == {"model": "ortho"} and render.parse_camera("equirect") == {"model": "equirect"}
    assert render.parse_camera("fisheye") == {"model": "fisheye"} and render.parse_camera("stereo") == {"model": "stereo"}
    assert render.parse_camera("fisheye:180") == {"model": "fisheye", "angle": float(np.float32(np.pi))}
    assert render.parse_camera("fisheye:360")["angle"] == float(np.float32(2 * np.pi))
    assert render.parse_camera("stereo:0.1") == {"model": "stereo", "ipd": 0.1}
    for spec in ("cube", "fisheye:0", "fisheye:361", "fisheye:x", "fisheye:nan", "stereo:-1", "stereo:inf", "ortho:1", "equirect:2", "pinhole:1"):
        with pytest.raises(ValueError):
            render.parse_camera(spec)
    for spec in ("fisheye:180", "stereo:0.1", "ortho"):
        camera_model_params(**render.parse_camera(spec))  # what the flag makes is what the binding takes


def test_cli_refuses_bad_flags():
    run = lambda *a: subprocess.run([sys.executable, "-m", "fspt_amd.render", *a], cwd=ROOT, capture_output=True, text=True, timeout=120)
    r = run("--help")
    assert r.returncode == 0 and "--camera" in r.stdout
    r = run("--camera", "cube", "--out", "x.png")
    assert r.returncode == 2 and "unknown model" in r.stderr
    r = run("--camera", "fisheye:400", "--out", "x.png")
    assert r.returncode == 2 and "(0, 360]" in r.stderr
    r = run("--camera", "equirect", "--adaptive", "0.01", "--spp", "64", "--out", "x.png")
    assert r.returncode == 2 and "cannot be combined" in r.stderr


def test_scene_file_camera_argument():
    from fspt_amd import scene_file as F
    assert F._camera_model_params(None) is None and F._camera_model_params({"model": "pinhole"}) is None
    assert F._camera_model_params({"model": "fisheye", "angle": 2.0}) == {"model": "fisheye", "angle": 2.0}
    with pytest.raises(TypeError):
        F._camera_model_params({"model": "fisheye", "fov": 2.0})
    with pytest.raises(ValueError):
        F._camera_model_params({"model": "fisheye", "angle": 7.0})
    with pytest.raises(ValueError):
        F._camera_model_params({"model": "equirect"}, adaptive=0.01)
    with pytest.raises(ValueError):
        F._camera_model_params({"model": "equirect"}, temporal={})
