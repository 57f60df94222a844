"""The GPU sky without a device: the restatements are pinned to the reference's own output, the maps and sun
positions the GPU tests use meet the conditions those tests rest on, every refusal of every new entry comes before a device
is touched, and the Python host routes its arguments to the right entry."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import envbins_ref as E
import sky_cases as SC
import sky_ref as K
from fspt_amd import Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUN = (0.5, 0.6, 0.4)


# ---- the bins' restatement -------------------------------------------------------------------------------------------
def test_envbins_ref_equals_the_reference():
    """... on the odd-sized golden image, whose bins are env_sampler.js's own output, and on a synthetic map"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "js_env_bins_odd.npz"))
    env, w, h = np.asarray(g["env"], np.uint8), int(g["env_w"]), int(g["env_h"])
    got = E.env_bins(env, w, h)
    assert np.array_equal(got, np.asarray(g["bins"], np.uint32).reshape(-1))
    assert np.array_equal(got, S.env_bins(env, w, h))
    env, w, h = S.synthetic_env(64, 32)
    assert np.array_equal(E.env_bins(env, w, h), S.env_bins(env, w, h))


@pytest.fixture(scope="module")
def bins_maps():
    return SC.bins_maps()


def test_envbins_ref_equals_the_cpu_builder_on_every_map(bins_maps):
    for name, (env, w, h) in bins_maps.items():
        assert np.array_equal(E.env_bins(env, w, h), S.env_bins(env, w, h)), name


def test_decision_margins(bins_maps):
    """Any float64 summation order over w h non-negative terms errs by less than w h 2^-53 total, and the thresholds are at
    least total / 64: at 256 x 128 at most 2.4e-10 of the threshold.  A margin of 1e-6 leaves more than three orders of
    magnitude, so on these maps the GPU's table and the CPU's loop must take every decision alike."""
    assert 64 * 256 * 128 * 2.0 ** -53 < 2.4e-10
    for name, (env, w, h) in bins_maps.items():
        m = E.decision_margin(env, w, h)
        assert m >= 1e-6, (name, m)
    assert E.decision_margin(np.zeros(16 * 8 * 4, np.uint8), 16, 8) == math.inf
    # a constant non-zero map ties exactly (16 x 8: a box of two texels holds total / 64): what the maps above must not do
    flat = np.tile(np.array([100, 100, 100, 128], np.uint8), 16 * 8)
    assert E.decision_margin(flat, 16, 8) == 0.0


def test_odd_maps_leave_the_texel_grid(bins_maps):
    """7 x 3, 15 x 7 and 33 x 17 halve into boxes with fractional corners: the path the table cannot serve"""
    for w, h in SC.BINS_NAN:
        box = E.leaves(bins_maps[f"odd_{w}x{h}"][0], w, h)
        assert (box[:, :2] != np.floor(box[:, :2])).any(), (w, h)
    for w, h in ((8, 4), (64, 32)):
        box = E.leaves(bins_maps[f"synthetic_{w}x{h}"][0], w, h)
        assert (box == np.floor(box)).all()


# ---- the sky's restatement -------------------------------------------------------------------------------------------
def test_sky_ref_forms_agree():
    """the kernel's order of operations and the model as its text states it are the same function (float64)"""
    for sun in ((0.0, 1.0, 0.0), SUN, (1.0, 0.0, 0.0), (0.8, -0.17, 0.1)):
        a, _ = K.sky(sun, 12, 6, turbidity=3.0)
        b = K.sky_text(sun, 12, 6, turbidity=3.0)
        assert K.rel_error(a, b) < 1e-6, sun


def test_sky_ref_sanity():
    noon, info = K.sky((0.0, 1.0, 0.0), 32, 16)
    night, _ = K.sky((0.3, -0.5, 0.1), 32, 16)
    dusk, _ = K.sky((1.0, 0.02, 0.0), 32, 16)
    for img in (noon, night, dusk):
        assert np.isfinite(img).all() and (img >= 0).all()
    assert night.sum() < 1e-6 * noon.sum() and 0 < dusk.sum() < noon.sum()
    assert noon[:8, :, 2].mean() > noon[:8, :, 0].mean()  # a blue sky
    assert dusk[7, 0, 0] > dusk[7, 0, 2]  # a red horizon towards the sun
    # the disc: exactly the sky texels with mu >= cos(sun_radius)
    sun = SC.texel_centre(64, 32, 40, 9)
    with_disc, info = K.sky(sun, 64, 32, sun_radius=0.1)
    s = K.unit_sun(sun).astype(np.float64)
    dx, dy, dz = K.directions(64, 32, np.float64)
    mu = dx * s[0] + dy * s[1] + dz * s[2]
    assert np.array_equal(info["disc"], (mu >= math.cos(float(np.float32(0.1)))) & ~info["ground"])
    assert info["disc"][9, 40] and 2 <= info["disc"].sum() < 64
    bright = with_disc[..., 1] > 10 * np.median(with_disc[..., 1])
    assert np.array_equal(bright, info["disc"])


def test_generator_cases_keep_off_the_disc_edge():
    """the condition test_sky_gpu's generator cases rest on: no texel's mu within 1e-5 of cos(sun_radius) - a float32
    rounding of mu (6e-8) cannot move a texel into or out of the disc"""
    cos_r = math.cos(float(np.float32(0.02)))
    for w, h in SC.GEN_SIZES:
        dx, dy, dz = K.directions(w, h, np.float64)
        for name, sun in SC.suns(w, h).items():
            s = K.unit_sun(sun).astype(np.float64)
            mu = dx * s[0] + dy * s[1] + dz * s[2]
            assert np.abs(mu - cos_r).min() > 1e-5, (w, h, name)
            if name == "centre":
                assert mu.max() > 1 - 1e-6


def test_encode_restatement():
    lin = np.array([[[1.0, 0.5, 0.25], [1.0000001, 0.0, 0.0], [0.0, 0.0, 0.0], [np.nan, -1.0, np.inf], [3.0, 1e-9, 2.0], [1e38, 3e38, 0.0]]], np.float32)
    got = K.encode(lin)[0]
    assert got[0].tolist() == [255, 128, 64, 128]  # 2^0 >= 1: e = 0
    assert got[1].tolist() == [128, 0, 0, 129]     # just above 1: e = 1
    assert got[2].tolist() == [0, 0, 0, 128 - 19]  # max(..., 1e-6): 2^-19 >= 1e-6 > 2^-20
    assert got[3].tolist() == [0, 0, 0, 128 - 19]
    assert got[4].tolist() == [191, 0, 128, 130]
    assert got[5, 3] == 255


# ---- refusals, before a device is touched ----------------------------------------------------------------------------
def test_tuning_defaults_are_the_hosts():
    text = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    d = {k.lower(): float(v.rstrip("f")) for k, v in re.findall(r"#define FSPT_SKY_([A-Z_]+) ([0-9.]+f?)", text)}
    want = dict(S.SKY_DEFAULTS, ground_albedo=S.SKY_DEFAULTS["ground_albedo"][0])
    assert {k: d[k] for k in want} == want
    assert d["max_view_samples"] == 64 and d["max_light_samples"] == 32
    assert {k: v for k, v in K.DEFAULTS.items()} == S.SKY_DEFAULTS


REFUSED_PARAMS = {
    "sun_dir is zero": dict(sun=(0.0, 0.0, 0.0)), "sun_dir[1] is not finite": dict(sun=(0.0, float("inf"), 0.0)),
    "sun_dir[0] is not finite": dict(sun=(float("nan"), 1.0, 0.0)),
    "turbidity": dict(turbidity=64.5), "turbidity = -": dict(turbidity=-0.1), "turbidity = nan": dict(turbidity=float("nan")),
    "sun_intensity": dict(sun_intensity=-1.0), "sun_intensity = inf": dict(sun_intensity=float("inf")),
    "sun_radius": dict(sun_radius=0.0), "sun_radius = 0.6": dict(sun_radius=0.6), "gain": dict(gain=-0.5),
    "ground_albedo[0]": dict(ground_albedo=(1.5, 0.3, 0.3)), "ground_albedo[2]": dict(ground_albedo=(0.3, 0.3, -0.1)),
    "view_samples = 0": dict(view_samples=0), "view_samples = 65": dict(view_samples=65),
    "light_samples = 0": dict(light_samples=0), "light_samples = 33": dict(light_samples=33),
}


def test_every_refusal_comes_without_a_device():
    lib = L.lib()
    err = lambda: lib.fspt_last_error().decode()
    good = S.sky_params(SUN)
    out = np.zeros(8 * 4 * 4, np.uint8)
    fake = C.c_void_p(1)  # a scene handle no refusal may look into

    def sky_entries(p, w, h):
        return (("fspt_sky_generate", lambda: lib.fspt_sky_generate(0, p, w, h, L.u8ptr(out), None)),
                ("fspt_scene_update_sky", lambda: lib.fspt_scene_update_sky(fake, p, w, h)))

    for text, kw in REFUSED_PARAMS.items():
        kw = dict(kw)
        p = S.sky_params(kw.pop("sun", SUN), **kw)
        for name, call in sky_entries(C.byref(p), 8, 4):
            assert call() == -1, (name, text)
            assert err().startswith(name + ": ") and text in err(), (name, text, err())
    for w, h in ((0, 4), (8, 0), (65536, 4), (8, 65536)):
        for name, call in (*sky_entries(C.byref(good), w, h),
                           ("fspt_scene_update_environment_auto", lambda: lib.fspt_scene_update_environment_auto(fake, L.u8ptr(out), w, h)),
                           ("fspt_scene_update_environment_device", lambda: lib.fspt_scene_update_environment_device(fake, C.c_void_p(64), w, h)),
                           ("fspt_env_box_sums_eval", lambda: lib.fspt_env_box_sums_eval(0, L.u8ptr(out), w, h, L.u32ptr(np.zeros(4, np.uint32)), 1, np.zeros(1).ctypes.data_as(C.POINTER(C.c_double))))):
            assert call() == -1, (name, w, h)
            assert err().startswith(name + ": ") and "[1, 65535]" in err(), (name, err())
    n = C.c_uint32()
    for w, h in ((0, 4), (8, 0)):
        assert lib.fspt_env_bins_gpu(L.u8ptr(out), w, h, 0, None, 0, C.byref(n)) == -1 and "fspt_env_bins_gpu: NULL/empty argument" in err()
    assert lib.fspt_env_bins_gpu(L.u8ptr(out), 65536, 1, 0, None, 0, C.byref(n)) == -1 and "[1, 65535]" in err()
    assert lib.fspt_env_bins_gpu(None, 8, 4, 0, None, 0, C.byref(n)) == -1
    assert lib.fspt_env_bins_gpu(L.u8ptr(out), 8, 4, 0, None, 0, None) == -1
    for name, call in sky_entries(None, 8, 4):
        assert call() == -1 and err() == f"{name}: NULL params", name
    for name in ("fspt_scene_update_sky", "fspt_scene_update_environment_auto", "fspt_scene_update_environment_device"):
        args = (C.byref(good), 8, 4) if name.endswith("sky") else (L.u8ptr(out), 8, 4)
        assert getattr(lib, name)(None, *args) == -1 and err() == f"{name}: NULL scene", name
    assert lib.fspt_scene_update_environment_auto(fake, None, 8, 4) == -1 and "env is NULL" in err()
    assert lib.fspt_scene_update_environment_device(fake, None, 8, 4) == -1 and "env is NULL" in err()
    assert lib.fspt_scene_update_environment_device(fake, C.c_void_p(66), 8, 4) == -1 and "4-byte aligned" in err()
    assert lib.fspt_scene_last_sky_ms(None, None, None, None, None, None, None) == -1 and err() == "fspt_scene_last_sky_ms: NULL scene"
    assert lib.fspt_multi_update_sky(None, C.byref(good), 8, 4) == -1 and err() == "fspt_multi_update_sky: NULL handle"
    assert lib.fspt_multi_update_environment_auto(None, L.u8ptr(out), 8, 4) == -1 and err() == "fspt_multi_update_environment_auto: NULL handle"
    boxes = np.array([0, 0, 9, 4], np.uint32)
    one = np.zeros(1)
    assert lib.fspt_env_box_sums_eval(0, L.u8ptr(out), 8, 4, L.u32ptr(boxes), 1, one.ctypes.data_as(C.POINTER(C.c_double))) == -1 and "not inside" in err()
    assert lib.fspt_env_box_sums_eval(0, L.u8ptr(out), 8, 4, None, 1, one.ctypes.data_as(C.POINTER(C.c_double))) == -1
    # the existing entry keeps refusing a call without bins
    assert lib.fspt_scene_update_environment(fake, L.u8ptr(out), 8, 4, None, 0) == -1 and "radianceBins" in err()


def test_device_entries_need_a_device():
    """... and say so: FSPT_E_NO_DEVICE where there is none (where there is one, the same calls succeed)"""
    lib = L.lib()
    want = 0 if lib.fspt_device_count() > 0 else -2
    p = S.sky_params(SUN)
    out = np.zeros(8 * 4 * 4, np.uint8)
    n = C.c_uint32()
    one = np.zeros(1)
    boxes = np.array([0, 0, 8, 4], np.uint32)
    assert lib.fspt_sky_generate(0, C.byref(p), 8, 4, L.u8ptr(out), None) == want
    assert lib.fspt_env_bins_gpu(L.u8ptr(out), 8, 4, 0, None, 0, C.byref(n)) == want
    assert lib.fspt_env_box_sums_eval(0, L.u8ptr(out), 8, 4, L.u32ptr(boxes), 1, one.ctypes.data_as(C.POINTER(C.c_double))) == want
    if want:
        assert b"no CPU fallback" in lib.fspt_last_error()
        with pytest.raises(L.FsptError) as e:
            S.sky(SUN, 8, 4)
        assert e.value.code == -2
        with pytest.raises(L.FsptError):
            S.env_bins(out, 8, 4, device=0)


# ---- the Python host's routing ---------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the library: records (entry, arguments), returns FSPT_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fspt_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.fixture
def recorder(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: r)
    return r


def _bare_scene():
    sc = Scene.__new__(Scene)
    sc._h, sc.device = C.c_void_p(1), 0
    return sc


def test_python_routing(recorder):
    sc = _bare_scene()
    env = np.zeros(8 * 4 * 4, np.uint8)
    sc.update_environment(env, 8, 4)
    sc.update_environment(env, 8, 4, np.array([0, 0, 8, 4], np.uint32))
    sc.update_environment(None, 0, 0, np.array([0, 0, 1, 1], np.uint32))
    sc.update_sky((0, 2, 0), turbidity=3, ground_albedo=0.5, view_samples=4)
    sc.update_sky(SUN, 64, 32)
    names = [c[0] for c in recorder.calls]
    assert names == ["fspt_scene_update_environment_auto", "fspt_scene_update_environment", "fspt_scene_update_environment",
                     "fspt_scene_update_sky", "fspt_scene_update_sky"]
    assert recorder.calls[0][1][2:] == (8, 4)
    p = recorder.calls[3][1][1]._obj
    assert recorder.calls[3][1][2:] == (1024, 512) and recorder.calls[4][1][2:] == (64, 32)
    assert (list(p.sun_dir), p.turbidity, p.sun_intensity, p.sun_radius, p.gain, list(p.ground_albedo), p.view_samples, p.light_samples) == \
        ([0.0, 2.0, 0.0], 3.0, 20.0, np.float32(0.02), 1.0, [0.5, 0.5, 0.5], 4, 8)
    for bad in (lambda: sc.update_environment(None, 0, 0), lambda: sc.update_environment(env, 8, 5), lambda: sc.update_sky(SUN, 1.5, 4),
                lambda: sc.update_sky((1, 0), 8, 4), lambda: sc.update_sky(SUN, 8, 4, ground_albedo=(1, 2)), lambda: sc.update_sky(SUN, 8, 4, view_samples=2.5),
                lambda: S.env_bins(env, 8, 5, device=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        sc.update_sky(SUN, 8, 4, turbidty=2)
    assert len(recorder.calls) == 5
    S.sky(SUN, 8, 4)
    S.env_bins(env, 8, 4, device=1)
    assert [c[0] for c in recorder.calls[5:]] == ["fspt_sky_generate", "fspt_env_bins_gpu"] and recorder.calls[6][1][3] == 1


def test_sun_direction():
    assert np.allclose(S.sun_direction(0, 0), (1, 0, 0)) and np.allclose(S.sun_direction(90, 0), (0, 0, 1), atol=1e-15)
    assert np.allclose(S.sun_direction(123, 90), (0, 1, 0), atol=1e-15)
    d = S.sun_direction(30, 45)
    assert abs(sum(c * c for c in d) - 1) < 1e-15 and d[0] > 0 and d[2] > 0


def test_command_line_sky():
    from fspt_amd import render as R
    assert R.parse_sky(None) is None
    at = R.parse_sky("10,20,3", "50,-5", "64x32")
    assert at(0.0) == dict(sun_dir=S.sun_direction(10, 20), width=64, height=32, turbidity=3.0)
    assert at(1.0)["sun_dir"] == S.sun_direction(50, -5) and at(0.5)["sun_dir"] == S.sun_direction(30, 7.5)
    assert R.parse_sky("90,45")(0.7) == dict(sun_dir=S.sun_direction(90, 45), width=1024, height=512, turbidity=1.0)
    for bad in (("a,b",), ("1",), ("1,2,3,4",), ("1,nan",), ("1,2", "3"), ("1,2", None, "64")):
        with pytest.raises(ValueError):
            R.parse_sky(*bad)
    for argv in (["--sky-to", "1,2"], ["--sky", "1,2", "--sky-to", "3,4"], ["--sky", "x"]):
        with pytest.raises(SystemExit):
            R.main(argv)


# ---- the Node host on the mock library -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("sky_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "sky_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "sky_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_sky_calls_reach_the_library(js_report):
    r = js_report
    assert r["c0"] == 0
    assert r["c1"] == pytest.approx(1 + 8 * 10000 + 0.003, abs=1e-6)        # a sky of 8 texels' width, turbidity 3
    assert r["c2"] == pytest.approx(2 + 1024 * 10000 + 0.001, abs=1e-6)     # the defaults: 1024 wide, turbidity 1
    assert r["c3"] == pytest.approx(102 + 3 * 10000 + 0.001, abs=1e-6)      # an auto environment 3 wide
    assert r["cost_after_refused"] == r["c3"]                                 # nothing refused reached it
    assert r["sky"] == [5, 2, 40, [4, 2, 7, 129], [4, 2, 7, 129]]             # samples and the device went through
    assert r["bins"] == [0, 0, 5, 2, 3, 0, 0, 0]


def test_js_sky_argument_checks(js_report):
    r = js_report
    for k in ("no_object", "no_sun", "short_sun"):
        assert r[k].startswith("TypeError: updateSky: expected {sunDir"), (k, r[k])
    assert r["unknown"] == "TypeError: updateSky: unknown parameter turbidty"
    assert r["albedo"].startswith("RangeError: updateSky: groundAlbedo")
    assert r["samples"] == "RangeError: updateSky: viewSamples must be a count"
    assert all(m and m.startswith("Error") for m in r["refused_by_library"]), r["refused_by_library"]
    assert r["auto_short"] == "RangeError: updateEnvironmentAuto: env must be a Uint8Array of 3 x 2 x 4 bytes"
    assert r["auto_zero"].startswith("RangeError: updateEnvironmentAuto: an env needs envW >= 1")
    assert r["auto_null"].startswith("RangeError: updateEnvironmentAuto: env must be a Uint8Array")
    assert r["still_needs_bins"].startswith("RangeError: updateEnvironment: bins must be a Uint32Array")
    assert r["addon_len"].startswith("RangeError: fspt_napi: a sky needs 10 floats")
    assert r["addon_type"].startswith("TypeError: fspt_napi: expected a TypedArray")
    assert r["addon_env_len"].startswith("RangeError: fspt_napi: updateEnvironmentAuto needs envW")
    assert r["addon_bins_len"].startswith("RangeError: fspt_napi: rgbe length")
    assert all(m and "handle" in m for m in r["target_as_scene"]), r["target_as_scene"]


def test_js_sky_render_in_flight_guard(js_report):
    r = js_report
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["after"] == [None, None]
    assert all(m and "destroyed" in m for m in r["closed"]), r["closed"]
