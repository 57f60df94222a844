"""CPU checks of next-event estimation of emissive triangles (fspt_target_set_lights): the host alias builder
realises w_i / sum w, also on degenerate weights; the C entry points exist, validate their arguments and refuse a process
without a device; the Python host and the render CLI validate theirs; and the JS host's setLights() reaches the library
and refuses to run while a renderAsync job is in flight (the addon built against tests/napi_mock)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lights_ref as R
from fspt_amd import _lib as L
from fspt_amd import light_alias_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_alias(w):
    w = np.asarray(w, np.float32)
    prob, alias = light_alias_table(w)
    assert prob.dtype == np.float32 and alias.dtype == np.uint32
    assert (alias < w.size).all() and (prob >= 0).all() and (prob <= 1).all()
    want = w.astype(np.float64) / w.astype(np.float64).sum()
    got = R.realised(prob, alias)
    # float32 prob: an entry's realised probability is off by at most its alias contributions' rounding (2^-24 each, / n)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7 / w.size), np.abs(got - want).max()
    assert abs(got.sum() - 1.0) < 1e-6
    return prob, alias, got


def test_alias_reproduces_the_weights():
    rng = np.random.default_rng(1)
    for n in (2, 3, 7, 100, 4097):
        check_alias(rng.uniform(0.0, 10.0, n))
    check_alias(rng.exponential(1.0, 1000) ** 4)


def test_alias_degenerate_inputs():
    _, alias, got = check_alias([3.5])
    assert alias[0] == 0 and got[0] == 1.0
    prob, alias, got = check_alias(np.full(64, 0.25))
    assert (prob == 1.0).all() and np.array_equal(alias, np.arange(64))
    w = 10.0 ** np.linspace(-30, 30, 61)
    check_alias(w)
    w = np.array([0.0, 1.0, 0.0, 3.0, 0.0, 0.0, 2.0])
    _, _, got = check_alias(w)
    assert (got[w == 0] == 0).all()


def test_alias_refuses_bad_weights():
    for bad in ([0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [np.inf, 1.0]):
        with pytest.raises(L.FsptError):
            light_alias_table(bad)
    with pytest.raises(ValueError):
        light_alias_table([])


def test_entry_points_exist_and_validate():
    lib = C.CDLL(L.LIB_PATH)
    for n in ("fspt_target_set_lights", "fspt_target_get_lights", "fspt_scene_light_count", "fspt_scene_light_table",
              "fspt_light_sample_eval", "fspt_light_alias_table"):
        assert hasattr(lib, n) and n in L.SIGNATURES
    lib = L.lib()
    assert lib.fspt_target_set_lights(None, 1, 0.5) == -1
    assert lib.fspt_target_get_lights(None, None, None) == -1
    assert lib.fspt_scene_light_count(None, None) == -1
    assert lib.fspt_scene_light_table(None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.fspt_light_sample_eval(None, None, 0, None, None) == -1
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # bad arguments are refused before the handle is looked at
    for mode, f in ((2, 0.5), (-1, 0.5), (1, 0.0), (1, -0.5), (1, 1.5), (1, float("nan")), (0, float("inf"))):
        assert lib.fspt_target_set_lights(fake, mode, f) == -1, (mode, f)
    assert lib.fspt_target_set_lights(fake, 7, 0.5) == -1 and b"FSPT_LIGHTS_EMITTERS" in lib.fspt_last_error()
    assert lib.fspt_target_set_lights(fake, 1, 2.0) == -1 and b"(0, 1]" in lib.fspt_last_error()
    assert lib.fspt_scene_light_count(fake, None) == -1
    assert lib.fspt_light_alias_table(None, 3, None, None) == -1


def test_no_device():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # (zeroed: device 0, no table yet)
    n = C.c_uint32()
    assert lib.fspt_scene_light_count(fake, C.byref(n)) == -2
    assert b"no CPU fallback" in lib.fspt_last_error()
    assert lib.fspt_scene_light_table(fake, C.byref(n), None, None, None, None, None, None, None, None) == -2
    q = np.zeros(10, np.float32); tri = np.zeros(1, np.int32); out = np.zeros(8, np.float32)
    assert lib.fspt_light_sample_eval(fake, L.fptr(q), 1, tri.ctypes.data_as(C.POINTER(C.c_int32)), L.fptr(out)) == -2


def test_python_argument_checks():
    from fspt_amd.tracer import PathTracer
    pt = PathTracer.__new__(PathTracer)  # (the checks run before the library is called)
    pt._t = C.c_void_p()
    with pytest.raises(ValueError):
        pt.set_lights("area")
    for f in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError):
            pt.set_lights("emitters", f)
    for f in ("0.5", None, True):
        with pytest.raises(TypeError):
            pt.set_lights("emitters", f)


def test_cli_flags():
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--lights" in r.stdout and "--emitter-fraction" in r.stdout
    for args, msg in ((["--lights", "--emitter-fraction", "0"], "(0, 1]"), (["--lights", "--emitter-fraction", "1.5"], "(0, 1]"),
                      (["--emitter-fraction", "0.25"], "needs --lights")):
        r = subprocess.run([sys.executable, "-m", "fspt_amd.render"] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("lights_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "lights_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out, log = os.path.join(d, "out.json"), os.path.join(d, "calls.txt")
    env = dict(os.environ, FSPT_MOCK_LIGHTS_LOG=log)
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "lights_mock_check.js"), d, out], timeout=120, env=env)
    rep = json.load(open(out))
    rep["calls"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return rep


def test_js_set_lights_checks_and_reaches_the_library(js_report):
    assert js_report["mode"] == "RangeError: setLights: mode must be 'off' or 'emitters'"
    assert js_report["fraction"] == "RangeError: setLights: emitterFraction must be a number in (0, 1]"
    assert js_report["nan"] == js_report["fraction"]
    assert js_report["ok"] is None and js_report["after"] is None
    assert js_report["calls"] == ["1 0.250", "1 0.500", "0 1.000", "1 0.750"]


def test_js_set_lights_guarded(js_report):
    assert js_report["during"] == "Error: render in flight"
    assert js_report["wrong_kind"] == "TypeError: fspt_napi: expected a target handle"
    assert js_report["destroyed"] == "Error: fspt_napi: the target handle was destroyed"
