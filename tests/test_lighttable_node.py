"""The light-table builder switch in the Node host: setLightBuilder / getLightBuilder on the mock library (no
GPU) - the argument checks, the calls through the addon and its handle guards."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("lightbuilder_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "lightbuilder_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out, log = os.path.join(d, "out.json"), os.path.join(d, "calls.txt")
    env = dict(os.environ, FSPT_MOCK_LIGHTBUILDER_LOG=log)
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "lightbuilder_mock_check.js"), d, out], timeout=120, env=env)
    rep = json.load(open(out))
    rep["calls"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return rep


def test_js_light_builder_checks_and_reaches_the_library(js_report):
    r = js_report
    assert r["first"] == "host"
    assert r["bad"] == "RangeError: setLightBuilder: builder must be 'host' or 'gpu'" == r["none"]
    assert r["ok"] is None and r["gpu"] == "gpu"
    assert r["back"] is None and r["host"] == "host"
    assert r["addon_bad"] is not None and r["addon_bad"].startswith("Error")  # the library's refusal
    assert r["after"] is None
    assert r["calls"] == ["1", "0", "1"]  # nothing refused reached the library


def test_js_light_builder_guarded(js_report):
    r = js_report
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["wrong_kind"] == ["TypeError: fspt_napi: expected a scene handle"] * 2
    assert r["destroyed"] == ["Error: fspt_napi: the scene handle was destroyed"] * 2
