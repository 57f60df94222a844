"""The vertex-position update in the Node host: setMesh / updateVertices / readMesh on the mock library (no GPU)."""
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
    d = str(tmp_path_factory.mktemp("mesh_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "mesh_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "mesh_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_mesh_calls_reach_the_library(js_report):
    r = js_report
    assert r["no_mesh"] is not None and r["no_mesh"].startswith("Error")
    assert r["no_read"] is not None and r["read_before_update"] is not None
    assert r["cost_mesh"] == 40000             # max(vertex) + 1 = 4 vertices, no flags, ranks or rest copy
    assert r["cost_updates"] == 40002          # two updates reached the library
    assert r["read"] == [True, 18, 2, True, 54, 4]
    assert r["wrong_count"] is not None        # 3 positions for 4 vertices: the library refuses
    assert r["cost_full"] == 3001152           # nVertices given, smooth flags, ranks, rest copy
    assert r["cost_full_update"] == 3001153
    assert r["cost_static"] == 30053           # the static marker does not count as an index
    assert r["cost_dropped"] == 3              # setMesh(null)


def test_js_mesh_argument_checks(js_report):
    r = js_report
    assert r["short_vertex"] == "RangeError: setMesh: vertex must be a Uint32Array of 2 x 3 indices" == r["u16_vertex"]
    assert r["f32_uv"] == "RangeError: setMesh: uv must be a Float64Array of 2 x 6 values" == r["no_uv"]
    assert r["short_smooth"] == "RangeError: setMesh: smooth must be a Uint8Array of 2 flags"
    assert r["short_rank"] == "RangeError: setMesh: rank must be a Uint32Array of 2 ranks"
    assert r["short_tri"] == "RangeError: setMesh: tri must be a Float32Array of 2 x 9 floats"
    assert r["short_norm"] == "RangeError: setMesh: norm must be a Float32Array of 2 x 27 floats"
    assert r["static_no_rest"] == "RangeError: setMesh: static triangles need the rest tri and norm" == r["static_no_norm"]
    assert r["few_vertices"] == "RangeError: setMesh: nVertices must be an integer in [max(vertex) + 1, 2^32 - 2]" == r["many_vertices"]
    assert r["pos_len"] == "RangeError: updateVertices: pos must be a Float32Array of n_vertices x 3 floats" == r["pos_type"]
    assert r["cost_after_refused"] == r["cost_dropped"]  # nothing refused reached the library
    assert r["addon_len"].startswith("RangeError: fspt_napi: setMesh needs 3 indices") and r["addon_uv"] == r["addon_len"]
    assert r["addon_pos"] == "RangeError: fspt_napi: updateVertices needs 3 floats per vertex"
    assert all(e is not None and "Error" in e for e in r["target_as_scene"])


def test_js_mesh_guarded_while_rendering(js_report):
    r = js_report
    assert all(e is not None and "render in flight" in e for e in r["during"])
    assert r["after"] == [None, None, None]
    assert all(e is not None for e in r["closed"])
