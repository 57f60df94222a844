"""CPU checks of the pipelined present (include/fspt.h fspt_present): the entry point is exported and bound, refuses NULL
arguments and a process without a device, and the JS host's present() checks its buffer and refuses to run while a
renderAsync job is in flight (the addon built against tests/napi_mock, as tests/test_napi_handles.py does)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from fspt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "fspt_present") and "fspt_present" in L.SIGNATURES
    from fspt_amd import PathTracer
    assert callable(PathTracer.present)


def test_null_arguments_invalid():
    lib = L.lib()
    out = np.zeros(64, np.uint8)
    n = C.c_uint32(99)
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    assert lib.fspt_present(None, 1.0, 1.0, 0, 3.0, 1.0, L.u8ptr(out), C.byref(n)) == -1
    assert lib.fspt_present(fake, 1.0, 1.0, 0, 3.0, 1.0, None, C.byref(n)) == -1
    assert lib.fspt_present(fake, 1.0, 1.0, 0, 3.0, 1.0, L.u8ptr(out), None) == -1
    assert n.value == 99


def test_no_device():
    """Without a HIP device the call fails with FSPT_E_NO_DEVICE before it looks at the target (a stand-in handle that is
    never dereferenced)."""
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    out = np.zeros(64, np.uint8)
    n = C.c_uint32(99)
    assert lib.fspt_present(fake, 1.0, 1.0, 0, 3.0, 1.0, L.u8ptr(out), C.byref(n)) == -2
    assert b"no CPU fallback" in lib.fspt_last_error()
    assert n.value == 99 and not out.any()


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    d = str(tmp_path_factory.mktemp("present_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "present_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "present_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_present_checks_its_buffer(js_report):
    assert js_report["short"] == "RangeError: present: need W*H*4 bytes"
    assert js_report["missing"] == "RangeError: present: need W*H*4 bytes"


def test_js_present_goes_through_the_addon(js_report):
    assert js_report["ticks"] == 7
    assert js_report["frame"] == [0xAB] * 24


def test_js_present_refused_during_render_async(js_report):
    assert js_report["during"] == "Error: render in flight"
    assert js_report["after"] is None
