"""CPU checks of the Owen-scrambled Sobol sampler (fspt_target_set_sampler): the numpy restatement has the
(0,m,2)-net property it is built for and stays in [0, 1) at sample indices near 2^32; the C entry points exist, validate
and refuse a process without a device; the Python host validates its arguments; and the JS host's setSampler() reaches
the library and refuses to run while a renderAsync job is in flight (the addon built against tests/napi_mock)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sobol_ref as R
from fspt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def is_net(seed, pixel, pair, m):
    """The first 2^m samples of (dims 2*pair, 2*pair+1) put exactly one point in every 2^a x 2^(m-a) box."""
    n = 1 << m
    s = np.arange(n, dtype=np.uint64)
    x = R.value_bits(seed, pixel, s, 2 * pair) >> np.uint32(8)
    y = R.value_bits(seed, pixel, s, 2 * pair + 1) >> np.uint32(8)
    for a in range(m + 1):
        bx = (x >> np.uint32(24 - a)).astype(np.int64)
        by = (y >> np.uint32(24 - (m - a))).astype(np.int64)
        if not (np.bincount(bx * (1 << (m - a)) + by, minlength=n) == 1).all():
            return False
    return True


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEF])
def test_reference_is_a_net(seed):
    for pixel in (0, 77, 123456, 2 ** 24 - 1):
        for pair in (0, 1, 2, 5, 258):
            for m in range(1, 11):
                assert is_net(seed, pixel, pair, m), (seed, pixel, pair, m)


def test_sobol1_fast_form_matches_the_loop():
    """fspt_math.hpp sobol1: the superset-XOR transform of the index bits, then a reversal, equals the issue's loop."""
    i = np.random.default_rng(3).integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    f = i.copy()
    for sh, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF), (16, 0x0000FFFF)):
        f ^= (f >> np.uint32(sh)) & np.uint32(m)
    assert np.array_equal(R.rev(f), R.sobol1(i))


def test_values_near_2_32_stay_in_range():
    s = np.arange(2 ** 32 - 4096, 2 ** 32, dtype=np.uint64)
    for dim in (0, 1, 7, 516, 519):
        v = R.value(9, 1234, s, dim)
        assert v.dtype == np.float32 and v.min() >= 0.0 and v.max() < 1.0
        assert len(np.unique(v)) > 4000


def test_entry_points_exist_and_validate():
    lib = C.CDLL(L.LIB_PATH)
    for n in ("fspt_target_set_sampler", "fspt_target_get_sampler", "fspt_sampler_eval"):
        assert hasattr(lib, n) and n in L.SIGNATURES
    lib = L.lib()
    assert lib.fspt_target_set_sampler(None, 1, 0) == -1
    assert lib.fspt_target_get_sampler(None, None, None) == -1
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # a bad sampler is refused before the handle is looked at
    assert lib.fspt_target_set_sampler(fake, 2, 0) == -1 and lib.fspt_target_set_sampler(fake, -1, 0) == -1
    assert b"FSPT_SAMPLER_SOBOL" in lib.fspt_last_error()
    a = np.zeros(4, np.uint32)
    assert lib.fspt_sampler_eval(0, 0, None, L.u32ptr(a), L.u32ptr(a), 4, None) == -1


def test_no_device():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    a = np.zeros(4, np.uint32)
    out = np.zeros(4, np.float32)
    assert lib.fspt_sampler_eval(0, 0, L.u32ptr(a), L.u32ptr(a), L.u32ptr(a), 4, L.fptr(out)) == -2
    assert b"no CPU fallback" in lib.fspt_last_error()
    from fspt_amd import FsptError, sampler_eval
    with pytest.raises(FsptError):
        sampler_eval(0, [1], [2], [3])


def test_python_arguments_validated():
    from fspt_amd import PathTracer, sampler_eval
    from fspt_amd import tracer as T

    class Fake:  # set_sampler validates before it reaches the library
        _t = None
    for kind, seed, exc in (("halton", 0, ValueError), ("sobol", -1, ValueError), ("sobol", 2 ** 32, ValueError),
                            ("sobol", 1.5, TypeError), ("sobol", True, TypeError), ("sobol", "3", TypeError)):
        with pytest.raises(exc):
            PathTracer.set_sampler(Fake(), kind, seed)
    with pytest.raises(TypeError):
        sampler_eval(0, [0.5], [0], [0])
    with pytest.raises(ValueError):
        sampler_eval(0, [0], [-1], [0])
    with pytest.raises(ValueError):
        sampler_eval(0, [0], [2 ** 32], [0])
    assert T.SAMPLERS == {"reference": 0, "sobol": 1}


def test_cli_flags():
    r = subprocess.run(["python", "-m", "fspt_amd.render", "--sampler", "sobol", "--sampler-seed", "-1"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--sampler-seed" in r.stderr
    r = subprocess.run(["python", "-m", "fspt_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "--sampler" in r.stdout and "sobol" in r.stdout


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    d = str(tmp_path_factory.mktemp("sampler_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "sampler_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out, log = os.path.join(d, "out.json"), os.path.join(d, "calls.txt")
    env = dict(os.environ, FSPT_MOCK_SAMPLER_LOG=log)
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "sampler_mock_check.js"), d, out], timeout=120, env=env)
    rep = json.load(open(out))
    rep["calls"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return rep


def test_js_set_sampler_checks_and_reaches_the_library(js_report):
    assert js_report["kind"] == "RangeError: setSampler: kind must be 'reference' or 'sobol'"
    assert js_report["seed"] == "RangeError: setSampler: seed must be an integer in [0, 2^32)"
    assert js_report["ok"] is None and js_report["after"] is None
    assert js_report["calls"] == ["1 4000000000", "0 0", "1 5"]


def test_js_set_sampler_guarded(js_report):
    assert js_report["during"] == "Error: render in flight"
    assert js_report["wrong_kind"] == "TypeError: fspt_napi: expected a target handle"
    assert js_report["destroyed"] == "Error: fspt_napi: the target handle was destroyed"
