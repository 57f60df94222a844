"""Temporal history clamp (fspt_temporal_set_clamp), the part that needs no GPU: the entry points exist and
check their arguments, the Python host and the CLI validate, the float64 restatement the GPU tests compare against
(tests/clamp_ref.py) has the identities the rule promises, the exempt set of the GPU test's own inputs stays under its
cap, and the Node host runs on the mock library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import clamp_ref as R
from fspt_amd import _lib as L
from fspt_amd import tracer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ("fspt_temporal_set_clamp",)
TUNING = ("fspt_temporal_read_fast", "fspt_temporal_clamp_last_ms", "fspt_temporal_clamp_eval")
INF, NAN = float("inf"), float("nan")


def test_entry_points_exist_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "fspt.h")).read()
    tun = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in BOUNDARY:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/fspt.h"
    for name in TUNING:
        assert re.search(r"\bint\s+%s\s*\(" % name, tun), f"{name} is not declared in include/fspt_tuning.h"
    for name in BOUNDARY + TUNING:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert L.SIGNATURES["fspt_temporal_set_clamp"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float])
    lib = L.lib()
    buf = np.zeros(16, np.float32)
    assert lib.fspt_temporal_set_clamp(None, 1, 16.0, 2.0) == -1
    assert b"fspt_temporal_set_clamp: NULL argument" in lib.fspt_last_error()
    assert lib.fspt_temporal_set_clamp(None, 0, 0.0, 0.0) == -1
    assert lib.fspt_temporal_read_fast(None, L.fptr(buf)) == -1
    assert lib.fspt_temporal_clamp_last_ms(None, L.fptr(buf)) == -1
    assert b"NULL" in lib.fspt_last_error()
    assert lib.fspt_abi_version() == 4  # entry points are only added


def test_library_refuses_bad_arguments():
    """fspt_temporal_clamp_eval checks NULL arguments and sigma_scale before it looks for a device"""
    lib = L.lib()
    h, f, out = (np.zeros((2, 2, 4), np.float32) for _ in range(3))
    for bad in (-1.0, -1e-30, NAN, -INF):
        assert lib.fspt_temporal_clamp_eval(0, L.fptr(h), L.fptr(f), 2, 2, bad, L.fptr(out), None, None) == -1, bad
        assert b"fspt_temporal_clamp_eval: need" in lib.fspt_last_error()
    assert lib.fspt_temporal_clamp_eval(0, None, L.fptr(f), 2, 2, 2.0, L.fptr(out), None, None) == -1
    assert lib.fspt_temporal_clamp_eval(0, L.fptr(h), None, 2, 2, 2.0, L.fptr(out), None, None) == -1
    assert lib.fspt_temporal_clamp_eval(0, L.fptr(h), L.fptr(f), 2, 2, 2.0, None, None, None) == -1
    if lib.fspt_device_count() == 0:
        for s in (0.0, 2.0, INF):
            assert lib.fspt_temporal_clamp_eval(0, L.fptr(h), L.fptr(f), 2, 2, s, L.fptr(out), None, None) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_host_validates():
    tun = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    for k, name in (("fast_history", "FAST_HISTORY"), ("sigma_scale", "SIGMA_SCALE")):
        assert float(re.search(r"#define FSPT_TEMPORAL_CLAMP_%s ([0-9.eE+-]+)f?\b" % name, tun).group(1)) == TR.CLAMP_DEFAULTS[k]
    js = open(os.path.join(ROOT, "fspt_amd", "js", "fspt.js")).read()
    m = re.search(r"fastHistory: ([0-9.]+), sigmaScale: ([0-9.]+) };  // include/fspt_tuning.h FSPT_TEMPORAL_CLAMP", js)
    assert (float(m.group(1)), float(m.group(2))) == (TR.CLAMP_DEFAULTS["fast_history"], TR.CLAMP_DEFAULTS["sigma_scale"])
    assert TR._clamp_params() == (TR.CLAMP_DEFAULTS["fast_history"], TR.CLAMP_DEFAULTS["sigma_scale"])
    assert TR._clamp_params(8, INF) == (8.0, INF) and TR._clamp_params(1, 0) == (1.0, 0.0)
    for bad in (dict(fast_history=0.5), dict(fast_history=INF), dict(fast_history=NAN), dict(fast_history=-4), dict(sigma_scale=-1.0), dict(sigma_scale=NAN)):
        with pytest.raises(ValueError, match="history clamp"):
            TR._clamp_params(**bad)
    sig = inspect.signature(TR.PathTracer.temporal_set_clamp).parameters
    assert list(sig) == ["self", "on", "fast_history", "sigma_scale"] and sig["on"].default is True
    assert sig["fast_history"].default is None and sig["sigma_scale"].default is None
    for name in ("temporal_fast", "temporal_clamp_last_ms"):
        assert hasattr(TR.PathTracer, name)
    import fspt_amd
    assert fspt_amd.temporal_clamp_eval is TR.temporal_clamp_eval
    a4 = np.zeros((3, 2, 4), np.float32)
    for args in ((a4[..., :3], a4), (a4, a4[:2]), (a4, a4[..., :3])):
        with pytest.raises(ValueError):
            TR.temporal_clamp_eval(*args)
    with pytest.raises(ValueError, match="history clamp"):
        TR.temporal_clamp_eval(a4, a4, sigma_scale=-2.0)
    from fspt_amd import scene_file as F
    for bad, exc in (({"sigma_scale": -1.0}, ValueError), ({"fast_history": 0.0}, ValueError), ({"sigma": 2.0}, TypeError)):
        with pytest.raises(exc):
            F.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, bvh="refit", temporal={"clamp": bad})


def test_cli_refuses_clamp_without_temporal_and_a_negative_sigma():
    import subprocess, sys
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--temporal-clamp", "--out", "x.png"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--temporal-clamp needs --temporal" in r.stderr
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--scene", "x_{frame}.json", "--frames", "0:2", "--bvh", "refit", "--temporal",
                        "--temporal-clamp=-1", "--out", "x{frame}.png"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--temporal-clamp SIGMA must be >= 0" in r.stderr


# ---- the restatement's identities -------------------------------------------------------------------------------------
def test_sigma_inf_is_the_identity():
    hist, fast = R.synthetic(17, 33)
    out, lo, hi = R.clamp(hist, fast, INF)
    assert np.array_equal(out, hist.astype(np.float64))
    assert np.all(lo == -INF) and np.all(hi == INF) and not np.isnan(lo).any() and not np.isnan(hi).any()
    assert not R.exempt(hist, fast, INF).any()


def test_constant_fast_history_gives_a_point_box():
    rng = np.random.default_rng(5)
    fast = np.zeros((9, 11, 4), np.float32)
    fast[..., :3] = np.float32([0.75, 2.0, 0.125])  # (dyadic: the float64 sums are exact)
    hist = rng.uniform(0, 4, (9, 11, 4)).astype(np.float32)
    for s in (0.0, 1.0, 2.0, 1e6):
        mu, sd, lo, hi, _ = R.box(fast, s)
        assert np.all(sd == 0.0) and np.array_equal(lo, mu) and np.array_equal(hi, mu)
        assert np.array_equal(mu, np.broadcast_to(np.float64([0.75, 2.0, 0.125]), mu.shape))
        out, _, _ = R.clamp(hist, fast, s)
        assert np.array_equal(out[..., :3], mu) and np.array_equal(out[..., 3], hist[..., 3].astype(np.float64))


def test_box_of_a_1x1_image_is_the_pixel():
    fast = np.float32([[[0.3, 5.0, 0.0, 7.0]]])
    hist = np.float32([[[9.0, 1.0, 2.0, 33.0]]])
    for s in (0.0, 2.0):
        out, lo, hi = R.clamp(hist, fast, s)
        assert np.array_equal(lo[0, 0], fast[0, 0, :3].astype(np.float64)) and np.array_equal(hi, lo)
        assert np.array_equal(out[0, 0], np.float64([fast[0, 0, 0], fast[0, 0, 1], fast[0, 0, 2], 33.0]))


def test_border_counts_are_9_15_and_25():
    cnt = R.window_sums(np.zeros((8, 9, 4), np.float32))[0]
    assert cnt[0, 0] == cnt[0, -1] == cnt[-1, 0] == cnt[-1, -1] == 9       # a corner: 3 x 3
    assert cnt[0, 1] == cnt[1, 0] == 12 and cnt[1, 1] == 16                # one step in
    assert cnt[0, 4] == cnt[4, 0] == cnt[-1, 4] == cnt[4, -1] == 15        # an edge: 3 x 5
    assert cnt[2, 2] == cnt[4, 4] == cnt[5, 6] == 25                       # the interior
    assert sorted(np.unique(cnt)) == [9, 12, 15, 16, 20, 25]
    assert np.array_equal(R.window_sums(np.zeros((2, 3, 4), np.float32))[0], np.full((2, 3), 6.0))  # smaller than the window


def test_inside_values_pass_and_outputs_lie_in_the_box():
    for W, H in R.SHAPES:
        hist, fast = R.synthetic(W, H)
        for s in (0.0, 1.0, 2.0):
            out, lo, hi = R.clamp(hist, fast, s)
            h = hist[..., :3].astype(np.float64)
            assert np.all(out[..., :3] >= lo) and np.all(out[..., :3] <= hi)
            inside = (h >= lo) & (h <= hi)
            assert np.array_equal(out[..., :3][inside], h[inside])
            again, _, _ = R.clamp(out, fast, s)
            assert np.array_equal(again, out)


def test_synthetic_inputs_reach_every_regime():
    """what the GPU test's cases promise: exact-zero spread, spread up to 1e6 x the mean, values inside, on and far outside"""
    hist, fast = R.synthetic(50, 37)
    mu, sd, lo, hi, _ = R.box(fast, 1.0)
    assert (sd == 0.0).mean() > 0.1
    assert (sd > 1e6 * np.abs(mu)).any() and (sd > 3.0 * np.abs(mu)).mean() > 0.05
    h = hist[..., :3].astype(np.float64)
    assert ((h > lo) & (h < hi)).mean() > 0.1 and ((h == lo.astype(np.float32)) | (h == hi.astype(np.float32))).any()
    assert (h > hi + 50 * sd + 1.0).mean() > 0.02 and (h < lo).mean() > 0.1


@pytest.mark.parametrize("shape", R.SHAPES + [R.BIG_SHAPE])
def test_exempt_set_of_the_gpu_inputs_is_capped(shape):
    """the values the GPU test does not compare (their branch may flip) are decided by the restatement alone: at most 1 %
    of a case's values, asserted here on the same inputs"""
    hist, fast = R.synthetic(*shape)
    for s in R.SIGMAS:
        ex = R.exempt(hist, fast, s)
        assert ex.sum() <= R.EXEMPT_CAP * ex.size, (shape, s, int(ex.sum()), ex.size)


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("clamp_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "clamp_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "clamp_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_clamp_call_and_handles(js_report):
    r = js_report
    assert r["initial"] == [0.0, 0.0, 0.0, 0.0]
    assert r["defaults"] == [1.0, TR.CLAMP_DEFAULTS["fast_history"], TR.CLAMP_DEFAULTS["sigma_scale"], 1.0]
    assert r["both"] == [1.0, 8.0, 1.5, 2.0]
    assert r["inf"] == [1.0, TR.CLAMP_DEFAULTS["fast_history"], None, 3.0]  # (JSON has no Infinity)
    assert r["off"][0] == 0.0 and r["off"][3] == 4.0
    assert r["unknown"] == "RangeError: temporalSetClamp: unknown parameter fast"
    assert r["not_a_number"].startswith("TypeError")
    assert all(b is not None for b in r["bad"]) and r["off_ignores_numbers"] is None
    assert "handle" in r["scene_as_target"] and r["too_few"] is not None
    assert r["during"] == "Error: render in flight" and r["after"] is None
    assert r["last"][0] == 1.0
    assert "destroyed" in r["closed"]
