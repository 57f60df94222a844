"""CPU checks of adaptive sampling (fspt_render_adaptive): the float64 restatement's estimator is unbiased at
every split the schedule produces, the schedule's edge cases, the C entry points' argument checks and their refusal
without a device, the Python host's and the CLI's checks, and the JS host's renderAdaptive() / readSampleCounts() through
the addon (built against tests/napi_mock plus tests/adaptive_mock_stub.c)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as R
from fspt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_splits_cover_one_to_one_down_to_power_of_two():
    sp = R.decision_splits(1024, 32)
    assert sp[0] == (32, 64) and sp[-1] == (512, 1024)
    ratios = {m / (n - m) for m, n in sp}
    assert 1.0 in ratios and max(ratios) == 16.0  # m:(n-m) from 1:1 to 2^k:1
    assert all(n % 32 == 0 and 0 < m < n for m, n in sp)


def test_estimator_unbiased_on_gaussian_streams():
    rng = np.random.default_rng(7)
    P, mu, sigma = 400_000, 0.3, 0.8
    for m, n in sorted(set(R.decision_splits(1024, 32))):
        a = rng.normal(mu, sigma / np.sqrt(m), P)          # the mean of samples 1..m
        b = rng.normal(mu, sigma / np.sqrt(n - m), P)      # the mean of samples m+1..n
        I = (m * a + (n - m) * b) / n
        v = R.variance_estimate(I, a, m, n)
        # v / Var(I_n) is chi-square with one degree of freedom: the mean of P of them is 1 +- sqrt(2 / P) = 0.2 %
        assert abs(v.mean() / (sigma * sigma / n) - 1.0) < 0.012, (m, n, v.mean() * n / sigma ** 2)
        # and the closed form the kernel evaluates
        assert np.allclose(v, m * (I - a) ** 2 / (n - m), rtol=1e-6, atol=1e-12)


def synthetic_frames(W, H, max_ticks, rt, seed=3):
    """Running means of per-pixel Gaussian streams whose noise grows with the tile column."""
    rng = np.random.default_rng(seed)
    sig = np.repeat(np.linspace(0.01, 1.0, (W + 31) // 32), 32)[:W][None, :, None] * np.ones((H, 1, 3))
    mean = np.full((H, W, 3), 0.5)
    s = np.zeros((H, W, 3))
    frames = {}
    for n in range(rt, max_ticks + 1, rt):
        s += rng.normal(mean * rt, sig * np.sqrt(rt))
        frames[n] = np.concatenate([(s / n).astype(np.float32), np.ones((H, W, 1), np.float32)], axis=2)
    return frames


def test_schedule_edge_cases():
    W, H, rt = 96, 64, 8
    fr = synthetic_frames(W, H, 64, rt)
    c, e, _, rounds = R.schedule(fr, 0.0, max_ticks=64, min_ticks=16, round_ticks=rt)
    assert (c == 64).all() and rounds == 8 and (e > 0).all()            # threshold 0: every tile runs to max
    c, _, _, rounds = R.schedule(fr, np.inf, max_ticks=64, min_ticks=16, round_ticks=rt)
    assert (c == 16).all() and rounds == 2                               # threshold inf: every tile stops at min = 2R
    c, _, _, rounds = R.schedule(fr, 1e-9, max_ticks=32, min_ticks=32, round_ticks=rt)
    assert (c == 32).all() and rounds == 4                               # max = min
    c, e, _, _ = R.schedule(fr, 2e-3, max_ticks=64, min_ticks=16, round_ticks=rt)
    assert c[:, 0].max() < c[:, -1].min()                                # the quiet tiles stop first
    assert ((e < 2e-3) | (c == 64)).all()
    c, _, _, _ = R.schedule(fr, 0.0, max_ticks=64, min_ticks=16, round_ticks=rt, viewport=(40, 20))
    assert (c[:1, :2] == 64).all() and (c[1:] == 0).all() and (c[:, 2:] == 0).all()
    px = R.expand(c, W, H, viewport=(40, 20))
    assert (px[:20, :40] == 64).all() and px.sum() == 64 * 40 * 20


def _cam():
    cp = L.CameraParams()
    cp.num_bounces = 4
    return cp


BAD_PARAMS = [(1e-3, 1024, 64, 1), (1e-3, 1024, 64, 129), (1e-3, 1024, 48, 32), (1e-3, 1024, 32, 32), (1e-3, 1000, 64, 32),
              (1e-3, 32, 64, 32), (-1e-3, 1024, 64, 32), (float("nan"), 1024, 64, 32), (float("inf"), 1024, 64, 32)]


def test_entry_points_exist_and_validate():
    lib = C.CDLL(L.LIB_PATH)
    for n in ("fspt_render_adaptive", "fspt_read_sample_counts", "fspt_adaptive_last_stats"):
        assert hasattr(lib, n) and n in L.SIGNATURES
    lib = L.lib()
    ok = L.AdaptiveParams(1e-3, 1024, 64, 32)
    assert lib.fspt_render_adaptive(None, C.byref(_cam()), C.byref(ok), 1) == -1
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)  # bad arguments are refused before the handle is looked at
    assert lib.fspt_render_adaptive(fake, None, C.byref(ok), 1) == -1
    assert lib.fspt_render_adaptive(fake, C.byref(_cam()), None, 1) == -1
    for t, mx, mn, r in BAD_PARAMS:
        assert lib.fspt_render_adaptive(fake, C.byref(_cam()), C.byref(L.AdaptiveParams(t, mx, mn, r)), 1) == -1, (t, mx, mn, r)
    assert b"round_ticks" in (lib.fspt_render_adaptive(fake, C.byref(_cam()), C.byref(L.AdaptiveParams(0.0, 64, 64, 1)), 1) and
                              lib.fspt_last_error())
    assert lib.fspt_read_sample_counts(None, None) == -1
    assert lib.fspt_adaptive_last_stats(None, None, None, None, None, 0) == -1


def test_no_device():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    for prm in (L.AdaptiveParams(1e-3, 1024, 64, 32), L.AdaptiveParams(0.0, 64, 64, 32), L.AdaptiveParams(0.0, 256, 4, 2)):
        assert lib.fspt_render_adaptive(fake, C.byref(_cam()), C.byref(prm), 1) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_argument_checks():
    from fspt_amd.tracer import PathTracer
    pt = PathTracer.__new__(PathTracer)  # (the checks run before the library is called)
    pt._t = C.c_void_p()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pt.render_adaptive(bad)
    for bad in ("0.01", None, True):
        with pytest.raises(TypeError):
            pt.render_adaptive(bad)
    with pytest.raises(TypeError):
        pt.render_adaptive(0.01, max_ticks=1024.0)
    with pytest.raises(ValueError):
        pt.render_adaptive(0.01, round_ticks=-32)


def test_cli_flags():
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--adaptive" in r.stdout and "--sample-map" in r.stdout
    for args, msg in ((["--adaptive", "-1"], "finite relative MSE"), (["--adaptive", "nan"], "finite relative MSE"),
                      (["--adaptive", "0.01", "--spp", "100"], "multiple of 32"), (["--adaptive", "0.01", "--spp", "32"], "at least 64"),
                      (["--sample-map", "m.png"], "needs --adaptive")):
        r = subprocess.run([sys.executable, "-m", "fspt_amd.render"] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("adaptive_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "adaptive_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out, log = os.path.join(d, "out.json"), os.path.join(d, "calls.txt")
    env = dict(os.environ, FSPT_MOCK_ADAPTIVE_LOG=log)
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "adaptive_mock_check.js"), d, out], timeout=120, env=env)
    rep = json.load(open(out))
    rep["calls"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return rep


def test_js_render_adaptive_checks_and_reaches_the_library(js_report):
    assert js_report["target"] == "RangeError: renderAdaptive: targetRelMse must be a finite number >= 0"
    assert js_report["nan"] == js_report["target"] and js_report["missing"] == js_report["target"]
    assert js_report["ticks"] == "RangeError: renderAdaptive: maxTicks must be an integer in [0, 2^32)"
    assert js_report["invalid"].startswith("Error: libfspt error -1")
    assert js_report["n"] == 256 and js_report["pingpong"] == 256 and js_report["advanced"] is True
    assert js_report["counts"] == [256, 256, 256, 0, 0, 0]
    assert js_report["counts_len"] == "RangeError: readSampleCounts: need a Uint32Array of W*H counts"
    assert js_report["calls"] == ["0.002500 1024 64 32 1", "0.000000 256 64 32 7"]


def test_js_render_adaptive_guarded(js_report):
    assert js_report["during"] == "Error: render in flight"
    assert js_report["wrong_kind"] == "TypeError: fspt_napi: expected a target handle"
    assert js_report["destroyed"] == "Error: fspt_napi: the target handle was destroyed"
