"""Auto-exposure (fspt_target_set_auto_exposure), the part that needs no GPU: the entry points exist and check
their arguments, the Python host and the CLI validate, the restatement the GPU tests compare against (tests/exposure_ref.py)
has the identities the rule promises, and the Node host runs on the mock library."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exposure_ref as R
from fspt_amd import _lib as L
from fspt_amd import tracer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ("fspt_target_set_auto_exposure", "fspt_exposure_reset", "fspt_exposure_get")
TUNING = ("fspt_exposure_eval", "fspt_exposure_last_ms", "fspt_exposure_last_draw_ms", "fspt_exposure_set_form")
F = np.float32
INF, NAN = float("inf"), float("nan")
BAD_PARAMS = (dict(key=0.0), dict(key=-1.0), dict(key=NAN), dict(key=INF), dict(low=-0.1), dict(low=0.9, high=0.1), dict(low=0.5, high=0.5),
              dict(high=1.5), dict(adapt_up=0.0), dict(adapt_up=1.5), dict(adapt_down=0.0), dict(adapt_down=-1.0), dict(adapt_down=NAN),
              dict(min_log2=2.0, max_log2=1.0), dict(min_log2=-INF), dict(max_log2=INF))


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
    assert "typedef struct fspt_exposure_params { float key, low, high, adapt_up, adapt_down, min_log2, max_log2; } fspt_exposure_params;" in hdr
    assert L.SIGNATURES["fspt_target_set_auto_exposure"] == (C.c_int, [C.c_void_p, C.c_int, C.POINTER(L.ExposureParams)])
    assert L.SIGNATURES["fspt_exposure_get"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32)])
    assert [n for n, _ in L.ExposureParams._fields_] == list(R.DEFAULTS) and C.sizeof(L.ExposureParams) == 28
    assert C.sizeof(L.ExposureState) == 32
    lib = L.lib()
    f, u = C.c_float(), C.c_uint32()
    assert lib.fspt_target_set_auto_exposure(None, 1, None) == -1
    assert b"fspt_target_set_auto_exposure: NULL argument" in lib.fspt_last_error()
    assert lib.fspt_target_set_auto_exposure(None, 0, None) == -1
    assert lib.fspt_exposure_reset(None) == -1
    assert lib.fspt_exposure_get(None, C.byref(f), C.byref(f), C.byref(u)) == -1
    assert lib.fspt_exposure_last_ms(None, (C.c_float * 2)()) == -1
    assert lib.fspt_exposure_last_draw_ms(None, C.byref(f)) == -1
    assert b"NULL" in lib.fspt_last_error()
    assert lib.fspt_exposure_set_form(2) == -1 and lib.fspt_exposure_set_form(-1) == -1 and lib.fspt_exposure_set_form(0) == 0
    assert lib.fspt_abi_version() == 4  # entry points are only added


def test_library_refuses_bad_parameters():
    """fspt_exposure_eval checks NULL arguments, the parameters and the viewport before it looks for a device"""
    lib = L.lib()
    img = np.ones((2, 3, 4), F)
    hist = np.zeros(256, np.uint32)
    hp = hist.ctypes.data_as(C.POINTER(C.c_uint32))
    st = L.ExposureState()
    ok = L.ExposureParams(*(R.DEFAULTS[k] for k in R.DEFAULTS))
    for bad in BAD_PARAMS:
        prm = L.ExposureParams(*({**R.DEFAULTS, **bad}[k] for k in R.DEFAULTS))
        assert lib.fspt_exposure_eval(0, L.fptr(img), 3, 2, 3, 2, C.byref(prm), None, hp, C.byref(st)) == -1, bad
        assert b"fspt_exposure_eval: need finite parameters" in lib.fspt_last_error()
    assert lib.fspt_exposure_eval(0, None, 3, 2, 3, 2, C.byref(ok), None, hp, C.byref(st)) == -1
    assert lib.fspt_exposure_eval(0, L.fptr(img), 3, 2, 3, 2, C.byref(ok), None, None, C.byref(st)) == -1
    assert lib.fspt_exposure_eval(0, L.fptr(img), 3, 2, 3, 2, C.byref(ok), None, hp, None) == -1
    for vw, vh in ((4, 2), (3, 3), (0, 2), (3, 0)):
        assert lib.fspt_exposure_eval(0, L.fptr(img), 3, 2, vw, vh, C.byref(ok), None, hp, C.byref(st)) == -1, (vw, vh)
    if lib.fspt_device_count() == 0:
        assert lib.fspt_exposure_eval(0, L.fptr(img), 3, 2, 3, 2, None, None, hp, C.byref(st)) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_host_validates():
    tun = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    for k in R.DEFAULTS:
        assert float(re.search(r"#define FSPT_EXPOSURE_%s (-?[0-9.eE+]+)f?\b" % k.upper(), tun).group(1)) == TR.EXPOSURE_DEFAULTS[k] == R.DEFAULTS[k]
    js = open(os.path.join(ROOT, "fspt_amd", "js", "fspt.js")).read()
    m = re.search(r"key: ([0-9.]+), low: ([0-9.]+), high: ([0-9.]+), adaptUp: ([0-9.]+), adaptDown: ([0-9.]+), minLog2: (-?[0-9.]+), maxLog2: ([0-9.]+) };  // include/fspt_tuning.h FSPT_EXPOSURE", js)
    assert [float(x) for x in m.groups()] == [R.DEFAULTS[k] for k in R.DEFAULTS]
    p = TR._exposure_params({})
    assert [getattr(p, k) for k in R.DEFAULTS] == [float(F(R.DEFAULTS[k])) for k in R.DEFAULTS]
    assert TR._exposure_params(dict(key=0.5, adapt_up=0.25)).adapt_up == 0.25
    for bad in BAD_PARAMS:
        with pytest.raises(ValueError, match="auto-exposure"):
            TR._exposure_params(bad)
    with pytest.raises(TypeError, match="unknown auto-exposure"):
        TR._exposure_params(dict(keys=1.0))
    sig = inspect.signature(TR.PathTracer.set_auto_exposure).parameters
    assert list(sig) == ["self", "on", "params"] and sig["on"].default is True
    for name in ("exposure", "exposure_reset", "exposure_last_ms"):
        assert hasattr(TR.PathTracer, name)
    import fspt_amd
    assert fspt_amd.exposure_eval is TR.exposure_eval
    a4 = np.zeros((3, 2, 4), F)
    for args, kw in (((a4[..., :3],), {}), ((a4,), dict(viewport=(3, 3))), ((a4,), dict(viewport=(0, 1))), ((a4,), dict(key=-1.0))):
        with pytest.raises(ValueError):
            TR.exposure_eval(*args, **kw)
    from fspt_amd import scene_file as SF
    assert 0.0 < SF.SEQUENCE_ADAPT < 1.0
    assert SF._auto_exposure_params(None) is None and SF._auto_exposure_params(False) is None
    assert SF._auto_exposure_params(True) == {} and SF._auto_exposure_params(True, 0.25) == {"adapt_up": 0.25, "adapt_down": 0.25}
    assert SF._auto_exposure_params({"adapt_up": 1.0}, 0.25) == {"adapt_up": 1.0}
    for bad, exc in (({"key": -1.0}, ValueError), ({"keyy": 1.0}, TypeError)):
        with pytest.raises(exc):
            SF.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, auto_exposure=bad)
        with pytest.raises(exc):
            SF.render_frame(None, {}, 8, 8, auto_exposure=bad)


def test_cli_refuses_what_it_cannot_honour():
    run = lambda *a: subprocess.run([sys.executable, "-m", "fspt_amd.render", *a], cwd=ROOT, capture_output=True, text=True)
    for bad in ("0", "-1", "nan", "inf"):
        r = run("--auto-exposure=" + bad, "--out", "x.png")
        assert r.returncode == 2 and "--auto-exposure KEY must be a finite value > 0" in r.stderr, bad
    r = run("--scene", "x_{frame}.json", "--frames", "0:2", "--auto-exposure", "--exposure", "2", "--out", "x{frame}.png")
    assert r.returncode == 2 and "takes its compensation from the scene files" in r.stderr


# ---- the restatement's identities -------------------------------------------------------------------------------------
def test_fma32_is_a_correctly_rounded_fma():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = (rng.uniform(0.5, 2.0, 4000) * 2.0 ** rng.integers(-20, 20, 4000)).astype(F)
    b = F(0.7152)
    c = (-a.astype(np.float64) * np.float64(b) * (1.0 + rng.uniform(-1e-6, 1e-6, 4000))).astype(F)  # (heavy cancellation)
    c[::2] = (rng.uniform(0.5, 2.0, 2000) * 2.0 ** rng.integers(-30, 30, 2000)).astype(F)
    got = R.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b)) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), i


def test_powers_of_two_land_in_bin_8_e_plus_16():
    for e in range(-16, 16):
        assert R.bins_of(F(2.0 ** e)) == 8 * (e + 16), e
        for m in range(8):
            assert R.bins_of(F(2.0 ** e * (1 + m / 8))) == 8 * (e + 16) + m
            assert R.bins_of(np.nextafter(F(2.0 ** e * (1 + m / 8)), F(0))) == 8 * (e + 16) + m - 1  # (-1 below 2^-16: left out)
    assert R.bins_of(F(2.0 ** 16)) == 255 and R.bins_of(F(np.inf)) == 255 and R.bins_of(F(3e38)) == 255
    assert R.bins_of(np.nextafter(F(2.0 ** 16), F(0))) == 255


def test_what_is_left_out():
    assert R.bins_of(F(2.0 ** -16)) == 0 and R.bins_of(np.nextafter(F(2.0 ** -16), F(0))) == -1
    for v in (0.0, -0.0, -1.0, -np.inf, np.nan, 1e-45, 1e-39, 2.0 ** -17):
        assert R.bins_of(F(v)) == -1, v
    img = R.image(17, 33, "excluded")
    h, st = R.meter(img)
    assert h.sum() == 0 and st == R.FIRST  # N = 0: never set, exposure 1
    prev = R.resolve(R.histogram(R.image(5, 5, "constant")))
    assert R.resolve(h, prev) == prev      # N = 0 leaves the state alone


def test_constant_image_fills_one_bin_and_the_mean_is_its_value():
    img = R.image(50, 37, "constant")
    L0 = R.luma(img[0, 0])
    h, st = R.meter(img)
    b = int(R.bins_of(L0))
    assert h[b] == 50 * 37 and h.sum() == 50 * 37
    assert st["log2_mean"] == R.bin_value(b) and abs(R.bin_value(b) - np.log2(float(L0))) <= 1.0 / 16
    assert st["log2_exposure"] == float(np.log2(np.float64(F(0.18)))) - R.bin_value(b) and st["valid"] == 1 and st["metered"] == 50 * 37
    vp = R.meter(img, viewport=(7, 5))[1]
    assert vp["metered"] == 35 and vp["log2_mean"] == st["log2_mean"]


def test_low_0_high_1_keeps_everything():
    img = R.image(17, 33, "noise")
    h = R.histogram(img)
    st = R.resolve(h, low=0.0, high=1.0)
    want = sum(int(h[b]) * R.bin_value(b) for b in range(256)) / int(h.sum())
    assert abs(st["log2_mean"] - want) <= R.GAMMA_BOUND
    # the percentiles cut: dropping the brightest tenth lowers the mean, dropping the darkest raises it
    assert R.resolve(h, low=0.0, high=0.9)["log2_mean"] < st["log2_mean"] < R.resolve(h, low=0.1, high=1.0)["log2_mean"]
    one = np.zeros(256, np.uint32); one[40] = 1
    assert R.resolve(one, low=0.4, high=0.5)["log2_mean"] == R.bin_value(40)  # K >= 1 for one pixel


def test_adaptation():
    h = R.histogram(R.image(16, 16, "noise"))
    wide = dict(min_log2=-40.0, max_log2=40.0)  # (30 octaves of noise meter far from 1: the clamp is tested on its own below)
    target = R.resolve(h, **wide)["log2_exposure"]
    for e0 in (target - 3.0, target + 2.5):
        prev = dict(R.FIRST, valid=1, log2_exposure=e0)
        assert R.resolve(h, prev, adapt_up=1.0, adapt_down=1.0, **wide)["log2_exposure"] == pytest.approx(target, abs=1e-12)  # 1 = instant
        a = 0.25
        st = prev
        for n in range(1, 9):  # a static image: target + (e0 - target)(1 - a)^n
            st = R.resolve(h, st, adapt_up=a, adapt_down=a, **wide)
            assert st["log2_exposure"] == pytest.approx(target + (e0 - target) * (1 - a) ** n, abs=1e-12)
    # brighter scene (target below the state) takes adapt_up, darker adapt_down
    up = R.resolve(h, dict(R.FIRST, valid=1, log2_exposure=target + 2.0), adapt_up=0.5, adapt_down=0.125, **wide)
    dn = R.resolve(h, dict(R.FIRST, valid=1, log2_exposure=target - 2.0), adapt_up=0.5, adapt_down=0.125, **wide)
    assert up["log2_exposure"] == pytest.approx(target + 1.0) and dn["log2_exposure"] == pytest.approx(target - 1.75)
    # an invalid previous state is not adapted from; the clamp holds
    assert R.resolve(h, dict(R.FIRST, log2_exposure=5.0), adapt_up=0.25, adapt_down=0.25, **wide)["log2_exposure"] == target
    lo = float(np.ceil(target)) + 1.0  # (an integer: exact as the float32 the library holds)
    st = R.resolve(h, min_log2=lo, max_log2=lo + 2.0)
    assert st["log2_exposure"] == lo and st["exposure"] == F(2.0 ** lo)
    assert R.resolve(h, min_log2=lo - 9.0, max_log2=lo - 4.0)["log2_exposure"] == lo - 4.0


def test_inputs_reach_every_branch():
    Ls = R.edge_lumas()
    assert Ls.size == 771 and np.array_equal(R.luma(R.rgb_for_luma(Ls)), Ls)
    b = R.bins_of(Ls)
    assert (b == -1).sum() == 1 and set(b[b >= 0]) == set(range(256))  # only the float below 2^-16 is left out; every bin is reached
    sp = R.luma(R.image(50, 37, "special"))
    assert np.isnan(sp).any() and np.isposinf(sp).any() and (sp < 0).any() and (sp == 0).any() and ((sp > 0) & (sp < 1.2e-38)).any() and (sp >= 65536).any()
    h = R.histogram(R.image(50, 37, "noise"))
    assert (h > 0).sum() > 200
    assert R.histogram(R.image(50, 37, "excluded")).sum() == 0


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("exposure_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "exposure_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "exposure_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_auto_exposure_calls_and_handles(js_report):
    r = js_report
    assert r["off_get"] is not None and r["off_reset"] is not None
    assert r["defaults"] == {"exposure": float(F(0.18)), "log2Mean": 1.0, "metered": 1001}
    assert r["some"] == {"exposure": 0.5, "log2Mean": 0.25, "metered": 2001}
    assert r["reset"] == {"exposure": 1.0, "log2Mean": 0.25, "metered": 2011}
    assert r["unknown"] == "RangeError: setAutoExposure: unknown parameter keyValue"
    assert r["not_a_number"].startswith("TypeError")
    assert all(b is not None for b in r["bad"])
    assert "handle" in r["scene_as_target"] and r["too_few"] is not None
    assert r["during"] == ["Error: render in flight"] * 3 and r["after"] is None
    assert r["off_again"] is not None
    assert "destroyed" in r["closed"]
