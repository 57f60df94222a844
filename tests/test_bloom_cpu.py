"""Bloom (fspt_target_set_bloom), the part that needs no GPU: the entry points exist and check their arguments,
the Python host and the CLI validate, the restatement the GPU tests compare against (tests/bloom_ref.py) has the identities
the rule promises, and the Node host runs on the mock library."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bloom_ref as R
from fspt_amd import _lib as L
from fspt_amd import tracer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ("fspt_target_set_bloom", "fspt_target_get_bloom")
TUNING = ("fspt_bloom_eval", "fspt_bloom_texels", "fspt_bloom_set_form", "fspt_bloom_set_tail_texels", "fspt_bloom_last_ms")
F = np.float32
INF, NAN = float("inf"), float("nan")
BAD_PARAMS = (dict(intensity=-0.1), dict(intensity=1.5), dict(intensity=NAN), dict(intensity=INF), dict(scatter=-0.5), dict(scatter=1.0001),
              dict(scatter=NAN), dict(scatter=-INF), dict(levels=0), dict(levels=9))


def test_entry_points_exist_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "fspt.h")).read()
    tun = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in BOUNDARY:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/fspt.h"
    for name in TUNING:
        assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % name, tun), f"{name} is not declared in include/fspt_tuning.h"
    for name in BOUNDARY + TUNING:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert "typedef struct fspt_bloom_params { float intensity, scatter; uint32_t levels; } fspt_bloom_params;" in hdr
    assert L.SIGNATURES["fspt_target_set_bloom"] == (C.c_int, [C.c_void_p, C.c_int, C.POINTER(L.BloomParams)])
    assert L.SIGNATURES["fspt_target_get_bloom"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(L.BloomParams)])
    assert [n for n, _ in L.BloomParams._fields_] == list(R.DEFAULTS) and C.sizeof(L.BloomParams) == 12
    lib = L.lib()
    on, prm = C.c_int(), L.BloomParams()
    assert lib.fspt_target_set_bloom(None, 1, None) == -1
    assert b"fspt_target_set_bloom: NULL argument" in lib.fspt_last_error()
    assert lib.fspt_target_set_bloom(None, 0, None) == -1
    assert lib.fspt_target_get_bloom(None, C.byref(on), C.byref(prm)) == -1
    assert lib.fspt_bloom_last_ms(None, (C.c_float * 4)()) == -1
    assert b"NULL" in lib.fspt_last_error()
    assert lib.fspt_bloom_set_form(2) == -1 and lib.fspt_bloom_set_form(-1) == -1 and lib.fspt_bloom_set_form(0) == 0
    assert lib.fspt_bloom_set_tail_texels(0) == 0
    assert lib.fspt_abi_version() == 4  # entry points are only added


def test_library_refuses_bad_parameters():
    """fspt_bloom_eval checks NULL arguments, the parameters and the viewport before it looks for a device"""
    lib = L.lib()
    img = np.ones((2, 3, 4), F)
    n = C.c_uint32()
    ok = L.BloomParams(*(R.DEFAULTS[k] for k in R.DEFAULTS))
    ev = lambda rgba, vw, vh, prm: lib.fspt_bloom_eval(0, rgba, 3, 2, vw, vh, prm, C.byref(n), None, None, None, None)
    for bad in BAD_PARAMS:
        prm = L.BloomParams(*({**R.DEFAULTS, **bad}[k] for k in R.DEFAULTS))
        assert ev(L.fptr(img), 3, 2, C.byref(prm)) == -1, bad
        assert b"fspt_bloom_eval: need finite intensity and scatter in [0, 1] and levels in [1, 8]" in lib.fspt_last_error()
    assert ev(None, 3, 2, C.byref(ok)) == -1
    for vw, vh in ((4, 2), (3, 3), (0, 2), (3, 0)):
        assert ev(L.fptr(img), vw, vh, C.byref(ok)) == -1, (vw, vh)
    if lib.fspt_device_count() == 0:
        assert ev(L.fptr(img), 3, 2, None) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_host_validates():
    tun = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    for k in R.DEFAULTS:
        assert float(re.search(r"#define FSPT_BLOOM_%s (-?[0-9.eE+]+)f?\b" % k.upper(), tun).group(1)) == TR.BLOOM_DEFAULTS[k] == R.DEFAULTS[k]
    for name, want in (("MAX_LEVELS", R.MAX_LEVELS), ("CLAMP", R.CLAMP), ("TAIL_TEXELS", R.TAIL_TEXELS)):
        assert float(re.search(r"#define FSPT_BLOOM_%s ([0-9.]+)f?\b" % name, tun).group(1)) == want
    assert TR.BLOOM_MAX_LEVELS == R.MAX_LEVELS
    js = open(os.path.join(ROOT, "fspt_amd", "js", "fspt.js")).read()
    m = re.search(r"intensity: ([0-9.]+), scatter: ([0-9.]+), levels: ([0-9]+) };  // include/fspt_tuning.h FSPT_BLOOM", js)
    assert [float(x) for x in m.groups()] == [R.DEFAULTS[k] for k in R.DEFAULTS]
    p = TR._bloom_params({})
    assert (p.intensity, p.scatter, p.levels) == (float(F(0.05)), float(F(0.7)), 6)
    assert TR._bloom_params(dict(intensity=0.5, levels=3)).levels == 3
    for bad in BAD_PARAMS + (dict(levels=2.5), dict(levels=True)):
        with pytest.raises(ValueError, match="bloom"):
            TR._bloom_params(bad)
    with pytest.raises(TypeError, match="unknown bloom"):
        TR._bloom_params(dict(intensify=1.0))
    sig = inspect.signature(TR.PathTracer.set_bloom).parameters
    assert list(sig) == ["self", "on", "params"] and sig["on"].default is True
    assert isinstance(TR.PathTracer.bloom, property) and hasattr(TR.PathTracer, "bloom_last_ms")
    import fspt_amd
    assert fspt_amd.bloom_eval is TR.bloom_eval and fspt_amd.bloom_set_form is TR.bloom_set_form
    a4 = np.zeros((3, 2, 4), F)
    for args, kw in (((a4[..., :3],), {}), ((a4,), dict(viewport=(3, 3))), ((a4,), dict(viewport=(0, 1))), ((a4,), dict(intensity=-1.0))):
        with pytest.raises(ValueError):
            TR.bloom_eval(*args, **kw)
    from fspt_amd import scene_file as SF
    assert SF._bloom_params(None) is None and SF._bloom_params(False) is None
    assert SF._bloom_params(True) == {} and SF._bloom_params({"intensity": 0.2}) == {"intensity": 0.2}
    for name in ("render_frame", "render_sequence"):
        assert inspect.signature(getattr(SF, name)).parameters["bloom"].default is None
    for bad, exc in (({"intensity": -1.0}, ValueError), ({"intense": 1.0}, TypeError)):
        with pytest.raises(exc):
            SF.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, bloom=bad)
        with pytest.raises(exc):
            SF.render_frame(None, {}, 8, 8, bloom=bad)


def test_cli_refuses_what_it_cannot_honour():
    run = lambda *a: subprocess.run([sys.executable, "-m", "fspt_amd.render", *a], cwd=ROOT, capture_output=True, text=True)
    for bad in ("-0.5", "1.5", "nan", "inf"):
        r = run("--bloom=" + bad, "--out", "x.png")
        assert r.returncode == 2 and "--bloom INTENSITY must be a finite value in [0, 1]" in r.stderr, bad
    assert "--bloom [INTENSITY]" in run("--help").stdout


# ---- the restatement's identities -------------------------------------------------------------------------------------
def test_level_count_follows_the_size_rule():
    want = {(1, 1): [], (1, 9): [], (9, 1): [], (2, 2): [(1, 1)], (3, 2): [(2, 1)], (5, 7): [(3, 4), (2, 2), (1, 1)],
            (1920, 1080): [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]}
    for (w, h), lv in want.items():
        assert R.sizes(w, h) == lv, (w, h)
        assert TR.bloom_levels(w, h) == lv, (w, h)  # (the library's own host arithmetic)
    assert len(R.sizes(1920, 1080, 8)) == 8 and R.sizes(1920, 1080, 8)[-1] == (8, 5) and len(R.sizes(5, 7, 2)) == 2
    assert len(TR.bloom_levels(1920, 1080, 8)) == 8 and len(TR.bloom_levels(5, 7, 2)) == 2
    n = C.c_uint32()
    assert L.lib().fspt_bloom_texels(1920, 1080, 6, C.byref(n)) == sum(w * h for w, h in want[(1920, 1080)]) and n.value == 6
    assert sum(w * h for w, h in R.sizes(1920, 1080, 8)) * 3 <= 1920 * 1080 + 3 * 4096  # the pyramid: at most a third of the accumulator


def test_constant_dyadic_image_is_constant_at_every_level():
    for W, H in ((5, 7), (50, 37), (131, 67)):
        img = R.image(W, H, "constant")
        c = img[0, 0, :3].astype(np.float64)
        for params in ({}, dict(scatter=0.25, intensity=1.0, levels=8), dict(scatter=1.0), dict(scatter=0.0, intensity=0.0)):
            r = R.pyramid(img, **params)
            for a in r["down"] + r["up"] + [r["bloom"], r["mix"]]:
                assert (a == c).all(), (W, H, params)


@pytest.mark.parametrize("k", [-3, 5])
def test_scaling_by_a_power_of_two_scales_every_output_exactly(k):
    rng = np.random.default_rng(4)
    img = np.ones((37, 50, 4), F)
    img[..., :3] = (2.0 ** rng.uniform(-4.0, 4.0, (37, 50, 3))).astype(F)  # (under the clamp at either scale)
    a = R.pyramid(img, scatter=0.5, intensity=0.25)
    scaled = img.copy(); scaled[..., :3] *= F(2.0 ** k)
    b = R.pyramid(scaled, scatter=0.5, intensity=0.25)
    for x, y in zip(a["down"] + a["up"] + [a["bloom"], a["mix"]], b["down"] + b["up"] + [b["bloom"], b["mix"]]):
        assert np.array_equal(x * 2.0 ** k, y)


def test_an_impulse_spreads_as_the_outer_product_of_the_taps():
    w4 = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
    img = np.zeros((16, 16, 4), F)
    img[8, 6, 0] = 64.0  # source (6, 8): output x gets tap i where 2x - 1 + i == 6 -> x = 2 (i = 3), x = 3 (i = 1)
    d1 = R.pyramid(img, levels=1)["down"][0][..., 0]
    want = np.zeros((8, 8))
    for x, i in ((2, 3), (3, 1)):
        for y, j in ((3, 3), (4, 1)):  # source y = 8: 2y - 1 + j == 8
            want[y, x] = 64.0 * w4[i] * w4[j]
    assert np.array_equal(d1, want) and d1.sum() == 64.0 * (4 / 8) ** 2
    # at the corner the clamp folds tap 0 onto tap 1: source (0, 0) reaches output 0 with weight (1 + 3) / 8 per axis
    img = np.zeros((16, 16, 4), F)
    img[0, 0, 1] = 64.0
    d1 = R.pyramid(img, levels=1)["down"][0][..., 1]
    assert d1[0, 0] == 64.0 * 0.25 and np.count_nonzero(d1) == 1
    # at the far edge of an odd level the last output's taps 2 and 3 fold onto the last texel
    img = np.zeros((5, 5, 4), F)
    img[4, 4, 2] = 64.0  # outputs 0..2; x = 2 reads 3, 4, 5 -> 4, 6 -> 4: weight (3 + 3 + 1) / 8
    d1 = R.pyramid(img, levels=1)["down"][0][..., 2]
    assert d1[2, 2] == 64.0 * (7 / 8) ** 2 and d1[1, 1] == 64.0 * (1 / 8) ** 2 and d1[1, 2] == 64.0 * (7 / 8) * (1 / 8) and d1[0].sum() == 0.0  # (x = 1 reads 1 .. 4: tap 3)


def test_scatter_0_and_intensity_0():
    img = R.image(17, 33, "noise")
    r = R.pyramid(img, scatter=0.0)
    assert all(np.array_equal(u, d) for u, d in zip(r["up"], r["down"]))  # U_k = D_k
    assert np.array_equal(r["bloom"], R.up(r["down"][0], 17, 33))        # B = up(D_1)
    for kind in ("noise", "special"):
        img = R.image(17, 33, kind)
        assert np.array_equal(R.pyramid(img, intensity=0.0)["mix"], R.sanitise(img[..., :3]))  # mix = s(input)
    s = R.sanitise(F([np.nan, -1.0, -np.inf, np.inf, 2000.0, 1024.0, 0.5, 1e-40, -0.0]))
    assert np.array_equal(s, [0.0, 0.0, 0.0, 1024.0, 1024.0, 1024.0, 0.5, float(F(1e-40)), 0.0])


def test_the_tent_and_the_bound():
    c0, c1 = R.tent_taps(7, 4)
    assert list(c0) == [0, 0, 1, 1, 2, 2, 3] and list(c1) == [0, 1, 0, 2, 1, 3, 2]
    u = R.up(np.arange(12.0).reshape(3, 4, 1), 7, 5)
    assert u.shape == (5, 7, 1) and u[0, 0, 0] == 0.0 and u[1, 1, 0] == 0.75 * (0.75 * 0 + 0.25 * 1) + 0.25 * (0.75 * 4 + 0.25 * 5)
    r = R.pyramid(R.image(50, 37, "noise"))
    assert r["n"] == 6 and r["mix_tol"].max() < 61 * 2.0 ** -24 * 1024 * 3 and r["mix_tol"][:37, :50].min() > 0
    assert all((t > 0).all() for t in r["down_tol"] + r["up_tol"])
    vp = R.pyramid(R.image(50, 37, "noise"), viewport=(23, 19))
    assert vp["bloom"].shape == (19, 23, 3) and np.array_equal(vp["mix"][19:], R.image(50, 37, "noise")[19:, :, :3]) and (vp["mix_tol"][:, 23:] == 0).all()
    sp = R.image(50, 37, "special")[..., :3]
    assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and (sp < 0).any() and ((sp > 0) & (sp < 1.2e-38)).any() and (sp > 1024).any()
    assert np.isfinite(R.pyramid(R.image(50, 37, "special"))["mix"]).all()


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("bloom_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "bloom_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "bloom_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_bloom_calls_and_handles(js_report):
    r = js_report
    f = lambda v: float(F(v))
    assert r["off"] is None
    assert r["defaults"] == {"intensity": f(0.05), "scatter": f(0.7), "levels": 106}
    assert r["some"] == {"intensity": 0.5, "scatter": f(0.7), "levels": 203}
    assert r["unknown"] == "RangeError: setBloom: unknown parameter intensify"
    assert r["not_a_number"].startswith("TypeError") and r["fraction"].startswith("RangeError")
    assert all(b is not None for b in r["bad"])
    assert r["kept"] == r["some"], "a refused call changed the parameters"
    assert "handle" in r["scene_as_target"] and r["too_few"] is not None
    assert r["during"] == ["Error: render in flight"] * 2 and r["after"] is None
    assert r["off_again"] is None
    assert "destroyed" in r["closed"]
