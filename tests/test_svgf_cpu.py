"""SVGF variance guidance (fspt_temporal_set_moments / fspt_temporal_denoise_variance), the part that needs no
GPU: the entry points exist and check their arguments, the Python host validates, the float64 restatement the GPU tests
compare against (tests/svgf_ref.py) has the identities the rule promises, and the Node host runs on the mock library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import atrous_inputs as I
import atrous_ref as A
import svgf_ref as V
from fspt_amd import _lib as L
from fspt_amd import tracer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ("fspt_temporal_set_moments", "fspt_temporal_denoise_variance")
TUNING = ("fspt_temporal_read_variance", "fspt_svgf_last_ms", "fspt_svgf_eval")


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
    lib = L.lib()
    buf = np.zeros(16, np.float32)
    assert lib.fspt_temporal_set_moments(None, 1) == -1
    assert b"fspt_temporal_set_moments: NULL argument" in lib.fspt_last_error()
    assert lib.fspt_temporal_denoise_variance(None, None, L.fptr(buf)) == -1
    assert lib.fspt_temporal_read_variance(None, L.fptr(buf), L.fptr(buf)) == -1
    assert lib.fspt_svgf_last_ms(None, L.fptr(buf)) == -1
    assert b"NULL" in lib.fspt_last_error()
    assert lib.fspt_abi_version() == 4  # entry points are only added


BAD_PARAMS = [dict(iterations=17), dict(sigma_color=-1.0), dict(sigma_color=float("nan")), dict(sigma_normal=-1.0),
              dict(sigma_normal=float("inf")), dict(sigma_depth=0.0), dict(sigma_depth=float("nan"))]


def test_library_refuses_bad_parameters():
    """fspt_svgf_eval checks NULL arguments and the parameter ranges before it looks for a device"""
    lib = L.lib()
    a4, a2, a8, out, v = (np.zeros((2, 2, c), np.float32) for c in (4, 2, 8, 4, 1))
    args = (L.fptr(a4), L.fptr(a2), L.fptr(a8))
    for bad in BAD_PARAMS:
        p = {**V.DEFAULTS, **bad}
        prm = L.DenoiseParams(p["iterations"], p["sigma_color"], p["sigma_normal"], p["sigma_depth"])
        assert lib.fspt_svgf_eval(0, *args, 2, 2, 1, C.byref(prm), L.fptr(out), L.fptr(v), L.fptr(v)) == -1, bad
        assert b"fspt_svgf_eval: need iterations <= 16" in lib.fspt_last_error()
    assert lib.fspt_svgf_eval(0, *args, 2, 2, 0, None, L.fptr(out), None, None) == -1  # n = 0
    assert lib.fspt_svgf_eval(0, *args, 2, 2, 1, None, None, None, None) == -1        # NULL out
    assert lib.fspt_svgf_eval(0, args[0], None, args[2], 2, 2, 1, None, L.fptr(out), None, None) == -1  # NULL moments
    if lib.fspt_device_count() == 0:
        for prm in (None, L.DenoiseParams(0, float("inf"), 0.0, float("inf")), L.DenoiseParams(16, 0.0, 1e9, 1e-30)):
            assert lib.fspt_svgf_eval(0, *args, 2, 2, 1, C.byref(prm) if prm else None, L.fptr(out), None, None) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_host_validates():
    assert TR.SVGF_DEFAULTS == V.DEFAULTS
    hdr = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    for k, name in (("iterations", "ITERATIONS"), ("sigma_color", "SIGMA_L"), ("sigma_normal", "SIGMA_NORMAL"), ("sigma_depth", "SIGMA_DEPTH")):
        assert float(re.search(r"#define FSPT_SVGF_%s ([0-9.eE+-]+)f?\b" % name, hdr).group(1)) == V.DEFAULTS[k]
    for bad in BAD_PARAMS + [dict(iterations=2.5), dict(iterations=-1)]:
        with pytest.raises(ValueError):
            TR._svgf_params(bad)
    with pytest.raises(TypeError):
        TR._svgf_params(dict(alpha=1.0))
    assert TR._svgf_params({}) is None and TR._svgf_params(dict(iterations=None)) is None
    p = TR._svgf_params(dict(sigma_color=2.0))
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth) == (4, 2.0, 32.0, np.float32(0.05))
    assert TR._svgf_params(dict(iterations=3)).sigma_color == 8.0
    assert TR._svgf_params(dict(sigma_color=float("inf"))).sigma_color == float("inf")
    a4, a2, a8 = np.zeros((3, 2, 4), np.float32), np.zeros((3, 2, 2), np.float32), np.zeros((3, 2, 8), np.float32)
    for args in ((a4[..., :3], a2, a8), (a4, a4, a8), (a4, a2, a4), (a4, a2[:2], a8)):
        with pytest.raises(ValueError):
            TR.svgf_eval(*args)
    with pytest.raises(ValueError):
        TR.svgf_eval(a4, a2, a8, n=0)
    for name in ("temporal_set_moments", "temporal_variance", "svgf_last_ms"):
        assert hasattr(TR.PathTracer, name)
    import inspect
    assert "variance" in inspect.signature(TR.PathTracer.temporal_denoise).parameters
    import fspt_amd
    assert fspt_amd.svgf_eval is TR.svgf_eval
    from fspt_amd import scene_file as F
    assert "variance" in inspect.signature(F.render_sequence).parameters
    with pytest.raises(ValueError, match="variance needs temporal"):
        F.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, bvh="refit", variance=True)
    with pytest.raises(ValueError, match="variance needs temporal"):
        F.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, bvh="refit", temporal=True, variance=True)


def test_cli_refuses_variance_guided_without_temporal():
    import subprocess, sys
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--variance-guided", "--out", "x.png"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--variance-guided needs --temporal and --atrous K" in r.stderr


# ---- the restatement's identities -------------------------------------------------------------------------------------
def test_sigma_l_inf_is_the_unguided_colour_weight():
    """sl = +inf reproduces atrous_ref with sigma_color = +inf exactly, whatever the variance"""
    acc, f = I.synthetic(40, 56)
    var = np.random.default_rng(1).uniform(0, 1e6, acc.shape[:2])
    for k in (0, 1, 3, 5):
        for rest in (dict(), dict(sigma_normal=0.0), dict(sigma_depth=np.inf), dict(sigma_normal=0.0, sigma_depth=np.inf)):
            got, _ = V.guided_atrous(acc, var, f, iterations=k, sigma_color=np.inf, **rest)
            want = A.atrous(acc, f, iterations=k, sigma_color=np.inf, **{**dict(sigma_normal=32.0, sigma_depth=0.05), **rest})
            assert np.array_equal(got, want, equal_nan=True), (k, rest)


def flat_features(H, W):
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = (0.5, 0.25, 0.75); f[..., 3] = 2.0; f[..., 6] = 1.0; f[..., 7] = 1.0
    return f


def test_constant_image_zero_variance_passes_unchanged():
    H, W = 20, 28
    f = flat_features(H, W)
    hist = np.zeros((H, W, 4), np.float32)
    hist[..., :3] = (0.25, 0.5, 0.125); hist[..., 3] = np.where(np.arange(W) % 2, 16.0, 2.0)  # both variance branches
    m = np.zeros((H, W, 2)); m[..., 0] = 3.0; m[..., 1] = 9.0  # M2 = M1 M1, and every weighted sum of them is exact
    for k in (1, 4):
        out, v, vk, _ = V.svgf(hist, m, f, 2, iterations=k)
        assert (v == 0).all() and (vk == 0).all()
        assert np.allclose(out[..., :3], hist[..., :3], rtol=1e-14) and (out[..., 3] == 1).all()


def test_variance_of_an_unguided_iteration_is_the_b3_closed_form():
    """all edge weights off: var' = sum B^2 var / (sum B)^2 - for a constant variance c away from the border, c (sum_i B_i^2)^2
    = c (70 / 256)^2, and twice that factor after two iterations"""
    H, W = 40, 40
    f = flat_features(H, W)
    hist = np.random.default_rng(2).uniform(0, 1, (H, W, 4)).astype(np.float32)
    var = np.full((H, W), 3.0)
    off = dict(sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf)
    b2 = float((V.B3 ** 2).sum()) ** 2
    assert b2 == (70.0 / 256.0) ** 2
    _, v1 = V.guided_atrous(hist, var, f, iterations=1, **off)
    assert np.allclose(v1[2:-2, 2:-2], 3.0 * b2, rtol=1e-14)
    _, v2 = V.guided_atrous(hist, var, f, iterations=2, **off)
    assert np.allclose(v2[6:-6, 6:-6], 3.0 * b2 * b2, rtol=1e-14)
    # at the corner the 3 x 3 taps that are left: sum B^2 / (sum B)^2 of (6, 4, 1) / 16 per axis
    c = (36 + 16 + 1) / (6 + 4 + 1) ** 2
    assert np.isclose(v1[0, 0], 3.0 * c * c, rtol=1e-14)


def test_temporal_and_spatial_estimates_agree_on_iid_noise():
    """A field of independent values l ~ N(mu, s^2), one per pixel, with M = (l, l l) and flat features: the 7 x 7 fallback
    (Fe = 1) estimates s^2 (49 - 1) / 49 from 49 samples; the relative spread of a 49-sample variance of a normal is
    sqrt(2 / 48) = 0.204, so the mean over the 34 x 34 interior pixels (about 23 independent windows) lies within
    4 x 0.204 / sqrt(23) = 17 % of it.  The temporal branch on the moments of 49 such values per pixel (Fe = 49) gives
    the variance of the MEAN, the same sample variance / 49, from 1 600 independent pixels."""
    H, W, mu, s = 40, 40, 5.0, 0.7
    rng = np.random.default_rng(11)
    f = flat_features(H, W)
    l = rng.normal(mu, s, (H, W))
    hist = np.ones((H, W, 4)); hist[..., 3] = 1.0
    v_sp, _ = V.variance(hist, np.stack([l, l * l], -1), f, 1)
    inner = v_sp[3:-3, 3:-3]
    assert abs(inner.mean() / (s * s * 48 / 49) - 1) < 0.17
    ls = rng.normal(mu, s, (49, H, W))
    hist[..., 3] = 49.0
    v_t, _ = V.variance(hist, np.stack([ls.mean(0), (ls * ls).mean(0)], -1), f, 1)
    assert abs(v_t.mean() * 49 / (s * s * 48 / 49) - 1) < 4 * 0.204 / np.sqrt(H * W)  # 1 600 independent pixels: 2 %
    # per pixel both are a 49-sample variance: the same expected value, a ratio of means near 1
    assert abs(v_t.mean() * 49 / inner.mean() - 1) < 0.2
    # Fe between 1 and 4 divides the spatial estimate; Fe below 1 does not
    hist[..., 3] = 2.0
    assert np.allclose(V.variance(hist, np.stack([l, l * l], -1), f, 1)[0], v_sp / 2)
    hist[..., 3] = 1.0
    assert np.allclose(V.variance(hist, np.stack([l, l * l], -1), f, 2)[0], v_sp)


def test_blend_of_the_moments_is_the_colour_blend():
    """static view, single tap: Mout = Hm + (m - Hm) n / (N + n); without a history: m"""
    import temporal_ref as T
    H, W = 6, 9
    G = np.zeros((H, W, 8), np.float32)
    G[..., 0] = 2.0; G[..., 6] = 1.0; G[..., 7] = 1.0
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    M = np.stack([xs, ys, np.full_like(xs, 2.0), np.ones_like(xs)], -1)
    f = flat_features(H, W)
    rng = np.random.default_rng(5)
    acc = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    hist = rng.uniform(0, 2, (H, W, 4)).astype(np.float32); hist[..., 3] = 6.0
    mh = rng.uniform(0, 2, (H, W, 2)).astype(np.float32)
    m = V.frame_moments(acc, f)
    assert np.array_equal(V.blend_moments(acc, M, G, None, None, None, f, 2), m)
    assert np.array_equal(V.blend_moments(acc, M, G, hist, None, G, f, 2), m)
    got = V.blend_moments(acc, M, G, hist, mh, G, f, 2)
    assert np.allclose(got, mh + (m - mh) * (2 / 8), rtol=1e-14)
    # a rejected history (depth): m
    gp = G.copy(); gp[..., 0] = 3.0
    assert np.array_equal(V.blend_moments(acc, M, G, hist, mh, gp, f, 2), m)


def test_synthetic_history_reaches_both_branches_and_extremes():
    hist, mom, f = V.synthetic_history(80, 120, n=2)
    Fe = hist[..., 3] / 2
    assert (Fe < 1).any() and (Fe == 4).any() and ((Fe > 1) & (Fe < 4)).any() and (Fe > 4).any()
    v, _ = V.variance(hist, mom, f, 2)
    assert np.isfinite(v).all() and ((v == 0) & (Fe >= 4) & (mom[..., 0] > 0)).sum() > 100 and (v > 1e9).sum() > 100


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("svgf_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "temporal_mock_stub.c"), os.path.join(ROOT, "tests", "svgf_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "svgf_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_variance_calls_and_handles(js_report):
    r = js_report
    f = lambda x: float(np.float32(x))
    assert r["off"] is not None and r["off_again"] is not None  # the library's FSPT_E_STATE comes up as an Error
    assert r["d1"] == [-1.0, 0.0, 0.0, 0.0, 1.0, 1.0] and r["d1_type"] == "Float32Array" and r["d1_len"] == 24  # defaults go down as NULL
    assert r["d2"] == [3.0, 2.5, 32.0, f(0.05), 1.0, 1.0]
    assert r["same_buffer"] is True and r["no_readback"] is True
    assert r["short_out"] == "RangeError: temporalDenoiseVariance: need W*H*4 floats"
    assert r["bad_iterations"] == "RangeError: fspt_napi: iterations must be an integer in [0, 16]"
    assert r["bad_sigma"] is not None
    assert r["addon_len"].startswith("RangeError")
    assert all("handle" in c for c in r["scene_as_target"])
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["after"] is None and r["sets"] == 3.0
    assert all("destroyed" in c for c in r["closed"])


def test_per_pixel_bound_covers_a_perturbed_run():
    """svgf_ref.guided_atrous_bounded is guided_atrous plus a bound: the same output, and the restatement run on inputs off
    by one float32 rounding (the least any float32 run is off by) stays inside the bound at every value, on the set with
    exact zeros and huge variances and on the floored one"""
    import svgf_ref as V
    for floor in (False, True):
        hist, mom, f = V.synthetic_history(40, 56, n=2, floor=floor)
        v = V.variance(hist, mom, f, 2)[0].astype(np.float32)
        rng = np.random.default_rng(7)
        bent = hist.astype(np.float64)
        bent[..., :3] *= 1 + V.U32 * rng.uniform(-1, 1, bent[..., :3].shape)
        for K in (1, 3, 5):
            out, vk, E, Av = V.guided_atrous_bounded(hist, v, f, iterations=K)
            ref, ref_vk = V.guided_atrous(hist, v, f, iterations=K)
            assert np.allclose(out, ref, rtol=1e-12, atol=0) and np.allclose(vk, ref_vk, rtol=1e-12, atol=0)
            assert np.isfinite(E).all() and np.isfinite(Av).all()
            o2, v2 = V.guided_atrous(bent, v, f, iterations=K)
            assert (np.abs(o2[..., :3] - ref[..., :3]) <= E).all() and (np.abs(v2 - ref_vk) <= Av).all()
            if K <= 3:  # (and it is no formality: 0.84-1.00 of the values within 1e-3 relative)
                assert (E <= 1e-3 * np.abs(ref[..., :3]) + 1e-5).mean() > 0.8
