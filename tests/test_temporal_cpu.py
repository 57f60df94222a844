"""Temporal accumulation (fspt_temporal_*), the part that needs no GPU: the entry points exist and check their
arguments, the Python host validates parameters, and the float64 restatement the GPU tests compare against
(tests/temporal_ref.py) has the identities the rule promises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import rebuild_ref as RB
import temporal_ref as T
from refit_moves import rotated
from fspt_amd import _lib as L
from fspt_amd import tracer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ("fspt_temporal_accumulate", "fspt_temporal_reset", "fspt_temporal_denoise", "fspt_temporal_draw",
            "fspt_scene_motion_begin", "fspt_scene_motion_end")
TUNING = ("fspt_temporal_read_gbuffer", "fspt_temporal_last_ms", "fspt_temporal_eval", "fspt_scene_slot_triangles")


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
    cp = L.CameraParams()
    buf = np.zeros(16, np.float32)
    u8 = np.zeros(16, np.uint8)
    assert lib.fspt_temporal_accumulate(None, C.byref(cp), None, None) == -1
    assert b"fspt_temporal_accumulate: NULL argument" in lib.fspt_last_error()
    assert lib.fspt_temporal_reset(None) == -1
    assert lib.fspt_temporal_denoise(None, None, L.fptr(buf)) == -1
    assert lib.fspt_temporal_draw(None, 1.0, 1.0, 0, L.u8ptr(u8)) == -1
    assert lib.fspt_temporal_read_gbuffer(None, L.fptr(buf), L.fptr(buf)) == -1
    assert lib.fspt_temporal_last_ms(None, L.fptr(buf)) == -1
    assert lib.fspt_scene_motion_begin(None) == -1 and lib.fspt_scene_motion_end(None) == -1
    assert lib.fspt_scene_slot_triangles(None, None, None) == -1
    assert b"NULL" in lib.fspt_last_error()


BAD_PARAMS = [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(max_history=0.5), dict(max_history=float("nan")),
              dict(depth_tol=-1.0), dict(normal_cos=1.5), dict(normal_cos=-1.5), dict(normal_cos=float("nan"))]


def test_library_refuses_bad_parameters():
    """fspt_temporal_eval checks NULL arguments and the parameter ranges before it looks for a device"""
    lib = L.lib()
    a4, a8, out = np.zeros((2, 2, 4), np.float32), np.zeros((2, 2, 8), np.float32), np.zeros((2, 2, 4), np.float32)
    args = (L.fptr(a4), L.fptr(a4), L.fptr(a8), L.fptr(a4), L.fptr(a8))
    for bad in BAD_PARAMS:
        prm = L.TemporalParams(**{**T.DEFAULTS, **bad})
        assert lib.fspt_temporal_eval(0, *args, 2, 2, 1, C.byref(prm), L.fptr(out)) == -1, bad
        assert b"alpha in [0, 1]" in lib.fspt_last_error()
    assert lib.fspt_temporal_eval(0, *args, 2, 2, 0, None, L.fptr(out)) == -1  # n = 0
    assert lib.fspt_temporal_eval(0, *args, 2, 2, 1, None, None) == -1       # NULL out
    assert lib.fspt_temporal_eval(0, args[0], args[1], args[2], args[3], None, 2, 2, 1, None, L.fptr(out)) == -1  # hist without g_prev
    if lib.fspt_device_count() == 0:
        for prm in (None, L.TemporalParams(0.2, 8.0, 0.0, -1.0), L.TemporalParams(1.0, 1.0, 1e9, 1.0)):
            assert lib.fspt_temporal_eval(0, *args, 2, 2, 1, C.byref(prm) if prm else None, L.fptr(out)) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()


def test_python_host_validates():
    assert TR.TEMPORAL_DEFAULTS == T.DEFAULTS
    hdr = open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    for k, v in TR.TEMPORAL_DEFAULTS.items():
        assert float(re.search(r"#define FSPT_TEMPORAL_%s ([0-9.eE+-]+)f" % k.upper(), hdr).group(1)) == v
    js = open(os.path.join(ROOT, "fspt_amd", "js", "fspt.js")).read()
    jd = re.search(r"const d = \{ alpha: ([0-9.]+), maxHistory: ([0-9.]+), depthTol: ([0-9.]+), normalCos: ([0-9.]+) \};", js)
    assert [float(x) for x in jd.groups()] == [T.DEFAULTS[k] for k in ("alpha", "max_history", "depth_tol", "normal_cos")]  # the JS copy
    for bad in BAD_PARAMS:
        with pytest.raises(ValueError):
            TR._temporal_params(bad)
    with pytest.raises(TypeError):
        TR._temporal_params(dict(sigma=1.0))
    assert TR._temporal_params({}) is None
    p = TR._temporal_params(dict(alpha=0.25))
    assert (p.alpha, p.max_history, p.depth_tol) == (0.25, 64.0, np.float32(0.05))
    a4, a8 = np.zeros((3, 2, 4), np.float32), np.zeros((3, 2, 8), np.float32)
    for args in ((a4[..., :3], a4, a8), (a4, a8, a8), (a4, a4, a4), (a4, a4, a8, a4, None), (a4, a4, a8, a4, a4)):
        with pytest.raises(ValueError):
            TR.temporal_eval(*args)
    with pytest.raises(ValueError):
        TR.temporal_eval(a4, a4, a8, n=0)
    for name in ("temporal_accumulate", "temporal_reset", "temporal_denoise", "temporal_draw", "temporal_gbuffer"):
        assert hasattr(TR.PathTracer, name)
    assert hasattr(TR.Scene, "motion_begin") and hasattr(TR.Scene, "motion_end")
    from fspt_amd import scene_file as F
    with pytest.raises(ValueError, match="refit"):
        F.render_sequence("x{frame}.json", range(2), "o{frame}.png", 8, 8, temporal=True)


# ---- the restatement's identities -------------------------------------------------------------------------------------
def oracle_gbuffer(arrays, W, H, cam):
    """G as the rule defines it, from the oracle's first hits on the restatement's centre rays"""
    o, d = T.centre_rays(W, H, cam["P"], cam["I"], cam["fov_scale"])
    pos = np.zeros((H, W, 4), np.float32); pos[..., :3] = o
    d4 = np.zeros((H, W, 4), np.float32); d4[..., :3] = d
    fh = O.trace(arrays, W, H, pos, d4, 0, 0.5, 0.0, 4, np.zeros((H, W, 4), np.float32), first_hits=True).reshape(H, W)
    hit = fh["index"] >= 0
    G = np.zeros((H, W, 8), np.float32)
    G[..., 0] = np.where(hit, fh["t"], np.float32(T.MAX_T))
    G[..., 1] = np.where(hit, fh["index"], -1).astype(np.int32).view(np.float32)  # (the triangle stands in for the slot here)
    G[..., 2:4] = np.where(hit[..., None], fh["bary"][..., 1:3], 0)
    G[..., 4:7] = np.where(hit[..., None], fh["macro_normal"], 0)
    G[..., 7] = hit
    return G, d


GBUFFER_CASES = [(name, W, H) for name in ("small", "textured") for W, H in ((96, 64), (67, 45))]  # tests/test_temporal_gpu.py's


@pytest.mark.parametrize("name,W,H", GBUFFER_CASES)
def test_gbuffer_exempt_share_of_the_test_cameras(small_scene, camera, name, W, H):
    """The pixels the GPU G-buffer test exempts - the restatement's own float64 triangle differs from the oracle's on the
    float32 centre rays - are decided here, without a GPU, and stay under 1 % for the cameras and shapes that test uses."""
    from fspt_amd import scene as S
    arrays = {"small": small_scene, "textured": S.textured_test_scene()}[name]
    o, d = T.centre_rays(W, H, camera["P"], camera["I"], camera["fov_scale"])
    t32, idx32 = O.intersect(arrays, T.rays6(o, d))[:2]
    exempt, t64, idx64, bv, bw = T.gbuffer_exempt(arrays, W, H, camera["P"], camera["I"], camera["fov_scale"], idx32)
    print("exempt", name, W, H, int(exempt.sum()))
    assert exempt.sum() <= 0.01 * W * H
    ok = ~exempt & (idx64 >= 0)
    assert 0 < ok.sum() < W * H
    # where they agree on the triangle they agree on the distance and the weights to float32 rounding of a well-conditioned hit
    assert np.allclose(np.asarray(t32).reshape(H, W)[ok], t64[ok], rtol=1e-4)
    G, _ = oracle_gbuffer(arrays, W, H, camera)
    assert np.allclose(G[..., 2][ok], bv[ok], atol=1e-3) and np.allclose(G[..., 3][ok], bw[ok], atol=1e-3)


def test_same_camera_static_scene_is_the_identity(small_scene, camera):
    """integer sample positions, a single tap of weight 1, every hit pixel valid: the blend is the running mean"""
    W, H = 48, 36
    cam3 = (camera["P"], camera["I"], camera["fov_scale"])
    G, d = oracle_gbuffer(small_scene, W, H, camera)
    hit = G[..., 7] != 0
    assert 0 < hit.sum() < W * H
    m = T.motion(G, d, cam3, cam3)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    assert np.abs(m["sx_raw"] - xs).max() < 1e-3 and np.abs(m["sy_raw"] - ys).max() < 1e-3  # float32 t and d, float64 after
    assert np.array_equal(m["sx"], xs) and np.array_equal(m["sy"], ys)
    assert np.array_equal(m["kind"], np.where(hit, 1.0, 2.0))
    assert np.allclose(m["dist"][hit], G[..., 0][hit], rtol=1e-6)
    M = np.stack([m["sx"], m["sy"], m["dist"], m["kind"]], -1).astype(np.float32)
    rng = np.random.default_rng(3)
    hist = rng.uniform(0, 2, (H, W, 4)).astype(np.float32); hist[..., 3] = 16
    I = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    out, margin = T.blend(I, M, G, hist, G, 4)
    assert np.isfinite(margin[hit]).all() and (margin[hit] > 1e-3).all()  # no self-rejection anywhere near
    want = hist[..., :3].astype(np.float64) + (I[..., :3].astype(np.float64) - hist[..., :3]) * (4 / 20)
    assert np.allclose(out[..., :3], want, rtol=1e-12) and (out[..., 3] == 20).all()
    f32 = T.running_mean_f32(hist, I, 4)
    assert np.allclose(f32, out, rtol=1e-6)


def synthetic(H=5, W=7):
    G = np.zeros((H, W, 8), np.float32)
    G[..., 0] = 2.0; G[..., 1] = np.int32(0).view(np.float32); G[..., 6] = 1.0; G[..., 7] = 1.0
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    M = np.stack([xs, ys, np.full_like(xs, 2.0), np.ones_like(xs)], -1)
    return G, M


def test_constant_history_constant_frame_and_clamps():
    G, M = synthetic()
    M[..., 0] += 0.25; M[..., 1] -= 0.5  # four taps, some outside the image
    hist = np.full(G.shape[:2] + (4,), 0.75, np.float32); hist[..., 3] = 8
    I = np.full(G.shape[:2] + (4,), 0.75, np.float32); I[..., 3] = 1
    out, _ = T.blend(I, M, G, hist, G, 2)
    assert np.allclose(out[..., :3], 0.75, rtol=1e-15) and (out[..., 3] == 10).all()
    # max_history clamps the length before the blend weight is taken and after
    hist[..., 3] = 100
    out, _ = T.blend(2 * I, M, G, hist, G, 2, max_history=6.0)
    assert (out[..., 3] == 6).all() and np.allclose(out[..., :3], 0.75 + 0.75 * (2 / 8), rtol=1e-15)
    # alpha = 1 returns I; no history returns I with length n (clamped)
    out, _ = T.blend(2 * I, M, G, hist, G, 2, alpha=1.0)
    assert np.array_equal(out[..., :3], (2 * I)[..., :3].astype(np.float64))
    out, _ = T.blend(2 * I, M, G, None, None, 9, max_history=4.0)
    assert np.array_equal(out[..., :3], (2 * I)[..., :3].astype(np.float64)) and (out[..., 3] == 4).all()


def test_validity_tests_reject():
    G, M = synthetic()
    hist = np.ones(G.shape[:2] + (4,), np.float32); hist[..., 3] = 4
    I = np.zeros(G.shape[:2] + (4,), np.float32)
    for change in ("depth", "normal", "miss", "behind", "outside"):
        gp, m = G.copy(), M.copy()
        if change == "depth":
            gp[..., 0] = 2.0 * 1.06
        elif change == "normal":
            gp[..., 4:7] = (1, 0, 0)
        elif change == "miss":
            gp[..., 7] = 0
        elif change == "behind":
            m[..., 3] = 0
        else:
            m[..., 0] = -5
        out, _ = T.blend(I, m, G, hist, gp, 3)
        assert (out[..., :3] == 0).all() and (out[..., 3] == 3).all(), change
    out, _ = T.blend(I, M, G, hist, G, 3)
    assert np.allclose(out[..., :3], 4 / 7) and (out[..., 3] == 7).all()


def test_rebuild_order_keeps_slot_correspondence(small_scene):
    """A snapshot taken before a move, permuted by the order the rebuild returns, still holds in position k the OLD
    vertices of the triangle that the rebuilt scene holds in position k."""
    a = small_scene
    tri1, norm1 = rotated(a.tri, a.norm)
    order, fresh = RB.expected(a, tri1, norm1)
    assert not np.array_equal(order, np.arange(a.n_tris))
    ident = np.arange(a.n_tris)
    snap = T.snapshot_from_triangles(a.tri, ident)           # per triangle, old leaf order
    perm = T.permute_snapshot(snap, order)
    assert np.array_equal(perm, T.snapshot_from_triangles(a.tri.reshape(-1, 9)[order.astype(np.int64)], ident))
    # the moved triangle in new position k is the rotation of the snapshot's triangle in position k
    want, _ = rotated(a.tri, a.norm)
    assert np.array_equal(fresh.tri.reshape(-1, 9), want.reshape(-1, 9)[order.astype(np.int64)])
    assert np.allclose(fresh.tri.reshape(-1, 9)[:, :3] - perm[:, :3], (want.reshape(-1, 9) - a.tri.reshape(-1, 9))[order.astype(np.int64)][:, :3], atol=1e-6)


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("temporal_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "temporal_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "temporal_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_temporal_calls_and_handles(js_report):
    """The Node host's temporal calls on the mock library: defaults go down as NULL, given parameters as given, the camera is
    the tracer's, bad parameters and arrays are refused before the library, handles are guarded during a renderAsync."""
    r = js_report
    f = lambda x: float(np.float32(x))
    assert "fspt_temporal_draw" in r["draw_before"] or "Error" in r["draw_before"]
    assert r["h1"] == [0.0, 64.0, f(0.05), f(0.95), 1.0, 0.0, 0.75] and r["h1_type"] == "Float32Array" and r["h1_len"] == 24
    assert r["h2"] == [0.25, 8.0, f(0.05), f(0.95), 2.0, 2.0, 0.75]
    assert r["same_buffer"] is True and r["h3"] == [3.0, 0.0]
    for k in ("alpha", "history", "depth", "normal", "nan"):
        assert r["bad_" + k] == "RangeError: temporalAccumulate: need alpha in [0, 1], maxHistory >= 1, depthTol >= 0, normalCos in [-1, 1]", k
    assert r["bad_unknown"] == "RangeError: temporalAccumulate: unknown parameter sigma"
    assert r["short_out"] == "RangeError: temporalAccumulate: need W*H*4 floats"
    assert r["no_readback"] is True
    assert r["calls_after_refused"] == 5.0
    assert r["denoise"] == [3.0] and r["denoise_default"] == [-1.0]
    assert r["draw"] == [12, 9, 1]
    assert r["draw_short"] == "RangeError: temporalDraw: need W*H*4 bytes"
    assert r["addon_range"].startswith("RangeError: fspt_napi: temporalAccumulate needs alpha in [0, 1]")
    assert r["addon_len"].startswith("RangeError")
    assert "handle" in r["scene_as_target"] and "handle" in r["target_as_scene"]
    assert r["during"] == ["Error: render in flight"] * 6
    assert r["after"] is None and r["calls_after_reset"] == 1.0
    assert all("destroyed" in c for c in r["closed"])
