"""Temporal accumulation on the GPU (fspt_temporal_*) against the float64 restatement of tests/temporal_ref.py
and the oracle.

Float32 bounds used below, EPS = 2^-24 (half an ulp, the error of one correctly rounded operation):
  * G-buffer: the GPU's centre ray and the restatement's are the same float32 operations on the same inputs, and the oracle
    computes t, the barycentric weights and macroNormal from that ray with the arithmetic the kernels share with it, so G
    is compared EXACTLY on every pixel that is not exempt; the exempt pixels - where the float64 restatement's own closest
    triangle (tests/temporal_ref.py closest_hit) differs from the oracle's - are decided without the GPU and capped at 1 %.
  * motion: v = X' - P_prev has ~6 roundings of terms of magnitude |X'| + |P_prev| + |v| behind it (t d + P or the two fma
    chains of the snapshot, the subtraction, the float32 basis: 3 more roundings per component), each of the three dot
    products adds 3, the two divisions and the map to pixels 6: the relative error of icx / icy is below 24 EPS x scale with
    scale = (|X'| + |P_prev| + |v|) / (a |I| fov) (tests/temporal_ref.py returns it), which is W / 2 (H / 2) pixels per
    unit: |dsx| <= 24 EPS scale W / 2 + 8 EPS (|sx| + W).  MOTION_OPS = 24 below.  A pixel whose unsnapped coordinate lies
    within that bound of the snap threshold may snap either way and is compared against both.
  * blend: at most 4 taps, 4 fma and one division per channel, the blend 4 operations: 16 EPS relative to the largest
    magnitude involved; BLEND_RTOL = 2e-6 > 16 EPS.  Taps whose depth or normal test lies within 1e-5 of its threshold
    (relative; float32 evaluates depth_tol * M.z and the dot product with 3-4 roundings = 2.4e-7) are exempt.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import temporal_ref as T
from refit_moves import rotated
from fspt_amd import PathTracer, _lib as L, denoise_eval, scene as S, temporal_eval

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
MOTION_OPS = 24
BLEND_RTOL = 2e-6


def make_pt(arrays, W, H, cam):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    return pt


def moved_camera(camera, kind):
    c = dict(camera)
    P, I = np.array(c["P"], np.float64), np.array(c["I"], np.float64)
    if kind == "translate":
        c["P"] = list(P + [0.11, 0.04, -0.07])
    elif kind == "rotate":
        th = np.radians(4.0)
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        c["I"] = list(R @ I)
    elif kind == "fov":
        c["fov_scale"] = c["fov_scale"] * 1.3
    elif kind == "behind":  # far beyond the scene, looking on: everything the other camera sees lies behind this one
        c["P"] = list(P + 2.2 * I / np.linalg.norm(I) * np.linalg.norm(P))
    return c


def frame(pt, cam, n=2, seed=5, **params):
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.clear()
    pt.seed(seed)
    pt.render(n)
    return pt.temporal_accumulate(**params)


# ---- 1. the G-buffer ------------------------------------------------------------------------------------------------
def oracle_first_hits(arrays, W, H, cam):
    o, d = T.centre_rays(W, H, cam["P"], cam["I"], cam["fov_scale"])
    pos = np.zeros((H, W, 4), np.float32); pos[..., :3] = o
    d4 = np.zeros((H, W, 4), np.float32); d4[..., :3] = d
    return O.trace(arrays, W, H, pos, d4, 0, 0.5, 0.0, 4, np.zeros((H, W, 4), np.float32), first_hits=True).reshape(H, W), o, d


@pytest.mark.parametrize("W,H", [(96, 64), (67, 45)])
@pytest.mark.parametrize("name", ["small", "textured"])
def test_gbuffer_matches_intersect_and_oracle(small_scene, camera, name, W, H):
    arrays = {"small": small_scene, "textured": S.textured_test_scene()}[name]
    pt = make_pt(arrays, W, H, camera)
    pt.render(1)
    pt.temporal_accumulate()
    G, M = pt.temporal_gbuffer()
    assert (M == 0).all()  # the first call has no previous camera
    fh, o, d = oracle_first_hits(arrays, W, H, camera)
    t, idx, _, _ = pt.scene.intersect(T.rays6(o, d))
    t, idx = t.reshape(H, W), idx.reshape(H, W)
    slot = np.ascontiguousarray(G[..., 1]).view(np.int32)
    st = pt.scene.slot_triangles()
    tri = np.where(slot >= 0, st[np.maximum(slot, 0)].astype(np.int64), -1)
    assert np.array_equal(G[..., 7], (slot >= 0).astype(np.float32))
    miss_row = np.array([np.float32(T.MAX_T).view(np.uint32), 0xFFFFFFFF, 0, 0, 0, 0, 0, 0], np.uint32)
    assert (np.ascontiguousarray(G).view(np.uint32)[slot < 0] == miss_row).all()
    # exempt: pixels where the float64 restatement's own triangle differs from the oracle's on the float32 rays - decided
    # without the GPU, capped at 1 % (tests/test_temporal_cpu.py checks the cap for these cameras on the CPU as well)
    exempt, t64, idx64, bv64, bw64 = T.gbuffer_exempt(arrays, W, H, camera["P"], camera["I"], camera["fov_scale"], fh["index"])
    print("gbuffer exempt", int(exempt.sum()), "of", W * H)
    assert exempt.sum() <= 0.01 * W * H
    ok = ~exempt
    # everywhere else the GPU's triangle is the restatement's (= the oracle's), hits and misses alike ...
    assert np.array_equal(tri[ok], idx64[ok])
    # ... slot and t are fspt_intersect's on the same rays ...
    assert np.array_equal(tri[ok], idx[ok]) and np.array_equal(G[..., 0][ok], t[ok])
    # ... and t, the barycentric weights and the normal are the oracle's, which computes them from the same ray with the
    # arithmetic the kernels share with it: a bound of 0 (see the module docstring)
    okh = ok & (idx64 >= 0)
    assert 0 < okh.sum() < W * H
    assert np.array_equal(G[..., 0][okh], fh["t"][okh])
    assert np.array_equal(G[..., 2:4][okh], fh["bary"][..., 1:3][okh])
    assert np.array_equal(G[..., 4:7][okh], fh["macro_normal"][okh])
    print("gbuffer worst |t - t64| / t64", float((np.abs(G[..., 0][okh] - t64[okh]) / t64[okh]).max()),
          "worst |bary - bary64|", float(np.abs(G[..., 2][okh] - bv64[okh]).max()))
    pt.close()


# ---- 2. the motion buffer -------------------------------------------------------------------------------------------
def check_motion(G, M, d, cam, prev, W, H, snapshot=None, label=""):
    m = T.motion(G, d, cam, prev, snapshot)
    kind = M[..., 3]
    # a = 0 decides `behind`: exempt where |a| is within its float32 error of 0
    near0 = np.abs(m["a"]) < 64 * EPS * np.maximum(m["scale"] * np.abs(m["a"]), 1.0)
    ok_kind = (kind == m["kind"]) | near0
    assert ok_kind.all(), (label, int((~ok_kind).sum()))
    assert near0.sum() <= 0.01 * W * H
    live = (kind != 0) & (m["kind"] != 0)
    worst = 0.0
    for c, raw, snapped, res in ((0, m["sx_raw"], m["sx"], W), (1, m["sy_raw"], m["sy"], H)):
        tol = MOTION_OPS * EPS * m["scale"] * res / 2 + 8 * EPS * (np.abs(raw) + res)
        err_s = np.abs(M[..., c] - snapped)
        err_r = np.abs(M[..., c] - raw)
        r = np.floor(raw + 0.5)
        at_threshold = np.abs(np.abs(raw - r) - T.SNAP) <= tol
        err = np.where(at_threshold, np.minimum(err_s, err_r), err_s)
        # far outside the image the bound scales with |raw| alone; such positions have no tap
        far = np.abs(raw) > 1e6
        worst = max(worst, float((err / tol)[live & ~far].max(initial=0.0)))
        assert (err <= tol)[live & ~far].all(), (label, c, float((err / tol)[live & ~far].max()))
    hitp = live & (kind == 1)
    dtol = 12 * EPS * (m["scale"] * np.abs(m["a"]) * np.linalg.norm(np.asarray(prev[1], np.float64)) * float(prev[2]))
    assert (np.abs(M[..., 2] - m["dist"]) <= dtol + 4 * EPS * m["dist"])[hitp].all(), label
    assert (M[..., 2][live & (kind == 2)] == 0).all()
    print("motion", label, "worst err / bound", round(worst, 3), "behind", int((kind == 0).sum()), "miss", int((kind == 2).sum()))
    return m


@pytest.mark.parametrize("kind", ["translate", "rotate", "fov", "behind"])
def test_motion_static_scene(small_scene, camera, kind):
    W, H = 96, 64
    pt = make_pt(small_scene, W, H, camera)
    cam0, cam1 = camera, moved_camera(camera, kind)
    if kind == "behind":  # the PREVIOUS camera is the one that has the geometry behind it
        cam0, cam1 = cam1, cam0
    frame(pt, cam0)
    frame(pt, cam1)
    G, M = pt.temporal_gbuffer()
    _, d = T.centre_rays(W, H, cam1["P"], cam1["I"], cam1["fov_scale"])
    m = check_motion(G, M, d, (cam1["P"], cam1["I"], cam1["fov_scale"]), (cam0["P"], cam0["I"], cam0["fov_scale"]), W, H, label=kind)
    assert (M[..., 3] == 2).sum() > 0 or kind == "behind"  # misses are covered
    if kind == "behind":
        assert (M[..., 3] == 0).sum() > 0.2 * W * H
    else:
        assert (m["kind"] == 1).sum() > 0.2 * W * H
    pt.close()


def test_motion_moving_geometry_refit_then_rebuild(small_scene, camera):
    """a refitted scene with a motion origin, and the same scene after a rebuild: X' comes from the snapshot's triangle of
    the slot the ray hit, whatever the rebuild did to the slots"""
    W, H = 96, 64
    a = small_scene
    pt = make_pt(a, W, H, camera)
    frame(pt, camera)
    cam = (camera["P"], camera["I"], camera["fov_scale"])
    _, d = T.centre_rays(W, H, *cam)
    tri1, norm1 = rotated(a.tri, a.norm)
    pt.scene.motion_begin()
    snap0 = T.snapshot_from_triangles(a.tri, pt.scene.slot_triangles())
    pt.update_geometry(tri1, norm1)
    frame(pt, camera)
    G, M = pt.temporal_gbuffer()
    m = check_motion(G, M, d, cam, cam, W, H, snap0, "refit")
    moved = (np.abs(m["sx_raw"] - np.arange(W)[None, :]) > 0.5) & (m["kind"] == 1)
    assert moved.sum() > 0.1 * W * H  # the rotation does move the picture
    # without the snapshot the restatement lands elsewhere: the origin is what the GPU used
    m_static = T.motion(G, d, cam, cam, None)
    assert np.abs(m_static["sx"] - M[..., 0])[m["kind"] == 1].max() > 0.5
    # second move, from a NEW origin, then a rebuild in between: slots change, the snapshot follows
    pt.scene.motion_begin()
    tri2, norm2 = rotated(tri1, norm1)
    order = pt.rebuild_geometry(tri2, norm2)
    assert not np.array_equal(order, np.arange(a.n_tris))
    snap1 = T.snapshot_from_triangles(tri1.reshape(-1, 9)[order.astype(np.int64)], pt.scene.slot_triangles())
    frame(pt, camera)
    G, M = pt.temporal_gbuffer()
    check_motion(G, M, d, cam, cam, W, H, snap1, "rebuild")
    pt.scene.motion_end()
    frame(pt, camera)
    G, M = pt.temporal_gbuffer()
    check_motion(G, M, d, cam, cam, W, H, None, "motion_end")
    pt.close()


# ---- 3. the blend pass on synthetic inputs --------------------------------------------------------------------------
def blend_inputs(W, H, seed):
    """Inputs that reach every branch: sample positions anywhere from 3 pixels outside to 3 inside the far border (taps
    outside, 1-4 taps inside), integer positions (snapped: one tap), hit and miss pixels against hit and miss history,
    previous depths within / at / beyond the tolerance, previous normals turned by 0-60 degrees, history lengths
    around max_history, kinds 0 / 1 / 2."""
    rng = np.random.default_rng(seed)
    G = np.zeros((H, W, 8), np.float32); gp = np.zeros((H, W, 8), np.float32)

    def gbuf(g):
        hit = rng.random((H, W)) < 0.8
        n = rng.normal(size=(H, W, 3)); n[..., 2] += 3.0
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        g[..., 0] = np.where(hit, rng.uniform(1.0, 3.0, (H, W)), T.MAX_T)
        g[..., 1] = np.where(hit, rng.integers(0, 100, (H, W)), -1).astype(np.int32).view(np.float32)
        g[..., 2:4] = rng.uniform(0, 0.5, (H, W, 2)) * hit[..., None]
        g[..., 4:7] = n * hit[..., None]
        g[..., 7] = hit
        return hit
    hit = gbuf(G); gbuf(gp)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    sx = xs + rng.uniform(-3, 3, (H, W)); sy = ys + rng.uniform(-3, 3, (H, W))
    whole = rng.random((H, W)) < 0.2
    sx = np.where(whole, np.round(sx), sx); sy = np.where(whole, np.round(sy), sy)
    M = np.zeros((H, W, 4), np.float32)
    M[..., 0], M[..., 1] = sx, sy
    # M.z near the previous depth at the nearest tap, so that the depth test passes, sits at its edge or fails
    qx, qy = np.clip(np.round(sx), 0, W - 1).astype(int), np.clip(np.round(sy), 0, H - 1).astype(int)
    M[..., 2] = np.where(hit, gp[qy, qx, 0] * rng.choice([1.0, 1.02, 1.049, 1.2], (H, W)), 0.0)
    M[..., 2] = np.where(M[..., 2] > 1e4, 2.0, M[..., 2])
    M[..., 3] = np.where(rng.random((H, W)) < 0.05, 0.0, np.where(hit, 1.0, 2.0))
    hist = rng.uniform(0, 4, (H, W, 4)).astype(np.float32)
    hist[..., 3] = rng.choice([1.0, 7.5, 60.0, 64.0, 200.0], (H, W))
    I = rng.uniform(0, 4, (H, W, 4)).astype(np.float32); I[..., 3] = 1
    return I, M, G, hist, gp


def check_blend(I, M, G, hist, gp, n, **kw):
    got = temporal_eval(I, M, G, hist, gp, n=n, **kw)
    ref, margin = T.blend(I, M, G, hist, gp, n, **{**T.DEFAULTS, **kw})
    exempt = margin < 1e-5
    assert exempt.mean() <= 0.01, exempt.mean()
    ok = ~exempt
    none = (ref[..., 3] == min(n, kw.get("max_history", 64.0))) & (ref[..., :3] == I[..., :3]).all(-1)
    # `out = I, bit for bit` where nothing counts
    assert np.array_equal(got[..., :3][ok & none], I[..., :3][ok & none])
    scale = np.maximum(np.abs(ref[..., :3]).max(-1), np.maximum(np.abs(I[..., :3]).max(-1), 4.0))[..., None]
    err = np.abs(got[..., :3] - ref[..., :3]) / scale
    assert (err[ok] <= BLEND_RTOL).all(), float(err[ok].max())
    assert (np.abs(got[..., 3] - ref[..., 3])[ok] <= BLEND_RTOL * np.maximum(ref[..., 3][ok], 1.0)).all()
    return got, ref, none


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (17, 5), (67, 45), (1920, 1080)])
def test_blend_matches_reference(W, H):
    I, M, G, hist, gp = blend_inputs(W, H, 7 + W)
    got, ref, none = check_blend(I, M, G, hist, gp, 4)
    if W * H > 1000:
        # every branch was reached
        assert 0.05 < none.mean() < 0.95
        assert ((ref[..., 3] == 64.0) & ~none).any() and ((ref[..., 3] < 64.0) & ~none).any()
        assert (M[..., 3] == 2).any() and (M[..., 3] == 0).any()
    for kw in (dict(alpha=0.2), dict(alpha=1.0), dict(max_history=8.0), dict(depth_tol=1e-3, normal_cos=-1.0),
               dict(depth_tol=0.3, normal_cos=1.0)):
        if W * H < 100000:
            check_blend(I, M, G, hist, gp, 3, **kw)
    out = temporal_eval(I, M, G, None, None, n=5)
    assert np.array_equal(out[..., :3], I[..., :3]) and (out[..., 3] == 5).all()


def test_blend_tap_counts():
    """all taps invalid, one to three valid, borders: a 3 x 3 image probed corner by corner"""
    W = H = 3
    G = np.zeros((H, W, 8), np.float32); G[..., 0] = 2; G[..., 6] = 1; G[..., 7] = 1
    hist = np.zeros((H, W, 4), np.float32); hist[..., 3] = 1
    hist[..., 0] = np.arange(9, dtype=np.float32).reshape(3, 3)
    I = np.zeros((H, W, 4), np.float32)
    for sx, sy, want_taps in ((0.5, 0.5, 4), (-0.5, 0.5, 2), (-0.5, -0.5, 1), (2.5, 2.5, 1), (2.5, 1.0, 1), (1.0, 1.0, 1), (-1.5, 0, 0), (3.0, 1.0, 0)):
        M = np.zeros((H, W, 4), np.float32); M[..., 0] = sx; M[..., 1] = sy; M[..., 2] = 2; M[..., 3] = 1
        got = temporal_eval(I, M, G, hist, G, n=1)
        ref, _ = T.blend(I, M, G, hist, G, 1)
        assert np.allclose(got, ref, rtol=BLEND_RTOL, atol=1e-6), (sx, sy)
        assert (got[..., 3] == (2 if want_taps else 1)).all(), (sx, sy)
    # depth_tol = 0 keeps a tap of exactly the reprojected depth
    M = np.zeros((H, W, 4), np.float32); M[..., 0] = 0.5; M[..., 1] = 0.5; M[..., 2] = 2; M[..., 3] = 1
    assert (temporal_eval(I, M, G, hist, G, n=1, depth_tol=0.0)[..., 3] == 2).all()
    # three of four: knock one tap out by depth
    gp = G.copy(); gp[1, 1, 0] = 3
    M = np.zeros((H, W, 4), np.float32); M[..., 0] = 0.5; M[..., 1] = 0.5; M[..., 2] = 2; M[..., 3] = 1
    got = temporal_eval(I, M, G, hist, gp, n=1)
    assert np.allclose(got[..., 0], (0 + 1 + 3) / 3 / 2, rtol=1e-6)


# ---- 4. exact properties on rendered frames -------------------------------------------------------------------------
def test_static_frames_are_the_sequential_mean(small_scene, camera):
    W, H, n, K = 96, 64, 3, 5
    pt = make_pt(small_scene, W, H, camera)
    twin = make_pt(small_scene, W, H, camera)
    hist = None
    for k in range(K):
        pt.clear(); pt.seed(11 + k); pt.render(n)
        I = pt.readRadiance()
        out = pt.temporal_accumulate(max_history=12.0)
        assert pt.readRadiance().tobytes() == I.tobytes()  # the accumulator is only read
        G, M = pt.temporal_gbuffer()
        hit = G[..., 7] != 0
        if hist is None:
            want = I.copy(); want[..., 3] = n
            assert np.array_equal(out, want)
        else:
            xs, ys = np.meshgrid(np.arange(W), np.arange(H))
            assert np.array_equal(M[..., 0], xs) and np.array_equal(M[..., 1], ys)  # snapped: one tap of weight 1
            want = T.running_mean_f32(hist, I, n, max_history=12.0)
            assert np.array_equal(out, want)
            assert (out[..., 3] == min((k + 1) * n, 12)).all()  # no self-rejection: hits and misses alike
        hist = out
    assert 0 < hit.sum() < W * H
    # a later render equals one on a target that never accumulated
    for p in (pt, twin):
        p.clear(); p.seed(77); p.render(4)
    assert pt.readRadiance().tobytes() == twin.readRadiance().tobytes()
    pt.close(); twin.close()


def test_disoccluded_pixels_hold_the_frame(small_scene, camera):
    W, H, n = 96, 64, 2
    pt = make_pt(small_scene, W, H, camera)
    frame(pt, camera, n)
    G0, _ = pt.temporal_gbuffer()
    h0 = pt.temporal_accumulate()  # (a second call with the same frame: the history the next one reads)
    G0, _ = pt.temporal_gbuffer()
    cam1 = moved_camera(camera, "translate")
    out = frame(pt, cam1, n, seed=9)
    I = pt.readRadiance()
    G, M = pt.temporal_gbuffer()
    ref, margin = T.blend(I, M, G, h0, G0, n)
    dis = (ref[..., 3] == n) & (margin > 1e-5)
    print("disoccluded", int(dis.sum()), "reprojected", int((ref[..., 3] > n).sum()))
    assert dis.sum() > 20 and (ref[..., 3] > n).sum() > 0.5 * W * H
    assert np.array_equal(out[..., :3][dis], I[..., :3][dis]) and (out[..., 3][dis] == n).all()
    ok = margin > 1e-5
    assert np.allclose(out[ok], ref[ok], rtol=1e-5, atol=1e-6)
    pt.close()


# ---- 5. quality -----------------------------------------------------------------------------------------------------
def test_quality(medium_scene, camera):
    """tools/temporal_quality.py's two sequences at its own size (320 x 240, 8 frames of 4 spp, a 2-degree orbit step; the
    geometry sequence with refit_moves' rotation in 8 steps).  Relative MSE of the last frame against 4 096 spp.
    Measured on the MI355X with the shipped defaults: temporal / raw = 0.2025 (raw 0.585), temporal + a-trous /
    raw = 0.0023, moving geometry with the motion origin / raw = 0.0350 (without it 0.117); thresholds = measured x 1.5.  In every case a temporal frame must beat the raw
    frame, and the moving-geometry run without a motion origin must be worse than the run with it."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import temporal_quality as Q
    cam = Q.camera_sequence(medium_scene, camera)
    cam.pop("gt")
    print("quality camera", cam)
    assert cam["temporal"] < cam["raw"] and cam["temporal_atrous"] < cam["raw"]
    assert cam["temporal"] <= Q.MEASURED["camera_temporal_over_raw"] * 1.5 * cam["raw"], cam
    assert cam["temporal_atrous"] <= Q.MEASURED["camera_temporal_atrous_over_raw"] * 1.5 * cam["raw"], cam
    geo = Q.geometry_sequence(medium_scene, camera)
    print("quality geometry", geo)
    assert geo["with_origin"] < geo["raw"]
    assert geo["with_origin"] <= Q.MEASURED["geometry_with_origin_over_raw"] * 1.5 * geo["raw"], geo
    assert geo["without_origin"] > geo["with_origin"], geo


# ---- 6. plumbing ----------------------------------------------------------------------------------------------------
def test_denoise_draw_reset_and_errors(small_scene, camera):
    W, H = 64, 48
    pt = make_pt(small_scene, W, H, camera)
    lib = L.lib()
    cp = pt._camera_params()
    assert lib.fspt_temporal_accumulate(pt._t, ctypes.byref(cp), None, None) == -6  # no tick yet
    assert b"no sample" in lib.fspt_last_error()
    with pytest.raises(L.FsptError) as e:
        pt.temporal_draw()
    assert e.value.code == -6
    pt.render(2)
    for bad in (dict(alpha=2.0), dict(max_history=0.0), dict(depth_tol=-1.0), dict(normal_cos=2.0)):
        prm = L.TemporalParams(**{**T.DEFAULTS, **bad})
        assert lib.fspt_temporal_accumulate(pt._t, ctypes.byref(cp), ctypes.byref(prm), None) == -1
    assert lib.fspt_temporal_accumulate(pt._t, None, None, None) == -1
    pt.set_viewport(32, 24)
    assert lib.fspt_temporal_accumulate(pt._t, ctypes.byref(cp), None, None) == -6
    pt.set_viewport(0, 0)
    pt.set_shard(0, 2)
    assert lib.fspt_temporal_accumulate(pt._t, ctypes.byref(cp), None, None) == -6
    pt.set_shard(0, 1)
    h1 = pt.temporal_accumulate()
    h2 = pt.temporal_accumulate()
    assert (h1[..., 3] == 2).all() and (h2[..., 3] == 4).all()
    with pytest.raises(L.FsptError) as e:
        pt.temporal_denoise()  # no features yet
    assert e.value.code == -6
    pt.features(4, 3)
    den = pt.temporal_denoise(iterations=3)
    assert np.array_equal(den, denoise_eval(h2, pt.readFeatures(), iterations=3))
    rgba = pt.temporal_draw(1.2, 0.9, denoised=True)
    assert np.array_equal(rgba, pt.drawDenoised(1.2, 0.9))
    # the denoised frame temporal_draw shows is temporal_denoise's of the current history: a plain denoise() (same buffer) or
    # a new accumulate invalidates it
    pt.denoise(iterations=1)
    with pytest.raises(L.FsptError) as e:
        pt.temporal_draw(1.2, 0.9, denoised=True)
    assert e.value.code == -6
    assert np.array_equal(pt.temporal_denoise(iterations=3), den) and np.array_equal(pt.temporal_draw(1.2, 0.9, denoised=True), rgba)
    # temporal_draw of the history = draw of an accumulator holding it
    twin = make_pt(small_scene, W, H, camera)
    import torch
    buf = torch.from_numpy(h2.copy()).cuda()
    twin.bind_accumulator(buf.data_ptr(), keep=buf)
    assert np.array_equal(pt.temporal_draw(1.2, 0.9), twin.draw(1.2, 0.9))
    twin.close()
    pt.temporal_reset()
    h3 = pt.temporal_accumulate()
    assert np.array_equal(h3, h1)
    ms = pt.temporal_last_ms()
    assert ms[0] > 0 and ms[1] > 0
    pt.close()


def test_pipelines_recorded_ticks_and_present(small_scene, camera):
    """every pipeline setting leaves results equal; recorded two-call ticks and a target under fspt_present are flushed"""
    W, H = 64, 48
    outs = []
    for mode in ("wavefront", "stream", "mega", "ticks", "present"):
        pt = make_pt(small_scene, W, H, camera)
        pt.seed(3)
        if mode == "stream":
            pt.set_pipeline(2)
        elif mode == "mega":
            pt.set_pipeline(0)
        if mode in ("ticks", "present"):
            for _ in range(3):
                pt.tick()
                if mode == "present":
                    pt.present()
        else:
            pt.render(3)
        a = pt.temporal_accumulate()
        pt.clear(); pt.seed(4)
        if mode in ("ticks", "present"):
            for _ in range(2):
                pt.tick()
        else:
            pt.render(2)
        b = pt.temporal_accumulate()
        outs.append((a, b))
        pt.close()
    for a, b in outs[1:]:
        assert np.array_equal(a, outs[0][0]) and np.array_equal(b, outs[0][1])
    assert (outs[0][1][..., 3] == 5).all()


def test_no_memory_growth(small_scene, camera):
    from fspt_amd import device_memory
    pt = make_pt(small_scene, 128, 96, camera)
    pt.render(1)
    pt.temporal_accumulate()
    pt.sync()
    free0 = device_memory(0)[0]
    for _ in range(20):
        pt.temporal_accumulate(read=False)
    pt.sync()
    assert device_memory(0)[0] >= free0 - (1 << 20)
    pt.close()


def _write_frames(tmp_path, n_frames):
    """scene files of a panel (explicit uvs: only its vertices change from frame to frame, so the frames refit) that swings
    over a cube-sphere and a floor, one JSON per frame"""
    import json
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    (root / "mesh" / "ball.obj").write_text("mtllib ball.mtl\nusemtl glow\n" + S.cube_sphere_obj(4))  # (the scene's only light)
    (root / "mesh" / "ball.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    for f in range(n_frames):
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 3, "exposure": 1.2,
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6],
                                   "emittance": [0, 0, 0]},
                                  {"path": "mesh/ball.obj", "scale": 0.4, "translate": [-0.2, 0.0, 0.0], "diffuse": [0.8, 0.3, 0.2],
                                   "emittance": [3, 3, 3], "normals": "smooth"}],
                 "animated_props": [{"path": "mesh/quad.obj", "scale": 0.8, "translate": [0.4 - 0.15 * f, 0.3 + 0.05 * f, -0.3 + 0.1 * f],
                                     "rotate": [{"axis": [1, 0, 0], "angle": 0.5 + 0.1 * f}], "diffuse": [0.2, 0.5, 0.8],
                                     "emittance": [0, 0, 0]}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def _frames_by_hand(pattern, root, W, H, n_frames, params, atrous, seed=1, origin=True):
    """issue section 4's protocol on a tracer driven by hand: motion_begin, update_geometry, clear, render with seed + k,
    temporal_accumulate, (features, temporal_denoise,) temporal_draw -> the RGB frames, top row first"""
    from fspt_amd import scene_file as F
    base, settings = F.load_scene_file(pattern.format(frame=0), root, bvh="sah", keep_order=True)
    pt = PathTracer(base, W, H, num_bounces=4)
    frames = []
    for k in range(n_frames):
        if k:
            g, settings = F.load_scene_file(pattern.format(frame=k), root, geometry_only=True)
            tri, norm = S.geometry_in_leaf_order(base.meta["tri_order"], g.tri, g.norm)
            if origin:
                pt.scene.motion_begin()
            pt.update_geometry(tri, norm)
        pt.clear()
        pt.eye, pt.dir = list(settings["eye"]), list(settings["dir"])
        pt.fovScale, pt.envTheta = settings["fov_scale"], settings["env_theta"]
        pt.lensFeatures = [settings["focus"], settings["aperture"]]
        pt.seed(seed + k)
        pt.render(int(settings["samples"]))
        pt.temporal_accumulate(read=False, **params)
        if atrous:
            pt.features(8, seed)
            pt.temporal_denoise(iterations=atrous)
        frames.append(pt.temporal_draw(settings["exposure"], 1.0, denoised=atrous > 0)[::-1, :, :3].copy())
    pt.close(); pt.scene.close()
    return frames


@pytest.mark.parametrize("atrous", [0, 2])
def test_render_sequence_temporal(tmp_path, atrous):
    """render_sequence(bvh="refit", temporal=...) follows the frame protocol: the frames it writes are temporal_draw of a
    tracer driven by hand the same way, pixel for pixel - with and without the a-trous filter on the temporal result"""
    from PIL import Image
    from fspt_amd import scene_file as F
    W, H = 48, 32
    pattern, root = _write_frames(tmp_path, 3)
    log = []
    params = {"max_history": 6.0, "depth_tol": 0.1}
    out = F.render_sequence(pattern, range(3), str(tmp_path / "t" / "{frame}.png"), W, H, root, bvh="refit",
                            temporal={**params, "atrous": atrous}, on_frame=lambda f, how: log.append(how))
    assert log == ["build", "refit", "refit"] and len(out) == 3
    want = _frames_by_hand(pattern, root, W, H, 3, params, atrous)
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(out[k]))[:, :, :3], want[k]), k
    assert want[2].max() > 0 and (want[2] > 0).mean() > 0.1  # (a lit picture)
    # the protocol matters: without the motion origin, or without the history, the last frame is another picture
    assert not np.array_equal(want[2], _frames_by_hand(pattern, root, W, H, 3, params, atrous, origin=False)[2])
    assert not np.array_equal(want[2], _frames_by_hand(pattern, root, W, H, 3, {**params, "alpha": 1.0}, atrous)[2])
    with pytest.raises(ValueError, match="adaptive"):
        F.render_sequence(pattern, range(2), str(tmp_path / "a" / "{frame}.png"), W, H, root, bvh="refit", temporal=True, adaptive=0.01)


def test_render_cli_temporal(tmp_path):
    """python -m fspt_amd.render --frames A:B --bvh refit --temporal --atrous K writes render_sequence's frames"""
    import os, subprocess, sys
    from PIL import Image
    W, H = 48, 32
    pattern, root = _write_frames(tmp_path, 3)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outp = str(tmp_path / "cli" / "{frame}.png")
    subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--scene", pattern, "--assets", root, "--frames", "0:3", "--bvh", "refit",
                           "--temporal", "--atrous", "2", "--bounces", "4", "--width", str(W), "--height", str(H), "--out", outp], cwd=repo, timeout=600)
    want = _frames_by_hand(pattern, root, W, H, 3, {}, 2)
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(outp.format(frame=k)))[:, :, :3], want[k]), k
    assert (want[2] > 0).mean() > 0.1


def test_node_host_matches_python(tmp_path):
    import json, os, shutil, subprocess
    import lights_ref as LR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("node") is None or not os.path.exists(os.path.join(root, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    e1 = LR.scene_e1()  # (no environment map: the job files stay small)
    W, H, n = 64, 48, 3
    cam = dict(S.BUNNY_CAMERA)
    cam2 = dict(cam); cam2["P"] = [cam["P"][0] + 0.1, cam["P"][1], cam["P"][2] + 0.05]
    tri2, norm2 = rotated(e1.tri, e1.norm, deg=3.0)
    pt = make_pt(e1, W, H, cam)
    pt.seed(3); pt.render(n)
    h1 = pt.temporal_accumulate()
    pt.scene.motion_begin()
    pt.update_geometry(tri2, norm2)
    pt.set_camera(cam2["P"], cam2["I"], cam2["fov_scale"], cam2["env_theta"], cam2["focal_depth"], cam2["aperture"])
    pt.clear(); pt.seed(7); pt.render(n)
    h2 = pt.temporal_accumulate(max_history=5.0, depth_tol=0.1)
    pt.features(4, 3)
    den = pt.temporal_denoise(iterations=2)
    draw_den, draw = pt.temporal_draw(1.2, 0.9, True), pt.temporal_draw(1.2, 0.9, False)
    pt.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    tri2.tofile(os.path.join(d, "tri2.bin")); norm2.tofile(os.path.join(d, "norm2.bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=n, cam=cam, cam2=cam2,
                lens=S.lens_features(cam["focal_depth"], cam["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(root, "tests", "temporal_node_check.js"), os.path.join(root, "fspt_amd", "js"), d], timeout=300)
    rd = lambda name, dt, c: np.fromfile(os.path.join(d, name + ".bin"), dt).reshape(H, W, c)
    assert (h2[..., 3] > n).sum() > 0.3 * W * H  # history was reprojected through the move
    assert np.array_equal(rd("h1", np.float32, 4), h1) and np.array_equal(rd("h2", np.float32, 4), h2)
    assert np.array_equal(rd("den", np.float32, 4), den)
    assert np.array_equal(rd("draw_den", np.uint8, 4), draw_den) and np.array_equal(rd("draw", np.uint8, 4), draw)
