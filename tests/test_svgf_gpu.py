"""SVGF variance guidance on the GPU: k_temporal_blend<true>, k_svgf_variance and k_atrous<true> against the
float64 restatement of tests/svgf_ref.py.

Bounds, u = 2^-24 (one correctly rounded float32 operation):
  * variance.  v is a DIFFERENCE: max(0, M2 - M1 M1) / Fe.  The product, the subtraction, Fe = length / n and the division
    are one rounding each of terms no larger than scale = max(M2, M1 M1) / Fe (svgf_ref.variance returns it): |dv| <= 4 u
    scale.  The spatial branch sums 49 non-negative terms by fma (49 u relative for S1 and for S2) with weights wn wz whose
    float32 values are off by a factor within e^(20 u sn) (test_denoise_gpu.sigma_normal_rtol's cosine bound) times
    e^(3 u 88) (the depth exponent, three roundings, below 88 wherever the weight is not 0): dw = 20 u sn + 264 u; S1 S1
    doubles its error: |dv| <= (3 (49 u + 2 dw) + 4 u) scale.  No relative bound on v itself exists where M2 ~ M1 M1.
  * filter.  Compared against the restatement run on the GPU's OWN v (the variance stage is held to its bound above, and
    wl is arbitrarily sensitive to v near 0, so feeding the float64 v would test the variance twice and the filter not at
    all).  With wl off (sl = +inf) the filter is k_atrous's arithmetic plus one fma and one division for the variance:
    test_denoise_gpu.check_bound as it stands, for the colour and for the variance.  With wl on the exponent
    |Lp - Lq| / lden_p multiplies a relative error of the luminances by L / lden, which no global figure bounds usefully
    (1e4 at a pixel whose neighbourhood has variance 0).  So the bound is PER PIXEL: svgf_ref.guided_atrous_bounded
    propagates, through every tap of every iteration, an absolute error of u and of var from the reference's own float64
    states (its docstring is the derivation).  Each pixel is held to the larger of check_bound's tolerance and its own
    bound, and the bounds are tight: check_per_pixel asserts how many lie within ten times check_bound's tolerance.  The
    set with a variance floor (svgf_ref.synthetic_history(floor=True)) keeps wl well conditioned everywhere; the set with
    exact zeros and huge values keeps the finiteness claims."""
import os

import numpy as np
import pytest

import atrous_ref as A
import svgf_ref as V
import temporal_ref as T
from test_denoise_gpu import SHAPES, WEIGHTS, check_bound, check_in_hull
from fspt_amd import PathTracer, scene as S, svgf_eval, temporal_eval

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def variance_bound(scale, hist, n, sn):
    dw = 20 * U * sn + 264 * U
    spatial = 3 * (49 * U + 2 * dw) + 4 * U
    Fe = hist[..., 3].astype(np.float64) / n
    return np.where(Fe >= 4, 4 * U, spatial) * scale


def check_per_pixel(got, ref, E, floor_rel, K):
    """|got - ref| <= max(check_bound's tolerance, E) at every value; and the bound is no formality: at least 85 % of the
    values up to four iterations, and half at five, are held within ten times check_bound's tolerance (fractions of the
    reference alone: 0.90 and 0.57 are the lowest over this file's cases)"""
    assert np.isfinite(E).all() and np.isfinite(ref).all()
    cb = np.where(np.abs(ref) > 1e-3, floor_rel * np.abs(ref), 1e-6)
    tol = np.maximum(cb, E)
    worst = float((np.abs(got - ref) / tol).max())
    tight = float((E <= 10 * cb).mean())
    print("  at check_bound's own tolerance %.3f of the values, within ten times it %.3f, worst error / bound %.3g"
          % ((E <= cb).mean(), tight, worst))
    assert worst <= 1.0, worst
    assert tight >= (0.85 if K <= 4 else 0.5), tight


def run(hist, mom, f, n, **kw):
    p = {**V.DEFAULTS, **kw}
    out, vin, vout = svgf_eval(hist, mom, f, n=n, **kw)
    ref_v, scale = V.variance(hist, mom, f, n, p["sigma_normal"], p["sigma_depth"])
    err = np.abs(vin - ref_v)
    bound = variance_bound(scale, hist, n, p["sigma_normal"]) + 1e-30
    print("variance: worst error / bound %.3g" % float((err / bound).max()))
    assert np.isfinite(vin).all() and (vin >= 0).all() and (err <= bound).all(), float((err / bound).max())
    K = p["iterations"]
    print("filter: K %d sl %g" % (K, p["sigma_color"]))
    assert np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all()
    if K == 0:
        assert np.array_equal(out, hist) and np.array_equal(vout, vin)
    elif np.isinf(p["sigma_color"]):
        ref, ref_vk = V.guided_atrous(hist, vin, f, **p)
        check_bound(out, ref)
        check_bound(vout, ref_vk, 2e-4)  # (w w: the weights' error twice)
    else:
        ref, ref_vk, E, Av = V.guided_atrous_bounded(hist, vin, f, **p)
        check_in_hull(out, hist, f)
        check_per_pixel(out[..., :3], ref[..., :3], E, 1e-4, K)
        check_per_pixel(vout, ref_vk, Av, 2e-4, K)
    return out, vin, vout


@pytest.mark.parametrize("W,H", SHAPES)
def test_svgf_eval_shapes_and_iterations(W, H):
    for floor in (False, True):
        hist, mom, f = V.synthetic_history(H, W, n=2, floor=floor)
        for k in range(6):
            run(hist, mom, f, 2, iterations=k)
            run(hist, mom, f, 2, iterations=k, sigma_color=np.inf)


@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_svgf_eval_weights_one_at_a_time(weights):
    """test_denoise_gpu's four settings; "colour only" is the variance-guided luminance weight alone"""
    for W, H in ((120, 80), (17, 16)):
        for floor in (False, True):
            hist, mom, f = V.synthetic_history(H, W, n=3, floor=floor)
            for k in (1, 2, 3, 5):
                run(hist, mom, f, 3, iterations=k, **WEIGHTS[weights])


def test_svgf_eval_variance_extremes():
    """exactly 0 (12-bit moments whose square is exact, long history) and up to 1e12 x the mean"""
    hist, mom, f = V.synthetic_history(80, 120, n=2)
    out, vin, vout = run(hist, mom, f, 2, iterations=2)
    Fe = hist[..., 3] / 2
    zero = (Fe >= 4) & (mom[..., 1] == mom[..., 0] * mom[..., 0])
    assert zero.sum() > 100 and (vin[zero] == 0).all() and (vin > 1e9).sum() > 100
    # a frame whose variance is 0 everywhere: wl is a delta on equal luminances, the output stays finite
    m0 = mom.copy(); m0[..., 1] = m0[..., 0] * m0[..., 0]
    h0 = hist.copy(); h0[..., 3] = 64
    out, vin, vout = svgf_eval(h0, m0, f, n=2, iterations=3)
    assert np.isfinite(out).all() and (vout == 0).all()
    assert (vin[mom[..., 1] == mom[..., 0] * mom[..., 0]] == 0).all()


def test_svgf_eval_full_hd():
    """1920 x 1080 at two iterations, checked on five windows grown by the filter's reach (test_denoise_gpu's scheme)"""
    H, W, k = 1080, 1920, 2
    hist, mom, f = V.synthetic_history(H, W, n=2)
    out, vin, vout = svgf_eval(hist, mom, f, n=2, iterations=k, sigma_color=np.inf)
    assert np.isfinite(out).all()
    r = 2 * (2 ** k - 1) + 3
    for y0, x0 in ((0, 0), (0, W - 64), (H - 64, 0), (H - 64, W - 64), (H // 2 - 32, W // 2 - 32)):
        y1, x1 = y0 + 64, x0 + 64
        ey0, ex0, ey1, ex1 = max(0, y0 - r), max(0, x0 - r), min(H, y1 + r), min(W, x1 + r)
        win = (slice(ey0, ey1), slice(ex0, ex1))
        inner = (slice(y0 - ey0, y1 - ey0), slice(x0 - ex0, x1 - ex0))
        ref_v, scale = V.variance(hist[win], mom[win], f[win], 2)
        assert (np.abs(vin[win] - ref_v)[inner] <= (variance_bound(scale, hist[win], 2, 32.0) + 1e-30)[inner]).all()
        ref, ref_vk = V.guided_atrous(hist[win], vin[win], f[win], iterations=k, sigma_color=np.inf)
        check_bound(out[y0:y1, x0:x1], ref[inner])
        check_bound(vout[y0:y1, x0:x1], ref_vk[inner], 2e-4)


# ---- the target path ----------------------------------------------------------------------------------------------------
def make_pt(arrays, W, H, cam):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    return pt


def frame(pt, n, seed, **params):
    pt.clear(); pt.seed(seed); pt.render(n)
    return pt.temporal_accumulate(**params)


def luma_f32(acc, f):
    """l as the kernel rounds it: three divisions, (0.2126 r + 0.7152 g) + 0.0722 b, every operation float32"""
    F = np.float32
    u = (acc[..., :3] / np.maximum(f[..., :3], F(1e-3))).astype(F)
    return ((F(0.2126) * u[..., 0] + F(0.7152) * u[..., 1]).astype(F) + F(0.0722) * u[..., 2]).astype(F)


def test_states_and_refusals(small_scene, camera):
    from fspt_amd import FsptError
    pt = make_pt(small_scene, 64, 48, camera)
    pt.render(2)
    with pytest.raises(FsptError, match="moments are off"):
        pt.temporal_denoise(variance=True)
    pt.temporal_set_moments(True)
    with pytest.raises(FsptError, match="no fspt_features call yet"):
        pt.temporal_accumulate()
    pt.features(2, 1)
    with pytest.raises(FsptError, match="no fspt_temporal_accumulate call"):
        pt.temporal_denoise(variance=True)
    pt.temporal_accumulate()
    with pytest.raises(FsptError, match="no fspt_temporal_denoise_variance call"):
        pt.temporal_variance()
    pt.temporal_variance(variance=False)
    pt.temporal_denoise(variance=True)
    pt.temporal_variance()
    with pytest.raises(ValueError):
        pt.temporal_denoise(variance=True, sigma_depth=0.0)
    pt.temporal_reset()  # drops the moments with the history
    with pytest.raises(FsptError, match="no fspt_temporal_accumulate call"):
        pt.temporal_denoise(variance=True)
    pt.temporal_accumulate()
    pt.temporal_set_moments(False); pt.temporal_set_moments(True)  # re-enabled: both histories restart together
    with pytest.raises(FsptError, match="no fspt_temporal_accumulate call"):
        pt.temporal_denoise(variance=True)
    pt.close()


def test_colour_history_identical_and_accumulator_untouched(small_scene, camera):
    W, H = 96, 64
    cam2 = dict(camera); cam2["P"] = [camera["P"][0] + 0.1, camera["P"][1], camera["P"][2] + 0.05]
    outs = []
    for on in (False, True):
        pt = make_pt(small_scene, W, H, camera)
        if on:
            pt.temporal_set_moments(True)
        hs = []
        for k, c in enumerate((camera, cam2, camera)):
            pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])
            pt.clear(); pt.seed(3 + k); pt.render(2)
            pt.features(2, 1)
            acc = pt.readRadiance()
            hs.append(pt.temporal_accumulate(max_history=8.0))
            assert np.array_equal(pt.readRadiance(), acc)
        hs.append(pt.temporal_denoise(iterations=2))  # the parent's filter, with the mode on and off
        if on:
            pt.temporal_denoise(variance=True)
            assert np.array_equal(pt.readRadiance(), acc)
        outs.append(hs)
        pt.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert (outs[0][1][..., 3] > 2).mean() > 0.3  # the history was reprojected through the move


def test_static_camera_running_mean_disocclusion_reset(small_scene, camera):
    W, H, n, K = 80, 60, 2, 6
    pt = make_pt(small_scene, W, H, camera)
    pt.temporal_set_moments(True)
    pt.features(4, 1)
    f = pt.readFeatures()
    F = np.float32
    M = None
    for k in range(K):
        h = frame(pt, n, 10 + k, max_history=8.0)
        l = luma_f32(pt.readRadiance(), f)
        m = np.stack([l, (l * l).astype(F)], -1)
        if M is None:
            M, N = m, np.full((H, W), F(min(n, 8)))
        else:  # temporal_ref.running_mean_f32's operations on the two moments
            a = (F(n) / (N + F(n)).astype(F)).astype(F)[..., None]
            M = (M + ((m - M).astype(F) * a).astype(F)).astype(F)
            N = np.minimum((N + F(n)).astype(F), F(8))
        _, got = pt.temporal_variance(variance=False)
        assert np.array_equal(got, M), k
        assert np.array_equal(h[..., 3], N)  # Fe = length / n = min(k + 1, cap / n)
    # a camera far beyond the scene: every surface pixel is disoccluded and holds (l, l l)
    far = dict(camera)
    P, I = np.array(camera["P"], np.float64), np.array(camera["I"], np.float64)
    far["P"] = list(P + 2.2 * I / np.linalg.norm(I) * np.linalg.norm(P))
    pt.set_camera(far["P"], far["I"], far["fov_scale"], far["env_theta"], far["focal_depth"], far["aperture"])
    pt.features(4, 1)
    f = pt.readFeatures()
    h = frame(pt, n, 99)
    l = luma_f32(pt.readRadiance(), f)
    dis = h[..., 3] == n  # (the sky reprojects by direction and keeps its history)
    assert dis.mean() > 0.3 and not dis.all()
    got = pt.temporal_variance(variance=False)[1]
    assert np.array_equal(got[dis], np.stack([l, (l * l).astype(F)], -1)[dis]) and not np.array_equal(got[~dis][:, 0], l[~dis])
    # reset: the next call starts the moments again
    frame(pt, n, 100)
    pt.temporal_reset()
    h = frame(pt, n, 101)
    l = luma_f32(pt.readRadiance(), f)
    assert np.array_equal(pt.temporal_variance(variance=False)[1], np.stack([l, (l * l).astype(F)], -1))
    pt.close()


def test_moments_blend_matches_reference_under_motion(small_scene, camera):
    """a moved camera: fractional taps.  Mout against svgf_ref.blend_moments on the read-back buffers, within the blend's
    16 u (test_temporal_gpu BLEND_RTOL = 2e-6) of the largest moment involved, away from taps near a validity threshold"""
    W, H, n = 96, 64, 2
    cam2 = dict(camera); cam2["P"] = [camera["P"][0] + 0.11, camera["P"][1] + 0.04, camera["P"][2] - 0.07]
    pt = make_pt(small_scene, W, H, camera)
    pt.temporal_set_moments(True)
    pt.features(2, 1)
    h1 = frame(pt, n, 5)
    g1, _ = pt.temporal_gbuffer()
    _, m1 = pt.temporal_variance(variance=False)
    pt.set_camera(cam2["P"], cam2["I"], cam2["fov_scale"], cam2["env_theta"], cam2["focal_depth"], cam2["aperture"])
    pt.features(2, 1)
    f2 = pt.readFeatures()
    h2 = frame(pt, n, 6)
    acc = pt.readRadiance()
    g2, mo2 = pt.temporal_gbuffer()
    _, m2 = pt.temporal_variance(variance=False)
    want = V.blend_moments(acc, mo2, g2, h1, m1, g1, f2, n)
    _, margin = T.blend(acc, mo2, g2, h1, g1, n)
    ok = margin > 1e-5
    assert ok.mean() > 0.9 and (h2[..., 3] > n).mean() > 0.3
    # every term is >= 0; with a zero input the blend returns Hm (1 - a), and 1 - a >= 1/2 (N >= n): Hm <= twice that
    mag = V.frame_moments(acc, f2) + 2 * V.blend_moments(np.zeros_like(acc), mo2, g2, h1, m1, g1, f2, n)
    assert (np.abs(m2 - want)[ok] <= 2e-6 * mag[ok] + 1e-30).all()
    pt.close()


def test_target_path_is_svgf_eval_and_draws(small_scene, camera):
    W, H, n = 96, 64, 3
    pt = make_pt(small_scene, W, H, camera)
    pt.temporal_set_moments(True)
    pt.features(4, 1)
    for k in range(3):
        hist = frame(pt, n, 20 + k, max_history=7.0)  # Fe = 1, 2, 7/3: the spatial branch
    f = pt.readFeatures()
    _, mom = pt.temporal_variance(variance=False)
    for kw in (dict(), dict(iterations=2, sigma_color=2.0), dict(iterations=0), dict(iterations=1, sigma_normal=0.0)):
        got = pt.temporal_denoise(variance=True, **kw)
        v, _ = pt.temporal_variance()
        out, vin, _ = svgf_eval(hist, mom, f, n=n, **kw)
        assert np.array_equal(got, out) and np.array_equal(v, vin), kw
    pt.temporal_denoise(variance=True, iterations=0)  # K = 0 copies the history: drawing it is drawing the history
    assert np.array_equal(pt.temporal_draw(1.2, 0.9, True), pt.temporal_draw(1.2, 0.9, False))
    pt.temporal_denoise(variance=True)
    assert not np.array_equal(pt.temporal_draw(1.2, 0.9, True), pt.temporal_draw(1.2, 0.9, False))
    ms = pt.svgf_last_ms()
    assert ms[0] > 0 and ms[1] > 0
    for _ in range(4):
        hist = frame(pt, n, 40, max_history=64.0)
    assert (hist[..., 3] / n >= 4).all()  # the temporal branch
    got = pt.temporal_denoise(variance=True)
    out, vin, _ = svgf_eval(hist, pt.temporal_variance(variance=False)[1], f, n=n)
    assert np.array_equal(got, out) and np.array_equal(pt.temporal_variance()[0], vin)
    pt.close()


def test_no_memory_growth(small_scene, camera):
    from fspt_amd import device_memory
    pt = make_pt(small_scene, 128, 96, camera)
    pt.temporal_set_moments(True)
    pt.render(1); pt.features(1, 1)
    pt.temporal_accumulate(); pt.temporal_denoise(variance=True)
    pt.sync()
    free0 = device_memory(0)[0]
    for _ in range(20):
        pt.temporal_accumulate(read=False)
        pt.temporal_denoise(variance=True)
    pt.sync()
    assert device_memory(0)[0] >= free0 - (1 << 20)
    pt.close()


# ---- hosts ----------------------------------------------------------------------------------------------------------------
def _frames_by_hand(pattern, root, W, H, n_frames, atrous, seed=1, variance=True):
    from fspt_amd import scene_file as F
    base, settings = F.load_scene_file(pattern.format(frame=0), root, bvh="sah", keep_order=True)
    pt = PathTracer(base, W, H, num_bounces=4)
    if variance:
        pt.temporal_set_moments(True)
    frames = []
    for k in range(n_frames):
        if k:
            g, settings = F.load_scene_file(pattern.format(frame=k), root, geometry_only=True)
            tri, norm = S.geometry_in_leaf_order(base.meta["tri_order"], g.tri, g.norm)
            pt.scene.motion_begin()
            pt.update_geometry(tri, norm)
        pt.clear()
        pt.eye, pt.dir = list(settings["eye"]), list(settings["dir"])
        pt.fovScale, pt.envTheta = settings["fov_scale"], settings["env_theta"]
        pt.lensFeatures = [settings["focus"], settings["aperture"]]
        pt.seed(seed + k)
        pt.render(int(settings["samples"]))
        pt.features(8, seed)
        pt.temporal_accumulate(read=False)
        pt.temporal_denoise(iterations=atrous, variance=variance)
        frames.append(pt.temporal_draw(settings["exposure"], 1.0, denoised=True)[::-1, :, :3].copy())
    pt.close(); pt.scene.close()
    return frames


def test_render_sequence_and_cli_variance(tmp_path):
    import subprocess, sys
    from PIL import Image
    from fspt_amd import scene_file as F
    from test_temporal_gpu import _write_frames
    W, H = 48, 32
    pattern, root = _write_frames(tmp_path, 3)
    out = F.render_sequence(pattern, range(3), str(tmp_path / "v" / "{frame}.png"), W, H, root, bvh="refit", temporal={"atrous": 2}, variance=True)
    want = _frames_by_hand(pattern, root, W, H, 3, 2)
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(out[k]))[:, :, :3], want[k]), k
    assert (want[2] > 0).mean() > 0.1
    assert not np.array_equal(want[2], _frames_by_hand(pattern, root, W, H, 3, 2, variance=False)[2])  # another filter
    outp = str(tmp_path / "cli" / "{frame}.png")
    subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--scene", pattern, "--assets", root, "--frames", "0:3", "--bvh", "refit",
                           "--temporal", "--atrous", "2", "--variance-guided", "--bounces", "4", "--width", str(W), "--height", str(H),
                           "--out", outp], cwd=ROOT, timeout=600)
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(outp.format(frame=k)))[:, :, :3], want[k]), k


def test_node_host_matches_python(tmp_path):
    import json, shutil, subprocess
    import lights_ref as LR
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    e1 = LR.scene_e1()
    W, H, n = 64, 48, 3
    cam = dict(S.BUNNY_CAMERA)
    cam2 = dict(cam); cam2["P"] = [cam["P"][0] + 0.1, cam["P"][1], cam["P"][2] + 0.05]
    pt = make_pt(e1, W, H, cam)
    pt.temporal_set_moments(True)
    pt.seed(3); pt.render(n); pt.features(4, 3)
    h1 = pt.temporal_accumulate()
    pt.set_camera(cam2["P"], cam2["I"], cam2["fov_scale"], cam2["env_theta"], cam2["focal_depth"], cam2["aperture"])
    pt.clear(); pt.seed(7); pt.render(n); pt.features(4, 3)
    h2 = pt.temporal_accumulate()
    den = pt.temporal_denoise(iterations=2, sigma_color=3.0, variance=True)
    draw_den = pt.temporal_draw(1.2, 0.9, True)
    pt.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=n, cam=cam, cam2=cam2,
                lens=S.lens_features(cam["focal_depth"], cam["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "svgf_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    rd = lambda name, dt, c: np.fromfile(os.path.join(d, name + ".bin"), dt).reshape(H, W, c)
    assert np.array_equal(rd("h1", np.float32, 4), h1) and np.array_equal(rd("h2", np.float32, 4), h2)
    assert np.array_equal(rd("den", np.float32, 4), den) and np.array_equal(rd("draw_den", np.uint8, 4), draw_den)
    assert not np.array_equal(den, h2)


# ---- quality ----------------------------------------------------------------------------------------------------------------
def test_quality_against_the_fixed_rule(medium_scene, camera):
    """tools/temporal_quality.py's three sequences, the variance-guided filter against fspt_temporal_denoise on the same
    frames in the same process - the guided filter at the library's defaults against the fixed rule at the best row of its
    own scan for each sequence: lower relative MSE on the shadow-edge sequence, no worse on DESIGN 8.8's two.
    NOT an out-of-sample result: the guided defaults (K, sl) were chosen by a scan on these same three sequences, and
    sigma_normal / sigma_depth were never scanned; what the test holds is that the shipped defaults keep beating the
    fixed rule's per-sequence best on them."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import temporal_quality as Q
    r = Q.variance_comparison(medium_scene, camera)
    for name, row in r.items():
        print(name, {k: round(v, 6) for k, v in row.items()})
    assert r["edges"]["variance"] < r["edges"]["fixed_best"]
    assert r["camera"]["variance"] <= r["camera"]["fixed_best"] and r["geometry"]["variance"] <= r["geometry"]["fixed_best"]
