"""Temporal history clamp on the device (fspt_temporal_set_clamp): k_temporal_clamp against the float64
restatement tests/clamp_ref.py, its exact properties on the hook's own box, the fast history and the bit-identities on
a target with a moving camera, the hosts, and the change-of-light sequence of tools/temporal_quality.py.

Bounds (clamp_ref.tolerances; u = 2^-24, gamma(k) = k u / (1 - k u), cnt = the window's taps inside the image, A = mean |F|,
M2 = mean F^2 over them): mu to gamma(cnt) A (relative to mu for non-negative values: cnt - 1 additions and a division);
m2 - mu^2 to the ABSOLUTE e = gamma(cnt + 2) (M2 + 2 A^2) (cnt fmas and a division for m2, mu^2 with twice mu's error
and its own rounding, the subtraction's rounding); sd inherits min(e / (2 sd), sqrt(e)); lo, hi and a clamped output to
tol(mu) + sigma_scale tol(sd).  A value the restatement leaves unclamped must come back bit for bit.  Exempt: values whose
hist lies within that tolerance of lo or hi IN THE RESTATEMENT (their branch may flip); at most 1 % per case, also
asserted without a device by tests/test_clamp_cpu.py.  Measured on the MI355X: DESIGN 8.10."""
import os

import numpy as np
import pytest

import clamp_ref as R
from fspt_amd import PathTracer, scene as S, temporal_clamp_eval

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
_cases = {}


def case(W, H):
    """inputs and, per sigma_scale, the hook's result: computed once, shared, never written to"""
    if (W, H) not in _cases:
        hist, fast = R.synthetic(W, H)
        got = {s: temporal_clamp_eval(hist, fast, sigma_scale=s) for s in R.SIGMAS}
        for a in (hist, fast) + tuple(x for g in got.values() for x in g):
            a.setflags(write=False)
        _cases[(W, H)] = (hist, fast, got)
    return _cases[(W, H)]


def worst_ratio(err, tol):
    """max err / tol; a zero tolerance (a window of exact zeros) asks for a zero error"""
    ok = tol > 0
    r = np.where(ok, err / np.where(ok, tol, 1.0), np.where(err > 0, INF, 0.0))
    return float(np.max(r)) if r.size else 0.0


def check_case(W, H):
    hist, fast, got = case(W, H)
    h = hist[..., :3].astype(np.float64)
    worst = 0.0
    for s in R.SIGMAS:
        out, lo, hi = got[s]
        ref, rlo, rhi = R.clamp(hist, fast, s)
        assert np.array_equal(out[..., 3], hist[..., 3]), "the length is untouched"
        assert np.all(lo[..., 3] == 0) and np.all(hi[..., 3] == 0)
        if s == INF:
            assert np.array_equal(out, hist) and np.all(lo[..., :3] == -INF) and np.all(hi[..., :3] == INF)
            continue
        tol = R.tolerances(fast, s)[3]
        for name, g, r in (("lo", lo, rlo), ("hi", hi, rhi)):
            err = np.abs(g[..., :3].astype(np.float64) - r)
            ratio = worst_ratio(err, tol)
            print(f"{W}x{H} sigma_scale {s:g}: {name} worst error / bound {ratio:.4f}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (W, H, s, name, ratio)
        ex = R.exempt(hist, fast, s)
        assert ex.sum() <= R.EXEMPT_CAP * ex.size
        clamped = (ref[..., :3] != h) & ~ex
        kept = (ref[..., :3] == h) & ~ex
        assert np.array_equal(out[..., :3][kept], hist[..., :3][kept]), "a value inside the box comes back bit for bit"
        err = np.abs(out[..., :3].astype(np.float64) - ref[..., :3])[clamped]
        if err.size:
            ratio = worst_ratio(err, tol[clamped])
            print(f"{W}x{H} sigma_scale {s:g}: clamped output worst error / bound {ratio:.4f} ({int(clamped.sum())} clamped, {int(kept.sum())} kept, {int(ex.sum())} exempt)")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (W, H, s, ratio)
    print(f"{W}x{H}: worst error / bound {worst:.4f}")


# ---- 1. the hook against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_clamp_eval_against_restatement(W, H):
    check_case(W, H)


def test_clamp_eval_full_hd():
    check_case(*R.BIG_SHAPE)


# ---- 2. exact properties, on the hook's own box -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", R.SHAPES[2:])
def test_exact_properties_on_the_hooks_own_box(W, H):
    hist, fast, got = case(W, H)
    for s in (0.0, 1.0, 2.0):
        out, lo, hi = got[s]
        o, l, u, h = out[..., :3], lo[..., :3], hi[..., :3], hist[..., :3]
        assert np.all(l <= u)
        assert np.all(o >= l) and np.all(o <= u), "every output lies in [lo, hi]"
        inside = (h >= l) & (h <= u)
        assert np.array_equal(o[inside], h[inside]), "an input already inside is returned bit for bit"
        assert np.array_equal(o[h < l], l[h < l]) and np.array_equal(o[h > u], u[h > u])
        assert np.array_equal(out[..., 3], hist[..., 3])
        again, l2, u2 = temporal_clamp_eval(out, fast, sigma_scale=s)
        assert np.array_equal(again, out), "clamping twice is clamping once"
        assert np.array_equal(l2, lo) and np.array_equal(u2, hi)
        if s == 0.0:
            assert np.array_equal(lo, hi)
    if W >= 16:
        assert inside.any() and (~inside).any()


# ---- 3. the target path -----------------------------------------------------------------------------------------------------
CAMS = 4


def make_pt(arrays, W, H, cam):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    set_cam(pt, cam)
    return pt


def set_cam(pt, c):
    pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])


def moved(camera, k):
    c = dict(camera)
    c["P"] = [camera["P"][0] + 0.05 * k, camera["P"][1], camera["P"][2] + 0.025 * k]
    c["env_theta"] = camera["env_theta"] + (1.2 if k >= 2 else 0.0)  # (the light changes under the moving camera)
    return c


def run_frames(arrays, camera, W, H, clamp=None, moments=False, frames=CAMS, read_fast=True, **params):
    """frames of 2 spp from a camera that moves every frame -> (histories, fast histories, accumulators)"""
    pt = make_pt(arrays, W, H, camera)
    if moments:
        pt.temporal_set_moments(True)
    if clamp is not None:
        pt.temporal_set_clamp(True, **clamp)
    hs, fs, accs = [], [], []
    for k in range(frames):
        set_cam(pt, moved(camera, k))
        pt.clear(); pt.seed(3 + k); pt.render(2)
        if moments:
            pt.features(2, 1)
        acc = pt.readRadiance()
        hs.append(pt.temporal_accumulate(**params))
        if clamp is not None and read_fast:
            fs.append(pt.temporal_fast())
        assert np.array_equal(pt.readRadiance(), acc), "the accumulator is only read"
        accs.append(acc)
    pt.close()
    return hs, fs, accs


@pytest.fixture(scope="module")
def plain(small_scene, camera):
    """the mode off: the parent's long history with max_history 64 (the default) and with max_history = 6 (what the
    fast history of fast_history 6 must equal)"""
    W, H = 96, 64
    long_, _, accs = run_frames(small_scene, camera, W, H)
    short, _, _ = run_frames(small_scene, camera, W, H, max_history=6.0)
    for a in long_ + short + accs:
        a.setflags(write=False)
    return W, H, long_, short, accs


@pytest.mark.parametrize("moments", [False, True])
def test_sigma_inf_keeps_the_long_history_bit_for_bit(small_scene, camera, plain, moments):
    W, H, long_, short, accs = plain
    hs, fs, accs2 = run_frames(small_scene, camera, W, H, clamp=dict(fast_history=6.0, sigma_scale=INF), moments=moments)
    for k in range(CAMS):
        assert np.array_equal(hs[k], long_[k]), k
        assert np.array_equal(fs[k], short[k]), k
        assert np.array_equal(accs2[k], accs[k])  # later renders are unchanged
    assert (long_[-1][..., 3] > 2).mean() > 0.3  # the history was reprojected through the moves
    assert not np.array_equal(long_[-1], short[-1])


def test_fast_history_is_the_parents_accumulate_under_a_finite_clamp(small_scene, camera, plain):
    W, H, long_, short, accs = plain
    hs, fs, accs2 = run_frames(small_scene, camera, W, H, clamp=dict(fast_history=6.0, sigma_scale=1.0))
    for k in range(CAMS):
        assert np.array_equal(fs[k], short[k]), k  # the fast history never reads the (now clamped) long one
        assert np.array_equal(accs2[k], accs[k])
        assert np.array_equal(hs[k][..., 3], long_[k][..., 3]), "the length is not clamped"
    assert not np.array_equal(hs[-1], long_[-1])  # the clamp bound somewhere
    # every frame's history lies in the box the hook computes from that frame's fast history
    _, lo, hi = temporal_clamp_eval(hs[-1], fs[-1], sigma_scale=1.0)
    assert np.all(hs[-1][..., :3] >= lo[..., :3]) and np.all(hs[-1][..., :3] <= hi[..., :3])


def test_target_path_equals_the_hook(small_scene, camera):
    """pass 3 on a target = the hook on read-back buffers: the unclamped history of this frame comes from a twin target
    that runs the same frames with sigma_scale = +inf up to the last frame's blend"""
    W, H = 80, 56
    q = dict(fast_history=6.0, sigma_scale=1.5)
    a = make_pt(small_scene, W, H, camera); a.temporal_set_clamp(True, **q)
    b = make_pt(small_scene, W, H, camera); b.temporal_set_clamp(True, **q)
    for k in range(3):
        for pt in (a, b):
            set_cam(pt, moved(camera, k))
            pt.clear(); pt.seed(11 + k); pt.render(2)
        if k == 2:
            b.temporal_set_clamp(True, fast_history=6.0, sigma_scale=INF)  # parameters only: the history stays
        ha, hb = a.temporal_accumulate(), b.temporal_accumulate()
    fa, fb = a.temporal_fast(), b.temporal_fast()
    assert np.array_equal(fa, fb)
    assert (hb[..., 3] > 2).mean() > 0.3, "the parameter change kept the history"
    want, _, _ = temporal_clamp_eval(hb, fb, sigma_scale=1.5)
    assert np.array_equal(ha, want)
    assert not np.array_equal(ha, hb)
    assert a.temporal_clamp_last_ms() > 0.0 and b.temporal_clamp_last_ms() >= 0.0
    # the clamped value IS the history: the drawing reads it
    da, db = a.temporal_draw(1.0, 1.0), b.temporal_draw(1.0, 1.0)
    assert not np.array_equal(da, db)
    a.close(); b.close()


def test_states_reset_and_reenable(small_scene, camera):
    from fspt_amd import FsptError
    W, H = 64, 48
    pt = make_pt(small_scene, W, H, camera)
    pt.render(2)
    with pytest.raises(FsptError, match="clamp on"):
        pt.temporal_fast()
    with pytest.raises(FsptError, match="clamp on"):
        pt.temporal_clamp_last_ms()
    for bad in (dict(fast_history=0.5), dict(fast_history=INF), dict(sigma_scale=-1.0), dict(sigma_scale=float("nan"))):
        with pytest.raises(ValueError):
            pt.temporal_set_clamp(True, **bad)
    from fspt_amd import _lib as L
    for fh, ss in ((0.5, 2.0), (INF, 2.0), (float("nan"), 2.0), (16.0, -1.0), (16.0, float("nan"))):
        assert L.lib().fspt_temporal_set_clamp(pt._t, 1, fh, ss) == -1
    h0 = pt.temporal_accumulate()
    pt.temporal_set_clamp(True, fast_history=4.0, sigma_scale=INF)  # on over an existing history: it is dropped
    with pytest.raises(FsptError, match="clamp on"):
        pt.temporal_fast()
    h1 = pt.temporal_accumulate()
    most = lambda a, v: (a[..., 3] == v).mean() > 0.98  # (a static camera: every pixel but a few silhouette ones finds itself)
    assert np.all(h1[..., 3] == 2.0) and np.array_equal(h1[..., :3], h0[..., :3])  # a first frame again
    assert np.array_equal(pt.temporal_fast(), h1)
    h2 = pt.temporal_accumulate()
    f2 = pt.temporal_fast()
    assert most(h2, 4.0) and most(f2, 4.0)
    h3 = pt.temporal_accumulate()
    assert most(h3, 6.0) and most(pt.temporal_fast(), 4.0)  # capped at fast_history
    pt.temporal_set_clamp(True, fast_history=8.0, sigma_scale=3.0)  # parameters only: both histories stay
    h4 = pt.temporal_accumulate()
    assert most(h4, 8.0) and most(pt.temporal_fast(), 6.0)
    pt.temporal_reset()  # drops both
    with pytest.raises(FsptError, match="clamp on"):
        pt.temporal_fast()
    h5 = pt.temporal_accumulate()
    assert np.all(h5[..., 3] == 2.0) and np.all(pt.temporal_fast()[..., 3] == 2.0)
    pt.temporal_set_clamp(False)
    with pytest.raises(FsptError, match="clamp on"):
        pt.temporal_fast()
    h6 = pt.temporal_accumulate()
    assert most(h6, 4.0)  # switching off keeps the long history
    pt.temporal_set_clamp(True)  # re-enabled: both restart together
    h7 = pt.temporal_accumulate()
    assert np.all(h7[..., 3] == 2.0) and np.all(pt.temporal_fast()[..., 3] == 2.0)
    pt.close()


def test_dropping_the_history_drops_everything_that_describes_it(small_scene, camera):
    """The moments, the variance, the fast history and the denoised frame mean something only beside the history they were
    made from: whichever call drops the history - the other mode switched on, or a reset - every reader of them refuses
    with FSPT_E_STATE until the next accumulate, which starts all of them together."""
    from fspt_amd import FsptError
    pt = make_pt(small_scene, 16, 12, camera)
    pt.features(2, 1)

    def frame():
        pt.clear(); pt.render(2)
        return pt.temporal_accumulate()

    def all_refuse():
        for read in (pt.temporal_fast, lambda: pt.temporal_draw(1.0, 1.0, denoised=True),
                     lambda: pt.temporal_denoise(variance=True), pt.temporal_variance):
            with pytest.raises(FsptError) as e:
                read()
            assert e.value.code == -6  # FSPT_E_STATE

    def restarts():  # a first frame again: every length is the frame's 2 samples
        assert np.all(frame()[..., 3] == 2.0) and np.all(pt.temporal_fast()[..., 3] == 2.0)

    # A: the clamp on, a history, a denoised frame of it; then the moments on
    pt.temporal_set_clamp(True)
    frame(); pt.temporal_denoise(iterations=1); pt.temporal_fast()
    pt.temporal_set_moments(True)
    all_refuse()
    restarts()
    # C: both modes on, everything valid; then a reset
    pt.temporal_denoise(variance=True); pt.temporal_variance(); pt.temporal_draw(1.0, 1.0, denoised=True)
    pt.temporal_reset()
    all_refuse()
    restarts()
    # B: the moments on, a history and its variance; then the clamp on
    pt.temporal_set_clamp(False)
    frame(); pt.temporal_denoise(variance=True); pt.temporal_variance()
    pt.temporal_set_clamp(True)
    all_refuse()
    restarts()
    pt.close()


def test_no_memory_growth(small_scene, camera):
    from fspt_amd import device_memory
    pt = make_pt(small_scene, 128, 96, camera)
    pt.temporal_set_clamp(True)
    pt.render(1)
    pt.temporal_accumulate()
    pt.sync()
    free0 = device_memory(0)[0]
    for k in range(20):
        pt.temporal_set_clamp(True, sigma_scale=1.0 + k % 3)
        pt.temporal_accumulate(read=False)
    pt.sync()
    assert device_memory(0)[0] >= free0 - (1 << 20)
    pt.close()


# ---- 4. hosts ---------------------------------------------------------------------------------------------------------------
def _frames_by_hand(pattern, root, W, H, n_frames, clamp, seed=1):
    from fspt_amd import scene_file as F
    base, settings = F.load_scene_file(pattern.format(frame=0), root, bvh="sah", keep_order=True)
    pt = PathTracer(base, W, H, num_bounces=4)
    if clamp is not None:
        pt.temporal_set_clamp(True, **clamp)
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
        pt.temporal_accumulate(read=False)
        frames.append(pt.temporal_draw(settings["exposure"], 1.0)[::-1, :, :3].copy())
    pt.close(); pt.scene.close()
    return frames


def test_render_sequence_and_cli_clamp(tmp_path):
    import subprocess, sys
    from PIL import Image
    from fspt_amd import scene_file as F
    from test_temporal_gpu import _write_frames
    W, H = 48, 32
    pattern, root = _write_frames(tmp_path, 3)
    q = dict(fast_history=3.0, sigma_scale=0.5)
    out = F.render_sequence(pattern, range(3), str(tmp_path / "v" / "{frame}.png"), W, H, root, bvh="refit", temporal={"clamp": q})
    want = _frames_by_hand(pattern, root, W, H, 3, q)
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(out[k]))[:, :, :3], want[k]), k
    assert (want[2] > 0).mean() > 0.1
    assert not np.array_equal(want[2], _frames_by_hand(pattern, root, W, H, 3, None)[2])  # the clamp bound
    out = F.render_sequence(pattern, range(3), str(tmp_path / "d" / "{frame}.png"), W, H, root, bvh="refit", temporal={"clamp": True})
    dflt = _frames_by_hand(pattern, root, W, H, 3, {})
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(out[k]))[:, :, :3], dflt[k]), k
    half = _frames_by_hand(pattern, root, W, H, 3, dict(sigma_scale=0.5))
    for flag, ref in ((["--temporal-clamp"], dflt), (["--temporal-clamp", "0.5"], half)):
        outp = str(tmp_path / ("cli%d" % len(flag)) / "{frame}.png")
        subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--scene", pattern, "--assets", root, "--frames", "0:3", "--bvh", "refit",
                               "--temporal"] + flag + ["--bounces", "4", "--width", str(W), "--height", str(H), "--out", outp], cwd=ROOT, timeout=600)
        for k in range(3):
            assert np.array_equal(np.asarray(Image.open(outp.format(frame=k)))[:, :, :3], ref[k]), (flag, k)


def test_node_host_matches_python(tmp_path, small_scene, camera):
    import json, shutil, subprocess
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, n = 64, 48, 3
    cam = {k: camera[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")}
    cam2 = dict(cam); cam2["P"] = [cam["P"][0] + 0.1, cam["P"][1], cam["P"][2] + 0.05]
    cam3 = dict(cam2); cam3["env_theta"] = cam["env_theta"] + 1.5
    pt = make_pt(small_scene, W, H, cam)
    pt.temporal_set_clamp(True, fast_history=4.0, sigma_scale=1.0)
    hs = []
    for c, seed in ((cam, 3), (cam2, 7), (cam3, 9)):
        set_cam(pt, c)
        pt.clear(); pt.seed(seed); pt.render(n)
        hs.append(pt.temporal_accumulate())
    draw = pt.temporal_draw(1.2, 0.9, False)
    pt.close()
    d = str(tmp_path)
    e = small_scene
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins", "env"):
        getattr(e, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e.atlas_res, atlasLayers=e.atlas_layers, leafSize=e.leaf_size, envW=e.env_w, envH=e.env_h, W=W, H=H, n=n, cam=cam, cam2=cam2,
                lens=S.lens_features(cam["focal_depth"], cam["aperture"]), fastHistory=4.0, sigmaScale=1.0)
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "clamp_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    rd = lambda name, dt, c: np.fromfile(os.path.join(d, name + ".bin"), dt).reshape(H, W, c)
    for k in range(3):
        assert np.array_equal(rd("h%d" % (k + 1), np.float32, 4), hs[k]), k
    assert np.array_equal(rd("draw", np.uint8, 4), draw)


# ---- 5. quality -------------------------------------------------------------------------------------------------------------
def test_quality_over_a_change_of_light(camera):
    """tools/temporal_quality.py's LIGHT sequence (scene E3, 320 x 240, fixed camera, 4 spp per frame, 16 frames at env_theta
    t0, 8 at t0 + 90 degrees; relative MSE of the last frame against 4 096 spp at t0 + 90), the clamp off and on from the same
    inputs in the same process: on is below off, and within 1.5 x the on / off ratio measured on the MI355X."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import temporal_quality as Q
    r = Q.clamp_comparison(camera)["light"]
    print("light sequence:", {k: round(v, 6) for k, v in r.items()}, "on / off", round(r["on"] / r["off"], 4))
    assert r["on"] < r["off"]
    assert r["on"] / r["off"] <= 1.5 * Q.CLAMP_MEASURED["light_on_over_off"]
