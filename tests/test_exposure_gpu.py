"""Auto-exposure on the device (fspt_target_set_auto_exposure): k_exposure_histogram and k_exposure_resolve
against the restatement tests/exposure_ref.py, exact properties of the hook's own output, the mode on a target (every drawing
entry, the pipelined present, the states), and the hosts.

The histogram is integer work on float32 bits the restatement reproduces exactly: array_equal, no tolerance, no exempt set.
The mean is 256 products and sums in double with |v| <= 16 and a division: gamma(258) x 16 = 4.6e-13 (exposure_ref.GAMMA_BOUND);
the tolerance is an absolute 1e-9, whose slack covers only the device's double log2 / exp2 (the log2 of the exposure is held
to the same).  The exposure itself: within 2 float32 ulp of the restatement's."""
import os

import numpy as np
import pytest

import exposure_ref as R
from fspt_amd import PathTracer, exposure_eval, exposure_set_form, scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
gamma = lambda k: k * 2.0 ** -53 / (1 - k * 2.0 ** -53)
assert R.GAMMA_BOUND == gamma(258) * 16 and R.GAMMA_BOUND < R.MEAN_TOL == 1e-9
PREV = dict(R.FIRST, valid=1, log2_exposure=1.25, exposure=F(2.0 ** 1.25))
SLOW = dict(adapt_up=0.5, adapt_down=0.125)
_images = {}


def image(W, H, kind):
    """an input, made once, shared, never written to"""
    if (W, H, kind) not in _images:
        img = R.image(W, H, kind)
        img.setflags(write=False)
        _images[(W, H, kind)] = img
    return _images[(W, H, kind)]


def check_state(got, want, what):
    assert got["cleared"], "the resolve left counts in the histogram"
    assert got["valid"] == want["valid"] and got["metered"] == want["metered"], what
    if not want["valid"]:
        assert got["exposure"] == F(1.0), what
        return
    dm, de = abs(got["log2_mean"] - want["log2_mean"]), abs(got["log2_exposure"] - want["log2_exposure"])
    du = R.ulp_diff32(got["exposure"], want["exposure"])
    print(f"{what}: |mean - ref| {dm:.3e}, |log2 exposure - ref| {de:.3e} (bound {R.GAMMA_BOUND:.1e}, tolerance {R.MEAN_TOL:.0e}), exposure {du} ulp")
    assert dm <= R.MEAN_TOL and de <= R.MEAN_TOL and du <= 2, what


def check_case(W, H, kind, viewport=None):
    img = image(W, H, kind)
    ref_h = R.histogram(img, viewport)
    # a first metering with the defaults; one that adapts (from above and from below the target) with other percentiles and a key
    for prev, params in ((None, {}), (PREV, dict(SLOW, low=0.0, high=1.0, key=0.5)), (dict(PREV, log2_exposure=-7.5), dict(SLOW, low=0.45, high=0.55))):
        h, st = exposure_eval(img, viewport=viewport, prev=prev, **params)
        assert np.array_equal(h, ref_h), (W, H, kind, viewport)
        want = R.resolve(ref_h, prev, **params)
        if ref_h.sum() == 0:  # N = 0: the state is left as it was
            assert st["metered"] == (prev or R.FIRST)["metered"] and st["valid"] == (prev or R.FIRST)["valid"]
            assert st["exposure"] == (prev or R.FIRST)["exposure"] and st["log2_exposure"] == (prev or R.FIRST)["log2_exposure"] and st["cleared"]
            continue
        check_state(st, want, f"{W}x{H} {kind} {viewport} {sorted(params)}")


# ---- 1. the hook against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_eval_against_restatement(W, H, kind):
    check_case(W, H, kind)


@pytest.mark.parametrize("kind", R.KINDS)
def test_eval_with_a_viewport_smaller_than_the_image(kind):
    check_case(50, 37, kind, viewport=(23, 19))
    check_case(17, 33, kind, viewport=(17, 5))
    check_case(17, 33, kind, viewport=(1, 33))


@pytest.mark.parametrize("kind", R.KINDS)
def test_eval_full_hd(kind):
    check_case(*R.BIG_SHAPE, kind)


def test_both_forms_give_the_same_bits():
    try:
        for W, H, kind in ((50, 37, "constant"), (50, 37, "noise"), (17, 33, "special"), (1920, 1080, "edges"), (1920, 1080, "constant")):
            exposure_set_form(0)
            h0, s0 = exposure_eval(image(W, H, kind), prev=PREV, **SLOW)
            exposure_set_form(1)
            h1, s1 = exposure_eval(image(W, H, kind), prev=PREV, **SLOW)
            assert np.array_equal(h0, h1) and s0 == s1 and np.array_equal(h0, R.histogram(image(W, H, kind)))
    finally:
        exposure_set_form(0)  # the shipped one


# ---- 2. exact properties of the hook's own output ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(17, 33), (50, 37)])
def test_exact_properties(W, H):
    for kind in R.KINDS:
        img = image(W, H, kind)
        for vp in (None, (W - 3, H - 2)):
            h, st = exposure_eval(img, viewport=vp, prev=PREV, **SLOW)
            sub = img if vp is None else img[:vp[1], :vp[0]]
            L = R.luma(sub)
            with np.errstate(invalid="ignore"):
                kept = int((L >= F(2.0 ** -16)).sum())
            assert int(h.sum()) == kept and st["cleared"]
            assert st["metered"] == (kept if kept else PREV["metered"])
            h2, st2 = exposure_eval(img, viewport=vp, prev=PREV, **SLOW)  # the same previous state: identical bits
            assert np.array_equal(h, h2) and st == st2


@pytest.mark.parametrize("k", [-3, 5])
def test_scaling_by_a_power_of_two_shifts_the_histogram(k):
    rng = np.random.default_rng(2)
    img = np.ones((37, 50, 4), F)
    img[..., :3] = (2.0 ** rng.uniform(-9.0, 9.0, (37, 50, 3))).astype(F)  # (no value leaves [2^-16, 2^16) under either scale)
    wide = dict(min_log2=-30.0, max_log2=30.0)
    h0, s0 = exposure_eval(img, **wide)
    scaled = img.copy(); scaled[..., :3] *= F(2.0 ** k)
    h1, s1 = exposure_eval(scaled, **wide)
    assert h0.sum() == h1.sum() == 37 * 50
    assert np.array_equal(np.roll(h0, 8 * k), h1) and h0[: max(0, -8 * k)].sum() == 0 and h0[256 - max(0, 8 * k):].sum() == 0
    assert R.ulp_diff32(F(s1["exposure"] * F(2.0 ** k)), s0["exposure"]) <= 2
    assert abs(s1["log2_mean"] - (s0["log2_mean"] + k)) <= 2 * R.GAMMA_BOUND


# ---- 3. on a target ---------------------------------------------------------------------------------------------------------
W0, H0 = 64, 48


def make_pt(arrays, camera, W=W0, H=H0):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(**{k: camera[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")})
    pt.seed(5)
    return pt


def test_mode_off_is_the_parents_path_and_on_is_a_compensation(small_scene, camera):
    pt = make_pt(small_scene, camera)
    pt.render(4)
    rad = pt.readRadiance()
    before = [pt.draw(1.3, 0.9), pt.draw(0.7, 1.0, True, 2.0), pt.draw(1.0, 1.0, False, 3.0, 0.5)]
    pt.set_auto_exposure(True)
    assert pt.exposure() == (F(1.0), 0.0, 0)  # never metered: exposure 1
    on = pt.draw(1.3, 0.9)
    e, mean, n = pt.exposure()
    h, st = exposure_eval(rad)  # the target meters its accumulator: the hook on the read-back gives the same record
    assert (e, n) == (st["exposure"], st["metered"]) and mean == float(F(st["log2_mean"])) and 0 < n <= W0 * H0
    assert e != F(1.0)
    on2 = pt.draw(0.7, 1.0, True, 2.0)
    on3 = pt.draw(1.0, 1.0, False, 3.0, 0.5)
    assert pt.exposure()[0] == e  # (instant adaptation, a static accumulator)
    assert min(pt.exposure_last_ms()) > 0.0  # (histogram, resolve, k_draw_auto)
    assert np.array_equal(pt.readRadiance(), rad), "the accumulator is only read"
    pt.set_auto_exposure(False)
    assert [np.array_equal(a, b) for a, b in zip(before, [pt.draw(1.3, 0.9), pt.draw(0.7, 1.0, True, 2.0), pt.draw(1.0, 1.0, False, 3.0, 0.5)])] == [True] * 3
    assert np.array_equal(on, pt.draw(F(F(1.3) * e), 0.9))
    assert np.array_equal(on2, pt.draw(F(F(0.7) * e), 1.0, True, 2.0))
    assert np.array_equal(on3, pt.draw(F(e), 1.0, False, 3.0, 0.5))
    assert not np.array_equal(on, before[0])
    pt.close()


def test_denoised_and_temporal_draws_meter_their_own_buffers(small_scene, camera):
    pt = make_pt(small_scene, camera)
    pt.render(3)
    pt.features(4, 1)
    den = pt.denoise(iterations=2)
    hist = pt.temporal_accumulate()
    off = (pt.drawDenoised(1.1, 1.0), pt.temporal_draw(1.1, 1.0))
    pt.set_auto_exposure(True)
    d1 = pt.drawDenoised(1.1, 1.0)
    e1 = pt.exposure()
    d2 = pt.temporal_draw(1.1, 1.0)
    e2 = pt.exposure()
    assert e1[0] == exposure_eval(den)[1]["exposure"]
    assert e2[0] == exposure_eval(hist)[1]["exposure"] and e1[0] != e2[0]  # (each meters its own buffer: the filtered frame, the history)
    pt.set_auto_exposure(False)
    assert np.array_equal(d1, pt.drawDenoised(F(F(1.1) * e1[0]), 1.0)) and np.array_equal(d2, pt.temporal_draw(F(F(1.1) * e2[0]), 1.0))
    assert np.array_equal(off[0], pt.drawDenoised(1.1, 1.0)) and np.array_equal(off[1], pt.temporal_draw(1.1, 1.0))
    pt.close()


def test_present_keeps_its_latency_and_orders_the_state(small_scene, camera):
    """present k + 1 returns the frame fspt_draw gives after the same ticks; with a SLOW adaptation every frame's exposure
    depends on all the meterings before it, so equal frames also show that the state's read-modify-write is ordered across
    the two lanes' streams"""
    a, b, c = (make_pt(small_scene, camera) for _ in range(3))
    a.set_auto_exposure(True, **SLOW); b.set_auto_exposure(True, **SLOW)
    pattern = (2, 1, 3, 2, 0, 2, 1)
    got, ticks, want, ticks_off = [], [], [], []
    for n in pattern:
        for pt in (a, b, c):
            for _ in range(n):
                pt.tick()
        f, t = a.present(1.2, 0.9)
        got.append(None if f is None else f.copy()); ticks.append(t)
        ticks_off.append(c.present(1.2, 0.9)[1])
        want.append(b.draw(1.2, 0.9))
    assert ticks == ticks_off and ticks[0] == 0 and ticks[-1] == sum(pattern[:-1]), "the pipelining is intact"
    for k in range(1, len(pattern)):
        assert np.array_equal(got[k], want[k - 1]), k
    assert a.exposure() == b.exposure()  # (joins the present: the last frame's metering included)
    assert np.array_equal(a.readRadiance(), c.readRadiance())
    for pt in (a, b, c):
        pt.close()


def test_states_reset_reenable_and_a_cleared_target(small_scene, camera):
    from fspt_amd import FsptError, _lib as L
    pt = make_pt(small_scene, camera)
    pt.render(2)
    for call in (pt.exposure, pt.exposure_reset, pt.exposure_last_ms):
        with pytest.raises(FsptError):
            call()
    for bad in (dict(key=0.0), dict(low=0.9, high=0.1), dict(adapt_up=0.0), dict(min_log2=1.0, max_log2=0.0)):
        with pytest.raises(ValueError):
            pt.set_auto_exposure(True, **bad)
        prm = L.ExposureParams(*({**R.DEFAULTS, **bad}[k] for k in R.DEFAULTS))
        assert L.lib().fspt_target_set_auto_exposure(pt._t, 1, prm) == -1
    rad = pt.readRadiance()
    h = R.histogram(rad)
    pt.set_auto_exposure(True, **SLOW)
    pt.draw()
    s1 = R.resolve(h, None, **SLOW)
    assert pt.exposure()[0] == exposure_eval(rad, **SLOW)[1]["exposure"] and R.ulp_diff32(pt.exposure()[0], s1["exposure"]) <= 2
    assert pt.exposure()[2] == int(h.sum())  # (were the histogram not cleared, the second metering would count double)
    pt.set_auto_exposure(True, key=0.5, **SLOW)  # parameters only: the state stays, the next metering adapts from it
    pt.draw()
    s2 = R.resolve(h, s1, key=0.5, **SLOW)
    assert R.ulp_diff32(pt.exposure()[0], s2["exposure"]) <= 2 and pt.exposure()[2] == int(h.sum())
    assert s2["log2_exposure"] == pytest.approx(s1["log2_exposure"] + (np.log2(0.5 / 0.18)) * 0.125, abs=1e-6)
    kept = pt.exposure()
    pt.clear()  # a cleared target: N = 0, the exposure stays where it was
    blank = pt.draw()
    assert pt.exposure() == kept and len(np.unique(blank.reshape(-1, 4), axis=0)) == 1
    pt.seed(5); pt.render(2)
    rad = pt.readRadiance()
    h = R.histogram(rad)
    pt.exposure_reset()  # the next metering is a first one
    assert pt.exposure() == (F(1.0), 0.0, 0)
    pt.draw()
    assert R.ulp_diff32(pt.exposure()[0], R.resolve(h, None, key=0.5, **SLOW)["exposure"]) <= 2
    pt.set_auto_exposure(False)
    with pytest.raises(FsptError):
        pt.exposure()
    pt.set_auto_exposure(True)  # re-enabled: from a first metering, with the defaults
    assert pt.exposure() == (F(1.0), 0.0, 0)
    pt.draw()
    assert R.ulp_diff32(pt.exposure()[0], R.resolve(h)["exposure"]) <= 2
    pt.set_viewport(40, 20)  # the viewport is what is metered
    pt.draw()
    assert pt.exposure()[2] == int(R.histogram(rad, (40, 20)).sum())
    pt.close()
    sh = make_pt(small_scene, camera)
    sh.set_shard(0, 2, 32)
    with pytest.raises(FsptError) as ei:
        sh.set_auto_exposure(True)
    assert ei.value.code == -6
    sh.close()


def test_no_memory_growth(small_scene, camera):
    from fspt_amd import device_memory
    pt = make_pt(small_scene, camera, 128, 96)
    pt.set_auto_exposure(True)
    pt.render(1)
    pt.draw()
    pt.sync()
    free0 = device_memory(0)[0]
    for k in range(20):
        pt.set_auto_exposure(True, key=0.1 + 0.01 * k)
        pt.draw()
    pt.sync()
    assert device_memory(0)[0] >= free0 - (1 << 20)
    pt.close()


# ---- 4. hosts ---------------------------------------------------------------------------------------------------------------
def _frames_by_hand(pattern, root, W, H, n_frames, params, temporal, seed=1):
    from fspt_amd import scene_file as SF
    base, settings = SF.load_scene_file(pattern.format(frame=0), root, bvh="sah", keep_order=True)
    pt = PathTracer(base, W, H, num_bounces=4)
    pt.set_auto_exposure(True, **params)
    frames = []
    for k in range(n_frames):
        if k:
            g, settings = SF.load_scene_file(pattern.format(frame=k), root, geometry_only=True)
            tri, norm = S.geometry_in_leaf_order(base.meta["tri_order"], g.tri, g.norm)
            if temporal:
                pt.scene.motion_begin()
            pt.update_geometry(tri, norm)
        pt.clear()
        pt.eye, pt.dir = list(settings["eye"]), list(settings["dir"])
        pt.fovScale, pt.envTheta = settings["fov_scale"], settings["env_theta"]
        pt.lensFeatures = [settings["focus"], settings["aperture"]]
        pt.seed(seed + k if temporal else seed)
        pt.render(int(settings["samples"]))
        if temporal:
            pt.temporal_accumulate(read=False)
            frames.append(pt.temporal_draw(settings["exposure"], 1.0)[::-1, :, :3].copy())
        else:
            frames.append(pt.draw(settings["exposure"], 1.0)[::-1, :, :3].copy())
    pt.close(); pt.scene.close()
    return frames


def test_render_sequence_and_cli(tmp_path):
    import subprocess, sys
    from PIL import Image
    from fspt_amd import scene_file as SF
    from test_temporal_gpu import _write_frames
    W, H = 48, 32
    pattern, root = _write_frames(tmp_path, 3)
    slow = dict(adapt_up=SF.SEQUENCE_ADAPT, adapt_down=SF.SEQUENCE_ADAPT)
    load = lambda out: [np.asarray(Image.open(p))[:, :, :3] for p in out]
    for temporal in (False, True):
        kw = dict(bvh="refit", temporal=True if temporal else None)
        tag = "t" if temporal else "p"
        want = _frames_by_hand(pattern, root, W, H, 3, slow, temporal)
        got = load(SF.render_sequence(pattern, range(3), str(tmp_path / (tag + "a") / "{frame}.png"), W, H, root, auto_exposure=True, **kw))
        off = load(SF.render_sequence(pattern, range(3), str(tmp_path / (tag + "o") / "{frame}.png"), W, H, root, **kw))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and not np.array_equal(got[2], off[2])
        q = dict(key=0.3, adapt_up=1.0, adapt_down=1.0)
        got = load(SF.render_sequence(pattern, range(3), str(tmp_path / (tag + "q") / "{frame}.png"), W, H, root, auto_exposure=q, **kw))
        assert all(np.array_equal(g, w) for g, w in zip(got, _frames_by_hand(pattern, root, W, H, 3, q, temporal)))
    for flag, params in ((["--auto-exposure", "0.3"], dict(slow, key=0.3)),):
        outp = str(tmp_path / ("cli%d" % len(flag)) / "{frame}.png")
        subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--scene", pattern, "--assets", root, "--frames", "0:3", "--bvh", "refit",
                               "--temporal"] + flag + ["--bounces", "4", "--width", str(W), "--height", str(H), "--out", outp], cwd=ROOT, timeout=600)
        ref = _frames_by_hand(pattern, root, W, H, 3, params, True)
        for k in range(3):
            assert np.array_equal(np.asarray(Image.open(outp.format(frame=k)))[:, :, :3], ref[k]), (flag, k)


def test_node_host_matches_python(tmp_path, small_scene, camera):
    import json, shutil, subprocess
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, n = 64, 48, 3
    cam = {k: camera[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")}
    pt = PathTracer(small_scene, W, H, num_bounces=4)
    pt.set_camera(**cam)
    pt.set_auto_exposure(True, key=0.25, adapt_up=0.5, adapt_down=0.25)
    pt.seed(3); pt.render(n)
    d1 = pt.draw(1.2, 0.9, False, 3.0)
    s1 = pt.exposure()
    pt.envTheta = cam["env_theta"] + 1.5
    pt.clear(); pt.seed(7); pt.render(n)
    d2 = pt.draw(1.2, 0.9, False, 3.0)
    s2 = pt.exposure()
    pt.close()
    d = str(tmp_path)
    e = small_scene
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins", "env"):
        getattr(e, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e.atlas_res, atlasLayers=e.atlas_layers, leafSize=e.leaf_size, envW=e.env_w, envH=e.env_h, W=W, H=H, n=n, cam=cam,
                lens=S.lens_features(cam["focal_depth"], cam["aperture"]), params=dict(key=0.25, adaptUp=0.5, adaptDown=0.25))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "exposure_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    rd = lambda name: np.fromfile(os.path.join(d, name + ".bin"), np.uint8).reshape(H, W, 4)
    assert np.array_equal(rd("d1"), d1) and np.array_equal(rd("d2"), d2) and not np.array_equal(d1, d2)
    js = json.load(open(os.path.join(d, "state.json")))
    for got, want in zip(js, (s1, s2)):
        assert (F(got["exposure"]), got["log2Mean"], got["metered"]) == want
    assert s1[0] != s2[0]
