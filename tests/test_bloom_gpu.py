"""Bloom on the device (fspt_target_set_bloom): k_bloom_down, k_bloom_up, k_bloom_tail and the draw's mix against
the float64 restatement tests/bloom_ref.py, exact properties of the hook's own output, the mode on a target (every drawing
entry, the pipelined present, the allocation), and the hosts.

Every texel of every D_k, every U_k, B and c' is compared; there is no exempt set.  The tolerance is not chosen: it is
gamma(m) x the recursion run on magnitudes, m the roundings on the deepest path in the order fspt_tuning.h fixes (D_k 6 k,
U_k 6 n + 4 (n - k), B 10 n - 2, c' 10 n), plus 2^-126 per operation for results under the smallest normal float32
(bloom_ref.py's docstring has the count).  Measured on MI355X: the worst error was 0.689 of that bound (1920 x 1080 noise; 0.571 on the small shapes; the
tests print it per case)."""
import os

import numpy as np
import pytest

import bloom_ref as R
from fspt_amd import PathTracer, bloom_eval, bloom_set_form, bloom_set_tail_texels, exposure_eval, scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OTHER = dict(scatter=0.35, intensity=0.6, levels=8)
_images, _refs = {}, {}


def image(W, H, kind):
    """an input, made once, shared, never written to"""
    if (W, H, kind) not in _images:
        img = R.image(W, H, kind)
        img.setflags(write=False)
        _images[(W, H, kind)] = img
    return _images[(W, H, kind)]


def reference(W, H, kind, viewport=None, **params):
    key = (W, H, kind, viewport, tuple(sorted(params.items())))
    if key not in _refs:
        _refs[key] = R.pyramid(image(W, H, kind), viewport, **params)
    return _refs[key]


def compare(got, ref, what):
    """every texel of every array against the restatement; returns the worst error as a fraction of its bound"""
    ds, us, bloom, mix = got
    assert len(ds) == len(us) == ref["n"], what
    worst = 0.0
    pairs = [("D%d" % (k + 1), ds[k], ref["down"][k], ref["down_tol"][k]) for k in range(ref["n"])]
    pairs += [("U%d" % (k + 1), us[k], ref["up"][k], ref["up_tol"][k]) for k in range(ref["n"])]
    pairs += [("B", bloom, ref["bloom"], ref["bloom_tol"]), ("mix", mix, ref["mix"], ref["mix_tol"])]
    for name, g, r, tol in pairs:
        g = g[..., :3].astype(np.float64)
        assert g.shape == r.shape, (what, name)
        same = (g == r) | (np.isnan(g) & np.isnan(r))  # (identical values, the plainly drawn source's NaN and inf included)
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(g - r))
        frac = float(np.max(np.where(same, 0.0, err / np.where(tol > 0, tol, 1.0)), initial=0.0))
        worst = max(worst, frac)
        with np.errstate(invalid="ignore"):
            bad = ~same & ~(err <= tol)
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} texels beyond the bound, worst {frac:.3f} of it"
    print(f"{what}: worst error {worst:.3f} of the bound")
    return worst


def check_case(W, H, kind, viewport=None, param_sets=({}, OTHER)):
    img = image(W, H, kind)
    for params in param_sets:
        got = bloom_eval(img, viewport=viewport, **params)
        compare(got, reference(W, H, kind, viewport, **params), f"{W}x{H} {kind} {viewport} {sorted(params)}")
        assert np.array_equal(got[3][..., 3], img[..., 3]) and all((d[..., 3] == 0).all() for d in got[0] + got[1])


# ---- 1. the hook against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_eval_against_restatement(W, H, kind):
    check_case(W, H, kind)


@pytest.mark.parametrize("kind", ("constant", "tile", "noise", "special"))
def test_eval_with_a_viewport_smaller_than_the_image(kind):
    for (W, H), vp in R.VIEWPORTS:
        check_case(W, H, kind, viewport=vp)
        got = bloom_eval(image(W, H, kind), viewport=vp)
        outside = np.ones((H, W), bool); outside[:vp[1], :vp[0]] = False
        assert np.array_equal(got[3][outside].view(np.uint32), image(W, H, kind)[outside].view(np.uint32)), "outside the viewport: the source"


def test_eval_full_hd():
    check_case(*R.BIG_SHAPE, "noise", param_sets=({},))


def test_one_texel_wide_is_the_plain_draw():
    for W, H in ((1, 1), (1, 9), (9, 1)):
        img = image(W, H, "special")
        ds, us, bloom, mix = bloom_eval(img)
        assert ds == [] and us == [] and np.array_equal(mix.view(np.uint32), img.view(np.uint32))


# ---- 2. exact properties, bit for bit ---------------------------------------------------------------------------------------
def bits(got):
    ds, us, bloom, mix = got
    return [a.view(np.uint32) for a in ds + us + [bloom, mix]]


def forms(img, viewport=None, thresholds=(1 << 30, 1, 0), **params):
    """the hook's output in the per-level form and in the tail form at each threshold (everything the LDS holds in the tail,
    nothing, the shipped value)"""
    try:
        bloom_set_form(0)
        out = [bits(bloom_eval(img, viewport=viewport, **params))]
        bloom_set_form(1)
        for t in thresholds:
            bloom_set_tail_texels(t)
            out.append(bits(bloom_eval(img, viewport=viewport, **params)))
    finally:
        bloom_set_form(0); bloom_set_tail_texels(0)
    return out


@pytest.mark.parametrize("W,H", R.SHAPES)
def test_both_forms_give_the_same_bits(W, H):
    for kind in ("tile", "noise", "special"):
        for params in ({}, OTHER):
            base, *others = forms(image(W, H, kind), **params)
            for k, o in enumerate(others):
                assert len(o) == len(base) and all(np.array_equal(a, b) for a, b in zip(base, o)), (W, H, kind, params, k)
    (Wv, Hv), vp = R.VIEWPORTS[1]
    base, *others = forms(image(Wv, Hv, "noise"), viewport=vp)
    assert all(all(np.array_equal(a, b) for a, b in zip(base, o)) for o in others)


def test_both_forms_give_the_same_bits_full_hd():
    # 2048: 60 x 34 and below in the tail; 8192: 120 x 68 too (above 64 KiB of LDS); 2^30: whatever the LDS holds
    base, *others = forms(image(*R.BIG_SHAPE, "noise"), thresholds=(2048, 8192, 1 << 30))
    for k, o in enumerate(others):
        assert all(np.array_equal(a, b) for a, b in zip(base, o)), k


def test_constant_scaling_and_repeatability():
    for W, H in ((5, 7), (50, 37), (131, 67)):
        img = image(W, H, "constant")
        for params in ({}, OTHER):
            ds, us, bloom, mix = bloom_eval(img, **params)
            for a in ds + us + [bloom, mix]:
                assert (a[..., :3] == img[0, 0, :3]).all(), (W, H, params)
    rng = np.random.default_rng(4)
    img = np.ones((67, 131, 4), F)
    img[..., :3] = (2.0 ** rng.uniform(-4.0, 4.0, (67, 131, 3))).astype(F)  # (under the clamp and far from denormals at either scale)
    a = bloom_eval(img, scatter=0.5, intensity=0.25)
    assert all(np.array_equal(x, y) for x, y in zip(bits(a), bits(bloom_eval(img, scatter=0.5, intensity=0.25)))), "the same input twice"
    for k in (-3, 5):
        scaled = img.copy(); scaled[..., :3] *= F(2.0 ** k)
        b = bloom_eval(scaled, scatter=0.5, intensity=0.25)
        for x, y in zip(a[0] + a[1] + [a[2], a[3]], b[0] + b[1] + [b[2], b[3]]):
            assert np.array_equal(x[..., :3] * F(2.0 ** k), y[..., :3]), k
    sp = bloom_eval(image(50, 37, "special"), intensity=0.0)[3]
    assert np.array_equal(sp[..., :3], R.sanitise(image(50, 37, "special")[..., :3]).astype(F))  # intensity 0: s(input)


# ---- 3. on a target ---------------------------------------------------------------------------------------------------------
W0, H0 = 64, 48
PRM = dict(intensity=0.4, scatter=0.6, levels=4)  # (strong enough to move bytes at 64 x 48)


def make_pt(arrays, camera, W=W0, H=H0):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(**{k: camera[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")})
    pt.seed(5)
    return pt


class Plain:
    """a mode-off target whose accumulator is bound to a given buffer"""

    def __init__(self, arrays, camera):
        self.pt = make_pt(arrays, camera)

    def on(self, buf):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(buf, F)).to("cuda:0")
        torch.cuda.synchronize()
        self.pt.bind_accumulator(t.data_ptr(), keep=t)
        return self.pt


def test_every_drawing_entry_draws_the_mix(small_scene, camera):
    pt = make_pt(small_scene, camera)
    plain = Plain(small_scene, camera)
    pt.render(4)
    rad = pt.readRadiance()
    calls = [lambda p, e=1.0: p.draw(F(F(1.3) * F(e)), 0.9), lambda p, e=1.0: p.draw(F(F(1.0) * F(e)), 1.0, False, 3.0, 0.5),
             lambda p, e=1.0: p.draw(F(F(0.8) * F(e)), 1.0, False, 3.0, 0.25)]
    before = [c(pt) for c in calls] + [pt.draw(0.7, 1.0, True, 2.0)]
    assert pt.bloom is None
    pt.set_bloom(True, **PRM)
    assert pt.bloom == {"intensity": float(F(0.4)), "scatter": float(F(0.6)), "levels": 4}
    mix = bloom_eval(rad, **PRM)[3]
    for k, c in enumerate(calls):  # fspt_draw, fspt_draw_scaled at two scales
        on = c(pt)
        assert np.array_equal(on, c(plain.on(mix))), k
        assert not np.array_equal(on, before[k]), k
    assert min(pt.bloom_last_ms()) >= 0.0 and pt.bloom_last_ms()[0] > 0.0 and pt.bloom_last_ms()[3] > 0.0
    # a viewport smaller than the image: the pyramid is the viewport's, texels outside it are drawn plain
    pt.set_viewport(40, 20)
    mix_vp = bloom_eval(rad, viewport=(40, 20), **PRM)[3]
    for c in calls[:2]:
        assert np.array_equal(c(pt), c(plain.on(mix_vp)))
    assert not np.array_equal(mix_vp, mix)
    pt.set_viewport(0, 0)
    # with auto-exposure on: the source buffer is metered, not the bloomed one
    pt.set_auto_exposure(True)
    on = [c(pt) for c in calls]
    e = pt.exposure()[0]
    assert e == exposure_eval(rad)[1]["exposure"] and e != F(1.0)
    for k, c in enumerate(calls):
        assert np.array_equal(on[k], c(plain.on(mix), e)), k
    pt.set_auto_exposure(False)
    # intensity 0, with and without the firefly filter: the mode-off bytes
    pt.set_bloom(True, intensity=0.0)
    assert np.array_equal(pt.draw(1.3, 0.9), before[0]) and np.array_equal(pt.draw(0.7, 1.0, True, 2.0), before[3])
    assert np.array_equal(pt.readRadiance(), rad), "the accumulator is only read"
    pt.set_bloom(False)
    assert pt.bloom is None
    assert all(np.array_equal(a, b) for a, b in zip(before, [c(pt) for c in calls] + [pt.draw(0.7, 1.0, True, 2.0)])), "off again: the same bytes"
    pt.close(); plain.pt.close()


def test_denoised_and_temporal_draws_bloom_their_own_buffers(small_scene, camera):
    pt = make_pt(small_scene, camera)
    plain = Plain(small_scene, camera)
    pt.render(3)
    pt.features(4, 1)
    den = pt.denoise(iterations=2)
    hist = pt.temporal_accumulate()
    off = (pt.drawDenoised(1.1, 1.0), pt.temporal_draw(1.1, 1.0))
    for auto in (False, True):
        pt.set_bloom(True, **PRM)
        if auto:
            pt.set_auto_exposure(True)
        d1 = pt.drawDenoised(1.1, 0.95)
        e1 = pt.exposure()[0] if auto else F(1.0)
        d2 = pt.temporal_draw(1.1, 0.95)
        e2 = pt.exposure()[0] if auto else F(1.0)
        assert np.array_equal(d1, plain.on(bloom_eval(den, **PRM)[3]).draw(F(F(1.1) * e1), 0.95, False, 0.0, 1.0))
        assert np.array_equal(d2, plain.on(bloom_eval(hist, **PRM)[3]).draw(F(F(1.1) * e2), 0.95, False, 0.0, 1.0))
        assert not np.array_equal(d1, d2)
        pt.set_bloom(False); pt.set_auto_exposure(False)
    assert np.array_equal(off[0], pt.drawDenoised(1.1, 1.0)) and np.array_equal(off[1], pt.temporal_draw(1.1, 1.0))
    pt.close(); plain.pt.close()


def test_present_keeps_its_latency_and_orders_the_pyramid(small_scene, camera):
    """present k + 1 returns the frame fspt_draw gives after the same ticks, and its ticks sequence is the mode-off one; the
    pyramid is rewritten by every frame on alternating streams, so equal frames also show that its reuse is ordered"""
    a, b, c = (make_pt(small_scene, camera) for _ in range(3))
    a.set_bloom(True, **PRM); b.set_bloom(True, **PRM)
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
    assert np.array_equal(a.readRadiance(), c.readRadiance())
    plain = Plain(small_scene, camera)
    assert np.array_equal(want[-1], plain.on(bloom_eval(b.readRadiance(), **PRM)[3]).draw(1.2, 0.9))
    for pt in (a, b, c, plain.pt):
        pt.close()


def test_refusals_allocation_and_memory(small_scene, camera):
    from fspt_amd import FsptError, _lib as L, device_memory
    pt = make_pt(small_scene, camera, 128, 96)
    with pytest.raises(FsptError):
        pt.bloom_last_ms()
    for bad in (dict(intensity=-0.1), dict(scatter=2.0), dict(levels=0), dict(levels=9)):
        with pytest.raises(ValueError):
            pt.set_bloom(True, **bad)
        prm = L.BloomParams(*({**R.DEFAULTS, **bad}[k] for k in R.DEFAULTS))
        assert L.lib().fspt_target_set_bloom(pt._t, 1, prm) == -1
    assert pt.bloom is None
    pt.render(1)
    pt.sync()
    free_off = device_memory(0)[0]
    pt.set_bloom(True)
    pt.draw()
    pt.sync()
    free0 = device_memory(0)[0]
    assert free0 <= free_off  # (the pyramid: 128 x 96 x 16 / 3 bytes, below the allocator's granule or not)
    first = pt.draw()
    for k in range(20):  # a parameter change keeps the allocation; 20 draws do not grow
        pt.set_bloom(True, intensity=0.05 + 0.01 * k, levels=1 + k % 8)
        pt.draw()
    pt.sync()
    assert device_memory(0)[0] >= free0 - (1 << 20)
    pt.set_bloom(True)
    assert np.array_equal(pt.draw(), first)
    pt.set_bloom(False)
    pt.sync()
    assert device_memory(0)[0] >= free0
    pt.close()
    sh = make_pt(small_scene, camera)
    sh.set_shard(0, 2, 32)
    with pytest.raises(FsptError) as ei:
        sh.set_bloom(True)
    assert ei.value.code == -6
    sh.close()


# ---- 4. hosts ---------------------------------------------------------------------------------------------------------------
def _frames_by_hand(pattern, root, W, H, n_frames, params, temporal, seed=1):
    from fspt_amd import scene_file as SF
    base, settings = SF.load_scene_file(pattern.format(frame=0), root, bvh="sah", keep_order=True)
    pt = PathTracer(base, W, H, num_bounces=4)
    pt.set_bloom(True, **params)
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
    pattern, root = _write_frames(tmp_path, 2)
    load = lambda out: [np.asarray(Image.open(p))[:, :, :3] for p in out]
    q = dict(intensity=0.3, scatter=0.5, levels=3)
    for temporal in (False, True):
        kw = dict(bvh="refit", temporal=True if temporal else None)
        tag = "t" if temporal else "p"
        got = load(SF.render_sequence(pattern, range(2), str(tmp_path / (tag + "a") / "{frame}.png"), W, H, root, bloom=q, **kw))
        off = load(SF.render_sequence(pattern, range(2), str(tmp_path / (tag + "o") / "{frame}.png"), W, H, root, **kw))
        want = _frames_by_hand(pattern, root, W, H, 2, q, temporal)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and not np.array_equal(got[1], off[1])
    got = load(SF.render_sequence(pattern, range(2), str(tmp_path / "b" / "{frame}.png"), W, H, root, bloom=True))  # (a tracer per frame)
    assert all(np.array_equal(g, w) for g, w in zip(got, _frames_by_hand(pattern, root, W, H, 2, {}, False)))
    outp = str(tmp_path / "cli" / "{frame}.png")
    subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--scene", pattern, "--assets", root, "--frames", "0:2", "--bvh", "refit",
                           "--temporal", "--bloom", "0.3", "--bounces", "4", "--width", str(W), "--height", str(H), "--out", outp], cwd=ROOT, timeout=600)
    ref = _frames_by_hand(pattern, root, W, H, 2, dict(intensity=0.3), True)
    for k in range(2):
        assert np.array_equal(np.asarray(Image.open(outp.format(frame=k)))[:, :, :3], ref[k]), k


def test_node_host_matches_python(tmp_path, small_scene, camera):
    import json, shutil, subprocess
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, n = 64, 48, 3
    cam = {k: camera[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")}
    pt = PathTracer(small_scene, W, H, num_bounces=4)
    pt.set_camera(**cam)
    pt.set_bloom(True, **PRM)
    pt.seed(3); pt.render(n)
    d1, s1 = pt.draw(1.2, 0.9, False, 3.0), pt.bloom
    pt.set_bloom(True, intensity=0.9, levels=2)
    d2, s2 = pt.draw(1.2, 0.9, True, 2.0), pt.bloom
    pt.set_bloom(False)
    d3 = pt.draw(1.2, 0.9, False, 3.0)
    pt.close()
    d = str(tmp_path)
    e = small_scene
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins", "env"):
        getattr(e, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e.atlas_res, atlasLayers=e.atlas_layers, leafSize=e.leaf_size, envW=e.env_w, envH=e.env_h, W=W, H=H, n=n, cam=cam,
                lens=S.lens_features(cam["focal_depth"], cam["aperture"]), params=PRM, params2=dict(intensity=0.9, levels=2))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "bloom_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    rd = lambda name: np.fromfile(os.path.join(d, name + ".bin"), np.uint8).reshape(H, W, 4)
    assert np.array_equal(rd("d1"), d1) and np.array_equal(rd("d2"), d2) and np.array_equal(rd("d3"), d3)
    assert len({d1.tobytes(), d2.tobytes(), d3.tobytes()}) == 3
    assert json.load(open(os.path.join(d, "state.json"))) == [s1, s2, None]
