"""The GPU sky on the MI355X: k_sky_generate against the float64 restatement of the model, the summed-area
table against math.fsum, fspt_env_bins_gpu against fspt_env_bins byte for byte, and a live scene whose light is generated,
binned and tiled on the device against a scene created fresh from the same bytes - no tolerance there."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import envbins_ref as E
import sky_cases as SC
import sky_ref as K
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S
from refit_moves import rotated

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 96, 64, 8
SUN = (0.5, 0.6, 0.4)
SKY_W, SKY_H = 64, 32


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", SC.GEN_SAMPLES, ids=lambda s: f"n{s[0]}m{s[1]}")
@pytest.mark.parametrize("size", SC.GEN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generator_against_float64(size, samples):
    """linear_out against sky_ref in float64, per channel relative to |ref| + 1e-6 I gain.  The bound is 8 x the error of the
    same restatement run in float32 on the same case (another summation order, the hardware's exp and sin: a few float32
    roundings more, whatever the kernel is); rgbe_out is the restated encode of the kernel's own linear_out, byte for byte."""
    w, h = size
    for name, sun, kw in SC.generator_cases(w, h, samples):
        rgbe, _, _, lin = S.sky(sun, w, h, linear=True, **kw)
        ref64, _ = K.sky(sun, w, h, **kw)
        ref32, _ = K.sky(sun, w, h, dtype=np.float32, **kw)
        assert np.isfinite(lin).all()
        bound = 8.0 * K.rel_error(ref32, ref64)
        err = K.rel_error(lin, ref64)
        print(f"sky {w}x{h} N{samples[0]} M{samples[1]} {name}: gpu {err:.3e} float32 restatement {bound / 8:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
        assert np.array_equal(rgbe.reshape(h, w, 4), K.encode(lin)), name


def test_generator_outputs_are_optional_and_repeatable():
    p = S.sky_params(SUN)
    rgbe = np.zeros(SKY_W * SKY_H * 4, np.uint8)
    lin = np.zeros(SKY_W * SKY_H * 3, np.float32)
    lib = L.lib()
    assert lib.fspt_sky_generate(0, C.byref(p), SKY_W, SKY_H, L.u8ptr(rgbe), None) == 0
    assert lib.fspt_sky_generate(0, C.byref(p), SKY_W, SKY_H, None, L.fptr(lin)) == 0
    assert lib.fspt_sky_generate(0, C.byref(p), SKY_W, SKY_H, None, None) == 0
    both = S.sky(SUN, SKY_W, SKY_H, linear=True)
    assert np.array_equal(both[0], rgbe) and np.array_equal(both[3].reshape(-1).view(np.uint32), lin.view(np.uint32))
    # a longer sun vector is the same sun
    assert np.array_equal(S.sky(tuple(3.0 * c for c in SUN), SKY_W, SKY_H)[0], rgbe)
    assert rgbe.reshape(-1, 4)[:, :3].max() > 0


# ---- the summed-area table -------------------------------------------------------------------------------------------
def box_sums(env, w, h, boxes):
    out = np.zeros(len(boxes), np.float64)
    boxes = np.ascontiguousarray(boxes, np.uint32)
    L.check(L.lib().fspt_env_box_sums_eval(0, L.u8ptr(env), w, h, L.u32ptr(boxes), len(boxes), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


@pytest.mark.parametrize("size", SC.BOX_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_box_sums_against_fsum(size):
    """each sum within 4 w h 2^-53 total of the correctly rounded one (four table entries, each a float64 sum of at most w h
    non-negative terms, in whatever order); two runs give the same bytes"""
    w, h = size
    env = SC.box_map(w, h)
    rad = E.radiance(env, w, h)
    total = math.fsum(rad.ravel())
    assert total > 0
    boxes = SC.boxes_for(w, h)
    got = box_sums(env, w, h, boxes)
    tol = 4.0 * w * h * 2.0 ** -53 * total
    worst = 0.0
    for b, g in zip(boxes, got):
        want = E.box_sum(rad, b)
        worst = max(worst, abs(g - want))
        assert abs(g - want) <= tol, (tuple(b), g, want, tol)
    print(f"box sums {w}x{h}: worst |error| {worst:.3e}, bound {tol:.3e}, total {total:.6e}")
    assert np.array_equal(got.view(np.uint64), box_sums(env, w, h, boxes).view(np.uint64))


# ---- the bins --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bins_maps():
    return SC.bins_maps()


BINS_NAMES = (*(f"{k}_{w}x{h}" for w, h in SC.BINS_SYNTHETIC for k in ("synthetic", "sky")), "zero_16x8", "hot_32x16",
              *(f"odd_{w}x{h}" for w, h in SC.BINS_NAN), "golden_odd")


def test_bins_names_are_the_maps(bins_maps):
    assert sorted(BINS_NAMES) == sorted(bins_maps)


@pytest.mark.parametrize("name", BINS_NAMES)
def test_gpu_bins_equal_cpu_bins(bins_maps, name):
    env, w, h = bins_maps[name]
    want = S.env_bins(env, w, h)
    got = S.env_bins(env, w, h, device=0)
    assert got.size == want.size and np.array_equal(got, want), (got.size // 4, want.size // 4)
    if name == "zero_16x8":
        assert got.tolist() == [0, 0, 16, 8]
    # the count alone, and a capacity below it
    n = C.c_uint32()
    L.check(L.lib().fspt_env_bins_gpu(L.u8ptr(env), w, h, 0, None, 0, C.byref(n)))
    assert n.value == want.size // 4
    if n.value > 1:
        part = np.full(4 * n.value, 0xFFFFFFFF, np.uint32)
        L.check(L.lib().fspt_env_bins_gpu(L.u8ptr(env), w, h, 0, L.u32ptr(part), n.value - 1, C.byref(n)))
        assert n.value == want.size // 4 and np.array_equal(part[:-4], want[:-4]) and (part[-4:] == 0xFFFFFFFF).all()


def test_gpu_bins_of_a_gpu_sky():
    rgbe, w, h = S.sky(SUN, 256, 128)
    assert E.decision_margin(rgbe, w, h) >= 1e-6  # (the condition under which the order of a float64 sum cannot matter)
    assert np.array_equal(S.env_bins(rgbe, w, h, device=0), S.env_bins(rgbe, w, h))


# ---- a live scene ----------------------------------------------------------------------------------------------------
def make_pt(sc, pipeline="wavefront", sampler=None, seed=7):
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if sampler:
        pt.set_sampler(sampler, 11)
    return pt


def frame(sc, n=TICKS, **kw):
    pt = make_pt(sc, **kw)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img.view(np.uint32)


def with_map(a, env, w, h):
    return dataclasses.replace(a, env=np.asarray(env, np.uint8), env_w=w, env_h=h, bins=S.env_bins(env, w, h))


def with_sky(a, sun=SUN, w=SKY_W, h=SKY_H, **kw):
    """`a` under fspt_sky_generate's bytes and fspt_env_bins of them: what update_sky must be indistinguishable from"""
    rgbe, w, h = S.sky(sun, w, h, **kw)
    return with_map(a, rgbe, w, h)


def light(sc):
    return [sc.read_appearance("env"), sc.read_appearance("bins")]


def assert_same_light(A, B, kws=(dict(),)):
    for x, y in zip(light(A), light(B)):
        assert x.size == y.size and np.array_equal(x, y)
    for kw in kws:
        fa, fb = frame(A, **kw), frame(B, **kw)
        assert np.array_equal(fa, fb), (kw, int((fa != fb).any(-1).sum()))


ALL = [dict(pipeline=p, sampler=s) for p in ("wavefront", "stream") for s in (None, "sobol")]


@pytest.mark.parametrize("case", ("default", "odd_size_dusk"))
def test_update_sky_equals_fresh_scene(small_scene, case):
    kw = dict() if case == "default" else dict(sun=(0.9, 0.05, -0.3), w=65, h=33, turbidity=4.0, gain=2.0, ground_albedo=(0.1, 0.5, 0.9))
    B = Scene(with_sky(small_scene, **kw))
    A = Scene(small_scene)
    f0 = frame(A)
    A.update_sky(kw.get("sun", SUN), kw.get("w", SKY_W), kw.get("h", SKY_H), **{k: v for k, v in kw.items() if k not in ("sun", "w", "h")})
    assert_same_light(A, B, ALL)
    assert not np.array_equal(frame(A), f0)
    last = A.last_sky()
    assert last["sky_ms"] > 0 and last["bins_ms"] > 0 and last["tile_ms"] > 0 and last["readbacks"] == 1
    assert last["n_bins"] == B.arrays.bins.size // 4 and last["launches"] == 1 + 3 + 1 + 66 + 1 + 1 + 1
    A.close(); B.close()


def test_auto_and_device_forms(small_scene):
    import torch
    rgbe, w, h = S.sky(SUN, SKY_W, SKY_H)
    B = Scene(with_map(small_scene, rgbe, w, h))
    A = Scene(small_scene)
    A.update_environment(rgbe, w, h)  # bins=None: fspt_scene_update_environment_auto
    assert_same_light(A, B, ALL[:2])
    assert A.last_sky()["sky_ms"] == 0.0 and A.last_sky()["launches"] == 3 + 1 + 66 + 1 + 1 + 1
    A.close()
    A = Scene(small_scene)
    t = torch.from_numpy(rgbe.copy()).to("cuda:0")
    A.update_environment(t, w, h)  # a tensor on the scene's device: fspt_scene_update_environment_device
    assert_same_light(A, B, ALL[:2])
    assert np.array_equal(t.cpu().numpy(), rgbe)  # read in place, not written
    # another map, other bins: the synthetic one
    env, w2, h2 = S.synthetic_env(15, 7)
    A.update_environment(env, w2, h2)
    C2 = Scene(with_map(small_scene, env, w2, h2))
    assert_same_light(A, C2)
    A.close(); B.close(); C2.close()


def test_there_and_back(small_scene):
    sc = Scene(small_scene)
    f0 = frame(sc)
    sc.update_sky(SUN, SKY_W, SKY_H)
    B = Scene(with_sky(small_scene))
    assert_same_light(sc, B)
    B.close()
    sc.update_environment(None, 0, 0, np.array([0, 0, 1, 1], np.uint32))
    none = dataclasses.replace(small_scene, env=None, env_w=0, env_h=0, bins=np.array([0, 0, 1, 1], np.uint32))
    B = Scene(none)
    assert_same_light(sc, B)
    B.close()
    sc.update_environment(small_scene.env, small_scene.env_w, small_scene.env_h)
    assert np.array_equal(frame(sc), f0)
    sc.close()


def test_composes_with_refit_and_materials():
    import appearance_cases as AC
    import refit_ref as R
    t = S.textured_test_scene(16)
    a1 = AC.retex(t, 9, 5, 81, new_uv=True)
    tri, norm = rotated(t.tri, t.norm)
    want = with_sky(dataclasses.replace(a1, tri=tri, norm=norm, bvh=R.refit(a1.bvh, tri)))
    B = Scene(want)
    steps = {"sky": lambda A: A.update_sky(SUN, SKY_W, SKY_H), "geometry": lambda A: A.update_geometry(tri, norm),
             "materials": lambda A: A.update_materials(a1.mat, a1.uv, a1.atlas, a1.atlas_res, a1.atlas_layers)}
    for order in (("sky", "geometry", "materials"), ("materials", "geometry", "sky")):
        A = Scene(t)
        for s in order:
            steps[s](A)
        for k in range(6):
            assert np.array_equal(A.read_appearance(k), B.read_appearance(k)), (order, k)
        assert np.array_equal(frame(A), frame(B)), order
        A.close()
    B.close()


def test_recorded_ticks_and_a_present_see_the_old_light(small_scene):
    out = []
    for sync_first in (False, True):
        sc = Scene(small_scene); pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        sc.update_sky(SUN, SKY_W, SKY_H)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance().view(np.uint32))
        pt.close(); sc.close()
    assert np.array_equal(out[0], out[1])
    sc = Scene(small_scene); pt = make_pt(sc)
    ref = Scene(small_scene); pr = make_pt(ref)
    for _ in range(2):
        pt.tick(); pr.tick()
    img, n = pt.present()
    assert img is None and n == 0
    pre = pr.draw()
    sc.update_sky(SUN, SKY_W, SKY_H); ref.update_sky(SUN, SKY_W, SKY_H)
    for _ in range(2):
        pt.tick(); pr.tick()
    img, n = pt.present()
    assert n == 2 and np.array_equal(img, pre)  # the frame in flight: the old light, once
    post = pr.draw()
    assert not np.array_equal(post, pre)
    pt.tick(); pr.tick()
    img, n = pt.present()
    assert n == 4 and np.array_equal(img, post)
    pt.close(); pr.close(); sc.close(); ref.close()


def test_refused_calls_leave_the_scene_unchanged(small_scene):
    import torch
    sc = Scene(small_scene)
    sc.update_sky(SUN, SKY_W, SKY_H)
    before, last = light(sc), sc.last_sky()
    lib, h = L.lib(), sc._h
    env = L.u8ptr(small_scene.env)
    good = S.sky_params(SUN)
    bad = [S.sky_params((0, 0, 0)), S.sky_params((float("nan"), 1, 0)), S.sky_params(SUN, turbidity=65.0), S.sky_params(SUN, sun_radius=0.0),
           S.sky_params(SUN, view_samples=65), S.sky_params(SUN, light_samples=0), S.sky_params(SUN, ground_albedo=1.5), S.sky_params(SUN, gain=-1.0)]
    odd = torch.zeros(SKY_W * SKY_H * 4 + 1, dtype=torch.uint8, device="cuda:0")
    calls = [lambda: lib.fspt_scene_update_sky(None, C.byref(good), 8, 4), lambda: lib.fspt_scene_update_sky(h, None, 8, 4),
             lambda: lib.fspt_scene_update_sky(h, C.byref(good), 0, 4), lambda: lib.fspt_scene_update_sky(h, C.byref(good), 8, 65536),
             *(lambda p=p: lib.fspt_scene_update_sky(h, C.byref(p), 8, 4) for p in bad),
             lambda: lib.fspt_scene_update_environment_auto(None, env, 64, 32), lambda: lib.fspt_scene_update_environment_auto(h, None, 64, 32),
             lambda: lib.fspt_scene_update_environment_auto(h, env, 0, 32), lambda: lib.fspt_scene_update_environment_auto(h, env, 64, 65536),
             lambda: lib.fspt_scene_update_environment_device(h, None, 64, 32),
             lambda: lib.fspt_scene_update_environment_device(h, C.c_void_p(odd.data_ptr() + 1), SKY_W, SKY_H)]
    for k, call in enumerate(calls):
        assert call() == -1, k
    for x, y in zip(before, light(sc)):
        assert np.array_equal(x, y)
    assert sc.last_sky() == last
    with pytest.raises(ValueError):
        sc.update_environment(np.zeros(15, np.uint8), 2, 2)
    with pytest.raises(TypeError):
        sc.update_environment(torch.zeros(16, dtype=torch.float32, device="cuda:0"), 2, 2)
    sc.close()


def test_history_is_kept_over_a_sky_change(small_scene):
    out = {}
    for how in ("same", "other"):
        sc = Scene(small_scene); pt = make_pt(sc)
        sc.update_sky(SUN, SKY_W, SKY_H)
        pt.render(TICKS)
        pt.temporal_accumulate(read=False)
        sc.update_sky(SUN if how == "same" else (-0.7, 0.2, 0.1), SKY_W, SKY_H)
        pt.clear(); pt.render(TICKS)
        out[how] = pt.temporal_accumulate()
        pt.close(); sc.close()
    a, b = out["same"], out["other"]
    assert np.array_equal(a[..., 3].view(np.uint32), b[..., 3].view(np.uint32)) and (a[..., 3] > 1).any()
    assert not np.array_equal(a[..., :3], b[..., :3])


def test_multi_update_sky_equals_single_scene(small_scene):
    m = MultiPathTracer(small_scene, W, H, devices=(0,), num_bounces=4)
    m.set_camera(**CAM); m.seed(7)
    m.render(2)
    m.update_sky(SUN, SKY_W, SKY_H)
    m.clear(); m.seed(7); m.render(TICKS)
    got = m.readRadiance().view(np.uint32)
    B = Scene(with_sky(small_scene))
    assert np.array_equal(got, frame(B))
    rgbe, w, h = S.sky((-0.7, 0.2, 0.1), SKY_W, SKY_H)
    m.update_environment(rgbe, w, h)
    m.clear(); m.seed(7); m.render(TICKS)
    got = m.readRadiance().view(np.uint32)
    m.close(); B.close()
    B = Scene(with_map(small_scene, rgbe, w, h))
    assert np.array_equal(got, frame(B))
    B.close()


# ---- sequences -------------------------------------------------------------------------------------------------------
def test_render_sequence_sky(tmp_path):
    """three frames of one scene under a moving sun: the kept tracer's scene gets update_sky per frame (build / sky / sky), and
    every picture is the one a scene created fresh for that frame under the same sky gives"""
    import json
    from PIL import Image
    from fspt_amd import scene_file as F
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    (root / "mesh" / "ball.obj").write_text(S.cube_sphere_obj(4))
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 4, "exposure": 1.2,
             "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6], "emittance": [0, 0, 0]},
                              {"path": "mesh/ball.obj", "scale": 0.4, "translate": [-0.4, 0, 0], "diffuse": [0.8, 0.3, 0.2], "emittance": [0, 0, 0], "normals": "smooth"}]}
    for f in range(3):
        (root / "scene" / f"day_{f}.json").write_text(json.dumps(scene))
    pattern = str(root / "scene" / "day_{frame}.json")
    skies = [dict(sun_dir=S.sun_direction(20.0 * f, 50.0 - 24.0 * f), width=SKY_W, height=SKY_H, turbidity=2.0) for f in range(3)]
    log = []
    kept = F.render_sequence(pattern, range(3), str(tmp_path / "kept" / "{frame}.png"), W, H, str(root), bvh="refit", samples=4,
                             sky=skies, on_frame=lambda f, how: log.append(how))
    assert log == ["build", "sky", "sky"]
    fresh = F.render_sequence(pattern, range(3), str(tmp_path / "fresh" / "{frame}.png"), W, H, str(root), bvh="sah", samples=4,
                              sky=lambda n: skies[n])
    by_hand = []
    for f in range(3):
        arrays, settings = F.load_scene_file(pattern.format(frame=f), str(root))
        d = dict(skies[f])
        rgbe, w, h = S.sky(d.pop("sun_dir"), d.pop("width"), d.pop("height"), **d)
        rgba, _ = F.render_frame(with_map(arrays, rgbe, w, h), settings, W, H, samples=4)
        out = str(tmp_path / f"hand_{f}.png")
        Image.fromarray(rgba[:, :, :3]).save(out)
        by_hand.append(out)
    pics = [[open(p, "rb").read() for p in run] for run in (kept, fresh, by_hand)]
    assert pics[0] == pics[1] == pics[2]
    assert len(set(pics[0])) == 3  # the light moved
    with pytest.raises(ValueError):
        F.render_sequence(pattern, range(1), str(tmp_path / "bad" / "{frame}.png"), W, H, str(root), bvh="refit", samples=4, sky=[dict(width=8)])


# ---- the Node host ---------------------------------------------------------------------------------------------------
def test_node_sky_matches_python(small_scene, tmp_path):
    import json
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("node") is None or not os.path.exists(os.path.join(root, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    a0 = small_scene
    sun2 = (-0.7, 0.2, 0.1)
    B = Scene(with_sky(a0, turbidity=3.0)); want = frame(B, n=6); B.close()
    rgbe2, w2, h2 = S.sky(sun2, 33, 17, view_samples=4, light_samples=2)
    B = Scene(with_map(a0, rgbe2, w2, h2)); want2 = frame(B, n=6); B.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins", "env"):
        getattr(a0, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=a0.atlas_res, atlasLayers=a0.atlas_layers, envW=a0.env_w, envH=a0.env_h, leafSize=a0.leaf_size, W=W, H=H, n=6, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]), sky=dict(sunDir=list(SUN), width=SKY_W, height=SKY_H, turbidity=3.0),
                sky2=dict(sunDir=list(sun2), width=33, height=17, viewSamples=4, lightSamples=2))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(root, "tests", "sky_node_check.js"), os.path.join(root, "fspt_amd", "js"), d], timeout=300)
    assert np.array_equal(np.fromfile(os.path.join(d, "out.bin"), np.uint32).reshape(H, W, 4), want)
    assert np.array_equal(np.fromfile(os.path.join(d, "sky.bin"), np.uint8), rgbe2)
    assert np.array_equal(np.fromfile(os.path.join(d, "bins.bin"), np.uint32), S.env_bins(rgbe2, w2, h2))
    assert np.array_equal(np.fromfile(os.path.join(d, "out2.bin"), np.uint32).reshape(H, W, 4), want2)
