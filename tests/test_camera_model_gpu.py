"""The opt-in camera models (include/fspt.h fspt_target_set_camera_model) on the MI355X: the rays equal the
numpy restatement of the rule (tests/camera_model_ref.py) as uint32 words; a frame under a model equals the frame made of
set_rays(reference rays of tick k) + trace(k) tick by tick on every pipeline, in the recorded form and through
set_rays_device; the guides follow the camera; present, the setter's state, the refusals, shards, the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_model_ref as R
import oracle as O
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, TICKS = 96, 64, 8
CAM = dict(S.BUNNY_CAMERA)
MODELS = ("ortho", "fisheye", "equirect", "stereo")
MODEL_KW = {"ortho": {}, "fisheye": {"angle": 2.5}, "equirect": {}, "stereo": {"ipd": 0.1}}
PIPELINES = ("megakernel", "wavefront", "stream")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lens_of(aperture):
    return S.lens_features(CAM["focal_depth"], aperture)


def ref_rays(model, w, h, rand_base, aperture=0.0, sampler="reference", seed=0, tick=0):
    return R.rays(model, w, h, CAM["P"], CAM["I"], CAM["fov_scale"], lens_of(aperture), rand_base, sampler=sampler, seed=seed,
                  tick=tick, **MODEL_KW[model])


@pytest.fixture(scope="module")
def scenes(small_scene):
    # (not closed here: a tracer keeps its scene alive, and a tracer that a failing test left open must not outlive it)
    return {"small": Scene(small_scene), "textured": Scene(S.textured_test_scene())}


def make_pt(sc, model=None, pipeline="wavefront", w=W, h=H, aperture=None, seed=7):
    pt = PathTracer(sc, w, h, num_bounces=4)
    cam = dict(CAM)
    if aperture is not None:
        cam["aperture"] = aperture
    pt.set_camera(**cam)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if model is not None:
        pt.set_camera_model(model, **MODEL_KW[model])
    return pt


_tick_rays = {}


def tick_rays(model, seed=7):
    """The reference rays of ticks 0 .. TICKS - 1 of a W x H tracer seeded `seed` (BUNNY_CAMERA's aperture), with the
    randBase values of the trace calls: computed once per model, shared, never written."""
    if (model, seed) not in _tick_rays:
        rb = O.rand_base_stream(seed, 2 * TICKS)
        out = []
        for k in range(TICKS):
            pos, d = ref_rays(model, W, H, rb[2 * k], CAM["aperture"])
            pos.setflags(write=False); d.setflags(write=False)
            out.append((pos, d, rb[2 * k + 1]))
        _tick_rays[(model, seed)] = out
    return _tick_rays[(model, seed)]


# ---- 1. rays, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aperture", [0.0, 0.02])
@pytest.mark.parametrize("shape", [(96, 64), (33, 18), (1, 2)])
@pytest.mark.parametrize("sampler", ["reference", "sobol"])
@pytest.mark.parametrize("model", MODELS)
def test_rays_equal_the_rule(scenes, model, sampler, shape, aperture):
    w, h = shape
    pt = make_pt(scenes["small"], model, w=w, h=h, aperture=aperture)
    if sampler == "sobol":
        pt.set_sampler("sobol", 5)
    for rb in (1234.5, 77.25):
        pt.drawCamera(rb)
        pos, d = pt.readRays()
        want = ref_rays(model, w, h, rb, aperture, sampler, 5, 0)
        assert np.array_equal(bits(pos), bits(want[0])), (model, sampler, shape, "pos", int((bits(pos) != bits(want[0])).sum()))
        assert np.array_equal(bits(d), bits(want[1])), (model, sampler, shape, "dir", int((bits(d) != bits(want[1])).sum()))
    pt.close()


@pytest.mark.parametrize("model", MODELS)
def test_sobol_rays_follow_acc_ticks(scenes, model):
    """The Sobol sample index of materialised rays is acc_ticks: 0 on a fresh target, 3 after three ticks."""
    pt = make_pt(scenes["small"], model, w=33, h=18)
    pt.set_sampler("sobol", 9)
    got = []
    for ticks in (0, 3):
        if ticks:
            pt.render(ticks)
        pt.drawCamera(10.5)
        pos, d = pt.readRays()
        want = ref_rays(model, 33, 18, 10.5, CAM["aperture"], "sobol", 9, ticks)
        assert np.array_equal(bits(pos), bits(want[0])) and np.array_equal(bits(d), bits(want[1])), (model, ticks)
        got.append(d)
    assert not np.array_equal(got[0], got[1])
    pt.close()


@pytest.mark.parametrize("model", MODELS)
def test_viewport_rays(scenes, model):
    """A 17 x 10 viewport on the 33 x 18 target: inside it the rule (for the TARGET's size), outside it what was there."""
    w, h, vw, vh = 33, 18, 17, 10
    pt = make_pt(scenes["small"], model, w=w, h=h)
    mark = np.full((h, w, 4), -7.5, np.float32)
    pt.setRays(mark, mark * 2)
    pt.set_viewport(vw, vh)
    pt.drawCamera(99.0)
    pos, d = pt.readRays()
    want = ref_rays(model, w, h, 99.0, CAM["aperture"])
    inside = np.zeros((h, w), bool); inside[:vh, :vw] = True
    assert np.array_equal(bits(pos)[inside], bits(want[0])[inside]) and np.array_equal(bits(d)[inside], bits(want[1])[inside])
    assert np.array_equal(pos[~inside], mark[~inside]) and np.array_equal(d[~inside], (mark * 2)[~inside])
    pt.close()


# ---- 2. frames, bit for bit -------------------------------------------------------------------------------------------
def frame_from_reference_rays(sc, model, pipeline, device_rays=False):
    pt = make_pt(sc, None, pipeline)
    for k, (pos, d, rb_trace) in enumerate(tick_rays(model)):
        if device_rays:
            import torch
            tp, td = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(d)).cuda()
            torch.cuda.synchronize()
            pt.set_rays_device(tp, td)
        else:
            pt.setRays(pos, d)
        pt.drawTracer(k, rb_trace)
    img = pt.readRadiance()
    pt.close()
    return img


@pytest.mark.parametrize("scene", ["small", "textured"])
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("model", MODELS)
def test_frames_equal_traced_reference_rays(scenes, model, pipeline, scene):
    sc = scenes[scene]
    other = make_pt(sc, None, pipeline)  # a second target on the same scene, left at pinhole
    other.render(TICKS); before = other.readRadiance()
    want = frame_from_reference_rays(sc, model, pipeline)
    pt = make_pt(sc, model, pipeline)
    pt.render(TICKS)
    got = pt.readRadiance()
    assert np.array_equal(bits(got), bits(want)), (model, pipeline, scene, int((bits(got) != bits(want)).any(-1).sum()))
    assert not np.array_equal(got, before)
    # the recorded two-call form: camera + trace x 8, then one read
    pt.clear(); pt.seed(7)
    for _ in range(TICKS):
        pt.tick()
    assert np.array_equal(bits(pt.readRadiance()), bits(want)), (model, pipeline, scene, "recorded")
    pt.close()
    other.clear(); other.seed(7); other.render(TICKS)
    assert np.array_equal(bits(other.readRadiance()), bits(before))
    other.close()


@pytest.mark.parametrize("model,pipeline", [("equirect", p) for p in PIPELINES] + [(m, "wavefront") for m in MODELS if m != "equirect"])
def test_set_rays_device(scenes, model, pipeline):
    sc = scenes["small"]
    want = frame_from_reference_rays(sc, model, pipeline)
    got = frame_from_reference_rays(sc, model, pipeline, device_rays=True)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("model", MODELS)
def test_recorded_camera_rays_survive_a_render(scenes, model):
    """A render under a model writes the ray buffers tick by tick.  The rays of an earlier camera call that were already
    materialised are made again when somebody looks: read_rays and trace_test answer as they do under pinhole."""
    sc = scenes["small"]
    pt = make_pt(sc, model)
    pt.drawCamera(321.5)
    want = ref_rays(model, W, H, 321.5, CAM["aperture"])
    pos, d = pt.readRays()  # materialises: nothing is recorded any more
    assert np.array_equal(bits(pos), bits(want[0])) and np.array_equal(bits(d), bits(want[1]))
    pt.render(3)
    pos, d = pt.readRays()
    assert np.array_equal(bits(pos), bits(want[0])) and np.array_equal(bits(d), bits(want[1])), model
    pt.render(2)
    pt.clear(); pt.drawTracerTest(0)
    b = make_pt(sc, None)
    b.setRays(*want); b.drawTracerTest(0)
    assert np.array_equal(bits(pt.readRadiance()), bits(b.readRadiance()))
    pt.close(); b.close()


@pytest.mark.parametrize("device_rays", [False, True])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_injected_rays_do_not_survive_a_render(scenes, pipeline, device_rays):
    """Injected rays are gone once a render under a model has written the buffers: the next trace is refused (-6) instead of
    tracing the model's rays, and works again after the caller injects anew - with the frame explicit calls give."""
    sc = scenes["small"]
    pos, d, rb = tick_rays("fisheye")[0]

    def inject(pt):
        if device_rays:
            import torch
            tp, td = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(d)).cuda()
            torch.cuda.synchronize()
            pt.set_rays_device(tp, td)
        else:
            pt.setRays(pos, d)

    a, b = make_pt(sc, "equirect", pipeline), make_pt(sc, "equirect", pipeline)
    inject(a); a.drawTracer(0, rb)
    a.pingpong = 1; a.render(2)
    with pytest.raises(FsptError) as e:
        a.drawTracer(3, rb)
    assert e.value.code == -6
    with pytest.raises(FsptError):
        a.readRays()
    inject(a); a.drawTracer(3, rb)
    b.setRays(pos, d); b.drawTracer(0, rb)
    b.pingpong = 1; b.render(2)
    b.setRays(pos, d); b.drawTracer(3, rb)
    assert np.array_equal(bits(a.readRadiance()), bits(b.readRadiance()))
    a.close(); b.close()


def test_set_rays_device_checks_its_arguments(scenes):
    import torch
    pt = make_pt(scenes["small"], None)
    ok = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError):
        pt.set_rays_device(np.zeros(W * H * 4, np.float32), ok)
    with pytest.raises(ValueError):
        pt.set_rays_device(ok.cpu(), ok)
    with pytest.raises(ValueError):
        pt.set_rays_device(ok[:-4], ok)
    with pytest.raises(ValueError):
        pt.set_rays_device(ok.double(), ok)
    pt.close()


# ---- 3. guides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_guides_follow_the_camera(scenes, model):
    sc = scenes["small"]
    pt = make_pt(sc, model)
    pt.features(samples=1, seed=11)
    feat = pt.readFeatures()
    pos, d = ref_rays(model, W, H, O.rand_base_stream(11, 1)[0], CAM["aperture"])
    rays = np.concatenate([pos[..., :3].reshape(-1, 3), d[..., :3].reshape(-1, 3)], 1).astype(np.float32)
    t, idx = sc.intersect(rays)[:2]
    assert np.array_equal(bits(feat[..., 3]).reshape(-1), bits(t))
    assert np.array_equal(feat[..., 7].reshape(-1), (np.asarray(idx) >= 0).astype(np.float32))
    hits = int((np.asarray(idx) >= 0).sum())
    assert hits > 0 and (model == "ortho" or hits < idx.size)  # (hits and misses; the ortho frame lies inside the scene's outline)
    pt.close()


# ---- 4. present ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["wavefront", "stream", "megakernel"])
def test_present_under_a_model(scenes, pipeline):
    """present under a model returns draw()'s frames of the same ticks rendered serially, one call late.  A setter joins: the
    ticks of the frame in flight are in the accumulator afterwards, the pipeline is drained (the next present has nothing to
    show) and goes on as before."""
    sc = scenes["small"]
    a, b = make_pt(sc, "equirect", pipeline), make_pt(sc, "equirect", pipeline)
    a.tick(); a.tick()
    assert a.present() == (None, 0)
    b.tick(); b.tick(); f2 = b.draw()
    a.tick(); b.tick()
    img, n = a.present()
    assert n == 2 and np.array_equal(img, f2)
    f3 = b.draw()
    a.set_camera_model("equirect"); b.set_camera_model("equirect")  # joins with the 3-tick frame in flight
    assert np.array_equal(bits(a.readRadiance()), bits(b.readRadiance()))
    a.tick(); b.tick()
    assert a.present() == (None, 0)
    f4 = b.draw()
    a.tick(); b.tick()
    img, n = a.present()
    assert n == 4 and np.array_equal(img, f4) and not np.array_equal(f4, f3)
    assert np.array_equal(bits(a.readRadiance()), bits(b.readRadiance()))
    a.close(); b.close()


# ---- 5. state -----------------------------------------------------------------------------------------------------------
def test_setter_flushes_under_the_old_model_and_does_not_clear(scenes):
    sc = scenes["small"]
    a = make_pt(sc, None)
    for _ in range(4):
        a.tick()  # recorded under pinhole
    a.set_camera_model("equirect")
    for _ in range(4):
        a.tick()
    b = make_pt(sc, None)
    b.render(4)
    four = b.readRadiance()
    b.set_camera_model("equirect")
    assert np.array_equal(bits(b.readRadiance()), bits(four))  # not cleared
    b.render(4)
    want = b.readRadiance()
    assert np.array_equal(bits(a.readRadiance()), bits(want))
    assert not np.array_equal(want, four)
    a.close(); b.close()


def test_get_returns_what_was_set(scenes):
    pt = make_pt(scenes["small"], None)
    assert pt.camera_model == {"model": "pinhole", "angle": float(np.float32(np.pi)), "ipd": float(np.float32(0.064))}
    pt.set_camera_model("fisheye", angle=2.5)
    assert pt.camera_model["model"] == "fisheye" and pt.camera_model["angle"] == 2.5
    pt.set_camera_model("stereo", ipd=0.25)
    assert pt.camera_model["model"] == "stereo" and pt.camera_model["ipd"] == 0.25
    pt.set_camera_model("fisheye", angle=float(np.float32(2 * np.pi)))  # the closed end of the range
    pt.set_camera_model(None)
    assert pt.camera_model["model"] == "pinhole"
    pt.close()


BAD = [(5, np.pi, 0.064), (-1, np.pi, 0.064), (2, 0.0, 0.064), (2, -1.0, 0.064), (2, 6.3, 0.064), (2, np.nan, 0.064),
       (2, np.inf, 0.064), (4, np.pi, -0.01), (4, np.pi, np.nan), (4, np.pi, np.inf)]


@pytest.mark.parametrize("bad", BAD)
def test_invalid_arguments_change_nothing(scenes, bad):
    pt = make_pt(scenes["small"], "fisheye")
    pt.render(2); first = pt.readRadiance()
    was = pt.camera_model
    prm = L.CameraModelParams(int(bad[0]), float(bad[1]), float(bad[2]))
    assert L.lib().fspt_target_set_camera_model(pt._t, C.byref(prm)) == -1
    assert L.lib().fspt_last_error()
    assert pt.camera_model == was
    pt.clear(); pt.seed(7); pt.render(2)
    assert np.array_equal(bits(pt.readRadiance()), bits(first))
    pt.close()


def test_stereo_needs_an_even_height(scenes):
    pt = make_pt(scenes["small"], "equirect", w=33, h=17)
    pt.render(2); first = pt.readRadiance()
    with pytest.raises(FsptError) as e:
        pt.set_camera_model("stereo")
    assert e.value.code == -1 and "even" in str(e.value)
    assert pt.camera_model["model"] == "equirect"
    pt.clear(); pt.seed(7); pt.render(2)
    assert np.array_equal(bits(pt.readRadiance()), bits(first))
    pt.close()


def test_adaptive_and_temporal_are_refused_under_a_model(scenes):
    pt = make_pt(scenes["small"], "fisheye")
    pt.render(2)
    with pytest.raises(FsptError) as e:
        pt.render_adaptive(1e-3, max_ticks=64, min_ticks=64, round_ticks=32)
    assert e.value.code == -6 and "fisheye" in str(e.value)
    with pytest.raises(FsptError) as e:
        pt.temporal_accumulate()
    assert e.value.code == -6 and "fisheye" in str(e.value)
    pt.set_camera_model(None)
    assert pt.render_adaptive(1e-3, max_ticks=64, min_ticks=64, round_ticks=32) == 64
    assert pt.temporal_accumulate().shape == (H, W, 4)
    pt.close()


def test_trace_test_uses_the_model(scenes):
    """drawTracerTest (the traversal-step heat map) walks the model's rays: the same picture from the injected reference rays."""
    sc = scenes["small"]
    a, b = make_pt(sc, "equirect"), make_pt(sc, None)
    a.drawCamera(42.0); a.drawTracerTest(0)
    pos, d = ref_rays("equirect", W, H, 42.0, CAM["aperture"])
    b.setRays(pos, d); b.drawTracerTest(0)
    got = a.readRadiance()
    assert np.array_equal(bits(got), bits(b.readRadiance())) and got[..., 0].max() > 0
    a.close(); b.close()


def test_camera_model_time_hook(scenes):
    """fspt_camera_model_time (the measurement hook): refused under pinhole; under a model it reports a time and a recorded
    camera call's rays are made again afterwards."""
    pt = make_pt(scenes["small"], None, w=33, h=18)
    ms = C.c_float(-1.0)
    cp = pt._camera_params()
    assert L.lib().fspt_camera_model_time(pt._t, C.byref(cp), 4, C.byref(ms)) == -6
    assert L.lib().fspt_camera_model_time(pt._t, C.byref(cp), 0, C.byref(ms)) == -1
    pt.set_camera_model("stereo", **MODEL_KW["stereo"])
    pt.drawCamera(5.5)
    assert L.lib().fspt_camera_model_time(pt._t, C.byref(cp), 4, C.byref(ms)) == 0 and ms.value > 0
    pos, d = pt.readRays()
    want = ref_rays("stereo", 33, 18, 5.5, CAM["aperture"])
    assert np.array_equal(bits(pos), bits(want[0])) and np.array_equal(bits(d), bits(want[1]))
    assert L.lib().fspt_camera_model_time(pt._t, C.byref(cp), 2, C.byref(ms)) == 0  # (materialised rays: made again too)
    pos, d = pt.readRays()
    assert np.array_equal(bits(pos), bits(want[0])) and np.array_equal(bits(d), bits(want[1]))
    pt.close()


# ---- 6. shards ------------------------------------------------------------------------------------------------------------
def test_shards_sum_to_the_frame(scenes):
    sc = scenes["small"]
    whole = make_pt(sc, "equirect"); whole.render(TICKS); want = whole.readRadiance(); whole.close()
    parts = []
    for s in range(2):
        pt = make_pt(sc, "equirect")
        pt.set_shard(s, 2)
        pt.render(TICKS)
        parts.append(pt.readRadiance())
        pt.close()
    assert (parts[0][..., :3] != 0).any() and (parts[1][..., :3] != 0).any()
    assert not ((parts[0] != 0) & (parts[1] != 0)).any()  # a pixel belongs to one shard
    assert np.array_equal(bits(parts[0] + parts[1]), bits(want))


def test_multi_tracer_equals_the_single_target(small_scene, scenes):
    one = make_pt(scenes["small"], "stereo"); one.render(TICKS); want = one.readRadiance(); one.close()
    mp = MultiPathTracer(small_scene, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    mp.set_camera_model("stereo", **MODEL_KW["stereo"])
    mp.render(TICKS)
    got = mp.readRadiance()
    mp.close()
    assert np.array_equal(bits(got), bits(want))


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------
def test_cli_camera_flag(tmp_path):
    from PIL import Image
    w, h, spp = 64, 32, 4
    out = {}
    for name in ("equirect", "pinhole"):
        out[name] = str(tmp_path / (name + ".png"))
        subprocess.check_call([sys.executable, "-m", "fspt_amd.render", "--camera", name, "--width", str(w), "--height", str(h),
                               "--spp", str(spp), "--bounces", "4", "--mesh-n", "8", "--out", out[name]], cwd=ROOT, timeout=300)
    pt = PathTracer(S.bunny_scene(n=8), w, h, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.set_camera_model("equirect")
    pt.render(spp)
    rgba = pt.draw(1.0, 1.0, False)
    pt.close(); pt.scene.close()
    direct = str(tmp_path / "direct.png")
    Image.fromarray(rgba[::-1, :, :3]).save(direct)
    assert open(out["equirect"], "rb").read() == open(direct, "rb").read()
    assert open(out["equirect"], "rb").read() != open(out["pinhole"], "rb").read()
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--camera", "stereo", "--width", "16", "--height", "9", "--spp", "1",
                        "--mesh-n", "8", "--out", str(tmp_path / "odd.png")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "even target height" in r.stderr
