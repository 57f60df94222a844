"""The pipelined present (include/fspt.h fspt_present) on the MI355X: call k returns the frame call k-1
enqueued - bit for bit oracle.draw of the oracle's accumulator at that tick - with its sample count; the accumulator ends
where n x tick() leaves it; draw arguments are forwarded; every other entry joins the pipeline and behaves as without
present, while ticks that run at once do not join; every scheduler / memory form gives the same frames; close() with a
present in flight returns;
and the Node host returns the Python host's bytes."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from fspt_amd import PathTracer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"small": (96, 64), "medium": (128, 96)}


def make_pt(arrays, W, H, cam, seed=7):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.seed(seed)
    return pt


class Oracle:
    """The oracle's accumulator, advanced tick by tick with the tracer's own xorshift state."""

    def __init__(self, arrays, W, H, cam):
        self.a, self.W, self.H, self.cam = arrays, W, H, cam
        self.acc = np.zeros((H, W, 4), np.float32)
        self.counters = O.OCounters()

    def ticks(self, pt, n):
        """n x pt.tick() and the same ticks in the oracle."""
        first, state = pt.pingpong, pt._rng.value
        for _ in range(n):
            pt.tick()
        O.render(self.a, self.W, self.H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, pt.num_bounces,
                 first, n, state, self.acc, counters=self.counters)


def run_oracle_frames(pt, orc, pattern, **kw):
    """Record pattern[k] ticks before present k; check every returned frame against oracle.draw of the accumulator the
    previous present saw.  Returns the frames."""
    W, H = pt.resolution
    seen, frames = [], []
    for k, n in enumerate(pattern):
        orc.ticks(pt, n)
        out = np.full((H, W, 4), 7, np.uint8)
        img, ticks = pt.present(out=out, **kw)
        if k == 0:
            assert img is None and ticks == 0 and (out == 7).all()  # nothing presented yet, out untouched
        else:
            assert ticks == seen[-1][0], (k, ticks)
            assert img is out and np.array_equal(img, O.draw(seen[-1][1], **kw)), k
            frames.append(img.copy())
        seen.append((pt.pingpong, orc.acc.copy()))
    return frames


@pytest.mark.parametrize("name", ["small", "medium"])
def test_frame_by_frame(small_scene, medium_scene, camera, name):
    arrays = {"small": small_scene, "medium": medium_scene}[name]
    W, H = SIZES[name]
    pt = make_pt(arrays, W, H, camera)
    orc = Oracle(arrays, W, H, camera)
    run_oracle_frames(pt, orc, [1] * 12)
    pt.sync()
    got = pt.readRadiance()
    assert np.array_equal(got, orc.acc)
    fresh = make_pt(arrays, W, H, camera)
    for _ in range(12):
        fresh.tick()
    assert np.array_equal(fresh.readRadiance(), got)
    fresh.close()
    assert pt.path_state_bytes()[0] > 0
    pt.close()


def test_uneven_batches(small_scene, camera):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    orc = Oracle(small_scene, W, H, camera)
    run_oracle_frames(pt, orc, [1, 3, 2, 5, 1])
    pt.sync()
    assert np.array_equal(pt.readRadiance(), orc.acc)
    pt.close()


@pytest.mark.parametrize("kw", [dict(exposure=1.7, saturation=0.6), dict(denoise=True, max_sigma=1.5), dict(scale=0.25)])
def test_draw_parameters_forwarded(small_scene, camera, kw):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    run_oracle_frames(pt, Oracle(small_scene, W, H, camera), [1] * 5, **kw)
    pt.close()


def test_view_change_inside_one_present(small_scene, camera):
    """Two runs of different views flushed by one present: both resolve in tick order."""
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    orc = Oracle(small_scene, W, H, camera)
    pt.present()
    for k in range(4):
        orc.ticks(pt, 2)
        pt.set_camera([p + 0.05 * (k + 1) for p in camera["P"]], camera["I"], camera["fov_scale"], camera["env_theta"],
                      camera["focal_depth"], camera["aperture"])
        orc.ticks(pt, 1)
        want = orc.acc.copy()
        pt.present()
        img, ticks = pt.present()  # (nothing recorded: draws the unchanged accumulator)
        assert ticks == pt.pingpong and np.array_equal(img, O.draw(want))
    pt.close()


JOINS = ["set_camera", "clear", "readRadiance", "draw", "denoise", "setRays", "render"]


def _join_step(pt, which, cam, rays):
    """One call that joins the pipeline; returns what it observed (None if nothing)."""
    if which == "set_camera":
        pt.set_camera([p + 0.1 for p in cam["P"]], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    elif which == "clear":
        pt.clear()
    elif which == "readRadiance":
        return pt.readRadiance()
    elif which == "draw":
        return pt.draw(1.2, 0.9)
    elif which == "denoise":
        pt.features(2, 3)
        return pt.denoise()
    elif which == "setRays":
        pt.setRays(*rays)
        pt.drawTracer(pt.pingpong, 17.0)
        pt.pingpong += 1
    elif which == "render":
        pt.render(3)
    return None


@pytest.mark.parametrize("which", JOINS)
def test_joins(small_scene, camera, which):
    """present, <call>, present, present against tick / <call> / tick without present: the call observes the same
    state, and the accumulator and the frames come out the same."""
    W, H = SIZES["small"]
    rng = np.random.default_rng(5)
    pos = np.zeros((H, W, 4), np.float32); pos[..., :3] = camera["P"]; pos[..., 3] = 1
    d = rng.normal(size=(H, W, 4)).astype(np.float32); d[..., 3] = 0
    d[..., :3] /= np.linalg.norm(d[..., :3], axis=-1, keepdims=True)
    rays = (pos, d)
    a, b = make_pt(small_scene, W, H, camera), make_pt(small_scene, W, H, camera)
    a.tick(); a.tick(); a.present(); a.tick(); a.present()
    b.tick(); b.tick(); b.tick()
    ga, gb = _join_step(a, which, camera, rays), _join_step(b, which, camera, rays)
    if ga is not None:
        assert np.array_equal(ga, gb)
    a.tick(); fa0 = a.present()
    if which != "set_camera":  # (set_camera is the host's own state: tick() records the new view, nothing joins)
        assert fa0 == (None, 0)  # the join drained the pipeline
    a.tick(); fa, ta = a.present()
    b.tick(); want = b.draw()
    b.tick()
    assert ta == b.pingpong - 1 and np.array_equal(fa, want)
    a.sync(); b.sync()
    assert np.array_equal(a.readRadiance(), b.readRadiance())
    a.close(); b.close()


def _one_lane_limit(arrays, W, H, camera):
    """(bytes of one one-tick lane, bytes of two) measured on a probe target."""
    p = make_pt(arrays, W, H, camera)
    p.tick(); p.sync()
    one = p.path_state_bytes()[0]
    p.tick(); p.present(); p.tick(); p.present(); p.tick(); p.present()
    two = p.path_state_bytes()[0]
    p.close()
    return one, two


FORMS = ["batch", "stream", "megakernel", "one_lane", "counters", "viewport", "shard", "bound"]


@pytest.mark.parametrize("form", FORMS)
def test_forms(small_scene, camera, form):
    """Every form gives the frames [tick(); draw()] gives on a twin target, and the same final accumulator."""
    W, H = SIZES["small"]
    keep = []

    def setup(pt):
        if form == "stream":
            pt.set_pipeline("stream")
        elif form == "megakernel":
            pt.set_pipeline("megakernel")
        elif form == "one_lane":
            pt.set_memory_limit(limit)
        elif form == "counters":
            pt.enable_counters(True)
        elif form == "viewport":
            pt.set_viewport(W // 2 + 8, H // 2)
        elif form == "shard":
            pt.set_shard(1, 3, 16)
        elif form == "bound":
            import torch
            acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            keep.append(acc)
            pt.bind_accumulator(acc.data_ptr(), keep=acc)

    one, two = _one_lane_limit(small_scene, W, H, camera)
    assert two == 2 * one  # path_state_bytes counts both lanes
    limit = one + 1024  # lane 0 fits, a second lane does not
    a, b = make_pt(small_scene, W, H, camera), make_pt(small_scene, W, H, camera)
    setup(a); setup(b)
    orc = Oracle(small_scene, W, H, camera) if form == "counters" else None
    n = 8
    for k in range(n):
        if orc is not None:
            orc.ticks(a, 1)
        else:
            a.tick()
        img, ticks = a.present()
        if k > 0:
            assert ticks == k and np.array_equal(img, want), k
        b.tick(); want = b.draw()
    a.sync(); b.sync()
    ra, rb = a.readRadiance(), b.readRadiance()
    assert np.array_equal(ra, rb)
    if form == "counters":
        assert np.array_equal(ra, orc.acc)
        assert a.counters() == orc.counters.as_dict()
    if form == "one_lane":
        assert a.path_state_bytes()[0] == one <= limit
    if form == "batch":
        assert a.path_state_bytes()[0] == two
    if form == "bound":
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(keep[0].cpu().numpy(), ra)
    a.close(); b.close()


def test_close_with_present_in_flight(small_scene, camera):
    """close() with a present in flight returns; the library's accounting of a new target of the same size starts from
    nothing and makes the same two lanes again (free-memory deltas of a shared device are not asserted on)."""
    W, H = 256, 192
    pt = make_pt(small_scene, W, H, camera)
    for _ in range(3):
        pt.tick(); pt.present()
    held = pt.path_state_bytes()[0]
    assert held > 0
    pt.tick(); pt.present()  # in flight
    pt.close()
    # the library's own accounting on a new target of the same size: it starts from nothing and makes the same lanes
    q = make_pt(small_scene, W, H, camera)
    assert q.path_state_bytes()[0] == 0
    for _ in range(3):
        q.tick(); q.present()
    assert q.path_state_bytes()[0] == held
    q.close()


@pytest.mark.parametrize("mode", ["undeferred", "batch1", "injected"])
def test_tick_flushes_do_not_join(small_scene, camera, mode):
    """A tick that runs at once - set_deferred(False), a batch size of 1, a tick from injected rays - is recorded work,
    not a join: [tick(); present()] still returns the previous frame, equal to [tick(); draw()] on a twin (and to the
    oracle where the ticks come from the camera)."""
    W, H = SIZES["small"]
    a, b = make_pt(small_scene, W, H, camera), make_pt(small_scene, W, H, camera)
    orc = None
    if mode == "undeferred":
        a.set_deferred(False); b.set_deferred(False)
        orc = Oracle(small_scene, W, H, camera)
    elif mode == "batch1":
        a.set_pipeline("wavefront", 1); b.set_pipeline("wavefront", 1)
        orc = Oracle(small_scene, W, H, camera)
    else:
        rng = np.random.default_rng(3)
        pos = np.zeros((H, W, 4), np.float32); pos[..., :3] = camera["P"]; pos[..., 3] = 1
        d = rng.normal(size=(H, W, 4)).astype(np.float32); d[..., 3] = 0
        d[..., :3] /= np.linalg.norm(d[..., :3], axis=-1, keepdims=True)
        a.setRays(pos, d); b.setRays(pos, d)
    for k in range(6):
        if mode == "injected":
            a.drawTracer(k, 100.0 + k); b.drawTracer(k, 100.0 + k)
            a.pingpong = b.pingpong = k + 1
        elif orc is not None:
            orc.ticks(a, 1)
            b.tick()
        img, ticks = a.present()
        if k == 0:
            assert img is None and ticks == 0
        else:
            assert ticks == k and np.array_equal(img, want), k
            if orc is not None:
                assert np.array_equal(img, O.draw(acc_prev)), k
        want = b.draw()
        if orc is not None:
            acc_prev = orc.acc.copy()
    a.close(); b.close()


def test_present_with_nothing_recorded(small_scene, camera):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    assert pt.present() == (None, 0)
    assert pt.present() == (None, 0)  # no tick has reached the accumulator: nothing to present
    orc = Oracle(small_scene, W, H, camera)
    orc.ticks(pt, 3)
    pt.present()
    for _ in range(3):
        img, ticks = pt.present()
        assert ticks == 3 and np.array_equal(img, O.draw(orc.acc))
    pt.close()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")),
                    reason="node or the built addon is missing")
def test_node_host(small_scene, camera, tmp_path):
    """fspt.js present() returns the Python host's frames and tick counts; during renderAsync it throws."""
    import base64
    from fspt_amd import scene as S
    W, H, seed, ticks = 96, 64, 13, 5
    env, ew, eh = S.synthetic_env(64, 32)
    job = {"props": S.bunny_props(), "objs": {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ},
           "env": {"rgbe_b64": base64.b64encode(env.tobytes()).decode(), "width": ew, "height": eh},
           "W": W, "H": H, "bounces": 4, "seed": seed, "ticks": ticks,
           "cam": dict(P=camera["P"], I=camera["I"], fov_scale=camera["fov_scale"], env_theta=camera["env_theta"], lens=camera["lens"])}
    jp, op = tmp_path / "job.json", tmp_path / "out.json"
    jp.write_text(json.dumps(job))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "present_node_check.js"), str(jp), str(op)], timeout=300)
    out = json.loads(op.read_text())
    pt = make_pt(small_scene, W, H, camera, seed)
    want = []
    for _ in range(ticks):
        pt.tick()
        img, n = pt.present(1.3, 0.9)
        want.append([n, base64.b64encode(img.tobytes()).decode() if n else None])
    pt.close()
    assert out["frames"] == want
    assert out["during"] == "render in flight" and out["after"] is None
