"""GPU part transforms (fspt_scene_set_pose / fspt_scene_update_transforms) on the MI355X.  No tolerance but
in the last test: k_pose_transform's output equals tests/pose_ref.py word for word, and a scene posed by matrices is
indistinguishable from a twin that was handed pose_ref's arrays through update_geometry - hits, step and leaf counts,
two-level nodes, SAH cost, light table, frames of every pipeline, temporal reprojection."""
import json
import os

import numpy as np
import pytest

import lights_ref as LR
import oracle as O
import pose_ref as PR
from conftest import random_rays
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene, device_memory
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 64, 48, 4
SCENES = ("one", "small", "gpu", "textured", "lights")
SETS = ("identity", "rotate", "scale", "shear", "mirror")
N_SYNTH = 5


def one_triangle_scene():
    env, w, h = S.synthetic_env(64, 32)
    prop = {"path": "t.obj", "scale": 1.5, "translate": [0.0, -0.4, 0.0], "diffuse": [0.8, 0.6, 0.3], "emittance": [0, 0, 0]}
    return S.build_scene([prop], {"t.obj": "v -1 0 0.5\nv 1 0 0.5\nv 0 1 -0.5\nf 1 2 3\n"}, env=env, env_w=w, env_h=h)


@pytest.fixture(scope="module")
def scenes(small_scene):
    return {"one": one_triangle_scene(), "small": small_scene,
            "gpu": S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu", keep_order=True),
            "textured": S.textured_test_scene(keep_order=True), "lights": LR.scene_e1()}


def synthetic_parts(T):
    """ids that interleave inside leaves; part 3 stays empty"""
    part = ((np.arange(T, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(N_SYNTH)
    part[part == 3] = 0
    return part.astype(np.uint32)


def part_choices(arrays):
    """[(name, part, n_parts)]"""
    out = [("synthetic", synthetic_parts(arrays.n_tris), N_SYNTH)]
    if "tri_part" in arrays.meta:
        out.append(("props", arrays.meta["tri_part"], int(arrays.meta["tri_part"].max()) + 1))
    return out


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return S._rotation_matrix(axis, angle)


def transform_set(name, n_parts):
    out = np.zeros((n_parts, 3, 4), np.float64)
    for p in range(n_parts):
        if name == "identity":
            A, t = np.eye(3), np.zeros(3)
        elif name == "rotate":
            A, t = rot([1 + p, 2, -0.5 * p], 0.3 + 0.45 * p), np.array([0.05 * p, -0.03, 0.02 * p])
        elif name == "scale":
            A, t = 0.37 * np.eye(3), np.zeros(3)
        elif name == "shear":
            A, t = np.diag([1.3, 0.6, 0.9 + 0.05 * p]) + np.array([[0, 0.4, 0], [0, 0, 0], [0.1 * p, 0, 0]]), np.array([0.0, 0.1, 0.0])
        elif name == "mirror":
            A, t = rot([0, 1, 0.2 * p], 0.2) @ np.diag([1.0, -1.0, 1.0]), np.array([0.0, -0.2, 0.0])
        out[p, :, :3], out[p, :, 3] = A, t
    return out.reshape(n_parts, 12).astype(np.float32)


def ray_set(arrays):
    cam = O.camera(W, H, CAM["P"], CAM["I"], CAM["fov_scale"], S.lens_features(CAM["focal_depth"], CAM["aperture"]), 3.0)
    camr = np.concatenate([cam[0][..., :3].reshape(-1, 3), cam[1][..., :3].reshape(-1, 3)], 1).astype(np.float32)
    return np.concatenate([camr, random_rays(arrays, 2048, 1)]).astype(np.float32)


def make_pt(sc, pipeline="wavefront", lights=False, seed=7, w=W, h=H):
    pt = PathTracer(sc, w, h, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if lights:
        pt.set_lights("emitters", 0.5)
    return pt


def again(pt, n=TICKS, seed=7):
    pt.clear(); pt.seed(seed); pt.render(n)
    return pt.readRadiance()


def frame(sc, n=TICKS, **kw):
    pt = make_pt(sc, **kw)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same_hits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- the kernel, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_kernel_equals_the_reference(scenes, name):
    arrays = scenes[name]
    sc = Scene(arrays)
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    try:
        for pname, part, n_parts in part_choices(arrays):
            sc.set_pose(part, n_parts=n_parts)
            for sname in SETS:
                xf = transform_set(sname, n_parts)
                sc.update_transforms(xf)
                got_t, got_n = sc.read_pose()
                want_t, want_n = PR.pose(part, rest_t, rest_n, xf)
                assert np.array_equal(bits(got_t), bits(want_t)), (pname, sname, int((bits(got_t) != bits(want_t)).sum()))
                assert np.array_equal(bits(got_n), bits(want_n)), (pname, sname, int((bits(got_n) != bits(want_n)).sum()))
                if sname == "identity":  # value for value (only the sign of a zero may differ)
                    assert (got_t == rest_t).all() and (got_n == rest_n).all()
                else:
                    assert not np.array_equal(got_t, rest_t)
            ms = sc.last_pose_ms()
            assert ms["launches"] >= 3 and ms["transform_ms"] > 0 and ms["refit_ms"] > 0
        # a pose without rest normals poses the vertices alone
        part, n_parts = part_choices(arrays)[0][1:]
        sc.set_pose(part, arrays.tri, None, n_parts=n_parts)
        xf = transform_set("rotate", n_parts)
        sc.update_transforms(xf)
        got_t, got_n = sc.read_pose()
        assert got_n is None and np.array_equal(bits(got_t), bits(PR.pose(part, rest_t, None, xf)[0]))
    finally:
        sc.close()


# ---- the scene, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_posed_scene_equals_updated_twin(scenes, name):
    arrays = scenes[name]
    pname, part, n_parts = part_choices(arrays)[-1]
    A, B = Scene(arrays), Scene(arrays)
    A.set_pose(part, n_parts=n_parts)
    lights = name == "lights"
    tracers = [(make_pt(A, pipeline=p, lights=l), make_pt(B, pipeline=p, lights=l))
               for p in ("megakernel", "wavefront", "stream") for l in ((False, True) if lights else (False,))]
    rays = ray_set(arrays)
    try:
        for sname in SETS:
            xf = transform_set(sname, n_parts)
            tri, norm = PR.pose(part, arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27), xf)
            A.update_transforms(xf)
            B.update_geometry(tri, norm)
            ha, hb = A.intersect(rays), B.intersect(rays)
            for k, what in enumerate(("t", "index", "steps", "leaves")):
                assert np.array_equal(bits(ha[k]), bits(hb[k])), (sname, what)
            assert A.two_level_nodes() == B.two_level_nodes()
            if B.two_level_nodes()[0]:
                assert same_hits(A.intersect(rays, two_level=True), B.intersect(rays, two_level=True))
            assert A.sah_cost() == B.sah_cost()
            if lights:
                ta, tb = A.light_table(), B.light_table()
                for key in tb:
                    assert np.array_equal(bits(ta[key]), bits(tb[key])), (sname, key)
            for pa, pb in tracers:
                fa, fb = again(pa), again(pb)
                assert np.array_equal(fa, fb), (sname, int((fa != fb).any(-1).sum()))
                assert np.isfinite(fa).all()
        if name != "one":
            assert fa[..., :3].max() > 0
    finally:
        for pa, pb in tracers:
            pa.close(); pb.close()
        A.close(); B.close()


def test_pose_without_rest_normals_leaves_the_normals_alone(scenes):
    arrays = scenes["textured"]
    _, part, n_parts = part_choices(arrays)[-1]
    xf = transform_set("rotate", n_parts)
    A, B = Scene(arrays), Scene(arrays)
    A.set_pose(part, arrays.tri, None, n_parts=n_parts)
    A.update_transforms(xf)
    B.update_geometry(PR.pose(part, arrays.tri.reshape(-1, 9), None, xf)[0])
    assert np.array_equal(frame(A), frame(B))
    assert np.array_equal(A.read_appearance("hitrec"), B.read_appearance("hitrec"))
    A.close(); B.close()


# ---- rebuild ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "textured"))
def test_rebuild_permutes_the_pose(scenes, name):
    arrays = scenes[name]
    _, part, n_parts = part_choices(arrays)[0]
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    x1, x2 = transform_set("shear", n_parts), transform_set("rotate", n_parts)
    t1, n1 = PR.pose(part, rest_t, rest_n, x1)
    A, B = Scene(arrays), Scene(arrays)
    A.set_pose(part, n_parts=n_parts)
    order = A.rebuild_geometry(t1, n1).astype(np.int64)
    assert np.array_equal(B.rebuild_geometry(t1, n1), order)
    assert not np.array_equal(order, np.arange(arrays.n_tris))
    with pytest.raises(FsptError) as ei:
        A.read_pose()  # the staging array is the rebuild's
    assert ei.value.code == -6
    A.update_transforms(x2)  # nothing from the caller: the scene permuted part ids and rest mesh
    t2, n2 = PR.pose(part[order], rest_t[order], rest_n[order], x2)
    B.update_geometry(t2, n2)
    got_t, got_n = A.read_pose()
    assert np.array_equal(bits(got_t), bits(t2)) and np.array_equal(bits(got_n), bits(n2))
    rays = ray_set(arrays)
    assert same_hits(A.intersect(rays), B.intersect(rays))
    assert A.sah_cost() == B.sah_cost() and A.two_level_nodes() == B.two_level_nodes()
    for pipeline in ("megakernel", "wavefront", "stream"):
        assert np.array_equal(frame(A, pipeline=pipeline), frame(B, pipeline=pipeline))
    with pytest.raises(ValueError):
        A.set_pose(part)  # the default rest mesh is gone with the order
    A.close(); B.close()


# ---- ordering --------------------------------------------------------------------------------------------------------
def test_recorded_ticks_run_before_the_transforms(scenes):
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    xf = transform_set("rotate", n_parts)
    out = []
    for sync_first in (False, True):
        sc = Scene(arrays); sc.set_pose(part, n_parts=n_parts)
        pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        pt.update_transforms(xf)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance())
        pt.close(); sc.close()
    assert np.array_equal(out[0], out[1])
    sc = Scene(arrays); pt = make_pt(sc)
    for _ in range(6):
        pt.tick()
    assert not np.array_equal(pt.readRadiance(), out[0])  # neither all-old nor all-new
    pt.close(); sc.close()


def test_present_around_the_transforms(scenes):
    """A frame in flight when the call arrives is presented once, unchanged; the yardstick is a second tracer that draws
    (blocking) where the first presents, on a twin that gets update_geometry."""
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    xf = transform_set("rotate", n_parts)
    tri, norm = PR.pose(part, arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27), xf)
    sc = Scene(arrays); sc.set_pose(part, n_parts=n_parts); pt = make_pt(sc)
    ref = Scene(arrays); pr = make_pt(ref)

    def ticks(n):
        for _ in range(n):
            pt.tick(); pr.tick()

    ticks(2)
    img, n = pt.present()
    assert img is None and n == 0
    pre = pr.draw()
    pt.update_transforms(xf); pr.update_geometry(tri, norm)
    ticks(2)
    img, n = pt.present()
    assert n == 2 and np.array_equal(img, pre)  # the pre-update frame, once
    post = pr.draw()
    assert not np.array_equal(post, pre)
    ticks(1)
    img, n = pt.present()
    assert n == 4 and np.array_equal(img, post)
    post = pr.draw()
    img, n = pt.present()
    assert n == 5 and np.array_equal(img, post)
    assert np.array_equal(pt.readRadiance(), pr.readRadiance())
    pt.close(); pr.close(); sc.close(); ref.close()


def test_two_targets_both_see_the_new_pose(scenes):
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    xf = transform_set("mirror", n_parts)
    tri, norm = PR.pose(part, arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27), xf)
    sc = Scene(arrays); sc.set_pose(part, n_parts=n_parts)
    p1, p2 = make_pt(sc), make_pt(sc, pipeline="stream", w=48, h=32)
    first = (again(p1), again(p2))
    p1.tick(); p2.tick()  # recorded on both when the call arrives
    p1.update_transforms(xf)
    B = Scene(arrays); B.update_geometry(tri, norm)
    q1, q2 = make_pt(B), make_pt(B, pipeline="stream", w=48, h=32)
    for a, b in ((p1, q1), (p2, q2)):
        assert np.array_equal(again(a), again(b))
    sc.update_transforms(transform_set("identity", n_parts))  # back to the rest pose
    for p, want in zip((p1, p2), first):
        assert np.array_equal(again(p), want)
    for p in (p1, p2, q1, q2):
        p.close()
    sc.close(); B.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_unchanged(scenes):
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    sc = Scene(arrays)
    pt = make_pt(sc)
    f0 = again(pt)
    rays = ray_set(arrays)
    h0 = sc.intersect(rays)
    good = transform_set("rotate", n_parts)
    with pytest.raises(FsptError) as ei:
        sc.update_transforms(good)  # no pose
    assert ei.value.code == -6
    with pytest.raises(FsptError) as ei:
        sc.set_pose(part, n_parts=3)  # ids up to 4
    assert ei.value.code == -1
    with pytest.raises(FsptError) as ei:
        sc.update_transforms(good)  # still no pose
    assert ei.value.code == -6
    sc.set_pose(part, n_parts=n_parts)
    nan = good.copy(); nan[2, 5] = np.nan
    singular = good.copy(); singular[1, 0:3] = 0.0
    overflow = good.copy(); overflow[:] = np.float32([3e38, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])  # finite, regular; 3e38 x 2 is not
    assert np.abs(arrays.tri.reshape(-1, 3)[:, 0]).max() > 1.5
    for what, xf in (("n_parts", good[:-1]), ("nan", nan), ("singular", singular), ("overflow", overflow)):
        with pytest.raises(FsptError) as ei:
            sc.update_transforms(xf)
        assert ei.value.code == -1, what
        if what in ("nan", "singular"):
            assert f"part {2 if what == 'nan' else 1}" in str(ei.value)
        assert same_hits(sc.intersect(rays), h0), what
        assert np.array_equal(again(pt), f0), what
    with pytest.raises(ValueError):
        sc.update_transforms(good.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        sc.set_pose(part[:-1])
    # read_pose hands out only a frame the scene took: a refusal on the host leaves the accepted frame readable, one by
    # the refit's check (the kernel has overwritten the staging array by then) leaves none
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    first = transform_set("shear", n_parts)
    sc.update_transforms(first)
    want = PR.pose(part, rest_t, rest_n, first)
    f1, h1 = again(pt), sc.intersect(rays)
    for what, xf in (("n_parts", good[:-1]), ("nan", nan), ("singular", singular)):
        with pytest.raises(FsptError) as ei:
            sc.update_transforms(xf)
        assert ei.value.code == -1, what
        got = sc.read_pose()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), what
    with pytest.raises(FsptError) as ei:
        sc.update_transforms(overflow)
    assert ei.value.code == -1
    with pytest.raises(FsptError) as ei:
        sc.read_pose()
    assert ei.value.code == -6 and "fspt_scene_read_pose" in str(ei.value)
    assert same_hits(sc.intersect(rays), h1) and np.array_equal(again(pt), f1)  # the scene keeps the frame it took
    sc.update_transforms(good)  # and the pose still works
    want = PR.pose(part, rest_t, rest_n, good)
    got = sc.read_pose()
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not np.array_equal(again(pt), f0)
    pt.close(); sc.close()


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_pose_memory_is_taken_by_set_pose_and_returned():
    arrays = S.bunny_scene(n=76, env_size=(64, 32), bvh="gpu", keep_order=True)
    part = arrays.meta["tri_part"]
    pose_bytes = arrays.n_tris * (4 + 36 + 108)
    assert pose_bytes > (8 << 20)
    slack = 4 << 20  # two allocations, each rounded to the allocator's granularity of up to 2 MiB
    sc = Scene(arrays)
    sc.update_geometry(arrays.tri, arrays.norm)  # the refit's own tables and staging array exist from here on
    free0 = device_memory(0)[0]
    sc.update_geometry(arrays.tri, arrays.norm)
    assert abs(device_memory(0)[0] - free0) <= slack  # a scene that sets no pose takes nothing more
    sc.set_pose(part, arrays.tri, arrays.norm)
    free1 = device_memory(0)[0]
    assert free0 - free1 >= pose_bytes - slack and free0 - free1 <= pose_bytes + slack
    sc.update_transforms(transform_set("rotate", 3))
    assert abs(device_memory(0)[0] - free1) <= slack  # the posed arrays go to the staging array the refit owns
    sc.set_pose(None)
    assert abs(device_memory(0)[0] - free0) <= slack
    sc.close()


# ---- multi -----------------------------------------------------------------------------------------------------------
def test_multi_update_transforms(scenes):
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    xf = transform_set("rotate", n_parts)
    mp = MultiPathTracer(arrays, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    mp.set_pose(part)
    mp.update_transforms(xf)
    mp.render(TICKS)
    got = mp.readRadiance()
    mp.close()
    B = Scene(arrays)
    B.update_geometry(*PR.pose(part, arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27), xf))
    assert np.array_equal(got, frame(B))
    B.close()


# ---- temporal --------------------------------------------------------------------------------------------------------
def test_temporal_reprojection_follows_the_pose(scenes):
    arrays = scenes["small"]
    _, part, n_parts = part_choices(arrays)[0]
    xf = transform_set("rotate", n_parts)
    tri, norm = PR.pose(part, arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27), xf)
    out = []
    for posed in (True, False):
        sc = Scene(arrays)
        pt = make_pt(sc)
        pt.render(TICKS)
        pt.temporal_accumulate()
        sc.motion_begin()
        if posed:
            sc.set_pose(part, n_parts=n_parts); sc.update_transforms(xf)
        else:
            sc.update_geometry(tri, norm)
        pt.clear(); pt.seed(9); pt.render(TICKS)
        out.append((pt.temporal_accumulate(), pt.temporal_gbuffer()))
        pt.close(); sc.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))
    for a, b in zip(out[0][1], out[1][1]):
        assert np.array_equal(bits(a), bits(b))
    assert np.abs(out[0][1][1]).max() > 0  # something moved on the screen


def _write_frames(tmp_path, n_frames, recolour_from=None):
    """three hand-written frames: a glowing ball turns, grows and moves over a floor, under world transforms that change too"""
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    (root / "mesh" / "ball.obj").write_text("mtllib ball.mtl\nusemtl glow\n" + S.cube_sphere_obj(4))
    (root / "mesh" / "ball.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")
    for f in range(n_frames):
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 64, "exposure": 1.2,
                 "worldTransforms": [{"rotate": [{"axis": [0, 1, 0], "angle": 0.05 * f}]}, {"translate": [0.0, 0.02 * f, 0.0]}],
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "emittance": [0, 0, 0],
                                   "diffuse": [0.7, 0.7, 0.6] if recolour_from is None or f < recolour_from else [0.2, 0.5, 0.7]}],
                 "animated_props": [{"path": "mesh/ball.obj", "scale": 0.4 + 0.05 * f, "translate": [-0.4 + 0.4 * f, 0.05 * f, 0.0],
                                     "rotate": [{"axis": [0, 1, 0], "angle": 0.3 * f}, {"axis": [1, 0, 0], "angle": 0.2 * f}],
                                     "diffuse": [0.8, 0.3, 0.2], "emittance": [3, 3, 3], "normals": "smooth"}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def test_render_sequence_pose(tmp_path):
    """The pose path against the parse path at 64 spp: the same noise (same seeds), matrices in float32 instead of float64.
    Bound: 2 / 255 mean absolute difference of the 8-bit pictures (the issue's)."""
    from PIL import Image
    from fspt_amd import scene_file as F
    pattern, root = _write_frames(tmp_path, 3)
    log = []
    got = F.render_sequence(pattern, range(3), str(tmp_path / "pose" / "{frame}.png"), W, H, root, bvh="refit", pose=True,
                            on_frame=lambda f, how: log.append(how))
    assert log == ["build", "pose", "pose"] and len(got) == 3 and all(os.path.exists(p) for p in got)
    log2 = []
    want = F.render_sequence(pattern, range(3), str(tmp_path / "parse" / "{frame}.png"), W, H, root, bvh="refit",
                             on_frame=lambda f, how: log2.append(how))
    # (the ball's OBJ has no `vt`: the loader derives its uvs from the moved positions, so the parse path may report "appearance")
    assert log2[0] == "build" and "build" not in log2[1:]
    assert open(got[0], "rb").read() == open(want[0], "rb").read()
    a, b = (np.asarray(Image.open(p[1]), np.float64) for p in (got, want))
    mad = np.abs(a - b).mean()
    print(f"middle frame: mean absolute difference {mad:.4f} / 255 between the pose path and the parse path")
    assert mad <= 2.0
    assert a.max() > 0
    assert np.abs(a - np.asarray(Image.open(got[0]), np.float64)).mean() > 2.0  # the frames do differ
    with pytest.raises(ValueError):
        F.render_sequence(pattern, range(1), str(tmp_path / "x" / "{frame}.png"), W, H, root, bvh="sah", pose=True)
    # a frame that changes a material takes the parse path; the pose is re-set from it and the next frame poses from there
    pattern, root = _write_frames(tmp_path / "b", 5, recolour_from=3)
    log = []
    got = F.render_sequence(pattern, range(5), str(tmp_path / "b" / "pose" / "{frame}.png"), W, H, root, bvh="refit", pose=True,
                            on_frame=lambda f, how: log.append(how))
    assert log[:3] == ["build", "pose", "pose"] and log[3] in ("refit", "appearance") and log[4] == "pose"
    want = F.render_sequence(pattern, range(5), str(tmp_path / "b" / "parse" / "{frame}.png"), W, H, root, bvh="refit")
    # Here most vertices differ from the parse path's in the last bit (the rest frame is itself rounded), and the reference's
    # sampler re-seeds every bounce from the hit POSITION (tracer.fs:458): the two pictures then carry independent noise, and
    # their per-pixel difference measures 64 spp of noise (4.9 / 255 when this was written), not the pose.  What the pose
    # could get wrong is a bias, so the same bound is put on 8 x 8 block means, where independent noise shrinks 8-fold.
    assert open(got[3], "rb").read() == open(want[3], "rb").read()  # the parse-path frame between them is the same picture
    a, b = (np.asarray(Image.open(p[4]), np.float64) for p in (got, want))
    blocks = lambda x: x.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3))
    print(f"frame after a re-set pose: mean absolute difference {np.abs(a - b).mean():.4f} / 255 per pixel, "
          f"{np.abs(blocks(a) - blocks(b)).mean():.4f} / 255 on 8 x 8 block means")
    assert np.abs(blocks(a) - blocks(b)).mean() <= 2.0
    assert np.abs(a - np.asarray(Image.open(got[2]), np.float64)).mean() > 2.0  # (the floor changed colour)
