"""In-place geometry update (fspt_scene_update_geometry) on the MI355X.  No tolerance anywhere: a refitted
scene must be indistinguishable from a scene created from scratch out of the same topology, the moved triangles and the
boxes tests/refit_ref.py recomputes on the host - in closest hits, traversal step and leaf counts, two-level nodes, light
table and rendered frames - and equal to the oracle on those arrays."""
import dataclasses
import json
import os

import numpy as np
import pytest

import hitref as HR
import lights_ref as LR
import oracle as O
import rays as RY
import refit_ref as R
from conftest import random_rays
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene, device_memory
from fspt_amd import _lib as L
from fspt_amd import scene as S
from refit_moves import rotated, sine

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H = 64, 48


# ---- scenes and moves ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(small_scene, medium_scene):
    return {"small": small_scene, "medium": medium_scene, "textured": S.textured_test_scene(), "lights": LR.scene_e1(),
            "gpu": S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu")}


def flatten_leaf(arrays):
    """every triangle one leaf owns collapsed onto that leaf's first vertex: a leaf box of zero extent"""
    tri = arrays.tri.copy().reshape(-1, 3, 3)
    leaf, first, cnt = R.ownership(arrays.bvh, arrays.n_tris)
    k = int(np.argmax(cnt > 0)) if arrays.n_tris < 8 else int(np.flatnonzero(cnt > 0)[len(leaf) // 2])
    tri[first[k]:first[k] + cnt[k]] = tri[first[k], 0]
    return tri.reshape(-1)


def moved(arrays, move):
    """(tri, norm or None) of the move"""
    if move == "identity":
        return arrays.tri.copy(), arrays.norm.copy()
    if move == "rotate":
        return rotated(arrays.tri, arrays.norm)
    if move == "translate":
        return (arrays.tri.reshape(-1, 3) + np.float32([0.11, -0.07, 0.05])).astype(np.float32).reshape(-1), None
    if move == "sine1":
        return sine(arrays.tri, 0.01), None
    if move == "sine10":
        return sine(arrays.tri, 0.1), None
    if move == "flatten":
        return flatten_leaf(arrays), None
    raise KeyError(move)


MOVES = ("identity", "rotate", "translate", "sine1", "sine10", "flatten")
SCENES = ("small", "medium", "textured", "lights", "gpu")


def fresh_arrays(arrays, tri, norm):
    """arrays' of the issue: the moved data under the same topology with refit_ref's boxes"""
    return dataclasses.replace(arrays, tri=np.ascontiguousarray(tri, np.float32),
                               norm=arrays.norm if norm is None else np.ascontiguousarray(norm, np.float32),
                               bvh=R.refit(arrays.bvh, tri))


def ray_set(arrays, n=192):
    cam = O.camera(W, H, CAM["P"], CAM["I"], CAM["fov_scale"], S.lens_features(CAM["focal_depth"], CAM["aperture"]), 3.0)
    camr = np.concatenate([cam[0][..., :3].reshape(-1, 3), cam[1][..., :3].reshape(-1, 3)], 1).astype(np.float32)
    fam = [r for r, _ in RY.all_families(arrays, 5, n)]
    return np.concatenate([camr, random_rays(arrays, 2048, 1)] + fam).astype(np.float32)


def make_pt(sc, pipeline="wavefront", sampler=None, lights=False, seed=7, w=W, h=H):
    pt = PathTracer(sc, w, h, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if sampler:
        pt.set_sampler(sampler, 11)
    if lights:
        pt.set_lights("emitters", 0.5)
    return pt


def frame(sc, n=8, **kw):
    pt = make_pt(sc, **kw)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img


def same_hits(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


# ---- 5: equivalence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_updated_scene_equals_fresh_scene(scenes, name, move):
    arrays = scenes[name]
    tri, norm = moved(arrays, move)
    fresh = fresh_arrays(arrays, tri, norm)
    A = Scene(arrays)
    A.update_geometry(tri, norm)
    B = Scene(fresh)
    try:
        rays = ray_set(fresh)
        ha, hb = A.intersect(rays), B.intersect(rays)
        for k, what in enumerate(("t", "index", "steps", "leaves")):
            x, y = ha[k], hb[k]
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, int((x.view(np.uint32) != y.view(np.uint32)).sum()))
        assert A.two_level_nodes() == B.two_level_nodes()
        if B.two_level_nodes()[0]:
            assert same_hits(A.intersect(rays, two_level=True), B.intersect(rays, two_level=True))
            assert same_hits(A.intersect(rays, two_level=True), ha)
        assert A.depth == B.depth
        assert A.light_count() == B.light_count()
        ta, tb = A.light_table(), B.light_table()
        assert sorted(ta) == sorted(tb)
        for key in ta:
            assert np.array_equal(ta[key].view(np.uint32), tb[key].view(np.uint32)), key
        for pipeline in ("wavefront", "stream", "megakernel"):
            for sampler in (None, "sobol"):
                for lights in (False, True):
                    kw = dict(pipeline=pipeline, sampler=sampler, lights=lights)
                    fa, fb = frame(A, **kw), frame(B, **kw)
                    assert np.array_equal(fa, fb), (kw, int((fa != fb).any(-1).sum()))
                    assert np.isfinite(fa).all()
    finally:
        A.close(); B.close()


# ---- 6: against the oracle directly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("move", ("rotate", "sine10", "flatten"))
@pytest.mark.parametrize("name", ("small", "textured", "gpu"))
def test_updated_scene_equals_oracle(scenes, name, move):
    arrays = scenes[name]
    tri, norm = moved(arrays, move)
    fresh = fresh_arrays(arrays, tri, norm)
    A = Scene(arrays)
    A.update_geometry(tri, norm)
    got = frame(A, n=4, seed=1)
    A.close()
    want = np.zeros((H, W, 4), np.float32)
    O.render(fresh, W, H, CAM["P"], CAM["I"], CAM["fov_scale"], S.lens_features(CAM["focal_depth"], CAM["aperture"]),
             CAM["env_theta"], 4, 0, 4, 1, want)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    assert got[..., :3].max() > 0


# ---- 7: against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "medium"))
def test_deformed_hits_agree_with_float64(scenes, name):
    """test_traversal_gpu.py's acceptance rule with its own bounds (tests/hitref.py).  Which rays the rule sets aside as
    ambiguous is decided by the arrays and the rays alone, so the share set aside for the updated scene IS the share set
    aside for the fresh one; both must pass on every decisive ray."""
    arrays = scenes[name]
    tri, _ = moved(arrays, "sine10")
    fresh = fresh_arrays(arrays, tri, None)
    A = Scene(arrays)
    A.update_geometry(tri)
    B = Scene(fresh)
    for rays, fam in RY.all_families(fresh, 2, 512):
        ref = HR.classify(fresh, rays)
        ta, ia, _, _ = A.intersect(rays)
        tb, ib, _, _ = B.intersect(rays)
        bad = ref.mismatches(ta, ia)
        assert not bad, f"{fam}: " + "; ".join(ref.describe(i, ta, ia) for i in bad[:3])
        assert not ref.mismatches(tb, ib), fam
        print(f"{name} {fam}: ambiguous share {float((ref.kind < 0).mean()):.4f} (the same classification judges both scenes)")
    A.close(); B.close()


# ---- 8: identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "gpu"))
def test_identity_update_changes_nothing(scenes, name):
    arrays = scenes[name]
    sc = Scene(arrays)
    rays = ray_set(arrays)
    h0, f0, q0, c0 = sc.intersect(rays), frame(sc), sc.two_level_nodes(), sc.sah_cost()
    sc.update_geometry(arrays.tri, arrays.norm)
    assert same_hits(sc.intersect(rays), h0)
    assert np.array_equal(frame(sc), f0)
    assert sc.two_level_nodes() == q0 and sc.sah_cost() == c0
    sc.close()


# ---- 9: device form --------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form(scenes):
    import torch
    arrays = scenes["medium"]
    keep = (arrays.tri.copy(), arrays.norm.copy(), arrays.bvh.copy())
    tri, norm = moved(arrays, "rotate")
    A = Scene(arrays)
    A.update_geometry(tri, norm)
    D = Scene(arrays)
    D.update_geometry(torch.from_numpy(tri).to("cuda:0"), torch.from_numpy(norm).to("cuda:0"))
    rays = ray_set(fresh_arrays(arrays, tri, norm))
    assert same_hits(A.intersect(rays), D.intersect(rays))
    assert np.array_equal(frame(A), frame(D))
    t2 = torch.from_numpy(moved(arrays, "sine1")[0]).to("cuda:0")
    A.update_geometry(t2.cpu().numpy()); D.update_geometry(t2)  # norm=None keeps the rotated normals
    assert np.array_equal(frame(A), frame(D))
    with pytest.raises(TypeError):
        D.update_geometry(t2, norm)  # one on the device, one on the host
    with pytest.raises(ValueError):
        D.update_geometry(t2[:-9])
    with pytest.raises(TypeError):
        D.update_geometry(t2.double())
    assert arrays.tri.tobytes() == keep[0].tobytes() and arrays.norm.tobytes() == keep[1].tobytes() and arrays.bvh.tobytes() == keep[2].tobytes()
    A.close(); D.close()


# ---- 10: ordering ----------------------------------------------------------------------------------------------------
def test_recorded_ticks_run_before_the_update(scenes):
    """drawCamera / drawTracer pairs recorded (deferred) before the update see the OLD geometry, ticks after it the new:
    the same accumulator as a run that syncs before updating."""
    arrays = scenes["small"]
    tri, norm = moved(arrays, "rotate")
    out = []
    for sync_first in (False, True):
        sc = Scene(arrays)
        pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        pt.update_geometry(tri, norm)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance())
        pt.close(); sc.close()
    assert np.array_equal(out[0], out[1])
    # and it is neither all-old nor all-new
    sc = Scene(arrays); pt = make_pt(sc)
    for _ in range(6):
        pt.tick()
    assert not np.array_equal(pt.readRadiance(), out[0])
    pt.close(); sc.close()


def test_present_around_an_update(scenes):
    """A frame in flight when the update arrives is presented once, unchanged; the frames after it show the new geometry.
    The yardstick is a second tracer that draws (blocking) where the first presents."""
    arrays = scenes["small"]
    tri, norm = moved(arrays, "rotate")
    sc = Scene(arrays); pt = make_pt(sc)
    ref = Scene(arrays); pr = make_pt(ref)

    def ticks(n):
        for _ in range(n):
            pt.tick(); pr.tick()

    ticks(2)
    img, n = pt.present()
    assert img is None and n == 0
    pre = pr.draw()
    pt.update_geometry(tri, norm); pr.update_geometry(tri, norm)
    ticks(2)
    img, n = pt.present()
    assert n == 2 and np.array_equal(img, pre)        # the pre-update frame, once
    post = pr.draw()
    assert not np.array_equal(post, pre)
    ticks(1)
    img, n = pt.present()
    assert n == 4 and np.array_equal(img, post)       # then post-update frames
    post = pr.draw()
    img, n = pt.present()
    assert n == 5 and np.array_equal(img, post)
    assert np.array_equal(pt.readRadiance(), pr.readRadiance())
    pt.close(); pr.close(); sc.close(); ref.close()


def test_two_targets_and_moving_back(scenes):
    arrays = scenes["small"]
    tri, norm = moved(arrays, "rotate")
    sc = Scene(arrays)
    p1, p2 = make_pt(sc), make_pt(sc, pipeline="stream", w=48, h=32)
    p1.render(8); p2.render(8)
    first = (p1.readRadiance(), p2.readRadiance())
    p1.tick(); p2.tick()  # recorded on both when the update arrives
    p1.update_geometry(tri, norm)
    B = Scene(fresh_arrays(arrays, tri, norm))
    q1, q2 = make_pt(B), make_pt(B, pipeline="stream", w=48, h=32)
    for a, b in ((p1, q1), (p2, q2)):
        a.clear(); a.seed(7); a.render(8); b.render(8)
        assert np.array_equal(a.readRadiance(), b.readRadiance())
    sc.update_geometry(arrays.tri, arrays.norm)  # move back
    for p, want in zip((p1, p2), first):
        p.clear(); p.seed(7); p.render(8)
        assert np.array_equal(p.readRadiance(), want)
    for p in (p1, p2, q1, q2):
        p.close()
    sc.close(); B.close()


def test_multi_update(scenes):
    arrays = scenes["small"]
    tri, norm = moved(arrays, "rotate")
    mp = MultiPathTracer(arrays, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    mp.update_geometry(tri, norm)
    mp.render(8)
    got = mp.readRadiance()
    mp.close()
    B = Scene(fresh_arrays(arrays, tri, norm))
    assert np.array_equal(got, frame(B))
    B.close()


# ---- 11: errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_unchanged(scenes):
    import torch
    arrays = scenes["small"]
    sc = Scene(arrays)
    f0 = frame(sc)
    rays = ray_set(arrays)
    h0 = sc.intersect(rays)
    for bad_val in (np.nan, np.inf, -np.inf):
        for which in ("tri", "norm"):
            tri, norm = sine(arrays.tri, 0.1), arrays.norm.copy()
            (tri if which == "tri" else norm)[arrays.n_tris * 4 + 1] = bad_val
            for dev in (False, True):
                with pytest.raises(FsptError) as ei:
                    if dev:
                        sc.update_geometry(torch.from_numpy(tri).to("cuda:0"), torch.from_numpy(norm).to("cuda:0"))
                    else:
                        sc.update_geometry(tri, norm)
                assert ei.value.code == -1, (bad_val, which, dev)
    assert same_hits(sc.intersect(rays), h0) and np.array_equal(frame(sc), f0)
    lib = L.lib()
    assert lib.fspt_scene_update_geometry(sc._h, None, None) == -1
    assert lib.fspt_scene_update_geometry_device(sc._h, None, None) == -1
    assert lib.fspt_scene_sah_cost(sc._h, None) == -1
    for n in (arrays.tri.size - 9, arrays.tri.size + 9):
        with pytest.raises(ValueError):
            sc.update_geometry(np.zeros(n, np.float32))
    with pytest.raises(ValueError):
        sc.update_geometry(arrays.tri, arrays.norm[:-27])
    sc.close()
    # two leaves that share a triStart: the scene renders, but cannot be refitted
    bvh = arrays.bvh.copy().reshape(-1, 9)
    w = bvh[:, :3].view(np.int32)
    leaves = np.flatnonzero(w[:, 2] > -1)
    w[leaves[1], 2] = w[leaves[0], 2]
    shared = Scene(dataclasses.replace(arrays, bvh=bvh.reshape(-1)))
    with pytest.raises(FsptError) as ei:
        shared.update_geometry(arrays.tri)
    assert ei.value.code == -6 and "not refittable" in str(ei.value)
    shared.close()


# ---- 12: nothing new for scenes that never update --------------------------------------------------------------------
def test_scene_that_never_updates_allocates_nothing_new(scenes):
    """The free-memory deltas tests/test_parity_gpu.py::test_closed_tracers_return_their_device_memory accepts, around a
    scene and a tracer that never update; and an update's device copies go back when the scene closes."""
    arrays = scenes["medium"]

    def cycle(update):
        sc = Scene(arrays)
        pt = make_pt(sc, w=256, h=192)
        pt.render(2); pt.readRadiance()
        if update:
            sc.update_geometry(arrays.tri, arrays.norm)
        pt.close(); sc.close()

    cycle(False)  # the yardstick run: what the runtime keeps of a stream's queues is its own pool
    free1 = device_memory(0)[0]
    cycle(False)
    assert device_memory(0)[0] >= free1 - (4 << 20)
    cycle(True)
    assert device_memory(0)[0] >= free1 - (4 << 20)


# ---- 13: SAH cost ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "medium", "gpu"))
def test_sah_cost(scenes, name):
    arrays = scenes[name]
    sc = Scene(arrays)
    c0 = sc.sah_cost()
    assert c0 == pytest.approx(R.sah_cost(arrays.bvh, arrays.n_tris), rel=1e-12)
    assert c0 == pytest.approx(S.sah_cost(arrays), rel=1e-12)
    import importlib.util
    spec = importlib.util.spec_from_file_location("bvh_build_bench", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "bvh_build_bench.py"))
    bb = importlib.util.module_from_spec(spec); spec.loader.exec_module(bb)
    assert c0 == pytest.approx(bb.sah_cost(arrays), rel=1e-12)
    tri = sine(arrays.tri, 0.1)
    sc.update_geometry(tri)
    c1 = sc.sah_cost()
    assert c1 == pytest.approx(R.sah_cost(R.refit(arrays.bvh, tri), arrays.n_tris), rel=1e-12)
    print(f"{name}: sah_cost {c0:.4f} -> {c1:.4f} under the 10 % sine deformation")
    assert c1 >= c0
    sc.close()


# ---- 14: render_sequence(bvh="refit") --------------------------------------------------------------------------------
def _write_frames(tmp_path, n_frames, extra_tri_frame=None):
    """scene files of a glowing cube-sphere that moves over a quad, one JSON per frame"""
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    glow = "mtllib ball.mtl\nusemtl glow\n"
    (root / "mesh" / "ball.obj").write_text(glow + S.cube_sphere_obj(4))
    (root / "mesh" / "ball6.obj").write_text(glow + S.cube_sphere_obj(6))
    (root / "mesh" / "ball.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    for f in range(n_frames):
        ball = "mesh/ball6.obj" if f == extra_tri_frame else "mesh/ball.obj"
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 4, "exposure": 1.2,
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6],
                                   "emittance": [0, 0, 0]}],
                 "animated_props": [{"path": ball, "scale": 0.4, "translate": [-0.4 + 0.4 * f, 0.05 * f, 0.0],
                                     "rotate": [{"axis": [0, 1, 0], "angle": 0.3 * f}], "diffuse": [0.8, 0.3, 0.2],
                                     "emittance": [3, 3, 3], "normals": "smooth"}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def test_render_sequence_refit(tmp_path):
    from PIL import Image
    from fspt_amd import scene_file as F
    pattern, root = _write_frames(tmp_path, 3)
    got = F.render_sequence(pattern, range(3), str(tmp_path / "refit" / "{frame}.png"), W, H, root, bvh="refit", samples=4)
    # the same frames rendered from scratch on per-frame arrays whose tree is frame 0's with refit_ref's boxes
    a0, _ = F.load_scene_file(pattern.format(frame=0), root, keep_order=True)
    for f in range(3):
        g, settings = F.load_scene_file(pattern.format(frame=f), root, geometry_only=True)
        tri, norm = S.geometry_in_leaf_order(a0, g.tri, g.norm)
        arr = a0 if f == 0 else fresh_arrays(a0, tri, norm)
        rgba, _ = F.render_frame(arr, settings, W, H, samples=4)
        want = str(tmp_path / "want" / f"{f}.png")
        os.makedirs(os.path.dirname(want), exist_ok=True)
        Image.fromarray(rgba[:, :, :3]).save(want)
        assert open(got[f], "rb").read() == open(want, "rb").read(), f
    assert open(got[0], "rb").read() != open(got[2], "rb").read()
    assert np.asarray(Image.open(got[2])).max() > 0
    # a frame with another triangle count rebuilds
    pattern, root = _write_frames(tmp_path / "b", 3, extra_tri_frame=1)
    log = []
    got = F.render_sequence(pattern, range(3), str(tmp_path / "b" / "refit" / "{frame}.png"), W, H, root, bvh="refit", samples=4,
                            on_frame=lambda f, how: log.append(how))
    assert log == ["build", "build", "build"]
    want = F.render_sequence(pattern, range(3), str(tmp_path / "b" / "sah" / "{frame}.png"), W, H, root, bvh="sah", samples=4)
    for a, b in zip(got, want):
        assert open(a, "rb").read() == open(b, "rb").read()


# ---- the Node host ---------------------------------------------------------------------------------------------------
def test_node_update_geometry_matches_python(scenes, tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("node") is None or not os.path.exists(os.path.join(root, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    e1 = scenes["lights"]  # (no environment map: the job files stay small)
    tri, norm = moved(e1, "rotate")
    B = Scene(fresh_arrays(e1, tri, norm))
    want, cost = frame(B, n=6), B.sah_cost()
    B.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    tri.tofile(os.path.join(d, "tri2.bin")); norm.tofile(os.path.join(d, "norm2.bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=6, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(root, "tests", "refit_node_check.js"), os.path.join(root, "fspt_amd", "js"), d],
                          timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got, want)
    c = json.load(open(os.path.join(d, "cost.json")))
    assert c["after"] == cost and c["before"] == pytest.approx(R.sah_cost(e1.bvh, e1.n_tris), rel=1e-12)
