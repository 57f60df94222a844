"""In-place BVH rebuild (fspt_scene_rebuild_geometry) on the MI355X.  No tolerance anywhere: after the call
the scene must be indistinguishable from a scene created from scratch out of tests/rebuild_ref.py's arrays - the binned-SAH
tree of tests/bvh_binned_ref.py over the new triangles in the order given, the per-triangle data permuted by it - in
closest hits, step and leaf counts of both node forms, depth, two-level nodes, light table, SAH cost and frames of every
pipeline, sampler and light mode; and the order it returns must be that tree's."""
import dataclasses
import json
import os

import numpy as np
import pytest

import lights_ref as LR
import oracle as O
import rebuild_ref as RB
import refit_ref as R
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene, device_memory
from fspt_amd import _lib as L
from fspt_amd import scene as S
from refit_moves import sine
from test_refit_gpu import CAM, H, W, frame, fresh_arrays, make_pt, moved, ray_set, same_hits

pytestmark = pytest.mark.gpu
MOVES = ("identity", "rotate", "sine1", "sine10", "flatten")
SCENES = ("small", "medium", "textured", "lights", "gpu")


@pytest.fixture(scope="module")
def scenes(small_scene, medium_scene):
    return {"small": small_scene, "medium": medium_scene, "textured": S.textured_test_scene(), "lights": LR.scene_e1(),
            "gpu": S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu")}


def assert_same_scene(A, B, rays, frames=True):
    """everything the rule lists, array_equal"""
    ha, hb = A.intersect(rays), B.intersect(rays)
    for k, what in enumerate(("t", "index", "steps", "leaves")):
        x, y = ha[k].view(np.uint32), hb[k].view(np.uint32)
        assert np.array_equal(x, y), (what, int((x != y).sum()))
    assert A.two_level_nodes() == B.two_level_nodes()
    if B.two_level_nodes()[0]:
        assert same_hits(A.intersect(rays, two_level=True), B.intersect(rays, two_level=True))
    assert A.depth == B.depth
    assert A.sah_cost() == B.sah_cost()
    assert A.light_count() == B.light_count()
    ta, tb = A.light_table(), B.light_table()
    assert sorted(ta) == sorted(tb)
    for key in ta:
        assert np.array_equal(ta[key].view(np.uint32), tb[key].view(np.uint32)), key
    if not frames:
        return
    for pipeline in ("wavefront", "stream", "megakernel"):
        for sampler in (None, "sobol"):
            for lights in (False, True):
                kw = dict(pipeline=pipeline, sampler=sampler, lights=lights)
                fa, fb = frame(A, **kw), frame(B, **kw)
                assert np.array_equal(fa, fb), (kw, int((fa != fb).any(-1).sum()))
                assert np.isfinite(fa).all()


# ---- 1: the rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_rebuilt_scene_equals_fresh_scene(scenes, name, move):
    arrays = scenes[name]
    tri, norm = moved(arrays, move)
    if move == "identity":
        norm = None  # every triangle keeps the record it has
    order, fresh = RB.expected(arrays, tri, norm)
    A = Scene(arrays)
    got = A.rebuild_geometry(tri, norm)
    B = Scene(fresh)
    try:
        assert got.dtype == np.uint32 and np.array_equal(got, order)
        if (name, move) == ("medium", "sine10"):
            assert not np.array_equal(order, np.arange(arrays.n_tris))  # (else this case shows nothing)
        assert_same_scene(A, B, ray_set(fresh))
        ms = A.last_rebuild_ms()
        assert ms["launches"] > 0 and ms["readbacks"] >= 3 and ms["build_ms"] > 0 and ms["install_ms"] > 0
    finally:
        A.close(); B.close()


# ---- 2: against the oracle directly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("move", ("rotate", "sine10", "flatten"))
@pytest.mark.parametrize("name", ("small", "textured", "gpu"))
def test_rebuilt_scene_equals_oracle(scenes, name, move):
    arrays = scenes[name]
    tri, norm = moved(arrays, move)
    _, fresh = RB.expected(arrays, tri, norm)
    A = Scene(arrays)
    A.rebuild_geometry(tri, norm)
    got = frame(A, n=8, seed=1)
    A.close()
    want = np.zeros((H, W, 4), np.float32)
    O.render(fresh, W, H, CAM["P"], CAM["I"], CAM["fov_scale"], S.lens_features(CAM["focal_depth"], CAM["aperture"]),
             CAM["env_theta"], 4, 0, 8, 1, want)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    assert got[..., :3].max() > 0


# ---- 3: identity -----------------------------------------------------------------------------------------------------
def test_identity_rebuild_of_a_binned_tree_changes_nothing(scenes):
    arrays = scenes["gpu"]
    sc = Scene(arrays)
    rays = ray_set(arrays)
    h0, f0, q0, c0, d0 = sc.intersect(rays), frame(sc), sc.two_level_nodes(), sc.sah_cost(), sc.depth
    for norm in (None, arrays.norm):
        order = sc.rebuild_geometry(arrays.tri, norm)
        assert np.array_equal(order, np.arange(arrays.n_tris, dtype=np.uint32))
        assert same_hits(sc.intersect(rays), h0)
        assert np.array_equal(frame(sc), f0)
        assert sc.two_level_nodes() == q0 and sc.sah_cost() == c0 and sc.depth == d0
    sc.close()


# ---- 4: targets that live through a rebuild --------------------------------------------------------------------------
@pytest.mark.parametrize("name,move", (("small", "sine10"), ("medium", "rotate"), ("lights", "sine1")))
def test_targets_survive_the_rebuild(scenes, name, move):
    """A target made before the rebuild renders, after clear(), what a target made after it renders.  medium x rotate is
    the case where the depth changes (13 -> 15 by the restatement: asserted), so the traversal stack and the
    suspended-traversal records change size under a live target; lights x sine1 goes 9 -> 8."""
    arrays = scenes[name]
    tri, norm = moved(arrays, move)
    _, fresh = RB.expected(arrays, tri, norm)
    if (name, move) in (("medium", "rotate"), ("lights", "sine1")):
        assert fresh.depth != arrays.depth
    kws = [dict(pipeline=p, sampler=s, lights=l) for p in ("wavefront", "stream", "megakernel")
           for s, l in ((None, False), ("sobol", False), (None, True), ("sobol", True))]
    sc = Scene(arrays)
    old = [make_pt(sc, **kw) for kw in kws]
    for p in old:
        p.render(8)
    for p in old[:3]:
        p.tick()  # recorded when the rebuild arrives
    old[0].rebuild_geometry(tri, norm)
    assert sc.depth == fresh.depth
    for p, kw in zip(old, kws):
        p.clear(); p.seed(7); p.render(8)
        q = make_pt(sc, **kw)
        q.render(8)
        a, b = p.readRadiance(), q.readRadiance()
        assert np.array_equal(a, b), (kw, int((a != b).any(-1).sum()))
        q.close()
    for p in old:
        p.close()
    sc.close()


# ---- 5: update after rebuild, rebuild after rebuild ------------------------------------------------------------------
def test_update_after_rebuild_and_rebuild_back(scenes):
    arrays = scenes["small"]
    tri1, norm1 = moved(arrays, "rotate")
    o1, f1 = RB.expected(arrays, tri1, norm1)
    sc = Scene(arrays)
    order = sc.rebuild_geometry(tri1, norm1).astype(np.int64)
    # refit in the NEW leaf order
    tri2 = sine(arrays.tri, 0.1).reshape(-1, 9)[order].reshape(-1)
    sc.update_geometry(tri2)
    B = Scene(fresh_arrays(f1, tri2, None))
    assert_same_scene(sc, B, ray_set(f1), frames=False)
    assert np.array_equal(frame(sc), frame(B))
    B.close()
    # back to the original triangles, fed in the new leaf order: expected() applied twice
    back_tri = arrays.tri.reshape(-1, 9)[order].reshape(-1)
    back_norm = arrays.norm.reshape(-1, 27)[order].reshape(-1)
    o2, f2 = RB.expected(f1, back_tri, back_norm)
    got = sc.rebuild_geometry(back_tri, back_norm)
    assert np.array_equal(got, o2)
    B = Scene(f2)
    assert_same_scene(sc, B, ray_set(f2), frames=False)
    assert np.array_equal(frame(sc, lights=True), frame(B, lights=True))
    sc.close(); B.close()


# ---- 6: device form, ordering ----------------------------------------------------------------------------------------
def test_device_form_equals_host_form(scenes):
    import torch
    arrays = scenes["medium"]
    keep = (arrays.tri.copy(), arrays.norm.copy(), arrays.bvh.copy())
    tri, norm = moved(arrays, "rotate")
    A = Scene(arrays)
    oa = A.rebuild_geometry(tri, norm)
    D = Scene(arrays)
    od = D.rebuild_geometry(torch.from_numpy(tri).to("cuda:0"), torch.from_numpy(norm).to("cuda:0"))
    assert od.is_cuda and od.dtype == torch.int64 and np.array_equal(od.cpu().numpy(), oa.astype(np.int64))
    assert_same_scene(A, D, ray_set(RB.expected(arrays, tri, norm)[1]), frames=False)
    assert np.array_equal(frame(A), frame(D))
    t2 = torch.from_numpy(moved(arrays, "sine1")[0]).to("cuda:0").reshape(-1, 9)[od].reshape(-1).contiguous()
    oa2, od2 = A.rebuild_geometry(t2.cpu().numpy()), D.rebuild_geometry(t2)  # norm=None keeps the rotated normals
    assert np.array_equal(od2.cpu().numpy(), oa2.astype(np.int64))
    assert np.array_equal(frame(A), frame(D)) and A.sah_cost() == D.sah_cost()
    with pytest.raises(TypeError):
        D.rebuild_geometry(t2, norm)
    with pytest.raises(ValueError):
        D.rebuild_geometry(t2[:-9])
    with pytest.raises(TypeError):
        D.rebuild_geometry(t2.double())
    assert arrays.tri.tobytes() == keep[0].tobytes() and arrays.norm.tobytes() == keep[1].tobytes() and arrays.bvh.tobytes() == keep[2].tobytes()
    A.close(); D.close()


def test_recorded_ticks_run_before_the_rebuild(scenes):
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
        pt.rebuild_geometry(tri, norm)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance())
        pt.close(); sc.close()
    assert np.array_equal(out[0], out[1])
    sc = Scene(arrays); pt = make_pt(sc)
    for _ in range(6):
        pt.tick()
    assert not np.array_equal(pt.readRadiance(), out[0])
    pt.close(); sc.close()


def test_present_around_a_rebuild(scenes):
    """A frame in flight when the rebuild arrives is presented once, unchanged; the frames after it show the new scene.
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
    pt.rebuild_geometry(tri, norm); pr.rebuild_geometry(tri, norm)
    ticks(2)
    img, n = pt.present()
    assert n == 2 and np.array_equal(img, pre)        # the pre-rebuild frame, once
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


# ---- 7: errors, memory -----------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_unchanged(scenes):
    import torch
    arrays = scenes["small"]
    sc = Scene(arrays)
    pt = make_pt(sc)
    f0, c0 = frame(sc), sc.sah_cost()
    rays = ray_set(arrays)
    h0 = sc.intersect(rays)
    for bad_val in (np.nan, np.inf):
        for which in ("tri", "norm"):
            tri, norm = sine(arrays.tri, 0.1), arrays.norm.copy()
            (tri if which == "tri" else norm)[arrays.n_tris * 4 + 1] = bad_val
            for dev in (False, True):
                with pytest.raises(FsptError) as ei:
                    if dev:
                        sc.rebuild_geometry(torch.from_numpy(tri).to("cuda:0"), torch.from_numpy(norm).to("cuda:0"))
                    else:
                        sc.rebuild_geometry(tri, norm)
                assert ei.value.code == -1, (bad_val, which, dev)
    lib = L.lib()
    assert lib.fspt_scene_rebuild_geometry(sc._h, None, None, None) == -1
    assert lib.fspt_scene_rebuild_geometry_device(sc._h, None, None, None) == -1
    for n in (arrays.tri.size - 9, arrays.tri.size + 9):
        with pytest.raises(ValueError):
            sc.rebuild_geometry(np.zeros(n, np.float32))
    with pytest.raises(ValueError):
        sc.rebuild_geometry(arrays.tri, arrays.norm[:-27])
    assert same_hits(sc.intersect(rays), h0) and np.array_equal(frame(sc), f0) and sc.sah_cost() == c0
    pt.render(8)
    assert np.array_equal(pt.readRadiance(), f0)
    pt.close(); sc.close()
    # two leaves that share a triStart: the scene renders, but the triangle -> slot map is undefined
    bvh = arrays.bvh.copy().reshape(-1, 9)
    w = bvh[:, :3].view(np.int32)
    leaves = np.flatnonzero(w[:, 2] > -1)
    w[leaves[1], 2] = w[leaves[0], 2]
    shared = Scene(dataclasses.replace(arrays, bvh=bvh.reshape(-1)))
    f0, h0 = frame(shared), shared.intersect(rays)
    with pytest.raises(FsptError) as ei:
        shared.rebuild_geometry(arrays.tri)
    assert ei.value.code == -6 and "not refittable" in str(ei.value)
    assert same_hits(shared.intersect(rays), h0) and np.array_equal(frame(shared), f0)
    shared.close()


def test_twenty_rebuilds_do_not_grow(scenes):
    """free device memory after 20 rebuilds (alternating two shapes, host and device form) against after the first two, with
    the slack tests/test_refit_gpu.py accepts for what the runtime keeps in its own pools"""
    import torch
    arrays = scenes["medium"]
    sc = Scene(arrays)
    pt = make_pt(sc, w=256, h=192)
    a = arrays.tri
    b = sine(arrays.tri, 0.1)
    order = np.arange(arrays.n_tris, dtype=np.int64)

    def step(tri, dev):
        nonlocal order
        t = np.ascontiguousarray(tri.reshape(-1, 9)[order]).reshape(-1)
        o = sc.rebuild_geometry(torch.from_numpy(t).to("cuda:0") if dev else t)
        order = order[(o.cpu().numpy() if dev else o).astype(np.int64)]
        pt.clear(); pt.render(2)

    step(b, False); step(a, True)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    free1 = device_memory(0)[0]
    for i in range(20):
        step(b if i % 2 == 0 else a, i % 4 >= 2)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    assert device_memory(0)[0] >= free1 - (4 << 20)
    assert np.array_equal(np.sort(order), np.arange(arrays.n_tris)) and np.isfinite(pt.readRadiance()).all()
    pt.close(); sc.close()


# ---- 8: SAH cost, multi, render_sequence, Node -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "medium", "gpu"))
def test_sah_cost_is_the_fresh_scenes(scenes, name):
    arrays = scenes[name]
    tri = sine(arrays.tri, 0.1)
    _, fresh = RB.expected(arrays, tri)
    sc = Scene(arrays)
    sc.update_geometry(tri)
    refit_cost = sc.sah_cost()
    sc.rebuild_geometry(tri)
    c = sc.sah_cost()
    B = Scene(fresh)
    assert c == B.sah_cost()  # the same float64: the same node order of the sum
    assert c == pytest.approx(S.sah_cost(fresh), rel=1e-12) and c == pytest.approx(R.sah_cost(fresh.bvh, fresh.n_tris), rel=1e-12)
    print(f"{name}: sah_cost refitted {refit_cost:.4f}, rebuilt in place {c:.4f} under the 10 % sine deformation")
    sc.close(); B.close()


def test_multi_rebuild(scenes):
    arrays = scenes["small"]
    tri, norm = moved(arrays, "rotate")
    order, fresh = RB.expected(arrays, tri, norm)
    mp = MultiPathTracer(arrays, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    assert np.array_equal(mp.rebuild_geometry(tri, norm), order)
    mp.render(8)
    got = mp.readRadiance()
    mp.close()
    B = Scene(fresh)
    assert np.array_equal(got, frame(B))
    B.close()


def _write_frames(tmp_path, n_frames):
    """scene files of a textured panel (explicit uvs, so that only its vertices change) that swings over a glowing
    cube-sphere and a floor, one JSON per frame"""
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    (root / "mesh" / "ball.obj").write_text("mtllib ball.mtl\nusemtl glow\n" + S.cube_sphere_obj(4))
    (root / "mesh" / "ball.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    for f in range(n_frames):
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 4, "exposure": 1.2,
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6],
                                   "emittance": [0, 0, 0]},
                                  {"path": "mesh/ball.obj", "scale": 0.4, "translate": [-0.2, 0.0, 0.0], "diffuse": [0.8, 0.3, 0.2],
                                   "emittance": [3, 3, 3], "normals": "smooth"}],
                 "animated_props": [{"path": "mesh/quad.obj", "scale": 0.8, "translate": [0.5 - 0.5 * f, 0.3 + 0.2 * f, -0.3 + 0.3 * f],
                                     "rotate": [{"axis": [1, 0, 0], "angle": 0.5 + 0.4 * f}], "diffuse": [0.2, 0.5, 0.8],
                                     "emittance": [0, 0, 0]}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def test_render_sequence_rebuilds_in_place(tmp_path):
    """rebuild_above = 0 fires on every refitted frame; the frames equal those of per-frame scenes that hold the binned tree
    of the same input order (tests/rebuild_ref.py applied frame after frame)."""
    from PIL import Image
    from fspt_amd import scene_file as F
    pattern, root = _write_frames(tmp_path, 3)
    log = []
    got = F.render_sequence(pattern, range(3), str(tmp_path / "inplace" / "{frame}.png"), W, H, root, bvh="refit", samples=4,
                            rebuild_above=0.0, on_frame=lambda f, how: log.append(how))
    assert log == ["build", "rebuild", "rebuild"]
    a0, _ = F.load_scene_file(pattern.format(frame=0), root, keep_order=True)
    cur, leaf_order = a0, a0.meta["tri_order"]
    for f in range(3):
        g, settings = F.load_scene_file(pattern.format(frame=f), root, geometry_only=True)
        if f > 0:
            tri, norm = S.geometry_in_leaf_order(leaf_order, g.tri, g.norm)
            order, cur = RB.expected(cur, tri, norm)
            leaf_order = S.compose_order(leaf_order, order)
        rgba, _ = F.render_frame(cur, settings, W, H, samples=4)
        want = str(tmp_path / "want" / f"{f}.png")
        os.makedirs(os.path.dirname(want), exist_ok=True)
        Image.fromarray(rgba[:, :, :3]).save(want)
        assert open(got[f], "rb").read() == open(want, "rb").read(), f
    assert open(got[0], "rb").read() != open(got[2], "rb").read()
    # the default is still "never"
    log = []
    F.render_sequence(pattern, range(3), str(tmp_path / "never" / "{frame}.png"), W, H, root, bvh="refit", samples=4,
                      on_frame=lambda f, how: log.append(how))
    assert log == ["build", "refit", "refit"]


def test_node_rebuild_geometry_matches_python(scenes, tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("node") is None or not os.path.exists(os.path.join(root, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    e1 = scenes["lights"]  # (no environment map: the job files stay small)
    tri, norm = moved(e1, "rotate")
    order, fresh = RB.expected(e1, tri, norm)
    B = Scene(fresh)
    want, cost = frame(B, n=6), B.sah_cost()
    B.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    tri.tofile(os.path.join(d, "tri2.bin")); norm.tofile(os.path.join(d, "norm2.bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=6, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(root, "tests", "rebuild_node_check.js"), os.path.join(root, "fspt_amd", "js"), d],
                          timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(np.fromfile(os.path.join(d, "order.bin"), np.uint32), order)
    assert json.load(open(os.path.join(d, "cost.json")))["after"] == cost
