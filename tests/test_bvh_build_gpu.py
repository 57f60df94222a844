"""fspt_builder_build_gpu: the binned-SAH tree built on the GPU is byte-equal to its numpy restatement
(tests/bvh_binned_ref.py), is a valid reference-layout tree on a 1 M-triangle scene, renders and intersects bit-equal to
the oracle on every pipeline, finds the same closest hits as the reference's tree, builds degenerate soups the
reference's builder cannot, and leaves the calling thread's device alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bvh_binned_ref as BR
import hitref as HR
import oracle as O
import rays as R
from fspt_amd import PathTracer, Scene, _lib as L, scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bvh", "tri", "mat", "norm", "uv")
E_INVALID, E_STATE = -1, -6  # include/fspt.h


def both_trees(make, *args):
    """the scene of make(*args) from each builder, with the triangle order: (sah arrays, gpu arrays)"""
    return (BR.rebuild(make, *args, bvh="sah", keep_order=True), BR.rebuild(make, *args, bvh="gpu", keep_order=True))


def scene_pair(name):
    if name == "small":
        return both_trees(S.bunny_scene, 8, (64, 32))
    if name == "medium":
        return both_trees(S.bunny_scene, 24, (256, 128), 3.0)
    if name == "c2":
        return both_trees(S.bunny_scene, 76, (64, 32))
    if name == "textured":
        return both_trees(S.textured_test_scene)
    return both_trees(R.fuzz_scene, int(name[4:]))


def assert_matches_restatement(cpu, gpu):
    tree, want = BR.expected_arrays(cpu)
    for f in FIELDS:
        got = getattr(gpu, f)
        assert got.shape == want[f].shape, f
        assert np.array_equal(got.view(np.uint32), want[f].view(np.uint32)), f
    assert gpu.depth == tree.depth
    assert np.array_equal(gpu.meta["tri_order"], tree.order)
    return tree


@pytest.mark.parametrize("name", ["small", "medium", "textured", "c2"] + [f"fuzz{s}" for s in range(8)])
def test_byte_equal_to_restatement(name):
    cpu, gpu = scene_pair(name)
    assert gpu.meta["bvh"] == "gpu" and cpu.meta["bvh"] == "sah"
    tree = assert_matches_restatement(cpu, gpu)
    print(f"\n{name}: {gpu.n_tris} triangles, {gpu.n_nodes} nodes (reference tree {cpu.n_nodes}), depth {gpu.depth} "
          f"(reference {cpu.depth}), SAH splits {tree.sah_split[tree.left >= 0].mean():.3f}")


def test_two_builds_byte_equal():
    a1 = S.bunny_scene(n=76, env_size=(64, 32), bvh="gpu")
    a2 = S.bunny_scene(n=76, env_size=(64, 32), bvh="gpu")
    for f in FIELDS:
        assert np.array_equal(getattr(a1, f).view(np.uint32), getattr(a2, f).view(np.uint32)), f
    assert a1.depth == a2.depth


def check_structure(arrays):
    BR.check_tree(arrays.bvh, arrays.tri, arrays.leaf_size, arrays.depth)


def test_c3_structure():
    cpu_free = S.bunny_scene(n=289, env_size=(64, 32), bvh="gpu")
    check_structure(cpu_free)
    # every triangle exactly once: the packed triangles are a permutation of the scene's
    a = S.build_scene(S.bunny_props(), {"synthetic/cube_sphere.obj": S.cube_sphere_obj(289), "synthetic/quad.obj": S.QUAD_OBJ},
                      bvh="gpu", keep_order=True)
    order = a.meta["tri_order"]
    assert np.array_equal(np.sort(order), np.arange(a.n_tris))
    assert np.array_equal(a.bvh.view(np.uint32), cpu_free.bvh.view(np.uint32))
    sc = Scene(cpu_free)  # fspt_scene_create accepts it
    assert sc.depth == cpu_free.depth
    print(f"\nc3: {cpu_free.n_tris} triangles, {cpu_free.n_nodes} nodes, depth {cpu_free.depth}")


def _render_both(arrays, pipeline, W=96, H=64, nb=6, ticks=3, seed=9):
    cam = S.BUNNY_CAMERA
    pt = PathTracer(arrays, W, H, num_bounces=nb)
    try:
        pt.set_pipeline(pipeline)
        pt.set_camera(**cam)
        pt.seed(seed)
        pt.render(ticks)
        got = pt.readRadiance()
    finally:
        pt.close()
        pt.scene.close()
    want = np.zeros((H, W, 4), np.float32)
    O.render(arrays, W, H, cam["P"], cam["I"], cam["fov_scale"], S.lens_features(cam["focal_depth"], cam["aperture"]),
             cam["env_theta"], nb, 0, ticks, seed, want)
    return got, want


@pytest.mark.parametrize("pipeline", ["wavefront", "stream", "megakernel"])
@pytest.mark.parametrize("name", ["medium", "fuzz3"])
def test_render_bitwise_on_gpu_tree(name, pipeline):
    _, gpu = scene_pair(name)
    got, want = _render_both(gpu, pipeline)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", ["small", "medium"] + [f"fuzz{s}" for s in range(8)])
def test_intersect_on_gpu_tree(name):
    _, arrays = scene_pair(name)
    sc = Scene(arrays)
    for rays, fam in R.all_families(arrays, 3, 512):
        rt, ridx, rsteps, rleaves = O.intersect(arrays, rays)
        t, idx, steps, leaves = sc.intersect(rays)
        assert np.array_equal(idx, ridx) and np.array_equal(t.view(np.uint32), rt.view(np.uint32)), fam
        assert np.array_equal(steps, rsteps) and np.array_equal(leaves, rleaves), fam
        ref = HR.classify(arrays, rays)
        bad = ref.mismatches(t, idx)
        assert not bad, f"{fam}: " + "; ".join(ref.describe(i, t, idx) for i in bad[:3])


def test_same_closest_hits_across_trees():
    cpu, gpu = scene_pair("medium")
    sa, sg = Scene(cpu), Scene(gpu)
    tc, tg = cpu.tri.reshape(-1, 9), gpu.tri.reshape(-1, 9)
    n_dec = 0
    for rays, fam in R.all_families(cpu, 5, 1024):
        ref = HR.classify(cpu, rays)
        t1, i1, s1, _ = sa.intersect(rays)
        t2, i2, s2, _ = sg.intersect(rays)
        dec = np.flatnonzero(ref.kind >= 0)
        n_dec += dec.size
        assert np.array_equal(t1[dec].view(np.uint32), t2[dec].view(np.uint32)), fam
        hit = dec[i1[dec] >= 0]
        assert np.array_equal(i2[hit] >= 0, np.ones(hit.size, bool)), fam
        single = [k for k in hit if len(ref.ties[k][0]) == 1]
        assert np.array_equal(tc[i1[single]].view(np.uint32), tg[i2[single]].view(np.uint32)), fam
    assert n_dec > 0
    cam = S.BUNNY_CAMERA
    dist = []
    for bvh in ("sah", "gpu"):
        a = S.build_scene(S.bunny_props(), {"synthetic/cube_sphere.obj": S.cube_sphere_obj(24), "synthetic/quad.obj": S.QUAD_OBJ},
                          bvh=bvh, focus_rays=[(cam["P"], cam["I"]), ([0, 3, 0], [0, -1, 0]), ([5, 5, 5], [1, 0, 0])])
        dist.append(a.meta["focus"])
    assert dist[0] == dist[1]


def _with_degenerate(kind):
    """the small scene plus 1 000 coincident triangles, or 1 000 zero-area triangles at one point"""
    if kind == "coincident":
        extra = "\n".join(["v 0.1 0.2 0.3", "v 0.4 0.25 0.3", "v 0.2 0.6 0.35"] + ["f 1 2 3"] * 1000) + "\n"
    else:
        extra = "\n".join(["v 0.1 0.2 0.3"] + ["f 1 1 1"] * 1000) + "\n"
    props = S.bunny_props() + [{"path": "d.obj", "scale": 1, "rotate": [], "translate": [0, 0, 0], "emittance": [0, 0, 0],
                                "normals": "flat", "diffuse": [0.5, 0.5, 0.5]}]
    texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ, "d.obj": extra}
    env, w, h = S.synthetic_env(64, 32)
    return props, texts, env, w, h


@pytest.mark.parametrize("kind", ["coincident", "zero_area"])
def test_degenerate_soups(kind):
    props, texts, env, w, h = _with_degenerate(kind)
    if kind == "coincident":
        cpu = S.build_scene(props, texts, env=env, env_w=w, env_h=h)
        assert cpu.depth > 64
        with pytest.raises(L.FsptError):
            Scene(cpu)
    else:
        with pytest.raises(L.FsptError):
            S.build_scene(props, texts, env=env, env_w=w, env_h=h)
    gpu = S.build_scene(props, texts, env=env, env_w=w, env_h=h, bvh="gpu", keep_order=True)
    check_structure(gpu)
    tree = BR.build(BR.geometry_order(gpu)["tri"], gpu.leaf_size)
    assert np.array_equal(gpu.bvh.view(np.uint32), tree.bvh.view(np.uint32))
    sc = Scene(gpu)
    assert sc.depth == gpu.depth
    sc.close()
    got, want = _render_both(gpu, "wavefront")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_current_device_unchanged():
    import torch
    torch.cuda.set_device(0)
    before = torch.cuda.current_device()
    S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu", device=0)
    assert torch.cuda.current_device() == before
    lib = L.lib()
    b = C.c_void_p()
    L.check(lib.fspt_builder_create(C.byref(b)))
    try:
        assert lib.fspt_builder_build_gpu(b, 4, L.lib().fspt_device_count()) == E_INVALID  # out of range
    finally:
        lib.fspt_builder_destroy(b)
    assert torch.cuda.current_device() == before


def test_gpu_stats_and_order():
    """fspt_builder_gpu_stats after a GPU build (launches and readbacks of the level loop), FSPT_E_STATE after a CPU one"""
    lib = L.lib()
    b = C.c_void_p()
    L.check(lib.fspt_builder_create(C.byref(b)))
    try:
        pd = L.PropDesc()
        pd.scale = 1.0
        text = S.cube_sphere_obj(24).encode()
        L.check(lib.fspt_builder_add_obj(b, text, len(text), C.byref(pd)))
        L.check(lib.fspt_builder_build_gpu(b, 4, 0))
        ms, la, rb = C.c_float(), C.c_uint32(), C.c_uint32()
        L.check(lib.fspt_builder_gpu_stats(b, C.byref(ms), C.byref(la), C.byref(rb)))
        assert ms.value > 0 and la.value >= 2 and rb.value >= 2
        L.check(lib.fspt_builder_build(b, 4))
        assert lib.fspt_builder_gpu_stats(b, C.byref(ms), C.byref(la), C.byref(rb)) == E_STATE
    finally:
        lib.fspt_builder_destroy(b)


def test_node_build_scene_gpu(tmp_path):
    """buildScene(..., {bvh: 'gpu'}) through the real addon gives the Python host's arrays"""
    import base64
    objs = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ}
    jp, op = str(tmp_path / "job.json"), str(tmp_path / "out.json")
    json.dump({"props": S.bunny_props(), "objs": objs, "device": 0}, open(jp, "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "bvh_node_check.js"), jp, op], timeout=300)
    out = json.load(open(op))
    a = S.build_scene(S.bunny_props(), objs, bvh="gpu")
    assert out["builder"] == "gpu" and out["depth"] == a.depth
    for f in FIELDS:
        got = np.frombuffer(base64.b64decode(out[f]), np.uint32)
        assert np.array_equal(got, getattr(a, f).view(np.uint32)), f
