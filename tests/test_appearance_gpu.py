"""In-place appearance update (fspt_scene_update_materials / _environment) on the MI355X.  No tolerance
anywhere: a scene updated to new materials, uvs, atlas and environment must be indistinguishable from a scene created from
the same arrays - in the bytes of the six buffers the update writes (which fspt_scene_create lays out with its own host
loops), in the light table and in rendered frames."""
import dataclasses
import json
import os

import numpy as np
import pytest

import appearance_cases as AC
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene, set_texture_interleave_budget
from fspt_amd import scene as S
from refit_moves import rotated

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 96, 64, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bases(small_scene):
    return AC.bases(small_scene)


@pytest.fixture(scope="module")
def pairs(bases):
    return AC.pairs(bases)


PAIR_NAMES = (*(f"res_{r}" for r in AC.ATLAS_RES), "res_1_to_16", "layers_shrink", "layers_grow", "image_to_const", "const_to_image",
              "all_const", "set_forms", "budget_0", "id_corners", "emissive_on", "emissive_off", "e3_dielectric_off", "e3_dielectric_on",
              "uv_kept", "small_retex", "fuzz_leaf5", *(f"env_{w}x{h}" for w, h in AC.ENV_SIZES), "env_none", "env_back", "env_one_bin")


def test_pair_names_are_the_cases(pairs):
    assert sorted(PAIR_NAMES) == sorted(pairs)


def make_pt(sc, pipeline="wavefront", sampler=None, lights=False, seed=7):
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if sampler:
        pt.set_sampler(sampler, 11)
    if lights:
        pt.set_lights("emitters", 0.5)
    return pt


def frame(sc, n=TICKS, **kw):
    pt = make_pt(sc, **kw)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img.view(np.uint32)  # (bit for bit: a NaN a random normal map may produce compares like any other word)


def update(sc, a, uv=True, atlas=True):
    sc.update_materials(a.mat, a.uv if uv else None, a.atlas if atlas else None, a.atlas_res, a.atlas_layers)
    sc.update_environment(a.env, a.env_w, a.env_h, a.bins)


def buffers(sc):
    return [sc.read_appearance(k) for k in range(6)]


def assert_same_scene(A, B, kws):
    for k, (x, y) in enumerate(zip(buffers(A), buffers(B))):
        assert x.size == y.size and np.array_equal(x, y), (Scene.APPEARANCE[k], x.size, y.size, int((x != y).sum()) if x.size == y.size else -1)
    assert A.light_count() == B.light_count()
    ta, tb = A.light_table(), B.light_table()
    for key in ta:
        assert np.array_equal(ta[key].view(np.uint32), tb[key].view(np.uint32)), key
    for kw in kws:
        fa, fb = frame(A, **kw), frame(B, **kw)
        assert np.array_equal(fa, fb), (kw, int((fa != fb).any(-1).sum()))


def product(name):
    if name in AC.FULL_PRODUCT:
        return [dict(pipeline=p, sampler=s, lights=l) for p in ("wavefront", "stream", "megakernel") for s in (None, "sobol") for l in (False, True)]
    return [dict(lights=False), dict(lights=True)]


# ---- equivalence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PAIR_NAMES)
def test_updated_scene_equals_fresh_scene(pairs, name):
    a0, a1, opt = pairs[name]
    try:
        if "budget" in opt:
            set_texture_interleave_budget(opt["budget"])
        A, B = Scene(a0), Scene(a1)
        try:
            update(A, a1, uv=opt.get("uv", True))
            assert_same_scene(A, B, product(name))
            if name == "budget_0":
                assert (A.read_appearance("tex_sets").view(np.uint32)[0::12] != AC.TEXSET_QUAD).all() and A.read_appearance("atlas4").size == 0
            if name == "set_forms":
                assert sorted(set(A.read_appearance("tex_sets").view(np.uint32)[0::12].tolist())) == [0, 1, 2]
        finally:
            A.close(); B.close()
    finally:
        set_texture_interleave_budget(AC.DEFAULT_BUDGET)


def test_emissive_layer_switches_the_light_table(pairs):
    dark, lit, _ = pairs["emissive_on"]
    sc = Scene(dark)
    pt = make_pt(sc, lights=True)
    assert sc.light_count() == 0
    update(sc, lit)
    n = sc.light_count()
    assert n > 0
    pt.render(2)
    assert pt.readRadiance()[..., :3].max() > 0
    update(sc, dark, atlas=False)
    assert sc.light_count() == 0
    update(sc, lit, atlas=False)
    assert sc.light_count() == n
    pt.close(); sc.close()


def test_dielectric_flip_on_the_stream_scheduler(pairs):
    """has_dielectric sets the stream scheduler's horizon at every launch: a target that has RUN under the other value must
    render like a fresh one"""
    e3, off, _ = pairs["e3_dielectric_off"]
    for a0, a1 in ((e3, off), (off, e3)):
        A = Scene(a0)
        pt = make_pt(A, pipeline="stream")
        pt.render(TICKS)
        update(A, a1)
        pt.clear(); pt.seed(7); pt.render(TICKS)
        got = pt.readRadiance().view(np.uint32)
        pt.close()
        B = Scene(a1)
        assert np.array_equal(got, frame(B, pipeline="stream"))
        assert np.array_equal(got, frame(B, pipeline="wavefront"))
        A.close(); B.close()


# ---- uv and atlas arguments ------------------------------------------------------------------------------------------
def test_uv_and_atlas_arguments(pairs):
    t, a1, _ = pairs["res_9"]
    sc = Scene(t)
    with pytest.raises(FsptError) as e:
        sc.update_materials(t.mat)  # never updated: there is no retained atlas
    assert e.value.code == -6
    assert sc.last_appearance()["retained"] == 0
    sc.update_materials(a1.mat, None, a1.atlas, a1.atlas_res, a1.atlas_layers)  # uv None keeps the uvs
    kept = dataclasses.replace(a1, uv=t.uv)
    B = Scene(kept)
    assert_same_scene(sc, B, [dict()])
    B.close()
    assert sc.last_appearance()["retained"] == a1.atlas.size
    # a second update without an atlas lays the retained one out again, under other ids and uvs
    a2 = dataclasses.replace(a1, mat=AC.retex(t, 9, 5, 77).mat, uv=a1.uv)
    sc.update_materials(a2.mat, a2.uv)
    last = sc.last_appearance()
    assert last["retained"] == a1.atlas.size and last["uploaded"] < a1.atlas.size + t.n_tris * 80
    B = Scene(a2)
    assert_same_scene(sc, B, [dict()])
    B.close(); sc.close()


# ---- environment -----------------------------------------------------------------------------------------------------
def test_environment_there_and_back(bases):
    small = bases["small"]
    none = AC.with_env(small, None, None, 0)
    sc = Scene(small)
    f0 = frame(sc)
    for a in (none, AC.with_env(small, 15, 7, 3), small):
        sc.update_environment(a.env, a.env_w, a.env_h, a.bins)
        B = Scene(a)
        assert_same_scene(sc, B, [dict()])
        B.close()
    assert np.array_equal(frame(sc), f0)
    sc.close()


# ---- composition with the geometry updates ---------------------------------------------------------------------------
def hitrec(sc):
    return sc.read_appearance("hitrec")


def test_composes_with_refit_and_rebuild(bases):
    import refit_ref as R
    t = bases["textured"]
    a1 = AC.retex(t, 9, 5, 81, new_uv=True)
    tri, norm = rotated(t.tri, t.norm)
    moved = lambda a: dataclasses.replace(a, tri=tri, norm=norm, bvh=R.refit(a.bvh, tri))
    # materials after a refit, and a refit after materials
    for first in ("geometry", "materials"):
        A = Scene(t)
        for step in (("geometry", "materials") if first == "geometry" else ("materials", "geometry")):
            if step == "geometry":
                A.update_geometry(tri, norm)
            else:
                update(A, a1)
        B = Scene(moved(a1))
        assert np.array_equal(hitrec(A), hitrec(B)), first
        assert_same_scene(A, B, [dict(), dict(lights=True)])
        A.close(); B.close()
    # materials after a rebuild: mat / uv in the composed order
    A = Scene(t)
    order = A.rebuild_geometry(tri, norm)
    A.update_materials(a1.mat.reshape(-1, 12)[order], a1.uv.reshape(-1, 6)[order], a1.atlas, a1.atlas_res, a1.atlas_layers)
    slot = A.slot_triangles()
    rec = hitrec(A).view(np.float32).reshape(-1, 48)
    live = slot < t.n_tris
    assert np.array_equal(rec[live, 36:42].view(np.uint32), a1.uv.reshape(-1, 6)[order][slot[live]].view(np.uint32))
    assert np.array_equal(rec[live, 46:48].view(np.uint32), a1.mat.reshape(-1, 12)[order][slot[live]][:, 9:11].view(np.uint32))
    assert not rec[~live].view(np.uint32).any()
    # ... and the other order of the two calls gives the same scene: materials first, then the rebuild (which carries the
    # material part of every record to its new slot)
    C2 = Scene(t)
    update(C2, a1)
    assert np.array_equal(order, C2.rebuild_geometry(tri, norm))
    A.update_environment(a1.env, a1.env_w, a1.env_h, a1.bins)
    ra, rc = hitrec(A).view(np.uint32).reshape(-1, 48), hitrec(C2).view(np.uint32).reshape(-1, 48)
    assert np.array_equal(np.delete(ra, 42, 1), np.delete(rc, 42, 1))  # (word 42, the set id, is numbered by first appearance in each order)
    for kw in (dict(), dict(lights=True)):
        assert np.array_equal(frame(A, **kw), frame(C2, **kw)), kw
    A.close(); C2.close()


def test_fuzz_padding_slots_stay_zero(pairs):
    a0, a1, _ = pairs["fuzz_leaf5"]
    sc = Scene(a0)
    update(sc, a1)
    slot = sc.slot_triangles()
    rec = hitrec(sc).view(np.uint32).reshape(-1, 48)
    assert (slot >= a0.n_tris).any() and not rec[slot >= a0.n_tris].any()
    sc.close()


# ---- per-target state survives ---------------------------------------------------------------------------------------
def test_target_state_survives(bases):
    small = bases["small"]
    other = AC.with_env(small, 64, 32, 5)
    out = {}
    for how in ("identity", "other", "other_reset"):
        sc = Scene(small)
        pt = make_pt(sc)
        pt.set_auto_exposure(True, adapt_up=0.5, adapt_down=0.5)
        pt.render(TICKS)
        pt.temporal_accumulate(read=False)
        pt.draw()
        n0 = pt.exposure()[2]
        a = small if how == "identity" else other
        sc.update_environment(a.env, a.env_w, a.env_h, a.bins)
        if how == "other_reset":
            pt.exposure_reset()
        pt.clear(); pt.render(TICKS)
        hist = pt.temporal_accumulate()
        pt.draw()
        out[how] = (hist, n0, pt.exposure())
        pt.close(); sc.close()
    (hi, n0i, ei), (ho, n0o, eo), (_, _, er) = out["identity"], out["other"], out["other_reset"]
    assert np.array_equal(hi[..., 3].view(np.uint32), ho[..., 3].view(np.uint32))  # reprojection reads geometry only
    assert (hi[..., 3] > 1).any() and ((ho[..., 3] > 1) == (hi[..., 3] > 1)).all()  # the history was kept, not restarted
    assert not np.array_equal(hi[..., :3], ho[..., :3])
    # the exposure kept metering and ADAPTED from its state: a reset before the second frame gives another value
    assert n0i == n0o > 0 and eo[2] > 0 and er[2] == eo[2]
    assert eo[0] != er[0]


# ---- ordering --------------------------------------------------------------------------------------------------------
def test_recorded_ticks_run_before_the_update(pairs):
    a0, a1, _ = pairs["res_9"]
    out = []
    for sync_first in (False, True):
        sc = Scene(a0)
        pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        update(sc, a1)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance())
        pt.close(); sc.close()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    sc = Scene(a0); pt = make_pt(sc)
    for _ in range(6):
        pt.tick()
    assert not np.array_equal(pt.readRadiance().view(np.uint32), out[0].view(np.uint32))
    pt.close(); sc.close()


def test_present_around_an_update(pairs):
    a0, a1, _ = pairs["res_9"]
    sc = Scene(a0); pt = make_pt(sc)
    ref = Scene(a0); pr = make_pt(ref)

    def ticks(n):
        for _ in range(n):
            pt.tick(); pr.tick()

    ticks(2)
    img, n = pt.present()
    assert img is None and n == 0
    pre = pr.draw()
    update(sc, a1); update(ref, a1)
    ticks(2)
    img, n = pt.present()
    assert n == 2 and np.array_equal(img, pre)        # the pre-update frame, once
    post = pr.draw()
    assert not np.array_equal(post, pre)
    ticks(1)
    img, n = pt.present()
    assert n == 4 and np.array_equal(img, post)
    pt.close(); pr.close(); sc.close(); ref.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_unchanged(pairs):
    from fspt_amd import _lib as L
    a0, a1, _ = pairs["res_9"]
    sc = Scene(a0)
    update(sc, a1)
    before, last = buffers(sc), sc.last_appearance()
    lib, h = L.lib(), sc._h
    mat, atlas, bins = L.fptr(a1.mat), L.u8ptr(a1.atlas), L.u32ptr(a1.bins)
    env = L.u8ptr(a1.env)
    calls = [lambda: lib.fspt_scene_update_materials(None, mat, None, atlas, 9, 5),
             lambda: lib.fspt_scene_update_materials(h, None, None, atlas, 9, 5),
             lambda: lib.fspt_scene_update_materials(h, mat, None, atlas, 0, 5),
             lambda: lib.fspt_scene_update_materials(h, mat, None, atlas, 9, 0),
             lambda: lib.fspt_scene_update_environment(None, env, a1.env_w, a1.env_h, bins, 1),
             lambda: lib.fspt_scene_update_environment(h, env, 0, a1.env_h, bins, 1),
             lambda: lib.fspt_scene_update_environment(h, env, a1.env_w, 0, bins, 1),
             lambda: lib.fspt_scene_update_environment(h, env, a1.env_w, a1.env_h, None, 1),
             lambda: lib.fspt_scene_update_environment(h, env, a1.env_w, a1.env_h, bins, 0)]
    for k, call in enumerate(calls):
        assert call() == -1, k
    after, now = buffers(sc), sc.last_appearance()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert {k: now[k] for k in ("launches", "uploaded", "retained")} == {k: last[k] for k in ("launches", "uploaded", "retained")}
    assert now["ms"] in (0.0, last["ms"])
    # the messages of fspt_scene_create where the condition is the same
    lib.fspt_scene_update_materials(h, mat, None, atlas, 0, 5)
    assert "atlas must have at least one layer" in lib.fspt_last_error().decode()
    lib.fspt_scene_update_environment(h, env, 0, 4, bins, 1)
    assert "env given with zero size" in lib.fspt_last_error().decode()
    lib.fspt_scene_update_environment(h, env, 8, 4, bins, 0)
    assert "radianceBins must hold at least one bin" in lib.fspt_last_error().decode()
    sc.close()


def test_never_updated_scene_retains_nothing(bases):
    sc = Scene(bases["textured"])
    frame(sc)
    assert sc.last_appearance() == dict(ms=0.0, launches=0, uploaded=0, retained=0)
    sc.close()


# ---- several devices -------------------------------------------------------------------------------------------------
def test_multi_update_equals_single_scene(pairs):
    a0, a1, _ = pairs["res_9"]
    m = MultiPathTracer(a0, W, H, devices=(0,), num_bounces=4)
    m.set_camera(**CAM); m.seed(7)
    m.render(2)
    m.update_materials(a1.mat, a1.uv, a1.atlas, a1.atlas_res, a1.atlas_layers)
    m.update_environment(a1.env, a1.env_w, a1.env_h, a1.bins)
    m.clear(); m.seed(7); m.render(TICKS)
    got = m.readRadiance().view(np.uint32)
    m.close()
    B = Scene(a1)
    assert np.array_equal(got, frame(B))
    B.close()


# ---- sequences -------------------------------------------------------------------------------------------------------
def _write_frames(tmp_path, n_frames):
    """scene files of a glowing cube-sphere that moves over a quad: the ball's kem changes in frame 1 (and stays), an
    environment map appears in frame 2"""
    from PIL import Image
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir(); (root / "env").mkdir()
    for k, kem in enumerate(("0.9 0.7 0.5", "0.2 0.9 0.3")):
        (root / "mesh" / f"ball{k}.obj").write_text(f"mtllib ball{k}.mtl\nusemtl glow\n" + S.cube_sphere_obj(4))
        (root / "mesh" / f"ball{k}.mtl").write_text(f"newmtl glow\nkd 0.8 0.3 0.2\nkem {kem}\n")
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    env, w, h = S.synthetic_env(16, 8)
    Image.fromarray(np.asarray(env, np.uint8).reshape(h, w, 4), mode="RGBA").save(str(root / "env" / "sky.png"))
    for f in range(n_frames):
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 4, "exposure": 1.2,
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6],
                                   "emittance": [0, 0, 0]}],
                 "animated_props": [{"path": f"mesh/ball{min(f, 1)}.obj", "scale": 0.4, "translate": [-0.4 + 0.4 * f, 0.05 * f, 0.0],
                                     "rotate": [{"axis": [0, 1, 0], "angle": 0.3 * f}], "diffuse": [0.8, 0.3, 0.2],
                                     "emittance": [3, 3, 3], "normals": "smooth"}]}
        if f >= 2:
            scene["environment"] = "env/sky.png"
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def test_render_sequence_appearance(tmp_path):
    from fspt_amd import scene_file as F
    pattern, root = _write_frames(tmp_path, 3)
    logs, runs = {}, {}
    for mode, kw in (("refit", {}), ("sah", {}), ("temporal", dict(temporal=True))):
        log = []
        runs[mode] = F.render_sequence(pattern, range(3), str(tmp_path / mode / "{frame}.png"), W, H, root,
                                       bvh="sah" if mode == "sah" else "refit", samples=4, on_frame=lambda f, how: log.append(how), **kw)
        logs[mode] = log
    assert logs["refit"] == ["build", "appearance", "appearance"] == logs["temporal"]
    assert logs["sah"] == ["build"] * 3
    for a, b in zip(runs["refit"], runs["sah"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    # the temporal run used its history: its frame 2 differs from frame 2 of a run whose frames are built one by one (frame k
    # renders with seed + k, so that run's frame 2 gets seed 3), which has no history
    alone = F.render_sequence(pattern, [2], str(tmp_path / "alone" / "{frame}.png"), W, H, root, bvh="refit", samples=4, temporal=True, seed=3)
    assert open(runs["temporal"][2], "rb").read() != open(alone[0], "rb").read()


# ---- the Node host ---------------------------------------------------------------------------------------------------
def test_node_updates_match_python(pairs, tmp_path):
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    a0, a1, _ = pairs["res_9"]
    B = Scene(a1)
    want = frame(B, n=6)
    B.close()
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins", "env"):
        getattr(a0, k).tofile(os.path.join(d, k + ".bin"))
    for k in ("mat", "uv", "atlas", "bins", "env"):
        getattr(a1, k).tofile(os.path.join(d, k + "2.bin"))
    meta = dict(atlasRes=a0.atlas_res, atlasLayers=a0.atlas_layers, envW=a0.env_w, envH=a0.env_h, leafSize=a0.leaf_size, W=W, H=H, n=6,
                atlasRes2=a1.atlas_res, atlasLayers2=a1.atlas_layers, envW2=a1.env_w, envH2=a1.env_h, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "appearance_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.uint32).reshape(H, W, 4)
    assert np.array_equal(got, want)
