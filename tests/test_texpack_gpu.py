"""The GPU texture packer on the MI355X.  No tolerance anywhere: k_tex_resample's raw atlas must be the numpy
restatement of the arithmetic contract (tests/texpack_ref.py) byte for byte, and a scene whose textures were packed on the
device - whole or layer by layer - must be indistinguishable from a scene created from the restatement's atlas: in the six
buffers an appearance update writes, in the light table and in rendered frames."""
import ctypes as C
import dataclasses
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import appearance_cases as AC
import texpack_ref as R
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S
from refit_moves import rotated

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 96, 64, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KWS = [dict(pipeline=p, lights=l) for p in ("wavefront", "megakernel") for l in (False, True)]


@pytest.fixture(scope="module")
def textured():
    return S.textured_test_scene(16)


@pytest.fixture(scope="module")
def sources():
    return [R.source(w, h) for w, h in R.SOURCE_SHAPES]


# ---- fspt_atlas_pack_gpu against the restatement -----------------------------------------------------------------------
def all_flags_desc(sources, res):
    """every source under every swizzle, corrected and not: 72 layers"""
    layers = [R.image_layer(i, c, sw) for i in range(len(sources)) for sw in R.SWIZZLES for c in (False, True)]
    return {"res": res, "images": sources, "layers": layers}


def assert_pack(desc):
    got, want = S.atlas_pack_gpu(desc, 0), R.pack(desc)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        per = desc["res"] ** 2 * 4
        bad = sorted(set((np.nonzero(got != want)[0] // per).tolist()))
        raise AssertionError(f"res {desc['res']}: {int((got != want).sum())} bytes differ, in layers {bad[:12]}: {[desc['layers'][l] for l in bad[:3]]}")


@pytest.mark.parametrize("res", R.RESOLUTIONS)
def test_pack_equals_restatement(sources, res):
    assert_pack(all_flags_desc(sources, res))


def test_pack_equals_restatement_at_512(sources):
    """more than one block row per layer and a grid-stride: 262 144 texels, magnified and minified"""
    d = {"res": 512, "images": sources, "layers": [R.image_layer(8, True, (0, 2, 1, 3)), R.image_layer(7, False), R.image_layer(0, True),
                                                    R.image_layer(2, False, (3, 2, 1, 0)), {"kind": "color", "color": [0.25, 0.5, 0.75]}]}
    assert_pack(d)


def test_pack_layer_mixes(sources):
    cols = [[-0.25, 1.5, 0.5], [0.5 / 255, 1.5 / 255, 2.5 / 255], [127.5 / 255, 254.5 / 255, 0.0], [1.0, 0.999, 0.7]]
    res = 9
    px = np.random.default_rng(3).integers(0, 256, (res, res, 4), dtype=np.uint8)
    images = sources + [px]
    mixed = [{"kind": "color", "color": cols[0]}, R.image_layer(4, True), {"kind": "pixels", "image": len(sources)}, R.image_layer(4, False, (1, 1, 1, 1)),
             {"kind": "color", "color": cols[1]}, {"kind": "color", "color": cols[2]}, R.image_layer(8, True, (3, 2, 1, 0)), {"kind": "color", "color": cols[3]}]
    assert_pack({"res": res, "images": images, "layers": mixed})
    assert_pack({"res": res, "images": images, "layers": [mixed[2]]})            # a single copied layer
    assert_pack({"res": res, "images": images, "layers": [mixed[6]]})            # a single resampled layer
    assert_pack({"res": 1, "images": [], "layers": [mixed[4]]})                  # a colours-only atlas
    assert_pack({"res": 5, "images": images, "layers": [mixed[k % 8] if k % 8 != 2 else mixed[1] for k in range(40)]})  # 40 layers
    # colours agree with TexturePacker.get_pixels, which quantises them in float64
    p = S.TexturePacker(4)
    for c in cols + [[k * 0.5 / 255] * 3 for k in range(1, 40, 2)]:
        p.add_color(c)
    assert np.array_equal(p.get_pixels(device=0), p.get_pixels())
    t = S.atlas_pack_last_ms()
    assert t["kernel_ms"] > 0 and t["upload_ms"] >= 0 and t["readback_ms"] >= 0


# ---- build_scene(textures="gpu") ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [16, 33])
def test_build_scene_gpu_atlas(res):
    cpu, gpu = S.textured_test_scene(res), S.textured_test_scene(res, textures="gpu")
    assert gpu.atlas_res == cpu.atlas_res == res and gpu.atlas_layers == cpu.atlas_layers
    desc = gpu.meta["packer"].pack_desc()
    assert np.array_equal(gpu.atlas, R.pack(desc))                                # every layer: through the restatement
    a, b = cpu.atlas.reshape(cpu.atlas_layers, -1), gpu.atlas.reshape(cpu.atlas_layers, -1)
    plain = [l for l, y in enumerate(desc["layers"]) if not y.get("corrected")]
    assert 0 < len(plain) < len(desc["layers"])                                   # the diffuse map is sRGB-corrected
    for l in plain:
        assert np.array_equal(a[l], b[l]), l                                      # uncorrected sources and colours: the default's bytes
    for f in ("bvh", "tri", "mat", "norm", "uv", "bins"):
        assert np.array_equal(getattr(cpu, f).view(np.uint32), getattr(gpu, f).view(np.uint32)), f  # (bvh holds integer words)


# ---- a scene updated from sources against a fresh scene ----------------------------------------------------------------
def make_pt(sc, pipeline="wavefront", lights=False, seed=7):
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if lights:
        pt.set_lights("emitters", 0.5)
    return pt


def frame(sc, n=TICKS, **kw):
    pt = make_pt(sc, **kw)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img.view(np.uint32)


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


def random_desc(res, layers, seed, const=(0,), flat=()):
    """a description of `layers` layers: those in `const` flat colours, those in `flat` images of one texel (the resample of
    a 1 x 1 source is a constant layer), the others images of assorted shapes and flags"""
    rng = np.random.default_rng(seed)
    shapes = [(7, 5), (16, 16), (3, 9), (33, 17), (2, 2)]
    images, out = [], []
    for l in range(layers):
        if l in const:
            out.append({"kind": "color", "color": rng.uniform(-0.1, 1.1, 3).tolist()})
            continue
        w, h = (1, 1) if l in flat else shapes[(l + seed) % len(shapes)]
        images.append(R.source(w, h, seed=seed * 31 + l))
        out.append(R.image_layer(len(images) - 1, bool((l + seed) % 2), R.SWIZZLES[(l + seed) % 3]))
    return {"res": res, "images": images, "layers": out}


def arrays_of(t, desc, seed, table=None, new_uv=True):
    """`t` with layer ids for desc's layers and the restatement's atlas of desc"""
    a = AC.retex(t, desc["res"], len(desc["layers"]), seed, table=table, new_uv=new_uv)
    return dataclasses.replace(a, atlas=R.pack(desc))


@pytest.mark.parametrize("res", [16, 9, 5, 1])
def test_update_textures_equals_fresh_scene(textured, res):
    desc = random_desc(res, 5, res)
    a1 = arrays_of(textured, desc, res)
    A, B = Scene(textured), Scene(a1)
    try:
        A.update_textures(a1.mat, a1.uv, desc)
        assert_same_scene(A, B, KWS)
        last = A.last_appearance()
        src = sum(im.size for im in desc["images"])
        assert last["retained"] == a1.atlas.size
        assert src <= last["uploaded"] <= src + 32 * 5 + textured.n_tris * 80 + 48 * 64  # the sources, the records, mat | set | uv, the set table
    finally:
        A.close(); B.close()


def test_atlas_shape_changes_across_updates(textured):
    """res 16 -> 9 -> 16, a layer that turns constant and back, under the same ids"""
    tab = [[1, 0, 2, 1], [1, 1, 1, 1], [2, 1, 0, 0]]
    steps = [random_desc(9, 3, 21), random_desc(9, 3, 21, flat=(1,)), random_desc(9, 3, 21), random_desc(16, 3, 22)]
    A = Scene(textured)
    pt = make_pt(A)
    pt.render(2)
    try:
        for k, desc in enumerate(steps):
            a = arrays_of(textured, desc, 21, table=tab)
            A.update_textures(a.mat, a.uv, desc)
            B = Scene(a)
            assert_same_scene(A, B, KWS[:2])
            B.close()
            kinds = A.read_appearance("tex_sets").view(np.uint32)[0::12].tolist()
            if k == 1:
                assert kinds[1] == AC.TEXSET_CONST, kinds   # the set of layer 1 alone
            else:
                assert kinds[1] != AC.TEXSET_CONST, kinds
    finally:
        pt.close(); A.close()


def test_emissive_layer_switches_the_light_table(textured):
    desc = random_desc(8, 3, 60)
    desc["layers"][0] = {"kind": "color", "color": [0.0, 0.0, 0.0]}
    dark = arrays_of(textured, desc, 60, table=[[1, 0, 2, 1]])
    lit = dataclasses.replace(dark, mat=dark.mat.copy())
    lit.mat.reshape(-1, 12)[: textured.n_tris // 2, AC.MAT_EMISSIVE] = 1
    sc = Scene(textured)
    pt = make_pt(sc, lights=True)
    try:
        sc.update_textures(dark.mat, dark.uv, desc)
        assert sc.light_count() == 0
        sc.update_textures(lit.mat, lit.uv, desc)
        n = sc.light_count()
        assert n > 0
        B = Scene(lit)
        assert_same_scene(sc, B, [dict(lights=True)])
        B.close()
        pt.render(2)
        assert pt.readRadiance()[..., :3].max() > 0
        sc.update_textures(dark.mat, dark.uv, desc)
        assert sc.light_count() == 0
    finally:
        pt.close(); sc.close()


# ---- patches -----------------------------------------------------------------------------------------------------------
def patched(desc, ids, layers, images):
    """desc with layers[k] (indexing `images`) in place of layer ids[k]"""
    out = {"res": desc["res"], "images": list(desc["images"]) + list(images), "layers": list(desc["layers"])}
    for i, y in zip(ids, layers):
        out["layers"][i] = dict(y, image=y["image"] + len(desc["images"])) if "image" in y else y
    return out


def patch_cases(res):
    one = ([2], [R.image_layer(0, True, (0, 2, 1, 3))], [R.source(11, 6, seed=5)])
    px = np.random.default_rng(9).integers(0, 256, (res, res, 4), dtype=np.uint8); px[..., 3] = 255
    three = ([4, 0, 1], [{"kind": "color", "color": [0.9, 0.2, 0.4]}, R.image_layer(0, False), {"kind": "pixels", "image": 1}], [R.source(5, 5, seed=6), px])
    return {"one": one, "three": three}


@pytest.mark.parametrize("which", ["one", "three"])
def test_patch_equals_full_update(textured, which):
    res = 9
    desc = random_desc(res, 5, 33)
    a = arrays_of(textured, desc, 33)
    ids, layers, images = patch_cases(res)[which]
    full = patched(desc, ids, layers, images)
    A, B = Scene(textured), Scene(textured)
    try:
        A.update_textures(a.mat, a.uv, desc)
        A.patch_textures(ids, layers, images)
        B.update_textures(a.mat, a.uv, full)
        assert_same_scene(A, B, KWS[:2])
        assert A.last_appearance()["uploaded"] < B.last_appearance()["uploaded"]  # the patch's sources, not the description's
        fresh = Scene(dataclasses.replace(a, atlas=R.pack(full)))
        assert_same_scene(A, fresh, [dict()])
        fresh.close()
        # a later update without an atlas lays the PATCHED atlas out again
        a2 = AC.retex(textured, res, 5, 77)
        A.update_materials(a2.mat, None)
        C2 = Scene(dataclasses.replace(a2, atlas=R.pack(full), uv=a.uv))
        assert_same_scene(A, C2, [dict()])
        C2.close()
    finally:
        A.close(); B.close()


def test_patch_needs_a_retained_atlas(textured):
    sc = Scene(textured)
    try:
        with pytest.raises(FsptError) as e:
            sc.patch_textures([0], [{"kind": "color", "color": [1, 0, 0]}], [], res=16)
        assert e.value.code == -6
        assert sc.last_appearance() == dict(ms=0.0, launches=0, uploaded=0, retained=0)
    finally:
        sc.close()


def test_patch_composes_with_refit_and_rebuild(textured):
    t, res = textured, 9
    desc = random_desc(res, 5, 41)
    a = arrays_of(t, desc, 41)
    ids, layers, images = patch_cases(res)["three"]
    full = patched(desc, ids, layers, images)
    tri, norm = rotated(t.tri, t.norm)
    for geometry in ("refit", "rebuild"):
        for first in ("geometry", "patch"):
            A, B = Scene(t), Scene(t)
            try:
                A.update_textures(a.mat, a.uv, desc)
                order = np.arange(t.n_tris)
                for step in (("geometry", "patch") if first == "geometry" else ("patch", "geometry")):
                    if step == "patch":
                        A.patch_textures(ids, layers, images)
                    elif geometry == "refit":
                        A.update_geometry(tri, norm)
                    else:
                        order = A.rebuild_geometry(tri, norm)
                # B: the same geometry call, then one full update in the resulting leaf order
                if geometry == "refit":
                    B.update_geometry(tri, norm)
                else:
                    assert np.array_equal(order, B.rebuild_geometry(tri, norm))
                B.update_textures(a.mat.reshape(-1, 12)[order], a.uv.reshape(-1, 6)[order], full)
                if geometry == "rebuild" and first == "patch":
                    # (the set ids were numbered in the old leaf order: everything but word 42 of the records and the order of
                    # the table's rows is pinned by the frames)
                    for kw in KWS[:2]:
                        assert np.array_equal(frame(A, **kw), frame(B, **kw)), (geometry, first, kw)
                else:
                    assert_same_scene(A, B, KWS[:2])
            finally:
                A.close(); B.close()


# ---- device forms ------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_host_form(textured):
    import torch
    res = 9
    desc = random_desc(res, 5, 51)
    a = arrays_of(textured, desc, 51)
    ids, layers, images = patch_cases(res)["three"]
    dev = lambda ims: [torch.from_numpy(np.ascontiguousarray(im)).to("cuda:0") for im in ims]
    A, B = Scene(textured), Scene(textured)
    try:
        A.update_textures(a.mat, a.uv, dict(desc, images=dev(desc["images"])))
        B.update_textures(a.mat, a.uv, desc)
        assert_same_scene(A, B, [dict()])
        assert A.last_appearance()["uploaded"] < B.last_appearance()["uploaded"] - sum(im.size for im in desc["images"]) + 1
        A.patch_textures(ids, layers, dev(images))
        B.patch_textures(ids, layers, images)
        assert_same_scene(A, B, [dict()])
        with pytest.raises(TypeError, match="all host arrays or all device tensors"):
            A.patch_textures(ids, layers, [dev(images)[0], images[1]])
        # a source that is not 4-byte aligned is refused on the host
        p, _, _, keep = S.texture_pack_struct(dict(desc, images=dev(desc["images"])), 0)
        p.images[0].rgba = p.images[0].rgba + 1
        assert L.lib().fspt_scene_update_textures_device(A._h, L.fptr(a.mat), None, C.byref(p)) == -1
        assert b"4-byte aligned" in L.lib().fspt_last_error()
        assert_same_scene(A, B, [])
    finally:
        A.close(); B.close()


# ---- refused calls, accounting, memory ---------------------------------------------------------------------------------
def test_refused_calls_leave_the_scene_unchanged(textured):
    INVALID, good_desc = R.INVALID, R.good_desc
    res = 4
    desc = random_desc(res, 5, 61)
    a = arrays_of(textured, desc, 61)
    sc = Scene(textured)
    try:
        sc.update_textures(a.mat, a.uv, desc)
        before, last = buffers(sc), sc.last_appearance()
        lib, h, mat = L.lib(), sc._h, L.fptr(a.mat)
        ids = np.array([0, 1, 2], np.uint32)
        for name in sorted(INVALID):
            p, _, _, keep = S.texture_pack_struct(good_desc(res))
            INVALID[name](p)
            assert lib.fspt_scene_update_textures(h, mat, None, C.byref(p)) == -1, name
            assert lib.fspt_scene_patch_textures(h, L.u32ptr(ids), p.n_layers, C.byref(p)) == -1, name
        p, _, _, keep = S.texture_pack_struct(good_desc(res))
        assert lib.fspt_scene_update_textures(h, None, None, C.byref(p)) == -1                         # NULL mat
        assert lib.fspt_scene_update_textures(h, mat, None, None) == -1
        assert lib.fspt_scene_patch_textures(h, None, 3, C.byref(p)) == -1
        assert lib.fspt_scene_patch_textures(h, L.u32ptr(ids), 2, C.byref(p)) == -1
        assert lib.fspt_scene_patch_textures(h, L.u32ptr(np.array([0, 5, 2], np.uint32)), 3, C.byref(p)) == -1   # the atlas has layers 0..4
        assert lib.fspt_scene_patch_textures(h, L.u32ptr(np.array([3, 1, 3], np.uint32)), 3, C.byref(p)) == -1   # twice
        p8, _, _, keep8 = S.texture_pack_struct(good_desc(8))
        assert lib.fspt_scene_patch_textures(h, L.u32ptr(ids), 3, C.byref(p8)) == -1                   # res is the retained atlas's
        after, now = buffers(sc), sc.last_appearance()
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert now == last
        assert now["retained"] == res * res * 5 * 4
        assert lib.fspt_scene_patch_textures(h, L.u32ptr(ids), 3, C.byref(p)) == 0                     # ... and the good call goes through
        assert sc.last_appearance()["retained"] == res * res * 5 * 4
    finally:
        sc.close()


def test_updates_do_not_grow_memory(textured):
    lib = L.lib()

    def free():
        f, t = C.c_uint64(), C.c_uint64()
        L.check(lib.fspt_device_memory(0, C.byref(f), C.byref(t)))
        return int(f.value)

    descs = [random_desc(16, 5, 71), random_desc(9, 4, 72)]
    arrs = [arrays_of(textured, d, 71 + k) for k, d in enumerate(descs)]
    sc = Scene(textured)
    try:
        for k in range(4):  # (the first calls make the events and the allocator's pools)
            sc.update_textures(arrs[k % 2].mat, arrs[k % 2].uv, descs[k % 2])
            sc.patch_textures([1], [{"kind": "color", "color": [0.1, 0.2, 0.3]}], [])
        f0 = free()
        for k in range(20):
            sc.update_textures(arrs[k % 2].mat, arrs[k % 2].uv, descs[k % 2])
            sc.patch_textures([1], [{"kind": "color", "color": [0.1, 0.2, 0.3]}], [])
        assert free() >= f0 - (1 << 20), (f0, free())
    finally:
        sc.close()


# ---- hosts -------------------------------------------------------------------------------------------------------------
def test_multi_update_equals_single_scene(textured):
    res = 9
    desc = random_desc(res, 5, 81)
    a = arrays_of(textured, desc, 81)
    ids, layers, images = patch_cases(res)["one"]
    m = MultiPathTracer(textured, W, H, devices=(0,), num_bounces=4)
    try:
        m.set_camera(**CAM); m.seed(7)
        m.render(2)
        m.update_textures(a.mat, a.uv, desc)
        m.patch_textures(ids, layers, images)
        m.clear(); m.seed(7); m.render(TICKS)
        got = m.readRadiance().view(np.uint32)
    finally:
        m.close()
    B = Scene(dataclasses.replace(a, atlas=R.pack(patched(desc, ids, layers, images))))
    try:
        assert np.array_equal(got, frame(B))
    finally:
        B.close()


def test_node_host_matches_python(textured, tmp_path):
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node / the addon not available")
    res = 9
    desc = random_desc(res, 5, 91)
    a = arrays_of(textured, desc, 91)
    ids, layers, images = patch_cases(res)["three"]
    full = patched(desc, ids, layers, images)
    B = Scene(a); want = frame(B, n=6); B.close()
    B = Scene(dataclasses.replace(a, atlas=R.pack(full))); want2 = frame(B, n=6); B.close()
    d = str(tmp_path)
    t = textured
    for k in ("bvh", "tri", "mat", "norm", "uv", "bins", "env"):
        getattr(t, k).tofile(os.path.join(d, k + ".bin"))
    t.atlas.tofile(os.path.join(d, "atlas0.bin")); a.mat.tofile(os.path.join(d, "mat1.bin")); a.uv.tofile(os.path.join(d, "uv1.bin"))

    def dump(ims, tag):
        out = []
        for i, im in enumerate(ims):
            np.ascontiguousarray(im).tofile(os.path.join(d, f"{tag}{i}.bin"))
            out.append(dict(file=f"{tag}{i}", w=int(im.shape[1]), h=int(im.shape[0])))
        return out

    js_layers = lambda ls: [dict(y, swizzle=list(y["swizzle"])) if "swizzle" in y else y for y in ls]
    meta = dict(atlasRes=t.atlas_res, atlasLayers=t.atlas_layers, envW=t.env_w, envH=t.env_h, leafSize=t.leaf_size, W=W, H=H, n=6, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]),
                textures=dict(res=res, images=dump(desc["images"], "img"), layers=js_layers(desc["layers"])),
                patch=dict(ids=[int(i) for i in ids], layers=js_layers(layers), images=dump(images, "pimg")))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "texpack_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d], timeout=300)
    assert np.array_equal(np.fromfile(os.path.join(d, "atlas.bin"), np.uint8), a.atlas)
    assert np.array_equal(np.fromfile(os.path.join(d, "out.bin"), np.uint32).reshape(H, W, 4), want)
    assert np.array_equal(np.fromfile(os.path.join(d, "out2.bin"), np.uint32).reshape(H, W, 4), want2)


def _write_frames(tmp_path):
    """three scene files of an image-mapped quad under a moving ball; the middle frame names another metallic-roughness map
    (uncorrected sources only: the two packers then give the same bytes)"""
    from PIL import Image
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir(); (root / "tex").mkdir()
    (root / "mesh" / "quad.obj").write_text(S.QUAD_OBJ)
    (root / "mesh" / "ball.obj").write_text("mtllib ball.mtl\nusemtl glow\n" + S.cube_sphere_obj(4))
    (root / "mesh" / "ball.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")
    rng = np.random.default_rng(4)
    for name, shape in (("mr0", (12, 12)), ("mr1", (7, 12)), ("nrm", (12, 9))):
        im = rng.integers(0, 256, shape + (4,), dtype=np.uint8); im[..., 3] = 255
        if name == "nrm":
            im[..., :2] = 118 + im[..., :2] // 12; im[..., 2] = 240
        Image.fromarray(im, mode="RGBA").save(str(root / "tex" / f"{name}.png"))
    for f in range(3):
        scene = {"cameraPos": [0.0, 0.6, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 4, "exposure": 1.2, "atlasRes": 16,
                 "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6], "emittance": [0, 0, 0],
                                   "metallicRoughness": f"tex/mr{f % 2}.png", "normal": "tex/nrm.png", "normals": "flat"}],
                 "animated_props": [{"path": "mesh/ball.obj", "scale": 0.4, "translate": [-0.4 + 0.4 * f, 0.05 * f, 0.0], "diffuse": [0.8, 0.3, 0.2],
                                     "emittance": [2, 2, 2], "normals": "smooth"}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return root


def test_render_sequence_gpu_textures(tmp_path):
    from fspt_amd import scene_file as F
    root = _write_frames(tmp_path)
    out = {}
    for tex in ("cpu", "gpu"):
        how = []
        files = F.render_sequence(str(root / "scene" / "anim_{frame}.json"), range(3), str(tmp_path / tex / "{frame}.png"), W, H, str(root),
                                  bvh="refit", textures=tex, samples=4, on_frame=lambda n, h: how.append(h))
        assert how == ["build", "appearance", "appearance"], how
        out[tex] = [open(f, "rb").read() for f in files]
    assert out["cpu"] == out["gpu"]
    assert len(set(out["gpu"])) == 3 and min(len(x) for x in out["gpu"]) > 1000   # three different pictures, none of them blank
