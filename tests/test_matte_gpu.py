"""ID mattes (include/fspt.h fspt_mattes, fspt_scene_set_matte_ids, the Cryptomatte layers of fspt_draw_exr) on
the MI355X, bit for bit against tests/matte_ref.py's rank rule applied to the oracle's first-hit triangle indices - one
O.trace(first_hits=True) per value of the randBase stream, as test_denoise_gpu.py checks fspt_features - and byte for byte
against matte_ref's OpenEXR writer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import exr_ref as X
import matte_ref as M
import fspt_amd
from fspt_amd import FsptError, PathTracer, Scene, _lib as L, scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = dict(S.BUNNY_CAMERA, aperture=0.3)  # test_every_branch: chosen on the CPU - on the small scene the reference loses 387 samples, has ties and id-0 hits
EVERY_SEED, EVERY_SAMPLES = 3, 64


def make_pt(arrays, W, H, cam, aperture=None):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"] if aperture is None else aperture)
    return pt


def first_hit_indices(arrays, W, H, pt, seed, n):
    """int [H, W, n]: the oracle's first-hit triangle of every pixel for each of the n randBase values, -1 = a miss"""
    out = np.zeros((H, W, n), np.int64)
    for s, rb in enumerate(O.rand_base_stream(seed, n)):
        pos, d = O.camera(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, rb)
        acc = np.zeros((H, W, 4), np.float32)
        out[..., s] = O.trace(arrays, W, H, pos, d, 0, 0.5, pt.envTheta, 4, acc, first_hits=True).reshape(H, W)["index"]
    return out


def sample_ids(idx, ids):
    return np.where(idx >= 0, np.asarray(ids, np.uint32)[np.clip(idx, 0, None)], np.uint32(0)).astype(np.uint32)


def names_mod(n_tris, m, prefix="t"):
    """ids hash(prefix + str(k % m)) as set_matte takes them: (labels, names)"""
    return np.arange(n_tris) % m, [prefix + "%d" % k for k in range(m)]


def ids_of(labels, names):
    h = np.array([M.matte_hash(n) for n in names], np.uint32)
    return np.where(np.asarray(labels) >= 0, h[np.clip(labels, 0, None)], np.uint32(0)).astype(np.uint32)


def check_kind(pt, kind, idx, ids, lost=True):
    want_ids, want_cov, want_lost = M.rank(sample_ids(idx, ids))
    got_ids, got_cov = pt.read_mattes(kind)
    assert np.array_equal(got_ids, want_ids), int((got_ids != want_ids).any(-1).sum())
    assert np.array_equal(got_cov.view(np.uint32), want_cov.view(np.uint32))
    if lost:
        assert pt.mattes_lost(kind) == want_lost
    return want_ids, want_cov, want_lost


# ---- the pass against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "textured"])
def test_one_sample(small_scene, camera, name):
    arrays = {"small": small_scene, "textured": S.textured_test_scene()}[name]
    W, H, seed = 96, 64, 11
    pt = make_pt(arrays, W, H, camera)
    labels, names = names_mod(arrays.n_tris, 5)
    pt.scene.set_matte("object", labels, names)
    pt.mattes(1, seed)
    idx = first_hit_indices(arrays, W, H, pt, seed, 1)
    hit = idx[..., 0] >= 0
    assert 0 < hit.sum() < W * H  # hits and misses both present
    ids, cov = pt.read_mattes("object")
    assert np.array_equal(ids[..., 0][hit], ids_of(labels, names)[idx[..., 0][hit]])
    assert (cov[..., 0][hit] == 1.0).all()
    assert not ids[~hit].any() and not cov[~hit].any() and not ids[..., 1:].any() and not cov[..., 1:].any()
    assert pt.mattes_lost("object") == 0
    pt.close()


@pytest.mark.parametrize("name", ["small", "textured"])
def test_eight_samples_two_kinds_from_one_trace(small_scene, camera, name):
    arrays = {"small": small_scene, "textured": S.textured_test_scene()}[name]
    W, H, seed, n = 80, 56, 5, 8
    pt = make_pt(arrays, W, H, camera)
    lo, no = names_mod(arrays.n_tris, 5)
    lm, nm = names_mod(arrays.n_tris, 7, "m")
    pt.scene.set_matte("object", lo, no)
    pt.scene.set_matte("material", lm, nm)
    pt.mattes(n, seed)
    idx = first_hit_indices(arrays, W, H, pt, seed, n)
    _, cov, _ = check_kind(pt, "object", idx, ids_of(lo, no))
    check_kind(pt, "material", idx, ids_of(lm, nm))
    assert ((cov[..., 0] > 0) & (cov[..., 0] < 1)).any()
    pt.close()


def every_branch_reference(arrays, pt, W, H):
    labels = np.arange(arrays.n_tris)
    labels[labels % 4 == 3] = -1  # every fourth triangle has no matte
    names = ["tri%d" % k for k in range(arrays.n_tris)]
    idx = first_hit_indices(arrays, W, H, pt, EVERY_SEED, EVERY_SAMPLES)
    return labels, names, idx


def test_every_branch(small_scene):
    """15 x 17, 64 samples, an id per triangle, a lens wide enough to blur: the reference itself must show a full table with
    lost samples, a tie between two ranks and samples skipped for id 0 before the device is compared with it"""
    W, H = 15, 17
    pt = make_pt(small_scene, W, H, EVERY)
    labels, names, idx = every_branch_reference(small_scene, pt, W, H)
    ids = ids_of(labels, names)
    sid = sample_ids(idx, ids)
    want_ids, want_cov, want_lost = M.rank(sid)
    assert want_lost > 0
    assert ((want_cov[..., :-1] == want_cov[..., 1:]) & (want_cov[..., 1:] > 0)).any()  # a tie between two ranks
    assert ((idx >= 0) & (sid == 0)).any()                                              # a hit whose triangle has id 0
    pt.scene.set_matte("object", labels, names)
    pt.mattes(EVERY_SAMPLES, EVERY_SEED)
    check_kind(pt, "object", idx, ids)
    pt.close()


@pytest.mark.parametrize("W,H", [(1, 1), (15, 17), (255, 3), (257, 1), (53, 29)])
def test_shapes(small_scene, camera, W, H):
    pt = make_pt(small_scene, W, H, camera)
    lo, no = names_mod(small_scene.n_tris, 5)
    lm, nm = names_mod(small_scene.n_tris, 3, "m")
    pt.scene.set_matte("object", lo, no)
    pt.scene.set_matte("material", lm, nm)
    pt.mattes(3, 4)
    idx = first_hit_indices(small_scene, W, H, pt, 4, 3)
    check_kind(pt, "object", idx, ids_of(lo, no))
    check_kind(pt, "material", idx, ids_of(lm, nm))
    pt.close()


CHAIN_CAMERA = dict(P=[64 + 2.5, 0.05, 0.1], I=[-1.0, -0.01, -0.02], fov_scale=0.5, env_theta=1.66, focal_depth=2.0, aperture=0.02)
VARIANT_CAMERA = dict(P=[0.3, 1.2, 3.4], I=[-0.05, -0.3, -0.95], fov_scale=0.5, env_theta=1.66, focal_depth=2.0, aperture=0.02)


@pytest.mark.parametrize("case", ["chain depth 63", "gpu-built tree", "refractive"])
def test_trees(small_scene, camera, case):
    from rays import chain_scene
    from test_goldens import scene_from_golden
    if case == "chain depth 63":
        W, H, arrays, cam = 72, 40, chain_scene(64, small_scene), CHAIN_CAMERA
    elif case == "gpu-built tree":
        W, H, arrays, cam = 53, 29, S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu"), camera
    else:
        W, H, arrays, cam = 72, 40, scene_from_golden("variant"), VARIANT_CAMERA
    pt = make_pt(arrays, W, H, cam)
    labels, names = names_mod(arrays.n_tris, 11)
    pt.scene.set_matte("material", labels, names)  # (one kind, and not the first: table a holds the material ids)
    pt.mattes(3, 8)
    idx = first_hit_indices(arrays, W, H, pt, 8, 3)
    ids, _, _ = check_kind(pt, "material", idx, ids_of(labels, names))
    assert ids.any()
    with pytest.raises(FsptError) as e:
        pt.read_mattes("object")
    assert e.value.code == -6
    pt.close()


def test_camera_model(small_scene, camera):
    """equirect: per pixel the counts add up to the hits fspt_features counts for the same rays"""
    W, H, n, seed = 64, 32, 8, 6
    pt = make_pt(small_scene, W, H, camera)
    pt.set_camera_model("equirect")
    labels, names = names_mod(small_scene.n_tris, 5)
    pt.scene.set_matte("object", labels, names)
    pt.mattes(n, seed)
    pt.features(n, seed)
    _, cov = pt.read_mattes("object")
    hits = np.rint(pt.readFeatures()[..., 7].astype(np.float64) * n)
    assert 0 < hits.sum() < W * H * n
    assert np.array_equal(np.rint(cov.astype(np.float64) * n).sum(-1), hits)
    assert pt.mattes_lost("object") == 0
    pt.close()


def test_moving_scenes(small_scene, camera):
    from test_refit_gpu import fresh_arrays, moved
    import rebuild_ref as RB
    W, H, n, seed = 48, 36, 4, 9
    arrays = small_scene
    pt = make_pt(arrays, W, H, camera)
    labels, names = np.arange(arrays.n_tris) % 13, ["p%d" % k for k in range(13)]
    ids = ids_of(labels, names)
    pt.scene.set_matte("object", labels, names)
    tri, norm = moved(arrays, "sine10")
    pt.update_geometry(tri, norm)
    pt.mattes(n, seed)
    now = fresh_arrays(arrays, tri, norm)
    check_kind(pt, "object", first_hit_indices(now, W, H, pt, seed, n), ids)
    tri2, norm2 = moved(now, "rotate")
    order, fresh = RB.expected(now, tri2, norm2)
    got = pt.rebuild_geometry(tri2, norm2)
    assert np.array_equal(got, order) and not np.array_equal(order, np.arange(arrays.n_tris))
    pt.mattes(n, seed)
    check_kind(pt, "object", first_hit_indices(fresh, W, H, pt, seed, n), ids[order.astype(np.int64)])
    pt.close()


def test_default_mattes(camera):
    """objects from the props, materials from the distinct rows of mat in order of first appearance"""
    arrays = S.bunny_scene(n=8, env_size=(64, 32), keep_order=True)
    W, H = 48, 32
    pt = make_pt(arrays, W, H, camera)
    pt.scene.set_default_mattes()
    props = arrays.meta["prop_names"]
    assert len(props) == int(arrays.meta["tri_part"].max()) + 1 and all(p.startswith("%d:" % i) for i, p in enumerate(props))
    rows = [r.tobytes() for r in np.ascontiguousarray(arrays.mat, np.float32).reshape(-1, 12)]
    distinct = []
    for r in rows:
        if r not in distinct:
            distinct.append(r)
    mat_names = ["m%04d" % k for k in range(len(distinct))]
    assert pt.scene.matte_manifests == {0: M.manifest(props), 1: M.manifest(mat_names)}
    pt.mattes(2, 3)
    idx = first_hit_indices(arrays, W, H, pt, 3, 2)
    check_kind(pt, "object", idx, ids_of(arrays.meta["tri_part"], props))
    ids, _, _ = check_kind(pt, "material", idx, ids_of([distinct.index(r) for r in rows], mat_names))
    assert len(np.unique(ids)) > 2  # more than one material and the empty rank
    pt.close()


# ---- the file --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered(small_scene, camera):
    """a tracer with a render, features and a mattes pass of both kinds, and what its buffers hold"""
    W, H = 37, 21
    pt = make_pt(small_scene, W, H, camera)
    lo, no = names_mod(small_scene.n_tris, 5)
    lm, nm = names_mod(small_scene.n_tris, 7, "mat \"x\" ")
    pt.scene.set_matte("object", lo, no)
    pt.scene.set_matte("material", lm, nm)
    pt.seed(3)
    pt.render(4)
    pt.features(4, 2)
    pt.mattes(8, 2)
    bufs = dict(rgba=pt.readRadiance(), feat=pt.readFeatures(), ranks={k: pt.read_mattes(k, raw=True) for k in (0, 1)},
                manifests={M.OBJECT: M.manifest(no), M.MATERIAL: M.manifest(nm)})
    yield pt, bufs
    pt.close()


@pytest.mark.parametrize("float32", [False, True])
@pytest.mark.parametrize("compression", ["none", "zips", "zip"])
def test_draw_exr_is_the_restatements_file(rendered, compression, float32):
    pt, b = rendered
    layers = ("alpha", "albedo", "normal", "depth", "crypto_object", "crypto_material")
    got = pt.draw_exr(compression=compression, float32=float32, layers=layers)
    kw = dict(compression=fspt_amd.tracer.EXR_COMPRESSIONS[compression], pixel_type=X.FLOAT if float32 else X.HALF, layers=63)
    want = M.encode(b["rgba"], b["feat"], b["ranks"], b["manifests"], bottom_up=True, **kw)
    assert got == want, (len(got), len(want), next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None))
    assert len(got) <= M.bound(37, 21, manifests=b["manifests"], **kw)
    f = M.read(got)
    for kind in (M.OBJECT, M.MATERIAL):
        ids, cov = pt.read_mattes(kind)
        assert np.array_equal(f["mattes"][kind][0], ids[::-1]) and np.array_equal(f["mattes"][kind][1].view(np.uint32), cov[::-1].view(np.uint32))
        assert f["manifests"][kind] == b["manifests"][kind]
    # the stand-alone entry on the same buffers, and one kind alone
    assert fspt_amd.exr_encode(b["rgba"], b["feat"], compression, float32, layers, bottom_up=True,
                               mattes={"object": (b["ranks"][0], b["manifests"][0]), "material": (b["ranks"][1], b["manifests"][1])}) == want
    one = pt.draw_exr(compression=compression, float32=float32, layers=("crypto_material",))
    assert one == M.encode(b["rgba"], None, b["ranks"], b["manifests"], bottom_up=True, **dict(kw, layers=32))


def test_cap_and_the_plain_file(rendered):
    pt, b = rendered
    lib = L.lib()
    want = M.encode(b["rgba"], b["feat"], b["ranks"], b["manifests"], bottom_up=True, layers=63)
    p = L.ExrParams(3, 1, 63, 0)
    buf, n = np.full(len(want) + 8, 7, np.uint8), C.c_size_t(123)
    assert lib.fspt_draw_exr(pt._t, 0, C.byref(p), L.u8ptr(buf), len(want) - 1, C.byref(n)) == -1
    assert n.value == len(want) and (buf == 7).all()
    assert lib.fspt_draw_exr(pt._t, 0, C.byref(p), L.u8ptr(buf), len(want), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want and (buf[n.value:] == 7).all()
    # behind a mattes pass the file without matte layers is still exr_ref's
    assert pt.draw_exr(layers=15) == X.encode(b["rgba"], b["feat"], bottom_up=True, layers=15)
    # and the entries that do not take the bits refuse them as before
    with pytest.raises(FsptError) as e:
        fspt_amd.exr_encode(b["rgba"], b["feat"], layers=16 | 15)
    assert e.value.code == -1


def test_untouched(small_scene, camera):
    W, H = 40, 30
    out = []
    for with_pass in (False, True):
        pt = make_pt(small_scene, W, H, camera)
        labels, names = names_mod(small_scene.n_tris, 5)
        pt.scene.set_matte("object", labels, names)
        pt.seed(5)
        pt.render(3)
        pt.features(2, 7)
        if with_pass:
            pt.mattes(4, 7)
        pt.render(2)
        out.append((pt.readRadiance(), pt.readFeatures()))
        pt.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_errors(small_scene, camera):
    W, H = 16, 12
    pt = make_pt(small_scene, W, H, camera)
    lib = L.lib()

    def code(fn):
        with pytest.raises(FsptError) as e:
            fn()
        return e.value.code, str(e.value)

    assert code(lambda: pt.mattes(2, 1))[0] == -6  # no ids
    labels, names = names_mod(small_scene.n_tris, 5)
    pt.scene.set_matte("object", labels, names)
    assert code(lambda: pt.read_mattes("object"))[0] == -6
    assert code(lambda: pt.mattes_lost("object"))[0] == -6
    assert code(lambda: pt.draw_exr(layers=("crypto_object",)))[0] == -6
    assert code(lambda: pt.mattes(0, 1))[0] == -1
    assert code(lambda: pt.mattes(65536, 1))[0] == -1
    pt.mattes(2, 1)
    assert code(lambda: pt.draw_exr(layers=("crypto_material",)))[0] == -6  # a kind the pass did not compute
    before = pt.read_mattes("object")
    bad = ids_of(labels, names)
    for k, v in ((7, 0x00400000), (3, 0x7F800001), (5, 0xFF800000), (9, 0x80000001)):
        ids = bad.copy()
        ids[k] = v
        c, text = code(lambda: pt.scene.set_matte_ids("object", ids))
        assert c == -1 and "ids[%d]" % k in text
    pt.mattes(2, 1)  # the old table is still there
    after = pt.read_mattes("object")
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert lib.fspt_mattes(pt._t, None, 1, 1) == -1
    pt.scene.set_matte("object", None, None)
    assert code(lambda: pt.mattes(2, 1))[0] == -6
    pt.close()


# ---- the Node host ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")),
                    reason="node or the built addon is missing")
def test_node_host_matches_python_host(small_scene, camera, tmp_path):
    """fspt.js setMatte / mattes / readMattes / drawExr / exrEncode({mattes}) give the Python host's bytes; while a renderAsync
    job is in flight they throw Error('render in flight')."""
    import base64
    import json
    W, H, seed, ticks, samples, mseed = 64, 40, 13, 3, 8, 3
    no, nm = ["obj %d" % k for k in range(5)], ["m%04d" % k for k in range(3)]
    env, ew, eh = S.synthetic_env(64, 32)
    job = {"props": S.bunny_props(), "objs": {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ},
           "env": {"rgbe_b64": base64.b64encode(env.tobytes()).decode(), "width": ew, "height": eh},
           "W": W, "H": H, "bounces": 4, "seed": seed, "ticks": ticks, "samples": samples, "matte_seed": mseed, "object_names": no, "material_names": nm,
           "cam": dict(P=camera["P"], I=camera["I"], fov_scale=camera["fov_scale"], env_theta=camera["env_theta"], lens=camera["lens"])}
    jp, op = tmp_path / "job.json", tmp_path / "out.json"
    jp.write_text(json.dumps(job))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "matte_node_check.js"), str(jp), str(op)], timeout=300)
    out = json.loads(op.read_text())
    dec = lambda k: base64.b64decode(out[k])
    assert out["n_tris"] == small_scene.n_tris
    pt = make_pt(small_scene, W, H, camera)
    pt.scene.set_matte("object", np.arange(small_scene.n_tris) % 5, no)
    pt.scene.set_matte("material", np.arange(small_scene.n_tris) % 3, nm)
    pt.seed(seed)
    pt.render(ticks)
    pt.mattes(samples, mseed)
    assert dec("object") == pt.read_mattes("object", raw=True).tobytes() and dec("material") == pt.read_mattes("material", raw=True).tobytes()
    ids, cov = pt.read_mattes("object")
    assert dec("object_ids") == ids.tobytes() and dec("object_cov") == cov.tobytes() and ids[..., 0].any()
    assert out["lost"] == [pt.mattes_lost("object"), pt.mattes_lost("material")]
    want = pt.draw_exr(compression="zips", layers=("alpha", "crypto_object", "crypto_material"))
    assert dec("file") == want and dec("encoded") == want
    assert M.read(want)["manifests"] == {0: M.manifest(no), 1: M.manifest(nm)}
    assert out["during"] == {"mattes": "render in flight", "readMattes": "render in flight", "drawExr": "render in flight"}
    assert out["after"] is None
    pt.close()
