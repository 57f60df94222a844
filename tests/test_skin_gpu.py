"""GPU skinning (fspt_scene_set_skin / fspt_scene_update_skin) on the MI355X.  No tolerance anywhere:
k_skin_transform's output equals tests/skin_ref.py word for word, and a scene skinned from joint matrices and morph weights
is indistinguishable from a twin that was handed skin_ref's arrays through update_geometry - hits, step and leaf counts,
two-level nodes, SAH cost, light table, frames of every pipeline, temporal reprojection."""
import numpy as np
import pytest

import lights_ref as LR
import oracle as O
import pose_ref as PR
import skin_ref as SR
from conftest import random_rays
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene, skin_set_form
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 64, 48, 4
SCENES = ("one", "small", "gpu", "textured", "lights", "soup22", "soup86")
JOINTS = (1, 2, 5, 300)  # 5: joint 3 stays unused; 300: ids need the high byte
PATTERNS = ("one_hot", "dyadic", "general", "zero_slots")
FRAMES = ("identity", "rotate", "scale", "shear_mirror")
MORPHS = ((0, False), (1, False), (1, True), (3, False), (3, True))  # (targets, with morph_norm)
MORPH_W = (0.0, 1.0, 0.3)


def one_triangle_scene():
    env, w, h = S.synthetic_env(64, 32)
    prop = {"path": "t.obj", "scale": 1.5, "translate": [0.0, -0.4, 0.0], "diffuse": [0.8, 0.6, 0.3], "emittance": [0, 0, 0]}
    return S.build_scene([prop], {"t.obj": "v -1 0 0.5\nv 1 0 0.5\nv 0 1 -0.5\nf 1 2 3\n"}, env=env, env_w=w, env_h=h)


def soup_scene(n):
    """n loose triangles in front of the camera: 22 -> 66 corners (cross a wave), 86 -> 258 (cross a block)"""
    rng = np.random.default_rng(n)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) * [1.2, 0.8, 0.8]
    v = (c + rng.normal(0, 0.25, (n, 3, 3))).reshape(-1, 3)
    text = "".join("v %.6f %.6f %.6f\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(n))
    env, w, h = S.synthetic_env(64, 32)
    prop = {"path": "s.obj", "scale": 1.0, "translate": [0.0, 0.0, 0.0], "diffuse": [0.7, 0.5, 0.4], "emittance": [0, 0, 0]}
    a = S.build_scene([prop], {"s.obj": text}, env=env, env_w=w, env_h=h)
    assert a.n_tris == n
    return a


@pytest.fixture(scope="module")
def scenes(small_scene):
    return {"one": one_triangle_scene(), "small": small_scene,
            "gpu": S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu", keep_order=True),
            "textured": S.textured_test_scene(keep_order=True), "lights": LR.scene_e1(),
            "soup22": soup_scene(22), "soup86": soup_scene(86)}


def hashed(n, salt):
    """a hash of the corner-slot index: ids interleave inside leaves"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt * 7919)
    return ((i * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFFFFFF)


def joint_ids(T, n_joints, salt=0):
    ids = (hashed(T * 12, salt) % np.uint64(n_joints)).astype(np.uint16)
    if n_joints == 5:
        ids[ids == 3] = 0
    if n_joints == 300 and T * 12 >= 24:
        ids[5], ids[18] = 299, 256  # the high byte is used whatever the hash says
    return ids.reshape(T, 3, 4)


def weight_pattern(name, T):
    slot = (hashed(T * 3, 1) % np.uint64(4)).astype(np.int64)
    w = np.zeros((T * 3, 4), np.float32)
    if name == "one_hot":
        w[np.arange(T * 3), slot] = 1.0
    elif name == "dyadic":
        base = np.float32([0.5, 0.25, 0.125, 0.125])
        w = np.stack([np.roll(base, s) for s in slot])
    elif name == "general":
        raw = (hashed(T * 12, 2) % np.uint64(1000)).astype(np.float64).reshape(-1, 4) + 1.0
        w = (raw / raw.sum(1, keepdims=True)).astype(np.float32)
    elif name == "zero_slots":  # two live influences; the other two slots weigh 0 and point at arbitrary valid joints
        w[:, 0], w[:, 1] = 0.7, 0.3
        w = np.stack([np.roll(r, s) for r, s in zip(w, slot)])
    return w.reshape(T, 3, 4)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return S._rotation_matrix(axis, angle)


def frame_set(name, n_joints):
    out = np.zeros((n_joints, 3, 4), np.float64)
    for p in range(n_joints):
        k = p % 7
        if name == "identity":
            A, t = np.eye(3), np.zeros(3)
        elif name == "rotate":
            A, t = rot([1 + k, 2, -0.5 * k], 0.3 + 0.1 * k), np.array([0.05 * k, -0.03, 0.02 * k])
        elif name == "scale":
            A, t = 0.37 * np.eye(3), np.zeros(3)
        elif name == "shear_mirror":
            A = (np.diag([1.3, 0.6, 0.9 + 0.05 * k]) + np.array([[0, 0.4, 0], [0, 0, 0], [0.1 * k, 0, 0]])) @ np.diag([1.0, -1.0, 1.0])
            t = np.array([0.0, 0.1, 0.0])
        out[p, :, :3], out[p, :, 3] = A, t
    return out.reshape(n_joints, 12).astype(np.float32)


def morph_targets(T, n_morph, with_norm):
    if not n_morph:
        return None, None
    rng = np.random.default_rng(100 + n_morph)
    morph = rng.normal(0, 0.03, (n_morph, T, 9)).astype(np.float32)
    return morph, rng.normal(0, 0.1, (n_morph, T, 27)).astype(np.float32) if with_norm else None


def morph_weights(n_morph, k):
    return None if not n_morph else np.float32([MORPH_W[(k + m) % 3] for m in range(n_morph)])


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


def simple_skin(arrays, n_joints=5, pattern="general", n_morph=0, with_norm=False):
    T = arrays.n_tris
    return (joint_ids(T, n_joints), weight_pattern(pattern, T)) + morph_targets(T, n_morph, with_norm)


def reference(arrays, skin, xf, mw=None):
    j, w, morph, mnorm = skin
    return SR.skin(j, w, arrays.tri, arrays.norm, xf, morph, mnorm, mw)


# ---- every combination: the kernel and the scene, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("n_joints", JOINTS)
@pytest.mark.parametrize("name", SCENES)
def test_skinned_scene_equals_the_reference_and_its_twin(scenes, name, n_joints):
    arrays = scenes[name]
    T = arrays.n_tris
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    A, B = Scene(arrays), Scene(arrays)
    lights = name == "lights"
    tracers = [(make_pt(A, pipeline=p, lights=l), make_pt(B, pipeline=p, lights=l))
               for p in ("megakernel", "wavefront", "stream") for l in ((False, True) if lights else (False,))]
    rays = ray_set(arrays)
    joints = joint_ids(T, n_joints)
    lit = False
    try:
        for pattern in PATTERNS:
            weights = weight_pattern(pattern, T)
            for n_morph, with_norm in MORPHS:
                morph, mnorm = morph_targets(T, n_morph, with_norm)
                A.set_skin(joints, weights, morph=morph, morph_norm=mnorm, n_joints=n_joints)
                assert A.last_skin["bytes"] == T * (24 + 48 + 36 + 108) + n_morph * T * (36 + (108 if with_norm else 0)) + n_joints * 48 + n_morph * 4
                for k, fname in enumerate(FRAMES):
                    what = (pattern, n_morph, with_norm, fname)
                    xf, mw = frame_set(fname, n_joints), morph_weights(n_morph, k)
                    want_t, want_n = SR.skin(joints, weights, rest_t, rest_n, xf, morph, mnorm, mw)
                    A.update_skin(xf, mw)
                    got_t, got_n = A.read_skin()
                    assert np.array_equal(bits(got_t), bits(want_t)), (what, int((bits(got_t) != bits(want_t)).sum()))
                    assert np.array_equal(bits(got_n), bits(want_n)), (what, int((bits(got_n) != bits(want_n)).sum()))
                    if fname == "identity" and pattern in ("one_hot", "dyadic") and (mw is None or not mw.any()):
                        assert (got_t == rest_t).all() and (got_n == rest_n).all(), what  # value for value (the sign of a zero may differ)
                    elif fname != "identity":
                        assert not np.array_equal(got_t, rest_t), what
                    B.update_geometry(want_t, want_n)
                    ha, hb = A.intersect(rays), B.intersect(rays)
                    for i, part in enumerate(("t", "index", "steps", "leaves")):
                        assert np.array_equal(bits(ha[i]), bits(hb[i])), (what, part)
                    assert A.two_level_nodes() == B.two_level_nodes(), what
                    if B.two_level_nodes()[0]:
                        assert same_hits(A.intersect(rays, two_level=True), B.intersect(rays, two_level=True)), what
                    assert A.sah_cost() == B.sah_cost(), what
                    if lights:
                        ta, tb = A.light_table(), B.light_table()
                        for key in tb:
                            assert np.array_equal(bits(ta[key]), bits(tb[key])), (what, key)
                    for pa, pb in tracers:
                        fa, fb = again(pa), again(pb)
                        assert np.array_equal(fa, fb), (what, int((fa != fb).any(-1).sum()))
                        assert np.isfinite(fa).all(), what
                        lit = lit or fa[..., :3].max() > 0
        ms = A.last_skin
        assert ms["launches"] >= 3 and ms["skin_ms"] > 0 and ms["refit_ms"] > 0
        assert lit  # (not every frame: the mirrored emitter of the lights scene faces away from everything)
    finally:
        for pa, pb in tracers:
            pa.close(); pb.close()
        A.close(); B.close()


def test_skin_without_rest_normals_leaves_the_normals_alone(scenes):
    arrays = scenes["textured"]
    j, w, morph, _ = simple_skin(arrays, n_morph=1)
    xf, mw = frame_set("rotate", 5), np.float32([0.3])
    A, B = Scene(arrays), Scene(arrays)
    A.set_skin(j, w, arrays.tri, None, morph)
    A.update_skin(xf, mw)
    got_t, got_n = A.read_skin()
    want_t, _ = SR.skin(j, w, arrays.tri, None, xf, morph, None, mw)
    assert got_n is None and np.array_equal(bits(got_t), bits(want_t))
    B.update_geometry(want_t)
    assert np.array_equal(frame(A), frame(B))
    assert np.array_equal(A.read_appearance("hitrec"), B.read_appearance("hitrec"))
    A.close(); B.close()


# ---- the joint table's two forms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints", (16, 1365, 1366))  # 1365 x 48 bytes is the last table the LDS form stages
def test_both_joint_table_forms_give_the_same_bits(scenes, n_joints):
    arrays = scenes["soup86"]
    T = arrays.n_tris
    joints, weights = joint_ids(T, n_joints), weight_pattern("general", T)
    joints[0, 0, 0], joints[-1, -1, -1] = n_joints - 1, n_joints - 1
    morph, mnorm = morph_targets(T, 1, True)
    xf, mw = frame_set("rotate", n_joints), np.float32([0.3])
    want = SR.skin(joints, weights, arrays.tri, arrays.norm, xf, morph, mnorm, mw)
    sc = Scene(arrays)
    sc.set_skin(joints, weights, morph=morph, morph_norm=mnorm, n_joints=n_joints)
    try:
        for form in (0, 1):
            skin_set_form(form)
            sc.update_skin(xf, mw)
            got = sc.read_skin()
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), form
    finally:
        skin_set_form(0)
        sc.close()


# ---- the device form -------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(scenes):
    import torch
    arrays = scenes["small"]
    skin = simple_skin(arrays, n_morph=3, with_norm=True)
    xf, mw = frame_set("rotate", 5), morph_weights(3, 0)
    A, B = Scene(arrays), Scene(arrays)
    for sc in (A, B):
        sc.set_skin(skin[0], skin[1], morph=skin[2], morph_norm=skin[3])
    A.update_skin(xf, mw)
    d_xf = torch.from_numpy(xf).to("cuda:0") * 1.0  # (computed on the device)
    d_mw = torch.from_numpy(mw).to("cuda:0") * 1.0
    B.update_skin(d_xf, d_mw)
    for a, b in zip(A.read_skin(), B.read_skin()):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(frame(A), frame(B))
    assert A.sah_cost() == B.sah_cost()
    with pytest.raises(TypeError):
        B.update_skin(d_xf, mw)  # one on the device, one on the host
    with pytest.raises(TypeError):
        B.update_skin(d_xf.double(), d_mw)
    with pytest.raises(ValueError):
        B.update_skin(torch.zeros(61, device="cuda:0")[1:], d_mw)  # not 16-byte aligned
    f0 = frame(B)
    with pytest.raises(FsptError) as ei:
        B.update_skin(d_xf * float("nan"), d_mw)  # no host check: the refit's finiteness check refuses the result
    assert ei.value.code == -1
    assert np.array_equal(frame(B), f0)
    with pytest.raises(FsptError) as ei:
        B.read_skin()  # the refused frame is in the staging array: nothing is handed out
    assert ei.value.code == -6 and "fspt_scene_read_skin" in str(ei.value)
    B.update_skin(d_xf, d_mw)
    for a, b in zip(reference(arrays, skin, xf, mw), B.read_skin()):
        assert np.array_equal(bits(a), bits(b))
    # no morph weights for a skin without targets
    B.set_skin(skin[0], skin[1])
    B.update_skin(d_xf)
    assert np.array_equal(bits(B.read_skin()[0]), bits(SR.skin(skin[0], skin[1], arrays.tri, arrays.norm, xf)[0]))
    A.close(); B.close()


# ---- rebuild ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "textured"))
def test_rebuild_permutes_the_skin(scenes, name):
    arrays = scenes[name]
    T = arrays.n_tris
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    j, w, morph, mnorm = simple_skin(arrays, n_joints=300, n_morph=3, with_norm=True)
    x1, x2 = frame_set("shear_mirror", 300), frame_set("rotate", 300)
    m1, m2 = morph_weights(3, 1), morph_weights(3, 2)
    A, B = Scene(arrays), Scene(arrays)
    A.set_skin(j, w, morph=morph, morph_norm=mnorm, n_joints=300)
    A.update_skin(x1, m1)
    t1, n1 = A.read_skin()
    assert np.array_equal(bits(t1), bits(SR.skin(j, w, rest_t, rest_n, x1, morph, mnorm, m1)[0]))
    order = A.rebuild_geometry(t1, n1).astype(np.int64)
    assert np.array_equal(B.rebuild_geometry(t1, n1), order)
    assert not np.array_equal(order, np.arange(T))
    with pytest.raises(FsptError) as ei:
        A.read_skin()  # the staging array is the rebuild's
    assert ei.value.code == -6
    A.update_skin(x2, m2)  # nothing from the caller: the scene permuted ids, weights, rest mesh and targets
    t2, n2 = SR.skin(j[order], w[order], rest_t[order], rest_n[order], x2, morph[:, order], mnorm[:, order], m2)
    B.update_geometry(t2, n2)
    got_t, got_n = A.read_skin()
    assert np.array_equal(bits(got_t), bits(t2)) and np.array_equal(bits(got_n), bits(n2))
    rays = ray_set(arrays)
    assert same_hits(A.intersect(rays), B.intersect(rays))
    assert A.sah_cost() == B.sah_cost() and A.two_level_nodes() == B.two_level_nodes()
    for pipeline in ("megakernel", "wavefront", "stream"):
        assert np.array_equal(frame(A, pipeline=pipeline), frame(B, pipeline=pipeline))
    with pytest.raises(ValueError):
        A.set_skin(j, w)  # the default rest mesh is gone with the order
    A.close(); B.close()


# ---- pose and skin on one scene --------------------------------------------------------------------------------------
def test_pose_and_skin_alternate(scenes):
    arrays = scenes["small"]
    T = arrays.n_tris
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    j, w, _, _ = simple_skin(arrays)
    part = (hashed(T, 3) % np.uint64(3)).astype(np.uint32)
    xs, xp = frame_set("rotate", 5), frame_set("shear_mirror", 3)
    A, B = Scene(arrays), Scene(arrays)
    A.set_pose(part, n_parts=3)
    A.set_skin(j, w)
    for sc_read in (A.read_pose, A.read_skin):
        with pytest.raises(FsptError) as ei:
            sc_read()
        assert ei.value.code == -6
    for _ in range(2):
        A.update_skin(xs)
        want = SR.skin(j, w, rest_t, rest_n, xs)
        got = A.read_skin()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        with pytest.raises(FsptError) as ei:
            A.read_pose()  # the staging array holds the skin's output
        assert ei.value.code == -6 and "fspt_scene_read_pose" in str(ei.value)
        B.update_geometry(*want)
        assert np.array_equal(frame(A), frame(B))
        A.update_transforms(xp)
        want = PR.pose(part, rest_t, rest_n, xp)
        got = A.read_pose()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        with pytest.raises(FsptError) as ei:
            A.read_skin()
        assert ei.value.code == -6 and "fspt_scene_read_skin" in str(ei.value)
        B.update_geometry(*want)
        assert np.array_equal(frame(A), frame(B))
    A.update_skin(xs)
    A.update_geometry(rest_t, rest_n)  # a host upload reuses the array too
    with pytest.raises(FsptError):
        A.read_skin()
    A.close(); B.close()


# ---- ordering --------------------------------------------------------------------------------------------------------
def test_recorded_ticks_run_before_the_skin(scenes):
    arrays = scenes["small"]
    j, w, _, _ = simple_skin(arrays)
    xf = frame_set("rotate", 5)
    out = []
    for sync_first in (False, True):
        sc = Scene(arrays); sc.set_skin(j, w)
        pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        pt.update_skin(xf)
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


def test_present_around_the_skin(scenes):
    """A frame in flight when the call arrives is presented once, unchanged; the yardstick is a second tracer that draws
    (blocking) where the first presents, on a twin that gets update_geometry."""
    arrays = scenes["small"]
    skin = simple_skin(arrays, n_morph=1)
    xf, mw = frame_set("rotate", 5), np.float32([1.0])
    tri, norm = reference(arrays, skin, xf, mw)
    sc = Scene(arrays); sc.set_skin(skin[0], skin[1], morph=skin[2]); pt = make_pt(sc)
    ref = Scene(arrays); pr = make_pt(ref)

    def ticks(n):
        for _ in range(n):
            pt.tick(); pr.tick()

    ticks(2)
    img, n = pt.present()
    assert img is None and n == 0
    pre = pr.draw()
    pt.update_skin(xf, mw); pr.update_geometry(tri, norm)
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


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_unchanged(scenes):
    arrays = scenes["small"]
    T = arrays.n_tris
    j, w, morph, _ = simple_skin(arrays, n_morph=1)
    sc = Scene(arrays)
    pt = make_pt(sc)
    f0 = again(pt)
    rays = ray_set(arrays)
    h0 = sc.intersect(rays)
    good, mw = frame_set("rotate", 5), np.float32([0.3])
    assert sc.last_skin["bytes"] == 0
    with pytest.raises(FsptError) as ei:
        sc.update_skin(good, mw)  # no skin
    assert ei.value.code == -6
    with pytest.raises(FsptError) as ei:
        sc.set_skin(j, w, morph=morph, n_joints=3)  # ids up to 4
    assert ei.value.code == -1 and "joints[" in str(ei.value)
    bad_w = w.copy(); bad_w[T // 2, 1, 2] = np.inf
    with pytest.raises(FsptError) as ei:
        sc.set_skin(j, bad_w, morph=morph)
    assert ei.value.code == -1 and f"weights[{(T // 2) * 12 + 6}]" in str(ei.value)
    with pytest.raises(FsptError) as ei:
        sc.update_skin(good, mw)  # still no skin
    assert ei.value.code == -6 and sc.last_skin["bytes"] == 0
    sc.set_skin(j, w, morph=morph)
    assert sc.last_skin["bytes"] == T * 216 + T * 36 + 5 * 48 + 4
    nan = good.copy(); nan[2, 5] = np.nan
    collapse = np.zeros_like(good)  # every blend is the zero matrix: q == 0, the frames are NaN
    half = good.copy(); half[1] = 0.0  # only corners that weigh joint 1 alone collapse
    one_hot = weight_pattern("one_hot", T)
    cases = [("n_joints", good[:-1], mw), ("n_morph", good, np.float32([0.3, 0.1])), ("no_weights", good, None), ("nan", nan, mw),
             ("nan_weight", good, np.float32([np.nan])), ("inf_weight", good, np.float32([np.inf])), ("collapse", collapse, mw)]
    for what, xf, m in cases:
        with pytest.raises(FsptError) as ei:
            sc.update_skin(xf, m)
        assert ei.value.code == -1, what
        if what == "nan":
            assert "joint 2" in str(ei.value)
        if what in ("nan_weight", "inf_weight"):
            assert "morph target 0" in str(ei.value)
        if what == "collapse":
            assert "not finite" in str(ei.value)
        assert same_hits(sc.intersect(rays), h0), what
        assert np.array_equal(again(pt), f0), what
    sc.set_skin(j, one_hot, morph=morph)
    assert (j.reshape(-1, 4)[np.arange(T * 3), one_hot.reshape(-1, 4).argmax(1)] == 1).any()
    with pytest.raises(FsptError) as ei:
        sc.update_skin(half, mw)  # some corners collapse: refused whole
    assert ei.value.code == -1
    assert same_hits(sc.intersect(rays), h0) and np.array_equal(again(pt), f0)
    with pytest.raises(ValueError):
        sc.update_skin(good.reshape(-1)[:-1], mw)
    with pytest.raises(ValueError):
        sc.set_skin(j[:-1], w)
    # read_skin hands out only a frame the scene took: a refusal on the host leaves the accepted frame readable, one by
    # the refit's check (the kernel has overwritten the staging array by then) leaves none
    skin = (j, one_hot, morph, None)
    first = frame_set("shear_mirror", 5)
    sc.update_skin(first, mw)
    want = reference(arrays, skin, first, mw)
    f1, h1 = again(pt), sc.intersect(rays)
    for what, xf, m in (("n_joints", good[:-1], mw), ("nan", nan, mw), ("nan_weight", good, np.float32([np.nan]))):
        with pytest.raises(FsptError) as ei:
            sc.update_skin(xf, m)
        assert ei.value.code == -1, what
        got = sc.read_skin()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), what
    with pytest.raises(FsptError) as ei:
        sc.update_skin(collapse, mw)
    assert ei.value.code == -1
    with pytest.raises(FsptError) as ei:
        sc.read_skin()
    assert ei.value.code == -6 and "fspt_scene_read_skin" in str(ei.value)
    assert same_hits(sc.intersect(rays), h1) and np.array_equal(again(pt), f1)  # the scene keeps the frame it took
    sc.update_skin(good, mw)  # and the skin still works
    want = reference(arrays, skin, good, mw)
    got = sc.read_skin()
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not np.array_equal(again(pt), f0)
    sc.set_skin(None)
    assert sc.last_skin["bytes"] == 0
    with pytest.raises(FsptError) as ei:
        sc.update_skin(good, mw)
    assert ei.value.code == -6
    sc.set_skin(None)  # dropping twice is fine
    pt.close(); sc.close()


# ---- multi -----------------------------------------------------------------------------------------------------------
def test_multi_update_skin(scenes):
    arrays = scenes["small"]
    skin = simple_skin(arrays, n_morph=1, with_norm=True)
    xf, mw = frame_set("rotate", 5), np.float32([0.3])
    mp = MultiPathTracer(arrays, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    mp.set_skin(skin[0], skin[1], morph=skin[2], morph_norm=skin[3])
    mp.update_skin(xf, mw)
    mp.render(TICKS)
    got = mp.readRadiance()
    mp.close()
    B = Scene(arrays)
    B.update_geometry(*reference(arrays, skin, xf, mw))
    assert np.array_equal(got, frame(B))
    B.close()


# ---- temporal --------------------------------------------------------------------------------------------------------
def test_temporal_reprojection_follows_the_skin(scenes):
    arrays = scenes["small"]
    skin = simple_skin(arrays, n_morph=1)
    xf, mw = frame_set("rotate", 5), np.float32([1.0])
    tri, norm = reference(arrays, skin, xf, mw)
    out = []
    for skinned in (True, False):
        sc = Scene(arrays)
        pt = make_pt(sc)
        pt.render(TICKS)
        pt.temporal_accumulate()
        sc.motion_begin()
        if skinned:
            sc.set_skin(skin[0], skin[1], morph=skin[2]); sc.update_skin(xf, mw)
        else:
            sc.update_geometry(tri, norm)
        pt.clear(); pt.seed(9); pt.render(TICKS)
        out.append((pt.temporal_accumulate(), pt.temporal_gbuffer()))
        sc.motion_end()
        pt.close(); sc.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))
    for a, b in zip(out[0][1], out[1][1]):
        assert np.array_equal(bits(a), bits(b))
    assert np.abs(out[0][1][1]).max() > 0  # something moved on the screen
