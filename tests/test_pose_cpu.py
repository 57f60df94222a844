"""GPU part transforms, what needs no device: the host part of the rule (the derived matrices D and N and
what is refused), prop_matrix against the scene builder, the pose-frame classifier, meta["tri_part"], NULL handles."""
import json

import numpy as np
import pytest

import pose_ref as PR
from fspt_amd import _lib as L
from fspt_amd import scene as S
from fspt_amd import scene_file as F


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return S._rotation_matrix(axis, angle)


def xf_of(A, t=(0, 0, 0)):
    with np.errstate(over="ignore"):
        return np.concatenate([np.asarray(A, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(np.float32).reshape(1, 12)


def lib_derive(xf):
    """(rc, out [n, 30], bad part) of fspt_pose_matrices_eval"""
    xf = np.ascontiguousarray(xf, np.float32).reshape(-1, 12)
    out = np.zeros((xf.shape[0], 30), np.float32)
    bad = np.zeros(1, np.uint32)
    rc = L.lib().fspt_pose_matrices_eval(L.fptr(xf), xf.shape[0], L.fptr(out), L.u32ptr(bad))
    return rc, out, int(bad[0])


# ---- derived matrices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1.0, 0.37, 250.0, 1e-12))
def test_similarity_gives_the_rotation(scale):
    R = rot([1, 2, -0.5], 0.83) @ rot([0, 1, 0], -2.1)
    rc, out, _ = lib_derive(xf_of(R * scale, (1, 2, 3)))
    assert rc == 0
    D, N = out[0, 12:21].reshape(3, 3), out[0, 21:30].reshape(3, 3)
    assert np.abs(D - R).max() <= 1e-6 and np.abs(N - R).max() <= 1e-6
    assert np.array_equal(out[0, :12], xf_of(R * scale, (1, 2, 3))[0])


def test_mirror_gives_minus_the_rotation():
    R = rot([0.3, -1, 0.2], 1.1)
    M = R @ np.diag([1.0, -1.0, 1.0]) * 0.5
    rc, out, _ = lib_derive(xf_of(M))
    assert rc == 0
    D, N = out[0, 12:21], out[0, 21:30]
    assert np.abs(N + D).max() <= 1e-6
    assert np.abs(D.reshape(3, 3) - M / 0.5).max() <= 1e-6


def test_library_equals_the_reference_bit_for_bit():
    rng = np.random.default_rng(3)
    xf = rng.normal(0, 1, (64, 12)).astype(np.float32)
    xf[:8] *= np.float32(1e-18); xf[8:16] *= np.float32(1e15)
    xf[16] = xf_of(np.diag([2.0, 0.5, 3.0]) + np.array([[0, 0.7, 0], [0, 0, 0], [0.1, 0, 0]]))  # non-uniform scale + shear
    rc, out, _ = lib_derive(xf)
    assert rc == 0
    a, D, N = PR.derive(xf)
    assert np.array_equal(out[:, :12].view(np.uint32), a.reshape(-1, 12).view(np.uint32))
    assert np.array_equal(out[:, 12:21].view(np.uint32), D.reshape(-1, 9).view(np.uint32))
    assert np.array_equal(out[:, 21:30].view(np.uint32), N.reshape(-1, 9).view(np.uint32))


@pytest.mark.parametrize("what", ("singular", "zero", "nan", "inf", "nan_translation"))
def test_bad_matrices_are_refused_naming_the_part(what):
    good = xf_of(np.eye(3))
    bad = {"singular": xf_of([[1, 2, 3], [2, 4, 6], [0, 1, 0]]), "zero": xf_of(np.zeros((3, 3))),
           "nan": xf_of([[1, 0, 0], [0, np.nan, 0], [0, 0, 1]]),
           "inf": xf_of([[1, 0, 0], [0, 1e39, 0], [0, 0, 1]]),  # float32(1e39) overflows
           "nan_translation": xf_of(np.eye(3), (0, np.nan, 0))}[what]
    xf = np.concatenate([good, good, bad, good])
    rc, _, part = lib_derive(xf)
    assert rc == -1 and part == 2
    assert b"part 2" in L.lib().fspt_last_error()
    with pytest.raises(PR.Rejected) as ei:
        PR.derive(xf)
    assert ei.value.part == 2


def test_reference_identity_reproduces_the_rest_pose():
    rng = np.random.default_rng(5)
    tri = rng.normal(0, 3, (7, 9)).astype(np.float32)
    norm = rng.normal(0, 1, (7, 27)).astype(np.float32)
    tri[0, 0] = -0.0
    t2, n2 = PR.pose(np.arange(7) % 2, tri, norm, np.concatenate([xf_of(np.eye(3))] * 2))
    assert (t2 == tri).all() and (n2 == norm).all()


# ---- prop_matrix -----------------------------------------------------------------------------------------------------
def test_prop_matrix_agrees_with_the_builder(tmp_path):
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    obj = S.cube_sphere_obj(3)
    (root / "mesh" / "ball.obj").write_text(obj)
    prop = {"path": "mesh/ball.obj", "scale": 0.4, "translate": [-0.4, 0.25, 1.5], "diffuse": [0.8, 0.3, 0.2], "emittance": [0, 0, 0],
            "rotate": [{"axis": [0, 1, 0], "angle": 0.7}, {"axis": [0.6, 0, 0.8], "angle": -1.9}]}
    world = [{"rotate": [{"axis": [1, 0, 0], "angle": 0.4}]}, {"translate": [0.5, -2.0, 0.25]},
             {"rotate": [{"axis": [0, 0, 1], "angle": 2.2}], "translate": [9, 9, 9]}]  # (a rotate entry's translate is ignored)
    scene = {"props": [prop], "worldTransforms": world}
    (root / "scene" / "s.json").write_text(json.dumps(scene))
    g, _ = F.load_scene_file(str(root / "scene" / "s.json"), str(root), geometry_only=True)
    verts = np.array([[float(x) for x in l.split()[1:]] for l in obj.split("\n") if l.startswith("v ")], np.float64)
    faces = np.array([[int(x) - 1 for x in l.split()[1:]] for l in obj.split("\n") if l.startswith("f ")], np.int64)
    m = S.prop_matrix(prop, world)
    assert m.shape == (3, 4) and m.dtype == np.float64
    want = verts[faces].reshape(-1, 3) @ m[:, :3].T + m[:, 3]
    got = g.tri.reshape(-1, 3).astype(np.float64)
    extent = (got.max(0) - got.min(0)).max()
    assert np.abs(got - want).max() <= 1e-5 * extent
    # and the matrices of a frame pair take one frame's triangles to the other's
    prop2 = dict(prop, scale=0.55, translate=[0.1, 0.0, -0.3], rotate=[{"axis": [0, 1, 0], "angle": 1.3}])
    scene2 = {"props": [prop2], "worldTransforms": world[:2]}
    (root / "scene" / "t.json").write_text(json.dumps(scene2))
    g2, _ = F.load_scene_file(str(root / "scene" / "t.json"), str(root), geometry_only=True)
    assert F.sequence_pose_frame(scene, scene2)
    xf = F.sequence_pose_matrices(scene, scene2)
    assert xf.shape == (1, 12) and xf.dtype == np.float32
    t2, n2 = PR.pose(np.zeros(g.n_tris, np.int64), g.tri.reshape(-1, 9), g.norm.reshape(-1, 27), xf)
    assert np.abs(t2.reshape(-1) - g2.tri).max() <= 1e-5 * extent
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    # the normals (every third frame vector) agree in direction; this OBJ has no `vt`, and the loader then derives uvs, and
    # from them the tangents, from the MOVED vertex positions (obj_loader.js:63-103): those are not a function of the rest frame
    assert np.abs(unit(n2.reshape(-1, 3)[::3]) - unit(g2.norm.reshape(-1, 3)[::3])).max() <= 1e-5


# ---- the classifier --------------------------------------------------------------------------------------------------
def test_pose_frame_classifier():
    base = {"cameraPos": [0, 0.6, 2.4], "samples": 4, "worldTransforms": [{"translate": [0, 1, 0]}],
            "static_props": [{"path": "mesh/quad.obj", "scale": 2.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.6]}],
            "animated_props": {"ball": {"path": "mesh/ball.obj", "scale": 0.4, "translate": [0, 0, 0],
                                        "rotate": [{"axis": [0, 1, 0], "angle": 0.0}], "diffuse": [0.8, 0.3, 0.2], "emittance": [3, 3, 3]}}}
    copy = lambda: json.loads(json.dumps(base))
    assert F.sequence_pose_frame(base, copy())
    moved = copy()
    moved["animated_props"]["ball"].update(translate=[0.4, 0.05, 0], rotate=[{"axis": [0, 1, 0], "angle": 0.3}], scale=0.5)
    del moved["static_props"][0]["translate"]
    moved["worldTransforms"] = [{"rotate": [{"axis": [1, 0, 0], "angle": 0.1}]}]
    assert F.sequence_pose_frame(base, moved)          # only transforms changed
    material = copy(); material["animated_props"]["ball"]["diffuse"] = [0.1, 0.3, 0.2]
    assert not F.sequence_pose_frame(base, material)   # a material changed
    normalize = copy(); normalize["normalize"] = 1.0
    assert not F.sequence_pose_frame(base, normalize) and not F.sequence_pose_frame(normalize, normalize)
    fewer = copy(); fewer["static_props"] = []
    assert not F.sequence_pose_frame(base, fewer)      # the prop count changed
    mesh = copy(); mesh["animated_props"]["ball"]["path"] = "mesh/ball6.obj"
    assert not F.sequence_pose_frame(base, mesh)
    xf = F.sequence_pose_matrices(base, moved)
    assert xf.shape == (2, 12)
    assert np.array_equal(F.sequence_pose_matrices(base, copy()), np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (2, 1)))


# ---- meta["tri_part"] ------------------------------------------------------------------------------------------------
def test_tri_part_matches_the_prop_triangle_counts():
    a = S.bunny_scene(n=8, env_size=(64, 32), keep_order=True)
    part, order = a.meta["tri_part"], a.meta["tri_order"]
    assert part.shape == (a.n_tris,) and part.dtype == np.uint32
    assert np.bincount(part, minlength=3).tolist() == [12 * 8 * 8, 2, 2]
    # parse order is prop after prop
    assert np.array_equal(part, np.repeat(np.arange(3), [768, 2, 2])[order.astype(np.int64)])
    assert "tri_part" not in S.bunny_scene(n=8, env_size=(64, 32)).meta


# ---- NULL handles, no device -----------------------------------------------------------------------------------------
def test_null_scene_is_refused_without_a_device():
    lib = L.lib()
    one = np.zeros(12, np.float32)
    part = np.zeros(1, np.uint32)
    assert lib.fspt_scene_set_pose(None, L.u32ptr(part), 1, L.fptr(one), None) == -1
    assert lib.fspt_scene_update_transforms(None, L.fptr(one), 1) == -1
    assert lib.fspt_scene_read_pose(None, L.fptr(one), None) == -1
    assert lib.fspt_scene_last_pose_ms(None, None, None, None) == -1
    assert lib.fspt_multi_set_pose(None, L.u32ptr(part), 1, L.fptr(one), None) == -1
    assert lib.fspt_multi_update_transforms(None, L.fptr(one), 1) == -1
    assert lib.fspt_pose_matrices_eval(None, 1, L.fptr(one), None) == -1
