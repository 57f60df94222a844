"""The vertex-position update (fspt_scene_set_mesh / fspt_scene_update_vertices) without a GPU: tests/mesh_ref.py's
float64 restatement of obj_loader.js's normal rules equals the native builder - which tests/test_goldens.py pins against the
reference - bit for bit on meshes built from float32-exact OBJ text, fed the arrays fspt_builder_get_mesh reports; and the
entries refuse what the header says they refuse before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from fspt_amd import _lib as L
from fspt_amd import scene as S

import mesh_ref as R

E_INVALID, E_STATE = -1, -6  # include/fspt.h
PROP = {"path": "m.obj", "diffuse": [0.8, 0.6, 0.3], "emittance": [0, 0, 0]}


def build(mesh, normals):
    pos, faces, vts, face_vt = mesh
    text = R.obj_text(pos, faces, vts, face_vt)
    return S.build_scene([dict(PROP, normals=normals)], {"m.obj": text}, keep_order=True, keep_mesh=True, leaf_size=2)


def constant_vt(mesh):
    pos, faces, _, _ = mesh
    return pos, faces, np.array([[0.5, 0.5]]), [(0, 0, 0)] * len(faces)


TETRA = (np.array([[0, 0, 0], [1, 0, 0.125], [0.25, 1, 0], [0.5, 0.375, 1]], np.float32), [(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)],
         np.array([[0.1, 0.2], [0.8, 0.25], [0.4, 0.9], [0.6, 0.55]]), [(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)])
MESHES = {
    "one_triangle": R.strip_mesh(1),
    "tetrahedron": TETRA,
    "grid_5x5": R.grid_mesh(5, 5),
    "fan_65": R.fan_mesh(65),
    "constant_vt": constant_vt(R.grid_mesh(4, 3)),
    "folded_12": R.folded_pair((1, 2)),
    "folded_01": R.folded_pair((0, 1)),
}


@pytest.mark.parametrize("normals", ["flat", "smooth"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_restatement_equals_the_builder(name, normals):
    a = build(MESHES[name], normals)
    m = a.meta
    T = a.n_tris
    assert m["tri_vertex"].shape == (T, 3) and m["tri_uv64"].shape == (T, 6) and m["n_vertices"] == len(MESHES[name][0])
    assert np.array_equal(m["vertices"].view(np.uint32), np.asarray(MESHES[name][0], np.float32).view(np.uint32))
    assert np.array_equal(m["tri_smooth"], np.full(T, normals == "smooth", np.uint8)) and not m["tri_static"].any()
    tri, norm = R.mesh_ref(m["tri_vertex"], m["tri_uv64"], m["vertices"], smooth=m["tri_smooth"], rank=m["tri_order"])
    assert np.array_equal(tri.view(np.uint32).reshape(-1), a.tri.view(np.uint32).reshape(-1))
    assert R.same_bits_nan_by_position(norm, a.norm)
    nan = np.isnan(a.norm.reshape(T, 3, 9))
    if name == "folded_01" and normals == "smooth":
        # the quirk leaves a NaN in the record: the tangent and bitangent pushed by a corner whose test fired, one place late
        assert nan.any() and not nan[:, :, :3].any()
        assert np.array_equal(nan[:, :, 3:].all(axis=2), nan[:, :, 3:].any(axis=2))
    else:
        assert not nan.any()
    if name == "constant_vt":  # every corner took the fallback cross(n, (0, 1, 0))
        n64 = a.norm.reshape(T, 3, 9)[:, :, :3].astype(np.float64)
        assert np.allclose(a.norm.reshape(T, 3, 9)[:, :, 3], -n64[:, :, 2], atol=1e-6)
    if name == "folded_12" and normals == "smooth":
        n = a.norm.reshape(T, 3, 9)[:, :, :3]
        assert (n[:, 1:] == 0).all() and (n[:, 0] != 0).any()  # the mean at the shared vertices is exactly 0


def test_rank_is_the_order_of_the_sum():
    """a vertex of valence 65: its row holds every incident face once, in the order the OBJ's faces were parsed, whatever
    the leaf order; a face that names a vertex twice is there twice"""
    a = build(MESHES["fan_65"], "smooth")
    m = a.meta
    row_v, row_f = R.vertex_rows(m["tri_vertex"], m["tri_order"])
    assert row_v.size == 65 * 3 and np.array_equal(row_v, np.sort(row_v))
    centre = row_f[row_v == 0]
    assert np.array_equal(m["tri_order"][centre], np.arange(65)) and not np.array_equal(centre, np.arange(65))
    v2, f2 = R.vertex_rows([[0, 1, 0], [1, 0, 2]], [1, 0])
    assert v2.tolist() == [0, 0, 0, 1, 1, 2] and f2.tolist() == [1, 0, 0, 1, 0, 1]


def test_meta_marks_what_cannot_be_meshed():
    pos, faces, vts, fvt = R.grid_mesh(3, 3)
    texts = {"m.obj": R.obj_text(pos, faces, vts, fvt), "n.obj": R.obj_text(pos + np.float32(2), faces),
             "o.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvt 0.1 0.1\nvt 0.9 0.1\nvt 0.1 0.9\nf 1/1/1 2/2/1 3/3/1\n"}
    props = [dict(PROP, path="m.obj", normals="smooth"), dict(PROP, path="n.obj"), dict(PROP, path="o.obj", normals="mesh")]
    a = S.build_scene(props, texts, keep_order=True, keep_mesh=True)
    m = a.meta
    part = m["tri_part"]
    assert m["n_vertices"] == 9 + 9 + 3
    assert np.array_equal(m["tri_static"], part != 0) and np.array_equal(m["tri_smooth"], (part == 0).astype(np.uint8))
    assert np.isnan(m["tri_uv64"][part == 1]).all() and np.isfinite(m["tri_uv64"][part != 1]).all()
    for p, lo in ((0, 0), (1, 9), (2, 18)):  # the indices are global over the OBJs
        v = m["tri_vertex"][part == p]
        assert v.min() >= lo and v.max() < lo + (3 if p == 2 else 9)
    with pytest.raises(ValueError):
        S.build_scene(props, texts, keep_mesh=True)


def test_a_vertex_no_face_names_is_reported_where_the_loader_would_put_it():
    """meta["vertices"] can go back to update_vertices as it is: every entry is finite, used or not"""
    text = "v 0 0 0\nv 1 0 0\nv 5 6 7\nv 0 1 0\nvt 0.1 0.1\nvt 0.9 0.1\nvt 0.1 0.9\nf 1/1 2/2 4/3\nv 8 9 10\n"
    a = S.build_scene([dict(PROP, scale=2.0, translate=[1, 0, 0])], {"m.obj": text}, keep_order=True, keep_mesh=True)
    assert a.meta["n_vertices"] == 5 and a.meta["tri_vertex"].tolist() == [[0, 1, 3]]
    assert np.array_equal(a.meta["vertices"], np.float32([[1, 0, 0], [3, 0, 0], [11, 12, 14], [1, 2, 0], [17, 18, 20]]))
    b = S.build_scene([dict(PROP, scale=2.0, translate=[1, 0, 0])], {"m.obj": text}, keep_order=True, keep_mesh=True, normalize=1.0)
    assert np.isfinite(b.meta["vertices"]).all() and np.array_equal(b.meta["vertices"][[0, 1, 3]].reshape(-1), b.tri)


def desc(vertex, uv, nv, smooth=None, rank=None, tri=None, norm=None):
    vertex = np.ascontiguousarray(vertex, np.uint32).reshape(-1)
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1)
    keep = [vertex, uv]
    p = lambda a, t: None if a is None else (keep.append(a), a.ctypes.data_as(C.POINTER(t)))[1]
    smooth = None if smooth is None else np.ascontiguousarray(smooth, np.uint8)
    rank = None if rank is None else np.ascontiguousarray(rank, np.uint32)
    tri = None if tri is None else np.ascontiguousarray(tri, np.float32)
    norm = None if norm is None else np.ascontiguousarray(norm, np.float32)
    d = L.MeshDesc(L.u32ptr(vertex), nv, uv.ctypes.data_as(C.POINTER(C.c_double)), p(smooth, C.c_uint8), p(rank, C.c_uint32), p(tri, C.c_float), p(norm, C.c_float))
    return d, keep


def frames_eval_rc(d, T):
    """fspt_mesh_frames_eval validates the description before it looks for a device"""
    pos = np.zeros(64 * 3, np.float32)
    out = np.zeros(T * 36, np.float32)
    return L.lib().fspt_mesh_frames_eval(0, C.byref(d[0]), T, L.fptr(pos), L.fptr(out), None)


def test_set_mesh_refusals():
    lib = L.lib()
    V = [[0, 1, 2], [2, 1, 3]]
    UV = [[0.1, 0.1, 0.9, 0.1, 0.1, 0.9]] * 2
    S_ = L.MESH_STATIC
    rest_t, rest_n = np.ones((2, 9), np.float32), np.ones((2, 27), np.float32)
    bad_uv = [UV[0], [0.1, 0.1, np.nan, 0.1, 0.1, 0.9]]
    cases = {
        "n_vertices": desc(V, UV, 0),
        "index": desc(V, UV, 3),
        "partly static": desc([[0, 1, 2], [S_, 1, 3]], UV, 4, tri=rest_t, norm=rest_n),
        "uv": desc(V, bad_uv, 4),
        "rank": desc(V, UV, 4, rank=[5, 5]),
        "rest": desc([[0, 1, 2], [S_, S_, S_]], UV, 4),
        "rest norm": desc([[0, 1, 2], [S_, S_, S_]], UV, 4, tri=rest_t),
    }
    for name, d in cases.items():
        assert frames_eval_rc(d, 2) == E_INVALID, name
        assert lib.fspt_last_error().startswith(b"fspt_mesh_frames_eval: "), name
    assert b"partly static" in (frames_eval_rc(cases["partly static"], 2), lib.fspt_last_error())[1]
    assert b"rank 5" in (frames_eval_rc(cases["rank"], 2), lib.fspt_last_error())[1]
    # a static triangle's uv is not looked at (a triangle without vt reports NaN and can only be static)
    ok = desc([[0, 1, 2], [S_, S_, S_]], bad_uv, 4, tri=rest_t, norm=rest_n)
    assert frames_eval_rc(ok, 2) in (0, -2)  # FSPT_OK, or FSPT_E_NO_DEVICE: the description passed
    # NULL pointers, through the ABI's argument checks
    null_v = L.MeshDesc(None, 4, ok[0].uv, None, None, None, None)
    assert lib.fspt_mesh_frames_eval(0, C.byref(null_v), 2, None, None, None) == E_INVALID
    assert lib.fspt_mesh_frames_eval(0, None, 2, None, None, None) == E_INVALID
    assert lib.fspt_scene_set_mesh(None, C.byref(ok[0])) == E_INVALID and b"NULL scene" in lib.fspt_last_error()
    pos = np.zeros(12, np.float32)
    for fn in (lib.fspt_scene_update_vertices, lib.fspt_multi_update_vertices):
        assert fn(None, L.fptr(pos), 4) == E_INVALID
    assert lib.fspt_scene_update_vertices_device(None, None, 4) == E_INVALID
    assert lib.fspt_multi_set_mesh(None, None) == E_INVALID and lib.fspt_last_error() == b"fspt_multi_set_mesh: NULL handle"
    assert lib.fspt_scene_read_mesh(None, None, None) == E_INVALID
    assert lib.fspt_scene_last_mesh_ms(None, None, None, None, None) == E_INVALID
    assert lib.fspt_f64_probe_eval(0, 2, None, None, 0, None) == E_INVALID
    assert lib.fspt_builder_get_mesh(None, None, None, None, None) == E_STATE


def test_python_argument_checks():
    from fspt_amd.tracer import Scene
    a = build(MESHES["tetrahedron"], "flat")
    with pytest.raises(ValueError):
        Scene._mesh_desc("set_mesh", a, True, None, None, None, None, None, None, None, None)  # the scene has moved
    with pytest.raises(ValueError):
        Scene._mesh_desc("set_mesh", a, False, a.meta["tri_vertex"][:2], a.meta["tri_uv64"], None, None, None, None, None, None)
    with pytest.raises(ValueError):
        Scene._mesh_frame("update_vertices", np.zeros(7, np.float32), None)
    d, keep = Scene._mesh_desc("set_mesh", a, False, None, None, None, None, None, [True, False, False, False], None, None)
    assert d.n_vertices == 4 and keep[0][:3].tolist() == [L.MESH_STATIC] * 3 and bool(d.tri) and bool(d.norm)


def test_sequence_classification_and_positions():
    """render_sequence(mesh=True)'s two pure functions: which frames are the build frame with other `v` lines, and the
    positions such a frame hands to update_vertices"""
    from fspt_amd import scene_file as F
    pos, faces, vts, fvt = R.grid_mesh(3, 3)
    a = R.obj_text(pos, faces, vts, fvt)
    b = R.obj_text(pos + np.float32(0.25), faces, vts, fvt)
    floor = "v 0.5 0.0 0.5\nv 0.5 0.0 -0.5\nv -0.5 0.0 -0.5\nf 1 3 2\n"
    scene = lambda path, **kw: dict({"cameraPos": [0, 0, 2], "props": [dict(PROP, path=path), dict(PROP, path="floor.obj", scale=2.0, translate=[0, -0.5, 0])]}, **kw)
    base = scene("a.obj")
    assert F.sequence_mesh_frame(base, [a, floor], scene("b.obj"), [b, floor])
    assert F.sequence_mesh_frame(base, [a, floor], base, [a, floor])
    assert not F.sequence_mesh_frame(base, [a, floor], scene("b.obj", exposure=2.0), [b, floor])            # another setting
    assert not F.sequence_mesh_frame(base, [a, floor], scene("b.obj"), [b.replace("f 1/1", "f 2/2", 1), floor])  # another face
    assert not F.sequence_mesh_frame(base, [a, floor], scene("b.obj"), [b + "v 0 0 0\n", floor])             # another vertex count
    assert not F.sequence_mesh_frame(base, [a, floor], scene("b.obj"), [b])
    assert not F.sequence_mesh_frame(scene("a.obj", normalize=1.0), [a, floor], scene("b.obj", normalize=1.0), [b, floor])
    p = F.sequence_mesh_positions(scene("b.obj"), [b, floor])
    assert p.dtype == np.float32 and p.shape == (12, 3)
    assert np.array_equal(p[:9], pos + np.float32(0.25))  # an identity prop: the float32-exact `v` values themselves
    assert np.array_equal(p[9:], np.float32([[1, -0.5, 1], [1, -0.5, -1], [-1, -0.5, -1]]))
    # ... which are the builder's world positions
    arrays = S.build_scene(S.merge_scene_props(scene("b.obj")), {"b.obj": b, "floor.obj": floor}, keep_order=True, keep_mesh=True)
    assert np.array_equal(arrays.meta["vertices"], p)
