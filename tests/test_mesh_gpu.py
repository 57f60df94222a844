"""The vertex-position update (fspt_scene_set_mesh / fspt_scene_update_vertices) on the MI355X.  No tolerance
anywhere: float64 sqrt and / on the device are correctly rounded, the derive kernels equal tests/mesh_ref.py word for word
(NaNs by position: payloads differ between hosts and the GPU), and a scene given new vertex positions is indistinguishable
from a twin that was handed mesh_ref's arrays through update_geometry - frames of every pipeline, lights on and off, light
table, temporal reprojection."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as R
from fspt_amd import FsptError, MultiPathTracer, PathTracer, Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S
from test_mesh_cpu import desc

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H, TICKS = 48, 32, 3
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the probe: the contract needs float64 sqrt and / correctly rounded ------------------------------------------------
def hashed_u64(n, seed):
    x = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    for m in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        x ^= x >> np.uint64(33)
        x *= np.uint64(m)
    return x ^ (x >> np.uint64(33))


def probe_operands(n, seed):
    """doubles with hashed mantissas over the whole exponent range, subnormals, and the values normalize() meets"""
    raw = hashed_u64(n, seed)
    full = (raw & np.uint64(0x7FFFFFFFFFFFFFFF)).view(np.float64)           # any exponent, subnormal operands included
    near1 = ((raw & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    sub = (raw & np.uint64(0x000FFFFFFFFFFFFF)).view(np.float64)            # subnormal
    small = near1 * 2.0 ** -1022                                             # products / quotients land in the subnormals
    out = np.concatenate([full[: n // 4], near1[n // 4: n // 2], sub[n // 2: 5 * n // 8], small[5 * n // 8: 3 * n // 4],
                          (near1 * near1)[3 * n // 4:]])
    return out[np.isfinite(out)]


def probe(op, a, b=None):
    a = np.ascontiguousarray(a, np.float64)
    b = None if b is None else np.ascontiguousarray(b, np.float64)
    out = np.zeros_like(a)
    p = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))
    L.check(L.lib().fspt_f64_probe_eval(0, op, p(a), p(b), a.size, p(out)))
    return out


def test_f64_sqrt_and_division_are_correctly_rounded():
    a, b = probe_operands(100_000, 1), probe_operands(100_000, 2)
    n = min(a.size, b.size)
    a, b = a[:n], b[:n]
    got = probe(0, a)
    assert np.array_equal(got.view(np.uint64), np.sqrt(a).view(np.uint64)), int((got.view(np.uint64) != np.sqrt(a).view(np.uint64)).sum())
    ones = np.ones_like(a)
    with np.errstate(all="ignore"):
        for x, y in ((a, b), (ones, a), (a * 2.0 ** -1000, b * 2.0 ** 20), (ones, np.arange(1.0, n + 1.0))):
            want = x / y
            got = probe(1, x, y)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got.view(np.uint64) != want.view(np.uint64)).sum())
        sub = (a * 2.0 ** -1000) / (b * 2.0 ** 20)
        assert ((sub != 0) & (np.abs(sub) < 2.0 ** -1022)).any()  # subnormal results are among them


# ---- the derive kernels against the restatement -----------------------------------------------------------------------
def frames_eval(vertex, uv, pos, smooth=None, rank=None, tri=None, norm=None):
    vertex = np.asarray(vertex, np.uint32).reshape(-1, 3)
    T = vertex.shape[0]
    pos = np.ascontiguousarray(pos, np.float32)
    d, keep = desc(vertex, uv, pos.shape[0], smooth, rank, tri, norm)
    out_t, out_n = np.zeros((T, 9), np.float32), np.zeros((T, 27), np.float32)
    L.check(L.lib().fspt_mesh_frames_eval(0, C.byref(d), T, L.fptr(pos), L.fptr(out_t), L.fptr(out_n)))
    return out_t, out_n


def mesh_arrays(mesh):
    pos, faces, vts, fvt = mesh
    uv = np.asarray(vts, np.float64)[np.asarray(fvt).reshape(-1)].reshape(-1, 6)
    return np.asarray(faces, np.uint32), uv, np.asarray(pos, np.float32)


def scrambled_rank(T):
    return np.argsort(hashed_u64(T, 5), kind="stable").astype(np.uint32)


# (the kernels hold 21 triangles per wave and 84 per block: 21 / 22 and 84 / 85 are their own edges)
MESHES = {"T1": R.strip_mesh(1), "T4": R.strip_mesh(4), "T255": R.strip_mesh(255), "T256": R.strip_mesh(256), "T257": R.strip_mesh(257),
          "T21": R.strip_mesh(21), "T22": R.strip_mesh(22), "T84": R.strip_mesh(84), "T85": R.strip_mesh(85),
          "grid5": R.grid_mesh(5, 5), "fan63": R.fan_mesh(63), "fan64": R.fan_mesh(64), "fan65": R.fan_mesh(65), "fan257": R.fan_mesh(257)}


@pytest.mark.parametrize("flags", ("flat", "smooth", "mixed"))
@pytest.mark.parametrize("name", sorted(MESHES))
def test_frame_arrays_equal_the_restatement(name, flags):
    vertex, uv, pos = mesh_arrays(MESHES[name])
    T = vertex.shape[0]
    smooth = {"flat": None, "smooth": np.ones(T, np.uint8), "mixed": (hashed_u64(T, 9) & np.uint64(1)).astype(np.uint8)}[flags]
    for rank in (None, scrambled_rank(T)):
        for k in range(2):  # the rest positions, and a hashed deformation of them
            p = pos + np.float32(0.1 * k) * R.hashed(pos.size, 20 + k).reshape(pos.shape)
            want = R.mesh_ref(vertex, uv, p, smooth, rank)
            got = frames_eval(vertex, uv, p, smooth, rank)
            assert np.array_equal(bits(got[0]), bits(want[0])), (rank is None, k)
            assert R.same_bits_nan_by_position(got[1], want[1]), (rank is None, k, int((bits(got[1]) != bits(want[1])).sum()))
            assert np.isfinite(want[1]).all()


def test_constant_vt_takes_the_fallback_everywhere():
    vertex, _, pos = mesh_arrays(R.grid_mesh(6, 5))
    T = vertex.shape[0]
    uv = np.full((T, 6), 0.5)
    for smooth in (None, np.ones(T, np.uint8)):
        want = R.mesh_ref(vertex, uv, pos, smooth)
        got = frames_eval(vertex, uv, pos, smooth)
        assert np.isfinite(want[1]).all() and np.array_equal(bits(got[1]), bits(want[1]))
        n = want[1].reshape(T, 3, 9)
        assert np.array_equal(n[:, :, 3], -n[:, :, 2])  # cross(n, (0, 1, 0)).x = -n.z


def nan_pattern_mesh(pattern):
    """One smooth triangle (p0, p1, p2) whose corners in `pattern` sit on vertices with a zero vertex normal: each such vertex
    is shared with a partner triangle over the points (p0, p2, p1) - the same two edge vectors swapped, so its normal is the
    exact negative - whose other two corners are vertices of their own, so nothing else is disturbed."""
    base = np.array([[0, 0, 0], [1, 0, 0.25], [0.25, 1, 0]], np.float32)
    pos = [p for p in base]
    faces = [(0, 1, 2)]
    place = {0: 0, 1: 2, 2: 1}  # where point j sits in the partner
    for c in sorted(pattern):
        f = [0, 0, 0]
        for j in range(3):
            if j == c:
                f[place[j]] = c
            else:
                f[place[j]] = len(pos)
                pos.append(base[j])
        faces.append(tuple(f))
    pos = np.asarray(pos, np.float32)
    vts = np.stack([pos[:, 0] * 0.5 + 0.2, pos[:, 1] * 0.6 + 0.1], axis=1).astype(np.float64)
    return pos, faces, vts, faces


# what obj_loader.js:93-99 leaves in entries 0..2, replayed by hand: the corner of the main triangle that keeps a NaN
NAN_PATTERNS = {(2,): None, (1, 2): None, (0, 1, 2): None, (0,): 1, (1,): 2, (0, 1): 2, (0, 2): 1}


@pytest.mark.parametrize("pattern", sorted(NAN_PATTERNS))
def test_every_nan_pattern_of_the_quirk(pattern):
    vertex, uv, pos = mesh_arrays(nan_pattern_mesh(pattern))
    T = vertex.shape[0]
    smooth = np.ones(T, np.uint8)
    want = R.mesh_ref(vertex, uv, pos, smooth)
    got = frames_eval(vertex, uv, pos, smooth)
    assert np.array_equal(bits(got[0]), bits(want[0])) and R.same_bits_nan_by_position(got[1], want[1])
    main = np.isnan(want[1].reshape(T, 3, 9)[0])
    n0 = want[1].reshape(T, 3, 9)[0, :, :3]
    assert [c for c in range(3) if not n0[c].any()] == list(pattern)  # exactly those corners have a zero normal
    left = NAN_PATTERNS[pattern]
    assert main[:, :3].sum() == 0
    assert [c for c in range(3) if main[c, 3:].any()] == ([] if left is None else [left])


def test_static_triangles_keep_their_rest_bytes():
    vertex, uv, pos = mesh_arrays(R.grid_mesh(5, 5))
    T = vertex.shape[0]
    static = (hashed_u64(T, 3) % np.uint64(3) == 0)
    assert static.any() and not static.all()
    rest_t = R.hashed(T * 9, 40).reshape(T, 9)
    rest_n = R.hashed(T * 27, 41).reshape(T, 27)
    v = vertex.copy(); v[static] = R.STATIC
    uvs = uv.copy(); uvs[static] = np.nan  # (not looked at)
    smooth = np.ones(T, np.uint8)
    want = R.mesh_ref(v, uvs, pos, smooth, None, rest_t, rest_n)
    got = frames_eval(v, uvs, pos, smooth, None, rest_t, rest_n)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[0][static]), bits(rest_t[static])) and np.array_equal(bits(got[1][static]), bits(rest_n[static]))
    # a static triangle is not incident to its former vertices: the neighbours' means differ from the all-meshed ones
    assert not np.array_equal(bits(got[1][~static]), bits(R.mesh_ref(vertex, uv, pos, smooth)[1][~static]))


# ---- a scene ----------------------------------------------------------------------------------------------------------
def cloth_scene(grid=9, fan=9, shuffle=False):
    """a smooth grid x grid cloth, a flat fan, and - static, they have no vt - a floor and a small emitter; shuffle: the
    cloth's faces in a hashed order"""
    pos, faces, vts, fvt = R.grid_mesh(grid, grid, seed=7)
    if shuffle:
        perm = np.argsort(hashed_u64(len(faces), 11), kind="stable")
        faces, fvt = np.asarray(faces)[perm], np.asarray(fvt)[perm]
    cloth = R.obj_text((pos - np.float32([0.5, 0.5, 0.0])) * np.float32(1.4), faces, vts, fvt)
    fpos, ffaces, fvts, ffvt = R.fan_mesh(fan)
    fan = R.obj_text(fpos * np.float32(0.4) + np.float32([0.9, 0.2, 0.3]), ffaces, fvts, ffvt)
    quad = "v 0.5 0.0 0.5\nv 0.5 0.0 -0.5\nv -0.5 0.0 -0.5\nv -0.5 0.0 0.5\nf 1 3 2\nf 3 1 4\n"
    lamp = "mtllib lamp.mtl\nusemtl lamp\n" + quad
    props = [
        {"path": "m/cloth.obj", "normals": "smooth", "diffuse": [0.8, 0.5, 0.3], "emittance": [0, 0, 0], "rotate": [{"angle": -0.9, "axis": [1, 0, 0]}]},
        {"path": "m/fan.obj", "normals": "flat", "diffuse": [0.3, 0.6, 0.8], "emittance": [0, 0, 0]},
        {"path": "m/quad.obj", "scale": 5, "translate": [0, -0.9, 0], "diffuse": [0.6, 0.6, 0.6], "emittance": [0, 0, 0]},
        {"path": "m/lamp.obj", "scale": 0.6, "translate": [0.2, 1.4, 0.2], "rotate": [{"angle": 3.14159265, "axis": [1, 0, 0]}], "emittance": [1, 1, 1]},
    ]
    env, w, h = S.synthetic_env(64, 32)
    return S.build_scene(props, {"m/cloth.obj": cloth, "m/fan.obj": fan, "m/quad.obj": quad, "m/lamp.obj": lamp}, mtl_texts={"m/lamp.mtl": "newmtl lamp\nkd 1 1 1\nkem 6 5.5 4.5\n"},
                         env=env, env_w=w, env_h=h, keep_order=True, keep_mesh=True)


@pytest.fixture(scope="module")
def cloth():
    a = cloth_scene()
    m = a.meta
    assert m["tri_static"].sum() == 4 and m["tri_smooth"].sum() == 128 and a.n_tris == 128 + 9 + 4
    return a


def deformed(arrays, k):
    """hashed deformation k of the scene's vertices (float32), and what mesh_ref makes of it in leaf order `order`"""
    v = arrays.meta["vertices"]
    return (v + np.float32(0.06) * R.hashed(v.size, 50 + k).reshape(v.shape)).astype(np.float32)


def reference(arrays, pos, order=None):
    m = arrays.meta
    sel = np.arange(arrays.n_tris) if order is None else np.asarray(order, np.int64)
    vertex = m["tri_vertex"].copy()
    vertex[m["tri_static"]] = R.STATIC
    return R.mesh_ref(vertex[sel], m["tri_uv64"][sel], pos, m["tri_smooth"][sel], m["tri_order"][sel],
                      arrays.tri.reshape(-1, 9)[sel], arrays.norm.reshape(-1, 27)[sel])


def make_pt(sc, pipeline="wavefront", lights=False, seed=7):
    pt = PathTracer(sc, W, H, num_bounces=4)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if lights:
        pt.set_lights("emitters", 0.5)
    return pt


def again(pt, n=TICKS, seed=7):
    pt.clear(); pt.seed(seed); pt.render(n)
    return pt.readRadiance()


def frame(sc, **kw):
    pt = make_pt(sc, **kw)
    pt.render(TICKS)
    img = pt.readRadiance()
    pt.close()
    return img


def test_updated_scene_equals_the_reference_and_its_twin(cloth):
    A, B = Scene(cloth), Scene(cloth)
    tracers = [(make_pt(A, pipeline=p, lights=l), make_pt(B, pipeline=p, lights=l)) for p in ("megakernel", "wavefront") for l in (False, True)]
    try:
        A.set_mesh()
        assert A.last_mesh["bytes"] > 0
        f_rest = again(tracers[0][0])
        for k in range(3):
            pos = deformed(cloth, k)
            want_t, want_n = reference(cloth, pos)
            assert np.isfinite(want_n).all()
            A.update_vertices(pos)
            got_t, got_n = A.read_mesh()
            assert np.array_equal(bits(got_t), bits(want_t)) and np.array_equal(bits(got_n), bits(want_n)), k
            st = cloth.meta["tri_static"]
            assert np.array_equal(bits(got_t[st]), bits(cloth.tri.reshape(-1, 9)[st]))
            B.update_geometry(want_t, want_n)
            assert A.sah_cost() == B.sah_cost()
            ta, tb = A.light_table(), B.light_table()
            assert len(tb["tris"]) and all(np.array_equal(ta[key].view(np.uint8), tb[key].view(np.uint8)) for key in tb)
            for pa, pb in tracers:
                fa, fb = again(pa), again(pb)
                assert np.array_equal(fa, fb) and np.isfinite(fa).all(), k
            assert not np.array_equal(fa, f_rest) or k
        ms = A.last_mesh
        assert ms["launches"] >= 5 and ms["derive_ms"] > 0 and ms["refit_ms"] > 0
    finally:
        for pa, pb in tracers:
            pa.close(); pb.close()
        A.close(); B.close()


def test_device_form_equals_the_host_form(cloth):
    import torch
    pos = deformed(cloth, 1)
    A, B = Scene(cloth), Scene(cloth)
    A.set_mesh(); B.set_mesh()
    A.update_vertices(pos)
    d_pos = torch.from_numpy(pos).to("cuda:0") * 1.0  # (computed on the device)
    B.update_vertices(d_pos)
    for a, b in zip(A.read_mesh(), B.read_mesh()):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(frame(A), frame(B))
    with pytest.raises(TypeError):
        B.update_vertices(d_pos.double())
    with pytest.raises(FsptError) as ei:
        B.update_vertices(d_pos[:-1].contiguous())
    assert ei.value.code == -1
    A.close(); B.close()


def test_rebuild_permutes_the_mesh(cloth):
    T = cloth.n_tris
    A, B = Scene(cloth), Scene(cloth)
    A.set_mesh()
    p1, p2 = deformed(cloth, 1), deformed(cloth, 2)
    A.update_vertices(p1)
    t1, n1 = A.read_mesh()
    order = A.rebuild_geometry(t1, n1).astype(np.int64)
    assert np.array_equal(B.rebuild_geometry(t1, n1), order) and not np.array_equal(order, np.arange(T))
    with pytest.raises(FsptError) as ei:
        A.read_mesh()  # the staging array is the rebuild's
    assert ei.value.code == -6
    A.update_vertices(p2)  # nothing from the caller: the scene permuted indices, constants, face ids and the rest copy
    want_t, want_n = reference(cloth, p2, order)
    assert np.array_equal(S.compose_order(cloth.meta["tri_order"], order), cloth.meta["tri_order"][order])
    got_t, got_n = A.read_mesh()
    assert np.array_equal(bits(got_t), bits(want_t)) and np.array_equal(bits(got_n), bits(want_n))
    B.update_geometry(want_t, want_n)
    for pipeline in ("megakernel", "wavefront"):
        assert np.array_equal(frame(A, pipeline=pipeline), frame(B, pipeline=pipeline))
    with pytest.raises(ValueError):
        A.set_mesh()  # the meta's order is no longer the scene's
    A.close(); B.close()


def test_mesh_pose_and_skin_alternate(cloth):
    import pose_ref as PR
    import skin_ref as SR
    T = cloth.n_tris
    rest_t, rest_n = cloth.tri.reshape(-1, 9), cloth.norm.reshape(-1, 27)
    part = (hashed_u64(T, 3) % np.uint64(2)).astype(np.uint32)
    xp = np.float32([[1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, 0], [0.9, 0, 0, 0, 0, 1.1, 0, 0, 0, 0, 1, 0.02]])
    joints = np.zeros((T, 3, 4), np.uint16)
    weights = np.zeros((T, 3, 4), np.float32); weights[..., 0] = 1
    xs = np.float32([[1, 0, 0, 0, 0, 1, 0, 0.03, 0, 0, 1, 0]])
    A, B = Scene(cloth), Scene(cloth)
    A.set_mesh(); A.set_pose(part, n_parts=2); A.set_skin(joints, weights)
    for read in (A.read_mesh, A.read_pose, A.read_skin):
        with pytest.raises(FsptError) as ei:
            read()
        assert ei.value.code == -6
    pos = deformed(cloth, 0)
    steps = [("mesh", lambda: A.update_vertices(pos), A.read_mesh, lambda: reference(cloth, pos)),
             ("pose", lambda: A.update_transforms(xp), A.read_pose, lambda: PR.pose(part, rest_t, rest_n, xp)),
             ("mesh", lambda: A.update_vertices(pos), A.read_mesh, lambda: reference(cloth, pos)),
             ("skin", lambda: A.update_skin(xs), A.read_skin, lambda: SR.skin(joints, weights, rest_t, rest_n, xs))]
    for _ in range(2):
        for name, run, read, ref in steps:
            run()
            want, got = ref(), read()
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), name
            for other, r in (("mesh", A.read_mesh), ("pose", A.read_pose), ("skin", A.read_skin)):
                if other != name:
                    with pytest.raises(FsptError) as ei:
                        r()
                    assert ei.value.code == -6 and f"fspt_scene_read_{other}" in str(ei.value)
            B.update_geometry(*want)
            assert np.array_equal(frame(A), frame(B)), name
    A.update_vertices(pos)
    A.update_geometry(rest_t, rest_n)  # a host upload reuses the array too
    with pytest.raises(FsptError):
        A.read_mesh()
    A.close(); B.close()


def test_rebuild_permutes_all_three_deformers():
    """T = 257: odd, one past a 256-thread block of k_rebuild_permute at one word per triangle, no multiple of the derive
    kernels' 21 triangles per wave.  Pose, skin (two morph targets with morph_norm) and mesh are set at once; one rebuild
    permutes every array that follows the triangles, and each deformer then works with nothing from the caller."""
    import pose_ref as PR
    import skin_ref as SR
    arrays = cloth_scene(grid=11, fan=53, shuffle=True)
    T, m = arrays.n_tris, arrays.meta
    assert T == 257 and m["tri_static"].sum() == 4 and m["tri_smooth"].sum() == 200
    rest_t, rest_n = arrays.tri.reshape(-1, 9), arrays.norm.reshape(-1, 27)
    part = (hashed_u64(T, 3) % np.uint64(3)).astype(np.uint32)
    xp = np.float32([[1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, 0], [0.9, 0, 0, 0, 0, 1.1, 0, 0, 0, 0, 1, 0.02], [0, -1, 0, 0, 1.2, 0.3, 0, 0.1, 0, 0, 1, 0]])
    joints = (hashed_u64(T * 12, 4) % np.uint64(5)).astype(np.uint16).reshape(T, 3, 4)
    raw = (hashed_u64(T * 12, 5) % np.uint64(1000)).astype(np.float64).reshape(-1, 4) + 1.0
    weights = (raw / raw.sum(1, keepdims=True)).astype(np.float32).reshape(T, 3, 4)
    morph = (np.float32(0.03) * R.hashed(2 * T * 9, 21)).reshape(2, T, 9)
    mnorm = (np.float32(0.1) * R.hashed(2 * T * 27, 22)).reshape(2, T, 27)
    xs = np.float32([[1, 0, 0, 0.01 * k, 0.1 * k, 1, 0, 0.03, 0, 0, 1 - 0.05 * k, 0] for k in range(5)])
    mw = np.float32([0.6, -0.25])
    pos = deformed(arrays, 0)
    A = Scene(arrays)
    A.set_mesh(); A.set_pose(part, n_parts=3); A.set_skin(joints, weights, morph=morph, morph_norm=mnorm)
    held = A.last_skin["bytes"], A.last_mesh["bytes"]
    assert held[0] == T * 216 + 2 * T * 144 + 5 * 48 + 2 * 4 and held[1] > 0
    order = A.rebuild_geometry(rest_t, rest_n).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(T)) and not np.array_equal(order, np.arange(T))
    reads = (("pose", A.read_pose), ("skin", A.read_skin), ("mesh", A.read_mesh))
    for _, read in reads:
        with pytest.raises(FsptError) as ei:
            read()  # the staging array is the rebuild's
        assert ei.value.code == -6
    steps = [("pose", lambda: A.update_transforms(xp), lambda: PR.pose(part[order], rest_t[order], rest_n[order], xp)),
             ("skin", lambda: A.update_skin(xs, mw), lambda: SR.skin(joints[order], weights[order], rest_t[order], rest_n[order], xs, morph[:, order], mnorm[:, order], mw)),
             ("mesh", lambda: A.update_vertices(pos), lambda: reference(arrays, pos, order))]
    for name, run, ref in steps:
        want = ref()
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), name  # (else the refit would refuse the frame)
        run()
        for other, read in reads:
            if other != name:
                with pytest.raises(FsptError) as ei:
                    read()
                assert ei.value.code == -6 and f"fspt_scene_read_{other}" in str(ei.value)
        got = dict(reads)[name]()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), name
    assert (A.last_skin["bytes"], A.last_mesh["bytes"]) == held
    A.close()


def test_recorded_ticks_run_before_the_update(cloth):
    pos = deformed(cloth, 1)
    out = []
    for sync_first in (False, True):
        sc = Scene(cloth); sc.set_mesh()
        pt = make_pt(sc)
        for _ in range(3):
            pt.tick()
        if sync_first:
            pt.sync()
        pt.update_vertices(pos)
        for _ in range(3):
            pt.tick()
        out.append(pt.readRadiance())
        pt.close(); sc.close()
    assert np.array_equal(out[0], out[1])
    sc = Scene(cloth); pt = make_pt(sc)
    for _ in range(6):
        pt.tick()
    assert not np.array_equal(pt.readRadiance(), out[0])  # neither all-old nor all-new
    pt.close(); sc.close()


def test_errors_leave_the_scene_unchanged(cloth):
    m = cloth.meta
    sc = Scene(cloth)
    pt = make_pt(sc)
    f0 = again(pt)
    pos = deformed(cloth, 1)
    assert sc.last_mesh["bytes"] == 0
    with pytest.raises(FsptError) as ei:
        sc.update_vertices(pos)  # no mesh
    assert ei.value.code == -6
    with pytest.raises(FsptError) as ei:
        sc.set_mesh(m["tri_vertex"], m["tri_uv64"], m["n_vertices"], m["tri_smooth"], m["tri_order"])  # the static ones have no vt
    assert ei.value.code == -1 and "uv[" in str(ei.value)
    with pytest.raises(FsptError) as ei:
        sc.set_mesh(n_vertices=5)
    assert ei.value.code == -1 and "vertex[" in str(ei.value)
    with pytest.raises(FsptError) as ei:
        sc.update_vertices(pos)  # still no mesh
    assert ei.value.code == -6
    sc.set_mesh()
    collapsed = pos.copy()
    v = m["tri_vertex"][np.nonzero(~m["tri_static"])[0][0]]
    collapsed[v[1]] = collapsed[v[0]]  # a face of zero area: its normal is 0 * inf
    nan = pos.copy(); nan[v[2], 1] = np.nan
    for what, p in (("count", pos[:-1]), ("nan", nan), ("collapsed", collapsed)):
        with pytest.raises(FsptError) as ei:
            sc.update_vertices(p)
        assert ei.value.code == -1, what
        if what == "collapsed":
            assert "not finite" in str(ei.value)
        assert np.array_equal(again(pt), f0), what
        with pytest.raises(FsptError) as ei:
            sc.read_mesh()  # nothing has been accepted yet: what the refit's check refused is not handed out
        assert ei.value.code == -6, what
    import torch
    with pytest.raises(FsptError) as ei:
        sc.update_vertices(torch.from_numpy(collapsed).to("cuda:0"))  # no host check: the refit's check refuses the result
    assert ei.value.code == -1 and np.array_equal(again(pt), f0)
    sc.update_vertices(pos)  # and the mesh still works
    f1 = again(pt)
    assert not np.array_equal(f1, f0)
    want = reference(cloth, pos)
    assert np.array_equal(bits(sc.read_mesh()[1]), bits(want[1]))
    with pytest.raises(FsptError):
        sc.update_vertices(collapsed)  # refused after an accepted frame: the scene keeps that frame, read_mesh has nothing
    assert np.array_equal(again(pt), f1)
    with pytest.raises(FsptError) as ei:
        sc.read_mesh()
    assert ei.value.code == -6
    sc.update_vertices(pos)
    assert np.array_equal(bits(sc.read_mesh()[1]), bits(want[1]))
    sc.set_mesh(drop=True)
    assert sc.last_mesh["bytes"] == 0
    with pytest.raises(FsptError) as ei:
        sc.update_vertices(pos)
    assert ei.value.code == -6
    sc.set_mesh(drop=True)  # dropping twice is fine
    pt.close(); sc.close()


def test_a_scene_that_is_not_refittable_takes_no_mesh(cloth):
    """two leaves that share a triStart (tests/test_refit_gpu.py): the scene renders, but cannot be refitted - set_mesh
    refuses it with FSPT_E_STATE, update_vertices then finds no mesh, and the scene renders as before"""
    import dataclasses
    bvh = cloth.bvh.copy().reshape(-1, 9)
    w = bvh[:, :3].view(np.int32)
    leaves = np.flatnonzero(w[:, 2] > -1)
    w[leaves[1], 2] = w[leaves[0], 2]
    sc = Scene(dataclasses.replace(cloth, bvh=bvh.reshape(-1)))
    pt = make_pt(sc)
    f0 = again(pt)
    with pytest.raises(FsptError) as ei:
        sc.set_mesh()
    assert ei.value.code == -6 and "fspt_scene_set_mesh: scene is not refittable" in str(ei.value)
    assert sc.last_mesh["bytes"] == 0
    import torch
    for pos in (deformed(cloth, 1), torch.from_numpy(deformed(cloth, 1)).to("cuda:0")):
        with pytest.raises(FsptError) as ei:
            sc.update_vertices(pos)
        assert ei.value.code == -6
    assert np.array_equal(again(pt), f0) and np.isfinite(f0).all() and f0[..., :3].max() > 0
    pt.close(); sc.close()


def test_multi_update_vertices(cloth):
    pos = deformed(cloth, 2)
    mp = MultiPathTracer(cloth, W, H, devices=(0, 0), num_bounces=4)
    mp.set_camera(**CAM); mp.seed(7)
    mp.set_mesh()
    mp.update_vertices(pos)
    mp.render(TICKS)
    got = mp.readRadiance()
    mp.close()
    B = Scene(cloth)
    B.update_geometry(*reference(cloth, pos))
    assert np.array_equal(got, frame(B))
    B.close()


def test_temporal_reprojection_follows_the_vertices(cloth):
    pos = deformed(cloth, 1)
    tri, norm = reference(cloth, pos)
    out = []
    for meshed in (True, False):
        sc = Scene(cloth)
        pt = make_pt(sc)
        pt.render(TICKS)
        pt.temporal_accumulate()
        sc.motion_begin()
        if meshed:
            sc.set_mesh(); sc.update_vertices(pos)
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


def test_gpu_light_builder_sees_the_same_table(cloth):
    pos = deformed(cloth, 0)
    A, B = Scene(cloth), Scene(cloth)
    pa, pb = make_pt(A, lights=True), make_pt(B, lights=True)
    A.set_light_builder("gpu"); B.set_light_builder("gpu")
    A.set_mesh(); A.update_vertices(pos)
    B.update_geometry(*reference(cloth, pos))
    ta, tb = A.light_table(), B.light_table()
    assert len(tb) and all(np.array_equal(ta[k].view(np.uint8), tb[k].view(np.uint8)) for k in tb)
    assert np.array_equal(again(pa), again(pb))
    pa.close(); pb.close(); A.close(); B.close()


# ---- render_sequence ----------------------------------------------------------------------------------------------------
def _write_frames(tmp_path, n_frames, recolour=None):
    """hand-written frames: a smooth cloth (an identity prop with float32-exact `v` lines, one OBJ per frame) over a floor
    that has no vt"""
    import json
    root = tmp_path / "web"
    (root / "scene").mkdir(parents=True); (root / "mesh").mkdir()
    (root / "mesh" / "floor.obj").write_text("v 0.5 0.0 0.5\nv 0.5 0.0 -0.5\nv -0.5 0.0 -0.5\nv -0.5 0.0 0.5\nf 1 3 2\nf 3 1 4\n")
    (root / "mesh" / "cloth.mtl").write_text("newmtl glow\nkd 0.8 0.3 0.2\nkem 0.9 0.7 0.5\n")  # the scene's light: it has no environment
    pos, faces, vts, fvt = R.grid_mesh(7, 7, seed=11)
    # beside the camera's central ray, which also passes over the floor's far edge: the auto-focus ray misses in both paths
    # (the mesh path shoots it through Scene.intersect in float32, the parse path through the builder in float64)
    pos = (pos - np.float32([0.5, 0.3, 0.0])) * np.float32(1.5) + np.float32([0.85, 0.0, 0.0])
    for f in range(n_frames):
        p = pos + np.float32(0.05 * f) * R.hashed(pos.size, 70).reshape(pos.shape)
        (root / "mesh" / f"cloth_{f}.obj").write_text("mtllib cloth.mtl\nusemtl glow\n" + R.obj_text(p, faces, vts, fvt))
        scene = {"cameraPos": [0.0, 0.5, 2.4], "cameraDir": [0.0, -0.2, -1.0], "samples": 16, "exposure": 1.2,
                 "static_props": [{"path": "mesh/floor.obj", "scale": 4.0, "translate": [0, -0.6, 0], "emittance": [0, 0, 0],
                                   "diffuse": [0.2, 0.5, 0.7] if f == recolour else [0.7, 0.7, 0.6]}],
                 "animated_props": [{"path": f"mesh/cloth_{f}.obj", "diffuse": [0.8, 0.3, 0.2], "emittance": [3, 3, 3], "normals": "smooth"}]}
        (root / "scene" / f"anim_{f}.json").write_text(json.dumps(scene))
    return str(root / "scene" / "anim_{frame}.json"), str(root)


def test_render_sequence_mesh(tmp_path):
    """The mesh path against the parse path.  The cloth's prop is the identity and its `v` values are float32-exact, so both
    paths hold the same positions and - the derive kernels being the builder's arithmetic - write the same files.  That
    holds for the geometry; the frames are also laid out so that the auto-focus ray misses in both paths (_write_frames):
    where it hits, the mesh path's float32 Scene.intersect and the parse path's float64 builder can give focus settings
    that differ in the last bits, and then the pictures carry different noise - not covered here."""
    import os
    from fspt_amd import scene_file as F
    pattern, root = _write_frames(tmp_path, 4, recolour=2)
    log, log2 = [], []
    got = F.render_sequence(pattern, range(4), str(tmp_path / "mesh" / "{frame}.png"), W, H, root, bvh="refit", mesh=True,
                            on_frame=lambda f, how: log.append(how))
    want = F.render_sequence(pattern, range(4), str(tmp_path / "parse" / "{frame}.png"), W, H, root, bvh="refit",
                             on_frame=lambda f, how: log2.append(how))
    # frame 2 recolours the floor: the parse path, after which the mesh path rests
    assert log == ["build", "mesh", "appearance", "appearance"] and log2[0] == "build" and "build" not in log2[1:]
    assert len(got) == 4 and all(os.path.exists(p) for p in got)
    for a, b in zip(got, want):
        assert open(a, "rb").read() == open(b, "rb").read()
    from PIL import Image
    a, b = (np.asarray(Image.open(p), np.float64) for p in got[:2])
    assert a.max() > 0 and np.abs(a - b).mean() > 0.5  # lit, and the frames do differ
    with pytest.raises(ValueError):
        F.render_sequence(pattern, range(1), str(tmp_path / "x" / "{frame}.png"), W, H, root, bvh="sah", mesh=True)
