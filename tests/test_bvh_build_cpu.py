"""CPU checks of the opt-in binned-SAH builder (fspt_builder_build_gpu): the numpy restatement's own
invariants on the test scenes and on degenerate soups the reference's builder cannot handle; the C entry point's argument
and state errors, which it returns before any device call; the Python host's option; and the JS host's buildScene({bvh:
'gpu'}) through the addon built against tests/napi_mock."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bvh_binned_ref as BR
import rays as R
from fspt_amd import _lib as L, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_STATE = -1, -2, -6  # include/fspt.h


def check_restatement(arrays):
    """arrays built by the reference's builder with keep_order=True; the restatement's tree over the same triangles"""
    g = BR.geometry_order(arrays)
    t = BR.build(g["tri"], arrays.leaf_size)
    BR.check_tree(t.bvh, g["tri"][t.order], arrays.leaf_size, t.depth)
    assert np.array_equal(np.sort(t.order), np.arange(arrays.n_tris))
    # the children of every interior node split its range, both non-empty; a median split only where SAH had no taker
    interior = np.flatnonzero(t.left >= 0)
    assert np.array_equal(t.lo[t.left[interior]], t.lo[interior])
    assert np.array_equal(t.cnt[t.left[interior]] + t.cnt[t.right[interior]], t.cnt[interior])
    assert (t.cnt[t.left[interior]] > 0).all() and (t.cnt[t.right[interior]] > 0).all()
    assert (t.cnt[t.left < 0] <= arrays.leaf_size).all() and (t.cnt[interior] > arrays.leaf_size).all()
    med = interior[~t.sah_split[interior]]
    assert np.array_equal(t.cnt[t.left[med]], t.cnt[med] // 2)
    # deterministic
    t2 = BR.build(g["tri"], arrays.leaf_size)
    assert np.array_equal(t.bvh.view(np.uint32), t2.bvh.view(np.uint32)) and np.array_equal(t.order, t2.order)
    return t


def test_restatement_small_and_medium():
    for n, env in ((8, (64, 32)), (24, (256, 128))):
        a = BR.rebuild(S.bunny_scene, n, env, keep_order=True)
        t = check_restatement(a)
        assert t.sah_split[t.left >= 0].all()  # a well-shaped mesh never needs the fallback
        assert t.depth <= a.depth + 2


@pytest.mark.parametrize("seed", range(8))
def test_restatement_fuzz(seed):
    a = BR.rebuild(R.fuzz_scene, seed, keep_order=True)
    check_restatement(a)


def soup(kind, n=1000):
    """verts [n, 9]: coincident triangles, zero-area triangles at one point, or a mix with a few ordinary ones"""
    one = np.array([0.1, 0.2, 0.3, 0.4, 0.25, 0.3, 0.2, 0.6, 0.35], np.float32)
    if kind == "coincident":
        return np.tile(one, (n, 1))
    if kind == "point":
        return np.tile(np.array([0.1, 0.2, 0.3] * 3, np.float32), (n, 1))
    rng = np.random.default_rng(1)
    v = np.tile(one, (n, 1))
    v[::7] = rng.normal(size=(v[::7].shape[0], 9)).astype(np.float32)
    v[1::5, 3:] = np.tile(v[1::5, :3], (1, 2))  # zero-area members
    v[2::11] = -0.0                           # signed zeros
    return v


@pytest.mark.parametrize("kind", ["coincident", "point", "mixed"])
@pytest.mark.parametrize("leaf_size", [1, 4, 64])
def test_restatement_degenerate_soups(kind, leaf_size):
    v = soup(kind)
    t = BR.build(v, leaf_size)
    BR.check_tree(t.bvh, v[t.order], leaf_size, t.depth)
    if kind != "mixed":
        assert not t.sah_split.any()  # no valid candidate: floor(n/2) all the way down, a balanced tree
        assert t.depth == BR.levels_below(v.shape[0], leaf_size)


def test_restatement_depth_guard():
    """A chain the SAH would build (ever smaller triangles nested at one corner) is cut by the guard: with a guard of 8
    levels the tree still ends within it, and some splits fall back to the median."""
    k = np.arange(200, dtype=np.float64)
    s = (0.5 ** (k / 4)).astype(np.float32)
    v = np.zeros((200, 9), np.float32)
    v[:, 3] = s; v[:, 7] = s
    free = BR.build(v, 1)
    assert free.depth > 8
    t = BR.build(v, 1, max_depth=8)
    BR.check_tree(t.bvh, v[t.order], 1, t.depth)
    assert t.depth <= 8 and not t.sah_split[t.left >= 0].all()


def test_restatement_rejects_non_finite():
    v = soup("mixed", 20)
    v[3, 4] = np.inf
    with pytest.raises(ValueError):
        BR.build(v, 4)


def _builder(obj=None, commit=True):
    lib = L.lib()
    b = C.c_void_p()
    L.check(lib.fspt_builder_create(C.byref(b)))
    if obj is not None:
        pd = L.PropDesc()
        pd.scale = 1.0
        text = obj.encode()
        if commit:
            L.check(lib.fspt_builder_add_obj(b, text, len(text), C.byref(pd)))
        else:
            ng = C.c_uint32()
            L.check(lib.fspt_builder_parse_obj(b, text, len(text), C.byref(pd), None, 0, None, 0, C.byref(ng)))
    return b


TRI_OBJ = "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 3 2\n"


def test_build_gpu_argument_and_state_errors():
    lib = L.lib()
    assert lib.fspt_builder_build_gpu(None, 4, 0) == E_INVALID
    b = _builder(TRI_OBJ)
    try:
        for leaf, dev in ((0, 0), (65, 0), (4, -1)):
            assert lib.fspt_builder_build_gpu(b, leaf, dev) == E_INVALID, (leaf, dev)
        assert b"leaf_size" in lib.fspt_last_error() or b"device" in lib.fspt_last_error()
        ms = C.c_float()
        assert lib.fspt_builder_gpu_stats(b, C.byref(ms), None, None) == E_STATE  # nothing built yet
        if lib.fspt_device_count() == 0:
            assert lib.fspt_builder_build_gpu(b, 4, 0) == E_NO_DEVICE
            assert lib.fspt_builder_counts(b, None, None, None) == E_STATE  # a failed build leaves nothing built
        L.check(lib.fspt_builder_build(b, 4))
        assert lib.fspt_builder_gpu_stats(b, C.byref(ms), None, None) == E_STATE  # the CPU builder's tree
        order = np.zeros(2, np.uint32)
        L.check(lib.fspt_builder_tri_order(b, L.u32ptr(order)))
        assert sorted(order.tolist()) == [0, 1]
    finally:
        lib.fspt_builder_destroy(b)
    empty = _builder()
    try:
        assert lib.fspt_builder_build_gpu(empty, 4, 0) == E_INVALID
        assert b"no triangles" in lib.fspt_last_error()
        assert lib.fspt_builder_tri_order(empty, L.u32ptr(np.zeros(1, np.uint32))) == E_STATE
    finally:
        lib.fspt_builder_destroy(empty)
    pending = _builder(TRI_OBJ, commit=False)
    try:
        assert lib.fspt_builder_build_gpu(pending, 4, 0) == E_STATE
    finally:
        lib.fspt_builder_destroy(pending)
    # a vertex that is finite in float64 but not in float32, and a NaN one
    for obj in ("v 0 0 0\nv 1e39 0 0\nv 0 1 0\nf 1 2 3\n", "v 0 0 0\nv nan 0 0\nv 0 1 0\nf 1 2 3\n"):
        bad = _builder(obj)
        try:
            assert lib.fspt_builder_build_gpu(bad, 4, 0) == E_INVALID
            assert b"non-finite" in lib.fspt_last_error()
        finally:
            lib.fspt_builder_destroy(bad)


def test_python_option():
    with pytest.raises(ValueError):
        S.build_scene(S.bunny_props(), {"synthetic/cube_sphere.obj": S.cube_sphere_obj(2), "synthetic/quad.obj": S.QUAD_OBJ},
                      bvh="bvh.js")
    a = S.build_scene(S.bunny_props(), {"synthetic/cube_sphere.obj": S.cube_sphere_obj(2), "synthetic/quad.obj": S.QUAD_OBJ},
                      keep_order=True)
    assert a.meta["bvh"] == "sah" and sorted(a.meta["tri_order"].tolist()) == list(range(a.n_tris))
    out = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--bvh", "median"], capture_output=True, text=True, cwd=ROOT,
                         timeout=120)
    assert out.returncode == 2 and "--bvh" in out.stderr


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    d = str(tmp_path_factory.mktemp("bvh_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "bvh_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out, log = os.path.join(d, "out.json"), os.path.join(d, "calls.txt")
    env = dict(os.environ, FSPT_MOCK_BVH_LOG=log)
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "bvh_mock_check.js"), d, out], timeout=120, env=env)
    rep = json.load(open(out))
    rep["calls"] = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return rep


def test_js_build_scene_gpu_reaches_the_library(js_report):
    assert js_report["bad_option"] == "RangeError: buildScene: opts.bvh must be 'sah' or 'gpu'"
    # the mock builds no tree: the call goes through, reading the arrays back is refused by the (stubbed) library
    assert js_report["gpu"] == js_report["gpu_default_device"] == "Error: libfspt error -100: mock"
    assert js_report["refused"] == "Error: libfspt error -1: mock"
    assert js_report["not_a_builder"] is not None
    assert js_report["calls"] == ["8 1", "2 0"]
