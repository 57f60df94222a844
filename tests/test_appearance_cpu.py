"""In-place appearance update: what needs no GPU.  The set classification fspt_scene_create and
fspt_scene_update_materials share against the numpy restatement of tests/appearance_cases.py, the argument checks of the
library, the Python binding and the Node host (on the mock library), and render_sequence's frame classification."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import appearance_cases as AC
from fspt_amd import Scene, set_texture_interleave_budget
from fspt_amd import _lib as L
from fspt_amd import scene as S
from fspt_amd import scene_file as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def classify(mat, n_layers, res, is_const, first):
    mat = np.ascontiguousarray(mat, np.float32)
    n = mat.size // 12
    tri_set, n_sets = np.zeros(n, np.uint32), C.c_uint32()
    tab = np.zeros((n, 12), np.uint32)  # (at most one set per triangle)
    is_const, first = np.ascontiguousarray(is_const, np.uint8), np.ascontiguousarray(first, np.uint32)
    L.check(L.lib().fspt_texset_classify_eval(L.fptr(mat), n, n_layers, res, L.u8ptr(is_const), L.u32ptr(first), L.u32ptr(tri_set),
                                              C.byref(n_sets), L.u32ptr(tab), n))
    return tri_set, tab[:n_sets.value]


CORNERS = [-1, 0.49, 0.5, 0.51, 1.49, 1.5, 2.5, 3.49, 3.5, 3.6, 4.6, 100.0, -0.5, -0.51, np.nan, np.inf, -np.inf, 1e30, 2.4999998]


@pytest.mark.parametrize("n_layers", (1, 2, 4, 5))
def test_layer_ids_resolve_like_the_restatement(n_layers):
    """layer_of's corners, one triangle per id in the diffuse slot: the layer shows as the set's first texel"""
    mat = np.zeros((len(CORNERS), 12), np.float32)
    mat[:, 0] = CORNERS
    first = np.arange(100, 100 + n_layers, dtype=np.uint32)
    _, tab = classify(mat, n_layers, 4, np.ones(n_layers, np.uint8), first)
    tri_set, _ = classify(mat, n_layers, 4, np.ones(n_layers, np.uint8), first)
    got = tab[tri_set, 4] - 100
    assert np.array_equal(got, AC.layer_of_ref(CORNERS, n_layers)), (got, AC.layer_of_ref(CORNERS, n_layers))
    assert AC.layer_of_ref([0.5, 0.49, np.nan, -1, np.inf], 3).tolist() == [1, 0, 0, 0, 2]


@pytest.mark.parametrize("budget", (AC.DEFAULT_BUDGET, 0, 128 * 6))
@pytest.mark.parametrize("res", (1, 5, 9))
def test_classification_equals_the_restatement(res, budget):
    rng = np.random.default_rng(res * 7 + (budget % 97))
    layers = 6
    is_const = np.array([1, 0, 0, 1, 0, 0], np.uint8) if res > 1 else np.ones(layers, np.uint8)
    first = rng.integers(0, 2 ** 32, layers, dtype=np.uint64).astype(np.uint32)
    # every key corner: one image layer, two, the same layer twice, all constant, ids off both ends, NaN; then random rows
    rows = [[1, 0, 0, 0], [1, 2, 0, 0], [4, 4, 0, 3], [4, 4, 3, 5], [0, 3, 3, 0], [-1, 7.6, np.nan, np.inf], [1, 0, 0, 0], [2, 1, 0.49, 0.5]]
    rows += rng.uniform(-1, layers + 1, (40, 4)).tolist()
    mat = np.zeros((len(rows), 12), np.float32)
    mat[:, [AC.MAT_DIFFUSE, AC.MAT_EMISSIVE, AC.MAT_NORMAL, AC.MAT_MR]] = np.asarray(rows, np.float32)
    try:
        set_texture_interleave_budget(budget)
        tri_set, tab = classify(mat, layers, res, is_const, first)
    finally:
        set_texture_interleave_budget(AC.DEFAULT_BUDGET)
    want_set, want_tab = AC.classify_ref(mat, layers, res, is_const, first, budget)
    assert np.array_equal(tri_set, want_set)
    assert np.array_equal(tab, want_tab)
    kinds = set(tab[:, 0].tolist())
    if res > 1:
        assert AC.TEXSET_SEPARATE in kinds and AC.TEXSET_CONST in kinds and ((AC.TEXSET_QUAD in kinds) == (budget >= ((res + 3) // 4) * ((res + 1) // 2) * 128))
        if budget == 128 * 6 and res == 5:  # 2 x 3 tiles per interleaved image: the budget holds exactly one
            assert (tab[:, 0] == AC.TEXSET_QUAD).sum() == 1
    else:
        assert kinds == {AC.TEXSET_CONST}


def test_library_argument_checks_need_no_device(small_scene):
    lib = L.lib()
    mat, atlas, bins = L.fptr(small_scene.mat), L.u8ptr(small_scene.atlas), L.u32ptr(small_scene.bins)
    n = C.c_uint64()
    assert lib.fspt_scene_update_materials(None, mat, None, atlas, 1, 1) == -1
    assert lib.fspt_scene_update_environment(None, None, 0, 0, bins, 1) == -1
    assert lib.fspt_multi_update_materials(None, mat, None, atlas, 1, 1) == -1
    assert lib.fspt_multi_update_environment(None, None, 0, 0, bins, 1) == -1
    assert lib.fspt_scene_read_appearance(None, 0, None, 0, C.byref(n)) == -1
    assert lib.fspt_scene_last_appearance_ms(None, None, None, None, None) == -1
    assert lib.fspt_texset_classify_eval(None, 1, 1, 1, None, None, None, None, None, 0) == -1


def test_binding_checks_sizes(small_scene):
    """Scene.update_materials / update_environment refuse arrays of the wrong size before the library sees them"""
    sc = Scene.__new__(Scene)  # (no device: the checks come first)
    sc.arrays, sc._h = small_scene, C.c_void_p()
    with pytest.raises(ValueError, match="x 12"):
        sc.update_materials(small_scene.mat[:-12])
    with pytest.raises(ValueError, match="x 6"):
        sc.update_materials(small_scene.mat, small_scene.uv[:-6])
    with pytest.raises(ValueError, match="atlas_res and atlas_layers"):
        sc.update_materials(small_scene.mat, None, small_scene.atlas)
    with pytest.raises(ValueError, match="RGBA8 texels"):
        sc.update_materials(small_scene.mat, None, small_scene.atlas, small_scene.atlas_res + 1, small_scene.atlas_layers)
    with pytest.raises(ValueError, match="bins are required"):
        sc.update_environment(None, 0, 0, None)
    with pytest.raises(ValueError, match="RGBE texels"):
        sc.update_environment(small_scene.env, small_scene.env_w + 1, small_scene.env_h, small_scene.bins)


# ---- render_sequence's frame classification --------------------------------------------------------------------------
def test_sequence_frame_classification():
    t = S.textured_test_scene(8)
    order = np.random.default_rng(1).permutation(t.n_tris)  # the base's leaf order: parse index per leaf position
    parse = lambda a: dataclasses.replace(a, mat=a.mat.reshape(-1, 12)[np.argsort(order)].reshape(-1), uv=a.uv.reshape(-1, 6)[np.argsort(order)].reshape(-1))
    held = F.held_appearance(t)
    assert F.sequence_frame_changes(held, parse(t), order) == {}
    m = t.mat.copy(); m[7] = 0.25
    ch = F.sequence_frame_changes(held, parse(dataclasses.replace(t, mat=m)), order)
    assert sorted(ch) == ["mat"] and np.array_equal(ch["mat"].reshape(-1), m)
    assert sorted(F.sequence_frame_changes(held, parse(dataclasses.replace(t, uv=t.uv + 1)), order)) == ["uv"]
    a2 = AC.retex(t, 4, 3, 1)
    assert sorted(F.sequence_frame_changes(held, parse(a2), order)) == ["atlas", "mat"]
    same_bytes_other_shape = dataclasses.replace(t, atlas_res=t.atlas_res * 2, atlas_layers=t.atlas_layers)
    assert "atlas" in F.sequence_frame_changes(held, parse(same_bytes_other_shape), order)
    e = AC.with_env(t, 8, 4, 2)
    assert sorted(F.sequence_frame_changes(held, parse(e), order)) == ["bins", "env"]
    assert sorted(F.sequence_frame_changes(held, parse(AC.with_env(t, None, None, 0)), order)) == ["bins", "env"]
    # -0.0 for 0.0 in mat is a change (the arrays are compared as bytes), a NaN that stays is none
    z = t.mat.copy(); z[4] = -0.0
    assert sorted(F.sequence_frame_changes(held, parse(dataclasses.replace(t, mat=z)), order)) == ["mat"]
    nan = t.mat.copy(); nan[5] = np.nan
    assert F.sequence_frame_changes(F.held_appearance(dataclasses.replace(t, mat=nan)), parse(dataclasses.replace(t, mat=nan)), order) == {}
    # another triangle count: a new scene
    fewer = dataclasses.replace(t, tri=t.tri[:-9], mat=t.mat[:-12], uv=t.uv[:-6], norm=t.norm[:-27])
    assert F.sequence_frame_changes(held, fewer, order[:-1]) is None
    # what persists is uploaded once: after held.update(changes) the same frame is a plain refit
    held.update(ch)
    assert F.sequence_frame_changes(held, parse(dataclasses.replace(t, mat=m)), order) == {}


# ---- the Node host on the mock library -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    import shutil
    import subprocess
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("appearance_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "appearance_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "appearance_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_updates_reach_the_library(js_report):
    r = js_report
    assert r["c0"] == 0
    assert r["c1"] == 13                      # mat + uv + atlas
    assert r["c2"] == 15                      # twice mat alone
    assert r["c3"] == 115 + 2 * 10000         # an environment with two bins
    assert r["c4"] == 1215 + 1 * 10000        # no map, one bin
    assert r["cost_after_refused"] == r["c4"]  # nothing refused reached it


def test_js_argument_checks(js_report):
    r = js_report
    assert r["short_mat"] == "RangeError: updateMaterials: mat must be a Float32Array of 2 x 12 floats"
    assert r["f64_mat"] == r["short_mat"]
    assert r["short_uv"] == "RangeError: updateMaterials: uv must be a Float32Array of 2 x 6 floats"
    assert r["short_atlas"] == "RangeError: updateMaterials: atlas must be a Uint8Array of 2 x 2 x 3 x 4 bytes"
    assert r["atlas_no_shape"].startswith("RangeError: updateMaterials: an atlas needs atlasRes")
    assert r["no_object"].startswith("TypeError: updateMaterials: expected")
    assert r["no_bins"].startswith("RangeError: updateEnvironment: bins must be a Uint32Array")
    assert r["odd_bins"] == r["no_bins"]
    assert r["short_env"] == "RangeError: updateEnvironment: env must be a Uint8Array of 3 x 2 x 4 bytes"
    assert r["env_zero"].startswith("RangeError: updateEnvironment: an env needs envW >= 1")
    assert r["addon_len"].startswith("RangeError: fspt_napi: updateMaterials needs 12 floats")
    assert r["addon_atlas"].startswith("RangeError: fspt_napi: updateMaterials needs atlasRes")
    assert r["addon_type"].startswith("TypeError: fspt_napi: expected a TypedArray")
    assert r["addon_no_bins"].startswith("TypeError: fspt_napi: expected a TypedArray")
    assert r["addon_env_len"].startswith("RangeError: fspt_napi: updateEnvironment needs envW")
    assert all(m and "handle" in m for m in r["target_as_scene"]), r["target_as_scene"]


def test_js_render_in_flight_guard(js_report):
    r = js_report
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["after"] == [None, None]
    assert all(m and "destroyed" in m for m in r["closed"]), r["closed"]
