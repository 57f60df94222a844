"""The GPU texture packer as far as no device is needed: the two committed decode tables, the numpy restatement
of the arithmetic contract (tests/texpack_ref.py) against scene.resample_image, TexturePacker.pack_desc(), and every refusal
of the texture entries - on the library, on the binding and on the Node host against a mock."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import texpack_ref as R
from fspt_amd import Scene, MultiPathTracer
from fspt_amd import _lib as L
from fspt_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tables ----------------------------------------------------------------------------------------------------------
def srgb64(c):
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def test_tables():
    lin, srgb = S.texture_decode_tables()
    assert lin.dtype == np.float32 and srgb.dtype == np.float32
    want_lin = np.arange(256).astype(np.float32) / np.float32(255)
    assert np.array_equal(lin.view(np.uint32), want_lin.view(np.uint32))
    exact = np.array([srgb64(i / 255) for i in range(256)], np.float64)
    ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)  # (of the float32 next to the exact value)
    err = np.abs(srgb.astype(np.float64) - exact) / np.where(ulp > 0, ulp, 1.0)
    print("srgb table: max error %.3f ulp" % err.max())
    assert (err <= 1.0).all(), (int(err.argmax()), float(err.max()))
    assert (np.diff(srgb) >= 0).all()
    assert srgb[0] == 0.0 and srgb[255] == 1.0


def test_tables_are_the_generator_output():
    """the committed header is what tools/make_texture_tables.py writes, and the library hands out its bits"""
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "make_texture_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    text = open(os.path.join(ROOT, "fspt_amd", "csrc", "fspt_texpack_tables.hpp")).read()
    import re
    words = np.array([int(x, 16) for x in re.findall(r"0x([0-9A-F]{8})u", text)], np.uint32)
    lin, srgb = S.texture_decode_tables()
    assert words.size == 512 and np.array_equal(words[:256], lin.view(np.uint32)) and np.array_equal(words[256:], srgb.view(np.uint32))
    assert L.lib().fspt_texture_decode_tables(None, L.fptr(srgb)) == -1


# ---- the restatement against scene.resample_image --------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CPU_SHAPES + [((300, 200), 33), ((1, 7), 9), ((7, 1), 2), ((2, 2), 1)], ids=lambda s: f"{s[0][0]}x{s[0][1]}_to_{s[1]}")
def test_restatement_uncorrected_is_resample_image(shape):
    (w, h), res = shape
    im = R.source(w, h)
    for sw in R.SWIZZLES:
        assert np.array_equal(R.resample(im, res, False, sw), S.resample_image(im, res, False, sw)), sw


@pytest.mark.parametrize("shape", R.CPU_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_to_{s[1]}")
def test_restatement_corrected_stays_within_one_code(shape):
    """scene.resample_image decodes sRGB with numpy's float32 pow, the restatement with the committed table (183 of 256
    entries differ): no byte may differ by more than 1 code, at most 0.1 % of the bytes at all"""
    (w, h), res = shape
    im = R.source(w, h)
    for sw in R.SWIZZLES:
        a, b = R.resample(im, res, True, sw).astype(np.int32), S.resample_image(im, res, True, sw).astype(np.int32)
        d = np.abs(a - b)
        print(f"{w}x{h} -> {res} {sw}: max {d.max()} code, {int((d > 0).sum())} of {d.size} bytes differ")
        assert d.max() <= 1
        assert (d > 0).sum() <= 0.001 * d.size


def test_restatement_decodes_rgb_only_and_clamps_rows():
    """the properties a wrong kernel would break, on the restatement itself: alpha is never sRGB-decoded, columns wrap,
    rows clamp"""
    im = np.zeros((2, 2, 4), np.uint8)
    im[..., :3] = 255
    im[..., 3] = 128
    out = R.resample(im, 2, True)
    assert (out[..., :3] == math.floor(np.float32(128 / 255) * 255 + 0.5)).all()  # srgb[255] = 1, alpha linear
    im = np.zeros((2, 2, 4), np.uint8); im[..., 3] = 255
    im[0, :, 0] = 255            # top row red
    im[:, 0, 1] = 255            # left column green
    out = R.resample(im, 8)      # magnified x 4: u < 0 at x = 0 wraps to the last column, v clamps at both edges
    assert out[0, :, 0].max() == 0 and out[-1, :, 0].min() == 255          # (output row 0 = bottom = source row 1)
    assert out[0, 0, 1] == 159 and out[0, 7, 1] == 96                      # columns 0 and 7 blend across the seam (clamped: 255 and 0)


# ---- pack_desc -------------------------------------------------------------------------------------------------------
def test_pack_desc_follows_get_pixels_rules():
    p = S.TexturePacker(2048)
    a, b = R.source(16, 8), R.source(5, 12, seed=1)
    assert p.add_texture("a.png", a, corrected=True) == 0
    assert p.add_color([0.5, 0.25, 1.5]) == 1
    assert p.add_texture("a.png", a, corrected=False, swizzle=(0, 2, 1, 3)) == 2  # layer 0 is never de-duplicated: a second layer
    assert p.add_texture("b.png", b, corrected=False) == 3
    assert p.add_texture("b.png", b, swizzle=(1, 1, 1, 1)) == 3                   # ... every other layer is; the LAST swizzle decides
    assert p.add_texture("a.png", a, corrected=True) == 2
    d = p.pack_desc()
    assert d["res"] == 12 == p.get_resolution()                                   # the tallest source, below atlas_res
    assert len(d["images"]) == 2 and d["images"][0] is p.images["a.png"]["rgba"]
    want = p.describe()
    assert len(d["layers"]) == len(want) == 4
    for y, w in zip(d["layers"], want):
        if "color" in w:
            assert y == {"kind": "color", "color": w["color"]}
        else:
            assert y["kind"] == "image" and y["corrected"] == w["corrected"] and list(y["swizzle"]) == (w["swizzle"] or [0, 1, 2, 3])
    assert d["layers"][0]["image"] == d["layers"][2]["image"] == 0 and d["layers"][3]["image"] == 1
    assert d["layers"][0]["corrected"] is False and d["layers"][0]["swizzle"] == (0, 2, 1, 3)   # the image's flags when the atlas is written
    assert d["layers"][3]["swizzle"] == (1, 1, 1, 1)
    # the description is the atlas: restated layer by layer it is get_pixels() (no layer here is corrected)
    assert np.array_equal(R.pack(d), p.get_pixels())
    # a pre-resampled layer goes as it is and raises max_res like get_pixels
    q = S.TexturePacker(4)
    q.add_color([1, 0, 0]); q.add_pixels("px", np.full((4, 4, 4), 7, np.uint8))
    dq = q.pack_desc()
    assert dq["res"] == 4 and dq["layers"][1] == {"kind": "pixels", "image": 0} and np.array_equal(R.pack(dq), q.get_pixels())
    q.add_pixels("small", np.zeros((2, 2, 4), np.uint8))
    with pytest.raises(ValueError, match="res x res"):
        q.pack_desc()
    # colours only: a 1 x 1 atlas
    c = S.TexturePacker(2048); c.add_color([0.2, 0.4, 0.6])
    assert c.pack_desc() == {"res": 1, "images": [], "layers": [{"kind": "color", "color": [0.2, 0.4, 0.6]}]}


def test_colours_cross_the_abi_as_their_bytes():
    """a flat colour is quantised in float64 on the host; the float32 the ABI carries must give the same byte in the library"""
    cols = [k * 0.5 / 255 for k in range(0, 512, 7)] + [-0.5, 1.5, 0.7, 0.1, 0.3, 1 / 3]
    desc = {"res": 1, "images": [], "layers": [{"kind": "color", "color": [c, c, c]} for c in cols]}
    p, _, _, keep = S.texture_pack_struct(desc)
    for l, c in enumerate(cols):
        want = R.color_texel([c] * 3)[0]
        got = math.floor(min(max(float(p.layers[l].color[0]), 0.0), 1.0) * 255.0 + 0.5)
        assert got == want, (c, got, want)


# ---- refusals --------------------------------------------------------------------------------------------------------
good_desc, INVALID = R.good_desc, R.INVALID


@pytest.mark.parametrize("name", sorted(INVALID))
def test_library_refuses_before_it_needs_a_device(name):
    lib = L.lib()
    out = np.zeros(4 * 4 * 3 * 4, np.uint8)
    p, _, _, keep = S.texture_pack_struct(good_desc())
    assert lib.fspt_texture_pack_check_eval(C.byref(p), None, 0, 0, 0) == 0
    INVALID[name](p)
    for call in (lambda: lib.fspt_atlas_pack_gpu(0, C.byref(p), L.u8ptr(out)),
                 lambda: lib.fspt_texture_pack_check_eval(C.byref(p), None, 0, 0, 0),
                 lambda: lib.fspt_texture_pack_check_eval(C.byref(p), L.u32ptr(np.arange(p.n_layers, dtype=np.uint32)), p.n_layers, 8, 4)):
        assert call() == -1, name
        assert lib.fspt_last_error()


def test_library_refuses_null_and_patch_arguments():
    lib = L.lib()
    p, _, _, keep = S.texture_pack_struct(good_desc())
    out = np.zeros(4 * 4 * 3 * 4, np.uint8)
    mat = np.zeros(12, np.float32)
    ids = np.array([0, 5, 2], np.uint32)
    assert lib.fspt_atlas_pack_gpu(0, None, L.u8ptr(out)) == -1
    assert lib.fspt_atlas_pack_gpu(0, C.byref(p), None) == -1
    for fn in (lib.fspt_scene_update_textures, lib.fspt_scene_update_textures_device, lib.fspt_multi_update_textures):
        assert fn(None, L.fptr(mat), None, C.byref(p)) == -1
    for fn in (lib.fspt_scene_patch_textures, lib.fspt_scene_patch_textures_device, lib.fspt_multi_patch_textures):
        assert fn(None, L.u32ptr(ids), 3, C.byref(p)) == -1
    assert lib.fspt_last_error() == b"fspt_multi_patch_textures: NULL handle"
    chk = lib.fspt_texture_pack_check_eval
    assert chk(C.byref(p), L.u32ptr(ids), 3, 6, 4) == 0
    assert chk(None, L.u32ptr(ids), 3, 6, 4) == -1
    assert chk(C.byref(p), None, 3, 6, 4) == -1                                          # NULL layer_ids
    assert chk(C.byref(p), L.u32ptr(ids), 2, 6, 4) == -1                                 # as many ids as layers
    assert chk(C.byref(p), L.u32ptr(ids), 3, 5, 4) == -1 and b"5 layers" in lib.fspt_last_error()    # an id at raw_layers
    assert chk(C.byref(p), L.u32ptr(np.array([2, 0, 2], np.uint32)), 3, 6, 4) == -1 and b"twice" in lib.fspt_last_error()
    assert chk(C.byref(p), L.u32ptr(ids), 3, 6, 8) == -1 and b"retained atlas has 8" in lib.fspt_last_error()  # res is the retained one
    assert chk(C.byref(p), L.u32ptr(ids), 3, 0, 0) == -6                                 # FSPT_E_STATE: nothing retained


def test_without_a_device_the_packer_fails_loudly():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(L.FsptError) as e:
        S.atlas_pack_gpu(good_desc(), 0)
    assert e.value.code == -2


def test_binding_checks_sizes(small_scene):
    sc = Scene.__new__(Scene)  # (no device: the checks come first)
    sc.arrays, sc._h, sc.device = small_scene, C.c_void_p(), 0
    d = good_desc()
    with pytest.raises(ValueError, match="x 12"):
        sc.update_textures(small_scene.mat[:-12], None, d)
    with pytest.raises(ValueError, match="x 6"):
        sc.update_textures(small_scene.mat, small_scene.uv[:-6], d)
    with pytest.raises(ValueError, match=r"not \[h, w, 4\]"):
        sc.update_textures(small_scene.mat, None, dict(d, images=[np.zeros((3, 5, 3), np.uint8), d["images"][1]]))
    with pytest.raises(ValueError, match="swizzle"):
        sc.update_textures(small_scene.mat, None, dict(d, layers=[R.image_layer(0, False, (0, 1, 2))]))
    with pytest.raises(KeyError):
        sc.update_textures(small_scene.mat, None, dict(d, layers=[{"kind": "image"}]))
    with pytest.raises(ValueError, match="2 layer ids for 1 layers"):
        sc.patch_textures([0, 1], [d["layers"][0]], [])
    with pytest.raises(TypeError, match="integers"):
        sc.patch_textures([0.5], [d["layers"][0]], [])
    with pytest.raises(ValueError, match="textures must be one of"):
        S.build_scene([], {}, textures="opencl")
    # what passes the binding reaches the library, which refuses the NULL handle
    with pytest.raises(L.FsptError) as e:
        sc.update_textures(small_scene.mat, None, d)
    assert e.value.code == -1
    with pytest.raises(L.FsptError):
        sc.patch_textures([1], [d["layers"][0]], [])
    m = MultiPathTracer.__new__(MultiPathTracer)
    m.arrays, m._m = small_scene, C.c_void_p()
    with pytest.raises(L.FsptError, match="fspt_multi_update_textures: NULL handle"):
        m.update_textures(small_scene.mat, None, d)
    with pytest.raises(L.FsptError, match="fspt_multi_patch_textures: NULL handle"):
        m.patch_textures([1], [d["layers"][0]], [])


# ---- the Node host on the mock library -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    import json
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / node headers not available")
    d = str(tmp_path_factory.mktemp("texpack_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "texpack_mock_stub.c"), "-lm"])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "texpack_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_pack_desc_follows_pixels_rules(js_report):
    r = js_report
    assert r["ids"] == [0, 1, 2, 3, 3]                       # layer 0 is added again, every other layer is found
    pd = r["pack_desc"]
    assert pd["res"] == 12 and pd["n_images"] == 2 and pd["same"] is True
    assert pd["layers"] == [{"kind": "image", "image": 0, "corrected": False, "swizzle": [0, 2, 1, 3]}, {"kind": "color", "color": [0.5, 0.25, 1.5]},
                            {"kind": "image", "image": 0, "corrected": False, "swizzle": [0, 2, 1, 3]}, {"kind": "image", "image": 1, "corrected": False, "swizzle": [0, 1, 2, 3]}]
    for y, w in zip(pd["layers"], r["describe"]):            # the describe() layer list
        assert ("color" in w and y["color"] == w["color"]) or (y["corrected"] == w["corrected"] and y["swizzle"] == (w["swizzle"] or [0, 1, 2, 3]))


def test_js_calls_reach_the_library(js_report):
    r = js_report
    assert r["atlas"] == [4 * 4 * 3 * 4, [0, 26, 0, 129], [1, 0, 16 + 2, 129], [2, 1, 0, 129]]   # kinds, colour byte, flags and the device went through
    assert r["pixels_device"] == [1, 0, 2, 130]                                                 # AtlasLayers.pixels({device: 2})
    assert r["c0"] == 0
    assert r["patch_no_atlas"] == "Error: libfspt error -6: mock"
    assert r["c1"] == pytest.approx(3 + 4 * 10000 + 124e-6, abs=1e-9)          # mat + uv, res 4, 3 x 5 + 4 x 4 texels
    assert r["c2"] == pytest.approx(4 + 12 * 10000 + 752e-6, abs=1e-9)         # an AtlasLayers: res 12, its two images once each
    assert r["patch_other_res"] == "Error: libfspt error -1: mock"
    assert r["c3"] == pytest.approx(204 + 12 * 10000 + 16e-6, abs=1e-9)        # two layers patched from one 2 x 2 image
    assert r["cost_after_refused"] == r["c3"]                                    # nothing refused reached it
    assert r["clamped_image"] is None                                            # a Uint8ClampedArray's bytes go as they are


def test_js_argument_checks(js_report):
    r = js_report
    assert r["no_object"] == ["TypeError: updateTextures: expected {mat, uv, textures}", "TypeError: patchTextures: expected {layerIds, layers, images, res}",
                              "TypeError: atlasPackGpu: expected a texture description {res, images, layers}"]
    assert "x 12 floats" in r["short_mat"] and "x 6 floats" in r["short_uv"] and r["no_textures"].startswith("TypeError: updateTextures: expected a texture description")
    for k in ("short_image", "u16_image"):
        assert r[k] == "RangeError: atlasPackGpu: images[0] must be {width, height, data: width x height x 4 bytes}", k
    assert r["res_float"] == "RangeError: atlasPackGpu: res must be an integer"
    assert "swizzle must hold 4" in r["short_swizzle"] and "color must hold 3" in r["short_colour"] and "index into images" in r["image_float"]
    assert r["ids_count"] == "RangeError: patchTextures: 2 layer ids for 1 layers" and r["ids_type"].startswith("TypeError: patchTextures: layerIds")
    assert sorted(r["refused_by_library"]) == sorted(["res_0", "res_16385", "no_layers", "w_0", "h_16385", "image_index", "swizzle_4", "swizzle_nan", "kind_3",
                                                      "kind_word", "colour_nan", "colour_inf", "pixels_not_res"])
    for k, v in r["refused_by_library"].items():
        assert v == ["Error: libfspt error -1: mock"] * 2, k
    assert r["patch_refused"] == ["Error: libfspt error -1: mock"] * 2
    # the addon checks the sizes again
    assert "2 words (w, h) per image" in r["addon_dims"] and "w * h RGBA8 texels per image" in r["addon_image_len"] and "10 floats per layer" in r["addon_layers_len"]
    assert r["addon_images_type"].startswith("TypeError") and r["addon_image_type"].startswith("TypeError")
    assert "12 floats (mat)" in r["addon_mat"] and "one layer id per layer" in r["addon_ids"]
    assert r["target_as_scene"] == ["TypeError: fspt_napi: expected a scene handle"] * 2


def test_js_render_in_flight_guard(js_report):
    r = js_report
    assert r["during"] == ["Error: render in flight"] * 2
    assert r["after"] == [None, None]
    assert r["closed"] == ["Error: fspt_napi: the scene handle was destroyed"] * 2
