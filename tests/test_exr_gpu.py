"""The GPU OpenEXR encoder (include/fspt.h fspt_exr_*, fspt_draw_exr) on the MI355X against the integer
restatement tests/exr_ref.py, byte for byte: one pixel and one column, ZIP with one block and with a last block of one line,
blocks longer than a deflate chunk and segments off 4-byte alignment, the three compressions, HALF and FLOAT, every layer
combination, compressed and raw blocks in one file under both forms of the fallback, the conversion's edge values as pixels,
both row orders; the device form; draw_exr against the buffers it stands for, its state and cap checks, and a draw between
two presents."""
import ctypes as C

import numpy as np
import pytest

import fspt_amd
from fspt_amd import PathTracer, _lib as L

import exr_ref as X
from exr_cases import ALL_LAYERS, buffers, case_id, cases, radiance, reference

pytestmark = pytest.mark.gpu

CASES = cases()
COMP = {X.NONE: "none", X.ZIPS: "zips", X.ZIP: "zip"}


def gpu_file(case, rgba, feat, **kw):
    _, _, _, comp, pt, layers, cb, up, _ = case
    return fspt_amd.exr_encode(rgba, feat, COMP[comp], pt == X.FLOAT, layers, cb, up, **kw)


def explain(got, want):
    """where two files part, for the assertion's message"""
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at {at}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_file_is_the_restatements(case):
    want, st = reference(case)
    rgba, feat = buffers(case)
    got = gpu_file(case, rgba, feat)
    assert got == want, explain(got, want)
    if case[0] == "split":  # the raw fallback's other form: a kept copy instead of a second conversion
        assert True in st["raw"] and False in st["raw"]
        fspt_amd.exr_set_form(1)
        try:
            got = gpu_file(case, rgba, feat)
        finally:
            fspt_amd.exr_set_form(0)
        assert got == want, explain(got, want)


def test_more_blocks_than_the_offset_scan_is_wide():
    """what the restatement says of the cases that put k_exr_offsets' scan past its first tile (each of them is one of
    test_the_file_is_the_restatements' cases): the block counts, two chunks a block, and compressed and raw blocks in one
    file on both sides of block 256"""
    wide = {c[1:4]: reference(c)[1] for c in CASES if c[6] == 256 and c[2] >= 256}
    assert {k: len(st["raw"]) for k, st in wide.items()} == {(3, 256, X.ZIPS): 256, (3, 257, X.ZIPS): 257, (2, 513, X.ZIPS): 513, (50, 257, X.ZIPS): 257,
                                                            (1, 4112, X.ZIP): 257, (2, 300, X.NONE): 300, (40, 300, X.ZIPS): 300}
    assert len(wide[(50, 257, X.ZIPS)]["kinds"]) == 514
    mixed = wide[(40, 300, X.ZIPS)]["raw"]
    assert {True, False} == set(mixed[:256]) == set(mixed[256:])


def test_row_order_device_form_and_determinism():
    import torch
    case = next(c for c in CASES if c[1:3] == (301, 18) and c[5] == (X.ALPHA | X.DEPTH))
    want, _ = reference(case)
    rgba, feat = buffers(case)
    up = case[7]
    # the other row order of the flipped buffers is the same file
    flipped = (case[:7] + (not up,) + case[8:])
    assert gpu_file(flipped, np.ascontiguousarray(rgba[::-1]), np.ascontiguousarray(feat[::-1])) == want
    for _ in range(3):  # the deflate's bits are OR-ed into shared words in no fixed order
        assert gpu_file(case, rgba, feat) == want
    tr, tf = torch.from_numpy(rgba).to("cuda:0"), torch.from_numpy(feat).to("cuda:0")
    assert gpu_file(case, tr, tf) == want
    plain = next(c for c in CASES if c[1:3] == (301, 18) and c[3] == X.ZIPS)
    assert gpu_file(plain, torch.from_numpy(buffers(plain)[0]).to("cuda:0"), None) == reference(plain)[0]
    # features that no layer asks for change nothing, and need not be there
    rgb = next(c for c in CASES if c[1:3] == (3, 33) and c[4] == X.FLOAT)
    assert gpu_file(rgb, buffers(rgb)[0], np.full((33, 3, 8), 7.0, np.float32)) == reference(rgb)[0]


def test_strided_tensors_on_a_side_stream():
    """rgba and features as views of wider tensors, written on a stream of their own: exr_encode copies both to contiguous
    tensors on that stream and waits for it behind the second copy, before the library reads them on its own stream"""
    import torch
    case = next(c for c in CASES if c[1:3] == (301, 18) and c[5] == (X.ALPHA | X.DEPTH))
    want, _ = reference(case)
    rgba, feat = buffers(case)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wide_r = torch.zeros((18, 301, 6), dtype=torch.float32, device="cuda:0")
        wide_f = torch.zeros((18, 301, 11), dtype=torch.float32, device="cuda:0")
        wide_r[..., 1:5] = torch.from_numpy(rgba).to("cuda:0")
        wide_f[..., 2:10] = torch.from_numpy(feat).to("cuda:0")
        tr, tf = wide_r[..., 1:5], wide_f[..., 2:10]
        assert not tr.is_contiguous() and not tf.is_contiguous()
        got = gpu_file(case, tr, tf)
    assert got == want, explain(got, want)


def test_cap_and_errors():
    lib = L.lib()
    case = next(c for c in CASES if c[1:3] == (3, 16) and c[4] == X.HALF)
    want, _ = reference(case)
    rgba, feat = buffers(case)
    p = L.ExrParams(case[3], case[4], case[5], case[6])
    buf = np.full(len(want) + 8, 7, np.uint8)
    n = C.c_size_t(123)
    args = (0, L.fptr(rgba), L.fptr(feat), 3, 16, 1 if case[7] else 0, C.byref(p), L.u8ptr(buf))
    assert lib.fspt_exr_encode(*args, len(want) - 1, C.byref(n)) == -1
    assert n.value == len(want) and (buf == 7).all() and b"fspt_exr_encode" in lib.fspt_last_error()
    assert lib.fspt_exr_encode(*args, len(want), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want and (buf[n.value:] == 7).all()
    ms, bus = fspt_amd.exr_last_ms()
    assert all(x > 0 for x in ms) and bus == len(want) + 8
    # NULL parameters: ZIP, HALF, RGB, the default chunk
    a = radiance("rendered", 20, 20)
    big = np.zeros(X.bound(20, 20), np.uint8)
    assert lib.fspt_exr_encode(0, L.fptr(a), None, 20, 20, 0, None, L.u8ptr(big), big.size, C.byref(n)) == 0
    assert big[:n.value].tobytes() == X.encode(a)


# ---- the target's entry ---------------------------------------------------------------------------------------------
W, H = 64, 48


def make_pt(arrays, cam, seed=7):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.seed(seed)
    return pt


def test_draw_exr_is_the_buffer_encoded(small_scene, camera):
    pt = make_pt(small_scene, camera)
    pt.set_auto_exposure(True)  # (neither takes part: the file is scene-linear)
    pt.set_bloom(True)
    pt.render(3)
    for source in ("denoised", "temporal", "temporal_denoised"):
        with pytest.raises(fspt_amd.FsptError) as e:
            pt.draw_exr(source)
        assert e.value.code == -6, source
    for layers in ("albedo", "normal", "depth", "alpha,depth"):  # feature layers and no features() yet
        with pytest.raises(fspt_amd.FsptError, match="fspt_draw_exr") as e:
            pt.draw_exr(layers=layers)
        assert e.value.code == -6, layers
    rad = pt.readRadiance()
    assert pt.draw_exr() == fspt_amd.exr_encode(rad, bottom_up=True) == X.encode(rad, None, True)
    assert pt.draw_exr(layers="alpha", float32=True, compression="none") == X.encode(rad, None, True, X.NONE, X.FLOAT, X.ALPHA)
    pt.features(samples=2)
    feat = pt.readFeatures()
    got = pt.draw_exr(layers="albedo,normal,depth,alpha", chunk_bytes=4096)
    assert got == fspt_amd.exr_encode(rad, feat, layers=ALL_LAYERS, chunk_bytes=4096, bottom_up=True)
    assert got == X.encode(rad, feat, True, X.ZIP, X.HALF, ALL_LAYERS, 4096)
    planes = X.read(got)["planes"]
    assert np.array_equal(planes["Z"], feat[::-1, :, 3]) and (planes["Z"] == 1e5).any()  # misses, which no half holds
    assert np.array_equal(planes["R"], rad[::-1, :, 0].astype(np.float16)) and (planes["A"] == 1).all()
    den = pt.denoise(iterations=2)
    assert pt.draw_exr("denoised", "zips", layers="depth") == X.encode(den, feat, True, X.ZIPS, X.HALF, X.DEPTH)
    tmp = pt.temporal_accumulate()
    assert pt.draw_exr("temporal", float32=True, layers="alpha") == X.encode(tmp, None, True, X.ZIP, X.FLOAT, X.ALPHA)
    tden = pt.temporal_denoise(iterations=1)
    assert pt.draw_exr("temporal_denoised", layers="normal") == X.encode(tden, feat, True, X.ZIP, X.HALF, X.NORMAL)
    with pytest.raises(ValueError):
        pt.draw_exr("radiance")
    # a buffer one byte short: -1, the size needed, nothing written
    lib, p = L.lib(), L.ExrParams(3, 1, ALL_LAYERS, 4096)
    need = len(got)
    buf, n = np.full(need + 16, 9, np.uint8), C.c_size_t()
    assert lib.fspt_draw_exr(pt._t, 0, C.byref(p), L.u8ptr(buf), need - 1, C.byref(n)) == -1
    assert n.value == need and (buf == 9).all() and b"fspt_draw_exr" in lib.fspt_last_error()
    assert lib.fspt_draw_exr(pt._t, 0, C.byref(p), L.u8ptr(buf), need, C.byref(n)) == 0
    assert buf[:n.value].tobytes() == got and (buf[need:] == 9).all()
    pt.close()


def test_draw_exr_between_two_presents(small_scene, camera):
    """as draw_png: the draw joins the pipeline - the frame in flight is dropped, the next present starts over - and the
    file is that of the accumulator as it stands, the ticks recorded so far included"""
    pt = make_pt(small_scene, camera)
    pt.tick(); pt.tick()
    assert pt.present()[1] == 0
    pt.tick()
    frame, ticks = pt.present()
    assert ticks == 2 and frame is not None
    pt.tick()
    got = pt.draw_exr(layers="alpha")
    assert got == X.encode(pt.readRadiance(), None, True, X.ZIP, X.HALF, X.ALPHA)
    ref = make_pt(small_scene, camera)
    ref.render(4)
    assert got == ref.draw_exr(layers="alpha")
    assert pt.present()[1] == 0  # (first call after a join: nothing to present yet)
    png_side = make_pt(small_scene, camera)
    png_side.tick(); png_side.tick()
    png_side.present(); png_side.tick(); png_side.present(); png_side.tick()
    png_side.draw_png()
    assert png_side.present()[1] == 0
    for t in (pt, ref, png_side):
        t.close()


def test_hosts_write_exr(tmp_path):
    """render.py --out x.exr writes the file draw_exr returns; --hdr x.exr next to a PNG; write_image the file exr_encode returns"""
    from fspt_amd import render as R, scene as S
    from fspt_amd.scene_file import write_image
    out, hdr, npy = tmp_path / "x.exr", tmp_path / "h.exr", tmp_path / "h.npy"
    common = ["--width", "40", "--height", "24", "--spp", "3", "--mesh-n", "8", "--bounces", "4"]
    R.main(["--out", str(out), "--exr-layers", "albedo,depth", "--exr-compression", "zips"] + common)
    R.main(["--out", str(tmp_path / "x.png"), "--hdr", str(hdr), "--exr-float"] + common)
    R.main(["--out", str(tmp_path / "y.png"), "--hdr", str(npy)] + common)
    pt = PathTracer(S.bunny_scene(n=8), 40, 24, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.render(3)
    rad = pt.readRadiance()
    pt.features(8, 1)
    assert out.read_bytes() == pt.draw_exr(layers="albedo,depth", compression="zips") == X.encode(rad, pt.readFeatures(), True, X.ZIPS, X.HALF, X.ALBEDO | X.DEPTH)
    assert hdr.read_bytes() == X.encode(rad, None, True, X.ZIP, X.FLOAT)
    assert np.array_equal(np.load(str(npy)), rad)  # any other --hdr name stays .npy
    pt.close()
    top_down = np.ascontiguousarray(rad[::-1])
    write_image(str(tmp_path / "a.exr"), top_down)
    assert (tmp_path / "a.exr").read_bytes() == X.encode(top_down)
    write_image(str(tmp_path / "b.exr"), top_down, exr={"compression": "none", "layers": "alpha", "float32": True})
    assert (tmp_path / "b.exr").read_bytes() == X.encode(top_down, None, False, X.NONE, X.FLOAT, X.ALPHA)
