"""The GPU JPEG encoder (include/fspt.h fspt_jpeg_*, fspt_draw_jpeg, fspt_present_jpeg) on the MI355X against the
integer restatement tests/jpeg_ref.py: stage one's coefficients and the whole file, byte for byte, at sizes on and off the
MCU grid, one workgroup and many, every setting, both row orders; the device form; determinism; draw_jpeg against the
drawing entries it stands for; present_jpeg frame by frame, its cap check and its mixing with present."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import fspt_amd
from fspt_amd import PathTracer, _lib as L

import jpeg_ref as J
from jpeg_cases import CONTENTS, image

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (8, 8), (16, 16), (17, 9), (33, 16), (19, 37)]
LARGE = (256, 144)  # many workgroups and intervals; 9 MCU rows of 4:2:0 and 18 of 4:4:4: more than 8 markers, RSTn wraps
SUBS = (("444", J.S444), ("420", J.S420))
QUALITIES = (1, 10, 75, 100)
RESTARTS = (0, 1, 3, 65535)


def check_case(w, h, sub, quality, restart, content, bottom_up):
    a = image(content, w, h)
    want_c = J.coefficients(a, bottom_up, quality, sub[1])
    got_c = fspt_amd.jpeg_coefficients_eval(a, quality, sub[0], bottom_up)
    assert got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (w, h, sub[0], quality, content, bottom_up)
    want = J.encode(a, bottom_up, quality, sub[1], restart)
    got = fspt_amd.jpeg_encode(a, quality, sub[0], restart, bottom_up)
    assert got == want, (w, h, sub[0], quality, restart, content, bottom_up, len(got), len(want))
    b = a.copy()
    b[..., 3] = 255 - b[..., 3]  # another alpha: the same file
    assert fspt_amd.jpeg_encode(b, quality, sub[0], restart, bottom_up) == want
    return want


@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_sizes_every_setting(size):
    """both subsamplings x four qualities x four intervals, the five contents and the two row orders dealt round-robin so
    that every size meets each of them under every subsampling"""
    seen = set()
    for k, (sub, quality, restart) in enumerate(itertools.product(SUBS, QUALITIES, RESTARTS)):
        content, bottom_up = CONTENTS[k % 5], bool((k // 5 + k) & 1)
        check_case(size[0], size[1], sub, quality, restart, content, bottom_up)
        seen.add((sub[0], content)); seen.add((sub[0], bottom_up))
    assert len(seen) == 2 * 5 + 2 * 2


@pytest.mark.parametrize("content", CONTENTS)
def test_many_workgroups_and_intervals(content):
    w, h = LARGE
    wraps = False
    for k, (sub, restart) in enumerate(itertools.product(SUBS, RESTARTS)):
        quality = QUALITIES[(k + CONTENTS.index(content)) % 4]
        want = check_case(w, h, sub, quality, restart, content, bool(k & 1))
        _, mw, mh = J.mcu_grid(w, h, sub[1])
        ri = J.restart_interval(w, h, sub[1], restart)
        markers = (mw * mh + ri - 1) // ri - 1
        wraps = wraps or markers > 8
        assert want.count(b"\xFF\xD0") == (markers + 7) // 8  # (0xFF in the data is stuffed: only markers match) RST0 comes again after RST7
    assert wraps


@pytest.mark.parametrize("size,intervals", (((128, 128), 256), ((8, 2056), 257), ((8, 4104), 513)), ids=lambda v: str(v).replace(" ", ""))
def test_interval_counts_around_the_offset_scans_width(size, intervals):
    """every MCU an interval: as many intervals as k_jpeg_offsets scans in one tile of 256, one more, and two tiles and one -
    the carry from tile to tile, and RSTn wrapping many times"""
    w, h = size
    _, mw, mh = J.mcu_grid(w, h, J.S444)
    assert J.restart_interval(w, h, J.S444, 1) == 1 and mw * mh == intervals
    want = check_case(w, h, ("444", J.S444), 75, 1, "noise", bool(intervals & 1))
    assert want.count(b"\xFF\xD0") == (intervals - 1 + 7) // 8


def test_every_quality_on_one_image():
    a = image("noise", 24, 16)
    for q in (1, 2, 25, 49, 50, 51, 90, 99, 100):
        assert fspt_amd.jpeg_encode(a, q, "444") == J.encode(a, False, q, J.S444)


def test_device_form_and_determinism():
    import torch
    w, h = LARGE
    a = image("noise", w, h)
    first = fspt_amd.jpeg_encode(a, 100, "420", 0, True)
    assert first == J.encode(a, True, 100, J.S420, 0)
    for _ in range(3):  # the bits of neighbouring blocks are OR-ed into shared words in no fixed order
        assert fspt_amd.jpeg_encode(a, 100, "420", 0, True) == first
    t = torch.from_numpy(a).to("cuda:0")
    assert fspt_amd.jpeg_encode(t, 100, "420", 0, True) == first
    assert fspt_amd.jpeg_encode(t, 75, "444", 3, False) == J.encode(a, False, 75, J.S444, 3)


def test_cap_and_errors():
    lib = L.lib()
    a = image("noise", 33, 16)
    want = J.encode(a)
    p = L.JpegParams(85, 1, 0)
    buf = np.full(len(want) + 8, 7, np.uint8)
    n = C.c_size_t(123)
    assert lib.fspt_jpeg_encode(0, L.u8ptr(a), 33, 16, 0, C.byref(p), L.u8ptr(buf), len(want) - 1, C.byref(n)) == -1
    assert n.value == len(want) and (buf == 7).all() and b"fspt_jpeg_encode" in lib.fspt_last_error()
    assert lib.fspt_jpeg_encode(0, L.u8ptr(a), 33, 16, 0, C.byref(p), L.u8ptr(buf), len(want), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want and (buf[n.value:] == 7).all()
    assert lib.fspt_jpeg_encode(0, L.u8ptr(a), 33, 16, 0, None, L.u8ptr(buf), buf.size, C.byref(n)) == 0  # NULL = 85, 420, 0
    assert buf[:n.value].tobytes() == want
    b = C.c_size_t()
    assert lib.fspt_jpeg_bound(33, 16, C.byref(p), C.byref(b)) == 0 and b.value >= len(want)


def test_pillow_decodes_the_gpu_files():
    """the GPU's 64x80 files are Pillow's own, so they decode to what Pillow's decode"""
    Image = pytest.importorskip("PIL.Image")
    a = image("noise", 64, 80)
    for sub, quality in itertools.product(SUBS, (10, 85)):
        got = fspt_amd.jpeg_encode(a, quality, sub[0], 3)
        ref = io.BytesIO()
        Image.fromarray(a[..., :3]).save(ref, "JPEG", quality=quality, subsampling=0 if sub[1] == J.S444 else 2, optimize=False, restart_marker_blocks=3)
        assert got == ref.getvalue()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), np.asarray(Image.open(io.BytesIO(ref.getvalue()))))


# ---- the target's entries -------------------------------------------------------------------------------------------
W, H = 64, 48


def make_pt(arrays, cam, seed=7):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.seed(seed)
    return pt


def test_draw_jpeg_is_the_drawing_entry_encoded(small_scene, camera):
    pt = make_pt(small_scene, camera)
    pt.set_auto_exposure(True)
    pt.set_bloom(True)
    enc = dict(quality=75, subsampling="444", restart_mcus=3)
    # a missing denoise or temporal state: the error of the entry the source stands for
    pt.render(2)
    for source, entry in (("denoised", lambda: pt.drawDenoised()), ("temporal", lambda: pt.temporal_draw()),
                          ("temporal_denoised", lambda: pt.temporal_draw(denoised=True))):
        with pytest.raises(fspt_amd.FsptError) as e1:
            entry()
        with pytest.raises(fspt_amd.FsptError) as e2:
            pt.draw_jpeg(source)
        assert e1.value.args == e2.value.args and "-6" in str(e2.value), source
    pt.render(6)
    pt.features(samples=2)
    pt.denoise(iterations=2)
    pt.exposure_reset()
    want = pt.drawDenoised(1.3, 0.8)
    pt.exposure_reset()
    assert pt.draw_jpeg("denoised", 1.3, 0.8, **enc) == fspt_amd.jpeg_encode(want, bottom_up=True, **enc)
    pt.temporal_accumulate(read=False)
    with pytest.raises(fspt_amd.FsptError) as e1:
        pt.temporal_draw(denoised=True)
    with pytest.raises(fspt_amd.FsptError) as e2:
        pt.draw_jpeg("temporal_denoised")
    assert e1.value.args == e2.value.args
    pt.temporal_denoise(iterations=1)
    for source, denoised in (("temporal", False), ("temporal_denoised", True)):
        pt.exposure_reset()
        want = pt.temporal_draw(0.9, 1.1, denoised=denoised)
        pt.exposure_reset()
        assert pt.draw_jpeg(source, 0.9, 1.1, **enc) == fspt_amd.jpeg_encode(want, bottom_up=True, **enc), source
    # the accumulator, under a viewport and a scale below 1 (the temporal stages refuse a viewport: last)
    pt.set_viewport(48, 32)
    pt.render(3)
    for kw in (dict(scale=0.5), dict(denoise=True, max_sigma=1.5, exposure=1.4)):
        pt.exposure_reset()
        want = pt.draw(**kw)
        pt.exposure_reset()
        got = pt.draw_jpeg("accumulator", **kw)  # the defaults: 85, 4:2:0, one MCU row per interval
        assert got == fspt_amd.jpeg_encode(want, bottom_up=True) == J.encode(want, True), kw
    with pytest.raises(ValueError):
        pt.draw_jpeg("radiance")
    pt.close()


def test_present_jpeg_frame_by_frame(small_scene, camera):
    pt, twin, plain = make_pt(small_scene, camera), make_pt(small_scene, camera), make_pt(small_scene, camera)
    kw = dict(exposure=1.2, quality=60, subsampling="420", restart_mcus=2)
    frames = []
    for k in range(6):
        pt.tick()
        data, ticks = pt.present_jpeg(**kw)
        if k == 0:
            assert data is None and ticks == 0
        else:
            assert ticks == k
            while twin.pingpong < k:
                twin.tick()
            assert data == twin.draw_jpeg("accumulator", **kw), k
            frames.append(data)
    assert len(set(frames)) > 1
    # a buffer one byte short: -1, the size needed, nothing written; the frame is dropped and the pipeline goes on
    lib, p = L.lib(), L.JpegParams(60, 1, 2)
    twin.tick()  # tick 6: what the next call returns
    need = len(twin.draw_jpeg("accumulator", **kw))
    buf, n, t = np.full(need + 16, 9, np.uint8), C.c_size_t(), C.c_uint32(77)
    pt.tick()
    assert lib.fspt_present_jpeg(pt._t, 1.2, 1.0, 0, 3.0, 1.0, C.byref(p), L.u8ptr(buf), need - 1, C.byref(n), C.byref(t)) == -1
    assert n.value == need and (buf == 9).all() and b"fspt_present_jpeg" in lib.fspt_last_error()
    pt.tick()
    twin.tick(); twin.tick()
    data, ticks = pt.present_jpeg(**kw)  # the frame the refused call enqueued: tick 7
    assert ticks == 7
    twin7 = make_pt(small_scene, camera)
    for _ in range(7):
        twin7.tick()
    assert data == twin7.draw_jpeg("accumulator", **kw)
    twin7.close()
    # alternating with present: a call returns the previous frame only when the same entry enqueued it
    img, ticks = pt.present(exposure=1.2)
    assert img is None and ticks == 0            # the frame in flight was a file
    pt.tick()
    img, ticks = pt.present(exposure=1.2)
    assert ticks == 8 and np.array_equal(img, twin.draw(exposure=1.2))
    pt.tick()
    data, ticks = pt.present_jpeg(**kw)
    assert data is None and ticks == 0           # the frame in flight was RGBA8
    data, ticks = pt.present_jpeg(**kw)
    assert ticks == 10 and data is not None
    # the accumulator ends where present alone leaves it
    pt.sync()
    for _ in range(10):
        plain.tick()
        plain.present()
    plain.sync()
    assert pt.pingpong == plain.pingpong == 10 and np.array_equal(pt.readRadiance(), plain.readRadiance())
    for x in (pt, twin, plain):
        x.close()


def test_hosts_write_jpeg(tmp_path, small_scene, camera):
    """render.py --out x.jpg writes the file draw_jpeg returns, and the viewer's frame loop yields present_jpeg's files"""
    import os
    import sys
    from fspt_amd import render as R, scene as S
    out = tmp_path / "x.jpg"
    R.main(["--out", str(out), "--jpeg-quality", "70", "--jpeg-444", "--width", "40", "--height", "24", "--spp", "3", "--mesh-n", "8", "--bounces", "4"])
    pt = PathTracer(S.bunny_scene(n=8), 40, 24, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.render(3)
    want = pt.draw_jpeg(quality=70, subsampling="444")
    assert out.read_bytes() == want == J.encode(pt.draw(), True, 70, J.S444)
    pt.close()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import view_server as V
    pt, twin = make_pt(small_scene, camera), make_pt(small_scene, camera)
    got = list(itertools.islice(V.frames(pt, 1.0, 85, False, max_ticks=3), 4))
    for k, data in enumerate(got):  # frames of 1, 2, 3 ticks, then the converged frame again
        if twin.pingpong < min(k + 1, 3):
            twin.tick()
        assert data == twin.draw_jpeg(), k
    assert got[2] == got[3] != got[1]
    pt.close(); twin.close()
