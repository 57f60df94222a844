"""The GPU PNG encoder (include/fspt.h fspt_png_*, fspt_draw_png) on the MI355X against the integer
restatement tests/png_ref.py: stage one's filtered stream and the whole file, byte for byte, at sizes of one chunk and many,
chunk boundaries inside rows and inside runs, both channel counts, both row orders, every filter, both code limits; the
device form; determinism; alpha; draw_png against the drawing entries it stands for, its cap check and a change of the
parameters between two calls."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import fspt_amd
from fspt_amd import PathTracer, _lib as L

import png_ref as P
from png_cases import CONTENTS, FIBONACCI, FIBONACCI_CL, LARGE, SMALL, image

pytestmark = pytest.mark.gpu


def check_case(a, channels, filt, chunk_bytes, bottom_up):
    stats = {}
    want = P.encode(a, bottom_up, channels, filt, chunk_bytes, stats)
    key = (a.shape, channels, filt, chunk_bytes, bottom_up)
    got_s = fspt_amd.png_filtered_eval(a, channels, filt, bottom_up)
    assert got_s.tobytes() == stats["stream"], key
    got = fspt_amd.png_encode(a, channels, filt, chunk_bytes, bottom_up)
    assert got == want, (key, len(got), len(want))
    return want, stats


@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_sizes_every_setting(size):
    """adaptive and the five fixed filters x both channel counts x chunks of 256, 1000 and the default; the contents and
    the row orders dealt round-robin"""
    seen = set()
    for k, (filt, channels, cb) in enumerate(itertools.product((P.ADAPTIVE, 0, 1, 2, 3, 4), (3, 4), (256, 1000, 0))):
        content, bottom_up = CONTENTS[k % len(CONTENTS)], bool((k // len(CONTENTS) + k) & 1)
        check_case(image(content, *size), channels, filt, cb, bottom_up)
        seen.add(content); seen.add(bottom_up)
    assert len(seen) == len(CONTENTS) + 2


@pytest.mark.parametrize("content", CONTENTS)
def test_many_chunks(content):
    """(256, 144): four chunks of 32 KiB at three channels, and more of the smaller ones; `runs` under filter 0, where its
    runs of 258 and more bytes survive and straddle the chunks"""
    a = image(content, *LARGE)
    k = CONTENTS.index(content)
    filt = 0 if content == "runs" else P.ADAPTIVE
    _, st = check_case(a, 3, filt, 32768, bool(k & 1))
    assert len(st["blocks"]) == 4
    check_case(a, 4, filt, (0, 8192, 5000)[k % 3], not k & 1)
    if content == "noise":
        assert set(st["blocks"]) == {P.STORED}
    if content == "runs":
        assert set(st["blocks"]) == {P.DYNAMIC} and any(n >= 258 for kind, n in P.tokens(st["stream"][:32768]) if kind == "len")


@pytest.mark.parametrize("size,chunks", (((85, 256), 256), ((85, 257), 257), ((85, 513), 513), ((86, 255), 258)), ids=lambda v: str(v).replace(" ", ""))
def test_chunk_counts_around_the_offset_scans_width(size, chunks):
    """chunks of 256 bytes, a row of 85 RGB pixels being one: as many chunks as k_png_offsets scans in one tile of 256, one
    more, and two tiles and one - the carries of the offsets and of the Adler sums from tile to tile; 86 pixels: chunks off
    the row boundaries and a partial last one"""
    a = image("rendered", *size)
    _, st = check_case(a, 3, P.ADAPTIVE, 256, False)
    assert len(st["blocks"]) == chunks
    if chunks == 257:  # four channels: 341 bytes a row, 343 chunks off the rows
        _, st = check_case(a, 4, P.ADAPTIVE, 256, True)
        assert len(st["blocks"]) == (size[1] * (1 + 4 * size[0]) + 255) // 256 > 256


def test_both_code_limits_are_hit():
    """the literal/length code against 15 bits and the code-length code against 7: the restatement's statistics say that the
    limit was met, and the device's file is the restatement's"""
    _, st = check_case(image("fibonacci", FIBONACCI["w"], FIBONACCI["h"]), 3, 0, 32768, False)
    assert st["blocks"] == [P.DYNAMIC] and st["max_len"] == [15]
    _, st = check_case(image("fibonacci_cl", FIBONACCI_CL["w"], FIBONACCI_CL["h"]), 3, 0, 32768, False)
    assert st["blocks"] == [P.DYNAMIC] and st["max_cl_len"] == [7]


def test_device_form_determinism_and_alpha():
    import torch
    a = image("rendered", *LARGE)
    first = fspt_amd.png_encode(a, 3, "adaptive", 0, True)
    assert first == P.encode(a, True)
    for _ in range(3):  # the bits of neighbouring lanes are OR-ed into shared words in no fixed order
        assert fspt_amd.png_encode(a, 3, "adaptive", 0, True) == first
    t = torch.from_numpy(a).to("cuda:0")
    assert fspt_amd.png_encode(t, 3, "adaptive", 0, True) == first
    assert fspt_amd.png_encode(t, 4, "paeth", 1000, False) == P.encode(a, False, 4, 4, 1000)
    b = a.copy()
    b[..., 3] = 255 - b[..., 3]  # another alpha: the same RGB file, another and correct RGBA file
    assert fspt_amd.png_encode(b, 3, "adaptive", 0, True) == first
    got = fspt_amd.png_encode(b, 4)
    assert got == P.encode(b, False, 4) != fspt_amd.png_encode(a, 4)
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), b)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(first))), a[::-1, :, :3])


def test_cap_and_errors():
    lib = L.lib()
    a = image("gradient", 33, 16)
    want = P.encode(a)
    p = L.PngParams(3, 5, 0)
    buf = np.full(len(want) + 8, 7, np.uint8)
    n = C.c_size_t(123)
    assert lib.fspt_png_encode(0, L.u8ptr(a), 33, 16, 0, C.byref(p), L.u8ptr(buf), len(want) - 1, C.byref(n)) == -1
    assert n.value == len(want) and (buf == 7).all() and b"fspt_png_encode" in lib.fspt_last_error()
    assert lib.fspt_png_encode(0, L.u8ptr(a), 33, 16, 0, C.byref(p), L.u8ptr(buf), len(want), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want and (buf[n.value:] == 7).all()
    assert lib.fspt_png_encode(0, L.u8ptr(a), 33, 16, 0, None, L.u8ptr(buf), buf.size, C.byref(n)) == 0  # NULL = 3, adaptive, the default chunk
    assert buf[:n.value].tobytes() == want
    ms, bus = fspt_amd.png_last_ms()
    assert all(x > 0 for x in ms) and bus == len(want) + 4


# ---- the target's entry ---------------------------------------------------------------------------------------------
W, H = 64, 48


def make_pt(arrays, cam, seed=7):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.seed(seed)
    return pt


def decoded(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)))


def test_draw_png_is_the_drawing_entry_encoded(small_scene, camera):
    pt = make_pt(small_scene, camera)
    pt.set_auto_exposure(True)
    pt.set_bloom(True)
    pt.render(2)
    for source, entry in (("denoised", lambda: pt.drawDenoised()), ("temporal", lambda: pt.temporal_draw())):
        with pytest.raises(fspt_amd.FsptError) as e1:
            entry()
        with pytest.raises(fspt_amd.FsptError) as e2:
            pt.draw_png(source)
        assert e1.value.args == e2.value.args, source
    pt.render(6)
    pt.features(samples=2)
    pt.denoise(iterations=2)
    pt.exposure_reset()
    want = pt.drawDenoised(1.3, 0.8)
    pt.exposure_reset()
    got = pt.draw_png("denoised", 1.3, 0.8, channels=4, chunk_bytes=1000)
    assert got == P.encode(want, True, 4, P.ADAPTIVE, 1000)
    assert np.array_equal(decoded(got), want[::-1])
    pt.temporal_accumulate(read=False)
    pt.temporal_denoise(iterations=1)
    for source, denoised in (("temporal", False), ("temporal_denoised", True)):
        pt.exposure_reset()
        want = pt.temporal_draw(0.9, 1.1, denoised=denoised)
        pt.exposure_reset()
        got = pt.draw_png(source, 0.9, 1.1)  # the parameters change from call to call: RGB, the default chunk
        assert got == P.encode(want, True) and np.array_equal(decoded(got), want[::-1, :, :3]), source
    pt.set_viewport(48, 32)
    pt.render(3)
    for kw, enc in ((dict(scale=0.5), dict(filter="up", chunk_bytes=256)), (dict(denoise=True, max_sigma=1.5, exposure=1.4), dict(channels=4))):
        pt.exposure_reset()
        want = pt.draw(**kw)
        pt.exposure_reset()
        got = pt.draw_png("accumulator", **kw, **enc)
        ch = enc.get("channels", 3)
        assert got == P.encode(want, True, ch, fspt_amd.tracer.PNG_FILTERS[enc.get("filter", "adaptive")], enc.get("chunk_bytes", 0)), kw
        assert np.array_equal(decoded(got), want[::-1, :, :ch])
    with pytest.raises(ValueError):
        pt.draw_png("radiance")
    # a buffer one byte short: -1, the size needed, nothing written
    lib, p = L.lib(), L.PngParams(4, 5, 0)
    need = len(got)
    buf, n = np.full(need + 16, 9, np.uint8), C.c_size_t()
    pt.exposure_reset()
    assert lib.fspt_draw_png(pt._t, 0, 1.4, 1.0, 1, 1.5, 1.0, C.byref(p), L.u8ptr(buf), need - 1, C.byref(n)) == -1
    assert n.value == need and (buf == 9).all() and b"fspt_draw_png" in lib.fspt_last_error()
    pt.exposure_reset()
    assert lib.fspt_draw_png(pt._t, 0, 1.4, 1.0, 1, 1.5, 1.0, C.byref(p), L.u8ptr(buf), need, C.byref(n)) == 0
    assert buf[:n.value].tobytes() == got and (buf[need:] == 9).all()
    pt.close()


def test_hosts_write_png(tmp_path):
    """render.py --out x.png --png-gpu writes the file draw_png returns; write_image(png=...) the file png_encode returns"""
    from fspt_amd import render as R, scene as S
    from fspt_amd.scene_file import write_image
    out = tmp_path / "x.png"
    R.main(["--out", str(out), "--png-gpu", "--width", "40", "--height", "24", "--spp", "3", "--mesh-n", "8", "--bounces", "4"])
    pt = PathTracer(S.bunny_scene(n=8), 40, 24, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.render(3)
    frame = pt.draw()
    assert out.read_bytes() == pt.draw_png() == P.encode(frame, True)
    pt.close()
    top_down = np.ascontiguousarray(frame[::-1])
    write_image(str(tmp_path / "a.png"), top_down, png="gpu")
    assert (tmp_path / "a.png").read_bytes() == P.encode(top_down)
    write_image(str(tmp_path / "b.png"), top_down, png={"channels": 4, "filter": "sub", "chunk_bytes": 512})
    assert (tmp_path / "b.png").read_bytes() == P.encode(top_down, False, 4, 1, 512)
