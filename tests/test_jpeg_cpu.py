"""The JPEG encoder on a box without a GPU: the integer restatement tests/jpeg_ref.py - the yardstick of
tests/test_jpeg_gpu.py - against libjpeg (Pillow) file for file; 4:2:0 off the MCU grid, where the restatement is the
definition, by decoded error; the Node host's decoder on its files; fspt_jpeg_bound; the ABI's argument checks and its
refusal to compute without a device; the MJPEG framing; the hosts' .jpg output flags; the committed tables."""
import ctypes as C
import io
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fspt_amd import _lib as L

import jpeg_ref as J
from jpeg_cases import CONTENTS, image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (10, 50, 85, 100)
NONE = 65535  # "no restart markers": an interval longer than any image here (libjpeg writes DRI 65535 too, so whole files compare)
RESTARTS = (NONE, 1, 3)
ON_GRID = ((J.S444, [(1, 1), (9, 17), (19, 37), (64, 80)]), (J.S420, [(16, 16), (32, 48), (64, 80)]))
OFF_GRID_420 = [(9, 17), (19, 37), (8, 23), (30, 16), (17, 32)]


def pillow_file(a, quality, sub, restart):
    from PIL import Image
    b = io.BytesIO()
    kw = {"restart_marker_blocks": restart} if restart else {}
    Image.fromarray(a[..., :3]).save(b, "JPEG", quality=quality, subsampling=0 if sub == J.S444 else 2, optimize=False, **kw)
    return b.getvalue()


def decoded(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


@pytest.mark.parametrize("content", CONTENTS)
def test_restatement_is_libjpeg_on_the_grid(content):
    """whole files, byte for byte - headers, tables (the quality rule and Annex K as typed here), entropy-coded data,
    markers: no header field needed to be excepted"""
    pytest.importorskip("PIL")
    n = 0
    for sub, sizes in ON_GRID:
        for (w, h), quality, restart in itertools.product(sizes, QUALITIES, RESTARTS):
            a = image(content, w, h)
            assert J.encode(a, False, quality, sub, restart) == pillow_file(a, quality, sub, restart), (content, sub, w, h, quality, restart)
            n += 1
    assert n == 7 * 4 * 3


def test_restatement_default_interval_and_row_order():
    """restart_mcus 0 = one MCU row (libjpeg's restart_in_rows = 1); bottom_up reads the rows the other way round; a file
    without DRI (Pillow's default) has the restatement's entropy-coded segment when no marker falls inside the image"""
    pytest.importorskip("PIL")
    from PIL import Image
    a = image("noise", 64, 80)
    for sub, pil_sub in ((J.S444, 0), (J.S420, 2)):
        b = io.BytesIO()
        Image.fromarray(a[..., :3]).save(b, "JPEG", quality=85, subsampling=pil_sub, optimize=False, restart_marker_rows=1)
        assert J.encode(a, False, 85, sub, 0) == b.getvalue()
        assert J.encode(a[::-1], True, 85, sub, 0) == b.getvalue()
        mine, plain = J.encode(a, False, 85, sub, NONE), pillow_file(a, 85, sub, 0)
        dri = mine.index(b"\xFF\xDD")
        assert mine[:dri] + mine[dri + 6:] == plain


@pytest.mark.parametrize("size", OFF_GRID_420, ids=lambda s: f"{s[0]}x{s[1]}")
def test_420_off_the_grid_decodes_as_well_as_libjpeg(size):
    """libjpeg pads the downsampled chroma and inserts dummy blocks there; the restatement replicates the image's edge to
    the MCU grid first.  Both are valid files of the true size; the picture must be as good: mean absolute error against
    the source within 0.5 grey levels of Pillow's own file's (measured differences: at most 0.23)"""
    pytest.importorskip("PIL")
    w, h = size
    for content, quality, restart in itertools.product(("noise", "gradient", "saturated"), QUALITIES, (NONE, 1)):
        a = image(content, w, h)
        mine, ref = decoded(J.encode(a, False, quality, J.S420, restart)), decoded(pillow_file(a, quality, J.S420, restart))
        assert mine.shape == ref.shape == (h, w, 3)
        src = a[..., :3].astype(np.float64)
        e_mine, e_ref = np.abs(mine - src).mean(), np.abs(ref - src).mean()
        print(f"{w}x{h} {content} q{quality} r{restart}: mae {e_mine:.3f} vs libjpeg {e_ref:.3f}")
        assert e_mine <= e_ref + 0.5, (content, quality, restart, e_mine, e_ref)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_decoder_reads_the_restatements_files(tmp_path):
    """fspt_amd/js/jpeg.js decodes them to exactly what libjpeg decodes them to"""
    pytest.importorskip("PIL")
    from test_node_host import dec, run_node
    files = {}
    cases = [(J.S444, 19, 37, 85, 3, "noise"), (J.S444, 1, 1, 10, 0, "constant"), (J.S420, 64, 80, 100, 1, "saturated"),
             (J.S420, 17, 32, 50, 0, "gradient"), (J.S420, 30, 16, 85, NONE, "checkerboard")]
    for k, (sub, w, h, quality, restart, content) in enumerate(cases):
        data = J.encode(image(content, w, h), bool(k & 1), quality, sub, restart)
        f = str(tmp_path / f"{k}.jpg")
        open(f, "wb").write(data)
        files[f] = np.dstack([decoded(data), np.full((h, w), 255, np.uint8)])
    out = run_node("jpeg", {"files": sorted(files)})
    assert not out["errors"]
    for f, want in files.items():
        d = out["decoded"][f]
        assert (d["height"], d["width"]) == want.shape[:2] and np.array_equal(dec(d["rgba"], np.uint8).reshape(want.shape), want), f


def bound(w, h, p):
    n = C.c_size_t()
    assert L.lib().fspt_jpeg_bound(w, h, C.byref(p) if p is not None else None, C.byref(n)) == 0
    return n.value


def test_bound_holds_and_is_monotone():
    for (sub, restart), (w, h) in itertools.product(((J.S444, 0), (J.S420, 0), (J.S444, 1), (J.S420, 3)), ((1, 1), (17, 9), (64, 80))):
        a = image("noise", w, h)
        b = bound(w, h, L.JpegParams(100, sub, restart))
        assert b == J.bound(w, h, sub, restart) >= len(J.encode(a, False, 100, sub, restart)), (sub, restart, w, h)
    assert bound(64, 80, None) == bound(64, 80, L.JpegParams(85, J.S420, 0))
    for p in (L.JpegParams(85, J.S444, 0), L.JpegParams(85, J.S420, 0), L.JpegParams(85, J.S420, 5)):
        for w in range(1, 70):
            assert bound(w, 33, p) <= bound(w + 1, 33, p) and bound(33, w, p) <= bound(33, w + 1, p)
    assert bound(65535, 65535, L.JpegParams(100, J.S444, 1)) == J.bound(65535, 65535, J.S444, 1) > 2 ** 32  # size_t arithmetic


DEVICE_ENTRIES = ("fspt_jpeg_encode", "fspt_jpeg_encode_device")


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fspt.h")).read() + open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("fspt_jpeg_bound", "fspt_jpeg_encode", "fspt_jpeg_encode_device", "fspt_draw_jpeg", "fspt_present_jpeg",
                 "fspt_jpeg_coefficients_eval", "fspt_jpeg_last_ms"):
        assert f"int {name}(" in text and hasattr(lib, name) and name in L.SIGNATURES, name
    assert "FSPT_JPEG_444 = 0, FSPT_JPEG_420 = 1" in text and "FSPT_SOURCE_TEMPORAL_DENOISED = 3" in text


def test_invalid_arguments_are_refused_before_a_device_is_touched():
    lib = L.lib()
    a = image("noise", 8, 8)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    ok = L.JpegParams(85, 1, 0)

    def refused(name, rc):
        assert rc == -1 and name.encode() in lib.fspt_last_error(), (name, rc, lib.fspt_last_error())
        assert n.value == 77 and (out == 5).all()
    for name in DEVICE_ENTRIES:
        fn = getattr(lib, name)
        src = L.u8ptr(a) if name == "fspt_jpeg_encode" else C.c_void_p(a.ctypes.data)
        refused(name, fn(0, None, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        refused(name, fn(0, src, 8, 8, 0, C.byref(ok), None, out.size, C.byref(n)))
        refused(name, fn(0, src, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, None))
        for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
            refused(name, fn(0, src, w, h, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        for bad in (L.JpegParams(0, 1, 0), L.JpegParams(101, 1, 0), L.JpegParams(85, 2, 0), L.JpegParams(85, 1, 65536)):
            refused(name, fn(0, src, 8, 8, 0, C.byref(bad), L.u8ptr(out), out.size, C.byref(n)))
    coef = np.zeros(6 * 64, np.int16)
    cp = coef.ctypes.data_as(C.POINTER(C.c_int16))
    refused("fspt_jpeg_coefficients_eval", lib.fspt_jpeg_coefficients_eval(0, L.u8ptr(a), 8, 8, 0, C.byref(ok), None))
    refused("fspt_jpeg_coefficients_eval", lib.fspt_jpeg_coefficients_eval(0, L.u8ptr(a), 8, 8, 0, C.byref(L.JpegParams(0, 1, 0)), cp))
    b = C.c_size_t(77)
    assert lib.fspt_jpeg_bound(8, 8, C.byref(ok), None) == -1 and b"fspt_jpeg_bound" in lib.fspt_last_error()
    for w, h, p in ((0, 8, ok), (8, 65536, ok), (8, 8, L.JpegParams(85, 7, 0)), (8, 8, L.JpegParams(200, 0, 0)), (8, 8, L.JpegParams(85, 0, 70000))):
        assert lib.fspt_jpeg_bound(w, h, C.byref(p), C.byref(b)) == -1 and b"fspt_jpeg_bound" in lib.fspt_last_error() and b.value == 77
    # the target's entries: a NULL target, before anything else
    t = C.c_uint32(9)
    refused("fspt_draw_jpeg", lib.fspt_draw_jpeg(None, 0, 1.0, 1.0, 0, 3.0, 1.0, None, L.u8ptr(out), out.size, C.byref(n)))
    refused("fspt_present_jpeg", lib.fspt_present_jpeg(None, 1.0, 1.0, 0, 3.0, 1.0, None, L.u8ptr(out), out.size, C.byref(n), C.byref(t)))
    assert t.value == 9
    assert lib.fspt_jpeg_last_ms(None, None) == -1


def test_no_device_no_encode():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    a = image("noise", 8, 8)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    for name in DEVICE_ENTRIES:
        src = L.u8ptr(a) if name == "fspt_jpeg_encode" else C.c_void_p(a.ctypes.data)
        assert getattr(lib, name)(0, src, 8, 8, 0, None, L.u8ptr(out), out.size, C.byref(n)) == -2
        assert name.encode() in lib.fspt_last_error() and b"no CPU fallback" in lib.fspt_last_error()
        assert n.value == 77 and (out == 5).all()
    coef = np.zeros(6 * 64, np.int16)
    assert lib.fspt_jpeg_coefficients_eval(0, L.u8ptr(a), 8, 8, 0, None, coef.ctypes.data_as(C.POINTER(C.c_int16))) == -2
    assert b"no CPU fallback" in lib.fspt_last_error() and not coef.any()
    import fspt_amd
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        fspt_amd.jpeg_encode(a)


def test_wrapper_argument_checks():
    import fspt_amd
    with pytest.raises(ValueError):
        fspt_amd.jpeg_encode(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        fspt_amd.jpeg_encode(np.zeros((8, 8, 4), np.uint8), subsampling="422")
    assert fspt_amd.jpeg_bound(64, 80) == J.bound(64, 80)


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    """the addon built against tests/napi_mock and tests/jpeg_mock_stub.c, as tests/test_present_cpu.py does"""
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    import json
    d = str(tmp_path_factory.mktemp("jpeg_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "jpeg_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "jpeg_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def mock_file(tag, a, quality=85, sub=1, restart=0):
    return [0xFF, 0xD8, ord(tag), a, quality, sub * 16 + restart, 0xFF, 0xD9]


def test_js_jpeg_calls_go_through_the_addon(js_report):
    r = js_report
    assert r["draw"] == mock_file("D", 3, 60, 0, 3) and r["drawIsBuffer"]       # source temporalDenoised = 3
    assert r["drawDefault"] == mock_file("D", 0) and r["bufferBytes"] == 3 * 2 * 4 + 1024
    assert r["present"] == {"jpeg": mock_file("P", 1, 50), "ticks": 7, "isBuffer": True}
    assert r["presentNothing"] == {"jpeg": None, "ticks": 0}
    assert r["encode"] == mock_file("E", 5 * 2 + 1, 90) and r["encodeIsBuffer"]


def test_js_jpeg_buffer_grows_to_the_bound(js_report):
    r = js_report
    assert r["grownDraw"] == mock_file("D", 1) and r["grownBytes"] == 1000 + 3 * 2
    assert r["droppedPresent"] == {"jpeg": None, "ticks": 0, "bytes": 1000 + 3 * 2} and r["afterDrop"] == 7


def test_js_jpeg_argument_checks(js_report):
    r = js_report
    assert r["badSource"] == "RangeError: drawJpeg: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'"
    assert r["badSub"] == "RangeError: presentJpeg: subsampling must be '444' or '420'"
    assert r["badQuality"] == "RangeError: drawJpeg: quality must be an integer in 1..100"
    assert r["badRestart"] == "RangeError: presentJpeg: restartMcus must be an integer in 0..65535"
    assert r["encodeShort"] == "RangeError: jpegEncode: need a Uint8Array of width*height*4 bytes"
    assert r["encodeBadSub"] == "RangeError: jpegEncode: subsampling must be '444' or '420'"


def test_js_jpeg_refused_during_render_async(js_report):
    r = js_report
    assert r["duringDraw"] == r["duringPresent"] == "Error: render in flight" and r["after"] is None


def test_mjpeg_part_framing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import view_server as V
    data = J.encode(image("gradient", 8, 8))
    part = V.mjpeg_part(data)
    head, _, rest = part.partition(b"\r\n\r\n")
    assert head.split(b"\r\n") == [b"--" + V.BOUNDARY.encode(), b"Content-Type: image/jpeg", b"Content-Length: %d" % len(data)]
    assert rest == data + b"\r\n"
    assert V.mjpeg_part(bytearray(b"ab")).endswith(b"\r\n\r\nab\r\n")
    stream = V.mjpeg_part(data) + V.mjpeg_part(data[:100])  # parts follow one another without anything between them
    assert stream.count(b"--" + V.BOUNDARY.encode() + b"\r\n") == 2


def test_render_cli_takes_jpg(tmp_path):
    """--out x.jpg is parsed with its flags, and without a device the render is refused with the usual message"""
    import fspt_amd
    from fspt_amd import render as R
    from fspt_amd.scene_file import is_jpeg_path
    assert is_jpeg_path("a/b.JPG") and is_jpeg_path("x.jpeg") and not is_jpeg_path("x.png") and not is_jpeg_path("jpg")
    for bad in (["--out", "x.png", "--jpeg-444"], ["--out", "x.png", "--jpeg-quality", "50"], ["--out", "x.jpg", "--jpeg-quality", "0"]):
        with pytest.raises(SystemExit):
            R.main(bad)
    if L.lib().fspt_device_count() > 0:
        pytest.skip("GPU present")
    out = tmp_path / "x.jpg"
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        R.main(["--out", str(out), "--jpeg-quality", "90", "--jpeg-444", "--width", "32", "--height", "16", "--spp", "1", "--mesh-n", "4"])
    assert not out.exists()


def test_committed_tables_are_the_generators():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_jpeg_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_jpeg_tables as T
    assert T.zigzag() == J.ZIGZAG and T.QUANT_LUMA == J.QUANT_LUMA and T.QUANT_CHROMA == J.QUANT_CHROMA
    assert T.AC_LUMA_VALS == J.AC_LUMA_VALS and T.AC_CHROMA_VALS == J.AC_CHROMA_VALS
    assert "JPEG_BLOCK_MAX_BITS = 1660u" in T.text()
