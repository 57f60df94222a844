"""The OpenEXR encoder (include/fspt.h fspt_exr_*, fspt_draw_exr) without a GPU: tests/exr_ref.py's writer
restatement against its independent strict reader on every case the GPU has to reproduce, the half conversion against numpy
and an explicit edge list, the host-only entries and every refusal that comes before a device is touched, the wrappers'
argument checks, and the JS host on a mock library."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from fspt_amd import _lib as L

import exr_ref as X
from exr_cases import ALL_LAYERS, EDGE_BITS, buffers, case_id, cases, radiance, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()
ENCODE_ENTRIES = ("fspt_exr_encode", "fspt_exr_encode_device")
SOURCE = {"A": 3, "B": 2, "G": 1, "R": 0, "albedo.R": 4, "albedo.G": 5, "albedo.B": 6, "Z": 7, "N.X": 8, "N.Y": 9, "N.Z": 10}


def stated_conversion(values, ptype):
    """float32 values as the file has to hold them, by numpy's conversion and not the restatement's: bit patterns"""
    v = np.ascontiguousarray(values, np.float32)
    nan = np.isnan(v)
    if ptype == X.HALF:
        with np.errstate(over="ignore"):
            return np.where(nan, np.uint16(0x7E00), np.where(nan, np.float32(0), v).astype(np.float16).view(np.uint16))
    return np.where(nan, np.uint32(0x7FC00000), v.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reader_returns_what_the_writer_was_given(case):
    kind, w, h, comp, pt, layers, cb, up, _ = case
    data, st = reference(case)
    rgba, feat = buffers(case)
    got = X.read(data)
    assert (got["w"], got["h"], got["compression"]) == (w, h, comp)
    assert [n for n, _ in got["channels"]] == [n for n, _, _ in X.channel_list(pt, layers)]
    assert got["raw"] == st["raw"]
    src = rgba if feat is None else np.concatenate([rgba, feat], axis=2)
    if up:
        src = src[::-1]
    for name, t in got["channels"]:
        assert t == (X.FLOAT if name == "Z" else pt), name
        want = stated_conversion(src[..., SOURCE[name]], t)
        assert np.array_equal(got["planes"][name].view(want.dtype), want), name
    assert len(data) <= X.bound(w, h, comp, pt, layers)
    n = C.c_size_t()
    p = L.ExrParams(comp, pt, layers, cb)
    assert L.lib().fspt_exr_bound(w, h, C.byref(p), C.byref(n)) == 0 and n.value == X.bound(w, h, comp, pt, layers)


def test_the_split_image_has_compressed_and_raw_blocks():
    seen = 0
    for case in CASES:
        if case[0] != "split":
            continue
        data, st = reference(case)
        half = len(st["raw"]) // 2
        want = [False] * half + [True] * (len(st["raw"]) - half)  # the buffer's first rows are constant, its last ones noise
        assert st["raw"] == (want[::-1] if case[7] else want), case_id(case)
        got = X.read(data)
        for k, raw in enumerate(st["raw"]):
            assert (got["sizes"][k] == len(st["blocks"][k])) == raw
        seen += 1
    assert seen == 2


def test_half_conversion_against_numpy_and_the_edges():
    rng = np.random.default_rng(5)
    bits = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                           # dense around the half range's ends, where rounding carries into the exponent or leaves the normal range
                           (0x33000000 + rng.integers(0, 0x06000000, 100000)).astype(np.uint32), (0x47000000 + rng.integers(0, 0x01000000, 50000)).astype(np.uint32),
                           np.arange(0x387FC000, 0x38804000, dtype=np.uint32), np.array(EDGE_BITS, np.uint32)])
    v = bits.view(np.float32)
    ok = ~np.isnan(v)
    with np.errstate(over="ignore"):
        want = v[ok].astype(np.float16).view(np.uint16)
    assert np.array_equal(X.half_bits(bits[ok]), want)
    assert (X.half_bits(bits[~ok]) == 0x7E00).all() and (X.float_bits(bits[~ok]) == 0x7FC00000).all()
    assert np.array_equal(X.float_bits(bits[ok]), bits[ok])
    edges = {0x00000000: 0x0000, 0x80000000: 0x8000, 0x33800000: 0x0001, 0x33000000: 0x0000, 0x33000001: 0x0001, 0xB3000000: 0x8000, 0xB3000001: 0x8001,
             0x477FE000: 0x7BFF, 0x477FF000: 0x7C00, 0x477FEFFF: 0x7BFF, 0xC77FF000: 0xFC00, 0x7F7FFFFF: 0x7C00, 0xFF7FFFFF: 0xFC00,
             0x00800000: 0x0000, 0x80800000: 0x8000, 0x00000001: 0x0000, 0x007FFFFF: 0x0000, 0x80000001: 0x8000, 0x38800000: 0x0400, 0x387FFFFF: 0x0400,
             0x387FE000: 0x0400, 0x33C00000: 0x0002, 0x34400000: 0x0003, 0x34200000: 0x0002, 0x3F800000: 0x3C00, 0x3F801000: 0x3C00, 0x3F803000: 0x3C02,
             0x3F801001: 0x3C01, 0xBF800FFF: 0xBC00, 0x47800000: 0x7C00, 0x7F800000: 0x7C00, 0xFF800000: 0xFC00, 0x7FC00000: 0x7E00, 0xFFC00000: 0x7E00,
             0x7F800001: 0x7E00, 0xFF800001: 0x7E00, 0x7FFFFFFF: 0x7E00, 0xFFFFFFFF: 0x7E00, 0x7FA5A5A5: 0x7E00, 0xFFC00001: 0x7E00}
    assert set(edges) <= set(EDGE_BITS)
    for b, hb in edges.items():
        assert int(X.half_bits(np.array([b], np.uint32))[0]) == hb, hex(b)


def test_the_file_by_hand():
    """a 2 x 1 RGB HALF file without compression, byte by byte; and the same pixels' ZIPS block inflated by zlib"""
    rgba = np.array([[[1.0, 2.0, 0.5, 9.0], [-2.0, 65536.0, 0.0, 9.0]]], np.float32)
    data = X.encode(rgba, compression=X.NONE)
    hdr = X.header(2, 1, X.NONE, X.channel_list())
    assert hdr.startswith(b"\x76\x2f\x31\x01\x02\x00\x00\x00channels\0chlist\0" + struct.pack("<i", 3 * 18 + 1) + b"B\0" + struct.pack("<iIii", 1, 0, 1, 1) + b"G\0")
    assert hdr.endswith(b"screenWindowWidth\0float\0\x04\0\0\0\0\0\x80\x3f\0")
    raw = struct.pack("<6H", 0x3800, 0x0000, 0x4000, 0x7C00, 0x3C00, 0xC000)  # B, G, R planes
    assert data == hdr + struct.pack("<Qii", len(hdr) + 8, 0, 12) + raw
    wide = np.repeat(rgba, 40, axis=0).reshape(1, 80, 4)  # the two pixels 40 times in a row
    z = X.encode(wide, compression=X.ZIPS)
    got = X.read(z)
    assert got["raw"] == [False] and got["sizes"][0] < 80 * 6
    at = len(X.header(80, 1, X.ZIPS, X.channel_list())) + 8 + 8
    raw80 = b"".join(struct.pack("<80H", *(pair * 40)) for pair in ([0x3800, 0x0000], [0x4000, 0x7C00], [0x3C00, 0xC000]))
    tt = raw80[0::2] + raw80[1::2]
    assert zlib.decompress(z[at:]) == bytes([tt[0]] + [(tt[i] - tt[i - 1] + 128) & 255 for i in range(1, len(tt))])


def test_reader_is_strict():
    data = bytearray(reference(CASES[-3])[0])
    X.read(bytes(data))
    for at, what in ((0, "magic"), (4, "version"), (len(data) - 1, None)):
        bad = bytearray(data)
        bad[at] ^= 0x40
        if what:
            with pytest.raises(X.ExrError, match=what):
                X.read(bytes(bad))
    with pytest.raises(X.ExrError, match="behind the last block"):
        X.read(bytes(data) + b"\0")
    with pytest.raises(X.ExrError):
        X.read(bytes(data[:-1]))
    hdr_len = len(X.header(len(EDGE_BITS), 3, X.ZIP, X.channel_list(X.HALF, ALL_LAYERS)))
    bad = bytearray(data)
    bad[hdr_len] ^= 1  # the first entry of the offset table
    with pytest.raises(X.ExrError, match="offset of block 0"):
        X.read(bytes(bad))
    bad = bytearray(data)
    bad[8:16] = b"Channels"
    with pytest.raises(X.ExrError, match="attributes"):
        X.read(bytes(bad))


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fspt.h")).read() + open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("fspt_exr_bound", "fspt_exr_encode", "fspt_exr_encode_device", "fspt_draw_exr", "fspt_exr_last_ms", "fspt_exr_set_form"):
        assert f"int {name}(" in text and hasattr(lib, name) and name in L.SIGNATURES, name
    assert "uint32_t compression, pixel_type, layers, chunk_bytes;" in text and "FSPT_EXR_ZIPS = 2, FSPT_EXR_ZIP = 3" in text
    assert "FSPT_EXR_ALPHA = 1, FSPT_EXR_ALBEDO = 2, FSPT_EXR_NORMAL = 4, FSPT_EXR_DEPTH = 8" in text


def test_invalid_arguments_are_refused_before_a_device_is_touched():
    lib = L.lib()
    a, f = radiance("rendered", 8, 8), np.zeros((8, 8, 8), np.float32)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    ok = L.ExrParams(3, 1, 0, 0)
    bad_params = (L.ExrParams(1, 1, 0, 0), L.ExrParams(4, 1, 0, 0), L.ExrParams(3, 0, 0, 0), L.ExrParams(3, 3, 0, 0), L.ExrParams(3, 1, 16, 0),
                  L.ExrParams(3, 1, 0, 255), L.ExrParams(3, 1, 0, 32769))

    def refused(name, rc):
        assert rc == -1 and name.encode() in lib.fspt_last_error(), (name, rc, lib.fspt_last_error())
        assert n.value == 77 and (out == 5).all()
    for name in ENCODE_ENTRIES:
        fn = getattr(lib, name)
        src, fsrc = (L.fptr(a), L.fptr(f)) if name == "fspt_exr_encode" else (C.c_void_p(a.ctypes.data), C.c_void_p(f.ctypes.data))
        refused(name, fn(0, None, fsrc, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        refused(name, fn(0, src, None, 8, 8, 0, C.byref(ok), None, out.size, C.byref(n)))
        refused(name, fn(0, src, None, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, None))
        for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
            refused(name, fn(0, src, None, w, h, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        for bad in bad_params:
            refused(name, fn(0, src, fsrc, 8, 8, 0, C.byref(bad), L.u8ptr(out), out.size, C.byref(n)))
        for layers in (X.ALBEDO, X.NORMAL, X.DEPTH, ALL_LAYERS):  # feature layers and no features
            p = L.ExrParams(3, 1, layers, 0)
            refused(name, fn(0, src, None, 8, 8, 0, C.byref(p), L.u8ptr(out), out.size, C.byref(n)))
        refused(name, fn(0, src, None, 65535, 65535, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))  # a file that could pass 4 GiB
    b = C.c_size_t(77)
    assert lib.fspt_exr_bound(8, 8, C.byref(ok), None) == -1 and b"fspt_exr_bound" in lib.fspt_last_error()
    for w, h, p in [(0, 8, ok), (8, 65536, ok)] + [(8, 8, p) for p in bad_params]:
        assert lib.fspt_exr_bound(w, h, C.byref(p), C.byref(b)) == -1 and b"fspt_exr_bound" in lib.fspt_last_error() and b.value == 77
    assert lib.fspt_exr_bound(65535, 65535, C.byref(ok), C.byref(b)) == 0 and b.value == X.bound(65535, 65535)  # the host-only entry has no 4 GiB limit
    assert lib.fspt_exr_bound(64, 48, None, C.byref(b)) == 0 and b.value == X.bound(64, 48, X.ZIP, X.HALF, 0)  # NULL = ZIP, HALF, RGB
    refused("fspt_draw_exr", lib.fspt_draw_exr(None, 0, None, L.u8ptr(out), out.size, C.byref(n)))
    assert lib.fspt_exr_last_ms(None, None) == -1
    assert lib.fspt_exr_set_form(2) == -1 and lib.fspt_exr_set_form(0) == 0


def test_no_device_no_encode():
    import fspt_amd
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        return  # (tests/test_exr_gpu.py has the device's side)
    a = radiance("rendered", 8, 8)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    for name in ENCODE_ENTRIES:
        src = L.fptr(a) if name == "fspt_exr_encode" else C.c_void_p(a.ctypes.data)
        assert getattr(lib, name)(0, src, None, 8, 8, 0, None, L.u8ptr(out), out.size, C.byref(n)) == -2
        assert name.encode() in lib.fspt_last_error() and b"no CPU fallback" in lib.fspt_last_error()
        assert n.value == 77 and (out == 5).all()
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        fspt_amd.exr_encode(a)


def test_wrapper_argument_checks(tmp_path):
    import fspt_amd
    from fspt_amd.scene_file import write_image
    a = radiance("rendered", 9, 5)
    with pytest.raises(ValueError):
        fspt_amd.exr_encode(a[..., :3])
    with pytest.raises(ValueError):
        fspt_amd.exr_encode(a.astype(np.float64))
    with pytest.raises(ValueError):
        fspt_amd.exr_encode(a, compression="piz")
    with pytest.raises(ValueError):
        fspt_amd.exr_encode(a, layers=["uv"])
    with pytest.raises(ValueError):
        fspt_amd.exr_encode(a, np.zeros((5, 9, 4), np.float32), layers=["albedo"])
    assert fspt_amd.exr_bound(64, 80) == X.bound(64, 80)
    assert fspt_amd.exr_bound(64, 80, "zips", True, "albedo,depth") == X.bound(64, 80, X.ZIPS, X.FLOAT, X.ALBEDO | X.DEPTH)
    assert fspt_amd.exr_bound(7, 3, "none", False, ALL_LAYERS) == X.bound(7, 3, X.NONE, X.HALF, ALL_LAYERS)
    with pytest.raises(ValueError):
        write_image(str(tmp_path / "x.exr"), np.zeros((5, 9, 4), np.uint8))  # an .exr takes the float radiance, not a drawn frame
    if L.lib().fspt_device_count() <= 0:
        with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
            write_image(str(tmp_path / "z.exr"), a)
        assert not (tmp_path / "z.exr").exists()


def test_render_cli_takes_exr(tmp_path, capsys):
    """the EXR options are parsed and checked with their own messages; a valid command line gets past the parser and,
    without a device, is refused by the library with the usual message"""
    import fspt_amd
    from fspt_amd import render as R

    def refused(argv, text):
        with pytest.raises(SystemExit):
            R.main(argv)
        assert text in capsys.readouterr().err, argv
    refused(["--out", "x.png", "--exr-layers", "albedo"], "--exr-layers, --exr-float and --exr-compression need an --out or --hdr that ends in .exr")
    refused(["--out", "x.png", "--hdr", "x.npy", "--exr-float"], "need an --out or --hdr that ends in .exr")
    refused(["--out", "x.exr", "--exr-layers", "uv"], "--exr-layers: layers must be among")
    refused(["--out", "x.exr", "--exr-compression", "piz"], "--exr-compression: invalid choice: 'piz'")
    refused(["--scene", "s.json", "--out", "x.exr", "--exr-layers", "depth"], "--exr-layers albedo, normal and depth are available for the built-in scene")
    if L.lib().fspt_device_count() > 0:
        return  # (tests/test_exr_gpu.py test_hosts_write_exr renders through these options)
    small = ["--width", "32", "--height", "16", "--spp", "1", "--mesh-n", "4"]
    for argv in (["--out", str(tmp_path / "x.exr"), "--exr-layers", "albedo,alpha", "--exr-float", "--exr-compression", "zips"],
                 ["--out", str(tmp_path / "x.png"), "--hdr", str(tmp_path / "h.exr"), "--exr-compression", "none"]):
        with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):  # past the parser: the first call that needs a device
            R.main(argv + small)
    assert not (tmp_path / "x.exr").exists() and not (tmp_path / "h.exr").exists()


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    """the addon built against tests/napi_mock and tests/exr_mock_stub.c, as tests/test_png_cpu.py does"""
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    import json
    d = str(tmp_path_factory.mktemp("exr_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "png_mock_stub.c"), os.path.join(ROOT, "tests", "exr_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "exr_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def mock_file(tag, a, compression=3, ptype=1, layers=0, chunk=0, feat=0):
    return [ord(tag), a, compression, ptype, layers, chunk >> 8, feat] + list(b"X")


def test_js_exr_calls_go_through_the_addon(js_report):
    r = js_report
    assert r["draw"] == mock_file("D", 3, 2, 2, 1 | 8, 512) and r["drawIsBuffer"]  # source temporalDenoised = 3
    assert r["drawDefault"] == mock_file("D", 0)
    assert r["grownDraw"] == mock_file("D", 1, layers=15) and r["grownBytes"] == 3000 + 3 * 2 * 44
    assert r["encode"] == mock_file("E", 5 * 2 + 1, 0, 1, 2, 1024, 1) and r["encodeIsBuffer"]
    assert r["encodePlain"] == mock_file("E", 5 * 2)


def test_js_exr_argument_checks(js_report):
    r = js_report
    assert r["badSource"] == "RangeError: drawExr: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'"
    assert r["badCompression"] == "RangeError: drawExr: compression must be 'none', 'zips' or 'zip'"
    assert r["badLayer"] == "RangeError: drawExr: layers must be among 'alpha', 'albedo', 'normal' and 'depth'"
    assert r["badChunk"] == "RangeError: drawExr: chunkBytes must be 0 or an integer in 256..32768"
    assert r["encodeShort"] == "RangeError: exrEncode: need a Float32Array of width*height*4 floats"
    assert r["encodeNoFeatures"] == "RangeError: exrEncode: the albedo, normal and depth layers need features, a Float32Array of width*height*8 floats"
    assert r["duringDraw"] is not None and r["after"] is None
