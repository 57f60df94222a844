"""The PNG encoder on a box without a GPU: the integer restatement tests/png_ref.py - the yardstick of
tests/test_png_gpu.py - against things that are not it: Pillow's and the Node host's decoders, zlib's inflate, crc32 and
adler32, an inverse filter written here; its size against zlib's own Z_RLE chunk by chunk; fspt_png_bound; the ABI's
argument checks and its refusal to compute without a device; the hosts' flags on the mock; the committed tables."""
import base64
import ctypes as C
import heapq
import io
import itertools
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

from fspt_amd import _lib as L

import png_ref as P
from png_cases import CONTENTS, FIBONACCI, FIBONACCI_CL, LARGE, RUNS, SMALL, image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def settings():
    """(content, w, h, channels, filter, chunk_bytes, bottom_up): every small size with every content, the channel counts,
    filters, chunk sizes and row orders dealt round-robin; then the large size"""
    k = 0
    for (w, h), content in itertools.product(SMALL, CONTENTS):
        yield content, w, h, 3 + (k & 1), (P.ADAPTIVE, 0, 1, P.ADAPTIVE, 2, 3, 4)[k % 7], (256, 1000, 0)[k % 3], bool((k // 2) & 1)
        k += 1
    for content in CONTENTS:
        yield content, LARGE[0], LARGE[1], 3, 0 if content == "runs" else P.ADAPTIVE, 32768, False
        yield content, LARGE[0], LARGE[1], 4, P.ADAPTIVE, (0, 8192, 5000)[k % 3], True
        k += 1
    yield ("fibonacci", FIBONACCI["w"], FIBONACCI["h"], 3, 0, 32768, False)
    yield ("fibonacci_cl", FIBONACCI_CL["w"], FIBONACCI_CL["h"], 3, 0, 32768, False)


@pytest.fixture(scope="module")
def encoded():
    """every case's file and statistics, made once"""
    out = []
    for content, w, h, ch, filt, cb, up in settings():
        a = image(content, w, h)
        st = {}
        out.append(((content, w, h, ch, filt, cb, up), a, P.encode(a, up, ch, filt, cb, st), st))
    return out


def unfilter(stream, w, h, ch):
    """the PNG specification's reconstruction, integers only -> [h, w, ch]"""
    row = 1 + w * ch
    out = np.zeros((h, w * ch), np.int32)
    for y in range(h):
        t, line = stream[y * row], stream[y * row + 1:(y + 1) * row]
        up = out[y - 1] if y else np.zeros(w * ch, np.int32)
        for i, v in enumerate(line):
            a = out[y, i - ch] if i >= ch else 0
            b = up[i]
            c = up[i - ch] if i >= ch else 0
            if t == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                pred = (0, a, b, (a + b) >> 1)[t]
            out[y, i] = (v + pred) & 255
    return out.reshape(h, w, ch).astype(np.uint8)


def chunks_of(data):
    """[(type, payload, crc)] of a PNG file behind its signature"""
    assert data[:8] == P.SIGNATURE
    out, i = [], 8
    while i < len(data):
        n = int.from_bytes(data[i:i + 4], "big")
        out.append((data[i + 4:i + 8], data[i + 8:i + 8 + n], int.from_bytes(data[i + 8 + n:i + 12 + n], "big")))
        i += 12 + n
    assert i == len(data)
    return out


def test_files_decode_to_the_input_and_their_parts_check(encoded):
    Image = pytest.importorskip("PIL.Image")
    for key, a, data, st in encoded:
        content, w, h, ch, filt, cb, up = key
        src = (a[::-1] if up else a)[..., :ch]
        im = Image.open(io.BytesIO(data))
        assert im.mode == ("RGB" if ch == 3 else "RGBA") and np.array_equal(np.asarray(im), src), key
        parts = chunks_of(data)
        assert [t for t, _, _ in parts] == [b"IHDR"] + [b"IDAT"] * (len(st["blocks"]) + 1) + [b"IEND"], key
        for t, payload, crc in parts:
            assert crc == zlib.crc32(t + payload), key
        idat = [p for t, p, _ in parts if t == b"IDAT"]
        assert idat == st["idat"] and (idat[0][0] * 256 + idat[0][1]) % 31 == 0
        stream = zlib.decompress(b"".join(idat))
        assert stream == st["stream"] and len(stream) == h * (1 + w * ch), key
        assert idat[-1] == zlib.adler32(stream).to_bytes(4, "big"), key
        if filt != P.ADAPTIVE:
            assert set(st["filters"]) == {filt}, key
        if w * h <= 1024 or content in ("rendered", "gradient"):  # (the inverse here is a Python loop per byte)
            assert np.array_equal(unfilter(stream, w, h, ch), src), key
        assert len(data) <= P.bound(w, h, ch, cb), key


def test_statistics_cover_the_format(encoded):
    """both block types, a match of 258, Up on equal rows, and the adaptive rule choosing more than one filter"""
    blocks, chosen, longest = set(), set(), 0
    for key, a, data, st in encoded:
        blocks |= set(st["blocks"])
        if key[4] == P.ADAPTIVE:
            chosen |= set(st["filters"])
        if key[0] == "rows_equal" and key[4] == P.ADAPTIVE and key[3] == 3:  # (alpha is random: RGB rows only)
            assert set(st["filters"][1:]) == {2}, key
        cb = P.resolve_chunk_bytes(key[5])
        for k in range(0, len(st["stream"]), cb):
            longest = max([longest] + [n for kind, n in P.tokens(st["stream"][k:k + cb]) if kind == "len"])
    assert blocks == {P.STORED, P.DYNAMIC} and longest == 258 and 2 in chosen and len(chosen) > 1


def depth_unlimited(freq):
    """the longest code of Huffman's tree without a limit (a heap, not the restatement's merge)"""
    heap = [(f, s, 0) for s, f in enumerate(freq) if f]
    heapq.heapify(heap)
    k = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return heap[0][2]


def test_both_code_limits_are_actually_hit(encoded):
    by = {key[0]: st for key, _, _, st in encoded}
    for content, limit, stat in (("fibonacci", 15, "max_len"), ("fibonacci_cl", 7, "max_cl_len")):
        st = by[content]
        assert st["blocks"] == [P.DYNAMIC] and st[stat] == [limit]
        freq = [0] * 286
        for kind, v in P.tokens(st["stream"]):
            freq[v if kind == "lit" else P.len_symbol(v)[0]] += 1
        freq[256] = 1
        if content == "fibonacci_cl":
            ll = P.code_lengths(freq, 15)
            assert max(ll) == depth_unlimited(freq) == 12  # (the literal/length code itself is not limited here)
            hlit = max(s for s in range(286) if ll[s]) + 1
            freq = [0] * 19
            for s, _, _ in P.rle_lengths(ll[:hlit] + [1]):
                freq[s] += 1
            assert not freq[16]
        assert depth_unlimited(freq) > limit, content


def test_code_lengths_are_a_prefix_code():
    """Kraft's sum is exactly one for two or more symbols, whatever the histogram, and the limit holds"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(2, 287))
        freq = [0] * 286
        for s in rng.choice(286, n, replace=False):
            freq[s] = int(rng.integers(1, 4)) if trial & 1 else int(2 ** rng.uniform(0, 15))
        for max_bits, syms in ((15, 286), (7, 19)):
            f = freq[:syms]
            lens = P.code_lengths(f, max_bits)
            used = [v for v in lens if v]
            if len(used) < 2:
                continue
            assert max(used) <= max_bits and sum(2 ** (max_bits - v) for v in used) == 2 ** max_bits
            assert all((v > 0) == (c > 0) for v, c in zip(lens, f))
            order = sorted((c, s) for s, c in enumerate(f) if c)
            assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(order, order[1:]))  # never a longer code for a more frequent symbol


def test_runs_tokens_are_closed_form():
    for r in RUNS + (259 + 258, 3 * 258 + 1, 3 * 258 + 3):
        toks = P.tokens(bytes([7]) * r + bytes([8]))
        assert toks[0] == ("lit", 7) and toks[-1] == ("lit", 8)
        assert 1 + sum(n if kind == "len" else 1 for kind, n in toks[1:-1]) == r
        lens = [n for kind, n in toks if kind == "len"]
        assert all(3 <= n <= 258 for n in lens) and lens[:-1] == [258] * (len(lens) - 1)
        assert sum(1 for kind, _ in toks[1:-1] if kind == "lit") <= 2


def z_rle(stream, cb):
    """zlib's own Z_RLE strategy (level 6, raw deflate), chunk by chunk"""
    total = 0
    for k in range(0, len(stream), cb):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += len(co.compress(stream[k:k + cb]) + co.flush())
    return total


def test_size_against_zlib_rle_and_constant_colour(encoded):
    """The size condition: on `rendered` and `gradient` at (256, 144) the IDAT payload - zlib header, empty stored blocks and
    Adler-32 included - is not larger than zlib's Z_RLE on the same chunks (measured here, chunks of 32 KiB: rendered 69 504
    against 69 614, gradient 17 023 against 17 051: no margin is needed).  A constant colour: under 1 % of the raw size
    (545 bytes against 110 592)."""
    seen = 0
    for key, a, data, st in encoded:
        if key[1:3] == LARGE and key[3] == 3 and key[0] in ("rendered", "gradient"):
            mine, ref = sum(map(len, st["idat"])), z_rle(st["stream"], 32768)
            print(key[0], "idat", mine, "zlib Z_RLE", ref)
            assert mine <= ref, key
            seen += 1
        if key[1:3] == LARGE and key[3] == 3 and key[0] == "constant":
            print("constant", len(data), "of", LARGE[0] * LARGE[1] * 3)
            assert len(data) * 100 < LARGE[0] * LARGE[1] * 3
            seen += 1
    assert seen == 3


def bound(w, h, p):
    n = C.c_size_t()
    assert L.lib().fspt_png_bound(w, h, None if p is None else C.byref(p), C.byref(n)) == 0
    return n.value


def test_bound_holds_and_noise_comes_close(encoded):
    for key, a, data, st in encoded:
        content, w, h, ch, filt, cb, up = key
        assert bound(w, h, L.PngParams(ch, filt, cb)) == P.bound(w, h, ch, cb) >= len(data), key
    w, h = LARGE
    for cb in (256, 1000, 32768):
        st = {}
        data = P.encode(image("noise", w, h), False, 4, P.ADAPTIVE, cb, st)
        assert set(st["blocks"]) == {P.STORED}
        assert 0 <= P.bound(w, h, 4, cb) - len(data) == 5 * len(st["blocks"])  # a stored chunk has no empty block behind it
    assert bound(64, 80, None) == bound(64, 80, L.PngParams(3, 5, 0)) == bound(64, 80, L.PngParams(0, 5, P.CHUNK_DEFAULT))
    assert bound(65535, 65535, L.PngParams(4, 5, 256)) == P.bound(65535, 65535, 4, 256) > 2 ** 32  # size_t arithmetic
    assert f"#define FSPT_PNG_CHUNK {P.CHUNK_DEFAULT}u" in open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()


DEVICE_ENTRIES = ("fspt_png_encode", "fspt_png_encode_device")


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fspt.h")).read() + open(os.path.join(ROOT, "include", "fspt_tuning.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("fspt_png_bound", "fspt_png_encode", "fspt_png_encode_device", "fspt_draw_png", "fspt_png_filtered_eval", "fspt_png_last_ms"):
        assert f"int {name}(" in text and hasattr(lib, name) and name in L.SIGNATURES, name
    assert "FSPT_PNG_FILTER_ADAPTIVE = 5" in text and "uint32_t channels, filter, chunk_bytes;" in text


def test_invalid_arguments_are_refused_before_a_device_is_touched():
    lib = L.lib()
    a = image("noise", 8, 8)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    ok = L.PngParams(3, 5, 0)
    bad_params = (L.PngParams(1, 5, 0), L.PngParams(5, 5, 0), L.PngParams(3, 6, 0), L.PngParams(3, 5, 255), L.PngParams(3, 5, 32769))

    def refused(name, rc):
        assert rc == -1 and name.encode() in lib.fspt_last_error(), (name, rc, lib.fspt_last_error())
        assert n.value == 77 and (out == 5).all()
    for name in DEVICE_ENTRIES:
        fn = getattr(lib, name)
        src = L.u8ptr(a) if name == "fspt_png_encode" else C.c_void_p(a.ctypes.data)
        refused(name, fn(0, None, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        refused(name, fn(0, src, 8, 8, 0, C.byref(ok), None, out.size, C.byref(n)))
        refused(name, fn(0, src, 8, 8, 0, C.byref(ok), L.u8ptr(out), out.size, None))
        for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
            refused(name, fn(0, src, w, h, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))
        for bad in bad_params:
            refused(name, fn(0, src, 8, 8, 0, C.byref(bad), L.u8ptr(out), out.size, C.byref(n)))
        refused(name, fn(0, src, 65535, 65535, 0, C.byref(ok), L.u8ptr(out), out.size, C.byref(n)))  # a file that could pass 4 GiB
    refused("fspt_png_filtered_eval", lib.fspt_png_filtered_eval(0, L.u8ptr(a), 8, 8, 0, C.byref(ok), None))
    refused("fspt_png_filtered_eval", lib.fspt_png_filtered_eval(0, L.u8ptr(a), 8, 8, 0, C.byref(bad_params[0]), L.u8ptr(out)))
    b = C.c_size_t(77)
    assert lib.fspt_png_bound(8, 8, C.byref(ok), None) == -1 and b"fspt_png_bound" in lib.fspt_last_error()
    for w, h, p in [(0, 8, ok), (8, 65536, ok)] + [(8, 8, p) for p in bad_params]:
        assert lib.fspt_png_bound(w, h, C.byref(p), C.byref(b)) == -1 and b"fspt_png_bound" in lib.fspt_last_error() and b.value == 77
    refused("fspt_draw_png", lib.fspt_draw_png(None, 0, 1.0, 1.0, 0, 3.0, 1.0, None, L.u8ptr(out), out.size, C.byref(n)))
    assert lib.fspt_png_last_ms(None, None) == -1


def test_no_device_no_encode():
    import fspt_amd
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        return  # (tests/test_png_gpu.py has the device's side)
    a = image("noise", 8, 8)
    out, n = np.full(4096, 5, np.uint8), C.c_size_t(77)
    for name in DEVICE_ENTRIES:
        src = L.u8ptr(a) if name == "fspt_png_encode" else C.c_void_p(a.ctypes.data)
        assert getattr(lib, name)(0, src, 8, 8, 0, None, L.u8ptr(out), out.size, C.byref(n)) == -2
        assert name.encode() in lib.fspt_last_error() and b"no CPU fallback" in lib.fspt_last_error()
        assert n.value == 77 and (out == 5).all()
    assert lib.fspt_png_filtered_eval(0, L.u8ptr(a), 8, 8, 0, None, L.u8ptr(out)) == -2
    assert b"no CPU fallback" in lib.fspt_last_error() and (out == 5).all()
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        fspt_amd.png_encode(a)
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        fspt_amd.png_filtered_eval(a)


def test_wrapper_argument_checks(tmp_path):
    import fspt_amd
    from fspt_amd.scene_file import write_image
    with pytest.raises(ValueError):
        fspt_amd.png_encode(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        fspt_amd.png_encode(np.zeros((8, 8, 4), np.uint8), channels=2)
    with pytest.raises(ValueError):
        fspt_amd.png_encode(np.zeros((8, 8, 4), np.uint8), filter="best")
    assert fspt_amd.png_bound(64, 80) == P.bound(64, 80) and fspt_amd.png_bound(64, 80, 4, "up", 256) == P.bound(64, 80, 4, 256)
    a = image("gradient", 9, 5)
    with pytest.raises(ValueError):
        write_image(str(tmp_path / "x.png"), a, png="host")
    write_image(str(tmp_path / "y.png"), a)  # the default stays Pillow on the host
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "y.png"))), a[..., :3])
    if L.lib().fspt_device_count() <= 0:
        for png in ("gpu", {"channels": 4}):
            with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
                write_image(str(tmp_path / "z.png"), a, png=png)
        assert not (tmp_path / "z.png").exists()


def test_render_cli_takes_png_gpu(tmp_path):
    """--png-gpu is parsed, needs a .png, and without a device the render is refused with the usual message"""
    import fspt_amd
    from fspt_amd import render as R
    with pytest.raises(SystemExit):
        R.main(["--out", "x.jpg", "--png-gpu"])
    if L.lib().fspt_device_count() > 0:
        return
    out = tmp_path / "x.png"
    with pytest.raises(fspt_amd.FsptError, match="no CPU fallback"):
        R.main(["--out", str(out), "--png-gpu", "--width", "32", "--height", "16", "--spp", "1", "--mesh-n", "4"])
    assert not out.exists()


def test_node_decoder_reads_the_restatements_files(tmp_path):
    """fspt_amd/js/scene_file.js decodePng - Node's zlib - reads them to exactly the input"""
    from test_node_host import ADDON, dec, run_node
    if shutil.which("node") is None or not os.path.exists(ADDON):
        pytest.skip("node or the built addon is missing")
    files = {}
    cases = [("rendered", 19, 37, 3, P.ADAPTIVE, 256, False), ("noise", 17, 9, 4, P.ADAPTIVE, 0, True), ("runs", 300, 1, 3, 0, 256, False),
             ("constant", 1, 1, 4, 4, 0, False), ("gradient", 85, 3, 4, 3, 1000, True), ("fibonacci", FIBONACCI["w"], FIBONACCI["h"], 3, 0, 32768, False)]
    for k, (content, w, h, ch, filt, cb, up) in enumerate(cases):
        a = image(content, w, h)
        f = str(tmp_path / f"{k}.png")
        open(f, "wb").write(P.encode(a, up, ch, filt, cb))
        want = (a[::-1] if up else a).copy()
        if ch == 3:
            want[..., 3] = 255
        files[f] = want
    px = np.zeros((1, 1, 4), np.uint8)
    out = run_node("png", {"files": sorted(files), "encode": {"rgba_b64": base64.b64encode(px.tobytes()).decode(), "width": 1, "height": 1,
                                                              "out4": str(tmp_path / "o4.png"), "out3": str(tmp_path / "o3.png")}})
    for f, want in files.items():
        d = out["decoded"][f]
        assert (d["height"], d["width"]) == want.shape[:2], f
        assert np.array_equal(dec(d["rgba"], np.uint8).reshape(want.shape), want), os.path.basename(f)


@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    """the addon built against tests/napi_mock and tests/png_mock_stub.c, as tests/test_jpeg_cpu.py does"""
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    import json
    d = str(tmp_path_factory.mktemp("png_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "png_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "png_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def mock_file(tag, a, channels=3, filt=5, chunk=0):
    return [ord(tag), a, channels, filt, chunk >> 8] + list(b"IEN")


def test_js_png_calls_go_through_the_addon(js_report):
    r = js_report
    assert r["draw"] == mock_file("D", 3, 4, 4, 512) and r["drawIsBuffer"]      # source temporalDenoised = 3
    assert r["drawDefault"] == mock_file("D", 0) and r["bufferBytes"] == 3 * 2 * 4 + 1024
    assert r["grownDraw"] == mock_file("D", 1) and r["grownBytes"] == 2000 + 3 * 2
    assert r["encode"] == mock_file("E", 5 * 2 + 1, 3, 2, 1024) and r["encodeIsBuffer"]
    assert r["filtered"] == [4 * 16 + 1] * (3 * (1 + 2 * 4))


def test_js_png_argument_checks(js_report):
    r = js_report
    assert r["badSource"] == "RangeError: drawPng: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'"
    assert r["badChannels"] == "RangeError: drawPng: channels must be 3 or 4"
    assert r["badFilter"] == "RangeError: drawPng: filter must be 'none', 'sub', 'up', 'average', 'paeth' or 'adaptive'"
    assert r["badChunk"] == "RangeError: drawPng: chunkBytes must be 0 or an integer in 256..32768"
    assert r["encodeShort"] == "RangeError: pngEncode: need a Uint8Array of width*height*4 bytes"
    assert r["encodeBadFilter"] == "RangeError: pngEncode: filter must be 'none', 'sub', 'up', 'average', 'paeth' or 'adaptive'"
    assert r["duringDraw"] == "Error: render in flight" and r["after"] is None


def test_committed_tables_are_the_generators():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_png_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_png_tables as T
    assert T.crc_table() == P.CRC_TABLE and T.CL_ORDER == P.CL_ORDER
    for n, e in zip(range(3, 259), T.length_codes()):
        sym, bits, base = P.len_symbol(n)
        assert (e & 0xFFF, (e >> 12) & 15, e >> 16) == (sym, bits, n - base)
    data = bytes(range(256)) * 3
    for cut in (0, 1, 255, 700, len(data)):  # the powers move a checksum past what follows
        assert T.shift(zlib.crc32(data[:cut]), len(data) - cut) ^ zlib.crc32(data[cut:]) == zlib.crc32(data)
    assert f"PNG_CRC_IDAT = 0x{zlib.crc32(b'IDAT'):08X}u" in T.text()
