"""ID mattes without a GPU: fspt_matte_hash and fspt_exr_bound_mattes against tests/matte_ref.py, the
refusals that come before a device is touched, the restatement's own writer-to-reader round trip and the properties of
its rank rule."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import exr_ref as X
import matte_ref as M
import fspt_amd
from fspt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = [(b"", 0, 0x00000000), (b"hello", 0, 0x248BFA47), (b"CryptoObject", 0, 0x3AE39A58), (b"CryptoMaterial", 0, 0xBE359D67),
           (b"Hello, world!", 1234, 0xFAF6CDB3), (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD)]


def test_murmur_vectors_and_the_float_rule():
    for data, seed, want in VECTORS:
        assert M.murmur3_32(data, seed) == want
    assert M.float_rule(0x00000000) == 0x00800000 and M.float_rule(0x807FFFFF) == 0x80FFFFFF
    assert M.float_rule(0x7F800001) == 0x7F000001 and M.float_rule(0xFFFFFFFF) == 0xFF7FFFFF
    assert M.float_rule(0x3AE39A58) == 0x3AE39A58
    assert M.layer_key(M.OBJECT)[0][:7] == "3ae39a5" and M.layer_key(M.MATERIAL)[0][:7] == "be359d6"


def test_library_hash_is_the_restatements():
    lib = L.lib()
    for data, seed, want in VECTORS:
        if seed == 0:
            assert lib.fspt_matte_hash(data, len(data)) == M.float_rule(want)
    # names whose raw hash has exponent field 0 or 255, found by search: the float rule flips bit 23
    low, high = [], []
    for k in range(200000):
        e = (M.murmur3_32(b"name%d" % k) >> 23) & 255
        if e == 0 and len(low) < 3:
            low.append("name%d" % k)
        if e == 255 and len(high) < 3:
            high.append("name%d" % k)
        if len(low) == 3 and len(high) == 3:
            break
    assert len(low) == 3 and len(high) == 3
    for n in low + high:
        raw = M.murmur3_32(n.encode())
        assert fspt_amd.matte_hash(n) == raw ^ (1 << 23) == M.matte_hash(n)
        assert (fspt_amd.matte_hash(n) >> 23) & 255 in (1, 254)
    for n in ["", "a", "ab", "abc", "abcd", "abcde", "0:bunny.obj", "m0007", "été", "x" * 1000]:
        assert fspt_amd.matte_hash(n) == M.matte_hash(n)
    assert lib.fspt_matte_hash(None, 0) == M.matte_hash(b"")


def test_manifest():
    names = ["0:a.obj", "1:b \"q\".obj", "m0002"]
    want = b'{"0:a.obj":"%08x","1:b \\"q\\".obj":"%08x","m0002":"%08x"}' % tuple(M.matte_hash(n) for n in names)
    assert M.manifest(names) == want == fspt_amd.matte_manifest(names)
    assert M.manifest([]) == b"{}" == fspt_amd.matte_manifest([])


def mattes_struct(manifests):
    m = L.ExrMattes()
    for k, b in manifests.items():
        m.manifest[k], m.manifest_len[k] = b, len(b)
    return m


@pytest.mark.parametrize("layers", [16, 32, 48, 63, 15, 0, 16 | 8, 32 | 1])
def test_bound_is_the_restatements(layers):
    lib = L.lib()
    manifests = {M.OBJECT: M.manifest(["a", "b"]), M.MATERIAL: b"x" * 5000}
    for w, h in ((1, 1), (37, 21), (300, 17), (65535, 2)):
        for comp in (X.NONE, X.ZIPS, X.ZIP):
            for pt in (X.HALF, X.FLOAT):
                p, n = L.ExrParams(comp, pt, layers, 0), C.c_size_t()
                for man in ({}, manifests, {M.MATERIAL: manifests[M.MATERIAL]}):
                    m = mattes_struct(man)
                    assert lib.fspt_exr_bound_mattes(w, h, C.byref(p), C.byref(m), C.byref(n)) == 0
                    assert n.value == M.bound(w, h, comp, pt, layers, man)
                assert lib.fspt_exr_bound_mattes(w, h, C.byref(p), None, C.byref(n)) == 0 and n.value == M.bound(w, h, comp, pt, layers)
                if not layers & 48:
                    assert n.value == X.bound(w, h, comp, pt, layers)


def test_refusals_before_a_device():
    lib = L.lib()
    n = C.c_size_t(7)
    rgba, ranks = np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 12), np.float32)
    out = np.full(4096, 7, np.uint8)

    def bound(layers, m=None, w=3, h=2):
        p = L.ExrParams(3, 1, layers, 0)
        return lib.fspt_exr_bound_mattes(w, h, C.byref(p), None if m is None else C.byref(m), C.byref(n))

    assert bound(64) == -1 and b"unknown layer bits" in lib.fspt_last_error()
    assert bound(16, w=0) == -1
    p16 = L.ExrParams(3, 1, 16, 0)
    assert lib.fspt_exr_bound(3, 2, C.byref(p16), C.byref(n)) == -1 and b"unknown layer bits" in lib.fspt_last_error()  # as before
    assert lib.fspt_exr_bound_mattes(3, 2, C.byref(p16), None, None) == -1
    long = mattes_struct({M.OBJECT: b"x" * ((1 << 20) + 1)})
    assert bound(16, long) == -1
    assert bound(32, long) == 0  # (the kind is not in the file)
    assert bound(16, mattes_struct({M.OBJECT: b"x" * (1 << 20)})) == 0
    nul = L.ExrMattes()
    nul.manifest_len[0] = 5
    assert bound(16, nul) == -1
    # the encode entries: the old ones refuse the bits, the new ones want the ranks of the kinds asked for
    args = (L.fptr(rgba), None)
    tail = (3, 2, 1, C.byref(p16), L.u8ptr(out), out.size, C.byref(n))
    assert lib.fspt_exr_encode(0, *args, *tail) == -1 and b"unknown layer bits" in lib.fspt_last_error()
    assert lib.fspt_exr_encode_mattes(0, *args, None, *tail) == -1 and b"ranks" in lib.fspt_last_error()
    m = L.ExrMattes()
    m.ranks[1] = ranks.ctypes.data
    assert lib.fspt_exr_encode_mattes(0, *args, C.byref(m), *tail) == -1 and b"ranks" in lib.fspt_last_error()
    assert lib.fspt_exr_encode_mattes_device(0, *args, C.byref(m), *tail) == -1
    assert lib.fspt_exr_encode_mattes(0, None, None, C.byref(m), *tail) == -1
    assert (out == 7).all()
    # scene and target entries: NULL handles
    ids = np.zeros(4, np.uint32)
    assert lib.fspt_scene_set_matte_ids(None, 0, L.u32ptr(ids)) == -1
    assert lib.fspt_scene_set_matte_manifest(None, 0, b"{}", 2) == -1
    cam = L.CameraParams()
    assert lib.fspt_mattes(None, C.byref(cam), 1, 1) == -1
    assert lib.fspt_read_mattes(None, 0, L.fptr(ranks)) == -1
    lost = C.c_uint64()
    assert lib.fspt_mattes_lost(None, 0, C.byref(lost)) == -1
    with pytest.raises(ValueError):
        fspt_amd.tracer._matte_kind("asset")


def some_ranks(rng, h, w, names):
    """a plausible buffer: per pixel up to six distinct ids with counts out of 8"""
    hashes = np.array([M.matte_hash(n) for n in names], np.uint32)
    sid = hashes[rng.integers(0, len(names), (h, w, 8))]
    sid[rng.random((h, w, 8)) < 0.2] = 0
    ids, cov, _ = M.rank(sid)
    return M.pack(ids, cov), ids, cov


@pytest.mark.parametrize("comp", [X.NONE, X.ZIPS, X.ZIP])
@pytest.mark.parametrize("ptype", [X.HALF, X.FLOAT])
def test_restatement_round_trip(comp, ptype):
    rng = np.random.default_rng(5)
    h, w = 19, 23
    rgba = rng.random((h, w, 4)).astype(np.float32)
    feat = rng.random((h, w, 8)).astype(np.float32)
    names_o, names_m = ["o%d" % k for k in range(9)], ["m%04d" % k for k in range(4)]
    ro, io, co = some_ranks(rng, h, w, names_o)
    rm, im, cm = some_ranks(rng, h, w, names_m)
    man = {M.OBJECT: M.manifest(names_o)}
    for layers in (63, 16, 32 | 8, 48):
        for up in (False, True):
            f = M.encode(rgba, feat, {M.OBJECT: ro, M.MATERIAL: rm}, man, bottom_up=up, compression=comp, pixel_type=ptype, layers=layers)
            assert len(f) <= M.bound(w, h, comp, ptype, layers, man)
            r = M.read(f)
            names = [n for n, _ in r["channels"]]
            assert names == sorted(names, key=str.encode) and (r["w"], r["h"]) == (w, h)
            flip = (lambda a: a[::-1]) if up else (lambda a: a)
            assert sorted(r["mattes"]) == [k for k in (0, 1) if layers & (16 << k)]
            if layers & 16:
                assert np.array_equal(r["mattes"][0][0], flip(io)) and np.array_equal(r["mattes"][0][1], flip(co))
                assert r["manifests"][0] == man[0]
                assert names.index("B") < names.index("CryptoObject00.A") < names.index("CryptoObject02.R") < names.index("G")
            if layers & 32:
                assert np.array_equal(r["mattes"][1][0], flip(im)) and np.array_equal(r["mattes"][1][1], flip(cm))
                assert r["manifests"][1] is None
            if layers & 48 == 48:
                assert names.index("CryptoMaterial02.R") < names.index("CryptoObject00.A")
            want = np.float16(flip(rgba)[..., 0]) if ptype == X.HALF else flip(rgba)[..., 0]
            assert np.array_equal(r["planes"]["R"], want)
    # without a matte layer the file is exr_ref's
    assert M.encode(rgba, feat, compression=comp, pixel_type=ptype, layers=15) == X.encode(rgba, feat, compression=comp, pixel_type=ptype, layers=15)
    # and the strict reader refuses a tampered one
    f = bytearray(M.encode(rgba, feat, {M.OBJECT: ro}, man, compression=comp, pixel_type=ptype, layers=16))
    at = f.index(b"uint32_to_float32")
    f[at] ^= 1
    with pytest.raises(M.MatteExrError):
        M.read(bytes(f))


def test_rank_rule_properties():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n_ids, s = int(rng.integers(1, 12)), int(rng.integers(1, 65))
        pool = np.array([M.matte_hash("id%d" % k) for k in range(n_ids)], np.uint32)
        sid = pool[rng.integers(0, n_ids, s)]
        sid[rng.random(s) < 0.25] = 0
        ranked, lost, slots = M.rank_pixel(sid)
        assert sum(c for _, c in ranked) + lost == int((sid != 0).sum())  # counts plus lost = hits
        counts = [c for _, c in ranked]
        assert counts == sorted(counts, reverse=True)
        first_seen = [v for v, _ in slots]
        for a, b in zip(ranked, ranked[1:]):  # ties: first seen first
            if a[1] == b[1] and b[1] > 0:
                assert first_seen.index(a[0]) < first_seen.index(b[0])
        distinct = []
        for v in sid:
            if v and int(v) not in distinct:
                distinct.append(int(v))
        assert first_seen == distinct[:6]  # the first six distinct ids hold the slots, every other one is dropped
        assert lost == sum(int((sid == v).sum()) for v in distinct[6:])
        assert all(v == 0 and c == 0 for v, c in ranked[len(slots):])
    # a tie, and the full table, spelled out
    ranked, lost, _ = M.rank_pixel([5, 9, 9, 5, 0, 7])
    assert ranked[:3] == [(5, 2), (9, 2), (7, 1)] and lost == 0
    ranked, lost, _ = M.rank_pixel([1, 2, 3, 4, 5, 6, 7, 7, 8, 6])
    assert ranked[0] == (6, 2) and [v for v, _ in ranked[1:]] == [1, 2, 3, 4, 5] and lost == 3
    ids, cov, total = M.rank(np.array([[[3, 3, 0, 4]]], np.uint32))
    assert ids[0, 0].tolist() == [3, 4, 0, 0, 0, 0] and cov[0, 0].tolist() == [0.5, 0.25, 0, 0, 0, 0] and total == 0


# ---- the Node host on the mock library --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def js_report(tmp_path_factory):
    """the addon built against tests/napi_mock and tests/matte_mock_stub.c, as tests/test_exr_cpu.py does"""
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node or the Node headers are missing")
    d = str(tmp_path_factory.mktemp("matte_mock"))
    inc = os.path.join(ROOT, "include")
    mock = os.path.join(ROOT, "tests", "napi_mock")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I" + inc, "-o", os.path.join(d, "libfspt.so"),
                           os.path.join(mock, "libfspt_mock.c"), os.path.join(mock, "libfspt_mock_stubs.c"),
                           os.path.join(ROOT, "tests", "matte_mock_stub.c")])
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I/usr/include/node", "-I" + inc, "-DNODE_GYP_MODULE_NAME=fspt_napi",
                           "-o", os.path.join(d, "fspt_napi.node"), os.path.join(ROOT, "fspt_amd", "csrc", "fspt_napi.c"),
                           "-L" + d, "-lfspt", "-Wl,-rpath," + d])
    shutil.copy(os.path.join(ROOT, "fspt_amd", "js", "fspt.js"), d)  # (fspt.js loads ./fspt_napi.node: the mock's)
    out = os.path.join(d, "out.json")
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "matte_mock_check.js"), d, out], timeout=120)
    return json.load(open(out))


def test_js_host_on_the_mock(js_report):
    r = js_report
    names = ["", "hello", "CryptoObject", "CryptoMaterial", "0:a.obj", '1:b "q".obj', "\u00e9t\u00e9"]
    assert r["hashes"] == [M.matte_hash(n) for n in names]
    assert r["manifest"].encode() == M.manifest(names[4:]) == fspt_amd.matte_manifest(names[4:])
    assert r["noIds"] is not None  # the library's FSPT_E_STATE, thrown
    assert r["badKind"] == "RangeError: setMatte: kind must be 'object' or 'material'"
    assert r["badCount"] == "RangeError: setMatte: triLabel must hold 1 labels"
    assert r["badLabel"] == "RangeError: setMatte: label 1, 1 names"
    man_o, man_m = M.manifest(["a", "b"]), M.manifest(["m0000"])
    assert r["object"] == {"id": M.matte_hash("b"), "cov": 1.0, "samples": 4.0, "seed": 9.0, "manifestLen": len(man_o), "lengths": [36, 36]}
    assert r["material"] == {"id": 0, "manifestLen": len(man_m)}  # a negative label: no matte
    assert r["lost"] == [1000, 1001]
    assert r["badReadKind"] == "RangeError: readMattes: kind must be 'object' or 'material'"
    assert all(x is not None and "handle" in x for x in r["wrongHandle"])
    assert r["draw"] == [ord("D"), 0, 2, 1, 1 | 16 | 32, 0, 0, 0, 0, 0, 0, ord("X")]
    assert r["drawBufferBytes"] == 3000 + 3 * 2 * 140 + len(man_o) + len(man_m)  # the bound counts the scene's manifests
    assert r["badLayer"] == "RangeError: drawExr: layers must be among 'alpha', 'albedo', 'normal' and 'depth'"
    assert r["encode"] == [ord("M"), 5 * 2 + 1, 3, 1, 48, 1, 1, 9, 0, ord("{"), 0, ord("X")]
    assert r["encodeShortRanks"] == "RangeError: exrEncode: matte ranks must be a Float32Array of width*height*12 floats"
    assert r["droppedManifest"] is None
    assert r["during"] == ["Error: render in flight"] * 4 and r["after"] is None
