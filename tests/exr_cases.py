"""tests/exr_cases.py - the buffers and settings the OpenEXR tests encode (tests/test_exr_cpu.py, tests/test_exr_gpu.py):
radiance float32 [h, w, 4] and features float32 [h, w, 8] (albedo rgb, t, normal xyz, hit), both with row 0 wherever the
case's bottom_up puts it."""
import itertools

import numpy as np

import exr_ref as X


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


# the half conversion's edges, as float32 bit patterns: +-0; 2^-24, 2^-25 (a tie: to 0), the next float above it; 65504,
# 65520 (a tie: to infinity), the float below it; the largest and the smallest float32; float32 subnormals; the half normal /
# subnormal border and ties inside the subnormals; +-infinity; NaNs of both signs and several payloads
EDGE_BITS = [0x00000000, 0x80000000, 0x33800000, 0x33000000, 0x33000001, 0xB3000000, 0xB3000001, 0x477FE000, 0x477FF000, 0x477FEFFF, 0xC77FF000,
             0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x00000001, 0x007FFFFF, 0x80000001, 0x38800000, 0x387FFFFF, 0x387FE000, 0x387FF000,
             0x33C00000, 0x34400000, 0x34200000, 0x3F800000, 0x3F801000, 0x3F803000, 0x3F801001, 0xBF800FFF, 0x47800000,
             0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5, 0xFFC00001]
ALL_LAYERS = X.ALPHA | X.ALBEDO | X.NORMAL | X.DEPTH


def radiance(kind, w, h, seed=0):
    rng = np.random.default_rng([seed, w, h, ("rendered", "bits", "split", "edges", "constant").index(kind)])
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    if kind == "rendered":  # smooth shading with noise, values above 1, a fourth float of 1
        a = np.stack([0.4 + 0.3 * np.sin(x / 7.0 + y / 5.0), 0.2 + 0.01 * x, 3.0 * np.exp(-((x - w / 2) ** 2 + (y - h / 2) ** 2) / (1.0 + w * h / 8.0)), np.ones_like(x)], -1)
        a[..., :3] *= rng.uniform(0.7, 1.3, (h, w, 3))
        return a.astype(np.float32)
    if kind == "bits":  # every byte of every float random, the NaNs and infinities among them
        return rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    if kind == "split":  # file's upper half constant, lower half random bits: blocks that deflate well and blocks that fall back to raw
        a = np.full((h, w, 4), 0.25, np.float32)
        a[h // 2:] = rng.integers(0, 1 << 32, (h - h // 2, w, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
        return a
    if kind == "edges":  # the edge list in every channel, each channel at another phase
        e = _f32(EDGE_BITS)
        idx = (np.arange(h * w).reshape(h, w, 1) + np.array([0, 5, 11, 17])) % len(e)
        return e[idx]
    if kind == "constant":
        return np.full((h, w, 4), 0.5, np.float32)
    raise ValueError(kind)


def features(w, h, seed=0, edges=False):
    rng = np.random.default_rng([seed, w, h, 77])
    f = np.zeros((h, w, 8), np.float32)
    f[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3))
    f[..., 3] = np.where(rng.uniform(size=(h, w)) < 0.2, 1e5, rng.uniform(0.5, 9.0, (h, w)))  # a miss: 1e5, which no half holds
    n = rng.normal(size=(h, w, 3))
    f[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    f[..., 7] = rng.integers(0, 2, (h, w))
    if edges:
        e = _f32(EDGE_BITS)
        f = e[(np.arange(h * w * 8).reshape(h, w, 8) * 7) % len(e)]
    return f


# (kind, w, h, compression, pixel type, layers, chunk_bytes, bottom_up, with features) - the files the GPU has to reproduce
def cases():
    out = []
    for (w, h), comp, pt in itertools.product(((1, 1), (1, 17)), (X.NONE, X.ZIPS, X.ZIP), (X.HALF, X.FLOAT)):
        out.append(("bits" if pt == X.FLOAT else "rendered", w, h, comp, pt, X.ALPHA if w * h > 1 else 0, 256, bool(h & comp & 1), False))
    # ZIP with exactly one block, and with a last block of one line
    for (w, h), pt in itertools.product(((3, 16), (3, 33)), (X.HALF, X.FLOAT)):
        out.append(("rendered", w, h, X.ZIP, pt, X.DEPTH if pt == X.HALF else 0, 0, h == 33, pt == X.HALF))
    # a ZIP block longer than a chunk and no multiple of it: 301 * 6 * 16 = 28 896 bytes at 4 KiB, whose last block has two lines
    out.append(("rendered", 301, 18, X.ZIP, X.HALF, 0, 4096, True, False))
    # segments off 4-byte alignment: ZIPS lines of 301 * 6 = 1806 bytes (2 mod 4) in chunks of 1000, and ZIP chunks of an odd size
    out.append(("rendered", 301, 18, X.ZIPS, X.HALF, 0, 1000, False, False))
    out.append(("rendered", 301, 18, X.ZIP, X.HALF, X.ALPHA | X.DEPTH, 4099, False, True))
    out.append(("rendered", 301, 5, X.ZIPS, X.HALF, ALL_LAYERS, 4096, True, True))
    out.append(("rendered", 77, 19, X.NONE, X.HALF, ALL_LAYERS, 0, True, True))
    # every layer combination, HALF (with Z: mixed HALF + FLOAT rows) and FLOAT, compressions and row orders dealt round-robin
    for layers, pt in itertools.product(range(16), (X.HALF, X.FLOAT)):
        k = layers * 2 + pt
        out.append(("rendered", 5, 18, (X.ZIP, X.ZIPS, X.NONE)[k % 3], pt, layers, 256 if k % 2 else 0, bool(k & 2), bool(layers & X.GUIDED) or bool(k & 4)))
    # compressed and raw blocks in one file
    out.append(("split", 24, 64, X.ZIP, X.FLOAT, 0, 0, False, False))
    out.append(("split", 24, 6, X.ZIPS, X.FLOAT, X.ALPHA, 300, True, False))
    # block counts at, just past and two tiles past the offset scan's width of 256: its 64-bit carry from tile to tile
    for w, h in ((3, 256), (3, 257), (2, 513)):
        out.append(("rendered", w, h, X.ZIPS, X.HALF, 0, 256, False, False))
    out.append(("rendered", 50, 257, X.ZIPS, X.HALF, 0, 256, True, False))  # 300 bytes a line: two chunks a block, 514 chunks
    out.append(("rendered", 1, 4112, X.ZIP, X.HALF, 0, 256, False, False))  # 257 blocks of 16 lines
    out.append(("rendered", 2, 300, X.NONE, X.HALF, 0, 256, True, False))
    out.append(("rendered", 40, 300, X.ZIPS, X.HALF, 0, 256, False, False))  # 240 bytes a line: some deflate, some stay raw, on both sides of block 256
    # the edge values as pixels (tests/test_exr_cpu.py takes the first of them as CASES[-3]: they stay last)
    for pt, comp in ((X.HALF, X.ZIP), (X.FLOAT, X.ZIPS), (X.HALF, X.NONE)):
        out.append(("edges", len(EDGE_BITS), 3, comp, pt, ALL_LAYERS, 0, False, True))
    return out


def case_id(c):
    kind, w, h, comp, pt, layers, cb, up, feat = c
    return f"{kind}-{w}x{h}-{ {0: 'none', 2: 'zips', 3: 'zip'}[comp] }-{'half' if pt == 1 else 'float'}-l{layers}-c{cb}-{'up' if up else 'down'}{'-f' if feat else ''}".replace(" ", "")


def buffers(c):
    kind, w, h, _, _, _, _, _, feat = c
    return radiance(kind, w, h), (features(w, h, edges=kind == "edges") if feat else None)


_files = {}


def reference(c):
    """(the restatement's file, its stats) of a case, computed once"""
    if c not in _files:
        kind, w, h, comp, pt, layers, cb, up, _ = c
        rgba, feat = buffers(c)
        st = {}
        _files[c] = (X.encode(rgba, feat, up, comp, pt, layers, cb, st), st)
    return _files[c]
