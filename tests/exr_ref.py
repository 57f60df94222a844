"""tests/exr_ref.py - the OpenEXR encoder of DESIGN 8.21, twice and independently.

encode(): the writer restated in integers and numpy, the definition the GPU encoder (fspt_amd/csrc/fspt_exr.hip) has to
reproduce byte for byte.  Its deflate is tests/png_ref.py's chunk statement: a block's predicted bytes are one zlib stream
(78 01, the chunks of chunk_bytes from the block's first byte, the last one with BFINAL, the big-endian Adler-32).

read(): a strict reader written from the file's description alone; it shares no code with the writer, inflates with
Python's zlib and refuses whatever the description does not allow.

The file (little-endian): 76 2f 31 01, 02 00 00 00; the attributes channels, compression, dataWindow, displayWindow,
lineOrder, pixelAspectRatio, screenWindowCenter, screenWindowWidth as name\\0 type\\0 int32 size, value; 00; one uint64 per
block: its absolute offset; the blocks (1 scanline for none and ZIPS, 16 for ZIP): int32 y, int32 size, data.  A block's
uncompressed data: per scanline, per channel in file order, w values.  ZIP / ZIPS: even bytes first, odd bytes behind them,
each byte from the second on minus the byte before it plus 128, deflated; raw when that is not shorter."""
import struct
import zlib

import numpy as np

import png_ref as P

NONE, ZIPS, ZIP = 0, 2, 3
HALF, FLOAT = 1, 2
ALPHA, ALBEDO, NORMAL, DEPTH = 1, 2, 4, 8
GUIDED = ALBEDO | NORMAL | DEPTH
CHUNK_DEFAULT = 8192  # FSPT_EXR_CHUNK
# (name, layer bit or 0 = always, the float it is: 0..3 of rgba, 4 + k of the features (albedo rgb, t, normal xyz, hit), always FLOAT)
CHANNELS = [("A", ALPHA, 3, False), ("B", 0, 2, False), ("G", 0, 1, False), ("N.X", NORMAL, 8, False), ("N.Y", NORMAL, 9, False),
            ("N.Z", NORMAL, 10, False), ("R", 0, 0, False), ("Z", DEPTH, 7, True), ("albedo.B", ALBEDO, 6, False),
            ("albedo.G", ALBEDO, 5, False), ("albedo.R", ALBEDO, 4, False)]


# --------------------------------------------------------------------------------------------------------------------
# the writer
# --------------------------------------------------------------------------------------------------------------------
def half_bits(u):
    """float32 bit patterns (uint32) -> binary16 bit patterns (uint16): round to nearest even, overflow to infinity,
    subnormal results exact, every NaN 0x7E00.  Integers only."""
    u = np.asarray(u, np.uint32).astype(np.int64)
    s, a = (u >> 16) & 0x8000, u & 0x7FFFFFFF
    r = a - 0x38000000
    h, rem = r >> 13, r & 0x1FFF
    normal = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1)))
    e = a >> 23
    sh = np.clip(126 - e, 14, 24)
    m = (a & 0x7FFFFF) | 0x800000
    hs, rs, halfway = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
    sub = hs + ((rs > halfway) | ((rs == halfway) & ((hs & 1) == 1)))
    out = np.where(a > 0x7F800000, 0x7E00,
                   np.where(a >= 0x47800000, s | 0x7C00, np.where(a >= 0x38800000, s | normal, np.where(e < 102, s, s | sub))))
    return out.astype(np.uint16)


def float_bits(u):
    """float32 bit patterns as the file holds them: every NaN 0x7FC00000"""
    u = np.asarray(u, np.uint32)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint32(0x7FC00000), u).astype(np.uint32)


def channel_list(pixel_type=HALF, layers=0):
    """[(name, pixel type, source float)] in file order"""
    return [(n, FLOAT if always_float else pixel_type, src) for n, bit, src, always_float in CHANNELS if not bit or layers & bit]


def header(w, h, compression, chans):
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value

    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t, _ in chans) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (bytes([0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0]) + attr(b"channels", b"chlist", chlist) + attr(b"compression", b"compression", bytes([compression]))
            + attr(b"dataWindow", b"box2i", box) + attr(b"displayWindow", b"box2i", box) + attr(b"lineOrder", b"lineOrder", b"\0")
            + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
            + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def predict(raw):
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
    out = t.copy()
    out[1:] = (t[1:] - t[:-1] + 128) & 255
    return out.astype(np.uint8).tobytes()


def zlib_stream(data, cb, kinds=None):
    """one zlib stream of `data` in png_ref's chunks"""
    out = bytearray(P.ZLIB_HEADER)
    n_chunks = (len(data) + cb - 1) // cb
    for k in range(n_chunks):
        body, btype, _, _ = P.deflate_chunk(data[k * cb:(k + 1) * cb], k == n_chunks - 1)
        out += body
        if kinds is not None:
            kinds.append(btype)
    a, b = P.adler_pair(data)
    return bytes(out) + ((b << 16) | a).to_bytes(4, "big")


def resolve_chunk_bytes(chunk_bytes):
    if chunk_bytes == 0:
        return CHUNK_DEFAULT
    if not P.CHUNK_MIN <= chunk_bytes <= P.CHUNK_MAX:
        raise ValueError("chunk_bytes must be 0 or in 256..32768")
    return chunk_bytes


def planes(rgba, features, bottom_up, chans):
    """per channel its values as the file holds them, top-down: uint16 or uint32 [h, w]"""
    rgba = np.ascontiguousarray(rgba, np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError("need float32 [h, w, 4]")
    src = rgba.view(np.uint32)
    if any(s >= 4 for _, _, s in chans):
        f = np.ascontiguousarray(features, np.float32)
        if f.shape != rgba.shape[:2] + (8,):
            raise ValueError("need features float32 [h, w, 8]")
        src = np.concatenate([src, f.view(np.uint32)], axis=2)
    if bottom_up:
        src = src[::-1]
    return [half_bits(src[..., s]) if t == HALF else float_bits(src[..., s]) for _, t, s in chans]


def encode(rgba, features=None, bottom_up=False, compression=ZIP, pixel_type=HALF, layers=0, chunk_bytes=0, stats=None):
    """The file.  stats (a dict, or None) receives "raw" (per block: stored raw?), "kinds" (the BTYPE of every deflate
    chunk) and "blocks" (each block's uncompressed bytes)."""
    if compression not in (NONE, ZIPS, ZIP) or pixel_type not in (HALF, FLOAT) or layers & ~15:
        raise ValueError("unknown compression, pixel type or layer bit")
    cb = resolve_chunk_bytes(chunk_bytes)
    chans = channel_list(pixel_type, layers)
    pl = planes(rgba, features, bottom_up, chans)
    h, w = pl[0].shape
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError("width and height must be in 1..65535")
    lpb = 16 if compression == ZIP else 1
    hdr = header(w, h, compression, chans)
    st = {"raw": [], "kinds": [], "blocks": []}
    blocks = []
    for y0 in range(0, h, lpb):
        raw = b"".join(p[y].astype("<u2" if p.dtype == np.uint16 else "<u4").tobytes() for y in range(y0, min(y0 + lpb, h)) for p in pl)
        data = raw
        if compression != NONE:
            z = zlib_stream(predict(raw), cb, st["kinds"])
            if len(z) < len(raw):
                data = z
        st["raw"].append(data is raw)
        st["blocks"].append(raw)
        blocks.append(struct.pack("<ii", y0, len(data)) + data)
    out, at = bytearray(hdr), len(hdr) + 8 * len(blocks)
    for b in blocks:
        out += struct.pack("<Q", at)
        at += len(b)
    for b in blocks:
        out += b
    if stats is not None:
        stats.update(st)
    return bytes(out)


def bound(w, h, compression=ZIP, pixel_type=HALF, layers=0):
    """fspt_exr_bound: the header, per block a table entry and (y, size), and every block raw"""
    chans = channel_list(pixel_type, layers)
    lpb = 16 if compression == ZIP else 1
    return len(header(w, h, compression, chans)) + ((h + lpb - 1) // lpb) * 16 + w * h * sum(2 if t == HALF else 4 for _, t, _ in chans)


# --------------------------------------------------------------------------------------------------------------------
# the reader
# --------------------------------------------------------------------------------------------------------------------
class ExrError(ValueError):
    pass


REQUIRED = [("channels", "chlist", None), ("compression", "compression", 1), ("dataWindow", "box2i", 16), ("displayWindow", "box2i", 16),
            ("lineOrder", "lineOrder", 1), ("pixelAspectRatio", "float", 4), ("screenWindowCenter", "v2f", 8), ("screenWindowWidth", "float", 4)]
KNOWN_NAMES = ["A", "B", "G", "N.X", "N.Y", "N.Z", "R", "Z", "albedo.B", "albedo.G", "albedo.R"]


def _need(cond, what):
    if not cond:
        raise ExrError(what)


def _cstr(d, at):
    end = d.find(b"\0", at)
    _need(end >= 0, "unterminated string")
    return d[at:end].decode("ascii"), end + 1


def read(data):
    """-> {"w", "h", "compression", "channels": [(name, type)], "planes": {name: float16 / float32 [h, w], top-down},
    "sizes": [per block], "raw": [per block: stored raw?]}"""
    d = bytes(data)
    _need(d[:4] == b"\x76\x2f\x31\x01", "magic")
    _need(d[4:8] == b"\x02\x00\x00\x00", "version word")
    at, attrs = 8, []
    while True:
        _need(at < len(d), "header runs off the file")
        if d[at] == 0:
            at += 1
            break
        name, at = _cstr(d, at)
        kind, at = _cstr(d, at)
        (size,) = struct.unpack_from("<i", d, at)
        at += 4
        _need(size >= 0 and at + size <= len(d), "attribute size")
        attrs.append((name, kind, d[at:at + size]))
        at += size
    _need([a[0] for a in attrs] == [r[0] for r in REQUIRED], "attributes and their order: %r" % [a[0] for a in attrs])
    val = {}
    for (name, kind, value), (_, want_kind, want_size) in zip(attrs, REQUIRED):
        _need(kind == want_kind, "type of " + name)
        _need(want_size is None or len(value) == want_size, "size of " + name)
        val[name] = value
    chans, c, v = [], 0, val["channels"]
    while True:
        _need(c < len(v), "channel list runs off its attribute")
        if v[c] == 0:
            _need(c + 1 == len(v), "bytes behind the channel list")
            break
        name, c = _cstr(v, c)
        _need(c + 16 <= len(v), "channel entry")
        ptype, plinear, r0, r1, r2, xs, ys = struct.unpack_from("<iBBBBii", v, c)
        c += 16
        _need(ptype in (1, 2) and plinear == 0 and (r0, r1, r2) == (0, 0, 0) and xs == 1 and ys == 1, "channel entry of " + name)
        chans.append((name, ptype))
    names = [n for n, _ in chans]
    _need(names == sorted(names, key=lambda s: s.encode()) and len(set(names)) == len(names), "channel order")
    _need(all(n in KNOWN_NAMES for n in names) and all(n in names for n in "RGB"), "channel names")
    _need(all(t == 2 for n, t in chans if n == "Z"), "Z must be FLOAT")
    _need(len({t for n, t in chans if n != "Z"}) == 1, "one pixel type for all channels but Z")
    comp = val["compression"][0]
    _need(comp in (0, 2, 3), "compression")
    x0, y0, x1, y1 = struct.unpack("<4i", val["dataWindow"])
    _need((x0, y0) == (0, 0) and x1 >= 0 and y1 >= 0, "dataWindow")
    _need(val["displayWindow"] == val["dataWindow"], "displayWindow")
    _need(val["lineOrder"] == b"\0", "lineOrder")
    _need(struct.unpack("<f", val["pixelAspectRatio"]) == (1.0,), "pixelAspectRatio")
    _need(struct.unpack("<2f", val["screenWindowCenter"]) == (0.0, 0.0), "screenWindowCenter")
    _need(struct.unpack("<f", val["screenWindowWidth"]) == (1.0,), "screenWindowWidth")
    w, h = x1 + 1, y1 + 1
    per_block = 16 if comp == 3 else 1
    n_blocks = -(-h // per_block)
    _need(at + 8 * n_blocks <= len(d), "offset table")
    table = struct.unpack_from("<%dQ" % n_blocks, d, at)
    at += 8 * n_blocks
    widths = [2 if t == 1 else 4 for _, t in chans]
    line = w * sum(widths)
    rows = {n: np.zeros((h, w), np.float16 if t == 1 else np.float32) for n, t in chans}
    sizes, raws = [], []
    for k in range(n_blocks):
        _need(table[k] == at, "offset of block %d: %d, the blocks so far end at %d" % (k, table[k], at))
        _need(at + 8 <= len(d), "block header")
        y, size = struct.unpack_from("<ii", d, at)
        at += 8
        lines = min(per_block, h - k * per_block)
        n = lines * line
        _need(y == k * per_block, "y of block %d" % k)
        _need(0 < size <= n and at + size <= len(d), "size of block %d" % k)
        _need(comp != 0 or size == n, "an uncompressed block's size")
        body = d[at:at + size]
        at += size
        if size < n:
            t = zlib.decompress(body)
            _need(len(t) == n, "inflated length of block %d" % k)
            acc = np.cumsum(np.frombuffer(t, np.uint8).astype(np.int64) - 128) + 128  # t[i] = t'[i] + t[i-1] - 128, t[0] = t'[0]
            u = (acc & 255).astype(np.uint8)
            first = (n + 1) // 2
            raw = np.empty(n, np.uint8)
            raw[0::2] = u[:first]
            raw[1::2] = u[first:]
            body = raw.tobytes()
        sizes.append(size)
        raws.append(size == n)
        pos = 0
        for ln in range(lines):
            for (name, t), bw in zip(chans, widths):
                rows[name][k * per_block + ln] = np.frombuffer(body, "<f2" if t == 1 else "<f4", w, pos)
                pos += bw * w
    _need(at == len(d), "bytes behind the last block")
    return {"w": w, "h": h, "compression": comp, "channels": chans, "planes": rows, "sizes": sizes, "raw": raws}
