"""tests/matte_ref.py - the ID mattes of DESIGN 8.25, stated in Python: what fspt_matte_hash, fspt_mattes and the OpenEXR
encoder's Cryptomatte layers have to reproduce bit for bit.

murmur3_32 / matte_hash / manifest: the ids and their names.  rank: the per-pixel rule, from a list of per-sample ids.
encode / bound: exr_ref's writer with the matte channels and the cryptomatte/ header attributes, built from exr_ref's
pieces.  read: a strict reader of such files, written from the description alone; it inflates with Python's zlib and
refuses whatever the description does not allow (exr_ref.read refuses the new names, so this one stands beside it).

The file is exr_ref's with, per kind present, twelve FLOAT channels Crypto<Object|Material>0<0|1|2>.<R|G|B|A> - R G B A of
level j = id(2j), coverage(2j), id(2j + 1), coverage(2j + 1) - in the byte order of all channel names, and directly behind
`compression` the string attributes cryptomatte/<key>/conversion = uint32_to_float32, /hash = MurmurHash3_32, /manifest
(when there is one), /name, in the byte order of their names; <key> = the first seven hex digits of matte_hash(name)."""
import json
import struct
import zlib

import numpy as np

import exr_ref as E

OBJECT, MATERIAL = 0, 1
RANKS = 6
CRYPTO_OBJECT, CRYPTO_MATERIAL = 16, 32
LAYER_NAMES = {OBJECT: "CryptoObject", MATERIAL: "CryptoMaterial"}
LAYER_BITS = {OBJECT: CRYPTO_OBJECT, MATERIAL: CRYPTO_MATERIAL}
MANIFEST_MAX = 1 << 20
M32 = 0xFFFFFFFF


# --------------------------------------------------------------------------------------------------------------------
# ids
# --------------------------------------------------------------------------------------------------------------------
def murmur3_32(data, seed=0):
    """MurmurHash3_x86_32 of bytes"""
    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & M32

    data = bytes(data)
    h, n = seed & M32, len(data)
    for i in range(0, n - n % 4, 4):
        k = struct.unpack_from("<I", data, i)[0]
        k = (k * 0xCC9E2D51) & M32
        k = rotl(k, 15)
        k = (k * 0x1B873593) & M32
        h ^= k
        h = rotl(h, 13)
        h = (h * 5 + 0xE6546B64) & M32
    tail, k = data[n - n % 4:], 0
    for j in reversed(range(len(tail))):
        k ^= tail[j] << (8 * j)
    if tail:
        k = (k * 0xCC9E2D51) & M32
        k = rotl(k, 15)
        k = (k * 0x1B873593) & M32
        h ^= k
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def float_rule(h):
    """Cryptomatte's: the id is read as a float32, so its exponent field is neither 0 (zero, subnormal) nor 255 (inf, NaN)"""
    return h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h


def matte_hash(name):
    return float_rule(murmur3_32(name if isinstance(name, bytes) else str(name).encode("utf-8")))


def manifest(names):
    """{"name":"%08x", ...} in the order given"""
    return ("{" + ",".join('%s:"%08x"' % (json.dumps(str(n)), matte_hash(n)) for n in names) + "}").encode("utf-8")


def layer_key(kind):
    return "%08x" % matte_hash(LAYER_NAMES[kind]), LAYER_NAMES[kind]


# --------------------------------------------------------------------------------------------------------------------
# the rank rule
# --------------------------------------------------------------------------------------------------------------------
def rank_pixel(sample_ids):
    """One pixel, its samples' ids in sample order (0: a miss or no matte) -> ([(id, count)] x 6 by rank, lost, the table
    in slot order).  A slot that holds the id counts it; else the lowest empty slot takes it; else the sample is lost.
    Ranks: count descending, ties by slot ascending."""
    slots, lost = [], 0
    for v in sample_ids:
        v = int(v)
        if v == 0:
            continue
        for s in slots:
            if s[0] == v:
                s[1] += 1
                break
        else:
            if len(slots) < RANKS:
                slots.append([v, 1])
            else:
                lost += 1
    order = sorted(range(len(slots)), key=lambda k: (-slots[k][1], k))
    ranked = [tuple(slots[k]) for k in order] + [(0, 0)] * (RANKS - len(slots))
    return ranked, lost, [tuple(s) for s in slots]


def rank(sample_ids):
    """sample_ids uint32 [H, W, S] -> (ids uint32 [H, W, 6], coverage float32 [H, W, 6], lost samples in all); the coverage is
    one IEEE division float32(count) / float32(S)"""
    a = np.asarray(sample_ids, np.uint32)
    H, W, S = a.shape
    ids, cnt, lost = np.zeros((H, W, RANKS), np.uint32), np.zeros((H, W, RANKS), np.float32), 0
    for y in range(H):
        for x in range(W):
            r, n, _ = rank_pixel(a[y, x])
            ids[y, x] = [v for v, _ in r]
            cnt[y, x] = [c for _, c in r]
            lost += n
    return ids, (cnt / np.float32(S)).astype(np.float32), lost


def pack(ids, cov):
    """(ids, coverage) [H, W, 6] -> float32 [H, W, 12]: id0 c0 .. id5 c5, the ids' bits as floats (fspt_read_mattes' buffer)"""
    out = np.zeros(ids.shape[:2] + (12,), np.uint32)
    out[..., 0::2] = np.asarray(ids, np.uint32)
    out[..., 1::2] = np.ascontiguousarray(cov, np.float32).view(np.uint32)
    return out.view(np.float32)


# --------------------------------------------------------------------------------------------------------------------
# the writer
# --------------------------------------------------------------------------------------------------------------------
def channel_list(pixel_type=E.HALF, layers=0):
    """[(name, pixel type, source float)] in file order: exr_ref's, and for a kind's bit its twelve FLOAT channels; source 12 +
    f / 24 + f = float f of the object / material ranks"""
    chans = list(E.channel_list(pixel_type, layers & 15))
    for kind, base in ((OBJECT, 12), (MATERIAL, 24)):
        if layers & LAYER_BITS[kind]:
            for j in range(3):
                for k, c in enumerate("RGBA"):
                    chans.append(("%s%02d.%s" % (LAYER_NAMES[kind], j, c), E.FLOAT, base + 4 * j + k))
    return sorted(chans, key=lambda c: c[0].encode())


def _attr(name, kind, value):
    return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value


def header(w, h, compression, chans, layers, manifests):
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t, _ in chans) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    meta = []
    for kind in (OBJECT, MATERIAL):
        if not layers & LAYER_BITS[kind]:
            continue
        key, name = layer_key(kind)
        items = {"conversion": b"uint32_to_float32", "hash": b"MurmurHash3_32", "name": name.encode()}
        if manifests.get(kind):
            items["manifest"] = bytes(manifests[kind])
        meta += [(("cryptomatte/%s/%s" % (key[:7], k)).encode(), v) for k, v in items.items()]
    meta.sort(key=lambda kv: kv[0])
    return (bytes([0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0]) + _attr(b"channels", b"chlist", chlist) + _attr(b"compression", b"compression", bytes([compression]))
            + b"".join(_attr(k, b"string", v) for k, v in meta)
            + _attr(b"dataWindow", b"box2i", box) + _attr(b"displayWindow", b"box2i", box) + _attr(b"lineOrder", b"lineOrder", b"\0")
            + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + _attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def _check(compression, pixel_type, layers, manifests):
    if compression not in (E.NONE, E.ZIPS, E.ZIP) or pixel_type not in (E.HALF, E.FLOAT) or layers & ~63:
        raise ValueError("unknown compression, pixel type or layer bit")
    if any(len(m or b"") > MANIFEST_MAX for m in manifests.values()):
        raise ValueError("a manifest holds at most 2^20 bytes")


def planes(rgba, features, ranks, bottom_up, chans):
    """per channel its values as the file holds them, top-down: uint16 or uint32 [h, w]; ranks: {kind: float32 [h, w, 12]}"""
    rgba = np.ascontiguousarray(rgba, np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError("need float32 [h, w, 4]")
    src = np.zeros(rgba.shape[:2] + (36,), np.uint32)
    src[..., :4] = rgba.view(np.uint32)
    need = {s for _, _, s in chans}
    if any(4 <= s < 12 for s in need):
        f = np.ascontiguousarray(features, np.float32)
        if f.shape != rgba.shape[:2] + (8,):
            raise ValueError("need features float32 [h, w, 8]")
        src[..., 4:12] = f.view(np.uint32)
    for kind, base in ((OBJECT, 12), (MATERIAL, 24)):
        if any(base <= s < base + 12 for s in need):
            r = np.ascontiguousarray(ranks[kind], np.float32)
            if r.shape != rgba.shape[:2] + (12,):
                raise ValueError("need ranks float32 [h, w, 12]")
            src[..., base:base + 12] = r.view(np.uint32)
    if bottom_up:
        src = src[::-1]
    return [E.half_bits(src[..., s]) if t == E.HALF else E.float_bits(src[..., s]) for _, t, s in chans]


def encode(rgba, features=None, ranks=None, manifests=None, bottom_up=False, compression=E.ZIP, pixel_type=E.HALF, layers=0, chunk_bytes=0):
    """The file.  ranks / manifests: {OBJECT / MATERIAL: float32 [h, w, 12] / bytes}"""
    manifests = manifests or {}
    _check(compression, pixel_type, layers, manifests)
    cb = E.resolve_chunk_bytes(chunk_bytes)
    chans = channel_list(pixel_type, layers)
    pl = planes(rgba, features, ranks or {}, bottom_up, chans)
    h, w = pl[0].shape
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError("width and height must be in 1..65535")
    lpb = 16 if compression == E.ZIP else 1
    hdr = header(w, h, compression, chans, layers, manifests)
    blocks = []
    for y0 in range(0, h, lpb):
        raw = b"".join(p[y].astype("<u2" if p.dtype == np.uint16 else "<u4").tobytes() for y in range(y0, min(y0 + lpb, h)) for p in pl)
        data = raw
        if compression != E.NONE:
            z = E.zlib_stream(E.predict(raw), cb)
            if len(z) < len(raw):
                data = z
        blocks.append(struct.pack("<ii", y0, len(data)) + data)
    out, at = bytearray(hdr), len(hdr) + 8 * len(blocks)
    for b in blocks:
        out += struct.pack("<Q", at)
        at += len(b)
    for b in blocks:
        out += b
    return bytes(out)


def bound(w, h, compression=E.ZIP, pixel_type=E.HALF, layers=0, manifests=None):
    """fspt_exr_bound_mattes: the header, per block a table entry and (y, size), and every block raw"""
    manifests = manifests or {}
    _check(compression, pixel_type, layers, manifests)
    chans = channel_list(pixel_type, layers)
    lpb = 16 if compression == E.ZIP else 1
    return len(header(w, h, compression, chans, layers, manifests)) + ((h + lpb - 1) // lpb) * 16 + w * h * sum(2 if t == E.HALF else 4 for _, t, _ in chans)


# --------------------------------------------------------------------------------------------------------------------
# the reader
# --------------------------------------------------------------------------------------------------------------------
class MatteExrError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise MatteExrError(what)


def _cstr(d, at):
    end = d.find(b"\0", at)
    _need(end >= 0, "unterminated string")
    return d[at:end].decode("ascii"), end + 1


HEAD = [("channels", "chlist", None), ("compression", "compression", 1)]
TAIL = [("dataWindow", "box2i", 16), ("displayWindow", "box2i", 16), ("lineOrder", "lineOrder", 1), ("pixelAspectRatio", "float", 4),
        ("screenWindowCenter", "v2f", 8), ("screenWindowWidth", "float", 4)]


def read(data):
    """-> {"w", "h", "compression", "channels": [(name, type)], "planes": {name: float16 / float32 [h, w], top-down},
    "mattes": {kind: (ids uint32 [h, w, 6], coverage float32 [h, w, 6])}, top-down, "manifests": {kind: bytes or None}}"""
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
        _need(at + 4 <= len(d), "attribute size word")
        (size,) = struct.unpack_from("<i", d, at)
        at += 4
        _need(size >= 0 and at + size <= len(d), "attribute size")
        attrs.append((name, kind, d[at:at + size]))
        at += size
    names = [a[0] for a in attrs]
    _need(len(attrs) >= 8 and names[:2] == [r[0] for r in HEAD] and names[-6:] == [r[0] for r in TAIL], "attributes and their order: %r" % names)
    val = {}
    for (name, kind, value), (_, want_kind, want_size) in zip(attrs[:2] + attrs[-6:], HEAD + TAIL):
        _need(kind == want_kind, "type of " + name)
        _need(want_size is None or len(value) == want_size, "size of " + name)
        val[name] = value
    # the channels
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
    cnames = [n for n, _ in chans]
    _need(cnames == sorted(cnames, key=lambda s: s.encode()) and len(set(cnames)) == len(cnames), "channel order")
    crypto = {kind: ["%s%02d.%s" % (LAYER_NAMES[kind], j, ch) for j in range(3) for ch in "RGBA"] for kind in (OBJECT, MATERIAL)}
    present = [kind for kind in (OBJECT, MATERIAL) if any(n in cnames for n in crypto[kind])]
    for kind in present:
        _need(all(n in cnames for n in crypto[kind]), "a kind's twelve channels")
    every_crypto = {n for kind in (OBJECT, MATERIAL) for n in crypto[kind]}
    _need(all(n in E.KNOWN_NAMES or n in every_crypto for n in cnames) and all(n in cnames for n in "RGB"), "channel names")
    _need(all(t == 2 for n, t in chans if n == "Z" or n in every_crypto), "Z and the matte channels must be FLOAT")
    _need(len({t for n, t in chans if n != "Z" and n not in every_crypto}) == 1, "one pixel type for all channels but Z and the mattes")
    # the metadata: exactly the present kinds' attributes, in the byte order of their names, all strings
    meta = attrs[2:-6]
    _need([a[0] for a in meta] == sorted((a[0] for a in meta), key=lambda s: s.encode()), "order of the cryptomatte attributes")
    _need(all(k == "string" for _, k, _ in meta), "type of a cryptomatte attribute")
    got, manifests = {a[0]: a[2] for a in meta}, {}
    _need(len(got) == len(meta), "a cryptomatte attribute twice")
    want_names = set()
    for kind in present:
        key, lname = layer_key(kind)
        pre = "cryptomatte/%s/" % key[:7]
        _need(got.get(pre + "conversion") == b"uint32_to_float32", "conversion of " + lname)
        _need(got.get(pre + "hash") == b"MurmurHash3_32", "hash of " + lname)
        _need(got.get(pre + "name") == lname.encode(), "name of " + lname)
        want_names |= {pre + "conversion", pre + "hash", pre + "name"}
        manifests[kind] = got.get(pre + "manifest")
        if manifests[kind] is not None:
            _need(0 < len(manifests[kind]) <= MANIFEST_MAX, "manifest of " + lname)
            want_names.add(pre + "manifest")
    _need(set(got) == want_names, "cryptomatte attributes: %r" % sorted(got))
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
    rows = {n: np.zeros((h, w), np.uint16 if t == 1 else np.uint32) for n, t in chans}  # the bits: an id is not a number
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
            acc = np.cumsum(np.frombuffer(t, np.uint8).astype(np.int64) - 128) + 128
            u = (acc & 255).astype(np.uint8)
            first = (n + 1) // 2
            raw = np.empty(n, np.uint8)
            raw[0::2] = u[:first]
            raw[1::2] = u[first:]
            body = raw.tobytes()
        pos = 0
        for ln in range(lines):
            for (name, t), bw in zip(chans, widths):
                rows[name][k * per_block + ln] = np.frombuffer(body, "<u2" if t == 1 else "<u4", w, pos)
                pos += bw * w
    _need(at == len(d), "bytes behind the last block")
    mattes = {}
    for kind in present:
        ids, cov = np.zeros((h, w, RANKS), np.uint32), np.zeros((h, w, RANKS), np.uint32)
        for j in range(3):
            pre = "%s%02d." % (LAYER_NAMES[kind], j)
            ids[..., 2 * j], cov[..., 2 * j], ids[..., 2 * j + 1], cov[..., 2 * j + 1] = rows[pre + "R"], rows[pre + "G"], rows[pre + "B"], rows[pre + "A"]
        mattes[kind] = (ids, cov.view(np.float32))
    planes_out = {n: rows[n].view(np.float16 if t == 1 else np.float32) for n, t in chans}
    return {"w": w, "h": h, "compression": comp, "channels": chans, "planes": planes_out, "mattes": mattes, "manifests": manifests}
