"""tests/png_ref.py - the PNG encoder of DESIGN 8.20 restated in integers: the definition the GPU encoder
(fspt_amd/csrc/fspt_png.hip, fspt_deflate.hip) has to reproduce byte for byte.  numpy for the filter stage, a plain Python bit writer behind
it.  No float takes part, and nothing of zlib: the checksums are written out here and tests/test_png_cpu.py compares them
(and the files) with zlib and Pillow.

The file: signature, IHDR (8 bit, colour type 2 or 6, no interlace), one IDAT per deflate chunk (the first one begins with
the zlib header 78 01), one 4-byte IDAT with the Adler-32 of the filtered stream, IEND.

The deflate stream: the filtered stream cut at multiples of chunk_bytes; a chunk starts on a byte boundary and is one
block.  Its tokens are literals and matches of distance 1 (tokens()).  Its dynamic block's codes follow from the token
histogram alone (code_lengths(), rle_lengths()); when that block, rounded up to bytes, is not shorter than the stored block
(5 + the chunk's bytes) the chunk is stored.  A dynamic chunk that is not the last is followed by an empty stored block,
which ends on a byte boundary; the last chunk carries BFINAL and is padded with zero bits."""
import numpy as np

ADAPTIVE = 5                     # FSPT_PNG_FILTER_ADAPTIVE; 0..4 = None, Sub, Up, Average, Paeth for every row
CHUNK_DEFAULT = 16384            # FSPT_PNG_CHUNK
CHUNK_MIN, CHUNK_MAX = 256, 32768
STORED, DYNAMIC = 0, 2           # BTYPE
SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])
ZLIB_HEADER = bytes([0x78, 0x01])  # deflate, 32 KiB window, no dictionary; 0x7801 = 31 * 991
IEND = bytes([0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82])
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ADLER_MOD = 65521

# RFC 1951 3.2.5: a match length 3..258 -> (symbol, extra bits, base)
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LEN_BASE = []
for _k, _e in enumerate(LEN_EXTRA):
    LEN_BASE.append(258 if _k == 28 else 3 if _k == 0 else LEN_BASE[-1] + (1 << LEN_EXTRA[_k - 1]))


def len_symbol(n):
    k = 28 if n == 258 else max(j for j in range(28) if LEN_BASE[j] <= n)
    return 257 + k, LEN_EXTRA[k], LEN_BASE[k]


CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    CRC_TABLE.append(_c)


def crc32(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    for b in data:
        c = CRC_TABLE[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler_pair(data):
    """(A, B) of Adler-32 over `data` from the initial state (1, 0)"""
    a, b = 1, 0
    for v in data:
        a = (a + v) % ADLER_MOD
        b = (b + a) % ADLER_MOD
    return a, b


def adler_combine(p1, p2, len2):
    """the pair of two streams one behind the other, from their own pairs"""
    return (p1[0] + p2[0] - 1) % ADLER_MOD, (p1[1] + p2[1] + len2 * (p1[0] - 1)) % ADLER_MOD


# --------------------------------------------------------------------------------------------------------------------
# stage one: the filtered stream
# --------------------------------------------------------------------------------------------------------------------
def filtered(rgba, bottom_up=False, channels=3, filt=ADAPTIVE):
    """(the stream as bytes: h rows of 1 + w * channels, the filter type chosen per row)"""
    a = np.asarray(rgba)
    if a.ndim != 3 or a.shape[2] != 4 or a.dtype != np.uint8:
        raise ValueError("need uint8 [h, w, 4]")
    if channels not in (3, 4) or not 0 <= filt <= ADAPTIVE:
        raise ValueError("channels 3 or 4, filter 0..5")
    if bottom_up:
        a = a[::-1]
    h, w = a.shape[:2]
    rows = a[..., :channels].reshape(h, w * channels).astype(np.int32)
    out, chosen = bytearray(), []
    zero = np.zeros(w * channels, np.int32)
    for y in range(h):
        x = rows[y]
        up = rows[y - 1] if y else zero
        left = np.concatenate([zero[:channels], x[:-channels]]) if w > 1 else zero[:channels].copy()
        ul = np.concatenate([zero[:channels], up[:-channels]]) if w > 1 else zero[:channels].copy()
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        res = [(x - pred) & 255 for pred in (zero, left, up, (left + up) >> 1, paeth)]
        if filt == ADAPTIVE:
            cost = [int(np.where(r < 128, r, 256 - r).sum()) for r in res]
            t = cost.index(min(cost))  # a tie: the lowest type
        else:
            t = filt
        chosen.append(t)
        out.append(t)
        out += res[t].astype(np.uint8).tobytes()
    return bytes(out), chosen


# --------------------------------------------------------------------------------------------------------------------
# stage two: deflate, chunk by chunk
# --------------------------------------------------------------------------------------------------------------------
def tokens(chunk):
    """A maximal run of R equal bytes (its first byte differs from the one before it, or starts the chunk) is one literal,
    then matches of distance 1 and length min(remaining, 258) while at least 3 remain, then 1 or 2 literals.
    -> [(literal,) | (length,)]; a token is a function of its position in its run and of the run's length alone"""
    out, i, n = [], 0, len(chunk)
    while i < n:
        r = 1
        while i + r < n and chunk[i + r] == chunk[i]:
            r += 1
        out.append(("lit", chunk[i]))
        rem = r - 1
        while rem >= 3:
            t = min(rem, 258)
            out.append(("len", t))
            rem -= t
        out += [("lit", chunk[i])] * rem
        i += r
    return out


def code_lengths(freq, max_bits):
    """The length-limited code of a histogram, a function of the histogram alone.
    1. The used symbols (freq > 0), sorted by (freq, symbol) ascending: the leaves.  One leaf: length 1.
    2. Huffman's tree by the two-queue merge: n - 1 times the two smallest of (next leaf, next internal node) are joined;
       when a leaf and an internal node weigh the same the leaf is taken first.  count[d] = leaves at depth d, depths
       above max_bits counted at max_bits.
    3. While the Kraft sum (sum of count[d] << (max_bits - d)) exceeds 1 << max_bits: one code leaves max_bits, and the
       longest shorter code that exists is split - count[max_bits] -= 1; the largest d < max_bits with count[d] > 0:
       count[d] -= 1, count[d + 1] += 2; the sum falls by one.
    4. Lengths are handed out along the sorted order from its end: the most frequent symbols get the shortest codes."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    lens = [0] * len(freq)
    n = len(used)
    if n == 0:
        return lens
    if n == 1:
        lens[used[0][1]] = 1
        return lens
    leaf = [f for f, _ in used]
    node, parent_leaf, parent_node = [], [0] * n, [0] * (n - 1)
    i = j = 0
    for k in range(n - 1):
        w = 0
        for _ in range(2):
            if i < n and (j >= k or leaf[i] <= node[j]):
                w += leaf[i]
                parent_leaf[i] = k
                i += 1
            else:
                w += node[j]
                parent_node[j] = k
                j += 1
        node.append(w)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[parent_node[k]] + 1
    count = [0] * (max_bits + 1)
    for i in range(n):
        count[min(depth[parent_leaf[i]] + 1, max_bits)] += 1
    total = sum(count[d] << (max_bits - d) for d in range(1, max_bits + 1))
    while total > 1 << max_bits:
        count[max_bits] -= 1
        d = max(d for d in range(1, max_bits) if count[d])
        count[d] -= 1
        count[d + 1] += 2
        total -= 1
    r = n
    for d in range(1, max_bits + 1):
        for _ in range(count[d]):
            r -= 1
            lens[used[r][1]] = d
    return lens


def canonical(lens):
    """RFC 1951 3.2.2: symbol -> code (most significant bit first)"""
    max_bits = max(lens)
    count = [0] * (max_bits + 2)
    for v in lens:
        if v:
            count[v] += 1
    nxt, code = [0] * (max_bits + 2), 0
    for d in range(1, max_bits + 1):
        code = (code + count[d - 1]) << 1
        nxt[d] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = nxt[v]
            nxt[v] += 1
    return out


def rle_lengths(seq):
    """The code lengths as code-length symbols, greedy from the left.  At position i with value v and r equal values from
    there on: v = 0 and r >= 11: symbol 18 for min(r, 138); v = 0 and r >= 3: symbol 17 for r; v != 0, the value before i
    is v too and r >= 3: symbol 16 for min(r, 6); else v itself.  -> [(symbol, extra value, extra bits)]"""
    out, i, m = [], 0, len(seq)
    while i < m:
        v, r = seq[i], 1
        while i + r < m and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            t = min(r, 138)
            out.append((18, t - 11, 7))
        elif v == 0 and r >= 3:
            t = r
            out.append((17, t - 3, 3))
        elif v and i and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, t - 3, 2))
        else:
            t = 1
            out.append((v, 0, 0))
        i += t
    return out


class BitWriter:
    """deflate's order: bits fill a byte from its least significant end; Huffman codes go in most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def deflate_chunk(chunk, last):
    """-> (the chunk's bytes in the deflate stream, block type, longest literal/length code, longest code-length code)"""
    n = len(chunk)
    toks = tokens(chunk)
    freq = [0] * 286
    for kind, v in toks:
        freq[v if kind == "lit" else len_symbol(v)[0]] += 1
    freq[256] = 1
    ll = code_lengths(freq, 15)
    hlit = max(s for s in range(286) if ll[s]) + 1  # >= 257: the end-of-block symbol is used
    syms = rle_lengths(ll[:hlit] + [1])             # one distance code, of one bit, always
    cfreq = [0] * 19
    for s, _, _ in syms:
        cfreq[s] += 1
    cl = code_lengths(cfreq, 7)
    hclen = max(k for k in range(19) if cl[CL_ORDER[k]]) + 1
    hclen = max(hclen, 4)
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl[s] + e for s, _, e in syms)
    for kind, v in toks:
        bits += ll[v] if kind == "lit" else ll[len_symbol(v)[0]] + len_symbol(v)[1] + 1
    bits += ll[256]
    if (bits + 7) // 8 >= 5 + n:
        return bytes([1 if last else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(chunk), STORED, 0, 0
    w = BitWriter()
    w.bits(1 if last else 0, 1)
    w.bits(DYNAMIC, 2)
    w.bits(hlit - 257, 5)
    w.bits(0, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl[CL_ORDER[k]], 3)
    ccode = canonical(cl)
    for s, v, e in syms:
        w.code(ccode[s], cl[s])
        w.bits(v, e)
    lcode = canonical(ll)
    for kind, v in toks:
        if kind == "lit":
            w.code(lcode[v], ll[v])
        else:
            s, e, base = len_symbol(v)
            w.code(lcode[s], ll[s])
            w.bits(v - base, e)
            w.bits(0, 1)  # distance code 0: distance 1
    w.code(lcode[256], ll[256])
    assert len(w.out) * 8 + w.n == bits
    if not last:
        w.bits(0, 3)  # an empty stored block: the next chunk starts on a byte boundary
        w.align()
        w.out += bytes([0, 0, 255, 255])
    w.align()
    return bytes(w.out), DYNAMIC, max(ll), max(cl)


def chunk(kind, payload):
    body = kind + payload
    return len(payload).to_bytes(4, "big") + body + crc32(body).to_bytes(4, "big")


def resolve_chunk_bytes(chunk_bytes):
    if chunk_bytes == 0:
        return CHUNK_DEFAULT
    if not CHUNK_MIN <= chunk_bytes <= CHUNK_MAX:
        raise ValueError("chunk_bytes must be 0 or in 256..32768")
    return chunk_bytes


def encode(rgba, bottom_up=False, channels=3, filt=ADAPTIVE, chunk_bytes=0, stats=None):
    """The file.  stats (a dict, or None) receives "filters" (per row), "blocks" (BTYPE per chunk), "max_len" and
    "max_cl_len" (per chunk: its longest literal/length and code-length code, 0 for a stored chunk), "idat" (the payloads)
    and "stream" (the filtered stream)."""
    cb = resolve_chunk_bytes(chunk_bytes)
    stream, chosen = filtered(rgba, bottom_up, channels, filt)
    h, w = np.asarray(rgba).shape[:2]
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError("width and height must be in 1..65535")
    out = bytearray(SIGNATURE)
    out += chunk(b"IHDR", w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 2 if channels == 3 else 6, 0, 0, 0]))
    st = {"filters": chosen, "blocks": [], "max_len": [], "max_cl_len": [], "idat": [], "stream": stream}
    pair = (1, 0)
    n_chunks = (len(stream) + cb - 1) // cb
    for k in range(n_chunks):
        part = stream[k * cb:(k + 1) * cb]
        data, btype, ml, mc = deflate_chunk(part, k == n_chunks - 1)
        payload = (ZLIB_HEADER if k == 0 else b"") + data
        out += chunk(b"IDAT", payload)
        pair = adler_combine(pair, adler_pair(part), len(part))
        st["blocks"].append(btype)
        st["max_len"].append(ml)
        st["max_cl_len"].append(mc)
        st["idat"].append(payload)
    trailer = ((pair[1] << 16) | pair[0]).to_bytes(4, "big")
    st["idat"].append(trailer)
    out += chunk(b"IDAT", trailer)
    out += IEND
    if stats is not None:
        stats.update(st)
    return bytes(out)


def bound(w, h, channels=3, chunk_bytes=0):
    """fspt_png_bound: signature, IHDR, zlib header, the Adler IDAT, IEND; per chunk its bytes, a stored header, the
    empty stored block, an IDAT's framing"""
    cb = resolve_chunk_bytes(chunk_bytes)
    n = h * (1 + w * channels)
    return 8 + 25 + 2 + 16 + 12 + n + ((n + cb - 1) // cb) * (5 + 5 + 12)
