#!/usr/bin/env python3
"""tools/make_png_tables.py - the PNG encoder's constant tables from the standards' definitions.

CRC-32 (ISO 3309, the PNG specification's annex D, reflected polynomial 0xEDB88320): the byte table, and the powers
x^(8 * 2^k) mod P that move a checksum past 2^k bytes - a workgroup's lanes take the checksum of a slice each and the sum of
the moved checksums is the whole's (CRC is linear over GF(2); this is zlib's crc32_combine written as a sum).  RFC 1951
3.2.5: per match length 3..258 its symbol, its number of extra bits and their value in one word; 3.2.7: the order of the
code-length code's lengths.  The output is fspt_amd/csrc/fspt_png_tables.hpp.
    usage: python tools/make_png_tables.py [--check]     (--check: compare with the committed file, write nothing)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "fspt_amd", "csrc", "fspt_png_tables.hpp")
POLY = 0xEDB88320
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def crc_table():
    out = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        out.append(c)
    return out


def crc32(data, table=crc_table()):
    c = 0xFFFFFFFF
    for b in data:
        c = table[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mulmod(a, b):
    """a * b mod P, polynomials over GF(2) in the reflected order: bit 31 is x^0"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def x8_powers(n=16):
    """x^(8 * 2^k) mod P for k < n"""
    p = 0x40000000  # x^1
    out = []
    for k in range(3 + n):
        if k >= 3:
            out.append(p)
        p = mulmod(p, p)
    return out


def shift(crc, n_bytes, powers=x8_powers()):
    """the checksum `crc` of a message as its share of the checksum of that message followed by n_bytes more"""
    k = 0
    while n_bytes:
        if n_bytes & 1:
            crc = mulmod(powers[k], crc)
        n_bytes >>= 1
        k += 1
    return crc


def length_codes():
    """per length 3..258: symbol | extra bits << 12 | extra value << 16"""
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    base = []
    for k, e in enumerate(extra):
        base.append(258 if k == 28 else 3 if k == 0 else base[-1] + (1 << extra[k - 1]))
    out = []
    for n in range(3, 259):
        k = 28 if n == 258 else max(j for j in range(28) if base[j] <= n)
        assert n - base[k] < 1 << extra[k]
        out.append((257 + k) | (extra[k] << 12) | ((n - base[k]) << 16))
    return out


def rows(vals, per, fmt):
    return ["  " + " ".join(fmt(v) + "," for v in vals[r:r + per]) for r in range(0, len(vals), per)]


def text():
    out = ["// fspt_png_tables.hpp - written by tools/make_png_tables.py; do not edit.  The PNG encoder's constant tables (DESIGN 8.20):",
           "// CRC-32's byte table and the powers that move a checksum past 2^k bytes, RFC 1951's match lengths and code-length order.",
           "#pragma once", "#include <cstdint>", "namespace fspt {"]

    def arr(decl, vals, per, fmt):
        out.append(f"static constexpr {decl} = {{")
        out.extend(rows(vals, per, fmt))
        out.append("};")
    x8 = lambda v: f"0x{v:08X}u"  # noqa: E731
    arr("uint32_t PNG_CRC_TABLE[256]", crc_table(), 8, x8)
    arr("uint32_t PNG_CRC_X8POW[16]", x8_powers(), 8, x8)             # x^(8 * 2^k) mod P
    arr("uint32_t PNG_LEN_CODE[256]", length_codes(), 8, x8)          # [length - 3] = symbol | extra bits << 12 | extra value << 16
    arr("uint8_t PNG_CL_ORDER[19]", CL_ORDER, 19, lambda v: f"{v:2d}")
    out.append(f"static constexpr uint32_t PNG_CRC_POLY = 0x{POLY:08X}u;")
    out.append(f"static constexpr uint32_t PNG_CRC_IDAT = 0x{crc32(b'IDAT'):08X}u; // the checksum of the four bytes every IDAT's checksum starts with")
    out.append("} // namespace fspt")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    t = text()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if open(OUT).read() == t else "fspt_png_tables.hpp differs from the generator's output")
    open(OUT, "w").write(t)
    print("wrote", os.path.relpath(OUT, ROOT))
