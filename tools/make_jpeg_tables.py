#!/usr/bin/env python3
"""tools/make_jpeg_tables.py - the JPEG encoder's constant tables from the standard's values.

ITU-T T.81: the zig-zag sequence (Figure A.6), Annex K's two quantisation tables (K.1, K.2) and four Huffman tables
(K.3 - K.6) as BITS / HUFFVAL lists.  Derived here, so that nothing is derived on the device: the inverse zig-zag, and
per table the codes of Annex C as (code << 8 | length) indexed by symbol, 0 where a symbol has no code.  The per-block
worst case the scratch buffer is sized by follows from the same tables: the longest DC code plus its category's bits,
and 63 times the longest AC code plus its size bits.  The output is fspt_amd/csrc/fspt_jpeg_tables.hpp.
    usage: python tools/make_jpeg_tables.py [--check]     (--check: compare with the committed file, write nothing)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "fspt_amd", "csrc", "fspt_jpeg_tables.hpp")


def zigzag():
    """Figure A.6: the natural (row-major) index of every zig-zag position, walked along the anti-diagonals"""
    out = []
    for s in range(15):
        rows = range(max(0, s - 7), min(s, 7) + 1)
        for r in (rows if s & 1 else reversed(rows)):
            out.append(r * 8 + (s - r))
    return out


QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]


AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]


def codes(bits, vals, n):
    """Annex C: (code << 8 | length) per symbol < n, 0 where the table has none"""
    out, code, k = [0] * n, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code << 8) | length
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals) == sum(bits)
    return out


def worst_block_bits(dc, ac):
    """the longest code of one block: a DC category's code and bits, then 63 coefficients of run 0"""
    return max((c & 255) + s for s, c in enumerate(dc) if c) + 63 * max((c & 255) + (s & 15) for s, c in enumerate(ac) if c and s & 15)


def rows(vals, per, fmt):
    return ["  " + " ".join(fmt(v) + "," for v in vals[r:r + per]) for r in range(0, len(vals), per)]


def text():
    zz = zigzag()
    inv = [zz.index(k) for k in range(64)]
    dc = [codes(DC_LUMA_BITS, DC_VALS, 12), codes(DC_CHROMA_BITS, DC_VALS, 12)]
    ac = [codes(AC_LUMA_BITS, AC_LUMA_VALS, 256), codes(AC_CHROMA_BITS, AC_CHROMA_VALS, 256)]
    worst = max(worst_block_bits(dc[k], ac[k]) for k in range(2))
    out = ["// fspt_jpeg_tables.hpp - written by tools/make_jpeg_tables.py; do not edit.  The JPEG encoder's constant tables (DESIGN 8.19):",
           "// ITU-T T.81 Figure A.6 and Annex K as given, and what Annex C derives from them.",
           "#pragma once", "#include <cstdint>", "namespace fspt {"]

    def arr(decl, vals, per=16, fmt=lambda v: f"{v:3d}"):
        out.append(f"static constexpr {decl} = {{")
        out.extend(rows(vals, per, fmt))
        out.append("};")
    arr("uint8_t JPEG_ZIGZAG[64]", zz)          # natural index of zig-zag position k
    arr("uint8_t JPEG_ZIGZAG_INV[64]", inv)     # zig-zag position of natural index k
    arr("uint8_t JPEG_QUANT_LUMA[64]", QUANT_LUMA)
    arr("uint8_t JPEG_QUANT_CHROMA[64]", QUANT_CHROMA)
    for name, bits, vals in (("DC_LUMA", DC_LUMA_BITS, DC_VALS), ("AC_LUMA", AC_LUMA_BITS, AC_LUMA_VALS),
                             ("DC_CHROMA", DC_CHROMA_BITS, DC_VALS), ("AC_CHROMA", AC_CHROMA_BITS, AC_CHROMA_VALS)):
        arr(f"uint8_t JPEG_{name}_BITS[16]", bits)
        arr(f"uint8_t JPEG_{name}_VALS[{len(vals)}]", vals, 24, lambda v: f"0x{v:02X}")
    x8 = lambda v: f"0x{v:06X}u"  # noqa: E731
    arr("uint32_t JPEG_DC_CODES[2][12]", dc[0] + dc[1], 12, x8)      # [luma | chroma][category] = code << 8 | length
    arr("uint32_t JPEG_AC_CODES[2][256]", ac[0] + ac[1], 8, x8)      # [luma | chroma][run << 4 | size]
    out.append(f"static constexpr uint32_t JPEG_BLOCK_MAX_BITS = {worst}u; // the longest code of one block, before byte stuffing")
    out.append("} // namespace fspt")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    t = text()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if open(OUT).read() == t else "fspt_jpeg_tables.hpp differs from the generator's output")
    open(OUT, "w").write(t)
    print("wrote", os.path.relpath(OUT, ROOT))
