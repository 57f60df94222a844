#!/usr/bin/env python3
"""tools/make_texture_tables.py - the texture packer's two decode tables as float32 bit patterns.

  lin[i]  = fround(i / 255)
  srgb[i] = fround(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4)),  c = i / 255 in float64

the sRGB decode of fspt.js resampleImage and scene.resample_image evaluated in float64 and rounded ONCE: every entry is the
float32 nearest the exact decode, srgb[0] = 0, srgb[255] = 1, and the table does not decrease.  (The hosts' own tables round
after every step in float32 - fround(c + 0.055), fround(. / 1.055), fround(pow) - and miss the exact decode by up to 3.6 ulp,
130 of 256 entries by more than one, srgb[255] = 1 - 2^-23 among them; --hosts prints that comparison.)  The output is
fspt_amd/csrc/fspt_texpack_tables.hpp: data, so that no division and no pow runs on the device and no libm decides a texel.
    usage: python tools/make_texture_tables.py [--check | --hosts]     (--check: compare with the committed file, write nothing)
"""
import math
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "fspt_amd", "csrc", "fspt_texpack_tables.hpp")


def fround(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def srgb_decode(c):
    return c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)


def tables():
    return [fround(i / 255) for i in range(256)], [fround(srgb_decode(i / 255)) for i in range(256)]


def host_srgb():
    """fspt.js resampleImage's table: the same decode with every intermediate rounded to float32"""
    out = []
    for i in range(256):
        c = fround(i / 255)
        out.append(fround(c / 12.92) if c <= 0.04045 else fround(math.pow(fround(fround(c + 0.055) / 1.055), 2.4)))
    return out


def text():
    lin, srgb = tables()
    out = ["// fspt_texpack_tables.hpp - written by tools/make_texture_tables.py; do not edit.  The texture packer's decode tables",
           "// (DESIGN 8.18) as float32 bit patterns: lin[i] = i / 255, srgb[i] = the sRGB decode of lin[i].",
           "#pragma once", "#include <cstdint>", "namespace fspt {"]
    for name, tab in (("TEX_LIN_BITS", lin), ("TEX_SRGB_BITS", srgb)):
        out.append(f"static constexpr uint32_t {name}[256] = {{")
        for r in range(0, 256, 8):
            out.append("  " + " ".join(f"0x{bits(v):08X}u," for v in tab[r:r + 8]))
        out.append("};")
    out.append("} // namespace fspt")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    t = text()
    if "--hosts" in sys.argv[1:]:
        import numpy as np
        mine, theirs = np.array(tables()[1], np.float32), np.array(host_srgb(), np.float32)
        exact = np.array([srgb_decode(i / 255) for i in range(256)])
        err = np.abs(theirs.astype(np.float64) - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
        print(f"hosts' float32-chained table: {int((mine != theirs).sum())} of 256 entries differ from the committed one; "
              f"max {err.max():.2f} ulp from the float64 decode, {int((err > 1).sum())} entries above 1 ulp; srgb[255] = {theirs[255]!r}")
        sys.exit(0)
    if "--check" in sys.argv[1:]:
        sys.exit(0 if open(OUT).read() == t else "fspt_texpack_tables.hpp differs from the generator's output")
    open(OUT, "w").write(t)
    print("wrote", os.path.relpath(OUT, ROOT))
