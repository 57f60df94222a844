"""tests/jpeg_ref.py - the baseline JPEG encoder of DESIGN 8.19 restated in integers: the definition the GPU encoder
(fspt_amd/csrc/fspt_jpeg.hip) has to reproduce byte for byte, and itself byte-identical to libjpeg on the MCU grid
(tests/test_jpeg_cpu.py compares it with Pillow).  numpy for the block stages, a plain Python bit writer behind them.
No float takes part.  The tables are this file's own copy of Annex K (the library's are written by
tools/make_jpeg_tables.py)."""
import numpy as np

S444, S420 = 0, 1

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]


def huff_codes(bits, vals):
    """Annex C: symbol -> (code, length), codes handed out in order of length"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality):
    """Annex K's tables under libjpeg's quality rule, natural (row-major) order: (luma, chroma)"""
    if not 1 <= quality <= 100:
        raise ValueError("quality must be in 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (QUANT_LUMA, QUANT_CHROMA))


def mcu_grid(w, h, subsampling):
    m = 16 if subsampling == S420 else 8
    return m, (w + m - 1) // m, (h + m - 1) // m


def restart_interval(w, h, subsampling, restart_mcus):
    """MCUs per interval as DRI carries it: 0 = one MCU row"""
    return restart_mcus if restart_mcus else mcu_grid(w, h, subsampling)[1]


def _fix(x):
    return int(x * 65536 + 0.5)


def planes(rgba, bottom_up, subsampling):
    """The image on its MCU grid, top-down: Y, Cb, Cr as int32 planes (the chroma planes halved for 4:2:0)"""
    a = np.asarray(rgba)
    h, w = a.shape[:2]
    if bottom_up:
        a = a[::-1]
    m, mw, mh = mcu_grid(w, h, subsampling)
    rgb = a[..., :3].astype(np.int64)
    rgb = np.concatenate([rgb, np.repeat(rgb[:, -1:], mw * m - w, axis=1)], axis=1)  # the last column, then the last row
    rgb = np.concatenate([rgb, np.repeat(rgb[-1:], mh * m - h, axis=0)], axis=0)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    if subsampling == S420:
        bias = np.tile(np.array([1, 2]), Cb.shape[1] // 4)[None, :]  # 1 in even output columns, 2 in odd ones

        def down(c):
            return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        Cb, Cr = down(Cb), down(Cr)
    return Y.astype(np.int32), Cb.astype(np.int32), Cr.astype(np.int32)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """jpeg_fdct_islow's pass over the LAST axis of d ([..., 8] int64)"""
    CB, PB = 13, 2
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CB - PB if first else CB + PB
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PB, (t10 - t11) << PB
    else:
        o[0], o[4] = _descale(t10 + t11, PB), _descale(t10 - t11, PB)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(blocks, q):
    """blocks [n, 8, 8] samples, q 64 natural-order divisors -> [n, 64] quantised coefficients in zig-zag order (int16)"""
    d = blocks.astype(np.int64) - 128
    d = _fdct_pass(d, True)                                  # rows
    d = _fdct_pass(d.transpose(0, 2, 1), False).transpose(0, 2, 1)  # columns
    c = d.reshape(-1, 64)
    assert np.abs(c).max(initial=0) < 2 ** 31
    qv = np.asarray(q, np.int64)[None, :] << 3
    m = (np.abs(c) + (qv >> 1)) // qv
    return (np.where(c < 0, -m, m)[:, ZIGZAG]).astype(np.int16)


def coefficients(rgba, bottom_up=False, quality=85, subsampling=S420):
    """Stage one: the quantised coefficients, [blocks, 64] int16 in zig-zag order, MCU-major - per MCU Y Cb Cr (4:4:4) or
    Y00 Y01 Y10 Y11 Cb Cr (4:2:0)"""
    h, w = np.asarray(rgba).shape[:2]
    _, mw, mh = mcu_grid(w, h, subsampling)
    Y, Cb, Cr = planes(rgba, bottom_up, subsampling)
    ql, qc = quant_tables(quality)

    def blocks(p):  # [rows of blocks, columns of blocks, 64]
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        return p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8), bh, bw
    yb, ybh, ybw = blocks(Y)
    yc = fdct_quant(yb, ql).reshape(ybh, ybw, 64)
    cb = fdct_quant(blocks(Cb)[0], qc).reshape(mh, mw, 64)
    cr = fdct_quant(blocks(Cr)[0], qc).reshape(mh, mw, 64)
    if subsampling == S420:
        ys = [yc[0::2, 0::2], yc[0::2, 1::2], yc[1::2, 0::2], yc[1::2, 1::2]]
    else:
        ys = [yc]
    return np.stack(ys + [cb, cr], axis=2).reshape(-1, 64)


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _encode_block(bw, c, pred, dc, ac):
    diff = int(c[0]) - pred
    nb = abs(diff).bit_length()
    bw.put(*dc[nb])
    if nb:
        bw.put((diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb)
    run = 0
    for k in range(1, 64):
        v = int(c[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        nb = abs(v).bit_length()
        bw.put(*ac[(run << 4) | nb])
        bw.put((v if v >= 0 else v - 1) & ((1 << nb) - 1), nb)
        run = 0
    if run:
        bw.put(*ac[0x00])
    return int(c[0])


def entropy(coef, subsampling, interval):
    """Stage two: the entropy-coded segment (RSTn markers included, no EOI) of MCU-major coefficients"""
    bpm = 6 if subsampling == S420 else 3
    comp = [0, 0, 0, 0, 1, 2] if subsampling == S420 else [0, 1, 2]
    n_mcu = len(coef) // bpm
    out = bytearray()
    rst = 0
    for first in range(0, n_mcu, interval):
        bw, pred = _Bits(), [0, 0, 0]
        for m in range(first, min(first + interval, n_mcu)):
            for j in range(bpm):
                ci = comp[j]
                pred[ci] = _encode_block(bw, coef[m * bpm + j], pred[ci], DC_CODES[min(ci, 1)], AC_CODES[min(ci, 1)])
        bw.flush()
        out += bw.out
        if first + interval < n_mcu:
            out += bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
    return bytes(out)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(w, h, quality=85, subsampling=S420, restart_mcus=0):
    """SOI .. SOS in libjpeg's layout (as Pillow writes it)"""
    ql, qc = quant_tables(quality)
    out = b"\xFF\xD8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, [0] + [ql[k] for k in ZIGZAG]) + _seg(0xDB, [1] + [qc[k] for k in ZIGZAG])
    hv = 0x22 if subsampling == S420 else 0x11
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _seg(0xC4, [tc_th] + bits + vals)
    out += _seg(0xDD, restart_interval(w, h, subsampling, restart_mcus).to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgba, bottom_up=False, quality=85, subsampling=S420, restart_mcus=0):
    """The whole file.  rgba: uint8 [h, w, 4] (alpha ignored)"""
    a = np.asarray(rgba)
    h, w = a.shape[:2]
    if a.ndim != 3 or a.shape[2] != 4 or not (1 <= w <= 65535 and 1 <= h <= 65535) or not 0 <= restart_mcus <= 65535 or subsampling not in (S444, S420):
        raise ValueError("bad argument")
    coef = coefficients(a, bottom_up, quality, subsampling)
    return header(w, h, quality, subsampling, restart_mcus) + entropy(coef, subsampling, restart_interval(w, h, subsampling, restart_mcus)) + b"\xFF\xD9"


def bound(w, h, subsampling=S420, restart_mcus=0):
    """fspt_jpeg_bound restated: header, 416 bytes per block (1660 bits at most, every byte stuffed), per interval a pad
    byte (stuffed) and a marker"""
    _, mw, mh = mcu_grid(w, h, subsampling)
    n_mcu = mw * mh
    ri = restart_interval(w, h, subsampling, restart_mcus)
    return len(header(1, 1)) + n_mcu * (6 if subsampling == S420 else 3) * 416 + ((n_mcu + ri - 1) // ri) * 4 + 2
