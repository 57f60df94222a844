// fspt_exr.hip - an OpenEXR encoder on the GPU: scene-linear radiance (W*H float4) and, for the feature layers,
// the first-hit guides (W*H x 2 float4) become a single-part scanline OpenEXR 2 file in device memory, so that only the file's
// bytes cross the bus.  Integer arithmetic throughout (the half conversion included: no denormal mode takes part); the bytes
// are tests/exr_ref.py's, which states the format.
//   k_exr_rows      one lane per pixel of a scanline: every channel's value canonicalised and converted, then its bytes
//                   written where the block's reordered and predicted stream has them - the even bytes of a block in its
//                   first half, the odd ones behind them, each minus the byte to its left in that order, which is a byte of
//                   the value before it (the neighbouring pixel, the end of the channel before, the end of the scanline
//                   before; at the seam the block's last even byte).  Compression none: the planar bytes into the file.
//   k_deflate       (fspt_deflate.hip) a block is a segment: a zlib stream of its own, in chunks that restart at its first byte
//   k_exr_offsets   per block the chunks' lengths and Adler pairs combined, compressed or raw, a scan of the sizes in 64 bits:
//                   the header, the offset table and every block's (y, size)
//   k_exr_pack      one workgroup per chunk: its deflated bytes, or, where its block fell back, that range of the raw block
#include "fspt_internal.hpp"
#include "fspt_encode_device.hpp"

namespace fspt {
namespace {

constexpr uint32_t EXR_RT = 256u; // lanes of a rows workgroup

struct ExrRowsP {
  const uint4 *rgba, *feat; // the floats as their bits
  uint32_t w, h, bottom_up, n_ch, lpb, predicted, keep_raw;
  uint32_t line_bytes, block_bytes;
  const ExrChannel *ch;     // n_ch of them, in device memory behind the header (an array in the arguments, indexed by a variable, would be copied to scratch)
  uint8_t *stream;          // a block of the predicted stream every block_bytes
  uint8_t *raw;             // raw blocks every raw_stride, raw_skip bytes in
  size_t raw_stride, raw_skip;
};

// float32 bits -> binary16 bits, round to nearest even: overflow to infinity, results below 2^-14 as exact subnormals, every
// NaN 0x7E00.  Integers only, so float32 subnormals (which all round to zero) need no mode of the hardware.
__device__ __forceinline__ uint32_t exr_half(uint32_t u) {
  const uint32_t s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return 0x7E00u;
  if (a >= 0x47800000u) return s | 0x7C00u; // 65536 and above, infinity
  if (a >= 0x38800000u) {                   // 2^-14 and above: exponent rebiased by 112, 13 bits dropped; a carry out of the
    const uint32_t r = a - 0x38000000u;     // mantissa moves into the exponent, from 65520 on into infinity's
    const uint32_t h = r >> 13, rem = r & 0x1FFFu;
    return s | (h + ((rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ? 1u : 0u));
  }
  const uint32_t e = a >> 23;
  if (e < 102u) return s; // below 2^-25: zero (2^-25 itself is a tie between 0 and 2^-24 and goes to the even 0 below)
  const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, sh = 126u - e; // 14..24: the value in units of 2^-24
  const uint32_t h = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  return s | (h + ((rem > half || (rem == half && (h & 1u))) ? 1u : 0u));
}

// a channel's value as the file holds it: 2 or 4 bytes, little-endian
__device__ __forceinline__ uint32_t exr_conv(uint32_t u, uint32_t bytes) {
  if (bytes == 2u) return exr_half(u);
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : u;
}

struct ExrPx { uint32_t a0, a1, a2, a3, f0, f1, f2, f3, f4, f5, f6, f7; };

// the pixel x of file scanline y (0 = the top)
__device__ __forceinline__ ExrPx exr_load(const ExrRowsP &p, uint32_t x, uint32_t y) {
  const uint32_t row = p.bottom_up ? p.h - 1u - y : y;
  const size_t i = (size_t)row * p.w + x;
  const uint4 a = p.rgba[i];
  uint4 g = make_uint4(0u, 0u, 0u, 0u), n = g;
  if (p.feat) { g = p.feat[2u * i]; n = p.feat[2u * i + 1u]; }
  return ExrPx{a.x, a.y, a.z, a.w, g.x, g.y, g.z, g.w, n.x, n.y, n.z, n.w};
}

__device__ __forceinline__ uint32_t exr_sel(const ExrPx &q, uint32_t src) {
  // masks, not conditionals: a conditional among neighbouring members is turned into an indexed load, which puts the pixel in scratch
  const uint32_t k = src & 3u, m0 = 0u - (uint32_t)(k == 0u), m1 = 0u - (uint32_t)(k == 1u), m2 = 0u - (uint32_t)(k == 2u), m3 = 0u - (uint32_t)(k == 3u);
  const uint32_t a = (q.a0 & m0) | (q.a1 & m1) | (q.a2 & m2) | (q.a3 & m3);
  const uint32_t g = (q.f0 & m0) | (q.f1 & m1) | (q.f2 & m2) | (q.f3 & m3);
  const uint32_t n = (q.f4 & m0) | (q.f5 & m1) | (q.f6 & m2) | (q.f7 & m3);
  return (a & (0u - (uint32_t)(src < 4u))) | (g & (0u - (uint32_t)((src >> 2) == 1u))) | (n & (0u - (uint32_t)(src >= 8u)));
}

// a value's last even and last odd byte: what the first even and the first odd byte of the next value are predicted from
__device__ __forceinline__ uint32_t exr_last_even(uint32_t v, uint32_t bytes) { return bytes == 2u ? v & 255u : (v >> 16) & 255u; }
__device__ __forceinline__ uint32_t exr_last_odd(uint32_t v, uint32_t bytes) { return bytes == 2u ? (v >> 8) & 255u : v >> 24; }

__global__ void __launch_bounds__(EXR_RT) k_exr_rows(ExrRowsP p) {
  const uint32_t x = blockIdx.x * EXR_RT + threadIdx.x, y = blockIdx.y;
  if (x >= p.w) return;
  const uint32_t b = y / p.lpb, l = y - b * p.lpb;
  const uint32_t lines = min(p.lpb, p.h - b * p.lpb), half = lines * p.line_bytes / 2u; // (every value has 2 or 4 bytes: a block's length is even)
  // the value before this one in the block's order: the pixel to the left in the same channel; for the first pixel the last
  // pixel of the channel before; for the first channel that of the last channel of the scanline before; and for the block's
  // first value, at the seam of the two halves, the block's last value.  (wrap: one address for the whole wave.)
  const ExrPx cur = exr_load(p, x, y);
  const ExrPx left = exr_load(p, x ? x - 1u : p.w - 1u, y);
  const ExrPx wrap = exr_load(p, p.w - 1u, l ? y - 1u : b * p.lpb + lines - 1u);
  uint8_t *t = p.stream + (size_t)b * p.block_bytes;
  uint8_t *r = p.raw + (size_t)b * p.raw_stride + p.raw_skip;
  for (uint32_t c = 0; c < p.n_ch; ++c) {
    const ExrChannel ch = p.ch[c];
    const uint32_t v = exr_conv(exr_sel(cur, ch.src), ch.bytes);
    const uint32_t q = l * p.line_bytes + ch.off * p.w + x * ch.bytes; // the value's first byte in the raw block
    if (p.keep_raw) {
      r[q] = (uint8_t)v; r[q + 1u] = (uint8_t)(v >> 8);
      if (ch.bytes == 4u) { r[q + 2u] = (uint8_t)(v >> 16); r[q + 3u] = (uint8_t)(v >> 24); }
    }
    if (!p.predicted) continue;
    uint32_t pe, po;
    if (x) { const uint32_t u = exr_conv(exr_sel(left, ch.src), ch.bytes); pe = exr_last_even(u, ch.bytes); po = exr_last_odd(u, ch.bytes); }
    else {
      const ExrChannel pc = p.ch[c ? c - 1u : p.n_ch - 1u];
      const uint32_t u = exr_conv(c ? exr_sel(left, pc.src) : exr_sel(wrap, pc.src), pc.bytes);
      pe = exr_last_even(u, pc.bytes); po = exr_last_odd(u, pc.bytes);
    }
    const uint32_t i = q >> 1;
    const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u;
    t[i] = (uint8_t)(q ? b0 - pe + 128u : b0); // (the block's first byte stays as it is)
    t[half + i] = (uint8_t)(b1 - (q ? po : pe) + 128u); // (the seam: the first odd byte follows the block's last even byte)
    if (ch.bytes == 4u) {
      const uint32_t b2 = (v >> 16) & 255u, b3 = v >> 24;
      t[i + 1u] = (uint8_t)(b2 - b0 + 128u);
      t[half + i + 1u] = (uint8_t)(b3 - b1 + 128u);
    }
  }
}

// byte q of raw block b, converted again from the floats (form 0 of the raw fallback)
__device__ __forceinline__ uint32_t exr_raw_byte(const ExrRowsP &p, uint32_t b, uint32_t q) {
  const uint32_t l = q / p.line_bytes, o = q - l * p.line_bytes;
  uint32_t c = 0;
  while (c + 1u < p.n_ch && p.ch[c + 1u].off * p.w <= o) ++c;
  const ExrChannel ch = p.ch[c];
  const uint32_t in = o - ch.off * p.w, x = in / ch.bytes, k = in - x * ch.bytes;
  const uint32_t y = b * p.lpb + l, row = p.bottom_up ? p.h - 1u - y : y;
  const size_t i = (size_t)row * p.w + x;
  const uint32_t u = ch.src < 4u ? ((const uint32_t *)p.rgba)[4u * i + ch.src] : ((const uint32_t *)p.feat)[8u * i + ch.src - 4u];
  return (exr_conv(u, ch.bytes) >> (8u * k)) & 255u;
}

struct ExrOffP {
  const uint32_t *meta;
  const uint8_t *hdr;
  uint32_t hdr_len, n_blocks, cps, cb, lpb, h, line_bytes, compressed;
  uint32_t *chunk_off;
  uint64_t *blk;
  uint8_t *out;
};

__device__ __forceinline__ void exr_put_le(uint8_t *o, uint64_t v, uint32_t n) { for (uint32_t i = 0; i < n; ++i) o[i] = (uint8_t)(v >> (8u * i)); }

// The header; per block: where its chunks land in it, its zlib stream's length (the chunks, and 4 bytes of Adler-32: the
// chunks' pairs combined in order, A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1)), raw where that is not shorter; a scan of
// (8 + size) in 64 bits from the end of the offset table: the table's entry and the block's (y, size).
__global__ void __launch_bounds__(256) k_exr_offsets(ExrOffP p) {
  __shared__ uint64_t s[256];
  __shared__ uint64_t running;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < p.hdr_len; i += 256u) p.out[i] = p.hdr[i];
  if (t == 0) running = (uint64_t)p.hdr_len + 8ull * p.n_blocks;
  __syncthreads();
  for (uint32_t base = 0; base < p.n_blocks; base += 256u) {
    const uint32_t i = base + t;
    uint32_t size = 0, adler = 0;
    if (i < p.n_blocks) {
      const uint32_t n_b = min(p.lpb, p.h - i * p.lpb) * p.line_bytes;
      size = n_b;
      if (p.compressed) {
        const uint32_t nck = (n_b + p.cb - 1u) / p.cb;
        uint32_t len = 0, A = 1u, B = 0u;
        for (uint32_t j = 0; j < nck; ++j) {
          const uint32_t k = i * p.cps + j;
          const uint32_t *m = p.meta + (size_t)k * DEFLATE_META;
          p.chunk_off[k] = len;
          len += m[0];
          const uint32_t len2 = min(p.cb, n_b - j * p.cb);
          B = (uint32_t)((B + m[3] + (uint64_t)len2 * ((A + DEFLATE_ADLER - 1u) % DEFLATE_ADLER)) % DEFLATE_ADLER);
          A = (A + m[2] + DEFLATE_ADLER - 1u) % DEFLATE_ADLER;
        }
        if (len + 4u < n_b) size = len + 4u;
        adler = (B << 16) | A;
      }
    }
    const uint64_t v = i < p.n_blocks ? 8ull + size : 0ull;
    enc_scan256(s, v);
    const uint64_t off = running + s[t] - v;
    if (i < p.n_blocks) {
      p.blk[2u * i] = off; p.blk[2u * i + 1u] = ((uint64_t)size << 32) | adler;
      exr_put_le(p.out + p.hdr_len + 8ull * i, off, 8u);
      exr_put_le(p.out + off, i * p.lpb, 4u);
      exr_put_le(p.out + off + 4u, size, 4u);
    }
    __syncthreads();
    if (t == 255u) running += s[255];
    __syncthreads();
  }
  if (t == 0) p.blk[2u * p.n_blocks] = running;
}

struct ExrPackP {
  const uint32_t *meta, *chunk_off;
  const uint64_t *blk;
  const uint8_t *scratch;
  size_t slot_bytes;
  uint32_t cps, cb, form;
  uint8_t *out;
};

__global__ void __launch_bounds__(256) k_exr_pack(ExrPackP p, ExrRowsP r) {
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  const uint32_t b = k / p.cps, j = k - b * p.cps;
  const uint32_t n_b = min(r.lpb, r.h - b * r.lpb) * r.line_bytes;
  const uint32_t q0 = j * p.cb, n = min(p.cb, n_b - q0);
  const uint64_t rec = p.blk[2u * b + 1u];
  const uint32_t size = (uint32_t)(rec >> 32);
  uint8_t *dst = p.out + p.blk[2u * b] + 8u;
  if (size < n_b) {
    const uint32_t L = p.meta[(size_t)k * DEFLATE_META];
    const uint8_t *src = p.scratch + (size_t)k * p.slot_bytes;
    dst += p.chunk_off[k];
    for (uint32_t i = t; i < L; i += 256u) dst[i] = src[i];
    if (q0 + n == n_b && t < 4u) dst[L + t] = (uint8_t)((uint32_t)rec >> (24u - 8u * t)); // the Adler-32, big-endian
  } else if (p.form) {
    const uint8_t *src = r.raw + (size_t)b * r.raw_stride + r.raw_skip + q0;
    for (uint32_t i = t; i < n; i += 256u) dst[q0 + i] = src[i];
  } else {
    for (uint32_t i = t; i < n; i += 256u) dst[q0 + i] = (uint8_t)exr_raw_byte(r, b, q0 + i);
  }
}

int g_exr_form = 0;

struct HdrWriter {
  uint8_t *d;
  uint32_t n = 0;
  bool full = false; // something did not fit EXR_HEADER_MAX: nothing is written past it
  void bytes(const void *s, uint32_t k) {
    if (full || k > EXR_HEADER_MAX - n) { full = true; return; }
    std::memcpy(d + n, s, k); n += k;
  }
  void u8(uint32_t v) { const uint8_t b = (uint8_t)v; bytes(&b, 1u); }
  void i32(uint32_t v) { for (int i = 0; i < 4; ++i) u8(v >> (8 * i)); }
  void f32(float f) { uint32_t v; std::memcpy(&v, &f, 4); i32(v); }
  void str(const char *s) { bytes(s, (uint32_t)std::strlen(s) + 1u); }
  void attr(const char *name, const char *type, uint32_t size) { str(name); str(type); i32(size); }
};

const fspt_exr_params EXR_DEFAULTS = {(uint32_t)FSPT_EXR_ZIP, (uint32_t)FSPT_EXR_HALF, 0u, FSPT_EXR_CHUNK};

} // namespace

int exr_plan(const fspt_exr_params *prm, uint32_t w, uint32_t h, bool for_device, const char *fn, ExrPlan &pl) {
  const fspt_exr_params q = prm ? *prm : EXR_DEFAULTS;
  if (w == 0 || h == 0 || w > 65535u || h > 65535u) { fspt_set_error("%s: width and height must be in 1..65535", fn); return FSPT_E_INVALID; }
  if (q.compression != (uint32_t)FSPT_EXR_NONE && q.compression != (uint32_t)FSPT_EXR_ZIPS && q.compression != (uint32_t)FSPT_EXR_ZIP) { fspt_set_error("%s: unknown compression %u", fn, q.compression); return FSPT_E_INVALID; }
  if (q.pixel_type != (uint32_t)FSPT_EXR_HALF && q.pixel_type != (uint32_t)FSPT_EXR_FLOAT) { fspt_set_error("%s: unknown pixel type %u", fn, q.pixel_type); return FSPT_E_INVALID; }
  if (q.layers & ~15u) { fspt_set_error("%s: unknown layer bits 0x%x", fn, q.layers); return FSPT_E_INVALID; }
  if (q.chunk_bytes != 0u && (q.chunk_bytes < DEFLATE_CHUNK_MIN || q.chunk_bytes > DEFLATE_CHUNK_MAX)) { fspt_set_error("%s: chunk_bytes must be 0 or in 256..32768", fn); return FSPT_E_INVALID; }
  pl = ExrPlan{};
  pl.w = w; pl.h = h; pl.compression = q.compression; pl.pixel_type = q.pixel_type; pl.layers = q.layers;
  pl.cb = q.chunk_bytes ? q.chunk_bytes : FSPT_EXR_CHUNK;
  pl.form = (uint32_t)g_exr_form;
  // the channels in the order of their names' bytes; src: the rgba float, or 4 + the feature float (albedo rgb, t, normal xyz, hit)
  static const struct { const char *name; uint32_t layer, src; bool is_float; } ALL[EXR_MAX_CHANNELS] = {
      {"A", FSPT_EXR_ALPHA, 3u, false}, {"B", 0u, 2u, false}, {"G", 0u, 1u, false}, {"N.X", FSPT_EXR_NORMAL, 8u, false}, {"N.Y", FSPT_EXR_NORMAL, 9u, false},
      {"N.Z", FSPT_EXR_NORMAL, 10u, false}, {"R", 0u, 0u, false}, {"Z", FSPT_EXR_DEPTH, 7u, true}, {"albedo.B", FSPT_EXR_ALBEDO, 6u, false},
      {"albedo.G", FSPT_EXR_ALBEDO, 5u, false}, {"albedo.R", FSPT_EXR_ALBEDO, 4u, false}};
  HdrWriter hw{pl.hdr};
  const uint8_t magic[8] = {0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0};
  hw.bytes(magic, 8);
  uint32_t chl = 1u;
  for (const auto &c : ALL) if (!c.layer || (q.layers & c.layer)) chl += (uint32_t)std::strlen(c.name) + 1u + 16u;
  hw.attr("channels", "chlist", chl);
  for (const auto &c : ALL) {
    if (c.layer && !(q.layers & c.layer)) continue;
    const uint32_t type = c.is_float ? (uint32_t)FSPT_EXR_FLOAT : q.pixel_type;
    pl.ch[pl.n_ch++] = ExrChannel{c.src, type == (uint32_t)FSPT_EXR_HALF ? 2u : 4u, pl.px_bytes};
    pl.px_bytes += type == (uint32_t)FSPT_EXR_HALF ? 2u : 4u;
    hw.str(c.name); hw.i32(type); hw.i32(0u); hw.i32(1u); hw.i32(1u);
  }
  hw.u8(0);
  hw.attr("compression", "compression", 1u); hw.u8(q.compression);
  hw.attr("dataWindow", "box2i", 16u); hw.i32(0); hw.i32(0); hw.i32(w - 1u); hw.i32(h - 1u);
  hw.attr("displayWindow", "box2i", 16u); hw.i32(0); hw.i32(0); hw.i32(w - 1u); hw.i32(h - 1u);
  hw.attr("lineOrder", "lineOrder", 1u); hw.u8(0);
  hw.attr("pixelAspectRatio", "float", 4u); hw.f32(1.0f);
  hw.attr("screenWindowCenter", "v2f", 8u); hw.f32(0.0f); hw.f32(0.0f);
  hw.attr("screenWindowWidth", "float", 4u); hw.f32(1.0f);
  hw.u8(0);
  if (hw.full) { fspt_set_error("%s: the header does not fit %u bytes", fn, EXR_HEADER_MAX); return FSPT_E_INVALID; } // (a longer channel list: raise EXR_HEADER_MAX)
  pl.hdr_len = hw.n;
  pl.lpb = q.compression == (uint32_t)FSPT_EXR_ZIP ? 16u : 1u;
  pl.n_blocks = (h + pl.lpb - 1u) / pl.lpb;
  pl.line_bytes = (size_t)w * pl.px_bytes;
  pl.block_bytes = pl.line_bytes * pl.lpb;
  pl.data_bytes = pl.line_bytes * h;
  pl.bound = pl.hdr_len + (size_t)pl.n_blocks * 16u + pl.data_bytes; // (a block is never longer than its raw bytes)
  if (for_device && pl.bound > 0xFFFFFFFFull) { fspt_set_error("%s: a file of %u x %u with these channels could pass 4 GiB", fn, w, h); return FSPT_E_INVALID; }
  // no chunk is longer than a block: the slots and the deflate's LDS are sized by what a workgroup can get (a ZIPS scanline is
  // often far below the chunk size); the file's bytes do not depend on it
  pl.cb = (uint32_t)std::min<size_t>(pl.cb, pl.block_bytes);
  pl.cps = (uint32_t)((pl.block_bytes + pl.cb - 1u) / pl.cb);
  const size_t last = pl.data_bytes - (size_t)(pl.n_blocks - 1u) * pl.block_bytes;
  pl.n_chunks = (pl.n_blocks - 1u) * pl.cps + (uint32_t)((last + pl.cb - 1u) / pl.cb);
  pl.slot_bytes = deflate_slot_bytes(pl.cb);
  return FSPT_OK;
}

static bool same_plan(const ExrPlan &a, const ExrPlan &b) {
  return a.w == b.w && a.h == b.h && a.compression == b.compression && a.pixel_type == b.pixel_type && a.layers == b.layers && a.cb == b.cb && a.form == b.form;
}

hipError_t exr_ensure(ExrEnc &e, const ExrPlan &pl, size_t out_bytes) {
  hipError_t err = enc_ensure_out(e.c, 1, out_bytes);
  if (err != hipSuccess || (e.c.valid && same_plan(e.pl, pl))) return err;
  enc_replan(e.c);
  const bool z = pl.compression != (uint32_t)FSPT_EXR_NONE;
  enc_make(e.c, err, e.cfg, EXR_HEADER_MAX + sizeof pl.ch);
  enc_make(e.c, err, e.blk, ((size_t)pl.n_blocks * 2u + 1u) * 8u);
  enc_make(e.c, err, e.stream, pl.data_bytes + 8u, z);
  enc_make(e.c, err, e.raw, pl.data_bytes + 8u, z && pl.form);
  enc_make(e.c, err, e.scratch, (size_t)pl.n_chunks * pl.slot_bytes, z);
  enc_make(e.c, err, e.meta, (size_t)pl.n_chunks * (DEFLATE_META + 1u) * 4u, z);
  e.chunk_off = e.meta ? e.meta + (size_t)pl.n_chunks * DEFLATE_META : nullptr;
  if (err == hipSuccess) err = hipMemcpy(e.cfg, pl.hdr, pl.hdr_len, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(e.cfg + EXR_HEADER_MAX, pl.ch, sizeof pl.ch, hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  e.pl = pl; e.c.valid = true;
  return hipSuccess;
}

// The whole encode into e.c.out[0] on `st`; the file's length lands in e.blk[2 n_blocks].  Events 0..3 bracket the three stages.
hipError_t exr_launch(ExrEnc &e, const float4 *rgba, const float4 *feat, int bottom_up, hipStream_t st) {
  const ExrPlan &pl = e.pl;
  const bool z = pl.compression != (uint32_t)FSPT_EXR_NONE;
  uint8_t *const out = e.c.out[0];
  ExrRowsP r{};
  r.rgba = (const uint4 *)rgba; r.feat = (const uint4 *)feat;
  r.w = pl.w; r.h = pl.h; r.bottom_up = bottom_up ? 1u : 0u; r.n_ch = pl.n_ch; r.lpb = pl.lpb;
  r.predicted = z ? 1u : 0u; r.keep_raw = !z || pl.form ? 1u : 0u;
  r.line_bytes = (uint32_t)pl.line_bytes; r.block_bytes = (uint32_t)pl.block_bytes;
  r.ch = (const ExrChannel *)(e.cfg + EXR_HEADER_MAX);
  r.stream = e.stream;
  if (z) { r.raw = e.raw; r.raw_stride = pl.block_bytes; r.raw_skip = 0; }
  else { r.raw = out; r.raw_stride = pl.line_bytes + 8u; r.raw_skip = (size_t)pl.hdr_len + 8u * (size_t)pl.n_blocks + 8u; } // straight into the file
  hipError_t err = hipEventRecord(e.c.ev[0], st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_exr_rows, dim3((pl.w + EXR_RT - 1u) / EXR_RT, pl.h), dim3(EXR_RT), 0, st, r);
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[1], st);
  if (err == hipSuccess && z) {
    const DeflateP d{e.stream, pl.data_bytes, pl.block_bytes, pl.cb, pl.cps, 0u, e.scratch, pl.slot_bytes, e.meta}; // a segment per block
    err = deflate_launch(d, pl.n_chunks, st);
  }
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[2], st);
  if (err != hipSuccess) return err;
  const ExrOffP o{e.meta, e.cfg, pl.hdr_len, pl.n_blocks, pl.cps, pl.cb, pl.lpb, pl.h, (uint32_t)pl.line_bytes, z ? 1u : 0u, e.chunk_off, e.blk, out};
  hipLaunchKernelGGL(k_exr_offsets, dim3(1), dim3(256), 0, st, o);
  if (z) {
    const ExrPackP k{e.meta, e.chunk_off, e.blk, e.scratch, pl.slot_bytes, pl.cps, pl.cb, pl.form, out};
    hipLaunchKernelGGL(k_exr_pack, dim3(pl.n_chunks), dim3(256), 0, st, k, r);
  }
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[3], st);
  return err;
}

int exr_collect(ExrEnc &e, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn) {
  return enc_collect(e.blk + 2u * (size_t)e.pl.n_blocks, e.c.out[0], out, cap, bytes_out, st, fn, g_exr_format);
}

} // namespace fspt

// The stand-alone entries: NULL and range checks first, then the device.
static int exr_encode_any(const char *fn, int device, const float *rgba, const float *features, bool on_device, uint32_t w, uint32_t h, int bottom_up,
                          const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  if (!rgba || !out || !bytes_out) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  fspt::ExrPlan pl;
  const int rc = fspt::exr_plan(p, w, h, true, fn, pl);
  if (rc) return rc;
  const bool guided = (pl.layers & ((uint32_t)FSPT_EXR_ALBEDO | (uint32_t)FSPT_EXR_NORMAL | (uint32_t)FSPT_EXR_DEPTH)) != 0u;
  if (guided && !features) { fspt_set_error("%s: feature layers need the features", fn); return FSPT_E_INVALID; }
  fspt::ExrEnc e;
  const auto launch = [&](fspt::Hold &hold) {
    const size_t px = (size_t)w * h;
    const float4 *src = (const float4 *)rgba, *feat = guided ? (const float4 *)features : nullptr;
    hipError_t err = hipSuccess;
    if (!on_device) { // one buffer: the radiance, the features behind it
      void *d = nullptr;
      err = hold.make(&d, px * (guided ? 48u : 16u));
      if (err == hipSuccess) err = hipMemcpy(d, rgba, px * 16u, hipMemcpyHostToDevice);
      if (err == hipSuccess && guided) err = hipMemcpy((char *)d + px * 16u, features, px * 32u, hipMemcpyHostToDevice);
      src = (const float4 *)d; feat = guided ? src + px : nullptr;
    }
    if (err == hipSuccess) err = fspt::exr_launch(e, src, feat, bottom_up, nullptr);
    return err;
  };
  return fspt::enc_run(fn, device, e.c, fspt::g_exr_format, [&] { return fspt::exr_ensure(e, pl, pl.bound); }, launch,
                       [&] { return fspt::exr_collect(e, nullptr, out, cap, bytes_out, fn); });
}

extern "C" {

int fspt_exr_bound(uint32_t w, uint32_t h, const fspt_exr_params *p, size_t *bytes) {
  return fspt::enc_bound<fspt::ExrPlan>("fspt_exr_bound", bytes, [&](fspt::ExrPlan &pl) { return fspt::exr_plan(p, w, h, false, "fspt_exr_bound", pl); });
}

int fspt_exr_encode(int device, const float *rgba, const float *features, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return exr_encode_any("fspt_exr_encode", device, rgba, features, false, w, h, bottom_up, p, out, cap, bytes_out);
}

int fspt_exr_encode_device(int device, const float *rgba, const float *features, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return exr_encode_any("fspt_exr_encode_device", device, rgba, features, true, w, h, bottom_up, p, out, cap, bytes_out);
}

int fspt_exr_set_form(int form) {
  if (form != 0 && form != 1) { fspt_set_error("fspt_exr_set_form: form must be 0 or 1"); return FSPT_E_INVALID; }
  fspt::g_exr_form = form;
  return FSPT_OK;
}

int fspt_exr_last_ms(float ms[3], uint64_t *bus_bytes) { return fspt::enc_last_ms(fspt::g_exr_format, "fspt_exr_last_ms", ms, bus_bytes); }

} // extern "C"
