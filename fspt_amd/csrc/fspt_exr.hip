// fspt_exr.hip - an OpenEXR encoder on the GPU: scene-linear radiance (W*H float4) and, for the feature layers,
// the first-hit guides (W*H x 2 float4) become a single-part scanline OpenEXR 2 file in device memory, so that only the file's
// bytes cross the bus.  Integer arithmetic throughout (the half conversion included: no denormal mode takes part); the bytes
// are tests/exr_ref.py's, which states the format.
//   k_exr_rows<MATTES>  one lane per pixel of a scanline: every channel's value canonicalised and converted, then its bytes
//                   written where the block's reordered and predicted stream has them - the even bytes of a block in its
//                   first half, the odd ones behind them, each minus the byte to its left in that order, which is a byte of
//                   the value before it (the neighbouring pixel, the end of the channel before, the end of the scanline
//                   before; at the seam the block's last even byte).  Compression none: the planar bytes into the file.
//                   MATTES (chosen only by a plan with a Cryptomatte layer): up to 35 channels, the 24 rank
//                   floats of the two kinds among them; a channel's three values are fetched by its source float, a
//                   wave-uniform choice among the four buffers, where the other instantiation keeps the pixel in registers.
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
  const uint32_t *rank_o, *rank_m; // the object / material ranks, 12 floats per pixel (named, not an array: see `ch`)
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

// source float `src` of pixel i, whichever buffer holds it (src is the same for the whole wave: a scalar branch)
__device__ __forceinline__ uint32_t exr_word(const ExrRowsP &p, uint32_t src, size_t i) {
  if (src < 4u) return ((const uint32_t *)p.rgba)[4u * i + src];
  if (src < 12u) return ((const uint32_t *)p.feat)[8u * i + src - 4u];
  return src < 24u ? p.rank_o[12u * i + src - 12u] : p.rank_m[12u * i + src - 24u];
}

// A pixel as the rows kernel holds it.  Without mattes: its twelve floats in registers, picked by exr_sel.  With them:
// its index, and a load per channel (48 floats in registers three times over would leave no room for anything else).
template <bool MATTES> struct ExrAt;
template <> struct ExrAt<false> {
  ExrPx q;
  __device__ __forceinline__ ExrAt(const ExrRowsP &p, uint32_t x, uint32_t y) : q(exr_load(p, x, y)) {}
  __device__ __forceinline__ uint32_t get(const ExrRowsP &, uint32_t src) const { return exr_sel(q, src); }
};
template <> struct ExrAt<true> {
  size_t i;
  __device__ __forceinline__ ExrAt(const ExrRowsP &p, uint32_t x, uint32_t y) : i((size_t)(p.bottom_up ? p.h - 1u - y : y) * p.w + x) {}
  __device__ __forceinline__ uint32_t get(const ExrRowsP &p, uint32_t src) const { return exr_word(p, src, i); }
};

template <bool MATTES>
__global__ void __launch_bounds__(EXR_RT) k_exr_rows(ExrRowsP p) {
  const uint32_t x = blockIdx.x * EXR_RT + threadIdx.x, y = blockIdx.y;
  if (x >= p.w) return;
  const uint32_t b = y / p.lpb, l = y - b * p.lpb;
  const uint32_t lines = min(p.lpb, p.h - b * p.lpb), half = lines * p.line_bytes / 2u; // (every value has 2 or 4 bytes: a block's length is even)
  // the value before this one in the block's order: the pixel to the left in the same channel; for the first pixel the last
  // pixel of the channel before; for the first channel that of the last channel of the scanline before; and for the block's
  // first value, at the seam of the two halves, the block's last value.  (wrap: one address for the whole wave.)
  const ExrAt<MATTES> cur(p, x, y);
  const ExrAt<MATTES> left(p, x ? x - 1u : p.w - 1u, y);
  const ExrAt<MATTES> wrap(p, p.w - 1u, l ? y - 1u : b * p.lpb + lines - 1u);
  uint8_t *t = p.stream + (size_t)b * p.block_bytes;
  uint8_t *r = p.raw + (size_t)b * p.raw_stride + p.raw_skip;
  for (uint32_t c = 0; c < p.n_ch; ++c) {
    const ExrChannel ch = p.ch[c];
    const uint32_t v = exr_conv(cur.get(p, ch.src), ch.bytes);
    const uint32_t q = l * p.line_bytes + ch.off * p.w + x * ch.bytes; // the value's first byte in the raw block
    if (p.keep_raw) {
      r[q] = (uint8_t)v; r[q + 1u] = (uint8_t)(v >> 8);
      if (ch.bytes == 4u) { r[q + 2u] = (uint8_t)(v >> 16); r[q + 3u] = (uint8_t)(v >> 24); }
    }
    if (!p.predicted) continue;
    uint32_t pe, po;
    if (x) { const uint32_t u = exr_conv(left.get(p, ch.src), ch.bytes); pe = exr_last_even(u, ch.bytes); po = exr_last_odd(u, ch.bytes); }
    else {
      const ExrChannel pc = p.ch[c ? c - 1u : p.n_ch - 1u];
      const uint32_t u = exr_conv(c ? left.get(p, pc.src) : wrap.get(p, pc.src), pc.bytes);
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
  return (exr_conv(exr_word(p, ch.src, i), ch.bytes) >> (8u * k)) & 255u;
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
  std::vector<uint8_t> &d; // the plan's header: as long as its channels and attributes make it
  void bytes(const void *s, size_t k) { d.insert(d.end(), (const uint8_t *)s, (const uint8_t *)s + k); }
  void u8(uint32_t v) { const uint8_t b = (uint8_t)v; bytes(&b, 1u); }
  void i32(uint32_t v) { for (int i = 0; i < 4; ++i) u8(v >> (8 * i)); }
  void f32(float f) { uint32_t v; std::memcpy(&v, &f, 4); i32(v); }
  void str(const char *s) { bytes(s, (uint32_t)std::strlen(s) + 1u); }
  void attr(const char *name, const char *type, uint32_t size) { str(name); str(type); i32(size); }
};

const fspt_exr_params EXR_DEFAULTS = {(uint32_t)FSPT_EXR_ZIP, (uint32_t)FSPT_EXR_HALF, 0u, FSPT_EXR_CHUNK};

} // namespace

int exr_plan(const fspt_exr_params *prm, uint32_t w, uint32_t h, bool for_device, const char *fn, ExrPlan &pl, bool crypto, const ExrMattes *mt) {
  const fspt_exr_params q = prm ? *prm : EXR_DEFAULTS;
  if (w == 0 || h == 0 || w > 65535u || h > 65535u) { fspt_set_error("%s: width and height must be in 1..65535", fn); return FSPT_E_INVALID; }
  if (q.compression != (uint32_t)FSPT_EXR_NONE && q.compression != (uint32_t)FSPT_EXR_ZIPS && q.compression != (uint32_t)FSPT_EXR_ZIP) { fspt_set_error("%s: unknown compression %u", fn, q.compression); return FSPT_E_INVALID; }
  if (q.pixel_type != (uint32_t)FSPT_EXR_HALF && q.pixel_type != (uint32_t)FSPT_EXR_FLOAT) { fspt_set_error("%s: unknown pixel type %u", fn, q.pixel_type); return FSPT_E_INVALID; }
  const uint32_t crypto_bits = (uint32_t)FSPT_EXR_CRYPTO_OBJECT | (uint32_t)FSPT_EXR_CRYPTO_MATERIAL;
  if (q.layers & ~(crypto ? 15u | crypto_bits : 15u)) { fspt_set_error("%s: unknown layer bits 0x%x", fn, q.layers); return FSPT_E_INVALID; }
  if (q.chunk_bytes != 0u && (q.chunk_bytes < DEFLATE_CHUNK_MIN || q.chunk_bytes > DEFLATE_CHUNK_MAX)) { fspt_set_error("%s: chunk_bytes must be 0 or in 256..32768", fn); return FSPT_E_INVALID; }
  for (int k = 0; k < 2 && mt; ++k)
    if ((q.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT << k)) && (mt->manifest_len[k] > EXR_MANIFEST_MAX || (mt->manifest_len[k] && !mt->manifest[k]))) {
      fspt_set_error("%s: manifest %d must be at most %u bytes, and not NULL when it has a length", fn, k, EXR_MANIFEST_MAX);
      return FSPT_E_INVALID;
    }
  pl = ExrPlan{};
  pl.w = w; pl.h = h; pl.compression = q.compression; pl.pixel_type = q.pixel_type; pl.layers = q.layers;
  pl.cb = q.chunk_bytes ? q.chunk_bytes : FSPT_EXR_CHUNK;
  pl.form = (uint32_t)g_exr_form;
  // the channels in the order of their names' bytes; src: the rgba float, or 4 + the feature float (albedo rgb, t, normal xyz, hit)
  // (the Cryptomatte levels, DESIGN 8.25: R G B A of level j = rank floats 4j .. 4j + 3, material 24.., object 12.., always FLOAT)
#define EXR_CRYPTO_LEVEL(name, layer, base) {name ".A", layer, (base) + 3u, true}, {name ".B", layer, (base) + 2u, true}, {name ".G", layer, (base) + 1u, true}, {name ".R", layer, (base), true}
  static const struct { const char *name; uint32_t layer, src; bool is_float; } ALL[EXR_MAX_CHANNELS] = {
      {"A", FSPT_EXR_ALPHA, 3u, false}, {"B", 0u, 2u, false},
      EXR_CRYPTO_LEVEL("CryptoMaterial00", FSPT_EXR_CRYPTO_MATERIAL, 24u), EXR_CRYPTO_LEVEL("CryptoMaterial01", FSPT_EXR_CRYPTO_MATERIAL, 28u), EXR_CRYPTO_LEVEL("CryptoMaterial02", FSPT_EXR_CRYPTO_MATERIAL, 32u),
      EXR_CRYPTO_LEVEL("CryptoObject00", FSPT_EXR_CRYPTO_OBJECT, 12u), EXR_CRYPTO_LEVEL("CryptoObject01", FSPT_EXR_CRYPTO_OBJECT, 16u), EXR_CRYPTO_LEVEL("CryptoObject02", FSPT_EXR_CRYPTO_OBJECT, 20u),
      {"G", 0u, 1u, false}, {"N.X", FSPT_EXR_NORMAL, 8u, false}, {"N.Y", FSPT_EXR_NORMAL, 9u, false},
      {"N.Z", FSPT_EXR_NORMAL, 10u, false}, {"R", 0u, 0u, false}, {"Z", FSPT_EXR_DEPTH, 7u, true}, {"albedo.B", FSPT_EXR_ALBEDO, 6u, false},
      {"albedo.G", FSPT_EXR_ALBEDO, 5u, false}, {"albedo.R", FSPT_EXR_ALBEDO, 4u, false}};
#undef EXR_CRYPTO_LEVEL
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
  // Cryptomatte's metadata, a kind's four attributes under the first seven hex digits of its layer name's hash: the
  // attributes stay in the byte order of their names (object 3ae39a5, material be359d6)
  for (int k = 0; k < 2; ++k) {
    if (!(q.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT << k))) continue;
    const char *layer = k == FSPT_MATTE_OBJECT ? "CryptoObject" : "CryptoMaterial";
    char key[16], name[48];
    std::snprintf(key, sizeof key, "%08x", fspt_matte_hash(layer, std::strlen(layer)));
    key[7] = 0;
    const auto text = [&](const char *what, const char *v, size_t n) {
      std::snprintf(name, sizeof name, "cryptomatte/%s/%s", key, what);
      hw.attr(name, "string", (uint32_t)n); hw.bytes(v, n);
    };
    text("conversion", "uint32_to_float32", 17u);
    text("hash", "MurmurHash3_32", 14u);
    if (mt && mt->manifest_len[k]) text("manifest", mt->manifest[k], mt->manifest_len[k]);
    text("name", layer, std::strlen(layer));
  }
  hw.attr("dataWindow", "box2i", 16u); hw.i32(0); hw.i32(0); hw.i32(w - 1u); hw.i32(h - 1u);
  hw.attr("displayWindow", "box2i", 16u); hw.i32(0); hw.i32(0); hw.i32(w - 1u); hw.i32(h - 1u);
  hw.attr("lineOrder", "lineOrder", 1u); hw.u8(0);
  hw.attr("pixelAspectRatio", "float", 4u); hw.f32(1.0f);
  hw.attr("screenWindowCenter", "v2f", 8u); hw.f32(0.0f); hw.f32(0.0f);
  hw.attr("screenWindowWidth", "float", 4u); hw.f32(1.0f);
  hw.u8(0);
  pl.hdr_len = (uint32_t)pl.hdr.size();
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
  return a.w == b.w && a.h == b.h && a.compression == b.compression && a.pixel_type == b.pixel_type && a.layers == b.layers && a.cb == b.cb && a.form == b.form &&
         a.hdr == b.hdr; // (the manifests are a part of the header)
}

hipError_t exr_ensure(ExrEnc &e, const ExrPlan &pl, size_t out_bytes) {
  hipError_t err = enc_ensure_out(e.c, 1, out_bytes);
  if (err != hipSuccess || (e.c.valid && same_plan(e.pl, pl))) return err;
  enc_replan(e.c);
  const bool z = pl.compression != (uint32_t)FSPT_EXR_NONE;
  const size_t ch_at = ((size_t)pl.hdr_len + 15u) & ~(size_t)15u; // the channels behind the header
  enc_make(e.c, err, e.cfg, ch_at + sizeof pl.ch);
  enc_make(e.c, err, e.blk, ((size_t)pl.n_blocks * 2u + 1u) * 8u);
  enc_make(e.c, err, e.stream, pl.data_bytes + 8u, z);
  enc_make(e.c, err, e.raw, pl.data_bytes + 8u, z && pl.form);
  enc_make(e.c, err, e.scratch, (size_t)pl.n_chunks * pl.slot_bytes, z);
  enc_make(e.c, err, e.meta, (size_t)pl.n_chunks * (DEFLATE_META + 1u) * 4u, z);
  e.chunk_off = e.meta ? e.meta + (size_t)pl.n_chunks * DEFLATE_META : nullptr;
  if (err == hipSuccess) err = hipMemcpy(e.cfg, pl.hdr.data(), pl.hdr_len, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(e.cfg + ch_at, pl.ch, sizeof pl.ch, hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  e.pl = pl; e.c.valid = true;
  return hipSuccess;
}

// The whole encode into e.c.out[0] on `st`; the file's length lands in e.blk[2 n_blocks].  Events 0..3 bracket the three stages.
hipError_t exr_launch(ExrEnc &e, const float4 *rgba, const float4 *feat, int bottom_up, hipStream_t st, const ExrMattes *mt) {
  const ExrPlan &pl = e.pl;
  const bool z = pl.compression != (uint32_t)FSPT_EXR_NONE;
  uint8_t *const out = e.c.out[0];
  ExrRowsP r{};
  r.rgba = (const uint4 *)rgba; r.feat = (const uint4 *)feat;
  const bool mattes = (pl.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT | (uint32_t)FSPT_EXR_CRYPTO_MATERIAL)) != 0u;
  if (mattes) {
    if (!mt) return hipErrorInvalidValue;
    r.rank_o = (pl.layers & (uint32_t)FSPT_EXR_CRYPTO_OBJECT) ? (const uint32_t *)mt->ranks[0] : nullptr;
    r.rank_m = (pl.layers & (uint32_t)FSPT_EXR_CRYPTO_MATERIAL) ? (const uint32_t *)mt->ranks[1] : nullptr;
    if (((pl.layers & (uint32_t)FSPT_EXR_CRYPTO_OBJECT) && !r.rank_o) || ((pl.layers & (uint32_t)FSPT_EXR_CRYPTO_MATERIAL) && !r.rank_m)) return hipErrorInvalidValue;
  }
  r.w = pl.w; r.h = pl.h; r.bottom_up = bottom_up ? 1u : 0u; r.n_ch = pl.n_ch; r.lpb = pl.lpb;
  r.predicted = z ? 1u : 0u; r.keep_raw = !z || pl.form ? 1u : 0u;
  r.line_bytes = (uint32_t)pl.line_bytes; r.block_bytes = (uint32_t)pl.block_bytes;
  r.ch = (const ExrChannel *)(e.cfg + (((size_t)pl.hdr_len + 15u) & ~(size_t)15u));
  r.stream = e.stream;
  if (z) { r.raw = e.raw; r.raw_stride = pl.block_bytes; r.raw_skip = 0; }
  else { r.raw = out; r.raw_stride = pl.line_bytes + 8u; r.raw_skip = (size_t)pl.hdr_len + 8u * (size_t)pl.n_blocks + 8u; } // straight into the file
  hipError_t err = hipEventRecord(e.c.ev[0], st);
  if (err != hipSuccess) return err;
  const dim3 rows_grid((pl.w + EXR_RT - 1u) / EXR_RT, pl.h);
  if (mattes) hipLaunchKernelGGL(k_exr_rows<true>, rows_grid, dim3(EXR_RT), 0, st, r);
  else hipLaunchKernelGGL(k_exr_rows<false>, rows_grid, dim3(EXR_RT), 0, st, r);
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

// a caller's fspt_exr_mattes as the plan and the launch take it (m NULL: nothing given)
static fspt::ExrMattes exr_mattes_of(const fspt_exr_mattes *m) {
  fspt::ExrMattes mt{};
  for (int k = 0; k < 2 && m; ++k) { mt.ranks[k] = (const float4 *)m->ranks[k]; mt.manifest[k] = m->manifest[k]; mt.manifest_len[k] = m->manifest_len[k]; }
  return mt;
}

// The stand-alone entries: NULL and range checks first, then the device.  crypto: the _mattes forms, which accept the
// Cryptomatte layer bits and need m's ranks for the kinds asked for.
static int exr_encode_any(const char *fn, int device, const float *rgba, const float *features, bool on_device, uint32_t w, uint32_t h, int bottom_up,
                          const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out, bool crypto = false, const fspt_exr_mattes *m = nullptr) {
  if (!rgba || !out || !bytes_out) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  fspt::ExrPlan pl;
  fspt::ExrMattes mt = exr_mattes_of(m);
  const int rc = fspt::exr_plan(p, w, h, true, fn, pl, crypto, &mt);
  if (rc) return rc;
  for (int k = 0; k < 2; ++k)
    if ((pl.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT << k)) && !mt.ranks[k]) { fspt_set_error("%s: matte layer %d needs its ranks", fn, k); return FSPT_E_INVALID; }
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
    for (int k = 0; k < 2 && !on_device; ++k) { // a kind's ranks, 12 floats per pixel, in a buffer of their own
      if (!(pl.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT << k))) continue;
      const void *d = nullptr;
      if (err == hipSuccess) err = fspt::enc_upload(hold, mt.ranks[k], px * 48u, &d);
      mt.ranks[k] = (const float4 *)d;
    }
    if (err == hipSuccess) err = fspt::exr_launch(e, src, feat, bottom_up, nullptr, &mt);
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

int fspt_exr_bound_mattes(uint32_t w, uint32_t h, const fspt_exr_params *p, const fspt_exr_mattes *m, size_t *bytes) {
  const fspt::ExrMattes mt = exr_mattes_of(m);
  return fspt::enc_bound<fspt::ExrPlan>("fspt_exr_bound_mattes", bytes, [&](fspt::ExrPlan &pl) { return fspt::exr_plan(p, w, h, false, "fspt_exr_bound_mattes", pl, true, &mt); });
}

int fspt_exr_encode_mattes(int device, const float *rgba, const float *features, const fspt_exr_mattes *m, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return exr_encode_any("fspt_exr_encode_mattes", device, rgba, features, false, w, h, bottom_up, p, out, cap, bytes_out, true, m);
}

int fspt_exr_encode_mattes_device(int device, const float *rgba, const float *features, const fspt_exr_mattes *m, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return exr_encode_any("fspt_exr_encode_mattes_device", device, rgba, features, true, w, h, bottom_up, p, out, cap, bytes_out, true, m);
}

int fspt_exr_set_form(int form) {
  if (form != 0 && form != 1) { fspt_set_error("fspt_exr_set_form: form must be 0 or 1"); return FSPT_E_INVALID; }
  fspt::g_exr_form = form;
  return FSPT_OK;
}

int fspt_exr_last_ms(float ms[3], uint64_t *bus_bytes) { return fspt::enc_last_ms(fspt::g_exr_format, "fspt_exr_last_ms", ms, bus_bytes); }

} // extern "C"
