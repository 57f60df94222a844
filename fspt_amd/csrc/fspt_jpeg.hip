// fspt_jpeg.hip - a baseline JPEG encoder on the GPU: the drawn RGBA8 frame, which draw_launch leaves in
// device memory, becomes a JFIF file there, so that only the file's bytes cross the bus.  Integer arithmetic throughout,
// libjpeg's (rgb_ycc_convert, h2v2_downsample, jpeg_fdct_islow, Annex K tables under its quality rule): the bytes are
// tests/jpeg_ref.py's, which are libjpeg's on the MCU grid.
//   k_jpeg_blocks<SUB>  colour conversion, 4:2:0 downsampling, both DCT passes, quantisation: int16 coefficients in zig-zag
//                       order, MCU-major.  One wave = 8 blocks; a lane is a row of its block, then, through LDS, a column.
//   k_jpeg_entropy      one wave per restart interval, 64 blocks at a time: lanes size their blocks, a wave scan gives bit
//                       offsets, the codes are OR-ed into an LDS bit buffer (disjoint bits: order does not matter), a
//                       ballot scan counts the 0xFF bytes, the stuffed bytes go to the interval's scratch slot.
//   k_jpeg_offsets      a scan of the interval lengths (each followed by a 2-byte marker): where every interval lands
//   k_jpeg_pack         header and intervals into one contiguous stream, RSTn between them, EOI, the byte count
#include "fspt_internal.hpp"
#include "fspt_encode_device.hpp"
#include "fspt_jpeg_tables.hpp"

namespace fspt {
namespace {

// The scratch slot of an interval is sized for the worst case.  A block's longest code, from the tables
// (JPEG_BLOCK_MAX_BITS, derived by tools/make_jpeg_tables.py): the chroma DC code of category 11 with its 11 bits (22),
// then 63 coefficients of run 0 and size 10 under a 16-bit code (63 x 26 = 1638; ZRL and EOB only replace coefficients):
// 1660 bits = 208 bytes rounded up, and every byte may be 0xFF and stuffed: 416.  Per interval one more (stuffed) pad byte.
static_assert(JPEG_BLOCK_MAX_BITS == 1660u, "the scratch sizing below is derived for these tables");
constexpr uint32_t JPEG_BLOCK_MAX_BYTES = 2u * ((JPEG_BLOCK_MAX_BITS + 7u) / 8u); // 416
constexpr uint32_t JPEG_INTERVAL_EXTRA = 4u;                                      // pad byte, stuffed; its marker is the packer's
constexpr uint32_t EN_CHUNK = 64u;                                                // blocks per pass of an entropy wave: one per lane
constexpr uint32_t EN_WORDS = (7u + EN_CHUNK * JPEG_BLOCK_MAX_BITS + 31u) / 32u + 7u; // bit buffer of a pass, the carried bits in front

// libjpeg's FIX(x) = (int)(x * 65536 + 0.5), evaluated by the compiler
constexpr int FIXC(double x) { return (int)(x * 65536.0 + 0.5); }
constexpr int C_Y_R = FIXC(.299), C_Y_G = FIXC(.587), C_Y_B = FIXC(.114), C_CB_R = FIXC(.16874), C_CB_G = FIXC(.33126), C_HALF = FIXC(.5),
              C_CR_G = FIXC(.41869), C_CR_B = FIXC(.08131);
static_assert(C_Y_R == 19595 && C_Y_G == 38470 && C_Y_B == 7471 && C_CB_R == 11059 && C_CB_G == 21709 && C_HALF == 32768 && C_CR_G == 27439 && C_CR_B == 5329, "rgb_ycc_convert");

struct JpegBlocksP {
  const uint32_t *rgba; // w x h texels
  uint32_t w, h, bottom_up;
  uint32_t mw, n_blocks;
  const uint16_t *q;    // [luma | chroma][64] divisors, natural order
  int16_t *coef;        // n_blocks x 64
};

// component comp (0 Y, 1 Cb, 2 Cr) of the texel at (x, y) of the top-down image extended by its last column and row
__device__ __forceinline__ int jpeg_sample(const JpegBlocksP &p, uint32_t x, uint32_t y, int comp) {
  x = min(x, p.w - 1u); y = min(y, p.h - 1u);
  const uint32_t row = p.bottom_up ? p.h - 1u - y : y;
  const uint32_t t = p.rgba[(size_t)row * p.w + x];
  const int R = (int)(t & 255u), G = (int)((t >> 8) & 255u), B = (int)((t >> 16) & 255u);
  if (comp == 0) return (C_Y_R * R + C_Y_G * G + C_Y_B * B + 32768) >> 16;
  if (comp == 1) return (-C_CB_R * R - C_CB_G * G + C_HALF * B + (128 << 16) + 32767) >> 16;
  return (C_HALF * R - C_CR_G * G - C_CR_B * B + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jpeg_fdct_islow's pass over 8 values: FIRST = the row pass (output scaled by 4), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int CB = 13, PB = 2, N = FIRST ? CB - PB : CB + PB;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) { d[0] = (t10 + t11) << PB; d[4] = (t10 - t11) << PB; }
  else { d[0] = descale(t10 + t11, PB); d[4] = descale(t10 - t11, PB); }
  int z1 = (t12 + t13) * 4433;
  d[2] = descale(z1 + t13 * 6270, N);
  d[6] = descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  d[7] = descale(t4 + z1 + z3, N); d[5] = descale(t5 + z2 + z4, N);
  d[3] = descale(t6 + z2 + z3, N); d[1] = descale(t7 + z1 + z4, N);
}

template <int SUB>
__global__ void __launch_bounds__(64) k_jpeg_blocks(JpegBlocksP p) {
  constexpr uint32_t BPM = SUB ? 6u : 3u;
  __shared__ int tile[8 * 72];                       // [block][row * 9 + column]: rows padded, no bank is hit twice
  __shared__ __attribute__((aligned(16))) int16_t zz[8 * 64];
  const uint32_t lane = threadIdx.x, blk = lane >> 3, r = lane & 7u;
  const uint32_t b = blockIdx.x * 8u + blk;
  const bool live = b < p.n_blocks;
  const uint32_t mcu = b / BPM, j = b - mcu * BPM;
  const uint32_t my = mcu / p.mw, mx = mcu - my * p.mw;
  const int comp = SUB ? (j < 4u ? 0 : (int)j - 3) : (int)j;
  int d[8];
  if (live) { // a lane = row r of its block
    if (SUB && comp) {
      const uint32_t y = my * 16u + 2u * r, x0 = mx * 16u;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t x = x0 + 2u * c;
        const int s = jpeg_sample(p, x, y, comp) + jpeg_sample(p, x + 1u, y, comp) + jpeg_sample(p, x, y + 1u, comp) + jpeg_sample(p, x + 1u, y + 1u, comp);
        d[c] = ((s + 1 + (c & 1)) >> 2) - 128;     // h2v2_downsample: bias 1, 2, 1, 2, ...
      }
    } else {
      const uint32_t y = SUB ? my * 16u + (j >> 1) * 8u + r : my * 8u + r, x0 = SUB ? mx * 16u + (j & 1u) * 8u : mx * 8u;
#pragma unroll
      for (int c = 0; c < 8; ++c) d[c] = jpeg_sample(p, x0 + c, y, comp) - 128;
    }
    fdct8<true>(d);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = 0;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) tile[blk * 72u + r * 9u + c] = d[c];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = tile[blk * 72u + k * 9u + r]; // the lane = column r of its block
  fdct8<false>(d);
  const uint16_t *q = p.q + (comp ? 64 : 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t nat = (uint32_t)k * 8u + r;
    const uint32_t qv = (uint32_t)q[nat] << 3;
    const uint32_t m = ((uint32_t)abs(d[k]) + (qv >> 1)) / qv; // an exact integer division
    zz[blk * 64u + JPEG_ZIGZAG_INV[nat]] = (int16_t)(d[k] < 0 ? -(int)m : (int)m);
  }
  __syncthreads();
  if (live) ((uint4 *)(p.coef + (size_t)blockIdx.x * 512u))[lane] = ((const uint4 *)zz)[lane]; // 8 coefficients per lane, 1 KiB per wave
}

struct JpegEntropyP {
  const int16_t *coef;
  uint32_t n_mcu, ri, bpm;
  uint8_t *scratch;
  size_t slot_bytes;
  uint32_t *len; // per interval: its stuffed bytes, padded
};

// A lane's writer into the LDS bit buffer: bit position p counts from the buffer's first bit, most significant first
struct BitSink {
  uint32_t *buf;
  uint32_t p, w, acc;
  __device__ __forceinline__ void put(uint32_t code, uint32_t len) { // len <= 26
    const uint64_t v = (uint64_t)code << (64u - (p & 31u) - len);
    acc |= (uint32_t)(v >> 32);
    p += len;
    if ((p >> 5) != w) { atomicOr(&buf[w], acc); acc = (uint32_t)v; ++w; }
  }
  __device__ __forceinline__ void flush() { if (acc) atomicOr(&buf[w], acc); }
};

// One block's code: its length in bits, and with EMIT the bits themselves.  pred: the DC it is predicted from.
template <bool EMIT>
__device__ __forceinline__ uint32_t jpeg_code_block(const int16_t *c, int pred, const uint32_t *dc, const uint32_t *ac, BitSink &sink) {
  uint32_t bits = 0, run = 0;
  auto sym = [&](uint32_t entry, int v, uint32_t nb) { // a Huffman code followed by the nb low bits of v (v - 1 when negative)
    const uint32_t len = (entry & 255u) + nb;
    bits += len;
    if (EMIT) sink.put(((entry >> 8) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), len);
  };
#pragma unroll 1
  for (uint32_t g = 0; g < 8u; ++g) {
    const uint4 q = ((const uint4 *)c)[g];
    const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const int v = (int)(int16_t)(wds[k >> 1] >> ((k & 1u) * 16u));
      if (g == 0 && k == 0) {
        const int diff = v - pred;
        const uint32_t nb = 32u - (uint32_t)__clz(abs(diff));
        sym(dc[min(nb, 11u)], diff, nb);
      } else if (v == 0) {
        ++run;
      } else {
        while (run > 15u) { sym(ac[0xF0], 0, 0); run -= 16u; }
        const uint32_t nb = 32u - (uint32_t)__clz(abs(v));
        sym(ac[((run << 4) | nb) & 255u], v, nb);
        run = 0;
      }
    }
  }
  if (run) sym(ac[0], 0, 0);
  return bits;
}

__global__ void __launch_bounds__(64) k_jpeg_entropy(JpegEntropyP p) {
  __shared__ uint32_t s_dc[2 * 12], s_ac[2 * 256], s_bits[EN_WORDS];
  const uint32_t lane = threadIdx.x;
  if (lane < 24u) s_dc[lane] = JPEG_DC_CODES[lane / 12u][lane % 12u];
  for (uint32_t i = lane; i < 512u; i += 64u) s_ac[i] = JPEG_AC_CODES[i >> 8][i & 255u];
  const uint32_t mcu0 = blockIdx.x * p.ri, mcus = min(p.ri, p.n_mcu - mcu0);
  const uint32_t nb = mcus * p.bpm;
  const size_t block0 = (size_t)mcu0 * p.bpm;
  uint8_t *dst = p.scratch + (size_t)blockIdx.x * p.slot_bytes;
  uint32_t out = 0;                      // bytes written (wave-uniform)
  uint32_t carry_bits = 0, carry_val = 0; // the bits of an unfinished byte, carried into the next pass
  auto byte_at = [&](uint32_t i) { return (s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u; };
  for (uint32_t base = 0; base < nb; base += EN_CHUNK) {
    __syncthreads();
    for (uint32_t i = lane; i < EN_WORDS; i += 64u) s_bits[i] = i == 0 ? carry_val << 24 : 0u;
    __syncthreads();
    const uint32_t i = base + lane;
    const bool live = i < nb;
    const uint32_t m = i / p.bpm, j = i - m * p.bpm;
    // the previous block of the same component in this interval
    uint32_t back = p.bpm == 3u ? 3u : j == 0u ? 3u : j < 4u ? 1u : 6u;
    const bool has_prev = p.bpm == 6u && j >= 1u && j < 4u ? true : m > 0u;
    const uint32_t tab = p.bpm == 3u ? (j > 0u) : (j >= 4u);
    const int16_t *c = p.coef + (block0 + (live ? i : 0u)) * 64u;
    const int pred = live && has_prev ? (int)c[-(int)(back * 64u)] : 0;
    BitSink sink{s_bits, 0, 0, 0};
    const uint32_t mine = live ? jpeg_code_block<false>(c, pred, s_dc + tab * 12u, s_ac + tab * 256u, sink) : 0u;
    uint32_t incl = mine; // the wave's inclusive scan
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) { const uint32_t o = __shfl_up(incl, s); if (lane >= s) incl += o; }
    const uint32_t total = carry_bits + __shfl(incl, 63);
    if (live) {
      sink.p = carry_bits + incl - mine; sink.w = sink.p >> 5;
      jpeg_code_block<true>(c, pred, s_dc + tab * 12u, s_ac + tab * 256u, sink);
      sink.flush();
    }
    __syncthreads();
    uint32_t nbytes = total >> 3;
    const uint32_t rem = total & 7u;
    const bool last = base + EN_CHUNK >= nb;
    if (last && rem) { // the interval ends: 1-bits to the byte
      if (lane == 0) s_bits[nbytes >> 2] |= ((1u << (8u - rem)) - 1u) << (24u - 8u * (nbytes & 3u));
      ++nbytes;
      __syncthreads();
    }
    for (uint32_t i0 = 0; i0 < nbytes; i0 += 64u) { // byte stuffing: a ballot counts the 0xFF bytes in front of a lane's
      const uint32_t k = i0 + lane;
      const bool have = k < nbytes;
      const uint32_t v = have ? byte_at(k) : 0u;
      const unsigned long long ff = __ballot(v == 255u);
      if (have) {
        uint8_t *o = dst + out + lane + __popcll(ff & ((1ull << lane) - 1ull));
        o[0] = (uint8_t)v;
        if (v == 255u) o[1] = 0;
      }
      out += min(64u, nbytes - i0) + (uint32_t)__popcll(ff);
    }
    carry_bits = last ? 0u : rem;
    carry_val = carry_bits ? byte_at(nbytes) & (0xFF00u >> carry_bits) & 255u : 0u;
  }
  if (lane == 0) p.len[blockIdx.x] = out;
}

// off[k] = hdr_len + sum over i < k of (len[i] + 2): an interval's bytes and the marker behind it; off[n] = the file's length
__global__ void __launch_bounds__(256) k_jpeg_offsets(const uint32_t *__restrict__ len, uint32_t n, uint32_t hdr_len, uint32_t *__restrict__ off) {
  __shared__ uint32_t s[256];
  __shared__ uint32_t running;
  const uint32_t t = threadIdx.x;
  if (t == 0) running = hdr_len;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 256u) {
    const uint32_t i = base + t;
    const uint32_t v = i < n ? len[i] + 2u : 0u;
    enc_scan256(s, v);
    const uint32_t r = running;
    if (i < n) off[i] = r + s[t] - v;
    __syncthreads();
    if (t == 255u) running = r + s[255];
    __syncthreads();
  }
  if (t == 0) off[n] = running;
}

__global__ void __launch_bounds__(256) k_jpeg_pack(const uint8_t *__restrict__ hdr, uint32_t hdr_len, const uint8_t *__restrict__ scratch, size_t slot_bytes,
                                                    const uint32_t *__restrict__ len, const uint32_t *__restrict__ off, uint32_t n, uint8_t *__restrict__ out) {
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  if (k == 0) for (uint32_t i = t; i < hdr_len; i += 256u) out[i] = hdr[i];
  const uint8_t *src = scratch + (size_t)k * slot_bytes;
  const uint32_t L = len[k];
  uint8_t *dst = out + off[k];
  for (uint32_t i = t; i < L; i += 256u) dst[i] = src[i];
  if (t == 0) { dst[L] = 0xFF; dst[L + 1u] = k + 1u == n ? 0xD9 : (uint8_t)(0xD0u + (k & 7u)); } // RSTn between intervals, EOI behind the last
}

void put_segment(std::vector<uint8_t> &o, uint8_t marker, const std::vector<uint8_t> &payload) {
  const size_t n = payload.size() + 2;
  o.push_back(0xFF); o.push_back(marker); o.push_back((uint8_t)(n >> 8)); o.push_back((uint8_t)n);
  o.insert(o.end(), payload.begin(), payload.end());
}

} // namespace

static const fspt_jpeg_params JPEG_DEFAULTS = {85u, (uint32_t)FSPT_JPEG_420, 0u};

int jpeg_check_params(const fspt_jpeg_params *prm, const char *fn) {
  const fspt_jpeg_params q = prm ? *prm : JPEG_DEFAULTS;
  if (q.quality < 1u || q.quality > 100u) { fspt_set_error("%s: quality must be in 1..100", fn); return FSPT_E_INVALID; }
  if (q.subsampling != (uint32_t)FSPT_JPEG_444 && q.subsampling != (uint32_t)FSPT_JPEG_420) { fspt_set_error("%s: unknown subsampling %u", fn, q.subsampling); return FSPT_E_INVALID; }
  if (q.restart_mcus > 65535u) { fspt_set_error("%s: restart_mcus must be at most 65535", fn); return FSPT_E_INVALID; }
  return FSPT_OK;
}

int jpeg_plan(const fspt_jpeg_params *prm, uint32_t w, uint32_t h, const char *fn, JpegPlan &pl) {
  const fspt_jpeg_params q = prm ? *prm : JPEG_DEFAULTS;
  if (w == 0 || h == 0 || w > 65535u || h > 65535u) { fspt_set_error("%s: width and height must be in 1..65535", fn); return FSPT_E_INVALID; }
  const int rc = jpeg_check_params(prm, fn);
  if (rc) return rc;
  pl = JpegPlan{};
  pl.w = w; pl.h = h; pl.quality = q.quality; pl.sub = q.subsampling;
  const uint32_t m = pl.sub ? 16u : 8u;
  pl.mw = (w + m - 1u) / m; pl.mh = (h + m - 1u) / m;
  pl.n_mcu = pl.mw * pl.mh;
  pl.bpm = pl.sub ? 6u : 3u;
  pl.ri = q.restart_mcus ? q.restart_mcus : pl.mw; // 0: one MCU row (at most 8192 MCUs)
  pl.n_int = (pl.n_mcu + pl.ri - 1u) / pl.ri;
  pl.n_blocks = (uint64_t)pl.n_mcu * pl.bpm;
  pl.slot_bytes = (size_t)std::min(pl.ri, pl.n_mcu) * pl.bpm * JPEG_BLOCK_MAX_BYTES + JPEG_INTERVAL_EXTRA;
  pl.bound = (size_t)JPEG_HEADER_BYTES + (size_t)pl.n_blocks * JPEG_BLOCK_MAX_BYTES + (size_t)pl.n_int * 4u + 2u;
  return FSPT_OK;
}

size_t jpeg_bound_max(uint32_t w, uint32_t h) {
  JpegPlan pl;
  const fspt_jpeg_params worst = {100u, (uint32_t)FSPT_JPEG_444, 1u}; // the most blocks and the most intervals
  jpeg_plan(&worst, w, h, "jpeg", pl);
  return pl.bound;
}

// SOI .. SOS as libjpeg lays them out: JFIF 1.01 without density units, the two DQT, SOF0, the four DHT, DRI, SOS
static void jpeg_header(const JpegPlan &pl, std::vector<uint8_t> &o, uint16_t q[128]) {
  const uint32_t s = pl.quality < 50u ? 5000u / pl.quality : 200u - 2u * pl.quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) q[t * 64 + k] = (uint16_t)std::min(std::max(((t ? JPEG_QUANT_CHROMA[k] : JPEG_QUANT_LUMA[k]) * s + 50u) / 100u, 1u), 255u);
  o.assign({0xFF, 0xD8});
  put_segment(o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    std::vector<uint8_t> s8{(uint8_t)t};
    for (int k = 0; k < 64; ++k) s8.push_back((uint8_t)q[t * 64 + JPEG_ZIGZAG[k]]);
    put_segment(o, 0xDB, s8);
  }
  const uint8_t hv = pl.sub ? 0x22 : 0x11;
  put_segment(o, 0xC0, {8, (uint8_t)(pl.h >> 8), (uint8_t)pl.h, (uint8_t)(pl.w >> 8), (uint8_t)pl.w, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
  auto dht = [&](uint8_t id, const uint8_t *bits, const uint8_t *vals, size_t n) {
    std::vector<uint8_t> s8{id};
    s8.insert(s8.end(), bits, bits + 16); s8.insert(s8.end(), vals, vals + n);
    put_segment(o, 0xC4, s8);
  };
  dht(0x00, JPEG_DC_LUMA_BITS, JPEG_DC_LUMA_VALS, sizeof JPEG_DC_LUMA_VALS); dht(0x10, JPEG_AC_LUMA_BITS, JPEG_AC_LUMA_VALS, sizeof JPEG_AC_LUMA_VALS);
  dht(0x01, JPEG_DC_CHROMA_BITS, JPEG_DC_CHROMA_VALS, sizeof JPEG_DC_CHROMA_VALS); dht(0x11, JPEG_AC_CHROMA_BITS, JPEG_AC_CHROMA_VALS, sizeof JPEG_AC_CHROMA_VALS);
  put_segment(o, 0xDD, {(uint8_t)(pl.ri >> 8), (uint8_t)pl.ri});
  put_segment(o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

static bool same_plan(const JpegPlan &a, const JpegPlan &b) {
  return a.w == b.w && a.h == b.h && a.quality == b.quality && a.sub == b.sub && a.ri == b.ri;
}

// The encoder's device memory for `pl`: the header and divisors once per (size, parameters), the work buffers, and n_out
// output buffers of out_bytes each (>= pl.bound; they outlive a change of the parameters).  Nothing of it may be in use.
hipError_t jpeg_ensure(JpegEnc &e, const JpegPlan &pl, int n_out, size_t out_bytes) {
  hipError_t err = enc_ensure_out(e.c, n_out, out_bytes);
  if (err != hipSuccess || (e.c.valid && same_plan(e.pl, pl))) return err;
  enc_replan(e.c);
  std::vector<uint8_t> hdr;
  uint16_t q[128];
  jpeg_header(pl, hdr, q);
  if (hdr.size() != JPEG_HEADER_BYTES) return hipErrorInvalidValue; // (fspt_jpeg_bound counts on it)
  const size_t blocks8 = ((size_t)pl.n_blocks + 7u) / 8u * 8u;      // k_jpeg_blocks stores whole waves of live blocks only; padded all the same
  enc_make(e.c, err, e.cfg, 256 + hdr.size());
  enc_make(e.c, err, e.coef, blocks8 * 128u);
  enc_make(e.c, err, e.scratch, (size_t)pl.n_int * pl.slot_bytes);
  enc_make(e.c, err, e.len, ((size_t)pl.n_int * 2u + 1u) * 4u);
  e.off = e.len ? e.len + pl.n_int : nullptr;
  if (err == hipSuccess) err = hipMemcpy(e.cfg, q, 256, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(e.cfg + 256, hdr.data(), hdr.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  e.pl = pl; e.c.valid = true;
  return hipSuccess;
}

hipError_t jpeg_launch_blocks(JpegEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st) {
  const JpegPlan &pl = e.pl;
  JpegBlocksP b{rgba, pl.w, pl.h, bottom_up ? 1u : 0u, pl.mw, (uint32_t)pl.n_blocks, (const uint16_t *)e.cfg, e.coef};
  const uint32_t grid = (uint32_t)((pl.n_blocks + 7u) / 8u);
  if (pl.sub) hipLaunchKernelGGL(k_jpeg_blocks<1>, dim3(grid), dim3(64), 0, st, b);
  else hipLaunchKernelGGL(k_jpeg_blocks<0>, dim3(grid), dim3(64), 0, st, b);
  return hipGetLastError();
}

// The whole encode of `rgba` (device memory, w x h texels) into e.c.out[slot] on `st`; the file's length lands in
// e.off[n_int].  Events 0..3 bracket the three stages.  No host read, no synchronisation.
hipError_t jpeg_launch(JpegEnc &e, const uint32_t *rgba, int bottom_up, int slot, hipStream_t st) {
  const JpegPlan &pl = e.pl;
  hipError_t err = hipEventRecord(e.c.ev[0], st);
  if (err == hipSuccess) err = jpeg_launch_blocks(e, rgba, bottom_up, st);
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[1], st);
  if (err != hipSuccess) return err;
  JpegEntropyP en{e.coef, pl.n_mcu, pl.ri, pl.bpm, e.scratch, pl.slot_bytes, e.len};
  hipLaunchKernelGGL(k_jpeg_entropy, dim3(pl.n_int), dim3(64), 0, st, en);
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[2], st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_jpeg_offsets, dim3(1), dim3(256), 0, st, (const uint32_t *)e.len, pl.n_int, JPEG_HEADER_BYTES, e.off);
  hipLaunchKernelGGL(k_jpeg_pack, dim3(pl.n_int), dim3(256), 0, st, (const uint8_t *)e.cfg + 256, JPEG_HEADER_BYTES, (const uint8_t *)e.scratch, pl.slot_bytes,
                     (const uint32_t *)e.len, (const uint32_t *)e.off, pl.n_int, e.c.out[slot]);
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[3], st);
  return err;
}

int jpeg_collect(JpegEnc &e, int slot, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn) {
  return enc_collect(e.off + e.pl.n_int, e.c.out[slot], out, cap, bytes_out, st, fn, g_jpeg_format);
}

} // namespace fspt

// The stand-alone entries: NULL and range checks first, then the device.  coef_out: fspt_jpeg_coefficients_eval's form,
// stage one alone and its coefficients copied back.
static int jpeg_encode_any(const char *fn, int device, const uint8_t *rgba8, bool on_device, uint32_t w, uint32_t h, int bottom_up,
                           const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out, int16_t *coef_out) {
  if (!rgba8 || (coef_out ? false : !out || !bytes_out)) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  fspt::JpegPlan pl;
  const int rc = fspt::jpeg_plan(p, w, h, fn, pl);
  if (rc) return rc;
  fspt::JpegEnc e;
  const auto launch = [&](fspt::Hold &hold) {
    const void *src = rgba8;
    hipError_t err = on_device ? hipSuccess : fspt::enc_upload(hold, rgba8, (size_t)w * h * 4, &src);
    if (err == hipSuccess) err = coef_out ? fspt::jpeg_launch_blocks(e, (const uint32_t *)src, bottom_up, nullptr) : fspt::jpeg_launch(e, (const uint32_t *)src, bottom_up, 0, nullptr);
    if (err == hipSuccess && coef_out) err = hipMemcpy(coef_out, e.coef, (size_t)pl.n_blocks * 128u, hipMemcpyDeviceToHost);
    return err;
  };
  const auto ensure = [&] { return fspt::jpeg_ensure(e, pl, coef_out ? 0 : 1, pl.bound); };
  if (coef_out) return fspt::enc_run(fn, device, e.c, fspt::g_jpeg_format, ensure, launch, nullptr);
  return fspt::enc_run(fn, device, e.c, fspt::g_jpeg_format, ensure, launch, [&] { return fspt::jpeg_collect(e, 0, nullptr, out, cap, bytes_out, fn); });
}

extern "C" {

int fspt_jpeg_bound(uint32_t w, uint32_t h, const fspt_jpeg_params *p, size_t *bytes) {
  return fspt::enc_bound<fspt::JpegPlan>("fspt_jpeg_bound", bytes, [&](fspt::JpegPlan &pl) { return fspt::jpeg_plan(p, w, h, "fspt_jpeg_bound", pl); });
}

int fspt_jpeg_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return jpeg_encode_any("fspt_jpeg_encode", device, rgba8, false, w, h, bottom_up, p, out, cap, bytes_out, nullptr);
}

int fspt_jpeg_encode_device(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return jpeg_encode_any("fspt_jpeg_encode_device", device, rgba8, true, w, h, bottom_up, p, out, cap, bytes_out, nullptr);
}

int fspt_jpeg_coefficients_eval(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, int16_t *coef_out) {
  if (!coef_out) { fspt_set_error("fspt_jpeg_coefficients_eval: NULL argument"); return FSPT_E_INVALID; }
  return jpeg_encode_any("fspt_jpeg_coefficients_eval", device, rgba8, false, w, h, bottom_up, p, nullptr, 0, nullptr, coef_out);
}

int fspt_jpeg_last_ms(float ms[3], uint64_t *bus_bytes) { return fspt::enc_last_ms(fspt::g_jpeg_format, "fspt_jpeg_last_ms", ms, bus_bytes); }

} // extern "C"
