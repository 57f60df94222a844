// fspt_png.hip - a PNG encoder on the GPU: the drawn RGBA8 frame, which draw_launch leaves in device memory,
// becomes a lossless PNG file there, so that only the file's bytes cross the bus.  Integer arithmetic throughout; the bytes
// are tests/png_ref.py's, which states the format: the five filters under the smallest sum of signed magnitudes, deflate in
// independent chunks of literals and distance-1 matches under a length-limited dynamic Huffman code per chunk.
//   k_png_filter    one workgroup per row: the five filters' costs from the raw neighbours, reduced across the workgroup,
//                   then the chosen residuals into the flat stream, a whole dword per lane where the row owns it
//   k_png_deflate   (also the OpenEXR encoder's, fspt_exr.hip: the input is segments, each a zlib stream of its own whose chunks restart
//                   at its first byte; a PNG is one segment)  one workgroup per chunk: run heads and lengths by a scan, tokens in closed form per position, the
//                   histogram by LDS atomics, the code by a rank sort and one lane's merge, the bits OR-ed into an LDS
//                   buffer at scanned offsets (disjoint bits: order does not matter), the stored block where it is not
//                   longer, the chunk's Adler pair and its IDAT's CRC-32 as sums over the lanes' slices
//   k_png_offsets   a scan of the chunk lengths (each with an IDAT's 12 bytes): where every IDAT lands; the Adler pairs
//                   combined in chunk order
//   k_png_pack      header and IDATs into one contiguous stream, the Adler IDAT, IEND, the byte count
#include "fspt_internal.hpp"
#include "fspt_png_tables.hpp"

namespace fspt {
namespace {

constexpr uint32_t PNG_FT = 256u;       // lanes of a filter workgroup
constexpr uint32_t PNG_DT = 512u;       // lanes of a deflate workgroup
constexpr uint32_t PNG_NSYM = 286u;     // literal/length symbols
constexpr uint32_t PNG_SYMS = 288u;     // (arrays of them)
constexpr uint32_t PNG_ADLER = DEFLATE_ADLER;
constexpr uint32_t PNG_CHUNK_MIN = DEFLATE_CHUNK_MIN, PNG_CHUNK_MAX = DEFLATE_CHUNK_MAX;
constexpr uint32_t PNG_CHUNK_EXTRA = 12u; // beyond a chunk's own bytes: the zlib header (2), a stored header (5) and the empty stored block (5) at the most
constexpr uint32_t PNG_META = DEFLATE_META; // words per chunk: bytes, CRC-32, Adler A, Adler B

struct PngFilterP {
  const uint32_t *rgba; // w x h texels
  uint32_t w, h, bottom_up, channels, filter, row_bytes;
  uint8_t *stream;      // h rows of row_bytes = 1 + w * channels
};

// the texel at (x, y) of the top-down image; 0 to the left of it and above it
__device__ __forceinline__ uint32_t png_texel(const PngFilterP &p, int x, int y) {
  if (x < 0 || y < 0) return 0u;
  const uint32_t row = p.bottom_up ? p.h - 1u - (uint32_t)y : (uint32_t)y;
  return p.rgba[(size_t)row * p.w + (uint32_t)x];
}

// the PNG specification's filters: x the byte, a its left, b its upper, c its upper-left neighbour
__device__ __forceinline__ uint32_t png_residual(uint32_t type, int x, int a, int b, int c) {
  int pred = 0;
  if (type == 1u) pred = a;
  else if (type == 2u) pred = b;
  else if (type == 3u) pred = (a + b) >> 1;
  else if (type == 4u) {
    const int pp = a + b - c, pa = abs(pp - a), pb = abs(pp - b), pc = abs(pp - c);
    pred = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
  }
  return (uint32_t)(x - pred) & 255u;
}

__global__ void __launch_bounds__(PNG_FT) k_png_filter(PngFilterP p) {
  __shared__ uint32_t s_cost[5];
  __shared__ uint32_t s_type;
  const uint32_t t = threadIdx.x;
  const int y = (int)blockIdx.x;
  uint32_t type = p.filter;
  if (type == (uint32_t)FSPT_PNG_FILTER_ADAPTIVE) {
    if (t < 5u) s_cost[t] = 0u;
    __syncthreads();
    uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t x = t; x < p.w; x += PNG_FT) {
      const uint32_t cur = png_texel(p, (int)x, y), left = png_texel(p, (int)x - 1, y), up = png_texel(p, (int)x, y - 1), ul = png_texel(p, (int)x - 1, y - 1);
#pragma unroll
      for (uint32_t ch = 0; ch < 4u; ++ch) {
        if (ch >= p.channels) break;
        const int xv = (int)((cur >> (8u * ch)) & 255u), a = (int)((left >> (8u * ch)) & 255u), b = (int)((up >> (8u * ch)) & 255u), c = (int)((ul >> (8u * ch)) & 255u);
#pragma unroll
        for (uint32_t k = 0; k < 5u; ++k) {
          const uint32_t r = png_residual(k, xv, a, b, c);
          cost[k] += r < 128u ? r : 256u - r; // (at most 128 * 4 * 65535: no overflow)
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) {
      uint32_t v = cost[k];
#pragma unroll
      for (uint32_t s = 32u; s; s >>= 1) v += __shfl_down(v, s);
      if ((t & 63u) == 0u) atomicAdd(&s_cost[k], v);
    }
    __syncthreads();
    if (t == 0) {
      uint32_t best = 0;
      for (uint32_t k = 1; k < 5u; ++k) if (s_cost[k] < s_cost[best]) best = k; // a tie: the lowest type
      s_type = best;
    }
    __syncthreads();
    type = s_type;
  }
  // the row's bytes [S, E) of the flat stream, a dword of the stream's own grid per lane: stored whole where the row owns it
  const size_t S = (size_t)y * p.row_bytes, E = S + p.row_bytes;
  for (size_t d = (S & ~(size_t)3) + 4u * t; d < E; d += 4u * PNG_FT) {
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const size_t pos = d + k;
      if (pos < S || pos >= E) continue;
      const uint32_t j = (uint32_t)(pos - S);
      uint32_t v = type;
      if (j) {
        const uint32_t px = p.channels == 4u ? (j - 1u) >> 2 : (j - 1u) / 3u, ch = j - 1u - px * p.channels;
        const uint32_t cur = png_texel(p, (int)px, y), left = png_texel(p, (int)px - 1, y), up = png_texel(p, (int)px, y - 1), ul = png_texel(p, (int)px - 1, y - 1);
        v = png_residual(type, (int)((cur >> (8u * ch)) & 255u), (int)((left >> (8u * ch)) & 255u), (int)((up >> (8u * ch)) & 255u), (int)((ul >> (8u * ch)) & 255u));
      }
      word |= v << (8u * k);
    }
    if (d >= S && d + 4u <= E) *(uint32_t *)(p.stream + d) = word;
    else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k) if (d + k >= S && d + k < E) p.stream[d + k] = (uint8_t)(word >> (8u * k));
    }
  }
}

using PngDeflateP = DeflateP; // (fspt_internal.hpp: the OpenEXR encoder launches the same kernel)

// a lane's writer into the LDS bit buffer, deflate's order: bit position p counts from the least significant bit of word 0
struct LsbSink {
  uint32_t *buf;
  uint32_t p, w, acc;
  __device__ __forceinline__ LsbSink(uint32_t *b, uint32_t at) : buf(b), p(at), w(at >> 5), acc(0u) {}
  __device__ __forceinline__ void put(uint32_t v, uint32_t len) { // len <= 32
    const uint64_t x = (uint64_t)v << (p & 31u);
    acc |= (uint32_t)x;
    p += len;
    if ((p >> 5) != w) { atomicOr(&buf[w], acc); acc = (uint32_t)(x >> 32); ++w; }
  }
  __device__ __forceinline__ void flush() { if (acc) atomicOr(&buf[w], acc); }
};

// the tables of one code under construction
struct PngHuff {
  uint32_t key[PNG_SYMS], leafw[PNG_SYMS], nodew[PNG_SYMS], depth[PNG_SYMS];
  uint16_t sorted[PNG_SYMS], pleaf[PNG_SYMS], pnode[PNG_SYMS];
  uint32_t count[16], cum[16], next[16];
  uint32_t n;
};

// tests/png_ref.py's code_lengths and canonical, by the whole workgroup (nsym <= PNG_DT): len[s] and the code of s with its
// bits reversed, as deflate packs it.  Ends with a barrier.
__device__ void png_build_code(const uint32_t *freq, uint32_t nsym, uint32_t maxb, uint32_t *len, uint32_t *code, PngHuff &H) {
  const uint32_t t = threadIdx.x;
  const uint32_t f = t < nsym ? freq[t] : 0u;
  if (t < nsym) { H.key[t] = f ? (f << 9) | t : 0xFFFFFFFFu; len[t] = 0u; code[t] = 0u; } // (f <= 32769: 25 bits)
  if (t < 16u) H.count[t] = 0u;
  if (t == 0) H.n = 0u;
  __syncthreads();
  if (f) { // the rank sort: (frequency, symbol) ascending
    const uint32_t mine = H.key[t];
    uint32_t rank = 0;
    for (uint32_t s = 0; s < nsym; ++s) rank += H.key[s] < mine ? 1u : 0u;
    H.sorted[rank] = (uint16_t)t; H.leafw[rank] = f;
    atomicAdd(&H.n, 1u);
  }
  __syncthreads();
  const uint32_t n = H.n;
  if (t == 0) { // Huffman's tree by the two-queue merge, a leaf first where the weights tie
    if (n == 1u) H.count[1] = 1u;
    else if (n > 1u) {
      uint32_t i = 0, j = 0;
      for (uint32_t k = 0; k + 1u < n; ++k) {
        uint32_t wsum = 0;
        for (uint32_t r = 0; r < 2u; ++r) {
          if (i < n && (j >= k || H.leafw[i] <= H.nodew[j])) { wsum += H.leafw[i]; H.pleaf[i] = (uint16_t)k; ++i; }
          else { wsum += H.nodew[j]; H.pnode[j] = (uint16_t)k; ++j; }
        }
        H.nodew[k] = wsum;
      }
      H.depth[n - 2u] = 0u;
      for (uint32_t k = n - 2u; k-- > 0u;) H.depth[k] = H.depth[H.pnode[k]] + 1u;
    }
  }
  __syncthreads();
  if (n > 1u && t < n) atomicAdd(&H.count[min(H.depth[H.pleaf[t]] + 1u, maxb)], 1u);
  __syncthreads();
  if (t == 0 && n) { // the limit: while the Kraft sum is too large one code leaves maxb and the longest shorter one is split
    uint32_t total = 0;
    for (uint32_t d = 1; d <= maxb; ++d) total += H.count[d] << (maxb - d);
    while (total > (1u << maxb)) {
      --H.count[maxb];
      for (uint32_t d = maxb - 1u; d >= 1u; --d) if (H.count[d]) { --H.count[d]; H.count[d + 1u] += 2u; break; }
      --total;
    }
    uint32_t c = 0, cd = 0;
    for (uint32_t d = 1; d <= maxb; ++d) {
      c += H.count[d]; H.cum[d] = c;
      cd = (cd + H.count[d - 1u]) << 1; H.next[d] = cd;
    }
  }
  __syncthreads();
  if (t < n) { // lengths along the sorted order from its end
    const uint32_t q = n - 1u - t;
    uint32_t d = 1;
    while (d < maxb && H.cum[d] <= q) ++d;
    len[H.sorted[t]] = d;
  }
  __syncthreads();
  if (t < nsym) {
    const uint32_t L = len[t];
    if (L) {
      uint32_t r = 0;
      for (uint32_t s = 0; s < t; ++s) r += len[s] == L ? 1u : 0u;
      code[t] = __brev(H.next[L] + r) >> (32u - L);
    }
  }
  __syncthreads();
}

// The tokens of the bytes [lo, hi) of a chunk, in order: f(literal, 0) or f(-, match length).  head_lo: where the run that
// holds lo starts; next_hi: the first run head at or behind hi (the chunk's end when there is none).  A run of R bytes from
// s is a literal, then for the M = R - 1 bytes behind it matches of 258 and one of what is left while that is 3 or more,
// else literals: the token of a position follows from s and M alone.
template <class F>
__device__ __forceinline__ void png_walk(const uint8_t *in, uint32_t lo, uint32_t hi, uint32_t head_lo, uint32_t next_hi, F f) {
  uint32_t i = lo, s = head_lo;
  while (i < hi) {
    const uint32_t v = in[i];
    uint32_t e = i + 1u;
    while (e < hi && in[e] == v) ++e;
    const uint32_t stop = e;  // this lane's share of the run: [i, stop)
    if (e == hi) e = next_hi; // the run may go on in the next lanes' bytes
    const uint32_t M = e - s - 1u;
    for (uint32_t pos = i; pos < stop; ++pos) {
      if (pos == s) { f(v, 0u); continue; }
      const uint32_t j = pos - s - 1u, bs = j - j % 258u, rem = M - bs;
      if (rem < 3u) f(v, 0u);
      else if (j == bs) f(0u, min(rem, 258u));
    }
    i = stop; s = stop;
  }
}

// `crc` (a finished CRC-32) of a message as its share of the CRC-32 of that message followed by n_bytes more: times
// x^(8 n_bytes) mod P, bit 31 = x^0
__device__ __forceinline__ uint32_t png_crc_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    if (a & (0x80000000u >> i)) r ^= b;
    b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
  }
  return r;
}
__device__ __forceinline__ uint32_t png_crc_shift(uint32_t crc, uint32_t n_bytes) {
  for (uint32_t k = 0; n_bytes; n_bytes >>= 1, ++k) if (n_bytes & 1u) crc = png_crc_mul(PNG_CRC_X8POW[k & 15u], crc);
  return crc;
}

__global__ void __launch_bounds__(PNG_DT) k_png_deflate(PngDeflateP p) {
  extern __shared__ uint32_t s_dyn[]; // the chunk | its output
  __shared__ PngHuff H;
  __shared__ uint32_t s_freq[PNG_SYMS], s_len[PNG_SYMS], s_code[PNG_SYMS], s_cfreq[32], s_clen[32], s_ccode[32], s_syms[320];
  __shared__ uint32_t s_scan[PNG_DT], s_scan2[PNG_DT], s_crc[256], s_lencode[256];
  __shared__ uint32_t s_nsyms, s_hlit, s_hclen, s_hbits, s_red[3];
  const uint32_t t = threadIdx.x, k = blockIdx.x;
  // chunk j of segment seg: a segment is a zlib stream of its own, and its chunks restart at its first byte
  const uint32_t seg = k / p.cps, j = k - seg * p.cps;
  const size_t seg_base = (size_t)seg * p.seg_bytes, seg_len = min(p.seg_bytes, p.stream_bytes - seg_base);
  const size_t base = seg_base + (size_t)j * p.cb;
  const uint32_t n = (uint32_t)min((size_t)p.cb, seg_len - (size_t)j * p.cb);
  const bool first = j == 0u, last = (size_t)j * p.cb + n == seg_len;
  const uint32_t in_words = (p.cb + 3u) / 4u + 1u, out_words = (p.cb + PNG_CHUNK_EXTRA + 3u) / 4u + 2u;
  uint32_t *s_out = s_dyn + in_words;
  const uint8_t *in = (const uint8_t *)s_dyn;
  uint8_t *outb = (uint8_t *)s_out;

  // 1. the chunk, the tables, empty histograms and an empty bit buffer
  const uint8_t *src = p.stream + base;
  const bool aligned = (base & 3u) == 0u;
  for (uint32_t i = t; i * 4u < n; i += PNG_DT) {
    uint32_t word = 0;
    if (aligned && i * 4u + 4u <= n) word = *(const uint32_t *)(src + i * 4u);
    else for (uint32_t b = 0; b < 4u; ++b) if (i * 4u + b < n) word |= (uint32_t)src[i * 4u + b] << (8u * b);
    s_dyn[i] = word;
  }
  for (uint32_t i = t; i < out_words; i += PNG_DT) s_out[i] = 0u;
  if (t < PNG_SYMS) s_freq[t] = t == 256u ? 1u : 0u; // the end-of-block symbol
  if (t < 32u) s_cfreq[t] = 0u;
  if (t < 256u) { s_crc[t] = PNG_CRC_TABLE[t]; s_lencode[t] = PNG_LEN_CODE[t]; }
  if (t < 3u) s_red[t] = 0u;
  __syncthreads();

  // 2. run heads: per lane the first and the last head of its bytes; a forward max-scan and a backward min-scan across the lanes
  const uint32_t span = (n + PNG_DT - 1u) / PNG_DT;
  const uint32_t lo = min(t * span, n), hi = min(lo + span, n);
  uint32_t first_head = n, last_head1 = 0u; // (the last one + 1; 0 = none)
  for (uint32_t i = lo; i < hi; ++i)
    if (i == 0u || in[i] != in[i - 1u]) { if (first_head == n) first_head = i; last_head1 = i + 1u; }
  s_scan[t] = last_head1; s_scan2[t] = first_head;
  __syncthreads();
  for (uint32_t d = 1; d < PNG_DT; d <<= 1) {
    uint32_t a = s_scan[t], b = s_scan2[t];
    if (t >= d) a = max(a, s_scan[t - d]);
    if (t + d < PNG_DT) b = min(b, s_scan2[t + d]);
    __syncthreads();
    s_scan[t] = a; s_scan2[t] = b;
    __syncthreads();
  }
  const uint32_t head_lo = first_head == lo || t == 0u ? lo : s_scan[t - 1u] - 1u; // (byte 0 is a head, and lane 0's)
  const uint32_t next_hi = t + 1u < PNG_DT ? s_scan2[t + 1u] : n;
  __syncthreads();

  // 3. the histogram
  png_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) { atomicAdd(&s_freq[len ? s_lencode[len - 3u] & 0xFFFu : lit], 1u); });
  __syncthreads();

  // 4. the literal/length code; its lengths run-length coded by one lane; the code-length code
  png_build_code(s_freq, PNG_NSYM, 15u, s_len, s_code, H);
  if (t == 0) {
    uint32_t hlit = PNG_NSYM;
    while (!s_len[hlit - 1u]) --hlit; // >= 257
    const uint32_t m = hlit + 1u;      // and the one distance code, of one bit
    auto at = [&](uint32_t i) { return i < hlit ? s_len[i] : 1u; };
    uint32_t ns = 0;
    for (uint32_t i = 0; i < m;) {
      const uint32_t v = at(i);
      uint32_t r = 1;
      while (i + r < m && at(i + r) == v) ++r;
      uint32_t sym = v, eb = 0, ev = 0, adv = 1;
      if (v == 0u && r >= 11u) { adv = min(r, 138u); sym = 18u; eb = 7u; ev = adv - 11u; }
      else if (v == 0u && r >= 3u) { adv = r; sym = 17u; eb = 3u; ev = adv - 3u; }
      else if (v && i && at(i - 1u) == v && r >= 3u) { adv = min(r, 6u); sym = 16u; eb = 2u; ev = adv - 3u; }
      s_syms[ns++] = sym | (eb << 8) | (ev << 16);
      ++s_cfreq[sym];
      i += adv;
    }
    s_nsyms = ns; s_hlit = hlit;
  }
  __syncthreads();
  png_build_code(s_cfreq, 19u, 7u, s_clen, s_ccode, H);
  if (t == 0) {
    uint32_t hclen = 19;
    while (hclen > 4u && !s_clen[PNG_CL_ORDER[hclen - 1u]]) --hclen;
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen;
    for (uint32_t i = 0; i < s_nsyms; ++i) bits += s_clen[s_syms[i] & 255u] + ((s_syms[i] >> 8) & 255u);
    s_hclen = hclen; s_hbits = bits;
  }
  __syncthreads();

  // 5. the tokens' sizes, scanned: where each lane's bits start, and the block's exact length before anything is emitted
  uint32_t mine = 0;
  png_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) {
    if (len) { const uint32_t e = s_lencode[len - 3u]; mine += s_len[e & 0xFFFu] + ((e >> 12) & 15u) + 1u; }
    else mine += s_len[lit];
  });
  s_scan[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < PNG_DT; d <<= 1) {
    uint32_t a = s_scan[t];
    if (t >= d) a += s_scan[t - d];
    __syncthreads();
    s_scan[t] = a;
    __syncthreads();
  }
  const uint32_t body = s_scan[PNG_DT - 1u];
  const uint32_t dyn_bits = s_hbits + body + s_len[256];
  const uint32_t ob = first ? 2u : 0u; // the zlib header in front of a segment's first chunk
  const bool stored = (dyn_bits + 7u) / 8u >= 5u + n;
  uint32_t L; // the chunk's bytes in the file
  if (stored) {
    if (t == 0) {
      outb[ob] = last ? 1u : 0u;
      outb[ob + 1u] = (uint8_t)n; outb[ob + 2u] = (uint8_t)(n >> 8); outb[ob + 3u] = (uint8_t)~n; outb[ob + 4u] = (uint8_t)(~n >> 8);
    }
    for (uint32_t i = t; i < n; i += PNG_DT) outb[ob + 5u + i] = in[i];
    L = ob + 5u + n;
  } else { // (shorter than the stored block: the buffer holds it)
    const uint32_t at0 = ob * 8u;
    if (t == 0) { // the header, and the end-of-block symbol
      LsbSink sink(s_out, at0);
      sink.put(last ? 1u : 0u, 1u); sink.put(2u, 2u);
      sink.put(s_hlit - 257u, 5u); sink.put(0u, 5u); sink.put(s_hclen - 4u, 4u);
      for (uint32_t i = 0; i < s_hclen; ++i) sink.put(s_clen[PNG_CL_ORDER[i]], 3u);
      for (uint32_t i = 0; i < s_nsyms; ++i) {
        const uint32_t e = s_syms[i], sym = e & 255u, cl = s_clen[sym];
        sink.put(s_ccode[sym] | ((e >> 16) << cl), cl + ((e >> 8) & 255u));
      }
      sink.flush();
      LsbSink eob(s_out, at0 + s_hbits + body);
      eob.put(s_code[256], s_len[256]);
      eob.flush();
    }
    LsbSink sink(s_out, at0 + s_hbits + s_scan[t] - mine);
    png_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) {
      if (len) {
        const uint32_t e = s_lencode[len - 3u], sym = e & 0xFFFu, cl = s_len[sym];
        sink.put(s_code[sym] | ((e >> 16) << cl), cl + ((e >> 12) & 15u) + 1u); // the distance code 0 behind it: distance 1
      } else sink.put(s_code[lit], s_len[lit]);
    });
    sink.flush();
    const uint32_t end_bits = at0 + dyn_bits;
    if (last) L = (end_bits + 7u) / 8u;
    else { // an empty stored block: three zero bits, zeros to the byte, 00 00 FF FF
      const uint32_t at = (end_bits + 3u + 7u) / 8u;
      L = at + 4u;
    }
  }
  __syncthreads();
  if (t == 0) {
    if (first) { outb[0] = 0x78; outb[1] = 0x01; }
    if (!stored && !last) { outb[L - 2u] = 0xFF; outb[L - 1u] = 0xFF; }
  }
  __syncthreads();

  // 6. the IDAT's CRC-32 ("IDAT", then the L bytes) and the chunk's Adler pair: sums over the lanes' slices
  {
    const uint32_t cspan = (L + PNG_DT - 1u) / PNG_DT, clo = min(t * cspan, L), chi = min(clo + cspan, L);
    uint32_t x = 0;
    if (p.crc && chi > clo) {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t i = clo; i < chi; ++i) c = s_crc[(c ^ outb[i]) & 255u] ^ (c >> 8);
      x = png_crc_shift(~c, L - chi);
    }
    if (p.crc && t == 0) x ^= png_crc_shift(PNG_CRC_IDAT, L);
    uint32_t sa = 0, sb = 0; // (a lane: at most 64 bytes of 255 at a weight of 32768)
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t v = in[i]; sa += v; sb += (n - i) * v; }
    sb %= PNG_ADLER;
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) { x ^= __shfl_xor(x, s); sa += __shfl_xor(sa, s); sb += __shfl_xor(sb, s); }
    if ((t & 63u) == 0u) { atomicXor(&s_red[0], x); atomicAdd(&s_red[1], sa); atomicAdd(&s_red[2], sb); }
  }
  __syncthreads();
  if (t == 0) {
    uint32_t *m = p.meta + (size_t)k * PNG_META;
    m[0] = L; m[1] = s_red[0]; m[2] = (1u + s_red[1]) % PNG_ADLER; m[3] = (n + s_red[2]) % PNG_ADLER;
  }
  uint32_t *dst = (uint32_t *)(p.scratch + (size_t)k * p.slot_bytes);
  for (uint32_t i = t; i * 4u < L; i += PNG_DT) dst[i] = s_out[i];
}

// off[k] = hdr_len + sum over i < k of (len[i] + 12): where chunk k's IDAT starts; off[n] = where the Adler IDAT starts,
// off[n + 1] = the file's length, off[n + 2] = the Adler-32 of the whole stream: the chunks' pairs combined in order,
// A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1)
__global__ void __launch_bounds__(256) k_png_offsets(const uint32_t *__restrict__ meta, uint32_t n, uint32_t hdr_len, uint32_t cb, size_t stream_bytes, uint32_t *__restrict__ off) {
  __shared__ uint32_t s[256], sa[256];
  __shared__ uint32_t running, running_a, sum_b;
  const uint32_t t = threadIdx.x;
  if (t == 0) { running = hdr_len; running_a = 0u; sum_b = 0u; }
  __syncthreads();
  uint32_t my_b = 0;
  for (uint32_t base = 0; base < n; base += 256u) {
    const uint32_t i = base + t;
    const uint32_t v = i < n ? meta[(size_t)i * PNG_META] + 12u : 0u;
    const uint32_t a = i < n ? meta[(size_t)i * PNG_META + 2u] + PNG_ADLER - 1u : 0u; // A - 1 mod 65521
    s[t] = v; sa[t] = i < n ? a % PNG_ADLER : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
      const uint32_t o = t >= d ? s[t - d] : 0u, oa = t >= d ? sa[t - d] : 0u;
      __syncthreads();
      s[t] += o; sa[t] += oa; // (256 values below 65521)
      __syncthreads();
    }
    const uint32_t r = running, ra = running_a;
    if (i < n) {
      off[i] = r + s[t] - v;
      const uint32_t before = (ra + sa[t] - a % PNG_ADLER) % PNG_ADLER; // A - 1 of everything in front of chunk i
      const uint32_t len_in = (uint32_t)min((size_t)cb, stream_bytes - (size_t)i * cb);
      my_b = (uint32_t)((my_b + meta[(size_t)i * PNG_META + 3u] + (uint64_t)(len_in % PNG_ADLER) * before) % PNG_ADLER);
    }
    __syncthreads();
    if (t == 255u) { running = r + s[255]; running_a = (ra + sa[255]) % PNG_ADLER; }
    __syncthreads();
  }
  atomicAdd(&sum_b, my_b);
  __syncthreads();
  if (t == 0) {
    off[n] = running; off[n + 1u] = running + 16u + 12u;
    off[n + 2u] = ((sum_b % PNG_ADLER) << 16) | ((1u + running_a) % PNG_ADLER);
  }
}

__device__ __forceinline__ void png_put_be(uint8_t *o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }

__global__ void __launch_bounds__(256) k_png_pack(const uint8_t *__restrict__ hdr, uint32_t hdr_len, const uint8_t *__restrict__ scratch, size_t slot_bytes,
                                                   const uint32_t *__restrict__ meta, const uint32_t *__restrict__ off, uint32_t n, uint8_t *__restrict__ out) {
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  if (k == 0) for (uint32_t i = t; i < hdr_len; i += 256u) out[i] = hdr[i];
  const uint8_t *src = scratch + (size_t)k * slot_bytes;
  const uint32_t L = meta[(size_t)k * PNG_META];
  uint8_t *dst = out + off[k];
  for (uint32_t i = t; i < L; i += 256u) dst[8u + i] = src[i];
  if (t == 0) {
    png_put_be(dst, L);
    dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    png_put_be(dst + 8u + L, meta[(size_t)k * PNG_META + 1u]);
  }
  if (k + 1u == n && t == 64u) { // the Adler-32 in an IDAT of its own, and IEND
    uint8_t *o = out + off[n];
    const uint8_t tail[28] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82};
    for (uint32_t i = 0; i < 28u; ++i) o[i] = tail[i];
    png_put_be(o + 8u, off[n + 2u]);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 4; i < 12u; ++i) c = PNG_CRC_TABLE[(c ^ o[i]) & 255u] ^ (c >> 8);
    png_put_be(o + 12u, ~c);
  }
}

float g_png_ms[3] = {0.0f, 0.0f, 0.0f};
uint64_t g_png_bus_bytes = 0;

uint32_t host_crc(const uint8_t *d, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = PNG_CRC_TABLE[(c ^ d[i]) & 255u] ^ (c >> 8);
  return ~c;
}

size_t png_bound_of(uint32_t w, uint32_t h, uint32_t channels, uint32_t cb) {
  const size_t stream = (size_t)h * (1u + (size_t)w * channels);
  return 8u + 25u + 2u + 16u + 12u + stream + (stream + cb - 1u) / cb * (5u + 5u + 12u);
}

size_t png_dyn_lds(uint32_t cb) { return (((size_t)cb + 3u) / 4u + 1u + ((size_t)cb + PNG_CHUNK_EXTRA + 3u) / 4u + 2u) * 4u; }

} // namespace

size_t deflate_slot_bytes(uint32_t cb) { return ((size_t)cb + PNG_CHUNK_EXTRA + 3u) / 4u * 4u + 4u; }

hipError_t deflate_launch(const DeflateP &p, uint32_t n_chunks, hipStream_t st) {
  const size_t lds = png_dyn_lds(p.cb);
  if (lds > 48u * 1024u) {
    const hipError_t err = hipFuncSetAttribute((const void *)k_png_deflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)png_dyn_lds(PNG_CHUNK_MAX));
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_png_deflate, dim3(n_chunks), dim3(PNG_DT), lds, st, p);
  return hipGetLastError();
}

static const fspt_png_params PNG_DEFAULTS = {3u, (uint32_t)FSPT_PNG_FILTER_ADAPTIVE, FSPT_PNG_CHUNK};

int png_check_params(const fspt_png_params *prm, const char *fn) {
  const fspt_png_params q = prm ? *prm : PNG_DEFAULTS;
  if (q.channels != 0u && q.channels != 3u && q.channels != 4u) { fspt_set_error("%s: channels must be 3 or 4", fn); return FSPT_E_INVALID; }
  if (q.filter > (uint32_t)FSPT_PNG_FILTER_ADAPTIVE) { fspt_set_error("%s: unknown filter %u", fn, q.filter); return FSPT_E_INVALID; }
  if (q.chunk_bytes != 0u && (q.chunk_bytes < PNG_CHUNK_MIN || q.chunk_bytes > PNG_CHUNK_MAX)) { fspt_set_error("%s: chunk_bytes must be 0 or in 256..32768", fn); return FSPT_E_INVALID; }
  return FSPT_OK;
}

int png_plan(const fspt_png_params *prm, uint32_t w, uint32_t h, bool for_device, const char *fn, PngPlan &pl) {
  const fspt_png_params q = prm ? *prm : PNG_DEFAULTS;
  if (w == 0 || h == 0 || w > 65535u || h > 65535u) { fspt_set_error("%s: width and height must be in 1..65535", fn); return FSPT_E_INVALID; }
  const int rc = png_check_params(prm, fn);
  if (rc) return rc;
  pl = PngPlan{};
  pl.w = w; pl.h = h; pl.channels = q.channels ? q.channels : 3u; pl.filter = q.filter;
  pl.cb = q.chunk_bytes ? q.chunk_bytes : FSPT_PNG_CHUNK;
  pl.row_bytes = 1u + w * pl.channels;
  pl.stream_bytes = (size_t)h * pl.row_bytes;
  pl.bound = png_bound_of(w, h, pl.channels, pl.cb);
  if (for_device && pl.bound > 0xFFFFFFFFull) { fspt_set_error("%s: a file of %u x %u could pass 4 GiB", fn, w, h); return FSPT_E_INVALID; }
  pl.n_chunks = (uint32_t)((pl.stream_bytes + pl.cb - 1u) / pl.cb);
  pl.slot_bytes = deflate_slot_bytes(pl.cb);
  return FSPT_OK;
}

size_t png_bound_max(uint32_t w, uint32_t h, uint32_t cb) { return png_bound_of(w, h, 4u, cb); }

static bool same_plan(const PngPlan &a, const PngPlan &b) {
  return a.w == b.w && a.h == b.h && a.channels == b.channels && a.filter == b.filter && a.cb == b.cb;
}

void png_release(PngEnc &e) {
  hipFree(e.cfg); hipFree(e.stream); hipFree(e.scratch); hipFree(e.meta); hipFree(e.out);
  for (hipEvent_t &ev : e.ev) { if (ev) hipEventDestroy(ev); ev = nullptr; }
  e.cfg = nullptr; e.stream = nullptr; e.scratch = nullptr; e.meta = nullptr; e.off = nullptr; e.out = nullptr;
  e.valid = false; e.out_bytes = 0;
}

// The encoder's device memory for `pl`: the header once per (size, parameters), the work buffers, and with_out an output
// buffer of out_bytes (>= pl.bound; it outlives a change of the parameters and grows).  Nothing of it may be in use.
hipError_t png_ensure(PngEnc &e, const PngPlan &pl, bool with_out, size_t out_bytes) {
  hipError_t err = hipSuccess;
  if (with_out && !(e.out && e.out_bytes >= out_bytes)) {
    hipFree(e.out); e.out = nullptr; e.out_bytes = 0;
    err = hipMalloc((void **)&e.out, out_bytes);
    if (err == hipSuccess) e.out_bytes = out_bytes;
  }
  for (hipEvent_t &ev : e.ev) if (!ev && err == hipSuccess) err = hipEventCreate(&ev);
  if (err != hipSuccess || (e.valid && same_plan(e.pl, pl))) return err;
  hipFree(e.cfg); hipFree(e.stream); hipFree(e.scratch); hipFree(e.meta);
  e.cfg = nullptr; e.stream = nullptr; e.scratch = nullptr; e.meta = nullptr; e.off = nullptr; e.valid = false;
  uint8_t hdr[PNG_HEADER_BYTES] = {137, 80, 78, 71, 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                   (uint8_t)(pl.w >> 24), (uint8_t)(pl.w >> 16), (uint8_t)(pl.w >> 8), (uint8_t)pl.w,
                                   (uint8_t)(pl.h >> 24), (uint8_t)(pl.h >> 16), (uint8_t)(pl.h >> 8), (uint8_t)pl.h,
                                   8, (uint8_t)(pl.channels == 3u ? 2 : 6), 0, 0, 0};
  const uint32_t c = host_crc(hdr + 12, 17);
  hdr[29] = (uint8_t)(c >> 24); hdr[30] = (uint8_t)(c >> 16); hdr[31] = (uint8_t)(c >> 8); hdr[32] = (uint8_t)c;
  err = hipMalloc((void **)&e.cfg, 64);
  if (err == hipSuccess) err = hipMalloc((void **)&e.stream, (pl.stream_bytes + 3u) / 4u * 4u + 4u);
  if (err == hipSuccess) err = hipMalloc((void **)&e.scratch, (size_t)pl.n_chunks * pl.slot_bytes);
  if (err == hipSuccess) err = hipMalloc((void **)&e.meta, ((size_t)pl.n_chunks * (PNG_META + 1u) + 3u) * 4u);
  if (err == hipSuccess) err = hipMemcpy(e.cfg, hdr, sizeof hdr, hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  e.off = e.meta + (size_t)pl.n_chunks * PNG_META;
  e.pl = pl; e.valid = true;
  return hipSuccess;
}

hipError_t png_launch_filter(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st) {
  const PngPlan &pl = e.pl;
  PngFilterP f{rgba, pl.w, pl.h, bottom_up ? 1u : 0u, pl.channels, pl.filter, pl.row_bytes, e.stream};
  hipLaunchKernelGGL(k_png_filter, dim3(pl.h), dim3(PNG_FT), 0, st, f);
  return hipGetLastError();
}

// The whole encode of `rgba` (device memory, w x h texels) into e.out on `st`; the file's length lands in
// e.off[n_chunks + 1].  Events 0..3 bracket the three stages.  No host read, no synchronisation.
hipError_t png_launch(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st) {
  const PngPlan &pl = e.pl;
  hipError_t err = hipEventRecord(e.ev[0], st);
  if (err == hipSuccess) err = png_launch_filter(e, rgba, bottom_up, st);
  if (err == hipSuccess) err = hipEventRecord(e.ev[1], st);
  if (err != hipSuccess) return err;
  const DeflateP d{e.stream, pl.stream_bytes, pl.stream_bytes, pl.cb, pl.n_chunks, 1u, e.scratch, pl.slot_bytes, e.meta}; // one segment
  err = deflate_launch(d, pl.n_chunks, st);
  if (err == hipSuccess) err = hipEventRecord(e.ev[2], st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_png_offsets, dim3(1), dim3(256), 0, st, (const uint32_t *)e.meta, pl.n_chunks, PNG_HEADER_BYTES, pl.cb, pl.stream_bytes, e.off);
  hipLaunchKernelGGL(k_png_pack, dim3(pl.n_chunks), dim3(256), 0, st, (const uint8_t *)e.cfg, PNG_HEADER_BYTES, (const uint8_t *)e.scratch, pl.slot_bytes,
                     (const uint32_t *)e.meta, (const uint32_t *)e.off, pl.n_chunks, e.out);
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.ev[3], st);
  return err;
}

int png_collect(PngEnc &e, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn) {
  uint32_t n = 0;
  hipError_t err = hipMemcpyAsync(&n, e.off + e.pl.n_chunks + 1u, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) { fspt_set_error("%s: %s", fn, hipGetErrorString(err)); return FSPT_E_HIP; }
  *bytes_out = n;
  if (cap < n) { fspt_set_error("%s: the file takes %u bytes, the buffer holds %zu", fn, n, cap); return FSPT_E_INVALID; }
  err = hipMemcpyAsync(out, e.out, n, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) { fspt_set_error("%s: %s", fn, hipGetErrorString(err)); return FSPT_E_HIP; }
  g_png_bus_bytes = (uint64_t)n + 4u;
  return FSPT_OK;
}

void png_note_ms(PngEnc &e) {
  for (int k = 0; k < 3; ++k) if (hipEventElapsedTime(&g_png_ms[k], e.ev[k], e.ev[k + 1]) != hipSuccess) g_png_ms[k] = 0.0f;
  (void)hipGetLastError();
}

} // namespace fspt

// The stand-alone entries: NULL and range checks first, then the device.  stream_out: fspt_png_filtered_eval's form.
static int png_encode_any(const char *fn, int device, const uint8_t *rgba8, bool on_device, uint32_t w, uint32_t h, int bottom_up,
                          const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out, uint8_t *stream_out) {
  if (!rgba8 || (stream_out ? false : !out || !bytes_out)) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  fspt::PngPlan pl;
  int rc = fspt::png_plan(p, w, h, true, fn, pl);
  if (rc) return rc;
  if (fspt_device_count() <= 0) { fspt_set_error("%s: no HIP device available; libfspt has no CPU fallback", fn); return FSPT_E_NO_DEVICE; }
  if ((rc = check_device(device))) return rc;
  fspt::PngEnc e;
  fspt::Hold hold;
  const uint32_t *src = (const uint32_t *)rgba8;
  hipError_t err = fspt::png_ensure(e, pl, !stream_out, pl.bound);
  if (err == hipSuccess && !on_device) {
    void *d = nullptr;
    err = hold.make(&d, (size_t)w * h * 4);
    if (err == hipSuccess) err = hipMemcpy(d, rgba8, (size_t)w * h * 4, hipMemcpyHostToDevice);
    src = (const uint32_t *)d;
  }
  if (err == hipSuccess) err = stream_out ? fspt::png_launch_filter(e, src, bottom_up, nullptr) : fspt::png_launch(e, src, bottom_up, nullptr);
  if (err == hipSuccess && stream_out) err = hipMemcpy(stream_out, e.stream, pl.stream_bytes, hipMemcpyDeviceToHost);
  if (err != hipSuccess) {
    (void)hipDeviceSynchronize(); (void)hipGetLastError();
    fspt_set_error("%s: %s", fn, hipGetErrorString(err));
    rc = err == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
  } else if (!stream_out) {
    rc = fspt::png_collect(e, nullptr, out, cap, bytes_out, fn);
    if (rc == FSPT_OK || rc == FSPT_E_INVALID) fspt::png_note_ms(e);
  }
  fspt::png_release(e);
  return rc;
}

extern "C" {

int fspt_png_bound(uint32_t w, uint32_t h, const fspt_png_params *p, size_t *bytes) {
  if (!bytes) { fspt_set_error("fspt_png_bound: NULL argument"); return FSPT_E_INVALID; }
  fspt::PngPlan pl;
  const int rc = fspt::png_plan(p, w, h, false, "fspt_png_bound", pl);
  if (rc == FSPT_OK) *bytes = pl.bound;
  return rc;
}

int fspt_png_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return png_encode_any("fspt_png_encode", device, rgba8, false, w, h, bottom_up, p, out, cap, bytes_out, nullptr);
}

int fspt_png_encode_device(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  return png_encode_any("fspt_png_encode_device", device, rgba8, true, w, h, bottom_up, p, out, cap, bytes_out, nullptr);
}

int fspt_png_filtered_eval(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *stream_out) {
  if (!stream_out) { fspt_set_error("fspt_png_filtered_eval: NULL argument"); return FSPT_E_INVALID; }
  return png_encode_any("fspt_png_filtered_eval", device, rgba8, false, w, h, bottom_up, p, nullptr, 0, nullptr, stream_out);
}

int fspt_png_last_ms(float ms[3], uint64_t *bus_bytes) {
  if (!ms) { fspt_set_error("fspt_png_last_ms: NULL argument"); return FSPT_E_INVALID; }
  std::memcpy(ms, fspt::g_png_ms, sizeof fspt::g_png_ms);
  if (bus_bytes) *bus_bytes = fspt::g_png_bus_bytes;
  return FSPT_OK;
}

} // extern "C"
