// fspt_deflate.hip - the deflate the PNG and the OpenEXR encoder share (DeflateP in fspt_internal.hpp):
// the input is segments, each a zlib stream of its own whose chunks restart at its first byte; a PNG is one segment, an
// OpenEXR file one per block.
//   k_deflate   one workgroup per chunk: run heads and lengths by a scan, tokens in closed form per position, the histogram
//               by LDS atomics, the code by a rank sort and one lane's merge, the bits OR-ed into an LDS buffer at scanned
//               offsets (disjoint bits: order does not matter), the stored block where it is not longer, the chunk's Adler
//               pair and, for a PNG, its IDAT's CRC-32 as sums over the lanes' slices
#include "fspt_internal.hpp"
#include "fspt_png_tables.hpp"

namespace fspt {
namespace {

constexpr uint32_t DEFLATE_DT = 512u;       // lanes of a deflate workgroup
constexpr uint32_t DEFLATE_NSYM = 286u;     // literal/length symbols
constexpr uint32_t DEFLATE_SYMS = 288u;     // (arrays of them)

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
struct DeflateHuff {
  uint32_t key[DEFLATE_SYMS], leafw[DEFLATE_SYMS], nodew[DEFLATE_SYMS], depth[DEFLATE_SYMS];
  uint16_t sorted[DEFLATE_SYMS], pleaf[DEFLATE_SYMS], pnode[DEFLATE_SYMS];
  uint32_t count[16], cum[16], next[16];
  uint32_t n;
};

// tests/png_ref.py's code_lengths and canonical, by the whole workgroup (nsym <= DEFLATE_DT): len[s] and the code of s with its
// bits reversed, as deflate packs it.  Ends with a barrier.
__device__ void deflate_build_code(const uint32_t *freq, uint32_t nsym, uint32_t maxb, uint32_t *len, uint32_t *code, DeflateHuff &H) {
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
__device__ __forceinline__ void deflate_walk(const uint8_t *in, uint32_t lo, uint32_t hi, uint32_t head_lo, uint32_t next_hi, F f) {
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

__global__ void __launch_bounds__(DEFLATE_DT) k_deflate(DeflateP p) {
  extern __shared__ uint32_t s_dyn[]; // the chunk | its output
  __shared__ DeflateHuff H;
  __shared__ uint32_t s_freq[DEFLATE_SYMS], s_len[DEFLATE_SYMS], s_code[DEFLATE_SYMS], s_cfreq[32], s_clen[32], s_ccode[32], s_syms[320];
  __shared__ uint32_t s_scan[DEFLATE_DT], s_scan2[DEFLATE_DT], s_crc[256], s_lencode[256];
  __shared__ uint32_t s_nsyms, s_hlit, s_hclen, s_hbits, s_red[3];
  const uint32_t t = threadIdx.x, k = blockIdx.x;
  // chunk j of segment seg: a segment is a zlib stream of its own, and its chunks restart at its first byte
  const uint32_t seg = k / p.cps, j = k - seg * p.cps;
  const size_t seg_base = (size_t)seg * p.seg_bytes, seg_len = min(p.seg_bytes, p.stream_bytes - seg_base);
  const size_t base = seg_base + (size_t)j * p.cb;
  const uint32_t n = (uint32_t)min((size_t)p.cb, seg_len - (size_t)j * p.cb);
  const bool first = j == 0u, last = (size_t)j * p.cb + n == seg_len;
  const uint32_t in_words = (p.cb + 3u) / 4u + 1u, out_words = (p.cb + DEFLATE_CHUNK_EXTRA + 3u) / 4u + 2u;
  uint32_t *s_out = s_dyn + in_words;
  const uint8_t *in = (const uint8_t *)s_dyn;
  uint8_t *outb = (uint8_t *)s_out;

  // 1. the chunk, the tables, empty histograms and an empty bit buffer
  const uint8_t *src = p.stream + base;
  const bool aligned = (base & 3u) == 0u;
  for (uint32_t i = t; i * 4u < n; i += DEFLATE_DT) {
    uint32_t word = 0;
    if (aligned && i * 4u + 4u <= n) word = *(const uint32_t *)(src + i * 4u);
    else for (uint32_t b = 0; b < 4u; ++b) if (i * 4u + b < n) word |= (uint32_t)src[i * 4u + b] << (8u * b);
    s_dyn[i] = word;
  }
  for (uint32_t i = t; i < out_words; i += DEFLATE_DT) s_out[i] = 0u;
  if (t < DEFLATE_SYMS) s_freq[t] = t == 256u ? 1u : 0u; // the end-of-block symbol
  if (t < 32u) s_cfreq[t] = 0u;
  if (t < 256u) { s_crc[t] = PNG_CRC_TABLE[t]; s_lencode[t] = PNG_LEN_CODE[t]; }
  if (t < 3u) s_red[t] = 0u;
  __syncthreads();

  // 2. run heads: per lane the first and the last head of its bytes; a forward max-scan and a backward min-scan across the lanes
  const uint32_t span = (n + DEFLATE_DT - 1u) / DEFLATE_DT;
  const uint32_t lo = min(t * span, n), hi = min(lo + span, n);
  uint32_t first_head = n, last_head1 = 0u; // (the last one + 1; 0 = none)
  for (uint32_t i = lo; i < hi; ++i)
    if (i == 0u || in[i] != in[i - 1u]) { if (first_head == n) first_head = i; last_head1 = i + 1u; }
  s_scan[t] = last_head1; s_scan2[t] = first_head;
  __syncthreads();
  for (uint32_t d = 1; d < DEFLATE_DT; d <<= 1) {
    uint32_t a = s_scan[t], b = s_scan2[t];
    if (t >= d) a = max(a, s_scan[t - d]);
    if (t + d < DEFLATE_DT) b = min(b, s_scan2[t + d]);
    __syncthreads();
    s_scan[t] = a; s_scan2[t] = b;
    __syncthreads();
  }
  const uint32_t head_lo = first_head == lo || t == 0u ? lo : s_scan[t - 1u] - 1u; // (byte 0 is a head, and lane 0's)
  const uint32_t next_hi = t + 1u < DEFLATE_DT ? s_scan2[t + 1u] : n;
  __syncthreads();

  // 3. the histogram
  deflate_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) { atomicAdd(&s_freq[len ? s_lencode[len - 3u] & 0xFFFu : lit], 1u); });
  __syncthreads();

  // 4. the literal/length code; its lengths run-length coded by one lane; the code-length code
  deflate_build_code(s_freq, DEFLATE_NSYM, 15u, s_len, s_code, H);
  if (t == 0) {
    uint32_t hlit = DEFLATE_NSYM;
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
  deflate_build_code(s_cfreq, 19u, 7u, s_clen, s_ccode, H);
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
  deflate_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) {
    if (len) { const uint32_t e = s_lencode[len - 3u]; mine += s_len[e & 0xFFFu] + ((e >> 12) & 15u) + 1u; }
    else mine += s_len[lit];
  });
  s_scan[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < DEFLATE_DT; d <<= 1) {
    uint32_t a = s_scan[t];
    if (t >= d) a += s_scan[t - d];
    __syncthreads();
    s_scan[t] = a;
    __syncthreads();
  }
  const uint32_t body = s_scan[DEFLATE_DT - 1u];
  const uint32_t dyn_bits = s_hbits + body + s_len[256];
  const uint32_t ob = first ? 2u : 0u; // the zlib header in front of a segment's first chunk
  const bool stored = (dyn_bits + 7u) / 8u >= 5u + n;
  uint32_t L; // the chunk's bytes in the file
  if (stored) {
    if (t == 0) {
      outb[ob] = last ? 1u : 0u;
      outb[ob + 1u] = (uint8_t)n; outb[ob + 2u] = (uint8_t)(n >> 8); outb[ob + 3u] = (uint8_t)~n; outb[ob + 4u] = (uint8_t)(~n >> 8);
    }
    for (uint32_t i = t; i < n; i += DEFLATE_DT) outb[ob + 5u + i] = in[i];
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
    deflate_walk(in, lo, hi, head_lo, next_hi, [&](uint32_t lit, uint32_t len) {
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
    const uint32_t cspan = (L + DEFLATE_DT - 1u) / DEFLATE_DT, clo = min(t * cspan, L), chi = min(clo + cspan, L);
    uint32_t x = 0;
    if (p.crc && chi > clo) {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t i = clo; i < chi; ++i) c = s_crc[(c ^ outb[i]) & 255u] ^ (c >> 8);
      x = png_crc_shift(~c, L - chi);
    }
    if (p.crc && t == 0) x ^= png_crc_shift(PNG_CRC_IDAT, L);
    uint32_t sa = 0, sb = 0; // (a lane: at most 64 bytes of 255 at a weight of 32768)
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t v = in[i]; sa += v; sb += (n - i) * v; }
    sb %= DEFLATE_ADLER;
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) { x ^= __shfl_xor(x, s); sa += __shfl_xor(sa, s); sb += __shfl_xor(sb, s); }
    if ((t & 63u) == 0u) { atomicXor(&s_red[0], x); atomicAdd(&s_red[1], sa); atomicAdd(&s_red[2], sb); }
  }
  __syncthreads();
  if (t == 0) {
    uint32_t *m = p.meta + (size_t)k * DEFLATE_META;
    m[0] = L; m[1] = s_red[0]; m[2] = (1u + s_red[1]) % DEFLATE_ADLER; m[3] = (n + s_red[2]) % DEFLATE_ADLER;
  }
  uint32_t *dst = (uint32_t *)(p.scratch + (size_t)k * p.slot_bytes);
  for (uint32_t i = t; i * 4u < L; i += DEFLATE_DT) dst[i] = s_out[i];
}

size_t deflate_dyn_lds(uint32_t cb) { return (((size_t)cb + 3u) / 4u + 1u + ((size_t)cb + DEFLATE_CHUNK_EXTRA + 3u) / 4u + 2u) * 4u; }

} // namespace

size_t deflate_slot_bytes(uint32_t cb) { return ((size_t)cb + DEFLATE_CHUNK_EXTRA + 3u) / 4u * 4u + 4u; }

hipError_t deflate_launch(const DeflateP &p, uint32_t n_chunks, hipStream_t st) {
  const size_t lds = deflate_dyn_lds(p.cb);
  if (lds > 48u * 1024u) {
    const hipError_t err = hipFuncSetAttribute((const void *)k_deflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)deflate_dyn_lds(DEFLATE_CHUNK_MAX));
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_deflate, dim3(n_chunks), dim3(DEFLATE_DT), lds, st, p);
  return hipGetLastError();
}

} // namespace fspt
