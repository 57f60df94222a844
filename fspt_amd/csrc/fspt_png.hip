// fspt_png.hip - a PNG encoder on the GPU: the drawn RGBA8 frame, which draw_launch leaves in device memory,
// becomes a lossless PNG file there, so that only the file's bytes cross the bus.  Integer arithmetic throughout; the bytes
// are tests/png_ref.py's, which states the format: the five filters under the smallest sum of signed magnitudes, deflate in
// independent chunks of literals and distance-1 matches under a length-limited dynamic Huffman code per chunk.
//   k_png_filter    one workgroup per row: the five filters' costs from the raw neighbours, reduced across the workgroup,
//                   then the chosen residuals into the flat stream, a whole dword per lane where the row owns it
//   k_deflate       (fspt_deflate.hip, the OpenEXR encoder's too) one workgroup per chunk of the stream: its deflated bytes, its
//                   Adler pair and its IDAT's CRC-32
//   k_png_offsets   a scan of the chunk lengths (each with an IDAT's 12 bytes): where every IDAT lands; the Adler pairs
//                   combined in chunk order
//   k_png_pack      header and IDATs into one contiguous stream, the Adler IDAT, IEND, the byte count
#include "fspt_internal.hpp"
#include "fspt_encode_device.hpp"
#include "fspt_png_tables.hpp"

namespace fspt {
namespace {

constexpr uint32_t PNG_FT = 256u;       // lanes of a filter workgroup

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
    const uint32_t v = i < n ? meta[(size_t)i * DEFLATE_META] + 12u : 0u;
    const uint32_t a = i < n ? meta[(size_t)i * DEFLATE_META + 2u] + DEFLATE_ADLER - 1u : 0u; // A - 1 mod 65521
    uint32_t *const both[2] = {s, sa};
    const uint32_t vs[2] = {v, i < n ? a % DEFLATE_ADLER : 0u}; // (256 values below 65521)
    enc_scan256(both, vs);
    const uint32_t r = running, ra = running_a;
    if (i < n) {
      off[i] = r + s[t] - v;
      const uint32_t before = (ra + sa[t] - a % DEFLATE_ADLER) % DEFLATE_ADLER; // A - 1 of everything in front of chunk i
      const uint32_t len_in = (uint32_t)min((size_t)cb, stream_bytes - (size_t)i * cb);
      my_b = (uint32_t)((my_b + meta[(size_t)i * DEFLATE_META + 3u] + (uint64_t)(len_in % DEFLATE_ADLER) * before) % DEFLATE_ADLER);
    }
    __syncthreads();
    if (t == 255u) { running = r + s[255]; running_a = (ra + sa[255]) % DEFLATE_ADLER; }
    __syncthreads();
  }
  atomicAdd(&sum_b, my_b);
  __syncthreads();
  if (t == 0) {
    off[n] = running; off[n + 1u] = running + 16u + 12u;
    off[n + 2u] = ((sum_b % DEFLATE_ADLER) << 16) | ((1u + running_a) % DEFLATE_ADLER);
  }
}

__device__ __forceinline__ void png_put_be(uint8_t *o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }

__global__ void __launch_bounds__(256) k_png_pack(const uint8_t *__restrict__ hdr, uint32_t hdr_len, const uint8_t *__restrict__ scratch, size_t slot_bytes,
                                                   const uint32_t *__restrict__ meta, const uint32_t *__restrict__ off, uint32_t n, uint8_t *__restrict__ out) {
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  if (k == 0) for (uint32_t i = t; i < hdr_len; i += 256u) out[i] = hdr[i];
  const uint8_t *src = scratch + (size_t)k * slot_bytes;
  const uint32_t L = meta[(size_t)k * DEFLATE_META];
  uint8_t *dst = out + off[k];
  for (uint32_t i = t; i < L; i += 256u) dst[8u + i] = src[i];
  if (t == 0) {
    png_put_be(dst, L);
    dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    png_put_be(dst + 8u + L, meta[(size_t)k * DEFLATE_META + 1u]);
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

uint32_t host_crc(const uint8_t *d, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = PNG_CRC_TABLE[(c ^ d[i]) & 255u] ^ (c >> 8);
  return ~c;
}

size_t png_bound_of(uint32_t w, uint32_t h, uint32_t channels, uint32_t cb) {
  const size_t stream = (size_t)h * (1u + (size_t)w * channels);
  return 8u + 25u + 2u + 16u + 12u + stream + (stream + cb - 1u) / cb * (5u + 5u + 12u);
}

} // namespace

static const fspt_png_params PNG_DEFAULTS = {3u, (uint32_t)FSPT_PNG_FILTER_ADAPTIVE, FSPT_PNG_CHUNK};

int png_check_params(const fspt_png_params *prm, const char *fn) {
  const fspt_png_params q = prm ? *prm : PNG_DEFAULTS;
  if (q.channels != 0u && q.channels != 3u && q.channels != 4u) { fspt_set_error("%s: channels must be 3 or 4", fn); return FSPT_E_INVALID; }
  if (q.filter > (uint32_t)FSPT_PNG_FILTER_ADAPTIVE) { fspt_set_error("%s: unknown filter %u", fn, q.filter); return FSPT_E_INVALID; }
  if (q.chunk_bytes != 0u && (q.chunk_bytes < DEFLATE_CHUNK_MIN || q.chunk_bytes > DEFLATE_CHUNK_MAX)) { fspt_set_error("%s: chunk_bytes must be 0 or in 256..32768", fn); return FSPT_E_INVALID; }
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

// The encoder's device memory for `pl`: the header once per (size, parameters), the work buffers, and n_out (0 or 1) output
// buffers of out_bytes (>= pl.bound; it outlives a change of the parameters and grows).  Nothing of it may be in use.
hipError_t png_ensure(PngEnc &e, const PngPlan &pl, int n_out, size_t out_bytes) {
  hipError_t err = enc_ensure_out(e.c, n_out, out_bytes);
  if (err != hipSuccess || (e.c.valid && same_plan(e.pl, pl))) return err;
  enc_replan(e.c);
  uint8_t hdr[PNG_HEADER_BYTES] = {137, 80, 78, 71, 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                   (uint8_t)(pl.w >> 24), (uint8_t)(pl.w >> 16), (uint8_t)(pl.w >> 8), (uint8_t)pl.w,
                                   (uint8_t)(pl.h >> 24), (uint8_t)(pl.h >> 16), (uint8_t)(pl.h >> 8), (uint8_t)pl.h,
                                   8, (uint8_t)(pl.channels == 3u ? 2 : 6), 0, 0, 0};
  const uint32_t c = host_crc(hdr + 12, 17);
  hdr[29] = (uint8_t)(c >> 24); hdr[30] = (uint8_t)(c >> 16); hdr[31] = (uint8_t)(c >> 8); hdr[32] = (uint8_t)c;
  enc_make(e.c, err, e.cfg, 64);
  enc_make(e.c, err, e.stream, (pl.stream_bytes + 3u) / 4u * 4u + 4u);
  enc_make(e.c, err, e.scratch, (size_t)pl.n_chunks * pl.slot_bytes);
  enc_make(e.c, err, e.meta, ((size_t)pl.n_chunks * (DEFLATE_META + 1u) + 3u) * 4u);
  e.off = e.meta ? e.meta + (size_t)pl.n_chunks * DEFLATE_META : nullptr;
  if (err == hipSuccess) err = hipMemcpy(e.cfg, hdr, sizeof hdr, hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  e.pl = pl; e.c.valid = true;
  return hipSuccess;
}

hipError_t png_launch_filter(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st) {
  const PngPlan &pl = e.pl;
  PngFilterP f{rgba, pl.w, pl.h, bottom_up ? 1u : 0u, pl.channels, pl.filter, pl.row_bytes, e.stream};
  hipLaunchKernelGGL(k_png_filter, dim3(pl.h), dim3(PNG_FT), 0, st, f);
  return hipGetLastError();
}

// The whole encode of `rgba` (device memory, w x h texels) into e.c.out[0] on `st`; the file's length lands in
// e.off[n_chunks + 1].  Events 0..3 bracket the three stages.  No host read, no synchronisation.
hipError_t png_launch(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st) {
  const PngPlan &pl = e.pl;
  hipError_t err = hipEventRecord(e.c.ev[0], st);
  if (err == hipSuccess) err = png_launch_filter(e, rgba, bottom_up, st);
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[1], st);
  if (err != hipSuccess) return err;
  const DeflateP d{e.stream, pl.stream_bytes, pl.stream_bytes, pl.cb, pl.n_chunks, 1u, e.scratch, pl.slot_bytes, e.meta}; // one segment
  err = deflate_launch(d, pl.n_chunks, st);
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[2], st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_png_offsets, dim3(1), dim3(256), 0, st, (const uint32_t *)e.meta, pl.n_chunks, PNG_HEADER_BYTES, pl.cb, pl.stream_bytes, e.off);
  hipLaunchKernelGGL(k_png_pack, dim3(pl.n_chunks), dim3(256), 0, st, (const uint8_t *)e.cfg, PNG_HEADER_BYTES, (const uint8_t *)e.scratch, pl.slot_bytes,
                     (const uint32_t *)e.meta, (const uint32_t *)e.off, pl.n_chunks, e.c.out[0]);
  err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(e.c.ev[3], st);
  return err;
}

int png_collect(PngEnc &e, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn) {
  return enc_collect(e.off + e.pl.n_chunks + 1u, e.c.out[0], out, cap, bytes_out, st, fn, g_png_format);
}

} // namespace fspt

// The stand-alone entries: NULL and range checks first, then the device.  stream_out: fspt_png_filtered_eval's form, stage
// one alone and its stream copied back.
static int png_encode_any(const char *fn, int device, const uint8_t *rgba8, bool on_device, uint32_t w, uint32_t h, int bottom_up,
                          const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out, uint8_t *stream_out) {
  if (!rgba8 || (stream_out ? false : !out || !bytes_out)) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  fspt::PngPlan pl;
  const int rc = fspt::png_plan(p, w, h, true, fn, pl);
  if (rc) return rc;
  fspt::PngEnc e;
  const auto launch = [&](fspt::Hold &hold) {
    const void *src = rgba8;
    hipError_t err = on_device ? hipSuccess : fspt::enc_upload(hold, rgba8, (size_t)w * h * 4, &src);
    if (err == hipSuccess) err = stream_out ? fspt::png_launch_filter(e, (const uint32_t *)src, bottom_up, nullptr) : fspt::png_launch(e, (const uint32_t *)src, bottom_up, nullptr);
    if (err == hipSuccess && stream_out) err = hipMemcpy(stream_out, e.stream, pl.stream_bytes, hipMemcpyDeviceToHost);
    return err;
  };
  const auto ensure = [&] { return fspt::png_ensure(e, pl, stream_out ? 0 : 1, pl.bound); };
  if (stream_out) return fspt::enc_run(fn, device, e.c, fspt::g_png_format, ensure, launch, nullptr);
  return fspt::enc_run(fn, device, e.c, fspt::g_png_format, ensure, launch, [&] { return fspt::png_collect(e, nullptr, out, cap, bytes_out, fn); });
}

extern "C" {

int fspt_png_bound(uint32_t w, uint32_t h, const fspt_png_params *p, size_t *bytes) {
  return fspt::enc_bound<fspt::PngPlan>("fspt_png_bound", bytes, [&](fspt::PngPlan &pl) { return fspt::png_plan(p, w, h, false, "fspt_png_bound", pl); });
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

int fspt_png_last_ms(float ms[3], uint64_t *bus_bytes) { return fspt::enc_last_ms(fspt::g_png_format, "fspt_png_last_ms", ms, bus_bytes); }

} // extern "C"
