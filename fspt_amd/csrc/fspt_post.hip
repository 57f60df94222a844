// fspt_post.hip - the image-space kernels of libfspt: the device side of fspt_post.cpp.  The rule that divides the kernel
// files: whatever reads a DScene is fspt_kernels.hip (the renderers) or fspt_passes.hip (the stand-alone passes, among them
// the two of the image chain that trace rays: k_features, k_temporal_gbuffer); this file holds whatever reads only images - the draw,
// bloom, auto-exposure, the a-trous filter, the temporal blend, the history clamp and the SVGF variance estimate - with
// their launchers.  Nothing the path tracer's benchmark times lives here.
#include "fspt_device.hpp"
#include "fspt_math.hpp"

namespace fspt {
using namespace fm;

#define WAVE 64
#define BLOCK_THREADS 256

// draw.fs (1-93): exposure -> ACES fit -> saturation -> gamma (+ optional 5x5 firefly filter) -> RGBA8
FM_DEV float draw_luma(V3 c) { return dot(c, v3(0.2126f, 0.7152f, 0.0722f)); }
FM_DEV V3 draw_fetch(const float4 *acc, int W, int H, int x, int y) {
  if (x < 0 || y < 0 || x >= W || y >= H) return v3(0.0f, 0.0f, 0.0f);
  float4 p = acc[(size_t)y * W + x];
  return v3(p.x, p.y, p.z);
}
FM_DEV float rrt_odt(float v) {
  float a = fma_(v, v + 0.0245786f, -0.000090537f);
  float b = fma_(v, fma_(0.983729f, v, 0.4329510f), 0.238081f);
  return a / b;
}
// Bloom, the two pieces the draw and the pyramid kernels share.  s(v) = v >= 0 ? min(v, 1024) : 0: NaN and
// negatives become 0, +inf the path kernels' own per-sample clamp.  up(U)(x, y): the 2 x 2 tent over the coarser level U
// (w x h), 3/4 on the texel under (x, y) and 1/4 on its neighbour towards (x, y)'s side, clamped; horizontal first:
// fma(3/4, fma(3/4, U00, U10 / 4), fma(3/4, U01, U11 / 4) / 4).  The weights are dyadic: the three fma round, nothing else.
constexpr float BLOOM_CLAMP = 1024.0f;
FM_DEV float bloom_s(float v) { return v >= 0.0f ? (v < BLOOM_CLAMP ? v : BLOOM_CLAMP) : 0.0f; }
FM_DEV V3 bloom_s3(V3 c) { return v3(bloom_s(c.x), bloom_s(c.y), bloom_s(c.z)); }
FM_DEV float bloom_tent(float u00, float u10, float u01, float u11) {
  return fma_(0.75f, fma_(0.75f, u00, 0.25f * u10), 0.25f * fma_(0.75f, u01, 0.25f * u11));
}
FM_DEV V3 bloom_up(const float4 *U, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
  const uint32_t cx0 = x >> 1, cy0 = y >> 1;
  const uint32_t cx1 = (x & 1u) ? (cx0 + 1u < w ? cx0 + 1u : w - 1u) : (cx0 ? cx0 - 1u : 0u);
  const uint32_t cy1 = (y & 1u) ? (cy0 + 1u < h ? cy0 + 1u : h - 1u) : (cy0 ? cy0 - 1u : 0u);
  const float4 a = U[(size_t)cy0 * w + cx0], b = U[(size_t)cy0 * w + cx1], c = U[(size_t)cy1 * w + cx0], d = U[(size_t)cy1 * w + cx1];
  return v3(bloom_tent(a.x, b.x, c.x, d.x), bloom_tent(a.y, b.y, c.y, d.y), bloom_tent(a.z, b.z, c.z, d.z));
}
// what the draw multiplies by the exposure: c' = fma(intensity, B - s(c), s(c)), B = up(U_1) at the source texel (x, y)
FM_DEV V3 bloom_mix(V3 c, V3 B, float intensity) {
  const V3 c0 = bloom_s3(c);
  return v3(fma_(intensity, B.x - c0.x, c0.x), fma_(intensity, B.y - c0.y, c0.y), fma_(intensity, B.z - c0.z, c0.z));
}
template <bool BLOOM>
FM_DEV void draw_pixel(const float4 *acc, uint32_t W, uint32_t H, float exposure, float saturation, int denoise, float maxSigma,
                       float scale, uint32_t *out, const BloomDraw &bl) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  // ivec2(gl_FragCoord * scale) (draw.fs:59,87): the reference draws with scale 0.25 while the camera moves
  int x = (int)(((float)(i % W) + 0.5f) * scale), y = (int)(((float)(i / W) + 0.5f) * scale);
  V3 c;
  if (denoise) {
    float sum = 0.0f, sq = 0.0f, middleLuma = 0.0f;
    V3 middle = v3(0.0f, 0.0f, 0.0f);
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b) {
        int ox = a - 2, oy = b - 2;
        V3 col = draw_fetch(acc, (int)W, (int)H, x + ox, y + oy);
        float l = draw_luma(col);
        if (ox == 0 && oy == 0) { middle = col; middleLuma = l; continue; }
        sum += l;
        sq = fma_(l, l, sq);
      }
    float mean = sum / 24.0f;
    float variance = fma_(-mean, mean, sq / 24.0f);
    float sigma = sqrt_(variance);
    if (abs_(middleLuma - mean) > maxSigma * sigma) middle = middle * (mean / middleLuma);
    c = middle;
  } else {
    c = draw_fetch(acc, (int)W, (int)H, x, y);
  }
  if (BLOOM) { // (a source texel outside the viewport is drawn plain)
    if (x >= 0 && y >= 0 && (uint32_t)x < bl.vw && (uint32_t)y < bl.vh) c = bloom_mix(c, bloom_up(bl.u1, bl.w1, bl.h1, (uint32_t)x, (uint32_t)y), bl.intensity);
  }
  c = c * exposure;
  V3 a = v3(dot(c, v3(0.59719f, 0.35458f, 0.04823f)), dot(c, v3(0.07600f, 0.90834f, 0.01566f)),
            dot(c, v3(0.02840f, 0.13383f, 0.83777f)));
  a = v3(rrt_odt(a.x), rrt_odt(a.y), rrt_odt(a.z));
  V3 m = v3(dot(a, v3(1.60475f, -0.53108f, -0.07367f)), dot(a, v3(-0.10208f, 1.10813f, -0.00605f)),
            dot(a, v3(-0.00327f, -0.07276f, 1.07602f)));
  m = v3(clamp_(m.x, 0.0f, 1.0f), clamp_(m.y, 0.0f, 1.0f), clamp_(m.z, 0.0f, 1.0f));
  float l = draw_luma(m);
  float os = 1.0f - saturation;
  m = v3(fma_(m.x, saturation, l * os), fma_(m.y, saturation, l * os), fma_(m.z, saturation, l * os));
  float g0 = pow_(m.x, 0.454545f), g1 = pow_(m.y, 0.454545f), g2 = pow_(m.z, 0.454545f);
  uint32_t r8 = (uint32_t)floor_(fma_(clamp_(g0, 0.0f, 1.0f), 255.0f, 0.5f));
  uint32_t g8 = (uint32_t)floor_(fma_(clamp_(g1, 0.0f, 1.0f), 255.0f, 0.5f));
  uint32_t b8 = (uint32_t)floor_(fma_(clamp_(g2, 0.0f, 1.0f), 255.0f, 0.5f));
  out[i] = r8 | (g8 << 8) | (b8 << 16) | 0xFF000000u;
}
__global__ __launch_bounds__(BLOCK_THREADS) void k_draw(const float4 *acc, uint32_t W, uint32_t H, float exposure,
                                                       float saturation, int denoise, float maxSigma, float scale,
                                                       uint32_t *out) {
  draw_pixel<false>(acc, W, H, exposure, saturation, denoise, maxSigma, scale, out, BloomDraw{});
}
// Auto-exposure: the caller's exposure becomes a compensation of the metered one, read from device memory
// (k_exposure_resolve wrote it on this stream, or on one ordered before it); everything after the product is k_draw.
__global__ __launch_bounds__(BLOCK_THREADS) void k_draw_auto(const float4 *acc, uint32_t W, uint32_t H, float exposure,
                                                            float saturation, int denoise, float maxSigma, float scale,
                                                            uint32_t *out, const ExposureState *state) {
  draw_pixel<false>(acc, W, H, exposure * state->exposure, saturation, denoise, maxSigma, scale, out, BloomDraw{});
}
// Bloom (the rule in full: fspt_tuning.h).  k_draw_bloom is draw_pixel with the mix in front of the exposure:
// c' = fma(intensity, up(U_1)(x, y) - s(c), s(c)) at the source texel, c the texel or the firefly-filtered middle.  AUTO reads
// the exposure record as k_draw_auto does.
template <bool AUTO>
__global__ __launch_bounds__(BLOCK_THREADS) void k_draw_bloom(const float4 *acc, uint32_t W, uint32_t H, float exposure,
                                                             float saturation, int denoise, float maxSigma, float scale,
                                                             uint32_t *out, const ExposureState *state, const BloomDraw bl) {
  draw_pixel<true>(acc, W, H, AUTO ? exposure * state->exposure : exposure, saturation, denoise, maxSigma, scale, out, bl);
}
// B and c' of every viewport texel with denoise = 0, through the draw's own device functions (fspt_bloom_eval, a test hook):
// bloom_out is vw x vh, mix_out W x H (outside the viewport: the source, as the draw draws it plain); .w = the source's
__global__ __launch_bounds__(BLOCK_THREADS) void k_bloom_mix(const float4 *src, uint32_t W, uint32_t H, const BloomDraw bl,
                                                            float4 *bloom_out, float4 *mix_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t x = i % W, y = i / W;
  const float4 p = src[i];
  if (x >= bl.vw || y >= bl.vh) { mix_out[i] = p; return; }
  const V3 B = bloom_up(bl.u1, bl.w1, bl.h1, x, y);
  const V3 m = bloom_mix(v3(p.x, p.y, p.z), B, bl.intensity);
  bloom_out[(size_t)y * bl.vw + x] = make_float4(B.x, B.y, B.z, p.w);
  mix_out[i] = make_float4(m.x, m.y, m.z, p.w);
}

// One 1-D pass of the down filter, w = (1, 3, 3, 1) / 8: ((a1 + a2) 3 + (a0 + a3)) / 8 - three additions and the product by 3
// round (3 m is m + 2 m rounded once), the division by 8 is exact.
FM_DEV float bloom_down4(float a0, float a1, float a2, float a3) {
  const float m = a1 + a2;
  return (3.0f * m + (a0 + a3)) * 0.125f;
}
// D_{k+1} from S_k (ws x hs texels at a pitch of `pitch`), separable, horizontal first.  A workgroup makes a 32 x 8 tile of
// outputs: it stages the 66 x 18 source texels the tile needs (coordinates clamped to the level: every load is in bounds) with
// 16-byte loads into three planes of LDS, FIRST sanitising them; the horizontal pass of the 18 rows goes into LDS, the vertical
// pass out of it.  Without the staging a source texel would be fetched up to four times through the caches.  LDS: a plane's
// rows are 66 floats (even, so a row starts 8-byte aligned); in the horizontal pass lane x reads columns 2 x .. 2 x + 3 as two
// 8-byte reads - 32 lanes at a stride of 8 bytes cover the 64 banks once, and the wave's other half reads another row in its
// own group; in the vertical pass lane x reads column x: consecutive dwords.
constexpr uint32_t BLOOM_TX = 32, BLOOM_TY = 8, BLOOM_SX = 2 * BLOOM_TX + 2, BLOOM_SY = 2 * BLOOM_TY + 2;
static_assert(BLOOM_TX * BLOOM_TY == BLOCK_THREADS && BLOOM_SX % 2 == 0, "one output per thread; 8-byte aligned rows");
template <bool FIRST>
__global__ __launch_bounds__(BLOCK_THREADS) void k_bloom_down(const float4 *src, uint32_t pitch, uint32_t ws, uint32_t hs, float4 *dst,
                                                             uint32_t wd, uint32_t hd) {
  __shared__ __attribute__((aligned(16))) float s[3][BLOOM_SY][BLOOM_SX];
  __shared__ float t[3][BLOOM_SY][BLOOM_TX];
  const int x0 = 2 * (int)(blockIdx.x * BLOOM_TX) - 1, y0 = 2 * (int)(blockIdx.y * BLOOM_TY) - 1;
  for (uint32_t k = threadIdx.x; k < BLOOM_SX * BLOOM_SY; k += BLOCK_THREADS) {
    const uint32_t i = k % BLOOM_SX, j = k / BLOOM_SX;
    int sx = x0 + (int)i, sy = y0 + (int)j;
    sx = sx < 0 ? 0 : (sx > (int)ws - 1 ? (int)ws - 1 : sx);
    sy = sy < 0 ? 0 : (sy > (int)hs - 1 ? (int)hs - 1 : sy);
    const float4 p = src[(size_t)sy * pitch + sx];
    s[0][j][i] = FIRST ? bloom_s(p.x) : p.x;
    s[1][j][i] = FIRST ? bloom_s(p.y) : p.y;
    s[2][j][i] = FIRST ? bloom_s(p.z) : p.z;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < BLOOM_TX * BLOOM_SY; k += BLOCK_THREADS) {
    const uint32_t x = k % BLOOM_TX, j = k / BLOOM_TX;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float2 a = *(const float2 *)&s[c][j][2 * x], b = *(const float2 *)&s[c][j][2 * x + 2];
      t[c][j][x] = bloom_down4(a.x, a.y, b.x, b.y);
    }
  }
  __syncthreads();
  const uint32_t tx = threadIdx.x % BLOOM_TX, ty = threadIdx.x / BLOOM_TX;
  const uint32_t x = blockIdx.x * BLOOM_TX + tx, y = blockIdx.y * BLOOM_TY + ty;
  if (x >= wd || y >= hd) return;
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = bloom_down4(t[c][2 * ty][tx], t[c][2 * ty + 1][tx], t[c][2 * ty + 2][tx], t[c][2 * ty + 3][tx]);
  dst[(size_t)y * wd + x] = make_float4(o[0], o[1], o[2], 0.0f);
}

// U_k = fma(scatter, up(U_{k+1}) - D_k, D_k), one thread per texel, in place over D_k (a thread reads only its own D_k texel)
__global__ __launch_bounds__(BLOCK_THREADS) void k_bloom_up(float4 *dk, uint32_t w, uint32_t h, const float4 *up, uint32_t wu, uint32_t hu,
                                                           float scatter) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const V3 u = bloom_up(up, wu, hu, i % w, i / w);
  const float4 d = dk[i];
  dk[i] = make_float4(fma_(scatter, u.x - d.x, d.x), fma_(scatter, u.y - d.y, d.y), fma_(scatter, u.z - d.z, d.z), 0.0f);
}

// The pyramid's small end in one workgroup: level k (w x h, in global memory) is loaded into LDS, every lower level is built
// there, combined back up in place, and U_k is written over D_k.  2 (n - k) launches become one.  LDS holds the levels one
// behind the other, three floats a texel (a stride of three dwords: no bank conflict); the host sizes it (bloom_plan) and
// starts the tail only where it fits.  The operations and their order are the per-level kernels': a texel's four horizontal
// passes are recomputed per output instead of stored, which gives the same bits.  dbg_down / dbg_up (NULL in a draw): where
// D_j and U_j of the levels below k go, one behind the other, for fspt_bloom_eval.
constexpr uint32_t BLOOM_TAIL_THREADS = 1024;
FM_DEV uint32_t bloom_cl(int v, uint32_t n) { return v < 0 ? 0u : ((uint32_t)v > n - 1u ? n - 1u : (uint32_t)v); }
__global__ __launch_bounds__(BLOOM_TAIL_THREADS) void k_bloom_tail(const BloomTailP p) {
  extern __shared__ float lds[];
  const uint32_t n0 = p.w * p.h;
  for (uint32_t i = threadIdx.x; i < n0; i += BLOOM_TAIL_THREADS) {
    const float4 v = p.lvl[i];
    lds[3 * i] = v.x; lds[3 * i + 1] = v.y; lds[3 * i + 2] = v.z;
  }
  __syncthreads();
  // down: level j at `at` (ws x hs) -> level j + 1 behind it
  uint32_t at = 0, ws = p.w, hs = p.h, dbg = 0;
  for (uint32_t j = 0; j < p.below; ++j) {
    const uint32_t wd = (ws + 1u) >> 1, hd = (hs + 1u) >> 1, to = at + ws * hs;
    const float *S = lds + 3 * (size_t)at;
    for (uint32_t i = threadIdx.x; i < wd * hd; i += BLOOM_TAIL_THREADS) {
      const uint32_t x = i % wd, y = i / wd;
      uint32_t cx[4], cy[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { cx[q] = bloom_cl(2 * (int)x - 1 + q, ws); cy[q] = bloom_cl(2 * (int)y - 1 + q, hs); }
      float o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float *row = S + 3 * (size_t)(cy[q] * ws) + c;
          r[q] = bloom_down4(row[3 * cx[0]], row[3 * cx[1]], row[3 * cx[2]], row[3 * cx[3]]);
        }
        o[c] = bloom_down4(r[0], r[1], r[2], r[3]);
        lds[3 * (size_t)(to + i) + c] = o[c];
      }
      if (p.dbg_down) p.dbg_down[dbg + i] = make_float4(o[0], o[1], o[2], 0.0f);
    }
    __syncthreads();
    dbg += wd * hd;
    at = to; ws = wd; hs = hd;
  }
  // U of the last level is its D
  if (p.dbg_up && p.below)
    for (uint32_t i = threadIdx.x; i < ws * hs; i += BLOOM_TAIL_THREADS)
      p.dbg_up[dbg - ws * hs + i] = make_float4(lds[3 * (size_t)(at + i)], lds[3 * (size_t)(at + i) + 1], lds[3 * (size_t)(at + i) + 2], 0.0f);
  // up: level j + 1 at `at` (ws x hs) -> level j in front of it, whose size comes from walking down from the top again
  for (uint32_t j = p.below; j-- > 0;) {
    uint32_t wf = p.w, hf = p.h, af = 0, df = 0; // level j of the tail: size, LDS offset, debug offset of its END
    for (uint32_t q = 0; q < j; ++q) { af += wf * hf; wf = (wf + 1u) >> 1; hf = (hf + 1u) >> 1; df += wf * hf; }
    const float *U = lds + 3 * (size_t)at;
    for (uint32_t i = threadIdx.x; i < wf * hf; i += BLOOM_TAIL_THREADS) {
      const uint32_t x = i % wf, y = i / wf;
      const uint32_t cx0 = x >> 1, cy0 = y >> 1;
      const uint32_t cx1 = (x & 1u) ? (cx0 + 1u < ws ? cx0 + 1u : ws - 1u) : (cx0 ? cx0 - 1u : 0u);
      const uint32_t cy1 = (y & 1u) ? (cy0 + 1u < hs ? cy0 + 1u : hs - 1u) : (cy0 ? cy0 - 1u : 0u);
      float o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = bloom_tent(U[3 * (size_t)(cy0 * ws + cx0) + c], U[3 * (size_t)(cy0 * ws + cx1) + c], U[3 * (size_t)(cy1 * ws + cx0) + c],
                                   U[3 * (size_t)(cy1 * ws + cx1) + c]);
        const float d = lds[3 * (size_t)(af + i) + c];
        o[c] = fma_(p.scatter, u - d, d);
        lds[3 * (size_t)(af + i) + c] = o[c];
      }
      if (j == 0) p.lvl[i] = make_float4(o[0], o[1], o[2], 0.0f);
      else if (p.dbg_up) p.dbg_up[df - wf * hf + i] = make_float4(o[0], o[1], o[2], 0.0f);
    }
    __syncthreads();
    at = af; ws = wf; hs = hf;
  }
}

// The luminance histogram of the viewport: 256 bins, piecewise-linear in log2 and taken from the float's bits -
// 32 octaves from 2^-16 with 8 sub-bins each; !(L >= 2^-16) (zero, negatives, NaN, denormals) is left out, +inf and
// everything from 2^16 up lands in bin 255.  A fixed grid strides over the viewport's pixels (16-byte loads), every block
// counts in LDS and adds its non-zero bins to the global histogram with integer atomics: sums of integers, so the result
// does not depend on the order.  COMBINE: flat walls or a sky put a whole wave into one bin, and 64 LDS atomics on one
// address run one after the other; the lanes that share the first active lane's bin are counted by a ballot and added by
// that lane alone, the rest add for themselves.  Measured: no difference at 1920 x 1080, the plain form ships.
constexpr uint32_t EXPOSURE_GRID = 512; // blocks at most: the global flush is <= 512 x (non-zero bins) atomics
FM_DEV int exposure_bin(float4 p) {
  const float L = draw_luma(v3(p.x, p.y, p.z));
  if (!(L >= 1.52587890625e-05f)) return -1; // 2^-16
  const uint32_t b = (__float_as_uint(L) >> 20) - ((127u - 16u) << 3);
  return (int)(b < 255u ? b : 255u);
}
template <bool COMBINE>
__global__ __launch_bounds__(BLOCK_THREADS) void k_exposure_histogram(const float4 *src, uint32_t W, uint32_t vw, uint32_t vh,
                                                                     uint32_t *hist) {
  __shared__ uint32_t h[EXPOSURE_BINS];
  for (uint32_t k = threadIdx.x; k < EXPOSURE_BINS; k += blockDim.x) h[k] = 0u;
  __syncthreads();
  const uint32_t n = vw * vh;
  // (the loop bound is the same for every lane of a block: the ballot below sees whole waves)
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    int bin = -1;
    if (i < n) bin = exposure_bin(src[vw == W ? (size_t)i : (size_t)(i / vw) * W + i % vw]);
    if (COMBINE) {
      const unsigned long long act = __ballot(bin >= 0);
      if (act) {
        const int leader = __builtin_ctzll(act);
        const int lb = __shfl(bin, leader, WAVE);
        const unsigned long long same = __ballot(bin == lb);
        if ((int)(threadIdx.x & (WAVE - 1)) == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        else if (bin >= 0 && bin != lb) atomicAdd(&h[bin], 1u);
      }
    } else {
      if (bin >= 0) atomicAdd(&h[bin], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < EXPOSURE_BINS; k += blockDim.x) {
    const uint32_t c = h[k];
    if (c) atomicAdd(&hist[k], c);
  }
}

// log2(1 + (m + 0.5) / 8), m = 0..7: the centre of a sub-bin, linear in the mantissa (memory, not a lane's array: no scratch)
__device__ const double EXPOSURE_SUB[8] = {0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128, 0.6438561897747247, 0.7548875021634686, 0.8579809951275721, 0.9541963103868752};
// The metered exposure from the histogram, one block, float64: the pixels between the low and high
// percentiles by bin, their mean log2 luminance from the bins' centres, the exposure that puts it at the key, adapted from
// the previous state in log2 and clamped.  The 256 terms are summed in ascending order by one lane; the block reads the
// counts and zeroes the histogram for the next metering.  N = 0 leaves the state as it is.  Vector stores only.
__global__ __launch_bounds__(EXPOSURE_BINS) void k_exposure_resolve(uint32_t *hist, ExposureState *state, const ExposureP p) {
  __shared__ uint32_t cnt[EXPOSURE_BINS];
  cnt[threadIdx.x] = hist[threadIdx.x];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint64_t N = 0;
  for (int b = 0; b < (int)EXPOSURE_BINS; ++b) N += cnt[b];
  if (N == 0) return;
  const uint64_t r0 = (uint64_t)floor((double)p.low * (double)N), r1 = (uint64_t)ceil((double)p.high * (double)N);
  uint64_t at = 0, K = 0;
  double sum = 0.0;
  for (int b = 0; b < (int)EXPOSURE_BINS; ++b) {
    const uint64_t lo = at > r0 ? at : r0, hi = at + cnt[b] < r1 ? at + cnt[b] : r1;
    at += cnt[b];
    if (hi <= lo) continue;
    const double v = (double)((b >> 3) - 16) + EXPOSURE_SUB[b & 7];
    sum += (double)(hi - lo) * v;
    K += hi - lo;
  }
  const double mean = sum / (double)K;
  const double target = log2((double)p.key) - mean;
  double e = target;
  if (state->valid) {
    const double prev = state->log2_exposure;
    e = prev + (target - prev) * (double)(target < prev ? p.adapt_up : p.adapt_down);
  }
  e = e < (double)p.min_log2 ? (double)p.min_log2 : e > (double)p.max_log2 ? (double)p.max_log2 : e;
  state->exposure = (float)exp2(e);
  state->log2_exposure = e;
  state->log2_mean = mean;
  state->metered = (uint32_t)N;
  state->valid = 1u;
}

// ---- guided denoiser: the a-trous filter; its guide buffers come from k_features (fspt_passes.hip) -----------------
// One iteration of the edge-avoiding a-trous filter (include/fspt.h): 5 x 5 B3 taps `step` pixels apart,
// weighted by luminance, normal and depth similarity; 16 x 16-pixel blocks, every tap read through the caches.  The first
// iteration reads the accumulator and divides the albedo out on the fly (u0 = c / max(a, 1e-3)); the last multiplies
// it back in.
FM_DEV float luma(float4 u) { return (0.2126f * u.x + 0.7152f * u.y) + 0.0722f * u.z; }
FM_DEV float4 atrous_load(const AtrousP &p, size_t q, float4 f0) {
  float4 u = p.src[q];
  if (p.demod) u = make_float4(u.x / max_(f0.x, 1e-3f), u.y / max_(f0.y, 1e-3f), u.z / max_(f0.z, 1e-3f), 1.0f);
  return u;
}
// the variance a tap of the variance-guided instantiation reads: the first iteration's from k_svgf_variance's buffer, a
// later one's from the .w lane the iteration before wrote
FM_DEV float atrous_var(const AtrousP &p, size_t q) { return p.demod ? p.var[q] : p.src[q].w; }
// VAR: the luminance weight is exp(-|Lp - Lq| / (sl sqrt(gv_p) + 1e-4)), gv_p the 3 x 3 binomial blur of the
// input variance around p, and the variance is filtered along (sum w^2 var / (sum w)^2) in the .w lane
template <bool VAR>
__global__ __launch_bounds__(BLOCK_THREADS) void k_atrous(const AtrousP p) {
  const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int W = (int)p.W, H = (int)p.H;
  if (x >= W || y >= H) return;
  const float B[5] = {1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f};
  const size_t ip = (size_t)y * W + x;
  const float4 fp0 = p.feat[2 * ip], fp1 = p.feat[2 * ip + 1];
  const float4 up = atrous_load(p, ip, fp0);
  const float Lp = luma(up);
  const float lenp = sqrt_(fma_(fp1.z, fp1.z, fma_(fp1.y, fp1.y, fp1.x * fp1.x)));
  const bool hp = fp1.w != 0.0f;
  const float zden = p.sz_step * max_(fp0.w, 1e-3f); // sigma_z * step * max(z_p, 1e-3)
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
  float sv = 0.0f, lden = 0.0f;
  if (VAR && p.sl != INFINITY) {
    const float G[3] = {0.25f, 0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
    for (int j = -1; j <= 1; ++j) {
      const int yy = y + j;
      if (yy < 0 || yy >= H) continue;
      for (int i = -1; i <= 1; ++i) {
        const int xx = x + i;
        if (xx < 0 || xx >= W) continue;
        const float g = G[i + 1] * G[j + 1];
        gs = fma_(g, atrous_var(p, (size_t)yy * W + xx), gs);
        gw += g;
      }
    }
    lden = p.sl * sqrt_(gs / gw) + 1e-4f;
  }
  for (int j = -2; j <= 2; ++j) {
    const int yy = y + j * p.step;
    if (yy < 0 || yy >= H) continue;
    for (int i = -2; i <= 2; ++i) {
      const int xx = x + i * p.step;
      if (xx < 0 || xx >= W) continue;
      const size_t iq = (size_t)yy * W + xx;
      const float4 fq0 = p.feat[2 * iq], fq1 = p.feat[2 * iq + 1];
      const float4 uq = atrous_load(p, iq, fq0);
      float w = B[i + 2] * B[j + 2];
      if (VAR) {
        if (p.sl != INFINITY) w *= exp2f(-(abs_(Lp - luma(uq)) / lden) * 1.44269504f);
      } else if (p.sc_step != INFINITY) {
        const float Lq = luma(uq);
        w *= exp2f(-(abs_(Lp - Lq) / (p.sc_step * (Lp + Lq) + 1e-4f)) * 1.44269504f);
      }
      if (p.sn != 0.0f && (i != 0 || j != 0)) {
        const bool hq = fq1.w != 0.0f;
        if (hp || hq) {
          const float lenq = sqrt_(fma_(fq1.z, fq1.z, fma_(fq1.y, fq1.y, fq1.x * fq1.x)));
          if (hp != hq || lenp == 0.0f || lenq == 0.0f) w = 0.0f;
          else {
            // clamped: for two equal normals the float32 cosine rounds to 1 + 2^-23 about one time in five, and
            // (1 + 2^-23)^sn exceeds 1 (inf from sn ~ 1e9 on: sw = inf, the pixel NaN)
            const float c = min_(fma_(fp1.z, fq1.z, fma_(fp1.y, fq1.y, fp1.x * fq1.x)) / (lenp * lenq), 1.0f);
            w *= c > 0.0f ? exp2f(p.sn * log2f(c)) : 0.0f;
          }
        }
      }
      // equal depths weigh 1: zden underflows to 0 for a tiny sigma_depth, and 0 / 0 would make the centre tap NaN
      const float dz = abs_(fp0.w - fq0.w);
      if (p.sz_step != INFINITY && dz != 0.0f) w *= exp2f(-(dz / zden) * 1.44269504f);
      sr = fma_(w, uq.x, sr); sg = fma_(w, uq.y, sg); sb = fma_(w, uq.z, sb);
      sw += w;
      if (VAR) sv = fma_(w * w, atrous_var(p, iq), sv);
    }
  }
  float4 o = make_float4(sr / sw, sg / sw, sb / sw, VAR ? sv / (sw * sw) : 1.0f);
  if (VAR && p.var_dst) p.var_dst[ip] = o.w;
  if (p.remod) o = make_float4(fp0.x * o.x, fp0.y * o.y, fp0.z * o.z, 1.0f);
  p.dst[ip] = o;
}

// ---- temporal accumulation: the image-space stages; the G-buffer pass is k_temporal_gbuffer (fspt_kernels.hip) ----
// The blend pass (image space only): the history at M's sample position - four bilinear taps, each tested against this
// pixel's surface - blended with the accumulator.  One writer per pixel, vector stores, no atomics.
// MOM: the same taps, tests, weights and blend factor also carry the two luminance moments (l, l^2) of the
// DEMODULATED input, u = I.rgb / max(albedo, 1e-3) as atrous_load divides; the colour written is the same bit for bit.
// FAST: the same taps, tests and weights also carry a second colour history whose length is capped at
// fast_history - the colour's own recursion with that cap, never reading the long history: one more 16-byte load per
// accepted tap and one more 16-byte store.  Colour and moments written are the same bit for bit.
template <bool MOM, bool FAST>
__global__ __launch_bounds__(BLOCK_THREADS) void k_temporal_blend(const TemporalBP p) {
  const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int W = (int)p.W, H = (int)p.H;
  if (x >= W || y >= H) return;
  const size_t ip = (size_t)y * W + x;
  const float4 I = p.accum[ip];
  const float4 m = p.m[ip];
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
  float s1 = 0.0f, s2 = 0.0f;
  float fr = 0.0f, fg = 0.0f, fb = 0.0f, fn = 0.0f;
  // (a position further than a pixel outside the image has no tap inside it: refused before the float -> int conversion)
  if (p.has_hist && m.w != TM_KIND_NONE && m.x > -1.0f && m.y > -1.0f && m.x < (float)W && m.y < (float)H) {
    const float4 g1 = p.g[2 * ip + 1];
    const float flx = floor_(m.x), fly = floor_(m.y);
    const float ax = m.x - flx, ay = m.y - fly;
    const int x0 = (int)flx, y0 = (int)fly;
    const float ztol = p.depth_tol * m.z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = k & 1, j = k >> 1;
      const int xx = x0 + i, yy = y0 + j;
      const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
      if (xx < 0 || yy < 0 || xx >= W || yy >= H || !(w > 0.0f)) continue;
      const size_t iq = (size_t)yy * W + xx;
      const float4 q0 = p.g_prev[2 * iq], q1 = p.g_prev[2 * iq + 1];
      if (q1.w != g1.w) continue;
      if (g1.w != 0.0f) {
        if (!(abs_(q0.x - m.z) <= ztol)) continue;
        if (!(fma_(g1.z, q1.z, fma_(g1.y, q1.y, g1.x * q1.x)) >= p.normal_cos)) continue;
      }
      const float4 h = p.hist[iq];
      sr = fma_(w, h.x, sr); sg = fma_(w, h.y, sg); sb = fma_(w, h.z, sb); sn = fma_(w, h.w, sn);
      sw += w;
      if (MOM && p.has_mom) {
        const float2 hm = p.mom_hist[iq];
        s1 = fma_(w, hm.x, s1); s2 = fma_(w, hm.y, s2);
      }
      if (FAST && p.has_fast) {
        const float4 f = p.fast_hist[iq];
        fr = fma_(w, f.x, fr); fg = fma_(w, f.y, fg); fb = fma_(w, f.z, fb); fn = fma_(w, f.w, fn);
      }
    }
  }
  float4 o;
  float2 mo;
  if (MOM) {
    const float4 a0 = p.feat[2 * ip];
    const float l = luma(make_float4(I.x / max_(a0.x, 1e-3f), I.y / max_(a0.y, 1e-3f), I.z / max_(a0.z, 1e-3f), 1.0f));
    mo = make_float2(l, l * l);
  }
  if (sw > 0.0f) {
    const float Hr = sr / sw, Hg = sg / sw, Hb = sb / sw;
    const float N = min_(sn / sw, p.max_history);
    const float a = max_(p.n / (N + p.n), p.alpha);
    o = make_float4(Hr + (I.x - Hr) * a, Hg + (I.y - Hg) * a, Hb + (I.z - Hb) * a, min_(N + p.n, p.max_history));
    if (MOM && p.has_mom) {
      const float H1 = s1 / sw, H2 = s2 / sw;
      mo = make_float2(H1 + (mo.x - H1) * a, H2 + (mo.y - H2) * a);
    }
  } else {
    o = make_float4(I.x, I.y, I.z, min_(p.n, p.max_history));
  }
  p.out[ip] = o;
  if (MOM) p.mom_out[ip] = mo;
  if (FAST) {
    float4 f;
    if (sw > 0.0f && p.has_fast) {
      const float Hr = fr / sw, Hg = fg / sw, Hb = fb / sw;
      const float N = min_(fn / sw, p.fast_history);
      const float a = max_(p.n / (N + p.n), p.alpha);
      f = make_float4(Hr + (I.x - Hr) * a, Hg + (I.y - Hg) * a, Hb + (I.z - Hb) * a, min_(N + p.n, p.fast_history));
    } else {
      f = make_float4(I.x, I.y, I.z, min_(p.n, p.fast_history));
    }
    p.fast_out[ip] = f;
  }
}

// The history clamp: per channel the mean and spread of the fast history over the 5 x 5 window inside the
// image, the long history clamped into mean +- sigma_scale spread, in place (one reader and one writer per pixel; .w, the
// length, untouched).  Every pixel reads all 25 taps every frame, so the block stages its 20 x 20 footprint of the fast
// history in LDS once (6.4 KB; a tap outside the image is staged as zero and left out of the count) and sums the window
// directly from there, row-major, with one fma per tap and moment.  Vector stores, no atomics, no scratch.
constexpr int CLAMP_TILE = 16 + 2 * CLAMP_RADIUS;
__global__ __launch_bounds__(BLOCK_THREADS) void k_temporal_clamp(const ClampP p) {
  __shared__ float4 tile[CLAMP_TILE * CLAMP_TILE];
  const int W = (int)p.W, H = (int)p.H;
  const int bx = (int)(blockIdx.x * 16) - CLAMP_RADIUS, by = (int)(blockIdx.y * 16) - CLAMP_RADIUS;
  const int tid = (int)(threadIdx.y * 16 + threadIdx.x);
  for (int k = tid; k < CLAMP_TILE * CLAMP_TILE; k += 256) {
    const int xx = bx + k % CLAMP_TILE, yy = by + k / CLAMP_TILE;
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (xx >= 0 && yy >= 0 && xx < W && yy < H) f = p.fast[(size_t)yy * W + xx];
    tile[k] = f;
  }
  __syncthreads();
  const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
  if (x >= W || y >= H) return;
  const int x0 = x - CLAMP_RADIUS < 0 ? 0 : x - CLAMP_RADIUS, x1 = x + CLAMP_RADIUS >= W ? W - 1 : x + CLAMP_RADIUS;
  const int y0 = y - CLAMP_RADIUS < 0 ? 0 : y - CLAMP_RADIUS, y1 = y + CLAMP_RADIUS >= H ? H - 1 : y + CLAMP_RADIUS;
  const float cnt = (float)((x1 - x0 + 1) * (y1 - y0 + 1));
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, qr = 0.0f, qg = 0.0f, qb = 0.0f;
#pragma unroll
  for (int j = 0; j <= 2 * CLAMP_RADIUS; ++j) {
#pragma unroll
    for (int i = 0; i <= 2 * CLAMP_RADIUS; ++i) {
      const float4 f = tile[((int)threadIdx.y + j) * CLAMP_TILE + (int)threadIdx.x + i]; // (zero outside the image)
      sr += f.x; sg += f.y; sb += f.z;
      qr = fma_(f.x, f.x, qr); qg = fma_(f.y, f.y, qg); qb = fma_(f.z, f.z, qb);
    }
  }
  const float mr = sr / cnt, mg = sg / cnt, mb = sb / cnt;
  const float dr = sqrt_(max_(0.0f, qr / cnt - mr * mr)), dg = sqrt_(max_(0.0f, qg / cnt - mg * mg)), db = sqrt_(max_(0.0f, qb / cnt - mb * mb));
  const float s = p.sigma_scale;
  const float4 lo = make_float4(fma_(-s, dr, mr), fma_(-s, dg, mg), fma_(-s, db, mb), 0.0f);
  const float4 hi = make_float4(fma_(s, dr, mr), fma_(s, dg, mg), fma_(s, db, mb), 0.0f);
  const size_t ip = (size_t)y * W + x;
  const float4 h = p.hist[ip];
  const float4 o = make_float4(min_(max_(h.x, lo.x), hi.x), min_(max_(h.y, lo.y), hi.y), min_(max_(h.z, lo.z), hi.z), h.w);
  if (p.out) {
    p.out[ip] = o;
    if (p.lo) p.lo[ip] = lo;
    if (p.hi) p.hi[ip] = hi;
  } else {
    p.hist[ip] = o;
  }
}

// The variance of the luminance the guided filter is about to read: from the temporal moments where the
// history is at least SVGF_MIN_HISTORY effective frames long, else from the moments of the 7 x 7 neighbourhood weighted by
// k_atrous's own normal and depth weights at step 1 (centre weight 1).  Every tap is read through the caches: only pixels
// with a short history walk the window (a wave whose lanes all have a long one skips it), so a 22 x 22 LDS tile of moments
// and features - 19 KB a block, loaded by every block - would be paid where nothing reads it.
__global__ __launch_bounds__(BLOCK_THREADS) void k_svgf_variance(const SvgfVarP p) {
  const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)(blockIdx.y * blockDim.y + threadIdx.y);
  const int W = (int)p.W, H = (int)p.H;
  if (x >= W || y >= H) return;
  const size_t ip = (size_t)y * W + x;
  const float Fe = p.hist[ip].w / p.n;
  const float2 mp = p.mom[ip];
  float v;
  if (Fe >= SVGF_MIN_HISTORY) {
    v = max_(0.0f, mp.y - mp.x * mp.x) / Fe;
  } else {
    const float4 fp0 = p.feat[2 * ip], fp1 = p.feat[2 * ip + 1];
    const float lenp = sqrt_(fma_(fp1.z, fp1.z, fma_(fp1.y, fp1.y, fp1.x * fp1.x)));
    const bool hp = fp1.w != 0.0f;
    const float zden = p.sz * max_(fp0.w, 1e-3f);
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    for (int j = -SVGF_WINDOW; j <= SVGF_WINDOW; ++j) {
      const int yy = y + j;
      if (yy < 0 || yy >= H) continue;
      for (int i = -SVGF_WINDOW; i <= SVGF_WINDOW; ++i) {
        const int xx = x + i;
        if (xx < 0 || xx >= W) continue;
        const size_t iq = (size_t)yy * W + xx;
        float w = 1.0f;
        if (i != 0 || j != 0) {
          const float4 fq0 = p.feat[2 * iq], fq1 = p.feat[2 * iq + 1];
          if (p.sn != 0.0f) {
            const bool hq = fq1.w != 0.0f;
            if (hp || hq) {
              const float lenq = sqrt_(fma_(fq1.z, fq1.z, fma_(fq1.y, fq1.y, fq1.x * fq1.x)));
              if (hp != hq || lenp == 0.0f || lenq == 0.0f) w = 0.0f;
              else {
                const float c = min_(fma_(fp1.z, fq1.z, fma_(fp1.y, fq1.y, fp1.x * fq1.x)) / (lenp * lenq), 1.0f);
                w *= c > 0.0f ? exp2f(p.sn * log2f(c)) : 0.0f;
              }
            }
          }
          const float dz = abs_(fp0.w - fq0.w);
          if (p.sz != INFINITY && dz != 0.0f) w *= exp2f(-(dz / zden) * 1.44269504f);
        }
        const float2 mq = p.mom[iq];
        s1 = fma_(w, mq.x, s1); s2 = fma_(w, mq.y, s2);
        sw += w;
      }
    }
    const float S1 = s1 / sw, S2 = s2 / sw;
    v = max_(0.0f, S2 - S1 * S1) / max_(Fe, 1.0f);
  }
  p.var[ip] = v;
}

// ---- launchers.  The two grids of the image passes: blocks of BLOCK_THREADS over n elements, 16 x 16-pixel blocks over p.W x p.H ----
static uint32_t blocks_for(uint32_t n) { return (n + BLOCK_THREADS - 1) / BLOCK_THREADS; }
template <class K, class P> static hipError_t launch_pixels(K kernel, const P &p, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3((p.W + 15) / 16, (p.H + 15) / 16), dim3(16, 16), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_draw(const float4 *acc, uint32_t W, uint32_t H, float exposure, float saturation, int denoise, float max_sigma,
                       float scale, uint32_t *out, const ExposureState *state, const BloomDraw *bloom, hipStream_t stream) {
  const dim3 grid(blocks_for(W * H)), block(BLOCK_THREADS);
  if (bloom && state) hipLaunchKernelGGL(k_draw_bloom<true>, grid, block, 0, stream, acc, W, H, exposure, saturation, denoise, max_sigma, scale, out, state, *bloom);
  else if (bloom) hipLaunchKernelGGL(k_draw_bloom<false>, grid, block, 0, stream, acc, W, H, exposure, saturation, denoise, max_sigma, scale, out, state, *bloom);
  else if (state) hipLaunchKernelGGL(k_draw_auto, grid, block, 0, stream, acc, W, H, exposure, saturation, denoise, max_sigma, scale, out, state);
  else hipLaunchKernelGGL(k_draw, grid, block, 0, stream, acc, W, H, exposure, saturation, denoise, max_sigma, scale, out);
  return hipGetLastError();
}

// ---- bloom ----
int g_bloom_form = BLOOM_FORM;                    // the shipped form, or fspt_bloom_set_form's
uint32_t g_bloom_tail_texels = BLOOM_TAIL_TEXELS; // ... fspt_bloom_set_tail_texels'

BloomPlan bloom_plan(uint32_t vw, uint32_t vh, uint32_t levels, int form, uint32_t tail_texels) {
  BloomPlan q{};
  q.w[0] = vw; q.h[0] = vh;
  uint32_t n = 0;
  size_t off = 0;
  while (n < levels && n < BLOOM_MAX_LEVELS && (q.w[n] < q.h[n] ? q.w[n] : q.h[n]) > 1u) {
    q.w[n + 1] = (q.w[n] + 1u) >> 1; q.h[n + 1] = (q.h[n] + 1u) >> 1;
    q.off[n + 1] = off;
    off += (size_t)q.w[n + 1] * q.h[n + 1];
    ++n;
  }
  q.n = n; q.texels = off;
  // the tail: from the first level whose texels are few enough AND whose levels, three floats a texel, fit the LDS
  if (form == 1)
    for (uint32_t k = 1; k < n; ++k) {
      const size_t bytes = (off - q.off[k]) * 12;
      if ((size_t)q.w[k] * q.h[k] <= tail_texels && bytes <= BLOOM_TAIL_LDS_MAX) { q.tail = k; q.tail_lds = bytes; break; }
    }
  return q;
}

static hipError_t launch_bloom_down(const float4 *src, uint32_t pitch, uint32_t ws, uint32_t hs, float4 *dst, uint32_t wd, uint32_t hd,
                                    bool first, hipStream_t stream) {
  const dim3 grid((wd + BLOOM_TX - 1) / BLOOM_TX, (hd + BLOOM_TY - 1) / BLOOM_TY), block(BLOCK_THREADS);
  if (first) hipLaunchKernelGGL(k_bloom_down<true>, grid, block, 0, stream, src, pitch, ws, hs, dst, wd, hd);
  else hipLaunchKernelGGL(k_bloom_down<false>, grid, block, 0, stream, src, pitch, ws, hs, dst, wd, hd);
  return hipGetLastError();
}

static hipError_t launch_bloom_up(float4 *dk, uint32_t w, uint32_t h, const float4 *up, uint32_t wu, uint32_t hu, float scatter, hipStream_t stream) {
  hipLaunchKernelGGL(k_bloom_up, dim3(blocks_for(w * h)), dim3(BLOCK_THREADS), 0, stream, dk, w, h, up, wu, hu, scatter);
  return hipGetLastError();
}

static hipError_t launch_bloom_tail(const BloomTailP &p, size_t lds_bytes, hipStream_t stream) {
  if (lds_bytes > BLOOM_TAIL_LDS_MAX) return hipErrorInvalidValue;
  if (lds_bytes > 65536) { // (above the 64 KiB every kernel may have the limit is raised per function)
    hipError_t e = hipFuncSetAttribute((const void *)k_bloom_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BLOOM_TAIL_LDS_MAX);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_bloom_tail, dim3(1), dim3(BLOOM_TAIL_THREADS), lds_bytes, stream, p);
  return hipGetLastError();
}

// the whole chain in front of a draw: D_1 .. D_n into `pyr` (the levels one behind the other, q.off), combined in place to U_1 .. ;
// ev (NULL or 4 events): before the down chain, behind it, behind the tail, behind the up chain.  dbg_*: see k_bloom_tail;
// down_snapshot (NULL in a draw): the D levels as the down chain left them are copied there before anything is combined.
hipError_t launch_bloom_chain(const float4 *src, uint32_t pitch, const BloomPlan &q, float scatter, float4 *pyr, hipEvent_t *ev,
                              float4 *down_snapshot, float4 *dbg_up, hipStream_t stream) {
  hipError_t e = ev ? hipEventRecord(ev[0], stream) : hipSuccess;
  const uint32_t last = q.tail ? q.tail : q.n; // the last level the down chain makes
  for (uint32_t k = 0; k < last && e == hipSuccess; ++k)
    e = launch_bloom_down(k ? pyr + q.off[k] : src, k ? q.w[k] : pitch, q.w[k], q.h[k], pyr + q.off[k + 1], q.w[k + 1], q.h[k + 1], k == 0, stream);
  if (e == hipSuccess && down_snapshot) e = hipMemcpyAsync(down_snapshot, pyr, q.texels * sizeof(float4), hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess && ev) e = hipEventRecord(ev[1], stream);
  if (e == hipSuccess && q.tail) {
    const BloomTailP p{pyr + q.off[q.tail], q.w[q.tail], q.h[q.tail], q.n - q.tail, scatter,
                       down_snapshot ? down_snapshot + q.off[q.tail + 1] : nullptr, dbg_up ? dbg_up + q.off[q.tail + 1] : nullptr};
    e = launch_bloom_tail(p, q.tail_lds, stream);
  }
  if (e == hipSuccess && ev) e = hipEventRecord(ev[2], stream);
  for (uint32_t k = last; k-- > 1 && e == hipSuccess;)
    e = launch_bloom_up(pyr + q.off[k], q.w[k], q.h[k], pyr + q.off[k + 1], q.w[k + 1], q.h[k + 1], scatter, stream);
  if (e == hipSuccess && ev) e = hipEventRecord(ev[3], stream);
  return e;
}

hipError_t launch_bloom_mix(const float4 *src, uint32_t W, uint32_t H, const BloomDraw &bl, float4 *bloom_out, float4 *mix_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_bloom_mix, dim3(blocks_for(W * H)), dim3(BLOCK_THREADS), 0, stream, src, W, H, bl, bloom_out, mix_out);
  return hipGetLastError();
}

// ---- auto-exposure ----
int g_exposure_form = 0; // (the two forms measure the same at 1920 x 1080; the plain one ships)

hipError_t launch_exposure_histogram(const float4 *src, uint32_t W, uint32_t vw, uint32_t vh, uint32_t *hist, int form, hipStream_t stream) {
  const uint32_t n = vw * vh;
  if (n == 0) return hipSuccess;
  const uint32_t blocks = blocks_for(n);
  const dim3 grid(blocks < EXPOSURE_GRID ? blocks : EXPOSURE_GRID), block(BLOCK_THREADS);
  if (form) hipLaunchKernelGGL(k_exposure_histogram<true>, grid, block, 0, stream, src, W, vw, vh, hist);
  else hipLaunchKernelGGL(k_exposure_histogram<false>, grid, block, 0, stream, src, W, vw, vh, hist);
  return hipGetLastError();
}

hipError_t launch_exposure_resolve(uint32_t *hist, ExposureState *state, const ExposureP &p, hipStream_t stream) {
  hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(EXPOSURE_BINS), 0, stream, hist, state, p);
  return hipGetLastError();
}

// ---- denoiser and temporal stages ----
hipError_t launch_atrous(const AtrousP &p, bool var, hipStream_t stream) {
  return var ? launch_pixels(k_atrous<true>, p, stream) : launch_pixels(k_atrous<false>, p, stream);
}
hipError_t launch_temporal_blend(const TemporalBP &p, hipStream_t stream) {
  if (p.fast_out) return p.mom_out ? launch_pixels(k_temporal_blend<true, true>, p, stream) : launch_pixels(k_temporal_blend<false, true>, p, stream);
  return p.mom_out ? launch_pixels(k_temporal_blend<true, false>, p, stream) : launch_pixels(k_temporal_blend<false, false>, p, stream);
}
hipError_t launch_temporal_clamp(const ClampP &p, hipStream_t stream) { return launch_pixels(k_temporal_clamp, p, stream); }
hipError_t launch_svgf_variance(const SvgfVarP &p, hipStream_t stream) { return launch_pixels(k_svgf_variance, p, stream); }

} // namespace fspt
