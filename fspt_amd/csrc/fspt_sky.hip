// fspt_sky.hip - the light side of a live scene, made on the GPU:
//   k_sky_generate   one thread per texel of a w x h equirect map: single-scattering Rayleigh + Mie (the model: fspt_tuning.h;
//                    tests/sky_ref.py restates it), the linear radiance and / or its RGBE bytes
//   k_env_radiance   per texel env_sampler.js's getRadiance in float64, into a (w + 1) x (h + 1) table with a zero border,
//                    and the brightest texel (an integer max of the bit patterns: exact, no order)
//   k_sat_rows       the table's rows summed left to right: one wave per row, a wave64 scan per 64 texels and a carry
//   k_sat_cols       its columns summed top to bottom: one thread per column
//   k_bins_root, k_bins_split   env_sampler.js's bisplit (scene_build.cpp fspt_env_bins states it) level by level: one
//                    thread per box of the frontier, its first half's sum from four table reads
//   k_bins_count, k_bins_emit   leaves per subtree bottom-up, offsets top-down: the bins in the recursion's depth-first order
// Every float64 sum has a fixed order (the scans' shape, then ((S11 - S01) - S10) + S00), so two runs give the same bytes.
// A box whose first corner is not a pair of integers is summed as the reference sums it - texel by texel through
// getRadiance's byte index, which for such coordinates is mostly no integer (NaN) and now and then a misaligned read -
// by its one thread: the rare path (odd sizes, below the first halving).
#include "fspt_internal.hpp"

namespace fspt {
namespace {

const uint32_t SKY_BS = 256;
const uint32_t BINS_LEVELS = 66; // depths 0 .. 65: a box of depth 65 is a leaf (depth > 64)

// ---------------------------------------------------------------------------
// the sky
// ---------------------------------------------------------------------------
struct SkyArgs {
  float sx, sy, sz;        // the unit sun direction
  float bR[3], bM, bMe;    // scattering coefficients; Mie extinction
  float I, gain, alb_pi[3];
  float cos_r, disc;       // cos(sun_radius), I / (pi sun_radius^2)
  uint32_t N, M;
};

#define SKY_RE 6360000.0f
#define SKY_RA 6420000.0f
#define SKY_HR 7994.0f
#define SKY_HM 1200.0f
#define SKY_OY 6360001.0f              // the observer's height above the centre
#define SKY_CE 12720001.0f             // |o|^2 - Re^2 = (oy - Re)(oy + Re), exact
#define SKY_CA (-59999.0f * 12780001.0f) // |o|^2 - Ra^2 = (oy - Ra)(oy + Ra)
#define SKY_K (60000.0f * 12780000.0f) // Ra^2 - Re^2
#define SKY_RE2 (SKY_RE * SKY_RE)
#define SKY_PI 3.14159274101257324f

// height above the ground of a point with |p|^2 - Re^2 = a: (|p| - Re)(|p| + Re) = a, without the cancellation of |p| - Re
__device__ inline float sky_height(float a) { return a / (sqrtf(SKY_RE2 + a) + SKY_RE); }

// The light ray from a point with |p|^2 - Re^2 = a and p . s = ps to the top of the atmosphere: the two optical depths in M
// midpoint samples; false when a midpoint lies below the ground.
__device__ inline bool sky_light_ray(float a, float ps, uint32_t M, float &lR, float &lM) {
  const float tl = -ps + sqrtf(ps * ps - (a - SKY_K));
  const float dl = tl / (float)M;
  bool lit = true;
  lR = 0.0f; lM = 0.0f;
  for (uint32_t j = 0; j < M; ++j) {
    const float l = ((float)j + 0.5f) * dl;
    const float hl = sky_height(a + l * (2.0f * ps + l));
    if (hl < 0.0f) lit = false;
    lR += expf(-hl / SKY_HR) * dl;
    lM += expf(-hl / SKY_HM) * dl;
  }
  return lit;
}

// e = the smallest integer with 2^e >= m (m >= 1e-6: a normal float), from the float's own fields
__device__ inline int sky_ceil_log2(float m) {
  const uint32_t b = __float_as_uint(m);
  return (int)((b >> 23) & 255u) - 127 + ((b & 0x7FFFFFu) ? 1 : 0);
}

__device__ inline uint32_t sky_encode(float r, float g, float b) {
  r = (isfinite(r) && r > 0.0f) ? r : 0.0f;
  g = (isfinite(g) && g > 0.0f) ? g : 0.0f;
  b = (isfinite(b) && b > 0.0f) ? b : 0.0f;
  const float m = fmaxf(fmaxf(r, g), fmaxf(b, 1e-6f));
  int e = sky_ceil_log2(m);
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  const float c[3] = {r, g, b};
  uint32_t out = (uint32_t)(e + 128) << 24;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float q = floorf(ldexpf(c[k], -e) * 255.0f + 0.5f);
    q = q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q);
    out |= (uint32_t)q << (8 * k);
  }
  return out;
}

// lin: w * h * 3 floats or NULL; rgbe: w * h words or NULL.  blockIdx.y = the row, so that a wave is 64 texels of one row.
__global__ void k_sky_generate(SkyArgs P, uint32_t w, uint32_t h, uint32_t y0, float *__restrict__ lin, uint32_t *__restrict__ rgbe) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = y0 + blockIdx.y;
  if (x >= w || y >= h) return;
  const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
  const float theta = 2.0f * SKY_PI * u, phi = SKY_PI * v;
  const float sp = sinf(phi), cp = cosf(phi);
  const float dx = cosf(theta) * sp, dy = cp, dz = sinf(theta) * sp;
  const float mu = (dx * P.sx + dy * P.sy) + dz * P.sz;
  const float b = SKY_OY * dy; // o . d
  const float t_atm = -b + sqrtf(b * b - SKY_CA);
  const float disc_e = b * b - SKY_CE;
  float t_gnd = -1.0f;
  if (disc_e >= 0.0f) t_gnd = -b - sqrtf(disc_e);
  const bool ground = t_gnd > 0.0f;
  const float t_max = ground ? t_gnd : t_atm;
  const float ds = t_max / (float)P.N;
  const float os = SKY_OY * P.sy; // o . s
  float tR = 0.0f, tM = 0.0f;
  float sumR[3] = {0.0f, 0.0f, 0.0f}, sumM[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t i = 0; i < P.N; ++i) {
    const float t = ((float)i + 0.5f) * ds;
    const float a = SKY_CE + t * (2.0f * b + t); // |p|^2 - Re^2
    const float hv = sky_height(a);
    const float rR = expf(-hv / SKY_HR) * ds, rM = expf(-hv / SKY_HM) * ds;
    tR += rR; tM += rM;
    float lR, lM;
    const bool lit = sky_light_ray(a, os + t * mu, P.M, lR, lM);
    if (lit) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float T = expf(-(P.bR[c] * (tR + lR) + P.bMe * (tM + lM)));
        sumR[c] += T * rR;
        sumM[c] += T * rM;
      }
    }
  }
  const float g = 0.76f, m2 = 1.0f + mu * mu;
  const float pR = 3.0f / (16.0f * SKY_PI) * m2;
  const float den = 1.0f + g * g - 2.0f * g * mu;
  const float pM = 3.0f / (8.0f * SKY_PI) * ((1.0f - g * g) * m2) / ((2.0f + g * g) * (den * sqrtf(den)));
  float L[3], Tv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    L[c] = P.I * (sumR[c] * P.bR[c] * pR + sumM[c] * P.bM * pM);
    Tv[c] = expf(-(P.bR[c] * tR + P.bMe * tM));
  }
  if (ground) {
    const float ag = SKY_CE + t_gnd * (2.0f * b + t_gnd), psg = os + t_gnd * mu;
    const float ns = psg / sqrtf(SKY_RE2 + ag);
    float lR, lM;
    const bool lit = sky_light_ray(ag, psg, P.M, lR, lM);
    if (lit && ns > 0.0f) {
#pragma unroll
      for (int c = 0; c < 3; ++c) L[c] += Tv[c] * P.alb_pi[c] * (P.I * expf(-(P.bR[c] * lR + P.bMe * lM)) * ns);
    }
  } else if (mu >= P.cos_r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] += P.disc * Tv[c];
  }
  const size_t at = (size_t)y * w + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) L[c] *= P.gain;
  if (lin) { lin[at * 3] = L[0]; lin[at * 3 + 1] = L[1]; lin[at * 3 + 2] = L[2]; }
  if (rgbe) rgbe[at] = sky_encode(L[0], L[1], L[2]);
}

SkyArgs sky_args(const fspt_sky_params *p) {
  SkyArgs A;
  A.sx = p->sun_dir[0]; A.sy = p->sun_dir[1]; A.sz = p->sun_dir[2];
  A.bR[0] = 5.8e-6f; A.bR[1] = 13.5e-6f; A.bR[2] = 33.1e-6f;
  A.bM = (float)((double)p->turbidity * 21e-6);
  A.bMe = (float)(1.1 * (double)p->turbidity * 21e-6);
  A.I = p->sun_intensity; A.gain = p->gain;
  for (int c = 0; c < 3; ++c) A.alb_pi[c] = (float)((double)p->ground_albedo[c] / M_PI);
  A.cos_r = (float)std::cos((double)p->sun_radius);
  A.disc = (float)((double)p->sun_intensity / (M_PI * (double)p->sun_radius * (double)p->sun_radius));
  A.N = p->view_samples; A.M = p->light_samples;
  return A;
}

hipError_t sky_launch(const fspt_sky_params *p, uint32_t w, uint32_t h, float *lin, uint32_t *rgbe, hipStream_t st, uint32_t *launches) {
  const SkyArgs A = sky_args(p);
  for (uint32_t y0 = 0; y0 < h; y0 += 65535u) { // (grid.y <= 65535: one launch)
    const uint32_t rows = std::min<uint32_t>(h - y0, 65535u);
    hipLaunchKernelGGL(k_sky_generate, dim3((w + SKY_BS - 1) / SKY_BS, rows), dim3(SKY_BS), 0, st, A, w, h, y0, lin, rgbe);
    ++*launches;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// the bins
// ---------------------------------------------------------------------------
struct BinNode { double rad, x0, y0, x1, y1; uint32_t child /* first of two; 0 = a leaf */, count, off, pad; };
struct BinsCtl { unsigned long long bright; uint32_t start[BINS_LEVELS + 2], cnt[BINS_LEVELS + 2], n_bins, overflow; };

// getRadiance + pixelAt (env_sampler.js:6-21) of the four bytes at `at`, in scene_build.cpp radiance_at's order
__device__ inline double env_radiance_bytes(const uint8_t *__restrict__ d, size_t at) {
  const double c0 = (double)d[at], c1 = (double)d[at + 1], c2 = (double)d[at + 2];
  const double power = __longlong_as_double((long long)(1023 + (int)d[at + 3] - 128) << 52); // 2^(E - 128), exact
  const double n0 = power * c0 / 255.0, n1 = power * c1 / 255.0, n2 = power * c2 / 255.0;
  return 0.2126 * n0 + 0.7152 * n1 + 0.0722 * n2;
}

// ... at any coordinates: a byte index that is no integer, or runs out of the map, reads `undefined` -> NaN
__device__ inline double env_radiance_at(const uint8_t *__restrict__ d, double w4, double lim, double x, double y) {
  const double base = (y * w4) + (x * 4.0);
  if (base != floor(base) || !(base >= 0.0 && base + 3.0 < lim)) return __longlong_as_double(0x7FF8000000000000ll);
  return env_radiance_bytes(d, (size_t)base);
}

__device__ inline double sat_box(const double *__restrict__ S, size_t pitch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
  return ((S[(size_t)y1 * pitch + x1] - S[(size_t)y0 * pitch + x1]) - S[(size_t)y1 * pitch + x0]) + S[(size_t)y0 * pitch + x0];
}

// one thread per table entry: row 0 and column 0 are zero, entry (y + 1, x + 1) = texel (x, y)'s radiance
__global__ void k_env_radiance(const uint8_t *__restrict__ rgbe, uint32_t w, uint32_t h, double *__restrict__ S, BinsCtl *__restrict__ ctl) {
  const size_t pitch = (size_t)w + 1, n = pitch * ((size_t)h + 1);
  unsigned long long top = 0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t yy = i / pitch, xx = i - yy * pitch;
    double r = 0.0;
    if (xx && yy) {
      r = env_radiance_bytes(rgbe, ((yy - 1) * w + (xx - 1)) * 4);
      const unsigned long long bits = (unsigned long long)__double_as_longlong(r); // r >= 0: the bits order as the values
      top = bits > top ? bits : top;
    }
    S[i] = r;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(top, d);
    top = o > top ? o : top;
  }
  if ((threadIdx.x & 63u) == 0 && top) atomicMax(&ctl->bright, top);
}

__global__ void k_sat_rows(double *__restrict__ S, uint32_t w, uint32_t h) {
  const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= h) return; // (a whole wave)
  double *r = S + ((size_t)row + 1) * ((size_t)w + 1) + 1;
  double carry = 0.0;
  for (uint32_t xb = 0; xb < w; xb += 64u) {
    const uint32_t x = xb + lane;
    double v = x < w ? r[x] : 0.0;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const double o = __shfl_up(v, d);
      if (lane >= d) v = o + v;
    }
    v = carry + v;
    if (x < w) r[x] = v;
    carry = __shfl(v, 63);
  }
}

__global__ void k_sat_cols(double *__restrict__ S, uint32_t w, uint32_t h) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w) return;
  const size_t pitch = (size_t)w + 1;
  double *c = S + pitch + 1 + x;
  double acc = 0.0;
#pragma unroll 8
  for (uint32_t y = 0; y < h; ++y) {
    acc = acc + c[(size_t)y * pitch];
    c[(size_t)y * pitch] = acc;
  }
}

__global__ void k_bins_root(BinNode *__restrict__ pool, BinsCtl *__restrict__ ctl, const double *__restrict__ S, uint32_t w, uint32_t h) {
  BinNode n;
  n.rad = S[(size_t)h * ((size_t)w + 1) + w];
  n.x0 = 0.0; n.y0 = 0.0; n.x1 = (double)w; n.y1 = (double)h;
  n.child = 0u; n.count = 0u; n.off = 0u; n.pad = 0u;
  pool[0] = n;
  ctl->start[0] = 0u; ctl->cnt[0] = 1u;
}

// the sum bisplit takes over its first half: `for (x = x0; x < xs; x++) for (y = y0; y < ys; y++) sub += getRadiance(x, y)`
__device__ double bins_first_half(const uint8_t *__restrict__ rgbe, const double *__restrict__ S, uint32_t w, uint32_t h,
                                  double x0, double y0, double xs, double ys) {
  if (!(x0 < xs) || !(y0 < ys)) return 0.0; // (an empty loop; NaN never gets here: the coordinates are finite)
  if (x0 == floor(x0) && y0 == floor(y0)) { // integer x and y all the way: the texels [x0, ceil xs) x [y0, ceil ys)
    return sat_box(S, (size_t)w + 1, (uint32_t)x0, (uint32_t)y0, min((uint32_t)ceil(xs), w), min((uint32_t)ceil(ys), h)); // (boxes lie inside the map: the min never bites)
  }
  const double w4 = (double)w * 4.0, lim = (double)w * (double)h * 4.0;
  double sub = 0.0;
  for (double x = x0; x < xs; x++)
    for (double y = y0; y < ys; y++) {
      sub += env_radiance_at(rgbe, w4, lim, x, y);
      if (sub != sub) return sub; // (NaN stays NaN)
    }
  return sub;
}

// level k of the recursion: every box of depth k stops or is cut; its two children join level k + 1
__global__ void k_bins_split(BinNode *__restrict__ pool, uint32_t pool_cap, BinsCtl *__restrict__ ctl, uint32_t k, const uint8_t *__restrict__ rgbe,
                             const double *__restrict__ S, uint32_t w, uint32_t h) {
  const uint32_t start = ctl->start[k], n = min(ctl->cnt[k], pool_cap - min(ctl->start[k], pool_cap)); // (never past the pool)
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->start[k + 1] = start + n;
  if (n == 0u) return;
  const double total = S[(size_t)h * ((size_t)w + 1) + w], brightest = __longlong_as_double((long long)ctl->bright);
  const double a = total / 64, b = brightest / 2;
  const double min_rad = a > b ? a : b;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const BinNode nd = pool[start + i];
    const double x0 = nd.x0, y0 = nd.y0, x1 = nd.x1, y1 = nd.y1;
    if (nd.rad <= min_rad || (y1 - y0) * (x1 - x0) < 2 || k > 64u) continue; // a leaf: child stays 0
    const bool vert = (x1 - x0) > (y1 - y0);
    double xs = x1, ys = (y1 - y0) / 2 + y0;
    if (vert) { xs = (x1 - x0) / 2 + x0; ys = y1; }
    const double sub = bins_first_half(rgbe, S, w, h, x0, y0, xs, ys);
    const uint32_t c = start + n + atomicAdd(&ctl->cnt[k + 1], 2u);
    if (c + 1u >= pool_cap || c < start) { ctl->overflow = 1u; continue; } // (cannot happen: leaves are disjoint, of area >= 1)
    BinNode l, r;
    l.rad = sub; l.x0 = x0; l.y0 = y0; l.x1 = xs; l.y1 = ys;
    r.rad = nd.rad - sub; r.x1 = x1; r.y1 = y1;
    if (vert) { r.x0 = xs; r.y0 = y0; } else { r.x0 = x0; r.y0 = ys; }
    l.child = r.child = 0u; l.count = r.count = 0u; l.off = r.off = 0u; l.pad = r.pad = 0u;
    pool[c] = l; pool[c + 1u] = r;
    pool[start + i].child = c;
  }
}

// one block: leaves below every box, deepest level first
__global__ void k_bins_count(BinNode *__restrict__ pool, uint32_t pool_cap, BinsCtl *__restrict__ ctl) {
  for (int k = (int)BINS_LEVELS - 1; k >= 0; --k) {
    const uint32_t start = ctl->start[k];
    const uint32_t n = min(ctl->cnt[k], pool_cap - min(start, pool_cap));
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      BinNode *nd = pool + start + i;
      const uint32_t c = nd->child;
      nd->count = (c && c + 1u < pool_cap) ? pool[c].count + pool[c + 1u].count : 1u;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ctl->n_bins = pool[0].count;
}

// one block: a box's bins start at `off`; its first child's come first.  ToUint16 of the coordinates (new Uint16Array(boxes)).
__global__ void k_bins_emit(BinNode *__restrict__ pool, uint32_t pool_cap, const BinsCtl *__restrict__ ctl, uint4 *__restrict__ bins, uint32_t cap) {
  for (uint32_t k = 0; k < BINS_LEVELS; ++k) {
    const uint32_t start = ctl->start[k];
    const uint32_t n = min(ctl->cnt[k], pool_cap - min(start, pool_cap));
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const BinNode nd = pool[start + i];
      const uint32_t c = nd.child;
      if (c && c + 1u < pool_cap) {
        pool[c].off = nd.off;
        pool[c + 1u].off = nd.off + pool[c].count;
      } else if (nd.off < cap) {
        bins[nd.off] = make_uint4((uint32_t)nd.x0 & 0xFFFFu, (uint32_t)nd.y0 & 0xFFFFu, (uint32_t)nd.x1 & 0xFFFFu, (uint32_t)nd.y1 & 0xFFFFu);
      }
    }
    __syncthreads();
  }
}

struct BinsWork { double *sat = nullptr; BinNode *pool = nullptr; BinsCtl *ctl = nullptr; uint32_t pool_cap = 0; };

#define SKY_E(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// the table of a raw map (device memory, 4-byte aligned): radiance, rows, columns
hipError_t table_build(const uint8_t *rgbe, uint32_t w, uint32_t h, Hold &hold, BinsWork &W, hipStream_t st, uint32_t *launches) {
  const size_t n = ((size_t)w + 1) * ((size_t)h + 1);
  SKY_E(hold.make((void **)&W.sat, n * 8));
  SKY_E(hold.make((void **)&W.ctl, sizeof(BinsCtl)));
  SKY_E(hipMemsetAsync(W.ctl, 0, sizeof(BinsCtl), st));
  const uint32_t blocks = (uint32_t)std::min<size_t>((n + SKY_BS - 1) / SKY_BS, 1u << 16);
  hipLaunchKernelGGL(k_env_radiance, dim3(blocks), dim3(SKY_BS), 0, st, rgbe, w, h, W.sat, W.ctl);
  hipLaunchKernelGGL(k_sat_rows, dim3((h + 3u) / 4u), dim3(256), 0, st, W.sat, w, h);
  hipLaunchKernelGGL(k_sat_cols, dim3((w + 63u) / 64u), dim3(64), 0, st, W.sat, w, h);
  *launches += 3;
  return hipGetLastError();
}

// ... and the tree over it, counted: *n_bins is read back (the one read-back; it waits for the stream)
hipError_t bins_build(const uint8_t *rgbe, uint32_t w, uint32_t h, Hold &hold, BinsWork &W, hipStream_t st, uint32_t *launches, uint32_t *n_bins) {
  SKY_E(table_build(rgbe, w, h, hold, W, st, launches));
  // 2 w h - 1 boxes at most: leaves are disjoint, of area >= 1.  An odd capacity: the root, then whole pairs.
  W.pool_cap = (uint32_t)std::min<uint64_t>(2ull * w * h + 1ull, 0xFFFFFFFDull);
  SKY_E(hold.make((void **)&W.pool, (size_t)W.pool_cap * sizeof(BinNode)));
  hipLaunchKernelGGL(k_bins_root, dim3(1), dim3(1), 0, st, W.pool, W.ctl, W.sat, w, h);
  for (uint32_t k = 0; k < BINS_LEVELS; ++k) { // a fixed number of launches: an empty level returns at once
    const uint64_t most = std::min<uint64_t>(k < 32u ? 1ull << k : ~0ull, W.pool_cap); // boxes a level can hold
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((most + SKY_BS - 1) / SKY_BS, 1024u);
    hipLaunchKernelGGL(k_bins_split, dim3(blocks), dim3(SKY_BS), 0, st, W.pool, W.pool_cap, W.ctl, k, rgbe, W.sat, w, h);
  }
  hipLaunchKernelGGL(k_bins_count, dim3(1), dim3(1024), 0, st, W.pool, W.pool_cap, W.ctl);
  *launches += BINS_LEVELS + 2;
  SKY_E(hipGetLastError());
  uint32_t back[2] = {0u, 0u}; // n_bins, overflow
  SKY_E(hipMemcpyAsync(back, &W.ctl->n_bins, 8, hipMemcpyDeviceToHost, st));
  SKY_E(hipStreamSynchronize(st));
  if (back[1]) return hipErrorOutOfMemory; // the tree outgrew a pool of 2^32 boxes
  *n_bins = back[0];
  return hipSuccess;
}

hipError_t bins_emit(BinsWork &W, uint4 *bins, uint32_t cap, hipStream_t st, uint32_t *launches) {
  hipLaunchKernelGGL(k_bins_emit, dim3(1), dim3(1024), 0, st, W.pool, W.pool_cap, W.ctl, bins, cap);
  ++*launches;
  return hipGetLastError();
}

__global__ void k_box_sums(const double *__restrict__ S, uint32_t w, const uint4 *__restrict__ boxes, uint32_t n, double *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 b = boxes[i];
  out[i] = sat_box(S, (size_t)w + 1, b.x, b.y, b.z, b.w);
}

int run_fail(const char *fn, hipError_t e) {
  (void)hipGetLastError();
  fspt_set_error("%s: %s", fn, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
}

} // namespace

int sky_generate_run(const fspt_sky_params *p, uint32_t w, uint32_t h, uint8_t *rgbe_out, float *linear_out) {
  const char *fn = "fspt_sky_generate";
  Hold hold;
  const size_t n = (size_t)w * h;
  float *lin = nullptr;
  uint32_t *rgbe = nullptr;
  uint32_t launches = 0;
  hipError_t e = hipSuccess;
  if (linear_out) e = hold.make((void **)&lin, n * 12);
  if (e == hipSuccess && rgbe_out) e = hold.make((void **)&rgbe, n * 4);
  if (e == hipSuccess) e = sky_launch(p, w, h, lin, rgbe, nullptr, &launches);
  if (e == hipSuccess && linear_out) e = hipMemcpy(linear_out, lin, n * 12, hipMemcpyDeviceToHost);
  if (e == hipSuccess && rgbe_out) e = hipMemcpy(rgbe_out, rgbe, n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e == hipSuccess ? FSPT_OK : run_fail(fn, e);
}

int env_bins_run(const uint8_t *rgbe, uint32_t w, uint32_t h, uint32_t *bins, uint32_t cap, uint32_t *n_bins) {
  const char *fn = "fspt_env_bins_gpu";
  Hold hold;
  BinsWork W;
  void *raw = nullptr, *out = nullptr;
  uint32_t launches = 0, nb = 0;
  const size_t bytes = (size_t)w * h * 4;
  hipError_t e = hold.make(&raw, bytes);
  if (e == hipSuccess) e = hipMemcpy(raw, rgbe, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = bins_build((const uint8_t *)raw, w, h, hold, W, nullptr, &launches, &nb);
  const uint32_t m = nb < cap ? nb : cap;
  if (e == hipSuccess && bins && m) {
    e = hold.make(&out, (size_t)m * 16);
    if (e == hipSuccess) e = bins_emit(W, (uint4 *)out, m, nullptr, &launches);
    if (e == hipSuccess) e = hipMemcpy(bins, out, (size_t)m * 16, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return run_fail(fn, e);
  *n_bins = nb;
  return FSPT_OK;
}

int env_box_sums_run(const uint8_t *rgbe, uint32_t w, uint32_t h, const uint32_t *boxes, uint32_t n, double *out) {
  const char *fn = "fspt_env_box_sums_eval";
  Hold hold;
  BinsWork W;
  void *raw = nullptr, *d_box = nullptr, *d_out = nullptr;
  uint32_t launches = 0;
  const size_t bytes = (size_t)w * h * 4;
  hipError_t e = hold.make(&raw, bytes);
  if (e == hipSuccess) e = hold.make(&d_box, (size_t)n * 16);
  if (e == hipSuccess) e = hold.make(&d_out, (size_t)n * 8);
  if (e == hipSuccess) e = hipMemcpy(raw, rgbe, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_box, boxes, (size_t)n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = table_build((const uint8_t *)raw, w, h, hold, W, nullptr, &launches);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_box_sums, dim3((n + SKY_BS - 1) / SKY_BS), dim3(SKY_BS), 0, nullptr, W.sat, w, (const uint4 *)d_box, n, (double *)d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost);
  return e == hipSuccess ? FSPT_OK : run_fail(fn, e);
}

int environment_gpu(fspt_scene *s, const char *fn, const uint8_t *env, bool env_on_device, const fspt_sky_params *sky, uint32_t w, uint32_t h) {
  fspt_scene::Sky &K = s->sky;
  for (hipEvent_t &ev : K.ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  hipStream_t st = nullptr;
  Hold hold;
  BinsWork W;
  void *raw = env_on_device ? (void *)env : nullptr, *n_env = nullptr, *n_bins_d = nullptr;
  const size_t raw_bytes = (size_t)w * h * 4, env_bytes = env_tiled_texels(w, h) * 4;
  uint32_t launches = 0, nb = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  hipError_t e = hipSuccess;
  // everything new first: the scene keeps what it has until all of it exists
  if (!env_on_device) e = hold.make(&raw, raw_bytes);
  if (e == hipSuccess) e = hold.make(&n_env, env_bytes);
  if (e == hipSuccess && !env_on_device && !sky) e = hipMemcpy(raw, env, raw_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipEventRecord(K.ev[0], st);
  if (e == hipSuccess && sky) e = sky_launch(sky, w, h, nullptr, (uint32_t *)raw, st, &launches);
  if (e == hipSuccess) e = hipEventRecord(K.ev[1], st);
  if (e == hipSuccess) e = bins_build((const uint8_t *)raw, w, h, hold, W, st, &launches, &nb);
  if (e == hipSuccess) e = hold.make(&n_bins_d, (size_t)nb * 16);
  if (e == hipSuccess) e = bins_emit(W, (uint4 *)n_bins_d, nb, st, &launches);
  if (e == hipSuccess) e = hipEventRecord(K.ev[2], st);
  if (e == hipSuccess) { e = env_tile_launch((const uint32_t *)raw, w, h, (uint32_t *)n_env, st); ++launches; }
  if (e == hipSuccess) e = hipEventRecord(K.ev[3], st);
  if (e == hipSuccess) e = hipEventSynchronize(K.ev[3]);
  for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventElapsedTime(&ms[i], K.ev[i], K.ev[i + 1]);
  if (e != hipSuccess) return ap_fail(fn, e);
  hold.take(n_env); hold.take(n_bins_d);
  environment_swap(s, n_env, env_bytes, w, h, n_bins_d, nb);
  K.sky_ms = sky ? ms[0] : 0.0f; K.bins_ms = ms[1]; K.tile_ms = ms[2];
  K.launches = launches; K.readbacks = 1u; K.n_bins = nb;
  return FSPT_OK;
}

void sky_release(fspt_scene *s) {
  for (hipEvent_t &e : s->sky.ev) if (e) { hipEventDestroy(e); e = nullptr; }
}

} // namespace fspt
