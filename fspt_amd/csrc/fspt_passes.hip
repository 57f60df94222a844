// fspt_passes.hip - the stand-alone passes and test hooks of libfspt: gfx950 kernels that no renderer calls, each with its
// launcher, one copy of each.  They are built on the device code the renderers use (fspt_traverse.hpp, fspt_surface.hpp,
// fspt_camera_model.hpp), so a pass computes what the path kernels compute, bit for bit.
//   k_camera<SMP, MODEL>   one tick's rays into the target's ray buffers: camera.fs as a stand-alone pass (the pinhole camera
//                          is otherwise fused into the path kernels), or an opt-in camera model, once per tick in
//                          front of the single-tick trace from the ray buffers
//   k_intersect            intersectScene for a list of rays (fspt_intersect)
//   k_features<MODEL>      the denoiser's guide buffers of the first hit, under the target's camera
//   k_mattes<MODEL, NK>    the ID mattes of the first hit: k_features' rays, a ranking table per kind in registers
//   k_temporal_gbuffer     the G-buffer and motion pass of temporal accumulation
//   k_adaptive_error / k_adaptive_select   adaptive sampling's per-tile error and tile list
//   k_sampler_eval, k_math                 test hooks: the Sobol sampler and fspt-math, value by value
// The camera model (and k_camera's sampler) is a template parameter chosen by the launcher: no switch in a kernel.
#include "fspt_traverse.hpp"
#include "fspt_surface.hpp"
#include "fspt_camera_model.hpp"

namespace fspt {

// the camera model of a launch as the compile-time argument of f (a std::integral_constant); a missing model is an error
template <class F> static hipError_t with_model(int model, F &&f) {
  switch (model) {
    case CAM_PINHOLE: return f(std::integral_constant<int, CAM_PINHOLE>{});
    case CAM_ORTHO: return f(std::integral_constant<int, CAM_ORTHO>{});
    case CAM_FISHEYE: return f(std::integral_constant<int, CAM_FISHEYE>{});
    case CAM_EQUIRECT: return f(std::integral_constant<int, CAM_EQUIRECT>{});
    case CAM_STEREO: return f(std::integral_constant<int, CAM_STEREO>{});
    default: return hipErrorInvalidValue;
  }
}

// Ray generation (drawCamera, main.js:741-756).  One thread per pixel of the target in row order; a lane stores two
// float4 (pos, dir), so a wave's stores are two contiguous 1 KB runs.  Nothing is loaded from memory but the kernel
// arguments, nothing is shared between lanes: no LDS.
template <int SMP, int MODEL>
__global__ __launch_bounds__(BLOCK_THREADS) void k_camera(uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, CameraP cam, CameraModelP cm,
                                                         float randBase, uint32_t sseed, uint32_t sample, float4 *pos, float4 *dir) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t x = i % W, y = i / W;
  if (x >= vw || y >= vh) return; // outside gl.viewport: the ray textures keep their old texels
  V3 o, d;
  ray_of<SMP, MODEL>(x, y, W, H, cam, cm, randBase, sseed, sample, o, d);
  pos[i] = make_float4(o.x, o.y, o.z, 1.0f);
  dir[i] = make_float4(d.x, d.y, d.z, 1.0f);
}

// the Sobol sampler's device function for n (pixel, sample, dim) triples (fspt_sampler_eval, a test hook)
__global__ void k_sampler_eval(uint32_t seed, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, uint32_t n, float *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sobol_value(seed, pixel[i], sample[i], dim[i]);
}

// intersectScene as a stand-alone pass
__global__ __launch_bounds__(BLOCK_THREADS) void k_intersect(const IntersectP p) {
  extern __shared__ int lds_stack[];
  int *stack = lane_stack(lds_stack, threadIdx.x, p.scene.stack_n);
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  V3 o = v3(p.rays[i * 6], p.rays[i * 6 + 1], p.rays[i * 6 + 2]);
  V3 d = v3(p.rays[i * 6 + 3], p.rays[i * 6 + 4], p.rays[i * 6 + 5]);
  Counters cnt = {0, 0, 0, 0, 0, 0};
  int hitA, hitB;
  float tB;
  if (p.wide) trace_rays<true, false, true>(p.scene, stack, o, false, d, d, hitA, tB, hitB, cnt);
  else trace_rays<true, false>(p.scene, stack, o, false, d, d, hitA, tB, hitB, cnt);
  p.t_out[i] = tB;
  p.index_out[i] = slot_to_tri(p.scene, hitB); // the reference's triangle index (tracer.fs:360)
  if (p.steps_out) p.steps_out[i] = cnt.steps;
  if (p.leaves_out) p.leaves_out[i] = cnt.leaves;
}

__global__ void k_math(int op, const float *a, const float *b, uint32_t n, float *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = a[i], y = b ? b[i] : 0.0f, r = 0.0f;
  switch (op) {
    case 0: r = sin_(x); break;
    case 1: r = cos_(x); break;
    case 2: r = atan2_(x, y); break;
    case 3: r = asin_(x); break;
    case 4: r = exp2_(x); break;
    case 5: r = x / y; break;
    case 6: r = sqrt_(x); break;
    case 7: { float sd = x; r = rnd(sd); break; }
    case 8: r = fract_(x); break;
    case 9: r = log2_(x); break;
    case 10: r = pow_(x, y); break;
    default: r = 0.0f;
  }
  out[i] = r;
}

// ---------------------------------------------------------------------------
// Guided denoiser: the guide buffers of the first hit (the a-trous filter that reads them: fspt_post.hip).
// ---------------------------------------------------------------------------
// fspt_rand_base_next on the device: the s-th value of the host stream seeded with `seed` (same integer steps, same one
// rounding in the float multiply: bit-identical)
FM_DEV float rand_base_step(uint64_t &st) {
  uint64_t x = st;
  x ^= x >> 12;
  x ^= x << 25;
  x ^= x >> 27;
  st = x;
  const uint64_t r = x * 2685821657736338717ULL;
  return ((float)(r >> 40) * (1.0f / 16777216.0f)) * 10000.0f;
}

// The kernel's parameter block is FeatureP under the pinhole camera, which has no parameters, and FeatureModelP under a model
FM_DEV const FeatureP &feature_p(const FeatureP &p) { return p; }
FM_DEV const FeatureP &feature_p(const FeatureModelP &p) { return p.f; }
FM_DEV CameraModelP model_p(const FeatureP &) { return CameraModelP{}; }
FM_DEV const CameraModelP &model_p(const FeatureModelP &p) { return p.cm; }

// One thread per pixel of the whole target (16 x 16-pixel blocks: a wave's camera rays start on a 16 x 4 patch), `samples`
// camera rays each - exactly k_camera's ray for randBase r_s, under the same camera model, so that the guides follow the
// camera - traced to their closest hit with the wave's LDS stack like k_intersect.  Per pixel: the float32 sums in sample
// order / samples of (texDiffuse, t) and (macroNormal, hit); a miss counts as albedo (1, 1, 1), normal 0, depth MAX_T, hit 0.
template <int MODEL, class P>
__global__ __launch_bounds__(BLOCK_THREADS) void k_features(const P pp) {
  extern __shared__ int lds_stack[];
  const FeatureP &p = feature_p(pp);
  const DScene &S = p.scene;
  int *stack = lane_stack(lds_stack, threadIdx.y * blockDim.x + threadIdx.x, S.stack_n);
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= p.W || y >= p.H) return;
  Counters cnt = {0, 0, 0, 0, 0, 0};
  uint64_t st = p.seed;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, z = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, hits = 0.0f;
  for (uint32_t s = 0; s < p.samples; ++s) {
    const float rb = rand_base_step(st);
    V3 o, d;
    ray_of<SMP_REF, MODEL>(x, y, p.W, p.H, p.cam, model_p(pp), rb, 0u, 0u, o, d);
    int hitA, hitB;
    float tB;
    trace_rays<false, false>(S, stack, o, false, d, d, hitA, tB, hitB, cnt);
    V3 a = v3(1.0f, 1.0f, 1.0f), n = v3(0.0f, 0.0f, 0.0f);
    float h = 0.0f;
    if (hitB >= 0) {
      first_hit_guides(S, o, d, tB, hitB, a, n);
      h = 1.0f;
    }
    ar += a.x; ag += a.y; ab += a.z; z += tB;
    nx += n.x; ny += n.y; nz += n.z; hits += h;
  }
  const float fs = (float)p.samples;
  const size_t i = (size_t)y * p.W + x;
  p.feat[2 * i] = make_float4(ar / fs, ag / fs, ab / fs, z / fs);
  p.feat[2 * i + 1] = make_float4(nx / fs, ny / fs, nz / fs, hits / fs);
}

// ---- ID mattes (fspt_mattes) ---------------------------------------------------------------------------
// A pixel's ranking table of one kind: six (id, count) slots, empty = id 0, filled from slot 0 up.  Twelve named scalars
// and no array: every step below is an unrolled compare-and-select, so the table stays in registers (an array indexed by
// a variable, or a conditional among neighbouring members, would go through scratch - see fspt_exr.hip's exr_sel).
struct MatteTab { uint32_t i0, i1, i2, i3, i4, i5, c0, c1, c2, c3, c4, c5; };

// One sample's id (0: a miss or a triangle without a matte, skipped): the slot that holds it counts it, else the lowest
// empty slot takes (id, 1), else the sample is lost.  Returns the samples lost: 0 or 1.
FM_DEV uint32_t matte_count(MatteTab &t, uint32_t id) {
  const bool live = id != 0u;
  const bool h0 = live && t.i0 == id, h1 = live && t.i1 == id, h2 = live && t.i2 == id, h3 = live && t.i3 == id, h4 = live && t.i4 == id, h5 = live && t.i5 == id;
  const bool take = live && !(h0 || h1 || h2 || h3 || h4 || h5);
  const bool e0 = take && t.i0 == 0u, e1 = take && t.i0 != 0u && t.i1 == 0u, e2 = take && t.i1 != 0u && t.i2 == 0u, e3 = take && t.i2 != 0u && t.i3 == 0u,
             e4 = take && t.i3 != 0u && t.i4 == 0u, e5 = take && t.i4 != 0u && t.i5 == 0u;
  const uint32_t lost = (uint32_t)(take && t.i5 != 0u);
  t.i0 = e0 ? id : t.i0; t.i1 = e1 ? id : t.i1; t.i2 = e2 ? id : t.i2; t.i3 = e3 ? id : t.i3; t.i4 = e4 ? id : t.i4; t.i5 = e5 ? id : t.i5;
  t.c0 += (uint32_t)(h0 || e0); t.c1 += (uint32_t)(h1 || e1); t.c2 += (uint32_t)(h2 || e2); t.c3 += (uint32_t)(h3 || e3); t.c4 += (uint32_t)(h4 || e4); t.c5 += (uint32_t)(h5 || e5);
  return lost;
}

// compare-exchange of two (key, id) pairs: the larger key first
#define MATTE_CX(ka, ia, kb, ib) do { const bool sw_ = ka < kb; const uint32_t k0_ = sw_ ? kb : ka, k1_ = sw_ ? ka : kb, i0_ = sw_ ? ib : ia, i1_ = sw_ ? ia : ib; ka = k0_; kb = k1_; ia = i0_; ib = i1_; } while (0)

// The ranks of a table - its slots by count descending, ties by slot ascending - as the pixel's three float4: a fixed
// 12-comparator sorting network on the unique keys (count << 3) | (7 - slot), the ids carried along.
FM_DEV void matte_store(const MatteTab &t, float fs, float4 *out) {
  uint32_t k0 = (t.c0 << 3) | 7u, k1 = (t.c1 << 3) | 6u, k2 = (t.c2 << 3) | 5u, k3 = (t.c3 << 3) | 4u, k4 = (t.c4 << 3) | 3u, k5 = (t.c5 << 3) | 2u;
  uint32_t i0 = t.i0, i1 = t.i1, i2 = t.i2, i3 = t.i3, i4 = t.i4, i5 = t.i5;
  MATTE_CX(k0, i0, k5, i5); MATTE_CX(k1, i1, k3, i3); MATTE_CX(k2, i2, k4, i4);
  MATTE_CX(k1, i1, k2, i2); MATTE_CX(k3, i3, k4, i4);
  MATTE_CX(k0, i0, k3, i3); MATTE_CX(k2, i2, k5, i5);
  MATTE_CX(k0, i0, k1, i1); MATTE_CX(k2, i2, k3, i3); MATTE_CX(k4, i4, k5, i5);
  MATTE_CX(k1, i1, k2, i2); MATTE_CX(k3, i3, k4, i4);
  out[0] = make_float4(__uint_as_float(i0), (float)(k0 >> 3) / fs, __uint_as_float(i1), (float)(k1 >> 3) / fs);
  out[1] = make_float4(__uint_as_float(i2), (float)(k2 >> 3) / fs, __uint_as_float(i3), (float)(k3 >> 3) / fs);
  out[2] = make_float4(__uint_as_float(i4), (float)(k4 >> 3) / fs, __uint_as_float(i5), (float)(k5 >> 3) / fs);
}

// a wave's lost samples into the kind's counter: one atomic per wave that lost any
FM_DEV void matte_lost(uint32_t lost, unsigned long long *counter) {
  for (int off = WAVE / 2; off > 0; off >>= 1) lost += __shfl_down(lost, off, WAVE);
  if (((threadIdx.y * blockDim.x + threadIdx.x) & (WAVE - 1)) == 0 && lost) atomicAdd(counter, (unsigned long long)lost);
}

FM_DEV const MatteP &matte_p(const MatteP &p) { return p; }
FM_DEV const MatteP &matte_p(const MatteModelP &p) { return p.m; }
FM_DEV CameraModelP model_p(const MatteP &) { return CameraModelP{}; }
FM_DEV const CameraModelP &model_p(const MatteModelP &p) { return p.cm; }

// One thread per pixel of the whole target, 16 x 16-pixel blocks and the wave's LDS stack like k_features, whose rays these
// are: sample s is ray_of's ray for the s-th randBase of the stream, traced once to its closest hit; the hit triangle's id
// of each kind (NK = 1: table a alone, 2: a and b from the same hit) goes through matte_count in sample order.  A lane
// outside the target traces nothing and stays for the wave's sum of lost samples.
template <int MODEL, int NK, class P>
__global__ __launch_bounds__(BLOCK_THREADS) void k_mattes(const P pp) {
  extern __shared__ int lds_stack[];
  const MatteP &m = matte_p(pp);
  const FeatureP &p = m.f;
  const DScene &S = p.scene;
  int *stack = lane_stack(lds_stack, threadIdx.y * blockDim.x + threadIdx.x, S.stack_n);
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  const bool inside = x < p.W && y < p.H;
  Counters cnt = {0, 0, 0, 0, 0, 0};
  uint64_t st = p.seed;
  MatteTab ta = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, tb = ta;
  uint32_t lost_a = 0u, lost_b = 0u;
  const uint32_t n = inside ? p.samples : 0u;
  for (uint32_t s = 0; s < n; ++s) {
    const float rb = rand_base_step(st);
    V3 o, d;
    ray_of<SMP_REF, MODEL>(x, y, p.W, p.H, p.cam, model_p(pp), rb, 0u, 0u, o, d);
    int hitA, hitB;
    float tB;
    trace_rays<false, false>(S, stack, o, false, d, d, hitA, tB, hitB, cnt);
    const int tri = slot_to_tri(S, hitB);
    lost_a += matte_count(ta, tri >= 0 ? m.ids_a[tri] : 0u);
    if constexpr (NK == 2) lost_b += matte_count(tb, tri >= 0 ? m.ids_b[tri] : 0u);
  }
  const float fs = (float)p.samples;
  const size_t i = (size_t)y * p.W + x;
  if (inside) matte_store(ta, fs, m.out_a + 3 * i);
  matte_lost(lost_a, m.lost_a);
  if constexpr (NK == 2) {
    if (inside) matte_store(tb, fs, m.out_b + 3 * i);
    matte_lost(lost_b, m.lost_b);
  }
}

// ---- temporal accumulation (fspt_temporal_accumulate): the G-buffer pass (blend, clamp, variance: fspt_post.hip) ----
// The G-buffer and motion pass: one thread per pixel of the whole target, 16 x 16-pixel blocks and the wave's LDS stack
// like k_features.  The CENTRE ray - camera_ray without pixel jitter and without lens offset: o = P, d = normalize(screen -
// P), `screen` by camera_ray's own operations - is traced to its closest hit; G = (t, slot bits, bv, bw), (macroNormal, hit).
// The hit point's position in the PREVIOUS frame (the motion-origin snapshot's triangle of the same slot at the same
// barycentric weights, or the point itself) is projected into the previous camera: M = (sx, sy, |v|, kind).
__global__ __launch_bounds__(BLOCK_THREADS) void k_temporal_gbuffer(const TemporalGP p) {
  extern __shared__ int lds_stack[];
  const DScene &S = p.scene;
  int *stack = lane_stack(lds_stack, threadIdx.y * blockDim.x + threadIdx.x, S.stack_n);
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= p.W || y >= p.H) return;
  const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
  const float resx = (float)p.W, resy = (float)p.H;
  const float uvx = fma_(fx / resx, 2.0f, -1.0f), uvy = fma_(fy / resy, 2.0f, -1.0f);
  V3 Iv, Pv, basisX, basisY;
  camera_basis(p.cam, Iv, Pv, basisX, basisY);
  const float fov = p.cam.fov_scale;
  const float icx = uvx * (resx / resy), icy = uvy * 1.0f;
  V3 screen;
  screen.x = (fma_(icy * basisY.x, fov, (icx * basisX.x) * fov) + Iv.x) + Pv.x;
  screen.y = (fma_(icy * basisY.y, fov, (icx * basisX.y) * fov) + Iv.y) + Pv.y;
  screen.z = (fma_(icy * basisY.z, fov, (icx * basisX.z) * fov) + Iv.z) + Pv.z;
  const V3 o = Pv, d = normalize(screen - Pv);
  Counters cnt = {0, 0, 0, 0, 0, 0};
  int hitA, hitB;
  float tB;
  trace_rays<false, false>(S, stack, o, false, d, d, hitA, tB, hitB, cnt);
  const size_t i = (size_t)y * p.W + x;
  V3 n = v3(0.0f, 0.0f, 0.0f), xp = d;
  float bv = 0.0f, bw = 0.0f;
  const bool hit = hitB >= 0;
  if (hit) {
    HitGeom g;
    V3 albedo;
    first_hit_guides(S, o, d, tB, hitB, albedo, n, g);
    bv = g.w.y; bw = g.w.z;
    xp = g.origin; // o + t d
    if (p.origin) { // where the same point of the same triangle was when fspt_scene_motion_begin took the snapshot
      const float *mp = p.origin + (size_t)hitB * MOTION_FLOATS; // v1.xyz e1.xyz e2.xyz
      xp = v3(fma_(bw, mp[6], fma_(bv, mp[3], mp[0])), fma_(bw, mp[7], fma_(bv, mp[4], mp[1])), fma_(bw, mp[8], fma_(bv, mp[5], mp[2])));
    }
  }
  p.g[2 * i] = make_float4(hit ? tB : MAX_T, __int_as_float(hit ? hitB : -1), bv, bw);
  p.g[2 * i + 1] = make_float4(n.x, n.y, n.z, hit ? 1.0f : 0.0f);
  float4 m = make_float4(0.0f, 0.0f, 0.0f, TM_KIND_NONE);
  if (p.has_prev) {
    V3 I2, P2, bX, bY;
    camera_basis(p.prev, I2, P2, bX, bY);
    const V3 v = hit ? xp - P2 : d;
    const float a = dot(v, I2) / dot(I2, I2);
    if (a > 0.0f) {
      const float den = a * p.prev.fov_scale;
      const float jcx = dot(v, bX) / den, jcy = dot(v, bY) / den;
      float sx = ((jcx * (resy / resx)) + 1.0f) * (resx * 0.5f) - 0.5f;
      float sy = (jcy + 1.0f) * (resy * 0.5f) - 0.5f;
      const float rx = floor_(sx + 0.5f), ry = floor_(sy + 0.5f);
      if (abs_(sx - rx) <= TM_SNAP) sx = rx;
      if (abs_(sy - ry) <= TM_SNAP) sy = ry;
      m = make_float4(sx, sy, hit ? sqrt_(dot(v, v)) : 0.0f, hit ? TM_KIND_HIT : TM_KIND_MISS);
    }
  }
  p.m[i] = m;
}

// ---- adaptive sampling (fspt_render_adaptive) -------------------------------------------------------------
// One workgroup per active tile (list order).  Every thread sums its pixels (j = thread, thread + 256, ... of the tile,
// row-major) in float64, the wave folds its 64 sums by shuffles and the four wave sums are added in wave order: the same
// bits on every run.  E_T = sum over the tile's viewport pixels and 3 channels of r / (3 pixels), with
// r = v / (I^2 + 0.01) and v = (B - S)^2 m (n - m) / n^2 = m (I - S)^2 / (n - m)  (B = (n I - m S) / (n - m)).
// m = 0: no estimate, only S := I;  refresh: S := I as well (read once, written in the same pass).
__global__ __launch_bounds__(BLOCK_THREADS) void k_adaptive_error(const AdaptiveP p) {
  __shared__ double wsum[BLOCK_THREADS / WAVE];
  const uint32_t g = p.list_in[blockIdx.x];
  const uint32_t x0 = (g % p.tiles_x) * p.tile, y0 = (g / p.tiles_x) * p.tile;
  const uint32_t wx = min(p.tile, p.vw - x0), wy = min(p.tile, p.vh - y0); // (listed tiles meet the viewport)
  const bool est = p.m != 0u, store = p.refresh != 0u || !est;
  const double scale = est ? (double)p.m / (double)(p.n - p.m) : 0.0;
  double acc = 0.0;
  for (uint32_t j = threadIdx.x; j < wx * wy; j += BLOCK_THREADS) {
    const uint32_t y = y0 + j / wx, x = x0 + j % wx;
    const size_t i = (size_t)y * p.W + x;
    const float4 I = p.accum[i];
    if (est) {
      const float4 S = p.snap[i];
      const double c[3] = {(double)I.x, (double)I.y, (double)I.z}, d[3] = {(double)I.x - (double)S.x, (double)I.y - (double)S.y,
                                                                          (double)I.z - (double)S.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) acc += (scale * (d[k] * d[k])) / (c[k] * c[k] + 0.01);
    }
    if (store) p.snap[i] = I;
  }
  if (!est) return;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int off = WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, WAVE);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < BLOCK_THREADS / WAVE; ++w) t += wsum[w];
    p.err[g] = t / (3.0 * (double)(wx * wy));
  }
}

// One workgroup of ADAPTIVE_SELECT_THREADS walks list_in in chunks: a tile retires when n = max_ticks or (n >= min_ticks
// and E_T < target) - count[g] = n, err[g] keeps the E_T that retired it - and every other tile goes to list_out at its
// rank among the kept ones (ballot + mbcnt inside a wave, the wave totals from LDS in wave order): ascending order, no
// atomics.  *n_out = the kept tiles.
#define ADAPTIVE_SELECT_THREADS 1024
__global__ __launch_bounds__(ADAPTIVE_SELECT_THREADS) void k_adaptive_select(const AdaptiveP p) {
  __shared__ uint32_t wcount[ADAPTIVE_SELECT_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  uint32_t base_out = 0;
  for (uint32_t base = 0; base < p.n_in; base += ADAPTIVE_SELECT_THREADS) {
    const uint32_t i = base + threadIdx.x;
    bool keep = false;
    uint32_t g = 0;
    if (i < p.n_in) {
      g = p.list_in[i];
      const bool retire = p.n >= p.max_ticks || (p.n >= p.min_ticks && p.err[g] < p.target);
      if (retire) p.count[g] = p.n;
      keep = !retire;
    }
    const unsigned long long mask = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < ADAPTIVE_SELECT_THREADS / WAVE; ++w) {
      if (w < wave) before += wcount[w];
      total += wcount[w];
    }
    if (keep) p.list_out[base_out + before + rank] = g;
    base_out += total;
    __syncthreads(); // (wcount is rewritten by the next chunk)
  }
  if (threadIdx.x == 0) *p.n_out = base_out;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_camera(uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const CameraP &cam, const CameraModelP &cm, float rand_base,
                         float4 *pos, float4 *dir, hipStream_t stream, uint32_t sampler, uint32_t smp_seed, uint32_t sample) {
  const uint32_t n = W * H;
  if (n == 0) return hipSuccess;
  if (sampler > 1u) return hipErrorInvalidValue;
  const dim3 g((n + BLOCK_THREADS - 1) / BLOCK_THREADS), b(BLOCK_THREADS);
  const hipError_t e = with_model(cm.model, [&](auto M) {
    // (the reference sampler takes no seed and no sample number)
    if (sampler) hipLaunchKernelGGL((k_camera<SMP_SOBOL, M>), g, b, 0, stream, W, H, vw, vh, cam, cm, rand_base, smp_seed, sample, pos, dir);
    else hipLaunchKernelGGL((k_camera<SMP_REF, M>), g, b, 0, stream, W, H, vw, vh, cam, cm, rand_base, 0u, 0u, pos, dir);
    return hipSuccess;
  });
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_sampler_eval(uint32_t seed, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, uint32_t n,
                               float *out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sampler_eval, dim3((n + 255) / 256), dim3(256), 0, stream, seed, pixel, sample, dim, n, out);
  return hipGetLastError();
}

hipError_t launch_intersect(const IntersectP &p, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  const hipError_t e = launch(k_intersect, dim3((p.n + BLOCK_THREADS - 1) / BLOCK_THREADS), dim3(BLOCK_THREADS), stack_bytes(p.scene), stream, p);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_math(int op, const float *a, const float *b, uint32_t n, float *out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_math, dim3((n + 255) / 256), dim3(256), 0, stream, op, a, b, n, out);
  return hipGetLastError();
}

hipError_t launch_features(const FeatureP &p, const CameraModelP &cm, hipStream_t stream) {
  const dim3 g((p.W + 15) / 16, (p.H + 15) / 16), b(16, 16);
  const size_t lds = stack_bytes(p.scene);
  const hipError_t e = with_model(cm.model, [&](auto M) {
    if constexpr (M == CAM_PINHOLE) return launch(k_features<M, FeatureP>, g, b, lds, stream, p);
    else return launch(k_features<M, FeatureModelP>, g, b, lds, stream, FeatureModelP{p, cm});
  });
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_mattes(const MatteP &p, const CameraModelP &cm, hipStream_t stream) {
  const FeatureP &f = p.f;
  const dim3 g((f.W + 15) / 16, (f.H + 15) / 16), b(16, 16);
  const size_t lds = stack_bytes(f.scene);
  hipError_t e = hipMemsetAsync(p.lost_a, 0, 8, stream);
  if (e == hipSuccess && p.ids_b) e = hipMemsetAsync(p.lost_b, 0, 8, stream);
  if (e != hipSuccess) return e;
  e = with_model(cm.model, [&](auto M) {
    if constexpr (M == CAM_PINHOLE) return p.ids_b ? launch(k_mattes<M, 2, MatteP>, g, b, lds, stream, p) : launch(k_mattes<M, 1, MatteP>, g, b, lds, stream, p);
    else return p.ids_b ? launch(k_mattes<M, 2, MatteModelP>, g, b, lds, stream, MatteModelP{p, cm}) : launch(k_mattes<M, 1, MatteModelP>, g, b, lds, stream, MatteModelP{p, cm});
  });
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_temporal_gbuffer(const TemporalGP &p, hipStream_t stream) {
  const hipError_t e = launch(k_temporal_gbuffer, dim3((p.W + 15) / 16, (p.H + 15) / 16), dim3(16, 16), stack_bytes(p.scene), stream, p);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_adaptive_error(const AdaptiveP &p, hipStream_t stream) {
  if (p.n_in == 0) return hipSuccess;
  hipLaunchKernelGGL(k_adaptive_error, dim3(p.n_in), dim3(BLOCK_THREADS), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_adaptive_select(const AdaptiveP &p, hipStream_t stream) {
  hipLaunchKernelGGL(k_adaptive_select, dim3(1), dim3(ADAPTIVE_SELECT_THREADS), 0, stream, p);
  return hipGetLastError();
}

} // namespace fspt
