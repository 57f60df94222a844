// fspt_camera_model.hpp - the ray of pixel (x, y) under every camera, two separate statements of two rules:
//   camera_ray   the pinhole camera, the reference's camera.fs; the path kernels (fspt_kernels.hip) fuse it into their first
//                launch.  camera_basis: its basis alone, for a pass that projects a point back (k_temporal_gbuffer).
//   model_ray    the opt-in camera models (fspt_target_set_camera_model): FSPT_CAMERA_ORTHO / _FISHEYE / _EQUIRECT /
//                _STEREO (CAM_* here).  The rule of DESIGN 8.15 and nothing else; tests/camera_model_ref.py restates it in
//                numpy from that text.
//   ray_of       the one or the other by the compile-time MODEL: what the stand-alone passes (fspt_passes.hip: k_camera,
//                k_features) are written against, so that there is one copy of each.
// Rng, the random numbers of a path, is here because camera_ray draws the first four of them.
// Arithmetic: the contract of DESIGN 2 - float32, an fma exactly where one is written.
#pragma once
#include "fspt_device.hpp"
#include "fspt_math.hpp"

namespace fspt {
using namespace fm;

// The random numbers of a path (compile-time choice, fspt.h fspt_target_set_sampler): SMP_REF is the reference's rnd()
// from its running float seed; SMP_SOBOL the Owen-scrambled Sobol sampler (fspt_math.hpp), whose dimension is the number
// of values the sample has drawn so far - camera_ray dims 0..3, then shade_hit's calls in order.
enum { SMP_REF = 0, SMP_SOBOL = 1 };
template <int SMP>
struct Rng {
  float ref;                         // SMP_REF
  uint32_t seed, pixel, sample, dim; // SMP_SOBOL
  FM_DEV float next() {
    if constexpr (SMP == SMP_SOBOL) return sobol_value(seed, pixel, sample, dim++);
    else return rnd(ref);
  }
};

// ---------------------------------------------------------------------------
// camera.fs main (37-46) for pixel (x, y); SMP_SOBOL: sample `sample` of the sampler seeded `sseed`, dims 0..3
// ---------------------------------------------------------------------------
template <int SMP>
FM_DEV void camera_ray(uint32_t x, uint32_t y, uint32_t W, uint32_t H, const CameraP &cam, float randBase, uint32_t sseed,
                       uint32_t sample, V3 &o, V3 &d) {
  float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
  float resx = (float)W, resy = (float)H;
  float uvx = fma_(fx / resx, 2.0f, -1.0f), uvy = fma_(fy / resy, 2.0f, -1.0f);
  Rng<SMP> rng{fma_(fx, resy, randBase) + fy, sseed, y * W + x, sample, 0u};
  V3 Iv = v3(cam.I[0], cam.I[1], cam.I[2]), Pv = v3(cam.P[0], cam.P[1], cam.P[2]);
  V3 basisX = normalize(cross(Iv, v3(0.0f, 1.0f, 0.0f)));
  V3 basisY = normalize(cross(basisX, Iv));
  float fov = cam.fov_scale;
  float icx = uvx * (resx / resy), icy = uvy * 1.0f;
  V3 screen;
  screen.x = (fma_(icy * basisY.x, fov, (icx * basisX.x) * fov) + Iv.x) + Pv.x;
  screen.y = (fma_(icy * basisY.y, fov, (icx * basisX.y) * fov) + Iv.y) + Pv.y;
  screen.z = (fma_(icy * basisY.z, fov, (icx * basisX.z) * fov) + Iv.z) + Pv.z;
  float theta = (rng.next() * M_PI_F) * 2.0f;
  float r = sqrt_(rng.next()) * 1.414f;
  float st, ct;
  sincos_(theta, st, ct);
  V3 aa;
  aa.x = (r * ((basisX.x * ct) / resx + (basisY.x * st) / resy)) * fov;
  aa.y = (r * ((basisX.y * ct) / resx + (basisY.y * st) / resy)) * fov;
  aa.z = (r * ((basisX.z * ct) / resx + (basisY.z * st) / resy)) * fov;
  float theta2 = (rng.next() * M_PI_F) * 2.0f;
  float s2, c2;
  sincos_(theta2, s2, c2);
  float sq = sqrt_(rng.next());
  float lx = cam.lens[0], ly = cam.lens[1];
  V3 dof;
  dof.x = (fma_(s2, basisY.x, c2 * basisX.x) * ly) * sq;
  dof.y = (fma_(s2, basisY.y, c2 * basisX.y) * ly) * sq;
  dof.z = (fma_(s2, basisY.z, c2 * basisX.z) * ly) * sq;
  o = Pv + dof;
  V3 tgt = v3(fma_(dof.x, lx, screen.x + aa.x), fma_(dof.y, lx, screen.y + aa.y), fma_(dof.z, lx, screen.z + aa.z));
  d = normalize(tgt - o);
}
FM_DEV void camera_ray(uint32_t x, uint32_t y, uint32_t W, uint32_t H, const CameraP &cam, float randBase, V3 &o, V3 &d) {
  camera_ray<SMP_REF>(x, y, W, H, cam, randBase, 0u, 0u, o, d);
}
// camera.fs's basis of a camera: basisX, basisY as camera_ray computes them (same float32 operations)
FM_DEV void camera_basis(const CameraP &cam, V3 &Iv, V3 &Pv, V3 &basisX, V3 &basisY) {
  Iv = v3(cam.I[0], cam.I[1], cam.I[2]); Pv = v3(cam.P[0], cam.P[1], cam.P[2]);
  basisX = normalize(cross(Iv, v3(0.0f, 1.0f, 0.0f)));
  basisY = normalize(cross(basisX, Iv));
}

// ---------------------------------------------------------------------------
// The opt-in camera models
// ---------------------------------------------------------------------------

// SMP: FSPT_SAMPLER_REFERENCE (0) - the reference's rnd() from the seed fma(fx, resy, randBase) + fy - or FSPT_SAMPLER_SOBOL
// (1) - dims 0..3 of sample `sample` of pixel y * W + x.  The four draws are camera_ray's, in its order.
template <int SMP, int MODEL>
FM_DEV void model_ray(uint32_t x, uint32_t y, uint32_t W, uint32_t H, const CameraP &cam, const CameraModelP &cm, float randBase,
                      uint32_t sseed, uint32_t sample, fm::V3 &o, fm::V3 &d) {
  using namespace fm;
  const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
  const float resx = (float)W, resy = (float)H;
  float u0, u1, u2, u3;
  if constexpr (SMP == 1) {
    const uint32_t pixel = y * W + x;
    u0 = sobol_value(sseed, pixel, sample, 0u); u1 = sobol_value(sseed, pixel, sample, 1u);
    u2 = sobol_value(sseed, pixel, sample, 2u); u3 = sobol_value(sseed, pixel, sample, 3u);
  } else {
    float seed = fma_(fx, resy, randBase) + fy;
    u0 = rnd(seed); u1 = rnd(seed); u2 = rnd(seed); u3 = rnd(seed);
  }
  const V3 Iv = v3(cam.I[0], cam.I[1], cam.I[2]), Pv = v3(cam.P[0], cam.P[1], cam.P[2]);
  const V3 basisX = normalize(cross(Iv, v3(0.0f, 1.0f, 0.0f)));
  const V3 basisY = normalize(cross(basisX, Iv));
  const V3 F = normalize(Iv);
  const float aspect = resx / resy;
  // the jitter: a disc of radius 0.707 pixels around the pixel centre, in pixel units
  const float theta = (u0 * M_PI_F) * 2.0f;
  const float r = sqrt_(u1) * 0.707f;
  float st, ct;
  sincos_(theta, st, ct);
  const float px = fma_(r, ct, fx), py = fma_(r, st, fy);
  const float u = fma_(px / resx, 2.0f, -1.0f);
  float v;
  bool upper = false;
  if constexpr (MODEL == CAM_STEREO) {
    const uint32_t half = H / 2u;
    upper = y >= half;
    const float y_half = upper ? (float)half : 0.0f;
    v = fma_((py - y_half) / (resy * 0.5f), 2.0f, -1.0f);
  } else {
    v = fma_(py / resy, 2.0f, -1.0f);
  }
  V3 o0 = Pv, d0 = F;
  if constexpr (MODEL == CAM_ORTHO) {
    const float a = u * aspect, fov = cam.fov_scale;
    o0.x = fma_(v * basisY.x, fov, (a * basisX.x) * fov) + Pv.x;
    o0.y = fma_(v * basisY.y, fov, (a * basisX.y) * fov) + Pv.y;
    o0.z = fma_(v * basisY.z, fov, (a * basisX.z) * fov) + Pv.z;
  } else if constexpr (MODEL == CAM_FISHEYE) {
    const float sx = u * aspect, sy = v;
    const float rho = sqrt_(fma_(sy, sy, sx * sx));
    const float phi = min_(rho * (cm.angle * 0.5f), M_PI_F);
    float sp, cp;
    sincos_(phi, sp, cp);
    if (rho != 0.0f) {
      const float ex = sx / rho, ey = sy / rho;
      d0.x = fma_(sp, fma_(ey, basisY.x, ex * basisX.x), cp * F.x);
      d0.y = fma_(sp, fma_(ey, basisY.y, ex * basisX.y), cp * F.y);
      d0.z = fma_(sp, fma_(ey, basisY.z, ex * basisX.z), cp * F.z);
    }
  } else { // EQUIRECT, STEREO
    const float lon = u * M_PI_F, lat = v * (M_PI_F * 0.5f);
    float sl, cl, sa, ca;
    sincos_(lon, sl, cl);
    sincos_(lat, sa, ca);
    d0.x = fma_(sa, basisY.x, ca * fma_(sl, basisX.x, cl * F.x));
    d0.y = fma_(sa, basisY.y, ca * fma_(sl, basisX.y, cl * F.y));
    d0.z = fma_(sa, basisY.z, ca * fma_(sl, basisX.z, cl * F.z));
    if constexpr (MODEL == CAM_STEREO) {
      const float e = upper ? -(cm.ipd * 0.5f) : cm.ipd * 0.5f; // the upper half of the picture is the left eye
      o0.x = fma_(e, fma_(-sl, F.x, cl * basisX.x), Pv.x);
      o0.y = fma_(e, fma_(-sl, F.y, cl * basisX.y), Pv.y);
      o0.z = fma_(e, fma_(-sl, F.z, cl * basisX.z), Pv.z);
    }
  }
  const float lx = cam.lens[0], ly = cam.lens[1];
  if (ly == 0.0f || lx >= 1.0f) { o = o0; d = d0; return; }
  // thin lens: the aperture disc in the basisX / basisY plane, the focus at distance f along the unlensed ray
  const float f = 1.0f / (1.0f - lx);
  const float theta2 = (u2 * M_PI_F) * 2.0f;
  float s2, c2;
  sincos_(theta2, s2, c2);
  const float sq = sqrt_(u3);
  V3 dof;
  dof.x = (fma_(s2, basisY.x, c2 * basisX.x) * ly) * sq;
  dof.y = (fma_(s2, basisY.y, c2 * basisX.y) * ly) * sq;
  dof.z = (fma_(s2, basisY.z, c2 * basisX.z) * ly) * sq;
  o = o0 + dof;
  const V3 tgt = v3(fma_(f, d0.x, o0.x), fma_(f, d0.y, o0.y), fma_(f, d0.z, o0.z));
  d = normalize(tgt - o);
}

// The ray of pixel (x, y) under camera MODEL (CAM_*): the pinhole camera's, which has no parameters (cm is not read), or the model's
template <int SMP, int MODEL>
FM_DEV void ray_of(uint32_t x, uint32_t y, uint32_t W, uint32_t H, const CameraP &cam, const CameraModelP &cm, float randBase,
                   uint32_t sseed, uint32_t sample, V3 &o, V3 &d) {
  if constexpr (MODEL == CAM_PINHOLE) camera_ray<SMP>(x, y, W, H, cam, randBase, sseed, sample, o, d);
  else model_ray<SMP, MODEL>(x, y, W, H, cam, cm, randBase, sseed, sample, o, d);
}

} // namespace fspt
