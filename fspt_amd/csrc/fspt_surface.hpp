// fspt_surface.hpp - from a hit to surface data: the tiled texture fetches, material<> (the four atlas layers of a material
// texture set at one uv), the hit record (HitGeom / hit_geom), macro_normal and first_hit_guides.  shade_hit and the emitter
// code (fspt_kernels.hip) and the passes that store a first hit's albedo and normal (fspt_passes.hip: k_features,
// k_temporal_gbuffer) are built on these, so a guide is what the path tracer itself would shade with, bit for bit.
#pragma once
#include "fspt_device.hpp"
#include "fspt_math.hpp"

namespace fspt {
using namespace fm;

#ifndef FSPT_TAP2
#define FSPT_TAP2 1
#endif

// ---------------------------------------------------------------------------
// Texture fetches (sampler state: main.js:170-180, 548-559)
// ---------------------------------------------------------------------------
// (float)b / 255.0f, exactly (verified for all 256 bytes: one Newton step on
// the rounded reciprocal is correctly rounded for these operands)
FM_DEV float unorm8(uint32_t b) {
  const float rc = 1.0f / 255.0f;
  float x = (float)b;
  float q = x * rc;
  float r = fma_(-q, 255.0f, x);
  return fma_(r, rc, q);
}
FM_DEV int wrap_repeat(int i, int n) { int m = i % n; return m < 0 ? m + n : m; }
FM_DEV int wrap_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
FM_DEV float safe_floor_coord(float u) {
  float f = floor_(u);
  if (!(f > -1.0e9f && f < 1.0e9f)) f = 0.0f;
  return f;
}
struct Tap4 { uint32_t t00, t10, t01, t11; float a, b; };
// Texel (i, j) of a w-wide image stored in tiles of 2^WL2 x 2^HL2 texels (fspt_device.hpp): one tile = one 128-byte
// cache line, so the 2 x 2 footprint of a bilinear fetch lies in 1.4 lines on average (8 x 4 tiles) instead of 2 rows = 2 lines.
template <int WL2, int HL2>
FM_DEV uint32_t tile_offset(int i, int j, int tiles_x) {
  return (uint32_t)(((j >> HL2) * tiles_x + (i >> WL2)) << (WL2 + HL2)) + (uint32_t)(((j & ((1 << HL2) - 1)) << WL2) + (i & ((1 << WL2) - 1)));
}
// Footprint of a bilinear fetch at (s, t): the wrapped texel coordinates and the two weights.  Shared by the four atlas
// layers a shading event reads at the same uv (tracer.fs:453-456): the wrap / floor arithmetic is done once.
struct TexCoord { int i0, i1, j0, j1; float a, b; };
FM_DEV TexCoord bilinear_coord(int w, int h, float s, float t, bool repeat_t) {
  TexCoord c;
  float u = fma_(s, (float)w, -0.5f), v = fma_(t, (float)h, -0.5f);
  float fu = safe_floor_coord(u), fv = safe_floor_coord(v);
  float a = u - fu, b = v - fv;
  if (!(a >= 0.0f && a <= 1.0f)) a = 0.0f;
  if (!(b >= 0.0f && b <= 1.0f)) b = 0.0f;
  int i0 = (int)fu, j0 = (int)fv;
  c.i1 = wrap_repeat(i0 + 1, w);
  c.i0 = wrap_repeat(i0, w);
  if (repeat_t) { c.j1 = wrap_repeat(j0 + 1, h); c.j0 = wrap_repeat(j0, h); }
  else { c.j1 = wrap_clamp(j0 + 1, h); c.j0 = wrap_clamp(j0, h); }
  c.a = a; c.b = b;
  return c;
}
// ... and its four texel offsets in a single-layer image (8 x 4-texel tiles)
struct TapGeom { uint32_t o00, o10, o01, o11; float a, b; bool pair; };
FM_DEV TapGeom tap_geom(const TexCoord &c, int w) {
  TapGeom g;
  const int tiles_x = (w + TEX_TILE_W - 1) >> TEX_TILE_W_LOG2;
  g.o00 = tile_offset<TEX_TILE_W_LOG2, TEX_TILE_H_LOG2>(c.i0, c.j0, tiles_x);
  g.o01 = tile_offset<TEX_TILE_W_LOG2, TEX_TILE_H_LOG2>(c.i0, c.j1, tiles_x);
  g.o10 = tile_offset<TEX_TILE_W_LOG2, TEX_TILE_H_LOG2>(c.i1, c.j0, tiles_x);
  g.o11 = tile_offset<TEX_TILE_W_LOG2, TEX_TILE_H_LOG2>(c.i1, c.j1, tiles_x);
  // the two taps of a row are neighbours unless the column wraps or leaves the tile: one 8-byte load (dword-aligned)
  // instead of two 4-byte loads - half the lane-requests on the vector-memory pipeline, same texel values
  g.pair = FSPT_TAP2 && c.i1 == c.i0 + 1 && (TEX_TILE_W == 1 || (c.i0 & (TEX_TILE_W - 1)) != TEX_TILE_W - 1);
  g.a = c.a; g.b = c.b;
  return g;
}
FM_DEV Tap4 fetch_taps(const uint32_t *texels, const TapGeom &g) {
  Tap4 r;
  typedef uint32_t u2a __attribute__((ext_vector_type(2), aligned(4)));
  if (g.pair) {
    u2a q0 = *reinterpret_cast<const u2a *>(texels + g.o00), q1 = *reinterpret_cast<const u2a *>(texels + g.o01);
    r.t00 = q0.x; r.t10 = q0.y; r.t01 = q1.x; r.t11 = q1.y;
  } else {
    r.t00 = texels[g.o00]; r.t10 = texels[g.o10];
    r.t01 = texels[g.o01]; r.t11 = texels[g.o11];
  }
  r.a = g.a; r.b = g.b;
  return r;
}
FM_DEV Tap4 bilinear_taps(const uint32_t *texels, int w, int h, float s, float t, bool repeat_t) {
  return fetch_taps(texels, tap_geom(bilinear_coord(w, h, s, t, repeat_t), w));
}
FM_DEV float tap_channel(const Tap4 &tp, int ch) {
  float t00 = unorm8((tp.t00 >> (8 * ch)) & 255u), t10 = unorm8((tp.t10 >> (8 * ch)) & 255u);
  float t01 = unorm8((tp.t01 >> (8 * ch)) & 255u), t11 = unorm8((tp.t11 >> (8 * ch)) & 255u);
  return lerp_(lerp_(t00, t10, tp.a), lerp_(t01, t11, tp.a), tp.b);
}
// One atlas layer of a material texture set in SEPARATE form: its tiled image, or - a layer whose texels are all equal
// (TexturePacker fills a whole res x res layer for every flat colour once one image is in the atlas,
// texture_packer.js:36-42) is not stored - its one texel: lerp(x, x, a) = fma(a, 0, x) = x exactly, so four equal taps
// give the same bits as the fetch would.
FM_DEV Tap4 layer_taps(const DScene &S, const TapGeom &g, uint32_t base_tiles, uint32_t texel) {
  if (base_tiles == LAYER_CONST) {
    Tap4 r;
    r.t00 = r.t10 = r.t01 = r.t11 = texel;
    r.a = g.a; r.b = g.b;
    return r;
  }
  return fetch_taps(S.atlas + (size_t)base_tiles * (TEX_TILE_W * TEX_TILE_H), g);
}

// ---------------------------------------------------------------------------
// Materials: texture(texArray, vec3(uv, layer)) x 4 (tracer.fs:453-456)
// ---------------------------------------------------------------------------
FM_DEV V3 unorm8_rgb(uint32_t q) { return v3(unorm8(q & 255u), unorm8((q >> 8) & 255u), unorm8((q >> 16) & 255u)); }
FM_DEV V3 tap_rgb(const Tap4 &q) { return v3(tap_channel(q, 0), tap_channel(q, 1), tap_channel(q, 2)); }
// The layers of material texture set `set` (hit record word 42; fspt_device.hpp TexSet) at uv (s, t), the four layers'
// texels of ONE footprint: D texDiffuse, E texEmissive, R metallic and rough (not yet squared), N texNormal.  A layer
// that is not asked for issues no load; the outputs of the others are left alone.
template <bool D, bool E, bool R, bool N>
FM_DEV void material(const DScene &S, uint32_t set, float s, float t, V3 &texDiffuse, V3 &texEmissive, float &metallic,
                     float &rough, V3 &texNormal) {
  const uint4 *tset = S.tex_sets + (size_t)set * 3;
  const uint4 ts0 = tset[0], ts1 = tset[1];
  if (ts0.x == TEXSET_CONST) {
    // four flat colours (texture_packer.js:36-42; every material of a colours-only atlas): the four bilinear taps are
    // the same texel and lerp(x, x, a) = fma(a, 0, x) = x exactly, so the filter arithmetic is skipped (bit-identical)
    if (D) texDiffuse = unorm8_rgb(ts1.x);
    if (E) texEmissive = unorm8_rgb(ts1.y);
    if (R) { metallic = unorm8(ts1.z & 255u); rough = unorm8((ts1.z >> 8) & 255u); }
    if (N) texNormal = v3((unorm8(ts1.w & 255u) - 0.5f) * 2.0f, (unorm8((ts1.w >> 8) & 255u) - 0.5f) * 2.0f,
                          (unorm8((ts1.w >> 16) & 255u) - 0.0f) * 1.0f);
    return;
  }
  const TexCoord tc = bilinear_coord((int)S.atlas_res, (int)S.atlas_res, s, t, true);
  Tap4 qd, qe, qr, qn;
  if (ts0.x == TEXSET_QUAD) {
    // the four layers interleaved texel by texel (4 x 2-texel tiles of 16-byte texels): one 16-byte load per tap
    // brings all four layers, and the footprint lies in 1.9 lines instead of 4 x 1.4
    const uint4 *img = S.atlas4 + (size_t)ts0.y * 8u;
    const int tiles_x = ((int)S.atlas_res + 3) >> 2;
    const uint4 t00 = img[tile_offset<2, 1>(tc.i0, tc.j0, tiles_x)], t10 = img[tile_offset<2, 1>(tc.i1, tc.j0, tiles_x)];
    const uint4 t01 = img[tile_offset<2, 1>(tc.i0, tc.j1, tiles_x)], t11 = img[tile_offset<2, 1>(tc.i1, tc.j1, tiles_x)];
    qd = Tap4{t00.x, t10.x, t01.x, t11.x, tc.a, tc.b};
    qe = Tap4{t00.y, t10.y, t01.y, t11.y, tc.a, tc.b};
    qr = Tap4{t00.z, t10.z, t01.z, t11.z, tc.a, tc.b};
    qn = Tap4{t00.w, t10.w, t01.w, t11.w, tc.a, tc.b};
  } else {
    // separate single-layer images (a set with one image layer, or sets beyond the interleaving budget): all loads
    // of the image layers are issued before the first texel is decoded
    const uint4 ts2 = tset[2];
    const TapGeom tg = tap_geom(tc, (int)S.atlas_res);
    if (D) qd = layer_taps(S, tg, ts2.x, ts1.x);
    if (E) qe = layer_taps(S, tg, ts2.y, ts1.y);
    if (R) qr = layer_taps(S, tg, ts2.z, ts1.z);
    if (N) qn = layer_taps(S, tg, ts2.w, ts1.w);
  }
  if (D) texDiffuse = tap_rgb(qd);
  if (E) texEmissive = tap_rgb(qe);
  if (R) { metallic = tap_channel(qr, 0); rough = tap_channel(qr, 1); }
  if (N) texNormal = v3((tap_channel(qn, 0) - 0.5f) * 2.0f, (tap_channel(qn, 1) - 0.5f) * 2.0f, (tap_channel(qn, 2) - 0.0f) * 1.0f);
}

// The hit record of slot ti (192 B = 3 whole cache lines) and what shade_hit and first_hit_guides compute from it before
// shading: the hit point of ray (ro, rd) at tHit, its barycentric weights and its texture coordinates
struct HitGeom {
  V3 v1, e1, e2;                         // the triangle: its first vertex and two edges
  V3 n1, t1, b1, n2, t2, b2, n3, t3, b3; // the vertices' normal, tangent and bitangent
  uint32_t set;                          // the triangle's material texture set (hit record word 42)
  float ior, dielectric;
  V3 origin, w;                          // the hit point and its barycentric weights
  float tcx, tcy;                        // its texture coordinates
};
FM_DEV void hit_geom(const DScene &S, int ti, V3 ro, V3 rd, float tHit, HitGeom &g) {
  const float4 *hp = S.hitrec + (size_t)ti * HITREC_F4;
  const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3], h4 = hp[4], h5 = hp[5], h6 = hp[6], h7 = hp[7], h8 = hp[8],
               h9 = hp[9], h10 = hp[10], h11 = hp[11];
  g.v1 = v3(h0.x, h0.y, h0.z); g.e1 = v3(h0.w, h1.x, h1.y); g.e2 = v3(h1.z, h1.w, h2.x);
  g.n1 = v3(h2.y, h2.z, h2.w); g.t1 = v3(h3.x, h3.y, h3.z); g.b1 = v3(h3.w, h4.x, h4.y);
  g.n2 = v3(h4.z, h4.w, h5.x); g.t2 = v3(h5.y, h5.z, h5.w); g.b2 = v3(h6.x, h6.y, h6.z);
  g.n3 = v3(h6.w, h7.x, h7.y); g.t3 = v3(h7.z, h7.w, h8.x); g.b3 = v3(h8.y, h8.z, h8.w);
  g.set = __float_as_uint(h10.z); g.ior = h11.z; g.dielectric = h11.w;
  g.origin = vfma(rd, tHit, ro);
  // barycentricWeights (tracer.fs:339-353); v0 = e1, v1 = e2
  const V3 vv2 = g.origin - g.v1;
  const float d00 = dot(g.e1, g.e1), d01 = dot(g.e1, g.e2), d11 = dot(g.e2, g.e2);
  const float d20 = dot(vv2, g.e1), d21 = dot(vv2, g.e2);
  const float invDenom = 1.0f / fma_(d00, d11, -(d01 * d01));
  const float bv = fma_(d11, d20, -(d01 * d21)) * invDenom;
  const float bw = fma_(d00, d21, -(d01 * d20)) * invDenom;
  g.w = v3((1.0f - bv) - bw, bv, bw);
  g.tcx = fma_(g.w.z, h10.x, fma_(g.w.y, h9.z, g.w.x * h9.x));
  g.tcy = fma_(g.w.z, h10.y, fma_(g.w.y, h9.w, g.w.x * h9.y));
}
// macroNormal: texNormal in the interpolated tangent frame (tracer.fs:457-460), before the `inside` flip; baryNormal is
// the interpolated vertex normal
FM_DEV V3 macro_normal(const HitGeom &g, V3 texNormal, V3 &baryNormal) {
  baryNormal = bary3(g.w, g.n1, g.n2, g.n3);
  const V3 baryTangent = bary3(g.w, g.t1, g.t2, g.t3);
  const V3 baryBitangent = bary3(g.w, g.b1, g.b2, g.b3);
  return normalize(v3(fma_(texNormal.z, baryNormal.x, fma_(texNormal.y, baryBitangent.x, texNormal.x * baryTangent.x)),
                      fma_(texNormal.z, baryNormal.y, fma_(texNormal.y, baryBitangent.y, texNormal.x * baryTangent.y)),
                      fma_(texNormal.z, baryNormal.z, fma_(texNormal.y, baryBitangent.z, texNormal.x * baryTangent.z))));
}

// What shade_hit computes at hit (tHit, slot ti) of ray (ro, rd) before the `inside` flip: texDiffuse and macroNormal
// (tracer.fs:447-470), through shade_hit's own helpers; only the diffuse and normal layers are fetched.  `g`: the hit
// record they were computed from, for a caller that needs more of it (k_temporal_gbuffer: the hit point and its weights).
FM_DEV void first_hit_guides(const DScene &S, V3 ro, V3 rd, float tHit, int ti, V3 &albedo, V3 &normal, HitGeom &g) {
  hit_geom(S, ti, ro, rd, tHit, g);
  V3 texEmissive, texNormal, baryNormal;
  float metallic, rough;
  material<true, false, false, true>(S, g.set, g.tcx, g.tcy, albedo, texEmissive, metallic, rough, texNormal);
  normal = macro_normal(g, texNormal, baryNormal);
}
FM_DEV void first_hit_guides(const DScene &S, V3 ro, V3 rd, float tHit, int ti, V3 &albedo, V3 &normal) {
  HitGeom g;
  first_hit_guides(S, ro, rd, tHit, ti, albedo, normal, g);
}

} // namespace fspt
