// fspt_traverse.hpp - the BVH walk every kernel that traces a ray shares (fspt_kernels.hip: the two renderers, k_bvh_test;
// fspt_passes.hip: k_intersect, k_features, k_temporal_gbuffer): the box and triangle tests, the leaf code, trace_rays and
// trace_slice, the layout of a wave's deferred-child stack in LDS (lane_stack) and, next to it, what a launcher of such a
// kernel needs on the host (stack_bytes, allow_lds, launch).  Traversal order, pruning rule and the 4-triangle leaf
// over-read are the reference's (fspt_kernels.hip's header); arithmetic is "fspt-math" (fspt_math.hpp).
#pragma once
#include "fspt_device.hpp"
#include "fspt_math.hpp"

namespace fspt {
using namespace fm;

#define WAVE 64
#define BLOCK_THREADS 256
#define WAVES_PER_BLOCK (BLOCK_THREADS / WAVE)

// ---------------------------------------------------------------------------
// rayBoxIntersect (tracer.fs:317-326) for BOTH child boxes of a node; 1/dir hoisted (same value every call).
// Packed FP32: gfx950 issues v_pk_add_f32 / v_pk_mul_f32 (two IEEE binary32 operations per lane) at the rate of one
// scalar operation, and the traversal kernels are bound by VALU issue (profiles/r02: 0.85-0.98 of the issue rate), so
// the node stores the slab bounds in the pairs the arithmetic wants (fspt_device.hpp): the 12 subtractions and 12
// multiplications of a step are 6 + 6 instructions.  Same operations on the same operands as the scalar form:
// bit-identical results.
// ---------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4)));
FM_DEV f2 mk2(float a, float b) { return (f2){a, b}; }
FM_DEV f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
FM_DEV float slab(f2 txy1, f2 txy2, f2 tz) {
  float tMax = min_(min_(max_(txy1.x, txy2.x), max_(txy1.y, txy2.y)), max_(tz.x, tz.y));
  float tMin = max_(max_(min_(txy1.x, txy2.x), min_(txy1.y, txy2.y)), min_(tz.x, tz.y));
  return (tMax >= tMin && tMax > 0.0f) ? tMin : MAX_T;
}
FM_DEV void node_test(float4 n0, float4 n1, float4 n2, V3 o, V3 inv, float &tl, float &tr) {
  const f2 oxy = mk2(o.x, o.y), ixy = mk2(inv.x, inv.y), oz = mk2(o.z, o.z), iz = mk2(inv.z, inv.z);
  const f2 l1 = (mk2(n0.x, n0.y) - oxy) * ixy, l2 = (mk2(n0.z, n0.w) - oxy) * ixy; // left: (t1x, t1y), (t2x, t2y)
  const f2 r1 = (mk2(n1.x, n1.y) - oxy) * ixy, r2 = (mk2(n1.z, n1.w) - oxy) * ixy; // right
  const f2 lz = (mk2(n2.x, n2.y) - oz) * iz, rz = (mk2(n2.z, n2.w) - oz) * iz;     // (t1z, t2z) left, right
  tl = slab(l1, l2, lz);
  tr = slab(r1, r2, rz);
}
// The two child references of a node (f4[3].xy): ONE 8-byte load.  (Written as an int2 / int4 access the compiler
// widens it to 16 bytes.)
FM_DEV int2 node_refs(const float4 *n) {
  const long long rr = *reinterpret_cast<const long long *>(n + 3);
  return make_int2((int)(rr & 0xffffffffll), (int)(rr >> 32));
}

// One step of intersectScene at an interior node (tracer.fs:382-401) once the two entry distances are known: descend
// into the nearer child that is hit (the other one, if hit too, goes on the stack), or pop.  Returns which child the
// walk descends into: 0 left, 1 right, -1 neither (cur then holds the popped reference).
FM_DEV int node_decide(float tl, float tr, int refL, int refR, float t, int *stack, int &sp, int &cur) {
  const bool hl = tl < t, hr = tr < t;
  const bool swap = tl > tr; // tracer.fs:384: right first only when strictly nearer
  if (hl && hr) {
    stack[sp * WAVE] = swap ? refL : refR;
    sp++;
    cur = swap ? refR : refL;
    return swap ? 1 : 0;
  }
  if (hl) { cur = refL; return 0; }
  if (hr) { cur = refR; return 1; }
  if (sp > 0) { sp--; cur = stack[sp * WAVE]; }
  else cur = REF_SENTINEL;
  return -1;
}
// TWO steps on one two-level node (fspt_device.hpp "quad"; the eight loads are the caller's: global or LDS): the step at
// the node itself - its children's boxes are the unions of the stored grandchildren's, derived exactly - and, when the
// walk descends into a child that is an interior node, that child's step right away: result.t has not changed in
// between (no leaf was visited), so it is the test the one-level walk makes after its next fetch.  `steps` counts the
// reference's loop iterations exactly as the one-level walk does.
template <bool COUNT>
FM_DEV void quad_step(float4 a0, float4 a1, float4 a2, int4 ar, float4 b0, float4 b1, float4 b2, int2 br, V3 o, V3 inv, float t,
                      int *stack, int &sp, int &cur, uint32_t &steps) {
  const float4 n0 = make_float4(min_(a0.x, a1.x), min_(a0.y, a1.y), max_(a0.z, a1.z), max_(a0.w, a1.w)); // box(L) = box(LL) U box(LR)
  const float4 n1 = make_float4(min_(b0.x, b1.x), min_(b0.y, b1.y), max_(b0.z, b1.z), max_(b0.w, b1.w)); // box(R)
  const float4 n2 = make_float4(min_(a2.x, a2.z), max_(a2.y, a2.w), min_(b2.x, b2.z), max_(b2.y, b2.w));
  float tl, tr;
  node_test(n0, n1, n2, o, inv, tl, tr);
  const int side = node_decide(tl, tr, ar.z, ar.w, t, stack, sp, cur);
  if (side < 0 || cur < 0) return; // popped, or the child is a leaf (its record is the next fetch)
  if (COUNT) steps++;
  const bool right = side != 0;
  const float4 c0 = right ? b0 : a0, c1 = right ? b1 : a1, c2 = right ? b2 : a2;
  node_test(c0, c1, c2, o, inv, tl, tr);
  node_decide(tl, tr, right ? br.x : ar.x, right ? br.y : ar.y, t, stack, sp, cur);
}
FM_DEV void quad_load(const float4 *q, float4 &a0, float4 &a1, float4 &a2, int4 &ar, float4 &b0, float4 &b1, float4 &b2, int2 &br) {
  a0 = q[0]; a1 = q[1]; a2 = q[2];
  const float4 r = q[3];
  ar = make_int4(__float_as_int(r.x), __float_as_int(r.y), __float_as_int(r.z), __float_as_int(r.w));
  b0 = q[4]; b1 = q[5]; b2 = q[6];
  br = node_refs(q + 4);
}

// rayTriangleIntersect (tracer.fs:300-315) on a pre-edged triangle; the early
// returns become one predicate with the same NaN behaviour.
FM_DEV float ray_tri(V3 o, V3 d, V3 v1, V3 e1, V3 e2) {
  V3 p = cross(d, e2);
  float det = dot(e1, p);
  float invDet = 1.0f / det;
  V3 t = o - v1;
  float u = dot(t, p) * invDet;
  V3 q = cross(t, e1);
  float v = dot(d, q) * invDet;
  float dist = dot(e2, q) * invDet;
  bool miss = (abs_(det) < EPSILON) || (u < 0.0f) || (u > 1.0f) || (v < 0.0f) || (u + v > 1.0f) || !(dist > EPSILON);
  return miss ? MAX_T : dist;
}

// Two triangles at once (packed FP32, see node_test): component c of the pair is (tri_a.c, tri_b.c).  Every
// operation is ray_tri's, on the same operands, in the same order.
FM_DEV f2 ray_tri2(V3 o, V3 d, f2 v1x, f2 v1y, f2 v1z, f2 e1x, f2 e1y, f2 e1z, f2 e2x, f2 e2y, f2 e2z) {
  const f2 dx = mk2(d.x, d.x), dy = mk2(d.y, d.y), dz = mk2(d.z, d.z);
  const f2 px = fma2(dy, e2z, -(dz * e2y)), py = fma2(dz, e2x, -(dx * e2z)), pz = fma2(dx, e2y, -(dy * e2x)); // cross(d, e2)
  const f2 det = fma2(e1z, pz, fma2(e1y, py, e1x * px));
  const f2 invDet = mk2(1.0f / det.x, 1.0f / det.y);
  const f2 tx = mk2(o.x, o.x) - v1x, ty = mk2(o.y, o.y) - v1y, tz = mk2(o.z, o.z) - v1z;
  const f2 u = fma2(tz, pz, fma2(ty, py, tx * px)) * invDet;
  const f2 qx = fma2(ty, e1z, -(tz * e1y)), qy = fma2(tz, e1x, -(tx * e1z)), qz = fma2(tx, e1y, -(ty * e1x)); // cross(t, e1)
  const f2 v = fma2(dz, qz, fma2(dy, qy, dx * qx)) * invDet;
  const f2 dist = fma2(e2z, qz, fma2(e2y, qy, e2x * qx)) * invDet;
  const f2 uv = u + v;
  const bool m0 = (abs_(det.x) < EPSILON) || (u.x < 0.0f) || (u.x > 1.0f) || (v.x < 0.0f) || (uv.x > 1.0f) || !(dist.x > EPSILON);
  const bool m1 = (abs_(det.y) < EPSILON) || (u.y < 0.0f) || (u.y > 1.0f) || (v.y < 0.0f) || (uv.y > 1.0f) || !(dist.y > EPSILON);
  return mk2(m0 ? MAX_T : dist.x, m1 ? MAX_T : dist.y);
}

// ---------------------------------------------------------------------------
// processLeaf (tracer.fs:355-364): always LEAF_SIZE triangles from the leaf's first one, strict `<` update in
// triangle order.  Leaf record `leaf` (fspt_device.hpp): the LEAF_SIZE pre-edged triangles the reference would read,
// component-major - for LEAF_SIZE = 4 nine 16-byte loads whose halves are the operand pairs of ray_tri2.
// `hit` becomes the leaf SLOT (leaf * LEAF_SIZE + i): the index the hit records are stored under; slot_to_tri gives
// the reference's triangle index where one is reported (fspt_intersect).
// ---------------------------------------------------------------------------
FM_DEV void process_leaf(const float *__restrict__ leaves, uint32_t leaf_size, int leaf, V3 o, V3 d, float &t, int &hit) {
  if (leaf_size == 4) {
    const f4u *q = reinterpret_cast<const f4u *>(leaves) + (size_t)leaf * TRI_FLOATS;
    const f4u c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3], c4 = q[4], c5 = q[5], c6 = q[6], c7 = q[7], c8 = q[8];
    const f2 a = ray_tri2(o, d, c0.xy, c1.xy, c2.xy, c3.xy, c4.xy, c5.xy, c6.xy, c7.xy, c8.xy);
    const f2 b = ray_tri2(o, d, c0.zw, c1.zw, c2.zw, c3.zw, c4.zw, c5.zw, c6.zw, c7.zw, c8.zw);
    const int s0 = leaf * 4;
    if (a.x < t) { t = a.x; hit = s0; }
    if (a.y < t) { t = a.y; hit = s0 + 1; }
    if (b.x < t) { t = b.x; hit = s0 + 2; }
    if (b.y < t) { t = b.y; hit = s0 + 3; }
  } else {
    const float *a = leaves + (size_t)leaf * leaf_size * TRI_FLOATS;
    for (uint32_t i = 0; i < leaf_size; ++i) {
      float res = ray_tri(o, d, v3(a[i], a[leaf_size + i], a[2 * leaf_size + i]),
                          v3(a[3 * leaf_size + i], a[4 * leaf_size + i], a[5 * leaf_size + i]),
                          v3(a[6 * leaf_size + i], a[7 * leaf_size + i], a[8 * leaf_size + i]));
      if (res < t) { t = res; hit = leaf * (int)leaf_size + (int)i; }
    }
  }
}
// leaf slot -> the reference's triangle index (first triangle of the leaf + i, tracer.fs:360); -1 stays -1
FM_DEV int slot_to_tri(const DScene &S, int slot) { return slot < 0 ? -1 : (int)S.slot_tri[slot]; }

struct Counters {
  uint32_t samples, rays, steps, leaves, shades, envs;
};

// ---------------------------------------------------------------------------
// intersectScene (tracer.fs:366-404) for up to two rays sharing an origin:
// ray A (optional: the NEE shadow ray, tracer.fs:501) then ray B (primary or
// extension ray, tracer.fs:440,507).  `stack` points at this lane's column of
// the wave's LDS stack (entry k at stack[k*64]).
// ---------------------------------------------------------------------------
// ANYHIT: ray A stops at its first hit (only `shadow.index == -1` is consumed, tracer.fs:502).
// WIDE: walk the two-level nodes (S.quads, must be non-NULL): two steps per memory round trip, same walk.
// tA: ray A's t bound (an emitter shadow ray ends short of its light point; MAX_T otherwise)
template <bool COUNT, bool ANYHIT, bool WIDE = false>
FM_DEV void trace_rays(const DScene &S, int *stack, V3 o, bool hasA, V3 dA, V3 dB, int &hitA, float &tB, int &hitB,
                       Counters &cnt, float tA = MAX_T) {
  int slot = hasA ? 0 : 1;
  V3 d = hasA ? dA : dB;
  V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  float t = hasA ? tA : MAX_T;
  int hit = -1;
  int cur = S.root_ref;
  int sp = 0;
  hitA = -1;
  if (COUNT) cnt.rays++;
  const float4 *__restrict__ nodes = WIDE ? S.quads : S.nodes;
  const float *__restrict__ leaves = S.leaves;
  const uint32_t leaf_size = S.leaf_size;
  while (true) {
    // ---- interior nodes ----------------------------------------------------
    while (cur >= 0) {
      if (COUNT) cnt.steps++;
      if constexpr (WIDE) {
        float4 a0, a1, a2, b0, b1, b2; int4 ar; int2 br;
        quad_load(nodes + (size_t)cur * QUAD_F4, a0, a1, a2, ar, b0, b1, b2, br);
        quad_step<COUNT>(a0, a1, a2, ar, b0, b1, b2, br, o, inv, t, stack, sp, cur, cnt.steps);
        continue;
      }
      const float4 *n = nodes + (size_t)cur * NODE_F4;
      float4 n0 = n[0], n1 = n[1], n2 = n[2];
      const int2 n3 = node_refs(n);
      float tl, tr;
      node_test(n0, n1, n2, o, inv, tl, tr);
      bool hl = tl < t, hr = tr < t;
      bool swap = tl > tr; // tracer.fs:384: right first only when strictly nearer
      int nearRef = swap ? n3.y : n3.x;
      int farRef = swap ? n3.x : n3.y;
      if (hl && hr) {
        stack[sp * WAVE] = farRef;
        sp++;
        cur = nearRef;
      } else if (hl) {
        cur = n3.x;
      } else if (hr) {
        cur = n3.y;
      } else if (sp > 0) {
        sp--;
        cur = stack[sp * WAVE];
      } else {
        cur = REF_SENTINEL;
      }
    }
    if (cur == REF_SENTINEL) {
      if (slot == 0) { // shadow ray done: only its hit/miss is consumed (tracer.fs:502)
        hitA = hit;
        slot = 1;
        d = dB;
        inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        t = MAX_T;
        hit = -1;
        cur = S.root_ref;
        if (COUNT) cnt.rays++;
        continue;
      }
      break;
    }
    // ---- leaf: processLeaf (tracer.fs:355-364), always leaf_size triangles ----
    {
      if (COUNT) { cnt.steps++; cnt.leaves++; }
      int ts = ~cur;
      process_leaf(leaves, leaf_size, ts, o, d, t, hit);
      if (sp > 0) { sp--; cur = stack[sp * WAVE]; }
      else cur = REF_SENTINEL;
      if (ANYHIT && slot == 0 && hit != -1) cur = REF_SENTINEL;
    }
  }
  tB = t;
  hitB = hit;
}

// intersectScene (tracer.fs:366-404) for ONE ray per lane, in SLICES: the traversal state (node reference, stack depth,
// t, hit; the stack itself is the lane's LDS column) is the caller's and survives the call.  A lane walks on from
// where it stands until its ray is finished (cur == REF_SENTINEL) or it has done `budget` loop iterations in this call;
// the call returns when no lane has anything left to do within its budget.  `anyhit`: stop at the first hit (NEE
// shadow rays, tracer.fs:502).  Same node sequence and arithmetic as trace_rays, whatever the slicing.
// WIDE: 0 the 64-byte nodes, 1 the two-level nodes, 2 the caller says per call (`wide_now`, wave-uniform): the traversal
// state - node reference, stack entries - means the same in both walks (the two arrays are indexed alike), so a ray can
// change form between any two steps.
template <bool COUNT, int WIDE = 0>
FM_DEV void trace_slice(const DScene &S, int *stack, V3 o, V3 d, V3 inv /* 1 / d */, bool anyhit, int &cur, int &sp, float &t, int &hit,
                        uint32_t budget, uint32_t &n /* loop iterations (memory round trips) this lane has used of the budget */, Counters &cnt,
                        bool wide_now = false) {
  const float4 *__restrict__ nodes = S.nodes;
  const float4 *__restrict__ quads = S.quads;
  const float *__restrict__ leaves = S.leaves;
  const uint32_t leaf_size = S.leaf_size;
  while (cur != REF_SENTINEL && n < budget) {
    while (cur >= 0 && n < budget) {
      if (COUNT) cnt.steps++;
      ++n;
      if (WIDE == 1 || (WIDE == 2 && wide_now)) {
        float4 a0, a1, a2, b0, b1, b2; int4 ar; int2 br;
        quad_load(quads + (size_t)cur * QUAD_F4, a0, a1, a2, ar, b0, b1, b2, br);
        quad_step<COUNT>(a0, a1, a2, ar, b0, b1, b2, br, o, inv, t, stack, sp, cur, cnt.steps);
        continue;
      }
      const float4 *nd = nodes + (size_t)cur * NODE_F4;
      float4 n0 = nd[0], n1 = nd[1], n2 = nd[2];
      const int2 n3 = node_refs(nd);
      float tl, tr;
      node_test(n0, n1, n2, o, inv, tl, tr);
      bool hl = tl < t, hr = tr < t;
      bool swap = tl > tr; // tracer.fs:384: right first only when strictly nearer
      int nearRef = swap ? n3.y : n3.x;
      int farRef = swap ? n3.x : n3.y;
      if (hl && hr) {
        stack[sp * WAVE] = farRef;
        sp++;
        cur = nearRef;
      } else if (hl) {
        cur = n3.x;
      } else if (hr) {
        cur = n3.y;
      } else if (sp > 0) {
        sp--;
        cur = stack[sp * WAVE];
      } else {
        cur = REF_SENTINEL;
      }
    }
    if (cur >= 0 || cur == REF_SENTINEL) break; // out of budget on an interior node / finished
    if (COUNT) { cnt.steps++; cnt.leaves++; }
    ++n;
    process_leaf(leaves, leaf_size, ~cur, o, d, t, hit);
    if (sp > 0) { sp--; cur = stack[sp * WAVE]; }
    else cur = REF_SENTINEL;
    if (anyhit && hit != -1) cur = REF_SENTINEL;
  }
}

// ---------------------------------------------------------------------------
// The wave's stack in dynamic LDS: S.stack_n entries per lane, entry k of a lane at stack[k * WAVE], the waves of a block
// one after the other.  lane_stack: the column of thread `tid` of the block (its `stack` argument above).
// ---------------------------------------------------------------------------
FM_DEV int *lane_stack(int *lds_stack, uint32_t tid, uint32_t stack_n) {
  const int lane = (int)(tid & (WAVE - 1));
  const int wave = (int)(tid / WAVE);
  return lds_stack + (size_t)wave * stack_n * WAVE + lane;
}
// ... and its size for a BLOCK_THREADS block.  A launch with more than 48 KB of dynamic LDS (trees deeper than 47 levels
// here) makes the per-kernel opt-in first; gfx950 has 160 KB per CU.
static size_t stack_bytes(const DScene &S) { return (size_t)WAVES_PER_BLOCK * S.stack_n * WAVE * sizeof(int); }
template <class K>
static hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 48u * 1024u) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// `kernel` with `lds` bytes of dynamic LDS; the caller collects the launch's error with hipGetLastError
template <class K, class P>
static hipError_t launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const P &p) {
  const hipError_t e = allow_lds(kernel, lds);
  if (e == hipSuccess) hipLaunchKernelGGL(kernel, grid, block, lds, stream, p);
  return e;
}

} // namespace fspt
