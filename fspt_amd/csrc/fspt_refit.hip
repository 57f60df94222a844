// fspt_refit.hip - in-place geometry update (fspt_scene_update_geometry): new triangles for an unchanged tree.
// Everything the update recomputes is recomputed here, on the scene's own device arrays:
//   k_refit_check       is every input word finite?  (before the first write: a bad update leaves the scene as it was)
//   k_refit_records     leaf records (v1, e1, e2 component-major) and the geometry part of the 192-byte hit records
//   k_refit_leaf_boxes  a leaf's box = min / max over the vertices of the triangles it OWNS
//   k_refit_level       one tree level: a node's box = the union of its children's, written into its parent's record
//   k_refit_quads       the two-level nodes from the refitted 64-byte nodes + fspt_scene_create's usability test
// and what installs a NEW tree over the same triangles (fspt_scene_rebuild_geometry; rebuild_run below):
//   k_rebuild_slot_map  triangle -> the old leaf slot of the leaf that owns it (one writer per triangle)
//   k_rebuild_permute   the caller's tri / norm in the new leaf order (what refit_run is then fed); the pose of DESIGN 8.14, the skin of 8.16, the mesh of 8.24
//   k_rebuild_gather    per NEW leaf slot: the 192-byte hit record of its triangle's old slot (12 lanes x 16 bytes), slot_tri,
//                       and the "-1" padding of the leaf records
//   k_rebuild_nodes     the interior nodes' child references
// Schedule: one launch per tree level, deepest first (depth - 1 launches, no atomics on box words: a level only reads what
// the launches before it wrote, and two siblings write different words of their parent's record).  Min and max are taken on
// the order-preserving integer keys of fspt_bvh_build.hip (-0 < +0), which is the rule tests/refit_ref.py restates.
#include "fspt_internal.hpp"

#include <chrono>

namespace fspt {
namespace {

__device__ __forceinline__ uint32_t rkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rfloat(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float kmin(float a, float b) { const uint32_t x = rkey(a), y = rkey(b); return rfloat(x < y ? x : y); }
__device__ __forceinline__ float kmax(float a, float b) { const uint32_t x = rkey(a), y = rkey(b); return rfloat(x > y ? x : y); }

// box slot 2 r + side of the 64-byte node r (fspt_device.hpp): side 0 = f[0 1 | 2 3 | 8 9], side 1 = f[4 5 | 6 7 | 10 11]
__device__ __forceinline__ void box_store(float *nodes, uint32_t slot, const float lo[3], const float hi[3]) {
  float *f = nodes + (size_t)(slot >> 1) * 16;
  const uint32_t s = slot & 1u;
  f[4 * s + 0] = lo[0]; f[4 * s + 1] = lo[1]; f[4 * s + 2] = hi[0]; f[4 * s + 3] = hi[1];
  f[8 + 2 * s] = lo[2]; f[9 + 2 * s] = hi[2];
}

__global__ void k_refit_check(const uint32_t *__restrict__ a, size_t n, uint32_t *flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    bad = bad || (a[i] & 0x7f800000u) == 0x7f800000u; // inf or NaN
  if (bad) atomicOr(flag, 1u);
}

// one thread per leaf slot (record L, position k): triangle leaf_first[L] + k, when it exists (the "-1" padding stays)
__global__ void k_refit_records(const float *__restrict__ tri, const float *__restrict__ norm, const uint32_t *__restrict__ leaf_first,
                                uint32_t n_leaves, uint32_t LS, uint32_t T, float *__restrict__ leaves, float *__restrict__ hitrec) {
  const size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= (size_t)n_leaves * LS) return;
  const uint32_t L = (uint32_t)(sl / LS), k = (uint32_t)(sl % LS);
  const uint32_t ti = leaf_first[L] + k;
  if (ti >= T) return;
  const float *v = tri + (size_t)ti * 9;
  float o[9];
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  o[3] = v[3] - v[0]; o[4] = v[4] - v[1]; o[5] = v[5] - v[2]; // e1 = v2 - v1, as fspt_scene_create
  o[6] = v[6] - v[0]; o[7] = v[7] - v[1]; o[8] = v[8] - v[2]; // e2 = v3 - v1
  float *rec = leaves + (size_t)L * LS * 9;
  float *h = hitrec + sl * 48;
#pragma unroll
  for (int c = 0; c < 9; ++c) { rec[(size_t)c * LS + k] = o[c]; h[c] = o[c]; }
  if (norm) {
    const float *nn = norm + (size_t)ti * 27;
    for (int c = 0; c < 27; ++c) h[9 + c] = nn[c];
  }
}

__global__ void k_refit_leaf_boxes(const float *__restrict__ tri, const uint32_t *__restrict__ leaf_first, const uint32_t *__restrict__ leaf_cnt,
                                   const uint32_t *__restrict__ leaf_dst, uint32_t n_leaves, uint32_t T, uint32_t n_interior, float *__restrict__ nodes) {
  const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
  if (L >= n_leaves) return;
  const uint32_t first = leaf_first[L], dst = leaf_dst[L];
  uint32_t cnt = leaf_cnt[L];
  if (first >= T || (dst >> 1) >= n_interior) return; // (NO_DST: the root)
  if (cnt > T - first) cnt = T - first;
  if (cnt == 0) return; // a leaf that owns no triangle keeps its box
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t i = 0; i < cnt; ++i) {
    const float *v = tri + (size_t)(first + i) * 9;
    for (int c = 0; c < 9; ++c) {
      const uint32_t x = rkey(v[c]);
      lo[c % 3] = x < lo[c % 3] ? x : lo[c % 3];
      hi[c % 3] = x > hi[c % 3] ? x : hi[c % 3];
    }
  }
  const float flo[3] = {rfloat(lo[0]), rfloat(lo[1]), rfloat(lo[2])}, fhi[3] = {rfloat(hi[0]), rfloat(hi[1]), rfloat(hi[2])};
  box_store(nodes, dst, flo, fhi);
}

// lvl[2 j] = the node's own record, lvl[2 j + 1] = the box slot its box goes to
__global__ void k_refit_level(const uint32_t *__restrict__ lvl, uint32_t n, uint32_t n_interior, float *nodes) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = lvl[2 * j], dst = lvl[2 * j + 1];
  if (r >= n_interior || (dst >> 1) >= n_interior) return;
  const float *f = nodes + (size_t)r * 16;
  const float lo[3] = {kmin(f[0], f[4]), kmin(f[1], f[5]), kmin(f[8], f[10])};
  const float hi[3] = {kmax(f[2], f[6]), kmax(f[3], f[7]), kmax(f[9], f[11])};
  box_store(nodes, dst, lo, hi);
}

// one thread per (interior node r, child k): part k of r's two-level node (fspt_device.hpp), and fspt_scene_create's test
// of that part: the child's box is the union of the part's two boxes bit for bit, under the float comparison the traversal
// makes (two candidates that compare equal must be the same bits: -0 / +0), no NaN
__global__ void k_refit_quads(const float *__restrict__ nodes, uint32_t n_interior, float *__restrict__ quads, uint32_t *flag) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= 2u * n_interior) return;
  const uint32_t r = id >> 1, k = id & 1u;
  const float *n = nodes + (size_t)r * 16;
  const int *ni = (const int *)n;
  const int cref = ni[12 + k];
  const float cb[6] = {n[4 * k], n[4 * k + 1], n[8 + 2 * k], n[4 * k + 2], n[4 * k + 3], n[9 + 2 * k]}; // the child's box: min.xyz max.xyz
  float part[12];
  int pair[2] = {REF_SENTINEL, REF_SENTINEL};
  if (cref < 0 || (uint32_t)cref >= n_interior) { // a leaf: its own box, twice
    part[0] = part[4] = cb[0]; part[1] = part[5] = cb[1]; part[2] = part[6] = cb[3]; part[3] = part[7] = cb[4];
    part[8] = part[10] = cb[2]; part[9] = part[11] = cb[5];
  } else {
    const float *cn = nodes + (size_t)cref * 16;
    for (int c = 0; c < 12; ++c) part[c] = cn[c];
    pair[0] = ((const int *)cn)[12]; pair[1] = ((const int *)cn)[13];
  }
  float *q = quads + (size_t)r * 32 + 16 * k;
  for (int c = 0; c < 12; ++c) q[c] = part[c];
  int *qi = (int *)q;
  qi[12] = pair[0]; qi[13] = pair[1];
  qi[14] = k == 0 ? ni[12] : 0; qi[15] = k == 0 ? ni[13] : 0;
  const float lo[3][2] = {{part[0], part[4]}, {part[1], part[5]}, {part[8], part[10]}};
  const float hi[3][2] = {{part[2], part[6]}, {part[3], part[7]}, {part[9], part[11]}};
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const float mn = lo[a][0] < lo[a][1] ? lo[a][0] : lo[a][1], mx = hi[a][0] > hi[a][1] ? hi[a][0] : hi[a][1];
    if (lo[a][0] != lo[a][0] || lo[a][1] != lo[a][1] || hi[a][0] != hi[a][0] || hi[a][1] != hi[a][1]) ok = false;
    if (lo[a][0] == lo[a][1] && __float_as_uint(lo[a][0]) != __float_as_uint(lo[a][1])) ok = false;
    if (hi[a][0] == hi[a][1] && __float_as_uint(hi[a][0]) != __float_as_uint(hi[a][1])) ok = false;
    if (__float_as_uint(mn) != __float_as_uint(cb[a]) || __float_as_uint(mx) != __float_as_uint(cb[3 + a])) ok = false;
  }
  if (!ok) atomicOr(flag, 1u);
}

// ---- a new tree over the same triangles ----
// one thread per old leaf slot: the owning leaf's slot of triangle leaf_first[L] + k, k < leaf_cnt[L] (the owned ranges tile
// [0, T): every triangle has one writer)
__global__ void k_rebuild_slot_map(const uint32_t *__restrict__ leaf_first, const uint32_t *__restrict__ leaf_cnt, uint32_t n_leaves,
                                   uint32_t LS, uint32_t T, uint32_t *__restrict__ map) {
  const size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= (size_t)n_leaves * LS) return;
  const uint32_t L = (uint32_t)(sl / LS), k = (uint32_t)(sl % LS);
  const uint32_t ti = leaf_first[L] + k;
  if (k < leaf_cnt[L] && ti < T) map[ti] = (uint32_t)sl;
}

// dst[i * W + c] = src[order[i] * W + c]: one thread per output word
__global__ void k_rebuild_permute(const float *__restrict__ src, const uint32_t *__restrict__ order, uint32_t T, uint32_t W, float *__restrict__ dst) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (size_t)T * W) return;
  const uint32_t i = (uint32_t)(id / W), c = (uint32_t)(id % W);
  const uint32_t o = order[i];
  dst[id] = o < T ? src[(size_t)o * W + c] : 0.0f;
}

// 12 lanes per new leaf slot (L, k), one float4 of its hit record each: the record of the old slot of triangle
// order[leaf_first[L] + k] (refit_run then rewrites floats 0-8, and 9-35 when the caller gave normals); zeros, and the
// leaf record's "-1" triangle, where the slot lies beyond the last triangle
__global__ void k_rebuild_gather(const float4 *__restrict__ old_rec, size_t old_slots, const uint32_t *__restrict__ map,
                                 const uint32_t *__restrict__ order, const uint32_t *__restrict__ leaf_first, uint32_t n_leaves, uint32_t LS,
                                 uint32_t T, float4 *__restrict__ rec, uint32_t *__restrict__ slot_tri, float *__restrict__ leaves) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t sl = id / 12;
  const uint32_t j = (uint32_t)(id % 12);
  if (sl >= (size_t)n_leaves * LS) return;
  const uint32_t L = (uint32_t)(sl / LS), k = (uint32_t)(sl % LS);
  const uint32_t ti = leaf_first[L] + k;
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (ti < T) {
    const uint32_t o = order[ti];
    const uint32_t src = o < T ? map[o] : 0xFFFFFFFFu;
    if ((size_t)src < old_slots) v = old_rec[(size_t)src * 12 + j];
  } else if (j < 9) {
    leaves[(size_t)L * LS * 9 + (size_t)j * LS + k] = j < 3 ? -1.0f : 0.0f; // v1 = (-1, -1, -1), e1 = e2 = 0
  }
  rec[sl * 12 + j] = v;
  if (j == 0) slot_tri[sl] = ti;
}

// the motion-origin snapshot through the same map as k_rebuild_gather: 9 lanes per new leaf slot, one float each
__global__ void k_rebuild_gather_motion(const float *__restrict__ old_mo, size_t old_slots, const uint32_t *__restrict__ map,
                                        const uint32_t *__restrict__ order, const uint32_t *__restrict__ leaf_first, uint32_t n_leaves,
                                        uint32_t LS, uint32_t T, float *__restrict__ mo) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t sl = id / 9;
  const uint32_t j = (uint32_t)(id % 9);
  if (sl >= (size_t)n_leaves * LS) return;
  const uint32_t ti = leaf_first[(uint32_t)(sl / LS)] + (uint32_t)(sl % LS);
  float v = 0.0f;
  if (ti < T) {
    const uint32_t o = order[ti];
    const uint32_t src = o < T ? map[o] : 0xFFFFFFFFu;
    if ((size_t)src < old_slots) v = old_mo[(size_t)src * 9 + j];
  }
  mo[sl * 9 + j] = v;
}

// node r's words 12-15: its children's references (cref[2 r], cref[2 r + 1]), 0, 0; the boxes are the refit's
__global__ void k_rebuild_nodes(const int32_t *__restrict__ cref, uint32_t n_interior, int4 *__restrict__ nodes) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_interior) return;
  nodes[(size_t)r * 4 + 3] = make_int4(cref[2 * r], cref[2 * r + 1], 0, 0);
}

inline uint32_t blocks_for(size_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

} // namespace

int refit_prepare(fspt_scene *s) {
  fspt_scene::Refit &R = s->rf;
  if (R.d_flag) return FSPT_OK;
  const size_t nl = R.leaf_first.size();
  HIP_TRY(hipMalloc((void **)&R.d_leaf, (nl ? nl : 1) * 12));
  HIP_TRY(hipMalloc((void **)&R.d_lvl, (R.lvl_nodes.size() ? R.lvl_nodes.size() : 1) * 4));
  if (nl) {
    HIP_TRY(hipMemcpy(R.d_leaf, R.leaf_first.data(), nl * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.d_leaf + nl, R.leaf_cnt.data(), nl * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.d_leaf + 2 * nl, R.leaf_dst.data(), nl * 4, hipMemcpyHostToDevice));
  }
  if (!R.lvl_nodes.empty()) HIP_TRY(hipMemcpy(R.d_lvl, R.lvl_nodes.data(), R.lvl_nodes.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipEventCreate(&R.ev[0]));
  HIP_TRY(hipEventCreate(&R.ev[1]));
  HIP_TRY(hipMalloc((void **)&R.d_flag, 8)); // last: marks the copies complete
  return FSPT_OK;
}

void refit_release(fspt_scene *s) {
  fspt_scene::Refit &R = s->rf;
  hipFree(R.d_leaf); hipFree(R.d_lvl); hipFree(R.d_flag); hipFree(R.stage);
  for (hipEvent_t &e : R.ev) if (e) { hipEventDestroy(e); e = nullptr; }
  R.d_leaf = R.d_lvl = R.d_flag = nullptr; R.stage = nullptr;
}

// k_refit_check over tri and norm (may be NULL) on the NULL stream, behind the caller's memset of the flag, and the flag's
// read-back, which waits for it: *finite = 0 when a word is inf or NaN.  *launches grows by the kernels launched.
static int check_finite_launch(fspt_scene *s, const float *tri, const float *norm, int *finite, uint32_t *launches) {
  const uint32_t BS = 256;
  uint32_t *flag = s->rf.d_flag, got = 0u;
  const struct { const float *p; size_t n; } arrays[] = {{tri, (size_t)s->n_tris * 9}, {norm, (size_t)s->n_tris * 27}};
  for (const auto &a : arrays) {
    if (!a.p) continue;
    hipLaunchKernelGGL(k_refit_check, dim3(std::min<uint32_t>(blocks_for(a.n, BS), 4096u)), dim3(BS), 0, nullptr, (const uint32_t *)a.p, a.n, flag);
    ++*launches;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(&got, flag, 4, hipMemcpyDeviceToHost));
  *finite = got == 0u;
  return FSPT_OK;
}

int refit_run(fspt_scene *s, const float *tri, const float *norm, int *finite, int *quads_ok) {
  fspt_scene::Refit &R = s->rf;
  const uint32_t T = s->n_tris, LS = s->d.leaf_size, nl = (uint32_t)R.leaf_first.size(), NI = s->n_interior;
  const uint32_t BS = 256;
  hipStream_t st = nullptr;
  uint32_t quads_bad = 0u;
  HIP_TRY(hipMemsetAsync(R.d_flag, 0, 8, st));
  HIP_TRY(hipEventRecord(R.ev[0], st));
  uint32_t launches = 0;
  const int rc = check_finite_launch(s, tri, norm, finite, &launches);
  if (rc || !*finite) return rc;
  const uint32_t *lf = R.d_leaf, *lc = R.d_leaf + nl, *ld = R.d_leaf + 2 * (size_t)nl;
  if (nl) {
    hipLaunchKernelGGL(k_refit_records, dim3(blocks_for((size_t)nl * LS, BS)), dim3(BS), 0, st, tri, norm, lf, nl, LS, T, (float *)s->tris, (float *)s->shade);
    ++launches;
  }
  if (nl && NI) {
    hipLaunchKernelGGL(k_refit_leaf_boxes, dim3(blocks_for(nl, BS)), dim3(BS), 0, st, tri, lf, lc, ld, nl, T, NI, (float *)s->nodes);
    ++launches;
    for (size_t k = 0; k + 1 < R.lvl_off.size(); ++k) {
      const uint32_t a = R.lvl_off[k], n = R.lvl_off[k + 1] - a;
      if (!n) continue;
      hipLaunchKernelGGL(k_refit_level, dim3(blocks_for(n, BS)), dim3(BS), 0, st, R.d_lvl + 2 * (size_t)a, n, NI, (float *)s->nodes);
      ++launches;
    }
    if (s->quads) {
      hipLaunchKernelGGL(k_refit_quads, dim3(blocks_for(2 * (size_t)NI, BS)), dim3(BS), 0, st, (const float *)s->nodes, NI, (float *)s->quads, R.d_flag + 1);
      ++launches;
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(R.ev[1], st));
  HIP_TRY(hipMemcpy(&quads_bad, R.d_flag + 1, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipEventSynchronize(R.ev[1]));
  HIP_TRY(hipEventElapsedTime(&R.last_ms, R.ev[0], R.ev[1]));
  R.last_launches = launches;
  *quads_ok = s->quads && NI > 0 && quads_bad == 0u;
  return FSPT_OK;
}

int refit_check(fspt_scene *s, const float *tri, const float *norm, int *finite) {
  uint32_t launches = 0;
  HIP_TRY(hipMemsetAsync(s->rf.d_flag, 0, 4, nullptr));
  return check_finite_launch(s, tri, norm, finite, &launches);
}

namespace {
// the new tree until it is installed: freed unless `keep` is set
struct RebuildGuard {
  fspt_scene ns;
  BvhGpuDevice bt;
  uint32_t *d_map = nullptr;
  int32_t *d_cref = nullptr;
  Hold moved; // the deformers' arrays that follow the triangles, in the new leaf order
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool keep = false;
  ~RebuildGuard() {
    bvh_device_release(bt);
    hipFree(d_map); hipFree(d_cref);
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (keep) { moved.p.clear(); return; }
    geometry_free(ns);
    refit_release(&ns);
  }
};
int rebuild_alloc(void **p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); fspt_set_error("fspt_scene_rebuild_geometry: out of device memory (%zu bytes)", bytes); return FSPT_E_NOMEM; }
  HIP_TRY(e);
  return FSPT_OK;
}
#define REBUILD_ALLOC(p, bytes) do { int rc_a = rebuild_alloc((void **)(p), (bytes)); if (rc_a) return rc_a; } while (0)
} // namespace

int rebuild_run(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out, bool order_on_device) {
  const uint32_t T = s->n_tris, LS = s->d.leaf_size, BS = 256;
  RebuildGuard G;
  fspt_scene &ns = G.ns;
  // 1. the build kernels, from the caller's device array; the tree stays on the device
  int rc = bvh_build_device(tri, T, LS, G.bt);
  if (rc) return rc;
  // 2. topology only comes back: 16 bytes per node
  const uint32_t nn = G.bt.n_nodes;
  std::vector<int32_t> left(nn), right(nn);
  std::vector<uint32_t> lo(nn), cnt(nn);
  HIP_TRY(hipMemcpy(left.data(), G.bt.left, (size_t)nn * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(right.data(), G.bt.right, (size_t)nn * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(lo.data(), G.bt.lo, (size_t)nn * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cnt.data(), G.bt.cnt, (size_t)nn * 4, hipMemcpyDeviceToHost));
  // 3. the host's integer work: pre-order words as fspt_scene_create would be handed them, then its own numbering
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> pre;
  std::vector<uint32_t> gid, node_depth;
  uint32_t depth = 0;
  if (const char *what = bvh_preorder(left.data(), right.data(), lo.data(), cnt.data(), nn, T, LS, pre, gid, node_depth, &depth)) {
    fspt_set_error("fspt_scene_rebuild_geometry: inconsistent tree from the device (%s)", what);
    return FSPT_E_HIP;
  }
  std::vector<int32_t> words((size_t)nn * 3);
  for (uint32_t i = 0; i < nn; ++i) {
    const uint32_t g = gid[i];
    int32_t *w = &words[(size_t)i * 3];
    if (left[g] < 0) { w[0] = -1; w[1] = -1; w[2] = (int32_t)lo[g]; }
    else { w[0] = pre[(size_t)left[g]]; w[1] = pre[(size_t)right[g]]; w[2] = -1; }
  }
  TreeTopology tp;
  rc = tree_topology(words.data(), 12, nn, T, tp);
  if (rc) return rc;
  tree_refit_tables(words.data(), 12, nn, T, tp, ns.rf);
  const uint32_t NI = tp.n_interior, nl = (uint32_t)tp.leaf_first.size();
  std::vector<int32_t> cref(2 * (size_t)(NI ? NI : 1), 0);
  for (uint32_t i = 0; i < nn; ++i)
    if (words[(size_t)i * 3 + 2] <= -1) {
      cref[2 * (size_t)tp.ref[i]] = tp.ref[(size_t)words[(size_t)i * 3]];
      cref[2 * (size_t)tp.ref[i] + 1] = tp.ref[(size_t)words[(size_t)i * 3 + 1]];
    }
  const float host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!ns.rf.ok || !nl) { fspt_set_error("fspt_scene_rebuild_geometry: the built tree is not refittable"); return FSPT_E_HIP; }
  // 4. the new arrays - every allocation before the first change to `s`
  ns.device = s->device;
  ns.n_tris = T;
  ns.d.leaf_size = LS;
  ns.n_interior = NI;
  const size_t n_slots = (size_t)nl * LS, old_slots = s->n_slots;
  REBUILD_ALLOC(&ns.nodes, (size_t)(NI ? NI : 1) * 64);
  if (NI) REBUILD_ALLOC(&ns.quads, (size_t)NI * fspt::QUAD_F4 * 16u);
  REBUILD_ALLOC(&ns.tris, n_slots * 9 * 4);
  REBUILD_ALLOC(&ns.slot_tri, n_slots * 4);
  REBUILD_ALLOC(&ns.shade, n_slots * 192);
  if (s->motion) REBUILD_ALLOC(&ns.motion, n_slots * 36);
  REBUILD_ALLOC(&ns.rf.stage, (size_t)T * 36 * 4); // tri | norm in the new leaf order; the scene's staging array from now on
  REBUILD_ALLOC(&G.d_map, (size_t)T * 4);
  REBUILD_ALLOC(&G.d_cref, cref.size() * 4);
  // every deformer's arrays that follow their triangles (ids and float64 constants as words)
  std::vector<DeformArray> follow;
  for (fspt_scene::StageOwner who : {fspt_scene::STAGE_POSE, fspt_scene::STAGE_SKIN, fspt_scene::STAGE_MESH})
    for (const DeformArray &a : deform_arrays(s, who)) if (a.follows && *a.p) follow.push_back(a);
  for (uint32_t *&ids : s->matte_ids) if (ids) follow.push_back(DeformArray{(void **)&ids, T, {1u, 0u}, 1, true}); // the matte ids, a word per triangle
  for (const DeformArray &a : follow) {
    void *p = nullptr;
    REBUILD_ALLOC(&p, (size_t)T * (a.span[0] + a.span[1]) * 4 * a.slices);
    G.moved.p.push_back(p);
  }
  rc = refit_prepare(&ns);
  if (rc) return rc;
  HIP_TRY(hipEventCreate(&G.ev[0]));
  HIP_TRY(hipEventCreate(&G.ev[1]));
  // 5. the install kernels (NULL stream, like refit_run, which finishes the job: leaf records, hit floats 0-8 / 9-35, boxes, quads)
  hipStream_t st = nullptr;
  uint32_t launches = 0;
  HIP_TRY(hipMemcpy(G.d_cref, cref.data(), cref.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(G.ev[0], st));
  HIP_TRY(hipMemsetAsync(ns.nodes, 0, (size_t)(NI ? NI : 1) * 64, st));
  HIP_TRY(hipMemsetAsync(G.d_map, 0xFF, (size_t)T * 4, st));
  const uint32_t old_nl = (uint32_t)s->rf.leaf_first.size();
  hipLaunchKernelGGL(k_rebuild_slot_map, dim3(blocks_for((size_t)old_nl * LS, BS)), dim3(BS), 0, st, s->rf.d_leaf, s->rf.d_leaf + old_nl, old_nl, LS, T, G.d_map);
  float *ptri = ns.rf.stage, *pnorm = norm ? ns.rf.stage + (size_t)T * 9 : nullptr;
  hipLaunchKernelGGL(k_rebuild_permute, dim3(blocks_for((size_t)T * 9, BS)), dim3(BS), 0, st, tri, G.bt.order, T, 9u, ptri);
  launches += 2;
  if (norm) { hipLaunchKernelGGL(k_rebuild_permute, dim3(blocks_for((size_t)T * 27, BS)), dim3(BS), 0, st, norm, G.bt.order, T, 27u, pnorm); ++launches; }
  for (size_t i = 0; i < follow.size(); ++i) { // span by span, slice by slice
    const float *src = (const float *)*follow[i].p;
    float *dst = (float *)G.moved.p[i];
    size_t at = 0;
    for (size_t m = 0; m < follow[i].slices; ++m)
      for (const uint32_t W : follow[i].span) {
        if (!W) continue;
        hipLaunchKernelGGL(k_rebuild_permute, dim3(blocks_for((size_t)T * W, BS)), dim3(BS), 0, st, src + at, G.bt.order, T, W, dst + at);
        at += (size_t)T * W;
        ++launches;
      }
  }
  hipLaunchKernelGGL(k_rebuild_gather, dim3(blocks_for(n_slots * 12, BS)), dim3(BS), 0, st, (const float4 *)s->shade, old_slots, G.d_map, G.bt.order,
                     ns.rf.d_leaf, nl, LS, T, (float4 *)ns.shade, (uint32_t *)ns.slot_tri, (float *)ns.tris);
  ++launches;
  if (s->motion) { // slot s of the snapshot stays the triangle in slot s
    hipLaunchKernelGGL(k_rebuild_gather_motion, dim3(blocks_for(n_slots * 9, BS)), dim3(BS), 0, st, (const float *)s->motion, old_slots, G.d_map,
                       G.bt.order, ns.rf.d_leaf, nl, LS, T, (float *)ns.motion);
    ++launches;
  }
  if (NI) { hipLaunchKernelGGL(k_rebuild_nodes, dim3(blocks_for(NI, BS)), dim3(BS), 0, st, G.d_cref, NI, (int4 *)ns.nodes); ++launches; }
  HIP_TRY(hipGetLastError());
  int finite = 1, quads_ok = 0;
  rc = refit_run(&ns, ptri, pnorm, &finite, &quads_ok);
  if (rc) return rc;
  if (!finite) { fspt_set_error("fspt_scene_rebuild_geometry: a value of tri / norm is not finite (scene unchanged)"); return FSPT_E_INVALID; }
  HIP_TRY(hipEventRecord(G.ev[1], st));
  if (order_out) HIP_TRY(hipMemcpy(order_out, G.bt.order, (size_t)T * 4, order_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  float install_ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&install_ms, G.ev[0], G.ev[1]));
  // 6. everything has succeeded: swap, then free the old tree
  G.keep = true;
  geometry_free(*s);
  refit_release(s);
  for (size_t i = 0; i < follow.size(); ++i) { hipFree(*follow[i].p); *follow[i].p = G.moved.p[i]; }
  s->rf = std::move(ns.rf);
  stage_disown(s); // (rf.stage is a new array: what read_pose / _skin / _mesh would return is gone)
  s->motion = ns.motion; s->nodes = ns.nodes; s->quads = ns.quads; s->tris = ns.tris; s->slot_tri = ns.slot_tri; s->shade = ns.shade;
  geometry_publish(s, tp, nn, n_slots, quads_ok != 0);
  s->rb.build_ms = G.bt.kernel_ms;
  s->rb.install_ms = install_ms;
  s->rb.host_ms = host_ms;
  s->rb.launches = G.bt.launches + launches + s->rf.last_launches;
  s->rb.readbacks = G.bt.readbacks + 1;
  return FSPT_OK;
}

} // namespace fspt
