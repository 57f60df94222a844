// fspt_refit.hip - in-place geometry update (fspt_scene_update_geometry): new triangles for an unchanged tree.
// Everything the update recomputes is recomputed here, on the scene's own device arrays:
//   k_refit_check       is every input word finite?  (before the first write: a bad update leaves the scene as it was)
//   k_refit_records     leaf records (v1, e1, e2 component-major) and the geometry part of the 192-byte hit records
//   k_refit_leaf_boxes  a leaf's box = min / max over the vertices of the triangles it OWNS
//   k_refit_level       one tree level: a node's box = the union of its children's, written into its parent's record
//   k_refit_quads       the two-level nodes from the refitted 64-byte nodes + fspt_scene_create's usability test
// Schedule: one launch per tree level, deepest first (depth - 1 launches, no atomics on box words: a level only reads what
// the launches before it wrote, and two siblings write different words of their parent's record).  Min and max are taken on
// the order-preserving integer keys of fspt_bvh_build.hip (-0 < +0), which is the rule tests/refit_ref.py restates.
#include "fspt_internal.hpp"

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

int refit_run(fspt_scene *s, const float *tri, const float *norm, int *finite, int *quads_ok) {
  fspt_scene::Refit &R = s->rf;
  const uint32_t T = s->n_tris, LS = s->d.leaf_size, nl = (uint32_t)R.leaf_first.size(), NI = s->n_interior;
  const uint32_t BS = 256;
  hipStream_t st = nullptr;
  uint32_t flags[2] = {0u, 0u};
  HIP_TRY(hipMemsetAsync(R.d_flag, 0, 8, st));
  HIP_TRY(hipEventRecord(R.ev[0], st));
  uint32_t launches = 0;
  {
    const size_t n = (size_t)T * 9;
    hipLaunchKernelGGL(k_refit_check, dim3(std::min<uint32_t>(blocks_for(n, BS), 4096u)), dim3(BS), 0, st, (const uint32_t *)tri, n, R.d_flag);
    ++launches;
    if (norm) {
      const size_t m = (size_t)T * 27;
      hipLaunchKernelGGL(k_refit_check, dim3(std::min<uint32_t>(blocks_for(m, BS), 4096u)), dim3(BS), 0, st, (const uint32_t *)norm, m, R.d_flag);
      ++launches;
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(flags, R.d_flag, 4, hipMemcpyDeviceToHost)); // (waits for the check)
  *finite = flags[0] == 0u;
  if (flags[0]) return FSPT_OK;
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
  HIP_TRY(hipMemcpy(flags + 1, R.d_flag + 1, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipEventSynchronize(R.ev[1]));
  HIP_TRY(hipEventElapsedTime(&R.last_ms, R.ev[0], R.ev[1]));
  R.last_launches = launches;
  *quads_ok = s->quads && NI > 0 && flags[1] == 0u;
  return FSPT_OK;
}

} // namespace fspt
