// fspt_bvh_build.hip - the opt-in GPU BVH builder behind fspt_builder_build_gpu.
//
// Top-down binned SAH, K = FSPT_BVH_BINS bins per axis, fully deterministic.  The algorithm is pinned (include/fspt.h,
// tests/bvh_binned_ref.py restates it in numpy and the GPU tests compare the two byte for byte):
//   * triangle box = componentwise min/max of its three float32 vertices, centroid c = (bmin + bmax) * 0.5f;
//   * a node owns a contiguous range of the current triangle order; box and centroid bounds are min/max over it;
//   * n <= leaf_size: leaf.  Otherwise, on each axis whose centroid extent e > 0, bin b = bin_of(c) (below) and try the
//     K-1 planes j: cost = SA(L)/SA(P)*nL + SA(R)/SA(P)*nR in float64 on the float32 boxes; valid if nL, nR > 0 and not
//     NaN; the first strict minimum over axis 0..2, j ascending wins;
//   * depth guard: take the SAH split only if d + 1 + lv(n_child) <= max_depth for both children, else (or when no
//     candidate is valid) split at floor(n/2) in the current order;
//   * stable partition (left keeps its order, then right).
// min/max run on order-preserving integer keys (-0 < +0, no NaN: the host refuses non-finite vertices), so every box is
// exact and independent of the order the reductions meet their inputs; counts are integers; partitions are scans.  No
// float is ever summed with an atomic.
//
// Schedule.  Nodes larger than SMALL are split level by level over all CUs: per level a plan kernel cuts the level's
// nodes into CHUNK-triangle chunks, then bounds / bins (LDS pre-aggregation per chunk, one partial per chunk) / split (one
// block per node reduces its chunks' bins and decides, then emits the children) / count / scatter (a stable segmented
// partition from per-chunk left counts) - 6 launches and one 4-byte readback per level.  Every node of at most SMALL
// triangles goes to the finisher: one block builds the node's whole subtree in LDS.  Node ids are handed out by an
// atomic counter, so their numbering varies from run to run; the host renumbers the tree in pre-order from its
// structure, which does not vary, and packs the reference-layout arrays (scene_build.cpp).
#include "fspt_internal.hpp"

#include <hip/hip_runtime.h>

#define FSPT_BVH_BINS 32

namespace fspt {
namespace {

constexpr int K = FSPT_BVH_BINS;
constexpr int BT = 256;            // threads per block of every kernel
constexpr int NW = BT / 64;
constexpr uint32_t CHUNK = 4096;   // triangles per chunk of a level-synchronous node
constexpr uint32_t SMALL = 1024;   // largest node the finisher takes (its triangles' records sit in LDS)
constexpr int BIN_W = 8;           // words per bin: count, min key xyz, max key xyz, pad
constexpr int NB = 3 * K * BIN_W;  // words of one bin set
constexpr int NC = 3 * K;          // candidate slots (j = 0 is never valid)
constexpr int STACK = 128;         // finisher's local stack (the guard bounds the depth by 63)

// triangle record: box keys (min xyz, max xyz), centroid (float bits), pad
struct Prim { uint32_t w[12]; };

__host__ __device__ inline uint32_t fkey(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float kfloat(uint32_t k) {
  uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// the bin of centroid coordinate c: min(K-1, (uint)((c - cmin) * (K / e))), with NaN -> 0 and +inf -> K-1
__device__ inline uint32_t bin_of(float c, float cmin, float scl) {
  const float f = (c - cmin) * scl;
  return f >= (float)K ? (uint32_t)(K - 1) : (f > 0.0f ? (uint32_t)f : 0u);
}
// ceil(log2(ceil(n / leaf_size))): the fewest levels below a node of n triangles
__device__ inline uint32_t levels_below(uint32_t n, uint32_t ls) {
  const uint32_t m = (uint32_t)(((uint64_t)n + ls - 1) / ls);
  return m <= 1 ? 0u : 32u - (uint32_t)__builtin_clz(m - 1);
}
__device__ inline double surface_area(const uint32_t lo[3], const uint32_t hi[3]) {
  const double xl = (double)kfloat(hi[0]) - (double)kfloat(lo[0]);
  const double yl = (double)kfloat(hi[1]) - (double)kfloat(lo[1]);
  const double zl = (double)kfloat(hi[2]) - (double)kfloat(lo[2]);
  return (xl * yl + xl * zl + yl * zl) * 2;
}

__device__ inline uint32_t wave_min(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// bounds accumulator: [0..2] box min, [3..5] box max, [6..8] centroid min, [9..11] centroid max (keys)
__device__ inline void bounds_init(uint32_t b[12]) {
  for (int k = 0; k < 3; ++k) { b[k] = 0xffffffffu; b[3 + k] = 0u; b[6 + k] = 0xffffffffu; b[9 + k] = 0u; }
}
__device__ inline void bounds_add_prim(uint32_t b[12], const uint32_t *w) {
  for (int k = 0; k < 3; ++k) {
    b[k] = min(b[k], w[k]);
    b[3 + k] = max(b[3 + k], w[3 + k]);
    const uint32_t ck = fkey(__uint_as_float(w[6 + k]));
    b[6 + k] = min(b[6 + k], ck);
    b[9 + k] = max(b[9 + k], ck);
  }
}
__device__ inline void bounds_add(uint32_t b[12], const uint32_t *o) {
  for (int k = 0; k < 3; ++k) {
    b[k] = min(b[k], o[k]); b[3 + k] = max(b[3 + k], o[3 + k]);
    b[6 + k] = min(b[6 + k], o[6 + k]); b[9 + k] = max(b[9 + k], o[9 + k]);
  }
}
// block-wide: every thread's b[] -> s_out[12]; every thread must call it
__device__ __forceinline__ void block_bounds(uint32_t b[12], uint32_t *s_out) {
  if (threadIdx.x < 12) s_out[threadIdx.x] = (threadIdx.x % 6) < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  for (int k = 0; k < 12; ++k) {
    const uint32_t v = (k % 6) < 3 ? wave_min(b[k]) : wave_max(b[k]);
    if ((threadIdx.x & 63) == 0) { if ((k % 6) < 3) atomicMin(&s_out[k], v); else atomicMax(&s_out[k], v); }
  }
  __syncthreads();
}

// exclusive prefix of a flag over the block (thread order); *total = number of set flags; every thread must call it
__device__ uint32_t block_scan_flag(bool f, uint32_t *s_w, uint32_t *total) {
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t pre = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int i = 0; i < NW; ++i) { if (i < w) off += s_w[i]; tot += s_w[i]; }
  __syncthreads();
  *total = tot;
  return off + pre;
}

// per-axis binning parameters from a node's centroid bounds
struct AxisBins { float cmin[3], scl[3]; bool ok[3]; };
__device__ inline AxisBins axis_bins(const uint32_t *nb) {
  AxisBins a;
  for (int k = 0; k < 3; ++k) {
    a.cmin[k] = kfloat(nb[6 + k]);
    const float e = kfloat(nb[9 + k]) - a.cmin[k];
    a.ok[k] = e > 0.0f;
    a.scl[k] = (float)K / e;
  }
  return a;
}
__device__ inline void bins_init(uint32_t *s_bins) {
  for (int i = threadIdx.x; i < NB; i += BT) {
    const int f = i % BIN_W;
    s_bins[i] = (f >= 1 && f <= 3) ? 0xffffffffu : 0u;
  }
}
__device__ inline void bins_add_prim(uint32_t *s_bins, const AxisBins &ab, const uint32_t *w) {
  for (int a = 0; a < 3; ++a) {
    if (!ab.ok[a]) continue;
    uint32_t *bn = s_bins + (a * K + (int)bin_of(__uint_as_float(w[6 + a]), ab.cmin[a], ab.scl[a])) * BIN_W;
    atomicAdd(&bn[0], 1u);
    for (int k = 0; k < 3; ++k) { atomicMin(&bn[1 + k], w[k]); atomicMax(&bn[4 + k], w[3 + k]); }
  }
}

// decision: axis (-1: median split), plane j, left count nl
struct Decision { int axis; uint32_t j, nl; };

// The split of a node of n triangles at depth d from its bin set (LDS) and bounds (nb: keys); every thread must call it.
__device__ Decision choose_split(const uint32_t *s_bins, const uint32_t *nb, uint32_t n, uint32_t d, uint32_t leaf_size,
                                 uint32_t max_depth, double *s_cost, uint32_t *s_nl, Decision *s_dec) {
  const AxisBins ab = axis_bins(nb);
  const int t = threadIdx.x;
  if (t < NC) {
    const int a = t / K, j = t % K;
    double cost = NAN;
    uint32_t nl = 0;
    if (j > 0 && ab.ok[a]) {
      uint32_t llo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, lhi[3] = {0, 0, 0};
      uint32_t rlo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, rhi[3] = {0, 0, 0};
      uint32_t nr = 0;
      for (int b = 0; b < K; ++b) {
        const uint32_t *bn = s_bins + (a * K + b) * BIN_W;
        if (b < j) {
          nl += bn[0];
          for (int k = 0; k < 3; ++k) { llo[k] = min(llo[k], bn[1 + k]); lhi[k] = max(lhi[k], bn[4 + k]); }
        } else {
          nr += bn[0];
          for (int k = 0; k < 3; ++k) { rlo[k] = min(rlo[k], bn[1 + k]); rhi[k] = max(rhi[k], bn[4 + k]); }
        }
      }
      if (nl > 0 && nr > 0) {
        const double sp = surface_area(nb, nb + 3);
        cost = surface_area(llo, lhi) / sp * (double)nl + surface_area(rlo, rhi) / sp * (double)nr;
      }
    }
    s_cost[t] = cost;
    s_nl[t] = nl;
  }
  __syncthreads();
  if (t == 0) {
    double best = INFINITY;
    int bi = -1;
    for (int c = 0; c < NC; ++c)
      if (!__builtin_isnan(s_cost[c]) && s_cost[c] < best) { best = s_cost[c]; bi = c; }
    Decision dec{-1, 0u, n / 2};
    if (bi >= 0) {
      const uint32_t nl = s_nl[bi], nr = n - nl;
      if (d + 1 + levels_below(nl, leaf_size) <= max_depth && d + 1 + levels_below(nr, leaf_size) <= max_depth)
        dec = Decision{bi / K, (uint32_t)(bi % K), nl};
    }
    *s_dec = dec;
  }
  __syncthreads();
  return *s_dec;
}

__device__ inline bool goes_left(const Decision &dec, const AxisBins &ab, float c_axis, uint32_t r) {
  if (dec.axis < 0) return r < dec.nl;
  return bin_of(c_axis, ab.cmin[dec.axis], ab.scl[dec.axis]) < dec.j;
}

struct Dev {
  const float *verts;
  Prim *prim;
  uint32_t *order[2];     // level-synchronous ping-pong
  uint32_t *order_final;  // written by the finisher
  uint32_t *node_lo, *node_n, *node_depth;
  int32_t *node_left, *node_right;
  uint32_t *node_box;     // 12 keys per node: box min/max, centroid min/max
  uint32_t *list[2];      // large nodes of the current / next level (node ids)
  uint32_t *fin;          // finisher nodes: id | parity << 31
  uint32_t *chunk_first;  // per large node of the level: its first chunk (M + 1)
  uint32_t *chunk_bounds; // 12 per chunk
  uint32_t *chunk_bins;   // NB per chunk
  uint32_t *chunk_left;   // per chunk
  Decision *dec;          // per large node of the level
  uint32_t *ctr;          // [0] nodes, [1] finisher nodes, [2] large nodes of the next level, [3] chunks of the level
  uint32_t n, leaf_size, max_depth;
};

__global__ void __launch_bounds__(BT) k_prep(Dev D) {
  const uint32_t i = blockIdx.x * BT + threadIdx.x;
  if (i == 0) {
    D.node_lo[0] = 0; D.node_n[0] = D.n; D.node_depth[0] = 0;
    D.ctr[0] = 1;
    if (D.n > SMALL) { D.list[0][0] = 0; D.ctr[1] = 0; } else { D.fin[0] = 0; D.ctr[1] = 1; }
    D.ctr[2] = 0; D.ctr[3] = 0;
  }
  if (i >= D.n) return;
  const float *v = D.verts + (size_t)i * 9;
  Prim p;
  for (int a = 0; a < 3; ++a) {
    const uint32_t k0 = fkey(v[a]), k1 = fkey(v[3 + a]), k2 = fkey(v[6 + a]);
    p.w[a] = min(min(k0, k1), k2);
    p.w[3 + a] = max(max(k0, k1), k2);
    const float c = (kfloat(p.w[a]) + kfloat(p.w[3 + a])) * 0.5f;
    p.w[6 + a] = __float_as_uint(c);
    p.w[9 + a] = 0;
  }
  D.prim[i] = p;
  D.order[0][i] = i;
}

// chunk offsets of the level's m_count nodes (one block)
__global__ void __launch_bounds__(BT) k_plan(Dev D, int cur, uint32_t m_count) {
  __shared__ uint32_t s_w[NW], s_carry;
  if (threadIdx.x == 0) { s_carry = 0; D.ctr[2] = 0; }
  __syncthreads();
  for (uint32_t base = 0; base < m_count; base += BT) {
    const uint32_t m = base + threadIdx.x;
    const uint32_t c = m < m_count ? (D.node_n[D.list[cur][m]] + CHUNK - 1) / CHUNK : 0;
    // inclusive scan over the block by waves
    uint32_t x = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)x, o);
      if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t off = s_carry;
    for (int i = 0; i < (int)(threadIdx.x >> 6); ++i) off += s_w[i];
    if (m < m_count) D.chunk_first[m] = off + x - c;
    __syncthreads();
    if (threadIdx.x == BT - 1) s_carry = off + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) { D.chunk_first[m_count] = s_carry; D.ctr[3] = s_carry; }
}

// the chunk's node (index into the level list) and its range [beg, end) relative to the node
struct ChunkRef { uint32_t m, id, lo, n, beg, end, first, last; };
__device__ bool chunk_ref(const Dev &D, int cur, uint32_t m_count, ChunkRef *s_ref) {
  if (threadIdx.x == 0) {
    ChunkRef r{};
    const uint32_t c = blockIdx.x;
    r.m = 0xffffffffu;
    if (c < D.chunk_first[m_count]) {
      uint32_t lo = 0, hi = m_count;  // largest m with chunk_first[m] <= c
      while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (D.chunk_first[mid] <= c) lo = mid; else hi = mid; }
      r.m = lo;
      r.id = D.list[cur][lo];
      r.lo = D.node_lo[r.id];
      r.n = D.node_n[r.id];
      r.first = D.chunk_first[lo];
      r.last = D.chunk_first[lo + 1];
      r.beg = (c - r.first) * CHUNK;
      r.end = min(r.n, r.beg + CHUNK);
    }
    *s_ref = r;
  }
  __syncthreads();
  return s_ref->m != 0xffffffffu;
}

__global__ void __launch_bounds__(BT) k_chunk_bounds(Dev D, int cur, uint32_t m_count) {
  __shared__ ChunkRef s_ref;
  __shared__ uint32_t s_b[12];
  if (!chunk_ref(D, cur, m_count, &s_ref)) return;
  const ChunkRef r = s_ref;
  uint32_t b[12];
  bounds_init(b);
  const uint32_t *ord = D.order[cur] + r.lo;
  for (uint32_t i = r.beg + threadIdx.x; i < r.end; i += BT) bounds_add_prim(b, D.prim[ord[i]].w);
  block_bounds(b, s_b);
  if (threadIdx.x < 12) D.chunk_bounds[(size_t)blockIdx.x * 12 + threadIdx.x] = s_b[threadIdx.x];
}

// node bounds (from its chunks' partials; the node's first chunk stores them), then this chunk's bins
__global__ void __launch_bounds__(BT) k_chunk_bin(Dev D, int cur, uint32_t m_count) {
  __shared__ ChunkRef s_ref;
  __shared__ uint32_t s_b[12];
  __shared__ uint32_t s_bins[NB];
  if (!chunk_ref(D, cur, m_count, &s_ref)) return;
  const ChunkRef r = s_ref;
  uint32_t b[12];
  bounds_init(b);
  for (uint32_t c = r.first + threadIdx.x; c < r.last; c += BT) bounds_add(b, D.chunk_bounds + (size_t)c * 12);
  block_bounds(b, s_b);
  if (blockIdx.x == r.first && threadIdx.x < 12) D.node_box[(size_t)r.id * 12 + threadIdx.x] = s_b[threadIdx.x];
  const AxisBins ab = axis_bins(s_b);
  bins_init(s_bins);
  __syncthreads();
  const uint32_t *ord = D.order[cur] + r.lo;
  for (uint32_t i = r.beg + threadIdx.x; i < r.end; i += BT) bins_add_prim(s_bins, ab, D.prim[ord[i]].w);
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += BT) D.chunk_bins[(size_t)blockIdx.x * NB + i] = s_bins[i];
}

// one block per large node: reduce the chunks' bins, decide, emit the two children
__global__ void __launch_bounds__(BT) k_node_split(Dev D, int cur, uint32_t m_count) {
  __shared__ uint32_t s_bins[NB], s_nb[12], s_nl[NC];
  __shared__ double s_cost[NC];
  __shared__ Decision s_dec;
  const uint32_t m = blockIdx.x;
  const uint32_t id = D.list[cur][m];
  const uint32_t c0 = D.chunk_first[m], c1 = D.chunk_first[m + 1];
  for (int i = threadIdx.x; i < NB; i += BT) {
    const int f = i % BIN_W;
    uint32_t v = (f >= 1 && f <= 3) ? 0xffffffffu : 0u;
    for (uint32_t c = c0; c < c1; ++c) {
      const uint32_t x = D.chunk_bins[(size_t)c * NB + i];
      v = f == 0 ? v + x : ((f <= 3) ? min(v, x) : max(v, x));
    }
    s_bins[i] = v;
  }
  if (threadIdx.x < 12) s_nb[threadIdx.x] = D.node_box[(size_t)id * 12 + threadIdx.x];
  __syncthreads();
  const uint32_t n = D.node_n[id], d = D.node_depth[id];
  const Decision dec = choose_split(s_bins, s_nb, n, d, D.leaf_size, D.max_depth, s_cost, s_nl, &s_dec);
  if (threadIdx.x == 0) {
    D.dec[m] = dec;
    const uint32_t ch = atomicAdd(&D.ctr[0], 2u);
    D.node_left[id] = (int32_t)ch;
    D.node_right[id] = (int32_t)(ch + 1);
    const uint32_t lo = D.node_lo[id];
    const uint32_t cn[2] = {dec.nl, n - dec.nl}, clo[2] = {lo, lo + dec.nl};
    for (int k = 0; k < 2; ++k) {
      const uint32_t c = ch + k;
      D.node_lo[c] = clo[k]; D.node_n[c] = cn[k]; D.node_depth[c] = d + 1;
      if (cn[k] > SMALL) D.list[cur ^ 1][atomicAdd(&D.ctr[2], 1u)] = c;
      else D.fin[atomicAdd(&D.ctr[1], 1u)] = c | ((uint32_t)(cur ^ 1) << 31);
    }
  }
}

__global__ void __launch_bounds__(BT) k_chunk_count(Dev D, int cur, uint32_t m_count) {
  __shared__ ChunkRef s_ref;
  __shared__ uint32_t s_w[NW];
  if (!chunk_ref(D, cur, m_count, &s_ref)) return;
  const ChunkRef r = s_ref;
  const Decision dec = D.dec[r.m];
  const AxisBins ab = axis_bins(D.node_box + (size_t)r.id * 12);
  const uint32_t *ord = D.order[cur] + r.lo;
  uint32_t cnt = 0;
  for (uint32_t i = r.beg + threadIdx.x; i < r.end; i += BT) {
    const float c = dec.axis >= 0 ? __uint_as_float(D.prim[ord[i]].w[6 + dec.axis]) : 0.0f;
    cnt += goes_left(dec, ab, c, i) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < NW; ++w) t += s_w[w];
    D.chunk_left[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(BT) k_chunk_scatter(Dev D, int cur, uint32_t m_count) {
  __shared__ ChunkRef s_ref;
  __shared__ uint32_t s_w[NW];
  if (!chunk_ref(D, cur, m_count, &s_ref)) return;
  const ChunkRef r = s_ref;
  const Decision dec = D.dec[r.m];
  const AxisBins ab = axis_bins(D.node_box + (size_t)r.id * 12);
  // left items of the node's earlier chunks
  uint32_t part = 0;
  for (uint32_t c = r.first + threadIdx.x; c < blockIdx.x; c += BT) part += D.chunk_left[c];
  for (int o = 32; o > 0; o >>= 1) part += (uint32_t)__shfl_xor((int)part, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = part;
  __syncthreads();
  uint32_t lbase = 0;
  for (int w = 0; w < NW; ++w) lbase += s_w[w];
  __syncthreads();
  const uint32_t *src = D.order[cur] + r.lo;
  uint32_t *dst = D.order[cur ^ 1] + r.lo;
  for (uint32_t base = r.beg; base < r.end; base += BT) {
    const uint32_t i = base + threadIdx.x;
    const bool in = i < r.end;
    const uint32_t t = in ? src[i] : 0u;
    const float c = (in && dec.axis >= 0) ? __uint_as_float(D.prim[t].w[6 + dec.axis]) : 0.0f;
    const bool left = in && goes_left(dec, ab, c, i);
    uint32_t tot;
    const uint32_t pre = block_scan_flag(left, s_w, &tot);
    if (in) {
      const uint32_t L = lbase + pre;  // left items before i in the node
      const uint32_t o = left ? L : dec.nl + (i - L);
      if (o < r.n) dst[o] = t;         // (always: the flags are the ones the split counted)
    }
    lbase += tot;
  }
}

// one block per node of at most SMALL triangles: its whole subtree, in LDS
__global__ void __launch_bounds__(BT) k_finish(Dev D) {
  __shared__ uint32_t s_rec[SMALL * 9];  // box keys + centroid bits per local triangle (odd stride: no bank conflicts)
  __shared__ uint32_t s_tid[SMALL];
  __shared__ uint16_t s_idx[SMALL], s_tmp[SMALL];
  __shared__ uint32_t s_bins[NB], s_nb[12], s_nl[NC], s_w[NW];
  __shared__ double s_cost[NC];
  __shared__ Decision s_dec;
  __shared__ uint32_t s_stack[STACK][4];  // local start, n, depth, node id
  __shared__ int s_sp;
  const uint32_t e = D.fin[blockIdx.x];
  const uint32_t root = e & 0x7fffffffu, par = e >> 31;
  const uint32_t glo = D.node_lo[root], gn = D.node_n[root];
  for (uint32_t i = threadIdx.x; i < gn; i += BT) {
    const uint32_t t = D.order[par][glo + i];
    s_tid[i] = t;
    const Prim p = D.prim[t];
    for (int k = 0; k < 9; ++k) s_rec[i * 9 + k] = p.w[k];
    s_idx[i] = (uint16_t)i;
  }
  if (threadIdx.x == 0) {
    s_stack[0][0] = 0; s_stack[0][1] = gn; s_stack[0][2] = D.node_depth[root]; s_stack[0][3] = root;
    s_sp = 1;
  }
  __syncthreads();
  while (s_sp > 0) {
    const int sp = s_sp;
    const uint32_t s = s_stack[sp - 1][0], n = s_stack[sp - 1][1], d = s_stack[sp - 1][2], id = s_stack[sp - 1][3];
    __syncthreads();
    if (threadIdx.x == 0) s_sp = sp - 1;
    uint32_t b[12];
    bounds_init(b);
    for (uint32_t i = threadIdx.x; i < n; i += BT) bounds_add_prim(b, &s_rec[s_idx[s + i] * 9]);
    block_bounds(b, s_nb);
    if (threadIdx.x < 12) D.node_box[(size_t)id * 12 + threadIdx.x] = s_nb[threadIdx.x];
    if (n <= D.leaf_size) {
      if (threadIdx.x == 0) { D.node_left[id] = -1; D.node_right[id] = -1; }
      __syncthreads();
      continue;
    }
    const AxisBins ab = axis_bins(s_nb);
    bins_init(s_bins);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += BT) bins_add_prim(s_bins, ab, &s_rec[s_idx[s + i] * 9]);
    __syncthreads();
    const Decision dec = choose_split(s_bins, s_nb, n, d, D.leaf_size, D.max_depth, s_cost, s_nl, &s_dec);
    uint32_t lbase = 0;
    for (uint32_t base = 0; base < n; base += BT) {
      const uint32_t i = base + threadIdx.x;
      const bool in = i < n;
      const uint16_t li = in ? s_idx[s + i] : (uint16_t)0;
      const float c = (in && dec.axis >= 0) ? __uint_as_float(s_rec[li * 9 + 6 + dec.axis]) : 0.0f;
      const bool left = in && goes_left(dec, ab, c, i);
      uint32_t tot;
      const uint32_t pre = block_scan_flag(left, s_w, &tot);
      if (in) {
        const uint32_t L = lbase + pre;
        const uint32_t o = left ? L : dec.nl + (i - L);
        if (o < n) s_tmp[s + o] = li;
      }
      lbase += tot;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += BT) s_idx[s + i] = s_tmp[s + i];
    if (threadIdx.x == 0) {
      const uint32_t ch = atomicAdd(&D.ctr[0], 2u);
      D.node_left[id] = (int32_t)ch;
      D.node_right[id] = (int32_t)(ch + 1);
      const uint32_t nr = n - dec.nl, sr = s + dec.nl;
      D.node_lo[ch] = glo + s; D.node_n[ch] = dec.nl; D.node_depth[ch] = d + 1;
      D.node_lo[ch + 1] = glo + sr; D.node_n[ch + 1] = nr; D.node_depth[ch + 1] = d + 1;
      // right below left: the left subtree is built first (the order does not matter for the result)
      const int q = s_sp;
      s_stack[q][0] = sr; s_stack[q][1] = nr; s_stack[q][2] = d + 1; s_stack[q][3] = ch + 1;
      s_stack[q + 1][0] = s; s_stack[q + 1][1] = dec.nl; s_stack[q + 1][2] = d + 1; s_stack[q + 1][3] = ch;
      s_sp = q + 2;
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < gn; i += BT) D.order_final[glo + i] = s_tid[s_idx[i]];
}

struct DevBufs {
  std::vector<void *> p;
  ~DevBufs() { for (void *q : p) (void)hipFree(q); }
  template <class T> hipError_t alloc(T **out, size_t count) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, count ? count * sizeof(T) : sizeof(T));
    if (e == hipSuccess) { p.push_back(q); *out = (T *)q; }
    return e;
  }
};
struct DeviceRestore {
  int prev = -1;
  ~DeviceRestore() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct StreamGuard {
  hipStream_t s = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~StreamGuard() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace

// The build proper, on the current device: vertices from host memory (uploaded on the build's stream) or already on the
// device; the tree stays in B's buffers (D) with *nn nodes.  One stream, waited for before it returns.
static int build_core(const float *verts_host, const float *verts_dev, uint32_t n, uint32_t leaf_size, DevBufs &B, StreamGuard &G, Dev &D,
                      uint32_t *nn_out, float *kernel_ms, uint32_t *launches_out, uint32_t *readbacks_out) {
  const uint32_t max_depth = bvh_max_depth();
  uint32_t launches = 0, readbacks = 0;
  const size_t N = n, NN = 2 * N;  // a binary tree with at most n leaves has fewer than 2n nodes
  const size_t max_large = N / SMALL + 1, max_chunks = (N + CHUNK - 1) / CHUNK + max_large;
  Prim *prim;
  float *verts_d = nullptr;
  if (verts_host) HIP_TRY(B.alloc(&verts_d, N * 9));
  HIP_TRY(B.alloc(&prim, N));
  HIP_TRY(B.alloc(&D.order[0], N));
  HIP_TRY(B.alloc(&D.order[1], N));
  HIP_TRY(B.alloc(&D.order_final, N));
  HIP_TRY(B.alloc(&D.node_lo, NN));
  HIP_TRY(B.alloc(&D.node_n, NN));
  HIP_TRY(B.alloc(&D.node_depth, NN));
  HIP_TRY(B.alloc(&D.node_left, NN));
  HIP_TRY(B.alloc(&D.node_right, NN));
  HIP_TRY(B.alloc(&D.node_box, NN * 12));
  HIP_TRY(B.alloc(&D.list[0], max_large));
  HIP_TRY(B.alloc(&D.list[1], max_large));
  HIP_TRY(B.alloc(&D.fin, N));
  HIP_TRY(B.alloc(&D.chunk_first, max_large + 1));
  HIP_TRY(B.alloc(&D.chunk_bounds, max_chunks * 12));
  HIP_TRY(B.alloc(&D.chunk_bins, max_chunks * NB));
  HIP_TRY(B.alloc(&D.chunk_left, max_chunks));
  HIP_TRY(B.alloc(&D.dec, max_large));
  HIP_TRY(B.alloc(&D.ctr, 4));
  D.verts = verts_host ? verts_d : verts_dev;
  D.prim = prim;
  D.n = n;
  D.leaf_size = leaf_size;
  D.max_depth = max_depth;
  HIP_TRY(hipStreamCreateWithFlags(&G.s, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&G.ev[0]));
  HIP_TRY(hipEventCreate(&G.ev[1]));
  if (verts_host) HIP_TRY(hipMemcpyAsync(verts_d, verts_host, N * 9 * sizeof(float), hipMemcpyHostToDevice, G.s));
  HIP_TRY(hipEventRecord(G.ev[0], G.s));
  hipLaunchKernelGGL(k_prep, dim3((unsigned)((N + BT - 1) / BT)), dim3(BT), 0, G.s, D);
  HIP_TRY(hipGetLastError());
  launches++;
  uint32_t m_count = n > SMALL ? 1u : 0u;
  int cur = 0;
  while (m_count > 0) {
    const unsigned grid_c = (unsigned)((N + CHUNK - 1) / CHUNK + m_count);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(BT), 0, G.s, D, cur, m_count);
    hipLaunchKernelGGL(k_chunk_bounds, dim3(grid_c), dim3(BT), 0, G.s, D, cur, m_count);
    hipLaunchKernelGGL(k_chunk_bin, dim3(grid_c), dim3(BT), 0, G.s, D, cur, m_count);
    hipLaunchKernelGGL(k_node_split, dim3(m_count), dim3(BT), 0, G.s, D, cur, m_count);
    hipLaunchKernelGGL(k_chunk_count, dim3(grid_c), dim3(BT), 0, G.s, D, cur, m_count);
    hipLaunchKernelGGL(k_chunk_scatter, dim3(grid_c), dim3(BT), 0, G.s, D, cur, m_count);
    HIP_TRY(hipGetLastError());
    launches += 6;
    HIP_TRY(hipMemcpyAsync(&m_count, D.ctr + 2, 4, hipMemcpyDeviceToHost, G.s));
    HIP_TRY(hipStreamSynchronize(G.s));
    readbacks++;
    if (m_count > max_large) { fspt_set_error("fspt_builder_build_gpu: level list overflow (%u)", m_count); return FSPT_E_HIP; }
    cur ^= 1;
  }
  uint32_t ctr[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(ctr, D.ctr, 8, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipStreamSynchronize(G.s));
  readbacks++;
  if (ctr[1] > 0) {
    hipLaunchKernelGGL(k_finish, dim3(ctr[1]), dim3(BT), 0, G.s, D);
    HIP_TRY(hipGetLastError());
    launches++;
  }
  HIP_TRY(hipEventRecord(G.ev[1], G.s));
  HIP_TRY(hipMemcpyAsync(ctr, D.ctr, 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipStreamSynchronize(G.s));
  readbacks++;
  const uint32_t nn = ctr[0];
  if (nn == 0 || nn >= NN) { fspt_set_error("fspt_builder_build_gpu: node count %u out of range", nn); return FSPT_E_HIP; }
  HIP_TRY(hipEventElapsedTime(kernel_ms, G.ev[0], G.ev[1]));
  *nn_out = nn;
  *launches_out = launches;
  *readbacks_out = readbacks;
  return FSPT_OK;
}

int bvh_build_gpu(const float *verts, uint32_t n, uint32_t leaf_size, int device, BvhGpuResult &out) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    fspt_set_error("fspt_builder_build_gpu: no HIP device available");
    return FSPT_E_NO_DEVICE;
  }
  if (device >= count) { fspt_set_error("fspt_builder_build_gpu: device %d out of range (have %d)", device, count); return FSPT_E_INVALID; }
  DeviceRestore restore;
  HIP_TRY(hipGetDevice(&restore.prev));
  HIP_TRY(hipSetDevice(device));
  out.launches = 0;
  out.readbacks = 0;
  DevBufs B;
  Dev D{};
  StreamGuard G;
  uint32_t nn = 0;
  const int rc = build_core(verts, nullptr, n, leaf_size, B, G, D, &nn, &out.kernel_ms, &out.launches, &out.readbacks);
  if (rc) return rc;
  const size_t N = n;
  out.left.resize(nn); out.right.resize(nn); out.lo.resize(nn); out.cnt.resize(nn); out.box_keys.resize((size_t)nn * 12);
  out.order.resize(N);
  HIP_TRY(hipMemcpyAsync(out.left.data(), D.node_left, nn * 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipMemcpyAsync(out.right.data(), D.node_right, nn * 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipMemcpyAsync(out.lo.data(), D.node_lo, nn * 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipMemcpyAsync(out.cnt.data(), D.node_n, nn * 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipMemcpyAsync(out.box_keys.data(), D.node_box, (size_t)nn * 48, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipMemcpyAsync(out.order.data(), D.order_final, N * 4, hipMemcpyDeviceToHost, G.s));
  HIP_TRY(hipStreamSynchronize(G.s));
  out.readbacks++;
  return FSPT_OK;
}

int bvh_build_device(const float *verts_dev, uint32_t n, uint32_t leaf_size, BvhGpuDevice &out) {
  DevBufs *B = new DevBufs();
  Dev D{};
  StreamGuard G;
  const int rc = build_core(nullptr, verts_dev, n, leaf_size, *B, G, D, &out.n_nodes, &out.kernel_ms, &out.launches, &out.readbacks);
  if (rc) { delete B; return rc; }
  out.order = D.order_final; out.lo = D.node_lo; out.cnt = D.node_n; out.left = D.node_left; out.right = D.node_right;
  out.bufs = B;
  return FSPT_OK;
}

void bvh_device_release(BvhGpuDevice &t) {
  delete (DevBufs *)t.bufs;
  t = BvhGpuDevice{};
}

const char *bvh_preorder(const int32_t *left, const int32_t *right, const uint32_t *lo, const uint32_t *cnt, size_t nn, size_t nt,
                         uint32_t leaf_size, std::vector<int32_t> &pre, std::vector<uint32_t> &gid, std::vector<uint32_t> &node_depth,
                         uint32_t *depth_out) {
  pre.assign(nn, -1);
  gid.clear(); node_depth.clear();
  gid.reserve(nn); node_depth.reserve(nn);
  std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};
  uint32_t depth = 0, next_lo = 0;
  while (!st.empty()) {
    const uint32_t g = st.back().first, d = st.back().second;
    st.pop_back();
    if (g >= nn || pre[g] >= 0) return "node visited twice or out of range";
    pre[g] = (int32_t)gid.size();
    gid.push_back(g);
    node_depth.push_back(d);
    depth = std::max(depth, d);
    const uint32_t hi = lo[g] + cnt[g];
    if (hi < lo[g] || hi > nt) return "range";
    if (left[g] < 0) {
      if (lo[g] != next_lo || cnt[g] == 0 || cnt[g] > leaf_size) return "leaf range";
      next_lo = hi;
    } else {
      if (right[g] < 0) return "children";
      st.push_back({(uint32_t)right[g], d + 1});
      st.push_back({(uint32_t)left[g], d + 1});
    }
  }
  if (gid.size() != nn || next_lo != nt) return "coverage";
  if (depth > bvh_max_depth()) return "depth";
  *depth_out = depth;
  return nullptr;
}

float bvh_key_float(uint32_t k) { return kfloat(k); }

uint32_t bvh_max_depth() {
  const size_t l = wf_max_stack_entries() < 64 ? wf_max_stack_entries() : 64;
  return (uint32_t)(l - 1);
}

}  // namespace fspt
