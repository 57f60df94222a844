// fspt_lights_build.hip - the emitter light table of a live scene, built on the GPU (opt-in:
// fspt_scene_set_light_builder).  The table's definition is integer, so no scan or summation order shows in its bits;
// tests/lighttable_ref.py restates it.
//   k_lt_tri_slot       per triangle its lowest leaf slot (atomicMin over slot_tri): kept until the tree's topology changes
//   k_lt_tri_slot_seal  the same array as k_light_weights takes it: slot 0 for a triangle in no leaf
//   k_lt_entries_count  per 256 triangles: how many have w > 0; the largest weight (an integer max of the bit patterns);
//                       a non-finite or negative weight raises the error word
//   k_lt_scan_counts    the exclusive scan of those counts (one workgroup); n
//   k_lt_entries        the entries in ascending triangle order: tris[], ent_slot[], their weights, the triangle-to-entry map
//   k_lt_quant          q_e = max(1, rint(w_e / w_max 2^32)) and T = sum q (integer atomics)
//   k_lt_classify       per 256 entries: the lights (n q < T), the sums of their deficits and of 2^40 - floor(prob 2^40), and the
//                       sum of the heavies' excesses (128-bit: n T passes 2^64 from a few 10^4 entries on)
//   k_lt_scan_sums      the exclusive scan of those four (one workgroup); the number of lights
//   k_lt_lists          the two lists in entry order with their inclusive sums D_j, X_k, C_j
//   k_lt_emit           per entry one binary search (a light: its heavy over X; a heavy: j*(k) and j*(k - 1) over D):
//                       (prob bits, alias) as one uint2, and light_p
//   k_lt_pick           light_pick per leaf slot through the triangle-to-entry map
// The one blocking read of a build is the 8 bytes {n, error}; buffers grow and never shrink.
#include "fspt_internal.hpp"
#include "fspt_encode_device.hpp"

namespace fspt {
namespace {

const uint32_t LT_BS = 256;
const uint32_t LT_NONE = 0xFFFFFFFFu;
const uint32_t LT_HEAVY = 0x80000000u;   // rank word: the entry is heavy; the low bits its index in its list
const uint32_t LT_MAX_ENTRIES = 1u << 23;
const uint32_t LT_E_WEIGHT = 1u, LT_E_ZERO = 2u, LT_E_MANY = 4u;
#define LT_2P32 4294967296.0
#define LT_2P40 1099511627776.0

struct U128 {
  uint64_t lo, hi;
  U128() = default;
  __host__ __device__ constexpr U128(uint64_t l) : lo(l), hi(0) {}
  __host__ __device__ constexpr U128(int l) : lo((uint64_t)l), hi(0) {}
  __host__ __device__ U128 &operator+=(const U128 &o) {
    const uint64_t l = lo + o.lo;
    hi += o.hi + (l < lo ? 1u : 0u);
    lo = l;
    return *this;
  }
};
__device__ __forceinline__ bool lt128(const U128 &a, const U128 &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ U128 sub128(const U128 &a, const U128 &b) {
  U128 r;
  r.lo = a.lo - b.lo;
  r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
  return r;
}

// what a build leaves on the device for the host (the first 8 bytes) and for its own later kernels
struct LtHeader {
  uint32_t n, err;
  uint32_t wmax_bits, n_light;
  unsigned long long T;
};

// ---------------------------------------------------------------------------
// triangles -> entries
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LT_BS) void k_lt_tri_slot(const uint32_t *slot_tri, uint32_t n_slots, uint32_t n_tris, uint32_t *first) {
  const uint32_t sl = blockIdx.x * LT_BS + threadIdx.x;
  if (sl >= n_slots) return;
  const uint32_t t = slot_tri[sl];
  if (t < n_tris) atomicMin(&first[t], sl);
}
__global__ __launch_bounds__(LT_BS) void k_lt_tri_slot_seal(const uint32_t *first, uint32_t n_tris, uint32_t *fed) {
  const uint32_t i = blockIdx.x * LT_BS + threadIdx.x;
  if (i < n_tris) fed[i] = first[i] == LT_NONE ? 0u : first[i];
}

// `first` NULL (the raw-weights hook): every weight is an entry, zeros included
__device__ __forceinline__ float lt_weight(const float *w, const uint32_t *first, uint32_t i) {
  return (first && first[i] == LT_NONE) ? 0.0f : w[i]; // (a triangle in no leaf: never hit)
}

__global__ __launch_bounds__(LT_BS) void k_lt_entries_count(float *w, const uint32_t *first, uint32_t n_tris, uint32_t *blk, LtHeader *hdr) {
  __shared__ uint32_t s_max;
  const uint32_t i = blockIdx.x * LT_BS + threadIdx.x;
  if (threadIdx.x == 0) s_max = 0u;
  __syncthreads();
  bool flag = false;
  if (i < n_tris) {
    const float wi = lt_weight(w, first, i);
    if (first) w[i] = wi;
    if (!(wi >= 0.0f) || !(wi <= 3.402823466e+38f)) atomicOr(&hdr->err, LT_E_WEIGHT);
    else {
      flag = !first || wi > 0.0f;
      if (wi > 0.0f) atomicMax(&s_max, __float_as_uint(wi));
    }
  }
  const uint32_t cnt = (uint32_t)__syncthreads_count(flag);
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = cnt;
    if (s_max) atomicMax(&hdr->wmax_bits, s_max);
  }
}

__global__ __launch_bounds__(LT_BS) void k_lt_scan_counts(uint32_t *blk, uint32_t nb, int raw, LtHeader *hdr) {
  __shared__ uint32_t s[LT_BS];
  uint32_t carry = 0u;
  for (uint32_t base = 0; base < nb; base += LT_BS) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? blk[i] : 0u;
    enc_scan256(s, v);
    if (i < nb) blk[i] = carry + s[threadIdx.x] - v;
    carry += s[LT_BS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hdr->n = carry;
    uint32_t err = 0u;
    if (carry > LT_MAX_ENTRIES) err |= LT_E_MANY;
    if (raw && hdr->wmax_bits == 0u) err |= LT_E_ZERO;
    if (err) atomicOr(&hdr->err, err);
  }
}

__global__ __launch_bounds__(LT_BS) void k_lt_entries(const float *w, const uint32_t *first, const uint32_t *fed, uint32_t n_tris, const uint32_t *blk,
                                                      uint32_t *tris, uint32_t *ent_slot, float *ent_w, uint32_t *tri_entry) {
  __shared__ uint32_t s[LT_BS];
  const uint32_t i = blockIdx.x * LT_BS + threadIdx.x;
  float wi = 0.0f;
  bool flag = false;
  if (i < n_tris) {
    wi = lt_weight(w, first, i);
    flag = (wi >= 0.0f) && (wi <= 3.402823466e+38f) && (!first || wi > 0.0f);
  }
  enc_scan256(s, flag ? 1u : 0u);
  if (i >= n_tris) return;
  const uint32_t e = blk[blockIdx.x] + s[threadIdx.x] - 1u; // (used when flag only)
  if (flag) {
    ent_w[e] = wi;
    if (tris) { tris[e] = i; ent_slot[e] = fed[i]; }
  }
  if (tri_entry) tri_entry[i] = flag ? e : LT_NONE;
}

// ---------------------------------------------------------------------------
// entries -> table
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LT_BS) void k_lt_quant(const float *ent_w, uint32_t n, unsigned long long *q, LtHeader *hdr) {
  __shared__ unsigned long long s_sum;
  const uint32_t e = blockIdx.x * LT_BS + threadIdx.x;
  if (threadIdx.x == 0) s_sum = 0ull;
  __syncthreads();
  if (e < n) {
    const float we = ent_w[e];
    unsigned long long qe = 0ull;
    if (we > 0.0f) {
      const double r = rint((double)we / (double)__uint_as_float(hdr->wmax_bits) * LT_2P32);
      qe = (unsigned long long)r;
      if (qe < 1ull) qe = 1ull;
    }
    q[e] = qe;
    atomicAdd(&s_sum, qe);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(&hdr->T, s_sum);
}

__device__ __forceinline__ float lt_prob(uint64_t r, uint64_t T) { return (float)((double)r / (double)T); }
__device__ __forceinline__ uint64_t lt_moved(float prob) { return (1ull << 40) - (uint64_t)floor((double)prob * LT_2P40); }

// an entry's part in the four sums: a light's deficit d and c = 2^40 - floor(prob 2^40), a heavy's excess x
struct LtClass { bool light; uint64_t d, x, c; };
__device__ __forceinline__ LtClass lt_class(const unsigned long long *q, uint32_t e, uint32_t n, uint64_t T) {
  LtClass k = {false, 0ull, 0ull, 0ull};
  if (e >= n) return k;
  const uint64_t m = (uint64_t)n * q[e];
  if (m < T) { k.light = true; k.d = T - m; k.c = lt_moved(lt_prob(m, T)); }
  else k.x = m - T;
  return k;
}

__global__ __launch_bounds__(LT_BS) void k_lt_classify(const unsigned long long *q, uint32_t n, const LtHeader *hdr, U128 *blk_d, U128 *blk_x,
                                                       unsigned long long *blk_c, uint32_t *blk_n) {
  __shared__ U128 sd[LT_BS], sx[LT_BS];
  __shared__ uint64_t sc[LT_BS];
  const LtClass k = lt_class(q, blockIdx.x * LT_BS + threadIdx.x, n, hdr->T);
  {
    U128 *const a[2] = {sd, sx};
    const U128 v[2] = {U128(k.d), U128(k.x)};
    enc_scan256(a, v);
  }
  enc_scan256(sc, k.c);
  const uint32_t cnt = (uint32_t)__syncthreads_count(k.light);
  if (threadIdx.x == 0) {
    blk_d[blockIdx.x] = sd[LT_BS - 1]; blk_x[blockIdx.x] = sx[LT_BS - 1];
    blk_c[blockIdx.x] = sc[LT_BS - 1]; blk_n[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(LT_BS) void k_lt_scan_sums(U128 *blk_d, U128 *blk_x, unsigned long long *blk_c, uint32_t *blk_n, uint32_t nb, LtHeader *hdr) {
  __shared__ U128 sd[LT_BS], sx[LT_BS];
  __shared__ uint64_t sc[LT_BS], sn[LT_BS];
  U128 cd(0), cx(0);
  uint64_t cc = 0ull, cn = 0ull;
  for (uint32_t base = 0; base < nb; base += LT_BS) {
    const uint32_t i = base + threadIdx.x;
    const bool in = i < nb;
    const U128 vd = in ? blk_d[i] : U128(0), vx = in ? blk_x[i] : U128(0);
    const uint64_t vc = in ? blk_c[i] : 0ull, vn = in ? (uint64_t)blk_n[i] : 0ull;
    {
      U128 *const a[2] = {sd, sx};
      const U128 v[2] = {vd, vx};
      enc_scan256(a, v);
    }
    {
      uint64_t *const a[2] = {sc, sn};
      const uint64_t v[2] = {vc, vn};
      enc_scan256(a, v);
    }
    if (in) {
      // exclusive: the inclusive sum of the blocks before this one
      U128 d = cd, x = cx;
      if (threadIdx.x) { d += sd[threadIdx.x - 1]; x += sx[threadIdx.x - 1]; }
      blk_d[i] = d; blk_x[i] = x;
      blk_c[i] = cc + sc[threadIdx.x] - vc;
      blk_n[i] = (uint32_t)(cn + sn[threadIdx.x] - vn);
    }
    cd += sd[LT_BS - 1]; cx += sx[LT_BS - 1]; cc += sc[LT_BS - 1]; cn += sn[LT_BS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) hdr->n_light = (uint32_t)cn;
}

// lights: DX[j], C[j], idx[j] for j < a; heavies: DX[a + k], idx[a + k]
__global__ __launch_bounds__(LT_BS) void k_lt_lists(const unsigned long long *q, uint32_t n, const LtHeader *hdr, const U128 *blk_d, const U128 *blk_x,
                                                    const unsigned long long *blk_c, const uint32_t *blk_n, U128 *DX, unsigned long long *C,
                                                    uint32_t *idx, uint32_t *rank) {
  __shared__ U128 sd[LT_BS], sx[LT_BS];
  __shared__ uint64_t sc[LT_BS], sn[LT_BS];
  const uint32_t e = blockIdx.x * LT_BS + threadIdx.x;
  const LtClass k = lt_class(q, e, n, hdr->T);
  {
    U128 *const a[2] = {sd, sx};
    const U128 v[2] = {U128(k.d), U128(k.x)};
    enc_scan256(a, v);
  }
  {
    uint64_t *const a[2] = {sc, sn};
    const uint64_t v[2] = {k.c, k.light ? 1ull : 0ull};
    enc_scan256(a, v);
  }
  if (e >= n) return;
  const uint32_t a = hdr->n_light;
  const uint32_t lights_before = blk_n[blockIdx.x] + (uint32_t)sn[threadIdx.x] - (k.light ? 1u : 0u);
  if (k.light) {
    const uint32_t j = lights_before;
    U128 d = blk_d[blockIdx.x];
    d += sd[threadIdx.x];
    DX[j] = d; C[j] = blk_c[blockIdx.x] + sc[threadIdx.x]; idx[j] = e; rank[e] = j;
  } else {
    const uint32_t kk = e - lights_before;
    U128 x = blk_x[blockIdx.x];
    x += sx[threadIdx.x];
    DX[a + kk] = x; idx[a + kk] = e; rank[e] = LT_HEAVY | kk;
  }
}

// heavy k of b, its inclusive excess X_k: j*(k) = #{j in 1..a : D_{j-1} < X_k}
__device__ __forceinline__ uint32_t lt_jstar(const U128 *D, uint32_t a, const U128 &X) {
  if (a == 0u || !(X.lo | X.hi)) return 0u; // (D_0 = 0 < X_k only when X_k > 0)
  uint32_t lo = 0u, hi = a - 1u;            // the number of D_1 .. D_{a-1} below X_k
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (lt128(D[mid], X)) lo = mid + 1u; else hi = mid;
  }
  return 1u + lo;
}
// the residual of heavy k: T + X_k - D_{j*(k)}, in (0, T]
__device__ __forceinline__ uint64_t lt_heavy_r(const U128 *D, uint32_t a, const U128 &X, uint64_t T, uint32_t &js) {
  js = lt_jstar(D, a, X);
  U128 v = X;
  v += U128(T);
  return sub128(v, js ? D[js - 1u] : U128(0)).lo;
}

__global__ __launch_bounds__(LT_BS) void k_lt_emit(const unsigned long long *q, uint32_t n, const LtHeader *hdr, const U128 *DX, const unsigned long long *C,
                                                   const uint32_t *idx, const uint32_t *rank, uint2 *ent, float *light_p) {
  const uint32_t e = blockIdx.x * LT_BS + threadIdx.x;
  if (e >= n) return;
  const uint64_t T = hdr->T;
  const uint32_t a = hdr->n_light, b = n - a;
  const U128 *D = DX, *X = DX + a;
  const uint32_t rk = rank[e];
  float prob;
  uint32_t alias;
  uint64_t S = 0ull;
  if (!(rk & LT_HEAVY)) {
    const U128 dp = rk ? D[rk - 1u] : U128(0);
    uint32_t lo = 0u, hi = b - 1u; // min{k : X_k > D_{j-1}}: it exists, the deficits from j on sum to more than nothing
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (lt128(dp, X[mid])) hi = mid; else lo = mid + 1u;
    }
    alias = idx[a + lo];
    prob = lt_prob((uint64_t)n * q[e], T);
  } else {
    const uint32_t k = rk & ~LT_HEAVY;
    uint32_t js, jp = 0u;
    const uint64_t r = lt_heavy_r(D, a, X[k], T, js);
    prob = lt_prob(r, T);
    alias = (r < T && k + 1u < b) ? idx[a + k + 1u] : e; // (r = T for the last heavy)
    S = (js ? C[js - 1u] : 0ull);
    if (k) {
      const uint64_t rp = lt_heavy_r(D, a, X[k - 1u], T, jp);
      S -= (jp ? C[jp - 1u] : 0ull);
      if (rp < T) S += lt_moved(lt_prob(rp, T));
    }
  }
  ent[e] = make_uint2(__float_as_uint(prob), alias);
  light_p[e] = (float)(((double)prob + (double)S * (1.0 / LT_2P40)) / (double)n);
}

__global__ __launch_bounds__(LT_BS) void k_lt_pick(const uint32_t *slot_tri, uint32_t n_slots, uint32_t n_tris, const uint32_t *tri_entry, const float *light_p,
                                                   float *pick) {
  const uint32_t sl = blockIdx.x * LT_BS + threadIdx.x;
  if (sl >= n_slots) return;
  const uint32_t t = slot_tri[sl];
  const uint32_t e = t < n_tris ? tri_entry[t] : LT_NONE;
  pick[sl] = e != LT_NONE ? light_p[e] : 0.0f;
}

inline dim3 grid_of(size_t n) { return dim3((uint32_t)((n + LT_BS - 1) / LT_BS)); }

int lt_fail(const char *fn, hipError_t e) {
  (void)hipGetLastError();
  fspt_set_error("%s: %s", fn, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
}

} // namespace

// The builder's device memory: it grows and never shrinks, so that a steady-state update allocates nothing.
struct LightsWork {
  struct Buf { void *p = nullptr; size_t cap = 0; };
  enum { HDR, FIRST, FED, W, TRI_ENTRY, TRIS, ENT_SLOT, ENT_W, BLK_N, Q, BLK_D, BLK_X, BLK_C, DXS, CS, IDX, RANK, ENT, LP, REC, REC_W, PICK, N_BUF };
  Buf b[N_BUF];
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t grow(int k, size_t bytes) {
    Buf &u = b[k];
    if (bytes <= u.cap) return hipSuccess;
    hipFree(u.p); u.p = nullptr; u.cap = 0;
    const hipError_t e = hipMalloc(&u.p, bytes);
    if (e == hipSuccess) u.cap = bytes; else u.p = nullptr;
    return e;
  }
  template <class T> T *at(int k) const { return (T *)b[k].p; }
  ~LightsWork() {
    for (Buf &u : b) hipFree(u.p);
    for (hipEvent_t &e : ev) if (e) hipEventDestroy(e);
  }
};

namespace {

// the per-triangle half on `st`: entries of w[0..n_tris) (first / fed NULL: the raw hook, zeros kept); leaves the header
hipError_t lt_entries_launch(LightsWork &K, float *w, const uint32_t *first, const uint32_t *fed, uint32_t n_tris, bool with_tris, hipStream_t st) {
  const uint32_t nb = (n_tris + LT_BS - 1) / LT_BS;
  hipError_t e = K.grow(LightsWork::HDR, sizeof(LtHeader));
  if (e == hipSuccess) e = K.grow(LightsWork::BLK_N, (size_t)(nb ? nb : 1u) * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::ENT_W, (size_t)n_tris * 4);
  if (e == hipSuccess && with_tris) e = K.grow(LightsWork::TRIS, (size_t)n_tris * 4);
  if (e == hipSuccess && with_tris) e = K.grow(LightsWork::ENT_SLOT, (size_t)n_tris * 4);
  if (e == hipSuccess && with_tris) e = K.grow(LightsWork::TRI_ENTRY, (size_t)n_tris * 4);
  if (e != hipSuccess) return e;
  LtHeader *hdr = K.at<LtHeader>(LightsWork::HDR);
  uint32_t *blk = K.at<uint32_t>(LightsWork::BLK_N);
  e = hipMemsetAsync(hdr, 0, sizeof(LtHeader), st);
  if (e != hipSuccess) return e;
  if (nb) hipLaunchKernelGGL(k_lt_entries_count, dim3(nb), dim3(LT_BS), 0, st, w, first, n_tris, blk, hdr);
  hipLaunchKernelGGL(k_lt_scan_counts, dim3(1), dim3(LT_BS), 0, st, blk, nb, first ? 0 : 1, hdr);
  if (nb)
    hipLaunchKernelGGL(k_lt_entries, dim3(nb), dim3(LT_BS), 0, st, (const float *)w, first, fed, n_tris, (const uint32_t *)blk,
                       with_tris ? K.at<uint32_t>(LightsWork::TRIS) : nullptr, with_tris ? K.at<uint32_t>(LightsWork::ENT_SLOT) : nullptr,
                       K.at<float>(LightsWork::ENT_W), with_tris ? K.at<uint32_t>(LightsWork::TRI_ENTRY) : nullptr);
  return hipGetLastError();
}

// the per-entry half on `st`: n in [1, 2^23] entries (ENT_W, the header's w_max) -> ENT (prob bits, alias) and LP
hipError_t lt_table_launch(LightsWork &K, uint32_t n, hipStream_t st) {
  const uint32_t nb = (n + LT_BS - 1) / LT_BS;
  hipError_t e = K.grow(LightsWork::Q, (size_t)n * 8);
  if (e == hipSuccess) e = K.grow(LightsWork::BLK_D, (size_t)nb * 16);
  if (e == hipSuccess) e = K.grow(LightsWork::BLK_X, (size_t)nb * 16);
  if (e == hipSuccess) e = K.grow(LightsWork::BLK_C, (size_t)nb * 8);
  if (e == hipSuccess) e = K.grow(LightsWork::BLK_N, (size_t)nb * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::DXS, (size_t)n * 16);
  if (e == hipSuccess) e = K.grow(LightsWork::CS, (size_t)n * 8);
  if (e == hipSuccess) e = K.grow(LightsWork::IDX, (size_t)n * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::RANK, (size_t)n * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::ENT, (size_t)n * 8);
  if (e == hipSuccess) e = K.grow(LightsWork::LP, (size_t)n * 4);
  if (e != hipSuccess) return e;
  LtHeader *hdr = K.at<LtHeader>(LightsWork::HDR);
  unsigned long long *q = K.at<unsigned long long>(LightsWork::Q), *blk_c = K.at<unsigned long long>(LightsWork::BLK_C), *C = K.at<unsigned long long>(LightsWork::CS);
  U128 *blk_d = K.at<U128>(LightsWork::BLK_D), *blk_x = K.at<U128>(LightsWork::BLK_X), *DX = K.at<U128>(LightsWork::DXS);
  uint32_t *blk_n = K.at<uint32_t>(LightsWork::BLK_N), *idx = K.at<uint32_t>(LightsWork::IDX), *rank = K.at<uint32_t>(LightsWork::RANK);
  hipLaunchKernelGGL(k_lt_quant, dim3(nb), dim3(LT_BS), 0, st, K.at<const float>(LightsWork::ENT_W), n, q, hdr);
  hipLaunchKernelGGL(k_lt_classify, dim3(nb), dim3(LT_BS), 0, st, (const unsigned long long *)q, n, (const LtHeader *)hdr, blk_d, blk_x, blk_c, blk_n);
  hipLaunchKernelGGL(k_lt_scan_sums, dim3(1), dim3(LT_BS), 0, st, blk_d, blk_x, blk_c, blk_n, nb, hdr);
  hipLaunchKernelGGL(k_lt_lists, dim3(nb), dim3(LT_BS), 0, st, (const unsigned long long *)q, n, (const LtHeader *)hdr, (const U128 *)blk_d, (const U128 *)blk_x,
                     (const unsigned long long *)blk_c, (const uint32_t *)blk_n, DX, C, idx, rank);
  hipLaunchKernelGGL(k_lt_emit, dim3(nb), dim3(LT_BS), 0, st, (const unsigned long long *)q, n, (const LtHeader *)hdr, (const U128 *)DX, (const unsigned long long *)C,
                     (const uint32_t *)idx, (const uint32_t *)rank, K.at<uint2>(LightsWork::ENT), K.at<float>(LightsWork::LP));
  return hipGetLastError();
}

// the one blocking read of a build: {n, error}; counted in *d2h
int lt_read_header(LightsWork &K, const char *fn, uint32_t &n, uint64_t *d2h) {
  uint32_t h[2] = {0u, 0u};
  const hipError_t e = hipMemcpy(h, K.b[LightsWork::HDR].p, sizeof h, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return lt_fail(fn, e);
  *d2h += sizeof h;
  n = h[0];
  if (h[1] & LT_E_WEIGHT) { fspt_set_error("%s: bad weights (a weight is negative or not finite)", fn); return FSPT_E_INVALID; }
  if (h[1] & LT_E_ZERO) { fspt_set_error("%s: bad weights (no weight is above 0)", fn); return FSPT_E_INVALID; }
  if (h[1] & LT_E_MANY) { fspt_set_error("%s: %u entries, the GPU builder takes at most %u", fn, n, LT_MAX_ENTRIES); return FSPT_E_INVALID; }
  return FSPT_OK;
}

} // namespace

int lights_build_gpu(fspt_scene *s) {
  const char *fn = "light table";
  if (!s->lg.work) s->lg.work = new LightsWork();
  LightsWork &K = *s->lg.work;
  hipStream_t st = nullptr;
  const uint32_t T = s->n_tris;
  const size_t slots_n = s->n_slots;
  const uint32_t *slot_tri = (const uint32_t *)s->slot_tri;
  hipError_t e = hipSuccess;
  for (hipEvent_t &ev : K.ev) if (!ev && e == hipSuccess) e = hipEventCreate(&ev);
  if (e == hipSuccess) e = K.grow(LightsWork::FIRST, (size_t)T * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::FED, (size_t)T * 4);
  if (e == hipSuccess) e = K.grow(LightsWork::W, (size_t)T * 4);
  s->lg.timed = false; // (ev[0] and ev[1] bracket a build again only when this one reaches its end)
  s->lg.bytes_d2h = s->lg.bytes_h2d = 0; // counted where a copy is issued: this build issues no upload
  if (e == hipSuccess) e = hipEventRecord(K.ev[0], st);
  if (e != hipSuccess) return lt_fail(fn, e);
  uint32_t *first = K.at<uint32_t>(LightsWork::FIRST), *fed = K.at<uint32_t>(LightsWork::FED);
  float *w = K.at<float>(LightsWork::W);
  if (!s->lg.topo_valid) {
    e = hipMemsetAsync(first, 0xFF, (size_t)T * 4, st);
    if (e != hipSuccess) return lt_fail(fn, e);
    if (slots_n) hipLaunchKernelGGL(k_lt_tri_slot, grid_of(slots_n), dim3(LT_BS), 0, st, slot_tri, (uint32_t)slots_n, T, first);
    hipLaunchKernelGGL(k_lt_tri_slot_seal, grid_of(T), dim3(LT_BS), 0, st, (const uint32_t *)first, T, fed);
    s->lg.topo_valid = true;
  }
  e = launch_light_weights(s->d, fed, T, w, nullptr, st);
  if (e == hipSuccess) e = lt_entries_launch(K, w, first, fed, T, true, st);
  if (e != hipSuccess) { s->lg.topo_valid = false; return lt_fail(fn, e); }
  uint32_t n = 0;
  const int rc = lt_read_header(K, fn, n, &s->lg.bytes_d2h);
  if (rc) return rc;
  if (n) {
    e = lt_table_launch(K, n, st);
    if (e == hipSuccess) e = K.grow(LightsWork::REC, (size_t)n * 64);
    if (e == hipSuccess) e = K.grow(LightsWork::REC_W, (size_t)n * 4);
    if (e == hipSuccess) e = K.grow(LightsWork::PICK, slots_n * 4);
    if (e == hipSuccess) e = launch_light_weights(s->d, K.at<uint32_t>(LightsWork::ENT_SLOT), n, K.at<float>(LightsWork::REC_W), K.at<float4>(LightsWork::REC), st);
    if (e == hipSuccess && slots_n) {
      hipLaunchKernelGGL(k_lt_pick, grid_of(slots_n), dim3(LT_BS), 0, st, slot_tri, (uint32_t)slots_n, T, K.at<const uint32_t>(LightsWork::TRI_ENTRY),
                         K.at<const float>(LightsWork::LP), K.at<float>(LightsWork::PICK));
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipEventRecord(K.ev[1], st);
  if (e == hipSuccess) e = hipEventSynchronize(K.ev[1]); // every later call sees the table, as after the host build
  if (e != hipSuccess) return lt_fail(fn, e);
  s->lg.timed = true;
  s->d.light_alias = n ? K.at<const uint2>(LightsWork::ENT) : nullptr;
  s->d.light_rec = n ? K.at<const float4>(LightsWork::REC) : nullptr;
  s->d.light_p = n ? K.at<const float>(LightsWork::LP) : nullptr;
  s->d.light_pick = n ? K.at<const float>(LightsWork::PICK) : nullptr;
  s->d.n_lights = n;
  s->lg.mirrors_valid = false;
  return FSPT_OK;
}

// the host copies fspt_scene_light_table and fspt_light_sample_eval read, from the GPU builder's arrays
int lights_mirrors_gpu(fspt_scene *s) {
  const char *fn = "light table";
  LightsWork &K = *s->lg.work;
  const uint32_t T = s->n_tris, n = s->d.n_lights;
  const size_t slots_n = s->n_slots;
  s->l_weight.assign(T, 0.0f); s->l_slot_tri.assign(slots_n, 0u); s->l_pick_h.assign(slots_n, 0.0f);
  s->l_tri.assign(n, 0u); s->l_prob.assign(n, 0.0f); s->l_alias_h.assign(n, 0u);
  std::vector<uint32_t> ent(2 * (size_t)n);
  hipError_t e = hipSuccess;
  if (T) e = hipMemcpy(s->l_weight.data(), K.b[LightsWork::W].p, (size_t)T * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && slots_n) e = hipMemcpy(s->l_slot_tri.data(), s->slot_tri, slots_n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && n) e = hipMemcpy(s->l_tri.data(), K.b[LightsWork::TRIS].p, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && n) e = hipMemcpy(ent.data(), K.b[LightsWork::ENT].p, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && n && slots_n) e = hipMemcpy(s->l_pick_h.data(), K.b[LightsWork::PICK].p, slots_n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return lt_fail(fn, e);
  for (uint32_t i = 0; i < n; ++i) { std::memcpy(&s->l_prob[i], &ent[2 * (size_t)i], 4); s->l_alias_h[i] = ent[2 * (size_t)i + 1]; }
  s->lg.mirrors_valid = true;
  return FSPT_OK;
}

int lights_build_ms(fspt_scene *s, float *ms) {
  *ms = 0.0f;
  if (!s->lg.work || !s->lg.timed) return FSPT_OK;
  const hipError_t e = hipEventElapsedTime(ms, s->lg.work->ev[0], s->lg.work->ev[1]);
  return e == hipSuccess ? FSPT_OK : lt_fail("fspt_scene_light_build_stats", e);
}

void lights_release(fspt_scene *s) {
  delete s->lg.work;
  s->lg.work = nullptr;
}

int light_alias_table_gpu_run(const float *weights, uint32_t n, float *prob, uint32_t *alias, float *light_p) {
  const char *fn = "fspt_light_alias_table_gpu";
  LightsWork K;
  hipStream_t st = nullptr;
  hipError_t e = K.grow(LightsWork::W, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpy(K.b[LightsWork::W].p, weights, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = lt_entries_launch(K, K.at<float>(LightsWork::W), nullptr, nullptr, n, false, st);
  if (e != hipSuccess) return lt_fail(fn, e);
  uint32_t m = 0;
  uint64_t d2h = 0;
  const int rc = lt_read_header(K, fn, m, &d2h);
  if (rc) return rc;
  e = lt_table_launch(K, n, st);
  std::vector<uint32_t> ent(2 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(ent.data(), K.b[LightsWork::ENT].p, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && light_p) e = hipMemcpy(light_p, K.b[LightsWork::LP].p, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return lt_fail(fn, e);
  for (uint32_t i = 0; i < n; ++i) {
    if (prob) std::memcpy(&prob[i], &ent[2 * (size_t)i], 4);
    if (alias) alias[i] = ent[2 * (size_t)i + 1];
  }
  return FSPT_OK;
}

} // namespace fspt
