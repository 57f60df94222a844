// fspt_appearance.hip - in-place appearance update (fspt_scene_update_materials / _environment): new materials,
// uvs, atlas texels and environment for an unchanged tree.  The layouts fspt_scene_create makes with host loops are made
// here on the GPU, from the raw arrays as the caller holds them:
//   k_ap_layer_const  per atlas layer: does every texel equal texel 0?  (one flag + the first texel per layer come back)
//   k_ap_tile_layer   a raw image -> 8 x 4-texel tiles (fspt_scene.cpp tile_image): the single-layer images of SEPARATE sets
//   k_ap_interleave   four layers -> one image of 16-byte texels in 4 x 2-texel tiles: a QUAD set
//   k_ap_env_tile     the environment in the form FSPT_ENV_APRON selects
//   k_ap_records      floats 36..47 of every leaf slot's hit record: uv, texture set, ior, dielectric
// Which layers form which set, and in which form, is decided on the host by texset_classify (fspt_scene.cpp), the function
// fspt_scene_create uses: the set numbering is creation's.  Every kernel is one thread per OUTPUT element in output order,
// so a wave's stores are one contiguous run (16 bytes per lane in k_ap_interleave, 4 elsewhere) and its loads are runs of
// a tile row; nothing is shared between lanes, so there is no LDS and no atomic but the one "differs" flag per layer.
// Everything new is built in buffers of its own; only when all of it exists are the scene's pointers swapped and the old
// buffers freed - a failed allocation leaves the scene rendering as before.
#include "fspt_internal.hpp"

namespace fspt {
namespace {

const uint32_t AP_BS = 256;
// blocks of AP_BS threads for n elements, grid-stride beyond 2^20 blocks
uint32_t ap_blocks(size_t n) {
  const size_t b = (n + AP_BS - 1) / AP_BS;
  return (uint32_t)(b < 1 ? 1 : (b > (1u << 20) ? (1u << 20) : b));
}
#define AP_FOR(i, n) for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (size_t)gridDim.x * blockDim.x)

// out[2 l] = 1 when some texel of layer l differs from its texel 0 (zeroed before the launch), out[2 l + 1] = texel 0.
// blockIdx.y = the layer; per_layer texels each.
__global__ void k_ap_layer_const(const uint32_t *__restrict__ raw, size_t per_layer, uint32_t *__restrict__ out) {
  const uint32_t l = blockIdx.y;
  const uint32_t *src = raw + (size_t)l * per_layer;
  const uint32_t v0 = src[0];
  bool differs = false;
  AP_FOR(i, per_layer) differs = differs || src[i] != v0;
  if (differs) atomicOr(&out[2 * l], 1u);
  if (blockIdx.x == 0 && threadIdx.x == 0) out[2 * l + 1] = v0;
}

// src: w x h texels row-major; dst: ceil(w / 8) x ceil(h / 4) tiles of 8 x 4 texels, zero beyond the image
__global__ void k_ap_tile_layer(const uint32_t *__restrict__ src, uint32_t w, uint32_t h, uint32_t tx, size_t n_out, uint32_t *__restrict__ dst) {
  constexpr uint32_t TW = (uint32_t)TEX_TILE_W, TH = (uint32_t)TEX_TILE_H;
  AP_FOR(o, n_out) {
    const size_t tile = o / (TW * TH);
    const uint32_t in = (uint32_t)(o % (TW * TH));
    const uint32_t i = (uint32_t)(tile % tx) * TW + in % TW, j = (uint32_t)(tile / tx) * TH + in / TW;
    dst[o] = (i < w && j < h) ? src[(size_t)j * w + i] : 0u;
  }
}

struct ApQuad { uint32_t layer[4], is_const[4], first[4]; };

// raw: res x res texels per layer; dst: ceil(res / 4) x ceil(res / 2) tiles of 4 x 2 texels of 16 bytes (diffuse,
// emissive, mr, normal), zero beyond the image; a constant layer contributes its one texel
__global__ void k_ap_interleave(const uint32_t *__restrict__ raw, uint32_t res, uint32_t qtx, size_t n_out, ApQuad q, uint4 *__restrict__ dst) {
  const size_t per_layer = (size_t)res * res;
  AP_FOR(o, n_out) {
    const size_t tile = o >> 3;
    const uint32_t in = (uint32_t)(o & 7u);
    const uint32_t ix = (uint32_t)(tile % qtx) * 4u + (in & 3u), jy = (uint32_t)(tile / qtx) * 2u + (in >> 2);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (ix < res && jy < res) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = q.is_const[k] ? q.first[k] : raw[(size_t)q.layer[k] * per_layer + (size_t)jy * res + ix];
    }
    dst[o] = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

// overlapping 8 x 4-texel tiles: tile (a, b) = texels [7a, 7a + 8) x [3b, 3b + 4), REPEAT in s, CLAMP in t (main.js:174-178)
__global__ void k_ap_env_tile(const uint32_t *__restrict__ src, uint32_t w, uint32_t h, uint32_t tx, size_t n_out, uint32_t *__restrict__ dst) {
  AP_FOR(o, n_out) {
    const size_t tile = o >> 5;
    const uint32_t in = (uint32_t)(o & 31u), la = in & 7u, lb = in >> 3;
    const uint32_t a = (uint32_t)(tile % tx), b = (uint32_t)(tile / tx);
    const uint32_t i = (7u * a + la) % w;
    uint32_t j = 3u * b + lb;
    if (j > h - 1u) j = h - 1u;
    dst[o] = src[(size_t)j * w + i];
  }
}

// one thread per (leaf slot, float 36 + c): c 0..5 uv (only when given), 6 the texture set, 7..9 zero, 10 ior, 11 dielectric
__global__ void k_ap_records(const float *__restrict__ mat, const float *__restrict__ uv, const uint32_t *__restrict__ tri_set,
                             const uint32_t *__restrict__ slot_tri, size_t n_slots, uint32_t T, float *__restrict__ hitrec) {
  AP_FOR(id, n_slots * 12) {
    const size_t sl = id / 12;
    const uint32_t c = (uint32_t)(id % 12);
    const uint32_t ti = slot_tri[sl];
    if (ti >= T) continue; // "-1" padding: stays zero
    float *o = hitrec + sl * 48 + 36;
    if (c < 6u) { if (uv) o[c] = uv[(size_t)ti * 6 + c]; }
    else if (c == 6u) o[c] = __uint_as_float(tri_set[ti]);
    else if (c < 10u) o[c] = 0.0f;
    else o[c] = mat[(size_t)ti * 12 + (c - 1u)]; // 10 <- m[9] ior, 11 <- m[10] dielectric
  }
}

int ap_events(fspt_scene *s) {
  for (hipEvent_t &e : s->ap.ev) if (!e) HIP_TRY(hipEventCreate(&e));
  return FSPT_OK;
}

} // namespace

void appearance_release(fspt_scene *s) {
  hipFree(s->ap.raw);
  s->ap.raw = nullptr;
  for (hipEvent_t &e : s->ap.ev) if (e) { hipEventDestroy(e); e = nullptr; }
}

// The scene's current matTex as far as an appearance update reads it, in the current leaf order, from what the device
// holds: the four layer ids of every triangle's set (A.keys, the sets of the last materials call, behind the set index in
// its hit record), ior and dielectric (floats 46, 47).  A rebuild moves the records with their triangles, so this is the
// current order whatever happened since.
static int ap_current_mat(fspt_scene *s, const char *fn, std::vector<float> &mat) {
  const fspt_scene::Appearance &A = s->ap;
  const uint32_t T = s->n_tris;
  std::vector<uint32_t> slot_tri(s->n_slots);
  std::vector<float> rec(s->n_slots * 12);
  HIP_TRY(hipMemcpy(slot_tri.data(), s->slot_tri, s->n_slots * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(rec.data(), 48, (const char *)s->shade + 144, 192, 48, s->n_slots, hipMemcpyDeviceToHost));
  mat.assign((size_t)T * 12, 0.0f);
  for (size_t sl = 0; sl < s->n_slots; ++sl) {
    const uint32_t ti = slot_tri[sl];
    if (ti >= T) continue;
    uint32_t set = 0;
    std::memcpy(&set, &rec[sl * 12 + 6], 4);
    if (set >= A.keys.size()) { fspt_set_error("%s: a hit record names texture set %u, the last materials call made %zu", fn, set, A.keys.size()); return FSPT_E_STATE; }
    float *m = &mat[(size_t)ti * 12];
    m[0] = (float)A.keys[set][0]; m[1] = (float)A.keys[set][1]; m[3] = (float)A.keys[set][2]; m[2] = (float)A.keys[set][3];
    m[9] = rec[sl * 12 + 10]; m[10] = rec[sl * 12 + 11];
  }
  return FSPT_OK;
}

int appearance_materials(fspt_scene *s, const float *mat, const float *uv, const uint8_t *atlas, uint32_t res, uint32_t layers, const ApTextures *tx) {
  const char *fn = tx ? tx->fn : "fspt_scene_update_materials";
  fspt_scene::Appearance &A = s->ap;
  const uint32_t T = s->n_tris;
  const bool patch = tx && tx->layer_ids;
  std::vector<float> cur_mat;
  if (patch) { // (the retained atlas exists: the caller has looked)
    if (const int rc = ap_current_mat(s, fn, cur_mat)) return rc;
    mat = cur_mat.data();
  }
  hipStream_t st = nullptr;
  int rc = ap_events(s);
  if (rc) return rc;
  Hold hold;
  hipError_t e = hipSuccess;
  uint64_t uploaded = 0;
  uint32_t launches = 0;
  bool ev0 = false;
  auto begin = [&]() { if (!ev0 && e == hipSuccess) { e = hipEventRecord(A.ev[0], st); ev0 = true; } };
  // ---- the raw atlas: the caller's, uploaded, or the retained one ----
  void *raw = A.raw;
  std::vector<uint8_t> is_const = A.is_const;
  std::vector<uint32_t> first = A.first;
  if (tx) { res = tx->p->res; layers = patch ? A.raw_layers : tx->p->n_layers; }
  if (atlas || tx) {
    // a new raw atlas of this call's own: the caller's bytes, or packed here on the device from the caller's
    // sources - a patch packs its layers into a copy of the retained one, and only their flags are asked for again
    const size_t per_layer = (size_t)res * res, bytes = per_layer * layers * 4;
    const uint32_t n_flag = patch ? tx->p->n_layers : layers;
    uint32_t *d_flag = nullptr;
    e = hold.make(&raw, bytes);
    if (e == hipSuccess) e = hold.make((void **)&d_flag, (size_t)n_flag * 8);
    if (atlas) {
      if (e == hipSuccess) e = hipMemcpy(raw, atlas, bytes, hipMemcpyHostToDevice);
      uploaded += bytes;
    } else {
      if (e == hipSuccess && patch) e = hipMemcpyAsync(raw, A.raw, bytes, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) {
        e = texpack_launch(hold, tx->p, tx->on_device, tx->layer_ids, (uint32_t *)raw, st, A.ev[0], &uploaded, &launches);
        ev0 = e == hipSuccess;
      }
    }
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, (size_t)n_flag * 8, st);
    begin();
    if (e == hipSuccess) {
      const uint32_t bx = std::min<uint32_t>(ap_blocks(per_layer), 1024u);
      for (uint32_t l0 = 0; !patch && l0 < layers; l0 += 65535u) { // (grid.y <= 65535)
        const uint32_t nl = std::min<uint32_t>(layers - l0, 65535u);
        hipLaunchKernelGGL(k_ap_layer_const, dim3(bx, nl), dim3(AP_BS), 0, st, (const uint32_t *)raw + (size_t)l0 * per_layer, per_layer, d_flag + 2 * (size_t)l0);
        ++launches;
      }
      for (uint32_t k = 0; patch && k < n_flag; ++k) {
        hipLaunchKernelGGL(k_ap_layer_const, dim3(bx, 1), dim3(AP_BS), 0, st, (const uint32_t *)raw + (size_t)tx->layer_ids[k] * per_layer, per_layer, d_flag + 2 * (size_t)k);
        ++launches;
      }
      e = hipGetLastError();
    }
    std::vector<uint32_t> flags((size_t)n_flag * 2, 0u);
    if (e == hipSuccess) e = hipMemcpy(flags.data(), d_flag, flags.size() * 4, hipMemcpyDeviceToHost); // (waits for the kernel)
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return ap_fail(fn, e); } // (nothing in flight reads a buffer `hold` frees)
    if (!patch) { is_const.assign(layers, 0); first.assign(layers, 0u); }
    for (uint32_t k = 0; k < n_flag; ++k) {
      const uint32_t l = patch ? tx->layer_ids[k] : k;
      is_const[l] = flags[2 * k] == 0u; first[l] = flags[2 * k + 1];
    }
  } else {
    res = A.raw_res; layers = A.raw_layers;
  }
  const size_t per_layer = (size_t)res * res;
  // ---- the sets (host; creation's function) ----
  TexSetPlan pl;
  if ((rc = texset_classify(mat, T, layers, res, is_const.data(), first.data(), pl))) return rc;
  bool has_dielectric = false;
  for (uint32_t i = 0; i < T; ++i)
    if (mat[(size_t)i * 12 + 10] >= 0.0f) has_dielectric = true;
  // ---- every new buffer ----
  const uint32_t n_sets = (uint32_t)pl.keys.size();
  void *n_atlas = nullptr, *n_atlas4 = nullptr, *n_tab = nullptr, *stage = nullptr;
  const size_t single_bytes = (size_t)pl.single_texels * 4, stage_floats = (size_t)T * (12 + (uv ? 6 : 0) + 1);
  e = hold.make(&n_atlas, single_bytes);
  if (e == hipSuccess) e = hold.make(&n_atlas4, pl.quad_bytes);
  if (e == hipSuccess) e = hold.make(&n_tab, pl.tab.size() * 4);
  if (e == hipSuccess) e = hold.make(&stage, stage_floats * 4); // mat | tri_set | uv
  float *d_mat = (float *)stage, *d_uv = uv ? d_mat + (size_t)T * 13 : nullptr;
  uint32_t *d_set = (uint32_t *)(d_mat + (size_t)T * 12);
  if (e == hipSuccess) e = hipMemcpy(n_tab, pl.tab.data(), pl.tab.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_mat, mat, (size_t)T * 48, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_set, pl.tri_set.data(), (size_t)T * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && uv) e = hipMemcpy(d_uv, uv, (size_t)T * 24, hipMemcpyHostToDevice);
  uploaded += pl.tab.size() * 4 + stage_floats * 4;
  begin();
  if (e == hipSuccess) {
    const uint32_t tx = (res + TEX_TILE_W - 1) / TEX_TILE_W, ty = (res + TEX_TILE_H - 1) / TEX_TILE_H;
    const size_t layer_texels = (size_t)tx * ty * TEX_TILE_W * TEX_TILE_H;
    for (size_t k = 0; k < pl.single_layers.size(); ++k) {
      hipLaunchKernelGGL(k_ap_tile_layer, dim3(ap_blocks(layer_texels)), dim3(AP_BS), 0, st, (const uint32_t *)raw + (size_t)pl.single_layers[k] * per_layer,
                         res, res, tx, layer_texels, (uint32_t *)n_atlas + k * layer_texels);
      ++launches;
    }
    const uint32_t qtx = (res + 3u) / 4u, qty = (res + 1u) / 2u;
    const size_t quad_texels = (size_t)qtx * qty * 8;
    for (uint32_t si = 0; si < n_sets; ++si) {
      if (pl.kind[si] != TEXSET_QUAD) continue;
      ApQuad q;
      for (int k = 0; k < 4; ++k) { q.layer[k] = pl.keys[si][k]; q.is_const[k] = is_const[q.layer[k]]; q.first[k] = first[q.layer[k]]; }
      hipLaunchKernelGGL(k_ap_interleave, dim3(ap_blocks(quad_texels)), dim3(AP_BS), 0, st, (const uint32_t *)raw, res, qtx, quad_texels, q,
                         (uint4 *)n_atlas4 + (size_t)pl.tab[(size_t)si * 12 + 1] * 8);
      ++launches;
    }
    e = hipGetLastError();
  }
  // the layouts exist before a hit record names a set of theirs
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ap_fail(fn, e);
  // ---- the hit records (in place: the one step that cannot fail for want of memory), then the swap ----
  hipLaunchKernelGGL(k_ap_records, dim3(ap_blocks(s->n_slots * 12)), dim3(AP_BS), 0, st, d_mat, d_uv, d_set, (const uint32_t *)s->slot_tri, s->n_slots, T, (float *)s->shade);
  ++launches;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(A.ev[1], st));
  HIP_TRY(hipEventSynchronize(A.ev[1]));
  HIP_TRY(hipEventElapsedTime(&A.last_ms, A.ev[0], A.ev[1]));
  hold.take(n_atlas); hold.take(n_atlas4); hold.take(n_tab);
  atlas_install(s, n_atlas, single_bytes, n_atlas4, pl.quad_bytes, n_tab, n_sets, res, layers); // (frees the old three)
  s->has_dielectric = has_dielectric;
  A.keys = pl.keys;
  if (atlas || tx) { // ... and the retained raw atlas after them
    void *old_raw = A.raw;
    hold.take(raw);
    A.raw = raw; A.raw_res = res; A.raw_layers = layers;
    A.is_const.swap(is_const); A.first.swap(first);
    hipFree(old_raw);
  }
  A.last_launches = launches;
  A.last_uploaded = uploaded;
  return FSPT_OK;
}

size_t env_tiled_texels(uint32_t w, uint32_t h) {
#if FSPT_ENV_APRON
  const uint32_t tx = (w + 6u) / 7u, ty = (h + 2u) / 3u;
#else
  const uint32_t tx = (w + TEX_TILE_W - 1) / TEX_TILE_W, ty = (h + TEX_TILE_H - 1) / TEX_TILE_H;
#endif
  return (size_t)tx * ty * 32u;
}

hipError_t env_tile_launch(const uint32_t *raw, uint32_t w, uint32_t h, uint32_t *dst, hipStream_t st) {
  const size_t n_out = env_tiled_texels(w, h);
#if FSPT_ENV_APRON
  hipLaunchKernelGGL(k_ap_env_tile, dim3(ap_blocks(n_out)), dim3(AP_BS), 0, st, raw, w, h, (w + 6u) / 7u, n_out, dst);
#else
  hipLaunchKernelGGL(k_ap_tile_layer, dim3(ap_blocks(n_out)), dim3(AP_BS), 0, st, raw, w, h, (w + TEX_TILE_W - 1) / TEX_TILE_W, n_out, dst);
#endif
  return hipGetLastError();
}

void environment_swap(fspt_scene *s, void *n_env, uint64_t env_bytes, uint32_t w, uint32_t h, void *n_bins_d, uint32_t n_bins) {
  void *old[2] = {s->env, s->bins};
  s->env = n_env; s->bins = n_bins_d; s->env_bytes = env_bytes;
  s->d.env = (const uint32_t *)s->env; s->d.bins = (const uint4 *)s->bins;
  s->d.env_w = n_env ? w : 0; s->d.env_h = n_env ? h : 0; s->d.n_bins = n_bins;
  for (void *o : old) hipFree(o);
}

int appearance_environment(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h, const uint32_t *bins, uint32_t n_bins) {
  const char *fn = "fspt_scene_update_environment";
  fspt_scene::Appearance &A = s->ap;
  hipStream_t st = nullptr;
  int rc = ap_events(s);
  if (rc) return rc;
  Hold hold;
  void *n_bins_d = nullptr, *n_env = nullptr, *raw = nullptr;
  uint64_t uploaded = (uint64_t)n_bins * 16, env_bytes = 0;
  uint32_t launches = 0;
  hipError_t e = hold.make(&n_bins_d, (size_t)n_bins * 16);
  if (e == hipSuccess) e = hipMemcpy(n_bins_d, bins, (size_t)n_bins * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipEventRecord(A.ev[0], st);
  if (e == hipSuccess && env) {
    const size_t raw_bytes = (size_t)w * h * 4;
    env_bytes = env_tiled_texels(w, h) * 4;
    e = hold.make(&raw, raw_bytes);
    if (e == hipSuccess) e = hold.make(&n_env, env_bytes);
    if (e == hipSuccess) e = hipMemcpy(raw, env, raw_bytes, hipMemcpyHostToDevice);
    uploaded += raw_bytes;
    if (e == hipSuccess) {
      e = env_tile_launch((const uint32_t *)raw, w, h, (uint32_t *)n_env, st);
      ++launches;
    }
  }
  if (e == hipSuccess) e = hipEventRecord(A.ev[1], st);
  if (e == hipSuccess) e = hipEventSynchronize(A.ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&A.last_ms, A.ev[0], A.ev[1]);
  if (e != hipSuccess) return ap_fail(fn, e);
  hold.take(n_bins_d);
  if (n_env) hold.take(n_env);
  environment_swap(s, n_env, env_bytes, w, h, n_bins_d, n_bins);
  A.last_launches = launches;
  A.last_uploaded = uploaded;
  return FSPT_OK;
}

} // namespace fspt
