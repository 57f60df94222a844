// fspt_scene.cpp - the scene object: fspt_scene_create and what it is made of.  Mirrors the scene upload of the reference's
// main.js (initBVH 408-437, initAtlas 548-560).  In file order: the host tiling, the emitter light table, the integer tree
// work, the texture-set plan, the one install and one release of every scene part that a live-scene update shares
// (geometry_publish / geometry_free, atlas_install; the environment's is fspt::environment_swap), then fspt_scene_create as
// named steps, one host layout each.  Those layouts are the independent statement the GPU layout kernels (fspt_refit.hip,
// fspt_appearance.hip, fspt_sky.hip) are tested against byte for byte: plain host code, never routed through a kernel.
#include "fspt_internal.hpp"

#ifndef FSPT_NODE_TREELET
#define FSPT_NODE_TREELET 0 // nodes per treelet below the breadth-first top of the tree; 0 = pre-order (profiles/r02: A/B on the 1 M-triangle scene)
#endif

// Bytes of interleaved four-layer texture images (TEXSET_QUAD) a scene may allocate; sets beyond it fetch their image
// layers from single-layer images (fspt_set_texture_interleave_budget).
static std::atomic<uint64_t> g_texset_budget{8ull << 30};

// RGBA8 image (row-major, w x h) -> 8 x 4-texel tiles (fspt_device.hpp: TEX_TILE_*), padded to whole tiles.
// Returns the number of texels of the tiled image; with src == nullptr only that.
static size_t tile_image(const uint8_t *src, uint32_t w, uint32_t h, std::vector<uint32_t> &out) {
  const uint32_t tx = (w + fspt::TEX_TILE_W - 1) / fspt::TEX_TILE_W, ty = (h + fspt::TEX_TILE_H - 1) / fspt::TEX_TILE_H;
  const size_t n = (size_t)tx * ty * fspt::TEX_TILE_W * fspt::TEX_TILE_H;
  if (!src) return n;
  out.assign(n, 0u);
  for (uint32_t j = 0; j < h; ++j)
    for (uint32_t i = 0; i < w; ++i) {
      uint32_t v;
      std::memcpy(&v, src + ((size_t)j * w + i) * 4, 4);
      out[((size_t)(j / fspt::TEX_TILE_H) * tx + i / fspt::TEX_TILE_W) * (fspt::TEX_TILE_W * fspt::TEX_TILE_H) +
          (j % fspt::TEX_TILE_H) * fspt::TEX_TILE_W + (i % fspt::TEX_TILE_W)] = v;
    }
  return n;
}

// Vose alias table in float64 (stored float32): entry i is taken with probability (prob_i + sum_{alias_j = i} (1 - prob_j)) / n
static bool alias_build(const float *w, uint32_t n, std::vector<float> &prob, std::vector<uint32_t> &alias) {
  double sum = 0.0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!(w[i] >= 0.0f) || !std::isfinite(w[i])) return false;
    sum += (double)w[i];
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) return false;
  std::vector<double> sc(n);
  std::vector<uint32_t> small, large;
  for (uint32_t i = 0; i < n; ++i) {
    sc[i] = ((double)w[i] / sum) * (double)n;
    (sc[i] < 1.0 ? small : large).push_back(i);
  }
  prob.assign(n, 1.0f);
  alias.resize(n);
  for (uint32_t i = 0; i < n; ++i) alias[i] = i;
  while (!small.empty() && !large.empty()) {
    const uint32_t l = small.back(), g = large.back();
    small.pop_back(); large.pop_back();
    prob[l] = (float)sc[l];
    alias[l] = g;
    sc[g] = (sc[g] + sc[l]) - 1.0;
    (sc[g] < 1.0 ? small : large).push_back(g);
  }
  // what is left holds probability 1 up to rounding: kept whole
  return true;
}

// the host copies of the table, which the GPU builder fills only when somebody asks
static int light_mirrors_ensure(fspt_scene *s) {
  if (s->lg.builder != FSPT_LIGHT_BUILDER_GPU || s->lg.mirrors_valid) return FSPT_OK;
  return fspt::lights_mirrors_gpu(s);
}

// The scene's emitter light table: per-triangle weights on the device (k_light_weights over one leaf slot of
// each triangle), the alias table of the triangles with weight > 0 on the host, their light records on the device
int light_table_ensure(fspt_scene *s) {
  if (s->lights_built) return FSPT_OK;
  int rc = check_device(s->device);
  if (rc) return rc;
  if (s->lg.builder == FSPT_LIGHT_BUILDER_GPU) { // (the same arrays, made by fspt_lights_build.hip's kernels)
    rc = fspt::lights_build_gpu(s);
    if (rc) return rc;
    s->lg.built_by = FSPT_LIGHT_BUILDER_GPU;
    s->lights_built = true;
    return FSPT_OK;
  }
  const uint32_t T = s->n_tris;
  for (hipEvent_t &ev : s->lg.host_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  s->lg.host_timed = false;
  // leaf slots and their triangles (the hit records are stored per slot)
  const size_t slots_n = s->n_slots;
  s->l_slot_tri.resize(slots_n);
  {
    const hipError_t e = hipMemcpy(s->l_slot_tri.data(), s->slot_tri, slots_n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { fspt_set_error("light table: %s", hipGetErrorString(e)); return FSPT_E_HIP; }
  }
  std::vector<uint32_t> first(T, 0xFFFFFFFFu);
  for (size_t sl = slots_n; sl-- > 0;) if (s->l_slot_tri[sl] < T) first[s->l_slot_tri[sl]] = (uint32_t)sl;
  std::vector<uint32_t> tri_slot(T, 0u);
  for (uint32_t i = 0; i < T; ++i) tri_slot[i] = first[i] == 0xFFFFFFFFu ? 0u : first[i];
  uint32_t *d_slots = nullptr;
  float *d_w = nullptr;
  hipError_t e = hipMalloc((void **)&d_slots, (size_t)T * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&d_w, (size_t)T * 4);
  if (e == hipSuccess) e = hipEventRecord(s->lg.host_ev[0], nullptr);
  if (e == hipSuccess) e = hipMemcpy(d_slots, tri_slot.data(), (size_t)T * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = fspt::launch_light_weights(s->d, d_slots, T, d_w, nullptr, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  s->l_weight.assign(T, 0.0f);
  if (e == hipSuccess) e = hipMemcpy(s->l_weight.data(), d_w, (size_t)T * 4, hipMemcpyDeviceToHost);
  for (uint32_t i = 0; i < T; ++i) if (first[i] == 0xFFFFFFFFu) s->l_weight[i] = 0.0f; // (a triangle in no leaf: never hit)
  s->l_tri.clear();
  std::vector<float> wl;
  std::vector<uint32_t> ent_slot;
  for (uint32_t i = 0; i < T; ++i)
    if (s->l_weight[i] > 0.0f) { s->l_tri.push_back(i); wl.push_back(s->l_weight[i]); ent_slot.push_back(tri_slot[i]); }
  const uint32_t n = (uint32_t)s->l_tri.size();
  s->l_prob.clear(); s->l_alias_h.clear();
  std::vector<float> lp(n, 0.0f);
  s->l_pick_h.assign(slots_n, 0.0f);
  if (e == hipSuccess && n > 0) {
    if (!alias_build(wl.data(), n, s->l_prob, s->l_alias_h)) { hipFree(d_slots); hipFree(d_w); fspt_set_error("light table: bad weights"); return FSPT_E_INVALID; }
    std::vector<double> real(n, 0.0);
    for (uint32_t i = 0; i < n; ++i) {
      real[i] += (double)s->l_prob[i];
      if (s->l_alias_h[i] != i) real[s->l_alias_h[i]] += 1.0 - (double)s->l_prob[i];
    }
    std::vector<float> tri_p(T, 0.0f);
    for (uint32_t i = 0; i < n; ++i) { lp[i] = (float)(real[i] / (double)n); tri_p[s->l_tri[i]] = lp[i]; }
    for (size_t sl = 0; sl < slots_n; ++sl) if (s->l_slot_tri[sl] < T) s->l_pick_h[sl] = tri_p[s->l_slot_tri[sl]];
    std::vector<uint32_t> al(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) { std::memcpy(&al[2 * i], &s->l_prob[i], 4); al[2 * i + 1] = s->l_alias_h[i]; }
    e = hipMalloc(&s->l_alias, (size_t)n * 8);
    if (e == hipSuccess) e = hipMemcpy(s->l_alias, al.data(), (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&s->l_p, (size_t)n * 4);
    if (e == hipSuccess) e = hipMemcpy(s->l_p, lp.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&s->l_rec, (size_t)n * 64);
    if (e == hipSuccess) e = hipMemcpy(d_slots, ent_slot.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = fspt::launch_light_weights(s->d, d_slots, n, d_w, (float4 *)s->l_rec, nullptr);
    if (e == hipSuccess) e = hipMalloc(&s->l_pick, slots_n * 4);
    if (e == hipSuccess) e = hipMemcpy(s->l_pick, s->l_pick_h.data(), slots_n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipEventRecord(s->lg.host_ev[1], nullptr);
  hipFree(d_slots); hipFree(d_w);
  if (e != hipSuccess) { fspt_set_error("light table: %s", hipGetErrorString(e)); return FSPT_E_HIP; }
  s->lg.host_timed = true;
  s->lg.built_by = FSPT_LIGHT_BUILDER_HOST;
  s->lg.bytes_d2h = (uint64_t)slots_n * 4 + (uint64_t)T * 4;
  s->lg.bytes_h2d = (uint64_t)T * 4 + (n ? (uint64_t)n * 16 + (uint64_t)slots_n * 4 : 0u);
  s->d.light_alias = (const uint2 *)s->l_alias;
  s->d.light_rec = (const float4 *)s->l_rec;
  s->d.light_p = (const float *)s->l_p;
  s->d.light_pick = (const float *)s->l_pick;
  s->d.n_lights = n;
  s->lights_built = true;
  return FSPT_OK;
}

// ---- the integer part of fspt_scene_create: what follows from the tree's (left, right, triStart) words alone ----
namespace {
struct TreeWords {
  const char *base; size_t stride;
  int32_t operator()(uint32_t node, int w) const { int32_t v; std::memcpy(&v, base + (size_t)node * stride + (size_t)w * 4, 4); return v; }
};
}

int tree_topology(const void *words, size_t stride_bytes, uint32_t N, uint32_t T, TreeTopology &tp) {
  const TreeWords word{(const char *)words, stride_bytes};
  // ---- validate + renumber interior nodes ------------------------------------------
  // The first TOP_BFS interior nodes in breadth-first order get the lowest numbers (every ray walks the top of
  // the tree: the traversal kernel keeps a prefix of them in LDS); the rest keep their pre-order.
  std::vector<int32_t> &ref = tp.ref;
  std::vector<uint32_t> &leaf_first = tp.leaf_first; // first triangle of every leaf, in node order
  uint32_t &n_interior = tp.n_interior;
  ref.assign(N, 0); leaf_first.clear(); n_interior = 0;
  for (uint32_t i = 0; i < N; ++i) {
    int32_t l = word(i, 0), r = word(i, 1), ts = word(i, 2);
    if (ts > -1) {
      if ((uint32_t)ts > T) { fspt_set_error("node %u: triStart %d > n_tris %u", i, ts, T); return FSPT_E_INVALID; }
      ref[i] = ~(int32_t)leaf_first.size(); // leaf record index
      leaf_first.push_back((uint32_t)ts);
    } else {
      // serializeTree is pre-order (bvh.js:33-50): children come after their parent.
      if (l <= (int32_t)i || r <= (int32_t)i || (uint32_t)l >= N || (uint32_t)r >= N) {
        fspt_set_error("node %u: child indices (%d,%d) violate pre-order / range [%u,%u)", i, l, r, i + 1, N);
        return FSPT_E_INVALID;
      }
      ref[i] = INT32_MAX; // interior, numbered below
      n_interior++;
    }
  }
  {
    const uint32_t TOP_BFS = 256;
    uint32_t next = 0;
    std::vector<uint32_t> queue;
    if (N && word(0, 2) <= -1) queue.push_back(0);
    for (size_t q = 0; q < queue.size() && next < TOP_BFS; ++q) {
      uint32_t i = queue[q];
      ref[i] = (int32_t)next++;
      uint32_t l = (uint32_t)word(i, 0), r = (uint32_t)word(i, 1);
      if (word(l, 2) <= -1) queue.push_back(l);
      if (word(r, 2) <= -1) queue.push_back(r);
    }
#if FSPT_NODE_TREELET > 1
    // Below the breadth-first top: TREELETS.  A treelet = a subtree root and its descendants in breadth-first order, up to
    // FSPT_NODE_TREELET nodes, stored contiguously; the treelets hanging off it follow, depth-first.  A ray that enters
    // a treelet finds the next few levels of its descent - and the sibling it will pop later - in the same or the next
    // 128-byte lines, instead of one line per level (pre-order keeps only the LEFT child next to its parent).  Only the
    // numbering changes: same nodes, same boxes, same traversal order, bit-identical results.
    {
      std::vector<uint32_t> roots; // subtree roots waiting to be laid out (a stack: depth-first over treelets)
      for (size_t q = queue.size(); q-- > 0;)
        if (ref[queue[q]] == INT32_MAX) roots.push_back(queue[q]); // discovered by the top's BFS but beyond its budget
      std::vector<uint32_t> local;
      while (!roots.empty()) {
        const uint32_t root = roots.back();
        roots.pop_back();
        local.assign(1, root);
        for (size_t q = 0; q < local.size(); ++q) {
          const uint32_t i = local[q];
          ref[i] = (int32_t)next++;
          const uint32_t ch[2] = {(uint32_t)word(i, 0), (uint32_t)word(i, 1)};
          for (uint32_t c : ch)
            if (word(c, 2) <= -1 && local.size() < (size_t)FSPT_NODE_TREELET) local.push_back(c);
        }
        // children of the treelet's nodes that did not fit: roots of the next treelets (right before left on the
        // stack, so the left subtree is laid out first, like pre-order)
        for (size_t q = local.size(); q-- > 0;) {
          const uint32_t i = local[q];
          const uint32_t ch[2] = {(uint32_t)word(i, 1), (uint32_t)word(i, 0)};
          for (uint32_t c : ch)
            if (word(c, 2) <= -1 && ref[c] == INT32_MAX) roots.push_back(c);
        }
      }
    }
#endif
    for (uint32_t i = 0; i < N; ++i)
      if (ref[i] == INT32_MAX) ref[i] = (int32_t)next++; // (pre-order for whatever is left: nothing, with treelets)
  }
  // depth of every node (root 0); a child's depth = parent's + 1
  tp.depth.assign(N, 0);
  tp.max_depth = 0;
  for (uint32_t i = 0; i < N; ++i) {
    if (word(i, 2) > -1) continue;
    const int32_t l = word(i, 0), r = word(i, 1);
    tp.depth[l] = tp.depth[i] + 1;
    tp.depth[r] = tp.depth[i] + 1;
    if (tp.depth[i] + 1 > tp.max_depth) tp.max_depth = tp.depth[i] + 1;
  }
  return FSPT_OK;
}

// ---- what fspt_scene_update_geometry needs of a tree (host memory; fspt_internal.hpp) ----
void tree_refit_tables(const void *words, size_t stride_bytes, uint32_t N, uint32_t T, const TreeTopology &tp, fspt_scene::Refit &R) {
  const TreeWords word{(const char *)words, stride_bytes};
  const std::vector<int32_t> &ref = tp.ref;
  const std::vector<uint32_t> &leaf_first = tp.leaf_first, &depth = tp.depth;
  const size_t n_leaves = leaf_first.size();
  const uint32_t max_depth = tp.max_depth;
  R.lvl_nodes.clear();
  const uint32_t NO = fspt_scene::Refit::NO_DST;
  R.ok = true;
  R.node_dst.assign(N, NO);
  R.node_owned.assign(N, NO);
  for (uint32_t i = 0; i < N; ++i) {
    if (word(i, 2) > -1) continue;
    const uint32_t ch[2] = {(uint32_t)word(i, 0), (uint32_t)word(i, 1)};
    for (uint32_t k = 0; k < 2; ++k) {
      if (R.node_dst[ch[k]] != NO || (k == 1 && ch[1] == ch[0])) R.ok = false; // a node with two parents
      R.node_dst[ch[k]] = 2u * (uint32_t)ref[i] + k;
    }
  }
  // ownership: a leaf owns [triStart, the next larger triStart among the leaves, or n_tris)
  std::vector<uint32_t> by_first(n_leaves);
  for (size_t L = 0; L < n_leaves; ++L) by_first[L] = (uint32_t)L;
  std::sort(by_first.begin(), by_first.end(), [&](uint32_t a, uint32_t b) { return leaf_first[a] < leaf_first[b]; });
  R.leaf_first = leaf_first;
  R.leaf_cnt.assign(n_leaves, 0u);
  R.leaf_dst.assign(n_leaves, NO);
  for (size_t q = 0; q < n_leaves; ++q) {
    const uint32_t a = leaf_first[by_first[q]], b = q + 1 < n_leaves ? leaf_first[by_first[q + 1]] : T;
    if (q + 1 < n_leaves && a == b) R.ok = false; // two leaves with the same range
    R.leaf_cnt[by_first[q]] = b - a;
  }
  if (!n_leaves || leaf_first[by_first[0]] != 0u) R.ok = false; // triangles below the first triStart belong to no leaf
  std::vector<std::vector<uint32_t>> levels(max_depth + 1);
  for (uint32_t i = 0; i < N; ++i) {
    if (word(i, 2) > -1) { const uint32_t L = (uint32_t)~ref[i]; R.leaf_dst[L] = R.node_dst[i]; R.node_owned[i] = R.leaf_cnt[L]; }
    else if (i > 0 && R.node_dst[i] != NO) { levels[depth[i]].push_back((uint32_t)ref[i]); levels[depth[i]].push_back(R.node_dst[i]); }
  }
  R.lvl_off.assign(1, 0u);
  for (size_t dpt = levels.size(); dpt-- > 0;) {
    if (levels[dpt].empty()) continue;
    R.lvl_nodes.insert(R.lvl_nodes.end(), levels[dpt].begin(), levels[dpt].end());
    R.lvl_off.push_back((uint32_t)(R.lvl_nodes.size() / 2));
  }
}

// ---- material texture sets: the four atlas layers a triangle samples at one uv (tracer.fs:453-456) ----
// layer = clamp(floor(id + 0.5), 0, layers - 1) as texture(sampler2DArray) selects it; same binary32 arithmetic here
uint32_t texset_layer_of(float id, uint32_t n_layers) {
  const float x = std::floor(id + 0.5f);
  if (!(x >= 0.0f)) return 0u; // negative, NaN (the device's float -> int conversion gives 0 for NaN)
  if (x >= (float)(n_layers - 1u)) return n_layers - 1u;
  return (uint32_t)x;
}

// A layer whose texels are all equal - every flat colour: TexturePacker fills whole layers with them
// (texture_packer.js:36-42), and a colours-only atlas is 1 x 1 - is never stored: its texel sits in the sets that use
// it.  A set with two or more image layers gets ONE interleaved image (16-byte texels: diffuse, emissive, mr, normal;
// 4 x 2-texel tiles = 128 bytes), as long as the interleaving budget lasts; the image layers of the other sets are
// stored once each as single-layer images in 8 x 4-texel tiles.
int texset_classify(const float *mat, uint32_t T, uint32_t n_layers, uint32_t res, const uint8_t *is_const, const uint32_t *first, TexSetPlan &pl) {
  std::map<std::array<uint32_t, 4>, uint32_t> set_ids;
  std::vector<std::array<uint32_t, 4>> &set_keys = pl.keys;
  set_keys.clear();
  pl.tri_set.assign(T, 0u);
  for (uint32_t i = 0; i < T; ++i) {
    const float *m = mat + (size_t)i * 12;
    const std::array<uint32_t, 4> key = {texset_layer_of(m[0], n_layers), texset_layer_of(m[1], n_layers), texset_layer_of(m[3], n_layers), texset_layer_of(m[2], n_layers)}; // diffuse, emissive, mr, normal
    auto it = set_ids.find(key);
    if (it == set_ids.end()) {
      it = set_ids.emplace(key, (uint32_t)set_keys.size()).first;
      set_keys.push_back(key);
    }
    pl.tri_set[i] = it->second;
  }
  const uint32_t n_sets = (uint32_t)set_keys.size();
  const uint32_t qtx = (res + 3u) / 4u, qty = (res + 1u) / 2u;
  const size_t quad_tiles = (size_t)qtx * qty;             // 128-byte tiles per interleaved image
  std::vector<uint32_t> &tab = pl.tab, &kind = pl.kind;
  tab.assign((size_t)n_sets * 12, 0u); kind.assign(n_sets, fspt::TEXSET_CONST);
  std::vector<int64_t> &layer_base = pl.layer_base;         // single-layer image of a layer, in tiles (-1: not stored)
  layer_base.assign(n_layers, -1);
  pl.single_layers.clear();
  uint64_t quad_bytes = 0;
  uint32_t n_quad = 0;
  for (uint32_t si = 0; si < n_sets; ++si) {
    const auto &key = set_keys[si];
    uint32_t n_img = 0, distinct[4];
    for (int k = 0; k < 4; ++k) {
      if (is_const[key[k]]) continue;
      bool seen = false;
      for (uint32_t q = 0; q < n_img; ++q) seen = seen || distinct[q] == key[k];
      if (!seen) distinct[n_img++] = key[k];
    }
    if (n_img >= 2 && quad_bytes + quad_tiles * 128u <= g_texset_budget && (n_quad + 1ull) * quad_tiles < 0xFFFFFFFFull) {
      kind[si] = fspt::TEXSET_QUAD;
      quad_bytes += quad_tiles * 128u;
      n_quad++;
    } else if (n_img >= 1) {
      kind[si] = fspt::TEXSET_SEPARATE;
    }
  }
  // single-layer images: the image layers of SEPARATE sets
  std::vector<uint32_t> none;
  const size_t layer_texels = tile_image(nullptr, res, res, none);
  size_t single = 0; // texels
  for (uint32_t si = 0; si < n_sets; ++si) {
    if (kind[si] != fspt::TEXSET_SEPARATE) continue;
    for (int k = 0; k < 4; ++k) {
      const uint32_t l = set_keys[si][k];
      if (is_const[l] || layer_base[l] >= 0) continue;
      layer_base[l] = (int64_t)(single / (fspt::TEX_TILE_W * fspt::TEX_TILE_H));
      pl.single_layers.push_back(l);
      single += layer_texels;
    }
  }
  pl.quad_bytes = quad_bytes;
  pl.single_texels = single;
  if (single / (fspt::TEX_TILE_W * fspt::TEX_TILE_H) >= 0xFFFFFFFFull) {
    fspt_set_error("atlas too large: %zu texels of image layers", single);
    return FSPT_E_INVALID;
  }
  uint32_t qi = 0;
  for (uint32_t si = 0; si < n_sets; ++si) {
    const auto &key = set_keys[si];
    uint32_t *q = &tab[(size_t)si * 12];
    q[0] = kind[si];
    for (int k = 0; k < 4; ++k) {
      q[4 + k] = first[key[k]];
      q[8 + k] = (kind[si] == fspt::TEXSET_SEPARATE && !is_const[key[k]]) ? (uint32_t)layer_base[key[k]] : fspt::LAYER_CONST;
    }
    if (kind[si] != fspt::TEXSET_QUAD) continue;
    q[1] = (uint32_t)(qi * quad_tiles);
    qi++;
  }
  return FSPT_OK;
}

int geometry_changed_lights(fspt_scene *s) {
  int rc = FSPT_OK;
  // the emitter light table depends on the triangles' areas: release it; light_table_ensure rebuilds it from the device arrays
  if (s->lights_built) {
    hipFree(s->l_alias); hipFree(s->l_rec); hipFree(s->l_p); hipFree(s->l_pick);
    s->l_alias = s->l_rec = s->l_p = s->l_pick = nullptr;
    s->d.light_alias = nullptr; s->d.light_rec = nullptr; s->d.light_p = nullptr; s->d.light_pick = nullptr;
    s->d.n_lights = 0;
    s->lights_built = false;
    s->lg.mirrors_valid = false; // (the GPU builder's arrays stay allocated: its next build writes them again)
  }
  for (fspt_target *t : s->targets)
    if (t->lights == FSPT_LIGHTS_EMITTERS) { rc = light_table_ensure(s); if (rc) return rc; break; }
  return FSPT_OK;
}

// ---- one install and one release per scene part (fspt_internal.hpp): shared by fspt_scene_create and the live-scene updates ----
// The geometry's DScene fields and counts, from the scene's own array pointers (set by the caller) and the tree they hold
void geometry_publish(fspt_scene *s, const TreeTopology &tp, uint32_t n_nodes, size_t n_slots, bool quads_ok) {
  s->d.nodes = (const float4 *)s->nodes;
  s->d.quads = quads_ok ? (const float4 *)s->quads : nullptr; // (not usable: the boxes are not unions, see pack_quads / k_refit_quads)
  s->d.leaves = (const float *)s->tris; s->d.slot_tri = (const uint32_t *)s->slot_tri; s->d.hitrec = (const float4 *)s->shade;
  s->d.root_ref = tp.ref[0];
  // Entries of a lane's traversal stack: one more than the walk can use (it pushes a far child only at an interior node,
  // the deepest of which sits at depth max_depth - 1).  Dropping the spare entry gives the 1 M-triangle scene - depth 22 -
  // its sixth resident trace block per CU at the price of the LDS copy of the top of the tree (8 nodes instead of 31):
  // measured +-0 (profiles/r06/ab_final_constants_c3.log, f_spare0), so the spare stays.
  s->d.stack_n = tp.max_depth + 1;
  s->d.n_top = tp.n_interior < 256u ? tp.n_interior : 256u; // interior nodes numbered breadth-first
  s->lg.topo_valid = false; // (the GPU light builder's triangle-to-slot arrays)
  s->depth = tp.max_depth; s->n_nodes = n_nodes; s->n_interior = tp.n_interior; s->n_slots = n_slots;
}

// The scene's atlas and texture-set table become the new device buffers; the old ones are freed (like fspt::environment_swap).
void atlas_install(fspt_scene *s, void *n_atlas, uint64_t atlas_bytes, void *n_atlas4, uint64_t atlas4_bytes, void *n_tab, uint32_t n_sets, uint32_t res, uint32_t layers) {
  void *old[3] = {s->atlas, s->atlas4, s->tex_sets};
  s->atlas = n_atlas; s->atlas4 = n_atlas4; s->tex_sets = n_tab;
  s->atlas_bytes = atlas_bytes; s->atlas4_bytes = atlas4_bytes;
  s->d.atlas = (const uint32_t *)s->atlas; s->d.atlas4 = (const uint4 *)s->atlas4; s->d.tex_sets = (const uint4 *)s->tex_sets;
  s->d.n_tex_sets = n_sets; s->d.atlas_res = res; s->d.atlas_layers = layers;
  for (void *o : old) hipFree(o);
}

// ---- fspt_scene_create's steps: the argument refusals in their order, then one layout each from the caller's arrays ----
static int desc_check(const fspt_scene_desc *desc) {
  if (!desc->bvh || !desc->tri || !desc->mat || !desc->norm || !desc->uv || desc->n_nodes == 0 || desc->n_tris == 0) { fspt_set_error("fspt_scene_create: bvh/tri/mat/norm/uv must be non-empty"); return FSPT_E_INVALID; }
  if (!desc->atlas || desc->atlas_res == 0 || desc->atlas_layers == 0) { fspt_set_error("fspt_scene_create: atlas must have at least one layer"); return FSPT_E_INVALID; }
  if (!desc->bins || desc->n_bins == 0) { fspt_set_error("fspt_scene_create: radianceBins must hold at least one bin (main.js:292)"); return FSPT_E_INVALID; }
  if (desc->env && (desc->env_w == 0 || desc->env_h == 0)) { fspt_set_error("fspt_scene_create: env given with zero size"); return FSPT_E_INVALID; }
  if (desc->leaf_size == 0 || desc->leaf_size > 64) { fspt_set_error("fspt_scene_create: leaf_size %u out of range [1,64]", desc->leaf_size); return FSPT_E_INVALID; }
  return FSPT_OK;
}

// 64-byte interior records, at their native index (TreeTopology::ref): the children's boxes, then their refs as int32 bits.
// bvh = 9 floats per reference node: left, right, triStart (words) | box min.xyz max.xyz.  No interior node: one zero record.
static std::vector<float> pack_nodes(const TreeWords &word, const float *bvh, uint32_t N, const TreeTopology &tp) {
  std::vector<float> nodes((size_t)(tp.n_interior ? tp.n_interior : 1) * 16, 0.0f);
  for (uint32_t i = 0; i < N; ++i) {
    if (word(i, 2) > -1) continue;
    const int32_t l = word(i, 0), r = word(i, 1);
    float *n = &nodes[(size_t)tp.ref[i] * 16];
    const float *lb = bvh + (size_t)l * 9 + 3, *rb = bvh + (size_t)r * 9 + 3;
    n[0] = lb[0]; n[1] = lb[1]; n[2] = lb[3]; n[3] = lb[4];   // lmin.xy lmax.xy
    n[4] = rb[0]; n[5] = rb[1]; n[6] = rb[3]; n[7] = rb[4];   // rmin.xy rmax.xy
    n[8] = lb[2]; n[9] = lb[5]; n[10] = rb[2]; n[11] = rb[5]; // lmin.z lmax.z rmin.z rmax.z
    const int32_t lr[4] = {tp.ref[l], tp.ref[r], 0, 0};
    std::memcpy(n + 12, lr, 16);
  }
  return nodes;
}

// Two-level nodes (fspt_device.hpp "quad"): the node records of both children side by side, one cache line.  Usable only
// when every interior node's box IS the union of its children's boxes, bit for bit (true for bvh.js trees: a node's box is built
// from its own triangles); checked here on the caller's arrays.  Returns whether they are; `quads` is empty otherwise.
static bool pack_quads(const TreeWords &word, const float *bvh, uint32_t N, const TreeTopology &tp, const std::vector<float> &nodes, std::vector<float> &quads) {
  const std::vector<int32_t> &ref = tp.ref;
  if (!tp.n_interior) return false;
  bool quad_ok = true;
  quads.assign((size_t)tp.n_interior * 32, 0.0f);
  auto bits = [](float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; };
  for (uint32_t i = 0; i < N && quad_ok; ++i) {
    if (word(i, 2) > -1) continue;
    const int32_t ch[2] = {word(i, 0), word(i, 1)};
    float *q = &quads[(size_t)ref[i] * 32];
    int32_t refs[8] = {fspt::REF_SENTINEL, fspt::REF_SENTINEL, ref[ch[0]], ref[ch[1]], fspt::REF_SENTINEL, fspt::REF_SENTINEL, 0, 0};
    for (int k = 0; k < 2 && quad_ok; ++k) {
      const int32_t c = ch[k];
      float *part = q + 16 * k;
      const float *cb = bvh + (size_t)c * 9 + 3; // the child's own box: min.xyz max.xyz
      if (word(c, 2) > -1) { // a leaf: its own box, twice
        part[0] = part[4] = cb[0]; part[1] = part[5] = cb[1]; part[2] = part[6] = cb[3]; part[3] = part[7] = cb[4];
        part[8] = part[10] = cb[2]; part[9] = part[11] = cb[5];
      } else {
        const float *cn = &nodes[(size_t)ref[c] * 16];
        std::memcpy(part, cn, 48);
        std::memcpy(&refs[4 * k], cn + 12, 8);
      }
      // box(c) == union of the two boxes of its part, exactly?  (the comparison the device's v_min / v_max make; a pair
      // of candidates that compare equal must be the same bits: -0 / +0)
      const float lo[3][2] = {{part[0], part[4]}, {part[1], part[5]}, {part[8], part[10]}};
      const float hi[3][2] = {{part[2], part[6]}, {part[3], part[7]}, {part[9], part[11]}};
      for (int a = 0; a < 3 && quad_ok; ++a) {
        const float mn = lo[a][0] < lo[a][1] ? lo[a][0] : lo[a][1], mx = hi[a][0] > hi[a][1] ? hi[a][0] : hi[a][1];
        if (std::isnan(lo[a][0]) || std::isnan(lo[a][1]) || std::isnan(hi[a][0]) || std::isnan(hi[a][1])) quad_ok = false;
        if (lo[a][0] == lo[a][1] && bits(lo[a][0]) != bits(lo[a][1])) quad_ok = false;
        if (hi[a][0] == hi[a][1] && bits(hi[a][0]) != bits(hi[a][1])) quad_ok = false;
        if (bits(mn) != bits(cb[a]) || bits(mx) != bits(cb[3 + a])) quad_ok = false;
      }
    }
    std::memcpy(q + 12, &refs[0], 16);
    std::memcpy(q + 28, &refs[4], 16);
  }
  if (!quad_ok) quads.clear();
  return quad_ok;
}

// Pre-edged triangles (v1, e1 = v2 - v1, e2 = v3 - v1), padded by leaf_size "-1" triangles (main.js:150-152)
static std::vector<float> pack_triangles(const float *tri, uint32_t T, uint32_t leaf_size) {
  const uint32_t TP = T + leaf_size;
  std::vector<float> tris((size_t)TP * 9, 0.0f);
  for (uint32_t i = 0; i < TP; ++i) {
    float v[9];
    if (i < T) std::memcpy(v, tri + (size_t)i * 9, 36);
    else for (int k = 0; k < 9; ++k) v[k] = -1.0f;
    float *o = &tris[(size_t)i * 9];
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    o[3] = v[3] - v[0]; o[4] = v[4] - v[1]; o[5] = v[5] - v[2]; // e1 = v2 - v1 (tracer.fs:301)
    o[6] = v[6] - v[0]; o[7] = v[7] - v[1]; o[8] = v[8] - v[2]; // e2 = v3 - v1 (tracer.fs:302)
  }
  return tris;
}

// Leaf records: the leaf_size triangles processLeaf reads from each leaf's first one, component-major (9 x LS floats),
// and slot_tri: leaf slot (L, k) holds triangle leaf_first[L] + k.  No leaf: one zero record.
static void pack_leaves(const std::vector<float> &tris, const std::vector<uint32_t> &leaf_first, uint32_t LS, std::vector<float> &leaves, std::vector<uint32_t> &slot_tri) {
  const size_t n_leaves = leaf_first.size();
  leaves.assign((n_leaves ? n_leaves : 1) * (size_t)LS * 9, 0.0f);
  slot_tri.assign((n_leaves ? n_leaves : 1) * (size_t)LS, 0u);
  for (size_t L = 0; L < n_leaves; ++L) {
    float *rec = &leaves[L * LS * 9];
    for (uint32_t k = 0; k < LS; ++k) {
      const uint32_t ti = leaf_first[L] + k; // <= T - 1 + leaf_size: inside the padded array
      for (int c = 0; c < 9; ++c) rec[(size_t)c * LS + k] = tris[(size_t)ti * 9 + c];
      slot_tri[L * LS + k] = ti;
    }
  }
}

// Per atlas layer (RGBA8, res x res, layer-major): its texel 0, and whether every texel equals it - a flat colour (texset_classify)
static void layer_flags(const uint8_t *atlas, uint32_t res, uint32_t n_layers, std::vector<uint8_t> &is_const, std::vector<uint32_t> &first) {
  const size_t per_layer = (size_t)res * res;
  is_const.assign(n_layers, 1); first.assign(n_layers, 0u);
  for (uint32_t l = 0; l < n_layers; ++l) {
    const uint8_t *src = atlas + (size_t)l * per_layer * 4;
    std::memcpy(&first[l], src, 4);
    for (size_t k = 1; k < per_layer && is_const[l]; ++k) is_const[l] = std::memcmp(src + k * 4, &first[l], 4) == 0;
  }
}

// 192-byte hit records, one per leaf SLOT (what the traversal reports), 48 floats: 0-8 the pre-edged triangle, 9-35 norm, 36-41 uv, 42 the material
// texture set (diffuse, emissive, mr, normal layers) as bits, 46 ior, 47 dielectric; a padding slot stays zero.  *has_dielectric: some triangle can refract.
static std::vector<float> pack_hit_records(const fspt_scene_desc *desc, const std::vector<float> &tris, const std::vector<uint32_t> &slot_tri, size_t n_used,
                                           const std::vector<uint32_t> &tri_set, bool *has_dielectric) {
  const uint32_t T = desc->n_tris;
  std::vector<float> shade(slot_tri.size() * 48, 0.0f);
  for (size_t sl = 0; sl < n_used; ++sl) {
    const uint32_t i = slot_tri[sl];
    if (i >= T) continue; // "-1" padding: never hit (det = 0)
    float *o = &shade[sl * 48];
    std::memcpy(o, &tris[(size_t)i * 9], 36);
    std::memcpy(o + 9, desc->norm + (size_t)i * 27, 27 * 4);
    std::memcpy(o + 36, desc->uv + (size_t)i * 6, 6 * 4);
    const float *m = desc->mat + (size_t)i * 12;
    std::memcpy(&o[42], &tri_set[i], 4);
    o[46] = m[9]; o[47] = m[10];
  }
  *has_dielectric = false;
  for (uint32_t i = 0; i < T; ++i)
    if (desc->mat[(size_t)i * 12 + 10] >= 0.0f) *has_dielectric = true;
  return shade;
}

// A new device buffer with `bytes` of host memory in it, owned by `hold`
static hipError_t upload(fspt::Hold &hold, void **dst, const void *src, size_t bytes) {
  const hipError_t e = hold.make(dst, bytes);
  return e == hipSuccess && bytes ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : e;
}

// The atlas texset_classify planned, tiled here on the host: buf[0] the single-layer images (pl.single_layers in order, each
// through tile_image), buf[1] the interleaved images (a QUAD set's four layers as one image of 16-byte texels in 4 x 2-texel
// tiles, a flat layer as its texel 0; one set at a time through one reused buffer, straight into its slice), buf[2] the table.
static hipError_t upload_atlas(fspt::Hold &hold, const fspt_scene_desc *desc, const TexSetPlan &pl, const std::vector<uint8_t> &is_const, const std::vector<uint32_t> &first, void *buf[3]) {
  const uint32_t res = desc->atlas_res;
  const size_t per_layer = (size_t)res * res;
  const uint32_t qtx = (res + 3u) / 4u, qty = (res + 1u) / 2u;
  const size_t quad_tiles = (size_t)qtx * qty;             // 128-byte tiles per interleaved image
  std::vector<uint32_t> single, tiled, quad;                 // the single-layer images, tiled; one layer; one interleaved image
  for (uint32_t l : pl.single_layers) {
    tile_image(desc->atlas + (size_t)l * per_layer * 4, res, res, tiled);
    single.insert(single.end(), tiled.begin(), tiled.end());
  }
  hipError_t e = upload(hold, &buf[0], single.data(), single.size() * 4);
  if (e == hipSuccess) e = hold.make(&buf[1], pl.quad_bytes);
  uint32_t qi = 0;
  for (size_t si = 0; si < pl.keys.size() && e == hipSuccess; ++si) {
    if (pl.kind[si] != fspt::TEXSET_QUAD) continue;
    quad.assign(quad_tiles * 32, 0u);
    for (int k = 0; k < 4; ++k) {
      const uint32_t l = pl.keys[si][k];
      const uint8_t *src = desc->atlas + (size_t)l * per_layer * 4;
      for (uint32_t jy = 0; jy < res; ++jy)
        for (uint32_t ix = 0; ix < res; ++ix) {
          uint32_t v = first[l];
          if (!is_const[l]) std::memcpy(&v, src + ((size_t)jy * res + ix) * 4, 4);
          quad[(((size_t)(jy >> 1) * qtx + (ix >> 2)) * 8 + ((jy & 1u) << 2) + (ix & 3u)) * 4 + k] = v;
        }
    }
    e = hipMemcpy((char *)buf[1] + (size_t)qi * quad_tiles * 128u, quad.data(), quad.size() * 4, hipMemcpyHostToDevice);
    qi++;
  }
  if (e == hipSuccess) e = upload(hold, &buf[2], pl.tab.data(), pl.tab.size() * 4);
  return e;
}

// The environment map (RGBE, w x h) as stored
static std::vector<uint32_t> tile_environment(const uint8_t *env, uint32_t w, uint32_t h) {
  std::vector<uint32_t> tiled;
#if FSPT_ENV_APRON
  // overlapping 8 x 4-texel tiles: tile (a, b) = texels [7a, 7a + 8) x [3b, 3b + 4), REPEAT in s, CLAMP in t (main.js:174-178)
  const uint32_t tx = (w + 6u) / 7u, ty = (h + 2u) / 3u;
  tiled.assign((size_t)tx * ty * 32u, 0u);
  for (uint32_t b = 0; b < ty; ++b)
    for (uint32_t a = 0; a < tx; ++a)
      for (uint32_t lb = 0; lb < 4; ++lb)
        for (uint32_t la = 0; la < 8; ++la) {
          const uint32_t i = (7u * a + la) % w;
          uint32_t j = 3u * b + lb;
          if (j > h - 1u) j = h - 1u;
          std::memcpy(&tiled[((size_t)b * tx + a) * 32u + lb * 8u + la], env + ((size_t)j * w + i) * 4, 4);
        }
#else
  tile_image(env, w, h, tiled); // the atlas layers' 8 x 4-texel tiles
#endif
  return tiled;
}

extern "C" {

int fspt_light_alias_table(const float *weights, uint32_t n, float *prob, uint32_t *alias) {
  if (!weights || !prob || !alias || n == 0) { fspt_set_error("fspt_light_alias_table: NULL/empty argument"); return FSPT_E_INVALID; }
  std::vector<float> p;
  std::vector<uint32_t> a;
  if (!alias_build(weights, n, p, a)) {
    fspt_set_error("fspt_light_alias_table: weights must be finite and >= 0 with a positive finite sum");
    return FSPT_E_INVALID;
  }
  std::memcpy(prob, p.data(), (size_t)n * 4);
  std::memcpy(alias, a.data(), (size_t)n * 4);
  return FSPT_OK;
}

int fspt_set_texture_interleave_budget(uint64_t bytes) {
  g_texset_budget = bytes;
  return FSPT_OK;
}

// check, topology, pack (host only: a malformed description is refused on a machine without a GPU), device, upload, install
int fspt_scene_create(const fspt_scene_desc *desc, int device, fspt_scene **out) {
  if (!desc || !out) { fspt_set_error("fspt_scene_create: NULL argument"); return FSPT_E_INVALID; }
  *out = nullptr;
  int rc = desc_check(desc);
  if (rc) return rc;
  const uint32_t N = desc->n_nodes, T = desc->n_tris, LS = desc->leaf_size;
  TreeTopology tp;
  if ((rc = tree_topology(desc->bvh, 36, N, T, tp))) return rc;
  if (tp.max_depth + 1 > 64 || tp.max_depth + 1 > fspt::wf_max_stack_entries()) {
    // the reference's stack is int[64] (tracer.fs:368); here one entry per level, in LDS (all 64 fit: 128 KB of the CU's
    // 160 KB under the 512-thread primary launch)
    fspt_set_error("BVH depth %u exceeds the traversal stack (64)", tp.max_depth);
    return FSPT_E_INVALID;
  }
  std::vector<float> quads, leaves;
  std::vector<uint32_t> slot_tri, first;
  std::vector<uint8_t> is_const;
  const TreeWords word{(const char *)desc->bvh, 36};
  const std::vector<float> nodes = pack_nodes(word, desc->bvh, N, tp);
  const bool quads_ok = pack_quads(word, desc->bvh, N, tp, nodes, quads);
  const std::vector<float> tris = pack_triangles(desc->tri, T, LS);
  pack_leaves(tris, tp.leaf_first, LS, leaves, slot_tri);
  layer_flags(desc->atlas, desc->atlas_res, desc->atlas_layers, is_const, first);
  TexSetPlan pl;
  if ((rc = texset_classify(desc->mat, T, desc->atlas_layers, desc->atlas_res, is_const.data(), first.data(), pl))) return rc;
  bool has_dielectric = false;
  const std::vector<float> shade = pack_hit_records(desc, tris, slot_tri, tp.leaf_first.size() * LS, pl.tri_set, &has_dielectric);
  if ((rc = check_device(device))) return rc; // (everything above is host work: no device, no upload)
  fspt_scene *s = new fspt_scene();
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->num_cus = prop.multiProcessorCount;
  s->device = device; s->n_tris = T; s->d.leaf_size = LS; s->has_dielectric = has_dielectric;
  fspt::Hold hold; // every device buffer, until the installs below hand them to the scene
  void *atlas[3] = {nullptr, nullptr, nullptr}, *env = nullptr, *bins = nullptr;
  uint64_t env_bytes = 0;
  hipError_t e = upload(hold, &s->nodes, nodes.data(), nodes.size() * 4);
  if (e == hipSuccess && quads_ok) e = upload(hold, &s->quads, quads.data(), quads.size() * 4);
  if (e == hipSuccess) e = upload(hold, &s->tris, leaves.data(), leaves.size() * 4);
  if (e == hipSuccess) e = upload(hold, &s->slot_tri, slot_tri.data(), slot_tri.size() * 4);
  if (e == hipSuccess) e = upload(hold, &s->shade, shade.data(), shade.size() * 4);
  if (e == hipSuccess) e = upload_atlas(hold, desc, pl, is_const, first, atlas);
  if (e == hipSuccess && desc->env) {
    const std::vector<uint32_t> tiled = tile_environment(desc->env, desc->env_w, desc->env_h);
    e = upload(hold, &env, tiled.data(), tiled.size() * 4);
    env_bytes = tiled.size() * 4;
  }
  if (e == hipSuccess) e = upload(hold, &bins, desc->bins, (size_t)desc->n_bins * 16);
  if (e != hipSuccess) { fspt_set_error("scene upload failed: %s", hipGetErrorString(e)); delete s; return FSPT_E_HIP; } // (`hold` frees the buffers)
  hold.p.clear();
  geometry_publish(s, tp, N, slot_tri.size(), quads_ok);
  atlas_install(s, atlas[0], pl.single_texels * 4, atlas[1], pl.quad_bytes, atlas[2], (uint32_t)pl.keys.size(), desc->atlas_res, desc->atlas_layers);
  fspt::environment_swap(s, env, env_bytes, desc->env_w, desc->env_h, bins, desc->n_bins);
  tree_refit_tables(desc->bvh, 36, N, T, tp, s->rf);
  *out = s;
  return FSPT_OK;
}

int fspt_scene_destroy(fspt_scene *s) {
  if (!s) return FSPT_OK;
  hipSetDevice(s->device);
  geometry_free(*s);
  hipFree(s->atlas); hipFree(s->atlas4); hipFree(s->tex_sets); hipFree(s->env); hipFree(s->bins); hipFree(s->l_alias); hipFree(s->l_rec); hipFree(s->l_p); hipFree(s->l_pick);
  hipFree(s->matte_ids[0]); hipFree(s->matte_ids[1]);
  fspt::refit_release(s);
  fspt::appearance_release(s);
  for (fspt_scene::StageOwner who : {fspt_scene::STAGE_POSE, fspt_scene::STAGE_SKIN, fspt_scene::STAGE_MESH}) fspt::deformer_release(s, who);
  for (hipEvent_t ev : s->deform_ev) if (ev) hipEventDestroy(ev);
  fspt::sky_release(s);
  fspt::lights_release(s);
  for (hipEvent_t &ev : s->lg.host_ev) if (ev) hipEventDestroy(ev);
  delete s;
  return FSPT_OK;
}

int fspt_scene_depth(const fspt_scene *s, uint32_t *depth) {
  if (!s || !depth) { fspt_set_error("fspt_scene_depth: NULL argument"); return FSPT_E_INVALID; }
  *depth = s->depth;
  return FSPT_OK;
}

int fspt_scene_light_count(fspt_scene *s, uint32_t *n_lights) {
  if (!s || !n_lights) { fspt_set_error("fspt_scene_light_count: NULL argument"); return FSPT_E_INVALID; }
  const int rc = light_table_ensure(s);
  if (rc) return rc;
  *n_lights = s->d.n_lights;
  return FSPT_OK;
}

int fspt_scene_light_table(fspt_scene *s, uint32_t *n_tris, uint32_t *n_lights, uint32_t *n_slots, float *weights, float *prob,
                           uint32_t *alias, uint32_t *tris, float *pick, uint32_t *slot_tri) {
  if (!s) { fspt_set_error("fspt_scene_light_table: NULL scene"); return FSPT_E_INVALID; }
  int rc = light_table_ensure(s);
  if (!rc) rc = light_mirrors_ensure(s);
  if (rc) return rc;
  if (n_tris) *n_tris = (uint32_t)s->l_weight.size();
  if (n_lights) *n_lights = (uint32_t)s->l_tri.size();
  if (n_slots) *n_slots = (uint32_t)s->l_pick_h.size();
  auto put = [](auto *dst, const auto &v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
  put(weights, s->l_weight); put(prob, s->l_prob); put(alias, s->l_alias_h); put(tris, s->l_tri); put(pick, s->l_pick_h);
  put(slot_tri, s->l_slot_tri);
  return FSPT_OK;
}

int fspt_light_sample_eval(fspt_scene *s, const float *in, uint32_t n, int32_t *tri, float *out) {
  if (!s || !in || !tri || !out) { fspt_set_error("fspt_light_sample_eval: NULL argument"); return FSPT_E_INVALID; }
  int rc = light_table_ensure(s);
  if (rc) return rc;
  if (s->d.n_lights == 0) { fspt_set_error("fspt_light_sample_eval: the scene has no emitter"); return FSPT_E_STATE; }
  if (n == 0) return FSPT_OK;
  // one allocation, in floats: in (10 n) | out (8 n) | entry (n)
  Staging st((size_t)n * 76);
  if (!st.ok()) return st.done("fspt_light_sample_eval");
  float *const d_in = (float *)st.base, *const d_out = d_in + (size_t)n * 10;
  int *const d_e = (int *)(d_out + (size_t)n * 8);
  st.up(d_in, in, (size_t)n * 40);
  if (st.ok()) st.e = fspt::launch_light_eval(s->d, d_in, n, d_e, d_out, nullptr);
  st.sync();
  st.down(out, d_out, (size_t)n * 32);
  st.down(tri, d_e, (size_t)n * 4);
  if ((rc = st.done("fspt_light_sample_eval"))) return rc;
  if ((rc = light_mirrors_ensure(s))) return rc;
  for (uint32_t i = 0; i < n; ++i) tri[i] = (int32_t)s->l_tri[(uint32_t)tri[i]];
  return FSPT_OK;
}

int fspt_scene_set_light_builder(fspt_scene *s, int builder) {
  if (!s) { fspt_set_error("fspt_scene_set_light_builder: NULL scene"); return FSPT_E_INVALID; }
  if (builder != FSPT_LIGHT_BUILDER_HOST && builder != FSPT_LIGHT_BUILDER_GPU) {
    fspt_set_error("fspt_scene_set_light_builder: builder must be FSPT_LIGHT_BUILDER_HOST (0) or FSPT_LIGHT_BUILDER_GPU (1), got %d", builder);
    return FSPT_E_INVALID;
  }
  int rc = check_device(s->device);
  if (!rc) rc = geometry_order_targets(s); // the targets' recorded ticks see the table they were recorded under
  if (rc) return rc;
  const int old = s->lg.builder;
  s->lg.builder = builder;
  rc = geometry_changed_lights(s);
  if (rc) s->lg.builder = old; // (the table stays dropped, as after a live-scene update whose rebuild fails: the next use builds it)
  return rc;
}

int fspt_scene_get_light_builder(fspt_scene *s, int *builder) {
  if (!s || !builder) { fspt_set_error("fspt_scene_get_light_builder: NULL argument"); return FSPT_E_INVALID; }
  *builder = s->lg.builder;
  return FSPT_OK;
}

int fspt_scene_light_build_stats(fspt_scene *s, uint64_t *bytes_d2h, uint64_t *bytes_h2d, float *ms) {
  if (!s) { fspt_set_error("fspt_scene_light_build_stats: NULL scene"); return FSPT_E_INVALID; }
  if (bytes_d2h) *bytes_d2h = s->lg.bytes_d2h;
  if (bytes_h2d) *bytes_h2d = s->lg.bytes_h2d;
  if (!ms) return FSPT_OK;
  *ms = 0.0f;
  int rc = check_device(s->device);
  if (rc) return rc;
  if (s->lg.built_by == FSPT_LIGHT_BUILDER_GPU) return fspt::lights_build_ms(s, ms);
  if (s->lg.built_by == FSPT_LIGHT_BUILDER_HOST && s->lg.host_timed) {
    HIP_TRY(hipEventSynchronize(s->lg.host_ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, s->lg.host_ev[0], s->lg.host_ev[1]));
  }
  return FSPT_OK;
}

int fspt_light_alias_table_gpu(int device, const float *weights, uint32_t n, float *prob, uint32_t *alias, float *light_p) {
  if (!weights || n == 0) { fspt_set_error("fspt_light_alias_table_gpu: NULL/empty argument"); return FSPT_E_INVALID; }
  if (n > (1u << 23)) { fspt_set_error("fspt_light_alias_table_gpu: %u entries, the GPU builder takes at most %u", n, 1u << 23); return FSPT_E_INVALID; }
  const int rc = check_device(device);
  if (rc) return rc;
  return fspt::light_alias_table_gpu_run(weights, n, prob, alias, light_p);
}

int fspt_scene_two_level_nodes(const fspt_scene *s, int *present, uint64_t *bytes) {
  if (!s) { fspt_set_error("fspt_scene_two_level_nodes: NULL argument"); return FSPT_E_INVALID; }
  if (present) *present = s->d.quads != nullptr; // (after an update: what a scene created from the same data would have)
  if (bytes) *bytes = s->d.quads ? (uint64_t)s->n_interior * fspt::QUAD_F4 * 16u : 0u;
  return FSPT_OK;
}

// texset_classify as a host-only hook (tests): set of every triangle, the sets' 12-word rows (up to cap_sets of them)
int fspt_texset_classify_eval(const float *mat, uint32_t n_tris, uint32_t n_layers, uint32_t res, const uint8_t *is_const, const uint32_t *first,
                              uint32_t *tri_set, uint32_t *n_sets, uint32_t *tab, uint32_t cap_sets) {
  if (!mat || !is_const || !first || !n_sets || n_tris == 0 || n_layers == 0 || res == 0) { fspt_set_error("fspt_texset_classify_eval: NULL/empty argument"); return FSPT_E_INVALID; }
  TexSetPlan pl;
  const int rc = texset_classify(mat, n_tris, n_layers, res, is_const, first, pl);
  if (rc) return rc;
  *n_sets = (uint32_t)pl.keys.size();
  if (tri_set) std::memcpy(tri_set, pl.tri_set.data(), (size_t)n_tris * 4);
  if (tab) std::memcpy(tab, pl.tab.data(), (size_t)std::min<uint32_t>(cap_sets, *n_sets) * 48);
  return FSPT_OK;
}

} // extern "C"
