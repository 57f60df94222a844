// fspt_internal.hpp - what the translation units of libfspt's host side share: the scene and target objects behind the
// opaque handles of include/fspt.h, the tuning defaults, and the helpers that cross file boundaries.
//   fspt_api.cpp           the target object, every entry point that is neither the scene, a scheduler, the image chain nor a live-scene update (include/fspt.h order)
//   fspt_scene.cpp         the scene object: fspt_scene_create's host layouts, the one install and release of every scene part, the emitter light table
//   fspt_scene_update.cpp  what changes a live scene or reports on such a change: refit, rebuild, pose, skin, mesh, appearance, motion origin
//   fspt_post.cpp          the image chain behind the accumulator: draw, denoiser, temporal stages, auto-exposure, bloom
//   fspt_sched_batch.cpp   the batch scheduler of the wavefront pipeline (render_wavefront) and its path state
//   fspt_sched_stream.cpp  the stream scheduler (render_stream): a fixed pool of live paths
//   fspt_multi.cpp         one frame over several devices (fspt_multi_*), tile pack / unpack, the optional RCCL exchange
//   fspt_encode.cpp        what the three encoders' host halves share: output buffers and events, delivery, stage times, the stand-alone sequence
//   scene_build.cpp        the native scene builder (OBJ / MTL / SAH BVH; no GPU)
// and the device side, declared in fspt_device.hpp:
//   fspt_kernels.hip       the renderers: the path tracer's two execution strategies, k_bvh_test, k_tile_pack, the light table
//   fspt_passes.hip        the passes no renderer calls: k_camera (every camera model), k_intersect, k_features, k_temporal_gbuffer,
//                          k_adaptive_*, the test hooks; both on fspt_traverse.hpp, fspt_surface.hpp, fspt_camera_model.hpp
//   fspt_post.hip          every kernel that reads only images: what fspt_post.cpp launches, but for k_features and k_temporal_gbuffer
//   fspt_bvh_build.hip     the GPU BVH builder;  fspt_refit.hip  in-place refit and rebuild;  fspt_pose.hip  part transforms, skinning and the vertex-position update
//   fspt_appearance.hip    in-place appearance update: the texture-set, atlas and environment layouts and the material part of the hit records
//   fspt_sky.hip           the sky generator and the environment's importance bins, built on the GPU
//   fspt_lights_build.hip  the emitter light table of a live scene, built on the GPU (opt-in)
//   fspt_jpeg.hip          the baseline JPEG encoder behind fspt_jpeg_encode, fspt_draw_jpeg and fspt_present_jpeg, and its stand-alone entries
//   fspt_png.hip           the PNG encoder behind fspt_png_encode and fspt_draw_png, and its stand-alone entries
//   fspt_exr.hip           the OpenEXR encoder behind fspt_exr_encode and fspt_draw_exr, and its stand-alone entries
//   fspt_deflate.hip       the deflate of the last two (deflate_launch);  fspt_encode_device.hpp  the offsets kernels' scan
#pragma once
#include "../../include/fspt.h"
#include "../../include/fspt_tuning.h"
#include "fspt_device.hpp"

#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

void fspt_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      fspt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
      return FSPT_E_HIP;                                                                          \
    }                                                                                             \
  } while (0)

namespace fspt { struct LightsWork; } // (fspt_lights_build.hip) the GPU light-table builder's device memory

struct fspt_scene {
  int device = 0;
  int num_cus = 256;
  fspt::DScene d{};
  void *nodes = nullptr, *quads = nullptr /* two-level nodes, or NULL */, *tris = nullptr /* leaf records */, *slot_tri = nullptr, *shade = nullptr, *atlas = nullptr, *atlas4 = nullptr, *tex_sets = nullptr, *env = nullptr, *bins = nullptr;
  uint32_t depth = 0, n_nodes = 0, n_tris = 0, n_interior = 0;
  bool has_dielectric = false; // some triangle can refract (tracer.fs:481-488: unbounded path length)
  // emitter light table, built by light_table_ensure on the first target that turns FSPT_LIGHTS_EMITTERS on;
  // device arrays behind d.light_*, host copies for fspt_scene_light_table
  size_t n_slots = 0;   // leaf slots (hit records, slot_tri entries)
  bool lights_built = false;
  void *l_alias = nullptr, *l_rec = nullptr, *l_p = nullptr, *l_pick = nullptr;
  std::vector<float> l_weight;      // per triangle (reference order)
  std::vector<uint32_t> l_tri;      // per table entry: its triangle
  std::vector<float> l_prob;        // per entry
  std::vector<uint32_t> l_alias_h;  // per entry
  std::vector<float> l_pick_h;      // per leaf slot
  std::vector<uint32_t> l_slot_tri; // per leaf slot: its triangle
  // fspt_scene_set_light_builder (fspt_lights_build.hip).  Under FSPT_LIGHT_BUILDER_GPU the d.light_* arrays
  // live in `work` (made by the first such build; l_alias .. l_pick stay NULL) and the host copies above are filled only
  // when fspt_scene_light_table or fspt_light_sample_eval asks.  A scene that never opts in allocates no device memory for it;
  // its host build creates the two events of host_ev and records them around its device work (fspt_scene_light_build_stats).
  struct LightsGpu {
    int builder = FSPT_LIGHT_BUILDER_HOST;
    fspt::LightsWork *work = nullptr;
    bool topo_valid = false;        // work's triangle-to-slot arrays match the tree (geometry_publish clears it)
    bool mirrors_valid = false;     // the host copies hold the table `work` holds
    bool timed = false;             // work's events bracket a build
    int built_by = -1;              // the builder of the last build (-1: none yet): whose events fspt_scene_light_build_stats reads
    uint64_t bytes_d2h = 0, bytes_h2d = 0; // what that build moved over the bus
    hipEvent_t host_ev[2] = {nullptr, nullptr}; // around the host builder's device work
    bool host_timed = false;
  } lg;
  // fspt_scene_update_geometry.  The scene knows its live targets (fspt_target_create / _destroy), so that an
  // update is ordered against their recorded ticks and their streams.  `rf` is what a refit needs of the reference tree and
  // fspt_scene_create no longer has when it returns: host memory until the first update, which makes the device copies
  // (fspt_refit.hip) - a scene that is never updated allocates nothing for it on the GPU.
  std::vector<fspt_target *> targets;
  enum StageOwner { STAGE_NONE, STAGE_POSE, STAGE_SKIN, STAGE_MESH };
  struct Refit {
    static const uint32_t NO_DST = 0xFFFFFFFFu;
    bool ok = false;                  // the leaves' triStarts are distinct and tile [0, n_tris); every node has one parent
    // per leaf record: first triangle, triangles owned ([first, next larger first or n_tris)), and where its box lives:
    // box slot 2 * (parent's native index) + side in `nodes` (NO_DST: the root, whose box is stored nowhere)
    std::vector<uint32_t> leaf_first, leaf_cnt, leaf_dst;
    // interior nodes but the root, deepest level first: (own native index, box slot); lvl_off[k] .. lvl_off[k + 1] = level k
    std::vector<uint32_t> lvl_nodes, lvl_off;
    // per reference node, pre-order (fspt_scene_sah_cost): box slot, triangles owned (interior: NO_DST)
    std::vector<uint32_t> node_dst, node_owned;
    // device side, made by the first update
    uint32_t *d_leaf = nullptr;       // leaf_first | leaf_cnt | leaf_dst
    uint32_t *d_lvl = nullptr;        // lvl_nodes
    uint32_t *d_flag = nullptr;       // [0] non-finite input seen, [1] the two-level nodes are not usable
    float *stage = nullptr;           // the staging array, tri 9 T | norm 27 T: a host form's upload or a deformer's output
    StageOwner stage_owner = STAGE_NONE; // whose accepted frame `stage` holds (stage_disown; granted by the update path alone)
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.0f;             // kernels of the last update, first to last
    uint32_t last_launches = 0;
  } rf;
  // the most recent fspt_scene_rebuild_geometry (fspt_scene_last_rebuild_ms)
  struct Rebuild { float build_ms = 0.0f, install_ms = 0.0f, host_ms = 0.0f; uint32_t launches = 0, readbacks = 0; } rb;
  // motion origin (fspt_scene_motion_begin): floats 0-8 of every leaf slot's hit record as they were at the
  // last motion_begin (n_slots x 36 bytes; NULL: the scene is static).  A refit leaves it alone, a rebuild permutes it.
  void *motion = nullptr;
  // bytes of atlas (single-layer images), atlas4 (interleaved images) and env as laid out (fspt_scene_read_appearance)
  uint64_t atlas_bytes = 0, atlas4_bytes = 0, env_bytes = 0;
  // fspt_scene_update_materials / _environment (fspt_appearance.hip).  `raw` is the atlas the most recent
  // update_materials call carried, as given (RGBA8, layer-major): what a later call with atlas == NULL lays out again.  Like
  // rf.stage it is made by the first such call - a scene whose appearance is never updated allocates nothing for it.
  struct Appearance {
    void *raw = nullptr;
    uint32_t raw_res = 0, raw_layers = 0;
    std::vector<uint8_t> is_const;  // per layer of `raw` (k_ap_layer_const's answer, kept with it)
    std::vector<uint32_t> first;    // per layer: its texel 0
    std::vector<std::array<uint32_t, 4>> keys; // per texture set of the last materials call: its four layers (fspt_scene_patch_textures)
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.0f;           // kernels of the last update, first to last
    uint32_t last_launches = 0;
    uint64_t last_uploaded = 0;     // host -> device bytes of the last update
  } ap;
  // fspt_scene_set_pose / fspt_scene_update_transforms (fspt_pose.hip): per triangle (current leaf order) a part
  // id and the rest mesh, on the device; a rebuild permutes them with the triangles.  A scene that never sets a pose
  // allocates nothing for it; the posed arrays go to rf.stage, which an accepted frame owns as STAGE_POSE.
  struct Pose {
    uint32_t *part = nullptr;       // n_tris ids < n_parts (NULL: no pose)
    float *rest = nullptr;          // n_tris x 9 rest vertices | n_tris x 27 rest normTex records when has_norm
    bool has_norm = false;
    uint32_t n_parts = 0;
    float *mats = nullptr;          // the last call's n_parts x 30 floats (a | D | N); grows as needed
    uint32_t mats_cap = 0;          // parts it holds
    float last_ms = 0.0f;           // k_pose_transform of the last call
  } pose;
  // fspt_scene_set_skin / fspt_scene_update_skin (fspt_pose.hip): per triangle corner (current leaf order) four
  // joint ids and weights, the rest mesh and the morph targets, on the device; a rebuild permutes them with the triangles.
  // A scene that never sets a skin allocates nothing for it; the skinned arrays go to rf.stage (STAGE_SKIN).
  struct Skin {
    uint16_t *joints = nullptr;     // n_tris x 3 x 4 ids < n_joints (NULL: no skin)
    float *weights = nullptr;       // n_tris x 3 x 4
    float *rest = nullptr;          // n_tris x 9 rest vertices | n_tris x 27 rest normTex records when has_norm
    float *morph = nullptr;         // n_morph x n_tris x 9 deltas (NULL: n_morph == 0)
    float *morph_norm = nullptr;    // n_morph x n_tris x 27 deltas, or NULL
    float *frame = nullptr;         // the host form's upload: n_joints x 12 floats | n_morph weights
    bool has_norm = false;
    uint32_t n_joints = 0, n_morph = 0;
    float last_ms = 0.0f;           // k_skin_transform of the last call
  } skin;
  // fspt_scene_set_mesh / fspt_scene_update_vertices (fspt_pose.hip): an indexed mesh whose normal frames are
  // derived from new vertex positions every frame.  Per triangle (current leaf order; a rebuild permutes them) the corner
  // indices, three uv constants, a face id and the rest copy of the static ones; per vertex the incident faces by face id
  // (a rebuild leaves them alone).  A scene that never sets a mesh allocates nothing for it; the derived arrays go to rf.stage (STAGE_MESH).
  struct Mesh {
    uint32_t *vertex = nullptr;     // n_tris x 3 indices < n_vertices, or 3 x FSPT_MESH_STATIC (NULL: no mesh)
    double *cst = nullptr;          // n_tris x 3: du1[1], du0[1], r of calcTangents, float64 (static: 0)
    uint32_t *face = nullptr;       // n_tris: the face id (leaf position at set_mesh), bit 31 = smooth
    float *rest = nullptr;          // n_tris x 9 | n_tris x 27 rest copy, or NULL when no triangle is static
    uint32_t *adj_off = nullptr;    // n_vertices + 1: a vertex's span in adj_face (NULL: no triangle is smooth)
    uint32_t *adj_face = nullptr;   // per incident corner a face id, ascending rank of the face
    double *fnorm = nullptr;        // scratch, n_tris x 3 by face id: the face normals (NULL: no triangle is smooth)
    double *vnorm = nullptr;        // scratch, n_vertices x 3: total * (1 / count)
    float *pos = nullptr;           // the host form's upload: n_vertices x 3
    uint32_t n_vertices = 0, n_adj = 0; // n_adj = adj_off[n_vertices], the entries of adj_face
    float last_ms = 0.0f;           // the derive kernels of the last call, first to last
    float pass_ms[3] = {0.0f, 0.0f, 0.0f}; // k_mesh_faces | k_mesh_vertex_normals | k_mesh_smooth_frames (a flat-only mesh: the first alone)
    uint32_t last_launches = 0;
  } mesh;
  // the events that time a deformer's kernels, whichever it is: first, last, and between the mesh's three passes.  Made by the
  // first update_transforms / _skin / _vertices, destroyed with the scene.
  hipEvent_t deform_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // fspt_scene_update_sky / _environment_auto / _environment_device (fspt_sky.hip): the last such call
  struct Sky {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float sky_ms = 0.0f, bins_ms = 0.0f, tile_ms = 0.0f; // the generator | radiance, table, tree and the n_bins read-back | the tiling
    uint32_t launches = 0, readbacks = 0, n_bins = 0;
  } sky;
  // fspt_scene_set_matte_ids / _manifest: per kind (FSPT_MATTE_*) one id per triangle (current leaf order; a
  // rebuild permutes it), on the device, NULL: the kind has no ids; the manifest's bytes stay on the host, for a file header.
  uint32_t *matte_ids[2] = {nullptr, nullptr};
  std::string matte_manifest[2];
};
// Material texture sets: what fspt_scene_create and fspt_scene_update_materials derive from matTex's layer ids and
// the per-layer "every texel equal" flags - the sets in first-appearance order, each triangle's set, a set's form under the
// interleaving budget, where the single-layer images go, and the 12-word table rows.  Host only; one statement for both.
struct TexSetPlan {
  std::vector<std::array<uint32_t, 4>> keys; // per set: diffuse, emissive, mr, normal layer
  std::vector<uint32_t> tri_set;             // per triangle
  std::vector<uint32_t> kind;                // per set: fspt::TEXSET_*
  std::vector<int64_t> layer_base;           // per layer: base of its single-layer image in 128-byte tiles (-1: not stored)
  std::vector<uint32_t> single_layers;       // the layers stored as single-layer images, in storage order
  std::vector<uint32_t> tab;                 // 12 words per set (fspt_device.hpp)
  uint64_t quad_bytes = 0;                   // bytes of the interleaved images (a QUAD set's base: tab[12 si + 1] tiles)
  uint64_t single_texels = 0;                // texels of the single-layer images, tiled
};
uint32_t texset_layer_of(float id, uint32_t n_layers); // clamp(floor(id + 0.5), 0, n_layers - 1), NaN -> 0
// is_const / first: n_layers entries.  FSPT_E_INVALID: the single-layer images exceed 2^32 tiles.
int texset_classify(const float *mat, uint32_t n_tris, uint32_t n_layers, uint32_t res, const uint8_t *is_const, const uint32_t *first, TexSetPlan &pl);
int geometry_order_targets(fspt_scene *s);  // (fspt_api.cpp) orders a scene-changing call against every target, leaves the device idle
int geometry_changed_lights(fspt_scene *s); // (fspt_scene.cpp) releases the emitter light table and rebuilds it if a target uses it
// What fspt_scene_create derives from the reference tree's three integer words per node (left, right, triStart; a node
// with triStart > -1 is a leaf) and nothing else: shared with fspt_scene_rebuild_geometry, which gets its words from the
// GPU builder.  `words` + i * stride = node i's words (any alignment).
struct TreeTopology {
  std::vector<int32_t> ref;         // per reference node: its native index (interior: breadth-first top, then treelets) or ~(leaf record)
  std::vector<uint32_t> leaf_first; // per leaf record: its first triangle
  std::vector<uint32_t> depth;      // per reference node (root 0)
  uint32_t n_interior = 0, max_depth = 0;
};
int tree_topology(const void *words, size_t stride_bytes, uint32_t N, uint32_t T, TreeTopology &tp); // validates; FSPT_E_INVALID
void tree_refit_tables(const void *words, size_t stride_bytes, uint32_t N, uint32_t T, const TreeTopology &tp, fspt_scene::Refit &R);
// (fspt_scene.cpp) The one install and one release per scene part, shared by fspt_scene_create and the live-scene updates (the
// environment's: fspt::environment_swap below).  geometry_publish: every geometry field of s->d and the scene's counts, from s->nodes /
// quads / tris / slot_tri / shade (set by the caller) and their tree.  geometry_free: those five and s->motion.  atlas_install frees the old.
void geometry_publish(fspt_scene *s, const TreeTopology &tp, uint32_t n_nodes, size_t n_slots, bool quads_ok);
inline void geometry_free(fspt_scene &s) { for (void **p : {&s.nodes, &s.quads, &s.tris, &s.slot_tri, &s.shade, &s.motion}) { hipFree(*p); *p = nullptr; } }
void atlas_install(fspt_scene *s, void *n_atlas, uint64_t atlas_bytes, void *n_atlas4, uint64_t atlas4_bytes, void *n_tab, uint32_t n_sets, uint32_t res, uint32_t layers);
namespace fspt { // fspt_refit.hip
int refit_prepare(fspt_scene *s);  // the device copies of s->rf (idempotent)
void refit_release(fspt_scene *s);
// tri / norm (may be NULL): device memory.  *finite = 0: a non-finite value, nothing written.  *quads_ok: the rebuilt
// two-level nodes (s->quads, must be allocated) are usable.  Runs on the NULL stream and waits for it.
int refit_run(fspt_scene *s, const float *tri, const float *norm, int *finite, int *quads_ok);
// k_refit_check alone (s->rf prepared): *finite = 0 when a word of tri / norm (device memory) is inf or NaN
int refit_check(fspt_scene *s, const float *tri, const float *norm, int *finite);
// fspt_scene_rebuild_geometry's device side: a new tree over tri (device memory, the scene's leaf order), built
// by fspt_bvh_build.hip's kernels and installed in `s`; the scene is untouched unless FSPT_OK comes back.  The caller has
// ordered the call against the targets, prepared s->rf and checked tri / norm.  order_out: NULL, host or device memory.
int rebuild_run(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out, bool order_on_device);
// fspt_appearance.hip: the callers have validated their arguments and ordered the call against the targets.
// tx (atlas NULL): the raw atlas is packed on the device from tx->p - all of it, or, with layer_ids, those
// layers of a copy of the retained one (mat is then ignored: the scene's current materials are read back) - and becomes the
// retained atlas like an uploaded one.  fn names the entry in errors.
struct ApTextures { const fspt_texture_pack *p; bool on_device; const uint32_t *layer_ids; const char *fn; };
int appearance_materials(fspt_scene *s, const float *mat, const float *uv, const uint8_t *atlas, uint32_t res, uint32_t layers, const ApTextures *tx = nullptr);
int appearance_environment(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h, const uint32_t *bins, uint32_t n_bins);
void appearance_release(fspt_scene *s);
// device buffers of a transaction: freed unless taken
struct Hold {
  std::vector<void *> p;
  ~Hold() { clear(); }
  void clear() { for (void *q : p) hipFree(q); p.clear(); }
  hipError_t make(void **dst, size_t bytes) {
    *dst = nullptr;
    const hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
    if (e == hipSuccess) p.push_back(*dst); else *dst = nullptr;
    return e;
  }
  void take(void *q) { p.erase(std::remove(p.begin(), p.end(), q), p.end()); }
};
inline int ap_fail(const char *fn, hipError_t e) {
  (void)hipGetLastError();
  fspt_set_error("%s: %s (scene unchanged)", fn, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
}
// fspt_texpack.hip.  texpack_launch: a checked description's layers into `raw` (device memory, res^2 texels per
// layer; layer l, or layer_ids[l]) on `st`: uploads the records and - host form - the sources into buffers of `hold`, records
// ev_begin (may be NULL) and launches k_tex_resample; does not wait.  atlas_pack_run: fspt_atlas_pack_gpu's device side on the
// current device; atlas_pack_times: its last split (host clock around the uploads and the read-back, events around the kernel).
hipError_t texpack_launch(Hold &hold, const fspt_texture_pack *p, bool on_device, const uint32_t *layer_ids, uint32_t *raw, hipStream_t st,
                          hipEvent_t ev_begin, uint64_t *uploaded, uint32_t *launches);
int atlas_pack_run(const fspt_texture_pack *p, uint8_t *atlas_out);
void atlas_pack_times(float *upload_ms, float *kernel_ms, float *readback_ms);
// the environment's last two steps, shared by fspt_scene_update_environment and the GPU sky entries (fspt_sky.hip): the
// tiled form of a raw w x h RGBE map (device memory; dst holds env_tiled_texels words), and the swap of the scene's
// environment and bins for new device buffers (n_env NULL = no map), which frees the old ones
size_t env_tiled_texels(uint32_t w, uint32_t h);
hipError_t env_tile_launch(const uint32_t *raw, uint32_t w, uint32_t h, uint32_t *dst, hipStream_t st);
void environment_swap(fspt_scene *s, void *n_env, uint64_t env_bytes, uint32_t w, uint32_t h, void *n_bins_d, uint32_t n_bins);
// fspt_sky.hip.  Arguments are validated by the callers; `p` has a unit sun_dir.
// sky_generate_run / env_bins_run / env_box_sums_run: the stand-alone entries' device side on the current device, host pointers.
int sky_generate_run(const fspt_sky_params *p, uint32_t w, uint32_t h, uint8_t *rgbe_out, float *linear_out);
int env_bins_run(const uint8_t *rgbe, uint32_t w, uint32_t h, uint32_t *bins, uint32_t cap, uint32_t *n_bins);
int env_box_sums_run(const uint8_t *rgbe, uint32_t w, uint32_t h, const uint32_t *boxes, uint32_t n, double *out);
// The scene entries' transaction (the call is ordered against the targets): the raw map is `env` (host memory, or the scene's
// device memory when env_on_device) or, with `sky`, generated; bins are built from it on the device, it is tiled, and only
// then are the scene's buffers swapped and s->sky filled in.
int environment_gpu(fspt_scene *s, const char *fn, const uint8_t *env, bool env_on_device, const fspt_sky_params *sky, uint32_t w, uint32_t h);
void sky_release(fspt_scene *s);
// fspt_lights_build.hip.  lights_build_gpu: light_table_ensure's work under FSPT_LIGHT_BUILDER_GPU, on the NULL
// stream and waited for - the table from the scene's device arrays into s->lg.work and s->d.light_*, one 8-byte read.
// lights_mirrors_gpu: the host copies of that table.  lights_build_ms: the GPU time of the last such build (0: none).
// light_alias_table_gpu_run: fspt_light_alias_table_gpu's device side on the current device, host pointers.
int lights_build_gpu(fspt_scene *s);
int lights_mirrors_gpu(fspt_scene *s);
int lights_build_ms(fspt_scene *s, float *ms);
void lights_release(fspt_scene *s);
int light_alias_table_gpu_run(const float *weights, uint32_t n, float *prob, uint32_t *alias, float *light_p);
// fspt_encode.cpp: what the host halves of the three encoders below share.  EncCommon: the part of an encoder's
// device memory that does not depend on the format - the output buffers, which only grow and outlive a change of the
// parameters, the events around the three stages of the last launch, and `work`, the owner of every buffer made for the
// current plan (the encoders keep typed pointers into it, made by enc_make and good while `valid`).  EncFormat: what delivery and the
// fspt_*_last_ms entries know of a format.
struct EncCommon {
  bool valid = false; // `work` holds the buffers of the encoder's plan
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t *out[2] = {nullptr, nullptr};
  size_t out_bytes = 0; // of every out[k] that is there
  Hold work;
};
struct EncFormat {
  const char *noun;   // what a buffer too small is told it cannot hold: "frame" or "file"
  uint32_t len_bytes; // the device's length word: 4 or 8 bytes
  float ms[3];        // the stage times of the last stand-alone encode
  uint64_t bus_bytes; // what its delivery brought to the host: the file and its length word
};
extern EncFormat g_jpeg_format, g_png_format, g_exr_format;
hipError_t enc_ensure_out(EncCommon &c, int n_out, size_t out_bytes); // n_out buffers of at least out_bytes, and the events; nothing of `c` may be in use
void enc_replan(EncCommon &c);                                        // the work buffers go: a new plan makes its own
void enc_release(EncCommon &c);
// *bytes_out = n; cap < n: FSPT_E_INVALID, out untouched; else n bytes of dev copied on st, which is waited for
int enc_deliver(const uint8_t *dev, uint64_t n, uint8_t *out, size_t cap, size_t *bytes_out, hipStream_t st, const char *fn, EncFormat &f);
// what every blocking entry ends with: the length word at len_dev is read on st, st is waited for, then enc_deliver
int enc_collect(const void *len_dev, const uint8_t *dev, uint8_t *out, size_t cap, size_t *bytes_out, hipStream_t st, const char *fn, EncFormat &f);
int enc_last_ms(const EncFormat &f, const char *fn, float ms[3], uint64_t *bus_bytes);
void enc_note_ms(const EncCommon &c, EncFormat &f); // the stage times of a finished launch, for fspt_*_last_ms
// A stand-alone entry behind its NULL checks and its plan: the device, `ensure`, `launch` (uploads what is on the host into
// buffers of the Hold, then launches), `collect` - whose stage times are noted when it returns FSPT_OK or FSPT_E_INVALID -
// and the release of `c`.  The stage-one forms have nothing to collect: their launch copies back, and they pass nullptr.
int enc_enter(const char *fn, int device);                   // a device at all, then this one
int enc_fail(const char *fn, hipError_t err);                // the device is drained, the error set: FSPT_E_NOMEM or FSPT_E_HIP
template <class Ensure, class Launch, class Collect>
int enc_run(const char *fn, int device, EncCommon &c, EncFormat &f, Ensure ensure, Launch launch, Collect collect) {
  int rc = enc_enter(fn, device);
  if (rc) return rc;
  Hold hold;
  hipError_t err = ensure();
  if (err == hipSuccess) err = launch(hold);
  if (err != hipSuccess) rc = enc_fail(fn, err);
  else if constexpr (!std::is_same<Collect, std::nullptr_t>::value) {
    rc = collect();
    if (rc == FSPT_OK || rc == FSPT_E_INVALID) enc_note_ms(c, f);
  }
  enc_release(c);
  return rc;
}
// a work buffer of the plan being made in its typed pointer, which stays NULL when the plan does not want it or an earlier one failed
template <class P>
void enc_make(EncCommon &c, hipError_t &err, P *&ptr, size_t bytes, bool wanted = true) {
  ptr = nullptr;
  if (wanted && err == hipSuccess) err = c.work.make((void **)&ptr, bytes);
}
hipError_t enc_upload(Hold &hold, const void *host, size_t bytes, const void **dev); // *dev: a buffer of the Hold with the host's bytes
// fspt_*_bound: plan(pl) validates; no device touched
template <class Plan, class F>
int enc_bound(const char *fn, size_t *bytes, F plan) {
  if (!bytes) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  Plan pl;
  const int rc = plan(pl);
  if (rc == FSPT_OK) *bytes = pl.bound;
  return rc;
}
// fspt_jpeg.hip: the baseline JPEG encoder.  JpegPlan: what follows from a size and checked parameters, on the
// host.  JpegEnc: the device memory of one encoder - the header and divisors of its plan, the work buffers, up to two
// output buffers - owned by a target (fspt_draw_jpeg, fspt_present_jpeg) or by one stand-alone call.
static const uint32_t JPEG_HEADER_BYTES = 629u; // SOI .. SOS: the same for every size and setting
struct JpegPlan {
  uint32_t w, h, quality, sub, ri; // ri: MCUs per restart interval as DRI carries it
  uint32_t mw, mh, n_mcu, bpm, n_blocks, n_int;
  size_t slot_bytes; // an interval's scratch slot
  size_t bound;      // no file of this plan is longer
};
struct JpegEnc {
  JpegPlan pl{};
  EncCommon c;
  uint8_t *cfg = nullptr;     // 128 uint16 divisors | the header
  int16_t *coef = nullptr;    // stage one's output
  uint8_t *scratch = nullptr; // n_int slots
  uint32_t *len = nullptr, *off = nullptr; // per interval: bytes | where it lands; off[n_int] = the file's length
};
int jpeg_check_params(const fspt_jpeg_params *prm, const char *fn); // the parameters alone (a target's entries: before the handle is looked at)
int jpeg_plan(const fspt_jpeg_params *prm, uint32_t w, uint32_t h, const char *fn, JpegPlan &pl); // validates: FSPT_E_INVALID, no device touched
size_t jpeg_bound_max(uint32_t w, uint32_t h);                                                    // the largest bound of any parameters
hipError_t jpeg_ensure(JpegEnc &e, const JpegPlan &pl, int n_out, size_t out_bytes);              // nothing of `e` may be in use
hipError_t jpeg_launch_blocks(JpegEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st);
hipError_t jpeg_launch(JpegEnc &e, const uint32_t *rgba, int bottom_up, int slot, hipStream_t st); // no host read, no synchronisation
int jpeg_collect(JpegEnc &e, int slot, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn);
// fspt_png.hip: the PNG encoder.  PngPlan: what follows from a size and checked parameters, on the host.
// PngEnc: the device memory of one encoder - the signature and IHDR of its plan, the filtered stream, a scratch slot and a
// record (bytes, CRC-32, Adler pair) per chunk, one output buffer - owned by a target (fspt_draw_png) or by one stand-alone call.
static const uint32_t PNG_HEADER_BYTES = 33u; // signature and IHDR
struct PngPlan {
  uint32_t w, h, channels, filter, cb; // cb: the bytes of the filtered stream per chunk
  uint32_t row_bytes, n_chunks;
  size_t stream_bytes;
  size_t slot_bytes; // a chunk's scratch slot
  size_t bound;      // no file of this plan is longer
};
struct PngEnc {
  PngPlan pl{};
  EncCommon c;
  uint8_t *cfg = nullptr;     // the header
  uint8_t *stream = nullptr;  // stage one's output
  uint8_t *scratch = nullptr; // n_chunks slots
  uint32_t *meta = nullptr, *off = nullptr; // per chunk: 4 words | where its IDAT lands; off[n_chunks + 1] = the file's length
};
int png_check_params(const fspt_png_params *prm, const char *fn); // the parameters alone (a target's entry: before the handle is looked at)
int png_plan(const fspt_png_params *prm, uint32_t w, uint32_t h, bool for_device, const char *fn, PngPlan &pl); // validates: FSPT_E_INVALID, no device touched; for_device: the file must stay below 4 GiB
size_t png_bound_max(uint32_t w, uint32_t h, uint32_t cb);                             // the largest bound of any parameters with chunks of cb
hipError_t png_ensure(PngEnc &e, const PngPlan &pl, int n_out, size_t out_bytes);     // nothing of `e` may be in use
hipError_t png_launch_filter(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st);
hipError_t png_launch(PngEnc &e, const uint32_t *rgba, int bottom_up, hipStream_t st); // no host read, no synchronisation
int png_collect(PngEnc &e, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn);
// fspt_deflate.hip: the deflate both encoders share (k_deflate): `stream` is n_seg segments of seg_bytes one behind the
// other (the last holds what is left of stream_bytes), each one zlib stream of its own, cut into chunks of cb from its first
// byte: chunk k is chunk k % cps of segment k / cps.  The first chunk of a segment carries the zlib header, the last one
// BFINAL; a chunk's bytes land in its scratch slot and (bytes, CRC-32 of its IDAT when `crc`, Adler A, B) in its 4 words of
// `meta`.  PNG is one segment: seg_bytes = stream_bytes, cps = n_chunks.
static const uint32_t DEFLATE_META = 4u, DEFLATE_CHUNK_MIN = 256u, DEFLATE_CHUNK_MAX = 32768u, DEFLATE_ADLER = 65521u;
static const uint32_t DEFLATE_CHUNK_EXTRA = 12u; // beyond a chunk's own bytes: the zlib header (2), a stored header (5) and the empty stored block (5) at the most
struct DeflateP {
  const uint8_t *stream;
  size_t stream_bytes, seg_bytes;
  uint32_t cb, cps, crc;
  uint8_t *scratch;
  size_t slot_bytes;
  uint32_t *meta;
};
size_t deflate_slot_bytes(uint32_t cb);
hipError_t deflate_launch(const DeflateP &p, uint32_t n_chunks, hipStream_t st);
// fspt_exr.hip: the OpenEXR encoder.  ExrPlan: what follows from a size and checked parameters, on the host.
// ExrEnc: the device memory of one encoder - the header of its plan, the predicted stream and the raw bytes of every block,
// the deflate's slots and records, a record per block, one output buffer - owned by a target (fspt_draw_exr) or by one
// stand-alone call.
// The Cryptomatte layers add twelve FLOAT channels per kind and header attributes that carry the manifests, so
// the header is sized per plan; a plan with a matte layer runs the second instantiation of k_exr_rows, every other plan today's.
static const uint32_t EXR_MAX_CHANNELS = 35u, EXR_MANIFEST_MAX = 1u << 20;
struct ExrChannel { uint32_t src, bytes, off; }; // src: 0..3 = the rgba float, 4..11 = the feature float src - 4, 12..23 / 24..35 = float src - 12 / - 24 of the object / material ranks; off: in units of w bytes within a scanline
struct ExrMattes { const float4 *ranks[2]; const char *manifest[2]; size_t manifest_len[2]; }; // by FSPT_MATTE_*; ranks in device memory (the plan reads the manifests alone)
struct ExrPlan {
  uint32_t w, h, compression, pixel_type, layers, cb, form;
  uint32_t n_ch, px_bytes, lpb, n_blocks, cps, n_chunks, hdr_len;
  ExrChannel ch[EXR_MAX_CHANNELS]; // in file order
  size_t line_bytes, block_bytes, data_bytes; // a scanline | a full block | every block, uncompressed
  size_t slot_bytes, bound;
  std::vector<uint8_t> hdr; // hdr_len bytes
};
struct ExrEnc {
  ExrPlan pl{};
  EncCommon c;
  uint8_t *cfg = nullptr;                    // the header, then (16-byte aligned) the channels
  uint8_t *stream = nullptr, *raw = nullptr; // the deflate's input | the same blocks as they are (form 1)
  uint8_t *scratch = nullptr;
  uint32_t *meta = nullptr, *chunk_off = nullptr; // per chunk: 4 words | where its bytes start in its block's data
  uint64_t *blk = nullptr;                        // per block: the block's offset in the file, (size << 32 | Adler-32); blk[2 n_blocks] = the file's length
};
// validates: FSPT_E_INVALID, no device touched.  crypto: the entry accepts the Cryptomatte layer bits; m (or NULL: none): their manifests
int exr_plan(const fspt_exr_params *prm, uint32_t w, uint32_t h, bool for_device, const char *fn, ExrPlan &pl, bool crypto = false, const ExrMattes *m = nullptr);
hipError_t exr_ensure(ExrEnc &e, const ExrPlan &pl, size_t out_bytes);                 // nothing of `e` may be in use
hipError_t exr_launch(ExrEnc &e, const float4 *rgba, const float4 *feat, int bottom_up, hipStream_t st, const ExrMattes *m = nullptr); // no host read, no synchronisation; m: the ranks of the plan's matte layers
int exr_collect(ExrEnc &e, hipStream_t st, uint8_t *out, size_t cap, size_t *bytes_out, const char *fn);
// fspt_pose.hip: the three deformers that fill s->rf.stage (tri 9 T | norm 27 T) - part transforms, skinning
// (8.16), the vertex-position update (8.24).  Set, update, read, release and rebuild are stated once for all of them
// (fspt_scene_update.cpp, rebuild_run); what is a deformer's own is its frame upload and its launch, below.
// A deformer's device arrays, once, as data: `rows` rows of span[0] + span[1] words in each of `slices` slices.  An array
// that follows the triangles (rows = n_tris) is permuted span by span and slice by slice when a rebuild changes the leaf
// order: rest = 9 T | 27 T in one allocation is two spans, a morph array one slice per target.  *p NULL: not there.
struct DeformArray { void **p; size_t rows; uint32_t span[2]; size_t slices; bool follows; };
std::vector<DeformArray> deform_arrays(fspt_scene::Pose &P, size_t T);
std::vector<DeformArray> deform_arrays(fspt_scene::Skin &K, size_t T);
std::vector<DeformArray> deform_arrays(fspt_scene::Mesh &M, size_t T);
inline std::vector<DeformArray> deform_arrays(fspt_scene *s, fspt_scene::StageOwner who) {
  return who == fspt_scene::STAGE_POSE ? deform_arrays(s->pose, s->n_tris) : who == fspt_scene::STAGE_SKIN ? deform_arrays(s->skin, s->n_tris) : deform_arrays(s->mesh, s->n_tris);
}
uint64_t deform_bytes(const std::vector<DeformArray> &arrays); // what the arrays that are there hold
void mesh_release(fspt_scene::Mesh &M);                        // (a mesh without a scene: fspt_mesh_frames_eval)
void deformer_release(fspt_scene *s, fspt_scene::StageOwner who); // frees its arrays, resets it, takes the staging array from it
// The staging array is about to be written, or `only`'s arrays to change: no frame (of `only`) is handed out any more.
inline void stage_disown(fspt_scene *s, fspt_scene::StageOwner only = fspt_scene::STAGE_NONE) {
  if (only == fspt_scene::STAGE_NONE || s->rf.stage_owner == only) s->rf.stage_owner = fspt_scene::STAGE_NONE;
}
// The frame uploads (host forms; the device of the scene is current): pose_upload grows pose.mats as needed and takes
// n_parts x 30 floats (a | D | N); skin_upload takes n_joints x 12 floats | n_morph weights into skin.frame.
// The launches: a deformer's kernels into s->rf.stage (allocated) on the NULL stream, no wait; they return the kernels
// launched.  skin_run: xf (16-byte aligned) and morph_w are device memory.  mesh_run needs no scene: the derive kernels of
// M for T triangles from pos (n_vertices x 3 floats, device memory) into stage; `between`: two events recorded between the passes.
int pose_upload(fspt_scene::Pose &P, const float *mats_host);
uint32_t pose_run(fspt_scene *s);
int skin_upload(fspt_scene::Skin &K, const float *xf, const float *morph_w);
uint32_t skin_run(fspt_scene *s, const float *xf, const float *morph_w);
uint32_t mesh_run(const fspt_scene::Mesh &M, uint32_t T, const float *pos, float *stage, hipEvent_t *between = nullptr);
int f64_probe_run(int op, const double *a, const double *b, uint32_t n, double *out);
// the joint table's form: 0 = read from global memory, 1 = staged once per block in LDS when it fits SKIN_LDS_MAX_BYTES
extern int g_skin_form;
#ifndef SKIN_FORM
#define SKIN_FORM 0
#endif
static const size_t SKIN_LDS_MAX_BYTES = 64u << 10; // 1 365 joints
}
int light_table_ensure(fspt_scene *s); // (fspt_scene.cpp) builds the table once; FSPT_OK when it exists
#ifndef FSPT_LIGHTS_ENV_Q_MAX
#define FSPT_LIGHTS_ENV_Q_MAX 0.875f // largest q of a scene with an environment map (fspt_sched_batch.cpp fill_trace_params)
#endif

static const int WF_ARRAYS = 15;
#ifndef FSPT_TAIL_SLICE_LARGE
#define FSPT_TAIL_SLICE_LARGE 16u // scenes of >= 2^18 triangles (fspt_sched_batch.cpp wf_tail_slice)
#endif
#ifndef FSPT_TAIL_SLICE_SMALL
#define FSPT_TAIL_SLICE_SMALL 32u
#endif
#ifndef FSPT_SUSP_BUDGET
#define FSPT_SUSP_BUDGET 24 // profiles/r03/ab_trace_suspend_budget.log: 0 / 16 / 24 / 32 / 48 -> 3 883 / 3 938 / 3 940 / 3 935 / 3 921 Msamples/s in 20-step regions (same box, twice)
#endif
static const uint32_t ST_DEFAULT_SUSP_BUDGET = FSPT_SUSP_BUDGET;
// Library's choice of the node form (fspt_target::node_form = -1), per kernel class.  Measured (profiles/r05/ab_two_level_*.log,
// one box, interleaved): the two-level nodes LOSE in every regime they were built for - tail kernel 0.037 -> 0.040-0.045 ms
// per tick (C2, 20 ticks), 0.82 -> 0.80-0.92 (single tick), 0.125 -> 0.145 (1 M triangles); trace launches 0.170 -> 0.21 /
// 0.215 -> 0.26; primary 0.127 -> 0.138 / 0.176 -> 0.193.  Halving the dependent round trips buys nothing because a step's
// time is not a cache-miss latency: it is the CU's vector-memory front end working through the lane-requests of all its
// resident waves (16 waves x 4 instructions x (4.6 + 0.63 x active lanes) cycles = the 1 900 clocks per step round-4
// measured in the tail kernel), and a two-level fetch issues 8 requests where the walk needs 4 or 8.  The ADAPTIVE tail
// (two-level nodes only once a wave's list is used up - the launch's end phase, a few lanes walking dependent chains on a
// mostly idle chip) loses as well: 0.037-0.039 -> 0.038-0.040 / 0.80-0.82 -> 0.83-0.88 / 0.120-0.128 -> 0.136-0.145
// (ab_tail_adaptive_*.log) - the second node array is touched by that phase alone, so its lines come from the Infinity Cache
// or HBM where the 64-byte nodes, which every trace launch keeps warm, hit the L2: half as many fetches at twice the
// latency.  So: everything off; the form stays selectable (fspt_target_set_node_form) and tested.
#ifndef FSPT_WIDE_PRIMARY
#define FSPT_WIDE_PRIMARY 0
#endif
#ifndef FSPT_WIDE_TAIL
#define FSPT_WIDE_TAIL 0
#endif
#ifndef FSPT_CARRY_BLOCKS
#define FSPT_CARRY_BLOCKS 0u // trailing blocks of a logic launch that do k_wf_carry's work; 0: a launch of its own per round (rounds 3-4).
// Measured (profiles/r05/ab_fixed_costs_*.log): 4 blocks x 512 threads are a straggler - a few thousand records, one
// memory-side atomic each - the logic launch waits for: logic 0.124 -> 0.152 ms per tick on C2, 0.125 -> 0.178 on the 1 M-triangle scene
#endif
#ifndef FSPT_BATCH_ON_TARGET_STREAM
#define FSPT_BATCH_ON_TARGET_STREAM 1 // the batch scheduler's launches go to the target's stream (0: a stream of their own behind events, rounds 1-4)
#endif
#ifndef FSPT_MIN_BATCH
#define FSPT_MIN_BATCH 8 // ticks a batch of the batch scheduler holds at least; a frame whose path state allows fewer runs on the stream scheduler
#endif
#ifndef FSPT_RESOLVE_CLEARS
#define FSPT_RESOLVE_CLEARS 1 // the batch's resolve launch hands the live-path counts to the host and clears counters + pool heads (0: fill / copy commands)
#endif
#ifndef FSPT_WIDE_TRACE_BELOW
#define FSPT_WIDE_TRACE_BELOW 0u // paths
#endif
struct fspt_target {
  fspt_scene *scene = nullptr;
  uint32_t W = 0, H = 0;
  float4 *accum_own = nullptr;
  float4 *accum = nullptr;
  float4 *ray_pos = nullptr, *ray_dir = nullptr;
  bool rays_valid = false;
  uint32_t *work_counters = nullptr; // ring of zeroed work counters, one per launch
  uint32_t n_work_counters = 0;
  unsigned long long *counters = nullptr; // 6 x u64 on device
  int count = 0; // fspt_enable_counters: 0 off, 1 the reference's work, 2 the production kernels' work
  uint32_t shard = 0, n_shards = 1, tile = 32;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  uint32_t last_launches = 0;
  // wavefront pipeline
  uint32_t vw = 0, vh = 0;    // viewport (gl.viewport of the two draws); default = the whole target
  int pipeline = 1;           // 0 = megakernel, 1 = wavefront
  int sampler = 0;            // FSPT_SAMPLER_REFERENCE / FSPT_SAMPLER_SOBOL (fspt_target_set_sampler)
  uint32_t sampler_seed = 0;  // FSPT_SAMPLER_SOBOL's seed
  int lights = 0;             // FSPT_LIGHTS_OFF / FSPT_LIGHTS_EMITTERS (fspt_target_set_lights)
  float emitter_fraction = 0.5f; // q of a scene with an environment map (1 without one)
  int sched = 0;              // wavefront pipeline: 0 = batch scheduler (all ticks x all pixels per batch), 1 = stream (fixed pool)
  bool stream_fallback = false; // sched 0, but the path state of FSPT_MIN_BATCH ticks did not fit: calls run on the stream scheduler (cleared by every setter that changes what fits)
  uint32_t pool_paths = 0;    // stream: paths per state set and lane (0 = default)
  int stream_drain = -1;      // stream: iterations after the last generating one before the tail kernel takes over (-1 = default)
  uint32_t stream_iter_cap = 0; // stream, test hook: at most this many iterations per run (the finishing launch does the rest)
  uint32_t susp_budget = ST_DEFAULT_SUSP_BUDGET; // traversal steps a starved trace wave walks on before it parks its rays (0 = never)
  int stream_overlap = -1;      // stream: plan / primary / resolve on a second HIP stream beside the previous trace (1), everything on one stream (0), default (-1)
  uint32_t batch_ticks = 128; // ticks traced together by the wavefront pipeline (58 GB of path state at 1080p;
                              // measured 64 / 128 / 256 -> 3 619 / 3 794 / 3 750 Msamples/s, profiles/r01)
  // Path state and streams of the wavefront pipeline (either scheduler).  (Two such lanes with overlapped half-batches
  // were measured in rounds 1-3 and gained nothing worth their memory: profiles/r02, profiles/r03/ab_staggered_lanes.log.)
  struct WfLane {
    void *mem[WF_ARRAYS] = {};
    fspt::WfCounts *counts = nullptr;
    uint32_t *heads = nullptr;             // trace pool heads (fspt_device.hpp)
    fspt::WfCounts *counts_host = nullptr; // pinned copy of the last batch's per-round counts (tail heuristic)
    uint32_t *live_host = nullptr, *live_dev = nullptr; // ... or (counts_live) the live paths per round as the resolve launch wrote them: pinned host memory and its device address
    bool counts_live = false;
    hipEvent_t counts_ready = nullptr;
    bool counts_pending = false;
    uint32_t counts_slots = 0;             // slots of the batch the copy describes
    uint32_t slots = 0;        // allocated path slots (batch scheduler)
    hipStream_t stream = nullptr;
    hipEvent_t resolved = nullptr; // this lane's most recent resolve has finished
    // stream scheduler (fspt_device.hpp: WfStreamCtl): a pool of st_cap paths per state set + a ring of st_fin finished colours
    uint32_t st_cap = 0, st_fin = 0;
    hipStream_t stream_b = nullptr;          // plan / primary / resolve run here, beside the previous iteration's trace
    hipEvent_t ev_logic[fspt::WF_RING] = {}, ev_b[fspt::WF_RING] = {}, ev_run = nullptr, ev_b_last = nullptr;
    fspt::WfStreamCtl *ctl = nullptr;
    fspt::WfStreamCtl *ctl_host = nullptr;   // pinned copy of the last run's statistics (never waited for)
    hipEvent_t ctl_ready = nullptr;
    bool ctl_pending = false;
    uint64_t ctl_key = 0, stat_key = 0;      // what the pending copy / the known statistics describe (units, ticks, pool, bounces)
    uint32_t ctl_units = 0;                  // units of the run the pending copy describes
    uint32_t stat_gen_iters = 0;             // iterations the last such run needed to hand out all its units
    uint64_t bytes = 0;                      // path-state bytes this lane holds (either scheduler)
    int *susp[2] = {nullptr, nullptr};       // suspended-traversal records of the trace launches (fspt_device.hpp), ping-pong
    uint32_t susp_stride = 0;
    size_t susp_recs = 0;                    // records per buffer
    uint64_t susp_bytes = 0;                 // both buffers
    bool zeroed = false;                     // counts / heads / ctl are zero (cleared behind the previous batch, off the next one's critical path)
  } wf;
  // Deferred two-call ticks (fspt_camera + fspt_trace): recorded, executed in batches at the next flush point
  struct Deferred { fspt_camera_params cam; float rb_cam; uint32_t tick; float rb_trace; };
  std::vector<Deferred> pending;
  fspt_camera_params last_cam{}; // the most recent fspt_camera call (num_bounces / env_theta filled in by fspt_trace)
  float last_rb_cam = 0.0f;
  bool cam_recorded = false;     // last_cam is valid and newer than the ray buffers' contents
  bool rays_injected = false;    // the ray buffers hold caller-supplied rays (fspt_set_rays): trace them as they are
  bool defer = true;             // fspt_target_set_deferred
  // fspt_target_set_camera_model: model != FSPT_CAMERA_PINHOLE sends every tick through k_camera
  // (fspt_passes.hip) into the ray buffers and the single-tick trace from them (render_ticks)
  fspt::CameraModelP cam_model{fspt::CAM_PINHOLE, 3.14159265f, 0.064f};
  // Primary-form tuner (batch scheduler): k_wf_primary has two forms of its traversal phase with identical results
  // (fspt_kernels.hip).  Which is faster depends on the scene and the batch size, so the target measures: HIP events
  // around the primary launch of a batch, read back without waiting at the start of a later batch.  Per batch size: the
  // first batch runs the form the scene's size suggests (X), the second the other one (Y), and as a rule that settles it
  // - see prim_choose for the one case that takes a third batch.
  int primary_form = 0;      // fspt_target_set_primary_form: 0 measure and choose, 1 / 2 forced
  // batch ticks -> [form] {best ms per sample so far (< 0: none), measurements taken}
  struct PrimStat { double best[3] = {-1.0, -1.0, -1.0}; uint32_t runs[3] = {0, 0, 0}; };
  std::map<uint32_t, PrimStat> prim_ms;
  hipEvent_t prim_ev[2] = {nullptr, nullptr};
  bool prim_pending = false;
  uint32_t prim_pending_form = 0, prim_pending_ticks = 0;
  double prim_pending_samples = 0.0;
  // Node form per kernel class (fspt_target_set_node_form): -1 the library's choice, 0 the 64-byte nodes, 1 the two-level
  // nodes (fspt_device.hpp "quad"; only where the scene has them).  [0] primary launch, [1] trace launches, [2] tail kernel.
  int node_form[3] = {-1, -1, -1};
  uint32_t wide_trace_below = FSPT_WIDE_TRACE_BELOW; // library's choice for a trace launch: two-level nodes when it expects fewer paths than this
  int tail_round = -1;       // fspt_target_set_tail: -1 adaptive, 0 never, r >= 1 after round r
  float live_frac[80] = {};  // live paths after round r / slots of the batch, from the most recent finished batch
  bool live_known = false;
  uint32_t ticks_seen = 0;   // largest n_ticks of any call so far: path state is sized for min(batch_ticks, ticks_seen)
  uint64_t mem_limit = 0;    // fspt_target_set_memory_limit: cap on the path-state bytes of this target (0 = none)
  hipEvent_t ev_start = nullptr;
  // per-launch stage timing (HIP events on the target's stream)
  std::vector<hipEvent_t> ev_pool;
  std::vector<int> ev_kind;   // kernel class of pair i
  uint32_t ev_used = 0;       // pairs used by the last render
  bool ev_overflow = false;
  bool stage_events = true;   // fspt_target_set_stage_timing: a HIP event pair around every launch (fspt_last_stage_ms)
  // guided denoiser (fspt_features / fspt_denoise / fspt_draw_denoised): allocated on first use
  float4 *feat = nullptr;                 // 2 x float4 per pixel (fspt_read_features)
  float4 *dn_tmp[2] = {nullptr, nullptr}; // a-trous ping-pong
  float4 *dn_out = nullptr;               // the last denoised frame
  bool feat_valid = false, dn_valid = false;
  // fspt_present: a swap chain with one frame of latency.  Under present the batch scheduler alternates
  // batches between two lanes: lane 0 = wf on the target's stream, lane 1 = pr_lane on a stream of its own, sized for
  // the present batches it runs (not for ticks_seen).  Every other entry joins first (present_join).
  WfLane pr_lane;
  uint32_t pr_next = 0;              // lane of the next present batch
  hipEvent_t pr_acc = nullptr;       // recorded behind the last present launch that read or wrote the accumulator ...
  hipStream_t pr_acc_stream = nullptr; // ... on this stream (nullptr: no such launch since the last join)
  hipEvent_t pr_hop = nullptr;       // lane 1 waits for the target's stream behind this event ...
  bool pr_dirty = true;              // ... when something may have been enqueued there since the last present
  bool pr_active = false;            // present work may be in flight on the lane streams
  uint32_t *pr_dev[2] = {nullptr, nullptr}; // k_draw's frames (device) and their copies (pinned host), by slot
  uint8_t *pr_host[2] = {nullptr, nullptr};
  hipEvent_t pr_copied[2] = {nullptr, nullptr};
  uint32_t pr_ticks[2] = {0, 0};     // the frame's sample count (1 + its newest tick index; 0: no tick yet)
  int pr_slot = -1;                  // slot of the frame the last present enqueued (-1: none since the last join)
  uint32_t acc_ticks = 0;            // 1 + the index of the most recent tick traced into the accumulator (0: none since
                                     // create / fspt_clear; fspt_target_bind_accumulator does not reset it)
  // fspt_render_adaptive: while tile_list is set (only inside that call) every pipeline traces the n_listed
  // tiles it names instead of the shard's round-robin.  The device buffers are allocated on the first call.
  const uint32_t *tile_list = nullptr;
  uint32_t n_listed = 0;
  float4 *ad_snap = nullptr;                 // S: W*H
  uint32_t *ad_list[2] = {nullptr, nullptr}; // active tiles, ping-pong
  uint32_t *ad_count = nullptr;              // per tile: retired count; [n_tiles] = the select kernel's list length
  double *ad_err = nullptr;                  // per tile: E_T
  uint32_t ad_tiles = 0;                     // tiles the buffers hold
  // the last run (fspt_read_sample_counts, fspt_adaptive_last_stats)
  bool ad_valid = false;
  uint32_t ad_rounds = 0, ad_vw = 0, ad_vh = 0, ad_tile = 0;
  uint64_t ad_samples = 0;
  std::vector<uint32_t> ad_count_host;
  std::vector<double> ad_err_host;
  // temporal accumulation (fspt_temporal_*): allocated on the first accumulate, 112 bytes per pixel
  float4 *tm_hist[2] = {nullptr, nullptr}; // history ping-pong (rgb, length); tm_cur = the current one
  float4 *tm_g[2] = {nullptr, nullptr};    // G-buffer ping-pong: [tm_cur] = the last call's (the next call's g_prev)
  float4 *tm_m = nullptr;                  // the last call's motion buffer
  int tm_cur = 0;
  bool tm_valid = false;                   // there is a history (an accumulate since create / fspt_temporal_reset)
  bool tm_dn_valid = false;                // dn_out holds fspt_temporal_denoise's result of the CURRENT history (not fspt_denoise's)
  bool tm_gm_valid = false;                // tm_g[tm_cur] / tm_m hold a call's buffers (fspt_temporal_read_gbuffer)
  fspt::CameraP tm_cam{};                  // the previous frame's camera
  hipEvent_t tm_ev[3] = {nullptr, nullptr, nullptr}; // around the two passes of the last call
  bool tm_timed = false;
  // SVGF variance guidance (fspt_temporal_set_moments / _denoise_variance): allocated on enable, 16 bytes per pixel
  float2 *tm_mom[2] = {nullptr, nullptr};  // luminance-moment ping-pong (M1, M2), indexed like tm_hist
  float *tm_var = nullptr;                 // k_svgf_variance's output (allocated by the first fspt_temporal_denoise_variance)
  bool tm_moments = false;                 // the mode
  bool tm_mom_valid = false;               // tm_mom[tm_cur] belongs to tm_hist[tm_cur] (an accumulate since enable / reset)
  bool tm_var_valid = false;               // tm_var is the variance of the CURRENT history
  float tm_n = 0.0f;                       // acc_ticks of the last accumulate (Fe = length / n)
  hipEvent_t sv_ev[3] = {nullptr, nullptr, nullptr}; // around k_svgf_variance and the guided iterations of the last call
  bool sv_timed = false;
  // history clamp (fspt_temporal_set_clamp): allocated on enable, 32 bytes per pixel
  float4 *tm_fast[2] = {nullptr, nullptr}; // fast-history ping-pong (rgb, length), indexed like tm_hist
  bool tm_clamp = false;                   // the mode
  bool tm_fast_valid = false;              // tm_fast[tm_cur] belongs to tm_hist[tm_cur] (an accumulate since enable / reset)
  float tm_fast_history = 0.0f, tm_sigma_scale = 0.0f;
  hipEvent_t cl_ev[2] = {nullptr, nullptr}; // around k_temporal_clamp of the last accumulate
  bool cl_timed = false;
  // auto-exposure (fspt_target_set_auto_exposure): allocated on enable, 1 KiB of histogram + 32 bytes of state
  uint32_t *ax_hist = nullptr;             // 256 counts, zero between meterings (k_exposure_resolve clears them)
  fspt::ExposureState *ax_state = nullptr; // behind the histogram, in the same allocation
  bool ax_on = false;                      // the mode
  fspt::ExposureP ax_p{};
  hipEvent_t ax_ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the two kernels of the last metering and its k_draw_auto
  bool ax_timed = false;
  // bloom (fspt_target_set_bloom): the pyramid, allocated on enable for W x H at 8 levels, read-modify-write state of every bloomed draw
  float4 *bl_pyr = nullptr;
  bool bl_on = false;
  fspt::BloomP bl_p{};
  hipEvent_t bl_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // down chain | tail | up chain | draw of the last bloomed draw
  bool bl_timed = false;
  // JPEG output (fspt_draw_jpeg / fspt_present_jpeg): allocated on first use.  Under present a slot holds either
  // fspt_present's RGBA8 frame (pr_host) or fspt_present_jpeg's file (jp.c.out[slot], its length in jp_count[slot])
  fspt::JpegEnc jp;
  uint32_t *enc_frame = nullptr;              // fspt_draw_jpeg's and fspt_draw_png's drawn frame, W*H texels
  fspt::PngEnc pg;                            // PNG output (fspt_draw_png): allocated on first use
  uint32_t pg_cb = 0;                         // the smallest chunk size fspt_draw_png was asked for: pg.c.out[0] is sized for it
  fspt::ExrEnc ex;                            // OpenEXR output (fspt_draw_exr): allocated on first use
  size_t ex_bound = 0;                        // the largest bound fspt_draw_exr was asked for: ex.c.out[0] is sized for it
  uint32_t *jp_count[2] = {nullptr, nullptr}; // pinned host memory: a slot's byte count, current behind pr_copied[slot]
  int pr_kind[2] = {0, 0};                    // 0: an RGBA8 frame, 1: a JPEG file
  hipStream_t jp_copy = nullptr;              // a present file's bytes come to the host here: the copy waits for no stream that holds the next frame
  // ID mattes (fspt_mattes): allocated on first use.  mt[k]: 3 x float4 per pixel of kind k; mt_lost: the
  // two kinds' lost-sample counters; mt_valid[k]: the last pass computed kind k.  (Last: the fields above keep their places.)
  float4 *mt[2] = {nullptr, nullptr};
  unsigned long long *mt_lost = nullptr;
  bool mt_valid[2] = {false, false};
};

static const uint32_t WORK_RING = 4096;
static const uint32_t PR_LANE_TICKS = 4; // fspt_present's second lane: runs of at most this many ticks (longer ones: lane 0)
static const uint32_t WF_ROUNDS_MAX = fspt::MAX_PATH_ITERS + 4;
static const uint32_t EV_PAIRS = 4096;
static const size_t WF_HEADS_BYTES = (size_t)(WF_ROUNDS_MAX + 2) * fspt::WF_HEADS * fspt::WF_HEAD_STRIDE * sizeof(uint32_t);
static const uint64_t WF_SLOT_BUDGET = 448ull << 20; // path slots, 216 B each (up to 101 GB of the 288 GB HBM: a 4K frame x 56 ticks)
static_assert(WF_SLOT_BUDGET < (1ull << 29), "k_wf_trace keeps a path's state index in 29 bits");


// bytes per path slot of every path-state array (fspt_device.hpp: WfP)
// two state sets of A B C E D P (float4) | hit (float2) | shadow_hit (int) | fin (3 floats)   = 216 bytes per slot
static const size_t WF_ARRAY_BYTES[WF_ARRAYS] = {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 8, 4, 12};

// Geometry of a stream run: n_batch ticks of a lane's share of the frame.
struct StPlan {
  uint32_t cap, unit_slots, take_max, horizon, ring_slots, units;
};

#define FLUSH_OR_RETURN(t) do { int rc_f = flush_pending(t); if (rc_f) return rc_f; } while (0)

// ---- fspt_api.cpp
int check_device(int device);
int flush_pending(fspt_target *t);     // execute the recorded two-call ticks (and join a pipelined present first; fspt_trace's
                                       // own flushes do not join: under present they go through present_flush)
int present_join(fspt_target *t);      // wait for everything fspt_present enqueued on the lane streams
int materialise_rays(fspt_target *t);  // the ray buffers as the most recent fspt_camera call left them
const char *camera_model_name(int model); // "pinhole", "ortho", ... (error messages)
uint32_t clamp_bounces(uint32_t nb);
// ---- fspt_scene_update.cpp: entry points and *_eval / set_form hooks only; what it needs of fspt_api.cpp (geometry_order_targets),
// of fspt_scene.cpp (geometry_changed_lights) and of the .hip files is declared with the scene object above
// ---- fspt_post.cpp
// k_draw of `src` on `st` into `out` (device memory), through the target's auto-exposure and bloom when they are on
hipError_t draw_launch(fspt_target *t, const float4 *src, float exposure, float saturation, int denoise, float max_sigma,
                       float scale, uint32_t *out, hipStream_t st);
void post_release(fspt_target *t); // fspt_target_destroy: the image chain's buffers and events (the streams are idle)
// ---- the *_eval test hooks (fspt_api.cpp, fspt_scene.cpp, fspt_scene_update.cpp, fspt_post.cpp)
// A hook's device memory: ONE allocation, freed when the scope ends.  The first HIP error sticks in `e`: up, down and sync
// are no-ops behind it, and a hook launches with `if (s.ok()) s.e = launch(..)`.  `base` is NULL when the allocation
// failed: a hook returns done() at once then, before it forms a pointer into the block.  sync() stands apart from done()
// because the downloads lie between them.
struct Staging {
  char *base = nullptr;
  hipError_t e;
  explicit Staging(size_t bytes) { e = hipMalloc((void **)&base, bytes); if (e != hipSuccess) base = nullptr; }
  ~Staging() { hipFree(base); }
  Staging(const Staging &) = delete;
  Staging &operator=(const Staging &) = delete;
  bool ok() const { return e == hipSuccess; }
  void up(void *dst, const void *host, size_t bytes) { if (ok() && host) e = hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice); }
  void down(void *host, const void *src, size_t bytes) { if (ok() && host) e = hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost); }
  void sync() { if (ok()) e = hipDeviceSynchronize(); }
  int done(const char *fn) const {
    if (ok()) return FSPT_OK;
    fspt_set_error("%s: %s", fn, hipGetErrorString(e));
    return FSPT_E_HIP;
  }
};
// ---- fspt_sched_batch.cpp
void fill_trace_params(fspt_target *t, fspt::TraceP &p);
uint64_t susp_need(const fspt_target *t, uint64_t max_paths, uint32_t *stride_out, size_t *recs_out);
int susp_ensure(fspt_target *t, fspt_target::WfLane &ln, uint64_t max_paths, bool *on);
size_t wf_slot_bytes();
void wf_release(fspt_target::WfLane &ln);
void wf_release_all(fspt_target::WfLane &ln); // ... and its suspension records
int wf_plan_and_ensure(fspt_target *t, uint64_t work_total, uint32_t n_ticks, uint32_t &batch);
void prim_collect(fspt_target *t, bool wait);
void prim_reset(fspt_target *t);
uint32_t prim_choose(const fspt_target *t, uint32_t ticks);
int ev_begin(fspt_target *t, int kind, hipStream_t stream);
void ev_end(fspt_target *t, int i, hipStream_t stream);
void wf_collect_counts(fspt_target *t, fspt_target::WfLane &ln);
uint32_t wide_bit(const fspt_target *t, int kind, double paths);
uint32_t wf_tail_slice(const fspt_target *t); // fspt_sched_batch.cpp: the tail kernel's slice length for this target's scene
int render_wavefront(fspt_target *t, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks,
                     const float *rb_cam, const float *rb_trace, bool rays_from_buffers);
// fspt_present's form: the batches of a run on lane `lane` (0: wf on the target's stream, 1: pr_lane); the resolve waits for
// pr_acc and records it.  FSPT_E_NOMEM: lane 1 does not fit (nothing launched).
int render_wavefront_present(fspt_target *t, uint32_t lane, const fspt_camera_params *cam, uint32_t first_tick,
                             uint32_t n_ticks, const float *rb_cam, const float *rb_trace);
// ---- fspt_sched_stream.cpp
int st_ensure(fspt_target *t, fspt_target::WfLane &ln, uint32_t cap, uint32_t fin_slots, uint64_t budget_bytes);
int st_plan(const fspt_target *t, uint32_t units, uint32_t nbt, uint32_t nb, StPlan &pl);
int render_stream(fspt_target *t, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks,
                  const float *rb_cam, const float *rb_trace, bool rays_from_buffers);
// ---- fspt_bvh_build.hip: the GPU binned-SAH builder behind fspt_builder_build_gpu (scene_build.cpp packs its result)
namespace fspt {
struct BvhGpuResult {
  std::vector<int32_t> left, right; // children per node (-1, -1: leaf); node 0 is the root, the rest in no fixed order
  std::vector<uint32_t> lo, cnt;    // the node's triangle range [lo, lo + cnt) of `order`
  std::vector<uint32_t> box_keys;   // 12 per node: box min.xyz max.xyz, centroid min.xyz max.xyz as ordered keys
  std::vector<uint32_t> order;      // triangle indices in leaf order
  float kernel_ms = 0.0f;           // first kernel to last, from events (the per-level readbacks included)
  uint32_t launches = 0, readbacks = 0;
};
// n > 0 triangles of 9 finite floats, 1 <= leaf_size <= 64, device >= 0; leaves the calling thread's device as it was.
int bvh_build_gpu(const float *verts, uint32_t n, uint32_t leaf_size, int device, BvhGpuResult &out);
// The same kernels from vertices that are already on the CURRENT device, the result left there: `order` (n words) and, per
// node, left / right / lo / cnt (n_nodes words each; node 0 is the root).  bvh_device_release frees it.
struct BvhGpuDevice {
  const uint32_t *order = nullptr, *lo = nullptr, *cnt = nullptr;
  const int32_t *left = nullptr, *right = nullptr;
  uint32_t n_nodes = 0;
  float kernel_ms = 0.0f;
  uint32_t launches = 0, readbacks = 0;
  void *bufs = nullptr;
};
int bvh_build_device(const float *verts_dev, uint32_t n, uint32_t leaf_size, BvhGpuDevice &out);
void bvh_device_release(BvhGpuDevice &t);
// Pre-order numbering (left child first) of a builder tree of nn nodes over nt triangles: gid[p] = the builder's id of
// pre-order node p, pre[] its inverse, node_depth[p], *depth the deepest.  Checks that it is one tree whose leaves hold
// 1 .. leaf_size triangles and tile [0, nt) in pre-order; returns what is wrong, or NULL.
const char *bvh_preorder(const int32_t *left, const int32_t *right, const uint32_t *lo, const uint32_t *cnt, size_t nn, size_t nt,
                         uint32_t leaf_size, std::vector<int32_t> &pre, std::vector<uint32_t> &gid, std::vector<uint32_t> &node_depth,
                         uint32_t *depth);
float bvh_key_float(uint32_t k);
uint32_t bvh_max_depth(); // deepest node depth fspt_scene_create accepts: min(64, wf_max_stack_entries()) - 1
}  // namespace fspt
