/*
 * fspt.h — C ABI of libfspt, the MI355X-native replacement for the WebGL2 draw-call boundary of apbodnar/FSPT's path-trace hot path.
 *
 * The reference has no plugin/FFI interface: its hot path (shader/tracer.fs) sits behind the WebGL2 calls issued by main.js.
 * Every entry point below names the reference call site it replaces (file:line in /root/reference).  INTEGRATION.md shows
 * the N-API stub a maintainer of the reference would add to main.js to call these instead of gl.*.
 *
 * Conventions
 *   - plain C, no C++/torch/HIP types in any signature;
 *   - every function returns 0 on success, <0 (FSPT_E_*) on error; fspt_last_error() returns a thread-local message (reference: console.log / throw);
 *   - the library COPIES every host array it is given (caller may free after the call returns);
 *   - all calls for one target come from one host thread at a time (the reference is a single JS thread: main.js:838-857); work is enqueued on HIP
 *     streams - the two-call ticks even later, see fspt_camera - and only fspt_read_*, fspt_draw*, fspt_sync, fspt_get_counters and the fspt_last_* timers block;
 *   - there is NO CPU fallback: without a HIP device every device entry point fails with FSPT_E_NO_DEVICE.
 */
#ifndef FSPT_H
#define FSPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 6): the entry points rounds 5-6 added (fspt_intersect_form, fspt_scene_two_level_nodes, fspt_target_set_node_form,
 * fspt_target_set_stage_timing, fspt_target_shard_slots / _pack_tiles / _unpack_tiles, fspt_multi_set_exchange /
 * _get_exchange, fspt_multi_last_stage_ms) and two changes of behaviour: fspt_target_destroy DROPS recorded ticks (a host
 * that wants them executed calls fspt_sync first - PathTracer.close() does), and under fspt_target_set_memory_limit a frame
 * that cannot hold 8 ticks of path state runs on the stream scheduler's bounded pool.  The bindings compare
 * fspt_abi_version() with this value when they load the library. */
#define FSPT_ABI_VERSION 4

enum {
  FSPT_OK = 0,
  FSPT_E_INVALID = -1,   /* bad argument / inconsistent sizes            */
  FSPT_E_NO_DEVICE = -2, /* no HIP device or HIP runtime error at init   */
  FSPT_E_HIP = -3,       /* HIP runtime error (message has the details)  */
  FSPT_E_NOMEM = -4,
  FSPT_E_PARSE = -5,     /* scene pipeline: malformed OBJ / image        */
  FSPT_E_STATE = -6      /* call order (e.g. trace before camera)        */
};

typedef struct fspt_scene fspt_scene; typedef struct fspt_target fspt_target;
typedef struct fspt_builder fspt_builder;

/* ------------------------------------------------------------------------
 * Scene upload.  Replaces the texture uploads of initBVH (main.js:408-437),
 * initAtlas (main.js:548-560) and createEnvironmentMapImg (main.js:170-180).
 * Arrays are exactly what the reference hands to gl.texImage2D, WITHOUT the
 * padBuffer() padding (main.js:143-154) — pass the un-padded element counts.
 * ---------------------------------------------------------------------- */
typedef struct fspt_scene_desc {
  const float *bvh;       /* bvhTex (main.js:369-370,272-282): 9 words per node, pre-order: left, right, triStart as  */
  uint32_t n_nodes;       /* raw int32 bits in float slots (maskBVHBuffer) | min.xyz | max.xyz                        */
  const float *tri;       /* triTex (main.js:374): 9 floats per triangle v1 v2 v3, leaf order                          */
  uint32_t n_tris;
  const float *mat;       /* matTex (main.js:377-382): 12 floats per triangle [diffuseLayer emissiveLayer normalLayer  */
                          /* | mrLayer 0 0 | emittance.rgb | ior dielectric 0]                                         */
  const float *norm;      /* normTex (main.js:383-385): 27 floats per triangle, per vertex n, t, bt                    */
  const float *uv;        /* uvTex (main.js:386): 6 floats per triangle                                                */
  const uint8_t *atlas;   /* texArray (main.js:548-559): RGBA8, atlas_res^2 * atlas_layers texels, layer-major, GL rows */
  uint32_t atlas_res, atlas_layers;
  const uint8_t *env;     /* envTex (main.js:170-180): RGBE in RGBA8, env_w * env_h texels; NULL = black (main.js:303-307) */
  uint32_t env_w, env_h;
  const uint32_t *bins;   /* radianceBins (tracer.fs:21, env_sampler.js:73): n_bins x (x0,y0,x1,y1); n_bins >= 1       */
  uint32_t n_bins;
  uint32_t leaf_size;     /* '#define LEAF_SIZE' spliced into the shader (main.js:45,895)                              */
} fspt_scene_desc;

/* device = HIP device ordinal.  Builds the MI355X-native layouts (64-byte two-child nodes, 144-byte leaf records, 192-byte hit records, material texture sets in 128-byte tiles; DESIGN.md 3). */
int fspt_scene_create(const fspt_scene_desc *desc, int device, fspt_scene **out); int fspt_scene_destroy(fspt_scene *scene);
int fspt_scene_depth(const fspt_scene *scene, uint32_t *depth); /* Maximum depth of the uploaded tree (root = 0); sizes the LDS stacks. */
/* Moving geometry (DESIGN 8.6): new vertices (9 floats) and, unless norm is NULL, normTex records (27 floats) for the n_tris triangles in leaf order; the tree is REFITTED on the GPU (leaf and hit records, every box bottom-up, two-level nodes, light
 * table) exactly as fspt_scene_create would build it from the same topology.  Non-finite input: FSPT_E_INVALID, scene unchanged; leaves that do not tile [0, n_tris): FSPT_E_STATE.  Blocking; ordered against every target; accumulators are not cleared.  _rebuild_
 * (DESIGN 8.7): same input, a NEW tree - fspt_builder_build_gpu's binned SAH over tri in the order given - built on the GPU, installed in the same scene (targets stay valid; errors leave it as it was); order_out (or NULL)[k] = input index of the triangle now at leaf position k: the leaf order of later calls */
int fspt_scene_update_geometry(fspt_scene *s, const float *tri, const float *norm); int fspt_scene_rebuild_geometry(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out); /* host pointers */
int fspt_scene_update_geometry_device(fspt_scene *s, const float *tri, const float *norm); int fspt_scene_rebuild_geometry_device(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out); /* memory of the scene's device */ /* Part transforms (DESIGN 8.14): set_pose hands the scene a part id < n_parts per triangle and the rest tri (9 floats) / norm (27, or NULL: the records' normal part is left alone) in the current leaf order (host pointers; part NULL drops the pose; renders nothing differently; a rebuild permutes it).  update_transforms: xf = n_parts x 12 floats, row-major 3 x 4 (a00 a01 a02 tx | ...); a kernel poses the rest mesh (normals by the cofactor matrix, tangents by the matrix, both scaled to the matrix's rms) and the tree is refitted exactly as fspt_scene_update_geometry_device on the posed arrays.  FSPT_E_STATE without a pose; FSPT_E_INVALID (scene unchanged): wrong n_parts, a non-finite or singular matrix, an overflowing product. */ int fspt_scene_set_pose(fspt_scene *s, const uint32_t *part, uint32_t n_parts, const float *tri, const float *norm); int fspt_scene_update_transforms(fspt_scene *s, const float *xf, uint32_t n_parts); /* Skinning (DESIGN 8.16): set_skin hands the scene, per triangle corner (3 per triangle, current leaf order), joints (4 ids < n_joints) and weights (4 finite floats, used as given), the rest tri (9 floats per triangle) / norm (27, or NULL), and n_morph <= 64 morph targets as deltas, target-major: morph [n_morph][T][9], morph_norm [n_morph][T][27] (or NULL; needs norm); host pointers, validated before anything is touched, d NULL drops the skin; a rebuild permutes it.  update_skin: xf = n_joints x 12 floats, row-major 3 x 4 per joint, morph_w = n_morph floats (NULL when 0); a kernel applies the morphs, blends the four matrices, poses vertex and frame per corner and the tree is refitted exactly as fspt_scene_update_geometry_device on those arrays.  _device: xf (16-byte aligned) / morph_w in the scene's device memory, no host check.  FSPT_E_STATE without a skin; FSPT_E_INVALID (scene unchanged): other counts, a non-finite matrix or weight, a blend that collapses or overflows. */ typedef struct fspt_skin_desc { const uint16_t *joints; const float *weights; uint32_t n_joints; const float *tri, *norm, *morph, *morph_norm; uint32_t n_morph; } fspt_skin_desc; int fspt_scene_set_skin(fspt_scene *s, const fspt_skin_desc *d); int fspt_scene_update_skin(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph); int fspt_scene_update_skin_device(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph);
#define FSPT_MESH_STATIC 0xFFFFFFFFu /* fspt_mesh_desc.vertex: all three of a triangle = it is static */
/* Vertex-position update (DESIGN 8.24): set_mesh hands the scene an indexed mesh - per triangle (current leaf order) three vertex indices < n_vertices (all three FSPT_MESH_STATIC: a static triangle, which keeps the rest tri / norm given here), the six raw vt values in float64 (before obj_loader.js's EPSILON offsets), a smooth flag (NULL: all flat) and the rank its face normal is summed in (distinct; NULL: the leaf position); host pointers, validated before anything is touched, d NULL drops the mesh; a rebuild permutes it.  update_vertices: pos = n_vertices x 3 float32; kernels derive tri and the normal frames by obj_loader.js's rules in float64 (face normal; for smooth triangles the unnormalised mean of the incident face normals in rank order; calcTangents with its isNaN fallback) and the tree is refitted exactly as fspt_scene_update_geometry_device on those arrays.  _device: pos in the scene's device memory, no host check.  FSPT_E_STATE without a mesh; FSPT_E_INVALID (scene unchanged): another count, an index out of range, a partly static triangle, a non-finite uv or position, a repeated rank, a static triangle without a rest copy, a face that collapses. */
typedef struct fspt_mesh_desc { const uint32_t *vertex; uint32_t n_vertices; const double *uv; const uint8_t *smooth; const uint32_t *rank; const float *tri, *norm; } fspt_mesh_desc; int fspt_scene_set_mesh(fspt_scene *s, const fspt_mesh_desc *d); int fspt_scene_update_vertices(fspt_scene *s, const float *pos, uint32_t n_vertices); int fspt_scene_update_vertices_device(fspt_scene *s, const float *pos, uint32_t n_vertices);
int fspt_scene_sah_cost(fspt_scene *s, double *cost); /* SAH cost of the current boxes relative to the root's area, float64 */ /* Appearance (DESIGN 8.13): new matTex (12 floats per triangle, current leaf order), uvs (or NULL: kept) and atlas (or NULL: the one the scene's last update_materials call carried, FSPT_E_STATE when none did; res / layers may differ from the scene's) | new environment (NULL = black) and bins.  Laid out on the GPU; afterwards the scene renders bit for bit like fspt_scene_create of the same arrays.  Blocking; ordered against every target like fspt_scene_update_geometry; validated like fspt_scene_create; an error leaves the scene as it was; accumulators and per-target state are not touched. */ int fspt_scene_update_materials(fspt_scene *s, const float *mat, const float *uv, const uint8_t *atlas, uint32_t atlas_res, uint32_t atlas_layers); int fspt_scene_update_environment(fspt_scene *s, const uint8_t *env, uint32_t env_w, uint32_t env_h, const uint32_t *bins, uint32_t n_bins); /* Texture packing (DESIGN 8.18): the raw atlas made on the GPU from decoded sources - per layer a flat colour, a res x res RGBA8 image copied as given (GL rows), or an RGBA8 image (row 0 = top) resampled bilinearly (REPEAT in s, CLAMP_TO_EDGE in t), sRGB-decoded when corrected, swizzled, premultiplied; float32, bit for bit the hosts' resample_image. atlas_pack_gpu stands alone (atlas_out: res^2 * n_layers * 4 bytes). update_textures = fspt_scene_update_materials with the atlas packed on the scene's device (only the sources cross the bus); patch_textures: p->layers[k] replaces layer layer_ids[k] of the retained atlas (p->res = its res; FSPT_E_STATE without one), the scene is laid out again with its current materials. _device: images[i].rgba in the scene's device memory (4-byte aligned, not checked on the host). FSPT_E_INVALID before anything is touched: NULL, res / w / h of 0 or above 16384, n_layers == 0, an image index out of range, a swizzle entry above 3, an unknown kind, a non-finite colour, a _PIXELS image that is not res x res, a layer id at or above the retained layers or twice. */ enum { FSPT_TEXLAYER_COLOR = 0, FSPT_TEXLAYER_IMAGE = 1, FSPT_TEXLAYER_PIXELS = 2 }; typedef struct fspt_texture_image { const uint8_t *rgba; uint32_t w, h; } fspt_texture_image; typedef struct fspt_texture_layer { int32_t kind; float color[3]; uint32_t image; uint32_t corrected; uint8_t swizzle[4]; } fspt_texture_layer; typedef struct fspt_texture_pack { const fspt_texture_image *images; uint32_t n_images; const fspt_texture_layer *layers; uint32_t n_layers; uint32_t res; } fspt_texture_pack; int fspt_texture_decode_tables(float lin[256], float srgb[256]); int fspt_atlas_pack_gpu(int device, const fspt_texture_pack *p, uint8_t *atlas_out); int fspt_scene_update_textures(fspt_scene *s, const float *mat, const float *uv, const fspt_texture_pack *p); int fspt_scene_update_textures_device(fspt_scene *s, const float *mat, const float *uv, const fspt_texture_pack *p); int fspt_scene_patch_textures(fspt_scene *s, const uint32_t *layer_ids, uint32_t n, const fspt_texture_pack *p); int fspt_scene_patch_textures_device(fspt_scene *s, const uint32_t *layer_ids, uint32_t n, const fspt_texture_pack *p);

/* ------------------------------------------------------------------------
 * Render target.  Replaces initBuffers (main.js:598-617): the RGBA32F screen textures (a single accumulator here: each
 * pixel reads/writes only itself, tracer.fs:516-517) and the two RGBA32F camera textures.
 * Sharding (SURVEY 8e): tile x tile pixel tiles dealt round-robin (tile index % n_shards == shard); a target traces
 * only its own tiles and leaves every other pixel of its full-size accumulator at zero (a sum over shards = the frame).
 * ---------------------------------------------------------------------- */
int fspt_target_create(fspt_scene *scene, uint32_t width, uint32_t height, fspt_target **out); int fspt_target_destroy(fspt_target *target);
int fspt_target_set_shard(fspt_target *target, uint32_t shard, uint32_t n_shards, uint32_t tile);
/* Use caller-owned device memory (W*H*4 floats, e.g. a torch tensor) as the accumulator so that a collective can run
 * on it in place; NULL restores the library's own buffer.  The bound buffer is only current after fspt_sync,
 * fspt_read_radiance or fspt_draw (recorded ticks, the library's own streams); re-binding flushes the recorded ticks
 * into the old buffer, fspt_target_destroy DROPS them and never writes to a caller-owned buffer. */
int fspt_target_bind_accumulator(fspt_target *target, void *device_ptr);
int fspt_target_size(fspt_target *target, uint32_t *width, uint32_t *height); /* as created (fspt_read_radiance / fspt_draw write W*H*4 elements) */
int fspt_target_accumulator(fspt_target *target, void **device_ptr); /* device pointer of the accumulator in use (W*H*4 floats) */

/* drawCamera (main.js:741-756) -> camera.fs:37-46.  lens = lensFeatures = [1 - 1/focalDepth, apertureSize].
 * Like WebGL's draw calls the two-call form is DEFERRED: fspt_camera records its arguments, fspt_trace records the
 * tick, and recorded ticks run - consecutive ticks with an unchanged view as ONE wavefront batch - when something
 * observes or changes what they depend on (fspt_read_*, fspt_draw, fspt_sync, fspt_clear, fspt_get_counters, every
 * setter, fspt_render, fspt_set_rays) or when a batch of them has accumulated.  Results are bit-identical; an error of
 * a deferred tick is reported by the call that flushes it.  (fspt_tuning.h: fspt_target_set_deferred.) */
int fspt_camera(fspt_target *target, const float P[3], const float I[3], float fov_scale, const float lens[2], float rand_base);
/* Inject ray buffers instead (W*H*4 floats each, rows bottom-up; traced at once, from the buffers). */
int fspt_set_rays(fspt_target *target, const float *pos, const float *dir);
int fspt_read_rays(fspt_target *target, float *pos, float *dir);
/* fspt_set_rays from memory of the scene's device: copied on the target's stream, no host sync; pos / dir must be complete, and stay allocated and unmodified until the target is next synchronised. */
int fspt_set_rays_device(fspt_target *target, const float *pos, const float *dir);

/* drawTracer(i) (main.js:758-807) -> tracer.fs:436-518.  One sample for every
 * pixel from the current ray buffers, running-mean accumulate with weight
 * tick.  num_bounces is tracer.fs:9's compile-time NUM_BOUNCES made a
 * run-time argument (reference value 4).                                     */
int fspt_trace(fspt_target *target, uint32_t tick, float rand_base, float env_theta, uint32_t num_bounces);
/* tracer.fs:488 `i--` (refraction) makes the reference's loop unbounded: libfspt ends a path after FSPT_MAX_BOUNCES iterations; a larger num_bounces means that. */
#define FSPT_MAX_BOUNCES 64

/* drawTracer in `mode=test` (main.js:879-883, bvh_test.fs:224-232): the camera ray's traversal-loop iterations x 0.001 folded into the mean, no clamp. */
int fspt_trace_test(fspt_target *target, uint32_t tick);

/* tick() loop (main.js:838-857): n_ticks x (drawCamera + drawTracer) from tick first_tick, Math.random()*10000
 * (main.js:748,777) replaced by the xorshift64* stream below seeded with `seed`: two draws per tick, camera first.
 * Results are identical to the fspt_camera + fspt_trace pair. */
typedef struct fspt_camera_params {
  float P[3];
  float I[3];
  float fov_scale;
  float lens[2];
  float env_theta;
  uint32_t num_bounces;
} fspt_camera_params;
int fspt_render(fspt_target *target, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks, uint64_t seed);
/* The host PRNG of fspt_render: state' = xorshift64*(state); returns float(u >> 40) * 2^-24 * 10000 in [0, 10000). */
float fspt_rand_base_next(uint64_t *state);

/* gl.viewport(0, 0, w, h) (main.js:744,761; resScale 0.25 while dragging, main.js:840): only pixels x < w, y < h are traced; 0, 0 = the whole target. */
int fspt_target_set_viewport(fspt_target *target, uint32_t w, uint32_t h);
enum { FSPT_SAMPLER_REFERENCE = 0, FSPT_SAMPLER_SOBOL = 1 }; /* the paths' random numbers: rnd() bit for bit (default) | Owen-scrambled Sobol (DESIGN 8.2) */
int fspt_target_set_sampler(fspt_target *target, int sampler, uint32_t seed); int fspt_target_get_sampler(fspt_target *target, int *sampler, uint32_t *seed);
/* Camera models (DESIGN.md 8.15, INTEGRATION.md).  PINHOLE (default): camera.fs, fused into the path kernels.  ORTHO: parallel rays along I.  FISHEYE: equidistant,
 * angle = field of view over the frame height in radians, in (0, 2 pi].  EQUIRECT: 360 x 180 degrees.  STEREO: over-under omnidirectional stereo, ipd in scene units >= 0,
 * even height.  A flush point, does not clear; NULL = pinhole; FSPT_E_INVALID changes nothing.  Ticks are not batched under a model; adaptive / temporal: FSPT_E_STATE. */
enum { FSPT_CAMERA_PINHOLE = 0, FSPT_CAMERA_ORTHO = 1, FSPT_CAMERA_FISHEYE = 2, FSPT_CAMERA_EQUIRECT = 3, FSPT_CAMERA_STEREO = 4 };
typedef struct fspt_camera_model_params { int model; float angle; float ipd; } fspt_camera_model_params;
int fspt_target_set_camera_model(fspt_target *target, const fspt_camera_model_params *params);
int fspt_target_get_camera_model(fspt_target *target, fspt_camera_model_params *params);
enum { FSPT_LIGHTS_OFF = 0, FSPT_LIGHTS_EMITTERS = 1 }; /* NEE of emissive triangles: off (default, the reference bit for bit) | emitters (DESIGN 8.3; fspt_tuning.h) */ int fspt_target_set_lights(fspt_target *target, int mode, float emitter_fraction); int fspt_target_get_lights(fspt_target *target, int *mode, float *emitter_fraction); int fspt_scene_light_count(fspt_scene *scene, uint32_t *n_lights); /* who builds that table (DESIGN 8.23; fspt_tuning.h): the host (default) | the GPU (opt-in: 8 bytes cross the bus; the same entries, not the same bytes); setting it drops the table and rebuilds it when a target has the mode on; if that rebuild fails the builder stays what it was */ enum { FSPT_LIGHT_BUILDER_HOST = 0, FSPT_LIGHT_BUILDER_GPU = 1 }; int fspt_scene_set_light_builder(fspt_scene *scene, int builder); int fspt_scene_get_light_builder(fspt_scene *scene, int *builder);
/* Several GPUs (one frame cut into 32x32 tiles over the devices of a node; the reference has nothing here - README.md:28
 * lists "Tiled rendering" as a TODO): include/fspt_multi.h, included at the end of this file. */

/* clear() (main.js:826-836). */
int fspt_clear(fspt_target *target); int fspt_sync(fspt_target *target);
/* Adaptive sampling (DESIGN 8.5): fspt_clear, then ticks 0, 1, ... in rounds of round_ticks (fspt_render's randBase
 * stream from `seed`) over the ACTIVE tiles (tile x tile pixels meeting the viewport; all at first).  S = the means after
 * m ticks (m = round_ticks, then n whenever n >= 2m); after n > m ticks a tile's E_T = mean over its pixels and channels
 * of m (I - S)^2 / ((n - m)(I^2 + 0.01)); it retires with count n when n >= min_ticks and E_T < target_rel_mse, or at
 * n = max_ticks.  A tile retired after n ticks holds fspt_render(t, cam, 0, n, seed)'s pixels bit for bit; target 0
 * = fspt_render(max_ticks).  Afterwards the target is as fspt_render leaves it for the largest count run (rounds x
 * round_ticks, fspt_adaptive_last_stats).  Ranges: round_ticks in [2, 128], min_ticks a multiple >= 2 round_ticks,
 * max_ticks a multiple >= min_ticks, target finite >= 0 (else FSPT_E_INVALID); sharded target: FSPT_E_STATE. */
typedef struct fspt_adaptive_params { double target_rel_mse; uint32_t max_ticks, min_ticks, round_ticks; } fspt_adaptive_params;
int fspt_render_adaptive(fspt_target *target, const fspt_camera_params *cam, const fspt_adaptive_params *params, uint64_t seed);
/* The last fspt_render_adaptive's ticks per pixel: W*H counts, rows bottom-up, 0 outside its viewport (FSPT_E_STATE before one). */
int fspt_read_sample_counts(fspt_target *target, uint32_t *out);
/* What draw.fs:87 reads: RGBA32F, W*H*4 floats, row 0 = bottom, a = 1.  Blocking (syncs the stream first). */
int fspt_read_radiance(fspt_target *target, float *out);

/* drawQuad (main.js:809-824) -> draw.fs:82-93: exposure, ACES fit, saturation, gamma 1/2.2 and the
 * optional 5x5 firefly filter (draw.fs:52-80, max_sigma = the `sigma` slider) on the current
 * accumulator; writes what the canvas would hold: RGBA8, W*H*4 bytes, row 0 = bottom.  Blocking. */
int fspt_draw(fspt_target *target, float exposure, float saturation, int denoise, float max_sigma, uint8_t *out_rgba8);
/* The same with draw.fs's `scale` uniform (draw.fs:59,87: texel = ivec2(gl_FragCoord * scale)): 0.25 while the camera is dragged (main.js:819,840), else 1. */
int fspt_draw_scaled(fspt_target *target, float exposure, float saturation, int denoise, float max_sigma, float scale, uint8_t *out_rgba8);
/* drawQuad inside tick() (main.js:838-857), pipelined with one frame of latency (DESIGN.md 4.3): enqueues the ticks recorded since the last flush and
 * fspt_draw_scaled's k_draw of the result, then writes the frame the PREVIOUS call enqueued to out_rgba8 and its sample count (1 + its newest tick index) to
 * *ticks_out, blocking only for that frame.  *ticks_out = 0: nothing to present (first call after a join; out untouched).  Every entry but fspt_camera and fspt_trace joins. */
int fspt_present(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale, uint8_t *out_rgba8, uint32_t *ticks_out); /* JPEG output (DESIGN 8.19): a baseline JFIF file (Annex K tables under libjpeg's quality rule, restart_mcus MCUs per restart interval, 0 = one MCU row) made on the GPU from an RGBA8 frame (alpha ignored; bottom_up: row 0 is the bottom, as fspt_draw writes it), byte for byte libjpeg's on the MCU grid; only the file crosses the bus. FSPT_E_INVALID before a device is touched: NULL, w or h of 0 or above 65535, quality outside 1..100, an unknown subsampling or source, restart_mcus above 65535. cap smaller than the file: FSPT_E_INVALID, *bytes_out = the size needed, out untouched. */ enum { FSPT_JPEG_444 = 0, FSPT_JPEG_420 = 1 }; typedef struct fspt_jpeg_params { uint32_t quality, subsampling, restart_mcus; } fspt_jpeg_params; /* NULL = 85, 420, 0 */ enum { FSPT_SOURCE_ACCUMULATOR = 0, FSPT_SOURCE_DENOISED = 1, FSPT_SOURCE_TEMPORAL = 2, FSPT_SOURCE_TEMPORAL_DENOISED = 3 }; int fspt_jpeg_bound(uint32_t w, uint32_t h, const fspt_jpeg_params *p, size_t *bytes); /* host only: no frame is longer */ int fspt_jpeg_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* host pointers */ int fspt_jpeg_encode_device(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* rgba8 in device memory, out on the host */ /* fspt_draw_scaled (source ACCUMULATOR), fspt_draw_denoised (DENOISED; denoise, max_sigma and scale are not used) or fspt_temporal_draw (TEMPORAL, TEMPORAL_DENOISED) of the same arguments, with their errors, then fspt_jpeg_encode of that frame with bottom_up = 1; the frame stays on the device. */ int fspt_draw_jpeg(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* fspt_present with the encode enqueued behind the draw: the PREVIOUS call's file, exactly *bytes_out bytes of it, and its sample count; *ticks_out = 0 and *bytes_out = 0: nothing to present. fspt_present and fspt_present_jpeg may alternate on a target: a call returns the previous frame only when the same entry enqueued it, otherwise it waits for that frame, drops it and returns ticks 0. A frame refused because cap is too small is dropped. */ int fspt_present_jpeg(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out, uint32_t *ticks_out); /* PNG output (DESIGN 8.20): a lossless PNG file (8 bit, RGB = colour type 2 or RGBA = colour type 6 with straight alpha, no interlace) made on the GPU from an RGBA8 frame (bottom_up as above), byte for byte tests/png_ref.py's: the five filters with the smallest sum of signed magnitudes per row (or one fixed filter), then deflate in independent chunks of chunk_bytes of the filtered stream - literals and distance-1 matches under a dynamic Huffman code per chunk, a stored block where that is not shorter - one IDAT per chunk and one for the Adler-32.  Only the file crosses the bus.  FSPT_E_INVALID before a device is touched: NULL, w or h of 0 or above 65535, channels other than 0, 3, 4, a filter above FSPT_PNG_FILTER_ADAPTIVE, chunk_bytes other than 0 or 256..32768, an unknown source, a file that could pass 4 GiB.  cap smaller than the file: FSPT_E_INVALID, bytes_out = the size needed, out untouched. */ enum { FSPT_PNG_FILTER_NONE = 0, FSPT_PNG_FILTER_SUB = 1, FSPT_PNG_FILTER_UP = 2, FSPT_PNG_FILTER_AVERAGE = 3, FSPT_PNG_FILTER_PAETH = 4, FSPT_PNG_FILTER_ADAPTIVE = 5 }; typedef struct fspt_png_params { uint32_t channels, filter, chunk_bytes; } fspt_png_params; /* NULL = 3, adaptive, FSPT_PNG_CHUNK; channels 0 and chunk_bytes 0 = those defaults too */ int fspt_png_bound(uint32_t w, uint32_t h, const fspt_png_params *p, size_t *bytes); /* host only: no file is longer */ int fspt_png_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* host pointers */ int fspt_png_encode_device(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* rgba8: device memory of `device`; out: host */ /* fspt_draw's frame (source, exposure .. scale as fspt_draw_jpeg's: auto-exposure and bloom take part) as a PNG file; blocking */ int fspt_draw_png(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* OpenEXR output (DESIGN 8.21): a single-part scanline OpenEXR 2 file made on the GPU from W*H*4 floats of scene-linear radiance (no exposure, bloom or tone map) and, for the feature layers, fspt_read_features' W*H*8 floats; byte for byte tests/exr_ref.py's.  Channels in file order, those present: A B G N.X N.Y N.Z R Z albedo.B albedo.G albedo.R.  R G B always; the others by `layers`.  Z (the first hit's distance, 1e5 for a miss) is always FLOAT, the rest take pixel_type.  A is the source's fourth float as stored: 1 in the accumulator and in a denoised buffer, the history length in a temporal one. HALF is round-to-nearest-even in integer arithmetic; every NaN becomes 0x7E00 / 0x7FC00000.  bottom_up: row 0 of the buffers is the bottom (as every library buffer); the file's scanline 0 is the top.  ZIP deflates blocks of 16 scanlines, ZIPS of one, each a zlib stream of its own cut into chunks of chunk_bytes; a block that deflate does not shorten is stored raw.  Only the file crosses the bus.  FSPT_E_INVALID before a device is touched: NULL (features only where a feature layer asks for them), w or h of 0 or above 65535, an unknown compression, pixel type, layer bit or source, chunk_bytes other than 0 or 256..32768, a file that could pass 4 GiB.  cap smaller than the file: FSPT_E_INVALID, *bytes_out = the size needed, out untouched. */ enum { FSPT_EXR_NONE = 0, FSPT_EXR_ZIPS = 2, FSPT_EXR_ZIP = 3 }; enum { FSPT_EXR_HALF = 1, FSPT_EXR_FLOAT = 2 }; enum { FSPT_EXR_ALPHA = 1, FSPT_EXR_ALBEDO = 2, FSPT_EXR_NORMAL = 4, FSPT_EXR_DEPTH = 8 }; typedef struct fspt_exr_params { uint32_t compression, pixel_type, layers, chunk_bytes; } fspt_exr_params; /* NULL = ZIP, HALF, 0 (RGB), FSPT_EXR_CHUNK; chunk_bytes 0 = that default too */ int fspt_exr_bound(uint32_t w, uint32_t h, const fspt_exr_params *p, size_t *bytes); /* host only: no file is longer */ int fspt_exr_encode(int device, const float *rgba, const float *features, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* host pointers */ int fspt_exr_encode_device(int device, const float *rgba, const float *features, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* rgba, features: device memory of `device`, 16-byte aligned; out: host */ /* The buffer `source` stands for (the accumulator, fspt_denoise's, fspt_temporal_accumulate's or fspt_temporal_denoise's result; FSPT_E_STATE as the entry that draws it) and, for feature layers, fspt_features' buffer (FSPT_E_STATE without one) as an OpenEXR file; blocking; joins a present. */ int fspt_draw_exr(fspt_target *t, int source, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out);

/* Guided denoiser (DESIGN.md 8; the reference lists "denoising" under post processing).  fspt_features: `samples` camera
 * rays per pixel of the whole target (k_camera's ray for randBase r_s, the s-th fspt_rand_base_next value from `seed`) to
 * their first hit; per pixel the float32 means of (texDiffuse, t) and (macroNormal before the `inside` flip, hit), a miss
 * counting as (1,1,1), 1e5, (0,0,0), 0.  fspt_denoise: K edge-avoiding a-trous iterations on the current accumulator c
 * with the features a, n, z, h:  u = c / max(a, 1e-3);  u'(p) = sum_q w u(q) / sum_q w over q = p + 2^k (i, j), i, j in
 * -2..2 inside the image;  w = B[i] B[j] wc wn wz, B = (1,4,6,4,1)/16;  wc = exp(-|L(u_p) - L(u_q)| / (sc 2^-k (L(u_p) +
 * L(u_q)) + 1e-4)), L = Rec.709 luma;  wn = 1 if sn = 0, q = p or h_p = h_q = 0, else 0 if one h or one |n| is 0, else
 * clamp(n_p.n_q / |n_p||n_q|, 0, 1)^sn;  wz = 1 if z_p = z_q, else exp(-|z_p - z_q| / (sz 2^k max(z_p, 1e-3)));  out =
 * (a u_K, 1) (K = 0: c).  sc = sz = +inf switch wc, wz off.  fspt_draw_denoised: fspt_draw (denoise 0, scale 1) of it. */
typedef struct fspt_denoise_params { uint32_t iterations; float sigma_color, sigma_normal, sigma_depth; } fspt_denoise_params;
#define FSPT_DENOISE_ITERATIONS 4    /* defaults (params NULL): the best of a 78-setting scan on the MI355X (DESIGN 8.1) */
#define FSPT_DENOISE_SIGMA_COLOR 4.0f
#define FSPT_DENOISE_SIGMA_NORMAL 32.0f
#define FSPT_DENOISE_SIGMA_DEPTH 0.05f
int fspt_features(fspt_target *t, const fspt_camera_params *cam, uint32_t samples, uint64_t seed); /* samples >= 1 */
int fspt_read_features(fspt_target *t, float *out);              /* W*H*8 floats, rows bottom-up; blocking */
int fspt_denoise(fspt_target *t, const fspt_denoise_params *p, float *out); /* p NULL = defaults, iterations <= 16; out W*H*4 floats or NULL: keep on the device */
int fspt_draw_denoised(fspt_target *t, float exposure, float saturation, uint8_t *out_rgba8);
/* Temporal accumulation (DESIGN 8.8; the rule, defaults and ranges: fspt_tuning.h).  One call = one frame: the previous call's result, reprojected through the first hit of
 * every pixel's centre ray, is blended with the accumulator (only read).  fspt_scene_motion_begin snapshots the triangles: what moves until the next accumulate is reprojected from there. */
typedef struct fspt_temporal_params { float alpha, max_history, depth_tol, normal_cos; } fspt_temporal_params;
int fspt_temporal_accumulate(fspt_target *t, const fspt_camera_params *cam, const fspt_temporal_params *p, float *out); /* p NULL = defaults; out W*H*4 (rgb, length) or NULL */
int fspt_temporal_reset(fspt_target *t);                                                    /* the next accumulate is a first one */
int fspt_temporal_denoise(fspt_target *t, const fspt_denoise_params *p, float *out);        /* fspt_denoise of the temporal result */
int fspt_temporal_draw(fspt_target *t, float exposure, float saturation, int denoised, uint8_t *out_rgba8); /* fspt_draw / fspt_draw_denoised of it */
int fspt_scene_motion_begin(fspt_scene *s); int fspt_scene_motion_end(fspt_scene *s);       /* snapshot (a rebuild permutes it) | drop it: static scene */
int fspt_temporal_set_moments(fspt_target *t, int on); /* SVGF variance guidance (DESIGN 8.9; rule and defaults: fspt_tuning.h): accumulate also carries luminance moments; default off */
int fspt_temporal_denoise_variance(fspt_target *t, const fspt_denoise_params *p, float *out); /* fspt_temporal_denoise guided by the variance estimate; sigma_color = sigma_l */
int fspt_temporal_set_clamp(fspt_target *t, int on, float fast_history, float sigma_scale); /* history clamp (DESIGN 8.10; rule and defaults: fspt_tuning.h): a fast history bounds the long one; default off */
/* Auto-exposure (DESIGN 8.11; rule and defaults: fspt_tuning.h): every drawing entry first meters the buffer it draws (a luminance histogram of the viewport, on the GPU, no host read) and its `exposure` argument becomes a compensation of the metered value. */ typedef struct fspt_exposure_params { float key, low, high, adapt_up, adapt_down, min_log2, max_log2; } fspt_exposure_params;
int fspt_target_set_auto_exposure(fspt_target *t, int on, const fspt_exposure_params *p); /* p NULL = defaults; default off */ int fspt_exposure_reset(fspt_target *t); /* the next metering is a first one */
int fspt_exposure_get(fspt_target *t, float *exposure, float *log2_mean, uint32_t *metered); /* blocking; joins a present */ /* Bloom (DESIGN 8.12; rule and defaults: fspt_tuning.h): every drawing entry first builds an HDR pyramid of the buffer it draws and mixes its glow in before the exposure. */ typedef struct fspt_bloom_params { float intensity, scatter; uint32_t levels; } fspt_bloom_params; int fspt_target_set_bloom(fspt_target *t, int on, const fspt_bloom_params *p); /* p NULL = defaults; default off */ int fspt_target_get_bloom(fspt_target *t, int *on, fspt_bloom_params *p);
/* intersectScene (tracer.fs:366-404) as a stand-alone entry: n rays (origin xyz, dir xyz) -> closest hit t and triangle index (-1 = miss, t = 1e5), optionally loop-iteration and leaf-visit counts per ray.  Host pointers. */
int fspt_intersect(fspt_scene *scene, const float *rays, uint32_t n, float *t_out, int32_t *index_out, uint32_t *steps_out, uint32_t *leaves_out); /* ID mattes (DESIGN 8.25): per pixel, which objects and which materials cover it and by how much, as Cryptomatte stores it.  An id is a 32-bit name hash kept as the bits of a normal finite float: fspt_matte_hash = MurmurHash3_x86_32 (seed 0) of the bytes, then h ^= 1 << 23 when the exponent field (h >> 23) & 255 is 0 or 255. set_matte_ids: one id per triangle of the scene's current tri array (the index fspt_intersect reports, the order update_geometry takes), copied to the device; 0 = no matte (counts like a miss); any other id with exponent field 0 or 255: FSPT_E_INVALID naming the first such index, nothing changed; NULL drops the kind.  The table survives the update entries; a rebuild permutes it with the order it returns.  set_matte_manifest: opaque bytes (at most 2^20) kept on the host for the file header; NULL / 0 = none. fspt_mattes: `samples` (1..65535) camera rays per pixel of the whole target - the very rays fspt_features(cam, samples, seed) traces - each traced once; per kind with ids a table of FSPT_MATTE_RANKS slots: a hit's id raises its slot's count, else takes the lowest empty slot, else the sample is lost.  Ranks = slots by count descending, ties first seen first; rank r = (the id's bits as a float, (float)count / (float)samples), empty ranks (0, 0).  FSPT_E_STATE: no ids of any kind.  A flush point, joins a present, clears nothing.  read_mattes: W*H*12 floats (id0 c0 .. id5 c5), rows bottom-up; mattes_lost: the samples the last pass dropped; both blocking, FSPT_E_STATE before a pass or for a kind it did not compute. */ enum { FSPT_MATTE_OBJECT = 0, FSPT_MATTE_MATERIAL = 1 };
#define FSPT_MATTE_RANKS 6
uint32_t fspt_matte_hash(const char *name, size_t len); /* host only */ int fspt_scene_set_matte_ids(fspt_scene *s, int kind, const uint32_t *ids); int fspt_scene_set_matte_manifest(fspt_scene *s, int kind, const char *json, size_t len); int fspt_mattes(fspt_target *t, const fspt_camera_params *cam, uint32_t samples, uint64_t seed); int fspt_read_mattes(fspt_target *t, int kind, float *out); int fspt_mattes_lost(fspt_target *t, int kind, uint64_t *lost); /* Cryptomatte layers in an OpenEXR file (DESIGN 8.25): fspt_exr_* with two more layer bits, accepted by these entries and by fspt_draw_exr (which takes the target's matte buffers and the scene's manifests; a bit without a pass for that kind: FSPT_E_STATE) and refused by fspt_exr_bound / _encode / _encode_device as before.  Per kind present twelve FLOAT channels Crypto<Object|Material>0<0|1|2>.<R|G|B|A> = id(2j), cov(2j), id(2j+1), cov(2j+1) of level j, in the file's byte-sorted channel order (between B and G, material first), and directly behind `compression` the string attributes cryptomatte/<key>/conversion = uint32_to_float32, /hash = MurmurHash3_32, /manifest (when given), /name, <key> = the first seven hex digits of the layer name's hash.  ranks[k]: W*H*12 floats as fspt_read_mattes returns them (needed where the bit is set), manifest[k] / manifest_len[k]: at most 2^20 bytes, NULL / 0 = none; m NULL in the bound: no manifests. */ enum { FSPT_EXR_CRYPTO_OBJECT = 16, FSPT_EXR_CRYPTO_MATERIAL = 32 }; typedef struct fspt_exr_mattes { const float *ranks[2]; const char *manifest[2]; size_t manifest_len[2]; } fspt_exr_mattes; /* by FSPT_MATTE_* */ int fspt_exr_bound_mattes(uint32_t w, uint32_t h, const fspt_exr_params *p, const fspt_exr_mattes *m, size_t *bytes); /* host only */ int fspt_exr_encode_mattes(int device, const float *rgba, const float *features, const fspt_exr_mattes *m, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* host pointers */ int fspt_exr_encode_mattes_device(int device, const float *rgba, const float *features, const fspt_exr_mattes *m, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out); /* rgba, features, ranks: device memory of `device`, 16-byte aligned; manifests and out: host */

/* Work counters for the byte accounting of SURVEY 8d, summed since the last fspt_clear / fspt_counters_reset while
 * counting is enabled (slower kernel variants).  enable = 1 counts the REFERENCE's work (NEE shadow rays traced to
 * their closest hit like tracer.fs:501: equal to the oracle's counters), 2 the production kernels' (shadow rays stop
 * at the first hit - only `shadow.index == -1` is consumed, tracer.fs:502); radiance is identical. */
typedef struct fspt_counters {
  uint64_t samples;     /* tracer.fs main() invocations                      */
  uint64_t rays;        /* intersectScene calls            (tracer.fs:366)   */
  uint64_t steps;       /* while(idx>-1) iterations        (tracer.fs:373)   */
  uint64_t leaves;      /* processLeaf calls               (tracer.fs:380)   */
  uint64_t shades;      /* bounce-loop iterations          (tracer.fs:446)   */
  uint64_t env_lookups; /* envSample calls                 (tracer.fs:416)   */
} fspt_counters;
int fspt_enable_counters(fspt_target *target, int enable); int fspt_get_counters(fspt_target *target, fspt_counters *out); int fspt_counters_reset(fspt_target *target);

/* ------------------------------------------------------------------------
 * Scene pipeline (host side, CPU; SURVEY 8f-1/8f-2): obj_loader.js + bvh.js + the packing loops of initBVH with the
 * same decisions in the same float64 arithmetic (1M triangles take the JS builder 2.5 min / 4 GB).
 * ---------------------------------------------------------------------- */
typedef struct fspt_prop_desc {
  const double *rotate; /* one scene-JSON prop (obj_loader.js:20-38): n_rotate x (axis.xyz, angle) in order, ... */
  uint32_t n_rotate;
  double scale;         /* ... then scale, then translate */
  double translate[3];
  uint32_t normals_mode; /* 0 = "flat"/default, 1 = "smooth", 2 = "mesh" (obj_loader.js:144,196) */
  double diffuse_layer, emissive_layer, normal_layer, mr_layer; /* getMaterial (main.js:206-270): atlas layer ids etc. */
  double emittance[3];
  double ior, dielectric;
} fspt_prop_desc;

/* one element of scene.worldTransforms (obj_loader.js:26-36): `if (t.rotate) rotations (positions and
 * normals) else if (t.translate) translation (positions only)`; has_rotate = the key is present. */
typedef struct fspt_world_transform {
  const double *rotate; /* n_rotate x 4: axis.x axis.y axis.z angle */
  uint32_t n_rotate;
  uint32_t has_rotate;
  double translate[3];
  uint32_t has_translate;
} fspt_world_transform;

/* getMaterial's result for one OBJ group (main.js:206-270, packed by main.js:376-382) */
typedef struct fspt_group_material {
  double diffuse_layer, emissive_layer, normal_layer, mr_layer;
  double emittance[3];
  double ior, dielectric;
} fspt_group_material;

int fspt_builder_create(fspt_builder **out); int fspt_builder_destroy(fspt_builder *b);
/* parseMesh (obj_loader.js:6-215) for one prop: v / vt / vn / f, fan triangulation, negative indices, transforms,
 * normals, tangents. */
int fspt_builder_add_obj(fspt_builder *b, const char *obj_text, size_t len, const fspt_prop_desc *prop);
/* The same in two steps, for OBJs whose `usemtl` groups carry their own materials (mtl_loader.js, getMaterial): parse
 * (scene.worldTransforms, prop.skips), list the groups in the reference's iteration order (Object.entries: array-index
 * names first), let the host resolve one material per group, commit.  mtllib = ordinal of the `mtllib` line current at
 * the group's first face (-1: none). */
int fspt_builder_parse_obj(fspt_builder *b, const char *obj_text, size_t len, const fspt_prop_desc *prop,
                           const fspt_world_transform *world, uint32_t n_world,
                           const char *const *skips, uint32_t n_skips, uint32_t *n_groups);
int fspt_builder_group_info(const fspt_builder *b, uint32_t group, const char **name, uint32_t *n_tris, int32_t *mtllib);
int fspt_builder_mtllib_name(const fspt_builder *b, uint32_t index, const char **name);
int fspt_builder_commit_obj(fspt_builder *b, const fspt_group_material *mats, uint32_t n_groups);
/* scene.normalize (main.js:337-348): centre on the scene bounds and scale the longest side to 2*size. */
int fspt_builder_normalize(fspt_builder *b, double size);
/* new BVH(geometry, leaf_size) + serializeTree + packing (bvh.js:5-91, main.js:355-392); _gpu: binned SAH on `device` (DESIGN 8.4) */
int fspt_builder_build(fspt_builder *b, uint32_t leaf_size); int fspt_builder_build_gpu(fspt_builder *b, uint32_t leaf_size, int device);
int fspt_builder_counts(const fspt_builder *b, uint32_t *n_nodes, uint32_t *n_tris, uint32_t *depth);
/* shootAutoFocusRay (main.js:447-546) on the built tree, in float64: distance along (eye, dir) to the first
 * triangle, 1e6 when there is none; the reference then sets lensFeatures[0] = 1 - 1/dist. */
int fspt_builder_autofocus(const fspt_builder *b, const double eye[3], const double dir[3], double *dist);
/* Copies the packed reference-layout arrays (bvh 9*n_nodes, tri 9*n_tris, mat 12*n_tris, norm 27*n_tris, uv 6*n_tris). */
int fspt_builder_get(const fspt_builder *b, float *bvh, float *tri, float *mat, float *norm, float *uv);
/* ProcessEnvRadiance (env_sampler.js:1-74) on raw RGBE bytes.  Writes up to
 * cap bins (4 uint32 each) and the real count to *n_bins. */
int fspt_env_bins(const uint8_t *rgbe, uint32_t w, uint32_t h, uint32_t *bins, uint32_t cap, uint32_t *n_bins); /* The same bins, built on HIP device `device` from a summed-area table of the map (DESIGN 8.17): same contract, host pointers. */ int fspt_env_bins_gpu(const uint8_t *rgbe, uint32_t w, uint32_t h, int device, uint32_t *bins, uint32_t cap, uint32_t *n_bins); /* GPU sky (DESIGN 8.17; the model, defaults and ranges: fspt_tuning.h): single-scattering Rayleigh + Mie seen from the ground, as a w x h equirect map in envSample's mapping (row 0 = straight up), 1..65535 texels per side.  sun_dir: finite, non-zero, normalised by the library; below the horizon is night.  A value out of range: FSPT_E_INVALID, before a device is touched. */ typedef struct fspt_sky_params { float sun_dir[3]; float turbidity, sun_intensity, sun_radius, gain; float ground_albedo[3]; uint32_t view_samples, light_samples; } fspt_sky_params; /* rgbe_out: w*h*4 bytes (RGBE as the environment takes it); linear_out: w*h*3 floats, the radiance before the encode.  Either may be NULL.  Host pointers. */ int fspt_sky_generate(int device, const fspt_sky_params *p, uint32_t w, uint32_t h, uint8_t *rgbe_out, float *linear_out); /* fspt_scene_update_environment without the host's bins: _auto takes host RGBE, _device RGBE in the scene's device memory, and the bins are built on the GPU from the uploaded map; _sky generates the map there too, so that no texel crosses the bus. Afterwards the scene renders bit for bit like fspt_scene_create of the same bytes and fspt_env_bins of them.  Blocking; ordered against every target; an error leaves the scene as it was; accumulators and per-target state are not touched. */ int fspt_scene_update_environment_auto(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h); int fspt_scene_update_environment_device(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h); int fspt_scene_update_sky(fspt_scene *s, const fspt_sky_params *p, uint32_t w, uint32_t h);

const char *fspt_last_error(void); int fspt_abi_version(void); int fspt_device_count(void); /* visible HIP devices (0 when none / no driver) */

#ifdef __cplusplus
}
#endif
#include "fspt_multi.h"
#endif /* FSPT_H */
