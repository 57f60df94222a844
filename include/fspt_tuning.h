/*
 * fspt_tuning.h — scheduling knobs and measurement hooks of libfspt.
 *
 * Nothing here has a counterpart in the reference (one fragment-shader invocation walks a whole path,
 * tracer.fs:436-518; its whole state is two accumulators and two ray textures, main.js:598-617) and nothing here can
 * change a rendered value: every setting gives bit-identical results.  The drop-in boundary is include/fspt.h; a host
 * that only wants what main.js does never includes this file.  bench.py, the tests and tools/ do.
 */
#ifndef FSPT_TUNING_H
#define FSPT_TUNING_H

#include "fspt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Execution strategy of fspt_trace / fspt_render:
 *   1 "wavefront, batches" (default): primary -> [trace <-> logic] x rounds [-> tail] -> resolve, queue-driven kernels
 *      over batch_ticks ticks at a time (0 keeps the current batch size; default and max 128); path state = every
 *      (pixel, tick) of a batch, 216 bytes each;
 *   2 "wavefront, stream": the same kernels over a FIXED pool of live paths that is kept full (path regeneration
 *      between launches): every launch is pool-sized whatever the call's tick count, path state is the pool
 *      (fspt_target_set_pool) and a ring of finished samples; a run covers batch_ticks (<= 128) ticks;
 *   0 "megakernel": one persistent kernel per tick (path regeneration in place), no path state in memory. */
int fspt_target_set_pipeline(fspt_target *target, int pipeline, uint32_t batch_ticks);
/* Stream scheduler: `paths` = live paths each state set holds (0 = default, 16 Mi; 204 bytes per path; never more than
 * the call's samples); `drain_iterations` = trace/logic iterations after the last one that generated samples before
 * the tail kernel runs the rest to completion (-1 = default); `max_iterations` caps the iterations of a run (0 = no
 * cap; a test hook: the finishing launch then generates what the cursor has not handed out); `overlap` = 1: plan /
 * primary / resolve of an iteration on a second HIP stream beside the previous iteration's trace, 0: one stream,
 * -1: default. */
int fspt_target_set_pool(fspt_target *target, uint32_t paths, int drain_iterations, uint32_t max_iterations, int overlap);
/* Suspended traversals: a trace launch ends on its longest ray.  A wave that can get no more rays walks on for `steps`
 * traversal steps, then writes its unfinished traversals (node, t, hit, stack) to records and ends; the next trace
 * launch resumes them first (the path lags a round, at most four times).  0 = never; default 24.  Not used by the
 * counting kernel variants. */
int fspt_target_set_trace_budget(fspt_target *target, uint32_t steps);
/* When the batch scheduler hands the remaining live paths to the tail kernel (one launch that alternates traversal and
 * shading per path until it ends): -1 (default) decides from the previous batch's live-path counts and measured
 * launch times, 0 never (except for paths that refraction keeps alive beyond NUM_BOUNCES rounds, tracer.fs:488),
 * r >= 1 after round r. */
int fspt_target_set_tail(fspt_target *target, int round);
/* Node form of the traversal, per kernel class.  Every interior node has a 64-byte record (the boxes of its two
 * children: one of the reference's traversal steps, tracer.fs:372-392, per memory round trip) and - when
 * fspt_scene_create found every box of the tree to be the exact union of its children's boxes, which holds for every
 * tree bvh.js builds (bvh.js:120-126) - a 128-byte two-LEVEL record (the boxes of the four grandchildren, from which the
 * children's are derived exactly): two steps per round trip at twice the requests per fetch, the same nodes visited in
 * the same order.  The first is faster where the vector-memory request rate binds (large trace launches on a
 * cache-resident scene), the second where a launch is a bundle of dependent chains (tail kernel, small trace launches,
 * scenes beyond the L2).  primary / trace / tail: -1 the library's choice, 0 the 64-byte nodes, 1 the two-level nodes;
 * tail = 2: ADAPTIVE - the 64-byte nodes while a wave can refill its lanes from the list of live paths, the two-level
 * nodes from then on (a traversal changes form in mid-walk: node references and stack entries mean the same in both);
 * trace_below >= 0: the library's choice for a trace launch is "two-level when it expects fewer paths than this" (from
 * the previous batch's live-path counts); < 0 keeps the current threshold.  Ignored on a scene without two-level nodes
 * and by the counting kernel variants. */
int fspt_target_set_node_form(fspt_target *target, int primary, int trace, int tail, int64_t trace_below);
/* Whether the scene has two-level nodes, and their size in bytes (either pointer may be NULL). */
int fspt_scene_two_level_nodes(const fspt_scene *scene, int *present, uint64_t *bytes);
/* The most recent fspt_scene_update_geometry[_device]: GPU time from its first kernel to its last (HIP events; the 4-byte
 * readback of the finite check lies between them) and the kernels it launched (one per tree level among them). */
int fspt_scene_last_update_ms(fspt_scene *scene, float *ms, uint32_t *launches);
/* The most recent fspt_scene_rebuild_geometry[_device]: GPU ms of the build kernels (their per-level readbacks
 * included), GPU ms of the install kernels (slot map, permute, gather, child references, the refit), host ms of the
 * numbering, kernels launched, readbacks (the builder's 4-byte ones + the one of the topology).  Any pointer may be NULL. */
int fspt_scene_last_rebuild_ms(fspt_scene *scene, float *build_ms, float *install_ms, float *host_ms, uint32_t *launches, uint32_t *readbacks);
/* Part transforms, test and measurement hooks.
 * read_pose: the posed tri (n_tris x 9) / norm (n_tris x 27; either may be NULL) the most recent fspt_scene_update_transforms
 * wrote to the staging array the refit read (FSPT_E_STATE when another call has reused the array since).
 * last_pose_ms: GPU ms of k_pose_transform, GPU ms of the refit behind it (as fspt_scene_last_update_ms), kernels launched.
 * pose_matrices_eval: the host part of the rule alone, no device: out = n_parts x 30 floats (a | D | N);
 * FSPT_E_INVALID and *bad_part for a non-finite or singular matrix. */
int fspt_scene_read_pose(fspt_scene *s, float *tri, float *norm);
int fspt_scene_last_pose_ms(fspt_scene *s, float *transform_ms, float *refit_ms, uint32_t *launches);
int fspt_pose_matrices_eval(const float *xf, uint32_t n_parts, float *out, uint32_t *bad_part);
/* Skinning, test and measurement hooks.
 * read_skin: the tri' (n_tris x 9) / norm' (n_tris x 27; either may be NULL) the most recent fspt_scene_update_skin[_device]
 * wrote to the staging array the refit read (FSPT_E_STATE when another call has reused the array since).
 * last_skin_ms: GPU ms of k_skin_transform, GPU ms of the refit behind it, kernels launched, and the bytes the skin holds on
 * the device by the library's accounting: n_tris x (24 + 48 + 36 [+ 108 with norm]) + n_morph x n_tris x (36 [+ 108 with
 * morph_norm]) + n_joints x 48 + n_morph x 4 (the host form's frame); 0 without a skin.  Any pointer may be NULL.
 * skin_check_eval: fspt_scene_set_skin's validation alone, no device and no scene: FSPT_E_INVALID with the reason and the
 * offending index in fspt_last_error and in *bad_index (the corner-slot index into joints / weights, the element index into
 * tri / norm / morph / morph_norm; untouched for a refused count or pointer).
 * skin_set_form: measurement switch, process-wide: where k_skin_transform reads the joint table from, 0 = global memory,
 * 1 = staged once per block in LDS (tables of up to 64 KiB; larger ones are read from global memory).  The bits are the same. */
#define FSPT_SKIN_MAX_MORPH 64
int fspt_scene_read_skin(fspt_scene *s, float *tri, float *norm);
int fspt_scene_last_skin_ms(fspt_scene *s, float *skin_ms, float *refit_ms, uint32_t *launches, uint64_t *bytes);
int fspt_skin_check_eval(const fspt_skin_desc *d, uint32_t n_tris, uint64_t *bad_index);
int fspt_skin_set_form(int form);
/* Vertex-position update, test and measurement hooks.
 * read_mesh: the tri (n_tris x 9) / norm (n_tris x 27; either may be NULL) the most recent fspt_scene_update_vertices[_device]
 * wrote to the staging array the refit read (FSPT_E_STATE when another call has reused the array since, a refused
 * fspt_scene_update_vertices among them: what the refit's check refused is not handed out).
 * last_mesh_ms: GPU ms of the derive kernels (first to last), GPU ms of the refit behind them, kernels launched, and the
 * bytes the mesh holds on the device by the library's accounting: n_tris x (12 + 24 + 4 [+ 144 with a static triangle])
 * + n_vertices x 12 (the host form's frame) and, with a smooth triangle, (n_vertices + 1) x 4 + incident corners x 4 +
 * n_tris x 24 + n_vertices x 24; 0 without a mesh.  Any pointer may be NULL.
 * last_mesh_pass_ms: derive_ms pass by pass: k_mesh_faces, k_mesh_vertex_normals, k_mesh_smooth_frames (a flat-only mesh
 * runs the first alone: the other two are 0).
 * mesh_frames_eval: fspt_scene_set_mesh's validation (first, without a device: FSPT_E_INVALID with the reason), then the
 * derive kernels alone on `device` - no scene, no refit and so no non-finite check: what the isNaN quirk leaves is seen.
 * f64_probe_eval: out[i] = sqrt(a[i]) (op 0; b unused) or a[i] / b[i] (op 1) in float64 as those kernels compile them:
 * the contract needs both correctly rounded. */
int fspt_scene_read_mesh(fspt_scene *s, float *tri, float *norm);
int fspt_scene_last_mesh_ms(fspt_scene *s, float *derive_ms, float *refit_ms, uint32_t *launches, uint64_t *bytes);
int fspt_scene_last_mesh_pass_ms(fspt_scene *s, float ms[3]);
int fspt_mesh_frames_eval(int device, const fspt_mesh_desc *d, uint32_t n_tris, const float *pos, float *tri_out, float *norm_out);
int fspt_f64_probe_eval(int device, int op, const double *a, const double *b, uint32_t n, double *out);
/* Camera models, measurement hook: k_camera of the target's model (FSPT_E_STATE under pinhole) `reps` times
 * into the ray buffers on the target's stream between two HIP events; *ms_per_launch = their distance / reps.  Blocking; a flush
 * point; the ray buffers are overwritten (a recorded fspt_camera call's rays are made again on demand; injected rays are gone:
 * fspt_set_rays again before the next fspt_trace). */
int fspt_camera_model_time(fspt_target *target, const fspt_camera_params *cam, uint32_t reps, float *ms_per_launch);
/* Appearance update, test and measurement hooks.
 * what: 0 texture-set table, 1 single-layer tiled images, 2 interleaved images, 3 environment tiles, 4 bins, 5 hit records.
 * Copies min(cap, size) bytes and writes the size to *bytes (out NULL: only that).  Blocking. */
int fspt_scene_read_appearance(fspt_scene *s, int what, void *out, uint64_t cap, uint64_t *bytes);
/* the last appearance update: kernels first to last (HIP events; the read-back of the per-layer flags and the host's set
 * classification lie between them), launches, bytes uploaded, raw-atlas bytes retained on the device (0: never updated) */
int fspt_scene_last_appearance_ms(fspt_scene *s, float *ms, uint32_t *launches, uint64_t *uploaded, uint64_t *retained);
/* the last fspt_atlas_pack_gpu of this process: the uploads and the read-back by the host's clock, the kernel by HIP events */
int fspt_atlas_pack_last_ms(float *upload_ms, float *kernel_ms, float *readback_ms);
/* The argument checks of the texture entries on the host alone: a whole description (layer_ids NULL and n 0), or a patch of
 * n layers against a retained atlas of raw_layers layers of raw_res^2 texels (raw_layers 0: none, FSPT_E_STATE).  No device. */
int fspt_texture_pack_check_eval(const fspt_texture_pack *p, const uint32_t *layer_ids, uint32_t n, uint32_t raw_layers, uint32_t raw_res);
/* The set classification fspt_scene_create and fspt_scene_update_materials share, on the host alone: per triangle its
 * texture set, *n_sets, and the first min(cap_sets, *n_sets) 12-word rows of the set table, from matTex, the per-layer
 * "every texel equal" flags and first texels, under the current interleaving budget.  No device. */
int fspt_texset_classify_eval(const float *mat, uint32_t n_tris, uint32_t n_layers, uint32_t res, const uint8_t *is_const, const uint32_t *first,
                              uint32_t *tri_set, uint32_t *n_sets, uint32_t *tab, uint32_t cap_sets);
/* GPU sky (fspt.h: fspt_sky_generate, fspt_scene_update_sky).  A planet of radius Re = 6 360 km under an atmosphere
 * up to Ra = 6 420 km; Rayleigh scale height 7994 m, betaR = (5.8, 13.5, 33.1)e-6 / m; Mie scale height 1200 m, betaM =
 * turbidity x 21e-6 / m on every channel, extinction 1.1 betaM, g = 0.76; the observer stands 1 m above the ground.  Per texel
 * the view ray (to the ground or the top of the atmosphere) is cut into view_samples midpoint samples; from each a light ray to
 * the top of the atmosphere in light_samples midpoint samples (one below the ground: that view sample is in the planet's
 * shadow); L = sun_intensity (sumR betaR pR + sumM betaM pM), plus the lit ground (albedo / pi x the transmitted irradiance)
 * where the ray ends on it, plus the disc (sun_intensity T / (pi sun_radius^2)) where mu >= cos(sun_radius) and it does
 * not; all times gain.  The encode: non-finite or negative -> 0; e = the smallest integer with 2^e >= max(r, g, b, 1e-6),
 * clamped to [-127, 127]; bytes floor(c 2^-e 255 + 0.5) clamped to [0, 255], e + 128.  tests/sky_ref.py restates both.
 * Ranges (else FSPT_E_INVALID): turbidity [0, 64], sun_intensity >= 0, sun_radius (0, 0.5], gain >= 0, ground_albedo [0, 1],
 * view_samples [1, 64], light_samples [1, 32], all finite.  The defaults are conventions (Nishita's constants), not measurements. */
#define FSPT_SKY_TURBIDITY 1.0f
#define FSPT_SKY_SUN_INTENSITY 20.0f
#define FSPT_SKY_SUN_RADIUS 0.02f
#define FSPT_SKY_GAIN 1.0f
#define FSPT_SKY_GROUND_ALBEDO 0.3f
#define FSPT_SKY_VIEW_SAMPLES 16
#define FSPT_SKY_LIGHT_SAMPLES 8
#define FSPT_SKY_MAX_VIEW_SAMPLES 64
#define FSPT_SKY_MAX_LIGHT_SAMPLES 32
/* the last update_sky / update_environment_auto / _device of the scene, from HIP events: the generator (0 without one); the
 * bins - radiance, the two table scans, the tree levels, the count, the read-back of n_bins and the emit; the tiling.
 * launches and readbacks count kernel launches and device -> host copies; n_bins what was built. */
int fspt_scene_last_sky_ms(fspt_scene *s, float *sky_ms, float *bins_ms, float *tile_ms, uint32_t *launches, uint32_t *readbacks, uint32_t *n_bins);
/* Test hook: the device's summed-area-table sum of the map's per-texel radiance (env_sampler.js getRadiance, float64) over n
 * integer boxes (x0, y0, x1, y1), x0 <= x1 <= w, y0 <= y1 <= h: what the tree build reads.  Host pointers. */
int fspt_env_box_sums_eval(int device, const uint8_t *rgbe, uint32_t w, uint32_t h, const uint32_t *boxes, uint32_t n, double *out);
/* fspt_intersect (fspt.h) walking the two-level nodes (two_level != 0; FSPT_E_INVALID when the scene has none): t, index
 * and the per-ray step / leaf counts must equal the one-level walk's (tests). */
int fspt_intersect_form(fspt_scene *scene, int two_level, const float *rays, uint32_t n, float *t_out, int32_t *index_out,
                        uint32_t *steps_out, uint32_t *leaves_out);
/* The primary launch (ray generation + the camera ray's traversal + its shading) has two forms of its traversal phase:
 * 1 = one traversal per lane (a wave waits for its longest ray), 2 = per-lane refill over 2 x 64 samples per wave.  0
 * (default): the batch scheduler times both on the target's own batches (HIP events around the launch, read back
 * without waiting): per batch size the first batch runs the form the scene's size suggests, the second the other one,
 * a third batch is spent only when the first form lost by no more than its cold start explains; then the faster form
 * runs - form 1 on the 70 k-triangle scene, form 2 on the 1 M-triangle one. */
int fspt_target_set_primary_form(fspt_target *target, int form);
/* Measurement switch, process-wide: the logic launch (k_wf_logic) lists the paths it shades per block iteration and shades them
 * in whole waves; the lanes that own those paths fetch their state rows beside the finishing paths' and park them in LDS, so
 * that the shading pass does not fetch the same memory lines a second time.  entries: -1 = the library's choice (what two
 * resident blocks per CU leave of the LDS), 0 = no stash (every listed path is read from memory again), n = at most n entries
 * of 96 bytes; listed paths beyond the stash are read from memory.  FSPT_E_INVALID below -1.  The bits are the same. */
int fspt_logic_set_stash(int entries);
/* The form the next batch of `batch_ticks` ticks will use and what has been measured for that batch size so far
 * (best ms per sample of form 1, form 2; < 0: not measured yet).  Blocking (waits for a measurement in flight). */
int fspt_target_get_primary_form(fspt_target *target, uint32_t batch_ticks, int *form, double ms_per_sample[2]);
/* fspt_trace executes at once (0) instead of being recorded and batched (1, default; fspt.h: fspt_camera). */
int fspt_target_set_deferred(fspt_target *target, int enable);
/* Cap on the target's path-state bytes (0 = none): state sets, ray results, finished samples and suspension records
 * together.  A batch that does not fit the cap - or the free device memory - is halved, down to 8 ticks (or the call's
 * own tick count, if that is less); a frame that cannot hold that much runs its calls on the STREAM scheduler instead,
 * whose path state is a fixed pool sized to the cap (its runs shortened until two units of the pool fit); suspension
 * records that would take more than a quarter of the cap are not used.  Results never depend on any of it.
 * FSPT_E_NOMEM when not even a pool of two one-tick units (128 paths) fits. */
int fspt_target_set_memory_limit(fspt_target *target, uint64_t bytes);
/* Path-state bytes currently allocated by this target (state sets, ray results, finished samples, suspension
 * records) and the batch size in use (after any halving). */
int fspt_target_path_state_bytes(fspt_target *target, uint64_t *bytes, uint32_t *batch_ticks);
/* Allocate (and touch) the path state for the current resolution / shard / batch_ticks now instead of lazily inside
 * the first fspt_trace / fspt_render.  Blocking. */
int fspt_target_prepare(fspt_target *target);
/* Live paths after wavefront round r (r = 1: the primary launch) as a fraction of the batch's samples, from the most
 * recent batch: frac[r] for r < n_rounds (frac[0] unused).  Blocking. */
int fspt_target_live_paths(fspt_target *target, double *frac, uint32_t n_rounds);
/* The last fspt_render_adaptive (FSPT_E_STATE before one): its rounds, the samples it traced (sum over tiles of count x
 * viewport pixels), and per tile (row-major, tiles_x = ceil(W / 32) by default) the count and the E_T that retired it (0, 0
 * for a tile outside the viewport).  The arrays may be NULL; otherwise they hold `cap` >= the tile count entries. */
int fspt_adaptive_last_stats(fspt_target *target, uint32_t *rounds, uint64_t *samples, double *tile_err, uint32_t *tile_ticks, uint32_t cap);
/* Memory fspt_scene_create may spend on INTERLEAVED material textures (process-wide; scenes created afterwards;
 * default 8 GiB): a material that samples two or more image layers at one uv (tracer.fs:453-456) gets one image with
 * 16-byte texels, so that a shading event's 16 taps lie in ~2 cache lines instead of ~6; materials beyond the budget
 * read their layers from single-layer images. */
int fspt_set_texture_interleave_budget(uint64_t bytes);

/* ---- measurement ---------------------------------------------------------------------------------------------------- */
/* Per-launch stage timing: a HIP event pair around every kernel launch of the wavefront pipeline, what fspt_last_stage_ms
 * reads (default on).  The events are not free - two timestamp markers per launch, ~30 launches per 20-tick batch: 1.3 % of
 * a 20-tick region (profiles/r05/ab_stage_events.log) - so a host that only wants frames switches them off; the events
 * around the whole call (fspt_last_kernel_ms) stay.  With them off fspt_last_stage_ms reports zeros. */
int fspt_target_set_stage_timing(fspt_target *target, int enable);
/* HIP-event time of the most recent fspt_trace / fspt_render on this target (total ms, kernel launches).  Blocking. */
int fspt_last_kernel_ms(fspt_target *target, float *ms, uint32_t *launches);
/* ... per kernel class {primary, trace, logic, resolve, tail}: summed HIP-event durations and launch counts.  With
 * the stream scheduler's two HIP streams the classes overlap (their sum exceeds fspt_last_kernel_ms).  Blocking. */
int fspt_last_stage_ms(fspt_target *target, float ms[5], uint32_t launches[5]);
/* Of the traversal steps counted since fspt_counters_reset, how many k_wf_trace served from its LDS copy of the top of
 * the tree instead of the vector-memory pipeline (bench.py's request-rate roofline). */
int fspt_get_trace_lds_steps(fspt_target *target, uint64_t *steps);

/* Free and total memory of a device as the HIP runtime reports it (hipMemGetInfo): what a host sizes its batches against,
 * and how the tests check that dropped tracers give their memory back. */
int fspt_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* Of the builder's last fspt_builder_build_gpu: HIP-event time from its first kernel to its last (the per-level
 * readbacks included), kernel launches, device-to-host readbacks.  FSPT_E_STATE after fspt_builder_build. */
int fspt_builder_gpu_stats(const fspt_builder *b, float *kernel_ms, uint32_t *launches, uint32_t *readbacks);
/* The built tree's triangle order (n_tris): packed triangle k (fspt_builder_get) is the builder's triangle order[k], in the
 * order the OBJs added them - what a second builder's tree is compared against triangle by triangle. */
int fspt_builder_tri_order(const fspt_builder *b, uint32_t *order);
/* The builder's triangles in PARSE order, packed like fspt_builder_get's arrays (9 / 12 / 27 / 6 floats each; NULL = skip);
 * works before a build: what a host moves and hands to fspt_scene_update_geometry through fspt_builder_tri_order's order. */
int fspt_builder_geometry(const fspt_builder *b, uint32_t *n_tris, float *tri, float *mat, float *norm, float *uv);
/* The built tree's triangles as an indexed mesh (fspt_scene_set_mesh), in leaf order: vertex = 3 indices per
 * triangle, made global over the OBJs by an offset per OBJ; uv = the 6 raw vt values in float64, before calcTangents'
 * offsets (NaN for a triangle without vt: its uvs depend on the positions, so it can only be static); *n_vertices = the
 * `v` lines of all OBJs; positions = their world positions (n_vertices x 3, float32 of the float64 the builder holds; a
 * vertex no face names is transformed like the others, so the array can go back to fspt_scene_update_vertices as it is).
 * Any pointer may be NULL. */
int fspt_builder_get_mesh(const fspt_builder *b, uint32_t *vertex, double *uv, uint32_t *n_vertices, float *positions);

/* ---- test hook ------------------------------------------------------------------------------------------------------ */
/* Device-side evaluation of the deterministic math primitives (DESIGN.md
 * "fspt-math"), for bitwise comparison against the oracle's C versions.
 * op: see FSPT_MATH_* ; a, b: n inputs each (b may be NULL for unary ops). */
enum {
  FSPT_MATH_SIN = 0, FSPT_MATH_COS = 1, FSPT_MATH_ATAN2 = 2, FSPT_MATH_ASIN = 3,
  FSPT_MATH_EXP2 = 4, FSPT_MATH_DIV = 5, FSPT_MATH_SQRT = 6, FSPT_MATH_RND = 7,
  FSPT_MATH_FRACT = 8, FSPT_MATH_LOG2 = 9, FSPT_MATH_POW = 10
};
int fspt_math_eval(int device, int op, const float *a, const float *b, uint32_t n,
                   float *out);
/* fspt_target_set_sampler (fspt.h): FSPT_SAMPLER_SOBOL draws value(seed, pixel, sample, dim) with pixel = y*W + x
 * of the full target, sample = the tick (the running mean's weight index) and dim = the values the sample has drawn so far
 * (the camera ray 0..3, then each shaded hit in call order: 6 values, 8 on the Lambert branch).  rand_base arguments and
 * fspt_render's seed then do not affect radiance; rays materialised before they are traced (fspt_read_rays,
 * fspt_trace_test) use sample index 1 + the last tick accumulated (0 after create or fspt_clear).  Every pipeline and
 * scheduler gives the same bits.  Like every setter it runs the recorded ticks first and keeps the accumulator.
 * Test hook: the FSPT_SAMPLER_SOBOL device function value(seed, pixel[i], sample[i], dim[i]) for n triples (host arrays). */
int fspt_sampler_eval(int device, uint32_t seed, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim,
                      uint32_t n, float *out);
/* fspt_denoise (fspt.h) test hook: the same k_atrous launches, on host arrays in the library's layouts - accum
 * W*H*4 floats, features W*H*8 floats (fspt_read_features) - instead of a target's; out: the W*H*4 denoised floats.
 * p NULL = defaults; the parameters fspt_denoise refuses are refused here too, with the same codes. */
int fspt_denoise_eval(int device, const float *accum, const float *features, uint32_t W, uint32_t H,
                      const fspt_denoise_params *p, float *out);
/* fspt_temporal_accumulate (fspt.h).  Pass 1, per pixel p: the CENTRE ray (fspt_camera's ray without pixel jitter and
 * lens offset) to its closest hit: G(p) = (t, leaf slot as int bits, bv, bw), (macroNormal.xyz, hit); a miss: (1e5, -1, 0, 0), (0, 0, 0, 0).
 * X' = the hit point (static scene) or v1' + bv e1' + bw e2' of the same slot in fspt_scene_motion_begin's snapshot; v = X' - P_prev
 * (a miss: v = the ray direction); with the previous call's camera (bX, bY, I, fov): a = v.I / I.I (a <= 0: behind), icx = v.bX / (a fov),
 * icy = v.bY / (a fov), sx = (icx H / W + 1) W / 2 - 0.5, sy = (icy + 1) H / 2 - 0.5, each SNAPPED to the nearest integer when within
 * 1/128 of it; M(p) = (sx, sy, |v| or 0 for a miss, kind), kind 0 = no previous call or behind, 1 = hit, 2 = miss.
 * Pass 2: taps q = floor(sx, sy) + {0, 1}^2 with bilinear weights w_q; a tap counts when w_q > 0, q lies in the image, hit(q) = hit(p),
 * and for hits |t_prev(q) - M.z| <= depth_tol M.z and n(p) . n_prev(q) >= normal_cos.  H = sum w_q hist(q).rgb / sum w_q,
 * N = min(sum w_q hist(q).w / sum w_q, max_history), a = max(n / (N + n), alpha), n = the accumulator's ticks:
 * out = (H + (I - H) a, min(N + n, max_history)); no tap counts: out = (I.rgb, min(n, max_history)).  Then out is the history, G the
 * previous G-buffer, cam the previous camera.  Ranges: alpha in [0, 1], max_history >= 1, depth_tol >= 0, normal_cos in [-1, 1] (else
 * FSPT_E_INVALID); FSPT_E_STATE: no tick in the accumulator, a sharded target, a viewport smaller than the target. */
#define FSPT_TEMPORAL_ALPHA 0.0f         /* defaults (params NULL): the best row of DESIGN 8.8's scan */
#define FSPT_TEMPORAL_MAX_HISTORY 64.0f
#define FSPT_TEMPORAL_DEPTH_TOL 0.05f
#define FSPT_TEMPORAL_NORMAL_COS 0.95f
/* G (W*H*8 floats) and M (W*H*4 floats) of the last fspt_temporal_accumulate, rows bottom-up; either may be NULL.  Blocking. */
int fspt_temporal_read_gbuffer(fspt_target *t, float *g_out, float *m_out);
/* The scene's leaf slots (what G's slot and the traversal's hit index address) and, per slot, the triangle it holds in the scene's
 * current leaf order (0xFFFFFFFF-style values beyond n_tris: an empty slot).  Either pointer may be NULL; sizes first. */
int fspt_scene_slot_triangles(fspt_scene *s, uint32_t *n_slots, uint32_t *slot_tri);
/* GPU ms of the last call's two passes, from HIP events: ms[0] the G-buffer and motion pass, ms[1] the blend pass.  Blocking. */
int fspt_temporal_last_ms(fspt_target *t, float ms[2]);
/* Test hook: the blend pass alone on host arrays in the library's layouts - accum, motion, hist W*H*4 floats, g, g_prev W*H*8
 * floats, n = the accumulator's ticks (>= 1) - out: W*H*4.  hist NULL (then g_prev may be NULL): no history. */
int fspt_temporal_eval(int device, const float *accum, const float *motion, const float *g, const float *hist, const float *g_prev,
                       uint32_t W, uint32_t H, uint32_t n, const fspt_temporal_params *p, float *out);
/* SVGF variance guidance (fspt.h fspt_temporal_set_moments / fspt_temporal_denoise_variance).  With moments on (16 bytes per
 * pixel, a ping-pong pair of (M1, M2); FSPT_E_STATE from fspt_temporal_accumulate before any fspt_features) the blend pass also carries two
 * luminance moments of the DEMODULATED input: u = I.rgb / max(albedo, 1e-3), l = L(u) (Rec.709 luma), m = (l, l l); with the colour's taps,
 * tests, weights w_q and blend factor a: Hm = sum w_q mom(q) / sum w_q, Mout = Hm + (m - Hm) a; no tap counts or no moments history:
 * Mout = m.  The colour is the same bit for bit.  Variance (k_svgf_variance): Fe = out.w / n; Fe >= 4: v = max(0, M2 - M1 M1) / Fe; else over
 * the 7 x 7 window inside the image with fspt_denoise's wn wz at step 1 (k = 0; the centre weighs 1): S1 = sum w M1 / sum w, S2 likewise,
 * v = max(0, S2 - S1 S1) / max(Fe, 1): the variance of the luminance of the temporal MEAN the filter reads.  Filter: fspt_denoise's
 * iterations on the history with wc replaced by wl = exp(-|L(u_p) - L(u_q)| / (sl sqrt(gv_p) + 1e-4)), gv_p = the (1,2,1) x (1,2,1) / 16 blur
 * (renormalised inside the image) of the iteration's input variance at p's 3 x 3 neighbours one pixel apart, sl = sigma_color = +inf:
 * wl = 1; the variance goes along, var'(p) = sum w w var(q) / (sum w)^2, v into iteration 0; out = (a u_K, 1) into fspt_denoise's buffer
 * (fspt_temporal_draw(denoised = 1) draws it; K = 0: the history).  FSPT_E_INVALID: NULL, fspt_denoise's parameter ranges; FSPT_E_STATE:
 * moments off, no accumulate since they were switched on or since fspt_temporal_reset, no features, a sharded target. */
#define FSPT_SVGF_ITERATIONS 4    /* defaults (params NULL): the best row of DESIGN 8.9's scan (the SVGF paper's sigma_l = 4 loses on a moving camera) */
#define FSPT_SVGF_SIGMA_L 8.0f
#define FSPT_SVGF_SIGMA_NORMAL 32.0f
#define FSPT_SVGF_SIGMA_DEPTH 0.05f
/* v of the last fspt_temporal_denoise_variance (W*H floats) and (M1, M2) of the last accumulate (W*H*2 floats), rows bottom-up; either may be
 * NULL (the moments alone need no denoise call).  Blocking. */
int fspt_temporal_read_variance(fspt_target *t, float *var_out, float *moments_out);
/* GPU ms of the last fspt_temporal_denoise_variance, from HIP events: ms[0] k_svgf_variance, ms[1] the guided iterations (the moments blend
 * is fspt_temporal_last_ms's ms[1]).  Blocking. */
int fspt_svgf_last_ms(fspt_target *t, float ms[2]);
/* Test hook: k_svgf_variance and the guided iterations on host arrays in the library's layouts - hist W*H*4 floats (rgb, length), moments
 * W*H*2, features W*H*8, n = the accumulator's ticks (>= 1) - out: the W*H*4 filtered floats; var_in, var_out (W*H each, may be NULL): v and
 * the variance the last iteration leaves (K = 0: v).  p NULL = the defaults above. */
int fspt_svgf_eval(int device, const float *hist, const float *moments, const float *features, uint32_t W, uint32_t H, uint32_t n,
                   const fspt_denoise_params *p, float *out, float *var_in, float *var_out);
/* Temporal history clamp (fspt.h fspt_temporal_set_clamp): k_temporal_blend rejects history on geometry only, so a change of the
 * LIGHT enters a long history at n / (max_history + n) per frame.  With the mode on (32 bytes per pixel, a ping-pong pair of float4) pass 2
 * also carries a FAST history F (rgb, length) through the colour's own four taps, acceptance tests and bilinear weights w_q, with the colour's
 * recursion and fast_history (in samples, like max_history; finite, >= 1) in max_history's place: Hf = sum w_q F(q).rgb / sum w_q,
 * Nf = min(sum w_q F(q).w / sum w_q, fast_history), af = max(n / (Nf + n), alpha), Fout = (Hf + (I - Hf) af, min(Nf + n, fast_history)); no tap
 * counts or no fast history: Fout = (I.rgb, min(n, fast_history)).  F never reads the long history: it is what fspt_temporal_accumulate with
 * max_history = fast_history computes, bit for bit; the colour and the moments of pass 2 are the same bit for bit.  Pass 3 (k_temporal_clamp),
 * per pixel p and channel c over the taps of the 5 x 5 window around p that lie inside the image (cnt of them): mu = sum Fout_c / cnt,
 * m2 = sum Fout_c Fout_c / cnt, sd = sqrt(max(0, m2 - mu mu)), lo = mu - sigma_scale sd, hi = mu + sigma_scale sd,
 * out_c = min(max(hist_c, lo), hi); .w, the length, is untouched.  sigma_scale >= 0; +inf: the clamp never binds (pass 3 is skipped; no
 * inf * 0).  The clamped value IS the history: out, fspt_temporal_denoise[_variance], fspt_temporal_draw and the next call's taps read it;
 * the moments of 8.9 are not clamped.  Where the light is stable the box holds the long history and nothing changes; where it changed the long
 * history is pulled to what the last fast_history samples saw.  Switching the mode on drops an existing history (both start together, as
 * fspt_temporal_set_moments does); a call that changes only the two parameters keeps both; fspt_temporal_reset drops both; off frees the
 * pair.  FSPT_E_INVALID: NULL, a non-finite or below-1 fast_history, a negative or NaN sigma_scale; FSPT_E_STATE: a sharded target. */
#define FSPT_TEMPORAL_CLAMP_FAST_HISTORY 32.0f /* defaults of the hosts (the C call takes both): the best row of DESIGN 8.10's scan, which started from 16 and 2 */
#define FSPT_TEMPORAL_CLAMP_SIGMA_SCALE 1.0f
/* Fout of the last fspt_temporal_accumulate with the clamp on: W*H*4 floats (rgb, length), rows bottom-up.  Blocking. */
int fspt_temporal_read_fast(fspt_target *t, float *out);
/* GPU ms of pass 3 of the last fspt_temporal_accumulate with the clamp on, from HIP events (sigma_scale = +inf: an empty interval);
 * fspt_temporal_last_ms keeps its two values.  Blocking. */
int fspt_temporal_clamp_last_ms(fspt_target *t, float *ms);
/* Test hook: k_temporal_clamp on host arrays - hist, fast, out: W*H*4 floats (rgb, length); lo_out, hi_out (W*H*4 each, may be NULL): the
 * box per channel, .w = 0 (sigma_scale = +inf: -inf / +inf and out = hist, without a launch). */
int fspt_temporal_clamp_eval(int device, const float *hist, const float *fast, uint32_t W, uint32_t H, float sigma_scale,
                             float *out, float *lo_out, float *hi_out);
/* Auto-exposure (fspt.h fspt_target_set_auto_exposure).  Luma: L = fma(b, 0.0722, fma(g, 0.7152, r 0.2126)) in float32 (k_draw's own).  Bin:
 * a pixel with !(L >= 2^-16) (zero, negatives, NaN, denormals) is left out; else bin = min((float_bits(L) >> 20) - ((127 - 16) << 3), 255): 32 octaves
 * from 2^-16 with 8 sub-bins each, piecewise-linear in log2, no log2 per pixel; +inf and everything from 2^16 up: bin 255.  The target's viewport is
 * metered.  Resolve (one block, float64): N = the sum of the counts; N = 0 leaves the state untouched (never set: exposure 1).  Of the pixels sorted by
 * bin the ranks [floor(low N), ceil(high N)) are kept, kept_b = the overlap of bin b's rank range with it, K = sum kept_b;
 * v_b = (b >> 3) - 16 + log2(1 + ((b & 7) + 0.5) / 8); mean = (sum over b ascending of kept_b v_b) / K; target = log2(key) - mean; in log2 of the exposure:
 * no valid previous state: e = target, else e = prev + (target - prev) a, a = adapt_up when the scene got brighter (target < prev), else adapt_down, both in
 * (0, 1], 1 = instant (a host with a clock passes 1 - exp(-dt speed)); e clamped to [min_log2, max_log2]; exposure = (float)exp2(e).  A draw with the mode on
 * multiplies its exposure argument by that float32, in float32; the rest is k_draw.  State: 1 KiB of histogram + 32 bytes, allocated on enable, freed on
 * disable and with the target; a call that changes only the parameters keeps the adapted state.  No drawing entry gains a host synchronisation.
 * FSPT_E_INVALID: NULL, non-finite fields, key <= 0, low / high outside 0 <= low < high <= 1, adapt_* outside (0, 1], min_log2 > max_log2; FSPT_E_STATE: a
 * sharded target, fspt_exposure_reset / _get with the mode off.  fspt_multi_* targets are not metered.
 * The defaults are conventions, not measurements: the key is Reinhard's middle grey, the percentiles are UE4's histogram metering; instant adaptation
 * suits a still (render_sequence picks a slower one). */
#define FSPT_EXPOSURE_KEY 0.18f
#define FSPT_EXPOSURE_LOW 0.10f
#define FSPT_EXPOSURE_HIGH 0.90f
#define FSPT_EXPOSURE_ADAPT_UP 1.0f
#define FSPT_EXPOSURE_ADAPT_DOWN 1.0f
#define FSPT_EXPOSURE_MIN_LOG2 -8.0f
#define FSPT_EXPOSURE_MAX_LOG2 8.0f
/* The device's exposure record.  reserved: 0 on the device; fspt_exposure_eval stores the OR of the histogram's words AFTER the resolve there (0: cleared). */
typedef struct fspt_exposure_state { float exposure; uint32_t valid, metered, reserved; double log2_exposure, log2_mean; } fspt_exposure_state;
/* Test hook: the two production kernels on a host array - rgba W*H*4 floats, metered over x < vw, y < vh (0, 0 = the whole image); prev NULL = never
 * metered; hist_out = the 256 counts k_exposure_histogram left (before the resolve cleared them), state_out = what the resolve wrote.  p NULL = defaults. */
int fspt_exposure_eval(int device, const float *rgba, uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const fspt_exposure_params *p,
                       const fspt_exposure_state *prev, uint32_t *hist_out, fspt_exposure_state *state_out);
/* GPU ms of the last metering on this target, from HIP events: ms[0] k_exposure_histogram, ms[1] k_exposure_resolve.  Blocking. */
int fspt_exposure_last_ms(fspt_target *t, float ms[2]);
/* ... and of the k_draw_auto behind it: what the metering's cost is set against.  Blocking. */
int fspt_exposure_last_draw_ms(fspt_target *t, float *ms);
/* Measurement switch, process-wide: k_exposure_histogram's form, 0 (shipped) = one LDS atomic per pixel, 1 = the lanes that share the first active lane's
 * bin are counted by a ballot and added once.  The histogram is the same bit for bit. */
int fspt_exposure_set_form(int form);
/* Bloom (fspt.h fspt_target_set_bloom): the threshold-free, energy-conserving "scatter" pyramid, taken from the HDR buffer a drawing entry is
 * about to draw, before the exposure.  All of it in float32, in exactly this order (both kernel forms and the draw follow it; tests/bloom_ref.py restates it).
 * Sanitise, per channel: s(v) = v >= 0 ? min(v, FSPT_BLOOM_CLAMP) : 0 - NaN and negatives become 0, +inf the clamp (the path kernels' own per-sample clamp),
 * so one bad texel cannot poison the frame through the pyramid.  Level 0 is the drawn buffer restricted to the viewport vw x vh; nothing outside it is read.
 * Sizes: w_{k+1} = (w_k + 1) >> 1, the same for h; j = the smallest k with min(w_k, h_k) == 1; n = min(levels, j) levels are built; n = 0 (a 1 x N or N x 1
 * viewport): the draw is the plain draw.
 * Down: D_{k+1}(x, y) = sum_{j,i in 0..3} w_j w_i S_k(clamp(2x - 1 + i, 0, w_k - 1), clamp(2y - 1 + j, 0, h_k - 1)), w = (1, 3, 3, 1) / 8, S_0 = s(level 0),
 * S_k = D_k; separable, horizontal first; one pass of taps a0..a3 is ((a1 + a2) * 3 + (a0 + a3)) * 0.125, evaluated as written: a1 + a2, its product by 3,
 * a0 + a3 and the sum of the two round (four roundings, three deep), the product by 1/8 is exact.
 * Up: up(U)(x, y), the 2 x 2 tent over the coarser level U (w x h): cx0 = x >> 1, cx1 = clamp(cx0 + ((x & 1) ? 1 : -1), 0, w - 1), weights 3/4 on cx0 and 1/4
 * on cx1, the same in y; horizontal first: up = fma(3/4, fma(3/4, U(cx0, cy0), U(cx1, cy0) / 4), fma(3/4, U(cx0, cy1), U(cx1, cy1) / 4) / 4): two roundings deep.
 * Combine: U_n = D_n; for k = n - 1 .. 1: U_k = fma(scatter, up(U_{k+1}) - D_k, D_k) (the difference rounds, the fma rounds), in place over D_k;
 * B = up(U_1) at level-0 coordinates.
 * Draw: the source texel (x, y) = ivec2(frag * scale) as before; c = that texel, or the firefly-filtered `middle` under `denoise`; c0 = s(c);
 * c' = fma(intensity, B(x, y) - c0, c0) per channel; c' * exposure goes into the rest of the draw unchanged.  A source texel outside the viewport is drawn plain.
 * Consequences: the weights are dyadic, so only additions (and the two parameter fma) round; scaling the input by a power of two scales every level by exactly
 * that power, away from the clamp and from denormals; on a finite, non-negative buffer under the clamp intensity = 0 gives the mode-off bytes; auto-exposure
 * (8.11) meters the source buffer, not the bloomed one.  Roundings on the deepest path: D_k 6 k, U_k 6 n + 4 (n - k), B 10 n - 2, c' 10 n.
 * State: the pyramid, allocated on enable for the target's W x H at FSPT_BLOOM_MAX_LEVELS (16 bytes a texel, at most a third of the accumulator), freed on disable
 * and with the target; a call that changes only the parameters keeps it.  No drawing entry gains a host synchronisation.  FSPT_E_INVALID: NULL, non-finite
 * fields, intensity or scatter outside [0, 1], levels outside [1, FSPT_BLOOM_MAX_LEVELS]; FSPT_E_STATE: a sharded target.  fspt_multi_* targets are not bloomed.
 * The defaults are conventions, not measurements (Jimenez' / Unity's scatter form). */
#define FSPT_BLOOM_INTENSITY 0.05f
#define FSPT_BLOOM_SCATTER 0.7f
#define FSPT_BLOOM_LEVELS 6
#define FSPT_BLOOM_MAX_LEVELS 8
#define FSPT_BLOOM_CLAMP 1024.0f
/* k_bloom_tail (form 1) takes over at the first level k >= 1 with w_k h_k <= this many texels (and whose levels fit the LDS at 12 bytes a texel: about
 * 4/3 of the first one's).  2048: 60 x 34 of 1920 x 1080 and below, 30 KiB; the other candidate, 8192, adds 120 x 68 and needs 126 KiB of the 160. */
#define FSPT_BLOOM_TAIL_TEXELS 2048
/* Test hook: the production kernels on a host array - rgba W*H*4 floats, viewport vw x vh (0, 0 = the whole image), p NULL = defaults.  *n_out = n;
 * down_out = D_1 .. D_n and up_out = U_1 .. U_n, each level w_k*h_k*4 floats (.w = 0), one behind the other (room for fspt_bloom_texels(vw, vh, levels)
 * texels each); bloom_out = B, vw*vh*4 floats; mix_out = c' with denoise = 0, W*H*4 floats: the float32 the draw multiplies by the exposure (outside the
 * viewport and with n = 0: the source; .w = the source's).  Any output may be NULL. */
int fspt_bloom_eval(int device, const float *rgba, uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const fspt_bloom_params *p, uint32_t *n_out,
                    float *down_out, float *up_out, float *bloom_out, float *mix_out);
/* Host arithmetic, no device: n of a vw x vh viewport (*n_out, may be NULL); returns the texels of levels 1 .. n. */
uint64_t fspt_bloom_texels(uint32_t vw, uint32_t vh, uint32_t levels, uint32_t *n_out);
/* Measurement switches, process-wide: the form, 0 = one launch per level, 1 = k_bloom_tail below the threshold; and the threshold (0 = FSPT_BLOOM_TAIL_TEXELS
 * again), so that small shapes can run wholly in the tail or wholly outside it.  The bits are the same. */
int fspt_bloom_set_form(int form);
int fspt_bloom_set_tail_texels(uint32_t n);
/* GPU ms of the last bloomed draw on this target, from HIP events: ms[0] the down chain, ms[1] the tail, ms[2] the up chain, ms[3] k_draw_bloom.  Blocking. */
int fspt_bloom_last_ms(fspt_target *t, float ms[4]);
/* fspt_target_set_lights (fspt.h): FSPT_LIGHTS_EMITTERS lets each shading vertex spend its shadow ray on a
 * point of an emissive triangle (probability q = emitter_fraction, in (0, 1]; at most 0.875 with an environment map, 1
 * when the scene has none)
 * instead of the environment, MIS-weighted against BSDF hits on emitters: the same expected image as FSPT_LIGHTS_OFF, lower
 * variance where geometry lights the scene.  The scene's light table is built on the first call that turns the mode on
 * (fspt_scene_light_count: its entries - emissive triangles of non-zero estimated power - building it if needed).  Like
 * every setter it runs the recorded ticks first and keeps the accumulator.
 * Emitter light table, test hooks.
 * fspt_scene_light_table: builds the table if needed and reads it back.  Sizes first (any may be NULL): triangles,
 * entries, leaf slots; then the arrays (any may be NULL): weights[n_tris] (A * mean luma of 30 * emissive * diffuse over
 * 16 stratified points, 0 for a triangle that emits nothing), prob[n_lights] and alias[n_lights] (the float32 Vose table),
 * tris[n_lights] (an entry's triangle), pick[n_slots] (the probability the stored table realises for the slot's triangle,
 * 0 outside the table), slot_tri[n_slots] (a leaf slot's triangle). */
int fspt_scene_light_table(fspt_scene *scene, uint32_t *n_tris, uint32_t *n_lights, uint32_t *n_slots, float *weights,
                           float *prob, uint32_t *alias, uint32_t *tris, float *pick, uint32_t *slot_tri);
/* the device's emitter sample for n queries of 10 floats (ro.xyz, n.xyz, u0, u1, u2, u3; u0 - the strategy value - is not
 * used, u1 is the alias draw v itself): tri[i] = the sampled entry's triangle, out[8 i ..] = point.xyz, pdf_L (solid angle, realised selection
 * probability), Le.rgb, n . w.  FSPT_E_STATE when the scene has no emitter. */
int fspt_light_sample_eval(fspt_scene *scene, const float *in, uint32_t n, int32_t *tri, float *out);
/* pure host function: the Vose alias table (float64, stored float32) of n weights (finite, >= 0, some > 0) */
int fspt_light_alias_table(const float *weights, uint32_t n, float *prob, uint32_t *alias);
/* The GPU builder's table (fspt_scene_set_light_builder), in integers so that no summation order shows:
 * q_e = max(1, rint(w_e / w_max 2^32)), T = sum q, mass m_e = n q_e against a bucket of T; the lights (m < T) and the heavies
 * in entry order with their inclusive deficits D_j and excesses X_k (128-bit); light l_j keeps m and is aliased to the first
 * heavy with X_k > D_{j-1}; heavy h_k keeps r = T + X_k - D_{j*(k)}, j*(k) = #{j : D_{j-1} < X_k}, and is aliased to h_{k+1}
 * when r < T; prob = (float)(r / T); light_p[e] = (float)((prob_e + 2^-40 sum over the entries aliased to e of
 * (2^40 - floor(prob_j 2^40))) / n).  At most 2^23 entries.  tests/lighttable_ref.py restates it.
 * fspt_light_alias_table_gpu, test hook: that table of n raw weights (finite, >= 0, some > 0; a weight of 0 is kept as an
 * entry with q = 0) on HIP device `device`; prob, alias, light_p hold n values (any may be NULL).
 * fspt_scene_light_build_stats: what the scene's last table build - of either builder - moved over the bus, and its GPU time
 * from HIP events around its device work (the host builder's span includes the host's work between its two launches).
 * Zeros before the first build.  Blocking. */
int fspt_light_alias_table_gpu(int device, const float *weights, uint32_t n, float *prob, uint32_t *alias, float *light_p);
int fspt_scene_light_build_stats(fspt_scene *scene, uint64_t *bytes_d2h, uint64_t *bytes_h2d, float *ms);
/* JPEG encoder, test hooks.  fspt_jpeg_coefficients_eval: stage one alone - the quantised coefficients of
 * fspt_jpeg_encode's arguments (host pointers), 64 int16 per block in zig-zag order, blocks MCU-major: per MCU Y Cb Cr
 * (4:4:4) or Y00 Y01 Y10 Y11 Cb Cr (4:2:0); coef_out holds 64 * blocks values.  fspt_jpeg_last_ms: the three stages
 * (blocks, entropy, offsets + pack) of the last fspt_jpeg_encode / _encode_device call from HIP events, and (or NULL) the
 * bytes it brought to the host. */
int fspt_jpeg_coefficients_eval(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, int16_t *coef_out);
int fspt_jpeg_last_ms(float ms[3], uint64_t *bus_bytes);
/* PNG encoder.  FSPT_PNG_CHUNK: the bytes of the filtered stream one deflate chunk (one workgroup, one IDAT)
 * takes when fspt_png_params.chunk_bytes is 0; 8.20 has the time and size tables it was chosen from.
 * fspt_png_filtered_eval: stage one alone - the filtered stream of fspt_png_encode's arguments (host pointers), h rows of
 * 1 + w * channels bytes.  fspt_png_last_ms: the three stages (filter, deflate, offsets + pack) of the last fspt_png_encode /
 * _encode_device call from HIP events, and (or NULL) the bytes it brought to the host. */
#define FSPT_PNG_CHUNK 16384u
int fspt_png_filtered_eval(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *stream_out);
int fspt_png_last_ms(float ms[3], uint64_t *bus_bytes);
/* OpenEXR encoder.  FSPT_EXR_CHUNK: the bytes of a block's predicted stream one deflate chunk (one workgroup)
 * takes when fspt_exr_params.chunk_bytes is 0; 8.21 has the table it was chosen from.  fspt_exr_set_form: where a block that
 * falls back to raw takes its bytes from - 0 (default) = k_exr_pack converts them again from the floats, 1 = k_exr_rows keeps
 * a raw copy of every block next to the predicted one.  The files are the same.  fspt_exr_last_ms: the three stages (rows,
 * deflate, offsets + pack) of the last fspt_exr_encode / _encode_device and the bytes that call brought to the host. */
#define FSPT_EXR_CHUNK 8192u
int fspt_exr_set_form(int form);
int fspt_exr_last_ms(float ms[3], uint64_t *bus_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FSPT_TUNING_H */
