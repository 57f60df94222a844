// fspt_device.hpp — device data layouts, launch parameter blocks and launcher declarations shared by the two kernel
// files (fspt_kernels.hip: whatever reads a DScene; fspt_post.hip: whatever reads only images) and the host side of the
// C ABI (fspt_api.cpp, fspt_post.cpp, the schedulers, fspt_multi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fspt {

// Traversal references.  ref >= 0: interior node index (native numbering,
// root = 0); ref < 0: leaf, leaf record = ~ref; REF_SENTINEL: empty stack.
constexpr int REF_SENTINEL = (int)0x80000000;

constexpr float MAX_T = 100000.0f;       // tracer.fs:10
constexpr float EPSILON = 0.000001f;     // tracer.fs:11
constexpr float M_PI_F = 3.14159265f;    // tracer.fs:12
constexpr float M_TAU_F = M_PI_F * 2.0f; // tracer.fs:13
constexpr float INV_PI_F = 1.0f / M_PI_F;
constexpr int MAX_PATH_ITERS = 64;       // cap on tracer.fs:488's unbounded i--

// Textures (environment, atlas layers with res > 1) are stored in tiles of 8 x 4 texels = 128 bytes = one cache line
// (rows of tiles, a tile's texels row-major), images padded to whole tiles.
#ifndef FSPT_TEX_TILE_W_LOG2
#define FSPT_TEX_TILE_W_LOG2 3
#define FSPT_TEX_TILE_H_LOG2 2
#endif
constexpr int TEX_TILE_W_LOG2 = FSPT_TEX_TILE_W_LOG2, TEX_TILE_H_LOG2 = FSPT_TEX_TILE_H_LOG2; // 0, 0 = plain row-major (A/B)
constexpr int TEX_TILE_W = 1 << TEX_TILE_W_LOG2, TEX_TILE_H = 1 << TEX_TILE_H_LOG2;

#ifndef FSPT_ENV_APRON
#define FSPT_ENV_APRON 1 // the environment map in overlapping tiles (fspt_kernels.hip env_taps); 0: disjoint tiles (A/B)
#endif
constexpr uint32_t LAYER_CONST = 0xFFFFFFFFu;
// Material texture set (3 x uint4 per set, DScene::tex_sets; a triangle's hit record names its set): the four atlas
// layers a shading event samples at one uv (tracer.fs:453-456: diffuse, emissive, metallic-roughness, normal), resolved
// at scene creation (layer = clamp(floor(id + 0.5)), the same binary32 arithmetic):
//   [0] = kind, base of the interleaved image (in 128-byte tiles), 0, 0
//   [1] = the four layers' texel where the layer is constant (every flat colour)
//   [2] = SEPARATE form: per layer the base of its tiled single-layer image (in 128-byte tiles) or LAYER_CONST
constexpr uint32_t TEXSET_CONST = 0u;    // four flat colours: no fetch at all
constexpr uint32_t TEXSET_SEPARATE = 1u; // image layers fetched from single-layer images (8 x 4-texel tiles)
constexpr uint32_t TEXSET_QUAD = 2u;     // the four layers interleaved texel by texel: 4 x 2-texel tiles of 16-byte texels

constexpr int NODE_F4 = 4;   // 64-byte two-child node = 4 x float4
constexpr int QUAD_F4 = 8;   // 128-byte two-LEVEL node (below) = 8 x float4 = one cache line
constexpr int TRI_FLOATS = 9;  // pre-edged triangle: v1, e1 = v2 - v1, e2 = v3 - v1 (tracer.fs:301-302 precomputed)
constexpr int HITREC_F4 = 12; // 192-byte hit record (shading) = 12 x float4 = exactly 3 cache lines

// Node (64 B), the slab bounds of both children in the pairs the packed-FP32 box test consumes (fspt_kernels.hip node_test):
//                f4[0] = lmin.xy lmax.xy   f4[1] = rmin.xy rmax.xy
//                f4[2] = lmin.z lmax.z rmin.z rmax.z   f4[3] = (int) left_ref right_ref 0 0
//   (tracer.fs:374-378 fetches the header of `current` and then, dependently,
//    the boxes of both children: 3 round trips; here one.)
// Two-level node ("quad", 128 B = ONE cache line, one per interior node N with children L, R; DScene::quads): what a lane
//   needs to take TWO of the reference's traversal steps (tracer.fs:372-392 at idx = N, then at idx = the child it
//   descends into) on one memory round trip - for the launches that are bundles of DEPENDENT chains (tail kernel, small
//   trace launches, the 1 M-triangle scene), where a step costs a cache-miss latency, not a request slot:
//                f4[0..2] = the node record of L (the boxes of L's children LL, LR, in the layout above)
//                f4[3]    = (int) LL_ref LR_ref L_ref R_ref
//                f4[4..6] = the node record of R (boxes of RL, RR)      f4[7] = (int) RL_ref RR_ref 0 0
//   The boxes of L and R themselves - what the step at N tests - are NOT stored: bvh.js builds every node's box from ITS
//   triangles' vertices (BoundingBox.addNode, bvh.js:120-126), so box(L) = union(box(LL), box(LR)) exactly, in binary32
//   (min / max are exact and rounding is monotone); the lane derives them with 12 v_min / v_max.  fspt_scene_create
//   VERIFIES that identity bit for bit on every interior node of the arrays it is given and builds no quads otherwise
//   (DScene::quads = NULL: every launch then uses the 64-byte nodes).  A child that is a leaf has no children: its part
//   holds its own box twice (the union is the box).  Same nodes tested against the same t in the same order, the far
//   child pushed as a child, the far grandchild as a grandchild: the node sequence, the counters and every result are
//   those of the one-level walk.
// Leaf record (LEAF_SIZE x 36 B = 144 B for LEAF_SIZE 4): the LEAF_SIZE consecutive triangles the reference's processLeaf
//   reads from the leaf's first one (tracer.fs:355-364 - a leaf with fewer triangles reads on into its successors, the
//   last leaves into the "-1" padding, main.js:150-152), pre-edged, COMPONENT-major: floats [c * LEAF_SIZE + i] =
//   component c (v1.xyz e1.xyz e2.xyz) of triangle i.  For LEAF_SIZE 4 that is nine 16-byte loads whose halves are the
//   operand pairs of the two-triangles-at-once intersection (ray_tri2).  A leaf's ref is ~(its record index);
//   slot_tri[record * LEAF_SIZE + i] = that triangle's index in the reference's order (what tracer.fs:360 reports).
// HitRec (192 B, 64-byte aligned = exactly 3 cache lines per shaded hit), one per leaf SLOT - the traversal's hit index
//   addresses it directly, no translation on the path (a triangle that is also an earlier leaf's over-read has a copy there):
//   floats 0..8 the same v1,e1,e2; 9..35 normTex record (n,t,bt per vertex,
//   main.js:383-385); 36..41 uv (main.js:386); 42 (uint bits) the material texture set of the triangle's four
//   layer ids (main.js:377-379); 46 ior; 47 dielectric.
struct DScene {
  const float4 *nodes;
  const float4 *quads;  // two-level nodes, indexed like `nodes` (NULL: the scene's boxes are not unions of their children's)
  const float *leaves;  // leaf records (see above)
  const uint32_t *slot_tri; // leaf slot -> triangle index
  const float4 *hitrec; // 12 x float4 per triangle
  const uint32_t *atlas; // RGBA8 texels of the single-layer images (SEPARATE sets), each tiled (TEX_TILE_*)
  const uint4 *atlas4;   // interleaved four-layer images (QUAD sets)
  const uint4 *tex_sets; // 3 x uint4 per material texture set
  const uint32_t *env;   // RGBE texels, tiled (NULL = black default environment)
  const uint4 *bins;
  uint32_t atlas_res, atlas_layers;
  uint32_t n_tex_sets;
  uint32_t env_w, env_h;
  uint32_t n_bins;
  uint32_t leaf_size;
  int root_ref;
  uint32_t stack_n; // LDS stack entries per lane (tree depth + 1)
  uint32_t n_top;   // nodes [0, n_top) are the top of the tree in breadth-first order
  // emitter light table (fspt_target_set_lights; built on the first target that turns the mode on, NULL before):
  //   light_alias[i] = (prob_i bits, alias_i): Vose alias table over the n_lights entries
  //   light_rec[4 i .. 4 i + 3] = 64-byte light record: v1.xyz e1.xyz e2.xyz, uv0 uv1 uv2, (uint bits) texture set
  //   light_p[i] = the probability the float32 table realises for entry i; light_pick[slot] = that of the slot's triangle (0: none)
  const uint2 *light_alias;
  const float4 *light_rec;
  const float *light_p;
  const float *light_pick;
  uint32_t n_lights;
};

struct CameraP {
  float P[3];
  float I[3];
  float fov_scale;
  float lens[2];
};

// the opt-in camera models (fspt.h fspt_camera_model_params; the rule: fspt_camera_model.hpp); CAM_* = FSPT_CAMERA_*
enum { CAM_PINHOLE = 0, CAM_ORTHO = 1, CAM_FISHEYE = 2, CAM_EQUIRECT = 3, CAM_STEREO = 4 };
struct CameraModelP { int model; float angle; float ipd; };

struct TraceP {
  DScene scene;
  uint32_t W, H;
  uint32_t vw, vh; // gl.viewport(0, 0, vw, vh): only these pixels are drawn (main.js:744,761)
  uint32_t tick;
  float rand_base;     // drawTracer's randBase
  float rand_base_cam; // drawCamera's randBase (fused ray generation only)
  float env_theta;
  uint32_t num_bounces;
  CameraP cam;
  const float4 *ray_pos; // ray buffers (two-call form)
  const float4 *ray_dir;
  float4 *accum;
  uint32_t *work_counter;       // zeroed before the launch
  unsigned long long *counters; // 6 x u64 (COUNT variants) or NULL
  // sharding
  uint32_t shard, n_shards, tile;
  uint32_t tiles_x, tiles_y, n_owned_tiles;
  const uint32_t *tile_list; // NULL: the shard's tiles round-robin; else n_owned_tiles tile indices (fspt_render_adaptive)
  uint32_t sampler;  // FSPT_SAMPLER_*: which instantiation launch_trace picks
  uint32_t smp_seed; // FSPT_SAMPLER_SOBOL's seed
  uint32_t lights;   // 1: the FSPT_LIGHTS_EMITTERS instantiations (only when scene.n_lights > 0)
  float light_q;     // q, the probability a vertex's NEE goes to an emitter (emitter_fraction, 1 without an environment map)
};

struct IntersectP {
  DScene scene;
  const float *rays; // 6 floats per ray
  uint32_t n;
  uint32_t wide;     // walk the two-level nodes (scene.quads must exist)
  float *t_out;
  int *index_out;
  uint32_t *steps_out;
  uint32_t *leaves_out;
};

// ---------------------------------------------------------------------------
// Wavefront pipeline (fspt_render's default): the same per-path arithmetic cut
// into queue-driven kernels so that every lane of a wave does the same kind of
// work:  primary (ray generation + camera-ray traversal + its shading) -> [ trace <-> logic ] x rounds
//        [-> tail: the last few live paths run to completion in one kernel] -> resolve.
//   slot s = w * n_batch + j  : sample of tick (first_tick + j) for work index w
//   (pixel via work_to_pixel); a batch holds n_batch ticks.  Pixel-major on purpose:
//   the ticks of one pixel are neighbours in the primary launch, so a wave's camera rays are
//   near-identical (coherent traversal, broadcast node loads) and shade the same triangle.
// Path state is DENSE: round r's logic launch writes the state of its survivors to consecutive indices
//   k = 0 .. n_r-1 of state set (r & 1) (the other set is its input), so every later access - the trace kernel's
//   ray loads and result stores, the next round's loads - touches whole cache lines.  (Round 1 kept the state at
//   the path's fixed slot: after a few rounds the survivors are sparse and every 16-byte access moved a 64-byte
//   line - 4x the bytes, profiles/r01.)  float4 SoA arrays, per set:
//   A  ro.xyz, slot (uint bits)          B  rd.xyz, flags (bits: 0-7 bounce, 8-15 iters, 16 primary, 17 hasShadow, 18 colour is +0)
//   C  accumulatedReflectance.xyz, weights.y
//   E  color.xyz, -   (only touched while the colour is non-zero)
//   D  envDir.xyz, weights.x             P  reflectance*envThroughput.xyz, -     (only when the path has a NEE shadow ray)
//   FSPT_LIGHTS_EMITTERS instantiations: P.w = the shadow ray's t bound (MAX_T: environment; below: an
//   emitter point).  A path whose last vertex could sample an emitter (q > 0) has flag WF_FLAG_LQ and D / P are written
//   whatever its shadow ray: D.w then holds q / pb (pb = that vertex's bsdfPdf: the MIS weight of an emitter its
//   extension ray hits) and weights.x is 1 (folded into P.xyz).
// Per round (indexed like the state): hit (t, index) of the extension ray, shadow_hit = index of the NEE ray.
// fin[slot]: the finished sample colour, slot-major (a wave's finishing paths are neighbours).
// ---------------------------------------------------------------------------
constexpr int WF_MAX_BATCH = 128;
constexpr int WF_HIT_TERMINAL = -2; // hit[k].index of an extension ray that hit something but whose path has no bounce left
constexpr int WF_HIT_PENDING = -3;  // hit[k].index of a path whose traversal was SUSPENDED by the trace launch (hit[k].t = its record)
constexpr uint32_t WF_FLAG_PRIMARY = 1u << 16, WF_FLAG_SHADOW = 1u << 17, WF_FLAG_COLZERO = 1u << 18;
// FSPT_LIGHTS_EMITTERS instantiations only: bit 15 (the top bit of the iteration count, which never exceeds
// MAX_PATH_ITERS = 64 and so is read through a 7-bit mask there): D.w holds q / pb, see above
constexpr uint32_t WF_FLAG_LQ = 1u << 15;
static_assert(MAX_PATH_ITERS < 128, "WF_FLAG_LQ: the iteration count must fit 7 bits");
// Suspended traversals (k_wf_trace): what a trace launch costs beyond its work is its LONGEST ray - a dependent chain of
// up to a few hundred node fetches that a handful of lanes walk while the rest of the chip idles (~0.2 ms per launch,
// profiles/r03).  A wave that can get no more work and has been walking for WfP::susp_budget steps writes the state of
// its unfinished rays (node, t, hit, the LDS stack) to a record and ends; k_wf_carry (in front of the logic launch) moves
// such a path on to the next state set unchanged (flag WF_FLAG_SUSP: the next trace launch must not start its rays afresh), and the next
// trace launch resumes the records FIRST, beside its bulk of new rays.  Same traversal, same result; a path lags one
// round per suspension (at most WF_LAG_MAX: the count lives in bits 20-22 of the flags).
constexpr uint32_t WF_FLAG_SUSP = 1u << 19;
#ifndef FSPT_WF_LAG_MAX
#define FSPT_WF_LAG_MAX 4
#endif
constexpr uint32_t WF_LAG_SHIFT = 20, WF_LAG_MASK = 7u, WF_LAG_MAX = FSPT_WF_LAG_MAX;
// Sobol sampler only (fspt.h FSPT_SAMPLER_SOBOL): bits 23-31 of the flags hold half the path's sampler dimension count
// (always even, at most 4 + 12 * MAX_PATH_ITERS = 772 with emitter sampling: 9 bits)
constexpr uint32_t WF_DIM_SHIFT = 23;
static_assert(((4u + 12u * MAX_PATH_ITERS) >> 1) < (1u << (32u - WF_DIM_SHIFT)), "WF_DIM_SHIFT: dimension count does not fit");
constexpr int WF_SUSP_HEADER = 8; // ints before the stack entries of a record: state index, node, t, hit, sp | ray << 8, shadow result, -, -
#ifndef FSPT_WF_HEADS
#define FSPT_WF_HEADS 16
#endif
constexpr int WF_HEADS = FSPT_WF_HEADS; // work-pool heads of the trace kernel (one per item segment; waves steal from the others)

#ifndef FSPT_WF_HEAD_STRIDE
#define FSPT_WF_HEAD_STRIDE 64 // uint32 words between two pool heads (256 bytes)
#endif
constexpr int WF_HEAD_STRIDE = FSPT_WF_HEAD_STRIDE;
struct alignas(128) WfCounts { // one per round, zeroed before the batch
  uint32_t n_ext;          // live paths written by this round's primary / logic launch
  uint32_t n_susp;         // traversals this round's trace launch suspended (records for the next one)
  uint32_t pad[30];
};
// Trace / tail kernel work-pool heads: WF_HEADS per round, each in a memory line (and channel) of its own
// (WfP::heads[(round * WF_HEADS + stripe) * WF_HEAD_STRIDE]): device-scope atomics execute at the memory side and
// same-LINE atomics serialise like same-address ones (~15 ns each) - 16 heads packed in one 64-byte line behaved
// exactly like a single head (profiles/r02/ab_trace_pool_heads.log).

struct WfSet { float4 *A, *B, *C, *E, *D, *P; };

// ---------------------------------------------------------------------------
// Streaming scheduler (fspt_target_set_pipeline code 2): a FIXED pool of path state that is kept full.
//   The (work index, tick) samples of a run of n_batch ticks are numbered pixel-major exactly like a batch's slots
//   (g = w * n_batch + j) and cut into UNITS of 64 work indices x n_batch ticks (one 8x8 pixel patch, all its ticks).
//   Iteration i:   plan(i)    takes as many units from the device-side cursor as are GUARANTEED to fit the state set:
//                             cap - (live paths of set i-1)  - every live path may survive, every new sample may too
//                  primary(i) camera rays + their traversal + shading for those units; survivors -> set i&1
//                  logic(i)   one S step for the live paths of set (i-1)&1; survivors -> set i&1 (same counter)
//                  trace(i)   the rays of set i&1
//                  resolve    folds the units whose every path has ended (generated >= num_bounces iterations ago;
//                             MAX_PATH_ITERS when a material can refract) into the accumulator, ticks in order
//   so every trace / logic launch is about the size of the pool whatever the call's tick count, paths of all ages
//   mixed; path state is cap x 204 bytes + a ring of finished colours, not (pixels x ticks) x 216 bytes.  plan /
//   primary / resolve run on a second stream beside the previous iteration's trace.  After the last iteration the tail
//   kernel runs whatever is alive to completion AND generates whatever the cursor has not handed out (the host only
//   estimates the iteration count; nothing depends on the estimate but speed).
//   fin is a RING of ring_slots entries (a multiple of the unit size, > everything in flight); the slot id a path
//   carries is its ring position (slot % n_batch is still its tick).
// ---------------------------------------------------------------------------
constexpr int WF_RING = 4;    // iterations whose counters / pool heads exist at the same time (even: set parity = index parity)
constexpr int WF_HIST = 128;  // cursor history kept for the resolve (> MAX_PATH_ITERS + 2)
struct alignas(128) WfStreamCtl {
  uint32_t cursor;       // next unit nobody has generated yet (may overshoot the run's units, work_total / 64, at the very end)
  uint32_t reserved;
  uint32_t n_iters;      // statistics of the run, read back by the host without waiting (tunes its iteration estimate)
  uint32_t last_gen_it;  // last iteration that took units
  uint32_t max_live;
  uint32_t fin_gen_units; // units the finishing tail launch had to generate itself
  uint32_t pad[26];
  unsigned long long sum_live;
  unsigned long long pad2[15];
  uint32_t plan_start[WF_RING], plan_units[WF_RING]; // iteration i's chunk of units
  uint32_t hist[WF_HIST]; // cursor after plan(i), i % WF_HIST
};

struct WfP {
  uint32_t gen_rays; // primary launch: 1 = camera.fs in the kernel, 0 = read the ray buffers (two-call form)
  uint32_t lds_top; // top-of-tree nodes k_wf_trace keeps in LDS (<= scene.n_top; set by launch_wf)
  DScene scene;
  WfSet set[2];
  float *fin;  // finished sample colours [slot][3]
  float2 *hit;
  int *shadow_hit;
  WfCounts *counts;
  uint32_t *heads; // pool heads, see above
  uint32_t round;  // batch scheduler: the round (1 = primary); stream: the iteration
  // which counter / state set a launch reads and writes (batch: round - 1 / round; stream: iteration mod WF_RING)
  uint32_t cnt_in, cnt_out, set_in, set_out;
  WfStreamCtl *ctl;     // NULL = batch scheduler
  uint32_t ring_slots;  // entries of the fin ring (batch: n_batch * work_total = no wrap)
  uint32_t cap;         // stream: paths a state set holds
  uint32_t take_max;    // stream: units plan(i) takes at most
  int res_from, res_to; // resolve (stream): fold the units between hist[res_from] (< 0: unit 0) and hist[res_to] (-2: all)
  uint32_t finish;      // tail (stream): also generate what the cursor has not handed out
  uint32_t serial;      // plan (stream): it runs AFTER logic(i) (one HIP stream) and sees the real survivors in counts[cnt_out]
  int *susp[2];         // suspended-traversal records: trace(i) writes susp[cnt_out & 1], resumes susp[cnt_in & 1]
  uint32_t susp_stride; // ints per record (WF_SUSP_HEADER + stack entries, a multiple of 4)
  uint32_t susp_budget; // traversal steps a wave walks on after its last refill before it suspends (0: never)
  // batch scheduler, resolve launch (the last kernel of a batch): block 0 copies the rounds' live-path counts to
  // `live_out` (pinned host memory: the tail heuristic's statistics) and clears the counters and pool heads of
  // `zero_rounds` rounds for the next batch - instead of two fill commands and a copy command behind every batch
  uint32_t *live_out;
  uint32_t zero_rounds;
  uint32_t carry_blocks; // logic launch: this many trailing blocks do k_wf_carry's work instead (one launch less per round)
  uint32_t tail_slice;    // tail kernel: traversal steps of a lane per T phase (0: WF_TAIL_SLICE); the host picks it by scene size
  uint32_t tail_adaptive; // tail kernel with its `wide` bit set: two-level nodes only once the wave's list is used up (k_wf_tail WIDE = 2)
  uint32_t wide;        // bit k: kernel class k (WF_K_PRIMARY / WF_K_TRACE / WF_K_TAIL) walks the two-level nodes (scene.quads; same results)
  uint32_t primary_r;   // k_wf_primary: 1 = one traversal per lane, 2 = per-lane refill over 2 x 64 samples per wave (same results)
  uint32_t W, H;
  uint32_t vw, vh; // viewport, as in TraceP
  uint32_t work_total; // work indices per tick (owned tiles * tile^2)
  uint32_t n_batch;    // ticks in this batch (<= WF_MAX_BATCH)
  uint32_t first_tick;
  float rb_cam[WF_MAX_BATCH];
  float rb_trace[WF_MAX_BATCH];
  float env_theta;
  uint32_t num_bounces;
  CameraP cam;
  const float4 *ray_pos, *ray_dir; // ray buffers (two-call form, n_batch == 1)
  float4 *accum;
  unsigned long long *counters;
  uint32_t shard, n_shards, tile, tiles_x, tiles_y, n_owned_tiles;
  const uint32_t *tile_list; // as in TraceP
  uint32_t sampler;  // as in TraceP; a slot's sample index is first_tick + slot % n_batch
  uint32_t smp_seed;
  uint32_t lights;   // as in TraceP
  float light_q;
  uint32_t stash;    // k_wf_logic: entries of its LDS stash of shaded paths' rows (0: none; set by launch_wf)
};

// kernel classes; also the slots of fspt_last_stage_ms
enum { WF_K_PRIMARY = 0, WF_K_TRACE = 1, WF_K_LOGIC = 2, WF_K_RESOLVE = 3, WF_K_TAIL = 4, WF_K_KINDS = 5 /* timed classes */, WF_K_PLAN = 6 /* not timed */, WF_K_CARRY = 7 /* not timed */ };

// multi-device read-out: a shard's own pixels <-> a packed array in work-index order (work_to_pixel)
struct TilePackP {
  float4 *accum;   // full-size W x H accumulator
  float4 *packed;  // n_owned_tiles * tile^2 entries (channels 3: that many RGB triples, alpha = 1 on unpack, tracer.fs:517)
  uint32_t channels; // 0 / 4: RGBA, 3: RGB
  uint32_t W, H, vw, vh;
  uint32_t shard, n_shards, tile, tiles_x, tiles_y, n_owned_tiles;
  const uint32_t *tile_list; // always NULL (work_to_pixel reads it)
};

// guided denoiser (fspt_denoise.*)
struct FeatureP {
  DScene scene;
  uint32_t W, H;
  CameraP cam;
  uint32_t samples;
  uint64_t seed;  // the camera rays' randBase values: fspt_rand_base_next's stream from this state
  float4 *feat;   // 2 x float4 per pixel: (albedo.rgb, depth), (normal.xyz, coverage)
};
struct FeatureModelP { FeatureP f; CameraModelP cm; }; // k_features under a camera model (the pinhole camera's block is FeatureP)
// ID mattes (fspt_mattes): k_mattes traces k_features' rays; f.feat is not used.  Table a (and b, when the launch
// carries two kinds): one id per triangle, 3 x float4 per pixel of ranks, a 64-bit counter of lost samples.  Named members,
// not arrays: an array in the arguments indexed by a variable would be copied to scratch.
struct MatteP {
  FeatureP f;
  const uint32_t *ids_a, *ids_b;
  float4 *out_a, *out_b;
  unsigned long long *lost_a, *lost_b;
};
struct MatteModelP { MatteP m; CameraModelP cm; };
struct AtrousP {
  const float4 *src; // u^k, or (demod) the accumulator
  float4 *dst;
  const float4 *feat;
  uint32_t W, H;
  int step;          // 2^k
  int demod, remod;  // first iteration: u0 = c / max(a, 1e-3); last: out = a * u^K
  float sc_step;     // sigma_c * 2^-k (INFINITY: w_c = 1)
  float sn;          // sigma_n (0: w_n = 1)
  float sz_step;     // sigma_z * 2^k (INFINITY: w_z = 1)
  // variance-guided instantiation only (fspt_temporal_denoise_variance)
  const float *var;  // k_svgf_variance's output, read by the FIRST iteration; later ones carry the variance in src.w
  float sl;          // sigma_l in standard deviations (INFINITY: w_l = 1); sc_step is unused
  float *var_dst;    // the LAST iteration's output variance, which its (a u, 1) has no lane for (test hook), or NULL
};

// temporal accumulation (fspt_temporal_*)
constexpr int MOTION_FLOATS = 9;      // motion-origin snapshot: floats 0-8 (v1 e1 e2) of a slot's hit record
constexpr float TM_KIND_NONE = 0.0f;  // M.w: no previous frame, or the point lies behind the previous camera
constexpr float TM_KIND_HIT = 1.0f;
constexpr float TM_KIND_MISS = 2.0f;
constexpr float TM_SNAP = 1.0f / 128.0f; // a sample coordinate this close to an integer IS that integer
struct TemporalGP {
  DScene scene;
  uint32_t W, H;
  CameraP cam;          // this frame's camera (lens unused: the centre ray is a pinhole ray)
  CameraP prev;         // the previous frame's
  uint32_t has_prev;    // 0: first frame after create / reset - M.w = TM_KIND_NONE everywhere
  const float *origin;  // motion-origin snapshot (MOTION_FLOATS floats per leaf slot) or NULL: static geometry
  float4 *g;            // 2 x float4 per pixel: (t, slot bits, bv, bw), (macroNormal.xyz, hit)
  float4 *m;            // float4 per pixel: (sx, sy, |v| or 0, kind)
};
struct TemporalBP {
  const float4 *accum;  // I: the mean of n samples of this frame
  const float4 *m, *g;  // this frame's motion and G-buffer
  const float4 *hist, *g_prev; // the previous frame's result and G-buffer (unused when has_hist = 0)
  float4 *out;          // the new history: rgb, length
  uint32_t W, H;
  uint32_t has_hist;
  float n;              // acc_ticks
  float alpha, max_history, depth_tol, normal_cos;
  // moments instantiation only (fspt_temporal_set_moments)
  const float4 *feat;      // the features: feat[2 i].xyz = the albedo the input is demodulated by
  const float2 *mom_hist;  // the previous call's (M1, M2) (unused when has_mom = 0)
  float2 *mom_out;
  uint32_t has_mom;
  // fast-history instantiations only (fspt_temporal_set_clamp)
  const float4 *fast_hist; // the previous call's fast history: rgb, length (unused when has_fast = 0)
  float4 *fast_out;
  uint32_t has_fast;
  float fast_history;      // its cap, in samples: takes max_history's place in the colour's recursion
};
// SVGF variance estimate (k_svgf_variance)
constexpr float SVGF_MIN_HISTORY = 4.0f; // effective frames from which the temporal moments alone give the variance
constexpr int SVGF_WINDOW = 3;           // the spatial fallback's window reaches this far: 7 x 7
struct SvgfVarP {
  const float4 *hist;  // the history after the blend: .w = its length
  const float2 *mom;   // (M1, M2)
  const float4 *feat;
  float *var;          // W*H
  uint32_t W, H;
  float n;             // acc_ticks of the accumulate that wrote hist
  float sn, sz;        // sigma_normal, sigma_depth (step 1)
};
// history clamp (k_temporal_clamp): hist.rgb into mu +- sigma_scale sd of the fast history's 5 x 5 window
constexpr int CLAMP_RADIUS = 2;
struct ClampP {
  float4 *hist;        // the long history after the blend, clamped IN PLACE (.w untouched) - or, with out != NULL, only read
  const float4 *fast;  // the fast history after the blend
  float4 *out;         // test hook: the result goes here instead, and (lo.rgb, 0) / (hi.rgb, 0) to lo / hi where not NULL
  float4 *lo, *hi;
  uint32_t W, H;
  float sigma_scale;   // finite (+inf never launches)
};

// adaptive sampling (fspt_render_adaptive): after n ticks, with the snapshot S taken after m < n ticks
struct AdaptiveP {
  const float4 *accum; // I = the mean of n ticks
  float4 *snap;        // S = the mean of the first m
  const uint32_t *list_in; // the n_in active tiles, ascending
  uint32_t *list_out;
  uint32_t n_in;
  uint32_t *n_out;     // the length of list_out (one word)
  uint32_t *count;     // per tile: the tick count it retired with (written when it retires)
  double *err;         // per tile: E_T (k_adaptive_error) / the E_T that retired it
  uint32_t W, vw, vh, tile, tiles_x;
  uint32_t n, m;       // m = 0: only the snapshot (S := I)
  uint32_t refresh;    // 1: S := I for the tiles of the list in the same pass
  uint32_t min_ticks, max_ticks;
  double target;
};

// auto-exposure (fspt_target_set_auto_exposure)
constexpr uint32_t EXPOSURE_BINS = 256; // 32 octaves from 2^-16, 8 sub-bins each
struct ExposureP { float key, low, high, adapt_up, adapt_down, min_log2, max_log2; }; // fspt_exposure_params, validated
struct ExposureState {      // 32 bytes of device memory (fspt_exposure_state): what k_exposure_resolve writes and k_draw_auto reads
  float exposure;           // (float)exp2(log2_exposure); 1 until the first metering that saw a pixel
  uint32_t valid;           // there is a previous state to adapt from
  uint32_t metered, pad;    // N of the last metering with N > 0
  double log2_exposure, log2_mean;
};
// bloom (fspt_target_set_bloom; the rule: fspt_tuning.h)
constexpr uint32_t BLOOM_MAX_LEVELS = 8;          // FSPT_BLOOM_MAX_LEVELS
constexpr size_t BLOOM_TAIL_LDS_MAX = 160 * 1024; // what one workgroup may hold on gfx950
constexpr int BLOOM_FORM = 0;                     // shipped: 0 = one launch per level, 1 = the fused tail (cost table)
constexpr uint32_t BLOOM_TAIL_TEXELS = 2048;      // FSPT_BLOOM_TAIL_TEXELS: 60 x 34 of 1920 x 1080 and below, 30 KiB of LDS
struct BloomP { float intensity, scatter; uint32_t levels; }; // fspt_bloom_params, validated
struct BloomDraw { const float4 *u1; uint32_t w1, h1, vw, vh; float intensity; }; // what k_draw_bloom needs: U_1, its size, the viewport
struct BloomTailP { float4 *lvl; uint32_t w, h, below; float scatter; float4 *dbg_down, *dbg_up; };
struct BloomPlan {          // the pyramid of a vw x vh viewport
  uint32_t n;               // levels below level 0: min(levels, the first level with a side of 1); 0 = the plain draw
  uint32_t w[BLOOM_MAX_LEVELS + 1], h[BLOOM_MAX_LEVELS + 1];
  size_t off[BLOOM_MAX_LEVELS + 2]; // level k's first texel in the pyramid, k >= 1
  size_t texels;            // of levels 1 .. n
  uint32_t tail;            // the level k_bloom_tail starts at, 0 = no tail
  size_t tail_lds;          // its LDS bytes
};

// ---------------------------------------------------------------------------
// launchers of fspt_kernels.hip: the renderers, their draw and read-out helpers, the light table
// ---------------------------------------------------------------------------
hipError_t launch_trace(const TraceP &p, bool gen_rays, bool count, int num_cus, hipStream_t stream);
// count: 0 = production kernels; 1 = counting variants doing the reference's work (NEE shadow rays traced to the closest
// hit, tracer.fs:501); 2 = counting variants of the production work (shadow rays stop at the first hit)
hipError_t launch_wf(int kernel, const WfP &p, int count, int num_cus, hipStream_t stream);
extern int g_logic_stash; // k_wf_logic's LDS stash (fspt_logic_set_stash): -1 the library's choice, 0 none, n at most n entries
size_t wf_max_stack_entries(); // deepest tree (entries per lane) whose traversal stacks fit the LDS of every kernel
hipError_t launch_tile_pack(const TilePackP &p, bool unpack, hipStream_t stream);
hipError_t launch_bvh_test(const TraceP &p, hipStream_t stream);
// light table build (fspt_target_set_lights): w[i] for the triangle in leaf slot slots[i]; with rec != NULL
// also its 64-byte light record rec[4 i .. 4 i + 3]
hipError_t launch_light_weights(const DScene &S, const uint32_t *slots, uint32_t n, float *w, float4 *rec, hipStream_t stream);
// fspt_light_sample_eval: 10 floats per query (ro.xyz, n.xyz, u0..u3) -> entry index, 8 floats (x.xyz, pdf_L, Le.rgb, n . w)
hipError_t launch_light_eval(const DScene &S, const float *in, uint32_t n, int *entry, float *out, hipStream_t stream);

// ---------------------------------------------------------------------------
// launchers of fspt_passes.hip: the stand-alone passes and test hooks, which no renderer calls
// ---------------------------------------------------------------------------
// the ray buffers of a tick under camera model cm.model (CAM_PINHOLE: camera.fs as a pass; a missing model or sampler: hipErrorInvalidValue)
hipError_t launch_camera(uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const CameraP &cam, const CameraModelP &cm, float rand_base,
                         float4 *pos, float4 *dir, hipStream_t stream, uint32_t sampler, uint32_t smp_seed, uint32_t sample);
// the Sobol sampler's value for n (pixel, sample, dim) triples (fspt_sampler_eval)
hipError_t launch_sampler_eval(uint32_t seed, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, uint32_t n,
                               float *out, hipStream_t stream);
hipError_t launch_intersect(const IntersectP &p, hipStream_t stream);
hipError_t launch_math(int op, const float *a, const float *b, uint32_t n, float *out, hipStream_t stream);
// one workgroup per active tile: E_T = mean over the tile's viewport pixels and 3 channels of m (I - S)^2 / ((n - m)(I^2 + 0.01))
hipError_t launch_adaptive_error(const AdaptiveP &p, hipStream_t stream);
// one workgroup: retire the tiles of list_in whose E_T decides it, list the rest in list_out (same order), *n_out
hipError_t launch_adaptive_select(const AdaptiveP &p, hipStream_t stream);
// the two passes of the image chain that trace rays (fspt_post.cpp launches them)
hipError_t launch_features(const FeatureP &p, const CameraModelP &cm, hipStream_t stream); // (the guides follow the camera model)
hipError_t launch_mattes(const MatteP &p, const CameraModelP &cm, hipStream_t stream);    // kinds: table a alone (ids_b NULL) or both; zeroes the lost counters first
hipError_t launch_temporal_gbuffer(const TemporalGP &p, hipStream_t stream);

// ---------------------------------------------------------------------------
// launchers of fspt_post.hip: whatever reads only images
// ---------------------------------------------------------------------------
// k_draw, or with state != NULL k_draw_auto, with bloom != NULL k_draw_bloom (<true> where state != NULL too)
hipError_t launch_draw(const float4 *acc, uint32_t W, uint32_t H, float exposure, float saturation, int denoise, float max_sigma,
                       float scale, uint32_t *out, const ExposureState *state, const BloomDraw *bloom, hipStream_t stream);
hipError_t launch_atrous(const AtrousP &p, bool var, hipStream_t stream); // (var: the variance-guided instantiation)
hipError_t launch_temporal_blend(const TemporalBP &p, hipStream_t stream); // (p.mom_out != NULL: the moments instantiations; p.fast_out != NULL: the fast-history ones)
hipError_t launch_temporal_clamp(const ClampP &p, hipStream_t stream);
hipError_t launch_svgf_variance(const SvgfVarP &p, hipStream_t stream);
extern int g_exposure_form; // the shipped form, or fspt_exposure_set_form's (a measurement switch)
// form 0: one LDS atomic per pixel; 1: the first active lane's bin is counted by a ballot (same histogram bit for bit)
hipError_t launch_exposure_histogram(const float4 *src, uint32_t W, uint32_t vw, uint32_t vh, uint32_t *hist, int form, hipStream_t stream);
hipError_t launch_exposure_resolve(uint32_t *hist, ExposureState *state, const ExposureP &p, hipStream_t stream); // (zeroes hist)
extern int g_bloom_form;
extern uint32_t g_bloom_tail_texels;
BloomPlan bloom_plan(uint32_t vw, uint32_t vh, uint32_t levels, int form, uint32_t tail_texels);
hipError_t launch_bloom_chain(const float4 *src, uint32_t pitch, const BloomPlan &q, float scatter, float4 *pyr, hipEvent_t *ev,
                              float4 *down_snapshot, float4 *dbg_up, hipStream_t stream);
hipError_t launch_bloom_mix(const float4 *src, uint32_t W, uint32_t H, const BloomDraw &bl, float4 *bloom_out, float4 *mix_out, hipStream_t stream);

} // namespace fspt
