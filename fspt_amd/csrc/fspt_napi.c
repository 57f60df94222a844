/*
 * fspt_napi.c — thin N-API addon over the libfspt C ABI (include/fspt.h).
 *
 * The reference's host language is JavaScript; this is the binding a
 * maintainer loads from main.js in place of the WebGL2 calls.
 * Every export is a 1:1 wrapper: TypedArrays in, a caller-owned Float32Array
 * out, libfspt error codes become JS Errors carrying fspt_last_error().
 *
 *   sceneCreate({bvh,tri,mat,norm,uv: Float32Array, atlas: Uint8Array, atlasRes,
 *                atlasLayers, env: Uint8Array|null, envW, envH, bins: Uint32Array,
 *                leafSize}, device)                -> scene handle   (initBVH uploads, main.js:408-437)
 *   targetCreate(scene, W, H)                      -> target handle  (initBuffers, main.js:598-617)
 *   camera(target, P[3], I[3], fovScale, lens[2], randBase)          (drawCamera, main.js:741-756)
 *   trace(target, tick, randBase, envTheta, numBounces)              (drawTracer, main.js:758-807)
 *   traceTest(target, tick)                                          (drawTracer with bvh_test.fs, mode=test)
 *   render(target, {P,I,fovScale,lens,envTheta,numBounces}, firstTick, nTicks, seed)
 *   clear(target) / sync(target)                                     (clear, main.js:826-836)
 *   readRadiance(target, Float32Array(W*H*4))                        (what draw.fs:87 reads)
 *   draw(target, exposure, saturation, denoise, maxSigma, Uint8Array(W*H*4))   (drawQuad, main.js:809-824)
 *   setShard(target, shard, nShards, tile) / setPipeline(target, pipeline, batch)
 *   setMemoryLimit(target, bytes) / pathStateBytes(target) -> {bytes, batchTicks} / prepare(target) / setTail(target, round) / setDeferred(target, on)
 *   renderAsync(target, params, firstTick, nTicks, seed) -> Promise   (fspt_render + fspt_sync as napi_async_work)
 *   multiCreate(sceneDesc, [devices], W, H) -> multi handle; multiCamera / multiTrace / multiRender / multiRenderAsync /
 *   multiClear / multiSync / multiReadRadiance / multiDraw / multiTarget(multi, i) / multiDestroy   (fspt_multi_*: one frame
 *   over several GPUs from this one JS thread, tiles gathered onto the first device at read-out)
 *   multiSetExchange / multiGetExchange / multiLastStageMs(multi, nDevices) -> Float32Array(nDevices * 4)
 * Handles are napi externals with finalizers (a dropped tracer frees its device memory when it is collected), and while
 * a renderAsync job runs every other call on its target / multi throws Error('render in flight') - see "handles" below.
 *   enableCounters(target, on) / counters(target) -> object
 *   builderCreate / builderParseObj / builderCommit / builderNormalize / builderBuild / builderBuildGpu / builderAutofocus /
 *   builderDestroy                                                   (native obj_loader.js + bvh.js, 1:1 fspt_builder_*)
 *   envBins(Uint8Array rgbe, w, h) -> Uint32Array                    (native env_sampler.js)
 *   sceneDestroy / targetDestroy / deviceCount / abiVersion / setTextureInterleaveBudget
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

#define NAPI_OK(call)                                                  \
  do {                                                                 \
    if ((call) != napi_ok) {                                           \
      napi_throw_error(env, NULL, "fspt_napi: N-API call failed: " #call); \
      return NULL;                                                     \
    }                                                                  \
  } while (0)

#define FSPT_OK_OR_THROW(call)                                         \
  do {                                                                 \
    int rc_ = (call);                                                  \
    if (rc_ != 0) {                                                    \
      char msg_[640];                                                  \
      snprintf(msg_, sizeof(msg_), "libfspt error %d: %s", rc_, fspt_last_error()); \
      napi_throw_error(env, NULL, msg_);                               \
      return NULL;                                                     \
    }                                                                  \
  } while (0)

static napi_value undefined(napi_env env) { napi_value u; napi_get_undefined(env, &u); return u; }

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
    napi_throw_type_error(env, NULL, "fspt_napi: wrong number of arguments");
    return -1;
  }
  return 0;
}

/* typed array -> pointer + element count; NULL/undefined allowed when optional */
static int typed(napi_env env, napi_value v, napi_typedarray_type want, int optional, void **data, size_t *len) {
  napi_valuetype vt;
  napi_typeof(env, v, &vt);
  if (optional && (vt == napi_undefined || vt == napi_null)) { *data = NULL; *len = 0; return 0; }
  bool is = false;
  napi_is_typedarray(env, v, &is);
  napi_typedarray_type t;
  if (!is || napi_get_typedarray_info(env, v, &t, len, data, NULL, NULL) != napi_ok || t != want) {
    napi_throw_type_error(env, NULL, "fspt_napi: expected a TypedArray of the documented element type");
    return -1;
  }
  return 0;
}

static int prop(napi_env env, napi_value obj, const char *name, napi_value *out) {
  if (napi_get_named_property(env, obj, name, out) != napi_ok) {
    napi_throw_type_error(env, NULL, "fspt_napi: missing property");
    return -1;
  }
  return 0;
}
static int prop_u32(napi_env env, napi_value obj, const char *name, uint32_t *out) {
  napi_value v;
  if (prop(env, obj, name, &v)) return -1;
  if (napi_get_value_uint32(env, v, out) != napi_ok) { napi_throw_type_error(env, NULL, name); return -1; }
  return 0;
}
static int get_f64(napi_env env, napi_value v, double *out) {
  if (napi_get_value_double(env, v, out) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: expected a number"); return -1; }
  return 0;
}
static int prop_f64(napi_env env, napi_value obj, const char *name, double dflt, double *out) {
  napi_value v; napi_valuetype vt;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) { *out = dflt; return 0; }
  napi_typeof(env, v, &vt);
  if (vt == napi_undefined || vt == napi_null) { *out = dflt; return 0; }
  return get_f64(env, v, out);
}
/* NUM_BOUNCES from JS: a finite integer in [0, FSPT_MAX_BOUNCES].  A plain uint32 conversion would turn -1 into
 * 4294967295 and 2.5 into 2 silently; anything outside the range is a caller bug, reported as a RangeError. */
static int get_bounces(napi_env env, napi_value v, uint32_t *out) {
  double d;
  if (get_f64(env, v, &d)) return -1;
  if (!(d >= 0.0 && d <= (double)FSPT_MAX_BOUNCES) || d != (double)(uint32_t)d) {
    napi_throw_range_error(env, NULL, "fspt_napi: numBounces must be an integer in [0, 64]");
    return -1;
  }
  *out = (uint32_t)d;
  return 0;
}
static int float_list(napi_env env, napi_value arr, float *out, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e; double d;
    if (napi_get_element(env, arr, i, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) {
      napi_throw_type_error(env, NULL, "fspt_napi: expected an array of numbers");
      return -1;
    }
    out[i] = (float)d;
  }
  return 0;
}
/* ---------------------------------------------------------------- handles
 * A handle is an napi external around a small box, not the bare library pointer:
 *   - the box knows what it holds, so a scene passed where a target is expected is a TypeError, not a crash;
 *   - `busy` counts the renderAsync jobs in flight on it: while a libuv worker is inside fspt_render, every other addon
 *     call on that target / multi (readRadiance, tick, clear, destroy, ...) throws Error('render in flight') instead
 *     of racing the worker (the library's contract is one thread at a time per target, include/fspt.h; the reference's
 *     tick() is single-threaded, main.js:838-857).  Set and cleared on the JS thread only;
 *   - the external has a finalizer: a tracer that is dropped without close() gives its device memory back when the
 *     JS object is collected (fspt_target_destroy waits for the target's stream first);
 *   - a target keeps its scene alive (a strong reference to the scene's external), a multi's per-device target
 *     (multiTarget) keeps the multi alive and dies with it; sceneDestroy refuses while targets of the scene exist. */
enum { H_SCENE = 1, H_TARGET = 2, H_MULTI = 3, H_BUILDER = 4 };
static const char *const kind_name[] = {"?", "scene", "target", "multi", "builder"};
typedef struct fspt_handle {
  int kind;
  void *ptr;                   /* NULL once destroyed */
  int owned;                   /* 0: a multi's per-device target: owned by the multi */
  int busy;                    /* renderAsync jobs in flight on this handle (a target's job also counts on its scene) */
  int children;                /* scene: live targets made from it */
  struct fspt_handle *parent;  /* target -> scene box; multi's target -> multi box (valid while parent_ref is held) */
  napi_ref parent_ref;
} fspt_handle;

static void handle_release(napi_env env, fspt_handle *b) {
  if (b->ptr && b->owned) {
    switch (b->kind) {
      case H_SCENE: fspt_scene_destroy((fspt_scene *)b->ptr); break;
      case H_TARGET: fspt_target_destroy((fspt_target *)b->ptr); break; /* waits for its stream, drops recorded ticks */
      case H_MULTI: fspt_multi_destroy((fspt_multi *)b->ptr); break;
      case H_BUILDER: fspt_builder_destroy((fspt_builder *)b->ptr); break;
    }
  }
  b->ptr = NULL;
  if (b->parent) {
    if (b->kind == H_TARGET && b->owned && b->parent->children > 0) b->parent->children--;
    b->parent = NULL;
  }
  if (b->parent_ref) { napi_delete_reference(env, b->parent_ref); b->parent_ref = NULL; }
}
static void handle_finalize(napi_env env, void *data, void *hint) {
  (void)hint;
  fspt_handle *b = (fspt_handle *)data;
  handle_release(env, b); /* (never busy here: a job in flight holds a reference to the external) */
  free(b);
}
/* parent_val / parent: the external and box this handle keeps alive (NULL: none) */
static napi_value make_handle(napi_env env, int kind, void *ptr, int owned, napi_value parent_val, fspt_handle *parent) {
  fspt_handle *b = (fspt_handle *)calloc(1, sizeof(fspt_handle));
  napi_value ext;
  if (!b) { napi_throw_error(env, NULL, "fspt_napi: out of memory"); return NULL; }
  b->kind = kind; b->ptr = ptr; b->owned = owned; b->parent = parent;
  if (parent && napi_create_reference(env, parent_val, 1, &b->parent_ref) != napi_ok) b->parent = NULL;
  if (napi_create_external(env, b, handle_finalize, NULL, &ext) != napi_ok) {
    handle_release(env, b); free(b);
    napi_throw_error(env, NULL, "fspt_napi: napi_create_external failed");
    return NULL;
  }
  if (b->parent && kind == H_TARGET && owned) b->parent->children++;
  return ext;
}
static int handle_busy(const fspt_handle *b) { return b->busy || (!b->owned && b->parent && b->parent->busy); }
static int unwrap_box(napi_env env, napi_value v, int kind, fspt_handle **out) {
  void *d = NULL;
  napi_valuetype vt;
  if (napi_typeof(env, v, &vt) != napi_ok || vt != napi_external || napi_get_value_external(env, v, &d) != napi_ok || !d ||
      ((fspt_handle *)d)->kind != kind) {
    char msg[96];
    snprintf(msg, sizeof msg, "fspt_napi: expected a %s handle", kind_name[kind]);
    napi_throw_type_error(env, NULL, msg);
    return -1;
  }
  fspt_handle *b = (fspt_handle *)d;
  if (!b->ptr || (!b->owned && (!b->parent || !b->parent->ptr))) {
    char msg[96];
    snprintf(msg, sizeof msg, "fspt_napi: the %s handle was destroyed", kind_name[kind]);
    napi_throw_error(env, NULL, msg);
    return -1;
  }
  *out = b;
  return 0;
}
/* the library pointer behind a handle; throws (and returns non-zero) on a wrong / destroyed handle and while a
 * renderAsync job is in flight on it */
static int unwrap_k(napi_env env, napi_value v, int kind, void **out) {
  fspt_handle *b;
  if (unwrap_box(env, v, kind, &b)) return -1;
  if (handle_busy(b)) { napi_throw_error(env, NULL, "render in flight"); return -1; }
  *out = b->ptr;
  return 0;
}

/* ------------------------------------------------------------------ scene */
/* {bvh, tri, mat, norm, uv, atlas, atlasRes, atlasLayers, env, envW, envH, bins, leafSize} -> fspt_scene_desc viewing
 * the TypedArrays (valid while the JS object is alive, i.e. for the duration of the call) */
static int parse_scene_desc(napi_env env, napi_value obj, fspt_scene_desc *d) {
  memset(d, 0, sizeof(*d));
  napi_value v; void *p; size_t n;
  if (prop(env, obj, "bvh", &v) || typed(env, v, napi_float32_array, 0, &p, &n)) return -1;
  d->bvh = (const float *)p; d->n_nodes = (uint32_t)(n / 9);
  if (prop(env, obj, "tri", &v) || typed(env, v, napi_float32_array, 0, &p, &n)) return -1;
  d->tri = (const float *)p; d->n_tris = (uint32_t)(n / 9);
  size_t nm, nn, nu;
  if (prop(env, obj, "mat", &v) || typed(env, v, napi_float32_array, 0, &p, &nm)) return -1;
  d->mat = (const float *)p;
  if (prop(env, obj, "norm", &v) || typed(env, v, napi_float32_array, 0, &p, &nn)) return -1;
  d->norm = (const float *)p;
  if (prop(env, obj, "uv", &v) || typed(env, v, napi_float32_array, 0, &p, &nu)) return -1;
  d->uv = (const float *)p;
  if (nm != (size_t)d->n_tris * 12 || nn != (size_t)d->n_tris * 27 || nu != (size_t)d->n_tris * 6) {
    napi_throw_range_error(env, NULL, "fspt_napi: mat/norm/uv lengths do not match tri (12/27/6 floats per triangle)");
    return -1;
  }
  if (prop(env, obj, "atlas", &v) || typed(env, v, napi_uint8_array, 0, &p, &n)) return -1;
  d->atlas = (const uint8_t *)p;
  if (prop_u32(env, obj, "atlasRes", &d->atlas_res) || prop_u32(env, obj, "atlasLayers", &d->atlas_layers)) return -1;
  if (n != (size_t)d->atlas_res * d->atlas_res * d->atlas_layers * 4) {
    napi_throw_range_error(env, NULL, "fspt_napi: atlas length != atlasRes^2 * atlasLayers * 4");
    return -1;
  }
  if (prop(env, obj, "env", &v) || typed(env, v, napi_uint8_array, 1, &p, &n)) return -1;
  d->env = (const uint8_t *)p;
  if (d->env) {
    if (prop_u32(env, obj, "envW", &d->env_w) || prop_u32(env, obj, "envH", &d->env_h)) return -1;
    if (n != (size_t)d->env_w * d->env_h * 4) { napi_throw_range_error(env, NULL, "fspt_napi: env length != envW*envH*4"); return -1; }
  }
  if (prop(env, obj, "bins", &v) || typed(env, v, napi_uint32_array, 0, &p, &n)) return -1;
  d->bins = (const uint32_t *)p; d->n_bins = (uint32_t)(n / 4);
  if (prop_u32(env, obj, "leafSize", &d->leaf_size)) return -1;
  return 0;
}
static napi_value SceneCreate(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (get_args(env, info, 2, a)) return NULL;
  fspt_scene_desc d;
  if (parse_scene_desc(env, a[0], &d)) return NULL;
  int32_t device = 0;
  napi_get_value_int32(env, a[1], &device);
  fspt_scene *s = NULL;
  FSPT_OK_OR_THROW(fspt_scene_create(&d, device, &s));
  napi_value ext = make_handle(env, H_SCENE, s, 1, NULL, NULL);
  if (!ext) fspt_scene_destroy(s);
  return ext;
}
static napi_value SceneDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h; fspt_handle *hb;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_SCENE, &h) || unwrap_box(env, a[0], H_SCENE, &hb)) return NULL;
  if (hb->children > 0) { napi_throw_error(env, NULL, "fspt_napi: the scene still has targets (destroy them first)"); return NULL; }
  handle_release(env, hb);
  return undefined(env);
}

/* sceneUpdateGeometry(scene, nTris, tri Float32Array, norm Float32Array | null): fspt_scene_update_geometry.
 * nTris is the count the scene was created with (the JS host knows it): the arrays must hold 9 / 27 floats per triangle.
 * Guarded like every scene call: a renderAsync job on a target of the scene counts on the scene ('render in flight'). */
static napi_value SceneUpdateGeometry(napi_env env, napi_callback_info info) {
  napi_value a[4]; void *h, *tri = NULL, *norm = NULL; size_t nt = 0, nn = 0; uint32_t n = 0;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_float32_array, 0, &tri, &nt) || typed(env, a[3], napi_float32_array, 1, &norm, &nn)) return NULL;
  if (nt != (size_t)n * 9 || (norm && nn != (size_t)n * 27)) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateGeometry needs 9 floats (tri) and 27 floats (norm) per triangle of the scene");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_scene_update_geometry((fspt_scene *)h, (const float *)tri, (const float *)norm));
  return undefined(env);
}
/* sceneRebuildGeometry(scene, nTris, tri, norm | null) -> Uint32Array order: fspt_scene_rebuild_geometry; the
 * arguments and the guard of sceneUpdateGeometry. */
static napi_value SceneRebuildGeometry(napi_env env, napi_callback_info info) {
  napi_value a[4], ab, ta; void *h, *tri = NULL, *norm = NULL, *order = NULL; size_t nt = 0, nn = 0; uint32_t n = 0;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_float32_array, 0, &tri, &nt) || typed(env, a[3], napi_float32_array, 1, &norm, &nn)) return NULL;
  if (nt != (size_t)n * 9 || (norm && nn != (size_t)n * 27)) {
    napi_throw_range_error(env, NULL, "fspt_napi: rebuildGeometry needs 9 floats (tri) and 27 floats (norm) per triangle of the scene");
    return NULL;
  }
  NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 4, &order, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_uint32_array, (size_t)n, ab, 0, &ta));
  FSPT_OK_OR_THROW(fspt_scene_rebuild_geometry((fspt_scene *)h, (const float *)tri, (const float *)norm, (uint32_t *)order));
  return ta;
}
/* sceneSetPose(scene, nTris, part Uint32Array | null, nParts, tri Float32Array | null, norm Float32Array | null):
 * fspt_scene_set_pose.  part null drops the pose; else one id < nParts per triangle and the rest mesh, 9 / 27
 * floats per triangle.  The guard of sceneUpdateGeometry. */
static napi_value SceneSetPose(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h, *part = NULL, *tri = NULL, *norm = NULL; size_t np = 0, nt = 0, nn = 0; uint32_t n = 0, parts = 0;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_uint32_array, 1, &part, &np)) return NULL;
  if (!part) { FSPT_OK_OR_THROW(fspt_scene_set_pose((fspt_scene *)h, NULL, 0, NULL, NULL)); return undefined(env); }
  NAPI_OK(napi_get_value_uint32(env, a[3], &parts));
  if (typed(env, a[4], napi_float32_array, 0, &tri, &nt) || typed(env, a[5], napi_float32_array, 1, &norm, &nn)) return NULL;
  if (np != (size_t)n || nt != (size_t)n * 9 || (norm && nn != (size_t)n * 27)) {
    napi_throw_range_error(env, NULL, "fspt_napi: setPose needs 1 id (part), 9 floats (tri) and 27 floats (norm) per triangle of the scene");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_scene_set_pose((fspt_scene *)h, (const uint32_t *)part, parts, (const float *)tri, (const float *)norm));
  return undefined(env);
}
/* sceneUpdateTransforms(scene, xf Float32Array): fspt_scene_update_transforms with xf.length / 12 parts. */
static napi_value SceneUpdateTransforms(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h, *xf = NULL; size_t nx = 0;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_float32_array, 0, &xf, &nx)) return NULL;
  if (nx == 0 || nx % 12) { napi_throw_range_error(env, NULL, "fspt_napi: updateTransforms needs 12 floats per part"); return NULL; }
  FSPT_OK_OR_THROW(fspt_scene_update_transforms((fspt_scene *)h, (const float *)xf, (uint32_t)(nx / 12)));
  return undefined(env);
}
/* sceneSetSkin(scene, nTris, joints Uint16Array | null, weights Float32Array, nJoints, tri Float32Array, norm Float32Array | null,
 * morph Float32Array | null, morphNorm Float32Array | null): fspt_scene_set_skin.  joints null drops the skin; else
 * per triangle 12 ids and 12 weights (4 per corner), the rest mesh (9 / 27 floats) and nMorph = morph.length / (nTris * 9)
 * targets of 9 / 27 floats per triangle.  The guard of sceneUpdateGeometry. */
static napi_value SceneSetSkin(napi_env env, napi_callback_info info) {
  napi_value a[9]; void *h, *joints = NULL, *weights = NULL, *tri = NULL, *norm = NULL, *morph = NULL, *mnorm = NULL;
  size_t nj = 0, nw = 0, nt = 0, nn = 0, nm = 0, nmn = 0; uint32_t n = 0, n_joints = 0;
  fspt_skin_desc d;
  if (get_args(env, info, 9, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_uint16_array, 1, &joints, &nj)) return NULL;
  if (!joints) { FSPT_OK_OR_THROW(fspt_scene_set_skin((fspt_scene *)h, NULL)); return undefined(env); }
  if (typed(env, a[3], napi_float32_array, 0, &weights, &nw)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[4], &n_joints));
  if (typed(env, a[5], napi_float32_array, 0, &tri, &nt) || typed(env, a[6], napi_float32_array, 1, &norm, &nn) ||
      typed(env, a[7], napi_float32_array, 1, &morph, &nm) || typed(env, a[8], napi_float32_array, 1, &mnorm, &nmn)) return NULL;
  if (nj != (size_t)n * 12 || nw != (size_t)n * 12 || nt != (size_t)n * 9 || (norm && nn != (size_t)n * 27)) {
    napi_throw_range_error(env, NULL, "fspt_napi: setSkin needs 12 ids (joints), 12 floats (weights), 9 floats (tri) and 27 floats (norm) per triangle of the scene");
    return NULL;
  }
  if ((morph && (n == 0 || nm == 0 || nm % ((size_t)n * 9))) || (mnorm && (!morph || nmn != nm * 3))) {
    napi_throw_range_error(env, NULL, "fspt_napi: setSkin needs 9 floats (morph) and 27 floats (morphNorm) per triangle and morph target");
    return NULL;
  }
  d.joints = (const uint16_t *)joints; d.weights = (const float *)weights; d.n_joints = n_joints;
  d.tri = (const float *)tri; d.norm = (const float *)norm; d.morph = (const float *)morph; d.morph_norm = (const float *)mnorm;
  d.n_morph = morph ? (uint32_t)(nm / ((size_t)n * 9)) : 0;
  FSPT_OK_OR_THROW(fspt_scene_set_skin((fspt_scene *)h, &d));
  return undefined(env);
}
/* sceneUpdateSkin(scene, xf Float32Array, morphWeights Float32Array | null): fspt_scene_update_skin with xf.length / 12 joints
 * and morphWeights.length targets. */
static napi_value SceneUpdateSkin(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h, *xf = NULL, *mw = NULL; size_t nx = 0, nm = 0;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_float32_array, 0, &xf, &nx) || typed(env, a[2], napi_float32_array, 1, &mw, &nm)) return NULL;
  if (nx == 0 || nx % 12) { napi_throw_range_error(env, NULL, "fspt_napi: updateSkin needs 12 floats per joint"); return NULL; }
  FSPT_OK_OR_THROW(fspt_scene_update_skin((fspt_scene *)h, (const float *)xf, (uint32_t)(nx / 12), nm ? (const float *)mw : NULL, (uint32_t)nm));
  return undefined(env);
}
/* sceneSetMesh(scene, nTris, vertex Uint32Array | null, nVertices, uv Float64Array, smooth Uint8Array | null, rank Uint32Array | null,
 * tri Float32Array | null, norm Float32Array | null): fspt_scene_set_mesh.  vertex null drops the mesh; else per
 * triangle 3 indices (0xFFFFFFFF three times: static), 6 raw vt values, a smooth flag, a rank, and the rest 9 / 27 floats the
 * static triangles keep.  The guard of sceneUpdateGeometry. */
static napi_value SceneSetMesh(napi_env env, napi_callback_info info) {
  napi_value a[9]; void *h, *vertex = NULL, *uv = NULL, *smooth = NULL, *rank = NULL, *tri = NULL, *norm = NULL;
  size_t nv = 0, nu = 0, ns = 0, nr = 0, nt = 0, nn = 0; uint32_t n = 0, n_vertices = 0;
  fspt_mesh_desc d;
  if (get_args(env, info, 9, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_uint32_array, 1, &vertex, &nv)) return NULL;
  if (!vertex) { FSPT_OK_OR_THROW(fspt_scene_set_mesh((fspt_scene *)h, NULL)); return undefined(env); }
  NAPI_OK(napi_get_value_uint32(env, a[3], &n_vertices));
  if (typed(env, a[4], napi_float64_array, 0, &uv, &nu) || typed(env, a[5], napi_uint8_array, 1, &smooth, &ns) || typed(env, a[6], napi_uint32_array, 1, &rank, &nr) ||
      typed(env, a[7], napi_float32_array, 1, &tri, &nt) || typed(env, a[8], napi_float32_array, 1, &norm, &nn)) return NULL;
  if (nv != (size_t)n * 3 || nu != (size_t)n * 6 || (smooth && ns != (size_t)n) || (rank && nr != (size_t)n) || (tri && nt != (size_t)n * 9) || (norm && nn != (size_t)n * 27)) {
    napi_throw_range_error(env, NULL, "fspt_napi: setMesh needs 3 indices (vertex), 6 doubles (uv), 1 flag (smooth), 1 rank, 9 floats (tri) and 27 floats (norm) per triangle of the scene");
    return NULL;
  }
  d.vertex = (const uint32_t *)vertex; d.n_vertices = n_vertices; d.uv = (const double *)uv; d.smooth = (const uint8_t *)smooth;
  d.rank = (const uint32_t *)rank; d.tri = (const float *)tri; d.norm = (const float *)norm;
  FSPT_OK_OR_THROW(fspt_scene_set_mesh((fspt_scene *)h, &d));
  return undefined(env);
}
/* sceneUpdateVertices(scene, pos Float32Array): fspt_scene_update_vertices with pos.length / 3 vertices. */
static napi_value SceneUpdateVertices(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h, *pos = NULL; size_t np = 0;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_float32_array, 0, &pos, &np)) return NULL;
  if (np == 0 || np % 3) { napi_throw_range_error(env, NULL, "fspt_napi: updateVertices needs 3 floats per vertex"); return NULL; }
  FSPT_OK_OR_THROW(fspt_scene_update_vertices((fspt_scene *)h, (const float *)pos, (uint32_t)(np / 3)));
  return undefined(env);
}
/* sceneReadMesh(scene, nTris) -> { tri: Float32Array, norm: Float32Array }: fspt_scene_read_mesh. */
static napi_value SceneReadMesh(napi_env env, napi_callback_info info) {
  napi_value a[2], ab, tt, tn, out; void *h, *tri = NULL, *norm = NULL; uint32_t n = 0;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 36, &tri, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_float32_array, (size_t)n * 9, ab, 0, &tt));
  NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 108, &norm, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_float32_array, (size_t)n * 27, ab, 0, &tn));
  FSPT_OK_OR_THROW(fspt_scene_read_mesh((fspt_scene *)h, (float *)tri, (float *)norm));
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "tri", tt));
  NAPI_OK(napi_set_named_property(env, out, "norm", tn));
  return out;
}
/* sceneUpdateMaterials(scene, nTris, mat Float32Array, uv Float32Array | null, atlas Uint8Array | null, atlasRes, atlasLayers):
 * fspt_scene_update_materials.  12 / 6 floats per triangle of the scene; an atlas holds atlasRes^2 * atlasLayers
 * RGBA8 texels (null: the atlas of the scene's last call that carried one).  The guard of sceneUpdateGeometry. */
static napi_value SceneUpdateMaterials(napi_env env, napi_callback_info info) {
  napi_value a[7]; void *h, *mat = NULL, *uv = NULL, *atlas = NULL; size_t nm = 0, nu = 0, na = 0; uint32_t n = 0, res = 0, layers = 0;
  if (get_args(env, info, 7, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_float32_array, 0, &mat, &nm) || typed(env, a[3], napi_float32_array, 1, &uv, &nu) ||
      typed(env, a[4], napi_uint8_array, 1, &atlas, &na)) return NULL;
  if (atlas) { NAPI_OK(napi_get_value_uint32(env, a[5], &res)); NAPI_OK(napi_get_value_uint32(env, a[6], &layers)); }
  if (nm != (size_t)n * 12 || (uv && nu != (size_t)n * 6)) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateMaterials needs 12 floats (mat) and 6 floats (uv) per triangle of the scene");
    return NULL;
  }
  if (atlas && (uint64_t)na != (uint64_t)res * res * layers * 4u) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateMaterials needs atlasRes * atlasRes * atlasLayers RGBA8 texels (atlas)");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_scene_update_materials((fspt_scene *)h, (const float *)mat, (const float *)uv, (const uint8_t *)atlas, res, layers));
  return undefined(env);
}
/* sceneUpdateEnvironment(scene, env Uint8Array | null, envW, envH, bins Uint32Array): fspt_scene_update_environment. */
static napi_value SceneUpdateEnvironment(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h, *map = NULL, *bins = NULL; size_t ne = 0, nb = 0; uint32_t w = 0, hh = 0;
  if (get_args(env, info, 5, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_uint8_array, 1, &map, &ne) || typed(env, a[4], napi_uint32_array, 0, &bins, &nb)) return NULL;
  if (map) { NAPI_OK(napi_get_value_uint32(env, a[2], &w)); NAPI_OK(napi_get_value_uint32(env, a[3], &hh)); }
  if (map && (uint64_t)ne != (uint64_t)w * hh * 4u) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateEnvironment needs envW * envH RGBE texels (env)");
    return NULL;
  }
  if (nb % 4) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateEnvironment needs 4 words per bin (bins)");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_scene_update_environment((fspt_scene *)h, (const uint8_t *)map, w, hh, (const uint32_t *)bins, (uint32_t)(nb / 4)));
  return undefined(env);
}
/* Texture packing on the GPU.  A description crosses as: images - an Array of Uint8Array (RGBA8, row 0 = top) -,
 * dims - a Uint32Array of (w, h) per image -, layers - a Float32Array of 10 per layer: kind, colour.rgb, image, corrected,
 * swizzle x 4 -, and res.  The sizes are checked here (every image holds w * h * 4 bytes); the values are the library's to
 * refuse.  tex_desc_free() after the call, whatever it returned. */
typedef struct { fspt_texture_pack p; fspt_texture_image *images; fspt_texture_layer *layers; } tex_desc;
static void tex_desc_free(tex_desc *d) { free(d->images); free(d->layers); d->images = NULL; d->layers = NULL; }
static int tex_desc_args(napi_env env, napi_value images, napi_value dims, napi_value layers, napi_value res, tex_desc *d) {
  void *dm = NULL, *ly = NULL; size_t nd = 0, nl = 0; uint32_t n_images = 0, r = 0; bool is_array = false;
  memset(d, 0, sizeof *d);
  if (napi_is_array(env, images, &is_array) != napi_ok || !is_array || napi_get_array_length(env, images, &n_images) != napi_ok) {
    napi_throw_type_error(env, NULL, "fspt_napi: a texture description needs an Array of Uint8Array (images)"); return -1;
  }
  if (typed(env, dims, napi_uint32_array, 0, &dm, &nd) || typed(env, layers, napi_float32_array, 0, &ly, &nl)) return -1;
  if (napi_get_value_uint32(env, res, &r) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: a texture description needs res"); return -1; }
  if (nd != (size_t)n_images * 2) { napi_throw_range_error(env, NULL, "fspt_napi: a texture description needs 2 words (w, h) per image (dims)"); return -1; }
  if (nl % 10) { napi_throw_range_error(env, NULL, "fspt_napi: a texture description needs 10 floats per layer (layers)"); return -1; }
  d->images = (fspt_texture_image *)calloc(n_images ? n_images : 1, sizeof *d->images);
  d->layers = (fspt_texture_layer *)calloc(nl / 10 ? nl / 10 : 1, sizeof *d->layers);
  if (!d->images || !d->layers) { tex_desc_free(d); napi_throw_error(env, NULL, "fspt_napi: out of memory"); return -1; }
  for (uint32_t i = 0; i < n_images; ++i) {
    napi_value v; void *px = NULL; size_t np = 0;
    const uint32_t w = ((const uint32_t *)dm)[2 * i], h = ((const uint32_t *)dm)[2 * i + 1];
    if (napi_get_element(env, images, i, &v) != napi_ok || typed(env, v, napi_uint8_array, 0, &px, &np)) { tex_desc_free(d); return -1; }
    if ((uint64_t)np != (uint64_t)w * h * 4u) {
      tex_desc_free(d);
      napi_throw_range_error(env, NULL, "fspt_napi: a texture description needs w * h RGBA8 texels per image (images, dims)"); return -1;
    }
    d->images[i].rgba = (const uint8_t *)px; d->images[i].w = w; d->images[i].h = h;
  }
  for (size_t l = 0; l < nl / 10; ++l) {
    const float *q = (const float *)ly + l * 10;
    fspt_texture_layer *y = &d->layers[l];
    y->kind = (q[0] >= -1.0f && q[0] <= 1024.0f) ? (int32_t)q[0] : -1;        /* (NaN and what no int32 holds: no kind) */
    y->color[0] = q[1]; y->color[1] = q[2]; y->color[2] = q[3];
    y->image = (q[4] >= 0.0f && q[4] < 4294967040.0f) ? (uint32_t)q[4] : 0xFFFFFFFFu;
    y->corrected = q[5] != 0.0f;
    for (int k = 0; k < 4; ++k) y->swizzle[k] = (q[6 + k] >= 0.0f && q[6 + k] <= 255.0f) ? (uint8_t)q[6 + k] : 255;
  }
  d->p.images = d->images; d->p.n_images = n_images; d->p.layers = d->layers; d->p.n_layers = (uint32_t)(nl / 10); d->p.res = r;
  return 0;
}
static napi_value tex_throw(napi_env env, int rc) {
  char msg[640];
  snprintf(msg, sizeof msg, "libfspt error %d: %s", rc, fspt_last_error());
  napi_throw_error(env, NULL, msg);
  return NULL;
}
/* atlasPackGpu(device, images, dims, layers, res) -> Uint8Array of res^2 * nLayers RGBA8 texels: fspt_atlas_pack_gpu. */
static napi_value AtlasPackGpu(napi_env env, napi_callback_info info) {
  napi_value a[5], ab, ta; void *data = NULL; int32_t device = 0; tex_desc d; int rc;
  if (get_args(env, info, 5, a)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[0], &device));
  if (tex_desc_args(env, a[1], a[2], a[3], a[4], &d)) return NULL;
  if ((rc = fspt_texture_pack_check_eval(&d.p, NULL, 0, 0, 0))) { tex_desc_free(&d); return tex_throw(env, rc); } /* (the refusals, before anything is allocated) */
  const size_t bytes = (size_t)d.p.res * d.p.res * d.p.n_layers * 4;
  if (napi_create_arraybuffer(env, bytes, &data, &ab) != napi_ok || napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta) != napi_ok) {
    tex_desc_free(&d); napi_throw_error(env, NULL, "fspt_napi: N-API call failed: the atlas"); return NULL;
  }
  rc = fspt_atlas_pack_gpu(device, &d.p, (uint8_t *)data);
  tex_desc_free(&d);
  return rc ? tex_throw(env, rc) : ta;
}
/* sceneUpdateTextures(scene, nTris, mat Float32Array, uv Float32Array | null, images, dims, layers, res): fspt_scene_update_textures.
 * 12 / 6 floats per triangle of the scene.  The guard of sceneUpdateGeometry. */
static napi_value SceneUpdateTextures(napi_env env, napi_callback_info info) {
  napi_value a[8]; void *h, *mat = NULL, *uv = NULL; size_t nm = 0, nu = 0; uint32_t n = 0; tex_desc d; int rc;
  if (get_args(env, info, 8, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (typed(env, a[2], napi_float32_array, 0, &mat, &nm) || typed(env, a[3], napi_float32_array, 1, &uv, &nu)) return NULL;
  if (nm != (size_t)n * 12 || (uv && nu != (size_t)n * 6)) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateTextures needs 12 floats (mat) and 6 floats (uv) per triangle of the scene");
    return NULL;
  }
  if (tex_desc_args(env, a[4], a[5], a[6], a[7], &d)) return NULL;
  rc = fspt_scene_update_textures((fspt_scene *)h, (const float *)mat, (const float *)uv, &d.p);
  tex_desc_free(&d);
  return rc ? tex_throw(env, rc) : undefined(env);
}
/* scenePatchTextures(scene, layerIds Uint32Array, images, dims, layers, res): fspt_scene_patch_textures - one id per layer of the
 * description.  The guard of sceneUpdateGeometry. */
static napi_value ScenePatchTextures(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h, *ids = NULL; size_t ni = 0; tex_desc d; int rc;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_uint32_array, 0, &ids, &ni)) return NULL;
  if (tex_desc_args(env, a[2], a[3], a[4], a[5], &d)) return NULL;
  if (ni != d.p.n_layers) {
    tex_desc_free(&d);
    napi_throw_range_error(env, NULL, "fspt_napi: patchTextures needs one layer id per layer of the description");
    return NULL;
  }
  rc = fspt_scene_patch_textures((fspt_scene *)h, (const uint32_t *)ids, (uint32_t)ni, &d.p);
  tex_desc_free(&d);
  return rc ? tex_throw(env, rc) : undefined(env);
}
/* GPU sky.  A sky's parameters cross as a Float32Array(10) - sun_dir.xyz, turbidity, sun_intensity, sun_radius, gain,
 * ground_albedo.rgb - and two counts; the library checks the ranges. */
static int sky_params_arg(napi_env env, napi_value f, napi_value vs, napi_value ls, fspt_sky_params *p) {
  void *d = NULL; size_t n = 0; uint32_t v = 0, l = 0;
  if (typed(env, f, napi_float32_array, 0, &d, &n)) return -1;
  if (n != 10) { napi_throw_range_error(env, NULL, "fspt_napi: a sky needs 10 floats (sun_dir, turbidity, sun_intensity, sun_radius, gain, ground_albedo)"); return -1; }
  if (napi_get_value_uint32(env, vs, &v) != napi_ok || napi_get_value_uint32(env, ls, &l) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: a sky needs viewSamples and lightSamples"); return -1; }
  const float *q = (const float *)d;
  p->sun_dir[0] = q[0]; p->sun_dir[1] = q[1]; p->sun_dir[2] = q[2];
  p->turbidity = q[3]; p->sun_intensity = q[4]; p->sun_radius = q[5]; p->gain = q[6];
  p->ground_albedo[0] = q[7]; p->ground_albedo[1] = q[8]; p->ground_albedo[2] = q[9];
  p->view_samples = v; p->light_samples = l;
  return 0;
}
/* sceneUpdateSky(scene, params Float32Array(10), viewSamples, lightSamples, w, h): fspt_scene_update_sky.  The guard of sceneUpdateGeometry. */
static napi_value SceneUpdateSky(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h; uint32_t w = 0, hh = 0; fspt_sky_params p;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_SCENE, &h) || sky_params_arg(env, a[1], a[2], a[3], &p)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[4], &w)); NAPI_OK(napi_get_value_uint32(env, a[5], &hh));
  FSPT_OK_OR_THROW(fspt_scene_update_sky((fspt_scene *)h, &p, w, hh));
  return undefined(env);
}
/* sceneUpdateEnvironmentAuto(scene, env Uint8Array, envW, envH): fspt_scene_update_environment_auto - the bins are built on the GPU. */
static napi_value SceneUpdateEnvironmentAuto(napi_env env, napi_callback_info info) {
  napi_value a[4]; void *h, *map = NULL; size_t ne = 0; uint32_t w = 0, hh = 0;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  if (typed(env, a[1], napi_uint8_array, 0, &map, &ne)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &w)); NAPI_OK(napi_get_value_uint32(env, a[3], &hh));
  if ((uint64_t)ne != (uint64_t)w * hh * 4u) {
    napi_throw_range_error(env, NULL, "fspt_napi: updateEnvironmentAuto needs envW * envH RGBE texels (env)");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_scene_update_environment_auto((fspt_scene *)h, (const uint8_t *)map, w, hh));
  return undefined(env);
}
/* skyGenerate(device, params Float32Array(10), viewSamples, lightSamples, w, h) -> Uint8Array RGBE: fspt_sky_generate. */
static napi_value SkyGenerate(napi_env env, napi_callback_info info) {
  napi_value a[6], ab, ta; void *data; int32_t device = 0; uint32_t w = 0, hh = 0; fspt_sky_params p;
  if (get_args(env, info, 6, a) || sky_params_arg(env, a[1], a[2], a[3], &p)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[0], &device));
  NAPI_OK(napi_get_value_uint32(env, a[4], &w)); NAPI_OK(napi_get_value_uint32(env, a[5], &hh));
  FSPT_OK_OR_THROW(fspt_sky_generate(device, &p, w, hh, NULL, NULL)); /* (the refusals, before anything is allocated) */
  NAPI_OK(napi_create_arraybuffer(env, (size_t)w * hh * 4, &data, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_uint8_array, (size_t)w * hh * 4, ab, 0, &ta));
  FSPT_OK_OR_THROW(fspt_sky_generate(device, &p, w, hh, (uint8_t *)data, NULL));
  return ta;
}
/* envBinsGpu(rgbe Uint8Array, w, h, device) -> Uint32Array: fspt_env_bins_gpu. */
static napi_value EnvBinsGpu(napi_env env, napi_callback_info info) {
  napi_value a[4], ab, ta; void *p, *data; size_t n; uint32_t w, h, nb = 0; int32_t device = 0;
  if (get_args(env, info, 4, a) || typed(env, a[0], napi_uint8_array, 0, &p, &n)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &w)); NAPI_OK(napi_get_value_uint32(env, a[2], &h)); NAPI_OK(napi_get_value_int32(env, a[3], &device));
  if (n != (size_t)w * h * 4) { napi_throw_range_error(env, NULL, "fspt_napi: rgbe length != w*h*4"); return NULL; }
  FSPT_OK_OR_THROW(fspt_env_bins_gpu((const uint8_t *)p, w, h, device, NULL, 0, &nb));
  NAPI_OK(napi_create_arraybuffer(env, (size_t)nb * 16, &data, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_uint32_array, (size_t)nb * 4, ab, 0, &ta));
  FSPT_OK_OR_THROW(fspt_env_bins_gpu((const uint8_t *)p, w, h, device, (uint32_t *)data, nb, &nb));
  return ta;
}
static napi_value SceneSahCost(napi_env env, napi_callback_info info) {
  napi_value a[1], v; void *h; double cost = 0.0;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_scene_sah_cost((fspt_scene *)h, &cost));
  NAPI_OK(napi_create_double(env, cost, &v));
  return v;
}

/* ----------------------------------------------------------------- target */
static napi_value TargetCreate(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; uint32_t W, H;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &W));
  NAPI_OK(napi_get_value_uint32(env, a[2], &H));
  fspt_target *t = NULL;
  fspt_handle *sb;
  if (unwrap_box(env, a[0], H_SCENE, &sb)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_create((fspt_scene *)h, W, H, &t));
  napi_value ext = make_handle(env, H_TARGET, t, 1, a[0], sb);
  if (!ext) fspt_target_destroy(t);
  return ext;
}
static napi_value TargetDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h; fspt_handle *hb;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h) || unwrap_box(env, a[0], H_TARGET, &hb)) return NULL;
  if (!hb->owned) { napi_throw_error(env, NULL, "fspt_napi: a multi's per-device target is destroyed with the multi"); return NULL; }
  handle_release(env, hb);
  return undefined(env);
}
static napi_value Camera(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h; float P[3], I[3], lens[2]; double fov, rb;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (float_list(env, a[1], P, 3) || float_list(env, a[2], I, 3) || get_f64(env, a[3], &fov) || float_list(env, a[4], lens, 2) ||
      get_f64(env, a[5], &rb)) return NULL;
  FSPT_OK_OR_THROW(fspt_camera((fspt_target *)h, P, I, (float)fov, lens, (float)rb));
  return undefined(env);
}
static napi_value TraceTest(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; uint32_t tick;
  if (get_args(env, info, 2, a)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &tick));
  FSPT_OK_OR_THROW(fspt_trace_test((fspt_target *)h, tick));
  return undefined(env);
}
static napi_value Trace(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h; uint32_t tick, nb; double rb, theta;
  if (get_args(env, info, 5, a)) return NULL;
  /* scalars first: a bad numBounces is reported as such even when the handle is bad too */
  if (get_f64(env, a[2], &rb) || get_f64(env, a[3], &theta) || get_bounces(env, a[4], &nb)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &tick));
  FSPT_OK_OR_THROW(fspt_trace((fspt_target *)h, tick, (float)rb, (float)theta, nb));
  return undefined(env);
}
static int parse_camera_params(napi_env env, napi_value obj, fspt_camera_params *cp) {
  napi_value v; double d;
  memset(cp, 0, sizeof(*cp));
  if (prop(env, obj, "P", &v) || float_list(env, v, cp->P, 3)) return -1;
  if (prop(env, obj, "I", &v) || float_list(env, v, cp->I, 3)) return -1;
  if (prop(env, obj, "lens", &v) || float_list(env, v, cp->lens, 2)) return -1;
  if (prop_f64(env, obj, "fovScale", 0.5, &d)) return -1;
  cp->fov_scale = (float)d;
  if (prop_f64(env, obj, "envTheta", 0.0, &d)) return -1;
  cp->env_theta = (float)d;
  napi_value nbv; napi_valuetype nbt = napi_undefined;
  cp->num_bounces = 4; /* tracer.fs:9 */
  if (napi_get_named_property(env, obj, "numBounces", &nbv) == napi_ok) napi_typeof(env, nbv, &nbt);
  if (nbt != napi_undefined && nbt != napi_null && get_bounces(env, nbv, &cp->num_bounces)) return -1;
  return 0;
}
/* seed: BigInt (full 64-bit xorshift state) or a number < 2^53 */
static int parse_seed(napi_env env, napi_value v, uint64_t *seed64) {
  napi_valuetype st;
  napi_typeof(env, v, &st);
  if (st == napi_bigint) {
    bool lossless = true;
    if (napi_get_value_bigint_uint64(env, v, seed64, &lossless) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: bad seed"); return -1; }
    return 0;
  }
  double seed;
  if (get_f64(env, v, &seed)) return -1;
  *seed64 = (uint64_t)seed;
  return 0;
}
static napi_value Render(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h; uint32_t first, n; uint64_t seed64 = 0;
  if (get_args(env, info, 5, a)) return NULL;
  fspt_camera_params cp;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &first));
  NAPI_OK(napi_get_value_uint32(env, a[3], &n));
  if (parse_seed(env, a[4], &seed64)) return NULL;
  FSPT_OK_OR_THROW(fspt_render((fspt_target *)h, &cp, first, n, seed64));
  return undefined(env);
}

/* renderAsync(target, params, firstTick, nTicks, seed) -> Promise<undefined>
 * fspt_render + fspt_sync on a libuv worker thread (napi_async_work), so an interactive host keeps its event loop
 * while a long batch runs.  The caller must not touch the target until the promise settles: all calls for
 * one target still come from one thread AT A TIME (include/fspt.h). */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  fspt_handle *box;      /* the handle the job runs on: busy until render_complete */
  napi_ref box_ref;      /* keeps its external (and so the box and the target) alive while the worker runs */
  fspt_target *target;
  fspt_multi *multi;
  fspt_camera_params cp;
  uint32_t first, n;
  uint64_t seed;
  int rc;
  char err[600];
} render_job;
static void render_execute(napi_env env, void *data) {
  (void)env;
  render_job *j = (render_job *)data;
  if (j->multi) {
    j->rc = fspt_multi_render(j->multi, &j->cp, j->first, j->n, j->seed);
    if (j->rc == 0) j->rc = fspt_multi_sync(j->multi);
  } else {
    j->rc = fspt_render(j->target, &j->cp, j->first, j->n, j->seed);
    if (j->rc == 0) j->rc = fspt_sync(j->target);
  }
  /* fspt_last_error() is thread-local: fetch it on the thread that made the call */
  if (j->rc != 0) snprintf(j->err, sizeof(j->err), "libfspt error %d: %s", j->rc, fspt_last_error());
}
static void render_complete(napi_env env, napi_status status, void *data) {
  render_job *j = (render_job *)data;
  napi_value v;
  /* the target is the JS thread's again BEFORE the promise settles (its reactions may call readRadiance at once) */
  if (j->box) { j->box->busy--; if (j->box->kind == H_TARGET && j->box->owned && j->box->parent) j->box->parent->busy--; }
  if (status == napi_ok && j->rc == 0) {
    napi_get_undefined(env, &v);
    napi_resolve_deferred(env, j->deferred, v);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "fspt_napi: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    napi_reject_deferred(env, j->deferred, v);
  }
  if (j->box_ref) napi_delete_reference(env, j->box_ref);
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value render_async(napi_env env, napi_callback_info info, int multi) {
  napi_value a[5], promise, name; fspt_handle *hb = NULL; uint64_t seed64 = 0;
  if (get_args(env, info, 5, a)) return NULL;
  render_job *j = (render_job *)calloc(1, sizeof(render_job));
  if (!j) { napi_throw_error(env, NULL, "fspt_napi: out of memory"); return NULL; }
  if (parse_camera_params(env, a[1], &j->cp) || unwrap_box(env, a[0], multi ? H_MULTI : H_TARGET, &hb) || parse_seed(env, a[4], &seed64) ||
      napi_get_value_uint32(env, a[2], &j->first) != napi_ok || napi_get_value_uint32(env, a[3], &j->n) != napi_ok) {
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    if (!pending) napi_throw_type_error(env, NULL, "fspt_napi: renderAsync(target, params, firstTick, nTicks, seed)");
    free(j);
    return NULL;
  }
  if (handle_busy(hb)) { free(j); napi_throw_error(env, NULL, "render in flight"); return NULL; } /* one job at a time per target */
  if (multi) j->multi = (fspt_multi *)hb->ptr; else j->target = (fspt_target *)hb->ptr;
  j->seed = seed64;
  if (napi_create_reference(env, a[0], 1, &j->box_ref) != napi_ok) { free(j); napi_throw_error(env, NULL, "fspt_napi: napi_create_reference failed"); return NULL; }
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "fspt_render", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, render_execute, render_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    if (j->work) napi_delete_async_work(env, j->work); /* created but not queued */
    napi_delete_reference(env, j->box_ref);
    free(j);
    napi_throw_error(env, NULL, "fspt_napi: could not queue the async work");
    return NULL;
  }
  /* from here until render_complete every other call on this handle throws 'render in flight' (unwrap_k) */
  j->box = hb;
  hb->busy++;
  if (hb->kind == H_TARGET && hb->owned && hb->parent) hb->parent->busy++;
  return promise;
}
static napi_value RenderAsync(napi_env env, napi_callback_info info) { return render_async(env, info, 0); }
static napi_value MultiRenderAsync(napi_env env, napi_callback_info info) { return render_async(env, info, 1); }

/* ------------------------------------------------------- several devices (fspt_multi_*) */
static napi_value MultiCreate(napi_env env, napi_callback_info info) {
  /* multiCreate(sceneDesc, [device, ...], W, H) */
  napi_value a[4]; uint32_t n = 0, W, H; int devices[64];
  if (get_args(env, info, 4, a)) return NULL;
  fspt_scene_desc d;
  if (parse_scene_desc(env, a[0], &d)) return NULL;
  if (napi_get_array_length(env, a[1], &n) != napi_ok || n == 0 || n > 64) { napi_throw_range_error(env, NULL, "fspt_napi: devices must be an array of 1..64 ordinals"); return NULL; }
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e; int32_t v;
    if (napi_get_element(env, a[1], i, &e) != napi_ok || napi_get_value_int32(env, e, &v) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: device ordinals must be numbers"); return NULL; }
    devices[i] = v;
  }
  NAPI_OK(napi_get_value_uint32(env, a[2], &W));
  NAPI_OK(napi_get_value_uint32(env, a[3], &H));
  fspt_multi *m = NULL;
  FSPT_OK_OR_THROW(fspt_multi_create(&d, devices, n, W, H, &m));
  napi_value ext = make_handle(env, H_MULTI, m, 1, NULL, NULL);
  if (!ext) fspt_multi_destroy(m);
  return ext;
}
static napi_value MultiDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h; fspt_handle *hb;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_MULTI, &h) || unwrap_box(env, a[0], H_MULTI, &hb)) return NULL;
  handle_release(env, hb); /* its per-device target handles (multiTarget) are dead from here on */
  return undefined(env);
}
static napi_value MultiTarget(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; uint32_t i; fspt_target *t = NULL; fspt_handle *mb;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_MULTI, &h) || unwrap_box(env, a[0], H_MULTI, &mb)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &i));
  FSPT_OK_OR_THROW(fspt_multi_target((fspt_multi *)h, i, &t));
  return make_handle(env, H_TARGET, t, 0, a[0], mb); /* borrowed: lives and dies with the multi */
}
static napi_value MultiCamera(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h; float P[3], I[3], lens[2]; double fov, rb;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  if (float_list(env, a[1], P, 3) || float_list(env, a[2], I, 3) || get_f64(env, a[3], &fov) || float_list(env, a[4], lens, 2) ||
      get_f64(env, a[5], &rb)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_camera((fspt_multi *)h, P, I, (float)fov, lens, (float)rb));
  return undefined(env);
}
static napi_value MultiTrace(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h; uint32_t tick, nb; double rb, theta;
  if (get_args(env, info, 5, a)) return NULL;
  if (get_f64(env, a[2], &rb) || get_f64(env, a[3], &theta) || get_bounces(env, a[4], &nb)) return NULL;
  if (unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &tick));
  FSPT_OK_OR_THROW(fspt_multi_trace((fspt_multi *)h, tick, (float)rb, (float)theta, nb));
  return undefined(env);
}
static napi_value MultiRender(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h; uint32_t first, n; uint64_t seed64 = 0;
  if (get_args(env, info, 5, a)) return NULL;
  fspt_camera_params cp;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  if (unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &first));
  NAPI_OK(napi_get_value_uint32(env, a[3], &n));
  if (parse_seed(env, a[4], &seed64)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_render((fspt_multi *)h, &cp, first, n, seed64));
  return undefined(env);
}
static napi_value MultiClear(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_clear((fspt_multi *)h));
  return undefined(env);
}
/* multiSetExchange(multi, mode): 0 peer copies, 1 RCCL send / recv of the packed tiles, 2 RCCL sum-reduce (fspt_multi.h) */
static napi_value MultiSetExchange(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; int32_t mode;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &mode));
  FSPT_OK_OR_THROW(fspt_multi_set_exchange((fspt_multi *)h, mode));
  return undefined(env);
}
/* multiGetExchange(multi) -> {mode, rcclVersion} */
static napi_value MultiGetExchange(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; void *h; int mode = 0, ver = 0;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_get_exchange((fspt_multi *)h, &mode, &ver));
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_int32(env, mode, &v));
  NAPI_OK(napi_set_named_property(env, o, "mode", v));
  NAPI_OK(napi_create_int32(env, ver, &v));
  NAPI_OK(napi_set_named_property(env, o, "rcclVersion", v));
  return o;
}
/* multiLastStageMs(multi, nDevices) -> Float32Array(nDevices * 4): per device render / pack / transfer / scatter ms of the
 * most recent render + read-out (fspt_multi_last_stage_ms, include/fspt_multi.h; -1 = the stage did not run) */
static napi_value MultiLastStageMs(napi_env env, napi_callback_info info) {
  napi_value a[2], ab, ta; void *h, *data; uint32_t n;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (n == 0 || n > 64) { napi_throw_range_error(env, NULL, "fspt_napi: nDevices must be 1..64"); return NULL; }
  NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 16, &data, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_float32_array, (size_t)n * 4, ab, 0, &ta));
  FSPT_OK_OR_THROW(fspt_multi_last_stage_ms((fspt_multi *)h, (float *)data, n));
  return ta;
}
static napi_value MultiSync(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_sync((fspt_multi *)h));
  return undefined(env);
}
/* The library writes W*H*4 elements into the caller's TypedArray: a shorter one is a heap overflow. */
static int check_frame_len(napi_env env, size_t n, uint32_t W, uint32_t H) {
  if (n == (size_t)W * H * 4u) return 0;
  char msg[160];
  snprintf(msg, sizeof msg, "fspt_napi: array of %zu elements, the %ux%u frame needs %zu", n, W, H, (size_t)W * H * 4u);
  napi_throw_range_error(env, NULL, msg);
  return 1;
}
static int check_target_len(napi_env env, void *h, size_t n) {
  uint32_t W = 0, H = 0;
  if (fspt_target_size((fspt_target *)h, &W, &H) != FSPT_OK) { napi_throw_error(env, NULL, fspt_last_error()); return 1; }
  return check_frame_len(env, n, W, H);
}
static int check_multi_len(napi_env env, void *h, size_t n) {
  uint32_t W = 0, H = 0;
  if (fspt_multi_size((fspt_multi *)h, &W, &H) != FSPT_OK) { napi_throw_error(env, NULL, fspt_last_error()); return 1; }
  return check_frame_len(env, n, W, H);
}
static napi_value MultiReadRadiance(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h, *p; size_t n;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_MULTI, &h) || typed(env, a[1], napi_float32_array, 0, &p, &n)) return NULL;
  if (check_multi_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_read_radiance((fspt_multi *)h, (float *)p));
  return a[1];
}
static napi_value MultiDraw(napi_env env, napi_callback_info info) {
  napi_value a[6]; void *h, *p; size_t n; double ex, sat, sig; bool den;
  if (get_args(env, info, 6, a) || unwrap_k(env, a[0], H_MULTI, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[3], &den));
  if (get_f64(env, a[4], &sig) || typed(env, a[5], napi_uint8_array, 0, &p, &n)) return NULL;
  if (check_multi_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_multi_draw((fspt_multi *)h, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (uint8_t *)p));
  return a[5];
}
static napi_value SetDeferred(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; bool on;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  FSPT_OK_OR_THROW(fspt_target_set_deferred((fspt_target *)h, on ? 1 : 0));
  return undefined(env);
}
static napi_value SetTail(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; int32_t r;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &r));
  FSPT_OK_OR_THROW(fspt_target_set_tail((fspt_target *)h, r));
  return undefined(env);
}
/* setStageTiming(target, on): the per-launch HIP event pairs behind fspt_last_stage_ms (fspt_tuning.h) */
static napi_value SetStageTiming(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; bool on;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  FSPT_OK_OR_THROW(fspt_target_set_stage_timing((fspt_target *)h, on ? 1 : 0));
  return undefined(env);
}
static napi_value Clear(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_clear((fspt_target *)h));
  return undefined(env);
}
static napi_value Sync(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_sync((fspt_target *)h));
  return undefined(env);
}
static napi_value ReadRadiance(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h, *p; size_t n;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h) || typed(env, a[1], napi_float32_array, 0, &p, &n)) return NULL;
  if (check_target_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_read_radiance((fspt_target *)h, (float *)p));
  return a[1];
}
static napi_value Draw(napi_env env, napi_callback_info info) {
  /* draw(target, exposure, saturation, denoise, maxSigma, Uint8Array(W*H*4)[, scale]) : drawQuad (main.js:809-824) */
  napi_value a[7]; void *h, *p; size_t n, argc = 7; double ex, sat, sig, scale = 1.0; bool den;
  if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 6) {
    napi_throw_type_error(env, NULL, "fspt_napi: wrong number of arguments");
    return NULL;
  }
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[3], &den));
  if (get_f64(env, a[4], &sig) || typed(env, a[5], napi_uint8_array, 0, &p, &n)) return NULL;
  if (argc > 6) { napi_valuetype vt; napi_typeof(env, a[6], &vt); if (vt == napi_number && get_f64(env, a[6], &scale)) return NULL; }
  if (check_target_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_draw_scaled((fspt_target *)h, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (float)scale, (uint8_t *)p));
  return a[5];
}
static napi_value Present(napi_env env, napi_callback_info info) {
  /* present(target, exposure, saturation, denoise, maxSigma, Uint8Array(W*H*4), scale) -> ticks: fspt_present (drawQuad
   * inside tick(), one frame of latency; 0 = nothing presented, the array untouched) */
  napi_value a[7], r; void *h, *p; size_t n; double ex, sat, sig, scale; bool den; uint32_t ticks = 0;
  if (get_args(env, info, 7, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[3], &den));
  if (get_f64(env, a[4], &sig) || typed(env, a[5], napi_uint8_array, 0, &p, &n) || get_f64(env, a[6], &scale)) return NULL;
  if (check_target_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_present((fspt_target *)h, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (float)scale, (uint8_t *)p, &ticks));
  NAPI_OK(napi_create_uint32(env, ticks, &r));
  return r;
}
/* JPEG output (include/fspt.h fspt_jpeg_* / fspt_draw_jpeg / fspt_present_jpeg).  The file is written into a
 * Uint8Array the JS host keeps; a call answers the bytes written, or -(bytes needed) when the array is too small (the
 * library's FSPT_E_INVALID with *bytes_out above cap: nothing was written; a present frame refused so is dropped). */
static int jpeg_args(napi_env env, const napi_value *a, fspt_jpeg_params *p) { /* quality, subsampling, restartMcus */
  double q, s, r;
  if (get_f64(env, a[0], &q) || get_f64(env, a[1], &s) || get_f64(env, a[2], &r)) return -1;
  if (!(q >= 0.0 && q <= 4294967295.0 && s >= 0.0 && s <= 4294967295.0 && r >= 0.0 && r <= 4294967295.0)) {
    napi_throw_range_error(env, NULL, "fspt_napi: JPEG parameters must be non-negative integers");
    return -1;
  }
  p->quality = (uint32_t)q; p->subsampling = (uint32_t)s; p->restart_mcus = (uint32_t)r;
  return 0;
}
static napi_value jpeg_answer(napi_env env, int rc, size_t cap, size_t bytes) {
  napi_value r;
  if (rc == FSPT_E_INVALID && bytes > cap) { NAPI_OK(napi_create_double(env, -(double)bytes, &r)); return r; }
  FSPT_OK_OR_THROW(rc);
  NAPI_OK(napi_create_double(env, (double)bytes, &r));
  return r;
}
static napi_value JpegBound(napi_env env, napi_callback_info info) {
  /* jpegBound(width, height, quality, subsampling, restartMcus) -> bytes no file exceeds */
  napi_value a[5], r; double w, h; fspt_jpeg_params p; size_t n = 0;
  if (get_args(env, info, 5, a) || get_f64(env, a[0], &w) || get_f64(env, a[1], &h) || jpeg_args(env, a + 2, &p)) return NULL;
  FSPT_OK_OR_THROW(fspt_jpeg_bound(w >= 0.0 && w <= 4294967295.0 ? (uint32_t)w : 0u, h >= 0.0 && h <= 4294967295.0 ? (uint32_t)h : 0u, &p, &n));
  NAPI_OK(napi_create_double(env, (double)n, &r));
  return r;
}
static napi_value JpegEncode(napi_env env, napi_callback_info info) {
  /* jpegEncode(device, Uint8Array(w*h*4), width, height, bottomUp, quality, subsampling, restartMcus, Uint8Array out) */
  napi_value a[9]; void *src, *dst; size_t ns, nd, bytes = 0; double dev, w, h; bool up; fspt_jpeg_params p;
  if (get_args(env, info, 9, a) || get_f64(env, a[0], &dev) || typed(env, a[1], napi_uint8_array, 0, &src, &ns) || get_f64(env, a[2], &w) || get_f64(env, a[3], &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[4], &up));
  if (jpeg_args(env, a + 5, &p) || typed(env, a[8], napi_uint8_array, 0, &dst, &nd)) return NULL;
  if (!(w >= 1.0 && w <= 65535.0 && h >= 1.0 && h <= 65535.0) || (double)ns != w * h * 4.0) {
    napi_throw_range_error(env, NULL, "jpegEncode: need width*height*4 bytes, width and height in 1..65535");
    return NULL;
  }
  const int rc = fspt_jpeg_encode((int)dev, (const uint8_t *)src, (uint32_t)w, (uint32_t)h, up ? 1 : 0, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
static napi_value DrawJpeg(napi_env env, napi_callback_info info) {
  /* drawJpeg(target, source, exposure, saturation, denoise, maxSigma, scale, quality, subsampling, restartMcus, Uint8Array out) */
  napi_value a[11]; void *h, *dst; size_t nd, bytes = 0; double src, ex, sat, sig, scale; bool den; fspt_jpeg_params p;
  if (get_args(env, info, 11, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &src) || get_f64(env, a[2], &ex) || get_f64(env, a[3], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[4], &den));
  if (get_f64(env, a[5], &sig) || get_f64(env, a[6], &scale) || jpeg_args(env, a + 7, &p) || typed(env, a[10], napi_uint8_array, 0, &dst, &nd)) return NULL;
  const int rc = fspt_draw_jpeg((fspt_target *)h, (int)src, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (float)scale, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
static napi_value PresentJpeg(napi_env env, napi_callback_info info) {
  /* presentJpeg(target, exposure, saturation, denoise, maxSigma, scale, quality, subsampling, restartMcus, Uint8Array out)
   * -> [bytes (or -needed), ticks]: fspt_present_jpeg; ticks 0 = nothing presented */
  napi_value a[10], r, v; void *h, *dst; size_t nd, bytes = 0; double ex, sat, sig, scale; bool den; fspt_jpeg_params p; uint32_t ticks = 0;
  if (get_args(env, info, 10, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[3], &den));
  if (get_f64(env, a[4], &sig) || get_f64(env, a[5], &scale) || jpeg_args(env, a + 6, &p) || typed(env, a[9], napi_uint8_array, 0, &dst, &nd)) return NULL;
  const int rc = fspt_present_jpeg((fspt_target *)h, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (float)scale, &p, (uint8_t *)dst, nd, &bytes, &ticks);
  if (!(v = jpeg_answer(env, rc, nd, bytes))) return NULL;
  NAPI_OK(napi_create_array_with_length(env, 2, &r));
  NAPI_OK(napi_set_element(env, r, 0, v));
  NAPI_OK(napi_create_uint32(env, ticks, &v));
  NAPI_OK(napi_set_element(env, r, 1, v));
  return r;
}
/* PNG output (include/fspt.h fspt_png_* / fspt_draw_png): as the JPEG entries above - the file goes into a
 * Uint8Array the JS host keeps, the answer is the bytes written or -(bytes needed). */
static int png_args(napi_env env, const napi_value *a, fspt_png_params *p) { /* channels, filter, chunkBytes */
  double c, f, b;
  if (get_f64(env, a[0], &c) || get_f64(env, a[1], &f) || get_f64(env, a[2], &b)) return -1;
  if (!(c >= 0.0 && c <= 4294967295.0 && f >= 0.0 && f <= 4294967295.0 && b >= 0.0 && b <= 4294967295.0)) {
    napi_throw_range_error(env, NULL, "fspt_napi: PNG parameters must be non-negative integers");
    return -1;
  }
  p->channels = (uint32_t)c; p->filter = (uint32_t)f; p->chunk_bytes = (uint32_t)b;
  return 0;
}
static napi_value PngBound(napi_env env, napi_callback_info info) {
  /* pngBound(width, height, channels, filter, chunkBytes) -> bytes no file exceeds */
  napi_value a[5], r; double w, h; fspt_png_params p; size_t n = 0;
  if (get_args(env, info, 5, a) || get_f64(env, a[0], &w) || get_f64(env, a[1], &h) || png_args(env, a + 2, &p)) return NULL;
  FSPT_OK_OR_THROW(fspt_png_bound(w >= 0.0 && w <= 4294967295.0 ? (uint32_t)w : 0u, h >= 0.0 && h <= 4294967295.0 ? (uint32_t)h : 0u, &p, &n));
  NAPI_OK(napi_create_double(env, (double)n, &r));
  return r;
}
static int png_image_args(napi_env env, const napi_value *a, const char *fn, double *dev, void **src, uint32_t *w, uint32_t *h, bool *up, fspt_png_params *p) {
  /* device, Uint8Array(w*h*4), width, height, bottomUp, channels, filter, chunkBytes */
  size_t ns; double dw, dh; char msg[96];
  if (get_f64(env, a[0], dev) || typed(env, a[1], napi_uint8_array, 0, src, &ns) || get_f64(env, a[2], &dw) || get_f64(env, a[3], &dh)) return -1;
  if (napi_get_value_bool(env, a[4], up) != napi_ok || png_args(env, a + 5, p)) return -1;
  if (!(dw >= 1.0 && dw <= 65535.0 && dh >= 1.0 && dh <= 65535.0) || (double)ns != dw * dh * 4.0) {
    snprintf(msg, sizeof msg, "%s: need width*height*4 bytes, width and height in 1..65535", fn);
    napi_throw_range_error(env, NULL, msg);
    return -1;
  }
  *w = (uint32_t)dw; *h = (uint32_t)dh;
  return 0;
}
static napi_value PngEncode(napi_env env, napi_callback_info info) {
  /* pngEncode(device, Uint8Array(w*h*4), width, height, bottomUp, channels, filter, chunkBytes, Uint8Array out) */
  napi_value a[9]; void *src, *dst; size_t nd, bytes = 0; double dev; uint32_t w, h; bool up; fspt_png_params p;
  if (get_args(env, info, 9, a) || png_image_args(env, a, "pngEncode", &dev, &src, &w, &h, &up, &p) || typed(env, a[8], napi_uint8_array, 0, &dst, &nd)) return NULL;
  const int rc = fspt_png_encode((int)dev, (const uint8_t *)src, w, h, up ? 1 : 0, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
static napi_value PngFilteredEval(napi_env env, napi_callback_info info) {
  /* pngFilteredEval(device, Uint8Array(w*h*4), width, height, bottomUp, channels, filter, chunkBytes, Uint8Array(h * (1 + w * channels)) out) */
  napi_value a[9]; void *src, *dst; size_t nd; double dev; uint32_t w, h; bool up; fspt_png_params p;
  if (get_args(env, info, 9, a) || png_image_args(env, a, "pngFilteredEval", &dev, &src, &w, &h, &up, &p) || typed(env, a[8], napi_uint8_array, 0, &dst, &nd)) return NULL;
  if ((p.channels != 3u && p.channels != 4u) || nd != (size_t)h * (1u + (size_t)w * p.channels)) {
    napi_throw_range_error(env, NULL, "pngFilteredEval: need channels 3 or 4 and an output of height * (1 + width * channels) bytes");
    return NULL;
  }
  FSPT_OK_OR_THROW(fspt_png_filtered_eval((int)dev, (const uint8_t *)src, w, h, up ? 1 : 0, &p, (uint8_t *)dst));
  return NULL;
}
static napi_value DrawPng(napi_env env, napi_callback_info info) {
  /* drawPng(target, source, exposure, saturation, denoise, maxSigma, scale, channels, filter, chunkBytes, Uint8Array out) */
  napi_value a[11]; void *h, *dst; size_t nd, bytes = 0; double src, ex, sat, sig, scale; bool den; fspt_png_params p;
  if (get_args(env, info, 11, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &src) || get_f64(env, a[2], &ex) || get_f64(env, a[3], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[4], &den));
  if (get_f64(env, a[5], &sig) || get_f64(env, a[6], &scale) || png_args(env, a + 7, &p) || typed(env, a[10], napi_uint8_array, 0, &dst, &nd)) return NULL;
  const int rc = fspt_draw_png((fspt_target *)h, (int)src, (float)ex, (float)sat, den ? 1 : 0, (float)sig, (float)scale, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
/* OpenEXR output (include/fspt.h fspt_exr_* / fspt_draw_exr): as the PNG entries above */
static int exr_args(napi_env env, const napi_value *a, fspt_exr_params *p) { /* compression, pixelType, layers, chunkBytes */
  double v[4];
  for (int i = 0; i < 4; ++i) {
    if (get_f64(env, a[i], &v[i])) return -1;
    if (!(v[i] >= 0.0 && v[i] <= 4294967295.0)) { napi_throw_range_error(env, NULL, "fspt_napi: EXR parameters must be non-negative integers"); return -1; }
  }
  p->compression = (uint32_t)v[0]; p->pixel_type = (uint32_t)v[1]; p->layers = (uint32_t)v[2]; p->chunk_bytes = (uint32_t)v[3];
  return 0;
}
static napi_value ExrBound(napi_env env, napi_callback_info info) {
  /* exrBound(width, height, compression, pixelType, layers, chunkBytes) -> bytes no file exceeds */
  napi_value a[6], r; double w, h; fspt_exr_params p; size_t n = 0;
  if (get_args(env, info, 6, a) || get_f64(env, a[0], &w) || get_f64(env, a[1], &h) || exr_args(env, a + 2, &p)) return NULL;
  FSPT_OK_OR_THROW(fspt_exr_bound(w >= 0.0 && w <= 4294967295.0 ? (uint32_t)w : 0u, h >= 0.0 && h <= 4294967295.0 ? (uint32_t)h : 0u, &p, &n));
  NAPI_OK(napi_create_double(env, (double)n, &r));
  return r;
}
static napi_value ExrEncode(napi_env env, napi_callback_info info) {
  /* exrEncode(device, Float32Array(w*h*4), Float32Array(w*h*8) | null, width, height, bottomUp, compression, pixelType, layers, chunkBytes, Uint8Array out) */
  napi_value a[11]; void *src, *feat, *dst; size_t ns, nf, nd, bytes = 0; double dev, w, h; bool up; fspt_exr_params p;
  if (get_args(env, info, 11, a) || get_f64(env, a[0], &dev) || typed(env, a[1], napi_float32_array, 0, &src, &ns) || typed(env, a[2], napi_float32_array, 1, &feat, &nf)) return NULL;
  if (get_f64(env, a[3], &w) || get_f64(env, a[4], &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[5], &up));
  if (exr_args(env, a + 6, &p) || typed(env, a[10], napi_uint8_array, 0, &dst, &nd)) return NULL;
  if (!(w >= 1.0 && w <= 65535.0 && h >= 1.0 && h <= 65535.0) || (double)ns != w * h * 4.0 || (feat && (double)nf != w * h * 8.0)) {
    napi_throw_range_error(env, NULL, "exrEncode: need width*height*4 floats, features of width*height*8 floats or null, width and height in 1..65535");
    return NULL;
  }
  const int rc = fspt_exr_encode((int)dev, (const float *)src, (const float *)feat, (uint32_t)w, (uint32_t)h, up ? 1 : 0, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
static napi_value DrawExr(napi_env env, napi_callback_info info) {
  /* drawExr(target, source, compression, pixelType, layers, chunkBytes, Uint8Array out) */
  napi_value a[7]; void *h, *dst; size_t nd, bytes = 0; double src; fspt_exr_params p;
  if (get_args(env, info, 7, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &src) || exr_args(env, a + 2, &p) || typed(env, a[6], napi_uint8_array, 0, &dst, &nd)) return NULL;
  const int rc = fspt_draw_exr((fspt_target *)h, (int)src, &p, (uint8_t *)dst, nd, &bytes);
  return jpeg_answer(env, rc, nd, bytes);
}
/* ID mattes (include/fspt.h fspt_matte_hash .. fspt_exr_encode_mattes).  A manifest is a JS string or null; the
 * copies made here are freed before the call returns (the library keeps its own). */
static int matte_text(napi_env env, napi_value v, char **text, size_t *len) { /* string | null | undefined -> malloc'd UTF-8 or NULL */
  napi_valuetype vt;
  *text = NULL; *len = 0;
  if (napi_typeof(env, v, &vt) != napi_ok) return -1;
  if (vt == napi_null || vt == napi_undefined) return 0;
  if (napi_get_value_string_utf8(env, v, NULL, 0, len) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: expected a string or null"); return -1; }
  *text = (char *)malloc(*len + 1);
  if (!*text) { napi_throw_error(env, NULL, "fspt_napi: out of memory"); return -1; }
  napi_get_value_string_utf8(env, v, *text, *len + 1, len);
  return 0;
}
static int matte_kind(napi_env env, napi_value v, int *kind) {
  double k;
  if (get_f64(env, v, &k)) return -1;
  if (k != 0.0 && k != 1.0) { napi_throw_range_error(env, NULL, "fspt_napi: kind must be 0 (object) or 1 (material)"); return -1; }
  *kind = (int)k;
  return 0;
}
static napi_value MatteHash(napi_env env, napi_callback_info info) {
  /* matteHash(name) -> the 32-bit id */
  napi_value a[1], r; char *text; size_t len;
  if (get_args(env, info, 1, a) || matte_text(env, a[0], &text, &len)) return NULL;
  const uint32_t h = fspt_matte_hash(text, len);
  free(text);
  NAPI_OK(napi_create_uint32(env, h, &r));
  return r;
}
static napi_value SceneSetMatte(napi_env env, napi_callback_info info) {
  /* sceneSetMatte(scene, nTris, kind, ids Uint32Array | null (drops the kind), manifest string | null): both setters; the guard of sceneUpdateGeometry */
  napi_value a[5]; void *h, *ids = NULL; size_t ni = 0, len = 0; uint32_t n = 0; int kind = 0; char *text = NULL;
  if (get_args(env, info, 5, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &n));
  if (matte_kind(env, a[2], &kind) || typed(env, a[3], napi_uint32_array, 1, &ids, &ni)) return NULL;
  if (ids && ni != (size_t)n) { napi_throw_range_error(env, NULL, "fspt_napi: setMatte needs 1 id per triangle of the scene"); return NULL; }
  if (matte_text(env, a[4], &text, &len)) return NULL;
  int rc = fspt_scene_set_matte_ids((fspt_scene *)h, kind, (const uint32_t *)ids);
  if (rc == FSPT_OK) rc = fspt_scene_set_matte_manifest((fspt_scene *)h, kind, ids ? text : NULL, ids ? len : 0);
  free(text);
  FSPT_OK_OR_THROW(rc);
  return undefined(env);
}
static napi_value Mattes(napi_env env, napi_callback_info info) {
  /* mattes(target, params (as render), samples, seed) */
  napi_value a[4]; void *h; uint32_t n; uint64_t seed64 = 0;
  if (get_args(env, info, 4, a)) return NULL;
  fspt_camera_params cp;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &n));
  if (parse_seed(env, a[3], &seed64)) return NULL;
  FSPT_OK_OR_THROW(fspt_mattes((fspt_target *)h, &cp, n, seed64));
  return undefined(env);
}
static napi_value ReadMattes(napi_env env, napi_callback_info info) {
  /* readMattes(target, kind, Float32Array(W*H*12)) -> the array */
  napi_value a[3]; void *h, *p; size_t n; int kind; uint32_t W = 0, H = 0;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h) || matte_kind(env, a[1], &kind) || typed(env, a[2], napi_float32_array, 0, &p, &n)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_size((fspt_target *)h, &W, &H));
  if (n != (size_t)W * H * 12) { napi_throw_range_error(env, NULL, "fspt_napi: readMattes needs W*H*12 floats"); return NULL; }
  FSPT_OK_OR_THROW(fspt_read_mattes((fspt_target *)h, kind, (float *)p));
  return a[2];
}
static napi_value MattesLost(napi_env env, napi_callback_info info) {
  /* mattesLost(target, kind) -> samples the last pass dropped */
  napi_value a[2], r; void *h; int kind; uint64_t lost = 0;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h) || matte_kind(env, a[1], &kind)) return NULL;
  FSPT_OK_OR_THROW(fspt_mattes_lost((fspt_target *)h, kind, &lost));
  NAPI_OK(napi_create_double(env, (double)lost, &r));
  return r;
}
static napi_value ExrBoundMattes(napi_env env, napi_callback_info info) {
  /* exrBoundMattes(width, height, compression, pixelType, layers, chunkBytes, objectManifest string | null, materialManifest string | null) */
  napi_value a[8], r; double w, h; fspt_exr_params p; size_t n = 0; fspt_exr_mattes m; char *t0 = NULL, *t1 = NULL;
  memset(&m, 0, sizeof m);
  if (get_args(env, info, 8, a) || get_f64(env, a[0], &w) || get_f64(env, a[1], &h) || exr_args(env, a + 2, &p)) return NULL;
  if (matte_text(env, a[6], &t0, &m.manifest_len[0])) return NULL;
  if (matte_text(env, a[7], &t1, &m.manifest_len[1])) { free(t0); return NULL; }
  m.manifest[0] = t0; m.manifest[1] = t1;
  const int rc = fspt_exr_bound_mattes(w >= 0.0 && w <= 4294967295.0 ? (uint32_t)w : 0u, h >= 0.0 && h <= 4294967295.0 ? (uint32_t)h : 0u, &p, &m, &n);
  free(t0); free(t1);
  FSPT_OK_OR_THROW(rc);
  NAPI_OK(napi_create_double(env, (double)n, &r));
  return r;
}
static napi_value ExrEncodeMattes(napi_env env, napi_callback_info info) {
  /* exrEncodeMattes(device, Float32Array(w*h*4), Float32Array(w*h*8) | null, object ranks Float32Array(w*h*12) | null, material ranks | null,
   *                 objectManifest string | null, materialManifest string | null, width, height, bottomUp, compression, pixelType, layers, chunkBytes, Uint8Array out) */
  napi_value a[15]; void *src, *feat, *r0, *r1, *dst; size_t ns, nf, n0, n1, nd, bytes = 0; double dev, w, h; bool up; fspt_exr_params p; fspt_exr_mattes m; char *t0 = NULL, *t1 = NULL;
  memset(&m, 0, sizeof m);
  if (get_args(env, info, 15, a) || get_f64(env, a[0], &dev) || typed(env, a[1], napi_float32_array, 0, &src, &ns) || typed(env, a[2], napi_float32_array, 1, &feat, &nf)) return NULL;
  if (typed(env, a[3], napi_float32_array, 1, &r0, &n0) || typed(env, a[4], napi_float32_array, 1, &r1, &n1)) return NULL;
  if (get_f64(env, a[7], &w) || get_f64(env, a[8], &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[9], &up));
  if (exr_args(env, a + 10, &p) || typed(env, a[14], napi_uint8_array, 0, &dst, &nd)) return NULL;
  if (!(w >= 1.0 && w <= 65535.0 && h >= 1.0 && h <= 65535.0) || (double)ns != w * h * 4.0 || (feat && (double)nf != w * h * 8.0) || (r0 && (double)n0 != w * h * 12.0) || (r1 && (double)n1 != w * h * 12.0)) {
    napi_throw_range_error(env, NULL, "exrEncode: need width*height*4 floats, features of width*height*8 floats or null, ranks of width*height*12 floats or null, width and height in 1..65535");
    return NULL;
  }
  if (matte_text(env, a[5], &t0, &m.manifest_len[0])) return NULL;
  if (matte_text(env, a[6], &t1, &m.manifest_len[1])) { free(t0); return NULL; }
  m.ranks[0] = (const float *)r0; m.ranks[1] = (const float *)r1; m.manifest[0] = t0; m.manifest[1] = t1;
  const int rc = fspt_exr_encode_mattes((int)dev, (const float *)src, (const float *)feat, &m, (uint32_t)w, (uint32_t)h, up ? 1 : 0, &p, (uint8_t *)dst, nd, &bytes);
  free(t0); free(t1);
  return jpeg_answer(env, rc, nd, bytes);
}
/* guided denoiser (include/fspt.h fspt_features / fspt_denoise / fspt_draw_denoised) */
static napi_value Features(napi_env env, napi_callback_info info) {
  /* features(target, params (as render), samples, seed) */
  napi_value a[4]; void *h; uint32_t n; uint64_t seed64 = 0;
  if (get_args(env, info, 4, a)) return NULL;
  fspt_camera_params cp;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &n));
  if (parse_seed(env, a[3], &seed64)) return NULL;
  FSPT_OK_OR_THROW(fspt_features((fspt_target *)h, &cp, n, seed64));
  return undefined(env);
}
static napi_value Denoise(napi_env env, napi_callback_info info) {
  /* denoise(target, {iterations, sigmaColor, sigmaNormal, sigmaDepth} | null = defaults, Float32Array(W*H*4) | null) */
  napi_value a[3]; void *h, *p = NULL; size_t n = 0; napi_valuetype vt;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  fspt_denoise_params dp = {FSPT_DENOISE_ITERATIONS, FSPT_DENOISE_SIGMA_COLOR, FSPT_DENOISE_SIGMA_NORMAL, FSPT_DENOISE_SIGMA_DEPTH};
  NAPI_OK(napi_typeof(env, a[1], &vt));
  const int given = vt == napi_object;
  if (given) {
    double k, c, nn, z;
    if (prop_f64(env, a[1], "iterations", dp.iterations, &k) || prop_f64(env, a[1], "sigmaColor", dp.sigma_color, &c) ||
        prop_f64(env, a[1], "sigmaNormal", dp.sigma_normal, &nn) || prop_f64(env, a[1], "sigmaDepth", dp.sigma_depth, &z)) return NULL;
    if (!(k >= 0.0 && k <= 16.0 && k == (double)(uint32_t)k)) { napi_throw_range_error(env, NULL, "fspt_napi: iterations must be an integer in [0, 16]"); return NULL; }
    dp.iterations = (uint32_t)k; dp.sigma_color = (float)c; dp.sigma_normal = (float)nn; dp.sigma_depth = (float)z;
  }
  NAPI_OK(napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[2], napi_float32_array, 0, &p, &n) || check_target_len(env, h, n)) return NULL;
  }
  FSPT_OK_OR_THROW(fspt_denoise((fspt_target *)h, given ? &dp : NULL, (float *)p));
  return p ? a[2] : undefined(env);
}
static napi_value DrawDenoised(napi_env env, napi_callback_info info) {
  /* drawDenoised(target, exposure, saturation, Uint8Array(W*H*4)) */
  napi_value a[4]; void *h, *p; size_t n; double ex, sat;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat) || typed(env, a[3], napi_uint8_array, 0, &p, &n)) return NULL;
  if (check_target_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_draw_denoised((fspt_target *)h, (float)ex, (float)sat, (uint8_t *)p));
  return a[3];
}
/* temporal accumulation (include/fspt.h fspt_temporal_*, fspt_scene_motion_*) */
static napi_value TemporalAccumulate(napi_env env, napi_callback_info info) {
  /* temporalAccumulate(target, params (as render), {alpha, maxHistory, depthTol, normalCos} | null = defaults, Float32Array(W*H*4) | null) */
  napi_value a[4]; void *h, *p = NULL; size_t n = 0; napi_valuetype vt;
  if (get_args(env, info, 4, a)) return NULL;
  fspt_camera_params cp;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  if (unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  fspt_temporal_params tp = {FSPT_TEMPORAL_ALPHA, FSPT_TEMPORAL_MAX_HISTORY, FSPT_TEMPORAL_DEPTH_TOL, FSPT_TEMPORAL_NORMAL_COS};
  NAPI_OK(napi_typeof(env, a[2], &vt));
  const int given = vt == napi_object;
  if (given) {
    double al, mh, dt, nc;
    if (prop_f64(env, a[2], "alpha", tp.alpha, &al) || prop_f64(env, a[2], "maxHistory", tp.max_history, &mh) ||
        prop_f64(env, a[2], "depthTol", tp.depth_tol, &dt) || prop_f64(env, a[2], "normalCos", tp.normal_cos, &nc)) return NULL;
    if (!(al >= 0.0 && al <= 1.0 && mh >= 1.0 && dt >= 0.0 && nc >= -1.0 && nc <= 1.0)) {
      napi_throw_range_error(env, NULL, "fspt_napi: temporalAccumulate needs alpha in [0, 1], maxHistory >= 1, depthTol >= 0, normalCos in [-1, 1]");
      return NULL;
    }
    tp.alpha = (float)al; tp.max_history = (float)mh; tp.depth_tol = (float)dt; tp.normal_cos = (float)nc;
  }
  NAPI_OK(napi_typeof(env, a[3], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[3], napi_float32_array, 0, &p, &n) || check_target_len(env, h, n)) return NULL;
  }
  FSPT_OK_OR_THROW(fspt_temporal_accumulate((fspt_target *)h, &cp, given ? &tp : NULL, (float *)p));
  return p ? a[3] : undefined(env);
}
static napi_value TemporalReset(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_temporal_reset((fspt_target *)h));
  return undefined(env);
}
static napi_value TemporalDenoise(napi_env env, napi_callback_info info) {
  /* temporalDenoise(target, opts | null, Float32Array(W*H*4) | null): denoise's arguments, fspt_temporal_denoise */
  napi_value a[3]; void *h, *p = NULL; size_t n = 0; napi_valuetype vt;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  fspt_denoise_params dp = {FSPT_DENOISE_ITERATIONS, FSPT_DENOISE_SIGMA_COLOR, FSPT_DENOISE_SIGMA_NORMAL, FSPT_DENOISE_SIGMA_DEPTH};
  NAPI_OK(napi_typeof(env, a[1], &vt));
  const int given = vt == napi_object;
  if (given) {
    double k, c, nn, z;
    if (prop_f64(env, a[1], "iterations", dp.iterations, &k) || prop_f64(env, a[1], "sigmaColor", dp.sigma_color, &c) ||
        prop_f64(env, a[1], "sigmaNormal", dp.sigma_normal, &nn) || prop_f64(env, a[1], "sigmaDepth", dp.sigma_depth, &z)) return NULL;
    if (!(k >= 0.0 && k <= 16.0 && k == (double)(uint32_t)k)) { napi_throw_range_error(env, NULL, "fspt_napi: iterations must be an integer in [0, 16]"); return NULL; }
    dp.iterations = (uint32_t)k; dp.sigma_color = (float)c; dp.sigma_normal = (float)nn; dp.sigma_depth = (float)z;
  }
  NAPI_OK(napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[2], napi_float32_array, 0, &p, &n) || check_target_len(env, h, n)) return NULL;
  }
  FSPT_OK_OR_THROW(fspt_temporal_denoise((fspt_target *)h, given ? &dp : NULL, (float *)p));
  return p ? a[2] : undefined(env);
}
/* temporalSetMoments(target, on) / temporalDenoiseVariance(target, opts | null, Float32Array(W*H*4) | null): SVGF variance guidance */
static napi_value TemporalSetMoments(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; bool on;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  FSPT_OK_OR_THROW(fspt_temporal_set_moments((fspt_target *)h, on ? 1 : 0));
  return undefined(env);
}
/* temporalSetClamp(target, on, fastHistory, sigmaScale): the history clamp; the numbers are the library's to refuse */
static napi_value TemporalSetClamp(napi_env env, napi_callback_info info) {
  napi_value a[4]; void *h; bool on; double fh, ss;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  NAPI_OK(napi_get_value_double(env, a[2], &fh));
  NAPI_OK(napi_get_value_double(env, a[3], &ss));
  FSPT_OK_OR_THROW(fspt_temporal_set_clamp((fspt_target *)h, on ? 1 : 0, (float)fh, (float)ss));
  return undefined(env);
}
/* setAutoExposure(target, on, key, low, high, adaptUp, adaptDown, minLog2, maxLog2) / exposure(target) -> {exposure, log2Mean, metered} /
 * exposureReset(target): auto-exposure; the numbers are the library's to refuse */
static napi_value SetAutoExposure(napi_env env, napi_callback_info info) {
  napi_value a[9]; void *h; bool on; double v[7];
  if (get_args(env, info, 9, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  for (int k = 0; k < 7; ++k) NAPI_OK(napi_get_value_double(env, a[2 + k], &v[k]));
  fspt_exposure_params p = {(float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5], (float)v[6]};
  FSPT_OK_OR_THROW(fspt_target_set_auto_exposure((fspt_target *)h, on ? 1 : 0, &p));
  return undefined(env);
}
static napi_value Exposure(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; void *h; float e = 0.0f, m = 0.0f; uint32_t n = 0;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_exposure_get((fspt_target *)h, &e, &m, &n));
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_double(env, (double)e, &v));
  NAPI_OK(napi_set_named_property(env, o, "exposure", v));
  NAPI_OK(napi_create_double(env, (double)m, &v));
  NAPI_OK(napi_set_named_property(env, o, "log2Mean", v));
  NAPI_OK(napi_create_uint32(env, n, &v));
  NAPI_OK(napi_set_named_property(env, o, "metered", v));
  return o;
}
static napi_value ExposureReset(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_exposure_reset((fspt_target *)h));
  return undefined(env);
}
/* setBloom(target, on, intensity, scatter, levels) / bloom(target) -> {intensity, scatter, levels} or null (off): bloom; the numbers
 * are the library's to refuse */
static napi_value SetBloom(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h; bool on; double v[3];
  if (get_args(env, info, 5, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  for (int k = 0; k < 3; ++k) NAPI_OK(napi_get_value_double(env, a[2 + k], &v[k]));
  if (!(v[2] >= 0.0 && v[2] <= 4294967295.0) || v[2] != (double)(uint32_t)v[2]) { napi_throw_range_error(env, NULL, "setBloom: levels must be a whole number"); return NULL; }
  fspt_bloom_params p = {(float)v[0], (float)v[1], (uint32_t)v[2]};
  FSPT_OK_OR_THROW(fspt_target_set_bloom((fspt_target *)h, on ? 1 : 0, &p));
  return undefined(env);
}
static napi_value Bloom(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; void *h; int on = 0; fspt_bloom_params p;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_get_bloom((fspt_target *)h, &on, &p));
  if (!on) { NAPI_OK(napi_get_null(env, &o)); return o; }
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_double(env, (double)p.intensity, &v));
  NAPI_OK(napi_set_named_property(env, o, "intensity", v));
  NAPI_OK(napi_create_double(env, (double)p.scatter, &v));
  NAPI_OK(napi_set_named_property(env, o, "scatter", v));
  NAPI_OK(napi_create_uint32(env, p.levels, &v));
  NAPI_OK(napi_set_named_property(env, o, "levels", v));
  return o;
}
static napi_value TemporalDenoiseVariance(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h, *p = NULL; size_t n = 0; napi_valuetype vt;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  fspt_denoise_params dp = {FSPT_SVGF_ITERATIONS, FSPT_SVGF_SIGMA_L, FSPT_SVGF_SIGMA_NORMAL, FSPT_SVGF_SIGMA_DEPTH};
  NAPI_OK(napi_typeof(env, a[1], &vt));
  const int given = vt == napi_object;
  if (given) {
    double k, c, nn, z;
    if (prop_f64(env, a[1], "iterations", dp.iterations, &k) || prop_f64(env, a[1], "sigmaColor", dp.sigma_color, &c) ||
        prop_f64(env, a[1], "sigmaNormal", dp.sigma_normal, &nn) || prop_f64(env, a[1], "sigmaDepth", dp.sigma_depth, &z)) return NULL;
    if (!(k >= 0.0 && k <= 16.0 && k == (double)(uint32_t)k)) { napi_throw_range_error(env, NULL, "fspt_napi: iterations must be an integer in [0, 16]"); return NULL; }
    dp.iterations = (uint32_t)k; dp.sigma_color = (float)c; dp.sigma_normal = (float)nn; dp.sigma_depth = (float)z;
  }
  NAPI_OK(napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    if (typed(env, a[2], napi_float32_array, 0, &p, &n) || check_target_len(env, h, n)) return NULL;
  }
  FSPT_OK_OR_THROW(fspt_temporal_denoise_variance((fspt_target *)h, given ? &dp : NULL, (float *)p));
  return p ? a[2] : undefined(env);
}
static napi_value TemporalDraw(napi_env env, napi_callback_info info) {
  /* temporalDraw(target, exposure, saturation, denoised, Uint8Array(W*H*4)) */
  napi_value a[5]; void *h, *p; size_t n; double ex, sat; bool den;
  if (get_args(env, info, 5, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (get_f64(env, a[1], &ex) || get_f64(env, a[2], &sat)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[3], &den));
  if (typed(env, a[4], napi_uint8_array, 0, &p, &n) || check_target_len(env, h, n)) return NULL;
  FSPT_OK_OR_THROW(fspt_temporal_draw((fspt_target *)h, (float)ex, (float)sat, den ? 1 : 0, (uint8_t *)p));
  return a[4];
}
/* sceneMotionBegin(scene) / sceneMotionEnd(scene): guarded like every scene call */
static napi_value SceneMotionBegin(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_scene_motion_begin((fspt_scene *)h));
  return undefined(env);
}
static napi_value SceneMotionEnd(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_scene_motion_end((fspt_scene *)h));
  return undefined(env);
}
static napi_value SetViewport(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; uint32_t w, hh;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &w));
  NAPI_OK(napi_get_value_uint32(env, a[2], &hh));
  FSPT_OK_OR_THROW(fspt_target_set_viewport((fspt_target *)h, w, hh));
  return undefined(env);
}
/* setSampler(target, kind, seed): fspt_target_set_sampler (kind: FSPT_SAMPLER_REFERENCE / FSPT_SAMPLER_SOBOL) */
static napi_value SetSampler(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; int32_t kind; uint32_t seed;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &kind));
  NAPI_OK(napi_get_value_uint32(env, a[2], &seed));
  FSPT_OK_OR_THROW(fspt_target_set_sampler((fspt_target *)h, kind, seed));
  return undefined(env);
}
/* setLights(target, mode, emitterFraction): fspt_target_set_lights (mode: FSPT_LIGHTS_OFF / FSPT_LIGHTS_EMITTERS) */
static napi_value SetLights(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; int32_t mode; double f;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &mode));
  NAPI_OK(napi_get_value_double(env, a[2], &f));
  FSPT_OK_OR_THROW(fspt_target_set_lights((fspt_target *)h, mode, (float)f));
  return undefined(env);
}
/* sceneSetLightBuilder(scene, builder) / sceneGetLightBuilder(scene) -> builder: fspt_scene_set_light_builder / _get_ (DESIGN
 * 8.23; builder: FSPT_LIGHT_BUILDER_HOST / FSPT_LIGHT_BUILDER_GPU).  The guard of sceneUpdateGeometry. */
static napi_value SceneSetLightBuilder(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; int32_t builder;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &builder));
  FSPT_OK_OR_THROW(fspt_scene_set_light_builder((fspt_scene *)h, builder));
  return undefined(env);
}
static napi_value SceneGetLightBuilder(napi_env env, napi_callback_info info) {
  napi_value a[1], r; void *h; int builder = 0;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_SCENE, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_scene_get_light_builder((fspt_scene *)h, &builder));
  NAPI_OK(napi_create_int32(env, builder, &r));
  return r;
}
/* setCameraModel(target, model, angle, ipd): fspt_target_set_camera_model (model: FSPT_CAMERA_*).  fspt.js has
 * checked the arguments; they are checked again here (the target's height for STEREO: by the library). */
static napi_value SetCameraModel(napi_env env, napi_callback_info info) {
  napi_value a[4]; void *h; int32_t model; double angle, ipd; fspt_camera_model_params p;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &model));
  NAPI_OK(napi_get_value_double(env, a[2], &angle));
  NAPI_OK(napi_get_value_double(env, a[3], &ipd));
  if (model < FSPT_CAMERA_PINHOLE || model > FSPT_CAMERA_STEREO) {
    napi_throw_range_error(env, NULL, "fspt_napi: setCameraModel: unknown model");
    return NULL;
  }
  if (model == FSPT_CAMERA_FISHEYE && !((float)angle > 0.0f && (float)angle <= 6.2831855f)) {
    napi_throw_range_error(env, NULL, "fspt_napi: setCameraModel: angle must lie in (0, 2 pi]");
    return NULL;
  }
  if (model == FSPT_CAMERA_STEREO && !((float)ipd >= 0.0f && (float)ipd <= 3.0e38f)) {
    napi_throw_range_error(env, NULL, "fspt_napi: setCameraModel: ipd must be finite and >= 0");
    return NULL;
  }
  p.model = model; p.angle = (float)angle; p.ipd = (float)ipd;
  FSPT_OK_OR_THROW(fspt_target_set_camera_model((fspt_target *)h, &p));
  return undefined(env);
}
/* cameraModel(target) -> { model, angle, ipd }: fspt_target_get_camera_model */
static napi_value CameraModel(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; void *h; fspt_camera_model_params p;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_get_camera_model((fspt_target *)h, &p));
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_int32(env, p.model, &v));
  NAPI_OK(napi_set_named_property(env, o, "model", v));
  NAPI_OK(napi_create_double(env, (double)p.angle, &v));
  NAPI_OK(napi_set_named_property(env, o, "angle", v));
  NAPI_OK(napi_create_double(env, (double)p.ipd, &v));
  NAPI_OK(napi_set_named_property(env, o, "ipd", v));
  return o;
}
/* renderAdaptive(target, params, targetRelMse, maxTicks, minTicks, roundTicks, seed) -> the largest count run:
 * fspt_render_adaptive (include/fspt.h) */
static napi_value RenderAdaptive(napi_env env, napi_callback_info info) {
  napi_value a[7], r; void *h; fspt_camera_params cp; fspt_adaptive_params q; uint64_t seed64 = 0; uint32_t rounds = 0;
  if (get_args(env, info, 7, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (parse_camera_params(env, a[1], &cp)) return NULL;
  NAPI_OK(napi_get_value_double(env, a[2], &q.target_rel_mse));
  NAPI_OK(napi_get_value_uint32(env, a[3], &q.max_ticks));
  NAPI_OK(napi_get_value_uint32(env, a[4], &q.min_ticks));
  NAPI_OK(napi_get_value_uint32(env, a[5], &q.round_ticks));
  if (parse_seed(env, a[6], &seed64)) return NULL;
  FSPT_OK_OR_THROW(fspt_render_adaptive((fspt_target *)h, &cp, &q, seed64));
  FSPT_OK_OR_THROW(fspt_adaptive_last_stats((fspt_target *)h, &rounds, NULL, NULL, NULL, 0));
  NAPI_OK(napi_create_uint32(env, rounds * q.round_ticks, &r));
  return r;
}
/* readSampleCounts(target, Uint32Array(W*H)): fspt_read_sample_counts */
static napi_value ReadSampleCounts(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h, *p; size_t n; uint32_t W, H;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  if (typed(env, a[1], napi_uint32_array, 0, &p, &n)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_size((fspt_target *)h, &W, &H));
  if (n != (size_t)W * H) { napi_throw_range_error(env, NULL, "readSampleCounts: the array must hold W*H counts"); return NULL; }
  FSPT_OK_OR_THROW(fspt_read_sample_counts((fspt_target *)h, (uint32_t *)p));
  return a[1];
}
static napi_value SetShard(napi_env env, napi_callback_info info) {
  napi_value a[4]; void *h; uint32_t s, n, tile;
  if (get_args(env, info, 4, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &s));
  NAPI_OK(napi_get_value_uint32(env, a[2], &n));
  NAPI_OK(napi_get_value_uint32(env, a[3], &tile));
  FSPT_OK_OR_THROW(fspt_target_set_shard((fspt_target *)h, s, n, tile));
  return undefined(env);
}
static napi_value SetPipeline(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; int32_t p; uint32_t b;
  if (get_args(env, info, 3, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[1], &p));
  NAPI_OK(napi_get_value_uint32(env, a[2], &b));
  FSPT_OK_OR_THROW(fspt_target_set_pipeline((fspt_target *)h, p, b));
  return undefined(env);
}
static napi_value SetPool(napi_env env, napi_callback_info info) {
  /* setPool(target, paths, drainIterations, maxIterations, overlap): fspt_target_set_pool (stream scheduler) */
  napi_value a[5]; void *h; uint32_t paths, cap; int32_t drain, overlap;
  if (get_args(env, info, 5, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &paths));
  NAPI_OK(napi_get_value_int32(env, a[2], &drain));
  NAPI_OK(napi_get_value_uint32(env, a[3], &cap));
  NAPI_OK(napi_get_value_int32(env, a[4], &overlap));
  FSPT_OK_OR_THROW(fspt_target_set_pool((fspt_target *)h, paths, drain, cap, overlap));
  return undefined(env);
}
static napi_value SetTraceBudget(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; uint32_t steps;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &steps));
  FSPT_OK_OR_THROW(fspt_target_set_trace_budget((fspt_target *)h, steps));
  return undefined(env);
}
static napi_value SetMemoryLimit(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; double bytes;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h) || get_f64(env, a[1], &bytes)) return NULL;
  if (!(bytes >= 0.0 && bytes < 1.8e19)) { napi_throw_range_error(env, NULL, "fspt_napi: memory limit must be >= 0 bytes"); return NULL; }
  FSPT_OK_OR_THROW(fspt_target_set_memory_limit((fspt_target *)h, (uint64_t)bytes));
  return undefined(env);
}
static napi_value SetTextureInterleaveBudget(napi_env env, napi_callback_info info) {
  napi_value a[1]; double bytes;
  if (get_args(env, info, 1, a) || get_f64(env, a[0], &bytes)) return NULL;
  if (!(bytes >= 0.0 && bytes < 1.8e19)) { napi_throw_range_error(env, NULL, "fspt_napi: budget must be >= 0 bytes"); return NULL; }
  FSPT_OK_OR_THROW(fspt_set_texture_interleave_budget((uint64_t)bytes));
  return undefined(env);
}
static napi_value PathStateBytes(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; void *h; uint64_t bytes = 0; uint32_t batch = 0;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_path_state_bytes((fspt_target *)h, &bytes, &batch));
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_double(env, (double)bytes, &v));
  NAPI_OK(napi_set_named_property(env, o, "bytes", v));
  NAPI_OK(napi_create_uint32(env, batch, &v));
  NAPI_OK(napi_set_named_property(env, o, "batchTicks", v));
  return o;
}
static napi_value Prepare(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  FSPT_OK_OR_THROW(fspt_target_prepare((fspt_target *)h));
  return undefined(env);
}
static napi_value EnableCounters(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; bool on;
  if (get_args(env, info, 2, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  NAPI_OK(napi_get_value_bool(env, a[1], &on));
  FSPT_OK_OR_THROW(fspt_enable_counters((fspt_target *)h, on ? 1 : 0));
  return undefined(env);
}
static napi_value GetCounters(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a) || unwrap_k(env, a[0], H_TARGET, &h)) return NULL;
  fspt_counters c;
  FSPT_OK_OR_THROW(fspt_get_counters((fspt_target *)h, &c));
  napi_value o, v;
  NAPI_OK(napi_create_object(env, &o));
  const char *names[6] = {"samples", "rays", "steps", "leaves", "shades", "envLookups"};
  uint64_t vals[6] = {c.samples, c.rays, c.steps, c.leaves, c.shades, c.env_lookups};
  for (int i = 0; i < 6; ++i) {
    NAPI_OK(napi_create_double(env, (double)vals[i], &v));
    NAPI_OK(napi_set_named_property(env, o, names[i], v));
  }
  return o;
}

/* --------------------------------------------------------- scene pipeline */
static napi_value f32_out(napi_env env, size_t n, float **data) {
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, n * 4, (void **)data, &ab) != napi_ok) return NULL;
  if (napi_create_typedarray(env, napi_float32_array, n, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}
/* --- native scene builder, one call per fspt_builder_* entry point (orchestrated by fspt.js buildScene) --- */
static int read_rotations(napi_env env, napi_value obj, double *rot, uint32_t cap, uint32_t *n, bool *present) {
  napi_value v;
  *n = 0; *present = false;
  if (napi_get_named_property(env, obj, "rotate", &v) != napi_ok) return 0;
  bool isarr = false;
  napi_is_array(env, v, &isarr);
  if (!isarr) return 0;
  *present = true;
  napi_get_array_length(env, v, n);
  if (*n > cap) { napi_throw_range_error(env, NULL, "fspt_napi: too many rotations (max 16)"); return -1; }
  for (uint32_t r = 0; r < *n; ++r) {
    napi_value re, ax, e;
    napi_get_element(env, v, r, &re);
    if (prop(env, re, "axis", &ax)) return -1;
    for (uint32_t k = 0; k < 3; ++k) { napi_get_element(env, ax, k, &e); if (get_f64(env, e, &rot[4 * r + k])) return -1; }
    if (prop_f64(env, re, "angle", 0.0, &rot[4 * r + 3])) return -1;
  }
  return 0;
}
static int read_vec3(napi_env env, napi_value obj, const char *name, double *out, bool *present) {
  napi_value v;
  *present = false;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
  bool isarr = false;
  napi_is_array(env, v, &isarr);
  if (!isarr) return 0;
  *present = true;
  for (uint32_t k = 0; k < 3; ++k) { napi_value e; napi_get_element(env, v, k, &e); if (get_f64(env, e, &out[k])) return -1; }
  return 0;
}
static char *dup_string(napi_env env, napi_value v, size_t *len) {
  if (napi_get_value_string_utf8(env, v, NULL, 0, len) != napi_ok) { napi_throw_type_error(env, NULL, "fspt_napi: expected a string"); return NULL; }
  char *text = (char *)malloc(*len + 1);
  napi_get_value_string_utf8(env, v, text, *len + 1, len);
  return text;
}
static napi_value BuilderCreate(napi_env env, napi_callback_info info) {
  (void)info;
  fspt_builder *b = NULL;
  FSPT_OK_OR_THROW(fspt_builder_create(&b));
  napi_value h = make_handle(env, H_BUILDER, b, 1, NULL, NULL);
  if (!h) fspt_builder_destroy(b);
  return h;
}
static napi_value BuilderDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1]; void *h;
  if (get_args(env, info, 1, a)) return NULL;
  fspt_handle *hb;
  if (unwrap_k(env, a[0], H_BUILDER, &h) || unwrap_box(env, a[0], H_BUILDER, &hb)) return NULL;
  handle_release(env, hb);
  return undefined(env);
}
/* builderParseObj(b, objText, {rotate, scale, translate, normals}, worldTransforms[] | null, skips[] | null)
 *   -> [{name, nTris, mtllib: string | null}]   groups in the reference's iteration order */
#define MAX_WORLD 16
static napi_value BuilderParseObj(napi_env env, napi_callback_info info) {
  napi_value a[5]; void *h;
  if (get_args(env, info, 5, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  fspt_builder *b = (fspt_builder *)h;
  fspt_prop_desc pd;
  memset(&pd, 0, sizeof(pd));
  double rot[4 * 16];
  uint32_t nrot = 0; bool present;
  if (read_rotations(env, a[2], rot, 16, &nrot, &present)) return NULL;
  pd.rotate = rot; pd.n_rotate = nrot;
  if (prop_f64(env, a[2], "scale", 1.0, &pd.scale)) return NULL;
  if (read_vec3(env, a[2], "translate", pd.translate, &present)) return NULL;
  napi_value v;
  if (napi_get_named_property(env, a[2], "normals", &v) == napi_ok) {
    char buf[16]; size_t len = 0;
    if (napi_get_value_string_utf8(env, v, buf, sizeof(buf), &len) == napi_ok) {
      if (!strcmp(buf, "smooth")) pd.normals_mode = 1; else if (!strcmp(buf, "mesh")) pd.normals_mode = 2;
    }
  }
  /* scene.worldTransforms */
  fspt_world_transform wt[MAX_WORLD];
  static double wrot[MAX_WORLD][4 * 16];
  uint32_t nworld = 0;
  bool isarr = false;
  memset(wt, 0, sizeof(wt));
  napi_is_array(env, a[3], &isarr);
  if (isarr) {
    napi_get_array_length(env, a[3], &nworld);
    if (nworld > MAX_WORLD) { napi_throw_range_error(env, NULL, "fspt_napi: too many worldTransforms (max 16)"); return NULL; }
    for (uint32_t i = 0; i < nworld; ++i) {
      napi_value e; bool has;
      napi_get_element(env, a[3], i, &e);
      if (read_rotations(env, e, wrot[i], 16, &wt[i].n_rotate, &has)) return NULL;
      wt[i].rotate = wrot[i]; wt[i].has_rotate = has ? 1u : 0u;
      if (!has) { if (read_vec3(env, e, "translate", wt[i].translate, &has)) return NULL; wt[i].has_translate = has ? 1u : 0u; }
    }
  }
  /* prop.skips */
  char *skips[64]; uint32_t nskips = 0;
  napi_is_array(env, a[4], &isarr);
  if (isarr) {
    uint32_t n = 0;
    napi_get_array_length(env, a[4], &n);
    if (n > 64) n = 64;
    for (uint32_t i = 0; i < n; ++i) {
      napi_value e; size_t len;
      napi_get_element(env, a[4], i, &e);
      napi_value str;
      if (napi_coerce_to_string(env, e, &str) != napi_ok) continue;
      skips[nskips] = dup_string(env, str, &len);
      if (skips[nskips]) nskips++;
    }
  }
  size_t len = 0;
  char *text = dup_string(env, a[1], &len);
  napi_value result = NULL;
  if (text) {
    uint32_t ng = 0;
    int rc = fspt_builder_parse_obj(b, text, len, &pd, wt, nworld, (const char *const *)skips, nskips, &ng);
    free(text);
    if (rc) {
      char msg[640]; snprintf(msg, sizeof(msg), "libfspt error %d: %s", rc, fspt_last_error()); napi_throw_error(env, NULL, msg);
    } else {
      napi_create_array_with_length(env, ng, &result);
      for (uint32_t g = 0; g < ng; ++g) {
        const char *name; uint32_t nt; int32_t mi;
        fspt_builder_group_info(b, g, &name, &nt, &mi);
        napi_value o, vv;
        napi_create_object(env, &o);
        napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &vv); napi_set_named_property(env, o, "name", vv);
        napi_create_uint32(env, nt, &vv); napi_set_named_property(env, o, "nTris", vv);
        if (mi >= 0) { const char *ln; fspt_builder_mtllib_name(b, (uint32_t)mi, &ln); napi_create_string_utf8(env, ln, NAPI_AUTO_LENGTH, &vv); }
        else napi_get_null(env, &vv);
        napi_set_named_property(env, o, "mtllib", vv);
        napi_set_element(env, result, g, o);
      }
    }
  }
  for (uint32_t i = 0; i < nskips; ++i) free(skips[i]);
  return result;
}
/* builderCommit(b, [{diffuseIndex, specularIndex, normalIndex, roughnessIndex, emittance[3], ior, dielectric}]) */
static napi_value BuilderCommit(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h;
  if (get_args(env, info, 2, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, a[1], &n));
  fspt_group_material *gm = (fspt_group_material *)calloc(n ? n : 1, sizeof(*gm));
  napi_value result = NULL;
  for (uint32_t i = 0; i < n; ++i) {
    napi_value m; bool present;
    napi_get_element(env, a[1], i, &m);
    if (prop_f64(env, m, "diffuseIndex", 0, &gm[i].diffuse_layer) || prop_f64(env, m, "specularIndex", 0, &gm[i].emissive_layer) ||
        prop_f64(env, m, "normalIndex", 0, &gm[i].normal_layer) || prop_f64(env, m, "roughnessIndex", 0, &gm[i].mr_layer) ||
        prop_f64(env, m, "ior", 1.4, &gm[i].ior) || prop_f64(env, m, "dielectric", -1, &gm[i].dielectric) ||
        read_vec3(env, m, "emittance", gm[i].emittance, &present)) goto done;
  }
  {
    int rc = fspt_builder_commit_obj((fspt_builder *)h, gm, n);
    if (rc) { char msg[640]; snprintf(msg, sizeof(msg), "libfspt error %d: %s", rc, fspt_last_error()); napi_throw_error(env, NULL, msg); goto done; }
    result = undefined(env);
  }
done:
  free(gm);
  return result;
}
static napi_value BuilderNormalize(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; double size;
  if (get_args(env, info, 2, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  if (get_f64(env, a[1], &size)) return NULL;
  FSPT_OK_OR_THROW(fspt_builder_normalize((fspt_builder *)h, size));
  return undefined(env);
}
/* the built tree's arrays: {bvh,tri,mat,norm,uv: Float32Array, depth} */
static napi_value builder_arrays(napi_env env, fspt_builder *b) {
  uint32_t nn, nt, depth;
  FSPT_OK_OR_THROW(fspt_builder_counts(b, &nn, &nt, &depth));
  float *bvh, *tri, *mat, *norm, *uv;
  napi_value o, v;
  napi_create_object(env, &o);
  napi_value tb = f32_out(env, (size_t)nn * 9, &bvh), tt = f32_out(env, (size_t)nt * 9, &tri), tm = f32_out(env, (size_t)nt * 12, &mat),
             tn = f32_out(env, (size_t)nt * 27, &norm), tu = f32_out(env, (size_t)nt * 6, &uv);
  if (!tb || !tt || !tm || !tn || !tu) { napi_throw_error(env, NULL, "fspt_napi: allocation failed"); return NULL; }
  fspt_builder_get(b, bvh, tri, mat, norm, uv);
  napi_set_named_property(env, o, "bvh", tb); napi_set_named_property(env, o, "tri", tt); napi_set_named_property(env, o, "mat", tm);
  napi_set_named_property(env, o, "norm", tn); napi_set_named_property(env, o, "uv", tu);
  napi_create_uint32(env, depth, &v); napi_set_named_property(env, o, "depth", v);
  return o;
}
/* builderBuild(b, leafSize) -> {bvh,tri,mat,norm,uv: Float32Array, depth} */
static napi_value BuilderBuild(napi_env env, napi_callback_info info) {
  napi_value a[2]; void *h; uint32_t leaf = 4;
  if (get_args(env, info, 2, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &leaf));
  FSPT_OK_OR_THROW(fspt_builder_build((fspt_builder *)h, leaf));
  return builder_arrays(env, (fspt_builder *)h);
}
/* builderBuildGpu(b, leafSize, device) -> the same, from the binned-SAH tree built on `device` */
static napi_value BuilderBuildGpu(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; uint32_t leaf = 4; int32_t device = 0;
  if (get_args(env, info, 3, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &leaf));
  NAPI_OK(napi_get_value_int32(env, a[2], &device));
  FSPT_OK_OR_THROW(fspt_builder_build_gpu((fspt_builder *)h, leaf, device));
  return builder_arrays(env, (fspt_builder *)h);
}
/* builderAutofocus(b, eye[3], dir[3]) -> distance (shootAutoFocusRay, main.js:447-546) */
static napi_value BuilderAutofocus(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *h; double eye[3], dir[3], dist = 0;
  if (get_args(env, info, 3, a)) return NULL;
  if (unwrap_k(env, a[0], H_BUILDER, &h)) return NULL;
  for (uint32_t k = 0; k < 3; ++k) {
    napi_value e;
    napi_get_element(env, a[1], k, &e); if (get_f64(env, e, &eye[k])) return NULL;
    napi_get_element(env, a[2], k, &e); if (get_f64(env, e, &dir[k])) return NULL;
  }
  FSPT_OK_OR_THROW(fspt_builder_autofocus((fspt_builder *)h, eye, dir, &dist));
  napi_value v;
  NAPI_OK(napi_create_double(env, dist, &v));
  return v;
}
static napi_value EnvBins(napi_env env, napi_callback_info info) {
  napi_value a[3]; void *p; size_t n; uint32_t w, h;
  if (get_args(env, info, 3, a) || typed(env, a[0], napi_uint8_array, 0, &p, &n)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[1], &w));
  NAPI_OK(napi_get_value_uint32(env, a[2], &h));
  if (n != (size_t)w * h * 4) { napi_throw_range_error(env, NULL, "fspt_napi: rgbe length != w*h*4"); return NULL; }
  uint32_t nb = 0;
  FSPT_OK_OR_THROW(fspt_env_bins((const uint8_t *)p, w, h, NULL, 0, &nb));
  napi_value ab, ta; void *data;
  NAPI_OK(napi_create_arraybuffer(env, (size_t)nb * 16, &data, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_uint32_array, (size_t)nb * 4, ab, 0, &ta));
  FSPT_OK_OR_THROW(fspt_env_bins((const uint8_t *)p, w, h, (uint32_t *)data, nb, &nb));
  return ta;
}
static napi_value RandBaseNext(napi_env env, napi_callback_info info) {
  /* state is a BigUint64Array(1) so the 64-bit xorshift state survives the JS boundary */
  napi_value a[1]; void *p; size_t n;
  if (get_args(env, info, 1, a) || typed(env, a[0], napi_biguint64_array, 0, &p, &n) || n < 1) return NULL;
  napi_value v;
  NAPI_OK(napi_create_double(env, (double)fspt_rand_base_next((uint64_t *)p), &v));
  return v;
}
static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  napi_value v; napi_create_int32(env, fspt_device_count(), &v); return v;
}
/* deviceMemory(device) -> {free, total} in bytes (fspt_device_memory) */
static napi_value DeviceMemory(napi_env env, napi_callback_info info) {
  napi_value a[1], o, v; int32_t dev; uint64_t f = 0, t = 0;
  if (get_args(env, info, 1, a)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[0], &dev));
  FSPT_OK_OR_THROW(fspt_device_memory(dev, &f, &t));
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_double(env, (double)f, &v));
  NAPI_OK(napi_set_named_property(env, o, "free", v));
  NAPI_OK(napi_create_double(env, (double)t, &v));
  NAPI_OK(napi_set_named_property(env, o, "total", v));
  return o;
}
static napi_value AbiVersion(napi_env env, napi_callback_info info) {
  napi_value v; napi_create_int32(env, fspt_abi_version(), &v); return v;
}

static napi_value Init(napi_env env, napi_value exports) {
  struct { const char *name; napi_callback fn; } fns[] = {
      {"sceneCreate", SceneCreate}, {"sceneDestroy", SceneDestroy}, {"sceneUpdateGeometry", SceneUpdateGeometry}, {"sceneRebuildGeometry", SceneRebuildGeometry}, {"sceneSahCost", SceneSahCost}, {"sceneUpdateMaterials", SceneUpdateMaterials}, {"sceneUpdateEnvironment", SceneUpdateEnvironment}, {"sceneUpdateSky", SceneUpdateSky}, {"sceneUpdateEnvironmentAuto", SceneUpdateEnvironmentAuto}, {"skyGenerate", SkyGenerate}, {"atlasPackGpu", AtlasPackGpu}, {"sceneUpdateTextures", SceneUpdateTextures}, {"scenePatchTextures", ScenePatchTextures}, {"envBinsGpu", EnvBinsGpu}, {"sceneSetPose", SceneSetPose}, {"sceneUpdateTransforms", SceneUpdateTransforms}, {"sceneSetSkin", SceneSetSkin}, {"sceneUpdateSkin", SceneUpdateSkin}, {"sceneSetMesh", SceneSetMesh}, {"sceneUpdateVertices", SceneUpdateVertices}, {"sceneReadMesh", SceneReadMesh}, {"targetCreate", TargetCreate},
      {"targetDestroy", TargetDestroy}, {"camera", Camera}, {"trace", Trace}, {"traceTest", TraceTest}, {"render", Render}, {"clear", Clear},
      {"sync", Sync}, {"readRadiance", ReadRadiance}, {"draw", Draw}, {"present", Present}, {"jpegBound", JpegBound}, {"jpegEncode", JpegEncode}, {"drawJpeg", DrawJpeg}, {"presentJpeg", PresentJpeg}, {"pngBound", PngBound}, {"pngEncode", PngEncode}, {"pngFilteredEval", PngFilteredEval}, {"drawPng", DrawPng}, {"exrBound", ExrBound}, {"exrEncode", ExrEncode}, {"drawExr", DrawExr}, {"matteHash", MatteHash}, {"sceneSetMatte", SceneSetMatte}, {"mattes", Mattes}, {"readMattes", ReadMattes}, {"mattesLost", MattesLost}, {"exrBoundMattes", ExrBoundMattes}, {"exrEncodeMattes", ExrEncodeMattes}, {"features", Features}, {"denoise", Denoise}, {"drawDenoised", DrawDenoised}, {"temporalAccumulate", TemporalAccumulate}, {"temporalReset", TemporalReset}, {"temporalDenoise", TemporalDenoise}, {"temporalDraw", TemporalDraw}, {"temporalSetMoments", TemporalSetMoments}, {"temporalSetClamp", TemporalSetClamp}, {"setAutoExposure", SetAutoExposure}, {"exposure", Exposure}, {"exposureReset", ExposureReset}, {"setBloom", SetBloom}, {"bloom", Bloom}, {"temporalDenoiseVariance", TemporalDenoiseVariance}, {"sceneMotionBegin", SceneMotionBegin}, {"sceneMotionEnd", SceneMotionEnd}, {"setShard", SetShard}, {"setViewport", SetViewport}, {"setCameraModel", SetCameraModel}, {"cameraModel", CameraModel}, {"setSampler", SetSampler}, {"setLights", SetLights}, {"sceneSetLightBuilder", SceneSetLightBuilder}, {"sceneGetLightBuilder", SceneGetLightBuilder}, {"renderAdaptive", RenderAdaptive}, {"readSampleCounts", ReadSampleCounts}, {"setPipeline", SetPipeline}, {"setPool", SetPool}, {"setTraceBudget", SetTraceBudget},
      {"setMemoryLimit", SetMemoryLimit}, {"setTextureInterleaveBudget", SetTextureInterleaveBudget}, {"pathStateBytes", PathStateBytes}, {"prepare", Prepare}, {"setTail", SetTail}, {"setDeferred", SetDeferred}, {"setStageTiming", SetStageTiming},
      {"renderAsync", RenderAsync}, {"multiCreate", MultiCreate}, {"multiDestroy", MultiDestroy}, {"multiTarget", MultiTarget},
      {"multiCamera", MultiCamera}, {"multiTrace", MultiTrace}, {"multiRender", MultiRender}, {"multiRenderAsync", MultiRenderAsync},
      {"multiClear", MultiClear}, {"multiSync", MultiSync}, {"multiSetExchange", MultiSetExchange}, {"multiGetExchange", MultiGetExchange}, {"multiLastStageMs", MultiLastStageMs}, {"multiReadRadiance", MultiReadRadiance}, {"multiDraw", MultiDraw},
      {"enableCounters", EnableCounters}, {"counters", GetCounters}, {"builderCreate", BuilderCreate}, {"builderDestroy", BuilderDestroy},
      {"builderParseObj", BuilderParseObj}, {"builderCommit", BuilderCommit}, {"builderNormalize", BuilderNormalize},
      {"builderBuild", BuilderBuild}, {"builderBuildGpu", BuilderBuildGpu}, {"builderAutofocus", BuilderAutofocus}, {"envBins", EnvBins},
      {"randBaseNext", RandBaseNext}, {"deviceCount", DeviceCount}, {"deviceMemory", DeviceMemory}, {"abiVersion", AbiVersion}};
  for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
  }
  return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
