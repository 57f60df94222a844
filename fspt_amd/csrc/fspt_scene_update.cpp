// fspt_scene_update.cpp - every entry that changes a live scene, or reports on such a change: in-place geometry update
// (DESIGN 8.6), rebuild (8.7), appearance update (8.13), part transforms (8.14), skinning (8.16), the vertex-position update (8.24), the GPU sky (8.17), the motion origin (8.8)
// and the read-outs that go with them.  What the families share stands once, first - for the three deformers that fill the
// staging array that is their whole set, drop, update and read path; every refusal names the calling entry.
#include "fspt_internal.hpp"
#include "fspt_texpack_check.hpp"

// ---------------------------------------------------------------------------
// the shared steps
// ---------------------------------------------------------------------------
// A host array's finite check (p may be NULL: nothing to check).  FSPT_E_INVALID with the error set and *bad = the index.
static int check_finite(const char *fn, const char *name, const float *p, size_t n, uint64_t *bad = nullptr) {
  for (size_t i = 0; p && i < n; ++i)
    if (!std::isfinite(p[i])) {
      if (bad) *bad = i;
      fspt_set_error("%s: %s[%zu] is not finite", fn, name, i);
      return FSPT_E_INVALID;
    }
  return FSPT_OK;
}

// ... of host tri (T x 9) and norm (T x 27, may be NULL).  It needs no device: the entries refuse before anything is touched.
static int check_geometry_finite(const char *fn, size_t T, const float *tri, const float *norm) {
  const int rc = check_finite(fn, "tri", tri, T * 9);
  return rc ? rc : check_finite(fn, "norm", norm, T * 27);
}

static int refuse_not_finite_on_device(const char *fn) {
  fspt_set_error("%s: a value of tri / norm is not finite (scene unchanged)", fn);
  return FSPT_E_INVALID;
}

// (rebuild_geometry asks more of the leaves and says so in a text of its own)
static int refuse_not_refittable(const char *fn) {
  fspt_set_error("%s: scene is not refittable (the leaves' triStarts must be distinct and tile [0, n_tris), every node have one parent)", fn);
  return FSPT_E_STATE;
}

// Begin a scene change: the scene's device current, every target's earlier work done, the device idle.
static int begin_scene_change(fspt_scene *s) {
  const int rc = check_device(s->device);
  return rc ? rc : geometry_order_targets(s);
}

// Begin a refit: a scene change with the device copies of s->rf in place.
static int begin_refit(fspt_scene *s) {
  const int rc = begin_scene_change(s);
  return rc ? rc : fspt::refit_prepare(s);
}

// The staging array, tri (T x 9) | norm (T x 27): made by the first call that fills it - a host-form upload, a pose, a skin or a mesh.
// (Not a part of begin_refit: the device forms of update_geometry / rebuild_geometry never fill it and allocate nothing for it.)
static int stage_ensure(fspt_scene *s) {
  const size_t T = s->n_tris;
  if (!s->rf.stage) HIP_TRY(hipMalloc((void **)&s->rf.stage, T * 36 * 4));
  return FSPT_OK;
}

// Host tri / norm into the staging array; the arguments are re-pointed at the copies.
static int stage_upload(fspt_scene *s, const float *&tri, const float *&norm) {
  const int rc = stage_ensure(s);
  if (rc) return rc;
  const size_t T = s->n_tris;
  fspt::stage_disown(s);
  HIP_TRY(hipMemcpy(s->rf.stage, tri, T * 9 * 4, hipMemcpyHostToDevice));
  if (norm) HIP_TRY(hipMemcpy(s->rf.stage + T * 9, norm, T * 27 * 4, hipMemcpyHostToDevice));
  tri = s->rf.stage;
  if (norm) norm = s->rf.stage + T * 9;
  return FSPT_OK;
}

// fspt_scene_read_pose / _skin / _mesh: the staging array's tri / norm (either may be NULL) to the host, while it holds a
// frame of `who` that the refit accepted.  `none` / `no_norm`: the entry's texts for "no such frame" / "it fills no norm".
static int read_stage(fspt_scene *s, const char *fn, fspt_scene::StageOwner who, bool has_norm, float *tri, float *norm, const char *none, const char *no_norm) {
  if (!s || (!tri && !norm)) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  if (s->rf.stage_owner != who) { fspt_set_error("%s: %s", fn, none); return FSPT_E_STATE; }
  if (norm && !has_norm) { fspt_set_error("%s: %s", fn, no_norm); return FSPT_E_STATE; }
  const int rc = check_device(s->device);
  if (rc) return rc;
  const size_t T = s->n_tris;
  if (tri) HIP_TRY(hipMemcpy(tri, s->rf.stage, T * 9 * 4, hipMemcpyDeviceToHost));
  if (norm) HIP_TRY(hipMemcpy(norm, s->rf.stage + T * 9, T * 27 * 4, hipMemcpyDeviceToHost));
  return FSPT_OK;
}

// What the scene's targets MEASURED is forgotten: the live-path fractions behind the tail hand-over and the stream
// scheduler's run statistics; with `primary_form` the primary-form timings too.  Accumulators, path state and settings stay.
static void targets_forget_measurements(fspt_scene *s, bool primary_form) {
  for (fspt_target *t : s->targets) {
    if (primary_form) prim_reset(t);
    t->live_known = false;
    for (fspt_target::WfLane *ln : {&t->wf, &t->pr_lane}) { ln->counts_pending = false; ln->ctl_pending = false; ln->stat_key = 0; ln->stat_gen_iters = 0; }
  }
}

// New device arrays first, so that a failure leaves what the scene had: the caller swaps on hipSuccess.  An entry with
// `alloc` allocates *dst; one with `src` uploads `bytes` to *dst + at.  On an error every allocation made here is freed.
struct DevicePart { void **dst; const void *src; size_t bytes, alloc, at; };
static hipError_t alloc_and_upload(const DevicePart *parts, size_t n) {
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < n && e == hipSuccess; ++i) {
    const DevicePart &p = parts[i];
    if (p.alloc) e = hipMalloc(p.dst, p.alloc);
    if (e == hipSuccess && p.src && p.bytes) e = hipMemcpy((char *)*p.dst + p.at, p.src, p.bytes, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) return e;
  for (size_t i = 0; i < n; ++i) if (parts[i].alloc) hipFree(*parts[i].dst);
  (void)hipGetLastError();
  return e;
}

// ... and when that failed: the code, and the text with the entry's own counts in its parenthesis
static int refuse_hip(const char *fn, hipError_t e, const char *counts_fmt, ...) {
  char counts[128];
  va_list ap;
  va_start(ap, counts_fmt);
  vsnprintf(counts, sizeof(counts), counts_fmt, ap);
  va_end(ap);
  fspt_set_error("%s: %s (%s)", fn, hipGetErrorString(e), counts);
  return e == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
}

// fspt_scene_set_pose / _skin / _mesh with a NULL description: a deformer that is not set is dropped without touching a device
static int drop_deformer(fspt_scene *s, fspt_scene::StageOwner who, bool is_set) {
  if (!is_set) return FSPT_OK;
  const int rc = check_device(s->device);
  if (rc) return rc;
  fspt::deformer_release(s, who);
  return FSPT_OK;
}

// the refit of update_geometry and of the deformers proper (kernels in fspt_refit.hip): tri / norm are device
// memory, the call is ordered and s->rf prepared
static int refit_device_arrays(fspt_scene *s, const float *tri, const float *norm, const char *fn) {
  int rc = FSPT_OK;
  if (!s->quads && s->n_interior) { // a scene created from refitted boxes may have two-level nodes where this one had none
    HIP_TRY(hipMalloc(&s->quads, (size_t)s->n_interior * fspt::QUAD_F4 * 16u));
  }
  int finite = 1, quads_ok = 0;
  rc = fspt::refit_run(s, tri, norm, &finite, &quads_ok);
  if (rc) return rc;
  if (!finite) return refuse_not_finite_on_device(fn);
  s->d.quads = quads_ok ? (const float4 *)s->quads : nullptr;
  return geometry_changed_lights(s);
}

// Fill the staging array, then refit from it: what update_transforms, update_skin and update_vertices share once their
// arguments are checked.  `upload` (a host form's frame; FSPT_OK or the error) runs with the scene's device current and
// outside the timing; `enqueue` puts the deformer's kernels on the NULL stream - three passes record deform_ev[2] and [3]
// between them - and returns its launches.  *ms: first kernel to last; pass_ms / launches: may be NULL.  `who` owns the
// staging array once the refit has accepted the frame, and nobody does from the first write on until then.
template <class Upload, class Enqueue>
static int deform_and_refit(fspt_scene *s, const char *fn, fspt_scene::StageOwner who, bool has_norm, float *ms, float *pass_ms, uint32_t *launches, Upload upload, Enqueue enqueue) {
  int rc = begin_refit(s);
  if (rc || (rc = stage_ensure(s))) return rc;
  hipEvent_t *ev = s->deform_ev;
  for (int i = 0; i < 4; ++i) if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
  if ((rc = upload())) return rc;
  fspt::stage_disown(s);
  HIP_TRY(hipEventRecord(ev[0], nullptr));
  const uint32_t n = enqueue();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev[1], nullptr));
  HIP_TRY(hipEventSynchronize(ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, ev[0], ev[1]));
  if (launches) *launches = n;
  if (pass_ms) {
    pass_ms[0] = *ms; pass_ms[1] = pass_ms[2] = 0.0f;
    if (n == 3) { // faces | vertex normals | smooth frames
      HIP_TRY(hipEventElapsedTime(&pass_ms[0], ev[0], ev[2]));
      HIP_TRY(hipEventElapsedTime(&pass_ms[1], ev[2], ev[3]));
      HIP_TRY(hipEventElapsedTime(&pass_ms[2], ev[3], ev[1]));
    }
  }
  const size_t T = s->n_tris;
  if ((rc = refit_device_arrays(s, s->rf.stage, has_norm ? s->rf.stage + T * 9 : nullptr, fn))) return rc;
  s->rf.stage_owner = who; // (a refused frame is not handed out by fspt_scene_read_pose / _skin / _mesh)
  return FSPT_OK;
}

extern "C" {

// ---------------------------------------------------------------------------
// in-place geometry update (kernels in fspt_refit.hip)
// ---------------------------------------------------------------------------
static int update_geometry(fspt_scene *s, const float *tri, const float *norm, bool on_device, const char *fn) {
  if (!s || !tri) { fspt_set_error("%s: NULL scene or tri", fn); return FSPT_E_INVALID; }
  int rc = FSPT_OK;
  if (!on_device && (rc = check_geometry_finite(fn, s->n_tris, tri, norm))) return rc;
  if (!s->rf.ok) return refuse_not_refittable(fn);
  if ((rc = begin_refit(s))) return rc;
  if (!on_device && (rc = stage_upload(s, tri, norm))) return rc;
  return refit_device_arrays(s, tri, norm, fn);
}

int fspt_scene_update_geometry(fspt_scene *s, const float *tri, const float *norm) {
  return update_geometry(s, tri, norm, false, "fspt_scene_update_geometry");
}

int fspt_scene_update_geometry_device(fspt_scene *s, const float *tri, const float *norm) {
  return update_geometry(s, tri, norm, true, "fspt_scene_update_geometry_device");
}

int fspt_scene_last_update_ms(fspt_scene *s, float *ms, uint32_t *launches) {
  if (!s) { fspt_set_error("fspt_scene_last_update_ms: NULL scene"); return FSPT_E_INVALID; }
  if (ms) *ms = s->rf.last_ms;
  if (launches) *launches = s->rf.last_launches;
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// GPU part transforms (kernel in fspt_pose.hip)
// ---------------------------------------------------------------------------
// The rule's host part, float64 in the stated order (tests/pose_ref.py restates it): per part a (12) | D (9) | N (9).
// NULL: every part is fine; else the reason, with *bad = the part.
static const char *pose_matrices(const float *xf, uint32_t n_parts, float *out, uint32_t *bad) {
  for (uint32_t p = 0; p < n_parts; ++p) {
    const float *x = xf + (size_t)p * 12;
    float *o = out + (size_t)p * 30;
    *bad = p;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(x[i])) return "an entry is not finite";
    double A[3][3], Cf[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = (double)x[4 * i + j];
    double q = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) q = q + A[i][j] * A[i][j];
    const double g = std::sqrt(q / 3.0);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        Cf[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1];
      }
    const double det = (A[0][0] * Cf[0][0] + A[0][1] * Cf[0][1]) + A[0][2] * Cf[0][2];
    if (det == 0.0) return "the matrix is singular";
    const double gg = g * g;
    for (int i = 0; i < 12; ++i) o[i] = x[i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        o[12 + 3 * i + j] = (float)(A[i][j] / g);
        o[21 + 3 * i + j] = (float)(Cf[i][j] / gg);
      }
    for (int i = 12; i < 30; ++i) if (!std::isfinite(o[i])) return "a derived matrix is not finite";
  }
  return nullptr;
}

int fspt_pose_matrices_eval(const float *xf, uint32_t n_parts, float *out, uint32_t *bad_part) {
  if (!xf || !out || n_parts == 0) { fspt_set_error("fspt_pose_matrices_eval: NULL/empty argument"); return FSPT_E_INVALID; }
  uint32_t bad = 0;
  if (const char *why = pose_matrices(xf, n_parts, out, &bad)) {
    if (bad_part) *bad_part = bad;
    fspt_set_error("fspt_pose_matrices_eval: part %u: %s", bad, why);
    return FSPT_E_INVALID;
  }
  return FSPT_OK;
}

int fspt_scene_set_pose(fspt_scene *s, const uint32_t *part, uint32_t n_parts, const float *tri, const float *norm) {
  if (!s) { fspt_set_error("fspt_scene_set_pose: NULL scene"); return FSPT_E_INVALID; }
  if (!part) return drop_deformer(s, fspt_scene::STAGE_POSE, s->pose.part || s->pose.mats);
  if (!tri || n_parts == 0) { fspt_set_error("fspt_scene_set_pose: tri is NULL or n_parts is 0"); return FSPT_E_INVALID; }
  const size_t T = s->n_tris;
  for (size_t i = 0; i < T; ++i) if (part[i] >= n_parts) { fspt_set_error("fspt_scene_set_pose: part[%zu] = %u, n_parts = %u", i, part[i], n_parts); return FSPT_E_INVALID; }
  int rc = check_geometry_finite("fspt_scene_set_pose", T, tri, norm);
  if (rc) return rc;
  if (!s->rf.ok) return refuse_not_refittable("fspt_scene_set_pose");
  if ((rc = check_device(s->device))) return rc;
  // the new arrays first: an allocation that fails leaves the old pose
  uint32_t *d_part = nullptr;
  float *d_rest = nullptr;
  const size_t T1 = T ? T : 1;
  const DevicePart parts[] = {{(void **)&d_part, part, T * 4, T1 * 4, 0}, {(void **)&d_rest, tri, T * 36, T1 * (norm ? 144 : 36), 0},
                              {(void **)&d_rest, norm, T * 108, 0, T * 36}};
  const hipError_t e = alloc_and_upload(parts, 3);
  if (e != hipSuccess) return refuse_hip("fspt_scene_set_pose", e, "%zu triangles", T);
  hipFree(s->pose.part); hipFree(s->pose.rest); // (pose.mats stays: it holds matrices, whatever the triangles)
  s->pose.part = d_part; s->pose.rest = d_rest;
  s->pose.has_norm = norm != nullptr;
  s->pose.n_parts = n_parts;
  fspt::stage_disown(s, fspt_scene::STAGE_POSE);
  return FSPT_OK;
}

int fspt_scene_update_transforms(fspt_scene *s, const float *xf, uint32_t n_parts) {
  if (!s || !xf) { fspt_set_error("fspt_scene_update_transforms: NULL scene or xf"); return FSPT_E_INVALID; }
  if (!s->pose.part) { fspt_set_error("fspt_scene_update_transforms: the scene has no pose (fspt_scene_set_pose)"); return FSPT_E_STATE; }
  if (n_parts != s->pose.n_parts) { fspt_set_error("fspt_scene_update_transforms: %u matrices, the pose has %u parts", n_parts, s->pose.n_parts); return FSPT_E_INVALID; }
  std::vector<float> mats((size_t)n_parts * 30);
  uint32_t bad = 0;
  if (const char *why = pose_matrices(xf, n_parts, mats.data(), &bad)) {
    fspt_set_error("fspt_scene_update_transforms: part %u: %s (scene unchanged)", bad, why);
    return FSPT_E_INVALID;
  }
  return deform_and_refit(s, "fspt_scene_update_transforms", fspt_scene::STAGE_POSE, s->pose.has_norm, &s->pose.last_ms, nullptr, nullptr,
                          [&] { return fspt::pose_upload(s->pose, mats.data()); }, [&] { return fspt::pose_run(s); });
}

int fspt_scene_read_pose(fspt_scene *s, float *tri, float *norm) {
  return read_stage(s, "fspt_scene_read_pose", fspt_scene::STAGE_POSE, s && s->pose.has_norm, tri, norm,
                    "no fspt_scene_update_transforms since the pose was set, the scene rebuilt or its geometry uploaded", "the pose has no rest norm");
}

int fspt_scene_last_pose_ms(fspt_scene *s, float *transform_ms, float *refit_ms, uint32_t *launches) {
  if (!s) { fspt_set_error("fspt_scene_last_pose_ms: NULL scene"); return FSPT_E_INVALID; }
  if (transform_ms) *transform_ms = s->pose.last_ms;
  if (refit_ms) *refit_ms = s->rf.last_ms;
  if (launches) *launches = s->rf.last_launches + 1u;
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// GPU skinning (kernel in fspt_pose.hip)
// ---------------------------------------------------------------------------
// fspt_scene_set_skin's validation: host only.  FSPT_OK, or FSPT_E_INVALID with the error set and *bad = the index.
static int skin_check(const fspt_skin_desc *d, size_t T, const char *fn, uint64_t *bad) {
  if (!d || !d->joints || !d->weights || !d->tri) { fspt_set_error("%s: joints, weights or tri is NULL", fn); return FSPT_E_INVALID; }
  if (d->n_joints < 1 || d->n_joints > 65535) { fspt_set_error("%s: n_joints = %u, must lie in [1, 65535]", fn, d->n_joints); return FSPT_E_INVALID; }
  if (d->n_morph > FSPT_SKIN_MAX_MORPH) { fspt_set_error("%s: n_morph = %u, at most %d", fn, d->n_morph, FSPT_SKIN_MAX_MORPH); return FSPT_E_INVALID; }
  if (d->n_morph && !d->morph) { fspt_set_error("%s: n_morph = %u but morph is NULL", fn, d->n_morph); return FSPT_E_INVALID; }
  if (d->morph_norm && !d->norm) { fspt_set_error("%s: morph_norm needs a rest norm", fn); return FSPT_E_INVALID; }
  if (d->morph_norm && !d->n_morph) { fspt_set_error("%s: morph_norm given with n_morph = 0", fn); return FSPT_E_INVALID; }
  const size_t slots = T * 12;
  for (size_t i = 0; i < slots; ++i)
    if (d->joints[i] >= d->n_joints) { *bad = i; fspt_set_error("%s: joints[%zu] = %u, n_joints = %u", fn, i, (unsigned)d->joints[i], d->n_joints); return FSPT_E_INVALID; }
  const struct { const char *name; const float *p; size_t n; } arrays[] = {
      {"weights", d->weights, slots}, {"tri", d->tri, T * 9}, {"norm", d->norm, T * 27},
      {"morph", d->n_morph ? d->morph : nullptr, (size_t)d->n_morph * T * 9}, {"morph_norm", d->morph_norm, (size_t)d->n_morph * T * 27}};
  for (const auto &a : arrays)
    if (const int rc = check_finite(fn, a.name, a.p, a.n, bad)) return rc;
  return FSPT_OK;
}

int fspt_skin_check_eval(const fspt_skin_desc *d, uint32_t n_tris, uint64_t *bad_index) {
  uint64_t bad = 0;
  const int rc = skin_check(d, n_tris, "fspt_skin_check_eval", &bad);
  if (rc && bad_index) *bad_index = bad;
  return rc;
}

int fspt_skin_set_form(int form) {
  if (form != 0 && form != 1) { fspt_set_error("fspt_skin_set_form: form must be 0 or 1"); return FSPT_E_INVALID; }
  fspt::g_skin_form = form;
  return FSPT_OK;
}

int fspt_scene_set_skin(fspt_scene *s, const fspt_skin_desc *d) {
  if (!s) { fspt_set_error("fspt_scene_set_skin: NULL scene"); return FSPT_E_INVALID; }
  if (!d) return drop_deformer(s, fspt_scene::STAGE_SKIN, s->skin.joints != nullptr);
  const size_t T = s->n_tris;
  uint64_t bad = 0;
  int rc = skin_check(d, T, "fspt_scene_set_skin", &bad);
  if (rc) return rc;
  if (!s->rf.ok) return refuse_not_refittable("fspt_scene_set_skin");
  rc = check_device(s->device);
  if (rc) return rc;
  // the new arrays first: an allocation that fails leaves the old skin
  fspt_scene::Skin N;
  const size_t T1 = T ? T : 1, M = d->n_morph;
  const DevicePart parts[] = {
      {(void **)&N.joints, d->joints, T * 24, T1 * 24, 0}, {(void **)&N.weights, d->weights, T * 48, T1 * 48, 0},
      {(void **)&N.rest, d->tri, T * 36, T1 * (d->norm ? 144 : 36), 0},
      {(void **)&N.morph, d->morph, M * T * 36, M * T1 * 36, 0}, {(void **)&N.morph_norm, d->morph_norm, M * T * 108, d->morph_norm ? M * T1 * 108 : 0, 0},
      {(void **)&N.frame, nullptr, 0, (size_t)d->n_joints * 48 + M * 4, 0}, {(void **)&N.rest, d->norm, T * 108, 0, T * 36}};
  const hipError_t e = alloc_and_upload(parts, sizeof(parts) / sizeof(parts[0]));
  if (e != hipSuccess) return refuse_hip("fspt_scene_set_skin", e, "%zu triangles, %u joints, %u morph targets", T, d->n_joints, d->n_morph);
  N.has_norm = d->norm != nullptr;
  N.n_joints = d->n_joints;
  N.n_morph = d->n_morph;
  fspt::deformer_release(s, fspt_scene::STAGE_SKIN);
  s->skin = N;
  return FSPT_OK;
}

static int update_skin(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph, bool on_device, const char *fn) {
  if (!s || !xf) { fspt_set_error("%s: NULL scene or xf", fn); return FSPT_E_INVALID; }
  const fspt_scene::Skin &K = s->skin;
  if (!K.joints) { fspt_set_error("%s: the scene has no skin (fspt_scene_set_skin)", fn); return FSPT_E_STATE; }
  if (n_joints != K.n_joints) { fspt_set_error("%s: %u matrices, the skin has %u joints", fn, n_joints, K.n_joints); return FSPT_E_INVALID; }
  if (n_morph != K.n_morph) { fspt_set_error("%s: %u morph weights, the skin has %u targets", fn, n_morph, K.n_morph); return FSPT_E_INVALID; }
  if (n_morph && !morph_w) { fspt_set_error("%s: morph_w is NULL, the skin has %u targets", fn, n_morph); return FSPT_E_INVALID; }
  if (on_device) {
    if ((uintptr_t)xf % 16) { fspt_set_error("%s: xf must be 16-byte aligned", fn); return FSPT_E_INVALID; }
  } else { // the host form's check needs no device: refuse before anything is touched
    for (uint32_t j = 0; j < n_joints; ++j)
      for (int i = 0; i < 12; ++i)
        if (!std::isfinite(xf[(size_t)j * 12 + i])) { fspt_set_error("%s: joint %u: an entry is not finite (scene unchanged)", fn, j); return FSPT_E_INVALID; }
    for (uint32_t m = 0; m < n_morph; ++m)
      if (!std::isfinite(morph_w[m])) { fspt_set_error("%s: morph target %u: its weight is not finite (scene unchanged)", fn, m); return FSPT_E_INVALID; }
  }
  // the host form's frame goes to the skin's own buffer: n_joints x 12 floats | n_morph weights
  const float *d_xf = on_device ? xf : K.frame, *d_w = on_device ? morph_w : K.frame + (size_t)K.n_joints * 12;
  return deform_and_refit(s, fn, fspt_scene::STAGE_SKIN, K.has_norm, &s->skin.last_ms, nullptr, nullptr,
                          [&] { return on_device ? FSPT_OK : fspt::skin_upload(s->skin, xf, morph_w); }, [&] { return fspt::skin_run(s, d_xf, d_w); });
}

int fspt_scene_update_skin(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph) {
  return update_skin(s, xf, n_joints, morph_w, n_morph, false, "fspt_scene_update_skin");
}

int fspt_scene_update_skin_device(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph) {
  return update_skin(s, xf, n_joints, morph_w, n_morph, true, "fspt_scene_update_skin_device");
}

int fspt_scene_read_skin(fspt_scene *s, float *tri, float *norm) {
  return read_stage(s, "fspt_scene_read_skin", fspt_scene::STAGE_SKIN, s && s->skin.has_norm, tri, norm,
                    "no fspt_scene_update_skin since the skin was set, the scene rebuilt, posed or its geometry uploaded", "the skin has no rest norm");
}

int fspt_scene_last_skin_ms(fspt_scene *s, float *skin_ms, float *refit_ms, uint32_t *launches, uint64_t *bytes) {
  if (!s) { fspt_set_error("fspt_scene_last_skin_ms: NULL scene"); return FSPT_E_INVALID; }
  if (skin_ms) *skin_ms = s->skin.last_ms;
  if (refit_ms) *refit_ms = s->rf.last_ms;
  if (launches) *launches = s->rf.last_launches + 1u;
  if (bytes) *bytes = fspt::deform_bytes(fspt::deform_arrays(s->skin, s->n_tris));
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// vertex-position update (kernels in fspt_pose.hip)
// ---------------------------------------------------------------------------
// What fspt_scene_set_mesh derives on the host, once: the uv constants of calcTangents in float64 (scene_build.cpp's
// statement of obj_loader.js:72-84), the face words, and the vertex -> face rows sorted by rank.
struct MeshHost {
  std::vector<double> cst;
  std::vector<uint32_t> face, adj_off, adj_face;
  bool any_static = false, any_smooth = false;
};

// fspt_scene_set_mesh's validation and host work: no device.  FSPT_OK, or FSPT_E_INVALID with the error set and *bad = the index.
static int mesh_check(const fspt_mesh_desc *d, size_t T, const char *fn, uint64_t *bad, MeshHost &H) {
  if (!d || !d->vertex || !d->uv) { fspt_set_error("%s: the description, vertex or uv is NULL", fn); return FSPT_E_INVALID; }
  if (d->n_vertices == 0 || d->n_vertices == FSPT_MESH_STATIC) { fspt_set_error("%s: n_vertices = %u, must lie in [1, 2^32 - 2]", fn, d->n_vertices); return FSPT_E_INVALID; }
  if (T >= (1u << 31)) { fspt_set_error("%s: %zu triangles, at most 2^31 - 1", fn, T); return FSPT_E_INVALID; }
  H.cst.assign(T * 3, 0.0);
  H.face.resize(T);
  const double EPS = 2.220446049250313e-16; // Number.EPSILON
  for (size_t t = 0; t < T; ++t) {
    const uint32_t *v = d->vertex + t * 3;
    const int n_static = (v[0] == FSPT_MESH_STATIC) + (v[1] == FSPT_MESH_STATIC) + (v[2] == FSPT_MESH_STATIC);
    const bool smooth = d->smooth && d->smooth[t];
    H.face[t] = (uint32_t)t | (smooth && !n_static ? 0x80000000u : 0u);
    if (n_static == 3) {
      if (!d->tri || !d->norm) { *bad = t; fspt_set_error("%s: triangle %zu is static but the rest tri / norm is NULL", fn, t); return FSPT_E_INVALID; }
      for (size_t i = 0; i < 36; ++i) {
        const float x = i < 9 ? d->tri[t * 9 + i] : d->norm[t * 27 + (i - 9)];
        if (!std::isfinite(x)) { *bad = t; fspt_set_error("%s: static triangle %zu: a rest value is not finite", fn, t); return FSPT_E_INVALID; }
      }
      H.any_static = true;
      continue;
    }
    if (n_static) { *bad = t; fspt_set_error("%s: triangle %zu is only partly static", fn, t); return FSPT_E_INVALID; }
    for (int i = 0; i < 3; ++i)
      if (v[i] >= d->n_vertices) { *bad = t * 3 + i; fspt_set_error("%s: vertex[%zu] = %u, n_vertices = %u", fn, t * 3 + i, v[i], d->n_vertices); return FSPT_E_INVALID; }
    double uv[3][2];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 2; ++k) {
        const double raw = d->uv[t * 6 + i * 2 + k];
        if (!std::isfinite(raw)) { *bad = t * 6 + i * 2 + k; fspt_set_error("%s: uv[%zu] is not finite (a triangle without vt can only be static)", fn, t * 6 + i * 2 + k); return FSPT_E_INVALID; }
        uv[i][k] = raw + EPS * (i + 1);
      }
    const double du0[2] = {uv[1][0] - uv[0][0], uv[1][1] - uv[0][1]};
    const double du1[2] = {uv[2][0] - uv[0][0], uv[2][1] - uv[0][1]};
    const double r = 1.0 / ((du0[0] * du1[1]) - (du0[1] * du1[0]));
    H.cst[t * 3] = du1[1]; H.cst[t * 3 + 1] = du0[1]; H.cst[t * 3 + 2] = r; // (r may be inf / NaN: degenerate uvs, the quirk's case)
    H.any_smooth = H.any_smooth || smooth;
  }
  // the order the face normals are summed in
  std::vector<uint32_t> by_rank(T);
  for (size_t t = 0; t < T; ++t) by_rank[t] = (uint32_t)t;
  if (d->rank) {
    std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) { return d->rank[a] < d->rank[b]; });
    for (size_t k = 1; k < T; ++k)
      if (d->rank[by_rank[k]] == d->rank[by_rank[k - 1]]) { *bad = by_rank[k]; fspt_set_error("%s: rank %u is given to triangles %u and %u", fn, d->rank[by_rank[k]], by_rank[k - 1], by_rank[k]); return FSPT_E_INVALID; }
  }
  if (!H.any_smooth) return FSPT_OK;
  H.adj_off.assign((size_t)d->n_vertices + 1, 0u);
  for (size_t t = 0; t < T; ++t)
    for (int i = 0; i < 3; ++i)
      if (d->vertex[t * 3 + i] != FSPT_MESH_STATIC) ++H.adj_off[(size_t)d->vertex[t * 3 + i] + 1];
  for (size_t v = 0; v < d->n_vertices; ++v) H.adj_off[v + 1] += H.adj_off[v];
  H.adj_face.resize(H.adj_off[d->n_vertices]);
  std::vector<uint32_t> at(H.adj_off.begin(), H.adj_off.end() - 1);
  for (size_t k = 0; k < T; ++k) { // a face that names a vertex twice is pushed twice (obj_loader.js:154-158)
    const uint32_t t = by_rank[k];
    for (int i = 0; i < 3; ++i)
      if (d->vertex[(size_t)t * 3 + i] != FSPT_MESH_STATIC) H.adj_face[at[d->vertex[(size_t)t * 3 + i]]++] = t;
  }
  return FSPT_OK;
}

// the device side of a checked description; the new arrays first (a failure leaves *out untouched and frees its own)
static hipError_t mesh_upload(const fspt_mesh_desc *d, size_t T, const MeshHost &H, fspt_scene::Mesh *out) {
  fspt_scene::Mesh N;
  const size_t T1 = T ? T : 1, nv = d->n_vertices, na = H.adj_face.size();
  const bool sm = H.any_smooth, st = H.any_static;
  const DevicePart parts[] = {
      {(void **)&N.vertex, d->vertex, T * 12, T1 * 12, 0}, {(void **)&N.cst, H.cst.data(), T * 24, T1 * 24, 0}, {(void **)&N.face, H.face.data(), T * 4, T1 * 4, 0},
      {(void **)&N.pos, nullptr, 0, nv * 12, 0},
      {(void **)&N.rest, st ? d->tri : nullptr, T * 36, st ? T1 * 144 : 0, 0}, {(void **)&N.rest, st ? d->norm : nullptr, T * 108, 0, T * 36},
      {(void **)&N.adj_off, sm ? H.adj_off.data() : nullptr, (nv + 1) * 4, sm ? (nv + 1) * 4 : 0, 0},
      {(void **)&N.adj_face, sm ? H.adj_face.data() : nullptr, na * 4, sm ? (na ? na : 1) * 4 : 0, 0},
      {(void **)&N.fnorm, nullptr, 0, sm ? T1 * 24 : 0, 0}, {(void **)&N.vnorm, nullptr, 0, sm ? nv * 24 : 0, 0}};
  const hipError_t e = alloc_and_upload(parts, sizeof(parts) / sizeof(parts[0]));
  if (e != hipSuccess) return e;
  N.n_vertices = d->n_vertices;
  N.n_adj = (uint32_t)na;
  *out = N;
  return hipSuccess;
}

int fspt_scene_set_mesh(fspt_scene *s, const fspt_mesh_desc *d) {
  const char *fn = "fspt_scene_set_mesh";
  if (!s) { fspt_set_error("%s: NULL scene", fn); return FSPT_E_INVALID; }
  if (!d) return drop_deformer(s, fspt_scene::STAGE_MESH, s->mesh.vertex != nullptr);
  const size_t T = s->n_tris;
  uint64_t bad = 0;
  MeshHost H;
  int rc = mesh_check(d, T, fn, &bad, H);
  if (rc) return rc;
  if (!s->rf.ok) return refuse_not_refittable(fn);
  if ((rc = check_device(s->device))) return rc;
  fspt_scene::Mesh N; // the new arrays first: an allocation that fails leaves the old mesh
  const hipError_t e = mesh_upload(d, T, H, &N);
  if (e != hipSuccess) return refuse_hip(fn, e, "%zu triangles, %u vertices", T, d->n_vertices);
  fspt::deformer_release(s, fspt_scene::STAGE_MESH);
  s->mesh = N;
  return FSPT_OK;
}

static int update_vertices(fspt_scene *s, const float *pos, uint32_t n_vertices, bool on_device, const char *fn) {
  if (!s || !pos) { fspt_set_error("%s: NULL scene or pos", fn); return FSPT_E_INVALID; }
  if (!s->mesh.vertex) { fspt_set_error("%s: the scene has no mesh (fspt_scene_set_mesh)", fn); return FSPT_E_STATE; }
  if (n_vertices != s->mesh.n_vertices) { fspt_set_error("%s: %u positions, the mesh has %u vertices", fn, n_vertices, s->mesh.n_vertices); return FSPT_E_INVALID; }
  if (on_device) {
    if ((uintptr_t)pos % 4) { fspt_set_error("%s: pos must be 4-byte aligned", fn); return FSPT_E_INVALID; }
  } else if (const int rc = check_finite(fn, "pos", pos, (size_t)n_vertices * 3)) { // no device needed: refuse before anything is touched
    return rc;
  }
  fspt_scene::Mesh &M = s->mesh;
  const float *d_pos = on_device ? pos : M.pos; // the host form's frame goes to the mesh's own buffer
  return deform_and_refit(s, fn, fspt_scene::STAGE_MESH, true, &M.last_ms, M.pass_ms, &M.last_launches,
                          [&] { if (!on_device) HIP_TRY(hipMemcpy(M.pos, pos, (size_t)M.n_vertices * 12, hipMemcpyHostToDevice)); return FSPT_OK; },
                          [&] { return fspt::mesh_run(M, s->n_tris, d_pos, s->rf.stage, s->deform_ev + 2); });
}

int fspt_scene_update_vertices(fspt_scene *s, const float *pos, uint32_t n_vertices) {
  return update_vertices(s, pos, n_vertices, false, "fspt_scene_update_vertices");
}

int fspt_scene_update_vertices_device(fspt_scene *s, const float *pos, uint32_t n_vertices) {
  return update_vertices(s, pos, n_vertices, true, "fspt_scene_update_vertices_device");
}

int fspt_scene_read_mesh(fspt_scene *s, float *tri, float *norm) {
  return read_stage(s, "fspt_scene_read_mesh", fspt_scene::STAGE_MESH, true, tri, norm,
                    "no fspt_scene_update_vertices since the mesh was set, the scene rebuilt, posed, skinned or its geometry uploaded", "");
}

int fspt_scene_last_mesh_ms(fspt_scene *s, float *derive_ms, float *refit_ms, uint32_t *launches, uint64_t *bytes) {
  if (!s) { fspt_set_error("fspt_scene_last_mesh_ms: NULL scene"); return FSPT_E_INVALID; }
  if (derive_ms) *derive_ms = s->mesh.last_ms;
  if (refit_ms) *refit_ms = s->rf.last_ms;
  if (launches) *launches = s->rf.last_launches + s->mesh.last_launches;
  if (bytes) *bytes = fspt::deform_bytes(fspt::deform_arrays(s->mesh, s->n_tris));
  return FSPT_OK;
}

int fspt_scene_last_mesh_pass_ms(fspt_scene *s, float ms[3]) {
  if (!s || !ms) { fspt_set_error("fspt_scene_last_mesh_pass_ms: NULL argument"); return FSPT_E_INVALID; }
  for (int i = 0; i < 3; ++i) ms[i] = s->mesh.pass_ms[i];
  return FSPT_OK;
}

// The derive kernels alone: no scene, no refit and so no non-finite check.  The description is validated first, without a device.
int fspt_mesh_frames_eval(int device, const fspt_mesh_desc *d, uint32_t n_tris, const float *pos, float *tri_out, float *norm_out) {
  const char *fn = "fspt_mesh_frames_eval";
  uint64_t bad = 0;
  MeshHost H;
  int rc = mesh_check(d, n_tris, fn, &bad, H);
  if (rc) return rc;
  if (!pos || n_tris == 0 || (!tri_out && !norm_out)) { fspt_set_error("%s: NULL/empty argument", fn); return FSPT_E_INVALID; }
  if ((rc = check_device(device))) return rc;
  struct Temp { fspt_scene::Mesh M; float *stage = nullptr; ~Temp() { fspt::mesh_release(M); hipFree(stage); } } tmp;
  hipError_t e = mesh_upload(d, n_tris, H, &tmp.M);
  if (e == hipSuccess) e = hipMalloc((void **)&tmp.stage, (size_t)n_tris * 144);
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse_hip(fn, e, "%zu triangles, %u vertices", (size_t)n_tris, d->n_vertices); }
  HIP_TRY(hipMemcpy(tmp.M.pos, pos, (size_t)d->n_vertices * 12, hipMemcpyHostToDevice));
  fspt::mesh_run(tmp.M, n_tris, tmp.M.pos, tmp.stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  if (tri_out) HIP_TRY(hipMemcpy(tri_out, tmp.stage, (size_t)n_tris * 36, hipMemcpyDeviceToHost));
  if (norm_out) HIP_TRY(hipMemcpy(norm_out, tmp.stage + (size_t)n_tris * 9, (size_t)n_tris * 108, hipMemcpyDeviceToHost));
  return FSPT_OK;
}

int fspt_f64_probe_eval(int device, int op, const double *a, const double *b, uint32_t n, double *out) {
  if (!a || !out || !n || (op != 0 && op != 1) || (op == 1 && !b)) { fspt_set_error("fspt_f64_probe_eval: NULL/empty argument or op not 0 (sqrt) / 1 (div)"); return FSPT_E_INVALID; }
  const int rc = check_device(device);
  return rc ? rc : fspt::f64_probe_run(op, a, b, n, out);
}

// ---------------------------------------------------------------------------
// in-place rebuild (fspt_refit.hip rebuild_run)
// ---------------------------------------------------------------------------
static int rebuild_geometry(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out, bool on_device, const char *fn) {
  if (!s || !tri) { fspt_set_error("%s: NULL scene or tri", fn); return FSPT_E_INVALID; }
  int rc = FSPT_OK;
  if (!on_device && (rc = check_geometry_finite(fn, s->n_tris, tri, norm))) return rc;
  // the triangle -> old slot map needs every triangle in a slot of the leaf that owns it
  bool mapped = s->rf.ok;
  for (size_t L = 0; mapped && L < s->rf.leaf_cnt.size(); ++L) mapped = s->rf.leaf_cnt[L] <= s->d.leaf_size;
  if (!mapped) {
    fspt_set_error("%s: scene is not refittable (the leaves' triStarts must be distinct and tile [0, n_tris) in steps of at most leaf_size, every node have one parent)", fn);
    return FSPT_E_STATE;
  }
  struct Restore { int prev = -1; ~Restore() { if (prev >= 0) (void)hipSetDevice(prev); } } restore; // the caller's current device stays
  if (hipGetDevice(&restore.prev) != hipSuccess) restore.prev = -1;
  if ((rc = begin_refit(s))) return rc;
  if (!on_device) {
    // (the upload takes the staging array from its owner at once: a rebuild that fails behind it must not leave
    // fspt_scene_read_pose / _skin / _mesh handing out the uploaded arrays)
    if ((rc = stage_upload(s, tri, norm))) return rc;
  } else {
    int finite = 1;
    rc = fspt::refit_check(s, tri, norm, &finite);
    if (rc) return rc;
    if (!finite) return refuse_not_finite_on_device(fn);
  }
  rc = fspt::rebuild_run(s, tri, norm, order_out, on_device);
  if (rc) return rc;
  // Every target now behaves like one created after the rebuild.  The DScene (arrays, root_ref, stack_n, n_top, quads) is
  // copied from the scene at every launch, and the LDS stack, the launch shapes and the node form are computed from it
  // there; the suspended-traversal records are re-made by susp_ensure when stack_n changed their stride.  What a target
  // measured on the old tree is forgotten, the primary-form timings included.
  targets_forget_measurements(s, true);
  return geometry_changed_lights(s);
}

int fspt_scene_rebuild_geometry(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out) {
  return rebuild_geometry(s, tri, norm, order_out, false, "fspt_scene_rebuild_geometry");
}

int fspt_scene_rebuild_geometry_device(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out) {
  return rebuild_geometry(s, tri, norm, order_out, true, "fspt_scene_rebuild_geometry_device");
}

int fspt_scene_last_rebuild_ms(fspt_scene *s, float *build_ms, float *install_ms, float *host_ms, uint32_t *launches, uint32_t *readbacks) {
  if (!s) { fspt_set_error("fspt_scene_last_rebuild_ms: NULL scene"); return FSPT_E_INVALID; }
  if (build_ms) *build_ms = s->rb.build_ms;
  if (install_ms) *install_ms = s->rb.install_ms;
  if (host_ms) *host_ms = s->rb.host_ms;
  if (launches) *launches = s->rb.launches;
  if (readbacks) *readbacks = s->rb.readbacks;
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// in-place appearance update (kernels in fspt_appearance.hip)
// ---------------------------------------------------------------------------
int fspt_scene_update_materials(fspt_scene *s, const float *mat, const float *uv, const uint8_t *atlas, uint32_t atlas_res, uint32_t atlas_layers) {
  if (!s || !mat) { fspt_set_error("fspt_scene_update_materials: NULL scene or mat"); return FSPT_E_INVALID; }
  if (atlas && (atlas_res == 0 || atlas_layers == 0)) {
    fspt_set_error("fspt_scene_update_materials: atlas must have at least one layer");
    return FSPT_E_INVALID;
  }
  if (!atlas && !s->ap.raw) {
    fspt_set_error("fspt_scene_update_materials: atlas is NULL and no earlier call of this scene carried one");
    return FSPT_E_STATE;
  }
  int rc = begin_scene_change(s);
  if (rc) return rc;
  const bool was = s->has_dielectric;
  if ((rc = fspt::appearance_materials(s, mat, uv, atlas, atlas_res, atlas_layers))) return rc;
  // the stream scheduler's horizon and the batch scheduler's tail rule read has_dielectric at every launch; what a lane
  // measured under the other horizon (iterations a run needed, live-path fractions) is forgotten with it
  if (was != s->has_dielectric) targets_forget_measurements(s, false);
  return geometry_changed_lights(s); // the table depends on the emissive layers and their texels
}

// ---------------------------------------------------------------------------
// texture packing on the GPU (kernel in fspt_texpack.hip, checks in fspt_texpack_check.hpp)
// ---------------------------------------------------------------------------
int fspt_atlas_pack_gpu(int device, const fspt_texture_pack *p, uint8_t *atlas_out) {
  int rc = fspt::texpack_check("fspt_atlas_pack_gpu", p, false);
  if (rc) return rc;
  if (!atlas_out) { fspt_set_error("fspt_atlas_pack_gpu: NULL atlas_out"); return FSPT_E_INVALID; }
  if ((rc = check_device(device))) return rc;
  return fspt::atlas_pack_run(p, atlas_out);
}

int fspt_atlas_pack_last_ms(float *upload_ms, float *kernel_ms, float *readback_ms) {
  fspt::atlas_pack_times(upload_ms, kernel_ms, readback_ms);
  return FSPT_OK;
}

// the argument checks as a host-only hook (tests): a whole description (layer_ids NULL), or a patch of n layers against a
// retained atlas of raw_layers layers of raw_res^2 texels (raw_layers 0: none, FSPT_E_STATE)
int fspt_texture_pack_check_eval(const fspt_texture_pack *p, const uint32_t *layer_ids, uint32_t n, uint32_t raw_layers, uint32_t raw_res) {
  const char *fn = "fspt_texture_pack_check_eval";
  const bool patch = layer_ids || n;
  const int rc = fspt::texpack_check(fn, p, false, layer_ids, n, raw_layers, raw_res, patch);
  if (rc || !patch || raw_layers) return rc;
  fspt_set_error("%s: no earlier call of this scene carried an atlas to patch", fn);
  return FSPT_E_STATE;
}

// fspt_scene_update_materials with the atlas packed on the device: the same order against the targets, transaction,
// retained atlas, light table and has_dielectric handling
static int update_textures(fspt_scene *s, const float *mat, const float *uv, const uint32_t *layer_ids, uint32_t n_ids, const fspt_texture_pack *p, bool patch, bool on_device, const char *fn) {
  if (!s || (!patch && !mat)) { fspt_set_error("%s: NULL scene%s", fn, patch ? "" : " or mat"); return FSPT_E_INVALID; }
  int rc = fspt::texpack_check(fn, p, on_device, layer_ids, n_ids, s->ap.raw ? s->ap.raw_layers : 0u, s->ap.raw_res, patch);
  if (rc) return rc;
  if (patch && !s->ap.raw) {
    fspt_set_error("%s: no earlier call of this scene carried an atlas to patch", fn);
    return FSPT_E_STATE;
  }
  if ((rc = begin_scene_change(s))) return rc;
  const bool was = s->has_dielectric;
  const fspt::ApTextures tx = {p, on_device, patch ? layer_ids : nullptr, fn};
  if ((rc = fspt::appearance_materials(s, mat, uv, nullptr, 0, 0, &tx))) return rc;
  if (was != s->has_dielectric) targets_forget_measurements(s, false);
  return geometry_changed_lights(s);
}

int fspt_scene_update_textures(fspt_scene *s, const float *mat, const float *uv, const fspt_texture_pack *p) {
  return update_textures(s, mat, uv, nullptr, 0, p, false, false, "fspt_scene_update_textures");
}
int fspt_scene_update_textures_device(fspt_scene *s, const float *mat, const float *uv, const fspt_texture_pack *p) {
  return update_textures(s, mat, uv, nullptr, 0, p, false, true, "fspt_scene_update_textures_device");
}
int fspt_scene_patch_textures(fspt_scene *s, const uint32_t *layer_ids, uint32_t n, const fspt_texture_pack *p) {
  return update_textures(s, nullptr, nullptr, layer_ids, n, p, true, false, "fspt_scene_patch_textures");
}
int fspt_scene_patch_textures_device(fspt_scene *s, const uint32_t *layer_ids, uint32_t n, const fspt_texture_pack *p) {
  return update_textures(s, nullptr, nullptr, layer_ids, n, p, true, true, "fspt_scene_patch_textures_device");
}

int fspt_scene_update_environment(fspt_scene *s, const uint8_t *env, uint32_t env_w, uint32_t env_h, const uint32_t *bins, uint32_t n_bins) {
  if (!s) { fspt_set_error("fspt_scene_update_environment: NULL scene"); return FSPT_E_INVALID; }
  if (!bins || n_bins == 0) {
    fspt_set_error("fspt_scene_update_environment: radianceBins must hold at least one bin (main.js:292)");
    return FSPT_E_INVALID;
  }
  if (env && (env_w == 0 || env_h == 0)) {
    fspt_set_error("fspt_scene_update_environment: env given with zero size");
    return FSPT_E_INVALID;
  }
  const int rc = begin_scene_change(s);
  if (rc) return rc;
  return fspt::appearance_environment(s, env, env_w, env_h, bins, n_bins);
}

// ---------------------------------------------------------------------------
// GPU sky and GPU-built bins (kernels in fspt_sky.hip)
// ---------------------------------------------------------------------------
static int check_map_size(const char *fn, uint32_t w, uint32_t h) {
  if (w < 1 || w > 65535 || h < 1 || h > 65535) { fspt_set_error("%s: a map of %u x %u texels, each side must lie in [1, 65535]", fn, w, h); return FSPT_E_INVALID; }
  return FSPT_OK;
}

// fspt_tuning.h's rule, on the host alone.  *out = the parameters with a unit sun_dir (normalised in float64).
static int sky_check(const char *fn, const fspt_sky_params *p, uint32_t w, uint32_t h, fspt_sky_params *out) {
  if (!p) { fspt_set_error("%s: NULL params", fn); return FSPT_E_INVALID; }
  if (const int rc = check_map_size(fn, w, h)) return rc;
  double q = 0.0;
  for (int i = 0; i < 3; ++i) {
    if (!std::isfinite(p->sun_dir[i])) { fspt_set_error("%s: sun_dir[%d] is not finite", fn, i); return FSPT_E_INVALID; }
    q += (double)p->sun_dir[i] * (double)p->sun_dir[i];
  }
  if (!(q > 0.0)) { fspt_set_error("%s: sun_dir is zero", fn); return FSPT_E_INVALID; }
  if (!(p->turbidity >= 0.0f && p->turbidity <= 64.0f)) { fspt_set_error("%s: turbidity = %g, must lie in [0, 64]", fn, (double)p->turbidity); return FSPT_E_INVALID; }
  if (!(p->sun_intensity >= 0.0f) || !std::isfinite(p->sun_intensity)) { fspt_set_error("%s: sun_intensity = %g, must be finite and >= 0", fn, (double)p->sun_intensity); return FSPT_E_INVALID; }
  if (!(p->sun_radius > 0.0f && p->sun_radius <= 0.5f)) { fspt_set_error("%s: sun_radius = %g, must lie in (0, 0.5]", fn, (double)p->sun_radius); return FSPT_E_INVALID; }
  if (!(p->gain >= 0.0f) || !std::isfinite(p->gain)) { fspt_set_error("%s: gain = %g, must be finite and >= 0", fn, (double)p->gain); return FSPT_E_INVALID; }
  for (int i = 0; i < 3; ++i)
    if (!(p->ground_albedo[i] >= 0.0f && p->ground_albedo[i] <= 1.0f)) { fspt_set_error("%s: ground_albedo[%d] = %g, must lie in [0, 1]", fn, i, (double)p->ground_albedo[i]); return FSPT_E_INVALID; }
  if (p->view_samples < 1 || p->view_samples > FSPT_SKY_MAX_VIEW_SAMPLES) { fspt_set_error("%s: view_samples = %u, must lie in [1, %d]", fn, p->view_samples, FSPT_SKY_MAX_VIEW_SAMPLES); return FSPT_E_INVALID; }
  if (p->light_samples < 1 || p->light_samples > FSPT_SKY_MAX_LIGHT_SAMPLES) { fspt_set_error("%s: light_samples = %u, must lie in [1, %d]", fn, p->light_samples, FSPT_SKY_MAX_LIGHT_SAMPLES); return FSPT_E_INVALID; }
  *out = *p;
  const double len = std::sqrt(q);
  for (int i = 0; i < 3; ++i) out->sun_dir[i] = (float)((double)p->sun_dir[i] / len);
  return FSPT_OK;
}

int fspt_sky_generate(int device, const fspt_sky_params *p, uint32_t w, uint32_t h, uint8_t *rgbe_out, float *linear_out) {
  fspt_sky_params n;
  int rc = sky_check("fspt_sky_generate", p, w, h, &n);
  if (rc || (rc = check_device(device))) return rc;
  if (!rgbe_out && !linear_out) return FSPT_OK;
  return fspt::sky_generate_run(&n, w, h, rgbe_out, linear_out);
}

int fspt_env_bins_gpu(const uint8_t *rgbe, uint32_t w, uint32_t h, int device, uint32_t *bins, uint32_t cap, uint32_t *n_bins) {
  if (!rgbe || !w || !h || !n_bins) { fspt_set_error("fspt_env_bins_gpu: NULL/empty argument"); return FSPT_E_INVALID; }
  int rc = check_map_size("fspt_env_bins_gpu", w, h);
  if (rc || (rc = check_device(device))) return rc;
  return fspt::env_bins_run(rgbe, w, h, bins, cap, n_bins);
}

int fspt_env_box_sums_eval(int device, const uint8_t *rgbe, uint32_t w, uint32_t h, const uint32_t *boxes, uint32_t n, double *out) {
  if (!rgbe || !boxes || !out || !n) { fspt_set_error("fspt_env_box_sums_eval: NULL/empty argument"); return FSPT_E_INVALID; }
  int rc = check_map_size("fspt_env_box_sums_eval", w, h);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t *b = boxes + (size_t)i * 4;
    if (b[0] > b[2] || b[2] > w || b[1] > b[3] || b[3] > h) { fspt_set_error("fspt_env_box_sums_eval: box %u = (%u, %u, %u, %u) is not inside the %u x %u map", i, b[0], b[1], b[2], b[3], w, h); return FSPT_E_INVALID; }
  }
  if ((rc = check_device(device))) return rc;
  return fspt::env_box_sums_run(rgbe, w, h, boxes, n, out);
}

static int update_environment_gpu(fspt_scene *s, const uint8_t *env, bool on_device, const fspt_sky_params *sky, uint32_t w, uint32_t h, const char *fn) {
  if (!s) { fspt_set_error("%s: NULL scene", fn); return FSPT_E_INVALID; }
  fspt_sky_params n;
  int rc = FSPT_OK;
  if (sky) {
    if ((rc = sky_check(fn, sky, w, h, &n))) return rc;
  } else {
    if (!env) { fspt_set_error("%s: env is NULL (fspt_scene_update_environment takes a scene's map away)", fn); return FSPT_E_INVALID; }
    if ((rc = check_map_size(fn, w, h))) return rc;
    if (on_device && (uintptr_t)env % 4) { fspt_set_error("%s: env must be 4-byte aligned", fn); return FSPT_E_INVALID; }
  }
  if ((rc = begin_scene_change(s))) return rc;
  return fspt::environment_gpu(s, fn, env, on_device, sky ? &n : nullptr, w, h);
}

int fspt_scene_update_environment_auto(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h) {
  return update_environment_gpu(s, env, false, nullptr, w, h, "fspt_scene_update_environment_auto");
}

int fspt_scene_update_environment_device(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h) {
  return update_environment_gpu(s, env, true, nullptr, w, h, "fspt_scene_update_environment_device");
}

int fspt_scene_update_sky(fspt_scene *s, const fspt_sky_params *p, uint32_t w, uint32_t h) {
  if (!p) { fspt_set_error("fspt_scene_update_sky: NULL params"); return FSPT_E_INVALID; }
  return update_environment_gpu(s, nullptr, false, p, w, h, "fspt_scene_update_sky");
}

int fspt_scene_last_sky_ms(fspt_scene *s, float *sky_ms, float *bins_ms, float *tile_ms, uint32_t *launches, uint32_t *readbacks, uint32_t *n_bins) {
  if (!s) { fspt_set_error("fspt_scene_last_sky_ms: NULL scene"); return FSPT_E_INVALID; }
  if (sky_ms) *sky_ms = s->sky.sky_ms;
  if (bins_ms) *bins_ms = s->sky.bins_ms;
  if (tile_ms) *tile_ms = s->sky.tile_ms;
  if (launches) *launches = s->sky.launches;
  if (readbacks) *readbacks = s->sky.readbacks;
  if (n_bins) *n_bins = s->sky.n_bins;
  return FSPT_OK;
}

int fspt_scene_read_appearance(fspt_scene *s, int what, void *out, uint64_t cap, uint64_t *bytes) {
  if (!s || what < 0 || what > 5) { fspt_set_error("fspt_scene_read_appearance: NULL scene or what not in [0, 5]"); return FSPT_E_INVALID; }
  const void *src[6] = {s->tex_sets, s->atlas, s->atlas4, s->env, s->bins, s->shade};
  const uint64_t size[6] = {(uint64_t)s->d.n_tex_sets * 48u, s->atlas_bytes, s->atlas4_bytes, s->env_bytes, (uint64_t)s->d.n_bins * 16u, (uint64_t)s->n_slots * 192u};
  if (bytes) *bytes = size[what];
  const uint64_t n = cap < size[what] ? cap : size[what];
  if (!out || !n) return FSPT_OK;
  int rc = check_device(s->device);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, src[what], n, hipMemcpyDeviceToHost));
  return FSPT_OK;
}

int fspt_scene_last_appearance_ms(fspt_scene *s, float *ms, uint32_t *launches, uint64_t *uploaded, uint64_t *retained) {
  if (!s) { fspt_set_error("fspt_scene_last_appearance_ms: NULL scene"); return FSPT_E_INVALID; }
  if (ms) *ms = s->ap.last_ms;
  if (launches) *launches = s->ap.last_launches;
  if (uploaded) *uploaded = s->ap.last_uploaded;
  if (retained) *retained = s->ap.raw ? (uint64_t)s->ap.raw_res * s->ap.raw_res * s->ap.raw_layers * 4u : 0u;
  return FSPT_OK;
}


// sum over the leaves of SA / SA(root) x triangles owned + sum over the interior nodes of SA / SA(root), float64, in the
// reference's node order, from the boxes the device holds now (a node's box sits in its parent's record; the root's is
// the union of its children's)
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) { fspt_set_error("fspt_scene_sah_cost: NULL argument"); return FSPT_E_INVALID; }
  int rc = check_device(s->device);
  if (rc) return rc;
  if (!s->n_interior) { *cost = (double)s->n_tris; return FSPT_OK; } // the root is the one leaf
  std::vector<float> nodes((size_t)s->n_interior * 16); // (only an update writes the boxes, and it has finished when it returns)
  HIP_TRY(hipMemcpy(nodes.data(), s->nodes, nodes.size() * 4, hipMemcpyDeviceToHost));
  auto area = [](const float lo[3], const float hi[3]) {
    const double e0 = (double)hi[0] - (double)lo[0], e1 = (double)hi[1] - (double)lo[1], e2 = (double)hi[2] - (double)lo[2];
    return (e0 * e1 + e0 * e2 + e1 * e2) * 2.0;
  };
  auto box_at = [&](uint32_t slot, float lo[3], float hi[3]) {
    const float *f = &nodes[(size_t)(slot >> 1) * 16];
    const uint32_t k = slot & 1u;
    lo[0] = f[4 * k]; lo[1] = f[4 * k + 1]; lo[2] = f[8 + 2 * k];
    hi[0] = f[4 * k + 2]; hi[1] = f[4 * k + 3]; hi[2] = f[9 + 2 * k];
  };
  const uint32_t NO = fspt_scene::Refit::NO_DST;
  float lo[3], hi[3], l2[3], h2[3];
  box_at(2u * (uint32_t)s->d.root_ref, lo, hi);
  box_at(2u * (uint32_t)s->d.root_ref + 1u, l2, h2);
  for (int a = 0; a < 3; ++a) { lo[a] = l2[a] < lo[a] ? l2[a] : lo[a]; hi[a] = h2[a] > hi[a] ? h2[a] : hi[a]; }
  const double root = area(lo, hi);
  double sum = root; // the root itself
  for (uint32_t i = 1; i < s->n_nodes; ++i) {
    if (s->rf.node_dst[i] == NO) continue; // not reachable from the root
    box_at(s->rf.node_dst[i], lo, hi);
    const double sa = area(lo, hi);
    sum += s->rf.node_owned[i] == NO ? sa : sa * (double)s->rf.node_owned[i];
  }
  *cost = sum / root;
  return FSPT_OK;
}

// Motion origin: floats 0-8 (v1, e1, e2) of every leaf slot's hit record as they are now.
int fspt_scene_motion_begin(fspt_scene *s) {
  if (!s) { fspt_set_error("fspt_scene_motion_begin: NULL scene"); return FSPT_E_INVALID; }
  const int rc = begin_scene_change(s); // (an accumulate in flight reads the old snapshot)
  if (rc) return rc;
  if (!s->motion) HIP_TRY(hipMalloc(&s->motion, (s->n_slots ? s->n_slots : 1) * 36));
  if (s->n_slots) HIP_TRY(hipMemcpy2D(s->motion, 36, s->shade, 192, 36, s->n_slots, hipMemcpyDeviceToDevice));
  return FSPT_OK;
}

int fspt_scene_slot_triangles(fspt_scene *s, uint32_t *n_slots, uint32_t *slot_tri) {
  if (!s || (!n_slots && !slot_tri)) { fspt_set_error("fspt_scene_slot_triangles: NULL argument"); return FSPT_E_INVALID; }
  if (n_slots) *n_slots = (uint32_t)s->n_slots;
  if (!slot_tri) return FSPT_OK;
  int rc = check_device(s->device);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(slot_tri, s->slot_tri, s->n_slots * 4, hipMemcpyDeviceToHost));
  return FSPT_OK;
}

int fspt_scene_motion_end(fspt_scene *s) {
  if (!s) { fspt_set_error("fspt_scene_motion_end: NULL scene"); return FSPT_E_INVALID; }
  if (!s->motion) return FSPT_OK;
  const int rc = begin_scene_change(s);
  if (rc) return rc;
  HIP_TRY(hipFree(s->motion));
  s->motion = nullptr;
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// ID mattes: the ids and manifests a scene carries (the pass: fspt_post.cpp fspt_mattes)
// ---------------------------------------------------------------------------
// MurmurHash3_x86_32, seed 0, then Cryptomatte's float rule: the id is read as a float, so its exponent is neither 0 nor 255
uint32_t fspt_matte_hash(const char *name, size_t len) {
  const uint8_t *d = (const uint8_t *)name;
  const auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
  uint32_t h = 0u;
  const size_t nb = name ? len / 4 : 0;
  if (!name) len = 0;
  for (size_t i = 0; i < nb; ++i) {
    uint32_t k = (uint32_t)d[4 * i] | (uint32_t)d[4 * i + 1] << 8 | (uint32_t)d[4 * i + 2] << 16 | (uint32_t)d[4 * i + 3] << 24;
    k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u;
    h ^= k; h = rotl(h, 13); h = h * 5u + 0xe6546b64u;
  }
  uint32_t k = 0u;
  const uint8_t *tail = d + nb * 4;
  switch (len & 3u) {
    case 3: k ^= (uint32_t)tail[2] << 16; // fall through
    case 2: k ^= (uint32_t)tail[1] << 8;  // fall through
    case 1: k ^= tail[0]; k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u; h ^= k;
  }
  h ^= (uint32_t)len;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  const uint32_t e = (h >> 23) & 255u;
  return e == 0u || e == 255u ? h ^ (1u << 23) : h;
}

static int matte_kind_check(const fspt_scene *s, int kind, const char *fn) {
  if (!s) { fspt_set_error("%s: NULL scene", fn); return FSPT_E_INVALID; }
  if (kind != FSPT_MATTE_OBJECT && kind != FSPT_MATTE_MATERIAL) { fspt_set_error("%s: unknown kind %d", fn, kind); return FSPT_E_INVALID; }
  return FSPT_OK;
}

int fspt_scene_set_matte_ids(fspt_scene *s, int kind, const uint32_t *ids) {
  const char *fn = "fspt_scene_set_matte_ids";
  int rc = matte_kind_check(s, kind, fn);
  if (rc) return rc;
  const size_t T = s->n_tris;
  for (size_t i = 0; ids && i < T; ++i) { // (a normal finite float: the encoder's NaN canonicalisation never touches an id)
    const uint32_t e = (ids[i] >> 23) & 255u;
    if (ids[i] != 0u && (e == 0u || e == 255u)) { fspt_set_error("%s: ids[%zu] = 0x%08x has exponent field %u (ids unchanged)", fn, i, ids[i], e); return FSPT_E_INVALID; }
  }
  if (!ids && !s->matte_ids[kind]) return FSPT_OK; // nothing to drop: no device touched
  if ((rc = begin_scene_change(s))) return rc;    // (a pass a target has enqueued reads the old table)
  uint32_t *d = nullptr;
  if (ids) {
    const DevicePart part = {(void **)&d, ids, T * 4, (T ? T : 1) * 4, 0};
    const hipError_t e = alloc_and_upload(&part, 1);
    if (e != hipSuccess) return refuse_hip(fn, e, "%zu triangles", T);
  }
  hipFree(s->matte_ids[kind]);
  s->matte_ids[kind] = d;
  return FSPT_OK;
}

int fspt_scene_set_matte_manifest(fspt_scene *s, int kind, const char *json, size_t len) {
  const char *fn = "fspt_scene_set_matte_manifest";
  const int rc = matte_kind_check(s, kind, fn);
  if (rc) return rc;
  if (len > fspt::EXR_MANIFEST_MAX) { fspt_set_error("%s: a manifest holds at most %u bytes", fn, fspt::EXR_MANIFEST_MAX); return FSPT_E_INVALID; }
  s->matte_manifest[kind].assign(json && len ? json : "", json ? len : 0);
  return FSPT_OK;
}

} // extern "C"
