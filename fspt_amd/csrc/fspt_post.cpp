// fspt_post.cpp - the image chain behind the accumulator: draw, the guided denoiser, temporal accumulation with its
// variance guidance and history clamp, auto-exposure, bloom, and their test hooks (include/fspt.h order within each).
#include "fspt_internal.hpp"

// A HIP error inside a shared helper, reported under the name of the entry point it works for
static int hip_fail(const char *fn, hipError_t e) {
  fspt_set_error("%s: %s", fn, hipGetErrorString(e));
  return FSPT_E_HIP;
}

// dst (host memory) = src (device memory) on the target's stream, and wait for it
static int read_back(fspt_target *t, void *dst, const void *src, size_t bytes, const char *fn) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  return e == hipSuccess ? FSPT_OK : hip_fail(fn, e);
}

// The timing queries: ms[k] = ev[k] -> ev[k + 1], k < n, of the last call that recorded the events (`timed`; `what` names it)
static int last_ms(fspt_target *t, float *ms, int n, const hipEvent_t *ev, bool timed, const char *fn, const char *what) {
  if (!t || !ms) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (!timed) { fspt_set_error("%s: no %s yet", fn, what); return FSPT_E_STATE; }
  hipError_t e = hipSetDevice(t->scene->device);
  if (e == hipSuccess) e = hipEventSynchronize(ev[n]);
  for (int k = 0; k < n && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
  return e == hipSuccess ? FSPT_OK : hip_fail(fn, e);
}

// Auto-exposure's metering of `src` on `st`: histogram, resolve, the events around them.
static hipError_t draw_meter(fspt_target *t, const float4 *src, hipStream_t st) {
  hipError_t e = hipEventRecord(t->ax_ev[0], st);
  if (e == hipSuccess) e = fspt::launch_exposure_histogram(src, t->W, t->vw, t->vh, t->ax_hist, fspt::g_exposure_form, st);
  if (e == hipSuccess) e = hipEventRecord(t->ax_ev[1], st);
  if (e == hipSuccess) e = fspt::launch_exposure_resolve(t->ax_hist, t->ax_state, t->ax_p, st);
  if (e == hipSuccess) e = hipEventRecord(t->ax_ev[2], st);
  return e;
}

// k_draw of `src` on `st`.  No host read, no synchronisation.
// Auto-exposure on: the buffer is metered first, on the same stream - histogram, resolve - and the draw
// multiplies the caller's exposure by the value the resolve left in device memory.
// Bloom on: behind the metering (it meters the source buffer), the pyramid chain on the same stream - down,
// tail or not, up, all into t->bl_pyr - and k_draw_bloom, which mixes up(U_1) into the texel in front of the exposure.  A
// plan of no level (a viewport one texel wide or high): the plain draw.
hipError_t draw_launch(fspt_target *t, const float4 *src, float exposure, float saturation, int denoise, float max_sigma,
                       float scale, uint32_t *out, hipStream_t st) {
  hipError_t e = hipSuccess;
  if (t->ax_on) {
    if ((e = draw_meter(t, src, st)) != hipSuccess) return e;
    t->ax_timed = true;
  }
  fspt::BloomPlan q;
  q.n = 0;
  if (t->bl_on) {
    q = fspt::bloom_plan(t->vw, t->vh, t->bl_p.levels, fspt::g_bloom_form, fspt::g_bloom_tail_texels);
    t->bl_timed = false;
  }
  const fspt::ExposureState *state = t->ax_on ? t->ax_state : nullptr;
  if (q.n) {
    e = fspt::launch_bloom_chain(src, t->W, q, t->bl_p.scatter, t->bl_pyr, t->bl_ev, nullptr, nullptr, st);
    const fspt::BloomDraw bl{t->bl_pyr + q.off[1], q.w[1], q.h[1], t->vw, t->vh, t->bl_p.intensity};
    if (e == hipSuccess) e = fspt::launch_draw(src, t->W, t->H, exposure, saturation, denoise, max_sigma, scale, out, state, &bl, st);
    if (e == hipSuccess) e = hipEventRecord(t->bl_ev[4], st);
    if (e == hipSuccess) t->bl_timed = true;
  } else {
    e = fspt::launch_draw(src, t->W, t->H, exposure, saturation, denoise, max_sigma, scale, out, state, nullptr, st);
  }
  if (e == hipSuccess && t->ax_on) e = hipEventRecord(t->ax_ev[3], st);
  return e;
}

// The drawing entries' common end: draw_launch into a scratch buffer on the target's stream, the frame copied to the host
static int draw_to_host(fspt_target *t, const float4 *src, float exposure, float saturation, int denoise, float max_sigma,
                        float scale, uint8_t *out_rgba8, const char *fn) {
  size_t n = (size_t)t->W * t->H;
  uint32_t *d = nullptr;
  HIP_TRY(hipMalloc((void **)&d, n * 4));
  hipError_t e = draw_launch(t, src, exposure, saturation, denoise, max_sigma, scale, d, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_rgba8, d, n * 4, hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  hipFree(d);
  return e == hipSuccess ? FSPT_OK : hip_fail(fn, e);
}

extern "C" {

int fspt_draw(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, uint8_t *out_rgba8) {
  return fspt_draw_scaled(t, exposure, saturation, denoise, max_sigma, 1.0f, out_rgba8);
}

int fspt_draw_scaled(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale,
                     uint8_t *out_rgba8) {
  if (!t || !out_rgba8) { fspt_set_error("fspt_draw: NULL argument"); return FSPT_E_INVALID; }
  if (!(scale > 0.0f && scale <= 1.0f)) { fspt_set_error("fspt_draw: scale must be in (0, 1]"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  return draw_to_host(t, t->accum, exposure, saturation, denoise, max_sigma, scale, out_rgba8, "fspt_draw");
}

// ---------------------------------------------------------------------------
// guided denoiser
// ---------------------------------------------------------------------------
// NULL arguments first, then the device: every call fails with FSPT_E_NO_DEVICE where no HIP device is visible
static int dn_enter(fspt_target *t, bool args_ok, const char *fn) {
  if (!t || !args_ok) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  if (fspt_device_count() <= 0) { fspt_set_error("%s: no HIP device available; libfspt has no CPU fallback", fn); return FSPT_E_NO_DEVICE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  return FSPT_OK;
}
// A mode switched off (dn_enter joined a present: once the stream is idle nothing reads the mode's buffers).  `release`
// frees them and clears what says that they hold something; post_release uses the same four functions.
static int mode_off(fspt_target *t, void (*release)(fspt_target *), const char *fn) {
  const hipError_t e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) return hip_fail(fn, e);
  release(t);
  return FSPT_OK;
}
static int dn_alloc(float4 **buf, size_t bytes) {
  if (!*buf) HIP_TRY(hipMalloc((void **)buf, bytes));
  return FSPT_OK;
}
// sigma_color, sigma_depth: +inf switches the weight off; sigma_normal: 0 switches it off (it is an exponent)
static int dn_check_params(const fspt_denoise_params &q, const char *fn) {
  if (q.iterations > 16u || !(q.sigma_color >= 0.0f) || !(q.sigma_depth > 0.0f) || !(q.sigma_normal >= 0.0f && q.sigma_normal < INFINITY)) {
    fspt_set_error("%s: need iterations <= 16, sigma_color >= 0, sigma_normal in [0, inf), sigma_depth > 0", fn);
    return FSPT_E_INVALID;
  }
  return FSPT_OK;
}
// What every filtering entry does with its parameters: the caller's or the defaults, checked
static int dn_params(const fspt_denoise_params *prm, const fspt_denoise_params &dflt, const char *fn, fspt_denoise_params &q) {
  q = prm ? *prm : dflt;
  return dn_check_params(q, fn);
}
// ... and, behind its own state checks, with the target's buffers: dn_out (whose content is no longer a result) and, for
// more than one iteration, the ping-pong pair
static int dn_buffers(fspt_target *t, const fspt_denoise_params &q) {
  const size_t px = (size_t)t->W * t->H;
  int rc = dn_alloc(&t->dn_out, px * 16);
  if (rc) return rc;
  t->dn_valid = false;
  if (q.iterations > 1u && ((rc = dn_alloc(&t->dn_tmp[0], px * 16)) || (rc = dn_alloc(&t->dn_tmp[1], px * 16)))) return rc;
  return FSPT_OK;
}
static const fspt_denoise_params DN_DEFAULTS = {FSPT_DENOISE_ITERATIONS, FSPT_DENOISE_SIGMA_COLOR, FSPT_DENOISE_SIGMA_NORMAL, FSPT_DENOISE_SIGMA_DEPTH};
// The K launches of k_atrous: src -> out (W*H float4 each) guided by feat (2 W*H float4), ping-ponging through tmp[0..1]
// (needed when K > 1); K = 0 copies src.  var == NULL: the colour-guided filter, sigma_color halving per iteration.
// Otherwise the variance-guided one: the variance from `var` into the first iteration and in the .w lane
// between them, sigma_color as sigma_l; var_out (test hook; may be NULL): the last iteration's variance
static hipError_t atrous_run(const fspt_denoise_params &q, const float4 *src, const float4 *feat, uint32_t W, uint32_t H,
                             float4 *const tmp[2], float4 *out, float *var, float *var_out, hipStream_t stream) {
  const size_t px = (size_t)W * H;
  hipError_t e = hipSuccess;
  if (q.iterations == 0) {
    if (var && var_out && (e = hipMemcpyAsync(var_out, var, px * 4, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
    return hipMemcpyAsync(out, src, px * 16, hipMemcpyDeviceToDevice, stream);
  }
  for (uint32_t k = 0; k < q.iterations; ++k) {
    fspt::AtrousP p{};
    p.src = k == 0 ? src : tmp[(k - 1) & 1u];
    p.dst = k + 1 == q.iterations ? out : tmp[k & 1u];
    p.feat = feat;
    p.W = W; p.H = H;
    p.step = 1 << k;
    p.demod = k == 0; p.remod = k + 1 == q.iterations;
    p.sn = q.sigma_normal;
    p.sz_step = std::ldexp(q.sigma_depth, (int)k);
    if (var) {
      p.var = var; p.sl = q.sigma_color;
      p.var_dst = p.remod ? var_out : nullptr;
    } else {
      p.sc_step = std::ldexp(q.sigma_color, -(int)k);
    }
    if ((e = fspt::launch_atrous(p, var != nullptr, stream)) != hipSuccess) return e;
  }
  return hipSuccess;
}

int fspt_features(fspt_target *t, const fspt_camera_params *cam, uint32_t samples, uint64_t seed) {
  int rc = dn_enter(t, cam != nullptr, "fspt_features");
  if (rc) return rc;
  if (samples == 0) { fspt_set_error("fspt_features: samples must be >= 1"); return FSPT_E_INVALID; }
  const size_t px = (size_t)t->W * t->H;
  if ((rc = dn_alloc(&t->feat, px * 32))) return rc;
  fspt::FeatureP p{};
  p.scene = t->scene->d;
  p.W = t->W; p.H = t->H;
  std::memcpy(p.cam.P, cam->P, 12); std::memcpy(p.cam.I, cam->I, 12);
  p.cam.fov_scale = cam->fov_scale; p.cam.lens[0] = cam->lens[0]; p.cam.lens[1] = cam->lens[1];
  p.samples = samples;
  p.seed = seed;
  p.feat = t->feat;
  t->feat_valid = false;
  HIP_TRY(fspt::launch_features(p, t->cam_model, t->stream)); // (the guides follow the camera model)
  t->feat_valid = true;
  return FSPT_OK;
}

int fspt_read_features(fspt_target *t, float *out) {
  int rc = dn_enter(t, out != nullptr, "fspt_read_features");
  if (rc) return rc;
  if (!t->feat_valid) { fspt_set_error("fspt_read_features: no fspt_features call yet"); return FSPT_E_STATE; }
  return read_back(t, out, t->feat, (size_t)t->W * t->H * 32, "fspt_read_features");
}

// ID mattes: k_features' rays once more, the ids of the scene's kinds ranked per pixel.  The kinds with ids
// fill the launch's tables in kind order; nothing but the matte buffers is written.
int fspt_mattes(fspt_target *t, const fspt_camera_params *cam, uint32_t samples, uint64_t seed) {
  const char *fn = "fspt_mattes";
  if (t && cam && (samples == 0 || samples > 65535u)) { fspt_set_error("%s: samples must be in 1..65535", fn); return FSPT_E_INVALID; }
  int rc = dn_enter(t, cam != nullptr, fn);
  if (rc) return rc;
  const fspt_scene *sc = t->scene;
  if (!sc->matte_ids[0] && !sc->matte_ids[1]) { fspt_set_error("%s: the scene has no matte ids (fspt_scene_set_matte_ids)", fn); return FSPT_E_STATE; }
  const size_t px = (size_t)t->W * t->H;
  if (!t->mt_lost) HIP_TRY(hipMalloc((void **)&t->mt_lost, 16));
  for (int k = 0; k < 2; ++k) if (sc->matte_ids[k] && (rc = dn_alloc(&t->mt[k], px * 48))) return rc;
  fspt::MatteP p{};
  p.f.scene = sc->d;
  p.f.W = t->W; p.f.H = t->H;
  std::memcpy(p.f.cam.P, cam->P, 12); std::memcpy(p.f.cam.I, cam->I, 12);
  p.f.cam.fov_scale = cam->fov_scale; p.f.cam.lens[0] = cam->lens[0]; p.f.cam.lens[1] = cam->lens[1];
  p.f.samples = samples;
  p.f.seed = seed;
  const int a = sc->matte_ids[0] ? 0 : 1; // table a: the first kind with ids; table b: the material ids when both have
  p.ids_a = sc->matte_ids[a]; p.out_a = t->mt[a]; p.lost_a = t->mt_lost + a;
  if (a == 0 && sc->matte_ids[1]) { p.ids_b = sc->matte_ids[1]; p.out_b = t->mt[1]; p.lost_b = t->mt_lost + 1; }
  t->mt_valid[0] = t->mt_valid[1] = false;
  HIP_TRY(fspt::launch_mattes(p, t->cam_model, t->stream));
  for (int k = 0; k < 2; ++k) t->mt_valid[k] = sc->matte_ids[k] != nullptr;
  return FSPT_OK;
}

// what fspt_read_mattes and fspt_mattes_lost start with
static int mattes_enter(fspt_target *t, int kind, bool args_ok, const char *fn) {
  if (t && args_ok && kind != FSPT_MATTE_OBJECT && kind != FSPT_MATTE_MATERIAL) { fspt_set_error("%s: unknown kind %d", fn, kind); return FSPT_E_INVALID; }
  const int rc = dn_enter(t, args_ok, fn);
  if (rc) return rc;
  if (!t->mt_valid[kind]) { fspt_set_error("%s: no fspt_mattes call yet that computed kind %d", fn, kind); return FSPT_E_STATE; }
  return FSPT_OK;
}

int fspt_read_mattes(fspt_target *t, int kind, float *out) {
  const int rc = mattes_enter(t, kind, out != nullptr, "fspt_read_mattes");
  return rc ? rc : read_back(t, out, t->mt[kind], (size_t)t->W * t->H * 48, "fspt_read_mattes");
}

int fspt_mattes_lost(fspt_target *t, int kind, uint64_t *lost) {
  const int rc = mattes_enter(t, kind, lost != nullptr, "fspt_mattes_lost");
  return rc ? rc : read_back(t, lost, t->mt_lost + kind, 8, "fspt_mattes_lost");
}

int fspt_denoise(fspt_target *t, const fspt_denoise_params *prm, float *out) {
  int rc = dn_enter(t, true, "fspt_denoise");
  if (rc) return rc;
  fspt_denoise_params q;
  if ((rc = dn_params(prm, DN_DEFAULTS, "fspt_denoise", q))) return rc;
  if (!t->feat_valid) { fspt_set_error("fspt_denoise: no fspt_features call yet"); return FSPT_E_STATE; }
  if ((rc = dn_buffers(t, q))) return rc;
  t->tm_dn_valid = false; // (dn_out is shared with fspt_temporal_denoise)
  HIP_TRY(atrous_run(q, t->accum, t->feat, t->W, t->H, t->dn_tmp, t->dn_out, nullptr, nullptr, t->stream));
  t->dn_valid = true;
  return out ? read_back(t, out, t->dn_out, (size_t)t->W * t->H * 16, "fspt_denoise") : FSPT_OK;
}

int fspt_draw_denoised(fspt_target *t, float exposure, float saturation, uint8_t *out_rgba8) {
  int rc = dn_enter(t, out_rgba8 != nullptr, "fspt_draw_denoised");
  if (rc) return rc;
  if (!t->dn_valid) { fspt_set_error("fspt_draw_denoised: no fspt_denoise call yet"); return FSPT_E_STATE; }
  return draw_to_host(t, t->dn_out, exposure, saturation, 0, 0.0f, 1.0f, out_rgba8, "fspt_draw_denoised");
}

int fspt_denoise_eval(int device, const float *accum, const float *features, uint32_t W, uint32_t H,
                      const fspt_denoise_params *prm, float *out) {
  if (!accum || !features || !out) { fspt_set_error("fspt_denoise_eval: NULL argument"); return FSPT_E_INVALID; }
  int rc = check_device(device);
  if (rc) return rc;
  fspt_denoise_params q;
  if ((rc = dn_params(prm, DN_DEFAULTS, "fspt_denoise_eval", q))) return rc;
  const size_t px = (size_t)W * H;
  if (px == 0) return FSPT_OK;
  HIP_TRY(hipSetDevice(device));
  // one allocation: accum, out, tmp[0], tmp[1] (W*H float4 each), then the features (2 W*H float4)
  Staging s(px * 16 * 6);
  if (!s.ok()) return s.done("fspt_denoise_eval");
  float4 *const d = (float4 *)s.base;
  float4 *const tmp[2] = {d + 2 * px, d + 3 * px};
  s.up(d, accum, px * 16);
  s.up(d + 4 * px, features, px * 32);
  if (s.ok()) s.e = atrous_run(q, d, d + 4 * px, W, H, tmp, d + px, nullptr, nullptr, nullptr);
  s.sync();
  s.down(out, d + px, px * 16);
  return s.done("fspt_denoise_eval");
}

// ---------------------------------------------------------------------------
// temporal accumulation (k_temporal_gbuffer / k_temporal_blend)
// ---------------------------------------------------------------------------
static int tm_check_params(const fspt_temporal_params &q, const char *fn) {
  if (!(q.alpha >= 0.0f && q.alpha <= 1.0f) || !(q.max_history >= 1.0f) || !(q.depth_tol >= 0.0f) || !(q.normal_cos >= -1.0f && q.normal_cos <= 1.0f)) {
    fspt_set_error("%s: need alpha in [0, 1], max_history >= 1, depth_tol >= 0, normal_cos in [-1, 1]", fn);
    return FSPT_E_INVALID;
  }
  return FSPT_OK;
}
static const fspt_temporal_params TM_DEFAULTS = {FSPT_TEMPORAL_ALPHA, FSPT_TEMPORAL_MAX_HISTORY, FSPT_TEMPORAL_DEPTH_TOL, FSPT_TEMPORAL_NORMAL_COS};
static void tm_fill_blend(fspt::TemporalBP &b, const fspt_temporal_params &q, uint32_t W, uint32_t H, float n) {
  b.W = W; b.H = H; b.n = n;
  b.alpha = q.alpha; b.max_history = q.max_history; b.depth_tol = q.depth_tol; b.normal_cos = q.normal_cos;
}

// The history is gone: the next accumulate is a first one.  tm_valid is the history; the four flags behind it say that a
// buffer belongs to THAT history and mean something only while tm_valid holds (every reader tests it first), so
// whatever drops the history drops them all - a buffer that depends on the history gets its flag here, nowhere else.
static void tm_drop_history(fspt_target *t) {
  t->tm_valid = false;
  t->tm_dn_valid = false;                           // (a denoised frame of the previous history is not the next one's)
  t->tm_mom_valid = false; t->tm_var_valid = false; // (the moments go with the history they describe)
  t->tm_fast_valid = false;                         // (and so does the fast history)
}

int fspt_temporal_accumulate(fspt_target *t, const fspt_camera_params *cam, const fspt_temporal_params *prm, float *out) {
  if (!t || !cam) { fspt_set_error("fspt_temporal_accumulate: NULL argument"); return FSPT_E_INVALID; }
  fspt_temporal_params q = TM_DEFAULTS;
  if (prm) q = *prm;
  int rc = tm_check_params(q, "fspt_temporal_accumulate");
  if (rc) return rc;
  if ((rc = dn_enter(t, true, "fspt_temporal_accumulate"))) return rc;
  if (t->n_shards > 1) { fspt_set_error("fspt_temporal_accumulate: sharded target (its accumulator holds a part of the frame)"); return FSPT_E_STATE; }
  if (t->cam_model.model != FSPT_CAMERA_PINHOLE) {
    fspt_set_error("fspt_temporal_accumulate: not under camera model '%s' (reprojection through a non-pinhole projection is a follow-up)", camera_model_name(t->cam_model.model));
    return FSPT_E_STATE;
  }
  if (t->vw != t->W || t->vh != t->H) { fspt_set_error("fspt_temporal_accumulate: the viewport %ux%u is smaller than the target", t->vw, t->vh); return FSPT_E_STATE; }
  if (t->acc_ticks == 0) { fspt_set_error("fspt_temporal_accumulate: the accumulator holds no sample (render first)"); return FSPT_E_STATE; }
  if (t->tm_moments && !t->feat_valid) { fspt_set_error("fspt_temporal_accumulate: moments are on and there is no fspt_features call yet (the input is demodulated by its albedo)"); return FSPT_E_STATE; }
  const size_t px = (size_t)t->W * t->H;
  for (int k = 0; k < 2; ++k) {
    if ((rc = dn_alloc(&t->tm_hist[k], px * 16)) || (rc = dn_alloc(&t->tm_g[k], px * 32))) return rc;
  }
  if ((rc = dn_alloc(&t->tm_m, px * 16))) return rc;
  for (hipEvent_t &ev : t->tm_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  const int cur = t->tm_cur, nx = cur ^ 1;
  fspt::TemporalGP g{};
  g.scene = t->scene->d;
  g.W = t->W; g.H = t->H;
  std::memcpy(g.cam.P, cam->P, 12); std::memcpy(g.cam.I, cam->I, 12);
  g.cam.fov_scale = cam->fov_scale;
  g.prev = t->tm_cam;
  g.has_prev = t->tm_valid ? 1u : 0u;
  g.origin = (const float *)t->scene->motion;
  g.g = t->tm_g[nx]; g.m = t->tm_m;
  fspt::TemporalBP b{};
  tm_fill_blend(b, q, t->W, t->H, (float)t->acc_ticks);
  b.accum = t->accum; b.m = t->tm_m; b.g = t->tm_g[nx];
  b.hist = t->tm_hist[cur]; b.g_prev = t->tm_g[cur];
  b.out = t->tm_hist[nx];
  b.has_hist = g.has_prev;
  if (t->tm_moments) { // the moments instantiation: the same taps also carry (M1, M2)
    b.feat = t->feat; b.mom_hist = t->tm_mom[cur]; b.mom_out = t->tm_mom[nx];
    b.has_mom = b.has_hist; // (the two histories start together: fspt_temporal_set_moments, fspt_temporal_reset)
  }
  if (t->tm_clamp) { // the fast-history instantiation: the same taps also carry F, capped at fast_history
    b.fast_hist = t->tm_fast[cur]; b.fast_out = t->tm_fast[nx];
    b.has_fast = b.has_hist && t->tm_fast_valid ? 1u : 0u; // (the two histories start together: fspt_temporal_set_clamp, fspt_temporal_reset)
    b.fast_history = t->tm_fast_history;
    for (hipEvent_t &ev : t->cl_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  }
  tm_drop_history(t); // (an error below leaves no half-written history behind)
  t->tm_gm_valid = false;
  t->tm_timed = false; t->cl_timed = false;
  HIP_TRY(hipEventRecord(t->tm_ev[0], t->stream));
  HIP_TRY(fspt::launch_temporal_gbuffer(g, t->stream));
  HIP_TRY(hipEventRecord(t->tm_ev[1], t->stream));
  HIP_TRY(fspt::launch_temporal_blend(b, t->stream));
  HIP_TRY(hipEventRecord(t->tm_ev[2], t->stream));
  if (t->tm_clamp) { // pass 3: the long history into the fast one's box, in place (sigma_scale = +inf: no launch, never inf * 0)
    HIP_TRY(hipEventRecord(t->cl_ev[0], t->stream));
    if (t->tm_sigma_scale != INFINITY) {
      fspt::ClampP c{};
      c.hist = t->tm_hist[nx]; c.fast = t->tm_fast[nx];
      c.W = t->W; c.H = t->H; c.sigma_scale = t->tm_sigma_scale;
      HIP_TRY(fspt::launch_temporal_clamp(c, t->stream));
    }
    HIP_TRY(hipEventRecord(t->cl_ev[1], t->stream));
    t->tm_fast_valid = true; t->cl_timed = true;
  }
  t->tm_cur = nx;
  t->tm_cam = g.cam;
  t->tm_valid = true; t->tm_gm_valid = true; t->tm_timed = true;
  t->tm_mom_valid = t->tm_moments;
  t->tm_n = (float)t->acc_ticks;
  return out ? read_back(t, out, t->tm_hist[nx], px * 16, "fspt_temporal_accumulate") : FSPT_OK;
}

int fspt_temporal_reset(fspt_target *t) {
  if (!t) { fspt_set_error("fspt_temporal_reset: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  tm_drop_history(t);
  return FSPT_OK;
}

int fspt_temporal_denoise(fspt_target *t, const fspt_denoise_params *prm, float *out) {
  int rc = dn_enter(t, true, "fspt_temporal_denoise");
  if (rc) return rc;
  fspt_denoise_params q;
  if ((rc = dn_params(prm, DN_DEFAULTS, "fspt_temporal_denoise", q))) return rc;
  if (!t->tm_valid) { fspt_set_error("fspt_temporal_denoise: no fspt_temporal_accumulate call yet"); return FSPT_E_STATE; }
  if (!t->feat_valid) { fspt_set_error("fspt_temporal_denoise: no fspt_features call yet"); return FSPT_E_STATE; }
  if ((rc = dn_buffers(t, q))) return rc;
  t->tm_dn_valid = false;
  HIP_TRY(atrous_run(q, t->tm_hist[t->tm_cur], t->feat, t->W, t->H, t->dn_tmp, t->dn_out, nullptr, nullptr, t->stream));
  t->dn_valid = true; t->tm_dn_valid = true;
  return out ? read_back(t, out, t->dn_out, (size_t)t->W * t->H * 16, "fspt_temporal_denoise") : FSPT_OK;
}

int fspt_temporal_draw(fspt_target *t, float exposure, float saturation, int denoised, uint8_t *out_rgba8) {
  int rc = dn_enter(t, out_rgba8 != nullptr, "fspt_temporal_draw");
  if (rc) return rc;
  if (!t->tm_valid) { fspt_set_error("fspt_temporal_draw: no fspt_temporal_accumulate call yet"); return FSPT_E_STATE; }
  if (denoised && !t->tm_dn_valid) { fspt_set_error("fspt_temporal_draw: no fspt_temporal_denoise call since the last fspt_temporal_accumulate / fspt_denoise"); return FSPT_E_STATE; }
  return draw_to_host(t, denoised ? t->dn_out : t->tm_hist[t->tm_cur], exposure, saturation, 0, 0.0f, 1.0f, out_rgba8, "fspt_temporal_draw");
}

int fspt_temporal_read_gbuffer(fspt_target *t, float *g_out, float *m_out) {
  int rc = dn_enter(t, g_out || m_out, "fspt_temporal_read_gbuffer");
  if (rc) return rc;
  if (!t->tm_gm_valid) { fspt_set_error("fspt_temporal_read_gbuffer: no fspt_temporal_accumulate call yet"); return FSPT_E_STATE; }
  const size_t px = (size_t)t->W * t->H;
  if (g_out) HIP_TRY(hipMemcpyAsync(g_out, t->tm_g[t->tm_cur], px * 32, hipMemcpyDeviceToHost, t->stream));
  if (m_out) HIP_TRY(hipMemcpyAsync(m_out, t->tm_m, px * 16, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

int fspt_temporal_last_ms(fspt_target *t, float ms[2]) {
  return last_ms(t, ms, 2, t ? t->tm_ev : nullptr, t && t->tm_timed, "fspt_temporal_last_ms", "fspt_temporal_accumulate call");
}

int fspt_temporal_eval(int device, const float *accum, const float *motion, const float *g, const float *hist, const float *g_prev,
                       uint32_t W, uint32_t H, uint32_t n, const fspt_temporal_params *prm, float *out) {
  if (!accum || !motion || !g || !out || (hist && !g_prev)) { fspt_set_error("fspt_temporal_eval: NULL argument"); return FSPT_E_INVALID; }
  fspt_temporal_params q = TM_DEFAULTS;
  if (prm) q = *prm;
  int rc = tm_check_params(q, "fspt_temporal_eval");
  if (rc) return rc;
  if (n == 0) { fspt_set_error("fspt_temporal_eval: n must be >= 1"); return FSPT_E_INVALID; }
  if ((rc = check_device(device))) return rc;
  const size_t px = (size_t)W * H;
  if (px == 0) return FSPT_OK;
  HIP_TRY(hipSetDevice(device));
  // one allocation, in float4: accum | motion | out | hist (px each) | g | g_prev (2 px each)
  Staging s(px * 16 * 8);
  if (!s.ok()) return s.done("fspt_temporal_eval");
  float4 *const d = (float4 *)s.base;
  s.up(d, accum, px * 16);
  s.up(d + px, motion, px * 16);
  s.up(d + 4 * px, g, px * 32);
  s.up(d + 3 * px, hist, px * 16);
  if (hist) s.up(d + 6 * px, g_prev, px * 32);
  if (s.ok()) {
    fspt::TemporalBP b{};
    tm_fill_blend(b, q, W, H, (float)n);
    b.accum = d; b.m = d + px; b.out = d + 2 * px; b.hist = d + 3 * px; b.g = d + 4 * px; b.g_prev = d + 6 * px;
    b.has_hist = hist ? 1u : 0u;
    s.e = fspt::launch_temporal_blend(b, nullptr);
  }
  s.sync();
  s.down(out, d + 2 * px, px * 16);
  return s.done("fspt_temporal_eval");
}

// ---------------------------------------------------------------------------
// SVGF variance guidance (k_temporal_blend<true> / k_svgf_variance / k_atrous<true>)
// ---------------------------------------------------------------------------
static void sv_free(fspt_target *t) {
  hipFree(t->tm_mom[0]); hipFree(t->tm_mom[1]); hipFree(t->tm_var);
  t->tm_mom[0] = t->tm_mom[1] = nullptr; t->tm_var = nullptr;
  t->tm_moments = t->tm_mom_valid = t->tm_var_valid = false;
}

int fspt_temporal_set_moments(fspt_target *t, int on) {
  int rc = dn_enter(t, true, "fspt_temporal_set_moments");
  if (rc) return rc;
  if (!on) return mode_off(t, sv_free, "fspt_temporal_set_moments");
  if (t->n_shards > 1) { fspt_set_error("fspt_temporal_set_moments: sharded target"); return FSPT_E_STATE; }
  if (t->tm_moments) return FSPT_OK;
  const size_t px = (size_t)t->W * t->H;
  for (int k = 0; k < 2; ++k) {
    if (!t->tm_mom[k]) HIP_TRY(hipMalloc((void **)&t->tm_mom[k], px * 8));
  }
  t->tm_moments = true;
  // off -> on drops the colour history with it, as fspt_temporal_reset does: moments of one frame beside a colour history
  // of N would blend at the colour's n / (N + n), stay one sample's (M2 - M1 M1 = 0) and leave the guided filter a delta
  tm_drop_history(t);
  return FSPT_OK;
}

static const fspt_denoise_params SV_DEFAULTS = {FSPT_SVGF_ITERATIONS, FSPT_SVGF_SIGMA_L, FSPT_SVGF_SIGMA_NORMAL, FSPT_SVGF_SIGMA_DEPTH};
// k_svgf_variance into `var`, `mid` (may be NULL) recorded behind it, then atrous_run's variance-guided form
static hipError_t sv_run(const fspt_denoise_params &q, const float4 *hist, const float2 *mom, const float4 *feat, uint32_t W, uint32_t H,
                         float n, float4 *const tmp[2], float4 *out, float *var, float *var_out, hipStream_t stream, hipEvent_t mid) {
  fspt::SvgfVarP v{};
  v.hist = hist; v.mom = mom; v.feat = feat; v.var = var;
  v.W = W; v.H = H; v.n = n;
  v.sn = q.sigma_normal; v.sz = q.sigma_depth;
  hipError_t e = fspt::launch_svgf_variance(v, stream);
  if (e == hipSuccess && mid) e = hipEventRecord(mid, stream);
  if (e != hipSuccess) return e;
  return atrous_run(q, hist, feat, W, H, tmp, out, var, var_out, stream);
}

int fspt_temporal_denoise_variance(fspt_target *t, const fspt_denoise_params *prm, float *out) {
  int rc = dn_enter(t, true, "fspt_temporal_denoise_variance");
  if (rc) return rc;
  fspt_denoise_params q;
  if ((rc = dn_params(prm, SV_DEFAULTS, "fspt_temporal_denoise_variance", q))) return rc;
  if (t->n_shards > 1) { fspt_set_error("fspt_temporal_denoise_variance: sharded target"); return FSPT_E_STATE; }
  if (!t->tm_moments) { fspt_set_error("fspt_temporal_denoise_variance: moments are off (fspt_temporal_set_moments)"); return FSPT_E_STATE; }
  if (!t->tm_valid || !t->tm_mom_valid) { fspt_set_error("fspt_temporal_denoise_variance: no fspt_temporal_accumulate call since the moments were switched on / the last reset"); return FSPT_E_STATE; }
  if (!t->feat_valid) { fspt_set_error("fspt_temporal_denoise_variance: no fspt_features call yet"); return FSPT_E_STATE; }
  const size_t px = (size_t)t->W * t->H;
  if ((rc = dn_buffers(t, q))) return rc;
  if (!t->tm_var) HIP_TRY(hipMalloc((void **)&t->tm_var, px * 4));
  for (hipEvent_t &ev : t->sv_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  t->tm_dn_valid = false; t->tm_var_valid = false; t->sv_timed = false;
  HIP_TRY(hipEventRecord(t->sv_ev[0], t->stream));
  HIP_TRY(sv_run(q, t->tm_hist[t->tm_cur], t->tm_mom[t->tm_cur], t->feat, t->W, t->H, t->tm_n, t->dn_tmp, t->dn_out, t->tm_var, nullptr, t->stream, t->sv_ev[1]));
  HIP_TRY(hipEventRecord(t->sv_ev[2], t->stream));
  t->dn_valid = true; t->tm_dn_valid = true; t->tm_var_valid = true; t->sv_timed = true;
  return out ? read_back(t, out, t->dn_out, px * 16, "fspt_temporal_denoise_variance") : FSPT_OK;
}

int fspt_temporal_read_variance(fspt_target *t, float *var_out, float *mom_out) {
  int rc = dn_enter(t, var_out || mom_out, "fspt_temporal_read_variance");
  if (rc) return rc;
  if (!t->tm_moments || !t->tm_valid || !t->tm_mom_valid) { fspt_set_error("fspt_temporal_read_variance: no fspt_temporal_accumulate call with moments on yet"); return FSPT_E_STATE; }
  if (var_out && !t->tm_var_valid) { fspt_set_error("fspt_temporal_read_variance: no fspt_temporal_denoise_variance call since the last fspt_temporal_accumulate"); return FSPT_E_STATE; }
  const size_t px = (size_t)t->W * t->H;
  if (var_out) HIP_TRY(hipMemcpyAsync(var_out, t->tm_var, px * 4, hipMemcpyDeviceToHost, t->stream));
  if (mom_out) HIP_TRY(hipMemcpyAsync(mom_out, t->tm_mom[t->tm_cur], px * 8, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

int fspt_svgf_last_ms(fspt_target *t, float ms[2]) {
  return last_ms(t, ms, 2, t ? t->sv_ev : nullptr, t && t->sv_timed, "fspt_svgf_last_ms", "fspt_temporal_denoise_variance call");
}

int fspt_svgf_eval(int device, const float *hist, const float *moments, const float *features, uint32_t W, uint32_t H, uint32_t n,
                   const fspt_denoise_params *prm, float *out, float *var_in, float *var_out) {
  if (!hist || !moments || !features || !out) { fspt_set_error("fspt_svgf_eval: NULL argument"); return FSPT_E_INVALID; }
  fspt_denoise_params q;
  int rc = dn_params(prm, SV_DEFAULTS, "fspt_svgf_eval", q);
  if (rc) return rc;
  if (n == 0) { fspt_set_error("fspt_svgf_eval: n must be >= 1"); return FSPT_E_INVALID; }
  if ((rc = check_device(device))) return rc;
  const size_t px = (size_t)W * H;
  if (px == 0) return FSPT_OK;
  HIP_TRY(hipSetDevice(device));
  // one allocation, in float4: hist | out | tmp[0] | tmp[1] (px each) | features (2 px) | moments (px / 2) | var, var' (px / 4 each)
  Staging s(px * 16 * 7 + 64);
  if (!s.ok()) return s.done("fspt_svgf_eval");
  float4 *const d = (float4 *)s.base;
  float4 *const tmp[2] = {d + 2 * px, d + 3 * px};
  float2 *const mom = (float2 *)(d + 6 * px);
  float *const var = (float *)(mom + px), *const var2 = var + px;
  s.up(d, hist, px * 16);
  s.up(d + 4 * px, features, px * 32);
  s.up(mom, moments, px * 8);
  if (s.ok()) s.e = sv_run(q, d, mom, d + 4 * px, W, H, (float)n, tmp, d + px, var, var2, nullptr, nullptr);
  s.sync();
  s.down(out, d + px, px * 16);
  s.down(var_in, var, px * 4);
  s.down(var_out, var2, px * 4);
  return s.done("fspt_svgf_eval");
}

// ---------------------------------------------------------------------------
// temporal history clamp (k_temporal_blend<*, true> / k_temporal_clamp)
// ---------------------------------------------------------------------------
static int cl_check_params(float fast_history, float sigma_scale, const char *fn) {
  if (!(fast_history >= 1.0f && fast_history < INFINITY) || !(sigma_scale >= 0.0f)) {
    fspt_set_error("%s: need a finite fast_history >= 1 and sigma_scale >= 0 (+inf: the clamp never binds)", fn);
    return FSPT_E_INVALID;
  }
  return FSPT_OK;
}

static void cl_free(fspt_target *t) {
  hipFree(t->tm_fast[0]); hipFree(t->tm_fast[1]);
  t->tm_fast[0] = t->tm_fast[1] = nullptr;
  t->tm_clamp = t->tm_fast_valid = t->cl_timed = false;
}

int fspt_temporal_set_clamp(fspt_target *t, int on, float fast_history, float sigma_scale) {
  if (!t) { fspt_set_error("fspt_temporal_set_clamp: NULL argument"); return FSPT_E_INVALID; }
  int rc;
  if (on && (rc = cl_check_params(fast_history, sigma_scale, "fspt_temporal_set_clamp"))) return rc;
  if ((rc = dn_enter(t, true, "fspt_temporal_set_clamp"))) return rc;
  if (!on) return mode_off(t, cl_free, "fspt_temporal_set_clamp");
  if (t->n_shards > 1) { fspt_set_error("fspt_temporal_set_clamp: sharded target"); return FSPT_E_STATE; }
  t->tm_fast_history = fast_history; t->tm_sigma_scale = sigma_scale; // (a change of the parameters alone keeps both histories)
  if (t->tm_clamp) return FSPT_OK;
  const size_t px = (size_t)t->W * t->H;
  for (int k = 0; k < 2; ++k) {
    if ((rc = dn_alloc(&t->tm_fast[k], px * 16))) return rc;
  }
  t->tm_clamp = true;
  // off -> on drops the long history with it, as fspt_temporal_set_moments does: the two histories start together
  tm_drop_history(t);
  return FSPT_OK;
}

int fspt_temporal_read_fast(fspt_target *t, float *out) {
  int rc = dn_enter(t, out != nullptr, "fspt_temporal_read_fast");
  if (rc) return rc;
  if (!t->tm_clamp || !t->tm_valid || !t->tm_fast_valid) { fspt_set_error("fspt_temporal_read_fast: no fspt_temporal_accumulate call with the clamp on yet"); return FSPT_E_STATE; }
  return read_back(t, out, t->tm_fast[t->tm_cur], (size_t)t->W * t->H * 16, "fspt_temporal_read_fast");
}

int fspt_temporal_clamp_last_ms(fspt_target *t, float *ms) {
  return last_ms(t, ms, 1, t ? t->cl_ev : nullptr, t && t->cl_timed, "fspt_temporal_clamp_last_ms", "fspt_temporal_accumulate call with the clamp on");
}

int fspt_temporal_clamp_eval(int device, const float *hist, const float *fast, uint32_t W, uint32_t H, float sigma_scale,
                             float *out, float *lo_out, float *hi_out) {
  if (!hist || !fast || !out) { fspt_set_error("fspt_temporal_clamp_eval: NULL argument"); return FSPT_E_INVALID; }
  int rc = cl_check_params(1.0f, sigma_scale, "fspt_temporal_clamp_eval");
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  const size_t px = (size_t)W * H;
  if (px == 0) return FSPT_OK;
  if (sigma_scale == INFINITY) { // the clamp never binds: no launch, the box is everything
    std::memcpy(out, hist, px * 16);
    for (size_t i = 0; i < px * 4; ++i) {
      if (lo_out) lo_out[i] = (i & 3) == 3 ? 0.0f : -INFINITY;
      if (hi_out) hi_out[i] = (i & 3) == 3 ? 0.0f : INFINITY;
    }
    return FSPT_OK;
  }
  HIP_TRY(hipSetDevice(device));
  // one allocation, in float4: hist | fast | out | lo | hi (px each)
  Staging s(px * 16 * 5);
  if (!s.ok()) return s.done("fspt_temporal_clamp_eval");
  float4 *const d = (float4 *)s.base;
  s.up(d, hist, px * 16);
  s.up(d + px, fast, px * 16);
  if (s.ok()) {
    fspt::ClampP c{};
    c.hist = d; c.fast = d + px; c.out = d + 2 * px; c.lo = d + 3 * px; c.hi = d + 4 * px;
    c.W = W; c.H = H; c.sigma_scale = sigma_scale;
    s.e = fspt::launch_temporal_clamp(c, nullptr);
  }
  s.sync();
  s.down(out, d + 2 * px, px * 16);
  s.down(lo_out, d + 3 * px, px * 16);
  s.down(hi_out, d + 4 * px, px * 16);
  return s.done("fspt_temporal_clamp_eval");
}

// ---------------------------------------------------------------------------
// auto-exposure (k_exposure_histogram / k_exposure_resolve / k_draw_auto)
// ---------------------------------------------------------------------------
static int ax_check_params(const fspt_exposure_params *p, fspt::ExposureP &q, const char *fn) {
  static const fspt_exposure_params dflt = {FSPT_EXPOSURE_KEY, FSPT_EXPOSURE_LOW, FSPT_EXPOSURE_HIGH, FSPT_EXPOSURE_ADAPT_UP, FSPT_EXPOSURE_ADAPT_DOWN,
                                            FSPT_EXPOSURE_MIN_LOG2, FSPT_EXPOSURE_MAX_LOG2};
  if (!p) p = &dflt;
  const float f[7] = {p->key, p->low, p->high, p->adapt_up, p->adapt_down, p->min_log2, p->max_log2};
  bool ok = true;
  for (float v : f) ok = ok && std::isfinite(v);
  ok = ok && p->key > 0.0f && p->low >= 0.0f && p->low < p->high && p->high <= 1.0f && p->adapt_up > 0.0f && p->adapt_up <= 1.0f &&
       p->adapt_down > 0.0f && p->adapt_down <= 1.0f && p->min_log2 <= p->max_log2;
  if (!ok) {
    fspt_set_error("%s: need finite parameters with key > 0, 0 <= low < high <= 1, adapt_up and adapt_down in (0, 1], min_log2 <= max_log2", fn);
    return FSPT_E_INVALID;
  }
  q = fspt::ExposureP{p->key, p->low, p->high, p->adapt_up, p->adapt_down, p->min_log2, p->max_log2};
  return FSPT_OK;
}
static const fspt::ExposureState AX_FIRST = {1.0f, 0u, 0u, 0u, 0.0, 0.0}; // never metered: exposure 1, nothing to adapt from
static_assert(sizeof(fspt::ExposureState) == sizeof(fspt_exposure_state) && sizeof(fspt_exposure_state) == 32, "fspt_exposure_state is the device's record");

int fspt_exposure_set_form(int form) {
  if (form != 0 && form != 1) { fspt_set_error("fspt_exposure_set_form: form must be 0 or 1"); return FSPT_E_INVALID; }
  fspt::g_exposure_form = form;
  return FSPT_OK;
}

static void ax_free(fspt_target *t) {
  hipFree(t->ax_hist);
  t->ax_hist = nullptr; t->ax_state = nullptr;
  t->ax_on = t->ax_timed = false;
}

int fspt_target_set_auto_exposure(fspt_target *t, int on, const fspt_exposure_params *p) {
  if (!t) { fspt_set_error("fspt_target_set_auto_exposure: NULL argument"); return FSPT_E_INVALID; }
  fspt::ExposureP q{};
  int rc;
  if (on && (rc = ax_check_params(p, q, "fspt_target_set_auto_exposure"))) return rc;
  if ((rc = dn_enter(t, true, "fspt_target_set_auto_exposure"))) return rc;
  if (!on) return mode_off(t, ax_free, "fspt_target_set_auto_exposure");
  if (t->n_shards > 1) { fspt_set_error("fspt_target_set_auto_exposure: sharded target"); return FSPT_E_STATE; }
  t->ax_p = q; // (a change of the parameters alone keeps the adapted state)
  if (t->ax_on) return FSPT_OK;
  const size_t hist_bytes = fspt::EXPOSURE_BINS * sizeof(uint32_t);
  if (!t->ax_hist) HIP_TRY(hipMalloc((void **)&t->ax_hist, hist_bytes + sizeof(fspt::ExposureState)));
  t->ax_state = (fspt::ExposureState *)(t->ax_hist + fspt::EXPOSURE_BINS);
  HIP_TRY(hipMemsetAsync(t->ax_hist, 0, hist_bytes, t->stream));
  HIP_TRY(hipMemcpyAsync(t->ax_state, &AX_FIRST, sizeof AX_FIRST, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  for (hipEvent_t &ev : t->ax_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  t->ax_on = true; t->ax_timed = false;
  return FSPT_OK;
}

int fspt_exposure_reset(fspt_target *t) {
  int rc = dn_enter(t, true, "fspt_exposure_reset");
  if (rc) return rc;
  if (!t->ax_on) { fspt_set_error("fspt_exposure_reset: auto-exposure is off"); return FSPT_E_STATE; }
  HIP_TRY(hipMemcpyAsync(t->ax_state, &AX_FIRST, sizeof AX_FIRST, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

int fspt_exposure_get(fspt_target *t, float *exposure, float *log2_mean, uint32_t *metered) {
  int rc = dn_enter(t, exposure || log2_mean || metered, "fspt_exposure_get");
  if (rc) return rc;
  if (!t->ax_on) { fspt_set_error("fspt_exposure_get: auto-exposure is off"); return FSPT_E_STATE; }
  fspt::ExposureState s;
  if ((rc = read_back(t, &s, t->ax_state, sizeof s, "fspt_exposure_get"))) return rc;
  if (exposure) *exposure = s.exposure;
  if (log2_mean) *log2_mean = (float)s.log2_mean;
  if (metered) *metered = s.metered;
  return FSPT_OK;
}

int fspt_exposure_last_ms(fspt_target *t, float ms[2]) {
  return last_ms(t, ms, 2, t ? t->ax_ev : nullptr, t && t->ax_timed, "fspt_exposure_last_ms", "draw with auto-exposure on");
}

int fspt_exposure_last_draw_ms(fspt_target *t, float *ms) {
  return last_ms(t, ms, 1, t ? t->ax_ev + 2 : nullptr, t && t->ax_timed, "fspt_exposure_last_draw_ms", "draw with auto-exposure on");
}

int fspt_exposure_eval(int device, const float *rgba, uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const fspt_exposure_params *p,
                       const fspt_exposure_state *prev, uint32_t *hist_out, fspt_exposure_state *state_out) {
  if (!rgba || !hist_out || !state_out) { fspt_set_error("fspt_exposure_eval: NULL argument"); return FSPT_E_INVALID; }
  fspt::ExposureP q{};
  int rc = ax_check_params(p, q, "fspt_exposure_eval");
  if (rc) return rc;
  if (vw == 0 && vh == 0) { vw = W; vh = H; } // (as fspt_target_set_viewport: 0, 0 = the whole image)
  if (W == 0 || H == 0 || vw == 0 || vh == 0 || vw > W || vh > H || (uint64_t)W * H > 0xFFFFFFFFull) {
    fspt_set_error("fspt_exposure_eval: need 1 <= vw <= W, 1 <= vh <= H and fewer than 2^32 pixels"); return FSPT_E_INVALID;
  }
  if ((rc = check_device(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t px = (size_t)W * H, hist_bytes = fspt::EXPOSURE_BINS * sizeof(uint32_t);
  // one allocation: image | histogram | state
  Staging s(px * 16 + hist_bytes + sizeof(fspt::ExposureState));
  if (!s.ok()) return s.done("fspt_exposure_eval");
  char *const d = s.base;
  uint32_t *hist = (uint32_t *)(d + px * 16);
  fspt::ExposureState *state = (fspt::ExposureState *)(d + px * 16 + hist_bytes);
  s.up(d, rgba, px * 16);
  if (s.ok()) s.e = hipMemset(hist, 0, hist_bytes);
  s.up(state, prev ? (const void *)prev : (const void *)&AX_FIRST, sizeof(fspt::ExposureState));
  if (s.ok()) s.e = fspt::launch_exposure_histogram((const float4 *)d, W, vw, vh, hist, fspt::g_exposure_form, nullptr);
  s.down(hist_out, hist, hist_bytes);
  if (s.ok()) s.e = fspt::launch_exposure_resolve(hist, state, q, nullptr);
  s.sync();
  s.down(state_out, state, sizeof(fspt::ExposureState));
  // reserved = the counts the resolve left behind, summed: 0 (it clears the histogram for the next metering)
  uint32_t left[fspt::EXPOSURE_BINS];
  s.down(left, hist, hist_bytes);
  if (s.ok()) { uint32_t any = 0; for (uint32_t c : left) any |= c; state_out->reserved = any; }
  return s.done("fspt_exposure_eval");
}

// ---------------------------------------------------------------------------
// bloom (k_bloom_down / k_bloom_up / k_bloom_tail / k_draw_bloom)
// ---------------------------------------------------------------------------
static int bl_check_params(const fspt_bloom_params *p, fspt::BloomP &q, const char *fn) {
  static const fspt_bloom_params dflt = {FSPT_BLOOM_INTENSITY, FSPT_BLOOM_SCATTER, FSPT_BLOOM_LEVELS};
  if (!p) p = &dflt;
  if (!(std::isfinite(p->intensity) && std::isfinite(p->scatter) && p->intensity >= 0.0f && p->intensity <= 1.0f && p->scatter >= 0.0f &&
        p->scatter <= 1.0f && p->levels >= 1u && p->levels <= (uint32_t)FSPT_BLOOM_MAX_LEVELS)) {
    fspt_set_error("%s: need finite intensity and scatter in [0, 1] and levels in [1, %d]", fn, FSPT_BLOOM_MAX_LEVELS);
    return FSPT_E_INVALID;
  }
  q = fspt::BloomP{p->intensity, p->scatter, p->levels};
  return FSPT_OK;
}
static_assert(FSPT_BLOOM_MAX_LEVELS == fspt::BLOOM_MAX_LEVELS && FSPT_BLOOM_TAIL_TEXELS == fspt::BLOOM_TAIL_TEXELS, "fspt_tuning.h names the device's constants");

int fspt_bloom_set_form(int form) {
  if (form != 0 && form != 1) { fspt_set_error("fspt_bloom_set_form: form must be 0 or 1"); return FSPT_E_INVALID; }
  fspt::g_bloom_form = form;
  return FSPT_OK;
}

int fspt_bloom_set_tail_texels(uint32_t n) {
  fspt::g_bloom_tail_texels = n ? n : fspt::BLOOM_TAIL_TEXELS;
  return FSPT_OK;
}

uint64_t fspt_bloom_texels(uint32_t vw, uint32_t vh, uint32_t levels, uint32_t *n_out) {
  if (vw == 0 || vh == 0) { if (n_out) *n_out = 0; return 0; }
  const fspt::BloomPlan q = fspt::bloom_plan(vw, vh, levels, 0, 0);
  if (n_out) *n_out = q.n;
  return q.texels;
}

static void bl_free(fspt_target *t) {
  hipFree(t->bl_pyr);
  t->bl_pyr = nullptr;
  t->bl_on = t->bl_timed = false;
}

int fspt_target_set_bloom(fspt_target *t, int on, const fspt_bloom_params *p) {
  if (!t) { fspt_set_error("fspt_target_set_bloom: NULL argument"); return FSPT_E_INVALID; }
  fspt::BloomP q{};
  int rc;
  if (on && (rc = bl_check_params(p, q, "fspt_target_set_bloom"))) return rc;
  if ((rc = dn_enter(t, true, "fspt_target_set_bloom"))) return rc;
  if (!on) return mode_off(t, bl_free, "fspt_target_set_bloom");
  if (t->n_shards > 1) { fspt_set_error("fspt_target_set_bloom: sharded target"); return FSPT_E_STATE; }
  t->bl_p = q; // (a change of the parameters alone keeps the allocation: it is sized for W x H at the most levels)
  if (t->bl_on) return FSPT_OK;
  const size_t texels = fspt::bloom_plan(t->W, t->H, fspt::BLOOM_MAX_LEVELS, 0, 0).texels;
  if (!t->bl_pyr) HIP_TRY(hipMalloc((void **)&t->bl_pyr, (texels ? texels : 1) * sizeof(float4)));
  for (hipEvent_t &ev : t->bl_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
  t->bl_on = true; t->bl_timed = false;
  return FSPT_OK;
}

int fspt_target_get_bloom(fspt_target *t, int *on, fspt_bloom_params *p) {
  if (!t || !on || !p) { fspt_set_error("fspt_target_get_bloom: NULL argument"); return FSPT_E_INVALID; }
  *on = t->bl_on ? 1 : 0;
  if (t->bl_on) *p = fspt_bloom_params{t->bl_p.intensity, t->bl_p.scatter, t->bl_p.levels};
  else *p = fspt_bloom_params{FSPT_BLOOM_INTENSITY, FSPT_BLOOM_SCATTER, FSPT_BLOOM_LEVELS};
  return FSPT_OK;
}

int fspt_bloom_last_ms(fspt_target *t, float ms[4]) {
  return last_ms(t, ms, 4, t ? t->bl_ev : nullptr, t && t->bl_on && t->bl_timed, "fspt_bloom_last_ms", "bloomed draw");
}

int fspt_bloom_eval(int device, const float *rgba, uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const fspt_bloom_params *p, uint32_t *n_out,
                    float *down_out, float *up_out, float *bloom_out, float *mix_out) {
  if (!rgba) { fspt_set_error("fspt_bloom_eval: NULL argument"); return FSPT_E_INVALID; }
  fspt::BloomP bp{};
  int rc = bl_check_params(p, bp, "fspt_bloom_eval");
  if (rc) return rc;
  if (vw == 0 && vh == 0) { vw = W; vh = H; } // (as fspt_target_set_viewport: 0, 0 = the whole image)
  if (W == 0 || H == 0 || vw == 0 || vh == 0 || vw > W || vh > H || (uint64_t)W * H > 0x7FFFFFFFull) {
    fspt_set_error("fspt_bloom_eval: need 1 <= vw <= W, 1 <= vh <= H and fewer than 2^31 pixels"); return FSPT_E_INVALID;
  }
  if ((rc = check_device(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const fspt::BloomPlan q = fspt::bloom_plan(vw, vh, bp.levels, fspt::g_bloom_form, fspt::g_bloom_tail_texels);
  if (n_out) *n_out = q.n;
  const size_t px = (size_t)W * H, vpx = (size_t)vw * vh;
  if (q.n == 0) { // the plain draw: nothing is built, the draw multiplies the source by the exposure
    if (mix_out) memcpy(mix_out, rgba, px * 16);
    if (bloom_out) for (uint32_t y = 0; y < vh; ++y) memcpy(bloom_out + (size_t)y * vw * 4, rgba + (size_t)y * W * 4, (size_t)vw * 16);
    return FSPT_OK;
  }
  // one allocation: image | pyramid (U in the end) | the D levels as the down chain left them | B | c'
  Staging s((px + 2 * q.texels + vpx + px) * sizeof(float4));
  if (!s.ok()) return s.done("fspt_bloom_eval");
  float4 *const d = (float4 *)s.base;
  float4 *pyr = d + px, *snap = pyr + q.texels, *B = snap + q.texels, *mix = B + vpx;
  s.up(d, rgba, px * 16);
  if (s.ok()) s.e = fspt::launch_bloom_chain(d, W, q, bp.scatter, pyr, nullptr, snap, pyr, nullptr);
  const fspt::BloomDraw bl{pyr + q.off[1], q.w[1], q.h[1], vw, vh, bp.intensity};
  if (s.ok()) s.e = fspt::launch_bloom_mix(d, W, H, bl, B, mix, nullptr);
  s.sync();
  s.down(down_out, snap, q.texels * 16);
  s.down(up_out, pyr, q.texels * 16);
  s.down(bloom_out, B, vpx * 16);
  s.down(mix_out, mix, px * 16);
  return s.done("fspt_bloom_eval");
}

// ---------------------------------------------------------------------------
// Encoded output: JPEG (fspt_jpeg.hip), PNG (8.20; fspt_png.hip), OpenEXR (8.21; fspt_exr.hip)
// ---------------------------------------------------------------------------
// fspt_draw_jpeg's and fspt_draw_png's frame: that of the entry the source stands for, refused as that entry refuses it
static int encoded_source(fspt_target *t, int source, const float4 *&src, int &denoise, float &max_sigma, float &scale) {
  src = t->accum;
  if (source == FSPT_SOURCE_DENOISED) {
    if (!t->dn_valid) { fspt_set_error("fspt_draw_denoised: no fspt_denoise call yet"); return FSPT_E_STATE; }
    src = t->dn_out;
  } else if (source != FSPT_SOURCE_ACCUMULATOR) {
    if (!t->tm_valid) { fspt_set_error("fspt_temporal_draw: no fspt_temporal_accumulate call yet"); return FSPT_E_STATE; }
    if (source == FSPT_SOURCE_TEMPORAL_DENOISED && !t->tm_dn_valid) { fspt_set_error("fspt_temporal_draw: no fspt_temporal_denoise call since the last fspt_temporal_accumulate / fspt_denoise"); return FSPT_E_STATE; }
    src = source == FSPT_SOURCE_TEMPORAL_DENOISED ? t->dn_out : t->tm_hist[t->tm_cur];
  }
  if (source != FSPT_SOURCE_ACCUMULATOR) { denoise = 0; max_sigma = 0.0f; scale = 1.0f; }
  return FSPT_OK;
}

} // extern "C"

// what every fspt_draw_<format> starts with
static int encoded_args(const fspt_target *t, int source, const uint8_t *out, const size_t *bytes_out, const char *fn) {
  if (!t || !out || !bytes_out) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  if (source < FSPT_SOURCE_ACCUMULATOR || source > FSPT_SOURCE_TEMPORAL_DENOISED) { fspt_set_error("%s: unknown source %d", fn, source); return FSPT_E_INVALID; }
  return FSPT_OK;
}

// fspt_draw_jpeg and fspt_draw_png up to the collect: the refusals in their order - arguments, `check` (the parameters alone),
// the scale, the pipeline, `plan`, the source's state - then `ensure`, the frame drawn into t->enc_frame, `launch` on t->stream
template <class Check, class Plan, class Ensure, class Launch>
static int draw_encoded(fspt_target *t, const char *fn, int source, float exposure, float saturation, int denoise, float max_sigma, float scale,
                        const uint8_t *out, const size_t *bytes_out, Check check, Plan plan, Ensure ensure, Launch launch) {
  int rc = encoded_args(t, source, out, bytes_out, fn);
  if (rc || (rc = check())) return rc;
  if (source == FSPT_SOURCE_ACCUMULATOR && !(scale > 0.0f && scale <= 1.0f)) { fspt_set_error("%s: scale must be in (0, 1]", fn); return FSPT_E_INVALID; }
  if ((rc = dn_enter(t, true, fn))) return rc; // (joins a present: nothing of the encoders is in use behind it)
  if ((rc = plan())) return rc;
  const float4 *src = nullptr;
  if ((rc = encoded_source(t, source, src, denoise, max_sigma, scale))) return rc;
  if (!t->enc_frame) HIP_TRY(hipMalloc((void **)&t->enc_frame, (size_t)t->W * t->H * 4));
  hipError_t e = ensure();
  if (e == hipSuccess) e = draw_launch(t, src, exposure, saturation, denoise, max_sigma, scale, t->enc_frame, t->stream);
  if (e == hipSuccess) e = launch();
  return e == hipSuccess ? FSPT_OK : hip_fail(fn, e);
}

extern "C" {

int fspt_draw_jpeg(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale,
                   const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  const char *fn = "fspt_draw_jpeg";
  fspt::JpegPlan pl;
  const int rc = draw_encoded(t, fn, source, exposure, saturation, denoise, max_sigma, scale, out, bytes_out,
                              [&] { return fspt::jpeg_check_params(p, fn); }, [&] { return fspt::jpeg_plan(p, t->W, t->H, fn, pl); },
                              [&] { return fspt::jpeg_ensure(t->jp, pl, 1, fspt::jpeg_bound_max(t->W, t->H)); },
                              [&] { return fspt::jpeg_launch(t->jp, t->enc_frame, 1, 0, t->stream); });
  return rc ? rc : fspt::jpeg_collect(t->jp, 0, t->stream, out, cap, bytes_out, fn);
}

int fspt_draw_png(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale,
                  const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  const char *fn = "fspt_draw_png";
  fspt::PngPlan pl;
  const int rc = draw_encoded(t, fn, source, exposure, saturation, denoise, max_sigma, scale, out, bytes_out,
                              [&] { return fspt::png_check_params(p, fn); }, [&] { return fspt::png_plan(p, t->W, t->H, true, fn, pl); },
                              [&] { // the output buffer: the bound of RGBA at the smallest chunk size asked for so far; it grows, and outlives a change of the parameters
                                t->pg_cb = t->pg_cb ? std::min(t->pg_cb, pl.cb) : pl.cb;
                                return fspt::png_ensure(t->pg, pl, 1, fspt::png_bound_max(t->W, t->H, t->pg_cb));
                              },
                              [&] { return fspt::png_launch(t->pg, t->enc_frame, 1, t->stream); });
  return rc ? rc : fspt::png_collect(t->pg, t->stream, out, cap, bytes_out, fn);
}

// OpenEXR: the HDR buffer itself, no draw in front of it; the plan before the pipeline, the features' state last
int fspt_draw_exr(fspt_target *t, int source, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  const char *fn = "fspt_draw_exr";
  int rc = encoded_args(t, source, out, bytes_out, fn);
  if (rc) return rc;
  fspt::ExrPlan pl;
  fspt::ExrMattes mt{}; // the target's matte buffers and the scene's manifests
  for (int k = 0; k < 2; ++k) { mt.ranks[k] = t->mt[k]; mt.manifest[k] = t->scene->matte_manifest[k].data(); mt.manifest_len[k] = t->scene->matte_manifest[k].size(); }
  if ((rc = fspt::exr_plan(p, t->W, t->H, true, fn, pl, true, &mt))) return rc;
  if ((rc = dn_enter(t, true, fn))) return rc; // (joins a present)
  const float4 *src = nullptr;
  int denoise = 0; float max_sigma = 0.0f, scale = 1.0f;
  if ((rc = encoded_source(t, source, src, denoise, max_sigma, scale))) return rc;
  const bool guided = (pl.layers & ((uint32_t)FSPT_EXR_ALBEDO | (uint32_t)FSPT_EXR_NORMAL | (uint32_t)FSPT_EXR_DEPTH)) != 0u;
  if (guided && !t->feat_valid) { fspt_set_error("%s: feature layers and no fspt_features call yet", fn); return FSPT_E_STATE; }
  for (int k = 0; k < 2; ++k)
    if ((pl.layers & ((uint32_t)FSPT_EXR_CRYPTO_OBJECT << k)) && !t->mt_valid[k]) { fspt_set_error("%s: a matte layer and no fspt_mattes call yet that computed kind %d", fn, k); return FSPT_E_STATE; }
  // the output buffer: the largest bound asked for so far; it grows, and outlives a change of the parameters
  t->ex_bound = std::max(t->ex_bound, pl.bound);
  hipError_t e = fspt::exr_ensure(t->ex, pl, t->ex_bound);
  if (e == hipSuccess) e = fspt::exr_launch(t->ex, src, guided ? t->feat : nullptr, 1, t->stream, &mt);
  if (e != hipSuccess) return hip_fail(fn, e);
  return fspt::exr_collect(t->ex, t->stream, out, cap, bytes_out, fn);
}

} // extern "C"

// fspt_target_destroy's share of the image chain (both streams are idle): every buffer and event above
void post_release(fspt_target *t) {
  hipFree(t->mt[0]); hipFree(t->mt[1]); hipFree(t->mt_lost);
  hipFree(t->feat); hipFree(t->dn_tmp[0]); hipFree(t->dn_tmp[1]); hipFree(t->dn_out);
  hipFree(t->tm_hist[0]); hipFree(t->tm_hist[1]); hipFree(t->tm_g[0]); hipFree(t->tm_g[1]); hipFree(t->tm_m);
  sv_free(t); cl_free(t); ax_free(t); bl_free(t);
  fspt::enc_release(t->jp.c); fspt::enc_release(t->pg.c); fspt::enc_release(t->ex.c); hipFree(t->enc_frame);
  for (uint32_t *c : t->jp_count) if (c) hipHostFree(c);
  if (t->jp_copy) hipStreamDestroy(t->jp_copy);
  for (hipEvent_t ev : t->tm_ev) if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : t->sv_ev) if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : t->cl_ev) if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : t->ax_ev) if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : t->bl_ev) if (ev) hipEventDestroy(ev);
}
