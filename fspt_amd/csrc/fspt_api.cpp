// fspt_api.cpp — host side of the libfspt C ABI (include/fspt.h): the target object and what renders into it.
//
// Mirrors the WebGL2 resource/draw-call layer of the reference's main.js: render targets
// (initBuffers 598-617), drawCamera (741-756), drawTracer (758-807), clear
// (826-836) and the tick loop (838-857); the scene upload is fspt_scene.cpp.  No CPU fallback: every device entry
// point fails with FSPT_E_NO_DEVICE when there is no HIP device.
#include "fspt_internal.hpp"

static thread_local char g_err[512] = "";

void fspt_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    fspt_set_error("no HIP device available (%s); libfspt has no CPU fallback",
                   e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return FSPT_E_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    fspt_set_error("device %d out of range (have %d)", device, n);
    return FSPT_E_INVALID;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    fspt_set_error("hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return FSPT_E_NO_DEVICE;
  }
  return FSPT_OK;
}

const char *camera_model_name(int model) {
  static const char *const names[] = {"pinhole", "ortho", "fisheye", "equirect", "stereo"};
  return model >= 0 && model <= 4 ? names[model] : "?";
}

extern "C" {

const char *fspt_last_error(void) { return g_err; }
int fspt_abi_version(void) { return FSPT_ABI_VERSION; }

int fspt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fspt_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
  if (!free_bytes || !total_bytes) { fspt_set_error("fspt_device_memory: NULL argument"); return FSPT_E_INVALID; }
  if (fspt_device_count() <= 0) { fspt_set_error("fspt_device_memory: no HIP device"); return FSPT_E_NO_DEVICE; }
  size_t f = 0, t = 0;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemGetInfo(&f, &t));
  *free_bytes = f; *total_bytes = t;
  return FSPT_OK;
}

float fspt_rand_base_next(uint64_t *state) {
  uint64_t x = *state;
  x ^= x >> 12;
  x ^= x << 25;
  x ^= x >> 27;
  *state = x;
  uint64_t r = x * 2685821657736338717ULL;
  return ((float)(r >> 40) * (1.0f / 16777216.0f)) * 10000.0f;
}

// ---------------------------------------------------------------------------
// target
// ---------------------------------------------------------------------------
int fspt_target_create(fspt_scene *scene, uint32_t W, uint32_t H, fspt_target **out) {
  if (!scene || !out || W == 0 || H == 0) { fspt_set_error("fspt_target_create: bad argument"); return FSPT_E_INVALID; }
  if ((uint64_t)W * H > (1ull << 30)) { fspt_set_error("fspt_target_create: %ux%u too large", W, H); return FSPT_E_INVALID; }
  int rc = check_device(scene->device);
  if (rc) return rc;
  fspt_target *t = new fspt_target();
  t->scene = scene;
  t->W = W; t->H = H;
  t->vw = W; t->vh = H;
  size_t px = (size_t)W * H;
  hipError_t e = hipMalloc((void **)&t->accum_own, px * 16);
  if (e == hipSuccess) e = hipMalloc((void **)&t->ray_pos, px * 16);
  if (e == hipSuccess) e = hipMalloc((void **)&t->ray_dir, px * 16);
  if (e == hipSuccess) e = hipMalloc((void **)&t->work_counters, WORK_RING * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&t->counters, 8 * 8); // 6 work counters (fspt_counters) + [6] = traversal steps the trace kernel served from LDS
  if (e == hipSuccess) e = hipStreamCreate(&t->stream);
  if (e == hipSuccess) e = hipEventCreate(&t->ev0);
  if (e == hipSuccess) e = hipEventCreate(&t->ev1);
  if (e == hipSuccess) e = hipEventCreate(&t->ev_start);
  if (e == hipSuccess) e = hipEventCreate(&t->prim_ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&t->prim_ev[1]);
  {
    fspt_target::WfLane &ln = t->wf;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ln.stream_b, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.resolved, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.ev_run, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.ev_b_last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.ctl_ready, hipEventDisableTiming);
    for (int k = 0; k < fspt::WF_RING; ++k) {
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.ev_logic[k], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.ev_b[k], hipEventDisableTiming);
    }
  }
  if (e == hipSuccess) e = hipMemsetAsync(t->accum_own, 0, px * 16, t->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->counters, 0, 64, t->stream);
  if (e != hipSuccess) {
    fspt_set_error("fspt_target_create: %s", hipGetErrorString(e));
    fspt_target_destroy(t);
    return FSPT_E_HIP;
  }
  t->accum = t->accum_own;
  scene->targets.push_back(t); // (fspt_scene_update_geometry orders itself against every live target)
  *out = t;
  return FSPT_OK;
}

// A lane's path state, pinned copies, events and streams, in this order; what the lane never made is null.  Synchronises
// nothing but the lane's second stream: the callers have waited for the streams its work was on.
static void lane_destroy(fspt_target::WfLane &ln) {
  for (void *m : ln.mem) hipFree(m);
  hipFree(ln.counts); hipFree(ln.heads);
  if (ln.counts_host) hipHostFree(ln.counts_host);
  if (ln.live_host) hipHostFree(ln.live_host);
  if (ln.counts_ready) hipEventDestroy(ln.counts_ready);
  if (ln.resolved) hipEventDestroy(ln.resolved);
  if (ln.stream_b) hipStreamSynchronize(ln.stream_b);
  hipFree(ln.ctl);
  for (int *b : ln.susp) hipFree(b);
  if (ln.ctl_host) hipHostFree(ln.ctl_host);
  for (hipEvent_t ev : {ln.ev_run, ln.ev_b_last, ln.ctl_ready}) if (ev) hipEventDestroy(ev);
  for (int k = 0; k < fspt::WF_RING; ++k) { if (ln.ev_logic[k]) hipEventDestroy(ln.ev_logic[k]); if (ln.ev_b[k]) hipEventDestroy(ln.ev_b[k]); }
  if (ln.stream_b) hipStreamDestroy(ln.stream_b);
  if (ln.stream) hipStreamDestroy(ln.stream);
}

int fspt_target_destroy(fspt_target *t) {
  if (!t) return FSPT_OK;
  hipSetDevice(t->scene->device);
  { auto &v = t->scene->targets; v.erase(std::remove(v.begin(), v.end(), t), v.end()); }
  // Recorded ticks are dropped: nothing can observe the library's own accumulator any more, and a caller-owned one
  // (fspt_target_bind_accumulator) may already have been freed by its owner - destroy never writes to it.  A caller
  // that wants the recorded ticks in its buffer calls fspt_sync (or re-binds, which flushes) first.
  t->pending.clear();
  if (t->pr_lane.stream) hipStreamSynchronize(t->pr_lane.stream); // (fspt_present's second lane; its work comes first)
  if (t->stream) hipStreamSynchronize(t->stream);
  if (t->pr_lane.stream) wf_release_all(t->pr_lane); // (waits for the device: the wf lane below is torn down without that)
  lane_destroy(t->pr_lane);
  for (int k = 0; k < 2; ++k) {
    hipFree(t->pr_dev[k]);
    if (t->pr_host[k]) hipHostFree(t->pr_host[k]);
    if (t->pr_copied[k]) hipEventDestroy(t->pr_copied[k]);
  }
  for (hipEvent_t ev : {t->pr_acc, t->pr_hop}) if (ev) hipEventDestroy(ev);
  hipFree(t->accum_own); hipFree(t->ray_pos); hipFree(t->ray_dir); hipFree(t->work_counters); hipFree(t->counters);
  post_release(t);
  hipFree(t->ad_snap); hipFree(t->ad_list[0]); hipFree(t->ad_list[1]); hipFree(t->ad_count); hipFree(t->ad_err);
  lane_destroy(t->wf);
  if (t->ev_start) hipEventDestroy(t->ev_start);
  for (hipEvent_t ev : t->prim_ev) if (ev) hipEventDestroy(ev);
  for (hipEvent_t e : t->ev_pool) hipEventDestroy(e);
  if (t->ev0) hipEventDestroy(t->ev0);
  if (t->ev1) hipEventDestroy(t->ev1);
  if (t->stream) hipStreamDestroy(t->stream);
  delete t;
  return FSPT_OK;
}

int fspt_target_set_shard(fspt_target *t, uint32_t shard, uint32_t n_shards, uint32_t tile) {
  if (!t) { fspt_set_error("fspt_target_set_shard: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (n_shards == 0 || shard >= n_shards) { fspt_set_error("shard %u of %u invalid", shard, n_shards); return FSPT_E_INVALID; }
  if (tile == 0 || tile % 8 != 0 || tile > 256) { fspt_set_error("tile %u must be a multiple of 8 in [8,256]", tile); return FSPT_E_INVALID; }
  if (t->shard != shard || t->n_shards != n_shards || t->tile != tile) {
    prim_reset(t);
    if (t->stream_fallback) { HIP_TRY(hipSetDevice(t->scene->device)); wf_release(t->wf); t->stream_fallback = false; }
  }
  t->shard = shard; t->n_shards = n_shards; t->tile = tile;
  return FSPT_OK;
}

int fspt_target_bind_accumulator(fspt_target *t, void *device_ptr) {
  if (!t) { fspt_set_error("fspt_target_bind_accumulator: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  t->accum = device_ptr ? (float4 *)device_ptr : t->accum_own;
  return FSPT_OK;
}

int fspt_target_size(fspt_target *t, uint32_t *W, uint32_t *H) {
  if (!t || !W || !H) { fspt_set_error("fspt_target_size: NULL argument"); return FSPT_E_INVALID; }
  *W = t->W; *H = t->H;
  return FSPT_OK;
}

int fspt_target_accumulator(fspt_target *t, void **device_ptr) {
  if (!t || !device_ptr) { fspt_set_error("fspt_target_accumulator: NULL argument"); return FSPT_E_INVALID; }
  *device_ptr = t->accum;
  return FSPT_OK;
}

int fspt_camera(fspt_target *t, const float P[3], const float I[3], float fov_scale, const float lens[2],
                float rand_base) {
  if (!t || !P || !I || !lens) { fspt_set_error("fspt_camera: NULL argument"); return FSPT_E_INVALID; }
  // drawCamera is recorded, not launched: the ticks that use these rays generate them inside the path kernel (the ray
  // textures are only written when somebody looks at them: fspt_read_rays, fspt_trace_test)
  std::memset(&t->last_cam, 0, sizeof(t->last_cam));
  std::memcpy(t->last_cam.P, P, 12); std::memcpy(t->last_cam.I, I, 12);
  t->last_cam.fov_scale = fov_scale; t->last_cam.lens[0] = lens[0]; t->last_cam.lens[1] = lens[1];
  t->last_rb_cam = rand_base;
  t->cam_recorded = true;
  t->rays_injected = false;
  t->rays_valid = true;
  return FSPT_OK;
}

int fspt_set_rays(fspt_target *t, const float *pos, const float *dir) {
  if (!t || !pos || !dir) { fspt_set_error("fspt_set_rays: NULL argument"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  t->cam_recorded = false;
  t->rays_injected = true;
  size_t bytes = (size_t)t->W * t->H * 16;
  HIP_TRY(hipMemcpyAsync(t->ray_pos, pos, bytes, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipMemcpyAsync(t->ray_dir, dir, bytes, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->rays_valid = true;
  return FSPT_OK;
}

int fspt_set_rays_device(fspt_target *t, const float *pos, const float *dir) {
  if (!t || !pos || !dir) { fspt_set_error("fspt_set_rays_device: NULL argument"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  t->cam_recorded = false;
  t->rays_injected = true;
  size_t bytes = (size_t)t->W * t->H * 16;
  HIP_TRY(hipMemcpyAsync(t->ray_pos, pos, bytes, hipMemcpyDeviceToDevice, t->stream));
  HIP_TRY(hipMemcpyAsync(t->ray_dir, dir, bytes, hipMemcpyDeviceToDevice, t->stream));
  t->rays_valid = true;
  return FSPT_OK;
}

int fspt_read_rays(fspt_target *t, float *pos, float *dir) {
  if (!t || !pos || !dir) { fspt_set_error("fspt_read_rays: NULL argument"); return FSPT_E_INVALID; }
  if (!t->rays_valid) { fspt_set_error("fspt_read_rays: no rays generated yet"); return FSPT_E_STATE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  { int rcm = materialise_rays(t); if (rcm) return rcm; }
  size_t bytes = (size_t)t->W * t->H * 16;
  HIP_TRY(hipMemcpyAsync(pos, t->ray_pos, bytes, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipMemcpyAsync(dir, t->ray_dir, bytes, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

} // extern "C"

// Every path ends after MAX_PATH_ITERS loop iterations (the cap on tracer.fs:488's `i--`), and `i` never exceeds the
// iteration count: a larger NUM_BOUNCES cannot change any sample.  Clamping keeps the per-round tables
// (WfCounts[WF_ROUNDS_MAX + 2], the 8-bit bounce field of the path flags) in range for any caller value.
uint32_t clamp_bounces(uint32_t nb) { return nb > (uint32_t)FSPT_MAX_BOUNCES ? (uint32_t)FSPT_MAX_BOUNCES : nb; }

// n_ticks ticks with ray generation in the path kernels and explicit per-tick randBase values, on either pipeline
static int trace_from_buffers(fspt_target *t, uint32_t tick, float rand_base, float env_theta, uint32_t num_bounces, bool inner);
static fspt::CameraP camera_p(const fspt_camera_params &c) {
  fspt::CameraP p;
  std::memcpy(p.P, c.P, 12); std::memcpy(p.I, c.I, 12);
  p.fov_scale = c.fov_scale; p.lens[0] = c.lens[0]; p.lens[1] = c.lens[1];
  return p;
}
// k_camera under a camera model has overwritten the target's one pair of ray buffers with rays nobody asked to see.  What they held
// before: a recorded fspt_camera call not yet materialised (nothing to do), that call's materialised rays (made again when
// somebody looks at them: cam_recorded), or injected rays, which are gone - fspt_trace then answers FSPT_E_STATE rather than
// trace foreign rays, until the caller injects again.
static void ray_buffers_overwritten(fspt_target *t) {
  if (t->cam_recorded) return;
  if (t->rays_valid && !t->rays_injected) t->cam_recorded = true;
  else { t->rays_valid = false; t->rays_injected = false; }
}
// The same under a camera model: per tick the model's k_camera into the ray buffers, then the single-tick trace from
// the buffers (either pipeline, either scheduler), all on the target's stream in order - the trace of tick k has read the
// buffers before the camera kernel of tick k + 1 writes them, and nothing waits on the host.  Not batched.
static int render_ticks_model(fspt_target *t, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks,
                              const float *rbc, const float *rbt) {
  if (t->tile_list) { fspt_set_error("camera model '%s': tile lists are not supported", camera_model_name(t->cam_model.model)); return FSPT_E_STATE; }
  const fspt::CameraP c = camera_p(*cam);
  t->ev_used = 0; t->ev_overflow = false;
  HIP_TRY(hipEventRecord(t->ev0, t->stream));
  ray_buffers_overwritten(t);
  for (uint32_t k = 0; k < n_ticks; ++k) {
    HIP_TRY(fspt::launch_camera(t->W, t->H, t->vw, t->vh, c, t->cam_model, rbc[k], t->ray_pos, t->ray_dir, t->stream,
                                (uint32_t)t->sampler, t->sampler_seed, first_tick + k));
    int rc = trace_from_buffers(t, first_tick + k, rbt[k], cam->env_theta, cam->num_bounces, true);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(t->ev1, t->stream));
  t->timed = true; t->last_launches = n_ticks;
  t->acc_ticks = first_tick + n_ticks;
  return FSPT_OK;
}

static int render_ticks(fspt_target *t, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks,
                        const float *rbc, const float *rbt) {
  if (t->cam_model.model != FSPT_CAMERA_PINHOLE) return render_ticks_model(t, cam, first_tick, n_ticks, rbc, rbt);
  t->ev_used = 0; t->ev_overflow = false;
  if (t->pipeline == 1) {
    HIP_TRY(hipEventRecord(t->ev0, t->stream));
    int rc;
    if (t->sched == 1 || t->stream_fallback) {
      rc = render_stream(t, cam, first_tick, n_ticks, rbc, rbt, false);
    } else {
      rc = render_wavefront(t, cam, first_tick, n_ticks, rbc, rbt, false);
      if (rc == FSPT_E_NOMEM) {
        // fewer than FSPT_MIN_BATCH ticks of path state fit (nothing has been launched yet): the bounded pool instead
        t->stream_fallback = true;
        rc = render_stream(t, cam, first_tick, n_ticks, rbc, rbt, false);
      }
    }
    if (rc) return rc;
    HIP_TRY(hipEventRecord(t->ev1, t->stream));
    t->timed = true; t->last_launches = n_ticks;
    t->acc_ticks = first_tick + n_ticks;
    return FSPT_OK;
  }
  fspt::TraceP p{};
  fill_trace_params(t, p);
  std::memcpy(p.cam.P, cam->P, 12); std::memcpy(p.cam.I, cam->I, 12);
  p.cam.fov_scale = cam->fov_scale; p.cam.lens[0] = cam->lens[0]; p.cam.lens[1] = cam->lens[1];
  p.env_theta = cam->env_theta; p.num_bounces = cam->num_bounces;
  bool first = true;
  uint32_t done = 0;
  while (done < n_ticks) {
    uint32_t batch = n_ticks - done < WORK_RING ? n_ticks - done : WORK_RING;
    HIP_TRY(hipMemsetAsync(t->work_counters, 0, (size_t)batch * 4, t->stream));
    if (first) { HIP_TRY(hipEventRecord(t->ev0, t->stream)); first = false; }
    for (uint32_t k = 0; k < batch; ++k) {
      p.rand_base_cam = rbc[done + k];
      p.rand_base = rbt[done + k];
      p.tick = first_tick + done + k;
      p.work_counter = t->work_counters + k;
      HIP_TRY(fspt::launch_trace(p, true, t->count != 0, t->scene->num_cus, t->stream));
    }
    done += batch;
  }
  HIP_TRY(hipEventRecord(t->ev1, t->stream));
  t->timed = true; t->last_launches = n_ticks;
  t->acc_ticks = first_tick + n_ticks;
  return FSPT_OK;
}

// Execute the recorded two-call ticks: runs of consecutive ticks with the same camera / envTheta / NUM_BOUNCES go
// through the batched path (ray generation in the kernel from the recorded randBase values - the same arithmetic as
// k_camera followed by a trace of the ray buffers, tests/test_parity_gpu.py).  Called by everything that observes or
// changes state the ticks depend on.
static bool same_view(const fspt_camera_params &a, const fspt_camera_params &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
int flush_pending(fspt_target *t) {
  { int rc_j = present_join(t); if (rc_j) return rc_j; }
  if (t->pending.empty()) return FSPT_OK;
  std::vector<fspt_target::Deferred> q;
  q.swap(t->pending); // (a failing batch drops the rest: the error is reported once)
  HIP_TRY(hipSetDevice(t->scene->device));
  std::vector<float> rbc, rbt;
  size_t i = 0;
  while (i < q.size()) {
    size_t j = i + 1;
    while (j < q.size() && same_view(q[j].cam, q[i].cam) && q[j].tick == q[j - 1].tick + 1) ++j;
    rbc.clear(); rbt.clear();
    for (size_t k = i; k < j; ++k) { rbc.push_back(q[k].rb_cam); rbt.push_back(q[k].rb_trace); }
    int rc = render_ticks(t, &q[i].cam, q[i].tick, (uint32_t)(j - i), rbc.data(), rbt.data());
    if (rc) return rc;
    i = j;
  }
  return FSPT_OK;
}

// the ray buffers as the most recent fspt_camera call left them (drawCamera's two render targets)
int materialise_rays(fspt_target *t) {
  if (!t->cam_recorded) return FSPT_OK;
  fspt::CameraP c;
  std::memcpy(c.P, t->last_cam.P, 12); std::memcpy(c.I, t->last_cam.I, 12);
  c.fov_scale = t->last_cam.fov_scale; c.lens[0] = t->last_cam.lens[0]; c.lens[1] = t->last_cam.lens[1];
  // (the Sobol sampler: sample index acc_ticks - the tick that would trace these rays next)
  HIP_TRY(fspt::launch_camera(t->W, t->H, t->vw, t->vh, c, t->cam_model, t->last_rb_cam, t->ray_pos, t->ray_dir, t->stream,
                              (uint32_t)t->sampler, t->sampler_seed, t->acc_ticks));
  t->cam_recorded = false;
  return FSPT_OK;
}

static int present_flush(fspt_target *t); // (fspt_present: the recorded ticks without a join)

extern "C" {

// a tick traced from the ray buffers (fspt_set_rays), on the target's stream
// (inner: one tick of render_ticks_model's loop, which keeps the timing events around the whole run)
static int trace_from_buffers(fspt_target *t, uint32_t tick, float rand_base, float env_theta, uint32_t num_bounces, bool inner) {
  if (t->pipeline == 1) {
    fspt_camera_params cp{};
    cp.env_theta = env_theta; cp.num_bounces = num_bounces;
    if (!inner) {
      t->ev_used = 0; t->ev_overflow = false;
      HIP_TRY(hipEventRecord(t->ev0, t->stream));
    }
    int rc;
    if (t->sched == 1 || t->stream_fallback) {
      rc = render_stream(t, &cp, tick, 1, nullptr, &rand_base, true);
    } else {
      rc = render_wavefront(t, &cp, tick, 1, nullptr, &rand_base, true);
      if (rc == FSPT_E_NOMEM) { // as in render_ticks: the bounded pool when the batch scheduler's path state does not fit
        t->stream_fallback = true;
        rc = render_stream(t, &cp, tick, 1, nullptr, &rand_base, true);
      }
    }
    if (rc) return rc;
    if (!inner) HIP_TRY(hipEventRecord(t->ev1, t->stream));
    t->timed = true; t->last_launches = 1;
    t->acc_ticks = tick + 1;
    return FSPT_OK;
  }
  if (!inner) t->ev_used = 0;
  fspt::TraceP p{};
  fill_trace_params(t, p);
  p.tick = tick; p.rand_base = rand_base; p.rand_base_cam = 0.0f; p.env_theta = env_theta; p.num_bounces = num_bounces;
  HIP_TRY(hipMemsetAsync(t->work_counters, 0, 4, t->stream));
  p.work_counter = t->work_counters;
  if (!inner) HIP_TRY(hipEventRecord(t->ev0, t->stream));
  HIP_TRY(fspt::launch_trace(p, false, t->count != 0, t->scene->num_cus, t->stream));
  if (!inner) HIP_TRY(hipEventRecord(t->ev1, t->stream));
  t->timed = true; t->last_launches = 1;
  t->acc_ticks = tick + 1;
  return FSPT_OK;
}

int fspt_trace(fspt_target *t, uint32_t tick, float rand_base, float env_theta, uint32_t num_bounces) {
  if (!t) { fspt_set_error("fspt_trace: NULL target"); return FSPT_E_INVALID; }
  if (!t->rays_valid) { fspt_set_error("fspt_trace: call fspt_camera or fspt_set_rays first"); return FSPT_E_STATE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  num_bounces = clamp_bounces(num_bounces);
  if (!t->rays_injected) {
    // rays come from fspt_camera: record the tick; it runs with its neighbours in one batch at the next flush point
    fspt_target::Deferred d;
    d.cam = t->last_cam; d.cam.env_theta = env_theta; d.cam.num_bounces = num_bounces;
    d.rb_cam = t->last_rb_cam; d.tick = tick; d.rb_trace = rand_base;
    t->pending.push_back(d);
    // (running recorded ticks is not a join: under present they go the present way, and the frame in flight stays)
    if (!t->defer || t->pending.size() >= (size_t)t->batch_ticks) return t->pr_active ? present_flush(t) : flush_pending(t);
    return FSPT_OK;
  }
  if (t->pr_active) {
    // a tick is not a join: the recorded ticks go the present way, this one behind the last accumulator access
    int rc = present_flush(t);
    if (rc) return rc;
    if (t->pr_acc_stream && t->pr_acc_stream != t->stream) HIP_TRY(hipStreamWaitEvent(t->stream, t->pr_acc, 0));
    if ((rc = trace_from_buffers(t, tick, rand_base, env_theta, num_bounces, false))) return rc;
    HIP_TRY(hipEventRecord(t->pr_acc, t->stream));
    t->pr_acc_stream = t->stream;
    return FSPT_OK;
  }
  FLUSH_OR_RETURN(t);
  return trace_from_buffers(t, tick, rand_base, env_theta, num_bounces, false);
}

int fspt_trace_test(fspt_target *t, uint32_t tick) {
  if (!t) { fspt_set_error("fspt_trace_test: NULL target"); return FSPT_E_INVALID; }
  if (!t->rays_valid) { fspt_set_error("fspt_trace_test: call fspt_camera or fspt_set_rays first"); return FSPT_E_STATE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  int rcm = materialise_rays(t);
  if (rcm) return rcm;
  fspt::TraceP p{};
  fill_trace_params(t, p);
  p.tick = tick;
  t->ev_used = 0;
  HIP_TRY(hipEventRecord(t->ev0, t->stream));
  HIP_TRY(fspt::launch_bvh_test(p, t->stream));
  HIP_TRY(hipEventRecord(t->ev1, t->stream));
  t->timed = true; t->last_launches = 1;
  t->acc_ticks = tick + 1;
  return FSPT_OK;
}

int fspt_render(fspt_target *t, const fspt_camera_params *cam_in, uint32_t first_tick, uint32_t n_ticks, uint64_t seed) {
  if (!t || !cam_in) { fspt_set_error("fspt_render: NULL argument"); return FSPT_E_INVALID; }
  if (n_ticks == 0) return FSPT_OK;
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  fspt_camera_params cam_c = *cam_in;
  cam_c.num_bounces = clamp_bounces(cam_c.num_bounces);
  std::vector<float> rbc(n_ticks), rbt(n_ticks);
  uint64_t st0 = seed;
  for (uint32_t k = 0; k < n_ticks; ++k) { rbc[k] = fspt_rand_base_next(&st0); rbt[k] = fspt_rand_base_next(&st0); }
  return render_ticks(t, &cam_c, first_tick, n_ticks, rbc.data(), rbt.data());
}

// ---- adaptive sampling (include/fspt.h) -----------------------------------------------------------------
// Rounds of round_ticks ticks through render_ticks with the active tile list set (every pipeline traces only those
// tiles), then k_adaptive_error (E_T; the snapshot in the same pass) and, from min_ticks on, k_adaptive_select (the next
// list).  All active tiles share one tick count, so the running mean of a tile retired after n ticks is fspt_render's
// after n ticks.  One 4-byte read-back per decided round: the new list length.
static int ad_alloc(fspt_target *t, uint32_t n_tiles) {
  if (!t->ad_snap) HIP_TRY(hipMalloc((void **)&t->ad_snap, (size_t)t->W * t->H * 16));
  if (t->ad_tiles == n_tiles) return FSPT_OK;
  for (uint32_t *&b : t->ad_list) { hipFree(b); b = nullptr; }
  hipFree(t->ad_count); hipFree(t->ad_err);
  t->ad_count = nullptr; t->ad_err = nullptr; t->ad_tiles = 0;
  HIP_TRY(hipMalloc((void **)&t->ad_list[0], (size_t)n_tiles * 4));
  HIP_TRY(hipMalloc((void **)&t->ad_list[1], (size_t)n_tiles * 4));
  HIP_TRY(hipMalloc((void **)&t->ad_count, ((size_t)n_tiles + 1) * 4));
  HIP_TRY(hipMalloc((void **)&t->ad_err, (size_t)n_tiles * 8));
  t->ad_tiles = n_tiles;
  return FSPT_OK;
}

static int ad_rounds(fspt_target *t, const fspt_camera_params *cam, const fspt_adaptive_params *q, const float *rbc,
                     const float *rbt, uint32_t n_tiles, uint32_t tiles_x, uint32_t n_active) {
  const uint32_t R = q->round_ticks;
  fspt::AdaptiveP a{};
  a.accum = t->accum; a.snap = t->ad_snap; a.count = t->ad_count; a.err = t->ad_err; a.n_out = t->ad_count + n_tiles;
  a.W = t->W; a.vw = t->vw; a.vh = t->vh; a.tile = t->tile; a.tiles_x = tiles_x;
  a.min_ticks = q->min_ticks; a.max_ticks = q->max_ticks; a.target = q->target_rel_mse;
  uint32_t cur = 0, n = 0, m = 0;
  t->ad_rounds = 0;
  while (n < q->max_ticks && n_active > 0) {
    t->tile_list = t->ad_list[cur]; t->n_listed = n_active;
    int rc = render_ticks(t, cam, n, R, rbc + n, rbt + n);
    t->tile_list = nullptr; t->n_listed = 0;
    if (rc) return rc;
    n += R;
    t->ad_rounds++;
    a.list_in = t->ad_list[cur]; a.list_out = t->ad_list[cur ^ 1]; a.n_in = n_active; a.n = n;
    const bool decide = m != 0 && n >= q->min_ticks, refresh = m == 0 || n >= 2 * m;
    if (decide || refresh) {
      a.m = decide ? m : 0u; // (m = 0: the snapshot alone)
      a.refresh = refresh ? 1u : 0u;
      HIP_TRY(fspt::launch_adaptive_error(a, t->stream));
    }
    if (refresh) m = n;
    if (decide) {
      HIP_TRY(fspt::launch_adaptive_select(a, t->stream));
      HIP_TRY(hipMemcpyAsync(&n_active, a.n_out, 4, hipMemcpyDeviceToHost, t->stream));
      HIP_TRY(hipStreamSynchronize(t->stream));
      cur ^= 1;
    }
  }
  return FSPT_OK;
}

int fspt_render_adaptive(fspt_target *t, const fspt_camera_params *cam_in, const fspt_adaptive_params *q, uint64_t seed) {
  if (!t || !cam_in || !q) { fspt_set_error("fspt_render_adaptive: NULL argument"); return FSPT_E_INVALID; }
  const uint32_t R = q->round_ticks;
  if (R < 2 || R > 128) { fspt_set_error("fspt_render_adaptive: round_ticks %u not in [2, 128]", R); return FSPT_E_INVALID; }
  if (q->min_ticks % R || q->min_ticks < 2 * R) {
    fspt_set_error("fspt_render_adaptive: min_ticks %u must be a multiple of round_ticks %u, at least 2 rounds", q->min_ticks, R);
    return FSPT_E_INVALID;
  }
  if (q->max_ticks % R || q->max_ticks < q->min_ticks) {
    fspt_set_error("fspt_render_adaptive: max_ticks %u must be a multiple of round_ticks %u, at least min_ticks %u", q->max_ticks, R, q->min_ticks);
    return FSPT_E_INVALID;
  }
  if (!std::isfinite(q->target_rel_mse) || q->target_rel_mse < 0.0) {
    fspt_set_error("fspt_render_adaptive: target_rel_mse must be finite and >= 0");
    return FSPT_E_INVALID;
  }
  if (t->cam_model.model != FSPT_CAMERA_PINHOLE) {
    fspt_set_error("fspt_render_adaptive: not under camera model '%s' (tile lists through the per-tick route are a follow-up)", camera_model_name(t->cam_model.model));
    return FSPT_E_STATE;
  }
  { int rc = check_device(t->scene ? t->scene->device : 0); if (rc) return rc; }
  if (t->n_shards > 1) { fspt_set_error("fspt_render_adaptive: not on a sharded target (%u shards)", t->n_shards); return FSPT_E_STATE; }
  FLUSH_OR_RETURN(t);
  fspt_camera_params cam_c = *cam_in;
  cam_c.num_bounces = clamp_bounces(cam_c.num_bounces);
  const uint32_t tile = t->tile, tiles_x = (t->W + tile - 1) / tile, tiles_y = (t->H + tile - 1) / tile, n_tiles = tiles_x * tiles_y;
  { int rc = ad_alloc(t, n_tiles); if (rc) return rc; }
  std::vector<uint32_t> list;
  for (uint32_t g = 0; g < n_tiles; ++g)
    if ((g % tiles_x) * tile < t->vw && (g / tiles_x) * tile < t->vh) list.push_back(g);
  t->ad_valid = false;
  HIP_TRY(hipMemsetAsync(t->ad_count, 0, (size_t)n_tiles * 4, t->stream));
  HIP_TRY(hipMemsetAsync(t->ad_err, 0, (size_t)n_tiles * 8, t->stream));
  if (!list.empty()) HIP_TRY(hipMemcpyAsync(t->ad_list[0], list.data(), list.size() * 4, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipMemsetAsync(t->accum, 0, (size_t)t->W * t->H * 16, t->stream)); // (fspt_clear)
  t->acc_ticks = 0;
  std::vector<float> rbc(q->max_ticks), rbt(q->max_ticks);
  uint64_t st0 = seed;
  for (uint32_t k = 0; k < q->max_ticks; ++k) { rbc[k] = fspt_rand_base_next(&st0); rbt[k] = fspt_rand_base_next(&st0); }
  int rc = ad_rounds(t, &cam_c, q, rbc.data(), rbt.data(), n_tiles, tiles_x, (uint32_t)list.size());
  if (rc) return rc;
  t->ad_count_host.assign(n_tiles, 0u);
  t->ad_err_host.assign(n_tiles, 0.0);
  HIP_TRY(hipMemcpyAsync(t->ad_count_host.data(), t->ad_count, (size_t)n_tiles * 4, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipMemcpyAsync(t->ad_err_host.data(), t->ad_err, (size_t)n_tiles * 8, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  t->ad_samples = 0;
  for (uint32_t g = 0; g < n_tiles; ++g) {
    const uint32_t x0 = (g % tiles_x) * tile, y0 = (g / tiles_x) * tile;
    if (x0 >= t->vw || y0 >= t->vh) continue;
    t->ad_samples += (uint64_t)t->ad_count_host[g] * std::min(tile, t->vw - x0) * std::min(tile, t->vh - y0);
  }
  t->ad_vw = t->vw; t->ad_vh = t->vh; t->ad_tile = tile;
  t->ad_valid = true;
  return FSPT_OK;
}

int fspt_read_sample_counts(fspt_target *t, uint32_t *out) {
  if (!t || !out) { fspt_set_error("fspt_read_sample_counts: NULL argument"); return FSPT_E_INVALID; }
  if (!t->ad_valid) { fspt_set_error("fspt_read_sample_counts: no fspt_render_adaptive run yet"); return FSPT_E_STATE; }
  const uint32_t tile = t->ad_tile, tiles_x = (t->W + tile - 1) / tile;
  for (uint32_t y = 0; y < t->H; ++y)
    for (uint32_t x = 0; x < t->W; ++x)
      out[(size_t)y * t->W + x] = (x < t->ad_vw && y < t->ad_vh) ? t->ad_count_host[(y / tile) * tiles_x + x / tile] : 0u;
  return FSPT_OK;
}

int fspt_adaptive_last_stats(fspt_target *t, uint32_t *rounds, uint64_t *samples, double *tile_err, uint32_t *tile_ticks, uint32_t cap) {
  if (!t) { fspt_set_error("fspt_adaptive_last_stats: NULL target"); return FSPT_E_INVALID; }
  if (!t->ad_valid) { fspt_set_error("fspt_adaptive_last_stats: no fspt_render_adaptive run yet"); return FSPT_E_STATE; }
  const uint32_t n_tiles = (uint32_t)t->ad_count_host.size();
  if ((tile_err || tile_ticks) && cap < n_tiles) { fspt_set_error("fspt_adaptive_last_stats: cap %u < %u tiles", cap, n_tiles); return FSPT_E_INVALID; }
  if (rounds) *rounds = t->ad_rounds;
  if (samples) *samples = t->ad_samples;
  if (tile_err) std::memcpy(tile_err, t->ad_err_host.data(), (size_t)n_tiles * 8);
  if (tile_ticks) std::memcpy(tile_ticks, t->ad_count_host.data(), (size_t)n_tiles * 4);
  return FSPT_OK;
}

int fspt_target_set_deferred(fspt_target *t, int enable) {
  if (!t) { fspt_set_error("fspt_target_set_deferred: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  t->defer = enable != 0;
  return FSPT_OK;
}

int fspt_target_set_sampler(fspt_target *t, int sampler, uint32_t seed) {
  if (!t) { fspt_set_error("fspt_target_set_sampler: NULL target"); return FSPT_E_INVALID; }
  if (sampler != FSPT_SAMPLER_REFERENCE && sampler != FSPT_SAMPLER_SOBOL) {
    fspt_set_error("fspt_target_set_sampler: sampler must be FSPT_SAMPLER_REFERENCE (0) or FSPT_SAMPLER_SOBOL (1), got %d", sampler);
    return FSPT_E_INVALID;
  }
  FLUSH_OR_RETURN(t);
  t->sampler = sampler;
  t->sampler_seed = seed;
  return FSPT_OK;
}

int fspt_target_get_sampler(fspt_target *t, int *sampler, uint32_t *seed) {
  if (!t) { fspt_set_error("fspt_target_get_sampler: NULL target"); return FSPT_E_INVALID; }
  if (sampler) *sampler = t->sampler;
  if (seed) *seed = t->sampler_seed;
  return FSPT_OK;
}

int fspt_target_set_camera_model(fspt_target *t, const fspt_camera_model_params *p) {
  if (!t) { fspt_set_error("fspt_target_set_camera_model: NULL target"); return FSPT_E_INVALID; }
  fspt::CameraModelP m{fspt::CAM_PINHOLE, 3.14159265f, 0.064f};
  if (p) { m.model = p->model; m.angle = p->angle; m.ipd = p->ipd; }
  if (m.model < FSPT_CAMERA_PINHOLE || m.model > FSPT_CAMERA_STEREO) {
    fspt_set_error("fspt_target_set_camera_model: unknown model %d (0 pinhole, 1 ortho, 2 fisheye, 3 equirect, 4 stereo)", m.model);
    return FSPT_E_INVALID;
  }
  if (m.model == FSPT_CAMERA_FISHEYE && !(std::isfinite(m.angle) && m.angle > 0.0f && m.angle <= 6.2831855f)) {
    fspt_set_error("fspt_target_set_camera_model: fisheye angle must lie in (0, 2 pi] radians, got %g", (double)m.angle);
    return FSPT_E_INVALID;
  }
  if (m.model == FSPT_CAMERA_STEREO && !(std::isfinite(m.ipd) && m.ipd >= 0.0f)) {
    fspt_set_error("fspt_target_set_camera_model: stereo ipd must be finite and >= 0, got %g", (double)m.ipd);
    return FSPT_E_INVALID;
  }
  if (m.model == FSPT_CAMERA_STEREO && (t->H & 1u)) {
    fspt_set_error("fspt_target_set_camera_model: stereo (over-under) needs an even target height, got %u", t->H);
    return FSPT_E_INVALID;
  }
  FLUSH_OR_RETURN(t); // recorded ticks run under the old model
  // a recorded fspt_camera call stays recorded: its rays are made under the new model when somebody looks at them
  t->cam_model = m;
  return FSPT_OK;
}

int fspt_target_get_camera_model(fspt_target *t, fspt_camera_model_params *p) {
  if (!t || !p) { fspt_set_error("fspt_target_get_camera_model: NULL argument"); return FSPT_E_INVALID; }
  p->model = t->cam_model.model; p->angle = t->cam_model.angle; p->ipd = t->cam_model.ipd;
  return FSPT_OK;
}

int fspt_camera_model_time(fspt_target *t, const fspt_camera_params *cam, uint32_t reps, float *ms_per_launch) {
  if (!t || !cam || !ms_per_launch || reps == 0) { fspt_set_error("fspt_camera_model_time: NULL argument or reps == 0"); return FSPT_E_INVALID; }
  if (t->cam_model.model == FSPT_CAMERA_PINHOLE) { fspt_set_error("fspt_camera_model_time: the pinhole camera has no kernel of its own"); return FSPT_E_STATE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  const fspt::CameraP c = camera_p(*cam);
  HIP_TRY(hipEventRecord(t->ev0, t->stream));
  for (uint32_t k = 0; k < reps; ++k)
    HIP_TRY(fspt::launch_camera(t->W, t->H, t->vw, t->vh, c, t->cam_model, (float)k, t->ray_pos, t->ray_dir, t->stream,
                                (uint32_t)t->sampler, t->sampler_seed, k));
  HIP_TRY(hipEventRecord(t->ev1, t->stream));
  HIP_TRY(hipEventSynchronize(t->ev1));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, t->ev0, t->ev1));
  *ms_per_launch = ms / (float)reps;
  t->timed = false; // (ev0 / ev1 no longer bracket a render)
  ray_buffers_overwritten(t);
  return FSPT_OK;
}

int fspt_target_set_lights(fspt_target *t, int mode, float emitter_fraction) {
  if (!t) { fspt_set_error("fspt_target_set_lights: NULL target"); return FSPT_E_INVALID; }
  if (mode != FSPT_LIGHTS_OFF && mode != FSPT_LIGHTS_EMITTERS) {
    fspt_set_error("fspt_target_set_lights: mode must be FSPT_LIGHTS_OFF (0) or FSPT_LIGHTS_EMITTERS (1), got %d", mode);
    return FSPT_E_INVALID;
  }
  if (!(emitter_fraction > 0.0f && emitter_fraction <= 1.0f)) {
    fspt_set_error("fspt_target_set_lights: emitter_fraction must lie in (0, 1], got %g", (double)emitter_fraction);
    return FSPT_E_INVALID;
  }
  FLUSH_OR_RETURN(t);
  if (mode == FSPT_LIGHTS_EMITTERS) {
    const int rc = light_table_ensure(t->scene);
    if (rc) return rc;
  }
  t->lights = mode;
  t->emitter_fraction = emitter_fraction;
  return FSPT_OK;
}

int fspt_target_get_lights(fspt_target *t, int *mode, float *emitter_fraction) {
  if (!t) { fspt_set_error("fspt_target_get_lights: NULL target"); return FSPT_E_INVALID; }
  if (mode) *mode = t->lights;
  if (emitter_fraction) *emitter_fraction = t->emitter_fraction;
  return FSPT_OK;
}

int fspt_clear(fspt_target *t) {
  if (!t) { fspt_set_error("fspt_clear: NULL target"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipMemsetAsync(t->accum, 0, (size_t)t->W * t->H * 16, t->stream));
  t->acc_ticks = 0;
  return FSPT_OK;
}

int fspt_sync(fspt_target *t) {
  if (!t) { fspt_set_error("fspt_sync: NULL target"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

int fspt_read_radiance(fspt_target *t, float *out) {
  if (!t || !out) { fspt_set_error("fspt_read_radiance: NULL argument"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipMemcpyAsync(out, t->accum, (size_t)t->W * t->H * 16, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// pipelined present
// ---------------------------------------------------------------------------
} // extern "C"

// Every entry but fspt_camera / fspt_trace (recording) and fspt_present joins the pipeline through flush_pending: it
// waits for everything a present enqueued, so that its behaviour is what it was without present.
int present_join(fspt_target *t) {
  t->pr_dirty = true; // the caller may enqueue work on the target's stream: lane 1 waits for it at the next present
  if (!t->pr_active) return FSPT_OK;
  t->pr_active = false; t->pr_slot = -1; t->pr_acc_stream = nullptr;
  HIP_TRY(hipSetDevice(t->scene->device));
  if (t->pr_lane.stream) HIP_TRY(hipStreamSynchronize(t->pr_lane.stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return FSPT_OK;
}

static int present_alloc(fspt_target *t) {
  if (t->pr_acc) return FSPT_OK;
  const size_t bytes = (size_t)t->W * t->H * 4;
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(hipMalloc((void **)&t->pr_dev[k], bytes));
    HIP_TRY(hipHostMalloc((void **)&t->pr_host[k], bytes, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&t->pr_copied[k], hipEventDisableTiming));
  }
  HIP_TRY(hipEventCreateWithFlags(&t->pr_hop, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&t->pr_acc, hipEventDisableTiming)); // (last: it marks the set as complete)
  return FSPT_OK;
}

// One run of recorded ticks under present.  The batch scheduler alternates lanes; every other form runs on the target's
// stream behind the last accumulator access, in order.  Either way pr_acc / pr_acc_stream end behind the run's last write.
static int present_run(fspt_target *t, const fspt_camera_params *cam, uint32_t first_tick, uint32_t n_ticks,
                       const float *rbc, const float *rbt) {
  // (under a camera model every tick goes through the one pair of ray buffers: serially on the target's stream, below)
  if (t->pipeline == 1 && t->sched == 0 && !t->stream_fallback && t->cam_model.model == FSPT_CAMERA_PINHOLE) {
    uint32_t lane = t->pr_next;
    int rc = render_wavefront_present(t, lane, cam, first_tick, n_ticks, rbc, rbt);
    if (rc == FSPT_E_NOMEM && lane == 1) { lane = 0; rc = render_wavefront_present(t, 0, cam, first_tick, n_ticks, rbc, rbt); }
    if (rc != FSPT_E_NOMEM) {
      if (rc) return rc;
      t->pr_next = lane ^ 1u;
      t->acc_ticks = first_tick + n_ticks;
      return FSPT_OK;
    }
    // not even lane 0 fits the batch scheduler's floor: render_ticks moves the target to the stream scheduler
  }
  if (t->pr_acc_stream && t->pr_acc_stream != t->stream) HIP_TRY(hipStreamWaitEvent(t->stream, t->pr_acc, 0));
  int rc = render_ticks(t, cam, first_tick, n_ticks, rbc, rbt);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(t->pr_acc, t->stream));
  t->pr_acc_stream = t->stream;
  return FSPT_OK;
}

// The recorded ticks, in runs of one view as flush_pending forms them, the present way (no join).
static int present_flush(fspt_target *t) {
  std::vector<fspt_target::Deferred> q;
  q.swap(t->pending); // (a failing run drops the rest: the error is reported once)
  std::vector<float> rbc, rbt;
  size_t i = 0;
  while (i < q.size()) {
    size_t j = i + 1;
    while (j < q.size() && same_view(q[j].cam, q[i].cam) && q[j].tick == q[j - 1].tick + 1) ++j;
    rbc.clear(); rbt.clear();
    for (size_t k = i; k < j; ++k) { rbc.push_back(q[k].rb_cam); rbt.push_back(q[k].rb_trace); }
    int rc = present_run(t, &q[i].cam, q[i].tick, (uint32_t)(j - i), rbc.data(), rbt.data());
    if (rc) return rc;
    i = j;
  }
  return FSPT_OK;
}

extern "C" int fspt_present(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale,
                            uint8_t *out_rgba8, uint32_t *ticks_out) {
  if (!t || !out_rgba8 || !ticks_out) { fspt_set_error("fspt_present: NULL argument"); return FSPT_E_INVALID; }
  if (fspt_device_count() <= 0) { fspt_set_error("fspt_present: no HIP device available; libfspt has no CPU fallback"); return FSPT_E_NO_DEVICE; }
  if (!(scale > 0.0f && scale <= 1.0f)) { fspt_set_error("fspt_present: scale must be in (0, 1]"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  int rc = present_alloc(t);
  if (rc) return rc;
  t->pr_active = true;
  t->ev_used = 0; t->ev_overflow = false; // fspt_last_stage_ms: the batches this present enqueues
  if ((rc = present_flush(t))) return rc;
  hipStream_t ds = t->pr_acc_stream ? t->pr_acc_stream : t->stream; // (the stream of the last accumulator write)
  // this frame: k_draw behind the last accumulator write (same stream), into a device buffer of its slot, then a copy to
  // pinned memory
  const size_t n = (size_t)t->W * t->H;
  const int slot = t->pr_slot < 0 ? 0 : t->pr_slot ^ 1;
  HIP_TRY(draw_launch(t, t->accum, exposure, saturation, denoise, max_sigma, scale, t->pr_dev[slot], ds)); // (metered on ds too: DESIGN 8.11, ordering)
  HIP_TRY(hipEventRecord(t->pr_acc, ds)); // the next resolve writes the accumulator only after this draw has read it
  t->pr_acc_stream = ds;
  HIP_TRY(hipMemcpyAsync(t->pr_host[slot], t->pr_dev[slot], n * 4, hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipEventRecord(t->pr_copied[slot], ds));
  t->pr_ticks[slot] = t->acc_ticks;
  t->pr_kind[slot] = 0;
  // the previous present's frame
  const int prev = t->pr_slot;
  t->pr_slot = slot;
  *ticks_out = 0;
  if (prev >= 0) {
    HIP_TRY(hipEventSynchronize(t->pr_copied[prev]));
    if (t->pr_ticks[prev] && t->pr_kind[prev] == 0) { std::memcpy(out_rgba8, t->pr_host[prev], n * 4); *ticks_out = t->pr_ticks[prev]; } // (a file fspt_present_jpeg enqueued is dropped)
  }
  return FSPT_OK;
}

// fspt_present with the encode behind the draw, on the draw's stream: the frame stays on the device, its
// length comes to pinned memory in front of the slot's event, and the call that returns the file copies that many bytes.
// pr_acc is recorded behind the ENCODE: the next frame's resolve, and with it its draw and encode, which may run on the
// other lane's stream, start after this one has finished with the encoder's work buffers.
extern "C" int fspt_present_jpeg(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale,
                                 const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out, uint32_t *ticks_out) {
  const char *fn = "fspt_present_jpeg";
  if (!t || !out || !bytes_out || !ticks_out) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  int rc = fspt::jpeg_check_params(p, fn);
  if (rc) return rc;
  if (!(scale > 0.0f && scale <= 1.0f)) { fspt_set_error("%s: scale must be in (0, 1]", fn); return FSPT_E_INVALID; }
  if (fspt_device_count() <= 0) { fspt_set_error("%s: no HIP device available; libfspt has no CPU fallback", fn); return FSPT_E_NO_DEVICE; }
  fspt::JpegPlan pl;
  if ((rc = fspt::jpeg_plan(p, t->W, t->H, fn, pl))) return rc;
  HIP_TRY(hipSetDevice(t->scene->device));
  if ((rc = present_alloc(t))) return rc;
  for (uint32_t *&c : t->jp_count) if (!c) HIP_TRY(hipHostMalloc((void **)&c, sizeof(uint32_t), hipHostMallocDefault));
  if (!t->jp_copy) HIP_TRY(hipStreamCreateWithFlags(&t->jp_copy, hipStreamNonBlocking));
  // other parameters than the encoder's: its work buffers are made again, once the frame in flight is through with them
  if (t->pr_slot >= 0) {
    const fspt::JpegPlan &q = t->jp.pl;
    if (t->jp.c.valid && !(q.quality == pl.quality && q.sub == pl.sub && q.ri == pl.ri)) HIP_TRY(hipEventSynchronize(t->pr_copied[t->pr_slot]));
  }
  HIP_TRY(fspt::jpeg_ensure(t->jp, pl, 2, fspt::jpeg_bound_max(t->W, t->H)));
  t->pr_active = true;
  t->ev_used = 0; t->ev_overflow = false;
  if ((rc = present_flush(t))) return rc;
  hipStream_t ds = t->pr_acc_stream ? t->pr_acc_stream : t->stream;
  const int slot = t->pr_slot < 0 ? 0 : t->pr_slot ^ 1;
  HIP_TRY(draw_launch(t, t->accum, exposure, saturation, denoise, max_sigma, scale, t->pr_dev[slot], ds));
  HIP_TRY(fspt::jpeg_launch(t->jp, t->pr_dev[slot], 1, slot, ds));
  HIP_TRY(hipMemcpyAsync(t->jp_count[slot], t->jp.off + t->jp.pl.n_int, sizeof(uint32_t), hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipEventRecord(t->pr_acc, ds));
  t->pr_acc_stream = ds;
  HIP_TRY(hipEventRecord(t->pr_copied[slot], ds));
  t->pr_ticks[slot] = t->acc_ticks;
  t->pr_kind[slot] = 1;
  const int prev = t->pr_slot;
  t->pr_slot = slot;
  *ticks_out = 0; *bytes_out = 0;
  if (prev >= 0) {
    HIP_TRY(hipEventSynchronize(t->pr_copied[prev]));
    if (t->pr_ticks[prev] && t->pr_kind[prev] == 1) { // (an RGBA8 frame fspt_present enqueued is dropped)
      if ((rc = fspt::enc_deliver(t->jp.c.out[prev], *t->jp_count[prev], out, cap, bytes_out, t->jp_copy, fn, fspt::g_jpeg_format))) return rc; // (cap too small: the frame is dropped)
      *ticks_out = t->pr_ticks[prev];
    }
  }
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// what the live-scene update entries (fspt_scene_update.cpp) need of this file
// ---------------------------------------------------------------------------
// Orders a geometry call against every target of the scene, then leaves the device idle.
int geometry_order_targets(fspt_scene *s) {
  int rc = FSPT_OK;
  // every earlier call on any target of the scene sees the old geometry: run the recorded ticks (which joins a present
  // frame in flight), then wait for the device - the update's kernels run on the NULL stream and are waited for, so every
  // later call sees the new one
  // (a target under fspt_present keeps its frame in flight: its recorded ticks are enqueued the present way, without a
  // join, so the next fspt_present still returns the pre-update frame)
  for (fspt_target *t : s->targets) {
    if (t->pr_active) { t->pr_dirty = true; rc = present_flush(t); if (rc) return rc; }
    else FLUSH_OR_RETURN(t);
  }
  HIP_TRY(hipDeviceSynchronize());
  return FSPT_OK;
}

extern "C" {

int fspt_last_kernel_ms(fspt_target *t, float *ms, uint32_t *launches) {
  if (!t || !ms) { fspt_set_error("fspt_last_kernel_ms: NULL argument"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (!t->timed) { fspt_set_error("fspt_last_kernel_ms: nothing traced yet"); return FSPT_E_STATE; }
  HIP_TRY(hipSetDevice(t->scene->device));
  HIP_TRY(hipEventSynchronize(t->ev1));
  HIP_TRY(hipEventElapsedTime(ms, t->ev0, t->ev1));
  if (launches) *launches = t->last_launches;
  return FSPT_OK;
}

int fspt_target_set_viewport(fspt_target *t, uint32_t w, uint32_t h) {
  if (!t) { fspt_set_error("fspt_target_set_viewport: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (w > t->W || h > t->H) { fspt_set_error("fspt_target_set_viewport: %ux%u exceeds the target %ux%u", w, h, t->W, t->H); return FSPT_E_INVALID; }
  const uint32_t nw = w ? w : t->W, nh = h ? h : t->H;
  if (nw != t->vw || nh != t->vh) prim_reset(t);
  t->vw = nw;
  t->vh = nh;
  return FSPT_OK;
}

int fspt_target_set_pipeline(fspt_target *t, int pipeline, uint32_t batch_ticks) {
  if (!t) { fspt_set_error("fspt_target_set_pipeline: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (pipeline < 0 || pipeline > 2) { fspt_set_error("pipeline must be 0 (megakernel), 1 (wavefront, batches) or 2 (wavefront, stream)"); return FSPT_E_INVALID; }
  if (batch_ticks > (uint32_t)fspt::WF_MAX_BATCH) {
    fspt_set_error("batch_ticks must be <= %d", fspt::WF_MAX_BATCH);
    return FSPT_E_INVALID;
  }
  const int sched = pipeline == 2 ? 1 : 0;
  if (pipeline != 0 && (sched != t->sched || t->stream_fallback)) {
    // the two schedulers size the path state differently: give it back (the next render allocates what it needs)
    HIP_TRY(hipSetDevice(t->scene->device));
    wf_release(t->wf);
  }
  t->pipeline = pipeline == 0 ? 0 : 1;
  if (pipeline != 0) t->sched = sched;
  t->stream_fallback = false;
  if (batch_ticks) t->batch_ticks = batch_ticks;
  return FSPT_OK;
}

int fspt_target_set_pool(fspt_target *t, uint32_t paths, int drain_iterations, uint32_t max_iterations, int overlap) {
  if (!t) { fspt_set_error("fspt_target_set_pool: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (drain_iterations < -1 || drain_iterations > FSPT_MAX_BOUNCES + 1) { fspt_set_error("fspt_target_set_pool: drain_iterations must be -1 (default) or 0..%d", FSPT_MAX_BOUNCES + 1); return FSPT_E_INVALID; }
  t->pool_paths = paths;
  t->stream_drain = drain_iterations;
  t->stream_iter_cap = max_iterations;
  t->stream_overlap = overlap < 0 ? -1 : (overlap ? 1 : 0);
  return FSPT_OK;
}

int fspt_target_set_trace_budget(fspt_target *t, uint32_t steps) {
  if (!t) { fspt_set_error("fspt_target_set_trace_budget: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  t->susp_budget = steps;
  return FSPT_OK;
}

int fspt_logic_set_stash(int entries) {
  if (entries < -1) { fspt_set_error("fspt_logic_set_stash: entries must be -1 (the library's choice), 0 (none) or a cap"); return FSPT_E_INVALID; }
  fspt::g_logic_stash = entries;
  return FSPT_OK;
}

int fspt_target_set_primary_form(fspt_target *t, int form) {
  if (!t) { fspt_set_error("fspt_target_set_primary_form: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (form < 0 || form > 2) { fspt_set_error("fspt_target_set_primary_form: form must be 0 (measure and choose), 1 or 2"); return FSPT_E_INVALID; }
  t->primary_form = form;
  return FSPT_OK;
}

int fspt_target_get_primary_form(fspt_target *t, uint32_t batch_ticks, int *form, double ms_per_sample[2]) {
  if (!t || !form) { fspt_set_error("fspt_target_get_primary_form: NULL argument"); return FSPT_E_INVALID; }
  HIP_TRY(hipSetDevice(t->scene->device));
  prim_collect(t, true);
  double m1 = -1.0, m2 = -1.0;
  const auto it = t->prim_ms.find(batch_ticks);
  if (it != t->prim_ms.end()) { m1 = it->second.best[1]; m2 = it->second.best[2]; }
  *form = (t->primary_form == 1 || t->primary_form == 2) ? t->primary_form : (int)prim_choose(t, batch_ticks);
  if (ms_per_sample) { ms_per_sample[0] = m1; ms_per_sample[1] = m2; }
  return FSPT_OK;
}

int fspt_target_set_node_form(fspt_target *t, int primary, int trace, int tail, int64_t trace_below) {
  if (!t) { fspt_set_error("fspt_target_set_node_form: NULL target"); return FSPT_E_INVALID; }
  const int v[3] = {primary, trace, tail};
  for (int k = 0; k < 3; ++k)
    if (v[k] < -1 || v[k] > (k == 2 ? 2 : 1)) { fspt_set_error("fspt_target_set_node_form: form %d (want -1, 0, 1; the tail also 2 = adaptive)", v[k]); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  for (int k = 0; k < 3; ++k) t->node_form[k] = v[k];
  if (trace_below >= 0) t->wide_trace_below = trace_below > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)trace_below;
  prim_reset(t); // the primary-form measurements were taken with the other node form
  return FSPT_OK;
}

int fspt_target_set_stage_timing(fspt_target *t, int enable) {
  if (!t) { fspt_set_error("fspt_target_set_stage_timing: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  t->stage_events = enable != 0;
  return FSPT_OK;
}

int fspt_target_set_tail(fspt_target *t, int round) {
  if (!t) { fspt_set_error("fspt_target_set_tail: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (round < -1 || round > FSPT_MAX_BOUNCES + 1) { fspt_set_error("fspt_target_set_tail: round must be -1 (adaptive), 0 (never) or 1..%d", FSPT_MAX_BOUNCES + 1); return FSPT_E_INVALID; }
  t->tail_round = round;
  return FSPT_OK;
}

int fspt_target_live_paths(fspt_target *t, double *frac, uint32_t n_rounds) {
  if (!t || !frac) { fspt_set_error("fspt_target_live_paths: NULL argument"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  if (t->wf.counts_pending) {
    HIP_TRY(hipEventSynchronize(t->wf.counts_ready));
    wf_collect_counts(t, t->wf);
  }
  for (uint32_t r = 0; r < n_rounds; ++r) frac[r] = (t->live_known && r < 80) ? (double)t->live_frac[r] : 0.0;
  return t->live_known ? FSPT_OK : FSPT_E_STATE;
}

int fspt_target_set_memory_limit(fspt_target *t, uint64_t bytes) {
  if (!t) { fspt_set_error("fspt_target_set_memory_limit: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  if (t->stream_fallback) { HIP_TRY(hipSetDevice(t->scene->device)); wf_release(t->wf); t->stream_fallback = false; } // what fits is decided afresh
  if (t->pr_lane.bytes || t->pr_lane.susp_bytes) { HIP_TRY(hipSetDevice(t->scene->device)); wf_release_all(t->pr_lane); } // (fspt_present's second lane: made again if it fits)
  t->mem_limit = bytes;
  return FSPT_OK;
}

int fspt_target_path_state_bytes(fspt_target *t, uint64_t *bytes, uint32_t *batch_ticks) {
  if (!t || !bytes) { fspt_set_error("fspt_target_path_state_bytes: NULL argument"); return FSPT_E_INVALID; }
  uint64_t b = 0;
  b = t->wf.bytes + t->wf.susp_bytes + t->pr_lane.bytes + t->pr_lane.susp_bytes; // (fspt_present's second lane: 0 until present makes it)
  *bytes = b;
  if (batch_ticks) *batch_ticks = t->batch_ticks;
  return FSPT_OK;
}

int fspt_target_prepare(fspt_target *t) {
  if (!t) { fspt_set_error("fspt_target_prepare: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  if (t->pipeline != 1) return FSPT_OK;
  fspt::TraceP tp{};
  fill_trace_params(t, tp);
  const uint64_t work_total = (uint64_t)tp.n_owned_tiles * tp.tile * tp.tile;
  if (work_total == 0) return FSPT_OK;
  if (t->sched == 0 && !t->stream_fallback) {
    uint32_t batch;
    const int rc = wf_plan_and_ensure(t, work_total, 0, batch);
    if (rc != FSPT_E_NOMEM) return rc;
    t->stream_fallback = true; // (see render_ticks)
  }
  {
    // the pool of the configured steady state: runs of batch_ticks ticks (at most WF_MAX_BATCH per run)
    const uint32_t units_total = (uint32_t)(work_total >> 6);
    const uint32_t nbt = t->batch_ticks < (uint32_t)fspt::WF_MAX_BATCH ? (t->batch_ticks ? t->batch_ticks : 1u) : (uint32_t)fspt::WF_MAX_BATCH;
    StPlan pl;
    int rc = st_plan(t, units_total, nbt, clamp_bounces(t->last_cam.num_bounces ? t->last_cam.num_bounces : 8u), pl);
    if (rc == FSPT_OK) rc = st_ensure(t, t->wf, pl.cap, pl.ring_slots, t->mem_limit ? t->mem_limit : ~0ull);
    return rc;
  }
}

int fspt_last_stage_ms(fspt_target *t, float ms[5], uint32_t launches[5]) {
  if (!t || !ms || !launches) { fspt_set_error("fspt_last_stage_ms: NULL argument"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  HIP_TRY(hipStreamSynchronize(t->stream));
  for (int k = 0; k < fspt::WF_K_KINDS; ++k) { ms[k] = 0.0f; launches[k] = 0; }
  for (uint32_t i = 0; i < t->ev_used; ++i) {
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, t->ev_pool[2 * i], t->ev_pool[2 * i + 1]));
    int k = t->ev_kind[i];
    if (k >= 0 && k < fspt::WF_K_KINDS) { ms[k] += e; launches[k]++; }
  }
  if (t->ev_overflow) { fspt_set_error("stage timing: more than %u launches, timing truncated", EV_PAIRS); return FSPT_E_STATE; }
  return FSPT_OK;
}

int fspt_enable_counters(fspt_target *t, int enable) {
  if (!t) { fspt_set_error("fspt_enable_counters: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  t->count = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return FSPT_OK;
}

int fspt_counters_reset(fspt_target *t) {
  if (!t) { fspt_set_error("fspt_counters_reset: NULL target"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  HIP_TRY(hipMemsetAsync(t->counters, 0, 64, t->stream));
  return FSPT_OK;
}

int fspt_get_counters(fspt_target *t, fspt_counters *out) {
  if (!t || !out) { fspt_set_error("fspt_get_counters: NULL argument"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  unsigned long long v[6];
  HIP_TRY(hipMemcpyAsync(v, t->counters, 48, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  out->samples = v[0]; out->rays = v[1]; out->steps = v[2]; out->leaves = v[3]; out->shades = v[4];
  out->env_lookups = v[5];
  return FSPT_OK;
}

int fspt_get_trace_lds_steps(fspt_target *t, uint64_t *steps) {
  if (!t || !steps) { fspt_set_error("fspt_get_trace_lds_steps: NULL argument"); return FSPT_E_INVALID; }
  FLUSH_OR_RETURN(t);
  HIP_TRY(hipSetDevice(t->scene->device));
  unsigned long long v = 0;
  HIP_TRY(hipMemcpyAsync(&v, t->counters + 6, 8, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  *steps = v;
  return FSPT_OK;
}

// ---------------------------------------------------------------------------
// stand-alone intersect + math probes
// ---------------------------------------------------------------------------
int fspt_intersect(fspt_scene *s, const float *rays, uint32_t n, float *t_out, int32_t *index_out, uint32_t *steps_out,
                   uint32_t *leaves_out) {
  return fspt_intersect_form(s, 0, rays, n, t_out, index_out, steps_out, leaves_out);
}

int fspt_intersect_form(fspt_scene *s, int two_level, const float *rays, uint32_t n, float *t_out, int32_t *index_out, uint32_t *steps_out,
                        uint32_t *leaves_out) {
  if (!s || (n && (!rays || !t_out || !index_out))) { fspt_set_error("fspt_intersect: NULL argument"); return FSPT_E_INVALID; }
  if (two_level && !s->d.quads) { fspt_set_error("fspt_intersect_form: the scene has no two-level nodes (its boxes are not the unions of their children's)"); return FSPT_E_INVALID; }
  if (n == 0) return FSPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  float *d_rays = nullptr, *d_t = nullptr;
  int *d_i = nullptr;
  uint32_t *d_s = nullptr, *d_l = nullptr;
  int rc = FSPT_OK;
  hipError_t e = hipMalloc((void **)&d_rays, (size_t)n * 24);
  if (e == hipSuccess) e = hipMalloc((void **)&d_t, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&d_i, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&d_s, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&d_l, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, (size_t)n * 24, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    fspt::IntersectP p{};
    p.scene = s->d; p.rays = d_rays; p.n = n; p.t_out = d_t; p.index_out = d_i; p.steps_out = d_s; p.leaves_out = d_l;
    p.wide = two_level ? 1u : 0u;
    e = fspt::launch_intersect(p, nullptr);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(t_out, d_t, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(index_out, d_i, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && steps_out) e = hipMemcpy(steps_out, d_s, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && leaves_out) e = hipMemcpy(leaves_out, d_l, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { fspt_set_error("fspt_intersect: %s", hipGetErrorString(e)); rc = FSPT_E_HIP; }
  hipFree(d_rays); hipFree(d_t); hipFree(d_i); hipFree(d_s); hipFree(d_l);
  return rc;
}

int fspt_sampler_eval(int device, uint32_t seed, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, uint32_t n,
                      float *out) {
  if (!pixel || !sample || !dim || !out) { fspt_set_error("fspt_sampler_eval: NULL argument"); return FSPT_E_INVALID; }
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return FSPT_OK;
  const size_t bytes = (size_t)n * 4;
  // one allocation, in words: pixel | sample | dim | out (n each)
  Staging s(4 * bytes);
  if (!s.ok()) return s.done("fspt_sampler_eval");
  uint32_t *const d = (uint32_t *)s.base;
  s.up(d, pixel, bytes);
  s.up(d + n, sample, bytes);
  s.up(d + 2 * (size_t)n, dim, bytes);
  if (s.ok()) s.e = fspt::launch_sampler_eval(seed, d, d + n, d + 2 * (size_t)n, n, (float *)(d + 3 * (size_t)n), nullptr);
  s.sync();
  s.down(out, d + 3 * (size_t)n, bytes);
  return s.done("fspt_sampler_eval");
}

int fspt_math_eval(int device, int op, const float *a, const float *b, uint32_t n, float *out) {
  if (!a || !out) { fspt_set_error("fspt_math_eval: NULL argument"); return FSPT_E_INVALID; }
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return FSPT_OK;
  // one allocation, in floats: a | out | b (n each; no b: the kernel gets NULL)
  Staging s((size_t)n * 12);
  if (!s.ok()) return s.done("fspt_math_eval");
  float *const da = (float *)s.base, *const dout = da + n, *const db = b ? dout + n : nullptr;
  s.up(da, a, (size_t)n * 4);
  s.up(db, b, (size_t)n * 4);
  if (s.ok()) s.e = fspt::launch_math(op, da, db, n, dout, nullptr);
  s.sync();
  s.down(out, dout, (size_t)n * 4);
  return s.done("fspt_math_eval");
}

} // extern "C"
