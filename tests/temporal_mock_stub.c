/* temporal_mock_stub.c - fspt_temporal_* and fspt_scene_motion_* for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_temporal_cpu.py): validates like the library and records what reaches it.  The history a call returns is
 * (alpha, max_history, depth_tol, normal_cos) of the call (the defaults for NULL) in pixel 0 and the call count in pixel 1. */
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int g_calls, g_motion;
static uint32_t g_px = 3 * 2; /* the mock check's target */

int fspt_temporal_accumulate(fspt_target *t, const fspt_camera_params *cam, const fspt_temporal_params *p, float *out) {
  if (!t || !cam) return FSPT_E_INVALID;
  fspt_temporal_params q = {FSPT_TEMPORAL_ALPHA, FSPT_TEMPORAL_MAX_HISTORY, FSPT_TEMPORAL_DEPTH_TOL, FSPT_TEMPORAL_NORMAL_COS};
  if (p) q = *p;
  if (!(q.alpha >= 0.0f && q.alpha <= 1.0f) || !(q.max_history >= 1.0f) || !(q.depth_tol >= 0.0f) || !(q.normal_cos >= -1.0f && q.normal_cos <= 1.0f)) return FSPT_E_INVALID;
  ++g_calls;
  if (out) {
    memset(out, 0, (size_t)g_px * 16);
    out[0] = q.alpha; out[1] = q.max_history; out[2] = q.depth_tol; out[3] = q.normal_cos;
    out[4] = (float)g_calls; out[5] = (float)g_motion; out[6] = cam->fov_scale;
  }
  return FSPT_OK;
}
int fspt_temporal_reset(fspt_target *t) { if (!t) return FSPT_E_INVALID; g_calls = 0; return FSPT_OK; }
int fspt_temporal_denoise(fspt_target *t, const fspt_denoise_params *p, float *out) {
  if (!t) return FSPT_E_INVALID;
  if (!g_calls) return FSPT_E_STATE;
  if (out) { memset(out, 0, (size_t)g_px * 16); out[0] = p ? (float)p->iterations : -1.0f; }
  return FSPT_OK;
}
int fspt_temporal_draw(fspt_target *t, float exposure, float saturation, int denoised, uint8_t *out_rgba8) {
  if (!t || !out_rgba8) return FSPT_E_INVALID;
  if (!g_calls) return FSPT_E_STATE;
  memset(out_rgba8, 0, (size_t)g_px * 4);
  out_rgba8[0] = (uint8_t)(exposure * 10.0f); out_rgba8[1] = (uint8_t)(saturation * 10.0f); out_rgba8[2] = (uint8_t)denoised;
  return FSPT_OK;
}
int fspt_scene_motion_begin(fspt_scene *s) { if (!s) return FSPT_E_INVALID; ++g_motion; return FSPT_OK; }
int fspt_scene_motion_end(fspt_scene *s) { if (!s) return FSPT_E_INVALID; g_motion = 0; return FSPT_OK; }
